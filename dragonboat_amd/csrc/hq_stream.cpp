// hq_stream.cpp — the compact event stream from hq_event rows (include/hipquorum.h "event
// streams"; the codec is hq_stream_k.h): the encoder a producer holding rows can call (the wire
// decoder and a caller's own producer can write the stream directly), the decoder the host
// worker uses for stream input, and the rows as 16-byte records. The encoder from those records
// is hq_stream16.cpp. None of these entries allocates today; each runs in hq::guard all the same,
// so that no change to the codec can send an exception across the ABI, and answers with the code
// alone (no handle to keep a message in).
#include <cstring>

#include "../../include/hipquorum.h"
#include "hq_guard.h"
#include "hq_stream.h"
#include "hq_stream_k.h"

namespace hqs {
namespace {
// one group's rows ev[e0 .. e1) at p, in units (a run of repeats, or one row); false when fewer
// than HQ_EVENT_STREAM_MAX bytes are left before a unit, or there is no output at all (p NULL):
// so only when a row exists
template <class Ev>
__attribute__((always_inline)) inline bool encode_rows(uint8_t *&p, const uint8_t *end, const Ev *ev, uint64_t e0, uint64_t e1) {
    if (!p) return e0 >= e1;
    Prev pv;
    for (uint64_t e = e0; e < e1;) {
        if ((uint64_t)(end - p) < HQ_EVENT_STREAM_MAX) return false;
        e = encode_unit(p, ev, e, e1, pv);
    }
    return true;
}

// One event of a group's bytes at p (pv, run_left: the group's decoder state, as the encoder
// left it); false when the bytes do not hold a whole event
bool decode_one(const uint8_t *&p, const uint8_t *end, Prev &pv, uint64_t &run_left, hq_event &v) {
    std::memset(&v, 0, sizeof v);
    if (p >= end && !run_left) return false;
    const uint8_t h = run_left ? (uint8_t)0 : *p;
    if (run_left || ((h & 7) == HQ_EV_MESSAGE && ((h >> 3) & 7) == kCodeRun)) {
        // a run member: the group's previous message with another sender
        if (!run_left) {
            ++p;
            if (!pv.last || !get(p, end, run_left) || run_left == 0) return false;
            pv.run_seq = (h & 0x80) != 0;
            if (pv.run_seq) {          // the consecutive form: the first sender, the rest follow
                uint64_t f0;
                // (the encoder's bound, without the sum: neither operand may wrap it)
                if (!get(p, end, f0) || run_left > 0xFFFFFFFFull ||
                    f0 > 0xFFFFFFFFull - run_left)
                    return false;
                pv.run_from = (uint32_t)f0;
            }
        }
        --run_left;
        v.kind = HQ_EV_MESSAGE;
        v.type = pv.last == 1 ? HQ_MSG_REPLICATE_RESP : HQ_MSG_HEARTBEAT_RESP;
        v.reject = pv.last_reject;
        v.term = pv.term;
        if (pv.last == 1) {
            v.log_index = pv.index;
        } else {
            v.hint = pv.hint;
            v.hint_high = pv.high;
        }
        if (pv.run_seq) {
            v.from = pv.run_from++;
            return true;
        }
        return get(p, end, v.from);
    }
    ++p;
    v.kind = h & 7;
    bool ok = true;
    if (v.kind == HQ_EV_READ) {
        ok = get(p, end, v.hint) && get(p, end, v.hint_high);
    } else if (v.kind == HQ_EV_PROPOSE) {
        ok = get(p, end, v.log_index);
    } else if (v.kind == HQ_EV_MESSAGE) {
        const uint32_t code = (h >> 3) & 7;
        uint64_t t = code_type(code);
        if (code == 7) ok = get(p, end, t);
        if (code == 4) ok = pv.have_index;  // repeats an index the group has not sent
        v.type = (uint32_t)t;
        v.reject = (h >> 6) & 1;
        ok = ok && get(p, end, v.from);
        if (ok && !(h & 0x80)) ok = get(p, end, pv.term);
        v.term = pv.term;
        if (ok && (code == 0 || code == 7)) ok = get(p, end, v.log_index);
        if (code == 4) v.log_index = pv.index;
        if (ok && (code == 2 || code == 3 || code == 7))
            ok = get(p, end, v.hint) && get(p, end, v.hint_high);
        if (code == 5) {
            v.hint = pv.hint;
            v.hint_high = pv.high;
        }
        if (ok && (code == 0 || code == 4)) {
            pv.index = v.log_index;
            pv.have_index = true;
        }
        if (ok && (code == 2 || code == 5)) {
            pv.hint = v.hint;
            pv.high = v.hint_high;
        }
        pv.last = last_of(code);
        pv.last_reject = (uint8_t)v.reject;
    }
    return ok;
}
}  // namespace
uint8_t *encode_group(uint8_t *p, const uint8_t *end, const hq_event *ev, uint64_t n) {
    return encode_rows(p, end, ev, 0, n) ? p : nullptr;
}
uint8_t *encode_group(uint8_t *p, const uint8_t *end, const WireEvent *ev, uint64_t n) {
    return encode_rows(p, end, ev, 0, n) ? p : nullptr;
}
}  // namespace hqs

using namespace hqs;

extern "C" {

int hq_events_encode(uint64_t n_groups, const uint64_t *offsets, const hq_event *events,
                     uint8_t *out, uint64_t cap, uint64_t *boffsets) {
    if (!offsets || !boffsets || (n_groups && offsets[n_groups] > offsets[0] && !events))
        return HQ_E_INVAL;
    return hq::guard("hq_events_encode", [&] {
        uint8_t *p = out, *const end = out ? out + cap : nullptr;
        boffsets[0] = 0;
        for (uint64_t i = 0; i < n_groups; ++i) {
            if (!encode_rows(p, end, events, offsets[i], offsets[i + 1])) return HQ_E_STATE;
            boffsets[i + 1] = (uint64_t)(p - out);
        }
        return HQ_OK;
    });
}

int hq_events_encode_sized(uint64_t n_groups, const uint64_t *offsets, const hq_event *events,
                           uint8_t *out, uint64_t cap, uint32_t *sizes, uint64_t *n_bytes) {
    if (!offsets || !sizes || !n_bytes || (n_groups && offsets[n_groups] > offsets[0] && !events))
        return HQ_E_INVAL;
    return hq::guard("hq_events_encode_sized", [&] {
        uint8_t *p = out, *const end = out ? out + cap : nullptr;
        for (uint64_t i = 0; i < n_groups; ++i) {
            if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 0xFFFF)
                return HQ_E_INVAL;
            uint8_t *const g0 = p;
            if (!encode_rows(p, end, events, offsets[i], offsets[i + 1])) return HQ_E_STATE;
            if (p - g0 > 0xFFFF) return HQ_E_INVAL;
            sizes[i] = (uint32_t)(offsets[i + 1] - offsets[i]) | (uint32_t)(p - g0) << 16;
        }
        *n_bytes = (uint64_t)(p - out);
        return HQ_OK;
    });
}

int hq_events_decode(uint64_t n_groups, const uint64_t *offsets, const uint64_t *boffsets,
                     const uint8_t *bytes, hq_event *events) {
    if (!offsets || !boffsets || !events) return HQ_E_INVAL;
    return hq::guard("hq_events_decode", [&] {
        for (uint64_t i = 0; i < n_groups; ++i) {
            const uint8_t *p = bytes + boffsets[i], *const end = bytes + boffsets[i + 1];
            Prev pv;
            uint64_t run_left = 0;          // events still to come in the current run
            for (uint64_t e = offsets[i]; e < offsets[i + 1]; ++e)
                if (!decode_one(p, end, pv, run_left, events[e])) return HQ_E_INVAL;
            if (p != end || run_left) return HQ_E_INVAL;
        }
        return HQ_OK;
    });
}

int hq_events_count(uint64_t n_groups, const uint64_t *boffsets, const uint8_t *bytes,
                    uint64_t *offsets) {
    if (!boffsets || !offsets || (n_groups && boffsets[n_groups] > boffsets[0] && !bytes))
        return HQ_E_INVAL;
    return hq::guard("hq_events_count", [&] {
        offsets[0] = 0;
        for (uint64_t i = 0; i < n_groups; ++i) {
            if (boffsets[i + 1] < boffsets[i]) return HQ_E_INVAL;
            const uint8_t *p = bytes + boffsets[i], *const end = bytes + boffsets[i + 1];
            Prev pv;
            uint64_t run_left = 0, n = 0;
            hq_event v;
            while (p < end || run_left) {
                if (!decode_one(p, end, pv, run_left, v)) return HQ_E_INVAL;
                ++n;
            }
            offsets[i + 1] = offsets[i] + n;
        }
        return HQ_OK;
    });
}

int hq_events_to16(uint64_t n_groups, const uint64_t *offsets, const hq_event *events,
                   hq_event16 *out, uint64_t cap, uint64_t *offsets16) {
    if (!offsets || !offsets16 || (n_groups && offsets[n_groups] > offsets[0] && !events))
        return HQ_E_INVAL;
    return hq::guard("hq_events_to16", [&] {
        uint64_t k = 0;
        offsets16[0] = 0;
        for (uint64_t i = 0; i < n_groups; ++i) {
            if (offsets[i + 1] < offsets[i]) return HQ_E_INVAL;
            uint64_t ctx[2] = {0, 0};
            for (uint64_t j = offsets[i]; j < offsets[i + 1]; ++j) {
                const hq_event &e = events[j];
                hq_event16 r{};
                bool fits = e.kind >= 1 && e.kind <= 5 && e.reject <= 1;
                r.kind = (uint8_t)(e.kind | (e.reject ? 8u : 0u));
                if (fits && e.kind == HQ_EV_READ) {
                    fits = e.hint_high >> 32 == 0;
                    r.value = e.hint;
                    r.term = (uint32_t)e.hint_high;
                } else if (fits && e.kind == HQ_EV_PROPOSE) {
                    r.value = e.log_index;
                } else if (fits && e.kind == HQ_EV_MESSAGE) {
                    fits = e.type < 256 && e.from >> 16 == 0 && e.term >> 32 == 0;
                    r.type = (uint8_t)e.type;
                    r.from = (uint16_t)e.from;
                    r.term = (uint32_t)e.term;
                    if (e.type == HQ_MSG_HEARTBEAT_RESP || e.type == HQ_MSG_READ_INDEX) {
                        if (e.hint == ctx[0] && e.hint_high == ctx[1] && (e.hint | e.hint_high)) {
                            r.kind |= HQ_EV16_READ_CTX;
                        } else {
                            fits = fits && e.hint_high == 0;
                            r.value = e.hint;
                        }
                    } else if (e.type == HQ_MSG_REPLICATE_RESP ||
                               e.type == HQ_MSG_REQUEST_VOTE_RESP) {
                        r.value = e.log_index;   // (a RequestVoteResp carries nothing more)
                    } else {                     // another type: log_index, hint, hint_high
                        fits = fits && e.hint == 0 && e.hint_high == 0;
                        r.value = e.log_index;
                    }
                }
                if (fits) {
                    if (k + 1 > cap) return HQ_E_STATE;
                    out[k++] = r;
                } else {
                    if (k + 5 > cap) return HQ_E_STATE;
                    out[k] = hq_event16{};
                    out[k].kind = (uint8_t)HQ_EV16_FULL;
                    std::memset(out + k + 1, 0, 4 * sizeof(hq_event16));
                    std::memcpy(out + k + 1, &e, sizeof e);
                    k += 5;
                }
                if (e.kind == HQ_EV_READ) {
                    ctx[0] = e.hint;
                    ctx[1] = e.hint_high;
                }
            }
            offsets16[i + 1] = k;
        }
        return HQ_OK;
    });
}

}  // extern "C"
