// hq_wire.cpp — the step worker's input from the wire: raftpb.MessageBatch bytes decoded into
// hq_event rows (include/hipquorum.h "wire decode").
//
// The reference path is TCPTransport.serveConn -> Transport.handleRequest
// (internal/transport/transport.go:289-316: deployment id and binary version checks) ->
// messageHandler.HandleMessageBatch (nodehost.go:2021-2061: SnapshotReceived handled aside, a
// message for a cluster this host does not run dropped, the rest queued per cluster) ->
// node.handleReceivedMessages (node.go:1257-1287) draining the queue into Peer.Handle in arrival
// order, inside node.handleEvents' order (node.go:1113-1157: the local ReadIndex first, then the
// received messages, then the ticks, then the proposals). The bytes are the protobuf encoding of
// raftpb/raft.proto:154-168 (Message) and :191-196 (MessageBatch) as raft.pb.go marshals them
// (Message.MarshalTo raft.pb.go:2232-2300, MessageBatch.MarshalTo :2417-2445); the decoder
// accepts any valid proto2 encoding of them (fields in any order, unknown fields skipped, as
// Message.Unmarshal raft.pb.go:4831 / raft_optimized.go:654 do).
//
// No exception leaves an entry. Every int-returning entry with a wire runs its body in `guarded`
// (hq_guard.h: HQ_E_INVAL for no wire, an exception's code with "<entry>: out of memory" and the
// like in hq_wire_last_error), those that reach hq_wire_dev.hip through hq_wire_dev_* included: an
// exception from there is caught here. hq_wire_decode_batch and hq_wire_encode_batch have no
// handle and answer with the code alone. hq_wire_open allocates with new (std::nothrow);
// hq_wire_close and hq_wire_last_error return no code and allocate nothing: the three stay bare.
// What a caught exception leaves behind is said at each entry.
#include <algorithm>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/hipquorum.h"
#include "hq_dstep.h"
#include "hq_guard.h"
#include "hq_stream.h"
#include "hq_wire_codec.h"
#include "hq_wire_dev.h"

namespace {

using hqw::kSnapshotReceived;

// why hqw::decode_message rejected a message, in words
std::string message_error(const hqw::error &e) {
    switch (e.code) {
    case hqw::kVarintEnd: return "Message: unexpected end of data in a varint";
    case hqw::kVarintOverflow: return "Message: varint overflows 64 bits";
    case hqw::kFieldZero: return "Message: illegal field number 0";
    case hqw::kWrongType:
        return "Message: wrong wire type " + std::to_string(e.wt) + " for field " +
               std::to_string(e.field);
    case hqw::kGroup: return "Message: unsupported wire type (groups are not part of raft.proto)";
    case hqw::kFieldEnd: return "Message: unexpected end of data in a field";
    case hqw::kBytesEnd: return "Message: unexpected end of data in a length-delimited field";
    }
    return std::string();
}

// one event of the step as the wire keeps it (hq_stream.h): a decoded message's fields, or a
// local event's
using Rec = hqs::WireEvent;

// A Message in the field order raft.pb.go Message.MarshalTo writes (:2232-2296): every field of
// 1-10 with its tag in order, entries (11) repeated, the snapshot (12, always: nullable=false),
// hint_high (13), nothing else. false: not that layout (the general decoder takes it from the
// start, any field order); *entries counts field 11
inline bool decode_marshal_order(const uint8_t *b, size_t end, Rec &r, uint64_t &cluster,
                                 uint32_t &entries) {
    size_t p = 0;
    uint64_t v[10];
    // fields 1-10: tag (f + 1) << 3, a varint — unrolled, so that each field's tag is a constant
    // and each field's varint length has a branch of its own to predict (the lengths differ by
    // field and repeat from message to message)
#pragma GCC unroll 10
    for (uint32_t f = 0; f < 10; ++f) {
        if (p >= end || b[p] != (uint8_t)((f + 1) << 3)) return false;
        if (++p >= end || !hqw::varint(b, p, end, v[f])) return false;
    }
    entries = 0;
    while (p < end && b[p] == 0x5a) {              // entries: counted, not decoded
        uint64_t n;
        if (++p >= end || !hqw::varint(b, p, end, n) || (uint64_t)(end - p) < n) return false;
        p += n;
        ++entries;
    }
    uint64_t n, high;
    if (p >= end || b[p] != 0x62) return false;    // the snapshot
    if (++p >= end || !hqw::varint(b, p, end, n) || (uint64_t)(end - p) < n) return false;
    p += n;
    if (p >= end || b[p] != 0x68) return false;    // hint_high, the last field
    if (++p >= end || !hqw::varint(b, p, end, high) || p != end) return false;
    r.kind = HQ_EV_MESSAGE;
    r.type = (uint32_t)v[0];
    r.from = v[2];
    cluster = v[3];
    r.term = v[4];
    r.log_index = v[6];
    r.reject = v[8] != 0;
    r.hint = v[9];
    r.hint_high = high;
    return true;
}

// cluster id -> index in order of first appearance: open addressing, linear probing (a step
// looks every message's cluster up once; a node-based map costs more than the decode)
class ClusterIndex {
  public:
    void clear() {
        for (uint32_t i : used_) slots_[i].key = kEmpty;
        used_.clear();
        has_empty_ = false;
    }
    // the value of id, or false
    bool find(uint64_t id, uint32_t *v) const {
        return hqw::find(slots_.data(), slots_.size(), has_empty_, empty_val_, id, *v);
    }
    void prefetch(uint64_t id) const {
        if (!slots_.empty()) __builtin_prefetch(&slots_[hash(id) & (slots_.size() - 1)]);
    }
    size_t size() const { return used_.size() + has_empty_; }
    // The ids added since `mark()` leave again, last first: with linear probing the table is then
    // slot for slot what it was (no earlier id's probe passed the slot of a later one; a rehash
    // keeps the order of insertion), but for its capacity.
    struct Mark {
        size_t used;
        bool has_empty;
    };
    Mark mark() const { return Mark{used_.size(), has_empty_}; }
    void rollback(Mark m) {
        for (; used_.size() > m.used; used_.pop_back()) slots_[used_.back()].key = kEmpty;
        has_empty_ = m.has_empty;
    }
    // the index of id, inserting next if new (*fresh = true)
    uint32_t find_or_add(uint64_t id, uint32_t next, bool *fresh) {
        if ((used_.size() + 1) * 2 > slots_.size()) rehash(slots_.empty() ? 1024 : slots_.size() * 2);
        const uint64_t mask = slots_.size() - 1;
        for (uint64_t i = hash(id) & mask;; i = (i + 1) & mask) {
            if (slots_[i].key == id && id != kEmpty) {
                *fresh = false;
                return slots_[i].val;
            }
            if (slots_[i].key == kEmpty) {
                if (id == kEmpty) {                   // the one key the table cannot hold
                    if (!has_empty_) {
                        has_empty_ = true;
                        empty_val_ = next;
                        *fresh = true;
                        return next;
                    }
                    *fresh = false;
                    return empty_val_;
                }
                used_.push_back((uint32_t)i);     // (first: when it throws, the slot is still empty)
                slots_[i].key = id;
                slots_[i].val = next;
                *fresh = true;
                return next;
            }
        }
    }
  private:
    using Slot = hqw::Slot;
    static constexpr uint64_t kEmpty = hqw::kEmptyKey;
    static uint64_t hash(uint64_t x) { return hqw::hash_id(x); }
    void rehash(size_t cap) {
        std::vector<Slot> k(cap, Slot{kEmpty, 0, 0});
        std::vector<uint32_t> u;
        u.reserve(used_.size());
        for (uint32_t i : used_) {
            const uint64_t id = slots_[i].key;
            uint64_t j = hash(id) & (cap - 1);
            while (k[j].key != kEmpty) j = (j + 1) & (cap - 1);
            k[j] = slots_[i];
            u.push_back((uint32_t)j);
        }
        slots_.swap(k);
        used_.swap(u);
    }
    std::vector<Slot> slots_;
    std::vector<uint32_t> used_;
    bool has_empty_ = false;
    uint32_t empty_val_ = 0;
};

}  // namespace

// The worker's lifecycle epoch (hq_dstep.h). The reference is weak: the wire also builds without
// the worker's group store (a stand-alone check of this file over a stub worker), where no group
// is ever stopped and the epoch stands at 0.
uint64_t hq_worker_epoch(hq_worker *w) __attribute__((weak));
static uint64_t epoch_of(hq_worker *w) { return w && hq_worker_epoch ? hq_worker_epoch(w) : 0; }

struct hq_wire {
    uint64_t deployment_id = 0;
    std::string err;
    std::vector<Rec> recs;
    std::vector<uint64_t> clusters;
    ClusterIndex cluster_index;
    // attached (hq_wire_attach): a record's key is the worker's handle, resolved as it is
    // decoded through handle_of (cluster id -> handle, kept across steps; only clusters the
    // worker runs are kept in it). Handles change only when groups are started or stopped
    // (hq_worker_start_groups / _stop_groups): the worker's epoch then moves, and hq_wire_reset
    // drops the cache
    hq_worker *worker = nullptr;
    ClusterIndex handle_of;
    uint64_t worker_epoch = 0;         // the worker's epoch handle_of was filled under
    std::vector<uint64_t> pending;     // the cluster ids of a batch's records, before their keys
    hq_wire_stats stats{};
    // the assembled step input (valid until the next reset)
    std::vector<uint32_t> groups;
    std::vector<uint64_t> offsets;
    std::vector<hq_event> events;
    std::vector<uint64_t> boffsets;    // hq_wire_step_stream
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> cnt, perm, pos;   // the steps' counting sort (scatter)
    std::vector<uint32_t> handle;      // hq_wire_step_input: each cluster's handle
    std::vector<uint32_t> kcnt;        // attached: the records queued per handle (at h + 1)
    // the device mode (hq_wire_attach_device): batches are framed here and queued there; recs
    // holds the local events only
    hq_wire_dev *dev = nullptr;
    std::vector<hq_wire_span> spans;   // one batch's spans
    uint32_t batch_calls = 0;          // hq_wire_add_batch calls since the last reset
    const uint32_t *rejected = nullptr;   // the last device step's malformed batches
    uint64_t n_rejected = 0;
    uint64_t dev_queued = 0;           // messages queued on the device side

    void count_key(uint32_t k, uint32_t m = 1) {
        if ((size_t)k + 2 > kcnt.size()) kcnt.resize(std::max<size_t>((size_t)k + 2, 2 * kcnt.size()), 0);
        kcnt[(size_t)k + 1] += m;
    }
    static constexpr uint32_t kNoKey = UINT32_MAX;   // a record of a cluster the worker does not run
    std::vector<Rec> grp;              // hq_wire_step_sized: one group's events

    // hq_wire_add_batch and hq_wire_add_locals are all or nothing: unless `keep` is set, leaving
    // the scope (an exception, a refusal) puts recs, kcnt, clusters, cluster_index and stats back
    // to what they were when the entry began. Cluster ids newly cached in handle_of stay: a cache
    // of facts that hold until the worker's epoch moves. Nothing in it allocates.
    struct Undo {
        hq_wire &w;
        const size_t r0, c0;
        const ClusterIndex::Mark i0;
        const hq_wire_stats s0;
        size_t counted = 0;            // attached: kcnt holds the keys of recs[r0 .. r0 + counted)
        bool keep = false;
        explicit Undo(hq_wire &x)
            : w(x), r0(x.recs.size()), c0(x.clusters.size()), i0(x.cluster_index.mark()), s0(x.stats) {}
        // the records since r0 leave the queue (also: a batch dropped after its decode); kept
        // out of line, so that the entries' hot loops are what they were without it
        __attribute__((noinline)) void drop() {
            for (size_t i = r0; i < r0 + counted; ++i)
                if (w.recs[i].key != kNoKey) w.kcnt[(size_t)w.recs[i].key + 1]--;
            counted = 0;
            w.recs.resize(r0);
            w.clusters.resize(c0);
            w.cluster_index.rollback(i0);
        }
        ~Undo() {
            if (keep) return;
            drop();
            w.stats = s0;
        }
    };
    // an entry that needs an empty queue
    int need_empty(const char *entry) {
        if (recs.empty() && !dev_queued) return HQ_OK;
        return fail(HQ_E_STATE, std::string(entry) + ": events queued (reset first)");
    }
    // The tail of both attaches: the wire feeds `wk` from now on, through `d` in the device mode.
    // Everything that can throw or refuse comes before it: this only switches (a fresh handle
    // table and an emptied kcnt allocate nothing).
    void attach_to(hq_worker *wk, hq_wire_dev *d) noexcept {
        if (dev) hq_wire_dev_close(dev);
        dev = d;
        rejected = nullptr;
        n_rejected = 0;
        worker = wk;
        handle_of = ClusterIndex();
        worker_epoch = epoch_of(wk);
        kcnt.clear();
    }
    // attached: groups were started or stopped since the cache was filled, so a cluster may have
    // left its handle or come back in another one
    void follow_worker() noexcept {
        const uint64_t now = epoch_of(worker);
        if (now == worker_epoch) return;
        handle_of = ClusterIndex();
        worker_epoch = now;
    }
    // The counts in cnt (key k's at k + 1) made offsets, and the queue scattered by them into
    // perm: key k's records are perm[cnt[k] .. cnt[k + 1]), stable in arrival order. false (and
    // nothing scattered) when the counts are not the queue's.
    template <class KeyOf>
    bool scatter(KeyOf key_of) {
        const uint32_t nr = (uint32_t)recs.size();
        for (size_t i = 1; i < cnt.size(); ++i) cnt[i] += cnt[i - 1];
        if (cnt.back() != nr) return false;
        perm.resize(nr);
        pos.assign(cnt.begin(), cnt.end() - 1);
        for (uint32_t i = 0; i < nr; ++i) perm[pos[key_of(recs[i])]++] = i;
        return true;
    }

    int fail(int code, const std::string &m) {
        err = m;
        return code;
    }
    uint32_t cluster(uint64_t id) {
        bool fresh;
        const uint32_t k = cluster_index.find_or_add(id, (uint32_t)clusters.size(), &fresh);
        if (fresh) clusters.push_back(id);
        return k;
    }
    // the key of a cluster: its handle when attached (false: the worker does not run it), else
    // its index of first appearance
    bool key(uint64_t id, uint32_t *k) {
        if (!worker) {
            *k = cluster(id);
            return true;
        }
        if (handle_of.find(id, k)) return true;
        uint32_t h;
        if (hq_worker_find(worker, id, &h) != HQ_OK) return false;
        bool fresh;
        handle_of.find_or_add(id, h, &fresh);
        *k = h;
        return true;
    }
    // the records from r0 on got their cluster ids in `pending`: their keys, dropping (in place)
    // those of clusters the attached worker does not run; the handle table prefetched 8 ahead
    void resolve(size_t r0) {
        const size_t n = recs.size() - r0;
        size_t i = 0;
        for (; i < n; ++i) {                   // (no record dropped: keys set in place)
            if (worker && i + 8 < n) handle_of.prefetch(pending[i + 8]);
            if (!key(pending[i], &recs[r0 + i].key)) break;
        }
        if (i == n) return;
        size_t o = r0 + i;
        for (; i < n; ++i) {
            if (worker && i + 8 < n) handle_of.prefetch(pending[i + 8]);
            uint32_t k;
            if (!key(pending[i], &k)) {
                stats.dropped_no_cluster++;
                continue;
            }
            recs[o] = recs[r0 + i];
            recs[o++].key = k;
        }
        recs.resize(o);
    }
};

namespace {

// A C entry of the wire: HQ_E_INVAL for no wire, else the body's code, or an exception's
// (hq_guard.h) with its message in hq_wire_last_error.
struct KeepError {                     // (a type of its own: one guard_report for all entries)
    hq_wire *w;
    void operator()(int code, const std::string &m) const { w->fail(code, m); }
};
template <class Body>
int guarded(hq_wire *w, const char *entry, Body &&body) {
    if (!w) return HQ_E_INVAL;
    return hq::guard(entry, KeepError{w}, body);
}

}  // namespace

extern "C" {

int hq_wire_decode_batch(const uint8_t *bytes, size_t len, hq_wire_message *out, uint64_t cap,
                         uint64_t *count, hq_wire_batch_info *info) {
    if ((!bytes && len) || !count) return HQ_E_INVAL;
    return hq::guard("hq_wire_decode_batch", [&] {
        hq_wire_batch_info bi;
        const int rc = hqw::walk_batch(
            bytes, len, bi,
            [&](size_t, size_t body, size_t n) {
                hq_wire_message tmp;
                hqw::error e;
                hq_wire_message &dst = out && bi.n_messages < cap ? out[bi.n_messages] : tmp;
                return hqw::decode_message(bytes + body, n, dst, e) ? HQ_OK : HQ_E_INVAL;
            },
            [] {});
        *count = bi.n_messages;
        if (rc) return rc;
        if (info) *info = bi;
        return *count > cap && out ? HQ_E_STATE : HQ_OK;
    });
}

// The sending node's side (bench and tests): MessageBatch.MarshalTo (raft.pb.go:2417-2445) over
// Message.MarshalTo (:2232-2296) of the fields hq_wire_message carries, every nullable=false
// field written, the empty Snapshot's 24 bytes (Snapshot.MarshalTo :2142, Membership :2019)
int hq_wire_encode_batch(const hq_wire_message *msgs, uint64_t n, uint64_t deployment_id,
                         const uint8_t *source, size_t source_len, uint8_t *out, uint64_t cap,
                         uint64_t *len) {
    if ((n && !msgs) || !len || (source_len && !source) || (cap && !out)) return HQ_E_INVAL;
    return hq::guard("hq_wire_encode_batch", [&] {
        uint8_t *p = out, *const end = out + cap;
        for (uint64_t i = 0; i < n; ++i) {
            const hq_wire_message &m = msgs[i];
            if (m.n_entries) return HQ_E_INVAL;      // (entries are not marshalled here)
            const uint64_t reject = m.ev.reject ? 1u : 0u;
            const uint64_t size = hqw::body_size(m.ev.type, m.to, m.ev.from, m.cluster_id, m.ev.term,
                                                 m.log_term, m.ev.log_index, m.commit, reject,
                                                 m.ev.hint, m.ev.hint_high);
            if ((uint64_t)(end - p) < size + 1 + hqw::vlen(size)) return HQ_E_STATE;
            p = hqw::put_field(p, 0x0a, size);        // requests (1), length-delimited
            p = hqw::put_body(p, m.ev.type, m.to, m.ev.from, m.cluster_id, m.ev.term, m.log_term,
                              m.ev.log_index, m.commit, reject, m.ev.hint, m.ev.hint_high);
        }
        if ((uint64_t)(end - p) < 1 + 10 + 1 + 10 + source_len + 1 + 10) return HQ_E_STATE;
        p = hqw::put_trailer(p, deployment_id, source, source_len);
        *len = (uint64_t)(p - out);
        return HQ_OK;
    });
}

int hq_wire_open(uint64_t deployment_id, hq_wire **out) {
    if (!out) return HQ_E_INVAL;
    *out = new (std::nothrow) hq_wire();
    if (!*out) return HQ_E_NOMEM;
    (*out)->deployment_id = deployment_id;
    return HQ_OK;
}

void hq_wire_close(hq_wire *w) {
    if (w && w->dev) hq_wire_dev_close(w->dev);
    delete w;
}

const char *hq_wire_last_error(const hq_wire *w) { return w ? w->err.c_str() : ""; }

// hq_wire_attach, hq_wire_attach_device: after an exception (or a refusal) the wire is attached
// as it was: everything that can throw comes before the first field is switched (attach_to).
int hq_wire_attach(hq_wire *w, hq_worker *worker) {
    return guarded(w, "hq_wire_attach", [&] {
        if (const int rc = w->need_empty("hq_wire_attach")) return rc;
        w->attach_to(worker, nullptr);             // (back from the device mode, if in it)
        return HQ_OK;
    });
}

int hq_wire_attach_device(hq_wire *w, hq_worker *worker) {
    return guarded(w, "hq_wire_attach_device", [&] {
        if (!worker) return w->fail(HQ_E_INVAL, "hq_wire_attach_device: NULL worker");
        if (const int rc = w->need_empty("hq_wire_attach_device")) return rc;
        hq_wire_dev *dev = nullptr;
        const int rc = hq_wire_dev_open(worker, &dev);
        if (rc)
            return w->fail(rc, rc == HQ_E_INVAL ? "hq_wire_attach_device: not a device worker "
                                                  "(HQ_WORKER_ON_DEVICE)"
                                                : "hq_wire_attach_device: device buffers");
        w->attach_to(worker, dev);
        return HQ_OK;
    });
}

int hq_wire_reset(hq_wire *w) {
    return guarded(w, "hq_wire_reset", [&] {
        if (w->dev) hq_wire_dev_reset(w->dev);
        w->follow_worker();
        w->batch_calls = 0;
        w->dev_queued = 0;
        w->rejected = nullptr;
        w->n_rejected = 0;
        w->recs.clear();
        std::fill(w->kcnt.begin(), w->kcnt.end(), 0u);
        w->clusters.clear();
        w->cluster_index.clear();
        w->stats = hq_wire_stats{};
        return HQ_OK;
    });
}

int hq_wire_add_local(hq_wire *w, uint64_t cluster_id, const hq_event *events, uint64_t count) {
    return guarded(w, "hq_wire_add_local", [&] {
        if (count && !events) return HQ_E_INVAL;
        const uint64_t off[2] = {0, count};
        return hq_wire_add_locals(w, 1, &cluster_id, off, events);
    });
}

// All or nothing: after an exception the queue, the per-handle counts, the clusters seen and the
// stats are as before the call (hq_wire::Undo).
static int add_locals(hq_wire *w, uint64_t n, const uint64_t *cluster_ids, const uint64_t *offsets,
                      const hq_event *events) {
    if (n && (!cluster_ids || !offsets)) return HQ_E_INVAL;
    if (n && offsets[n] > offsets[0] && !events) return HQ_E_INVAL;
    for (uint64_t c = 0; c < n; ++c) {
        if (offsets[c + 1] < offsets[c])
            return w->fail(HQ_E_INVAL, "hq_wire_add_locals: offsets decrease");
        for (uint64_t i = offsets[c]; i < offsets[c + 1]; ++i) {
            switch (events[i].kind) {
            case HQ_EV_READ: case HQ_EV_CHECK_QUORUM: case HQ_EV_ELECTION: case HQ_EV_PROPOSE: break;
            default: return w->fail(HQ_E_INVAL, "hq_wire_add_local: kind must be a local event");
            }
        }
    }
    hq_wire::Undo undo(*w);
    for (uint64_t c = 0; c < n; ++c) {
        if (offsets[c + 1] == offsets[c]) continue;
        uint32_t k;
        if (!w->key(cluster_ids[c], &k)) {      // (a cluster the attached worker does not run)
            w->stats.dropped_no_cluster += offsets[c + 1] - offsets[c];
            continue;
        }
        for (uint64_t i = offsets[c]; i < offsets[c + 1]; ++i) {
            const hq_event &e = events[i];
            Rec r{};
            r.key = k;
            r.cat = e.kind == HQ_EV_READ ? 0 : e.kind == HQ_EV_PROPOSE ? 3 : 2;
            hqs::from_event(r, e);
            w->recs.push_back(r);
        }
        if (!w->worker) continue;
        w->count_key(k, (uint32_t)(offsets[c + 1] - offsets[c]));   // (the cluster's, at once)
        undo.counted = w->recs.size() - undo.r0;
    }
    undo.keep = true;
    return HQ_OK;
}

int hq_wire_add_locals(hq_wire *w, uint64_t n, const uint64_t *cluster_ids, const uint64_t *offsets,
                       const hq_event *events) {
    return guarded(w, "hq_wire_add_locals", [&] { return add_locals(w, n, cluster_ids, offsets, events); });
}

// The device mode: the batch framed (no message looked into), its own fields checked as below, its
// spans queued for hq_wire_step_device
static int add_batch_device(hq_wire *w, const uint8_t *bytes, size_t len) {
    const uint32_t index = w->batch_calls++;
    if (hq_wire_dev_framing(w->dev)) {               // framed at the step, on the device
        const int rc = hq_wire_dev_queue(w->dev, bytes, len, index);
        if (rc) return w->fail(rc, hq_wire_dev_error(w->dev));
        w->dev_queued++;
        return HQ_OK;
    }
    if (w->spans.empty()) w->spans.resize(1024);
    hq_wire_batch_info bi;
    uint64_t ns = 0;
    int rc = hq_wire_frame_batch(bytes, len, 0, w->spans.data(), w->spans.size(), &ns, &bi);
    if (rc == HQ_E_STATE) {
        w->spans.resize(ns);
        rc = hq_wire_frame_batch(bytes, len, 0, w->spans.data(), w->spans.size(), &ns, &bi);
    }
    if (rc) return w->fail(HQ_E_INVAL, "hq_wire_add_batch: malformed MessageBatch");
    hq_wire::Undo undo(*w);                          // (the stats: a batch that is not queued is
    w->stats.batches++;                              // not counted)
    w->stats.bytes += len;
    if (bi.deployment_id != w->deployment_id || bi.bin_ver != HQ_RPC_BIN_VERSION) {
        w->stats.dropped_batches++;
        w->stats.dropped_messages += bi.n_messages;
    } else if (bi.n_messages) {
        rc = hq_wire_dev_add_batch(w->dev, bytes, len, w->spans.data(), ns, bi.n_messages, index);
        if (rc) return w->fail(rc, hq_wire_dev_error(w->dev));
        w->dev_queued += bi.n_messages;
    }
    undo.keep = true;
    return HQ_OK;
}

// All or nothing: after an exception the queue, the per-handle counts, the clusters seen and the
// stats are as before the call (hq_wire::Undo; in the device mode the stats, and what
// hq_wire_dev_add_batch leaves of a batch it could not queue is its own). Cluster ids newly cached
// in handle_of may stay: a cache of facts that hold until the worker's epoch moves (hq_wire_reset).
static int add_batch(hq_wire *w, const uint8_t *bytes, size_t len) {
    if (!bytes && len) return w->fail(HQ_E_INVAL, "hq_wire_add_batch: NULL bytes");
    if (w->dev) return add_batch_device(w, bytes, len);
    // one pass: every message straight into a record (Message.MarshalTo's field order on the
    // fast path, any order on the general one) with its cluster id aside; the batch's own
    // fields (they follow the messages in the marshalled order) then decide whether the
    // records stay and their clusters are resolved to keys
    hq_wire::Undo undo(*w);
    const size_t r0 = undo.r0;
    w->pending.clear();
    uint64_t entries = 0, snap = 0, no_cluster = 0;
    // attached: each record's key (the worker's handle) looked up while the batch decodes,
    // kAhead messages behind the decode (the handle table's slot prefetched when the message is
    // decoded; a batch the deployment check drops afterwards only leaves its clusters' handles
    // cached); else the keys wait for that check (an index of first appearance must not see a
    // dropped batch)
    const bool now = w->worker != nullptr;
    constexpr size_t kAhead = 8;
    size_t looked = 0;
    auto look_up = [&]() {
        Rec &x = w->recs[r0 + looked];
        const uint64_t id = w->pending[looked];
        if (w->handle_of.find(id, &x.key) || w->key(id, &x.key)) {
            w->count_key(x.key);
        } else {
            x.key = hq_wire::kNoKey;
            ++no_cluster;
        }
        ++looked;
    };
    hqw::error err{};
    hq_wire_batch_info bi;
    auto on_message = [&](size_t, size_t body, size_t k) {
        const uint8_t *const m = bytes + body;
        Rec r;
        r.key = 0;
        r.pad = 0;
        r.pad2 = 0;
        uint64_t cid;
        uint32_t ent;
        if (!decode_marshal_order(m, k, r, cid, ent)) {
            hq_wire_message x;
            if (!hqw::decode_message(m, k, x, err)) return HQ_E_INVAL;
            hqs::from_event(r, x.ev);
            cid = x.cluster_id;
            ent = x.n_entries;
        }
        entries += ent;
        // HandleMessageBatch (nodehost.go:2039-2044): snapshot confirmations go aside
        if (r.type == kSnapshotReceived) {
            ++snap;
            return HQ_OK;
        }
        r.cat = 1;
        w->recs.push_back(r);
        w->pending.push_back(cid);
        if (now) {
            w->handle_of.prefetch(cid);
            if (w->pending.size() - looked > kAhead) look_up();
        }
        return HQ_OK;
    };
    int rc;
    try {
        rc = hqw::walk_batch(bytes, len, bi, on_message, [] {});
        while (now && looked < w->pending.size()) look_up();
    } catch (...) {                // (`looked` stays a local of the decode loop: `undo`
        undo.counted = looked;     // learns of the keys counted only here and below)
        throw;
    }
    undo.counted = looked;
    const uint64_t n = bi.n_messages;
    if (no_cluster && !rc) {       // the records of clusters the worker does not run leave
        size_t o = r0;
        for (size_t i = r0; i < w->recs.size(); ++i)
            if (w->recs[i].key != hq_wire::kNoKey) w->recs[o++] = w->recs[i];
        w->recs.resize(o);
        undo.counted = o - r0;
    }
    if (rc)                        // (the records leave with `undo`)
        return w->fail(HQ_E_INVAL, "hq_wire_add_batch: malformed MessageBatch" +
                                       (err.code ? ": " + message_error(err) : std::string()));
    w->stats.batches++;
    w->stats.bytes += len;
    // Transport.handleRequest (transport.go:289-300): the whole batch is dropped on a foreign
    // deployment id or binary version (none of its clusters is looked at)
    if (bi.deployment_id != w->deployment_id || bi.bin_ver != HQ_RPC_BIN_VERSION) {
        undo.drop();
        w->stats.dropped_batches++;
        w->stats.dropped_messages += n;
    } else {
        w->stats.messages += n;
        w->stats.entries += entries;
        w->stats.snapshot_received += snap;
        w->stats.dropped_no_cluster += no_cluster;
        if (!now) w->resolve(r0);
    }
    undo.keep = true;
    return HQ_OK;
}

int hq_wire_add_batch(hq_wire *w, const uint8_t *bytes, size_t len) {
    return guarded(w, "hq_wire_add_batch", [&] { return add_batch(w, bytes, len); });
}

// hq_wire_step_input, hq_wire_step_stream, hq_wire_step_sized: an exception leaves the queue and
// the stats untouched; what the call had assembled is invalid until the next successful call.
// (*dropped: the events of clusters the worker does not run, for the entry to count once nothing
// of it can throw any more)
static int step_input(hq_wire *w, hq_worker *worker, hq_step_input *out, uint64_t *dropped) {
    if (!worker || !out) return HQ_E_INVAL;
    if (w->worker) return w->fail(HQ_E_STATE, "hq_wire_step_input: attached (hq_wire_step_sized)");
    const uint32_t nc = (uint32_t)w->clusters.size();
    // handles; clusters this worker does not run are dropped (nodehost.go:2045-2046)
    w->handle.resize(nc);
    for (uint32_t k = 0; k < nc; ++k)
        if (hq_worker_find(worker, w->clusters[k], &w->handle[k]) != HQ_OK) w->handle[k] = UINT32_MAX;
    // counting sort by (cluster order of first appearance, category), stable in arrival order
    w->cnt.assign((size_t)nc * 4 + 1, 0);
    for (const auto &r : w->recs) w->cnt[(size_t)r.key * 4 + r.cat + 1]++;
    w->scatter([](const Rec &r) { return (size_t)r.key * 4 + r.cat; });
    w->groups.clear();
    w->offsets.assign(1, 0);
    w->events.clear();
    *dropped = 0;
    for (uint32_t k = 0; k < nc; ++k) {
        const uint64_t b = w->cnt[(size_t)k * 4], e = w->cnt[(size_t)k * 4 + 4];
        if (w->handle[k] == UINT32_MAX) {
            *dropped += e - b;
            continue;
        }
        if (b == e) continue;
        w->groups.push_back(w->handle[k]);
        for (uint64_t j = b; j < e; ++j) w->events.push_back(hqs::to_event(w->recs[w->perm[j]]));
        w->offsets.push_back(w->events.size());
    }
    out->n_groups = w->groups.size();
    out->groups = w->groups.data();
    out->offsets = w->offsets.data();
    out->events = w->events.data();
    return HQ_OK;
}

int hq_wire_step_input(hq_wire *w, hq_worker *worker, hq_step_input *out, hq_wire_stats *stats) {
    return guarded(w, "hq_wire_step_input", [&] {
        uint64_t dropped;
        const int rc = step_input(w, worker, out, &dropped);
        if (rc) return rc;
        w->stats.dropped_no_cluster += dropped;
        if (stats) *stats = w->stats;
        return HQ_OK;
    });
}

int hq_wire_step_stream(hq_wire *w, hq_worker *worker, hq_step_stream *out, hq_wire_stats *stats) {
    return guarded(w, "hq_wire_step_stream", [&] {
        if (!out) return HQ_E_INVAL;
        hq_step_input in;
        uint64_t dropped;
        int rc = step_input(w, worker, &in, &dropped);
        if (rc) return rc;
        w->boffsets.resize(in.n_groups + 1);
        w->bytes.resize((size_t)w->events.size() * HQ_EVENT_STREAM_MAX);
        w->stats.dropped_no_cluster += dropped;
        if (stats) *stats = w->stats;
        rc = hq_events_encode(in.n_groups, in.offsets, in.events, w->bytes.data(), w->bytes.size(),
                              w->boffsets.data());
        if (rc) return w->fail(rc, "hq_wire_step_stream: encode");
        out->n_groups = in.n_groups;
        out->groups = in.groups;
        out->offsets = in.offsets;
        out->boffsets = w->boffsets.data();
        out->bytes = w->bytes.data();
        out->sizes = nullptr;
        out->n_events = out->n_bytes = 0;
        out->sizes16 = nullptr;
        return HQ_OK;
    });
}

static int step_sized(hq_wire *w, uint8_t *bytes, uint64_t cap, uint16_t *sizes16, uint64_t n_cap,
                      hq_step_stream *out, hq_wire_stats *stats) {
    if (!out || (cap && !bytes)) return HQ_E_INVAL;
    if (!w->worker) return w->fail(HQ_E_STATE, "hq_wire_step_sized: no worker attached");
    if (w->dev) return w->fail(HQ_E_STATE, "hq_wire_step_sized: device mode (hq_wire_step_device)");
    uint64_t n = 0;
    if (hq_worker_group_count(w->worker, &n) != HQ_OK) return HQ_E_INVAL;
    if (n > n_cap || (n && !sizes16))
        return w->fail(HQ_E_INVAL, "hq_wire_step_sized: sizes16 holds fewer words than the worker's groups");
    // counting sort of the records by handle, stable in arrival order; each handle's records
    // then taken category by category (node.handleEvents: local ReadIndex, received messages,
    // ticks, proposals)
    // (the counts per handle were kept as the records were queued; the handle space only grows, so
    // every queued key is below n)
    w->cnt.assign(n + 1, 0);
    std::copy(w->kcnt.begin(), w->kcnt.begin() + std::min<size_t>(w->kcnt.size(), n + 1), w->cnt.begin());
    if (!w->scatter([](const Rec &r) { return r.key; }))
        return w->fail(HQ_E_STATE, "hq_wire_step_sized: a queued record's handle is past the worker's groups");
    uint8_t *p = bytes, *const end = bytes + cap;
    uint64_t events = 0;
    for (uint64_t h = 0; h < n; ++h) {
        const uint32_t b = w->cnt[h], e = w->cnt[h + 1];
        uint8_t *const g0 = p;
        if (e > b) {
            // the group's events gathered in arrival order; put in category order (a stable
            // insertion sort of the few out of place) when they are not already
            w->grp.resize(e - b);
            Rec *g = w->grp.data();
            bool sorted = true;
            for (uint32_t j = b; j < e; ++j) {
                g[j - b] = w->recs[w->perm[j]];
                sorted = sorted && (j == b || g[j - b - 1].cat <= g[j - b].cat);
            }
            if (!sorted)
                for (uint32_t x = 1; x < e - b; ++x)
                    for (uint32_t y = x; y > 0 && g[y - 1].cat > g[y].cat; --y) std::swap(g[y - 1], g[y]);
            p = hqs::encode_group(p, end, static_cast<const hqs::WireEvent *>(g), e - b);
            if (!p) return w->fail(HQ_E_STATE, "hq_wire_step_sized: the stream does not fit cap");
            if (p - g0 > 0xFFFF || e - b > 0xFFFF)
                return w->fail(HQ_E_INVAL, "hq_wire_step_sized: a group of 2^16 events or bytes");
            events += e - b;
        }
        sizes16[h] = (uint16_t)(p - g0);
    }
    *out = hq_step_stream{};
    out->n_groups = n;
    out->bytes = bytes;
    out->sizes16 = sizes16;
    out->n_events = events;
    out->n_bytes = (uint64_t)(p - bytes);
    if (stats) *stats = w->stats;
    return HQ_OK;
}

int hq_wire_step_sized(hq_wire *w, uint8_t *bytes, uint64_t cap, uint16_t *sizes16, uint64_t n_cap,
                       hq_step_stream *out, hq_wire_stats *stats) {
    return guarded(w, "hq_wire_step_sized", [&] { return step_sized(w, bytes, cap, sizes16, n_cap, out, stats); });
}

// What a failed device step leaves in the worker and in the device queue is unspecified, as
// after any failed step; the wire itself is usable again after hq_wire_reset.
int hq_wire_step_device(hq_wire *w, hq_step_output *out, hq_wire_stats *stats) {
    return guarded(w, "hq_wire_step_device", [&] {
        if (!out) return HQ_E_INVAL;
        if (!w->dev) return w->fail(HQ_E_STATE, "hq_wire_step_device: no device worker attached");
        uint64_t c[4], rejected_bytes = 0, n_bad_message = 0;
        hq_wire_stats add{};
        const int rc = hq_wire_dev_step(w->dev, static_cast<const hqs::WireEvent *>(w->recs.data()),
                                        w->recs.size(), out, c, &w->rejected, &w->n_rejected,
                                        &rejected_bytes, &n_bad_message, &add);
        if (rc) return w->fail(rc, hq_wire_dev_error(w->dev));
        if (stats) {
            // the kernels' counters beside the host's (with the framing on the device, the
            // batches' own counts come from its results); a batch dropped for a malformed message
            // is counted nowhere (as one hq_wire_add_batch rejects)
            *stats = w->stats;
            stats->batches += add.batches;
            stats->bytes += add.bytes;
            stats->dropped_batches += add.dropped_batches;
            stats->dropped_messages += add.dropped_messages;
            stats->messages += c[0];
            stats->entries += c[1];
            stats->snapshot_received += c[2];
            stats->dropped_no_cluster += c[3];
            stats->batches -= n_bad_message;
            stats->bytes -= rejected_bytes;
        }
        return HQ_OK;
    });
}

int hq_wire_set_device_framing(hq_wire *w, int on) {
    return guarded(w, "hq_wire_set_device_framing", [&] {
        if (!w->dev) return w->fail(HQ_E_STATE, "hq_wire_set_device_framing: no device worker attached");
        if (const int rc = w->need_empty("hq_wire_set_device_framing")) return rc;
        hq_wire_dev_set_framing(w->dev, on != 0, w->deployment_id);
        return HQ_OK;
    });
}

int hq_wire_device_frame_stats(hq_wire *w, uint64_t out[4]) {
    return guarded(w, "hq_wire_device_frame_stats", [&] {
        if (!out) return HQ_E_INVAL;
        if (!w->dev) return w->fail(HQ_E_STATE, "hq_wire_device_frame_stats: no device worker attached");
        hq_wire_dev_frame_stats(w->dev, out);
        return HQ_OK;
    });
}

int hq_wire_device_rejected(hq_wire *w, const uint32_t **batches, uint64_t *n) {
    return guarded(w, "hq_wire_device_rejected", [&] {
        if (!batches || !n) return HQ_E_INVAL;
        if (!w->dev) return w->fail(HQ_E_STATE, "hq_wire_device_rejected: no device worker attached");
        *batches = w->rejected;
        *n = w->n_rejected;
        return HQ_OK;
    });
}

}  // extern "C"
