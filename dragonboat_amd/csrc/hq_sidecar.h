// hq_sidecar.h — what the step worker's device modules share beside their kernels (hq_heartbeat,
// hq_heartbeat_wire, hq_config, hq_groups, hq_pool, hq_tick, hq_hb_received .hip): owning
// grow-on-demand buffers, the base of a module's struct with its one open and one close, and the
// two helpers every call ends with. For .hip files only; hq_worker_*.cpp see the modules' structs
// as opaque.
//
// The rule the modules keep with it: nothing of a call stays queued behind its return. Every
// return after a call's first operation on the stream goes through finish(), on the error paths
// too: what was queued may read the caller's memory or the module's pinned staging, which the
// caller or the next call rewrites, and a buffer may be freed as soon as a call has returned.
#pragma once

#include <hip/hip_runtime.h>

#include <new>

#include "hq_internal.h"

namespace hq {

// The stream waited for whatever `rc` says: nothing of a call stays queued behind its return.
inline int finish(hq_ctx *ctx, int rc, const char *what) {
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);     // (rc's message stands)
        return rc;
    }
    return check_hip(ctx, hipStreamSynchronize(ctx->stream), what);
}

// GPU time between two completed events (0 if it cannot be read)
inline uint64_t elapsed_ns(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return (uint64_t)((double)ms * 1e6);
}

// How much a buffer that is short is given. Capacity is memory footprint, so each keeps its rule:
enum class Headroom {
    kHalf,      // need + need / 2
    kExact64,   // need, rounded up to 64: the records of hq_groups.hip; a fetch of every group of a
                // large worker is hundreds of megabytes, so no headroom
    kHalf64,    // need + need / 2, rounded up to 64 (hq_pool.hip)
};
inline size_t with_headroom(size_t need, Headroom h) {
    if (h == Headroom::kExact64) return (need + 63) / 64 * 64;
    if (h == Headroom::kHalf64) return (need + need / 2 + 63) / 64 * 64;
    return need + need / 2;
}

// `cap()` elements of device (hipMalloc) or pinned host (hipHostMalloc) memory, owned. The device
// of the context that grew it must be current when it is destroyed (sidecar_close).
template <class T, bool kPinned>
class Buf {
public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { release(p_); }

    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t cap() const { return cap_; }

    // Exactly `count` elements if there are fewer, contents dropped. The new block is had before
    // the old one goes; on failure the old one stands. The caller knows that nothing queued uses
    // the old block.
    int reserve(hq_ctx *ctx, size_t count, const char *what) {
        if (count <= cap_) return HQ_OK;
        T *n = nullptr;
        int rc = alloc(ctx, &n, count, what);
        if (rc) return rc;
        adopt(n, count);
        return HQ_OK;
    }
    // At least `need` elements, as reserve(), with headroom when it has to grow.
    int grow(hq_ctx *ctx, size_t need, const char *what, Headroom h = Headroom::kHalf) {
        return need <= cap_ ? (int)HQ_OK : reserve(ctx, with_headroom(need, h), what);
    }

    // At least `need` elements with the first `keep` kept and every other byte `fill_byte`. The
    // fill and the copy are queued on the context's stream and waited for before the old block
    // goes; on failure the new block is freed and the old one stands.
    int grow_keep(hq_ctx *ctx, size_t need, size_t keep, int fill_byte, const char *what) {
        static_assert(!kPinned, "device buffers only");
        if (need <= cap_) return HQ_OK;
        const size_t want = with_headroom(need, Headroom::kHalf);
        T *n = nullptr;
        int rc = alloc(ctx, &n, want, what);
        if (rc) return rc;
        rc = check_hip(ctx, hipMemsetAsync(n, fill_byte, want * sizeof(T), ctx->stream), what);
        if (!rc && keep)
            rc = check_hip(ctx, hipMemcpyAsync(n, p_, keep * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream), what);
        rc = finish(ctx, rc, what);
        if (rc) {
            release(n);
            return rc;
        }
        adopt(n, want);
        return HQ_OK;
    }

private:
    static int alloc(hq_ctx *ctx, T **n, size_t count, const char *what) {
        void **v = reinterpret_cast<void **>(n);
        return check_hip(ctx, kPinned ? hipHostMalloc(v, count * sizeof(T), hipHostMallocDefault)
                                      : hipMalloc(v, count * sizeof(T)), what);
    }
    static void release(T *p) {
        if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
    }
    void adopt(T *n, size_t count) {
        release(p_);
        p_ = n;
        cap_ = count;
    }

    T *p_ = nullptr;
    size_t cap_ = 0;
};
template <class T> using DevBuf = Buf<T, false>;
template <class T> using PinBuf = Buf<T, true>;

// The base of a module's struct: its context, an event pair around a call's kernels, a device
// block for the error word (16 bytes unless the module keeps counts beside it) and a pinned block
// of 64 zeroed bytes for the totals and the error word as the host reads them. The module's own
// buffers are Buf members of the derived struct: sidecar_close frees them all.
struct Sidecar {
    hq_ctx *ctx = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DevBuf<uint64_t> dev;
    PinBuf<uint64_t> totals;

    uint32_t *error() const { return reinterpret_cast<uint32_t *>(dev.get()); }

    Sidecar() = default;
    Sidecar(const Sidecar &) = delete;
    Sidecar &operator=(const Sidecar &) = delete;
    ~Sidecar() {
        for (hipEvent_t e : {ev0, ev1})
            if (e) (void)hipEventDestroy(e);
    }
};

// Sets the device and waits for the context's stream, then frees everything: the wait stands here
// and not in ~Sidecar, which runs after the derived struct's buffers are gone.
template <class M>
void sidecar_close(M *m) {
    if (!m) return;
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->ctx->stream);
    delete m;
}

template <class M>
int sidecar_open(hq_ctx *ctx, M **out, const char *what, size_t dev_bytes = 16) {
    *out = nullptr;
    M *m = new (std::nothrow) M();
    if (!m) return HQ_E_NOMEM;
    m->ctx = ctx;
    int rc = check_hip(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    for (hipEvent_t *e : {&m->ev0, &m->ev1})
        if (!rc) rc = check_hip(ctx, hipEventCreate(e), "event");
    if (!rc) rc = m->dev.reserve(ctx, (dev_bytes + 7) / 8, what);
    if (!rc) rc = m->totals.reserve(ctx, 8, what);
    if (rc) {
        sidecar_close(m);
        return rc;
    }
    for (int i = 0; i < 8; ++i) m->totals[i] = 0;
    *out = m;
    return HQ_OK;
}

}  // namespace hq
