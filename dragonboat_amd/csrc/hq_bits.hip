// hq_bits.hip — ReadIndex, vote and CheckQuorum over per-group bitmaps, in three layouts, with
// their column -> tile packers and the hq_readindex*, hq_vote*, hq_check_quorum* and hq_tile_*
// launchers:
//   u8 columns and 1024-group byte tiles (k_bits): 16 groups per lane, byte-SWAR popcounts;
//   3-byte tiles (k_bits3): the same with the leader's own slot dropped;
//   bit planes (k_planes, k_planes_cq, k_cq_planes): 32 groups per lane, bit-sliced adders.
// Each is an HBM stream: 16-byte (planes: 4-byte) nontemporal loads, decisions in registers,
// outputs written as the bitmap words themselves. No LDS and no MFMA (DESIGN.md "Kernels").
#include "hq_launch.h"

namespace {

// ---- ReadIndex / vote / CheckQuorum over u8 bitmaps: 16 groups per lane ---------------------
struct BitsK {
    uint64_t G;
    uint32_t n_uniform, self_slot;
    const uint8_t *ack, *granted, *rejected;
    uint8_t *active;
    const uint8_t *nv;
    uint64_t *confirmed, *outcome, *has_quorum, *fallback;
    uint64_t n16;   // number of 16-group slots covered by the 64-group bitmap words
    uint64_t n16o;  // number of 16-group slots covered by the 32-group outcome words
    const uint8_t *tiles;  // HQ_LAYOUT_TILES: 1024-group tiles of rows [n] ack granted rejected
    uint32_t tile_rows;    // 4 with the per-group n row, else 3
};

constexpr int kRI = 1, kVOTE = 2, kCHECKQ = 4;

union V16 {
    uint4 v;
    u32x4 w;
    uint8_t b[16];
};

__device__ __forceinline__ V16 load16(const uint8_t *p, uint64_t g, uint64_t G) {
    V16 r;
    if (g + 16 <= G) {
        r.w = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p + g));
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) r.b[k] = (g + k < G) ? p[g + k] : 0;
    }
    return r;
}

// ---- SWAR helpers: four groups per 32-bit word, one byte each -------------------------------
constexpr uint32_t kB80 = 0x80808080u, kB01 = 0x01010101u;

// per-byte popcount (each result byte 0..8)
__device__ __forceinline__ uint32_t popc_bytes(uint32_t x) {
    x = x - ((x >> 1) & 0x55555555u);
    x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u);
    return (x + (x >> 4)) & 0x0F0F0F0Fu;
}
// bit 7 of each byte: a_byte >= b_byte, for bytes a, b < 128
__device__ __forceinline__ uint32_t ge_bytes(uint32_t a, uint32_t b) {
    return ((a | kB80) - b) & kB80;
}
// 4 flag bytes (0x80 / 0x00) -> 4 consecutive bits (group k -> bit k): a byte dot product with
// weights 1, 2, 4, 8 (v_dot4_u32_u8, full rate; the multiply it replaces is quarter rate)
__device__ __forceinline__ uint32_t pack4(uint32_t f) {
    return __builtin_amdgcn_udot4(f, 0x08040201u, 0u, false) >> 7;
}
// 4 flag bytes -> bits 0, 2, 4, 6 (the low bit of 2-bit fields); `hi` flags -> bits 1, 3, 5, 7
__device__ __forceinline__ uint32_t pack4x2(uint32_t f, uint32_t hi = 0) {
    return __builtin_amdgcn_udot4(f, 0x40100401u, __builtin_amdgcn_udot4(hi, 0x80200802u, 0u, false),
                                  false) >> 7;
}
// per-byte valid n in [1, 8] -> 0x80
__device__ __forceinline__ uint32_t valid_n(uint32_t n) {
    const uint32_t lo = n & 0x0F0F0F0Fu, hi = (n >> 4) & 0x0F0F0F0Fu;
    return (lo + 0x7F7F7F7Fu) & ~(lo + 0x77777777u) & ~(hi + 0x7F7F7F7Fu) & kB80;
}
// per-byte (1 << n) - 1 for n in [0, 8] with v_perm_b32 as a byte lookup table: selectors 0..7
// pick masks 0x00..0x7F from {0x7F3F1F0F, 0x07030100}; selector 13 (n = 8) yields 0xFF
__device__ __forceinline__ uint32_t mask_n(uint32_t n) {
    const uint32_t b3 = n & 0x08080808u;   // n = 8 -> selector 8 | 4 | 1 = 13 (no multiply)
    const uint32_t sel = n | (b3 >> 1) | (b3 >> 3);
    return __builtin_amdgcn_perm(0x7F3F1F0Fu, 0x07030100u, sel);
}

// One 16-group slot starting at group g. FULL: all 16 groups exist (g + 16 <= G), so every load
// is one unconditional 16-byte nontemporal load and no byte needs masking (the common case; the
// ragged tail slot takes the guarded path).
// TILED: the inputs are the slot's tile rows, loaded by the caller before it branches on the full
// tile test (so the four loads issue together); every tile is padded to 1024 groups, so even the
// ragged last slot holds 16 loaded bytes (the padding bytes are masked by `inr` like any byte
// beyond G).
template <int MODE, bool PERN, bool FULL, bool TILED = false, bool FB = true>
__device__ __forceinline__ void bits_slot(const BitsK &a, uint64_t g, uint32_t nu,
                                          const V16 *trow = nullptr) {
    const uint64_t slot = g >> 4;
    V16 nv = {}, ack = {}, gr = {}, rj = {}, ac = {};
    auto ld = [&](const uint8_t *p, uint32_t row = 0) -> V16 {
        if constexpr (TILED) {
            return trow[row];
        } else if constexpr (FULL) {
            V16 r;
            r.w = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p + g));
            return r;
        }
        return g < a.G ? load16(p, g, a.G) : V16{};
    };
    constexpr uint32_t r0 = PERN ? 1 : 0;   // tile rows: [n] ack granted rejected
    if constexpr (PERN) nv = ld(a.nv, 0);
    if constexpr (MODE & kRI) ack = ld(a.ack, r0);
    if constexpr (MODE & kVOTE) {
        gr = ld(a.granted, r0 + 1);
        rj = ld(a.rejected, r0 + 2);
    }
    if constexpr (MODE & kCHECKQ) ac = ld(a.active);
    uint32_t conf = 0, outc = 0, hq = 0, fb = 0;
    V16 keep;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        // bytes of groups >= G are excluded (their output bits stay 0)
        uint32_t inr = kB80;
        if constexpr (!FULL) {
            const uint64_t left = g < a.G ? a.G - g : 0;
            inr = left >= (uint64_t)(4 * w + 4) ? kB80
                  : left <= (uint64_t)(4 * w)   ? 0u
                                                : (kB80 >> (8 * (4 - (uint32_t)(left - 4 * w))));
        }
        const uint32_t n = PERN ? nv.w[w] : nu;
        const uint32_t ok = valid_n(n) & inr;
        const uint32_t mask = mask_n(n);
        const uint32_t quorum = ((n >> 1) & 0x7F7F7F7Fu) + kB01;  // n/2 + 1 (valid bytes)
        uint32_t bad = ~ok & inr;
        if constexpr (MODE & kRI) {
            // readindex.go:84: len(confirmed) + 1 >= quorum  <=>  acks >= quorum - 1
            const uint32_t c = popc_bytes(ack.w[w] & mask);
            conf |= pack4(ge_bytes(c, quorum - kB01) & ok) << (4 * w);
        }
        if constexpr (MODE & kVOTE) {
            const uint32_t gm = gr.w[w] & mask;
            const uint32_t rm = rj.w[w] & mask & ~gm;  // first response wins
            const uint32_t lead = ge_bytes(popc_bytes(gm), quorum) & ok;
            const uint32_t foll = ge_bytes(popc_bytes(rm), quorum) & ok & ~lead;
            const uint32_t cand = inr & ~lead & ~foll;
            // 2-bit codes: leader 2 (bit 1), candidate 1 (bit 0), follower 0
            outc |= pack4x2(cand, lead) << (8 * w);
        }
        if constexpr (MODE & kCHECKQ) {
            const uint32_t self = kB01 << a.self_slot;
            const uint32_t selfok = ge_bytes(n, (a.self_slot + 1) * kB01) & ok;
            bad = ~selfok & inr;
            const uint32_t c = popc_bytes((ac.w[w] | self) & mask);
            hq |= pack4(ge_bytes(c, quorum) & selfok) << (4 * w);
            // setNotActive for every voting member (raft.go:385, remote.go:196-198);
            // groups left to the CPU path keep their flags
            keep.w[w] = ac.w[w] & ((bad >> 7) * 0xFFu);
        }
        if constexpr (FB) fb |= pack4(bad) << (4 * w);
    }
    // 64-group bitmap words viewed as 16-bit slots, 32-group outcome words as 32-bit slots
    // (a full slot lies below G / 16 <= n16, n16o)
    if (FULL || slot < a.n16) {
        if constexpr (MODE & kRI) reinterpret_cast<uint16_t *>(a.confirmed)[slot] = conf;
        if constexpr (MODE & kCHECKQ) reinterpret_cast<uint16_t *>(a.has_quorum)[slot] = hq;
        if (FB && a.fallback) reinterpret_cast<uint16_t *>(a.fallback)[slot] = fb;
    }
    if constexpr (MODE & kVOTE) {
        if (FULL || slot < a.n16o) reinterpret_cast<uint32_t *>(a.outcome)[slot] = outc;
    }
    if constexpr (MODE & kCHECKQ) {
        if constexpr (FULL) {
            *reinterpret_cast<uint4 *>(a.active + g) = keep.v;
        } else {
            for (int k = 0; k < 16; ++k)
                if (g + k < a.G) a.active[g + k] = keep.b[k];
        }
    }
}

// FB = false (no fallback bitmap requested) drops the fallback bits' arithmetic (tiles only)
template <int MODE, bool PERN, int BLK, bool TILED = false, bool FB = true>
__global__ __launch_bounds__(BLK) void k_bits(const BitsK a) {
    const uint64_t tid = (uint64_t)blockIdx.x * BLK + threadIdx.x;
    const uint64_t step = (uint64_t)gridDim.x * BLK * 16;
    const uint32_t nu = a.n_uniform * kB01;  // n_uniform <= 8: no byte overflow
    if constexpr (TILED) {
        // one wave per 1024-group tile: the tile base is wave-uniform (scalar), lane i reads
        // bytes [16 i, 16 i + 16) of every row
        constexpr uint64_t R = PERN ? 4 : 3;
        const uint64_t lane = threadIdx.x & 63;
        const uint64_t wave = (uint64_t)blockIdx.x * (BLK / 64) +
                              __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const uint64_t nw = (uint64_t)gridDim.x * (BLK / 64);
        const uint64_t slots = a.n16o > a.n16 ? a.n16o : a.n16;
        const uint64_t ntiles = (slots * 16 + 1023) >> 10;
        for (uint64_t t = wave; t < ntiles; t += nw) {
            const uint8_t *base = a.tiles + t * (R << 10) + lane * 16;
            V16 rows[R];
#pragma unroll
            for (uint64_t r = 0; r < R; ++r)
                rows[r].w = __builtin_nontemporal_load(
                    reinterpret_cast<const u32x4 *>(base + (r << 10)));
            const uint64_t g = (t << 10) + lane * 16;
            if ((t << 10) + 1024 <= a.G)
                bits_slot<MODE, PERN, true, true, FB>(a, g, nu, rows);
            else
                bits_slot<MODE, PERN, false, true, FB>(a, g, nu, rows);
        }
        return;
    }
    for (uint64_t g = tid * 16; g < a.n16o * 16 || g < a.n16 * 16; g += step) {
        if (g + 16 <= a.G)
            bits_slot<MODE, PERN, true, TILED>(a, g, nu);
        else
            bits_slot<MODE, PERN, false, TILED>(a, g, nu);
    }
}

// ---- 3-byte bitmap tiles (hq_readindex_vote_tiles3_dev) -------------------------------------
// The leader's / candidate's own slot 0 carries no information: it never acks its own ReadIndex
// ctx (readindex.go:84 counts it as the +1), always grants its own vote (campaign, raft.go:1093)
// and never rejects it. So each of the three rows keeps the 7 bits of slots 1..7 (bit k = slot
// k + 1) and its bit 7 holds one bit of n - 1: ack row bit 0 of n - 1, granted row bit 1,
// rejected row bit 2. 3 bytes per group instead of 4 (rows [n] ack granted rejected), n always
// in [1, 8]: nothing to fall back on.
template <bool FULL>
__device__ __forceinline__ void bits3_slot(const BitsK &a, uint64_t g, const V16 *rows) {
    const uint64_t slot = g >> 4;
    uint32_t conf = 0, outc = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        uint32_t inr = kB80;
        if constexpr (!FULL) {
            const uint64_t left = g < a.G ? a.G - g : 0;
            inr = left >= (uint64_t)(4 * w + 4) ? kB80
                  : left <= (uint64_t)(4 * w)   ? 0u
                                                : (kB80 >> (8 * (4 - (uint32_t)(left - 4 * w))));
        }
        const uint32_t A = rows[0].w[w], Gr = rows[1].w[w], Rj = rows[2].w[w];
        const uint32_t nm1 = ((A >> 7) & kB01) | ((Gr >> 6) & 0x02020202u) | ((Rj >> 5) & 0x04040404u);
        const uint32_t mask = mask_n(nm1);                 // the other voters' bits 0 .. n-2
        const uint32_t half = ((nm1 + kB01) >> 1) & 0x7F7F7F7Fu;   // n/2 = quorum - 1
        // readindex.go:84: acks + 1 >= quorum <=> acks >= n/2
        conf |= pack4(ge_bytes(popc_bytes(A & mask), half) & inr) << (4 * w);
        // handleVoteResp: granted (self included) / rejected (first response wins) >= quorum
        const uint32_t gm = Gr & mask, rm = Rj & mask & ~gm;
        const uint32_t lead = ge_bytes(popc_bytes(gm), half) & inr;          // gm + 1 >= n/2 + 1
        const uint32_t foll = ge_bytes(popc_bytes(rm), half + kB01) & inr & ~lead;
        outc |= pack4x2(inr & ~lead & ~foll, lead) << (8 * w);
    }
    if (FULL || slot < a.n16) reinterpret_cast<uint16_t *>(a.confirmed)[slot] = conf;
    if (FULL || slot < a.n16o) reinterpret_cast<uint32_t *>(a.outcome)[slot] = outc;
}

// TPW tiles per wave and iteration, every row load of them issued before the first decision
// (2 took 12.6-12.7 vs 13.4-13.6 us per 16M-group launch on one box, 4 no better than 1)
constexpr int kB3TPW = 2;

template <int BLK>
__global__ __launch_bounds__(BLK) void k_bits3(const BitsK a) {
    const uint64_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (BLK / 64) +
                          __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t nw = (uint64_t)gridDim.x * (BLK / 64);
    const uint64_t slots = a.n16o > a.n16 ? a.n16o : a.n16;
    const uint64_t ntiles = (slots * 16 + 1023) >> 10;
    for (uint64_t t0 = wave * kB3TPW; t0 < ntiles; t0 += nw * kB3TPW) {
        V16 rows[kB3TPW][3];
#pragma unroll
        for (int j = 0; j < kB3TPW; ++j) {
            const uint64_t t = t0 + j < ntiles ? t0 + j : t0;   // wave-uniform
            const uint8_t *base = a.tiles + t * (3 << 10) + lane * 16;
#pragma unroll
            for (uint64_t r = 0; r < 3; ++r)
                rows[j][r].w = __builtin_nontemporal_load(
                    reinterpret_cast<const u32x4 *>(base + (r << 10)));
        }
#pragma unroll
        for (int j = 0; j < kB3TPW; ++j) {
            const uint64_t t = t0 + j;
            if (t >= ntiles) break;
            const uint64_t g = (t << 10) + lane * 16;
            if ((t << 10) + 1024 <= a.G) bits3_slot<true>(a, g, rows[j]);
            else bits3_slot<false>(a, g, rows[j]);
        }
    }
}

// columns -> 3-byte tiles: one thread per group; a group outside the contract (n not in
// [1, 8], its own slot acked / not granted / rejected) gets a fallback bit and zero bytes
__global__ __launch_bounds__(kBlock) void k_tile_bits3(uint64_t G, const uint8_t *nv, uint32_t nu,
                                                       const uint8_t *ack, const uint8_t *gr,
                                                       const uint8_t *rj, uint8_t *tiles,
                                                       uint64_t *fallback) {
    const uint64_t total = (G + 1023) / 1024 * 1024;
    for (uint64_t g0 = (uint64_t)blockIdx.x * kBlock; g0 < total; g0 += (uint64_t)gridDim.x * kBlock) {
        const uint64_t g = g0 + threadIdx.x;
        uint32_t A = 0, Gr = 0, Rj = 0;
        bool bad = false;
        if (g < G) {
            const uint32_t n = nv ? nv[g] : nu;
            const uint32_t a = ack[g], x = gr[g], r = rj[g];
            bad = n < 1 || n > 8 || (a & 1) || !(x & 1) || (r & 1);
            if (!bad) {
                const uint32_t keep = (1u << n) - 2u, m = n - 1;   // slots 1 .. n-1
                A = ((a & keep) >> 1) | ((m & 1) << 7);
                Gr = ((x & keep) >> 1) | (((m >> 1) & 1) << 7);
                Rj = ((r & keep) >> 1) | (((m >> 2) & 1) << 7);
            }
        }
        if (g < total) {
            uint8_t *row = tiles + (g >> 10) * (3 << 10) + (g & 1023);
            row[0] = (uint8_t)A;
            row[1024] = (uint8_t)Gr;
            row[2048] = (uint8_t)Rj;
        }
        const uint64_t b = __ballot(bad);
        if (fallback && (threadIdx.x & 63) == 0 && g < ((G + 63) & ~63ull)) fallback[g >> 6] = b;
    }
}

// ---- bit-plane tiles (hq_readindex_vote_planes_dev) -----------------------------------------
// The 3-byte tiles transposed: a 2048-group tile holds 24 planes of 256 bytes, plane 8r + b =
// bit b of row r's byte (rows ack, granted, rejected) for the tile's groups, bit j of dword k =
// group 32k + j. A lane takes 32 groups: one dword of every plane, and decides them with
// bitwise full adders and comparators over the planes (bit-sliced: ~6 instructions per group
// for both decisions, against ~15 for the byte-SWAR form of k_bits3). The confirmed plane is
// the confirmed bitmap word as it is; the outcome codes interleave the candidate and leader
// planes.
constexpr uint32_t kPlaneTile = HQ_PLANE_TILE_GROUPS;   // 2048
// tiles per wave and iteration (1: 10.3 us per 16M-group launch, 2: 10.7 us — 103 VGPRs, half
// the occupancy) and threads per block of the plane kernels
constexpr int kPlTPW = 1;
constexpr int kPlBlock = 256;
// tiles per wave of the fused ReadIndex + vote + CheckQuorum pass (one after the other)
constexpr int kPlCqTPW = 1;

__device__ __forceinline__ void full_add(uint32_t a, uint32_t b, uint32_t c, uint32_t &s,
                                         uint32_t &co) {
    const uint32_t t = a ^ b;
    s = t ^ c;
    co = (a & b) | (c & t);
}

// popcount of 7 planes as a 3-bit bit-sliced number (c0 + 2 c1 + 4 c2)
__device__ __forceinline__ void count7(const uint32_t *x, uint32_t &c0, uint32_t &c1,
                                       uint32_t &c2) {
    uint32_t s1, k1, s2, k2, k3;
    full_add(x[0], x[1], x[2], s1, k1);
    full_add(x[3], x[4], x[5], s2, k2);
    full_add(s1, s2, x[6], c0, k3);
    full_add(k1, k2, k3, c1, c2);
}

// (a2 a1 a0) >= (b2 b1 b0), bit-sliced
__device__ __forceinline__ uint32_t ge3(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t b0,
                                        uint32_t b1, uint32_t b2) {
    const uint32_t lt = (~a2 & b2) | (~(a2 ^ b2) & ((~a1 & b1) | (~(a1 ^ b1) & (~a0 & b0))));
    return ~lt;
}

// 2-bit codes of 32 groups: bit 2j = lo_j, bit 2j + 1 = hi_j (byte zip, then a perfect shuffle
// of each 16-bit unit)
__device__ __forceinline__ uint32_t shuffle16(uint32_t x) {
    x = (x & 0xF00FF00Fu) | ((x & 0x00F000F0u) << 4) | ((x >> 4) & 0x00F000F0u);
    x = (x & 0xC3C3C3C3u) | ((x & 0x0C0C0C0Cu) << 2) | ((x >> 2) & 0x0C0C0C0Cu);
    x = (x & 0x99999999u) | ((x & 0x22222222u) << 1) | ((x >> 1) & 0x22222222u);
    return x;
}

// CQ: also decide CheckQuorum for the same 32 groups from `act`, this lane's dword of the tile's
// 7 active-flag planes (plane k = the active flag of voting slot k + 1; the leader's slot 0
// counts implicitly, raft.go:384), masked to the group's voting slots by the n planes of `p`.
template <bool FULL, bool CQ = false>
__device__ __forceinline__ void planes_slot(const BitsK &a, uint64_t g, const uint32_t *p,
                                            const uint32_t *act = nullptr) {
    const uint32_t n0 = p[7], n1 = p[15], n2 = p[23];     // n - 1
    uint32_t m[7];                                        // slot k + 1 votes: n - 1 > k
    m[0] = n0 | n1 | n2;
    m[1] = n1 | n2;
    m[2] = n2 | (n1 & n0);
    m[3] = n2;
    m[4] = n2 & (n1 | n0);
    m[5] = n2 & n1;
    m[6] = n2 & n1 & n0;
    const uint32_t c = n1 & n0;                           // n / 2 = (n - 1 + 1) >> 1
    const uint32_t h0 = n1 ^ n0, h1 = n2 ^ c, h2 = n2 & c;
    uint32_t x[7], y[7], z[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        x[k] = p[k] & m[k];
        y[k] = p[8 + k] & m[k];
        z[k] = p[16 + k] & m[k] & ~y[k];                  // first response wins
    }
    uint32_t a0, a1, a2, g0, g1, g2, r0, r1, r2;
    count7(x, a0, a1, a2);
    count7(y, g0, g1, g2);
    count7(z, r0, r1, r2);
    uint32_t inr = ~0u;
    if constexpr (!FULL) {
        const uint64_t left = a.G - g;                    // g < G
        inr = left >= 32 ? ~0u : (1u << left) - 1u;
    }
    // readindex.go:84: acks + 1 >= quorum <=> acks >= n/2; handleVoteResp: granted + 1 >=
    // quorum, rejected >= quorum <=> rejected > n/2
    const uint32_t conf = ge3(a0, a1, a2, h0, h1, h2) & inr;
    const uint32_t lead = ge3(g0, g1, g2, h0, h1, h2) & inr;
    const uint32_t foll = ~ge3(h0, h1, h2, r0, r1, r2) & inr & ~lead;
    const uint32_t cand = inr & ~lead & ~foll;
    reinterpret_cast<uint32_t *>(a.confirmed)[g >> 5] = conf;
    if constexpr (CQ) {
        // leaderHasQuorum (raft.go:380-390): 1 + active voting slots >= n/2 + 1, the same
        // threshold as the ReadIndex acks
        uint32_t v[7], c0, c1, c2;
#pragma unroll
        for (int k = 0; k < 7; ++k) v[k] = act[k] & m[k];
        count7(v, c0, c1, c2);
        reinterpret_cast<uint32_t *>(a.has_quorum)[g >> 5] = ge3(c0, c1, c2, h0, h1, h2) & inr;
    }
    const uint32_t w0 = shuffle16(__builtin_amdgcn_perm(lead, cand, 0x05010400u));
    const uint32_t w1 = shuffle16(__builtin_amdgcn_perm(lead, cand, 0x07030602u));
    *reinterpret_cast<uint2 *>(reinterpret_cast<uint32_t *>(a.outcome) + (g >> 4)) =
        make_uint2(w0, w1);
}

template <int BLK>
__global__ __launch_bounds__(BLK) void k_planes(const BitsK a) {
    const uint64_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (BLK / 64) +
                          __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t nw = (uint64_t)gridDim.x * (BLK / 64);
    const uint64_t ntiles = (a.G + kPlaneTile - 1) / kPlaneTile;
    for (uint64_t t0 = wave * kPlTPW; t0 < ntiles; t0 += nw * kPlTPW) {
        uint32_t p[kPlTPW][24];
#pragma unroll
        for (int j = 0; j < kPlTPW; ++j) {
            const uint64_t t = t0 + j < ntiles ? t0 + j : t0;   // wave-uniform
            const uint32_t *base =
                reinterpret_cast<const uint32_t *>(a.tiles + t * (kPlaneTile * 3)) + lane;
#pragma unroll
            for (int q = 0; q < 24; ++q) p[j][q] = __builtin_nontemporal_load(base + q * 64);
        }
#pragma unroll
        for (int j = 0; j < kPlTPW; ++j) {
            const uint64_t t = t0 + j;
            if (t >= ntiles) break;
            const uint64_t g = t * kPlaneTile + lane * 32;
            if (t * kPlaneTile + kPlaneTile <= a.G) planes_slot<true>(a, g, p[j]);
            else if (g < a.G) planes_slot<false>(a, g, p[j]);
            else if (g < ((a.G + 63) & ~63ull))           // the rest of the last bitmap word
                reinterpret_cast<uint32_t *>(a.confirmed)[g >> 5] = 0;
        }
    }
}

// ReadIndex + vote + CheckQuorum in one pass (hq_readindex_vote_cq_planes_dev): a step worker
// decides all three for the same leader groups (readindex.go:77-116, raft.go:1968-1985,
// raft.go:380-390), so one launch reads a tile's 24 vote / ack planes and its 7 active-flag
// planes (a separate 1792-byte tile per 2048 groups, the layout hq_tile_cq_planes_dev builds with
// n_uniform 8 and self slot 0), writes the confirmed, outcome and has-quorum words and zeroes
// the active planes it read (setNotActive of every voting member, remote.go:196-198): one
// launch boundary instead of two.
template <int BLK>
__global__ __launch_bounds__(BLK) void k_planes_cq(const BitsK a, uint8_t *active_planes) {
    const uint64_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (BLK / 64) +
                          __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t nw = (uint64_t)gridDim.x * (BLK / 64);
    const uint64_t ntiles = (a.G + kPlaneTile - 1) / kPlaneTile;
    for (uint64_t t = wave; t < ntiles; t += nw) {
        const uint32_t *base = reinterpret_cast<const uint32_t *>(a.tiles + t * (kPlaneTile * 3)) + lane;
        uint32_t *abase = reinterpret_cast<uint32_t *>(active_planes + t * (7 * (kPlaneTile / 8))) + lane;
        uint32_t p[24], q[7];
#pragma unroll
        for (int k = 0; k < 24; ++k) p[k] = __builtin_nontemporal_load(base + k * 64);
#pragma unroll
        for (int k = 0; k < 7; ++k) q[k] = __builtin_nontemporal_load(abase + k * 64);
        // the zeroes go out right behind the loads of the same words (in order per wave):
        // 15.5-15.7 us per 16 M x 7 launch against 15.7-15.9 us with the zeroes after the
        // decision (profiles/r03c/ab_c4pq_zero_early.log)
#pragma unroll
        for (int k = 0; k < 7; ++k) __builtin_nontemporal_store(0u, abase + k * 64);
        const uint64_t g = t * kPlaneTile + lane * 32;
        if (t * kPlaneTile + kPlaneTile <= a.G) {
            planes_slot<true, true>(a, g, p, q);
        } else if (g < a.G) {
            planes_slot<false, true>(a, g, p, q);
        } else if (g < ((a.G + 63) & ~63ull)) {           // the rest of the last bitmap words
            reinterpret_cast<uint32_t *>(a.confirmed)[g >> 5] = 0;
            reinterpret_cast<uint32_t *>(a.has_quorum)[g >> 5] = 0;
        }
    }
}

// columns -> bit-plane tiles: one thread per group computes its 3 bytes (as k_tile_bits3), the
// wave's 64 groups become 24 ballots, lane q < 24 stores plane q's 8 bytes
__global__ __launch_bounds__(kBlock) void k_tile_planes(uint64_t G, const uint8_t *nv,
                                                        uint32_t nu, const uint8_t *ack,
                                                        const uint8_t *gr, const uint8_t *rj,
                                                        uint8_t *planes, uint64_t *fallback) {
    const uint64_t total = (G + kPlaneTile - 1) / kPlaneTile * kPlaneTile;
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t g0 = (uint64_t)blockIdx.x * kBlock; g0 < total;
         g0 += (uint64_t)gridDim.x * kBlock) {
        const uint64_t g = g0 + threadIdx.x;
        uint32_t bytes = 0;
        bool bad = false;
        if (g < G) {
            const uint32_t n = nv ? nv[g] : nu;
            const uint32_t av = ack[g], x = gr[g], r = rj[g];
            bad = n < 1 || n > 8 || (av & 1) || !(x & 1) || (r & 1);
            if (!bad) {
                const uint32_t keep = (1u << n) - 2u, m = n - 1;
                bytes = (((av & keep) >> 1) | ((m & 1) << 7)) |
                        ((((x & keep) >> 1) | (((m >> 1) & 1) << 7)) << 8) |
                        ((((r & keep) >> 1) | (((m >> 2) & 1) << 7)) << 16);
            }
        }
        uint64_t mine = 0;
#pragma unroll
        for (int q = 0; q < 24; ++q) {
            const uint64_t b = __ballot((bytes >> q) & 1);
            if (lane == (uint32_t)q) mine = b;
        }
        const uint64_t gw = g - lane;                     // the wave's first group
        if (gw < total && lane < 24)
            *reinterpret_cast<uint64_t *>(planes + (gw / kPlaneTile) * (kPlaneTile * 3) +
                                          lane * (kPlaneTile / 8) + (gw % kPlaneTile) / 8) = mine;
        const uint64_t b = __ballot(bad);
        if (fallback && lane == 0 && gw < ((G + 63) & ~63ull)) fallback[gw >> 6] = b;
    }
}

// ---- CheckQuorum over active-flag planes (hq_check_quorum_planes_dev) -----------------------
// The leader's own slot always counts (`nid == r.nodeID`, raft.go:384), so a group's CheckQuorum
// state is the active flags of its other voting slots plus its voter count. Plane k < 7 holds the
// active flag of the group's (k + 1)-th voting slot other than the leader, planes 7..9 the bits of
// n - 1 (per-group n); a uniform-n batch keeps only its n - 1 active planes. 2048-group tiles as
// the vote / ReadIndex planes, bit j of dword k of a plane = the tile's group 32 k + j. A lane
// decides 32 groups: 1 + popcount(the active planes masked to the group's slots) >= n/2 + 1,
// then zeroes the active planes it read (setNotActive of every voting member, raft.go:385,
// remote.go:196-198).
template <int P, bool PERN, int BLK>
__global__ __launch_bounds__(BLK) void k_cq_planes(uint64_t G, uint8_t *planes,
                                                   uint64_t *has_quorum) {
    constexpr int NP = PERN ? 10 : P;   // planes per tile
    constexpr int NA = PERN ? 7 : P;    // of which active planes
    const uint64_t lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (BLK / 64) +
                          __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t nw = (uint64_t)gridDim.x * (BLK / 64);
    const uint64_t ntiles = (G + kPlaneTile - 1) / kPlaneTile;
    uint32_t *out = reinterpret_cast<uint32_t *>(has_quorum);
    for (uint64_t t = wave; t < ntiles; t += nw) {
        uint32_t *base = reinterpret_cast<uint32_t *>(planes + t * (uint64_t)NP * (kPlaneTile / 8)) + lane;
        uint32_t p[NP > 0 ? NP : 1];
#pragma unroll
        for (int q = 0; q < NP; ++q) p[q] = __builtin_nontemporal_load(base + q * 64);
        uint32_t x[7] = {0, 0, 0, 0, 0, 0, 0};
        uint32_t h0, h1, h2;                              // n / 2, bit-sliced
        if constexpr (PERN) {
            const uint32_t n0 = p[7], n1 = p[8], n2 = p[9];
            const uint32_t m[7] = {n0 | n1 | n2, n1 | n2, n2 | (n1 & n0), n2, n2 & (n1 | n0),
                                   n2 & n1, n2 & n1 & n0};   // slot k + 1 votes: n - 1 > k
#pragma unroll
            for (int k = 0; k < 7; ++k) x[k] = p[k] & m[k];
            const uint32_t c = n1 & n0;
            h0 = n1 ^ n0;
            h1 = n2 ^ c;
            h2 = n2 & c;
        } else {
#pragma unroll
            for (int k = 0; k < NP; ++k) x[k] = p[k];
            constexpr int h = (P + 1) / 2;
            h0 = (h & 1) ? ~0u : 0u;
            h1 = (h & 2) ? ~0u : 0u;
            h2 = (h & 4) ? ~0u : 0u;
        }
        uint32_t c0, c1, c2;
        count7(x, c0, c1, c2);
        const uint32_t hq = ge3(c0, c1, c2, h0, h1, h2);
        const uint64_t g = t * kPlaneTile + lane * 32;
        if (g < G) {
            const uint64_t left = G - g;
            out[g >> 5] = left >= 32 ? hq : hq & ((1u << left) - 1u);
        } else if (g < ((G + 63) & ~63ull)) {             // the rest of the last bitmap word
            out[g >> 5] = 0;
        }
#pragma unroll
        for (int q = 0; q < NA; ++q) __builtin_nontemporal_store(0u, base + q * 64);
    }
}

// columns -> CheckQuorum planes: one thread per group packs the active flags of its voting slots
// other than self_slot (in slot order) and n - 1, the wave's 64 groups become one ballot per
// plane, lane q < NP stores plane q's 8 bytes
__global__ __launch_bounds__(kBlock) void k_tile_cq_planes(uint64_t G, const uint8_t *active,
                                                           const uint8_t *nv, uint32_t nu,
                                                           uint32_t self_slot, uint8_t *planes,
                                                           uint64_t *fallback) {
    const uint64_t total = (G + kPlaneTile - 1) / kPlaneTile * kPlaneTile;
    const uint32_t NP = nv ? 10u : nu - 1u;
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t g0 = (uint64_t)blockIdx.x * kBlock; g0 < total;
         g0 += (uint64_t)gridDim.x * kBlock) {
        const uint64_t g = g0 + threadIdx.x;
        uint32_t bits = 0;
        bool bad = false;
        if (g < G) {
            const uint32_t n = nv ? nv[g] : nu;
            bad = n < 1 || n > 8 || self_slot >= n;
            if (!bad) {
                const uint32_t a = active[g] & ((1u << n) - 1u);
                bits = (a & ((1u << self_slot) - 1u)) | ((a >> (self_slot + 1)) << self_slot);
                if (nv) bits |= (n - 1) << 7;
            }
        }
        uint64_t mine = 0;
#pragma unroll
        for (uint32_t q = 0; q < 10; ++q) {
            const uint64_t b = __ballot((bits >> q) & 1);
            if (lane == q) mine = b;
        }
        const uint64_t gw = g - lane;
        if (gw < total && lane < NP)
            *reinterpret_cast<uint64_t *>(planes + (gw / kPlaneTile) * (NP * (kPlaneTile / 8)) +
                                          lane * (kPlaneTile / 8) + (gw % kPlaneTile) / 8) = mine;
        const uint64_t b = __ballot(bad);
        if (fallback && lane == 0 && gw < ((G + 63) & ~63ull)) fallback[gw >> 6] = b;
    }
}

template <int MODE>
int launch_bits(hq_ctx *ctx, BitsK &k, const char *what) {
    if (!ctx) return HQ_E_INVAL;
    if (k.G == 0) return HQ_OK;
    if (!k.nv && !(k.tiles && k.tile_rows == 4) && (k.n_uniform < 1 || k.n_uniform > 8))
        return hq::fail(ctx, HQ_E_INVAL, std::string(what) + ": n_uniform must be 1..8");
    if (k.tiles && (k.nv || !hq::aligned16(k.tiles) || (k.tile_rows != 3 && k.tile_rows != 4)))
        return hq::fail(ctx, HQ_E_INVAL, std::string(what) + ": bad tiles");
    const uint8_t *ins[5] = {k.nv, k.ack, k.granted, k.rejected, k.active};
    for (const uint8_t *p : ins)
        if (p && !hq::aligned16(p))
            return hq::fail(ctx, HQ_E_INVAL, std::string(what) + ": byte arrays must be 16-byte aligned");
    k.n16 = hq::words64(k.G) * 4;
    k.n16o = (MODE & kVOTE) ? hq::words32(k.G) * 2 : 0;
    const uint64_t slots = k.n16 > k.n16o ? k.n16 : k.n16o;
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    const dim3 grid(grid_for(ctx, slots)), block(kBlock);
    if (k.tiles) {
        // tiles exist for the fused ReadIndex + vote pass only; rows [n] ack granted rejected
        if constexpr (MODE == (kRI | kVOTE))
            dispatch_bool(k.tile_rows == 4, [&](auto pern) {
                dispatch_bool(k.fallback != nullptr, [&](auto fb) {
                    hipLaunchKernelGGL((k_bits<MODE, decltype(pern)::value, kBlock, true,
                                               decltype(fb)::value>),
                                       grid, block, 0, ctx->stream, k);
                });
            });
    } else {
        dispatch_bool(k.nv != nullptr, [&](auto pern) {
            hipLaunchKernelGGL((k_bits<MODE, decltype(pern)::value, kBlock>), grid, block, 0,
                               ctx->stream, k);
        });
    }
    return hq::post_launch(ctx, what);
}

BitsK bits_args(uint64_t G, const uint8_t *nv, uint32_t nu, uint64_t *fallback) {
    BitsK k{};
    k.G = G;
    k.nv = nv;
    k.n_uniform = nu;
    k.fallback = fallback;
    return k;
}

}  // namespace

extern "C" int hq_readindex_dev(hq_ctx *ctx, uint64_t G, const uint8_t *ack,
                                const uint8_t *n_voting, uint32_t n_uniform, uint64_t *confirmed,
                                uint64_t *fallback) {
    if (ctx && G && (!ack || !confirmed))
        return hq::fail(ctx, HQ_E_INVAL, "hq_readindex: NULL ack/confirmed");
    BitsK k = bits_args(G, n_voting, n_uniform, fallback);
    k.ack = ack;
    k.confirmed = confirmed;
    return launch_bits<kRI>(ctx, k, "hq_readindex");
}

extern "C" int hq_vote_dev(hq_ctx *ctx, uint64_t G, const uint8_t *granted,
                           const uint8_t *rejected, const uint8_t *n_voting, uint32_t n_uniform,
                           uint64_t *outcome, uint64_t *fallback) {
    if (ctx && G && (!granted || !rejected || !outcome))
        return hq::fail(ctx, HQ_E_INVAL, "hq_vote: NULL granted/rejected/outcome");
    BitsK k = bits_args(G, n_voting, n_uniform, fallback);
    k.granted = granted;
    k.rejected = rejected;
    k.outcome = outcome;
    return launch_bits<kVOTE>(ctx, k, "hq_vote");
}

extern "C" int hq_readindex_vote_dev(hq_ctx *ctx, uint64_t G, const uint8_t *ack,
                                     const uint8_t *granted, const uint8_t *rejected,
                                     const uint8_t *n_voting, uint32_t n_uniform,
                                     uint64_t *confirmed, uint64_t *outcome, uint64_t *fallback) {
    if (ctx && G && (!ack || !granted || !rejected || !confirmed || !outcome))
        return hq::fail(ctx, HQ_E_INVAL, "hq_readindex_vote: NULL argument");
    BitsK k = bits_args(G, n_voting, n_uniform, fallback);
    k.ack = ack;
    k.granted = granted;
    k.rejected = rejected;
    k.confirmed = confirmed;
    k.outcome = outcome;
    return launch_bits<kRI | kVOTE>(ctx, k, "hq_readindex_vote");
}

extern "C" int hq_readindex_vote_tiles_dev(hq_ctx *ctx, uint64_t G, const uint8_t *tiles,
                                           uint32_t per_group_n, uint32_t n_uniform,
                                           uint64_t *confirmed, uint64_t *outcome,
                                           uint64_t *fallback) {
    if (ctx && G && (!tiles || !confirmed || !outcome))
        return hq::fail(ctx, HQ_E_INVAL, "hq_readindex_vote_tiles: NULL argument");
    BitsK k = bits_args(G, nullptr, n_uniform, fallback);
    k.tiles = tiles;
    k.tile_rows = per_group_n ? 4 : 3;
    k.confirmed = confirmed;
    k.outcome = outcome;
    return launch_bits<kRI | kVOTE>(ctx, k, "hq_readindex_vote_tiles");
}

extern "C" int hq_readindex_vote_tiles3_dev(hq_ctx *ctx, uint64_t G, const uint8_t *tiles,
                                            uint64_t *confirmed, uint64_t *outcome) {
    if (!ctx) return HQ_E_INVAL;
    if (G == 0) return HQ_OK;
    if (!tiles || !confirmed || !outcome || !hq::aligned16(tiles))
        return hq::fail(ctx, HQ_E_INVAL,
                        "hq_readindex_vote_tiles3: NULL argument or tiles not 16-byte aligned");
    BitsK k = bits_args(G, nullptr, 0, nullptr);
    k.tiles = tiles;
    k.tile_rows = 3;
    k.confirmed = confirmed;
    k.outcome = outcome;
    k.n16 = hq::words64(G) * 4;
    k.n16o = hq::words32(G) * 2;
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    const uint64_t ntiles = (G + 1023) / 1024;
    hipLaunchKernelGGL(k_bits3<256>, dim3(grid_for(ctx, (ntiles + kB3TPW - 1) / kB3TPW * 64, 256)),
                       dim3(256), 0, ctx->stream, k);
    return hq::post_launch(ctx, "hq_readindex_vote_tiles3");
}

extern "C" int hq_readindex_vote_planes_dev(hq_ctx *ctx, uint64_t G, const uint8_t *planes,
                                            uint64_t *confirmed, uint64_t *outcome) {
    if (!ctx) return HQ_E_INVAL;
    if (G == 0) return HQ_OK;
    if (!planes || !confirmed || !outcome || !hq::aligned16(planes))
        return hq::fail(ctx, HQ_E_INVAL,
                        "hq_readindex_vote_planes: NULL argument or planes not 16-byte aligned");
    BitsK k = bits_args(G, nullptr, 0, nullptr);
    k.tiles = planes;
    k.confirmed = confirmed;
    k.outcome = outcome;
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    const uint64_t ntiles = (G + kPlaneTile - 1) / kPlaneTile;
    hipLaunchKernelGGL(k_planes<kPlBlock>,
                       dim3(grid_for(ctx, (ntiles + kPlTPW - 1) / kPlTPW * 64, kPlBlock)),
                       dim3(kPlBlock), 0, ctx->stream, k);
    return hq::post_launch(ctx, "hq_readindex_vote_planes");
}

extern "C" int hq_readindex_vote_cq_planes_dev(hq_ctx *ctx, uint64_t G, const uint8_t *planes,
                                               uint8_t *active_planes, uint64_t *confirmed,
                                               uint64_t *outcome, uint64_t *has_quorum) {
    if (!ctx) return HQ_E_INVAL;
    if (G == 0) return HQ_OK;
    if (!planes || !active_planes || !confirmed || !outcome || !has_quorum ||
        !hq::aligned16(planes) || !hq::aligned16(active_planes))
        return hq::fail(ctx, HQ_E_INVAL,
                        "hq_readindex_vote_cq_planes: NULL argument or planes not 16-byte aligned");
    BitsK k = bits_args(G, nullptr, 0, nullptr);
    k.tiles = planes;
    k.confirmed = confirmed;
    k.outcome = outcome;
    k.has_quorum = has_quorum;
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    const uint64_t ntiles = (G + kPlaneTile - 1) / kPlaneTile;
    hipLaunchKernelGGL(k_planes_cq<kPlBlock>,
                       dim3(grid_for(ctx, (ntiles + kPlCqTPW - 1) / kPlCqTPW * 64, kPlBlock)),
                       dim3(kPlBlock), 0, ctx->stream, k, active_planes);
    return hq::post_launch(ctx, "hq_readindex_vote_cq_planes");
}

extern "C" int hq_tile_planes_dev(hq_ctx *ctx, uint64_t G, const uint8_t *ack,
                                  const uint8_t *granted, const uint8_t *rejected,
                                  const uint8_t *n_voting, uint32_t n_uniform, uint8_t *planes,
                                  uint64_t *fallback) {
    if (!ctx) return HQ_E_INVAL;
    if (G == 0) return HQ_OK;
    if (!ack || !granted || !rejected || !planes || (reinterpret_cast<uintptr_t>(planes) & 7))
        return hq::fail(ctx, HQ_E_INVAL, "hq_tile_planes: NULL argument or planes misaligned");
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tile_planes, dim3(grid_for(ctx, (G + kPlaneTile - 1) / kPlaneTile * kPlaneTile)),
                       dim3(kBlock), 0, ctx->stream, G, n_voting, n_uniform, ack, granted,
                       rejected, planes, fallback);
    return hq::post_launch(ctx, "k_tile_planes");
}

extern "C" int hq_tile_bits3_dev(hq_ctx *ctx, uint64_t G, const uint8_t *ack,
                                 const uint8_t *granted, const uint8_t *rejected,
                                 const uint8_t *n_voting, uint32_t n_uniform, uint8_t *tiles,
                                 uint64_t *fallback) {
    if (!ctx) return HQ_E_INVAL;
    if (G == 0) return HQ_OK;
    if (!ack || !granted || !rejected || !tiles)
        return hq::fail(ctx, HQ_E_INVAL, "hq_tile_bits3: NULL argument");
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tile_bits3, dim3(grid_for(ctx, (G + 1023) / 1024 * 1024)), dim3(kBlock), 0,
                       ctx->stream, G, n_voting, n_uniform, ack, granted, rejected, tiles,
                       fallback);
    return hq::post_launch(ctx, "k_tile_bits3");
}

namespace {
// one lane per 16 groups: 16-byte column loads (guarded at G) into the tile rows (padding zeroed)
__global__ __launch_bounds__(kBlock) void k_tile_bits(uint64_t G, const uint8_t *nv,
                                                      const uint8_t *ack, const uint8_t *gr,
                                                      const uint8_t *rj, uint8_t *tiles,
                                                      uint32_t rows) {
    const uint64_t slots = (G + HQ_BITS_TILE_GROUPS - 1) / HQ_BITS_TILE_GROUPS * (HQ_BITS_TILE_GROUPS / 16);
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < slots;
         t += (uint64_t)gridDim.x * kBlock) {
        const uint64_t g = t * 16;
        uint8_t *row = tiles + (g >> 10) * ((uint64_t)rows << 10) + (g & 1023);
        const uint8_t *cols[4] = {nv, ack, gr, rj};
        for (uint32_t r = 0; r < rows; ++r) {
            const uint8_t *c = cols[r + 4 - rows];
            *reinterpret_cast<uint4 *>(row + (r << 10)) = load16(c, g, G).v;
        }
    }
}
}  // namespace

extern "C" int hq_tile_bits_dev(hq_ctx *ctx, uint64_t G, const uint8_t *ack,
                                const uint8_t *granted, const uint8_t *rejected,
                                const uint8_t *n_voting, uint8_t *tiles) {
    if (!ctx) return HQ_E_INVAL;
    if (G == 0) return HQ_OK;
    if (!ack || !granted || !rejected || !tiles || !hq::aligned16(tiles) || !hq::aligned16(ack) ||
        !hq::aligned16(granted) || !hq::aligned16(rejected) ||
        (n_voting && !hq::aligned16(n_voting)))
        return hq::fail(ctx, HQ_E_INVAL, "hq_tile_bits_dev: NULL or misaligned argument");
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tile_bits, dim3(grid_for(ctx, hq_bits_tiles(G) * (HQ_BITS_TILE_GROUPS / 16))),
                       dim3(kBlock), 0, ctx->stream, G, n_voting, ack, granted, rejected, tiles,
                       n_voting ? 4u : 3u);
    return hq::post_launch(ctx, "k_tile_bits");
}

extern "C" int hq_check_quorum_dev(hq_ctx *ctx, uint64_t G, uint8_t *active,
                                   const uint8_t *n_voting, uint32_t n_uniform,
                                   uint32_t self_slot, uint64_t *has_quorum, uint64_t *fallback) {
    if (ctx && G && (!active || !has_quorum))
        return hq::fail(ctx, HQ_E_INVAL, "hq_check_quorum: NULL active/has_quorum");
    if (ctx && self_slot >= HQ_MAX_VOTERS)
        return hq::fail(ctx, HQ_E_INVAL, "hq_check_quorum: self_slot must be < 8");
    BitsK k = bits_args(G, n_voting, n_uniform, fallback);
    k.active = active;
    k.self_slot = self_slot;
    k.has_quorum = has_quorum;
    return launch_bits<kCHECKQ>(ctx, k, "hq_check_quorum");
}

extern "C" int hq_check_quorum_planes_dev(hq_ctx *ctx, uint64_t G, uint8_t *planes,
                                          uint32_t n_uniform, uint64_t *has_quorum) {
    if (!ctx) return HQ_E_INVAL;
    if (n_uniform > HQ_MAX_VOTERS)
        return hq::fail(ctx, HQ_E_INVAL, "hq_check_quorum_planes: n_uniform must be 0 or 1..8");
    if (G == 0) return HQ_OK;
    if (!has_quorum || (n_uniform != 1 && (!planes || !hq::aligned16(planes))))
        return hq::fail(ctx, HQ_E_INVAL,
                        "hq_check_quorum_planes: NULL argument or planes not 16-byte aligned");
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    constexpr int B = kPlBlock;
    const dim3 grid(grid_for(ctx, (G + kPlaneTile - 1) / kPlaneTile * 64, B));
    // n_uniform 0: per-group n (its planes in the tile); else n - 1 active planes
    dispatch<0, 1, 2, 3, 4, 5, 6, 7, 8>(n_uniform, [&](auto nu) {
        constexpr int n = decltype(nu)::value;
        hipLaunchKernelGGL((k_cq_planes<(n ? n - 1 : 0), n == 0, B>), grid, dim3(B), 0,
                           ctx->stream, G, planes, has_quorum);
    });
    return hq::post_launch(ctx, "hq_check_quorum_planes");
}

extern "C" int hq_tile_cq_planes_dev(hq_ctx *ctx, uint64_t G, const uint8_t *active,
                                     const uint8_t *n_voting, uint32_t n_uniform,
                                     uint32_t self_slot, uint8_t *planes, uint64_t *fallback) {
    if (!ctx) return HQ_E_INVAL;
    if (n_voting ? n_uniform != 0 : (n_uniform < 1 || n_uniform > HQ_MAX_VOTERS))
        return hq::fail(ctx, HQ_E_INVAL,
                        "hq_tile_cq_planes: per-group n_voting with n_uniform 0, or n_uniform 1..8");
    if (!n_voting && self_slot >= n_uniform)
        return hq::fail(ctx, HQ_E_INVAL, "hq_tile_cq_planes: self_slot >= n_uniform");
    if (G == 0) return HQ_OK;
    const bool no_planes = !n_voting && n_uniform == 1;   // a single-node batch has none
    if (!active || (!no_planes && (!planes || (reinterpret_cast<uintptr_t>(planes) & 7))))
        return hq::fail(ctx, HQ_E_INVAL, "hq_tile_cq_planes: NULL argument or planes misaligned");
    int rc = hq::pre_launch(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tile_cq_planes,
                       dim3(grid_for(ctx, (G + kPlaneTile - 1) / kPlaneTile * kPlaneTile)),
                       dim3(kBlock), 0, ctx->stream, G, active, n_voting, n_uniform, self_slot,
                       planes, fallback);
    return hq::post_launch(ctx, "k_tile_cq_planes");
}
