// reas_store.hpp -- the store forms of the reassembly kernels: source-aligned, destination-aligned, LDS-staged.
#pragma once

#include "dev_access.hpp"

namespace e2sar_amd {

// Dwords [lo/4, hi/4) of the register chunk v (lo < hi, both multiples of 4) to dst + lo:
// a payload's first and last 16-byte chunk.  The store instructions a wave issues are what
// its lanes need between them (exec-masked), so a wave holding one edge lane pays every
// form the edge takes: one store of the edge's length (dword, dwordx2 or dwordx3).  (Round
// 3, profiles/round3/s3_edge/: four conditional dword stores per edge -- four store
// instructions per edge wave -- were slower: config 3 scatter 227.6-232.0 vs 225.7-227.7 us.)
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef u32x2 __attribute__((aligned(4))) u32x2_a4;
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
__device__ __forceinline__ void st8(uint8_t *p, uint32_t a, uint32_t b)
{
    *(E2SAR_GLOBAL u32x2_a4 *)(p) = u32x2{a, b};
}
__device__ __forceinline__ void st12(uint8_t *p, uint32_t a, uint32_t b, uint32_t c)
{
    // a 12-byte store (clang widens vec3 stores to 16 bytes, so no C++ form is safe here)
    const u32x3 v{a, b, c};
    // s_nop: the hazard recognizer does not see inside inline asm (a VALU write of the store's
    // data registers right after a >64-bit store needs a wait state)
    asm volatile("global_store_dwordx3 %0, %1, off\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void store_dwords(uint8_t *dst, u32x4 v, uint32_t lo, uint32_t hi)
{
    const u32x4 w = rot_down(v, lo >> 2);
    const uint32_t n = (hi - lo) >> 2;
    uint8_t *p = dst + lo;
    if (n == 3u) st12(p, w.x, w.y, w.z);
    else if (n == 2u) st8(p, w.x, w.y);
    else if (n == 1u) st4(p, w.x);
    else st16u_nt(p, w);
}

__device__ __noinline__ void store_bytes(uint8_t *dst, u32x4 v, uint32_t lo, uint32_t hi)
{
    // bytes [lo, hi) of the 16-byte register chunk v to dst + (lo..hi); rare path
    for (uint32_t b = lo; b < hi; b++) st1(dst + b, (uint8_t)(v[b >> 2] >> (8u * (b & 3u))));
}

// Store the payload part of datagram chunk c (bytes [16c, 16c+16) of the slot) to its
// place in the event: whole 16-byte stores inside the payload, whole dwords at the two
// edges, bytes only for a sub-dword event tail or a non dword-congruent datagram.
__device__ __forceinline__ void scatter_chunk(const PktInfo pi, uint32_t c, u32x4 v)
{
    if (pi.plen == 0) return;
    // datagram bytes [16c, 16c+16) against the payload [hl, hl+plen)
    const uint32_t q0 = 16u * c;
    const uint32_t pend = pi.hl + pi.plen;
    if (q0 >= pend || q0 + 16u <= pi.hl) return;
    const uint32_t lo = (q0 < pi.hl) ? pi.hl - q0 : 0u;             // first chunk byte to keep
    const uint32_t hi = (q0 + 16u <= pend) ? 16u : pend - q0;        // one past the last
    uint8_t *dst = reinterpret_cast<uint8_t *>(pi.dst) + q0 - pi.hl;  // where chunk byte 0 goes
    const bool congruent = ((pi.dst - pi.hl) & 3u) == 0;
    if (lo == 0 && hi == 16u && congruent) {
        st16u_nt(dst, v);
    } else if (congruent) {
        const uint32_t l4 = (lo + 3u) & ~3u, t = hi & ~3u;         // lo is a multiple of 4 here
        if (l4 < t) store_dwords(dst, v, l4, t);
        if (t < hi && t >= lo) store_bytes(dst, v, t, hi);         // sub-dword event tail
    } else {
        store_bytes(dst, v, lo, hi);
    }
}

__device__ __forceinline__ PktInfo ld_info(const PktInfo *p)
{
    const u32x4 v = *(const E2SAR_GLOBAL u32x4 *)(p);
    PktInfo r;
    r.dst = ((uint64_t)v.y << 32) | v.x;
    r.plen = v.z;
    r.hl = v.w;
    return r;
}
// ... and its packing, in one 16-byte store; hlFlags: flag bits or-ed into hl (kPktCompletes)
__device__ __forceinline__ void st_info(PktInfo *p, const PktInfo &pi, uint32_t hlFlags = 0)
{
    st16(reinterpret_cast<uint8_t *>(p), u32x4{(uint32_t)pi.dst, (uint32_t)(pi.dst >> 32), pi.plen, pi.hl | hlFlags});
}

// Destination-aligned form of the same copy: chunk c of a payload whose phase in its event
// buffer is a (= bufferOffset mod 16; event buffers are 256-byte aligned in a 256-byte
// aligned arena) covers event bytes [(dst & ~15) + 16c, +16), i.e. datagram bytes from
// r = hl + 16c - a -- a multiple of 4 for a dword-congruent payload, so one dword-aligned
// 16-byte load, slid back by sh inside the slot at its end and shifted down in registers,
// feeds one aligned 16-byte store.
__device__ __forceinline__ uint32_t da_window(uint32_t c, uint32_t a, uint32_t hl, uint32_t stride, uint32_t &sh)
{
    const uint32_t r = hl + 16u * c - a;
    sh = (r + 16u > stride) ? r + 16u - stride : 0u;
    return r - sh;
}

// The part of destination-aligned 16-byte block c that a payload of plen bytes at phase a
// (= dst mod 16) covers: bytes [lo, hi) of the block.  lo > 0 only in the payload's first
// block, hi < 16 only in its last; bytes [edge_tail(hi), hi) are a sub-dword event tail.
__device__ __forceinline__ void edge_span(uint32_t c, uint32_t a, uint32_t plen, uint32_t &lo, uint32_t &hi)
{
    lo = (c == 0u) ? a : 0u;
    hi = (a + plen - 16u * c < 16u) ? a + plen - 16u * c : 16u;
}
__device__ __forceinline__ uint32_t edge_tail(uint32_t hi) { return hi & ~3u; }

// Store destination-aligned chunk c (loaded from the window of da_window) of the datagram
// at dgram: whole aligned 16-byte stores inside the payload, dwords at its two edges,
// bytes for a sub-dword event tail, byte copies for a payload that is not dword-congruent.
template <bool HO = false>
__device__ __forceinline__ void da_store(const PktInfo pi, uint32_t c, u32x4 x, const uint8_t *dgram, uint32_t stride)
{
    const uint32_t a = (uint32_t)pi.dst & 15u;
    if (pi.plen == 0u || 16u * c >= a + pi.plen) return;          // dropped, or past the payload
    uint8_t *D = reinterpret_cast<uint8_t *>((pi.dst & ~15ull) + 16ull * c);
    uint32_t lo, hi;
    edge_span(c, a, pi.plen, lo, hi);
    if ((a & 3u) == 0u) {
        uint32_t sh;
        (void)da_window(c, a, pi.hl, stride, sh);
        const u32x4 o = rot_down(x, sh >> 2);
        if (lo == 0u && hi == 16u) {
            st16_nt(D, o);
        } else {
            const uint32_t t = edge_tail(hi);                          // lo = a is a multiple of 4
            if (lo < t) store_dwords(D, o, lo, t);
            if (t < hi && t >= lo) store_bytes(D, o, t, hi);           // sub-dword event tail
        }
    } else {
        const uint8_t *s = dgram + pi.hl + 16u * c - a;                // + lo >= hl
        for (uint32_t b = lo; b < hi; b++) st1(D + b, HO ? ld1_sc1(s + b) : ld1(s + b));
    }
}

// Scatter stores: source-aligned chunks, staged through LDS into aligned stores
// (lds_stage_store) where scatter_stage() picks it, else stored at their misaligned
// destination (scatter_chunk).  (Round 3 measured destination-aligned stores built from
// neighbour-lane funnel shifts, or from every lane loading its chunk pair: cold leg 2221 /
// 2020 vs 2369 GiB/s -- what the aligned stores save the extra loads cost)

// Staged scatter (STAGE, chosen per launch by scatter_stage()): the one-round group's
// source-aligned chunks go through LDS.  Every dword of a payload is written to its destination phase in the group's LDS
// copy of the slot (datagram p at p * (stride + 16), payload byte t at a + t, a = dst mod
// 16), then after an LDS barrier every 16-byte event block is read back aligned and stored
// aligned: the loads need nothing from the work records, the stores are whole aligned
// 16-byte stores except at the payload's two edges.  A payload that is not dword-congruent
// with its destination (never at dword-multiple maxPld) is stored from registers as before.
template <int U, int TB>
__device__ __forceinline__ void lds_stage_store(const PktInfo *sinfo, const u32x4 (&x)[U], const uint32_t (&pp)[U],
                                                const uint32_t (&cc)[U], uint32_t nch, uint32_t gn, uint32_t stride)
{
    // one round of the group's slots (<= 256 * U chunks) plus 16 bytes of phase per datagram
    __shared__ uint32_t stage[(16u * TB * U + 64u * 16u) / 4u];
    const uint32_t ps = stride + 16u;                                  // LDS bytes per datagram
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t i = (uint32_t)u * TB + threadIdx.x;
        if (i >= nch) continue;
        const PktInfo pi = sinfo[pp[u]];
        if (pi.plen == 0u) continue;
        const uint32_t a = (uint32_t)pi.dst & 15u;
        if (((a - pi.hl) & 3u) != 0u) {                                // not dword-congruent
            scatter_chunk(pi, cc[u], x[u]);
            continue;
        }
        const uint32_t base = pp[u] * ps + a - pi.hl;                  // + slot byte offset
#pragma unroll
        for (uint32_t d = 0; d < 4; d++) {
            const uint32_t s = 16u * cc[u] + 4u * d;
            if (s >= pi.hl && s < pi.hl + pi.plen) stage[(base + s) >> 2] = x[u][d];
        }
    }
    lds_barrier();
    const uint32_t nbp = ps >> 4;                                      // 16-byte blocks per datagram
    const uint32_t total = gn * nbp;
    for (uint32_t k = threadIdx.x; k < total; k += TB) {
        const uint32_t p = k / nbp, b = k - p * nbp;
        const PktInfo pi = sinfo[p];
        if (pi.plen == 0u) continue;
        const uint32_t a = (uint32_t)pi.dst & 15u;
        if (((a - pi.hl) & 3u) != 0u || 16u * b >= a + pi.plen) continue;
        const uint32_t q = (p * ps + 16u * b) >> 2;
        const u32x4 o{stage[q], stage[q + 1], stage[q + 2], stage[q + 3]};
        uint8_t *D = reinterpret_cast<uint8_t *>((pi.dst & ~15ull) + 16ull * b);
        uint32_t lo, hi;
        edge_span(b, a, pi.plen, lo, hi);
        if (lo == 0u && hi == 16u) {
            st16_nt(D, o);
            continue;
        }
#pragma unroll
        for (uint32_t d = 0; d < 4; d++)
            if (4u * d >= lo && 4u * d + 4u <= hi) st4(D + 4u * d, o[d]);
        const uint32_t t = edge_tail(hi);                              // sub-dword event tail
        if (t < hi && t >= lo) store_bytes(D, o, t, hi);
    }
}

}  // namespace e2sar_amd
