// seg_device.hpp -- segmentation: event batch -> datagram batch (seg_kernel).
#pragma once

#include "dev_access.hpp"
#include "reas_table.hpp"
#include "wire.hpp"

namespace e2sar_amd {

// ---------------------------------------------------------------------------------
// segmentation

// Payload dword at byte offset r (a multiple of 4) of a datagram payload of L bytes,
// zero past L.  Reads only the dword that holds byte r, never the next one.
__device__ __forceinline__ uint32_t pl_dword(const uint8_t *pl, uint32_t r, uint32_t L)
{
    if (r >= L) return 0u;
    const uint32_t w = ld4(pl + r);
    return (r + 4u > L) ? (w & low_bytes_mask(L - r)) : w;
}

// Header dword i (0..8) of the datagram; w5 (bufferOffset) is the only per-datagram word.
struct SegHdr {
    uint32_t w0, w1, w2, w3, w4, w6, w7, w8;
};

__device__ __forceinline__ uint32_t seg_hdr_byte(const SegHdr &h, uint32_t w5, uint32_t q)
{
    const uint32_t i = q >> 2;
    uint32_t w = h.w0;
    w = (i == 1) ? h.w1 : w;
    w = (i == 2) ? h.w2 : w;
    w = (i == 3) ? h.w3 : w;
    w = (i == 4) ? h.w4 : w;
    w = (i == 5) ? w5 : w;
    w = (i == 6) ? h.w6 : w;
    w = (i == 7) ? h.w7 : w;
    w = (i == 8) ? h.w8 : w;
    return (w >> (8u * (q & 3u))) & 0xFFu;
}

// Generic case (event not dword-aligned, or maxPldLen % 4 != 0): byte loads.
__device__ __forceinline__ u32x4 seg_chunk_bytes(const SegHdr &h, uint32_t w5, const uint8_t *pl,
                                                 uint32_t L, uint32_t c)
{
    uint32_t o[4];
#pragma unroll
    for (uint32_t d = 0; d < 4; d++) {
        uint32_t w = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; b++) {
            const uint32_t q = 16u * c + 4u * d + b;
            uint32_t byte = 0;
            if (q < kLBREHdrLen) byte = seg_hdr_byte(h, w5, q);
            else if (q - kLBREHdrLen < L) byte = ld1(pl + (q - kLBREHdrLen));
            w |= byte << (8u * b);
        }
        o[d] = w;
    }
    u32x4 v;
    v.x = o[0];
    v.y = o[1];
    v.z = o[2];
    v.w = o[3];
    return v;
}

// grid.x = nEvents * blocksPerEvent; each block owns kBlock*U consecutive 16-byte
// chunks of ONE event's datagram range (event-major: every event field is a scalar).
// Datagram k of the event sits at pkts + (pktBase + k) * stride, so chunk j of the
// event lands at pkts + pktBase*stride + 16*j: the stores of a block are one contiguous
// run of memory.
//
// Chunk c of a datagram with payload pl[0, L): c = 0, 1 are LB / RE header words, c = 2
// is the RE eventNum low word + payload 0..11, c >= 3 is payload [16c-36, 16c-20).
// Every lane issues exactly one unconditional 16-byte load per chunk (phase 1) -- the
// window is slid back so it never leaves the event (a tail chunk reads the 16 bytes
// that END at its last dword, then shifts them down in registers) -- and only phase 2
// consumes them.  So no load result sits behind a branch and all U loads of a lane are
// in flight together.
// dCount (optional): the number of events is read on the device (the relay form, whose
// event table is built by relay_plan_kernel); blocks of events past it exit.
// The dword fast path (16-byte loads at dword alignment) is chosen per event from the
// event's own address and maxPld: a block handles one event, so the choice is uniform.
//
// HO (the chained form, segreas_kernel): every datagram byte and length is stored sc1 and,
// once the block's stores are done, the block adds the number of index-space chunks it
// covered in each reassembly group's range of datagrams to that group's counter
// (tiles[slot / tileG]); a group starts when its counter reaches its slots x stride/16.
constexpr int kSegBlock = 256;       // seg_kernel threads per workgroup (128 / 512 lost)
// seg_kernel<4> (16-KiB workgroups, events of more than 4 MiB of datagrams) at most 6
// workgroups per CU: config 3's segmentation 180.0-181.4 vs 185.3 us; seg_kernel<2> loses
// with any cap (7 / 6 / 5 per CU: 67.4-68.2 / 71.3-72.3 / 76.6-77.9 vs 67.7-70.0 us at 1 MiB;
// profiles/round4/ab/seg_occupancy.log)
constexpr uint32_t kSeg4PerCU = 6;
// One round of a segmentation block: index-space chunks [j0, j0 + SB*U) of event ev,
// bounded by jEnd (the event's chunk count, or the end of a local chained range).  `out` and
// outR address chunk outJ0, so every store offset is 16 * (j - outJ0), below 2^32.
struct SegEv {
    SegHdr h;
    const uint8_t *data;
    uint32_t pktBase, bytes, npk, spc, maxPld;
    float rspc;
    bool A4;
};

__device__ __forceinline__ SegEv seg_ev(const e2sar_hip_seg_event &ev, int lbVersion, uint32_t maxPld, uint32_t stride)
{
    HdrWords hw;
    lbre_words(hw, lbVersion, ev.entropy, ev.lbTick, ev.dataId, 0u, ev.bytes, ev.eventNum);
    SegEv E;
    E.h = SegHdr{hw.w[0], hw.w[1], hw.w[2], hw.w[3], hw.w[4], hw.w[6], hw.w[7], hw.w[8]};
    E.data = ev.data;
    E.pktBase = ev.pktBase;
    E.bytes = ev.bytes;
    E.npk = ev.bytes / maxPld + (ev.bytes % maxPld != 0u);     // bytes + maxPld - 1 wraps near 4 GiB
    E.spc = stride >> 4;
    E.maxPld = maxPld;
    E.rspc = 1.0f / (float)E.spc;
    E.A4 = (((uintptr_t)ev.data | maxPld) & 3u) == 0u;
    return E;
}

template <int U, bool HO, int SB>
__device__ __forceinline__ void seg_round(const SegEv &E, uint8_t *__restrict__ out, __amdgpu_buffer_rsrc_t outR,
                                          uint32_t outJ0, const uint8_t *safe, uint32_t *__restrict__ lens,
                                          uint32_t j0, uint32_t jEnd)
{
    const SegHdr h = E.h;        // a copy: a reference into E leaves E in scratch memory
    const uint32_t bytes = E.bytes, npk = E.npk, spc = E.spc, maxPld = E.maxPld;
    const bool A4 = E.A4;
    const float rspc = E.rspc;
    u32x4 x[U];
    uint32_t jj[U], cc[U], LL[U], kk[U], sh[U];
    bool rare[U];
    // ---- phase 1: one load per chunk ----
#pragma unroll
    for (int u = 0; u < U; u++) {
        const uint32_t j = j0 + (uint32_t)u * SB + threadIdx.x;
        jj[u] = 0xFFFFFFFFu;
        cc[u] = LL[u] = kk[u] = sh[u] = 0;
        rare[u] = false;
        const uint8_t *a = safe;
        if (j < jEnd) {
            // k = j / spc: a float reciprocal and a +-1 correction while k < 2^22 (the
            // estimate is then off by less than one); integer division for the datagrams of
            // larger events (npk is event-uniform, so the branch never diverges)
            const uint32_t k = (npk < (1u << 22)) ? div_recip(j, spc, rspc) : j / spc;
            const uint32_t c = j - k * spc;
            const uint32_t off = k * maxPld;
            const uint32_t L = (bytes - off > maxPld) ? maxPld : bytes - off;
            if (c == 0u && lens) {
                if (HO) st4_sc1(lens + E.pktBase + k, kLBREHdrLen + L);
                else lens[E.pktBase + k] = kLBREHdrLen + L;
            }
            if (16u * c < kLBREHdrLen + L) {          // else: chunk wholly past the datagram end
                jj[u] = j;
                cc[u] = c;
                LL[u] = L;
                kk[u] = k;
                const uint8_t *pl = E.data + off;
                if (!A4) {
                    rare[u] = true;
                } else if (c >= 3u) {
                    const uint32_t r = 16u * c - kLBREHdrLen;
                    const uint32_t n = (L - r < 16u) ? L - r : 16u;
                    const uint32_t rn = (n + 3u) & ~3u;
                    sh[u] = (16u - rn) >> 2;
                    a = pl + (r + rn - 16u);
                } else if (c == 2u) {
                    if (k > 0u && L >= 12u) a = pl - 4;       // previous datagram's last payload dword
                    else rare[u] = true;                      // event start / tiny datagram
                }
            }
        }
        x[u] = ld16_nt(a);
    }
    // ---- phase 2: header words, shifts, tail masks, stores ----
#pragma unroll
    for (int u = 0; u < U; u++) {
        if (jj[u] == 0xFFFFFFFFu) continue;
        const uint32_t c = cc[u], L = LL[u];
        const uint32_t w5 = bswap32(kk[u] * maxPld);
        const uint8_t *pl = E.data + kk[u] * maxPld;
        u32x4 o;
        if (rare[u]) {
            if (!A4) {
                o = seg_chunk_bytes(h, w5, pl, L, c);
            } else {        // c == 2 at an event start or in a datagram of < 12 payload bytes
                o.x = h.w8;
                o.y = pl_dword(pl, 0u, L);
                o.z = pl_dword(pl, 4u, L);
                o.w = pl_dword(pl, 8u, L);
            }
        } else if (c >= 3u) {
            const uint32_t r = 16u * c - kLBREHdrLen;
            o = rot_down(x[u], sh[u]);
            if (L - r < 16u) o = keep_low_bytes(o, L - r);
        } else if (c == 2u) {
            o = x[u];
            o.x = h.w8;
        } else if (c == 1u) {
            o = u32x4{h.w4, w5, h.w6, h.w7};
        } else {
            o = u32x4{h.w0, h.w1, h.w2, h.w3};
        }
        // plain stores: the batch stays in the Infinity Cache for the reassembly that reads it
        // next (nt stores: reas_kernel 97.8 vs 74 us, round 3)
        if (HO) st16_sc1(outR, 16u * (jj[u] - outJ0), o);
        else st16(out + 16u * (jj[u] - outJ0), o);
    }
}

// Unit bx (SB * U consecutive chunks) of event e: what a segmentation workgroup does once it
// knows its place, whether that came from an event-major grid (seg_block) or from a search
// over a unit prefix (seg_flat_kernel, seg_emit.hpp).
template <int U, bool HO, int SB = kBlock>
__device__ __forceinline__ void seg_unit(const e2sar_hip_seg_event *__restrict__ events, uint32_t e, uint32_t bx,
                                         int lbVersion, uint32_t maxPld, uint8_t *__restrict__ pkts, uint32_t stride,
                                         uint32_t *__restrict__ lens, uint32_t tileG, uint32_t *__restrict__ tiles)
{
    const e2sar_hip_seg_event ev = events[e];
    const SegEv E = seg_ev(ev, lbVersion, maxPld, stride);
    const uint32_t spc = E.spc;
    const uint32_t nch = E.npk * spc;
    const uint32_t j0 = bx * (uint32_t)(SB * U);
    if (j0 >= nch) return;

    // the block's first chunk: an event of more than 2^28 chunks (4 GiB of slots) puts 16 * j
    // past 32 bits, so the 64-bit part of the address is added here, once per block
    uint8_t *const out = pkts + (uint64_t)ev.pktBase * stride + 16ull * j0;
    const __amdgpu_buffer_rsrc_t outR = brsrc(out);                     // HO stores only
    const uint8_t *const safe = reinterpret_cast<const uint8_t *>(events + e);   // >= 16 valid bytes
    seg_round<U, HO, SB>(E, out, outR, j0, safe, lens, j0, nch);
    if (HO) {
        // every storing wave waits for its write-through stores, then one wave signals for
        // the workgroup behind the barrier
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x < 64) {
            const uint32_t j1 = (j0 + (uint32_t)(SB * U) < nch) ? j0 + (uint32_t)(SB * U) : nch;
            const uint64_t s0 = (uint64_t)ev.pktBase + j0 / spc, s1 = (uint64_t)ev.pktBase + (j1 - 1u) / spc;
            const uint64_t t0 = s0 / tileG, t1 = s1 / tileG;
            for (uint64_t t = t0 + (threadIdx.x & 63u); t <= t1; t += 64u) {
                const uint64_t tlo = t * tileG, thi = tlo + tileG;        // slots of group t
                const uint64_t clo = (tlo > ev.pktBase) ? (tlo - ev.pktBase) * spc : 0u;
                const uint64_t chi = (thi - ev.pktBase) * spc;            // thi > s0 >= pktBase
                const uint64_t lo = clo > j0 ? clo : j0, hi = chi < j1 ? chi : j1;
                __hip_atomic_fetch_add(tiles + t, (uint32_t)(hi - lo), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
#if E2SAR_TRACE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    TRACE_AT(1, 2, trace_hwid());
    TRACE_AT(1, 3, trace_now());
#endif
}

template <int U, bool HO, int SB = kBlock>
__device__ __forceinline__ void seg_block(const e2sar_hip_seg_event *__restrict__ events, uint32_t blocksPerEvent,
                                          int lbVersion, uint32_t maxPld, uint8_t *__restrict__ pkts, uint32_t stride,
                                          uint32_t *__restrict__ lens, const uint32_t *__restrict__ dCount,
                                          uint32_t blk, uint32_t tileG, uint32_t *__restrict__ tiles)
{
    TRACE_AT(1, 0, trace_now());
    const uint32_t e = blk / blocksPerEvent;
    const uint32_t bx = blk - e * blocksPerEvent;
    if (dCount && e >= *dCount) return;
    seg_unit<U, HO, SB>(events, e, bx, lbVersion, maxPld, pkts, stride, lens, tileG, tiles);
}

// stripe > 0 (XCD stripes): the dispatcher hands workgroup b to XCD b mod 8 (round robin,
// checked by tools/ubench_l2keep.hip), and workgroup b = 8k + x takes unit
// ((k / stripe) * 8 + x) * stripe + k % stripe, so units [m * stripe, (m + 1) * stripe) --
// a stripe of consecutive datagrams -- are all written on XCD m mod 8.  A reassembly
// launched with the matching group table (seg_groups) then reads every stripe on the XCD
// that wrote it, which reads measurably faster than lines another XCD wrote, also from
// the Infinity Cache.  Units are numbered e * blocksPerEvent + bx as
// without stripes; units past nUnits exit.
//
// recMode != 0 (e2sar_hip_segment_batch_recycle): workgroups from nSegBlocks on recycle the
// reassembler `rec` (reas_recycle_kernel's work; 2 = also drop completed records) instead of
// segmenting.  They run at the end of the launch, in the slots the last seg blocks free; no
// seg block touches the table, and the reassembly that used it ran before this launch.
template <int U>
__global__ __launch_bounds__(kSegBlock) void seg_kernel(const e2sar_hip_seg_event *__restrict__ events,
                                                              uint32_t blocksPerEvent, int lbVersion,
                                                              uint32_t maxPld, uint8_t *__restrict__ pkts,
                                                              uint32_t stride, uint32_t *__restrict__ lens,
                                                              const uint32_t *__restrict__ dCount, uint32_t stripe,
                                                              uint32_t nUnits, ReasDev rec, uint32_t nSegBlocks,
                                                              int recMode)
{
    uint32_t blk = blockIdx.x;
    if (recMode && blk >= nSegBlocks) {
        recycle_slots(rec, (blk - nSegBlocks) * kSegBlock + threadIdx.x, recMode == 2);
        return;
    }
    if (stripe) {
        const uint32_t x = blk & 7u, k = blk >> 3;
        blk = ((k / stripe) * 8u + x) * stripe + k % stripe;
        if (blk >= nUnits) return;
    }
    seg_block<U, false, kSegBlock>(events, blocksPerEvent, lbVersion, maxPld, pkts, stride, lens, dCount,
                                         blk, 1u, nullptr);
}

}  // namespace e2sar_amd
