// route.hpp -- multi-GPU routing of a landed datagram batch: the route_* kernels.
#pragma once

#include "dev_access.hpp"
#include "wire.hpp"

namespace e2sar_amd {

// ---------------------------------------------------------------------------------
// multi-GPU: route a landed datagram batch to the rank that owns each event
//
// owner(eventNum) = eventNum % world.  Datagrams that cannot be parsed stay
// on this rank (so their badHeaderDiscards are counted where they landed).  The packing
// is stable: datagrams keep their landing order inside each destination's span, so an
// in-order stream stays in order after the exchange.

constexpr uint32_t kMaxWorld = 64;

__device__ __forceinline__ uint32_t route_dest(const uint8_t *pkts, uint32_t stride, const uint32_t *lens,
                                               uint32_t p, int withLB, uint32_t world, uint32_t self)
{
    const uint32_t hl = withLB ? kLBREHdrLen : kREHdrLen;
    const uint32_t len = lens[p];
    if (len < hl || len > stride) return self;
    const uint8_t *re = pkts + (uint64_t)p * stride + (withLB ? kLBHdrLen : 0u);
    const u32x4 w = ld16(re);
    if (!re_valid(w.x)) return self;
    const uint64_t ev = ((uint64_t)bswap32(w.w) << 32) | bswap32(ld4(re + 16));
    return (uint32_t)(ev % world);
}

constexpr uint32_t kNoDest = 0xFFFFFFFFu;

// Destination of datagram p, or kNoDest past the batch and -- foreign-only routing
// (excludeSelf) -- for every datagram that stays here (owned here, or unparsable): those
// are reassembled where they landed by a reassembler set to this rank's ownership.
__device__ __forceinline__ uint32_t route_dest_x(const uint8_t *pkts, uint32_t stride, const uint32_t *lens,
                                                 uint32_t p, uint32_t n, int withLB, uint32_t world, uint32_t self,
                                                 int excludeSelf)
{
    if (p >= n) return kNoDest;
    const uint32_t d = route_dest(pkts, stride, lens, p, withLB, world, self);
    return (excludeSelf && d == self) ? kNoDest : d;
}

// per-block, per-destination counts (wave ballots, deterministic)
__global__ __launch_bounds__(kBlock) void route_hist_kernel(const uint8_t *__restrict__ pkts, uint32_t stride,
                                                            const uint32_t *__restrict__ lens, uint32_t n, int withLB,
                                                            uint32_t world, uint32_t self, int excludeSelf,
                                                            uint32_t *__restrict__ blockHist)
{
    __shared__ uint32_t cnt[kMaxWorld];
    for (uint32_t d = threadIdx.x; d < world; d += kBlock) cnt[d] = 0;
    __syncthreads();
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t dest = route_dest_x(pkts, stride, lens, p, n, withLB, world, self, excludeSelf);
    for (uint32_t d = 0; d < world; d++) {
        const uint64_t m = __ballot(dest == d);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt[d], (uint32_t)__builtin_popcountll(m));
    }
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < world; d += kBlock) blockHist[(uint64_t)blockIdx.x * world + d] = cnt[d];
}

// one block: exclusive scans -> per-block bases, per-destination counts and bases.
// For each destination the nBlocks counts are scanned 256 at a time (block_excl_scan, a
// running carry between tiles), so the scan costs nBlocks/256 block steps per destination
// instead of nBlocks dependent loads.
__global__ __launch_bounds__(kBlock) void route_scan_kernel(uint32_t *__restrict__ blockHist, uint32_t nBlocks,
                                                            uint32_t world, uint32_t *__restrict__ counts,
                                                            uint32_t *__restrict__ destBase)
{
    __shared__ uint32_t waveSum[kBlock / 64];
    __shared__ uint32_t tot[kMaxWorld];
    for (uint32_t d = 0; d < world; d++) {
        uint32_t carry = 0;
        for (uint32_t b0 = 0; b0 < nBlocks; b0 += kBlock) {
            const uint32_t b = b0 + threadIdx.x;
            const uint32_t c = (b < nBlocks) ? blockHist[(uint64_t)b * world + d] : 0u;
            uint32_t tile;
            const uint32_t before = block_excl_scan<uint32_t, kBlock / 64>(c, waveSum, tile);
            if (b < nBlocks) blockHist[(uint64_t)b * world + d] = carry + before;
            carry += tile;
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            tot[d] = carry;
            if (counts) counts[d] = carry;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t d = 0; d < world; d++) {
            destBase[d] = run;
            run += tot[d];
        }
    }
}

// copy every datagram slot (stride bytes) to its place in the send buffer.  Workgroup
// (g, s) = blockIdx (g * kPackSplit + s) recomputes the places of datagrams [256g, 256g+256)
// (header reads that hit in L2) and copies the s-th of kPackSplit slices of their chunks.
// A/B at 205 x 1 MiB, MTU 1500, spread landing (route = hist + scan + pack, per batch):
// split 1/2/4/8 -> 97/92/100/116 us with non-temporal datagram loads, which also leave the
// Infinity Cache to the packed copy that reassembly reads next (reas 108 -> 79 us).
constexpr uint32_t kPackSplit = 2;
__global__ __launch_bounds__(kBlock) void route_pack_kernel(const uint8_t *__restrict__ pkts, uint32_t stride,
                                                            const uint32_t *__restrict__ lens, uint32_t n, int withLB,
                                                            uint32_t world, uint32_t self, int excludeSelf,
                                                            const uint32_t *__restrict__ blockBase,
                                                            const uint32_t *__restrict__ destBase,
                                                            uint8_t *__restrict__ out, uint32_t *__restrict__ outLens)
{
    __shared__ uint32_t pos[kBlock];
    __shared__ uint32_t waveCnt[kBlock / 64][kMaxWorld];
    const uint32_t g = blockIdx.x / kPackSplit, sl = blockIdx.x % kPackSplit;
    const uint32_t p = g * kBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t dest = route_dest_x(pkts, stride, lens, p, n, withLB, world, self, excludeSelf);
    uint32_t rank = 0;
    for (uint32_t d = 0; d < world; d++) {
        const uint64_t m = __ballot(dest == d);
        if (dest == d) rank = (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (lane == 0) waveCnt[wv][d] = (uint32_t)__builtin_popcountll(m);
    }
    __syncthreads();
    pos[threadIdx.x] = kNoDest;
    if (dest != kNoDest) {
        uint32_t before = 0;
        for (uint32_t w = 0; w < wv; w++) before += waveCnt[w][dest];
        const uint32_t q = destBase[dest] + blockBase[(uint64_t)g * world + dest] + before + rank;
        pos[threadIdx.x] = q;
        if (sl == 0) outLens[q] = lens[p];
    }
    // foreign-only routing leaves most blocks with nothing to move at small world sizes
    if (!__syncthreads_or(dest != kNoDest)) return;
    const uint32_t p0 = g * kBlock;
    const uint32_t np = (n - p0 < kBlock) ? n - p0 : kBlock;
    const uint32_t spc = stride >> 4;
    const uint32_t nch = np * spc;
    const float rspc = 1.0f / (float)spc;
    // this workgroup's slice of the chunks, in two-phase rounds of 4 chunks per thread
    const uint32_t c0 = (uint32_t)((uint64_t)nch * sl / kPackSplit);
    const uint32_t c1 = (uint32_t)((uint64_t)nch * (sl + 1) / kPackSplit);
    constexpr int UR = 4;
    for (uint32_t r0 = c0; r0 < c1; r0 += kBlock * UR) {
        u32x4 x[UR];
        uint32_t qq[UR], cc[UR];
#pragma unroll
        for (int u = 0; u < UR; u++) {
            const uint32_t i = r0 + (uint32_t)u * kBlock + threadIdx.x;
            const uint32_t ic = (i < c1) ? i : c0;
            const uint32_t k = div_recip(ic, spc, rspc);
            cc[u] = ic - k * spc;
            qq[u] = (i < c1) ? pos[k] : kNoDest;                       // kNoDest: stays here
            x[u] = u32x4{0u, 0u, 0u, 0u};
            if (qq[u] != kNoDest)
                x[u] = ld16_nt(pkts + (uint64_t)(p0 + k) * stride + 16u * cc[u]);
        }
#pragma unroll
        for (int u = 0; u < UR; u++) {
            if (qq[u] != kNoDest) {
                uint8_t *o = out + (uint64_t)qq[u] * stride + 16u * cc[u];
                st16(o, x[u]);
            }
        }
    }
}

// Append routing in ONE launch (e2sar_hip_route_append): a workgroup of 256 datagrams counts
// its datagrams per destination (wave ballots), reserves room in each destination's region
// with one atomicAdd on that region's counter, and copies its datagrams there -- no
// histogram / scan launches in front of the copy (three dependent launches cost ~20 us per
// batch even when nothing is foreign).  Within a workgroup a destination's datagrams keep
// their order; workgroups append in the order they reserve.
__global__ __launch_bounds__(kBlock) void route_append_kernel(const uint8_t *__restrict__ pkts, uint32_t stride,
                                                              const uint32_t *__restrict__ lens, uint32_t n, int withLB,
                                                              uint32_t world, uint32_t self, int excludeSelf, uint32_t cap,
                                                              uint32_t *__restrict__ running, uint8_t *__restrict__ out,
                                                              uint32_t *__restrict__ outLens)
{
    __shared__ uint32_t pos[kBlock];
    __shared__ uint32_t waveCnt[kBlock / 64][kMaxWorld];
    __shared__ uint32_t base[kMaxWorld];
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t dest = route_dest_x(pkts, stride, lens, p, n, withLB, world, self, excludeSelf);
    uint32_t rank = 0;
    for (uint32_t d = 0; d < world; d++) {
        const uint64_t m = __ballot(dest == d);
        if (dest == d) rank = (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
        if (lane == 0) waveCnt[wv][d] = (uint32_t)__builtin_popcountll(m);
    }
    __syncthreads();
    if (threadIdx.x < world) {
        uint32_t tot = 0;
        for (uint32_t w = 0; w < kBlock / 64; w++) tot += waveCnt[w][threadIdx.x];
        base[threadIdx.x] = tot ? atomicAdd(&running[threadIdx.x], tot) : 0u;
    }
    __syncthreads();
    uint32_t q = kNoDest;
    if (dest != kNoDest) {
        uint32_t before = 0;
        for (uint32_t w = 0; w < wv; w++) before += waveCnt[w][dest];
        const uint32_t r = base[dest] + before + rank;
        if (r < cap) {                                        // nothing past the region; running still counts it
            q = dest * cap + r;
            outLens[q] = lens[p];
        }
    }
    pos[threadIdx.x] = q;
    if (!__syncthreads_or(q != kNoDest)) return;
    const uint32_t p0 = blockIdx.x * kBlock;
    const uint32_t np = (n - p0 < kBlock) ? n - p0 : kBlock;
    const uint32_t spc = stride >> 4;
    const uint32_t nch = np * spc;
    const float rspc = 1.0f / (float)spc;
    constexpr int UR = 4;
    for (uint32_t r0 = 0; r0 < nch; r0 += kBlock * UR) {
        u32x4 x[UR];
        uint32_t qq[UR], cc[UR];
#pragma unroll
        for (int u = 0; u < UR; u++) {
            const uint32_t i = r0 + (uint32_t)u * kBlock + threadIdx.x;
            const uint32_t ic = (i < nch) ? i : 0u;
            const uint32_t k = div_recip(ic, spc, rspc);
            cc[u] = ic - k * spc;
            qq[u] = (i < nch) ? pos[k] : kNoDest;
            x[u] = u32x4{0u, 0u, 0u, 0u};
            if (qq[u] != kNoDest)
                x[u] = ld16_nt(pkts + (uint64_t)(p0 + k) * stride + 16u * cc[u]);
        }
#pragma unroll
        for (int u = 0; u < UR; u++) {
            if (qq[u] != kNoDest) {
                uint8_t *o = out + (uint64_t)qq[u] * stride + 16u * cc[u];
                st16(o, x[u]);
            }
        }
    }
}

}  // namespace e2sar_amd
