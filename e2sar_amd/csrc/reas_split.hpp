// reas_split.hpp -- reassembly as two phases: the classify, scatter and pipelined scatter+classify kernels.
#pragma once

#include "dev_access.hpp"
#include "reas_classify.hpp"
#include "reas_store.hpp"

namespace e2sar_amd {

// ---------------------------------------------------------------------------------
// reassembly as two phases: classify (headers only, latency-bound) then scatter (bytes
// only, bandwidth-bound).  Each phase is a launch of its own, or -- the pipelined form --
// one launch scatters batch b while other workgroups of the same grid classify batch
// b+1, so the table round trips of b+1 run under the copy of b instead of in front of it.
//
// Work buffer of a classified batch of n datagrams: PktInfo[n] then FinishRec[n].  A run
// tail whose add completed its event sets kPktCompletes in its own PktInfo.hl and writes
// FinishRec[p]; the scatter workgroup that owns datagram p publishes the event after its
// own stores (the bytes of every workgroup are visible at the end of that launch).

constexpr uint32_t kPktCompletes = 0x80000000u;
constexpr uint32_t kFinKeepSlot = 0x80000000u;     // FinishRec.slot flag (reference-order mode)

// One wave: classify datagrams [p0, p0+64) of the batch.
__device__ __forceinline__ void classify_wave_to_work(const ReasDev &R, const uint8_t *__restrict__ pkts,
                                                      uint32_t stride, const uint32_t *__restrict__ lens,
                                                      uint32_t n, uint64_t now, PktInfo *__restrict__ info,
                                                      FinishRec *__restrict__ fin, uint32_t wave)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t p0 = wave * 64u;
    if (p0 >= n) return;                                       // wave-uniform
    const uint32_t gn = (n - p0 < 64u) ? n - p0 : 64u;
    const RawHdr raw = load_hdr(R.withLB != 0, pkts, stride, lens, p0 + ((lane < gn) ? lane : 0u));
    const Classified cl = classify_wave(R, raw, stride, lane < gn, now, wave);
    const bool done = completes(cl);
    if (lane < gn) st_info(info + p0 + lane, cl.info, done ? kPktCompletes : 0u);
    if (done) {
        FinishRec f;
        f.ev = cl.ev;
        f.boff = cl.boff;
        f.slot = cl.slot;
        f.bytes = cl.sbytes;
        f.frags = (uint32_t)(cl.old >> kAccFragShift) + cl.rc;
        f.d = cl.d;
        fin[p0 + lane] = f;
    }
}

// One workgroup: scatter datagrams [blk*G, blk*G+G) of a classified batch.
template <int U, bool NT, bool STAGE, int TB>
__device__ __forceinline__ void scatter_group(const ReasDev &R, const uint8_t *__restrict__ pkts, uint32_t stride,
                                              uint32_t n, uint32_t G, const PktInfo *__restrict__ info,
                                              const FinishRec *__restrict__ fin, uint32_t blk, PktInfo *sinfo)
{
    const uint32_t g0 = blk * G;
    const uint32_t gn = (n - g0 < G) ? n - g0 : G;
    const uint32_t lane = threadIdx.x & 63u;

    // every wave loads the records (cached) so no load result crosses a branch; they are
    // issued before the payload loads so waiting for them does not wait for the payload
    const PktInfo mine = ld_info(info + g0 + ((lane < gn) ? lane : 0u));

    const uint32_t spc = stride >> 4;
    uint32_t nch = gn * spc;
    const float rspc = 1.0f / (float)spc;
    const uint8_t *const bpk = pkts + (uint64_t)g0 * stride;
    u32x4 x[U];
    uint32_t pp[U], cc[U];
    auto issue = [&](uint32_t r0) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t i = r0 + (uint32_t)u * TB + threadIdx.x;
            const uint32_t ic = (i < nch) ? i : 0u;
            const uint32_t p = div_recip(ic, spc, rspc);
            pp[u] = p;
            cc[u] = ic - p * spc;
            const uint8_t *src = bpk + (uint64_t)p * stride + 16u * cc[u];
            x[u] = NT ? ld16_nt(src) : ld16(src);
        }
    };
    issue(0);
    bool fins = false;
    if (threadIdx.x < 64) {
        // a record that does not land inside the arena (a work buffer that was not filled
        // by classify for this batch) is dropped and flagged, never written through
        const uint64_t lo = (uint64_t)R.arena, hi = lo + R.arenaBytes;
        const bool inside = mine.plen == 0 || (mine.dst >= lo && mine.dst + mine.plen <= hi);
        if (lane < gn && !inside) atomicOr(&R.ctl->errorFlags, 8u);
        PktInfo v = (lane < gn && inside) ? mine : PktInfo{0ull, 0u, 0u};
        fins = (v.hl & kPktCompletes) != 0u;
        v.hl &= ~kPktCompletes;
        sinfo[lane] = v;
    }
    __syncthreads();

    if constexpr (STAGE) {
        if (nch <= (uint32_t)(TB * U)) {
            lds_stage_store<U, TB>(sinfo, x, pp, cc, nch, gn, stride);
            nch = 0;                                                 // done: skip the rounds below
        }
    }
    for (uint32_t r0 = 0; r0 < nch; r0 += (uint32_t)(TB * U)) {
        if (r0) issue(r0);
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t i = r0 + (uint32_t)u * TB + threadIdx.x;
            if (i >= nch) continue;
            scatter_chunk(sinfo[pp[u]], cc[u], x[u]);
        }
    }

    if (fins) {
        const FinishRec f = fin[g0 + lane];
        const uint32_t fs = f.slot & ~kFinKeepSlot;
        if (fs < R.tableSlots) complete_event(R, fs, f.ev, f.boff, f.bytes, f.d, f.frags, (f.slot & kFinKeepSlot) != 0u);
        else atomicOr(&R.ctl->errorFlags, 8u);
    }
}

// (Round 3-4: chunk-range scatter workgroups -- loads exactly a linear 16-KiB range of the
// slots whatever datagrams they belong to, registers or LDS-staged -- measured no better on
// config 3 and lost on the cold leg; removed)

// XCD-aware visit order of the scatter forms (round 5).  Workgroup b of a launch runs on XCD
// b mod 8 (round-robin dispatch; a speed assumption only, never correctness).  In dispatch
// order, consecutive scatter groups -- one 8976-byte datagram at MTU 9000, eight at 1500 --
// sat on different XCDs, so every group boundary (a 128-byte slot line shared by two
// datagrams, and at the destination a line shared by two payloads) was touched by two
// XCDs' L2s.  Here each XCD takes runs of kXcdRun consecutive groups, the eight XCDs' runs
// side by side, so the launch still moves through the batch as one front.  Config 3 (70 x 8
// MiB at MTU 9000, 65,730 one-datagram groups): split reassembly 231-234 -> 211-213 us with
// runs of 128 (32-128 within 2 us; 8 or 16 contiguous regions, one per XCD, 221-224 us;
// spreading the groups in flight over 64-70 regions 236-246 us), cold leg at MTU 1500
// unchanged within noise (profiles/round5/xcd_order/).  A bijection on [0, nb): the last
// nb mod (8 kXcdRun) groups keep their order.
constexpr uint32_t kXcdRun = 128;
__host__ __device__ constexpr uint32_t xcd_runs(uint32_t b, uint32_t nb)
{
    constexpr uint32_t W = 8u * kXcdRun;
    if (b >= nb / W * W) return b;
    const uint32_t w = b % W;
    return (b - w) + (w % 8u) * kXcdRun + w / 8u;
}
// every group is visited exactly once (checked at compile time around the window edges)
constexpr bool xcd_runs_bijective(uint32_t nb)
{
    bool seen[3200] = {};
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t g = xcd_runs(b, nb);
        if (g >= nb || seen[g]) return false;
        seen[g] = true;
    }
    return true;
}
static_assert(xcd_runs_bijective(1) && xcd_runs_bijective(1023) && xcd_runs_bijective(1024) &&
                  xcd_runs_bijective(1025) && xcd_runs_bijective(2048) && xcd_runs_bijective(3199),
              "xcd_runs must be a bijection on [0, nb)");

__global__ __launch_bounds__(kBlock) void reas_classify_kernel(ReasDev R, const uint8_t *__restrict__ pkts,
                                                               uint32_t stride, const uint32_t *__restrict__ lens,
                                                               uint32_t n, uint64_t now, PktInfo *__restrict__ info,
                                                               FinishRec *__restrict__ fin)
{
    classify_wave_to_work(R, pkts, stride, lens, n, now, info, fin, blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6));
}

template <int U, bool NT, bool STAGE, int TB = kScatBlock>
__global__ __launch_bounds__(TB) void reas_scatter_kernel(ReasDev R, const uint8_t *__restrict__ pkts,
                                                              uint32_t stride, uint32_t n, uint32_t G,
                                                              const PktInfo *__restrict__ info,
                                                              const FinishRec *__restrict__ fin)
{
    __shared__ PktInfo sinfo[64];
    scatter_group<U, NT, STAGE, TB>(R, pkts, stride, n, G, info, fin, xcd_runs(blockIdx.x, (n + G - 1u) / G), sinfo);
}

// Pipelined form: workgroups [clsStart, clsStart + nClsBlocks) classify batch b+1, the rest
// scatter batch b (in xcd_runs order: clsStart and nClsBlocks are multiples of 8, so a
// scatter workgroup's index keeps its XCD parity).
template <int U, bool NT, bool STAGE, int TB = kScatBlock>
__global__ __launch_bounds__(TB) void reas_scatter_classify_kernel(
    ReasDev R, uint32_t stride, const uint8_t *__restrict__ spk, uint32_t sn, uint32_t G,
    const PktInfo *__restrict__ sinfoG, const FinishRec *__restrict__ sfin, const uint8_t *__restrict__ cpk,
    const uint32_t *__restrict__ clens, uint32_t cn, uint64_t now, PktInfo *__restrict__ cinfo,
    FinishRec *__restrict__ cfin, uint32_t nClsBlocks, uint32_t clsStart)
{
    __shared__ PktInfo sinfo[64];
    // workgroups [clsStart, clsStart + nClsBlocks) classify, the others scatter
    const uint32_t b = blockIdx.x;
    if (b - clsStart < nClsBlocks) {
        classify_wave_to_work(R, cpk, stride, clens, cn, now, cinfo, cfin,
                              (b - clsStart) * (TB / 64) + (threadIdx.x >> 6));
        return;
    }
    const uint32_t sb = (b < clsStart) ? b : b - nClsBlocks;
    scatter_group<U, NT, STAGE, TB>(R, spk, stride, sn, G, sinfoG, sfin, xcd_runs(sb, (sn + G - 1u) / G), sinfo);
}

}  // namespace e2sar_amd
