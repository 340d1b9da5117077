// reas_fused.hpp -- reassembly as one fused kernel (reas_kernel), and its chained experimental sibling.
#pragma once

#include "dev_access.hpp"
#include "reas_classify.hpp"
#include "reas_copy.hpp"
#include "reas_store.hpp"
#include "seg_device.hpp"
#include "wire.hpp"

namespace e2sar_amd {

// ---------------------------------------------------------------------------------
// reassembly: one fused kernel

// Per-workgroup LDS of the fused reassembly: destinations of the group's datagrams, and
// the run tails' completion state (only the atomic's return value stays in registers during
// the copy, which keeps the kernel's occupancy up).
struct ReasGroupLds {
    PktInfo info[64];
    uint64_t ev[64], boff[64];
    uint32_t slot[64], bytes[64], d[64], rb[64], rc[64], tail[64];
};

// One group of gn <= 64 consecutive datagrams [g*G, g*G + gn), by the whole workgroup:
//   1. every wave loads the group's headers (lane p: datagram p); the load geometry of each
//      payload -- its phase in the event buffer and its length -- comes from them;
//   2. every thread issues its first U destination-aligned 16-byte payload loads;
//   3. wave 0 classifies (event table lookup/insert, run sums, counter atomics) while those
//      loads are in flight, and leaves each datagram's destination in LDS;
//   4. every thread stores its chunks (da_store), then loads and stores the rest round by
//      round (U chunks of 16 bytes per thread per round) -- 2 to 4 are group_copy
//      (reas_copy.hpp), which rows_kernel shares;
//   5. the run tails complete events (their atomic results are consumed last).
// HO: the chained form -- every datagram byte and length is read with sc1 loads (they were
// stored write-through by seg_block in the same launch).
template <int U, bool HO = false, int NT = kBlock>
__device__ __forceinline__ void reas_range(const ReasDev &R, const uint8_t *__restrict__ pkts, uint32_t stride,
                                           const uint32_t *__restrict__ lens, uint32_t g0, uint32_t gn, uint64_t now,
                                           uint32_t g, ReasGroupLds &L)
{
    const uint32_t tx = threadIdx.x;
    const bool w0 = tx < 64;
    const uint32_t lane = tx & 63u;

    TRACE_AT(0, 0, trace_now());
    // every wave issues the (cached) header loads so no load result crosses a branch
    const RawHdr raw = load_hdr<HO>(R.withLB != 0, pkts, stride, lens, g0 + ((lane < gn) ? lane : 0u));
    TRACE_WAIT();
    TRACE_AT(2, 0, trace_now());

    const uint32_t hl = R.withLB ? kLBREHdrLen : kREHdrLen;
    const uint32_t gPhase = bswap32(raw.re.y) & kPhaseMask;
    uint32_t gPlen = hdr_payload_len(raw.len, hl, stride);
    if (R.ownWorld > 1u && re_valid(raw.re.x) &&
        foreign_event(R, ((uint64_t)bswap32(raw.re.w) << 32) | bswap32(raw.re4)))
        gPlen = 0u;                                                    // another rank's: no payload loads

    unsigned long long old = 0;
    group_copy<U, HO, NT>(pkts, stride, g0, gn, hl, gPhase, gPlen, L.info, [&] {
        if (!w0) return;                                               // wave 0 classifies
        const Classified cl = classify_wave<true>(R, raw, stride, lane < gn, now, g);
        L.info[lane] = cl.info;
        old = cl.old;
        L.ev[lane] = cl.ev;
        L.boff[lane] = cl.boff;
        L.slot[lane] = cl.slot;
        L.bytes[lane] = cl.sbytes;
        L.d[lane] = cl.d;
        L.rb[lane] = cl.rb;
        L.rc[lane] = cl.rc;
        L.tail[lane] = cl.tailAdd ? 1u : 0u;
        TRACE_AT(0, 1, trace_now());
    });

    if (w0 && L.tail[lane]) {
        Classified cl;
        // in-order vmcnt: issued before the copy, this atomic's return (slow when ~100 groups
        // of one event add at once) would gate wave 0's first copy wait
        if (L.bytes[lane] >= kDeferAccBytes)
            old = atomicAdd(&R.slots[L.slot[lane]].acc, ((unsigned long long)L.rc[lane] << kAccFragShift) | L.rb[lane]);
        cl.old = old;
        cl.ev = L.ev[lane];
        cl.boff = L.boff[lane];
        cl.slot = L.slot[lane];
        cl.sbytes = L.bytes[lane];
        cl.d = L.d[lane];
        cl.rb = L.rb[lane];
        cl.rc = L.rc[lane];
        cl.tailAdd = true;
        classify_finish(R, cl);
    }
#if E2SAR_TRACE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    TRACE_AT(0, 3, trace_now());
#endif
}

// starts (optional): group g is datagrams [starts[g], starts[g+1]) (<= 64), e.g. the XCD
// stripes of the batch's segmentation (seg_groups); otherwise [g*G, g*G + G).
template <int U, bool HO = false, int NT = kBlock>
__device__ __forceinline__ void reas_group(const ReasDev &R, const uint8_t *__restrict__ pkts, uint32_t stride,
                                           const uint32_t *__restrict__ lens, uint32_t n, uint64_t now, uint32_t G,
                                           uint32_t g, ReasGroupLds &L, const uint32_t *__restrict__ starts = nullptr)
{
    uint32_t g0 = g * G;
    uint32_t gn = (n - g0 < G) ? n - g0 : G;
    if (starts) {
        // a caller-supplied device table: never trust it past the batch
        g0 = starts[g];
        if (g0 >= n) return;
        const uint32_t g1 = (starts[g + 1] < n) ? starts[g + 1] : n;
        if (g1 <= g0 || g1 - g0 > 64u) return;                       // empty or oversized group
        gn = g1 - g0;
    }
    reas_range<U, HO, NT>(R, pkts, stride, lens, g0, gn, now, g, L);
}

// reas_kernel's workgroup size for a slot stride
constexpr int kReasNTSmall = 768;   // slots of <= 4 KiB
constexpr int kReasNTJumbo = 512;
__host__ __device__ constexpr int reas_threads(uint32_t stride)
{
    return stride <= 4096u ? kReasNTSmall : kReasNTJumbo;
}

// reas_kernel: workgroup b reassembles datagrams [b*G, b*G + G) of the batch.
// (A/B: a resident grid drawing groups dynamically from per-XCD work counters, to even
// out XCDs that stream at different rates, ran 1.7-2.2x slower: a workgroup's groups are
// then classified one after another and every classification -- ~7 us of dependent table
// round trips -- sits in front of its copy, where the one-shot grid classifies all groups
// at once while the first round of loads is in flight.  Round 2 gave the resident grid a
// classifier wave that classifies the next group while copy waves copy the current one,
// then an LDS ring of classified groups: bit-exact, 79.7-81.8 us against 74-75 us here --
// the groups buffered per workgroup when the queues run dry lengthen the tail)
// NT threads per workgroup: wave 0 classifies while all NT/64 waves hold a round of loads
// (NT x U chunks) in flight.  Round 4 (profiles/round4/ab/reas_threads.log,
// reas_group_sizes.log): 768 threads (two workgroups of 12 waves per CU, 59-datagram
// groups in 1.8 rounds) take the 1 MiB @ MTU 1500 batch in 72.7-72.9 us against 75.4-75.7
// at 256 (six of 4 waves, 49 datagrams in 4.4 rounds); with jumbo slots 512 threads do
// best (71.0 against 73.4-74.0 us at 256 and 71.7 at 768); 1024 threads (one workgroup
// per CU) lose (82-84 us).
template <int U, int NT>
__global__ __launch_bounds__(NT) void reas_kernel(ReasDev R, const uint8_t *__restrict__ pkts, uint32_t stride,
                                                  const uint32_t *__restrict__ lens, uint32_t n, uint64_t now,
                                                  uint32_t G, const uint32_t *__restrict__ starts)
{
    __shared__ ReasGroupLds L;
    reas_group<U, false, NT>(R, pkts, stride, lens, n, now, G, blockIdx.x, L, starts);
}

// ---------------------------------------------------------------------------------
// chained form: segmentation of a batch and reassembly of the same datagrams in ONE launch.
// Workgroups [0, nSeg) are seg_kernel blocks (HO: write-through stores, then a per-group
// counter add); workgroups [nSeg, nSeg + groups) are reas_kernel groups, each of which
// waits until its counter shows every datagram of its range written, then runs as in
// reas_kernel with sc1 loads.  A group waits only on blocks with lower indices, which
// are dispatched before it and never wait, so the grid always drains; the wait is also
// bounded (2 s, error flag bit 4), so a miscount can never hang the device.  The group
// resets its counter for the next launch.  What this buys over two launches: the
// reassembly groups start while the last segmentation blocks finish (no kernel boundary,
// no half-empty tail between the two kernels).

#if E2SAR_HIP_EXPERIMENTAL
// seg blocks of 16 KiB (8-KiB blocks, as seg_kernel uses for 1 MiB events, made the chained
// launch 147 -> 158 us: twice the blocks at the reassembly occupancy)
constexpr int kChainSegU = 4;

__device__ __forceinline__ void wait_group_ready(const ReasDev &R, uint32_t *tiles, uint32_t g, uint32_t expect)
{
    if (threadIdx.x == 0) {
        uint32_t *t = tiles + g;
        uint64_t t0 = 0;
        for (uint32_t it = 0;; it++) {
            const uint32_t v = ld4_sc1(t);
            if (v >= expect) {
                if (v != expect) atomicOr(&R.ctl->errorFlags, 32u);           // over-count
                break;
            }
            const uint64_t now = __builtin_amdgcn_s_memrealtime();           // 100 MHz
            if (it == 0) t0 = now;
            else if (now - t0 > 200000000ull) {
                atomicOr(&R.ctl->errorFlags, 16u);                           // wait timed out
                break;
            }
            __builtin_amdgcn_s_sleep(2);
        }
        st4_sc1(t, 0u);
    }
    __syncthreads();
}

template <int U>
__global__ __launch_bounds__(kBlock) void segreas_kernel(ChainBatches cb, int lbVersion,
                                                                              uint32_t maxPld, uint32_t stride,
                                                                              ReasDev R, uint64_t now)
{
    __shared__ ReasGroupLds L;
    // grid: [seg(0) | reas(0) | seg(1) | reas(1) | ...]; a reassembly group depends only on
    // segmentation blocks of its own batch, all of which have lower indices
    uint32_t b = 0;
    while (b + 1u < cb.nb && blockIdx.x >= cb.b[b + 1u].start) b++;
    const ChainBatch &B = cb.b[b];
    const uint32_t local = blockIdx.x - B.start;
    if (local < B.nSeg) {
        seg_block<kChainSegU, true>(B.events, B.bpe, lbVersion, maxPld, B.pkts, stride, B.lens, nullptr, local,
                                           B.G, B.tiles);
        return;
    }
    const uint32_t g = local - B.nSeg;
    const uint32_t slots = (B.n - g * B.G < B.G) ? B.n - g * B.G : B.G;
    wait_group_ready(R, B.tiles, g, slots * (stride >> 4));
    reas_group<U, true>(R, B.pkts, stride, B.lens, B.n, now, B.G, g, L);
}

#endif  // E2SAR_HIP_EXPERIMENTAL

}  // namespace e2sar_amd
