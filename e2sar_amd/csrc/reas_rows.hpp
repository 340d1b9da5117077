// reas_rows.hpp -- reassembly straight into a dense [events, sources, pitch] tensor (e2sar_hip_rows_*): no table, no arena.
#pragma once

#include <type_traits>

#include "dev_access.hpp"
#include "reas_classify.hpp"
#include "reas_copy.hpp"
#include "reas_store.hpp"
#include "rows_div.hpp"
#include "wire.hpp"

namespace e2sar_amd {

// ---------------------------------------------------------------------------------
// A stream that numbers its events consecutively and names its sources by dataId needs no
// event table: the place of a fragment follows from its header alone -- row eventNum mod
// nEvents, cell j where ids[j] == dataId, byte bufferOffset.  What is left of reas_kernel's
// classification is one compare-and-swap per run head (the cell's length: whoever finds 0
// opens the cell) and one add per run tail (the cell's accumulator); the copy is reas_kernel's.
//   A window on a lattice (eventStep S > 1, the template parameter LAT) holds one rank's share of
// such a stream, the events with eventNum mod S == eventPhase: what was said of eventNum holds of
// the event's index eventNum / S, and a datagram of another rank's event is passed over at the
// price of its header -- every wave learns that before it issues a payload load (rows_range).
// LAT = false is the consecutive window: its code does not know the lattice.
//   The seen calls (e2sar_hip_rows_reassemble_seen, the template parameter SEEN) keep one bit per fragment of a
// cell -- fragment f = bufferOffset / fragBytes -- and take a fragment once: between the head's compare-and-swap
// and the tail's add stands one test-and-set of the bits, an atomicOr per stretch of a run inside one 32-bit
// word.  SEEN = false is the plain call: its code does not know the bits.

static_assert(sizeof(e2sar_hip_rows_cell) == 16 && offsetof(e2sar_hip_rows_cell, bytes) == 8 &&
                  offsetof(e2sar_hip_rows_cell, flags) == 12,
              "a cell is one 16-byte record: acc, bytes, flags");

// counts[] of a window
enum : uint32_t {
    kRowsComplete = 0, kRowsAccepted = 1, kRowsBytes = 2, kRowsLate = 3, kRowsEarly = 4, kRowsForeign = 5,
    kRowsBadHeader = 6, kRowsDataErr = 7, kRowsReleased = 8, kRowsReleasedComplete = 9,
    kRowsNotOwned = 10,            // a lattice only: another rank's event
    kRowsDuplicate = 11            // the seen calls only: a fragment whose bit was set
};

// Per-workgroup LDS: destinations of the group's datagrams, and what the run tails need
// after the copy (only the add's return value stays in a register meanwhile).
template <bool LAT = false, bool SEEN = false>
struct RowsGroupLds {
    PktInfo info[64];
    uint32_t cell[64], bytes[64], rb[64], tail[64];
    // the group's additions to counts[0..7] ([0]: known after the copy); a lattice: one more, to counts[10]; the
    // seen calls: one more behind that, to counts[11]
    uint64_t cnt[8 + (LAT ? 1 : 0) + (SEEN ? 1 : 0)];
};
// What the seen calls add to a window, and what stands in its place in a plain call's kernel arguments: nothing
struct RowsNoSeen {};
template <bool SEEN>
using RowsSeenArg = std::conditional_t<SEEN, RowsSeenDev, RowsNoSeen>;
static_assert(sizeof(RowsGroupLds<false>) == 2112, "the consecutive window's LDS is what it was");

// The lattice of a window with eventStep S > 1: the index eventNum / S of an event, and whether
// the window owns it (eventNum mod S == eventPhase).  Exact for every 64-bit eventNum and every
// S in [2, 2^32): with M = floor(2^64 / S) from the host (RowsDev.magic), ev * M / 2^64 lies in
// (ev / S - 1, ev / S], so the product's high half is the quotient or one below it, and the
// remainder -- below 2 S -- says which.  Four 32-bit multiplies and a compare: no division
// sequence, no scratch.
struct RowsPos {
    uint64_t q;
    bool owned;
};
__device__ __forceinline__ RowsPos rows_lattice(const RowsDev &W, uint64_t ev)
{
    uint64_t q = __umul64hi(ev, W.magic);
    uint64_t r = ev - q * W.step;
    if (r >= W.step) {
        q++;
        r -= W.step;
    }
    return RowsPos{q, r == W.phase};
}
// The upkeep kernels' view, the step a run-time value: the index of the window's first
// position, and the event numbers from one position to the next
__device__ __forceinline__ uint64_t rows_base_index(const RowsDev &W)
{
    const uint64_t b = *W.base;
    return W.step > 1u ? rows_lattice(W, b).q : b;
}
__device__ __forceinline__ uint64_t rows_stride(const RowsDev &W) { return W.step > 1u ? W.step : 1u; }
// eventNum of a raw header, as parse_hdr reads it
__device__ __forceinline__ uint64_t raw_event(const RawHdr &raw) { return ((uint64_t)bswap32(raw.re.w) << 32) | bswap32(raw.re4); }

// The number of lanes of a whole wave for which `on` holds, added to counts[k] by the wave's
// lane 0 -- no atomic when there is none.
__device__ __forceinline__ void rows_count(uint64_t *counts, uint32_t k, bool on)
{
    const uint64_t m = __ballot(on);
    if (m && (threadIdx.x & 63u) == 0u) atomicAdd((unsigned long long *)(counts + k), (unsigned long long)__builtin_popcountll(m));
}

// Classification of the group's datagrams by one whole wave (lane p: datagram p, `live`
// below gn): the rules of e2sar_hip_rows_reassemble in their order.  Leaves every
// datagram's destination in L.info, the run tails' state and the group's counts in L; returns
// the value the tail's accumulator add found (consumed after the copy, rows_finish).
template <bool LAT, bool SEEN>
__device__ __forceinline__ unsigned long long rows_classify(const RowsDev &W, const RowsSeenArg<SEEN> &Z, const RawHdr &raw,
                                                            uint32_t stride, bool live, RowsGroupLds<LAT, SEEN> &L)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t hl = W.withLB ? kLBREHdrLen : kREHdrLen;
    const ParsedHdr h = parse_hdr(raw, hl, stride, live);
    bool ok = h.ok, derr = h.derr;

    // a lattice: the event's index stands where its number stood; another rank's event stops here
    uint64_t idx = h.ev;
    bool notOwned = false;
    if constexpr (LAT) {
        const RowsPos p = rows_lattice(W, h.ev);
        idx = p.q;
        notOwned = ok && !p.owned;
        ok = ok && p.owned;
    }
    // the cell's column: the place of the dataId among the window's ids
    uint32_t j = ~0u;
    for (uint32_t k = 0; k < W.nIds; k++)
        if ((uint32_t)W.ids[k] == h.d) j = k;
    const bool foreign = ok && j == ~0u;
    ok = ok && !foreign;
    // the window, by 64-bit wrap-around distance from its base
    uint64_t dist = h.ev - *W.base;
    if constexpr (LAT) dist = idx - rows_lattice(W, *W.base).q;
    const bool outside = ok && dist >= (uint64_t)W.nEvents;
    const bool late = outside && (int64_t)dist < 0;
    ok = ok && !outside;
    // the fragment's own bounds: it opens nothing
    if (ok && (h.blen == 0u || (uint64_t)h.off + h.pl > h.blen)) {
        ok = false;
        derr = true;
    }
    // the grid of the seen calls (rule 4b): a fragment of more than 0 bytes lies on a multiple of fragBytes, is at
    // most that long, and its number is below maxFrags; it opens nothing otherwise
    uint32_t f = 0;
    if constexpr (SEEN) {
        const RowsQuot fq = rows_div(h.off, Z.fragBytes, Z.magic);
        f = fq.q;
        if (ok && h.pl > 0u && (fq.r != 0u || h.pl > Z.fragBytes || f >= Z.maxFrags)) {
            ok = false;
            derr = true;
        }
    }
    const uint32_t cell = ok ? ((uint32_t)idx & (W.nEvents - 1u)) * W.nIds + j : ~0u;

    // ---- runs of one cell: consecutive lanes of one (eventNum, dataId) inside the window ----
    const uint32_t pc = lane_prev(cell, ~0u), nc = lane_next(cell, ~0u);
    const bool head = ok && (lane == 0u || pc != cell);
    const bool tail = ok && (lane == 63u || nc != cell);
    e2sar_hip_rows_cell *const cp = W.cells + (ok ? cell : 0u);

    // the head opens the cell or learns its length: one compare-and-swap round trip per run
    uint32_t sb = 0;
    if (head) {
        // (A load in front, so that only openers pay the compare-and-swap, lost: two round
        // trips for them, and rows_kernel at MTU 1500 86.2 against 71.9 us)
        const uint32_t was = atomicCAS(&cp->bytes, 0u, h.blen);
        sb = was ? was : h.blen;
    }
    const int myhead = run_head_lane(__ballot(head), lane);
    sb = __shfl(sb, myhead);

    // bounds against the cell's length
    bool take = ok;
    if (take && (uint64_t)h.off + h.pl > sb) {
        take = false;
        derr = true;
    }
    // The seen calls (rule 5b): the fragment's bit, tested and set.  A stretch is a maximal sequence of consecutive
    // lanes whose fragments have bytes, share one word of the bits and rise in f from lane to lane: its bits are
    // distinct, so their sum (a scan, as the run sums below) is their union, and the stretch's last lane issues one
    // returning atomicOr for all of them -- a handful per in-order group, in one instruction, one round trip.  Two
    // copies of a fragment never share a stretch: their atomics are ordered by the memory system, and exactly
    // one finds the bit clear.
    bool dup = false;
    if constexpr (SEEN) {
        const bool part = take && h.pl > 0u;
        const uint64_t wi = part ? (uint64_t)cell * (Z.maxFrags >> 5) + (f >> 5) : ~0ull;
        const uint64_t pw = ((uint64_t)lane_prev((uint32_t)(wi >> 32), ~0u) << 32) | lane_prev((uint32_t)wi, ~0u);
        const uint64_t nw = ((uint64_t)lane_next((uint32_t)(wi >> 32), ~0u) << 32) | lane_next((uint32_t)wi, ~0u);
        const uint32_t pf = lane_prev(f, 0u), nf = lane_next(f, 0u);
        const bool first = part && (lane == 0u || pw != wi || pf >= f);
        const bool last = part && (lane == 63u || nw != wi || f >= nf);
        const uint32_t bit = part ? 1u << (f & 31u) : 0u;
        const uint32_t is = wave_incl_scan(bit);
        const uint32_t mask = is - __shfl(is - bit, run_head_lane(__ballot(first), lane));
        uint32_t was = 0;
        if (last) was = atomicOr(Z.seen + wi, mask);
        const uint64_t lasts = __ballot(last) & (~0ull << lane);       // part: its stretch's last lane is at or above it
        was = __shfl(was, lasts ? __builtin_ctzll(lasts) : (int)lane);
        dup = part && ((was >> (f & 31u)) & 1u) != 0u;
        take = take && !dup;
    }
    // segmented sums over the run (inclusive scans, then the difference at the head)
    const uint32_t xb = take ? h.pl : 0u, xc = take ? 1u : 0u;
    const uint32_t ib = wave_incl_scan(xb), ic = wave_incl_scan(xc);
    const uint32_t rb = ib - __shfl(ib - xb, myhead), rc = ic - __shfl(ic - xc, myhead);

    // the tail's add: its return value is wanted only after the copy
    unsigned long long old = 0;
    const bool tailAdd = tail && rc > 0u;
    if (tailAdd) old = atomicAdd((unsigned long long *)&cp->acc, ((unsigned long long)rc << kAccFragShift) | rb);
    // a fragment that passes the pitch: rare, so one atomic each
    const bool trunc = take && (uint64_t)h.off + h.pl > W.pitch;
    if (trunc) atomicOr(&cp->flags, E2SAR_HIP_ROWS_TRUNCATED);

    PktInfo pi;
    const uint32_t room = (h.off < W.pitch) ? W.pitch - h.off : 0u;
    pi.plen = take ? (h.pl < room ? h.pl : room) : 0u;
    pi.dst = pi.plen ? (uint64_t)(W.out + (uint64_t)cell * W.pitch + h.off) : 0ull;
    pi.hl = hl;
    L.info[lane] = pi;
    L.cell[lane] = cell;
    L.bytes[lane] = sb;
    L.rb[lane] = rb;
    L.tail[lane] = tailAdd ? 1u : 0u;

    // The workgroup's counts: this wave has classified all of its datagrams.  They wait in LDS
    // until the copy is over (rows_finish): every workgroup of the launch adds to the same
    // words, and vmcnt retires in order, so an add issued here would stand between this wave
    // and the second round of its copy.
    const uint32_t tl = take ? h.pl : 0u;                              // summed as 16-bit halves, as wave_stats does
    const uint64_t tb = (uint64_t)readlane(wave_incl_scan(tl & 0xFFFFu), 63) +
                        ((uint64_t)readlane(wave_incl_scan(tl >> 16), 63) << 16);
    const uint64_t votes[8] = {0ull, __ballot(take), 0ull, __ballot(late), __ballot(outside && !late), __ballot(foreign),
                               __ballot(h.bad), __ballot(derr)};
    const uint64_t voteNotOwned = LAT ? __ballot(notOwned) : 0ull;
    const uint64_t voteDup = SEEN ? __ballot(dup) : 0ull;
    if (lane == 0u) {
#pragma unroll
        for (uint32_t k = 0; k < 8u; k++) L.cnt[k] = (uint64_t)__builtin_popcountll(votes[k]);
        L.cnt[kRowsBytes] = tb;
        if constexpr (LAT) L.cnt[8] = (uint64_t)__builtin_popcountll(voteNotOwned);
        if constexpr (SEEN) L.cnt[LAT ? 9 : 8] = (uint64_t)__builtin_popcountll(voteDup);
    }
    return old;
}

// After the copy, by the classifying wave: a tail whose add of more than 0 bytes brought the
// cell's curBytes to its length marks the cell complete.
template <bool LAT, bool SEEN>
__device__ __forceinline__ void rows_finish(const RowsDev &W, unsigned long long old, const RowsGroupLds<LAT, SEEN> &L)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t rb = L.rb[lane];
    const bool done = L.tail[lane] && rb > 0u && (old & kAccBytesMask) + rb == (uint64_t)L.bytes[lane];
    if (done) atomicOr(&W.cells[L.cell[lane]].flags, E2SAR_HIP_ROWS_COMPLETE);
    // the workgroup's counts: lane k adds to counts[k], one instruction for all eight
    const uint64_t ndone = (uint64_t)__builtin_popcountll(__ballot(done));
    if constexpr (SEEN) {                                              // behind the eight: counts[10] (a lattice), counts[11]
        constexpr uint32_t nCnt = LAT ? 10u : 9u;
        if (lane < nCnt) {
            const uint64_t v = (lane == kRowsComplete) ? ndone : L.cnt[lane];
            const uint32_t k = lane < 8u ? lane : (lane == nCnt - 1u ? kRowsDuplicate : kRowsNotOwned);
            if (v) atomicAdd((unsigned long long *)(W.counts + k), (unsigned long long)v);
        }
    } else if constexpr (LAT) {                                        // lane 8: counts[10]
        if (lane < 9u) {
            const uint64_t v = (lane == kRowsComplete) ? ndone : L.cnt[lane];
            if (v) atomicAdd((unsigned long long *)(W.counts + (lane < 8u ? lane : kRowsNotOwned)), (unsigned long long)v);
        }
    } else if (lane < 8u) {
        const uint64_t v = (lane == kRowsComplete) ? ndone : L.cnt[lane];
        if (v) atomicAdd((unsigned long long *)(W.counts + lane), (unsigned long long)v);
    }
}

// One group of gn <= 64 consecutive datagrams [g0, g0 + gn), by the whole workgroup -- the
// steps of reas_range (reas_fused.hpp) around the same group_copy (reas_copy.hpp):
//   1. every wave loads the group's headers (lane p: datagram p); on a lattice every wave then
//      finds the datagrams of other ranks' events and loads no payload for them;
//   2. every thread issues its first U destination-aligned 16-byte payload loads -- the
//      phase is bufferOffset mod 16: cells are 256-byte aligned;
//   3. wave 0 classifies (rows_classify) while those loads are in flight;
//   4. every thread stores its chunks (da_store), then loads and stores the rest round by
//      round, the loads of round r + 1 issued before the stores of round r;
//   5. wave 0's run tails mark completed cells (rows_finish).
template <int U, int NT, bool LAT, bool SEEN>
__device__ __forceinline__ void rows_range(const RowsDev &W, const RowsSeenArg<SEEN> &Z, const uint8_t *__restrict__ pkts,
                                           uint32_t stride, const uint32_t *__restrict__ lens, uint32_t g0, uint32_t gn,
                                           RowsGroupLds<LAT, SEEN> &L)
{
    const bool w0 = threadIdx.x < 64;
    const uint32_t lane = threadIdx.x & 63u;

    const RawHdr raw = load_hdr(W.withLB != 0, pkts, stride, lens, g0 + ((lane < gn) ? lane : 0u));
    const uint32_t hl = W.withLB ? kLBREHdrLen : kREHdrLen;

    // Whatever else its header says, a datagram whose event number is not the window's is not
    // taken (rule 1 or 1b): payload length 0, as reas_range has it for a foreign event.
    uint32_t gPlen = hdr_payload_len(raw.len, hl, stride);
    if constexpr (LAT)
        if (!rows_lattice(W, raw_event(raw)).owned) gPlen = 0u;

    unsigned long long old = 0;
    group_copy<U, false, NT>(pkts, stride, g0, gn, hl, bswap32(raw.re.y) & kPhaseMask, gPlen, L.info,
                             [&] { if (w0) old = rows_classify<LAT, SEEN>(W, Z, raw, stride, lane < gn, L); });

    if (w0) rows_finish<LAT, SEEN>(W, old, L);
}

// rows_kernel: workgroup b takes datagrams [b*G, b*G + G) of the first n = min(*count,
// bound) (count NULL: bound); the grid is cdiv(bound, G).  A workgroup at or past n costs the
// load of one word and an exit (reas_devcount.hpp): no header load, no LDS, no counter.
// LAT: the window is on a lattice (RowsDev.step > 1).  SEEN: a seen call; its bits travel in an argument of their
// own behind the others, where a plain call has an empty one, so that a plain window's kernel reads what it read.
template <int U, int NT, bool LAT = false, bool SEEN = false>
__global__ __launch_bounds__(NT) void rows_kernel(RowsDev W, const uint8_t *__restrict__ pkts, uint32_t stride,
                                                  const uint32_t *__restrict__ lens, const uint32_t *__restrict__ count,
                                                  uint32_t bound, uint32_t G, RowsSeenArg<SEEN> Z)
{
    __shared__ RowsGroupLds<LAT, SEEN> L;
    const uint32_t n = count ? dev_count(count, bound) : bound;
    const uint64_t g0 = (uint64_t)blockIdx.x * G;
    if (g0 >= n) return;
    rows_range<U, NT, LAT, SEEN>(W, Z, pkts, stride, lens, (uint32_t)g0, (n - (uint32_t)g0 < G) ? n - (uint32_t)g0 : G, L);
}

// ---------------------------------------------------------------------------------
// the ring's upkeep

// k = min(*d_k, kMax, nEvents): the positions the window lets go of
__device__ __forceinline__ uint32_t rows_advance_k(const RowsDev &W, const uint32_t *__restrict__ d_k, uint32_t kMax)
{
    uint32_t k = kMax < W.nEvents ? kMax : W.nEvents;
    if (d_k) {
        const uint32_t v = *d_k;
        k = v < k ? v : k;
    }
    return k;
}

// Thread t < k * nIds: the cell of position t / nIds behind the base, source t % nIds, is counted
// (released incomplete, released complete) and zeroed.  The base moves in a launch of its
// own, after every workgroup here has read it.  Grid: cdiv(min(kMax, nEvents) * nIds, kBlock).
__global__ __launch_bounds__(kBlock) void rows_release_kernel(RowsDev W, const uint32_t *__restrict__ d_k, uint32_t kMax)
{
    const uint64_t k = rows_advance_k(W, d_k, kMax);
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool in = t < k * W.nIds;
    bool open = false, complete = false;
    if (in) {
        const uint64_t e = t / W.nIds;
        const uint64_t c = ((rows_base_index(W) + e) & (uint64_t)(W.nEvents - 1u)) * W.nIds + (t - e * W.nIds);
        uint8_t *cp = reinterpret_cast<uint8_t *>(W.cells + c);
        const u32x4 v = ld16(cp);
        complete = (v.w & E2SAR_HIP_ROWS_COMPLETE) != 0u;
        open = v.z != 0u && !complete;
        st16(cp, u32x4{0u, 0u, 0u, 0u});
    }
    rows_count(W.counts, kRowsReleased, open);
    rows_count(W.counts, kRowsReleasedComplete, complete);
}

// The seen calls' release: thread t < k * nIds * Q, Q = maxFrags / 128 the 16-byte words of a cell's bits, zeroes
// word t % Q of the cell t / Q (numbered as above); the thread of word 0 also counts and zeroes the cell, as
// rows_release_kernel does.  Grid: cdiv(min(kMax, nEvents) * nIds * Q, kBlock).
__global__ __launch_bounds__(kBlock) void rows_release_seen_kernel(RowsDev W, RowsSeenDev Z, const uint32_t *__restrict__ d_k,
                                                                  uint32_t kMax)
{
    const uint64_t k = rows_advance_k(W, d_k, kMax);
    const uint64_t Q = Z.maxFrags >> 7;
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool in = t < k * W.nIds * Q;
    bool open = false, complete = false;
    if (in) {
        const uint64_t u = t / Q, wq = t - u * Q;
        const uint64_t e = u / W.nIds;
        const uint64_t c = ((rows_base_index(W) + e) & (uint64_t)(W.nEvents - 1u)) * W.nIds + (u - e * W.nIds);
        if (wq == 0u) {
            uint8_t *cp = reinterpret_cast<uint8_t *>(W.cells + c);
            const u32x4 v = ld16(cp);
            complete = (v.w & E2SAR_HIP_ROWS_COMPLETE) != 0u;
            open = v.z != 0u && !complete;
            st16(cp, u32x4{0u, 0u, 0u, 0u});
        }
        st16(reinterpret_cast<uint8_t *>(Z.seen) + (c * Q + wq) * 16u, u32x4{0u, 0u, 0u, 0u});
    }
    rows_count(W.counts, kRowsReleased, open);
    rows_count(W.counts, kRowsReleasedComplete, complete);
}

__global__ __launch_bounds__(64) void rows_shift_kernel(RowsDev W, const uint32_t *__restrict__ d_k, uint32_t kMax)
{
    if (threadIdx.x == 0) *W.base += rows_advance_k(W, d_k, kMax) * rows_stride(W);
}

// Every cell and all 16 counts zeroed, the base set: stores only, so it can be captured
// where a memset node cannot.
__global__ __launch_bounds__(kBlock) void rows_clear_kernel(RowsDev W, uint64_t eventBase)
{
    const uint64_t nCells = (uint64_t)W.nEvents * W.nIds;
    for (uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x; c < nCells; c += (uint64_t)gridDim.x * kBlock)
        st16(reinterpret_cast<uint8_t *>(W.cells + c), u32x4{0u, 0u, 0u, 0u});
    if (blockIdx.x == 0) {
        if (threadIdx.x < 16u) W.counts[threadIdx.x] = 0ull;
        if (threadIdx.x == 16u) *W.base = eventBase;
    }
}

// The seen calls' clear: rows_clear_kernel, and every 16-byte word of the bits zeroed.
__global__ __launch_bounds__(kBlock) void rows_clear_seen_kernel(RowsDev W, RowsSeenDev Z, uint64_t eventBase)
{
    const uint64_t nCells = (uint64_t)W.nEvents * W.nIds, nWords = nCells * (Z.maxFrags >> 7);
    for (uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x; c < nCells; c += (uint64_t)gridDim.x * kBlock)
        st16(reinterpret_cast<uint8_t *>(W.cells + c), u32x4{0u, 0u, 0u, 0u});
    for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < nWords; q += (uint64_t)gridDim.x * kBlock)
        st16(reinterpret_cast<uint8_t *>(Z.seen) + q * 16u, u32x4{0u, 0u, 0u, 0u});
    if (blockIdx.x == 0) {
        if (threadIdx.x < 16u) W.counts[threadIdx.x] = 0ull;
        if (threadIdx.x == 16u) *W.base = eventBase;
    }
}

}  // namespace e2sar_amd
