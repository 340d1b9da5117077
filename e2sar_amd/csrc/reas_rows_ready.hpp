// reas_rows_ready.hpp -- which events of a rows window are ready (e2sar_hip_rows_ready): the window's delivery half,
// decided on the device, and the zero fill that makes the ready rows a dense tensor.
#pragma once

#include "dev_access.hpp"
#include "reas_rows.hpp"
#include "reas_upkeep.hpp"

namespace e2sar_amd {

// ---------------------------------------------------------------------------------
// Three launches.  rows_scan_kernel folds every event's cells into one summary, indexed by the
// event's distance from the base; rows_ready_kernel, one workgroup, finds the horizon and the
// prefix over the summaries and writes the counts and the records; rows_zero_kernel, where the
// rule asks for it, zeroes what the prefix's rows hold beyond their whole events.  None of them
// writes a cell, the base or the window's counts.

static_assert(sizeof(e2sar_hip_rows_event) == 32 && offsetof(e2sar_hip_rows_event, row) == 24 &&
                  offsetof(e2sar_hip_rows_event, flags) == 28,
              "an event record is 32 bytes: eventNum, presentMask, openMask, row, flags");

// The work buffer: N summaries {present, open} of 16 bytes, then N words that are not 0 where
// a cell of the event has TRUNCATED (64 ids leave no spare bit in the masks).
constexpr size_t rows_ready_work_size(uint32_t nEvents)
{
    return ((size_t)nEvents * 20u + 255u) & ~(size_t)255u;
}
__device__ __forceinline__ uint8_t *rows_summary(void *work, uint32_t i) { return static_cast<uint8_t *>(work) + 16ull * i; }
__device__ __forceinline__ uint8_t *rows_trunc(void *work, uint32_t nEvents, uint32_t i)
{
    return static_cast<uint8_t *>(work) + 16ull * nEvents + 4ull * i;
}

// Thread i < nEvents: the cells of position i (event base + i * step), nIds 16-byte loads, as two masks and a word.
// Grid: cdiv(nEvents, kBlock).
__global__ __launch_bounds__(kBlock) void rows_scan_kernel(RowsDev W, void *work)
{
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= W.nEvents) return;
    const uint32_t i = (uint32_t)t;
    const uint64_t c0 = ((rows_base_index(W) + i) & (uint64_t)(W.nEvents - 1u)) * W.nIds;
    uint64_t present = 0, open = 0;
    uint32_t trunc = 0;
    for (uint32_t j = 0; j < W.nIds; j++) {
        const u32x4 v = ld16(reinterpret_cast<const uint8_t *>(W.cells + c0 + j));
        if (v.w & E2SAR_HIP_ROWS_COMPLETE) present |= 1ull << j;
        if (v.z != 0u) open |= 1ull << j;
        trunc |= v.w & E2SAR_HIP_ROWS_TRUNCATED;
    }
    st16(rows_summary(work, i), u32x4{(uint32_t)present, (uint32_t)(present >> 32), (uint32_t)open, (uint32_t)(open >> 32)});
    st4(rows_trunc(work, W.nEvents, i), trunc);
}

// The rule of a call as the kernels take it: required is never 0 (all nIds bits stand in)
struct RowsRule {
    uint64_t required;
    uint32_t slack, kMax;
};

struct RowsSummary {
    uint64_t present, open;
};
__device__ __forceinline__ RowsSummary rows_summary_of(void *work, uint32_t i)
{
    const u32x4 v = ld16(rows_summary(work, i));
    return RowsSummary{((uint64_t)v.y << 32) | v.x, ((uint64_t)v.w << 32) | v.z};
}
// complete: every required cell is COMPLETE; given up: not complete, behind the horizon H by
// at least `slack` events (i < H, so H - 1 - i does not wrap; a slack of all ones is never reached)
__device__ __forceinline__ bool rows_complete(const RowsSummary &s, const RowsRule &rule)
{
    return (s.present & rule.required) == rule.required;
}
__device__ __forceinline__ bool rows_given_up(const RowsSummary &s, const RowsRule &rule, uint32_t i, uint32_t H)
{
    return !rows_complete(s, rule) && i < H && H - 1u - i >= rule.slack;
}

// One workgroup of kBlock threads over the summaries:
//   1. the horizon H, one past the last event with an open cell: a strided pass, then a maximum;
//   2. k, the first event of [0, min(kMax, nEvents)) that is neither complete nor given up,
//      kBlock events at a time (block_first);
//   3. the counts of the k events and their records, a strided pass and four block sums.
// ready: 8 words; events: min(kMax, nEvents) records or NULL.
__global__ __launch_bounds__(kBlock) void rows_ready_kernel(RowsDev W, RowsRule rule, void *work, uint32_t *ready,
                                                            e2sar_hip_rows_event *events)
{
    constexpr int NW = kBlock / 64;
    __shared__ uint32_t part[NW];
    const uint32_t N = W.nEvents;

    uint32_t h = 0;
    for (uint32_t i = threadIdx.x; i < N; i += kBlock)
        if (rows_summary_of(work, i).open != 0ull) h = i + 1u;
    h = wave_max_u32(h);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = h;
    __syncthreads();
    uint32_t H = 0;
    for (uint32_t w = 0; w < (uint32_t)NW; w++) H = part[w] > H ? part[w] : H;
    __syncthreads();

    const uint32_t L = rule.kMax < N ? rule.kMax : N;
    uint32_t k = L;
    for (uint32_t i0 = 0; i0 < L; i0 += kBlock) {
        const uint32_t i = i0 + threadIdx.x;
        bool stops = true;                                        // the end of the range stops the prefix too
        if (i < L) {
            const RowsSummary s = rows_summary_of(work, i);
            stops = !rows_complete(s, rule) && !rows_given_up(s, rule, i, H);
        }
        const uint32_t cut = block_first<uint32_t, NW>(stops, i, part);
        __syncthreads();
        if (cut != ~0u) {
            k = cut < L ? cut : L;
            break;
        }
    }

    const uint64_t base = *W.base, qb = rows_base_index(W), step = rows_stride(W);
    uint32_t nComplete = 0, nGivenUp = 0, cellsComplete = 0, cellsOpen = 0;
    for (uint32_t i = threadIdx.x; i < k; i += kBlock) {
        const RowsSummary s = rows_summary_of(work, i);
        const bool complete = rows_complete(s, rule);
        nComplete += complete ? 1u : 0u;
        nGivenUp += complete ? 0u : 1u;
        cellsComplete += (uint32_t)__builtin_popcountll(s.present);
        cellsOpen += (uint32_t)__builtin_popcountll(s.open & ~s.present);
        if (events) {
            e2sar_hip_rows_event ev;
            ev.eventNum = base + i * step;
            ev.presentMask = s.present;
            ev.openMask = s.open;
            ev.row = (uint32_t)((qb + i) & (uint64_t)(N - 1u));
            ev.flags = (complete ? E2SAR_HIP_ROWS_EV_COMPLETE : E2SAR_HIP_ROWS_EV_GIVEN_UP) |
                       (ld4(rows_trunc(work, N, i)) ? E2SAR_HIP_ROWS_EV_TRUNCATED : 0u);
            events[i] = ev;
        }
    }
    uint32_t sums[4] = {nComplete, nGivenUp, cellsComplete, cellsOpen};
#pragma unroll
    for (int q = 0; q < 4; q++) {
        uint32_t total;
        block_excl_scan<uint32_t, NW>(sums[q], part, total);
        sums[q] = total;
        __syncthreads();
    }
    if (threadIdx.x < 8u) {
        const uint32_t words[8] = {k, sums[0], sums[1], H, sums[2], sums[3], 0u, 0u};
        uint32_t v = 0;
#pragma unroll
        for (uint32_t q = 0; q < 8u; q++) v = (threadIdx.x == q) ? words[q] : v;
        ready[threadIdx.x] = v;
    }
}

// Workgroup p: piece p % perCell (kCopyPiece bytes, copy_piece's) of cell (p / perCell) % nIds
// of position (p / perCell) / nIds behind the base.  Past k = ready[0]: one load and out.  A piece wholly
// inside the first min(bytes, pitch) bytes of a COMPLETE cell: two loads and out -- every
// workgroup of a loss-free batch of pitch-long events.  Otherwise zeros from the end of the
// event's bytes (from 0 where the cell is not COMPLETE) to the end of the piece: 16-byte
// stores, and the chunk the event ends in byte by byte, so that no event byte is read or
// rewritten.  Grid: min(kMax, nEvents) * nIds * perCell.
__global__ __launch_bounds__(kBlock) void rows_zero_kernel(RowsDev W, const uint32_t *__restrict__ ready, uint32_t perCell)
{
    const uint32_t c = blockIdx.x / perCell;
    const uint32_t e = c / W.nIds;
    if (e >= ready[0]) return;
    const uint32_t j = c - e * W.nIds;
    const uint64_t cell = ((rows_base_index(W) + e) & (uint64_t)(W.nEvents - 1u)) * W.nIds + j;
    const u32x4 v = ld16(reinterpret_cast<const uint8_t *>(W.cells + cell));
    const uint32_t keep = (v.w & E2SAR_HIP_ROWS_COMPLETE) ? (v.z < W.pitch ? v.z : W.pitch) : 0u;
    const uint32_t pb = (blockIdx.x - c * perCell) * kCopyPiece;
    const uint32_t pe = (W.pitch - pb < kCopyPiece) ? W.pitch : pb + kCopyPiece;
    if (keep >= pe) return;
    uint8_t *row = W.out + cell * W.pitch;
    const uint32_t whole = keep & ~15u, zeroFrom = (keep + 15u) & ~15u;
#pragma unroll
    for (int u = 0; u < kCopyU; u++) {
        const uint32_t i = pb + 16u * ((uint32_t)u * kBlock + threadIdx.x);
        if (i >= zeroFrom && i < pe) st16(row + i, u32x4{0u, 0u, 0u, 0u});
    }
    if (whole < keep && whole >= pb && threadIdx.x < 16u) {
        const uint32_t b = whole + threadIdx.x;
        if (b >= keep) st1(row + b, (uint8_t)0);
    }
}

}  // namespace e2sar_amd
