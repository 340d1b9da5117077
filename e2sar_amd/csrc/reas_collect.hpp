// reas_collect.hpp -- device-side delivery: the events a reassembler completed, packed into a caller's device buffer.
#pragma once

#include "dev_access.hpp"
#include "reas_upkeep.hpp"

namespace e2sar_amd {

// ---------------------------------------------------------------------------------
// collect: completed records [first, first + avail) leave the arena without a host round
// trip, as one ragged packed buffer (pitch == 0: event i at the sum of the earlier events'
// lengths, each rounded up to `align`) or as fixed-pitch rows (event i at i * pitch, cut to
// pitch bytes and zero-filled up to it).  Two launches: collect_plan_kernel lays the events
// out and writes the index table and the counts; collect_copy_kernel moves the bytes, one
// 8-KiB piece per workgroup as copy_spans_kernel does, on a grid the host sizes from bounds
// alone -- it knows neither how many events there are nor how long they are.

__host__ __device__ constexpr uint32_t collect_pieces(uint64_t extent)
{
    return (uint32_t)((extent + kCopyPiece - 1u) / kCopyPiece);
}

// The arena bytes are read once: streaming loads, as copy_spans_kernel's (the A/B against
// cache-allocating loads is in DESIGN.md 4.8).
__device__ __forceinline__ u32x4 collect_ld16(const uint8_t *p) { return ld16_nt(p); }

// One workgroup, 256 records per step (relay_plan_kernel's shape).  Per step: a block-wide
// scan of the padded extents on top of a 64-bit carry gives every record its offset; the
// capacity cut is the first record whose end would pass outBytes, and nothing after it is
// taken, even if it would fit (record order is kept); a second scan, over the taken records
// only, gives each its first copy piece -- the exclusive prefix of ceil(extent / 8 KiB),
// kept in the index record's `reserved` word, where collect_copy_kernel searches it.
//
// The plan is one body under two kernels.  collect_plan_kernel takes `first` from the host.
// collect_next_plan_kernel (CURSOR) reads it from a device word when it runs, takes nothing
// when outBytes is 0, and leaves the word grown by the n it took: the cursor of a consumer
// that never asks the host where it stands (e2sar_hip_reas_collect_next).
template <bool CURSOR>
__device__ __forceinline__ void collect_plan(const ReasDev &R, uint32_t first, uint32_t *cursor, uint32_t maxEvents,
                                             uint64_t outBytes, uint32_t pitch, uint32_t align,
                                             e2sar_hip_collect_rec *__restrict__ index, uint64_t *__restrict__ counts)
{
    constexpr int kWaves = kBlock / 64;
    __shared__ uint64_t wavePad[kWaves], waveTaken[kWaves], waveCopied[kWaves];
    __shared__ uint32_t wavePieces[kWaves], waveCut[kWaves];
    __shared__ uint32_t sAvail, sLimit, sFirst;
    if (threadIdx.x == 0) {
        if (CURSOR) first = *cursor;
        const CompletedWindow w = completed_window(R, first, maxEvents);
        uint32_t limit = w.taken;
        if (pitch && outBytes / pitch < limit) limit = (uint32_t)(outBytes / pitch);
        if (CURSOR && outBytes == 0) limit = 0;
        sAvail = w.avail;
        sLimit = limit;
        if (CURSOR) sFirst = first;
    }
    __syncthreads();
    const uint32_t limit = sLimit;
    if (CURSOR) first = sFirst;
    uint32_t n = limit, pieces = 0;
    uint64_t carry = 0, copied = 0;                        // bytes of `out` spanned, event bytes copied
    for (uint32_t b0 = 0; b0 < limit; b0 += kBlock) {
        const uint32_t i = b0 + threadIdx.x;
        const bool active = i < limit;
        e2sar_hip_event_rec rec{};
        if (active) rec = R.completed[first + i];
        const uint64_t extent = pitch ? (uint64_t)pitch : (uint64_t)rec.bytes;
        const uint64_t pad = !active ? 0ull : pitch ? (uint64_t)pitch : (((uint64_t)rec.bytes + align - 1u) & ~(uint64_t)(align - 1u));
        uint64_t stepPad, stepTaken, stepCopied;
        uint32_t stepPieces;
        const uint64_t off = carry + block_excl_scan<uint64_t, kWaves>(pad, wavePad, stepPad);
        // rows were cut by outBytes / pitch above; a ragged event must end inside the buffer
        const bool fits = !active || pitch || off + rec.bytes <= outBytes;
        const uint32_t cut = block_first<uint32_t, kWaves>(!fits, i, waveCut);
        const bool taken = active && i < cut;
        const uint32_t np = taken ? collect_pieces(extent) : 0u;
        const uint64_t cp = !taken ? 0ull : rec.bytes < extent ? (uint64_t)rec.bytes : extent;
        const uint32_t incNp = block_scan_post(np, wavePieces);      // three scans behind one barrier
        block_scan_post(taken ? pad : (uint64_t)0, waveTaken);
        block_scan_post(cp, waveCopied);
        __syncthreads();
        const uint32_t before = pieces + block_scan_before<uint32_t, kWaves>(wavePieces, stepPieces);
        block_scan_before<uint64_t, kWaves>(waveTaken, stepTaken);
        block_scan_before<uint64_t, kWaves>(waveCopied, stepCopied);
        if (taken) {
            e2sar_hip_collect_rec o;
            o.eventNum = rec.eventNum;
            o.outOffset = off;
            o.bytes = rec.bytes;
            o.dataId = rec.dataId;
            o.flags = (uint16_t)((pitch && rec.bytes > pitch) ? E2SAR_HIP_COLLECT_TRUNCATED : 0);
            o.numFragments = rec.numFragments;
            o.reserved = before + incNp - np;
            index[i] = o;
        }
        pieces += stepPieces;
        carry += stepTaken;
        copied += stepCopied;
        if (cut != ~0u) {                                   // the same in every thread
            n = cut;
            break;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        counts[0] = n;
        counts[1] = carry;
        counts[2] = sAvail - n;
        counts[3] = copied;
        if (CURSOR) *cursor = first + n;
    }
}

__global__ __launch_bounds__(kBlock) void collect_plan_kernel(ReasDev R, uint32_t first, uint32_t maxEvents,
                                                              uint64_t outBytes, uint32_t pitch, uint32_t align,
                                                              e2sar_hip_collect_rec *__restrict__ index,
                                                              uint64_t *__restrict__ counts)
{
    collect_plan<false>(R, first, nullptr, maxEvents, outBytes, pitch, align, index, counts);
}

__global__ __launch_bounds__(kBlock) void collect_next_plan_kernel(ReasDev R, uint32_t *__restrict__ cursor,
                                                                   uint32_t maxEvents, uint64_t outBytes, uint32_t pitch,
                                                                   uint32_t align, e2sar_hip_collect_rec *__restrict__ index,
                                                                   uint64_t *__restrict__ counts)
{
    collect_plan<true>(R, 0u, cursor, maxEvents, outBytes, pitch, align, index, counts);
}

// One workgroup per 8-KiB piece of one event's extent (its bytes, or its row of `pitch`).
// The grid comes from bounds, so a workgroup first reads what collect_plan_kernel wrote on
// the stream before it: the event count, and from the last index record the piece total; a
// workgroup past the total exits.  The others find their event -- a row's by division, a
// ragged event's by binary search over the piece prefix, log2(n) workgroup-uniform loads of a
// table that sits in L2 -- and copy the piece as copy_spans_kernel does: every thread issues
// its kCopyU 16-byte loads before any store.  Arena event buffers are 256-byte aligned and
// outOffset at least 16-byte aligned, so there is no unaligned form.  Whole 16-byte chunks
// of the event are copied, the last bytes mod 16 go as byte stores (no load or store touches
// a byte past the event), and in row mode everything from the event's end to the pitch is
// stored as zeros.  The loop is a guard, not the plan: should the bounds ever undercount the
// pieces, the grid strides over the rest.
// The search and the piece are last_prefix_le and copy_piece (build_copy_kernel calls them),
// kept here in this kernel's own text: on the shared helpers, with the zero tail a run-time
// flag and as a template argument, a collect case measured outside the parent's bound
// (DESIGN.md 4.5).
__global__ __launch_bounds__(kBlock) void collect_copy_kernel(const uint8_t *__restrict__ arena,
                                                              const e2sar_hip_event_rec *__restrict__ completed,
                                                              uint8_t *__restrict__ out, uint32_t pitch,
                                                              const e2sar_hip_collect_rec *__restrict__ index,
                                                              const uint64_t *__restrict__ counts)
{
    const uint32_t n = (uint32_t)counts[0];
    if (n == 0) return;
    const uint32_t perRow = collect_pieces(pitch);
    const uint32_t total = index[n - 1u].reserved + (pitch ? perRow : collect_pieces(index[n - 1u].bytes));
    for (uint32_t p = blockIdx.x; p < total; p += gridDim.x) {
        uint32_t ev = 0;
        if (pitch) {
            ev = p / perRow;
        } else {
            uint32_t hi = n;                                // the last event whose first piece is <= p
            while (hi - ev > 1u) {
                const uint32_t mid = (ev + hi) >> 1;
                if (index[mid].reserved <= p) ev = mid;
                else hi = mid;
            }
        }
        const uint64_t dstOff = index[ev].outOffset;
        const uint32_t bytes = index[ev].bytes;
        const uint8_t *src = arena + completed[ev].arenaOffset;
        uint8_t *dst = out + dstOff;
        const uint64_t extent = pitch ? pitch : bytes;
        const uint64_t cp = bytes < extent ? bytes : extent;                  // event bytes in the extent
        const uint64_t whole = cp & ~15ull, zeroFrom = (cp + 15ull) & ~15ull;
        const uint64_t base = (uint64_t)(p - index[ev].reserved) * kCopyPiece;
        u32x4 x[kCopyU];
#pragma unroll
        for (int u = 0; u < kCopyU; u++) {
            const uint64_t i = base + 16ull * ((uint64_t)u * kBlock + threadIdx.x);
            x[u] = (i + 16 <= whole) ? collect_ld16(src + i) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int u = 0; u < kCopyU; u++) {
            const uint64_t i = base + 16ull * ((uint64_t)u * kBlock + threadIdx.x);
            if (i + 16 <= whole || (i >= zeroFrom && i < extent)) st16_nt(dst + i, x[u]);
        }
        // the chunk the event ends in: its bytes one by one, and in a row zeros up to the chunk's end
        if (whole < cp && whole >= base && whole - base < kCopyPiece && threadIdx.x < 16u) {
            const uint64_t b = whole + threadIdx.x;
            if (b < cp) st1(dst + b, ld1(src + b));
            else if (pitch) st1(dst + b, (uint8_t)0);
        }
    }
}

// collect_copy_kernel for e2sar_hip_reas_collect_next: the first taken record is not the
// host's to name -- it is the cursor collect_next_plan_kernel left, minus the n it took, from
// the list's base.  The same pieces, found and moved by the shared helpers; collect_copy_kernel
// keeps its own text, instruction for instruction, and so what it measured.
__global__ __launch_bounds__(kBlock) void collect_next_copy_kernel(const uint8_t *__restrict__ arena,
                                                                   const e2sar_hip_event_rec *__restrict__ completed,
                                                                   const uint32_t *__restrict__ cursor,
                                                                   uint8_t *__restrict__ out, uint32_t pitch,
                                                                   const e2sar_hip_collect_rec *__restrict__ index,
                                                                   const uint64_t *__restrict__ counts)
{
    const uint32_t n = (uint32_t)counts[0];
    if (n == 0) return;
    completed += *cursor - n;
    const uint32_t perRow = collect_pieces(pitch);
    const uint32_t total = index[n - 1u].reserved + (pitch ? perRow : collect_pieces(index[n - 1u].bytes));
    for (uint32_t p = blockIdx.x; p < total; p += gridDim.x) {
        const uint32_t ev = pitch ? p / perRow : last_prefix_le(p, n, [&](uint32_t i) { return index[i].reserved; });
        const uint32_t bytes = index[ev].bytes;
        const uint8_t *src = arena + completed[ev].arenaOffset;
        uint8_t *dst = out + index[ev].outOffset;
        const uint64_t base = (uint64_t)(p - index[ev].reserved) * kCopyPiece;
        if (pitch) copy_piece<true>(src, dst, bytes < pitch ? bytes : pitch, pitch, base);
        else copy_piece<false>(src, dst, bytes, bytes, base);
    }
}

}  // namespace e2sar_amd
