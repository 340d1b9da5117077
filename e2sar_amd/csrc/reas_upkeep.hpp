// reas_upkeep.hpp -- upkeep kernels: zero / fill / copy-spans, GC, recycle, compaction, relay plan.
#pragma once

#include "dev_access.hpp"
#include "reas_table.hpp"

namespace e2sar_amd {

// Zero nWords dwords.  Used instead of hipMemsetAsync wherever the launch may be captured
// into a HIP graph: on this ROCm captured hipMemsetAsync nodes write garbage from the
// second replay on (fill_bytes_kernel below).
__global__ __launch_bounds__(kBlock) void zero_words_kernel(uint32_t *p, uint64_t nWords)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nWords; i += (uint64_t)gridDim.x * kBlock)
        p[i] = 0u;
}

// Fill bytes [p, p + n) with v: bytes up to the first 16-byte boundary and after the last,
// 16-byte stores in between.  e2sar_hip_memset_d uses it instead of hipMemsetAsync: on this
// ROCm a captured hipMemsetAsync node of 64 bytes or more writes garbage from the second
// graph replay on (tools/graph_memset_probe.py); a kernel node replays clean.
__global__ __launch_bounds__(kBlock) void fill_bytes_kernel(uint8_t *p, uint8_t v, uint64_t n)
{
    const uint64_t head = ((16u - ((uintptr_t)p & 15u)) & 15u) < n ? ((16u - ((uintptr_t)p & 15u)) & 15u) : n;
    const uint64_t body = (n - head) & ~15ull;
    const uint64_t t0 = (uint64_t)blockIdx.x * kBlock + threadIdx.x, step = (uint64_t)gridDim.x * kBlock;
    if (t0 < head) st1(p + t0, v);
    const uint64_t tail0 = head + body;
    if (t0 < n - tail0) st1(p + tail0 + t0, v);
    const uint32_t w = 0x01010101u * v;
    const u32x4 q{w, w, w, w};
    for (uint64_t i = t0; i < body / 16u; i += step) st16(p + head + 16u * i, q);
}

// One 8-KiB piece of a copy, by one workgroup of kBlock threads: every thread issues its two
// 16-byte non-temporal loads before any store, as seg_kernel does, so a large copy streams
// at the plain-copy rate (the bench's HBM calibration copies 1 and 4 GiB with it).  8-KiB
// pieces copy faster than 16-KiB ones on random bytes (tools/ubench_store.hip: 6.06 vs 5.99
// TB/s at 1 GiB, 6.21 vs 5.99 at 4 GiB).
constexpr int kCopyU = 2;
constexpr uint32_t kCopyPiece = (uint32_t)kBlock * 16u * kCopyU;

// The piece that starts `base` bytes into an extent of `extent` bytes at dst, which holds cp
// event bytes from src and, with ZERO_TAIL, zeros behind them up to its end (a row or a cell;
// without, the extent ends with the bytes: a ragged event).  src, dst and a zeroed extent's
// length are 16-byte aligned.  The discipline of every copy that delivers events: all kCopyU
// loads of a thread before any store; whole 16-byte chunks of the event go as 16-byte stores,
// its last bytes mod 16 as byte stores; no byte past the event is loaded, none past the
// extent stored.  The source is read once: streaming loads (collect's A/B against
// cache-allocating loads is in DESIGN.md 4.8).  build_copy_kernel's piece; collect_copy_kernel
// and copy_spans_kernel hold the same body in their own text.
template <bool ZERO_TAIL>
__device__ __forceinline__ void copy_piece(const uint8_t *src, uint8_t *dst, uint64_t cp, uint64_t extent, uint64_t base)
{
    const uint64_t whole = cp & ~15ull, zeroFrom = (cp + 15ull) & ~15ull;
    u32x4 x[kCopyU];
#pragma unroll
    for (int u = 0; u < kCopyU; u++) {
        const uint64_t i = base + 16ull * ((uint64_t)u * kBlock + threadIdx.x);
        x[u] = (i + 16 <= whole) ? ld16_nt(src + i) : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int u = 0; u < kCopyU; u++) {
        const uint64_t i = base + 16ull * ((uint64_t)u * kBlock + threadIdx.x);
        if (i + 16 <= whole || (ZERO_TAIL && i >= zeroFrom && i < extent)) st16_nt(dst + i, x[u]);
    }
    // the chunk the event ends in: its bytes one by one, and with ZERO_TAIL zeros up to the chunk's end
    if (whole < cp && whole >= base && whole - base < kCopyPiece && threadIdx.x < 16u) {
        const uint64_t b = whole + threadIdx.x;
        if (b < cp) st1(dst + b, ld1(src + b));
        else if (ZERO_TAIL) st1(dst + b, (uint8_t)0);
    }
}

// Gather copy: blockIdx.y = span, blockIdx.x = its 8-KiB piece; 16-byte loads and stores when
// both ends are 16-byte aligned (arena event buffers are 256-aligned; callers lay
// destinations out 64-aligned), bytes otherwise and for the tail.  The aligned body is
// copy_piece's, kept in its own text: the unaligned fallback and the tail loop are this
// kernel's alone, and with copy_piece as the body (122 instructions for 104) one case of the
// gather measured outside the parent's bound.
__global__ __launch_bounds__(kBlock) void copy_spans_kernel(CopySpans cs)
{
    if (blockIdx.y >= cs.n) return;
    const CopySpan sp = cs.s[blockIdx.y];
    const uint64_t base = (uint64_t)blockIdx.x * kCopyPiece;
    if (base >= sp.bytes) return;
    const uint8_t *src = reinterpret_cast<const uint8_t *>(sp.src);
    uint8_t *dst = reinterpret_cast<uint8_t *>(sp.dst);
    const uint64_t end = (base + kCopyPiece < sp.bytes) ? base + kCopyPiece : sp.bytes;
    uint64_t b0 = base;
    if (((sp.src | sp.dst) & 15u) == 0) {
        const uint64_t whole = sp.bytes & ~15ull;
        u32x4 x[kCopyU];
#pragma unroll
        for (int u = 0; u < kCopyU; u++) {
            const uint64_t i = base + 16ull * ((uint64_t)u * kBlock + threadIdx.x);
            x[u] = (i + 16 <= whole) ? ld16_nt(src + i) : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int u = 0; u < kCopyU; u++) {
            const uint64_t i = base + 16ull * ((uint64_t)u * kBlock + threadIdx.x);
            if (i + 16 <= whole) st16_nt(dst + i, x[u]);
        }
        b0 = (whole > base) ? ((whole < end) ? whole : end) : base;
    }
    for (uint64_t b = b0 + threadIdx.x; b < end; b += kBlock) dst[b] = src[b];
}

// ---------------------------------------------------------------------------------
// GC / recycle

__global__ __launch_bounds__(kBlock) void reas_gc_kernel(ReasDev R, uint64_t now, uint64_t timeout)
{
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= R.tableSlots) return;
    ReasSlot *sl = R.slots + s;
    if (ld_agent(&sl->state) != kReady) return;
    const uint64_t created = ld_agent(&sl->created);
    if (now <= created || now - created <= timeout) return;     // inWaiting > timeout (cpp:262)
    if (atomicCAS(&sl->state, (uint32_t)kReady, (uint32_t)kLost) != kReady) return;
    atomicAdd(&R.ctl->reassemblyLoss, 1ull);
    atomicAdd(occ_in_progress(R, s), ~0ull);
    const uint32_t li = atomicAdd(&R.ctl->nLost, 1u);
    if (li < R.lostCapacity) {
        e2sar_hip_lost_rec rec;
        rec.eventNum = ld_agent(&sl->eventNum);
        rec.numFragments = ld_agent(&sl->acc) >> kAccFragShift;
        rec.dataId = (uint16_t)ld_agent(&sl->dataId);
        rec.enqueueLoss = 0;
        rec.reserved = 0;
        R.lost[li] = rec;
    }
}

__global__ __launch_bounds__(kBlock) void reas_recycle_kernel(ReasDev R, int dropCompleted)
{
    recycle_slots(R, blockIdx.x * kBlock + threadIdx.x, dropCompleted);
}

// Compaction: one block per slot of `from`.  Surviving (READY) events get a new buffer
// at the bottom of the `to` arena and a slot in the (empty) `to` table; their partial
// bytes are copied whole.  Nothing else touches either table during this launch, so the
// insert needs only the CAS for slot ownership among compacting blocks.
__global__ __launch_bounds__(kBlock) void reas_compact_kernel(ReasDev from, ReasDev to)
{
    __shared__ uint64_t sOff;
    const ReasSlot *sl = from.slots + blockIdx.x;
    if (sl->state != kReady) return;
    const uint32_t bytes = sl->bytes;
    if (threadIdx.x == 0) {
        uint64_t off = kNoBuf;
        if (sl->bufOff != kNoBuf) {
            const uint64_t need = ((uint64_t)bytes + 255ull) & ~255ull;
            off = atomicAdd(&to.ctl->compactTop, (unsigned long long)(need ? need : 256ull));
            if (off + bytes > to.arenaBytes) {
                off = kNoBuf;                      // cannot happen when to.arenaBytes >= from.arenaBytes
                atomicOr(&to.ctl->errorFlags, 2u);
            }
        }
        const uint32_t mask = to.tableSlots - 1u;
        uint32_t h = slot_hash(sl->eventNum, sl->dataId, mask);
        for (uint32_t probe = 0; probe < to.tableSlots; probe++, h = (h + 1u) & mask) {
            if (atomicCAS(&to.slots[h].state, (uint32_t)kEmpty, (uint32_t)kBusy) == kEmpty) {
                ReasSlot *d = to.slots + h;
                d->dataId = sl->dataId;
                d->bytes = bytes;
                d->eventNum = sl->eventNum;
                d->acc = sl->acc;
                d->bufOff = off;
                d->bvalid = 1u;
                d->created = sl->created;
                d->state = kReady;
                atomicAdd(&to.ctl->compactUsed, 1u);
                break;
            }
        }
        sOff = off;
    }
    __syncthreads();
    const uint64_t off = sOff;
    if (off == kNoBuf || sl->bufOff == kNoBuf) return;
    const uint8_t *src = from.arena + sl->bufOff;
    uint8_t *dst = to.arena + off;
    const uint32_t n16 = bytes >> 4;
    for (uint32_t i = threadIdx.x; i < n16; i += kBlock) st16(dst + 16u * i, ld16(src + 16u * i));
    for (uint32_t b = (n16 << 4) + threadIdx.x; b < bytes; b += kBlock) st1(dst + b, ld1(src + b));
}

__global__ void reas_compact_finish(ReasDev to)
{
    to.ctl->arenaTop = to.ctl->compactTop;
    to.ctl->tableUsed = to.ctl->compactUsed;
    for (uint32_t k = 0; k < kShards; k++) *occ_table_used(to, k) = 0ull;
    to.ctl->compactTop = 0;
    to.ctl->compactUsed = 0;
}

// ---------------------------------------------------------------------------------
// relay: the events a reassembler completed become a segmentation batch on the device
//
// One workgroup reads completed records [first, first + n) (n = min(maxEvents, records
// stored - first)), writes one seg descriptor per event -- the event's arena bytes, its RE
// eventNum and dataId as received, the batch's LB tick, entropy entropyBase + i -- with
// pktBase the exclusive prefix of ceil(bytes / maxPld) (a block-wide scan, 256 records per
// step), and counts[0] = n, counts[1] = the batch's datagram count.

// The completed-record window of a plan kernel, read by its one thread: the records stored
// from `first` on, and how many of them a plan bounded by `bound` takes.
struct CompletedWindow {
    uint32_t avail, taken;
};
__device__ __forceinline__ CompletedWindow completed_window(const ReasDev &R, uint32_t first, uint32_t bound)
{
    uint32_t stored = ld_agent(&R.ctl->nCompleted);
    if (stored > R.queueCapacity) stored = R.queueCapacity;            // records past it were lost
    const uint32_t avail = stored > first ? stored - first : 0u;
    return {avail, avail < bound ? avail : bound};
}

__global__ __launch_bounds__(kBlock) void relay_plan_kernel(ReasDev R, uint32_t first, uint32_t maxEvents,
                                                            uint32_t maxPld, uint64_t lbTick, uint32_t entropyBase,
                                                            e2sar_hip_seg_event *__restrict__ out,
                                                            uint32_t *__restrict__ counts)
{
    __shared__ uint32_t waveSum[kBlock / 64];
    __shared__ uint32_t sN;
    if (threadIdx.x == 0) sN = completed_window(R, first, maxEvents).taken;
    __syncthreads();
    const uint32_t n = sN;
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += kBlock) {
        const uint32_t i = b0 + threadIdx.x;
        e2sar_hip_event_rec rec{};
        if (i < n) rec = R.completed[first + i];
        const uint32_t np = (i < n) ? rec.bytes / maxPld + (rec.bytes % maxPld != 0u) : 0u;
        uint32_t step;
        const uint32_t before = block_excl_scan<uint32_t, kBlock / 64>(np, waveSum, step);
        if (i < n) {
            e2sar_hip_seg_event d;
            d.data = R.arena + rec.arenaOffset;
            d.eventNum = rec.eventNum;
            d.lbTick = lbTick;
            d.bytes = rec.bytes;
            d.pktBase = carry + before;
            d.dataId = rec.dataId;
            d.entropy = (uint16_t)(entropyBase + i);
            d.reserved = 0;
            out[i] = d;
        }
        carry += step;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        counts[0] = n;
        counts[1] = carry;
    }
}

}  // namespace e2sar_amd
