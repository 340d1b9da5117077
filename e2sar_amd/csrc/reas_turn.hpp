// reas_turn.hpp -- the turn: upkeep decided and done on the device, events in progress kept.
#pragma once

#include "dev_access.hpp"
#include "reas_table.hpp"
#include "reas_upkeep.hpp"

namespace e2sar_amd {

// ---------------------------------------------------------------------------------
// turn (e2sar_hip_reas_turn): what recycle(force = 0) and compact do behind a host wait and a
// read-back of ReasCtl, as four launches whose number and grids do not depend on device
// state, so that a graph holds them.  The first decides; every workgroup of the other three
// reads the verdict first and exits unless it is kTurnRan.
//
//   turn_decide_kernel  zeroes the alternate table (unseen by anything but compact and the
//                       turn; a host compact may have left it used), and its first thread
//                       writes the verdict to status[0]
//   turn_out_kernel     one thread per slot of the current table: an event in progress is
//                       aged out (as reas_gc_kernel loses one) or carried -- a buffer at the
//                       bottom of the alternate arena, its entry with the carry count + 1 in
//                       the alternate table, and one TurnMove in the move list
//   turn_copy_kernel    the moves' bytes, current arena -> alternate, spread over a fixed grid
//   turn_back_kernel    current slot s becomes alternate slot s, empty where that is empty --
//                       a table without tombstones, copied slot for slot, is a valid table, and
//                       this is also the clear -- and the moves' bytes return at the offsets
//                       they were given, so the current table and arena stay the ones every
//                       captured launch points at; one thread re-bases counters, list and cursor
//
// Only events in progress move, twice; next to a stream they are few.  The carry count of an
// event sits in ReasSlot::pad1[0]: zero when the slot is claimed (a slot is EMPTY only after
// it was zeroed), never written by find_or_create.

enum : uint64_t { kTurnSkipped = 0, kTurnRan = 1, kTurnUnconsumed = 2 };
constexpr uint32_t kNeverLost = 0xFFFFFFFFu;
constexpr uint32_t kTurnCopyGroups = 2048;         // workgroups that share the moves' bytes: 8 per CU

struct TurnMarks {
    uint64_t arenaMark;
    uint32_t recordMark, tableMark, maxCarries;
};

// One survivor's bytes: `bytes` from `src` in the current arena to `dst` in the alternate one,
// and back to `dst` in the current.  The list has tableSlots entries (e2sar_hip_reas_create).
struct TurnMove {
    uint64_t src, dst;
    uint32_t bytes, pad[3];
};
static_assert(sizeof(TurnMove) == 32, "two dwordx4 per move");

__global__ __launch_bounds__(kBlock) void turn_decide_kernel(ReasDev R, ReasSlot *__restrict__ altSlots,
                                                             const uint32_t *__restrict__ cursor, TurnMarks M,
                                                             uint64_t *__restrict__ status)
{
    const uint64_t nWords = (uint64_t)R.tableSlots * (sizeof(ReasSlot) / 16u);
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < nWords; i += (uint64_t)gridDim.x * kBlock)
        st16(reinterpret_cast<uint8_t *>(altSlots) + 16ull * i, u32x4{0u, 0u, 0u, 0u});
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t stored = ld_agent(&R.ctl->nCompleted);
    if (stored > R.queueCapacity) stored = R.queueCapacity;            // records past it were lost
    const uint64_t top = ld_agent(&R.ctl->arenaTop);
    uint64_t verdict = kTurnSkipped;
    if (*cursor < stored) {
        verdict = kTurnUnconsumed;                  // their records point into the arena: it stays
    } else {
        long long used = ld_agent(&R.ctl->tableUsed);
        for (uint32_t k = 0; k < kShards; k++) used += (long long)*occ_table_used(R, k);
        if (top >= M.arenaMark || stored >= M.recordMark || used >= (long long)M.tableMark) verdict = kTurnRan;
    }
    if (verdict == kTurnRan) {
        R.ctl->compactTop = 0;
        R.ctl->compactUsed = 0;
        R.ctl->turnAged = 0;
        R.ctl->turnMoves = 0;
    }
    status[0] = verdict;
    status[1] = 0;
    status[2] = 0;
    status[3] = top;
}

// Nothing else touches either table during this launch (the stream orders it), so the insert
// needs only the CAS for slot ownership among this launch's threads, as reas_compact_kernel's.
__global__ __launch_bounds__(kBlock) void turn_out_kernel(ReasDev from, ReasDev to, uint32_t maxCarries,
                                                          TurnMove *__restrict__ moves, const uint64_t *__restrict__ status)
{
    if (status[0] != kTurnRan) return;
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= from.tableSlots) return;
    const ReasSlot *sl = from.slots + s;
    if (sl->state != kReady) return;
    const uint32_t bytes = sl->bytes;
    const uint64_t carries = sl->pad1[0];
    if (maxCarries != kNeverLost && carries >= maxCarries) {
        // aged out: reas_gc_kernel's loss, word for word (turn_back_kernel clears the slot)
        atomicAdd(&from.ctl->reassemblyLoss, 1ull);
        atomicAdd(occ_in_progress(from, s), ~0ull);
        atomicAdd(&from.ctl->turnAged, 1u);
        const uint32_t li = atomicAdd(&from.ctl->nLost, 1u);
        if (li < from.lostCapacity) {
            e2sar_hip_lost_rec rec;
            rec.eventNum = sl->eventNum;
            rec.numFragments = sl->acc >> kAccFragShift;
            rec.dataId = (uint16_t)sl->dataId;
            rec.enqueueLoss = 0;
            rec.reserved = 0;
            from.lost[li] = rec;
        }
        return;
    }
    uint64_t off = kNoBuf;                         // a survivor without a buffer stays without one
    if (sl->bufOff != kNoBuf) {
        const uint64_t need = ((uint64_t)bytes + 255ull) & ~255ull;
        off = atomicAdd(&to.ctl->compactTop, (unsigned long long)(need ? need : 256ull));
        if (off + bytes > to.arenaBytes) {
            off = kNoBuf;                          // cannot happen: the survivors' buffers lay apart in an arena as large
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
            d->pad1[0] = carries + 1u;
            d->state = kReady;
            atomicAdd(&to.ctl->compactUsed, 1u);
            break;
        }
    }
    if (off != kNoBuf && bytes != 0u) {
        const uint32_t mi = atomicAdd(&to.ctl->turnMoves, 1u);      // below tableSlots: one per slot at most
        moves[mi] = TurnMove{sl->bufOff, off, bytes, {0u, 0u, 0u}};
    }
}

// The moves' bytes from arena `a` to arena `b`, by gridDim.x workgroups from `first` on: with
// fewer moves than workgroups every move is shared by gridDim.x / n of them, 8-KiB pieces dealt
// round; else every workgroup takes whole moves.  copy_piece's discipline; event buffers are
// 256-byte aligned in both arenas.
template <bool BACK>
__device__ __forceinline__ void turn_copy(const uint8_t *a, uint8_t *b, const TurnMove *__restrict__ moves, uint32_t n,
                                          uint32_t w, uint32_t groups)
{
    if (n == 0) return;
    const uint32_t share = n < groups ? groups / n : 1u;
    if (w / n >= share && n < groups) return;
    for (uint32_t e = n < groups ? w % n : w; e < n; e += groups) {
        const TurnMove m = moves[e];
        const uint32_t pieces = (uint32_t)(((uint64_t)m.bytes + kCopyPiece - 1u) / kCopyPiece);
        for (uint32_t p = n < groups ? w / n : 0u; p < pieces; p += share)
            copy_piece<false>(a + (BACK ? m.dst : m.src), b + m.dst, m.bytes, m.bytes, (uint64_t)p * kCopyPiece);
    }
}

__global__ __launch_bounds__(kBlock) void turn_copy_kernel(const uint8_t *__restrict__ arena, uint8_t *__restrict__ altArena,
                                                           const ReasCtl *__restrict__ ctl, const TurnMove *__restrict__ moves,
                                                           const uint64_t *__restrict__ status)
{
    if (status[0] != kTurnRan) return;
    turn_copy<false>(arena, altArena, moves, ctl->turnMoves, blockIdx.x, gridDim.x);
}

// from: the alternate table and arena, as turn_out_kernel and turn_copy_kernel left them; to:
// the current ones.  Workgroups [0, tableGroups): the table, one thread per slot, and the
// first thread the counters -- nothing in this launch reads what it writes; the rest: the bytes.
__global__ __launch_bounds__(kBlock) void turn_back_kernel(ReasDev from, ReasDev to, uint32_t tableGroups,
                                                           const TurnMove *__restrict__ moves, uint32_t *__restrict__ cursor,
                                                           uint64_t *__restrict__ status)
{
    if (status[0] != kTurnRan) return;
    if (blockIdx.x >= tableGroups) {
        turn_copy<true>(from.arena, to.arena, moves, to.ctl->turnMoves, blockIdx.x - tableGroups, gridDim.x - tableGroups);
        return;
    }
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    if (s < to.tableSlots) {
        // the slot as four 16-byte words (a ReasSlot held by value would live in scratch)
        const uint8_t *a = reinterpret_cast<const uint8_t *>(from.slots + s);
        uint8_t *b = reinterpret_cast<uint8_t *>(to.slots + s);
        u32x4 q[4];
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = ld16(a + 16 * k);
        const bool keep = q[0].x == kReady;                    // record A's first word: the state
#pragma unroll
        for (int k = 0; k < 4; k++) st16(b + 16 * k, keep ? q[k] : u32x4{0u, 0u, 0u, 0u});
    }
    if (s != 0) return;
    ReasCtl *c = to.ctl;
    const uint64_t top = c->compactTop;
    const uint32_t used = c->compactUsed;
    c->arenaTop = top;
    c->tableUsed = used;
    for (uint32_t k = 0; k < kShards; k++) *occ_table_used(to, k) = 0ull;
    c->nCompleted = 0;
    *cursor = 0;
    status[1] = used;
    status[2] = c->turnAged;
    status[3] = top;
    c->compactTop = 0;
    c->compactUsed = 0;
    c->turnAged = 0;
}

}  // namespace e2sar_amd
