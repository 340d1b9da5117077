// reas_table.hpp -- the event table protocol: slot states, lookup / insert, completion, recycling.
#pragma once

#include "dev_access.hpp"

namespace e2sar_amd {

// ---------------------------------------------------------------------------------
// reassembly: event table protocol
//
// slot.state: EMPTY -> BUSY (CAS by the inserting lane) -> READY (published with the key)
// -> DONE (completed) / LOST (GC'd).  A lookup claims first: CAS EMPTY->BUSY either makes
// the lane the creator (one round trip) or returns the slot's state.  The creator takes its
// buffer from the arena and publishes record B {bufOff, bytes, bvalid=1} and record A
// {READY, dataId, eventNum} as two 16-byte agent-scope (sc1) stores, without waiting for
// them; other lanes read A and B together (two sc1 loads, one round trip) until A is READY
// and B valid.  acc starts at 0 because a slot is EMPTY only after it was zeroed (slots
// are never reused within an arena epoch).

enum : uint32_t { kEmpty = 0, kBusy = 1, kReady = 2, kDone = 3, kLost = 4 };

// occupancy shard of a table slot (ReasOcc follows the ReasShard array)
__device__ __forceinline__ unsigned long long *occ_in_progress(const ReasDev &R, uint32_t slot)
{
    return reinterpret_cast<unsigned long long *>(&(reinterpret_cast<ReasOcc *>(R.shards + kShards) + slot % kShards)->inProgress);
}
__device__ __forceinline__ unsigned long long *occ_table_used(const ReasDev &R, uint32_t slot)
{
    return reinterpret_cast<unsigned long long *>(&(reinterpret_cast<ReasOcc *>(R.shards + kShards) + slot % kShards)->tableUsed);
}
// 16-byte agent-scope store and the pair of 16-byte agent-scope loads of records A and B
// (the forms the compiler emits for 4/8-byte agent-scope atomics, at 16 bytes).  The
// loads wait for their own results inside the asm.
__device__ __forceinline__ void st16_agent(void *p, u32x4 v)
{
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void ld_slot_ab(const ReasSlot *sl, u32x4 &A, u32x4 &B)
{
    asm volatile("global_load_dwordx4 %0, %2, off sc1\n\t"
                 "global_load_dwordx4 %1, %2, off offset:16 sc1\n\t"
                 "s_waitcnt vmcnt(0)"
                 : "=&v"(A), "=&v"(B)
                 : "v"(sl)
                 : "memory");
}

__device__ __forceinline__ uint32_t slot_hash(uint64_t ev, uint32_t d, uint32_t mask)
{
    // pair_hash (e2sarUtil.hpp:526-533) then a 64-bit finaliser so that event numbers
    // that differ only in high bits (ticks) or in dataId spread over the table.
    uint64_t t = d;
    uint64_t h = ev ^ (t | t << 16 | t << 32 | t << 48);
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    return (uint32_t)h & mask;
}

struct LookupResult {
    uint32_t slot;      // kNoSlot on failure
    uint32_t bytes;     // slot's bufferLength (from the packet that created it)
    uint64_t bufOff;    // arena offset or kNoBuf
};
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr uint64_t kNoBuf = ~0ull;
constexpr uint32_t kSpinLimit = 1u << 22;

// Record B's bvalid in reference-order mode for a key registered by ro_key_kernel whose
// event item (buffer, counters) does not exist yet: ro_walk_kernel creates items.
constexpr uint32_t kBNoItem = 2u;

// Called by a whole wave: lanes with want == false only take part in the loop.  The wave
// loops until every wanting lane has a result, and every pass is straight-line (claim;
// creators publish; the others read), so a lane never waits inside a divergent branch
// for a slot that another lane of the same wave is still creating.
// keyOnly (reference-order mode): a creator registers the key without an event buffer
// (record B = {kNoBuf, 0, kBNoItem}); the walk that follows creates the items.
template <bool keyOnly = false>
__device__ LookupResult find_or_create(const ReasDev &R, bool want, uint64_t ev, uint32_t d, uint32_t blen,
                                       uint64_t now)
{
    LookupResult res{kNoSlot, 0, kNoBuf};
    const uint32_t mask = R.tableSlots - 1u;
    uint32_t h = slot_hash(ev, d, mask);
    uint32_t probes = 0, spins = 0;
    bool active = want;
#if E2SAR_TRACE
    uint32_t pass = 0;
#endif
    bool claimed = false;          // the current slot is known to be past EMPTY: poll by loads
    while (__ballot(active)) {
        bool waiting = false, advance = false;
        if (active) {
            ReasSlot *sl = R.slots + h;
            // a slot never returns to EMPTY within an arena epoch, so once a claim has
            // failed, later passes poll records A/B with loads instead of repeating the CAS
            // (A/B: +1.1 % at 1 MiB / MTU 1500, +1.8 % at 8 MiB / MTU 9000)
            const uint32_t old = claimed ? (uint32_t)kBusy : atomicCAS(&sl->state, (uint32_t)kEmpty, (uint32_t)kBusy);
#if E2SAR_TRACE
            if (pass == 0) {
                TRACE_WAIT();
                TRACE_FIRST(2, 1, trace_now());
            }
#endif
            if (old == kEmpty && keyOnly) {
                st16_agent(&sl->bufOff, u32x4{(uint32_t)kNoBuf, (uint32_t)(kNoBuf >> 32), 0u, kBNoItem});
                st16_agent(sl, u32x4{(uint32_t)kReady, d, (uint32_t)ev, (uint32_t)(ev >> 32)});
                atomicAdd(occ_table_used(R, h), 1ull);
                res.slot = h;
                active = false;
            } else if (old == kEmpty) {
                // this lane owns the slot: buffer, then records B and A
                const uint64_t need = ((uint64_t)blen + 255ull) & ~255ull;
                uint64_t boff = atomicAdd(&R.ctl->arenaTop, (unsigned long long)(need ? need : 256ull));
                if (boff + blen > R.arenaBytes) {
                    boff = kNoBuf;
                    atomicOr(&R.ctl->errorFlags, 2u);
                }
                st_agent(&sl->created, now);
                st16_agent(&sl->bufOff, u32x4{(uint32_t)boff, (uint32_t)(boff >> 32), blen, 1u});
                st16_agent(sl, u32x4{(uint32_t)kReady, d, (uint32_t)ev, (uint32_t)(ev >> 32)});
                atomicAdd(occ_in_progress(R, h), 1ull);
                atomicAdd(occ_table_used(R, h), 1ull);
                res.slot = h;
                res.bytes = blen;
                res.bufOff = boff;
                active = false;
            } else if (old == kBusy || old == kReady) {
                u32x4 A, B;
                ld_slot_ab(sl, A, B);
                if (A.x == kReady && B.w != 0u) {
                    if (A.y == d && (((uint64_t)A.w << 32) | A.z) == ev) {
                        res.slot = h;
                        res.bytes = B.z;
                        res.bufOff = ((uint64_t)B.y << 32) | B.x;
                        active = false;
                    } else {
                        advance = true;                                // another event's slot
                    }
                } else if (A.x == kDone || A.x == kLost) {
                    advance = true;                                    // DONE / LOST meanwhile
                } else {
                    waiting = true;                // not published yet, or a read that overtook the claim
                    claimed = true;
                }
            } else {
                advance = true;                                        // DONE / LOST
            }
            if (advance) {
                claimed = false;
                h = (h + 1u) & mask;
                if (++probes >= R.tableSlots) {
                    atomicOr(&R.ctl->errorFlags, 1u);
                    active = false;
                }
            }
            if (waiting && ++spins > kSpinLimit) {
                atomicOr(&R.ctl->errorFlags, 4u);
                active = false;
            }
        }
        if (__ballot(waiting)) __builtin_amdgcn_s_sleep(kPollSleep);
#if E2SAR_TRACE
        pass++;
#endif
    }
#if E2SAR_TRACE
    if (__ballot(want)) {
        TRACE_FIRST(2, 2, trace_now());
        TRACE_FIRST(2, 3, pass);
    }
#endif
    return res;
}

// Completion (cpp:403-427): erase from the table, count, and hand the event to the
// completed queue (or record it lost when the queue is full or it had no buffer).
// keepSlot (reference-order mode): the walk that found the completion already left the
// slot in its final state (a later fragment of the key may have started a new item).
__device__ void complete_event(const ReasDev &R, uint32_t slot, uint64_t ev, uint64_t boff, uint32_t bytes,
                               uint32_t d, uint32_t frags, bool keepSlot = false)
{
    ReasSlot *sl = R.slots + slot;
    if (!keepSlot) st_agent(&sl->state, (uint32_t)kDone);      // erase from the map (cpp:409)
    atomicAdd(&R.shards[slot % kShards].eventSuccess, 1ull);   // cpp:426
    atomicAdd(occ_in_progress(R, slot), ~0ull);
    bool lostOnEnqueue = (boff == kNoBuf);
    if (!lostOnEnqueue) {
        const uint32_t idx = atomicAdd(&R.ctl->nCompleted, 1u);
        if (idx < R.queueCapacity) {
            e2sar_hip_event_rec rec;
            rec.eventNum = ev;
            rec.arenaOffset = boff;
            rec.bytes = bytes;
            rec.dataId = (uint16_t)d;
            rec.flags = 0;
            rec.numFragments = frags;
            rec.reserved = 0;
            R.completed[idx] = rec;
        } else {
            lostOnEnqueue = true;                              // queue full (hpp:140-145)
        }
    }
    if (lostOnEnqueue) {
        atomicAdd(&R.ctl->enqueueLoss, 1ull);
        const uint32_t li = atomicAdd(&R.ctl->nLost, 1u);
        if (li < R.lostCapacity) {
            e2sar_hip_lost_rec lr;
            lr.eventNum = ev;
            lr.numFragments = frags;
            lr.dataId = (uint16_t)d;
            lr.enqueueLoss = 1;
            lr.reserved = 0;
            R.lost[li] = lr;
        }
    }
}

__device__ void recycle_slots(const ReasDev &R, uint32_t s, int dropCompleted)
{
    if (s < R.tableSlots) {
        ReasSlot z{};
        R.slots[s] = z;
    }
    if (s == 0) {
        R.ctl->arenaTop = 0;
        R.ctl->tableUsed = 0;
        R.ctl->inProgress = 0;
        if (dropCompleted) R.ctl->nCompleted = 0;
    }
    if (s < kShards) {
        *occ_in_progress(R, s) = 0ull;
        *occ_table_used(R, s) = 0ull;
    }
}

}  // namespace e2sar_amd
