// reas_order.hpp -- reassembly in the reference's arrival order (the ro_* kernels).
#pragma once

#include "dev_access.hpp"
#include "reas_classify.hpp"
#include "reas_split.hpp"
#include "wire.hpp"

namespace e2sar_amd {

// ---------------------------------------------------------------------------------
// reassembly in the reference's arrival order (E2SAR_HIP_REAS_REFERENCE_ORDER)
//
// The reference's receive body takes datagrams one at a time (e2sarDPReassembler.cpp:
// 335-427), and for some inputs the order decides the outcome: a fragment with
// bufferOffset 0 always starts a new item, replacing (dropping) an item in progress under
// the same key (cpp:361-369); a fragment whose key has no item starts one (cpp:376-384),
// also after its event completed; completion is tested after every fragment (cpp:403), so
// a duplicate that arrives before the last fragment makes curBytes overshoot while one that
// arrives after completion starts an item of its own.  This mode reproduces that for any
// arrival order (batch order, then datagram order within a batch):
//   ro_key_kernel  : parse and validate every datagram (counters as classify_wave), register
//                    its key in the table (find_or_create<keyOnly>), write a 16-byte record
//                    {off, plen, blen, hl}, and file every run of consecutive positions of
//                    one key (per wave) in the key's bucket of kRoBucket runs (past that in
//                    an overflow list); a key's first run lists the key;
//   ro_place_kernel: one workgroup: hands the number of listed keys to the walk and resets
//                    the counters; only if a key overflowed its bucket, places and sorts by
//                    position the runs of every such key;
//   ro_walk_kernel : one wave per key orders its runs by position (rank and push, <= 64 runs) and
//                    walks that key's datagrams in arrival order with the reference's rules,
//                    creating items (arena buffers) as it goes, and writes the PktInfo /
//                    FinishRec work records of the split form;
//   reas_scatter_kernel then moves the bytes and publishes the completions.

// key of a datagram that does not take part (bad header, bounds, table full): no real slot,
// so it joins no run
constexpr uint32_t kRoNoSlot = 0xFFFFFFFFu;
// Key-pass workgroup: 1024 threads (round 6, profiles/round6/ro_keypass/): events
// interleaved datagram by datagram put the same keys in every workgroup of their span, and
// each workgroup registers a key and files its runs with one lookup and one returning atomic
// on that key's slot -- 1024-datagram workgroups make 4x fewer of those than 256: K = 64 /
// 205 interleaved events 190 / 425 -> 135-137 / 232-235 us per batch, K = 1 / 8 91.7-94.0 /
// 117-118 -> 91.2-91.8 / 113-114 (512 threads: 144-146 / 290-292; 1024 threads with two
// datagrams per lane, one workgroup per CU: 148-149 / 237 -- too few workgroups).
constexpr int kRoKeyBlock = 1024;

// The key pass's view of one datagram's header: parse_hdr, less what takes no part.
// (Returned by value: with `foreign` handed back through a reference the kernel grew by 18
// instructions.)
struct RoHdr {
    ParsedHdr h;
    bool foreign;
};
__device__ __forceinline__ RoHdr ro_parse_hdr(const ReasDev &R, const RawHdr &raw, uint32_t hl, uint32_t stride, bool live)
{
    ParsedHdr h = parse_hdr(raw, hl, stride, live);
    const bool foreign = h.ok && foreign_event(R, h.ev);      // another rank's event: takes no part
    if (foreign) h = ParsedHdr{0, 0, 0, 0, 0, false, false, false};
    // bounds against the fragment's own bufferLength, before the lookup (the reference
    // memcpy's unchecked at cpp:391; dropped and counted here)
    if (h.ok && (uint64_t)h.off + h.pl > h.blen) {
        h.ok = false;
        h.derr = true;
    }
    return RoHdr{h, foreign};
}

// Each head claims or finds its key's entry in the workgroup's table of NK entries (tags
// cleared by the caller) and returns it; called by every thread of the workgroup.
template <uint32_t NK>
__device__ __forceinline__ uint32_t ro_wg_key(bool head, uint64_t ev, uint32_t d, unsigned long long *wgEv,
                                              uint32_t *wgD, uint32_t *wgTag)
{
    uint32_t e = slot_hash(ev, d, NK - 1u);
    bool pending = head, check = false;
    __syncthreads();                                           // table cleared
    while (__syncthreads_or(pending)) {
        if (pending) {
            if (atomicCAS(&wgTag[e], 0u, 1u) == 0u) {
                wgEv[e] = ev;
                wgD[e] = d;
                pending = false;
            } else {
                check = true;
            }
        }
        __syncthreads();                                       // claimed keys are written
        if (check) {
            check = false;
            if (wgEv[e] == ev && wgD[e] == d) pending = false;
            else e = (e + 1u) & (NK - 1u);
        }
    }
    return e;
}

// Runs of consecutive positions of one key (one slot) within the wave -- they start at the
// heads -- filed in the slot's bucket (the run of index 0 lists the slot for the walk), past
// kRoBucket runs at their head's position in the overflow list.  k: the run's index in its key.
__device__ __forceinline__ void ro_file_runs(const RoScratch &sc, bool ok, uint32_t slot, uint32_t k, uint32_t p,
                                             uint32_t lane, uint32_t wave, bool waveLive)
{
    const uint32_t ks = ok ? slot : kRoNoSlot;
    const uint32_t pks = lane_prev(ks, kRoNoSlot), nks = lane_next(ks, kRoNoSlot);
    const bool rhead = ok && (lane == 0 || pks != ks);
    const bool rtail = ok && (lane == 63 || nks != ks);
    const uint64_t RT = __ballot(rtail);
    if (rhead) {
        const uint64_t below = (1ull << lane) - 1ull;
        const uint32_t len = (uint32_t)__builtin_ctzll(RT & ~below) - lane + 1u;   // to this run's last lane
        if (k == 0u) sc.active[atomicAdd(&sc.ctr[1], 1u)] = slot;
        if (k < kRoBucket) {
            sc.bucket[(size_t)slot * kRoBucket + k] = ((unsigned long long)p << 32) | len;
        } else {
            st16(reinterpret_cast<uint8_t *>(sc.runs + p), u32x4{slot, p, len, k});   // at its head's position
        }
    }
    // which lanes of this wave hold an overflow run (every wave writes its word; a flag tells
    // the place pass to look -- a plain store, not a counter all waves would contend on)
    const uint64_t OV = __ballot(rhead && k >= kRoBucket);
    if (lane == 0 && waveLive) {
        sc.ovMask[wave] = OV;
        if (OV) sc.ctr[0] = 1u;
    }
}

template <int TB>
__global__ __launch_bounds__(TB) void ro_key_kernel(ReasDev R, const uint8_t *__restrict__ pkts, uint32_t stride,
                                                    const uint32_t *__restrict__ lens, uint32_t n, uint64_t now,
                                                    RoScratch sc, PktInfo *__restrict__ info)
{
    // the workgroup's distinct keys (at most TB): one global lookup and one run-count
    // atomic per key per workgroup, not per wave
    constexpr uint32_t kWgKeys = 2u * TB;       // the per-workgroup key table
    __shared__ unsigned long long wgEv[kWgKeys];
    __shared__ uint32_t wgD[kWgKeys], wgTag[kWgKeys], wgCnt[kWgKeys], wgSlot[kWgKeys], wgBase[kWgKeys];
    const uint32_t wave = blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t p0 = wave * 64u;
    const bool waveLive = p0 < n;                              // (a wave past n still meets the barriers)
    const uint32_t gn = !waveLive ? 0u : (n - p0 < 64u) ? n - p0 : 64u;
    const bool live = lane < gn;
    const uint32_t p = waveLive ? p0 + (live ? lane : 0u) : 0u;
    for (uint32_t i = threadIdx.x; i < kWgKeys; i += TB) {
        wgTag[i] = 0u;
        wgCnt[i] = 0u;
    }
    const RawHdr raw = load_hdr(R.withLB != 0, pkts, stride, lens, p);
    const uint32_t hl = R.withLB ? kLBREHdrLen : kREHdrLen;
    const RoHdr rh = ro_parse_hdr(R, raw, hl, stride, live);
    ParsedHdr h = rh.h;
    const bool foreign = rh.foreign;
    // runs of equal keys: only the run head takes part.  Every head registers its key in the
    // workgroup's table itself and takes its run index there with one LDS atomic (round 6:
    // a per-wave loop that first collapsed the heads of one key took 64 passes in a wave of
    // 64 interleaved events; K = 64 / 205 136.5 / 233 -> 126.5 / 225 us per batch, in
    // order unchanged, profiles/round6/ro_keypass/)
    const uint64_t pev = ((uint64_t)lane_prev((uint32_t)(h.ev >> 32), 0u) << 32) | lane_prev((uint32_t)h.ev, 0u);
    const uint32_t pd = lane_prev(h.d, 0u), pok = lane_prev(h.ok ? 1u : 0u, 0u);
    const bool head = h.ok && (lane == 0 || !pok || pev != h.ev || pd != h.d);
    const uint32_t e = ro_wg_key<kWgKeys>(head, h.ev, h.d, wgEv, wgD, wgTag);
    // this head's run: its index among the workgroup's runs of the key
    uint32_t o = 0;
    if (head) o = atomicAdd(&wgCnt[e], 1u);
    __syncthreads();
    for (uint32_t b = 0; b < kWgKeys; b += TB) {               // one lookup + one atomic per key
        const uint32_t i = b + threadIdx.x;
        const bool want = wgTag[i] != 0u;
        const LookupResult lr = find_or_create<true>(R, want, wgEv[i], wgD[i], 0u, now);
        if (want) {
            wgSlot[i] = lr.slot;
            wgBase[i] = lr.slot != kNoSlot ? atomicAdd(&sc.runCnt[lr.slot], wgCnt[i]) : 0u;
        }
    }
    __syncthreads();
    const uint32_t hslot = head ? wgSlot[e] : kNoSlot;
    const uint32_t k = head ? wgBase[e] + o : 0u;            // this run's index in its key
    const uint32_t slot = __shfl(hslot, run_head_lane(__ballot(head), lane));
    if (h.ok && slot == kNoSlot) {                             // table full / probe timeout
        h.ok = false;
        h.derr = true;
    }
    if (live) {
        const u32x4 v = {h.off, h.pl, h.blen, hl};
        st16(reinterpret_cast<uint8_t *>(sc.recs + p), v);
        if (!h.ok) st_info(info + p, PktInfo{0ull, 0u, hl});   // takes no part
    }
    ro_file_runs(sc, h.ok, slot, k, p, lane, wave, waveLive);
    wave_stats(R, live && !foreign, (live && !foreign) ? raw.len : 0u, h.bad, h.derr, wave);
}

// Between the key pass and the walk: hands the count of listed keys to the walk (ctr[1] ->
// ctr[2]) and resets it for the next batch (ctr[0] is reset by the walk: every workgroup
// here reads it).  Only when some key filed more than kRoBucket runs (ctr[0] set: events
// interleaved in arrival, or very large ones) does it do more: an exclusive scan of the run
// counts of those keys gives each its place (runBase), and every overflow run (found by the
// key-pass waves' overflow masks, stored at its head's position) is copied to runBase + its
// index in the key (k, from the key pass's count) -- no atomics, no order: the key's walk
// wave orders them.  Every workgroup computes the scan itself, into LDS (no grid
// synchronisation), and places a share of the runs; a table above kPlaceLdsSlots slots is
// handled by workgroup 0 alone through the global runBase.
constexpr uint32_t kPlaceThreads = 256, kPlaceBlocks = 64, kPlaceLdsSlots = 16384;
__global__ __launch_bounds__(kPlaceThreads) void ro_place_kernel(RoScratch sc, uint32_t T, uint32_t n)
{
    __shared__ uint32_t base[kPlaceLdsSlots];
    __shared__ uint32_t part[kPlaceThreads / 64];
    const uint32_t t = threadIdx.x;
    const uint32_t nOver = sc.ctr[0];
    if (blockIdx.x == 0 && t == 0) {
        sc.ctr[2] = sc.ctr[1];
        sc.ctr[1] = 0u;
    }
    if (nOver == 0u) return;                                          // uniform: the usual case
    const bool inLds = T <= kPlaceLdsSlots;
    if (!inLds && blockIdx.x != 0) return;
    const uint32_t per = (T + kPlaceThreads - 1u) / kPlaceThreads;
    const uint32_t s0 = t * per < T ? t * per : T, s1 = s0 + per < T ? s0 + per : T;
    uint32_t sum = 0;
    for (uint32_t q = s0; q < s1; q++) {
        const uint32_t c = sc.runCnt[q];
        sum += c > kRoBucket ? c : 0u;
    }
    uint32_t all;
    uint32_t b = block_excl_scan<uint32_t, kPlaceThreads / 64>(sum, part, all);
    for (uint32_t q = s0; q < s1; q++) {
        const uint32_t c = sc.runCnt[q];
        if (inLds) base[q] = b;
        if (blockIdx.x == 0) sc.runBase[q] = b;
        b += c > kRoBucket ? c : 0u;
    }
    __syncthreads();                        // (global runBase: written and read by this workgroup)
    // one thread per datagram position: an overflow run sits at its head's position, marked
    // in its key-pass wave's mask
    const uint32_t nThreads = inLds ? gridDim.x * kPlaceThreads : kPlaceThreads;
    for (uint32_t p = (inLds ? blockIdx.x * kPlaceThreads : 0u) + t; p < n; p += nThreads) {
        if ((sc.ovMask[p >> 6] >> (p & 63u)) & 1ull) {
            const u32x4 run = ld16(reinterpret_cast<const uint8_t *>(sc.runs + p));   // slot, start, len, k
            const uint32_t rb = inLds ? base[run.x] : sc.runBase[run.x];
            sc.placed[rb + run.w] = ((unsigned long long)run.y << 32) | run.z;
        }
    }
}

// One wave per key walks the key's datagrams in arrival order, 64 at a time, with the
// reference's rules (cpp:361-427).  The key's runs are taken 64 at a time in position order --
// a slot of at most kRoBucket runs orders its bucket here (rank by start, one lane push), a
// larger one was placed and sorted by ro_place_kernel -- and a datagram index of
// the concatenated runs maps to its position by a binary search over the runs' prefix sums.  The item state (buffer, length, curBytes, fragments) is
// wave-uniform.  Within a chunk the walk goes segment by segment: a segment starts where a
// new item starts (offset 0, or no item in progress) and runs to the next offset-0 fragment;
// a masked prefix sum of the payload lengths finds the first fragment whose add makes
// curBytes equal the item's length (completion, cpp:403), which ends the segment early.
// Fragments that overrun the item (made by a fragment with another bufferLength) count as
// data errors and add nothing.  One segment per chunk is the usual case; duplicates, late
// offset-0 fragments and replays after completion add segments.
constexpr uint32_t kRoAhead = 4;
constexpr uint32_t kRoSortLds = 2048;       // runs of one key sorted in LDS by its wave (16 KiB)
// The walk runs one wave per workgroup with 32 KiB of LDS (round 6, profiles/round6/ro_walk/):
// four key waves per workgroup sharing a CU, 16 KiB each, left three quarters of the CUs
// idle and sent keys whose span outgrew a 16 KiB position bitmap to the run sort -- 205
// events interleaved 224 -> 151 us per batch, in order and K = 8 / 64 about 1 us faster.
constexpr uint32_t kRoWalkLds = 4096;       // 8-byte words of LDS per walk wave

// Bitonic sort of P = 128 NP keys in LDS by one wave: per stage each lane loads its NP
// pairs at once (one LDS round trip per stage, not one per pair), then compares and stores.
template <int NP>
__device__ __forceinline__ void wave_sort_lds(unsigned long long *v, uint32_t lane)
{
    constexpr uint32_t P = 128u * NP;
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            unsigned long long x[NP], y[NP];
            uint32_t ii[NP];
#pragma unroll
            for (uint32_t t = 0; t < (uint32_t)NP; t++) {
                const uint32_t q = lane + 64u * t;                   // pair q: elements i, i + j
                ii[t] = ((q & ~(j - 1u)) << 1) | (q & (j - 1u));
                x[t] = v[ii[t]];
                y[t] = v[ii[t] + j];
            }
#pragma unroll
            for (uint32_t t = 0; t < (uint32_t)NP; t++) {
                const bool up = (ii[t] & k) == 0u;
                if (up ? x[t] > y[t] : x[t] < y[t]) {
                    v[ii[t]] = y[t];
                    v[ii[t] + j] = x[t];
                }
            }
            wave_lds_sync();
        }
}

// Runs of a key of more than kRoBucket runs, in position order, for its walk wave: the
// bucket (bv, one run per lane) and the placed overflow runs (index >= kRoBucket), padded to
// a power of two and sorted by start -- up to kRoSortLds runs by a bitonic wave sort in the
// wave's LDS region, else in its region of sortTmp (at twice the
// key's place, so regions of different keys never meet) through agent-scope loads and
// stores, which every lane of the wave sees after the stage's vmcnt(0).  Returns where the
// sorted runs are.
__device__ unsigned long long *ro_sort_runs(const RoScratch &sc, uint32_t slot, uint32_t c, unsigned long long bv,
                                            unsigned long long *lds, uint32_t lane)
{
    const uint32_t rb = sc.runBase[slot];
    const unsigned long long *ov = sc.placed + rb;
    uint32_t P = 64;
    while (P < c) P <<= 1;
    if (P <= kRoSortLds) {
        for (uint32_t i = lane; i < P; i += 64u) lds[i] = i < kRoBucket ? bv : (i < c ? ov[i] : ~0ull);
        wave_lds_sync();
        if (P <= 128u) wave_sort_lds<1>(lds, lane);
        else if (P <= 256u) wave_sort_lds<2>(lds, lane);
        else if (P <= 512u) wave_sort_lds<4>(lds, lane);
        else if (P <= 1024u) wave_sort_lds<8>(lds, lane);
        else wave_sort_lds<16>(lds, lane);
        return lds;
    }
    unsigned long long *g = sc.sortTmp + 2ull * rb;
    for (uint32_t i = lane; i < P; i += 64u)
        __hip_atomic_store(g + i, i < kRoBucket ? bv : (i < c ? ov[i] : ~0ull), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (uint32_t k = 2; k <= P; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = lane; i < P; i += 64u) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const unsigned long long x = __hip_atomic_load(g + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned long long y = __hip_atomic_load(g + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (((i & k) == 0u) ? x > y : x < y) {
                        __hip_atomic_store(g + i, y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(g + l, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    return g;
}

// The positions of a key of more than kRoBucket runs, in arrival order, into the wave's LDS
// region, without sorting its runs: every run sets its positions' bits in a bitmap over the
// key's span (LDS atomic ORs), and the set bits read in order are the positions.  Returns
// how many (0 when bitmap and list do not fit the region: then the runs are sorted).
__device__ uint32_t ro_positions(const RoScratch &sc, uint32_t slot, uint32_t c, unsigned long long bv,
                                 unsigned long long *lds, uint32_t lane, uint32_t ldsWords)
{
    const unsigned long long *ov = sc.placed + sc.runBase[slot];
    uint32_t mn = 0xFFFFFFFFu, mx = 0, tl = 0;
    for (uint32_t i = lane; i < c; i += 64u) {
        const unsigned long long r = i < kRoBucket ? bv : ov[i];
        const uint32_t st = (uint32_t)(r >> 32), ln = (uint32_t)r;
        mn = min(mn, st);
        mx = max(mx, st + ln);
        tl += ln;
    }
    mn = wave_min_u32(mn);
    mx = wave_max_u32(mx);
    tl = readlane(wave_incl_scan(tl), 63);
    const uint32_t words = (mx - mn + 63u) / 64u;
    if ((size_t)words * 8u + (size_t)tl * 4u > (size_t)ldsWords * 8u) return 0u;     // wave-uniform
    for (uint32_t i = lane; i < words; i += 64u) lds[i] = 0ull;
    wave_lds_sync();
    for (uint32_t i = lane; i < c; i += 64u) {
        const unsigned long long r = i < kRoBucket ? bv : ov[i];
        const uint32_t b = (uint32_t)(r >> 32) - mn, ln = (uint32_t)r;   // 1..64 positions
        const unsigned long long m = ln >= 64u ? ~0ull : ((1ull << ln) - 1ull);
        const uint32_t o = b & 63u;
        atomicOr(&lds[b >> 6], m << o);
        if (o + ln > 64u) atomicOr(&lds[(b >> 6) + 1u], m >> (64u - o));
    }
    wave_lds_sync();
    // each lane reads a contiguous block of words; a wave scan of their counts places them
    const uint32_t wpl = (words + 63u) / 64u, w0 = lane * wpl, w1 = min(w0 + wpl, words);
    uint32_t cnt = 0;
    for (uint32_t x = w0; x < w1; x++) cnt += (uint32_t)__builtin_popcountll(lds[x]);
    uint32_t at = wave_incl_scan(cnt) - cnt;
    uint32_t *pos = reinterpret_cast<uint32_t *>(lds + words);
    for (uint32_t x = w0; x < w1; x++)
        for (unsigned long long m = lds[x]; m; m &= m - 1ull) pos[at++] = mn + x * 64u + (uint32_t)__builtin_ctzll(m);
    wave_lds_sync();
    // the list starts at lds + words: move it to the front (the walk reads it from there)
    uint32_t *dst = reinterpret_cast<uint32_t *>(lds);
    for (uint32_t i = lane; i < tl; i += 64u) {
        const uint32_t v = pos[i];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        dst[i] = v;
    }
    wave_lds_sync();
    return tl;
}

// The item in progress under a key (the device form of the reference's EventQueueItem) and
// the walk's tallies; wave-uniform.
struct RoItem {
    bool item;                    // an item is in progress
    uint64_t boff, cur, created;  // its buffer (arena offset, or kNoBuf), curBytes, firstSegment
    uint32_t ibytes, frags;       // its length (the bufferLength of the fragment that started it), fragments
    long long live;               // net change of items in progress
    uint32_t derr;                // fragments that overran their item
};
__device__ __forceinline__ RoItem ro_item_load(const ReasSlot *sl)
{
    RoItem it;
    it.item = sl->bvalid == 1u;                                // an item in progress from an earlier batch
    it.boff = sl->bufOff;
    it.ibytes = sl->bytes;
    it.cur = it.item ? (sl->acc & kAccBytesMask) : 0ull;
    it.frags = it.item ? (uint32_t)(sl->acc >> kAccFragShift) : 0u;
    it.created = sl->created;
    it.live = 0;
    it.derr = 0;
    return it;
}
__device__ __forceinline__ void ro_item_store(ReasSlot *sl, const RoItem &it)
{
    if (it.item) {
        sl->bufOff = it.boff;
        sl->bytes = it.ibytes;
        sl->bvalid = 1u;
        sl->acc = ((unsigned long long)it.frags << kAccFragShift) | (it.cur & kAccBytesMask);
        sl->created = it.created;
    } else {
        sl->state = kDone;                                     // no item left under this key
    }
}

// The key a wave walks, and where its work records go.
struct RoKey {
    uint64_t ev, now;
    uint32_t slot, d;
    PktInfo *info;
    FinishRec *fin;
};

// The buffer of a new item of blen bytes: lane 0 claims it from the arena, every lane gets
// it (kNoBuf, with the error flag set, when the arena is full).
__device__ __forceinline__ uint64_t ro_new_buffer(const ReasDev &R, uint32_t blen, uint32_t lane)
{
    const uint64_t need = ((uint64_t)blen + 255ull) & ~255ull;
    uint64_t nb = 0;
    if (lane == 0) nb = atomicAdd(&R.ctl->arenaTop, (unsigned long long)(need ? need : 256ull));
    nb = readlane_u64(nb, 0);
    if (nb + blen > R.arenaBytes) {
        if (lane == 0) atomicOr(&R.ctl->errorFlags, 2u);
        nb = kNoBuf;
    }
    return nb;
}

// One chunk of 64 datagrams of the key, in arrival order: datagrams [base, base + 64) of the
// tot being walked, lane by lane (q: position, rc: record).
__device__ __forceinline__ void ro_walk_chunk(const ReasDev &R, const RoKey &key, RoItem &it, uint32_t tot, uint32_t base,
                                              uint32_t q, const RoRec &rc, uint32_t lane)
{
    const bool valid = base + lane < tot;
    const uint32_t nv = (tot - base < 64u) ? tot - base : 64u;
    for (uint32_t t = 0; t < nv;) {
        if (!it.item || readlane(rc.off, t) == 0u) {
            // a new item (EventQueueItem(rehdr), hpp:89-98); at offset 0 it replaces the
            // one in progress (cpp:361-369), dropped without a lost record
            if (it.item) it.live--;
            const uint32_t blen = readlane(rc.blen, t);
            it.boff = ro_new_buffer(R, blen, lane);
            it.ibytes = blen;
            it.cur = 0;
            it.frags = 0;
            it.created = key.now;
            it.item = true;
            it.live++;
        }
        const uint64_t zm = __ballot(valid && rc.off == 0u && lane > t);
        const uint32_t v = zm ? (uint32_t)__builtin_ctzll(zm) : nv;      // next item start
        const bool inseg = lane >= t && lane < v;
        const bool viol = inseg && (uint64_t)rc.off + rc.plen > it.ibytes;
        const uint32_t P = wave_incl_scan((inseg && !viol) ? rc.plen : 0u);
        const uint64_t cm = __ballot(inseg && !viol && it.cur + P == (uint64_t)it.ibytes);
        const uint32_t end = cm ? (uint32_t)__builtin_ctzll(cm) + 1u : v;
        const bool inr = lane >= t && lane < end;
        it.frags += (uint32_t)__builtin_popcountll(__ballot(inr && !viol));     // cpp:398-400
        it.derr += (uint32_t)__builtin_popcountll(__ballot(inr && viol));
        it.cur += readlane(P, end - 1u);
        const bool comp = cm && lane == end - 1u;
        if (inr) {
            PktInfo pi{0ull, 0u, rc.hl};
            if (!viol && it.boff != kNoBuf) {
                pi.dst = (uint64_t)(R.arena + it.boff + rc.off);
                pi.plen = rc.plen;
            }
            if (comp) {                                        // cpp:403: complete, erase, enqueue
                FinishRec f;
                f.ev = key.ev;
                f.boff = it.boff;
                f.slot = key.slot | kFinKeepSlot;
                f.bytes = it.ibytes;
                f.frags = it.frags;
                f.d = key.d;
                key.fin[q] = f;
            }
            st_info(key.info + q, pi, comp ? kPktCompletes : 0u);
        }
        if (cm) it.item = false;                               // inProgress-- in complete_event
        t = end;
    }
}

// The walk of tot datagrams of the key, 64 at a time; q_of(base) is the position of datagram
// base + lane.  The records of the next kRoAhead - 1 chunks are in flight while a chunk is
// walked (the walk is a chain of dependent chunks over few waves: latency, not bandwidth,
// bounds it).  The ring is indexed statically (unrolled by kRoAhead); a chunk's slot is
// reloaded after the chunk is walked.  (Round 5: staging a key's records in LDS by LDS-DMA,
// 16 chunks per wait, measured 16.6 against this ring's 15.5 us per launch: the chunks' own
// work, ~0.8 us each at one wave per CU, not their loads, bounds the walk)
template <typename PosOf>
__device__ __forceinline__ void ro_walk_ring(const ReasDev &R, const RoKey &key, RoItem &it,
                                             const RoRec *__restrict__ recs, uint32_t tot, uint32_t lane, PosOf q_of)
{
    uint32_t qr[kRoAhead];
    RoRec rr[kRoAhead];
#pragma unroll
    for (uint32_t i = 0; i < kRoAhead; i++) {
        qr[i] = q_of(i * 64u);
        rr[i] = RoRec{0u, 0u, 0u, 0u};
        if (i * 64u + lane < tot) rr[i] = recs[qr[i]];
    }
    for (uint32_t b0 = 0; b0 < tot; b0 += kRoAhead * 64u) {
#pragma unroll
        for (uint32_t i = 0; i < kRoAhead; i++) {
            const uint32_t base = b0 + i * 64u;
            if (base < tot) {                                  // wave-uniform
                ro_walk_chunk(R, key, it, tot, base, qr[i], rr[i], lane);
                const uint32_t nxt = base + kRoAhead * 64u;
                if (nxt < tot) {
                    qr[i] = q_of(nxt);
                    if (nxt + lane < tot) rr[i] = recs[qr[i]];
                }
            }
        }
    }
}

// Position source of the ring over m <= 64 runs in position order, one per lane (rex: the
// exclusive prefix of their lengths, rstart: their starts).  Datagram base + lane lies in the
// last run whose prefix is <= it.  The runs that meet the chunk [base, base + 64) are ra..rb
// (usually two): a uniform loop over them with scalar reads, no per-lane search
struct RoRunPos {
    uint32_t m, rex, rstart, lane;
    __device__ __forceinline__ uint32_t operator()(uint32_t base) const
    {
        const uint32_t g = base + lane;
        const uint64_t b0 = __ballot(lane < m && rex <= base), b1 = __ballot(lane < m && rex < base + 64u);
        const int ra = b0 ? 63 - __builtin_clzll(b0) : 0, rb = b1 ? 63 - __builtin_clzll(b1) : 0;
        uint32_t qb = 0;
        for (int r = ra; r <= rb; r++) {
            const uint32_t sr = readlane(rex, (uint32_t)r);
            const uint32_t st = readlane(rstart, (uint32_t)r);
            if (g >= sr) qb = st - sr;
        }
        return qb + g;
    }
};

// Order the m runs of a bucket (start << 32 | length, one per lane) by start (the starts are
// distinct): each run's rank is the number of runs that start before it (m scalar reads),
// then one push per word to lane rank
__device__ __forceinline__ unsigned long long ro_order_bucket(unsigned long long rv, uint32_t m, uint32_t lane)
{
    const uint32_t mys = (uint32_t)(rv >> 32);
    uint32_t rank = 0;
    for (uint32_t r = 0; r < m; r++) rank += readlane(mys, r) < mys ? 1u : 0u;
    if (lane >= m) rank = lane;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_permute((int)(rank * 4u), (int)(uint32_t)rv);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_permute((int)(rank * 4u), (int)mys);
    return ((unsigned long long)hi << 32) | lo;
}

// WB waves per workgroup, LW 8-byte words of LDS per wave (the position bitmap and list, or
// the LDS sort of <= kRoSortLds runs)
template <int WB, uint32_t LW>
__global__ __launch_bounds__(WB * 64) void ro_walk_kernel(ReasDev R, RoScratch sc, uint32_t T, uint64_t now,
                                                          PktInfo *__restrict__ info, FinishRec *__restrict__ fin)
{
    static_assert(LW >= kRoSortLds, "the LDS sort needs kRoSortLds words");
    __shared__ unsigned long long roSort[WB][LW];
    const uint32_t w = blockIdx.x * (uint32_t)WB + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    // the chain of dependent loads before the walk proper is kept short: the key is read
    // beside the count of keys, and its bucket beside its run count
    const uint32_t nKeys = sc.ctr[2];
    const uint32_t slot = w < T ? sc.active[w] : 0u;
    if (w >= nKeys) return;                                    // wave-uniform
    const uint32_t nRuns = sc.runCnt[slot];
    const unsigned long long bv = sc.bucket[(size_t)slot * kRoBucket + lane];
    const bool inBucket = nRuns <= kRoBucket;
    if (w == 0 && lane == 0) sc.ctr[0] = 0u;                   // overflow runs: next batch
    unsigned long long *lds = roSort[threadIdx.x >> 6];
    const unsigned long long *runsOf = nullptr;
    uint32_t nPos = 0;                                         // > 0: the key's positions are in lds
    if (!inBucket) {
        nPos = ro_positions(sc, slot, nRuns, bv, lds, lane, LW);
        if (nPos == 0u) runsOf = ro_sort_runs(sc, slot, nRuns, bv, lds, lane);
    }
    const RoRec *__restrict__ recs = sc.recs;
    ReasSlot *sl = R.slots + slot;
    const RoKey key{sl->eventNum, now, slot, sl->dataId, info, fin};
    RoItem it = ro_item_load(sl);
    if (nPos) {
        // the key's positions in arrival order, from its position bitmap
        const uint32_t *pos = reinterpret_cast<const uint32_t *>(lds);
        ro_walk_ring(R, key, it, recs, nPos, lane, [=](uint32_t base) { return base + lane < nPos ? pos[base + lane] : 0u; });
    } else {
        for (uint32_t r0 = 0; r0 < nRuns; r0 += 64u) {
            // this batch of the key's runs, in position order: start << 32 | length per lane
            const uint32_t m = (nRuns - r0 < 64u) ? nRuns - r0 : 64u;
            unsigned long long rv = (lane < m) ? (inBucket ? bv : runsOf[r0 + lane]) : ~0ull;
            if (inBucket) rv = ro_order_bucket(rv, m, lane);
            const uint32_t rlen = (uint32_t)rv & 0xFFFFFFFFu, rstart = (uint32_t)(rv >> 32);
            const uint32_t rl = lane < m ? rlen : 0u;
            const uint32_t rin = wave_incl_scan(rl), rex = rin - rl;
            ro_walk_ring(R, key, it, recs, readlane(rin, 63), lane, RoRunPos{m, rex, rstart, lane});
        }
    }
    if (lane == 0) {
        sc.runCnt[slot] = 0u;                                  // next batch
        ro_item_store(sl, it);
        if (it.live) atomicAdd(occ_in_progress(R, slot), (unsigned long long)it.live);
        if (it.derr) atomicAdd(&R.shards[slot % kShards].dataErrCnt, (unsigned long long)it.derr);
    }
}

}  // namespace e2sar_amd
