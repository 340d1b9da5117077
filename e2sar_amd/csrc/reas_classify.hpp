// reas_classify.hpp -- classification of one wave of datagrams: header parse, event table lookup, run sums.
#pragma once

#include "dev_access.hpp"
#include "reas_table.hpp"
#include "wire.hpp"

namespace e2sar_amd {

// Raw header words of one datagram, loaded before the payload loads of the block so the
// classification chain overlaps them.
struct RawHdr {
    uint32_t len;
    u32x4 re;        // RE header dwords 0..3
    uint32_t re4;    // RE header dword 4 (eventNum low word)
};

// withLB: an LB header stands in front of the RE header
template <bool HO = false>
__device__ __forceinline__ RawHdr load_hdr(bool withLB, const uint8_t *__restrict__ pkts, uint32_t stride,
                                           const uint32_t *__restrict__ lens, uint32_t p)
{
    const uint8_t *re = pkts + (uint64_t)p * stride + (withLB ? kLBHdrLen : 0u);   // 16-byte aligned
    RawHdr h;
    if (HO) {       // bytes handed off inside the launch (chained form): sc1 loads
        h.len = ld4_sc1(lens + p);
        h.re.x = ld4_sc1(reinterpret_cast<const uint32_t *>(re));
        h.re.y = ld4_sc1(reinterpret_cast<const uint32_t *>(re + 4));
        h.re.z = ld4_sc1(reinterpret_cast<const uint32_t *>(re + 8));
        h.re.w = ld4_sc1(reinterpret_cast<const uint32_t *>(re + 12));
        h.re4 = ld4_sc1(reinterpret_cast<const uint32_t *>(re + 16));
        return h;
    }
    h.len = lens[p];
    h.re = ld16(re);
    h.re4 = ld4(re + 16);
    return h;
}

// True for an event another rank owns (ReasDev.ownWorld > 1; owner = eventNum % world, the
// key e2sarDPReassembler.hpp:224-229 steers receive threads by).  The modulo runs only when
// ownership is set (a uniform branch).
__device__ __forceinline__ bool foreign_event(const ReasDev &R, uint64_t ev)
{
    return R.ownWorld > 1u && (uint32_t)(ev % R.ownWorld) != R.ownSelf;
}

// Per-packet counters of one wave (cpp:331-357): one atomic per wave per counter, sharded.
// Whole wave active.
__device__ __forceinline__ void wave_stats(const ReasDev &R, bool live, uint32_t len, bool bad, bool derr,
                                           uint32_t shard)
{
    const uint64_t np = __builtin_popcountll(__ballot(live));
    const uint64_t nbad = __builtin_popcountll(__ballot(bad));
    const uint64_t nder = __builtin_popcountll(__ballot(derr));
    // 64 lengths summed as 16-bit halves (each half-sum fits 32 bits, whatever the lengths)
    const uint32_t tl = live ? len : 0u;
    const uint64_t tb = (uint64_t)readlane(wave_incl_scan(tl & 0xFFFFu), 63) +
                        ((uint64_t)readlane(wave_incl_scan(tl >> 16), 63) << 16);
    if ((threadIdx.x & 63u) == 0) {
        ReasShard *sh = R.shards + (shard % kShards);
        if (np) atomicAdd(&sh->totalPackets, (unsigned long long)np);
        if (tb) atomicAdd(&sh->totalBytes, (unsigned long long)tb);
        if (nbad) atomicAdd(&sh->badHeaderDiscards, (unsigned long long)nbad);
        if (nder) atomicAdd(&sh->dataErrCnt, (unsigned long long)nder);
    }
}

// RE header of one datagram -> key, offset, event length, payload length (cpp:340-357;
// REHdr::validate, e2sarHeaders.hpp:98-101).  Datagrams too short for the headers are bad
// headers; one longer than its slot (a truncated receive) is a data error.  The key pass of
// the reference-order mode uses it; classify_wave below carries its own copy of the same parse.
struct ParsedHdr {
    uint64_t ev;
    uint32_t d, off, blen, pl;
    bool ok, bad, derr;
};
__device__ __forceinline__ ParsedHdr parse_hdr(const RawHdr &raw, uint32_t hl, uint32_t stride, bool live)
{
    ParsedHdr h{0, 0, 0, 0, 0, false, false, false};
    if (!live) return h;
    if (raw.len < hl) {
        h.bad = true;
    } else if (raw.len > stride) {
        h.derr = true;
    } else if (!re_valid(raw.re.x)) {
        h.bad = true;
    } else {
        h.d = bswap16(raw.re.x >> 16);
        h.off = bswap32(raw.re.y);
        h.blen = bswap32(raw.re.z);
        h.ev = ((uint64_t)bswap32(raw.re.w) << 32) | bswap32(raw.re4);
        h.pl = raw.len - hl;
        h.ok = true;
    }
    return h;
}

// Per-lane classification result; the run tail's counter update is issued during
// classification and its return value consumed only after the payload stores.
struct Classified {
    PktInfo info;
    uint64_t ev;
    uint64_t boff;
    unsigned long long old;   // value returned by the run tail's atomic add
    uint32_t d, slot, sbytes, rb, rc;
    bool tailAdd;
};

// Executed by one whole wave (all 64 lanes, any subset live).  Consecutive lanes that
// carry the same (eventNum, dataId) form a run: only the run head touches the event
// table and only the run tail adds to the event's byte/fragment counter, so the
// per-event atomics are per run, not per datagram.
// DeferAcc: the run tail's add to the event's accumulator is left to the caller (the fused
// kernel issues it after its copy, so the copy's waits never sit behind that atomic).
template <bool DeferAcc = false>
__device__ Classified classify_wave(const ReasDev &R, const RawHdr &raw, uint32_t stride, bool live,
                                    uint64_t now, uint32_t shard)
{
    const int lane = threadIdx.x & 63;
    const uint32_t hl = R.withLB ? kLBREHdrLen : kREHdrLen;

    // the same parse as parse_hdr above, written out: through parse_hdr the fused and the
    // classify kernels' register allocation changes (a change to one is a change to both)
    uint32_t len = live ? raw.len : 0u;
    bool ok = false, bad = false, derr = false;
    uint64_t ev = 0;
    uint32_t d = 0, off = 0, blen = 0, pl = 0;
    if (live) {
        if (len < hl) {
            bad = true;                                       // too short to hold the headers
        } else if (len > stride) {
            derr = true;                                      // datagram overruns its slot
        } else if (!re_valid(raw.re.x)) {
            bad = true;                                       // cpp:351-357
        } else {
            d = bswap16(raw.re.x >> 16);
            off = bswap32(raw.re.y);
            blen = bswap32(raw.re.z);
            ev = ((uint64_t)bswap32(raw.re.w) << 32) | bswap32(raw.re4);
            pl = len - hl;
            ok = true;
        }
    }
    if (ok && foreign_event(R, ev)) {                         // another rank's event: not ours
        live = false;
        ok = false;
        len = 0;
        ev = 0;
        d = off = blen = pl = 0;
    }
    // bounds against the fragment's own bufferLength, before the lookup, as the
    // reference-order key pass has it: a fragment that overruns what its own header
    // announces creates no item (it used to claim a slot and a buffer that only the GC freed,
    // as a lost event of 0 fragments)
    if (ok && (uint64_t)off + pl > blen) {
        ok = false;
        derr = true;
    }

    // ---- runs of equal keys ----
    const uint64_t pev = ((uint64_t)lane_prev((uint32_t)(ev >> 32), 0u) << 32) | lane_prev((uint32_t)ev, 0u);
    const uint64_t nev = ((uint64_t)lane_next((uint32_t)(ev >> 32), 0u) << 32) | lane_next((uint32_t)ev, 0u);
    const uint32_t pd = lane_prev(d, 0u), nd = lane_next(d, 0u);
    const uint32_t pok = lane_prev(ok ? 1u : 0u, 0u), nok = lane_next(ok ? 1u : 0u, 0u);
    const bool head = ok && (lane == 0 || !pok || pev != ev || pd != d);
    const bool tail = ok && (lane == 63 || !nok || nev != ev || nd != d);

    // (Round 3 tried a group-key pre-pass -- the first and last key of every fused group
    // resolved by a kernel of its own -- and removed it: -1 us in reas_kernel, +9 us of
    // pre-pass)
    const LookupResult lr = find_or_create(R, head, ev, d, blen, now);

    const int myhead = run_head_lane(__ballot(head), (uint32_t)lane);
    const uint32_t slot = __shfl(lr.slot, myhead);
    const uint32_t sbytes = __shfl(lr.bytes, myhead);
    const uint64_t boff = shfl_u64(lr.bufOff, myhead);

    // bounds against the event's length (the reference memcpy has no check, cpp:391)
    bool take = ok && slot != kNoSlot;
    if (take && (uint64_t)off + pl > sbytes) {
        take = false;
        derr = true;
    }
    // segmented sums over the run (inclusive scans, then difference at the head)
    const uint32_t xb = take ? pl : 0u, xc = take ? 1u : 0u;
    const uint32_t ib = wave_incl_scan(xb), ic = wave_incl_scan(xc);
    const uint32_t hb = __shfl(ib - xb, myhead), hc = __shfl(ic - xc, myhead);

    Classified out;
    out.ev = ev;
    out.d = d;
    out.slot = slot;
    out.sbytes = sbytes;
    out.boff = boff;
    out.rb = ib - hb;
    out.rc = ic - hc;
    out.old = 0;
    out.tailAdd = tail && slot != kNoSlot;
    if (out.tailAdd && !(DeferAcc && sbytes >= kDeferAccBytes)) {
        const uint64_t add = ((uint64_t)out.rc << kAccFragShift) | out.rb;
        out.old = atomicAdd(&R.slots[slot].acc, (unsigned long long)add);   // consumed in classify_finish
    }

    const bool scatter = take && boff != kNoBuf;
    out.info.dst = scatter ? (uint64_t)(R.arena + boff + off) : 0ull;
    out.info.plen = scatter ? pl : 0u;
    out.info.hl = hl;
    if (ok && slot == kNoSlot) derr = true;                    // table full / probe timeout

    wave_stats(R, live, len, bad, derr, shard);
    return out;
}

// True when this run tail's add brought curBytes to the event length (cpp:403).  An add of
// no bytes brings it nowhere: it completes only an event of length 0, as that event's first
// add.  (An empty fragment that found curBytes already at the length -- its event whole but
// not yet marked DONE -- met the length a second time: the event was delivered twice.)
__device__ __forceinline__ bool completes(const Classified &c)
{
    if (!c.tailAdd) return false;
    const uint64_t nb = (c.old & kAccBytesMask) + c.rb;
    return c.rc > 0 && nb == c.sbytes && (c.rb > 0 || c.old == 0);
}

__device__ __forceinline__ void classify_finish(const ReasDev &R, const Classified &c)
{
    if (!completes(c)) return;
    complete_event(R, c.slot, c.ev, c.boff, c.sbytes, c.d, (uint32_t)(c.old >> kAccFragShift) + c.rc);
}

}  // namespace e2sar_amd
