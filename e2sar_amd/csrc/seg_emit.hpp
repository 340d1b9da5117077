// seg_emit.hpp -- device-side production: events whose count, lengths and offsets live in device memory, planned and segmented without the host.
#pragma once

#include "dev_access.hpp"
#include "seg_device.hpp"

namespace e2sar_amd {

// ---------------------------------------------------------------------------------
// emit: the send-side mirror of collect.  A producer on the GPU leaves its events in one
// region -- rows of `pitch` bytes, or ragged at 64-bit offsets -- with their lengths and
// their count in device memory.  Two launches: emit_plan_kernel applies the Segmenter's
// per-event rules (e2sarDPSegmenter.cpp:707-728, 901-948), writes ordinary seg descriptors
// and the counts; seg_flat_kernel moves the bytes with seg_kernel's round on a flat grid the
// host sizes from bounds alone -- it knows neither how many events there are nor how long
// they are.

// One workgroup, 256 events per step (relay_plan_kernel's and collect_plan_kernel's shape).
// Per step: a block-wide scan of the datagram counts on top of a 64-bit carry; the cut is
// the first event that lies outside its source or whose datagrams would pass maxPackets,
// and nothing after it is taken, even if it would fit (event order is kept); a second scan,
// over the taken events only, gives each its first unit -- the exclusive prefix of
// ceil(npk * spc / unitChunks), kept in the descriptor's `reserved` word, where
// seg_flat_kernel searches it.  An event outside its source counts no datagrams: its length
// is not to be trusted.
__global__ __launch_bounds__(kBlock) void emit_plan_kernel(EmitSrc S, EmitNum N, uint32_t maxEvents, uint32_t maxPld,
                                                           uint32_t maxPackets, uint32_t spc, uint32_t unitChunks,
                                                           e2sar_hip_seg_event *__restrict__ out,
                                                           uint32_t *__restrict__ counts)
{
    constexpr int kWaves = kBlock / 64;
    __shared__ uint64_t waveNp[kWaves], waveCut[kWaves];
    __shared__ uint32_t waveUnits[kWaves], wavePk[kWaves];
    __shared__ uint32_t sAvail, sShort;
    if (threadIdx.x == 0) {
        uint32_t avail = maxEvents;
        if (S.count) {
            const uint32_t c = *S.count;
            avail = c < maxEvents ? c : maxEvents;
        }
        uint32_t shortBy = 0;
        if (S.pitch && S.dataBytes / S.pitch < avail) {         // rows the count names, past the source's end
            avail = (uint32_t)(S.dataBytes / S.pitch);
            shortBy = 1;
        }
        sAvail = avail;
        sShort = shortBy;
    }
    __syncthreads();
    const uint32_t avail = sAvail;
    uint32_t n = avail, why = sShort ? 2u : 0u, units = 0, pk = 0;
    uint64_t carry = 0;                                     // datagrams of the events before this step
    for (uint32_t b0 = 0; b0 < avail; b0 += kBlock) {
        const uint32_t i = b0 + threadIdx.x;
        const bool active = i < avail;
        const uint32_t bytes = active ? S.bytes[i] : 0u;
        const uint64_t off = S.pitch ? (uint64_t)i * S.pitch : active ? S.offsets[i] : 0ull;
        const bool inside = S.pitch ? bytes <= S.pitch : (off <= S.dataBytes && bytes <= S.dataBytes - off);
        const uint32_t np = (active && inside) ? bytes / maxPld + (bytes % maxPld != 0u) : 0u;
        uint64_t stepNp;
        uint32_t stepUnits, stepPk;
        const uint64_t before = carry + block_excl_scan<uint64_t, kWaves>((uint64_t)np, waveNp, stepNp);
        const bool fails = active && (!inside || before + np > maxPackets);
        // the first failing event and why it fails (2: outside its source, 1: no room), in one key
        const uint64_t first = block_first<uint64_t, kWaves>(fails, ((uint64_t)i << 32) | (inside ? 1u : 2u), waveCut);
        const uint32_t cut = (uint32_t)(first >> 32), cutWhy = (uint32_t)first;
        const bool taken = active && i < cut;
        const uint32_t nu = taken ? (uint32_t)(((uint64_t)np * spc + unitChunks - 1u) / unitChunks) : 0u;
        const uint32_t incNu = block_scan_post(nu, waveUnits);       // two scans behind one barrier
        block_scan_post(taken ? np : 0u, wavePk);
        __syncthreads();
        const uint32_t firstUnit = units + block_scan_before<uint32_t, kWaves>(waveUnits, stepUnits) + incNu - nu;
        block_scan_before<uint32_t, kWaves>(wavePk, stepPk);
        if (taken) {
            const uint64_t tick = N.lbTickBase + (uint64_t)i * N.lbTickStep;
            e2sar_hip_seg_event d;
            d.data = S.data + off;
            d.eventNum = N.ticksAsEventNum ? tick : N.eventNums ? N.eventNums[i] : N.eventNumBase + i;
            d.lbTick = tick;
            d.bytes = bytes;
            d.pktBase = (uint32_t)before;                    // every event in front of a taken one is taken
            d.dataId = (uint16_t)N.dataId;
            d.entropy = (uint16_t)(N.entropyBase + i);
            d.reserved = firstUnit;
            out[i] = d;
        }
        carry += stepNp;
        units += stepUnits;
        pk += stepPk;
        if (cut != ~0u) {                                   // the same in every thread
            n = cut;
            why = cutWhy;
            break;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        counts[0] = n;
        counts[1] = pk;
        counts[2] = avail - n;
        counts[3] = why;
        counts[4] = units;
        counts[5] = counts[6] = counts[7] = 0u;
    }
}

// One workgroup per unit: kSegBlock * U consecutive 16-byte chunks of ONE event's datagram
// range, as seg_kernel's, but numbered flat over the taken events, so an event wastes less
// than one unit whatever the bound on its length was.  The grid comes from bounds, so a
// workgroup first reads what emit_plan_kernel wrote on the stream before it: the unit total;
// a workgroup past it exits.  The others find their event by last_prefix_le over the first
// units, workgroup-uniform loads of a table that sits in L2; its tie rule keeps an empty
// event from taking its successor's units.  No XCD stripes: matching them to a reassembler
// needs a group table only the host can build (seg_groups).
template <int U>
__global__ __launch_bounds__(kSegBlock) void seg_flat_kernel(const e2sar_hip_seg_event *__restrict__ events,
                                                             const uint32_t *__restrict__ counts, int lbVersion,
                                                             uint32_t maxPld, uint8_t *__restrict__ pkts, uint32_t stride,
                                                             uint32_t *__restrict__ lens)
{
    // The workgroups without a unit are the grid's tail.  Spreading the units evenly over the
    // grid instead (unit floor(b * total / grid)) lost: with half the grid idle every other
    // workgroup works, and those all sit on four of the eight XCDs
    const uint32_t p = blockIdx.x;
    if (p >= counts[4]) return;                             // no unit: also when no event was taken
    const uint32_t e = last_prefix_le(p, counts[0], [&](uint32_t i) { return events[i].reserved; });
    seg_unit<U, false, kSegBlock>(events, e, p - events[e].reserved, lbVersion, maxPld, pkts, stride, lens, 1u, nullptr);
}

}  // namespace e2sar_amd
