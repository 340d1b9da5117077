// reas_copy.hpp -- the copy rounds of one group of datagrams, shared by reas_kernel and rows_kernel.
#pragma once

#include "dev_access.hpp"
#include "reas_classify.hpp"
#include "reas_store.hpp"
#include "wire.hpp"

namespace e2sar_amd {

// The copy's store windows start on this many 16-byte blocks (one 128-byte line)
constexpr uint32_t kWinAlign = 8;

// A datagram's phase: where its payload lands within a 128-byte line, bswap32(RE dword 1) &
// kPhaseMask (bufferOffset mod 128 = dst mod 128: event buffers and cells are 256-byte aligned).
// The callers of group_copy write that expression themselves, next to their classification,
// which swaps the same word: the compiler then shares the swap, as it always has.  Behind a
// function it takes the field straight from the raw word instead, and reas_kernel's code
// changes with it (other registers, other LDS waits in front of the stores).
constexpr uint32_t kPhaseMask = 16u * kWinAlign - 1u;

// The payload bytes a datagram of `len` bytes in a slot of `stride` holds behind hl header bytes
__device__ __forceinline__ uint32_t hdr_payload_len(uint32_t len, uint32_t hl, uint32_t stride)
{
    return (len >= hl) ? ((len < stride) ? len : stride) - hl : 0u;
}

// The payload of gn <= 64 consecutive datagrams [g0, g0 + gn) to the destinations their
// classification finds, by the whole workgroup of NT threads, U chunks of 16 bytes per thread
// per round.  Lane p of every wave holds datagram p's phase (gPhase, see kPhaseMask) and the
// payload length to load for it (gPlen: hdr_payload_len, or 0 for a datagram the caller knows
// it will not take);
// classify() runs between the first round's loads and the barrier, and leaves every
// datagram's destination in info (LDS).  hl: the header bytes in front of a payload.
// HO: every datagram byte is read with sc1 loads (the chained form, reas_fused.hpp).
template <int U, bool HO, int NT, class Classify>
__device__ __forceinline__ void group_copy(const uint8_t *__restrict__ pkts, uint32_t stride, uint32_t g0, uint32_t gn,
                                           uint32_t hl, uint32_t gPhase, uint32_t gPlen, const PktInfo (&info)[64],
                                           Classify classify)
{
    const uint32_t tx = threadIdx.x;

    // Index space: datagram p owns S = spc + 14 rounded down to 8 positions, and its
    // destination-aligned chunk c sits at position p * S + f + c, f = its destination's
    // 16-byte block within a 128-byte line (dst mod 128 = bufferOffset mod 128: event
    // buffers and cells are 256-byte aligned).  Position ≡ destination block (mod 8), so every
    // wave's 64 positions store whole 128-byte lines at both ends of its window.  With one
    // position per chunk (S = spc), a window started and ended inside a line, the neighbouring
    // window's store instruction wrote the rest later, and the non-temporal lines left L2 in
    // between: 1.044x the payload in writes, 103 K partial write requests per launch; here
    // 1.003x and 16 K (profiles/round6/window_align/: reas_kernel at MTU 9000 68.2-68.8 vs
    // 69.9-70.8 us, at 1500 72.0-73.4 vs 72.8-74.6).  At MTU 1500 the padding costs no
    // round: 59 datagrams fill 1.77 rounds of 3072 chunks at S = 92 and 2.0 at S = 104.
    const uint32_t spc = stride >> 4;
    const uint32_t S = (spc + 2u * (kWinAlign - 1u)) & ~(kWinAlign - 1u);
    const uint32_t nch = gn * S;
    const float rS = 1.0f / (float)S;
    const uint8_t *const bpk = pkts + (uint64_t)g0 * stride;
    const __amdgpu_buffer_rsrc_t bpkR = brsrc(bpk);                     // HO loads only
    (void)bpkR;
    // position i -> (datagram, position within its S); recomputed at store time rather than
    // kept live across the classification (register pressure sets these kernels' occupancy)
    auto split_pos = [&](uint32_t i, uint32_t &p, uint32_t &j) {
        const uint32_t ic = (i < nch) ? i : 0u;
        p = div_recip(ic, S, rS);
        j = ic - p * S;
    };
    auto issue = [&](uint32_t r0, u32x4(&xs)[U]) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t i = r0 + (uint32_t)u * NT + tx;
            uint32_t p, j;
            split_pos(i, p, j);
            const uint32_t ph = __shfl(gPhase, (int)p), plen = __shfl(gPlen, (int)p);
            const uint32_t a = ph & 15u, f = ph >> 4, c = j - f;
            uint32_t off = 0, sh;
            if (i < nch && j >= f && 16u * c < a + plen && (a & 3u) == 0u) off = p * stride + da_window(c, a, hl, stride, sh);
            xs[u] = HO ? ld16_sc1(bpkR, off) : ld16(bpk + off);
        }
    };
    auto store = [&](uint32_t r0, const u32x4(&xs)[U]) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t i = r0 + (uint32_t)u * NT + tx;
            if (i >= nch) continue;
            uint32_t p, j;
            split_pos(i, p, j);
            const PktInfo pi = info[p];
            const uint32_t f = ((uint32_t)pi.dst >> 4) & (kWinAlign - 1u);
            if (j < f) continue;
            da_store<HO>(pi, j - f, xs[u], bpk + (uint64_t)p * stride, stride);
        }
    };
    u32x4 x[U], y[U];
    // round 0 is in flight while the classification runs.  (A/B, round 4: the first residency
    // wave's groups classifying before their round-0 loads, so their claims do not queue
    // behind 25 MB of loads, ran 0.5-2 us slower; round 1's loads in flight too -- the
    // pipeline's second register set live across the classification -- cut occupancy and
    // lost: DESIGN 4.5.)
    issue(0u, x);
    classify();
    lds_barrier();
    TRACE_AT(0, 2, trace_hwid());

    // software pipeline: the loads of round r+1 are issued before the stores of round r.
    // Loads, stores and atomics retire from vmcnt in issue order, so a load issued after
    // a store can only be waited for together with that store's write acknowledgement;
    // issued before it, round r+1's data is waited for while round r's stores drain.
    constexpr uint32_t RS = (uint32_t)(NT * U);
    if (RS < nch) issue(RS, y);
    store(0u, x);
    for (uint32_t r0 = RS; r0 < nch; r0 += 2 * RS) {
        if (r0 + RS < nch) issue(r0 + RS, x);
        store(r0, y);
        if (r0 + RS >= nch) break;
        if (r0 + 2 * RS < nch) issue(r0 + 2 * RS, y);
        store(r0 + RS, x);
    }
}

}  // namespace e2sar_amd
