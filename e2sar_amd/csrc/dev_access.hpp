// dev_access.hpp -- vector types, shared launch constants, trace macros and memory accessors of the device code, and
// its wave and workgroup idioms: lane moves and reads, wave scans and min / max, the wave's LDS sync, run heads, and the
// planners' block scan and first-failure cut, and the prefix search of the launches behind them.
#pragma once

#include "sar_kernels.hpp"

namespace e2sar_amd {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 __attribute__((aligned(4))) u32x4_a4;   // 16-byte access at dword alignment

constexpr int kBlock = 256;
// Launch geometry, fixed at the measured best (DESIGN.md 4.5 holds every A/B behind these
// numbers; round 5 removed the build-time switches whose alternatives lost).
constexpr int kScatBlock = 256;             // scatter / pipelined scatter+classify workgroup
constexpr uint32_t kPollSleep = 1;          // s_sleep units (64 clocks) between table slot polls
constexpr int kReasU = 4;                   // 16-byte chunks per thread per copy round (fused kernel)
constexpr int kScatU = 4;                   // the same for the scatter forms
// ... and for slots above 4 KiB: one 8976-byte datagram (561 chunks) fills 73 % of a
// 768-chunk round instead of 55 % of 1024.  Config 3's split reassembly 210.6-212.7 ->
// 207.7-208.9 us (profiles/round5/xcd_order/ab.log; 8 chunks, two datagrams a round: 215 us)
constexpr int kScatUJumbo = 3;
constexpr int kScatBlockJumbo = 256;        // scatter workgroup size for slots above 4 KiB
// fused kernel: run tails of events of at least this many bytes add to the event
// accumulator after the copy, not during classification
constexpr uint32_t kDeferAccBytes = 4194304u;
// Split / pipelined scatter loads: non-temporal for datagrams that were written long before
// (not in the Infinity Cache), plain for a batch just written -- chosen per launch
// (launch_reas_scatter's nt; capi.cpp: E2SAR_HIP_REAS_COLD_DATAGRAMS, or a batch too large to
// be cached).  Cold: a 205 x 1 MiB batch's scatter 85.1 (nt) vs 89.3 us (plain); hot: 68.0
// (plain) vs 89.4 us (nt), reference-order batches 124.8 vs 148.1 us (profiles/round2/ab3/nt).
constexpr uint32_t kReasChunksPerBlock = 9216u;      // fused group budget before balancing

// Timeline trace (experiment builds only, -DE2SAR_TRACE=1): per workgroup, s_memrealtime
// (100 MHz) at start, after classification, after the barrier and at the end, plus HW_ID.
#ifndef E2SAR_TRACE
#define E2SAR_TRACE 0
#endif
#if E2SAR_TRACE
constexpr uint32_t kTraceBlocks = 16384;
__device__ uint64_t g_trace[3][kTraceBlocks * 4];
#define TRACE_AT(k, slot, i) \
    do { if (threadIdx.x == 0 && blockIdx.x < kTraceBlocks) g_trace[k][blockIdx.x * 4 + (slot)] = (i); } while (0)
// by the first active lane of wave 0 (inside divergent code)
#define TRACE_FIRST(k, slot, i) \
    do { if (threadIdx.x < 64 && blockIdx.x < kTraceBlocks && \
             threadIdx.x == (uint32_t)(__builtin_ffsll((long long)__ballot(1)) - 1)) \
             g_trace[k][blockIdx.x * 4 + (slot)] = (i); } while (0)
#define TRACE_WAIT() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define TRACE_AT(k, slot, i) do {} while (0)
#define TRACE_FIRST(k, slot, i) do {} while (0)
#define TRACE_WAIT() do {} while (0)
#endif
__device__ __forceinline__ uint64_t trace_now() { return __builtin_amdgcn_s_memrealtime(); }
__device__ __forceinline__ uint64_t trace_hwid()
{
    uint32_t v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(v));
    uint32_t x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    return ((uint64_t)x << 32) | v;
}

// Global-address-space accessors: the event/packet/arena pointers reach the kernels
// through descriptor tables, so without these hipcc falls back to flat_* accesses.
#define E2SAR_GLOBAL __attribute__((address_space(1)))
__device__ __forceinline__ u32x4 ld16(const uint8_t *p) { return *(const E2SAR_GLOBAL u32x4_a4 *)(p); }
__device__ __forceinline__ void st16(uint8_t *p, u32x4 v) { *(E2SAR_GLOBAL u32x4 *)(p) = v; }
__device__ __forceinline__ uint32_t ld4(const uint8_t *p) { return *(const E2SAR_GLOBAL uint32_t *)(p); }
__device__ __forceinline__ void st4(uint8_t *p, uint32_t v) { *(E2SAR_GLOBAL uint32_t *)(p) = v; }
__device__ __forceinline__ uint8_t ld1(const uint8_t *p) { return *(const E2SAR_GLOBAL uint8_t *)(p); }
// Non-temporal forms for bytes touched once: event bytes read by seg_kernel, event bytes
// written by reas_kernel.  Datagram bytes keep the default policy so a batch written by
// seg_kernel can still be in L2 / Infinity Cache when reas_kernel reads it.
__device__ __forceinline__ u32x4 ld16_nt(const uint8_t *p)
{
    return __builtin_nontemporal_load((const E2SAR_GLOBAL u32x4_a4 *)(p));
}
__device__ __forceinline__ void st16_nt(uint8_t *p, u32x4 v) { __builtin_nontemporal_store(v, (E2SAR_GLOBAL u32x4 *)(p)); }
// 16-byte non-temporal store at a dword-aligned (not 16-byte-aligned) address: event
// bytes written by the reassembly kernels.  (Round 3, profiles/round3/ab_ntstore/ and
// s2_ab_store/: cache-allocating event stores evict the batch's datagrams from the Infinity
// Cache -- reas_kernel 74 -> 108 us; write-through (sc1) stores 153-220 us.)
__device__ __forceinline__ void st16u_nt(uint8_t *p, u32x4 v) { __builtin_nontemporal_store(v, (E2SAR_GLOBAL u32x4_a4 *)(p)); }
__device__ __forceinline__ void st1(uint8_t *p, uint8_t v) { *(E2SAR_GLOBAL uint8_t *)(p) = v; }

// Agent-coherent (sc1) forms for bytes handed from one workgroup to another inside a
// launch (the chained segment -> reassemble form): the producer stores every handed-off
// byte write-through (sc1), waits for its stores, then signals with an agent-scope atomic;
// the consumer reads every handed-off byte with sc1 loads (MI355X_MICROARCH.md,
// inter-workgroup visibility, first hand-off row).  16-byte forms go through a buffer
// resource whose base is workgroup-uniform (an SGPR operand), with the per-lane offset in
// a VGPR.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t brsrc(const void *base)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), (short)0, 0x7FFFFFFF, 0x00020000);
}
constexpr int kCpolSc1 = 16;
__device__ __forceinline__ u32x4 ld16_sc1(__amdgpu_buffer_rsrc_t r, uint32_t off)
{
    return __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, kCpolSc1);
}
__device__ __forceinline__ void st16_sc1(__amdgpu_buffer_rsrc_t r, uint32_t off, u32x4 v)
{
    __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)off, 0, kCpolSc1);
}
__device__ __forceinline__ uint32_t ld4_sc1(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st4_sc1(uint32_t *p, uint32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint8_t ld1_sc1(const uint8_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Workgroup barrier that orders LDS only.  __syncthreads() also waits for every global
// load and atomic the wave has outstanding; here a classifier's fire-and-forget counter
// atomics and the payload loads of the other waves stay in flight across it.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <typename T>
__device__ __forceinline__ T ld_agent(const T *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
struct id_t_ { typedef T type; };
template <typename T>
__device__ __forceinline__ void st_agent(T *p, typename id_t_<T>::type v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src)
{
    const uint32_t lo = __shfl((uint32_t)v, src);
    const uint32_t hi = __shfl((uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}
// DPP forms of the wave's neighbour moves and its prefix sum: VALU instructions instead of
// ds_bpermute round trips through the LDS pipe (the classification runs ~30 of those in a
// dependent chain otherwise, ~1 us at kernel start).  Whole wave active.
__device__ __forceinline__ uint32_t lane_prev(uint32_t v, uint32_t fill)     // lane i <- lane i-1
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t lane_next(uint32_t v, uint32_t fill)     // lane i <- lane i+1
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112 /* row_shr:2 */, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114 /* row_shr:4 */, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118 /* row_shr:8 */, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142 /* row_bcast:15 */, 0xa, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143 /* row_bcast:31 */, 0xc, 0xf, false);
    return v;
}

// The same sum by shuffles, for any integer width (the plan kernels' 64-bit scans); `lane`
// is the caller's lane index.  Whole wave active.
template <typename T>
__device__ __forceinline__ T wave_incl_scan_shfl(T v, uint32_t lane)
{
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(v, o);
        if (lane >= o) v += y;
    }
    return v;
}

// The value lane `lane` (wave-uniform) holds, as a scalar.
__device__ __forceinline__ uint32_t readlane(uint32_t v, uint32_t lane)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}
__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, uint32_t lane)
{
    return ((uint64_t)readlane((uint32_t)(v >> 32), lane) << 32) | readlane((uint32_t)v, lane);
}

// What one wave's lanes wrote to LDS is visible to all of them after this.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The last lane at or below `lane` whose bit is set in `heads` (the head of the run the lane
// is in), or `lane` itself if there is none.
__device__ __forceinline__ int run_head_lane(uint64_t heads, uint32_t lane)
{
    const uint64_t le = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);
    const uint64_t hm = heads & le;
    return hm ? 63 - __builtin_clzll(hm) : (int)lane;
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

// Scans over a workgroup of NW waves, all threads active (`part`: NW words of LDS).
// block_scan_post scans v in the wave and posts the wave's sum; after a barrier
// block_scan_before gives the sum of the waves in front of the caller's, and of all of them
// in `total`.  block_excl_scan is the two around their barrier: the exclusive prefix of v.
// The caller keeps a barrier between a scan's reads of `part` and the next writes to it.
template <typename T>
__device__ __forceinline__ T block_scan_post(T v, T *part)
{
    const T inc = wave_incl_scan_shfl(v, threadIdx.x & 63u);
    if ((threadIdx.x & 63u) == 63u) part[threadIdx.x >> 6] = inc;
    return inc;
}
template <typename T, int NW>
__device__ __forceinline__ T block_scan_before(const T *part, T &total)
{
    T before = total = 0;
    for (uint32_t w = 0; w < (uint32_t)NW; w++) {
        if (w < (threadIdx.x >> 6)) before += part[w];
        total += part[w];
    }
    return before;
}
template <typename T, int NW>
__device__ __forceinline__ T block_excl_scan(T v, T *part, T &total)
{
    const T inc = block_scan_post(v, part);
    __syncthreads();
    return block_scan_before<T, NW>(part, total) + inc - v;
}

// The key of the first thread of the workgroup for which `fails` holds, or all ones when
// there is none -- the cut of the collect and emit planners.  The keys ascend with the thread
// index (an index, or an index above a tag).  One barrier; `part` is NW words of LDS.
template <typename K, int NW>
__device__ __forceinline__ K block_first(bool fails, K key, K *part)
{
    const uint64_t miss = __ballot(fails);
    const K first = __shfl(key, miss ? __builtin_ctzll(miss) : 0);      // the wave's first
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = miss ? first : ~(K)0;
    __syncthreads();
    K cut = ~(K)0;
    for (uint32_t w = 0; w < (uint32_t)NW; w++) cut = part[w] < cut ? part[w] : cut;
    return cut;
}

// The last entry i of [0, n) with prefix(i) <= p, by binary search: prefix is an exclusive
// prefix sum (non-decreasing, prefix(0) == 0, which is never read) of what the entries hold --
// copy pieces, seg units -- and p one of the things held; log2(n) reads.  The tie rule: an
// empty entry shares its prefix with its successor, and the last one wins, so the answer is
// never an empty entry in front of the one that holds p; trailing empty entries have the
// total as their prefix, which no p reaches.  n == 0 gives 0 without a read.
template <typename F>
__host__ __device__ constexpr uint32_t last_prefix_le(uint32_t p, uint32_t n, F prefix)
{
    uint32_t i = 0, hi = n;
    while (hi - i > 1u) {
        const uint32_t mid = (i + hi) >> 1;
        if (prefix(mid) <= p) i = mid;
        else hi = mid;
    }
    return i;
}
// entries of 2, 0, 0, 3, 0, 1 and 0 things: p at every boundary, equal prefixes in front
// (of a table cut to start with them), in the middle and at the end
namespace prefix_pins {
constexpr uint32_t kPrefixPin[] = {0, 2, 2, 2, 5, 5, 6};
constexpr uint32_t prefix_pin(uint32_t p, uint32_t n, uint32_t from = 0)
{
    return last_prefix_le(p, n, [from](uint32_t i) { return kPrefixPin[from + i] - kPrefixPin[from]; });
}
static_assert(prefix_pin(0, 0) == 0 && prefix_pin(0, 1) == 0 && prefix_pin(9, 1) == 0, "none and one entry");
static_assert(prefix_pin(0, 2) == 0 && prefix_pin(1, 2) == 0 && prefix_pin(2, 2) == 1, "two entries");
static_assert(prefix_pin(0, 2, 1) == 1 && prefix_pin(0, 3, 1) == 2 && prefix_pin(0, 4, 1) == 2 && prefix_pin(2, 4, 1) == 2 &&
                  prefix_pin(3, 4, 1) == 3,
              "equal prefixes in front: the last of them");
static_assert(prefix_pin(0, 7) == 0 && prefix_pin(1, 7) == 0 && prefix_pin(2, 7) == 3 && prefix_pin(4, 7) == 3 &&
                  prefix_pin(5, 7) == 5,
              "equal prefixes in the middle: the last of them, at every boundary");
static_assert(prefix_pin(5, 6) == 5 && prefix_pin(4, 5) == 3 && prefix_pin(4, 6) == 3, "the total's last holder");
}  // namespace prefix_pins

// i / d from d's float reciprocal rd = 1.0f / d and a +-1 correction: exact while the
// quotient is below 2^22 (the estimate is then off by less than one).  The copy kernels
// turn a chunk index into (datagram, chunk within its slot) with it.
__device__ __forceinline__ uint32_t div_recip(uint32_t i, uint32_t d, float rd)
{
    uint32_t q = (uint32_t)((float)i * rd);
    if (q * d > i) q--;
    else if ((q + 1u) * d <= i) q++;
    return q;
}

// A batch's datagram count where it lives in device memory: one scalar load per workgroup
// (count is a kernel argument, so the address and the value are wave-uniform), clamped to the
// bound the launch was sized for.  count is not NULL: a kernel whose caller may pass none
// tests for that itself (rows_kernel).  With the test in here, the kernels that never see a
// NULL paid for it where they are cheapest -- a workgroup past the count, which only reads it
// and leaves: reas_dev_kernel with 63 of 64 workgroups past it took 13.0 us against 12.5-12.7.
__device__ __forceinline__ uint32_t dev_count(const uint32_t *__restrict__ count, uint32_t bound)
{
    const uint32_t c = *count;
    return c < bound ? c : bound;
}

__device__ __forceinline__ uint32_t low_bytes_mask(uint32_t n)   // keep the n (<4) low bytes
{
    return (n >= 4u) ? 0xFFFFFFFFu : ((1u << (8u * n)) - 1u);
}

// Drop the s (0..3, lane-varying) lowest dwords of x, shifting the rest down, zero fill.
__device__ __forceinline__ u32x4 rot_down(u32x4 x, uint32_t s)
{
    u32x4 o;
    o.x = (s == 0u) ? x.x : (s == 1u) ? x.y : (s == 2u) ? x.z : x.w;
    o.y = (s == 0u) ? x.y : (s == 1u) ? x.z : (s == 2u) ? x.w : 0u;
    o.z = (s == 0u) ? x.z : (s == 1u) ? x.w : 0u;
    o.w = (s == 0u) ? x.w : 0u;
    return o;
}

// Zero the bytes of o at and past n (n in [0, 16]).
__device__ __forceinline__ u32x4 keep_low_bytes(u32x4 o, uint32_t n)
{
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const int vb = (int)n - 4 * d;
        o[d] = (vb <= 0) ? 0u : (vb < 4) ? (o[d] & low_bytes_mask((uint32_t)vb)) : o[d];
    }
    return o;
}

}  // namespace e2sar_amd
