// sar_kernels.hip -- gfx950 kernels of the SAR data path.
//
//   seg_kernel      : event batch -> datagram batch   (replaces _send's fragment loop,
//                     e2sarDPSegmenter.cpp:702-770)
//   emit_plan + seg_flat : the same for events whose count, lengths and offsets live in
//                     device memory, with the per-event rules in front of the loop
//                     (cpp:707-728, 901-948) applied on the device
//   reas_classify   : datagram batch -> per-packet destination + event table updates
//                     (replaces the recv body's parse/validate/find-or-create/complete,
//                     e2sarDPReassembler.cpp:335-427)
//   reas_scatter    : payload bytes -> event buffers (the memcpy at cpp:391-392)
//   reas_gc         : timeout pass (cpp:252-274)
//
// All of it is byte movement bounded by HBM bandwidth; no MFMA.  The copy kernels move
// 16 bytes per lane per access: destination chunks are 16-byte aligned, and the source
// side is read with dword-aligned 16-byte loads (gfx950 serves dword-aligned
// global_load_dwordx4), so the 4-mod-16 skew that the 36-byte header puts between event
// bytes and datagram bytes costs no shuffles.
//
// The device code sits in one header per subsystem (dev_access, seg_device, reas_table,
// reas_classify, reas_store, reas_copy, reas_fused, reas_split, reas_devcount, reas_rows, reas_order, reas_upkeep, reas_rows_ready, reas_turn, reas_collect, reas_build, seg_emit, route), all
// compiled into this one translation unit (the build has no relocatable device code:
// seg_kernel calls recycle_slots, and the E2SAR_TRACE builds share one g_trace array); below
// them, the host launchers and their launch geometry.

#include "sar_kernels.hpp"

#include "dev_access.hpp"
#include "seg_device.hpp"
#include "reas_table.hpp"
#include "reas_classify.hpp"
#include "reas_store.hpp"
#include "reas_copy.hpp"
#include "reas_fused.hpp"
#include "reas_split.hpp"
#include "reas_devcount.hpp"
#include "reas_rows.hpp"
#include "reas_order.hpp"
#include "reas_upkeep.hpp"
#include "reas_rows_ready.hpp"
#include "reas_turn.hpp"
#include "reas_collect.hpp"
#include "reas_build.hpp"
#include "seg_emit.hpp"
#include "route.hpp"
#include "wire.hpp"

#include <algorithm>
#include <atomic>
#include <type_traits>

namespace e2sar_amd {

// ---------------------------------------------------------------------------------
// launchers

static inline uint32_t cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

hipError_t launch_zero_words(void *p, uint64_t nWords, hipStream_t stream)
{
    if (nWords == 0) return hipSuccess;
    const uint64_t blocks = (nWords + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(zero_words_kernel, dim3((uint32_t)(blocks < 4096 ? blocks : 4096)), dim3(kBlock), 0, stream,
                       static_cast<uint32_t *>(p), nWords);
    return hipGetLastError();
}

hipError_t launch_fill_bytes(void *p, int value, uint64_t n, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n / 16u + kBlock - 1u) / kBlock + 1u;
    hipLaunchKernelGGL(fill_bytes_kernel, dim3((uint32_t)(blocks < 4096 ? blocks : 4096)), dim3(kBlock), 0, stream,
                       static_cast<uint8_t *>(p), (uint8_t)value, n);
    return hipGetLastError();
}

hipError_t launch_copy_spans(const CopySpans &cs, uint64_t largest, hipStream_t stream)
{
    if (cs.n == 0 || largest == 0) return hipSuccess;
    const uint64_t bx = (largest + kCopyPiece - 1) / kCopyPiece;
    if (bx > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(copy_spans_kernel, dim3((uint32_t)bx, cs.n), dim3(kBlock), 0, stream, cs);
    return hipGetLastError();
}

// Occupancy caps by dynamic LDS: the dynamic LDS that holds a launch of `kernel` (its own
// static LDS included) to at most perCU workgroups per CU on the current device, from the
// device's LDS per CU and per workgroup -- 0 (no cap) where the cap cannot be expressed.
// The caps were measured on gfx950 (160 KiB of LDS per CU); computed here, they mean the
// same workgroups per CU on any LDS size instead of a fixed byte count.
template <typename K>
static size_t occupancy_lds(K kernel, uint32_t perCU)
{
    static std::atomic<int> ldsCU[64], ldsWG[64];
    int dev = 0;
    if (perCU == 0 || hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    int cu = ldsCU[dev].load(std::memory_order_relaxed), wg = ldsWG[dev].load(std::memory_order_relaxed);
    if (cu <= 0 || wg <= 0) {
        if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess ||
            hipDeviceGetAttribute(&wg, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || cu <= 0 || wg <= 0) {
            (void)hipGetLastError();
            return 0;
        }
        ldsCU[dev].store(cu, std::memory_order_relaxed);
        ldsWG[dev].store(wg, std::memory_order_relaxed);
    }
    hipFuncAttributes fa{};
    if (hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(kernel)) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    size_t T = ((size_t)cu / perCU) & ~(size_t)1023;                  // bytes per workgroup
    if (T > (size_t)wg) T = (size_t)wg;
    if (T <= fa.sharedSizeBytes || (size_t)cu / T != perCU) return 0;  // perCU fit, perCU + 1 do not
    return T - fa.sharedSizeBytes;
}

// Workgroups of NT threads of Kernel the current device holds at once (0 if unknown); cached
// per kernel and device.
template <auto Kernel, int NT>
static uint32_t resident_groups()
{
    static std::atomic<uint32_t> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    uint32_t c = cache[dev].load(std::memory_order_relaxed);
    if (c) return c;
    int per = 0, cus = 0;
    // the uncapped occupancy, as the jumbo launch's cap was measured (balancing on the
    // capped one tied, profiles/round4/ab/reas_small_caps.log)
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, Kernel, NT, 0) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || per <= 0 || cus <= 0)
        return 0;
    c = (uint32_t)per * (uint32_t)cus;
    cache[dev].store(c, std::memory_order_relaxed);
    return c;
}

// Residency-wave balancing, for seg_geom's stripes and reas_group_size's groups (each says
// why at its call): n items go to workgroups of about `target` items each, and `cap`
// workgroups are resident at once (0 = unknown: no balancing).  Returns the count per
// workgroup, at most maxCount and within [3/4, 4/3] of target, that puts the workgroup
// count just under a whole number of residency waves -- one wave fewer than target gives,
// or as many; the nearer to target wins, the fewer waves on a tie -- or target if none fits.
constexpr uint32_t balance_waves(uint64_t n, uint32_t target, uint32_t cap, uint32_t maxCount)
{
    if (cap == 0 || n == 0) return target;
    const uint64_t waves = ((n + target - 1) / target + cap - 1) / cap;
    uint32_t best = target, bestDev = ~0u;
    for (uint64_t k = (waves > 1 ? waves - 1 : waves); k <= waves; k++) {
        const uint64_t c = (n + k * cap - 1) / (k * cap);
        if (c > maxCount || 4u * c < 3u * target || 3u * c > 4u * target) continue;
        const uint32_t dev = (uint32_t)(c > target ? c - target : target - c);
        if (dev < bestDev) best = (uint32_t)c, bestDev = dev;
    }
    return best;
}
// 205 x 1 MiB at MTU 1500 (149,855 datagrams in slots of 92 chunks; 27,060 seg units): groups
// of 64 -> 49 datagrams at 1536 resident workgroups (256 threads), -> 59 at 512 (768 threads);
// stripes of 8 -> 9 units at 1536
static_assert(balance_waves(149855, 64, 1536, 64) == 49 && balance_waves(149855, 64, 512, 64) == 59 &&
                  balance_waves(27060, 8, 1536, 0xFFFF) == 9 && balance_waves(149855, 64, 0, 64) == 64,
              "balance_waves must reproduce the measured geometries");

// Geometry of seg_kernel for a batch: 16-byte chunks per thread, units per event and the
// XCD stripe (units per stripe, 0 = none).  One place, so the reassembly group table of
// seg_groups always matches the launch.
struct SegGeom {
    uint32_t U, unitChunks, bpe, stripe;
    uint64_t nUnits;
};
static bool seg_geom(uint32_t nEvents, uint32_t maxPacketsPerEvent, uint32_t stride, SegGeom &g)
{
    const uint32_t spc = stride >> 4;
    const uint64_t chunks = (uint64_t)maxPacketsPerEvent * spc;
    if (chunks > 0xFFFFFFFFull || spc == 0) return false;        // chunk index of an event is u32
    g.U = chunks <= (1u << 18) ? 2u : 4u;
    g.unitChunks = (uint32_t)kSegBlock * g.U;
    g.bpe = cdiv(chunks, g.unitChunks);
    g.nUnits = (uint64_t)g.bpe * nEvents;
    // a stripe of about one fused reassembly group, min(49, 9216 / spc) datagrams, then
    // balanced as reas_group_size balances its groups: the stripe count (= reassembly
    // workgroups) just under a whole number of the chip's residency waves, if that keeps
    // the stripe within [3/4, 4/3] of the target (205 x 1 MiB at MTU 1500: 8 -> 9 units,
    // 3383 -> 3007 groups for 2 x 1536 resident)
    const uint32_t target = std::min<uint32_t>(49u, std::max<uint32_t>(1u, kReasChunksPerBlock / spc));
    const uint32_t S0 = std::max<uint32_t>(1u, (uint32_t)((uint64_t)target * spc / g.unitChunks));
    g.stripe = balance_waves(g.nUnits, S0, resident_groups<reas_kernel<kReasU, kBlock>, kBlock>(), 0xFFFFu);
    return true;
}

hipError_t launch_segment(const e2sar_hip_seg_event *d_events, uint32_t nEvents,
                          uint32_t maxPacketsPerEvent, int lbVersion, uint32_t maxPld,
                          uint8_t *pkts, uint32_t stride, uint32_t *lens,
                          hipStream_t stream, const uint32_t *d_count, const ReasDev *rec, bool dropCompleted)
{
    if (nEvents == 0 || maxPacketsPerEvent == 0) return rec ? launch_recycle(*rec, dropCompleted, stream) : hipSuccess;
    SegGeom sg;
    if (!seg_geom(nEvents, maxPacketsPerEvent, stride, sg)) return hipErrorInvalidValue;
    const uint64_t segGrid = sg.stripe ? (sg.nUnits + 8ull * sg.stripe - 1) / (8ull * sg.stripe) * 8ull * sg.stripe
                                       : sg.nUnits;
    const uint64_t grid = segGrid + (rec ? cdiv(rec->tableSlots > kShards ? rec->tableSlots : (uint32_t)kShards,
                                                (uint32_t)kSegBlock) : 0u);
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const ReasDev none{};
    const ReasDev &rj = rec ? *rec : none;
    const int mode = rec ? (dropCompleted ? 2 : 1) : 0;
    if (sg.U == 2)
        hipLaunchKernelGGL((seg_kernel<2>), dim3((uint32_t)grid), dim3(kSegBlock), 0, stream, d_events,
                           sg.bpe, lbVersion, maxPld, pkts, stride, lens, d_count, sg.stripe, (uint32_t)sg.nUnits, rj,
                           (uint32_t)segGrid, mode);
    else
        hipLaunchKernelGGL((seg_kernel<4>), dim3((uint32_t)grid), dim3(kSegBlock), occupancy_lds(seg_kernel<4>, kSeg4PerCU),
                           stream, d_events, sg.bpe, lbVersion, maxPld, pkts, stride, lens, d_count, sg.stripe,
                           (uint32_t)sg.nUnits, rj, (uint32_t)segGrid, mode);
    return hipGetLastError();
}

// Reassembly groups that match seg_kernel's XCD stripes for a planned batch (host event
// table with pktBase, as e2sar_hip_seg_plan fills it): group m = the datagrams whose first
// chunk lies in stripe m (units [m * stripe, (m + 1) * stripe)), written on XCD m mod 8;
// reas_kernel workgroup m runs on the same XCD.  starts[0..nGroups], nGroups + 1 <= cap.
// Returns nGroups, or 0 when the batch has no stripes or a group would exceed 64
// datagrams (the caller then reassembles with the uniform groups).
uint32_t seg_groups(const e2sar_hip_seg_event *ev, uint32_t nEvents, uint32_t maxPacketsPerEvent, uint32_t maxPld,
                    uint32_t stride, uint32_t *starts, uint32_t cap)
{
    SegGeom sg;
    if (nEvents == 0 || maxPld == 0 || !seg_geom(nEvents, maxPacketsPerEvent, stride, sg) || !sg.stripe) return 0;
    const uint64_t nGroups = (sg.nUnits + sg.stripe - 1) / sg.stripe;
    if (nGroups + 1 > cap || nGroups > 0x7FFFFFFFull) return 0;
    const uint32_t spc = stride >> 4;
    uint64_t g = 0, total = 0;
    starts[0] = 0;
    for (uint32_t e = 0; e < nEvents; e++) {
        const uint32_t np = (uint32_t)(((uint64_t)ev[e].bytes + maxPld - 1u) / maxPld);   // 0 for an empty event
        const uint32_t base = ev[e].pktBase;
        for (uint32_t q = 0; q < np; q++) {
            const uint64_t m = ((uint64_t)e * sg.bpe + (uint64_t)q * spc / sg.unitChunks) / sg.stripe;
            while (g < m) {
                starts[++g] = base + q;
                if (starts[g] - starts[g - 1] > 64u) return 0;
            }
        }
        total = (uint64_t)base + np;
    }
    while (g < nGroups) {
        starts[++g] = (uint32_t)total;
        if (starts[g] - starts[g - 1] > 64u) return 0;
    }
    return (uint32_t)nGroups;
}

hipError_t launch_relay_plan(const ReasDev &R, uint32_t first, uint32_t maxEvents, uint32_t maxPld,
                             uint64_t lbTick, uint32_t entropyBase, e2sar_hip_seg_event *d_events,
                             uint32_t *d_counts, hipStream_t stream)
{
    hipLaunchKernelGGL(relay_plan_kernel, dim3(1), dim3(kBlock), 0, stream, R, first, maxEvents, maxPld, lbTick,
                       entropyBase, d_events, d_counts);
    return hipGetLastError();
}

hipError_t launch_collect(const ReasDev &R, uint32_t first, uint32_t maxEvents, uint8_t *out, uint64_t outBytes,
                          uint32_t pitch, uint32_t align, e2sar_hip_collect_rec *d_index, uint64_t *d_counts,
                          hipStream_t stream, uint32_t *d_cursor)
{
    if (d_cursor)
        hipLaunchKernelGGL(collect_next_plan_kernel, dim3(1), dim3(kBlock), 0, stream, R, d_cursor, maxEvents, outBytes,
                           pitch, align, d_index, d_counts);
    else
        hipLaunchKernelGGL(collect_plan_kernel, dim3(1), dim3(kBlock), 0, stream, R, first, maxEvents, outBytes, pitch,
                           align, d_index, d_counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || outBytes == 0) return e;                  // no room: the plan wrote n = 0
    // The copy's grid, from bounds only: n events of B bytes in all are at most B / piece + n
    // pieces; B is at most outBytes, and at most what the arena holds (ragged) or the rows of
    // the most events there can be.  collect_copy_kernel strides over any piece beyond it.
    const uint32_t most = std::min(maxEvents, R.queueCapacity);
    const uint64_t bound = pitch ? (uint64_t)most * pitch : R.arenaBytes;
    const uint64_t grid = (std::min(outBytes, bound) + kCopyPiece - 1) / kCopyPiece + most;
    const dim3 blocks((uint32_t)std::min<uint64_t>(grid, 0x7FFFFFFFull));
    // the first taken record: from the host, or from the cursor the plan has just moved
    if (d_cursor)
        hipLaunchKernelGGL(collect_next_copy_kernel, blocks, dim3(kBlock), 0, stream, R.arena, R.completed, d_cursor, out,
                           pitch, d_index, d_counts);
    else
        hipLaunchKernelGGL(collect_copy_kernel, blocks, dim3(kBlock), 0, stream, R.arena,
                           R.completed + std::min(first, R.queueCapacity), out, pitch, d_index, d_counts);
    return hipGetLastError();
}

size_t build_work_size(uint32_t maxRecords)
{
    return (maxRecords == 0 || maxRecords > kBuildMaxRecords) ? 0 : (size_t)build_work_bytes(maxRecords);
}

uint64_t build_copy_grid(const ReasDev &R, uint32_t maxRecords, uint32_t nIds, uint64_t outBytes, uint32_t pitch,
                         uint32_t maxGroups)
{
    // Bounds only, as launch_collect's.  Ragged: the members are distinct arena events, B bytes
    // in all, at most B / piece + their number pieces.  Cells: every cell of the most groups
    // there can be.
    const uint32_t most = std::min(maxRecords, R.queueCapacity);
    if (!pitch) return (std::min(outBytes, R.arenaBytes) + kCopyPiece - 1) / kCopyPiece + most;
    const uint64_t cell = (uint64_t)nIds * pitch;
    const uint64_t n = std::min<uint64_t>(std::min(most, maxGroups), outBytes / cell);
    return n * nIds * collect_pieces(pitch);                 // below 2^12 * 2^6 * 2^19
}

hipError_t launch_build(const ReasDev &R, uint32_t first, uint32_t maxRecords, const uint16_t *ids, uint32_t nIds,
                        uint8_t *out, uint64_t outBytes, uint32_t pitch, uint32_t align, e2sar_hip_collect_rec *d_members,
                        e2sar_hip_built_rec *d_groups, uint32_t maxGroups, uint64_t *d_counts, void *d_work,
                        hipStream_t stream)
{
    const uint64_t grid = outBytes ? build_copy_grid(R, maxRecords, nIds, outBytes, pitch, maxGroups) : 0;
    if (maxRecords == 0 || maxRecords > kBuildMaxRecords || nIds > kBuildMaxIds || (pitch && !nIds) ||
        grid > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    BuildIds I{};
    for (uint32_t j = 0; j < nIds; j++) I.id[j] = ids[j];
    hipLaunchKernelGGL(build_plan_kernel, dim3(1), dim3(kBuildBlock), 0, stream, R, first, maxRecords, I, nIds, outBytes,
                       pitch, align, d_members, d_groups, maxGroups, d_counts, static_cast<uint8_t *>(d_work));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || grid == 0) return e;                       // no room: the plan took nothing
    hipLaunchKernelGGL(build_copy_kernel, dim3((uint32_t)grid), dim3(kBlock), 0, stream, R.arena, out, pitch, nIds,
                       d_members, d_groups, d_counts, static_cast<const uint8_t *>(d_work));
    return hipGetLastError();
}

uint32_t seg_emit_u(uint64_t boundBytes, uint32_t maxPld, uint32_t stride)
{
    if (boundBytes == 0 || maxPld == 0) return 4u;
    const uint64_t chunks = (boundBytes + maxPld - 1) / maxPld * (stride >> 4);
    return chunks <= (1u << 18) ? 2u : 4u;                    // seg_geom's rule
}

uint64_t seg_emit_grid(uint32_t maxEvents, uint32_t maxPackets, uint32_t stride, uint32_t U)
{
    const uint64_t chunks = (uint64_t)maxPackets * (stride >> 4);
    if (chunks > 0xFFFFFFFFull || (stride >> 4) == 0) return 0;
    const uint64_t unitChunks = (uint64_t)kSegBlock * U;
    return (chunks + unitChunks - 1) / unitChunks + maxEvents;
}

hipError_t launch_seg_emit(const EmitSrc &S, const EmitNum &N, uint32_t maxEvents, int lbVersion, uint32_t maxPld,
                           uint8_t *pkts, uint32_t stride, uint32_t maxPackets, uint32_t *lens,
                           e2sar_hip_seg_event *d_events, uint32_t *d_counts, uint32_t U, hipStream_t stream)
{
    const uint64_t grid = seg_emit_grid(maxEvents, maxPackets, stride, U);
    if (maxEvents == 0 || maxPld == 0 || grid == 0 || grid > 0x7FFFFFFFull || (U != 2u && U != 4u)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(emit_plan_kernel, dim3(1), dim3(kBlock), 0, stream, S, N, maxEvents, maxPld, maxPackets, stride >> 4,
                       (uint32_t)kSegBlock * U, d_events, d_counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // n events of C chunks in all are at most C / unit + n units: the grid never undercounts
    if (U == 2)
        hipLaunchKernelGGL((seg_flat_kernel<2>), dim3((uint32_t)grid), dim3(kSegBlock), 0, stream, d_events, d_counts,
                           lbVersion, maxPld, pkts, stride, lens);
    else
        hipLaunchKernelGGL((seg_flat_kernel<4>), dim3((uint32_t)grid), dim3(kSegBlock),
                           occupancy_lds(seg_flat_kernel<4>, kSeg4PerCU), stream, d_events, d_counts, lbVersion, maxPld, pkts,
                           stride, lens);
    return hipGetLastError();
}

// Where the pipelined launch's classify workgroups sit, percent of the way through its
// scatter workgroups (launch_reas_scatter_classify)
constexpr uint32_t kPipeClsAtPercent = 75;

// Scatter workgroups of the launch: groups of G whole datagrams; returns G and the
// workgroup count.
__host__ __device__ constexpr int scatter_u(uint32_t stride) { return stride > 4096u ? kScatUJumbo : kScatU; }
__host__ __device__ constexpr int scatter_tb(uint32_t stride) { return stride > 4096u ? kScatBlockJumbo : kScatBlock; }
static uint32_t scatter_group_size(uint32_t stride)
{
    // datagrams per scatter workgroup: at most one round of 16-byte chunks (256 threads x
    // scatter_u), <= 64.  The scatter needs no table round trip, so it
    // streams best in one-round workgroups, like seg_kernel: at 205 x 1 MiB, MTU 1500, a
    // batch read back cold takes 81.5 us with 1K-chunk groups against 100.3 us with the
    // fused kernel's 9K budget (89.5 us at 2K); hot, 68.7 us.
    const uint32_t spc = stride >> 4;
    uint32_t G = 64;
    while (G > 1 && G * spc > (uint32_t)(scatter_tb(stride) * scatter_u(stride))) G >>= 1;
    return G;
}
static uint32_t scatter_geometry(uint32_t stride, uint32_t n, uint32_t &blocks)
{
    const uint32_t G = scatter_group_size(stride);
    blocks = cdiv(n, G);
    return G;
}

// fixedG: the reassembler's configured group size (e2sar_hip_reas_config.groupSize), 0 = auto;
// resident: resident_groups of the kernel that will run the groups
static uint32_t reas_group_size(uint32_t n, uint32_t stride, uint32_t fixedG, uint32_t (*resident)())
{
    if (fixedG) return fixedG < 64u ? fixedG : 64u;
    // datagrams per workgroup: at most kReasChunksPerBlock 16-byte chunks, <= 64.
    // (A/B: at MTU 1500 2K-chunk groups lose ~8 %, 1K ~30 %, 4K-12K equal; at MTU 9000 with
    // 8 MiB events 4K chunks (4 datagrams per group) lose 27 % to 9K-18K: per-event counter
    // and table traffic grows with groups per event)
    const uint32_t spc = stride >> 4, budget = kReasChunksPerBlock;
    uint32_t G = 64;
    while (G > 1 && G * spc > budget) G >>= 1;
    // Balance the launch over whole residency waves: with ceil(n/G) workgroups = 1.5 x
    // what the chip holds at once, the second wave starts late and the last ~15 us run
    // half-empty (tools/trace_reas.py). Pick G so the workgroup count is just under a
    // whole number of waves -- one wave more (smaller G) or one fewer (larger G) -- if
    // that keeps G within [3/4, 4/3] of the budget's G: much smaller groups put more
    // workgroups on each event's table slot and counter (8 MiB events at MTU 9000 lose
    // 9 % at G 16 -> 10). 205 x 1 MiB at MTU 1500: G 64 -> 49, 2342 -> 3059 groups,
    // reas_kernel 79.0 -> 77.6 us.
    return balance_waves(n, G, resident(), 64u);
}

// The jumbo-slot launch (512 threads) at most 2 workgroups per CU (16 waves instead of 24):
// MTU 9000 reas_kernel 71.2 -> 69.3 us (profiles/round4/ab/jumbo_cold_caps.log); the
// 768-thread launch is at 2 per CU by its registers already, and a cap there changes
// nothing (reas_caps.log).
constexpr uint32_t kReasJumboPerCU = 2;

// The fused kernels' workgroup size for a slot stride (reas_threads), handed to f as a value
// whose type carries it; and the dynamic LDS of a launch of that size: the jumbo cap.
template <typename F>
static void with_reas_threads(uint32_t stride, F f)
{
    reas_threads(stride) == kReasNTSmall ? f(std::integral_constant<int, kReasNTSmall>{})
                                         : f(std::integral_constant<int, kReasNTJumbo>{});
}
template <int NT, typename K>
static size_t reas_lds(K kernel)
{
    if constexpr (NT == kReasNTJumbo) return occupancy_lds(kernel, kReasJumboPerCU);
    else return 0;
}

// With d_count the batch is min(*d_count, n) datagrams: the group size, the grid and the
// kernel's size are those of a batch of n, the only number the host has.
hipError_t launch_reassemble(const ReasDev &R, const uint8_t *pkts, uint32_t stride, const uint32_t *lens, uint32_t n,
                             uint64_t now, hipStream_t stream, const uint32_t *d_count)
{
    constexpr int U = kReasU;
    if (n == 0) return hipSuccess;
    with_reas_threads(stride, [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        const uint32_t G = reas_group_size(n, stride, R.groupSize, resident_groups<reas_kernel<U, NT>, NT>);
        const dim3 groups(cdiv(n, G));
        if (d_count)
            hipLaunchKernelGGL((reas_dev_kernel<U, NT>), groups, dim3(NT), reas_lds<NT>(reas_dev_kernel<U, NT>), stream, R,
                               pkts, stride, lens, d_count, n, now, G);
        else
            hipLaunchKernelGGL((reas_kernel<U, NT>), groups, dim3(NT), reas_lds<NT>(reas_kernel<U, NT>), stream, R, pkts,
                               stride, lens, n, now, G, (const uint32_t *)nullptr);
    });
    return hipGetLastError();
}

// ---- rows family (reas_rows.hpp) ----

// The launch's geometry for a bound of maxPackets: G datagrams per workgroup -- reas_kernel's
// rule (reas_group_size), balanced over this kernel's residency; returns the grid.
// lattice: the window's eventStep is above 1; seen: a seen call -- the kernel is the instantiation that knows either.
static uint64_t rows_geometry(uint32_t maxPackets, uint32_t stride, bool lattice, bool seen, uint32_t &G)
{
    with_reas_threads(stride, [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        uint32_t (*const resident[4])() = {
            resident_groups<rows_kernel<kReasU, NT>, NT>, resident_groups<rows_kernel<kReasU, NT, true>, NT>,
            resident_groups<rows_kernel<kReasU, NT, false, true>, NT>, resident_groups<rows_kernel<kReasU, NT, true, true>, NT>};
        G = reas_group_size(maxPackets, stride, 0u, resident[(seen ? 2 : 0) + (lattice ? 1 : 0)]);
    });
    return ((uint64_t)maxPackets + G - 1u) / G;
}

uint64_t rows_grid(uint32_t maxPackets, uint32_t stride, bool lattice)
{
    uint32_t G = 1;
    return rows_geometry(maxPackets, stride, lattice, false, G);
}
uint64_t rows_seen_grid(uint32_t maxPackets, uint32_t stride, bool lattice)
{
    uint32_t G = 1;
    return rows_geometry(maxPackets, stride, lattice, true, G);
}

// One launch of rows_kernel<., ., LAT, SEEN>; Z is the seen calls' argument, or the plain calls' empty one
template <bool LAT, bool SEEN>
static hipError_t launch_rows_as(const RowsDev &W, const RowsSeenArg<SEEN> &Z, const uint8_t *pkts, uint32_t stride,
                                 const uint32_t *lens, const uint32_t *d_count, uint32_t maxPackets, hipStream_t stream)
{
    constexpr int U = kReasU;
    if (maxPackets == 0) return hipSuccess;
    uint32_t G = 1;
    const uint64_t grid = rows_geometry(maxPackets, stride, LAT, SEEN, G);
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    with_reas_threads(stride, [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        hipLaunchKernelGGL((rows_kernel<U, NT, LAT, SEEN>), dim3((uint32_t)grid), dim3(NT),
                           reas_lds<NT>(rows_kernel<U, NT, LAT, SEEN>), stream, W, pkts, stride, lens, d_count, maxPackets, G, Z);
    });
    return hipGetLastError();
}

hipError_t launch_rows(const RowsDev &W, const uint8_t *pkts, uint32_t stride, const uint32_t *lens,
                       const uint32_t *d_count, uint32_t maxPackets, hipStream_t stream)
{
    return W.step > 1u ? launch_rows_as<true, false>(W, RowsNoSeen{}, pkts, stride, lens, d_count, maxPackets, stream)
                       : launch_rows_as<false, false>(W, RowsNoSeen{}, pkts, stride, lens, d_count, maxPackets, stream);
}

hipError_t launch_rows_seen(const RowsDev &W, const RowsSeenDev &Z, const uint8_t *pkts, uint32_t stride, const uint32_t *lens,
                            const uint32_t *d_count, uint32_t maxPackets, hipStream_t stream)
{
    return W.step > 1u ? launch_rows_as<true, true>(W, Z, pkts, stride, lens, d_count, maxPackets, stream)
                       : launch_rows_as<false, true>(W, Z, pkts, stride, lens, d_count, maxPackets, stream);
}

hipError_t launch_rows_advance(const RowsDev &W, const uint32_t *d_k, uint32_t kMax, hipStream_t stream)
{
    const uint64_t cells = (uint64_t)(kMax < W.nEvents ? kMax : W.nEvents) * W.nIds;     // <= 2^32 - 1
    if (cells == 0) return hipSuccess;
    hipLaunchKernelGGL(rows_release_kernel, dim3(cdiv(cells, kBlock)), dim3(kBlock), 0, stream, W, d_k, kMax);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rows_shift_kernel, dim3(1), dim3(64), 0, stream, W, d_k, kMax);
    return hipGetLastError();
}

// cdiv(min(kMax, nEvents) * nIds * (maxFrags / 128), kBlock): the workgroups of rows_release_seen_kernel
uint64_t rows_release_seen_grid(const RowsDev &W, const RowsSeenDev &Z, uint32_t kMax)
{
    const uint64_t words = (uint64_t)(kMax < W.nEvents ? kMax : W.nEvents) * W.nIds * (Z.maxFrags >> 7);  // < 2^57
    return (words + kBlock - 1u) / kBlock;
}

hipError_t launch_rows_advance_seen(const RowsDev &W, const RowsSeenDev &Z, const uint32_t *d_k, uint32_t kMax,
                                    hipStream_t stream)
{
    const uint64_t grid = rows_release_seen_grid(W, Z, kMax);
    if (grid == 0) return hipSuccess;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rows_release_seen_kernel, dim3((uint32_t)grid), dim3(kBlock), 0, stream, W, Z, d_k, kMax);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rows_shift_kernel, dim3(1), dim3(64), 0, stream, W, d_k, kMax);
    return hipGetLastError();
}

// min(kMax, nEvents) * nIds * ceil(pitch / kCopyPiece): the workgroups of rows_zero_kernel
uint64_t rows_zero_grid(const RowsDev &W, uint32_t kMax)
{
    return (uint64_t)(kMax < W.nEvents ? kMax : W.nEvents) * W.nIds * (((uint64_t)W.pitch + kCopyPiece - 1u) / kCopyPiece);
}

size_t rows_ready_work_bytes(uint32_t nEvents) { return rows_ready_work_size(nEvents); }

hipError_t launch_rows_ready(const RowsDev &W, uint64_t required, uint32_t slack, uint32_t kMax, bool zero, uint32_t *d_ready,
                             e2sar_hip_rows_event *d_events, void *d_work, hipStream_t stream)
{
    const uint64_t pieces = zero ? rows_zero_grid(W, kMax) : 0;
    if (pieces > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rows_scan_kernel, dim3(cdiv(W.nEvents, kBlock)), dim3(kBlock), 0, stream, W, d_work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rows_ready_kernel, dim3(1), dim3(kBlock), 0, stream, W, RowsRule{required, slack, kMax}, d_work, d_ready,
                       d_events);
    e = hipGetLastError();
    if (e != hipSuccess || pieces == 0) return e;
    hipLaunchKernelGGL(rows_zero_kernel, dim3((uint32_t)pieces), dim3(kBlock), 0, stream, W, (const uint32_t *)d_ready,
                       (uint32_t)(((uint64_t)W.pitch + kCopyPiece - 1u) / kCopyPiece));
    return hipGetLastError();
}

hipError_t launch_rows_clear(const RowsDev &W, uint64_t eventBase, hipStream_t stream)
{
    const uint64_t blocks = ((uint64_t)W.nEvents * W.nIds + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(rows_clear_kernel, dim3((uint32_t)(blocks < 4096 ? blocks : 4096)), dim3(kBlock), 0, stream, W,
                       eventBase);
    return hipGetLastError();
}

hipError_t launch_rows_clear_seen(const RowsDev &W, const RowsSeenDev &Z, uint64_t eventBase, hipStream_t stream)
{
    const uint64_t blocks = ((uint64_t)W.nEvents * W.nIds * (Z.maxFrags >> 7) + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(rows_clear_seen_kernel, dim3((uint32_t)(blocks < 4096 ? blocks : 4096)), dim3(kBlock), 0, stream, W, Z,
                       eventBase);
    return hipGetLastError();
}

#if E2SAR_HIP_EXPERIMENTAL
hipError_t launch_reassemble_groups(const ReasDev &R, const uint8_t *pkts, uint32_t stride, const uint32_t *lens,
                                    uint32_t n, const uint32_t *starts, uint32_t nGroups, uint64_t now,
                                    hipStream_t stream)
{
    constexpr int U = kReasU;
    if (n == 0 || nGroups == 0) return hipSuccess;
    hipLaunchKernelGGL((reas_kernel<U, kBlock>), dim3(nGroups), dim3(kBlock), 0, stream, R, pkts, stride, lens, n, now, 64u,
                       starts);
    return hipGetLastError();
}

hipError_t launch_segreas(ChainBatches cb, int lbVersion, uint32_t maxPld, uint32_t stride, const ReasDev &R,
                          uint64_t now, hipStream_t stream)
{
    constexpr int U = kReasU;
    if (cb.nb == 0 || cb.nb > kChainMaxBatches) return hipErrorInvalidValue;
    uint64_t grid = 0;
    for (uint32_t b = 0; b < cb.nb; b++) {
        ChainBatch &B = cb.b[b];
        const uint64_t chunks = (uint64_t)B.maxPacketsPerEvent * (stride >> 4);
        if (chunks > 0xFFFFFFFFull) return hipErrorInvalidValue;
        B.bpe = (B.nEvents && B.n) ? cdiv(chunks, (uint64_t)kBlock * kChainSegU) : 0u;
        B.G = B.n ? reas_group_size(B.n, stride, R.groupSize, resident_groups<reas_kernel<U, kBlock>, kBlock>) : 1u;
        B.start = (uint32_t)grid;
        B.nSeg = B.bpe * B.nEvents;
        grid += (uint64_t)B.nSeg + (B.n ? cdiv(B.n, B.G) : 0u);
        if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    }
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL((segreas_kernel<U>), dim3((uint32_t)grid), dim3(kBlock), 0, stream, cb, lbVersion, maxPld, stride,
                       R, now);
    return hipGetLastError();
}

#endif  // E2SAR_HIP_EXPERIMENTAL

// With d_count (here and in launch_reas_scatter) the batch is min(*d_count, n) datagrams:
// the grids, the scatter group size and the work view are those of a batch of n.
hipError_t launch_reas_classify(const ReasDev &R, const uint8_t *pkts, uint32_t stride, const uint32_t *lens,
                                uint32_t n, uint64_t now, void *work, hipStream_t stream, const uint32_t *d_count)
{
    if (n == 0) return hipSuccess;
    const WorkView w = work_view(work, n);
    const dim3 grid(cdiv(n, kBlock));
    if (d_count)
        hipLaunchKernelGGL(reas_classify_dev_kernel, grid, dim3(kBlock), 0, stream, R, pkts, stride, lens, d_count, n, now,
                           w.info, w.fin);
    else
        hipLaunchKernelGGL(reas_classify_kernel, grid, dim3(kBlock), 0, stream, R, pkts, stride, lens, n, now, w.info, w.fin);
    return hipGetLastError();
}

// Staged stores (scatter_group<..., STAGE>: a one-round group's chunks pass through LDS so
// every event store is a whole aligned 16-byte store) per launch.  Measured per user,
// interleaved on one box (profiles/round4/ab/scatter_stores_*.log): config 3's split scatter
// (MTU 9000, streaming) 232.0-232.3 vs 235.9-236.4 us; cold leg at MTU 9000 83.4 vs 84.9-86.4
// us; hot split scatter at MTU 1500 67.3-67.5 vs 68.5-68.7 us; reference-order batches
// 123.0-123.6 vs 125.2-125.4 us; but the cold leg at MTU 1500 (8-datagram groups read from
// HBM, where the LDS barrier waits for the slowest of the group's loads) 84.9-85.5 vs
// 83.0-83.3 us.  So: staged unless the datagrams stream in at small strides.
static bool scatter_stage(uint32_t stride, bool nt) { return !nt || stride > 2048u; }

// An unstaged streaming scatter launch (cold datagrams at small strides) at most 6
// workgroups per CU instead of 8.  Round 4, cold leg at MTU 1500
// (profiles/round4/ab/scatter_occupancy.log): 82.7 vs 83.5-83.9 us per pipelined launch at
// 6 per CU, 84.8-86.0 at 5, 88.0-88.8 at 4; staged launches (their own 18 KiB of LDS) lose
// with any cap (config 3 284-286 vs 232 us at 3 per CU), so they keep none.
constexpr uint32_t kColdScatterPerCU = 6;
template <typename K>
static size_t scatter_lds(K kernel, bool stage, bool nt)
{
    return (!stage && nt) ? occupancy_lds(kernel, kColdScatterPerCU) : 0;
}

// The scatter kernels' template arguments for a slot stride and load policy: chunks per
// thread, streaming loads, staged stores, workgroup size.  with_scatter_variant hands the
// chosen set to f as a value whose type carries them, so the scatter and the pipelined
// scatter+classify launches instantiate the same six variants from one choice.
template <int U_, bool NT_, bool STAGE_, int TB_>
struct ScatterVariant {
    static constexpr int U = U_, TB = TB_;
    static constexpr bool NT = NT_, STAGE = STAGE_;
};
template <typename F>
static void with_scatter_variant(uint32_t stride, bool nt, F f)
{
    constexpr int U = kScatU, UJ = kScatUJumbo, TB = kScatBlock, TJ = kScatBlockJumbo;
    const bool st = scatter_stage(stride, nt);
    if (scatter_u(stride) == UJ) nt ? f(ScatterVariant<UJ, true, true, TJ>{}) : f(ScatterVariant<UJ, false, true, TJ>{});
    else if (nt) st ? f(ScatterVariant<U, true, true, TB>{}) : f(ScatterVariant<U, true, false, TB>{});
    else st ? f(ScatterVariant<U, false, true, TB>{}) : f(ScatterVariant<U, false, false, TB>{});
}

hipError_t launch_reas_scatter(const ReasDev &R, const uint8_t *pkts, uint32_t stride, uint32_t n,
                               const void *work, hipStream_t stream, bool nt, const uint32_t *d_count)
{
    if (n == 0) return hipSuccess;
    const WorkView w = work_view(work, n);
    uint32_t blocks = 0;
    const uint32_t G = scatter_geometry(stride, n, blocks);
    with_scatter_variant(stride, nt, [&](auto v) {
        using V = decltype(v);
        const auto launch = [&](auto kernel, auto... count) {
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(V::TB), scatter_lds(kernel, V::STAGE, V::NT), stream, R, pkts, stride,
                               count..., n, G, (const PktInfo *)w.info, (const FinishRec *)w.fin);
        };
        if (d_count) launch(reas_scatter_dev_kernel<V::U, V::NT, V::STAGE, V::TB>, d_count);
        else launch(reas_scatter_kernel<V::U, V::NT, V::STAGE, V::TB>);
    });
    return hipGetLastError();
}

hipError_t launch_reas_scatter_classify(const ReasDev &R, uint32_t stride, const uint8_t *spk, uint32_t sn,
                                        const void *swork, const uint8_t *cpk, const uint32_t *clens, uint32_t cn,
                                        uint64_t now, void *cwork, hipStream_t stream, bool nt)
{
    if (cn == 0) return launch_reas_scatter(R, spk, stride, sn, swork, stream, nt);
    if (sn == 0) return launch_reas_classify(R, cpk, stride, clens, cn, now, cwork, stream);
    const WorkView sw = work_view(swork, sn), cw = work_view(cwork, cn);
    uint32_t sblocks = 0;
    const uint32_t G = scatter_geometry(stride, sn, sblocks);
    const uint32_t nCls = (cdiv(cn, (uint32_t)scatter_tb(stride)) + 7u) & ~7u;     // multiples of 8: see xcd_runs
    // where the classify workgroups sit in the grid: kPipeClsAtPercent of the way
    // through the scatter workgroups.  At the front (0, round 2's form) they hold ~590
    // workgroup slots through their dependent round trips while the scatter ramps up; three
    // quarters of the way in they run beside the scatter's last quarter and finish with it
    // (cold leg, 205 x 1 MiB: 81.4-83.8 vs 83.9-87.0 us per launch over three boxes, 50 / 65 /
    // 80 / 88 % in between; profiles/round3/s3_cls/)
    const uint32_t clsStart = (uint32_t)((uint64_t)sblocks * kPipeClsAtPercent / 100u) & ~7u;
    with_scatter_variant(stride, nt, [&](auto v) {
        using V = decltype(v);
        const auto kernel = reas_scatter_classify_kernel<V::U, V::NT, V::STAGE, V::TB>;
        hipLaunchKernelGGL(kernel, dim3(nCls + sblocks), dim3(V::TB), scatter_lds(kernel, V::STAGE, V::NT), stream, R, stride,
                           spk, sn, G, (const PktInfo *)sw.info, (const FinishRec *)sw.fin, cpk, clens, cn, now, cw.info,
                           cw.fin, nCls, clsStart);
    });
    return hipGetLastError();
}

hipError_t launch_ro_classify(const ReasDev &R, const uint8_t *pkts, uint32_t stride, const uint32_t *lens,
                              uint32_t n, uint64_t now, void *work, void *scratch, size_t scratchBytes,
                              hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    size_t need;
    const RoScratch sc = ro_scratch_layout(scratch, n, R.tableSlots, &need);
    if (need > scratchBytes) return hipErrorInvalidValue;
    const WorkView w = work_view(work, n);
    hipLaunchKernelGGL((ro_key_kernel<kRoKeyBlock>), dim3(cdiv(n, (uint32_t)kRoKeyBlock)), dim3(kRoKeyBlock), 0, stream,
                       R, pkts, stride, lens, n, now, sc, w.info);
    hipLaunchKernelGGL(ro_place_kernel, dim3(kPlaceBlocks), dim3(kPlaceThreads), 0, stream, sc, R.tableSlots, n);
    // one wave per key: at most min(n, tableSlots) keys
    const uint32_t waves = n < R.tableSlots ? n : R.tableSlots;
    hipLaunchKernelGGL((ro_walk_kernel<1, kRoWalkLds>), dim3(waves), dim3(64), 0, stream, R, sc, R.tableSlots, now, w.info,
                       w.fin);
    return hipGetLastError();
}

hipError_t launch_gc(const ReasDev &R, uint64_t now, uint64_t timeout, hipStream_t stream)
{
    hipLaunchKernelGGL(reas_gc_kernel, dim3(cdiv(R.tableSlots, kBlock)), dim3(kBlock), 0, stream, R,
                       now, timeout);
    return hipGetLastError();
}

hipError_t launch_recycle(const ReasDev &R, bool dropCompleted, hipStream_t stream)
{
    hipLaunchKernelGGL(reas_recycle_kernel, dim3(cdiv(R.tableSlots, kBlock)), dim3(kBlock), 0, stream,
                       R, dropCompleted ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_compact(const ReasDev &from, const ReasDev &to, hipStream_t stream)
{
    hipError_t e = launch_zero_words(to.slots, sizeof(ReasSlot) / 4 * (uint64_t)to.tableSlots, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(reas_compact_kernel, dim3(from.tableSlots), dim3(kBlock), 0, stream, from, to);
    hipLaunchKernelGGL(reas_compact_finish, dim3(1), dim3(1), 0, stream, to);
    return hipGetLastError();
}

hipError_t launch_turn(const ReasDev &R, const ReasDev &alt, uint32_t *d_cursor, const e2sar_hip_turn_marks &marks,
                       uint64_t *d_status, void *moves, hipStream_t stream)
{
    static_assert(sizeof(TurnMove) == kTurnMoveBytes, "the move list is allocated by this size");
    // four launches whatever the device decides; the grids come from tableSlots alone
    const TurnMarks M{marks.arenaMark, marks.recordMark, marks.tableMark, marks.maxCarries};
    TurnMove *mv = static_cast<TurnMove *>(moves);
    const uint32_t tableGroups = cdiv(R.tableSlots, kBlock);
    hipLaunchKernelGGL(turn_decide_kernel, dim3(std::min<uint32_t>(4u * tableGroups, 4096u)), dim3(kBlock), 0, stream, R,
                       alt.slots, d_cursor, M, d_status);
    hipLaunchKernelGGL(turn_out_kernel, dim3(tableGroups), dim3(kBlock), 0, stream, R, alt, M.maxCarries, mv, d_status);
    hipLaunchKernelGGL(turn_copy_kernel, dim3(kTurnCopyGroups), dim3(kBlock), 0, stream, R.arena, alt.arena, R.ctl, mv,
                       d_status);
    hipLaunchKernelGGL(turn_back_kernel, dim3(tableGroups + kTurnCopyGroups), dim3(kBlock), 0, stream, alt, R, tableGroups,
                       mv, d_cursor, d_status);
    return hipGetLastError();
}

hipError_t launch_route_append(const uint8_t *pkts, uint32_t stride, const uint32_t *lens, uint32_t n, int withLB,
                               uint32_t world, uint32_t self, int excludeSelf, uint8_t *out, uint32_t *outLens,
                               uint32_t cap, uint32_t *running, hipStream_t stream)
{
    if (world == 0 || world > kMaxWorld || self >= world || cap == 0) return hipErrorInvalidValue;
    if ((uint64_t)cap * world > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(route_append_kernel, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, stream, pkts, stride, lens, n, withLB,
                       world, self, excludeSelf, cap, running, out, outLens);
    return hipGetLastError();
}

size_t route_workspace_bytes(uint32_t n, uint32_t world)
{
    const uint64_t nb = (n + kBlock - 1) / kBlock;
    return (size_t)((nb * world + world) * sizeof(uint32_t));
}

hipError_t launch_route(const uint8_t *pkts, uint32_t stride, const uint32_t *lens, uint32_t n, int withLB,
                        uint32_t world, uint32_t self, int excludeSelf, uint8_t *out, uint32_t *outLens,
                        uint32_t *counts, void *workspace, hipStream_t stream)
{
    if (world == 0 || world > kMaxWorld || self >= world) return hipErrorInvalidValue;
    if (n == 0) return counts ? launch_zero_words(counts, world, stream) : hipSuccess;
    const uint32_t nb = cdiv(n, kBlock);
    uint32_t *blockHist = static_cast<uint32_t *>(workspace);
    uint32_t *destBase = blockHist + (size_t)nb * world;
    hipLaunchKernelGGL(route_hist_kernel, dim3(nb), dim3(kBlock), 0, stream, pkts, stride, lens, n, withLB, world,
                       self, excludeSelf, blockHist);
    hipLaunchKernelGGL(route_scan_kernel, dim3(1), dim3(kBlock), 0, stream, blockHist, nb, world, counts, destBase);
    hipLaunchKernelGGL(route_pack_kernel, dim3(nb * kPackSplit), dim3(kBlock), 0, stream, pkts, stride, lens, n, withLB, world,
                       self, excludeSelf, blockHist, destBase, out, outLens);
    return hipGetLastError();
}

}  // namespace e2sar_amd

#if E2SAR_TRACE
// Experiment builds only: copy the timeline of the last reas_kernel (k = 0) or seg_kernel
// (k = 1) launch, 4 words per workgroup, to host memory.
extern "C" int e2sar_hip_debug_trace(int k, uint64_t *out, size_t words)
{
    if (k < 0 || k > 2 || words > e2sar_amd::kTraceBlocks * 4) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(e2sar_amd::g_trace), words * 8, (size_t)k * e2sar_amd::kTraceBlocks * 4 * 8,
                               hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
extern "C" int e2sar_hip_debug_trace_clear(void)
{
    static uint64_t zero[3 * e2sar_amd::kTraceBlocks * 4];
    return hipMemcpyToSymbol(HIP_SYMBOL(e2sar_amd::g_trace), zero, sizeof(zero)) == hipSuccess ? 0 : -1;
}
#endif
