// reas_devcount.hpp -- reassembly of a batch whose datagram count lives in device memory (e2sar_hip_reassemble_batch_dev).
#pragma once

#include "dev_access.hpp"
#include "reas_fused.hpp"
#include "reas_split.hpp"

namespace e2sar_amd {

// ---------------------------------------------------------------------------------
// The fused, classify and scatter kernels over n = min(*count, bound) datagrams, where only
// the bound is known when the launch is made: the host sizes the grid, the group size and
// the work buffer's layout from the bound, and every workgroup reads the count itself.  The
// kernels are the wrappers reas_kernel, reas_classify_kernel and reas_scatter_kernel are,
// over the same device functions (reas_group, classify_wave_to_work, scatter_group), handed n
// instead of the host's number; a workgroup whose group lies at or past n costs the load of
// one word and an exit -- no header load, no LDS, no counter.  So no byte of a slot and no
// length at or past n is read, and n = 0 leaves the reassembler as it was.  n is dev_count
// (dev_access.hpp).

// reas_kernel<U, NT> with the count read on the device: workgroup b reassembles datagrams
// [b*G, b*G + G) of the first n; the grid is cdiv(bound, G).
template <int U, int NT>
__global__ __launch_bounds__(NT) void reas_dev_kernel(ReasDev R, const uint8_t *__restrict__ pkts, uint32_t stride,
                                                      const uint32_t *__restrict__ lens,
                                                      const uint32_t *__restrict__ count, uint32_t bound, uint64_t now,
                                                      uint32_t G)
{
    __shared__ ReasGroupLds L;
    const uint32_t n = dev_count(count, bound);
    if ((uint64_t)blockIdx.x * G >= n) return;
    reas_group<U, false, NT>(R, pkts, stride, lens, n, now, G, blockIdx.x, L);
}

// reas_classify_kernel with the count read on the device; the grid is cdiv(bound, kBlock),
// and info / fin are the work view of the bound.
__global__ __launch_bounds__(kBlock) void reas_classify_dev_kernel(ReasDev R, const uint8_t *__restrict__ pkts,
                                                                   uint32_t stride, const uint32_t *__restrict__ lens,
                                                                   const uint32_t *__restrict__ count, uint32_t bound,
                                                                   uint64_t now, PktInfo *__restrict__ info,
                                                                   FinishRec *__restrict__ fin)
{
    const uint32_t n = dev_count(count, bound);
    if ((uint64_t)blockIdx.x * kBlock >= n) return;
    classify_wave_to_work(R, pkts, stride, lens, n, now, info, fin, blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6));
}

// reas_scatter_kernel with the count read on the device; the grid is cdiv(bound, G).  The
// visit order is xcd_runs over nb = cdiv(n, G) -- the groups there are, not the grid: the
// permutation is a bijection on [0, nb) only for the nb it is given, so with the grid's
// count it would send workgroups to groups past n and leave real ones unvisited.  Workgroups
// at or past nb leave before it is applied.
template <int U, bool NT, bool STAGE, int TB = kScatBlock>
__global__ __launch_bounds__(TB) void reas_scatter_dev_kernel(ReasDev R, const uint8_t *__restrict__ pkts,
                                                              uint32_t stride, const uint32_t *__restrict__ count,
                                                              uint32_t bound, uint32_t G,
                                                              const PktInfo *__restrict__ info,
                                                              const FinishRec *__restrict__ fin)
{
    __shared__ PktInfo sinfo[64];
    const uint32_t n = dev_count(count, bound);
    if ((uint64_t)blockIdx.x * G >= n) return;                        // blockIdx.x >= nb, without the division
    scatter_group<U, NT, STAGE, TB>(R, pkts, stride, n, G, info, fin, xcd_runs(blockIdx.x, (n + G - 1u) / G), sinfo);
}

}  // namespace e2sar_amd
