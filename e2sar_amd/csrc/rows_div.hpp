// rows_div.hpp -- bufferOffset / fragBytes of the rows family's seen calls (e2sar_hip_rows_reassemble_seen): plain
// C++ for the host and the device alike, so that the host's multiplier and the kernel's division are pinned by a
// host program over edge values (tests/test_rows_seen_cpu.py).
#pragma once

#include <cstdint>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define E2SAR_ROWS_DIV_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define E2SAR_ROWS_DIV_FN inline
#endif

namespace e2sar_amd {

// The host's multiplier for n / d: M = floor((2^64 - 1) / d), d > 0.
E2SAR_ROWS_DIV_FN uint64_t rows_div_magic(uint32_t d) { return ~0ull / d; }

// Quotient and remainder of n / d, exact for every 32-bit n and every d in [1, 2^32): M >= (2^64 - d) / d, so
// n * M / 2^64 lies in (n / d - 1, n / d] -- the product's high half is the quotient or one below it, and the
// remainder, below 2 d, says which.  One 64-bit high multiply and a compare: no division sequence.
struct RowsQuot {
    uint32_t q, r;
};
E2SAR_ROWS_DIV_FN RowsQuot rows_div(uint32_t n, uint32_t d, uint64_t M)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint64_t q = __umul64hi((uint64_t)n, M);
#else
    uint64_t q = (uint64_t)(((unsigned __int128)n * M) >> 64);
#endif
    uint64_t r = (uint64_t)n - q * d;
    if (r >= d) {
        q++;
        r -= d;
    }
    return RowsQuot{(uint32_t)q, (uint32_t)r};
}

}  // namespace e2sar_amd
