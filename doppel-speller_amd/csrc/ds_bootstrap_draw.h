// The draw of the paired bootstraps, in one place: ds_bootstrap.hip resamples outcome codes with it and ds_sweep.hip the
// records of a threshold sweep, and because both take unit j(b, k) for draw k of replicate b, the counts of a sweep's cell
// are those of ds_bootstrap_counts on that cell's codes, bit for bit.
//
//   j(b, k) = umulhi64(x, n_units)   x = the first kept output of the stream of (seed, DS_BOOTSTRAP_PURPOSE_DRAW, (b << 32) | k)
//   j(n_boot, k) = k                 the baseline: every unit once
#pragma once

#include "ds_train.h"

namespace ds {

__device__ __forceinline__ int64_t bootstrap_unit(uint64_t seed, int32_t b, int32_t n_boot, int64_t k, int64_t n_units)
{
    if (b == n_boot) return k;
    const uint64_t x = sample_key(seed, DS_BOOTSTRAP_PURPOSE_DRAW, (static_cast<uint64_t>(b) << 32) | static_cast<uint64_t>(k));
    return static_cast<int64_t>(__umul64hi(x, static_cast<uint64_t>(n_units)));
}

}  // namespace ds
