// The integer order of float32 values and the device radix sort on it, shared by the cuts (ds_cuts.hip) and the
// metrics (ds_metrics.hip).  One definition of the key, of the three kernels of a pass and of their launch sequence:
// both translation units include this header, each gets its own (static) instance of the same kernels.
//
// key(x) = 0xFFFFFFFF for a NaN (no other value maps there: NaNs sort last), else with -0.0 read as +0.0 the bits of x
// with all bits flipped when the sign is set and only the sign bit flipped otherwise (ascending keys = ascending x).
//
// The sort: four passes of an LSD radix sort by 8-bit digits, keys only, columns of n keys each in blockIdx.y, column
// c at keys + c * n:
//   ds_cuts_count_kernel    digit counts of a tile of kSortTile keys -> table[column][digit][tile]
//   ds_cuts_scan_kernel     exclusive scan of that table per column, in place
//   ds_cuts_scatter_kernel  stable scatter: rank inside a wave from __ballot over the digit's bits, across the waves
//                           of the workgroup through LDS, tiles of 256 keys in order
// A pass whose digit is the same in every key of a column ((OR ^ AND) of the column's keys has a zero byte there) is
// skipped for that column by all three kernels; the column's keys then stay in the buffer they are in.  After the four
// passes column c lies in keys_b when passes_done(col_or[c] ^ col_and[c], 4) is odd, else in keys_a.
// All sums are integer sums and every position is a function of the keys alone.  The tile bodies of the count and the
// scatter, and the workgroup scan, are those of ds_wave.h; the kernels here choose buffers, tile and digit.
#pragma once

#include <algorithm>

#include "ds_launch.h"
#include "ds_wave.h"

namespace ds {

constexpr int kSortThreads = 256;
constexpr int kSortWaves = kSortThreads / 64;
constexpr int kSortTile = 8192;          // keys of one column per workgroup and pass
constexpr int kScanThreads = 1024;

__device__ inline uint32_t cut_key(uint32_t bits)
{
    if ((bits & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;   // NaN
    if (bits == 0x80000000u) bits = 0u;                            // -0.0 counts as +0.0
    return (bits & 0x80000000u) ? ~bits : bits ^ 0x80000000u;
}

__device__ inline uint32_t cut_value_bits(uint32_t key) { return (key & 0x80000000u) ? key ^ 0x80000000u : ~key; }

// Is the digit of `pass` the same in every key of the column, and in which of the two buffers do the column's keys
// lie before that pass (1: the second one)?
__host__ __device__ inline bool pass_skipped(uint32_t differing, int pass)
{
    return ((differing >> (8 * pass)) & 0xffu) == 0u;
}
__host__ __device__ inline int passes_done(uint32_t differing, int pass)
{
    int done = 0;
    for (int p = 0; p < pass; ++p) done += pass_skipped(differing, p) ? 0 : 1;
    return done;
}

static __global__ __launch_bounds__(kSortThreads) void ds_cuts_count_kernel(const uint32_t *keys_a, const uint32_t *keys_b,
                                                                             int64_t n, int32_t pass,
                                                                             const uint32_t *col_or,
                                                                             const uint32_t *col_and, uint32_t *table,
                                                                             int64_t tiles)
{
    __shared__ uint32_t s_hist[256];
    const int col = blockIdx.y;
    const uint32_t differing = col_or[col] ^ col_and[col];
    if (pass_skipped(differing, pass)) return;
    const uint32_t *src = ((passes_done(differing, pass) & 1) ? keys_b : keys_a) + static_cast<int64_t>(col) * n;
    const int64_t begin = static_cast<int64_t>(blockIdx.x) * kSortTile, end = min(n, begin + kSortTile);
    radix_count_tile<kSortThreads>(src, begin, end, [pass](uint32_t key) { return (key >> (8 * pass)) & 0xffu; }, s_hist);
    table[(static_cast<int64_t>(col) * 256 + threadIdx.x) * tiles + blockIdx.x] = s_hist[threadIdx.x];
}

// table[column][digit][tile] -> the first position of (digit, tile) in the column's next buffer
static __global__ __launch_bounds__(kScanThreads) void ds_cuts_scan_kernel(uint32_t *table, int64_t tiles, int32_t pass,
                                                                            const uint32_t *col_or,
                                                                            const uint32_t *col_and)
{
    __shared__ uint32_t s_waves[kScanThreads / 64];
    const int col = blockIdx.x;
    if (pass_skipped(col_or[col] ^ col_and[col], pass)) return;
    uint32_t *mine = table + static_cast<int64_t>(col) * 256 * tiles;
    const int64_t count = 256 * tiles;
    uint32_t running = 0u;
    for (int64_t base = 0; base < count; base += kScanThreads) {
        const int64_t i = base + threadIdx.x;
        const uint32_t value = i < count ? mine[i] : 0u;
        uint32_t total;
        const uint32_t before = block_exclusive<kScanThreads>(value, s_waves, total);
        if (i < count) mine[i] = running + before;
        running += total;
    }
}

static __global__ __launch_bounds__(kSortThreads) void ds_cuts_scatter_kernel(uint32_t *keys_a, uint32_t *keys_b,
                                                                               int64_t n, int32_t pass,
                                                                               const uint32_t *col_or,
                                                                               const uint32_t *col_and,
                                                                               const uint32_t *table, int64_t tiles)
{
    __shared__ uint32_t s_next[256];                    // the next position of each digit for this workgroup
    __shared__ uint32_t s_wave_count[kSortWaves][256];  // keys of each digit in each wave of the current 256 keys
    const int col = blockIdx.y;
    const uint32_t differing = col_or[col] ^ col_and[col];
    if (pass_skipped(differing, pass)) return;
    const bool from_b = passes_done(differing, pass) & 1;
    const uint32_t *src = (from_b ? keys_b : keys_a) + static_cast<int64_t>(col) * n;
    uint32_t *dst = (from_b ? keys_a : keys_b) + static_cast<int64_t>(col) * n;
    s_next[threadIdx.x] = table[(static_cast<int64_t>(col) * 256 + threadIdx.x) * tiles + blockIdx.x];
    const int64_t begin = static_cast<int64_t>(blockIdx.x) * kSortTile, end = min(n, begin + kSortTile);
    radix_scatter_tile<kSortThreads>(src, dst, begin, end, n, [pass](uint32_t key) { return (key >> (8 * pass)) & 0xffu; },
                                     s_next, s_wave_count);
}

inline int64_t radix_tiles(int64_t n) { return (n + kSortTile - 1) / kSortTile; }

// The four passes for `columns` columns of n >= 1 keys each, enqueued on `stream`.  col_or / col_and hold the OR and
// the AND of every column's keys, table has 256 * radix_tiles(n) entries per column.
static inline int radix_sort_columns(hipStream_t stream, uint32_t *keys_a, uint32_t *keys_b, int64_t n, int32_t columns,
                                     const uint32_t *col_or, const uint32_t *col_and, uint32_t *table)
{
    const int64_t tiles = radix_tiles(n);
    for (int32_t pass = 0; pass < 4; ++pass) {
        DS_LAUNCH(ds_cuts_count_kernel, dim3(static_cast<unsigned>(tiles), columns), dim3(kSortThreads), 0,
                  stream, keys_a, keys_b, n, pass, col_or, col_and, table, tiles);
        DS_LAUNCH(ds_cuts_scan_kernel, dim3(columns), dim3(kScanThreads), 0, stream, table, tiles, pass, col_or,
                  col_and);
        DS_LAUNCH(ds_cuts_scatter_kernel, dim3(static_cast<unsigned>(tiles), columns), dim3(kSortThreads), 0,
                  stream, keys_a, keys_b, n, pass, col_or, col_and, table, tiles);
    }
    return DS_OK;
}

}  // namespace ds
