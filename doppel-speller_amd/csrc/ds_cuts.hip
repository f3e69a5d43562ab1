// The cut values of the trainer's bins (train.py feature_cuts / compute_cuts, DESIGN.md section 9 "Cuts") from a
// float32[n][nf] matrix that already lies in HBM: ds_feature_cuts_device.  Bit-identical to compute_cuts.
//
// Every comparison is made on integer keys, never on floats, so denormals and infinities cannot depend on a float mode:
//   key(x) = 0xFFFFFFFF for a NaN (no other value maps there: NaNs sort last), else with -0.0 read as +0.0 the bits of
//   x with all bits flipped when the sign is set and only the sign bit flipped otherwise (ascending keys = ascending x).
// The key and the sort (phase 2) live in ds_radix.h, which the metrics (ds_metrics.hip) include as well.
//
// Per group of columns, one launch per phase, no workgroup waits for another:
//   1. ds_cuts_key_kernel      row tiles of 64 rows through LDS -> column-major keys[g][n]; per column the number m of
//                              non-NaN values and the OR and the AND of its keys (one atomic each per workgroup and column)
//   2. four passes of an LSD radix sort by 8-bit digits, keys only, columns in blockIdx.y:
//        ds_cuts_count_kernel    digit counts of a tile of kSortTile keys -> table[column][digit][tile]
//        ds_cuts_scan_kernel     exclusive scan of that table per column, in place
//        ds_cuts_scatter_kernel  stable scatter: rank inside a wave from __ballot over the digit's bits, across the
//                                waves of the workgroup through LDS, tiles of 256 keys in order
//      A pass whose digit is the same in every key of a column ((OR ^ AND) has a zero byte there) is skipped for that
//      column by all three kernels; the column's keys then stay in the buffer they are in.
//   3. ds_cuts_pick_kernel     on the sorted keys of a column: heads (key[i] != key[i - 1], i < m) counted and compacted
//                              in order; at most max_bin - 1 of them: the distinct values without the smallest, else the
//                              picks key[(j * m) / (max_bin - 1)], j = 1 .. max_bin - 2, without repeats and without
//                              values equal to key[0] -> table[nf][254] and a count per column; the host packs them.
// All sums are integer sums and every position is a function of the keys alone: the result does not depend on the
// schedule, on the run or on the column group.
//
// Memory: the two key buffers of a group take 8 B per row and column, its count table 1 KiB per tile and column.  The
// group is the largest number of columns for which these stay under a QUARTER of the HBM that is free at the call
// (at least one column); ds_cuts_option("column_group", g) forces g columns per group for tests.
#include <algorithm>

#include "ds_launch.h"
#include "ds_options.h"
#include "ds_radix.h"

namespace ds {

constexpr int kCutsFeaturesMax = 96;     // = kTrainFeaturesMax
constexpr int kCutsMax = 254;            // = kTrainCutsMax
constexpr int kKeyTileRows = 64;
constexpr int kKeyThreads = 256;

// ---- 1. keys ---------------------------------------------------------------------------------------------------------
// Wave w of a workgroup owns the columns w, w + 4, ... of the group, lane l row l of the tile: a column's keys of a
// tile are one coalesced 256-byte store, and its count, OR and AND in LDS belong to that wave alone.
__global__ __launch_bounds__(kKeyThreads) void ds_cuts_key_kernel(const uint32_t *rows, int64_t n, int32_t nf, int32_t c0,
                                                                   int32_t g, uint32_t *keys, uint32_t *col_m,
                                                                   uint32_t *col_or, uint32_t *col_and)
{
    __shared__ uint32_t s_tile[kKeyTileRows * (kCutsFeaturesMax + 1)];
    __shared__ uint32_t s_m[kCutsFeaturesMax], s_or[kCutsFeaturesMax], s_and[kCutsFeaturesMax];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int stride = nf | 1;   // odd: the 64 rows of a column fall on different banks
    for (int f = threadIdx.x; f < g; f += kKeyThreads) {
        s_m[f] = 0u;
        s_or[f] = 0u;
        s_and[f] = 0xffffffffu;
    }
    for (int64_t first = static_cast<int64_t>(blockIdx.x) * kKeyTileRows; first < n;
         first += static_cast<int64_t>(gridDim.x) * kKeyTileRows) {
        const int rows_here = static_cast<int>(n - first < kKeyTileRows ? n - first : kKeyTileRows);
        __syncthreads();
        for (int e = threadIdx.x; e < rows_here * nf; e += kKeyThreads) {   // coalesced row-major read
            const int r = e / nf;
            s_tile[r * stride + (e - r * nf)] = rows[first * nf + e];
        }
        __syncthreads();
        const bool valid = lane < rows_here;
        for (int f = wave; f < g; f += kKeyThreads / 64) {
            const uint32_t key = valid ? cut_key(s_tile[lane * stride + c0 + f]) : 0xffffffffu;
            if (valid) keys[static_cast<int64_t>(f) * n + first + lane] = key;
            const uint32_t any = wave_or(valid ? key : 0u), all = wave_and(key);
            const uint32_t present = __popcll(__ballot(key != 0xffffffffu));
            if (lane == 0) {
                s_m[f] += present;
                s_or[f] |= any;
                s_and[f] &= all;
            }
        }
    }
    __syncthreads();
    for (int f = threadIdx.x; f < g; f += kKeyThreads) {
        if (s_m[f]) atomicAdd(&col_m[f], s_m[f]);
        atomicOr(&col_or[f], s_or[f]);
        atomicAnd(&col_and[f], s_and[f]);
    }
}

// ---- 2. the radix sort: ds_radix.h ----------------------------------------------------------------------------------

// ---- 3. the cuts of a sorted column ----------------------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void ds_cuts_pick_kernel(const uint32_t *keys_a, const uint32_t *keys_b,
                                                                     int64_t n, const uint32_t *col_or,
                                                                     const uint32_t *col_and, const uint32_t *col_m,
                                                                     int32_t max_bin, uint32_t *cut_table,
                                                                     int32_t *cut_counts)
{
    __shared__ uint32_t s_waves[kScanThreads / 64];
    const int col = blockIdx.x;
    const uint32_t differing = col_or[col] ^ col_and[col];
    const uint32_t *sorted = ((passes_done(differing, 4) & 1) ? keys_b : keys_a) + static_cast<int64_t>(col) * n;
    uint32_t *out = cut_table + static_cast<int64_t>(col) * kCutsMax;
    const int64_t m = col_m[col];
    if (m == 0) {
        if (threadIdx.x == 0) cut_counts[col] = 0;
        return;
    }
    // heads in order: head number h >= 1 (from 0) is a candidate cut while h <= 254
    uint32_t heads = 0u;
    for (int64_t base = 0; base < m; base += kScanThreads) {
        const int64_t i = base + threadIdx.x;
        const bool valid = i < m;
        const uint32_t key = valid ? sorted[i] : 0u;
        const bool head = valid && (i == 0 || key != sorted[i - 1]);
        uint32_t total;
        const uint32_t number = heads + block_exclusive<kScanThreads>(head ? 1u : 0u, s_waves, total);
        if (head && number >= 1u && number <= static_cast<uint32_t>(kCutsMax)) out[number - 1] = cut_value_bits(key);
        heads += total;
    }
    if (heads <= static_cast<uint32_t>(max_bin - 1)) {
        if (threadIdx.x == 0) cut_counts[col] = static_cast<int32_t>(heads) - 1;
        return;
    }
    __syncthreads();   // the picks overwrite the heads
    const int64_t j = threadIdx.x + 1;
    bool take = false;
    uint32_t key = 0u;
    if (j <= max_bin - 2) {
        key = sorted[(j * m) / (max_bin - 1)];
        take = key != sorted[0] && key != sorted[((j - 1) * m) / (max_bin - 1)];
    }
    uint32_t total;
    const uint32_t at = block_exclusive<kScanThreads>(take ? 1u : 0u, s_waves, total);
    if (take) out[at] = cut_value_bits(key);
    if (threadIdx.x == 0) cut_counts[col] = static_cast<int32_t>(total);
}

}  // namespace ds

namespace {

ds::Option g_column_group{"column_group", 0, ds::kCutsFeaturesMax, 0};   // 0: sized from the free HBM
ds::Option *const g_cuts_options[] = {&g_column_group};

}  // namespace

extern "C" {

int ds_cuts_option(const char *name, int64_t value)
{
    return ds::set_option("ds_cuts_option", g_cuts_options, name, value);
}

int ds_feature_cuts_device(const float *d_features, int64_t n, int32_t n_features, int32_t max_bin, float *cuts,
                           int32_t *cut_offsets, int device, void *stream)
{
    DS_REQUIRE(d_features && cuts && cut_offsets, "ds_feature_cuts_device: null pointer");
    DS_REQUIRE(n >= 1 && n <= INT32_MAX, "ds_feature_cuts_device: n = %lld rows out of range [1, 2^31)", (long long)n);
    DS_REQUIRE(n_features >= 1 && n_features <= ds::kCutsFeaturesMax,
               "ds_feature_cuts_device: n_features = %d out of range [1, %d]", n_features, ds::kCutsFeaturesMax);
    DS_REQUIRE(max_bin >= 2 && max_bin <= 256, "ds_feature_cuts_device: max_bin = %d out of range [2, 256]", max_bin);
    DS_HIP(hipSetDevice(device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t tiles = (n + ds::kSortTile - 1) / ds::kSortTile;
    const int64_t column_bytes = 8 * n + 1024 * tiles;
    size_t free_bytes = 0;
    DS_TRY(ds::check_free(column_bytes, "ds_feature_cuts_device: one column", &free_bytes));
    int64_t group = g_column_group.get();
    if (group == 0) group = static_cast<int64_t>(free_bytes / 4) / column_bytes;
    group = std::max<int64_t>(1, std::min<int64_t>(group, n_features));

    ds::DeviceBuffer<uint32_t> keys_a, keys_b, table, column_state, cut_table;
    ds::DeviceBuffer<int32_t> cut_counts;
    DS_TRY(keys_a.allocate(static_cast<size_t>(group * n)));
    DS_TRY(keys_b.allocate(static_cast<size_t>(group * n)));
    DS_TRY(table.allocate(static_cast<size_t>(group * 256 * tiles)));
    DS_TRY(column_state.allocate(3 * ds::kCutsFeaturesMax)); // m, OR, AND of the group's columns
    DS_TRY(cut_table.allocate(static_cast<size_t>(n_features) * ds::kCutsMax));
    DS_TRY(cut_counts.allocate(n_features));
    uint32_t *col_m = column_state.ptr, *col_or = col_m + ds::kCutsFeaturesMax, *col_and = col_or + ds::kCutsFeaturesMax;
    const int64_t row_tiles = (n + ds::kKeyTileRows - 1) / ds::kKeyTileRows;
    const unsigned key_grid = ds::grid_cap(row_tiles, int64_t(ds::compute_units(device)) * 8);
    for (int32_t c0 = 0; c0 < n_features; c0 += static_cast<int32_t>(group)) {
        const int32_t g = static_cast<int32_t>(std::min<int64_t>(group, n_features - c0));
        DS_HIP(hipMemsetAsync(col_m, 0, sizeof(uint32_t) * 2 * ds::kCutsFeaturesMax, s));
        DS_HIP(hipMemsetAsync(col_and, 0xff, sizeof(uint32_t) * ds::kCutsFeaturesMax, s));
        DS_LAUNCH(ds::ds_cuts_key_kernel, dim3(key_grid), dim3(ds::kKeyThreads), 0, s,
                  reinterpret_cast<const uint32_t *>(d_features), n, n_features, c0, g, keys_a.ptr, col_m, col_or,
                  col_and);
        DS_TRY(ds::radix_sort_columns(s, keys_a.ptr, keys_b.ptr, n, g, col_or, col_and, table.ptr));
        DS_LAUNCH(ds::ds_cuts_pick_kernel, dim3(g), dim3(ds::kScanThreads), 0, s, keys_a.ptr, keys_b.ptr, n,
                  col_or, col_and, col_m, max_bin, cut_table.ptr + static_cast<size_t>(c0) * ds::kCutsMax,
                  cut_counts.ptr + c0);
    }
    std::vector<uint32_t> host_table(static_cast<size_t>(n_features) * ds::kCutsMax);
    std::vector<int32_t> host_counts(n_features);
    DS_HIP(hipMemcpyAsync(host_table.data(), cut_table.ptr, host_table.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    DS_HIP(hipMemcpyAsync(host_counts.data(), cut_counts.ptr, host_counts.size() * sizeof(int32_t), hipMemcpyDeviceToHost,
                          s));
    DS_HIP(hipStreamSynchronize(s));
    cut_offsets[0] = 0;
    for (int32_t f = 0; f < n_features; ++f) {
        const int32_t count = host_counts[f];
        if (count < 0 || count > ds::kCutsMax) {
            ds::set_error("ds_feature_cuts_device: feature %d came back with %d cuts", f, count);
            return DS_E_HIP;
        }
        std::memcpy(cuts + cut_offsets[f], host_table.data() + static_cast<size_t>(f) * ds::kCutsMax,
                    sizeof(uint32_t) * count);
        cut_offsets[f + 1] = cut_offsets[f] + count;
    }
    return DS_OK;
}

}  // extern "C"
