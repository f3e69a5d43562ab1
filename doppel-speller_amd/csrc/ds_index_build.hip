// The truth index built on the device: ds_index_create_device uploads the caller's CSR and derives in HBM, byte for
// byte, every array that ds_index_create (ds_runtime.hip, build_index_image: the specification) derives on the host.
// Also ds_index_read (any array of any index back to the host) and ds_index_build_option.
//
// Every write position is a function of the input alone: the orders come from stable LSD radix sorts (8-bit digits,
// ranks inside a wave from __ballot, across the waves through LDS: ds_wave.h) and exclusive scans; no position is
// handed out by an atomic.  The only atomics are an atomicMin of the lowest bad column and an atomicOr of a flag.
//
// Stages (M = nnz postings, N rows, V columns, T tiles, stride = T + 1):
//   check      every posting strictly ascending within [0, N) in its column; a bad list ends the build before any
//              other kernel reads truth_idx (the column of a posting: binary search in rowptr)
//   row order  keys (order key of sums32 << 32 | row), sorted by bits 32..63 (skipped with DS_SORT_ROWS=0)
//              -> original row, position of a row, sums32 in internal order, record words 4 and 6
//   forward    keys (internal row << 32 | column) in the caller's column-major order, stable sort by the row bits
//              -> row_cols, row_start (row boundaries of the sorted keys)
//   lists      the same keys with their halves swapped, stable sort by the column bits -> every column's list in
//              internal rows, ascending (rowptr does not change)
//   rows       per row, over its forward columns in ascending order: signature words, float64 idf total
//              (literal_only), the two 64-bit hashes of the duplicate ranks
//   pointers   first posting of every (column, tile) cell by binary search in the column's list; E = exclusive scan
//              of "row is even" over the postings; quads per cell; exclusive scan (64-bit) -> col_ptr
//   postings   posting p of cell c goes to its part's start + its rank inside the part (from E); one thread per
//              cell writes the padding
//   tiles      tile_sums_min / tile_sums_max with the host's first-of-equals rule (-0.0 / +0.0) and its NaN rule
//   ranks      rows sorted by (hash a, hash b, sums32 bits), ties by ascending row: a run is a hash group, its last
//              row the group's largest; every other member is compared column by column with that row; rank = 1 +
//              verified members behind it in the run (exclusive scan of the verified flags), saturating at 65535
#include <algorithm>
#include <cstdlib>
#include <memory>

#include "ds_launch.h"
#include "ds_options.h"
#include "ds_wave.h"

namespace ds {
namespace {

constexpr int kBuildThreads = 256;
constexpr int kBuildTile = 2048;   // items of one workgroup in a sort pass or a scan
constexpr unsigned long long kNoBadColumn = ~0ull;

// bits of both row hashes the device build keeps (tests: collisions); 0: all 64
Option g_duplicate_hash_bits{"duplicate_hash_bits", 0, 64, 64, true};
Option *const g_index_build_options[] = {&g_duplicate_hash_bits};

inline unsigned blocks_for(int64_t n) { return static_cast<unsigned>((n + kBuildThreads - 1) / kBuildThreads); }
inline int64_t build_tiles(int64_t n) { return (n + kBuildTile - 1) / kBuildTile; }

// The column whose posting list holds posting p: the last g with rowptr[g] <= p (rowptr is monotone, p < rowptr[V]).
__device__ inline int64_t column_of(const int64_t *rowptr, int64_t V, int64_t p)
{
    int64_t low = 0, high = V;   // rowptr[low] <= p < rowptr[high]
    while (high - low > 1) {
        const int64_t middle = (low + high) >> 1;
        if (rowptr[middle] <= p) low = middle; else high = middle;
    }
    return low;
}

__global__ __launch_bounds__(kBuildThreads) void ds_build_check_kernel(const int64_t *rowptr, const int32_t *truth_idx,
                                                                        int64_t V, int64_t N, int64_t nnz,
                                                                        unsigned long long *bad_column)
{
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kBuildThreads + threadIdx.x;
    if (p >= nnz) return;
    const int64_t g = column_of(rowptr, V, p);
    const int64_t row = truth_idx[p], previous = p > rowptr[g] ? truth_idx[p - 1] : -1;
    if (!(row > previous && row < N)) atomicMin(bad_column, static_cast<unsigned long long>(g));
}

// ---- exclusive scan of up to 2^32 uint32 values, summed in 64 bits ---------------------------------------------------
// value i = in[i], or "the row of keys[i] is even" when keys is given; 0 from n_in on.  out may be in.
__device__ inline unsigned long long scan_load(const uint32_t *in, const uint64_t *keys, int64_t i, int64_t n_in)
{
    if (i >= n_in) return 0ull;
    return keys ? (~keys[i] & 1ull) : in[i];
}

__global__ __launch_bounds__(kBuildThreads) void ds_build_scan_reduce_kernel(const uint32_t *in, const uint64_t *keys,
                                                                              int64_t n_in, unsigned long long *spine)
{
    __shared__ unsigned long long s_waves[kBuildThreads / 64];
    const int64_t begin = static_cast<int64_t>(blockIdx.x) * kBuildTile;
    unsigned long long mine = 0ull, total;
    for (int j = 0; j < kBuildTile / kBuildThreads; ++j) mine += scan_load(in, keys, begin + j * kBuildThreads + threadIdx.x, n_in);
    (void)block_exclusive<kBuildThreads>(mine, s_waves, total);
    if (threadIdx.x == 0) spine[blockIdx.x] = total;
}

// spine[0 .. blocks) -> its exclusive prefix, spine[blocks] = the total
__global__ __launch_bounds__(kBuildThreads) void ds_build_scan_spine_kernel(unsigned long long *spine, int64_t blocks)
{
    __shared__ unsigned long long s_waves[kBuildThreads / 64];
    unsigned long long running = 0ull;
    for (int64_t base = 0; base < blocks; base += kBuildThreads) {
        const int64_t i = base + threadIdx.x;
        const unsigned long long value = i < blocks ? spine[i] : 0ull;
        unsigned long long total;
        const unsigned long long before = block_exclusive<kBuildThreads>(value, s_waves, total);
        if (i < blocks) spine[i] = running + before;
        running += total;
    }
    if (threadIdx.x == 0) spine[blocks] = running;
}

__global__ __launch_bounds__(kBuildThreads) void ds_build_scan_apply_kernel(const uint32_t *in, const uint64_t *keys,
                                                                             int64_t n_in, uint32_t *out, int64_t n_out,
                                                                             const unsigned long long *spine)
{
    __shared__ unsigned long long s_waves[kBuildThreads / 64];
    const int64_t begin = static_cast<int64_t>(blockIdx.x) * kBuildTile;
    unsigned long long running = spine[blockIdx.x];
    for (int j = 0; j < kBuildTile / kBuildThreads; ++j) {
        const int64_t i = begin + j * kBuildThreads + threadIdx.x;
        const unsigned long long value = scan_load(in, keys, i, n_in);
        unsigned long long total;
        const unsigned long long before = block_exclusive<kBuildThreads>(value, s_waves, total);
        if (i < n_out) out[i] = static_cast<uint32_t>(running + before);
        running += total;
    }
}

// ---- stable LSD radix sort of 64-bit items, keys only -----------------------------------------------------------------
// The digit of an item: bits [shift, shift + 8) of the item itself, or of field[low half of the item] when a field is
// given (the duplicate ranks sort row numbers by their hashes).
__device__ inline uint32_t build_digit(uint64_t item, const uint64_t *field, int32_t shift)
{
    const uint64_t value = field ? field[item & 0xffffffffull] : item;
    return static_cast<uint32_t>(value >> shift) & 0xffu;
}

__global__ __launch_bounds__(kBuildThreads) void ds_build_sort_count_kernel(const uint64_t *src, int64_t n,
                                                                             const uint64_t *field, int32_t shift,
                                                                             uint32_t *table, int64_t tiles)
{
    __shared__ uint32_t s_hist[256];
    const int64_t begin = static_cast<int64_t>(blockIdx.x) * kBuildTile, end = min(n, begin + kBuildTile);
    radix_count_tile<kBuildThreads>(src, begin, end, [=](uint64_t item) { return build_digit(item, field, shift); }, s_hist);
    table[static_cast<int64_t>(threadIdx.x) * tiles + blockIdx.x] = s_hist[threadIdx.x];
}

__global__ __launch_bounds__(kBuildThreads) void ds_build_sort_scatter_kernel(const uint64_t *src, uint64_t *dst, int64_t n,
                                                                               const uint64_t *field, int32_t shift,
                                                                               const uint32_t *table, int64_t tiles)
{
    __shared__ uint32_t s_next[256];                          // the next position of each digit for this workgroup
    __shared__ uint32_t s_wave_count[kBuildThreads / 64][256];  // items of each digit in each wave of the current 256
    s_next[threadIdx.x] = table[static_cast<int64_t>(threadIdx.x) * tiles + blockIdx.x];
    const int64_t begin = static_cast<int64_t>(blockIdx.x) * kBuildTile, end = min(n, begin + kBuildTile);
    radix_scatter_tile<kBuildThreads>(src, dst, begin, end, n, [=](uint64_t item) { return build_digit(item, field, shift); },
                                      s_next, s_wave_count);
}

// ---- row order -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBuildThreads) void ds_build_row_keys_kernel(const float *sums32, int64_t N, int32_t sort_rows,
                                                                           uint64_t *keys)
{
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kBuildThreads + threadIdx.x;
    if (t >= N) return;
    const uint32_t bits = __float_as_uint(sums32[t]);
    const uint32_t key = bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);   // ds_index_create's key: no case for -0.0 or NaN
    keys[t] = (static_cast<uint64_t>(sort_rows ? key : 0u) << 32) | static_cast<uint64_t>(t);
}

__global__ __launch_bounds__(kBuildThreads) void ds_build_rows_kernel(const uint64_t *keys, const float *sums32, int64_t N,
                                                                       int32_t *position, float *sums_internal,
                                                                       uint32_t *records)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBuildThreads + threadIdx.x;
    if (i >= N) return;
    const uint32_t original = static_cast<uint32_t>(keys[i]);
    const float sums = sums32[original];
    position[original] = static_cast<int32_t>(i);
    sums_internal[i] = sums;
    records[i * kRowRecordWords + 4] = __float_as_uint(sums);
    records[i * kRowRecordWords + 6] = original;
}

// ---- forward index and permuted lists --------------------------------------------------------------------------------
__global__ __launch_bounds__(kBuildThreads) void ds_build_forward_keys_kernel(const int64_t *rowptr, const int32_t *truth_idx,
                                                                               const int32_t *position, int64_t V,
                                                                               int64_t nnz, uint64_t *keys)
{
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kBuildThreads + threadIdx.x;
    if (p >= nnz) return;
    const uint64_t g = static_cast<uint64_t>(column_of(rowptr, V, p));
    keys[p] = (static_cast<uint64_t>(static_cast<uint32_t>(position[truth_idx[p]])) << 32) | g;
}

// sorted (row << 32 | column) -> row_cols, row_start (written at the row boundaries: every entry once), and the keys
// with their halves swapped for the sort by column
__global__ __launch_bounds__(kBuildThreads) void ds_build_forward_kernel(const uint64_t *sorted, int64_t nnz, int64_t N,
                                                                          int32_t wide_cols, void *row_cols,
                                                                          uint32_t *row_start, uint64_t *swapped)
{
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kBuildThreads + threadIdx.x;
    if (p >= nnz) return;
    const uint64_t key = sorted[p];
    const int64_t row = static_cast<int64_t>(key >> 32);
    const uint32_t g = static_cast<uint32_t>(key);
    if (wide_cols) static_cast<int32_t *>(row_cols)[p] = static_cast<int32_t>(g);
    else static_cast<uint16_t *>(row_cols)[p] = static_cast<uint16_t>(g);
    swapped[p] = (static_cast<uint64_t>(g) << 32) | static_cast<uint64_t>(row);
    const int64_t previous = p > 0 ? static_cast<int64_t>(sorted[p - 1] >> 32) : -1;
    for (int64_t r = previous + 1; r <= row && r <= N; ++r) row_start[r] = static_cast<uint32_t>(p);
    if (p == nnz - 1)
        for (int64_t r = row + 1; r <= N; ++r) row_start[r] = static_cast<uint32_t>(nnz);
}

__device__ inline uint32_t forward_column(const void *row_cols, int32_t wide_cols, uint32_t p)
{
    return wide_cols ? static_cast<uint32_t>(static_cast<const int32_t *>(row_cols)[p])
                     : static_cast<uint32_t>(static_cast<const uint16_t *>(row_cols)[p]);
}

// One thread per internal row, over its columns in ascending order: signature words 0..3 of the record, the float64
// idf total of the literal_only test (the host's row_total: sequential adds in ascending column order), the hashes.
__global__ __launch_bounds__(kBuildThreads) void ds_build_row_walk_kernel(const uint32_t *row_start, const void *row_cols,
                                                                           int32_t wide_cols, const float *idf32,
                                                                           const int8_t *sig_column, const float *sums_internal,
                                                                           int64_t N, uint64_t hash_mask, uint32_t *records,
                                                                           uint64_t *hash_a, uint64_t *hash_b,
                                                                           uint64_t *hash_bits, uint64_t *items,
                                                                           uint32_t *literal_only)
{
    const int64_t t = static_cast<int64_t>(blockIdx.x) * kBuildThreads + threadIdx.x;
    if (t >= N) return;
    uint32_t words[kSignatureWords] = {0u, 0u, 0u, 0u};
    double total = 0.0;
    uint64_t a = 0ull, b = 0ull;
    for (uint32_t p = row_start[t]; p < row_start[t + 1]; ++p) {
        const uint32_t g = forward_column(row_cols, wide_cols, p);
        total += static_cast<double>(idf32[g]);
        const int bit = sig_column[g];
#pragma unroll
        for (int w = 0; w < kSignatureWords; ++w) words[w] |= (bit >= 0 && (bit >> 5) == w) ? 1u << (bit & 31) : 0u;
        a += mix64(static_cast<uint64_t>(g) + 0x9e3779b97f4a7c15ull);
        b += mix64(static_cast<uint64_t>(g) * 0xd6e8feb86659fd93ull + 0x2545f4914f6cdd1dull);
    }
#pragma unroll
    for (int w = 0; w < kSignatureWords; ++w) records[t * kRowRecordWords + w] = words[w];
    const float sums = sums_internal[t];
    if (!(sums >= 0.f && sums < 1e30f) || static_cast<double>(sums) < total * (1.0 - 1e-4)) atomicOr(literal_only, 1u);
    hash_a[t] = a & hash_mask;
    hash_b[t] = b & hash_mask;
    hash_bits[t] = __float_as_uint(sums);
    items[t] = static_cast<uint64_t>(t);
}

// ---- list pointers and postings --------------------------------------------------------------------------------------
// cell (g, b): the first posting of column g with an internal row >= b * tile_rows; (g, n_tiles): the column's end
__global__ __launch_bounds__(kBuildThreads) void ds_build_cells_kernel(const int64_t *rowptr, const uint64_t *lists,
                                                                        int64_t cells, int64_t stride, int64_t tile_rows,
                                                                        uint32_t *cell_begin)
{
    const int64_t c = static_cast<int64_t>(blockIdx.x) * kBuildThreads + threadIdx.x;
    if (c >= cells) return;
    const int64_t g = c / stride, b = c - g * stride;
    int64_t low = rowptr[g], high = rowptr[g + 1];
    if (b == stride - 1) low = high;
    const uint64_t first_row = static_cast<uint64_t>(b * tile_rows);
    while (low < high) {   // lower bound of first_row among the rows of the list
        const int64_t middle = (low + high) >> 1;
        if ((lists[middle] & 0xffffffffull) < first_row) low = middle + 1; else high = middle;
    }
    cell_begin[c] = static_cast<uint32_t>(low);
}

// quads of every cell: ceil(even / 4) + ceil(odd / 4); 0 for the end entry of a column
__global__ __launch_bounds__(kBuildThreads) void ds_build_quads_kernel(const uint32_t *cell_begin, const uint32_t *even_before,
                                                                        int64_t cells, int64_t stride, uint32_t *col_ptr)
{
    const int64_t c = static_cast<int64_t>(blockIdx.x) * kBuildThreads + threadIdx.x;
    if (c >= cells) return;
    uint32_t quads = 0u;
    if (c % stride != stride - 1) {
        const uint32_t begin = cell_begin[c], end = cell_begin[c + 1];
        const uint32_t even = even_before[end] - even_before[begin], odd = (end - begin) - even;
        quads = (even + 3u) / 4u + (odd + 3u) / 4u;
    }
    col_ptr[c] = quads;
}

__global__ __launch_bounds__(kBuildThreads) void ds_build_fill_kernel(const uint64_t *lists, const uint32_t *cell_begin,
                                                                       const uint32_t *even_before, const uint32_t *col_ptr,
                                                                       const uint32_t *records, int64_t nnz, int64_t stride,
                                                                       int64_t tile_rows, uint64_t n_postings,
                                                                       uint16_t *postings, uint16_t *posting_sums)
{
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kBuildThreads + threadIdx.x;
    if (p >= nnz) return;
    const uint64_t key = lists[p];
    const int64_t g = static_cast<int64_t>(key >> 32), t = static_cast<int64_t>(key & 0xffffffffull);
    const int64_t b = t / tile_rows, c = g * stride + b;
    const uint32_t local = static_cast<uint32_t>(t - b * tile_rows), parity = local & 1u;
    const uint32_t begin = cell_begin[c], end = cell_begin[c + 1];
    const uint32_t even_here = even_before[static_cast<uint32_t>(p)] - even_before[begin];
    const uint32_t even_all = even_before[end] - even_before[begin];
    const uint64_t base = static_cast<uint64_t>(col_ptr[c]);
    const uint64_t at = parity ? (base + (even_all + 3u) / 4u) * 4u + (static_cast<uint32_t>(p) - begin - even_here)
                               : base * 4u + even_here;
    if (at >= n_postings) return;   // never true for pointers made from the same counts
    postings[at] = static_cast<uint16_t>((parity << 15) | (local >> 1));
    posting_sums[at] = static_cast<uint16_t>(records[t * kRowRecordWords] & 0xffffu);
}

__global__ __launch_bounds__(kBuildThreads) void ds_build_pad_kernel(const uint32_t *cell_begin, const uint32_t *even_before,
                                                                      const uint32_t *col_ptr, int64_t cells, int64_t stride,
                                                                      uint32_t pad_word, uint64_t n_postings,
                                                                      uint16_t *postings, uint16_t *posting_sums)
{
    const int64_t c = static_cast<int64_t>(blockIdx.x) * kBuildThreads + threadIdx.x;
    if (c >= cells || c % stride == stride - 1) return;
    const uint32_t begin = cell_begin[c], end = cell_begin[c + 1];
    const uint32_t even = even_before[end] - even_before[begin], odd = (end - begin) - even;
    const uint64_t part_begin[2] = {static_cast<uint64_t>(col_ptr[c]) * 4u,
                                    (static_cast<uint64_t>(col_ptr[c]) + (even + 3u) / 4u) * 4u};
    const uint32_t held[2] = {even, odd};
    for (uint32_t part = 0; part < 2; ++part)
        for (uint32_t i = held[part]; i < ((held[part] + 3u) & ~3u); ++i) {
            const uint64_t at = part_begin[part] + i;
            if (at >= n_postings) continue;
            postings[at] = static_cast<uint16_t>((part << 15) | pad_word);
            posting_sums[at] = static_cast<uint16_t>(0);
        }
}

// ---- tile bounds -----------------------------------------------------------------------------------------------------
// The host's loop keeps the first of equal values (std::min / std::max replace on a strict comparison only: -0.0 and +0.0)
// and never leaves a NaN it starts from, nor takes one later.  The same here: candidates are (value, row), the lower
// row wins among equal values, NaNs lose every comparison, and a tile whose first row is a NaN reports that NaN.
__global__ __launch_bounds__(kBuildThreads) void ds_build_tile_bounds_kernel(const float *sums_internal, int64_t N,
                                                                              int64_t tile_rows, float *tile_min,
                                                                              float *tile_max)
{
    __shared__ float s_low[kBuildThreads], s_high[kBuildThreads];
    __shared__ int64_t s_low_at[kBuildThreads], s_high_at[kBuildThreads];
    const int64_t first = static_cast<int64_t>(blockIdx.x) * tile_rows, last = min(N, first + tile_rows);
    float low = __uint_as_float(0x7f800000u), high = __uint_as_float(0xff800000u);
    int64_t low_at = INT64_MAX, high_at = INT64_MAX;
    for (int64_t t = first + threadIdx.x; t < last; t += kBuildThreads) {
        const float value = sums_internal[t];
        if (value < low || (value == low && t < low_at)) { low = value; low_at = t; }
        if (value > high || (value == high && t < high_at)) { high = value; high_at = t; }
    }
    s_low[threadIdx.x] = low; s_low_at[threadIdx.x] = low_at;
    s_high[threadIdx.x] = high; s_high_at[threadIdx.x] = high_at;
    __syncthreads();
    for (int half = kBuildThreads / 2; half > 0; half >>= 1) {
        if (threadIdx.x < half) {
            const float other_low = s_low[threadIdx.x + half], other_high = s_high[threadIdx.x + half];
            const int64_t other_low_at = s_low_at[threadIdx.x + half], other_high_at = s_high_at[threadIdx.x + half];
            if (other_low < s_low[threadIdx.x] || (other_low == s_low[threadIdx.x] && other_low_at < s_low_at[threadIdx.x])) {
                s_low[threadIdx.x] = other_low; s_low_at[threadIdx.x] = other_low_at;
            }
            if (other_high > s_high[threadIdx.x] || (other_high == s_high[threadIdx.x] && other_high_at < s_high_at[threadIdx.x])) {
                s_high[threadIdx.x] = other_high; s_high_at[threadIdx.x] = other_high_at;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float start = sums_internal[first];
        const bool nan_start = start != start;
        tile_min[blockIdx.x] = nan_start ? start : s_low[0];
        tile_max[blockIdx.x] = nan_start ? start : s_high[0];
    }
}

// ---- duplicate ranks -------------------------------------------------------------------------------------------------
// items: the rows sorted by (hash a, hash b, sums32 bits, row).  head[i] = 1 where a run (a hash group) begins.
__global__ __launch_bounds__(kBuildThreads) void ds_build_heads_kernel(const uint64_t *items, const uint64_t *hash_a,
                                                                        const uint64_t *hash_b, const uint64_t *hash_bits,
                                                                        int64_t N, uint32_t *head)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBuildThreads + threadIdx.x;
    if (i >= N) return;
    uint32_t begins = 1u;
    if (i > 0) {
        const uint64_t t = items[i], u = items[i - 1];
        begins = !(hash_a[t] == hash_a[u] && hash_b[t] == hash_b[u] && hash_bits[t] == hash_bits[u]);
    }
    head[i] = begins;
}

// run_end[group] = the last position of the group's run (group = heads before position i, plus head[i], minus 1)
__global__ __launch_bounds__(kBuildThreads) void ds_build_run_ends_kernel(const uint32_t *head, const uint32_t *heads_before,
                                                                           int64_t N, uint32_t *run_end)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBuildThreads + threadIdx.x;
    if (i >= N) return;
    if (i == N - 1 || head[i + 1]) run_end[heads_before[i] + head[i] - 1u] = static_cast<uint32_t>(i);
}

// verified[i] = 1 when the row at position i is not its group's largest row and its column list equals that row's
__global__ __launch_bounds__(kBuildThreads) void ds_build_verify_kernel(const uint64_t *items, const uint32_t *head,
                                                                         const uint32_t *heads_before, const uint32_t *run_end,
                                                                         const uint32_t *row_start, const void *row_cols,
                                                                         int32_t wide_cols, int64_t N, uint32_t *verified)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBuildThreads + threadIdx.x;
    if (i >= N) return;
    const uint32_t end = run_end[heads_before[i] + head[i] - 1u];
    uint32_t same = 0u;
    if (end != i) {
        const uint64_t t = items[i], first = items[end];
        const uint32_t mine = row_start[t], theirs = row_start[first], length = row_start[t + 1] - mine;
        same = length == row_start[first + 1] - theirs;
        for (uint32_t j = 0; same && j < length; ++j)
            same = forward_column(row_cols, wide_cols, mine + j) == forward_column(row_cols, wide_cols, theirs + j);
    }
    verified[i] = same;
}

// rank = the group's largest row + the verified members between this row and it, saturating; word 5 of the record
__global__ __launch_bounds__(kBuildThreads) void ds_build_ranks_kernel(const uint64_t *items, const uint32_t *head,
                                                                        const uint32_t *heads_before, const uint32_t *run_end,
                                                                        const uint32_t *verified, const uint32_t *verified_before,
                                                                        int64_t N, uint32_t *records)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBuildThreads + threadIdx.x;
    if (i >= N) return;
    uint32_t rank = 0u;
    if (verified[i]) {
        const uint32_t end = run_end[heads_before[i] + head[i] - 1u];
        rank = min(1u + verified_before[end] - verified_before[i + 1], 0xffffu);
    }
    records[items[i] * kRowRecordWords + 5] = rank;
}

// ---- launch sequences ------------------------------------------------------------------------------------------------
struct BuildScratch {
    DeviceBuffer<uint64_t> keys_a, keys_b;         // [max(nnz, N)] sort buffers
    DeviceBuffer<uint32_t> table;                  // [256][tiles] digit counts of a sort pass
    DeviceBuffer<unsigned long long> spine;        // block sums of a scan
};

int exclusive_scan(BuildScratch &scratch, const uint32_t *in, const uint64_t *keys, int64_t n_in, uint32_t *out, int64_t n_out)
{
    const int64_t blocks = build_tiles(n_out);
    DS_LAUNCH(ds_build_scan_reduce_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBuildThreads), 0, 0, in, keys, n_in,
              scratch.spine.ptr);
    DS_LAUNCH(ds_build_scan_spine_kernel, dim3(1), dim3(kBuildThreads), 0, 0, scratch.spine.ptr, blocks);
    DS_LAUNCH(ds_build_scan_apply_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBuildThreads), 0, 0, in, keys, n_in, out,
              n_out, scratch.spine.ptr);
    return DS_OK;
}

// Stable sort of the n items in `from` by bits [low, high) of their digit source; `from` names the result afterwards.
int sort_bits(BuildScratch &scratch, uint64_t *&from, uint64_t *&to, int64_t n, const uint64_t *field, int low, int high)
{
    const int64_t tiles = build_tiles(n);
    for (int shift = low; shift < high; shift += 8) {
        DS_LAUNCH(ds_build_sort_count_kernel, dim3(static_cast<unsigned>(tiles)), dim3(kBuildThreads), 0, 0, from, n, field,
                  shift, scratch.table.ptr, tiles);
        DS_TRY(exclusive_scan(scratch, scratch.table.ptr, nullptr, 256 * tiles, scratch.table.ptr, 256 * tiles));
        DS_LAUNCH(ds_build_sort_scatter_kernel, dim3(static_cast<unsigned>(tiles)), dim3(kBuildThreads), 0, 0, from, to, n,
                  field, shift, scratch.table.ptr, tiles);
        std::swap(from, to);
    }
    return DS_OK;
}

int bits_of(int64_t count)   // bits that hold every value below count
{
    int bits = 1;
    while (bits < 63 && (int64_t(1) << bits) < count) ++bits;
    return bits;
}

struct IndexDeleter {
    void operator()(ds_index *index) const { ds_index_destroy(index); }
};

}  // namespace
}  // namespace ds

extern "C" {

int ds_index_build_option(const char *name, int64_t value)
{
    return ds::set_option("ds_index_build_option", ds::g_index_build_options, name, value);
}

int ds_index_create_device(const int64_t *rowptr, const int32_t *truth_idx, const float *idf32, const float *sums32,
                           int64_t V, int64_t N, int device, ds_index **out)
{
    using namespace ds;
    DS_REQUIRE(out != nullptr, "ds_index_create: out is null");
    *out = nullptr;
    // ---- the host's checks, with its messages -------------------------------------------------------------------------
    const int64_t tile_rows = N > 0 ? choose_tile_rows(N) : 0;
    DS_REQUIRE(rowptr && idf32 && sums32, "ds_index_create: null input");
    DS_REQUIRE(V > 0 && N > 0, "ds_index_create: V and N must be positive (V=%lld N=%lld)", (long long)V, (long long)N);
    DS_REQUIRE(N < (int64_t(1) << 31) - kWideTileRows, "ds_index_create: N too large for int32 row indexes");
    DS_REQUIRE(tile_rows > 0 && tile_rows % 2 == 0 && tile_rows / 2 < 0x8000, "ds_index_create: bad tile size");
    DS_REQUIRE(rowptr[0] == 0, "ds_index_create: rowptr[0] must be 0");
    const int64_t nnz = rowptr[V];
    DS_REQUIRE(nnz >= 0 && (nnz == 0 || truth_idx), "ds_index_create: bad nnz / truth_idx");
    const int64_t n_tiles = (N + tile_rows - 1) / tile_rows, stride = n_tiles + 1, cells = V * stride;
    DS_REQUIRE(cells < (int64_t(1) << 40), "ds_index_create: list pointer table too large");
    for (int64_t g = 0; g < V; ++g)
        DS_REQUIRE(rowptr[g + 1] >= rowptr[g], "ds_index_create: rowptr not monotone at column %lld", (long long)g);
    DS_REQUIRE(nnz < (int64_t(1) << 32) - 1,
               "ds_index_create_device: %lld postings need 64-bit row starts, which only ds_index_create builds", (long long)nnz);
    const char *sort_switch = getenv("DS_SORT_ROWS");
    const bool sort_rows = sort_switch == nullptr || atoi(sort_switch) != 0;
    const bool wide_cols = V > 65536;

    // signature columns and the idf range test, from rowptr and idf32 alone: as the host build
    std::vector<int8_t> sig_column(static_cast<size_t>(V), static_cast<int8_t>(-1));
    {
        std::vector<int64_t> by_length(static_cast<size_t>(V));
        for (int64_t g = 0; g < V; ++g) by_length[static_cast<size_t>(g)] = g;
        const size_t top = static_cast<size_t>(std::min<int64_t>(V, kSignatureBits));
        std::partial_sort(by_length.begin(), by_length.begin() + top, by_length.end(), [&](int64_t x, int64_t y) {
            const int64_t lx = rowptr[x + 1] - rowptr[x], ly = rowptr[y + 1] - rowptr[y];
            return lx != ly ? lx > ly : x < y;
        });
        for (size_t bit = 0; bit < top; ++bit) {
            const int64_t g = by_length[bit];
            if ((rowptr[g + 1] - rowptr[g]) * 256 < N) break;
            sig_column[static_cast<size_t>(g)] = static_cast<int8_t>(bit);
        }
    }
    bool literal_only = false;
    for (int64_t g = 0; g < V && !literal_only; ++g) literal_only = !(idf32[g] >= 0.f && idf32[g] < 1e30f);

    // ---- does it fit?  (the formula of the header comment, before anything is allocated or launched) -----------------
    DS_HIP(hipSetDevice(device));
    const int64_t items_max = std::max(nnz, N), sort_tiles = build_tiles(items_max);
    const int64_t scan_max = std::max<int64_t>(std::max(nnz + 1, 256 * sort_tiles), std::max(cells, N + 1));
    const int64_t scratch_bytes = 8 * (V + 1) + 4 * nnz + 4 * N           // rowptr, truth_idx, the caller's sums32
                                  + 16 * items_max + 1024 * sort_tiles     // sort buffers, digit table
                                  + 8 * (build_tiles(scan_max) + 1)        // scan spine
                                  + 4 * (nnz + 1) + 4 * cells              // even rows before a posting, cell starts
                                  + 4 * N + 24 * N + 16 * N + 4 * (N + 1) + 16;   // position; hashes; heads, run ends, flags and their scans
    const int64_t quads_max = nnz / 4 + 2 * std::min(nnz, V * n_tiles);
    const int64_t index_bytes = 4 * cells + 16 * quads_max + 5 * V + 4 * (N + 8) + 8 * n_tiles + 32 * N + 4 * (N + 1) +
                                (wide_cols ? 4 : 2) * nnz + 4 * kControlWords;
    DS_TRY(check_free(scratch_bytes + index_bytes, "ds_index_create_device: scratch and index together"));

    // ---- upload and check --------------------------------------------------------------------------------------------
    DeviceBuffer<int64_t> d_rowptr;
    DeviceBuffer<int32_t> d_idx, position;
    DeviceBuffer<float> d_sums;
    DeviceBuffer<unsigned long long> d_flags;   // [0] lowest bad column, [1] (low word) literal_only
    DS_TRY(d_rowptr.upload(rowptr, static_cast<size_t>(V + 1)));
    DS_TRY(d_idx.upload(truth_idx, static_cast<size_t>(nnz)));
    DS_TRY(d_sums.upload(sums32, static_cast<size_t>(N)));
    const unsigned long long flags_start[2] = {kNoBadColumn, 0ull};
    DS_TRY(d_flags.upload(flags_start, 2));
    if (nnz > 0) {
        DS_LAUNCH(ds_build_check_kernel, dim3(blocks_for(nnz)), dim3(kBuildThreads), 0, 0, d_rowptr.ptr, d_idx.ptr, V, N, nnz,
                  d_flags.ptr);
        unsigned long long bad_column = kNoBadColumn;
        DS_HIP(hipMemcpy(&bad_column, d_flags.ptr, sizeof(bad_column), hipMemcpyDeviceToHost));
        // nothing below runs on rows that have not passed this check
        DS_REQUIRE(bad_column == kNoBadColumn, "ds_index_create: posting list of column %lld is not strictly ascending within [0, N)",
                   (long long)bad_column);
    }

    std::unique_ptr<ds_index, IndexDeleter> index(new ds_index());
    index->device = device;
    index->compute_units = compute_units(device);
    index->n_truth = N;
    index->n_columns = V;
    index->nnz = nnz;
    index->n_tiles = n_tiles;
    index->tile_rows = static_cast<int>(tile_rows);
    index->rows_sorted = sort_rows;
    index->forward_wide_start = false;
    index->forward_wide_cols = wide_cols;
    DS_TRY(index->idf32.upload(idf32, static_cast<size_t>(V)));
    DS_TRY(index->sig_column.upload(sig_column.data(), sig_column.size()));
    DS_TRY(index->sums32.allocate(static_cast<size_t>(N) + 8));
    DS_HIP(hipMemset(index->sums32.ptr, 0, index->sums32.bytes()));
    DS_TRY(index->signature.allocate(static_cast<size_t>(N) * kRowRecordWords));
    DS_HIP(hipMemset(index->signature.ptr, 0, index->signature.bytes()));
    DS_TRY(index->row_start.allocate(static_cast<size_t>(N + 1) * 4));
    DS_HIP(hipMemset(index->row_start.ptr, 0, index->row_start.bytes()));
    // the host's size, which ds_index_info reports: the columns themselves, 4 bytes only when there is none
    DS_TRY(index->row_cols.allocate(nnz > 0 ? static_cast<size_t>(nnz) * (wide_cols ? 4 : 2) : 4));
    DS_TRY(index->col_ptr.allocate(static_cast<size_t>(cells)));
    DS_TRY(index->tile_sums_min.allocate(static_cast<size_t>(n_tiles)));
    DS_TRY(index->tile_sums_max.allocate(static_cast<size_t>(n_tiles)));

    BuildScratch scratch;
    DS_TRY(scratch.keys_a.allocate(static_cast<size_t>(items_max)));
    DS_TRY(scratch.keys_b.allocate(static_cast<size_t>(items_max)));
    DS_TRY(scratch.table.allocate(static_cast<size_t>(256 * sort_tiles)));
    DS_TRY(scratch.spine.allocate(static_cast<size_t>(build_tiles(scan_max) + 1)));
    DS_TRY(position.allocate(static_cast<size_t>(N)));
    uint64_t *from = scratch.keys_a.ptr, *to = scratch.keys_b.ptr;
    uint32_t *records = index->signature.ptr;
    uint32_t *row_start = reinterpret_cast<uint32_t *>(index->row_start.ptr);
    const dim3 threads(kBuildThreads);

    // ---- internal row order ------------------------------------------------------------------------------------------
    DS_LAUNCH(ds_build_row_keys_kernel, dim3(blocks_for(N)), threads, 0, 0, d_sums.ptr, N, sort_rows ? 1 : 0, from);
    if (sort_rows) DS_TRY(sort_bits(scratch, from, to, N, nullptr, 32, 64));
    DS_LAUNCH(ds_build_rows_kernel, dim3(blocks_for(N)), threads, 0, 0, from, d_sums.ptr, N, position.ptr, index->sums32.ptr,
              records);

    // ---- forward index, then every column's list in internal rows ----------------------------------------------------
    DeviceBuffer<uint32_t> cell_begin, even_before;
    DS_TRY(cell_begin.allocate(static_cast<size_t>(cells)));
    DS_TRY(even_before.allocate(static_cast<size_t>(nnz) + 1));
    if (nnz > 0) {
        DS_LAUNCH(ds_build_forward_keys_kernel, dim3(blocks_for(nnz)), threads, 0, 0, d_rowptr.ptr, d_idx.ptr, position.ptr, V,
                  nnz, from);
        DS_TRY(sort_bits(scratch, from, to, nnz, nullptr, 32, 32 + bits_of(N)));
        DS_LAUNCH(ds_build_forward_kernel, dim3(blocks_for(nnz)), threads, 0, 0, from, nnz, N, wide_cols ? 1 : 0,
                  static_cast<void *>(index->row_cols.ptr), row_start, to);
        std::swap(from, to);
        DS_TRY(sort_bits(scratch, from, to, nnz, nullptr, 32, 32 + bits_of(V)));
    }
    const uint64_t *lists = from;   // (column << 32 | internal row), ascending: the permuted CSR
    uint64_t *items = to;           // the other sort buffer: free from here on (N <= its size)

    // ---- signatures, idf totals, hashes ------------------------------------------------------------------------------
    DeviceBuffer<uint64_t> hash_a, hash_b, hash_bits, items_other;
    DS_TRY(hash_a.allocate(static_cast<size_t>(N)));
    DS_TRY(hash_b.allocate(static_cast<size_t>(N)));
    DS_TRY(hash_bits.allocate(static_cast<size_t>(N)));
    const int hash_bits_kept = static_cast<int>(g_duplicate_hash_bits.get());
    const uint64_t hash_mask = hash_bits_kept == 64 ? ~0ull : (1ull << hash_bits_kept) - 1ull;
    DS_LAUNCH(ds_build_row_walk_kernel, dim3(blocks_for(N)), threads, 0, 0, row_start,
              static_cast<const void *>(index->row_cols.ptr), wide_cols ? 1 : 0, index->idf32.ptr, index->sig_column.ptr,
              index->sums32.ptr, N, hash_mask, records, hash_a.ptr, hash_b.ptr, hash_bits.ptr, items,
              reinterpret_cast<uint32_t *>(d_flags.ptr + 1));

    // ---- list pointers -----------------------------------------------------------------------------------------------
    DS_LAUNCH(ds_build_cells_kernel, dim3(blocks_for(cells)), threads, 0, 0, d_rowptr.ptr, lists, cells, stride, tile_rows,
              cell_begin.ptr);
    DS_TRY(exclusive_scan(scratch, nullptr, lists, nnz, even_before.ptr, nnz + 1));
    DS_LAUNCH(ds_build_quads_kernel, dim3(blocks_for(cells)), threads, 0, 0, cell_begin.ptr, even_before.ptr, cells, stride,
              index->col_ptr.ptr);
    DS_TRY(exclusive_scan(scratch, index->col_ptr.ptr, nullptr, cells, index->col_ptr.ptr, cells));
    unsigned long long quads = 0ull;
    DS_HIP(hipMemcpy(&quads, scratch.spine.ptr + build_tiles(cells), sizeof(quads), hipMemcpyDeviceToHost));
    DS_REQUIRE(quads < 0xfffffff0ull, "ds_index_create: more than 2^32 posting quads");
    index->n_quads = static_cast<int64_t>(quads);

    // ---- postings ----------------------------------------------------------------------------------------------------
    const uint64_t n_postings = quads * 4u;
    DS_TRY(index->postings.allocate(std::max<size_t>(4, static_cast<size_t>(n_postings))));
    DS_TRY(index->posting_sums.allocate(std::max<size_t>(4, static_cast<size_t>(n_postings))));
    if (nnz > 0) {
        DS_LAUNCH(ds_build_fill_kernel, dim3(blocks_for(nnz)), threads, 0, 0, lists, cell_begin.ptr, even_before.ptr,
                  index->col_ptr.ptr, records, nnz, stride, tile_rows, n_postings, index->postings.ptr,
                  index->posting_sums.ptr);
        DS_LAUNCH(ds_build_pad_kernel, dim3(blocks_for(cells)), threads, 0, 0, cell_begin.ptr, even_before.ptr, index->col_ptr.ptr,
                  cells, stride, static_cast<uint32_t>(tile_rows / 2), n_postings, index->postings.ptr,
                  index->posting_sums.ptr);
    }

    // ---- tile bounds -------------------------------------------------------------------------------------------------
    DS_LAUNCH(ds_build_tile_bounds_kernel, dim3(static_cast<unsigned>(n_tiles)), threads, 0, 0, index->sums32.ptr, N, tile_rows,
              index->tile_sums_min.ptr, index->tile_sums_max.ptr);

    // ---- duplicate ranks ---------------------------------------------------------------------------------------------
    // the sort buffer that held the lists is needed no more once the postings are filled: the rows take both buffers
    DeviceBuffer<uint32_t> head, heads_before, run_end, verified, verified_before;
    DS_TRY(head.allocate(static_cast<size_t>(N)));
    DS_TRY(heads_before.allocate(static_cast<size_t>(N)));
    DS_TRY(run_end.allocate(static_cast<size_t>(N)));
    DS_TRY(verified.allocate(static_cast<size_t>(N)));
    DS_TRY(verified_before.allocate(static_cast<size_t>(N) + 1));
    {
        uint64_t *rows_from = items, *rows_to = const_cast<uint64_t *>(lists);
        DS_TRY(sort_bits(scratch, rows_from, rows_to, N, hash_bits.ptr, 0, 32));
        DS_TRY(sort_bits(scratch, rows_from, rows_to, N, hash_b.ptr, 0, hash_bits_kept));
        DS_TRY(sort_bits(scratch, rows_from, rows_to, N, hash_a.ptr, 0, hash_bits_kept));
        DS_LAUNCH(ds_build_heads_kernel, dim3(blocks_for(N)), threads, 0, 0, rows_from, hash_a.ptr, hash_b.ptr, hash_bits.ptr,
                  N, head.ptr);
        DS_TRY(exclusive_scan(scratch, head.ptr, nullptr, N, heads_before.ptr, N));
        DS_LAUNCH(ds_build_run_ends_kernel, dim3(blocks_for(N)), threads, 0, 0, head.ptr, heads_before.ptr, N, run_end.ptr);
        DS_LAUNCH(ds_build_verify_kernel, dim3(blocks_for(N)), threads, 0, 0, rows_from, head.ptr, heads_before.ptr, run_end.ptr,
                  row_start, static_cast<const void *>(index->row_cols.ptr), wide_cols ? 1 : 0, N, verified.ptr);
        DS_TRY(exclusive_scan(scratch, verified.ptr, nullptr, N, verified_before.ptr, N + 1));
        DS_LAUNCH(ds_build_ranks_kernel, dim3(blocks_for(N)), threads, 0, 0, rows_from, head.ptr, heads_before.ptr, run_end.ptr,
                  verified.ptr, verified_before.ptr, N, records);
    }

    // ---- what the host keeps: literal_only, sums_min (the host's loop over the tile minima) -----------------------------
    unsigned long long flags_end[2] = {0ull, 0ull};
    DS_HIP(hipMemcpy(flags_end, d_flags.ptr, sizeof(flags_end), hipMemcpyDeviceToHost));   // waits for every kernel above
    index->literal_only = literal_only || (flags_end[1] & 1ull) != 0;
    {
        std::vector<float> tile_min(static_cast<size_t>(n_tiles));
        float first_sums = 0.f;
        DS_HIP(hipMemcpy(tile_min.data(), index->tile_sums_min.ptr, sizeof(float) * tile_min.size(), hipMemcpyDeviceToHost));
        DS_HIP(hipMemcpy(&first_sums, index->sums32.ptr, sizeof(float), hipMemcpyDeviceToHost));
        float sums_min = first_sums;
        for (int64_t b = 0; b < n_tiles; ++b) sums_min = std::min(sums_min, tile_min[static_cast<size_t>(b)]);
        index->sums_min = sums_min;
    }
    DS_TRY(index->control.allocate(kControlWords));
    if (hipStreamCreate(&index->stream) != hipSuccess || hipEventCreate(&index->event_begin) != hipSuccess ||
        hipEventCreate(&index->event_fast) != hipSuccess || hipEventCreate(&index->event_dense) != hipSuccess) {
        set_error("ds_index_create_device: hipStreamCreate / hipEventCreate failed");
        return DS_E_HIP;
    }
    DS_HIP(hipDeviceSynchronize());
    *out = index.release();
    return DS_OK;
}

int ds_index_read(const ds_index *index, const char *name, void *dst, size_t capacity, size_t *bytes)
{
    DS_REQUIRE(index && name && bytes, "ds_index_read: null argument");
    *bytes = 0;
    const void *source = nullptr;
    size_t size = 0;
    int64_t scalars[8] = {0};
    const size_t start_width = index->forward_wide_start ? 8 : 4, cols_width = index->forward_wide_cols ? 4 : 2;
    if (std::strcmp(name, "col_ptr") == 0) { source = index->col_ptr.ptr; size = index->col_ptr.bytes(); }
    else if (std::strcmp(name, "postings") == 0) { source = index->postings.ptr; size = static_cast<size_t>(index->n_quads) * 8; }
    else if (std::strcmp(name, "posting_sums") == 0) { source = index->posting_sums.ptr; size = static_cast<size_t>(index->n_quads) * 8; }
    else if (std::strcmp(name, "records") == 0) { source = index->signature.ptr; size = index->signature.bytes(); }
    else if (std::strcmp(name, "sums32") == 0) { source = index->sums32.ptr; size = index->sums32.bytes(); }
    else if (std::strcmp(name, "tile_sums_min") == 0) { source = index->tile_sums_min.ptr; size = index->tile_sums_min.bytes(); }
    else if (std::strcmp(name, "tile_sums_max") == 0) { source = index->tile_sums_max.ptr; size = index->tile_sums_max.bytes(); }
    else if (std::strcmp(name, "sig_column") == 0) { source = index->sig_column.ptr; size = index->sig_column.bytes(); }
    else if (std::strcmp(name, "row_start") == 0) { source = index->row_start.ptr; size = static_cast<size_t>(index->n_truth + 1) * start_width; }
    else if (std::strcmp(name, "row_cols") == 0) { source = index->row_cols.ptr; size = static_cast<size_t>(index->nnz) * cols_width; }
    else if (std::strcmp(name, "idf32") == 0) { source = index->idf32.ptr; size = index->idf32.bytes(); }
    else if (std::strcmp(name, "scalars") == 0) {
        uint32_t sums_min_bits;
        std::memcpy(&sums_min_bits, &index->sums_min, sizeof(sums_min_bits));
        scalars[0] = index->n_tiles;
        scalars[1] = index->n_quads;
        scalars[2] = sums_min_bits;
        scalars[3] = index->literal_only ? 1 : 0;
        scalars[4] = index->rows_sorted ? 1 : 0;
        scalars[5] = static_cast<int64_t>(start_width);
        scalars[6] = static_cast<int64_t>(cols_width);
        scalars[7] = index->tile_rows;
        size = sizeof(scalars);
    } else {
        ds::set_error("ds_index_read: unknown array '%s'", name);
        return DS_E_ARG;
    }
    *bytes = size;
    DS_REQUIRE(dst != nullptr && capacity >= size, "ds_index_read: '%s' holds %zu bytes, the buffer %zu", name, size, capacity);
    if (source == nullptr) {
        std::memcpy(dst, scalars, size);
        return DS_OK;
    }
    DS_HIP(hipSetDevice(index->device));
    if (size) DS_HIP(hipMemcpy(dst, source, size, hipMemcpyDeviceToHost));
    return DS_OK;
}

}  // extern "C"
