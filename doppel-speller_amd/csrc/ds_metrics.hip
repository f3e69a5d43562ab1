// AUC and weighted log loss of float32 margins that lie in HBM ("Metrics"): the kernels behind
// ds_auc_device / ds_weighted_logloss_device and behind the per-round metrics of ds_trainer_step and
// ds_trainer_batch_step (ds_metrics.h).
//
// AUC of the columns of a call, columns in blockIdx.y, no workgroup waits for another:
//   1. ds_metric_clear_kernel   the columns' counters and the OR / AND of their keys
//   2. ds_metric_key_kernel     keys[column][i] = cut_key(margin of the column's i-th negative row), i < n_neg, and the
//                               padding key 0xFFFFFFFF up to the common length n_keys; OR and AND of the negatives'
//                               keys, and the number of NaN ones (one atomic each per workgroup)
//   3. the radix sort of the cuts (ds_radix.h) over n_keys keys per column.  The padding sorts last whether its digits
//      count in the OR / AND or not (it starts at the tail, its digits are the largest, the scatter is stable), so it is
//      left out of them and passes are skipped as the negatives' own keys allow.  A NaN negative has the same key and
//      lies anywhere: it counts in the OR / AND.
//   4. ds_metric_search_kernel  one lane per positive row: lower and upper bound of its key among the column's sorted
//                               negatives -> concordant += lower, ties += upper - lower; a positive's key is below
//                               0xFFFFFFFF unless it is a NaN, which is counted instead.  Sums per wave by shuffles,
//                               per workgroup through LDS, then one 64-bit atomic per counter.
// The log loss is one pass over the column's rows (ds_metric_logloss_kernel) with the same reduction.
// Every sum is an integer sum and the sorted keys are a function of the keys alone: nothing depends on the schedule.

#include "ds_launch.h"
#include "ds_metrics.h"
#include "ds_options.h"
#include "ds_radix.h"

namespace ds {

constexpr int kMetricThreads = 256;
constexpr uint32_t kPaddingKey = 0xffffffffu;

__device__ inline uint32_t margin_key(const MetricColumn &column, int32_t row)
{
    return cut_key(__float_as_uint(column.base_margin + column.scores[row]));
}

__global__ __launch_bounds__(64) void ds_metric_clear_kernel(const int32_t *active, int32_t n_columns, uint32_t *col_or,
                                                              uint32_t *col_and, unsigned long long *counters)
{
    const int a = blockIdx.x * 64 + threadIdx.x;
    if (a >= n_columns) return;
    const int64_t m = active ? active[a] : a;
    col_or[a] = 0u;
    col_and[a] = 0xffffffffu;
    for (int i = 0; i < kMetricCounters; ++i) counters[m * kMetricCounters + i] = 0ull;
}

__global__ __launch_bounds__(kMetricThreads) void ds_metric_key_kernel(const MetricColumn *columns, const int32_t *active,
                                                                        int64_t n_keys, uint32_t *keys, uint32_t *col_or,
                                                                        uint32_t *col_and, unsigned long long *counters)
{
    __shared__ uint32_t s_or, s_and, s_nan;
    const int a = blockIdx.y, lane = threadIdx.x & 63;
    const int64_t m = active ? active[a] : a;
    const MetricColumn column = columns[m];
    if (threadIdx.x == 0) {
        s_or = 0u;
        s_and = 0xffffffffu;
        s_nan = 0u;
    }
    __syncthreads();
    uint32_t any = 0u, all = 0xffffffffu, nan = 0u;
    uint32_t *mine = keys + static_cast<int64_t>(a) * n_keys;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(kMetricThreads) + threadIdx.x; i < n_keys;
         i += static_cast<int64_t>(gridDim.x) * kMetricThreads) {
        uint32_t key = kPaddingKey;
        if (i < column.n_neg) {
            key = margin_key(column, column.neg_rows[i]);
            any |= key;
            all &= key;
            nan += key == kPaddingKey ? 1u : 0u;
        }
        mine[i] = key;
    }
    any = wave_or(any);
    all = wave_and(all);
    nan = wave_sum(nan);
    if (lane == 0) {
        atomicOr(&s_or, any);
        atomicAnd(&s_and, all);
        if (nan) atomicAdd(&s_nan, nan);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicOr(&col_or[a], s_or);
        atomicAnd(&col_and[a], s_and);
        if (s_nan) atomicAdd(&counters[m * kMetricCounters + 3], static_cast<unsigned long long>(s_nan));
    }
}

__global__ __launch_bounds__(kMetricThreads) void ds_metric_search_kernel(const MetricColumn *columns,
                                                                           const int32_t *active, int64_t n_keys,
                                                                           const uint32_t *keys_a, const uint32_t *keys_b,
                                                                           const uint32_t *col_or, const uint32_t *col_and,
                                                                           unsigned long long *counters)
{
    __shared__ unsigned long long s_sum[3];
    const int a = blockIdx.y, lane = threadIdx.x & 63;
    const int64_t m = active ? active[a] : a;
    const MetricColumn column = columns[m];
    const uint32_t *sorted = ((passes_done(col_or[a] ^ col_and[a], 4) & 1) ? keys_b : keys_a) +
                             static_cast<int64_t>(a) * n_keys;
    if (threadIdx.x < 3) s_sum[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long concordant = 0ull, ties = 0ull, nan = 0ull;
    for (int64_t j = blockIdx.x * static_cast<int64_t>(kMetricThreads) + threadIdx.x; j < column.n_pos;
         j += static_cast<int64_t>(gridDim.x) * kMetricThreads) {
        const uint32_t key = margin_key(column, column.pos_rows[j]);
        if (key == kPaddingKey) {
            ++nan;
            continue;
        }
        int32_t lo = 0, hi = column.n_neg;   // the number of negatives' keys below `key`
        while (lo < hi) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            if (sorted[mid] < key) lo = mid + 1; else hi = mid;
        }
        const int32_t below = lo;
        hi = column.n_neg;                   // ... and of those not above it
        while (lo < hi) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            if (sorted[mid] <= key) lo = mid + 1; else hi = mid;
        }
        concordant += static_cast<unsigned long long>(below);
        ties += static_cast<unsigned long long>(lo - below);
    }
    concordant = wave_sum(concordant);
    ties = wave_sum(ties);
    nan = wave_sum(nan);
    if (lane == 0) {
        if (concordant) atomicAdd(&s_sum[0], concordant);
        if (ties) atomicAdd(&s_sum[1], ties);
        if (nan) atomicAdd(&s_sum[2], nan);
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_sum[threadIdx.x]) atomicAdd(&counters[m * kMetricCounters + threadIdx.x], s_sum[threadIdx.x]);
}

__device__ inline void block_add(unsigned long long mine, unsigned long long *s_sum, unsigned long long *out)
{
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(s_sum, mine);
    __syncthreads();
    if (threadIdx.x == 0 && *s_sum) atomicAdd(out, *s_sum);
}

__global__ __launch_bounds__(kMetricThreads) void ds_metric_logloss_kernel(const MetricColumn *columns,
                                                                            const int32_t *active,
                                                                            unsigned long long *counters)
{
    __shared__ unsigned long long s_sum;
    const int a = blockIdx.y;
    const int64_t m = active ? active[a] : a;
    const MetricColumn column = columns[m];
    if (threadIdx.x == 0) s_sum = 0ull;
    __syncthreads();
    unsigned long long mine = 0ull;
    const int64_t rows = static_cast<int64_t>(column.n_neg) + column.n_pos;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(kMetricThreads) + threadIdx.x; i < rows;
         i += static_cast<int64_t>(gridDim.x) * kMetricThreads) {
        const bool positive = i >= column.n_neg;
        const int32_t row = positive ? column.pos_rows[i - column.n_neg] : column.neg_rows[i];
        mine += logloss_term(column.base_margin + column.scores[row], positive, column.beta);
    }
    block_add(mine, &s_sum, &counters[m * kMetricCounters + 4]);
}

// the same over the rows of one vector with its labels (ds_weighted_logloss_device)
__global__ __launch_bounds__(kMetricThreads) void ds_metric_logloss_rows_kernel(const float *margins, const float *labels,
                                                                                 int64_t n, double beta,
                                                                                 unsigned long long *out)
{
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0) s_sum = 0ull;
    __syncthreads();
    unsigned long long mine = 0ull;
    for (int64_t r = blockIdx.x * static_cast<int64_t>(kMetricThreads) + threadIdx.x; r < n;
         r += static_cast<int64_t>(gridDim.x) * kMetricThreads)
        mine += logloss_term(margins[r], labels[r] != 0.f, beta);
    block_add(mine, &s_sum, out);
}

// rows[0 .. counts[0]) = the rows with label 0, rows[n - counts[1] .. n) = the others, each in the order in which the
// waves arrive: the lists are sets, and every result is a sum over them.
__global__ __launch_bounds__(kMetricThreads) void ds_metric_split_kernel(const float *labels, int64_t n, int32_t *rows,
                                                                          uint32_t *counts)
{
    const int lane = threadIdx.x & 63;
    // whole waves enter the loop together: every lane of a wave takes part in its ballots
    const int64_t span = (n + 63) & ~int64_t(63);
    for (int64_t r = blockIdx.x * static_cast<int64_t>(kMetricThreads) + threadIdx.x; r < span;
         r += static_cast<int64_t>(gridDim.x) * kMetricThreads) {
        const bool valid = r < n;
        const bool negative = valid && labels[r] == 0.f;
        const unsigned long long negatives = __ballot(negative), positives = __ballot(valid && !negative);
        const unsigned long long lower = (1ull << lane) - 1ull;
        uint32_t first_neg = 0u, first_pos = 0u;
        if (lane == 0) {
            if (negatives) first_neg = atomicAdd(&counts[0], static_cast<uint32_t>(__popcll(negatives)));
            if (positives) first_pos = atomicAdd(&counts[1], static_cast<uint32_t>(__popcll(positives)));
        }
        first_neg = __shfl(first_neg, 0);
        first_pos = __shfl(first_pos, 0);
        if (negative) rows[first_neg + __popcll(negatives & lower)] = static_cast<int32_t>(r);
        else if (valid) rows[n - 1 - (first_pos + __popcll(positives & lower))] = static_cast<int32_t>(r);
    }
}

int64_t MetricScratch::bytes(int64_t keys, int32_t column_count)
{
    return (8 * keys + 1024 * radix_tiles(keys) + 8) * column_count;
}

int MetricScratch::allocate(int64_t keys, int32_t column_count)
{
    const size_t count = static_cast<size_t>(column_count);
    int status = keys_a.allocate(static_cast<size_t>(keys) * count);
    if (status == DS_OK) status = keys_b.allocate(static_cast<size_t>(keys) * count);
    if (status == DS_OK) status = table.allocate(static_cast<size_t>(256 * radix_tiles(keys)) * count);
    if (status == DS_OK) status = state.allocate(2 * count);
    n_keys = keys;
    columns = column_count;
    return status;
}

namespace {

Option g_metric_max_blocks{"max_blocks", 0, INT32_MAX, 0};   // 0: no cap
Option *const g_metrics_options[] = {&g_metric_max_blocks};

unsigned metric_grid(int64_t items, int compute_units, int64_t block_cap)
{
    const int64_t blocks = std::min<int64_t>((items + kMetricThreads - 1) / kMetricThreads, int64_t(compute_units) * 8);
    return grid_cap(blocks, g_metric_max_blocks.get(), block_cap);
}

}  // namespace

int metrics_enqueue(hipStream_t stream, int compute_units, uint32_t flags, const MetricColumn *d_columns,
                    const int32_t *d_active, int32_t n_columns, int64_t n_keys, int64_t max_pos, int64_t max_rows,
                    MetricScratch &scratch, unsigned long long *d_counters, int64_t block_cap)
{
    if (n_columns <= 0 || flags == 0) return DS_OK;
    if (!(flags & kMetricAuc)) n_keys = 0;   // nothing is sorted: the scratch may hold no key
    DS_REQUIRE(n_columns <= scratch.columns && n_keys >= 0 && n_keys <= scratch.n_keys,
               "metrics_enqueue: %d columns of %lld keys, scratch for %d of %lld", n_columns, (long long)n_keys,
               scratch.columns, (long long)scratch.n_keys);
    uint32_t *col_or = scratch.state.ptr, *col_and = col_or + scratch.columns;
    const unsigned columns = static_cast<unsigned>(n_columns);
    DS_LAUNCH(ds_metric_clear_kernel, dim3((columns + 63) / 64), dim3(64), 0, stream, d_active, n_columns, col_or,
              col_and, d_counters);
    if (flags & kMetricAuc) {
        if (n_keys > 0) {   // no negatives anywhere: nothing to sort, and the search reads no key
            DS_LAUNCH(ds_metric_key_kernel, dim3(metric_grid(n_keys, compute_units, block_cap), columns),
                      dim3(kMetricThreads), 0, stream, d_columns, d_active, n_keys, scratch.keys_a.ptr, col_or,
                      col_and, d_counters);
            DS_TRY(radix_sort_columns(stream, scratch.keys_a.ptr, scratch.keys_b.ptr, n_keys, n_columns, col_or,
                                      col_and, scratch.table.ptr));
        }
        DS_LAUNCH(ds_metric_search_kernel, dim3(metric_grid(max_pos, compute_units, block_cap), columns),
                  dim3(kMetricThreads), 0, stream, d_columns, d_active, n_keys, scratch.keys_a.ptr,
                  scratch.keys_b.ptr, col_or, col_and, d_counters);
    }
    if (flags & kMetricLogloss) {
        DS_LAUNCH(ds_metric_logloss_kernel, dim3(metric_grid(max_rows, compute_units, block_cap), columns),
                  dim3(kMetricThreads), 0, stream, d_columns, d_active, d_counters);
    }
    return DS_OK;
}

void metrics_row(uint32_t flags, const unsigned long long *counters, int64_t n_neg, int64_t n_pos, int64_t out[6])
{
    for (int i = 0; i < 6; ++i) out[i] = -1;
    if (flags & kMetricAuc) {
        out[0] = static_cast<int64_t>(counters[0]);
        out[1] = static_cast<int64_t>(counters[1]);
        out[2] = n_pos - static_cast<int64_t>(counters[2]);
        out[3] = n_neg - static_cast<int64_t>(counters[3]);
    }
    if (flags & kMetricLogloss) {
        out[4] = static_cast<int64_t>(counters[4]);
        out[5] = n_neg + n_pos;
    }
}

}  // namespace ds

namespace {

int device_of(const void *pointer, int *device)
{
    hipPointerAttribute_t attributes;
    if (hipPointerGetAttributes(&attributes, pointer) == hipSuccess) {
        *device = attributes.device;
        return DS_OK;
    }
    (void)hipGetLastError();
    DS_HIP(hipGetDevice(device));
    return DS_OK;
}

}  // namespace

static int auc_check_rows(const char *what, int64_t n)
{
    DS_REQUIRE(n >= 1 && n <= INT32_MAX, "%s: n = %lld rows out of range [1, 2^31)", what, (long long)n);
    return DS_OK;
}

// The body of both twins.  scores_at and labels_at name pointers into HBM that are read once `scratch` is allocated here:
// the caller's own arrays, or pieces that it has declared in `scratch`.
static int auc_run(const char *what, ds::Scratch &scratch, int device, const float *const *scores_at,
                   const float *const *labels_at, int64_t n, int64_t out[5], hipStream_t s)
{
    DS_HIP(hipSetDevice(device));
    const int units = ds::compute_units(device);
    int32_t *rows = nullptr;
    uint32_t *counts = nullptr;
    unsigned long long *counters = nullptr;
    ds::MetricColumn *columns = nullptr;
    scratch.add(&rows, static_cast<size_t>(n));
    scratch.add(&counts, 2);
    scratch.add(&counters, ds::kMetricCounters);
    scratch.add(&columns, 1);
    // the sort buffers follow once the negatives are counted: checked here for the worst case that every row is one
    DS_TRY(scratch.allocate(what, ds::MetricScratch::bytes(n, 1)));
    const float *d_scores = *scores_at, *d_labels = *labels_at;
    DS_HIP(hipMemsetAsync(counts, 0, sizeof(uint32_t) * 2, s));
    DS_LAUNCH(ds::ds_metric_split_kernel, dim3(ds::metric_grid(n, units, 0)), dim3(ds::kMetricThreads), 0, s,
              d_labels, n, rows, counts);
    uint32_t host_counts[2] = {0u, 0u};
    DS_HIP(hipMemcpyAsync(host_counts, counts, sizeof(host_counts), hipMemcpyDeviceToHost, s));
    DS_HIP(hipStreamSynchronize(s));   // the grids and the buffers of the sort depend on the number of negatives
    const int64_t n_neg = host_counts[0], n_pos = host_counts[1];
    if (n_neg + n_pos != n) {
        ds::set_error("%s: %lld + %lld rows listed of %lld", what, (long long)n_neg, (long long)n_pos, (long long)n);
        return DS_E_HIP;
    }
    ds::MetricScratch sort_buffers;
    DS_TRY(sort_buffers.allocate(n_neg, 1));
    const ds::MetricColumn column{d_scores, rows, rows + n_neg, static_cast<int32_t>(n_neg),
                                  static_cast<int32_t>(n_pos), 0.f, 0, 1.0};
    // the descriptor and the counters travel on `s` like the kernels between them; `column` and `host` are read and
    // written until that stream is synchronised, so every path below synchronises it before it returns
    unsigned long long host[ds::kMetricCounters];
    auto enqueue = [&]() -> int {
        DS_HIP(hipMemcpyAsync(columns, &column, sizeof(column), hipMemcpyHostToDevice, s));
        DS_TRY(ds::metrics_enqueue(s, units, ds::kMetricAuc, columns, nullptr, 1, n_neg, n_pos, n, sort_buffers, counters, 0));
        DS_HIP(hipMemcpyAsync(host, counters, sizeof(host), hipMemcpyDeviceToHost, s));
        return DS_OK;
    };
    const int status = enqueue();
    const hipError_t synced = hipStreamSynchronize(s);
    if (status != DS_OK) return status;
    DS_HIP(synced);
    int64_t row[6];
    ds::metrics_row(ds::kMetricAuc, host, n_neg, n_pos, row);
    for (int i = 0; i < 4; ++i) out[i] = row[i];
    out[4] = static_cast<int64_t>(host[2] + host[3]);
    return DS_OK;
}

extern "C" {

int ds_metrics_option(const char *name, int64_t value)
{
    return ds::set_option("ds_metrics_option", ds::g_metrics_options, name, value);
}

int ds_auc_device(const float *d_scores, const float *d_labels, int64_t n, int64_t out[5], void *stream)
{
    DS_REQUIRE(d_scores && d_labels && out, "ds_auc_device: null pointer");
    DS_TRY(auc_check_rows("ds_auc_device", n));
    int device = 0;
    DS_TRY(device_of(d_scores, &device));
    ds::Scratch scratch;
    return auc_run("ds_auc_device", scratch, device, &d_scores, &d_labels, n, out, static_cast<hipStream_t>(stream));
}

int ds_auc(const float *scores, const float *labels, int64_t n, int64_t out[5], int device)
{
    DS_REQUIRE(scores && labels && out, "ds_auc: null pointer");
    DS_TRY(auc_check_rows("ds_auc", n));
    ds::Scratch scratch;
    const float *d_scores = nullptr, *d_labels = nullptr;
    scratch.stage(&d_scores, scores, static_cast<size_t>(n));
    scratch.stage(&d_labels, labels, static_cast<size_t>(n));
    return auc_run("ds_auc", scratch, device, &d_scores, &d_labels, n, out, nullptr);
}

int ds_weighted_logloss_device(const float *d_margins, const float *d_labels, int64_t n, double beta, int64_t out[2],
                               void *stream)
{
    DS_REQUIRE(d_margins && d_labels && out, "ds_weighted_logloss_device: null pointer");
    DS_REQUIRE(n >= 1 && n <= INT32_MAX, "ds_weighted_logloss_device: n = %lld rows out of range [1, 2^31)", (long long)n);
    DS_REQUIRE(beta > 0 && beta < 1e30, "ds_weighted_logloss_device: beta = %g must be positive", beta);
    int device = 0;
    DS_TRY(device_of(d_margins, &device));
    DS_HIP(hipSetDevice(device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    ds::DeviceBuffer<unsigned long long> sum;
    DS_TRY(sum.allocate(1));
    DS_HIP(hipMemsetAsync(sum.ptr, 0, sum.bytes(), s));
    DS_LAUNCH(ds::ds_metric_logloss_rows_kernel, dim3(ds::metric_grid(n, ds::compute_units(device), 0)),
              dim3(ds::kMetricThreads), 0, s, d_margins, d_labels, n, beta, sum.ptr);
    unsigned long long host = 0ull;
    DS_HIP(hipMemcpyAsync(&host, sum.ptr, sizeof(host), hipMemcpyDeviceToHost, s));
    DS_HIP(hipStreamSynchronize(s));
    out[0] = static_cast<int64_t>(host);
    out[1] = n;
    return DS_OK;
}

}  // extern "C"
