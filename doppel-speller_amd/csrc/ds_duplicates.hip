// Duplicate groups ("Duplicate groups"): the connected components of the truth set under the links
// the stages before this one score, when the truth table is its own query table.  The state is a union-find forest
// int32 parent[n_truth] in HBM that lives across the chunk loop: parent[i] <= i always, parent[i] == i marks a root.
//
// The link rule for query row q (absolute row a = q_first + q) and slot j with t = rows[q*k + j]:
//   skipped  t < 0, t >= n_truth or t == a: reason 0;
//   close    ratios[q*k + j] > levenshtein_threshold                               (bit 0 of the reason);
//   model    predictions != NULL and predictions[q*k + j] > probability_threshold  (bit 1; float32, a NaN is not above);
//   exact    exact != NULL, e = exact[q], 0 <= e < n_truth, e != a.
// A non-zero reason joins a and t, an exact link joins a and e.  counts[0] += exact links, counts[1] += close slots,
// counts[2] += slots with model and not close.
//
// union(a, b) is lock-free: find both roots with path halving, hook the LARGER root under the smaller with one
// atomicCAS(&parent[hi], hi, lo).  Why that is safe whatever the schedule and whatever a load returns of the values an
// entry has held in this launch (the L1 of a CU and the L2 of an XCD are not refreshed by other CUs' stores):
//   - every value parent[x] ever holds is a row of x's tree that is <= x, and < x once x is not a root: a walk goes
//     strictly down in row numbers, so it ends, and it never leaves the tree;
//   - a root stops being one exactly once, by a CAS that succeeded (the CAS runs at the memory side: one winner).  A
//     halving store only writes entries it has seen as non-roots, and "non-root" is for good: it never undoes a hook;
//   - a walk that ends at a stale root is caught by the CAS, which hands back the entry's real value: the union goes on
//     from there, strictly lower than before, so it ends too without waiting for anybody's store to arrive.
// Hooking high under low makes the root of a finished component its lowest row, whatever the order of the links, the
// chunking or the schedule: labels and sizes are a pure function of the inputs.
//
// One thread per slot, flat over the chunk's n_queries * k slots (coalesced reads of rows, ratios and predictions, a
// coalesced reason store); slot 0 of a query also carries its exact link.  The grid is capped and strides; a thread
// keeps its three counts in registers, a wave adds them up and lane 0 adds them to HBM once (integer atomics).
#include <algorithm>
#include <cmath>

#include "ds_launch.h"
#include "ds_options.h"
#include "ds_wave.h"

namespace ds {

constexpr int kDuplicateThreads = 256;
constexpr int kDuplicateMaxBlocks = 2048;     // 8 workgroups per CU on 256 CUs; more slots or rows: the grid strides
constexpr int kDuplicateBlocksLimit = 1 << 20;

static Option g_duplicate_max_blocks{"max_blocks", 0, kDuplicateBlocksLimit, kDuplicateMaxBlocks, true};
static Option *const g_duplicate_options[] = {&g_duplicate_max_blocks};

__device__ __forceinline__ int32_t parent_load(const int32_t *parent, int32_t x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void parent_store(int32_t *parent, int32_t x, int32_t value)
{
    __hip_atomic_store(parent + x, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x's tree as far as this thread can see it, halving the path on the way
__device__ __forceinline__ int32_t duplicate_find(int32_t *parent, int32_t x)
{
    for (;;) {
        const int32_t p = parent_load(parent, x);
        if (p >= x) return x;                     // p == x: a root (p > x never occurs; it ends the walk all the same)
        const int32_t g = parent_load(parent, p);
        if (g >= p) return p;
        parent_store(parent, x, g);               // x is not a root and g < p < x is a row of its tree
        x = g;
    }
}

__device__ __forceinline__ void duplicate_union(int32_t *parent, int32_t a, int32_t b)
{
    for (;;) {
        a = duplicate_find(parent, a);
        b = duplicate_find(parent, b);
        if (a == b) return;
        const int32_t hi = max(a, b), lo = min(a, b);
        const int32_t seen = atomicCAS(parent + hi, hi, lo);
        if (seen == hi) return;
        // hi was hooked by somebody else: `seen` (< hi) is its real parent.  a + b went down: the loop ends.
        a = seen;
        b = lo;
    }
}

__global__ __launch_bounds__(kDuplicateThreads) void ds_duplicate_begin_kernel(int32_t *__restrict__ parent, int32_t n_truth)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kDuplicateThreads + threadIdx.x; i < n_truth;
         i += static_cast<int64_t>(gridDim.x) * kDuplicateThreads)
        parent[i] = static_cast<int32_t>(i);
}

struct LinkArgs {
    const int32_t *rows;          // [n_queries][k]
    const uint8_t *ratios;        // [n_queries][k]
    const float *predictions;     // [n_queries][k] or NULL
    const int32_t *exact;         // [n_queries] or NULL
    int32_t *parent;              // [n_truth]
    uint8_t *reason;              // [n_queries][k] or NULL
    unsigned long long *counts;   // [3]
    int64_t q_first, n_slots;
    int32_t k, n_truth, levenshtein_threshold;
    float probability_threshold;
};

__global__ __launch_bounds__(kDuplicateThreads) void ds_duplicate_links_kernel(LinkArgs a)
{
    unsigned long long n_exact = 0, n_close = 0, n_model = 0;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kDuplicateThreads + threadIdx.x; i < a.n_slots;
         i += static_cast<int64_t>(gridDim.x) * kDuplicateThreads) {
        const int64_t q = i / a.k;
        const int32_t row = static_cast<int32_t>(a.q_first + q);        // < n_truth: checked by the entry point
        const int32_t t = a.rows[i];
        int reason = 0;
        if (t >= 0 && t < a.n_truth && t != row) {
            const bool close = static_cast<int32_t>(a.ratios[i]) > a.levenshtein_threshold;
            const bool model = a.predictions != nullptr && a.predictions[i] > a.probability_threshold;
            reason = (close ? 1 : 0) | (model ? 2 : 0);
            n_close += close ? 1 : 0;
            n_model += model && !close ? 1 : 0;
        }
        if (a.reason != nullptr) a.reason[i] = static_cast<uint8_t>(reason);
        if (reason != 0) duplicate_union(a.parent, row, t);
        if (a.exact != nullptr && i - q * a.k == 0) {
            const int32_t e = a.exact[q];
            if (e >= 0 && e < a.n_truth && e != row) {
                ++n_exact;
                duplicate_union(a.parent, row, e);
            }
        }
    }
    n_exact = wave_sum(n_exact);
    n_close = wave_sum(n_close);
    n_model = wave_sum(n_model);
    if ((threadIdx.x & 63) == 0) {
        if (n_exact) atomicAdd(a.counts + 0, n_exact);
        if (n_close) atomicAdd(a.counts + 1, n_close);
        if (n_model) atomicAdd(a.counts + 2, n_model);
    }
}

// label[i] = the root of i (nobody hooks during this launch: the roots are final, and any value an entry holds
// meanwhile is a row of the same tree), size[i] = 0 for the count that follows
__global__ __launch_bounds__(kDuplicateThreads) void ds_duplicate_label_kernel(int32_t *__restrict__ parent, int32_t n_truth,
                                                                              int32_t *__restrict__ label,
                                                                              int32_t *__restrict__ size)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kDuplicateThreads + threadIdx.x; i < n_truth;
         i += static_cast<int64_t>(gridDim.x) * kDuplicateThreads) {
        const int32_t x = static_cast<int32_t>(i);
        label[i] = duplicate_find(parent, x);
        size[i] = 0;
    }
}

// one count per row into its root, and the forest compressed for good: a halving store of the launch before may have
// been the last word on an entry
__global__ __launch_bounds__(kDuplicateThreads) void ds_duplicate_count_kernel(const int32_t *__restrict__ label, int32_t n_truth,
                                                                              int32_t *__restrict__ parent,
                                                                              int32_t *__restrict__ size)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kDuplicateThreads + threadIdx.x; i < n_truth;
         i += static_cast<int64_t>(gridDim.x) * kDuplicateThreads) {
        const int32_t root = label[i];
        parent[i] = root;
        atomicAdd(size + root, 1);
    }
}

// the roots hold their component's count and are not written here; the others read their root's
__global__ __launch_bounds__(kDuplicateThreads) void ds_duplicate_size_kernel(const int32_t *__restrict__ label, int32_t n_truth,
                                                                             int32_t *size)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kDuplicateThreads + threadIdx.x; i < n_truth;
         i += static_cast<int64_t>(gridDim.x) * kDuplicateThreads) {
        const int32_t root = label[i];
        if (root != i) size[i] = __hip_atomic_load(size + root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

static dim3 duplicate_grid(int64_t items)
{
    const int64_t blocks = (items + kDuplicateThreads - 1) / kDuplicateThreads;
    return dim3(grid_cap(blocks, g_duplicate_max_blocks.get()));
}

}  // namespace ds

extern "C" {

int ds_duplicates_option(const char *name, int64_t value)
{
    return ds::set_option("ds_duplicates_option", ds::g_duplicate_options, name, value);
}

int ds_duplicate_begin_device(int32_t *d_parent, int64_t n_truth, int64_t *d_counts, void *stream)
{
    DS_REQUIRE(n_truth >= 0 && n_truth <= INT32_MAX, "ds_duplicate_begin_device: n_truth = %lld out of range [0, 2^31)",
               (long long)n_truth);
    DS_REQUIRE(d_parent && d_counts, "ds_duplicate_begin_device: null pointer");
    hipStream_t queue = static_cast<hipStream_t>(stream);
    DS_HIP(hipMemsetAsync(d_counts, 0, 3 * sizeof(int64_t), queue));
    if (n_truth == 0) return DS_OK;
    DS_LAUNCH(ds::ds_duplicate_begin_kernel, ds::duplicate_grid(n_truth), dim3(ds::kDuplicateThreads), 0, queue,
              d_parent, static_cast<int32_t>(n_truth));
    return DS_OK;
}

int ds_duplicate_links_device(const int32_t *d_rows, const uint8_t *d_ratios, const float *d_predictions,
                              const int32_t *d_exact, int64_t q_first, int64_t n_queries, int32_t k, int64_t n_truth,
                              int32_t levenshtein_threshold, float probability_threshold, int32_t *d_parent,
                              uint8_t *d_reason, int64_t *d_counts, void *stream)
{
    DS_REQUIRE(n_queries >= 0 && q_first >= 0, "ds_duplicate_links_device: negative count");
    DS_REQUIRE(n_truth >= 0 && n_truth <= INT32_MAX, "ds_duplicate_links_device: n_truth = %lld out of range [0, 2^31)",
               (long long)n_truth);
    DS_REQUIRE(k >= 1, "ds_duplicate_links_device: k = %d, must be positive", k);
    DS_REQUIRE(levenshtein_threshold >= 0 && levenshtein_threshold <= 100,
               "ds_duplicate_links_device: Levenshtein threshold %d out of range [0, 100]", levenshtein_threshold);
    DS_REQUIRE(std::isfinite(probability_threshold), "ds_duplicate_links_device: the probability threshold is not finite");
    DS_REQUIRE(d_rows && d_ratios && d_parent && d_counts, "ds_duplicate_links_device: null pointer");
    DS_REQUIRE(n_queries <= INT64_MAX / k, "ds_duplicate_links_device: too many pairs");
    if (n_queries == 0 || n_truth == 0) return DS_OK;
    // the query rows are rows of the truth table itself: every one indexes `parent`
    DS_REQUIRE(q_first <= n_truth && n_queries <= n_truth - q_first,
               "ds_duplicate_links_device: rows [%lld, %lld) are not rows of the %lld truth titles", (long long)q_first,
               (long long)(q_first + n_queries), (long long)n_truth);
    ds::LinkArgs args{};
    args.rows = d_rows; args.ratios = d_ratios; args.predictions = d_predictions; args.exact = d_exact;
    args.parent = d_parent; args.reason = d_reason; args.counts = reinterpret_cast<unsigned long long *>(d_counts);
    args.q_first = q_first; args.n_slots = n_queries * k; args.k = k; args.n_truth = static_cast<int32_t>(n_truth);
    args.levenshtein_threshold = levenshtein_threshold; args.probability_threshold = probability_threshold;
    DS_LAUNCH(ds::ds_duplicate_links_kernel, ds::duplicate_grid(args.n_slots), dim3(ds::kDuplicateThreads), 0,
              static_cast<hipStream_t>(stream), args);
    return DS_OK;
}

int ds_duplicate_finish_device(int32_t *d_parent, int64_t n_truth, int32_t *d_label, int32_t *d_size, void *stream)
{
    DS_REQUIRE(n_truth >= 0 && n_truth <= INT32_MAX, "ds_duplicate_finish_device: n_truth = %lld out of range [0, 2^31)",
               (long long)n_truth);
    DS_REQUIRE(d_parent && d_label && d_size, "ds_duplicate_finish_device: null pointer");
    if (n_truth == 0) return DS_OK;
    hipStream_t queue = static_cast<hipStream_t>(stream);
    const dim3 grid = ds::duplicate_grid(n_truth), block(ds::kDuplicateThreads);
    const int32_t n = static_cast<int32_t>(n_truth);
    DS_LAUNCH(ds::ds_duplicate_label_kernel, grid, block, 0, queue, d_parent, n, d_label, d_size);
    DS_LAUNCH(ds::ds_duplicate_count_kernel, grid, block, 0, queue, d_label, n, d_parent, d_size);
    DS_LAUNCH(ds::ds_duplicate_size_kernel, grid, block, 0, queue, d_label, n, d_size);
    return DS_OK;
}

}  // extern "C"
