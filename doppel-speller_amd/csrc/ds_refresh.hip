// Refreshing a model ("Refreshing a model"): xgboost's process_type="update", updater="refresh".
// Every split of a forest stays; rows with labels go through the trees in order, and every leaf is re-estimated from
// the gradient sums it now receives.  No histogram and no split search.
//
// Per tree two launches on one stream, no host sync between trees:
//   rows  one thread per row, striding: add the tree before's new leaf (through leaf_of[r], the node the row reached
//         there) to the row's float32 leaf sum, take p, g and h at the new margin in registers (train_row_gradient,
//         the trainers' own), walk this tree on the RAW features (forest_walk), store leaf_of[r], add (g, h) to the
//         leaf's pair of a table of 64-bit integers in LDS; the workgroup flushes the pairs that are not zero with
//         64-bit integer global adds (the pattern of train_histogram_group).  A tree with more nodes than the table
//         holds adds straight to HBM.  Integer adds commute: the sums are the same for any grid, cap and schedule.
//   leaf  one thread per node of the tree writes train_leaf_value of a leaf whose hessian sum is above 0 into a WORKING
//         COPY of the forest's value array; the forest itself is never written.
// A last pass adds the last tree's leaves and writes the margins.  The rows of an evaluation set run the same row
// kernel without the sums and add train_row_error at every tree prefix to one counter per prefix.
// The rows are read where they lie, row-major: a walk touches one value per level, eight at the most, of a row of at
// most 384 bytes, so staging whole rows in LDS (forest_stage_rows) would move more than the walk reads and would take
// the LDS that the table of sums uses.
#include "ds_launch.h"
#include "ds_forest.h"
#include "ds_train.h"

#include <algorithm>
#include <cmath>

namespace ds {

struct RefreshArgs {
    const int4 *nodes;
    const float *values;          // the working copy: thresholds of the splits, the leaves as refreshed so far
    const float *rows;            // float32[n][nf], raw
    const float *labels;
    const float *weights;         // nullable
    int32_t *leaf_of;             // [n] the node row r reached in the tree before; written for this tree
    float *leafsum;               // [n]
    unsigned long long *sums;     // [n_nodes][2] in HBM
    float *trace;                 // nullable: this tree's [n] probabilities
    unsigned long long *error;    // evaluation rows: the counter of this tree prefix, null for none
    int64_t n, root;
    int32_t nf, lds_nodes;        // lds_nodes: the tree's node count when its sums go through LDS, 0 when straight to HBM
    int32_t previous, pad;        // 0 for the first tree: the leaf sums start at zero
    float base_margin;
    double beta;
};

template <bool kSums>
__global__ __launch_bounds__(kRowThreads) void ds_refresh_rows_kernel(RefreshArgs a)
{
    extern __shared__ unsigned long long s_sums[];   // kSums: [lds_nodes][2]
    __shared__ unsigned long long s_error;
    if (kSums) {
        for (int i = threadIdx.x; i < 2 * a.lds_nodes; i += kRowThreads) s_sums[i] = 0ull;
    } else if (threadIdx.x == 0) {
        s_error = 0ull;
    }
    __syncthreads();
    unsigned long long mine = 0;
    for (int64_t r = blockIdx.x * static_cast<int64_t>(kRowThreads) + threadIdx.x; r < a.n;
         r += static_cast<int64_t>(gridDim.x) * kRowThreads) {
        float sum = 0.f;
        if (a.previous) sum = a.leafsum[r] + a.values[a.leaf_of[r]];
        a.leafsum[r] = sum;
        const float margin = a.base_margin + sum;
        const int64_t node = forest_walk(a.nodes, a.values, a.root, a.rows + r * a.nf);
        a.leaf_of[r] = static_cast<int32_t>(node);
        if (kSums) {
            const float p = forest_probability(margin);
            if (a.trace != nullptr) a.trace[r] = p;
            long long qg, qh;
            train_row_gradient(p, a.labels[r], a.weights, r, a.beta, &qg, &qh);
            if ((qg | qh) == 0ll) continue;   // a row of weight 0 would add zeros
            if (a.lds_nodes > 0) {
                unsigned long long *slot = s_sums + 2 * (node - a.root);
                atomicAdd(slot, static_cast<unsigned long long>(qg));
                atomicAdd(slot + 1, static_cast<unsigned long long>(qh));
            } else {
                unsigned long long *slot = a.sums + 2 * node;
                atomicAdd(slot, static_cast<unsigned long long>(qg));
                atomicAdd(slot + 1, static_cast<unsigned long long>(qh));
            }
        } else if (a.error != nullptr) {
            mine += train_row_error(margin, a.labels[r]);
        }
    }
    if (kSums) {
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * a.lds_nodes; i += kRowThreads) {
            const unsigned long long value = s_sums[i];
            if (value != 0ull) atomicAdd(a.sums + 2 * a.root + i, value);
        }
    } else {
        if (mine) atomicAdd(&s_error, mine);
        __syncthreads();
        if (threadIdx.x == 0 && s_error) atomicAdd(a.error, s_error);
    }
}

// one thread per node of the tree at `root`: a leaf whose hessian sum is above 0 takes its new value
__global__ __launch_bounds__(64) void ds_refresh_leaf_kernel(const int4 *nodes, const unsigned long long *sums,
                                                              float *values, int64_t root, int32_t tree_nodes,
                                                              double reg_lambda, double eta)
{
    const int32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= tree_nodes) return;
    const int64_t node = root + i;
    if (nodes[node].x >= 0) return;
    const long long qg = static_cast<long long>(sums[2 * node]), qh = static_cast<long long>(sums[2 * node + 1]);
    if (qh > 0) values[node] = train_leaf_value(qg, qh, reg_lambda, eta);
}

// the last tree's leaves added, the margins written (nullable) and the error of the whole forest counted (nullable)
__global__ __launch_bounds__(kRowThreads) void ds_refresh_tail_kernel(const float *values, const int32_t *leaf_of,
                                                                       const float *leafsum, const float *labels,
                                                                       float *margins, unsigned long long *error,
                                                                       int64_t n, int32_t previous, float base_margin)
{
    __shared__ unsigned long long s_error;
    if (threadIdx.x == 0) s_error = 0ull;
    __syncthreads();
    unsigned long long mine = 0;
    for (int64_t r = blockIdx.x * static_cast<int64_t>(kRowThreads) + threadIdx.x; r < n;
         r += static_cast<int64_t>(gridDim.x) * kRowThreads) {
        float sum = 0.f;
        if (previous) sum = leafsum[r] + values[leaf_of[r]];
        const float margin = base_margin + sum;
        if (margins != nullptr) margins[r] = margin;
        if (error != nullptr) mine += train_row_error(margin, labels[r]);
    }
    if (mine) atomicAdd(&s_error, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_error) atomicAdd(error, s_error);
}

// the custom error of the forest as given: forest_leaf_sum of the raw rows where they lie
__global__ __launch_bounds__(kRowThreads) void ds_refresh_initial_kernel(ForestView forest, const float *rows,
                                                                          const float *labels, int64_t n,
                                                                          unsigned long long *error)
{
    __shared__ unsigned long long s_error;
    if (threadIdx.x == 0) s_error = 0ull;
    __syncthreads();
    unsigned long long mine = 0;
    for (int64_t r = blockIdx.x * static_cast<int64_t>(kRowThreads) + threadIdx.x; r < n;
         r += static_cast<int64_t>(gridDim.x) * kRowThreads)
        mine += train_row_error(forest.base_margin + forest_leaf_sum(forest, rows + r * forest.n_features), labels[r]);
    if (mine) atomicAdd(&s_error, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_error) atomicAdd(error, s_error);
}

namespace {

struct RefreshCall {
    const ds_forest *forest;
    const float *features, *labels, *weights, *eval_features, *eval_labels;
    int64_t n, n_eval;
    double eta, reg_lambda, beta;
    int refresh_leaf;
    float *leaf_out;
    int64_t *node_sums;
    float *margins;
    int64_t *eval_errors, *empty_leaves;
    float *trace;
};

// Everything both entries refuse, before any device work
int refresh_check(const char *who, const RefreshCall &c)
{
    DS_REQUIRE(c.forest != nullptr, "%s: forest is null", who);
    const ds_forest *forest = c.forest;
    DS_REQUIRE(forest->n_features >= 1 && forest->n_features <= kTrainFeaturesMax,
               "%s: the forest has n_features = %d, out of range [1, %d]", who, forest->n_features, kTrainFeaturesMax);
    DS_REQUIRE(c.n >= 0 && c.n <= INT32_MAX, "%s: n = %lld rows out of range [0, 2^31)", who, (long long)c.n);
    DS_REQUIRE(c.n_eval >= 0 && c.n_eval <= INT32_MAX, "%s: n_eval = %lld rows out of range [0, 2^31)", who,
               (long long)c.n_eval);
    DS_REQUIRE(c.n == 0 || (c.features != nullptr && c.labels != nullptr), "%s: features or labels is null", who);
    DS_REQUIRE((c.eval_features != nullptr) == (c.n_eval > 0) && (c.n_eval == 0 || c.eval_labels != nullptr),
               "%s: eval_features, eval_labels and n_eval = %lld do not go together", who, (long long)c.n_eval);
    DS_REQUIRE(c.leaf_out != nullptr && c.node_sums != nullptr && c.empty_leaves != nullptr,
               "%s: leaf_out, node_sums or empty_leaves is null", who);
    DS_REQUIRE(c.refresh_leaf == 0 || c.refresh_leaf == 1, "%s: refresh_leaf = %d is neither 0 nor 1", who,
               c.refresh_leaf);
    DS_REQUIRE(c.eta > 0 && c.eta < 1e30, "%s: eta = %g must be positive", who, c.eta);
    DS_REQUIRE(c.reg_lambda >= 0 && c.reg_lambda < 1e30, "%s: reg_lambda = %g must not be negative", who, c.reg_lambda);
    DS_REQUIRE(c.beta > 0 && c.beta < 1e30, "%s: beta = %g must be positive", who, c.beta);
    DS_TRY(train_check_labels(who, "labels: ", c.labels, c.n));
    DS_TRY(train_check_labels(who, "eval_labels: ", c.eval_labels, c.n_eval));
    if (c.weights != nullptr) {
        DS_TRY(train_check_weights(who, c.weights, c.n, c.beta));
    } else {
        DS_REQUIRE(std::max(c.beta, 1.0) * static_cast<double>(c.n) <= 4294967296.0,
                   "%s: max(beta, 1) * n = %g exceeds 2^32 (the integer sums could overflow)", who,
                   std::max(c.beta, 1.0) * static_cast<double>(c.n));
    }
    std::vector<int32_t> parent;
    return forest_parents(forest, who, parent);
}

// a matrix in HBM must lie on the forest's device
int refresh_check_device(const char *who, const ds_forest *forest, const float *d_rows, const char *what)
{
    if (d_rows == nullptr) return DS_OK;
    hipPointerAttribute_t attributes;
    if (hipPointerGetAttributes(&attributes, d_rows) != hipSuccess) {
        (void)hipGetLastError();   // not a pointer the runtime knows: nothing to compare
        return DS_OK;
    }
    DS_REQUIRE(attributes.type != hipMemoryTypeDevice || attributes.device == forest->device,
               "%s: the forest lives on device %d, %s on device %d", who, forest->device, what, attributes.device);
    return DS_OK;
}

// The launches and the read-back.  rows_at and eval_at name pointers into HBM, read once `scratch` is allocated here:
// the caller's own matrices, complete in `stream`'s order, or pieces that the caller has declared in `scratch`.
int refresh_run(const char *who, const RefreshCall &c, Scratch &scratch, const float *const *rows_at,
                const float *const *eval_at, hipStream_t stream)
{
    const ds_forest *forest = c.forest;
    const int64_t n = c.n, n_eval = c.n_eval, n_nodes = forest->n_nodes;
    const int32_t n_trees = forest->n_trees, nf = forest->n_features;
    DS_HIP(hipSetDevice(forest->device));
    const int units = compute_units(forest->device);
    float *values = nullptr, *leafsum = nullptr, *eval_leafsum = nullptr, *d_labels = nullptr, *d_eval_labels = nullptr,
          *d_weights = nullptr, *d_margins = nullptr, *d_trace = nullptr;
    int32_t *leaf_of = nullptr, *eval_leaf_of = nullptr;
    unsigned long long *sums = nullptr, *errors = nullptr;
    const size_t counters = static_cast<size_t>(n_trees) + 1, value_slots = static_cast<size_t>(std::max<int64_t>(n_nodes, 1));
    scratch.add(&values, value_slots);
    scratch.add(&sums, 2 * value_slots);
    scratch.add(&errors, counters);
    scratch.add(&leafsum, static_cast<size_t>(n));
    scratch.add(&leaf_of, static_cast<size_t>(n));
    scratch.stage(&d_labels, c.labels, static_cast<size_t>(n));
    if (c.weights) scratch.stage(&d_weights, c.weights, static_cast<size_t>(n));
    if (c.margins) scratch.add(&d_margins, static_cast<size_t>(n));
    if (c.trace) scratch.add(&d_trace, static_cast<size_t>(n) * n_trees);
    scratch.add(&eval_leafsum, static_cast<size_t>(n_eval));
    scratch.add(&eval_leaf_of, static_cast<size_t>(n_eval));
    scratch.stage(&d_eval_labels, c.eval_labels, static_cast<size_t>(n_eval));
    DS_TRY(scratch.allocate(who));
    const float *d_rows = *rows_at, *d_eval = *eval_at;
    if (n_nodes)
        DS_HIP(hipMemcpyAsync(values, forest->threshold.ptr, sizeof(float) * n_nodes, hipMemcpyDeviceToDevice, stream));
    DS_HIP(hipMemsetAsync(sums, 0, sizeof(unsigned long long) * 2 * value_slots, stream));
    DS_HIP(hipMemsetAsync(errors, 0, sizeof(unsigned long long) * counters, stream));

    const int64_t table = forest->refresh_lds_nodes.get();
    auto grid = [&](int64_t items) {   // the trainers' row grid and cap, and the forest's own cap
        return grid_cap(train_row_grid(units, items), forest->max_blocks.get());
    };
    if (n_eval > 0) {
        DS_LAUNCH(ds_refresh_initial_kernel, dim3(grid(n_eval)), dim3(kRowThreads), 0, stream, forest->view(),
                  d_eval, d_eval_labels, n_eval, errors);
    }
    for (int32_t t = 0; t < n_trees; ++t) {
        const int64_t root = forest->h_offsets[t], tree_nodes = forest->h_offsets[t + 1] - root;
        RefreshArgs args{};
        args.nodes = forest->nodes.ptr;
        args.values = values;
        args.sums = sums;
        args.root = root;
        args.nf = nf;
        args.previous = t > 0;
        args.base_margin = forest->base_margin;
        args.beta = c.beta;
        if (n > 0) {
            args.rows = d_rows;
            args.labels = d_labels;
            args.weights = c.weights ? d_weights : nullptr;
            args.leaf_of = leaf_of;
            args.leafsum = leafsum;
            args.trace = c.trace ? d_trace + static_cast<int64_t>(t) * n : nullptr;
            args.n = n;
            args.lds_nodes = tree_nodes <= table ? static_cast<int32_t>(tree_nodes) : 0;
            DS_LAUNCH(ds_refresh_rows_kernel<true>, dim3(grid(n)), dim3(kRowThreads),
                      sizeof(unsigned long long) * 2 * args.lds_nodes, stream, args);
            if (c.refresh_leaf) {
                DS_LAUNCH(ds_refresh_leaf_kernel, dim3(static_cast<unsigned>((tree_nodes + 63) / 64)), dim3(64), 0,
                          stream, forest->nodes.ptr, sums, values, root, static_cast<int32_t>(tree_nodes),
                          c.reg_lambda, c.eta);
            }
        }
        if (n_eval > 0) {
            args.rows = d_eval;
            args.labels = d_eval_labels;
            args.weights = nullptr;
            args.leaf_of = eval_leaf_of;
            args.leafsum = eval_leafsum;
            args.trace = nullptr;
            args.error = t > 0 ? errors + t : nullptr;
            args.n = n_eval;
            args.lds_nodes = 0;
            DS_LAUNCH(ds_refresh_rows_kernel<false>, dim3(grid(n_eval)), dim3(kRowThreads), 0, stream, args);
        }
    }
    if (n > 0 && c.margins != nullptr) {
        DS_LAUNCH(ds_refresh_tail_kernel, dim3(grid(n)), dim3(kRowThreads), 0, stream, values, leaf_of,
                  leafsum, d_labels, d_margins, static_cast<unsigned long long *>(nullptr), n,
                  static_cast<int32_t>(n_trees > 0), forest->base_margin);
    }
    if (n_eval > 0 && n_trees > 0) {
        DS_LAUNCH(ds_refresh_tail_kernel, dim3(grid(n_eval)), dim3(kRowThreads), 0, stream, values,
                  eval_leaf_of, eval_leafsum, d_eval_labels, static_cast<float *>(nullptr),
                  errors + n_trees, n_eval, 1, forest->base_margin);
    }
    DS_HIP(hipStreamSynchronize(stream));

    if (n_nodes) {
        DS_HIP(hipMemcpy(c.leaf_out, values, sizeof(float) * n_nodes, hipMemcpyDeviceToHost));
        DS_HIP(hipMemcpy(c.node_sums, sums, sizeof(int64_t) * 2 * n_nodes, hipMemcpyDeviceToHost));
    }
    if (n > 0 && c.margins) DS_HIP(hipMemcpy(c.margins, d_margins, sizeof(float) * n, hipMemcpyDeviceToHost));
    if (n > 0 && c.trace && n_trees > 0)
        DS_HIP(hipMemcpy(c.trace, d_trace, sizeof(float) * n * n_trees, hipMemcpyDeviceToHost));
    if (c.eval_errors != nullptr) {
        if (n_eval > 0) {
            DS_HIP(hipMemcpy(c.eval_errors, errors, sizeof(int64_t) * counters, hipMemcpyDeviceToHost));
        } else {
            for (size_t i = 0; i < counters; ++i) c.eval_errors[i] = -1;
        }
    }
    // inner nodes: the sum of their two children, children before parents (a child's id is above its parent's)
    int64_t empty = 0;
    for (int32_t t = 0; t < n_trees; ++t) {
        const int64_t begin = forest->h_offsets[t], end = forest->h_offsets[t + 1];
        for (int64_t i = end - 1; i >= begin; --i) {
            const int4 info = forest->h_nodes[static_cast<size_t>(i)];
            if (info.x < 0) {
                empty += c.node_sums[2 * i + 1] == 0;
                continue;
            }
            for (int k = 0; k < 2; ++k)
                c.node_sums[2 * i + k] = c.node_sums[2 * (begin + info.y) + k] + c.node_sums[2 * (begin + info.z) + k];
        }
    }
    *c.empty_leaves = empty;
    return DS_OK;
}

}  // namespace

}  // namespace ds

extern "C" {

int ds_forest_refresh_device(const ds_forest *forest, const float *d_features, int64_t n, const float *labels,
                             const float *weights, const float *d_eval_features, const float *eval_labels, int64_t n_eval,
                             double eta, double reg_lambda, double beta, int refresh_leaf, float *leaf_out,
                             int64_t *node_sums, float *margins, int64_t *eval_errors, int64_t *empty_leaves, float *trace,
                             void *stream)
{
    const char *who = "ds_forest_refresh_device";
    const ds::RefreshCall call{forest, d_features, labels, weights, d_eval_features, eval_labels, n, n_eval, eta,
                               reg_lambda, beta, refresh_leaf, leaf_out, node_sums, margins, eval_errors, empty_leaves,
                               trace};
    DS_TRY(ds::refresh_check(who, call));
    DS_TRY(ds::refresh_check_device(who, forest, d_features, "d_features"));
    DS_TRY(ds::refresh_check_device(who, forest, d_eval_features, "d_eval_features"));
    ds::Scratch scratch;
    return ds::refresh_run(who, call, scratch, &d_features, &d_eval_features, static_cast<hipStream_t>(stream));
}

int ds_forest_refresh(const ds_forest *forest, const float *features, int64_t n, const float *labels,
                      const float *weights, const float *eval_features, const float *eval_labels, int64_t n_eval,
                      double eta, double reg_lambda, double beta, int refresh_leaf, float *leaf_out, int64_t *node_sums,
                      float *margins, int64_t *eval_errors, int64_t *empty_leaves, float *trace)
{
    const char *who = "ds_forest_refresh";
    const ds::RefreshCall call{forest, features, labels, weights, eval_features, eval_labels, n, n_eval, eta, reg_lambda,
                               beta, refresh_leaf, leaf_out, node_sums, margins, eval_errors, empty_leaves, trace};
    DS_TRY(ds::refresh_check(who, call));
    // every tree reads the matrices again: they are uploaded once, whole
    ds::Scratch scratch;
    const float *d_rows = nullptr, *d_eval = nullptr;
    scratch.stage(&d_rows, features, static_cast<size_t>(n) * forest->n_features);
    scratch.stage(&d_eval, eval_features, static_cast<size_t>(n_eval) * forest->n_features);
    return ds::refresh_run(who, call, scratch, &d_rows, &d_eval, nullptr);
}

}  // extern "C"
