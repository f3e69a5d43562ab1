// The tree ensemble as it lives in HBM and on the host, and the one copy of what every stage that sends a float32 row
// through it shares: the model as a kernel sees it (ForestView), the branch rule, the walk and the leaf sum, the
// staging of a workgroup's rows in LDS, and the step from a margin to a probability and a verdict.  Its users:
// ds_forest.hip (prediction), ds_contributions.hip (node cover, TreeSHAP and Saabas), ds_inspect.hip (permutation
// importance and partial dependence), ds_train.hip and ds_train_batch.hip (the trainers' seed from an init model),
// ds_refresh.hip (leaf refresh), and through ds_train.h the trainers' gradient and error kernels and ds_bootstrap.hip
// (outcome codes).
#pragma once

#include "ds_options.h"

namespace ds {

// The model as a kernel sees it: ds_forest::view() fills it.
struct ForestView {
    const int4 *nodes;             // (feature or -1, yes, no, missing) per node, tree-relative child ids
    const float *threshold;        // split condition, or the leaf value
    const int64_t *tree_offsets;
    int32_t n_trees, n_features;
    float base_margin;
};

constexpr int kForestThreads = 256;
constexpr int kForestFeaturesMax = 96;  // LDS staging: kForestThreads x n_features floats (66 for this reference)
constexpr int kContributionsMaxDepth = 16;  // splits on a root-to-leaf path at most (ds_forest_contributions*)
constexpr int kRefreshLdsNodesMax = 2048;   // nodes of a tree whose (g, h) sums a refresh workgroup keeps in LDS: 32 KiB
constexpr int kForestBlocksLimit = 1 << 20; // ds_forest_option("max_blocks") at most

// One element of a root-to-leaf path: all of the path's splits on one feature merged.  A row follows the element when
// its value v is NaN and nan_follows, or is not NaN and !(v < lo) && !(v >= hi) (a NaN bound stands for "no bound").
struct PathElement {
    int32_t feature;
    uint32_t nan_follows;
    float lo, hi;
    double zero_fraction;      // product of cover[child] / cover[parent] over the merged splits
    double zero_reciprocal;    // 1 / zero_fraction
};

// The branch rule of a float tree walk: at the split `info` with the cut `cut`, a NaN follows `missing`, value < cut
// `yes`, any other value `no`.  Returns the tree-relative child.  Every walk states the rule through this function, but
// for the K-chain loop of ds_inspect.hip, which says why it cannot.  The cut comes by pointer and is read only for a
// value that is not NaN: a walk that has not loaded it yet then loads it under that condition, and a cut taken by
// value, loaded for every row, measured 11% slower in ds_forest_kernel at the benchmark's shape.
__device__ __forceinline__ int forest_branch(int4 info, float value, const float *cut)
{
    return (value != value) ? info.w : (value < *cut ? info.y : info.z);
}

// The walk of one row through the tree whose root is node `root`.  Returns the leaf's node.  `row` holds the row's
// n_features values.  It takes pointers, not a view: ds_refresh.hip walks a working copy of the thresholds.
__device__ inline int64_t forest_walk(const int4 *nodes, const float *threshold, int64_t root, const float *row)
{
    int64_t node = root;
    int4 info = nodes[node];
    while (info.x >= 0) {
        node = root + forest_branch(info, row[info.x], threshold + node);
        info = nodes[node];
    }
    return node;
}

// The prediction rule for one row (ds_forest.hip's header): the float32 sum of the leaves the row reaches in the
// forest's trees, from zero in tree order, without the base margin.  `row` holds the row's n_features values.
__device__ inline float forest_leaf_sum(const ForestView &forest, const float *row)
{
    float sum = 0.f;  // xgboost: PredValue sums the leaves from zero, the base margin is added to that sum
    for (int32_t t = 0; t < forest.n_trees; ++t)
        sum = sum + forest.threshold[forest_walk(forest.nodes, forest.threshold, forest.tree_offsets[t], row)];
    return sum;
}

// Stages the kThreads-thread workgroup's rows, rows [first, first + rows_here) of the row-major float32[n][n_features]
// matrix `rows`, in LDS: value f of row r goes to staged[r * row_stride + f * feature_stride], read coalesced.  The
// strides are the caller's, and so is the layout.  Returns rows_here, at most kThreads.
// The barrier before the copy is this routine's: no thread still reads what the copy overwrites.  The barrier after it
// is the caller's, who may have more to write that the same barrier publishes: ds_contributions_kernel zeroes its sums.
template <int kThreads>
__device__ __forceinline__ int forest_stage_rows(const float *rows, int64_t n, int64_t first, int n_features,
                                                 float *staged, int row_stride, int feature_stride)
{
    const int rows_here = static_cast<int>(n - first < kThreads ? n - first : kThreads);
    __syncthreads();
    for (int e = threadIdx.x; e < rows_here * n_features; e += kThreads) {
        const int r = e / n_features, f = e - r * n_features;
        staged[r * row_stride + f * feature_stride] = rows[first * n_features + e];
    }
    return rows_here;
}

// From a margin to the probability, in float32, and from the probability to the verdict: positive iff (double)p > cut,
// which is false for a NaN.  Every result of this family is promised bit for bit, so these are the only statements.
__device__ __forceinline__ float forest_probability(float margin)
{
    return 1.0f / (1.0f + expf(-margin));
}

__device__ __forceinline__ bool forest_positive(float p, double cut)
{
    return static_cast<double>(p) > cut;
}

}  // namespace ds

struct ds_forest {
    int device = 0;
    int32_t n_trees = 0, n_features = 0;
    int64_t n_nodes = 0;
    float base_margin = 0.f;
    ds::DeviceBuffer<int4> nodes;          // (feature or -1, yes, no, missing) per node, tree-relative child ids
    ds::DeviceBuffer<float> threshold;     // split condition, or the leaf value
    ds::DeviceBuffer<int64_t> tree_offsets;
    // the same model on the host (what the path decomposition of ds_contributions.hip reads)
    std::vector<int4> h_nodes;
    std::vector<float> h_threshold;
    std::vector<int64_t> h_offsets;
    // node cover (ds_contributions.hip): none, counted on the device (integer counters in HBM) or installed by the caller
    enum CoverState { kCoverNone = 0, kCoverCounted = 1, kCoverSet = 2 };
    int cover_state = kCoverNone;
    std::vector<double> cover;                      // kCoverSet: the caller's values
    ds::DeviceBuffer<unsigned long long> counts;    // kCoverCounted: rows that reached each node
    int shape_checked = 0;                          // 0 not yet, 1 every tree is a proper binary tree
    std::vector<int32_t> parent;                    // global parent node of every node, -1 for a root or an unreachable node
    // ds_forest_option: the cap of every stage's grid (0: the stage's own, max_blocks.value_or(it)), ds_inspect.hip's jobs
    // per workgroup (0: its choice) and ds_refresh.hip's table size
    ds::Option max_blocks{"max_blocks", 0, ds::kForestBlocksLimit, 0, true};
    ds::Option inspect_jobs_per_block{"inspect_jobs_per_block", 0, INT32_MAX, 0};
    ds::Option refresh_lds_nodes{"refresh_lds_nodes", 0, ds::kRefreshLdsNodesMax, ds::kRefreshLdsNodesMax, true};
    // what the contributions kernels read, derived from the cover when they are first asked for
    bool prepared = false;
    int64_t n_paths = 0;
    int32_t max_elements = 0;
    double bias = 0.0;
    ds::DeviceBuffer<int32_t> path_start;           // [n_paths + 1] first element of every path
    ds::DeviceBuffer<double> path_leaf;             // [n_paths] leaf value
    ds::DeviceBuffer<ds::PathElement> elements;
    ds::DeviceBuffer<double> node_mean;             // [n_nodes] cover-weighted mean leaf value of the subtree

    ds::ForestView view() const
    {
        return ds::ForestView{nodes.ptr, threshold.ptr, tree_offsets.ptr, n_trees, n_features, base_margin};
    }
};

namespace ds {

// Every tree a proper binary tree (two different children, `missing` one of them, one parent per node): DS_E_ARG in the
// name of `what` otherwise.  parent[i] = the global parent node of node i, -1 for a root or an unreachable node.
// Defined in ds_contributions.hip, whose cover and paths rest on it; ds_refresh.hip's node sums do too.
int forest_parents(const ds_forest *forest, const char *what, std::vector<int32_t> &parent);

}  // namespace ds
