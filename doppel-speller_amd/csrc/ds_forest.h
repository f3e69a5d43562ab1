// The tree ensemble as it lives in HBM and on the host, shared by ds_forest.hip (prediction) and ds_contributions.hip
// (node cover and per-feature contributions).
#pragma once

#include "ds_common.h"

namespace ds {

constexpr int kForestThreads = 256;
constexpr int kForestFeaturesMax = 96;  // LDS staging: kForestThreads x n_features floats (66 for this reference)
constexpr int kContributionsMaxDepth = 16;  // splits on a root-to-leaf path at most (ds_forest_contributions*)
constexpr int kRefreshLdsNodesMax = 2048;   // nodes of a tree whose (g, h) sums a refresh workgroup keeps in LDS: 32 KiB

// One element of a root-to-leaf path: all of the path's splits on one feature merged.  A row follows the element when
// its value v is NaN and nan_follows, or is not NaN and !(v < lo) && !(v >= hi) (a NaN bound stands for "no bound").
struct PathElement {
    int32_t feature;
    uint32_t nan_follows;
    float lo, hi;
    double zero_fraction;      // product of cover[child] / cover[parent] over the merged splits
    double zero_reciprocal;    // 1 / zero_fraction
};

// The walk of one row through the tree whose root is node `root`: a NaN follows `missing`, value < threshold `yes`, any
// other value `no`.  Returns the leaf's node.  `row` holds the row's n_features values.
__device__ inline int64_t forest_walk(const int4 *nodes, const float *threshold, int64_t root, const float *row)
{
    int64_t node = root;
    int4 info = nodes[node];
    while (info.x >= 0) {
        const float value = row[info.x];
        const int next = (value != value) ? info.w : (value < threshold[node] ? info.y : info.z);
        node = root + next;
        info = nodes[node];
    }
    return node;
}

// The prediction rule for one row (ds_forest.hip's header): the float32 sum of the leaves the row reaches in the first
// n_trees trees, from zero in tree order, without the base margin.  `row` holds the row's n_features values (in LDS).
// Shared by ds_forest_kernel and by ds_train_seed_kernel (ds_train.hip), which starts a trainer's margins from a forest.
__device__ inline float forest_leaf_sum(const int4 *nodes, const float *threshold, const int64_t *tree_offsets,
                                        int32_t n_trees, const float *row)
{
    float sum = 0.f;  // xgboost: PredValue sums the leaves from zero, the base margin is added to that sum
    for (int32_t t = 0; t < n_trees; ++t) sum = sum + threshold[forest_walk(nodes, threshold, tree_offsets[t], row)];
    return sum;
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
    int64_t max_blocks = 0;                         // ds_forest_option("max_blocks"): 0 = the default of each stage
    int64_t inspect_jobs_per_block = 0;             // ds_forest_option("inspect_jobs_per_block"): 0 = ds_inspect.hip's choice
    int64_t refresh_lds_nodes = 0;                  // ds_forest_option("refresh_lds_nodes"): 0 = ds_refresh.hip's table size
    // what the contributions kernels read, derived from the cover when they are first asked for
    bool prepared = false;
    int64_t n_paths = 0;
    int32_t max_elements = 0;
    double bias = 0.0;
    ds::DeviceBuffer<int32_t> path_start;           // [n_paths + 1] first element of every path
    ds::DeviceBuffer<double> path_leaf;             // [n_paths] leaf value
    ds::DeviceBuffer<ds::PathElement> elements;
    ds::DeviceBuffer<double> node_mean;             // [n_nodes] cover-weighted mean leaf value of the subtree
};

namespace ds {

// Every tree a proper binary tree (two different children, `missing` one of them, one parent per node): DS_E_ARG in the
// name of `what` otherwise.  parent[i] = the global parent node of node i, -1 for a root or an unreachable node.
// Defined in ds_contributions.hip, whose cover and paths rest on it; ds_refresh.hip's node sums do too.
int forest_parents(const ds_forest *forest, const char *what, std::vector<int32_t> &parent);

}  // namespace ds
