// Next row f-4: the gradient-boosted tree ensemble applied to the 66 features
// (doppelspeller/predict.py:229-234: xgb.DMatrix(features); model.predict(..., ntree_limit=best_ntree_limit)), so that
// the feature matrix written by ds_construct_features_* never leaves HBM (264 B per pair saved).
//
// xgboost is a third-party dependency that is not part of the reference tree; the kernel follows the published
// prediction rule of a `binary:logistic` booster on a dense float32 matrix with missing = NaN: per tree, from the root,
// a NaN follows the node's `missing` child, otherwise value < split_condition follows `yes`, else `no`; leaf values of
// the first n_trees trees are added in tree order in float32 to the base margin; prediction = 1 / (1 + exp(-margin)).
// The GPU tests compare margins bit-for-bit with a CPU restatement; the float32 exp of the sigmoid is within 2 ulp of libm.
// Parity unpinned against the real library.
//
// One thread per row: the rows of a workgroup are staged in LDS (row-major 66-float reads would be uncoalesced), the
// node arrays (a few hundred KiB for a typical model) stay L2-resident and are walked by all rows of a wavefront in
// the same tree at the same time.
#include "ds_launch.h"
#include "ds_forest.h"

namespace ds {

struct ForestArgs {
    ForestView forest;
    const float *rows;
    float *margins;        // nullable
    float *probabilities;  // nullable
    int64_t n;
};

__global__ __launch_bounds__(kForestThreads) void ds_forest_kernel(ForestArgs a)
{
    extern __shared__ float staged[];  // [kForestThreads][n_features + 1] (+1: bank spread)
    const int stride = a.forest.n_features + 1;
    for (int64_t first = static_cast<int64_t>(blockIdx.x) * kForestThreads; first < a.n;
         first += static_cast<int64_t>(gridDim.x) * kForestThreads) {
        const int rows_here =
            forest_stage_rows<kForestThreads>(a.rows, a.n, first, a.forest.n_features, staged, stride, 1);
        __syncthreads();
        if (static_cast<int>(threadIdx.x) < rows_here) {
            const float margin = a.forest.base_margin + forest_leaf_sum(a.forest, staged + threadIdx.x * stride);
            if (a.margins) a.margins[first + threadIdx.x] = margin;
            if (a.probabilities) a.probabilities[first + threadIdx.x] = forest_probability(margin);
        }
    }
}

}  // namespace ds

extern "C" {

int ds_forest_create(const int32_t *feature, const float *threshold, const int32_t *yes, const int32_t *no,
                     const int32_t *missing, const int64_t *tree_offsets, int32_t n_trees, int32_t n_features,
                     float base_margin, int device, ds_forest **out)
{
    DS_REQUIRE(out != nullptr, "ds_forest_create: out is null");
    *out = nullptr;
    DS_REQUIRE(feature && threshold && yes && no && missing && tree_offsets, "ds_forest_create: null input");
    DS_REQUIRE(n_trees >= 0 && n_features >= 1 && n_features <= ds::kForestFeaturesMax,
               "ds_forest_create: n_trees=%d n_features=%d out of range", n_trees, n_features);
    DS_REQUIRE(tree_offsets[0] == 0, "ds_forest_create: tree_offsets[0] must be 0");
    const int64_t n_nodes = tree_offsets[n_trees];
    std::vector<int4> nodes(static_cast<size_t>(n_nodes));
    for (int32_t t = 0; t < n_trees; ++t) {
        const int64_t begin = tree_offsets[t], end = tree_offsets[t + 1];
        DS_REQUIRE(end > begin, "ds_forest_create: tree %d is empty", t);
        for (int64_t i = begin; i < end; ++i) {
            const int32_t f = feature[i];
            DS_REQUIRE(f < n_features, "ds_forest_create: node %lld splits on feature %d >= %d", (long long)i, f,
                       n_features);
            if (f >= 0) {
                const int64_t size = end - begin;
                // children must lie inside the tree and after their parent (no cycles: the walk always terminates)
                DS_REQUIRE(yes[i] > i - begin && yes[i] < size && no[i] > i - begin && no[i] < size &&
                               missing[i] > i - begin && missing[i] < size,
                           "ds_forest_create: node %lld has a child outside its tree or before itself", (long long)i);
            }
            nodes[static_cast<size_t>(i)] = make_int4(f >= 0 ? f : -1, yes[i], no[i], missing[i]);
        }
    }
    DS_HIP(hipSetDevice(device));
    ds_forest *forest = new ds_forest();
    forest->device = device;
    forest->n_trees = n_trees;
    forest->n_features = n_features;
    forest->n_nodes = n_nodes;
    forest->base_margin = base_margin;
    forest->h_threshold.assign(threshold, threshold + n_nodes);
    forest->h_offsets.assign(tree_offsets, tree_offsets + n_trees + 1);
    int status = forest->nodes.upload(nodes.data(), nodes.size());
    if (status == DS_OK && nodes.empty()) status = forest->nodes.allocate(1);
    if (status == DS_OK) status = forest->threshold.upload(threshold, static_cast<size_t>(n_nodes));
    if (status == DS_OK && n_nodes == 0) status = forest->threshold.allocate(1);
    if (status == DS_OK) status = forest->tree_offsets.upload(tree_offsets, static_cast<size_t>(n_trees) + 1);
    if (status != DS_OK) {
        delete forest;
        return status;
    }
    forest->h_nodes = std::move(nodes);
    *out = forest;
    return DS_OK;
}

void ds_forest_destroy(ds_forest *forest)
{
    if (!forest) return;
    (void)hipSetDevice(forest->device);
    delete forest;
}

int ds_forest_predict_device(ds_forest *forest, const float *d_rows, int64_t n, float *d_margins,
                             float *d_probabilities, void *stream)
{
    DS_REQUIRE(forest != nullptr && n >= 0, "ds_forest_predict: bad arguments");
    if (n == 0) return DS_OK;
    DS_REQUIRE(d_rows && (d_margins || d_probabilities), "ds_forest_predict: null pointer");
    DS_HIP(hipSetDevice(forest->device));
    const ds::ForestArgs args{forest->view(), d_rows, d_margins, d_probabilities, n};
    const int64_t blocks = (n + ds::kForestThreads - 1) / ds::kForestThreads;
    const int grid = static_cast<int>(std::min<int64_t>(blocks, 256 * 16));
    const size_t lds = static_cast<size_t>(ds::kForestThreads) * (forest->n_features + 1) * sizeof(float);
    DS_TRY(ds::allow_dynamic_lds(ds::ds_forest_kernel, lds));
    DS_LAUNCH(ds::ds_forest_kernel, dim3(grid), dim3(ds::kForestThreads), lds, static_cast<hipStream_t>(stream),
              args);
    return DS_OK;
}

int ds_forest_predict(ds_forest *forest, const float *rows, int64_t n, float *margins, float *probabilities)
{
    DS_REQUIRE(forest != nullptr && n >= 0, "ds_forest_predict: bad arguments");
    if (n == 0) return DS_OK;
    DS_REQUIRE(rows && (margins || probabilities), "ds_forest_predict: null pointer");
    DS_HIP(hipSetDevice(forest->device));
    ds::Scratch scratch;
    const float *d_rows = nullptr;
    float *d_margins = nullptr, *d_probabilities = nullptr;
    scratch.stage(&d_rows, rows, static_cast<size_t>(n) * forest->n_features);
    if (margins) scratch.add(&d_margins, static_cast<size_t>(n));
    if (probabilities) scratch.add(&d_probabilities, static_cast<size_t>(n));
    DS_TRY(scratch.allocate("ds_forest_predict"));
    DS_TRY(ds_forest_predict_device(forest, d_rows, n, d_margins, d_probabilities, nullptr));
    DS_HIP(hipDeviceSynchronize());
    if (margins) DS_HIP(hipMemcpy(margins, d_margins, sizeof(float) * n, hipMemcpyDeviceToHost));
    if (probabilities) DS_HIP(hipMemcpy(probabilities, d_probabilities, sizeof(float) * n, hipMemcpyDeviceToHost));
    return DS_OK;
}

}  // extern "C"
