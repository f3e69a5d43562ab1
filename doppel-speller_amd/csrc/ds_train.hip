// Training of the match model (doppelspeller/train.py: xgb.train with obj=weighted_log_loss, feval=custom_error):
// histogram gradient boosting with depth-wise growth on the device.  The rule (DESIGN.md section "Training") is
// restated by a NumPy model in the tests, which compare every tree, margin and error bit for bit.
//
// Data in HBM, per training matrix (n rows, nf features):
//   bins      uint8[nf][n]   feature-major: bin b < 255 of a value, 255 = NaN (the missing bin)
//   gh        int64[n][2]    quantized gradient and hessian of the current round, rint(g * 2^30), rint(h * 2^30)
//   weights   float[n]       only after ds_trainer_set_weights: g and h are multiplied by the row's weight first
//   node_of   int32[n]       heap id of the node a row sits in while a tree grows (-1: its leaf is already added)
//   leafsum   float[n]       sum of the leaves of the trees so far, in tree order (margin = kTrainBaseMargin + leafsum)
//   hist      int64[2^D - 1][nf][256][2]  per split candidate node (heap order, levels 0..D-1): (sum qg, sum qh)
//                            per bin; entry 255 = the missing bin
//   nodes     Node[2^(D+1) - 1] the tree being grown, heap order (children of i: 2i + 1, 2i + 2)
// Integer sums do not depend on the order of their terms: histograms, splits and trees are identical under any
// schedule and from run to run.
// The rule's device code lives in ds_train.h.  This file holds the kernels of a round, which run it for the models of a
// TrainView, the one launcher of a round (train_round_enqueue) and the host checks and helpers of both trainers, and the
// single trainer: a view of one model with nothing held out.  The batched trainer (ds_train_batch.hip) launches the same
// kernels through the same launcher with the model as a further grid dimension.
// Continuing from a model (ds_trainer_seed, DESIGN.md section 9 "Continuing from a model"): before the first round
// ds_train_seed_kernel sets leafsum to a forest's leaf sums of the RAW rows, and the trees count on from the forest's.

#include "ds_launch.h"
#include "ds_forest.h"
#include "ds_metrics.h"
#include "ds_train.h"

namespace ds {

// ---- binning: float32[n][nf] row-major -> uint8[nf][n]; all cuts staged in LDS ------------------------------------
__global__ __launch_bounds__(kRowThreads) void ds_train_bin_kernel(const float *rows, int64_t n, int32_t nf,
                                                                    const float *cuts, const int32_t *cut_offsets,
                                                                    uint8_t *bins)
{
    __shared__ float s_cuts[kTrainFeaturesMax * kTrainCutsMax];
    __shared__ int32_t s_offsets[kTrainFeaturesMax + 1];
    __shared__ float s_tile[kBinTileRows * kTrainFeaturesMax];
    for (int i = threadIdx.x; i <= nf; i += kRowThreads) s_offsets[i] = cut_offsets[i];
    __syncthreads();
    for (int i = threadIdx.x; i < s_offsets[nf]; i += kRowThreads) s_cuts[i] = cuts[i];
    for (int64_t first = static_cast<int64_t>(blockIdx.x) * kBinTileRows; first < n;
         first += static_cast<int64_t>(gridDim.x) * kBinTileRows) {
        const int rows_here = static_cast<int>(n - first < kBinTileRows ? n - first : kBinTileRows);
        __syncthreads();
        for (int e = threadIdx.x; e < rows_here * nf; e += kRowThreads)   // coalesced row-major read
            s_tile[e] = rows[first * nf + e];
        __syncthreads();
        for (int e = threadIdx.x; e < kBinTileRows * nf; e += kRowThreads) {
            const int f = e / kBinTileRows, r = e - f * kBinTileRows;   // consecutive lanes: consecutive rows of one feature
            if (r >= rows_here) continue;
            const float x = s_tile[r * nf + f];
            int bin = kMissingBin;
            if (x == x) {   // searchsorted(cuts, x, side="right"): the number of cuts <= x
                int lo = s_offsets[f], hi = s_offsets[f + 1];
                const int base = lo;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s_cuts[mid] <= x) lo = mid + 1; else hi = mid;
                }
                bin = lo - base;
            }
            bins[static_cast<int64_t>(f) * n + first + r] = static_cast<uint8_t>(bin);
        }
    }
}

// ---- the kernels of a round: ds_train.h's bodies for the models of a TrainView, of either trainer --------------------
// The model is v.active[the last grid dimension] (model 0 of a one-model view); the blocks of a model that has passed its own max_depth return at once.
// kFolds = false (the single trainer) reads no fold byte; kSampled = false reads nothing of the sampling view.

// start of a round: zero the active models' histograms (levels below their own max_depth), heaps, counts, errors; with
// monotone constraints the root's bounds are set here too
__global__ __launch_bounds__(kRowThreads) void ds_train_clear_kernel(TrainView v)
{
    const int32_t m = v.model_index(blockIdx.y);
    const int64_t at = blockIdx.x * static_cast<int64_t>(kRowThreads) + threadIdx.x;
    const int64_t step = static_cast<int64_t>(gridDim.x) * kRowThreads;
    const int64_t pairs = ((int64_t(1) << v.model(m).params.max_depth) - 1) * v.nf * 256;   // (g, h) of one bin
    ulonglong2 *hist = reinterpret_cast<ulonglong2 *>(v.hist + m * v.hist_stride);
    for (int64_t i = at; i < pairs; i += step) hist[i] = make_ulonglong2(0ull, 0ull);
    uint32_t *nodes = reinterpret_cast<uint32_t *>(v.nodes + static_cast<int64_t>(m) * v.slots);
    for (int64_t i = at; i < int64_t(v.slots) * (sizeof(Node) / 4); i += step) nodes[i] = 0u;
    int32_t *counts = v.counts + static_cast<int64_t>(m) * v.slots;
    for (int64_t i = at; i < v.slots; i += step) counts[i] = 0;
    if (at == 0) {
        v.errors[m] = 0ull;
        if (v.bounds != nullptr) {   // the root's weight is unbounded
            double *bounds = v.bounds + static_cast<int64_t>(m) * 2 * v.slots;
            bounds[0] = -INFINITY;
            bounds[1] = INFINITY;
        }
    }
}

// the feature sets of the round: blockIdx.x = the model
__global__ __launch_bounds__(kMaskThreads) void ds_train_feature_mask_kernel(TrainView v, TrainSamplingView s)
{
    const int32_t m = v.model_index(blockIdx.x);
    const TrainSampling sampling = s.record(m);   // in registers, as in the gradient kernel
    train_feature_masks(sampling, s.tree_of(m), v.nf, v.model(m).params.max_depth,
                        s.masks + static_cast<int64_t>(m) * kMaskBytes);
}

// blockIdx.x = a stride of rows, blockIdx.y = the model
template <bool kFolds, bool kSampled>
__global__ __launch_bounds__(kRowThreads) void ds_train_gradient_kernel(TrainView v, TrainSamplingView s)
{
    const int32_t m = v.model_index(blockIdx.y);
    const TrainModel model = v.model(m);
    TrainSampling sampling{};   // a copy in registers: through the pointer the body's row loop re-reads it past its stores
    if (kSampled) sampling = s.record(m);
    const uint32_t *held_before = nullptr;
    if (kFolds && kSampled && s.held_slot[m] >= 0) held_before = s.held_before + s.held_slot[m] * s.held_stride;
    train_gradient_rows<kFolds, kSampled>(v.leafsum + m * v.n, v.labels, v.n, kTrainBaseMargin, model.params.beta,
                                          v.probabilities + m * v.n, v.gh + 2 * m * v.n, v.node_of + m * v.n, v.fold,
                                          model.held_out, v.weights, kSampled ? &sampling : nullptr,
                                          kSampled ? s.tree_of(m) : 0, held_before);
}

// blockIdx.x = the chunk of rows, blockIdx.y = (feature group, node group), blockIdx.z = the model
template <bool kFolds, bool kSampled>
__global__ __launch_bounds__(kHistThreads) void ds_train_histogram_kernel(TrainView v, int32_t level, int32_t n_built,
                                                                           int32_t nodes_per_group,
                                                                           int32_t features_per_group,
                                                                           int32_t feature_groups)
{
    const int32_t m = v.model_index(blockIdx.z);
    const TrainModel model = v.model(m);
    if (level >= model.params.max_depth) return;   // the model's tree is finished: nothing pending
    train_histogram_group<kFolds, kSampled>(v.bins, v.gh + 2 * m * v.n, v.node_of + m * v.n,
                                            v.counts + int64_t(m) * v.slots, v.nodes + int64_t(m) * v.slots, v.n, v.nf,
                                            level, n_built, nodes_per_group, features_per_group, feature_groups,
                                            reinterpret_cast<unsigned long long *>(v.hist + m * v.hist_stride), v.fold,
                                            model.held_out);
}

// blockIdx.x = the node's index in its level, blockIdx.y = the feature, blockIdx.z = the model
// kMonotone = false reads neither v.monotone nor v.bounds
template <bool kSampled, bool kMonotone>
__global__ __launch_bounds__(256) void ds_train_split_feature_kernel(TrainView v, TrainSamplingView s, int32_t level)
{
    const int32_t m = v.model_index(blockIdx.z);
    const TrainModel model = v.model(m);
    if (level >= model.params.max_depth) return;
    train_split_feature<kSampled, kMonotone>(
        v.hist + m * v.hist_stride, v.counts + int64_t(m) * v.slots, v.nodes + int64_t(m) * v.slots, v.cut_offsets, v.nf,
        level, model.params, v.candidates + m * v.candidate_stride,
        kSampled ? s.masks + static_cast<int64_t>(m) * kMaskBytes + level * kTrainFeaturesMax : nullptr,
        kMonotone ? v.monotone : nullptr, kMonotone ? v.bounds + int64_t(m) * 2 * v.slots : nullptr);
}

// blockIdx.x = 64 nodes of the level, blockIdx.y = the model
template <bool kMonotone>
__global__ __launch_bounds__(64) void ds_train_split_kernel(TrainView v, int32_t level)
{
    const int32_t m = v.model_index(blockIdx.y);
    const TrainModel model = v.model(m);
    if (level >= model.params.max_depth) return;
    train_split_nodes<kMonotone>(v.candidates + m * v.candidate_stride, v.nodes + int64_t(m) * v.slots, v.nf, level,
                                 model.params, kMonotone ? v.monotone : nullptr,
                                 kMonotone ? v.bounds + int64_t(m) * 2 * v.slots : nullptr);
}

__global__ __launch_bounds__(kRowThreads) void ds_train_partition_kernel(TrainView v, int32_t level)
{
    const int32_t m = v.model_index(blockIdx.y);
    if (level >= v.model(m).params.max_depth) return;
    train_partition_rows(v.bins, v.nodes + int64_t(m) * v.slots, v.n, level, v.node_of + m * v.n, v.leafsum + m * v.n,
                         v.counts + int64_t(m) * v.slots);
}

// ---- evaluation rows: add the new tree, then the custom error of train.py:fast_custom_error ------------------------
__global__ __launch_bounds__(kRowThreads) void ds_train_eval_kernel(const uint8_t *bins, const Node *nodes, int64_t n,
                                                                     const float *labels, float base_margin,
                                                                     float *leafsum, unsigned long long *error)
{
    __shared__ unsigned long long s_error;
    if (threadIdx.x == 0) s_error = 0;
    __syncthreads();
    unsigned long long mine = 0;
    for (int64_t r = blockIdx.x * static_cast<int64_t>(kRowThreads) + threadIdx.x; r < n;
         r += static_cast<int64_t>(gridDim.x) * kRowThreads) {
        int32_t node = 0;
        Node rec = nodes[0];
        while (rec.state == kSplit) {
            const int bin = bins[static_cast<int64_t>(rec.feature) * n + r];
            const bool left = bin == kMissingBin ? rec.default_left != 0 : bin < rec.bin;
            node = 2 * node + (left ? 1 : 2);
            rec = nodes[node];
        }
        const float sum = leafsum[r] + rec.leaf;
        leafsum[r] = sum;
        mine += train_row_error(base_margin + sum, labels[r]);
    }
    if (mine) atomicAdd(&s_error, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_error) atomicAdd(error, s_error);
}

// ---- continuing from a model: a forest's leaf sums of the RAW rows, before the first round ---------------------------
// The init model's thresholds need not be cuts of this matrix, so it is walked over the float32 features and not over the
// bins.  One thread per row, the rows of a workgroup staged in LDS at an odd stride (n_features | 1): thread t reads
// word t * stride + f, and an odd stride spreads a wave's 64 rows over all 64 banks for any feature count.  The sum is
// the margin without the base margin; it goes to the leaf sums of all n_models models of the view (stride apart),
// held-out rows included.
struct SeedArgs {
    ForestView forest;
    const float *rows;
    float *leafsum;
    int64_t n, stride;
    int32_t n_models;
};

__global__ __launch_bounds__(kRowThreads) void ds_train_seed_kernel(SeedArgs a)
{
    extern __shared__ float s_rows[];   // [kRowThreads][n_features | 1]
    const int stride = a.forest.n_features | 1;
    for (int64_t first = static_cast<int64_t>(blockIdx.x) * kRowThreads; first < a.n;
         first += static_cast<int64_t>(gridDim.x) * kRowThreads) {
        const int rows_here =
            forest_stage_rows<kRowThreads>(a.rows, a.n, first, a.forest.n_features, s_rows, stride, 1);
        __syncthreads();
        if (static_cast<int>(threadIdx.x) < rows_here) {
            const float sum = forest_leaf_sum(a.forest, s_rows + threadIdx.x * stride);
            float *out = a.leafsum + first + threadIdx.x;
            for (int32_t m = 0; m < a.n_models; ++m) out[m * a.stride] = sum;
        }
    }
}

// the custom error of n rows at their margins as they stand (the initial error of a seeded trainer's evaluation set)
__global__ __launch_bounds__(kRowThreads) void ds_train_error_kernel(const float *leafsum, const float *labels, int64_t n,
                                                                      float base_margin, unsigned long long *error)
{
    __shared__ unsigned long long s_error;
    if (threadIdx.x == 0) s_error = 0;
    __syncthreads();
    unsigned long long mine = 0;
    for (int64_t r = blockIdx.x * static_cast<int64_t>(kRowThreads) + threadIdx.x; r < n;
         r += static_cast<int64_t>(gridDim.x) * kRowThreads)
        mine += train_row_error(base_margin + leafsum[r], labels[r]);
    if (mine) atomicAdd(&s_error, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_error) atomicAdd(error, s_error);
}

// ---- row gather of a float32[n_src][nf] matrix in HBM (the split of the training set) ------------------------------
__global__ __launch_bounds__(kRowThreads) void ds_gather_check_kernel(const int64_t *rows, int64_t n_rows, int64_t n_src,
                                                                       int32_t *errors)
{
    for (int64_t r = blockIdx.x * static_cast<int64_t>(kRowThreads) + threadIdx.x; r < n_rows;
         r += static_cast<int64_t>(gridDim.x) * kRowThreads)
        if (rows[r] < 0 || rows[r] >= n_src) atomicAdd(errors, 1);
}

// one dword per thread: consecutive lanes read and write consecutive dwords of a row
__global__ __launch_bounds__(kRowThreads) void ds_gather_rows_kernel(const uint32_t *src, int32_t nf, const int64_t *rows,
                                                                      int64_t n_rows, int64_t n_src, uint32_t *dst)
{
    const int64_t total = n_rows * nf;
    for (int64_t e = blockIdx.x * static_cast<int64_t>(kRowThreads) + threadIdx.x; e < total;
         e += static_cast<int64_t>(gridDim.x) * kRowThreads) {
        const int64_t r = e / nf, row = rows[r];
        if (row < 0 || row >= n_src) continue;   // refused by ds_gather_check_kernel before this launch; never read
        dst[e] = src[row * nf + (e - r * nf)];
    }
}

// ---- host code of both trainers (declared in ds_train.h) -------------------------------------------------------------
int train_bin_matrix(hipStream_t stream, int compute_units, const float *rows, bool in_hbm, int64_t n, int32_t nf,
                     const float *d_cuts, const int32_t *d_cut_offsets, DeviceBuffer<uint8_t> &out)
{
    DeviceBuffer<float> staged;
    DS_TRY(in_hbm ? DS_OK : staged.upload(rows, static_cast<size_t>(n) * nf));
    DS_TRY(out.allocate(static_cast<size_t>(n) * nf));
    const int64_t tiles = (n + kBinTileRows - 1) / kBinTileRows;
    const int grid = static_cast<int>(std::min<int64_t>(tiles, int64_t(compute_units) * 4));
    DS_LAUNCH(ds_train_bin_kernel, dim3(grid), dim3(kRowThreads), 0, stream, in_hbm ? rows : staged.ptr, n, nf,
              d_cuts, d_cut_offsets, out.ptr);
    DS_HIP(hipStreamSynchronize(stream));   // `staged` is freed on return; the caller's matrix is no longer read
    return DS_OK;
}

int train_check_cuts(const char *who, int32_t n_features, const float *cuts, const int32_t *cut_offsets)
{
    DS_REQUIRE(cut_offsets[0] == 0, "%s: cut_offsets[0] must be 0", who);
    for (int32_t f = 0; f < n_features; ++f) {
        const int32_t count = cut_offsets[f + 1] - cut_offsets[f];
        DS_REQUIRE(count >= 0 && count <= kTrainCutsMax, "%s: feature %d has %d cuts (at most %d)", who,
                   f, count, kTrainCutsMax);
        for (int32_t i = cut_offsets[f]; i < cut_offsets[f + 1]; ++i)
            DS_REQUIRE(cuts[i] == cuts[i] && (i == cut_offsets[f] || cuts[i - 1] < cuts[i]),
                       "%s: the cuts of feature %d are not strictly ascending", who, f);
    }
    return DS_OK;
}

int train_check_shape(const char *who, int64_t n, int32_t n_features)
{
    DS_REQUIRE(n >= 1 && n <= INT32_MAX, "%s: n = %lld rows out of range [1, 2^31)", who, (long long)n);
    DS_REQUIRE(n_features >= 1 && n_features <= kTrainFeaturesMax, "%s: n_features = %d out of range [1, %d]", who,
               n_features, kTrainFeaturesMax);
    return DS_OK;
}

namespace {

// the part of a refusal that names the batch's model: `format` with its index, nothing for model < 0
struct ModelName {
    char text[32] = "";
    ModelName(const char *format, int32_t model)
    {
        if (model >= 0) std::snprintf(text, sizeof(text), format, model);
    }
};

}  // namespace

int train_check_params(const char *who, int32_t model, double eta, double min_child_weight, double reg_lambda,
                       double beta)
{
    const ModelName name("params of model %d: ", model);
    DS_REQUIRE(eta > 0 && eta < 1e30 && min_child_weight >= 0 && min_child_weight < 1e30 && reg_lambda >= 0 &&
                   reg_lambda < 1e30 && beta > 0 && beta < 1e30 && reg_lambda + min_child_weight > 0,
               "%s: %seta, beta must be positive, min_child_weight, reg_lambda non-negative and not both 0", who,
               name.text);
    return DS_OK;
}

int train_check_labels(const char *who, const char *what, const float *labels, int64_t n)
{
    for (int64_t r = 0; r < n; ++r)
        DS_REQUIRE(labels[r] == 0.f || labels[r] == 1.f, "%s: %slabel %lld is not 0 or 1", who, what, (long long)r);
    return DS_OK;
}

int train_check_fractions(const char *who, int32_t model, const double *fractions)
{
    const ModelName name("model %d: ", model);
    const char *names[3] = {"subsample", "colsample_bytree", "colsample_bylevel"};
    for (int i = 0; i < 3; ++i)
        DS_REQUIRE(fractions[i] > 0 && fractions[i] <= 1, "%s: %s%s = %g out of range (0, 1]", who, name.text, names[i],
                   fractions[i]);
    return DS_OK;
}

int train_check_subsample(const char *who, int32_t model, double subsample, double reg_lambda)
{
    const ModelName name("model %d: ", model);
    DS_REQUIRE(subsample == 1 || reg_lambda > 0, "%s: %ssubsample < 1 needs reg_lambda > 0 (a round may draw no row)", who,
               name.text);
    return DS_OK;
}

int train_check_weights(const char *who, const float *weights, int64_t n, double beta)
{
    double total = 0.0;
    for (int64_t r = 0; r < n; ++r) {
        DS_REQUIRE(std::isfinite(weights[r]), "%s: weight %lld is not finite", who, (long long)r);
        DS_REQUIRE(weights[r] >= 0.f, "%s: weight %lld is negative", who, (long long)r);
        total += static_cast<double>(weights[r]);
    }
    // |g| <= max(beta, 1) * s_r and a histogram cell sums at most all rows: every int64 sum stays below 2^62 + n
    DS_REQUIRE(std::max(beta, 1.0) * total <= 4294967296.0,
               "%s: max(beta, 1) * the total weight = %g exceeds 2^32 (the integer sums could overflow)", who,
               std::max(beta, 1.0) * total);
    return DS_OK;
}

int train_create_setup(const char *who, int device, int32_t n_features, const float *cuts, const int32_t *cut_offsets,
                       hipStream_t *stream, DeviceBuffer<float> &d_cuts, DeviceBuffer<int32_t> &d_cut_offsets,
                       int *compute_units)
{
    *compute_units = ds::compute_units(device);
    if (hipStreamCreateWithFlags(stream, hipStreamNonBlocking) != hipSuccess) {
        set_error("%s: hipStreamCreate failed", who);
        return DS_E_HIP;
    }
    int status = d_cut_offsets.upload(cut_offsets, static_cast<size_t>(n_features) + 1);
    if (status == DS_OK) status = d_cuts.allocate(std::max<size_t>(1, static_cast<size_t>(cut_offsets[n_features])));
    if (status == DS_OK && cut_offsets[n_features] > 0)
        status = d_cuts.upload(cuts, static_cast<size_t>(cut_offsets[n_features]));
    return status;
}

void train_unpack_heap(const Node *heap, int64_t slots, int32_t *node_info, float *node_leaf)
{
    for (int64_t i = 0; i < slots; ++i) {
        const Node &node = heap[i];
        node_info[4 * i] = node.state;
        node_info[4 * i + 1] = node.feature;
        node_info[4 * i + 2] = node.bin;
        node_info[4 * i + 3] = node.default_left;
        node_leaf[i] = node.leaf;
    }
}

int train_check_seed_forest(const char *who, const ds_forest *forest, int device, int32_t n_features)
{
    DS_REQUIRE(forest != nullptr, "%s: forest is null", who);
    DS_REQUIRE(forest->device == device, "%s: the forest lives on device %d, the trainer on device %d", who,
               forest->device, device);
    DS_REQUIRE(forest->n_features == n_features, "%s: the forest has %d features, the trainer %d", who,
               forest->n_features, n_features);
    DS_REQUIRE(forest->base_margin == kTrainBaseMargin,
               "%s: the forest's base margin is %g, a trainer continues only from base margin %g (base_score 0.5)", who,
               forest->base_margin, kTrainBaseMargin);
    return DS_OK;
}

int train_seed_enqueue(hipStream_t stream, int compute_units, const ds_forest *forest, const float *rows, bool in_hbm,
                       int64_t n, float *leafsum, int32_t n_models, int64_t stride, DeviceBuffer<float> &staged)
{
    const int32_t nf = forest->n_features;
    const int64_t chunk_rows = in_hbm ? n : std::min<int64_t>(n, std::max<int64_t>(1, kSeedChunkBytes / (4 * int64_t(nf))));
    if (!in_hbm) {
        DS_TRY(staged.allocate(static_cast<size_t>(chunk_rows) * nf));
    }
    const size_t lds = static_cast<size_t>(kRowThreads) * (nf | 1) * sizeof(float);
    DS_TRY(ds::allow_dynamic_lds(ds_train_seed_kernel, lds));
    for (int64_t first = 0; first < n; first += chunk_rows) {
        const int64_t here = std::min(chunk_rows, n - first);
        if (!in_hbm)   // after the kernel of the chunk before, in stream order
            DS_HIP(hipMemcpyAsync(staged.ptr, rows + first * nf, sizeof(float) * here * nf, hipMemcpyHostToDevice, stream));
        const SeedArgs args{forest->view(), in_hbm ? rows : staged.ptr, leafsum + first, here, stride, n_models};
        DS_LAUNCH(ds_train_seed_kernel, dim3(train_row_grid(compute_units, here)), dim3(kRowThreads), lds,
                  stream, args);
    }
    return DS_OK;
}

// ---- one round of either trainer --------------------------------------------------------------------------------------
Option g_train_max_blocks{"max_blocks", 0, INT32_MAX, 0};   // 0: no cap

namespace {

template <bool kFolds, bool kSampled, bool kMonotone>
int enqueue_round(hipStream_t stream, const TrainView &v, const TrainSamplingView &s, int32_t n_active, int32_t depth,
                  int compute_units)
{
    const unsigned models = static_cast<unsigned>(n_active);
    const dim3 rows(train_row_grid(compute_units, v.n), models);
    DS_LAUNCH(ds_train_clear_kernel, dim3(train_row_grid(compute_units, v.hist_stride / 2), models),
              dim3(kRowThreads), 0, stream, v);
    if (kSampled) {   // the feature sets of this tree's levels, before the gradients of the rows drawn for it
        DS_LAUNCH(ds_train_feature_mask_kernel, dim3(models), dim3(kMaskThreads), 0, stream, v, s);
    }
    DS_LAUNCH((ds_train_gradient_kernel<kFolds, kSampled>), rows, dim3(kRowThreads), 0, stream, v, s);
    for (int32_t level = 0; level < depth; ++level) {
        const int32_t n_built = level == 0 ? 1 : 1 << (level - 1);
        const int32_t nodes_per_group = std::min(n_built, kHistSlots);
        const int32_t features_per_group = std::min<int32_t>(v.nf, kHistSlots / nodes_per_group);
        const int32_t feature_groups = (v.nf + features_per_group - 1) / features_per_group;
        const int32_t node_groups = (n_built + nodes_per_group - 1) / nodes_per_group;
        const int64_t groups = int64_t(feature_groups) * node_groups * n_active;
        // about 4 workgroups per CU in all, counted over the models, each over at least 2048 rows: the LDS adds dominate,
        // the flush (<= 8192 global adds per workgroup) stays a small part
        const unsigned chunks = grid_cap(std::min<int64_t>((v.n + 2047) / 2048, (int64_t(compute_units) * 4 + groups - 1) / groups),
                                         g_train_max_blocks.get());
        DS_LAUNCH((ds_train_histogram_kernel<kFolds, kSampled>),
                  dim3(chunks, feature_groups * node_groups, models), dim3(kHistThreads),
                  0, stream, v, level, n_built, nodes_per_group, features_per_group, feature_groups);
        DS_LAUNCH((ds_train_split_feature_kernel<kSampled, kMonotone>), dim3(1u << level, v.nf, models),
                  dim3(256), 0, stream, v, s, level);
        DS_LAUNCH(ds_train_split_kernel<kMonotone>, dim3(((1u << level) + 63) / 64, models), dim3(64), 0,
                  stream, v, level);
        DS_LAUNCH(ds_train_partition_kernel, rows, dim3(kRowThreads), 0, stream, v, level);
    }
    return DS_OK;
}

}  // namespace

unsigned train_row_grid(int compute_units, int64_t items)
{
    return grid_cap(std::min<int64_t>((items + kRowThreads - 1) / kRowThreads, int64_t(compute_units) * 8),
                    g_train_max_blocks.get());
}

int train_round_enqueue(hipStream_t stream, const TrainView &v, const TrainSamplingView *sampling, int32_t n_active,
                        int32_t depth, bool folds, int compute_units)
{
    const TrainSamplingView none{};
    if (v.monotone != nullptr) {   // the kMonotone forms of the two split kernels; every other kernel is the same one
        if (sampling != nullptr)
            return folds ? enqueue_round<true, true, true>(stream, v, *sampling, n_active, depth, compute_units)
                         : enqueue_round<false, true, true>(stream, v, *sampling, n_active, depth, compute_units);
        return folds ? enqueue_round<true, false, true>(stream, v, none, n_active, depth, compute_units)
                     : enqueue_round<false, false, true>(stream, v, none, n_active, depth, compute_units);
    }
    if (sampling != nullptr)
        return folds ? enqueue_round<true, true, false>(stream, v, *sampling, n_active, depth, compute_units)
                     : enqueue_round<false, true, false>(stream, v, *sampling, n_active, depth, compute_units);
    return folds ? enqueue_round<true, false, false>(stream, v, none, n_active, depth, compute_units)
                 : enqueue_round<false, false, false>(stream, v, none, n_active, depth, compute_units);
}

int train_check_monotone(const char *who, const int8_t *constraints, int32_t n_features, bool *any)
{
    *any = false;
    for (int32_t f = 0; f < n_features; ++f) {
        DS_REQUIRE(constraints[f] >= -1 && constraints[f] <= 1, "%s: constraint %d of feature %d is not -1, 0 or 1", who,
                   constraints[f], f);
        *any = *any || constraints[f] != 0;
    }
    return DS_OK;
}

}  // namespace ds

struct ds_trainer {
    int device = 0;
    int64_t n = 0, n_eval = 0;
    int32_t nf = 0;
    ds::TrainParams params{};
    bool has_labels = false, seeded = false;      // seeded: ds_trainer_seed has started the margins from a forest
    bool weighted = false;                        // ds_trainer_set_weights has been accepted
    bool constrained = false;                     // ds_trainer_set_monotone has been accepted (all zeros too)
    ds::DeviceBuffer<int8_t> monotone;            // ds_trainer_set_monotone with a non-zero entry: int8[nf] and
    ds::DeviceBuffer<double> bounds;              // double[slots][2], the weight bounds of every heap slot
    int64_t rounds = 0;
    int32_t tree_base = 0;                        // the trees of that forest: the number of this trainer's first tree
    hipStream_t stream = nullptr;
    ds::DeviceBuffer<uint8_t> bins, eval_bins;
    ds::DeviceBuffer<float> labels, eval_labels, leafsum, eval_leafsum, probabilities, cuts;
    ds::DeviceBuffer<float> weights;              // ds_trainer_set_weights: float[n], 4n more bytes
    ds::DeviceBuffer<int32_t> cut_offsets, node_of, counts;
    ds::DeviceBuffer<long long> gh, hist;
    ds::DeviceBuffer<ds::Node> nodes;
    ds::DeviceBuffer<ds::Candidate> candidates;   // [2^(max_depth - 1)][nf]: the best split per (node, feature)
    ds::DeviceBuffer<unsigned long long> error;
    ds::TrainView view{};                         // of this one model (`only`), strides = the array sizes, no folds
    bool sampled = false;                         // ds_trainer_set_sampling with a fraction below 1
    ds::DeviceBuffer<uint8_t> masks;              // [kTrainMaxDepth][kTrainFeaturesMax]: the feature sets of the round
    ds::TrainSamplingView sampling_view{};
    std::vector<int32_t> host_offsets;
    ds::Node *pinned_nodes = nullptr;
    unsigned long long *pinned_error = nullptr;
    int compute_units = 256;
    // per-round metrics (ds_trainer_set_metrics): column 0 = the training set, column 1 = the evaluation set
    uint32_t metric_flags = 0;
    ds::DeviceBuffer<int32_t> metric_rows;                  // per set: its negative rows, then its positive rows
    ds::DeviceBuffer<ds::MetricColumn> metric_columns;      // [2]
    ds::DeviceBuffer<unsigned long long> metric_counters;   // [2][kMetricCounters]
    ds::MetricScratch metric_scratch;                       // sized for the set with more negatives
    ds::MetricColumn metric_host[2]{};
    unsigned long long *pinned_metrics = nullptr;
    int64_t metric_cache[2][6];
    ~ds_trainer()
    {
        if (pinned_metrics) (void)hipHostFree(pinned_metrics);
        if (pinned_nodes) (void)hipHostFree(pinned_nodes);
        if (pinned_error) (void)hipHostFree(pinned_error);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

using ds::heap_nodes;

int bin_matrix(ds_trainer *t, const float *rows, bool in_hbm, int64_t n, ds::DeviceBuffer<uint8_t> &out)
{
    return ds::train_bin_matrix(t->stream, t->compute_units, rows, in_hbm, n, t->nf, t->cuts.ptr, t->cut_offsets.ptr, out);
}

using ds::check_free;

// ds_trainer_create (`who`, features on the host) and ds_trainer_create_device (features in HBM)
int create_trainer(const char *who, const float *features, bool in_hbm, int64_t n, int32_t n_features, const float *cuts,
                   const int32_t *cut_offsets, int32_t max_depth, double eta, double min_child_weight, double reg_lambda,
                   double beta, int device, ds_trainer **out)
{
    DS_REQUIRE(out != nullptr, "%s: out is null", who);
    *out = nullptr;
    DS_REQUIRE(features && cuts && cut_offsets, "%s: null input", who);
    DS_TRY(ds::train_check_shape(who, n, n_features));
    DS_REQUIRE(max_depth >= 1 && max_depth <= ds::kTrainMaxDepth, "%s: max_depth = %d out of range [1, %d]", who,
               max_depth, ds::kTrainMaxDepth);
    DS_TRY(ds::train_check_params(who, -1, eta, min_child_weight, reg_lambda, beta));
    DS_TRY(ds::train_check_cuts(who, n_features, cuts, cut_offsets));
    const int64_t hist_bytes = ds::hist_entries(max_depth, n_features) * 8;
    // bins (+ the staged rows of a host matrix), per-row state, histograms
    const int64_t bytes = n * n_features * (in_hbm ? 1 : 5) + n * 36 + hist_bytes;
    DS_HIP(hipSetDevice(device));
    DS_TRY(check_free(bytes, who));
    std::unique_ptr<ds_trainer> owner(new ds_trainer());
    ds_trainer *t = owner.get();
    t->device = device;
    t->n = n;
    t->nf = n_features;
    t->params = ds::TrainParams{max_depth, eta, min_child_weight, reg_lambda, beta};
    t->host_offsets.assign(cut_offsets, cut_offsets + n_features + 1);
    DS_TRY(ds::train_create_setup(who, device, n_features, cuts, cut_offsets, &t->stream, t->cuts, t->cut_offsets,
                                  &t->compute_units));
    DS_TRY(bin_matrix(t, features, in_hbm, n, t->bins));
    DS_TRY(t->labels.allocate(n));
    DS_TRY(t->leafsum.allocate(n));
    DS_TRY(t->probabilities.allocate(n));
    DS_TRY(t->node_of.allocate(n));
    DS_TRY(t->gh.allocate(2 * n));
    DS_TRY(t->hist.allocate(static_cast<size_t>(hist_bytes / 8)));
    DS_TRY(t->counts.allocate(heap_nodes(max_depth)));
    DS_TRY(t->nodes.allocate(heap_nodes(max_depth)));
    DS_TRY(t->candidates.allocate(static_cast<size_t>(ds::candidate_entries(max_depth, n_features))));
    DS_TRY(t->error.allocate(1));
    DS_HIP(hipHostMalloc(reinterpret_cast<void **>(&t->pinned_nodes), sizeof(ds::Node) * heap_nodes(max_depth)));
    DS_HIP(hipHostMalloc(reinterpret_cast<void **>(&t->pinned_error), sizeof(unsigned long long)));
    DS_HIP(hipMemsetAsync(t->leafsum.ptr, 0, sizeof(float) * n, t->stream));
    DS_HIP(hipStreamSynchronize(t->stream));
    t->view = ds::TrainView{t->bins.ptr, t->labels.ptr, nullptr, nullptr, t->cut_offsets.ptr, nullptr, nullptr,
                            t->gh.ptr, t->node_of.ptr, t->leafsum.ptr, t->probabilities.ptr, t->hist.ptr, t->nodes.ptr,
                            t->counts.ptr, t->candidates.ptr, t->error.ptr, n, hist_bytes / 8,
                            ds::candidate_entries(max_depth, n_features), n_features,
                            static_cast<int32_t>(heap_nodes(max_depth)), ds::TrainModel{t->params, -1, 0}};
    *out = owner.release();
    return DS_OK;
}

// ds_trainer_set_eval (`who`, features on the host) and ds_trainer_set_eval_device (features in HBM)
int set_eval(const char *who, ds_trainer *trainer, const float *features, bool in_hbm, const float *labels, int64_t n)
{
    DS_REQUIRE(trainer && features && labels, "%s: null argument", who);
    DS_REQUIRE(n >= 1 && n <= INT32_MAX, "%s: n = %lld rows out of range [1, 2^31)", who, (long long)n);
    DS_REQUIRE(trainer->rounds == 0, "%s: the evaluation set must be given before the first round", who);
    DS_REQUIRE(!trainer->seeded, "%s: the evaluation set must be given before the trainer is seeded", who);
    DS_REQUIRE(trainer->metric_flags == 0, "%s: the evaluation set must be given before ds_trainer_set_metrics", who);
    DS_TRY(ds::train_check_labels(who, "", labels, n));
    DS_HIP(hipSetDevice(trainer->device));
    DS_TRY(check_free(n * trainer->nf * (in_hbm ? 1 : 5) + n * 8, who));
    DS_TRY(bin_matrix(trainer, features, in_hbm, n, trainer->eval_bins));
    DS_TRY(trainer->eval_labels.upload(labels, n));
    DS_TRY(trainer->eval_leafsum.allocate(n));
    DS_HIP(hipMemsetAsync(trainer->eval_leafsum.ptr, 0, sizeof(float) * n, trainer->stream));
    DS_HIP(hipStreamSynchronize(trainer->stream));
    trainer->n_eval = n;
    return DS_OK;
}

// what ds_trainer_seed enqueues: the leaf sums of both sets, then the evaluation set's error at them
int enqueue_seed(ds_trainer *t, const ds_forest *forest, const float *features, const float *eval_features, bool in_hbm,
                 hipStream_t stream, ds::DeviceBuffer<float> &staged, ds::DeviceBuffer<float> &eval_staged)
{
    DS_TRY(ds::train_seed_enqueue(stream, t->compute_units, forest, features, in_hbm, t->n, t->leafsum.ptr, 1, t->n, staged));
    if (t->n_eval == 0) return DS_OK;
    DS_TRY(ds::train_seed_enqueue(stream, t->compute_units, forest, eval_features, in_hbm, t->n_eval,
                                  t->eval_leafsum.ptr, 1, t->n_eval, eval_staged));
    DS_HIP(hipMemsetAsync(t->error.ptr, 0, sizeof(unsigned long long), stream));
    DS_LAUNCH(ds::ds_train_error_kernel, dim3(ds::train_row_grid(t->compute_units, t->n_eval)),
              dim3(ds::kRowThreads), 0, stream, t->eval_leafsum.ptr, t->eval_labels.ptr, t->n_eval,
              ds::kTrainBaseMargin, t->error.ptr);
    DS_HIP(hipMemcpyAsync(t->pinned_error, t->error.ptr, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    return DS_OK;
}

// ds_trainer_seed (`who`, matrices on the host) and ds_trainer_seed_device (matrices in HBM, complete on `stream`)
int seed_trainer(const char *who, ds_trainer *t, const ds_forest *forest, const float *features, const float *eval_features,
                 bool in_hbm, int64_t *initial_error, hipStream_t stream)
{
    DS_REQUIRE(t != nullptr, "%s: trainer is null", who);
    DS_TRY(ds::train_check_seed_forest(who, forest, t->device, t->nf));
    DS_REQUIRE(features != nullptr, "%s: features is null", who);
    DS_REQUIRE(t->has_labels, "%s: no labels (ds_trainer_set_labels)", who);
    DS_REQUIRE((eval_features != nullptr) == (t->n_eval > 0),
               "%s: eval_features goes with the trainer's evaluation set (%lld rows)", who, (long long)t->n_eval);
    DS_REQUIRE(t->rounds == 0, "%s: the trainer must be seeded before the first round", who);
    DS_REQUIRE(!t->seeded, "%s: the trainer is already seeded", who);
    DS_HIP(hipSetDevice(t->device));
    if (!in_hbm) {   // one chunk per set at the most
        stream = t->stream;
        const int64_t rows = t->n + t->n_eval;
        DS_TRY(check_free(std::min(rows * t->nf * 4, 2 * ds::kSeedChunkBytes), who));
    }
    ds::DeviceBuffer<float> staged, eval_staged;
    t->seeded = true;   // whatever happens below: a trainer whose margins may be partly written is not seeded again
    const int status = enqueue_seed(t, forest, features, eval_features, in_hbm, stream, staged, eval_staged);
    const hipError_t synced = hipStreamSynchronize(stream);   // the call's one host sync; the staged chunks live until here
    if (status != DS_OK) return status;
    DS_HIP(synced);
    t->tree_base = forest->n_trees;
    if (initial_error) *initial_error = t->n_eval > 0 ? static_cast<int64_t>(*t->pinned_error) : -1;
    return DS_OK;
}

}  // namespace

extern "C" {

int ds_trainer_create(const float *features, int64_t n, int32_t n_features, const float *cuts,
                      const int32_t *cut_offsets, int32_t max_depth, double eta, double min_child_weight,
                      double reg_lambda, double beta, int device, ds_trainer **out)
{
    return create_trainer("ds_trainer_create", features, false, n, n_features, cuts, cut_offsets, max_depth, eta,
                          min_child_weight, reg_lambda, beta, device, out);
}

int ds_trainer_create_device(const float *d_features, int64_t n, int32_t n_features, const float *cuts,
                             const int32_t *cut_offsets, int32_t max_depth, double eta, double min_child_weight,
                             double reg_lambda, double beta, int device, ds_trainer **out)
{
    return create_trainer("ds_trainer_create_device", d_features, true, n, n_features, cuts, cut_offsets, max_depth, eta,
                          min_child_weight, reg_lambda, beta, device, out);
}

void ds_trainer_destroy(ds_trainer *trainer)
{
    if (!trainer) return;
    (void)hipSetDevice(trainer->device);
    delete trainer;
}

int ds_trainer_set_labels(ds_trainer *trainer, const float *labels)
{
    DS_REQUIRE(trainer && labels, "ds_trainer_set_labels: null argument");
    DS_REQUIRE(trainer->metric_flags == 0, "ds_trainer_set_labels: the labels must be set before ds_trainer_set_metrics");
    DS_TRY(ds::train_check_labels("ds_trainer_set_labels", "", labels, trainer->n));
    DS_HIP(hipSetDevice(trainer->device));
    DS_HIP(hipMemcpyAsync(trainer->labels.ptr, labels, sizeof(float) * trainer->n, hipMemcpyHostToDevice,
                          trainer->stream));
    DS_HIP(hipStreamSynchronize(trainer->stream));
    trainer->has_labels = true;
    return DS_OK;
}

int ds_trainer_set_weights(ds_trainer *trainer, const float *weights)
{
    const char *who = "ds_trainer_set_weights";
    DS_REQUIRE(trainer != nullptr, "%s: trainer is null", who);
    DS_REQUIRE(weights != nullptr, "%s: weights is null", who);
    ds_trainer *t = trainer;
    DS_REQUIRE(t->has_labels, "%s: no labels (ds_trainer_set_labels)", who);
    DS_REQUIRE(t->rounds == 0, "%s: the weights must be set before the first round", who);
    DS_REQUIRE(!t->weighted, "%s: the weights are already set", who);
    DS_TRY(ds::train_check_weights(who, weights, t->n, t->params.beta));
    bool positive = false;
    for (int64_t r = 0; r < t->n && !positive; ++r) positive = weights[r] > 0.f;
    DS_REQUIRE(positive, "%s: the total weight of the training rows is 0", who);
    DS_HIP(hipSetDevice(t->device));
    DS_TRY(check_free(t->n * 4, who));
    DS_TRY(t->weights.allocate(static_cast<size_t>(t->n)));
    DS_HIP(hipMemcpyAsync(t->weights.ptr, weights, sizeof(float) * t->n, hipMemcpyHostToDevice, t->stream));
    DS_HIP(hipStreamSynchronize(t->stream));
    t->view.weights = t->weights.ptr;
    t->weighted = true;
    return DS_OK;
}

int ds_trainer_set_monotone(ds_trainer *trainer, const int8_t *constraints)
{
    const char *who = "ds_trainer_set_monotone";
    DS_REQUIRE(trainer != nullptr, "%s: trainer is null", who);
    DS_REQUIRE(constraints != nullptr, "%s: constraints is null", who);
    ds_trainer *t = trainer;
    DS_REQUIRE(t->has_labels, "%s: no labels (ds_trainer_set_labels)", who);
    DS_REQUIRE(t->rounds == 0, "%s: the constraints must be set before the first round", who);
    DS_REQUIRE(!t->constrained, "%s: the constraints are already set", who);
    bool any = false;
    DS_TRY(ds::train_check_monotone(who, constraints, t->nf, &any));
    if (any) {   // all zeros: nothing is allocated and the plain kernels keep running
        DS_HIP(hipSetDevice(t->device));
        const size_t slots = static_cast<size_t>(t->view.slots);
        DS_TRY(t->monotone.allocate(static_cast<size_t>(t->nf)));
        DS_TRY(t->bounds.allocate(2 * slots));
        DS_HIP(hipMemcpyAsync(t->monotone.ptr, constraints, static_cast<size_t>(t->nf), hipMemcpyHostToDevice, t->stream));
        DS_HIP(hipMemsetAsync(t->bounds.ptr, 0, t->bounds.bytes(), t->stream));
        DS_HIP(hipStreamSynchronize(t->stream));
        t->view.monotone = t->monotone.ptr;
        t->view.bounds = t->bounds.ptr;
    }
    t->constrained = true;
    return DS_OK;
}

int ds_trainer_set_eval(ds_trainer *trainer, const float *features, const float *labels, int64_t n)
{
    return set_eval("ds_trainer_set_eval", trainer, features, false, labels, n);
}

int ds_trainer_set_eval_device(ds_trainer *trainer, const float *d_features, const float *labels, int64_t n)
{
    return set_eval("ds_trainer_set_eval_device", trainer, d_features, true, labels, n);
}

int ds_trainer_set_sampling(ds_trainer *trainer, double subsample, double colsample_bytree, double colsample_bylevel,
                            uint64_t sample_seed)
{
    DS_REQUIRE(trainer != nullptr, "ds_trainer_set_sampling: trainer is null");
    ds_trainer *t = trainer;
    const double fractions[3] = {subsample, colsample_bytree, colsample_bylevel};
    DS_TRY(ds::train_check_fractions("ds_trainer_set_sampling", -1, fractions));
    DS_REQUIRE(t->rounds == 0, "ds_trainer_set_sampling: the sampling must be set before the first round");
    DS_TRY(ds::train_check_subsample("ds_trainer_set_sampling", -1, subsample, t->params.reg_lambda));
    const ds::TrainSampling sampling{subsample, colsample_bytree, colsample_bylevel, sample_seed};
    if (sampling.any() && t->masks.ptr == nullptr) {
        DS_HIP(hipSetDevice(t->device));
        DS_TRY(t->masks.allocate(ds::kMaskBytes));
    }
    t->sampling_view = ds::TrainSamplingView{nullptr, nullptr, nullptr, nullptr, t->masks.ptr, 0, sampling, 0};
    t->sampled = sampling.any();   // every fraction 1: the plain kernels, whatever was set before
    return DS_OK;
}

int ds_trainer_seed(ds_trainer *trainer, const ds_forest *forest, const float *features, const float *eval_features,
                    int64_t *initial_error)
{
    return seed_trainer("ds_trainer_seed", trainer, forest, features, eval_features, false, initial_error, nullptr);
}

int ds_trainer_seed_device(ds_trainer *trainer, const ds_forest *forest, const float *d_features,
                           const float *d_eval_features, int64_t *initial_error, void *stream)
{
    return seed_trainer("ds_trainer_seed_device", trainer, forest, d_features, d_eval_features, true, initial_error,
                        static_cast<hipStream_t>(stream));
}

int ds_trainer_set_metrics(ds_trainer *trainer, uint32_t flags)
{
    DS_REQUIRE(trainer != nullptr, "ds_trainer_set_metrics: trainer is null");
    DS_REQUIRE((flags & ~(ds::kMetricAuc | ds::kMetricLogloss)) == 0u, "ds_trainer_set_metrics: unknown bits in flags = %u",
               flags);
    DS_REQUIRE(trainer->rounds == 0, "ds_trainer_set_metrics: the metrics must be set before the first round");
    ds_trainer *t = trainer;
    for (int set = 0; set < 2; ++set)
        for (int i = 0; i < 6; ++i) t->metric_cache[set][i] = -1;
    if (flags == 0u) {
        t->metric_flags = 0u;
        return DS_OK;
    }
    DS_REQUIRE(t->has_labels, "ds_trainer_set_metrics: no labels (ds_trainer_set_labels)");
    DS_HIP(hipSetDevice(t->device));
    DS_HIP(hipStreamSynchronize(t->stream));
    // the lists of negative and positive rows of both sets, from the labels the trainer holds
    const int64_t sizes[2] = {t->n, t->n_eval};
    const float *d_labels[2] = {t->labels.ptr, t->eval_labels.ptr};
    const float *d_scores[2] = {t->leafsum.ptr, t->eval_leafsum.ptr};
    std::vector<int32_t> rows(static_cast<size_t>(t->n + t->n_eval));
    std::vector<float> labels;
    int64_t first[2] = {0, t->n}, negatives[2] = {0, 0};
    for (int set = 0; set < 2; ++set) {
        labels.resize(static_cast<size_t>(sizes[set]));
        if (sizes[set] > 0)
            DS_HIP(hipMemcpy(labels.data(), d_labels[set], sizeof(float) * sizes[set], hipMemcpyDeviceToHost));
        for (int64_t r = 0; r < sizes[set]; ++r) negatives[set] += labels[r] == 0.f ? 1 : 0;
        int64_t at_neg = first[set], at_pos = first[set] + negatives[set];
        for (int64_t r = 0; r < sizes[set]; ++r) rows[labels[r] == 0.f ? at_neg++ : at_pos++] = static_cast<int32_t>(r);
    }
    const int64_t n_keys = (flags & ds::kMetricAuc) ? std::max(negatives[0], negatives[1]) : 0;
    DS_TRY(check_free(4 * int64_t(rows.size()) + ds::MetricScratch::bytes(n_keys, 1), "ds_trainer_set_metrics"));
    DS_TRY(t->metric_rows.upload(rows.data(), rows.size()));
    DS_TRY(t->metric_columns.allocate(2));
    DS_TRY(t->metric_counters.allocate(2 * ds::kMetricCounters));
    DS_TRY(t->metric_scratch.allocate(n_keys, 1));
    if (t->pinned_metrics == nullptr)
        DS_HIP(hipHostMalloc(reinterpret_cast<void **>(&t->pinned_metrics), sizeof(unsigned long long) * 2 * ds::kMetricCounters));
    for (int set = 0; set < 2; ++set) {
        const int32_t *list = t->metric_rows.ptr + first[set];
        t->metric_host[set] = ds::MetricColumn{d_scores[set], list, list + negatives[set],
                                               static_cast<int32_t>(negatives[set]),
                                               static_cast<int32_t>(sizes[set] - negatives[set]), ds::kTrainBaseMargin, 0,
                                               t->params.beta};
    }
    DS_HIP(hipMemcpy(t->metric_columns.ptr, t->metric_host, sizeof(t->metric_host), hipMemcpyHostToDevice));
    // on the trainer's own stream: it is non-blocking, so a memset on the null stream is not ordered in front of the rounds
    DS_HIP(hipMemsetAsync(t->metric_counters.ptr, 0, t->metric_counters.bytes(), t->stream));
    DS_HIP(hipStreamSynchronize(t->stream));
    t->metric_flags = flags;
    return DS_OK;
}

int ds_trainer_metrics(ds_trainer *trainer, int64_t out[2][6])
{
    DS_REQUIRE(trainer && out, "ds_trainer_metrics: null argument");
    for (int set = 0; set < 2; ++set)
        for (int i = 0; i < 6; ++i)
            out[set][i] = trainer->metric_flags && trainer->rounds > 0 ? trainer->metric_cache[set][i] : -1;
    return DS_OK;
}

int ds_gather_rows_device(const float *d_src, int32_t n_features, const int64_t *d_rows, int64_t n_rows, int64_t n_src,
                          float *d_dst, void *stream)
{
    DS_REQUIRE(n_features >= 1 && n_features <= ds::kTrainFeaturesMax,
               "ds_gather_rows_device: n_features = %d out of range [1, %d]", n_features, ds::kTrainFeaturesMax);
    DS_REQUIRE(n_rows >= 0 && n_rows <= INT32_MAX, "ds_gather_rows_device: n_rows = %lld out of range [0, 2^31)",
               (long long)n_rows);
    DS_REQUIRE(n_src >= 1 && n_src <= INT32_MAX, "ds_gather_rows_device: n_src = %lld out of range [1, 2^31)",
               (long long)n_src);
    if (n_rows == 0) return DS_OK;
    DS_REQUIRE(d_src && d_rows && d_dst, "ds_gather_rows_device: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ds::DeviceBuffer<int32_t> error;
    DS_TRY(error.allocate(1));
    int32_t errors = 0;
    DS_HIP(hipMemsetAsync(error.ptr, 0, sizeof(int32_t), s));
    const auto grid = [](int64_t items) {
        return dim3(static_cast<unsigned>(std::min<int64_t>((items + ds::kRowThreads - 1) / ds::kRowThreads, 256 * 16)));
    };
    DS_LAUNCH(ds::ds_gather_check_kernel, grid(n_rows), dim3(ds::kRowThreads), 0, s, d_rows, n_rows, n_src,
              error.ptr);
    DS_HIP(hipMemcpyAsync(&errors, error.ptr, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DS_HIP(hipStreamSynchronize(s));
    if (errors != 0) {
        ds::set_error("ds_gather_rows_device: %d row indexes are out of range [0, %lld)", errors, (long long)n_src);
        return DS_E_ARG;
    }
    DS_LAUNCH(ds::ds_gather_rows_kernel, grid(n_rows * n_features), dim3(ds::kRowThreads), 0, s,
              reinterpret_cast<const uint32_t *>(d_src), n_features, d_rows, n_rows, n_src,
              reinterpret_cast<uint32_t *>(d_dst));
    DS_HIP(hipStreamSynchronize(s));
    return DS_OK;
}

int ds_trainer_step(ds_trainer *trainer, int32_t *node_info, float *node_leaf, int64_t *eval_error)
{
    DS_REQUIRE(trainer && node_info && node_leaf, "ds_trainer_step: null argument");
    DS_REQUIRE(trainer->has_labels, "ds_trainer_step: no labels (ds_trainer_set_labels)");
    ds_trainer *t = trainer;
    DS_HIP(hipSetDevice(t->device));
    const int32_t depth = t->params.max_depth;
    hipStream_t stream = t->stream;
    // this tree's number indexes its streams: a seeded trainer counts on from the forest's trees
    if (t->sampled) t->sampling_view.tree = t->tree_base + static_cast<int32_t>(t->rounds);
    DS_TRY(ds::train_round_enqueue(stream, t->view, t->sampled ? &t->sampling_view : nullptr, 1, depth, false, t->compute_units));
    if (t->n_eval > 0) {
        DS_LAUNCH(ds::ds_train_eval_kernel, dim3(ds::train_row_grid(t->compute_units, t->n_eval)),
                  dim3(ds::kRowThreads), 0, stream, t->eval_bins.ptr, t->nodes.ptr, t->n_eval,
                  t->eval_labels.ptr, ds::kTrainBaseMargin, t->eval_leafsum.ptr, t->error.ptr);
    }
    DS_HIP(hipMemcpyAsync(t->pinned_nodes, t->nodes.ptr, t->nodes.bytes(), hipMemcpyDeviceToHost, stream));
    DS_HIP(hipMemcpyAsync(t->pinned_error, t->error.ptr, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    if (t->metric_flags) {   // over the margins the partition and eval kernels have just written
        for (int set = 0; set < (t->n_eval > 0 ? 2 : 1); ++set) {
            const ds::MetricColumn &column = t->metric_host[set];
            DS_TRY(ds::metrics_enqueue(stream, t->compute_units, t->metric_flags, t->metric_columns.ptr + set, nullptr,
                                       1, column.n_neg, column.n_pos, int64_t(column.n_neg) + column.n_pos,
                                       t->metric_scratch, t->metric_counters.ptr + set * ds::kMetricCounters, 0));
        }
        DS_HIP(hipMemcpyAsync(t->pinned_metrics, t->metric_counters.ptr, t->metric_counters.bytes(),
                              hipMemcpyDeviceToHost, stream));
    }
    DS_HIP(hipStreamSynchronize(stream));   // the round's one host sync
    ds::train_unpack_heap(t->pinned_nodes, heap_nodes(depth), node_info, node_leaf);
    if (eval_error) *eval_error = t->n_eval > 0 ? static_cast<int64_t>(*t->pinned_error) : -1;
    if (t->metric_flags)
        for (int set = 0; set < (t->n_eval > 0 ? 2 : 1); ++set)
            ds::metrics_row(t->metric_flags, t->pinned_metrics + set * ds::kMetricCounters, t->metric_host[set].n_neg,
                            t->metric_host[set].n_pos, t->metric_cache[set]);
    ++t->rounds;
    return DS_OK;
}

int ds_trainer_read(ds_trainer *trainer, float *margins, float *probabilities, int64_t *gradients, uint8_t *bins,
                    float *eval_margins)
{
    DS_REQUIRE(trainer != nullptr, "ds_trainer_read: trainer is null");
    DS_REQUIRE(eval_margins == nullptr || trainer->n_eval > 0, "ds_trainer_read: no evaluation set");
    ds_trainer *t = trainer;
    DS_HIP(hipSetDevice(t->device));
    DS_HIP(hipStreamSynchronize(t->stream));
    const size_t n = static_cast<size_t>(t->n);
    if (probabilities) DS_HIP(hipMemcpy(probabilities, t->probabilities.ptr, sizeof(float) * n, hipMemcpyDeviceToHost));
    if (gradients) DS_HIP(hipMemcpy(gradients, t->gh.ptr, sizeof(int64_t) * 2 * n, hipMemcpyDeviceToHost));
    if (bins) DS_HIP(hipMemcpy(bins, t->bins.ptr, n * t->nf, hipMemcpyDeviceToHost));
    auto add_base = [&](float *out, const float *d_sum, size_t count) -> int {
        DS_HIP(hipMemcpy(out, d_sum, sizeof(float) * count, hipMemcpyDeviceToHost));
        for (size_t r = 0; r < count; ++r) out[r] = ds::kTrainBaseMargin + out[r];   // ds_forest.hip: base + sum of leaves
        return DS_OK;
    };
    if (margins) {
        DS_TRY(add_base(margins, t->leafsum.ptr, n));
    }
    if (eval_margins) {
        DS_TRY(add_base(eval_margins, t->eval_leafsum.ptr, static_cast<size_t>(t->n_eval)));
    }
    return DS_OK;
}

}  // extern "C"
