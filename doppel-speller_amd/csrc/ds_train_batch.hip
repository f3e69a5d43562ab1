// Batched training for cross-validation and parameter search ("Cross-validation and tuning"):
// M boosters over ONE binned matrix, each with its own parameters and its own held-out fold, grown by the kernels and
// the launcher of ds_train.hip (train_round_enqueue over a TrainView, ds_train.h) with the model as a further grid
// dimension.  One round launches each kernel once for all active models and syncs with the host once.  This file holds
// what only the batch has: the folds, the active list, the held-out error and the per-model sampling and metrics.
//
// Shared by the models of a batch:
//   bins      uint8[nf][n]   as ds_train.hip's, from the cuts of the whole matrix
//   labels    float[n]
//   fold      uint8[n]       0 .. K-1
//   models    TrainModel[M]  parameters and the held-out fold h (-1: none) of every model
// Per model m, at m * the array's stride: gh int64[n][2], node_of int32[n], leafsum float[n], probabilities float[n],
//   hist int64[2^D - 1][nf][256][2], nodes Node[2^(D+1) - 1], counts int32[2^(D+1) - 1], candidates [2^(D-1)][nf] and
//   error uint64, D = the largest max_depth of the batch.
// Row r trains in model m iff fold[r] != h_m.  A held-out row carries (g, h) = (0, 0), is skipped by the histogram
// kernel, is routed through every new tree like any row, and counts in the model's error after the round.
//
// Subsampling (ds_trainer_batch_set_sampling; DESIGN.md section 9, "Subsampling"): every model has its own fractions,
// seed and tree count.  Once a model of the batch samples, a step launches the kSampled kernels for ALL active
// models; a model whose fractions are 1 draws nothing in them and grows the trees of the plain ones.  Added state:
//   sampling     TrainSampling[M]   trees int32[M]: the trees every model has grown before this step (host -> device
//                                   with the active list, no further sync)
//   masks        uint8[M][kTrainMaxDepth][kTrainFeaturesMax]  the feature sets of the round, one workgroup per model
//   held_before  uint32[slots][ceil(n / 64)]  rows of a held-out fold before row 64 w, one slot per fold that a model
//                                   with subsample < 1 holds out: the draw of row r is indexed by r's number among the
//                                   model's training rows, so that the model is ds_trainer's on those rows alone
//
// Metrics (ds_trainer_batch_set_metrics; DESIGN.md section 9, "Metrics"): AUC and log loss of every active model over the
// rows of its held-out fold, by the kernels of ds_metrics.hip with the active models in blockIdx.y.  Added state:
//   metric_rows     int32[<= n]       per fold that a model holds out: its negative rows, then its positive rows
//   metric_columns  MetricColumn[M]   model m's margins with the lists of its held-out fold
//   metric_scratch                    two key buffers and a count table per model, for the largest fold's negatives
//   metric_counters uint64[M][6]      copied back whole with the step's other results; the host keeps the active models'
//
// Sample weights (ds_trainer_batch_set_weights; DESIGN.md section 9, "Sample weights"): ONE float[n] shared by the models,
// like the labels (TrainView::weights, stride 0); the gradient kernel multiplies a row's (g, h) by its weight, and a
// held-out row stays (0, 0) whatever it weighs.  The entry checks on the host that every model's training rows weigh
// something and refuses by the model's number.  4n more bytes, outside ds_trainer_batch_bytes' formula.
//
// Monotone constraints (ds_trainer_batch_set_monotone; DESIGN.md section 9, "Monotone constraints"): ONE int8[nf] shared by
// the models (TrainView::monotone, stride 0) and per model the weight bounds of its heap slots (TrainView::bounds, stride
// 2 * slots); a step then launches the kMonotone forms of the two split kernels.  16 * slots * n_models + nf more bytes,
// outside ds_trainer_batch_bytes' formula.
//
// Continuing from a model (ds_trainer_batch_seed; DESIGN.md section 9, "Continuing from a model"): before the first step
// ds_train_seed_kernel walks a forest over the RAW matrix once per row and writes the leaf sum into all M leafsum columns;
// ds_batch_error_kernel then gives every model's held-out error at those margins, and every model's tree count starts at
// the forest's.
#include "ds_launch.h"
#include "ds_forest.h"
#include "ds_metrics.h"
#include "ds_train.h"

namespace ds {

constexpr int kBatchModelsMax = 256;
constexpr int kBatchFoldsMax = 255;

// ---- held-out error: ds_train_eval_kernel's rule over the rows of the model's held-out fold, at the margins that the
// partition kernel has just updated
__global__ __launch_bounds__(kRowThreads) void ds_batch_error_kernel(TrainView v)
{
    __shared__ unsigned long long s_error;
    const int32_t m = v.active[blockIdx.y];
    const int32_t held_out = v.models[m].held_out;
    if (held_out < 0) return;
    if (threadIdx.x == 0) s_error = 0;
    __syncthreads();
    const float *leafsum = v.leafsum + m * v.n;
    unsigned long long mine = 0;
    for (int64_t r = blockIdx.x * static_cast<int64_t>(kRowThreads) + threadIdx.x; r < v.n;
         r += static_cast<int64_t>(gridDim.x) * kRowThreads)
        if (static_cast<int32_t>(v.fold[r]) == held_out) mine += train_row_error(kTrainBaseMargin + leafsum[r], v.labels[r]);
    if (mine) atomicAdd(&s_error, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_error) atomicAdd(v.errors + m, s_error);
}

}  // namespace ds

struct ds_trainer_batch {
    int device = 0;
    int64_t n = 0;
    int32_t nf = 0, n_models = 0, max_depth = 0, slots = 0;
    std::vector<ds::TrainModel> models;
    hipStream_t stream = nullptr;
    ds::DeviceBuffer<uint8_t> bins, fold;
    ds::DeviceBuffer<float> labels, leafsum, probabilities, cuts;
    ds::DeviceBuffer<float> weights;           // ds_trainer_batch_set_weights: float[n] shared by the models, 4n more bytes
    bool weighted = false;
    bool constrained = false;                  // ds_trainer_batch_set_monotone has been accepted (all zeros too)
    ds::DeviceBuffer<int8_t> monotone;         // with a non-zero entry: int8[nf] shared by the models, and the weight
    ds::DeviceBuffer<double> bounds;           // bounds double[n_models][slots][2]
    ds::DeviceBuffer<int32_t> cut_offsets, node_of, counts, active;
    ds::DeviceBuffer<long long> gh, hist;
    ds::DeviceBuffer<ds::Node> nodes;
    ds::DeviceBuffer<ds::Candidate> candidates;
    ds::DeviceBuffer<unsigned long long> errors;
    ds::DeviceBuffer<ds::TrainModel> d_models;
    ds::Node *pinned_nodes = nullptr;          // [n_models][slots]
    unsigned long long *pinned_errors = nullptr;
    int32_t *pinned_active = nullptr;
    ds::TrainView view{};
    int compute_units = 256;
    // subsampling (ds_trainer_batch_set_sampling)
    bool stepped = false, sampled = false, seeded = false;
    std::vector<int32_t> tree_count;           // the trees every model has grown
    ds::DeviceBuffer<ds::TrainSampling> d_sampling;
    ds::DeviceBuffer<int32_t> d_trees, d_held_slot;
    ds::DeviceBuffer<uint32_t> d_held_before;
    ds::DeviceBuffer<uint8_t> masks;
    int32_t *pinned_trees = nullptr;
    ds::TrainSamplingView sampling_view{};
    // metrics (ds_trainer_batch_set_metrics)
    uint32_t metric_flags = 0;
    ds::DeviceBuffer<int32_t> metric_rows;
    ds::DeviceBuffer<ds::MetricColumn> metric_columns;
    ds::DeviceBuffer<unsigned long long> metric_counters;
    ds::MetricScratch metric_scratch;
    std::vector<ds::MetricColumn> metric_host;
    std::vector<int64_t> metric_cache;         // [n_models][6], -1 until a model's first step
    int64_t metric_keys = 0, metric_pos = 0, metric_fold_rows = 0;   // the largest over the held-out folds
    unsigned long long *pinned_metrics = nullptr;
    ~ds_trainer_batch()
    {
        if (pinned_metrics) (void)hipHostFree(pinned_metrics);
        if (pinned_trees) (void)hipHostFree(pinned_trees);
        if (pinned_nodes) (void)hipHostFree(pinned_nodes);
        if (pinned_errors) (void)hipHostFree(pinned_errors);
        if (pinned_active) (void)hipHostFree(pinned_active);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

using ds::candidate_entries;
using ds::heap_nodes;
using ds::hist_entries;

bool ranges_ok(int64_t n, int32_t n_features, int32_t n_models, int32_t max_depth)
{
    return n >= 1 && n <= INT32_MAX && n_features >= 1 && n_features <= ds::kTrainFeaturesMax && n_models >= 1 &&
           n_models <= ds::kBatchModelsMax && max_depth >= 1 && max_depth <= ds::kTrainMaxDepth;
}

int create_batch(const char *who, const float *features, bool in_hbm, int64_t n, int32_t n_features, const float *cuts,
                 const int32_t *cut_offsets, const float *labels, const uint8_t *fold, int32_t n_folds, int32_t n_models,
                 const double *params, const int32_t *held_out, int device, ds_trainer_batch **out)
{
    DS_REQUIRE(out != nullptr, "%s: out is null", who);
    *out = nullptr;
    DS_REQUIRE(features != nullptr, "%s: features is null", who);
    DS_REQUIRE(cuts != nullptr, "%s: cuts is null", who);
    DS_REQUIRE(cut_offsets != nullptr, "%s: cut_offsets is null", who);
    DS_REQUIRE(labels != nullptr, "%s: labels is null", who);
    DS_REQUIRE(fold != nullptr, "%s: fold is null", who);
    DS_REQUIRE(params != nullptr, "%s: params is null", who);
    DS_REQUIRE(held_out != nullptr, "%s: held_out is null", who);
    DS_TRY(ds::train_check_shape(who, n, n_features));
    DS_REQUIRE(n_models >= 1 && n_models <= ds::kBatchModelsMax, "%s: n_models = %d out of range [1, %d]", who, n_models,
               ds::kBatchModelsMax);
    DS_REQUIRE(n_folds >= 1 && n_folds <= ds::kBatchFoldsMax, "%s: n_folds = %d out of range [1, %d]", who, n_folds,
               ds::kBatchFoldsMax);
    std::vector<ds::TrainModel> models(n_models);
    int32_t depth = 1;
    for (int32_t m = 0; m < n_models; ++m) {
        const double *p = params + 5 * m;
        DS_REQUIRE(p[0] >= 1 && p[0] <= ds::kTrainMaxDepth && p[0] == static_cast<double>(static_cast<int32_t>(p[0])),
                   "%s: params of model %d: max_depth = %g is not an integer in [1, %d]", who, m, p[0],
                   ds::kTrainMaxDepth);
        DS_TRY(ds::train_check_params(who, m, p[1], p[2], p[3], p[4]));
        DS_REQUIRE(held_out[m] >= -1 && held_out[m] < n_folds, "%s: held_out[%d] = %d out of range [-1, %d)", who, m,
                   held_out[m], n_folds);
        models[m] = ds::TrainModel{ds::TrainParams{static_cast<int32_t>(p[0]), p[1], p[2], p[3], p[4]}, held_out[m], 0};
        depth = std::max(depth, models[m].params.max_depth);
    }
    DS_TRY(ds::train_check_cuts(who, n_features, cuts, cut_offsets));
    DS_TRY(ds::train_check_labels(who, "labels: ", labels, n));
    for (int64_t r = 0; r < n; ++r)
        DS_REQUIRE(fold[r] < n_folds, "%s: fold[%lld] = %d is not below n_folds = %d", who, (long long)r, fold[r],
                   n_folds);
    const int64_t bytes = ds_trainer_batch_bytes(n, n_features, n_models, depth) + (in_hbm ? 0 : n * n_features * 4);
    DS_HIP(hipSetDevice(device));
    DS_TRY(ds::check_free(bytes, who));
    std::unique_ptr<ds_trainer_batch> owner(new ds_trainer_batch());
    ds_trainer_batch *b = owner.get();
    b->device = device;
    b->n = n;
    b->nf = n_features;
    b->n_models = n_models;
    b->max_depth = depth;
    b->slots = static_cast<int32_t>(heap_nodes(depth));
    b->models = models;
    b->tree_count.assign(n_models, 0);
    const size_t M = static_cast<size_t>(n_models), rows = static_cast<size_t>(n);
    DS_TRY(ds::train_create_setup(who, device, n_features, cuts, cut_offsets, &b->stream, b->cuts, b->cut_offsets,
                                  &b->compute_units));
    DS_TRY(ds::train_bin_matrix(b->stream, b->compute_units, features, in_hbm, n, n_features, b->cuts.ptr,
                                b->cut_offsets.ptr, b->bins));
    DS_TRY(b->labels.upload(labels, rows));
    DS_TRY(b->fold.upload(fold, rows));
    DS_TRY(b->d_models.upload(models.data(), M));
    DS_TRY(b->active.allocate(M));
    DS_TRY(b->leafsum.allocate(M * rows));
    DS_TRY(b->probabilities.allocate(M * rows));
    DS_TRY(b->node_of.allocate(M * rows));
    DS_TRY(b->gh.allocate(2 * M * rows));
    DS_TRY(b->hist.allocate(M * static_cast<size_t>(hist_entries(depth, n_features))));
    DS_TRY(b->counts.allocate(M * b->slots));
    DS_TRY(b->nodes.allocate(M * b->slots));
    DS_TRY(b->candidates.allocate(M * static_cast<size_t>(candidate_entries(depth, n_features))));
    DS_TRY(b->errors.allocate(M));
    DS_HIP(hipHostMalloc(reinterpret_cast<void **>(&b->pinned_nodes), sizeof(ds::Node) * M * b->slots));
    DS_HIP(hipHostMalloc(reinterpret_cast<void **>(&b->pinned_errors), sizeof(unsigned long long) * M));
    DS_HIP(hipHostMalloc(reinterpret_cast<void **>(&b->pinned_active), sizeof(int32_t) * M));
    // every per-row array starts defined: the read-back of a model that has not stepped yet returns zeros
    DS_HIP(hipMemsetAsync(b->leafsum.ptr, 0, b->leafsum.bytes(), b->stream));
    DS_HIP(hipMemsetAsync(b->probabilities.ptr, 0, b->probabilities.bytes(), b->stream));
    DS_HIP(hipMemsetAsync(b->gh.ptr, 0, b->gh.bytes(), b->stream));
    DS_HIP(hipStreamSynchronize(b->stream));
    b->view = ds::TrainView{b->bins.ptr, b->labels.ptr, nullptr, b->fold.ptr, b->cut_offsets.ptr, b->d_models.ptr, b->active.ptr,
                            b->gh.ptr, b->node_of.ptr, b->leafsum.ptr, b->probabilities.ptr, b->hist.ptr, b->nodes.ptr,
                            b->counts.ptr, b->candidates.ptr, b->errors.ptr, n, hist_entries(depth, n_features),
                            candidate_entries(depth, n_features), n_features, b->slots};
    *out = owner.release();
    return DS_OK;
}

// what ds_trainer_batch_seed enqueues: the leaf sums of every model, then every model's held-out error at them
int enqueue_seed(ds_trainer_batch *b, const ds_forest *forest, const float *features, bool in_hbm, hipStream_t stream,
                 ds::DeviceBuffer<float> &staged)
{
    DS_TRY(ds::train_seed_enqueue(stream, b->compute_units, forest, features, in_hbm, b->n, b->leafsum.ptr, b->n_models,
                                  b->n, staged));
    for (int32_t m = 0; m < b->n_models; ++m) b->pinned_active[m] = m;   // the error kernel reads its models from here
    DS_HIP(hipMemcpyAsync(b->active.ptr, b->pinned_active, sizeof(int32_t) * b->n_models, hipMemcpyHostToDevice, stream));
    DS_HIP(hipMemsetAsync(b->errors.ptr, 0, b->errors.bytes(), stream));
    DS_LAUNCH(ds::ds_batch_error_kernel,
              dim3(ds::train_row_grid(b->compute_units, b->n), static_cast<unsigned>(b->n_models)),
              dim3(ds::kRowThreads), 0, stream, b->view);
    DS_HIP(hipMemcpyAsync(b->pinned_errors, b->errors.ptr, b->errors.bytes(), hipMemcpyDeviceToHost, stream));
    return DS_OK;
}

// ds_trainer_batch_seed (`who`, the matrix on the host) and ds_trainer_batch_seed_device (in HBM, complete on `stream`)
int seed_batch(const char *who, ds_trainer_batch *b, const ds_forest *forest, const float *features, bool in_hbm,
               int64_t *initial_errors, hipStream_t stream)
{
    DS_REQUIRE(b != nullptr, "%s: batch is null", who);
    DS_TRY(ds::train_check_seed_forest(who, forest, b->device, b->nf));
    DS_REQUIRE(features != nullptr, "%s: features is null", who);
    DS_REQUIRE(!b->stepped, "%s: the batch must be seeded before the first step", who);
    DS_REQUIRE(!b->seeded, "%s: the batch is already seeded", who);
    DS_HIP(hipSetDevice(b->device));
    if (!in_hbm) {
        stream = b->stream;
        DS_TRY(ds::check_free(std::min(b->n * b->nf * 4, ds::kSeedChunkBytes), who));
    }
    ds::DeviceBuffer<float> staged;
    b->seeded = true;   // whatever happens below: a batch whose margins may be partly written is not seeded again
    const int status = enqueue_seed(b, forest, features, in_hbm, stream, staged);
    const hipError_t synced = hipStreamSynchronize(stream);   // the call's one host sync; the staged chunk lives until here
    if (status != DS_OK) return status;
    DS_HIP(synced);
    b->tree_count.assign(b->n_models, forest->n_trees);   // every model's first tree has the forest's count as its number
    if (initial_errors)
        for (int32_t m = 0; m < b->n_models; ++m)
            initial_errors[m] = b->models[m].held_out >= 0 ? static_cast<int64_t>(b->pinned_errors[m]) : -1;
    return DS_OK;
}

}  // namespace

extern "C" {

int64_t ds_trainer_batch_bytes(int64_t n, int32_t n_features, int32_t n_models, int32_t max_depth)
{
    if (!ranges_ok(n, n_features, n_models, max_depth)) return -1;
    const int64_t per_model = n * 28 + hist_entries(max_depth, n_features) * 8 +
                              heap_nodes(max_depth) * int64_t(sizeof(ds::Node) + 4) +
                              candidate_entries(max_depth, n_features) * int64_t(sizeof(ds::Candidate)) +
                              int64_t(sizeof(ds::TrainModel)) + 12;
    return n * n_features + n * 5 + per_model * n_models;
}

int ds_trainer_batch_create(const float *features, int64_t n, int32_t n_features, const float *cuts,
                            const int32_t *cut_offsets, const float *labels, const uint8_t *fold, int32_t n_folds,
                            int32_t n_models, const double *params, const int32_t *held_out, int device,
                            ds_trainer_batch **out)
{
    return create_batch("ds_trainer_batch_create", features, false, n, n_features, cuts, cut_offsets, labels, fold,
                        n_folds, n_models, params, held_out, device, out);
}

int ds_trainer_batch_create_device(const float *d_features, int64_t n, int32_t n_features, const float *cuts,
                                   const int32_t *cut_offsets, const float *labels, const uint8_t *fold, int32_t n_folds,
                                   int32_t n_models, const double *params, const int32_t *held_out, int device,
                                   ds_trainer_batch **out)
{
    return create_batch("ds_trainer_batch_create_device", d_features, true, n, n_features, cuts, cut_offsets, labels,
                        fold, n_folds, n_models, params, held_out, device, out);
}

void ds_trainer_batch_destroy(ds_trainer_batch *batch)
{
    if (!batch) return;
    (void)hipSetDevice(batch->device);
    delete batch;
}

int ds_trainer_batch_option(const char *name, int64_t value)
{
    ds::Option *const table[] = {&ds::g_train_max_blocks};
    return ds::set_option("ds_trainer_batch_option", table, name, value);
}

int ds_trainer_batch_set_sampling(ds_trainer_batch *batch, const double *fractions, const uint64_t *sample_seeds)
{
    DS_REQUIRE(batch != nullptr, "ds_trainer_batch_set_sampling: batch is null");
    DS_REQUIRE(fractions != nullptr, "ds_trainer_batch_set_sampling: fractions is null");
    DS_REQUIRE(sample_seeds != nullptr, "ds_trainer_batch_set_sampling: sample_seeds is null");
    ds_trainer_batch *b = batch;
    std::vector<ds::TrainSampling> sampling(b->n_models);
    std::vector<int32_t> held_slot(b->n_models, -1), slot_of_fold(ds::kBatchFoldsMax, -1), slot_folds;
    bool any = false;
    for (int32_t m = 0; m < b->n_models; ++m) {
        const double *f = fractions + 3 * m;
        DS_TRY(ds::train_check_fractions("ds_trainer_batch_set_sampling", m, f));
        DS_TRY(ds::train_check_subsample("ds_trainer_batch_set_sampling", m, f[0], b->models[m].params.reg_lambda));
        sampling[m] = ds::TrainSampling{f[0], f[1], f[2], sample_seeds[m]};
        any = any || sampling[m].any();
        const int32_t held_out = b->models[m].held_out;
        if (f[0] < 1 && held_out >= 0) {
            if (slot_of_fold[held_out] < 0) {
                slot_of_fold[held_out] = static_cast<int32_t>(slot_folds.size());
                slot_folds.push_back(held_out);
            }
            held_slot[m] = slot_of_fold[held_out];
        }
    }
    DS_REQUIRE(!b->stepped, "ds_trainer_batch_set_sampling: the sampling must be set before the first step");
    if (!any) {   // every fraction is 1: the plain kernels, whatever was set before
        b->sampled = false;
        return DS_OK;
    }
    DS_HIP(hipSetDevice(b->device));
    const size_t M = static_cast<size_t>(b->n_models), waves = static_cast<size_t>((b->n + 63) / 64);
    std::vector<uint32_t> held_before(std::max<size_t>(1, slot_folds.size() * waves), 0u);
    if (!slot_folds.empty()) {   // rows of every wanted fold before each 64th row, from the folds the batch holds
        std::vector<uint8_t> fold(static_cast<size_t>(b->n));
        DS_HIP(hipMemcpy(fold.data(), b->fold.ptr, fold.size(), hipMemcpyDeviceToHost));
        std::vector<uint32_t> seen(ds::kBatchFoldsMax + 1, 0u);
        for (size_t r = 0; r < fold.size(); ++r) {
            if ((r & 63) == 0)
                for (size_t slot = 0; slot < slot_folds.size(); ++slot)
                    held_before[slot * waves + (r >> 6)] = seen[slot_folds[slot]];
            ++seen[fold[r]];
        }
    }
    DS_TRY(b->d_sampling.upload(sampling.data(), M));
    DS_TRY(b->d_held_slot.upload(held_slot.data(), M));
    DS_TRY(b->d_held_before.upload(held_before.data(), held_before.size()));
    if (b->d_trees.ptr == nullptr) DS_TRY(b->d_trees.allocate(M));
    if (b->masks.ptr == nullptr) DS_TRY(b->masks.allocate(M * ds::kMaskBytes));
    if (b->pinned_trees == nullptr)
        DS_HIP(hipHostMalloc(reinterpret_cast<void **>(&b->pinned_trees), sizeof(int32_t) * M));
    b->sampling_view = ds::TrainSamplingView{b->d_sampling.ptr, b->d_trees.ptr, b->d_held_before.ptr, b->d_held_slot.ptr,
                                             b->masks.ptr, static_cast<int64_t>(waves)};
    b->sampled = true;
    return DS_OK;
}

int ds_trainer_batch_set_weights(ds_trainer_batch *batch, const float *weights)
{
    const char *who = "ds_trainer_batch_set_weights";
    DS_REQUIRE(batch != nullptr, "%s: batch is null", who);
    DS_REQUIRE(weights != nullptr, "%s: weights is null", who);
    ds_trainer_batch *b = batch;
    DS_REQUIRE(!b->stepped, "%s: the weights must be set before the first step", who);
    DS_REQUIRE(!b->weighted, "%s: the weights are already set", who);
    double beta = 0.0;
    for (const ds::TrainModel &model : b->models) beta = std::max(beta, model.params.beta);
    DS_TRY(ds::train_check_weights(who, weights, b->n, beta));
    DS_HIP(hipSetDevice(b->device));
    // every model's training rows must weigh something: whether a fold (slot 0: any fold) has a row of positive weight
    std::vector<uint8_t> fold(static_cast<size_t>(b->n)), positive(ds::kBatchFoldsMax + 1, 0);
    DS_HIP(hipMemcpy(fold.data(), b->fold.ptr, fold.size(), hipMemcpyDeviceToHost));
    int32_t positive_folds = 0;
    for (int64_t r = 0; r < b->n; ++r)
        if (weights[r] > 0.f && !positive[fold[r]]) {
            positive[fold[r]] = 1;
            ++positive_folds;
        }
    for (int32_t m = 0; m < b->n_models; ++m) {
        const int32_t held_out = b->models[m].held_out;
        DS_REQUIRE(positive_folds - (held_out >= 0 && positive[held_out] ? 1 : 0) > 0,
                   "%s: model %d: the total weight of its training rows is 0", who, m);
    }
    DS_TRY(ds::check_free(b->n * 4, who));
    DS_TRY(b->weights.allocate(static_cast<size_t>(b->n)));
    DS_HIP(hipMemcpyAsync(b->weights.ptr, weights, sizeof(float) * b->n, hipMemcpyHostToDevice, b->stream));
    DS_HIP(hipStreamSynchronize(b->stream));
    b->view.weights = b->weights.ptr;
    b->weighted = true;
    return DS_OK;
}

int ds_trainer_batch_set_monotone(ds_trainer_batch *batch, const int8_t *constraints)
{
    const char *who = "ds_trainer_batch_set_monotone";
    DS_REQUIRE(batch != nullptr, "%s: batch is null", who);
    DS_REQUIRE(constraints != nullptr, "%s: constraints is null", who);
    ds_trainer_batch *b = batch;
    DS_REQUIRE(!b->stepped, "%s: the constraints must be set before the first step", who);
    DS_REQUIRE(!b->constrained, "%s: the constraints are already set", who);
    bool any = false;
    DS_TRY(ds::train_check_monotone(who, constraints, b->nf, &any));
    if (any) {   // all zeros: nothing is allocated and the plain kernels keep running
        DS_HIP(hipSetDevice(b->device));
        const size_t pairs = static_cast<size_t>(b->n_models) * b->slots;
        DS_TRY(ds::check_free(int64_t(16 * pairs) + b->nf, who));
        DS_TRY(b->monotone.allocate(static_cast<size_t>(b->nf)));
        DS_TRY(b->bounds.allocate(2 * pairs));
        DS_HIP(hipMemcpyAsync(b->monotone.ptr, constraints, static_cast<size_t>(b->nf), hipMemcpyHostToDevice, b->stream));
        DS_HIP(hipMemsetAsync(b->bounds.ptr, 0, b->bounds.bytes(), b->stream));
        DS_HIP(hipStreamSynchronize(b->stream));
        b->view.monotone = b->monotone.ptr;
        b->view.bounds = b->bounds.ptr;
    }
    b->constrained = true;
    return DS_OK;
}

int ds_trainer_batch_seed(ds_trainer_batch *batch, const ds_forest *forest, const float *features,
                          int64_t *initial_errors)
{
    return seed_batch("ds_trainer_batch_seed", batch, forest, features, false, initial_errors, nullptr);
}

int ds_trainer_batch_seed_device(ds_trainer_batch *batch, const ds_forest *forest, const float *d_features,
                                 int64_t *initial_errors, void *stream)
{
    return seed_batch("ds_trainer_batch_seed_device", batch, forest, d_features, true, initial_errors,
                      static_cast<hipStream_t>(stream));
}

int64_t ds_trainer_batch_metrics_bytes(int64_t n, int32_t n_models, int32_t n_folds)
{
    if (n < 1 || n > INT32_MAX || n_models < 1 || n_models > ds::kBatchModelsMax || n_folds < 1 ||
        n_folds > ds::kBatchFoldsMax)
        return -1;
    const int64_t keys = (n + n_folds - 1) / n_folds;
    return 4 * n + ds::MetricScratch::bytes(keys, n_models) +
           int64_t(n_models) * int64_t(sizeof(ds::MetricColumn) + sizeof(unsigned long long) * ds::kMetricCounters);
}

int ds_trainer_batch_set_metrics(ds_trainer_batch *batch, uint32_t flags)
{
    DS_REQUIRE(batch != nullptr, "ds_trainer_batch_set_metrics: batch is null");
    DS_REQUIRE((flags & ~(ds::kMetricAuc | ds::kMetricLogloss)) == 0u,
               "ds_trainer_batch_set_metrics: unknown bits in flags = %u", flags);
    ds_trainer_batch *b = batch;
    DS_REQUIRE(!b->stepped, "ds_trainer_batch_set_metrics: the metrics must be set before the first step");
    b->metric_cache.assign(static_cast<size_t>(b->n_models) * 6, -1);
    if (flags == 0u) {
        b->metric_flags = 0u;
        return DS_OK;
    }
    DS_HIP(hipSetDevice(b->device));
    // per fold that a model holds out: its negative rows, then its positive rows, in row order
    const size_t rows = static_cast<size_t>(b->n), M = static_cast<size_t>(b->n_models);
    std::vector<uint8_t> fold(rows);
    std::vector<float> labels(rows);
    DS_HIP(hipMemcpy(fold.data(), b->fold.ptr, rows, hipMemcpyDeviceToHost));
    DS_HIP(hipMemcpy(labels.data(), b->labels.ptr, rows * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<int64_t> neg(ds::kBatchFoldsMax + 1, 0), pos(ds::kBatchFoldsMax + 1, 0), first(ds::kBatchFoldsMax + 1, 0);
    std::vector<uint8_t> wanted(ds::kBatchFoldsMax + 1, 0);
    for (const ds::TrainModel &model : b->models)
        if (model.held_out >= 0) wanted[model.held_out] = 1;
    for (size_t r = 0; r < rows; ++r) ++(labels[r] == 0.f ? neg : pos)[fold[r]];
    int64_t listed = 0;
    b->metric_keys = b->metric_pos = b->metric_fold_rows = 0;
    for (int k = 0; k <= ds::kBatchFoldsMax; ++k) {
        if (!wanted[k]) continue;
        first[k] = listed;
        listed += neg[k] + pos[k];
        b->metric_keys = std::max(b->metric_keys, neg[k]);
        b->metric_pos = std::max(b->metric_pos, pos[k]);
        b->metric_fold_rows = std::max(b->metric_fold_rows, neg[k] + pos[k]);
    }
    if (!(flags & ds::kMetricAuc)) b->metric_keys = 0;
    std::vector<int32_t> lists(std::max<size_t>(1, static_cast<size_t>(listed)));
    std::vector<int64_t> at_neg(first), at_pos(first);
    for (int k = 0; k <= ds::kBatchFoldsMax; ++k) at_pos[k] += neg[k];
    for (size_t r = 0; r < rows; ++r)
        if (wanted[fold[r]]) lists[(labels[r] == 0.f ? at_neg : at_pos)[fold[r]]++] = static_cast<int32_t>(r);
    DS_TRY(ds::check_free(4 * listed + ds::MetricScratch::bytes(b->metric_keys, b->n_models), "ds_trainer_batch_set_metrics"));
    DS_TRY(b->metric_rows.upload(lists.data(), lists.size()));
    DS_TRY(b->metric_columns.allocate(M));
    DS_TRY(b->metric_counters.allocate(M * ds::kMetricCounters));
    DS_TRY(b->metric_scratch.allocate(b->metric_keys, b->n_models));
    if (b->pinned_metrics == nullptr)
        DS_HIP(hipHostMalloc(reinterpret_cast<void **>(&b->pinned_metrics), sizeof(unsigned long long) * M * ds::kMetricCounters));
    b->metric_host.assign(M, ds::MetricColumn{});
    for (size_t m = 0; m < M; ++m) {
        const int32_t k = b->models[m].held_out;
        ds::MetricColumn &column = b->metric_host[m];
        column.scores = b->leafsum.ptr + m * rows;
        column.base_margin = ds::kTrainBaseMargin;
        column.beta = b->models[m].params.beta;
        if (k < 0) continue;   // no held-out rows: empty lists, and the host reports -1
        column.neg_rows = b->metric_rows.ptr + first[k];
        column.pos_rows = column.neg_rows + neg[k];
        column.n_neg = static_cast<int32_t>(neg[k]);
        column.n_pos = static_cast<int32_t>(pos[k]);
    }
    DS_HIP(hipMemcpy(b->metric_columns.ptr, b->metric_host.data(), sizeof(ds::MetricColumn) * M, hipMemcpyHostToDevice));
    // on the batch's own stream: it is non-blocking, so a memset on the null stream is not ordered in front of the rounds
    DS_HIP(hipMemsetAsync(b->metric_counters.ptr, 0, b->metric_counters.bytes(), b->stream));
    DS_HIP(hipStreamSynchronize(b->stream));
    b->metric_flags = flags;
    return DS_OK;
}

int ds_trainer_batch_metrics(ds_trainer_batch *batch, int64_t *out)
{
    DS_REQUIRE(batch && out, "ds_trainer_batch_metrics: null argument");
    for (int64_t i = 0; i < int64_t(batch->n_models) * 6; ++i)
        out[i] = batch->metric_flags ? batch->metric_cache[static_cast<size_t>(i)] : -1;
    return DS_OK;
}

int ds_trainer_batch_step(ds_trainer_batch *batch, const uint8_t *active, int32_t *node_info, float *node_leaf,
                          int64_t *errors)
{
    DS_REQUIRE(batch && node_info && node_leaf && errors, "ds_trainer_batch_step: null argument");
    ds_trainer_batch *b = batch;
    int32_t n_active = 0, depth = 0;
    for (int32_t m = 0; m < b->n_models; ++m) {
        if (active && !active[m]) continue;
        b->pinned_active[n_active++] = m;
        depth = std::max(depth, b->models[m].params.max_depth);
    }
    if (n_active == 0) return DS_OK;
    DS_HIP(hipSetDevice(b->device));
    hipStream_t stream = b->stream;
    const ds::TrainView &v = b->view;
    DS_HIP(hipMemcpyAsync(b->active.ptr, b->pinned_active, sizeof(int32_t) * n_active, hipMemcpyHostToDevice, stream));
    if (b->sampled) {   // every model's own tree count indexes its streams, not the steps of the batch
        std::memcpy(b->pinned_trees, b->tree_count.data(), sizeof(int32_t) * b->n_models);
        DS_HIP(hipMemcpyAsync(b->d_trees.ptr, b->pinned_trees, sizeof(int32_t) * b->n_models, hipMemcpyHostToDevice,
                              stream));
    }
    DS_TRY(ds::train_round_enqueue(stream, v, b->sampled ? &b->sampling_view : nullptr, n_active, depth, true, b->compute_units));
    DS_LAUNCH(ds::ds_batch_error_kernel,
              dim3(ds::train_row_grid(b->compute_units, b->n), static_cast<unsigned>(n_active)),
              dim3(ds::kRowThreads), 0, stream, v);
    for (int32_t a = 0; a < n_active;) {   // the active models' heaps only: one copy per run of neighbouring models
        int32_t end = a + 1;
        while (end < n_active && b->pinned_active[end] == b->pinned_active[end - 1] + 1) ++end;
        const size_t first = static_cast<size_t>(b->pinned_active[a]) * b->slots;
        DS_HIP(hipMemcpyAsync(b->pinned_nodes + first, b->nodes.ptr + first, sizeof(ds::Node) * (end - a) * b->slots,
                              hipMemcpyDeviceToHost, stream));
        a = end;
    }
    DS_HIP(hipMemcpyAsync(b->pinned_errors, b->errors.ptr, b->errors.bytes(), hipMemcpyDeviceToHost, stream));
    if (b->metric_flags) {   // over the margins the partition kernels have just written
        DS_TRY(ds::metrics_enqueue(stream, b->compute_units, b->metric_flags, b->metric_columns.ptr, b->active.ptr,
                                   n_active, b->metric_keys, b->metric_pos, b->metric_fold_rows, b->metric_scratch,
                                   b->metric_counters.ptr, ds::g_train_max_blocks.get()));
        DS_HIP(hipMemcpyAsync(b->pinned_metrics, b->metric_counters.ptr, b->metric_counters.bytes(),
                              hipMemcpyDeviceToHost, stream));
    }
    DS_HIP(hipStreamSynchronize(stream));   // the step's one host sync
    b->stepped = true;
    for (int32_t a = 0; a < n_active; ++a) {
        const int64_t m = b->pinned_active[a];
        ++b->tree_count[m];
        ds::train_unpack_heap(b->pinned_nodes + m * b->slots, b->slots, node_info + m * b->slots * 4,
                              node_leaf + m * b->slots);
        errors[m] = b->models[m].held_out >= 0 ? static_cast<int64_t>(b->pinned_errors[m]) : -1;
        if (b->metric_flags && b->models[m].held_out >= 0)
            ds::metrics_row(b->metric_flags, b->pinned_metrics + m * ds::kMetricCounters, b->metric_host[m].n_neg,
                            b->metric_host[m].n_pos, b->metric_cache.data() + m * 6);
    }
    return DS_OK;
}

int ds_trainer_batch_read(ds_trainer_batch *batch, int32_t model, float *margins, float *probabilities,
                          int64_t *gradients, uint8_t *bins)
{
    DS_REQUIRE(batch != nullptr, "ds_trainer_batch_read: batch is null");
    DS_REQUIRE(model >= 0 && model < batch->n_models, "ds_trainer_batch_read: model = %d out of range [0, %d)", model,
               batch->n_models);
    ds_trainer_batch *b = batch;
    DS_HIP(hipSetDevice(b->device));
    DS_HIP(hipStreamSynchronize(b->stream));
    const size_t n = static_cast<size_t>(b->n), m = static_cast<size_t>(model);
    if (probabilities)
        DS_HIP(hipMemcpy(probabilities, b->probabilities.ptr + m * n, sizeof(float) * n, hipMemcpyDeviceToHost));
    if (gradients) DS_HIP(hipMemcpy(gradients, b->gh.ptr + 2 * m * n, sizeof(int64_t) * 2 * n, hipMemcpyDeviceToHost));
    if (bins) DS_HIP(hipMemcpy(bins, b->bins.ptr, n * b->nf, hipMemcpyDeviceToHost));
    if (margins) {
        DS_HIP(hipMemcpy(margins, b->leafsum.ptr + m * n, sizeof(float) * n, hipMemcpyDeviceToHost));
        for (size_t r = 0; r < n; ++r) margins[r] = ds::kTrainBaseMargin + margins[r];
    }
    return DS_OK;
}

}  // extern "C"
