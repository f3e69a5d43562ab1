// The training rule's device and host code shared by the single trainer (ds_train.hip, ds_trainer_*) and the batched
// trainer (ds_train_batch.hip, ds_trainer_batch_*): constants, node and parameter records, the view of a round's state,
// the body of every kernel of a round, and the host helpers of both (defined in ds_train.hip).  A body reads blockIdx.x /
// blockIdx.y as its kernel documents and takes pointers to ONE model's state.  The round's kernels (ds_train.hip) take a
// TrainView, add the model as a further grid dimension and offset the pointers; train_round_enqueue launches them for
// both trainers.  The single trainer is a view of one model with nothing held out and no fold array.
#pragma once

#include "ds_launch.h"
#include "ds_forest.h"
#include "ds_options.h"

namespace ds {

constexpr int kTrainFeaturesMax = 96;     // = kForestFeaturesMax: a trained model must load into ds_forest
constexpr int kTrainMaxDepth = 8;
constexpr int kTrainCutsMax = 254;        // max_bin 256: bins 0..254, 255 = missing
constexpr int kMissingBin = 255;
constexpr int kHistSlots = 16;            // (feature, node) histograms per workgroup: 16 x 256 x 16 B = 64 KiB of LDS
constexpr int kHistThreads = 512;
constexpr int kRowThreads = 256;
constexpr int kBinTileRows = 64;
constexpr double kQuantum = 1073741824.0; // 2^30
constexpr double kRtEps = 1e-6;           // xgboost's kRtEps: a split must gain more than this

enum NodeState : int32_t { kAbsent = 0, kPending = 1, kSplit = 2, kLeaf = 3 };

struct Node {
    int32_t state, feature, bin, default_left;
    float leaf;
    int32_t pad;
};

struct TrainParams {
    int32_t max_depth;
    double eta, min_child_weight, reg_lambda, beta;
};

// ---- row and column subsampling ("Subsampling") ------------------------------------------------
// The purposes of the sampling streams (include/doppel_amd.h; 1 and 2 are ds_training.hip's).
constexpr uint64_t kPurposeSampleRow = 3, kPurposeSampleTree = 4, kPurposeSampleLevel = 5;

struct TrainSampling {
    double subsample, colsample_bytree, colsample_bylevel;   // each in (0, 1]
    uint64_t seed;
    __host__ __device__ bool any() const { return subsample < 1.0 || colsample_bytree < 1.0 || colsample_bylevel < 1.0; }
};

// The first kept (third) output of the splitmix64 stream of (seed, purpose, index): ds_training.hip's Rng after its
// constructor, one next().
__host__ __device__ inline uint64_t sample_key(uint64_t seed, uint64_t purpose, uint64_t index)
{
    uint64_t z = seed * 0x9e3779b97f4a7c15ull + index * 0xd1342543de82ef95ull + purpose * 0xaf251af3b0f025b5ull +
                 3ull * 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// The model's `tree`-th tree (from 0) trains on its training row `row` (from 0, counted among the rows that train)
__device__ inline bool sample_row(const TrainSampling &sampling, int64_t tree, int64_t row)
{
    const uint64_t x = sample_key(sampling.seed, kPurposeSampleRow,
                                  (static_cast<uint64_t>(tree) << 32) | static_cast<uint64_t>(row));
    return static_cast<double>(x >> 11) * 0x1.0p-53 < sampling.subsample;
}

// ---- the state of a round: M models over one binned matrix, model m's part of a per-model array at m * its stride ----
constexpr float kTrainBaseMargin = 0.f;   // base_score 0.5

struct Candidate;   // the best split of one (node, feature), below

struct TrainModel {
    TrainParams params;
    int32_t held_out, pad;        // the fold whose rows do not train, -1 for none
};

struct TrainView {   // what every kernel of a round gets
    const uint8_t *bins;
    const float *labels;
    const float *weights;         // per-row sample weights, stride 0 like labels; null: every row weighs 1
    const uint8_t *fold;          // null without folds: the kFolds = false kernels never read it
    const int32_t *cut_offsets;
    const TrainModel *models;     // in HBM, with `active`; both null in a view of ONE model: model 0, the record `only`
    const int32_t *active;        // the models of this step: blockIdx.z (or the last grid dimension) indexes it
    long long *gh;                // stride 2n
    int32_t *node_of;             // stride n
    float *leafsum, *probabilities;   // stride n
    long long *hist;              // stride hist_stride
    Node *nodes;                  // stride slots
    int32_t *counts;              // stride slots
    Candidate *candidates;        // stride candidate_stride
    unsigned long long *errors;   // stride 1
    int64_t n, hist_stride, candidate_stride;
    int32_t nf, slots;
    TrainModel only;              // the one model of a view without `active`: read from the kernel arguments, as the
                                  // single trainer's parameters always were; at 10^5 rows its round is launch-bound
    // monotone constraints ("Monotone constraints"): both null without; only the kMonotone split
    // kernels and the clear kernel (the root's bounds) look at them
    const int8_t *monotone = nullptr;   // per feature -1, 0, +1: nf entries, stride 0 like weights
    double *bounds = nullptr;           // (lo, hi) of every heap slot's weight, stride 2 * slots
    __device__ int32_t model_index(unsigned i) const { return active != nullptr ? active[i] : 0; }
    __device__ TrainModel model(int32_t m) const
    {
        if (active != nullptr) return models[m];
        return only;
    }
};

struct TrainSamplingView {   // sampling == nullptr: of a view of ONE model, whose record is `only` and tree count `tree`
    const TrainSampling *sampling;
    const int32_t *trees;          // the trees every model has grown before this step
    const uint32_t *held_before;   // stride held_stride per slot; null without folds
    const int32_t *held_slot;      // per model: its slot of held_before, -1 for none; null without folds
    uint8_t *masks;                // stride kMaskBytes
    int64_t held_stride;
    TrainSampling only;
    int32_t tree;
    __device__ TrainSampling record(int32_t m) const
    {
        if (sampling != nullptr) return sampling[m];
        return only;
    }
    __device__ int32_t tree_of(int32_t m) const { return sampling != nullptr ? trees[m] : tree; }
};

inline int64_t heap_nodes(int32_t depth) { return (int64_t(2) << depth) - 1; }
inline int64_t hist_entries(int32_t depth, int32_t nf) { return ((int64_t(1) << depth) - 1) * nf * 512; }
inline int64_t candidate_entries(int32_t depth, int32_t nf) { return (int64_t(1) << (depth - 1)) * nf; }

// ---- host side, defined in ds_train.hip ------------------------------------------------------------------------------
// Bins of a float32[n][nf] matrix into `out` with the cuts in HBM.  A host matrix is uploaded through a temporary buffer,
// a matrix in HBM (in_hbm, complete before the call) is read where it lies and not kept.  Synchronises `stream` before it
// returns.
int train_bin_matrix(hipStream_t stream, int compute_units, const float *rows, bool in_hbm, int64_t n, int32_t nf,
                     const float *d_cuts, const int32_t *d_cut_offsets, DeviceBuffer<uint8_t> &out);
// The checks that every create entry (`who`) makes.  train_check_params names the batch's model, model < 0: no model;
// max_depth is checked by the entry, whose argument it is (an integer in one, a double of the params array in the other).
int train_check_shape(const char *who, int64_t n, int32_t n_features);
int train_check_params(const char *who, int32_t model, double eta, double min_child_weight, double reg_lambda,
                       double beta);
int train_check_cuts(const char *who, int32_t n_features, const float *cuts, const int32_t *cut_offsets);
// every label is 0 or 1; `what` ("" or "labels: ") names the argument where an entry has more than one array
int train_check_labels(const char *who, const char *what, const float *labels, int64_t n);
// the three fractions in (0, 1]; reg_lambda > 0 where rows are drawn; model as for train_check_params
int train_check_fractions(const char *who, int32_t model, const double *fractions);
int train_check_subsample(const char *who, int32_t model, double subsample, double reg_lambda);
// Sample weights ("Sample weights"): every weight finite and >= 0, and the overflow guard
// max(beta, 1) * sum(weights) <= 2^32 with the sum in double; beta is the largest among the models that share the array
int train_check_weights(const char *who, const float *weights, int64_t n, double beta);
// Monotone constraints ("Monotone constraints"): every entry -1, 0 or 1; *any: one is not 0
int train_check_monotone(const char *who, const int8_t *constraints, int32_t n_features, bool *any);
// What a create entry sets up on the current device: its stream, the cuts in HBM and the compute-unit count
int train_create_setup(const char *who, int device, int32_t n_features, const float *cuts, const int32_t *cut_offsets,
                       hipStream_t *stream, DeviceBuffer<float> &d_cuts, DeviceBuffer<int32_t> &d_cut_offsets,
                       int *compute_units);
// The grid of a kernel that strides over `items` rows: at most 8 workgroups per CU, and at most the test cap
// (ds_trainer_batch_option("max_blocks"), 0 = none) where one is set.  The results do not depend on it.
extern Option g_train_max_blocks;
unsigned train_row_grid(int compute_units, int64_t items);
// Enqueues one round for the n_active models of v.active on `stream` and does not synchronise: clear, the gradients
// (with `sampling`: the feature masks, then the gradients of the rows drawn), then per level < depth (the largest
// max_depth among the active models) histogram, split-feature, split and partition.  `folds`: v.fold holds rows out.
int train_round_enqueue(hipStream_t stream, const TrainView &v, const TrainSamplingView *sampling, int32_t n_active,
                        int32_t depth, bool folds, int compute_units);
// a heap of `slots` nodes copied back from the device -> node_info int32[slots][4] and node_leaf float[slots]
void train_unpack_heap(const Node *heap, int64_t slots, int32_t *node_info, float *node_leaf);
// ---- continuing from a model ("Continuing from a model") --------------------------------------
// What every seed entry (`who`) refuses of the forest: null, another device, another feature count, a base margin that
// is not kTrainBaseMargin
int train_check_seed_forest(const char *who, const ds_forest *forest, int device, int32_t n_features);
// Enqueues ds_train_seed_kernel on `stream` and does not synchronise: leafsum[m * stride + r] = the forest's leaf sum of
// row r of the raw float32[n][n_features] matrix, for every m < n_models.  A matrix in HBM is read where it lies; a host
// matrix goes through `staged` in chunks of at most kSeedChunkBytes, which the caller keeps (with the matrix) until it
// has synchronised the stream.
constexpr int64_t kSeedChunkBytes = int64_t(64) << 20;
int train_seed_enqueue(hipStream_t stream, int compute_units, const ds_forest *forest, const float *rows, bool in_hbm,
                       int64_t n, float *leafsum, int32_t n_models, int64_t stride, DeviceBuffer<float> &staged);

// ---- gradients of weighted_log_loss at the current margins ---------------------------------------------------------
// One row's quantized (g, h) at its float32 probability p: the one statement of this arithmetic, for the trainers'
// gradient kernel below and for the refresh of a finished model (ds_refresh.hip).  weights: null, every row weighs 1.
__device__ inline void train_row_gradient(float p, float label, const float *weights, int64_t r, double beta,
                                          long long *qg, long long *qh)
{
    const double y = label, pd = p;
    const double w = beta + y - beta * y;
    const double s = weights != nullptr ? weights[r] : 1.0;
    const double g = (pd * w - y) * s;
    const double h = (pd * (1.0 - pd) * w) * s;
    *qg = static_cast<long long>(rint(g * kQuantum));
    *qh = static_cast<long long>(rint(h * kQuantum));
}

// The value of a leaf with the quantized sums (qg, qh), unbounded: train_split_nodes' and the refresh's
__device__ inline float train_leaf_value(long long qg, long long qh, double lambda, double eta)
{
    const double g = static_cast<double>(qg) / kQuantum, h = static_cast<double>(qh) / kQuantum;
    return static_cast<float>((-g / (h + lambda)) * eta);
}

// kFolds: a row with fold[r] == held_out does not train: its (g, h) is (0, 0); everything else is written as for any row
// kSampled: with subsample < 1 a training row is drawn for this tree (sample_row) and an undrawn one is treated like a
// held-out row.  The draw is indexed by the row's number among the model's TRAINING rows: r itself without folds, else
// r - (held-out rows before r) = r - held_before[r / 64] - (held-out rows of r's wave in lower lanes); a wave's rows are
// 64 consecutive ones from a multiple of 64, whatever the grid.  held_before is null for a model that holds nothing out.
template <bool kFolds, bool kSampled = false>
__device__ inline void train_gradient_rows(const float *leafsum, const float *labels, int64_t n, float base_margin,
                                           double beta, float *probabilities, long long *gh, int32_t *node_of,
                                           const uint8_t *fold, int32_t held_out, const float *weights,
                                           const TrainSampling *sampling = nullptr, int64_t tree = 0,
                                           const uint32_t *held_before = nullptr)
{
    for (int64_t r = blockIdx.x * static_cast<int64_t>(kRowThreads) + threadIdx.x; r < n;
         r += static_cast<int64_t>(gridDim.x) * kRowThreads) {
        const float margin = base_margin + leafsum[r];
        const float p = forest_probability(margin);
        long long qg, qh;
        train_row_gradient(p, labels[r], weights, r, beta, &qg, &qh);
        bool trains = !kFolds || static_cast<int32_t>(fold[r]) != held_out;
        if (kSampled && sampling->subsample < 1.0) {   // the same answer in every row of a model
            int64_t row = r;
            if (kFolds && held_before != nullptr) {
                const unsigned long long held = __ballot(!trains);   // lanes past n have left the loop: no bits
                row = r - held_before[r >> 6] - __popcll(held & ((1ull << (threadIdx.x & 63)) - 1ull));
            }
            trains = trains && sample_row(*sampling, tree, row);
        }
        probabilities[r] = p;
        gh[2 * r] = trains ? qg : 0ll;
        gh[2 * r + 1] = trains ? qh : 0ll;
        node_of[r] = 0;
    }
}

// Which child of a split parent gets its histogram built (the one with fewer rows, the left one on a tie); the other
// one is parent - built.
__device__ inline bool is_built(const int32_t *counts, int32_t node)
{
    const bool left = (node & 1) == 1;
    const int32_t sibling = left ? node + 1 : node - 1;
    return left ? counts[node] <= counts[sibling] : counts[node] < counts[sibling];
}

// ---- histograms of one level ---------------------------------------------------------------------------------------
// Level d >= 1 builds one child per split parent of level d - 1 (slot j <-> the j-th parent of that level); level 0
// builds the root.  blockIdx.y = (feature group, node group): nodes_per_group x features_per_group <= kHistSlots
// histograms in LDS, summed with 64-bit LDS adds, flushed with 64-bit global adds (zeros skipped).
// kFolds: rows with fold[r] == held_out carry (0, 0) and are skipped, and a workgroup none of whose slots has a node
// to build returns before it reads a row; neither changes a bit of the sums.
// kSampled: a row whose (g, h) is (0, 0) -- an undrawn row -- is skipped as well; it would add zeros.
template <bool kFolds, bool kSampled = false>
__device__ inline void train_histogram_group(const uint8_t *bins, const long long *gh, const int32_t *node_of,
                                             const int32_t *counts, const Node *nodes, int64_t n, int32_t nf,
                                             int32_t level, int32_t n_built, int32_t nodes_per_group,
                                             int32_t features_per_group, int32_t feature_groups,
                                             unsigned long long *hist, const uint8_t *fold, int32_t held_out)
{
    __shared__ unsigned long long s_hist[kHistSlots * 256 * 2];
    __shared__ int32_t s_node[kHistSlots];   // heap id of the built node of each slot, -1 for none
    const int feature_group = blockIdx.y % feature_groups, node_group = blockIdx.y / feature_groups;
    const int f0 = feature_group * features_per_group;
    const int f_count = min(features_per_group, nf - f0);
    const int j0 = node_group * nodes_per_group;
    const int j_count = min(nodes_per_group, n_built - j0);
    int32_t node_here = -1;
    if (static_cast<int>(threadIdx.x) < j_count) {
        if (level == 0) {
            node_here = 0;
        } else {
            const int32_t parent = (1 << (level - 1)) - 1 + j0 + threadIdx.x;
            if (nodes[parent].state == kSplit)
                node_here = is_built(counts, 2 * parent + 1) ? 2 * parent + 1 : 2 * parent + 2;
        }
        s_node[threadIdx.x] = node_here;
    }
    if (kFolds) {
        if (!__syncthreads_or(node_here >= 0)) return;   // the same answer in every thread
    }
    for (int i = threadIdx.x; i < kHistSlots * 512; i += kHistThreads) s_hist[i] = 0ull;
    __syncthreads();
    const int32_t level_first = (1 << level) - 1;
    const int64_t chunk = (n + gridDim.x - 1) / gridDim.x;
    const int64_t begin = blockIdx.x * chunk, end = min(n, begin + chunk);
    for (int64_t r = begin + threadIdx.x; r < end; r += kHistThreads) {
        const int32_t node = node_of[r];
        if (node < level_first) continue;   // -1: finished
        if (kFolds && static_cast<int32_t>(fold[r]) == held_out) continue;
        const int j = level == 0 ? 0 : ((node - 1) >> 1) - ((1 << (level - 1)) - 1) - j0;
        if (j < 0 || j >= j_count || s_node[j] != node) continue;
        const long long g = gh[2 * r], h = gh[2 * r + 1];
        if (kSampled && (g | h) == 0ll) continue;
        for (int k = 0; k < f_count; ++k) {
            const int bin = bins[static_cast<int64_t>(f0 + k) * n + r];
            unsigned long long *slot = s_hist + ((k * nodes_per_group + j) * 256 + bin) * 2;
            atomicAdd(slot, static_cast<unsigned long long>(g));
            atomicAdd(slot + 1, static_cast<unsigned long long>(h));
        }
    }
    __syncthreads();
    const size_t node_stride = static_cast<size_t>(nf) * 512;
    for (int i = threadIdx.x; i < f_count * j_count * 512; i += kHistThreads) {
        const int k = i / (j_count * 512), rest = i - k * j_count * 512, j = rest / 512, e = rest - j * 512;
        const unsigned long long value = s_hist[(k * nodes_per_group + j) * 512 + e];
        if (value == 0ull || s_node[j] < 0) continue;
        atomicAdd(hist + s_node[j] * node_stride + static_cast<size_t>(f0 + k) * 512 + e, value);
    }
}

__device__ inline double node_gain(double g, double h, double lambda) { return g * g / (h + lambda); }

// ---- monotone constraints ("Monotone constraints") ---------------------------------------------
// The weight of a node with sums (g, h) clamped to the node's bounds [lo, hi], and its gain term: node_gain while the
// raw weight lies inside the bounds, the loss reduction at the clamped weight otherwise.  Infinite bounds give
// node_gain and the raw weight, bit for bit.
struct BoundedTerm {
    double weight, term;
};

__device__ inline BoundedTerm bounded_term(double g, double h, double lambda, double lo, double hi)
{
    const double w = -g / (h + lambda);
    const double clamped = fmin(fmax(w, lo), hi);
    if (lo <= w && w <= hi) return BoundedTerm{clamped, node_gain(g, h, lambda)};
    return BoundedTerm{clamped, -(((2.0 * g) * clamped) + (((h + lambda) * clamped) * clamped))};
}

struct Candidate {            // the best split of one (node, feature)
    double gain;              // -inf: no valid candidate
    long long left_g, left_h, total_g, total_h;
    int32_t bin, missing_left;
};

// ---- split choice, part 1: one workgroup per (node of the level, feature), one thread per bin ----------------------
// blockIdx.x = the node's index in its level, blockIdx.y = the feature.
// A node whose histogram was not built gets parent - built sibling (exact) first.  Prefix sums by an LDS scan; each
// thread b - 1 tries boundary b with the missing rows right, then left; the workgroup keeps the largest gain, the
// lower b on a tie.
// kSampled: a feature with level_mask[f] == 0 (outside the level's feature set) offers no boundary, like a feature
// with a single bin; its histogram is still completed by the subtraction and its totals still written, because a
// later level may include the feature and the node's leaf value comes from the totals of whichever feature wins.
// kMonotone: the three terms of a candidate's gain are bounded_term's under the node's own bounds (bounds[2 * node],
// bounds[2 * node + 1]), and after the min_child_weight test a candidate whose clamped child weights stand in the wrong
// order for monotone[f] is rejected.  The candidate order, the tie order and what thread 0 writes are unchanged.
template <bool kSampled = false, bool kMonotone = false>
__device__ inline void train_split_feature(long long *hist, const int32_t *counts, const Node *nodes,
                                           const int32_t *cut_offsets, int32_t nf, int32_t level,
                                           const TrainParams &params, Candidate *candidates,
                                           const uint8_t *level_mask = nullptr, const int8_t *monotone = nullptr,
                                           const double *bounds = nullptr)
{
    __shared__ long long s_g[256], s_h[256];
    __shared__ double s_gain[256];
    __shared__ int32_t s_key[256];   // 2 * b + missing_left of the thread's best, INT32_MAX for none
    const int32_t node = (1 << level) - 1 + blockIdx.x;
    if (level > 0 && nodes[(node - 1) >> 1].state != kSplit) return;   // the node does not exist
    const int f = blockIdx.y, t = threadIdx.x;
    const size_t node_stride = static_cast<size_t>(nf) * 512, at = static_cast<size_t>(f) * 512 + 2 * t;
    long long g, h;
    if (level == 0 || is_built(counts, node)) {
        g = hist[node * node_stride + at];
        h = hist[node * node_stride + at + 1];
    } else {
        const int32_t parent = (node - 1) >> 1, sibling = (node & 1) ? node + 1 : node - 1;
        g = hist[parent * node_stride + at] - hist[sibling * node_stride + at];
        h = hist[parent * node_stride + at + 1] - hist[sibling * node_stride + at + 1];
        hist[node * node_stride + at] = g;
        hist[node * node_stride + at + 1] = h;
    }
    s_g[t] = g;
    s_h[t] = h;
    __syncthreads();
    for (int offset = 1; offset < 256; offset <<= 1) {   // inclusive scan: s_g[t] = sum of bins 0 .. t
        const long long add_g = t >= offset ? s_g[t - offset] : 0, add_h = t >= offset ? s_h[t - offset] : 0;
        __syncthreads();
        s_g[t] += add_g;
        s_h[t] += add_h;
        __syncthreads();
    }
    const long long total_g = s_g[255], total_h = s_h[255];
    const long long missing_g = total_g - s_g[254], missing_h = total_h - s_h[254];
    const double lambda = params.reg_lambda, mcw = params.min_child_weight;
    const double G = static_cast<double>(total_g) / kQuantum, H = static_cast<double>(total_h) / kQuantum;
    double lo = 0.0, hi = 0.0;
    int sign = 0;
    if (kMonotone) {
        lo = bounds[2 * node];
        hi = bounds[2 * node + 1];
        sign = monotone[f];
    }
    const double parent_gain = kMonotone ? bounded_term(G, H, lambda, lo, hi).term : node_gain(G, H, lambda);
    const int b = t + 1, n_bins = cut_offsets[f + 1] - cut_offsets[f] + 1;
    double best = -INFINITY;
    int32_t key = INT32_MAX;
    if (b < n_bins && (!kSampled || level_mask[f] != 0)) {
        for (int missing_left = 0; missing_left < 2; ++missing_left) {   // missing right first
            const long long lg = s_g[t] + (missing_left ? missing_g : 0), lh = s_h[t] + (missing_left ? missing_h : 0);
            const double GL = static_cast<double>(lg) / kQuantum, HL = static_cast<double>(lh) / kQuantum;
            const double GR = static_cast<double>(total_g - lg) / kQuantum;
            const double HR = static_cast<double>(total_h - lh) / kQuantum;
            if (HL < mcw || HR < mcw) continue;
            double gain;
            if (kMonotone) {
                const BoundedTerm left = bounded_term(GL, HL, lambda, lo, hi), right = bounded_term(GR, HR, lambda, lo, hi);
                if ((sign > 0 && left.weight > right.weight) || (sign < 0 && left.weight < right.weight)) continue;
                gain = left.term + right.term - parent_gain;
            } else {
                gain = node_gain(GL, HL, lambda) + node_gain(GR, HR, lambda) - parent_gain;
            }
            if (gain > best) {
                best = gain;
                key = 2 * b + missing_left;
            }
        }
    }
    s_gain[t] = best;
    s_key[t] = key;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {   // larger gain, then the lower key (b, then missing right)
        if (t < half) {
            const double other = s_gain[t + half];
            if (other > s_gain[t] || (other == s_gain[t] && s_key[t + half] < s_key[t])) {
                s_gain[t] = other;
                s_key[t] = s_key[t + half];
            }
        }
        __syncthreads();
    }
    if (t != 0) return;
    Candidate out;
    out.gain = s_key[0] == INT32_MAX ? -INFINITY : s_gain[0];
    out.bin = s_key[0] == INT32_MAX ? 0 : s_key[0] >> 1;
    out.missing_left = s_key[0] == INT32_MAX ? 0 : s_key[0] & 1;
    out.left_g = out.bin > 0 ? s_g[out.bin - 1] + (out.missing_left ? missing_g : 0) : 0;
    out.left_h = out.bin > 0 ? s_h[out.bin - 1] + (out.missing_left ? missing_h : 0) : 0;
    out.total_g = total_g;
    out.total_h = total_h;
    candidates[static_cast<size_t>(blockIdx.x) * nf + f] = out;
}

// ---- split choice, part 2: one thread per node of the level over its features' candidates ---------------------------
// kMonotone: every leaf written is clamped to its own bounds, and a split writes its children's bounds: with mid the
// mean of the winner's two clamped weights (under this node's bounds), [lo, mid] and [mid, hi] for the lower and the
// higher side of a constrained feature, [lo, hi] for both children of an unconstrained one.
template <bool kMonotone = false>
__device__ inline void train_split_nodes(const Candidate *candidates, Node *nodes, int32_t nf, int32_t level,
                                         const TrainParams &params, const int8_t *monotone = nullptr,
                                         double *bounds = nullptr)
{
    const int32_t index = blockIdx.x * 64 + threadIdx.x;
    if (index >= (1 << level)) return;
    const int32_t node = (1 << level) - 1 + index;
    if (level > 0 && nodes[(node - 1) >> 1].state != kSplit) return;
    const Candidate *mine = candidates + static_cast<size_t>(index) * nf;
    int winner = 0;
    for (int k = 1; k < nf; ++k)   // strictly greater: a tie keeps the lower feature
        if (mine[k].gain > mine[winner].gain) winner = k;
    const double lambda = params.reg_lambda;
    auto leaf_value = [&](long long qg, long long qh, double lo = 0.0, double hi = 0.0) {
        const double g = static_cast<double>(qg) / kQuantum, h = static_cast<double>(qh) / kQuantum;
        if (kMonotone) return static_cast<float>(bounded_term(g, h, lambda, lo, hi).weight * params.eta);
        return train_leaf_value(qg, qh, lambda, params.eta);
    };
    double lo = 0.0, hi = 0.0;
    if (kMonotone) {
        lo = bounds[2 * node];
        hi = bounds[2 * node + 1];
    }
    const Candidate &best = mine[winner];
    const long long G = best.total_g, H = best.total_h;
    Node &out = nodes[node];
    out.feature = -1;
    out.bin = 0;
    out.default_left = 0;
    out.leaf = 0.f;
    if (best.gain > kRtEps) {
        out.state = kSplit;
        out.feature = winner;
        out.bin = best.bin;
        out.default_left = best.missing_left;
        const bool last = level + 1 == params.max_depth;
        Node &left = nodes[2 * node + 1], &right = nodes[2 * node + 2];
        left.state = right.state = last ? kLeaf : kPending;
        left.feature = right.feature = -1;
        double left_lo = lo, left_hi = hi, right_lo = lo, right_hi = hi;
        if (kMonotone) {
            const int sign = monotone[winner];
            const double wl = bounded_term(static_cast<double>(best.left_g) / kQuantum,
                                           static_cast<double>(best.left_h) / kQuantum, lambda, lo, hi).weight;
            const double wr = bounded_term(static_cast<double>(G - best.left_g) / kQuantum,
                                           static_cast<double>(H - best.left_h) / kQuantum, lambda, lo, hi).weight;
            const double mid = (wl + wr) / 2.0;
            if (sign > 0) {
                left_hi = mid;
                right_lo = mid;
            } else if (sign < 0) {
                left_lo = mid;
                right_hi = mid;
            }
            double *child = bounds + 2 * (2 * node + 1);   // the left child's pair, then the right child's
            child[0] = left_lo;
            child[1] = left_hi;
            child[2] = right_lo;
            child[3] = right_hi;
        }
        left.leaf = last ? leaf_value(best.left_g, best.left_h, left_lo, left_hi) : 0.f;
        right.leaf = last ? leaf_value(G - best.left_g, H - best.left_h, right_lo, right_hi) : 0.f;
    } else {
        out.state = kLeaf;
        out.leaf = leaf_value(G, H, lo, hi);
    }
}

// ---- row partition: rows of split nodes move to a child, rows that reach a leaf add it to their margin -------------
__device__ inline void train_partition_rows(const uint8_t *bins, const Node *nodes, int64_t n, int32_t level,
                                            int32_t *node_of, float *leafsum, int32_t *counts)
{
    __shared__ int32_t s_counts[2 << kTrainMaxDepth];
    const int32_t level_first = (1 << level) - 1, next_first = 2 * level_first + 1, next_width = 1 << (level + 1);
    for (int i = threadIdx.x; i < next_width; i += kRowThreads) s_counts[i] = 0;
    __syncthreads();
    for (int64_t r = blockIdx.x * static_cast<int64_t>(kRowThreads) + threadIdx.x; r < n;
         r += static_cast<int64_t>(gridDim.x) * kRowThreads) {
        int32_t node = node_of[r];
        if (node < level_first) continue;
        Node rec = nodes[node];
        if (rec.state == kSplit) {
            const int bin = bins[static_cast<int64_t>(rec.feature) * n + r];
            const bool left = bin == kMissingBin ? rec.default_left != 0 : bin < rec.bin;
            node = 2 * node + (left ? 1 : 2);
            rec = nodes[node];
        }
        if (rec.state == kLeaf) {
            leafsum[r] = leafsum[r] + rec.leaf;
            node_of[r] = -1;
        } else {
            node_of[r] = node;
            atomicAdd(&s_counts[node - next_first], 1);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < next_width; i += kRowThreads)
        if (s_counts[i]) atomicAdd(&counts[next_first + i], s_counts[i]);
}

// ---- feature sets of one tree: one workgroup of kMaskThreads >= nf threads, thread f = feature f ---------------------
// mask[d * kTrainFeaturesMax + f] = 1 iff feature f is in the set of level d < max_depth.  The tree's set: the k_tree =
// max(1, floor(colsample_bytree * nf)) features with the smallest key of the TREE stream, index (tree << 32) | f, ties
// to the lower f; level d's set: the k_level = max(1, floor(colsample_bylevel * k_tree)) features of the tree's set with
// the smallest key of the LEVEL stream, index (tree << 32) | (d << 8) | f.  A fraction of 1 takes the whole set, no draw.
constexpr int kMaskThreads = 128;
constexpr int kMaskBytes = kTrainMaxDepth * kTrainFeaturesMax;

__device__ inline void train_feature_masks(const TrainSampling &sampling, int64_t tree, int32_t nf, int32_t max_depth,
                                           uint8_t *mask)
{
    __shared__ uint64_t s_key[kTrainFeaturesMax];
    __shared__ uint8_t s_tree[kTrainFeaturesMax];
    const int f = threadIdx.x;
    const bool mine = f < nf;
    const uint64_t base = static_cast<uint64_t>(tree) << 32;
    const int k_tree = max(1, static_cast<int>(floor(sampling.colsample_bytree * nf)));
    bool in_tree = mine;
    if (sampling.colsample_bytree < 1.0) {
        const uint64_t key = sample_key(sampling.seed, kPurposeSampleTree, base | static_cast<uint64_t>(f));
        if (mine) s_key[f] = key;
        __syncthreads();
        int rank = 0;
        for (int g = 0; g < nf; ++g) rank += s_key[g] < key || (s_key[g] == key && g < f);
        in_tree = mine && rank < k_tree;
        __syncthreads();
    }
    if (mine) s_tree[f] = in_tree;
    __syncthreads();
    const int k_level = max(1, static_cast<int>(floor(sampling.colsample_bylevel * k_tree)));
    for (int d = 0; d < max_depth; ++d) {
        bool in_level = in_tree;
        if (sampling.colsample_bylevel < 1.0) {
            const uint64_t key = sample_key(sampling.seed, kPurposeSampleLevel,
                                            base | (static_cast<uint64_t>(d) << 8) | static_cast<uint64_t>(f));
            if (mine) s_key[f] = key;
            __syncthreads();
            int rank = 0;
            for (int g = 0; g < nf; ++g) rank += s_tree[g] && (s_key[g] < key || (s_key[g] == key && g < f));
            in_level = in_tree && rank < k_level;
            __syncthreads();
        }
        if (mine) mask[d * kTrainFeaturesMax + f] = in_level ? 1 : 0;
    }
}

// train.py:fast_custom_error of one row at its margin: 1 for a missed positive, 5 for a false positive
__device__ inline unsigned long long train_row_error(float margin, float label)
{
    const bool positive = forest_positive(forest_probability(margin), 0.9);  // settings.py PREDICTION_PROBABILITY_THRESHOLD
    if (label != 0.f) return positive ? 0 : 1;
    return positive ? 5 : 0;                               // FALSE_POSITIVE_PENALTY_FACTOR
}

}  // namespace ds
