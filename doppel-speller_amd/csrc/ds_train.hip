// Training of the match model (doppelspeller/train.py: xgb.train with obj=weighted_log_loss, feval=custom_error):
// histogram gradient boosting with depth-wise growth on the device.  The rule (DESIGN.md section "Training") is
// restated by a NumPy model in the tests, which compare every tree, margin and error bit for bit.
//
// Data in HBM, per training matrix (n rows, nf features):
//   bins      uint8[nf][n]   feature-major: bin b < 255 of a value, 255 = NaN (the missing bin)
//   gh        int64[n][2]    quantized gradient and hessian of the current round, rint(g * 2^30), rint(h * 2^30)
//   node_of   int32[n]       heap id of the node a row sits in while a tree grows (-1: its leaf is already added)
//   leafsum   float[n]       sum of the leaves of the trees so far, in tree order (margin = base_margin + leafsum)
//   hist      int64[2^D - 1][nf][256][2]  per split candidate node (heap order, levels 0..D-1): (sum qg, sum qh)
//                            per bin; entry 255 = the missing bin
//   nodes     Node[2^(D+1) - 1] the tree being grown, heap order (children of i: 2i + 1, 2i + 2)
// Integer sums do not depend on the order of their terms: histograms, splits and trees are identical under any
// schedule and from run to run.
#include "ds_common.h"

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

// ---- gradients of weighted_log_loss at the current margins ---------------------------------------------------------
__global__ __launch_bounds__(kRowThreads) void ds_train_gradient_kernel(const float *leafsum, const float *labels,
                                                                         int64_t n, float base_margin, double beta,
                                                                         float *probabilities, long long *gh,
                                                                         int32_t *node_of)
{
    for (int64_t r = blockIdx.x * static_cast<int64_t>(kRowThreads) + threadIdx.x; r < n;
         r += static_cast<int64_t>(gridDim.x) * kRowThreads) {
        const float margin = base_margin + leafsum[r];
        const float p = 1.0f / (1.0f + expf(-margin));   // ds_forest.hip's rule
        const double y = labels[r], pd = p;
        const double w = beta + y - beta * y;
        const double g = pd * w - y;
        const double h = pd * (1.0 - pd) * w;
        probabilities[r] = p;
        gh[2 * r] = static_cast<long long>(rint(g * kQuantum));
        gh[2 * r + 1] = static_cast<long long>(rint(h * kQuantum));
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
__global__ __launch_bounds__(kHistThreads) void ds_train_histogram_kernel(
    const uint8_t *bins, const long long *gh, const int32_t *node_of, const int32_t *counts, const Node *nodes,
    int64_t n, int32_t nf, int32_t level, int32_t n_built, int32_t nodes_per_group, int32_t features_per_group,
    int32_t feature_groups, unsigned long long *hist)
{
    __shared__ unsigned long long s_hist[kHistSlots * 256 * 2];
    __shared__ int32_t s_node[kHistSlots];   // heap id of the built node of each slot, -1 for none
    const int feature_group = blockIdx.y % feature_groups, node_group = blockIdx.y / feature_groups;
    const int f0 = feature_group * features_per_group;
    const int f_count = min(features_per_group, nf - f0);
    const int j0 = node_group * nodes_per_group;
    const int j_count = min(nodes_per_group, n_built - j0);
    for (int i = threadIdx.x; i < kHistSlots * 512; i += kHistThreads) s_hist[i] = 0ull;
    if (static_cast<int>(threadIdx.x) < j_count) {
        int32_t node = -1;
        if (level == 0) {
            node = 0;
        } else {
            const int32_t parent = (1 << (level - 1)) - 1 + j0 + threadIdx.x;
            if (nodes[parent].state == kSplit) node = is_built(counts, 2 * parent + 1) ? 2 * parent + 1 : 2 * parent + 2;
        }
        s_node[threadIdx.x] = node;
    }
    __syncthreads();
    const int32_t level_first = (1 << level) - 1;
    const int64_t chunk = (n + gridDim.x - 1) / gridDim.x;
    const int64_t begin = blockIdx.x * chunk, end = min(n, begin + chunk);
    for (int64_t r = begin + threadIdx.x; r < end; r += kHistThreads) {
        const int32_t node = node_of[r];
        if (node < level_first) continue;   // -1: finished
        const int j = level == 0 ? 0 : ((node - 1) >> 1) - ((1 << (level - 1)) - 1) - j0;
        if (j < 0 || j >= j_count || s_node[j] != node) continue;
        const long long g = gh[2 * r], h = gh[2 * r + 1];
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

struct Candidate {            // the best split of one (node, feature)
    double gain;              // -inf: no valid candidate
    long long left_g, left_h, total_g, total_h;
    int32_t bin, missing_left;
};

// ---- split choice, part 1: one workgroup per (node of the level, feature), one thread per bin ----------------------
// A node whose histogram was not built gets parent - built sibling (exact) first.  Prefix sums by an LDS scan; each
// thread b - 1 tries boundary b with the missing rows right, then left; the workgroup keeps the largest gain, the
// lower b on a tie.
__global__ __launch_bounds__(256) void ds_train_split_feature_kernel(long long *hist, const int32_t *counts,
                                                                      const Node *nodes, const int32_t *cut_offsets,
                                                                      int32_t nf, int32_t level, TrainParams params,
                                                                      Candidate *candidates)
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
    const double parent_gain = node_gain(G, H, lambda);
    const int b = t + 1, n_bins = cut_offsets[f + 1] - cut_offsets[f] + 1;
    double best = -INFINITY;
    int32_t key = INT32_MAX;
    if (b < n_bins) {
        for (int missing_left = 0; missing_left < 2; ++missing_left) {   // missing right first
            const long long lg = s_g[t] + (missing_left ? missing_g : 0), lh = s_h[t] + (missing_left ? missing_h : 0);
            const double GL = static_cast<double>(lg) / kQuantum, HL = static_cast<double>(lh) / kQuantum;
            const double GR = static_cast<double>(total_g - lg) / kQuantum;
            const double HR = static_cast<double>(total_h - lh) / kQuantum;
            if (HL < mcw || HR < mcw) continue;
            const double gain = node_gain(GL, HL, lambda) + node_gain(GR, HR, lambda) - parent_gain;
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
__global__ __launch_bounds__(64) void ds_train_split_kernel(const Candidate *candidates, Node *nodes, int32_t nf,
                                                             int32_t level, TrainParams params)
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
    auto leaf_value = [&](long long qg, long long qh) {
        const double g = static_cast<double>(qg) / kQuantum, h = static_cast<double>(qh) / kQuantum;
        return static_cast<float>((-g / (h + lambda)) * params.eta);
    };
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
        left.leaf = last ? leaf_value(best.left_g, best.left_h) : 0.f;
        right.leaf = last ? leaf_value(G - best.left_g, H - best.left_h) : 0.f;
    } else {
        out.state = kLeaf;
        out.leaf = leaf_value(G, H);
    }
}

// ---- row partition: rows of split nodes move to a child, rows that reach a leaf add it to their margin -------------
__global__ __launch_bounds__(kRowThreads) void ds_train_partition_kernel(const uint8_t *bins, const Node *nodes,
                                                                          int64_t n, int32_t level, int32_t *node_of,
                                                                          float *leafsum, int32_t *counts)
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
        const float margin = base_margin + sum;
        const float p = 1.0f / (1.0f + expf(-margin));
        const bool positive = static_cast<double>(p) > 0.9;   // settings.py PREDICTION_PROBABILITY_THRESHOLD
        if (labels[r] != 0.f) mine += positive ? 0 : 1;
        else mine += positive ? 5 : 0;                          // FALSE_POSITIVE_PENALTY_FACTOR
    }
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

}  // namespace ds

struct ds_trainer {
    int device = 0;
    int64_t n = 0, n_eval = 0;
    int32_t nf = 0;
    ds::TrainParams params{};
    float base_margin = 0.f;
    bool has_labels = false;
    int64_t rounds = 0;
    hipStream_t stream = nullptr;
    ds::DeviceBuffer<uint8_t> bins, eval_bins;
    ds::DeviceBuffer<float> labels, eval_labels, leafsum, eval_leafsum, probabilities, cuts;
    ds::DeviceBuffer<int32_t> cut_offsets, node_of, counts;
    ds::DeviceBuffer<long long> gh, hist;
    ds::DeviceBuffer<ds::Node> nodes;
    ds::DeviceBuffer<ds::Candidate> candidates;   // [2^(max_depth - 1)][nf]: the best split per (node, feature)
    ds::DeviceBuffer<unsigned long long> error;
    std::vector<int32_t> host_offsets;
    ds::Node *pinned_nodes = nullptr;
    unsigned long long *pinned_error = nullptr;
    int compute_units = 256;
    ~ds_trainer()
    {
        if (pinned_nodes) (void)hipHostFree(pinned_nodes);
        if (pinned_error) (void)hipHostFree(pinned_error);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

int64_t heap_nodes(int32_t depth) { return (int64_t(2) << depth) - 1; }

// bins of a float32[n][nf] matrix into `out`: a host matrix is uploaded through a temporary buffer, a matrix in HBM
// (in_hbm, complete before the call) is read where it lies and not kept
int bin_matrix(ds_trainer *t, const float *rows, bool in_hbm, int64_t n, ds::DeviceBuffer<uint8_t> &out)
{
    ds::DeviceBuffer<float> staged;
    int status = in_hbm ? DS_OK : staged.upload(rows, static_cast<size_t>(n) * t->nf);
    if (status == DS_OK) status = out.allocate(static_cast<size_t>(n) * t->nf);
    if (status != DS_OK) return status;
    const int64_t tiles = (n + ds::kBinTileRows - 1) / ds::kBinTileRows;
    const int grid = static_cast<int>(std::min<int64_t>(tiles, int64_t(t->compute_units) * 4));
    hipLaunchKernelGGL(ds::ds_train_bin_kernel, dim3(grid), dim3(ds::kRowThreads), 0, t->stream,
                       in_hbm ? rows : staged.ptr, n, t->nf, t->cuts.ptr, t->cut_offsets.ptr, out.ptr);
    DS_HIP(hipGetLastError());
    DS_HIP(hipStreamSynchronize(t->stream));   // `staged` is freed on return; the caller's matrix is no longer read
    return DS_OK;
}

int check_free(int64_t bytes, const char *what)
{
    size_t free_bytes = 0, total_bytes = 0;
    DS_HIP(hipMemGetInfo(&free_bytes, &total_bytes));
    if (static_cast<size_t>(bytes) + (size_t(64) << 20) > free_bytes) {   // 64 MiB of head room, as ds_exact
        ds::set_error("%s: needs %lld bytes of HBM, %zu are free", what, (long long)bytes, free_bytes);
        return DS_E_HIP;
    }
    return DS_OK;
}

int row_grid(const ds_trainer *t, int64_t n)
{
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((n + ds::kRowThreads - 1) / ds::kRowThreads,
                                                                   int64_t(t->compute_units) * 8)));
}

// ds_trainer_create (`who`, features on the host) and ds_trainer_create_device (features in HBM)
int create_trainer(const char *who, const float *features, bool in_hbm, int64_t n, int32_t n_features, const float *cuts,
                   const int32_t *cut_offsets, int32_t max_depth, double eta, double min_child_weight, double reg_lambda,
                   double beta, int device, ds_trainer **out)
{
    DS_REQUIRE(out != nullptr, "%s: out is null", who);
    *out = nullptr;
    DS_REQUIRE(features && cuts && cut_offsets, "%s: null input", who);
    DS_REQUIRE(n >= 1 && n <= INT32_MAX, "%s: n = %lld rows out of range [1, 2^31)", who, (long long)n);
    DS_REQUIRE(n_features >= 1 && n_features <= ds::kTrainFeaturesMax,
               "%s: n_features = %d out of range [1, %d]", who, n_features, ds::kTrainFeaturesMax);
    DS_REQUIRE(max_depth >= 1 && max_depth <= ds::kTrainMaxDepth, "%s: max_depth = %d out of range [1, %d]", who,
               max_depth, ds::kTrainMaxDepth);
    DS_REQUIRE(eta > 0 && eta < 1e30 && min_child_weight >= 0 && min_child_weight < 1e30 && reg_lambda >= 0 &&
                   reg_lambda < 1e30 && beta > 0 && beta < 1e30 && reg_lambda + min_child_weight > 0,
               "%s: eta, beta must be positive, min_child_weight, reg_lambda non-negative and not both 0", who);
    DS_REQUIRE(cut_offsets[0] == 0, "%s: cut_offsets[0] must be 0", who);
    for (int32_t f = 0; f < n_features; ++f) {
        const int32_t count = cut_offsets[f + 1] - cut_offsets[f];
        DS_REQUIRE(count >= 0 && count <= ds::kTrainCutsMax, "%s: feature %d has %d cuts (at most %d)", who,
                   f, count, ds::kTrainCutsMax);
        for (int32_t i = cut_offsets[f]; i < cut_offsets[f + 1]; ++i)
            DS_REQUIRE(cuts[i] == cuts[i] && (i == cut_offsets[f] || cuts[i - 1] < cuts[i]),
                       "%s: the cuts of feature %d are not strictly ascending", who, f);
    }
    const int64_t hist_bytes = ((int64_t(1) << max_depth) - 1) * n_features * 512 * 8;
    // bins (+ the staged rows of a host matrix), per-row state, histograms
    const int64_t bytes = n * n_features * (in_hbm ? 1 : 5) + n * 36 + hist_bytes;
    DS_HIP(hipSetDevice(device));
    if (int status = check_free(bytes, who); status != DS_OK) return status;
    ds_trainer *t = new ds_trainer();
    t->device = device;
    t->n = n;
    t->nf = n_features;
    t->params = ds::TrainParams{max_depth, eta, min_child_weight, reg_lambda, beta};
    t->host_offsets.assign(cut_offsets, cut_offsets + n_features + 1);
    hipDeviceProp_t props;
    if (hipGetDeviceProperties(&props, device) == hipSuccess && props.multiProcessorCount > 0)
        t->compute_units = props.multiProcessorCount;
    int status = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking) == hipSuccess ? DS_OK : DS_E_HIP;
    if (status != DS_OK) ds::set_error("%s: hipStreamCreate failed", who);
    if (status == DS_OK) status = t->cut_offsets.upload(cut_offsets, static_cast<size_t>(n_features) + 1);
    if (status == DS_OK) status = t->cuts.allocate(std::max<size_t>(1, static_cast<size_t>(cut_offsets[n_features])));
    if (status == DS_OK && cut_offsets[n_features] > 0)
        status = t->cuts.upload(cuts, static_cast<size_t>(cut_offsets[n_features]));
    if (status == DS_OK) status = bin_matrix(t, features, in_hbm, n, t->bins);
    if (status == DS_OK) status = t->labels.allocate(n);
    if (status == DS_OK) status = t->leafsum.allocate(n);
    if (status == DS_OK) status = t->probabilities.allocate(n);
    if (status == DS_OK) status = t->node_of.allocate(n);
    if (status == DS_OK) status = t->gh.allocate(2 * n);
    if (status == DS_OK) status = t->hist.allocate(static_cast<size_t>(hist_bytes / 8));
    if (status == DS_OK) status = t->counts.allocate(heap_nodes(max_depth));
    if (status == DS_OK) status = t->nodes.allocate(heap_nodes(max_depth));
    if (status == DS_OK) status = t->candidates.allocate((size_t(1) << (max_depth - 1)) * n_features);
    if (status == DS_OK) status = t->error.allocate(1);
    if (status == DS_OK && hipHostMalloc(reinterpret_cast<void **>(&t->pinned_nodes),
                                         sizeof(ds::Node) * heap_nodes(max_depth)) != hipSuccess) status = DS_E_HIP;
    if (status == DS_OK && hipHostMalloc(reinterpret_cast<void **>(&t->pinned_error), sizeof(unsigned long long)) !=
                               hipSuccess) status = DS_E_HIP;
    if (status == DS_OK && hipMemsetAsync(t->leafsum.ptr, 0, sizeof(float) * n, t->stream) != hipSuccess)
        status = DS_E_HIP;
    if (status == DS_OK && hipStreamSynchronize(t->stream) != hipSuccess) status = DS_E_HIP;
    if (status != DS_OK) {
        delete t;
        return status;
    }
    *out = t;
    return DS_OK;
}

// ds_trainer_set_eval (`who`, features on the host) and ds_trainer_set_eval_device (features in HBM)
int set_eval(const char *who, ds_trainer *trainer, const float *features, bool in_hbm, const float *labels, int64_t n)
{
    DS_REQUIRE(trainer && features && labels, "%s: null argument", who);
    DS_REQUIRE(n >= 1 && n <= INT32_MAX, "%s: n = %lld rows out of range [1, 2^31)", who, (long long)n);
    DS_REQUIRE(trainer->rounds == 0, "%s: the evaluation set must be given before the first round", who);
    for (int64_t r = 0; r < n; ++r)
        DS_REQUIRE(labels[r] == 0.f || labels[r] == 1.f, "%s: label %lld is not 0 or 1", who, (long long)r);
    DS_HIP(hipSetDevice(trainer->device));
    if (int status = check_free(n * trainer->nf * (in_hbm ? 1 : 5) + n * 8, who); status != DS_OK) return status;
    int status = bin_matrix(trainer, features, in_hbm, n, trainer->eval_bins);
    if (status == DS_OK) status = trainer->eval_labels.upload(labels, n);
    if (status == DS_OK) status = trainer->eval_leafsum.allocate(n);
    if (status != DS_OK) return status;
    DS_HIP(hipMemsetAsync(trainer->eval_leafsum.ptr, 0, sizeof(float) * n, trainer->stream));
    DS_HIP(hipStreamSynchronize(trainer->stream));
    trainer->n_eval = n;
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
    for (int64_t r = 0; r < trainer->n; ++r)
        DS_REQUIRE(labels[r] == 0.f || labels[r] == 1.f, "ds_trainer_set_labels: label %lld is not 0 or 1", (long long)r);
    DS_HIP(hipSetDevice(trainer->device));
    DS_HIP(hipMemcpyAsync(trainer->labels.ptr, labels, sizeof(float) * trainer->n, hipMemcpyHostToDevice,
                          trainer->stream));
    DS_HIP(hipStreamSynchronize(trainer->stream));
    trainer->has_labels = true;
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
    if (int status = error.allocate(1); status != DS_OK) return status;
    int32_t errors = 0;
    DS_HIP(hipMemsetAsync(error.ptr, 0, sizeof(int32_t), s));
    const auto grid = [](int64_t items) {
        return dim3(static_cast<unsigned>(std::min<int64_t>((items + ds::kRowThreads - 1) / ds::kRowThreads, 256 * 16)));
    };
    hipLaunchKernelGGL(ds::ds_gather_check_kernel, grid(n_rows), dim3(ds::kRowThreads), 0, s, d_rows, n_rows, n_src,
                       error.ptr);
    DS_HIP(hipGetLastError());
    DS_HIP(hipMemcpyAsync(&errors, error.ptr, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DS_HIP(hipStreamSynchronize(s));
    if (errors != 0) {
        ds::set_error("ds_gather_rows_device: %d row indexes are out of range [0, %lld)", errors, (long long)n_src);
        return DS_E_ARG;
    }
    hipLaunchKernelGGL(ds::ds_gather_rows_kernel, grid(n_rows * n_features), dim3(ds::kRowThreads), 0, s,
                       reinterpret_cast<const uint32_t *>(d_src), n_features, d_rows, n_rows, n_src,
                       reinterpret_cast<uint32_t *>(d_dst));
    DS_HIP(hipGetLastError());
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
    const int64_t slots = heap_nodes(depth), n = t->n;
    hipStream_t stream = t->stream;
    DS_HIP(hipMemsetAsync(t->hist.ptr, 0, t->hist.bytes(), stream));
    DS_HIP(hipMemsetAsync(t->nodes.ptr, 0, t->nodes.bytes(), stream));
    DS_HIP(hipMemsetAsync(t->counts.ptr, 0, t->counts.bytes(), stream));
    DS_HIP(hipMemsetAsync(t->error.ptr, 0, sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(ds::ds_train_gradient_kernel, dim3(row_grid(t, n)), dim3(ds::kRowThreads), 0, stream,
                       t->leafsum.ptr, t->labels.ptr, n, t->base_margin, t->params.beta, t->probabilities.ptr,
                       t->gh.ptr, t->node_of.ptr);
    DS_HIP(hipGetLastError());
    for (int32_t level = 0; level < depth; ++level) {
        const int32_t n_built = level == 0 ? 1 : 1 << (level - 1);
        const int32_t nodes_per_group = std::min(n_built, ds::kHistSlots);
        const int32_t features_per_group = std::min<int32_t>(t->nf, ds::kHistSlots / nodes_per_group);
        const int32_t feature_groups = (t->nf + features_per_group - 1) / features_per_group;
        const int32_t node_groups = (n_built + nodes_per_group - 1) / nodes_per_group;
        const int32_t groups = feature_groups * node_groups;
        // about 4 workgroups per CU in all, each over at least 2048 rows: the LDS adds dominate, the flush (<= 8192
        // global adds per workgroup) stays a small part
        const int64_t chunks = std::max<int64_t>(1, std::min<int64_t>((n + 2047) / 2048,
                                                                      (int64_t(t->compute_units) * 4 + groups - 1) / groups));
        hipLaunchKernelGGL(ds::ds_train_histogram_kernel, dim3(static_cast<unsigned>(chunks), groups),
                           dim3(ds::kHistThreads), 0, stream, t->bins.ptr, t->gh.ptr, t->node_of.ptr, t->counts.ptr,
                           t->nodes.ptr, n, t->nf, level, n_built, nodes_per_group, features_per_group, feature_groups,
                           reinterpret_cast<unsigned long long *>(t->hist.ptr));
        DS_HIP(hipGetLastError());
        hipLaunchKernelGGL(ds::ds_train_split_feature_kernel, dim3(1u << level, t->nf), dim3(256), 0, stream,
                           t->hist.ptr, t->counts.ptr, t->nodes.ptr, t->cut_offsets.ptr, t->nf, level, t->params,
                           t->candidates.ptr);
        DS_HIP(hipGetLastError());
        hipLaunchKernelGGL(ds::ds_train_split_kernel, dim3(((1u << level) + 63) / 64), dim3(64), 0, stream,
                           t->candidates.ptr, t->nodes.ptr, t->nf, level, t->params);
        DS_HIP(hipGetLastError());
        hipLaunchKernelGGL(ds::ds_train_partition_kernel, dim3(row_grid(t, n)), dim3(ds::kRowThreads), 0, stream,
                           t->bins.ptr, t->nodes.ptr, n, level, t->node_of.ptr, t->leafsum.ptr, t->counts.ptr);
        DS_HIP(hipGetLastError());
    }
    if (t->n_eval > 0) {
        hipLaunchKernelGGL(ds::ds_train_eval_kernel, dim3(row_grid(t, t->n_eval)), dim3(ds::kRowThreads), 0, stream,
                           t->eval_bins.ptr, t->nodes.ptr, t->n_eval, t->eval_labels.ptr, t->base_margin,
                           t->eval_leafsum.ptr, t->error.ptr);
        DS_HIP(hipGetLastError());
    }
    DS_HIP(hipMemcpyAsync(t->pinned_nodes, t->nodes.ptr, sizeof(ds::Node) * slots, hipMemcpyDeviceToHost, stream));
    DS_HIP(hipMemcpyAsync(t->pinned_error, t->error.ptr, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    DS_HIP(hipStreamSynchronize(stream));   // the round's one host sync
    for (int64_t i = 0; i < slots; ++i) {
        const ds::Node &node = t->pinned_nodes[i];
        node_info[4 * i] = node.state;
        node_info[4 * i + 1] = node.feature;
        node_info[4 * i + 2] = node.bin;
        node_info[4 * i + 3] = node.default_left;
        node_leaf[i] = node.leaf;
    }
    if (eval_error) *eval_error = t->n_eval > 0 ? static_cast<int64_t>(*t->pinned_error) : -1;
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
        for (size_t r = 0; r < count; ++r) out[r] = t->base_margin + out[r];   // ds_forest.hip: base + sum of leaves
        return DS_OK;
    };
    if (margins) {
        if (int status = add_base(margins, t->leafsum.ptr, n); status != DS_OK) return status;
    }
    if (eval_margins) {
        if (int status = add_base(eval_margins, t->eval_leafsum.ptr, static_cast<size_t>(t->n_eval)); status != DS_OK)
            return status;
    }
    return DS_OK;
}

}  // extern "C"
