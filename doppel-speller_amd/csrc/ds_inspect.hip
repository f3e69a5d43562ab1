// What the model needs and how it bends ("Model inspection"): the forest applied to a matrix under
// a table of JOBS, each of which changes one value of every row before the walk, and five integer sums per job.
//
//   BASELINE  the row as it is
//   PERMUTE   row[feature] = rows[perm(i)][feature]: the column shuffled by a closed-form permutation of (seed, feature,
//             repeat, n), a 4-round Feistel network over 2^(2b) >= n with cycle walking, keyed by the sampling stream
//   OVERRIDE  row[feature] = value (any float32, NaN and the infinities included)
//
// One thread per row.  The rows of a workgroup are staged in LDS, once per row block; the workgroup then runs its share
// of the jobs over them: a thread saves its row's value, writes the replacement (for PERMUTE one gathered float), walks
// the forest and puts the value back.  Nothing but the thread's own row is touched, so the job loop holds no barrier.
// Per job and wave the five terms are summed over the lanes and one lane adds them to the job's 64-bit counters in HBM.
// The grid is row blocks x job groups (an evaluation set of ten thousand rows is only forty row blocks); both
// dimensions stride, and every sum is an integer sum, so no number depends on the split.
#include "ds_launch.h"
#include "ds_forest.h"
#include "ds_metrics.h"
#include "ds_train.h"
#include "ds_wave.h"

#include <cmath>

namespace ds {

constexpr int kInspectMaxRowBlocks = 4096;       // default cap of the row dimension of the grid
constexpr int kInspectTargetBlocks = 2048;       // row blocks x job groups the default split aims at (2 workgroups of
                                                 // 68.6 KB fit a CU's LDS: four rounds of 512)
constexpr int kInspectMaxJobGroups = 65535;      // gridDim.y
constexpr int64_t kInspectRowsMax = int64_t(1) << 31;
constexpr uint32_t kInspectRepeatsMax = 1u << 16;
constexpr int kInspectCounters = DS_INSPECT_COUNTERS;

struct InspectArgs {
    const int4 *nodes;
    const float *threshold;
    const int64_t *tree_offsets;
    const float *rows;
    const float *target;              // nullable: every label 0
    const ds_inspect_job *jobs;
    unsigned long long *out;          // [n_jobs][5]: tp, tn, fp, fn, margin_sum (two's complement)
    int64_t n;
    uint64_t seed;
    double cut;                       // forest_positive's
    int32_t n_trees, n_features, n_jobs, jobs_per_block, n_groups;
    float base_margin;
};

// The keys and the geometry of one PERMUTE job's permutation of [0, n).
struct Permutation {
    uint64_t key[4];
    uint64_t n, mask;
    int b;
};

__host__ __device__ inline Permutation make_permutation(uint64_t seed, uint32_t feature, uint32_t repeat, uint64_t n)
{
    Permutation p;
    p.n = n;
    int bits = 0;   // bit_length(n - 1)
    for (uint64_t v = n > 0 ? n - 1 : 0; v; v >>= 1) ++bits;
    p.b = bits + 1 >= 2 ? (bits + 1) / 2 : 1;
    p.mask = (uint64_t(1) << p.b) - 1;
    for (uint64_t j = 0; j < 4; ++j)
        p.key[j] = sample_key(seed, DS_INSPECT_PURPOSE_PERMUTE,
                              (static_cast<uint64_t>(repeat) << 40) | (static_cast<uint64_t>(feature) << 32) | j);
    return p;
}

__host__ __device__ inline uint64_t permute_row(const Permutation &p, uint64_t i)
{
    if (p.n <= 1) return 0;
    uint64_t x = i;
    do {   // cycle walking: the network is a bijection of [0, 2^(2b)), so the walk from i < n comes back below n
        uint64_t left = x >> p.b, right = x & p.mask;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t next = left ^ (mix64(p.key[j] ^ right) & p.mask);
            left = right;
            right = next;
        }
        x = (left << p.b) | right;
    } while (x >= p.n);
    return x;
}

// Trees of a row walked at a time.  Measured once on an MI355X (331 jobs x 11,141 rows x 303 trees; DESIGN.md section 8,
// "Model inspection"): 1 tree 9.35 ms, 2 trees 7.06 ms, 4 trees 7.95 ms, 8 trees 7.86 ms.
constexpr int kInspectTrees = 2;

// forest_leaf_sum (ds_forest.h) with K trees of the row in flight: the same walks and the same float32 additions in
// the same order, so the same bits.  68.6 KB of staged rows leave a CU two workgroups, two waves per SIMD, and a walk is
// a chain of dependent loads from L2; K independent chains per thread overlap them where more waves cannot, and a
// node's split value is requested together with the node, not after it.  A chain that has reached its leaf keeps
// reloading it (from cache) until the K trees of all lanes are done.
template <int K>
__device__ inline float forest_leaf_sum_interleaved(const int4 *nodes, const float *threshold, const int64_t *tree_offsets,
                                                    int32_t n_trees, const float *row)
{
    float sum = 0.f;
    int32_t t = 0;
    for (; t + K <= n_trees; t += K) {
        int64_t root[K], node[K];
        int4 info[K];
        float cut[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            root[k] = tree_offsets[t + k];
            node[k] = root[k];
            info[k] = nodes[node[k]];
            cut[k] = threshold[node[k]];
        }
        for (;;) {
            bool inner = false;
#pragma unroll
            for (int k = 0; k < K; ++k) inner |= info[k].x >= 0;
            if (!inner) break;
            float value[K];
#pragma unroll
            for (int k = 0; k < K; ++k) value[k] = row[info[k].x >= 0 ? info[k].x : 0];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                // forest_branch's rule, written out: through the function (by value, by pointer, forced inline or not)
                // hipcc sinks a chain's LDS read and selects under a branch on its info.x, the chains no longer issue
                // together, and the 331-job shape above measured 7.80 ms against 7.31 ms
                const int next = (value[k] != value[k]) ? info[k].w : (value[k] < cut[k] ? info[k].y : info[k].z);
                if (info[k].x >= 0) node[k] = root[k] + next;
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                info[k] = nodes[node[k]];
                cut[k] = threshold[node[k]];
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) sum = sum + cut[k];   // tree order
    }
    for (; t < n_trees; ++t)   // the trees left over, one at a time
        sum = sum + threshold[forest_walk(nodes, threshold, tree_offsets[t], row)];
    return sum;
}

__global__ __launch_bounds__(kForestThreads) void ds_forest_inspect_kernel(InspectArgs a)
{
    extern __shared__ float staged[];  // [kForestThreads][n_features + 1]
    const int stride = a.n_features + 1;
    const int lane = threadIdx.x & 63;
    for (int64_t first = static_cast<int64_t>(blockIdx.x) * kForestThreads; first < a.n;
         first += static_cast<int64_t>(gridDim.x) * kForestThreads) {
        const int rows_here =
            forest_stage_rows<kForestThreads>(a.rows, a.n, first, a.n_features, staged, stride, 1);
        __syncthreads();
        if (static_cast<int>(threadIdx.x & ~63u) >= rows_here) continue;   // a wave without rows (the barriers are above)
        const bool active = static_cast<int>(threadIdx.x) < rows_here;
        const int64_t i = first + threadIdx.x;
        float *row = staged + threadIdx.x * stride;
        const bool actual = active && a.target != nullptr && a.target[i] != 0.f;
        for (int32_t group = blockIdx.y; group < a.n_groups; group += gridDim.y) {
            const int32_t begin = group * a.jobs_per_block;
            const int32_t end = begin + a.jobs_per_block < a.n_jobs ? begin + a.jobs_per_block : a.n_jobs;
            for (int32_t j = begin; j < end; ++j) {
                const ds_inspect_job job = a.jobs[j];   // wave-uniform
                unsigned long long tp = 0, tn = 0, fp = 0, fn = 0;
                long long quantised = 0;
                if (active) {
                    float saved = 0.f;
                    if (job.kind != DS_INSPECT_BASELINE) {
                        saved = row[job.feature];
                        float replacement = job.value;
                        if (job.kind == DS_INSPECT_PERMUTE) {
                            const Permutation p = make_permutation(a.seed, static_cast<uint32_t>(job.feature), job.repeat,
                                                                   static_cast<uint64_t>(a.n));
                            const uint64_t from = permute_row(p, static_cast<uint64_t>(i));
                            replacement = a.rows[static_cast<int64_t>(from) * a.n_features + job.feature];
                        }
                        row[job.feature] = replacement;
                    }
                    const float margin =
                        a.base_margin + forest_leaf_sum_interleaved<kInspectTrees>(
                                                             a.nodes, a.threshold, a.tree_offsets, a.n_trees, row);
                    if (job.kind != DS_INSPECT_BASELINE) row[job.feature] = saved;
                    const bool positive = forest_positive(forest_probability(margin), a.cut);
                    tp = positive && actual;
                    tn = !positive && !actual;
                    fp = positive && !actual;
                    fn = !positive && actual;
                    const double m = margin;
                    if (m == m) quantised = llrint(fmin(fmax(m, -kLoglossCap), kLoglossCap) * kLoglossScale);
                }
                tp = wave_sum(tp);
                tn = wave_sum(tn);
                fp = wave_sum(fp);
                fn = wave_sum(fn);
                const unsigned long long sum = wave_sum(static_cast<unsigned long long>(quantised));
                if (lane == 0) {
                    unsigned long long *out = a.out + static_cast<int64_t>(j) * kInspectCounters;
                    if (tp) atomicAdd(out + 0, tp);
                    if (tn) atomicAdd(out + 1, tn);
                    if (fp) atomicAdd(out + 2, fp);
                    if (fn) atomicAdd(out + 3, fn);
                    if (sum) atomicAdd(out + 4, sum);
                }
            }
        }
    }
}

// The checks of a job table that need no forest: kinds, and features and repeats within the limits of the rule.
static int check_jobs(const char *what, const ds_inspect_job *jobs, int32_t n_jobs, int32_t n_features)
{
    for (int32_t j = 0; j < n_jobs; ++j) {
        const ds_inspect_job &job = jobs[j];
        DS_REQUIRE(job.kind == DS_INSPECT_BASELINE || job.kind == DS_INSPECT_PERMUTE || job.kind == DS_INSPECT_OVERRIDE,
                   "%s: job %d has the unknown kind %d", what, j, job.kind);
        if (job.kind == DS_INSPECT_BASELINE) continue;
        DS_REQUIRE(job.feature >= 0 && job.feature < n_features, "%s: job %d names feature %d outside [0, %d)", what, j,
                   job.feature, n_features);
        DS_REQUIRE(job.kind != DS_INSPECT_PERMUTE || job.repeat < kInspectRepeatsMax,
                   "%s: job %d has repeat %u, below %u is allowed", what, j, job.repeat, kInspectRepeatsMax);
    }
    return DS_OK;
}

static int check_scalars(const char *what, int64_t n, int32_t n_jobs, double threshold)
{
    DS_REQUIRE(n_jobs >= 0, "%s: n_jobs = %d is negative", what, n_jobs);
    DS_REQUIRE(n >= 0 && n <= kInspectRowsMax, "%s: n = %lld outside [0, 2^31]", what, (long long)n);
    DS_REQUIRE(threshold > 0.0 && threshold < 1.0, "%s: threshold = %g is not in (0, 1)", what, threshold);
    return DS_OK;
}

// Zeroes the counters and launches the kernel over a job table that has been checked against the forest.
static int inspect_enqueue(ds_forest *forest, const float *d_rows, int64_t n, const float *d_target,
                           const ds_inspect_job *d_jobs, int32_t n_jobs, uint64_t seed, double threshold,
                           unsigned long long *d_out, hipStream_t stream)
{
    DS_HIP(hipSetDevice(forest->device));
    DS_HIP(hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * kInspectCounters * static_cast<size_t>(n_jobs), stream));
    if (n == 0) return DS_OK;
    InspectArgs args;
    args.nodes = forest->nodes.ptr;
    args.threshold = forest->threshold.ptr;
    args.tree_offsets = forest->tree_offsets.ptr;
    args.rows = d_rows;
    args.target = d_target;
    args.jobs = d_jobs;
    args.out = d_out;
    args.n = n;
    args.seed = seed;
    args.cut = threshold;
    args.n_trees = forest->n_trees;
    args.n_features = forest->n_features;
    args.n_jobs = n_jobs;
    args.base_margin = forest->base_margin;
    const int64_t blocks = (n + kForestThreads - 1) / kForestThreads;
    const int64_t row_grid = grid_cap(blocks, forest->max_blocks.value_or(kInspectMaxRowBlocks));
    int64_t per_block = forest->inspect_jobs_per_block.get();
    if (per_block <= 0) {   // enough workgroups for every CU, and as few stagings of a row block as that allows
        const int64_t groups = std::min<int64_t>(n_jobs, (kInspectTargetBlocks + row_grid - 1) / row_grid);
        per_block = (n_jobs + groups - 1) / groups;
    }
    per_block = std::min<int64_t>(per_block, n_jobs);
    args.jobs_per_block = static_cast<int32_t>(per_block);
    args.n_groups = static_cast<int32_t>((n_jobs + per_block - 1) / per_block);
    const int group_grid = std::min<int>(args.n_groups, kInspectMaxJobGroups);
    const size_t lds = static_cast<size_t>(kForestThreads) * (forest->n_features + 1) * sizeof(float);
    DS_TRY(ds::allow_dynamic_lds(ds_forest_inspect_kernel, lds));
    DS_LAUNCH(ds_forest_inspect_kernel, dim3(static_cast<unsigned>(row_grid), static_cast<unsigned>(group_grid)),
              dim3(kForestThreads), lds, stream, args);
    return DS_OK;
}

}  // namespace ds

extern "C" {

int ds_forest_inspect_device(ds_forest *forest, const float *d_rows, int64_t n, const float *d_target,
                             const ds_inspect_job *d_jobs, int32_t n_jobs, uint64_t seed, double threshold,
                             unsigned long long *d_out, void *stream)
{
    const char *what = "ds_forest_inspect_device";
    DS_TRY(ds::check_scalars(what, n, n_jobs, threshold));
    DS_REQUIRE(forest != nullptr, "%s: null forest", what);
    if (n_jobs == 0) return DS_OK;
    DS_REQUIRE(d_jobs != nullptr && d_out != nullptr && (n == 0 || d_rows != nullptr), "%s: null pointer", what);
    DS_HIP(hipSetDevice(forest->device));
    hipStream_t queue = static_cast<hipStream_t>(stream);
    // the table lies in HBM: it is read back and checked before anything walks a tree by it
    std::vector<ds_inspect_job> jobs(static_cast<size_t>(n_jobs));
    DS_HIP(hipMemcpyAsync(jobs.data(), d_jobs, jobs.size() * sizeof(ds_inspect_job), hipMemcpyDeviceToHost, queue));
    DS_HIP(hipStreamSynchronize(queue));
    DS_TRY(ds::check_jobs(what, jobs.data(), n_jobs, forest->n_features));
    return ds::inspect_enqueue(forest, d_rows, n, d_target, d_jobs, n_jobs, seed, threshold, d_out, queue);
}

int ds_forest_inspect(ds_forest *forest, const float *rows, int64_t n, const float *target, const ds_inspect_job *jobs,
                      int32_t n_jobs, uint64_t seed, double threshold, unsigned long long *out)
{
    const char *what = "ds_forest_inspect";
    int status = ds::check_scalars(what, n, n_jobs, threshold);
    if (status != DS_OK) return status;
    DS_REQUIRE(n_jobs == 0 || (jobs != nullptr && out != nullptr), "%s: null pointer", what);
    DS_REQUIRE(n == 0 || n_jobs == 0 || rows != nullptr, "%s: null pointer", what);
    status = ds::check_jobs(what, jobs, n_jobs, ds::kForestFeaturesMax);   // what can be refused without a forest
    if (status != DS_OK) return status;
    DS_REQUIRE(forest != nullptr, "%s: null forest", what);
    status = ds::check_jobs(what, jobs, n_jobs, forest->n_features);
    if (status != DS_OK) return status;
    if (n_jobs == 0) return DS_OK;
    const size_t counters = static_cast<size_t>(n_jobs) * ds::kInspectCounters;
    if (n == 0) {
        std::memset(out, 0, counters * sizeof(unsigned long long));
        return DS_OK;
    }
    DS_HIP(hipSetDevice(forest->device));
    ds::Scratch scratch;
    const float *d_rows = nullptr, *d_target = nullptr;
    const ds_inspect_job *d_jobs = nullptr;
    unsigned long long *d_out = nullptr;
    scratch.stage(&d_rows, rows, static_cast<size_t>(n) * forest->n_features);
    if (target) scratch.stage(&d_target, target, static_cast<size_t>(n));
    scratch.stage(&d_jobs, jobs, static_cast<size_t>(n_jobs));
    scratch.add(&d_out, counters);
    DS_TRY(scratch.allocate(what));
    DS_TRY(ds::inspect_enqueue(forest, d_rows, n, d_target, d_jobs, n_jobs, seed, threshold, d_out, nullptr));
    DS_HIP(hipDeviceSynchronize());
    DS_HIP(hipMemcpy(out, d_out, counters * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return DS_OK;
}

}  // extern "C"
