// Why the model gave a pair its margin: node cover counted on the device, and per-feature contributions of every row
// ("Contributions").
//
// Cover: the rows of a workgroup are staged in LDS; a row adds 1 to the 64-bit counter of the leaf
// it reaches in every tree (integer atomics: exact, whatever the schedule), and a second kernel sums the inner nodes from
// their children, one thread per tree (children follow their parent in node order, so one backward sweep does it).  The
// root of every tree therefore never sees an atomic.
//
// Contributions: path-dependent TreeSHAP (Lundberg, Erion and Lee 2018, Algorithm 2) without recursion.  When the cover
// is installed every tree is taken apart on the host into its root-to-leaf paths; the splits of a path on one feature
// merge into one element (an interval of the value, a NaN rule and the product of the cover fractions), which is what
// Algorithm 2's unwind-and-extend of a repeated feature amounts to.  One thread per row, one wavefront per workgroup:
// every lane walks the same path at the same time, so the path data are wave-uniform loads, and a lane keeps only the
// EXTEND weights (at most 17 float64, indexed by fully unrolled loops: registers, no scratch) and a bit per element.
// The row's sums live in LDS as float64 [feature][lane] next to the staged rows [feature][lane].  Paths are visited in
// tree order, leaves in node order, elements in path order, and every sum is a plain sequential float64 addition: the
// same bits whatever the grid.  approximate = 1 (Saabas) walks the row's own path and adds the change of the subtree mean.
#include "ds_launch.h"
#include "ds_forest.h"

#include <cmath>

namespace ds {

constexpr int kCoverMaxBlocks = 4096;            // default grid cap of the cover kernel (256 rows per workgroup)
constexpr int kContributionsThreads = 64;        // one wavefront: the rows of a workgroup
constexpr int kContributionsMaxBlocks = 8192;    // default grid cap of the contributions kernels
constexpr int kLaneStride = kContributionsThreads + 1;  // [feature][lane] images in LDS, padded: the transposing copies spread over the banks

struct CoverArgs {
    ForestView forest;
    const float *rows;
    unsigned long long *counts;
    int64_t n;
};

__global__ __launch_bounds__(kForestThreads) void ds_forest_cover_kernel(CoverArgs a)
{
    extern __shared__ float staged[];  // [kForestThreads][n_features + 1]
    const int stride = a.forest.n_features + 1;
    for (int64_t first = static_cast<int64_t>(blockIdx.x) * kForestThreads; first < a.n;
         first += static_cast<int64_t>(gridDim.x) * kForestThreads) {
        const int rows_here =
            forest_stage_rows<kForestThreads>(a.rows, a.n, first, a.forest.n_features, staged, stride, 1);
        __syncthreads();
        if (static_cast<int>(threadIdx.x) < rows_here) {
            const float *row = staged + threadIdx.x * stride;
            for (int32_t t = 0; t < a.forest.n_trees; ++t) {
                const int64_t leaf = forest_walk(a.forest.nodes, a.forest.threshold, a.forest.tree_offsets[t], row);
                atomicAdd(a.counts + leaf, 1ull);
            }
        }
    }
}

// inner nodes = the sum of their two children, backwards: a child's id is above its parent's
__global__ void ds_forest_cover_sum_kernel(const int4 *nodes, const int64_t *tree_offsets, int32_t n_trees,
                                           unsigned long long *counts)
{
    for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < n_trees;
         t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int64_t begin = tree_offsets[t], end = tree_offsets[t + 1];
        for (int64_t i = end - 1; i >= begin; --i) {
            const int4 info = nodes[i];
            if (info.x >= 0) counts[i] = counts[begin + info.y] + counts[begin + info.z];
        }
    }
}

// coefficients of EXTEND to l elements (up, back) and of UNWIND at l elements (one, back, zero): [l][j] for j < l
struct UnwindTable {
    double up[kContributionsMaxDepth + 1][kContributionsMaxDepth];     // (j + 1) / (l + 1)
    double one[kContributionsMaxDepth + 1][kContributionsMaxDepth];    // (l + 1) / (j + 1)
    double back[kContributionsMaxDepth + 1][kContributionsMaxDepth];   // (l - j) / (l + 1)
    double zero[kContributionsMaxDepth + 1][kContributionsMaxDepth];   // (l + 1) / (l - j)
};

constexpr UnwindTable make_unwind_table()
{
    UnwindTable table{};
    for (int l = 0; l <= kContributionsMaxDepth; ++l)
        for (int j = 0; j < kContributionsMaxDepth; ++j) {
            const bool used = j < l;
            table.up[l][j] = used ? (j + 1.0) / (l + 1.0) : 0.0;
            table.one[l][j] = used ? (l + 1.0) / (j + 1.0) : 0.0;
            table.back[l][j] = used ? static_cast<double>(l - j) / (l + 1.0) : 0.0;
            table.zero[l][j] = used ? (l + 1.0) / static_cast<double>(l - j) : 0.0;
        }
    return table;
}

__constant__ UnwindTable kUnwind = make_unwind_table();

struct ContributionsArgs {
    ForestView forest;
    const int32_t *path_start;
    const double *path_leaf;
    const PathElement *elements;
    const double *node_mean;
    const float *rows;
    double *out;            // [n][n_features + 1]
    double bias;
    int64_t n, n_paths;
};

// The contributions of one row over all paths, added to sums[feature * kLaneStride] (this lane's column).
template <int M>
__device__ __forceinline__ void shap_row(const ContributionsArgs &a, const float *row, double *sums)
{
    for (int64_t p = 0; p < a.n_paths; ++p) {
        const int32_t e0 = a.path_start[p];
        const int32_t m = a.path_start[p + 1] - e0;
        if (m == 0) continue;  // a single-leaf tree: all of it is bias
        const double leaf = a.path_leaf[p];
        // EXTEND, element after element: w[0..m] are the weights of the subsets by size; index 0 is the algorithm's
        // root element (zero and one fraction 1)
        double w[M + 1];
#pragma unroll
        for (int i = 0; i <= M; ++i) w[i] = 0.0;
        w[0] = 1.0;
        uint32_t follows = 0;
        for (int l = 1; l <= m; ++l) {
            const PathElement element = a.elements[e0 + l - 1];
            const float value = row[element.feature * kLaneStride];
            const bool one = (value != value) ? element.nan_follows != 0
                                              : (!(value < element.lo) && !(value >= element.hi));
            follows |= static_cast<uint32_t>(one) << (l - 1);
#pragma unroll
            for (int i = M - 1; i >= 0; --i) {  // w is indexed by the unrolled counter only: it stays in registers
                if (i < l) {
                    if (one) w[i + 1] = w[i + 1] + w[i] * kUnwind.up[l][i];
                    w[i] = element.zero_fraction * w[i] * kUnwind.back[l][i];
                }
            }
        }
        double top = 0.0;
#pragma unroll
        for (int i = 1; i <= M; ++i)
            if (i == m) top = w[i];
        // UNWIND each element in turn and sum what is left
        for (int i = 1; i <= m; ++i) {
            const PathElement element = a.elements[e0 + i - 1];
            const bool one = (follows >> (i - 1)) & 1u;
            double total = 0.0, next = top;
#pragma unroll
            for (int j = M - 1; j >= 0; --j) {
                if (j < m) {
                    if (one) {
                        const double part = next * kUnwind.one[m][j];
                        total = total + part;
                        next = w[j] - part * element.zero_fraction * kUnwind.back[m][j];
                    } else {
                        total = total + w[j] * element.zero_reciprocal * kUnwind.zero[m][j];
                    }
                }
            }
            double *sum = sums + element.feature * kLaneStride;
            *sum = *sum + total * ((one ? 1.0 : 0.0) - element.zero_fraction) * leaf;
        }
    }
}

// Saabas: along the row's own path every split adds the change of the subtree mean to its feature
__device__ __forceinline__ void saabas_row(const ContributionsArgs &a, const float *row, double *sums)
{
    for (int32_t t = 0; t < a.forest.n_trees; ++t) {
        const int64_t root = a.forest.tree_offsets[t];
        int64_t node = root;
        int4 info = a.forest.nodes[node];
        double mean = a.node_mean[node];
        while (info.x >= 0) {
            node = root + forest_branch(info, row[info.x * kLaneStride], a.forest.threshold + node);
            const double child = a.node_mean[node];
            double *sum = sums + info.x * kLaneStride;
            *sum = *sum + (child - mean);
            mean = child;
            info = a.forest.nodes[node];
        }
    }
}

// M > 0: TreeSHAP for paths of up to M elements; M == 0: Saabas
template <int M>
__global__ __launch_bounds__(kContributionsThreads) void ds_contributions_kernel(ContributionsArgs a)
{
    extern __shared__ double shared[];  // sums [n_features][kLaneStride] float64, then rows [n_features][kLaneStride] float32
    const int n_features = a.forest.n_features;
    double *sums = shared;
    float *staged = reinterpret_cast<float *>(shared + n_features * kLaneStride);
    const int lane = threadIdx.x;
    const int width = n_features + 1;
    for (int64_t first = static_cast<int64_t>(blockIdx.x) * kContributionsThreads; first < a.n;
         first += static_cast<int64_t>(gridDim.x) * kContributionsThreads) {
        const int rows_here =   // transposed; its barrier also ends the store loop's reads of the sums
            forest_stage_rows<kContributionsThreads>(a.rows, a.n, first, n_features, staged, 1, kLaneStride);
        for (int f = 0; f < n_features; ++f) sums[f * kLaneStride + lane] = 0.0;
        __syncthreads();
        if (lane < rows_here) {
            if constexpr (M > 0) shap_row<M>(a, staged + lane, sums + lane);
            else saabas_row(a, staged + lane, sums + lane);
        }
        __syncthreads();
        for (int e = lane; e < rows_here * width; e += kContributionsThreads) {  // coalesced store
            const int r = e / width, f = e - r * width;
            a.out[first * width + e] = f < n_features ? sums[f * kLaneStride + r] : a.bias;
        }
    }
}

// per query the candidate with the highest probability, the first on a tie (predict.py:239-242), and how many hold it
__global__ void ds_best_pairs_kernel(const int32_t *rows, const float *probabilities, int64_t n_queries, int32_t k,
                                     int64_t *best_pair, int32_t *best_row, float *best_probability, int32_t *best_count)
{
    for (int64_t q = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; q < n_queries;
         q += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        float best = probabilities[q * k];
        int where = 0, count = 1;
        for (int j = 1; j < k; ++j) {
            const float p = probabilities[q * k + j];
            if (p > best) { best = p; where = j; count = 1; }
            else if (p == best) ++count;
        }
        best_pair[q] = q * k + where;
        best_row[q] = rows[q * k + where];
        best_probability[q] = best;
        best_count[q] = count;
    }
}

// Every tree a proper binary tree (two different children, `missing` one of them, one parent per node): what cover
// sums and path decomposition rest on (declared in ds_forest.h).  check_shape keeps the answer in forest->parent.
int forest_parents(const ds_forest *forest, const char *what, std::vector<int32_t> &parent)
{
    DS_REQUIRE(forest->n_nodes <= INT32_MAX, "%s: %lld nodes", what, (long long)forest->n_nodes);
    parent.assign(static_cast<size_t>(forest->n_nodes), -1);
    for (int32_t t = 0; t < forest->n_trees; ++t) {
        const int64_t begin = forest->h_offsets[t], end = forest->h_offsets[t + 1];
        for (int64_t i = begin; i < end; ++i) {
            const int4 info = forest->h_nodes[static_cast<size_t>(i)];
            if (info.x < 0) continue;
            DS_REQUIRE(info.y != info.z && (info.w == info.y || info.w == info.z),
                       "%s: node %lld of tree %d is no binary split (yes %d, no %d, missing %d)", what,
                       (long long)(i - begin), t, info.y, info.z, info.w);
            for (const int child : {info.y, info.z}) {
                DS_REQUIRE(parent[static_cast<size_t>(begin + child)] < 0, "%s: node %d of tree %d has two parents", what,
                           child, t);
                parent[static_cast<size_t>(begin + child)] = static_cast<int32_t>(i);
            }
        }
        DS_REQUIRE(parent[static_cast<size_t>(begin)] < 0, "%s: the root of tree %d is somebody's child", what, t);
    }
    return DS_OK;
}

static int check_shape(ds_forest *forest, const char *what)
{
    if (forest->shape_checked) return DS_OK;
    std::vector<int32_t> parent;
    DS_TRY(forest_parents(forest, what, parent));
    forest->parent = std::move(parent);
    forest->shape_checked = 1;
    return DS_OK;
}

static void drop_prepared(ds_forest *forest)
{
    forest->prepared = false;
    forest->path_start.release();
    forest->path_leaf.release();
    forest->elements.release();
    forest->node_mean.release();
}

// The cover of every node as float64: the caller's values, or the counters (behind a synchronisation of the device).
static int read_cover(ds_forest *forest, std::vector<double> &cover, const char *what)
{
    DS_REQUIRE(forest->cover_state != ds_forest::kCoverNone, "%s: the forest has no cover", what);
    if (forest->cover_state == ds_forest::kCoverSet) {
        cover = forest->cover;
        return DS_OK;
    }
    std::vector<unsigned long long> counts(static_cast<size_t>(forest->n_nodes));
    DS_HIP(hipSetDevice(forest->device));
    DS_HIP(hipDeviceSynchronize());
    if (forest->n_nodes)
        DS_HIP(hipMemcpy(counts.data(), forest->counts.ptr, counts.size() * sizeof(unsigned long long),
                         hipMemcpyDeviceToHost));
    cover.resize(counts.size());
    for (size_t i = 0; i < counts.size(); ++i) cover[i] = static_cast<double>(counts[i]);
    return DS_OK;
}

// Paths, node means and the bias from the cover: once per installed cover.
static int prepare(ds_forest *forest, const char *what)
{
    if (forest->prepared) return DS_OK;
    int status = check_shape(forest, what);
    if (status != DS_OK) return status;
    std::vector<double> cover;
    status = read_cover(forest, cover, what);
    if (status != DS_OK) return status;
    const std::vector<int4> &nodes = forest->h_nodes;
    std::vector<int32_t> path_start{0};
    std::vector<double> path_leaf;
    std::vector<PathElement> elements;
    std::vector<int64_t> steps;  // the nodes of one path, leaf first
    int32_t max_elements = 0;
    const float none = std::nanf("");
    for (int32_t t = 0; t < forest->n_trees; ++t) {
        const int64_t begin = forest->h_offsets[t], end = forest->h_offsets[t + 1];
        for (int64_t leaf = begin; leaf < end; ++leaf) {
            if (nodes[static_cast<size_t>(leaf)].x >= 0) continue;
            steps.clear();
            for (int64_t node = leaf; node >= 0; node = forest->parent[static_cast<size_t>(node)]) steps.push_back(node);
            if (steps.back() != begin) continue;  // a leaf nothing leads to
            const int64_t depth = static_cast<int64_t>(steps.size()) - 1;
            DS_REQUIRE(depth <= kContributionsMaxDepth, "%s: tree %d is %lld splits deep, %d at most", what, t,
                       (long long)depth, kContributionsMaxDepth);
            const size_t first = elements.size();
            for (int64_t s = depth; s >= 1; --s) {  // from the root down
                const int64_t node = steps[static_cast<size_t>(s)], child = steps[static_cast<size_t>(s - 1)];
                const int4 info = nodes[static_cast<size_t>(node)];
                const double above = cover[static_cast<size_t>(node)], below = cover[static_cast<size_t>(child)];
                DS_REQUIRE(above > 0 && below > 0, "%s: node %lld of tree %d has no cover: every node a path visits needs one",
                           what, (long long)((above > 0 ? child : node) - begin), t);
                size_t at = first;
                while (at < elements.size() && elements[at].feature != info.x) ++at;
                if (at == elements.size()) elements.push_back(PathElement{info.x, 1u, none, none, 1.0, 1.0});
                PathElement &element = elements[at];
                const float cut = forest->h_threshold[static_cast<size_t>(node)];
                const bool yes = child - begin == info.y;
                if (cut != cut) {  // nothing is below a NaN cut: `yes` is never taken, `no` by every value
                    if (yes) { element.lo = INFINITY; element.hi = -INFINITY; }
                } else if (yes) {
                    element.hi = (element.hi != element.hi || cut < element.hi) ? cut : element.hi;
                } else {
                    element.lo = (element.lo != element.lo || cut > element.lo) ? cut : element.lo;
                }
                if (child - begin != info.w) element.nan_follows = 0u;
                element.zero_fraction = element.zero_fraction * (below / above);
            }
            for (size_t at = first; at < elements.size(); ++at)
                elements[at].zero_reciprocal = 1.0 / elements[at].zero_fraction;
            max_elements = std::max<int32_t>(max_elements, static_cast<int32_t>(elements.size() - first));
            DS_REQUIRE(elements.size() <= static_cast<size_t>(INT32_MAX), "%s: too many path elements", what);
            path_start.push_back(static_cast<int32_t>(elements.size()));
            path_leaf.push_back(static_cast<double>(forest->h_threshold[static_cast<size_t>(leaf)]));
        }
    }
    // subtree means, children before parents; a node no path visits keeps 0
    std::vector<double> mean(static_cast<size_t>(forest->n_nodes), 0.0);
    double bias = static_cast<double>(forest->base_margin);
    for (int32_t t = 0; t < forest->n_trees; ++t) {
        const int64_t begin = forest->h_offsets[t], end = forest->h_offsets[t + 1];
        for (int64_t i = end - 1; i >= begin; --i) {
            const int4 info = nodes[static_cast<size_t>(i)];
            if (info.x < 0) {
                mean[static_cast<size_t>(i)] = static_cast<double>(forest->h_threshold[static_cast<size_t>(i)]);
                continue;
            }
            const double above = cover[static_cast<size_t>(i)];
            if (!(above > 0)) continue;
            mean[static_cast<size_t>(i)] =
                cover[static_cast<size_t>(begin + info.y)] / above * mean[static_cast<size_t>(begin + info.y)] +
                cover[static_cast<size_t>(begin + info.z)] / above * mean[static_cast<size_t>(begin + info.z)];
        }
        bias = bias + mean[static_cast<size_t>(begin)];
    }
    DS_HIP(hipSetDevice(forest->device));
    status = forest->path_start.upload(path_start.data(), path_start.size());
    if (status == DS_OK) status = forest->path_leaf.upload(path_leaf.data(), path_leaf.size());
    if (status == DS_OK && path_leaf.empty()) status = forest->path_leaf.allocate(1);
    if (status == DS_OK) status = forest->elements.upload(elements.data(), elements.size());
    if (status == DS_OK && elements.empty()) status = forest->elements.allocate(1);
    if (status == DS_OK) status = forest->node_mean.upload(mean.data(), mean.size());
    if (status == DS_OK && mean.empty()) status = forest->node_mean.allocate(1);
    if (status != DS_OK) {
        drop_prepared(forest);
        return status;
    }
    forest->n_paths = static_cast<int64_t>(path_leaf.size());
    forest->max_elements = max_elements;
    forest->bias = bias;
    forest->prepared = true;
    return DS_OK;
}

template <int M>
static int launch_contributions(const ContributionsArgs &args, int grid, size_t lds, hipStream_t stream)
{
    DS_TRY(ds::allow_dynamic_lds(ds_contributions_kernel<M>, lds));
    DS_LAUNCH(ds_contributions_kernel<M>, dim3(grid), dim3(kContributionsThreads), lds, stream, args);
    return DS_OK;
}

}  // namespace ds

extern "C" {

int ds_forest_option(ds_forest *forest, const char *name, int64_t value)
{
    DS_REQUIRE(forest != nullptr, "ds_forest_option: null forest");
    ds::Option *const table[] = {&forest->max_blocks, &forest->inspect_jobs_per_block, &forest->refresh_lds_nodes};
    return ds::set_option("ds_forest_option", table, name, value);
}

int ds_forest_cover_device(ds_forest *forest, const float *d_rows, int64_t n, void *stream)
{
    DS_REQUIRE(forest != nullptr && n >= 0, "ds_forest_cover_device: bad arguments");
    DS_REQUIRE(n == 0 || d_rows != nullptr, "ds_forest_cover_device: null rows");
    DS_TRY(ds::check_shape(forest, "ds_forest_cover_device"));
    DS_HIP(hipSetDevice(forest->device));
    hipStream_t queue = static_cast<hipStream_t>(stream);
    if (forest->cover_state != ds_forest::kCoverCounted) {  // a fresh count replaces whatever was installed
        DS_TRY(forest->counts.allocate(static_cast<size_t>(std::max<int64_t>(forest->n_nodes, 1))));
        DS_HIP(hipMemsetAsync(forest->counts.ptr, 0, forest->counts.bytes(), queue));
        forest->cover.clear();
        forest->cover_state = ds_forest::kCoverCounted;
    }
    ds::drop_prepared(forest);
    if (n == 0 || forest->n_trees == 0) return DS_OK;
    const ds::CoverArgs args{forest->view(), d_rows, forest->counts.ptr, n};
    const int64_t blocks = (n + ds::kForestThreads - 1) / ds::kForestThreads;
    const int64_t cap = forest->max_blocks.value_or(ds::kCoverMaxBlocks);
    const unsigned grid = ds::grid_cap(blocks, cap);
    const size_t lds = static_cast<size_t>(ds::kForestThreads) * (forest->n_features + 1) * sizeof(float);
    DS_TRY(ds::allow_dynamic_lds(ds::ds_forest_cover_kernel, lds));
    DS_LAUNCH(ds::ds_forest_cover_kernel, dim3(grid), dim3(ds::kForestThreads), lds, queue, args);
    const unsigned sum_grid = ds::grid_cap((forest->n_trees + 63) / 64, cap);
    DS_LAUNCH(ds::ds_forest_cover_sum_kernel, dim3(sum_grid), dim3(64), 0, queue, forest->nodes.ptr,
              forest->tree_offsets.ptr, forest->n_trees, forest->counts.ptr);
    return DS_OK;
}

int ds_forest_cover_set(ds_forest *forest, const double *cover)
{
    DS_REQUIRE(forest != nullptr && (cover != nullptr || forest->n_nodes == 0), "ds_forest_cover_set: null pointer");
    for (int64_t i = 0; i < forest->n_nodes; ++i)
        DS_REQUIRE(std::isfinite(cover[i]) && cover[i] > 0, "ds_forest_cover_set: cover[%lld] = %g is not a positive number",
                   (long long)i, cover[i]);
    DS_HIP(hipSetDevice(forest->device));
    forest->cover.assign(cover, cover + forest->n_nodes);
    forest->counts.release();
    forest->cover_state = ds_forest::kCoverSet;
    ds::drop_prepared(forest);
    return DS_OK;
}

int ds_forest_cover_read(ds_forest *forest, double *cover)
{
    DS_REQUIRE(forest != nullptr && (cover != nullptr || forest->n_nodes == 0), "ds_forest_cover_read: null pointer");
    std::vector<double> values;
    DS_TRY(ds::read_cover(forest, values, "ds_forest_cover_read"));
    if (!values.empty()) std::memcpy(cover, values.data(), values.size() * sizeof(double));
    return DS_OK;
}

int ds_forest_cover_clear(ds_forest *forest)
{
    DS_REQUIRE(forest != nullptr, "ds_forest_cover_clear: null forest");
    DS_HIP(hipSetDevice(forest->device));
    DS_HIP(hipDeviceSynchronize());  // a count may still be running on some stream
    forest->cover.clear();
    forest->counts.release();
    forest->cover_state = ds_forest::kCoverNone;
    ds::drop_prepared(forest);
    return DS_OK;
}

int ds_forest_contributions_device(ds_forest *forest, const float *d_rows, int64_t n, double *d_out, int approximate,
                                   void *stream)
{
    DS_REQUIRE(forest != nullptr && n >= 0, "ds_forest_contributions: bad arguments");
    DS_REQUIRE(approximate == 0 || approximate == 1, "ds_forest_contributions: approximate = %d is neither 0 nor 1",
               approximate);
    DS_REQUIRE(forest->cover_state != ds_forest::kCoverNone, "ds_forest_contributions: the forest has no cover");
    DS_TRY(ds::prepare(forest, "ds_forest_contributions"));
    if (n == 0) return DS_OK;
    DS_REQUIRE(d_rows && d_out, "ds_forest_contributions: null pointer");
    DS_HIP(hipSetDevice(forest->device));
    ds::ContributionsArgs args;
    args.forest = forest->view();
    args.path_start = forest->path_start.ptr;
    args.path_leaf = forest->path_leaf.ptr;
    args.elements = forest->elements.ptr;
    args.node_mean = forest->node_mean.ptr;
    args.rows = d_rows;
    args.out = d_out;
    args.bias = forest->bias;
    args.n = n;
    args.n_paths = forest->n_paths;
    const int64_t blocks = (n + ds::kContributionsThreads - 1) / ds::kContributionsThreads;
    const int64_t cap = forest->max_blocks.value_or(ds::kContributionsMaxBlocks);
    const int grid = static_cast<int>(ds::grid_cap(blocks, cap));
    const size_t lds = static_cast<size_t>(forest->n_features) * ds::kLaneStride * (sizeof(double) + sizeof(float));
    hipStream_t queue = static_cast<hipStream_t>(stream);
    if (approximate) return ds::launch_contributions<0>(args, grid, lds, queue);
    if (forest->max_elements <= 8) return ds::launch_contributions<8>(args, grid, lds, queue);
    return ds::launch_contributions<ds::kContributionsMaxDepth>(args, grid, lds, queue);
}

int ds_forest_contributions(ds_forest *forest, const float *rows, int64_t n, double *out, int approximate)
{
    DS_REQUIRE(forest != nullptr && n >= 0, "ds_forest_contributions: bad arguments");
    DS_REQUIRE(n == 0 || (rows && out), "ds_forest_contributions: null pointer");
    DS_HIP(hipSetDevice(forest->device));
    ds::Scratch scratch;
    const float *d_rows = nullptr;
    double *d_out = nullptr;
    const size_t width = static_cast<size_t>(forest->n_features) + 1;
    scratch.stage(&d_rows, rows, static_cast<size_t>(n) * forest->n_features);
    scratch.add(&d_out, static_cast<size_t>(n) * width);
    DS_TRY(scratch.allocate("ds_forest_contributions"));
    DS_TRY(ds_forest_contributions_device(forest, d_rows, n, d_out, approximate, nullptr));
    DS_HIP(hipDeviceSynchronize());
    if (n) DS_HIP(hipMemcpy(out, d_out, sizeof(double) * static_cast<size_t>(n) * width, hipMemcpyDeviceToHost));
    return DS_OK;
}

int ds_best_pairs_device(const int32_t *d_rows, const float *d_probabilities, int64_t n_queries, int32_t k,
                         int64_t *d_best_pair, int32_t *d_best_row, float *d_best_probability, int32_t *d_best_count,
                         void *stream)
{
    DS_REQUIRE(n_queries >= 0 && k >= 1, "ds_best_pairs_device: bad query count / k");
    if (n_queries == 0) return DS_OK;
    DS_REQUIRE(d_rows && d_probabilities && d_best_pair && d_best_row && d_best_probability && d_best_count,
               "ds_best_pairs_device: null pointer");
    const int64_t blocks = std::min<int64_t>((n_queries + 255) / 256, 4096);
    DS_LAUNCH(ds::ds_best_pairs_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0,
              static_cast<hipStream_t>(stream), d_rows, d_probabilities, n_queries, k, d_best_pair, d_best_row,
              d_best_probability, d_best_count);
    return DS_OK;
}

}  // extern "C"
