// Threshold sweep ("Threshold sweep"): the decision rule of Prediction replayed for every cell of a
// grid of T Levenshtein thresholds x U probability thresholds over scores that depend on neither, and the four outcome
// counters of the reference's get-predictions-accuracy (cli.py:107-120) per cell, added into int64 counters in HBM.
//
// The rule for query q at cell (t, u) (predict.py:97-113, :163-183, :244-252; ds_exact_matches_device,
// ds_close_best_kernel, ds_select_matches_kernel), a stage's row counting only when it is >= 0:
//   exact   exact[q];
//   close   value(t) of candidate j = 0 when t > d[j], r[j] when r[j] > t, else s[j] (ds_close_parts_device); among the
//           candidates with value(t) > t the maximum, and its row when exactly one candidate holds it;
//   model   the maximum float32 probability of the k candidates (a NaN in front: none; a NaN behind it is passed over,
//           as the sequential scan of ds_select_matches_kernel does), its row when exactly one candidate holds it and
//           it is > prob[u];
//   none    -1.
// Counter 0: prediction != -1 and == actual[q]; 1: != -1 and != actual[q]; 2: -1 and actual[q] < 0; 3: -1 and
// actual[q] >= 0.
//
// Only the model stage reads u, and (row, maximum, unique) do not depend on the cell: per (query, t) the outcome is
// either the same for every u, or "matched" for the u below pos = #{u: maximum > prob[u]} (prob ascends) and "none"
// from pos on.  So a workgroup keeps, per t, four fixed counters and three histograms over pos = 0..U (by what the flip
// moves between: actual < 0, the model's row == actual, != actual) in LDS, turns the histograms into suffix sums at the
// end and adds one value per (cell, counter) to HBM with an integer atomic: the result does not depend on the order.
//
// One wave per query: the model stage is a wave-wide reduction over the k candidates; for the close stage every lane
// owns one t and walks the candidates, which the wave loads 64 at a time and hands round lane by lane (no cross-lane
// reduction, no LDS traffic per candidate).  gridDim.y tiles t so that a tile's counters fit kSweepLdsBytes of LDS
// (64 thresholds at U <= 46, 15 at U = 256: three workgroups per CU at the most); gridDim.x strides over the queries.
#include <algorithm>
#include <atomic>
#include <cmath>

#include "ds_common.h"

namespace ds {

constexpr int kSweepThreads = 256;
constexpr int kSweepWaves = kSweepThreads / 64;     // queries per workgroup and pass
constexpr int kSweepMaxBlocks = 256;                // workgroups along the queries: each adds a whole tile to HBM once
constexpr int kSweepQueriesPerGroup = 64;           // queries per workgroup below that cap ("queries_per_group")
constexpr int kSweepMaxT = 101, kSweepMaxU = 256;
constexpr int kSweepLdsBytes = 48 * 1024;
constexpr int64_t kSweepMaxQueries = int64_t(1) << 40;   // uint32 counters in LDS: a workgroup sees < 2^32 queries

static std::atomic<int64_t> g_sweep_queries_per_group{kSweepQueriesPerGroup};

struct SweepArgs {
    const int32_t *rows;          // [n_queries][k]
    const uint8_t *d, *r, *s;     // [n_queries][k]
    const float *predictions;     // [n_queries][k]
    const int32_t *exact;         // [n_queries]
    const int32_t *actual;        // [n_queries]
    const int32_t *lev;           // [T] ascending
    const float *prob;            // [U] ascending
    unsigned long long *counts;   // [T][U][4]
    int64_t n_queries;
    int32_t k, T, U, tile_t;
};

struct SweepBest {               // the model stage of one query
    float value;
    int32_t where, count;        // count == 0: no candidate yet
};

__device__ __forceinline__ SweepBest sweep_merge(SweepBest a, SweepBest b)
{
    if (b.count == 0) return a;
    if (a.count == 0) return b;
    if (b.value > a.value) return b;
    if (b.value == a.value) return {a.value, min(a.where, b.where), a.count + b.count};
    return a;
}

__global__ __launch_bounds__(kSweepThreads) void ds_threshold_sweep_kernel(SweepArgs a)
{
    extern __shared__ uint32_t sweep_lds[];   // [tile][4 fixed + 3 x (U + 1) histogram]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t_first = blockIdx.y * a.tile_t;
    const int n_t = min(a.tile_t, a.T - t_first);
    const int bins = a.U + 1, per_t = 4 + 3 * bins;
    for (int i = threadIdx.x; i < n_t * per_t; i += kSweepThreads) sweep_lds[i] = 0;
    __syncthreads();
    const bool owner = lane < n_t;
    const int t = owner ? a.lev[t_first + lane] : 0;
    uint32_t *mine = sweep_lds + (owner ? lane : 0) * per_t;

    for (int64_t q = static_cast<int64_t>(blockIdx.x) * kSweepWaves + wave; q < a.n_queries;
         q += static_cast<int64_t>(gridDim.x) * kSweepWaves) {
        const int64_t in = q * a.k;
        const int32_t exact = a.exact[q], actual = a.actual[q];

        // model: (maximum, first holder, holders) over the candidates that are not NaN
        SweepBest best = {0.f, 0, 0};
        for (int32_t j = lane; j < a.k; j += 64) {
            const float p = a.predictions[in + j];
            if (p == p) best = sweep_merge(best, {p, j, 1});
        }
        for (int step = 32; step >= 1; step >>= 1) {
            SweepBest other;
            other.value = __shfl_xor(best.value, step, 64);
            other.where = __shfl_xor(best.where, step, 64);
            other.count = __shfl_xor(best.count, step, 64);
            best = sweep_merge(best, other);
        }
        const float front = a.predictions[in];
        const int32_t model_row = best.count == 1 && front == front ? a.rows[in + best.where] : -1;
        int pos = 0;                      // thresholds below the maximum
        if (model_row >= 0)
            for (int u0 = 0; u0 < a.U; u0 += 64) {
                const int u = u0 + lane;
                pos += __popcll(__ballot(u < a.U && best.value > a.prob[u < a.U ? u : 0]));
            }

        // close: lane = threshold; the wave's 64 candidates go round one at a time
        int top = t, holders = 0;
        int32_t close_row = -1;
        for (int32_t j0 = 0; j0 < a.k; j0 += 64) {
            const int32_t j = j0 + lane;
            const bool inside = j < a.k;
            const int packed = inside ? a.d[in + j] | (a.r[in + j] << 8) | (a.s[in + j] << 16) : 0;
            const int32_t row = inside ? a.rows[in + j] : -1;
            const int filled = min(64, a.k - j0);
            for (int i = 0; i < filled; ++i) {
                const int parts = __builtin_amdgcn_readlane(packed, i);
                const int32_t parts_row = __builtin_amdgcn_readlane(row, i);
                const int d = parts & 255, r = (parts >> 8) & 255, s = (parts >> 16) & 255;
                const int value = t > d ? 0 : (r > t ? r : s);
                if (value > top) { top = value; holders = 1; close_row = parts_row; }
                else if (value == top && holders > 0) ++holders;
            }
        }

        if (owner) {
            int32_t prediction = -1;
            bool flips = false;
            if (exact >= 0) prediction = exact;
            else if (holders == 1 && close_row >= 0) prediction = close_row;
            else flips = model_row >= 0 && pos > 0;
            if (flips) {
                const int kind = actual < 0 ? 0 : (model_row == actual ? 1 : 2);
                atomicAdd(mine + 4 + kind * bins + pos, 1u);
            } else {
                const int counter = prediction >= 0 ? (prediction == actual ? 0 : 1) : (actual < 0 ? 2 : 3);
                atomicAdd(mine + counter, 1u);
            }
        }
    }
    __syncthreads();

    // histogram -> suffix sums: entry p = the queries with pos >= p (one thread per (t, kind) row)
    for (int row = threadIdx.x; row < n_t * 3; row += kSweepThreads) {
        uint32_t *h = sweep_lds + (row / 3) * per_t + 4 + (row % 3) * bins;
        uint32_t running = 0;
        for (int p = a.U; p >= 0; --p) {
            running += h[p];
            h[p] = running;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_t * a.U * 4; i += kSweepThreads) {
        const int counter = i & 3, u = (i >> 2) % a.U, local = (i >> 2) / a.U;
        const uint32_t *base = sweep_lds + local * per_t;
        const uint32_t *none = base + 4, *right = none + bins, *wrong = right + bins;   // actual < 0, row == actual, != actual
        uint32_t value = base[counter];
        if (counter == 0) value += right[u + 1];
        else if (counter == 1) value += none[u + 1] + wrong[u + 1];
        else if (counter == 2) value += none[0] - none[u + 1];
        else value += (right[0] - right[u + 1]) + (wrong[0] - wrong[u + 1]);
        if (value) atomicAdd(a.counts + (static_cast<int64_t>(t_first + local) * a.U + u) * 4 + counter, value);
    }
}

}  // namespace ds

extern "C" {

int ds_sweep_option(const char *name, int64_t value)
{
    DS_REQUIRE(name != nullptr, "ds_sweep_option: null name");
    if (std::strcmp(name, "queries_per_group") == 0) {
        DS_REQUIRE(value >= 0 && value <= (int64_t(1) << 30),
                   "ds_sweep_option: queries_per_group = %lld out of range [0, 2^30]", (long long)value);
        ds::g_sweep_queries_per_group = value == 0 ? ds::kSweepQueriesPerGroup : value;
        return DS_OK;
    }
    ds::set_error("ds_sweep_option: unknown option '%s'", name);
    return DS_E_ARG;
}

int ds_threshold_sweep_device(const int32_t *d_rows, const uint8_t *d_d, const uint8_t *d_r, const uint8_t *d_s,
                              const float *d_predictions, const int32_t *d_exact, const int32_t *d_actual_row,
                              int64_t n_queries, int32_t k, const int32_t *d_lev, int32_t T, const float *d_prob,
                              int32_t U, int64_t *d_counts, void *stream)
{
    DS_REQUIRE(n_queries >= 0 && n_queries <= ds::kSweepMaxQueries, "ds_threshold_sweep_device: n_queries = %lld out of range",
               (long long)n_queries);
    DS_REQUIRE(k >= 1, "ds_threshold_sweep_device: k = %d, must be positive", k);
    DS_REQUIRE(T >= 1 && T <= ds::kSweepMaxT, "ds_threshold_sweep_device: T = %d out of range [1, %d]", T, ds::kSweepMaxT);
    DS_REQUIRE(U >= 1 && U <= ds::kSweepMaxU, "ds_threshold_sweep_device: U = %d out of range [1, %d]", U, ds::kSweepMaxU);
    DS_REQUIRE(d_lev && d_prob && d_counts, "ds_threshold_sweep_device: null pointer");
    DS_REQUIRE(n_queries <= INT64_MAX / k, "ds_threshold_sweep_device: too many pairs");
    // the grid's values are read back and checked here: T + U small values behind one synchronisation of `stream`
    int32_t lev[ds::kSweepMaxT];
    float prob[ds::kSweepMaxU];
    hipStream_t queue = static_cast<hipStream_t>(stream);
    DS_HIP(hipMemcpyAsync(lev, d_lev, sizeof(int32_t) * T, hipMemcpyDeviceToHost, queue));
    DS_HIP(hipMemcpyAsync(prob, d_prob, sizeof(float) * U, hipMemcpyDeviceToHost, queue));
    DS_HIP(hipStreamSynchronize(queue));
    for (int32_t i = 0; i < T; ++i) {
        DS_REQUIRE(lev[i] >= 0 && lev[i] <= 100, "ds_threshold_sweep_device: Levenshtein threshold %d out of range [0, 100]",
                   lev[i]);
        DS_REQUIRE(i == 0 || lev[i] > lev[i - 1], "ds_threshold_sweep_device: Levenshtein thresholds must ascend strictly");
    }
    for (int32_t i = 0; i < U; ++i) {
        DS_REQUIRE(std::isfinite(prob[i]), "ds_threshold_sweep_device: probability threshold %d is not finite", i);
        DS_REQUIRE(i == 0 || prob[i] > prob[i - 1], "ds_threshold_sweep_device: probability thresholds must ascend strictly");
    }
    if (n_queries == 0) return DS_OK;
    DS_REQUIRE(d_rows && d_d && d_r && d_s && d_predictions && d_exact && d_actual_row,
               "ds_threshold_sweep_device: null pointer");
    ds::SweepArgs args{};
    args.rows = d_rows; args.d = d_d; args.r = d_r; args.s = d_s; args.predictions = d_predictions;
    args.exact = d_exact; args.actual = d_actual_row; args.lev = d_lev; args.prob = d_prob;
    args.counts = reinterpret_cast<unsigned long long *>(d_counts);
    args.n_queries = n_queries; args.k = k; args.T = T; args.U = U;
    const int per_t_bytes = (4 + 3 * (U + 1)) * static_cast<int>(sizeof(uint32_t));
    args.tile_t = std::max(1, std::min({static_cast<int>(T), 64, ds::kSweepLdsBytes / per_t_bytes}));
    const int64_t per_group = std::max<int64_t>(ds::g_sweep_queries_per_group, ds::kSweepWaves);
    const int64_t groups = std::min<int64_t>((n_queries + per_group - 1) / per_group, ds::kSweepMaxBlocks);
    const dim3 grid(static_cast<unsigned>(groups), static_cast<unsigned>((T + args.tile_t - 1) / args.tile_t));
    hipLaunchKernelGGL(ds::ds_threshold_sweep_kernel, grid, dim3(ds::kSweepThreads),
                       static_cast<size_t>(args.tile_t) * per_t_bytes, queue, args);
    DS_HIP(hipGetLastError());
    return DS_OK;
}

}  // extern "C"
