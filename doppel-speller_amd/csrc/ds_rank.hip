// Ranked matches ("Ranked matches"): per query the best n of its k candidates, in order, with their
// probabilities, Levenshtein ratios and stages, written in HBM so that only n entries per query travel back.
//
// The rule (this project's own; the reference stops at one answer per title, predict.py:239-242):
//   head   exact[q] when >= 0 (stage 1), else best[q] when >= 0 (stage 2), else none.  It takes slot 0 with probability
//          1.0 (predict.py:108,179) and the ratio of the first candidate that equals it; absent from the candidates, an
//          exact head has ratio 100 (identical titles) and a close head ratio 0;
//   rest   every candidate j with 0 <= rows[q, j] < n_truth and rows[q, j] != head, stage 3, ordered by the float32 BITS of
//          its probability descending, then j ascending: by the 64-bit key (bits << 32) | ~j descending.  The keys of a
//          query are distinct and never 0, so key 0 stands for "not a candidate";
//   slots  cut to n; an unfilled slot holds row -1, probability quiet NaN, ratio 0, stage 0.
//
// One wave per query, four queries per workgroup, a capped grid that strides over the queries.  Two kernels:
//   ds_rank_lds_kernel     k <= the "lds_keys" option (default and at most kRankLdsKeys): the keys go to LDS once, every lane
//                          counts the keys above each key it owns (every lane reads the same LDS address: a broadcast),
//                          and a key's count is its slot.  ceil(k / 64) * k LDS reads per lane whatever n is;
//   ds_rank_select_kernel  any k, no LDS: n rounds, each the wave-wide maximum of the keys below the previous round's (the
//                          keys are distinct, so "below the last one" needs no mark on what was taken), read from HBM
//                          again every round.  n * ceil(k / 64) loads per lane: cheap for the few best of a long list.
// Both write every one of the n slots of every query exactly once, from the same keys: the result is the same.
#include <algorithm>

#include "ds_launch.h"
#include "ds_options.h"
#include "ds_wave.h"

namespace ds {

constexpr int kRankThreads = 256;
constexpr int kRankWaves = kRankThreads / 64;   // queries per workgroup and pass
constexpr int kRankLdsKeys = 512;               // keys of one query in LDS: 4 KiB per wave, 16 KiB per workgroup
constexpr int kRankMaxBlocks = 4096;            // 16 waves per CU in flight on 256 CUs; more queries: the grid strides

static Option g_rank_lds_keys{"lds_keys", 0, kRankLdsKeys, kRankLdsKeys};   // 0: every query takes the select kernel
static Option *const g_rank_options[] = {&g_rank_lds_keys};

struct RankHead {
    int32_t row;     // -1: the query has no head
    int32_t stage;
};

__device__ __forceinline__ RankHead rank_head(const int32_t *exact_row, const int32_t *best_row, int64_t q)
{
    const int32_t e = exact_row ? exact_row[q] : -1;
    const int32_t b = best_row ? best_row[q] : -1;
    if (e >= 0) return {e, 1};
    if (b >= 0) return {b, 2};
    return {-1, 0};
}

// the key of candidate j (0: not part of the rest)
__device__ __forceinline__ uint64_t rank_key(int32_t row, float probability, int32_t j, int32_t head, int64_t n_truth)
{
    const bool valid = row >= 0 && row < n_truth && row != head;
    return valid ? position_key(__float_as_uint(probability), j) : 0ull;
}

// slot 0 of a query with a head (one lane); first_j: the first candidate that equals the head, k when none does
__device__ __forceinline__ void rank_write_head(RankHead head, int32_t first_j, int32_t k, const uint8_t *ratios,
                                                int32_t *out_row, float *out_probability, uint8_t *out_ratio,
                                                int8_t *out_stage)
{
    out_row[0] = head.row;
    out_probability[0] = 1.0f;
    out_ratio[0] = first_j < k ? ratios[first_j] : (head.stage == 1 ? 100 : 0);
    out_stage[0] = static_cast<int8_t>(head.stage);
}

// slots [filled, n) of a query (the whole wave)
__device__ __forceinline__ void rank_write_empty(int32_t filled, int32_t n, int lane, int32_t *out_row,
                                                 float *out_probability, uint8_t *out_ratio, int8_t *out_stage)
{
    for (int32_t slot = filled + lane; slot < n; slot += 64) {
        out_row[slot] = -1;
        out_probability[slot] = __uint_as_float(0x7fc00000u);
        out_ratio[slot] = 0;
        out_stage[slot] = 0;
    }
}

__global__ __launch_bounds__(kRankThreads) void ds_rank_lds_kernel(
    const int32_t *__restrict__ rows, const float *__restrict__ predictions, const uint8_t *__restrict__ ratios,
    const int32_t *__restrict__ exact_row, const int32_t *__restrict__ best_row, int64_t n_queries, int32_t k, int32_t n,
    int64_t n_truth, int32_t *__restrict__ out_row, float *__restrict__ out_probability, uint8_t *__restrict__ out_ratio,
    int8_t *__restrict__ out_stage)
{
    __shared__ uint64_t keys[kRankWaves][kRankLdsKeys];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t *mine = keys[wave];
    // every wave of a workgroup makes the same number of passes (the barriers below), a pass past the end does nothing
    for (int64_t base = static_cast<int64_t>(blockIdx.x) * kRankWaves; base < n_queries;
         base += static_cast<int64_t>(gridDim.x) * kRankWaves) {
        const int64_t q = base + wave;
        const bool live = q < n_queries;
        const int64_t in = live ? q * k : 0, out = live ? q * n : 0;
        RankHead head = {-1, 0};
        int32_t first_j = k, n_rest = 0;
        if (live) {
            head = rank_head(exact_row, best_row, q);
            for (int32_t j0 = 0; j0 < k; j0 += 64) {
                const int32_t j = j0 + lane;
                const int32_t row = j < k ? rows[in + j] : -1;
                const uint64_t key = j < k ? rank_key(row, predictions[in + j], j, head.row, n_truth) : 0ull;
                if (j < k) mine[j] = key;
                const unsigned long long heads = __ballot(j < k && head.row >= 0 && row == head.row);
                if (heads && first_j == k) first_j = j0 + __ffsll(heads) - 1;
                n_rest += __popcll(__ballot(key != 0));
            }
        }
        __syncthreads();
        if (live) {
            const int32_t lead = head.row >= 0 ? 1 : 0;
            if (lead && lane == 0)
                rank_write_head(head, first_j, k, ratios + in, out_row + out, out_probability + out, out_ratio + out,
                                out_stage + out);
            for (int32_t j = lane; j < k; j += 64) {
                const uint64_t key = mine[j];
                if (key == 0) continue;
                int32_t above = 0;
#pragma unroll 4
                for (int32_t i = 0; i < k; ++i) above += mine[i] > key ? 1 : 0;
                const int32_t slot = lead + above;
                if (slot < n) {
                    out_row[out + slot] = rows[in + j];
                    out_probability[out + slot] = __uint_as_float(static_cast<uint32_t>(key >> 32));
                    out_ratio[out + slot] = ratios[in + j];
                    out_stage[out + slot] = 3;
                }
            }
            rank_write_empty(lead + n_rest, n, lane, out_row + out, out_probability + out, out_ratio + out,
                             out_stage + out);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kRankThreads) void ds_rank_select_kernel(
    const int32_t *__restrict__ rows, const float *__restrict__ predictions, const uint8_t *__restrict__ ratios,
    const int32_t *__restrict__ exact_row, const int32_t *__restrict__ best_row, int64_t n_queries, int32_t k, int32_t n,
    int64_t n_truth, int32_t *__restrict__ out_row, float *__restrict__ out_probability, uint8_t *__restrict__ out_ratio,
    int8_t *__restrict__ out_stage)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t q = static_cast<int64_t>(blockIdx.x) * kRankWaves + wave; q < n_queries;
         q += static_cast<int64_t>(gridDim.x) * kRankWaves) {
        const int64_t in = q * k, out = q * n;
        const RankHead head = rank_head(exact_row, best_row, q);
        int32_t filled = 0;
        if (head.row >= 0) {
            int32_t first_j = k;
            for (int32_t j0 = 0; j0 < k && first_j == k; j0 += 64) {
                const int32_t j = j0 + lane;
                const unsigned long long heads = __ballot(j < k && rows[in + (j < k ? j : 0)] == head.row);
                if (heads) first_j = j0 + __ffsll(heads) - 1;
            }
            if (lane == 0)
                rank_write_head(head, first_j, k, ratios + in, out_row + out, out_probability + out, out_ratio + out,
                                out_stage + out);
            filled = 1;
        }
        uint64_t below = 0;      // the key of the previous round; the first round takes any key
        bool first = true;
        while (filled < n) {
            uint64_t best = 0;
            for (int32_t j = lane; j < k; j += 64) {
                const uint64_t key = rank_key(rows[in + j], predictions[in + j], j, head.row, n_truth);
                if ((first || key < below) && key > best) best = key;
            }
            best = wave_max(best);
            if (best == 0) break;          // the same in every lane: the rest is exhausted
            if (lane == 0) {
                const int32_t j = key_position(best);
                out_row[out + filled] = rows[in + j];
                out_probability[out + filled] = __uint_as_float(static_cast<uint32_t>(best >> 32));
                out_ratio[out + filled] = ratios[in + j];
                out_stage[out + filled] = 3;
            }
            below = best;
            first = false;
            ++filled;
        }
        rank_write_empty(filled, n, lane, out_row + out, out_probability + out, out_ratio + out, out_stage + out);
    }
}

}  // namespace ds

extern "C" {

int ds_rank_option(const char *name, int64_t value)
{
    return ds::set_option("ds_rank_option", ds::g_rank_options, name, value);
}

int ds_rank_matches_device(const int32_t *d_rows, const float *d_predictions, const uint8_t *d_ratios,
                           const int32_t *d_exact_row, const int32_t *d_best_row, int64_t n_queries, int32_t k,
                           int32_t n, int64_t n_truth, int32_t *d_out_row, float *d_out_probability,
                           uint8_t *d_out_ratio, int8_t *d_out_stage, void *stream)
{
    DS_REQUIRE(n_queries >= 0 && n_truth >= 0, "ds_rank_matches_device: negative count");
    DS_REQUIRE(k >= 1, "ds_rank_matches_device: k = %d, must be positive", k);
    DS_REQUIRE(n >= 1 && n <= k, "ds_rank_matches_device: n = %d out of range [1, k = %d]", n, k);
    DS_REQUIRE(d_rows && d_predictions && d_ratios && d_out_row && d_out_probability && d_out_ratio && d_out_stage,
               "ds_rank_matches_device: null pointer");
    DS_REQUIRE(n_queries <= INT64_MAX / k, "ds_rank_matches_device: too many pairs");
    if (n_queries == 0) return DS_OK;
    const int64_t passes = (n_queries + ds::kRankWaves - 1) / ds::kRankWaves;
    const dim3 grid(ds::grid_cap(passes, ds::kRankMaxBlocks));
    if (k <= ds::g_rank_lds_keys.get())
        DS_LAUNCH(ds::ds_rank_lds_kernel, grid, dim3(ds::kRankThreads), 0, static_cast<hipStream_t>(stream), d_rows,
                  d_predictions, d_ratios, d_exact_row, d_best_row, n_queries, k, n, n_truth, d_out_row,
                  d_out_probability, d_out_ratio, d_out_stage);
    else
        DS_LAUNCH(ds::ds_rank_select_kernel, grid, dim3(ds::kRankThreads), 0, static_cast<hipStream_t>(stream),
                  d_rows, d_predictions, d_ratios, d_exact_row, d_best_row, n_queries, k, n, n_truth, d_out_row,
                  d_out_probability, d_out_ratio, d_out_stage);
    return DS_OK;
}

}  // extern "C"
