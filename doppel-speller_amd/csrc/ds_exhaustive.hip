// Exhaustive matches ("Exhaustive matches"): per query the best n rows of the WHOLE truth table by the
// model's probability, with no candidate stage in front and no exact or close override -- the model alone.
//
// The rule (this project's own; the reference's README promises such a search, its code scores the Jaccard top_n only):
//   key    of truth row t with probability p: (float32 bits of p << 32) | (0xffffffff - t).  Probabilities are finite and
//          non-negative, so bit order is value order; rows are below 2^31, so a key is never 0 and 0 stands for "empty";
//   best   the n largest keys of a query, descending: by probability bits descending, then by row ascending;
//   slots  an unfilled slot (fewer than n truth rows) holds row -1 and the quiet NaN 0x7fc00000.
// The keys of a query are distinct, so its n largest are a set that no tiling, geometry or schedule can change.
//
// The pairs never exist all at once.  Per tile -- a rectangle of consecutive queries x consecutive truth rows of at most
// "tile_pairs" pairs -- ds_exhaustive_pairs_kernel writes the pair list (8 B per pair), the existing features and forest
// entry points turn it into probabilities, and the fold merges those into each query's running n keys in HBM:
//   ds_exhaustive_select_kernel   one workgroup per SLICE of kSliceKeys keys of one query, 16 keys per thread in registers.
//                                 n rounds: every thread's largest key below the previous round's, the wave-wide maximum
//                                 by shuffles, the workgroup's by four LDS words; the winner is the slice's next key.
//   level 0    keys made from the tile's probabilities, followed by the query's running list: ceil((rows + n) / 4096) slices;
//   level >= 1 the lists of the level before (n keys per slice) as one array per query, until one slice is left: that one
//              writes the running list.  Every level shrinks a query's keys by 4096 / n >= 64.
// One query whose tile holds millions of rows is spread over thousands of workgroups; no atomics, no arrival order.
#include <algorithm>

#include "ds_launch.h"
#include "ds_options.h"
#include "ds_wave.h"

namespace ds {

constexpr int kFoldThreads = 256;
constexpr int kFoldWaves = kFoldThreads / 64;
constexpr int kFoldKeysPerThread = 16;                          // 32 VGPRs of keys
constexpr int kSliceKeys = kFoldThreads * kFoldKeysPerThread;    // 4096 keys per workgroup
constexpr int kExhaustiveMaxN = 64;
// pairs of a tile at most: 2^24 pairs x 66 floats = 1.1e9 features, half of what a 32-bit count holds; the workspace of such
// a tile is 4.7 GB
constexpr int64_t kTilePairsMax = int64_t(1) << 24;
constexpr int64_t kBytesPerPair = DS_FEATURES_COUNT * 4 + 4 + 8;   // features, probability, pair (q, t)

static Option g_tile_pairs{"tile_pairs", 0, kTilePairsMax, 0};   // 0: the default (default_tile_pairs)
static Option *const g_exhaustive_options[] = {&g_tile_pairs};

__device__ __forceinline__ uint64_t exhaustive_key(float probability, int64_t row)
{
    return (static_cast<uint64_t>(__float_as_uint(probability)) << 32) | (0xffffffffu - static_cast<uint32_t>(row));
}

// pair i of the tile: query q_first + i / rows, truth row row_first + i % rows  (n_pairs = queries of the tile x rows < 2^31)
__global__ __launch_bounds__(256) void ds_exhaustive_pairs_kernel(int32_t q_first, int32_t row_first, uint32_t rows,
                                                                  uint32_t n_pairs, int32_t *__restrict__ pair_q,
                                                                  int32_t *__restrict__ pair_t)
{
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_pairs; i += gridDim.x * 256u) {
        const uint32_t q = i / rows;
        pair_q[i] = q_first + static_cast<int32_t>(q);
        pair_t[i] = row_first + static_cast<int32_t>(i - q * rows);
    }
}

struct FoldArgs {
    const float *probabilities;   // level 0: [n_queries][count] of rows row_first + j; null at the levels above
    const uint64_t *keys;         // level >= 1: [n_queries][count]
    const uint64_t *running;      // level 0: [n_queries][n], a query's keys behind its `count` probabilities; else null
    uint64_t *out;                // [n_queries][slices][n]; the last level (slices == 1): the running list
    int64_t count;                // keys of a query at this level, without the running list
    int64_t row_first;
    int64_t n_blocks;             // n_queries * slices
    int32_t slices;               // ceil((count + (running ? n : 0)) / kSliceKeys)
    int32_t n;
};

__global__ __launch_bounds__(kFoldThreads) void ds_exhaustive_select_kernel(FoldArgs a)
{
    __shared__ uint64_t wave_best[2][kFoldWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t total = a.count + (a.running ? a.n : 0);
    for (int64_t block = blockIdx.x; block < a.n_blocks; block += gridDim.x) {
        const int64_t q = block / a.slices;
        const int64_t first = (block - q * a.slices) * kSliceKeys;
        uint64_t keys[kFoldKeysPerThread];
#pragma unroll
        for (int r = 0; r < kFoldKeysPerThread; ++r) {   // consecutive threads read consecutive keys
            const int64_t i = first + r * kFoldThreads + threadIdx.x;
            uint64_t key = 0;
            if (i < a.count)
                key = a.probabilities ? exhaustive_key(a.probabilities[q * a.count + i], a.row_first + i)
                                      : a.keys[q * a.count + i];
            else if (i < total)
                key = a.running[q * a.n + (i - a.count)];
            keys[r] = key;
        }
        // the last level writes the list its first level read: every read of the workgroup is complete before a write
        __syncthreads();
        uint64_t *out = a.out + block * a.n;
        uint64_t below = ~0ull;                  // the key of the previous round (keys hold a row below 2^31: never ~0)
        int32_t filled = 0;
        for (; filled < a.n; ++filled) {
            uint64_t best = 0;
#pragma unroll
            for (int r = 0; r < kFoldKeysPerThread; ++r) {
                const uint64_t key = keys[r];
                best = (key < below && key > best) ? key : best;
            }
            best = wave_max(best);
            // one barrier per round: a wave that reads round r's words has passed round r's barrier, and nobody writes them
            // again before round r + 2, behind round r + 1's barrier
            if (lane == 0) wave_best[filled & 1][wave] = best;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < kFoldWaves; ++w) {
                const uint64_t other = wave_best[filled & 1][w];
                best = other > best ? other : best;
            }
            if (best == 0) break;                // the same in every thread: the slice is exhausted
            if (threadIdx.x == 0) out[filled] = best;
            below = best;
        }
        for (int32_t slot = filled + threadIdx.x; slot < a.n; slot += kFoldThreads) out[slot] = 0;
        __syncthreads();                         // wave_best is free for the next block of this workgroup
    }
}

__global__ __launch_bounds__(256) void ds_exhaustive_finish_kernel(const uint64_t *__restrict__ running, int64_t n_slots,
                                                                   int32_t *__restrict__ out_row,
                                                                   float *__restrict__ out_probability)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n_slots;
         i += static_cast<int64_t>(gridDim.x) * 256) {
        const uint64_t key = running[i];
        out_row[i] = key ? static_cast<int32_t>(0xffffffffu - static_cast<uint32_t>(key)) : -1;
        out_probability[i] = __uint_as_float(key ? static_cast<uint32_t>(key >> 32) : 0x7fc00000u);
    }
}

static int64_t slices_of(int64_t keys) { return (keys + kSliceKeys - 1) / kSliceKeys; }

// uint64 words of the two partial buffers a fold of n_queries x tile_rows needs: level 0's lists, then level 1's
static void partial_words(int64_t n_queries, int64_t tile_rows, int32_t n, int64_t *first, int64_t *second)
{
    const int64_t slices0 = slices_of(tile_rows + n);
    *first = slices0 > 1 ? n_queries * slices0 * n : 0;
    const int64_t slices1 = slices_of(slices0 * n);
    *second = slices0 > 1 && slices1 > 1 ? n_queries * slices1 * n : 0;
}

// the fold of one tile on buffers of the caller's (partial_words)
static int fold(const float *d_probabilities, int64_t n_queries, int64_t tile_rows, int64_t row_first, int32_t n,
                uint64_t *d_running, uint64_t *d_first, uint64_t *d_second, hipStream_t stream)
{
    FoldArgs args{};
    args.probabilities = d_probabilities;
    args.running = d_running;
    args.count = tile_rows;
    args.row_first = row_first;
    args.n = n;
    uint64_t *buffers[2] = {d_first, d_second};
    for (int level = 0;; ++level) {
        const int64_t slices = slices_of(args.count + (args.running ? n : 0));
        args.slices = static_cast<int32_t>(slices);
        args.n_blocks = n_queries * slices;
        args.out = slices == 1 ? d_running : buffers[level & 1];
        const unsigned grid = static_cast<unsigned>(std::min<int64_t>(args.n_blocks, 256 * 64));
        DS_LAUNCH(ds_exhaustive_select_kernel, dim3(grid), dim3(kFoldThreads), 0, stream, args);
        if (slices == 1) return DS_OK;
        args.probabilities = nullptr;
        args.running = nullptr;
        args.keys = args.out;
        args.count = slices * n;
    }
}

static int64_t default_tile_pairs()
{
    size_t free_bytes = 0, total_bytes = 0;
    if (hipMemGetInfo(&free_bytes, &total_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return kTilePairsMax;
    }
    // a quarter of the free HBM holds the whole workspace; the partial lists add 8 n / 4096 <= 1/8 byte per pair
    const int64_t fit = static_cast<int64_t>(free_bytes / 4) / (kBytesPerPair + 1);
    return std::max<int64_t>(1, std::min(fit, kTilePairsMax));
}

}  // namespace ds

extern "C" {

int ds_exhaustive_option(const char *name, int64_t value)
{
    return ds::set_option("ds_exhaustive_option", ds::g_exhaustive_options, name, value);
}

int ds_exhaustive_fold_device(const float *d_probabilities, int64_t n_queries, int64_t tile_rows, int64_t row_first,
                              int32_t n, uint64_t *d_running, void *stream)
{
    DS_REQUIRE(n_queries >= 0 && tile_rows >= 0 && row_first >= 0, "ds_exhaustive_fold_device: negative count");
    DS_REQUIRE(n >= 1 && n <= ds::kExhaustiveMaxN, "ds_exhaustive_fold_device: n = %d out of range [1, %d]", n,
               ds::kExhaustiveMaxN);
    DS_REQUIRE(d_probabilities && d_running, "ds_exhaustive_fold_device: null pointer");
    DS_REQUIRE(row_first + tile_rows <= (int64_t(1) << 31), "ds_exhaustive_fold_device: rows past 2^31");
    DS_REQUIRE(tile_rows == 0 || n_queries <= (int64_t(1) << 40) / tile_rows, "ds_exhaustive_fold_device: too many pairs");
    if (n_queries == 0 || tile_rows == 0) return DS_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int64_t first = 0, second = 0;
    ds::partial_words(n_queries, tile_rows, n, &first, &second);
    ds::DeviceBuffer<uint64_t> partials;    // freed on return, behind the synchronisation below
    if (first + second) {
        DS_TRY(partials.allocate(static_cast<size_t>(first + second)));
    }
    const int status = ds::fold(d_probabilities, n_queries, tile_rows, row_first, n, d_running, partials.ptr,
                                partials.ptr ? partials.ptr + first : nullptr, s);
    if (partials.ptr) DS_HIP(hipStreamSynchronize(s));
    return status;
}

int ds_exhaustive_finish_device(const uint64_t *d_running, int64_t n_queries, int32_t n, int32_t *d_out_row,
                                float *d_out_probability, void *stream)
{
    DS_REQUIRE(n_queries >= 0, "ds_exhaustive_finish_device: negative count");
    DS_REQUIRE(n >= 1 && n <= ds::kExhaustiveMaxN, "ds_exhaustive_finish_device: n = %d out of range [1, %d]", n,
               ds::kExhaustiveMaxN);
    DS_REQUIRE(d_running && d_out_row && d_out_probability, "ds_exhaustive_finish_device: null pointer");
    DS_REQUIRE(n_queries <= INT64_MAX / n, "ds_exhaustive_finish_device: too many slots");
    if (n_queries == 0) return DS_OK;
    const int64_t n_slots = n_queries * n;
    const unsigned grid = static_cast<unsigned>(std::min<int64_t>((n_slots + 255) / 256, 256 * 16));
    DS_LAUNCH(ds::ds_exhaustive_finish_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), d_running,
              n_slots, d_out_row, d_out_probability);
    return DS_OK;
}

int ds_exhaustive_rank_device(ds_titles *queries, ds_titles *truth, ds_forest *forest, int64_t q_first,
                              int64_t n_queries, int32_t n, uint8_t space_code, uint32_t n_truth, int32_t *d_out_row,
                              float *d_out_probability, void *stream)
{
    DS_REQUIRE(queries && truth && forest, "ds_exhaustive_rank_device: null handle");
    DS_REQUIRE(q_first >= 0 && n_queries >= 0, "ds_exhaustive_rank_device: negative count");
    DS_REQUIRE(n >= 1 && n <= ds::kExhaustiveMaxN, "ds_exhaustive_rank_device: n = %d out of range [1, %d]", n,
               ds::kExhaustiveMaxN);
    DS_REQUIRE(d_out_row && d_out_probability, "ds_exhaustive_rank_device: null pointer");
    DS_REQUIRE(n_queries <= queries->n - q_first, "ds_exhaustive_rank_device: queries [%lld, %lld) outside the table's %lld",
               (long long)q_first, (long long)(q_first + n_queries), (long long)queries->n);
    DS_REQUIRE(queries->n < (int64_t(1) << 31) && truth->n < (int64_t(1) << 31),
               "ds_exhaustive_rank_device: a table of 2^31 rows or more");
    DS_REQUIRE(queries->device == truth->device, "ds_exhaustive_rank_device: tables on different devices");
    DS_REQUIRE(truth->n == 0 || truth->has_counts, "ds_exhaustive_rank_device: the truth table has no word counts");
    if (n_queries == 0) return DS_OK;
    DS_HIP(hipSetDevice(truth->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t N = truth->n;
    const int64_t chosen = ds::g_tile_pairs.get();
    const int64_t tile_pairs = chosen > 0 ? chosen : ds::default_tile_pairs();
    // a tile: one query x tile_pairs rows of a long table, or as many whole queries as fit x all rows of a short one
    const int64_t tile_rows = std::min(N, tile_pairs);
    const int64_t tile_queries = tile_rows ? std::min(n_queries, std::max<int64_t>(1, tile_pairs / tile_rows)) : 0;
    const int64_t pairs = tile_queries * tile_rows;

    // one allocation per call: running keys, partial lists, features, probabilities, pair lists; freed on return
    int64_t first = 0, second = 0;
    if (pairs) ds::partial_words(tile_queries, tile_rows, n, &first, &second);
    const int64_t running_words = n_queries * n;
    size_t bytes = 0;
    auto carve = [&bytes](int64_t size) {    // every part starts on a 256-byte boundary, as an allocation of its own would
        const size_t at = bytes;
        bytes += (static_cast<size_t>(size) + 255) / 256 * 256;
        return at;
    };
    const size_t at_running = carve(running_words * 8), at_first = carve(first * 8), at_second = carve(second * 8);
    const size_t at_features = carve(pairs * DS_FEATURES_COUNT * 4), at_probabilities = carve(pairs * 4);
    const size_t at_pair_q = carve(pairs * 4), at_pair_t = carve(pairs * 4);
    ds::DeviceBuffer<unsigned char> workspace;
    DS_TRY(workspace.allocate(bytes));
    uint64_t *d_running = reinterpret_cast<uint64_t *>(workspace.ptr + at_running);
    uint64_t *d_first = reinterpret_cast<uint64_t *>(workspace.ptr + at_first);
    uint64_t *d_second = reinterpret_cast<uint64_t *>(workspace.ptr + at_second);
    float *d_features = reinterpret_cast<float *>(workspace.ptr + at_features);
    float *d_probabilities = reinterpret_cast<float *>(workspace.ptr + at_probabilities);
    int32_t *d_pair_q = reinterpret_cast<int32_t *>(workspace.ptr + at_pair_q);
    int32_t *d_pair_t = reinterpret_cast<int32_t *>(workspace.ptr + at_pair_t);

    int status = DS_OK;
    auto run = [&]() -> int {
        DS_HIP(hipMemsetAsync(d_running, 0, static_cast<size_t>(running_words) * 8, s));
        for (int64_t q0 = 0; q0 < n_queries && pairs; q0 += tile_queries) {
            const int64_t nq = std::min(tile_queries, n_queries - q0);
            for (int64_t r0 = 0; r0 < N; r0 += tile_rows) {
                const int64_t rows = std::min(tile_rows, N - r0), here = nq * rows;
                const unsigned grid = static_cast<unsigned>(std::min<int64_t>((here + 255) / 256, 256 * 16));
                DS_LAUNCH(ds::ds_exhaustive_pairs_kernel, dim3(grid), dim3(256), 0, s,
                          static_cast<int32_t>(q_first + q0), static_cast<int32_t>(r0),
                          static_cast<uint32_t>(rows), static_cast<uint32_t>(here), d_pair_q, d_pair_t);
                int step = ds_construct_features_indexed_device(queries, truth, d_pair_q, d_pair_t, q_first + q0,
                                                                static_cast<int32_t>(rows), space_code, n_truth, here,
                                                                d_features, stream);
                if (step == DS_OK) step = ds_forest_predict_device(forest, d_features, here, nullptr, d_probabilities, stream);
                if (step == DS_OK)
                    step = ds::fold(d_probabilities, nq, rows, r0, n, d_running + q0 * n, d_first, d_second, s);
                if (step != DS_OK) return step;
            }
        }
        return ds_exhaustive_finish_device(d_running, n_queries, n, d_out_row, d_out_probability, stream);
    };
    status = run();
    // the workspace is freed on return: everything that reads it is complete first (also after an error)
    const hipError_t synced = hipStreamSynchronize(s);
    if (status == DS_OK && synced != hipSuccess) return ds::hip_failed(synced, "hipStreamSynchronize", __FILE__, __LINE__);
    return status;
}

}  // extern "C"
