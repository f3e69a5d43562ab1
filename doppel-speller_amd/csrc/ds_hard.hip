// Hard negatives ("Hard negatives"): per train title the wrong candidates the model likes best, mined
// in HBM so that only the mined pairs travel back.
//
// The rule (this project's own; the reference samples its negatives at random, feature_engineering_prepare.py:25-57).
// For title i of a chunk, over the candidates j = 0 .. k-1 with truth row c_j = rows[i, j] and margin m_j = margins[i, j]:
//   eligible  0 <= c_j < n_truth, c_j != own[i], c_j not in exclude[i, 0 .. n_exclude) and m_j > min_margin (strict, both
//             sides float32; -INFINITY: no threshold);
//   order     by the 64-bit key (ord(m_j) << 32) | (uint32)~j descending, ord the monotone map of the float32 bits (all
//             bits flipped when the sign is set, else the sign bit set): -0.0 sorts below +0.0, equal margins go to the
//             smaller j.  The keys of a title are distinct and never 0, so key 0 stands for "not eligible" (the
//             convention of ds_rank.hip);
//   yield     the first min(hard_n, eligible) candidates in that order, maybe none.
// The output is dense: titles in title order, within a title in key order; slot s holds pair_q = q_first + i, pair_t =
// c_j, position = j, margin = m_j.  Every mined pair is a negative: there is no target array.
//
// One wave per title, four titles per workgroup, a capped grid that strides over the titles.  A title's first slot needs
// the counts of all titles before it, so there are two phases around a scan:
//   ds_hard_count_kernel  min(hard_n, eligible) of every title -> offsets[i];
//   ds_hard_scan_kernel   one workgroup: the exclusive scan of those counts (block_exclusive of ds_wave.h) in place, started
//                         from the running total in *total, which it then moves on: the next chunk continues where this one
//                         ended, and the result does not depend on how the titles are cut into chunks;
//   ds_hard_emit_kernel   hard_n rounds, each the wave-wide maximum of the keys below the previous round's (the scheme of
//                         ds_rank_select_kernel: distinct keys need no mark on what was taken); lane 0 writes slot
//                         offsets[i] + r.  Lists of up to 64 * kHardRegisterKeys candidates keep their keys in registers,
//                         longer ones compute them again every round.
// The exclusion list of a title is read once, a lane per entry, and handed to every lane by shuffles: a candidate is
// compared against 16 registers, not against global memory.
//
// Capacity: no slot >= capacity is written.  A chunk that would pass the capacity leaves -(pairs needed so far) in *total,
// every later chunk keeps it negative and writes nothing, and ds_hard_total reports it as DS_E_ARG.
#include <algorithm>

#include "ds_launch.h"
#include "ds_options.h"
#include "ds_wave.h"

namespace ds {

constexpr int kHardThreads = 256;
constexpr int kHardWaves = kHardThreads / 64;   // titles per workgroup and pass
constexpr int kHardMaxN = 16;
constexpr int kHardMaxExclude = 16;
constexpr int kHardRegisterKeys = 4;            // keys of a title per lane in registers: lists of up to 256 candidates
constexpr int kHardMaxBlocks = 4096;            // 16 waves per CU in flight on 256 CUs; more titles: the grid strides
constexpr int kHardBlocksLimit = 1 << 16;
constexpr int kHardScanThreads = 1024;

static Option g_hard_max_blocks{"max_blocks", 0, kHardBlocksLimit, kHardMaxBlocks, true};
static Option *const g_hard_options[] = {&g_hard_max_blocks};

// ascending order of the result = ascending order of the (finite) values, -0.0 below +0.0; and back
__device__ __forceinline__ uint32_t margin_order(float margin)
{
    const uint32_t bits = __float_as_uint(margin);
    return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u;
}
__device__ __forceinline__ float order_margin(uint32_t order)
{
    return __uint_as_float((order & 0x80000000u) ? order ^ 0x80000000u : ~order);
}

// what is the same for every candidate of a title, in every lane
struct HardTitle {
    int32_t own;
    int32_t exclude[kHardMaxExclude];   // -1 past n_exclude: equals no row inside the truth table
};

__device__ __forceinline__ HardTitle hard_title(const int32_t *own_row, const int32_t *exclude, int32_t n_exclude,
                                                int64_t q, int lane)
{
    HardTitle title;
    title.own = own_row[q];
    const int32_t mine = lane < n_exclude ? exclude[q * n_exclude + lane] : -1;
#pragma unroll
    for (int e = 0; e < kHardMaxExclude; ++e) title.exclude[e] = __shfl(mine, e, 64);
    return title;
}

// the key of candidate j (0: not eligible)
__device__ __forceinline__ uint64_t hard_key(int32_t row, float margin, int32_t j, const HardTitle &title,
                                             int64_t n_truth, float min_margin)
{
    bool eligible = row >= 0 && row < n_truth && row != title.own && margin > min_margin;
#pragma unroll
    for (int e = 0; e < kHardMaxExclude; ++e) eligible = eligible && row != title.exclude[e];
    return eligible ? position_key(margin_order(margin), j) : 0ull;
}

struct HardArgs {
    const int32_t *rows;       // [n_queries][k]
    const float *margins;      // [n_queries][k]
    const int32_t *own_row;    // [n_queries]
    const int32_t *exclude;    // [n_queries][n_exclude], null when n_exclude == 0
    int64_t n_queries, n_truth, q_first, capacity;
    int32_t k, n_exclude, hard_n;
    float min_margin;
    int64_t *offsets;          // [n_queries]: the count of a title, then its first slot
    int32_t *pair_q, *pair_t, *position;
    float *margin;
};

__global__ __launch_bounds__(kHardThreads) void ds_hard_count_kernel(HardArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t q = static_cast<int64_t>(blockIdx.x) * kHardWaves + wave; q < a.n_queries;
         q += static_cast<int64_t>(gridDim.x) * kHardWaves) {
        const int64_t in = q * a.k;
        const HardTitle title = hard_title(a.own_row, a.exclude, a.n_exclude, q, lane);
        int32_t eligible = 0;
        for (int32_t j0 = 0; j0 < a.k; j0 += 64) {
            const int32_t j = j0 + lane;
            const uint64_t key =
                j < a.k ? hard_key(a.rows[in + j], a.margins[in + j], j, title, a.n_truth, a.min_margin) : 0ull;
            eligible += __popcll(__ballot(key != 0));
        }
        if (lane == 0) a.offsets[q] = eligible < a.hard_n ? eligible : a.hard_n;
    }
}

// offsets[i] = |*total| + the counts before i; *total moves on by the sum, negative once the capacity is passed
__global__ __launch_bounds__(kHardScanThreads) void ds_hard_scan_kernel(int64_t *offsets, int64_t n_queries,
                                                                        int64_t capacity, int64_t *total)
{
    __shared__ uint32_t s_waves[kHardScanThreads / 64];
    const int64_t entry = *total;       // every thread reads it before the first barrier, thread 0 writes it after the last
    const int64_t base = entry < 0 ? -entry : entry;
    int64_t running = 0;
    for (int64_t first = 0; first < n_queries; first += kHardScanThreads) {
        const int64_t i = first + threadIdx.x;
        const uint32_t value = i < n_queries ? static_cast<uint32_t>(offsets[i]) : 0u;
        uint32_t sum;
        const uint32_t before = block_exclusive<kHardScanThreads>(value, s_waves, sum);
        if (i < n_queries) offsets[i] = base + running + before;
        running += sum;
    }
    if (threadIdx.x == 0) {
        const int64_t needed = base + running;
        *total = (entry < 0 || needed > capacity) ? -needed : needed;
    }
}

template <bool kRegisters>
__global__ __launch_bounds__(kHardThreads) void ds_hard_emit_kernel(HardArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t q = static_cast<int64_t>(blockIdx.x) * kHardWaves + wave; q < a.n_queries;
         q += static_cast<int64_t>(gridDim.x) * kHardWaves) {
        const int64_t in = q * a.k;
        const HardTitle title = hard_title(a.own_row, a.exclude, a.n_exclude, q, lane);
        uint64_t keys[kHardRegisterKeys];
        if (kRegisters) {
#pragma unroll
            for (int s = 0; s < kHardRegisterKeys; ++s) {
                const int32_t j = s * 64 + lane;
                keys[s] = j < a.k ? hard_key(a.rows[in + j], a.margins[in + j], j, title, a.n_truth, a.min_margin) : 0ull;
            }
        }
        int64_t slot = a.offsets[q];
        uint64_t below = ~0ull;          // no key reaches it: its margin would be a NaN, which is never eligible
        for (int32_t r = 0; r < a.hard_n; ++r) {
            uint64_t best = 0;
            if (kRegisters) {
#pragma unroll
                for (int s = 0; s < kHardRegisterKeys; ++s)
                    if (keys[s] < below && keys[s] > best) best = keys[s];
            } else {
                for (int32_t j = lane; j < a.k; j += 64) {
                    const uint64_t key = hard_key(a.rows[in + j], a.margins[in + j], j, title, a.n_truth, a.min_margin);
                    if (key < below && key > best) best = key;
                }
            }
            best = wave_max(best);
            if (best == 0) break;          // the same in every lane: no eligible candidate is left
            if (lane == 0 && slot < a.capacity) {
                const int32_t j = key_position(best);
                a.pair_q[slot] = static_cast<int32_t>(a.q_first + q);
                a.pair_t[slot] = a.rows[in + j];
                a.position[slot] = j;
                a.margin[slot] = order_margin(static_cast<uint32_t>(best >> 32));
            }
            below = best;
            ++slot;
        }
    }
}

}  // namespace ds

extern "C" {

int ds_hard_option(const char *name, int64_t value)
{
    return ds::set_option("ds_hard_option", ds::g_hard_options, name, value);
}

int ds_hard_negatives_device(const int32_t *d_rows, const float *d_margins, int64_t n_queries, int32_t k,
                             int64_t n_truth, const int32_t *d_own_row, const int32_t *d_exclude, int32_t n_exclude,
                             int32_t hard_n, float min_margin, int64_t q_first, int64_t *d_offsets, int64_t *d_total,
                             int64_t capacity, int32_t *d_pair_q, int32_t *d_pair_t, int32_t *d_position,
                             float *d_margin, void *stream)
{
    DS_REQUIRE(n_queries >= 0 && n_truth >= 0 && q_first >= 0 && capacity >= 0, "ds_hard_negatives_device: negative count");
    DS_REQUIRE(k >= 1, "ds_hard_negatives_device: k = %d, must be positive", k);
    DS_REQUIRE(hard_n >= 1 && hard_n <= std::min<int32_t>(ds::kHardMaxN, k),
               "ds_hard_negatives_device: hard_n = %d out of range [1, min(%d, k = %d)]", hard_n, ds::kHardMaxN, k);
    DS_REQUIRE(n_exclude >= 0 && n_exclude <= ds::kHardMaxExclude,
               "ds_hard_negatives_device: n_exclude = %d out of range [0, %d]", n_exclude, ds::kHardMaxExclude);
    DS_REQUIRE(n_exclude == 0 || d_exclude != nullptr, "ds_hard_negatives_device: n_exclude = %d with a null d_exclude",
               n_exclude);
    DS_REQUIRE(d_rows && d_margins && d_own_row && d_offsets && d_total && d_pair_q && d_pair_t && d_position && d_margin,
               "ds_hard_negatives_device: null pointer");
    DS_REQUIRE(min_margin == min_margin, "ds_hard_negatives_device: min_margin is a NaN");
    DS_REQUIRE(q_first <= INT32_MAX - n_queries, "ds_hard_negatives_device: title %lld does not fit an int32 pair_q",
               (long long)(q_first + n_queries));
    if (n_queries == 0) return DS_OK;
    ds::HardArgs a;
    a.rows = d_rows, a.margins = d_margins, a.own_row = d_own_row, a.exclude = n_exclude ? d_exclude : nullptr;
    a.n_queries = n_queries, a.n_truth = n_truth, a.q_first = q_first, a.capacity = capacity;
    a.k = k, a.n_exclude = n_exclude, a.hard_n = hard_n, a.min_margin = min_margin;
    a.offsets = d_offsets, a.pair_q = d_pair_q, a.pair_t = d_pair_t, a.position = d_position, a.margin = d_margin;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t passes = (n_queries + ds::kHardWaves - 1) / ds::kHardWaves;
    const dim3 grid(ds::grid_cap(passes, ds::g_hard_max_blocks.get()));
    DS_LAUNCH(ds::ds_hard_count_kernel, grid, dim3(ds::kHardThreads), 0, s, a);
    DS_LAUNCH(ds::ds_hard_scan_kernel, dim3(1), dim3(ds::kHardScanThreads), 0, s, d_offsets, n_queries, capacity,
              d_total);
    if (k <= 64 * ds::kHardRegisterKeys)
        DS_LAUNCH(ds::ds_hard_emit_kernel<true>, grid, dim3(ds::kHardThreads), 0, s, a);
    else
        DS_LAUNCH(ds::ds_hard_emit_kernel<false>, grid, dim3(ds::kHardThreads), 0, s, a);
    return DS_OK;
}

int ds_hard_total(const int64_t *d_total, int64_t *total, void *stream)
{
    DS_REQUIRE(d_total != nullptr && total != nullptr, "ds_hard_total: null pointer");
    DS_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    int64_t value = 0;
    DS_HIP(hipMemcpy(&value, d_total, sizeof(value), hipMemcpyDeviceToHost));
    *total = value < 0 ? -value : value;
    DS_REQUIRE(value >= 0, "ds_hard_total: the chunks mined %lld pairs, more than the capacity of their output arrays",
               (long long)-value);
    return DS_OK;
}

}  // extern "C"
