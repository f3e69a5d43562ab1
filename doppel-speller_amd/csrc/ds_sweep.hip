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
#include <cmath>

#include "ds_launch.h"
#include "ds_bootstrap_draw.h"
#include "ds_options.h"
#include "ds_wave.h"

namespace ds {

constexpr int kSweepThreads = 256;
constexpr int kSweepWaves = kSweepThreads / 64;     // queries per workgroup and pass
constexpr int kSweepMaxBlocks = 256;                // workgroups along the queries: each adds a whole tile to HBM once
constexpr int kSweepQueriesPerGroup = 64;           // queries per workgroup below that cap ("queries_per_group")
constexpr int kSweepMaxT = 101, kSweepMaxU = 256;
constexpr int kSweepLdsBytes = 48 * 1024;
constexpr int64_t kSweepMaxQueries = int64_t(1) << 40;   // uint32 counters in LDS: a workgroup sees < 2^32 queries

static Option g_sweep_queries_per_group{"queries_per_group", 0, int64_t(1) << 30, kSweepQueriesPerGroup, true};

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

// What the rule leaves of one query at the lane's threshold t, before any u is read: the outcome in the sweep's own
// numbering.  0..3: the same counter in every cell.  4..6: a flip of kind 0 (no actual row), 1 (the model's row is the
// actual one) or 2 (it is another one): "matched" for the u below pos, "none" from pos on; pos is in 1..U then.
struct SweepOutcome {
    int what, pos;
};

// The per-query part of the rule, for the wave that owns query q: the model reduction, pos, and the close walk with
// lane = threshold.  The one home of the rule: ds_threshold_sweep_kernel counts what it returns, ds_sweep_records_kernel
// writes it down.  Every lane of the wave calls it; the answer of a lane that owns no threshold means nothing.
__device__ __forceinline__ SweepOutcome sweep_query(const SweepArgs &a, int64_t q, int lane, int t)
{
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

    int32_t prediction = -1;
    bool flips = false;
    if (exact >= 0) prediction = exact;
    else if (holders == 1 && close_row >= 0) prediction = close_row;
    else flips = model_row >= 0 && pos > 0;
    if (flips) return {4 + (actual < 0 ? 0 : (model_row == actual ? 1 : 2)), pos};
    return {prediction >= 0 ? (prediction == actual ? 0 : 1) : (actual < 0 ? 2 : 3), 0};
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
        const SweepOutcome outcome = sweep_query(a, q, lane, t);
        if (owner) {
            if (outcome.what >= 4) atomicAdd(mine + 4 + (outcome.what - 4) * bins + outcome.pos, 1u);
            else atomicAdd(mine + outcome.what, 1u);
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

// ---- the record of a (title, t) (include/doppel_amd.h, "sweep records") -------------------------------------------------
// One wave per query as above, gridDim.y tiles t by 64, and the lane that owns a threshold writes sweep_query's answer as
// one uint16: the low three bits the outcome (0..3 fixed, in the numbering of bootstrap.ACCURACY_CODES; 4..6 the three
// flips), bits 3..15 pos for a flip and 0 otherwise.  A flip with pos == U is "matched" in every cell of the grid and is
// written as that fixed outcome, so a record is a function of the title's U outcomes alone (and pos is in 1..U - 1
// here; ds_sweep_bootstrap_device takes 1..U).  Nothing is counted, so there is no LDS and no atomic.
__device__ __forceinline__ uint16_t sweep_record(SweepOutcome outcome, int U)
{
    // sweep counter 0, 1, 2, 3 = code 3 (correctly matched), 1 (incorrectly matched), 0 (correctly not found), 2
    if (outcome.what < 4) return static_cast<uint16_t>(outcome.what == 0 ? 3 : outcome.what == 1 ? 1 : outcome.what == 2 ? 0 : 2);
    if (outcome.pos >= U) return static_cast<uint16_t>(outcome.what == 5 ? 3 : 1);
    return static_cast<uint16_t>(outcome.what | (outcome.pos << 3));
}

__global__ __launch_bounds__(kSweepThreads) void ds_sweep_records_kernel(SweepArgs a, uint16_t *records)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t_first = blockIdx.y * 64;
    const bool owner = t_first + lane < a.T;
    const int t = owner ? a.lev[t_first + lane] : 0;
    for (int64_t q = static_cast<int64_t>(blockIdx.x) * kSweepWaves + wave; q < a.n_queries;
         q += static_cast<int64_t>(gridDim.x) * kSweepWaves) {
        const SweepOutcome outcome = sweep_query(a, q, lane, t);
        if (owner) records[q * a.T + t_first + lane] = sweep_record(outcome, a.U);
    }
}

// ---- the paired bootstrap of every cell ("Bootstrap of the cells") ---------------------------------
// Replicate b draws n_units units, draw k by bootstrap_unit (ds_bootstrap_draw.h: the closed form of ds_bootstrap.hip), and
// a drawn unit adds all its titles (its member list; without units the title itself).  Replicate n_boot is the baseline.
//
// One WAVE owns a (replicate, tile of thresholds) and lane l owns threshold l of the tile.  The wave generates 64 draws at
// a time, one per lane, and hands them round with readlane; for a drawn title every owning lane reads its own record (a
// title's T records are contiguous: one coalesced read) and adds 1 to one of its 4 + 3 U counters in LDS: the four fixed
// outcomes, and per flip kind a histogram over pos = 1..U.  Counter s of lane l is word s * tile + l of the wave's
// region, so the lanes of one add sit on consecutive words when they agree on s, and nothing in LDS is shared between
// lanes: no barrier, no conflict between owners, and an LDS add without return is one instruction.  At the end a lane
// walks u upwards with the prefix sums of its three histograms and writes its [b][t][0..U)[4] block itself, so nothing
// in HBM is added to and nothing has to be zeroed.  Integer sums of the same terms: no bit depends on the tiling, the
// grid or the order.
//
// LDS: kSweepBootWaveBytes = 16 KiB per wave bounds the tile (64 thresholds up to U = 20, 26 at U = 50, 5 at U = 256)
// and the workgroup takes what its four tiles need, 64 KiB at the most: two workgroups (8 waves) per CU at worst, three
// on a 20 x 50 grid (48,960 B).  The loop waits on the record read, so waves per CU matter more than thresholds per wave.
// The counters are uint32: the launcher refuses n_units x the largest unit >= 2^32, the most one replicate can add.
constexpr int kSweepBootThreads = 256;
constexpr int kSweepBootWaves = kSweepBootThreads / 64;
constexpr int kSweepBootWaveBytes = 16 * 1024;
constexpr int kSweepBootMax = 1 << 16;
constexpr int64_t kSweepBootTitlesMax = (int64_t(1) << 31) - 1;
constexpr int kSweepBootMaxBlocks = 4096;              // default cap of the grid
constexpr int kSweepBootReplicatesPerGroup = kSweepBootWaves;
constexpr int kSweepBootRowThreads = 256;
constexpr int kSweepBootScanThreads = 1024;

// for tests (ds_sweep_option); no result depends on them
static Option g_sweep_boot_tile{"bootstrap_tile", 0, 64, 0};   // thresholds per tile; 0: what kSweepBootWaveBytes holds
static Option g_sweep_boot_max_blocks{"bootstrap_max_blocks", 0, 65535, kSweepBootMaxBlocks, true};
static Option g_sweep_boot_replicates_per_group{"bootstrap_replicates_per_group", 0, kSweepBootMax + 1,
                                                kSweepBootReplicatesPerGroup, true};
static Option *const g_sweep_options[] = {&g_sweep_queries_per_group, &g_sweep_boot_tile, &g_sweep_boot_max_blocks,
                                          &g_sweep_boot_replicates_per_group};

struct SweepBootArgs {
    const uint16_t *records;       // [n][T]
    const int32_t *offsets;        // [n_units + 1], null without units
    const int32_t *members;        // [n]: the titles of unit u are members[offsets[u] .. offsets[u + 1])
    unsigned long long *counts;    // [n_boot][T][U][4]
    unsigned long long *baseline;  // [T][U][4]
    uint64_t seed;
    int64_t n_units;
    int32_t T, U, tile_t, n_tiles, n_boot, per_group, n_groups;
};

// errors[0]: records that no (title, t) can have (low bits 7, a pos other than 0 on a fixed outcome, a pos outside 1..U on
// a flip); errors[1]: units outside [0, n_units).  With units, sizes[u] counts the titles of unit u.
__global__ __launch_bounds__(kSweepBootRowThreads) void ds_sweep_bootstrap_check_kernel(
    const uint16_t *records, const int32_t *unit, int64_t n, int32_t T, int32_t U, int64_t n_units, uint32_t *sizes,
    unsigned long long *errors)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kSweepBootRowThreads + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * kSweepBootRowThreads) {
        unsigned long long bad = 0;
        for (int32_t t = 0; t < T; ++t) {
            const uint32_t record = records[i * T + t], what = record & 7u, pos = record >> 3;
            bad += what == 7u || (what < 4u ? pos != 0u : (pos < 1u || pos > static_cast<uint32_t>(U)));
        }
        if (bad) atomicAdd(&errors[0], bad);
        if (unit != nullptr) {
            const int64_t u = unit[i];
            if (u < 0 || u >= n_units) atomicAdd(&errors[1], 1ull);
            else atomicAdd(&sizes[u], 1u);
        }
    }
}

// The counting sort's scan, one workgroup: offsets[u] = the titles of the units before u (offsets[n_units] = n), a copy
// of it in cursor for the fill, and errors[2] = the largest unit.
__global__ __launch_bounds__(kSweepBootScanThreads) void ds_sweep_bootstrap_scan_kernel(const uint32_t *sizes, int64_t n_units,
                                                                                       int32_t *offsets, uint32_t *cursor,
                                                                                       unsigned long long *errors)
{
    __shared__ uint32_t s_waves[kSweepBootScanThreads / 64];
    uint32_t running = 0u, largest = 0u;
    for (int64_t base = 0; base < n_units; base += kSweepBootScanThreads) {
        const int64_t u = base + threadIdx.x;
        const uint32_t value = u < n_units ? sizes[u] : 0u;
        uint32_t total;
        const uint32_t before = block_exclusive<kSweepBootScanThreads>(value, s_waves, total);
        if (u < n_units) {
            offsets[u] = static_cast<int32_t>(running + before);
            cursor[u] = running + before;
        }
        running += total;
        largest = max(largest, value);
    }
    largest = wave_max(largest);
    if ((threadIdx.x & 63) == 0) atomicMax(&errors[2], static_cast<unsigned long long>(largest));
    if (threadIdx.x == 0) offsets[n_units] = static_cast<int32_t>(running);
}

// The counting sort's scatter: title i takes the next free place of its unit.  The order inside a unit's list is the
// order of arrival; a drawn unit adds ALL its titles, and integer sums do not depend on the order of their terms.
__global__ __launch_bounds__(kSweepBootRowThreads) void ds_sweep_bootstrap_fill_kernel(const int32_t *unit, int64_t n,
                                                                                      uint32_t *cursor, int32_t *members)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kSweepBootRowThreads + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * kSweepBootRowThreads)
        members[atomicAdd(&cursor[unit[i]], 1u)] = static_cast<int32_t>(i);
}

// One record decoded into the lane's counters: slot 0..3 for a fixed outcome, 4 + kind * U + (pos - 1) for a flip.
__device__ __forceinline__ void sweep_boot_add(uint32_t *mine, int stride, int U, uint32_t record)
{
    const int what = record & 7u, pos = record >> 3;
    const int slot = what < 4 ? what : 4 + (what - 4) * U + pos - 1;
    atomicAdd(mine + slot * stride, 1u);
}

// `count` titles, title_at(i) the same in every lane: four record reads in flight, then their four adds.
template <typename TitleAt>
__device__ __forceinline__ void sweep_boot_titles(int count, TitleAt title_at, bool owner, const uint16_t *column,
                                                  int64_t T, uint32_t *mine, int stride, int U)
{
    int i = 0;
    for (; i + 4 <= count; i += 4) {
        const int64_t t0 = title_at(i), t1 = title_at(i + 1), t2 = title_at(i + 2), t3 = title_at(i + 3);
        if (owner) {
            const uint32_t r0 = column[t0 * T], r1 = column[t1 * T], r2 = column[t2 * T], r3 = column[t3 * T];
            sweep_boot_add(mine, stride, U, r0);
            sweep_boot_add(mine, stride, U, r1);
            sweep_boot_add(mine, stride, U, r2);
            sweep_boot_add(mine, stride, U, r3);
        }
    }
    for (; i < count; ++i) {
        const int64_t t0 = title_at(i);
        if (owner) sweep_boot_add(mine, stride, U, column[t0 * T]);
    }
}

template <bool kUnits>
__global__ __launch_bounds__(kSweepBootThreads) void ds_sweep_bootstrap_kernel(SweepBootArgs a)
{
    extern __shared__ uint32_t boot_lds[];   // [wave][4 + 3 U counters][tile_t lanes]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int U = a.U, stride = a.tile_t, slots = 4 + 3 * U;
    uint32_t *mine = boot_lds + wave * slots * stride + (lane < stride ? lane : 0);
    for (int32_t group = blockIdx.x; group < a.n_groups; group += gridDim.x) {
        const int32_t begin = group * a.per_group;
        const int32_t end = begin + a.per_group < a.n_boot + 1 ? begin + a.per_group : a.n_boot + 1;
        const int64_t items = static_cast<int64_t>(end - begin) * a.n_tiles;
        for (int64_t item = wave; item < items; item += kSweepBootWaves) {   // wave-uniform: no barrier anywhere
            const int32_t b = begin + static_cast<int32_t>(item / a.n_tiles);
            const int t_first = static_cast<int>(item % a.n_tiles) * a.tile_t;
            const bool owner = lane < a.tile_t && t_first + lane < a.T;
            if (owner)
                for (int s = 0; s < slots; ++s) mine[s * stride] = 0u;
            const uint16_t *column = a.records + t_first + (owner ? lane : 0);   // title i: column[i * T]
            for (int64_t k0 = 0; k0 < a.n_units; k0 += 64) {
                const int64_t k = k0 + lane;
                const int32_t drawn =
                    k < a.n_units ? static_cast<int32_t>(bootstrap_unit(a.seed, b, a.n_boot, k, a.n_units)) : 0;
                const int filled = static_cast<int>(a.n_units - k0 < 64 ? a.n_units - k0 : 64);
                if (!kUnits) {
                    sweep_boot_titles(filled, [drawn](int i) { return __builtin_amdgcn_readlane(drawn, i); }, owner,
                                      column, a.T, mine, stride, U);
                } else {
                    for (int i = 0; i < filled; ++i) {
                        const int32_t unit = __builtin_amdgcn_readlane(drawn, i);
                        const int32_t first = a.offsets[unit];
                        const int32_t *list = a.members + first;
                        sweep_boot_titles(a.offsets[unit + 1] - first, [list](int m) { return list[m]; }, owner, column,
                                          a.T, mine, stride, U);
                    }
                }
            }
            if (owner) {
                // cell u: a flip is "matched" while u < pos, that is for the histogram entries pos - 1 >= u
                unsigned long long *out = (b == a.n_boot ? a.baseline : a.counts + static_cast<int64_t>(b) * a.T * U * 4) +
                                          static_cast<int64_t>(t_first + lane) * U * 4;
                const uint32_t *none = mine + 4 * stride, *right = none + U * stride, *wrong = right + U * stride;
                uint32_t none_all = 0, right_all = 0, wrong_all = 0;
                for (int p = 0; p < U; ++p) {
                    none_all += none[p * stride];
                    right_all += right[p * stride];
                    wrong_all += wrong[p * stride];
                }
                const unsigned long long fixed0 = mine[0], fixed1 = mine[stride], fixed2 = mine[2 * stride],
                                         fixed3 = mine[3 * stride];
                uint32_t none_off = 0, right_off = 0, wrong_off = 0;   // the flips with pos <= u: "none" at u
                for (int u = 0; u < U; ++u) {
                    out[u * 4 + 0] = fixed0 + none_off;
                    out[u * 4 + 1] = fixed1 + (none_all - none_off) + (wrong_all - wrong_off);
                    out[u * 4 + 2] = fixed2 + right_off + wrong_off;
                    out[u * 4 + 3] = fixed3 + (right_all - right_off);
                    none_off += none[u * stride];
                    right_off += right[u * stride];
                    wrong_off += wrong[u * stride];
                }
            }
        }
    }
}

static int sweep_boot_tile(int32_t T, int32_t U)
{
    const int fits = kSweepBootWaveBytes / ((4 + 3 * U) * static_cast<int>(sizeof(uint32_t)));
    int tile = std::max(1, std::min({static_cast<int>(T), 64, fits}));
    const int64_t forced = g_sweep_boot_tile.get();
    if (forced > 0) tile = static_cast<int>(std::min<int64_t>(forced, tile));
    return tile;
}

template <bool kUnits>
static int sweep_boot_launch(const SweepBootArgs &args, unsigned grid, size_t lds)
{
    DS_TRY(ds::allow_dynamic_lds(ds_sweep_bootstrap_kernel<kUnits>, lds));
    DS_LAUNCH((ds_sweep_bootstrap_kernel<kUnits>), dim3(grid), dim3(kSweepBootThreads), lds, nullptr, args);
    return DS_OK;
}

// The argument checks that ds_threshold_sweep_device and ds_sweep_records_device share, the grid's values among them:
// those are read back and checked here, T + U small values behind one synchronisation of `queue`.
static int sweep_check(const char *what, int64_t n_queries, int32_t k, const int32_t *d_lev, int32_t T, const float *d_prob,
                       int32_t U, const void *d_out, hipStream_t queue)
{
    DS_REQUIRE(n_queries >= 0 && n_queries <= kSweepMaxQueries, "%s: n_queries = %lld out of range", what,
               (long long)n_queries);
    DS_REQUIRE(k >= 1, "%s: k = %d, must be positive", what, k);
    DS_REQUIRE(T >= 1 && T <= kSweepMaxT, "%s: T = %d out of range [1, %d]", what, T, kSweepMaxT);
    DS_REQUIRE(U >= 1 && U <= kSweepMaxU, "%s: U = %d out of range [1, %d]", what, U, kSweepMaxU);
    DS_REQUIRE(d_lev && d_prob && d_out, "%s: null pointer", what);
    DS_REQUIRE(n_queries <= INT64_MAX / k, "%s: too many pairs", what);
    int32_t lev[kSweepMaxT];
    float prob[kSweepMaxU];
    DS_HIP(hipMemcpyAsync(lev, d_lev, sizeof(int32_t) * T, hipMemcpyDeviceToHost, queue));
    DS_HIP(hipMemcpyAsync(prob, d_prob, sizeof(float) * U, hipMemcpyDeviceToHost, queue));
    DS_HIP(hipStreamSynchronize(queue));
    for (int32_t i = 0; i < T; ++i) {
        DS_REQUIRE(lev[i] >= 0 && lev[i] <= 100, "%s: Levenshtein threshold %d out of range [0, 100]", what, lev[i]);
        DS_REQUIRE(i == 0 || lev[i] > lev[i - 1], "%s: Levenshtein thresholds must ascend strictly", what);
    }
    for (int32_t i = 0; i < U; ++i) {
        DS_REQUIRE(std::isfinite(prob[i]), "%s: probability threshold %d is not finite", what, i);
        DS_REQUIRE(i == 0 || prob[i] > prob[i - 1], "%s: probability thresholds must ascend strictly", what);
    }
    return DS_OK;
}

static unsigned sweep_query_groups(int64_t n_queries)
{
    const int64_t per_group = std::max<int64_t>(g_sweep_queries_per_group.get(), kSweepWaves);
    return grid_cap((n_queries + per_group - 1) / per_group, kSweepMaxBlocks);
}

}  // namespace ds

extern "C" {

int ds_sweep_option(const char *name, int64_t value)
{
    return ds::set_option("ds_sweep_option", ds::g_sweep_options, name, value);
}

int ds_threshold_sweep_device(const int32_t *d_rows, const uint8_t *d_d, const uint8_t *d_r, const uint8_t *d_s,
                              const float *d_predictions, const int32_t *d_exact, const int32_t *d_actual_row,
                              int64_t n_queries, int32_t k, const int32_t *d_lev, int32_t T, const float *d_prob,
                              int32_t U, int64_t *d_counts, void *stream)
{
    hipStream_t queue = static_cast<hipStream_t>(stream);
    DS_TRY(ds::sweep_check("ds_threshold_sweep_device", n_queries, k, d_lev, T, d_prob, U, d_counts, queue));
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
    const dim3 grid(ds::sweep_query_groups(n_queries), static_cast<unsigned>((T + args.tile_t - 1) / args.tile_t));
    DS_LAUNCH(ds::ds_threshold_sweep_kernel, grid, dim3(ds::kSweepThreads),
              static_cast<size_t>(args.tile_t) * per_t_bytes, queue, args);
    return DS_OK;
}

int ds_sweep_records_device(const int32_t *d_rows, const uint8_t *d_d, const uint8_t *d_r, const uint8_t *d_s,
                            const float *d_predictions, const int32_t *d_exact, const int32_t *d_actual_row,
                            int64_t n_queries, int32_t k, const int32_t *d_lev, int32_t T, const float *d_prob, int32_t U,
                            uint16_t *d_records)
{
    DS_TRY(ds::sweep_check("ds_sweep_records_device", n_queries, k, d_lev, T, d_prob, U, d_records, nullptr));
    if (n_queries == 0) return DS_OK;
    DS_REQUIRE(d_rows && d_d && d_r && d_s && d_predictions && d_exact && d_actual_row,
               "ds_sweep_records_device: null pointer");
    ds::SweepArgs args{};
    args.rows = d_rows; args.d = d_d; args.r = d_r; args.s = d_s; args.predictions = d_predictions;
    args.exact = d_exact; args.actual = d_actual_row; args.lev = d_lev; args.prob = d_prob;
    args.n_queries = n_queries; args.k = k; args.T = T; args.U = U; args.tile_t = 64;
    const dim3 grid(ds::sweep_query_groups(n_queries), static_cast<unsigned>((T + 63) / 64));
    DS_LAUNCH(ds::ds_sweep_records_kernel, grid, dim3(ds::kSweepThreads), 0, nullptr, args, d_records);
    return DS_OK;
}

int ds_sweep_bootstrap_device(const uint16_t *d_records, int64_t n, int32_t T, int32_t U, const int32_t *d_unit,
                              int64_t n_units, int32_t n_boot, uint64_t seed, int64_t *d_counts, int64_t *d_baseline)
{
    const char *what = "ds_sweep_bootstrap_device";
    DS_REQUIRE(n >= 0 && n <= ds::kSweepBootTitlesMax, "%s: n = %lld outside [0, 2^31)", what, (long long)n);
    DS_REQUIRE(n_boot >= 1 && n_boot <= ds::kSweepBootMax, "%s: n_boot = %d outside [1, %d]", what, n_boot,
               ds::kSweepBootMax);
    DS_REQUIRE(T >= 1 && T <= ds::kSweepMaxT, "%s: T = %d out of range [1, %d]", what, T, ds::kSweepMaxT);
    DS_REQUIRE(U >= 1 && U <= ds::kSweepMaxU, "%s: U = %d out of range [1, %d]", what, U, ds::kSweepMaxU);
    if (d_unit != nullptr)
        DS_REQUIRE(n == 0 || (n_units >= 1 && n_units <= ds::kSweepBootTitlesMax), "%s: n_units = %lld outside [1, 2^31)",
                   what, (long long)n_units);
    else
        DS_REQUIRE(n_units == n, "%s: n_units = %lld, but without units every one of the %lld titles is its own unit", what,
                   (long long)n_units, (long long)n);
    DS_REQUIRE(d_counts != nullptr && d_baseline != nullptr && (n == 0 || d_records != nullptr), "%s: null pointer", what);
    const size_t cells = static_cast<size_t>(T) * U * 4;
    if (n == 0) {
        DS_HIP(hipMemsetAsync(d_counts, 0, sizeof(int64_t) * cells * n_boot, nullptr));
        DS_HIP(hipMemsetAsync(d_baseline, 0, sizeof(int64_t) * cells, nullptr));
        return DS_OK;
    }
    const bool units = d_unit != nullptr;
    ds::DeviceBuffer<unsigned long long> errors;
    ds::DeviceBuffer<uint32_t> sizes, cursor;
    ds::DeviceBuffer<int32_t> offsets, members;
    DS_TRY(errors.allocate(3));
    DS_HIP(hipMemsetAsync(errors.ptr, 0, errors.bytes(), nullptr));
    if (units) {
        DS_TRY(sizes.allocate(static_cast<size_t>(n_units)));
        DS_TRY(cursor.allocate(static_cast<size_t>(n_units)));
        DS_TRY(offsets.allocate(static_cast<size_t>(n_units) + 1));
        DS_TRY(members.allocate(static_cast<size_t>(n)));
        DS_HIP(hipMemsetAsync(sizes.ptr, 0, sizes.bytes(), nullptr));
    }
    const int64_t cap = ds::g_sweep_boot_max_blocks.get();
    const dim3 rows(ds::grid_cap((n + ds::kSweepBootRowThreads - 1) / ds::kSweepBootRowThreads, cap));
    DS_LAUNCH(ds::ds_sweep_bootstrap_check_kernel, rows, dim3(ds::kSweepBootRowThreads), 0, nullptr, d_records,
              d_unit, n, T, U, n_units, sizes.ptr, errors.ptr);
    if (units) {   // the scan reads sizes of valid units only; its offsets are used only when the check has passed
        DS_LAUNCH(ds::ds_sweep_bootstrap_scan_kernel, dim3(1), dim3(ds::kSweepBootScanThreads), 0, nullptr,
                  sizes.ptr, n_units, offsets.ptr, cursor.ptr, errors.ptr);
    }
    unsigned long long found[3] = {0, 0, 0};
    DS_HIP(hipMemcpyAsync(found, errors.ptr, sizeof(found), hipMemcpyDeviceToHost, nullptr));
    DS_HIP(hipStreamSynchronize(nullptr));
    DS_REQUIRE(found[0] == 0, "%s: %llu records are none that a (title, threshold) can have with U = %d", what, found[0], U);
    DS_REQUIRE(found[1] == 0, "%s: %llu units are outside [0, %lld)", what, found[1], (long long)n_units);
    // uint32 counters in LDS: a replicate adds at most n_units x the largest unit titles to one counter
    const unsigned long long largest = units ? found[2] : 1ull;
    DS_REQUIRE(static_cast<unsigned long long>(n_units) * largest < (1ull << 32),
               "%s: %lld units x %llu titles in the largest unit is 2^32 or more, what one replicate may add", what,
               (long long)n_units, largest);
    if (units) {
        DS_LAUNCH(ds::ds_sweep_bootstrap_fill_kernel, rows, dim3(ds::kSweepBootRowThreads), 0, nullptr, d_unit, n,
                  cursor.ptr, members.ptr);
    }
    ds::SweepBootArgs args{};
    args.records = d_records;
    args.offsets = offsets.ptr;
    args.members = members.ptr;
    args.counts = reinterpret_cast<unsigned long long *>(d_counts);
    args.baseline = reinterpret_cast<unsigned long long *>(d_baseline);
    args.seed = seed;
    args.n_units = n_units;
    args.T = T; args.U = U; args.n_boot = n_boot;
    args.tile_t = ds::sweep_boot_tile(T, U);
    args.n_tiles = (T + args.tile_t - 1) / args.tile_t;
    const int64_t replicates = static_cast<int64_t>(n_boot) + 1;   // and the baseline
    const int64_t per_group = std::min(ds::g_sweep_boot_replicates_per_group.get(), replicates);
    args.per_group = static_cast<int32_t>(per_group);
    args.n_groups = static_cast<int32_t>((replicates + per_group - 1) / per_group);
    const unsigned grid = ds::grid_cap(args.n_groups, cap);
    const size_t lds = static_cast<size_t>(ds::kSweepBootWaves) * (4 + 3 * U) * args.tile_t * sizeof(uint32_t);
    DS_TRY(units ? ds::sweep_boot_launch<true>(args, grid, lds) : ds::sweep_boot_launch<false>(args, grid, lds));
    if (units) DS_HIP(hipStreamSynchronize(nullptr));   // the member lists are freed on return
    return DS_OK;
}

}  // extern "C"
