// What the printed probability means ("Calibration"): the isotonic fit of 0/1 labels on a score, the
// step map it defines, and the reliability counters of a probability.  Every sum is an integer sum and every position a
// function of the keys alone: the same bits for any grid, any segment width and from run to run.
//
// ds_isotonic_fit_device, all on one stream with no host round trip before the last copy:
//   1. ds_isotonic_split_kernel    key = cut_key(score) (ds_radix.h); a NaN row is counted and dropped, the others go to
//                                  the column of their label (0: target == 0, 1: the rest), in the order in which the
//                                  waves arrive: a column is a multiset.  Both columns have length n; the tail keeps the
//                                  padding key 0xFFFFFFFF, which sorts last (ds_metrics.hip explains why it may stay out
//                                  of the OR / AND).
//   2. radix_sort_columns          both columns at once.
//   3. ds_isotonic_heads_kernel    element e of the negatives followed by the positives is a HEAD when it is the first of
//                                  its key there, and for a positive when no negative has that key (binary search).
//      ds_isotonic_tile_scan_kernel / ds_isotonic_scan_kernel: S[e] = the heads before e, S[n_neg + n_pos] = D.
//      ds_isotonic_points_kernel   a head writes point S-rank of its key in the merged order, with the two run lengths.
//   4. ds_isotonic_pool_kernel     level 1: a segment of W points per workgroup of one wave.  Every lane pools its own
//                                  slice of the segment by the stack algorithm in LDS, the slices' blocks are compacted
//                                  and lane 0 pools them to the end; the segment's blocks go to its own slots in HBM.
//      ds_isotonic_finish_kernel   level 2: one workgroup stages the survivors of many segments at a time in LDS and one
//                                  thread pools them to the end, its stack in the slots already consumed.
//      ds_isotonic_blocks_kernel   lo, hi, pos, neg of the K blocks.
// Two blocks are pooled when mean(left) >= mean(right), compared as pos_l * tot_r >= pos_r * tot_l in 64 bits (counts are
// below 2^31).  Pooling adjacent violators inside a window never joins what the global solution separates, and blocks of
// equal mean end in one level set whatever lies around them, so the result does not depend on the windows.
#include <algorithm>

#include "ds_launch.h"
#include "ds_metrics.h"
#include "ds_options.h"
#include "ds_radix.h"

namespace ds {

constexpr int kCalibrateThreads = 256;
constexpr int kCalibrateWaves = kCalibrateThreads / 64;
constexpr int kCalibrateDefaultBlocks = 2048;          // default cap of every grid
constexpr int kSplitRows = 8;                          // rows of a lane per pass of the split
constexpr int kSplitWaveRows = kSplitRows * 64;
constexpr int kCalibrateHeadTile = 2048;               // elements of one workgroup's piece of the head scan
constexpr int kCalibrateSegmentDefault = 1024;         // points of a level-1 segment
constexpr int kCalibrateSegmentMax = 2048;
constexpr uint32_t kFinishStack = 2048;                // blocks of the last level's stack kept in LDS
constexpr int64_t kCalibrateRowsMax = int64_t(1) << 31;   // exclusive
constexpr int kCalibrateEdgesInLds = 16384;            // block edges staged by the map: 64 KiB of keys
constexpr int kReliabilityBinsMax = 256;
constexpr uint32_t kNanKey = 0xffffffffu;

// for tests (ds_calibrate_option); no result depends on them
static Option g_calibrate_max_blocks{"max_blocks", 0, 65535, kCalibrateDefaultBlocks, true};
static Option g_calibrate_segment_points{"segment_points", 2, kCalibrateSegmentMax, kCalibrateSegmentDefault, true};
static Option *const g_calibrate_options[] = {&g_calibrate_max_blocks, &g_calibrate_segment_points};

// the uint32 state block of a fit in HBM
enum { kStateNeg = 0, kStatePos, kStateNan, kStatePoints, kStateBlocks, kStateSurvivors, kStateOr = 8, kStateAnd = 10,
       kStateWords = 12 };

static unsigned calibrate_grid(int64_t items)
{
    return grid_cap(items, g_calibrate_max_blocks.get());
}

__global__ void ds_isotonic_begin_kernel(uint32_t *state)
{
    if (threadIdx.x < kStateWords) state[threadIdx.x] = threadIdx.x >= kStateAnd ? 0xffffffffu : 0u;
}

// ---- 1. keys, split by label ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCalibrateThreads) void ds_isotonic_split_kernel(const float *scores, const float *labels,
                                                                               int64_t n, uint32_t *keys, uint32_t *state)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lower = (1ull << lane) - 1ull;
    uint32_t any[2] = {0u, 0u}, all[2] = {0xffffffffu, 0xffffffffu}, nan = 0u;
    // A wave takes kSplitRows * 64 consecutive rows per pass, lane l the rows l, l + 64, ...: one atomic per column and
    // pass reserves the places of all of them (one per 64 rows made the two counters the whole kernel's time).  The loop
    // bounds are wave-uniform: every lane of a wave takes part in its ballots.
    for (int64_t base = (blockIdx.x * static_cast<int64_t>(kCalibrateWaves) + wave) * kSplitWaveRows; base < n;
         base += static_cast<int64_t>(gridDim.x) * kCalibrateWaves * kSplitWaveRows) {
        uint32_t key[kSplitRows];
        unsigned long long negatives[kSplitRows], positives[kSplitRows];
        uint32_t count_neg = 0u, count_pos = 0u;
#pragma unroll
        for (int j = 0; j < kSplitRows; ++j) {
            const int64_t r = base + j * 64 + lane;
            const bool valid = r < n;
            key[j] = valid ? cut_key(__float_as_uint(scores[r])) : kNanKey;
            const bool kept = valid && key[j] != kNanKey;
            const bool positive = kept && labels[r] != 0.f;
            nan += valid && !kept ? 1u : 0u;
            negatives[j] = __ballot(kept && !positive);
            positives[j] = __ballot(positive);
            count_neg += __popcll(negatives[j]);
            count_pos += __popcll(positives[j]);
        }
        uint32_t first_neg = 0u, first_pos = 0u;
        if (lane == 0) {
            if (count_neg) first_neg = atomicAdd(&state[kStateNeg], count_neg);
            if (count_pos) first_pos = atomicAdd(&state[kStatePos], count_pos);
        }
        first_neg = __shfl(first_neg, 0);
        first_pos = __shfl(first_pos, 0);
#pragma unroll
        for (int j = 0; j < kSplitRows; ++j) {
            if ((negatives[j] >> lane) & 1ull) {
                keys[first_neg + __popcll(negatives[j] & lower)] = key[j];
                any[0] |= key[j];
                all[0] &= key[j];
            } else if ((positives[j] >> lane) & 1ull) {
                keys[n + first_pos + __popcll(positives[j] & lower)] = key[j];
                any[1] |= key[j];
                all[1] &= key[j];
            }
            first_neg += __popcll(negatives[j]);
            first_pos += __popcll(positives[j]);
        }
    }
    nan = wave_sum(nan);
    for (int c = 0; c < 2; ++c) {
        any[c] = wave_or(any[c]);
        all[c] = wave_and(all[c]);
    }
    if (lane == 0) {
        if (nan) atomicAdd(&state[kStateNan], nan);
        for (int c = 0; c < 2; ++c) {
            if (any[c]) atomicOr(&state[kStateOr + c], any[c]);
            if (all[c] != 0xffffffffu) atomicAnd(&state[kStateAnd + c], all[c]);
        }
    }
}

// ---- 3. one point per distinct key ---------------------------------------------------------------------------------------
struct SortedColumns {
    const uint32_t *neg, *pos;
    uint32_t n_neg, n_pos;
};

__device__ inline SortedColumns sorted_columns(const uint32_t *keys_a, const uint32_t *keys_b, int64_t n,
                                               const uint32_t *state)
{
    SortedColumns s;
    s.neg = (passes_done(state[kStateOr] ^ state[kStateAnd], 4) & 1) ? keys_b : keys_a;
    s.pos = ((passes_done(state[kStateOr + 1] ^ state[kStateAnd + 1], 4) & 1) ? keys_b : keys_a) + n;
    s.n_neg = state[kStateNeg];
    s.n_pos = state[kStatePos];
    return s;
}

// the number of keys of sorted[0, count) below `key` (kUpper: not above it), searched from `from`
template <bool kUpper>
__device__ inline uint32_t key_bound(const uint32_t *sorted, uint32_t from, uint32_t count, uint32_t key)
{
    uint32_t lo = from, hi = count;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (kUpper ? sorted[mid] <= key : sorted[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ inline bool is_head(const SortedColumns &s, uint32_t e)
{
    if (e < s.n_neg) return e == 0u || s.neg[e - 1] != s.neg[e];
    const uint32_t j = e - s.n_neg, key = s.pos[j];
    if (j > 0u && s.pos[j - 1] == key) return false;
    const uint32_t at = key_bound<false>(s.neg, 0u, s.n_neg, key);
    return !(at < s.n_neg && s.neg[at] == key);
}

// heads[e] = 1 for a head, e <= n_neg + n_pos (the last one is 0: it receives the total); totals[tile] = the tile's heads
__global__ __launch_bounds__(kCalibrateThreads) void ds_isotonic_heads_kernel(const uint32_t *keys_a, const uint32_t *keys_b,
                                                                               int64_t n, const uint32_t *state,
                                                                               uint32_t *heads, uint32_t *totals,
                                                                               int64_t tiles)
{
    __shared__ uint32_t s_sum;
    const SortedColumns s = sorted_columns(keys_a, keys_b, n, state);
    const int64_t count = static_cast<int64_t>(s.n_neg) + s.n_pos;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        if (threadIdx.x == 0) s_sum = 0u;
        __syncthreads();
        uint32_t mine = 0u;
        const int64_t begin = tile * kCalibrateHeadTile, end = std::min<int64_t>(begin + kCalibrateHeadTile, count + 1);
        for (int64_t e = begin + threadIdx.x; e < end; e += kCalibrateThreads) {
            const uint32_t head = e < count && is_head(s, static_cast<uint32_t>(e)) ? 1u : 0u;
            heads[e] = head;
            mine += head;
        }
        mine = wave_sum(mine);
        if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_sum, mine);
        __syncthreads();
        if (threadIdx.x == 0) totals[tile] = s_sum;
        __syncthreads();
    }
}

// exclusive scan of the tiles' totals in place, by one workgroup; the grand total is the number of points
__global__ __launch_bounds__(kScanThreads) void ds_isotonic_tile_scan_kernel(uint32_t *totals, int64_t tiles, uint32_t *state)
{
    __shared__ uint32_t s_waves[kScanThreads / 64];
    uint32_t running = 0u;
    for (int64_t base = 0; base < tiles; base += kScanThreads) {
        const int64_t i = base + threadIdx.x;
        const uint32_t value = i < tiles ? totals[i] : 0u;
        uint32_t total;
        const uint32_t before = block_exclusive<kScanThreads>(value, s_waves, total);
        if (i < tiles) totals[i] = running + before;
        running += total;
    }
    if (threadIdx.x == 0) state[kStatePoints] = running;
}

// heads[e] -> S[e], the heads before e
__global__ __launch_bounds__(kCalibrateThreads) void ds_isotonic_scan_kernel(const uint32_t *state, uint32_t *heads,
                                                                              const uint32_t *totals, int64_t tiles)
{
    __shared__ uint32_t s_waves[kCalibrateWaves];
    const int64_t count = static_cast<int64_t>(state[kStateNeg]) + state[kStatePos];
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        uint32_t running = totals[tile];
        const int64_t begin = tile * kCalibrateHeadTile, end = std::min<int64_t>(begin + kCalibrateHeadTile, count + 1);
        for (int64_t base = begin; base < end; base += kCalibrateThreads) {   // uniform over the workgroup
            const int64_t e = base + threadIdx.x;
            const uint32_t value = e < end ? heads[e] : 0u;
            uint32_t total;
            const uint32_t before = block_exclusive<kCalibrateThreads>(value, s_waves, total);
            if (e < end) heads[e] = running + before;
            running += total;
        }
    }
}

__global__ __launch_bounds__(kCalibrateThreads) void ds_isotonic_points_kernel(const uint32_t *keys_a, const uint32_t *keys_b,
                                                                                int64_t n, const uint32_t *state,
                                                                                const uint32_t *S, uint32_t *pt_key,
                                                                                uint32_t *pt_pos, uint32_t *pt_neg)
{
    const SortedColumns s = sorted_columns(keys_a, keys_b, n, state);
    const int64_t count = static_cast<int64_t>(s.n_neg) + s.n_pos;
    const uint32_t neg_heads = S[s.n_neg];
    for (int64_t e = blockIdx.x * static_cast<int64_t>(kCalibrateThreads) + threadIdx.x; e < count;
         e += static_cast<int64_t>(gridDim.x) * kCalibrateThreads) {
        if (S[e + 1] == S[e]) continue;
        uint32_t key, point, neg, pos;
        if (e < s.n_neg) {
            const uint32_t i = static_cast<uint32_t>(e);
            key = s.neg[i];
            const uint32_t first = key_bound<false>(s.pos, 0u, s.n_pos, key);
            neg = key_bound<true>(s.neg, i, s.n_neg, key) - i;
            pos = key_bound<true>(s.pos, first, s.n_pos, key) - first;
            point = S[i] + (S[s.n_neg + first] - neg_heads);   // the negatives' heads and the positives-only heads below
        } else {
            const uint32_t j = static_cast<uint32_t>(e - s.n_neg);
            key = s.pos[j];
            neg = 0u;
            pos = key_bound<true>(s.pos, j, s.n_pos, key) - j;
            point = (S[e] - neg_heads) + S[key_bound<false>(s.neg, 0u, s.n_neg, key)];
        }
        if (point < count) {   // always true: a rank among the heads
            pt_key[point] = key;
            pt_pos[point] = pos;
            pt_neg[point] = neg;
        }
    }
}

// ---- 4. pooling ----------------------------------------------------------------------------------------------------------
struct Block {
    uint32_t start, pos, neg;   // the first point of the block, its positives and negatives
};

__device__ __forceinline__ bool pools(const Block &left, const Block &right)   // mean(left) >= mean(right)
{
    const uint64_t left_total = static_cast<uint64_t>(left.pos) + left.neg;
    const uint64_t right_total = static_cast<uint64_t>(right.pos) + right.neg;
    return static_cast<uint64_t>(left.pos) * right_total >= static_cast<uint64_t>(right.pos) * left_total;
}

// The stack algorithm in place over count blocks at start[at .. ), pos[...], neg[...] (LDS): the stack is the prefix of
// what has been read.  Returns the number of blocks left.
__device__ inline uint32_t pool_in_place(uint32_t *start, uint32_t *pos, uint32_t *neg, uint32_t at, uint32_t count)
{
    uint32_t depth = 0u;
    for (uint32_t t = 0; t < count; ++t) {
        Block current{start[at + t], pos[at + t], neg[at + t]};
        while (depth > 0u) {
            const Block top{start[at + depth - 1], pos[at + depth - 1], neg[at + depth - 1]};
            if (!pools(top, current)) break;
            current.start = top.start;
            current.pos += top.pos;
            current.neg += top.neg;
            --depth;
        }
        start[at + depth] = current.start;
        pos[at + depth] = current.pos;
        neg[at + depth] = current.neg;
        ++depth;
    }
    return depth;
}

// Level 1.  Dynamic LDS: six arrays of `capacity` = W + 128 words.  The slice of lane l holds per = ceil(W / 64) points
// at l * (per + 1): the odd word of padding keeps the 64 stacks off each other's banks when per is a power of two.
__global__ __launch_bounds__(64) void ds_isotonic_pool_kernel(const uint32_t *pt_pos, const uint32_t *pt_neg,
                                                               const uint32_t *state, int32_t W, uint32_t *sv_start,
                                                               uint32_t *sv_pos, uint32_t *sv_neg, uint32_t *seg_count)
{
    extern __shared__ uint32_t s_pool[];
    __shared__ uint32_t s_waves[1];
    const uint32_t capacity = static_cast<uint32_t>(W) + 128u;
    uint32_t *a_start = s_pool, *a_pos = a_start + capacity, *a_neg = a_pos + capacity;
    uint32_t *b_start = a_neg + capacity, *b_pos = b_start + capacity, *b_neg = b_pos + capacity;
    const uint32_t lane = threadIdx.x, per = (static_cast<uint32_t>(W) + 63u) / 64u, stride = per + 1u;
    const int64_t points = state[kStatePoints];
    const int64_t segments = (points + W - 1) / W;
    for (int64_t segment = blockIdx.x; segment < segments; segment += gridDim.x) {
        const int64_t base = segment * W;
        const uint32_t m = static_cast<uint32_t>(std::min<int64_t>(W, points - base));
        for (uint32_t t = lane; t < m; t += 64u) {   // coalesced in HBM
            const uint32_t at = (t / per) * stride + t % per;
            a_start[at] = t;
            a_pos[at] = pt_pos[base + t];
            a_neg[at] = pt_neg[base + t];
        }
        __syncthreads();
        const uint32_t first = lane * per;
        const uint32_t own = first < m ? std::min(per, m - first) : 0u;
        const uint32_t kept = pool_in_place(a_start, a_pos, a_neg, lane * stride, own);
        uint32_t total;
        const uint32_t before = block_exclusive<64>(kept, s_waves, total);
        for (uint32_t t = 0; t < kept; ++t) {
            b_start[before + t] = a_start[lane * stride + t];
            b_pos[before + t] = a_pos[lane * stride + t];
            b_neg[before + t] = a_neg[lane * stride + t];
        }
        __syncthreads();
        uint32_t left = 0u;
        if (lane == 0u) left = pool_in_place(b_start, b_pos, b_neg, 0u, total);
        left = __shfl(left, 0);
        __syncthreads();
        for (uint32_t t = lane; t < left; t += 64u) {
            sv_start[base + t] = static_cast<uint32_t>(base) + b_start[t];
            sv_pos[base + t] = b_pos[t];
            sv_neg[base + t] = b_neg[t];
        }
        if (lane == 0u) seg_count[segment] = left;
        __syncthreads();
    }
}

// Level 2, one workgroup.  A round stages the survivors of as many whole segments as LDS holds (at least one, 256 at the
// most: a prefix sum of their counts, then a copy balanced over the threads) and thread 0 pools them; the time of a round
// is a few dependent trips to HBM, so rounds are what to save.  A pop is a dependent read of the stack, so block i of
// the stack lives in LDS while i < kFinishStack and is written out at the end; a deeper one lies in sv_*[i] at once.  The
// depth never exceeds the survivors consumed, and those of the round in hand are in LDS, so a write to sv_*[depth]
// never lands on a slot still to be read.
__global__ __launch_bounds__(kCalibrateThreads) void ds_isotonic_finish_kernel(uint32_t *state, int32_t W,
                                                                                uint32_t *sv_start, uint32_t *sv_pos,
                                                                                uint32_t *sv_neg, const uint32_t *seg_count)
{
    __shared__ uint32_t s_start[kCalibrateSegmentMax], s_pos[kCalibrateSegmentMax], s_neg[kCalibrateSegmentMax];
    __shared__ uint32_t s_before[kCalibrateThreads], s_waves[kCalibrateWaves], s_take, s_total;
    __shared__ uint32_t k_start[kFinishStack], k_pos[kFinishStack], k_neg[kFinishStack];
    const int64_t points = state[kStatePoints];
    const int64_t segments = (points + W - 1) / W;
    uint32_t depth = 0u, survivors = 0u;
    Block top{0u, 0u, 0u};   // sv_*[depth - 1], kept in registers by thread 0
    for (int64_t segment = 0; segment < segments;) {   // uniform over the workgroup
        const int64_t mine = segment + threadIdx.x;
        const uint32_t m = mine < segments ? min(seg_count[mine], static_cast<uint32_t>(W)) : 0u;
        uint32_t unused;
        const uint32_t before = block_exclusive<kCalibrateThreads>(m, s_waves, unused);
        // the segments taken are a prefix: before + m never falls from one thread to the next
        const bool taken = mine < segments && before + m <= static_cast<uint32_t>(kCalibrateSegmentMax);
        if (threadIdx.x == 0) {
            s_take = 0u;
            s_total = 0u;
        }
        s_before[threadIdx.x] = before;
        __syncthreads();
        if (taken) {
            atomicAdd(&s_take, 1u);
            atomicAdd(&s_total, m);
        }
        __syncthreads();
        const uint32_t take = s_take, total = s_total;   // take >= 1: a segment holds at most W <= 2048 blocks
        for (uint32_t e = threadIdx.x; e < total; e += kCalibrateThreads) {
            uint32_t low = 0u, high = take;   // the last taken segment that starts at or before e
            while (high - low > 1u) {
                const uint32_t mid = (low + high) >> 1;
                if (s_before[mid] <= e) low = mid; else high = mid;
            }
            const int64_t at = (segment + low) * W + (e - s_before[low]);
            s_start[e] = sv_start[at];
            s_pos[e] = sv_pos[at];
            s_neg[e] = sv_neg[at];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            survivors += total;
            for (uint32_t t = 0; t < total; ++t) {
                Block current{s_start[t], s_pos[t], s_neg[t]};
                while (depth > 0u && pools(top, current)) {
                    current.start = top.start;
                    current.pos += top.pos;
                    current.neg += top.neg;
                    --depth;
                    if (depth > 0u) {
                        const uint32_t under = depth - 1u;
                        top = under < kFinishStack ? Block{k_start[under], k_pos[under], k_neg[under]}
                                                   : Block{sv_start[under], sv_pos[under], sv_neg[under]};
                    }
                }
                if (depth < kFinishStack) {
                    k_start[depth] = current.start;
                    k_pos[depth] = current.pos;
                    k_neg[depth] = current.neg;
                } else {
                    sv_start[depth] = current.start;
                    sv_pos[depth] = current.pos;
                    sv_neg[depth] = current.neg;
                }
                top = current;
                ++depth;
            }
        }
        segment += take;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        state[kStateBlocks] = depth;
        state[kStateSurvivors] = survivors;
        s_total = depth;
    }
    __syncthreads();   // every slot has been consumed: the part of the stack kept in LDS goes to its place
    const uint32_t kept = s_total < kFinishStack ? s_total : static_cast<uint32_t>(kFinishStack);
    for (uint32_t i = threadIdx.x; i < kept; i += kCalibrateThreads) {
        sv_start[i] = k_start[i];
        sv_pos[i] = k_pos[i];
        sv_neg[i] = k_neg[i];
    }
}

__global__ __launch_bounds__(kCalibrateThreads) void ds_isotonic_blocks_kernel(const uint32_t *state, const uint32_t *pt_key,
                                                                                const uint32_t *sv_start,
                                                                                const uint32_t *sv_pos, const uint32_t *sv_neg,
                                                                                float *lo, float *hi, long long *pos,
                                                                                long long *neg)
{
    const int64_t blocks = state[kStateBlocks];
    const uint32_t points = state[kStatePoints];
    for (int64_t k = blockIdx.x * static_cast<int64_t>(kCalibrateThreads) + threadIdx.x; k < blocks;
         k += static_cast<int64_t>(gridDim.x) * kCalibrateThreads) {
        const uint32_t first = sv_start[k], next = k + 1 < blocks ? sv_start[k + 1] : points;
        lo[k] = __uint_as_float(cut_value_bits(pt_key[first]));
        hi[k] = __uint_as_float(cut_value_bits(pt_key[next - 1]));
        pos[k] = sv_pos[k];
        neg[k] = sv_neg[k];
    }
}

// ---- the map ---------------------------------------------------------------------------------------------------------------
// out[i] = value of the last block whose lower edge is not above scores[i] in key order; 0 below the first edge, NaN for
// a NaN score and when there is no block.  kLds: the edges' keys are staged in LDS (dynamic, K words).
template <bool kLds>
__global__ __launch_bounds__(kCalibrateThreads) void ds_calibration_apply_kernel(const float *lo, const float *value,
                                                                                  int32_t K, const float *scores, int64_t n,
                                                                                  float *out)
{
    extern __shared__ uint32_t s_edges[];
    if (kLds) {
        for (int32_t k = threadIdx.x; k < K; k += kCalibrateThreads) s_edges[k] = cut_key(__float_as_uint(lo[k]));
        __syncthreads();
    }
    for (int64_t i = blockIdx.x * static_cast<int64_t>(kCalibrateThreads) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * kCalibrateThreads) {
        const uint32_t key = cut_key(__float_as_uint(scores[i]));
        float result = __uint_as_float(0x7fc00000u);
        if (key != kNanKey && K > 0) {
            int32_t low = 0, high = K;   // the number of edges not above the key
            while (low < high) {
                const int32_t mid = low + ((high - low) >> 1);
                const uint32_t edge = kLds ? s_edges[mid] : cut_key(__float_as_uint(lo[mid]));
                if (edge <= key) low = mid + 1; else high = mid;
            }
            result = low > 0 ? value[low - 1] : 0.f;
        }
        out[i] = result;
    }
}

// ---- reliability -----------------------------------------------------------------------------------------------------------
// counters[bin][4] = rows, positives, sum rint(p * 2^30), sum rint((p - y)^2 * 2^30); bin n_bins takes the rows whose p is
// a NaN or outside [0, 1] (rows and positives only).  Every wave adds into its own table in LDS (integer LDS atomics:
// the lanes of a wave share bins), then adds each of its non-zero counters once to HBM.
__global__ __launch_bounds__(kCalibrateThreads) void ds_reliability_kernel(const float *probabilities, const float *labels,
                                                                            int64_t n, int32_t n_bins,
                                                                            unsigned long long *out)
{
    __shared__ unsigned long long s_table[kCalibrateWaves][(kReliabilityBinsMax + 1) * 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int counters = (n_bins + 1) * 4;
    unsigned long long *mine = s_table[wave];
    for (int c = lane; c < counters; c += 64) mine[c] = 0ull;
    __syncthreads();
    for (int64_t i = blockIdx.x * static_cast<int64_t>(kCalibrateThreads) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * kCalibrateThreads) {
        const double p = probabilities[i];
        const bool positive = labels[i] != 0.f;
        if (!(p >= 0.0 && p <= 1.0)) {
            atomicAdd(&mine[n_bins * 4], 1ull);
            if (positive) atomicAdd(&mine[n_bins * 4 + 1], 1ull);
            continue;
        }
        const int bin = std::min(static_cast<int>(floor(p * n_bins)), n_bins - 1);
        const double miss = p - (positive ? 1.0 : 0.0);
        const double square = miss * miss;
        atomicAdd(&mine[bin * 4], 1ull);
        if (positive) atomicAdd(&mine[bin * 4 + 1], 1ull);
        atomicAdd(&mine[bin * 4 + 2], static_cast<unsigned long long>(rint(p * 1073741824.0)));
        atomicAdd(&mine[bin * 4 + 3], static_cast<unsigned long long>(rint(square * 1073741824.0)));
    }
    __syncthreads();
    for (int c = lane; c < counters; c += 64)
        if (mine[c]) atomicAdd(&out[c], mine[c]);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// the scalar checks of both twins; clears `out`
static int isotonic_check_scalars(const char *what, int64_t n, int64_t out[4])
{
    DS_REQUIRE(out != nullptr, "%s: null out", what);
    DS_REQUIRE(n >= 0 && n < kCalibrateRowsMax, "%s: n = %lld outside [0, 2^31)", what, (long long)n);
    for (int i = 0; i < 4; ++i) out[i] = 0;
    return DS_OK;
}

// What the body shares with its host-pointer twin: pointers to the caller's pointers into HBM, read once `scratch` is
// allocated (they are the caller's own arrays, or pieces that it has declared in `scratch`).
struct IsotonicArrays {
    const float *const *scores, *const *labels;
    float *const *lo, *const *hi;
    long long *const *pos, *const *neg;
};

static int isotonic_enqueue(const char *what, Scratch &scratch, const IsotonicArrays &at, int64_t n, int64_t out[4],
                            hipStream_t stream)
{
    const int32_t W = static_cast<int32_t>(g_calibrate_segment_points.get());
    const int64_t head_tiles = (n + 1 + kCalibrateHeadTile - 1) / kCalibrateHeadTile;
    const int64_t max_segments = (n + W - 1) / W;
    uint32_t *keys_a = nullptr, *keys_b = nullptr, *table = nullptr, *state = nullptr, *S = nullptr, *totals = nullptr,
             *pt_key = nullptr, *pt_pos = nullptr, *pt_neg = nullptr, *seg_count = nullptr;
    scratch.add(&keys_a, static_cast<size_t>(2 * n));   // two sort buffers of 2 n keys
    scratch.add(&keys_b, static_cast<size_t>(2 * n));
    scratch.add(&table, static_cast<size_t>(2 * 256 * radix_tiles(n)));
    scratch.add(&state, kStateWords);
    scratch.add(&S, static_cast<size_t>(n + 1));
    scratch.add(&totals, static_cast<size_t>(head_tiles));
    scratch.add(&pt_key, static_cast<size_t>(n));
    scratch.add(&pt_pos, static_cast<size_t>(n));
    scratch.add(&pt_neg, static_cast<size_t>(n));
    scratch.add(&seg_count, static_cast<size_t>(max_segments));
    DS_TRY(scratch.allocate(what));
    const float *d_scores = *at.scores, *d_labels = *at.labels;
    float *d_lo = *at.lo, *d_hi = *at.hi;
    long long *d_pos = *at.pos, *d_neg = *at.neg;

    uint32_t host_state[kStateWords] = {};
    auto enqueue = [&]() -> int {
        DS_LAUNCH(ds_isotonic_begin_kernel, dim3(1), dim3(64), 0, stream, state);
        DS_HIP(hipMemsetAsync(keys_a, 0xff, sizeof(uint32_t) * 2 * n, stream));   // the padding key
        const dim3 threads(kCalibrateThreads);
        const unsigned row_grid = calibrate_grid((n + kCalibrateThreads - 1) / kCalibrateThreads);
        const int64_t split_rows = static_cast<int64_t>(kCalibrateWaves) * kSplitWaveRows;
        DS_LAUNCH(ds_isotonic_split_kernel, dim3(calibrate_grid((n + split_rows - 1) / split_rows)), threads, 0, stream, d_scores, d_labels, n, keys_a,
                  state);
        DS_TRY(radix_sort_columns(stream, keys_a, keys_b, n, 2, state + kStateOr,
                                  state + kStateAnd, table));
        DS_LAUNCH(ds_isotonic_heads_kernel, dim3(calibrate_grid(head_tiles)), threads, 0, stream, keys_a,
                  keys_b, n, state, S, totals, head_tiles);
        DS_LAUNCH(ds_isotonic_tile_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, totals, head_tiles,
                  state);
        DS_LAUNCH(ds_isotonic_scan_kernel, dim3(calibrate_grid(head_tiles)), threads, 0, stream, state, S,
                  totals, head_tiles);
        DS_LAUNCH(ds_isotonic_points_kernel, dim3(row_grid), threads, 0, stream, keys_a, keys_b, n,
                  state, S, pt_key, pt_pos, pt_neg);
        // the sorted keys are spent: the sort buffers hold the survivors from here on
        uint32_t *sv_start = keys_a, *sv_pos = keys_a + n, *sv_neg = keys_b;
        const size_t lds = sizeof(uint32_t) * 6 * (static_cast<size_t>(W) + 128);
        DS_TRY(ds::allow_dynamic_lds(ds_isotonic_pool_kernel, lds));
        DS_LAUNCH(ds_isotonic_pool_kernel, dim3(calibrate_grid(max_segments)), dim3(64), lds, stream, pt_pos,
                  pt_neg, state, W, sv_start, sv_pos, sv_neg, seg_count);
        DS_LAUNCH(ds_isotonic_finish_kernel, dim3(1), threads, 0, stream, state, W, sv_start, sv_pos, sv_neg,
                  seg_count);
        DS_LAUNCH(ds_isotonic_blocks_kernel, dim3(row_grid), threads, 0, stream, state, pt_key, sv_start,
                  sv_pos, sv_neg, d_lo, d_hi, d_pos, d_neg);
        DS_HIP(hipMemcpyAsync(host_state, state, sizeof(host_state), hipMemcpyDeviceToHost, stream));
        return DS_OK;
    };
    const int status = enqueue();
    const hipError_t synced = hipStreamSynchronize(stream);   // the scratch is freed on return
    if (status != DS_OK) return status;
    DS_HIP(synced);
    out[0] = host_state[kStateBlocks];
    out[1] = host_state[kStateNan];
    out[2] = host_state[kStatePoints];
    out[3] = host_state[kStateSurvivors];
    return DS_OK;
}

}  // namespace ds

extern "C" {

int ds_calibrate_option(const char *name, int64_t value)
{
    return ds::set_option("ds_calibrate_option", ds::g_calibrate_options, name, value);
}

int ds_isotonic_fit_device(const float *d_scores, const float *d_labels, int64_t n, float *d_lo, float *d_hi,
                           long long *d_pos, long long *d_neg, int64_t out[4], void *stream)
{
    const char *what = "ds_isotonic_fit_device";
    DS_TRY(ds::isotonic_check_scalars(what, n, out));
    if (n == 0) {
        DS_HIP(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
        return DS_OK;
    }
    DS_REQUIRE(d_scores && d_labels && d_lo && d_hi && d_pos && d_neg, "%s: null pointer", what);
    ds::Scratch scratch;
    return ds::isotonic_enqueue(what, scratch, {&d_scores, &d_labels, &d_lo, &d_hi, &d_pos, &d_neg}, n, out,
                                static_cast<hipStream_t>(stream));
}

int ds_isotonic_fit(const float *scores, const float *labels, int64_t n, float *lo, float *hi, long long *pos,
                    long long *neg, int64_t out[4], int device)
{
    const char *what = "ds_isotonic_fit";
    DS_TRY(ds::isotonic_check_scalars(what, n, out));
    if (n == 0) return DS_OK;
    DS_REQUIRE(scores && labels && lo && hi && pos && neg, "%s: null pointer", what);
    DS_HIP(hipSetDevice(device));
    ds::Scratch scratch;
    const float *d_scores = nullptr, *d_labels = nullptr;
    float *d_lo = nullptr, *d_hi = nullptr;
    long long *d_pos = nullptr, *d_neg = nullptr;
    scratch.stage(&d_scores, scores, static_cast<size_t>(n));
    scratch.stage(&d_labels, labels, static_cast<size_t>(n));
    scratch.add(&d_lo, static_cast<size_t>(n));
    scratch.add(&d_hi, static_cast<size_t>(n));
    scratch.add(&d_pos, static_cast<size_t>(n));
    scratch.add(&d_neg, static_cast<size_t>(n));
    DS_TRY(ds::isotonic_enqueue(what, scratch, {&d_scores, &d_labels, &d_lo, &d_hi, &d_pos, &d_neg}, n, out, nullptr));
    const size_t K = static_cast<size_t>(out[0]);
    if (K) {
        DS_HIP(hipMemcpy(lo, d_lo, K * sizeof(float), hipMemcpyDeviceToHost));
        DS_HIP(hipMemcpy(hi, d_hi, K * sizeof(float), hipMemcpyDeviceToHost));
        DS_HIP(hipMemcpy(pos, d_pos, K * sizeof(long long), hipMemcpyDeviceToHost));
        DS_HIP(hipMemcpy(neg, d_neg, K * sizeof(long long), hipMemcpyDeviceToHost));
    }
    return DS_OK;
}

int ds_calibration_apply_device(const float *d_lo, const float *d_value, int32_t K, const float *d_scores, int64_t n,
                                float *d_out, void *stream)
{
    const char *what = "ds_calibration_apply_device";
    DS_REQUIRE(K >= 0, "%s: K = %d is negative", what, K);
    DS_REQUIRE(n >= 0 && n < ds::kCalibrateRowsMax, "%s: n = %lld outside [0, 2^31)", what, (long long)n);
    if (n == 0) return DS_OK;
    DS_REQUIRE(d_scores && d_out && (K == 0 || (d_lo && d_value)), "%s: null pointer", what);
    const dim3 grid(ds::calibrate_grid((n + ds::kCalibrateThreads - 1) / ds::kCalibrateThreads));
    hipStream_t queue = static_cast<hipStream_t>(stream);
    if (K <= ds::kCalibrateEdgesInLds) {
        const size_t lds = sizeof(uint32_t) * static_cast<size_t>(K);
        DS_TRY(ds::allow_dynamic_lds(ds::ds_calibration_apply_kernel<true>, lds));
        DS_LAUNCH(ds::ds_calibration_apply_kernel<true>, grid, dim3(ds::kCalibrateThreads), lds, queue, d_lo,
                  d_value, K, d_scores, n, d_out);
    } else {
        DS_LAUNCH(ds::ds_calibration_apply_kernel<false>, grid, dim3(ds::kCalibrateThreads), 0, queue, d_lo,
                  d_value, K, d_scores, n, d_out);
    }
    return DS_OK;
}

int ds_reliability_device(const float *d_probabilities, const float *d_labels, int64_t n, int32_t n_bins, long long *d_out,
                          void *stream)
{
    const char *what = "ds_reliability_device";
    DS_REQUIRE(n_bins >= 1 && n_bins <= ds::kReliabilityBinsMax, "%s: n_bins = %d outside [1, %d]", what, n_bins,
               ds::kReliabilityBinsMax);
    DS_REQUIRE(n >= 0 && n < ds::kCalibrateRowsMax, "%s: n = %lld outside [0, 2^31)", what, (long long)n);
    DS_REQUIRE(d_out != nullptr && (n == 0 || (d_probabilities && d_labels)), "%s: null pointer", what);
    hipStream_t queue = static_cast<hipStream_t>(stream);
    DS_HIP(hipMemsetAsync(d_out, 0, sizeof(long long) * 4 * (static_cast<size_t>(n_bins) + 1), queue));
    if (n == 0) return DS_OK;
    DS_LAUNCH(ds::ds_reliability_kernel, dim3(ds::calibrate_grid((n + ds::kCalibrateThreads - 1) / ds::kCalibrateThreads)),
              dim3(ds::kCalibrateThreads), 0, queue, d_probabilities, d_labels, n, n_bins,
              reinterpret_cast<unsigned long long *>(d_out));
    return DS_OK;
}

}  // extern "C"
