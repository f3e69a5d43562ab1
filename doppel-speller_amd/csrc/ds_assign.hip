// One-to-one matches ("One-to-one matches"): Q ranked lists of n slots, as ds_rank_matches_device writes
// them, turned into one matching in which a truth row is given to one title at most.
//
// Edges.  Slot s of title q (absolute number: q_first + the chunk's local row) is an edge to t = row[q][s] when
//   0 <= t < n_truth;
//   stage 1 (exact) or 2 (close); or stage 3 with probability > probability_threshold (float32; a NaN is not above) and the
//   probability's sign bit clear;
//   no earlier slot of the title is an edge to t -- which is: no earlier slot passes the two tests above with the same row,
//   since the first slot that passes them for a row is always an edge.
// Its key, uint64, 0 = no edge:  class << 62 | payload << 31 | (2^31 - 1 - q)
//   class 3 / 2 / 1 for stage 1 / 2 / 3; payload 0 / the ratio / the float32 bits of the probability (below 2^31).
// A larger key is a better claim: exact over close over model, the higher score inside a class, the earlier title on equal
// scores.  The keys at one truth row come from different titles: they are distinct.
//
// Matching: deferred acceptance, the titles proposing in slot order, a truth row keeping the largest key it was offered.
//   held[n_truth]  uint64, starts at 0 and only grows (64-bit atomicMax);
//   next[Q]        the slot title q stands at (n: exhausted).
// A round, one lane per title: a title whose held[row[q][next]] == key[q][next] is held and idle, an exhausted title is idle;
// any other walks forward from `next`, skipping non-edges and rows that already hold more than its key (a plain load: held
// only grows, so a stale value that is above the key is above it for good), and offers its key with atomicMax elsewhere.  It
// stops where the value returned is below its key, and writes `next`.  A title turned away from t would be turned away at any
// later time as well: it never returns, and whatever the interleaving the fixed point is the title-optimal stable matching
// (McVitie-Wilson: the order of the proposals does not matter).  A round is one launch: its loads see everything the rounds
// before it wrote, so a round in which no title was active is a fixed point, not a stale view of one.  Every active title
// raises a held entry or moves its `next`: the rounds end.
//
// Activity and proposals are counted per wave (a ballot and a popcount per pass, one atomic per wave and launch).  The host
// enqueues "rounds_per_sync" rounds, each with its own activity counter, and reads the counters back once per batch; a round
// that finds the counter of the round before it at zero returns at once.
#include <algorithm>
#include <cmath>

#include "ds_launch.h"
#include "ds_options.h"
#include "ds_wave.h"

namespace ds {

constexpr int kAssignThreads = 256;
constexpr int kAssignMaxBlocks = 2048;        // 8 workgroups per CU on 256 CUs; more items: the grid strides
constexpr int kAssignBlocksLimit = 1 << 20;
constexpr int kAssignRoundsPerSync = 8;
constexpr int kAssignRoundsLimit = 1024;
constexpr uint64_t kAssignTitleMask = 0x7fffffffull;

static Option g_assign_max_blocks{"max_blocks", 0, kAssignBlocksLimit, kAssignMaxBlocks, true};
static Option g_assign_rounds_per_sync{"rounds_per_sync", 1, kAssignRoundsLimit, kAssignRoundsPerSync};
static Option *const g_assign_options[] = {&g_assign_max_blocks, &g_assign_rounds_per_sync};

// does slot i pass the tests that need no other slot?
__device__ __forceinline__ bool assign_eligible(int32_t row, float probability, int32_t stage, int32_t n_truth, float threshold)
{
    if (row < 0 || row >= n_truth) return false;
    if (stage == 1 || stage == 2) return true;
    return stage == 3 && probability > threshold && (__float_as_uint(probability) >> 31) == 0;
}

struct EdgeArgs {
    const int32_t *row;           // [n_queries][n], the chunk's
    const float *probability;
    const uint8_t *ratio;
    const int8_t *stage;
    uint64_t *edge_key;           // [n_total][n], the whole call's
    int32_t *edge_row;
    int64_t q_first, n_slots;
    int32_t n, n_truth;
    float threshold;
};

// one thread per slot, flat over the chunk's n_queries * n slots
__global__ __launch_bounds__(kAssignThreads) void ds_assign_edges_kernel(EdgeArgs a)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kAssignThreads + threadIdx.x; i < a.n_slots;
         i += static_cast<int64_t>(gridDim.x) * kAssignThreads) {
        const int64_t q = i / a.n;
        const int32_t s = static_cast<int32_t>(i - q * a.n);
        const int32_t row = a.row[i];
        const int32_t stage = a.stage[i];
        const float probability = a.probability[i];
        bool edge = assign_eligible(row, probability, stage, a.n_truth, a.threshold);
        for (int64_t j = i - s; edge && j < i; ++j)
            edge = !(a.row[j] == row && assign_eligible(row, a.probability[j], a.stage[j], a.n_truth, a.threshold));
        uint64_t key = 0;
        if (edge) {
            const uint64_t klass = stage == 1 ? 3 : stage == 2 ? 2 : 1;
            const uint64_t payload =
                stage == 1 ? 0u : stage == 2 ? static_cast<uint32_t>(a.ratio[i]) : __float_as_uint(probability);
            key = (klass << 62) | (payload << 31) | (kAssignTitleMask - static_cast<uint64_t>(a.q_first + q));
        }
        const int64_t out = a.q_first * a.n + i;
        a.edge_key[out] = key;
        a.edge_row[out] = row;
    }
}

__device__ __forceinline__ uint64_t held_load(const unsigned long long *held, int32_t t)
{
    return __hip_atomic_load(held + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One round.  activity[0] is this round's counter, `before` the counter of the round before it in the same batch (NULL for the
// first of a batch); proposals: the atomics that raised a held entry, added up over the rounds.
__global__ __launch_bounds__(kAssignThreads) void ds_assign_round_kernel(
    const int32_t *__restrict__ edge_row, const uint64_t *__restrict__ edge_key, int64_t n_queries, int32_t n, int32_t n_truth,
    unsigned long long *held, int32_t *__restrict__ next, const uint32_t *before, uint32_t *activity,
    unsigned long long *proposals)
{
    if (before != nullptr && *before == 0) return;
    uint32_t n_active = 0, n_raised = 0;          // the same in every lane of a wave
    // every lane of a wave makes the same number of passes (the ballots below); a pass past the end does nothing
    for (int64_t base = (static_cast<int64_t>(blockIdx.x) * kAssignThreads + threadIdx.x) & ~int64_t(63); base < n_queries;
         base += static_cast<int64_t>(gridDim.x) * kAssignThreads) {
        const int64_t q = base + (threadIdx.x & 63);
        bool active = false, raised = false;
        if (q < n_queries) {
            const int64_t slots = q * n;
            int32_t s = next[q];
            if (s >= 0 && s < n) {
                const uint64_t mine = edge_key[slots + s];
                const int32_t at = edge_row[slots + s];
                active = !(mine != 0 && at >= 0 && at < n_truth && held_load(held, at) == mine);
            }
            if (active) {
                for (; s < n; ++s) {
                    const uint64_t key = edge_key[slots + s];
                    const int32_t t = edge_row[slots + s];
                    if (key == 0 || t < 0 || t >= n_truth) continue;
                    if (held_load(held, t) > key) continue;               // turned away without an atomic
                    const uint64_t seen = atomicMax(held + t, static_cast<unsigned long long>(key));
                    if (seen < key) {
                        raised = true;
                        break;
                    }
                    if (seen == key) break;                                 // it holds t already (keys at a row are distinct)
                }
                next[q] = s;
            }
        }
        n_active += __popcll(__ballot(active));
        n_raised += __popcll(__ballot(raised));
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_active) atomicAdd(activity, n_active);
        if (n_raised) atomicAdd(proposals, static_cast<unsigned long long>(n_raised));
    }
}

// the outputs of every title and counts[0..4); counts[5] = rounds.  At the fixed point a title that is not exhausted holds
// the row of the slot it stands at.
__global__ __launch_bounds__(kAssignThreads) void ds_assign_finish_kernel(
    const int32_t *__restrict__ edge_row, const uint64_t *__restrict__ edge_key, int64_t n_queries, int32_t n, int32_t n_truth,
    const int32_t *__restrict__ next, int32_t *__restrict__ match_row, int32_t *__restrict__ match_slot,
    int32_t *__restrict__ first_row, unsigned long long *counts, long long rounds)
{
    unsigned long long n_edges = 0;                        // per lane: summed over the wave at the end
    uint32_t n_matched = 0, n_displaced = 0, n_left = 0;   // the same in every lane of a wave
    for (int64_t base = (static_cast<int64_t>(blockIdx.x) * kAssignThreads + threadIdx.x) & ~int64_t(63); base < n_queries;
         base += static_cast<int64_t>(gridDim.x) * kAssignThreads) {
        const int64_t q = base + (threadIdx.x & 63);
        bool matched = false, displaced = false;
        if (q < n_queries) {
            const int64_t slots = q * n;
            int32_t first = -1;
            for (int32_t s = 0; s < n; ++s) {
                const int32_t t = edge_row[slots + s];
                if (edge_key[slots + s] == 0 || t < 0 || t >= n_truth) continue;
                ++n_edges;
                if (first < 0) first = t;
            }
            const int32_t s = next[q];
            matched = s >= 0 && s < n;
            const int32_t mine = matched ? edge_row[slots + s] : -1;
            match_row[q] = mine;
            match_slot[q] = matched ? s : -1;
            first_row[q] = first;
            displaced = first >= 0 && mine != first;
        }
        n_matched += __popcll(__ballot(matched));
        n_displaced += __popcll(__ballot(displaced));
        n_left += __popcll(__ballot(displaced && !matched));
    }
    n_edges = wave_sum(n_edges);
    if ((threadIdx.x & 63) == 0) {
        if (n_edges) atomicAdd(counts + 0, n_edges);
        if (n_matched) atomicAdd(counts + 1, static_cast<unsigned long long>(n_matched));
        if (n_displaced) atomicAdd(counts + 2, static_cast<unsigned long long>(n_displaced));
        if (n_left) atomicAdd(counts + 3, static_cast<unsigned long long>(n_left));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[5] = static_cast<unsigned long long>(rounds);
}

static dim3 assign_grid(int64_t items)
{
    const int64_t blocks = (items + kAssignThreads - 1) / kAssignThreads;
    return dim3(grid_cap(blocks, g_assign_max_blocks.get()));
}

}  // namespace ds

extern "C" {

int ds_assign_option(const char *name, int64_t value)
{
    return ds::set_option("ds_assign_option", ds::g_assign_options, name, value);
}

int ds_assign_edges_device(const int32_t *d_row, const float *d_probability, const uint8_t *d_ratio, const int8_t *d_stage,
                           int64_t q_first, int64_t n_queries, int64_t n_total, int32_t n, int64_t n_truth,
                           float probability_threshold, uint64_t *d_edge_key, int32_t *d_edge_row, void *stream)
{
    DS_REQUIRE(n_queries >= 0 && q_first >= 0 && n_total >= 0, "ds_assign_edges_device: negative count");
    DS_REQUIRE(n_total <= INT32_MAX, "ds_assign_edges_device: %lld titles, must be below 2^31", (long long)n_total);
    DS_REQUIRE(n_truth >= 0 && n_truth <= INT32_MAX, "ds_assign_edges_device: n_truth = %lld out of range [0, 2^31)",
               (long long)n_truth);
    DS_REQUIRE(n >= 1, "ds_assign_edges_device: n = %d, must be positive", n);
    DS_REQUIRE(std::isfinite(probability_threshold), "ds_assign_edges_device: the probability threshold is not finite");
    DS_REQUIRE(d_row && d_probability && d_ratio && d_stage && d_edge_key && d_edge_row, "ds_assign_edges_device: null pointer");
    DS_REQUIRE(q_first <= n_total && n_queries <= n_total - q_first,
               "ds_assign_edges_device: titles [%lld, %lld) are not among the %lld of the call", (long long)q_first,
               (long long)(q_first + n_queries), (long long)n_total);
    if (n_queries == 0) return DS_OK;
    ds::EdgeArgs args{};
    args.row = d_row; args.probability = d_probability; args.ratio = d_ratio; args.stage = d_stage;
    args.edge_key = d_edge_key; args.edge_row = d_edge_row;
    args.q_first = q_first; args.n_slots = n_queries * n; args.n = n; args.n_truth = static_cast<int32_t>(n_truth);
    args.threshold = probability_threshold;
    DS_LAUNCH(ds::ds_assign_edges_kernel, ds::assign_grid(args.n_slots), dim3(ds::kAssignThreads), 0,
              static_cast<hipStream_t>(stream), args);
    return DS_OK;
}

int ds_assign_solve_device(const int32_t *d_edge_row, const uint64_t *d_edge_key, int64_t n_queries, int32_t n, int64_t n_truth,
                           uint64_t *d_held, int32_t *d_next, int32_t *d_match_row, int32_t *d_match_slot,
                           int32_t *d_first_row, int64_t *d_counts, void *stream)
{
    DS_REQUIRE(n_queries >= 0, "ds_assign_solve_device: negative count");
    DS_REQUIRE(n_queries <= INT32_MAX, "ds_assign_solve_device: %lld titles, must be below 2^31", (long long)n_queries);
    DS_REQUIRE(n_truth >= 0 && n_truth <= INT32_MAX, "ds_assign_solve_device: n_truth = %lld out of range [0, 2^31)",
               (long long)n_truth);
    DS_REQUIRE(n >= 1, "ds_assign_solve_device: n = %d, must be positive", n);
    DS_REQUIRE(d_edge_row && d_edge_key && d_held && d_next && d_match_row && d_match_slot && d_first_row && d_counts,
               "ds_assign_solve_device: null pointer");
    hipStream_t queue = static_cast<hipStream_t>(stream);
    DS_HIP(hipMemsetAsync(d_counts, 0, 6 * sizeof(int64_t), queue));
    if (n_queries == 0) {
        DS_HIP(hipStreamSynchronize(queue));
        return DS_OK;
    }
    if (n_truth) DS_HIP(hipMemsetAsync(d_held, 0, static_cast<size_t>(n_truth) * sizeof(uint64_t), queue));
    DS_HIP(hipMemsetAsync(d_next, 0, static_cast<size_t>(n_queries) * sizeof(int32_t), queue));

    const int batch = static_cast<int>(ds::g_assign_rounds_per_sync.get());
    ds::DeviceBuffer<uint32_t> activity;
    DS_TRY(activity.allocate(static_cast<size_t>(batch)));
    std::vector<uint32_t> seen(static_cast<size_t>(batch));
    const dim3 grid = ds::assign_grid(n_queries), block(ds::kAssignThreads);
    unsigned long long *held = reinterpret_cast<unsigned long long *>(d_held);
    unsigned long long *counts = reinterpret_cast<unsigned long long *>(d_counts);
    const int32_t truth = static_cast<int32_t>(n_truth);
    long long rounds = 0;                 // the rounds in which a title was active
    for (bool settled = false; !settled;) {
        DS_HIP(hipMemsetAsync(activity.ptr, 0, activity.bytes(), queue));
        for (int r = 0; r < batch; ++r) {
            DS_LAUNCH(ds::ds_assign_round_kernel, grid, block, 0, queue, d_edge_row, d_edge_key, n_queries, n, truth,
                      held, d_next, r ? activity.ptr + r - 1 : nullptr, activity.ptr + r, counts + 4);
        }
        DS_HIP(hipMemcpyAsync(seen.data(), activity.ptr, activity.bytes(), hipMemcpyDeviceToHost, queue));
        DS_HIP(hipStreamSynchronize(queue));
        for (int r = 0; r < batch && !settled; ++r) {
            if (seen[static_cast<size_t>(r)] == 0) settled = true;
            else ++rounds;
        }
    }
    DS_LAUNCH(ds::ds_assign_finish_kernel, grid, block, 0, queue, d_edge_row, d_edge_key, n_queries, n, truth, d_next,
              d_match_row, d_match_slot, d_first_row, counts, rounds);
    DS_HIP(hipStreamSynchronize(queue));
    return DS_OK;
}

}  // extern "C"
