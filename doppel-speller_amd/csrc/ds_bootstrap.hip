// Is a difference real ("Is a difference real: the paired bootstrap"): the outcome counts of M
// prediction sets over the same rows, resampled B times by UNIT (a train title, a fold group; by row without units).
//
//   codes[m][i] in {0, 1, 2, 3}   the outcome class of row i under set m
//   T[u][m][c]                    the rows of unit u with class c under set m (the unit table)
//   j(b, k) = umulhi64(x, U)      x = the first kept output of the stream of (seed, DS_BOOTSTRAP_PURPOSE_DRAW, (b << 32) | k)
//   counts[b][m][c] = sum over k < U of T[j(b, k)][m][c]
//
// Two kernels.  ds_bootstrap_check_kernel refuses a code above 3 or a unit outside [0, U) and, with units, builds T as
// uint32[U][M][4] by integer atomics.  Without units the table is the codes themselves and is not built.
//
// ds_bootstrap_kernel: one WAVE per (replicate, chunk of kBootstrapChunk draws); lane l takes the draws l, l + 64, ...
// of the chunk.  A workgroup stages the table in LDS once (when it fits; it reads HBM / L2 otherwise) and its waves run
// the replicates of its group over it, so the random gather of a draw is an LDS read.  A lane keeps its own partial
// counters for a tile of kBootstrapTile sets and the draws are generated again for every tile: a draw is some twenty
// integer instructions, its counters would be registers or LDS traffic.  With a unit table the partials are four uint64
// per set (an entry is below 2^32 and a chunk has 256 draws per lane).  Without one a draw adds 1 to one class, and the
// four classes share one uint64 as 16-bit fields: a lane adds at most 256 and the wave's sum over a chunk is at most
// kBootstrapChunk = 2^14, so no field carries into the next.  The partials are summed over the wave (ds_wave.h) and one
// lane adds each non-zero counter to the int64 output: one integer atomic per counter and wave.  Replicate B of the grid
// draws j = k: it is the baseline.  Integer sums throughout, so no bit depends on the grid, the chunking or the order.
#include "ds_launch.h"
#include "ds_bootstrap_draw.h"
#include "ds_train.h"
#include "ds_wave.h"

#include <algorithm>
#include <cmath>

namespace ds {

constexpr int kBootstrapThreads = 256;
constexpr int kBootstrapWaves = kBootstrapThreads / 64;
constexpr int kBootstrapTile = 4;                      // sets whose partial counters a lane holds at a time
constexpr int64_t kBootstrapChunk = 1 << 14;           // draws of one wave pass: 256 per lane
constexpr int64_t kBootstrapLdsBytes = 128 * 1024;     // the largest table staged (a CU has 160 KiB)
constexpr int kBootstrapSetsMax = 64;
constexpr int kBootstrapBootMax = 1 << 16;
constexpr int64_t kBootstrapRowsMax = int64_t(1) << 31;
constexpr int kBootstrapDefaultBlocks = 4096;          // default cap of either grid dimension
constexpr int kBootstrapTargetBlocks = 1024;           // replicate groups the default split aims at
constexpr int kBootstrapCheckThreads = 256;

static_assert(kBootstrapChunk / 64 * 64 == kBootstrapChunk && kBootstrapChunk < (1 << 16),
              "the wave's sum of a 16-bit field over a chunk must stay below 2^16");

// for tests (ds_bootstrap_option); no result depends on them
static Option g_bootstrap_max_blocks{"max_blocks", 0, 65535, kBootstrapDefaultBlocks, true};
static Option g_bootstrap_replicates_per_block{"replicates_per_block", 0, kBootstrapBootMax + 1, 0};   // 0: the launcher's choice
static Option g_bootstrap_table_in_lds{"table_in_lds", 0, 1, 1};
static Option *const g_bootstrap_options[] = {&g_bootstrap_max_blocks, &g_bootstrap_replicates_per_block,
                                              &g_bootstrap_table_in_lds};

struct BootstrapArgs {
    const uint8_t *codes;        // [M][n]
    const uint4 *table;          // [U][M], null without units
    unsigned long long *counts;  // [B][M][4]
    unsigned long long *baseline;  // [M][4]
    uint64_t seed;
    int64_t n_units;             // U
    int64_t n_chunks;
    int32_t n_sets, n_boot, per_block, n_groups;
    int32_t padded_sets;         // M rounded up to the tile: the stride of a staged row of codes
};

// ---- check, and the unit table ----------------------------------------------------------------------------------------
// One thread per row.  errors[0] counts the codes above 3, errors[1] the units outside [0, U), in 64 bits: n * M reaches
// 2^37, and a 32-bit count could wrap to 0 and pass.  A row with either adds nothing to the table (the caller refuses
// the call).
__global__ __launch_bounds__(kBootstrapCheckThreads) void ds_bootstrap_check_kernel(
    const uint8_t *codes, const int32_t *unit, int64_t n, int32_t n_sets, int64_t n_units, uint32_t *table,
    unsigned long long *errors)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBootstrapCheckThreads + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * kBootstrapCheckThreads) {
        int64_t u = i;
        if (unit != nullptr) {
            u = unit[i];
            if (u < 0 || u >= n_units) {
                atomicAdd(&errors[1], 1ull);
                u = -1;
            }
        }
        for (int32_t m = 0; m < n_sets; ++m) {
            const uint32_t code = codes[static_cast<int64_t>(m) * n + i];
            if (code > 3u)
                atomicAdd(&errors[0], 1ull);
            else if (table != nullptr && u >= 0)
                atomicAdd(&table[(u * n_sets + m) * 4 + code], 1u);
        }
    }
}

// ---- the resampling ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t bootstrap_draw(const BootstrapArgs &a, int32_t b, int64_t k)
{
    return bootstrap_unit(a.seed, b, a.n_boot, k, a.n_units);   // replicate n_boot is the baseline: every unit once
}

__device__ __forceinline__ void bootstrap_add(unsigned long long *out, unsigned long long value)
{
    if (value) atomicAdd(out, value);
}

// kUnits: the table is T (uint4 per unit and set), else the codes.  kLds: the table is staged in LDS.
template <bool kUnits, bool kLds>
__global__ __launch_bounds__(kBootstrapThreads) void ds_bootstrap_kernel(BootstrapArgs a)
{
    extern __shared__ uint4 staged_table[];   // kUnits: uint4[U][M]; else uint8[U][padded_sets] (16-byte aligned)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t M = a.n_sets, stride = a.padded_sets;
    const int64_t U = a.n_units;
    if (kLds) {
        if (kUnits) {
            for (int64_t e = threadIdx.x; e < U * M; e += kBootstrapThreads) staged_table[e] = a.table[e];
        } else {
            uint8_t *bytes = reinterpret_cast<uint8_t *>(staged_table);
            for (int32_t m = 0; m < stride; ++m)   // coalesced over the rows; the sets beyond M read as class 0
                for (int64_t u = threadIdx.x; u < U; u += kBootstrapThreads)
                    bytes[u * stride + m] = m < M ? a.codes[static_cast<int64_t>(m) * U + u] : uint8_t(0);
        }
        __syncthreads();
    }
    const uint32_t *staged_words = reinterpret_cast<const uint32_t *>(staged_table);
    for (int32_t group = blockIdx.x; group < a.n_groups; group += gridDim.x) {
        const int32_t begin = group * a.per_block;
        const int32_t end = begin + a.per_block < a.n_boot + 1 ? begin + a.per_block : a.n_boot + 1;
        for (int32_t b = begin + wave; b < end; b += kBootstrapWaves) {   // wave-uniform from here on: no barrier below
            unsigned long long *out = b == a.n_boot ? a.baseline : a.counts + static_cast<int64_t>(b) * M * 4;
            for (int64_t chunk = blockIdx.y; chunk < a.n_chunks; chunk += gridDim.y) {
                const int64_t first = chunk * kBootstrapChunk;
                const int64_t last = first + kBootstrapChunk < U ? first + kBootstrapChunk : U;
                for (int32_t m0 = 0; m0 < M; m0 += kBootstrapTile) {
                    if (kUnits) {
                        unsigned long long sum[kBootstrapTile][4] = {};
                        for (int64_t k = first + lane; k < last; k += 64) {
                            const int64_t j = bootstrap_draw(a, b, k);
#pragma unroll
                            for (int t = 0; t < kBootstrapTile; ++t) {
                                if (m0 + t < M) {
                                    const uint4 entry = kLds ? staged_table[j * M + m0 + t] : a.table[j * M + m0 + t];
                                    sum[t][0] += entry.x;
                                    sum[t][1] += entry.y;
                                    sum[t][2] += entry.z;
                                    sum[t][3] += entry.w;
                                }
                            }
                        }
#pragma unroll
                        for (int t = 0; t < kBootstrapTile; ++t) {
                            if (m0 + t >= M) break;   // wave-uniform
#pragma unroll
                            for (int c = 0; c < 4; ++c) {
                                const unsigned long long total = wave_sum(sum[t][c]);
                                if (lane == 0) bootstrap_add(out + (m0 + t) * 4 + c, total);
                            }
                        }
                    } else {
                        unsigned long long packed[kBootstrapTile] = {};   // four 16-bit fields, one per class
                        for (int64_t k = first + lane; k < last; k += 64) {
                            const int64_t j = bootstrap_draw(a, b, k);
                            if (kLds) {
                                const uint32_t word = staged_words[(j * stride + m0) >> 2];   // the tile's four codes
#pragma unroll
                                for (int t = 0; t < kBootstrapTile; ++t)
                                    packed[t] += 1ull << (((word >> (8 * t)) & 3u) * 16u);
                            } else {
#pragma unroll
                                for (int t = 0; t < kBootstrapTile; ++t)
                                    if (m0 + t < M)
                                        packed[t] += 1ull << ((a.codes[static_cast<int64_t>(m0 + t) * U + j] & 3u) * 16u);
                            }
                        }
#pragma unroll
                        for (int t = 0; t < kBootstrapTile; ++t) {
                            if (m0 + t >= M) break;   // wave-uniform
                            const unsigned long long total = wave_sum(packed[t]);   // every field at most 2^14
                            if (lane == 0) {
#pragma unroll
                                for (int c = 0; c < 4; ++c) bootstrap_add(out + (m0 + t) * 4 + c, (total >> (16 * c)) & 0xffffull);
                            }
                        }
                    }
                }
            }
        }
    }
}

// the outcome class of every row at its margin: tn 0, fp 1, fn 2, tp 3
__global__ __launch_bounds__(kBootstrapCheckThreads) void ds_outcome_codes_kernel(const float *margins, const float *target,
                                                                                 int64_t n, double cut, uint8_t *codes)
{
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBootstrapCheckThreads + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * kBootstrapCheckThreads) {
        const bool positive = forest_positive(forest_probability(margins[i]), cut);
        const bool actual = target[i] != 0.f;
        codes[i] = static_cast<uint8_t>((actual ? 2 : 0) + (positive ? 1 : 0));
    }
}

static int bootstrap_check_scalars(const char *what, int32_t n_sets, int64_t n, bool has_unit, int64_t n_units,
                                   int32_t n_boot)
{
    DS_REQUIRE(n_sets >= 1 && n_sets <= kBootstrapSetsMax, "%s: n_sets = %d outside [1, %d]", what, n_sets,
               kBootstrapSetsMax);
    DS_REQUIRE(n_boot >= 1 && n_boot <= kBootstrapBootMax, "%s: n_boot = %d outside [1, %d]", what, n_boot,
               kBootstrapBootMax);
    DS_REQUIRE(n >= 0 && n <= kBootstrapRowsMax, "%s: n = %lld outside [0, 2^31]", what, (long long)n);
    if (has_unit)
        DS_REQUIRE(n == 0 || (n_units >= 1 && n_units <= kBootstrapRowsMax), "%s: n_units = %lld outside [1, 2^31]", what,
                   (long long)n_units);
    else
        DS_REQUIRE(n_units == n, "%s: n_units = %lld, but without units every one of the %lld rows is its own unit", what,
                   (long long)n_units, (long long)n);
    return DS_OK;
}

static dim3 bootstrap_row_grid(int64_t n)
{
    return dim3(grid_cap((n + kBootstrapCheckThreads - 1) / kBootstrapCheckThreads, g_bootstrap_max_blocks.get()));
}

template <bool kUnits, bool kLds>
static int bootstrap_launch(const BootstrapArgs &args, dim3 grid, size_t lds, hipStream_t stream)
{
    DS_TRY(ds::allow_dynamic_lds(ds_bootstrap_kernel<kUnits, kLds>, lds));
    DS_LAUNCH((ds_bootstrap_kernel<kUnits, kLds>), grid, dim3(kBootstrapThreads), lds, stream, args);
    return DS_OK;
}

// The arguments have passed bootstrap_check_scalars and n > 0.  Each `_at` names a pointer into HBM that is read once
// `scratch` is allocated here: the caller's own, or a piece it has declared in `scratch`; unit_at is null without units.
static int bootstrap_enqueue(const char *what, Scratch &scratch, const uint8_t *const *codes_at, int32_t n_sets, int64_t n,
                             const int32_t *const *unit_at, int64_t n_units, int32_t n_boot, uint64_t seed,
                             long long *const *counts_at, long long *const *baseline_at, hipStream_t stream)
{
    unsigned long long *errors = nullptr;
    uint32_t *table = nullptr;
    const size_t table_words = unit_at ? static_cast<size_t>(n_units) * n_sets * 4 : 0;
    scratch.add(&errors, 2);
    scratch.add(&table, table_words);
    DS_TRY(scratch.allocate(what));
    const uint8_t *d_codes = *codes_at;
    const int32_t *d_unit = unit_at ? *unit_at : nullptr;
    long long *d_counts = *counts_at, *d_baseline = *baseline_at;
    DS_HIP(hipMemsetAsync(errors, 0, sizeof(unsigned long long) * 2, stream));
    if (table_words) DS_HIP(hipMemsetAsync(table, 0, sizeof(uint32_t) * table_words, stream));
    DS_LAUNCH(ds_bootstrap_check_kernel, bootstrap_row_grid(n), dim3(kBootstrapCheckThreads), 0, stream, d_codes,
              d_unit, n, n_sets, n_units, table, errors);
    unsigned long long found[2] = {0, 0};
    DS_HIP(hipMemcpyAsync(found, errors, sizeof(found), hipMemcpyDeviceToHost, stream));
    DS_HIP(hipStreamSynchronize(stream));
    DS_REQUIRE(found[0] == 0, "%s: %llu codes are above 3", what, found[0]);
    DS_REQUIRE(found[1] == 0, "%s: %llu units are outside [0, %lld)", what, found[1], (long long)n_units);

    const size_t counters = static_cast<size_t>(n_sets) * 4;
    DS_HIP(hipMemsetAsync(d_counts, 0, sizeof(long long) * counters * n_boot, stream));
    DS_HIP(hipMemsetAsync(d_baseline, 0, sizeof(long long) * counters, stream));
    BootstrapArgs args;
    args.codes = d_codes;
    args.table = reinterpret_cast<const uint4 *>(table);
    args.counts = reinterpret_cast<unsigned long long *>(d_counts);
    args.baseline = reinterpret_cast<unsigned long long *>(d_baseline);
    args.seed = seed;
    args.n_units = n_units;
    args.n_chunks = (n_units + kBootstrapChunk - 1) / kBootstrapChunk;
    args.n_sets = n_sets;
    args.n_boot = n_boot;
    args.padded_sets = (n_sets + kBootstrapTile - 1) / kBootstrapTile * kBootstrapTile;
    const int64_t replicates = static_cast<int64_t>(n_boot) + 1;   // and the baseline
    int64_t per_block = g_bootstrap_replicates_per_block.get();
    if (per_block <= 0)   // whole waves, and enough workgroups for every CU
        per_block = kBootstrapWaves * ((replicates + kBootstrapWaves * kBootstrapTargetBlocks - 1) /
                                       (kBootstrapWaves * kBootstrapTargetBlocks));
    per_block = std::min<int64_t>(per_block, replicates);
    args.per_block = static_cast<int32_t>(per_block);
    args.n_groups = static_cast<int32_t>((replicates + per_block - 1) / per_block);
    const int64_t cap = g_bootstrap_max_blocks.get();
    const unsigned grid_x = grid_cap(args.n_groups, cap);
    // a cap that was set holds for either dimension; the default leaves the grid 2 * cap workgroups in all
    const int64_t cap_y = g_bootstrap_max_blocks.is_set() ? cap : std::max<int64_t>(1, 2 * cap / grid_x);
    const dim3 grid(grid_x, grid_cap(args.n_chunks, cap_y, 65535));
    const bool units = d_unit != nullptr;
    const int64_t bytes = units ? n_units * n_sets * static_cast<int64_t>(sizeof(uint4)) : n_units * args.padded_sets;
    const bool in_lds = g_bootstrap_table_in_lds.get() != 0 && bytes <= kBootstrapLdsBytes;
    const size_t lds = in_lds ? static_cast<size_t>((bytes + 15) / 16 * 16) : 0;
    if (units)
        DS_TRY(in_lds ? bootstrap_launch<true, true>(args, grid, lds, stream)
                      : bootstrap_launch<true, false>(args, grid, 0, stream));
    else
        DS_TRY(in_lds ? bootstrap_launch<false, true>(args, grid, lds, stream)
                      : bootstrap_launch<false, false>(args, grid, 0, stream));
    DS_HIP(hipStreamSynchronize(stream));   // the table is freed on return
    return DS_OK;
}

}  // namespace ds

extern "C" {

int ds_bootstrap_option(const char *name, int64_t value)
{
    return ds::set_option("ds_bootstrap_option", ds::g_bootstrap_options, name, value);
}

int ds_bootstrap_counts_device(const uint8_t *d_codes, int32_t n_sets, int64_t n, const int32_t *d_unit, int64_t n_units,
                               int32_t n_boot, uint64_t seed, long long *d_counts, long long *d_baseline, void *stream)
{
    const char *what = "ds_bootstrap_counts_device";
    DS_TRY(ds::bootstrap_check_scalars(what, n_sets, n, d_unit != nullptr, n_units, n_boot));
    DS_REQUIRE(d_counts != nullptr && d_baseline != nullptr && (n == 0 || d_codes != nullptr), "%s: null pointer", what);
    hipStream_t queue = static_cast<hipStream_t>(stream);
    if (n == 0) {
        DS_HIP(hipMemsetAsync(d_counts, 0, sizeof(long long) * 4 * n_sets * static_cast<size_t>(n_boot), queue));
        DS_HIP(hipMemsetAsync(d_baseline, 0, sizeof(long long) * 4 * n_sets, queue));
        DS_HIP(hipStreamSynchronize(queue));
        return DS_OK;
    }
    ds::Scratch scratch;
    return ds::bootstrap_enqueue(what, scratch, &d_codes, n_sets, n, d_unit ? &d_unit : nullptr, n_units, n_boot, seed,
                                 &d_counts, &d_baseline, queue);
}

int ds_bootstrap_counts(const uint8_t *codes, int32_t n_sets, int64_t n, const int32_t *unit, int64_t n_units,
                        int32_t n_boot, uint64_t seed, long long *counts, long long *baseline)
{
    const char *what = "ds_bootstrap_counts";
    DS_TRY(ds::bootstrap_check_scalars(what, n_sets, n, unit != nullptr, n_units, n_boot));
    DS_REQUIRE(counts != nullptr && baseline != nullptr && (n == 0 || codes != nullptr), "%s: null pointer", what);
    const size_t counters = static_cast<size_t>(n_sets) * 4;
    for (int64_t e = 0; e < n * n_sets; ++e)
        DS_REQUIRE(codes[e] <= 3, "%s: the code %d of row %lld of set %lld is above 3", what, (int)codes[e],
                   (long long)(e % n), (long long)(e / n));
    if (unit != nullptr)
        for (int64_t i = 0; i < n; ++i)
            DS_REQUIRE(unit[i] >= 0 && unit[i] < n_units, "%s: unit[%lld] = %d is outside [0, %lld)", what, (long long)i,
                       unit[i], (long long)n_units);
    if (n == 0) {
        std::memset(counts, 0, sizeof(long long) * counters * n_boot);
        std::memset(baseline, 0, sizeof(long long) * counters);
        return DS_OK;
    }
    ds::Scratch scratch;
    const uint8_t *d_codes = nullptr;
    const int32_t *d_unit = nullptr;
    long long *d_counts = nullptr, *d_baseline = nullptr;
    scratch.stage(&d_codes, codes, static_cast<size_t>(n) * n_sets);
    if (unit) scratch.stage(&d_unit, unit, static_cast<size_t>(n));
    scratch.add(&d_counts, counters * n_boot);
    scratch.add(&d_baseline, counters);
    DS_TRY(ds::bootstrap_enqueue(what, scratch, &d_codes, n_sets, n, unit ? &d_unit : nullptr, n_units, n_boot, seed,
                                 &d_counts, &d_baseline, nullptr));
    DS_HIP(hipMemcpy(counts, d_counts, sizeof(long long) * counters * n_boot, hipMemcpyDeviceToHost));
    DS_HIP(hipMemcpy(baseline, d_baseline, sizeof(long long) * counters, hipMemcpyDeviceToHost));
    return DS_OK;
}

int ds_outcome_codes_device(const float *d_margins, const float *d_target, int64_t n, double threshold, uint8_t *d_codes,
                            void *stream)
{
    const char *what = "ds_outcome_codes_device";
    DS_REQUIRE(n >= 0 && n <= ds::kBootstrapRowsMax, "%s: n = %lld outside [0, 2^31]", what, (long long)n);
    DS_REQUIRE(threshold > 0.0 && threshold < 1.0, "%s: threshold = %g is not in (0, 1)", what, threshold);
    if (n == 0) return DS_OK;
    DS_REQUIRE(d_margins != nullptr && d_target != nullptr && d_codes != nullptr, "%s: null pointer", what);
    DS_LAUNCH(ds::ds_outcome_codes_kernel, ds::bootstrap_row_grid(n), dim3(ds::kBootstrapCheckThreads), 0,
              static_cast<hipStream_t>(stream), d_margins, d_target, n, threshold, d_codes);
    return DS_OK;
}

}  // extern "C"
