// Edit scripts of title pairs and the title generator that follows a learned profile (this project's own; DESIGN.md
// section 8, "Edit scripts and the learned misspelling model"; the rule is stated in include/doppel_amd.h).
//
// ds_edit_align: one wave per pair.  The optimal-string-alignment table D of a (the truth side, m rows) against b (the
// observed side, n columns) is filled row by row.  Lane l owns the columns j = 4l + 1 .. 4l + 4 of every row, so 64
// lanes cover the 255 columns a title can have.  Of a cell's four predecessors only D[i][j - 1] lies in the row being
// made; with base[j] = the minimum over the other three, D[i][j] = j + min(i, min over k <= j of (base[k] - k)), which
// is a prefix minimum: inside the lane's four columns, then over the lanes by six __shfl_up steps.  What a pair holds:
//   registers  per lane rows i - 1 and i - 2 of its four columns (8 values), its four characters of b and the one
//              before them, the byte of directions it is filling;
//   LDS        a and b (256 bytes each), the script while it is traced (512 bytes), and the direction of every cell by
//              the priority rule, 2 bits per cell: lane l's four columns of row i are one byte, four rows one dword at
//              [(i - 1) / 4][l], 256 bytes per four rows.  The store is sized by the longest truth title of the BATCH
//              (found by the check kernel that runs first anyway): 64 * ceil(m_max / 4) * 4 bytes, 4.5 KiB at 70
//              characters, 16 KiB at 255.
// Lane 0 walks the directions back from (m, n), writing the script backwards into LDS and counting the rare events
// (substitute, delete, insert, transpose) with 64-bit atomics in HBM; the frequent ones (match, seen) go to 64-bit
// counters in LDS that the workgroup adds to HBM once, at its end.  All sums are integer additions, so any order gives
// the same block.  The script leaves with one 8-byte store per lane.  A workgroup is pairs_per_group (4) waves, each
// with a pair of its own; a CU holds what its 160 KiB of LDS and 32 waves admit: 28 pairs at 70 characters, 9 at 255.
//
// ds_misspell_titles_profile: one lane per title as in ds_misspell_titles (ds_training.hip); the rates, the cumulative
// edit histogram and the substitute / insert tables (24 KiB) sit in LDS next to the lanes' working titles.
#include <algorithm>

#include "ds_launch.h"
#include "ds_options.h"
#include "ds_title_ops.h"
#include "ds_wave.h"

namespace ds {

constexpr int kEditCodes = 38;                    // 0 = the end of a title, 1..37 the characters
constexpr int kEditOpsStride = 512;               // bytes per script row of d_ops (>= 255 + 255)
constexpr int kEditPairBytes = 256 + 256 + kEditOpsStride;   // a, b, script
constexpr int kEditCounterBytes = 2 * kEditCodes * 8;         // match, seen
constexpr int kEditPairsPerGroup = 4, kEditMaxPairsPerGroup = 16, kEditMaxBlocks = 4096;
constexpr int kEditLdsLimit = 64 * 1024;
constexpr int kEditBig = 1 << 20;                 // above every distance
constexpr int64_t kProfileMaxCount = int64_t(1) << 40;
constexpr int kProfileScaleBits = 30;

static Option g_edit_pairs_per_group{"pairs_per_group", 0, kEditMaxPairsPerGroup, kEditPairsPerGroup, true};
static Option g_edit_max_blocks{"max_blocks", 0, 65536, kEditMaxBlocks, true};
static Option *const g_edit_options[] = {&g_edit_pairs_per_group, &g_edit_max_blocks};

struct EditSide {
    const uint8_t *enc, *len;
    const int32_t *rows;      // null: row i
    int64_t stride, n;
};

struct EditArgs {
    EditSide a, b;
    int64_t n;
    int32_t max_edits, dir_words;       // dir_words = ceil(longest a / 4): dwords per lane of the direction store
    int32_t *distance;
    uint8_t *ops;
    int32_t *ops_length;
    unsigned long long *counts;
};

__device__ __forceinline__ void edit_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// report[0] = pairs with a row out of range or a title that is not 3..255 codes 1..37, report[1] = the longest a
__global__ __launch_bounds__(256) void ds_edit_check_kernel(EditArgs args, int32_t *report)
{
    const int lane = threadIdx.x & 63;
    const int64_t waves = static_cast<int64_t>(gridDim.x) * (blockDim.x >> 6);
    int longest = 0, errors = 0;
    for (int64_t pair = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6); pair < args.n; pair += waves) {
        bool bad = false;
        for (int side = 0; side < 2; ++side) {
            const EditSide &s = side ? args.b : args.a;
            const int64_t row = s.rows ? s.rows[pair] : pair;
            if (row < 0 || row >= s.n) {
                bad = true;
                continue;
            }
            const int length = s.len[row];
            if (length < 3 || length > DS_MAX_CHARS || length > s.stride) {
                bad = true;
                continue;
            }
            for (int c = lane; c < length; c += 64) {
                const uint8_t code = s.enc[row * s.stride + c];
                bad = bad || code < kSpaceCode || code > kLastCode;
            }
            if (side == 0) longest = max(longest, length);
        }
        errors += __any(bad) ? 1 : 0;
    }
    if (lane == 0) {
        if (errors) atomicAdd(&report[0], errors);
        atomicMax(&report[1], longest);
    }
}

// One pair on one wave.  s_a, s_b: 256 bytes each, s_ops: 512 bytes, s_dir: dir_words x 64 dwords, all this wave's own.
__device__ void edit_align_pair(const EditArgs &args, int64_t pair, uint8_t *s_a, uint8_t *s_b, uint8_t *s_ops,
                                uint32_t *s_dir, unsigned long long *s_match, unsigned long long *s_seen)
{
    const int lane = threadIdx.x & 63;
    const int64_t row_a = args.a.rows ? args.a.rows[pair] : pair, row_b = args.b.rows ? args.b.rows[pair] : pair;
    const int m = args.a.len[row_a], n = args.b.len[row_b];
    const uint8_t *a = args.a.enc + row_a * args.a.stride, *b = args.b.enc + row_b * args.b.stride;
    edit_wave_sync();   // lane 0 has finished with the previous pair's LDS
    for (int c = lane; c < m; c += 64) s_a[c] = a[c];
    for (int c = lane; c < n; c += 64) s_b[c] = b[c];
    edit_wave_sync();

    // ---- forward: lane l holds the columns j0 .. j0 + 3
    const int j0 = 4 * lane + 1;
    int bc[4], bl[4];          // b[j - 1] and b[j - 2] of column j (0: no such character; never equal to a code)
#pragma unroll
    for (int c = 0; c < 4; ++c) bc[c] = j0 + c <= n ? s_b[j0 + c - 1] : 0;
    bl[0] = lane > 0 && j0 - 1 <= n ? s_b[j0 - 2] : 0;
#pragma unroll
    for (int c = 1; c < 4; ++c) bl[c] = bc[c - 1];
    int prev[4], prev2[4];     // D[i - 1][j], D[i - 2][j]
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        prev[c] = j0 + c;
        prev2[c] = 0;
    }
    uint32_t packed = 0;
    int a1 = 0;                // a[i - 2]
    for (int i = 1; i <= m; ++i) {
        const int a0 = s_a[i - 1];
        int left = __shfl_up(prev[3], 1);        // D[i - 1][j0 - 1]
        int two_a = __shfl_up(prev2[2], 1);      // D[i - 2][j0 - 2]
        int two_b = __shfl_up(prev2[3], 1);      // D[i - 2][j0 - 1]
        if (lane == 0) {
            left = i - 1;
            two_a = kEditBig;                    // column 1 has no transposition
            two_b = i - 2;
        }
        int diag[4], two[4], base[4], low[4];
        bool equal[4], swap[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + c;
            diag[c] = c == 0 ? left : prev[c - 1];
            two[c] = c == 0 ? two_a : c == 1 ? two_b : prev2[c - 2];
            equal[c] = a0 == bc[c];
            swap[c] = i > 1 && j > 1 && a0 == bl[c] && a1 == bc[c];
            int value = min(diag[c] + (equal[c] ? 0 : 1), prev[c] + 1);
            if (swap[c]) value = min(value, two[c] + 1);
            base[c] = j <= n ? value : kEditBig;
            low[c] = c == 0 ? base[c] - j : min(low[c - 1], base[c] - j);
        }
        int inclusive = low[3];
#pragma unroll
        for (int offset = 1; offset < 64; offset <<= 1) {
            const int other = __shfl_up(inclusive, offset);
            if (lane >= offset) inclusive = min(inclusive, other);
        }
        int before = __shfl_up(inclusive, 1);    // over the columns of the lanes before this one
        before = lane == 0 ? i : min(before, i); // and column 0: D[i][0] - 0 = i
        uint32_t byte = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int current = min(low[c], before) + j0 + c;
            const int direction = (equal[c] ? current == diag[c] : current == diag[c] + 1) ? 0
                                  : (swap[c] && current == two[c] + 1)                     ? 1
                                  : current == prev[c] + 1                                 ? 2
                                                                                           : 3;
            byte |= static_cast<uint32_t>(direction) << (2 * c);
            prev2[c] = prev[c];
            prev[c] = current;
        }
        packed |= byte << (8 * ((i - 1) & 3));
        if ((i & 3) == 0 || i == m) {
            s_dir[((i - 1) >> 2) * 64 + lane] = packed;
            packed = 0;
        }
        a1 = a0;
    }
    const int cn = (n - 1) & 3;
    const int distance = __shfl(cn == 0 ? prev[0] : cn == 1 ? prev[1] : cn == 2 ? prev[2] : prev[3], (n - 1) >> 2);
    edit_wave_sync();

    // ---- traceback on lane 0: the script backwards from the end of s_ops
    const bool counted = distance <= args.max_edits;
    unsigned long long *counts = args.counts;
    int length = 0;
    if (lane == 0) {
        int i = m, j = n, at = kEditOpsStride;
        while (i > 0 || j > 0) {   // at most m + n <= 510 steps: every step takes a character of a or of b
            int op;
            if (i == 0) op = DS_EDIT_OP_INSERT;
            else if (j == 0) op = DS_EDIT_OP_DELETE;
            else {
                const uint32_t word = s_dir[((i - 1) >> 2) * 64 + ((j - 1) >> 2)];
                const int direction = (word >> (8 * ((i - 1) & 3) + 2 * ((j - 1) & 3))) & 3;
                // a transposition is only ever stored at i, j > 1 (the forward pass checks it)
                op = direction == 0 ? (s_a[i - 1] == s_b[j - 1] ? DS_EDIT_OP_MATCH : DS_EDIT_OP_SUBSTITUTE)
                     : direction == 1 ? DS_EDIT_OP_TRANSPOSE
                                      : direction;
            }
            s_ops[--at] = static_cast<uint8_t>(op);
            if (counted && counts) {
                if (op == DS_EDIT_OP_MATCH) atomicAdd(&s_match[s_a[i - 1]], 1ull);
                else if (op == DS_EDIT_OP_SUBSTITUTE) atomicAdd(&counts[DS_EDIT_SUBSTITUTE + s_a[i - 1] * kEditCodes + s_b[j - 1]], 1ull);
                else if (op == DS_EDIT_OP_DELETE) atomicAdd(&counts[DS_EDIT_DELETE + s_a[i - 1]], 1ull);
                else if (op == DS_EDIT_OP_INSERT) atomicAdd(&counts[DS_EDIT_INSERT + (i < m ? s_a[i] : 0) * kEditCodes + s_b[j - 1]], 1ull);
                else atomicAdd(&counts[DS_EDIT_TRANSPOSE + s_a[i - 2] * kEditCodes + s_a[i - 1]], 1ull);
            }
            i -= op == DS_EDIT_OP_INSERT ? 0 : op == DS_EDIT_OP_TRANSPOSE ? 2 : 1;
            j -= op == DS_EDIT_OP_DELETE ? 0 : op == DS_EDIT_OP_TRANSPOSE ? 2 : 1;
        }
        length = kEditOpsStride - at;
        if (counts) {
            if (counted) {
                atomicAdd(&counts[DS_EDIT_COUNTED], 1ull);
                atomicAdd(&counts[DS_EDIT_EDITS + distance], 1ull);
                atomicAdd(&s_seen[0], 1ull);
            } else {
                atomicAdd(&counts[DS_EDIT_SKIPPED], 1ull);
            }
        }
        if (args.distance) args.distance[pair] = distance;
        if (args.ops_length) args.ops_length[pair] = length;
    }
    if (counted && counts)
        for (int c = lane; c < m; c += 64) atomicAdd(&s_seen[s_a[c]], 1ull);
    if (args.ops) {
        length = __shfl(length, 0);
        edit_wave_sync();
        const int start = kEditOpsStride - length;
        uint64_t value = 0;
#pragma unroll
        for (int byte = 0; byte < 8; ++byte) {
            const int index = 8 * lane + byte;
            if (index < length) value |= static_cast<uint64_t>(s_ops[start + index]) << (8 * byte);
        }
        reinterpret_cast<uint64_t *>(args.ops + pair * kEditOpsStride)[lane] = value;   // the whole row, zeros behind the script
    }
}

__global__ __launch_bounds__(1024) void ds_edit_align_kernel(EditArgs args)
{
    extern __shared__ __align__(16) unsigned char edit_lds[];
    const int wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    unsigned long long *s_match = reinterpret_cast<unsigned long long *>(edit_lds), *s_seen = s_match + kEditCodes;
    unsigned char *mine = edit_lds + kEditCounterBytes + static_cast<size_t>(wave) * (kEditPairBytes + args.dir_words * 256);
    for (int c = threadIdx.x; c < 2 * kEditCodes; c += blockDim.x) s_match[c] = 0ull;
    __syncthreads();
    for (int64_t pair = static_cast<int64_t>(blockIdx.x) * waves + wave; pair < args.n;
         pair += static_cast<int64_t>(gridDim.x) * waves)
        edit_align_pair(args, pair, mine, mine + 256, mine + 512, reinterpret_cast<uint32_t *>(mine + kEditPairBytes),
                        s_match, s_seen);
    __syncthreads();
    if (args.counts)
        for (int c = threadIdx.x; c < 2 * kEditCodes; c += blockDim.x) {
            const unsigned long long value = s_match[c];
            if (value) atomicAdd(&args.counts[c < kEditCodes ? DS_EDIT_MATCH + c : DS_EDIT_SEEN + c - kEditCodes], value);
        }
}

// ---- the generator that follows a profile ------------------------------------------------------------------------------
struct ProfileTables {
    uint64_t cumulative[33];                        // [d] = edits[1] + .. + edits[d]; [0] = 0
    uint64_t substitute[kEditCodes * kEditCodes];   // [a code][b code]
    uint64_t insert[kEditCodes * kEditCodes];       // [context][inserted code]
    uint32_t rate[4][kEditCodes];                   // substitute, delete, transpose, insert; units of 2^-30 per character
};

struct PositionWeights {
    uint32_t substitute, remove, transpose, insert;
    __device__ uint64_t sum() const { return uint64_t(substitute) + remove + transpose + insert; }
};

__device__ inline PositionWeights weights_at(const ProfileTables &tables, const uint8_t *w, int length, int p)
{
    PositionWeights x{0u, 0u, 0u, 0u};
    const int code = p < length ? w[p] : 0;
    if (p < length) {
        x.substitute = tables.rate[0][code];
        x.remove = length <= 3 ? 0u : tables.rate[1][code];
        x.transpose = p + 1 < length && w[p] != w[p + 1] ? tables.rate[2][code] : 0u;
    }
    x.insert = length >= DS_MAX_CHARS ? 0u : tables.rate[3][code];
    return x;
}

// a code drawn from row[0..37] by its counts, walking the codes in ascending order and leaving out `skip`
__device__ inline uint8_t draw_code(Rng &rng, const uint64_t *row, int skip)
{
    uint64_t sum = 0;
    for (int y = 0; y < kEditCodes; ++y) sum += y == skip ? 0ull : row[y];
    uint64_t r = rng.below64(sum);
    for (int y = 0; y < kEditCodes; ++y) {
        const uint64_t weight = y == skip ? 0ull : row[y];
        if (r < weight) return static_cast<uint8_t>(y);
        r -= weight;
    }
    return kSpaceCode;   // not reached: the chosen operation has a positive weight, so sum > 0
}

// the title in w after k edits drawn from the profile; the result (transformed) in t
__device__ int misspell_by_profile(Rng &rng, const ProfileTables &tables, uint8_t *w, uint8_t *t, int length)
{
    const uint64_t drawn = rng.below64(tables.cumulative[32]);
    int k = 1;
    while (k < 32 && tables.cumulative[k] <= drawn) ++k;
    for (int edit = 0; edit < k; ++edit) {
        uint64_t total = 0;
        for (int p = 0; p <= length; ++p) total += weights_at(tables, w, length, p).sum();
        if (total == 0) break;
        uint64_t r = rng.below64(total);
        for (int p = 0; p <= length; ++p) {
            const PositionWeights x = weights_at(tables, w, length, p);
            if (r >= x.sum()) {
                r -= x.sum();
                continue;
            }
            if (r < x.substitute) {
                w[p] = draw_code(rng, tables.substitute + w[p] * kEditCodes, w[p]);
            } else if (r < uint64_t(x.substitute) + x.remove) {
                erase_at(w, length, p);
            } else if (r < uint64_t(x.substitute) + x.remove + x.transpose) {
                const uint8_t first = w[p];
                w[p] = w[p + 1];
                w[p + 1] = first;
            } else {
                insert_at(w, length, p, draw_code(rng, tables.insert + (p < length ? w[p] : 0) * kEditCodes, -1));
            }
            break;
        }
    }
    return transform_into(w, length, t);
}

__global__ __launch_bounds__(kMisspellBlock) void ds_misspell_profile_kernel(
    const uint8_t *source_enc, const uint8_t *source_len, int64_t source_stride, int64_t n_source, const int32_t *rows,
    int64_t n, uint64_t seed, const ProfileTables *tables, uint8_t *out_enc, uint8_t *out_len, int32_t *error)
{
    __shared__ uint8_t work[kMisspellBlock][kWorkBytes];
    __shared__ uint8_t scratch[kMisspellBlock][kWorkBytes];
    __shared__ ProfileTables s_tables;
    const int lane = threadIdx.x;
    static_assert(sizeof(ProfileTables) % 4 == 0, "copied by dwords");
    for (int d = lane; d < static_cast<int>(sizeof(ProfileTables) / 4); d += kMisspellBlock)
        reinterpret_cast<uint32_t *>(&s_tables)[d] = reinterpret_cast<const uint32_t *>(tables)[d];
    __syncthreads();
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kMisspellBlock;
    const int64_t i = first + lane;
    uint8_t *w = work[lane], *t = scratch[lane];
    if (i < n) {
        const int64_t row = rows ? rows[i] : i;
        int length = 0;
        bool ok = row >= 0 && row < n_source;
        if (ok) {
            length = source_len[row];
            ok = length >= 3 && length <= DS_MAX_CHARS && length <= source_stride;
        }
        if (ok) {
            const uint8_t *title = source_enc + row * source_stride;
            bool letter = false;
            for (int c = 0; c < length; ++c) {
                const uint8_t code = title[c];
                w[c] = code;
                ok = ok && code >= kSpaceCode && code <= kLastCode;
                letter = letter || code != kSpaceCode;
            }
            ok = ok && letter;
        }
        if (ok) {
            Rng rng(seed, DS_MISSPELL_PURPOSE_PROFILE, static_cast<uint64_t>(row));
            length = misspell_by_profile(rng, s_tables, w, t, length);
        } else {
            atomicAdd(error, 1);
            length = 0;
            for (int c = 0; c < DS_MAX_CHARS; ++c) t[c] = 0;
        }
        out_len[i] = static_cast<uint8_t>(length);
    }
    __syncthreads();
    write_title_rows(scratch, first, n, out_enc);
}

// The checks of a profile and the rates derived from it, on the host.  Returns null when the profile is accepted, else
// what is wrong with it.
static const char *profile_tables_build(const int64_t *counts, ProfileTables &tables)
{
    constexpr int K = kEditCodes;
    for (int i = 0; i < DS_EDIT_COUNTS; ++i)
        if (counts[i] < 0 || counts[i] >= kProfileMaxCount) return "a count is negative or not below 2^40";
    const int64_t *seen = counts + DS_EDIT_SEEN, *match = counts + DS_EDIT_MATCH, *remove = counts + DS_EDIT_DELETE;
    const int64_t *substitute = counts + DS_EDIT_SUBSTITUTE, *insert = counts + DS_EDIT_INSERT;
    const int64_t *transpose = counts + DS_EDIT_TRANSPOSE;
    // what no alignment produces: an event of code 0 (the end of a title is only ever the context of an insertion), a
    // character substituted by itself
    bool impossible = match[0] != 0 || remove[0] != 0;
    for (int c = 0; c < K; ++c)
        impossible = impossible || substitute[c] != 0 || substitute[c * K] != 0 || substitute[c * K + c] != 0 ||
                     insert[c * K] != 0 || transpose[c] != 0 || transpose[c * K] != 0;
    if (impossible) return "a count that no alignment produces is not 0 (code 0 outside an insertion's context, or a "
                           "character substituted by itself)";
    tables.cumulative[0] = 0;
    for (int d = 1; d <= 32; ++d) tables.cumulative[d] = tables.cumulative[d - 1] + static_cast<uint64_t>(counts[DS_EDIT_EDITS + d]);
    if (tables.cumulative[32] == 0) return "edits[1..32] are all 0: the profile holds no misspelled pair";
    for (int c = 0; c < K; ++c) {
        unsigned __int128 sums[4] = {0, static_cast<unsigned __int128>(remove[c]), 0, 0};
        for (int y = 0; y < K; ++y) {
            sums[0] += static_cast<uint64_t>(substitute[c * K + y]);
            sums[2] += static_cast<uint64_t>(transpose[c * K + y]);
            sums[3] += static_cast<uint64_t>(insert[c * K + y]);
        }
        for (int r = 0; r < 4; ++r) {
            const unsigned __int128 rate = seen[c] == 0 ? 0 : (sums[r] << kProfileScaleBits) / static_cast<uint64_t>(seen[c]);
            if (rate >> 32) return "a rate is 4 events per seen character or more";
            tables.rate[r][c] = static_cast<uint32_t>(rate);
        }
    }
    for (int i = 0; i < K * K; ++i) {
        tables.substitute[i] = static_cast<uint64_t>(substitute[i]);
        tables.insert[i] = static_cast<uint64_t>(insert[i]);
    }
    return nullptr;
}

}  // namespace ds

extern "C" {

int ds_edit_option(const char *name, int64_t value)
{
    return ds::set_option("ds_edit_option", ds::g_edit_options, name, value);
}

int ds_edit_align(const ds_titles *truth, const int32_t *d_truth_rows, const ds_titles *observed,
                  const int32_t *d_observed_rows, int64_t n, int32_t max_edits, int32_t *d_distance, uint8_t *d_ops,
                  int32_t *d_ops_length, int64_t *d_counts)
{
    DS_REQUIRE(truth != nullptr && observed != nullptr, "ds_edit_align: null title table");
    DS_REQUIRE(truth->device == observed->device, "ds_edit_align: the two tables live on devices %d and %d", truth->device,
               observed->device);
    DS_REQUIRE(n >= 0 && n < (int64_t(1) << 31), "ds_edit_align: n = %lld out of range [0, 2^31)", (long long)n);
    DS_REQUIRE(max_edits >= 0 && max_edits <= 32, "ds_edit_align: max_edits = %d out of range [0, 32]", max_edits);
    DS_REQUIRE((d_ops == nullptr) == (d_ops_length == nullptr), "ds_edit_align: d_ops and d_ops_length go together");
    DS_REQUIRE(reinterpret_cast<uintptr_t>(d_ops) % 8 == 0, "ds_edit_align: d_ops is not 8-byte aligned");
    if (n == 0) return DS_OK;
    DS_HIP(hipSetDevice(truth->device));
    ds::EditArgs args{};
    args.a = {truth->enc.ptr, truth->len.ptr, d_truth_rows, truth->stride, truth->n};
    args.b = {observed->enc.ptr, observed->len.ptr, d_observed_rows, observed->stride, observed->n};
    args.n = n;
    args.max_edits = max_edits;
    args.distance = d_distance;
    args.ops = d_ops;
    args.ops_length = d_ops_length;
    args.counts = reinterpret_cast<unsigned long long *>(d_counts);
    const int64_t max_blocks = ds::g_edit_max_blocks.get();

    // every pair is checked before anything is written; the same pass finds the longest truth title
    ds::DeviceBuffer<int32_t> report;
    DS_TRY(report.allocate(2));
    int32_t found[2] = {0, 0};
    DS_HIP(hipMemsetAsync(report.ptr, 0, 2 * sizeof(int32_t), nullptr));
    DS_LAUNCH(ds::ds_edit_check_kernel, dim3(ds::grid_cap((n + 3) / 4, max_blocks)),
              dim3(256), 0, nullptr, args, report.ptr);
    DS_HIP(hipMemcpy(found, report.ptr, sizeof(found), hipMemcpyDeviceToHost));
    DS_REQUIRE(found[0] == 0, "ds_edit_align: %d pairs have a row out of range or a title that is not a transformed "
               "title (3..255 codes 1..37)", found[0]);

    args.dir_words = (found[1] + 3) / 4;
    const int64_t pair_bytes = ds::kEditPairBytes + int64_t(args.dir_words) * 256;
    int64_t pairs = ds::g_edit_pairs_per_group.get();
    pairs = std::max<int64_t>(1, std::min(pairs, (ds::kEditLdsLimit - ds::kEditCounterBytes) / pair_bytes));
    const size_t lds = static_cast<size_t>(ds::kEditCounterBytes + pairs * pair_bytes);
    DS_TRY(ds::allow_dynamic_lds(ds::ds_edit_align_kernel, lds));
    DS_LAUNCH(ds::ds_edit_align_kernel, dim3(ds::grid_cap((n + pairs - 1) / pairs, max_blocks)),
              dim3(static_cast<unsigned>(64 * pairs)), lds, nullptr, args);
    DS_HIP(hipStreamSynchronize(nullptr));
    return DS_OK;
}

int ds_misspell_titles_profile(ds_titles *source, const int32_t *d_rows, int64_t n, uint64_t seed, const int64_t *d_profile,
                               ds_titles **out)
{
    DS_REQUIRE(out != nullptr, "ds_misspell_titles_profile: out is null");
    *out = nullptr;
    DS_REQUIRE(source != nullptr && d_profile != nullptr, "ds_misspell_titles_profile: null source table or profile");
    DS_REQUIRE(n >= 1, "ds_misspell_titles_profile: need at least one title");
    DS_REQUIRE(n < (int64_t(1) << 31) / ds::kMisspellBlock * ds::kMisspellBlock, "ds_misspell_titles_profile: too many titles");
    DS_HIP(hipSetDevice(source->device));
    std::vector<int64_t> counts(DS_EDIT_COUNTS);
    DS_HIP(hipMemcpy(counts.data(), d_profile, counts.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    std::vector<ds::ProfileTables> tables(1);
    const char *wrong = ds::profile_tables_build(counts.data(), tables[0]);
    DS_REQUIRE(wrong == nullptr, "ds_misspell_titles_profile: %s", wrong);
    ds::DeviceBuffer<ds::ProfileTables> d_tables;
    DS_TRY(d_tables.upload(tables.data(), 1));

    std::unique_ptr<ds_titles> titles(new ds_titles());
    titles->device = source->device;
    titles->n = n;
    titles->stride = DS_MAX_CHARS;
    ds::DeviceBuffer<int32_t> error;
    DS_TRY(titles->enc.allocate(static_cast<size_t>(n) * DS_MAX_CHARS));
    DS_TRY(titles->len.allocate(static_cast<size_t>(n)));
    DS_TRY(error.allocate(1));
    int32_t errors = 0;
    DS_HIP(hipMemsetAsync(error.ptr, 0, sizeof(int32_t), nullptr));
    DS_LAUNCH(ds::ds_misspell_profile_kernel, dim3(static_cast<unsigned>((n + ds::kMisspellBlock - 1) / ds::kMisspellBlock)),
              dim3(ds::kMisspellBlock), 0, nullptr, source->enc.ptr, source->len.ptr, source->stride, source->n,
              d_rows, n, seed, d_tables.ptr, titles->enc.ptr, titles->len.ptr, error.ptr);
    DS_HIP(hipMemcpy(&errors, error.ptr, sizeof(int32_t), hipMemcpyDeviceToHost));
    DS_REQUIRE(errors == 0, "ds_misspell_titles_profile: %d rows are out of range or not transformed titles (3..255 codes 1..37, "
               "one letter or digit at least)", errors);
    *out = titles.release();
    return DS_OK;
}

}  // extern "C"
