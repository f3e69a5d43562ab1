// IDF-weighted Jaccard of a batch of query titles against every truth title + the reference's threshold top-k.
//
// Reference semantics (doppelspeller/match_maker.py):
//   fast_jaccard   :16-50   scores[t] = float32 sum, in the query's column order, of idf32[g] over the query's
//                           n-gram columns g whose posting list contains t;
//                           jaccard[t] = float64(scores[t]) / (float64(sums[t]) + (maxint - float64(scores[t])))
//   fast_arg_top_k :53-71   m = float32(k-th largest positive jaccard, 0 if fewer than k);
//                           threshold = float64(m) - float64(float32(1e-6));
//                           result = the k LARGEST ROW INDEXES among {t : jaccard[t] >= threshold}, descending.
//
// Two kernels (DESIGN.md section 3), compiled per geometry (narrow: 256-thread workgroups, four per CU, tiles of 12288
// truth rows; wide: 512 threads, two per CU, 28672 rows; a tile = 16-bit fixed-point scores, two rows per LDS word):
//   ds_jaccard_topk_kernel   workgroups pulling queries from a work queue.  The truth rows are visited tile by tile.
//       Scores are accumulated with order-free LDS integer atomics, i.e. only APPROXIMATELY (the reference's float32
//       rounding depends on the column order); rows whose approximate jaccard can still reach the running k-th largest
//       value minus a rigorous error margin become candidates; a radix select over the candidate buffer tightens the
//       running value.  Once a running value exists, columns whose total IDF cannot lift a row over it on their own
//       ("non-essential", the MaxScore rule of top-k retrieval) are no longer traversed: their IDF mass enters the
//       test as an upper bound.  Tiles with few essential postings are handled sparsely (scatter, then a collect
//       sweep over the same postings that takes and re-zeroes the touched rows) instead of scanning the whole tile;
//       raw entries of an epoch of consecutive sparse tiles are refined together (one 32-byte row record each).
//       After the last tile the surviving candidates are evaluated EXACTLY: membership of the row in each query
//       column's posting list (signature bit or binary search), float32 sum in the reference's column order, float64
//       finalise, then the reference's threshold / arg-select.  Results are bit-exact; the approximation only decides
//       where the exact arithmetic is spent.
//   ds_jaccard_dense_kernel  the literal algorithm (1024 threads, one workgroup per CU: ordered scatter with a barrier per
//       column into a float32 score tile, float64 finalise) as a STREAMING selection from the last tile down -- an LDS
//       buffer of (value, row) compacted by the running threshold and the k-dominators rule, no N-vector in HBM -- for
//       the queries the fast kernel cannot bound: more than 128 columns, maxint <= 0, fewer than k positive rows,
//       massive non-twin ties, a column listed twice.
//
// This file is compiled once per geometry (ds_jaccard_wide.hip, ds_jaccard_narrow.hip define DS_GEOMETRY_NAME and the
// constants below and include it); everything lives in namespace ds::DS_GEOMETRY_NAME, the C entry points are in
// ds_jaccard.hip.
#include <cfloat>
#include <type_traits>
#include <cstdlib>

#include "ds_launch.h"

namespace ds {
namespace DS_GEOMETRY_NAME {

constexpr int kTile = DS_TILE_ROWS;          // truth rows per tile (multiple of 4096): packed 16-bit scores, two per LDS word
// A posting is (parity << 15) | (tile-local row >> 1) = (half, word) of the row's packed score; all four postings of a quad
// share their half (the index stores a sub-list's even rows, then its odd rows, each part padded to whole quads).
constexpr uint32_t kPadWord = kTile / 2;     // padding entry of a posting quad: the trash word after the tile
constexpr uint32_t kPadQuad = kPadWord * 0x10001u;
__device__ __forceinline__ uint32_t posting_row(uint32_t posting) { return ((posting & 0x7fffu) << 1) | (posting >> 15); }
constexpr int kThreads = DS_THREADS;         // fast kernel: threads per workgroup
constexpr int kWorkgroupsPerCu = DS_WGS_PER_CU;
static_assert(kTile % 4096 == 0 && kTile < 65536, "tile rows: whole scan iterations, 15-bit word indexes");
static_assert(kThreads >= 256 && kThreads % 64 == 0, "the radix histogram is cleared by threads 0..255");
constexpr int kCandidates = DS_CANDIDATES;   // capacity of the per-query candidate buffer in LDS
constexpr int kSelectSlack = 128;            // a selection leaves at least this much room for new candidates (an overflow is recoverable: admission floor)
constexpr int kPtrTiles = DS_PTR_TILES;      // tiles whose list pointers are cached in LDS at a time

struct JaccardArgs {
    const uint32_t *col_ptr;
    const uint16_t *postings;
    const uint16_t *posting_sums;
    const float *idf32;
    const float *sums32;
    const float *tile_sums_min;
    const float *tile_sums_max;
    const uint4 *rows;          // 32-byte row records: [0] = signature, [1] = (sums32 bits, duplicate rank, the caller's row index, -)
    const int8_t *sig_column;
    const void *row_start;      // forward index: the columns of row t (internal order) are row_cols[row_start[t] .. row_start[t + 1]);
    const void *row_cols;       // uint32 / uint16 entries unless forward_wide_start / forward_wide_cols (int64 / int32)
    int32_t forward_wide_start, forward_wide_cols;
    const int64_t *q_rowptr;
    const int32_t *q_cols;
    const double *q_maxint;
    int32_t *out_rows;
    int32_t *status;
    int32_t *control;
    int32_t *slow_list;
    const int32_t *take_order;  // nullable: position in the work queue -> query
    unsigned long long *phase;  // nullable: per-phase shader-clock sums (diagnostics, DS_PHASE_TIMERS=1)
    int64_t n_truth;
    int64_t n_columns;
    int64_t n_queries;
    int32_t n_tiles;
    int32_t k;
    int32_t sparse_quads;       // tiles with at most this many essential quads are handled sparsely
    int32_t literal_only;       // index holds values outside the fast kernel's assumptions: hand every query over
    int32_t rows_sorted;        // the index's internal row order ascends with sums32 (ds_index_create): tiles are visited from the
                                // query's own sums32 outwards and skipped once out of the threshold's reach
    int32_t select_min;         // candidates that trigger a selection: max(k, 16), computed by the host
    int32_t select_growth;      // next selection at select_growth / 2 times the kept candidates
    int64_t n_quads;            // posting quads in the index (bounds of `postings`)
    int64_t nnz;                // postings in the index (bounds of `row_cols`)
    float sums_min;
};

// control words in HBM
enum { kCtlQueue = 0, kCtlSlowCount = 1, kCtlErrors = 2, kCtlExact = 3, kCtlSelects = 4, kCtlSlowQueue = 5,
       kCtlSparseTiles = 6, kCtlDenseTiles = 7, kCtlSkippedColumns = 8, kCtlReason = 9 /* 9..14 */,
       kCtlRedos = 15 /* epochs processed again after a candidate-buffer overflow in a sparse tile */,
       kCtlRefines = 16, kCtlRawEntries = 17, kCtlSurvivors = 18, kCtlRawSparse = 19,
       kCtlBytes = 28 /* 28..29: uint64, bytes the fast kernel requested from global memory (all queries) */ };

// Consecutive sparse tiles whose raw entries a wave refines together ("epoch"): the refinement's global gathers stall the
// whole workgroup at the tile's second barrier, so they are paid once per epoch instead of once per tile.  The tile of
// an entry within its epoch travels in the spare high bits of its 16-bit local row (2 bits for 12288-row tiles, 1 for
// 28672-row tiles).  Thresholds only change at epoch ends (every entry is refined under the bounds it was scored with).
constexpr int kEpochTiles = DS_EPOCH_TILES;
static_assert(kEpochTiles >= 1 && kEpochTiles <= 256 && (kEpochTiles & (kEpochTiles - 1)) == 0, "epoch: a power of two, at most 256 tiles");
// longer epochs than the spare bits allow keep the entry's tile in a byte of its own (64 more bytes of LDS per wave)
constexpr bool kEpochInBytes = static_cast<long long>(kTile + 2) * kEpochTiles > 65536;
constexpr int kEpochShift = kEpochInBytes ? 16 : 14;
static_assert(kEpochInBytes || kTile + 2 <= (1 << kEpochShift), "a local row (or a padding row, kTile + 1) and the epoch bits share 16 bits");
// LDS carve-up of the fast kernel (bytes)
constexpr int kScoreWords = kTile / 2 + 16;  // two 16-bit scores per word + the trash word of the padding entries
constexpr int kOffLo = kScoreWords * 4;
constexpr int kOffRow = kOffLo + kCandidates * 4;
constexpr int kOffRaw = kOffRow + kCandidates * 4;  // per wave: 64 raw entries (fixed-point score << 16 | tile-local row)
constexpr int kOffRawTile = kOffRaw + (kThreads / 64) * 64 * 4;  // per wave: 64 bytes, the entries' tiles within the epoch (long epochs)
constexpr int kOffCols = kOffRawTile + (kEpochInBytes ? (kThreads / 64) * 64 : 0);
constexpr int kOffIdf = kOffCols + kMaxQueryColumns * 4;
constexpr int kOffMass = kOffIdf + kMaxQueryColumns * 4;
constexpr int kOffBitIdf = kOffMass + kMaxQueryColumns * 4;
constexpr int kOffFixed = kOffBitIdf + kSignatureBits * 4;
constexpr int kOffRank = kOffFixed + kMaxQueryColumns * 4;    // three byte arrays: rank, order, signature bit per column
constexpr int kOffOrder = kOffRank + kMaxQueryColumns;
constexpr int kOffSigBit = kOffOrder + kMaxQueryColumns;
constexpr int kOffMassTable = kOffSigBit + kMaxQueryColumns;
constexpr int kOffPtr = kOffMassTable + 256 * 4;  // mass_low[256] then mass_high[256] (16 bits each), or the radix histogram
constexpr int kOffHist = kOffMassTable;  // the radix histogram shares the mass table: every selection is followed by
                                         // a rebuild of the table before its next use
constexpr int kOffQuadPrefix = kOffPtr + kMaxQueryColumns * (kPtrTiles + 1) * 4;  // per tile: quads before column j
constexpr int kOffQuadBase = kOffQuadPrefix + kMaxQueryColumns * 4;               // per tile: first quad of column j - prefix
// Item directory of a tile (DESIGN.md section 3, "work distribution"): which column a quad of the tile's flattened essential
// lists belongs to, answered with two LDS round trips instead of a 7-step binary search.  For tiles of at most
// kDirItems items whose non-empty essential lists number at most kDirColumns:
//   dir_entry[c]   (first quad of the c-th non-empty list - quads before it, fixed-point IDF)      c < kDirColumns
//   dir_mask[i]    bit p set <=> a non-empty list starts at quad 64 i + p of the sequence          i < kDirItems
//   dir_count[i]   non-empty lists that start before item i
// quad g of item i, lane p = g - 64 i, belongs to list  dir_count[i] + popcount(dir_mask[i] & bits 0..p) - 1.
// Two copies of everything, used by alternate tiles: the directory of the NEXT tile is built (and the tile's first
// posting quads are requested) before the barrier that ends the current tile, while slower waves still read the
// current one; a copy's start bits are zeroed one tile ahead of the ORs that fill it (no barrier of its own).
constexpr int kDirItems = 64, kDirColumns = 64;
constexpr int kOffDirEntry = kOffQuadBase + kMaxQueryColumns * 4;
constexpr int kOffDirMask = kOffDirEntry + 2 * kDirColumns * 8;
constexpr int kOffDirCount = kOffDirMask + 2 * kDirItems * 8;
constexpr int kOffCtrl = kOffDirCount + 2 * kDirItems;
constexpr int kFastLdsBytes = kOffCtrl + 192;  // 48 control words
static_assert((kFastLdsBytes + 256) * kWorkgroupsPerCu <= 160 * 1024, "LDS budget of one CU exceeded");
// rows the exact stage takes: all the candidate buffer holds, as far as its scratch (24 bytes per row) fits the score tile
constexpr int kExactRows = kCandidates * 24 + kMaxQueryColumns * 5 + kThreads * 2 <= kTile * 2 ? kCandidates : ((kTile * 2 - kMaxQueryColumns * 5 - kThreads * 2) / 24) & ~7;
constexpr int kExactValueOffset = kExactRows * 16;  // exact stage: hit masks uint32[m][4], then float64[m], then the query's
constexpr int kExactSortedOffset = kExactValueOffset + kExactRows * 8;  // columns in ascending order (int32[128] + their positions uint8[128])
constexpr int kExactCountOffset = kExactSortedOffset + kMaxQueryColumns * 5;   // uint32[kThreads / 2]: partial rank counts
static_assert(kExactValueOffset % 8 == 0 && kExactCountOffset % 4 == 0 && kExactCountOffset + kThreads * 2 <= kTile * 2,
              "exact-stage scratch fits the tile");
static_assert(kMaxQueryColumns == 128, "two ballots cover the query's columns");
constexpr int kKeep = (kCandidates + kThreads - 1) / kThreads;  // candidate entries a thread holds while compacting
constexpr int kSelectTrigger = kCandidates - kSelectSlack;
constexpr int kWaves = kThreads / 64;
constexpr float kFixedOne = 65000.f;  // fixed-point value of the query's total IDF mass (+ n <= 128 roundings < 2^16)
constexpr int kProbeMaxK = kThreads / 4;  // threshold bootstrap from one sample per thread: k well below the sample count
static_assert(2 * kThreads <= kCandidates - kSelectSlack, "two samples per thread fit the candidate buffer");

// LDS control words
enum { kLQuery = 0, kLCount, kLOverflow, kLDigit, kLRemain, kLCoef, kLPre, kLCut, kLKth0, kLKth1, kLBad, kLItems,
       kLUnused12 /* was the single hand-over word of the map built ahead: see kLAhead */, kLNonEssential, kLMass, kLSparse, kLSigMask /* 4 words */, kLQuant = kLSigMask + 4 /* quantisation error of the query's columns, 1/65536 units */, kLEnd,
       kLStartTile = 29 /* tiles whose largest sums32 lies below the query's max_intersection_possible */,
       kLFloor = 37 /* admission floor of the candidate buffer: the largest key ever dropped for lack of room (0: none) */,
       kLAhead = 38 /* 38..39, ONE WORD PER DIRECTORY COPY: (directory serves the tile) << 31 | quads of the tile whose item map was
                       built ahead into that copy.  Written by the builder wave of tile b for tile b + 1 (copy c ^ 1) while the other
                       waves may still be reading tile b's own word (copy c) at the tile's start: like the directory it describes, a
                       word is rewritten only two barriers after its last reader (round 3 had one word for both copies: a wave that
                       left the previous tile's barrier late read the NEXT tile's total, profiles/r04_failure_causes.md (c)) */,
       kLTileMask = 32 /* 4 words: signature mask of the columns the CURRENT tile was scored without */, kLTileSkip = 36 /* their number */,
       kLStats = 24 /* 5 words: per-workgroup sums of the per-query statistics */,
       kLBytes = 30 /* 30..31: uint64, bytes this workgroup requested from global memory */ };
static_assert(kLEnd <= kLStats && kLStats + 5 <= kLBytes && kLBytes + 2 <= 32 && kLBytes % 2 == 0, "LDS control words");
static_assert(kLTileSkip < kLFloor && kLFloor < kLAhead && kLAhead + 2 <= 48, "LDS control words 32..47");

// Workgroup-uniform values read from LDS or computed on the vector ALU live in VGPRs unless the compiler is told that
// they are uniform: `uniform` moves them to scalar registers (the kernel is VGPR-bound: 128 per lane at 2 WGs/CU).
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v))); }
__device__ __forceinline__ float uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ bool uniform(bool v) { return __builtin_amdgcn_readfirstlane(v ? 1 : 0) != 0; }

__device__ __forceinline__ float round_down_positive(double x)
{
    float f = static_cast<float>(x);
    if (static_cast<double>(f) > x) f = __uint_as_float(__float_as_uint(f) - 1u);
    return f;
}

__device__ __forceinline__ float round_up_positive(double x)
{
    float f = static_cast<float>(x);
    if (static_cast<double>(f) < x) f = __uint_as_float(__float_as_uint(f) + 1u);
    return f;
}

// Inclusive prefix sum over the 64 lanes of a wave with DPP moves (no LDS crossbar round trips): Hillis-Steele
// inside each row of 16 lanes, then lane 15 of a row into the next row, then lane 31 into the upper half.
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t value, int)
{
    int v = static_cast<int>(value);
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);  // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);  // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);  // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);  // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
    return static_cast<uint32_t>(v);
}

// The workgroup's control words in LDS.  Other threads change them between barriers, so every access must reach the
// LDS -- but NOT as `volatile`: the compiler does not infer the address space of volatile accesses and emits FLAT
// loads / stores (the flat path's latency plus an `s_waitcnt vmcnt(0) lgkmcnt(0)` that drains every outstanding global
// load; three of them per tile).  Relaxed atomic loads / stores are never cached or elided either and compile to
// ds_read_b32 / ds_write_b32.  (Round 2 kept volatile accesses in the wide geometry's fast kernel, where the change
// measured 2.3 % slower; with the argument block out of the scalar registers it measures 2 % faster -- round 3.)
struct ControlWord {
    int32_t *word;
    __device__ __forceinline__ explicit ControlWord(int32_t *pointer) : word(pointer) {}
    ControlWord(const ControlWord &) = default;
    ControlWord &operator=(const ControlWord &) = delete;  // `ctrl[a] = ctrl[b]` must go through int32_t
    __device__ __forceinline__ int32_t load() const { return __atomic_load_n(word, __ATOMIC_RELAXED); }
    __device__ __forceinline__ void store(int32_t value) const { __atomic_store_n(word, value, __ATOMIC_RELAXED); }
    __device__ __forceinline__ operator int32_t() const { return load(); }
    __device__ __forceinline__ const ControlWord &operator=(int32_t value) const
    {
        store(value);
        return *this;
    }
    __device__ __forceinline__ const ControlWord &operator+=(int32_t value) const
    {
        store(load() + value);
        return *this;
    }
};
struct ControlWords {
    int32_t *words;
    __device__ __forceinline__ ControlWord operator[](int index) const { return ControlWord{words + index}; }
    __device__ __forceinline__ int32_t *at(int index) const { return words + index; }
};
using DenseControlWords = ControlWords;  // literal kernel

// k-th largest key of keys[0..m) (m >= k) by an 8-bit radix select.  All threads of the workgroup call it.
// passes = 4: the exact k-th largest key; passes = 2: its upper 16 bits with the lower ones cleared, i.e. a LOWER
// BOUND within 2^-7 relative of it -- all a running threshold needs, at half the barriers.
__device__ __forceinline__ uint32_t radix_select_kth(const uint32_t *keys, int m, int k, uint32_t *hist, ControlWords ctrl,
                                     int passes)
{
    const int tid = threadIdx.x, lane = tid & 63;
    uint32_t prefix = 0, mask = 0;
    int remaining = k;
    for (int shift = 24; shift >= 32 - 8 * passes; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < m; i += kThreads) {
            const uint32_t key = keys[i];
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {  // lane owns bins 255-4*lane .. 252-4*lane (descending)
            const int b0 = 255 - 4 * lane;
            const uint32_t c0 = hist[b0], c1 = hist[b0 - 1], c2 = hist[b0 - 2], c3 = hist[b0 - 3];
            const uint32_t local = c0 + c1 + c2 + c3;
            const uint32_t inclusive = wave_inclusive_scan(local, lane);
            const uint32_t exclusive = inclusive - local;
            const uint32_t want = static_cast<uint32_t>(remaining);
            if (want > exclusive && want <= inclusive) {
                uint32_t r = want - exclusive;
                int digit = b0;
                if (r > c0) { r -= c0; digit = b0 - 1;
                    if (r > c1) { r -= c1; digit = b0 - 2;
                        if (r > c2) { r -= c2; digit = b0 - 3; } } }
                ctrl[kLDigit] = digit;
                ctrl[kLRemain] = static_cast<int32_t>(r);
            }
        }
        __syncthreads();
        prefix |= static_cast<uint32_t>(uniform(static_cast<int>(ctrl[kLDigit]))) << shift;
        mask |= 255u << shift;
        remaining = uniform(static_cast<int>(ctrl[kLRemain]));
    }
    return prefix;
}

// Everything the scan / collect phases need to turn an approximate score into a candidate.
struct Bounds {
    float coef;      // cut / (1 + cut), rounded down: row qualifies only if s + mass >= coef * (sums + maxint32)
    float pre;       // row-independent lower bound of the right-hand side (uses min(sums))
    float mass;      // upper bound of what the skipped (non-essential) columns can add to any score
    float maxint32;
};

// largest of the eight packed 16-bit values of four words
__device__ __forceinline__ uint32_t max_of_packed8(uint4 v)
{
    typedef unsigned short packed2 __attribute__((ext_vector_type(2)));
    const packed2 a = __builtin_elementwise_max(__builtin_bit_cast(packed2, v.x), __builtin_bit_cast(packed2, v.y));
    const packed2 b = __builtin_elementwise_max(__builtin_bit_cast(packed2, v.z), __builtin_bit_cast(packed2, v.w));
    const uint32_t m = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(a, b));
    return max(m & 0xffffu, m >> 16);
}

// per 16-bit half: the largest of the four words' halves
__device__ __forceinline__ uint32_t max_of_packed4(const uint32_t (&v)[4])
{
    typedef unsigned short packed2 __attribute__((ext_vector_type(2)));
    const packed2 a = __builtin_elementwise_max(__builtin_bit_cast(packed2, v[0]), __builtin_bit_cast(packed2, v[1]));
    const packed2 b = __builtin_elementwise_max(__builtin_bit_cast(packed2, v[2]), __builtin_bit_cast(packed2, v[3]));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(a, b));
}

// Loose test: can the row still qualify if every skipped (non-essential) column matched as well?
__device__ __forceinline__ bool may_qualify(float s, float sums, const Bounds &b)
{
    return s + b.mass >= b.coef * (sums + b.maxint32);
}

// Tight test on a complete approximate score + the radix key (float32 approximate jaccard) of a candidate.
__device__ __forceinline__ bool candidate_key(float s, float sums, const Bounds &b, uint32_t &key)
{
    if (!(s >= b.coef * (sums + b.maxint32))) return false;
    const float denominator = sums + (b.maxint32 - s);
    const float approx = s / denominator;
    key = (denominator > 0.f && approx == approx) ? __float_as_uint(approx) : 0x7f800000u;
    return true;
}

// The skipped (non-essential) columns: ranks 0..count-1 of the ascending-IDF order.  Only columns that own a
// signature bit are ever skipped, so completing a score is one 16-byte load per row.
struct Skipped {
    int count;
    uint32_t sig_mask[kSignatureWords];
};

// Adds what the skipped columns contribute to a row, from its membership signature.  Approximate (order-free) like
// the scatter itself.
__device__ __forceinline__ float complete_score(float s, uint4 signature, const Skipped &skipped, const float *bit_idf)
{
    const uint32_t words[kSignatureWords] = {signature.x, signature.y, signature.z, signature.w};
#pragma unroll
    for (int w = 0; w < kSignatureWords; ++w) {
        uint32_t bits = words[w] & skipped.sig_mask[w];
        while (bits) {
            s += bit_idf[w * 32 + __ffs(bits) - 1];
            bits &= bits - 1u;
        }
    }
    return s;
}

// Packed score tile: row r lives in half (r & 1) of word r >> 1.

// Wave-aggregated append to the candidate buffer.  Must be called by all active lanes of the wave together.
__device__ __forceinline__ void append_candidate(bool pass, uint32_t key, int32_t row, uint32_t *cand_key,
                                                 int32_t *cand_row, ControlWords ctrl, int lane)
{
    const unsigned long long votes = __ballot(pass);
    if (votes == 0) return;
    const int leader = __ffsll(votes) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(ctrl.at(kLCount), __popcll(votes));
    base = __shfl(base, leader);
    if (pass) {
        const int slot = base + __popcll(votes & ((1ull << lane) - 1ull));
        if (slot < kCandidates) {
            cand_key[slot] = key;
            cand_row[slot] = row;
        } else {
            ctrl[kLOverflow] = 1;
        }
    }
}

// Debug build (-DDS_BOUNDS_CHECK): every global access of the fast kernel whose index is data dependent is checked; the
// first violation is recorded in control[24..27] (site, index low/high, limit) and the access is skipped.
#ifdef DS_BOUNDS_CHECK
__device__ __forceinline__ void record_violation(int32_t *control, int site, int64_t index, int64_t limit)
{
    if (atomicCAS(&control[24], 0, site) == 0) {
        control[25] = static_cast<int32_t>(index & 0xffffffff);
        control[26] = static_cast<int32_t>(index >> 32);
        control[27] = static_cast<int32_t>(limit & 0x7fffffff);
    }
}
__device__ __forceinline__ bool in_bounds(int32_t *control, int site, int64_t index, int64_t limit)
{
    if (index >= 0 && index < limit) return true;
    record_violation(control, site, index, limit);
    return false;
}
#define DS_OK_INDEX(site, index, limit) in_bounds(a.control, site, static_cast<int64_t>(index), static_cast<int64_t>(limit))
#else
#define DS_OK_INDEX(site, index, limit) true
#endif

// Diagnostic phase timers: thread 0 adds the shader-clock delta since its previous stamp to an LDS accumulator
// (flushed to HBM once, at the end of the kernel, so that stamping does not put a global atomic in front of a barrier).
#ifdef DS_DIAGNOSTICS
#define DS_STAMP(slot)                                                     \
    do {                                                                   \
        if (a.phase != nullptr && tid == 0) {                              \
            const unsigned long long now_ = __builtin_amdgcn_s_memtime();  \
            phase_lds[slot] += now_ - stamp_;                              \
            stamp_ = now_;                                                 \
        }                                                                  \
    } while (0)
#define DS_COUNT(slot, value)                                              \
    do {                                                                   \
        if (a.phase != nullptr && tid == 0) atomicAdd(&a.control[slot], value); \
    } while (0)
#else
#define DS_STAMP(slot) do { } while (0)
#define DS_COUNT(slot, value) do { } while (0)
#endif

// kCountBytes: the instantiation that also counts the bytes it requests from global memory (ds_index_option
// "count_bytes"; bench.py runs it once, outside the timed region).  The counting costs 3 % in this register-bound
// kernel, so the production instantiation carries none of it; both do exactly the same work on the same data.
// kSecondSample: the instantiation whose threshold bootstrap takes TWO samples per thread, launched for k between a
// quarter and a half of the workgroup's threads (top-100 in the narrow geometry); a separate instantiation because
// the extra code costs the common one 6 % (register allocation) even when it is branched around.
template <bool kCountBytes, bool kSecondSample>
__global__ __launch_bounds__(kThreads, kWorkgroupsPerCu * kThreads / 256) void ds_jaccard_topk_kernel(const void *arguments)
{
    // The arguments live in device memory and are read through the CONSTANT address space: scalar loads that can be
    // repeated where a field is needed, instead of ~48 scalar registers held (and spilled) for the kernel's whole life.
    const __attribute__((address_space(4))) JaccardArgs &a =
        *reinterpret_cast<const __attribute__((address_space(4))) JaccardArgs *>(reinterpret_cast<uintptr_t>(arguments));
#ifdef DS_DIAGNOSTICS
    unsigned long long stamp_ = a.phase != nullptr ? __builtin_amdgcn_s_memtime() : 0ull;
    __shared__ unsigned long long phase_lds[16];
    if (threadIdx.x < 16) phase_lds[threadIdx.x] = 0ull;
#endif
    extern __shared__ __align__(16) unsigned char lds[];
    uint32_t *cand_key = reinterpret_cast<uint32_t *>(lds + kOffLo);
    int32_t *cand_row = reinterpret_cast<int32_t *>(lds + kOffRow);
    int32_t *cols = reinterpret_cast<int32_t *>(lds + kOffCols);
    float *idf = reinterpret_cast<float *>(lds + kOffIdf);
    uint8_t *rank = reinterpret_cast<uint8_t *>(lds + kOffRank);     // position of column j in ascending-IDF order
    uint8_t *order = reinterpret_cast<uint8_t *>(lds + kOffOrder);   // inverse: column at position r
    float *mass_upto = reinterpret_cast<float *>(lds + kOffMass);    // [r] = IDF mass of ranks 0..r, rounded up
    int8_t *sig_bit = reinterpret_cast<int8_t *>(lds + kOffSigBit);  // signature bit of column j or -1
    float *bit_idf = reinterpret_cast<float *>(lds + kOffBitIdf);     // IDF of the query column owning signature bit g
    uint32_t *fixed = reinterpret_cast<uint32_t *>(lds + kOffFixed);  // idf[j] in the query's fixed-point scale
    uint32_t *iscores = reinterpret_cast<uint32_t *>(lds);  // score tile: 16-bit fixed-point sums, row r in half (r & 1) of word r >> 1
    // mass_low[256] (by a posting's membership bits 0..7) and mass_high[256] (by bits 8..15): the integer tables of the
    // collect sweep's row test, rebuilt after a selection.  A row's need is the tile's gate.  The lists' padding entries
    // and the idle lanes take whatever the trash word holds: the sweep tells them by their word (kPadWord), never by a table.
    uint16_t *mass_low = reinterpret_cast<uint16_t *>(lds + kOffMassTable);
    uint16_t *mass_high = mass_low + 256;
    uint32_t *ptr_cache = reinterpret_cast<uint32_t *>(lds + kOffPtr);  // [column][span + 1], kMaxQueryColumns * (kPtrTiles + 1) words
    uint32_t *quad_prefix = reinterpret_cast<uint32_t *>(lds + kOffQuadPrefix);
    uint32_t *quad_base = reinterpret_cast<uint32_t *>(lds + kOffQuadBase);
    uint2 *dir_entry = reinterpret_cast<uint2 *>(lds + kOffDirEntry);
    uint32_t *dir_mask = reinterpret_cast<uint32_t *>(lds + kOffDirMask);   // [copy][item][2]
    uint8_t *dir_count = reinterpret_cast<uint8_t *>(lds + kOffDirCount);
    uint32_t *hist = reinterpret_cast<uint32_t *>(lds + kOffHist);
    const ControlWords ctrl{reinterpret_cast<int32_t *>(lds + kOffCtrl)};

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = uniform(tid >> 6);  // a scalar: conditions on the wave's items are scalar branches, not exec masks
    const int k = a.k;
    const int64_t ptr_stride = static_cast<int64_t>(a.n_tiles) + 1;
    // The kernel arguments arrive as 16-register tuples; under register pressure the allocator spills and reloads a
    // WHOLE tuple (16 v_readlane in front of every posting load that needs one pointer of it).  The two pointers of the
    // hot loops are therefore rebuilt from scalar copies of their halves -- registers of their own, outside any tuple --
    // and keep the global address space (plain global_load, not flat_load).
    typedef const unsigned long long __attribute__((address_space(1))) *GlobalQuads;
    auto load_quad = [](GlobalQuads base, uint32_t at) {
        const unsigned long long bits = base[at];
        return make_uint2(static_cast<uint32_t>(bits), static_cast<uint32_t>(bits >> 32));
    };
    auto own_registers = [](const void *pointer) {
        const uint64_t bits = reinterpret_cast<uint64_t>(pointer);
        const uint32_t lo = uniform(static_cast<uint32_t>(bits)), hi = uniform(static_cast<uint32_t>(bits >> 32));
        return reinterpret_cast<GlobalQuads>((static_cast<uint64_t>(hi) << 32) | lo);
    };
    const GlobalQuads quads = own_registers(a.postings), sums_quads = own_registers(a.posting_sums);
    // The per-tile sums32 ranges are read at workgroup-uniform indexes and never written while the kernel runs: through the
    // CONSTANT address space they are scalar loads (scalar cache, no vector register, no vmcnt wait in front of a scatter).
    typedef const float __attribute__((address_space(4))) *ConstantFloats;
    const ConstantFloats tile_sums_min = reinterpret_cast<ConstantFloats>(reinterpret_cast<uintptr_t>(a.tile_sums_min));
    const ConstantFloats tile_sums_max = reinterpret_cast<ConstantFloats>(reinterpret_cast<uintptr_t>(a.tile_sums_max));

    for (int i = tid * 4; i < kScoreWords; i += kThreads * 4)
        *reinterpret_cast<uint4 *>(&iscores[i]) = make_uint4(0u, 0u, 0u, 0u);
    if (tid < 5) ctrl[kLStats + tid] = 0;
    if (tid < 2) ctrl[kLBytes + tid] = 0;
    __syncthreads();
    // Global-memory bytes this workgroup REQUESTS (postings, per-posting info, sums32, signatures, list pointers, the
    // exact stage's probes): the algorithmic traffic of this kernel, reported by bench.py next to the PMC counters.
    unsigned long long *requested = reinterpret_cast<unsigned long long *>(lds + kOffCtrl + kLBytes * 4);
    // The sweeps' terms are workgroup-uniform: a query's total is summed in ONE scalar register, in units of 8 bytes, and
    // thread 0 adds it to the LDS word once per query; the refinement's gathers and the exact stage's probes are added
    // where they happen.  All of it exists in the counting instantiation only.
    uint32_t query_units = 0;
    auto count_units = [&](uint32_t units) { if constexpr (kCountBytes) query_units += units; };

    for (;;) {
        if (tid == 0) {
            ctrl[kLQuery] = atomicAdd(&a.control[kCtlQueue], 1);
            ctrl[kLCount] = 0;
            ctrl[kLOverflow] = 0;
            ctrl[kLBad] = 0;
            ctrl[kLQuant] = 0;
            ctrl[kLStartTile] = 0;
            ctrl[kLFloor] = 0;
        }
        __syncthreads();
        const int64_t position = uniform(static_cast<int>(ctrl[kLQuery]));
        if (position >= a.n_queries) break;  // exit condition reached by every wave: the queue head only grows
        const int64_t q = a.take_order != nullptr ? static_cast<int64_t>(a.take_order[position]) : position;

        const int64_t qbase = a.q_rowptr[q];
        const int64_t n64 = a.q_rowptr[q + 1] - qbase;
        const double maxint = a.q_maxint[q];
        bool slow = a.literal_only != 0 || n64 > kMaxQueryColumns || n64 < 0 || !(maxint > 0.0) || !(maxint < 1e30);
        int reason = slow ? 0 : -1;  // why the query is handed to the dense kernel (diagnostics)
        const int n = slow ? 0 : static_cast<int>(n64);
        if (tid < n) {
            const int32_t column = a.q_cols[qbase + tid];
            const bool bad = column < 0 || column >= a.n_columns;
            if (bad) ctrl[kLBad] = 1;
            cols[tid] = bad ? 0 : column;
            const float value = bad ? 0.f : a.idf32[column];
            const int bit = bad ? -1 : static_cast<int>(a.sig_column[column]);
            idf[tid] = value;
            sig_bit[tid] = static_cast<int8_t>(bit);
            if (bit >= 0) bit_idf[bit] = value;
        }
        if constexpr (kCountBytes) query_units = static_cast<uint32_t>(9 * n + 24 + 7) >> 3;
        if (a.rows_sorted && !slow) {
            // The rows a query can score highest against have sums32 near its own max_intersection_possible (jaccard <=
            // min / max of the two): with the index in ascending sums32 order, that is where the sweep starts.
            int below = 0;
            const float own = static_cast<float>(maxint);
            for (int t = tid; t < a.n_tiles; t += kThreads) below += a.tile_sums_max[t] < own;
            for (int d = 32; d > 0; d >>= 1) below += __shfl_xor(below, d);
            if (lane == 0 && below) atomicAdd(ctrl.at(kLStartTile), below);
        }
        __syncthreads();
        if (uniform(static_cast<int>(ctrl[kLBad]))) {
            if (tid == 0) {
                a.status[q] = kQueryErrorArg;
                atomicAdd(&a.control[kCtlErrors], 1);
            }
            for (int j = tid; j < k; j += kThreads) a.out_rows[q * k + j] = -1;
            __syncthreads();
            continue;
        }
        if (tid >= 64 && tid < kMaxQueryColumns) quad_prefix[tid] = 0xffffffffu;  // columns 64..127: see the item map
        if (tid < 4 * kDirItems) dir_mask[tid] = 0u;  // both copies of the item directory's start bits
        // ascending-IDF order of the query's columns and the IDF mass of every prefix of that order
        if (tid < n) {
            const float mine = idf[tid];
            int r = 0;
            double below = 0.0;
#pragma unroll 8
            for (int i = 0; i < n; ++i) {  // unrolled: the LDS reads of eight steps are in flight together
                const float other = idf[i];
                const bool first = (other < mine) | ((other == mine) & (i <= tid));
                r += first & (i != tid);
                below += first ? static_cast<double>(other) : 0.0;
            }
            rank[tid] = static_cast<uint8_t>(r);
            order[r] = static_cast<uint8_t>(tid);
            mass_upto[r] = round_up_positive(below * (1.0 + 3.814697265625e-06));
        }

        const float maxint32 = static_cast<float>(maxint);
        __syncthreads();
        // Scores are accumulated in unsigned 16-bit fixed point, two rows per LDS word (LDS integer atomics run ~14x
        // faster than ds_add_f32 on gfx950 and are order-independent): one unit = total/kFixedOne where total >=
        // every reachable score.  A row's sum is at most kFixedOne + n (every term rounds by < 1 unit) < 65536, so
        // the low half of a word never carries into the high half.
        const float total_mass = uniform(n > 0 ? fmaxf(maxint32, mass_upto[n - 1]) : maxint32);
        // the error margin below assumes maxint >= the idf total of the query's columns, as match_maker.py:197 computes
        // it; a caller-supplied smaller value (C ABI) sends the query to the literal kernel
        if (!slow && n > 0 && uniform(maxint32 < mass_upto[n - 1] * 0.999f)) { slow = true; reason = 0; }
        const float to_fixed = uniform(kFixedOne / total_mass), from_fixed = uniform(total_mass * (1.f / kFixedOne));
        if (tid < kMaxQueryColumns) {
            // fixed-point image of every column's IDF and the exact total of what the quantisation can be off by
            uint32_t off = 0;
            if (tid < n) {
                const uint32_t f = max(1u, static_cast<uint32_t>(idf[tid] * to_fixed + 0.5f));
                fixed[tid] = f;
                const double unit = static_cast<double>(from_fixed);
                off = static_cast<uint32_t>(fabs(static_cast<double>(idf[tid]) - f * unit) / unit * 65536.0) + 1u;
            }
            const uint32_t total_off = wave_inclusive_scan(off, lane);
            if (lane == 63) atomicAdd(ctrl.at(kLQuant), static_cast<int32_t>(total_off));
        }
        // |approximate jaccard - exact jaccard| <= margin (DESIGN.md "error margin of the prefilter"):
        // float32 evaluation + quantisation of n terms to one unit each (4 = bound of d jaccard / d score * total)
        // float32 evaluation + the measured quantisation error of this query's columns (<= 1 unit each; typically
        // a quarter of a unit), both relative to the total mass; 4 = bound of d jaccard / d score * total
        auto error_margin = [&]() {
            const double off_units = static_cast<double>(uniform(static_cast<int>(ctrl[kLQuant]))) * (1.0 / 65536.0);
            return (6.0 * n + 64.0) * 5.9604644775390625e-08 + off_units * (4.0 / kFixedOne) * 1.001;
        };
        Bounds bounds{0.f, FLT_MIN, 0.f, maxint32};
        float cut = 0.f, pending_mass = 0.f;  // mass of the columns skipped from the NEXT tile on
        // The signature masks of the skipped columns live in LDS control words, not in scalar registers: kLSigMask as the
        // last selection left them (in force from the next tile on), kLTileMask / kLTileSkip as the CURRENT tile was scored
        // (copied at the start of the first tile after a selection); only the refinement reads them.
        if (tid < 5) ctrl[kLTileMask + tid] = 0;
        bool sparse_mode = false;  // decided at every selection from the essential columns' remaining length
        bool rebuild_mass_table = false;
        int wanted_in = 0;               // the candidate buffer overflowed with this many rows wanting in (0: it did not): the next
                                         // selection also raises the admission floor
        int floor_shift = 0;             // ... to what should fill (kSelectTrigger - 64) >> floor_shift entries: every repetition
                                         // of the same rows halves it (the rest of an epoch brings more rows)
        bool tables_fresh = false;       // the tables were rebuilt at this tile's start: mass_low[255] is read once, behind a barrier
        uint32_t mass_units_max = 0;     // mass_low[255], the largest entry: the collect sweep's gate never goes below it
        const float to_fixed_low = uniform(to_fixed * (1.f - 9.5367431640625e-07f));  // < 1 / from_fixed: products round down
        const float to_fixed_high = uniform(to_fixed * (1.f + 9.5367431640625e-07f));  // > 1 / from_fixed: products round up
        int non_essential = 0;
        bool tight = false;
        int next_select = a.select_min;
        if (next_select > kSelectTrigger) next_select = kSelectTrigger;
        int selects = 0, sparse_tiles = 0, dense_tiles = 0, last_appended = 0;
        DS_STAMP(0);

        // Rows passing the register-level tests of a sweep are RAW entries (approximate essential score, row).  A wave
        // parks them in its private LDS buffer and refines them itself, 64 at a time and always before it leaves the
        // tile: exact sums, completion of the skipped columns from the signature, tight test -- one lane per entry,
        // no workgroup barrier; only the survivors reach the shared candidate buffer.  Every raw entry is therefore
        // refined under the set of skipped columns it was scored with.
        uint32_t *wave_raw = reinterpret_cast<uint32_t *>(lds + kOffRaw) + wave * 64;
        [[maybe_unused]] uint8_t *wave_raw_tile = reinterpret_cast<uint8_t *>(lds + kOffRawTile) + wave * 64;
        int64_t raw_tile_base = 0;  // first row of the epoch the parked entries belong to (they never outlive it)
        uint32_t raw_epoch_bits = 0;  // (tile - first tile of the epoch) << kEpochShift, or'ed into every new entry
        int raw_count = 0;  // wave-uniform
        auto flush_raw = [&]() {
            if (raw_count == 0) return;
            DS_COUNT(kCtlRefines, 1);
            if constexpr (kCountBytes)  // (sums32, duplicate rank) (+ signature) of the row record per raw entry
                if (lane == 0) atomicAdd(requested, static_cast<unsigned long long>(raw_count) * (ctrl[kLTileSkip] > 0 ? 24u : 8u));
            const bool mine = lane < raw_count;
            bool ok = false;
            uint32_t key = 0;
            int32_t t = -1;
            // rows at or below the admission floor were dropped for lack of room once; admitting them now would only hide that
            const uint32_t floor_key = uniform(static_cast<uint32_t>(ctrl[kLFloor]));
            Skipped skipped;
            skipped.count = uniform(static_cast<int>(ctrl[kLTileSkip]));
#pragma unroll
            for (int w = 0; w < kSignatureWords; ++w) skipped.sig_mask[w] = uniform(static_cast<uint32_t>(ctrl[kLTileMask + w]));
            if (mine) {
                const uint32_t entry = wave_raw[lane];
                const float raw = static_cast<float>(entry >> 16) * from_fixed;
                if constexpr (kEpochInBytes) {
                    t = static_cast<int32_t>(raw_tile_base + static_cast<int64_t>(wave_raw_tile[lane]) * kTile + (entry & 0xffffu));
                } else {
                    const uint32_t low = entry & 0xffffu;
                    t = static_cast<int32_t>(raw_tile_base + static_cast<int64_t>(low >> kEpochShift) * kTile +
                                             (low & ((1u << kEpochShift) - 1u)));
                }
                if (DS_OK_INDEX(1, t, a.n_truth)) {
                    // ONE cache line per refined row: its 32-byte record holds signature, sums32 and duplicate rank
                    const uint4 *record = a.rows + 2 * static_cast<int64_t>(t);
                    const uint2 tail = *reinterpret_cast<const uint2 *>(record + 1);
                    const float sums = __uint_as_float(tail.x);
                    const uint4 signature = skipped.count > 0 ? record[0] : make_uint4(0u, 0u, 0u, 0u);
                    // a row with k or more twins (same column set, same sums32) of larger index can never be among the
                    // k largest row indexes of match_maker.py:71, and the k-th largest value does not need it either
                    const bool shadowed = static_cast<int>(tail.y) >= k;
                    // a zero score reaches this point only through the collect sweep's rounding slack (a second
                    // posting of a row whose score another lane took): never a candidate
                    if (!shadowed && raw > 0.f && may_qualify(raw, sums, bounds)) {
                        const float full = complete_score(raw, signature, skipped, bit_idf);
                        ok = candidate_key(full, sums, bounds, key) && key > floor_key;
                    }
                }
            }
#ifdef DS_DIAGNOSTICS
            if (a.phase != nullptr) {  // every wave: raw entries refined / survivors
                const unsigned long long survivors = __ballot(ok);
                if (lane == 0) {
                    atomicAdd(&a.control[kCtlRawEntries], raw_count);
                    atomicAdd(&a.control[kCtlSurvivors], __popcll(survivors));
                }
            }
#endif
            raw_count = 0;
            append_candidate(ok, key, t, cand_key, cand_row, ctrl, lane);
        };
        auto append_raw = [&](bool pass, uint32_t fixed_score, uint32_t local_row) {
            const unsigned long long votes = __ballot(pass);
            if (votes == 0) return;
            const int count = __popcll(votes);
            if (raw_count + count > 64) flush_raw();
            if (pass) {
                const int slot = raw_count + __popcll(votes & ((1ull << lane) - 1ull));
                if constexpr (kEpochInBytes) {
                    wave_raw[slot] = (fixed_score << 16) | local_row;
                    wave_raw_tile[slot] = static_cast<uint8_t>(raw_epoch_bits);
                } else {
                    wave_raw[slot] = (fixed_score << 16) | raw_epoch_bits | local_row;
                }
            }
            raw_count += count;
        };

        int sparse_retries = 0;
        uint32_t dir_copy = 0;  // which copy of the item directory the current tile uses; flips with every tile that is processed
        // What the END of a sparse tile prepares for the next one (same epoch, same list-pointer block): its item directory
        // in the other copy and the posting quads of this wave's first round, requested before the barrier that ends the
        // tile -- their latency passes while the wave waits there and starts the next tile.
        constexpr int kRound = 3;
        bool ahead = false;  // workgroup-uniform: the previous tile built this tile's item map
        // the registers of a wave's round (quads, per-posting info, fixed-point IDF, lane has a quad)
        uint2 quad[kRound], quad_info[kRound];
        uint32_t quad_value[kRound];
        bool live[kRound];  // a wave without items still runs the collect sweep
#pragma unroll
        for (int u = 0; u < kRound; ++u) {
            quad[u] = quad_info[u] = make_uint2(0u, 0u);
            quad_value[u] = 0u;
            live[u] = false;
        }
        // The list pointers of the query's columns are cached in LDS for `span` tiles at a time: as many as the cache
        // holds for this query's number of columns (all 18 tiles of C2 for a query of up to 26 columns), so that the
        // reload -- an exposed global latency between two barriers -- happens rarely.
        const int span = n > 0 ? min(a.n_tiles, max(kPtrTiles, kMaxQueryColumns * (kPtrTiles + 1) / n - 1)) : kPtrTiles;
        int block_start = 0, block_end = 0;
        // Order of the tiles.  An epoch is a run of consecutive tiles [epoch_start, epoch_last] visited in ascending order (one
        // tile while tiles are dense).  With the rows in sums32 order the epochs start at the query's own sums32 and ascend
        // until the tiles' smallest sums32 is out of the threshold's reach (jaccard <= min(sums, maxint) / max(sums,
        // maxint) < cut), then descend from below the start tile, nearest epoch first, until the tiles' largest sums32 is.
        const bool sorted = a.rows_sorted != 0;
        const int start_tile = sorted ? min(uniform(static_cast<int>(ctrl[kLStartTile])), a.n_tiles - 1) : 0;
        int epoch_start = start_tile, epoch_last = start_tile;  // the current epoch
        int down_next = start_tile - 1;                          // last tile of the next descending epoch
        int up_next = start_tile + 1;                            // first tile of the next ascending epoch
        bool descending = false;
        int run_left = 0;  // epochs left before the sweep changes sides (it alternates in runs of one list-pointer block)
        // Epochs of sparse tiles have a fixed length, kEpochTiles.  Measured and NOT adopted in round 4 (profiles/r04_tuning.txt, batches
        // 10-11; the experiments are diffs in profiles/, not paths in this kernel): a ramp 1, 2, 4 of the length (top-100 redos 52,995
        // -> 23,969 per 100,000 queries, but the extra epoch ends cost more than the redos wherever k is small); an overflowing epoch
        // redone by halves (redo count unchanged, +1..2 %); adaptive lengths in the large-k instantiation only (redos -60 %, fast kernel
        // -1.8 %, but one or two queries per launch then end as "ties" on the literal kernel: the step does not move).
        int b = start_tile;
        while (!slow) {
            bool redo_tile = false;
            const float tile_min = tile_sums_min[b];  // scalar load, consumed behind the scatter
            if (__builtin_expect(b < block_start || b >= block_end, 0)) {  // list pointers of the next `span` tiles: one coalesced burst
                // ascending epochs: the block starts at this tile; descending epochs: it ENDS with the epoch, so that the
                // epochs below it are cached as well
                block_start = descending ? max(0, min(b, epoch_last - span + 1)) : b;  // (a block shorter than the epoch starts at the tile)
                block_end = block_start + span;
                __syncthreads();
                const int width = min(span, a.n_tiles - block_start) + 1;
                for (int e = tid; e < n * (span + 1); e += kThreads) {
                    const int j = e / (span + 1), i = e - j * (span + 1);
                    ptr_cache[e] = (i < width && DS_OK_INDEX(2, static_cast<int64_t>(cols[j]) * ptr_stride + block_start + i,
                                                            a.n_columns * ptr_stride))
                                       ? a.col_ptr[static_cast<int64_t>(cols[j]) * ptr_stride + block_start + i]
                                       : 0u;
                }
                count_units(static_cast<uint32_t>(n * width + 1) >> 1);
                __syncthreads();
            }
            const int bt = b - block_start;
            bounds.mass = pending_mass;  // what this tile's scores do NOT contain; fixed until the tile is done
            if (__builtin_expect(rebuild_mass_table, 0)) {  // used by the exchange sweep, i.e. after the barrier that ends the scatter
                rebuild_mass_table = false;
                tables_fresh = true;
                // the masks of the last selection are in force from this tile on (every use of the copy -- the refinement --
                // lies behind at least one barrier of this tile)
                if (tid < 4) ctrl[kLTileMask + tid] = static_cast<int32_t>(ctrl[kLSigMask + tid]);  // (an int32: word = word would copy the accessor)
                if (tid == 4) ctrl[kLTileSkip] = non_essential;
                if (tid < 256) {
                    const uint32_t skipped16 = static_cast<uint32_t>(ctrl[kLSigMask]) & 0xffffu;
                    // A posting carries its row's signature bits 0..15.  The collect sweep tests rows in the integer domain of
                    // the fixed-point scores, the tile's gate being every row's need:
                    //   score + mass_low[bits 0..7] - mass_high[bits 8..15] >= tile gate
                    // mass_low[x]  = the full skipped mass (rounded up, the skipped columns beyond bit 15 counted as held) minus
                    //                the skipped columns of bits 0..7 that x does NOT hold (rounded down),
                    // mass_high[x] = the skipped columns of bits 8..15 that x does NOT hold (rounded down).
                    // Both tables count what a row LACKS, so every entry shares the slack of the largest one, mass_low[255] (a
                    // row that holds everything): when the gate has to be raised to that entry, the test turns into "score >=
                    // what the row lacks", which still rejects only rows below the full mass (< pre).  No entry is capped.
                    // Single precision throughout: the sums are off by < 8 roundings of terms <= the full mass, which the
                    // factor covers; the unit conversions go through to_fixed_high / to_fixed_low, which over- and undercut
                    // 1 / from_fixed by more than the roundings of the products (no fp64, no divisions).  The rows that pass
                    // are a superset of those of `passes`.
                    float lacks_low = 0.f, lacks_high = 0.f;
                    for (int g = 0; g < 8; ++g) {
                        if (((skipped16 >> g) & 1u) && !((tid >> g) & 1)) lacks_low += bit_idf[g];
                        if (((skipped16 >> (g + 8)) & 1u) && !((tid >> g) & 1)) lacks_high += bit_idf[g + 8];
                    }
                    const float full_units = bounds.mass * to_fixed_high + 2.5f;
                    const uint32_t full = static_cast<uint32_t>(full_units < 65535.f ? full_units : 65535.f);
                    const uint32_t low = static_cast<uint32_t>(lacks_low * (1.f - 3.814697265625e-06f) * to_fixed_low);
                    const uint32_t high = static_cast<uint32_t>(lacks_high * (1.f - 3.814697265625e-06f) * to_fixed_low);
                    mass_low[tid] = static_cast<uint16_t>(full - min(low, full));
                    mass_high[tid] = static_cast<uint16_t>(min(high, 65535u));
                }
            }
            const bool sparse = tight && sparse_mode;
            // ---- work items of this tile.  The essential columns' posting quads of the tile form ONE sequence (column after
            // column); an item is 64 consecutive quads of it, so every lane of an item has a quad to work on whatever
            // the lengths of the single lists (items of one list each were 76 % full on C2).  Every wave computes the
            // same exclusive prefix of the lists' quad counts (lane j: columns j and j + 64, DPP scan) and writes it to
            // LDS -- all eight waves write the same values, a wave only ever reads what its own lanes wrote -- and a
            // lane finds the column of its quad by a branch-free binary search there: no ballots, no v_readlane, no
            // scalar instructions per item.
            // build_map(bt, copy, zero_other): the item map of tile `bt` of the pointer block into directory copy `copy`;
            // returns the tile's quads and whether the directory serves it (otherwise the prefix arrays of the binary
            // search were written -- there is ONE copy of those, so only the tile's own start may build them).
            auto build_map = [&](int tile_bt, uint32_t copy, bool at_start, bool &directory) {
                uint32_t *const mask = dir_mask + copy * (2 * kDirItems);
                if (!at_start) {  // built ahead by one wave: it zeroes the copy's start bits itself, in order with its ORs
                    mask[lane] = 0u;
                    mask[64 + lane] = 0u;
                }
                uint2 *const entry = dir_entry + copy * kDirColumns;
                uint8_t *const count = dir_count + copy * kDirItems;
                uint32_t quads_of[2] = {0u, 0u}, begin_of[2] = {0u, 0u};
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int j = lane + 64 * h;
                    if (j < n && rank[j] >= non_essential) {
                        begin_of[h] = ptr_cache[j * (span + 1) + tile_bt];
                        quads_of[h] = ptr_cache[j * (span + 1) + tile_bt + 1] - begin_of[h];
                    }
                }
                const uint32_t scan0 = wave_inclusive_scan(quads_of[0], lane);
                uint32_t total = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(scan0), 63));
                const uint32_t before0 = scan0 - quads_of[0];
                uint32_t before1 = 0;
                const unsigned long long started0 = __ballot(quads_of[0] != 0u);
                unsigned long long started1 = 0ull;
                if (n > 64) {
                    const uint32_t scan1 = wave_inclusive_scan(quads_of[1], lane);
                    before1 = total + scan1 - quads_of[1];
                    total += static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(scan1), 63));
                    started1 = __ballot(quads_of[1] != 0u);
                }
                const int lists0 = __popcll(started0), lists = lists0 + __popcll(started1);
                directory = total <= static_cast<uint32_t>(kDirItems * 64) && lists <= kDirColumns;
                if (directory) {
                    // every wave writes the same entries and ORs the same bits; a wave reads what its own lanes wrote
                    const uint32_t below0 = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(started0 >> 32),
                                                                      __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(started0), 0u));
                    if (quads_of[0] != 0u) {
                        entry[below0] = make_uint2(begin_of[0] - before0, fixed[lane]);
                        atomicOr(&mask[(before0 >> 6) * 2 + ((before0 >> 5) & 1u)], 1u << (before0 & 31u));
                    }
                    if (n > 64) {
                        const uint32_t below1 = lists0 + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(started1 >> 32),
                                                                                   __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(started1), 0u));
                        if (quads_of[1] != 0u) {
                            entry[below1] = make_uint2(begin_of[1] - before1, fixed[lane + 64]);
                            atomicOr(&mask[(before1 >> 6) * 2 + ((before1 >> 5) & 1u)], 1u << (before1 & 31u));
                        }
                    }
                    // lists that start before item `lane`: exclusive scan of the items' start-bit counts
                    const uint2 bits = *reinterpret_cast<const uint2 *>(&mask[2 * lane]);
                    const uint32_t starts = static_cast<uint32_t>(__popc(bits.x) + __popc(bits.y));
                    count[lane] = static_cast<uint8_t>(wave_inclusive_scan(starts, lane) - starts);
                } else if (at_start) {
                    quad_prefix[lane] = lane < n ? before0 : 0xffffffffu;  // columns beyond the query's: never found
                    quad_base[lane] = begin_of[0] - before0;
                    if (n > 64) {
                        quad_prefix[lane + 64] = lane + 64 < n ? before1 : 0xffffffffu;
                        quad_base[lane + 64] = begin_of[1] - before1;
                    }
                }
                return total;
            };
            // (this lane's quad, fixed-point IDF of its column) of work item `at` of a tile of `total` quads whose map is in
            // copy `copy`; false beyond the last quad.  Directory: two LDS round trips (start bits + count of the item,
            // then the list's entry); tiles beyond the directory's limits -- in practice the dense first tile -- take the
            // branch-free binary search.
            auto locate_in = [&](uint32_t copy, bool directory, uint32_t total, int at, uint32_t &first, uint32_t &value) {
                const uint32_t g = static_cast<uint32_t>(at) * 64u + lane;
                if (directory) {
                    const uint2 bits = *reinterpret_cast<const uint2 *>(&dir_mask[copy * (2 * kDirItems) + 2 * at]);
                    const uint32_t before = dir_count[copy * kDirItems + at];
                    const uint32_t below = __builtin_amdgcn_mbcnt_hi(bits.y, __builtin_amdgcn_mbcnt_lo(bits.x, 0u));
                    const uint32_t own = ((lane < 32 ? bits.x : bits.y) >> (lane & 31)) & 1u;
                    const uint2 entry = dir_entry[copy * kDirColumns + ((before + below + own - 1u) & (kDirColumns - 1))];
                    first = entry.x + g;
                    value = entry.y;
                } else {
                    uint32_t c = 0;
#pragma unroll
                    for (uint32_t bit = kMaxQueryColumns / 2; bit > 0; bit >>= 1) {  // largest c with quad_prefix[c] <= g
                        const uint32_t t = c + bit;
                        c = quad_prefix[t] <= g ? t : c;
                    }
                    first = quad_base[c] + g;
                    value = fixed[c];
                }
                return g < total;
            };
            // one round of this wave's items of a tile: locate, request the quads (and, for the round the collect sweep
            // keeps, the per-posting info)
            auto request_round = [&](uint32_t copy, bool directory, uint32_t total, int items, int round, bool keep,
                                     bool count_sparse, uint2 (&q)[kRound], uint2 (&info)[kRound], uint32_t (&value)[kRound],
                                     bool (&alive)[kRound]) {
#pragma unroll
                for (int u = 0; u < kRound; ++u) {
                    const int at = wave + (round + u) * kWaves;
                    uint32_t first = 0;
                    value[u] = 0;
                    alive[u] = at < items && locate_in(copy, directory, total, at, first, value[u]) &&
                               DS_OK_INDEX(3, first, a.n_quads);
                    q[u] = alive[u] ? load_quad(quads, first) : make_uint2(kPadQuad, kPadQuad);
                    if (keep)  // idle lanes carry the padding quad: the collect sweep's test turns its word away
                        info[u] = alive[u] ? load_quad(sums_quads, first) : make_uint2(0u, 0u);
                    if constexpr (kCountBytes) {  // 8 bytes per quad, 8 more for the row info of a kept round
                        const unsigned long long loaded = __ballot(alive[u]);
                        if (count_sparse && lane == 0)
                            atomicAdd(requested, static_cast<unsigned long long>(__popcll(loaded)) * (keep ? 16u : 8u));
                    }
                }
            };
            raw_tile_base = static_cast<int64_t>(epoch_start) * kTile;
            raw_epoch_bits = kEpochInBytes ? static_cast<uint32_t>(b - epoch_start)
                                           : static_cast<uint32_t>(b - epoch_start) << (kEpochShift & 15);
            const bool epoch_end = b >= epoch_last;
            // The NEXT tile's item map is built while this tile's posting quads are on their way (below) when the next tile
            // belongs to the same epoch -- same thresholds, same essential columns -- and its list pointers are cached:
            // by ONE wave (the waves take turns), into the other copy of the directory.
            const bool map_ahead = !epoch_end && b + 1 < block_end;
            const uint32_t tile_copy = dir_copy;
            if (!map_ahead) {
                // Nobody builds ahead in this tile: the other copy's start bits are zeroed for whoever builds the next
                // tile's map at its start.  Every wave is past its last read of them (a barrier ended the tile that used
                // them) and nobody ORs into them before this tile's barriers.  (A wave that builds ahead zeroes them
                // itself: one writer.)
                uint32_t *const other = dir_mask + (tile_copy ^ 1u) * (2 * kDirItems);
                other[lane] = 0u;
                other[64 + lane] = 0u;
            }
            bool use_directory = false;
            uint32_t total_quads = 0;
            if (ahead) {  // the previous tile built this tile's map into this tile's copy: (quads, served by the directory?)
                // ONE word per copy: bit 31 = the directory serves the tile, below it the tile's quads (one LDS round trip at
                // tile start).  This tile's builder writes the OTHER copy's word, so a wave that arrives here late still
                // finds its own tile's value.
                const uint32_t built = uniform(static_cast<uint32_t>(ctrl[kLAhead + static_cast<int>(tile_copy)]));
                total_quads = built & 0x7fffffffu;
                use_directory = (built >> 31) != 0u;
#ifdef DS_BOUNDS_CHECK
                {   // the hand-over itself is checked: the total recomputed from the cached list pointers of THIS tile (site 11)
                    uint32_t mine = 0;
                    for (int j = lane; j < n; j += 64)
                        if (rank[j] >= non_essential) mine += ptr_cache[j * (span + 1) + bt + 1] - ptr_cache[j * (span + 1) + bt];
                    for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d);
                    if (mine != total_quads) record_violation(a.control, 11, static_cast<int64_t>(total_quads), static_cast<int64_t>(mine));  // (handed over, recomputed)
                }
#endif
            }
            if (!use_directory) total_quads = build_map(bt, tile_copy, true, use_directory);
            ahead = map_ahead;
            dir_copy ^= 1u;
            const int n_items = static_cast<int>((total_quads + 63u) >> 6);
            auto locate = [&](int at, uint32_t &first, uint32_t &value) {
                return locate_in(tile_copy, use_directory, total_quads, at, first, value);
            };
            if constexpr (kCountBytes) {  // posting bytes of a dense tile: 8 per quad (a sparse tile's are counted where they are loaded)
                if (!sparse) count_units(total_quads);
            }
            DS_STAMP(1);

            const int64_t tile_base = static_cast<int64_t>(b) * kTile;
            // read here, where a barrier (end of the scatter) separates every thread's read from the next append (a sparse
            // tile has no use for it: one LDS round trip less in front of its scatter)
            int count_at_step = sparse ? 0 : uniform(static_cast<int>(ctrl[kLCount]));
            // row-independent gate of this tile: coef * (min sums of the tile + maxint), rounded down
            Bounds here = bounds;  // (+ the tile's own gate, computed behind the scatter: nothing in front of it needs it)
            // A sweep only runs the register-level tests and appends RAW entries (approximate essential score, row);
            // the wave refines them (flush_raw) before it leaves the tile.
            // branch-free on purpose: short-circuit evaluation would put every LDS read of the caller behind its own
            // exec-masked branch and wait for each one separately
            auto passes = [&](float s, float sums_lower_bound, float row_mass) {
                return (s > 0.f) & (s + row_mass >= here.pre) &
                       (s + row_mass >= here.coef * (sums_lower_bound + here.maxint32));
            };
            // four rows at a time: one ballot decides whether anything needs appending (the common case: nothing)
            auto consider4 = [&](const uint32_t (&fixed_score)[4], const uint32_t (&local)[4],
                                 const float (&sums_lower_bound)[4], const float (&row_mass)[4]) {
                bool pass[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    pass[e] = passes(static_cast<float>(fixed_score[e]) * from_fixed, sums_lower_bound[e], row_mass[e]);
                if (__ballot(pass[0] || pass[1] || pass[2] || pass[3]) == 0) return;
#pragma unroll
                for (int e = 0; e < 4; ++e) append_raw(pass[e], fixed_score[e], local[e]);
            };

            // ---- (1) scatter: fixed-point LDS atomics; padding entries hit the trash word.  Wave w takes the items
            // w, w + kWaves, ...: four of them (one quad per lane each) are in flight at a time.  On a sparse tile whose
            // the quads (and the per-posting info) of a wave's LAST round stay in registers for the collect sweep -- all of a
            // tile whose items fit one round; the earlier rounds of a longer tile are located and loaded again.
            int kept_round = 0;  // first item index (in units of kWaves) of the round the registers hold
#pragma unroll
            for (int u = 0; u < kRound; ++u) live[u] = false;
            const int count_before = count_at_step;
            for (int round = 0; wave + round * kWaves < n_items; round += kRound) {
                const bool keep = sparse && wave + (round + kRound) * kWaves >= n_items;  // this wave's last round
                kept_round = round;
                request_round(tile_copy, use_directory, total_quads, n_items, round, keep, sparse, quad, quad_info, quad_value, live);
                if (map_ahead && round == 0 && wave == (b & (kWaves - 1))) {
                    bool directory;
                    const uint32_t total = build_map(bt + 1, tile_copy ^ 1u, false, directory);
                    if (lane == 0) {
                        ctrl[kLAhead + static_cast<int>(tile_copy ^ 1u)] = static_cast<int32_t>(total | (directory ? 0x80000000u : 0u));
                    }
                }
                if (sparse) DS_STAMP(10);  // diagnostics: items located, loads requested
#pragma unroll
                for (int u = 0; u < kRound; ++u) {
                    // exec-masked on purpose: unconditional atomics of idle lanes on trash words measured slower
                    // (30.3 against 29.8 ms, profiles/r02_tuning.txt)
                    if (!live[u]) continue;
                    const uint32_t shifted = quad_value[u] << ((quad[u].x >> 11) & 16u);  // the quad's half: bit 15 of any posting
                    atomicAdd(&iscores[quad[u].x & 0x7fffu], shifted);
                    atomicAdd(&iscores[(quad[u].x >> 16) & 0x7fffu], shifted);
                    atomicAdd(&iscores[quad[u].y & 0x7fffu], shifted);
                    atomicAdd(&iscores[(quad[u].y >> 16) & 0x7fffu], shifted);
                }
            }
            if (map_ahead && wave >= n_items && wave == (b & (kWaves - 1))) {  // the builder had no item in this tile
                bool directory;
                const uint32_t total = build_map(bt + 1, tile_copy ^ 1u, false, directory);
                if (lane == 0) {
                    ctrl[kLAhead + static_cast<int>(tile_copy ^ 1u)] = static_cast<int32_t>(total | (directory ? 0x80000000u : 0u));
                }
            }
            if (sparse) DS_STAMP(15);  // diagnostics: the scatter loop of thread 0's wave; slot 6 is then the wait at the barrier
            __syncthreads();
            DS_STAMP(sparse ? 6 : 2);
            {
                const float gate = uniform(bounds.coef * (tile_min + maxint32) * (1.f - 3.814697265625e-06f));
                if (gate > here.pre) here.pre = gate;
            }

            if (sparse) {
                // ---- (2s) collect sweep over the same postings: the first lane to reach a row takes its score and
                // leaves zero behind (no scan of the whole tile)
                ++sparse_tiles;
                // Cheap integer pre-test on the taken fixed-point scores: a row can only pass `s + mass >= pre` if its
                // score reaches (pre - mass) in fixed-point units (rounded down, minus slack: a superset of the float
                // test).  Most quads have no such row and skip the per-row decoding and table lookups altogether.
                // A row whose score is zero here (another posting of the row took it first) has nothing but its mass entry:
                // the gate is kept at or above the largest one (mass_low[255]) so that such a row fails `have >= need` without a
                // test of its own.  (It can still pass when it owns every skipped column AND the gate had to be
                // raised, i.e. pre - mass is within the tables' 4 units of rounding slack; the refinement rejects it.)
                if (__builtin_expect(tables_fresh, 0)) {
                    tables_fresh = false;
                    mass_units_max = uniform(static_cast<uint32_t>(mass_low[255]));
                }
                const uint32_t gate_fixed = [&]() {  // the tile's row-independent bound `here.pre`, rounded down (float32:
                    // to_fixed_low undercuts 1 / from_fixed by more than the roundings of the product)
                    const float units = here.pre * to_fixed_low - 2.f;
                    const uint32_t gate = units > 0.f ? static_cast<uint32_t>(units) : 0u;
                    return max(gate, mass_units_max);
                }();
                auto collect = [&]() {
#pragma unroll
                    for (int u = 0; u < kRound; ++u) {
                        if (__ballot(live[u]) == 0) continue;
                        const uint32_t word[4] = {quad[u].x & 0x7fffu, (quad[u].x >> 16) & 0x7fffu, quad[u].y & 0x7fffu,
                                                  (quad[u].y >> 16) & 0x7fffu};
                        const uint32_t shift = (quad[u].x >> 11) & 16u;  // the quad's half
                        const uint32_t info[4] = {quad_info[u].x & 0xffffu, quad_info[u].x >> 16, quad_info[u].y & 0xffffu,
                                                  quad_info[u].y >> 16};
                        // pass <=> score + mass_low - mass_high >= gate <=> score >= gate - mass_low + mass_high (>= 0: see the gate).  (Rounds 2-3 issued the
                        // eight table look-ups of a quad in FRONT of its atomics, for every quad; batching a round's twelve
                        // atomics on top of the two-level test gained nothing: profiles/r04_tuning.txt.)
                        uint32_t least[4];
                        uint32_t taken[4];
                        // the four atomics of a quad are issued back to back and their results extracted afterwards
                        // (extraction inside the same branch would wait for every atomic separately)
                        uint32_t before[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) before[e] = 0u;
                        if (live[u]) {
                            // ONE exec-masked region per quad (idle lanes stay off the LDS); the padding entries of a
                            // list's last quad take from the trash word instead of being branched around one by one
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                before[e] = atomicAnd(&iscores[word[e]], ~(0xffffu << shift));
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) taken[e] = (before[e] >> shift) & 0xffffu;
#ifdef DS_DIAGNOSTICS
                        if (a.phase != nullptr) {  // selectivity of the row-independent gate, counted in FRONT of it (every wave-quad)
                            int touched = 0, level1 = 0;
                            for (int e = 0; e < 4; ++e) {
                                touched += taken[e] != 0u;
                                level1 += taken[e] != 0u && taken[e] + mass_units_max >= gate_fixed;
                            }
                            for (int d = 32; d > 0; d >>= 1) { touched += __shfl_xor(touched, d); level1 += __shfl_xor(level1, d); }
                            if (lane == 0) { atomicAdd(&a.control[20], touched); atomicAdd(&a.control[21], level1);
                                             atomicAdd(&a.control[22], 1); atomicAdd(&a.control[23], level1 != 0); }
                        }
#endif
                        // Level 1, no look-up: every entry of the two tables is bounded by the gate and the largest mass
                        // (least[e] >= gate_fixed - mass_low[255]), so a quad whose four scores all stay below that bound has
                        // no row for the exact test.  With the rows in sums32 order the tile's gate is sharp: 73 % (C2) /
                        // 83 % (C5 shape) of the wave-quads end here (diagnostics build, profiles/r04_phase_table_*).
                        // (the largest of the four by packed 16-bit maxima of the words as the atomics returned them, then the
                        // quad's half of the result: the single scores are only extracted for the quads that pass)
                        if (__ballot(((max_of_packed4(before) >> shift) & 0xffffu) >= gate_fixed - mass_units_max) == 0) continue;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            least[e] = gate_fixed - mass_low[info[e] & 0xffu] + mass_high[info[e] >> 8];
                        bool pass[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e)  // padding entries and idle lanes (the trash word's score is not zero): never; zero scores: see the gate
                            pass[e] = (taken[e] >= least[e]) & (word[e] != kPadWord);
                        if (__ballot(pass[0] | pass[1] | pass[2] | pass[3]) == 0) continue;
#pragma unroll
                        for (int e = 0; e < 4; ++e) append_raw(pass[e], taken[e], (word[e] << 1) | (shift >> 4));
                    }
                };
                collect();  // the wave's last round, still in registers
                for (int round = 0; round < kept_round; round += kRound) {  // the earlier ones
#pragma unroll
                    for (int u = 0; u < kRound; ++u) {
                        const int at = wave + (round + u) * kWaves;
                        uint32_t first = 0, value = 0;
                        live[u] = at < n_items && locate(at, first, value) && DS_OK_INDEX(3, first, a.n_quads);
                        quad[u] = live[u] ? load_quad(quads, first) : make_uint2(kPadQuad, kPadQuad);
                        quad_info[u] = live[u] ? load_quad(sums_quads, first) : make_uint2(0u, 0u);
                        if constexpr (kCountBytes) {
                            const unsigned long long loaded = __ballot(live[u]);
                            if (lane == 0) atomicAdd(requested, static_cast<unsigned long long>(__popcll(loaded)) * 16u);
                        }
                    }
                    collect();
                }
                DS_STAMP(13);  // diagnostics: the sweep itself (thread 0's wave) ...
                if (epoch_end) flush_raw();
                DS_STAMP(14);  // ... its refinement gathers ...
                __syncthreads();
                DS_STAMP(7);   // ... and the wait for the other waves at the barrier
                if (__builtin_expect(uniform(static_cast<int>(ctrl[kLOverflow])) != 0, 0)) {
                    // The sweep ran to its end, so the tile is all zero again, but some of its rows did not fit the
                    // buffer: tighten the threshold with what is buffered, drop this tile's entries and process the
                    // tile once more.
                    if (++sparse_retries > 5) { slow = true; reason = 2; break; }
                    wanted_in = uniform(static_cast<int>(ctrl[kLCount]));  // appends count on beyond the capacity
                    floor_shift = min(sparse_retries - 1, 3);
                    __syncthreads();
                    if (tid == 0) {
                        ctrl[kLCount] = kCandidates;
                        ctrl[kLOverflow] = 0;
                        atomicAdd(&a.control[kCtlRedos], 1);  // rare path: straight to HBM (ds_jaccard_sync stats[31])
                    }
                    if (tid < 2 * kDirItems) dir_mask[dir_copy * (2 * kDirItems) + tid] = 0u;  // a directory built ahead is dropped
                    ahead = false;
                    __syncthreads();
                    redo_tile = true;
                    raw_count = 0;  // entries still parked belong to the tiles that are processed again
                } else {
                    if (epoch_end) sparse_retries = 0;  // only a whole epoch without overflow ends a series of retries
                    DS_COUNT(kCtlRawSparse, ctrl[kLCount] - count_before);
                    if (!epoch_end) {  // the common case, spelled out: nothing below concerns a sparse tile inside its epoch
                        ++b;
                        continue;
                    }
                }
            }

            // ---- (2d) dense scan (and re-zero) of the tile; in steps while no running value exists
            const int64_t rows_left = a.n_truth - tile_base;
            const int limit = rows_left >= kTile ? kTile : static_cast<int>((rows_left + 7) & ~int64_t(7));
            int r0 = sparse ? limit : 0;
            if (!sparse) ++dense_tiles;
            bool select_now = sparse && (redo_tile || (epoch_end && uniform(static_cast<int>(ctrl[kLCount])) >= next_select));
            int retries = 0;
            bool probed = false;
            // rows to drop at the next pruning (rows that are scanned / collected again)
            int32_t drop_lo = redo_tile ? static_cast<int32_t>(raw_tile_base) : 0;  // the whole epoch is processed again
            int32_t drop_hi = redo_tile ? static_cast<int32_t>(tile_base + kTile) : 0;
            bool force_pending = redo_tile;
            while (r0 < limit || select_now) {
                bool force_select = force_pending;
                force_pending = false;
                if (r0 < limit && !tight && !probed && k <= (kSecondSample ? 2 : 1) * kProbeMaxK && count_at_step == 0) {
                    // ---- threshold bootstrap.  No threshold yet and nothing buffered: instead of flooding the
                    // candidate buffer with every positive row, each thread picks the best of its 32 rows of this
                    // tile (cross-multiplied comparison, no division) and contributes that row's key as a SAMPLE
                    // (row = -1: dropped by the compaction below).  The k-th largest of the kThreads samples is the
                    // k-th largest value of a subset of the rows, i.e. a valid lower estimate of the final k-th.
                    probed = true;
                    // No row's sums32 is read: with the tile's LARGEST sums32 in its place (the rows are in sums32 order: a
                    // tile's range is narrow) a row's value is still a lower estimate, and the best row is the best score.
                    const float tile_max = tile_sums_max[b];
                    uint32_t best_fixed = 0u;
                    [[maybe_unused]] int best_group = -1;  // kSecondSample: the 8-row group the first sample came from
                    for (int idx = tid * 8; idx < limit; idx += kThreads * 8) {
                        const uint4 raw4 = *reinterpret_cast<uint4 *>(&iscores[idx >> 1]);
                        const uint32_t words[4] = {raw4.x, raw4.y, raw4.z, raw4.w};
                        if constexpr (kSecondSample) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                const uint32_t fx = (words[e >> 1] >> ((e & 1) * 16)) & 0xffffu;
                                if (fx > best_fixed) {
                                    best_fixed = fx;
                                    best_group = idx;
                                }
                            }
                        } else {
                            best_fixed = max(best_fixed, max_of_packed8(raw4));  // three packed 16-bit maxima + one of the halves
                        }
                    }
                    const float best_s = static_cast<float>(best_fixed) * from_fixed;
                    uint32_t sample = 0u;
                    if (best_s > 0.f && !candidate_key(best_s, tile_max, bounds, sample)) sample = 0u;
                    cand_key[tid] = sample;
                    cand_row[tid] = -1;
                    if constexpr (kSecondSample) {
                        // second sample: the best row among the thread's rows OTHER than the first sample's 8-row group
                        uint32_t second_fixed = 0u;
                        for (int idx = tid * 8; idx < limit; idx += kThreads * 8) {
                            if (idx == best_group) continue;
                            const uint4 raw4 = *reinterpret_cast<uint4 *>(&iscores[idx >> 1]);
                            const uint32_t words[4] = {raw4.x, raw4.y, raw4.z, raw4.w};
#pragma unroll
                            for (int e = 0; e < 8; ++e) second_fixed = max(second_fixed, (words[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
                        }
                        const float second_s = static_cast<float>(second_fixed) * from_fixed;
                        uint32_t second = 0u;
                        if (second_s > 0.f && !candidate_key(second_s, tile_max, bounds, second)) second = 0u;
                        cand_key[tid + kThreads] = second;
                        cand_row[tid + kThreads] = -1;
                    }
                    if (tid == 0) ctrl[kLCount] = (kSecondSample ? 2 : 1) * kThreads;
                    __syncthreads();
                    force_select = true;
                    DS_STAMP(11);
                } else if (r0 < limit) {
                    // no running value yet: 512-row steps; afterwards the whole rest of the tile.  The scores of a step
                    // are zeroed only once the step has fitted into the candidate buffer: if a flood of rows above a
                    // still weak threshold overflows it, the step is undone, the threshold is tightened from what is
                    // already buffered, and the same rows are scanned again.
                    const int r1 = limit;
                    // a flood is only to be expected while there is no threshold, while it is young, or when the last
                    // step appended a lot; otherwise zero on the fly (one LDS pass and one barrier less) and treat an
                    // overflow as fatal.  Without a threshold every positive row is appended: a tile with more than
                    // a buffer's worth of them overflows once, which yields a threshold from ~1800 samples.
                    // (round 3: always.  With the rows in sums32 order the tiles around a query's start tile hold its strongest
                    // candidates: a flood can come at any time, and with the admission floor every overflow is recoverable.)
                    constexpr bool recoverable = true;
                    // A thread reads eight rows (one uint4 of packed scores) per iteration.
                    constexpr int kBatch = 1;
                    // the trip count is workgroup-uniform (a wave keeps all its lanes through the loop: the raw-entry
                    // buffer is addressed by lane); rows beyond the tile's end are masked by `valid`
                    // no row whose fixed-point score lies below this can satisfy score + mass >= pre (mass < pre by construction
                    // once a threshold exists, so untouched rows -- score 0 -- never pass then)
                    const float any_units = uniform((here.pre - here.mass) * to_fixed_low - 1.f);
                    const uint32_t any_fixed = any_units > 0.f ? static_cast<uint32_t>(any_units < 65535.f ? any_units : 65535.f) : 0u;
                    const int scan_steps = (r1 - r0 + kBatch * kThreads * 8 - 1) / (kBatch * kThreads * 8);
                    for (int step = 0; step < scan_steps; ++step) {
                        const int base = r0 + tid * 8 + step * kBatch * kThreads * 8;
#pragma unroll
                        for (int it = 0; it < kBatch; ++it) {
                            const int idx = base + it * kThreads * 8;
                            const bool valid = idx < r1;
                            const uint4 raw4 = valid ? *reinterpret_cast<uint4 *>(&iscores[idx >> 1]) : make_uint4(0u, 0u, 0u, 0u);
                            if (valid && !recoverable) *reinterpret_cast<uint4 *>(&iscores[idx >> 1]) = make_uint4(0u, 0u, 0u, 0u);
                            const uint32_t words[4] = {raw4.x, raw4.y, raw4.z, raw4.w};
                            // the eight rows' largest score against the fixed-point image of pre - mass (rounded down by more
                            // than the float test's roundings: a superset); the float tests only run for the groups that pass
                            if (__ballot(max_of_packed8(raw4) >= any_fixed) == 0) continue;
                            uint32_t fx[8];
#pragma unroll
                            for (int e = 0; e < 8; ++e) fx[e] = (words[e >> 1] >> ((e & 1) * 16)) & 0xffffu;
                            const float mass4[4] = {here.mass, here.mass, here.mass, here.mass};
                            // the tile's smallest sums32 stands in for the rows' own (no global read in a scan: the rows are in
                            // sums32 order, a tile's range is narrow; the refinement tests the survivors with their own)
                            const float bound4[4] = {tile_min, tile_min, tile_min, tile_min};
                            {
                                const uint32_t s4[4] = {fx[0], fx[1], fx[2], fx[3]};
                                const uint32_t rows4[4] = {static_cast<uint32_t>(idx), static_cast<uint32_t>(idx + 1),
                                                           static_cast<uint32_t>(idx + 2), static_cast<uint32_t>(idx + 3)};
                                consider4(s4, rows4, bound4, mass4);
                            }
                            {
                                const uint32_t s4[4] = {fx[4], fx[5], fx[6], fx[7]};
                                const uint32_t rows4[4] = {static_cast<uint32_t>(idx + 4), static_cast<uint32_t>(idx + 5),
                                                           static_cast<uint32_t>(idx + 6), static_cast<uint32_t>(idx + 7)};
                                consider4(s4, rows4, bound4, mass4);
                            }
                        }
                    }
                    flush_raw();
                    __syncthreads();
                    DS_STAMP(3);
                    last_appended = uniform(static_cast<int>(ctrl[kLCount])) - count_at_step;
                    if (uniform(static_cast<int>(ctrl[kLOverflow]))) {
                        // the buffer holds as many of the step's rows as fitted: tighten the threshold with them,
                        // drop the step's rows from the buffer and scan the same rows again
                        if (!recoverable || ++retries > 6) { slow = true; reason = 3; break; }
                        wanted_in = uniform(static_cast<int>(ctrl[kLCount]));  // appends count on beyond the capacity
                        floor_shift = min(retries - 1, 3);
                        __syncthreads();
                        if (tid == 0) {
                            ctrl[kLCount] = kCandidates;
                            ctrl[kLOverflow] = 0;
                        }
                        __syncthreads();
                        force_select = true;
                        drop_lo = static_cast<int32_t>(tile_base + r0);
                        drop_hi = static_cast<int32_t>(tile_base + r1);
                    } else {
                        if (recoverable) {
                            for (int idx = r0 + tid * 8; idx < r1; idx += kThreads * 8)
                                *reinterpret_cast<uint4 *>(&iscores[idx >> 1]) = make_uint4(0u, 0u, 0u, 0u);
                            __syncthreads();
                            DS_STAMP(9);
                        }
                        r0 = r1;
                        retries = 0;
                    }
                    DS_STAMP(12);
                }
                select_now = false;
                const int m = uniform(static_cast<int>(ctrl[kLCount]));
                if ((m < next_select && !force_select) || m < k) {
                    if (force_select) { slow = true; reason = 3; break; }  // nothing to tighten with
                    continue;
                }
                // ---- tighten: tau = k-th largest lower estimate seen so far; keep what can still qualify
                const uint32_t tau_key = radix_select_kth(cand_key, m, k, hist, ctrl, 2);
                ++selects;
                if (wanted_in > 0) {
                    // The buffer overflowed: what it holds is a sample (m of the `wanted_in` rows above the cut), and scanning
                    // the same rows again under the tightened cut alone overflows again when thousands of them lie within a
                    // few per cent of each other (the start tile of a weak query in sums32 order).  The sample's r-th largest
                    // key becomes the admission floor, r chosen so that about kSelectTrigger - 64 rows lie above it.  The
                    // answer stands if the FINAL cut ends above the floor (checked before the exact stage).
                    const int rank = static_cast<int>(static_cast<long long>(max((kSelectTrigger - 64) >> floor_shift, k + 16)) * m / max(wanted_in, m));
                    wanted_in = 0;
                    const uint32_t pivot = radix_select_kth(cand_key, m, max(1, min(m, rank)), hist, ctrl, 4);
                    if (tid == 0 && static_cast<uint32_t>(ctrl[kLFloor]) < pivot) ctrl[kLFloor] = static_cast<int32_t>(pivot);
                }
                if (wave == 0) {
                    const double tau = static_cast<double>(__uint_as_float(tau_key));
                    const double cut_value = tau - 2.0 * error_margin() - 2e-6;
                    float new_coef = 0.f, new_pre = FLT_MIN, new_cut = 0.f;
                    if (tau_key < 0x7f800000u && cut_value > 0.0) {
                        const double c = cut_value / (1.0 + cut_value) * (1.0 - 9.5367431640625e-07);
                        new_coef = round_down_positive(c);
                        new_cut = round_down_positive(cut_value);
                        // The smallest sums32 a row that can still qualify may have: jaccard = s / (sums + maxint - s) and
                        // s <= sums32[row], so the denominator is at least maxint and jaccard <= sums32 / maxint -- a row with
                        // sums32 < cut * maxint cannot qualify in whatever tile it lies (the band test at the epoch's end relies
                        // on the same inequality, with the same relative slack of 1e-5).  PRECONDITION, the band test's own:
                        // sums32[row] is the total of the row's columns (match_maker.py:174), short of it by float32 rounding
                        // at most.  ds_index_create admits rows whose sums32 lies up to 1e-4 below their total to this kernel;
                        // the slack of 1e-5 and the cut's own margin cover a relative shortfall d as long as cut * (2 * d - 1e-5)
                        // stays below the margin (s <= sums32 * (1 + d) gives jaccard <= cut * (1 + 2 * d) at the band's edge):
                        // about 5e-6, the rounding of a float32 total, not that whole range.  Every
                        // row that can qualify therefore needs s >= coef * (cut * maxint + maxint) = cut * maxint, (1 + cut)
                        // times the bound from the index's smallest sums32 alone.  `pre` stays an UPPER-bound test only ("a row
                        // whose upper bound lies below pre cannot qualify"); nothing reads it as a lower estimate.
                        const double band_edge = static_cast<double>(new_cut) * static_cast<double>(maxint32) * (1.0 - 1e-5);
                        const double sums_floor = band_edge > static_cast<double>(a.sums_min) ? band_edge
                                                                                              : static_cast<double>(a.sums_min);
                        const double p = static_cast<double>(new_coef) * (sums_floor + static_cast<double>(maxint32)) *
                                         (1.0 - 9.5367431640625e-07);
                        new_pre = p > static_cast<double>(FLT_MIN) ? round_down_positive(p) : FLT_MIN;
                    }
                    // non-essential columns: the longest ascending-IDF prefix whose total mass stays below `pre`
                    // and whose columns all own a signature bit (completion is then a single load per row)
                    int skip_count = 0;
                    {
                        const bool ok0 = lane < n && mass_upto[lane] < new_pre && sig_bit[order[lane]] >= 0;
                        const bool ok1 = lane + 64 < n && mass_upto[lane + 64] < new_pre && sig_bit[order[lane + 64]] >= 0;
                        const unsigned long long v0 = __ballot(ok0), v1 = __ballot(ok1);
                        skip_count = ~v0 ? __ffsll(static_cast<long long>(~v0)) - 1
                                         : 64 + (~v1 ? __ffsll(static_cast<long long>(~v1)) - 1 : 64);
                    }
                    uint32_t mask_bits[kSignatureWords] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int r = lane + 64 * h;
                        if (r < skip_count) {
                            const int bit = sig_bit[order[r]];
#pragma unroll
                            for (int w = 0; w < kSignatureWords; ++w)
                                if ((bit >> 5) == w) mask_bits[w] |= 1u << (bit & 31);
                        }
                    }
#pragma unroll
                    for (int w = 0; w < kSignatureWords; ++w)
                        for (int d = 32; d > 0; d >>= 1) mask_bits[w] |= __shfl_xor(mask_bits[w], d);
                    uint32_t essential_quads = 0;
                    count_units(static_cast<uint32_t>(n));  // two list pointers per column
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int j = lane + 64 * h;
                        if (j < n && rank[j] >= skip_count)  // quads of column j over all tiles (two list pointers)
                            essential_quads += a.col_ptr[static_cast<int64_t>(cols[j]) * ptr_stride + a.n_tiles] -
                                               a.col_ptr[static_cast<int64_t>(cols[j]) * ptr_stride];
                    }
                    for (int d = 32; d > 0; d >>= 1) essential_quads += __shfl_xor(essential_quads, d);
                    if (lane == 0) {
                        ctrl[kLSparse] = essential_quads / static_cast<uint32_t>(a.n_tiles) <=
                                         static_cast<uint32_t>(a.sparse_quads);
                        for (int w = 0; w < kSignatureWords; ++w) ctrl[kLSigMask + w] = static_cast<int32_t>(mask_bits[w]);
                        ctrl[kLCoef] = __float_as_int(new_coef);
                        ctrl[kLPre] = __float_as_int(new_pre);
                        ctrl[kLCut] = __float_as_int(new_cut);
                        ctrl[kLNonEssential] = skip_count;
                        ctrl[kLMass] = __float_as_int(skip_count > 0 ? mass_upto[skip_count - 1] : 0.f);
                    }
                }
                __syncthreads();
                bounds.coef = uniform(__int_as_float(ctrl[kLCoef]));
                bounds.pre = uniform(__int_as_float(ctrl[kLPre]));
                here.coef = bounds.coef;
                {
                    const float gate = uniform(bounds.coef * (tile_min + maxint32) * (1.f - 3.814697265625e-06f));
                    here.pre = gate > bounds.pre ? gate : bounds.pre;
                }
                pending_mass = uniform(__int_as_float(ctrl[kLMass]));
                rebuild_mass_table = true;
                cut = uniform(__int_as_float(ctrl[kLCut]));
                non_essential = uniform(static_cast<int>(ctrl[kLNonEssential]));
                sparse_mode = uniform(static_cast<int>(ctrl[kLSparse])) != 0;
                tight = true;
                // in-place compaction: read everything, barrier, rewrite the survivors (nothing at or below the admission
                // floor stays: the floor is the largest key ever turned away)
                const uint32_t floor_now = uniform(static_cast<uint32_t>(ctrl[kLFloor]));
                uint32_t keep_key[kKeep];
                int32_t keep_row[kKeep];
#pragma unroll
                for (int r = 0; r < kKeep; ++r) {
                    const int i = tid + r * kThreads;
                    keep_key[r] = i < m ? cand_key[i] : 0u;
                    keep_row[r] = i < m ? cand_row[i] : -1;
                }
                __syncthreads();
                if (tid == 0) ctrl[kLCount] = 0;
                __syncthreads();
#pragma unroll
                for (int r = 0; r < kKeep; ++r) {
                    if (keep_row[r] >= 0 && __uint_as_float(keep_key[r]) >= cut && keep_key[r] > floor_now &&
                        !(keep_row[r] >= drop_lo && keep_row[r] < drop_hi)) {
                        const int slot = atomicAdd(ctrl.at(kLCount), 1);
                        cand_key[slot] = keep_key[r];
                        cand_row[slot] = keep_row[r];
                    }
                }
                drop_lo = drop_hi = 0;
                __syncthreads();
                int kept = uniform(static_cast<int>(ctrl[kLCount]));
                __syncthreads();  // a retried scan appends right away: the count must be read by all threads first
                if (kept > kSelectTrigger) {
                    // More rows above the cut than the buffer may keep -- but the threshold is that of the rows seen SO FAR, and
                    // tiles still to come can only raise it (with the rows in sums32 order the first tiles hold a query's
                    // strongest candidates, thousands of near-equal ones for a weak query).  Keep the best `target` rows and
                    // remember the largest key dropped (the admission floor: later rows at or below it are turned away too).
                    // The answer stands if the FINAL cut ends above the floor; otherwise the query is handed over then.
                    const int target = max(kSelectTrigger - 64, min(kSelectTrigger - 16, k + 32));  // room for 64 + the slack's 256 new rows
                    const uint32_t pivot = radix_select_kth(cand_key, kept, target, hist, ctrl, 4);  // exact target-th largest key
#pragma unroll
                    for (int r = 0; r < kKeep; ++r) {
                        const int i = tid + r * kThreads;
                        keep_key[r] = i < kept ? cand_key[i] : 0u;
                        keep_row[r] = i < kept ? cand_row[i] : -1;
                    }
                    __syncthreads();
                    if (tid == 0) {
                        ctrl[kLCount] = 0;
                        if (static_cast<uint32_t>(ctrl[kLFloor]) < pivot) ctrl[kLFloor] = static_cast<int32_t>(pivot);
                    }
                    __syncthreads();
#pragma unroll
                    for (int r = 0; r < kKeep; ++r) {
                        if (keep_row[r] >= 0 && keep_key[r] > pivot) {
                            const int slot = atomicAdd(ctrl.at(kLCount), 1);
                            cand_key[slot] = keep_key[r];
                            cand_row[slot] = keep_row[r];
                        }
                    }
                    __syncthreads();
                    kept = uniform(static_cast<int>(ctrl[kLCount]));
                    __syncthreads();
                    if (kept < k) { slow = true; reason = 4; break; }  // the k best themselves tie at the pivot: the literal kernel
                }
                next_select = min(kSelectTrigger, max(a.select_growth * kept / 2, a.select_min));
                count_at_step = kept;
                DS_STAMP(4);
            }
            if (slow) break;
            if (redo_tile) {  // back onto the first tile of the epoch
                b = epoch_start;
                block_end = 0;  // its list pointers may lie in front of the cached block
                continue;
            }
            if (!epoch_end) {
                ++b;
                continue;
            }
            // the epoch is over: where the next one lies (thresholds as the selection above left them)
            const bool sparse_next = kEpochTiles > 1 && tight && sparse_mode;
            const int length = sparse_next ? kEpochTiles : 1;
            const bool bounded = sorted && cut > 0.f;
            // Both sides of the start tile hold candidates of decreasing promise the farther away they lie: the sweep alternates
            // between them in runs of one list-pointer block, so that the threshold (and with it both ends of the band) settles
            // early.  A side that has left the band stays out: the cut only rises.
            const bool up_ok = up_next < a.n_tiles && !(bounded && tile_sums_min[up_next] * cut > maxint32 * 1.00001f);
            const bool down_ok = down_next >= 0 && !(bounded && tile_sums_max[down_next] < cut * maxint32 * 0.99999f);
            if (up_ok && down_ok) {
                if (--run_left <= 0) {
                    descending = !descending;
                    run_left = max(1, span / length);
                }
            } else {
                descending = down_ok && !up_ok;
            }
            bool found = up_ok || down_ok;
            if (found && !descending) {
                epoch_start = up_next;
                epoch_last = min(up_next + length - 1, a.n_tiles - 1);
                up_next = epoch_last + 1;
            } else if (found) {
                epoch_last = down_next;
                epoch_start = max(0, down_next - length + 1);
                down_next = epoch_start - 1;
            }
            if (!found) break;  // every tile left is out of the threshold's reach
            b = epoch_start;
        }

        if (!slow) __syncthreads();
        int m = slow ? 0 : uniform(static_cast<int>(ctrl[kLCount]));
        // Fewer than k candidates: fewer than k rows have a positive score at all (nothing is pruned before k candidates
        // exist).  The literal kernel answers it without sweeping anything (the answer is the k largest row indexes).
        // rows were dropped for lack of room: the answer stands only if every one of them lies below the final cut
        const uint32_t dropped_key = slow ? 0u : uniform(static_cast<uint32_t>(ctrl[kLFloor]));
        if (!slow && dropped_key != 0u && m < k) { slow = true; reason = 4; }  // fewer than k left AFTER dropping rows: unknown
        if (!slow && m < k) { slow = true; reason = 5; }
        if (!slow) {
            // final tightening so that only k + near-ties + margin survivors are evaluated exactly (with exactly k rows left it
            // only serves the check of the admission floor)
            if (m > k || dropped_key != 0u) {
                const uint32_t tau_key = radix_select_kth(cand_key, m, k, hist, ctrl, 4);
                ++selects;
                const double tau = static_cast<double>(__uint_as_float(tau_key));
                const double cut_value = tau - 2.0 * error_margin() - 2e-6;
                const float final_cut =
                    (tau_key < 0x7f800000u && cut_value > 0.0) ? round_down_positive(cut_value) : 0.f;
                if (dropped_key != 0u && !(__uint_as_float(dropped_key) < final_cut)) { slow = true; reason = 4; }
                uint32_t keep_key[kKeep];
                int32_t keep_row[kKeep];
#pragma unroll
                for (int r = 0; r < kKeep; ++r) {
                    const int i = tid + r * kThreads;
                    keep_key[r] = i < m ? cand_key[i] : 0u;
                    keep_row[r] = i < m ? cand_row[i] : -1;
                }
                __syncthreads();
                if (tid == 0) ctrl[kLCount] = 0;
                __syncthreads();
#pragma unroll
                for (int r = 0; r < kKeep; ++r) {
                    if (keep_row[r] >= 0 && __uint_as_float(keep_key[r]) >= final_cut) {
                        const int slot = atomicAdd(ctrl.at(kLCount), 1);
                        cand_row[slot] = keep_row[r];
                    }
                }
                __syncthreads();
                m = uniform(static_cast<int>(ctrl[kLCount]));
            }
            DS_STAMP(4);
        }
        if (!slow && m > kExactRows) { slow = true; reason = 4; }  // (only a buffer larger than the exact stage's scratch gets here: near-ties)
        if (!slow) {
            // ---- exact evaluation.  Scratch lives in the (all-zero) score tile:
            //   hit masks   uint32[m][4]  (bit j = row is in the posting list of query column j)
            //   exact value float64[m]    behind them (kExactValueOffset)
            uint32_t *hit_mask = iscores;
            double *exact_jaccard = reinterpret_cast<double *>(lds + kExactValueOffset);
            // Which of the query's columns does a candidate row hold?  Round 4: from the FORWARD index -- the row's own ~21
            // columns, read in one go, each looked up among the query's columns (sorted copy in LDS) -- instead of searching
            // the row in every query column's posting list (one binary search of ~5 dependent global loads per (candidate,
            // column): 20.6 % of the kernel at top-100, 2,350 searches per query).
            int32_t *sorted_col = reinterpret_cast<int32_t *>(lds + kExactSortedOffset);       // [kMaxQueryColumns], ascending
            uint8_t *sorted_at = reinterpret_cast<uint8_t *>(lds + kExactSortedOffset + kMaxQueryColumns * 4);  // their positions in the query
            if (tid < kMaxQueryColumns) {
                int32_t mine = 0x7fffffff;   // beyond every column id: the search never lands on the padding
                int r = tid;
                if (tid < n) {
                    mine = cols[tid];
                    r = 0;
#pragma unroll 8
                    for (int i = 0; i < n; ++i) {
                        const int32_t other = cols[i];
                        r += (other < mine) | ((other == mine) & (i < tid));
                    }
                }
                // slots n..127 are written by the threads n..127 themselves (r = tid): together a permutation of 0..127
                sorted_col[r] = mine;
                sorted_at[r] = static_cast<uint8_t>(tid);
            }
            __syncthreads();
            uint32_t probe_bytes = 0;  // counting instantiation only
            constexpr int kSlots = 32;  // columns of a row handled per pass: one lane each (a second pass for rows of more)
            // The forward index in its narrow form (uint32 row starts, uint16 columns: every index whose nnz < 2^32 and V <= 65536) is
            // read by a copy of the loop without a branch per load; the other forms share the generic copy.
            auto membership = [&](auto narrow_tag) {
            constexpr bool kNarrow = decltype(narrow_tag)::value;
            const bool wide_start = !kNarrow && a.forward_wide_start != 0, wide_cols = !kNarrow && a.forward_wide_cols != 0;  // (workgroup-uniform)
            for (int pass_base = 0;; pass_base += kSlots) {
                bool more = false;
                // one (candidate, position in its column list) per thread and step, FOUR steps at a time: the steps' row_start pairs
                // are loaded together, then their columns, then the look-ups run -- two memory round trips per four steps
                // instead of two per step (top-100: 112 candidates x 32 slots = 14 steps per thread)
                constexpr int kSteps = 4;
                for (int p0 = tid; p0 < m * kSlots; p0 += kThreads * kSteps) {
                    int which[kSteps], slot[kSteps];
                    int64_t begin[kSteps], end[kSteps];
                    bool valid[kSteps];
#pragma unroll
                    for (int u = 0; u < kSteps; ++u) {
                        const int p = p0 + u * kThreads;
                        which[u] = p / kSlots;
                        slot[u] = pass_base + (p - which[u] * kSlots);
                        valid[u] = p < m * kSlots;
                        const int32_t t = valid[u] ? cand_row[which[u]] : 0;
                        valid[u] = valid[u] && DS_OK_INDEX(6, t, a.n_truth);
                        if (wide_start) {
                            begin[u] = valid[u] ? static_cast<const int64_t *>(a.row_start)[t] : 0;
                            end[u] = valid[u] ? static_cast<const int64_t *>(a.row_start)[t + 1] : 0;
                        } else {
                            begin[u] = valid[u] ? static_cast<int64_t>(static_cast<const uint32_t *>(a.row_start)[t]) : 0;
                            end[u] = valid[u] ? static_cast<int64_t>(static_cast<const uint32_t *>(a.row_start)[t + 1]) : 0;
                        }
                        if constexpr (kCountBytes) probe_bytes += (valid[u] && slot[u] == pass_base) ? (wide_start ? 16 : 8) : 0;
                    }
                    int32_t column[kSteps];
#pragma unroll
                    for (int u = 0; u < kSteps; ++u) {
                        const int64_t length = end[u] - begin[u];
                        more |= valid[u] && length > pass_base + kSlots;
                        valid[u] = valid[u] && slot[u] < length && DS_OK_INDEX(9, begin[u] + slot[u], a.nnz);
                        column[u] = !valid[u] ? -1
                                    : (wide_cols ? static_cast<const int32_t *>(a.row_cols)[begin[u] + slot[u]]
                                                 : static_cast<int32_t>(static_cast<const uint16_t *>(a.row_cols)[begin[u] + slot[u]]));
                        if constexpr (kCountBytes) probe_bytes += valid[u] ? (wide_cols ? 4 : 2) : 0;
                    }
#pragma unroll
                    for (int u = 0; u < kSteps; ++u) {
                        if (!valid[u]) continue;
                        int at = 0;  // the last slot whose column is <= `column` (slot 0 if none)
#pragma unroll
                        for (int bit = kMaxQueryColumns / 2; bit > 0; bit >>= 1) at = sorted_col[at + bit] <= column[u] ? at + bit : at;
                        if (sorted_col[at] == column[u]) {
                            const int j = sorted_at[at];
                            atomicOr(&hit_mask[which[u] * 4 + (j >> 5)], 1u << (j & 31));
                        }
                    }
                }
                if (!__syncthreads_or(more)) break;
            }
            };
            if (a.forward_wide_start == 0 && a.forward_wide_cols == 0) membership(std::true_type{});
            else membership(std::false_type{});
            if constexpr (kCountBytes) {
                if (tid < m) probe_bytes += 4;  // sums32 of the candidate
                if (probe_bytes) atomicAdd(requested, static_cast<unsigned long long>(probe_bytes));
            }
            __syncthreads();
            for (int i = tid; i < m; i += kThreads) {
                float score = 0.f;
                for (int word = 0; word < 4; ++word) {
                    uint32_t bits = hit_mask[i * 4 + word];
                    while (bits) {  // float32 accumulation in the query's column order (match_maker.py:46-48)
                        const int j = word * 32 + __ffs(bits) - 1;
                        score = score + idf[j];
                        bits &= bits - 1u;
                    }
                }
                const double s = static_cast<double>(score);
                if (!DS_OK_INDEX(7, cand_row[i], a.n_truth)) continue;
                exact_jaccard[i] = s / (static_cast<double>(a.sums32[cand_row[i]]) + (maxint - s));  // :50
                // the rows are visited in the index's internal order; match_maker.py:71 is about the caller's row indexes
                // (word 6 of the row record).  The candidate keys are not needed any more: their array takes them.
                cand_key[i] = reinterpret_cast<const uint32_t *>(a.rows + 2 * static_cast<int64_t>(cand_row[i]))[6];
            }
            __syncthreads();
            // k-th largest exact value (rank by counting; m is small) and, below, a qualifying row's place in the output (the
            // number of qualifying rows with a larger caller's row index): m * m comparisons each.  With m at most half the
            // workgroup every candidate's comparisons are split over kThreads / m threads (partial counts meet in LDS):
            // at top-100 (m ~ 112) the two loops were a seventh of the kernel with 112 of 256 threads at work.
            uint32_t *partial = reinterpret_cast<uint32_t *>(lds + kExactCountOffset);  // [m], zero between uses
            const int parts = m <= kThreads / 2 ? kThreads / m : 1;
            const int part = parts > 1 ? tid / m : 0, mine = parts > 1 ? tid - part * m : tid;
            const int j_begin = parts > 1 ? m * part / parts : 0, j_end = parts > 1 ? (part < parts ? m * (part + 1) / parts : 0) : m;
            if (parts > 1) {
                if (part < parts) {
                    const double v = exact_jaccard[mine];
                    int above = 0;
#pragma unroll 8
                    for (int j = j_begin; j < j_end; ++j) {
                        const double w = exact_jaccard[j];
                        above += (w > v) | ((w == v) & (j < mine));
                    }
                    if (above) atomicAdd(&partial[mine], static_cast<uint32_t>(above));
                }
                __syncthreads();
                if (tid < m) {
                    if (partial[tid] == static_cast<uint32_t>(k - 1)) {
                        const double v = exact_jaccard[tid];
                        ctrl[kLKth0] = __double2loint(v);
                        ctrl[kLKth1] = __double2hiint(v);
                    }
                    partial[tid] = 0u;
                }
            } else {
                for (int i = tid; i < m; i += kThreads) {
                    const double v = exact_jaccard[i];
                    int above = 0;
#pragma unroll 8
                    for (int j = 0; j < m; ++j) {  // unrolled: eight LDS reads in flight instead of one wait per value
                        const double w = exact_jaccard[j];
                        above += (w > v) | ((w == v) & (j < i));
                    }
                    if (above == k - 1) {
                        ctrl[kLKth0] = __double2loint(v);
                        ctrl[kLKth1] = __double2hiint(v);
                    }
                }
            }
            __syncthreads();
            const double kth = __hiloint2double(ctrl[kLKth1], ctrl[kLKth0]);
            const float kth32 = static_cast<float>(kth);                                       // match_maker.py:65
            const double threshold = static_cast<double>(kth32) - static_cast<double>(1e-6f);  // match_maker.py:70
            if (threshold <= 0.0) {
                // every row qualifies (zeros included): the k largest row indexes
                for (int j = tid; j < k; j += kThreads)
                    a.out_rows[q * k + j] = static_cast<int32_t>(a.n_truth - 1 - j);
            } else if (parts > 1) {
                const bool qualifies = part < parts && exact_jaccard[mine] >= threshold;       // match_maker.py:71
                const int32_t t = part < parts ? static_cast<int32_t>(cand_key[mine]) : 0;     // the caller's row index
                if (qualifies) {
                    int above = 0;
#pragma unroll 8
                    for (int j = j_begin; j < j_end; ++j) above += (exact_jaccard[j] >= threshold) & (static_cast<int32_t>(cand_key[j]) > t);
                    if (above) atomicAdd(&partial[mine], static_cast<uint32_t>(above));
                }
                __syncthreads();
                if (qualifies && part == 0) {
                    const int above = static_cast<int>(partial[mine]);
                    if (above < k && DS_OK_INDEX(8, q * k + above, a.n_queries * k)) a.out_rows[q * k + above] = t;
                }
            } else {
                for (int i = tid; i < m; i += kThreads) {
                    if (!(exact_jaccard[i] >= threshold)) continue;                            // match_maker.py:71
                    const int32_t t = static_cast<int32_t>(cand_key[i]);                       // the caller's row index
                    int above = 0;
#pragma unroll 8
                    for (int j = 0; j < m; ++j) above += (exact_jaccard[j] >= threshold) & (static_cast<int32_t>(cand_key[j]) > t);
                    if (above < k && DS_OK_INDEX(8, q * k + above, a.n_queries * k)) a.out_rows[q * k + above] = t;
                }
            }
            __syncthreads();
            for (int i = tid; i < m * 4; i += kThreads) hit_mask[i] = 0u;  // give the tile back zeroed
            for (int i = tid; i < m; i += kThreads) exact_jaccard[i] = 0.0;
            for (int i = tid; i < kMaxQueryColumns * 5 / 4; i += kThreads) reinterpret_cast<uint32_t *>(lds + kExactSortedOffset)[i] = 0u;
            if (tid < kThreads / 2) partial[tid] = 0u;
            if (tid == 0) {
                a.status[q] = kQueryDone;
                // statistics are summed per workgroup in LDS and reach HBM once, at the end of the kernel
                ctrl[kLStats + 0] += m;
                ctrl[kLStats + 1] += selects;
                ctrl[kLStats + 2] += sparse_tiles;
                ctrl[kLStats + 3] += dense_tiles;
                ctrl[kLStats + 4] += non_essential;
                if constexpr (kCountBytes) atomicAdd(requested, 8ull * query_units);
            }
            __syncthreads();
            DS_STAMP(5);
        } else {
            if (tid == 0) {
                a.status[q] = reason == 5 ? kQuerySlowFew : kQuerySlow;
                a.slow_list[atomicAdd(&a.control[kCtlSlowCount], 1)] = static_cast<int32_t>(q);
                if (reason >= 0) atomicAdd(&a.control[kCtlReason + reason], 1);
                if constexpr (kCountBytes) atomicAdd(requested, 8ull * query_units);
            }
            for (int i = tid * 4; i < kScoreWords; i += kThreads * 4)
                *reinterpret_cast<uint4 *>(&iscores[i]) = make_uint4(0u, 0u, 0u, 0u);
            __syncthreads();
            DS_STAMP(0);
        }
    }
    if constexpr (kCountBytes) {
        __syncthreads();
        if (tid == 0) atomicAdd(reinterpret_cast<unsigned long long *>(a.control + kCtlBytes), *requested);
    }
    if (tid == 0) {
        atomicAdd(&a.control[kCtlExact], ctrl[kLStats + 0]);
        atomicAdd(&a.control[kCtlSelects], ctrl[kLStats + 1]);
        atomicAdd(&a.control[kCtlSparseTiles], ctrl[kLStats + 2]);
        atomicAdd(&a.control[kCtlDenseTiles], ctrl[kLStats + 3]);
        atomicAdd(&a.control[kCtlSkippedColumns], ctrl[kLStats + 4]);
    }
#ifdef DS_DIAGNOSTICS
    if (a.phase != nullptr && tid == 0)
        for (int i = 0; i < 16; ++i) atomicAdd(&a.phase[i], phase_lds[i]);
#endif
}

// ---- the order in which the work queue hands out the queries ---------------------------------------------------------------
// Queries with many columns take longest; handed out first they keep the tail of the launch short (longest processing time
// first: C2 15.41 -> 15.06 ms, C3 shape 59.1 -> 57.3 ms with the queries pre-sorted on the host, profiles/r03_tuning.txt).
// A counting sort on the number of columns, 129 bins, descending: one pass counts, one pass places -- each workgroup
// reserves its share of every bin with ONE global atomic per bin (the order inside a bin does not matter).
constexpr int kOrderBins = 129, kOrderStride = 136, kOrderThreads = 256;
__device__ __forceinline__ int order_bin(const int64_t *q_rowptr, int64_t q)
{
    const int64_t n = q_rowptr[q + 1] - q_rowptr[q];
    return kOrderBins - 1 - static_cast<int>(n < 0 ? 0 : (n > kOrderBins - 1 ? kOrderBins - 1 : n));
}

__global__ __launch_bounds__(kOrderThreads) void ds_query_order_count_kernel(const int64_t *q_rowptr, int64_t n_queries,
                                                                              int64_t chunk, int32_t *bins)
{
    __shared__ int32_t local[kOrderBins];
    for (int i = threadIdx.x; i < kOrderBins; i += kOrderThreads) local[i] = 0;
    __syncthreads();
    const int64_t begin = static_cast<int64_t>(blockIdx.x) * chunk, end = begin + chunk < n_queries ? begin + chunk : n_queries;
    for (int64_t q = begin + threadIdx.x; q < end; q += kOrderThreads) atomicAdd(&local[order_bin(q_rowptr, q)], 1);
    __syncthreads();
    for (int i = threadIdx.x; i < kOrderBins; i += kOrderThreads)
        if (local[i] != 0) atomicAdd(&bins[i], local[i]);
}

__global__ __launch_bounds__(kOrderThreads) void ds_query_order_place_kernel(const int64_t *q_rowptr, int64_t n_queries,
                                                                              int64_t chunk, int32_t *bins, int32_t *take_order)
{
    __shared__ int32_t local[kOrderBins], start[kOrderBins];
    for (int i = threadIdx.x; i < kOrderBins; i += kOrderThreads) local[i] = 0;
    __syncthreads();
    const int64_t begin = static_cast<int64_t>(blockIdx.x) * chunk, end = begin + chunk < n_queries ? begin + chunk : n_queries;
    for (int64_t q = begin + threadIdx.x; q < end; q += kOrderThreads) atomicAdd(&local[order_bin(q_rowptr, q)], 1);
    __syncthreads();
    {   // first position of every bin (exclusive scan of the 129 counts) + this workgroup's share of the bin
        __shared__ int32_t scan[kOrderThreads];
        const int t = threadIdx.x;
        const int32_t count = t < kOrderBins ? bins[t] : 0;
        const int32_t share = (t < kOrderBins && local[t] != 0) ? atomicAdd(&bins[kOrderStride + t], local[t]) : 0;
        scan[t] = count;
        __syncthreads();
        for (int d = 1; d < kOrderThreads; d <<= 1) {
            const int32_t below = t >= d ? scan[t - d] : 0;
            __syncthreads();
            scan[t] += below;
            __syncthreads();
        }
        if (t < kOrderBins) start[t] = scan[t] - count + share;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kOrderBins; i += kOrderThreads) local[i] = 0;
    __syncthreads();
    for (int64_t q = begin + threadIdx.x; q < end; q += kOrderThreads) {
        const int bin = order_bin(q_rowptr, q);
        take_order[start[bin] + atomicAdd(&local[bin], 1)] = static_cast<int32_t>(q);
    }
}

// ---- a column listed twice in a query -------------------------------------------------------------------------------
// Impossible from match_maker.py:196 (the columns of a CSR row), possible through the C ABI: the reference's loop
// (match_maker.py:46-48) then adds the column's value twice, while the fast kernel's signature completion counts a
// skipped column once.  One wave per query checks the answered queries AFTER the fast kernel and hands those with a
// repeated column to the literal kernel, which follows the reference's loop -- the fast kernel itself stays untouched.
__global__ __launch_bounds__(256) void ds_jaccard_repeats_kernel(JaccardArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t q = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (q >= a.n_queries) return;
    const int64_t base = a.q_rowptr[q];
    const int64_t n = a.q_rowptr[q + 1] - base;
    if (n < 2 || n > kMaxQueryColumns) return;  // longer queries take the literal kernel anyway
    // lanes without a column hold distinct negative values (a negative column is an argument error, reported before)
    const int32_t mine0 = lane < n ? a.q_cols[base + lane] : -1 - lane;
    const int32_t mine1 = lane + 64 < n ? a.q_cols[base + lane + 64] : -65 - lane;
    bool repeated = false;
    for (int i = 0; i < static_cast<int>(n); ++i) {
        const int32_t other = __shfl(i < 64 ? mine0 : mine1, i & 63);
        repeated |= ((other == mine0) & (i != lane)) | ((other == mine1) & (i != lane + 64));
    }
    if (__ballot(repeated) == 0 || lane != 0) return;
    if (a.status[q] != kQueryDone) return;  // handed over already, or an argument error
    a.status[q] = kQuerySlow;
    a.slow_list[atomicAdd(&a.control[kCtlSlowCount], 1)] = static_cast<int32_t>(q);
    atomicAdd(&a.control[kCtlReason + 0], 1);
}

// ---- the literal algorithm for the queries the fast kernel hands over ------------------------------------------------
// fast_jaccard exactly as the reference runs it (ordered float32 accumulation per row, float64 finalise,
// match_maker.py:45-50), tile by tile FROM THE LAST TILE DOWN, and fast_arg_top_k (:53-71) as a streaming selection
// that needs no N-vector in HBM:
//   the rows that can still matter are kept in an LDS buffer of (float64 jaccard, row).  With T_run = float32(k-th
//   largest value seen so far) - 1e-6 (a lower bound of the final threshold, which only grows):
//     (a) a row below T_run is below the final threshold: dropped for good;
//     (b) a row r that has k rows of LARGER index with a value >= its own can be dropped too: if r qualifies at the end
//         so do those k rows, and :71 returns the k largest indexes; the k-th largest value does not need r either
//         (its k dominators keep it in place).
//   Rows arrive tile by tile, 1024 at a time; when the next 1024 might not fit, the buffer is compacted with (a) and, if
//   that is not enough, (b).  At the end the k-th largest float32 value of the buffer IS the reference's heap minimum.
constexpr int kDenseScoreFloats = kTile + 64;  // float32 score tile + trash slot
constexpr int kDenseChunk = 256;   // query columns whose (list begin, list end, idf) are staged in LDS at a time
constexpr int kDenseBuffer = 3072; // rows kept per query: value float64 + row int32 = 36 KiB
constexpr int kDenseOffHist = kDenseScoreFloats * 4;
constexpr int kDenseOffCtrl = kDenseOffHist + 256 * 4;
constexpr int kDenseOffStage = kDenseOffCtrl + 128;
constexpr int kDenseOffValue = kDenseOffStage + kDenseChunk * 12;
constexpr int kDenseOffRow = kDenseOffValue + kDenseBuffer * 8;
constexpr int kDenseLdsBytes = kDenseOffRow + kDenseBuffer * 4;
static_assert(kDenseLdsBytes <= 160 * 1024 && kDenseOffValue % 8 == 0, "LDS budget of the literal kernel");
constexpr int kDenseKeep = (kDenseBuffer + kDenseThreads - 1) / kDenseThreads;
enum { kDCount = 0, kDDigit, kDRemain, kDQuery, kDKept };

__device__ __forceinline__ uint32_t dense_key(double v)  // the float32 the reference's heap stores (match_maker.py:65)
{
    return v > 0.0 ? __float_as_uint(static_cast<float>(v)) : 0u;
}

// k-th largest float32 key of the m buffered values (m >= k); every thread of the workgroup calls it
__device__ __forceinline__ uint32_t dense_select_kth(const double *value, int m, int k, uint32_t *hist, DenseControlWords ctrl)
{
    const int tid = threadIdx.x;
    uint32_t prefix = 0, mask = 0;
    int remaining = k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < m; i += kDenseThreads) {
            const uint32_t key = dense_key(value[i]);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            int cumulative = 0, digit = 0;
            for (int d = 255; d >= 0; --d) {
                const int c = static_cast<int>(hist[d]);
                if (cumulative + c >= remaining) { digit = d; break; }
                cumulative += c;
            }
            ctrl[kDDigit] = digit;
            ctrl[kDRemain] = remaining - cumulative;
        }
        __syncthreads();
        prefix |= static_cast<uint32_t>(ctrl[kDDigit]) << shift;
        mask |= 255u << shift;
        remaining = ctrl[kDRemain];
    }
    return prefix;
}

__global__ __launch_bounds__(kDenseThreads) void ds_jaccard_dense_kernel(JaccardArgs a)
{
    extern __shared__ __align__(16) unsigned char lds[];
    float *scores = reinterpret_cast<float *>(lds);
    uint32_t *hist = reinterpret_cast<uint32_t *>(lds + kDenseOffHist);
    const DenseControlWords ctrl{reinterpret_cast<int32_t *>(lds + kDenseOffCtrl)};
    uint32_t *stage_begin = reinterpret_cast<uint32_t *>(lds + kDenseOffStage);
    uint32_t *stage_end = stage_begin + kDenseChunk;
    float *stage_value = reinterpret_cast<float *>(stage_end + kDenseChunk);
    double *value = reinterpret_cast<double *>(lds + kDenseOffValue);
    int32_t *row = reinterpret_cast<int32_t *>(lds + kDenseOffRow);

    const int tid = threadIdx.x, lane = tid & 63;
    const int k = a.k;
    const int64_t n_truth = a.n_truth;
    const int64_t ptr_stride = static_cast<int64_t>(a.n_tiles) + 1;
    const int n_slow = a.control[kCtlSlowCount];

    for (;;) {
        if (tid == 0) {
            ctrl[kDQuery] = atomicAdd(&a.control[kCtlSlowQueue], 1);
            ctrl[kDCount] = 0;
        }
        __syncthreads();
        const int item = ctrl[kDQuery];
        __syncthreads();
        if (item >= n_slow) break;  // exit condition reached by every wave: the queue head only grows
        const int64_t q = a.slow_list[item];
        const int64_t qbase = a.q_rowptr[q];
        const int64_t n = a.q_rowptr[q + 1] - qbase;
        const double maxint = a.q_maxint[q];

        if (a.status[q] == kQuerySlowFew) {
            // The fast kernel found fewer than k rows with a positive score (and its assumptions hold: no negative
            // value exists): the heap of match_maker.py:60-67 keeps a zero, the threshold is -1e-6, EVERY row qualifies
            // and :71 returns the k largest row indexes.
            for (int j = tid; j < k; j += kDenseThreads) a.out_rows[q * k + j] = static_cast<int32_t>(n_truth - 1 - j);
            if (tid == 0) a.status[q] = kQuerySlow;
            __syncthreads();
            continue;
        }
        bool bad = false;
        for (int64_t j = tid; j < n; j += kDenseThreads) {
            const int32_t column = a.q_cols[qbase + j];
            bad |= column < 0 || column >= a.n_columns;
        }
        if (__syncthreads_or(bad || n < 0)) {
            if (tid == 0) {
                a.status[q] = kQueryErrorArg;
                atomicAdd(&a.control[kCtlErrors], 1);
            }
            for (int j = tid; j < k; j += kDenseThreads) a.out_rows[q * k + j] = -1;
            continue;
        }

        // Compaction of the buffer: T_run from the k-th largest float32 value, rule (a), then rule (b) if the buffer is
        // still more than a quarter full.
        double t_run = -1.0;  // no threshold yet: every positive value is kept
        bool failed = false;
        auto compact = [&]() {
            __syncthreads();
            const int m = ctrl[kDCount];
            if (m >= k) {
                const uint32_t kth = dense_select_kth(value, m, k, hist, ctrl);
                const double tightened = static_cast<double>(__uint_as_float(kth)) - static_cast<double>(1e-6f);  // :70
                if (tightened > t_run) t_run = tightened;
            }
            double keep_value[kDenseKeep];
            int32_t keep_row[kDenseKeep];
#pragma unroll
            for (int r = 0; r < kDenseKeep; ++r) {
                const int i = tid + r * kDenseThreads;
                keep_value[r] = i < m ? value[i] : -1.0;
                keep_row[r] = i < m ? row[i] : -1;
                if (!(keep_value[r] >= t_run)) keep_row[r] = -1;                                   // rule (a)
            }
            if (tid == 0) ctrl[kDKept] = 0;  // survivors of rule (a)
            __syncthreads();
            int mine = 0;
#pragma unroll
            for (int r = 0; r < kDenseKeep; ++r) mine += keep_row[r] >= 0;
            if (mine) atomicAdd(ctrl.at(kDKept), mine);
            __syncthreads();
            if (ctrl[kDKept] > kDenseBuffer / 4) {                                                  // rule (b)
#pragma unroll
                for (int r = 0; r < kDenseKeep; ++r) {
                    if (keep_row[r] < 0) continue;
                    int dominators = 0;
                    for (int j = 0; j < m; ++j) {  // the buffer itself is still intact: read-only here
                        const int32_t other = row[j];
                        const double v = value[j];
                        dominators += (other > keep_row[r]) & (v >= keep_value[r]);
                    }
                    if (dominators >= k) keep_row[r] = -1;
                }
            }
            __syncthreads();
            if (tid == 0) ctrl[kDCount] = 0;
            __syncthreads();
#pragma unroll
            for (int r = 0; r < kDenseKeep; ++r) {
                if (keep_row[r] < 0) continue;
                const int slot = atomicAdd(ctrl.at(kDCount), 1);
                value[slot] = keep_value[r];
                row[slot] = keep_row[r];
            }
            __syncthreads();
        };

        // scores[] of tile b: ordered float32 accumulation, a barrier between two columns (match_maker.py:46-48)
        auto scatter_tile = [&](int b) {
            for (int i = tid; i < kDenseScoreFloats; i += kDenseThreads) scores[i] = 0.f;
            __syncthreads();
            for (int64_t j0 = 0; j0 < n; j0 += kDenseChunk) {
                // stage (list begin, list end, idf) of up to kDenseChunk columns: one round of loads instead of a
                // chain of three dependent loads in front of every column
                const int width = static_cast<int>(n - j0 < kDenseChunk ? n - j0 : kDenseChunk);
                if (tid < width) {
                    const int32_t column = a.q_cols[qbase + j0 + tid];
                    const uint32_t *ptr = a.col_ptr + static_cast<int64_t>(column) * ptr_stride + b;
                    stage_begin[tid] = ptr[0] * 4u;
                    stage_end[tid] = ptr[1] * 4u;
                    stage_value[tid] = a.idf32[column];
                }
                __syncthreads();
                // the first four strides of the next column's list are fetched before the barrier that ends the
                // current column, so that only the ordered LDS updates sit between two barriers
                uint32_t next[4];
                auto fetch = [&](int j) {
                    const uint32_t begin = stage_begin[j], end = stage_end[j];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const uint32_t i = begin + tid + u * kDenseThreads;
                        next[u] = i < end ? posting_row(a.postings[i]) : static_cast<uint32_t>(kTile);
                    }
                };
                fetch(0);
                for (int j = 0; j < width; ++j) {
                    const float idf = stage_value[j];
                    const uint32_t begin = stage_begin[j], end = stage_end[j];
                    uint32_t local[4] = {next[0], next[1], next[2], next[3]};
                    if (j + 1 < width) fetch(j + 1);
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (local[u] < kTile) scores[local[u]] = scores[local[u]] + idf;  // each row at most once per list
                    for (uint32_t i0 = begin + tid + 4 * kDenseThreads; i0 < end; i0 += 4 * kDenseThreads) {
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const uint32_t i = i0 + u * kDenseThreads;
                            local[u] = i < end ? posting_row(a.postings[i]) : static_cast<uint32_t>(kTile);
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (local[u] < kTile) scores[local[u]] = scores[local[u]] + idf;
                    }
                    __syncthreads();
                }
            }
        };

        for (int b = a.n_tiles - 1; b >= 0 && !failed; --b) {
            scatter_tile(b);
            // finalise the tile (match_maker.py:50), from its last rows down, and keep what can still matter.  Before a
            // chunk of rows is looked at the buffer has room for all of it: one barrier per chunk decides, uniformly,
            // whether to compact first.
            const int64_t tile_base = static_cast<int64_t>(b) * kTile;
            const int rows_here = static_cast<int>(n_truth - tile_base < kTile ? n_truth - tile_base : kTile);
            for (int top = rows_here; top > 0 && !failed; top -= kDenseThreads) {
                if (__syncthreads_or(ctrl[kDCount] > kDenseBuffer - kDenseThreads)) {
                    compact();
                    if (ctrl[kDCount] > kDenseBuffer - kDenseThreads) failed = true;  // (a) and (b) cannot make room
                    __syncthreads();
                    if (failed) break;
                }
                const int i = top - 1 - tid;
                double v = 0.0;
                if (i >= 0) {
                    const double s = static_cast<double>(scores[i]);
                    v = s / (static_cast<double>(a.sums32[tile_base + i]) + (maxint - s));
                }
                const bool keep = i >= 0 && v > 0.0 && v >= t_run;
                const unsigned long long votes = __ballot(keep);
                if (votes != 0) {
                    const int leader = __ffsll(votes) - 1;
                    int base = 0;
                    if (lane == leader) base = atomicAdd(ctrl.at(kDCount), __popcll(votes));
                    base = __shfl(base, leader);
                    if (keep) {
                        const int slot = base + __popcll(votes & ((1ull << lane) - 1ull));
                        value[slot] = v;
                        // the caller's row index (word 6 of the record): rule (b) and :71 are about those
                        row[slot] = static_cast<int32_t>(reinterpret_cast<const uint32_t *>(a.rows + 2 * (tile_base + i))[6]);
                    }
                }
            }
            __syncthreads();
        }
        if (failed) {
            for (int j = tid; j < k; j += kDenseThreads) a.out_rows[q * k + j] = -1;
            if (tid == 0) {
                a.status[q] = kQueryErrorTies;
                atomicAdd(&a.control[kCtlErrors], 1);
            }
            __syncthreads();
            continue;
        }
        __syncthreads();
        const int m = ctrl[kDCount];
        // fast_arg_top_k: the float32 heap ends as the k largest float32(value > 0) padded with zeros (:60-67)
        double threshold = -static_cast<double>(1e-6f);           // fewer than k positive values: heap minimum 0
        if (m >= k) threshold = static_cast<double>(__uint_as_float(dense_select_kth(value, m, k, hist, ctrl))) -
                                static_cast<double>(1e-6f);       // :70
        if (threshold <= 0.0 && !a.literal_only && maxint > 0.0) {
            // every row qualifies, zeros included (with idf >= 0, sums >= a row's own total and maxint > 0 every
            // denominator is positive and no value negative): (array >= threshold).nonzero()[0][::-1][:k] = the k
            // largest indexes
            for (int j = tid; j < k; j += kDenseThreads) a.out_rows[q * k + j] = static_cast<int32_t>(n_truth - 1 - j);
        } else if (threshold <= 0.0) {
            // Negative idf values or a non-positive max_intersection_possible (both possible through the C ABI only)
            // make negative or undefined jaccards: the rows at or above a non-positive threshold are the zero rows and
            // more -- nothing the buffer holds, and the tiles are not in the caller's row order.  The row scan
            // (ds_jaccard_sync) answers the query the reference's way.
            for (int j = tid; j < k; j += kDenseThreads) a.out_rows[q * k + j] = -1;
            if (tid == 0) {
                a.status[q] = kQueryErrorTies;
                atomicAdd(&a.control[kCtlErrors], 1);
            }
        } else {
            for (int i = tid; i < m; i += kDenseThreads) {
                if (!(value[i] >= threshold)) continue;           // :71
                const int32_t t = row[i];
                int above = 0;
                for (int j = 0; j < m; ++j) above += (value[j] >= threshold) & (row[j] > t);
                if (above < k) a.out_rows[q * k + above] = t;
            }
        }
        __syncthreads();
    }
}

// ---- last resort of the literal kernel -----------------------------------------------------------------------------------
// The streaming selection above keeps at most kDenseBuffer rows in LDS.  An input with more rows than that within 1e-6 of
// the k-th value that are neither twins nor k-dominated (values rising towards LOWER row indexes in steps below 1e-9: not
// what IDF sums of real titles produce, but the reference answers it) cannot be compacted: the query is then answered the
// way the reference itself does it -- the whole float64 jaccard row (match_maker.py:50) is written to a scratch vector
// in HBM (N doubles, allocated by ds_jaccard_sync on first need), the k-th largest float32 value is selected over it
// (:60-67), and the rows at or above the threshold are collected from the last row down (:71).  A few workgroups, each with a
// scratch vector of its own, one query after the other; slow and rare by construction.  It is also what answers EVERY query
// of a call with k above the selection kernels' limit (kMaxSelectK; match_maker.py:183-190 accepts any top_n <= N).
__global__ __launch_bounds__(kDenseThreads) void ds_jaccard_rowscan_kernel(JaccardArgs a, double *row_values,
                                                                          const int32_t *queries, int n_listed)
{
    extern __shared__ __align__(16) unsigned char lds[];
    float *scores = reinterpret_cast<float *>(lds);
    uint32_t *hist = reinterpret_cast<uint32_t *>(lds + kDenseOffHist);
    const DenseControlWords ctrl{reinterpret_cast<int32_t *>(lds + kDenseOffCtrl)};
    const int tid = threadIdx.x, lane = tid & 63;
    const int k = a.k;
    const int64_t n_truth = a.n_truth;
    const int64_t ptr_stride = static_cast<int64_t>(a.n_tiles) + 1;
    row_values += static_cast<int64_t>(blockIdx.x) * n_truth;  // one scratch vector per workgroup
    for (int item = blockIdx.x; item < n_listed; item += gridDim.x) {
        const int64_t q = queries[item];
        const int64_t qbase = a.q_rowptr[q];
        const int64_t n = a.q_rowptr[q + 1] - qbase;
        const double maxint = a.q_maxint[q];
        // fast_jaccard, tile by tile: ordered float32 accumulation (a barrier between two columns), float64 finalise
        for (int b = 0; b < a.n_tiles; ++b) {
            for (int i = tid; i < kDenseScoreFloats; i += kDenseThreads) scores[i] = 0.f;
            __syncthreads();
            for (int64_t j = 0; j < n; ++j) {
                const int32_t column = a.q_cols[qbase + j];
                const float idf = a.idf32[column];
                const uint32_t *ptr = a.col_ptr + static_cast<int64_t>(column) * ptr_stride + b;
                const uint32_t begin = ptr[0] * 4u, end = ptr[1] * 4u;
                for (uint32_t i = begin + tid; i < end; i += kDenseThreads) {
                    const uint32_t local = posting_row(a.postings[i]);
                    if (local < kTile) scores[local] = scores[local] + idf;  // each row at most once per list
                }
                __syncthreads();
            }
            const int64_t tile_base = static_cast<int64_t>(b) * kTile;
            const int rows_here = static_cast<int>(n_truth - tile_base < kTile ? n_truth - tile_base : kTile);
            for (int i = tid; i < rows_here; i += kDenseThreads) {
                const double s = static_cast<double>(scores[i]);
                const uint32_t original = reinterpret_cast<const uint32_t *>(a.rows + 2 * (tile_base + i))[6];
                row_values[original] = s / (static_cast<double>(a.sums32[tile_base + i]) + (maxint - s));  // the caller's row order
            }
            __syncthreads();
        }
        // fast_arg_top_k: the heap ends as the k largest float32(value > 0), padded with zeros -- the k-th largest key
        uint32_t prefix = 0, mask = 0;
        int remaining = k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int64_t i = tid; i < n_truth; i += kDenseThreads) {
                const uint32_t key = dense_key(row_values[i]);
                if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                int cumulative = 0, digit = 0;
                for (int d = 255; d >= 0; --d) {
                    const int c = static_cast<int>(hist[d]);
                    if (cumulative + c >= remaining) { digit = d; break; }
                    cumulative += c;
                }
                ctrl[kDDigit] = digit;
                ctrl[kDRemain] = remaining - cumulative;
            }
            __syncthreads();
            prefix |= static_cast<uint32_t>(ctrl[kDDigit]) << shift;
            mask |= 255u << shift;
            remaining = ctrl[kDRemain];
            __syncthreads();
        }
        const double threshold = static_cast<double>(__uint_as_float(prefix)) - static_cast<double>(1e-6f);  // :70
        // (array >= threshold).nonzero()[0][::-1][:k], from the last row down
        int found = 0;
        int32_t *wave_counts = reinterpret_cast<int32_t *>(hist);
        for (int64_t top = n_truth; top > 0 && found < k; top -= kDenseThreads) {
            const int64_t i = top - 1 - tid;  // thread 0 holds the largest row of the chunk
            const bool qualifies = i >= 0 && row_values[i] >= threshold;
            const unsigned long long votes = __ballot(qualifies);
            if (lane == 0) wave_counts[tid >> 6] = __popcll(votes);
            __syncthreads();
            int before = 0, total = 0;
            for (int w = 0; w < kDenseThreads / 64; ++w) {
                before += w < (tid >> 6) ? wave_counts[w] : 0;
                total += wave_counts[w];
            }
            const int position = found + before + __popcll(votes & ((1ull << lane) - 1ull));
            if (qualifies && position < k) a.out_rows[q * k + position] = static_cast<int32_t>(i);
            found += total;
            __syncthreads();
        }
        if (tid == 0) {
            if (found < k) {  // match_maker.py:188-189
                a.status[q] = kQueryErrorTopN;
            } else {
                a.status[q] = kQuerySlow;
                atomicSub(&a.control[kCtlErrors], 1);
            }
        }
        if (found < k)
            for (int j = found + tid; j < k; j += kDenseThreads) a.out_rows[q * k + j] = -1;
        __syncthreads();
    }
}

// k above kMaxSelectK: every query of the call is listed for the row scan (after the argument checks the literal kernel
// would have made: a column outside [0, V) is an argument error).
constexpr int kMaxSelectK = 512;  // the selection kernels' limit: candidate buffers of 768 / 1472 / 3072 rows
__global__ __launch_bounds__(256) void ds_jaccard_mark_rowscan_kernel(JaccardArgs a)
{
    const int64_t q = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (q >= a.n_queries) return;
    const int64_t base = a.q_rowptr[q], n = a.q_rowptr[q + 1] - base;
    bool bad = n < 0;
    for (int64_t j = 0; j < n && !bad; ++j) {
        const int32_t column = a.q_cols[base + j];
        bad = column < 0 || column >= a.n_columns;
    }
    a.status[q] = bad ? kQueryErrorArg : kQueryErrorTies;
    if (bad)
        for (int j = 0; j < a.k; ++j) a.out_rows[q * a.k + j] = -1;
    atomicAdd(&a.control[kCtlErrors], 1);  // the row scan takes its queries off this count again
}

// Host side of the last resort: the queries whose status is kQueryErrorTies are answered by the row-scan kernel.
int resolve_ties(ds_index *index, hipStream_t stream, const std::vector<int32_t> &status)
{
    std::vector<int32_t> listed;
    for (size_t q = 0; q < status.size(); ++q)
        if (status[q] == kQueryErrorTies) listed.push_back(static_cast<int32_t>(q));
    if (listed.empty()) return DS_OK;
    DS_REQUIRE(index->last_args.size() == sizeof(JaccardArgs), "ds_jaccard_sync: no launch to resolve");
    JaccardArgs args;
    std::memcpy(&args, index->last_args.data(), sizeof(args));
    // workgroups: as many scratch vectors of N doubles as fit 2 GiB, at most one per listed query and per CU
    const size_t rows = static_cast<size_t>(index->n_truth);
    size_t budget = size_t(2) << 30;   // ... and within a quarter of the device memory that is free right now
    size_t free_bytes = 0, total_bytes = 0;
    if (hipMemGetInfo(&free_bytes, &total_bytes) == hipSuccess) budget = std::min(budget, free_bytes / 4);
    size_t groups = std::min<size_t>(std::min<size_t>(listed.size(), static_cast<size_t>(index->compute_units)),
                                     std::max<size_t>(1, budget / (rows * sizeof(double))));
    if (index->row_scratch.count < groups * rows) {
        int allocated = index->row_scratch.allocate(groups * rows);
        if (allocated != DS_OK && groups > 1) {   // not enough memory for that many: one vector always worked before
            groups = 1;
            allocated = index->row_scratch.allocate(rows);
        }
        if (allocated != DS_OK) return allocated;
    }
    groups = std::min(groups, index->row_scratch.count / rows);
    DeviceBuffer<int32_t> d_listed;
    DS_TRY(d_listed.upload(listed.data(), listed.size()));
    DS_TRY(ds::allow_dynamic_lds(ds_jaccard_rowscan_kernel, kDenseLdsBytes));
    DS_LAUNCH(ds_jaccard_rowscan_kernel, dim3(static_cast<unsigned>(groups)), dim3(kDenseThreads), kDenseLdsBytes, stream, args,
              index->row_scratch.ptr, d_listed.ptr, static_cast<int>(listed.size()));
    DS_HIP(hipStreamSynchronize(stream));
    // several scratch vectors (up to 2 GiB) are not kept for the life of the index: the next call that needs them allocates again
    if (groups > 1) index->row_scratch.release();
    return DS_OK;
}

int launch(ds_index *index, const int64_t *d_q_rowptr, const int32_t *d_q_cols, const double *d_q_maxint,
                  int64_t Q, int32_t k, int32_t *d_out_rows, hipStream_t stream)
{
    DS_REQUIRE(index != nullptr, "ds_jaccard_topk: null index");
    DS_REQUIRE(Q >= 0 && Q < (int64_t(1) << 31) - 4096, "ds_jaccard_topk: bad query count %lld", (long long)Q);
    DS_REQUIRE(k >= 1, "ds_jaccard_topk: k must be >= 1");
    if (k > index->n_truth) {  // match_maker.py:188-189
        set_error("top_matches.shape[0] != self.top_n (k=%d > number of truth titles=%lld)", k,
                  (long long)index->n_truth);
        return DS_E_TOP_N;
    }
    DS_HIP(hipSetDevice(index->device));
    index->last_queries = Q;
    if (Q == 0) return DS_OK;
    DS_REQUIRE(d_q_rowptr && d_q_cols && d_q_maxint && d_out_rows, "ds_jaccard_topk: null pointer");
    if (index->status.count < static_cast<size_t>(Q)) {
        int status = index->status.allocate(static_cast<size_t>(Q));
        if (status == DS_OK) status = index->slow_list.allocate(static_cast<size_t>(Q));
        if (status == DS_OK) status = index->take_order.allocate(static_cast<size_t>(Q));
        if (status == DS_OK && index->order_bins.count == 0) status = index->order_bins.allocate(2 * kOrderStride);
        if (status != DS_OK) return status;
    }
    if (!index->attributes_set) {
        DS_TRY(ds::allow_dynamic_lds(ds_jaccard_topk_kernel<false, false>, kFastLdsBytes));
        DS_TRY(ds::allow_dynamic_lds(ds_jaccard_topk_kernel<false, true>, kFastLdsBytes));
        DS_TRY(ds::allow_dynamic_lds(ds_jaccard_topk_kernel<true, false>, kFastLdsBytes));
        DS_TRY(ds::allow_dynamic_lds(ds_jaccard_topk_kernel<true, true>, kFastLdsBytes));
        DS_TRY(ds::allow_dynamic_lds(ds_jaccard_dense_kernel, kDenseLdsBytes));
        index->attributes_set = true;
    }
    JaccardArgs args;
    args.col_ptr = index->col_ptr.ptr;
    args.postings = index->postings.ptr;
    args.posting_sums = index->posting_sums.ptr;
    args.idf32 = index->idf32.ptr;
    args.sums32 = index->sums32.ptr;
    args.tile_sums_min = index->tile_sums_min.ptr;
    args.tile_sums_max = index->tile_sums_max.ptr;
    args.rows = reinterpret_cast<const uint4 *>(index->signature.ptr);
    args.sig_column = index->sig_column.ptr;
    args.row_start = index->row_start.ptr;
    args.row_cols = index->row_cols.ptr;
    args.forward_wide_start = index->forward_wide_start ? 1 : 0;
    args.forward_wide_cols = index->forward_wide_cols ? 1 : 0;
    args.nnz = index->nnz;
    args.q_rowptr = d_q_rowptr;
    args.q_cols = d_q_cols;
    args.q_maxint = d_q_maxint;
    args.out_rows = d_out_rows;
    args.status = index->status.ptr;
    args.control = index->control.ptr;
    args.slow_list = index->slow_list.ptr;
    args.take_order = nullptr;
    if (index->query_order) {  // ds_index_option("query_order", 0): the caller's order (answers do not depend on it)
        const int blocks = static_cast<int>(std::min<int64_t>((Q + 4 * kOrderThreads - 1) / (4 * kOrderThreads), 256));
        const int64_t chunk = (Q + blocks - 1) / blocks;
        DS_HIP(hipMemsetAsync(index->order_bins.ptr, 0, 2 * kOrderStride * sizeof(int32_t), stream));
        DS_LAUNCH(ds_query_order_count_kernel, dim3(blocks), dim3(kOrderThreads), 0, stream, d_q_rowptr, Q, chunk,
                  index->order_bins.ptr);
        DS_LAUNCH(ds_query_order_place_kernel, dim3(blocks), dim3(kOrderThreads), 0, stream, d_q_rowptr, Q, chunk,
                  index->order_bins.ptr, index->take_order.ptr);
        args.take_order = index->take_order.ptr;
    }
    args.phase = nullptr;
#ifdef DS_DIAGNOSTICS   // the diagnostics build's switches; the product's launch reads nothing from the environment
    if (const char *timers = getenv("DS_PHASE_TIMERS"); timers != nullptr && timers[0] == '1') {
        if (index->phase.count == 0 && index->phase.allocate(16) != DS_OK) return DS_E_HIP;
        DS_HIP(hipMemsetAsync(index->phase.ptr, 0, 16 * sizeof(unsigned long long), stream));
        args.phase = index->phase.ptr;
    }
#endif
    args.n_truth = index->n_truth;
    args.n_columns = index->n_columns;
    args.n_queries = Q;
    args.n_tiles = static_cast<int32_t>(index->n_tiles);
    args.k = k;
    args.sparse_quads = 4096;  // measured on C2: 2048..8192 is the flat optimum for 28672-row tiles (profiles/r01_i_tuning.txt)
    args.sums_min = index->sums_min;
    args.literal_only = index->literal_only ? 1 : 0;
    args.rows_sorted = index->rows_sorted ? 1 : 0;
    // first / minimum candidate count that triggers a selection: measured with the epochs (profiles/r03_tuning.txt), C2 top-10:
    // 4k|64 19.75, 4k|32 19.63, 3k|16 19.54, 2k|32 19.59, 2k|16 19.67 ms; top-100: 4k 28.89, 3k 28.67, 2k 28.38 ms
    // Round 5, on the final kernels (profiles/r05_tuning.txt section 12): a selection as soon as k candidates are buffered and again
    // at 1.5 times what the last one kept (was 3 k and 2 times): top-100 -1.9 %, C3 shape -3.2 %, C5 shape -3.1 %, C2 +-0.
    args.select_min = std::max(k, 16);
    args.select_growth = 3;
    args.n_quads = index->n_quads;

    const int grid = static_cast<int>(std::min<int64_t>(Q, int64_t(index->compute_units) * kWorkgroupsPerCu));
    DS_HIP(hipMemsetAsync(index->control.ptr, 0, kControlWords * sizeof(int32_t), stream));
    DS_HIP(hipEventRecord(index->event_begin, stream));
    if (k > kMaxSelectK) {
        // The reference accepts any top_n <= N (match_maker.py:183-190); the selection kernels' LDS buffers do not.  Every
        // query is answered the reference's own way by the row scan (ds_jaccard_sync runs it): correct, not fast.
        args.take_order = nullptr;
        index->last_args.assign(reinterpret_cast<const unsigned char *>(&args), reinterpret_cast<const unsigned char *>(&args) + sizeof(args));
        index->resolve_ties = &resolve_ties;
        DS_LAUNCH(ds_jaccard_mark_rowscan_kernel, dim3(static_cast<unsigned>((Q + 255) / 256)), dim3(256), 0, stream, args);
        DS_HIP(hipEventRecord(index->event_fast, stream));
        DS_HIP(hipEventRecord(index->event_dense, stream));
        return DS_OK;
    }
    const bool second_sample = k > kProbeMaxK && k <= 2 * kProbeMaxK;
    auto kernel = index->count_bytes ? (second_sample ? ds_jaccard_topk_kernel<true, true> : ds_jaccard_topk_kernel<true, false>)
                                     : (second_sample ? ds_jaccard_topk_kernel<false, true> : ds_jaccard_topk_kernel<false, false>);
    static_assert(sizeof(JaccardArgs) <= 512, "ds_index::kernel_args");
    index->last_args.assign(reinterpret_cast<const unsigned char *>(&args), reinterpret_cast<const unsigned char *>(&args) + sizeof(args));
    index->resolve_ties = &resolve_ties;
    if (index->kernel_args.count == 0 && index->kernel_args.allocate(512) != DS_OK) return DS_E_HIP;
    DS_HIP(hipMemcpyAsync(index->kernel_args.ptr, &args, sizeof(args), hipMemcpyHostToDevice, stream));  // pageable source: staged before the call returns
    DS_LAUNCH(kernel, dim3(grid), dim3(kThreads), kFastLdsBytes, stream, static_cast<const void *>(index->kernel_args.ptr));
    DS_HIP(hipEventRecord(index->event_fast, stream));
    DS_LAUNCH(ds_jaccard_repeats_kernel, dim3(static_cast<unsigned>((Q + 3) / 4)), dim3(256), 0, stream, args);
    DS_LAUNCH(ds_jaccard_dense_kernel, dim3(index->compute_units), dim3(kDenseThreads), kDenseLdsBytes, stream, args);
    DS_HIP(hipEventRecord(index->event_dense, stream));
    return DS_OK;
}

int collect(ds_index *index, hipStream_t stream, int64_t stats[32])
{
    DS_REQUIRE(index != nullptr, "ds_jaccard_sync: null index");
    DS_HIP(hipSetDevice(index->device));
    int32_t control[kControlWords] = {0};
    DS_HIP(hipMemcpyAsync(control, index->control.ptr, sizeof(control), hipMemcpyDeviceToHost, stream));
    DS_HIP(hipStreamSynchronize(stream));
#ifdef DS_DIAGNOSTICS
    if (index->phase.ptr != nullptr && getenv("DS_PHASE_DUMP") != nullptr) {
        unsigned long long phase[16] = {0};
        DS_HIP(hipMemcpy(phase, index->phase.ptr, sizeof(phase), hipMemcpyDeviceToHost));
        fprintf(stderr, "phase cycles:");
        for (int i = 0; i < 16; ++i) fprintf(stderr, " %d=%llu", i, phase[i]);
        fprintf(stderr, "\n");
    }
#endif
    if (stats) {
        stats[0] = control[kCtlSlowCount];
        stats[1] = control[kCtlErrors];
        stats[2] = control[kCtlExact];
        stats[3] = control[kCtlSelects];
        for (int i = 4; i < 16; ++i) stats[i] = 0;
        if (index->phase.count) {
            unsigned long long phase[16];
            DS_HIP(hipMemcpy(phase, index->phase.ptr, sizeof(phase), hipMemcpyDeviceToHost));
            for (int i = 0; i < 8; ++i) stats[4 + i] = static_cast<int64_t>(phase[i]);
        }
        stats[12] = control[kCtlSparseTiles];
        stats[13] = control[kCtlDenseTiles];
        stats[14] = control[kCtlSkippedColumns];
        std::memcpy(&stats[15], &control[kCtlBytes], sizeof(int64_t));  // bytes requested by the fast kernel
        for (int i = 0; i < 6; ++i) stats[16 + i] = control[kCtlReason + i];
        stats[22] = control[kCtlRefines];
        stats[23] = control[kCtlRawEntries];
        stats[24] = control[kCtlSurvivors];
        stats[25] = control[kCtlRawSparse];
        float fast_ms = 0.f, dense_ms = 0.f;
        if (index->last_queries > 0 && hipEventElapsedTime(&fast_ms, index->event_begin, index->event_fast) == hipSuccess &&
            hipEventElapsedTime(&dense_ms, index->event_fast, index->event_dense) == hipSuccess) {
            stats[26] = static_cast<int64_t>(fast_ms * 1000.f);
            stats[27] = static_cast<int64_t>(dense_ms * 1000.f);
        } else {
            stats[26] = stats[27] = 0;
        }
        stats[28] = control[24];  // bounds-check record of -DDS_BOUNDS_CHECK builds: site, offending index, limit
        stats[29] = static_cast<int64_t>(static_cast<uint32_t>(control[25])) | (static_cast<int64_t>(control[26]) << 32);
        stats[30] = control[27];
        stats[31] = control[kCtlRedos];
#ifdef DS_DIAGNOSTICS
        if (getenv("DS_PHASE_DUMP") != nullptr)
            fprintf(stderr, "collect experiment: touched rows %d level-1 rows %d wave-quads %d wave-quads with level-1 %d\n",
                    control[20], control[21], control[22], control[23]);
#endif
    }
    if (control[kCtlErrors] != 0 && index->last_queries > 0) {
        std::vector<int32_t> status(static_cast<size_t>(index->last_queries));
        DS_HIP(hipMemcpy(status.data(), index->status.ptr, status.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        bool unresolved = false;
        for (int32_t value : status) unresolved = unresolved || value == kQueryErrorTies;
        if (unresolved && index->resolve_ties != nullptr) {  // the literal kernel's buffer could not hold a query's near-ties
            DS_TRY(index->resolve_ties(index, stream, status));
            DS_HIP(hipMemcpy(status.data(), index->status.ptr, status.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            DS_HIP(hipMemcpy(control, index->control.ptr, sizeof(control), hipMemcpyDeviceToHost));
            if (stats) stats[1] = control[kCtlErrors];
        }
        for (size_t q = 0; q < status.size(); ++q) {
            if (status[q] == kQueryErrorTopN) {
                set_error("top_matches.shape[0] != self.top_n (query %zu)", q);
                return DS_E_TOP_N;
            }
            if (status[q] == kQueryErrorTies) {
                set_error("ds_jaccard_topk: query %zu has more than %d rows within 1e-6 of its k-th largest jaccard that "
                          "are neither twins nor dominated (literal kernel buffer)", q, 3072);
                return DS_E_INTERNAL;
            }
            if (status[q] == kQueryErrorArg) {
                set_error("ds_jaccard_topk: query %zu has a column index outside [0, V)", q);
                return DS_E_ARG;
            }
        }
    }
    return DS_OK;
}

}  // namespace DS_GEOMETRY_NAME
}  // namespace ds
