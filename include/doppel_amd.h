/*
 * doppel_amd.h -- C ABI of libdoppel_amd.so, the MI355X (gfx950) implementation of doppel-speller's
 * candidate-generation-and-scoring hot path.
 *
 * Every entry point replaces one piece of the reference's numba-jitted path; the reference interface it stands in
 * for is cited as `file:line` relative to the reference repository (mhaseebtariq/doppel-speller).  The reference is
 * Python, so the "FFI" a maintainer would add is a ctypes binding: see INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; all buffers are caller-owned and contiguous;
 *   - functions return 0 on success and a negative DS_E_* code on failure; ds_last_error() returns a
 *     thread-local human-readable message for the last failure; no exception crosses the boundary;
 *   - "host" entry points take host pointers and copy H<->D themselves (synchronous); "_device" entry points take
 *     device pointers plus a hipStream_t (as void*) and only enqueue work on that stream;
 *   - a handle is bound to one device, owns its device memory, and is NOT thread-safe (one caller at a time,
 *     like the reference's single Python thread);
 *   - there is no CPU fallback: without a usable GPU every compute entry point fails with DS_E_HIP.
 *
 * Options
 *   The ds_*_option(name, value) setters are for tests: they move launch decisions (grid caps, tile sizes, the
 *   threshold between two kernels), and no result depends on an option.  An option is process-wide unless its setter
 *   takes a handle.  0 restores the default where the option's comment below says so.  A null name, an unknown name or
 *   a value outside the stated range changes nothing and returns DS_E_ARG, with the message
 *   "<setter>: <option> = <value> out of range [low, high]" for the last of the three.
 */
#ifndef DOPPEL_AMD_H
#define DOPPEL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DS_FEATURES_COUNT 66 /* feature_engineering.py:67  FEATURES_COUNT = 6 + 4 * NUMBER_OF_WORDS_FEATURES */
#define DS_WORDS 15          /* settings.py:65            NUMBER_OF_WORDS_FEATURES */
#define DS_MAX_CHARS 255     /* settings.py:68            MAX_CHARACTERS_ALLOWED_IN_THE_TITLE */

#define DS_OK 0
#define DS_E_ARG (-1)      /* invalid argument (null pointer, bad size, unsorted posting list ...) */
#define DS_E_HIP (-2)      /* HIP runtime failure (no device, out of memory, launch failure) */
#define DS_E_TOP_N (-3)    /* fewer than k rows qualify: the reference raises 'top_matches.shape[0] != self.top_n'
                              (match_maker.py:188-189) */
#define DS_E_INTERNAL (-4)

typedef struct ds_index ds_index;   /* truth inverted index resident in HBM (MatchMaker.__init__ product) */
typedef struct ds_titles ds_titles; /* table of encoded titles resident in HBM */
typedef struct ds_timer ds_timer;   /* pair of HIP events */
typedef struct ds_problem ds_problem; /* host-side product of the native index build (next row f-3) */
typedef struct ds_forest ds_forest;   /* tree ensemble resident in HBM (next row f-4) */
typedef struct ds_trainer ds_trainer; /* gradient-boosted tree trainer resident in HBM (train.py) */
typedef struct ds_trainer_batch ds_trainer_batch; /* many such trainers over one binned matrix (cross-validation) */
typedef struct ds_query_space ds_query_space; /* truth vocabulary of the query-rows kernels, resident in HBM */

/* ---- library ---------------------------------------------------------------------------------------------------- */
const char *ds_last_error(void);
int ds_version(void);
/* Identity of the sources this binary was compiled from: the first 16 hex digits of the SHA-256 over the files of
 * csrc/ and include/ (name and contents, names ascending), passed by the build as -DDS_BUILD_ID.  The Python loader
 * refuses a library whose id differs from the sources next to it (a stale .so cannot pass for a current one). */
const char *ds_build_id(void);
int ds_device_count(int *count);
int ds_device_name(int device, char *name, size_t capacity);
/* Free and total HBM of a device in bytes right now (hipMemGetInfo): callers size their batches with it. */
int ds_device_memory(int device, int64_t *free_bytes, int64_t *total_bytes);

/* ---- truth index:  MatchMaker.__init__ product (match_maker.py:99-107) ------------------------------------------ */
/* rowptr[V+1], truth_idx[nnz]: the V x N inverted index of match_maker.py:122-133 in CSR form (row g = n-gram
 * column g, entries = ascending truth row indexes).  idf32[V] = the constant per-posting value of :130.
 * sums32[N] = sums_matrix_truth of :102,174.  The per-posting value array of the reference is not stored.
 * The host part (tiling, signatures, duplicate ranks) runs on DS_HOST_THREADS threads (default: the CPUs of the
 * process, at most 32); DS_BUILD_LOG=1 prints its phase times on stderr. */
int ds_index_create(const int64_t *rowptr, const int32_t *truth_idx, const float *idf32, const float *sums32,
                    int64_t V, int64_t N, int device, ds_index **out);
/* The same index built on the device (ds_index_build.hip): same arguments, same checks, same error codes and
 * messages, and for the same input and tile size every array and scalar of the index equals what ds_index_create
 * uploads, byte for byte (radix sorts and scans only: no position depends on the arrival order of an atomic).  It
 * uploads rowptr, truth_idx, idf32 and sums32 and derives the rest in HBM; only the choice of the signature columns
 * (from rowptr) and the range test of idf32 stay on the host.  A posting list that is not strictly ascending within
 * [0, N) is refused by a kernel of its own before any other kernel reads the rows.  Returns synchronised.
 * Honours DS_SORT_ROWS=0 and DS_GEOMETRY as ds_index_create does.
 * Limits: nnz >= 2^32 - 1 needs 64-bit row starts, which only ds_index_create builds: DS_E_ARG.  Peak scratch, with
 * M = nnz, T = tiles, K = ceil(max(M, N) / 2048):
 *   16 max(M, N) + 1024 K + 8 M + 52 N + 4 V (T + 1) + 8 V + 8 ceil(max(M + 1, 256 K, V (T + 1), N + 1) / 2048) + 40 bytes
 * (two sort buffers, the digit table, truth_idx and the even-row scan, the per-row arrays, the cell starts, rowptr, the
 * scan spine).  Scratch plus the index's own arrays (postings at their upper bound M / 4 + 2 min(M, V T) quads) plus
 * 64 MiB are checked against the free HBM before anything is allocated or launched: DS_E_HIP, nothing left allocated. */
int ds_index_create_device(const int64_t *rowptr, const int32_t *truth_idx, const float *idf32, const float *sums32,
                           int64_t V, int64_t N, int device, ds_index **out);
/* Copies one array of an index (built either way) to the host.  name: "col_ptr" uint32[V][tiles + 1], "postings" and
 * "posting_sums" uint16[4 * quads], "records" uint32[N][8], "sums32" float[N + 8] (internal order, 8 zeros behind),
 * "tile_sums_min" / "tile_sums_max" float[tiles], "sig_column" int8[V], "row_start" uint32[N + 1] (int64 when
 * scalars[5] = 8), "row_cols" uint16[nnz] (int32 when scalars[6] = 4), "idf32" float[V], and "scalars" int64[8] =
 * n_tiles, n_quads, bits of sums_min, literal_only, rows_sorted, bytes of a row start, bytes of a forward column, tile
 * rows.  *bytes is always set to the array's size; an unknown name, a null dst or capacity < *bytes gives DS_E_ARG. */
int ds_index_read(const ds_index *index, const char *name, void *dst, size_t capacity, size_t *bytes);
/* Switches of the device build, for tests.  "duplicate_hash_bits" (0..64, default 0 = all): ds_index_create_device
 * keeps only that many low bits of both row hashes of the duplicate ranks, so that distinct rows share hash groups
 * and the rule "a member is compared with the group's largest row, never with another member" decides the ranks. */
int ds_index_build_option(const char *name, int64_t value);
void ds_index_destroy(ds_index *index);
/* Host-only part of ds_index_create, exported for tests: rank_out[t] = number of truth rows with the same column set
 * and the same sums32 bits as row t but a larger row index (saturating at 65535).  fast_arg_top_k returns the k
 * LARGEST ROW INDEXES at or above its threshold (match_maker.py:71): a row of rank >= k can never be returned. */
int ds_index_duplicate_ranks(const int64_t *rowptr, const int32_t *truth_idx, const float *sums32, int64_t V, int64_t N,
                             uint16_t *rank_out);
/* Host-only, for tests: FNV-1a digests of the arrays ds_index_create uploads, built for tiles of `tile_rows` rows.
 * digest[0..5] = list pointers, postings, per-posting info, row records, tile minima, signature columns; [6] = posting
 * quads; [7] = 1 when the index would be served by the literal kernel alone.  Must not depend on DS_HOST_THREADS. */
int ds_index_image_digest(const int64_t *rowptr, const int32_t *truth_idx, const float *idf32, const float *sums32,
                          int64_t V, int64_t N, int64_t tile_rows, uint64_t digest[8]);
/* Diagnostics switches of an index.  "count_bytes" (0 / 1): the next ds_jaccard_topk* calls run the instantiation of
 * the fast kernel that also counts the bytes it requests from global memory (reported by ds_jaccard_sync, stats[15]);
 * same work, same results, about 3 % slower -- bench.py runs it once outside the timed region for its roofline.
 * "query_order" (1 / 0, default 1): the fast kernel's work queue hands out the queries with most columns first (a device-side
 * counting sort; 0 = the caller's order; answers do not depend on it).
 * The product's launches read NOTHING from the environment.  Environment read by ds_index_create / the host builds only
 * (tests and A/B measurements): DS_HOST_THREADS, DS_BUILD_LOG=1, DS_SORT_ROWS=0, DS_GEOMETRY=narrow|wide.  The phase timers
 * (DS_PHASE_TIMERS=1 / DS_PHASE_DUMP) exist in -DDS_DIAGNOSTICS builds only. */
int ds_index_option(ds_index *index, const char *name, int64_t value);
/* info[0]=N info[1]=V info[2]=nnz info[3]=tile size info[4]=tiles info[5]=device bytes info[6]=padded postings
 * info[7]=bytes of the forward index (row starts uint32 while nnz < 2^32, columns uint16 while V <= 65536), part of info[5] */
int ds_index_info(const ds_index *index, int64_t info[8]);

/* ---- Jaccard top-k:  fast_jaccard + fast_arg_top_k (match_maker.py:16-71) behind get_closest_matches (:192-203) - */
/* For each query q: columns q_cols[q_rowptr[q] .. q_rowptr[q+1]) in ACCUMULATION ORDER (the order of
 * matrix_non_zero_columns[row], :118), q_maxint[q] = max_intersection_possible (:197, float64).
 * out_rows[q*k .. q*k+k) = truth ROW indexes in descending row-index order, exactly
 * `(array >= threshold).nonzero()[0][::-1][:k]` of :71 (the title_id mapping of :190 is the caller's).
 * Inputs the reference cannot produce are still answered as its loop would answer them (by the literal kernel): a
 * column listed twice in a query is added twice, more than 128 columns, a q_maxint below the columns' idf total. */
int ds_jaccard_topk(ds_index *index, const int64_t *q_rowptr, const int32_t *q_cols, const double *q_maxint,
                    int64_t Q, int32_t k, int32_t *out_rows);
/* Same with every array already in HBM; enqueues on `stream` and returns without synchronising.
 * q_nnz = q_rowptr[Q].  Errors detected on the device (DS_E_TOP_N ...) are reported by ds_jaccard_sync(). */
int ds_jaccard_topk_device(ds_index *index, const int64_t *d_q_rowptr, const int32_t *d_q_cols,
                           const double *d_q_maxint, int64_t Q, int32_t k, int32_t *d_out_rows, void *stream);
/* Waits for `stream`, returns the status of the last ds_jaccard_topk_device on this index;
 * stats[0]=queries answered by the exact dense kernel, stats[1]=queries in error, stats[2]=candidates evaluated
 * exactly (total), stats[3]=threshold selections run (total), stats[4..11]=shader-clock sums per kernel phase
 * (setup, list pointers, scatter, scan, select, exact stage, dense hand-over; only with DS_PHASE_TIMERS=1),
 * stats[12]=tiles handled sparsely, stats[13]=tiles scanned densely, stats[14]=skipped (non-essential) columns
 * summed over queries, stats[16..21]=queries handed to the dense kernel by reason (unsupported shape, work items,
 * candidate overflow in a sparse tile, in a dense tile, ties after pruning, fewer than k positive rows),
 * stats[22..25]=refine passes / raw entries / survivors / raw entries from sparse tiles (diagnostics),
 * stats[26]=duration of ds_jaccard_topk_kernel in microseconds (HIP events on the launch stream),
 * stats[27]=duration of ds_jaccard_dense_kernel in microseconds, stats[28..30]=first out-of-range index a
 * -DDS_BOUNDS_CHECK build caught (site, index, limit; all 0 otherwise), stats[31]=epochs of sparse tiles that were
 * processed again because the candidate buffer overflowed (the threshold is tightened first; results unaffected). */
int ds_jaccard_sync(ds_index *index, void *stream, int64_t stats[32]);
/* Per-query status of the last call (after synchronising `stream`): 0 = answered by the fast kernel, 1 = handed to and
 * answered by the literal kernel, 2 = fewer than k rows qualified (DS_E_TOP_N), 3 = bad column index (DS_E_ARG),
 * (4 is transient: a query whose near-ties did not fit the literal kernel's LDS buffer; ds_jaccard_sync answers it with a
 * full-row scan through a float64[N] scratch vector in HBM, allocated on first need, and the status becomes 1.)
 * stats[15] of ds_jaccard_sync = bytes requested by the fast kernel (only with ds_index_option "count_bytes"). */
int ds_jaccard_status(ds_index *index, void *stream, int32_t *status, int64_t Q);

/* ---- Levenshtein / features:  fast_levenshtein_ratio + construct_features (feature_engineering.py:25-169) ------- */
/* The 9-argument gufunc of feature_engineering.py:69-80 without the `dummy` argument: rows of q_enc / t_enc are
 * `stride` bytes apart (255 in predict.py:199-202), out = float32[n*66] written in place.  Host pointers: the pairs
 * travel in chunks of 16384 through pinned staging buffers (only the titles' own bytes, lengths and word counts are
 * shipped, not the padding), up to 8 host threads with a stream each overlap copy-in / kernel / copy-out; the staging
 * buffers (<= 110 MB pinned per device) are allocated by a device's first call and kept.  Calls for one device are
 * serialised by that device's mutex. */
int ds_construct_features(const uint8_t *q_len, const uint8_t *t_len, const uint8_t *q_enc, const uint8_t *t_enc,
                          const uint32_t *t_word_counts, uint8_t space_code, uint32_t n_truth, int64_t n,
                          int64_t stride, int device, float *out);

/* Encoded titles uploaded once (FeatureEngineering.encode_title rows, feature_engineering.py:298-307, and for a
 * truth table get_truth_words_counts rows, :309-319; word_counts may be NULL for a query table). */
int ds_titles_create(const uint8_t *enc, int64_t stride, const uint8_t *len, const uint32_t *word_counts, int64_t n,
                     int device, ds_titles **out);
void ds_titles_destroy(ds_titles *titles);
/* "truth_records" (default 1): the indexed entry points keep, per row of a TRUTH table, what construct_features derives from
 * the truth title alone (word boundaries, idf_s, ranks: feature_engineering.py:110-123,152-158) -- 160 bytes of HBM per row,
 * built on the first call that names (number_of_truth_titles, space_code).  0 frees them: everything per pair again. */
int ds_titles_option(ds_titles *titles, const char *name, int64_t value);
/* Pairs given as (query row, truth row) indexes into two tables: out[i] = construct_features(q[pair_q[i]],
 * t[pair_t[i]]).  Host pointers for pair_q / pair_t / out. */
int ds_construct_features_indexed(ds_titles *queries, ds_titles *truth, const int32_t *pair_q, const int32_t *pair_t,
                                  uint8_t space_code, uint32_t n_truth, int64_t n, float *out);
/* Device-resident variant for the fused pipeline: d_pair_t = the top-k rows written by ds_jaccard_topk_device,
 * pair i belongs to query row q_first + i / k when d_pair_q is NULL.  d_out = float32[n*66] in HBM.
 * A pair whose query row or truth row lies outside its table (negative, or >= the table's rows: e.g. the -1 rows of a
 * top-k that failed) is not an error: its 66 outputs are the quiet NaN 0x7fc00000, and no title is read for it.
 * The first call that names (n_truth, space_code) on a truth table builds its truth records on `stream` and waits for
 * them, which synchronises `stream` once (so does a device's first features launch of the process, for the ratio table):
 * they are then complete for a launch on any stream.  After that a call only enqueues on `stream`. */
int ds_construct_features_indexed_device(ds_titles *queries, ds_titles *truth, const int32_t *d_pair_q,
                                         const int32_t *d_pair_t, int64_t q_first, int32_t k, uint8_t space_code,
                                         uint32_t n_truth, int64_t n, float *d_out, void *stream);
/* fast_levenshtein_ratio (feature_engineering.py:25-63) for n independent pairs of code strings:
 * a = a_chars[a_off[i] .. a_off[i+1]), b likewise; out[i] = ratio (uint8).  Host pointers.
 * method 0 = bit-parallel LCS kernel (exact uint8-wrap DP where lengths require it), 1 = anti-diagonal DP kernel. */
int ds_levenshtein_ratio_batch(const uint8_t *a_chars, const int64_t *a_off, const uint8_t *b_chars,
                               const int64_t *b_off, int64_t n, int method, int device, uint8_t *out);
/* fast_levenshtein_ratio(a, b) (feature_engineering.py:25-63) for ONE pair of code strings on device 0, as SURVEY.md 8b
 * lists it ("for tests"): returns the reference's uint8 result (0..255) or a negative DS_E_* code.  A one-pair wrapper
 * over ds_levenshtein_ratio_batch (method 0): a kernel launch and two copies per call -- a test entry, not a hot path. */
int ds_levenshtein_ratio(const uint8_t *a, int la, const uint8_t *b, int lb);

/* ---- next row: Prediction._find_close_matches (predict.py:140-183) -------------------------------- */
/* For query row q (q_first + q in the query table) and its k candidate truth rows pair_t[q*k .. q*k+k):
 * ratios[q*k+j] = Prediction._get_levenshtein_ratio(query, candidate) (predict.py:147-156: length pre-filter,
 * common.levenshtein_ratio = int(round(python-Levenshtein ratio * 100)), token-sort fallback common.py:165-167);
 * best_row[q] = the candidate with the highest ratio > threshold if exactly one reaches it (predict.py:172-176), else
 * -1.  sort_key[256] = order of the character codes under Python's sorted() (the code points).  python-Levenshtein is
 * not part of the reference tree: its published definition is restated (parity pinned against the tests' CPU
 * restatement only).
 * ds_close_matches_device: the rows are in HBM, d_best_row may be NULL (ratios only); enqueued on `stream`.  A candidate
 * row outside the truth table (negative or >= its rows), or a query row outside the query table, has ratio 0 and is
 * never the best row (threshold >= 0: the best ratio has to exceed it).  Two empty titles have ratio 100 (the reference
 * divides by zero there). */
int ds_close_matches(ds_titles *queries, ds_titles *truth, const int32_t *pair_t, int32_t k, int64_t n_queries,
                     uint8_t space_code, const uint8_t *sort_key, int32_t threshold, uint8_t *ratios,
                     int32_t *best_row);
int ds_close_matches_device(ds_titles *queries, ds_titles *truth, const int32_t *d_pair_t, int64_t q_first, int32_t k,
                            int64_t n_queries, uint8_t space_code, const uint8_t *d_sort_key, int32_t threshold,
                            uint8_t *d_ratios, int32_t *d_best_row, void *stream);

/* ---- next row f-2: the pair list between the fuzzy step and the model, on the device (predict.py:172-183,195-204) ---
 * d_best_row[q] >= 0 marks a query the fuzzy step matched (ds_close_matches_device).  The remaining queries keep
 * their order; each contributes its k candidate rows d_rows[q*k .. q*k+k) in order: d_pair_q / d_pair_t (room for
 * n_queries * k entries) receive the (query row, truth row) index pairs for ds_construct_features_indexed_device,
 * query rows offset by q_first.  d_counts = int64[ds_remaining_pairs_counts_size(n_queries)]: [0] = remaining
 * queries, [1] = pairs, the rest is scratch.  Asynchronous on `stream`. */
int64_t ds_remaining_pairs_counts_size(int64_t n_queries);
int ds_remaining_pairs_device(const int32_t *d_best_row, const int32_t *d_rows, int64_t n_queries, int32_t k,
                              int64_t q_first, int32_t *d_pair_q, int32_t *d_pair_t, int64_t *d_counts, void *stream);
/* predict.py:246-252 for n_remaining queries of k consecutive pairs each: d_match_query[r] = the query row of group
 * r, d_match_row[r] = the truth row of its maximum prediction when that maximum is above `threshold`
 * (PREDICTION_PROBABILITY_THRESHOLD, settings.py:76) and a single pair holds it, else -1.  Asynchronous on `stream`. */
int ds_select_matches_device(const int32_t *d_pair_q, const int32_t *d_pair_t, const float *d_predictions,
                             int64_t n_remaining, int32_t k, float threshold, int32_t *d_match_query,
                             int32_t *d_match_row, void *stream);

/* ---- ranked matches: the best n of a query's k candidates, in order, with their scores ---------
 * The project's own rule; the reference keeps one answer per title (predict.py:239-242).  Per query q, over the
 * candidates j = 0 .. k-1 with truth row c_j = d_rows[q*k + j], probability p_j = d_predictions[q*k + j] (finite and
 * non-negative) and ratio r_j = d_ratios[q*k + j]:
 *   head   d_exact_row[q] when >= 0 (stage 1), else d_best_row[q] when >= 0 (stage 2), else none.  It takes slot 0 with
 *          probability 1.0 (what the reference stores for exact and close matches, predict.py:108,179) and the ratio of
 *          the first candidate that equals it; absent from the candidates (twins of rank >= k are left out of the
 *          index) an exact head has ratio 100 and a close head ratio 0;
 *   rest   every candidate with 0 <= c_j < n_truth and c_j != head, stage 3, ordered by the float32 BITS of p_j
 *          descending, then j ascending (a pure function of the inputs).  Other candidates are skipped;
 *   slots  the list is cut to n; an unfilled slot holds row -1, probability quiet NaN (0x7fc00000), ratio 0, stage 0.
 * The outputs are [n_queries][n] arrays in HBM; every slot is written.  d_exact_row and d_best_row may each be NULL ("no
 * such stage"); after ds_close_matches_device and ds_exact_matches_device on the same d_best_row, pass both.  DS_E_ARG: any
 * other null pointer, k < 1, n outside 1..k, a negative count.  n_queries == 0 launches nothing.  Any k works: up to
 * "lds_keys" candidates are ranked in LDS by counting, longer lists by n rounds of selection from HBM, with the same
 * result.  ds_rank_option("lds_keys", v), v in [0, 512] (default 512), is for tests: it moves that limit (0: always
 * select).  Asynchronous on `stream`. */
int ds_rank_matches_device(const int32_t *d_rows, const float *d_predictions, const uint8_t *d_ratios,
                           const int32_t *d_exact_row, const int32_t *d_best_row, int64_t n_queries, int32_t k,
                           int32_t n, int64_t n_truth, int32_t *d_out_row, float *d_out_probability,
                           uint8_t *d_out_ratio, int8_t *d_out_stage, void *stream);
int ds_rank_option(const char *name, int64_t value);

/* ---- exhaustive matches: the best n rows of the WHOLE truth table by the model ------------------
 * The project's own stage (the reference's README promises it, its code scores the Jaccard top_n only): the model alone,
 * with no candidate stage in front and no exact or close override.  Per query, over every truth row t with probability
 * p_t (finite and non-negative):
 *   key    (float32 BITS of p_t << 32) | (0xffffffff - t): never 0 for a row below 2^31, so 0 stands for "empty";
 *   best   the n largest keys, descending: by the probability's bits descending, then by t ascending.  The keys of a
 *          query are distinct, so the result is a pure function of the inputs, whatever the tiling or the schedule;
 *   slots  an unfilled slot (fewer than n truth rows) holds row -1 and probability quiet NaN (0x7fc00000).
 * n lies in 1..64.  DS_E_ARG, with nothing launched: a null pointer or handle, n outside 1..64, a negative count.
 *
 * ds_exhaustive_fold_device: the fold alone, on probabilities of the caller's (the entry the kernel tests drive).
 * d_probabilities is [n_queries][tile_rows] in HBM, column j of every query being truth row row_first + j;
 * d_running is [n_queries][n] keys in HBM, descending, 0 = empty (all 0 before the first fold).  After the call it holds
 * the n largest keys of what it held and the tile's.  Every truth row is folded once; the order and the sizes of the tiles
 * do not matter.  row_first + tile_rows <= 2^31.  n_queries == 0 or tile_rows == 0 launches nothing.  Enqueued on
 * `stream`; a tile of more than 4096 - n rows takes partial lists in HBM, allocated by the call and freed before it
 * returns, behind a synchronisation of `stream`. */
int ds_exhaustive_fold_device(const float *d_probabilities, int64_t n_queries, int64_t tile_rows, int64_t row_first,
                              int32_t n, uint64_t *d_running /* [n_queries][n] keys, 0 = empty */, void *stream);
/* d_out_row[q*n + s] / d_out_probability[q*n + s] = the row and the probability of key s of query q, (-1, quiet NaN)
 * for an empty key.  Every slot is written.  n_queries == 0 launches nothing.  Asynchronous on `stream`. */
int ds_exhaustive_finish_device(const uint64_t *d_running, int64_t n_queries, int32_t n, int32_t *d_out_row,
                                float *d_out_probability, void *stream);
/* The whole stage, for rows [q_first, q_first + n_queries) of `queries` against all rows of `truth` (a table with word
 * counts): per tile of pairs -- consecutive queries x consecutive truth rows -- a pair list, the features of
 * ds_construct_features_indexed_device (space_code, n_truth as there), the probabilities of ds_forest_predict_device and
 * the fold; then ds_exhaustive_finish_device into d_out_row / d_out_probability, [n_queries][n] in HBM.  At no time more
 * than one tile of pairs exists.  The workspace (276 bytes per pair of a tile, 8 n bytes per query, the fold's partial
 * lists) is allocated by the call and freed before it returns: `stream` is synchronised at the end.  A tile holds
 * "tile_pairs" pairs at most: by default what a quarter of the HBM free at the call holds, and no more than 2^24 pairs
 * (1.1e9 features; 4.7 GB).  n_queries == 0 launches nothing and writes nothing.
 * ds_exhaustive_option("tile_pairs", v), v in [0, 2^24], is for tests: the pairs of a tile, 0 = the default.  The
 * result does not depend on it. */
int ds_exhaustive_rank_device(ds_titles *queries, ds_titles *truth, ds_forest *forest, int64_t q_first,
                              int64_t n_queries, int32_t n, uint8_t space_code, uint32_t n_truth,
                              int32_t *d_out_row, float *d_out_probability, void *stream);
int ds_exhaustive_option(const char *name, int64_t value);   /* "tile_pairs": for tests, 0 = default */

/* ---- threshold sweep: the accuracy counters of cli.py:107-120 for a grid of both thresholds ----
 * ds_close_parts_device: the ratio of ds_close_matches_device taken apart, so that it can be read at any integer
 * threshold t afterwards: value(t) = 0 when t > d, r when r > t, else s, and the pair counts as close iff value(t) > t.
 * d = the floor of the length pre-filter's value (100 for two empty titles), r = the rounded ratio of the titles, s = that
 * of the token-sorted titles; uint8[n_queries * k] each in HBM, pair i = (query row q_first + i / k, truth row d_rows[i]).
 * What no t in [t_min, t_max] can read is not computed and written as 0: r and s when d < t_min, s when r > t_max.  A row
 * outside either table gives 0, 0, 0.  0 <= t_min <= t_max <= 100.  Asynchronous on `stream`. */
int ds_close_parts_device(ds_titles *queries, ds_titles *truth, const int32_t *d_rows, int64_t q_first, int32_t k,
                          int64_t n_queries, uint8_t space_code, const uint8_t *d_sort_key, int32_t t_min, int32_t t_max,
                          uint8_t *d_d, uint8_t *d_r, uint8_t *d_s, void *stream);
/* ds_threshold_sweep_device: for every cell (t = d_lev[i], u = d_prob[j]) the decision rule of Prediction on n_queries
 * queries of k candidates each, and d_counts[(i * U + j) * 4 + c] += the queries of outcome c.  A stage's row counts
 * when it is >= 0:
 *   exact  d_exact[q];
 *   close  the maximum value(t) among the candidates with value(t) > t, and d_rows of its holder when there is one only;
 *   model  the maximum of d_predictions[q * k ..) (float32; a NaN in front: none, behind it: passed over), and d_rows of
 *          its holder when there is one only and the maximum is > u (float32 compare);
 *   none   -1.
 * c = 0: a prediction equal to d_actual_row[q]; 1: a prediction that differs; 2: none and d_actual_row[q] < 0; 3: none
 * and d_actual_row[q] >= 0.  The counters are ADDED to (integer atomics: any order gives the same sums), so the chunks of
 * one evaluation accumulate; the caller zeroes them first.  d_lev: 1..101 integers in [0, 100], strictly ascending;
 * d_prob: 1..256 finite floats, strictly ascending; both in HBM, read back and checked by the call (one synchronisation
 * of `stream`), DS_E_ARG with nothing launched otherwise, as for k < 1 or a null pointer.  n_queries == 0 launches
 * nothing.  The kernel is enqueued on `stream`.
 * ds_sweep_option("queries_per_group", v) is for tests: the queries per workgroup below the cap of 256 workgroups
 * (0 = the default, 64); the result does not depend on it. */
int ds_threshold_sweep_device(const int32_t *d_rows, const uint8_t *d_d, const uint8_t *d_r, const uint8_t *d_s,
                              const float *d_predictions, const int32_t *d_exact, const int32_t *d_actual_row,
                              int64_t n_queries, int32_t k, const int32_t *d_lev, int32_t T, const float *d_prob,
                              int32_t U, int64_t *d_counts, void *stream);
int ds_sweep_option(const char *name, int64_t value);

/* ---- sweep records and the paired bootstrap of every cell ("Bootstrap of the cells") ------------
 * ds_sweep_records_device: the inputs, the argument checks and the read-back check of the grid of
 * ds_threshold_sweep_device, but nothing is counted: d_records[q * T + i] (uint16, a query's T records contiguous) holds
 * what the rule leaves of query q at threshold d_lev[i] for EVERY u.  The encoding is the contract between this kernel,
 * ds_sweep_bootstrap_device and the tests' oracle:
 *   bits 0..2   0..3: the same outcome in every cell, in the numbering of bootstrap.ACCURACY_CODES (0 correctly not
 *               found, 1 incorrectly matched, 2 incorrectly not found, 3 correctly matched);
 *               4: no actual row        outcome 1 at the cells u < pos, 0 from pos on;
 *               5: the model's row is the actual one      3 below pos, 2 from pos on;
 *               6: the model's row is another one         1 below pos, 2 from pos on;
 *               7 never occurs;
 *   bits 3..15  pos for 4, 5 and 6 (the number of d_prob values below the model's maximum), 0 for 0..3.  A flip whose
 *               pos is U has the same outcome in every cell and is written as that outcome (1 or 3), so a record is a
 *               function of the U outcomes alone and this kernel writes pos in 1..U - 1.
 * No stream parameter: the kernel is enqueued on the null stream, where every stage of Prediction runs, and the call
 * synchronises that stream once, for the grid check.  n_queries == 0 launches nothing.
 *
 * ds_sweep_bootstrap_device: the outcome counts of every cell under a paired bootstrap of the n titles by unit.
 * d_records: uint16[n][T] as above; d_unit: int32[n], the unit of every title in [0, n_units), or null: every title its
 * own unit, n_units == n.  Replicate b draws n_units units, draw k the unit
 *   j(b, k) = (x * n_units) >> 64, x = the first kept output of the stream of (seed, DS_BOOTSTRAP_PURPOSE_DRAW, (b << 32) | k),
 * exactly the draw of ds_bootstrap_counts_device, and a drawn unit adds all its titles (a unit without titles adds
 * nothing); the baseline takes every unit once.  d_counts: int64[n_boot][T][U][4], d_baseline: int64[T][U][4], the four
 * classes in the numbering above; every element is written (nothing is added to), so the caller need not zero them.
 * So d_counts[b][i][j] is what ds_bootstrap_counts_device gives for the outcome codes of cell (i, j), bit for bit.
 * Limits: n < 2^31, n_boot in 1..65536, T <= 101, U <= 256, and n_units x the largest unit < 2^32 (what one replicate
 * can add to a 32-bit counter).  DS_E_ARG with d_counts and d_baseline untouched for these, for a record with low bits 7,
 * with a pos other than 0 on 0..3 or outside 1..U on 4..6, and for a unit outside [0, n_units).
 * No stream parameter: everything is enqueued on the null stream.  The call synchronises it once for the error counters
 * of its check kernel and, with units, once more at the end, because the member lists it built are freed on return.
 * ds_sweep_option, for tests, no result depends on them: "bootstrap_tile" = thresholds per wave (0: what 16 KiB of LDS
 * per wave hold, 64 at the most), "bootstrap_max_blocks" = cap of the grid (0: 4096), "bootstrap_replicates_per_group" =
 * replicates per workgroup (0: 4). */
int ds_sweep_records_device(const int32_t *d_rows, const uint8_t *d_d, const uint8_t *d_r, const uint8_t *d_s,
                            const float *d_predictions, const int32_t *d_exact, const int32_t *d_actual_row,
                            int64_t n_queries, int32_t k, const int32_t *d_lev, int32_t T, const float *d_prob, int32_t U,
                            uint16_t *d_records);
int ds_sweep_bootstrap_device(const uint16_t *d_records, int64_t n, int32_t T, int32_t U, const int32_t *d_unit,
                              int64_t n_units, int32_t n_boot, uint64_t seed, int64_t *d_counts, int64_t *d_baseline);

/* ---- duplicate groups: the connected components of the truth set under its own links -----------
 * The project's own stage: the truth table is its own query table, the stages above score every row against its k
 * candidates, and the rows that score as one entity are joined into groups.  The state is a union-find forest
 * int32 d_parent[n_truth] in HBM, owned by the caller: d_parent[i] <= i always, d_parent[i] == i marks a root.  n_truth
 * is below 2^31.  All calls of one run go on one stream.
 *
 * ds_duplicate_begin_device: d_parent[i] = i and d_counts[0..3) = 0.  With n_truth == 0 no kernel is launched; the
 * counters are zeroed all the same (a memset on `stream`), so that what the caller reads back is defined.
 *
 * ds_duplicate_links_device: query rows [q_first, q_first + n_queries) of the truth table, slot j of query q (absolute
 * row a = q_first + q) holding t = d_rows[q*k + j]:
 *   skipped  t < 0, t >= n_truth or t == a;
 *   close    d_ratios[q*k + j] > levenshtein_threshold;
 *   model    d_predictions != NULL and d_predictions[q*k + j] > probability_threshold (float32; a NaN is not above);
 *   reason   d_reason[q*k + j] = close | model << 1, 0 for a skipped slot; every slot is written (d_reason may be NULL);
 *   links    a non-zero reason joins a and t; when d_exact != NULL and e = d_exact[q] has 0 <= e < n_truth and e != a, a
 *            and e are joined as well (identical titles meet in the last row that holds them: twins form one group
 *            even where the index left twins of rank >= k out of the candidates);
 *   counts   d_counts[0] += the exact links, [1] += the slots with close, [2] += the slots with model and not close
 *            (integer atomics: any order gives the same sums).
 * Joining is lock-free: both roots are found with path halving and the LARGER root is hooked under the smaller one by
 * one compare-and-swap, tried again from the value it returns when it loses.  The root of a component therefore ends as
 * its lowest row, whatever the schedule, the chunking or the order of the links.  Calls accumulate into d_parent.
 * DS_E_ARG, with nothing launched: any other null pointer, k < 1, a negative count, rows that are not rows of the truth
 * table (q_first + n_queries > n_truth), a threshold outside [0, 100], a probability threshold that is not finite.
 * n_queries == 0 or n_truth == 0 launches nothing.
 *
 * ds_duplicate_finish_device: d_label[i] = the root of i (its group's lowest row), d_size[i] = the rows with that label;
 * every entry of both is written.  d_parent is compressed on the way (every entry points at its root): the groups stay
 * the same and more links may follow.
 *
 * ds_duplicates_option("max_blocks", v), v in [0, 2^20], is for tests: the cap of every grid of this stage, which
 * strides beyond it (0 = the default, 2048); the result does not depend on it.  Asynchronous on `stream`. */
int ds_duplicate_begin_device(int32_t *d_parent, int64_t n_truth, int64_t *d_counts, void *stream);
int ds_duplicate_links_device(const int32_t *d_rows, const uint8_t *d_ratios, const float *d_predictions,
                              const int32_t *d_exact, int64_t q_first, int64_t n_queries, int32_t k, int64_t n_truth,
                              int32_t levenshtein_threshold, float probability_threshold, int32_t *d_parent,
                              uint8_t *d_reason, int64_t *d_counts, void *stream);
int ds_duplicate_finish_device(int32_t *d_parent, int64_t n_truth, int32_t *d_label, int32_t *d_size, void *stream);
int ds_duplicates_option(const char *name, int64_t value);

/* ---- one-to-one matches: each truth row given to one title at most ---------------------------------
 * The project's own stage: the ranked slots of ds_rank_matches_device, for ALL titles of a call (n_total < 2^31, n slots
 * each), turned into one matching by deferred acceptance with the titles proposing.
 *
 * Edges.  Slot s of title q holding t = row[q*n + s] is an edge to truth row t when
 *   0 <= t < n_truth;
 *   its stage is 1 (exact) or 2 (close); or its stage is 3, its probability > probability_threshold (float32 compare; a NaN
 *   is not above) and the probability's sign bit is clear;
 *   no earlier slot of q is an edge to t (ds_rank_matches_device never repeats a row; a caller of this ABI can).
 * Every other slot is no edge.  The key of an edge, uint64, 0 = no edge:
 *   class << 62 | payload << 31 | (2^31 - 1 - q)      q: the title's number in the whole call
 *   class 3 / 2 / 1 for stage 1 / 2 / 3, payload 0 / the ratio (0..100) / the float32 bits of the probability (< 2^31).
 * A truth row prefers the larger key: exact over close over model, the higher ratio or probability inside a class, the
 * earlier title on equal scores.  Two edges into one row come from different titles, so the keys at a row are distinct.
 * A title prefers its edges in slot order.  The result is the title-optimal stable matching: no edge (q, t) outside it has
 * q preferring t to what it got (or q unmatched) and t's key for q above the key t holds (or t free).  It is unique, and it
 * does not depend on the order of the proposals, hence not on the schedule, the chunking or the options below.  Where a
 * title's edges are in descending (class, payload) order -- ds_rank_matches_device's are -- it equals the greedy matching:
 * all edges by (class, payload) descending, q ascending, slot ascending, an edge taken when its title and row are free.
 *
 * ds_assign_edges_device: one chunk's slots, d_row / d_probability / d_ratio / d_stage [n_queries][n] as the rank stage
 * leaves them, titles [q_first, q_first + n_queries) of the call's n_total.  Writes the key AND the row of every slot of
 * the chunk into the call-wide d_edge_key / d_edge_row [n_total][n] at q_first * n (the rows are copied as they are, so
 * the chunk's buffers may be reused at once and the solver reads two arrays it owns).  Asynchronous on `stream`.
 * DS_E_ARG, with nothing launched: a null pointer, n < 1, a negative count, q_first + n_queries > n_total,
 * n_total >= 2^31, n_truth outside [0, 2^31), a threshold that is not finite.  n_queries == 0 launches nothing.
 *
 * ds_assign_solve_device: zeroes d_held (uint64[n_truth], the key each row holds), d_next (int32[n_queries], the slot a
 * title stands at) and d_counts, runs rounds to the fixed point, then writes per title
 *   d_match_row   the row it holds, -1: none        d_match_slot  the slot of that edge, -1
 *   d_first_row   the row of its first edge, -1 when it has no edge
 * and d_counts, int64[6]: [0] edges, [1] matched titles, [2] displaced titles (first_row >= 0 and match_row != first_row),
 * [3] the displaced titles left unmatched, [4] proposals (the atomics that raised a held entry), [5] rounds in which a
 * title was active.  [0..4) and the per-title outputs are a pure function of the edges; [4] and [5] depend on the schedule
 * and are diagnostics.  A slot whose key is not 0 but whose row lies outside [0, n_truth) is no edge here either.
 * A round is one launch, one lane per title: a title whose held[row] == key at its slot is idle, so is an exhausted one;
 * any other walks forward from its slot, skips non-edges and rows that hold more than its key, offers its key with a 64-bit
 * atomicMax elsewhere and stops where the value returned is below its key.  Rounds repeat until one in which no title was
 * active; the activity counters come back every "rounds_per_sync" rounds.  SYNCHRONISES `stream`: more than once on the way
 * (one read-back per batch of rounds) and at the end, so the outputs are complete when the call returns.  It allocates
 * 4 * rounds_per_sync bytes for the counters and frees them before it returns.
 * DS_E_ARG, with nothing launched: a null pointer, n < 1, n_queries < 0 or >= 2^31, n_truth outside [0, 2^31).
 * n_queries == 0 launches no kernel and leaves d_counts at zero.
 *
 * ds_assign_option is for tests: "rounds_per_sync" in [1, 1024] (default 8), "max_blocks" in [0, 2^20]: the cap of every
 * grid of this stage, which strides beyond it (0 = the default, 2048).  The result depends on neither. */
int ds_assign_edges_device(const int32_t *d_row, const float *d_probability, const uint8_t *d_ratio, const int8_t *d_stage,
                           int64_t q_first, int64_t n_queries, int64_t n_total, int32_t n, int64_t n_truth,
                           float probability_threshold, uint64_t *d_edge_key, int32_t *d_edge_row, void *stream);
int ds_assign_solve_device(const int32_t *d_edge_row, const uint64_t *d_edge_key, int64_t n_queries, int32_t n,
                           int64_t n_truth, uint64_t *d_held, int32_t *d_next, int32_t *d_match_row,
                           int32_t *d_match_slot, int32_t *d_first_row, int64_t *d_counts, void *stream);
int ds_assign_option(const char *name, int64_t value);

/* ---- exact matches: Prediction._find_exact_matches (predict.py:74-113) ---------------------------------------------
 * exact_row[q] = the truth row whose encoded title (length and bytes of the ds_titles rows) equals query row q's, the
 * LAST such row when several truth rows hold the title (the reference's {title: title_id} dict is filled in truth
 * order), -1 when none does.  The truth table's hash table (int32 rows, capacity = the power of two >= 2N: at most
 * 16 bytes per truth row) is built on the first call and kept on the handle; DS_E_HIP when it does not fit the free
 * HBM.  ds_titles_option(truth, "exact_table", 0) frees it; "exact_hash_bits" (1..64, default 64) keeps only the low
 * bits of the title hash (titles are always compared byte by byte; fewer bits only make the probe sequences longer);
 * changing it rebuilds the table on the next call.  Host pointers: */
int ds_exact_matches(ds_titles *truth, ds_titles *queries, int64_t n_queries, int32_t *exact_row);
/* Query rows [q_first, q_first + n_queries) of the query table, d_exact_row[0 .. n_queries) in HBM; enqueued on
 * `stream`.  When d_best_row is not NULL, d_best_row[q] = d_exact_row[q] wherever an exact match exists (the other
 * entries are left alone): called after ds_close_matches_device, ds_remaining_pairs_device then drops the exact and the
 * fuzzy matches in one pass. */
int ds_exact_matches_device(ds_titles *truth, ds_titles *queries, int64_t q_first, int64_t n_queries,
                            int32_t *d_exact_row, int32_t *d_best_row, void *stream);

/* ---- next row f-3: native index build ----------------------------------------------------------------------------
 * Replaces the Python / lil_matrix loops of MatchMaker.__init__ (doppelspeller/match_maker.py:84-181) and
 * get_n_grams / get_n_grams_counter (doppelspeller/common.py:145-151): from the transformed titles (byte strings,
 * concatenated, offsets[n + 1]) to the arrays ds_index_create and ds_jaccard_topk take.  Host code.  Column ids
 * ascend with the n-gram's byte string and a title's float32 idf sum runs in first-occurrence order of its n-grams
 * (the reference leaves both to Python's set iteration order).  The arrays belong to the handle.  Threaded over title
 * ranges (DS_HOST_THREADS, default: the CPUs of the process, at most 32); the result does not depend on the count. */
int ds_problem_create(const uint8_t *truth_chars, const int64_t *truth_offsets, int64_t n_truth,
                      const uint8_t *query_chars, const int64_t *query_offsets, int64_t n_queries, int32_t n_gram,
                      ds_problem **out);
void ds_problem_destroy(ds_problem *problem);
/* info: n_truth, n_queries, n_columns, nnz (truth), nnz (queries), n_gram */
int ds_problem_info(const ds_problem *problem, int64_t info[8]);
/* vocabulary[V]: the n-gram of every column as big-endian bytes in a uint32; any out pointer may be NULL */
int ds_problem_arrays(const ds_problem *problem, const uint32_t **vocabulary, const float **idf32, const double **idf64,
                      const int64_t **rowptr, const int32_t **truth_idx, const float **sums32, const int64_t **q_rowptr,
                      const int32_t **q_cols, const double **q_maxint);

/* The encoders of the features' inputs for whole collections, host code, threaded:
 * ds_encode_titles  = FeatureEngineering.encode_title (doppelspeller/feature_engineering.py:298-307) per title:
 *   out_enc[t*stride ..) = the title's characters mapped through code_of[256] (NULL: bytes as they are), 0-padded to
 *   `stride` (255 in the reference, settings.py:68); out_len[t] = its number of characters (predict.py:195-197);
 * ds_truth_word_counts = FeatureEngineering.get_truth_words_counts (:309-319) per title over the counter of
 *   common.py:140-142: out_counts[t*DS_WORDS + j] = the number of truth titles holding the j-th word of title t (a word
 *   repeated inside one title counts once), 0-padded.  separator[256] != 0 marks the bytes str.split() splits on. */
int ds_encode_titles(const uint8_t *chars, const int64_t *offsets, int64_t n, const uint8_t *code_of, int64_t stride,
                     uint8_t *out_enc, uint8_t *out_len);
int ds_truth_word_counts(const uint8_t *chars, const int64_t *offsets, int64_t n, const uint8_t *separator,
                         uint32_t *out_counts);

/* transform_title (doppelspeller/common.py:20-47) for n titles whose Unicode step (NFD + ASCII encoding, Python's
 * unicodedata) is already done: lower case, '-' -> ' ', keep [a-zA-Z0-9\s], ' +' -> ' ', strip, cut to max_characters
 * (settings.py:68 = 255), strip, '0'-pad titles shorter than n_gram.  out_chars needs offsets[n] + n * n_gram bytes. */
int ds_transform_titles(const uint8_t *chars, const int64_t *offsets, int64_t n, int32_t max_characters, int32_t n_gram,
                        uint8_t *out_chars, int64_t *out_offsets);

/* ---- next row f-4: tree-ensemble scoring of the feature matrix -----------------------------------------------------
 * Replaces xgb.DMatrix(features) + model.predict(features_d, ntree_limit=...) (doppelspeller/predict.py:229-234) for a
 * `binary:logistic` booster, on the float32[n, n_features] matrix that ds_construct_features_* left in HBM.  Nodes of
 * all trees are concatenated; tree t owns nodes [tree_offsets[t], tree_offsets[t + 1]); child ids are tree-relative
 * (xgboost's nodeid); feature[i] < 0 marks a leaf whose value is threshold[i]; a NaN feature follows `missing`,
 * value < threshold follows `yes`, else `no`.  base_margin = logit(base_score).  Pass only the first
 * best_ntree_limit trees to reproduce `ntree_limit`.  Either output pointer may be NULL.
 * xgboost is outside the reference tree: the published rule is restated, parity unpinned. */
int ds_forest_create(const int32_t *feature, const float *threshold, const int32_t *yes, const int32_t *no,
                     const int32_t *missing, const int64_t *tree_offsets, int32_t n_trees, int32_t n_features,
                     float base_margin, int device, ds_forest **out);
void ds_forest_destroy(ds_forest *forest);
int ds_forest_predict(ds_forest *forest, const float *rows, int64_t n, float *margins, float *probabilities);
/* The same for a matrix and outputs that lie in HBM.  Asynchronous on `stream`. */
int ds_forest_predict_device(ds_forest *forest, const float *d_rows, int64_t n, float *d_margins,
                             float *d_probabilities, void *stream);

/* ---- contributions: why the model gave a row its margin ("Contributions") -------------------------
 * Node cover = the weight of the background rows that reach a node, float64[n_nodes] in the forest's node order.  A
 * forest holds none (as created), a count made on the device, or values installed by the caller.
 *
 * ds_forest_cover_device: walks n dense float32[n, n_features] rows in HBM through every tree by the rule of
 * ds_forest_predict_device and adds 1 to a 64-bit integer counter of every node a row visits: exact, whatever the
 * schedule.  Successive calls accumulate; the first call after ds_forest_create, ds_forest_cover_set or
 * ds_forest_cover_clear starts from zero (and drops installed values).  Enqueued on `stream`.  n == 0 launches nothing.
 * ds_forest_cover_set: installs `cover` (host, n_nodes values; each finite and > 0, else DS_E_ARG) in place of any count.
 * ds_forest_cover_read: the installed values, or the counters as float64 (synchronises the device); DS_E_ARG with the
 * text "no cover" when the forest has none.  ds_forest_cover_clear: back to none.
 * Cover and contributions need every tree to be a proper binary tree: yes != no, missing one of the two, one parent per
 * node (DS_E_ARG otherwise; ds_forest_create itself accepts more).
 * ds_forest_option(forest, "max_blocks", v), v in [0, 2^20], is for tests: the cap of the grids of the cover and the
 * contributions kernels, which stride beyond it (0 = the defaults); no result depends on it.
 *
 * ds_forest_contributions_device: d_out = float64[n, n_features + 1] in HBM.  Column f of a row is the contribution of
 * feature f to the row's margin, summed over the trees in tree order; the last column is the bias: base_margin plus,
 * per tree, the cover-weighted mean of its leaves (mean(node) = sum over the two children of cover[child] / cover[node]
 * * mean(child)).  A row's columns sum to its margin up to rounding.
 *   approximate = 0  path-dependent TreeSHAP (Lundberg, Erion and Lee 2018, Algorithm 2; xgboost's pred_contribs): the
 *                    one fraction of a split follows the prediction rule (NaN -> missing, value < threshold -> yes,
 *                    else no), the zero fraction of a child is cover[child] / cover[parent].
 *   approximate = 1  Saabas (xgboost's approx_contribs): along the row's own path every split adds mean(child) -
 *                    mean(node) to its feature.
 * float64 throughout, no floating-point atomics: the same bits run after run and for any max_blocks.  A feature no tree
 * splits on gets exactly 0.0; a single-leaf tree adds its leaf to the bias only.  DS_E_ARG: no cover ("no cover"), a
 * node on a path whose cover is not positive (a count no row reached), a tree more than 16 splits deep (the message
 * names the tree; the limit applies here, not at ds_forest_create).  n == 0 is DS_OK.  The path tables are derived
 * from the cover by the first call after it changed (host work and uploads; the counters are read back behind a
 * synchronisation); after that a call only enqueues one kernel on `stream`.
 * ds_forest_contributions: the same for host arrays. */
int ds_forest_cover_device(ds_forest *forest, const float *d_rows, int64_t n, void *stream);
int ds_forest_cover_set(ds_forest *forest, const double *cover);
int ds_forest_cover_read(ds_forest *forest, double *cover);
int ds_forest_cover_clear(ds_forest *forest);
int ds_forest_option(ds_forest *forest, const char *name, int64_t value);
int ds_forest_contributions_device(ds_forest *forest, const float *d_rows, int64_t n, double *d_out, int approximate,
                                   void *stream);
int ds_forest_contributions(ds_forest *forest, const float *rows, int64_t n, double *out, int approximate);

/* ---- model inspection: permutation importance and partial dependence ("Model inspection") --------
 * A JOB changes one value of every row i of a float32[n, n_features] matrix before the forest is walked:
 *   DS_INSPECT_BASELINE  nothing (feature, value and repeat are ignored);
 *   DS_INSPECT_PERMUTE   row[feature] = rows[perm(i)][feature];
 *   DS_INSPECT_OVERRIDE  row[feature] = value, any float32 (a NaN takes the `missing` branches).
 * The margin of the changed row is base_margin + the float32 leaf sum of ds_forest_predict_device, unchanged.  Per job
 * DS_INSPECT_COUNTERS unsigned 64-bit integers are summed over the rows: tp, tn, fp, fn with
 * p = 1.0f / (1.0f + expf(-margin)), predicted positive iff (double)p > threshold, actual positive iff target[i] != 0
 * (a null target: every label 0), and margin_sum = the sum of llrint(clamp((double)margin, -2^11, 2^11) * 2^20) in
 * two's complement.  A NaN margin adds 0 to margin_sum and is not positive.  Integer sums: the same bits for any grid,
 * any split of the jobs over the workgroups and any order of the jobs.
 * perm is a function of (seed, feature, repeat, n, i) alone.  n == 1: perm(0) = 0.  Otherwise
 * b = max(1, ceil(bit_length(n - 1) / 2)), mask = 2^b - 1, k_j = the first kept output of the stream ("Randomness" below)
 * of (seed, purpose DS_INSPECT_PURPOSE_PERMUTE, index (repeat << 40) | (feature << 32) | j), j = 0..3, and from x = i:
 *   { L = x >> b; R = x & mask; for j in 0..3: (L, R) = (R, L ^ (mix64(k_j ^ R) & mask)); x = (L << b) | R } until x < n,
 * mix64 the splitmix64 finaliser: a 4-round Feistel network over [0, 2^(2b)), 2^(2b) < 4n, walked back into [0, n).
 * ds_forest_inspect_device: matrix, target (nullable), job table and d_out ([n_jobs][DS_INSPECT_COUNTERS], zeroed by the
 * call) lie in HBM.  The job table is read back and checked first, which synchronises `stream`; the rest is enqueued on
 * it.  ds_forest_inspect: the same for host arrays.  DS_E_ARG before any tree is walked: a null pointer, n_jobs < 0,
 * n outside [0, 2^31], threshold outside (0, 1), an unknown kind, and for a job that is no baseline a feature outside
 * [0, n_features) or (PERMUTE) a repeat of 2^16 or more.  n == 0 or n_jobs == 0 is DS_OK, the counters zeroed.
 * The grid is row blocks x job groups: "max_blocks" of the forest's options caps the first, "inspect_jobs_per_block"
 * (for tests; 0 = the launcher's choice) sets the jobs a workgroup runs per staged row block; no result depends on either. */
#define DS_INSPECT_BASELINE 0
#define DS_INSPECT_PERMUTE 1
#define DS_INSPECT_OVERRIDE 2
#define DS_INSPECT_COUNTERS 5
#define DS_INSPECT_PURPOSE_PERMUTE 6
typedef struct ds_inspect_job {
    int32_t kind;
    int32_t feature;
    float value;
    uint32_t repeat;
} ds_inspect_job;
int ds_forest_inspect_device(ds_forest *forest, const float *d_rows, int64_t n, const float *d_target,
                             const ds_inspect_job *d_jobs, int32_t n_jobs, uint64_t seed, double threshold,
                             unsigned long long *d_out, void *stream);
int ds_forest_inspect(ds_forest *forest, const float *rows, int64_t n, const float *target, const ds_inspect_job *jobs,
                      int32_t n_jobs, uint64_t seed, double threshold, unsigned long long *out);
/* Per query of k consecutive candidates the one with the highest probability, the first on a tie (predict.py:239-242; a
 * NaN never replaces an earlier candidate, and a NaN in slot 0 is never replaced itself: it stays the best, with count
 * 1, whatever follows): d_best_pair[q] = q * k + its slot (an index for ds_gather_rows_device),
 * d_best_row[q] = d_rows[that pair], d_best_probability[q], d_best_count[q] = the candidates that hold that
 * probability.  Asynchronous on `stream`; n_queries == 0 launches nothing. */
int ds_best_pairs_device(const int32_t *d_rows, const float *d_probabilities, int64_t n_queries, int32_t k,
                         int64_t *d_best_pair, int32_t *d_best_row, float *d_best_probability, int32_t *d_best_count,
                         void *stream);

/* ---- training of the match model: xgb.train(obj=weighted_log_loss, feval=custom_error) (doppelspeller/train.py) ----
 * Histogram gradient boosting, depth-wise, one tree per ds_trainer_step (DESIGN.md "Training").  features is the
 * float32[n][n_features] training matrix (NaN = missing), copied and binned on the device at create time: cuts[
 * cut_offsets[f] .. cut_offsets[f + 1]) are feature f's strictly ascending cut values (at most 254 each), bin(x) = the
 * number of cuts <= x.  Gradients of the weighted log loss with beta; eta, min_child_weight and reg_lambda as in
 * xgboost; base_score 0.5 (base margin 0).  max_depth 1..8, n_features 1..96.  Labels are 0 or 1. */
int ds_trainer_create(const float *features, int64_t n, int32_t n_features, const float *cuts,
                      const int32_t *cut_offsets, int32_t max_depth, double eta, double min_child_weight,
                      double reg_lambda, double beta, int device, ds_trainer **out);
void ds_trainer_destroy(ds_trainer *trainer);
int ds_trainer_set_labels(ds_trainer *trainer, const float *labels);
/* Optional evaluation set (before the first round): binned with the training cuts, routed through every new tree;
 * each step then reports train.py's custom error on it. */
int ds_trainer_set_eval(ds_trainer *trainer, const float *features, const float *labels, int64_t n);
/* Grows one tree and adds it to the training (and evaluation) margins.  The tree comes back in heap order
 * (children of node i: 2i + 1, 2i + 2; 2^(max_depth + 1) - 1 slots): node_info[4i .. 4i + 4) = (state: 0 absent,
 * 2 split, 3 leaf; feature; bin b: bins < b go left; missing goes left), node_leaf[i] = the leaf value.
 * eval_error (nullable) = the custom error after this round, -1 without an evaluation set.  One host sync. */
int ds_trainer_step(ds_trainer *trainer, int32_t *node_info, float *node_leaf, int64_t *eval_error);
/* Read-back for tests, every pointer nullable: training margins float[n] (base margin + leaves so far), the
 * probabilities float[n] and quantized (gradient, hessian) int64[n][2] of the last step, the bins uint8[n_features][n]
 * (feature-major, 255 = missing) and the evaluation margins float[n_eval]. */
int ds_trainer_read(ds_trainer *trainer, float *margins, float *probabilities, int64_t *gradients, uint8_t *bins,
                    float *eval_margins);
/* Row and column subsampling ("Subsampling"), valid only before the first ds_trainer_step.  The
 * three fractions lie in (0, 1]; all 1 (the state after create) runs the unsampled kernels.  The draws come from the
 * streams of "Randomness" below with seed = sample_seed, the first kept output x of a stream, and t = the trees grown so
 * far: purpose 3 (DS_SAMPLE_PURPOSE_ROW), index (t << 32) | r: training row r trains in tree t iff
 * (x >> 11) * 2^-53 < subsample, r counted among the rows that train (in a batch: the rows outside the model's held-out
 * fold, in row order); purpose 4 (DS_SAMPLE_PURPOSE_TREE), index (t << 32) | f: the tree uses the
 * max(1, floor(colsample_bytree * n_features)) features with the smallest x, ties to the lower f; purpose 5
 * (DS_SAMPLE_PURPOSE_LEVEL), index (t << 32) | (d << 8) | f: level d uses the max(1, floor(colsample_bylevel * k_tree))
 * features of the tree's set with the smallest x.  A fraction of 1 draws nothing.  An undrawn row is a held-out row for
 * that tree: gradient and hessian 0 (also in ds_trainer_read), in no histogram, routed through the tree.  A feature
 * outside a level's set offers no split there.  DS_E_ARG for a null trainer, a fraction outside (0, 1], a call after a
 * step, or subsample < 1 with reg_lambda = 0; a null trainer is refused before any device is touched. */
#define DS_SAMPLE_PURPOSE_ROW 3
#define DS_SAMPLE_PURPOSE_TREE 4
#define DS_SAMPLE_PURPOSE_LEVEL 5
int ds_trainer_set_sampling(ds_trainer *trainer, double subsample, double colsample_bytree, double colsample_bylevel,
                            uint64_t sample_seed);
/* Per-row sample weights in the objective ("Sample weights"): weights is a host float[n], like the
 * labels.  With p the float32 probability of row r, y its label and w = beta + y - beta y, every later step quantizes
 *   g = (p w - y) * s_r,  h = (p (1 - p) w) * s_r,  (rint(g * 2^30), rint(h * 2^30))
 * with the parenthesised factors computed as without weights and s_r widened to double before the one multiplication.
 * Everything after the gradients works on these integers as before: min_child_weight bounds a sum of weighted hessians.
 * A row of weight 0 carries (0, 0), like a held-out or undrawn row.  The weights do not touch the cuts, the subsample
 * draw (indexed by row number), the evaluation error, the metrics (counts over rows) or a forest's cover.
 * Legal once, after ds_trainer_set_labels and before the first step.  DS_E_ARG with a message, nothing launched and the
 * trainer still usable unweighted, for: a null pointer; a weight that is not finite or is negative; a total weight of 0
 * (the root would divide by zero with reg_lambda = 0); max(beta, 1) * sum(weights) > 2^32 with the sum in double (the
 * bounds |g| <= max(beta, 1) s_r, h <= max(beta, 1) s_r / 4 then keep every int64 histogram sum below 2^62 + n); a
 * second call; a call after a step.  The array costs 4 n bytes of HBM.  ds_trainer_read's gradients are the weighted
 * integers. */
int ds_trainer_set_weights(ds_trainer *trainer, const float *weights);
/* Monotone constraints per feature ("Monotone constraints"; xgboost's monotone_constraints):
 * constraints is a host int8[n_features] of -1, 0 and +1.  Every node of a tree carries bounds [lo, hi] on its weight,
 * the root's infinite, all in double.  With w = -G / (H + lambda) and w* = min(max(w, lo), hi), a node's gain term is
 * G G / (H + lambda) while lo <= w <= hi and -(2 G w* + (H + lambda) w* w*) otherwise; a candidate's gain is the terms
 * of its two children minus the node's, all under the node's bounds, and after the min_child_weight test a candidate on
 * feature f is rejected when constraints[f] > 0 and wL* > wR*, or constraints[f] < 0 and wL* < wR*.  The children of a
 * split on a constrained feature share mid = (wL* + wR*) / 2 as the bound between them, those of any other split
 * inherit [lo, hi], and every leaf is float(w* * eta) under its own bounds.  So every tree is monotone in each
 * constrained feature, and while no bound is finite every number is the unconstrained rule's, bit for bit.  Cuts,
 * gradients, histograms, draws, errors, metrics and cover are untouched.
 * Legal once, after ds_trainer_set_labels and before the first step.  DS_E_ARG with a message, nothing launched and the
 * trainer still usable unconstrained, for: a null pointer; a value outside {-1, 0, 1}; a second call; a call after a
 * step.  An all-zero array is accepted, allocates nothing and leaves the trainer unconstrained; any other costs
 * n_features + 16 * (2^(max_depth + 1) - 1) bytes of HBM. */
int ds_trainer_set_monotone(ds_trainer *trainer, const int8_t *constraints);

/* ---- the train-model step without a host copy of the feature matrix ("One call") ----------------
 * ds_feature_cuts_device: compute_cuts of a contiguous float32[n][n_features] matrix in HBM, bit-identical to the host
 * rule for any input: per column the non-NaN values with -0.0 read as +0.0; at most max_bin - 1 distinct ones: the sorted
 * distinct values without the smallest; else v[(j * m) / (max_bin - 1)], j = 1 .. max_bin - 2, of the m sorted values v,
 * without repeats and without values equal to v[0].  cuts (host, room for n_features * 254) receives cut_offsets[n_features]
 * values and cut_offsets (host, n_features + 1) their starts; nothing beyond those is written.  n in [1, 2^31),
 * n_features in [1, 96], max_bin in [2, 256].  Enqueued on `stream`, which is synchronised before returning; the matrix
 * must be complete on that stream.  ds_cuts_option("column_group", g) is for tests: g > 0 sorts g columns at a time
 * instead of what a quarter of the free HBM holds (0: back to that); the result does not depend on it. */
int ds_feature_cuts_device(const float *d_features, int64_t n, int32_t n_features, int32_t max_bin, float *cuts,
                           int32_t *cut_offsets, int device, void *stream);
int ds_cuts_option(const char *name, int64_t value);
/* ds_trainer_create / ds_trainer_set_eval for a contiguous float32[n][n_features] matrix that already lies in HBM on
 * `device` (the trainer's device for the evaluation set): no staged copy, the same binning kernel and so the same bins.
 * The caller must have finished writing the matrix (synchronise the stream that wrote it) before the call.  The entry
 * synchronises before it returns and keeps no pointer to the matrix, which may be freed afterwards.  Labels are host
 * pointers as in the host entries. */
int ds_trainer_create_device(const float *d_features, int64_t n, int32_t n_features, const float *cuts,
                             const int32_t *cut_offsets, int32_t max_depth, double eta, double min_child_weight,
                             double reg_lambda, double beta, int device, ds_trainer **out);
int ds_trainer_set_eval_device(ds_trainer *trainer, const float *d_features, const float *labels, int64_t n);
/* d_dst[i][..] = d_src[d_rows[i]][..] for i < n_rows: rows of n_features (1..96) float32, all pointers in the HBM of the
 * current device, d_rows in any order, repeats allowed.  A row index outside [0, n_src) is found by a check on the device
 * before the gather is launched: DS_E_ARG, no source row read and d_dst untouched.  n_rows = 0 does nothing.  Enqueued on
 * `stream`, which is synchronised before returning. */
int ds_gather_rows_device(const float *d_src, int32_t n_features, const int64_t *d_rows, int64_t n_rows, int64_t n_src,
                          float *d_dst, void *stream);

/* ---- batched training: cross-validation and parameter search ("Cross-validation and tuning") -------
 * One batch holds one binned training matrix and n_models (1..256) boosters, each grown by ds_trainer_step's rule with its
 * own parameters and its own held-out fold.  features, cuts, cut_offsets as for ds_trainer_create(_device): the cuts are
 * those of the WHOLE matrix.  labels float[n] (0 or 1) and fold uint8[n] (every value below n_folds, 1..255) are host
 * arrays.  params[5m .. 5m + 5) = max_depth (integral, 1..8), eta, min_child_weight, reg_lambda, beta of model m, in
 * ds_trainer_create's ranges; held_out[m] in [-1, n_folds).  Row r trains in model m iff fold[r] != held_out[m] (-1: every
 * row trains): a held-out row has gradient and hessian 0, adds nothing to any histogram, and is routed through every new
 * tree, which adds its leaf to the row's float32 leaf sum like any row's.  Model m's trees are so those of
 * ds_trainer_step on its training rows alone with the same cuts.  Any argument out of range or null: DS_E_ARG, nothing
 * launched, *out = NULL.  A batch that does not fit the free HBM (ds_trainer_batch_bytes, + 4 * n * n_features for the
 * staged copy of a host matrix) is refused with DS_E_HIP and a message that names both numbers.  The _device form reads a
 * matrix that lies complete in HBM and keeps no pointer to it. */
int ds_trainer_batch_create(const float *features, int64_t n, int32_t n_features, const float *cuts,
                            const int32_t *cut_offsets, const float *labels, const uint8_t *fold, int32_t n_folds,
                            int32_t n_models, const double *params, const int32_t *held_out, int device,
                            ds_trainer_batch **out);
int ds_trainer_batch_create_device(const float *d_features, int64_t n, int32_t n_features, const float *cuts,
                                   const int32_t *cut_offsets, const float *labels, const uint8_t *fold, int32_t n_folds,
                                   int32_t n_models, const double *params, const int32_t *held_out, int device,
                                   ds_trainer_batch **out);
void ds_trainer_batch_destroy(ds_trainer_batch *batch);
/* One round of every model m with active[m] != 0 (host array of n_models bytes; NULL: all of them): each kernel of the
 * round is launched once for all active models, levels run to the largest max_depth among them, one host sync.  The
 * trees come back as ds_trainer_step's heaps with slots = 2^(D + 1) - 1, D = the LARGEST max_depth of the batch, whatever
 * a model's own: node_info int32[n_models][slots][4], node_leaf float[n_models][slots].  errors int64[n_models]: train.py's
 * custom error (missed positives + 5 * false positives at p > 0.9) of model m's held-out rows at their margins after the
 * round, -1 for held_out[m] = -1.  An inactive model is not touched: its state stays as it was and its entries of the
 * three outputs are not written; the active ones behave as if it did not exist.  No active model: nothing is done. */
int ds_trainer_batch_step(ds_trainer_batch *batch, const uint8_t *active, int32_t *node_info, float *node_leaf,
                          int64_t *errors);
/* Read-back for tests, every pointer nullable: one model's margins float[n] of ALL rows, the probabilities float[n] and
 * quantized (gradient, hessian) int64[n][2] of its last step (zeros before its first), and the shared bins
 * uint8[n_features][n]. */
int ds_trainer_batch_read(ds_trainer_batch *batch, int32_t model, float *margins, float *probabilities,
                          int64_t *gradients, uint8_t *bins);
/* The bytes of HBM that ds_trainer_batch_create_device needs for n_models models whose largest max_depth is max_depth:
 * n * n_features + 5 n shared, and per model 28 n + (2^max_depth - 1) * n_features * 4096 + a few KiB.  -1 for
 * arguments outside the limits above.  Sample weights (ds_trainer_batch_set_weights) add 4 n bytes, shared by the
 * models, and monotone constraints (ds_trainer_batch_set_monotone) 16 * slots * n_models + n_features bytes; this
 * formula counts neither. */
int64_t ds_trainer_batch_bytes(int64_t n, int32_t n_features, int32_t n_models, int32_t max_depth);
/* ds_trainer_set_sampling for every model of a batch, valid only before the first ds_trainer_batch_step:
 * fractions[3m .. 3m + 3) = subsample, colsample_bytree, colsample_bylevel of model m, sample_seeds[m] its seed.  Every
 * model counts its own trees: a step in which it is inactive does not advance its streams.  A model's draws are those of
 * ds_trainer on its training rows alone, so are its trees.  Models with and without sampling share the launches of a
 * step, which keeps its one host sync; with every fraction 1 the unsampled kernels run.  Adds under 1 KiB per model, and
 * n / 16 bytes per fold that a model with subsample < 1 holds out.  DS_E_ARG as for ds_trainer_set_sampling, with the
 * model named. */
int ds_trainer_batch_set_sampling(ds_trainer_batch *batch, const double *fractions, const uint64_t *sample_seeds);
/* ds_trainer_set_weights for a batch: ONE host float[n] over all rows, shared by the models like the labels, legal once
 * and before the first ds_trainer_batch_step.  A held-out row stays (0, 0) whatever its weight, and a model's trees are
 * those of ds_trainer with the weights of its training rows.  The guard takes the largest beta among the models, and
 * the rows outside the held-out fold of EVERY model must have a total weight above 0: DS_E_ARG names the first model
 * that has none.  Adds 4 n bytes of HBM to ds_trainer_batch_bytes, whose formula does not count them. */
int ds_trainer_batch_set_weights(ds_trainer_batch *batch, const float *weights);
/* ds_trainer_set_monotone for a batch: ONE host int8[n_features] for all models, legal once and before the first
 * ds_trainer_batch_step; a model's trees are those of ds_trainer with the same constraints on its training rows.  With
 * slots = 2^(D + 1) - 1, D the largest max_depth of the batch, a vector that is not all zeros adds
 * 16 * slots * n_models + n_features bytes of HBM, which ds_trainer_batch_bytes does not count. */
int ds_trainer_batch_set_monotone(ds_trainer_batch *batch, const int8_t *constraints);
/* For tests: ds_trainer_batch_option("max_blocks", b) caps every grid of a training round that runs over rows at b
 * workgroups, which stride beyond it (0: back to the default).  It also caps the round of ds_trainer_step, which launches
 * the same kernels.  The results do not depend on it. */
int ds_trainer_batch_option(const char *name, int64_t value);

/* ---- metrics of a booster's margins, computed on the device ("Metrics") ---------------------------
 * AUC is taken over float32 MARGINS by integer key: NaN -> 0xFFFFFFFF, else with -0.0 read as +0.0 the bits with all
 * bits flipped when the sign is set and only the sign bit flipped otherwise (the order of the cuts).  With P the rows of
 * label 1 and N those of label 0 whose score is not a NaN, concordant = #{(p, n): key_p > key_n}, ties = #{(p, n):
 * key_p == key_n} and auc = (2 concordant + ties) / (2 |P| |N|), undefined when a class is empty.  A row with a NaN
 * score belongs to neither class.  The weighted log loss of a row is y * softplus(-m) + beta * (1 - y) * softplus(m) in
 * float64 from its float32 margin m, softplus(x) = max(x, 0) + log1p(exp(-|x|)); it saturates at 2^11 (a NaN term too)
 * and is quantised as rint(term * 2^20); the value reported is sum / 2^20 / rows.  With y in {0, 1} only the product that
 * does not vanish is computed, so an infinite margin on the row's own side costs 0 (not 0 * inf) and one on the other
 * side the cap.  Every number is an integer sum: the
 * same for any schedule and from run to run.
 *
 * ds_auc_device: out = (concordant, ties, positives, negatives, nan_rows) of d_scores[n] with d_labels[n] (0 = negative,
 * anything else positive), both in HBM, n in [1, 2^31).  The negatives' keys are sorted by the radix sort of the cuts;
 * scratch: 4 n bytes of row lists and 8 bytes + 1/8 byte of tables per negative, checked against the free HBM.
 * Enqueued on `stream` and synchronised before returning.  ds_auc does the same for host arrays on `device`.
 * ds_weighted_logloss_device: out = (fixed-point sum, rows) of d_margins[n] with d_labels[n]; enqueued on `stream` and
 * synchronised before returning, like ds_auc_device.
 * For tests: ds_metrics_option("max_blocks", b) caps every grid of the metric kernels that runs over rows at b
 * workgroups, which stride beyond it (0: back to the default; the grids of the sort are one workgroup per tile of keys).
 * The results do not depend on it. */
#define DS_METRIC_AUC 1u
#define DS_METRIC_LOGLOSS 2u
int ds_auc_device(const float *d_scores, const float *d_labels, int64_t n, int64_t out[5], void *stream);
int ds_auc(const float *scores, const float *labels, int64_t n, int64_t out[5], int device);
int ds_weighted_logloss_device(const float *d_margins, const float *d_labels, int64_t n, double beta, int64_t out[2],
                               void *stream);
int ds_metrics_option(const char *name, int64_t value);
/* Per-round metrics of a trainer: flags = DS_METRIC_AUC | DS_METRIC_LOGLOSS (0 switches them off).  Valid only before
 * the first step and after the labels (and the evaluation set, if any) are set; DS_E_ARG otherwise and for unknown bits.
 * The scratch -- the lists of negative and positive rows (4 bytes per row), the sort buffers for the larger set's
 * negatives, the counters -- is allocated here and only here.  Every later ds_trainer_step then enqueues the metric
 * kernels after the round's own, over the training margins (ALL training rows, whatever the subsampling) and over the
 * evaluation margins, and their counters come back with the round's one host sync.  Without flags a step launches,
 * copies and allocates exactly what it did before.
 * ds_trainer_metrics: the last step's values, from the host: out[0] for the training set, out[1] for the evaluation
 * set, each (concordant, ties, positives, negatives, logloss_sum, rows); -1 for a metric not requested, a set that does
 * not exist, or before the first step. */
int ds_trainer_set_metrics(ds_trainer *trainer, uint32_t flags);
int ds_trainer_metrics(ds_trainer *trainer, int64_t out[2][6]);
/* The same for a batch, over the rows of every model's HELD-OUT fold: valid only before the first step of the batch.
 * The rows of a fold are listed once (negatives, then positives); every step gathers the keys of the active models'
 * held-out negatives from their margins and sorts them with the models in the grid's second dimension, so that the sort
 * buffers hold about n / n_folds keys per model.  The step keeps its one host sync.
 * ds_trainer_batch_metrics: out[m] as above for every model after ITS last active step; -1 for held_out = -1 and before
 * the model's first step.
 * ds_trainer_batch_metrics_bytes: the HBM this adds for folds of equal size (the largest fold sets the buffers: 4 n for
 * the lists, per model 8 bytes per key and 1 KiB per 8192 keys); -1 for arguments out of range. */
int ds_trainer_batch_set_metrics(ds_trainer_batch *batch, uint32_t flags);
int ds_trainer_batch_metrics(ds_trainer_batch *batch, int64_t *out);
int64_t ds_trainer_batch_metrics_bytes(int64_t n, int32_t n_models, int32_t n_folds);

/* ---- continuing from a model: xgb.train(..., xgb_model=booster) ("Continuing from a model") -------
 * ds_trainer_seed starts a trainer's margins from `forest` instead of from zero.  A trainer keeps only bins, and the
 * forest's thresholds need not be cuts of this matrix, so the call takes the RAW float32[n][n_features] training matrix
 * again (and the evaluation matrix, float32[n_eval][n_features], exactly when the trainer has an evaluation set): one
 * kernel walks every tree of the forest per row by the rule of ds_forest_predict_device (NaN -> missing, else value <
 * threshold) and writes the float32 sum of the leaves, from zero in tree order, as the row's leaf sum.  After the call
 * the training margins are those of ds_forest_predict(forest, ...), bit for bit, every later ds_trainer_step grows the
 * tree a trainer would grow that had grown the forest's trees itself, and the sampling tree number t of
 * ds_trainer_set_sampling starts at the forest's tree count.  So k rounds, then a trainer seeded with those k trees and
 * stepped m times, give exactly the trees of k + m rounds.
 * *initial_error (nullable) = the custom error of the evaluation set at the seeded margins, -1 without an evaluation
 * set; it comes back with the call's one host sync.
 * Legal once per trainer, after ds_trainer_set_labels and ds_trainer_set_eval and before the first ds_trainer_step (the
 * evaluation set can no longer be given afterwards).  The forest must live on the trainer's device, have its n_features
 * and have base margin 0 (base_score 0.5), the trainer's own; its depth and tree count are free, zero trees are legal
 * (the margins stay 0).  DS_E_ARG with a message, nothing launched and no state changed: a null pointer, a second call,
 * a call after a step or before the labels, eval_features that does not go with the evaluation set, another device,
 * feature count or base margin.  A host matrix is uploaded in chunks of at most 64 MiB; no second full copy is held.
 * ds_trainer_seed_device: the same for matrices that lie complete in HBM; the kernels are enqueued on `stream`, which is
 * synchronised before returning.  The matrices are not kept.
 * ds_trainer_batch_seed(_device): the same for a batch.  The forest is evaluated once per row and the sum written to
 * the leaf sums of all n_models models, held-out rows included; every model's tree count starts at the forest's.
 * initial_errors int64[n_models] (nullable): the custom error of model m's held-out rows at the seeded margins, -1 for
 * held_out[m] = -1.  Legal once, before the first ds_trainer_batch_step.
 * A trainer or batch that is never seeded launches, allocates and copies exactly what it did before. */
int ds_trainer_seed(ds_trainer *trainer, const ds_forest *forest, const float *features, const float *eval_features,
                    int64_t *initial_error);
int ds_trainer_seed_device(ds_trainer *trainer, const ds_forest *forest, const float *d_features,
                           const float *d_eval_features, int64_t *initial_error, void *stream);
int ds_trainer_batch_seed(ds_trainer_batch *batch, const ds_forest *forest, const float *features,
                          int64_t *initial_errors);
int ds_trainer_batch_seed_device(ds_trainer_batch *batch, const ds_forest *forest, const float *d_features,
                                 int64_t *initial_errors, void *stream);

/* ---- refreshing a model: xgboost's process_type="update", updater="refresh" ("Refreshing a model")
 * ds_forest_refresh keeps every split of `forest` and re-estimates its leaves on n rows it may never have seen: the RAW
 * float32[n][n_features] matrix, labels in {0, 1} and optional float32 weights (null: every row weighs 1).  The forest is
 * not modified; the new values come back in leaf_out.  With b the forest's base margin, per row leafsum = 0 (float32),
 * then for every tree t in order:
 *   p = 1.0f / (1.0f + expf(-(b + leafsum))); (g, h) = the trainer's quantized gradient pair at p (ds_trainer_step's:
 *   w = beta + y - beta y, g = (p w - y) s, h = (p (1 - p) w) s in double, rint(x * 2^30) to int64);
 *   the row walks tree t by the rule of ds_forest_predict_device (NaN -> missing, else value < threshold -> yes) to a
 *   leaf l; QG_l, QH_l = the exact integer sums of g, h over the rows that reach l;
 *   with refresh_leaf = 1 a leaf with QH_l > 0 takes (float)((-(QG_l / 2^30) / (QH_l / 2^30 + reg_lambda)) * eta), the
 *   trainer's leaf value; a leaf with QH_l == 0 (no row reaches it, or only rows of weight 0) keeps its value; with
 *   refresh_leaf = 0 every leaf keeps its value;
 *   leafsum = leafsum + the (new) value of l, a float32 add.
 * So a forest grown by ds_trainer_step without sampling or constraints and refreshed on its own matrix, labels, weights,
 * eta, reg_lambda and beta comes back bit for bit.  Integer sums: the same bits for any grid and any schedule.
 * Outputs, host arrays in both forms: leaf_out float32[n_nodes], the forest's value array with the new leaves (a split
 * node holds its unchanged threshold); node_sums int64[n_nodes][2] = (QG, QH) in the forest's node order, an inner node
 * the sum of its two children (QH / 2^30 is xgboost's cover); margins (nullable) float32[n] = b + the final leafsum;
 * *empty_leaves = the leaves with QH == 0; trace (nullable, for tests) float32[n_trees][n], the p of every tree.
 * Evaluation set (eval_features null and n_eval 0 for none): raw float32[n_eval][n_features] rows and labels take the
 * same walk and margin update without sums; eval_errors (nullable) int64[n_trees + 1]: entry 0 the custom error
 * (ds_trainer_step's) of the forest as given, entry k that of the first k refreshed trees; all -1 without a set.
 * A host matrix is uploaded once, whole, because every tree reads it again: DS_E_HIP with the bytes needed and the bytes
 * free when it does not fit.  Two launches per tree on one stream, no host sync between trees, then one sync.
 * n == 0 launches nothing over training rows: leaf_out holds the forest's values and every sum is 0.
 * DS_E_ARG with a message naming the argument, before any device work: a null forest or output, a feature count above
 * 96, n or n_eval outside [0, 2^31), a label that is not 0 or 1, a weight that is negative or not finite,
 * max(beta, 1) * the total weight (without weights: * n) above 2^32 (the int64 sums could overflow), eta <= 0,
 * reg_lambda < 0, beta <= 0, refresh_leaf that is neither 0 nor 1, and a tree that is no proper binary tree (the rule of
 * ds_forest_cover_device).
 * ds_forest_refresh_device: the same for matrices that lie complete in HBM on the forest's device (another device is
 * DS_E_ARG), read where they lie; labels and weights stay host arrays.  The kernels are enqueued on `stream`, which is
 * synchronised before returning.
 * ds_forest_option(forest, "refresh_lds_nodes", v), v in [0, 2048], is for tests: a tree of at most v nodes sums in a
 * workgroup's LDS table before HBM, a larger one adds straight to HBM (0 = the default, 2048); "max_blocks" caps the row
 * grids.  No result depends on either. */
int ds_forest_refresh(const ds_forest *forest, const float *features, int64_t n, const float *labels,
                      const float *weights, const float *eval_features, const float *eval_labels, int64_t n_eval,
                      double eta, double reg_lambda, double beta, int refresh_leaf, float *leaf_out, int64_t *node_sums,
                      float *margins, int64_t *eval_errors, int64_t *empty_leaves, float *trace);
int ds_forest_refresh_device(const ds_forest *forest, const float *d_features, int64_t n, const float *labels,
                             const float *weights, const float *d_eval_features, const float *eval_labels, int64_t n_eval,
                             double eta, double reg_lambda, double beta, int refresh_leaf, float *leaf_out,
                             int64_t *node_sums, float *margins, int64_t *eval_errors, int64_t *empty_leaves, float *trace,
                             void *stream);

/* ---- is a difference real: the paired bootstrap of outcome counts ("Is a difference real") --------
 * codes: uint8[n_sets][n]; row i under prediction set m has the outcome class codes[m][i] in {0, 1, 2, 3}.  unit:
 * int32[n], the resampling unit of row i in [0, n_units), or null: then n_units must be n and every row is its own unit.
 * A unit may hold no row.  With U = n_units:
 *   T[u][m][c]        = the rows i with unit[i] == u and codes[m][i] == c;
 *   baseline[m][c]    = the sum over u of T[u][m][c];
 *   x(b, k)           = the first kept output of the stream ("Randomness" below) of (seed, purpose
 *                       DS_BOOTSTRAP_PURPOSE_DRAW, index (b << 32) | k);
 *   j(b, k)           = floor(x * U / 2^64), the high 64 bits of the 128-bit product;
 *   counts[b][m][c]   = the sum over k < U of T[j(b, k)][m][c], int64: replicate b draws U units, and all sets see the
 *                       same draws, which makes the comparison paired.
 * Integer sums: the same bits for any grid, any split of replicates or draws over workgroups and any order.
 * Limits: n_sets in [1, 64], n_boot in [1, 65536], n in [0, 2^31], n_units in [1, 2^31] when n > 0.
 * ds_bootstrap_counts_device: codes, units, d_counts ([n_boot][n_sets][4]) and d_baseline ([n_sets][4]) lie in HBM on the
 * current device.  A kernel checks every code and unit first (and builds T), and `stream` is synchronised for its verdict:
 * a code above 3 or a unit outside [0, n_units) is DS_E_ARG with both outputs untouched.  Then the outputs are zeroed
 * and the resampling runs; `stream` is synchronised before the call returns.  Scratch: 16 * n_units * n_sets bytes with
 * units, none without.  n == 0 is DS_OK with zeroed counters.  DS_E_ARG before any device work: a null pointer, a limit
 * exceeded, a null unit with n_units != n.  ds_bootstrap_counts: the same for host arrays, checked on the host.
 * ds_bootstrap_option is for tests: "max_blocks" (0 = the default) caps the grids, which stride beyond it;
 * "replicates_per_block" (0 = the launcher's choice) sets the replicates a workgroup runs over its staged table;
 * "table_in_lds" 0 reads the table from HBM, 1 (the default) stages it in LDS when it fits.  No result depends on them.
 * ds_outcome_codes_device: d_codes[i] = the outcome of margin d_margins[i] against d_target[i] by the rule of
 * ds_forest_inspect: p = 1.0f / (1.0f + expf(-margin)), predicted positive iff (double)p > threshold (a NaN margin is
 * not positive), actual positive iff target != 0; code 0 is tn, 1 fp, 2 fn, 3 tp.  Asynchronous on `stream`.  DS_E_ARG:
 * a null pointer with n > 0, n outside [0, 2^31], threshold outside (0, 1). */
#define DS_BOOTSTRAP_PURPOSE_DRAW 7
int ds_bootstrap_counts_device(const uint8_t *d_codes, int32_t n_sets, int64_t n, const int32_t *d_unit, int64_t n_units,
                               int32_t n_boot, uint64_t seed, long long *d_counts, long long *d_baseline, void *stream);
int ds_bootstrap_counts(const uint8_t *codes, int32_t n_sets, int64_t n, const int32_t *unit, int64_t n_units,
                        int32_t n_boot, uint64_t seed, long long *counts, long long *baseline);
int ds_bootstrap_option(const char *name, int64_t value);
int ds_outcome_codes_device(const float *d_margins, const float *d_target, int64_t n, double threshold, uint8_t *d_codes,
                            void *stream);

/* ---- what the probability means: isotonic calibration and reliability ("Calibration") -------------
 * scores, labels: float32[n].  A row is positive iff its label != 0.  Its place is key(score), the integer order of
 * float32 of the cuts and the metrics: -0.0 counts as +0.0, the infinities are ordinary ends, and a row whose score is a
 * NaN is counted apart and takes no part.  Rows of equal key are one POINT of weight pos + neg.  The fit is the isotonic
 * (non-decreasing) least-squares regression of the labels on the points, returned as its level sets: K blocks in
 * ascending order, block k with
 *   lo[k], hi[k]   the float32 values of its smallest and largest key,
 *   pos[k], neg[k] its positive and negative rows (int64),
 * and pos / (pos + neg) strictly increasing in k.  Means are compared by cross-multiplying the integer sums (counts are
 * below 2^31, the products fit 64 bits); no floating point enters, and the solution is unique, so the blocks are the
 * same bits for any grid, any segment width and from run to run.
 * The map of a calibration (lo, value): a score s takes value[k] of the last block with key(lo[k]) <= key(s), 0 when
 * key(s) < key(lo[0]), a NaN when s is a NaN or K == 0.  A look-up, no interpolation.
 * ds_isotonic_fit_device: the inputs and the four outputs (room for n blocks each) lie in HBM on the current device.
 * out[0] = K, out[1] = the NaN rows left out, out[2] = the distinct keys (points), out[3] = the blocks that entered the
 * last, serial pooling level.  Stages: keys split by label, both columns sorted by the radix sort of the cuts, one
 * point per distinct key, then pooling in two levels: segments of points pooled in LDS by a workgroup each, and the
 * survivors pooled to the end by one thread.  Limits: n in [0, 2^31); n == 0 or only NaN scores give K = 0.  A null
 * pointer with n > 0 or n out of range is DS_E_ARG before any device work.  Scratch: below 33 * n bytes + 1 MiB (the
 * sort's two buffers and table, the head scan, the points; 2 * n more at segment_points 2), checked against the free HBM (with 64 MiB of head room) before anything is allocated: DS_E_HIP.  `stream` is
 * synchronised before the call returns.  ds_isotonic_fit: the same for host arrays on `device` (32 * n bytes more).
 * ds_calibration_apply_device: d_out[i] = the map of d_scores[i]; d_lo, d_value float32[K], K >= 0, edges ascending.
 * The edges' keys are staged in LDS when K <= 16384 and read from HBM otherwise; one binary search per score.
 * Asynchronous on `stream`.  DS_E_ARG: a null pointer with n > 0 (d_lo, d_value may be null when K == 0), K < 0, n
 * outside [0, 2^31).
 * ds_reliability_device: d_out is int64[n_bins + 1][4], zeroed first.  A probability p in [0, 1] falls in bin
 * min(floor((double)p * n_bins), n_bins - 1) and adds 1, (label != 0), rint(p * 2^30) and rint((p - y)^2 * 2^30), the
 * last two in float64 with y = 0 or 1; a p that is a NaN or outside [0, 1] adds 1 and (label != 0) to row n_bins.
 * Integer sums.  n_bins in [1, 256], n in [0, 2^31); asynchronous on `stream`.
 * ds_calibrate_option is for tests: "max_blocks" (0 = the default) caps the grids, which stride beyond it;
 * "segment_points" (0 = the launcher's choice, else 2 .. 2048) sets the points of a first-level segment.  No result
 * depends on them. */
int ds_isotonic_fit_device(const float *d_scores, const float *d_labels, int64_t n, float *d_lo, float *d_hi,
                           long long *d_pos, long long *d_neg, int64_t *out, void *stream);
int ds_isotonic_fit(const float *scores, const float *labels, int64_t n, float *lo, float *hi, long long *pos,
                    long long *neg, int64_t *out, int device);
int ds_calibration_apply_device(const float *d_lo, const float *d_value, int32_t K, const float *d_scores, int64_t n,
                                float *d_out, void *stream);
int ds_reliability_device(const float *d_probabilities, const float *d_labels, int64_t n, int32_t n_bins, long long *d_out,
                          void *stream);
int ds_calibrate_option(const char *name, int64_t value);

/* ---- training set of the match model: FeatureEngineering.generate_train_and_evaluation_data_sets ----------------------
 * (doppelspeller/feature_engineering.py:172-378, feature_engineering_prepare.py).  Randomness: one splitmix64 stream per
 * (seed, purpose, index), state = seed * 0x9e3779b97f4a7c15 + index * 0xd1342543de82ef95 + purpose * 0xaf251af3b0f025b5
 * (mod 2^64), the first two outputs thrown away; below(n) = the high 64 bits of x * n; randint(a, b) = a + below(b - a + 1),
 * choice(seq) = seq[below(len)], sample(pop, k) = partial Fisher-Yates; the draws in the reference's order (DESIGN.md
 * section 8).
 *
 * ds_misspell_titles: *out = a new table (stride 255, no word counts) whose row i is generate_misspelled_name
 * (feature_engineering_prepare.py:165-173, transform_title included) of source row d_rows[i] (d_rows NULL: row i), drawn
 * from the purpose-1 stream of that source row.  Rows of the source must be transformed titles (3..255 codes 1..37, not
 * all spaces) and d_rows in range: DS_E_ARG otherwise.  Enqueued on `stream`, which is synchronised before returning. */
int ds_misspell_titles(ds_titles *source, const int32_t *d_rows, int64_t n, uint64_t seed, void *stream, ds_titles **out);
/* Copies a table back: enc[n * stride], len[n] (either may be NULL).  Synchronous. */
int ds_titles_read(const ds_titles *titles, uint8_t *enc, uint8_t *len);
/* get_closest_matches_per_training_row (feature_engineering_prepare.py:25-57) for n_queries train rows: d_rows[q * top_n
 * ..) = the top_n candidates of row q in get_closest_matches order (ds_jaccard_topk_device); sample sample_n (1..16, <=
 * top_n) of the positions with the purpose-2 stream of d_stream_index[q]; where d_own_row[q] >= 0 and the sample misses it,
 * it replaces the last sampled candidate.  Pair p = (q_first + q) * sample_n + j: d_pair_q[p] = q_first + q, d_pair_t[p] =
 * the truth row, d_target[p] = 1.0 where that row is d_own_row[q], else 0.  Asynchronous on `stream`. */
int ds_training_pairs_device(const int32_t *d_rows, int64_t n_queries, int32_t top_n, int32_t sample_n,
                             const int64_t *d_stream_index, const int32_t *d_own_row, uint64_t seed, int64_t q_first,
                             int32_t *d_pair_q, int32_t *d_pair_t, float *d_target, void *stream);

/* ---- edit scripts and the learned misspelling model ("Edit scripts and the learned misspelling
 * model"; this project's own) -----------------------------------------------------------------------------------------------
 * The alignment rule.  a is the correct title (a row of `truth`, m characters), b the observed one (a row of `observed`, n
 * characters); both are transformed titles, 3..255 codes 1..37.  D is the optimal-string-alignment distance over prefixes:
 * D[i][0] = i, D[0][j] = j, and D[i][j] is the least of D[i-1][j-1] + (a[i-1] != b[j-1]) (match or substitute), D[i-1][j] + 1
 * (delete: a[i-1] is missing in b), D[i][j-1] + 1 (insert: b[j-1] is not in a) and, when i, j > 1 and a[i-1] == b[j-2] and
 * a[i-2] == b[j-1], D[i-2][j-2] + 1 (transpose).  The traceback goes from (m, n) to (0, 0) and takes at (i, j) the first that
 * applies of: 1 match (i, j > 0, a[i-1] == b[j-1], D[i][j] == D[i-1][j-1]); 2 substitute (i, j > 0, D[i][j] == D[i-1][j-1] + 1);
 * 3 transpose (i, j > 1, the swap condition, D[i][j] == D[i-2][j-2] + 1); 4 delete (i > 0, D[i][j] == D[i-1][j] + 1); 5 insert.
 * The script is the traceback reversed, one byte per operation (DS_EDIT_OP_*); its length is at most m + n.
 *
 * The counts are one block of DS_EDIT_COUNTS int64 that is added to, never overwritten (the caller zeroes it; calls
 * accumulate).  A pair with D[m][n] > max_edits adds 1 to `skipped` and nothing else; every other pair adds 1 to `counted`,
 * to edits[D[m][n]], to seen[0] (one title end) and to seen[c] for every character c of a, and per operation of its script:
 * match[a[i-1]]; substitute[a[i-1]][b[j-1]]; delete[a[i-1]]; insert[context][b[j-1]], the context being a[i], the character in
 * front of which the insertion stands, or 0 at the end of a; transpose[a[i-2]][a[i-1]].  The tables are indexed by code,
 * 38 x 38 row-major.  Only integer additions: the block does not depend on the order of the pairs or on the launch.
 *
 * Aligns pair p = (truth row d_truth_rows[p], observed row d_observed_rows[p]) for p < n; a null row array means row p.
 * Outputs, each of which may be NULL (d_ops and d_ops_length only together): d_distance[p] = D[m][n]; d_ops + 512 * p = the
 * script followed by zeros, all 512 bytes written (d_ops 8-byte aligned); d_ops_length[p] = its length; d_counts = the block.
 * A skipped pair's distance and script are still written.  max_edits in 0..32, n in [0, 2^31); n == 0 launches nothing.
 * DS_E_ARG with nothing written: a null table, tables on two devices, n or max_edits out of range, one of d_ops and
 * d_ops_length alone, and, found by a check kernel over all pairs before anything else runs, a row out of range or a title
 * that is not 3..255 codes 1..37.
 * No stream parameter: the kernels are enqueued on the null stream, which is synchronised before returning (the check
 * kernel's verdict and the longest truth title, which sizes the LDS of the alignment kernel, come back first).
 * The option call is for tests, no result depends on it: "pairs_per_group" = waves, each with a pair, per workgroup
 * (0: 4; at most 16, and never more than 64 KiB of LDS hold), "max_blocks" = cap of the grids (0: 4096, at most 65536). */
#define DS_EDIT_OP_MATCH 0
#define DS_EDIT_OP_SUBSTITUTE 1
#define DS_EDIT_OP_DELETE 2
#define DS_EDIT_OP_INSERT 3
#define DS_EDIT_OP_TRANSPOSE 4
#define DS_EDIT_OPS_STRIDE 512
#define DS_EDIT_CODES 38
#define DS_EDIT_COUNTED 0                                       /* 1 */
#define DS_EDIT_SKIPPED 1                                       /* 1 */
#define DS_EDIT_EDITS 2                                         /* [33] */
#define DS_EDIT_SEEN (DS_EDIT_EDITS + 33)                       /* [38] */
#define DS_EDIT_MATCH (DS_EDIT_SEEN + DS_EDIT_CODES)            /* [38] */
#define DS_EDIT_DELETE (DS_EDIT_MATCH + DS_EDIT_CODES)          /* [38] */
#define DS_EDIT_SUBSTITUTE (DS_EDIT_DELETE + DS_EDIT_CODES)     /* [38][38] */
#define DS_EDIT_INSERT (DS_EDIT_SUBSTITUTE + DS_EDIT_CODES * DS_EDIT_CODES)   /* [38][38] */
#define DS_EDIT_TRANSPOSE (DS_EDIT_INSERT + DS_EDIT_CODES * DS_EDIT_CODES)    /* [38][38] */
#define DS_EDIT_COUNTS (DS_EDIT_TRANSPOSE + DS_EDIT_CODES * DS_EDIT_CODES)    /* 4481 int64 */
int ds_edit_align(const ds_titles *truth, const int32_t *d_truth_rows, const ds_titles *observed,
                  const int32_t *d_observed_rows, int64_t n, int32_t max_edits, int32_t *d_distance, uint8_t *d_ops,
                  int32_t *d_ops_length, int64_t *d_counts);
int ds_edit_option(const char *name, int64_t value);
/* *out = a new table (stride 255, no word counts) whose row i is source row d_rows[i] (d_rows NULL: row i) misspelled after
 * the counts block d_profile (DS_EDIT_COUNTS int64 in HBM, read back once and checked) and transformed.  Integer steps only:
 *   rates    with SCALE = 2^30 and S[c] the sum of a table's row c: rate_sub[c] = floor(SCALE * S_substitute[c] / seen[c]),
 *            rate_del[c] from delete[c], rate_tr[c] from transpose[c][*], rate_ins[c] from insert[c][*], c = 0..37; 0 where
 *            seen[c] == 0;
 *   stream   title i draws from the stream of (seed, DS_MISSPELL_PURPOSE_PROFILE, source row), as above; below(n) = the high
 *            64 bits of x * n with n up to 64 bits;
 *   edits    k = the smallest d >= 1 whose edits[1] + .. + edits[d] exceeds below(edits[1] + .. + edits[32]);
 *   an edit  of the working title w of length L: the positions p = 0 .. L in ascending order, at each the operations in the
 *            order substitute, delete, transpose, insert, weigh rate_sub[w[p]]; rate_del[w[p]], 0 when L <= 3; rate_tr[w[p]],
 *            0 unless p + 1 < L and w[p] != w[p+1]; rate_ins[w[p]] (rate_ins[0] at p == L), 0 when L >= 255; the first
 *            three are 0 at p == L.  T = the sum of all weights; T == 0 ends the title's edits; else below(T) picks the first
 *            (position, operation) whose cumulative weight exceeds it.  A substitute then draws the new code y != w[p] from
 *            the row substitute[w[p]][*] by below(the row's sum without y == w[p]), walking y upwards; an insert draws from
 *            insert[context][*] likewise and puts the code in front of w[p]; a transpose swaps w[p] and w[p+1];
 *   finish   transform_title as in ds_misspell_titles.
 * The profile is refused (DS_E_ARG, no table) when a count is negative or 2^40 or more, when edits[1..32] are all 0, when
 * a count that no alignment produces is not 0 (match, delete, substitute or transpose of code 0, an inserted code 0, a
 * character substituted by itself), or when a rate reaches 2^32 (4 events per seen character).  Source rows as for
 * ds_misspell_titles.  No stream parameter: the null stream, synchronised before returning. */
#define DS_MISSPELL_PURPOSE_PROFILE 8
int ds_misspell_titles_profile(ds_titles *source, const int32_t *d_rows, int64_t n, uint64_t seed, const int64_t *d_profile,
                               ds_titles **out);

/* ---- hard negatives: the wrong candidates a model likes best, mined on the device -----------------
 * The project's own rule; the reference draws its negatives at random (feature_engineering_prepare.py:25-57).  For title
 * i of a chunk of n_queries titles, over the candidates j = 0 .. k-1 with truth row c_j = d_rows[i*k + j] and margin m_j =
 * d_margins[i*k + j] (finite):
 *   eligible  0 <= c_j < n_truth, c_j != d_own_row[i] (-1: the title has no truth row), c_j not among d_exclude[i *
 *             n_exclude .. (i + 1) * n_exclude) (entries of -1 are ignored; n_exclude = 0 is legal and d_exclude may then
 *             be NULL), and m_j > min_margin: strict, both sides float32; -INFINITY means no threshold;
 *   order     by the 64-bit key (ord(m_j) << 32) | (uint32)~j descending.  ord is the monotone map of the float32 bits: all
 *             bits flipped when the sign bit is set, else the sign bit set.  So -0.0 sorts below +0.0 and equal margins go
 *             to the smaller j.  The keys of a title are distinct and never 0; 0 stands for "not eligible";
 *   yield     the first min(hard_n, eligible) candidates in that order; that may be none.
 * The output is dense: titles in title order, within a title in key order.  With *d_total = T on entry, the mined pairs of
 * this chunk take the slots T, T + 1, ... of four parallel arrays: d_pair_q = q_first + i, d_pair_t = c_j, d_position = j,
 * d_margin = m_j; on exit *d_total = T + the pairs of this chunk, so the next chunk continues there and the result does
 * not depend on how the titles are cut into chunks (nor on the grid: ds_hard_option("max_blocks", v), v in [0, 65536], 0 =
 * the default of 4096, is for tests).  Every mined pair is a negative: there is no target array.  Start *d_total at 0.
 * d_offsets: int64[n_queries] of scratch in HBM (a title's count, then its first slot).
 * Capacity: no slot >= capacity is ever written.  A chunk that would pass it leaves *d_total negative (minus the pairs
 * needed so far); every later chunk keeps it so and writes nothing.
 * DS_E_ARG before any device work: a null pointer, hard_n outside 1 .. min(16, k), n_exclude outside 0 .. 16, n_exclude
 * > 0 with a null d_exclude, a negative count, a NaN min_margin.  n_queries == 0 is DS_OK and launches nothing.
 * ds_hard_negatives_device enqueues three kernels on `stream` and does not synchronise.
 * ds_hard_total synchronises `stream` and reads the cell: *total = the pairs mined (needed, when the capacity was
 * passed: then the status is DS_E_ARG). */
int ds_hard_negatives_device(const int32_t *d_rows, const float *d_margins, int64_t n_queries, int32_t k,
                             int64_t n_truth, const int32_t *d_own_row, const int32_t *d_exclude, int32_t n_exclude,
                             int32_t hard_n, float min_margin, int64_t q_first, int64_t *d_offsets, int64_t *d_total,
                             int64_t capacity, int32_t *d_pair_q, int32_t *d_pair_t, int32_t *d_position,
                             float *d_margin, void *stream);
int ds_hard_total(const int64_t *d_total, int64_t *total, void *stream);
int ds_hard_option(const char *name, int64_t value);

/* ---- query side of Prediction on the device ("Query preparation") ---------------------------------
 * ds_prepare_titles: the n raw titles chars[offsets[i] .. offsets[i + 1]) (host pointers, offsets[0] = 0) are uploaded and
 * put through the byte work of ds_transform_titles (transform = 1: lower case, '-' -> ' ', keep [a-z0-9] and ASCII white
 * space, collapse runs of ' ', strip, cut to 255, strip, '0'-pad to 3) or taken as they are (transform = 0), then encoded
 * as ds_encode_titles with encode_title's codes (' ' 1, a-z 2..27, 0-9 28..37, any other byte 0) into *out = a new table
 * (stride 255, no word counts).  report[0..1] = 128-bit mask (bit b of the low / high word: byte b, resp. 64 + b) of the
 * bytes < 128 outside those 37 characters in the encoded titles (transform = 1) or in the raw ones (transform = 0), which
 * the caller refuses; report[2] = the first title longer than 255 characters with transform = 0, report[3] = the first
 * title holding a byte >= 128 (the Unicode step was skipped), -1 when there is none.  Either of the last two: DS_E_ARG and
 * no table, the report still filled.  Enqueued on `stream`, which is synchronised before returning. */
int ds_prepare_titles(const uint8_t *chars, const int64_t *offsets, int64_t n, int32_t transform, int device, void *stream,
                      ds_titles **out, int64_t report[4]);
/* The truth vocabulary of the native index build (ds_problem_arrays: strictly ascending big-endian tri-gram keys, idf32,
 * idf64) as a dense int32[37^3] column table, the idf arrays and max(idf64) in HBM. */
int ds_query_space_create(const uint32_t *vocabulary_keys, const float *idf32, const double *idf64, int64_t V, int device,
                          ds_query_space **out);
void ds_query_space_destroy(ds_query_space *space);
/* The Jaccard query rows of titles [first, first + n) of a table of encoded transformed titles, against the space's
 * vocabulary, bit-identical to the query rows of ds_problem_create(truth, queries) renumbered into the truth vocabulary:
 * the distinct tri-grams of a title in ascending byte order; a known one is listed in d_cols and adds idf64 to d_maxint
 * when its idf32 != 0; an unknown one is never listed and adds max(idf64) when float32(max(idf64)) != 0; d_maxint[q] is
 * the left-to-right float64 sum in that order.  Chunk-local CSR: d_rowptr[n + 1] (d_rowptr[0] = 0), d_cols ascending;
 * cols_capacity >= 253 * n.  Asynchronous on `stream`. */
int ds_query_rows_device(const ds_query_space *space, const ds_titles *titles, int64_t first, int64_t n, int64_t *d_rowptr,
                         int32_t *d_cols, double *d_maxint, int64_t cols_capacity, void *stream);

/* ---- device memory / stream / timing plumbing (so tests and bench.py can keep inputs resident in HBM) ----------- */
int ds_malloc(void **ptr, size_t bytes, int device);
int ds_free(void *ptr, int device);
int ds_memcpy_h2d(void *dst, const void *src, size_t bytes, int device);
int ds_memcpy_d2h(void *dst, const void *src, size_t bytes, int device);
int ds_memset(void *dst, int value, size_t bytes, int device);
int ds_memcpy_d2d_async(void *dst, const void *src, size_t bytes, int device, void *stream);
int ds_stream_create(int device, void **stream);   /* a HIP stream for the _device entry points and RCCL */
int ds_stream_destroy(void *stream, int device);
int ds_stream_sync(void *stream, int device);
int ds_timer_create(int device, ds_timer **out);
void ds_timer_destroy(ds_timer *timer);
int ds_timer_start(ds_timer *timer, void *stream);
int ds_timer_stop(ds_timer *timer, void *stream);
int ds_timer_elapsed_ms(ds_timer *timer, float *ms); /* synchronises on the stop event */

#ifdef __cplusplus
}
#endif
#endif /* DOPPEL_AMD_H */
