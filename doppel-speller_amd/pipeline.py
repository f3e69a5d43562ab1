"""The fused device-resident hot path: Jaccard top-k -> construct_features on the surviving (query, truth) pairs.

Mirrors the two hot loops of Prediction.generate_test_predictions (predict.py:126-127 and :215-219) without the
host round trip between them: the top-k rows written by the Jaccard kernels are consumed in HBM by the feature kernel
(pair i = (query i // k, truth row rows[i])).  Inputs are uploaded once; `step()` only enqueues kernels.

This class is the one owner of the device stage sequence: bench.py and the tests build it from a synthetic workload,
Prediction builds it with `over` on its own truth side and loads one chunk of queries at a time.
"""
import ctypes

import numpy as np

from . import _lib
from .distributed import slice_queries
from .feature_engineering import FEATURES_COUNT, LEVENSHTEIN_RATIO_THRESHOLD, SORT_KEY, SPACE_CODE, TitleTable
from .match_maker import TruthIndex

PREDICTION_PROBABILITY_THRESHOLD = 0.9  # settings.py:76
# device bytes per query and candidate: features (66 float32), prediction, top-k row, ratio, pair (q, t)
BYTES_PER_PAIR = FEATURES_COUNT * 4 + 4 + 4 + 1 + 8
BYTES_PER_RANK = 4 + 4 + 1 + 1          # one slot of the rank output: row, probability, ratio, stage
BYTES_PER_PARTS = 3                     # the close ratio taken apart, per pair: d, r, s
EXHAUSTIVE_MAX_N = 64                   # slots per query of the exhaustive stage at most (ds_exhaustive_rank_device)
# what the explain stage holds per query: best pair (8), its row, probability, count and margin (4 each), the gathered
# features (66 float32) and the contributions (67 float64)
BYTES_PER_EXPLAIN = 8 + 4 * 4 + FEATURES_COUNT * 4 + (FEATURES_COUNT + 1) * 8
MAX_GRAMS = 253                         # tri-grams of a 255-character title: columns of one query row at most


class CandidatePipeline:
    def __init__(self, workload, k, device=0, q_begin=0, q_end=None, rows_ptr=None):
        """workload: an object with the fields of synth.make_workload.  Queries [q_begin, q_end) are this GPU's shard.
        rows_ptr: optional device pointer of an int32[q, k] buffer owned by the caller; allocated here when omitted."""
        q_end = workload.n_queries if q_end is None else q_end
        self._setup(TruthIndex(workload.rowptr, workload.truth_idx, workload.idf32, workload.sums32, device),
                    TitleTable(workload.t_enc, workload.t_len, workload.t_counts, device),
                    TitleTable(workload.q_enc[q_begin:q_end], workload.q_len[q_begin:q_end], None, device),
                    k, q_end - q_begin, device, rows_ptr)
        self.load_queries(*slice_queries(workload.q_rowptr, workload.q_cols, workload.q_maxint, q_begin, q_end), 0)

    @classmethod
    def over(cls, index, truth_titles, query_titles, k, capacity, device=0):
        """A pipeline on a truth index and title tables owned by the caller (shared, never closed here), with the
        buffers of every stage allocated now for `capacity` queries; `load_queries` loads each chunk."""
        out = cls.__new__(cls)
        out._setup(index, truth_titles, query_titles, k, capacity, device, None)
        out._allocate_stages()
        return out

    def _setup(self, index, truth_titles, query_titles, k, capacity, device, rows_ptr):
        self.index, self.truth_titles, self.query_titles = index, truth_titles, query_titles
        self.k, self.capacity, self.device = k, capacity, device
        self.n_truth = truth_titles.n
        self.n_queries, self.q_first = capacity, 0
        self._rows = None
        if rows_ptr is None:
            self._rows = _lib.DeviceArray((capacity, k), np.int32, device)
        self.rows_ptr = _lib.pointer(self._rows if rows_ptr is None else rows_ptr)
        self.d_features = _lib.DeviceArray((capacity * k, FEATURES_COUNT), np.float32, device)
        self._close = self._exact = self._pairs = self._predictions = self._matches = None
        self._ranked, self._ranked_n = None, 0
        self._exhaustive, self._exhaustive_n = None, 0
        self._parts = None
        self._reasons = None
        self._explain = None

    def _allocate_stages(self):
        """The outputs of the stages after top-k (by `over`, or by the first of their enqueues)."""
        if self._close is not None:
            return
        n, device = self.capacity, self.device
        size = int(_lib.lib().ds_remaining_pairs_counts_size(n))
        self._close = (_lib.DeviceArray((n, self.k), np.uint8, device), _lib.DeviceArray((n,), np.int32, device),
                       _lib.DeviceArray.from_host(np.ascontiguousarray(SORT_KEY, dtype=np.uint8), device))
        self._exact = _lib.DeviceArray((max(n, 1),), np.int32, device)
        self._pairs = (_lib.DeviceArray((n * self.k,), np.int32, device),
                       _lib.DeviceArray((n * self.k,), np.int32, device), _lib.DeviceArray((size,), np.int64, device))
        self._predictions = _lib.DeviceArray((n * self.k,), np.float32, device)
        self._matches = (_lib.DeviceArray((n,), np.int32, device), _lib.DeviceArray((n,), np.int32, device))

    def load_queries(self, q_rowptr, q_cols, q_maxint, first, last=None):
        """Upload the CSR rows of queries [first, last) (default: to the end) of the query table: the next chunk."""
        last = q_rowptr.shape[0] - 1 if last is None else last
        if not 0 <= last - first <= self.capacity:
            raise ValueError(f"queries [{first}, {last}) do not fit the {self.capacity} the buffers hold")
        rowptr, cols, maxint = slice_queries(q_rowptr, q_cols, q_maxint, first, last)
        self.d_rowptr = _lib.DeviceArray.from_host(rowptr, self.device)
        self.d_cols = _lib.DeviceArray.from_host(cols if cols.shape[0] else np.zeros(1, np.int32), self.device)
        self.d_maxint = _lib.DeviceArray.from_host(maxint, self.device)
        self.n_queries, self.q_first = last - first, first

    def load_queries_device(self, space, first, last, stream=None):
        """The CSR rows of queries [first, last) of the query table derived on the device against `space` (a
        prediction.QuerySpace: ds_query_rows_device), into buffers allocated once for `capacity` queries."""
        n = last - first
        if not 0 <= n <= self.capacity:
            raise ValueError(f"queries [{first}, {last}) do not fit the {self.capacity} the buffers hold")
        if getattr(self, "_query_rows", None) is None:
            self._query_rows = (_lib.DeviceArray((self.capacity + 1,), np.int64, self.device),
                                _lib.DeviceArray((max(1, self.capacity * MAX_GRAMS),), np.int32, self.device),
                                _lib.DeviceArray((max(1, self.capacity),), np.float64, self.device))
        rowptr, cols, maxint = self._query_rows
        _lib.check(_lib.lib().ds_query_rows_device(space.handle, self.query_titles.handle, first, n, rowptr.ptr, cols.ptr,
                                                   maxint.ptr, cols.shape[0], _lib.pointer(stream)),
                   "ds_query_rows_device")
        self.d_rowptr, self.d_cols, self.d_maxint = rowptr, cols, maxint
        self.n_queries, self.q_first = n, first

    def enqueue_top_k(self, stream=None):
        self.index.top_k_device(self.d_rowptr, self.d_cols, self.d_maxint, self.n_queries, self.k, self.rows_ptr,
                                stream)

    def enqueue_features(self, stream=None):
        _lib.check(_lib.lib().ds_construct_features_indexed_device(
            self.query_titles.handle, self.truth_titles.handle, _lib.pointer(None), self.rows_ptr, self.q_first,
            self.k, SPACE_CODE, self.n_truth, self.n_queries * self.k, self.d_features.ptr, _lib.pointer(stream)),
            "ds_construct_features_indexed_device")

    def enqueue_close_matches(self, stream=None, threshold=LEVENSHTEIN_RATIO_THRESHOLD):
        """Next row f-1 in the same device-resident flow (predict.py:140-183): the fuzzy ratio of every (query,
        candidate) pair and the unique best candidate per query, read from the top-k rows in HBM."""
        self._allocate_stages()
        ratios, best, sort_key = self._close
        _lib.check(_lib.lib().ds_close_matches_device(
            self.query_titles.handle, self.truth_titles.handle, self.rows_ptr, self.q_first, self.k, self.n_queries,
            SPACE_CODE, sort_key.ptr, int(threshold), ratios.ptr, best.ptr, _lib.pointer(stream)),
            "ds_close_matches_device")

    def close_matches(self):
        """(ratios uint8[Q, k], best_row int32[Q]) of the last `enqueue_close_matches`."""
        return self._close[0].to_host(self.n_queries), self.best_rows()

    def best_rows(self):
        """int32[Q]: the best row of `close_matches`, overridden by the exact match where `enqueue_exact_matches`
        found one after it."""
        return self._close[1].to_host(self.n_queries)

    def enqueue_exact_matches(self, stream=None):
        """The exact stage (predict.py:97-113): per query the last truth row with the same transformed title, or -1.
        After `enqueue_close_matches` it also overrides that step's best row wherever an exact match exists, so that
        `enqueue_remaining_pairs` drops the exact and the fuzzy matches in one pass.  The truth table's hash table is
        built by the first call."""
        closed = self._close is not None
        self._allocate_stages()
        _lib.check(_lib.lib().ds_exact_matches_device(self.truth_titles.handle, self.query_titles.handle, self.q_first,
                                                      self.n_queries, self._exact.ptr,
                                                      self._close[1].ptr if closed else _lib.pointer(None),
                                                      _lib.pointer(stream)), "ds_exact_matches_device")

    def exact_matches(self):
        """int32[Q]: the truth row of every query's exact match (-1: none) of the last `enqueue_exact_matches`."""
        return self._exact.to_host(self.n_queries)

    def enqueue_remaining_pairs(self, stream=None):
        """Next row f-2 (predict.py:172-183): drop the queries the fuzzy step matched (`enqueue_close_matches` first)
        and compact the (query row, truth row) pairs of the others, in order, on the device.  The query rows are
        absolute rows of the query table (q_first + local row)."""
        pair_q, pair_t, counts = self._pairs
        _lib.check(_lib.lib().ds_remaining_pairs_device(self._close[1].ptr, self.rows_ptr, self.n_queries, self.k,
                                                        self.q_first, pair_q.ptr, pair_t.ptr, counts.ptr,
                                                        _lib.pointer(stream)), "ds_remaining_pairs_device")

    def remaining_counts(self, stream=None):
        """(remaining queries, pairs) of the last `enqueue_remaining_pairs` (synchronises the stream)."""
        _lib.check(_lib.lib().ds_stream_sync(_lib.pointer(stream), self.device), "sync")
        n_remaining, n_pairs = self._pairs[2].to_host(2)
        return int(n_remaining), int(n_pairs)

    def remaining_pairs(self, n_pairs):
        pair_q, pair_t, _ = self._pairs
        return pair_q.to_host(n_pairs), pair_t.to_host(n_pairs)

    def enqueue_features_remaining(self, n_pairs, stream=None):
        """construct_features on the compacted pair list only (predict.py:195-219), into the first n_pairs rows."""
        pair_q, pair_t, _ = self._pairs
        _lib.check(_lib.lib().ds_construct_features_indexed_device(
            self.query_titles.handle, self.truth_titles.handle, pair_q.ptr, pair_t.ptr, 0, self.k, SPACE_CODE,
            self.n_truth, n_pairs, self.d_features.ptr, _lib.pointer(stream)),
            "ds_construct_features_indexed_device")

    def enqueue_predict(self, model, stream=None, n_pairs=None):
        """Next row f-4: the tree ensemble (predict.py:229-234) on the feature matrix resident in HBM."""
        self._allocate_stages()
        n_pairs = self.n_queries * self.k if n_pairs is None else n_pairs
        model.predict_device(self.d_features, n_pairs, None, self._predictions, stream)

    def enqueue_select_matches(self, n_remaining, threshold=PREDICTION_PROBABILITY_THRESHOLD, stream=None):
        """predict.py:246-252 on the predictions of the compacted pairs: per remaining query the single pair with the
        maximum prediction above the threshold."""
        pair_q, pair_t, _ = self._pairs
        _lib.check(_lib.lib().ds_select_matches_device(pair_q.ptr, pair_t.ptr, self._predictions.ptr, n_remaining, self.k,
                                                       float(threshold), self._matches[0].ptr, self._matches[1].ptr,
                                                       _lib.pointer(stream)), "ds_select_matches_device")

    def enqueue_rank_matches(self, n, stream=None):
        """The best n candidates of every query in order (ds_rank_matches_device): the exact or close match first, then
        the others by the model's probability, over this pipeline's own buffers: the top-k rows, the predictions of
        `enqueue_predict` on all pairs, the ratios and best rows of `enqueue_close_matches` and the exact rows of
        `enqueue_exact_matches`.  The outputs are allocated by the first call, for `capacity` queries of n slots."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= self.k:
            raise ValueError(f"n must be an integer in [1, k = {self.k}], not {n!r}")
        self._allocate_stages()
        if self._ranked is None or self._ranked[0].shape[0] < self.capacity * n:
            size, device = max(1, self.capacity * int(n)), self.device
            self._ranked = (_lib.DeviceArray((size,), np.int32, device), _lib.DeviceArray((size,), np.float32, device),
                            _lib.DeviceArray((size,), np.uint8, device), _lib.DeviceArray((size,), np.int8, device))
        self._ranked_n = int(n)
        _lib.check(_lib.lib().ds_rank_matches_device(
            self.rows_ptr, self._predictions.ptr, self._close[0].ptr, self._exact.ptr, self._close[1].ptr,
            self.n_queries, self.k, self._ranked_n, self.n_truth, *(a.ptr for a in self._ranked), _lib.pointer(stream)),
            "ds_rank_matches_device")

    def ranked(self, n):
        """(rows int32[Q, n], probabilities float32[Q, n], ratios uint8[Q, n], stages int8[Q, n]) of the last
        `enqueue_rank_matches(n)`: only the n slots per query are copied back."""
        if n != self._ranked_n:
            raise ValueError(f"the last enqueue_rank_matches ranked {self._ranked_n} slots per query, not {n}")
        return tuple(a.to_host(self.n_queries * n).reshape(self.n_queries, n) for a in self._ranked)

    def ranked_probabilities_device(self):
        """The float32[Q * n] probabilities of the last `enqueue_rank_matches` where they lie in HBM."""
        return self._ranked[1]

    def exhaustive_probabilities_device(self):
        """The float32[Q * n] probabilities of the last `enqueue_exhaustive` where they lie in HBM."""
        return self._exhaustive[1]

    def explained_probabilities_device(self):
        """The float32[Q] probabilities of the last `enqueue_explain` where they lie in HBM."""
        return self._explain["probability"]

    def enqueue_assign_edges(self, keys, rows, probability_threshold, stream=None):
        """The one-to-one stage's view of this chunk's ranked slots (ds_assign_edges_device), after
        `enqueue_rank_matches(n)`, over its outputs: per slot the key of its edge (0: no edge) and its row, written into
        the call-wide `keys` uint64[Q, n] and `rows` int32[Q, n] in HBM at this chunk's first title (`q_first`).  A
        model slot is an edge when its probability is above `probability_threshold` (float32)."""
        if self._ranked is None or not self._ranked_n:
            raise ValueError("enqueue_rank_matches comes first")
        if tuple(keys.shape) != tuple(rows.shape) or len(keys.shape) != 2 or keys.shape[1] != self._ranked_n:
            raise ValueError(f"keys {tuple(keys.shape)} and rows {tuple(rows.shape)} must both be "
                             f"[titles, n = {self._ranked_n}]")
        _lib.check(_lib.lib().ds_assign_edges_device(
            *(a.ptr for a in self._ranked), self.q_first, self.n_queries, keys.shape[0], self._ranked_n, self.n_truth,
            float(probability_threshold), _lib.pointer(keys), _lib.pointer(rows), _lib.pointer(stream)),
            "ds_assign_edges_device")

    def enqueue_exhaustive(self, model, n, stream=None):
        """The best n rows of the WHOLE truth table per query by the model alone (ds_exhaustive_rank_device): tiles of
        pairs through the features and forest kernels, folded into n running keys per query, with no use of the top-k
        rows and no exact or close override.  The stage allocates its workspace per call and frees it before it
        returns, so `stream` is synchronised at the end.  The outputs are allocated by the first call, for `capacity`
        queries of n slots."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= EXHAUSTIVE_MAX_N:
            raise ValueError(f"n must be an integer in [1, {EXHAUSTIVE_MAX_N}], not {n!r}")
        if self._exhaustive is None or self._exhaustive[0].shape[0] < self.capacity * n:
            size, device = max(1, self.capacity * int(n)), self.device
            self._exhaustive = (_lib.DeviceArray((size,), np.int32, device), _lib.DeviceArray((size,), np.float32, device))
        self._exhaustive_n = int(n)
        _lib.check(_lib.lib().ds_exhaustive_rank_device(
            self.query_titles.handle, self.truth_titles.handle, model.handle, self.q_first, self.n_queries,
            self._exhaustive_n, SPACE_CODE, self.n_truth, *(a.ptr for a in self._exhaustive), _lib.pointer(stream)),
            "ds_exhaustive_rank_device")

    def exhaustive(self, n):
        """(rows int32[Q, n], probabilities float32[Q, n]) of the last `enqueue_exhaustive(model, n)`; a slot with no
        row (fewer than n truth titles) holds -1 and NaN."""
        if n != self._exhaustive_n:
            raise ValueError(f"the last enqueue_exhaustive kept {self._exhaustive_n} slots per query, not {n}")
        return tuple(a.to_host(self.n_queries * n).reshape(self.n_queries, n) for a in self._exhaustive)

    def enqueue_close_parts(self, t_min, t_max, stream=None):
        """The close ratio of every (query, candidate) pair taken apart (ds_close_parts_device), so that it can be read at
        any Levenshtein threshold in [t_min, t_max] afterwards; what no threshold of that range can read is skipped.  The
        three outputs are allocated by the first call, for `capacity` queries."""
        self._allocate_stages()
        if self._parts is None:
            self._parts = tuple(_lib.DeviceArray((self.capacity, self.k), np.uint8, self.device) for _ in range(3))
        _lib.check(_lib.lib().ds_close_parts_device(
            self.query_titles.handle, self.truth_titles.handle, self.rows_ptr, self.q_first, self.k, self.n_queries,
            SPACE_CODE, self._close[2].ptr, int(t_min), int(t_max), *(a.ptr for a in self._parts), _lib.pointer(stream)),
            "ds_close_parts_device")

    def close_parts(self):
        """(d, r, s), uint8[Q, k] each, of the last `enqueue_close_parts`: the ratio at an integer threshold t is 0 when
        t > d, r when r > t, else s."""
        return tuple(a.to_host(self.n_queries) for a in self._parts)

    def enqueue_threshold_sweep(self, actual_rows, lev, prob, counts, stream=None):
        """The outcome counters of every (Levenshtein threshold, probability threshold) cell for this chunk's queries,
        ADDED to `counts` (ds_threshold_sweep_device), over this pipeline's own buffers: the top-k rows, the parts of
        `enqueue_close_parts`, the predictions of `enqueue_predict` on all pairs and the exact rows of
        `enqueue_exact_matches`.  actual_rows: int32[Q] in HBM, the truth row each query should get, -1 for none; lev:
        int32[T] and prob: float32[U] in HBM, strictly ascending; counts: int64[T * U * 4] in HBM."""
        if self._parts is None:
            raise ValueError("enqueue_close_parts comes first")
        _lib.check(_lib.lib().ds_threshold_sweep_device(
            self.rows_ptr, *(a.ptr for a in self._parts), self._predictions.ptr, self._exact.ptr,
            _lib.pointer(actual_rows), self.n_queries, self.k, _lib.pointer(lev), lev.shape[0], _lib.pointer(prob),
            prob.shape[0], _lib.pointer(counts), _lib.pointer(stream)), "ds_threshold_sweep_device")

    def enqueue_sweep_records(self, actual_rows, lev, prob, records):
        """What the decision rule leaves of every query of this chunk at every Levenshtein threshold, for all probability
        thresholds at once (ds_sweep_records_device; the encoding is in include/doppel_amd.h), over the buffers that
        `enqueue_threshold_sweep` reads.  actual_rows, lev and prob as there; records: uint16[Q * T] in HBM, the place
        of this chunk's first query (a DeviceArray, a c_void_p or an address).  On the null stream, like every stage
        of Prediction."""
        if self._parts is None:
            raise ValueError("enqueue_close_parts comes first")
        _lib.check(_lib.lib().ds_sweep_records_device(
            self.rows_ptr, *(a.ptr for a in self._parts), self._predictions.ptr, self._exact.ptr,
            _lib.pointer(actual_rows), self.n_queries, self.k, _lib.pointer(lev), lev.shape[0], _lib.pointer(prob),
            prob.shape[0], _lib.pointer(records)), "ds_sweep_records_device")

    def enqueue_duplicate_links(self, parent, counts, levenshtein_threshold, probability_threshold, use_model,
                                reasons=False, stream=None):
        """The links among this chunk's rows and their candidates joined into the union-find forest `parent`
        (ds_duplicate_links_device), for a pipeline whose query table IS its truth table, over this pipeline's own
        buffers: the top-k rows, the ratios of `enqueue_close_matches`, the exact rows of `enqueue_exact_matches` and,
        with `use_model`, the predictions of `enqueue_predict` on all pairs.  parent: int32[n_truth] in HBM, counts:
        int64[3] in HBM (exact, close, model links), both started by ds_duplicate_begin_device and ADDED to.  reasons:
        keep the reason of every slot for `duplicate_reasons` (the buffer is allocated by the first call that asks)."""
        self._allocate_stages()
        if reasons and self._reasons is None:
            self._reasons = _lib.DeviceArray((self.capacity, self.k), np.uint8, self.device)
        _lib.check(_lib.lib().ds_duplicate_links_device(
            self.rows_ptr, self._close[0].ptr, self._predictions.ptr if use_model else _lib.pointer(None),
            self._exact.ptr, self.q_first, self.n_queries, self.k, self.n_truth, int(levenshtein_threshold),
            float(probability_threshold), _lib.pointer(parent), self._reasons.ptr if reasons else _lib.pointer(None),
            _lib.pointer(counts), _lib.pointer(stream)), "ds_duplicate_links_device")

    def duplicate_reasons(self):
        """uint8[Q, k] of the last `enqueue_duplicate_links(reasons=True)`: bit 0 close, bit 1 model, 0 for a slot that
        links nothing."""
        if self._reasons is None:
            raise ValueError("enqueue_duplicate_links(reasons=True) comes first")
        return self._reasons.to_host(self.n_queries)

    def enqueue_explain(self, model, approximate=False, stream=None):
        """Why the model scored each query's best candidate as it did, over this pipeline's own buffers: the best pair
        per query by the predictions of `enqueue_predict` on all pairs (ds_best_pairs_device: the highest probability,
        the first in top-k order on a tie), its feature row gathered from those of `enqueue_features`
        (ds_gather_rows_device), the margin of that row and its contributions (model.predict_contributions_device).
        The outputs are allocated by the first call, for `capacity` queries.  The gather synchronises `stream`."""
        self._allocate_stages()
        if self._explain is None:
            n, device, width = max(1, self.capacity), self.device, FEATURES_COUNT
            self._explain = dict(pair=_lib.DeviceArray((n,), np.int64, device), row=_lib.DeviceArray((n,), np.int32, device),
                                 probability=_lib.DeviceArray((n,), np.float32, device),
                                 count=_lib.DeviceArray((n,), np.int32, device),
                                 margin=_lib.DeviceArray((n,), np.float32, device),
                                 features=_lib.DeviceArray((n, width), np.float32, device),
                                 contributions=_lib.DeviceArray((n, width + 1), np.float64, device))
        e, library, n = self._explain, _lib.lib(), self.n_queries
        _lib.check(library.ds_best_pairs_device(self.rows_ptr, self._predictions.ptr, n, self.k, e["pair"].ptr,
                                                e["row"].ptr, e["probability"].ptr, e["count"].ptr,
                                                _lib.pointer(stream)), "ds_best_pairs_device")
        _lib.check(library.ds_gather_rows_device(self.d_features.ptr, FEATURES_COUNT, e["pair"].ptr, n, n * self.k,
                                                 e["features"].ptr, _lib.pointer(stream)), "ds_gather_rows_device")
        model.predict_device(e["features"], n, e["margin"], None, stream)
        model.predict_contributions_device(e["features"], n, e["contributions"], approximate, stream)

    def explained(self):
        """Of the last `enqueue_explain`, per query: (row int32[Q], probability float32[Q], count int32[Q] of the
        candidates that hold that probability, margin float32[Q], features float32[Q, 66], contributions
        float64[Q, 67], the bias last)."""
        e, n = self._explain, self.n_queries
        return tuple(e[name].to_host(n) for name in ("row", "probability", "count", "margin", "features",
                                                     "contributions"))

    def matches(self, n_remaining):
        """(query rows, matched truth row or -1) of the last `enqueue_select_matches`."""
        return self._matches[0].to_host(n_remaining), self._matches[1].to_host(n_remaining)

    def predictions(self, n_pairs=None):
        if n_pairs is None:
            return self._predictions.to_host(self.n_queries * self.k).reshape(self.n_queries, self.k)
        return self._predictions.to_host(n_pairs)

    def step(self, stream=None):
        self.enqueue_top_k(stream)
        self.enqueue_features(stream)

    def sync(self, stream=None):
        return self.index.sync(stream)

    def rows(self):
        out = np.empty((self.n_queries, self.k), dtype=np.int32)
        _lib.check(_lib.lib().ds_memcpy_d2h(_lib.pointer(out), self.rows_ptr, out.nbytes, self.device), "d2h")
        return out

    def features_of(self, queries):
        """float32[len(queries) * k, 66]: the feature rows of the given queries' pairs (one small copy per query)."""
        queries = np.asarray(queries, dtype=np.int64)
        out = np.empty((queries.shape[0] * self.k, FEATURES_COUNT), dtype=np.float32)
        row_bytes = FEATURES_COUNT * 4 * self.k
        for i, q in enumerate(queries):
            source = ctypes.c_void_p(self.d_features.ptr.value + int(q) * row_bytes)
            _lib.check(_lib.lib().ds_memcpy_d2h(ctypes.c_void_p(out.ctypes.data + i * row_bytes), source, row_bytes,
                                                self.device), "d2h")
        return out

    def features(self, n_pairs=None, first_pair=0):
        """float32[n_pairs, 66] of the last `enqueue_features`, pairs [first_pair, first_pair + n_pairs) (default: all)."""
        if n_pairs is None:
            n_pairs = self.n_queries * self.k - first_pair
        out = np.empty((n_pairs, FEATURES_COUNT), dtype=np.float32)
        source = ctypes.c_void_p(self.d_features.ptr.value + first_pair * FEATURES_COUNT * 4)
        _lib.check(_lib.lib().ds_memcpy_d2h(_lib.pointer(out), source, out.nbytes, self.device), "d2h")
        return out
