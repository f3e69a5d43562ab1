"""The reference's four prediction stages restated with the CPU oracle (predict.py:97-113 exact, :140-183 close,
:185-254 model, :256-272 finalise), shared by tests/test_gpu_prediction.py (which compares the device's answer with it)
and tests/test_reference_stages_cpu.py (which holds it against answers captured from the reference itself).  A plain
module like sweep_cases.py: no fixtures, no GPU; the oracle is an argument.
"""
import numpy as np
import pandas as pd

import doppel_speller_amd as ds
from doppel_speller_amd import prediction
from doppel_speller_amd.match_maker import NativeProblem


class Expected:
    """The stages restated with the oracle: exact dict, Jaccard top-k, close ratios, remaining pairs, features.
    rows: the candidate rows int32[Q, k] of every query, when they are given (no Jaccard stage then)."""

    def __init__(self, truth, queries, k, oracle, rows=None, levenshtein_threshold=94):
        self.truth, self.queries, self.oracle = truth, queries, oracle
        last = {}
        for row, title in enumerate(truth):
            last[title] = row
        self.exact = np.array([last.get(q, -1) for q in queries], dtype=np.int64)
        if rows is None:
            t_chars, t_offsets = prediction._pack(truth)
            q_chars, q_offsets = prediction._pack(queries)
            a = NativeProblem.from_flat(t_chars, t_offsets, q_chars, q_offsets, 3).arrays()
            rows = oracle.jaccard_topk(a["rowptr"], a["truth_idx"], a["idf32"], a["sums32"], a["q_rowptr"],
                                       a["q_cols"], a["q_maxint"], k)
        self.rows = np.asarray(rows)
        self.t_enc, self.t_len = ds.encode_titles(truth)
        self.q_enc, self.q_len = ds.encode_titles(queries)
        pair_q = np.repeat(np.arange(len(queries)), k)
        pair_t = self.rows.reshape(-1)
        ratios = oracle.close_ratios(self.q_len[pair_q], self.t_len[pair_t], self.q_enc[pair_q], self.t_enc[pair_t],
                                     ds.SPACE_CODE, ds.SORT_KEY, levenshtein_threshold)
        self.ratios = ratios.reshape(len(queries), k)
        frame = pd.DataFrame({"q": pair_q, "t": pair_t, "ratio": ratios.astype(np.int64)})
        frame = frame[frame["ratio"] > levenshtein_threshold]                           # predict.py:172
        frame = frame[frame.groupby("q")["ratio"].transform("max") == frame["ratio"]]    # :173-174
        frame = frame[~frame["q"].isin(frame.loc[frame["q"].duplicated(), "q"])]        # :176, :158-161
        self.close = np.full(len(queries), -1, dtype=np.int64)
        self.close[frame["q"].to_numpy()] = frame["t"].to_numpy()
        best = np.where(self.exact >= 0, self.exact, self.close)
        self.pair_q, self.pair_t = oracle.remaining_pairs(best, self.rows)
        self.k, self.n = k, len(queries)
        self._features = None

    @property
    def features(self):
        """construct_features of the remaining pairs (the word counts are those of the truth set itself)."""
        if self._features is None:
            t_chars, t_offsets = prediction._pack(self.truth)
            t_counts = ds.feature_engineering.truth_word_counts(t_chars, t_offsets, separators=(ord(" "),))
            self._features = self.oracle.construct_features(
                self.q_len[self.pair_q], self.t_len[self.pair_t], self.q_enc[self.pair_q], self.t_enc[self.pair_t],
                t_counts[self.pair_t], ds.SPACE_CODE, len(self.truth))
        return self._features

    def model_rows(self, probabilities, threshold, oracle):
        match_q, match_t = oracle.select_matches(self.pair_q, self.pair_t, probabilities, self.k, threshold)
        out = np.full(self.n, -1, dtype=np.int64)
        out[match_q] = match_t
        return out

    def final_rows(self, model_rows):
        """The row every query ends with, -1 for none: the exact stage first, then close, then the model (:120-121)."""
        return np.where(self.exact >= 0, self.exact, np.where(self.close >= 0, self.close, model_rows))
