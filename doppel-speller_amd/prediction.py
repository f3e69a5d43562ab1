"""Prediction.generate_test_predictions (doppelspeller/predict.py:256-300) end to end on the GPU: one answer per title.

The four stages of the reference, in its order of priority:

    1. exact    the transformed title is a truth title (predict.py:97-113; the last truth row of a title wins)
    2. close    the fuzzy ratio of a top-n candidate is above the Levenshtein threshold (:140-183)
    3. model    the tree ensemble on the features of the remaining queries' candidates (:185-254)
    4. none     title_id -1 (settings.TRAIN_NOT_FOUND_VALUE, :256-272)

Per chunk of queries every stage runs on the device (Jaccard top-k, close matches, the exact override, the pair list of
the remaining queries, construct_features, the forest, the match selection); the per-query results come back once.
The truth side (inverted index, encoded titles, word counts, the exact-match table) is built once by the constructor.

Differences from the reference, on purpose:
  - `truth_title_ids` must be unique: the reference keeps two dicts (title -> id, id -> title) whose meaning is only
    defined for unique ids.
  - `closest_search_single_title` returns the exact or close match when there is one; the reference raises there
    (`_find_matches_using_model` is reached with no rows and `np.vstack([])` fails).
"""
import collections
import contextlib
import ctypes
import time
import unicodedata

import numpy as np

from . import _lib
from .feature_engineering import (ALLOWED_CHARACTERS, LEVENSHTEIN_RATIO_THRESHOLD, TitleTable, encode_collection,
                                  truth_word_counts)
from .match_maker import NativeProblem, TruthIndex, validate_index_build
from .pipeline import (BYTES_PER_EXPLAIN, BYTES_PER_PAIR, BYTES_PER_PARTS, BYTES_PER_RANK, EXHAUSTIVE_MAX_N, MAX_GRAMS,
                       PREDICTION_PROBABILITY_THRESHOLD, CandidatePipeline)

TRAIN_NOT_FOUND_VALUE = -1               # settings.py:80
N_GRAM = 3                               # settings.py:15
PREPARE_QUERIES = ("device", "host")
STAGE_NONE, STAGE_EXACT, STAGE_CLOSE, STAGE_MODEL = 0, 1, 2, 3
RANKED_COLUMNS = ("test_index", "rank", "title_id", "match_row", "probability", "levenshtein_ratio", "stage")
EXHAUSTIVE_COLUMNS = ("test_index", "rank", "title_id", "match_row", "probability", "jaccard_position")
SWEEP_COLUMNS = ("levenshtein_threshold", "probability_threshold", "correctly_matched", "incorrectly_matched",
                 "correctly_not_found", "incorrectly_not_found", "custom_error")
ACCURACY_KEYS = SWEEP_COLUMNS[2:]
DUPLICATE_COLUMNS = ("group_id", "group_size", "title_id", "row")
LINK_COLUMNS = ("row", "match_row", "title_id", "match_title_id", "levenshtein_ratio", "probability", "stage")
EXPLAIN_COLUMNS = ("test_index", "match_row", "title_id", "probability", "margin", "bias", "stage", "answer_row")
ASSIGNMENT_COLUMNS = ("test_index", "match_row", "title_id", "stage", "probability", "levenshtein_ratio", "rank",
                      "first_choice_row", "displaced")
ASSIGNMENT_COUNTS = ("edges", "matched", "displaced", "displaced_unmatched", "proposals", "rounds")
ASSIGN_RESERVE_BYTES = 64 << 20          # HBM left free for the kernels that follow, as the native stages leave
REASON_CLOSE, REASON_MODEL = 1, 2        # bits of a slot's reason (ds_duplicate_links_device)
SWEEP_MAX_LEVENSHTEIN, SWEEP_MAX_PROBABILITY = 101, 256      # thresholds per axis at most (ds_threshold_sweep_device)
# what ranked_matches(keep_candidates=True) keeps of a call, per query: the top-n rows, their fuzzy ratios and model
# probabilities, the exact row and the close row (-1: none; the close row also where the exact stage matched)
Candidates = collections.namedtuple("Candidates", ("rows", "ratios", "probabilities", "exact", "close"))

_CODE_OF = np.zeros(256, dtype=np.uint8)      # ASCII byte -> code of encode_title (feature_engineering.py:298-307)
_ALLOWED = np.zeros(256, dtype=bool)          # the characters a transformed title may hold (the fill '-' is not one)
for _code, _character in enumerate(ALLOWED_CHARACTERS):
    _CODE_OF[ord(_character)] = _code
    _ALLOWED[ord(_character)] = _code != 0
ALLOWED_CHARACTERS_BYTES = np.frombuffer(ALLOWED_CHARACTERS.encode("ascii"), dtype=np.uint8)      # code -> ASCII byte


def _positive_integer(value, name, or_none=False):
    """`value` as an int; a bool, another type or a value below 1 is refused by `name` (None passes with or_none)."""
    if value is None and or_none:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 1:
        raise ValueError(f"{name} must be a positive integer{' or None' if or_none else ''}, not {value!r}")
    return int(value)


def _validate_chunk(chunk_queries):
    _positive_integer(chunk_queries, "chunk_queries", or_none=True)


def validate_truth(truth_titles, truth_title_ids, top_n):
    """The constructor's checks (no library needed): int64 ids, one per title, unique and non-negative."""
    ids = np.asarray(truth_title_ids)
    if ids.ndim != 1 or len(truth_titles) != ids.shape[0]:
        raise ValueError(f"{len(truth_titles)} truth titles but {ids.reshape(-1).shape[0]} title ids")
    if ids.shape[0] and not np.issubdtype(ids.dtype, np.integer):
        raise ValueError(f"truth title ids must be integers, not {ids.dtype}")
    ids = ids.astype(np.int64)
    if ids.shape[0] and ids.min() < 0:
        raise ValueError("truth title ids must be non-negative (-1 is the 'not found' answer)")
    if np.unique(ids).shape[0] != ids.shape[0]:
        raise ValueError("truth title ids must be unique")
    if _positive_integer(top_n, "top_n") > ids.shape[0]:
        raise ValueError(f"top_n = {top_n} exceeds the {ids.shape[0]} truth titles")
    return ids


def validate_queries(titles, test_index):
    """generate_test_predictions' checks: int64 test indexes, one per title, unique."""
    if test_index is None:
        return np.arange(len(titles), dtype=np.int64)
    index = np.asarray(test_index)
    if index.ndim != 1 or index.shape[0] != len(titles):
        raise ValueError(f"{len(titles)} titles but {index.reshape(-1).shape[0]} test indexes")
    if index.shape[0] and not np.issubdtype(index.dtype, np.integer):
        raise ValueError(f"test indexes must be integers, not {index.dtype}")
    index = index.astype(np.int64)
    if np.unique(index).shape[0] != index.shape[0]:
        raise ValueError("test indexes must be unique")
    return index


def validate_rank(n, top_n):
    """ranked_matches' check of `n` (no library needed): a positive integer up to the top_n candidates of a query."""
    if _positive_integer(n, "n") > top_n:
        raise ValueError(f"n = {n} exceeds the top_n = {top_n} candidates of a title")
    return int(n)


def title_ids_of(rows, truth_title_ids):
    """int64: the title id of every truth row of `rows`, -1 (TRAIN_NOT_FOUND_VALUE) where the row is -1."""
    rows = np.asarray(rows, dtype=np.int64)
    title_id = np.full(rows.shape[0], TRAIN_NOT_FOUND_VALUE, dtype=np.int64)
    title_id[rows >= 0] = np.asarray(truth_title_ids, dtype=np.int64)[rows[rows >= 0]]
    return title_id


def _filled_slots(test_index, filled):
    """(query, slot) of the true entries of `filled` [Q, n] in the order of a long frame: by test index, then slot."""
    query, slot = np.nonzero(filled)
    order = np.argsort(test_index[query], kind="stable")
    return query[order], slot[order]


def _rank_slots(count, n):
    """The unfilled [count, n] slots of the rank stage: rows, probabilities, ratios, stages."""
    return (np.full((count, n), -1, dtype=np.int32), np.full((count, n), np.nan, dtype=np.float32),
            np.zeros((count, n), dtype=np.uint8), np.zeros((count, n), dtype=np.int8))


def _with_calibrated(frame, calibrated):
    """The frame with `calibrated_probability` (float32, one value per line) directly after `probability`; the frame
    as it is for None."""
    if calibrated is not None:
        frame.insert(list(frame.columns).index("probability") + 1, "calibrated_probability",
                     np.asarray(calibrated, dtype=np.float32))
    return frame


def ranked_frame(test_index, rows, probabilities, ratios, stages, truth_title_ids, calibrated=None):
    """ranked_matches' answer from the [Q, n] slots of the rank stage: one line per filled slot (stage != 0), sorted by
    test_index, then rank (slot + 1: the filled slots of a query come first).  calibrated: None, or the calibrator's
    map of the [Q, n] probabilities; an exact or close slot, whose probability is the constant 1.0, keeps 1.0."""
    import pandas as pd
    test_index = np.asarray(test_index, dtype=np.int64)
    query, slot = _filled_slots(test_index, np.asarray(stages) != STAGE_NONE)
    match_row = np.asarray(rows)[query, slot].astype(np.int64)
    stage = np.asarray(stages, dtype=np.int8)[query, slot]
    if calibrated is not None:
        calibrated = np.where(stage == STAGE_MODEL, np.asarray(calibrated, dtype=np.float32)[query, slot], np.float32(1))
    return _with_calibrated(
        pd.DataFrame({"test_index": test_index[query], "rank": slot.astype(np.int64) + 1,
                      "title_id": np.asarray(truth_title_ids, dtype=np.int64)[match_row], "match_row": match_row,
                      "probability": np.asarray(probabilities, dtype=np.float32)[query, slot],
                      "levenshtein_ratio": np.asarray(ratios, dtype=np.uint8)[query, slot],
                      "stage": stage}, columns=list(RANKED_COLUMNS)), calibrated)


def validate_exhaustive(n, n_truth):
    """exhaustive_matches' check of `n` (no library needed): a positive integer up to 64 and up to the truth titles."""
    if _positive_integer(n, "n") > min(EXHAUSTIVE_MAX_N, n_truth):
        raise ValueError(f"n = {n} exceeds the smaller of {EXHAUSTIVE_MAX_N} and the {n_truth} truth titles")
    return int(n)


def jaccard_positions(rows, top_rows):
    """int32[Q, n]: where each of `rows` [Q, n] stands in its query's Jaccard rows `top_rows` [Q, top_n] (the first such
    column), -1 where it does not, and for an unfilled slot (row < 0)."""
    rows, top_rows = np.asarray(rows), np.asarray(top_rows)
    out = np.full(rows.shape, -1, dtype=np.int32)
    block = 4096                                    # queries at a time: block * n * top_n booleans
    for first in range(0, rows.shape[0], block):
        same = rows[first:first + block, :, None] == top_rows[first:first + block, None, :]
        same &= (rows[first:first + block] >= 0)[:, :, None]
        out[first:first + block] = np.where(same.any(axis=2), same.argmax(axis=2), -1)
    return out


def exhaustive_frame(test_index, rows, probabilities, top_rows, truth_title_ids, calibrated=None):
    """exhaustive_matches' answer from the [Q, n] slots of the exhaustive stage and the [Q, top_n] Jaccard rows: one line
    per filled slot (row >= 0), sorted by test_index, then rank (slot + 1: the filled slots of a query come first).
    calibrated: None, or the calibrator's map of the [Q, n] probabilities."""
    import pandas as pd
    test_index = np.asarray(test_index, dtype=np.int64)
    rows = np.asarray(rows)
    positions = jaccard_positions(rows, top_rows)
    query, slot = _filled_slots(test_index, rows >= 0)
    match_row = rows[query, slot].astype(np.int64)
    return _with_calibrated(
        pd.DataFrame({"test_index": test_index[query], "rank": slot.astype(np.int64) + 1,
                      "title_id": np.asarray(truth_title_ids, dtype=np.int64)[match_row], "match_row": match_row,
                      "probability": np.asarray(probabilities, dtype=np.float32)[query, slot],
                      "jaccard_position": positions[query, slot]}, columns=list(EXHAUSTIVE_COLUMNS)),
        None if calibrated is None else np.asarray(calibrated, dtype=np.float32)[query, slot])


def predictions_accuracy(predicted_title_ids, actual_title_ids):
    """get-predictions-accuracy (cli.py:107-128) on two aligned id arrays, -1 = not found: a dict of correctly_matched,
    incorrectly_matched, correctly_not_found, incorrectly_not_found and custom_error = incorrectly_not_found +
    5 * incorrectly_matched."""
    predicted, actual = np.asarray(predicted_title_ids), np.asarray(actual_title_ids)
    if predicted.ndim != 1 or predicted.shape != actual.shape:
        raise ValueError(f"{predicted.reshape(-1).shape[0]} predicted ids but {actual.reshape(-1).shape[0]} actual ids")
    found, same = predicted != TRAIN_NOT_FOUND_VALUE, predicted == actual
    counts = [int((found & same).sum()), int((found & ~same).sum()), int((~found & same).sum()),
              int((~found & ~same).sum())]
    return dict(zip(ACCURACY_KEYS, counts + [counts[3] + 5 * counts[1]]))


def _integers(values, what):
    values = np.asarray(values)
    if values.ndim != 1:
        raise ValueError(f"{what} must be one-dimensional")
    if values.shape[0] and (values.dtype == bool or not np.issubdtype(values.dtype, np.integer)):
        raise ValueError(f"{what} must be integers, not {values.dtype}")
    return values.astype(np.int64)


def validate_sweep(levenshtein_thresholds, probability_thresholds, actual_title_ids, truth_title_ids, n_titles):
    """threshold_sweep's checks (no library needed) -> (lev int32[T], prob float32[U], shown float64[U], actual_row
    int32[n_titles]).  The thresholds come back sorted and without repeats: 1..101 integers in [0, 100], and 1..256
    finite numbers that are compared as float32 (`shown` holds, for each, the first given number with that float32
    value).  actual_row is the truth row of every actual id, -1 for the id -1; any other id that is not one of
    truth_title_ids is refused by name."""
    lev = _integers(levenshtein_thresholds, "levenshtein_thresholds")
    if lev.shape[0] == 0 or lev.min() < 0 or lev.max() > 100:
        raise ValueError("levenshtein_thresholds must hold integers in [0, 100], one at least")
    lev = np.unique(lev).astype(np.int32)
    if lev.shape[0] > SWEEP_MAX_LEVENSHTEIN:
        raise ValueError(f"{lev.shape[0]} levenshtein_thresholds, {SWEEP_MAX_LEVENSHTEIN} at most")
    given = np.asarray(probability_thresholds)
    if given.ndim != 1 or given.shape[0] == 0 or given.dtype == bool or not (
            np.issubdtype(given.dtype, np.floating) or np.issubdtype(given.dtype, np.integer)):
        raise ValueError("probability_thresholds must be a one-dimensional sequence of numbers, one at least")
    given = given.astype(np.float64)
    with np.errstate(over="ignore"):
        prob = given.astype(np.float32)
    if not np.isfinite(prob).all():
        raise ValueError("probability_thresholds must be finite")
    prob, first = np.unique(prob, return_index=True)
    if prob.shape[0] > SWEEP_MAX_PROBABILITY:
        raise ValueError(f"{prob.shape[0]} probability_thresholds, {SWEEP_MAX_PROBABILITY} at most")
    actual = _integers(actual_title_ids, "actual_title_ids")
    if actual.shape[0] != n_titles:
        raise ValueError(f"{n_titles} titles but {actual.shape[0]} actual title ids")
    ids = np.asarray(truth_title_ids, dtype=np.int64)
    order = np.argsort(ids, kind="stable")
    at = np.minimum(np.searchsorted(ids[order], actual), max(ids.shape[0] - 1, 0))
    row = order[at] if ids.shape[0] else np.zeros(actual.shape[0], dtype=np.int64)
    known = (ids[row] == actual) if ids.shape[0] else np.zeros(actual.shape[0], dtype=bool)
    missing = actual != TRAIN_NOT_FOUND_VALUE
    if (missing & ~known).any():
        raise ValueError(f"actual title id {int(actual[missing & ~known][0])} is neither "
                         f"{TRAIN_NOT_FOUND_VALUE} nor an id of the truth set")
    return lev, prob, given[first], np.where(missing, row, -1).astype(np.int32)


def sweep_frame(lev, shown, counts):
    """threshold_sweep's answer from the counters int64[T, U, 4]: one line per cell, sorted by both thresholds."""
    import pandas as pd
    counts = np.asarray(counts, dtype=np.int64).reshape(len(lev), len(shown), 4)
    columns = {"levenshtein_threshold": np.repeat(np.asarray(lev, dtype=np.int64), len(shown)),
               "probability_threshold": np.tile(np.asarray(shown, dtype=np.float64), len(lev))}
    for c, name in enumerate(ACCURACY_KEYS[:4]):
        columns[name] = counts[:, :, c].reshape(-1)
    columns["custom_error"] = (counts[:, :, 3] + 5 * counts[:, :, 1]).reshape(-1)
    return pd.DataFrame(columns, columns=list(SWEEP_COLUMNS))


def validate_duplicates(levenshtein_threshold, probability_threshold):
    """duplicate_groups' checks of its thresholds (no library needed) -> (int, float): an integer in [0, 100] (a bool is
    refused) and a finite number, which is compared as float32 like probability_threshold."""
    if isinstance(levenshtein_threshold, bool) or not isinstance(levenshtein_threshold, (int, np.integer)) or \
            not 0 <= levenshtein_threshold <= 100:
        raise ValueError(f"levenshtein_threshold must be an integer in [0, 100], not {levenshtein_threshold!r}")
    if isinstance(probability_threshold, (bool, np.bool_)) or \
            not isinstance(probability_threshold, (int, float, np.integer, np.floating)):
        raise ValueError(f"probability_threshold must be a finite number, not {probability_threshold!r}")
    with np.errstate(over="ignore"):
        finite = np.isfinite(np.float32(probability_threshold))
    if not finite:
        raise ValueError(f"probability_threshold must be a finite number, not {probability_threshold!r}")
    return int(levenshtein_threshold), float(probability_threshold)


def duplicate_frame(labels, sizes, truth_title_ids):
    """duplicate_groups' answer from the labels (a row's group = the lowest row of it) and sizes int32[n_truth] of the
    finish step: one line per row whose group holds two rows at least, sorted by the group's lowest row, then by row;
    group_id is the title id of that lowest row."""
    import pandas as pd
    labels, sizes = np.asarray(labels).astype(np.int64), np.asarray(sizes).astype(np.int64)
    ids = np.asarray(truth_title_ids, dtype=np.int64)
    row = np.nonzero(sizes >= 2)[0].astype(np.int64)
    row = row[np.argsort(labels[row], kind="stable")]
    return pd.DataFrame({"group_id": ids[labels[row]], "group_size": sizes[row], "title_id": ids[row], "row": row},
                        columns=list(DUPLICATE_COLUMNS))


def links_frame(chunks, truth_title_ids, n_truth):
    """duplicate_groups' `links` from what each chunk copied back: (q_first, rows int32[Q, k], ratios uint8[Q, k],
    probabilities float32[Q, k] or None, exact int32[Q], reasons uint8[Q, k]).  One line per exact link (stage 1, ratio
    100, probability NaN) and per slot with a non-zero reason (stage 2 when close, else 3), sorted by row, then the
    exact link first, then by slot.  A link seen from both of its rows appears twice."""
    import pandas as pd
    ids = np.asarray(truth_title_ids, dtype=np.int64)
    parts = {name: [] for name in ("row", "match_row", "levenshtein_ratio", "probability", "stage")}
    for q_first, rows, ratios, probabilities, exact, reasons in chunks:
        count, k = rows.shape
        own = q_first + np.arange(count, dtype=np.int64)
        exact = exact.astype(np.int64)
        linked = np.nonzero((exact >= 0) & (exact < n_truth) & (exact != own))[0]
        query, slot = np.nonzero(reasons)
        order = np.argsort(np.concatenate((linked * (k + 1), query * (k + 1) + slot + 1)), kind="stable")
        slot_probability = np.full(query.shape[0], np.nan, np.float32) if probabilities is None else \
            probabilities[query, slot].astype(np.float32)
        slot_stage = np.where(reasons[query, slot] & REASON_CLOSE, STAGE_CLOSE, STAGE_MODEL).astype(np.int8)
        parts["row"].append(np.concatenate((own[linked], own[query]))[order])
        parts["match_row"].append(np.concatenate((exact[linked], rows[query, slot].astype(np.int64)))[order])
        parts["levenshtein_ratio"].append(
            np.concatenate((np.full(linked.shape[0], 100, np.uint8), ratios[query, slot].astype(np.uint8)))[order])
        parts["probability"].append(
            np.concatenate((np.full(linked.shape[0], np.nan, np.float32), slot_probability))[order])
        parts["stage"].append(np.concatenate((np.full(linked.shape[0], STAGE_EXACT, np.int8), slot_stage))[order])
    empty = {"row": np.int64, "match_row": np.int64, "levenshtein_ratio": np.uint8, "probability": np.float32,
             "stage": np.int8}
    columns = {name: np.concatenate(held) if held else np.zeros(0, empty[name]) for name, held in parts.items()}
    columns["title_id"], columns["match_title_id"] = ids[columns["row"]], ids[columns["match_row"]]
    return pd.DataFrame(columns, columns=list(LINK_COLUMNS))


def validate_assignment(n, top_n, probability_threshold):
    """one_to_one_matches' checks of `n` and its threshold (no library needed) -> (int, float): n as validate_rank, the
    threshold a finite number as validate_duplicates (it is compared as float32)."""
    n = validate_rank(n, top_n)
    return n, validate_duplicates(0, probability_threshold)[1]


def assignment_bytes(n_titles, n, n_truth):
    """The HBM the one-to-one stage holds across a call: key and row of every slot, the key every truth row holds, and
    per title the slot it stands at and its three outputs."""
    return 12 * int(n_titles) * int(n) + 8 * int(n_truth) + 16 * int(n_titles)


def assignment_frame(test_index, match_row, match_slot, first_row, rows, probabilities, ratios, stages, truth_title_ids):
    """one_to_one_matches' `assignment` from the solver's per-title outputs and the [Q, n] slots of the rank stage: one
    line per title in the order of the call.  The scores are those of the matched slot (rank = slot + 1); a title with
    no match has match_row -1, title_id -1, stage 0, probability NaN, ratio 0 and rank 0.  displaced: the title has a
    first choice and did not get it."""
    import pandas as pd
    match_row, match_slot = np.asarray(match_row, dtype=np.int64), np.asarray(match_slot, dtype=np.int64)
    first_row = np.asarray(first_row, dtype=np.int64)
    count = match_row.shape[0]
    found = match_row >= 0
    query, slot = np.nonzero(found)[0], match_slot[found]
    stage = np.zeros(count, dtype=np.int8)
    probability = np.full(count, np.nan, dtype=np.float32)
    ratio = np.zeros(count, dtype=np.uint8)
    if query.shape[0]:
        if not np.array_equal(np.asarray(rows)[query, slot], match_row[found]):
            raise ValueError("match_slot does not hold match_row")
        stage[found] = np.asarray(stages, dtype=np.int8)[query, slot]
        probability[found] = np.asarray(probabilities, dtype=np.float32)[query, slot]
        ratio[found] = np.asarray(ratios, dtype=np.uint8)[query, slot]
    return pd.DataFrame({"test_index": np.asarray(test_index, dtype=np.int64), "match_row": match_row,
                         "title_id": title_ids_of(match_row, truth_title_ids), "stage": stage,
                         "probability": probability, "levenshtein_ratio": ratio,
                         "rank": np.where(found, match_slot + 1, 0).astype(np.int64), "first_choice_row": first_row,
                         "displaced": (first_row >= 0) & (match_row != first_row)}, columns=list(ASSIGNMENT_COLUMNS))


def top_contributions(contributions, n=5):
    """(indices int64[Q, n], values float64[Q, n]): per row of `contributions` [Q, F] its n entries of the largest
    magnitude, the largest first, the lower index first on a tie.  n is cut to F."""
    contributions = np.asarray(contributions, dtype=np.float64)
    if contributions.ndim != 2:
        raise ValueError(f"contributions must be a [Q, F] matrix, not shape {contributions.shape}")
    n = _positive_integer(n, "n")
    order = np.argsort(-np.abs(contributions), axis=1, kind="stable")[:, :min(n, contributions.shape[1])]
    return order.astype(np.int64), np.take_along_axis(contributions, order, axis=1)


def explain_frame(test_index, match_row, probability, margin, bias, stage, answer_row, truth_title_ids,
                  calibrated=None):
    """explain's answer, one line per title in the order of the call.  calibrated: None, or the calibrator's map of
    `probability`, which is the model's own here whatever the stage."""
    import pandas as pd
    match_row = np.asarray(match_row, dtype=np.int64)
    ids = np.asarray(truth_title_ids, dtype=np.int64)
    return _with_calibrated(
        pd.DataFrame({"test_index": np.asarray(test_index, dtype=np.int64), "match_row": match_row,
                      "title_id": ids[match_row] if match_row.shape[0] else np.zeros(0, np.int64),
                      "probability": np.asarray(probability, dtype=np.float32),
                      "margin": np.asarray(margin, dtype=np.float32), "bias": np.asarray(bias, dtype=np.float64),
                      "stage": np.asarray(stage, dtype=np.int8),
                      "answer_row": np.asarray(answer_row, dtype=np.int64)}, columns=list(EXPLAIN_COLUMNS)), calibrated)


def combine_stages(exact_row, close_row, model_row):
    """Per query (match row, stage) from the three stages' rows (-1 = no match), in the reference's priority: a query
    an earlier stage matched never reaches a later one (predict.py:120-121, :183)."""
    exact_row, close_row, model_row = (np.asarray(a, dtype=np.int64) for a in (exact_row, close_row, model_row))
    row = np.where(exact_row >= 0, exact_row, np.where(close_row >= 0, close_row, model_row))
    stage = np.where(exact_row >= 0, STAGE_EXACT,
                     np.where(close_row >= 0, STAGE_CLOSE, np.where(model_row >= 0, STAGE_MODEL, STAGE_NONE)))
    return np.where(row >= 0, row, -1), stage.astype(np.int8)


def finalize_output(test_index, match_row, truth_title_ids):
    """_finalize_output (predict.py:256-272): a DataFrame [title_id, test_index], one row per test index sorted by it,
    title_id = the matched truth row's id or -1."""
    import pandas as pd
    test_index = np.asarray(test_index, dtype=np.int64)
    title_id = title_ids_of(match_row, truth_title_ids)
    order = np.argsort(test_index, kind="stable")
    return pd.DataFrame({"title_id": title_id[order], "test_index": test_index[order]}).reset_index(drop=True)


def _pack(titles):
    """ASCII byte strings -> (uint8 characters, int64 offsets[n + 1])."""
    encoded = [t.encode("ascii") for t in titles]
    offsets = np.zeros(len(encoded) + 1, dtype=np.int64)
    np.cumsum([len(e) for e in encoded], out=offsets[1:])
    chars = np.frombuffer(b"".join(encoded), dtype=np.uint8) if offsets[-1] else np.zeros(1, dtype=np.uint8)
    return np.ascontiguousarray(chars), offsets


def transform_or_keep(titles, transform):
    """The titles as str, put through transform_titles when `transform`."""
    from .text import transform_titles
    titles = [str(t) for t in titles]
    return transform_titles(titles) if transform else titles


def check_characters(chars, offsets, what):
    used = chars[:int(offsets[-1])]
    if used.shape[0] and not _ALLOWED[used].all():
        _refuse_characters(sorted(set(used[~_ALLOWED[used]].tolist())), what)


def _refuse_characters(bad, what):
    bad = bytes(bad).decode("latin-1")
    raise ValueError(f"{what} titles hold characters a transformed title cannot hold: {bad!r}")


def _validate_prepare(prepare_queries):
    if not isinstance(prepare_queries, str) or prepare_queries not in PREPARE_QUERIES:
        raise ValueError(f"prepare_queries must be one of {PREPARE_QUERIES}, not {prepare_queries!r}")


class DeviceTitles:
    """The query table made on the device by `prepare_queries` (ds_prepare_titles): encode_title rows of the
    transformed titles, stride 255, no word counts.  `.handle` / `.n` as a TitleTable."""

    def __init__(self, handle, n, device):
        self.handle, self.n, self.stride, self.device = handle, n, 255, device
        self.prepare_ms = 0.0

    def transformed(self, rows):
        """The transformed titles of the given rows as str, read back from the device (ds_titles_read)."""
        enc = np.empty((self.n, self.stride), dtype=np.uint8)
        lengths = np.empty(self.n, dtype=np.uint8)
        _lib.check(_lib.lib().ds_titles_read(self.handle, _lib.pointer(enc), _lib.pointer(lengths)), "ds_titles_read")
        return [ALLOWED_CHARACTERS_BYTES[enc[r, :lengths[r]]].tobytes().decode("ascii") for r in rows]

    def close(self):
        if self.handle:
            _lib.lib().ds_titles_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def prepare_queries(titles, transform, device=0):
    """The query table of `titles` made on the device: transform_titles (when `transform`) and encode_collection in one
    kernel (ds_prepare_titles), with the host path's checks and errors, in its order: a non-ASCII title without
    `transform` (UnicodeEncodeError), characters a transformed title cannot hold (check_characters' ValueError), a
    title longer than 255 characters without `transform` (DoppelError).  The host keeps the Unicode step (NFD +
    ASCII, transform_titles) for the non-ASCII titles only, and one join.  -> DeviceTitles."""
    titles = [str(t) for t in titles]
    joined = "".join(titles)
    if not joined.isascii():
        if transform:
            titles = [t if t.isascii() else unicodedata.normalize("NFD", t).encode("ascii", "ignore").decode("ascii")
                      for t in titles]
            joined = "".join(titles)
        else:
            for title in titles:          # _pack's error: the first title that is not ASCII
                title.encode("ascii")
    chars = np.frombuffer(joined.encode("ascii"), dtype=np.uint8) if joined else np.zeros(1, dtype=np.uint8)
    offsets = np.zeros(len(titles) + 1, dtype=np.int64)
    np.cumsum(np.fromiter(map(len, titles), dtype=np.int64, count=len(titles)), out=offsets[1:])
    handle = ctypes.c_void_p()
    report = np.zeros(4, dtype=np.int64)
    started = time.perf_counter()
    status = _lib.lib().ds_prepare_titles(_lib.pointer(chars), _lib.pointer(offsets), len(titles), int(bool(transform)),
                                          device, _lib.pointer(None), ctypes.byref(handle), _lib.pointer(report))
    out = DeviceTitles(handle, len(titles), device) if status == 0 else None
    if out is not None:
        out.prepare_ms = (time.perf_counter() - started) * 1000.0      # upload + kernel + synchronise
    mask = int(report[0].view(np.uint64)) | (int(report[1].view(np.uint64)) << 64)
    if mask:
        if out is not None:
            out.close()
        _refuse_characters([b for b in range(128) if (mask >> b) & 1], "query")
    _lib.check(status, "ds_prepare_titles")
    return out


class QuerySpace:
    """The truth vocabulary in HBM for `ds_query_rows_device` (ds_query_space_create): dense column table, idf arrays."""

    def __init__(self, vocabulary_keys, idf32, idf64, device=0):
        keys = np.ascontiguousarray(vocabulary_keys, dtype=np.uint32)
        idf32 = np.ascontiguousarray(idf32, dtype=np.float32)
        idf64 = np.ascontiguousarray(idf64, dtype=np.float64)
        self.device = device
        self.handle = ctypes.c_void_p()
        _lib.check(_lib.lib().ds_query_space_create(_lib.pointer(keys), _lib.pointer(idf32), _lib.pointer(idf64),
                                                    keys.shape[0], device, ctypes.byref(self.handle)),
                   "ds_query_space_create")

    def close(self):
        if self.handle:
            _lib.lib().ds_query_space_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def free_bytes(device):
    """The free HBM of the device now."""
    free, total = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().ds_device_memory(device, ctypes.byref(free), ctypes.byref(total)), "ds_device_memory")
    return int(free.value)


def default_chunk(device, bytes_per_query):
    """Queries per device pass: what a quarter of the device's free HBM holds at `bytes_per_query`."""
    return max(1, free_bytes(device) // 4 // bytes_per_query)


def column_table(vocabulary_keys):
    """int32[2^24]: the column of every tri-gram key of the vocabulary (big-endian bytes), -1 for the others."""
    table = np.full(1 << 24, -1, dtype=np.int32)
    table[np.asarray(vocabulary_keys, dtype=np.int64)] = np.arange(len(vocabulary_keys), dtype=np.int32)
    return table


def query_rows(chars, offsets, vocabulary_keys, idf32, idf64, n_gram=N_GRAM, columns=None):
    """The query side of the native index build (ds_problem_create, 'query rows') against a truth-only vocabulary:
    (q_rowptr, q_cols, q_maxint) as `NativeProblem(truth, queries)` computes them, with the columns renumbered into
    the truth's own vocabulary.  Both number their columns in ascending n-gram order, so a query's truth columns keep
    their order; an n-gram the truth set lacks has an empty posting list (dropped here: it adds nothing to the
    intersection) and the largest truth idf (kept in max_intersection_possible, match_maker.py:149-153,197), which
    is summed in the same ascending n-gram order, in float64.  columns: column_table(vocabulary_keys), when kept."""
    assert n_gram == 3, "vocabulary keys hold tri-grams"
    n = offsets.shape[0] - 1
    lengths = np.diff(offsets)
    counts = np.maximum(lengths - (n_gram - 1), 0)
    owner = np.repeat(np.arange(n, dtype=np.int64), counts)
    start = np.arange(owner.shape[0], dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts) + \
        np.repeat(offsets[:-1], counts)
    padded = np.concatenate((chars[:int(offsets[-1])], np.zeros(n_gram, np.uint8))).astype(np.int64)
    keys = (padded[start] << 16) | (padded[start + 1] << 8) | padded[start + 2]
    unique = np.unique((owner << 24) | keys)            # distinct n-grams per query, ascending
    owner, keys = unique >> 24, unique & 0xffffff
    column = (column_table(vocabulary_keys) if columns is None else columns)[keys]
    known = column >= 0
    column = np.where(known, column, 0)
    max_idf = float(np.max(idf64)) if idf64.shape[0] else 0.0
    value = np.where(known, np.asarray(idf64)[column], max_idf)
    nonzero = np.where(known, np.asarray(idf32)[column] != 0, np.float32(max_idf) != 0)   # explicit zeros vanish (:118)
    listed = known & nonzero
    q_cols = column[listed].astype(np.int32)
    q_rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(owner[listed], minlength=n), out=q_rowptr[1:])
    # float64 sums in ascending n-gram order: a [n, width] matrix padded with zeros at the end of each row
    owner, value = owner[nonzero], value[nonzero]
    per_query = np.bincount(owner, minlength=n)
    rank = np.arange(owner.shape[0]) - np.repeat(np.cumsum(per_query) - per_query, per_query)
    matrix = np.zeros((n, int(per_query.max()) if n and owner.shape[0] else 0), dtype=np.float64, order="F")
    matrix[owner, rank] = value
    q_maxint = np.zeros(n, dtype=np.float64)
    for j in range(matrix.shape[1]):
        q_maxint = q_maxint + matrix[:, j]
    return q_rowptr, q_cols, q_maxint


class TruthSide:
    """The device-resident truth side of a set of transformed titles: the vocabulary of the native index build, the
    Jaccard index (TruthIndex), the encoded titles with their word counts (TitleTable), and what `query_rows` needs to
    number a query's n-grams in that vocabulary.  build_index: "host" or "device", where the Jaccard index is built
    (TruthIndex); `index_build_ms` is the wall clock of that call."""

    def __init__(self, transformed_titles, device=0, build_index="host"):
        validate_index_build(build_index, "build_index")
        chars, offsets = _pack(transformed_titles)
        check_characters(chars, offsets, "truth")
        problem = NativeProblem.from_flat(chars, offsets, np.zeros(1, np.uint8), np.zeros(1, np.int64), N_GRAM)
        arrays = problem.arrays()
        self.vocabulary_keys, self.idf32, self.idf64 = arrays["vocabulary_keys"], arrays["idf32"], arrays["idf64"]
        self.columns = column_table(self.vocabulary_keys)
        started = time.perf_counter()
        self.index = TruthIndex(arrays["rowptr"], arrays["truth_idx"], arrays["idf32"], arrays["sums32"], device,
                                build=build_index)
        self.index_build_ms = (time.perf_counter() - started) * 1000.0    # the create call: it ends synchronised
        problem.close()
        enc, lengths = encode_collection(chars, offsets, _CODE_OF)
        counts = truth_word_counts(chars, offsets, separators=(ord(" "),))
        self.table = TitleTable(enc, lengths, counts, device)
        self.space = QuerySpace(self.vocabulary_keys, self.idf32, self.idf64, device)

    def query_rows(self, chars, offsets):
        return query_rows(chars, offsets, self.vocabulary_keys, self.idf32, self.idf64, columns=self.columns)


class StageClock:
    """The milliseconds of a call's stages, added to `timings` by name: a device stage between the two events of a
    _lib.Timer of its own (made when the stage first runs: one that never runs keeps its 0.0), a host stage by the wall
    clock."""

    def __init__(self, timings, device=0):
        self.timings, self._device, self._timers, self._pending = timings, device, {}, []

    def device(self, name, enqueue):
        """Runs enqueue() between the events of stage `name` on the null stream; `collect` reads the time."""
        if name not in self._timers:
            self._timers[name] = _lib.Timer(self._device)
        self._timers[name].start()
        enqueue()
        self._timers[name].stop()
        self._pending.append(name)

    def collect(self):
        """Adds the time of every stage run since the last collect, in their order (each read waits for the stage)."""
        pending, self._pending = self._pending, []
        for name in pending:
            self.timings[name] += self._timers[name].elapsed_ms()

    @contextlib.contextmanager
    def host(self, name):
        started = time.perf_counter()
        yield
        self.timings[name] += (time.perf_counter() - started) * 1000.0


class Prediction:
    """Prediction(truth_titles, truth_title_ids, model).generate_test_predictions(titles) -> the reference's
    final_output: a DataFrame [title_id, test_index] sorted by test_index, -1 where no stage found a match.

    truth_titles / titles: raw strings, put through transform_titles unless transform=False (then they must already
    be transformed titles: lower-case letters, digits and single spaces).  model: a ForestModel (the booster of
    predict.py:80-82).  chunk_queries: queries per device pass (default: what a quarter of the free HBM holds); the
    answer does not depend on it.  After a call, `details` holds per query match_row, title_id, stage (0 none,
    1 exact, 2 close, 3 model) and probability (1.0 for exact and close matches, the model's best candidate
    otherwise, NaN when the query never reached the model), and `timings` the milliseconds of every stage.
    prepare_queries: "device" (default) transforms and encodes the query titles and derives their Jaccard rows on the
    device (`prepare_queries`, CandidatePipeline.load_queries_device); "host" does it on the host (transform_titles,
    query_rows, encode_collection).  Both give the same answers, details and errors.
    build_index: "host" (default) or "device": where the truth index is built (TruthIndex); the index is the same.
    calibrator: None, or a calibration.Calibrator of the model's probability (ForestModel.calibrate, fit_isotonic):
    ranked_matches, exhaustive_matches and explain then carry one more column, `calibrated_probability`, directly after
    `probability`: the calibrator's map of it, computed on the device from the chunk's probability buffer (stage
    "calibrate" of `timings`), 1.0 for an exact or close slot.  Order, answers and thresholds are unchanged; to decide
    at a calibrated level q pass probability_threshold=calibrator.raw_threshold(q)."""

    def __init__(self, truth_titles, truth_title_ids, model, top_n=100, device=0, transform=True,
                 levenshtein_threshold=LEVENSHTEIN_RATIO_THRESHOLD,
                 probability_threshold=PREDICTION_PROBABILITY_THRESHOLD, chunk_queries=None, prepare_queries="device",
                 build_index="host", calibrator=None):
        truth_titles = list(truth_titles)
        self.truth_title_ids = validate_truth(truth_titles, truth_title_ids, top_n)
        _validate_chunk(chunk_queries)
        _validate_prepare(prepare_queries)
        validate_index_build(build_index, "build_index")
        if model is None or not hasattr(model, "predict_device"):
            raise ValueError("model must be a ForestModel")
        if calibrator is not None and not hasattr(calibrator, "transform_device"):
            raise ValueError("calibrator must be a Calibrator")
        self.calibrator = calibrator
        self.model = model
        self.top_n = int(top_n)
        self.device = device
        self.transform = transform
        self.levenshtein_threshold = int(levenshtein_threshold)
        self.probability_threshold = float(probability_threshold)
        self.chunk_queries = chunk_queries
        self.prepare_queries = prepare_queries
        self.details = None
        self.candidates = None
        self.link_counts = None
        self.links = None
        self.contributions = None
        self.explained_features = None
        self.assignment = None
        self.assignment_counts = None
        self.sweep_bootstrap = None
        self.timings = {}

        self.truth_titles = transform_or_keep(truth_titles, transform)
        self._truth = TruthSide(self.truth_titles, device, build_index=build_index)
        self.index, self.truth_table = self._truth.index, self._truth.table
        self.index_build_ms = self._truth.index_build_ms

    def _default_chunk(self, device_rows=False, rank_slots=0, parts=False, explain=False):
        # device_rows: the pipeline's own query CSR at capacity (rowptr, 253 columns, q_maxint per query)
        # rank_slots: the slots per query of the rank stage's output; parts: the close ratio taken apart, per pair
        # explain: the best pair of a query, its gathered features and its contributions
        return default_chunk(self.device, (BYTES_PER_PAIR + BYTES_PER_PARTS * parts) * self.top_n + 64 +
                             (8 + 4 * MAX_GRAMS + 8) * device_rows + BYTES_PER_RANK * rank_slots +
                             BYTES_PER_EXPLAIN * explain)

    def _stage_names(self, *names):
        """The zeroed timings of a call's stages; with a calibrator, "calibrate" among them."""
        return dict.fromkeys(names + (("calibrate",) if self.calibrator is not None else ()), 0.0)

    def _enqueue_calibrated(self, clock, d_probabilities, count):
        """Stage "calibrate": the calibrator's map of `count` probabilities where a stage left them in HBM, into a
        buffer of its own -> that buffer (the caller copies it back and frees it); None without a calibrator."""
        if self.calibrator is None:
            return None
        d_out = _lib.DeviceArray((max(1, count),), np.float32, self.device)
        clock.device("calibrate", lambda: self.calibrator.transform_device(d_probabilities, count, d_out, None,
                                                                           self.device))
        return d_out

    def generate_test_predictions(self, titles, test_index=None):
        """One answer per title (predict.py:274-300): DataFrame [title_id, test_index] sorted by test_index."""
        titles = list(titles)
        test_index = validate_queries(titles, test_index)
        self.details = self._run(titles, test_index)
        return finalize_output(test_index, self.details["match_row"].to_numpy(), self.truth_title_ids)

    def closest_search_single_title(self, title, exhaustive=False):
        """cli.py:64-84 (generate_test_predictions(single_prediction=True)): the best match of one title as a dict
        with the keys of predict.py:35-41.  Stage priority exact, close, model; the model stage takes the candidate with
        the highest probability, no threshold, the first in top-n order on a tie (predict.py:239-242).
        exhaustive: the model stage takes the best row of the WHOLE truth set instead (what the reference's README
        describes: `exhaustive_matches` with n = 1, the lowest row on a tie); exact and close matches keep their
        priority."""
        stripped = str(title).strip()
        if not stripped:
            raise ValueError("empty title")
        details = self._run([stripped], np.zeros(1, dtype=np.int64), single=True)
        if exhaustive and int(details["stage"].iloc[0]) not in (STAGE_EXACT, STAGE_CLOSE):
            timings = dict(self.timings)
            best = self.exhaustive_matches([stripped], n=1)
            timings["exhaustive"] = self.timings["exhaustive"]
            self.timings = timings
            details.loc[0, ["match_row", "title_id"]] = int(best["match_row"].iloc[0]), int(best["title_id"].iloc[0])
            details["stage"] = np.int8(STAGE_MODEL)
            details["probability"] = np.float32(best["probability"].iloc[0])
        self.details = details
        row = int(details["match_row"].iloc[0])
        queries = self._last_queries
        transformed = queries.transformed([0])[0] if isinstance(queries, DeviceTitles) else queries[0]
        return {"test_index": 0, "transformed_title": transformed,
                "match_transformed_title": self.truth_titles[row] if row >= 0 else None,
                "title_id": int(self.truth_title_ids[row]) if row >= 0 else TRAIN_NOT_FOUND_VALUE,
                "prediction": float(details["probability"].iloc[0])}

    def ranked_matches(self, titles, n=5, test_index=None, keep_candidates=False):
        """The best `n` candidates of every title, in order, with their scores: a DataFrame in long form [test_index,
        rank (from 1), title_id, match_row, probability, levenshtein_ratio, stage] sorted by test_index, then rank, one
        line per filled slot (a title with fewer than n candidates has fewer lines).

        The exact match of a title, else its close match, comes first with probability 1.0 (rank 1 is then the answer
        of generate_test_predictions); the other candidates of the Jaccard top_n follow at stage 3, by the model's
        probability descending, the earlier candidate first on a tie.  Every candidate is scored, also those of a
        title an earlier stage matched; the order is made on the device (CandidatePipeline.enqueue_rank_matches) and n
        entries per title come back.  keep_candidates: `candidates` then holds the call's intermediates (Candidates:
        rows int32[Q, top_n], ratios uint8[Q, top_n], probabilities float32[Q, top_n], exact int32[Q], close
        int32[Q]) in the order of `titles`, to re-rank by another rule; else it is None.  `details` is left alone."""
        n = validate_rank(n, self.top_n)
        titles = list(titles)
        test_index = validate_queries(titles, test_index)
        timings = self._stage_names("host_prepare", "top_k", "close_matches", "exact_matches", "features", "model",
                                    "rank", "copy_back")
        count, k = len(titles), self.top_n
        kept = Candidates(np.empty((count, k), np.int32), np.empty((count, k), np.uint8), np.empty((count, k), np.float32),
                          np.empty(count, np.int32), np.empty(count, np.int32)) if keep_candidates else None
        calibrated = None if self.calibrator is None else np.full((count, n), np.nan, dtype=np.float32)
        slots, _ = self._rank(titles, timings, n, kept, calibrated=calibrated)
        self.timings = timings
        self.candidates = kept
        return ranked_frame(test_index, *slots, self.truth_title_ids, calibrated=calibrated)

    def one_to_one_matches(self, titles, n=5, test_index=None, probability_threshold=None):
        """One answer per title, each truth title given to one title at most: the frame of generate_test_predictions,
        DataFrame [title_id, test_index] sorted by test_index, -1 where a title got nothing, and no title_id other than
        -1 twice.  For linking one de-duplicated file against another.

        Every title has the `n` ranked slots of ranked_matches(titles, n).  A slot is an edge when it is the exact or the
        close match, or a model candidate with a probability above `probability_threshold` (None: this instance's own;
        float32 compare).  A truth row keeps the best claim on it: exact over close over model, then the higher ratio or
        probability, then the earlier title of `titles`.  A title that loses a row goes on to its next edge, where it may
        displace somebody else in turn: deferred acceptance with the titles proposing, run on the device to its fixed
        point (CandidatePipeline.enqueue_assign_edges per chunk, ds_assign_solve_device once).  The result is the
        title-optimal stable matching; since a title's slots descend in score it is also what taking all edges in
        descending order of score, each when its title and its row are still free, would give.  It does not depend on
        chunk_queries or on the schedule; it does depend on the ORDER of `titles`, on equal scores.

        Where it differs from generate_test_predictions even when no two titles want the same row: the reference
        answers "none" when several candidates hold the maximum (the close stage, predict.py:158-161, and the model
        stage, predict.py:244-249); here the ranked slots break such a tie by the earlier candidate, so a title whose best
        model candidates tie above the threshold is matched.  A close tie has no head and its candidates stand as model
        candidates, under the probability threshold.

        After a call `assignment` holds, per title in the order of `titles`, [test_index, match_row, title_id, stage,
        probability, levenshtein_ratio, rank, first_choice_row, displaced]: the scores of the matched slot (rank = slot
        + 1, 0 for none; a matched exact or close head has probability 1.0), the row of the title's first edge (-1: it
        has none) and whether it got another answer than that.  `assignment_counts` holds edges, matched, displaced,
        displaced_unmatched (pure functions of the input) and proposals, rounds (diagnostics of the schedule).
        `details`, `candidates`, `links` and `contributions` are left alone."""
        n, threshold = validate_assignment(
            n, self.top_n, self.probability_threshold if probability_threshold is None else probability_threshold)
        titles = list(titles)
        test_index = validate_queries(titles, test_index)
        timings = dict.fromkeys(("host_prepare", "top_k", "close_matches", "exact_matches", "features", "model", "rank",
                                 "assign_edges", "assign", "copy_back"), 0.0)
        count, n_truth = len(titles), len(self.truth_titles)
        outputs = tuple(np.full(count, -1, dtype=np.int32) for _ in range(3))
        counts = np.zeros(len(ASSIGNMENT_COUNTS), dtype=np.int64)
        if count:
            needed, free = assignment_bytes(count, n, n_truth), free_bytes(self.device)
            if needed + ASSIGN_RESERVE_BYTES > free:
                raise _lib.DoppelError(f"one_to_one_matches: {count} titles of {n} slots against {n_truth} truth titles "
                                       f"need {needed} bytes of HBM, {free} are free")
            make = lambda shape, dtype: _lib.DeviceArray(shape, dtype, self.device)
            keys, rows = make((count, n), np.uint64), make((count, n), np.int32)
            held, standing = make((max(n_truth, 1),), np.uint64), make((count,), np.int32)
            device_outputs = tuple(make((count,), np.int32) for _ in range(3))
            device_counts = make((len(ASSIGNMENT_COUNTS),), np.int64)

        def edges(pipeline, clock):
            # 8. the keys of this chunk's slots into the call-wide arrays (the ranked buffers still hold the chunk)
            clock.device("assign_edges", lambda: pipeline.enqueue_assign_edges(keys, rows, threshold))
            clock.collect()

        slots, clock = self._rank(titles, timings, n, tail=edges)
        if count:
            clock.device("assign", lambda: _lib.check(_lib.lib().ds_assign_solve_device(
                rows.ptr, keys.ptr, count, n, n_truth, held.ptr, standing.ptr, *(a.ptr for a in device_outputs),
                device_counts.ptr, _lib.pointer(None)), "ds_assign_solve_device"))
            with clock.host("copy_back"):
                outputs, counts = tuple(a.to_host() for a in device_outputs), device_counts.to_host()
            clock.collect()
        self.timings = timings
        self.assignment = assignment_frame(test_index, *outputs, *slots, self.truth_title_ids)
        self.assignment_counts = dict(zip(ASSIGNMENT_COUNTS, (int(c) for c in counts)))
        return finalize_output(test_index, outputs[0], self.truth_title_ids)

    def exhaustive_matches(self, titles, n=5, test_index=None):
        """The best `n` rows of the WHOLE truth set for every title by the model alone, next to where the candidate
        stage put them: a DataFrame in long form [test_index, rank (from 1), title_id, match_row, probability
        (float32), jaccard_position (int32)] sorted by test_index, then rank.

        Every (title, truth title) pair is scored: features and forest on the device, a tile of pairs at a time, folded
        into n rows per title by the probability's float32 bits descending, the lower row first on a tie
        (CandidatePipeline.enqueue_exhaustive).  There is no exact or close override here.  jaccard_position is the
        column of match_row among the title's Jaccard top_n rows, -1 when the candidate stage did not produce it: a
        rank-1 row at -1 is a miss of the candidate stage, not of the model.  n: up to 64 and up to the truth titles.
        `details` and `candidates` are left alone."""
        n = validate_exhaustive(n, len(self.truth_titles))
        titles = list(titles)
        test_index = validate_queries(titles, test_index)
        timings = self._stage_names("host_prepare", "top_k", "exhaustive", "copy_back")
        count = len(titles)
        rows = np.full((count, n), -1, dtype=np.int32)
        probabilities = np.full((count, n), np.nan, dtype=np.float32)
        calibrated = None if self.calibrator is None else np.full((count, n), np.nan, dtype=np.float32)
        top_rows = np.full((count, self.top_n), -1, dtype=np.int32)
        for pipeline, clock in self._chunks(titles, timings):
            first, last = pipeline.q_first, pipeline.q_first + pipeline.n_queries
            self._top_k(pipeline, clock)
            clock.device("exhaustive", lambda: pipeline.enqueue_exhaustive(self.model, n))
            d_calibrated = self._enqueue_calibrated(clock, pipeline.exhaustive_probabilities_device(),
                                                    pipeline.n_queries * n)
            with clock.host("copy_back"):
                rows[first:last], probabilities[first:last] = pipeline.exhaustive(n)
                top_rows[first:last] = pipeline.rows()
                if d_calibrated is not None:
                    calibrated[first:last] = d_calibrated.to_host(pipeline.n_queries * n).reshape(-1, n)
                    d_calibrated.free()
            clock.collect()
        self.timings = timings
        return exhaustive_frame(test_index, rows, probabilities, top_rows, self.truth_title_ids, calibrated=calibrated)

    def explain(self, titles, test_index=None, approximate=False):
        """For every title the model's best candidate and why the model scored it so: a DataFrame [test_index,
        match_row, title_id, probability (float32), margin (float32), bias (float64), stage, answer_row], one line per
        title in the order of `titles`.

        The best candidate is the pair of the title's Jaccard top_n with the highest probability, the first in top-n
        order on a tie (predict.py:239-242); it is explained whether or not an earlier stage matched the title and
        whether or not it clears the probability threshold.  stage and answer_row are what generate_test_predictions
        answers for the title (answer_row -1: none), so a reader sees whether the explained pair is the answer.
        After a call `contributions` holds float64[Q, 66]: the share of each feature in the pair's margin (margin =
        bias + the sum of a line, up to the float32 rounding of the margin; FEATURE_NAMES names the columns,
        top_contributions picks the largest), and `explained_features` float32[Q, 66] the feature values themselves,
        both in the order of `titles`.  approximate: Saabas' method in place of TreeSHAP
        (ForestModel.predict_contributions).  Every stage runs on the device (CandidatePipeline.enqueue_explain);
        per title one pair's numbers come back.  The model needs a cover (ForestModel.fit_cover / set_cover,
        train_model(cover=True)): ValueError otherwise, before any device work.  `details` and `candidates` are left
        alone."""
        if getattr(self.model, "cover", None) is None:
            raise ValueError("the model has no cover: ForestModel.fit_cover, set_cover or train_model(cover=True) first")
        titles = list(titles)
        test_index = validate_queries(titles, test_index)
        timings = self._stage_names("host_prepare", "top_k", "close_matches", "exact_matches", "features", "model",
                                    "contributions", "copy_back")
        count, width = len(titles), self.model.n_features
        calibrated = None if self.calibrator is None else np.full(count, np.nan, dtype=np.float32)
        match_row, answer_row = np.full(count, -1, dtype=np.int64), np.full(count, -1, dtype=np.int64)
        probability, margin = np.full(count, np.nan, dtype=np.float32), np.full(count, np.nan, dtype=np.float32)
        stage = np.zeros(count, dtype=np.int8)
        features = np.empty((count, width), dtype=np.float32)
        contributions = np.empty((count, width + 1), dtype=np.float64)
        for pipeline, clock in self._chunks(titles, timings, explain=True):
            first, last = pipeline.q_first, pipeline.q_first + pipeline.n_queries
            # 1.-5. every pair scored, 6. the best pair per query, its features gathered, its margin and its contributions
            self._score_chunk(pipeline, clock, self.levenshtein_threshold)
            clock.device("contributions", lambda: pipeline.enqueue_explain(self.model, approximate))
            d_calibrated = self._enqueue_calibrated(clock, pipeline.explained_probabilities_device(), pipeline.n_queries)
            # 7. one copy back of one pair per query (synchronises the null stream the stages ran on)
            with clock.host("copy_back"):
                rows, best, held, margins, features[first:last], contributions[first:last] = pipeline.explained()
                exact, close = pipeline.exact_matches(), pipeline.best_rows()
                if d_calibrated is not None:
                    calibrated[first:last] = d_calibrated.to_host(pipeline.n_queries)
                    d_calibrated.free()
            clock.collect()
            # the answer of generate_test_predictions: the model matches only with a single best pair above the threshold
            model_row = np.where((best > np.float32(self.probability_threshold)) & (held == 1), rows, -1)
            answer_row[first:last], stage[first:last] = combine_stages(exact, np.where(exact >= 0, -1, close), model_row)
            match_row[first:last], probability[first:last], margin[first:last] = rows, best, margins
        self.timings = timings
        self.contributions = np.ascontiguousarray(contributions[:, :width])
        self.explained_features = features
        return explain_frame(test_index, match_row, probability, margin, contributions[:, width], stage, answer_row,
                             self.truth_title_ids, calibrated=calibrated)

    def threshold_sweep(self, titles, actual_title_ids, levenshtein_thresholds=None, probability_thresholds=None,
                        test_index=None, *, n_boot=0, groups=None, seed=0):
        """How the answers of generate_test_predictions(titles) would compare with `actual_title_ids` at every pair of
        (levenshtein_threshold, probability_threshold): a DataFrame in long form [levenshtein_threshold,
        probability_threshold, correctly_matched, incorrectly_matched, correctly_not_found, incorrectly_not_found,
        custom_error], one line per cell, sorted by the first two columns (get-predictions-accuracy, cli.py:107-128,
        for each cell).

        actual_title_ids: per title the id it should get, -1 for a title with no match.  The thresholds (None: this
        instance's own value) are sorted and de-duplicated: up to 101 integers in [0, 100] and up to 256 numbers,
        compared as float32 like probability_threshold.  Every pair is scored once, whatever the grid: top-k, the close
        ratio taken apart (CandidatePipeline.enqueue_close_parts), the exact stage, features and forest on all pairs;
        then one kernel replays the decision rule for every cell and counts (enqueue_threshold_sweep).  The counters
        stay on the device between the chunks and come back once.  `details` and `candidates` are left alone.

        n_boot > 0 adds the paired bootstrap of every cell (bootstrap.SweepBootstrap in `sweep_bootstrap`, None
        otherwise; the returned frame is the same): is the best cell really better than the next one, or than the
        defaults?  Next to the counters every chunk writes one 16-bit record per (title, Levenshtein threshold)
        (enqueue_sweep_records, stage "sweep_records") into one buffer of n x T x 2 bytes in HBM, and after the last
        chunk one call resamples the titles n_boot times for all cells at once (ds_sweep_bootstrap_device, stage
        "sweep_bootstrap").  groups: one value per title; titles that share one are drawn together (None: every title
        on its own).  seed: the draws are a closed-form function of it.  bootstrap.validate_sweep_bootstrap says what
        is accepted."""
        from . import bootstrap
        titles = list(titles)
        validate_queries(titles, test_index)
        lev, prob, shown, actual_row = validate_sweep(
            [self.levenshtein_threshold] if levenshtein_thresholds is None else levenshtein_thresholds,
            [self.probability_threshold] if probability_thresholds is None else probability_thresholds,
            actual_title_ids, self.truth_title_ids, len(titles))
        boot = bootstrap.validate_sweep_bootstrap(n_boot, seed, groups, len(titles), lev.shape[0], prob.shape[0])
        self.sweep_bootstrap = None
        timings = dict.fromkeys(("host_prepare", "top_k", "close_parts", "exact_matches", "features", "model", "sweep",
                                 "copy_back"), 0.0)
        if boot["n_boot"]:
            timings.update(sweep_records=0.0, sweep_bootstrap=0.0)
        counts = np.zeros(lev.shape[0] * prob.shape[0] * 4, dtype=np.int64)
        grid = records = None
        for pipeline, clock in self._chunks(titles, timings, parts=True):
            if grid is None:
                grid = (_lib.DeviceArray.from_host(lev, self.device), _lib.DeviceArray.from_host(prob, self.device),
                        _lib.DeviceArray.from_host(counts, self.device))
            actual = _lib.DeviceArray.from_host(actual_row[pipeline.q_first:pipeline.q_first + pipeline.n_queries],
                                                self.device)
            # 1.-5. every pair scored with the close ratio taken apart, 6. the rule replayed per cell (the sweep entry
            # synchronises once, to check the grid's values)
            self._score_chunk(pipeline, clock, parts=(int(lev[0]), int(lev[-1])))
            clock.device("sweep", lambda: pipeline.enqueue_threshold_sweep(actual, *grid))
            if boot["n_boot"]:
                if records is None:
                    records = _lib.DeviceArray((len(titles), lev.shape[0]), np.uint16, self.device)
                here = ctypes.c_void_p(records.ptr.value + pipeline.q_first * lev.shape[0] * 2)
                clock.device("sweep_records", lambda: pipeline.enqueue_sweep_records(actual, grid[0], grid[1], here))
            clock.collect()
        if boot["n_boot"]:
            # one call for all cells; it returns with its counts read back, so the wall clock holds the stage
            started = time.perf_counter()
            self.sweep_bootstrap = bootstrap.sweep_bootstrap_device(
                records, len(titles), lev, shown, boot["unit"], boot["n_units"], boot["n_boot"], boot["seed"], self.device,
                (self.levenshtein_threshold, self.probability_threshold))
            timings["sweep_bootstrap"] = (time.perf_counter() - started) * 1000.0
            if records is not None:
                records.free()
        if grid is not None:
            with clock.host("copy_back"):
                counts = grid[2].to_host()            # synchronises the null stream the stages ran on
        self.timings = timings
        return sweep_frame(lev, shown, counts)

    def evaluate(self, titles, actual_title_ids, test_index=None, *, n_boot=0, groups=None, seed=0):
        """The accuracy of generate_test_predictions(titles) against `actual_title_ids` at this instance's thresholds,
        as `predictions_accuracy` reports it: the one cell of `threshold_sweep`.  n_boot, groups and seed are passed on:
        with n_boot > 0 `sweep_bootstrap` holds that cell's bootstrap (its interval(level) is the error's interval)."""
        line = self.threshold_sweep(titles, actual_title_ids, test_index=test_index, n_boot=n_boot, groups=groups,
                                    seed=seed).iloc[0]
        return {name: int(line[name]) for name in ACCURACY_KEYS}

    def duplicate_groups(self, levenshtein_threshold=None, probability_threshold=None, model_links=True,
                         return_links=False):
        """The groups of truth titles that are duplicates of each other: a DataFrame [group_id, group_size, title_id,
        row], one line per truth row whose group holds two rows at least, sorted by the group's lowest row, then by row;
        group_id is the title_id of that lowest row.

        Every truth title is scored against its own Jaccard top_n as a query would be (the row itself normally takes
        one of the top_n slots, so a row sees top_n - 1 others).  Two rows are linked when they hold the same transformed
        title (the exact stage), when their fuzzy ratio is above levenshtein_threshold (the close stage) or, with
        model_links, when the model's probability for the pair is above probability_threshold; a threshold of None is
        this instance's own.  The groups are the connected components of the links: a row belongs to the group of any
        row it is linked to, directly or through others.  They are found on the device by a union-find that lives across
        the chunks (CandidatePipeline.enqueue_duplicate_links); labels, sizes and counters come back once.  With
        model_links=False neither features nor forest run.

        After a call `link_counts` holds the exact links, the slots that are close and the slots only the model links
        ({"exact", "close", "model"}; a link seen from both of its rows counts twice), and `links` is None or, with
        return_links, a DataFrame [row, match_row, title_id, match_title_id, levenshtein_ratio, probability, stage]:
        one line per exact link (stage 1, ratio 100, probability NaN) and per linking slot (stage 2 when close, else 3),
        sorted by row, the exact link first, then by slot; nothing is merged.  `details` and `candidates` are left
        alone.  The errors are those of generate_test_predictions(truth_titles)."""
        lev, prob = validate_duplicates(self.levenshtein_threshold if levenshtein_threshold is None else levenshtein_threshold,
                                        self.probability_threshold if probability_threshold is None else probability_threshold)
        timings = dict.fromkeys(("host_prepare", "prepare_queries", "top_k", "close_matches", "exact_matches", "features",
                                 "model", "links", "finish", "copy_back"), 0.0)
        n = len(self.truth_titles)
        parent, kept = None, []
        for pipeline, clock in self._chunks(None, timings, table=self.truth_table):      # the truth rows are the queries
            if parent is None:
                with clock.host("host_prepare"):
                    make = lambda shape, dtype: _lib.DeviceArray(shape, dtype, self.device)
                    parent, counts, labels, sizes = (make((n,), np.int32), make((3,), np.int64), make((n,), np.int32),
                                                     make((n,), np.int32))
                    _lib.check(_lib.lib().ds_duplicate_begin_device(parent.ptr, n, counts.ptr, _lib.pointer(None)),
                               "ds_duplicate_begin_device")
            # 1.-5. every pair scored (close and exact only without model_links), 6. the links
            self._score_chunk(pipeline, clock, lev, score_all=model_links)
            clock.device("links", lambda: pipeline.enqueue_duplicate_links(parent, counts, lev, prob, model_links,
                                                                           reasons=return_links))
            clock.collect()
            if return_links:
                with clock.host("copy_back"):
                    kept.append((pipeline.q_first, pipeline.rows(), pipeline.close_matches()[0],
                                 pipeline.predictions() if model_links else None, pipeline.exact_matches(),
                                 pipeline.duplicate_reasons()))
        clock.device("finish", lambda: _lib.check(_lib.lib().ds_duplicate_finish_device(
            parent.ptr, n, labels.ptr, sizes.ptr, _lib.pointer(None)), "ds_duplicate_finish_device"))
        clock.collect()
        with clock.host("copy_back"):
            host_labels, host_sizes, host_counts = labels.to_host(), sizes.to_host(), counts.to_host()
        self.timings = timings
        self.link_counts = dict(zip(("exact", "close", "model"), (int(c) for c in host_counts)))
        self.links = links_frame(kept, self.truth_title_ids, n) if return_links else None
        return duplicate_frame(host_labels, host_sizes, self.truth_title_ids)

    def _run(self, titles, test_index, single=False):
        import pandas as pd
        timings = dict.fromkeys(("host_prepare", "top_k", "close_matches", "exact_matches", "remaining_pairs",
                                 "features", "model", "select_matches", "copy_back"), 0.0)
        n = len(titles)
        match_row = np.full(n, -1, dtype=np.int64)
        stage = np.zeros(n, dtype=np.int8)
        probability = np.full(n, np.nan, dtype=np.float32)
        for pipeline, clock in self._chunks(titles, timings):
            self._chunk(pipeline, clock, match_row, stage, probability, single)
        self.timings = timings
        return pd.DataFrame({"test_index": test_index, "match_row": match_row,
                             "title_id": title_ids_of(match_row, self.truth_title_ids), "stage": stage,
                             "probability": probability})

    def _chunks(self, titles, timings, rank_slots=0, parts=False, explain=False, table=None):
        """The one loop over the queries: prepares the titles (on the device or on the host), then yields (pipeline,
        clock) with each chunk loaded in turn, clock being the call's StageClock on `timings`.  Fills timings'
        host_prepare and prepare_queries (a chunk's query rows stay pending on the clock, so the host goes on to enqueue
        top-k while they are derived: `_top_k` reads them); yields nothing for no titles.
        table: a query table made already (then `titles` is not looked at): its rows are derived on the device whatever
        `prepare_queries` says."""
        device_path = table is not None or self.prepare_queries == "device"
        if device_path:
            timings["prepare_queries"] = 0.0
        started = time.perf_counter()
        n = len(titles) if table is None else table.n
        if table is None and device_path:
            self._last_queries = table = prepare_queries(titles, self.transform, self.device) if n else None
            if n:
                timings["prepare_queries"] = table.prepare_ms
        elif table is None:
            self._last_queries = queries = transform_or_keep(titles, self.transform)
        if n == 0:
            return
        if not device_path:
            chars, offsets = _pack(queries)
            check_characters(chars, offsets, "query")
            q_rowptr, q_cols, q_maxint = self._truth.query_rows(chars, offsets)
            enc, lengths = encode_collection(chars, offsets, _CODE_OF)
            table = TitleTable(enc, lengths, None, self.device)
        chunk = min(n, self.chunk_queries or self._default_chunk(device_path, rank_slots, parts, explain))
        pipeline = CandidatePipeline.over(self.index, self.truth_table, table, self.top_n, chunk, self.device)
        timings["host_prepare"] = (time.perf_counter() - started) * 1000.0 - timings.get("prepare_queries", 0.0)
        clock = StageClock(timings, self.device)
        for first in range(0, n, chunk):
            last = min(n, first + chunk)
            if device_path:
                clock.device("prepare_queries", lambda: pipeline.load_queries_device(self._truth.space, first, last))
            else:
                pipeline.load_queries(q_rowptr, q_cols, q_maxint, first, last)
            yield pipeline, clock

    def _top_k(self, pipeline, clock):
        """Jaccard top-k, synchronised (ds_jaccard_sync reports errors and settles the queries it resolves late); its
        time and that of the chunk's query rows are read once it is through."""
        clock.device("top_k", pipeline.enqueue_top_k)
        pipeline.sync()
        clock.collect()

    def _score_chunk(self, pipeline, clock, levenshtein_threshold=None, parts=None, score_all=True):
        """The stages every scoring call starts a chunk with: 1. Jaccard top-k (synchronised), 2. close matches at the
        threshold (or, with parts = (t_min, t_max), the close ratio taken apart), 3. the exact stage overrides their
        best row and, with score_all, 4. features and 5. the forest on ALL pairs.  All but top-k stay pending on the
        clock."""
        self._top_k(pipeline, clock)
        if parts is None:
            clock.device("close_matches", lambda: pipeline.enqueue_close_matches(threshold=levenshtein_threshold))
        else:
            clock.device("close_parts", lambda: pipeline.enqueue_close_parts(*parts))
        clock.device("exact_matches", pipeline.enqueue_exact_matches)
        if score_all:
            clock.device("features", pipeline.enqueue_features)
            clock.device("model", lambda: pipeline.enqueue_predict(self.model))

    def _rank(self, titles, timings, n, kept=None, tail=None, calibrated=None):
        """The device work of ranked_matches, which one_to_one_matches shares: per chunk every pair scored, 6. the best n
        per query in order, 7. one copy back into the [Q, n] slots (and into `kept`), then tail(pipeline, clock) while
        the ranked buffers still hold the chunk.  calibrated: None, or float32[Q, n] for the calibrator's map of the
        ranked probabilities, made on the device.  -> (slots, the call's clock: None without titles)."""
        slots, clock = _rank_slots(len(titles), n), None
        for pipeline, clock in self._chunks(titles, timings, rank_slots=n):
            first, last = pipeline.q_first, pipeline.q_first + pipeline.n_queries
            self._score_chunk(pipeline, clock, self.levenshtein_threshold)
            clock.device("rank", lambda: pipeline.enqueue_rank_matches(n))
            d_calibrated = None if calibrated is None else \
                self._enqueue_calibrated(clock, pipeline.ranked_probabilities_device(), pipeline.n_queries * n)
            with clock.host("copy_back"):       # n entries per query (synchronises the null stream the stages ran on)
                for out, chunk in zip(slots, pipeline.ranked(n)):
                    out[first:last] = chunk
                if d_calibrated is not None:
                    calibrated[first:last] = d_calibrated.to_host(pipeline.n_queries * n).reshape(-1, n)
                    d_calibrated.free()
                if kept is not None:
                    exact, best = pipeline.exact_matches(), pipeline.best_rows()
                    kept.rows[first:last] = pipeline.rows()
                    kept.ratios[first:last] = pipeline.close_matches()[0]
                    kept.probabilities[first:last] = pipeline.predictions()
                    kept.exact[first:last] = exact
                    kept.close[first:last] = np.where(exact >= 0, -1, best)
            clock.collect()
            if tail is not None:
                tail(pipeline, clock)
        return slots, clock

    def _chunk(self, pipeline, clock, match_row, stage, probability, single):
        k, first, n = self.top_n, pipeline.q_first, pipeline.n_queries
        last = first + n
        # 1. top-k, 2. close matches, 3. the exact stage, 4. the pairs of the queries still unmatched
        self._score_chunk(pipeline, clock, self.levenshtein_threshold, score_all=False)
        clock.device("remaining_pairs", pipeline.enqueue_remaining_pairs)
        n_remaining, n_pairs = pipeline.remaining_counts()
        # 5. features of the remaining pairs, 6. the forest, 7. one match per remaining query
        clock.device("features", lambda: pipeline.enqueue_features_remaining(n_pairs))
        clock.device("model", lambda: pipeline.enqueue_predict(self.model, n_pairs=n_pairs))
        clock.device("select_matches", lambda: pipeline.enqueue_select_matches(n_remaining, self.probability_threshold))
        clock.collect()

        with clock.host("copy_back"):          # one copy back of the per-query results
            exact = pipeline.exact_matches()
            best = pipeline.best_rows()        # exact rows where they exist, else the close step's best row
            match_query, model_rows = pipeline.matches(n_remaining)
            predictions = pipeline.predictions(n_pairs).reshape(n_remaining, k)

        close = np.where(exact >= 0, -1, best)
        model = np.full(n, -1, dtype=np.int32)
        local = match_query.astype(np.int64) - first
        model[local] = model_rows
        rows, stages = combine_stages(exact, close, model)
        chunk_probability = np.full(n, np.nan, dtype=np.float32)
        chunk_probability[rows >= 0] = 1.0
        if n_remaining:
            chunk_probability[local] = predictions.max(axis=1)
        if single and n_remaining:
            # cli.py / predict.py:239-242: the model stage of one title takes the best candidate with no threshold,
            # the first in top-n order when several hold the maximum
            pair_t = pipeline.remaining_pairs(n_pairs)[1].reshape(n_remaining, k)
            where = int(np.argmax(predictions[0]))
            rows[local[0]] = pair_t[0, where]
            stages[local[0]] = STAGE_MODEL
        match_row[first:last] = rows
        stage[first:last] = stages
        probability[first:last] = chunk_probability
