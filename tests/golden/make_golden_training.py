#!/usr/bin/env python3
"""Golden vectors of the training-set generation (run in the BUILD container only, on the CPU):

    misspell_cases.npz   generate_misspelled_name (feature_engineering_prepare.py:165-173) of ~2,000 transformed example
                         truth titles longer than 9 characters and ~40 crafted edge titles, plus the reference's
                         EUCLIDEAN_NEIGHBOURS as a 26 x 26 matrix;
    training_rows.npz    FeatureEngineering._prepare_training_input_data (feature_engineering.py:207-274) on a slice of
                         the example data (3,000 truth titles, ~440 train rows with repeated ids and -1 rows): every
                         row's (kind, title, truth title, target), and per train row whether its top-100 has a near-tie
                         at the cut (the `margin_ok` test of make_golden.py);
    misspell_matrix.npz  generate_misspelled_name of the edge titles and of more crafted ones (digits only at 255
                         characters, a space where the cut falls, short titles with digits), each MATRIX_REPEATS times
                         with a stream of its own: per case the title, the answer, the names of the edit functions the
                         reference applied, whether each returned its input unchanged, and the string handed to
                         transform_title.

It runs the reference's own function bodies under make_golden.py's shims (numba as pass-through decorators), with
`random` in feature_engineering_prepare replaced by a replay object that draws from the port's stream (DESIGN.md
section 8, tests/training_set_oracle.py `Stream`): the misspelling of truth row / title i draws from the purpose-1 stream
of i, the sample of train row i (the random.sample right after get_closest_matches(i)) from the purpose-2 stream of i,
and the keyboard neighbours of a letter are listed in ascending character order.
The fixtures are written with fixed zip timestamps, so a second run reproduces the same bytes.  Nothing is written
under the reference tree.

Usage:  PYTHONHASHSEED=0 python tests/golden/make_golden_training.py
"""
import gzip
import io
import os
import shutil
import sys
import tempfile
import warnings
import zipfile

if os.environ.get("PYTHONHASHSEED") != "0":
    sys.exit("run with PYTHONHASHSEED=0 (the reference's sets and dicts are iterated)")
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
from training_set_oracle import Stream  # noqa: E402

REFERENCE = make_golden.REFERENCE
SEED = 0
N_TRUTH, N_TRAIN_FOUND, N_TRAIN_NEGATIVE, N_REPEATS = 3000, 350, 60, 30


class Replay:
    """Stands in for the `random` module of feature_engineering_prepare: randint / choice / sample from the current
    stream, which the wrappers below select before every title and every train row."""

    def __init__(self, seed):
        self.seed, self.stream = seed, None

    def use(self, purpose, index):
        self.stream = Stream(self.seed, purpose, index)

    def randint(self, a, b):
        return self.stream.randint(a, b)

    def choice(self, sequence):
        return self.stream.choice(sequence)

    def sample(self, population, k):
        return self.stream.sample(population, k)


def _save(path, **arrays):
    """np.savez_compressed with fixed timestamps (reproducible bytes)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as archive:
        for name, value in arrays.items():
            buffer = io.BytesIO()
            np.lib.format.write_array(buffer, np.asanyarray(value), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            archive.writestr(info, buffer.getvalue())


def _utf8(strings):
    return np.array([s.encode("utf-8") for s in strings])


def _edge_titles():
    words = ["alpha", "beta", "gamma", "delta", "mn", "pq", "zx", "limited", "holdings", "services"]
    long_title = " ".join(words[i % len(words)] for i in range(60))

    def cut(n):
        text = long_title[:n].rstrip()
        while len(text) < n:                       # grow the last word to exactly n characters
            text += "k"
        return text

    titles = [
        "abcde fghi", "abcdefghij", "a bcdefghij", "ab cdefghijk", "x yz",            # lengths 10, one letter first
        cut(254), cut(255), cut(253), "m" * 255, "p" * 254,                             # the cut, add_letter at 255
        "a b c d e f g h", "a b", "q w e r t y", "i o p l k j h g",                     # one-letter words
        "12 345 6789 00", "0 1 2 3 4 5 6 7 8 9", "1234567890", "000", "99 99",          # digits and spaces only
        "abcdefghijklmnop", "mnmnmnmnmn", "pppppppppppp", "zzzzzzzzzz",                 # one word
        "a 1 2 3 4 5 6 7 8", "b 0000000000", "1 a 2", "e 12345678",                     # removals that expose spaces
        "abc", "abcd", "ab c", "a bc", "aaa", "n m nn", "the company limited",           # short titles
        "coolblue bv", "great expectations ministries", "x" * 10 + " " + "y" * 10,
        "q 1 w 2 e 3 r 4 t 5 y 6", "0a 0b 0c 0d", "limited ltd plc llp inc",
    ]
    titles = [t for t in titles if 3 <= len(t) <= 255]
    assert len(titles) >= 40 and len(set(titles)) == len(titles)
    assert len(cut(254)) == 254 and len(cut(255)) == 255
    return titles


MATRIX_REPEATS = 64
EDITS = ("swap_word", "add_letter", "remove_letter", "replace_letter", "add_space", "remove_space")


def _matrix_titles():
    """The edge titles and the ones that reach what they cannot: long titles of digits only, a space where the cut to
    255 falls, short titles with a digit, long titles of one-letter words, more one-word titles."""
    one_letter_words = " ".join("abcdefghijklmnopqrstuvwxyz"[i % 26] for i in range(128))
    more = [
        "1" * 255, "1 " * 127 + "1",                                                    # long, digits and spaces only
        "k" * 253 + " k", "k" * 252 + " kk", "k" * 251 + " kkk", "k" * 254 + "b",       # a space at the cut
        "ab 1", "0 0", "a 1", "1 2", "7777",                                            # short, digits
        one_letter_words, one_letter_words[:253], "g" * 253 + "7", "h" * 126 + " " + "j" * 126 + "5",
        "qwe", "rtyu", "12345", "zxcvbnm",                                              # one word
    ]
    titles = _edge_titles() + more
    assert len(one_letter_words) == 255 and len(more[-6]) == 254 and len(more[-5]) == 254
    assert all(3 <= len(t) <= 255 for t in titles) and len(set(titles)) == len(titles)
    return titles


def _misspell_matrix(prepare, replay):
    """Every title of _matrix_titles MATRIX_REPEATS times, case i from the purpose-1 stream of i.  Per case: the
    reference's answer, the functions it applied in order, whether each returned its input, and the string that went
    into transform_title."""
    log = []

    def logged(name, function):
        def call(x, length):
            result = function(x, length)
            log.append((name, result == x, result))
            return result
        return call

    plain = {name: getattr(prepare, name) for name in EDITS}
    for name, function in plain.items():
        setattr(prepare, name, logged(name, function))
    cases = [title for title in _matrix_titles() for _ in range(MATRIX_REPEATS)]
    expected, functions, edited = [], [], []
    unchanged = np.zeros((len(cases), 2), dtype=bool)
    try:
        for index, title in enumerate(cases):
            del log[:]
            replay.use(1, index)
            expected.append(prepare.generate_misspelled_name(title))
            assert 1 <= len(log) <= 2
            functions.append(",".join(entry[0] for entry in log))
            unchanged[index, :len(log)] = [entry[1] for entry in log]
            edited.append(log[-1][2])
    finally:
        for name, function in plain.items():
            setattr(prepare, name, function)
    _save(f"{HERE}/misspell_matrix.npz", titles=_utf8(cases), expected=_utf8(expected), functions=_utf8(functions),
          unchanged=unchanged, edited=_utf8(edited), seed=np.uint64(SEED), repeats=np.int32(MATRIX_REPEATS))
    return len(cases)


def _train_slice(train_lines, truth_ids, rng):
    """Train CSV lines: the first rows whose id is in the truth slice and the first -1 rows, in file order, then
    N_REPEATS more rows holding ids of earlier rows (the raw truth name as title) at random places."""
    found, negative = [], []
    for line in train_lines:
        title_id = int(line.rsplit("|", 1)[1])
        if title_id in truth_ids and len(found) < N_TRAIN_FOUND:
            found.append(line)
        elif title_id == -1 and len(negative) < N_TRAIN_NEGATIVE:
            negative.append(line)
    chosen = set(found + negative)
    rows = [line for line in train_lines if line in chosen]
    repeated = rng.choice(len(found), N_REPEATS, replace=False)
    for r in repeated:
        title_id = int(found[r].rsplit("|", 1)[1])
        rows.insert(int(rng.randint(0, len(rows) + 1)), f"0|{truth_ids[title_id]}|{title_id}")
    return [f"{i}|{line.split('|', 1)[1]}" for i, line in enumerate(rows)]


def main():
    data_dir = tempfile.mkdtemp(prefix="ds_golden_training_")
    rng = np.random.RandomState(2024)
    with gzip.open(f"{REFERENCE}/example_dataset/example_truth.csv.gz", "rt") as handle:
        truth_header, *truth_lines = handle.read().splitlines()
    with gzip.open(f"{REFERENCE}/example_dataset/example_train.csv.gz", "rt") as handle:
        train_header, *train_lines = handle.read().splitlines()
    truth_lines = truth_lines[:N_TRUTH]
    truth_ids = {int(line.split("|", 1)[0]): line.split("|", 1)[1] for line in truth_lines}
    train_rows = _train_slice(train_lines, truth_ids, rng)
    with open(f"{data_dir}/example_truth.csv", "w") as handle:
        handle.write("\n".join([truth_header] + truth_lines) + "\n")
    with open(f"{data_dir}/example_train.csv", "w") as handle:
        handle.write("\n".join([train_header] + train_rows) + "\n")
    shutil.copy(f"{data_dir}/example_train.csv", f"{data_dir}/example_test.csv")   # read by nothing here
    os.environ["PROJECT_DATA_PATH"] = data_dir
    make_golden._install_shims()
    sys.path.insert(0, REFERENCE)
    warnings.simplefilter("ignore")

    import doppelspeller.constants as c
    import doppelspeller.settings as s
    from doppelspeller import common, feature_engineering, feature_engineering_prepare, match_maker

    replay = Replay(SEED)
    feature_engineering_prepare.random = replay
    # the same sets, each listed in ascending character order (the reference lists a set in its iteration order)
    feature_engineering_prepare.EUCLIDEAN_NEIGHBOURS = {
        letter: sorted(near) for letter, near in feature_engineering_prepare.EUCLIDEAN_NEIGHBOURS.items()}

    # ---- misspell_cases.npz: the example truth set's titles longer than 9 characters and the edge titles
    with gzip.open(f"{REFERENCE}/example_dataset/example_truth.csv.gz", "rt") as handle:
        every_title = [line.split("|", 1)[1] for line in handle.read().splitlines()[1:]]
    transformed = sorted(set(common.transform_title(t) for t in every_title))
    long_titles = [t for t in transformed if len(t) > 9]
    titles = [long_titles[i] for i in sorted(rng.choice(len(long_titles), 2000, replace=False))] + _edge_titles()
    expected = []
    for index, title in enumerate(titles):
        replay.use(1, index)
        expected.append(feature_engineering_prepare.generate_misspelled_name(title))
    letters = "abcdefghijklmnopqrstuvwxyz"
    neighbours = np.zeros((26, 26), dtype=bool)
    for letter, near in feature_engineering_prepare.EUCLIDEAN_NEIGHBOURS.items():
        for other in near:
            neighbours[letters.index(letter), letters.index(other)] = True
    _save(f"{HERE}/misspell_cases.npz", titles=_utf8(titles), expected=_utf8(expected), seed=np.uint64(SEED),
          neighbours=neighbours)

    # ---- training_rows.npz: _prepare_training_input_data with the replayed draws
    fe = feature_engineering.FeatureEngineering(c.DATA_TYPE_TRAIN)
    truth = fe.truth_data
    generated_rows = [row for row, title in enumerate(truth[c.COLUMN_TRANSFORMED_TITLE]) if len(title) > 9]
    calls = iter(generated_rows)

    def misspelled(title):           # the per-title call of _generate_dummy_train_data (feature_engineering.py:185-188)
        row = next(calls)
        assert truth[c.COLUMN_TRANSFORMED_TITLE].iloc[row] == title
        replay.use(1, row)
        return feature_engineering_prepare.generate_misspelled_name(title)

    closest = match_maker.MatchMaker.get_closest_matches

    def closest_matches(self, row_number):   # the random.sample of feature_engineering_prepare.py:45 follows each call
        replay.use(2, row_number)
        return closest(self, row_number)

    feature_engineering.generate_misspelled_name = misspelled
    match_maker.MatchMaker.get_closest_matches = closest_matches
    train_frame = fe.data.copy()
    rows = fe._prepare_training_input_data()
    match_maker.MatchMaker.get_closest_matches = closest
    assert next(calls, None) is None

    # near-ties at the top-100 cut, per train row (make_golden.py `margin_ok`)
    mm = match_maker.MatchMaker(train_frame.copy(), truth.copy(), s.TOP_N_RESULTS_TO_FIND_FOR_PREDICTING)
    q_maxint = np.array([sum([mm._get_idf_given_index(r) for r in mm.matrix_non_zero_columns[q]])
                         for q in range(len(train_frame))], dtype=np.float64)
    _, margin_ok = make_golden._match_maker_answers(match_maker, s, mm, q_maxint, len(train_frame),
                                                    s.TOP_N_RESULTS_TO_FIND_FOR_PREDICTING)
    _save(f"{HERE}/training_rows.npz",
          truth_titles=_utf8(truth[c.COLUMN_TITLE]), truth_ids=np.asarray(truth[c.COLUMN_TITLE_ID], dtype=np.int64),
          train_titles=_utf8(train_frame[c.COLUMN_TITLE]),
          train_ids=np.asarray(train_frame[c.COLUMN_TITLE_ID], dtype=np.int64),
          seed=np.uint64(SEED), top_n=np.int32(s.TOP_N_RESULTS_TO_FIND_FOR_PREDICTING),
          sample_n=np.int32(s.TOP_N_RESULTS_TO_FIND_FOR_TRAINING),
          kind=np.array([r[0] for r in rows], dtype=np.uint8), title=_utf8([r[1] for r in rows]),
          truth_title=_utf8([r[2] for r in rows]), target=np.array([r[3] for r in rows], dtype=np.uint8),
          near_tie=~margin_ok)
    shutil.rmtree(data_dir)

    # ---- misspell_matrix.npz: many draws per edge title, with the functions the reference applied
    n_cases = _misspell_matrix(feature_engineering_prepare, replay)
    print(f"misspell_cases.npz: {len(titles)} titles; training_rows.npz: {len(rows)} rows, "
          f"{int((~margin_ok).sum())} train rows with near-ties; misspell_matrix.npz: {n_cases} cases")


if __name__ == "__main__":
    main()
