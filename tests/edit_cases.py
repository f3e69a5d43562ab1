"""The cases of the edit-script tests (test_edits_cpu.py, test_gpu_edits.py): hand-written pairs with the script the rule
of DESIGN.md section 8 ("Edit scripts and the learned misspelling model") gives them, worked out by hand from the rule's
text, the length edges of the alignment kernel, and the labelled pairs of tests/golden/training_rows.npz."""
import os

import numpy as np

import edit_oracle as eo
import training_set_oracle as ts

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M, S, D, I, T = eo.MATCH, eo.SUBSTITUTE, eo.DELETE, eo.INSERT, eo.TRANSPOSE

# (truth title a, observed title b, distance, script)
HAND_PAIRS = [
    ("abc", "abc", 0, [M, M, M]),                                  # equal titles
    ("abc", "xabc", 1, [I, M, M, M]),                              # one insertion at the first position
    ("abc", "abcx", 1, [M, M, M, I]),                              # ... at the last
    ("xabc", "abc", 1, [D, M, M, M]),                              # one deletion at the first position
    ("abcx", "abc", 1, [M, M, M, D]),                              # ... at the last
    ("ab", "ba", 1, [T]),                                          # one transposition
    ("abz", "baz", 1, [T, M]),
    ("ca", "abc", 3, [I, S, S]),                                   # optimal string alignment, not true Damerau (2)
    ("zca", "zabc", 3, [M, I, S, S]),
    ("aab", "ab", 1, [D, M, M]),                                   # the tie rule deletes the FIRST a
    ("zaab", "zab", 1, [M, D, M, M]),
    ("abc", "xyz", 3, [S, S, S]),                                  # nothing in common
    ("abcdef", "bacdef", 1, [T, M, M, M, M]),                      # transposition at the first two characters
    ("abcdef", "abcdfe", 1, [M, M, M, M, T]),                      # ... at the last two
    ("the cat", "teh cat", 1, [M, T, M, M, M, M]),
    ("abcd", "acbd", 1, [M, T, M]),
]
DEVICE_HAND_PAIRS = [case for case in HAND_PAIRS if len(case[0]) >= 3 and len(case[1]) >= 3]


def codes(title):
    return ts.to_codes(title)


def _letters(rng, n, alphabet):
    return "".join(alphabet[i] for i in rng.randint(0, len(alphabet), n))


def length_edge_pairs():
    """(a, b) at the length edges: 3 and 255 on either side, equal and disjoint at 255 x 255, and every length on both
    sides of the lane (4 columns) and 64-column edges, mutated so that the distance is not trivial."""
    rng = np.random.RandomState(11)
    low, high = "abcdefghijklm ", "nopqrstuvwxyz0123456789"
    long_a, long_b = _letters(rng, 255, low), _letters(rng, 255, high)
    pairs = [("abc", "abd"), ("abc", long_a), (long_a, "abc"), (long_a, long_a), (long_a, long_b)]
    for n in (63, 64, 65, 127, 128, 129, 191, 192, 193, 254, 255):
        base = _letters(rng, n, low + high)
        other = list(base)
        other[n // 3], other[n // 3 + 1] = other[n // 3 + 1], other[n // 3]       # a swap
        other[n - 1] = "q" if other[n - 1] != "q" else "r"                         # a substitution in the last column
        del other[n // 2]                                                          # a deletion
        other = "".join(other)
        pairs += [(base, other), (other, base), (base, _letters(rng, max(3, n - 60), low + high))]
    return pairs


def max_edits_pairs():
    """Pairs of distance 4 and 5 (max_edits = 4: at and just above), 0, 32 and 33."""
    base = "abcdefghijklm" * 5
    out = [(base, base)]
    for edits in (4, 5, 32, 33):
        out.append((base, "z" * edits + base[edits:]))        # `edits` substitutions by a character base does not hold
    return out


def fixture_pairs(transform_titles):
    """The labelled pairs of training_rows.npz as transformed strings: (truth titles, train titles, truth row of every
    labelled train row, the labelled train rows)."""
    g = dict(np.load(os.path.join(GOLDEN, "training_rows.npz"), allow_pickle=False))
    truth = transform_titles([bytes(x).decode("utf-8") for x in g["truth_titles"]])
    train = transform_titles([bytes(x).decode("utf-8") for x in g["train_titles"]])
    row_of = {int(title_id): row for row, title_id in enumerate(g["truth_ids"])}
    labelled = [i for i, title_id in enumerate(g["train_ids"]) if int(title_id) >= 0]
    return truth, train, [row_of[int(g["train_ids"][i])] for i in labelled], labelled


def fixture_profile(transform_titles, max_edits=4):
    """The oracle's counts block of the fixture's labelled pairs."""
    truth, train, truth_rows, labelled = fixture_pairs(transform_titles)
    truth_codes, train_codes = [codes(t) for t in truth], [codes(t) for t in train]
    return eo.align_batch(truth_codes, truth_rows, train_codes, labelled, max_edits)[3]
