"""The inputs of the two-chunk run of the reference's generate_test_predictions (its chunk size of 10,000 is a local of the
function): 10,003 titles, top_n = 2, everything a formula of the title's number so that tests/golden/make_golden_predict.py
and tests/test_reference_stages_cpu.py build the same inputs and the fixture holds the answers only.  The last three titles,
alone in the second chunk, repeat titles 1, 2 and 3 with their candidates and probabilities.  A plain module: no fixtures.
"""
import numpy as np

N_TITLES, TOP_N, N_TRUTH, CHUNK = 10003, 2, 40, 10000
WORDS = ("alpha", "beta", "gamma", "delta", "omega", "north", "south", "capital", "global", "marine")
LEVELS = np.array([0.1, 0.5, np.float32(0.9), np.nextafter(np.float32(0.9), np.float32(1)), 0.95, 0.99], dtype=np.float32)


def source(i):
    """The number whose formulas title i follows: its own, or 1, 2, 3 for the three titles of the second chunk."""
    return i if i < CHUNK else i - CHUNK + 1


def truth_titles():
    """40 titles of 25 characters and more; rows 7 and 31 hold the title of row 3 (the last row of a title wins)."""
    titles = [f"{WORDS[r % 10]} {WORDS[(r * 3 + 1) % 10]} holdings number {r:03d}" for r in range(N_TRUTH)]
    titles[7] = titles[31] = titles[3]
    return titles


def truth_ids():
    return (9000 - 11 * np.arange(N_TRUTH)).astype(np.int64)


def titles():
    truth = truth_titles()
    out = []
    for i in range(N_TITLES):
        j = source(i)
        row = (j // 5) % N_TRUTH
        if j % 5 == 0:
            out.append(truth[row])                                    # exact
        elif j % 5 == 1:
            out.append(f"{truth[row]}{j % 10}")                       # one character more: a close match
        else:
            out.append(f"zq{j:05d} xv{(j * 7) % 1000:03d} unrelated title")
    return out


def rows():
    """int32[N_TITLES, 2]: the planted candidate rows; a title made from a truth row has that row first."""
    j = np.array([source(i) for i in range(N_TITLES)], dtype=np.int64)
    first = np.where(j % 5 <= 1, (j // 5) % N_TRUTH, (j * 3) % N_TRUTH)
    second = (j * 3 + 1 + j % 7) % N_TRUTH
    return np.stack([first, second], axis=1).astype(np.int32)


def probabilities():
    """float32[N_TITLES, 2]: every pair of the six levels in turn: ties, maxima at the float32 nearest to 0.9, at its upper
    neighbour and below it."""
    j = np.array([source(i) for i in range(N_TITLES)], dtype=np.int64)
    return np.stack([LEVELS[j % 6], LEVELS[(j // 6) % 6]], axis=1)
