"""The rule of ds_hard_negatives_device (include/doppel_amd.h, DESIGN.md section 8 "Hard negatives") restated twice, and
the named cases the tests mine.

    mine_sorted   a title at a time with a stable sort on (-margin, j), -0.0 put behind +0.0 by hand
    mine_keys     NumPy, through the 64-bit keys (ord(margin) << 32) | ~j, descending

Per title i: candidate j is eligible when 0 <= rows[i, j] < n_truth, rows[i, j] != own[i], rows[i, j] is not in
exclude[i, :] and margins[i, j] > min_margin (strict, float32); the title yields its first min(hard_n, eligible)
candidates by margin descending (-0.0 below +0.0), then j ascending.  The output is dense, titles in order:
(pair_q = q_first + i, pair_t = the row, position = j, margin) and the total.

Every case is built from fixed arrays and plain arithmetic: no random generator that could drift."""
import numpy as np

REGISTER_CANDIDATES = 256       # lists up to here keep their keys in registers (64 * kHardRegisterKeys), longer ones do not
NO_THRESHOLD = np.float32(-np.inf)


def _empty():
    return (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), 0)


def _pack(pairs):
    if not pairs:
        return _empty()
    q, t, j, bits = (np.array(column, dtype=np.int64) for column in zip(*pairs))
    return q.astype(np.int32), t.astype(np.int32), j.astype(np.int32), bits.astype(np.uint32).view(np.float32), len(pairs)


def mine_sorted(rows, margins, own, exclude, n_truth, hard_n, min_margin, q_first=0):
    margins = np.ascontiguousarray(margins, dtype=np.float32)
    bits = margins.view(np.uint32)
    threshold = np.float32(min_margin)
    pairs = []
    for i in range(rows.shape[0]):
        left_out = set() if exclude is None else {int(e) for e in exclude[i] if e != -1}
        eligible = [j for j in range(rows.shape[1])
                    if 0 <= int(rows[i, j]) < n_truth and int(rows[i, j]) != int(own[i]) and int(rows[i, j]) not in left_out
                    and margins[i, j] > threshold]
        # stable: equal margins keep the order of j; -0.0 == +0.0 as numbers, so the sign of a zero is the second key
        ordered = sorted(eligible, key=lambda j: (-float(margins[i, j]),
                                                  1 if margins[i, j] == 0 and np.signbit(margins[i, j]) else 0))
        pairs += [(q_first + i, int(rows[i, j]), j, int(bits[i, j])) for j in ordered[:hard_n]]
    return _pack(pairs)


def order_of(margins):
    """uint32: the monotone map of the float32 bits (all bits flipped when the sign is set, else the sign bit set)."""
    bits = np.ascontiguousarray(margins, dtype=np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def keys_of(rows, margins, own, exclude, n_truth, min_margin):
    """uint64[n, k]: the key of every candidate, 0 where it is not eligible."""
    rows = np.asarray(rows, dtype=np.int64)
    margins = np.ascontiguousarray(margins, dtype=np.float32)
    eligible = (rows >= 0) & (rows < n_truth) & (rows != np.asarray(own, dtype=np.int64)[:, None]) & \
        (margins > np.float32(min_margin))
    if exclude is not None and exclude.shape[1]:
        held = np.asarray(exclude, dtype=np.int64)
        eligible &= ~((rows[:, :, None] == held[:, None, :]) & (held[:, None, :] != -1)).any(axis=2)
    position = np.broadcast_to(np.arange(rows.shape[1], dtype=np.uint32), rows.shape)
    keys = (order_of(margins).astype(np.uint64) << np.uint64(32)) | (~position).astype(np.uint64)
    return np.where(eligible, keys, np.uint64(0))


def mine_keys(rows, margins, own, exclude, n_truth, hard_n, min_margin, q_first=0):
    keys = keys_of(rows, margins, own, exclude, n_truth, min_margin)
    bits = np.ascontiguousarray(margins, dtype=np.float32).view(np.uint32)
    pairs = []
    for i in range(keys.shape[0]):
        descending = np.sort(keys[i])[::-1]
        for key in descending[:hard_n]:
            if key == 0:
                break
            j = int(~np.uint32(key & np.uint64(0xffffffff)))
            pairs.append((q_first + i, int(rows[i, j]), j, int(bits[i, j])))
    return _pack(pairs)


def same_mined(a, b):
    """Bit for bit: four arrays of equal dtype and shape (the margins compared as their bits) and the total."""
    return a[4] == b[4] and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
                                for x, y in zip(a[:4], b[:4]))


# ---- the cases ------------------------------------------------------------------------------------------------------------
def _base(n, k, n_truth):
    """Distinct rows per title, inside the table; margins in steps of 1/8 between -6.25 and 6.25, with repeats once k
    passes 101."""
    assert n_truth >= k + n
    i, j = np.arange(n)[:, None], np.arange(k)[None, :]
    rows = ((i * 5 + j) % n_truth).astype(np.int32)
    margins = ((((j * 37 + i * 11) % 101) - 50) / 8).astype(np.float32)
    return rows, np.ascontiguousarray(margins)


def _case(rows, margins, own, exclude, n_truth, hard_n, min_margin=NO_THRESHOLD, q_first=0):
    exclude = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.int32)
    return dict(rows=np.ascontiguousarray(rows, dtype=np.int32), margins=np.ascontiguousarray(margins, dtype=np.float32),
                own=np.ascontiguousarray(own, dtype=np.int32), exclude=exclude, n_truth=int(n_truth), hard_n=int(hard_n),
                min_margin=np.float32(min_margin), q_first=int(q_first))


def _cases():
    cases = {}
    absent = lambda n: np.full(n, -1, np.int32)

    rows, margins = _base(1, 1, 4)
    cases["k1_single"] = _case(rows, margins, absent(1), None, 4, 1)                       # hard_n == k == 1, one title

    rows, margins = _base(4, 5, 40)
    cases["k5_own_first"] = _case(rows, margins, rows[:, 0], None, 40, 3, q_first=7)
    margins = margins.copy()
    margins[:, 4] = 6.5                                                                    # the own row would win
    cases["k5_own_last"] = _case(rows, margins, rows[:, 4], None, 40, 5)                   # hard_n == k, four titles

    rows, margins = _base(5, 64, 100)
    own = np.array([rows[0, 63], 99, -1, rows[3, 0], -1], dtype=np.int32)                  # last, not a candidate, none, first
    cases["k64_full"] = _case(rows, margins, own, None, 100, 16)

    rows, margins = _base(4, 65, 100)
    margins = margins.copy()
    margins[:, 10] = margins[:, 63] = margins[:, 64] = 7.0                                 # a tie on both sides of lane 63 / 64
    margins[:, 1] = margins[:, 2] = 6.75                                                   # and one between two lanes
    cases["k65_ties"] = _case(rows, margins, absent(4), None, 100, 3)
    cases["k65_ties_deep"] = _case(rows, margins, absent(4), None, 100, 16)

    rows, margins = _base(9, 100, 300)
    best = np.argsort(-margins, axis=1, kind="stable")
    exclude = np.full((9, 4), -1, dtype=np.int32)                                          # title 0: only -1 entries
    exclude[1, :2] = rows[1, best[1, :2]]                                                  # the two best, and two -1
    exclude[2] = [290, 291, 292, 293]                                                      # rows that are no candidates
    exclude[3] = [rows[3, best[3, 0]], -1, rows[3, best[3, 2]], 299]                       # a -1 between two that count
    exclude[4:] = rows[np.arange(4, 9), best[4:, 1]][:, None]                                         # the same row four times
    own = np.where(np.arange(9) % 2 == 0, rows[np.arange(9), best[:, 0]], -1)              # the best candidate is the own row
    cases["k100_exclude"] = _case(rows, margins, own, exclude, 300, 3, q_first=1000)

    rows, margins = _base(5, 130, 200)
    margins = -np.abs(margins) - np.float32(0.125)                                         # all negative, many equal
    cases["k130_negative"] = _case(rows, margins, rows[:, 129], None, 200, 16)

    for k in (REGISTER_CANDIDATES, REGISTER_CANDIDATES + 1):                               # the last list in registers, the first not
        rows, margins = _base(5, k, 400)
        margins = margins.copy()
        margins[:, k - 1] = 7.0                                                            # the last candidate wins
        cases[f"k{k}_path_edge"] = _case(rows, margins, absent(5), None, 400, 3)

    rows, margins = _base(4, 600, 700)
    margins = margins.copy()
    margins[1, :] = -3.0
    margins[1, [5, 599]] = 6.0                                                             # two above the threshold only
    margins[2, :] = 5.0                                                                    # none above it
    cases["k600_threshold"] = _case(rows, margins, absent(4), None, 700, 16, min_margin=5.0)

    rows = np.array([[3, 4, 5, 6, 7]] * 2, dtype=np.int32)
    margins = np.array([[-0.0, 0.0, -0.0, 0.0, -1.0], [0.0, -0.0, 0.0, -0.0, 1.0]], dtype=np.float32)
    cases["zeros"] = _case(rows, margins, absent(2), None, 10, 3)
    cases["zeros_threshold"] = _case(rows, margins, absent(2), None, 10, 5, min_margin=-0.0)   # nothing is above -0.0 but 1.0

    margins = np.array([[1.5, 0.25, 0.25, 2.0, -3.0], [0.25, 0.25, 0.25, 0.25, 0.25]], dtype=np.float32)
    cases["cut_at_the_threshold"] = _case(rows, margins, absent(2), None, 10, 3, min_margin=0.25)

    rows, margins = _base(5, 17, 30)
    rows = rows.copy()
    rows[:, 0], rows[:, 5], rows[:, 9], rows[:, 16] = -1, 30, -7, 35                        # -1, n_truth, and beyond both
    margins = margins.copy()
    margins[:, [0, 5, 9, 16]] = 7.0                                                        # they would all win
    cases["invalid_rows"] = _case(rows, margins, np.array([-1, 29, rows[2, 1], -1, rows[4, 15]]), None, 30, 3)

    rows, margins = _base(5, 16, 60)
    exclude = np.full((5, 16), -1, dtype=np.int32)
    exclude[1] = rows[1]                                                                   # every candidate of title 1 ...
    exclude[3] = rows[3][::-1]                                                             # ... and of title 3, in another order
    exclude[2, :14] = rows[2, :14]                                                         # title 2 keeps two
    cases["exclude_everything"] = _case(rows, margins, absent(5), exclude, 60, 16)         # hard_n == k == 16, 16 exclusions

    rows, margins = _base(9, 5, 60)
    cases["nothing_mined"] = _case(rows, margins, absent(9), None, 60, 3, min_margin=6.0)   # the largest margin there is
    cases["nine_titles"] = _case(rows, margins, rows[:, 2], np.zeros((9, 0), np.int32), 60, 1)
    return cases


CASES = _cases()


def chunk_of(case, first, last):
    """Titles [first, last) of a case as a call's arguments: q_first moves with them."""
    exclude = case["exclude"]
    return dict(case, rows=case["rows"][first:last], margins=case["margins"][first:last], own=case["own"][first:last],
                exclude=None if exclude is None else exclude[first:last], q_first=case["q_first"] + first)


def arguments(case):
    return tuple(case[name] for name in ("rows", "margins", "own", "exclude", "n_truth", "hard_n", "min_margin", "q_first"))
