"""The bootstrap of a threshold sweep's cells restated from the rule's text ("Bootstrap of the
cells"), out of what the other oracles already have, and the cases the CPU and the GPU test share.

    predictions[t][u][q]     sweep_cases.predictions_of: the truth row every query gets in every cell
    codes[t * U + u][q]      bootstrap_oracle.accuracy_codes of those against the actual rows
    counts, baseline         bootstrap_oracle.counts(codes, unit, n_units, B, seed), reshaped to [B][T][U][4] and [T][U][4]
    record[q][t]             from the U codes of (q, t) alone: all the same -> that code; otherwise a flip at
                             pos = the first u with a not-found code (0 or 2): kind 4 for codes 1 -> 0, 5 for 3 -> 2,
                             6 for 1 -> 2; the record is kind | pos << 3

None of it looks at the kernels' bookkeeping.  A flip can only be read off the codes when some cell is past it, so the
records of this module hold pos in 1..U - 1; a record with pos = U decodes to one code in every cell (`decode`), and the
kernel that writes records writes that code instead.
"""
import functools

import numpy as np

import bootstrap_oracle as bo
import sweep_cases as sc

SWEEP_COUNTER_OF_CODE = (2, 1, 3, 0)       # code c is the sweep's counter SWEEP_COUNTER_OF_CODE[c]
FLIPS = {(1, 0): 4, (3, 2): 5, (1, 2): 6}  # (code below pos, code from pos on) -> kind


def cell_codes(oracle, queries, lev, prob):
    """uint8[T * U][Q]."""
    rows, d, r, s, p, exact, actual = queries
    predictions = sc.predictions_of(oracle, rows, d, r, s, p, exact, lev, prob)
    cells = predictions.reshape(len(lev) * len(prob), rows.shape[0])
    return np.stack([bo.accuracy_codes(cells[c], actual) for c in range(cells.shape[0])])


def records_of(codes, T, U):
    """uint16[Q][T] from codes uint8[T * U][Q]."""
    by_cell = np.asarray(codes).reshape(T, U, -1)
    out = np.zeros((by_cell.shape[2], T), np.uint16)
    for t in range(T):
        for q in range(by_cell.shape[2]):
            column = by_cell[t, :, q].tolist()
            if len(set(column)) == 1:
                out[q, t] = column[0]
                continue
            pos = min(u for u in range(U) if column[u] in (0, 2))
            below, beyond = column[0], column[pos]
            assert column == [below] * pos + [beyond] * (U - pos), (t, q, column)    # one flip, and only downwards
            out[q, t] = FLIPS[(below, beyond)] | (pos << 3)
    return out


def decode(records, U):
    """uint8[T * U][Q] from uint16[Q][T]: the code of every title in every cell."""
    records = np.asarray(records).astype(np.int64)
    what, pos = records & 7, records >> 3
    assert (what < 7).all()
    below = np.select([what == 4, what == 5, what == 6], [1, 3, 1], what)
    beyond = np.select([what == 4, what == 5, what == 6], [0, 2, 2], what)
    u = np.arange(U)[None, None, :]
    cells = np.where((what[:, :, None] >= 4) & (u >= pos[:, :, None]), beyond[:, :, None], below[:, :, None])   # [Q][T][U]
    return np.ascontiguousarray(cells.transpose(1, 2, 0).reshape(-1, records.shape[0])).astype(np.uint8)


def counts(codes, T, U, unit, n_units, n_boot, seed):
    """(int64[B][T][U][4], int64[T][U][4])."""
    replicates, baseline = bo.counts(codes, unit, n_units, n_boot, seed)
    return replicates.reshape(n_boot, T, U, 4), baseline.reshape(T, U, 4)


# ---- the cases ----------------------------------------------------------------------------------------------------------
GRIDS = {"1x1": sc.grid(1, 1), "3x7": sc.GRID_3X7, "65x3": sc.grid(65, 3), "64x46": sc.grid(64, 46), "65x47": sc.grid(65, 47),
         "101x256": sc.grid(101, 256)}
# the records kernel: (queries, candidates, grid)
RECORD_CASES = [(1, 1, "1x1"), (1, 5, "3x7"), (4, 5, "3x7"), (5, 64, "3x7"), (257, 65, "3x7"), (257, 100, "3x7"),
                (257, 5, "1x1"), (5, 1, "3x7"), (257, 5, "64x46"), (257, 64, "65x47"), (5, 65, "101x256"), (4, 100, "65x3")]
# the bootstrap kernel: (titles, grid); every one runs without units and with 1, 2 and 65 units, B = 1 and 5
BOOT_CASES = [(1, "1x1"), (2, "3x7"), (63, "3x7"), (64, "65x3"), (65, "101x256"), (257, "3x7"), (257, "1x1"), (65, "65x3")]
UNITS = (None, 1, 2, 65)


def edge_positions(queries, prob):
    """Every eighth query behind the crafted ones is left to the model stage (no exact row, no close candidate) with one
    candidate above all others: just above the first threshold (the flip is at pos 1) or on the last one (above all but
    that: pos U - 1), in turn.  The actual rows stay as they were drawn, so every kind of flip comes up."""
    rows, d, r, s, p, exact, actual = queries
    for q in range(sc.CRAFTED, rows.shape[0], 8):
        d[q], r[q], s[q], p[q], exact[q] = 0, 0, 0, 0, -1
        p[q, q % rows.shape[1]] = np.nextafter(prob[0], np.float32(2)) if q % 16 < 8 else prob[-1]
        if q % 3 == 0:
            actual[q] = rows[q, q % rows.shape[1]]
    return queries


@functools.lru_cache(maxsize=None)
def record_case(oracle, n_queries, k, grid):
    """dict(queries, lev, prob, codes, records) of seeded queries (sweep_cases.make_queries, the crafted ones in front
    when they fit)."""
    lev, prob = GRIDS[grid]
    queries = edge_positions(sc.make_queries(n_queries, k, 400, seed=1000 + 7 * n_queries + k), prob)
    codes = cell_codes(oracle, queries, lev, prob)
    records = records_of(codes, len(lev), len(prob))
    for array in (codes, records):
        array.setflags(write=False)
    return dict(queries=queries, lev=lev, prob=prob, codes=codes, records=records)


def units_of(n, n_units, seed):
    """int32[n] for n_units units: one unit holds every title (n_units = 1, and the first of 2), else random; with more
    than one unit the last is always empty."""
    if n_units is None:
        return None
    if n_units <= 2:
        return np.zeros(n, np.int32)
    return np.random.RandomState(seed).randint(0, n_units - 1, n).astype(np.int32)


@functools.lru_cache(maxsize=None)
def boot_case(oracle, n, grid, n_units, n_boot):
    """dict(records, T, U, unit, n_units, n_boot, seed, counts, baseline): the records of the oracle for n seeded
    queries of 5 candidates, and the rule's counts.  The seed uses its high half."""
    c = record_case(oracle, n, 5, grid)
    T, U = len(c["lev"]), len(c["prob"])
    unit = units_of(n, n_units, 50 + n)
    seed = (0x5eed0000 + n) * 0x100000001 + (n_units or 0) + 3
    replicates, baseline = counts(c["codes"], T, U, unit, n if n_units is None else n_units, n_boot, seed)
    for array in (replicates, baseline):
        array.setflags(write=False)
    return dict(records=c["records"], codes=c["codes"], T=T, U=U, n=n, unit=unit, n_units=n if n_units is None else n_units,
                n_boot=n_boot, seed=seed, counts=replicates, baseline=baseline)
