"""The cases and the references of the hostile-value tests (value_cases.py; DESIGN.md section 9, "Order of values"),
proved on the CPU: the oracle's bins are an integer-key count of cuts, the integer-key tree walk reproduces every
existing oracle's walk on thresholds that are denormals, zeros, infinities and NaN, and the cases hold what they
claim, so that test_gpu_value_edges.py compares the device with references that agree with each other."""
import numpy as np
import pytest

import contributions_cases as cc
import forest_continue_oracle as continued
import forest_inspect_oracle as inspected
import forest_refresh_oracle as refreshed
import forest_train_oracle as trained
import value_cases as vc

FORESTS = ["hostile_forest", "trained_256", "trained_16"]


def forest_and_rows(name):
    if name == "hostile_forest":
        return vc.hostile_forest(0), vc.hostile_matrix(256).rows
    max_bin = int(name.split("_")[1])
    return vc.oracle_trained(max_bin), vc.hostile_matrix(max_bin).rows


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the references agree ---------------------------------------------------------------------------------------------
def test_key_restates_the_order_of_float32():
    values = np.concatenate([vc.ALWAYS, np.array([np.nan, 1.0, -1.0, 5e-39, -5e-39], np.float32),
                             vc.hostile_matrix(256).train[:200].reshape(-1)])
    keys = vc.key(values)
    present = ~np.isnan(values)
    assert (keys[~present] == 0xffffffff).all() and (keys[present] != 0xffffffff).all()
    a, b = values[present][:, None], values[present][None, :]
    assert np.array_equal(a < b, keys[present][:, None] < keys[present][None, :])
    assert np.array_equal(a == b, keys[present][:, None] == keys[present][None, :])
    assert vc.key(np.float32(-0.0)) == vc.key(np.float32(0.0)) == 0x80000000
    assert vc.key(vc.TINY) == 0x80000001 and vc.key(-vc.TINY) == 0x7ffffffe       # denormals keep their place
    assert not vc.below(np.float32(1.0), np.float32(np.nan)) and not vc.below(np.float32(np.nan), np.float32(1.0))


@pytest.mark.parametrize("max_bin", [256, 16, 2])
def test_oracle_bins_are_a_key_count_of_cuts_on_the_hostile_matrix(max_bin):
    h = vc.hostile_matrix(max_bin)
    assert h.rows.shape[1] == 22 and h.n_train == 6000 and h.rows.size <= 7000 * 96
    bins = trained.bins(h.rows, h.cuts)
    assert np.array_equal(bins, vc.key_bins(h.rows, h.cuts))
    assert (bins == trained.MISSING).any() and bins[bins != trained.MISSING].max() == min(max_bin - 2, 254)
    if max_bin == 256:
        cuts = np.concatenate(h.cuts)
        denormal = (cuts != 0) & (np.abs(cuts) < np.finfo(np.float32).tiny)
        assert int(denormal.sum()) == 231


def test_the_full_table_matrix_fills_every_entry_of_the_cut_table():
    x = vc.full_table_matrix()
    assert x.shape == (1000, 96) and x.size <= 7000 * 96
    cuts = trained.cuts(x)
    assert [c.shape[0] for c in cuts] == [254] * 96
    bins = trained.bins(x, cuts)
    assert np.array_equal(bins, vc.key_bins(x, cuts))
    assert all(bins[f][~np.isnan(x[:, f])].max() == 254 for f in range(96))        # the last cut decides somewhere
    tiny = np.finfo(np.float32).tiny
    denormal_columns = [f for f in range(96) if (np.abs(x[:, f][~np.isnan(x[:, f])]) < tiny).all()]
    assert len(denormal_columns) == 32 and all((x[:, f] < 0).any() and (x[:, f] > 0).any() for f in denormal_columns)
    assert np.isinf(x).any(axis=0).sum() >= 3 and np.isnan(x).any(axis=0).sum() >= 3
    assert sum(c[-1] == np.inf for c in cuts) >= 2 and np.unique(x[:, 1]).shape[0] == 255


@pytest.mark.parametrize("name", FORESTS)
def test_key_walk_reproduces_every_oracle_walk(oracle, name):
    forest, rows = forest_and_rows(name)
    leaves, counts = vc.key_walk(forest, rows)
    sums = vc.leaf_sums(forest, leaves)
    assert len(np.unique(sums)) > 20
    margins, _ = oracle.forest_predict(forest, rows)
    assert same_bits(margins, np.float32(0.0) + sums)                                  # the C oracle
    assert same_bits(continued.leaf_sums(forest, rows), sums)
    assert same_bits(inspected.leaf_sums(forest, rows), sums)
    for t in range(leaves.shape[0]):
        assert np.array_equal(refreshed.walk(forest, t, rows), leaves[t]), t
    assert np.array_equal(cc.node_counts(forest, rows), counts)
    roots = forest["tree_offsets"][:-1]
    assert (counts[roots] == rows.shape[0]).all()


# ---- the cases are what they claim ------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_bin", [256, 16])
def test_oracle_trees_split_on_denormals_zeros_and_infinity(max_bin):
    forest = vc.oracle_trained(max_bin)
    denormal, zero, infinite = vc.threshold_census(forest)
    print(f"max_bin {max_bin}: {denormal} denormal thresholds, {zero} equal to 0.0, {infinite} equal to +inf")
    assert forest["tree_offsets"].shape[0] - 1 == 12 and max(vc.tree_depths(forest)) == 4
    assert denormal >= 20 and zero >= 5 and infinite >= 5
    # every split threshold is met by an evaluation row on it, one step below it and one step above it
    h = vc.hostile_matrix(max_bin)
    split = forest["feature"] >= 0
    for f, cut in set(zip(forest["feature"][split].tolist(), forest["threshold"][split].tolist())):
        cut = np.float32(cut)
        column = vc.key(h.extra[:, f])
        for value in (cut, np.nextafter(cut, np.float32(-np.inf)), np.nextafter(cut, np.float32(np.inf))):
            assert (column == vc.key(value)).any(), (f, cut, value)
        assert h.extra[:, f].view(np.uint32).tolist().count(int(cut.view(np.uint32))) >= vc.REPLICAS


def branch_reach(forest, rows):
    """int64[n_nodes, 3]: the rows that leave each inner node through `yes`, `no` and `missing` (by value, so a NaN
    counts under `missing` only)."""
    out = np.zeros((forest["feature"].shape[0], 3), np.int64)
    for t in range(forest["tree_offsets"].shape[0] - 1):
        begin, end = int(forest["tree_offsets"][t]), int(forest["tree_offsets"][t + 1])
        reach = {begin: np.arange(rows.shape[0])}
        for node in range(begin, end):                                   # children come after their parent
            if forest["feature"][node] < 0:
                continue
            here = reach.pop(node)
            value = rows[here, forest["feature"][node]]
            nan = vc.is_nan(value)
            yes = vc.below(value, np.full(value.shape, forest["threshold"][node], np.float32))
            no = ~nan & ~yes
            out[node] = yes.sum(), no.sum(), nan.sum()
            to_yes = forest["missing"][node] == forest["yes"][node]
            reach[begin + int(forest["yes"][node])] = here[yes | (nan & to_yes)]
            reach[begin + int(forest["no"][node])] = here[no | (nan & ~to_yes)]
    return out


def test_hostile_forest_is_reached_through_every_branch():
    forest, rows = vc.hostile_forest(0), vc.hostile_matrix(256).rows
    assert forest["feature"].max() <= 21 and max(vc.tree_depths(forest)) == 6 and forest["base_margin"] == 0.0
    inner = np.flatnonzero(forest["feature"] >= 0)
    tree_of = np.searchsorted(forest["tree_offsets"], inner, side="right") - 1
    begin = forest["tree_offsets"][tree_of]
    yes, no, missing = (begin + forest[key][inner] for key in ("yes", "no", "missing"))
    assert (yes != no).all() and ((missing == yes) | (missing == no)).all()              # proper binary trees
    assert (yes > inner).all() and (no > inner).all()
    assert 0.3 < (missing == yes).mean() < 0.7                                           # `missing` to either side
    reach = branch_reach(forest, rows)[inner]
    cut = forest["threshold"][inner]
    barren = np.isnan(cut) | (cut == -np.inf)          # THE exceptions: no value is below a NaN or a -inf threshold
    assert barren.sum() >= 4 and np.isnan(cut).sum() >= 2 and (cut == -np.inf).sum() >= 2
    assert (reach[barren, 0] == 0).all()
    assert (reach[~barren, 0] > 0).all() and (reach[:, 1] > 0).all() and (reach[:, 2] > 0).all()
    denormal, zero, infinite = vc.threshold_census(forest)
    assert denormal >= 20 and zero >= 5 and infinite >= 1 and (np.abs(cut) == vc.FLT_MAX).any()
    assert (cut.view(np.uint32) == 0x80000000).any() and (cut.view(np.uint32) == 0).any()   # -0.0 and +0.0


def test_hostile_forest_paths_merge_bounds_and_rows_sit_on_them():
    forest, rows = vc.hostile_forest(0), vc.hostile_matrix(256).rows
    bounds = vc.merged_bounds(forest)
    assert max(splits for _, _, _, splits in bounds) >= 3                  # one feature three times on a path
    both = 0                                                               # `< +inf` and `>= -inf` on one feature
    for path in vc.paths(forest):
        taken = {(int(forest["feature"][node]), float(forest["threshold"][node]), went_yes) for node, went_yes in path}
        both += any((f, np.inf, True) in taken and (f, -np.inf, False) in taken for f in range(22))
    assert both >= 2
    on_lo = on_hi = 0
    for f, lo, hi, splits in bounds:
        if splits < 2 or lo is None or hi is None:
            continue
        column = vc.key(rows[:, f])
        on_lo += int((column == vc.key(np.float32(lo))).any())
        on_hi += int((column == vc.key(np.float32(hi))).any())
    print(f"merged elements with a row exactly on lo: {on_lo}, exactly on hi: {on_hi}")
    assert on_lo >= 5 and on_hi >= 5
