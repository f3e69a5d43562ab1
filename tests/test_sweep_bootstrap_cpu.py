"""The bootstrap of the sweep's cells without a GPU: the oracle of tests/sweep_bootstrap_oracle.py against the oracles it
is built from, the literal records of the crafted queries, validate_sweep_bootstrap, SweepBootstrap's statistics on
hand-made counts, and the C ABI surface."""
import os
import re

import numpy as np
import pytest

import bootstrap_oracle as bo
import sweep_bootstrap_oracle as so
import sweep_cases as sc
from doppel_speller_amd import _lib, bootstrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n_queries, k, grid", [(257, 5, "3x7"), (64, 65, "65x3"), (5, 65, "101x256"), (257, 5, "1x1")])
def test_decoding_the_expected_records_gives_back_the_codes(oracle, n_queries, k, grid):
    c = so.record_case(oracle, n_queries, k, grid)
    U = len(c["prob"])
    assert c["records"].shape == (n_queries, len(c["lev"])) and c["records"].dtype == np.uint16
    assert np.array_equal(so.decode(c["records"], U), c["codes"])
    what, pos = c["records"] & 7, c["records"] >> 3
    assert (what < 7).all() and (pos[what < 4] == 0).all()
    assert ((pos[what >= 4] >= 1) & (pos[what >= 4] <= U - 1)).all()


def test_a_record_with_pos_u_decodes_to_one_code_in_every_cell():
    records = np.array([[4 | (3 << 3), 5 | (3 << 3), 6 | (3 << 3)], [4 | (1 << 3), 5 | (2 << 3), 2]], np.uint16)
    codes = so.decode(records, 3).reshape(3, 3, 2)            # [t][u][q]
    assert codes[:, :, 0].tolist() == [[1, 1, 1], [3, 3, 3], [1, 1, 1]]
    assert codes[:, :, 1].tolist() == [[1, 0, 0], [3, 3, 2], [2, 2, 2]]


@pytest.mark.parametrize("n_queries, k, grid", [(257, 5, "3x7"), (5, 65, "101x256")])
def test_the_baseline_is_the_sweep_counters_renumbered(oracle, n_queries, k, grid):
    c = so.record_case(oracle, n_queries, k, grid)
    T, U = len(c["lev"]), len(c["prob"])
    _, baseline = so.counts(c["codes"], T, U, None, n_queries, 1, 0)
    swept = sc.sweep_counts(oracle, c["queries"], c["lev"], c["prob"])
    assert np.array_equal(baseline, swept[:, :, list(so.SWEEP_COUNTER_OF_CODE)])
    assert so.SWEEP_COUNTER_OF_CODE == tuple(sc.COUNTERS.index(name) for name in bootstrap.ACCURACY_CODES)


def test_the_crafted_queries_have_these_records(oracle):
    """On GRID_3X7 (t = 50, 90, 94; u = 0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99), query by query as
    sweep_cases.crafted_queries describes them."""
    lev, prob = sc.GRID_3X7
    for k in (5, 100):
        queries = sc.crafted_queries(k)
        records = so.records_of(so.cell_codes(oracle, queries, lev, prob), 3, 7)
        assert records.tolist() == [
            [3, 3, 3],                                  # 0: the exact row is the actual one
            [5 | (4 << 3)] * 3,                         # 1: the model's row at 0.8 is right below 0.9: pos 4
            [1, 3, 3],                                  # 2: the wrong candidate wins at 50, the right one at 90 and 94
            [0, 0, 0],                                  # 3: no match, none to find
            [6 | (2 << 3)] * 3,                         # 4: 0.5 is above 0.1 and 0.25 only, and the row is another one
            [1, 1, 1],                                  # 5: a close match for a title that has none
            [3, 6 | (4 << 3), 6 | (4 << 3)],            # 6: the close row at 50; the model's other row below 0.9 after
        ]


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", refuse)


def test_validate_sweep_bootstrap_accepts(no_library):
    v = bootstrap.validate_sweep_bootstrap()
    assert v == dict(n_boot=0, seed=0, unit=None, n_units=0)
    v = bootstrap.validate_sweep_bootstrap(65536, (1 << 63) - 1, None, 10, 2, 256)          # 2^25 exactly
    assert (v["n_boot"], v["seed"], v["unit"], v["n_units"]) == (65536, (1 << 63) - 1, None, 10)
    assert bootstrap.validate_sweep_bootstrap(1297, 0, None, 0, 101, 256)["n_boot"] == 1297  # 33,535,232 <= 2^25
    assert bootstrap.validate_sweep_bootstrap(0, 0, None, 5, 101, 256)["n_boot"] == 0
    v = bootstrap.validate_sweep_bootstrap(5, 3, ["b", "a", "b", "c"], 4)
    assert v["unit"].dtype == np.int32 and v["unit"].tolist() == [0, 1, 0, 2] and v["n_units"] == 3
    v = bootstrap.validate_sweep_bootstrap(5, np.int64(3), np.array([7, 7, -1]), 3, 20, 50)
    assert v["unit"].tolist() == [0, 0, 1] and v["n_units"] == 2 and v["seed"] == 3


@pytest.mark.parametrize("arguments, message", [
    (dict(n_boot=-1), r"n_boot must be an integer in \[0, 65536\]"), (dict(n_boot=65537), "n_boot"),
    (dict(n_boot=2.0), "n_boot"), (dict(n_boot=True), "n_boot"),
    (dict(seed=-1), "seed"), (dict(seed=1 << 63), "seed"), (dict(seed=0.5), "seed"),
    (dict(groups=[1, 2], n_titles=3), "one per title"), (dict(groups=[[1], [2]], n_titles=2), "one per title"),
    (dict(groups=[0.5, 1.5], n_titles=2), "integers or strings"),
    (dict(n_boot=65536, n_levenshtein=2, n_probability=256, n_titles=1, groups=[3, 4]), "one per title"),
    (dict(n_boot=1298, n_levenshtein=101, n_probability=256), r"1298 x 101 x 256 = 33561088 is above 2\^25 = 33554432"),
    (dict(n_boot=32769, n_levenshtein=4, n_probability=256), "32 bytes per replicate and cell, 1073774592 bytes"),
    (dict(n_levenshtein=102), "n_levenshtein"), (dict(n_probability=257), "n_probability"),
    (dict(n_titles=1 << 31), "n_titles"),
])
def test_validate_sweep_bootstrap_refuses(no_library, arguments, message):
    with pytest.raises(ValueError, match=message):
        bootstrap.validate_sweep_bootstrap(**arguments)


def test_threshold_sweep_checks_them_before_the_library(no_library):
    from doppel_speller_amd import prediction
    p = prediction.Prediction.__new__(prediction.Prediction)
    p.truth_title_ids, p.levenshtein_threshold, p.probability_threshold = np.array([10, 20], np.int64), 94, 0.9
    with pytest.raises(ValueError, match="n_boot"):
        p.threshold_sweep(["a"], [10], n_boot=-3)
    with pytest.raises(ValueError, match="one per title"):
        p.evaluate(["a"], [10], n_boot=5, groups=[1, 2])
    with pytest.raises(TypeError):
        p.threshold_sweep(["a"], [10], None, None, None, 5)                   # keyword only


def _hand_made():
    """Three replicates of a 2 x 2 grid.  Errors (code 2 + 5 x code 1), cells 0..3: replicate 0: 10, 10, 12, 15 (cells 0
    and 1 tie), replicate 1: 9, 7, 7, 7 (cells 1, 2 and 3 tie), replicate 2: 20, 11, 12, 13; baseline 8, 6, 6, 9."""
    errors = np.array([[10, 10, 12, 15], [9, 7, 7, 7], [20, 11, 12, 13]])
    baseline = np.array([8, 6, 6, 9])

    def counts_of(e):
        out = np.zeros(e.shape + (4,), np.int64)
        out[..., 1] = e // 5
        out[..., 2] = e % 5
        out[..., 0], out[..., 3] = 3, 100 - out[..., 1] - out[..., 2] - 3
        return out
    return bootstrap.SweepBootstrap(counts_of(errors).reshape(3, 2, 2, 4), counts_of(baseline).reshape(2, 2, 4), [90, 94],
                                    [0.5, 0.9], n_units=100, seed=4, reference=(94, 0.9)), errors, baseline


def test_sweep_bootstrap_statistics_on_hand_made_counts():
    s, errors, baseline = _hand_made()
    assert isinstance(s, bootstrap.ErrorBootstrap) and s.codes == bootstrap.ACCURACY_CODES and s.weight == 5.0
    assert s.names == ("90/0.5", "90/0.9", "94/0.5", "94/0.9") and s.n_sets == 4 and s.n_boot == 3
    assert s.levenshtein_thresholds.tolist() == [90, 94] and s.probability_thresholds.tolist() == [0.5, 0.9]
    assert s.errors.tolist() == errors.tolist() and s.baseline_errors.tolist() == baseline.tolist()
    assert [s.cell(90, 0.5), s.cell(90, 0.9), s.cell(94, 0.5), s.cell(94, np.float32(0.9))] == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="no cell"):
        s.cell(91, 0.5)
    assert s.best() == 1                                                       # 6 twice: the earlier cell
    # replicate 0: half a win each for cells 0 and 1; replicate 1: a third each for 1, 2 and 3; replicate 2: cell 1
    assert np.allclose(s.share_best, np.array([1 / 2, 1 / 2 + 1 / 3 + 1, 1 / 3, 1 / 3]) / 3, rtol=0, atol=1e-15)
    assert abs(s.share_best.sum() - 1.0) < 1e-15 and s.share_best.dtype == np.float64


@pytest.mark.parametrize("reference, level", [(None, 0.95), (1, 0.8), ("90/0.5", 0.95), ((94, 0.5), 0.5)])
def test_against_is_difference_cell_by_cell(reference, level):
    s, _, _ = _hand_made()
    frame = s.against(reference, level)
    at = {None: 3, 1: 1, "90/0.5": 0, (94, 0.5): 2}[reference]                 # None: the instance's own (94, 0.9)
    assert list(frame.columns) == ["levenshtein_threshold", "probability_threshold", "baseline", "mean", "low", "high",
                                   "share_better"]
    assert frame["levenshtein_threshold"].tolist() == [90, 90, 94, 94]
    assert frame["probability_threshold"].tolist() == [0.5, 0.9, 0.5, 0.9]
    for c in range(4):
        d = s.difference(c, at, level)
        line = frame.iloc[c]
        assert (line["baseline"], line["mean"], line["low"], line["high"], line["share_better"]) == \
            (d.baseline, d.mean, d.interval[0], d.interval[1], d.share_better), c
    # the reference cell is the best one when the grid does not hold the instance's thresholds, or there are none
    for other in (bootstrap.SweepBootstrap(s.counts.reshape(3, 2, 2, 4), s.baseline_counts, [90, 94], [0.5, 0.9],
                                           reference=(80, 0.9)),
                  bootstrap.SweepBootstrap(s.counts.reshape(3, 2, 2, 4), s.baseline_counts, [90, 94], [0.5, 0.9])):
        assert other.against()["baseline"].tolist() == (s.baseline_errors - s.baseline_errors[1]).tolist()


def test_the_frame_has_the_sweeps_columns_and_the_bootstraps():
    from doppel_speller_amd import prediction
    s, errors, baseline = _hand_made()
    frame = s.frame(0.9)
    assert tuple(frame.columns) == prediction.SWEEP_COLUMNS + ("mean_error", "standard_error", "low", "high", "share_best")
    plain = prediction.sweep_frame([90, 94], [0.5, 0.9], s.baseline_counts[:, [3, 1, 0, 2]])    # counter j = this code
    for name in prediction.SWEEP_COLUMNS:
        assert frame[name].tolist() == plain[name].tolist(), name
    assert frame["custom_error"].tolist() == baseline.tolist()
    assert frame["mean_error"].tolist() == errors.mean(axis=0).tolist()
    assert frame["standard_error"].tolist() == errors.std(axis=0, ddof=1).tolist()
    assert np.array_equal(frame[["low", "high"]].to_numpy(), s.interval(0.9))
    assert frame["share_best"].tolist() == s.share_best.tolist()


def test_header_declares_the_two_entry_points_without_a_stream():
    header = open(os.path.join(ROOT, "include", "doppel_amd.h")).read()

    def types_of(name):
        declaration = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert declaration, f"{name} is not declared"
        arguments = [a.strip() for a in declaration.group(1).replace("\n", " ").split(",")]
        assert not any("stream" in a for a in arguments), name
        return [a.rsplit(" ", 1)[0] + ("*" if a.rsplit(" ", 1)[1].startswith("*") else "") for a in arguments]

    assert types_of("ds_sweep_records_device") == [
        "const int32_t*", "const uint8_t*", "const uint8_t*", "const uint8_t*", "const float*", "const int32_t*",
        "const int32_t*", "int64_t", "int32_t", "const int32_t*", "int32_t", "const float*", "int32_t", "uint16_t*"]
    assert types_of("ds_sweep_bootstrap_device") == [
        "const uint16_t*", "int64_t", "int32_t", "int32_t", "const int32_t*", "int64_t", "int32_t", "uint64_t", "int64_t*",
        "int64_t*"]
    assert {"ds_sweep_records_device", "ds_sweep_bootstrap_device"} <= set(_lib.EXPORTED_SYMBOLS)
    import stream_cases
    prototypes = stream_cases.header_prototypes(header)
    assert "ds_sweep_records_device" not in prototypes and "ds_sweep_bootstrap_device" not in prototypes
    for name in ("ds_sweep_records_device", "ds_sweep_bootstrap_device"):
        comment = header[:header.index("int " + name)]
        comment = comment[comment.rindex("/*"):]
        assert "No stream parameter" in comment and "null stream" in comment and "synchronises" in comment, name


def test_package_exports():
    import doppel_speller_amd as ds
    assert ds.SweepBootstrap is bootstrap.SweepBootstrap and ds.validate_sweep_bootstrap is bootstrap.validate_sweep_bootstrap
    assert callable(ds.CandidatePipeline.enqueue_sweep_records)
    assert os.path.exists(os.path.join(ROOT, "examples", "sweep_bootstrap.py"))
