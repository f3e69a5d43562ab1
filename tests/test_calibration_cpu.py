"""Calibration, the parts that need no GPU ("Calibration"): the oracle's stack pooling against the
definition fit_i = max over a <= i of min over b >= i of mean(a .. b) in exact fractions, the properties of the step
map, raw_threshold against the map on every float32 neighbour of every edge, the Calibrator's host side, the report's
derived numbers, validate_calibration's refusals and the declarations."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import calibration_cases as cases
import calibration_oracle as oracle
from doppel_speller_amd import _lib
from doppel_speller_amd import calibration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT_CASES = cases.fit_cases()
QS = (0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99, 0.999999)


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was called before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", refuse)


def calibrator_of(fitted):
    return calibration.Calibrator(fitted["lo"], fitted["hi"], fitted["pos"], fitted["neg"], fitted["n_nan"])


def check_against_the_definition(scores, target, what):
    keys, pos, neg, _ = oracle.points(scores, target)
    fitted = oracle.fit(scores, target)
    want = oracle.brute_force(pos, neg)
    first = np.searchsorted(keys, oracle.cut_key(fitted["lo"]))
    last = np.searchsorted(keys, oracle.cut_key(fitted["hi"]))
    got = [None] * len(want)
    for k in range(first.shape[0]):
        value = Fraction(int(fitted["pos"][k]), int(fitted["pos"][k] + fitted["neg"][k]))
        for point in range(first[k], last[k] + 1):
            assert got[point] is None, what
            got[point] = value
    assert got == want, what
    values = [Fraction(int(p), int(p + q)) for p, q in zip(fitted["pos"], fitted["neg"])]
    assert all(a < b for a, b in zip(values, values[1:])), what
    assert int(fitted["pos"].sum() + fitted["neg"].sum()) + fitted["n_nan"] == scores.shape[0], what


def test_the_oracle_is_the_isotonic_fit_on_every_small_case():
    checked = 0
    for name, (scores, target) in FIT_CASES.items():
        if oracle.points(scores, target)[0].shape[0] <= 300:
            check_against_the_definition(scores, target, name)
            checked += 1
    assert checked >= 20


def test_the_oracle_is_the_isotonic_fit_on_random_inputs():
    rng = np.random.default_rng(11)
    for trial in range(200):
        n = int(rng.integers(1, 60))
        scores = rng.integers(0, int(rng.integers(1, 30)), n).astype(np.float32) - np.float32(7)
        target = (rng.random(n) < rng.random()).astype(np.float32)
        if trial % 5 == 0:
            scores[rng.random(n) < 0.2] = np.nan
        check_against_the_definition(scores, target, trial)


def test_the_key_order_is_the_order_of_the_values():
    values = np.array([-np.inf, -cases.FLT_MAX, -1.0, -cases.DENORMAL, 0.0, cases.DENORMAL, 1.0, cases.FLT_MAX, np.inf],
                      dtype=np.float32)
    keys = oracle.cut_key(values)
    assert (np.diff(keys.astype(np.int64)) > 0).all()
    assert oracle.key_value(keys).tobytes() == values.tobytes()
    assert oracle.cut_key(np.float32(-0.0)) == oracle.cut_key(np.float32(0.0))
    assert oracle.cut_key(np.array([np.nan, -np.nan], np.float32)).tolist() == [oracle.NAN_KEY] * 2
    assert calibration.cut_key(values).tobytes() == keys.tobytes()


@pytest.mark.parametrize("name", sorted(FIT_CASES))
def test_the_map_is_a_non_decreasing_look_up(name):
    scores, _ = FIT_CASES[name]
    fitted = oracle.fit(scores, FIT_CASES[name][1])
    c = calibrator_of(fitted)
    assert c.values.tobytes() == oracle.values(fitted["pos"], fitted["neg"]).tobytes()
    assert c.transform(fitted["lo"]).tobytes() == c.values32().tobytes()
    assert c.transform(fitted["hi"]).tobytes() == c.values32().tobytes()
    probes = np.concatenate([scores, oracle.neighbours(fitted["lo"]), oracle.neighbours(fitted["hi"]),
                             np.array([np.inf, -np.inf, 0.0, -0.0], np.float32)])
    mapped = c.transform(probes)
    assert mapped.tobytes() == oracle.transform(fitted["lo"], c.values, probes).tobytes()
    assert np.isnan(mapped[np.isnan(probes)]).all()
    real = ~np.isnan(probes)
    if len(c):
        assert not np.isnan(mapped[real]).any()
        order = np.argsort(oracle.cut_key(probes[real]), kind="stable")
        assert (np.diff(mapped[real][order]) >= 0).all()
        assert (mapped[real][oracle.cut_key(probes[real]) < oracle.cut_key(fitted["lo"][:1])[0]] == 0).all()
    else:
        assert np.isnan(mapped).all()


@pytest.mark.parametrize("name", sorted(FIT_CASES))
def test_raw_threshold_cuts_where_the_calibrated_value_does(name):
    """score > raw_threshold(q) exactly where transform(score) > q, on every float32 neighbour of every edge.  The two
    saturated answers are the rule's: -FLT_MAX when block 0 qualifies (then for the scores from lo[0] on that are above
    -FLT_MAX) and +FLT_MAX when no block does (then for the scores up to FLT_MAX)."""
    fitted = oracle.fit(*FIT_CASES[name])
    c = calibrator_of(fitted)
    probes = np.concatenate([oracle.neighbours(fitted["lo"]), oracle.neighbours(fitted["hi"]), FIT_CASES[name][0]])
    probes = probes[~np.isnan(probes)]
    for q in QS:
        t = c.raw_threshold(q)
        assert isinstance(t, np.float32)
        assert t.tobytes() == np.float32(oracle.raw_threshold(fitted["lo"], c.values, q)).tobytes()
        if t == -cases.FLT_MAX:
            asked = probes[(oracle.cut_key(probes) >= oracle.cut_key(fitted["lo"][:1])[0]) & (probes > -cases.FLT_MAX)]
        elif t == cases.FLT_MAX:
            asked = probes[probes <= cases.FLT_MAX]
        else:
            asked = probes
        with np.errstate(invalid="ignore"):
            assert np.array_equal(asked > t, c.transform(asked).astype(np.float64) > q), (name, q)


def test_save_and_load_round_trip(tmp_path):
    fitted = oracle.fit(*FIT_CASES["extremes"])
    c = calibration.Calibrator(fitted["lo"], fitted["hi"], fitted["pos"], fitted["neg"], 3, kind="margin")
    path = str(tmp_path / "calibrator.npz")
    c.save(path)
    back = calibration.Calibrator.load(path)
    assert back == c and back.kind == "margin" and back.n_nan == 3 and back.n_rows == c.n_rows
    assert back.values.tobytes() == c.values.tobytes()
    assert back != calibration.Calibrator(fitted["lo"], fitted["hi"], fitted["pos"], fitted["neg"], 3)
    assert back != calibration.Calibrator(fitted["lo"], fitted["hi"], fitted["pos"] + 1, fitted["neg"], 3, "margin")
    empty = calibration.Calibrator([], [], [], [])
    empty.save(path)
    assert calibration.Calibrator.load(path) == empty and len(empty) == 0
    assert list(c.frame().columns) == ["lo", "hi", "pos", "neg", "value"] and len(c.frame()) == len(c)


def test_the_report_derives_its_numbers_from_the_integers():
    probabilities = np.array([0.05, 0.15, 0.15, 0.95, 0.95, 0.95, 0.95, 2.0], np.float32)
    target = np.array([0, 0, 1, 1, 1, 1, 0, 1], np.float32)
    report = calibration.ReliabilityReport(oracle.reliability(probabilities, target, 10))
    assert (report.n, report.n_outside, report.n_bins) == (7, 1, 10)
    p, y = probabilities[:7].astype(np.float64), target[:7].astype(np.float64)
    assert report.brier == pytest.approx(((p - y) ** 2).mean(), abs=2.0 ** -30)
    gaps = {0: abs(0 - p[0]), 1: abs(0.5 - p[1]), 9: abs(0.75 - p[3])}
    assert report.ece == pytest.approx((1 * gaps[0] + 2 * gaps[1] + 4 * gaps[9]) / 7, abs=1e-8)
    assert report.mce == pytest.approx(max(gaps.values()), abs=1e-8)
    frame = report.frame()
    assert list(frame.columns) == ["low", "high", "rows", "positives", "mean_prediction", "observed_rate"]
    assert frame["rows"].tolist() == [1, 2, 0, 0, 0, 0, 0, 0, 0, 4] and np.isnan(frame["observed_rate"][2])
    empty = calibration.ReliabilityReport(np.zeros((11, 4), np.int64))
    assert empty.n == 0 and np.isnan(empty.ece) and np.isnan(empty.brier)


def test_validate_calibration_refuses_what_the_rule_does_not_cover(no_library):
    validate = calibration.validate_calibration
    good = validate(scores=[0.5, np.nan, np.inf], target=[1, 0, 2], n_bins=256, q=0.0)
    assert good["scores"].dtype == np.float32 and good["target"].dtype == np.float32 and good["n"] == 3
    for arguments in (dict(scores=[[0.5]], target=[1]), dict(scores=[0.5, 0.1], target=[1]),
                      dict(scores=[0.5], target=[[1]]), dict(scores=["a"], target=[1]), dict(scores=[0.5], target=[np.nan]),
                      dict(scores=[0.5], target=[np.inf]), dict(scores=[0.5], n=2), dict(n=-1), dict(n=1 << 31),
                      dict(n=1.5), dict(n=True), dict(n_bins=0), dict(n_bins=257), dict(n_bins=2.0), dict(n_bins=True),
                      dict(q=1.0), dict(q=-0.1), dict(q=np.nan), dict(q="x"), dict(q=None)):
        with pytest.raises(ValueError):
            validate(**arguments)
    with pytest.raises(ValueError):
        calibration.fit_isotonic([0.5], [np.nan])
    with pytest.raises(ValueError):
        calibration.fit_isotonic([0.5], None)
    with pytest.raises(ValueError):
        calibration.reliability([0.5], [1], n_bins=300)
    with pytest.raises(ValueError):
        calibration.fit_isotonic_device(None, 3, None)
    with pytest.raises(ValueError):
        calibration.Calibrator([0.1], [0.2], [1], [1]).raw_threshold(1.0)
    with pytest.raises(ValueError):
        calibration.Calibrator([0.1], [0.2, 0.3], [1], [1])
    with pytest.raises(ValueError):
        calibration.Calibrator([0.1], [0.2], [0], [0])


def test_the_surface_validates_before_any_device_work(no_library):
    import types
    import doppel_speller_amd as ds
    model = types.SimpleNamespace(n_features=3, device=0, handle=1)
    with pytest.raises(ValueError):
        ds.ForestModel.calibrate(model, np.zeros((2, 4), np.float32), [0, 1])
    with pytest.raises(ValueError):
        ds.ForestModel.calibrate(model, np.zeros((2, 3), np.float32), [0, np.nan])
    with pytest.raises(ValueError):
        ds.ForestModel.calibrate(model, np.zeros((2, 3), np.float32), [0])
    with pytest.raises(ValueError):
        ds.ForestModel.calibrate_device(model, None, 2, None)
    with pytest.raises(ValueError):
        ds.train_model(["a"], [1], ["a"], [1], calibrate=1)
    with pytest.raises(ValueError):
        ds.train_model(["a"], [1], ["a"], [1], calibrate=True, reliability_bins=0)
    with pytest.raises(ValueError):
        ds.Prediction(["abc"], [1], types.SimpleNamespace(predict_device=None), top_n=1, calibrator=object())


def test_the_entries_are_declared_exported_and_built():
    import doppel_speller_amd as ds
    with open(os.path.join(ROOT, "include", "doppel_amd.h")) as handle:
        header = handle.read()
    for name in ("ds_isotonic_fit_device", "ds_isotonic_fit", "ds_calibration_apply_device", "ds_reliability_device",
                 "ds_calibrate_option"):
        assert re.search(rf"^int {name}\(const ", header, re.M), name
        assert name in _lib.EXPORTED_SYMBOLS
    assert len(set(_lib.EXPORTED_SYMBOLS)) == len(_lib.EXPORTED_SYMBOLS)
    assert "ds_calibrate.hip" in _lib._SOURCES and len(set(_lib._SOURCES)) == len(_lib._SOURCES)
    assert "segment_points" in header and "max_blocks" in header
    for name in ("Calibrator", "ReliabilityReport", "fit_isotonic", "fit_isotonic_device", "reliability",
                 "reliability_device", "validate_calibration"):
        assert hasattr(ds, name), name
    assert callable(ds.ForestModel.calibrate) and callable(ds.ForestModel.calibrate_device)
    # the library builds for gfx950 here and exports the entries
    path = _lib.build_library()
    assert _lib.binary_id(path) == _lib.source_id()
    with open(path, "rb") as handle:
        image = handle.read()
    for name in ("ds_isotonic_fit_device", "ds_calibration_apply_device", "ds_reliability_device"):
        assert name.encode() + b"\0" in image, name
