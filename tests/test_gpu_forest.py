"""Next row f-4 on the GPU: the tree-ensemble kernel against the oracle restatement (xgboost itself is outside the
reference tree: parity unpinned against the library, bit-exact margins against oracle/doppel_oracle.c)."""
import numpy as np
import pytest

from test_forest_cpu import random_dump, random_rows

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_trees,depth,n", [(1, 1, 5), (60, 6, 10000), (300, 4, 3000)])
def test_forest_kernel_against_oracle(oracle, n_trees, depth, n):
    import doppel_speller_amd as ds
    dump = random_dump(n_trees + depth, n_trees=n_trees, depth=depth)
    model = ds.ForestModel.from_xgboost_dump(dump, 66)
    rows = random_rows(n, n)
    margins, probabilities = oracle.forest_predict(model.arrays, rows)
    assert np.array_equal(model.predict(rows, output_margin=True).view(np.uint32), margins.view(np.uint32))
    got = model.predict(rows)
    assert np.allclose(got, probabilities, rtol=3e-7, atol=0)       # float32 exp: device vs libm, <= 2 ulp
    assert ((got > 0) & (got < 1)).all()


def test_ntree_limit_and_base_score(oracle):
    import doppel_speller_amd as ds
    dump = random_dump(11, n_trees=30)
    rows = random_rows(12, 500)
    limited = ds.ForestModel.from_xgboost_dump(dump, 66, ntree_limit=7, base_score=0.2)
    margins, _ = oracle.forest_predict(limited.arrays, rows)
    assert limited.n_trees == 7
    assert np.array_equal(limited.predict(rows, output_margin=True).view(np.uint32), margins.view(np.uint32))


def test_bad_forests_are_rejected():
    import doppel_speller_amd as ds
    offsets = np.array([0, 3], np.int64)
    feature = np.array([0, -1, -1], np.int32)
    threshold = np.array([0.5, 1.0, 2.0], np.float32)
    ok = dict(yes=np.array([1, 0, 0], np.int32), no=np.array([2, 0, 0], np.int32), missing=np.array([1, 0, 0], np.int32))
    ds.ForestModel(feature, threshold, ok["yes"], ok["no"], ok["missing"], offsets, 66)
    with pytest.raises(ds.DoppelError):                                   # child before its parent: a cycle
        ds.ForestModel(feature, threshold, np.array([0, 0, 0], np.int32), ok["no"], ok["missing"], offsets, 66)
    with pytest.raises(ds.DoppelError):                                   # feature index out of range
        ds.ForestModel(np.array([70, -1, -1], np.int32), threshold, ok["yes"], ok["no"], ok["missing"], offsets, 66)


def test_predictions_inside_the_device_pipeline(oracle):
    import doppel_speller_amd as ds
    from doppel_speller_amd import synth
    w = synth.make_workload(20000, 500, seed=41)
    pipeline = ds.CandidatePipeline(w, 10)
    model = ds.ForestModel.from_xgboost_dump(random_dump(5, n_trees=80), ds.FEATURES_COUNT)
    pipeline.step()
    pipeline.enqueue_predict(model)
    assert pipeline.sync()["error_queries"] == 0
    features = pipeline.features()
    _, probabilities = oracle.forest_predict(model.arrays, features)
    assert np.allclose(pipeline.predictions().reshape(-1), probabilities, rtol=3e-7, atol=0)


def test_forest_kernel_past_one_grid_pass(oracle):
    """ds_forest_predict_device caps its grid at 256 x 16 workgroups of 256 rows: 1,048,576 rows per grid-stride pass.
    2.1M rows take three passes, and the last one ends in a partial workgroup."""
    import doppel_speller_amd as ds
    n = 2_100_000
    assert n > 2 * 4096 * 256 and n % 256 != 0
    model = ds.ForestModel.from_xgboost_dump(random_dump(71, n_trees=60, n_features=8), 8)
    rows = random_rows(72, n, n_features=8)
    margins, probabilities = oracle.forest_predict(model.arrays, rows)
    assert np.array_equal(model.predict(rows, output_margin=True).view(np.uint32), margins.view(np.uint32))
    assert np.allclose(model.predict(rows), probabilities, rtol=3e-7, atol=0)


@pytest.mark.parametrize("nf", [1, 47, 48, 96])
def test_forest_kernel_at_every_lds_layout(oracle, nf):
    """The rows of a workgroup are staged in 256 x (nf + 1) floats of LDS: nf = 47 fills the default 48 KiB exactly,
    nf = 48 is the first size that needs the hipFuncSetAttribute opt-in, 96 (99 KiB) the largest model."""
    import doppel_speller_amd as ds
    lds = 256 * (nf + 1) * 4
    assert (lds > 48 * 1024) == (nf >= 48) and (nf != 47 or lds == 48 * 1024)
    model = ds.ForestModel.from_xgboost_dump(random_dump(80 + nf, n_trees=40, n_features=nf, depth=8), nf)
    assert np.any(model.arrays["feature"] == nf - 1)          # the last staged column is read
    rows = random_rows(90 + nf, 3001, n_features=nf)
    assert np.isnan(rows).any()
    margins, probabilities = oracle.forest_predict(model.arrays, rows)
    assert np.array_equal(model.predict(rows, output_margin=True).view(np.uint32), margins.view(np.uint32))
    assert np.allclose(model.predict(rows), probabilities, rtol=3e-7, atol=0)


def test_forest_without_trees(oracle):
    """ds_forest_create admits a model of zero trees: every margin is the float32 base margin."""
    import doppel_speller_amd as ds
    model = ds.ForestModel.from_trees([], 5, base_margin=0.3)
    assert model.n_trees == 0
    rows = random_rows(3, 700, n_features=5)
    expected = np.full(700, np.float32(0.3))
    margins, probabilities = oracle.forest_predict(model.arrays, rows)
    assert np.array_equal(margins.view(np.uint32), expected.view(np.uint32))
    assert np.array_equal(model.predict(rows, output_margin=True).view(np.uint32), expected.view(np.uint32))
    assert np.allclose(model.predict(rows), probabilities, rtol=3e-7, atol=0)
