"""Edit scripts and the learned misspelling model on the GPU ("Edit scripts and the learned
misspelling model"; csrc/ds_edits.hip): distances, scripts, lengths and every count of ds_edit_align and every title of
ds_misspell_titles_profile byte for byte against the restatement of the rule (tests/edit_oracle.py)."""
import ctypes
import os

import numpy as np
import pytest

import edit_cases as cases
import edit_oracle as eo
import training_set_oracle as ts

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POISON = 0x5A


def _strings(array):
    return [bytes(x).decode("utf-8") for x in array]


def _expected_features(oracle, queries, truth_titles, truth_rows, n_truth):
    """oracle.construct_features of (query title i, truth title truth_rows[i])."""
    import doppel_speller_amd as ds
    from doppel_speller_amd.feature_engineering import truth_word_counts
    from doppel_speller_amd.prediction import _pack
    q_enc, q_len = ds.encode_titles(queries)
    t_enc, t_len = ds.encode_titles(truth_titles)
    chars, offsets = _pack(truth_titles)
    counts = truth_word_counts(chars, offsets, separators=(ord(" "),))
    rows = np.asarray(truth_rows, dtype=np.int64)
    return oracle.construct_features(q_len, t_len[rows], q_enc, t_enc[rows], counts[rows], ds.SPACE_CODE, n_truth)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _table(titles):
    import doppel_speller_amd as ds
    enc, lengths = ds.encode_titles(titles)
    return ds.TitleTable(enc, lengths, None, 0)


def _align(truth, truth_rows, observed, observed_rows, n, max_edits, counts=None, want=("distance", "ops", "lengths", "counts"),
           status=0):
    """ds_edit_align into poisoned outputs -> dict of host arrays (an output not in `want` is passed as NULL)."""
    from doppel_speller_amd import _lib
    host = {"distance": np.full(max(n, 1), 0x5A5A5A5A, np.int32), "ops": np.full((max(n, 1), 512), POISON, np.uint8),
            "lengths": np.full(max(n, 1), 0x5A5A5A5A, np.int32),
            "counts": np.zeros(eo.COUNTS, np.int64) if counts is None else counts}
    device = {name: _lib.DeviceArray.from_host(array) for name, array in host.items()}
    rows = [None if r is None else _lib.DeviceArray.from_host(np.asarray(r, dtype=np.int32)) for r in (truth_rows, observed_rows)]
    got = _lib.lib().ds_edit_align(truth.handle, _lib.pointer(rows[0]), observed.handle, _lib.pointer(rows[1]), n, max_edits,
                                   *(_lib.pointer(device[name] if name in want else None)
                                     for name in ("distance", "ops", "lengths", "counts")))
    assert got == status, _lib.lib().ds_last_error()
    return {name: array.to_host() for name, array in device.items()}


def _expect(truth, truth_rows, observed, observed_rows, max_edits, counts=None):
    distance, ops, lengths, counts = eo.align_batch([cases.codes(t) for t in truth], truth_rows,
                                                    [cases.codes(t) for t in observed], observed_rows, max_edits, counts)
    return {"distance": distance, "ops": ops, "lengths": lengths, "counts": counts}


def _same(got, expected, n=None):
    for name in ("distance", "ops", "lengths", "counts"):
        a, b = (got[name], expected[name]) if name == "counts" or n is None else (got[name][:n], expected[name][:n])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (name, np.nonzero(a.reshape(-1) != b.reshape(-1))[0][:8])


def _check_pairs(pairs, max_edits):
    truth, observed = [p[0] for p in pairs], [p[1] for p in pairs]
    got = _align(_table(truth), None, _table(observed), None, len(pairs), max_edits)
    expected = _expect(truth, None, observed, None, max_edits)
    _same(got, expected)
    return got


def test_hand_written_pairs():
    got = _check_pairs(cases.DEVICE_HAND_PAIRS, 4)
    for i, (_, _, distance, script) in enumerate(cases.DEVICE_HAND_PAIRS):
        assert got["distance"][i] == distance and got["ops"][i, :got["lengths"][i]].tolist() == script
        assert not got["ops"][i, got["lengths"][i]:].any()


def test_length_edges():
    pairs = cases.length_edge_pairs()
    lengths = {(len(a), len(b)) for a, b in pairs}
    assert {(3, 3), (3, 255), (255, 3), (255, 255)} <= lengths
    assert {n for pair in lengths for n in pair} >= {63, 64, 65, 127, 128, 129, 191, 192, 193, 254, 255}
    got = _check_pairs(pairs, 4)
    assert got["distance"][3] == 0 and got["distance"][4] == 255 and got["lengths"][4] == 255     # equal; disjoint
    assert got["distance"][1] >= 252 and got["counts"][eo.SKIPPED] > 0 and got["counts"][eo.COUNTED] > 0


@pytest.mark.parametrize("max_edits", [0, 4, 32])
def test_max_edits_at_and_above(max_edits):
    pairs = cases.max_edits_pairs()
    got = _check_pairs(pairs, max_edits)
    assert got["distance"].tolist() == [0, 4, 5, 32, 33]
    assert got["counts"][eo.COUNTED] == sum(d <= max_edits for d in (0, 4, 5, 32, 33))
    assert got["counts"][eo.SKIPPED] == sum(d > max_edits for d in (0, 4, 5, 32, 33))


@pytest.fixture(scope="module")
def fixture():
    """The 380 labelled pairs of training_rows.npz through row arrays that are a permutation with repeats."""
    import doppel_speller_amd as ds
    truth, train, truth_rows, labelled = cases.fixture_pairs(ds.transform_titles)
    rng = np.random.RandomState(3)
    pick = np.concatenate((rng.permutation(len(labelled)), rng.randint(0, len(labelled), 120)))
    truth_rows, train_rows = np.asarray(truth_rows)[pick], np.asarray(labelled)[pick]
    expected = _expect(truth, truth_rows, train, train_rows, 4)
    return dict(truth=truth, train=train, truth_rows=truth_rows, train_rows=train_rows, expected=expected,
                truth_table=_table(truth), train_table=_table(train), n=pick.shape[0])


def test_fixture_pairs_through_row_arrays(fixture):
    f = fixture
    got = _align(f["truth_table"], f["truth_rows"], f["train_table"], f["train_rows"], f["n"], 4)
    _same(got, f["expected"])
    assert got["counts"][eo.COUNTED] + got["counts"][eo.SKIPPED] == f["n"] == 500
    assert got["counts"][eo.SKIPPED] > 40


@pytest.mark.parametrize("pairs_per_group, max_blocks", [(1, 1), (2, 3), (3, 0), (16, 2), (0, 65536)])
def test_launch_geometry_changes_nothing(fixture, pairs_per_group, max_blocks):
    from doppel_speller_amd.edits import edit_option
    f = fixture
    try:
        edit_option("pairs_per_group", pairs_per_group)
        edit_option("max_blocks", max_blocks)
        got = _align(f["truth_table"], f["truth_rows"], f["train_table"], f["train_rows"], f["n"], 4)
    finally:
        edit_option("pairs_per_group", 0)
        edit_option("max_blocks", 0)
    _same(got, f["expected"])


def test_two_calls_add_into_one_block(fixture):
    f = fixture
    first = _align(f["truth_table"], f["truth_rows"][:200], f["train_table"], f["train_rows"][:200], 200, 4)
    both = _align(f["truth_table"], f["truth_rows"][200:], f["train_table"], f["train_rows"][200:], f["n"] - 200, 4,
                  counts=first["counts"])
    assert both["counts"].tobytes() == f["expected"]["counts"].tobytes()
    assert not np.array_equal(first["counts"], both["counts"])


def test_every_output_left_out_in_turn(fixture):
    f = fixture
    for want in (("ops", "lengths", "counts"), ("distance", "counts"), ("distance", "ops", "lengths"), ("counts",), ()):
        got = _align(f["truth_table"], f["truth_rows"], f["train_table"], f["train_rows"], f["n"], 4, want=want)
        for name in ("distance", "ops", "lengths"):
            if name in want:
                assert got[name].tobytes() == f["expected"][name].tobytes(), (want, name)
            else:
                assert (got[name].view(np.uint8) == POISON).all(), (want, name)
        assert got["counts"].tobytes() == (f["expected"]["counts"] if "counts" in want else eo.new_counts()).tobytes()


def test_no_pair_and_one_pair(fixture):
    f = fixture
    got = _align(f["truth_table"], f["truth_rows"], f["train_table"], f["train_rows"], 0, 4)
    assert (got["distance"].view(np.uint8) == POISON).all() and (got["ops"] == POISON).all() and not got["counts"].any()
    got = _align(f["truth_table"], f["truth_rows"], f["train_table"], f["train_rows"], 1, 4)
    _same(got, _expect(f["truth"], f["truth_rows"][:1], f["train"], f["train_rows"][:1], 4), 1)
    assert (got["distance"][1:].view(np.uint8) == POISON).all()


def test_argument_errors_leave_the_outputs_alone(fixture):
    from doppel_speller_amd import _lib
    import doppel_speller_amd as ds
    f = fixture
    n = f["n"]
    enc, lengths = ds.encode_titles(["abc", "abcd", "abcde"])
    short, zero, high = lengths.copy(), enc.copy(), enc.copy()
    short[1] = 2
    zero[2, 1] = 0
    high[0, 2] = 38
    good = ds.TitleTable(enc, lengths, None, 0)
    bad_tables = [ds.TitleTable(enc, short, None, 0), ds.TitleTable(zero, lengths, None, 0), ds.TitleTable(high, lengths, None, 0)]
    calls = [dict(max_edits=-1), dict(max_edits=33), dict(n=-1), dict(want=("distance", "ops", "counts")),
             dict(want=("distance", "lengths", "counts")),
             dict(truth_rows=np.where(np.arange(n) == 77, 3000, f["truth_rows"])),          # one row past the table
             dict(train_rows=np.where(np.arange(n) == n - 1, -1, f["train_rows"]))]
    for call in calls:
        arguments = dict(truth_rows=f["truth_rows"], train_rows=f["train_rows"], n=n, max_edits=4,
                         want=("distance", "ops", "lengths", "counts"))
        arguments.update(call)
        got = _align(f["truth_table"], arguments["truth_rows"], f["train_table"], arguments["train_rows"], arguments["n"],
                     arguments["max_edits"], want=arguments["want"], status=-1)
        assert all((got[name].view(np.uint8) == POISON).all() for name in ("distance", "ops", "lengths")), call
        assert not got["counts"].any(), call
    for table in bad_tables:
        for truth, observed in ((table, good), (good, table)):
            got = _align(truth, None, observed, None, 3, 4, status=-1)
            assert all((got[name].view(np.uint8) == POISON).all() for name in ("distance", "ops", "lengths"))
            assert not got["counts"].any() and b"transformed" in _lib.lib().ds_last_error()
    p = _lib.pointer(None)
    assert _lib.lib().ds_edit_align(p, p, good.handle, p, 1, 4, p, p, p, p) == -1
    assert _lib.lib().ds_edit_option(b"no_such_option", 1) == -1 and _lib.lib().ds_edit_option(b"pairs_per_group", 17) == -1


def test_python_entry_points_equal_the_oracle(fixture):
    import doppel_speller_amd as ds
    f = fixture
    truth = [f["truth"][r] for r in f["truth_rows"][:380]]
    train = [f["train"][r] for r in f["train_rows"][:380]]
    expected = _expect(truth, None, train, None, 4)
    scripts = ds.edit_operations(truth, train, transform=False)
    assert scripts.distance.tobytes() == expected["distance"].tobytes() and scripts.ops.tobytes() == expected["ops"].tobytes()
    assert scripts.lengths.tobytes() == expected["lengths"].tobytes()
    frame = scripts.frame()
    assert frame.shape[0] == int(sum((expected["ops"][i, :expected["lengths"][i]] != 0).sum() for i in range(380)))
    changed = int(np.nonzero(scripts.distance == 1)[0][0])
    assert scripts.render(changed).count("^") >= 1 and scripts.render(changed).split("\n")[2].strip("^ ") == ""
    profile = ds.fit_misspelling_profile(truth, train, transform=False)
    assert profile.counts.tobytes() == expected["counts"].tobytes() and profile.counted + profile.skipped == 380
    assert profile.max_edits == 4 and ds.fit_misspelling_profile([], []).counted == 0
    print("fixture at max_edits = 4:", profile.counted, "counted,", profile.skipped, "skipped; edits per title",
          profile.edits_per_title(), "; shares", profile.operation_shares(), "; keyboard share", profile.keyboard_share())


# ---- the generator -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    import doppel_speller_amd as ds
    counts = cases.fixture_profile(ds.transform_titles)
    return ds.MisspellingProfile(counts, 4), eo.Profile(counts)


def test_generator_equals_the_oracle(fitted):
    import doppel_speller_amd as ds
    from doppel_speller_amd.training_set import misspell_table
    profile, oracle = fitted
    titles = _strings(np.load(os.path.join(GOLDEN, "misspell_cases.npz"))["titles"])
    assert len(titles) == 2040 and max(len(t) for t in titles) == 255
    seed = 2 ** 63 + 12345
    got = ds.generate_misspelled_names(titles, seed=seed, profile=profile)
    expected = [eo.misspell_profile(title, seed, row, oracle) for row, title in enumerate(titles)]
    bad = [i for i in range(len(titles)) if got[i] != expected[i]]
    assert not bad, [(titles[i], got[i], expected[i]) for i in bad[:5]]
    assert all(3 <= len(t) <= 255 and set(t) <= set(ts.ALPHABET[1:]) for t in got)
    assert sum(a != b for a, b in zip(got, titles)) > 0.9 * len(titles)
    assert got != ds.generate_misspelled_names(titles, seed=seed) and \
        ds.generate_misspelled_names(titles[:200], seed=seed + 1, profile=profile) != got[:200]
    # a function of (seed, source row) alone: a subset through d_rows puts the titles on other lanes and workgroups
    table = _table(titles)
    rows = np.random.RandomState(5).permutation(len(titles))[:777]
    subset = misspell_table(table, rows, seed, profile=profile)
    enc, lengths = subset.read()
    assert subset.strings() == [got[r] for r in rows]
    assert all(not enc[i, lengths[i]:].any() for i in range(rows.shape[0]))          # zero-filled behind the title


def test_generator_with_all_rates_zero_and_its_refusals(fitted):
    import doppel_speller_amd as ds
    from doppel_speller_amd import _lib
    from doppel_speller_amd.training_set import misspell_table
    titles = _strings(np.load(os.path.join(GOLDEN, "misspell_cases.npz"))["titles"])[-300:]
    nothing = eo.new_counts()
    nothing[eo.EDITS + 2] = 5
    nothing[eo.SEEN:eo.SEEN + eo.CODES] = 100
    transformed = [ts.to_text(ts.transform_codes(ts.to_codes(title))) for title in titles]
    assert ds.generate_misspelled_names(titles, seed=1, profile=ds.MisspellingProfile(nothing)) == transformed
    # the library's own check of the block (validate_misspelling_profile is the Python twin)
    table = _table(titles)
    for index, value in ((eo.EDITS + 2, 0), (7, -1), (eo.SUBSTITUTED + 2 * eo.CODES + 2, 1), (eo.DELETED + 5, 400),
                         (eo.INSERTED + 3 * eo.CODES, 1), (eo.SEEN + 3, 1 << 40)):
        block = nothing.copy()
        block[index] = value
        d_block = _lib.DeviceArray.from_host(block)
        handle = ctypes.c_void_p(1)
        assert _lib.lib().ds_misspell_titles_profile(table.handle, None, len(titles), ctypes.c_uint64(0), d_block.ptr,
                                                     ctypes.byref(handle)) == -1, (index, value)
        assert handle.value is None
    enc = np.zeros((3, 255), dtype=np.uint8)
    enc[:, :4] = [2, 3, 1, 4]
    short = ds.TitleTable(enc, np.array([4, 2, 4], dtype=np.uint8), None, 0)
    assert len(misspell_table(short, [0, 2], 0, profile=fitted[0]).strings()) == 2
    for rows in ([0, 1], [0, 3]):
        with pytest.raises(_lib.DoppelError, match="out of range or not transformed"):
            misspell_table(short, rows, 0, profile=fitted[0])


# ---- FeatureEngineering and train_model ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engineering(fitted):
    import doppel_speller_amd as ds
    g = dict(np.load(os.path.join(GOLDEN, "training_rows.npz"), allow_pickle=False))
    arguments = dict(top_n=int(g["top_n"]), sample_n=int(g["sample_n"]), seed=int(g["seed"]),
                     evaluation_fractions={"negative": 0.05})
    titles = (_strings(g["truth_titles"]), g["truth_ids"], _strings(g["train_titles"]), g["train_ids"])
    plain = ds.FeatureEngineering(*titles, **arguments)
    plain_sets = plain.generate_train_and_evaluation_data_sets()
    learned = ds.FeatureEngineering(*titles, misspelling_profile=fitted[0], **arguments)
    learned_sets = learned.generate_train_and_evaluation_data_sets()
    return titles, arguments, plain, plain_sets, learned, learned_sets


def test_feature_engineering_with_a_profile(engineering, fitted, oracle):
    import doppel_speller_amd as ds
    titles, arguments, plain, plain_sets, learned, learned_sets = engineering
    generated = learned.rows["kind"].to_numpy() == ts.KIND_GENERATED
    truth_rows = learned.rows["truth_row"].to_numpy()[generated]
    every = ds.generate_misspelled_names(learned.truth_titles, seed=arguments["seed"], profile=fitted[0])
    assert learned.misspelled_titles == [every[r] for r in truth_rows]
    assert learned.misspelled_titles == [eo.misspell_profile(learned.truth_titles[r], arguments["seed"], int(r), fitted[1])
                                         for r in truth_rows]
    assert learned.misspelled_titles != plain.misspelled_titles
    # kinds 2 and 3 do not depend on the generator
    assert learned.rows.equals(plain.rows)
    assert _same_bits(learned.features[~generated], plain.features[~generated])
    expected = _expected_features(oracle, learned.misspelled_titles, learned.truth_titles, truth_rows, len(learned.truth_titles))
    assert _same_bits(learned.features[generated], expected)
    evaluation = learned.rows["evaluation"].to_numpy()
    assert _same_bits(learned_sets[0], learned.features[~evaluation]) and _same_bits(learned_sets[2], learned.features[evaluation])
    assert "misspell_profile" in learned.timings and "misspell_profile" not in plain.timings
    assert learned.timings["misspell"] == 0.0 and plain.timings["misspell"] > 0.0


def test_feature_engineering_fits_its_own_profile(engineering, fitted):
    import doppel_speller_amd as ds
    titles, arguments, plain, *_ = engineering
    own = plain.fit_misspelling_profile()
    labelled = np.nonzero(np.asarray(titles[3]) >= 0)[0]
    row_of = {int(title_id): row for row, title_id in enumerate(titles[1])}
    from_strings = ds.fit_misspelling_profile([titles[0][row_of[int(titles[3][i])]] for i in labelled],
                                              [titles[2][i] for i in labelled])
    assert own.counts.tobytes() == from_strings.counts.tobytes() == fitted[0].counts.tobytes()
    assert own.counted + own.skipped == 380 and own.max_edits == 4
    assert plain.fit_misspelling_profile(max_edits=0).counted == int(own.edits[0])


def test_train_model_fits_and_returns_the_profile(engineering, fitted):
    import doppel_speller_amd as ds
    titles, arguments, plain, plain_sets, learned, learned_sets = engineering
    result = ds.train_model(*titles, misspelling_profile="fit", num_boost_round=5, **arguments)
    assert isinstance(result.misspelling_profile, ds.MisspellingProfile) and result.model.n_trees >= 1
    assert result.misspelling_profile.counts.tobytes() == fitted[0].counts.tobytes()
    assert result.rows.equals(learned.rows) and result.error_matrix is not None
    assert "misspell_profile" in result.timings and "misspell_profile_fit" in result.timings
    without = ds.train_model(*titles, num_boost_round=5, **arguments)
    assert without.misspelling_profile is None and "misspell_profile" not in without.timings
    result.model.close()
    without.model.close()
