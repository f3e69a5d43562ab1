"""The query side of Prediction on the device (ds_prepare_titles, ds_query_rows_device) against the host path it
replaces: transform_titles + encode_collection + check_characters for the titles, query_rows for the Jaccard rows, and
Prediction(prepare_queries="host") for the answers, details and errors."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import doppel_speller_amd as ds
from doppel_speller_amd import _lib, prediction, synth
from doppel_speller_amd.feature_engineering import encode_collection
from doppel_speller_amd.match_maker import NativeProblem
from doppel_speller_amd.prediction import DeviceTitles, QuerySpace, prepare_queries

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALLOWED = set(" abcdefghijklmnopqrstuvwxyz0123456789")


def _prepare_raw(titles, transform):
    """ds_prepare_titles straight through ctypes: (status, enc, lengths, report) whatever the report holds."""
    titles = [t.encode("ascii") for t in titles]
    offsets = np.zeros(len(titles) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in titles], out=offsets[1:])
    chars = np.frombuffer(b"".join(titles) or b"\0", dtype=np.uint8)
    handle, report = ctypes.c_void_p(), np.zeros(4, dtype=np.int64)
    status = _lib.lib().ds_prepare_titles(_lib.pointer(chars), _lib.pointer(offsets), len(titles), int(transform), 0,
                                          None, ctypes.byref(handle), _lib.pointer(report))
    if status != 0:
        return status, None, None, report
    table = DeviceTitles(handle, len(titles), 0)
    enc = np.empty((len(titles), 255), dtype=np.uint8)
    lengths = np.empty(len(titles), dtype=np.uint8)
    _lib.check(_lib.lib().ds_titles_read(table.handle, _lib.pointer(enc), _lib.pointer(lengths)), "ds_titles_read")
    table.close()
    return status, enc, lengths, report


def _mask_bytes(report):
    mask = int(report[0].view(np.uint64)) | (int(report[1].view(np.uint64)) << 64)
    return sorted(b for b in range(128) if (mask >> b) & 1)


def _host_rows(titles):
    """encode_collection + the bytes check_characters refuses, of titles that are already transformed."""
    chars, offsets = prediction._pack(titles)
    enc, lengths = encode_collection(chars, offsets, prediction._CODE_OF)
    used = chars[:int(offsets[-1])]
    return enc, lengths, sorted(set(used[~prediction._ALLOWED[used]].tolist()))


def test_device_transform_matches_the_reference_vectors():
    with open(os.path.join(GOLDEN, "transform_title.json"), encoding="utf-8") as handle:
        vectors = json.load(handle)
    assert len(vectors) >= 300
    clean = [v for v in vectors if set(v["transformed"]) <= ALLOWED]
    table = prepare_queries([v["title"] for v in clean], True)
    assert table.transformed(range(len(clean))) == [v["transformed"] for v in clean]
    refused = [v for v in vectors if not set(v["transformed"]) <= ALLOWED]
    assert refused                       # white space other than ' ' survives transform_title
    for v in refused:
        bad = "".join(sorted(set(v["transformed"]) - ALLOWED))
        with pytest.raises(ValueError) as caught:
            prepare_queries([v["title"]], True)
        assert str(caught.value) == f"query titles hold characters a transformed title cannot hold: {bad!r}"
    print(f"{len(clean)} reference vectors equal, {len(refused)} refused as the host refuses them")


def _random_titles(count, seed):
    rng = random.Random(seed)
    pieces = (list("abcdefghijklmnopqrstuvwxyz") * 3 + list("ABCDEFGHIJKLMNOPQRSTUVWXYZ") + list("0123456789") * 2 +
              [" "] * 14 + ["-"] * 3 + ["\t", "\n", "\x0b", "\x0c", "\r", "\x1c", "\x1d", "\x1e", "\x1f"] +
              list(".,;:!?'\"()&/_+*#@%$~`^|<>=[]{}\\") + ["\x00", "\x07", "\x7f"])
    titles = []
    for i in range(count):
        length = rng.choice([rng.randint(0, 80), rng.randint(0, 600), rng.randint(253, 258), rng.randint(0, 3)])
        title = "".join(rng.choice(pieces) for _ in range(length))
        if i % 7 == 0:
            title = " " * rng.randint(0, 70) + title + rng.choice(["", " ", "\t", "   ", " \n "])
        if i % 11 == 0:
            title = title.replace(" ", "    ")
        titles.append(title)
    titles += ["a" * n for n in range(250, 260)] + [" " * 300 + "ab", "ab" + " " * 300 + "c", "x" + "\t" * 300 + "y"]
    return titles


def test_device_transform_matches_the_host_path():
    titles = _random_titles(20000, seed=11)
    status, enc, lengths, report = _prepare_raw(titles, True)
    assert status == 0 and report[2] == -1 and report[3] == -1
    host_enc, host_lengths, host_bad = _host_rows(ds.transform_titles(titles))
    assert np.array_equal(lengths, host_lengths)
    assert np.array_equal(enc, host_enc)
    assert _mask_bytes(report) == host_bad and host_bad

    # transform=False: the bytes as they are; titles beyond 255 characters are reported, the first one named
    status, enc, lengths, report = _prepare_raw(titles, False)
    first_long = next(i for i, t in enumerate(titles) if len(t) > 255)
    assert status == -1 and report[2] == first_long and report[3] == -1
    short = [t for t in titles if len(t) <= 255]
    status, enc, lengths, report = _prepare_raw(short, False)
    host_enc, host_lengths, host_bad = _host_rows(short)
    assert status == 0 and np.array_equal(lengths, host_lengths) and np.array_equal(enc, host_enc)
    assert _mask_bytes(report) == host_bad


def _query_case(truth, queries, chunks):
    """ds_query_rows_device == query_rows on the chunks [first, last) of the queries, rowptr / cols / q_maxint bits."""
    t_chars, t_offsets = prediction._pack(truth)
    problem = NativeProblem.from_flat(t_chars, t_offsets, np.zeros(1, np.uint8), np.zeros(1, np.int64), 3)
    a = problem.arrays()
    problem.close()
    q_chars, q_offsets = prediction._pack(queries)
    rowptr, cols, maxint = prediction.query_rows(q_chars, q_offsets, a["vocabulary_keys"], a["idf32"], a["idf64"])
    space = QuerySpace(a["vocabulary_keys"], a["idf32"], a["idf64"])
    table = prepare_queries(queries, False)
    n_max = max(last - first for first, last in chunks)
    d_rowptr = _lib.DeviceArray((n_max + 1,), np.int64)
    d_cols = _lib.DeviceArray((max(1, 253 * n_max),), np.int32)
    d_maxint = _lib.DeviceArray((max(1, n_max),), np.float64)
    for first, last in chunks:
        n = last - first
        _lib.check(_lib.lib().ds_query_rows_device(space.handle, table.handle, first, n, d_rowptr.ptr, d_cols.ptr,
                                                   d_maxint.ptr, d_cols.shape[0], None), "ds_query_rows_device")
        got_rowptr = d_rowptr.to_host(n + 1)
        want_rowptr, want_cols, want_maxint = ds.distributed.slice_queries(rowptr, cols, maxint, first, last)
        assert np.array_equal(got_rowptr, want_rowptr), (first, last)
        assert np.array_equal(d_cols.to_host(int(got_rowptr[-1])), want_cols), (first, last)
        assert np.array_equal(d_maxint.to_host(n).view(np.uint64), want_maxint.view(np.uint64)), (first, last)
    return a


def _whole(n):
    return [(0, n)]


def test_query_rows_synthetic_workload():
    w = synth.make_workload(20000, 5000, seed=3)
    truth, queries = synth._to_strings(w.t_flat, w.t_off), synth._to_strings(w.q_flat, w.q_off)
    _query_case(truth, queries, _whole(len(queries)) + [(17, 18), (4999, 5000), (1234, 1234), (5000, 5000),
                                                          (333, 4021), (0, 1)])


def test_query_rows_of_unknown_ngrams():
    rng = random.Random(5)
    truth = ["".join(rng.choice("abcdefgh ") for _ in range(rng.randint(3, 40))).strip() or "abc" for _ in range(3000)]
    queries = ["".join(rng.choice("mnopqrstuvwxyz0123456789 a") for _ in range(rng.randint(3, 80))).strip() or "xyz"
               for _ in range(2000)]
    _query_case(truth, queries, _whole(len(queries)) + [(100, 700), (1999, 2000)])


def test_query_rows_with_zero_idf():
    rng = random.Random(6)
    truth = ["qqq " + "".join(rng.choice("abcdefghij") for _ in range(rng.randint(3, 30))) for _ in range(2000)]
    queries = [t[:rng.randint(3, len(t))] + " qqq zz9" for t in truth[:500]] + ["qqq", "zzz", "qqqzzz"]
    a = _query_case(truth, queries, _whole(len(queries)) + [(7, 300)])
    assert (a["idf32"] == 0).sum() >= 1 and a["idf64"].max() > 0

    # every title holds every n-gram of the set: every idf is 0, unknown n-grams add nothing either
    same = ["abcd efg"] * 50
    a = _query_case(same, ["abcd efg", "bcd", "xyz abc", "zzzz", "abcd efgh"], _whole(5) + [(1, 4)])
    assert a["idf64"].max() == 0


def test_query_rows_at_the_length_limits():
    rng = random.Random(7)
    w = synth.make_workload(5000, 10, seed=4)
    truth = synth._to_strings(w.t_flat, w.t_off)
    letters = "abcdefghijklmnopqrstuvwxyz0123456789 "
    queries = ["abc", "a b", "000", "zzz", "9 9", " ab"[1:] + "c"]
    queries += ["".join(rng.choice(letters) for _ in range(253)).join("xy") for _ in range(20)]
    queries += [" ".join(truth[i:i + 30])[:255].strip().ljust(255, "a") for i in range(0, 600, 30)]
    queries += ["ab" * 127 + "a", "abc" * 85, "a" * 255]
    assert {len(q) for q in queries} == {3, 255}
    _query_case(truth, queries, _whole(len(queries)) + [(0, 1), (len(queries) - 1, len(queries)), (3, 30)])


# ---- Prediction on both paths -------------------------------------------------------------------------------------------
def _messy(title, rng):
    out = []
    for c in title:
        r = rng.random()
        if c == " " and r < 0.2:
            out.append(rng.choice(["-", "  ", " - ", " "]))
        elif c == "e" and r < 0.1:
            out.append(rng.choice(["é", "È", "É"]))
        elif r < 0.1:
            out.append(c.upper())
        elif r < 0.13:
            out.append(c + rng.choice(".,!'&()"))
        else:
            out.append(c)
    return rng.choice(["", " ", "  ", "'"]) + "".join(out) + rng.choice(["", " ", "!", " ."])


@pytest.fixture(scope="module")
def problem():
    """20,000 truth titles and 2,000 queries, 10 % of them verbatim truth titles (as test_gpu_prediction.py), with a raw,
    messy rendering of both for transform=True."""
    w = synth.make_workload(20000, 2000)
    truth = synth._to_strings(w.t_flat, w.t_off)
    ids = np.array(w.title_id, dtype=np.int64)
    rng = np.random.RandomState(21)
    queries = synth._to_strings(w.q_flat, w.q_off)
    for q, t in zip(rng.permutation(2000)[:200], rng.randint(0, len(truth), 200)):
        queries[q] = truth[t]
    forest = synth.make_forest(n_trees=100)
    model = ds.ForestModel(forest["feature"], forest["threshold"], forest["yes"], forest["no"], forest["missing"],
                           forest["tree_offsets"], forest["n_features"], forest["base_margin"])
    messy = random.Random(8)
    raw_truth = [_messy(t, messy) if i % 5 == 0 else t for i, t in enumerate(truth)]
    raw_queries = [_messy(q, messy) for q in queries]
    return truth, ids, queries, model, raw_truth, raw_queries


def _same_details(a, b):
    assert list(a.columns) == list(b.columns)
    for column in ("test_index", "match_row", "title_id", "stage"):
        assert np.array_equal(a[column].to_numpy(), b[column].to_numpy()), column
    assert np.array_equal(a["probability"].to_numpy().view(np.uint32), b["probability"].to_numpy().view(np.uint32))


@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("transform", [False, True])
def test_prediction_is_the_same_on_both_paths(problem, k, transform):
    truth, ids, queries, model, raw_truth, raw_queries = problem
    if transform:
        truth, queries = raw_truth, raw_queries
    device = ds.Prediction(truth, ids, model, top_n=k, transform=transform)
    host = ds.Prediction(truth, ids, model, top_n=k, transform=transform, prepare_queries="host")
    assert device.prepare_queries == "device"
    # a threshold at the median of the model stage's best probabilities: the model decides some queries, not all
    host.generate_test_predictions(queries)
    reached = host.details["probability"].to_numpy()[host.details["stage"].isin([0, 3]).to_numpy()]
    device.probability_threshold = host.probability_threshold = float(np.median(reached[~np.isnan(reached)]))
    for chunk in (None, 700):
        device.chunk_queries = host.chunk_queries = chunk
        want = host.generate_test_predictions(queries)
        got = device.generate_test_predictions(queries)
        assert got.equals(want), chunk
        _same_details(device.details, host.details)
        assert "prepare_queries" in device.timings and "prepare_queries" not in host.timings
    stage = device.details["stage"].to_numpy()
    assert (np.bincount(stage, minlength=4) > 0).all(), np.bincount(stage)
    subset, index = queries[:40], np.arange(40)[::-1] * 3
    device.chunk_queries = host.chunk_queries = 1
    got = device.generate_test_predictions(subset, test_index=index)
    assert got.equals(host.generate_test_predictions(subset, test_index=index))
    _same_details(device.details, host.details)
    assert device.generate_test_predictions([]).equals(host.generate_test_predictions([]))

    device.chunk_queries = host.chunk_queries = None
    picks = [0, 1] + [int(np.nonzero(stage == s)[0][0]) for s in (0, 1, 2, 3)]
    for q in picks:
        assert device.closest_search_single_title(queries[q]) == host.closest_search_single_title(queries[q]), q
        _same_details(device.details, host.details)
    print(f"top-{k} transform={transform}: stages {np.bincount(stage).tolist()}")


def test_errors_match_the_host_path(problem):
    truth, ids, queries, model, _, _ = problem
    device = ds.Prediction(truth, ids, model, top_n=10, transform=False)
    host = ds.Prediction(truth, ids, model, top_n=10, transform=False, prepare_queries="host")
    expected = host.generate_test_predictions(queries[:300])
    cases = [(queries[:5] + ["Abc def"], ValueError), (["ab\tcd"] + queries[:5], ValueError),
             (queries[:3] + ["a" * 256], ds.DoppelError), (queries[:3] + ["café"], UnicodeEncodeError),
             (["AB", "a" * 300], ValueError), (["a" * 300, "café"], UnicodeEncodeError),
             (["ok title", "x-y"], ValueError)]
    for titles, error in cases:
        with pytest.raises(error) as on_host:
            host.generate_test_predictions(titles)
        with pytest.raises(error) as on_device:
            device.generate_test_predictions(titles)
        if error is not ds.DoppelError:
            assert str(on_device.value) == str(on_host.value), titles
        assert device.generate_test_predictions(queries[:300]).equals(expected)
    with pytest.raises(ValueError) as on_host:
        host.closest_search_single_title("Mixed Case")
    with pytest.raises(ValueError) as on_device:
        device.closest_search_single_title("Mixed Case")
    assert str(on_device.value) == str(on_host.value)
