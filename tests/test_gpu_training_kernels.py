"""The two training-set kernels (csrc/ds_training.hip) through the C ABI in every launch form: ds_misspell_titles on the
misspelling matrix recorded from the reference (tests/golden/misspell_matrix.npz: every edit path many times per edge
title), with row lists that are permuted and repeated, full and partial blocks, source strides other than 255, a stream
of the caller's and every rejected input; ds_training_pairs_device at the edges of its sample, its blocks and its output
window.  Every comparison is bit for bit, against the recorded answers or tests/training_set_oracle.py."""
import ctypes
import os

import numpy as np
import pytest

import training_set_oracle as ts

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DS_E_ARG = -1
SEED = 0x5eed0123456789ab


def _strings(array):
    return [bytes(x).decode("utf-8") for x in array]


def _encode(titles, stride=255):
    """(uint8[n, stride] codes, uint8[n] lengths) of titles over the port's alphabet."""
    enc = np.zeros((len(titles), stride), dtype=np.uint8)
    for i, title in enumerate(titles):
        enc[i, :len(title)] = ts.to_codes(title)
    return enc, np.array([len(t) for t in titles], dtype=np.uint8)


def _table(titles, stride=255):
    import doppel_speller_amd as ds
    return ds.TitleTable(*_encode(titles, stride))


def _misspell(table, rows, n, seed, stream=None):
    """ds_misspell_titles as the C ABI takes it: (status, message, handle); rows None is a null d_rows."""
    from doppel_speller_amd import _lib
    d_rows = None if rows is None else _lib.DeviceArray.from_host(np.ascontiguousarray(rows, dtype=np.int32))
    handle = ctypes.c_void_p()
    status = _lib.lib().ds_misspell_titles(table.handle, _lib.pointer(d_rows), n, ctypes.c_uint64(seed),
                                           _lib.pointer(stream), ctypes.byref(handle))
    return status, _lib.lib().ds_last_error().decode("utf-8", "replace"), handle


def _image(table, rows, n, seed, stream=None):
    """The output table read raw: (uint8[n, 255], uint8[n])."""
    from doppel_speller_amd.training_set import _DeviceTitles
    status, message, handle = _misspell(table, rows, n, seed, stream)
    assert status == 0, message
    out = _DeviceTitles(handle, n)
    try:
        return out.read()
    finally:
        out.close()


def _assert_image(got, expected_strings, what):
    """Codes and lengths equal the expected strings', and every byte from a row's length up to 255 is zero."""
    enc, lengths = got
    expected_enc, expected_len = _encode(expected_strings)
    assert enc.shape == expected_enc.shape, what
    assert np.array_equal(lengths, expected_len), (what, np.nonzero(lengths != expected_len)[0][:5])
    bad = np.nonzero((enc != expected_enc).any(axis=1))[0]
    assert bad.size == 0, (what, bad[:5], [ts.to_text(enc[i, :lengths[i]]) for i in bad[:3]],
                           [expected_strings[i] for i in bad[:3]])
    assert not (enc * (np.arange(255)[None, :] >= lengths[:, None])).any(), what


@pytest.fixture(scope="module")
def matrix():
    g = dict(np.load(os.path.join(GOLDEN, "misspell_matrix.npz"), allow_pickle=False))
    return _strings(g["titles"]), _strings(g["expected"]), int(g["seed"])


@pytest.fixture(scope="module")
def source(matrix):
    """300 titles spread over the whole matrix (long, short, digits, one word, mixed), their table at stride 255 and
    the oracle's misspelling of every row under SEED with the row's own stream."""
    titles = [matrix[0][i] for i in np.linspace(0, len(matrix[0]) - 1, 300).astype(int)]
    assert max(map(len, titles)) == 255 and min(map(len, titles)) == 3 and len(set(titles)) > 50
    expected = [ts.misspell(title, SEED, row) for row, title in enumerate(titles)]
    return titles, _table(titles), expected


# ---- ds_misspell_titles ----------------------------------------------------------------------------------------------
def test_matrix_on_the_device_equals_the_reference(matrix):
    import doppel_speller_amd as ds
    titles, expected, seed = matrix
    got = ds.generate_misspelled_names(titles, seed=seed)
    bad = [i for i, (a, b) in enumerate(zip(got, expected)) if a != b]
    assert not bad, [(i, titles[i], got[i], expected[i]) for i in bad[:5]]
    _assert_image(_image(_table(titles), None, len(titles), seed), expected, "matrix")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129, 300])
def test_launch_forms_key_the_stream_on_the_source_row(source, n):
    """Output i misspells source row rows[i] with the stream of rows[i], whatever i is: a null d_rows, a permutation,
    a list with repeats, and one row 65 times; full blocks (dword stores) and partial ones (byte stores)."""
    titles, table, expected = source
    rng = np.random.RandomState(n)
    forms = {"identity": None, "permutation": rng.permutation(300)[:n], "repeats": rng.randint(0, 300, n)}
    if n == 65:
        forms["one row"] = np.full(65, 299)
        forms["one long row"] = np.full(65, int(np.argmax([len(t) for t in titles])))
    if n > 1:
        assert np.unique(forms["repeats"]).size < n
    for name, rows in forms.items():
        index = np.arange(n) if rows is None else rows
        if rows is not None and n > 1:
            assert not np.array_equal(index, np.arange(n))
        _assert_image(_image(table, rows, n, SEED), [expected[r] for r in index], (name, n))


def test_source_strides_other_than_255(source):
    titles = source[0]
    short = [t for t in titles if len(t) <= 64]
    longest = max(map(len, short))
    assert len(short) > 128 and longest < 64
    for stride, subset in ((longest, short), (64, short), (300, titles), (256, titles)):
        expected = [ts.misspell(title, SEED, row) for row, title in enumerate(subset)]
        at_255 = _image(_table(subset), None, len(subset), SEED)
        other = _image(_table(subset, stride), None, len(subset), SEED)
        assert np.array_equal(other[0], at_255[0]) and np.array_equal(other[1], at_255[1]), stride
        _assert_image(other, expected, stride)
        rows = np.random.RandomState(stride).randint(0, len(subset), 130)
        _assert_image(_image(_table(subset, stride), rows, 130, SEED), [expected[r] for r in rows], (stride, "rows"))


def test_a_stream_of_the_callers(source):
    from doppel_speller_amd import _lib
    titles, table, expected = source
    rows = np.random.RandomState(5).permutation(300)[:200]
    stream = ctypes.c_void_p()
    _lib.check(_lib.lib().ds_stream_create(0, ctypes.byref(stream)), "ds_stream_create")
    try:
        on_stream = _image(table, rows, 200, SEED, stream)
    finally:
        _lib.lib().ds_stream_destroy(stream, 0)
    on_null = _image(table, rows, 200, SEED)
    assert np.array_equal(on_stream[0], on_null[0]) and np.array_equal(on_stream[1], on_null[1])
    _assert_image(on_stream, [expected[r] for r in rows], "stream")


def test_rejections():
    """One bad row among 67 good ones is DS_E_ARG with the count in the message and *out left null; the table answers
    correctly afterwards."""
    good = ["alpha beta", "abc", "12 345", "k" * 255] * 17                       # rows 0..67
    enc, lengths = _encode(good + ["abcd"] * 4)
    enc[68, 2] = 0                                                               # code 0 inside the title
    enc[69, 1] = 38                                                              # a code above the alphabet
    enc[70, :4], lengths[70] = [1, 1, 1, 0], 3                                   # three spaces
    lengths[71] = 2                                                              # too short
    import doppel_speller_amd as ds
    table = ds.TitleTable(enc, lengths)
    expected = [ts.misspell(title, SEED, row) for row, title in enumerate(good)]
    base = np.arange(68)
    for what, bad_row in (("row -1", -1), ("row n", 72), ("code 0", 68), ("code 38", 69), ("spaces", 70),
                          ("length 2", 71)):
        for place in (0, 40, 67):                                                # first block, and the partial second one
            rows = base.copy()
            rows[place] = bad_row
            status, message, handle = _misspell(table, rows, 68, SEED)
            assert status == DS_E_ARG and handle.value is None, (what, place, status)
            assert "1 rows" in message, (what, message)
    rows = base.copy()
    rows[[3, 64, 66]] = [-1, 70, 72]
    status, message, handle = _misspell(table, rows, 68, SEED)
    assert status == DS_E_ARG and handle.value is None and "3 rows" in message, message
    status, message, handle = _misspell(table, None, 72, SEED)                   # identity over the four bad rows
    assert status == DS_E_ARG and handle.value is None and "4 rows" in message, message
    _assert_image(_image(table, base, 68, SEED), expected, "after the rejections")
    _assert_image(_image(table, None, 68, SEED), expected, "identity after the rejections")


def test_refuses_no_titles_and_a_null_out():
    from doppel_speller_amd import _lib
    table = _table(["abc", "abcd"])
    for n in (0, -1):
        status, message, handle = _misspell(table, None, n, SEED)
        assert status == DS_E_ARG and handle.value is None, (n, message)
    status = _lib.lib().ds_misspell_titles(table.handle, None, 1, ctypes.c_uint64(SEED), None, None)
    assert status == DS_E_ARG
    handle = ctypes.c_void_p()
    status = _lib.lib().ds_misspell_titles(None, None, 1, ctypes.c_uint64(SEED), None, ctypes.byref(handle))
    assert status == DS_E_ARG and handle.value is None


def test_seeds_one_bit_apart_differ_on_most_titles():
    """Streams of two seeds are unrelated, so an answer repeats only when both draws land on the same edits at the same
    places: for the example titles (10 characters and more) the commonest single answer, the title itself, has a
    probability well under 1/2."""
    import doppel_speller_amd as ds
    titles = _strings(np.load(os.path.join(GOLDEN, "misspell_cases.npz"))["titles"])[:1000]
    for bit in (0, 31, 63):
        a, b = SEED, SEED ^ (1 << bit)
        got_a, got_b = ds.generate_misspelled_names(titles, seed=a), ds.generate_misspelled_names(titles, seed=b)
        assert got_b == [ts.misspell(title, b, row) for row, title in enumerate(titles)]
        assert sum(x != y for x, y in zip(got_a, got_b)) > 0.5 * len(titles), bit


# ---- ds_training_pairs_device ----------------------------------------------------------------------------------------
SENTINEL_I, SENTINEL_F, TAIL = -77, -77.5, 33


def _sample(rows, own, index, top_n, sample_n, seed, q_first):
    """One call into outputs filled with a sentinel, TAIL entries longer than the call's window; asserts that nothing
    outside the window [(q_first) * sample_n, (q_first + n) * sample_n) changed.  Returns (pair_q, pair_t, target) of
    the window as [n, sample_n]."""
    from doppel_speller_amd import _lib
    n = rows.shape[0]
    first, last = q_first * sample_n, (q_first + n) * sample_n
    d = [_lib.DeviceArray.from_host(a) for a in (rows.astype(np.int32), index.astype(np.int64), own.astype(np.int32))]
    out = [_lib.DeviceArray.from_host(np.full(last + TAIL, fill, dtype))
           for fill, dtype in ((SENTINEL_I, np.int32), (SENTINEL_I, np.int32), (SENTINEL_F, np.float32))]
    _lib.check(_lib.lib().ds_training_pairs_device(
        d[0].ptr, n, top_n, sample_n, d[1].ptr, d[2].ptr, ctypes.c_uint64(seed), q_first, out[0].ptr, out[1].ptr,
        out[2].ptr, None), "ds_training_pairs_device")
    host = [o.to_host() for o in out]
    for array, fill in zip(host, (SENTINEL_I, SENTINEL_I, SENTINEL_F)):
        assert (array[:first] == fill).all() and (array[last:] == fill).all()
    return [array[first:last].reshape(n, sample_n) for array in host]


def _hostile_case(n, top_n, sample_n, seed, rng):
    """Candidate rows, own rows and stream indexes that walk the sampler's edges, by query i % 6:
    0: the own row twice among the candidates, at random places;
    1: the own row at the place that lands in the last sampled slot, and at one more place (every other time the one
       that lands in the first slot);
    2: a short top-k (-1 from some place on), own row absent;
    3: a short top-k, no own row (-1);
    4: own row absent from the candidates;
    5: own row once among them.
    Stream indexes: negative ones, the extremes of int64 and values of 2^40 and more."""
    n_truth = 100000
    rows = np.stack([rng.choice(n_truth, top_n, replace=False) for _ in range(n)]).astype(np.int32)
    index = rng.randint(2 ** 40, 2 ** 62, n).astype(np.int64)
    index[::2] = -rng.randint(1, 2 ** 62, (n + 1) // 2)
    special = [-1, -2 ** 63, 2 ** 63 - 1, 2 ** 40, -2 ** 40, 0]
    index[:min(n, len(special))] = special[:n]
    own = (n_truth + rng.randint(0, 1000, n)).astype(np.int32)
    for i in range(n):
        kind = i % 6
        if kind in (0, 1, 5):
            own[i] = rows[i, rng.randint(top_n)]
        if kind == 0 and top_n > 1:
            rows[i, rng.choice(top_n, 2, replace=False)] = own[i]
        if kind == 1 and top_n > 1:
            places = ts.Stream(seed, ts.PURPOSE_SAMPLE, int(index[i])).sample(range(top_n), sample_n)
            rows[i] = np.where(rows[i] == own[i], n_truth + 5000, rows[i])
            rows[i, places[-1]] = own[i]
            others = [p for p in range(top_n) if p != places[-1]]
            rows[i, places[0] if sample_n > 1 and (i // 6) % 2 else rng.choice(others)] = own[i]
        if kind in (2, 3):
            rows[i, rng.randint(1, top_n + 1):] = -1
        if kind == 3:
            own[i] = -1
    return rows, own, index


@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("top_n, sample_n", [(2, 2), (10, 10), (16, 16), (11, 3), (17, 16), (100, 10)])
def test_sampler_edges_equal_the_oracle(n, top_n, sample_n):
    seed, q_first = 2 ** 64 - 3, 3
    rng = np.random.RandomState(1000 * top_n + 10 * sample_n + n % 10)
    rows, own, index = _hostile_case(n, top_n, sample_n, seed, rng)
    pair_q, pair_t, target = _sample(rows, own, index, top_n, sample_n, seed, q_first)
    twice_in_sample = last_slot = 0
    for i in range(n):
        sample, expected_target = ts.sample_candidates(rows[i].tolist(), sample_n, int(own[i]), seed, int(index[i]))
        assert pair_t[i].tolist() == sample, (i, i % 6)
        assert target[i].tolist() == [float(y) for y in expected_target], (i, i % 6)
        assert (pair_q[i] == q_first + i).all()
        if own[i] >= 0:                                      # every sampled copy of the own row is a positive
            assert target[i].sum() == max(1, sample.count(int(own[i])))
        else:
            assert target[i].sum() == 0
        twice_in_sample += sample.count(int(own[i])) == 2 and own[i] >= 0
        last_slot += i % 6 == 1 and top_n > 1 and sample[-1] == own[i]
    if n >= 255:
        assert last_slot == len(range(1, n, 6)), "case 1 puts the own row into the last sampled slot"
        assert twice_in_sample >= 3


def test_sampler_one_candidate():
    """top_n = sample_n = 1: the only step draws below(1)."""
    n = 257
    rng = np.random.RandomState(11)
    rows = rng.randint(0, 1000, (n, 1)).astype(np.int32)
    own = np.where(np.arange(n) % 3 == 0, rows[:, 0], np.where(np.arange(n) % 3 == 1, 5000, -1)).astype(np.int32)
    index = rng.randint(-2 ** 62, 2 ** 62, n).astype(np.int64)
    pair_q, pair_t, target = _sample(rows, own, index, 1, 1, 9, 2)
    assert pair_t[:, 0].tolist() == np.where(own >= 0, own, rows[:, 0]).tolist()
    assert target[:, 0].tolist() == (own >= 0).astype(np.float32).tolist()
    for i in range(n):
        assert ts.sample_candidates(rows[i].tolist(), 1, int(own[i]), 9, int(index[i])) == \
            ([int(pair_t[i, 0])], [int(target[i, 0])])


def test_sampler_no_queries_and_too_many_pairs():
    from doppel_speller_amd import _lib
    p = _lib.pointer(None)
    call = _lib.lib().ds_training_pairs_device
    assert call(p, 0, 10, 10, p, p, ctypes.c_uint64(0), 0, p, p, p, p) == 0
    assert call(p, 0, 10, 10, p, p, ctypes.c_uint64(0), 12345, p, p, p, p) == 0
    # (q_first + n_queries) * sample_n reaches 2^31: refused before any pointer is read
    for n, sample_n, q_first in ((2 ** 27, 16, 0), (1, 16, 2 ** 27 - 1), (2 ** 31, 1, 0), (1, 1, 2 ** 31 - 1)):
        assert call(p, n, 100, sample_n, p, p, ctypes.c_uint64(0), q_first, p, p, p, p) == DS_E_ARG
        assert "too many pairs" in _lib.lib().ds_last_error().decode()
    for n, q_first in ((-1, 0), (1, -1)):
        assert call(p, n, 10, 10, p, p, ctypes.c_uint64(0), q_first, p, p, p, p) == DS_E_ARG
    assert call(p, 1, 10, 10, p, p, ctypes.c_uint64(0), 0, p, p, p, p) == DS_E_ARG    # null pointers with work to do
