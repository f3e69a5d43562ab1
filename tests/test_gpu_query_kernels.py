"""The query-side kernels through their C entries, on the cases tests/query_cases.py places on their edges (and
tests/test_query_cases_cpu.py proves to be there): ds_prepare_titles at every 64-byte step, at the 255 / 256 cut and on
titles of 70,000 bytes; ds_query_rows_device at every title length, sort width, table stride and call count around the
scan's 1024, with codes outside the 37; the exact-match table where its probe sequences pass the last slot;
ds_best_pairs_device against the literal loop of its header comment.  Everything is compared bit for bit or as equal
integers, outputs sit between 0x55-filled guards."""
import ctypes

import numpy as np
import pytest

import doppel_speller_amd as ds
import query_cases as qc
from doppel_speller_amd import _lib, prediction
from doppel_speller_amd.feature_engineering import encode_collection
from doppel_speller_amd.prediction import DeviceTitles, QuerySpace
from oracle import oracle

pytestmark = pytest.mark.gpu

GUARD = 4096                    # bytes of 0x55 in front of and behind every guarded output
MAX_BLOCKS, BLOCK = 4096, 256   # ds_best_pairs_device caps its grid there and strides over the rest


class Guarded:
    """`count` elements of `dtype` in HBM between two guard regions, all of it filled with 0x55."""

    def __init__(self, count, dtype):
        self.dtype, self.count = np.dtype(dtype), int(count)
        self.nbytes = self.count * self.dtype.itemsize
        self.raw = _lib.DeviceArray((2 * GUARD + self.nbytes,), np.uint8)
        _lib.check(_lib.lib().ds_memset(self.raw.ptr, 0x55, self.raw.nbytes, 0), "ds_memset")
        self.ptr = ctypes.c_void_p(self.raw.ptr.value + GUARD)

    def read(self):
        """The body; the guards on both sides must still hold 0x55."""
        host = self.raw.to_host()
        assert (host[:GUARD] == 0x55).all(), "bytes in front of the output were written"
        assert (host[GUARD + self.nbytes:] == 0x55).all(), "bytes behind the output were written"
        return host[GUARD:GUARD + self.nbytes].view(self.dtype)

    def untouched(self):
        return bool((self.read().view(np.uint8) == 0x55).all())


def _sync(stream=None):
    _lib.check(_lib.lib().ds_stream_sync(_lib.pointer(stream), 0), "ds_stream_sync")


@pytest.fixture(scope="module")
def stream():
    handle = ctypes.c_void_p()
    _lib.check(_lib.lib().ds_stream_create(0, ctypes.byref(handle)), "ds_stream_create")
    yield handle
    _lib.check(_lib.lib().ds_stream_destroy(handle, 0), "ds_stream_destroy")


# ---- ds_prepare_titles ------------------------------------------------------------------------------------------------

def _prepare(titles, transform, keep=False):
    """ds_prepare_titles straight through ctypes: (status, enc, lengths, report[, table]) whatever the report holds."""
    raw = [t.encode("ascii") for t in titles]
    offsets = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in raw], out=offsets[1:])
    chars = np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8)
    handle, report = ctypes.c_void_p(), np.zeros(4, dtype=np.int64)
    status = _lib.lib().ds_prepare_titles(_lib.pointer(chars), _lib.pointer(offsets), len(raw), int(transform), 0,
                                          None, ctypes.byref(handle), _lib.pointer(report))
    if status != 0:
        assert not handle.value
        return status, None, None, report
    table = DeviceTitles(handle, len(raw), 0)
    enc = np.empty((len(raw), 255), dtype=np.uint8)
    lengths = np.empty(len(raw), dtype=np.uint8)
    _lib.check(_lib.lib().ds_titles_read(table.handle, _lib.pointer(enc), _lib.pointer(lengths)), "ds_titles_read")
    if keep:
        return status, enc, lengths, report, table
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


def test_transform_of_the_whole_catalogue():
    titles = qc.transform_titles_catalogue()
    want = [oracle.transform_title(t) for t in titles]
    want_enc, want_lengths, want_bad = _host_rows(want)
    status, enc, lengths, report = _prepare(titles, True)
    assert status == 0 and report[2] == -1 and report[3] == -1
    wrong = np.nonzero((lengths != want_lengths) | (enc != want_enc).any(axis=1))[0]
    assert wrong.shape[0] == 0, [(int(r), titles[r][:300], want[r]) for r in wrong[:5]]
    assert _mask_bytes(report) == want_bad == [9, 10, 11, 12, 13, 28, 29, 30, 31]
    assert ds.transform_titles(titles) == want                     # the native host batch: three statements agree
    again = _prepare(titles, True)
    assert again[0] == 0 and np.array_equal(again[1], enc) and np.array_equal(again[2], lengths)
    assert np.array_equal(again[3], report)


def test_encoding_of_transformed_titles():
    titles, _ = qc.rows_titles()
    want_enc, want_lengths = qc.encode(titles)
    status, enc, lengths, report = _prepare(titles, False)
    assert status == 0 and report.tolist() == [0, 0, -1, -1]
    assert np.array_equal(lengths, want_lengths) and np.array_equal(enc, want_enc)
    fill = np.arange(255)[None, :] >= lengths[:, None]
    assert (enc[fill] == 0).all() and (enc[~fill] != 0).all()


def test_over_long_titles_are_reported_with_their_row():
    titles = ["abc"] * 70000
    titles[-1] = "a" * 256
    status, _, _, report = _prepare(titles, False)
    assert status == -1 and report[2] == 69999 and report[3] == -1
    assert b"title 69999 has 256 characters" in _lib.lib().ds_last_error()
    titles[0] = "b" * 256
    status, _, _, report = _prepare(titles, False)
    assert status == -1 and report[2] == 0 and report[3] == -1
    assert b"title 0 has 256 characters" in _lib.lib().ds_last_error()
    titles[0], titles[-1] = "b" * 255, "a" * 255
    status, enc, lengths, report = _prepare(titles, False)
    assert status == 0 and report[2] == -1 and lengths[0] == 255 == lengths[-1] and (lengths[1:-1] == 3).all()
    assert (enc[0] == qc.CODE_OF[ord("b")]).all() and (enc[-1] == qc.CODE_OF[ord("a")]).all()


# ---- ds_query_rows_device ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rows_case():
    titles, _ = qc.rows_titles()
    keys, idf32, idf64 = qc.vocabulary(qc.truth_titles())
    chars, offsets = prediction._pack(titles)
    reference = prediction.query_rows(chars, offsets, keys, idf32, idf64)
    return titles, (keys, idf32, idf64), reference, QuerySpace(keys, idf32, idf64)


def _query_rows(space, table, first, n):
    """One ds_query_rows_device call into guarded buffers -> (rowptr, the whole cols body, maxint)."""
    d_rowptr, d_cols, d_maxint = Guarded(n + 1, np.int64), Guarded(253 * n, np.int32), Guarded(n, np.float64)
    _lib.check(_lib.lib().ds_query_rows_device(space.handle, table.handle, first, n, d_rowptr.ptr, d_cols.ptr,
                                               d_maxint.ptr, 253 * n, None), "ds_query_rows_device")
    _sync()
    return d_rowptr.read(), d_cols.read(), d_maxint.read()


def _same_rows(got, want, what):
    rowptr, cols, maxint = got
    want_rowptr, want_cols, want_maxint = want
    assert np.array_equal(rowptr, want_rowptr), what
    used = int(want_rowptr[-1])
    assert np.array_equal(cols[:used], want_cols), what
    assert (cols[used:] == 0x55555555).all(), what                 # nothing behind the last listed column
    assert np.array_equal(maxint.view(np.uint64), want_maxint.view(np.uint64)), what


@pytest.mark.parametrize("kind", ["prepared", 255, 256, 300])
def test_query_rows_of_every_chunk(rows_case, kind):
    titles, _, reference, space = rows_case
    if kind == "prepared":
        status, _, _, _, table = _prepare(titles, False, keep=True)
        assert status == 0
    else:                                                          # ds_titles_create: junk behind every title's end
        table = ds.TitleTable(*qc.encode(titles, kind, junk=0 if kind == 255 else 7))
    for first, n in qc.chunks(len(titles)):
        got = _query_rows(space, table, first, n)
        if n == 0:                                                 # only rowptr[0] is written
            assert got[0].tolist() == [0] and got[1].shape == (0,) and got[2].shape == (0,)
        _same_rows(got, qc.slice_rows(*reference, first, n), (kind, first, n))
    table.close()


def test_query_rows_of_codes_outside_the_37(rows_case):
    _, (keys, idf32, idf64), _, space = rows_case
    enc, lengths = qc.invalid_code_rows()
    want = qc.rule_rows(enc, lengths, keys, idf32, idf64)
    for stride in (255, 300):
        wide = np.full((enc.shape[0], stride), 9, dtype=np.uint8)
        wide[:, :255] = enc
        table = ds.TitleTable(wide, lengths)
        for first, n in ((0, enc.shape[0]), (5, 20), (enc.shape[0] - 1, 1)):
            _same_rows(_query_rows(space, table, first, n), qc.slice_rows(*want, first, n), (stride, first, n))
        table.close()


# ---- exact matches ----------------------------------------------------------------------------------------------------

def test_exact_matches_of_every_table():
    for name, truth, queries in qc.exact_tables():
        expected = qc.exact_expected(truth, queries)
        truth_table, query_table = ds.TitleTable(*qc.encode(truth)), ds.TitleTable(*qc.encode(queries))
        assert np.array_equal(ds.exact_matches(truth_table, query_table), expected), (name, 64)
        truth_table.option("exact_hash_bits", 3)                    # eight start slots: the chains run on past slot 7
        assert np.array_equal(ds.exact_matches(truth_table, query_table), expected), (name, 3)
        truth_table.option("exact_table", 0)                        # freed, rebuilt by the next call
        assert np.array_equal(ds.exact_matches(truth_table, query_table), expected), (name, 3, "rebuilt")
        truth_table.option("exact_hash_bits", 64)
        assert np.array_equal(ds.exact_matches(truth_table, query_table), expected), (name, 64, "again")
        truth_table.option("exact_table", 0)
        assert np.array_equal(ds.exact_matches(truth_table, query_table), expected), (name, 64, "rebuilt")
        if name == "1024":                                          # the device form on a part of the query table
            first, n = 123, len(queries) - 123 - 7
            d_exact = Guarded(n, np.int32)
            _lib.check(_lib.lib().ds_exact_matches_device(truth_table.handle, query_table.handle, first, n,
                                                          d_exact.ptr, None, ctypes.c_void_p(0)),
                       "ds_exact_matches_device")
            _sync()
            assert np.array_equal(d_exact.read(), expected[first:first + n])
        truth_table.close()
        query_table.close()


# ---- ds_best_pairs_device ---------------------------------------------------------------------------------------------

def _best_pairs(rows, probabilities, stream):
    n, k = probabilities.shape
    d_rows, d_probabilities = _lib.DeviceArray.from_host(rows), _lib.DeviceArray.from_host(probabilities)
    outputs = [Guarded(n, dtype) for dtype in (np.int64, np.int32, np.uint32, np.int32)]
    _lib.check(_lib.lib().ds_best_pairs_device(d_rows.ptr, d_probabilities.ptr, n, k, *(o.ptr for o in outputs),
                                               _lib.pointer(stream)), "ds_best_pairs_device")
    _sync(stream)
    return outputs


def _same_best(outputs, want, what):
    for got, expected, name in zip(outputs, want, ("pair", "row", "probability bits", "count")):
        got = got.read()
        assert got.dtype == expected.dtype and np.array_equal(got, expected), (what, name)


@pytest.mark.parametrize("k", qc.BEST_KS)
def test_best_pairs_against_the_loop(k, stream):
    for n in (1, 255, 256, 257):
        rows, probabilities = qc.best_pair_case(n, k, seed=1000 * k + n)
        want = qc.best_pairs_loop(rows, probabilities)
        for s in (None, stream):
            _same_best(_best_pairs(rows, probabilities, s), want, (k, n, s is not None))


@pytest.mark.parametrize("k", [1, 2])
def test_best_pairs_past_the_grid(k, stream):
    n = MAX_BLOCKS * BLOCK + 1
    rows, probabilities = qc.best_pair_case(n, k, seed=77 + k)
    want = qc.best_pairs(rows, probabilities)
    for s in (None, stream):
        _same_best(_best_pairs(rows, probabilities, s), want, (k, s is not None))


def test_best_pairs_of_no_query_write_nothing(stream):
    d_in = _lib.DeviceArray((8,), np.int32)
    outputs = [Guarded(4, dtype) for dtype in (np.int64, np.int32, np.uint32, np.int32)]
    for s in (None, stream):
        _lib.check(_lib.lib().ds_best_pairs_device(d_in.ptr, d_in.ptr, 0, 7, *(o.ptr for o in outputs),
                                                   _lib.pointer(s)), "ds_best_pairs_device")
        _sync(s)
    assert all(o.untouched() for o in outputs)


def test_the_best_pair_indexes_the_feature_rows(stream):
    """What d_best_pair is for: ds_gather_rows_device with it picks the rows plain fancy indexing picks."""
    n, k, width = 257, 7, 5
    rows, probabilities = qc.best_pair_case(n, k, seed=9)
    want_pair = qc.best_pairs_loop(rows, probabilities)[0]
    source = np.random.RandomState(4).rand(n * k, width).astype(np.float32)
    outputs = _best_pairs(rows, probabilities, stream)
    d_source, d_picked = _lib.DeviceArray.from_host(source), Guarded(n * width, np.float32)
    _lib.check(_lib.lib().ds_gather_rows_device(d_source.ptr, width, outputs[0].ptr, n, n * k, d_picked.ptr,
                                                _lib.pointer(stream)), "ds_gather_rows_device")
    _sync(stream)
    assert np.array_equal(d_picked.read().reshape(n, width).view(np.uint32), source[want_pair].view(np.uint32))
    assert not np.array_equal(source[want_pair], source[np.arange(n) * k])       # not simply every first candidate
