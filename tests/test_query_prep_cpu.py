"""The device query preparation without a GPU: Prediction refuses a bad `prepare_queries` before any library call, and
the new C entry points (ds_query_space_create, ds_prepare_titles, ds_query_rows_device) refuse null pointers and bad
ranges with DS_E_ARG and a message before they touch a device."""
import ctypes

import numpy as np
import pytest

from doppel_speller_amd import _lib
from doppel_speller_amd.prediction import Prediction


@pytest.fixture
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was called before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", refuse)


@pytest.fixture(scope="module")
def library():
    import doppel_speller_amd as ds
    handle = ctypes.CDLL(ds.build_library())
    handle.ds_last_error.restype = ctypes.c_char_p
    return handle


def _p(array):
    return array.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("value", ["gpu", "Device", "", None, 1, True])
def test_bad_prepare_queries_is_refused(no_library, value):
    with pytest.raises(ValueError, match="prepare_queries"):
        Prediction(["abc", "abd"], [0, 1], object(), top_n=1, prepare_queries=value)


def test_query_space_argument_errors(library):
    out = ctypes.c_void_p()
    assert library.ds_query_space_create(None, None, None, ctypes.c_int64(3), 0, None) == -1
    assert b"out is null" in library.ds_last_error()
    assert library.ds_query_space_create(None, None, None, ctypes.c_int64(3), 0, ctypes.byref(out)) == -1
    assert b"null" in library.ds_last_error()
    assert library.ds_query_space_create(None, None, None, ctypes.c_int64(-1), 0, ctypes.byref(out)) == -1
    assert b"V=-1" in library.ds_last_error()
    idf32, idf64 = np.ones(2, np.float32), np.ones(2, np.float64)
    for keys in (np.array([0x616263, 0x616262], np.uint32), np.array([0x616263, 0x616263], np.uint32),
                 np.array([0x20616263, 0x20616264], np.uint32)):
        assert library.ds_query_space_create(_p(keys), _p(idf32), _p(idf64), ctypes.c_int64(2), 0,
                                             ctypes.byref(out)) == -1
        assert b"strictly ascending" in library.ds_last_error()
    assert not out.value


def test_prepare_titles_argument_errors(library):
    out = ctypes.c_void_p(1)
    report = np.zeros(4, np.int64)
    chars = np.frombuffer(b"abcdef", np.uint8).copy()
    offsets = np.array([0, 3, 6], np.int64)

    def call(chars_, offsets_, n, transform=1, out_=ctypes.byref(out), report_=_p(report)):
        return library.ds_prepare_titles(chars_, offsets_, ctypes.c_int64(n), transform, 0, None, out_, report_)

    assert call(_p(chars), _p(offsets), 2, report_=None) == -1
    assert b"null out" in library.ds_last_error()
    assert call(_p(chars), _p(offsets), 2, out_=None) == -1
    assert call(_p(chars), _p(offsets), 0) == -1 and b"n=0" in library.ds_last_error()
    assert not out.value and report.tolist() == [0, 0, -1, -1]
    assert call(_p(chars), _p(offsets), 2, transform=2) == -1 and b"transform" in library.ds_last_error()
    assert call(_p(chars), None, 2) == -1 and b"null offsets" in library.ds_last_error()
    assert call(None, _p(offsets), 2) == -1 and b"null chars" in library.ds_last_error()
    decreasing = np.array([0, 4, 3], np.int64)
    assert call(_p(chars), _p(decreasing), 2) == -1 and b"bad offsets at 1" in library.ds_last_error()
    shifted = np.array([1, 3, 6], np.int64)
    assert call(_p(chars), _p(shifted), 2) == -1 and b"offsets[0]" in library.ds_last_error()


def test_query_rows_device_argument_errors(library):
    buffer = np.zeros(1024, np.int64)
    assert library.ds_query_rows_device(None, None, ctypes.c_int64(0), ctypes.c_int64(1), _p(buffer), _p(buffer),
                                        _p(buffer), ctypes.c_int64(253), None) == -1
    assert b"null space" in library.ds_last_error()
