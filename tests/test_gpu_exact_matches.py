"""The exact stage (ds_exact_matches[_device]) against a dict built here in truth order: the last truth row of a title
wins (predict.py:74-78), every other query gets -1."""
import ctypes

import numpy as np
import pytest

import doppel_speller_amd as ds
from doppel_speller_amd import _lib, synth

pytestmark = pytest.mark.gpu


def _expected(truth, queries):
    last = {}
    for row, title in enumerate(truth):
        last[title] = row
    return np.array([last.get(q, -1) for q in queries], dtype=np.int32)


def _table(titles):
    enc, lengths = ds.encode_titles(titles)
    return ds.TitleTable(enc, lengths)


def _cases():
    rng = np.random.RandomState(3)
    w = synth.make_workload(5000, 10, seed=9)
    truth = synth._to_strings(w.t_flat, w.t_off)
    long_title = ("lorem ipsum dolor sit amet " * 10)[:255]
    for at in rng.randint(0, len(truth), 1000):                    # 1,000 copies of one short title: one long chain
        truth.insert(int(at), "abc")
    truth[17:17] = ["xyz", long_title, "qqq", long_title]
    picked = [truth[i] for i in rng.randint(0, len(truth), 600)]
    queries = picked + ["abc", "xyz", "xy", "xyzw", "ab", long_title, long_title[:254], long_title[:254] + "z",
                        "absent title 1", "qqq"]
    queries += [t[:-1] for t in picked[:50]] + [t + "s" for t in picked[50:100]]   # strict prefixes and extensions
    return truth, queries


def test_exact_matches_agree_with_a_dict_for_both_hash_widths():
    truth, queries = _cases()
    expected = _expected(truth, queries)
    assert (expected >= 0).sum() > 600 and (expected < 0).sum() > 50
    truth_table, query_table = _table(truth), _table(queries)
    found = ds.exact_matches(truth_table, query_table)
    assert np.array_equal(found, expected)
    truth_table.option("exact_hash_bits", 4)                         # 16 starting slots: byte comparisons decide
    assert np.array_equal(ds.exact_matches(truth_table, query_table), expected)
    truth_table.option("exact_hash_bits", 64)
    truth_table.option("exact_table", 0)                             # freed, rebuilt by the next call
    assert np.array_equal(ds.exact_matches(truth_table, query_table), expected)
    assert ds.exact_matches(truth_table, query_table, 0).shape == (0,)
    with pytest.raises(ds.DoppelError):
        truth_table.option("exact_hash_bits", 0)


def test_device_form_with_an_offset_and_the_best_row_override():
    truth, queries = _cases()
    expected = _expected(truth, queries)
    truth_table, query_table = _table(truth), _table(queries)
    first, n = 123, len(queries) - 123 - 7
    d_exact = _lib.DeviceArray((n,), np.int32)
    before = np.where(np.arange(n) % 3 == 0, -1, 1_000_000 + np.arange(n)).astype(np.int32)
    d_best = _lib.DeviceArray.from_host(before)
    _lib.check(_lib.lib().ds_exact_matches_device(truth_table.handle, query_table.handle, first, n, d_exact.ptr,
                                                  d_best.ptr, ctypes.c_void_p(0)), "ds_exact_matches_device")
    exact, best = d_exact.to_host(), d_best.to_host()
    assert np.array_equal(exact, expected[first:first + n])
    assert np.array_equal(best, np.where(exact >= 0, exact, before))
    status = _lib.lib().ds_exact_matches_device(truth_table.handle, query_table.handle, first, len(queries), d_exact.ptr,
                                                None, ctypes.c_void_p(0))
    assert status == -1                                              # rows beyond the query table: DS_E_ARG
    assert _lib.lib().ds_exact_matches_device(truth_table.handle, query_table.handle, 5, 0, None, None,
                                              ctypes.c_void_p(0)) == 0


def test_three_and_255_character_titles():
    truth = ["abc", "a" * 255, "abd", "a" * 254 + "b", "abc"]
    queries = ["abc", "a" * 255, "a" * 254, "a" * 254 + "b", "abe", "ab"]
    assert np.array_equal(ds.exact_matches(_table(truth), _table(queries)), _expected(truth, queries))


def test_two_million_truth_rows():
    """A build over many workgroups: encoded rows straight from the synthetic generator, duplicates appended."""
    _, t_flat, t_off = synth.make_truth(2_000_000, seed=4)
    rng = np.random.RandomState(8)
    copies = rng.randint(0, 2_000_000, 20_000)
    lengths = np.diff(t_off)
    take = np.concatenate([np.arange(t_off[i], t_off[i + 1]) for i in copies])
    t_flat = np.concatenate((t_flat, t_flat[take]))
    t_off = np.concatenate((t_off, t_off[-1] + np.cumsum(lengths[copies])))
    enc, t_len = ds.feature_engineering.encode_collection(t_flat, t_off)
    n = enc.shape[0]
    picked = rng.randint(0, n, 100_000)
    q_enc, q_len = enc[picked].copy(), t_len[picked].copy()
    q_enc[::7, 0] = (q_enc[::7, 0] % 36) + 2                         # some absent (or other) titles
    last = {}
    for row in range(n):
        last[enc[row, :t_len[row]].tobytes()] = row
    expected = np.array([last.get(q_enc[i, :q_len[i]].tobytes(), -1) for i in range(q_enc.shape[0])], np.int32)
    assert (expected < 0).sum() > 1000
    found = ds.exact_matches(ds.TitleTable(enc, t_len), ds.TitleTable(q_enc, q_len))
    assert np.array_equal(found, expected)
