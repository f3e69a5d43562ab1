"""What tests/query_cases.py generates, checked from the inputs alone: the committed enumeration, fixed block and seeds
place a case on every edge tests/test_gpu_query_kernels.py is named for.  A softer catalogue fails HERE instead of the GPU
tests quietly testing less.  `oracle.transform_title` (the pinned restatement of the reference's function) is the judge of
the transform catalogue; the plain-Python rule of the query rows is held against `prediction.query_rows`; the hash of the
exact-match table is restated and followed slot by slot; the best-pair loop is held against its one-pass form."""
import numpy as np
import pytest

import query_cases as qc
from oracle import oracle


@pytest.fixture(scope="module")
def catalogue():
    titles = qc.transform_titles_catalogue()
    return titles, [oracle.transform_title(t) for t in titles]


def test_the_enumeration_is_complete():
    tails = qc.tails()
    assert len(tails) == 19608 == len(set(tails)) and set("".join(tails)) == set(qc.TAIL_ALPHABET)
    titles = qc.enumerated_titles()
    assert len(titles) == 78432 == len(set(titles))
    for prefix, edge in zip(qc.PREFIXES[1:], (64, 128, 255)):     # the tail's five bytes lie across the boundary
        assert prefix < edge < prefix + 5
        assert sum(1 for t in titles if t.startswith("x" * prefix) and len(t) <= prefix + 7) == 19608


def test_transform_catalogue_pads_and_cuts(catalogue):
    titles, transformed = catalogue
    kept = [qc.collapsed(t) for t in titles]
    for text, want in zip(kept, transformed):                     # `collapsed` is the judge's text before the cut
        cut = text[:255].strip()
        assert want == (cut.rjust(3, "0") if len(text) < 3 else cut)
    lengths = np.array([len(text) for text in kept])
    padded, cut = int((lengths < 3).sum()), int((lengths > 255).sum())
    space_255 = sum(1 for text in kept if len(text) > 255 and text[254] == " ")
    space_256 = sum(1 for text in kept if len(text) > 255 and text[255] == " ")
    white_256 = sum(1 for text in kept if len(text) > 255 and text[255] in qc.WHITE)
    second_strip = [len(text[:255]) - len(text[:255].strip()) for text in kept]
    tab_inside = sum(1 for text in transformed if "\t" in text)
    figures = dict(titles=len(titles), padded=padded, cut=cut, space_255=space_255, space_256=space_256,
                   white_256=white_256, second_strip_over_1=sum(1 for s in second_strip if s > 1),
                   second_strip_max=max(second_strip), tab_inside=tab_inside,
                   kept_lengths=sorted(set(lengths[(lengths >= 253) & (lengths <= 258)].tolist())))
    print(figures)
    assert padded >= 1000 and cut >= 1000
    assert space_255 >= 1 and space_256 >= 1 and white_256 > space_256
    assert figures["second_strip_over_1"] >= 1 and figures["second_strip_max"] >= 4
    assert figures["kept_lengths"] == [253, 254, 255, 256, 257, 258] and 300 in lengths and (lengths == 0).sum() >= 10
    assert tab_inside > 0.3 * len(titles)                          # why the raw entry is used, not prepare_queries
    empty_padded = [want for text, want in zip(kept, transformed) if len(text) == 0]
    assert set(empty_padded) == {"000"}
    bad = set("".join(transformed)) - set(qc.SYMBOLS)
    assert bad == set(qc.WHITE) - {" "}                            # every white-space byte but ' ' reaches the bad mask
    raw_lengths = np.array([len(t) for t in titles])
    for total in (1000, 70000):
        long = lengths[raw_lengths == total]
        assert (long < 3).any() and (long == 255).any() and (long > 256).any(), total


@pytest.mark.parametrize("step", [64, 128])
def test_transform_catalogue_sits_on_the_step(step):
    prefix = step - 3
    enumerated = [t for t in qc.enumerated_titles() if t.startswith("x" * prefix) and len(t) <= prefix + 7]
    assert len(enumerated) == 19608
    fixed = [title for _, title in qc.fixed_titles()]
    for group, name in ((enumerated, "enumerated"), (fixed, "fixed")):
        straddling = sum(qc.space_run_straddles(t, step) for t in group)
        dash = sum(1 for t in group if len(t) > step and "-" in t[step - 1:step + 1])
        print(dict(step=step, group=name, straddling=straddling, dash=dash))
        assert straddling >= 10 and dash >= 5
    assert sum(qc.empty_step_between_spaces(t, step) for t in fixed) >= 4
    if step == 64:                                                # "a " + 126..130 removed characters + " b"
        assert sum(qc.empty_step_between_spaces("a " + "." * m + " b", 64) for m in range(126, 131)) == 5
    first = [qc.first_solid_offset(t) for t in fixed]
    for offset in (step - 1, step, step + 1):                     # the first solid byte in lane 63, lane 0 and lane 1
        assert first.count(offset) >= 2, offset
    # leading white space of exactly step bytes, all of it kept and none of it a solid character
    assert any(len(t) > step and qc.transform_trace(t)[0][:step].all() and qc.first_solid_offset(t) == step for t in fixed)
    white_only = [t for t in fixed if qc.first_solid_offset(t) < 0 and qc.transform_trace(t)[0].all()]
    assert {63, 64, 65, 128, 300} <= {len(t) for t in white_only}


@pytest.fixture(scope="module")
def rows_case():
    titles, styles = qc.rows_titles()
    keys, idf32, idf64 = qc.vocabulary(qc.truth_titles())
    return titles, styles, keys, idf32, idf64


def test_rows_catalogue_holds_every_length_and_kind(rows_case):
    titles, styles, keys, idf32, idf64 = rows_case
    assert len(titles) == qc.ROUNDS * 256 * 5 and set("".join(titles)) == set(qc.SYMBOLS)
    lengths = np.array([len(t) for t in titles])
    grams = qc.gram_counts(lengths)
    for style in qc.STYLES:
        of_style = np.array([s == style for s in styles])
        assert sorted(set(grams[of_style].tolist())) == list(range(254)), style
        assert np.bincount(lengths[of_style], minlength=256).tolist() == [qc.ROUNDS] * 256
    for edge in (64, 65, 128, 129):                               # both sides of the sort widths: lengths 66/67, 130/131
        assert (grams == edge).sum() == 5 * qc.ROUNDS
    distinct = np.array([qc.distinct_grams(t) for t in titles])
    assert (distinct == 0).sum() == 3 * 5 * qc.ROUNDS and (distinct == 1).sum() >= 253 * qc.ROUNDS
    assert (distinct == 253).sum() >= qc.ROUNDS and (distinct == 2).sum() >= 200 and (distinct == 3).sum() >= 200
    is_distinct = np.array([s == "distinct" for s in styles])
    assert np.array_equal(distinct[is_distinct], grams[is_distinct])
    # known, unknown and zero-idf tri-grams, each in many titles and all three together in some
    column = {int(k): c for c, k in enumerate(keys.tolist())}
    assert (idf32 == 0).sum() >= 2 and idf64.max() > 0
    kinds = np.zeros((len(titles), 3), dtype=bool)
    for row, title in enumerate(titles):
        for i in range(len(title) - 2):
            c = column.get(int.from_bytes(title[i:i + 3].encode("ascii"), "big"))
            kinds[row, 2 if c is None else int(idf32[c] == 0)] = True
    print(dict(listed=int(kinds[:, 0].sum()), zero_idf=int(kinds[:, 1].sum()), unknown=int(kinds[:, 2].sum()),
               all_three=int(kinds.all(axis=1).sum())))
    assert kinds[:, 0].sum() >= 1000 and kinds[:, 1].sum() >= 100 and kinds[:, 2].sum() >= 1000
    assert kinds.all(axis=1).sum() >= 10
    assert (kinds[:, 1] & ~kinds[:, 0] & ~kinds[:, 2] & (grams > 0)).sum() >= 10     # a title that lists nothing, adds nothing
    # every chunk count with first = 0 and first > 0, and the two empty chunks
    chunk_list = qc.chunks(len(titles))
    for n in (1, 1023, 1024, 1025, 2048, 2049, 3073):
        firsts = [first for first, count in chunk_list if count == n]
        assert 0 in firsts and any(first > 0 for first in firsts), n
    empties = [first for first, count in chunk_list if count == 0]
    assert len(titles) in empties and any(0 < first < len(titles) for first in empties)
    for first, n in chunk_list:
        if n >= 1023:
            here = grams[first:first + n]                           # every sort width and the empty row in every long call
            assert len(set(here.tolist())) >= 200 and (here == 0).any() and ((here >= 1) & (here <= 64)).any(), (first, n)
            assert ((here >= 65) & (here <= 128)).any() and (here >= 129).any(), (first, n)


def test_the_plain_rule_is_query_rows_on_valid_titles(rows_case):
    from doppel_speller_amd import prediction
    titles, _, keys, idf32, idf64 = rows_case
    chars, offsets = prediction._pack(titles)
    rowptr, cols, maxint = prediction.query_rows(chars, offsets, keys, idf32, idf64)
    enc, lengths = qc.encode(titles)
    rule = qc.rule_rows(enc, lengths, keys, idf32, idf64)
    assert np.array_equal(rule[0], rowptr) and np.array_equal(rule[1], cols)
    assert np.array_equal(rule[2].view(np.uint64), maxint.view(np.uint64))
    assert rowptr[-1] > 10000 and (np.diff(rowptr) == 0).sum() >= 50 and len(set(maxint.tolist())) > 1000
    for stride in (256, 300):                                      # the wider tables hold the same titles, junk behind them
        wide, wide_lengths = qc.encode(titles, stride, junk=7)
        assert wide.shape == (len(titles), stride) and np.array_equal(wide_lengths, lengths)
        assert np.array_equal(wide[:, :255][enc != 0], enc[enc != 0]) and (wide[lengths == 0] == 7).all()
    first, n = 100, 1025
    part = qc.slice_rows(rowptr, cols, maxint, first, n)
    assert part[0][0] == 0 and part[0][-1] == part[1].shape[0] and part[2].shape == (n,)


def test_invalid_code_rows(rows_case):
    _, _, keys, idf32, idf64 = rows_case
    enc, lengths = qc.invalid_code_rows()
    inside = np.arange(255)[None, :] < lengths[:, None]
    for code in (0, 38, 64, 255):
        assert ((enc == code) & inside).any(axis=1).sum() >= 10, code
    valid_code = (enc >= 1) & (enc <= 37)
    assert (valid_code & inside).any(axis=1).sum() >= 30 and {66, 67, 130, 131, 255, 3, 0, 1, 2} <= set(lengths.tolist())
    rowptr, cols, maxint = qc.rule_rows(enc, lengths, keys, idf32, idf64)
    max_idf = float(idf64.max())
    one_code = [r for r in range(enc.shape[0]) if lengths[r] >= 3 and len(set(enc[r, :lengths[r]].tolist())) == 1]
    assert len(one_code) >= 10                                     # one invalid triple, however long the row
    for r in one_code:
        assert rowptr[r + 1] == rowptr[r] and maxint[r] == max_idf
    assert rowptr[-1] >= 20 and (maxint[lengths < 3] == 0).all()
    # a valid title with the same triples counted by hand: every distinct invalid triple adds max_idf once
    row = np.array([255, 2, 3, 255, 2, 3, 255], dtype=np.uint8)    # triples (255,2,3) (2,3,255) (3,255,2) twice, (255,2,3) again
    table = np.zeros((1, 255), np.uint8)
    table[0, :7] = row
    _, none, total = qc.rule_rows(table, np.array([7], np.uint8), keys, idf32, idf64)
    assert none.shape == (0,) and total[0] == max_idf + max_idf + max_idf


def test_exact_tables_wrap(rows_case):
    # the first two outputs of splitmix64 seeded with 0 are its finaliser of the golden ratio and of twice that
    assert qc.exact_mix(0) == 0 and qc.exact_mix(0x9e3779b97f4a7c15) == 0xe220a8397b1dcdaf
    assert qc.exact_mix((2 * 0x9e3779b97f4a7c15) & (2 ** 64 - 1)) == 0x6e789e6aa1b965f4
    assert qc.title_hash(b"") == qc.exact_mix(0x9e3779b97f4a7c15)
    assert qc.title_hash(bytes(range(1, 10))) == qc.exact_mix(
        qc.exact_mix(qc.exact_mix(0x9e3779b97f4a7c15 ^ 9) ^ 0x0807060504030201) ^ 9)
    tables = qc.exact_tables()
    small = [t for t in tables if t[0].startswith("small")]
    assert len(small) == 200
    wrapping = 0
    for name, truth, queries in small:
        assert len(truth) == 8 == len(set(truth)) and all(3 <= len(t) <= 6 for t in truth)
        assert qc.capacity_of(len(truth)) == 16
        wrapping += qc.chains_past_the_end(truth) > 0
        assert qc.chains_past_the_end(truth, 3) == 0               # eight start slots: the chains end at slot 14 at most
    big = next(t for t in tables if t[0] == "1024")
    assert len(big[1]) == 1024 == len(set(big[1])) and qc.capacity_of(1024) == 2048
    print(dict(small_tables_that_wrap=wrapping, big_table_chains=qc.chains_past_the_end(big[1])))
    assert wrapping >= 10 and qc.chains_past_the_end(big[1]) >= 1
    for name, truth, queries in tables:
        expected = qc.exact_expected(truth, queries)
        assert len(queries) == len(set(queries))
        queries = set(queries)
        distinct = len(set(truth))
        assert (expected >= 0).sum() >= distinct and (expected < 0).sum() >= 6
        assert "" in queries and any(len(q) == 1 for q in queries) and any(len(q) == 2 for q in queries)
        for title in set(truth):                                   # every prefix and every extension is asked for
            assert all(title[:n] in queries for n in range(len(title)))
            assert len(title) == 255 or all(title + c in queries for c in qc.SYMBOLS)
    name, truth, queries = tables[-1]
    expected = dict(zip(queries, qc.exact_expected(truth, queries).tolist()))
    assert expected[""] == 12 and expected["a"] == 7 and expected["ab"] == 8 and expected["abc"] == 9
    assert expected[qc.LONG_TITLE] == 10 and expected["xyz"] == 5 and expected[qc.LONG_TITLE[:254]] == -1
    assert len(qc.LONG_TITLE) == 255 and expected["abd"] == 11 and expected["abe"] == -1


@pytest.mark.parametrize("k", qc.BEST_KS)
def test_best_pair_cases(k):
    rows, probabilities = qc.best_pair_case(257, k, seed=k)
    assert rows.dtype == np.int32 and probabilities.dtype == np.float32 and rows.shape == probabilities.shape == (257, k)
    assert (rows < 0).any() and (rows > 0).any()
    assert set(probabilities.view(np.uint32).reshape(-1).tolist()) == set(qc.POOL.view(np.uint32).tolist())
    found = set()
    for row in probabilities:
        found |= qc.situation_of(row)
    wanted = set(qc.SITUATIONS) if k >= 2 else {"all equal", "all nan"}
    assert found >= wanted, wanted - found
    for name, row in qc.named_rows(k).items():
        assert name in qc.situation_of(row), name
    loop = qc.best_pairs_loop(rows, probabilities)
    fast = qc.best_pairs(rows, probabilities)
    for a, b in zip(loop, fast):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    pair, row, bits, count = loop
    where = pair - np.arange(257) * k
    assert ((where >= 0) & (where < k)).all() and (count >= 1).all() and (count <= k).all()
    nan_first = np.isnan(probabilities[:, 0])
    assert nan_first.sum() >= 10 and (where[nan_first] == 0).all() and (count[nan_first] == 1).all()
    assert (bits[nan_first] == 0x7fc00000).all()
    if k >= 2:
        # np.argmax takes a NaN for the maximum wherever it stands: the loop does not, which is why the loop is the reference
        differs = where != np.argmax(probabilities, axis=1)
        assert differs.sum() >= 10
        assert (np.isnan(probabilities[differs]).any(axis=1)).all()
        assert (count > 1).sum() >= 20 and (count == k).sum() >= 1 and (where == k - 1).sum() >= 1
