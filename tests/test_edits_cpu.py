"""Edit scripts and the learned misspelling model without a GPU ("Edit scripts and the learned
misspelling model"): the oracle of the rule (tests/edit_oracle.py) on pairs whose script is worked out by hand, its
generator on profiles that leave it no choice, the C ABI surface, and the checks made before any device work."""
import os
import re

import numpy as np
import pytest

import edit_cases as cases
import edit_oracle as eo
import training_set_oracle as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B = ts.ALPHABET.index("a"), ts.ALPHABET.index("b")


@pytest.mark.parametrize("a, b, distance, script", cases.HAND_PAIRS)
def test_oracle_gives_the_hand_written_scripts(a, b, distance, script):
    assert eo.align(cases.codes(a), cases.codes(b)) == (distance, script)


def test_oracle_scripts_replay_and_cost_their_distance():
    """Every script turns a into b, and its operations that are not matches number the distance."""
    for a, b in cases.length_edge_pairs()[:8] + cases.max_edits_pairs() + [(p[0], p[1]) for p in cases.HAND_PAIRS]:
        ca, cb = cases.codes(a), cases.codes(b)
        distance, script = eo.align(ca, cb)
        out = []
        for op, i, j in eo.walk(ca, cb, script):
            if op in (eo.MATCH,):
                assert ca[i] == cb[j]
                out.append(ca[i])
            elif op == eo.SUBSTITUTE:
                assert ca[i] != cb[j]
                out.append(cb[j])
            elif op == eo.INSERT:
                out.append(cb[j])
            elif op == eo.TRANSPOSE:
                assert ca[i] != ca[i + 1]
                out += [ca[i + 1], ca[i]]
        assert out == cb and sum(op != eo.MATCH for op in script) == distance and len(script) <= len(ca) + len(cb)
    assert [eo.align(cases.codes(a), cases.codes(b))[0] for a, b in cases.max_edits_pairs()] == [0, 4, 5, 32, 33]


def test_oracle_counts_of_one_pair():
    a, b = cases.codes("the cat"), cases.codes("teh cbtx")
    distance, script = eo.align(a, b)
    assert (distance, script) == (3, [eo.MATCH, eo.TRANSPOSE, eo.MATCH, eo.MATCH, eo.SUBSTITUTE, eo.MATCH, eo.INSERT])
    counts = eo.new_counts()
    eo.count_pair(counts, a, b, distance, script, 4)
    p = eo.Views(counts)
    t, h, e, c = (ts.ALPHABET.index(x) for x in "thec")
    assert counts[eo.COUNTED] == 1 and counts[eo.SKIPPED] == 0 and p.edits[3] == 1 and p.edits.sum() == 1
    assert p.seen[0] == 1 and p.seen[t] == 2 and p.seen.sum() == 8 and p.match.sum() == 4 and p.match[t] == 2
    assert p.transpose[h, e] == 1 and p.transpose.sum() == 1 and p.substitute[A, B] == 1 and p.substitute.sum() == 1
    assert p.insert[0, ts.ALPHABET.index("x")] == 1 and p.insert.sum() == 1 and p.delete.sum() == 0
    skipped = eo.new_counts()
    eo.count_pair(skipped, a, b, distance, script, 2)
    assert skipped[eo.SKIPPED] == 1 and skipped.sum() == 1


def _profile(**tables):
    counts = eo.new_counts()
    counts[eo.EDITS + 1] = 1
    counts[eo.SEEN + 1:eo.SEEN + eo.CODES] = 1000
    for name, entries in tables.items():
        at = {"substitute": eo.SUBSTITUTED, "insert": eo.INSERTED, "transpose": eo.TRANSPOSED, "delete": eo.DELETED}[name]
        for index, value in entries.items():
            counts[at + (index[0] * eo.CODES + index[1] if isinstance(index, tuple) else index)] = value
    return counts


def test_oracle_generator_on_profiles_that_leave_no_choice():
    only_a_to_b = eo.Profile(_profile(substitute={(A, B): 7}))
    for seed in range(5):
        assert eo.misspell_profile("cat", seed, 0, only_a_to_b) == "cbt"
        assert eo.misspell_profile("dog", seed, 3, only_a_to_b) == "dog"          # no a: T == 0, unchanged
        got = eo.misspell_profile("banana", seed, seed, only_a_to_b)
        assert sorted(i for i, (x, y) in enumerate(zip("banana", got)) if x != y)[0] in (1, 3, 5)
        assert len(got) == 6 and sum(x != y for x, y in zip("banana", got)) == 1 and got.count("b") == 2
    assert len({eo.misspell_profile("banana", seed, 0, only_a_to_b) for seed in range(40)}) == 3
    only_deletions = eo.Profile(_profile(delete={c: 10 for c in range(1, eo.CODES)}))
    assert eo.misspell_profile("cat", 1, 0, only_deletions) == "cat"               # L == 3: nothing may go
    assert len(eo.misspell_profile("cats", 1, 0, only_deletions)) == 3
    only_insertions = eo.Profile(_profile(insert={(c, A): 10 for c in range(0, eo.CODES)}))
    assert eo.misspell_profile("a" * 255, 2, 0, only_insertions) == "a" * 255     # L == 255: nothing may come
    assert eo.misspell_profile("b" * 254, 2, 0, only_insertions).count("a") == 1
    only_swaps = eo.Profile(_profile(transpose={(A, B): 5}))
    assert eo.misspell_profile("xaby", 0, 0, only_swaps) == "xbay"
    assert eo.misspell_profile("xaa", 0, 0, only_swaps) == "xaa"     # equal neighbours are never swapped, nor the last character
    two_edits = _profile(substitute={(A, B): 7})
    two_edits[eo.EDITS + 1], two_edits[eo.EDITS + 2] = 0, 3
    assert eo.misspell_profile("banana", 0, 0, eo.Profile(two_edits)).count("b") == 3


def test_header_declares_the_entry_points_without_a_stream():
    header = open(os.path.join(ROOT, "include", "doppel_amd.h")).read()
    for name in ("ds_edit_align", "ds_misspell_titles_profile", "ds_edit_option"):
        prototype = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M | re.S)
        assert prototype, name
        assert "stream" not in prototype.group(1), name
    from doppel_speller_amd import _lib, edits
    assert {"ds_edit_align", "ds_misspell_titles_profile", "ds_edit_option"} <= set(_lib.EXPORTED_SYMBOLS)
    assert "ds_edits.hip" in _lib._SOURCES and len(set(_lib._SOURCES)) == len(_lib._SOURCES)
    # the layout of the counts block is the same in the header, the package and the oracle
    defines = dict(re.findall(r"^#define (DS_EDIT_[A-Z_]+) (.*?)\s*(?:/\*.*)?$", header, re.M))

    def value(name):
        return eval(re.sub(r"DS_EDIT_[A-Z_]+", lambda m: str(value(m.group(0))), defines[name]))
    for name, oracle_value, package_value in (
            ("COUNTED", eo.COUNTED, edits.COUNTED), ("SKIPPED", eo.SKIPPED, edits.SKIPPED), ("EDITS", eo.EDITS, edits.EDITS),
            ("SEEN", eo.SEEN, edits.SEEN), ("MATCH", eo.MATCHED, edits.MATCH), ("DELETE", eo.DELETED, edits.DELETE),
            ("SUBSTITUTE", eo.SUBSTITUTED, edits.SUBSTITUTE), ("INSERT", eo.INSERTED, edits.INSERT),
            ("TRANSPOSE", eo.TRANSPOSED, edits.TRANSPOSE), ("COUNTS", eo.COUNTS, edits.COUNTS),
            ("OPS_STRIDE", eo.OPS_STRIDE, edits.OPS_STRIDE), ("CODES", eo.CODES, edits.CODES)):
        assert value("DS_EDIT_" + name) == oracle_value == package_value, name
    assert [value("DS_EDIT_OP_" + name.upper()) for name in edits.OPERATIONS] == [0, 1, 2, 3, 4]
    assert re.search(r"#define DS_MISSPELL_PURPOSE_PROFILE 8\b", header) and eo.PURPOSE_PROFILE == 8


def test_validate_misspelling_profile_rejects_what_it_should():
    import doppel_speller_amd as ds
    from doppel_speller_amd import edits
    good = _profile(substitute={(A, B): 7}, insert={(0, A): 2}, delete={A: 1}, transpose={(A, B): 1})
    assert np.array_equal(ds.validate_misspelling_profile(good), good)
    assert np.array_equal(ds.validate_misspelling_profile(ds.MisspellingProfile(good)), good)

    def changed(index, value):
        out = good.copy()
        out[index] = value
        return out
    empty = good.copy()
    empty[eo.EDITS + 1:eo.EDITS + 33] = 0
    bad = [good[:-1], good.astype(np.float64), good.reshape(1, -1), changed(5, -1), changed(eo.SEEN + 3, 1 << 40), empty,
           changed(eo.SUBSTITUTED + A * eo.CODES + A, 1), changed(eo.SUBSTITUTED + A * eo.CODES, 1),
           changed(eo.SUBSTITUTED + A, 1), changed(eo.INSERTED + A * eo.CODES, 1), changed(eo.TRANSPOSED + B, 1),
           changed(eo.TRANSPOSED + B * eo.CODES, 1), changed(eo.MATCHED, 1), changed(eo.DELETED, 1),
           changed(eo.INSERTED + B * eo.CODES + A, 4000), changed(eo.DELETED + B, 4000)]
    for counts in bad:
        with pytest.raises(ValueError):
            ds.validate_misspelling_profile(counts)
    for counts in bad[3:]:                        # the oracle refuses the same blocks
        with pytest.raises(ValueError):
            eo.Profile(counts)
    assert ds.validate_misspelling_profile(changed(eo.DELETED + B, 3999)) is not None      # just below 4 per character
    for max_edits in (-1, 33, 2.0, True):
        with pytest.raises(ValueError):
            edits._max_edits(max_edits)
    from doppel_speller_amd.training_set import validate_profile_argument
    assert validate_profile_argument(None) is None and validate_profile_argument("fit") == "fit"
    for value in ("learn", good, 4, ds.MisspellingProfile(empty)):
        with pytest.raises(ValueError):
            validate_profile_argument(value)
    with pytest.raises(ValueError):
        ds.FeatureEngineering(["abc"], [1], ["abd"], [1], top_n=1, sample_n=1, misspelling_profile="learn")
    with pytest.raises(ValueError, match="truth titles but"):
        ds.edit_operations(["abc"], [])


def test_profile_views_report_and_storage(tmp_path):
    import doppel_speller_amd as ds
    counts = cases.fixture_profile(ds.transform_titles)
    profile = ds.MisspellingProfile(counts, 4)
    oracle = eo.Profile(counts)
    for name in ("edits", "seen", "match", "delete", "substitute", "insert", "transpose"):
        assert np.array_equal(getattr(profile, name), getattr(oracle, name)), name
    rates = profile.rates()
    assert rates["substitute"].tolist() == oracle.rate_sub and rates["delete"].tolist() == oracle.rate_del
    assert rates["transpose"].tolist() == oracle.rate_tr and rates["insert"].tolist() == oracle.rate_ins
    assert profile.edits_per_title() == {d: int(v) for d, v in enumerate(oracle.edits) if v}
    shares = profile.operation_shares()
    assert abs(sum(shares.values()) - 1.0) < 1e-12 and shares["substitute"] == oracle.substitute.sum() / (
        oracle.substitute.sum() + oracle.insert.sum() + oracle.delete.sum() + oracle.transpose.sum())
    near = sum(int(oracle.substitute[a, b]) for a in ts.NEIGHBOURS for b in ts.NEIGHBOURS[a])
    assert profile.keyboard_share() == near / int(oracle.substitute[2:28, 2:28].sum())
    frame = profile.frame(5)
    assert list(frame.columns) == ["operation", "from", "to", "count", "rate"] and frame.shape[0] == 5
    assert frame["count"].tolist() == sorted(frame["count"].tolist(), reverse=True)
    assert "keyboard neighbours" in profile.report()
    twice = profile.merged(profile)
    assert np.array_equal(twice.counts, 2 * counts) and twice.counted == 2 * profile.counted and twice.max_edits == 4
    path = str(tmp_path / "profile.npz")
    profile.save(path)
    loaded = ds.MisspellingProfile.load(path)
    assert np.array_equal(loaded.counts, counts) and loaded.max_edits == 4


def test_edit_scripts_frame_and_render():
    from doppel_speller_amd.edits import EditScripts
    pairs = [("the cat", "teh cbtx"), ("xabc", "abc")]
    scripts = [eo.align(cases.codes(a), cases.codes(b)) for a, b in pairs]
    ops = np.zeros((2, 512), np.uint8)
    for i, (_, script) in enumerate(scripts):
        ops[i, :len(script)] = script
    result = EditScripts([a for a, _ in pairs], [b for _, b in pairs], np.array([s[0] for s in scripts], np.int32), ops,
                         np.array([len(s[1]) for s in scripts], np.int32))
    assert result.frame().values.tolist() == [[0, 1, "transpose", "he", "eh"], [0, 5, "substitute", "a", "b"],
                                              [0, 7, "insert", "", "x"], [1, 0, "delete", "x", ""]]
    assert result.render(0) == "the cat-\nteh cbtx\n ^^  ^ ^"
    assert result.render(1) == "xabc\n-abc\n^"


def test_fixture_pairs_are_counted_or_skipped():
    import doppel_speller_amd as ds
    truth, train, truth_rows, labelled = cases.fixture_pairs(ds.transform_titles)
    assert len(labelled) == 380
    for max_edits in (0, 4, 32):
        counts = cases.fixture_profile(ds.transform_titles, max_edits)
        profile = eo.Views(counts)
        assert counts[eo.COUNTED] + counts[eo.SKIPPED] == 380 and profile.edits.sum() == counts[eo.COUNTED]
        assert profile.seen[0] == counts[eo.COUNTED]
        assert profile.seen[1:].sum() == profile.match.sum() + profile.delete.sum() + profile.substitute.sum() + \
            2 * profile.transpose.sum()
    print("max_edits = 4:", int(counts[eo.COUNTED]), "counted")
