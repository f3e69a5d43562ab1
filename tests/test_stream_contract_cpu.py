"""The contract table of tests/stream_cases.py against the text of include/doppel_amd.h: every prototype with a stream
parameter is classified exactly once, in words its own comment uses, and has a case that tests/test_gpu_stream_order.py
runs.  A new `_device` entry point cannot be added without declaring and testing its class."""
import os

import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    with open(os.path.join(ROOT, "include", "doppel_amd.h")) as handle:
        return handle.read()


def test_every_prototype_with_a_stream_is_in_the_table_exactly_once():
    prototypes = sc.header_prototypes(header())
    assert len(prototypes) > 40
    names = [name for name, _, _ in sc.CONTRACT]
    assert len(names) == len(set(names)), sorted(name for name in names if names.count(name) > 1)
    assert not set(names) & set(sc.PLUMBING)
    assert set(names) | set(sc.PLUMBING) == set(prototypes), (sorted(set(prototypes) - set(names) - set(sc.PLUMBING)),
                                                               sorted((set(names) | set(sc.PLUMBING)) - set(prototypes)))


def test_the_comment_in_front_of_each_prototype_says_its_class():
    text = header()
    prototypes = sc.header_prototypes(text)
    for name, cls, phrase in sc.CONTRACT:
        comment = sc.comment_before(text, prototypes[name][0])
        assert phrase in comment, (name, phrase, comment[-300:])
        assert any(wording in phrase for wording in sc.CLASS_WORDING[cls]), (name, cls, phrase)
        if cls == sc.E:            # a phrase that goes on to say "synchronised" is no promise to only enqueue
            assert "synchronised" not in phrase and "synchronises" not in phrase, (name, phrase)


def test_the_prototype_finder_sees_what_it_should():
    prototypes = sc.header_prototypes(header())
    assert "ds_stream_create" not in prototypes          # void **stream: it makes one
    assert "ds_forest_predict" not in prototypes and "ds_forest_predict_device" in prototypes
    assert "ds_exhaustive_fold_device" in prototypes     # a remark inside its parameter list


def test_every_decoy_has_another_answer_than_the_real_input(oracle):
    """A call that read its inputs before they were there gets the decoy's answer: that must not be the real one.  The
    builders need no GPU; the staged arrays of a case have the shapes and types of the real ones."""
    for name, build in sc.CASES.items():
        spec = build(oracle)
        assert spec.entry == name
        assert spec.oracle_answers_differ(), name
        want = spec.expect(spec.values(0))
        written = set(spec.outputs) | set(spec.host_outputs) | set(spec.inout)
        assert set(want) == written - set(spec.scratch), (name, sorted(want), sorted(written))


def test_every_row_has_a_case_or_a_stated_reason():
    covered, left_out = set(sc.CASES), set(sc.NOT_COVERED)
    assert not covered & left_out
    assert covered | left_out == {name for name, _, _ in sc.CONTRACT}, sorted(
        {name for name, _, _ in sc.CONTRACT} - covered - left_out)
    assert all(reason.strip() for reason in sc.NOT_COVERED.values())
