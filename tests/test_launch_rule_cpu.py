"""The host side of every stage goes through csrc/ds_launch.h ("Host side of a stage"): csrc/ read as text."""
import pathlib
import re

CSRC = pathlib.Path(__file__).resolve().parent.parent / "doppel-speller_amd" / "csrc"
SOURCES = {path.name: path.read_text() for path in sorted(CSRC.iterdir()) if path.suffix in (".hip", ".h", ".inc", ".cpp")}

# launches that stay spelled out, by file: ds_exact.hip releases the exact-match table when the launch that fills it fails
SPELLED_OUT_LAUNCHES = {"ds_launch.h": 1, "ds_exact.hip": 1}
# the two soft reads of free memory size work and refuse nothing
FREE_MEMORY_READS = {"ds_runtime.hip": 2, "ds_exhaustive.hip": 1, "ds_jaccard_impl.inc": 1}


def code(text):
    return "\n".join(line.split("//")[0] for line in text.splitlines())


def occurrences(word):
    found = {name: len(re.findall(r"\b%s\b" % re.escape(word), code(text))) for name, text in SOURCES.items()}
    return {name: count for name, count in found.items() if count}


def test_sources_are_read():
    assert len([name for name in SOURCES if name.endswith(".hip")]) == 28 and "ds_launch.h" in SOURCES


def test_launches_go_through_ds_launch():
    assert occurrences("hipLaunchKernelGGL") == SPELLED_OUT_LAUNCHES


def test_dynamic_lds_is_allowed_in_one_place():
    assert occurrences("hipFuncSetAttribute") == {"ds_launch.h": 1}


def test_free_memory_is_read_in_one_place():
    assert occurrences("hipMemGetInfo") == FREE_MEMORY_READS
    assert len(re.findall(r"<< 20\) > free_bytes", "".join(SOURCES.values()))) == 1   # one head-room rule


def test_old_idioms_are_gone():
    for word in ("train_check_free", "DS_BUILD_STEP", "refresh_work_bytes", "isotonic_scratch_bytes"):
        assert not any(word in text for text in SOURCES.values()), word
    assert not any("status = DS_E_HIP" in text for text in SOURCES.values())
