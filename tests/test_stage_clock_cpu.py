"""prediction.StageClock without a GPU: `_lib.Timer` is replaced by a fake that counts its constructions and reads and
returns scripted times."""
import types

import pytest

from doppel_speller_amd import _lib, prediction


class FakeTimer:
    made = []
    script = []

    def __init__(self, device=0):
        self.device, self.running, self.reads = device, False, 0
        FakeTimer.made.append(self)

    def start(self, stream=None):
        assert not self.running
        self.running = True

    def stop(self, stream=None):
        assert self.running
        self.running = False

    def elapsed_ms(self):
        assert not self.running
        self.reads += 1
        return FakeTimer.script.pop(0)


@pytest.fixture
def clock(monkeypatch):
    FakeTimer.made, FakeTimer.script = [], []
    monkeypatch.setattr(_lib, "Timer", FakeTimer)
    timings = dict.fromkeys(("top_k", "features", "model", "copy_back"), 0.0)
    return prediction.StageClock(timings, device=3), timings


def test_two_chunks_of_a_stage_accumulate_on_one_timer(clock):
    clock, timings = clock
    ran = []
    for chunk, ms in enumerate((1.5, 2.25)):
        FakeTimer.script.append(ms)
        clock.device("top_k", lambda: ran.append(chunk))
        clock.collect()
    assert ran == [0, 1] and timings["top_k"] == 3.75
    assert len(FakeTimer.made) == 1 and FakeTimer.made[0].device == 3 and FakeTimer.made[0].reads == 2


def test_a_stage_that_never_runs_keeps_zero_and_makes_no_timer(clock):
    clock, timings = clock
    assert FakeTimer.made == []
    FakeTimer.script = [4.0]
    clock.device("top_k", lambda: None)
    clock.collect()
    assert timings == {"top_k": 4.0, "features": 0.0, "model": 0.0, "copy_back": 0.0}
    assert len(FakeTimer.made) == 1


def test_collect_reads_each_pending_stage_once_in_the_order_they_ran(clock):
    clock, timings = clock
    clock.device("model", lambda: None)
    clock.device("top_k", lambda: None)
    clock.device("features", lambda: None)
    assert timings == dict.fromkeys(timings, 0.0) and all(timer.reads == 0 for timer in FakeTimer.made)
    FakeTimer.script = [1.0, 2.0, 4.0]            # handed out in the order of the reads
    clock.collect()
    assert (timings["model"], timings["top_k"], timings["features"]) == (1.0, 2.0, 4.0)
    assert [timer.reads for timer in FakeTimer.made] == [1, 1, 1]
    clock.collect()                               # nothing is pending: an empty script is not touched
    assert [timer.reads for timer in FakeTimer.made] == [1, 1, 1] and timings["model"] == 1.0


def test_host_adds_wall_clock_to_its_own_key(clock, monkeypatch):
    clock, timings = clock
    ticks = iter((10.0, 10.5, 20.0, 20.25))
    monkeypatch.setattr(prediction, "time", types.SimpleNamespace(perf_counter=lambda: next(ticks)))
    with clock.host("copy_back"):
        pass
    with clock.host("copy_back"):
        pass
    assert timings == {"top_k": 0.0, "features": 0.0, "model": 0.0, "copy_back": 750.0}
    assert FakeTimer.made == []


def test_an_error_inside_enqueue_propagates_and_leaves_nothing_pending(clock):
    clock, timings = clock

    def fail():
        raise RuntimeError("no kernel")

    with pytest.raises(RuntimeError, match="no kernel"):
        clock.device("features", fail)
    clock.collect()                               # would pop from the empty script if the stage were pending
    assert timings["features"] == 0.0 and all(timer.reads == 0 for timer in FakeTimer.made)
