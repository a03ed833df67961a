"""paths_amd._lib.LaunchTape and fork_behind against a fake library: what is recorded, in which order, who owns the events, and what
is refused.  No GPU and no built library: ``_lib.load`` is replaced by a fake that logs every call and keeps the one "pending" flag
the real library keeps per host thread."""
import threading

import pytest
import torch

from paths_amd import _lib

STOP_CAPABLE = "paths_topk"          # the fake's one stop-capable entry point: calling it takes the pending event


class FakeFn:
    def __init__(self, lib, name):
        self.lib, self.name, self.argtypes = lib, name, None

    def __call__(self, *args):
        lib, name = self.lib, self.name
        if name == "paths_stop_event_pending":
            return int(lib.pending)
        if name == "paths_last_error":
            return b"fake failure"
        lib.log.append((name, args))
        if name == "paths_event_create":
            lib.created += 1
            return lib.created                     # handles 1, 2, 3, ...
        if name == "paths_set_stop_event":
            lib.pending, lib.armed = True, args[0]
        elif name in ("paths_flush_stop_event", "paths_clear_stop_event", STOP_CAPABLE):
            lib.pending = False
        return 1 if name in lib.failing else 0


class FakeLib:
    def __init__(self):
        self.log, self.pending, self.armed, self.created, self.failing = [], False, None, 0, set()

    def __getattr__(self, name):                   # every entry point exists, once
        fn = FakeFn(self, name)
        setattr(self, name, fn)
        return fn

    def names(self, *only):
        return [n for n, _ in self.log if not only or n in only]


class FakeStream:
    def __init__(self, handle):
        self.cuda_stream, self.waited = handle, []

    def wait_stream(self, other):
        self.waited.append(other.cuda_stream)


@pytest.fixture
def lib(monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: fake)
    monkeypatch.setattr(_lib, "stream", lambda: 7)
    monkeypatch.setattr(_lib, "STOP_EVENTS", True)
    monkeypatch.setattr(_lib, "TAPE", None)
    return fake


SRC, DSTS = FakeStream(10), [FakeStream(11), FakeStream(12)]


def names(tape):
    return [name for _, _, name in tape.entries]


def test_stop_capable_call_last_in_the_block_needs_no_second_record(lib):
    tape = _lib.LaunchTape()
    with tape.record():
        with _lib.fork_behind(DSTS, SRC) as fb:
            _lib.call("paths_gemm", 1, 2)
            _lib.zeros((4,))                        # (a fill in front of the stop-capable kernel: it does not take the event)
            _lib.call(STOP_CAPABLE, 3)
    assert names(tape) == ["paths_set_stop_event", "paths_gemm", "paths_memset_zero", STOP_CAPABLE, "paths_flush_stop_event",
                           "paths_stream_wait_event", "paths_stream_wait_event"]
    assert fb.taken_at == 3
    assert [a for _, a, n in tape.entries if n == "paths_stream_wait_event"] == [(11, fb.ev), (12, fb.ev)]
    assert tape.entries[2][1] == (tape.entries[2][1][0], 16, 7)          # the fill: address, 4 floats, the patched stream


def test_launch_behind_the_stop_capable_call_records_the_event_again(lib):
    tape = _lib.LaunchTape()
    with tape.record():
        with _lib.fork_behind(DSTS, SRC) as fb:
            _lib.call(STOP_CAPABLE, 3)
            _lib.call("paths_gemm", 1, 2)
    assert names(tape) == ["paths_set_stop_event", STOP_CAPABLE, "paths_gemm", "paths_flush_stop_event", "paths_record_event",
                           "paths_stream_wait_event", "paths_stream_wait_event"]
    assert tape.entries[4][1] == (fb.ev, SRC.cuda_stream)


def test_block_without_a_stop_capable_call_flushes_and_waits(lib):
    tape = _lib.LaunchTape()
    with tape.record():
        with _lib.fork_behind(DSTS, SRC) as fb:
            _lib.call("paths_gemm", 1, 2)
    assert fb.taken_at is None
    assert names(tape) == ["paths_set_stop_event", "paths_gemm", "paths_flush_stop_event", "paths_stream_wait_event", "paths_stream_wait_event"]


def test_exception_in_the_block_disarms_and_the_tape_takes_the_next_block(lib):
    tape = _lib.LaunchTape()
    with tape.record():
        with pytest.raises(ZeroDivisionError):
            with _lib.fork_behind(DSTS, SRC):
                _lib.call("paths_gemm", 1, 2)
                1 / 0
        assert lib.names()[-1] == "paths_clear_stop_event" and not lib.pending
        assert names(tape) == ["paths_set_stop_event", "paths_gemm"]
        with _lib.fork_behind(DSTS[:1], SRC):
            _lib.call(STOP_CAPABLE, 3)
    assert names(tape)[2:] == ["paths_set_stop_event", STOP_CAPABLE, "paths_flush_stop_event", "paths_stream_wait_event"]


def test_nested_block_and_stale_pending_event_are_refused_before_arming(lib):
    tape = _lib.LaunchTape()
    with tape.record():
        with _lib.fork_behind(DSTS, SRC) as outer:
            with pytest.raises(_lib.PathsHipError, match="inside another"):
                with _lib.fork_behind(DSTS, SRC):
                    pass
            assert lib.names("paths_set_stop_event") == ["paths_set_stop_event"] and lib.armed == outer.ev and lib.pending
            assert tape.block is outer
            _lib.call(STOP_CAPABLE, 3)
        assert tape.block is None
        lib.pending = True                          # an event somebody armed and nothing took
        with pytest.raises(_lib.PathsHipError, match="pending"):
            with _lib.fork_behind(DSTS, SRC):
                pass
        assert lib.names("paths_set_stop_event") == ["paths_set_stop_event"] and tape.block is None
        lib.pending = False


def test_eager_and_stop_events_off_join_by_stream_wait(lib, monkeypatch):
    dsts = [FakeStream(21), FakeStream(22)]
    with _lib.fork_behind(dsts, SRC):
        _lib.call(STOP_CAPABLE, 3)
    assert [d.waited for d in dsts] == [[10], [10]] and lib.names() == [STOP_CAPABLE]
    monkeypatch.setattr(_lib, "STOP_EVENTS", False)
    tape = _lib.LaunchTape()
    with tape.record():
        with _lib.fork_behind(dsts, SRC):
            _lib.call(STOP_CAPABLE, 3)
    assert names(tape) == [STOP_CAPABLE, "paths_stream_wait", "paths_stream_wait"]
    assert [a for _, a, _ in tape.entries[1:]] == [(21, 10, 1), (22, 10, 2)] and [d.waited for d in dsts] == [[10, 10], [10, 10]]
    assert not set(lib.names()) & {"paths_set_stop_event", "paths_flush_stop_event", "paths_clear_stop_event", "paths_record_event",
                                   "paths_stream_wait_event"}


def _pass(tape):
    with tape.record():
        _lib.stream_wait(DSTS[0], SRC)
        with _lib.fork_behind(DSTS, SRC):
            _lib.call(STOP_CAPABLE, 3)
        _lib.stream_wait(SRC, DSTS[1])
    return [a for _, a, _ in tape.entries]


def test_recording_again_reuses_the_events_and_close_destroys_each_once(lib):
    tape = _lib.LaunchTape()
    first = _pass(tape)
    assert lib.created == 3
    assert _pass(tape) == first and lib.created == 3
    with pytest.raises(_lib.PathsHipError, match="not recording"):
        tape.next_event()                           # an event is taken only while recording
    tape.close()
    assert sorted(a[0] for n, a in lib.log if n == "paths_event_destroy") == [1, 2, 3] and tape.entries is None
    tape.close()
    assert len(lib.names("paths_event_destroy")) == 3
    _pass(tape)                                     # (a closed tape records again, on events of its own)
    assert lib.created == 6
    tape.close()
    assert sorted(a[0] for n, a in lib.log if n == "paths_event_destroy") == [1, 2, 3, 4, 5, 6]


def test_one_tape_records_at_a_time_and_none_is_left_behind(lib):
    a, b = _lib.LaunchTape(), _lib.LaunchTape()
    with a.record():
        assert _lib.TAPE is a
        with pytest.raises(_lib.PathsHipError, match="already being recorded"):
            with b.record():
                pass
        assert _lib.TAPE is a and b.entries is None
        _lib.call("paths_gemm", 1)
    assert _lib.TAPE is None and names(a) == ["paths_gemm"]
    with pytest.raises(ZeroDivisionError):
        with b.record():
            with _lib.fork_behind(DSTS, SRC):
                1 / 0
    assert _lib.TAPE is None and not lib.pending and b.block is None and b.thread is None
    lib.pending = True
    with pytest.raises(_lib.PathsHipError, match="pending"):
        with a.record():
            pass
    assert _lib.TAPE is None
    lib.pending = False
    _lib.call("paths_gemm", 2)                      # eager again: executed, recorded nowhere
    assert names(a) == ["paths_gemm"] and lib.names("paths_gemm") == ["paths_gemm"] * 2


def test_launch_from_another_thread_while_recording_raises_there(lib):
    tape, caught = _lib.LaunchTape(), []

    def other():
        for launch in (lambda: _lib.call("paths_gemm", 9), lambda: _lib.stream_wait(DSTS[0], SRC), lambda: _lib.zeros((2,))):
            try:
                launch()
            except _lib.PathsHipError as e:
                caught.append(str(e))

    with tape.record():
        _lib.call("paths_gemm", 1)
        th = threading.Thread(target=other)
        th.start()
        th.join()
        _lib.call("paths_gemm", 2)
    assert len(caught) == 3 and all("thread" in c for c in caught), caught
    assert [a for _, a, _ in tape.entries] == [(1,), (2,)] and lib.created == 0          # (nor did the foreign join take an event)


def test_play_stops_at_the_first_failure_and_names_it(lib):
    import ctypes as C
    tape = _lib.LaunchTape()
    lib.paths_gemm.argtypes, lib.paths_bad.argtypes, lib.paths_after.argtypes = [C.c_void_p, C.c_int], [C.c_int], [C.c_int]
    with tape.record():
        _lib.call("paths_gemm", None, 2)
        _lib.call("paths_bad", 3)
        _lib.call("paths_after", 4)
    entries = tape.converted()
    assert entries is tape.entries and [n for _, _, n in entries] == ["paths_gemm", "paths_bad", "paths_after"]
    assert entries[0][1][0] is None and isinstance(entries[0][1][1], C.c_int) and entries[0][1][1].value == 2
    del lib.log[:]
    tape.play(entries)
    assert lib.names() == ["paths_gemm", "paths_bad", "paths_after"]
    del lib.log[:]
    lib.failing.add("paths_bad")
    with pytest.raises(_lib.PathsHipError, match="paths_bad failed during tape replay: fake failure"):
        tape.play(entries)
    assert lib.names() == ["paths_gemm", "paths_bad", "paths_clear_stop_event"]
