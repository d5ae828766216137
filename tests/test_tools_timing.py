"""tools/_timing.py: the timing loop's logic over an event source that counts.  No GPU."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _timing as T  # noqa: E402


class CountingDevice:
    """stands for torch.cuda: every call, record and synchronise is logged; two events are 7 ms apart per call made between them"""

    def __init__(self):
        self.log = []
        self.is_available = lambda: True
        self.synchronize = lambda: self.log.append("sync")
        self.call = lambda: self.log.append("call")

    def Event(self, enable_timing):
        assert enable_timing
        e = type("Event", (), {})()
        e.record = lambda: (setattr(e, "at", len(self.log)), self.log.append("record"))
        e.elapsed_time = lambda other: 7.0 * self.log[e.at:other.at].count("call")
        return e


def test_interleaved_warms_every_variant_up_then_runs_rounds_in_order():
    calls = []
    variants = [(k, (lambda k=k: calls.append(k) or len(calls))) for k in "abc"]
    samples = T.interleaved(variants, reps=4, warmup=2)
    assert calls == list("aabbcc") + list("abc") * 4
    assert samples == {"a": [7, 10, 13, 16], "b": [8, 11, 14, 17], "c": [9, 12, 15, 18]}
    assert list(T.interleaved(dict(variants), reps=1, warmup=0)) == list("abc")


def test_event_ms_makes_batch_calls_between_one_pair_of_events():
    dev = CountingDevice()
    assert T.event_ms(dev.call, batch=20, dev=dev) == 7.0                 # 140 ms between the events, over twenty
    assert dev.log == ["sync", "record"] + ["call"] * 20 + ["record", "sync"]
    assert T.event_ms(dev.call, dev=dev) == 7.0


def test_host_clock_ms_times_k_calls_behind_the_warm_up_up_to_a_synchronise():
    dev = CountingDevice()
    assert 0.0 <= T.host_clock_ms(dev.call, k=3, warmup=2, dev=dev) < 1e3
    assert dev.log == ["call"] * 2 + ["sync"] + ["call"] * 3 + ["sync"]


def test_stat():
    assert T.stat([3, 1, 2]) == {"median": 2, "min": 1, "max": 3}


def test_emit_prints_and_writes_into_a_new_folder(tmp_path, capsys):
    out = tmp_path / "not" / "there" / "yet.json"
    T.emit({"a": {"b": 1.5}}, str(out))
    assert json.loads(capsys.readouterr().out) == {"a": {"b": 1.5}} == json.loads(out.read_text())
    T.emit({"a": 1})                                                      # no file asked for
    assert json.loads(capsys.readouterr().out) == {"a": 1}


def test_event_ms_raises_without_a_device(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    calls = []
    with pytest.raises(RuntimeError):
        T.event_ms(lambda: calls.append(1))
    with pytest.raises(RuntimeError):
        T.host_clock_ms(lambda: calls.append(1), k=1)
    assert calls == []
