"""Breaker events without a GPU: the restatement (tests/breaker_trace.py) against the oracle's breaker states and
against the transcribed CircuitBreakingIntegrationTest cases, and the record's layout against the C compiler."""
import ctypes
import glob
import json
import os
import subprocess

import numpy as np
import pytest

from tests import breaker_trace as B
from tests import local_trace as LT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ restatement == oracle, event by event
@pytest.mark.parametrize("seed", [12, 14, 15, 17])
def test_restatement_states_equal_the_oracle_after_every_event(seed):
    rng = np.random.default_rng(seed)
    n_res = 3
    rules = B.random_rules(rng, n_res)
    s = B.random_stream(rng, rules, 400, n_res)
    kinds = set(int(k) for k in s["kind"])
    assert kinds == {0, 1, 3}, "the stream holds entries, exits and revokes"
    orc = LT.Oracle(n_res, degrade_rules=rules)
    tr = B.BreakerTrace(rules)
    back = 0
    try:
        for i in range(len(s["kind"])):
            one = {k: np.ascontiguousarray(v[i:i + 1]) for k, v in s.items()}
            dec, wait = orc.replay(one)
            k, r, t = int(s["kind"][i]), int(s["resource"][i]), int(s["ts"][i])
            if i and t < int(s["ts"][i - 1]):
                back += 1
            if k == 0:
                kb = tr.entry(i, r, t)
                assert (int(dec[0]), int(wait[0])) == ((0, 0) if kb < 0 else (3, kb)), i
            elif k == 1:
                tr.exit(i, r, t, int(s["rt"][i]), bool(int(s["flags"][i]) & 2))
            else:
                tr.revoke(i, r, t)
            for res in range(n_res):
                assert [orc.cb_state(res, j) for j in range(len(tr.states(res)))] == tr.states(res), (i, res)
    finally:
        orc.close()
    ev = tr.events
    assert back > 0, "no timestamp went back"
    moves = {(e["prev"], e["next"]) for e in ev}
    assert moves == {(0, 1), (1, 2), (2, 1), (2, 0)}, moves
    _SEEN[seed] = ev


_SEEN = {}


def test_random_traces_hold_events_with_two_transitions():
    """Coverage of the traces above, over all seeds: some event moved two breakers, or one breaker twice."""
    for seed in (12, 14, 15, 17):
        if seed not in _SEEN:
            test_restatement_states_equal_the_oracle_after_every_event(seed)
    assert sum(1 for ev in _SEEN.values() for e in ev if e["sub"] > 0) >= 3


def test_probe_at_exactly_next_retry_and_one_before():
    rule = {"resource": 0, "grade": 2, "count": 0, "time_window": 1, "min_request_amount": 1, "stat_interval_ms": 1000}
    orc = LT.Oracle(1, degrade_rules=[rule])
    tr = B.BreakerTrace([rule])
    t0 = 1_700_000_000_000

    def one(kind, t, err=0):
        st = {"kind": np.array([kind], np.uint8), "resource": np.zeros(1, np.uint32), "ts": np.array([t], np.int64),
              "acquire": np.ones(1, np.int32), "flags": np.array([2 if err else 0], np.uint8),
              "rt": np.array([5], np.int64), "param": np.zeros(1, np.uint64)}
        return int(orc.replay(st)[0][0])
    try:
        assert one(0, t0) == 0 and tr.entry(0, 0, t0) < 0
        one(1, t0 + 5, err=1)
        tr.exit(1, 0, t0 + 5, 5, True)
        assert tr.state(0, 0) == B.OPEN == orc.cb_state(0, 0)
        retry = t0 + 5 + 1000
        assert one(0, retry - 1) == 3 and tr.entry(2, 0, retry - 1) == 0
        assert one(0, retry) == 0 and tr.entry(3, 0, retry) < 0
        assert tr.state(0, 0) == B.HALF_OPEN == orc.cb_state(0, 0)
    finally:
        orc.close()
    assert [(e["seq"], e["prev"], e["next"], e["value"]) for e in tr.events] == [(1, 0, 1, 1.0), (3, 1, 2, None)]


# ------------------------------------------------------------------ CircuitBreakingIntegrationTest, transcribed
KATS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "kat_CircuitBreakingIntegrationTest_*.json")))


def test_the_three_kats_are_there():
    assert [os.path.basename(p)[len("kat_CircuitBreakingIntegrationTest_"):-5] for p in KATS] == \
        ["testExceptionRatioMode", "testMultipleHalfOpenedBreakers", "testSlowRequestMode"]


def verify_state(states):
    """CircuitBreakingIntegrationTest.verifyState's sum."""
    return sum(1 if s == B.OPEN else -1 if s == B.HALF_OPEN else -2 for s in states)


@pytest.mark.parametrize("path", KATS, ids=[os.path.basename(p)[4:-5] for p in KATS])
def test_restatement_reproduces_the_kat(path):
    with open(path) as f:
        sc = json.load(f)
    ev, results, states = B.scenario_events(sc, sc["bases"][0])
    assert results == [op["expect"] for op in sc["ops"] if op["op"].startswith("flow_entry")]
    assert [{k: e[k] for k in ("breaker", "prev", "next", "value")} for e in ev] == sc["transitions"]
    for c in sc["state_checks"]:
        assert states[c["after_op"]] == c["states"]
        if "verify_state" in c:
            assert verify_state(states[c["after_op"]]) == c["verify_state"]
    assert states[-1] == sc["final_states"]
    if "final_verify_state" in sc:
        assert verify_state(states[-1]) == sc["final_verify_state"]


def test_blocked_probes_of_the_third_kat_move_twice_in_one_entry():
    with open([p for p in KATS if "MultipleHalfOpened" in p][0]) as f:
        sc = json.load(f)
    ev, results, _ = B.scenario_events(sc, sc["bases"][0])
    blocked = [i for i, r in enumerate(results) if not r]
    assert len(blocked) == 10
    by_seq = {}
    for e in ev:
        by_seq.setdefault(e["seq"], []).append((e["sub"], e["breaker"], e["prev"], e["next"], e["value"]))
    twice = [v for v in by_seq.values() if v == [(0, 0, B.OPEN, B.HALF_OPEN, None), (1, 0, B.HALF_OPEN, B.OPEN, 1.0)]]
    assert len(twice) == 10


# ------------------------------------------------------------------ the record's layout
def test_cb_event_layout_matches_the_c_compiler(tmp_path):
    """sizeof(sga_cb_event) == 40 and every field's offset, as gcc lays the header's struct out, equal the ctypes
    mirror and the numpy dtype the drain reads into."""
    from sentinel_amd import _lib
    from sentinel_amd.local import BREAKER_EVENT_DTYPE
    cls = _lib.SgaCbEvent
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sentinel_amd.h"', "int main(void) {",
             'printf("%zu\\n", sizeof(sga_cb_event));']
    expect = [ctypes.sizeof(cls)]
    for f, _ in cls._fields_:
        lines.append(f'printf("%zu\\n", offsetof(sga_cb_event, {f}));')
        expect.append(getattr(cls, f).offset)
    lines.append("return 0; }")
    src = tmp_path / "cb_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "cb_layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == expect
    assert got[0] == 40
    assert got[1:] == [0, 8, 16, 24, 28, 32, 36, 38, 39]
    assert BREAKER_EVENT_DTYPE.itemsize == 40
    assert [BREAKER_EVENT_DTYPE.fields[f][1] for f, _ in cls._fields_] == got[1:]


def test_library_exports_the_entry_points():
    from sentinel_amd import _lib
    L = _lib.load()
    assert hasattr(L, "sga_cb_events_enable") and hasattr(L, "sga_cb_events_drain")


def test_registry_keeps_observers_in_registration_order():
    """EventObserverRegistry over a sentinel stand-in: no engine is touched until an observer is added."""
    from sentinel_amd.local import BreakerEvent, CircuitBreakerState, EventObserverRegistry

    class Stub:
        enabled = 0

        def enable_breaker_events(self, max_events=0):
            self.enabled += 1
    s = Stub()
    reg = EventObserverRegistry(s)
    assert reg.get_state_change_observers() == [] and s.enabled == 0
    calls = []
    reg.add_state_change_observer("a", lambda *x: calls.append(("a",) + x))
    reg.add_state_change_observer("b", lambda *x: calls.append(("b",) + x))
    assert s.enabled == 2 and len(reg.get_state_change_observers()) == 2
    rule = object()
    O, H = CircuitBreakerState.OPEN, CircuitBreakerState.HALF_OPEN
    reg.dispatch([BreakerEvent(0, 0, 5, 0, 0, 1, O, H, rule, None), BreakerEvent(0, 1, 5, 0, 0, 1, H, O, rule, 1.0)])
    assert calls == [("a", O, H, rule, None), ("b", O, H, rule, None), ("a", H, O, rule, 1.0), ("b", H, O, rule, 1.0)]
    assert reg.remove_state_change_observer("a") and not reg.remove_state_change_observer("a")
    assert len(reg.get_state_change_observers()) == 1
    assert int(CircuitBreakerState.CLOSED) == 0 and int(O) == 1 and int(H) == 2


def test_an_observer_that_raises_loses_no_later_event():
    """The events after the one whose observer raised stay with the sentinel, ahead of whatever comes later."""
    from sentinel_amd.local import BreakerEvent, CircuitBreakerState, EventObserverRegistry

    class Stub:
        def __init__(self):
            self._held_events = []

        def enable_breaker_events(self, max_events=0):
            pass
    s = Stub()
    reg = EventObserverRegistry(s)
    seen = []

    def fn(prev, new, rule, value):
        seen.append(rule)
        if rule == "boom":
            raise RuntimeError("observer")
    reg.add_state_change_observer("a", fn)
    O, H = CircuitBreakerState.OPEN, CircuitBreakerState.HALF_OPEN
    evs = [BreakerEvent(i, 0, 5, 0, 0, 1, O, H, r, None) for i, r in enumerate(["x", "boom", "y", "z"])]
    s._held_events = ["later"]
    with pytest.raises(RuntimeError):
        reg.dispatch(evs)
    assert seen == ["x", "boom"] and s._held_events == evs[2:] + ["later"]
