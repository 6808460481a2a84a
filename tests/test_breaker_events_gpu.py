"""The engine's breaker event log on the GPU: every comparison is full list equality, field by field and value
included, against the restatement of tests/breaker_trace.py over the same events.

  KATs      the three transcribed CircuitBreakingIntegrationTest cases through LocalSentinel.entry / Entry.exit with
            a recording observer
  forms     local_shapes.build_d with the log on: k_cb_flows<1>, k_cb_flows<8>, a second round, the k_cbt_* tiles
            (child process under the test-only build: the dispatch counts say which form ran)
  k_lheavy  breaker-only resources whose chunk mixes entries and exits, the trip on the kHeavyChunk seam, and 17
            breakers (past kHeavyCbs) of which two trip on one exit
  paths     one 300-event trace through every submit path: the same events in the same order
  overflow, off (a twin engine without the log; the entry points' error codes), reload (epochs)
"""
import ctypes as C
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import breaker_trace as B
from tests import local_shapes as ls
from tests import local_trace as lt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = 1_700_000_000_000
FIELDS = ("seq", "sub", "ts", "resource", "breaker", "epoch", "prev", "next", "value")


def got_tuples(recs):
    """The drained records as tuples of FIELDS; value None where the reference passes null."""
    return [(int(r["seq"]), int(r["sub"]), int(r["ts"]), int(r["resource"]), int(r["breaker"]), int(r["epoch"]),
             int(r["prev"]), int(r["next"]), float(r["value"]) if int(r["next"]) == B.OPEN else None) for r in recs]


def exp_tuples(events):
    return [tuple(e[f] for f in FIELDS) for e in events]


def sentinel(n_res, degrade, flow=None, max_batch=1 << 16, log=0, **kw):
    """An engine and its LocalSentinel with the rules loaded; log: the event capacity (0: the default), None: the
    log stays off (the twin)."""
    from sentinel_amd.cluster import Engine
    from sentinel_amd.local import LocalSentinel
    from tests.test_local_parity_gpu import _load
    eng = Engine(max_batch=max_batch)
    s = LocalSentinel(eng, [f"r{i}" for i in range(n_res)], **kw)
    if log is not None:
        s.enable_breaker_events(log)
    _load(s, degrade=list(degrade))
    if flow:
        from sentinel_amd.local import FlowRuleManager
        FlowRuleManager(s).load_rules(flow)
    return eng, s


def submit(s, ch, **kw):
    return s.submit(ch["kind"], ch["resource"], ch["ts"], ch["acquire"], ch["flags"], ch["rt"], ch["param"], **kw)


def same_engine_state(s, twin, degrade, resources, now):
    """Breaker states and node views of a logged engine and its twin."""
    for r in sorted({d["resource"] for d in degrade}):
        for k in range(sum(1 for d in degrade if d["resource"] == r and B.is_valid_rule(d))):
            assert s.circuit_breaker_state(r, k) == twin.circuit_breaker_state(r, k), (r, k)
    for r in resources:
        assert s.node(int(r), now) == twin.node(int(r), now), r


def run_chunks(chunks, n_res, degrade, flow_dicts=(), max_batch=1 << 16, hook=None, predict=None):
    """Every chunk through a logged engine, its twin and the oracle; after each chunk the drained records equal the
    restatement's notifications of that chunk.  Returns (all expected events, dispatch forms per chunk)."""
    from tests.test_configs_fullsize_gpu import _local
    orc = lt.Oracle(n_res, list(flow_dicts), [], list(degrade))
    eng, s = _local(n_res, flow_dicts, (), degrade, max_batch=max_batch)
    teng, twin = _local(n_res, flow_dicts, (), degrade, max_batch=max_batch)
    s.enable_breaker_events()  # after the one rule load: epoch 1, seq from here
    tr = B.BreakerTrace(degrade)
    cb_res = sorted({d["resource"] for d in degrade})
    seq0, forms = 0, []
    try:
        for ci, ch in enumerate(chunks):
            before = {r: orc.cb_state(r, 0) for r in cb_res}
            exp_d, exp_w = orc.replay(ch)
            got_d, got_w = submit(s, ch)
            if hook is not None:
                forms.append(hook())
                if predict is not None:
                    exp_f = predict(ci, before.get)
                    assert forms[-1] == exp_f, (ci, {k: (forms[-1][k], exp_f[k]) for k in exp_f if forms[-1][k] != exp_f[k]})
            tw_d, tw_w = submit(twin, ch)
            if hook is not None:
                hook()  # the read-back counts this process's host chunks: the twin's is not the next chunk's
            assert np.array_equal(got_d, exp_d) and np.array_equal(got_w, exp_w), ci
            assert np.array_equal(got_d, tw_d) and np.array_equal(got_w, tw_w), ci
            n0 = len(tr.events)
            B.replay_stream(tr, ch, seq0, reach=exp_d)
            recs, lost = s.breaker_event_records()
            assert lost == 0
            got, exp = got_tuples(recs), exp_tuples(tr.events[n0:])
            assert got == exp, (ci, len(got), len(exp), [x for x in zip(got, exp) if x[0] != x[1]][:3])
            seq0 += len(ch["kind"])
        now = max(int(ch["ts"].max()) for ch in chunks) + 1
        same_engine_state(s, twin, degrade, cb_res, now)
        assert s.breaker_event_records()[0].size == 0
    finally:
        orc.close()
        eng.close()
        teng.close()
    return tr.events, forms


# ------------------------------------------------------------------ KATs
KATS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "kat_CircuitBreakingIntegrationTest_*.json")))


@pytest.mark.parametrize("path", KATS, ids=[os.path.basename(p)[4:-5] for p in KATS])
def test_kat_through_entry_and_exit_with_an_observer(path):
    from sentinel_amd.cluster import Engine
    from sentinel_amd.local import BlockException, CircuitBreakerState, DegradeRuleManager, LocalSentinel
    from sentinel_amd.rules import DegradeRule
    with open(path) as f:
        sc = json.load(f)
    assert len(KATS) == 3
    base = sc["bases"][0]
    exp_ev, exp_res, exp_states = B.scenario_events(sc, base)
    eng, teng = Engine(max_batch=1 << 12), Engine(max_batch=1 << 12)
    try:
        s = LocalSentinel(eng, ["res"])
        twin = LocalSentinel(teng, ["res"])  # never enables the log: the same calls, the same answers and state
        calls, other = [], []
        s.observers.add_state_change_observer("rec", lambda *a: calls.append(a))
        s.observers.add_state_change_observer("second", lambda *a: other.append(a))
        assert len(s.observers.get_state_change_observers()) == 2
        rules, now, results = None, base, []
        for op in sc["ops"]:
            k = op["op"]
            if k == "set_time":
                now = base + op["t"]
            elif k == "sleep":
                now += op["ms"]
            elif k == "flow_load_degrade":
                rules = [DegradeRule(resource="res", grade=r["grade"], count=r["count"], time_window=r["time_window"],
                                     min_request_amount=r["min_request_amount"],
                                     slow_ratio_threshold=r["slow_ratio_threshold"],
                                     stat_interval_ms=r["stat_interval_ms"]) for r in op["rules"]]
                DegradeRuleManager(s).load_rules(rules)
                DegradeRuleManager(twin).load_rules(rules)
            elif k in ("flow_entry_sleep", "flow_entry_error"):
                n0 = len(calls)
                try:
                    e = s.entry("res", now)
                except BlockException as ex:
                    e, how = None, (type(ex).__name__, ex.rule)
                try:
                    te = twin.entry("res", now)
                except BlockException as ex:
                    te, thow = None, (type(ex).__name__, ex.rule)
                assert (e is None) == (te is None) and (e.wait_ms == te.wait_ms if e else how == thow)
                results.append(e is not None)
                if e is not None:
                    now += op["ms"]
                    if k == "flow_entry_error":
                        e.trace_error()
                        te.trace_error()
                    e.exit(now)
                    te.exit(now)
                assert [s.circuit_breaker_state(0, j) for j in range(len(rules))] == \
                    [twin.circuit_breaker_state(0, j) for j in range(len(rules))]
                assert s.node(0, now) == twin.node(0, now)
                if e is None and "MultipleHalfOpened" in path and len(calls) > n0:
                    # a blocked probe: both transitions were delivered by the time entry() raised
                    O, H = CircuitBreakerState.OPEN, CircuitBreakerState.HALF_OPEN
                    assert calls[n0:] == [(O, H, rules[0], None), (H, O, rules[0], 1.0)]
        assert results == exp_res == [op["expect"] for op in sc["ops"] if op["op"].startswith("flow_entry")]
        want = [(CircuitBreakerState(e["prev"]), CircuitBreakerState(e["next"]), rules[e["breaker"]], e["value"])
                for e in exp_ev]
        assert calls == want
        assert all(c[2] is w[2] for c, w in zip(calls, want)), "the observer receives the loaded DegradeRule object"
        assert other == calls
        assert [(int(c[0]), int(c[1]), rules.index(c[2]), c[3]) for c in calls] == \
            [(t["prev"], t["next"], t["breaker"], t["value"]) for t in sc["transitions"]]
        assert [s.circuit_breaker_state(0, k) for k in range(len(rules))] == sc["final_states"] == exp_states[-1]
        assert s.breaker_events() == []
        assert twin.breaker_event_cap == 0 and twin.node(0, now + 1000) == s.node(0, now + 1000)
    finally:
        eng.close()
        teng.close()


# ------------------------------------------------------------------ children under the test-only build
def _hook():
    from sentinel_amd import _lib
    fn = _lib.load().sga_test_local_dispatch  # the product library does not have it
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_uint32), C.c_size_t]

    def hook():
        out = (C.c_uint32 * 12)()
        assert fn(out, 12) == 12
        return dict(zip(ls.FORM_KEYS, [int(x) for x in out]))
    return hook


def heavy_case(n):
    """Resources 0-2: one exception-count breaker each and n events, entries and exits mixed, the exit whose error
    trips it at the resource's sorted positions 511, 512, 513; later in the chunk the retry time comes, a probe
    passes and its exit closes the breaker.  Resource 3: 17 breakers, two of which trip on the same exit."""
    degrade = [{"resource": r, "grade": 2, "count": 3, "time_window": 1, "min_request_amount": 1,
                "stat_interval_ms": 100000} for r in range(3)]
    for k in range(17):  # breakers 5 and 11 trip at the third error, the others never
        degrade.append({"resource": 3, "grade": 2, "count": 2 if k in (5, 11) else 1000, "time_window": 60,
                        "min_request_amount": 1, "stat_interval_ms": 100000})
    parts = []
    for r, p in enumerate((511, 512, 513)):
        i = np.arange(n)
        kind = np.where((i - p) % 2 == 0, 1, 0)
        kind[0] = 0
        err = np.zeros(n, bool)
        err[[j for j in range(p - 1, 0, -1) if kind[j] == 1][:3]] = True  # three errors before: the count is 3
        err[p] = True                                                       # the fourth trips it (4 > 3)
        parts.append(ls.events(kind, r, T0 + 2 * i, flags=err.astype(np.uint8) * 2, rt=kind * 3))
    i = np.arange(n)
    kind = (i % 2).astype(np.int64)
    err = np.zeros(n, bool)
    err[[101, 301, 601]] = True
    parts.append(ls.events(kind, 3, T0 + 2 * i, flags=err.astype(np.uint8) * 2, rt=kind * 3))
    st = ls.concat(parts)
    o = np.argsort(st["ts"], kind="stable")
    return degrade, {k: np.ascontiguousarray(v[o]) for k, v in st.items()}


def sites_case():
    """Emit sites the shape table's flows do not reach, three chunks over breaker-only resources:
      r0  an OPEN breaker and 16,500 entries, the retry time inside the second tile: the tiled entry flow's probe
          (k_cbt_tiles<0>, k_cbt_fin)
      r1  a CLOSED breaker and 40 exits of which one steps back across a stat window, the trip after it:
          k_cb_flows' step-by-step fall-back
      r2, r3  a probe entry alone in chunk 1, then an exits-only flow in chunk 2 whose first exit is good (r2) or
          bad (r3): the HALF_OPEN exit stepped by k_cb_flows
      r4  66 breakers, past the 64 bits of the entry's mask: all trip on one exit, all probe on one entry, all close
    Resource 5 has no rule: filler that keeps every chunk on the pipeline."""
    one = {"grade": 2, "count": 0, "time_window": 1, "min_request_amount": 1, "stat_interval_ms": 1000}
    degrade = [dict(one, resource=0), dict(one, resource=1, count=3), dict(one, resource=2), dict(one, resource=3)]
    degrade += [dict(one, resource=4) for _ in range(66)]
    fill = lambda n, t: ls.events(0, 5, np.full(n, t))  # noqa: E731
    trip = [ls.events([0, 1], r, [T0, T0 + 1], flags=[0, 2], rt=[0, 1]) for r in (0, 2, 3, 4)]
    c0 = ls.concat(trip + [ls.events(0, 1, T0 + np.arange(40)), fill(1100, T0 + 2)])
    i = np.arange(16500)
    ts1 = T0 + 2000 + 30 * np.arange(40)
    ts1[20] = T0 + 500
    err1 = np.zeros(40, np.uint8)
    err1[22:31] = 2
    c1 = ls.concat([ls.events(0, 0, T0 + 880 + i // 80), ls.events(1, 1, ts1, flags=err1, rt=1),
                    ls.events(0, 2, [T0 + 1100]), ls.events(0, 3, [T0 + 1100]), ls.events(0, 4, [T0 + 1100])])
    c2 = ls.concat([ls.events(1, 2, T0 + 1200 + np.arange(3), flags=[0, 2, 0], rt=1),
                    ls.events(1, 3, T0 + 1200 + np.arange(3), flags=[2, 0, 0], rt=1),
                    ls.events(1, 4, [T0 + 1200], rt=1), fill(1100, T0 + 1300)])
    return degrade, [c0, c1, c2]


def child(what, arg):
    """Runs in a child process with SGA_LIB_VARIANT=testhooks; prints the dispatch forms."""
    hook = _hook()
    if what == "forms":
        c = ls.case(arg)
        ev, forms = run_chunks(c.chunks, c.n_res, c.degrade, c.flow,
                               max_batch=c.max_batch or max(len(ch["kind"]) for ch in c.chunks), hook=hook,
                               predict=lambda ci, cb: ls.predict_forms(c, ci, cb))
        moves = sorted({(e["prev"], e["next"]) for e in ev})
    elif what == "sites":
        degrade, chunks = sites_case()
        ev, forms = run_chunks(chunks, 6, degrade, hook=hook)
        moves = sorted({(e["prev"], e["next"]) for e in ev})
        n0, n1 = len(chunks[0]["kind"]), len(chunks[1]["kind"])
        at = lambda r, lo, hi: [(e["seq"] - lo, e["sub"], e["breaker"], e["prev"], e["next"], e["value"])  # noqa: E731
                                for e in ev if e["resource"] == r and lo <= e["seq"] < hi]
        assert at(0, n0, n0 + n1) == [(121 * 80, 0, 0, 1, 2, None)]            # the probe, in the second tile
        assert 121 * 80 >= ls.K_CB_ROUND
        assert at(1, n0, n0 + n1) == [(16500 + 25, 0, 0, 0, 1, 4.0)]           # the trip, after the step back
        assert at(2, n0 + n1, 1 << 40) == [(0, 0, 0, 2, 0, None), (1, 0, 0, 0, 1, 1.0)]
        assert at(3, n0 + n1, 1 << 40) == [(3, 0, 0, 2, 1, 1.0)]
        assert at(4, n0, n0 + n1) == [(16500 + 42, k, k, 1, 2, None) for k in range(66)]
        assert [x[1:] for x in at(4, 0, n0)] == [(k, k, 0, 1, 1.0) for k in range(66)]
        assert [x[1:] for x in at(4, n0 + n1, 1 << 40)] == [(k, k, 2, 0, None) for k in range(66)]
    else:
        n = int(arg)
        degrade, st = heavy_case(n)
        ev, forms = run_chunks([st], 4, degrade, hook=hook)
        moves = sorted({(e["prev"], e["next"]) for e in ev})
        trips = [e for e in ev if (e["prev"], e["next"]) == (0, 1)]
        for r, p in enumerate((511, 512, 513)):  # the trip is the event at the resource's sorted position p
            mine = np.nonzero(st["resource"] == r)[0]
            assert [e["seq"] for e in trips if e["resource"] == r] == [int(mine[p])], (r, p)
            assert [e["value"] for e in trips if e["resource"] == r] == [4.0]
        both = [(e["sub"], e["breaker"], e["value"]) for e in trips if e["resource"] == 3]
        assert both == [(0, 5, 3.0), (1, 11, 3.0)], both
    print("FORMS", json.dumps({"forms": forms, "moves": moves, "events": len(ev)}))


def run_child(what, arg):
    from sentinel_amd import _lib
    assert not hasattr(C.CDLL(_lib.LIB_PATH), "sga_test_local_dispatch")
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_breaker_events_gpu import child; "
            f"child({what!r}, {arg!r})")
    env = dict(os.environ, SGA_LIB_VARIANT="testhooks")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    line = [x for x in r.stdout.splitlines() if x.startswith("FORMS ")][-1]
    print(what, arg, line)
    return json.loads(line[6:])


@pytest.mark.parametrize("name", ["D4k", "D8k", "D16k"])
def test_forms(name):
    """build_d's flows trip at exits 1023 / 1024, 2047, 4094 / 4095 / 4096, 8190 / 8191 / 8192 and 16384 and at
    count == minRequestAmount, are probed at exactly the retry time and closed or reopened in the last chunk; the
    dispatch counts (compared with predict_forms in the child) say that the breaker-flow kernels decided them."""
    out = run_child("forms", name)
    tot = {k: sum(f[k] for f in out["forms"]) for k in ls.FORM_KEYS}
    assert tot["cb"] > 0 and tot["small"] == 0
    if name == "D16k":
        assert tot["tiled"] >= 1
    assert [tuple(m) for m in out["moves"]] == [(0, 1), (1, 2), (2, 0), (2, 1)]


def test_emit_sites_outside_the_shape_table():
    """sites_case: the tiled entry flow's probe, k_cb_flows' step-by-step fall-back and its stepped HALF_OPEN exit,
    and probes of breakers past the entry's 64-bit mask; the dispatch counts say that the breaker-flow kernels (and
    the tiles) took the flows."""
    out = run_child("sites", "")
    f = out["forms"]
    assert [x["small"] for x in f] == [0, 0, 0]
    assert f[1]["tiled"] == 1 and f[1]["cb"] == 4 and f[2]["cb"] == 2
    assert [tuple(m) for m in out["moves"]] == [(0, 1), (1, 2), (2, 0), (2, 1)]


@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_lheavy(n):
    out = run_child("heavy", n)
    f = out["forms"][0]
    assert f["heavy"] == (4 if n >= ls.K_HEAVY else 0) and f["small"] == 0 and f["cb"] == 0
    assert [tuple(m) for m in out["moves"]] == [(0, 1), (1, 2), (2, 0)]


# ------------------------------------------------------------------ paths
PATH_RULES = [{"resource": r, "grade": g, "count": c, "time_window": w, "min_request_amount": 1,
               "stat_interval_ms": 1000, "slow_ratio_threshold": 0.5}
              for r in range(2) for g, c, w in ((2, 1, 1), (0, 20, 2))]
N_PATH = 300
_PATH = {}


def path_trace():
    """The one trace of the paths test and what the restatement says of it (computed once)."""
    if not _PATH:
        rng = np.random.default_rng(43)
        st = B.random_stream(rng, PATH_RULES, N_PATH, 2, t0=T0)
        dec = []  # per event: None, or the entry's (decision, wait) -- a degrade block's detail is the breaker's index
        tr = B.BreakerTrace(PATH_RULES)
        for i in range(N_PATH):
            k, r, t = int(st["kind"][i]), int(st["resource"][i]), int(st["ts"][i])
            if k == 0:
                kb = tr.entry(i, r, t)
                dec.append((0, 0) if kb < 0 else (3, kb))
                continue
            dec.append(None)
            if k == 1:
                tr.exit(i, r, t, int(st["rt"][i]), bool(int(st["flags"][i]) & 2))
            else:
                tr.revoke(i, r, t)
        by_seq = {}
        for e in tr.events:
            by_seq.setdefault(e["seq"], []).append(e)
        kind = st["kind"]
        # a probe that the second breaker blocks; a probe that a revoke takes back; a bad and a good probe exit
        assert any(kind[q] == 0 and [(e["breaker"], e["prev"], e["next"]) for e in v] == [(0, 1, 2), (0, 2, 1)]
                   for q, v in by_seq.items())
        assert any(kind[q] == 3 and any((e["prev"], e["next"]) == (2, 1) for e in v) for q, v in by_seq.items())
        assert any(kind[q] == 1 and any((e["prev"], e["next"], e["value"]) == (2, 1, 1.0) for e in v)
                   for q, v in by_seq.items())
        assert any(kind[q] == 1 and any((e["prev"], e["next"]) == (2, 0) for e in v) for q, v in by_seq.items())
        n_fill = 1025 - N_PATH
        padded = ls.concat([st, ls.events(0, 2, np.full(n_fill, int(st["ts"][-1])))])
        _PATH.update(st=st, padded=padded, events=exp_tuples(tr.events), dec=dec)
    return _PATH


def check_decisions(p, got_d, got_w):
    for i, d in enumerate(p["dec"]):
        if d is not None:
            assert (int(got_d[i]), int(got_w[i])) == d, i


@pytest.mark.parametrize("path", ["small", "pipeline", "seq", "relate", "origin", "context", "device", "event_one"])
def test_paths(path):
    from sentinel_amd.local import SystemRule, SystemRuleManager
    from sentinel_amd.rules import FlowRule, RuleConstant
    p = path_trace()
    st, kw, flow, sub = p["st"], {}, None, {}
    if path in ("pipeline", "relate", "origin", "context"):
        st = p["padded"]
    if path == "relate":
        flow = [FlowRule(resource="r0", count=1e12, strategy=RuleConstant.STRATEGY_RELATE, ref_resource="r1")]
    if path == "origin":
        kw = {"origins": ["appA"]}
        flow = [FlowRule(resource="r0", count=1e12, limit_app="appA"), FlowRule(resource="r1", count=1e12, limit_app="appA")]
        sub = {"origin": np.ones(len(st["kind"]), np.uint32)}
    if path == "context":
        kw = {"contexts": ["ctxA"]}
        flow = [FlowRule(resource=f"r{r}", count=1e12, strategy=RuleConstant.STRATEGY_CHAIN, ref_resource="ctxA")
                for r in range(2)]
        sub = {"context": np.ones(len(st["kind"]), np.uint32)}
    if path == "seq":
        st = dict(st, flags=st["flags"] | np.uint8(8))

    def drive(log):
        """The trace through `path` on a fresh engine; log None: the twin that never enables the log."""
        eng, s = sentinel(3, PATH_RULES, flow=flow, log=log, **kw)
        try:
            return eng, s, run(s)
        except BaseException:
            eng.close()
            raise

    def run(s):
        if path == "seq":
            SystemRuleManager(s).load_rules([SystemRule(qps=1e12)])
        if path == "device":
            import torch
            base = int(st["ts"].min())
            dev = (lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).cuda())
            d, w = s.submit_device(dev(st["kind"], np.uint8), dev(st["resource"], np.int32), base,
                                   dev(st["ts"] - base, np.int32), dev(st["acquire"], np.int32),
                                   dev(st["flags"], np.uint8), dev(st["rt"], np.int64),
                                   dev(st["param"].astype(np.int64), np.int64))
            s.device_status()
            return d.cpu().numpy(), w.cpu().numpy()
        if path == "event_one":
            out = [s.event_one(int(st["kind"][i]), int(st["resource"][i]), int(st["ts"][i]), 1, int(st["flags"][i]),
                               int(st["rt"][i])) for i in range(N_PATH)]
            return np.array([o[0] for o in out]), np.array([o[1] for o in out])
        return submit(s, st, **sub)

    eng, s, (got_d, got_w) = drive(0)
    try:
        teng, twin, (tw_d, tw_w) = drive(None)
        try:
            check_decisions(p, got_d, got_w)
            recs, lost = s.breaker_event_records()
            assert lost == 0
            assert got_tuples(recs) == p["events"]
            for r in range(2):
                assert [s.circuit_breaker_state(r, k) for k in range(2)] == _final_states(p)[r]
            # the twin: the same decisions and waits on every event, the same breakers, the same node views
            assert twin.breaker_event_cap == 0
            assert np.array_equal(got_d, tw_d) and np.array_equal(got_w, tw_w)
            same_engine_state(s, twin, PATH_RULES, range(3), int(st["ts"].max()) + 1)
        finally:
            teng.close()
    finally:
        eng.close()


def _final_states(p):
    if "final" not in p:
        tr = B.BreakerTrace(PATH_RULES)
        B.replay_stream(tr, p["st"], 0)
        p["final"] = {r: tr.states(r) for r in range(2)}
    return p["final"]


# ------------------------------------------------------------------ overflow
def cycle_stream(cycles, t=T0, first=True, last_probe=True):
    """One resource, one exception-count breaker (count 0, recovery 1 s): a failing request trips it; then every
    cycle is a probe at exactly the retry time and its failing exit.  Returns (stream, next time)."""
    ev = []
    if first:
        ev += [(0, t, 0), (1, t + 1, 2)]
        t += 1
    for _ in range(cycles):
        t += 1000
        ev += [(0, t, 0), (1, t + 1, 2)]
        t += 1
    if last_probe:
        t += 1000
        ev += [(0, t, 0)]
    a = np.array(ev, np.int64)
    return ls.events(a[:, 0], 0, a[:, 1], flags=a[:, 2], rt=a[:, 0]), t


OVF_RULE = [{"resource": 0, "grade": 2, "count": 0, "time_window": 1, "min_request_amount": 1, "stat_interval_ms": 1000}]


def test_overflow_keeps_the_first_records_and_counts_the_rest():
    st, t = cycle_stream(49)  # 1 + 2 * 49 + 1 transitions
    tr = B.BreakerTrace(OVF_RULE)
    dec = []
    B.replay_stream(tr, st, 0, decisions=dec)
    assert len(tr.events) == 100
    eng, s = sentinel(1, OVF_RULE, log=64)
    teng, twin = sentinel(1, OVF_RULE, log=None)
    try:
        assert s.breaker_event_cap == 64
        got_d, got_w = submit(s, st)
        tw_d, tw_w = submit(twin, st)
        recs, lost = s.breaker_event_records()
        assert got_tuples(recs) == exp_tuples(tr.events[:64])
        assert lost == 36
        assert np.array_equal(got_d, tw_d) and np.array_equal(got_w, tw_w)
        assert [int(d) for d, e in zip(got_d, dec) if e is not None] == [e for e in dec if e is not None]
        same_engine_state(s, twin, OVF_RULE, [0], t + 1)
        assert s.circuit_breaker_state(0, 0) == B.HALF_OPEN == tr.state(0, 0)
        # the log goes on where the stream does: the lost counter is cleared, seq counts every submitted event
        more = ls.events([1], 0, [t + 1], flags=[2], rt=[1])
        submit(s, more)
        tr.exit(len(st["kind"]), 0, t + 1, 1, True)
        recs, lost = s.breaker_event_records()
        assert (got_tuples(recs), lost) == (exp_tuples(tr.events[100:]), 0) and len(recs) == 1
    finally:
        eng.close()
        teng.close()


# ------------------------------------------------------------------ off, and the entry points' answers
def test_entry_points_without_the_log_and_with_records_pending():
    from sentinel_amd import _lib
    from sentinel_amd.local import BREAKER_EVENT_DTYPE
    L = _lib.load()
    st, t = cycle_stream(0, last_probe=False)  # one trip
    eng, s = sentinel(1, OVF_RULE, log=None)
    try:
        buf = np.zeros(8, BREAKER_EVENT_DTYPE)
        n, lost = C.c_size_t(7), C.c_uint64(7)
        submit(s, st)
        assert L.sga_cb_events_drain(eng.handle, buf.ctypes.data, 8, C.byref(n), C.byref(lost)) == _lib.SGA_EINVAL
        assert s.breaker_event_cap == 0 and s.circuit_breaker_state(0, 0) == B.OPEN
        # enabled now: seq counts from here, and the trip before it is not in the log
        assert L.sga_cb_events_enable(eng.handle, 0) == 0
        assert L.sga_cb_events_drain(eng.handle, buf.ctypes.data, 8, C.byref(n), None) == 0 and n.value == 0
        probe, _ = cycle_stream(1, t=t, first=False, last_probe=False)  # O -> HO, HO -> O
        submit(s, probe)
        assert L.sga_cb_events_enable(eng.handle, 128) == _lib.SGA_EINVAL  # records pending
        assert L.sga_cb_events_drain(eng.handle, None, 0, C.byref(n), C.byref(lost)) == _lib.SGA_ERANGE
        assert n.value == 2
        assert L.sga_cb_events_drain(eng.handle, buf.ctypes.data, 1, C.byref(n), C.byref(lost)) == _lib.SGA_ERANGE
        assert n.value == 2  # nothing was removed
        assert L.sga_cb_events_drain(eng.handle, buf.ctypes.data, 8, C.byref(n), C.byref(lost)) == 0
        assert n.value == 2 and lost.value == 0
        assert [(x[0], x[1], x[6], x[7], x[8]) for x in got_tuples(buf[:2])] == [(0, 0, 1, 2, None), (1, 0, 2, 1, 1.0)]
        assert L.sga_cb_events_enable(eng.handle, 100) == 0  # empty: resized (to 128)
        assert L.sga_cb_events_drain(eng.handle, buf.ctypes.data, 8, C.byref(n), None) == 0 and n.value == 0
    finally:
        eng.close()


# ------------------------------------------------------------------ reload
def test_reload_keeps_old_records_on_their_epoch():
    from sentinel_amd.cluster import Engine
    from sentinel_amd.local import CircuitBreakerState as S
    from sentinel_amd.local import DegradeRuleManager, LocalSentinel
    from sentinel_amd.rules import DegradeRule
    eng, teng = Engine(max_batch=1 << 12), Engine(max_batch=1 << 12)
    try:
        s = LocalSentinel(eng, ["r0"])
        twin = LocalSentinel(teng, ["r0"])  # the same loads and events, the log never enabled
        tmgr = DegradeRuleManager(twin)
        s.enable_breaker_events()
        mgr = DegradeRuleManager(s)
        a = DegradeRule(resource="r0", grade=2, count=0, time_window=1, min_request_amount=1, stat_interval_ms=1000)
        b = DegradeRule(resource="r0", grade=2, count=1000, time_window=1, min_request_amount=1, stat_interval_ms=1000)
        mgr.load_rules([a])
        tmgr.load_rules([a])
        st, t = cycle_stream(0, last_probe=False)
        d0 = submit(s, st)  # trips a: one record pending, epoch 1, k 0
        t0 = submit(twin, st)
        mgr.load_rules([b, a])  # a unchanged keeps its breaker and is k 1 now; the load drains first
        tmgr.load_rules([b, a])
        assert [s.circuit_breaker_state(0, k) for k in range(2)] == [B.CLOSED, B.OPEN]
        old = s.breaker_events()
        assert [(e.seq, e.epoch, e.breaker, e.prev_state, e.new_state, e.snapshot_value) for e in old] == \
            [(1, 1, 0, S.CLOSED, S.OPEN, 1.0)]
        assert old[0].rule is a
        assert s.breaker_events() == []  # the reload itself emitted nothing
        probe, _ = cycle_stream(0, t=t, first=False, last_probe=True)
        d1 = submit(s, probe)
        t1 = submit(twin, probe)
        for got, tw in ((d0, t0), (d1, t1)):
            assert np.array_equal(got[0], tw[0]) and np.array_equal(got[1], tw[1])
        assert [twin.circuit_breaker_state(0, k) for k in range(2)] == [B.CLOSED, B.HALF_OPEN] == \
            [s.circuit_breaker_state(0, k) for k in range(2)]
        assert s.node(0, t + 2000) == twin.node(0, t + 2000) and twin.breaker_event_cap == 0
        new = s.breaker_events()
        assert [(e.seq, e.epoch, e.breaker, e.prev_state, e.new_state, e.snapshot_value) for e in new] == \
            [(2, 2, 1, S.OPEN, S.HALF_OPEN, None)]
        assert new[0].rule is a
    finally:
        eng.close()
        teng.close()
