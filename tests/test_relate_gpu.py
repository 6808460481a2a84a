"""GPU parity of FlowRules with strategy RELATE (FlowRuleChecker.java:96-116): resources linked by such rules
form a group whose events one lane decides in arrival order (k_lsmall, k_lflows inline, k_lgroup, k_lseq).

Bar: decisions and waits bit-identical to tests/relate_trace.py (the oracle driven event by event), and every
node getter of every resource identical at the stream's last timestamp.  The streams are built once per
configuration and shared by the cases that run them through different paths."""
import functools

import numpy as np
import pytest

from tests import local_trace as lt
from tests import relate_trace as rt

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000
NONE = 0xFFFFFFFF
ENTRY = 0xFFFFFFFF
RELATE = 1


# ------------------------------------------------------------------ engine side
def _sentinel(n_res, max_batch=1 << 16, small=None):
    from sentinel_amd.cluster import Engine
    from sentinel_amd.local import LocalSentinel
    eng = Engine(max_batch=max_batch)
    if small is not None:
        eng.set_small_batch(small)
    return eng, LocalSentinel(eng, [f"r{i}" for i in range(n_res)])


def _load_flow(s, rules):
    from sentinel_amd.local import FlowRuleManager
    from sentinel_amd.rules import FlowRule
    out = []
    for r in rules:
        ref = None
        if rt.is_relate(r):
            ref = "no-such-resource" if r.get("ref") is None else f"r{r['ref']}"
        out.append(FlowRule(resource=f"r{r['resource']}", count=r["count"], grade=r.get("grade", 1),
                            control_behavior=r.get("control_behavior", 0),
                            warm_up_period_sec=r.get("warm_up_period_sec", 10),
                            max_queueing_time_ms=r.get("max_queueing_time_ms", 500),
                            strategy=r.get("strategy", 0), ref_resource=ref))
    return FlowRuleManager(s).load_rules(out)


def _submit(s, st):
    return s.submit(st["kind"], st["resource"], st["ts"], st["acquire"], st["flags"], st["rt"], st["param"])


def _same(st, got, ed, ew, what):
    gd, gw = got
    bad = np.nonzero((gd != ed) | (gw != ew))[0]
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(gd)} events differ; first at {i}: kind={st['kind'][i]} "
                             f"res={st['resource'][i]} ts={st['ts'][i]} acq={st['acquire'][i]} "
                             f"flags={st['flags'][i]} gpu=({gd[i]},{gw[i]}) expected=({ed[i]},{ew[i]})")


def _nodes(s, tr, what):
    for rid, exp in tr["nodes"].items():
        v = s.node(rid, tr["t_end"])
        got = [getattr(v, g) for g in lt.NODE_GETTERS]
        assert got == exp, (what, rid, list(zip(lt.NODE_GETTERS, got, exp)))


def _finish(h, n_res, entry=False):
    """Ends the helper's stream: the trace the cases share (the node getters read once, at the last time)."""
    h.flush()
    st, ed, ew = h.stream()
    t_end = int(np.array([e[2] for e in h.ev]).max())
    nodes = {rid: h.node(rid, t_end) for rid in list(range(n_res)) + ([ENTRY] if entry else [])}
    tr = {"st": st, "ed": ed, "ew": ew, "t_end": t_end, "nodes": nodes, "counts": h.counts()}
    h.close()
    return tr


def _not_vacuous(tr):
    c = tr["counts"]
    assert c["blocks"] >= 100 and c["passes"] >= 100 and c["null"] >= 10, c


def _run(tr, rules, n_res, what, max_batch=1 << 16, small=None, groups=None):
    eng, s = _sentinel(n_res, max_batch, small)
    assert _load_flow(s, rules) == len(rules)
    for rid, lead in (groups or {}).items():
        assert s.group_of(rid) == lead, (rid, s.group_of(rid), lead)
    _same(tr["st"], _submit(s, tr["st"]), tr["ed"], tr["ew"], what)
    _nodes(s, tr, what)
    eng.close()


# ------------------------------------------------------------------ case 1 / 6 / 7 / 9: the pair
def _pair_rules(grade):
    a = {"resource": 0, "count": 20, "strategy": RELATE, "ref": 1} if grade == 1 else \
        {"resource": 0, "count": 3, "grade": 0, "strategy": RELATE, "ref": 1}
    return [a, {"resource": 1, "count": 50}, {"resource": 2, "count": 10}]


PAIR_RES = 4  # A, B, C and a bystander
PAIR_GROUPS = {0: 0, 1: 0, 2: NONE, 3: NONE}
PATHS = [("small", 1000, None), ("pipeline", 1 << 16, 0), ("pipeline_chunks", 4096, 0)]


@functools.lru_cache(maxsize=None)
def _pair_trace(grade, regress=0.0, inbound=False):
    """A -> B (QPS count 20, or THREAD count 3), B DIRECT 50, C DIRECT 10; 6000 entries, mean gap 2 ms, acquire
    1-2, rt 0-39, resources 0.4 / 0.4 / 0.2 after 50 entries on A and C only."""
    h = rt.RelateTrace(PAIR_RES, _pair_rules(grade), system=[{"qps": 1e9}] if inbound else None)
    h.generate(6000, 41 + grade, T0, [0.4, 0.4, 0.2], gap_mean=2.0, acq_max=2, rt_max=39, warm=50,
               warm_weights=[0.5, 0.0, 0.5], regress_pct=regress, inbound=inbound)
    tr = _finish(h, PAIR_RES, entry=inbound)
    _not_vacuous(tr)
    return tr


@pytest.mark.parametrize("path,max_batch,small", PATHS, ids=[p[0] for p in PATHS])
@pytest.mark.parametrize("grade", [1, 0], ids=["qps", "thread"])
def test_pair(grade, path, max_batch, small):
    """The small path (chunks of 1000 through k_lsmall) and the pipeline (one chunk, and chunks of 4096: the
    group's state carries across chunk boundaries)."""
    _run(_pair_trace(grade), _pair_rules(grade), PAIR_RES, f"pair {grade} {path}", max_batch, small, PAIR_GROUPS)


@pytest.mark.parametrize("path,max_batch,small", PATHS[:2], ids=[p[0] for p in PATHS[:2]])
def test_pair_clock_regressions(path, max_batch, small):
    """5 % of the entries stamped up to 800 ms back."""
    _run(_pair_trace(1, 0.05), _pair_rules(1), PAIR_RES, f"regress {path}", max_batch, small)


def test_pair_device_entry():
    """sga_submit_events_device decides the stream as the host entry does."""
    from tests.test_local_device_gpu import _dev
    tr = _pair_trace(1)
    eng, s = _sentinel(PAIR_RES, 1 << 13)
    _load_flow(s, _pair_rules(1))
    st = tr["st"]
    n, lo, k = len(st["kind"]), 0, 0
    sizes = [4000, 1500, 3100, 700, 100]
    while lo < n:
        hi = min(n, lo + sizes[k % len(sizes)])
        sub = lt.slice_stream(st, lo, hi)
        _same(sub, _dev(s, sub), tr["ed"][lo:hi], tr["ew"][lo:hi], f"device chunk at {lo}")
        lo, k = hi, k + 1
    _nodes(s, tr, "device")
    eng.close()


def test_pair_sequential_lane():
    """A SystemRule that never blocks (qps 1e9) and inbound events only: every chunk takes k_lseq.  ENTRY_NODE
    counts as the oracle's does."""
    from sentinel_amd.local import SystemRule, SystemRuleManager
    tr = _pair_trace(1, 0.0, True)
    eng, s = _sentinel(PAIR_RES, 4096, 0)
    _load_flow(s, _pair_rules(1))
    SystemRuleManager(s).load_rules([SystemRule(qps=1e9)])
    _same(tr["st"], _submit(s, tr["st"]), tr["ed"], tr["ew"], "k_lseq")
    _nodes(s, tr, "k_lseq")
    eng.close()


# ------------------------------------------------------------------ case 2: group shapes
SHAPE_RES = 12
SHAPE_RULES = [
    {"resource": 0, "count": 6, "strategy": RELATE, "ref": 1},             # chain 0 -> 1 -> 2, DIRECT rules on 2
    {"resource": 1, "count": 6, "strategy": RELATE, "ref": 2},
    {"resource": 2, "count": 8}, {"resource": 2, "count": 4, "grade": 0},
    {"resource": 3, "count": 10},                                          # a bystander with a rule
    {"resource": 4, "count": 6, "strategy": RELATE, "ref": 5},             # cycle 4 <-> 5
    {"resource": 5, "count": 6, "strategy": RELATE, "ref": 4},
    {"resource": 6, "count": 6, "strategy": RELATE, "ref": 7},             # two rules, two refs
    {"resource": 6, "count": 2, "grade": 0, "strategy": RELATE, "ref": 8},
    {"resource": 7, "count": 30}, {"resource": 8, "count": 12},
    {"resource": 9, "count": 5, "strategy": RELATE, "ref": 9},             # ref == self
    {"resource": 10, "count": 0, "strategy": RELATE, "ref": None},         # SGA_REF_NONE: never blocks
]
SHAPE_GROUPS = {0: 0, 1: 0, 2: 0, 3: NONE, 4: 4, 5: 4, 6: 6, 7: 6, 8: 6, 9: 9, 10: NONE, 11: NONE}


@functools.lru_cache(maxsize=None)
def _shape_trace():
    h = rt.RelateTrace(SHAPE_RES, SHAPE_RULES)
    h.generate(9000, 51, T0, [1.0] * SHAPE_RES, gap_mean=0.7, acq_max=2, rt_max=39)
    tr = _finish(h, SHAPE_RES)
    _not_vacuous(tr)
    return tr


@pytest.mark.parametrize("path,max_batch,small", PATHS[:2], ids=[p[0] for p in PATHS[:2]])
def test_group_shapes(path, max_batch, small):
    """A chain, a cycle, two RELATE rules with different refs on one resource, ref == self, and a rule whose ref
    names no resource (valid, counted as loaded, never blocks even with count 0); group_of reports each
    component's smallest member and SGA_REF_NONE for bystanders."""
    tr = _shape_trace()
    ten = tr["st"]["resource"] == 10
    assert ten.sum() > 100 and (tr["ed"][ten] == 0).all()
    _run(tr, SHAPE_RULES, SHAPE_RES, f"shapes {path}", max_batch, small, SHAPE_GROUPS)


@pytest.mark.parametrize("small", [None, 0], ids=["small", "pipeline"])
@pytest.mark.parametrize("first", ["pass", "blocked", "kind2"])
def test_count_zero_blocks_from_the_refs_first_entry(first, small):
    """RELATE 0 -> 1 with count 0 passes until resource 1's first event and blocks from then on, within one
    chunk: that first event is an entry that passes, an entry its own rule blocks, or a kind-2 event."""
    rules = [{"resource": 0, "count": 0, "strategy": RELATE, "ref": 1}]
    if first == "blocked":
        rules.append({"resource": 1, "count": 0})
    h = rt.RelateTrace(3, rules)
    t = T0
    for _ in range(3):
        t += 3
        assert h.step(0, t, t)[0] == 0
        h.step(2, t, t)
    t += 3
    if first == "kind2":
        h.other(2, 1, t)
    else:
        assert h.step(1, t, t)[0] == (1 if first == "blocked" else 0)
    for _ in range(3):
        t += 3
        assert h.step(0, t, t) == (1, 0)
        h.step(2, t, t)
    tr = _finish(h, 3)
    _run(tr, rules, 3, f"count 0, {first}", 1 << 12, small, {0: 0, 1: 0, 2: NONE})


# ------------------------------------------------------------------ case 3: segment lengths
# kGroupEvents (flow.hip) = 128: a group with fewer events in a chunk replays on its k_lflows lane, one with
# 128 or more by a wave of k_lgroup (tiles of 256 events: 1023 / 1024 / 1025 and 5000 cross tile ends)
LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 5000]
SEG_RES = 6
SEG_RULES = [{"resource": 0, "count": 3, "grade": 0, "strategy": RELATE, "ref": 1}, {"resource": 1, "count": 300},
             {"resource": 2, "count": 10}, {"resource": 3, "count": 20, "control_behavior": 2,
                                            "max_queueing_time_ms": 50},
             {"resource": 4, "count": 3, "grade": 0}]


@functools.lru_cache(maxsize=None)
def _segment_trace():
    """One chunk per length: the group {0, 1} gets exactly that many events (entries and exits) in it, the
    unrelated resources 2..5 share it.  Resource 1 stays unentered until 40 group events into the chunk of
    129: up to there every entry on 0 is a null-node pass, on the lane (below 128) and in k_lgroup (128, 129)."""
    h = rt.RelateTrace(SEG_RES, SEG_RULES)
    rng = np.random.default_rng(61)
    t = float(T0)
    bounds = [0]
    b_open = False
    for L in LENGTHS:
        cnt, extra, pre = 0, 0, 0
        while True:
            t += rng.exponential(1.0)
            now = int(t)
            full = False
            while h.heap and h.heap[0][0] <= now and not full:
                if h.heap[0][2] < 2 and cnt >= L:
                    full = True  # a group exit is due and the chunk has its share: the chunk ends here
                else:
                    cnt += 1 if h.pop_one() < 2 else 0
            if full or (cnt >= L and extra >= 150):
                break
            grp = pre >= 20 and cnt < L and rng.random() < 0.7
            b_open = b_open or (L == 129 and cnt >= 40)
            rid = (int(rng.integers(0, 2)) if b_open else 0) if grp else int(rng.integers(2, SEG_RES))
            h.step(rid, now, now, int(rng.integers(1, 3)), int(rng.integers(0, 40)), pop=False)
            cnt += 1 if grp else 0
            extra += 1 if cnt >= L and not grp else 0
            pre += 0 if grp else 1
        assert cnt == L, (cnt, L)
        bounds.append(h.mark())
    tr = _finish(h, SEG_RES)  # the exits still pending follow as a last chunk
    tr["bounds"] = bounds
    _not_vacuous(tr)
    return tr


def test_segment_lengths():
    tr = _segment_trace()
    st = tr["st"]
    eng, s = _sentinel(SEG_RES, 1 << 16, 0)
    _load_flow(s, SEG_RULES)
    for L, a, b in zip(LENGTHS, tr["bounds"], tr["bounds"][1:]):
        sub = lt.slice_stream(st, a, b)
        assert int((sub["resource"] < 2).sum()) == L and b - a > L
        _same(sub, _submit(s, sub), tr["ed"][a:b], tr["ew"][a:b], f"group segment of {L}")
    a = tr["bounds"][-1]
    if a < len(st["kind"]):
        sub = lt.slice_stream(st, a, len(st["kind"]))
        _same(sub, _submit(s, sub), tr["ed"][a:], tr["ew"][a:], "pending exits")
    _nodes(s, tr, "segments")
    eng.close()


# ------------------------------------------------------------------ case 4: RateLimiter ignores the node
def test_rate_limiter_relate():
    """RELATE RateLimiter 0 -> 1: before resource 1 is entered the rule passes and latestPassedTime stays
    untouched; from then on it is the DIRECT RateLimiter on 0 with a fresh rater (the controller never reads
    the node).  The oracle therefore holds no rule in the first phase and gets the DIRECT rule, whose rater
    starts fresh, at resource 1's first entry."""
    rl = {"resource": 0, "count": 10, "control_behavior": 2, "max_queueing_time_ms": 500}
    h = rt.RelateTrace(2, [])
    t = T0
    for _ in range(200):
        t += 1
        assert h.step(0, t, t, rt=5) == (0, 0)
    t += 1
    h.step(1, t, t, rt=5)
    h.load([rl])
    h.t = t
    h.generate(3000, 71, T0, [0.7, 0.3], gap_mean=8.0, acq_max=2, rt_max=20)
    tr = _finish(h, 2)
    d = tr["ed"][(tr["st"]["resource"] == 0) & (tr["st"]["kind"] == 0)][200:]
    assert (d == 1).sum() >= 100 and (d == 0).sum() >= 100
    for small in (None, 0):
        _run(tr, [dict(rl, strategy=RELATE, ref=1)], 2, f"rate limiter small={small}", 1 << 16, small, {0: 0, 1: 0})


# ------------------------------------------------------------------ case 5: a transparent rule, all controllers
@functools.lru_cache(maxsize=None)
def _transparent_trace():
    """8 pairs (A_k = 2k, B_k = 2k + 1) with the random controller mix of test_local_parity_gpu.  A_k carries
    [RELATE -> B_k, count 1e9] and then its own rules rewritten as RELATE -> A_k: the oracle holds them as the
    DIRECT rules they equal, the helper reads B_k's passQps before each entry on A_k once B_k has been entered
    (the transparent rule's only effect: the window rotation), and FLOW block details on A_k shift by one.  The
    first 80 entries go to the A side only: null-node passes of every controller before its B_k is entered."""
    from tests.test_local_parity_gpu import _random_flow_rules
    rng = np.random.default_rng(81)
    n_res = 16
    flow = []
    for r in _random_flow_rules(rng, n_res):
        if r["resource"] % 2 == 0:
            r = dict(r, strategy=RELATE, ref=r["resource"])
        flow.append(r)
    flow = [{"resource": a, "count": 1e9, "strategy": RELATE, "ref": a + 1} for a in range(0, n_res, 2)] + flow
    param = [{"resource": r, "count": float(rng.integers(2, 9))} for r in (1, 5, 9)]
    degrade = [{"resource": r, "grade": r % 3, "count": [40.0, 0.3, 5.0][r % 3], "slow_ratio_threshold": 0.5,
                "time_window": 1, "min_request_amount": 3} for r in (0, 3, 4, 7, 10)]
    h = rt.RelateTrace(n_res, flow, param, degrade, self_direct=True)
    h.generate(12000, 82, T0, [1.0] * n_res, gap_mean=0.4, acq_max=3, rt_max=40, prio_pct=0.15, err_pct=0.1,
               params=5, param_res=(1, 5, 9), regress_pct=0.01, warm=80, warm_weights=[1.0, 0.0] * (n_res // 2))
    tr = _finish(h, n_res)
    tr["rules"] = (flow, param, degrade)
    # not vacuous: the transparent rule never blocks by construction, so the RELATE blocks counted here are the
    # FLOW blocks of the A_k's own (self-referencing) rules
    c = tr["counts"]
    on_a = (tr["st"]["kind"] == 0) & (tr["st"]["resource"] % 2 == 0)
    assert c["passes"] >= 100 and c["null"] >= 10 and (tr["ed"][on_a] == 1).sum() >= 100, c
    d = tr["ed"][tr["st"]["kind"] == 0]
    assert all((d == k).sum() >= 20 for k in (0, 1, 2, 3, 4)), np.bincount(d)
    return tr


@pytest.mark.parametrize("path,max_batch,small", PATHS, ids=[p[0] for p in PATHS])
def test_transparent_rule_all_controllers(path, max_batch, small):
    """Default, THREAD, WarmUp, RateLimiter, WarmUp + RateLimiter, prioritized entries (the occupy path),
    breakers and parameter rules through the group replay."""
    from tests.test_local_parity_gpu import _load
    tr = _transparent_trace()
    flow, param, degrade = tr["rules"]
    eng, s = _sentinel(16, max_batch, small)
    assert _load_flow(s, flow) == len(flow)
    _load(s, None, param, degrade)
    for r in range(16):
        assert s.group_of(r) == r - r % 2
    _same(tr["st"], _submit(s, tr["st"]), tr["ed"], tr["ew"], f"transparent {path}")
    _nodes(s, tr, f"transparent {path}")
    eng.close()


# ------------------------------------------------------------------ case 8: reload
def test_reload():
    """RELATE rules, then the same resources under DIRECT-only rules, then RELATE again with count 0: raters
    reset, node statistics kept, groups re-derived, and the entered state survives (0 -> 1 blocks at once in
    the third phase, 2 -> 3 still passes: resource 3 was never entered)."""
    phases = [_pair_rules(1),
              [{"resource": 0, "count": 15}, {"resource": 1, "count": 50}, {"resource": 2, "count": 10}],
              [{"resource": 0, "count": 0, "strategy": RELATE, "ref": 1},
               {"resource": 2, "count": 0, "strategy": RELATE, "ref": 3}]]
    groups = [PAIR_GROUPS, {r: NONE for r in range(4)}, {0: 0, 1: 0, 2: 2, 3: 2}]
    h = rt.RelateTrace(PAIR_RES, phases[0])
    marks = [0]
    for k, rules in enumerate(phases):
        if k:
            h.load(rules)
        h.generate([6000, 3000, 400][k], 91 + k, T0, [0.4, 0.4, 0.2], gap_mean=2.0, acq_max=2, rt_max=39,
                   warm=50 if k == 0 else 0, warm_weights=[0.5, 0.0, 0.5])
        if k == 0:
            c = h.counts()
            assert c["blocks"] >= 100 and c["passes"] >= 100 and c["null"] >= 10, c
        if k == 2:
            h.flush()
        marks.append(h.mark())
    tr = _finish(h, PAIR_RES)
    st, ed = tr["st"], tr["ed"]
    last = slice(marks[2], marks[3])
    e0 = (st["resource"][last] == 0) & (st["kind"][last] == 0)
    e2 = (st["resource"][last] == 2) & (st["kind"][last] == 0)
    assert e0.sum() > 50 and (ed[last][e0] == 1).all() and e2.sum() > 20 and (ed[last][e2] == 0).all()
    for small in (None, 0):
        eng, s = _sentinel(PAIR_RES, 4096, small)
        for k, rules in enumerate(phases):
            assert _load_flow(s, rules) == len(rules)
            for rid, lead in groups[k].items():
                assert s.group_of(rid) == lead, (k, rid)
            a, b = marks[k], marks[k + 1]
            sub = lt.slice_stream(st, a, b)
            _same(sub, _submit(s, sub), ed[a:b], tr["ew"][a:b], f"reload phase {k} small={small}")
        _nodes(s, tr, f"reload small={small}")
        eng.close()


def test_mark_of_an_ungrouped_resource_on_the_pipeline():
    """ClusterNode existence of resources entered only while no rule groups them, in one pipeline chunk: the
    closed form of a single QPS rule (1), the same with 128 events or more (2: k_lwave), a RateLimiter run (3),
    a THREAD rule with more than 1024 events (4: k_lheavy), no rule at all (5), a kind-2 event only (6), and a
    resource entered and revoked in one chunk (7); 8 sees exits only, 9 nothing: neither is entered.  Then
    RELATE rules with count 0 naming each are loaded: 10 + k -> k blocks at once for k = 1..7 and passes for
    8 and 9."""
    n_res = 20
    direct = [{"resource": 1, "count": 5}, {"resource": 2, "count": 50},
              {"resource": 3, "count": 100, "control_behavior": 2, "max_queueing_time_ms": 100},
              {"resource": 4, "count": 4, "grade": 0}]
    h = rt.RelateTrace(n_res, direct)
    rng = np.random.default_rng(101)
    t = T0
    plan = [1] * 20 + [2] * 400 + [3] * 400 + [4] * 1500 + [5] * 30
    rng.shuffle(plan)
    for i, rid in enumerate(plan):
        t += int(rng.integers(0, 2))
        h.step(rid, t, t, 1, int(rng.integers(0, 30)))
        if i == 100:
            h.other(2, 6, t)
            assert h.step(7, t, t, 1, 0, pop=False)[0] == 0
            h.heap = [e for e in h.heap if e[2] != 7]  # revoked below instead of exited
            h.other(3, 7, t)
            h.other(1, 8, t, 0, 0, 5)  # an exit of nothing (acquire 0): no ClusterBuilderSlot.entry
    h.flush()
    m1 = h.mark()
    res = np.array([e[1] for e in h.ev])
    assert (res == 2).sum() >= 128 and (res == 4).sum() > 1024 and (res == 1).sum() < 128
    relate = [{"resource": 10 + k, "count": 0, "strategy": RELATE, "ref": k} for k in range(1, 10)]
    h.load(relate + direct)
    for k in range(1, 10):
        for _ in range(3):
            t += 2
            assert h.step(10 + k, t, t)[0] == (1 if k <= 7 else 0), k
    tr = _finish(h, n_res)
    st = tr["st"]
    eng, s = _sentinel(n_res, 1 << 16, 0)
    assert _load_flow(s, direct) == len(direct)
    assert all(s.group_of(r) == NONE for r in range(n_res))
    sub = lt.slice_stream(st, 0, m1)
    _same(sub, _submit(s, sub), tr["ed"][:m1], tr["ew"][:m1], "ungrouped phase")
    assert _load_flow(s, relate + direct) == len(relate) + len(direct)
    sub = lt.slice_stream(st, m1, len(st["kind"]))
    _same(sub, _submit(s, sub), tr["ed"][m1:], tr["ew"][m1:], "RELATE count 0 after the reload")
    _nodes(s, tr, "ungrouped marks")
    eng.close()
