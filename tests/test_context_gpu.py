"""GPU parity of contexts: events that carry a context create and count one DefaultNode per (resource, context)
pair (NodeSelectorSlot.java:158-177; DefaultNode's overrides count on it and on the ClusterNode), and a CHAIN
FlowRule reads the entry's DefaultNode when its refResource is the entry's context (FlowRuleChecker.java:96-116).

Bar: decisions and waits bit-identical to tests/context_trace.py, and every node getter of every resource, of
every context node and of every origin node identical at three query times.  What the helper refuses is hand
computed.  Each stream is built once and shared by the cases that run it through different paths."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import context_trace as ct
from tests import local_trace as lt

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000
ENOMEM, EINVAL = "rc=-12", "rc=-22"
T = 64  # the statistics pass's short / long threshold (flow.hip kOriginLong)
UNKNOWN = 0xFFFFFFFF


# ------------------------------------------------------------------ engine side
def _sentinel(n_res, n_origins, n_contexts, max_batch=1 << 16, small=None, max_cnodes=0, max_onodes=0):
    from sentinel_amd.cluster import Engine
    from sentinel_amd.local import LocalSentinel
    eng = Engine(max_batch=max_batch)
    if small is not None:
        eng.set_small_batch(small)
    return eng, LocalSentinel(eng, [f"r{i}" for i in range(n_res)], [f"o{i + 1}" for i in range(n_origins)] or None,
                              max_origin_nodes=max_onodes, contexts=[f"c{i + 1}" for i in range(n_contexts)],
                              max_context_nodes=max_cnodes)


def _load(s, flow=None, param=None, degrade=None, system=None):
    from sentinel_amd.local import SystemRule, SystemRuleManager
    from tests.test_local_parity_gpu import _load as load
    load(s, flow, param, degrade)
    if system is not None:
        SystemRuleManager(s).load_rules([SystemRule(**r) for r in system])


def _load_flow(s, rules):
    """FlowRules with "strategy": 2 and "ref" (a context id; None: a name nobody registered) or "limit_app"
    through FlowRuleManager."""
    from sentinel_amd.local import FlowRuleManager
    from sentinel_amd.rules import ClusterFlowConfig, FlowRule
    name = lambda l: "default" if not l else ("other" if l == "other" else f"o{l}")  # noqa: E731
    out = []
    for r in rules:
        chain = r.get("strategy") == 2
        out.append(FlowRule(
            resource=f"r{r['resource']}", count=r["count"], grade=r.get("grade", 1),
            control_behavior=r.get("control_behavior", 0), warm_up_period_sec=r.get("warm_up_period_sec", 10),
            max_queueing_time_ms=r.get("max_queueing_time_ms", 500), limit_app=name(r.get("limit_app")),
            strategy=2 if chain else 0,
            ref_resource=("nobody" if r.get("ref") is None else f"c{r['ref']}") if chain else None,
            cluster_mode=bool(r.get("cluster_mode")),
            cluster_config=ClusterFlowConfig(flow_id=7, fallback_to_local_when_fail=r.get("fallback", True))
            if r.get("cluster_mode") else None))
    return FlowRuleManager(s).load_rules(out)


def _submit(s, st, origins=True, contexts=True):
    return s.submit(st["kind"], st["resource"], st["ts"], st["acquire"], st["flags"], st["rt"], st["param"],
                    origin=st["origin"] if origins and s.origins else None,
                    context=st["context"] if contexts else None)


def _device(s, st, origins=True):
    """One chunk through submit_device with the context (and origin) column; status not read."""
    import torch
    dev = torch.device("cuda", 0)
    base = int(st["ts"].min())
    off = (st["ts"] - base).astype(np.uint32).view(np.int32)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    return s.submit_device(t(st["kind"], np.uint8), t(st["resource"], np.int32), base, t(off, np.int32),
                           t(st["acquire"], np.int32), flags=t(st["flags"], np.uint8), rt=t(st["rt"], np.int64),
                           param=t(st["param"], np.int64),
                           origin=t(st["origin"], np.int32) if origins and s.origins else None,
                           context=t(st["context"], np.int32))


def _same(st, got, ed, ew, what):
    gd, gw = got
    bad = np.nonzero((gd != ed) | (gw != ew))[0]
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(gd)} events differ; first at {i}: kind={st['kind'][i]} "
                             f"res={st['resource'][i]} origin={st['origin'][i]} context={st['context'][i]} "
                             f"ts={st['ts'][i]} gpu=({gd[i]},{gw[i]}) expected=({ed[i]},{ew[i]})")


def _view(v):
    return None if v is None else [getattr(v, g) for g in lt.NODE_GETTERS]


def _nodes(s, tr, n_res, what):
    """Every resource's node, every pair's context node and origin node (None for a pair without one) and the
    created sets."""
    for k, now in enumerate(tr["times"]):
        for rid, exp in tr["nodes"].items():
            got = _view(s.node(rid, now))
            assert got == exp[k], (what, "node", rid, now, list(zip(lt.NODE_GETTERS, got, exp[k])))
        for kind, book, read, n_ids in (("context", tr["cnodes"], s.default_node, len(s.contexts)),
                                        ("origin", tr["onodes"], s.origin_node, len(s.origins))):
            for rid in range(n_res):
                for i in range(1, n_ids + 1):
                    exp = book.get((rid, i))
                    got = _view(read(rid, i, now))
                    if exp is None:
                        assert got is None, (what, kind, "node of a pair never entered", rid, i)
                    else:
                        assert got == exp[k], (what, kind, "node", rid, i, now, list(zip(lt.NODE_GETTERS, got, exp[k])))
    for rid in range(n_res):
        assert s.default_nodes(rid) == [f"c{c}" for (r, c) in sorted(tr["cnodes"]) if r == rid], (what, rid)
        if s.origins:
            assert s.origin_nodes(rid) == [f"o{o}" for (r, o) in sorted(tr["onodes"]) if r == rid], (what, rid)


def _ev(rows):
    """(kind, resource, ts, acquire, flags, rt, param, origin, context) per event."""
    x = np.array(rows, dtype=np.int64).reshape(-1, 9)
    return {"kind": x[:, 0].astype(np.uint8), "resource": x[:, 1].astype(np.uint32), "ts": x[:, 2].copy(),
            "acquire": x[:, 3].astype(np.int32), "flags": x[:, 4].astype(np.uint8), "rt": x[:, 5].copy(),
            "param": x[:, 6].astype(np.uint64), "origin": x[:, 7].astype(np.uint32),
            "context": x[:, 8].astype(np.uint32)}


# ------------------------------------------------------------------ 1: one CHAIN-ruled resource
A, B, C_ = 1, 2, 3
# resource 0, in list order (FlowRuleComparator keeps it: every limitApp is default): CHAIN A (0), CHAIN B (1),
# a name nobody registered (2), the default WarmUp rule (3)
CHAIN = [{"resource": 0, "count": 25, "strategy": 2, "ref": A},
         {"resource": 0, "count": 40, "control_behavior": 2, "max_queueing_time_ms": 20, "strategy": 2, "ref": B},
         {"resource": 0, "count": 0, "strategy": 2, "ref": None},
         {"resource": 0, "count": 60, "control_behavior": 1, "warm_up_period_sec": 2},
         {"resource": 1, "count": 30}]
CHAIN_2 = [dict(r, count=r["count"] + 5) if r.get("ref") == A else r for r in CHAIN]  # the reload


@functools.lru_cache(maxsize=None)
def _chain_trace():
    """Resource 0 under CHAIN rules for contexts A (Default QPS) and B (RateLimiter) and a default WarmUp rule
    after them, resource 1 plain; traffic from A, B, the unruled C and context 0, crossed with two origins and
    none (the replay counts three nodes); 6,000 entries, a rule reload after 3,000 (raters reset, context nodes
    kept).  The seed was picked with the oracles alone so that the floors below hold."""
    h = ct.ContextTrace(2, 2, 3, CHAIN)
    h.generate(3000, 3, T0, [4, 1], [2, 1, 1], [1, 3, 3, 2], gap_mean=4.0, acq_max=2, rt_max=39, regress_pct=0.01,
               err_pct=0.1)
    mark = len(h.ev)
    h.load(CHAIN_2)
    t1 = int(h.ev[-1][2]) + 5
    h.generate(3000, 4, t1, [4, 1], [2, 1, 1], [1, 3, 3, 2], gap_mean=4.0, acq_max=2, rt_max=39, err_pct=0.1)
    tr = h.finish()
    tr["mark"] = mark
    # every rule both passes and blocks (rule 2 never applies: it does neither)
    for k in (0, 1, 3):
        assert tr["rule_block"].get((0, k), 0) >= 20, (k, tr["rule_block"])
    for k in (0, 1, -1):
        assert tr["rule_pass"].get((0, k), 0) >= 50, (k, tr["rule_pass"])
    assert (0, 2) not in tr["rule_block"] and len(tr["cnodes"]) == 6 and len(tr["onodes"]) == 4
    return tr


CHAIN_PATHS = [("chunks_100", 100, 0), ("chunks_3000", 3000, 0), ("small", 700, None)]


@pytest.mark.parametrize("path,chunk,small", CHAIN_PATHS, ids=[p[0] for p in CHAIN_PATHS])
def test_chain_rules(path, chunk, small):
    """Chunks of 100 (the group's segment stays on its k_lflows lane), of 3000 (k_lgroup) and the small path; the
    reload falls between two chunks."""
    tr = _chain_trace()
    st, mark = tr["st"], tr["mark"]
    eng, s = _sentinel(2, 2, 3, 1 << 12, small)
    assert _load_flow(s, CHAIN) == len(CHAIN)
    assert s.group_of(0) == 0 and s.group_of(1) == 0xFFFFFFFF
    gd, gw = [], []
    for lo, hi in [(0, mark), (mark, len(tr["ed"]))]:
        for a in range(lo, hi, chunk):
            d, w = _submit(s, lt.slice_stream(st, a, min(a + chunk, hi)))
            gd.append(d)
            gw.append(w)
        if hi == mark:
            assert _load_flow(s, CHAIN_2) == len(CHAIN_2)
    _same(st, (np.concatenate(gd), np.concatenate(gw)), tr["ed"], tr["ew"], path)
    _nodes(s, tr, 2, path)
    eng.close()


def test_chain_rules_device_entry_and_arrival_order_lane():
    """The same stream up to the reload through sga_submit_events_ctx_device, and (inbound, under a SystemRule
    that never blocks) through k_lseq: decisions only, the nodes are compared on the host paths above."""
    tr = _chain_trace()
    st = lt.slice_stream(tr["st"], 0, tr["mark"])
    ed, ew = tr["ed"][:tr["mark"]], tr["ew"][:tr["mark"]]
    eng, s = _sentinel(2, 2, 3, 1 << 13, 0)
    _load_flow(s, CHAIN)
    d, w = _device(s, st)
    s.device_status()
    _same(st, (d.cpu().numpy(), w.cpu().numpy()), ed, ew, "device")
    eng.close()
    eng, s = _sentinel(2, 2, 3, 1 << 13, 0)
    _load(s, system=[{"qps": 1e9}])
    _load_flow(s, CHAIN)
    _same(st, _submit(s, dict(st, flags=st["flags"] | 8)), ed, ew, "seq")
    eng.close()


# ------------------------------------------------------------------ 2: statistics pass only
MIX_RES, MIX_ORG, MIX_CTX = 8, 3, 4
MIX_FLOW = [{"resource": 0, "count": 60}, {"resource": 1, "count": 80, "control_behavior": 1, "warm_up_period_sec": 3},
            {"resource": 2, "count": 120, "control_behavior": 2, "max_queueing_time_ms": 30},
            {"resource": 3, "count": 90, "control_behavior": 3, "warm_up_period_sec": 2, "max_queueing_time_ms": 20},
            {"resource": 4, "count": 6, "grade": 0}, {"resource": 7, "count": 40}]
MIX_PARAM = [{"resource": 5, "count": 8, "burst_count": 2}]
MIX_DEGRADE = [{"resource": 6, "grade": 2, "count": 4, "time_window": 1, "min_request_amount": 3},
               {"resource": 7, "grade": 0, "count": 30, "time_window": 1, "slow_ratio_threshold": 0.5}]
MIX_SYSTEM = [{"qps": 1e9}]


@functools.lru_cache(maxsize=None)
def _mix_trace(inbound):
    """8 resources under the four controllers, a parameter rule and two breakers, no CHAIN rule; 4 contexts and
    none crossed with 3 origins and none; 15,000 entries and their exits: about 20,000 events."""
    h = ct.ContextTrace(MIX_RES, MIX_ORG, MIX_CTX, MIX_FLOW, MIX_PARAM, MIX_DEGRADE,
                        system=MIX_SYSTEM if inbound else None)
    h.generate(15000, 5 + inbound, T0, [3, 2, 2, 2, 1, 2, 2, 2], [2, 3, 2, 1], [1, 3, 2, 1, 1], gap_mean=1.0, acq_max=2,
               rt_max=39, regress_pct=0.02, inbound=inbound, err_pct=0.1, params=6, param_res=(5,))
    tr = h.finish(entry=inbound)
    d = tr["ed"][tr["st"]["kind"] == 0]
    assert len(tr["ed"]) >= 19000 and len(tr["cnodes"]) == MIX_RES * MIX_CTX and len(tr["onodes"]) == MIX_RES * MIX_ORG
    assert all((d == c).sum() >= 100 for c in (0, 1, 2, 3)), np.bincount(d)
    both = (tr["st"]["origin"] != 0) & (tr["st"]["context"] != 0)
    assert both.sum() > 5000 and (~both).sum() > 3000
    return tr


MIX_PATHS = [("pipeline", 1 << 16, 0, False), ("pipeline_chunks", 3000, 0, False), ("small", 1000, None, False),
             ("seq", 1 << 16, 0, True)]


@pytest.mark.parametrize("path,max_batch,small,inbound", MIX_PATHS, ids=[p[0] for p in MIX_PATHS])
def test_statistics_only(path, max_batch, small, inbound):
    """Both arrays: two sort elements per event on the pipeline paths (one chunk; chunks of 3000), the small
    path and the arrival-order lane."""
    tr = _mix_trace(inbound)
    eng, s = _sentinel(MIX_RES, MIX_ORG, MIX_CTX, max_batch, small)
    _load(s, MIX_FLOW, MIX_PARAM, MIX_DEGRADE, MIX_SYSTEM if inbound else None)
    _same(tr["st"], _submit(s, tr["st"]), tr["ed"], tr["ew"], path)
    _nodes(s, tr, MIX_RES, path)
    eng.close()


def test_statistics_only_device_entry():
    tr = _mix_trace(False)
    eng, s = _sentinel(MIX_RES, MIX_ORG, MIX_CTX, 1 << 15)
    _load(s, MIX_FLOW, MIX_PARAM, MIX_DEGRADE)
    d, w = _device(s, tr["st"])
    s.device_status()
    _same(tr["st"], (d.cpu().numpy(), w.cpu().numpy()), tr["ed"], tr["ew"], "device")
    _nodes(s, tr, MIX_RES, "device")
    eng.close()


@pytest.mark.parametrize("arrays", ["context_only", "origin_only", "neither"])
def test_decisions_do_not_depend_on_the_arrays(arrays):
    """The same stream with the context array alone (an engine without origins), without the context array, and
    without either: same decisions, same ClusterNodes, only the nodes of the arrays passed."""
    tr = _mix_trace(False)
    eng, s = _sentinel(MIX_RES, 0 if arrays == "context_only" else MIX_ORG, MIX_CTX)
    _load(s, MIX_FLOW, MIX_PARAM, MIX_DEGRADE)
    got = _submit(s, tr["st"], origins=arrays == "origin_only", contexts=arrays == "context_only")
    _same(tr["st"], got, tr["ed"], tr["ew"], arrays)
    _nodes(s, dict(tr, cnodes=tr["cnodes"] if arrays == "context_only" else {},
                   onodes=tr["onodes"] if arrays == "origin_only" else {}), MIX_RES, arrays)
    eng.close()


# ------------------------------------------------------------------ 3: segment shapes of the statistics pass
SHAPES = [T - 1, T, T + 1, 1023, 1024, 1025, 2049]
SHAPE_ONES = 300
SHAPE_RULES = [{"resource": r, "count": 150} for r in range(9)]


@functools.lru_cache(maxsize=None)
def _shape_trace():
    """One chunk.  Pair (k, context 1) gets SHAPES[k] events within 3 s.  Pair (7, 1): 400 events, one stamped
    700 ms back (a tile whose times decrease).  Pair (8, 1): 300 events 150 ms apart (a tile that spans 45 s).
    Beside them 300 pairs of one event each.  The events of resources 1, 4 and 6 and every other one-event pair
    carry an origin as well: two sort elements each."""
    n_res = 9 + SHAPE_ONES
    rng = np.random.default_rng(11)
    plan = []  # (arrival time, timestamp, resource, origin, context)
    for k, n in enumerate(SHAPES):
        plan += [(T0 + int(x), T0 + int(x), k, 1 if k in (1, 4, 6) else 0, 1)
                 for x in np.sort(rng.integers(0, 3000, size=n))]
    back = [T0 + int(x) for x in np.sort(rng.integers(800, 3000, size=400))]
    plan += [(t, t - 700 if j == 200 else t, 7, 0, 1) for j, t in enumerate(back)]
    plan += [(T0 + 150 * j, T0 + 150 * j, 8, 0, 1) for j in range(300)]
    for j in range(SHAPE_ONES):
        t = T0 + int(rng.integers(0, 3000))
        plan.append((t, t, 9 + j, 2 * (j % 2), 2))
    order = sorted(range(len(plan)), key=lambda i: (plan[i][0], i))
    h = ct.ContextTrace(n_res, 2, 2, SHAPE_RULES)
    open_ = {}
    for i in order:
        _, t, rid, o, c = plan[i]
        q = open_.setdefault(rid, [])
        if q and len(h.ev) % 3 == 2:  # every third event of a pair exits its oldest open entry
            te, acq = q.pop(0)
            h.other(1, rid, o, t, acq, 2 if len(h.ev) % 5 == 0 else 0, max(0, t - te), c=c)
        else:
            acq = 1 + i % 2
            if h.entry(rid, o, t, acq, c=c)[0] == 0:
                q.append((t, acq))
    tr = h.finish()
    st = tr["st"]
    sizes = {k: int(((st["resource"] == k) & (st["context"] == 1)).sum()) for k in range(9)}
    assert [sizes[k] for k in range(7)] == SHAPES and sizes[7] == 400 and sizes[8] == 300, sizes
    assert (np.diff(st["ts"][st["resource"] == 7]) < 0).sum() == 1
    assert len(st["kind"]) < 1 << 13 and len(tr["cnodes"]) == 9 + SHAPE_ONES
    assert len(tr["onodes"]) == 3 + SHAPE_ONES // 2
    for k in (4, 6):  # the long segments hold all three kinds of adds
        sel = st["resource"] == k
        assert (st["kind"][sel] == 1).sum() > 100 and (tr["ed"][sel] == 1).sum() > 100
    return tr


def test_segment_shapes():
    tr = _shape_trace()
    n_res = 9 + SHAPE_ONES
    eng, s = _sentinel(n_res, 2, 2, 1 << 13, 0)
    _load(s, SHAPE_RULES)
    _same(tr["st"], _submit(s, tr["st"]), tr["ed"], tr["ew"], "shapes")
    _nodes(s, tr, n_res, "shapes")
    eng.close()


# ------------------------------------------------------------------ 4: hand-computed cases (the helper refuses them)
def test_chain_rule_after_an_applicable_default_rule():
    """Resource 0: a DIRECT default rule QPS 2, then CHAIN c1 QPS 1 -- checked in that order."""
    for small in (None, 0):
        eng, s = _sentinel(1, 0, 2, 1 << 12, small)
        assert _load_flow(s, [{"resource": 0, "count": 2}, {"resource": 0, "count": 1, "strategy": 2, "ref": 1}]) == 2
        st = _ev([(0, 0, T0 + 1, 1, 0, 0, 0, 0, 1),    # c1: rule 0 0+1<=2, rule 1 0+1<=1: passes
                  (0, 0, T0 + 2, 1, 0, 0, 0, 0, 1),    # c1: rule 0 1+1<=2, rule 1 reads c1's node 1+1>1: blocked by 1
                  (0, 0, T0 + 3, 1, 0, 0, 0, 0, 2),    # c2: rule 0 1+1<=2, rule 1 does not apply: passes
                  (0, 0, T0 + 4, 1, 0, 0, 0, 0, 0),    # no context: rule 0 2+1>2: blocked by 0
                  (0, 0, T0 + 5, 1, 0, 0, 0, 0, 1)])   # c1: blocked by rule 0 before rule 1 is asked
        d, w = _submit(s, st)
        assert list(d) == [0, 1, 0, 1, 1] and list(w[[1, 3, 4]]) == [1, 0, 0], (small, d, w)
        now = T0 + 6
        a, b, n = s.default_node(0, 1, now), s.default_node(0, 2, now), s.node(0, now)
        assert (a.total_pass, a.total_block, a.cur_thread_num) == (1, 2, 1)
        assert (b.total_pass, b.total_block, b.cur_thread_num) == (1, 0, 1)
        assert (n.total_pass, n.total_block, n.cur_thread_num) == (2, 3, 2)
        assert s.default_nodes(0) == ["c1", "c2"]
        eng.close()


def test_prioritized_entry_under_a_chain_rule_occupies_on_the_default_node():
    """With every entry in context c1 the DefaultNode receives what the ClusterNode receives, so a CHAIN c1 rule
    must decide as the same rule with strategy DIRECT does, and c1's DefaultNode must read as that engine's
    ClusterNode -- occupy and waiting counters included.  The oracle decides the DIRECT stream: QPS 1, the
    second entry prioritized: it occupies the next bucket and waits 400 ms (SGA_PASS_WAIT).  The CHAIN engine's
    own ClusterNode gets no occupy counters (DefaultNode forwards none): a thread and no pass."""
    rows = [(0, 0, T0 + 100, 1, 0, 0, 0, 0, 1), (0, 0, T0 + 600, 1, 1, 0, 0, 0, 1), (0, 0, T0 + 700, 1, 1, 0, 0, 0, 1)]
    st = _ev(rows)
    orc = lt.Oracle(1, [{"resource": 0, "count": 1}])
    od, ow = orc.replay({k: v for k, v in st.items() if k not in ("origin", "context")})
    times = [T0 + 701, T0 + 1100, T0 + 2500]
    exp = [orc.node(0, t) for t in times]
    orc.close()
    assert list(od[:2]) == [0, 4] and list(ow[:2]) == [0, 400]
    eng, s = _sentinel(1, 0, 1, 1 << 12)
    assert _load_flow(s, [{"resource": 0, "count": 1, "strategy": 2, "ref": 1}]) == 1
    _same(st, _submit(s, st), od, ow, "chain, prioritized")
    for k, t in enumerate(times):
        assert _view(s.default_node(0, 1, t)) == exp[k], (t, list(zip(lt.NODE_GETTERS, _view(s.default_node(0, 1, t)), exp[k])))
    n = s.node(0, T0 + 701)
    assert (n.cur_thread_num, n.total_pass) == (int(((od == 0) | (od == 4)).sum()), int((od == 0).sum()))
    eng.close()


def test_pass_wait_counts_a_thread_only_on_the_context_node():
    """PriorityWaitException (StatisticSlot.java:101-104), no CHAIN rule: DIRECT QPS 1; the first entry (c2)
    passes, the prioritized second (c1) waits 400 ms: c1's node gets the thread and no pass."""
    st = _ev([(0, 0, T0 + 100, 1, 0, 0, 0, 0, 2), (0, 0, T0 + 600, 1, 1, 0, 0, 0, 1)])
    eng, s = _sentinel(1, 0, 2, 1 << 12)
    _load(s, [{"resource": 0, "count": 1}])
    d, w = _submit(s, st)
    assert list(d) == [0, 4] and list(w) == [0, 400]
    now = T0 + 601
    a, b = s.default_node(0, 1, now), s.default_node(0, 2, now)
    assert (a.cur_thread_num, a.total_pass, a.total_block, a.pass_qps) == (1, 0, 0, 0.0)
    assert (b.cur_thread_num, b.total_pass, b.total_block, b.pass_qps) == (1, 1, 0, 1.0)
    assert s.node(0, now).cur_thread_num == 2
    eng.close()


def test_chain_rule_in_cluster_mode_falls_back_to_its_context_node():
    """No token service: a cluster-mode CHAIN rule falls back to its local check (count 0 blocks the entries of
    its context and nobody else's); with fallbackToLocalWhenFail off it passes everybody."""
    st = _ev([(0, 0, T0 + 1, 1, 0, 0, 0, 0, 1), (0, 0, T0 + 2, 1, 0, 0, 0, 0, 2), (0, 0, T0 + 3, 1, 0, 0, 0, 0, 0)])
    for fallback, want in ((True, [1, 0, 0]), (False, [0, 0, 0])):
        eng, s = _sentinel(1, 0, 2, 1 << 12)
        assert _load_flow(s, [{"resource": 0, "count": 0, "strategy": 2, "ref": 1, "cluster_mode": True,
                               "fallback": fallback}]) == 1
        d, w = _submit(s, st)
        assert list(d) == want and w[0] == 0, (fallback, d, w)
        assert s.default_node(0, 1, T0 + 4).total_block == (1 if fallback else 0)
        eng.close()


def test_chain_rule_with_a_limit_app():
    """CHAIN c1 limited to origin o1, QPS 1: it applies to entries from o1 in c1 alone, and reads c1's
    DefaultNode -- which o2's entries in c1 count on too -- not o1's origin node."""
    eng, s = _sentinel(1, 2, 2, 1 << 12)
    assert _load_flow(s, [{"resource": 0, "count": 1, "strategy": 2, "ref": 1, "limit_app": 1}]) == 1
    st = _ev([(0, 0, T0 + 1, 1, 0, 0, 0, 2, 1),    # o2 in c1: the limitApp test fails, passes; c1's node: 1
              (0, 0, T0 + 2, 1, 0, 0, 0, 1, 1),    # o1 in c1: 1 + 1 > 1 on c1's node: blocked (o1's node is empty)
              (0, 0, T0 + 3, 1, 0, 0, 0, 1, 2),    # o1 in c2: another context, passes
              (0, 0, T0 + 4, 1, 0, 0, 0, 1, 0),    # o1, no context: passes
              (0, 0, T0 + 5, 1, 0, 0, 0, 0, 1)])   # no origin in c1: passes
    d, w = _submit(s, st)
    assert list(d) == [0, 1, 0, 0, 0] and w[1] == 0, (d, w)
    now = T0 + 6
    c1, o1 = s.default_node(0, 1, now), s.origin_node(0, 1, now)
    assert (c1.total_pass, c1.total_block, c1.cur_thread_num) == (2, 1, 2)
    assert (o1.total_pass, o1.total_block, o1.cur_thread_num) == (2, 1, 2)
    assert s.node(0, now).total_pass == 4 and s.node(0, now).total_block == 1
    eng.close()


@pytest.mark.parametrize("small", [None, 0], ids=["small", "pipeline"])
@pytest.mark.parametrize("chain", [False, True], ids=["statistics_pass", "chain_ruled"])
def test_blocked_revoked_orphan_and_early_exit_events(small, chain):
    """Kind 2 and kind 3 events with a context create and count; an exit of a pair never entered does not, nor
    one that arrives ahead of the pair's first entry in the same chunk."""
    rules = ([{"resource": 0, "count": 50, "strategy": 2, "ref": 3}] if chain else []) + [{"resource": 0, "count": 2}]
    h = ct.ContextTrace(3, 1, 3, rules)
    t = T0
    h.other(1, 0, 0, t, 1, 0, 7, c=1)           # an exit of (0, c1) ahead of its first entry: counts nothing
    h.other(2, 1, 0, t, 3, c=2)                 # a block outside the engine creates (1, c2)
    for k in range(4):                          # two passes, two blocks in c1 (the last two from o1)
        h.entry(0, k // 2, t + 1 + k, 1, c=1)
    h.other(3, 0, 0, t + 1, 1, c=1)             # the first pass revoked
    h.other(1, 0, 0, t + 40, 1, 2, 38, c=1)     # the second exits with an error
    h.other(1, 2, 0, t + 41, 1, 0, 5, c=3)      # an exit of (2, c3): no node before, none after
    h.other(1, 0, 0, t + 42, 1, 0, 5, c=3)      # an exit of (0, c3), whose resource has other context nodes
    h.other(3, 2, 1, t + 43, 2, c=1)            # a revoke creates (2, c1) and (2, o1)
    assert h.ccreated == {(1, 2), (0, 1), (2, 1)} and h.created == {(0, 1), (2, 1)}
    tr = h.finish()
    assert list(tr["ed"][2:6]) == [0, 0, 1, 1]
    eng, s = _sentinel(3, 1, 3, 1 << 12, small)
    assert _load_flow(s, rules) == len(rules)
    _same(tr["st"], _submit(s, tr["st"]), tr["ed"], tr["ew"], "edges")
    _nodes(s, tr, 3, "edges")
    eng.close()


# ------------------------------------------------------------------ 5: refusals
def _state(s, n_res, now):
    return ([_view(s.node(r, now)) for r in range(n_res)],
            {(r, c): _view(s.default_node(r, c, now)) for r in range(n_res) for c in range(1, len(s.contexts) + 1)},
            {(r, o): _view(s.origin_node(r, o, now)) for r in range(n_res) for o in range(1, len(s.origins) + 1)},
            [s.default_nodes(r) for r in range(n_res)], [s.origin_nodes(r) for r in range(n_res)])


def _refused(s, entry, st, rc):
    from sentinel_amd._lib import EngineError
    if entry == "device":
        d, _ = _device(s, st)
        with pytest.raises(EngineError, match=rc):
            s.device_status()
        assert (d.cpu().numpy() == -1).all()
    else:
        with pytest.raises(EngineError, match=rc):
            _submit(s, st)


@pytest.mark.parametrize("entry", ["host", "small", "device"])
def test_context_id_past_the_registered_ones_refuses_the_chunk(entry):
    """... and the origin pairs the chunk claimed are unborn again."""
    eng, s = _sentinel(2, 2, 3, 1 << 12, None if entry == "small" else 0)
    _submit(s, _ev([(0, 0, T0, 1, 0, 0, 0, 1, 1), (0, 1, T0 + 1, 1, 0, 0, 0, 0, 3)]))
    before = _state(s, 2, T0 + 10)
    # a new origin pair (1, o2) and a new context pair (0, c2) beside the bad id
    bad = _ev([(0, 1, T0 + 2, 1, 0, 0, 0, 2, 2), (0, 0, T0 + 3, 1, 0, 0, 0, 1, 2), (0, 1, T0 + 4, 1, 0, 0, 0, 0, 4)])
    _refused(s, entry, bad, EINVAL)
    assert _state(s, 2, T0 + 10) == before
    assert before[3] == [["c1"], ["c3"]] and before[4] == [["o1"], []]
    # the pairs are born by a later chunk that is applied
    assert list(_submit(s, lt.slice_stream(bad, 0, 2))[0]) == [0, 0]
    assert s.origin_nodes(1) == ["o2"] and s.default_nodes(0) == ["c1", "c2"] and s.default_nodes(1) == ["c2", "c3"]
    assert s.origin_node(1, 2, T0 + 10).total_pass == 1 and s.default_node(0, 2, T0 + 10).total_pass == 1
    eng.close()


@pytest.mark.parametrize("entry", ["host", "small", "device"])
def test_full_context_table_refuses_the_chunk(entry):
    """max_context_nodes = 4 and a fifth pair: SGA_ENOMEM, nothing of the chunk applied anywhere, the origin pair
    it claimed unborn again (the origin table has room)."""
    eng, s = _sentinel(3, 3, 3, 1 << 12, None if entry == "small" else 0, max_cnodes=4)
    _load(s, [{"resource": 0, "count": 5}])
    four = _ev([(0, 0, T0, 1, 0, 0, 0, 1, 1), (0, 0, T0 + 1, 1, 0, 0, 0, 0, 2), (0, 1, T0 + 2, 1, 0, 0, 0, 0, 1),
                (0, 2, T0 + 3, 1, 0, 0, 0, 0, 3)])
    assert list(_submit(s, four)[0]) == [0, 0, 0, 0]
    now = T0 + 20
    before = _state(s, 3, now)
    assert sum(v is not None for v in before[1].values()) == 4 and before[4] == [["o1"], [], []]
    fifth = _ev([(0, 0, T0 + 5, 1, 0, 0, 0, 2, 1), (0, 1, T0 + 6, 1, 0, 0, 0, 3, 2), (1, 0, T0 + 7, 1, 0, 3, 0, 0, 1)])
    _refused(s, entry, fifth, ENOMEM)
    assert _state(s, 3, now) == before
    # the table still serves the pairs it holds
    again = _ev([(1, 0, T0 + 8, 1, 0, 8, 0, 0, 1), (0, 2, T0 + 9, 2, 0, 0, 0, 2, 3)])
    assert list(_submit(s, again)[0]) == [0, 0]
    v = s.default_node(0, 1, now)
    assert (v.cur_thread_num, v.total_success, v.total_pass) == (0, 1, 1)
    assert s.default_node(2, 3, now).total_pass == 3 and s.origin_nodes(2) == ["o2"]
    eng.close()


def _raw_rules(rows):
    from sentinel_amd._lib import SgaFlowRule
    arr = (SgaFlowRule * len(rows))()
    for a, (res, count, strategy, ref) in zip(arr, rows):
        a.resource, a.grade, a.count, a.strategy, a.ref_resource = res, 1, count, strategy, ref
    return arr


def test_chain_rule_validity_through_the_three_loaders():
    """sga_load_flow_rules_ctx: a registered context and SGA_CONTEXT_UNKNOWN are valid (the latter counted, in
    its place, never applying), id 0 and an id past n_contexts are invalid rules; limit_app NULL is legal on an
    engine without origins.  The two older loaders keep rejecting strategy 2."""
    from sentinel_amd import _lib
    L = _lib.load()
    eng, s = _sentinel(1, 0, 2, 1 << 12)
    rows = [(0, 0, 2, UNKNOWN), (0, 0, 2, 0), (0, 0, 2, 3), (0, 1, 2, 2), (0, 5, 0, 0)]
    assert L.sga_load_flow_rules_ctx(eng.handle, _raw_rules(rows), None, len(rows)) == 3
    assert s.group_of(0) == 0
    st = _ev([(0, 0, T0 + 1, 1, 0, 0, 0, 0, 2), (0, 0, T0 + 2, 1, 0, 0, 0, 0, 2), (0, 0, T0 + 3, 1, 0, 0, 0, 0, 1)])
    d, w = _submit(s, st)
    # valid rules in place: unknown (0, count 0, never applies), CHAIN c2 (1), default (2)
    assert list(d) == [0, 1, 0] and w[1] == 1, (d, w)
    assert L.sga_load_flow_rules(eng.handle, _raw_rules(rows), len(rows)) == 1
    assert s.group_of(0) == 0xFFFFFFFF
    eng.close()
    eng, s = _sentinel(1, 1, 2, 1 << 12)
    lim = (C.c_uint32 * len(rows))()
    assert L.sga_load_flow_rules_origin(eng.handle, _raw_rules(rows), lim, len(rows)) == 1
    assert L.sga_load_flow_rules_ctx(eng.handle, _raw_rules(rows), lim, len(rows)) == 3
    eng.close()

