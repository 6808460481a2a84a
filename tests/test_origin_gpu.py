"""GPU parity of origin nodes: events that carry a caller origin create and count one StatisticNode per
(resource, origin) pair beside the resource's ClusterNode (ClusterBuilderSlot.java:104-107,
StatisticSlot.java:81-84, 101-104, 123-125, 160-161).

Bar: decisions and waits bit-identical to tests/origin_trace.py, and every node getter of every resource and
of every origin node identical at three query times.  Each stream is built once and shared by the cases that
run it through different paths."""
import functools

import numpy as np
import pytest

from tests import local_trace as lt
from tests import origin_trace as ot

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000
ENOMEM, EINVAL = "rc=-12", "rc=-22"
T = 64  # the statistics pass's short / long threshold (flow.hip kOriginLong)


# ------------------------------------------------------------------ engine side
def _sentinel(n_res, n_origins, max_batch=1 << 16, small=None, max_nodes=0):
    from sentinel_amd.cluster import Engine
    from sentinel_amd.local import LocalSentinel
    eng = Engine(max_batch=max_batch)
    if small is not None:
        eng.set_small_batch(small)
    return eng, LocalSentinel(eng, [f"r{i}" for i in range(n_res)], [f"o{i + 1}" for i in range(n_origins)],
                              max_origin_nodes=max_nodes)


def _load(s, flow=None, param=None, degrade=None, system=None):
    from sentinel_amd.local import SystemRule, SystemRuleManager
    from tests.test_local_parity_gpu import _load as load
    load(s, flow, param, degrade)
    if system is not None:
        SystemRuleManager(s).load_rules([SystemRule(**r) for r in system])


def _load_flow(s, rules):
    """FlowRules with a "limit_app" (an origin id or "other") and "ref" (RELATE) through FlowRuleManager."""
    from sentinel_amd.local import FlowRuleManager
    from sentinel_amd.rules import FlowRule
    name = lambda l: "default" if not l else ("other" if l == "other" else f"o{l}")  # noqa: E731
    return FlowRuleManager(s).load_rules([
        FlowRule(resource=f"r{r['resource']}", count=r["count"], grade=r.get("grade", 1),
                 control_behavior=r.get("control_behavior", 0), warm_up_period_sec=r.get("warm_up_period_sec", 10),
                 max_queueing_time_ms=r.get("max_queueing_time_ms", 500), limit_app=name(r.get("limit_app")),
                 strategy=1 if "ref" in r else 0, ref_resource=f"r{r['ref']}" if "ref" in r else None)
        for r in rules])


def _submit(s, st, origins=True):
    return s.submit(st["kind"], st["resource"], st["ts"], st["acquire"], st["flags"], st["rt"], st["param"],
                    origin=st["origin"] if origins else None)


def _device(s, st):
    """One chunk through submit_device with the origin column; host numpy (decision, wait), status not read."""
    import torch
    dev = torch.device("cuda", 0)
    base = int(st["ts"].min())
    off = (st["ts"] - base).astype(np.uint32).view(np.int32)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    d, w = s.submit_device(t(st["kind"], np.uint8), t(st["resource"], np.int32), base, t(off, np.int32),
                           t(st["acquire"], np.int32), flags=t(st["flags"], np.uint8), rt=t(st["rt"], np.int64),
                           param=t(st["param"], np.int64), origin=t(st["origin"], np.int32))
    return d, w


def _same(st, got, ed, ew, what):
    gd, gw = got
    bad = np.nonzero((gd != ed) | (gw != ew))[0]
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(gd)} events differ; first at {i}: kind={st['kind'][i]} "
                             f"res={st['resource'][i]} origin={st['origin'][i]} ts={st['ts'][i]} "
                             f"gpu=({gd[i]},{gw[i]}) expected=({ed[i]},{ew[i]})")


def _view(v):
    return None if v is None else [getattr(v, g) for g in lt.NODE_GETTERS]


def _nodes(s, tr, n_res, n_origins, what):
    """Every resource's node, every pair's origin node (None for a pair without one) and the created sets."""
    for k, now in enumerate(tr["times"]):
        for rid, exp in tr["nodes"].items():
            got = _view(s.node(rid, now))
            assert got == exp[k], (what, "node", rid, now, list(zip(lt.NODE_GETTERS, got, exp[k])))
        for rid in range(n_res):
            for o in range(1, n_origins + 1):
                exp = tr["onodes"].get((rid, o))
                got = _view(s.origin_node(rid, o, now))
                if exp is None:
                    assert got is None, (what, "origin node of a pair never entered", rid, o)
                else:
                    assert got == exp[k], (what, "origin node", rid, o, now, list(zip(lt.NODE_GETTERS, got, exp[k])))
    for rid in range(n_res):
        assert s.origin_nodes(rid) == [f"o{o}" for (r, o) in sorted(tr["onodes"]) if r == rid], (what, rid)


# ------------------------------------------------------------------ 1: statistics only
MIX_RES, MIX_ORG = 8, 5
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
    """8 resources under the four controllers (QPS and THREAD grade), a parameter rule and two breakers; 5
    origins and origin 0; 15,000 entries (mean gap 1 ms, acquire 1-2, rt 0-39, 2 % clock regressions, 10 %
    errors) and their exits: about 20,000 events.  inbound: every event EntryType.IN under a SystemRule that
    never blocks (the arrival-order lane, ENTRY_NODE)."""
    h = ot.OriginTrace(MIX_RES, MIX_ORG, MIX_FLOW, MIX_PARAM, MIX_DEGRADE, system=MIX_SYSTEM if inbound else None)
    h.generate(15000, 5 + inbound, T0, [3, 2, 2, 2, 1, 2, 2, 2], [2, 3, 2, 1, 1, 0.5], gap_mean=1.0, acq_max=2,
               rt_max=39, regress_pct=0.02, inbound=inbound, err_pct=0.1, params=6, param_res=(5,))
    tr = h.finish(entry=inbound)
    d = tr["ed"][tr["st"]["kind"] == 0]
    assert len(tr["ed"]) >= 19000 and len(tr["onodes"]) == MIX_RES * MIX_ORG
    assert all((d == c).sum() >= 100 for c in (0, 1, 2, 3)), np.bincount(d)  # passes and every kind of block
    return tr


MIX_PATHS = [("pipeline", 1 << 16, 0, False), ("pipeline_chunks", 3000, 0, False), ("small", 1000, None, False),
             ("seq", 1 << 16, 0, True)]


@pytest.mark.parametrize("path,max_batch,small,inbound", MIX_PATHS, ids=[p[0] for p in MIX_PATHS])
def test_statistics_only(path, max_batch, small, inbound):
    """The host pipeline (one chunk, and chunks of 3000: nodes carry across chunks), the small path (chunks of
    1000 through k_lsmall) and the arrival-order lane (a SystemRule loaded, inbound events)."""
    tr = _mix_trace(inbound)
    eng, s = _sentinel(MIX_RES, MIX_ORG, max_batch, small)
    _load(s, MIX_FLOW, MIX_PARAM, MIX_DEGRADE, MIX_SYSTEM if inbound else None)
    _same(tr["st"], _submit(s, tr["st"]), tr["ed"], tr["ew"], path)
    _nodes(s, tr, MIX_RES, MIX_ORG, path)
    eng.close()


def test_statistics_only_device_entry():
    """sga_submit_events_origin_device, one chunk."""
    tr = _mix_trace(False)
    eng, s = _sentinel(MIX_RES, MIX_ORG, 1 << 15)
    _load(s, MIX_FLOW, MIX_PARAM, MIX_DEGRADE)
    d, w = _device(s, tr["st"])
    s.device_status()
    _same(tr["st"], (d.cpu().numpy(), w.cpu().numpy()), tr["ed"], tr["ew"], "device")
    _nodes(s, tr, MIX_RES, MIX_ORG, "device")
    eng.close()


def test_decisions_do_not_depend_on_origins():
    """The same stream without its origin column: same decisions, same ClusterNodes, no origin node."""
    tr = _mix_trace(False)
    eng, s = _sentinel(MIX_RES, MIX_ORG)
    _load(s, MIX_FLOW, MIX_PARAM, MIX_DEGRADE)
    _same(tr["st"], _submit(s, tr["st"], origins=False), tr["ed"], tr["ew"], "no origins")
    _nodes(s, dict(tr, onodes={}), MIX_RES, MIX_ORG, "no origins")
    eng.close()


# ------------------------------------------------------------------ 2: segment shapes of the statistics pass
SHAPES = [T - 1, T, T + 1, 1023, 1024, 1025, 2049]
SHAPE_ONES = 300
SHAPE_RULES = [{"resource": r, "count": 150} for r in range(9)]


@functools.lru_cache(maxsize=None)
def _shape_trace():
    """One chunk.  Pair (k, origin 1) gets SHAPES[k] events within 3 s: below, at and past the short / long
    threshold, and one tile less one, one tile, one tile and one, two tiles and one.  Pair (7, 1): 400 events,
    one stamped 700 ms back (a tile whose times decrease).  Pair (8, 1): 300 events 150 ms apart (a tile that
    spans 45 s: more than 64 buckets).  Beside them 300 pairs of one event each.  Resources 0-8 allow 150 QPS,
    so the long segments hold passes, blocks and exits."""
    n_res = 9 + SHAPE_ONES
    rng = np.random.default_rng(11)
    plan = []  # (arrival time, timestamp, resource, origin)
    for k, n in enumerate(SHAPES):
        plan += [(T0 + int(x), T0 + int(x), k, 1) for x in np.sort(rng.integers(0, 3000, size=n))]
    back = [T0 + int(x) for x in np.sort(rng.integers(800, 3000, size=400))]
    plan += [(t, t - 700 if j == 200 else t, 7, 1) for j, t in enumerate(back)]
    plan += [(T0 + 150 * j, T0 + 150 * j, 8, 1) for j in range(300)]
    for j in range(SHAPE_ONES):
        t = T0 + int(rng.integers(0, 3000))
        plan.append((t, t, 9 + j, 2))
    order = sorted(range(len(plan)), key=lambda i: (plan[i][0], i))
    h = ot.OriginTrace(n_res, 2, SHAPE_RULES)
    open_ = {}
    for i in order:
        _, t, rid, o = plan[i]
        # every third event of a pair exits its oldest open entry, the others enter
        q = open_.setdefault(rid, [])
        if q and len(h.ev) % 3 == 2:
            te, acq = q.pop(0)
            h.other(1, rid, o, t, acq, 2 if len(h.ev) % 5 == 0 else 0, max(0, t - te))
        else:
            acq = 1 + i % 2
            if h.entry(rid, o, t, acq)[0] == 0:
                q.append((t, acq))
    tr = h.finish()
    st = tr["st"]
    sizes = {k: int(((st["resource"] == k) & (st["origin"] == 1)).sum()) for k in range(9)}
    assert [sizes[k] for k in range(7)] == SHAPES and sizes[7] == 400 and sizes[8] == 300, sizes
    assert (np.diff(st["ts"][st["resource"] == 7]) < 0).sum() == 1
    assert len(st["kind"]) < 1 << 13 and len(tr["onodes"]) == 9 + SHAPE_ONES
    for k in (4, 6):  # the long segments hold all three kinds of adds
        sel = st["resource"] == k
        assert (st["kind"][sel] == 1).sum() > 100 and (tr["ed"][sel] == 1).sum() > 100
    return tr


def test_segment_shapes():
    tr = _shape_trace()
    n_res = 9 + SHAPE_ONES
    eng, s = _sentinel(n_res, 2, 1 << 13, 0)
    _load(s, SHAPE_RULES)
    _same(tr["st"], _submit(s, tr["st"]), tr["ed"], tr["ew"], "shapes")
    _nodes(s, tr, n_res, 2, "shapes")
    eng.close()


# ------------------------------------------------------------------ 3: origin rules
A, B, C, D = 1, 2, 3, 4
# resource 0, in list order; FlowRuleComparator order: A (0), B (1), other (2), default (3)
RULED = [{"resource": 0, "count": 60, "control_behavior": 1, "warm_up_period_sec": 2},
         {"resource": 0, "count": 25, "limit_app": A},
         {"resource": 0, "count": 40, "control_behavior": 2, "max_queueing_time_ms": 20, "limit_app": B},
         {"resource": 0, "count": 1, "grade": 0, "limit_app": "other"},
         {"resource": 1, "count": 30}]
RULED_2 = [dict(r, count=r["count"] + 5) if r.get("limit_app") == A else r for r in RULED]  # the reload


@functools.lru_cache(maxsize=None)
def _ruled_trace():
    """Resource 0 under limitApp A (Default QPS), B (RateLimiter), other (Default THREAD) and a default WarmUp
    rule, resource 1 plain; traffic from A, B, the unnamed C and D and origin 0; 6,000 entries, a rule reload
    after 3,000 (raters reset, origin nodes kept).  The seed was picked with the oracles alone so that the
    floors below hold."""
    h = ot.OriginTrace(2, 4, RULED)
    h.generate(3000, 3, T0, [4, 1], [1, 3, 3, 2, 2], gap_mean=4.0, acq_max=2, rt_max=39, regress_pct=0.01, err_pct=0.1)
    mark = len(h.ev)
    h.load(RULED_2)
    t1 = int(h.ev[-1][2]) + 5
    h.generate(3000, 4, t1, [4, 1], [1, 3, 3, 2, 2], gap_mean=4.0, acq_max=2, rt_max=39, err_pct=0.1)
    tr = h.finish()
    tr["mark"] = mark
    c = tr["counts"]
    assert c["origin_block"] >= 50 and c["default_block"] >= 50, c
    assert c["full_pass"].get(A, 0) >= 50 and c["full_pass"].get(B, 0) >= 50, c
    st, ed, ew = tr["st"], tr["ed"], tr["ew"]
    flow = (st["kind"] == 0) & (st["resource"] == 0) & (ed == 1)
    assert all(((ew == k) & flow).sum() >= 20 for k in range(4)), np.bincount(ew[flow])  # every rule blocks
    return tr


RULED_PATHS = [("chunks_100", 100, 0), ("chunks_3000", 3000, 0), ("small", 700, None)]


@pytest.mark.parametrize("path,chunk,small", RULED_PATHS, ids=[p[0] for p in RULED_PATHS])
def test_origin_rules(path, chunk, small):
    """Chunks of 100 (the group's segment stays on its k_lflows lane, below 128 events), of 3000 (k_lgroup) and
    the small path; the reload falls between two chunks."""
    tr = _ruled_trace()
    st, mark = tr["st"], tr["mark"]
    eng, s = _sentinel(2, 4, 1 << 12, small)
    assert _load_flow(s, RULED) == len(RULED)
    assert s.group_of(0) == 0 and s.group_of(1) == 0xFFFFFFFF
    gd, gw = [], []
    for lo, hi in [(0, mark), (mark, len(tr["ed"]))]:
        for a in range(lo, hi, chunk):
            d, w = _submit(s, lt.slice_stream(st, a, min(a + chunk, hi)))
            gd.append(d)
            gw.append(w)
        if hi == mark:
            assert _load_flow(s, RULED_2) == len(RULED_2)
    _same(st, (np.concatenate(gd), np.concatenate(gw)), tr["ed"], tr["ew"], path)
    _nodes(s, tr, 2, 4, path)
    eng.close()


def test_origin_rules_device_entry_and_arrival_order_lane():
    """The same stream up to the reload through sga_submit_events_origin_device, and (inbound, under a SystemRule
    that never blocks) through k_lseq: decisions only, the nodes are compared on the host paths above."""
    tr = _ruled_trace()
    st = lt.slice_stream(tr["st"], 0, tr["mark"])
    ed, ew = tr["ed"][:tr["mark"]], tr["ew"][:tr["mark"]]
    eng, s = _sentinel(2, 4, 1 << 13, 0)
    _load_flow(s, RULED)
    d, w = _device(s, st)
    s.device_status()
    _same(st, (d.cpu().numpy(), w.cpu().numpy()), ed, ew, "device")
    eng.close()
    eng, s = _sentinel(2, 4, 1 << 13, 0)
    _load(s, system=MIX_SYSTEM)
    _load_flow(s, RULED)
    _same(st, _submit(s, dict(st, flags=st["flags"] | 8)), ed, ew, "seq")
    eng.close()


def test_relate_rule_with_a_limit_app():
    """Hand computed.  Resource 0: limitApp o1, RELATE to resource 1, QPS 1 -- the rule reads resource 1's
    ClusterNode for entries from o1 and nobody else's (FlowRuleChecker.java:136-166), null until resource 1 is
    entered."""
    eng, s = _sentinel(2, 2, 1 << 12)
    assert _load_flow(s, [{"resource": 0, "count": 1, "limit_app": 1, "ref": 1}]) == 1
    st = _ev([(0, 0, T0 + 1, 1, 0, 0, 0, 1),    # o1, resource 1 never entered: passes
              (0, 1, T0 + 2, 1, 0, 0, 0, 0),    # resource 1 passes 1
              (0, 0, T0 + 3, 1, 0, 0, 0, 1),    # o1: 1 + 1 > 1, blocked by rule 0
              (0, 0, T0 + 4, 1, 0, 0, 0, 2),    # o2: the rule does not apply
              (0, 0, T0 + 5, 1, 0, 0, 0, 0)])   # no origin: the rule does not apply
    d, w = _submit(s, st)
    assert list(d) == [0, 0, 1, 0, 0] and w[2] == 0, (d, w)
    v = s.origin_node(0, 1, T0 + 6)
    assert (v.total_pass, v.total_block, v.cur_thread_num) == (1, 1, 1)
    assert s.origin_node(0, 2, T0 + 6).total_pass == 1 and s.node(0, T0 + 6).total_block == 1
    eng.close()


# ------------------------------------------------------------------ 4: edges
def _ev(rows):
    x = np.array(rows, dtype=np.int64).reshape(-1, 8)
    return {"kind": x[:, 0].astype(np.uint8), "resource": x[:, 1].astype(np.uint32), "ts": x[:, 2].copy(),
            "acquire": x[:, 3].astype(np.int32), "flags": x[:, 4].astype(np.uint8), "rt": x[:, 5].copy(),
            "param": x[:, 6].astype(np.uint64), "origin": x[:, 7].astype(np.uint32)}


@pytest.mark.parametrize("small", [None, 0], ids=["small", "pipeline"])
def test_blocked_revoked_and_orphan_exit_events(small):
    """Kind 2 and kind 3 events with an origin create and count; an exit of a pair never entered does not."""
    h = ot.OriginTrace(3, 3, [{"resource": 0, "count": 2}])
    t = T0
    h.other(2, 1, 2, t, 3)                 # a block outside the engine creates (1, 2)
    for k in range(4):                     # two passes, two blocks from origin 1
        h.entry(0, 1, t + 1 + k, 1)
    h.other(3, 0, 1, t + 1, 1)             # the first pass revoked
    h.other(1, 0, 1, t + 40, 1, 2, 38)     # the second exits with an error
    h.other(1, 2, 3, t + 41, 1, 0, 5)      # an exit of (2, 3): no node before, none after
    h.other(1, 0, 3, t + 42, 1, 0, 5)      # an exit of (0, 3), whose resource has other origin nodes
    h.other(3, 2, 1, t + 43, 2)            # a revoke creates (2, 1)
    assert h.created == {(1, 2), (0, 1), (2, 1)}
    tr = h.finish()
    eng, s = _sentinel(3, 3, 1 << 12, small)
    _load(s, [{"resource": 0, "count": 2}])
    _same(tr["st"], _submit(s, tr["st"]), tr["ed"], tr["ew"], "edges")
    _nodes(s, tr, 3, 3, "edges")
    eng.close()


def test_exit_ahead_of_the_pair_s_first_entry_in_one_chunk():
    """The node exists from the entry on: an exit that arrives before it, in the same chunk, counts nothing."""
    for small in (None, 0):
        h = ot.OriginTrace(1, 1)
        h.other(1, 0, 1, T0, 1, 0, 7)
        h.entry(0, 1, T0 + 1, 1)
        h.other(1, 0, 1, T0 + 9, 1, 0, 8)
        tr = h.finish()
        assert tr["onodes"][(0, 1)][0][lt.NODE_GETTERS.index("total_success")] == 1
        eng, s = _sentinel(1, 1, 1 << 12, small)
        _same(tr["st"], _submit(s, tr["st"]), tr["ed"], tr["ew"], "early exit")
        _nodes(s, tr, 1, 1, "early exit")
        eng.close()


def test_pass_wait_counts_a_thread_only():
    """PriorityWaitException (StatisticSlot.java:101-104): the origin node gets the thread and no pass.  Hand
    computed: QPS 1; the first entry (origin 2) passes, the prioritized second (origin 1) occupies the next
    bucket, whose pass the first bucket's expiry frees, and waits for it: 400 ms."""
    rules = [{"resource": 0, "count": 1}]
    st = _ev([(0, 0, T0 + 100, 1, 0, 0, 0, 2), (0, 0, T0 + 600, 1, 1, 0, 0, 1)])
    orc = lt.Oracle(1, rules)
    od, ow = orc.replay({k: v for k, v in st.items() if k != "origin"})
    orc.close()
    assert list(od) == [0, 4] and list(ow) == [0, 400]
    eng, s = _sentinel(1, 2, 1 << 12)
    _load(s, rules)
    _same(st, _submit(s, st), od, ow, "pass wait")
    now = T0 + 601
    a, b = s.origin_node(0, 1, now), s.origin_node(0, 2, now)
    assert (a.cur_thread_num, a.total_pass, a.total_block, a.pass_qps) == (1, 0, 0, 0.0)
    assert (b.cur_thread_num, b.total_pass, b.total_block, b.pass_qps) == (1, 1, 0, 1.0)
    assert s.node(0, now).cur_thread_num == 2
    eng.close()


def test_origin_id_past_the_registered_ones_refuses_the_chunk():
    from sentinel_amd._lib import EngineError
    eng, s = _sentinel(2, 3, 1 << 12)
    good = _ev([(0, 0, T0, 1, 0, 0, 0, 1), (0, 1, T0 + 1, 1, 0, 0, 0, 3)])
    bad = _ev([(0, 0, T0 + 2, 1, 0, 0, 0, 2), (0, 1, T0 + 3, 1, 0, 0, 0, 4)])
    _submit(s, good)
    before = [_view(s.node(r, T0 + 10)) for r in range(2)]
    with pytest.raises(EngineError, match=EINVAL):
        _submit(s, bad)
    d, _ = _device(s, bad)
    with pytest.raises(EngineError, match=EINVAL):
        s.device_status()
    assert (d.cpu().numpy() == -1).all()
    assert [_view(s.node(r, T0 + 10)) for r in range(2)] == before
    assert s.origin_nodes(0) == ["o1"] and s.origin_nodes(1) == ["o3"]
    assert s.origin_node(0, 2, T0 + 10) is None
    eng.close()


@pytest.mark.parametrize("entry", ["host", "small", "device"])
def test_full_table_refuses_the_chunk(entry):
    """max_origin_nodes = 4 and a fifth pair: SGA_ENOMEM, nothing of the chunk applied anywhere."""
    from sentinel_amd._lib import EngineError
    eng, s = _sentinel(3, 3, 1 << 12, None if entry == "small" else 0, max_nodes=4)
    _load(s, [{"resource": 0, "count": 5}])
    four = _ev([(0, 0, T0, 1, 0, 0, 0, 1), (0, 0, T0 + 1, 1, 0, 0, 0, 2), (0, 1, T0 + 2, 1, 0, 0, 0, 1),
                (0, 2, T0 + 3, 1, 0, 0, 0, 3)])
    assert list(_submit(s, four)[0]) == [0, 0, 0, 0]
    now = T0 + 20
    before = [_view(s.node(r, now)) for r in range(3)]
    obefore = {(r, o): _view(s.origin_node(r, o, now)) for r in range(3) for o in (1, 2, 3)}
    assert sum(v is not None for v in obefore.values()) == 4
    fifth = _ev([(0, 0, T0 + 5, 1, 0, 0, 0, 1), (0, 1, T0 + 6, 1, 0, 0, 0, 2), (1, 0, T0 + 7, 1, 0, 3, 0, 1)])
    if entry == "device":
        d, _ = _device(s, fifth)
        with pytest.raises(EngineError, match=ENOMEM):
            s.device_status()
        assert (d.cpu().numpy() == -1).all()
    else:
        with pytest.raises(EngineError, match=ENOMEM):
            _submit(s, fifth)
    assert [_view(s.node(r, now)) for r in range(3)] == before
    assert {(r, o): _view(s.origin_node(r, o, now)) for r in range(3) for o in (1, 2, 3)} == obefore
    assert [s.origin_nodes(r) for r in range(3)] == [["o1", "o2"], ["o1"], ["o3"]]
    # the table still serves the pairs it holds
    again = _ev([(1, 0, T0 + 8, 1, 0, 8, 0, 1), (0, 2, T0 + 9, 2, 0, 0, 0, 3)])
    assert list(_submit(s, again)[0]) == [0, 0]
    v = s.origin_node(0, 1, now)
    assert (v.cur_thread_num, v.total_success, v.total_pass) == (0, 1, 1)
    assert s.origin_node(2, 3, now).total_pass == 3
    eng.close()


def test_unknown_limit_app_is_counted_and_never_applies():
    """A rule whose limitApp names an origin no event can carry is valid and counted (FlowRuleUtil.isValidRule)
    and selects no node for anybody (FlowRuleChecker.java:136-166)."""
    from sentinel_amd.local import FlowRuleManager
    from sentinel_amd.rules import FlowRule
    for listed_first in (True, False):
        eng, s = _sentinel(1, 1, 1 << 12)
        rules = [FlowRule(resource="r0", count=0, limit_app="nobody"), FlowRule(resource="r0", count=2)]
        assert FlowRuleManager(s).load_rules(rules if listed_first else rules[::-1]) == 2
        st = _ev([(0, 0, T0 + k, 1, 0, 0, 0, 1) for k in range(3)])
        d, w = _submit(s, st)
        # the default rule alone decides; FlowRuleComparator puts it after the other: block detail 1
        assert list(d) == [0, 0, 1] and w[2] == 1, (listed_first, d, w)
        eng.close()


def test_comparator_order_inside_the_cluster_mode_rules():
    """FlowRuleComparator (FlowRuleComparator.java:30-55): cluster-mode rules last, and among them, as among the
    others, a non-default limitApp first.  No token service: both cluster rules fall back to their local check,
    where the unknown limitApp selects no node and the default one (count 0) blocks -- at index 2, after the
    plain default rule and the cluster-mode rule with the unknown limitApp, however the two are listed."""
    from sentinel_amd.local import FlowRuleManager
    from sentinel_amd.rules import ClusterFlowConfig, FlowRule
    for listed_first in (True, False):
        eng, s = _sentinel(1, 1, 1 << 12)
        cl = [FlowRule(resource="r0", count=0, cluster_mode=True, cluster_config=ClusterFlowConfig(flow_id=7)),
              FlowRule(resource="r0", count=0, limit_app="nobody", cluster_mode=True,
                       cluster_config=ClusterFlowConfig(flow_id=8))]
        rules = (cl if listed_first else cl[::-1]) + [FlowRule(resource="r0", count=100)]
        assert FlowRuleManager(s).load_rules(rules) == 3
        d, w = _submit(s, _ev([(0, 0, T0, 1, 0, 0, 0, 1)]))
        # order: plain default (0), cluster unknown (1), cluster default (2)
        assert (int(d[0]), int(w[0])) == (1, 2), (listed_first, d, w)
        eng.close()


def test_bad_id_wins_over_a_full_table_on_both_entries():
    from sentinel_amd._lib import EngineError
    eng, s = _sentinel(2, 3, 1 << 12, 0, max_nodes=1)
    both = _ev([(0, 0, T0, 1, 0, 0, 0, 1), (0, 1, T0 + 1, 1, 0, 0, 0, 2), (0, 1, T0 + 2, 1, 0, 0, 0, 9)])
    with pytest.raises(EngineError, match=EINVAL):
        _submit(s, both)
    d, _ = _device(s, both)
    with pytest.raises(EngineError, match=EINVAL):
        s.device_status()
    assert (d.cpu().numpy() == -1).all()
    eng.close()
