"""Metric extensions on the GPU: the sums StatisticSlot's callbacks (MetricEntryCallback / MetricExitCallback,
StatisticSlot.java:65-175) would have formed, added by k_mx_add after each chunk's last kernel on every submit
entry and moved out by sga_metric_ext_drain.

The reference is tests/metric_ext_cases.add_reference: a dict over the same call's input columns and the decision
and wait arrays it returned.  Everything is an integer sum: every comparison in this file is an equality."""
import itertools

import numpy as np
import pytest

from tests import metric_ext_cases as mc
from tests.block_log_cases import T0

pytestmark = pytest.mark.gpu


def _flow(s, rules):
    from sentinel_amd.local import FlowRuleManager
    from sentinel_amd.rules import FlowRule
    return FlowRuleManager(s).load_rules([FlowRule(resource=s.resources[r], count=c) for r, c in rules])


def _sentinel(n_res, metric_extensions=True, max_batch=1 << 16, origins=None):
    from sentinel_amd.cluster import Engine
    from sentinel_amd.local import LocalSentinel
    eng = Engine(max_batch=max_batch)
    return eng, LocalSentinel(eng, [f"r{i}" for i in range(n_res)], origins, metric_extensions=metric_extensions)


def _submit(s, st):
    return s.submit(st["kind"], st["resource"], st["ts"], st["acquire"], st["flags"], st["rt"], st["param"],
                    origin=st.get("origin"))


def _ref(acc, s, st, d, w):
    return mc.add_reference(acc, len(s.resources), st["kind"], st["resource"], st["acquire"], st["flags"], st["rt"],
                            d, w, st.get("origin"))


def _drain_equals(s, acc):
    res, blk, le, lc = s.metric_ext_rows()
    assert (le, lc) == (0, 0)
    assert mc.res_tuples(res) == mc.expected_res(acc)
    assert mc.block_tuples(blk) == mc.expected_block(acc)
    return res, blk


def _device(s, st):
    import torch
    dev = torch.device("cuda", 0)
    base = int(st["ts"].min())
    off = (st["ts"] - base).astype(np.uint32).view(np.int32)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    return s.submit_device(t(st["kind"], np.uint8), t(st["resource"], np.int32), base, t(off, np.int32),
                           t(st["acquire"], np.int32), flags=t(st["flags"], np.uint8), rt=t(st["rt"], np.int64),
                           param=t(st["param"], np.int64))


# ------------------------------------------------------------------ 1: seams
_seam_case = itertools.count(1)


@pytest.fixture(scope="module")
def seam_engine():
    """One sentinel for every seam case: each case drains everything it summed."""
    eng, s = _sentinel(mc.SEAM_RES)
    yield s
    eng.close()


@pytest.mark.parametrize("acq_hi", [1, 3])
@pytest.mark.parametrize("pattern", ["one", "distinct"])
@pytest.mark.parametrize("n", mc.SEAM_SIZES)
def test_seams(seam_engine, n, pattern, acq_hi):
    """Every size around the wave (64), the tile (256) and the small-batch threshold (1,024 / 1,025), every event on
    one resource (the wave combine and the held resource) against a resource of its own for every event; passes,
    flow blocks, priority waits, exits with and without an error and kind 2 / 3 events interleaved."""
    s = seam_engine
    shift = 10_000 * next(_seam_case)  # a fresh pair of seconds, later than every earlier case's
    _flow(s, mc.rules(n))
    st = mc.stream(n, pattern, acq_hi)
    st["ts"] = st["ts"] + shift
    d, w = _submit(s, st)
    acc = _ref(mc.new_acc(), s, st, d, w)
    ent = st["kind"] == 0
    assert (d[~ent] == 0).all()
    if n >= 256:  # the stream really holds every class of event
        de = d[ent]
        print("entry decisions", {int(k): int((de == k).sum()) for k in np.unique(de)})
        assert (de == 0).any() and (de == 1).any() and (de == 4).any(), "passes, flow blocks, priority waits"
        assert {0, 1, 2, 3} <= set(st["kind"].tolist())
        ex = st["kind"] == 1
        assert (st["flags"][ex] & mc.EV_ERROR).any() and not (st["flags"][ex] & mc.EV_ERROR).all()
        lines = mc.expected_res(acc)
        if pattern == "one":
            assert len(lines) == 1 and lines[0][0] == mc.R_ONE
            assert 0 < lines[0][5] < lines[0][3], "errors are a part of the exits"
            assert lines[0][2] >= 5 and lines[0][4] == n // 4, "passes and exits meet on one line"
        else:
            assert len(lines) >= n // 2
        if acq_hi == 3:
            assert any(ln[1] != ln[2] for ln in lines), "acquire sums differ from event counts"
    _drain_equals(s, acc)
    res, blk, le, lc = s.metric_ext_rows()
    assert (len(res), len(blk), le, lc) == (0, 0, 0, 0), "a second drain returns nothing"


# ------------------------------------------------------------------ 2: the three differences from the node
def test_the_sums_are_not_the_nodes():
    eng, s = _sentinel(3)
    try:
        _flow(s, [(0, 5.0)])
        # (a) priority waits: onPass runs for them, node.addPassRequest does not
        # (eight plain entries fill the second's first half-second bucket; the prioritized ones behind them, in its
        # second bucket, can borrow from the next second, where that bucket will have left the window)
        n = 40
        late = np.arange(n) >= 8
        st = {"kind": np.zeros(n, np.uint8), "resource": np.zeros(n, np.uint32),
              "ts": T0 + np.where(late, 600, 100) + np.arange(n, dtype=np.int64), "acquire": np.ones(n, np.int32),
              "flags": np.where(late, mc.EV_PRIORITIZED, 0).astype(np.uint8), "rt": np.zeros(n, np.int64),
              "param": np.zeros(n, np.uint64)}
        d, w = _submit(s, st)
        waits, passes = int((d == 4).sum()), int((d == 0).sum())
        assert waits > 0 and passes > 0
        res, blk, _, _ = s.metric_ext_rows()
        assert len(res) == 1 and int(res[0]["pass"]) == passes + waits == int(res[0]["pass_events"])
        # StatisticSlot's PriorityWaitException branch calls onPass but no node.addPassRequest: the passes the node
        # holds for the entries' own second (its one-second window: passQps x 1 s) are the plain ones, the waits
        # sit in the borrow array as `waiting` and surface as passes of the next second.  Only the minute counter has
        # them already -- DefaultController calls node.addOccupiedPass, which adds to rollingCounterInMinute
        # (StatisticNode.java:347-350) -- so total_pass is no place to see the difference: 10 = 5 + 5 here.
        node = s.node(0, T0 + 700)
        node_pass = node.pass_qps * 1.0  # IntervalProperty.INTERVAL = 1 s
        print("ext pass", int(res[0]["pass"]), "node pass of the second", node_pass, "waiting", node.waiting,
              "minute total", node.total_pass)
        assert node_pass == passes and node.waiting == waits, "the node counts no pass for a PriorityWaitException"
        assert int(res[0]["pass"]) > node_pass
        assert node.total_pass == passes + waits, "addOccupiedPass feeds the minute counter"
        # (b) raw rt: the node caps at statistic_max_rt, the extension gets completeTime - createTimestamp
        assert s.statistic_max_rt == 5000
        k = 6
        st = {"kind": np.r_[np.zeros(k, np.uint8), np.ones(k, np.uint8)], "resource": np.full(2 * k, 1, np.uint32),
              "ts": T0 + 1100 + np.arange(2 * k, dtype=np.int64), "acquire": np.ones(2 * k, np.int32),
              "flags": np.zeros(2 * k, np.uint8), "rt": np.r_[np.zeros(k, np.int64), np.full(k, 7000, np.int64)],
              "param": np.zeros(2 * k, np.uint64)}
        _submit(s, st)
        res, _, _, _ = s.metric_ext_rows()
        assert mc.res_tuples(res) == [(1, k, k, k, k, 0, 0, 7000 * k, 7000)]
        node = s.node(1, T0 + 1200)
        # statisticMaxRt acts on the node through MetricBucket.minRt, which starts there and only goes down
        # (MetricBucket.java:57, ArrayMetric.java:154): the node reports a minimum rt of 5,000 ms for exits that all
        # took 7,000.  (This reference no longer cuts the rt it sums: the node's average is the raw 7,000 too.)
        print("raw rt: ext rt_max", int(res[0]["rt_max"]), "node min_rt", node.min_rt, "avg_rt", node.avg_rt)
        assert node.total_success == k and node.min_rt == 5000.0, "the node's rt is capped"
        assert int(res[0]["rt_max"]) > node.min_rt and int(res[0]["rt_sum"]) == k * 7000
        # (c) a negative rt is summed as given; rt_max stays at least 0
        st = {"kind": np.asarray([0, 0, 1, 1], np.uint8), "resource": np.full(4, 2, np.uint32),
              "ts": T0 + 1300 + np.arange(4, dtype=np.int64), "acquire": np.ones(4, np.int32),
              "flags": np.zeros(4, np.uint8), "rt": np.asarray([0, 0, -5, -9], np.int64),
              "param": np.zeros(4, np.uint64)}
        _submit(s, st)
        res, _, _, _ = s.metric_ext_rows()
        assert mc.res_tuples(res) == [(2, 2, 2, 2, 2, 0, 0, -14, 0)]
        node = s.node(2, T0 + 1400)
        print("negative rt: node avg_rt", node.avg_rt)
        assert node.total_success == 2, "the node saw the same two exits"
        st["rt"] = np.asarray([0, 0, -5, 3], np.int64)
        st["ts"] = st["ts"] + 10
        _submit(s, st)
        res, _, _, _ = s.metric_ext_rows()
        assert mc.res_tuples(res) == [(2, 2, 2, 2, 2, 0, 0, -2, 3)]
    finally:
        eng.close()


# ------------------------------------------------------------------ 3: every block class, end to end
RES = ["flowres", "clres", "paramres", "degres", "sysres", "authres"]
ORIGINS = ["appA", "appB"]


def _scenario(metric_extensions):
    """The shape of test_block_log_gpu._scenario: one small sentinel with origins and one rule of every kind; the
    same entries with or without the sums.  Returns (engine, sentinel, rules by name, outcomes)."""
    from sentinel_amd.cluster import Engine
    from sentinel_amd.local import (AuthorityRuleManager, BlockException, DegradeRuleManager, FlowRuleManager,
                                    LocalSentinel, ParamFlowRuleManager, SystemRule, SystemRuleManager)
    from sentinel_amd.rules import (AuthorityRule, ClusterFlowConfig, DegradeRule, FlowRule, ParamFlowRule,
                                    RuleConstant)
    eng = Engine(max_batch=1 << 12)
    s = LocalSentinel(eng, RES, ORIGINS, metric_extensions=metric_extensions)
    R = {
        "flow_default": FlowRule(resource="flowres", count=0),
        "flow_appA": FlowRule(resource="flowres", count=0, limit_app="appA"),
        "cl_cluster": FlowRule(resource="clres", count=0, cluster_mode=True,
                               cluster_config=ClusterFlowConfig(flow_id=77)),
        "cl_appA": FlowRule(resource="clres", count=1000, limit_app="appA"),
        "param": ParamFlowRule(resource="paramres", param_idx=0, count=0),
        "degrade": DegradeRule(resource="degres", grade=RuleConstant.DEGRADE_GRADE_EXCEPTION_COUNT, count=0,
                               time_window=10, min_request_amount=1),
        "auth": AuthorityRule(resource="authres", limit_app="appB", strategy=RuleConstant.AUTHORITY_BLACK),
    }
    FlowRuleManager(s).load_rules([R["flow_default"], R["cl_cluster"], R["flow_appA"], R["cl_appA"]])
    ParamFlowRuleManager(s).load_rules([R["param"]])
    DegradeRuleManager(s).load_rules([R["degrade"]])
    AuthorityRuleManager(s).load_rules([R["auth"]])
    SystemRuleManager(s).load_rules([SystemRule(qps=0)])
    out = []

    def enter(res, t, **kw):
        try:
            e = s.entry(res, T0 + t, **kw)
            out.append("pass")
            return e
        except BlockException as x:
            out.append(type(x).__name__)
            return None

    enter("flowres", 10, origin="appA", batch_count=2)     # the appA rule: detail 0
    enter("flowres", 11, origin="appB")                    # the default rule: detail 1
    enter("flowres", 12, origin="appB", batch_count=3)     # again: one row, block 4
    enter("clres", 20, origin="appA")                      # the cluster-mode rule, sorted last: detail 1
    enter("paramres", 30, args=(7,))
    enter("paramres", 31, args=("bob",), batch_count=2)    # another parameter, the same rule: the same row
    e = enter("degres", 40)                                # passes; its failed exit opens the breaker
    e.trace_error()
    e.exit(T0 + 47)
    enter("degres", 48, origin="appB")
    enter("sysres", 50, entry_type="IN")                   # SystemRule qps 0 on inbound entries
    enter("authres", 60, origin="appB")                    # black-listed
    e = enter("authres", 61, origin="appA", batch_count=2)  # passes
    e.exit(T0 + 64)
    # a block thrown by a slot outside the engine (kind 2), from appB
    s.submit([2], [s.ids["sysres"]], [T0 + 70], [3], origin=[s.origin_ids["appB"]])
    return eng, s, R, out


def test_every_block_class_reaches_a_recording_extension():
    from sentinel_amd.metric_extension import AdvancedMetricExtension, MetricExtension

    class Basic(mc.Recorder, MetricExtension):
        def add_pass(self, *a, **k): self._rec("add_pass", *a, **k)
        def add_block(self, *a, **k): self._rec("add_block", *a, **k)
        def add_success(self, *a, **k): self._rec("add_success", *a, **k)
        def add_exception(self, *a, **k): self._rec("add_exception", *a, **k)
        def add_rt(self, *a, **k): self._rec("add_rt", *a, **k)
        def increase_thread_num(self, *a, **k): self._rec("increase_thread_num", *a, **k)
        def decrease_thread_num(self, *a, **k): self._rec("decrease_thread_num", *a, **k)

    class Advanced(mc.Recorder, AdvancedMetricExtension):
        def on_blocked(self, *a, **k): self._rec("on_blocked", *a, **k)

    eng, s, R, out = _scenario(True)
    try:
        assert out == ["FlowException"] * 4 + ["ParamFlowException"] * 2 + ["pass", "DegradeException",
                                                                           "SystemBlockException",
                                                                           "AuthorityException", "pass"]
        basic, adv = Basic(), Advanced()
        assert s.poll_metric_extensions() == 0, "no extension registered: nothing is drained"
        s.metric_extensions.add(basic)
        s.metric_extensions.add(adv)
        assert s.poll_metric_extensions() > 0
        blocks = [(a[0], a[1], a[2], type(a[3]).__name__, a[3].rule, dict(k)["events"])
                  for name, a, k in basic.calls if name == "add_block"]
        want = [("flowres", 2, "appA", "FlowException", R["flow_appA"], 1),
                ("flowres", 4, "appB", "FlowException", R["flow_default"], 2),
                ("clres", 1, "appA", "FlowException", R["cl_cluster"], 1),
                ("paramres", 3, "", "ParamFlowException", R["param"], 2),
                ("degres", 1, "appB", "DegradeException", R["degrade"], 1),
                ("sysres", 1, "", "SystemBlockException", None, 1),
                ("sysres", 3, "appB", "BlockException", None, 1),
                ("authres", 1, "appB", "AuthorityException", R["auth"], 1)]
        assert [b[:4] + b[5:] for b in blocks] == [x[:4] + x[5:] for x in want]
        for got, exp in zip(blocks, want):
            assert got[4] is exp[4], (got[:4], "the exception carries the loaded rule object itself")
        lim = {a[0] + "/" + a[2]: a[3].rule_limit_app for name, a, k in basic.calls if name == "add_block"}
        assert lim["flowres/appA"] == "appA" and lim["flowres/appB"] == "default" and lim["sysres/"] == "qps"
        assert lim["authres/appB"] == "appB"
        assert [(a[0], a[1], a[2], type(a[3]).__name__) for _, a, _ in adv.calls] == [b[:4] for b in blocks]
        # the passes and exits of the same poll: degres (one failed exit, rt 7), authres (acquire 2, rt 3)
        rest = [(name, a, k) for name, a, k in basic.calls if name != "add_block"]
        assert rest == [("increase_thread_num", ("degres",), (("times", 1),)),
                        ("add_pass", ("degres", 1), (("events", 1),)),
                        ("add_rt", ("degres", 7), (("events", 1), ("rt_max", 7))),
                        ("add_success", ("degres", 1), (("events", 1),)),
                        ("decrease_thread_num", ("degres",), (("times", 1),)),
                        ("add_exception", ("degres", 1, None), (("events", 1),)),
                        ("increase_thread_num", ("authres",), (("times", 1),)),
                        ("add_pass", ("authres", 2), (("events", 1),)),
                        ("add_rt", ("authres", 3), (("events", 1), ("rt_max", 3))),
                        ("add_success", ("authres", 2), (("events", 1),)),
                        ("decrease_thread_num", ("authres",), (("times", 1),))]
        basic.calls.clear()
        assert s.poll_metric_extensions() == 0 and basic.calls == [], "an empty drain makes no call"
    finally:
        eng.close()


# ------------------------------------------------------------------ 7: no side effects
def test_the_sums_have_no_side_effects():
    """A twin without the feature, fed the same entries and then the same stream: identical outcomes, decisions,
    waits and node views of every table; its drain answers SGA_EINVAL."""
    from sentinel_amd import _lib
    engs = []
    try:
        got = []
        for on in (True, False):
            eng, s, _, out = _scenario(on)
            engs.append(eng)
            st = mc.stream(1500, "one")
            st["resource"] = (np.arange(1500) % len(RES)).astype(np.uint32)
            st["origin"] = (np.arange(1500) % 3).astype(np.uint32)
            st["ts"] = st["ts"] + 2000
            d, w = _submit(s, st)
            views = []
            for now in (T0 + 100, T0 + 3500, T0 + 70_000):
                for table in (_lib.SGA_NODES_RESOURCE, _lib.SGA_NODES_ORIGIN, _lib.SGA_NODES_CONTEXT):
                    ids = list(range(len(RES))) + [0xFFFFFFFF] if table == _lib.SGA_NODES_RESOURCE else None
                    views.append(s.query_nodes(table, now, ids).tobytes())
            got.append((out, d.tobytes(), w.tobytes(), views))
            if not on:
                assert mc.drain_raw(s, 16, 16)[0] == mc.EINVAL
                assert s.metric_extensions is None
        assert got[0] == got[1]
    finally:
        for e in engs:
            e.close()


# ------------------------------------------------------------------ 4: entries
def _entry_stream():
    n = 300
    st = mc.stream(n, "distinct")
    st["resource"][::5] = mc.R_ONE  # some resources shared, most of their own
    return n, st


def test_every_entry_gives_the_same_rows():
    """The small path, the host pipeline, the device entry and the event queue, one engine each, the same stream."""
    from sentinel_amd import _lib
    n, st = _entry_stream()
    engs = []
    try:
        rows = {}
        for how in ("small", "pipeline", "device", "queue"):
            eng, s = _sentinel(mc.R_FIRST + n + 8)
            engs.append(eng)
            _flow(s, mc.rules(n))
            if how == "small":
                d, w = _submit(s, st)
            elif how == "pipeline":
                assert _lib.load().sga_set_small_batch(eng.handle, 0) == 0
                d, w = _submit(s, st)
            elif how == "device":
                d, w = _device(s, st)
                s.device_status()
                d, w = d.cpu().numpy(), w.cpu().numpy()
            else:
                dw = [s.event_one(int(st["kind"][i]), int(st["resource"][i]), int(st["ts"][i]),
                                  int(st["acquire"][i]), int(st["flags"][i]), int(st["rt"][i])) for i in range(n)]
                d, w = np.asarray([x[0] for x in dw], np.int8), np.asarray([x[1] for x in dw], np.int32)
            acc = _ref(mc.new_acc(), s, st, d, w)
            assert len(acc["block"]) > n // 8 and len(mc.expected_res(acc)) > n // 4
            res, blk = _drain_equals(s, acc)
            rows[how] = (res.tobytes(), blk.tobytes())
        assert rows["small"] == rows["pipeline"] == rows["device"] == rows["queue"]
        # (s: the queue sentinel) posted exits are decided before the drain that follows them
        s.event_post(1, mc.R_ONE, int(st["ts"][-1]) + 1, 2, 0, 9)
        res, blk, _, _ = s.metric_ext_rows()
        assert mc.res_tuples(res) == [(mc.R_ONE, 0, 0, 2, 1, 0, 0, 9, 9)] and len(blk) == 0
    finally:
        for e in engs:
            e.close()


def test_a_refused_chunk_and_unknown_resources_add_nothing():
    from sentinel_amd._lib import EngineError
    n, st = _entry_stream()
    eng, s = _sentinel(mc.R_FIRST + n + 8)
    try:
        _flow(s, mc.rules(n))
        # a chunk the gate refuses (a negative acquire) answers -1 everywhere and adds nothing
        bad = {k: v.copy() for k, v in st.items()}
        bad["acquire"][11] = -1
        d, w = _device(s, bad)
        with pytest.raises(EngineError, match="rc=-22"):
            s.device_status()
        assert (d.cpu().numpy() == -1).all()
        res, blk, le, lc = s.metric_ext_rows()
        assert (len(res), len(blk), le, lc) == (0, 0, 0, 0)
        # an unknown resource id adds nothing: such events pass (no node, no rules), the rest of the call counts
        unk = {k: v.copy() for k, v in st.items()}
        unk["ts"] = unk["ts"] + 5000
        unk["resource"][8:40] = mc.R_FIRST + n + 8 + np.arange(32)
        assert {0, 1, 2, 3} <= set(unk["kind"][8:40].tolist())
        for dev in (False, True):
            if dev:
                d, w = _device(s, unk)
                s.device_status()
                d, w = d.cpu().numpy(), w.cpu().numpy()
            else:
                d, w = _submit(s, unk)
            assert (d[8:40] == 0).all()
            acc = _ref(mc.new_acc(), s, unk, d, w)
            res, blk = _drain_equals(s, acc)
            assert len(res) and int(res["resource"].max()) < len(s.resources)
            unk["ts"] = unk["ts"] + 5000
    finally:
        eng.close()


# ------------------------------------------------------------------ 5: persistence and drain
def _mixed(n, res, t_lo, t_hi, seed):
    rng = np.random.default_rng(seed)
    kind = rng.choice(np.asarray([0, 0, 1], np.uint8), n).astype(np.uint8)
    return {"kind": kind, "resource": rng.choice(np.asarray(res, np.uint32), n).astype(np.uint32),
            "ts": np.sort(rng.integers(t_lo, t_hi, n)).astype(np.int64),
            "acquire": rng.choice(np.asarray([1, 3], np.int32), n).astype(np.int32),
            "flags": np.where(kind == 1, rng.choice(np.asarray([0, 2], np.uint8), n), 0).astype(np.uint8),
            "rt": np.where(kind == 1, rng.integers(0, 9000, n), 0).astype(np.int64), "param": np.zeros(n, np.uint64)}


def test_sums_persist_across_chunks_and_calls_and_drain_as_deltas():
    from sentinel_amd import _lib
    from sentinel_amd.cluster import Engine
    from sentinel_amd.local import LocalSentinel
    eng = Engine(max_batch=2048)
    s = LocalSentinel(eng, [f"r{i}" for i in range(6)])
    try:
        _flow(s, [(0, 0.0), (1, 50.0)])
        # traffic before the feature is on counts for nothing
        st = _mixed(500, [0, 1, 2], T0, T0 + 1000, 1)
        _submit(s, st)
        assert mc.drain_raw(s, 8, 64)[0] == mc.EINVAL
        assert _lib.load().sga_metric_ext_enable(eng.handle, 64) == 0
        s.metric_ext_block_rows = 64
        rc, nr, nb, _, _, le, lc = mc.drain_raw(s, 8, 64)
        assert (rc, nr, nb, le, lc) == (0, 0, 0, 0, 0), "enabling after traffic counts from then on"
        acc = mc.new_acc()
        # one call of three chunks (2,048 + 2,048 + 904: two through the pipeline, one through k_lsmall)
        st = _mixed(5000, [0, 1, 2, 3], T0 + 1000, T0 + 2000, 2)
        _ref(acc, s, st, *_submit(s, st))
        # a second call
        st = _mixed(3000, [1, 2, 4], T0 + 2000, T0 + 3000, 3)
        _ref(acc, s, st, *_submit(s, st))
        want_res, want_blk = mc.expected_res(acc), mc.expected_block(acc)
        assert len(want_res) == 5 and len(want_blk) == 2
        assert any(ln[8] > 5000 for ln in want_res), "rt_max is uncapped"
        # either cap too small: SGA_ERANGE, both counts as needed, nothing changed
        for rcap, bcap in ((4, 64), (8, 1), (0, 0)):
            rc, nr, nb, _, _, _, _ = mc.drain_raw(s, rcap, bcap)
            assert (rc, nr, nb) == (mc.ERANGE, 5, 2), (rcap, bcap)
        rc, nr, nb, res, blk, le, lc = mc.drain_raw(s, 5, 2)
        assert (rc, nr, nb, le, lc) == (0, 5, 2, 0, 0)
        assert mc.res_tuples(res) == want_res and mc.block_tuples(blk) == want_blk
        # a drain returns deltas: the next one holds the third call alone
        acc = mc.new_acc()
        st = _mixed(1500, [0, 1, 5], T0 + 3000, T0 + 4000, 4)
        _ref(acc, s, st, *_submit(s, st))
        _drain_equals(s, acc)
        # a revoke drained apart from its entry is a negative delta
        s.submit([3], [2], [T0 + 4100], [3])
        res, blk, _, _ = s.metric_ext_rows()
        assert mc.res_tuples(res) == [(2, -3, -1, 0, 0, 0, 0, 0, 0)]
        assert mc.block_tuples(blk) == [(2, 0, 0, 0, 3, 1)]
        # with nothing pending the block table may be resized; with sums pending it may not
        assert _lib.load().sga_metric_ext_enable(eng.handle, 128) == 0
        s.submit([0], [2], [T0 + 4200], [1])
        assert _lib.load().sga_metric_ext_enable(eng.handle, 256) == mc.EINVAL
        assert mc.res_tuples(s.metric_ext_rows()[0]) == [(2, 1, 1, 0, 0, 0, 0, 0, 0)]
    finally:
        eng.close()


# ------------------------------------------------------------------ 6: overflow
def test_block_rows_overflow_into_the_lost_counters():
    """Block-row capacity 64, 4,097 distinct (resource, origin) block keys in one call.  Conservation is an equality:
    what the rows do not hold, the lost counters do; the per-resource sums cannot overflow and are unaffected."""
    n = 4097
    eng, s = _sentinel(n + 1, metric_extensions=64, origins=["appA", "appB"])
    try:
        _flow(s, [(r, 0.0) for r in range(n)])
        m = 2 * n
        i = np.arange(m)
        st = {"kind": (i % 2).astype(np.uint8),                       # a block, then an exit on the free resource
              "resource": np.where(i % 2 == 0, i // 2, n).astype(np.uint32),
              "ts": T0 + (i * 900) // m, "acquire": np.where(i % 3 == 0, 3, 1).astype(np.int32),
              "flags": np.zeros(m, np.uint8), "rt": np.where(i % 2 == 1, 4, 0).astype(np.int64),
              "param": np.zeros(m, np.uint64), "origin": (1 + (i // 2) % 2).astype(np.uint32)}
        d, w = _submit(s, st)
        ent = st["kind"] == 0
        assert (d[ent] == 1).all()
        acc = _ref(mc.new_acc(), s, st, d, w)
        assert len(acc["block"]) == n
        res, blk, lost_events, lost_count = s.metric_ext_rows()
        assert 0 < len(blk) <= 64 and lost_events > 0
        got = mc.block_tuples(blk)
        assert len({g[:4] for g in got}) == len(got), "no key twice"
        for g in got:
            assert g[:4] in acc["block"], "a row of no true key"
            assert tuple(acc["block"][g[:4]]) == g[4:], "one event a key: a row holds all of it"
        assert sum(g[4] for g in got) + lost_count == int(st["acquire"][ent].sum())
        assert sum(g[5] for g in got) + lost_events == n
        assert mc.res_tuples(res) == mc.expected_res(acc) and len(res) == 1 and int(res[0]["exits"]) == n
        res, blk, lost_events, lost_count = s.metric_ext_rows()
        assert (len(res), len(blk), lost_events, lost_count) == (0, 0, 0, 0), "the drain cleared the counters"
    finally:
        eng.close()
