"""Block log on the GPU: LogSlot's per-second block counts (LogSlot.java:34-47 -> EagleEyeLogUtil.log ->
StatLogger) aggregated by k_blog_add after each chunk's last kernel, on all three submit entries.

The reference of the aggregation is tests/block_log_cases.add_reference: a dict over the same call's returned
decision and wait arrays and its input columns; rows must equal it exactly (count and events are integer sums, so
there is no tolerance anywhere in this file)."""
import datetime
import itertools

import numpy as np
import pytest

from tests import block_log_cases as bc
from tests.block_log_cases import T0

pytestmark = pytest.mark.gpu

UTC = datetime.timezone.utc
ERANGE, EINVAL = -34, -22


def _flow(s, rules):
    from sentinel_amd.local import FlowRuleManager
    from sentinel_amd.rules import FlowRule
    return FlowRuleManager(s).load_rules([FlowRule(resource=s.resources[r], count=c) for r, c in rules])


def _sentinel(n_res, block_log=True, max_batch=1 << 16, origins=None):
    from sentinel_amd.cluster import Engine
    from sentinel_amd.local import LocalSentinel
    eng = Engine(max_batch=max_batch)
    return eng, LocalSentinel(eng, [f"r{i}" for i in range(n_res)], origins, block_log=block_log)


def _submit(s, st):
    return s.submit(st["kind"], st["resource"], st["ts"], st["acquire"], st["flags"], st["rt"], st["param"])


def _ref(acc, st, d, w):
    return bc.add_reference(acc, st["kind"], st["resource"], st["ts"], st["acquire"], d, w)


# ------------------------------------------------------------------ 1: seams
_seam_case = itertools.count(1)


@pytest.fixture(scope="module")
def seam_engine():
    """One sentinel for every seam case: each case drains everything it logged."""
    eng, s = _sentinel(bc.SEAM_RES)
    _flow(s, bc.seam_rules(max(bc.SEAM_SIZES)))
    yield s
    eng.close()


@pytest.mark.parametrize("pattern", ["one", "distinct"])
@pytest.mark.parametrize("n", bc.SEAM_SIZES)
def test_seams(seam_engine, n, pattern):
    """Every size around the wave (64), the block (256) and the small-batch threshold (1,024 / 1,025: k_lsmall over
    page-locked memory against the pipeline), one key for every block against a key of its own for every block, two
    seconds, acquire in {1, 3}; passes, exits, SGA_PASS_WAIT and kind 2 / 3 events interleaved."""
    s = seam_engine
    # each case starts a fresh pair of seconds, later than every earlier case's (the R_PACE windows move on)
    shift = 10_000 * next(_seam_case)
    st = bc.seam_stream(n, pattern)
    st["ts"] = st["ts"] + shift
    d, w = _submit(s, st)
    acc = _ref({}, st, d, w)
    ent = st["kind"] == 0
    assert (d[ent & (st["resource"] != bc.R_PACE) & (st["resource"] != bc.R_FREE)] == 1).all()
    assert (d[~ent] == 0).all()
    if n >= 256:  # the stream holds what must never appear: passes, waits, exits, kind 2 / 3
        pace = d[st["resource"] == bc.R_PACE]
        print("R_PACE decisions", {int(k): int((pace == k).sum()) for k in np.unique(pace)})
        assert (pace == 0).any() and (pace == 4).any() and (pace == 1).any()
        assert {0, 1, 2, 3} <= set(st["kind"].tolist())
        assert len({k[0] for k in acc}) == 2, "the blocks straddle a second"
        assert any(v[0] != v[1] for v in acc.values()), "count differs from events"
    rows, le, lc = s.block_rows()
    assert (le, lc) == (0, 0)
    assert bc.as_tuples(rows) == bc.expected_tuples(acc)
    if pattern == "one":
        assert len({(k[1], k[2]) for k in acc if k[1] == bc.R_HOT}) == 1
    else:
        assert len(acc) >= (5 * n) // 8
    rows, le, lc = s.block_rows()
    assert len(rows) == 0 and (le, lc) == (0, 0), "a drained log is empty"


# ------------------------------------------------------------------ 2 and 6: every exception class, end to end
RES = ["flowres", "clres", "paramres", "degres", "sysres", "authres"]
ORIGINS = ["appA", "appB"]


def _scenario(block_log):
    """One small sentinel with origins and one rule of every kind; the same entries with or without the log.
    Returns (engine, sentinel, rules by name, outcomes): outcomes = per entry the exception class name (or "pass"),
    its rule and its rule_limit_app."""
    from sentinel_amd.cluster import Engine
    from sentinel_amd.local import (AuthorityRuleManager, BlockException, DegradeRuleManager, FlowRuleManager,
                                    LocalSentinel, ParamFlowRuleManager, SystemRule, SystemRuleManager)
    from sentinel_amd.rules import (AuthorityRule, ClusterFlowConfig, DegradeRule, FlowRule, ParamFlowRule,
                                    RuleConstant)
    eng = Engine(max_batch=1 << 12)
    s = LocalSentinel(eng, RES, ORIGINS, block_log=block_log)
    R = {
        # list order default, appA: FlowRuleComparator puts the appA rule first
        "flow_default": FlowRule(resource="flowres", count=0),
        "flow_appA": FlowRule(resource="flowres", count=0, limit_app="appA"),
        # list order cluster, appA: the cluster-mode rule sorts last (no token service: it falls back to its local
        # check and blocks); the appA rule never blocks
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
            out.append(("pass", None, None))
            return e
        except BlockException as x:
            assert str(x) == res and x.resource == res
            out.append((type(x).__name__, x.rule, x.rule_limit_app))
            return None

    enter("flowres", 10, origin="appA", batch_count=2)     # the appA rule: detail 0
    enter("flowres", 11, origin="appB")                    # the default rule: detail 1
    enter("flowres", 12, origin="appB", batch_count=3)     # again: one row, count 4
    enter("clres", 20, origin="appA")                      # the cluster-mode rule, sorted last: detail 1
    enter("paramres", 30, args=(7,))
    enter("paramres", 31, args=("bob",), batch_count=2)
    enter("paramres", 32, args=([1, 2],))
    enter("paramres", 33, args=(True,))
    e = enter("degres", 40)                                # passes; its failed exit opens the breaker
    e.trace_error()
    e.exit(T0 + 41)
    enter("degres", 42, origin="appB")
    enter("sysres", 50, entry_type="IN")                   # SystemRule qps 0 on inbound entries
    enter("authres", 60, origin="appB")                    # black-listed
    enter("authres", 61, origin="appA")                    # passes
    return eng, s, R, out


@pytest.fixture(scope="module")
def scenario():
    eng, s, R, out = _scenario(True)
    yield s, R, out
    eng.close()


def test_every_exception_class_raises_with_its_rule(scenario):
    s, R, out = scenario
    want = [("FlowException", R["flow_appA"], "appA"), ("FlowException", R["flow_default"], "default"),
            ("FlowException", R["flow_default"], "default"), ("FlowException", R["cl_cluster"], "default"),
            ("ParamFlowException", R["param"], "7"), ("ParamFlowException", R["param"], "bob"),
            ("ParamFlowException", R["param"], "[1, 2]"), ("ParamFlowException", R["param"], "true"),
            ("pass", None, None), ("DegradeException", R["degrade"], "default"),
            ("SystemBlockException", None, "qps"), ("AuthorityException", R["auth"], "appB"), ("pass", None, None)]
    assert [(a, c) for a, _, c in out] == [(a, c) for a, _, c in want]
    for k, ((_, got, _), (_, exp, _)) in enumerate(zip(out, want)):
        assert got is exp, (k, "the exception carries the loaded rule object itself")


def test_block_rule_index_follows_the_loaders_order(scenario):
    """sga_block_rule_index: positions in the array the loader was given ([flow_default, cl_cluster, flow_appA,
    cl_appA]), through the comparator's reorder -- a non-default limitApp first, a cluster-mode rule last."""
    s, R, _ = scenario
    from sentinel_amd import _lib
    import ctypes as C
    assert s.block_rule_index(1, "flowres", 0) == 2 and s.block_rule_index(1, "flowres", 1) == 0
    assert s.block_rule_index(1, "clres", 0) == 3 and s.block_rule_index(1, "clres", 1) == 1
    assert s.block_rule(1, "clres", 1) is R["cl_cluster"] and s.block_rule(1, "flowres", 0) is R["flow_appA"]
    assert s.block_rule_index(2, "paramres", 0) == 0 and s.block_rule_index(3, "degres", 0) == 0
    assert s.block_rule(2, "paramres", 0) is R["param"] and s.block_rule(3, "degres", 0) is R["degrade"]
    assert s.block_rule(6, "authres", 0) is R["auth"] and s.block_rule(5, "sysres", 0) is None
    idx = C.c_uint32()
    L = _lib.load()
    for dec, res, detail in [(5, 4, 0), (6, 5, 0), (0, 0, 0), (4, 0, 0), (1, 0, 2), (1, 2, 0), (2, 2, 1), (3, 3, 1),
                             (1, len(RES), 0)]:
        assert L.sga_block_rule_index(s.engine.handle, dec, res, detail, C.byref(idx)) == EINVAL, (dec, res, detail)


def test_the_log_file_of_every_exception_class(scenario, tmp_path):
    """The lines as StatLogController.StatLogWriteTask writes them, written out from the reference's format:
    time|1|resource,ExceptionSimpleName,ruleLimitApp,origin|count,0."""
    from sentinel_amd.block_log import BlockLogWriter
    s, _, _ = scenario
    w = BlockLogWriter(s, str(tmp_path), tz=UTC)
    assert w.poll(T0 + 999) == 0, "the second is not finished"
    assert w.poll(T0 + 1000) == 10
    assert w.close() == 0
    lines = open(tmp_path / "sentinel-block.log", "rb").read().decode().splitlines(keepends=True)
    want = [f"{bc.STAMP}|1|flowres,FlowException,appA,appA|2,0\n",
            f"{bc.STAMP}|1|flowres,FlowException,default,appB|4,0\n",
            f"{bc.STAMP}|1|clres,FlowException,default,appA|1,0\n",
            f"{bc.STAMP}|1|paramres,ParamFlowException,7,|1,0\n",
            f"{bc.STAMP}|1|paramres,ParamFlowException,bob,|2,0\n",
            f"{bc.STAMP}|1|paramres,ParamFlowException,[1, 2],|1,0\n",
            f"{bc.STAMP}|1|paramres,ParamFlowException,true,|1,0\n",
            f"{bc.STAMP}|1|degres,DegradeException,default,appB|1,0\n",
            f"{bc.STAMP}|1|sysres,SystemBlockException,qps,|1,0\n",
            f"{bc.STAMP}|1|authres,AuthorityException,appB,appB|1,0\n"]
    # the order inside a second is unpinned (the reference walks a ConcurrentHashMap): resources ascend here, the
    # parameter rows by tag
    assert sorted(lines) == sorted(want)
    assert [x.split("|")[2].split(",")[0] for x in lines] == ["flowres"] * 2 + ["clres"] + ["paramres"] * 4 + [
        "degres", "sysres", "authres"]


def test_the_log_has_no_side_effects(scenario):
    """A twin without the log, fed the same entries: the same outcomes and every node view of every table
    identical; its drain answers SGA_EINVAL."""
    from sentinel_amd import _lib
    s, _, out = scenario
    eng2, s2, _, out2 = _scenario(False)
    try:
        assert [(a, c) for a, _, c in out] == [(a, c) for a, _, c in out2]
        for now in (T0 + 100, T0 + 1500, T0 + 70_000):
            for table in (_lib.SGA_NODES_RESOURCE, _lib.SGA_NODES_ORIGIN, _lib.SGA_NODES_CONTEXT):
                ids = list(range(len(RES))) + [0xFFFFFFFF] if table == _lib.SGA_NODES_RESOURCE else None
                a, b = s.query_nodes(table, now, ids), s2.query_nodes(table, now, ids)
                assert len(a) == len(b) and a.tobytes() == b.tobytes(), (now, table)
        rc, n, _, _, _ = bc.drain_raw(s2, T0 + 10_000, 16)
        assert rc == EINVAL
    finally:
        eng2.close()


def test_parameter_tags_of_every_argument_form():
    """The tag is args[paramIdx] of the blocking rule through ev_arg: the legacy SGA_EV_HAS_PARAM scalar, the legacy
    SGA_EV_PARAM_LIST list and SGA_EV_ARGS vectors, a positive index and a negative one the first check resolved."""
    from sentinel_amd.block_log import list_tag
    from sentinel_amd.local import EV_ARGS, EV_HAS_PARAM, EV_PARAM_LIST, ParamFlowRuleManager, encode_args
    from sentinel_amd.rules import ParamFlowRule
    eng, s = _sentinel(2)
    try:
        ParamFlowRuleManager(s).load_rules([ParamFlowRule(resource="r0", param_idx=0, count=0),
                                            ParamFlowRule(resource="r1", param_idx=-1, count=0)])
        pvals = []
        legacy_off = len(pvals)
        pvals.extend([5, 6, 7])
        ev = [  # (resource, flags, param word, expected (tag_kind, tag) or None for a pass)
            (0, EV_HAS_PARAM, 42, (0, 42)),
            (0, EV_HAS_PARAM | EV_PARAM_LIST, (legacy_off << 32) | 3, (1, list_tag([5, 6, 7]))),
            (0, EV_ARGS, encode_args((9, [1, 2]), pvals), (0, 9)),
            (1, EV_ARGS, encode_args((9, [1, 2]), pvals), (1, list_tag([1, 2]))),   # -1 of two arguments: index 1
            (1, EV_ARGS, encode_args((3, 4), pvals), (0, 4)),
            (1, EV_ARGS, encode_args((3, 4, 8), pvals), (0, 4)),                    # the index stays 1 once resolved
            (0, 0, 0, None),                                                        # no argument: the rule passes
            (0, EV_ARGS, encode_args((None,), pvals), None),                        # a null argument passes
        ]
        n = len(ev)
        res = np.asarray([e[0] for e in ev], np.uint32)
        ts = T0 + np.arange(n, dtype=np.int64)
        acq = np.asarray([1, 3] * (n // 2), np.int32)
        d, w = s.submit(np.zeros(n, np.uint8), res, ts, acq, [e[1] for e in ev], None, [e[2] for e in ev], pvals)
        assert d.tolist() == [2 if e[3] else 0 for e in ev]
        tags = {i: e[3] for i, e in enumerate(ev) if e[3]}
        acc = bc.add_reference({}, np.zeros(n, np.uint8), res, ts, acq, d, w, tags=tags)
        assert len(acc) == 5  # events 4 and 5 share a tuple
        rows, le, lc = s.block_rows(None)
        assert (le, lc) == (0, 0)
        assert bc.as_tuples(rows) == bc.expected_tuples(acc)
    finally:
        eng.close()


# ------------------------------------------------------------------ 3: persistence and drain
def _blocks(n, res, t_lo, t_hi, seed):
    rng = np.random.default_rng(seed)
    ts = np.sort(rng.integers(t_lo, t_hi, n)).astype(np.int64)
    return {"kind": np.zeros(n, np.uint8), "resource": rng.choice(np.asarray(res, np.uint32), n).astype(np.uint32),
            "ts": ts, "acquire": rng.choice(np.asarray([1, 3], np.int32), n).astype(np.int32),
            "flags": np.zeros(n, np.uint8), "rt": np.zeros(n, np.int64), "param": np.zeros(n, np.uint64)}


def test_rows_persist_across_chunks_and_calls_and_drain_by_second():
    eng, s = _sentinel(4, block_log=64, max_batch=2048)
    try:
        _flow(s, [(0, 0.0), (1, 0.0)])
        A, B = T0, T0 + 1000
        acc = {}
        # one call of three chunks (2,048 + 2,048 + 904: two through the pipeline, one through k_lsmall), all in A
        st = _blocks(5000, [0], A, A + 1000, 1)
        _ref(acc, st, *_submit(s, st))
        # a second call: A and B, both resources
        st = _blocks(3000, [0, 1], A + 500, B + 600, 2)
        _ref(acc, st, *_submit(s, st))
        assert len(acc) == 4 and sum(v[1] for v in acc.values()) == 8000
        # cap too small: SGA_ERANGE, the number needed, nothing removed
        rc, n, _, _, _ = bc.drain_raw(s, B + 500, 1)
        assert (rc, n) == (ERANGE, 2)
        # before_ms inside B: only A
        rc, n, rows, le, lc = bc.drain_raw(s, B + 500, 64)
        assert (rc, n, le, lc) == (0, 2, 0, 0)
        assert bc.as_tuples(rows) == bc.expected_tuples(acc, hi=B)
        for k in [k for k in acc if k[0] == A]:
            del acc[k]
        # further events of B's keys land in B's rows, which the drain moved to the other table
        st = _blocks(1500, [0, 1], B + 600, B + 1000, 3)
        _ref(acc, st, *_submit(s, st))
        # a late event for A: a fresh row
        st = _blocks(3, [1], A + 900, A + 901, 4)
        _ref(acc, st, *_submit(s, st))
        assert len(acc) == 3
        rc, n, _, _, _ = bc.drain_raw(s, B + 999, 64)
        assert (rc, n) == (0, 1), "B is not finished at B + 999; the late A row is"
        rows, le, lc = s.block_rows(None)
        assert (le, lc) == (0, 0)
        assert bc.as_tuples(rows) == bc.expected_tuples(acc, lo=B)
        assert len(s.block_rows(None)[0]) == 0
    finally:
        eng.close()


def test_enable_again_needs_an_empty_log():
    from sentinel_amd import _lib
    eng, s = _sentinel(2, block_log=64)
    try:
        _flow(s, [(0, 0.0)])
        L = _lib.load()
        assert L.sga_block_log_enable(eng.handle, 128) == 0, "an empty log may be resized"
        st = _blocks(10, [0], T0, T0 + 10, 5)
        _submit(s, st)
        assert L.sga_block_log_enable(eng.handle, 256) == EINVAL, "rows pending"
        assert len(s.block_rows(None)[0]) == 1
        assert L.sga_block_log_enable(eng.handle, 64) == 0
    finally:
        eng.close()


# ------------------------------------------------------------------ 4: overflow
def test_overflow_goes_to_the_lost_counters():
    """Capacity 64, 200 distinct keys in one chunk.  Conservation is a condition, not a tolerance: what the rows do
    not hold, the lost counters do."""
    eng, s = _sentinel(200, block_log=64)
    try:
        _flow(s, [(r, 0.0) for r in range(200)])
        n = 600
        st = _blocks(n, list(range(200)), T0, T0 + 1000, 6)
        st["resource"] = (np.arange(n) % 200).astype(np.uint32)  # every key three times
        d, w = _submit(s, st)
        assert (d == 1).all()
        acc = _ref({}, st, d, w)
        assert len(acc) == 200
        rows, lost_events, lost_count = s.block_rows(None)
        assert 0 < len(rows) <= 64 and lost_events > 0
        got = bc.as_tuples(rows)
        assert len({g[:7] for g in got}) == len(got), "no key twice"
        for g in got:
            assert g[:7] in acc, "a row of no true key"
            assert 0 < g[7] <= acc[g[:7]][0] and 0 < g[8] <= acc[g[:7]][1]
        assert sum(g[7] for g in got) + lost_count == int(st["acquire"].sum())
        assert sum(g[8] for g in got) + lost_events == n
        rows, lost_events, lost_count = s.block_rows(None)
        assert (len(rows), lost_events, lost_count) == (0, 0, 0), "the drain cleared the counters"
    finally:
        eng.close()


# ------------------------------------------------------------------ 5: device entry
def _device(s, st):
    import torch
    dev = torch.device("cuda", 0)
    base = int(st["ts"].min())
    off = (st["ts"] - base).astype(np.uint32).view(np.int32)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    d, w = s.submit_device(t(st["kind"], np.uint8), t(st["resource"], np.int32), base, t(off, np.int32),
                           t(st["acquire"], np.int32), flags=t(st["flags"], np.uint8), rt=t(st["rt"], np.int64),
                           param=t(st["param"], np.int64))
    return d, w


def test_device_entry_logs_what_the_host_entry_logs():
    from sentinel_amd._lib import EngineError
    n = 4097
    engs = []
    try:
        got = []
        for dev in (False, True):
            eng, s = _sentinel(bc.R_FIRST + n)
            engs.append(eng)
            _flow(s, bc.seam_rules(n))
            st = bc.seam_stream(n, "distinct")
            st["resource"][::16] = bc.R_HOT  # some keys shared, most of their own
            if dev:
                d, w = _device(s, st)
                s.device_status()
                d, w = d.cpu().numpy(), w.cpu().numpy()
            else:
                d, w = _submit(s, st)
            acc = _ref({}, st, d, w)
            rows, le, lc = s.block_rows(None)
            assert (le, lc) == (0, 0)
            assert bc.as_tuples(rows) == bc.expected_tuples(acc), "device" if dev else "host"
            got.append(rows.tobytes())
        assert got[0] == got[1]
        # (s: the device sentinel)  a chunk the gate refuses answers -1 for every event and logs nothing; the sticky status still reports it.
        # (An unknown resource id alone refuses nothing on either entry -- such an event has no node and no rules
        # and passes -- so the chunk carries one and is refused for a negative acquire.)
        st = bc.seam_stream(300, "one")
        st["resource"][8] = bc.R_FIRST + n + 5
        st["acquire"][11] = -1
        d, w = _device(s, st)
        with pytest.raises(EngineError, match="rc=-22"):
            s.device_status()
        assert (d.cpu().numpy() == -1).all()
        rows, le, lc = s.block_rows(None)
        assert len(rows) == 0 and (le, lc) == (0, 0)
        # the unknown resource id on its own: passes, is not logged, and the rest of the chunk is
        st["acquire"][11] = 1
        st["ts"] = st["ts"] + 5000
        d, w = _device(s, st)
        s.device_status()
        d, w = d.cpu().numpy(), w.cpu().numpy()
        assert st["kind"][8] == 0 and d[8] == 0
        rows, _, _ = s.block_rows(None)
        assert len(rows) and bc.as_tuples(rows) == bc.expected_tuples(_ref({}, st, d, w))
    finally:
        for e in engs:
            e.close()
