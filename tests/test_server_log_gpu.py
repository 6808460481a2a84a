"""Token server log on the GPU: ClusterServerStatLogUtil's per-second sums formed by k_slog_add behind every token
batch (sga_server_log_enable / sga_server_log_drain).

Expected rows never come from the engine: tests/server_log_cases.reduce_rows forms them from the C oracle's statuses
for the same trace, and every test also asserts that the engine's results equal the oracle's.  count and events
are integer sums: rows are compared exactly, there is no tolerance anywhere in this file."""
import ctypes as C
import datetime
import itertools
import os

import numpy as np
import pytest

from tests import server_log_cases as sc
from tests.server_log_cases import (FLOW_BLOCK, FLOW_BLOCK_PRIO, FLOW_PASS, FLOW_WAITING, PARAM_BLOCK, PARAM_PASS, T0,
                                    Oracle, as_tuples, expected_tuples, reduce_rows, same_results)

pytestmark = pytest.mark.gpu

ERANGE, EINVAL = -34, -22
INT64_MAX = (1 << 63) - 1


def _engine(rules=(), log=0, ns="default", limit=None, **kw):
    """An engine with `rules` (dicts as the oracle takes them); log: None = off, else max_rows."""
    from sentinel_amd import _lib, cluster
    kw.setdefault("max_batch", 1 << 14)
    eng = cluster.Engine(**kw)
    if rules:
        a = np.zeros(len(rules), dtype=cluster.CLUSTER_RULE_DTYPE)
        for i, r in enumerate(rules):
            a[i] = (r["flow_id"], r["count"], r.get("threshold_type", 0), r.get("sample_count", 10),
                    r.get("window_interval_ms", 1000), 1, 0, 0, 2000, 2000)
        rc = _lib.load().sga_load_cluster_flow_rules(eng.handle, ns.encode(),
                                                     a.ctypes.data_as(C.POINTER(_lib.SgaClusterFlowRule)), len(rules))
        assert rc == len(rules)
    if limit is not None:
        cluster.GlobalRequestLimiter(eng).init_if_absent(ns, float(limit))
    if log is not None:
        eng.server_log_enable(log)
    return eng


def _svc(eng):
    from sentinel_amd import cluster
    return cluster.DefaultTokenService(eng)


def _raw_drain(eng, before, cap):
    """sga_server_log_drain as the C caller sees it: (rc, n, rows, lost_events, lost_count)."""
    from sentinel_amd import _lib
    from sentinel_amd.server_log import SERVER_LOG_ROW_DTYPE
    out = np.zeros(max(cap, 1), dtype=SERVER_LOG_ROW_DTYPE)
    n, le, lc = C.c_size_t(), C.c_uint64(77), C.c_int64(77)
    rc = _lib.load().sga_server_log_drain(eng.handle, before, out.ctypes.data, cap, C.byref(n), C.byref(le), C.byref(lc))
    return rc, int(n.value), out, int(le.value), int(lc.value)


# ------------------------------------------------------------------ off by default
def test_off_by_default_and_log_changes_no_result():
    from sentinel_amd import _lib
    rules, trace = sc.path_rules(), sc.path_trace()
    off, on = _engine(rules, log=None), _engine(rules)
    rc, n, _, _, _ = _raw_drain(off, INT64_MAX, 16)
    assert rc == EINVAL, "an engine without the log"
    assert _lib.load().sga_server_log_drain(off.handle, INT64_MAX, None, 0, None, None, None) == EINVAL
    orc = Oracle(rules)
    for k, (f, a, p, t) in enumerate(trace):
        ref = orc.replay(f, a, p, t)
        g_off, g_on = _svc(off).request_tokens(f, a, p, t), _svc(on).request_tokens(f, a, p, t)
        assert g_off.tobytes() == g_on.tobytes(), k
        same_results(g_on, ref, k)
    assert _raw_drain(off, INT64_MAX, 16)[0] == EINVAL
    rows, le, lc = on.server_log_rows()
    assert len(rows) > 0 and (le, lc) == (0, 0)
    orc.close()
    off.close()
    on.close()


# ------------------------------------------------------------------ known answers
def test_kat_count_differs_from_events():
    """One GLOBAL rule of count 5, eight requests of acquire 2 in one millisecond: two pass, six are blocked."""
    rules = [{"flow_id": 9, "count": 5.0, "threshold_type": 1}]
    eng, orc = _engine(rules), Oracle(rules)
    f, a, p, t = np.full(8, 9), np.full(8, 2), np.zeros(8, np.uint8), np.full(8, T0 + 17)
    ref = orc.replay(f, a, p, t)
    same_results(_svc(eng).request_tokens(f, a, p, t), ref)
    assert ref[:, 0].tolist() == [0, 0, 1, 1, 1, 1, 1, 1]
    rows, le, lc = eng.server_log_rows()
    want = expected_tuples(reduce_rows({}, f, a, p, t, ref[:, 0]))
    assert want == [(T0, 9, FLOW_BLOCK, 0, 12, 6)] and as_tuples(rows) == want and (le, lc) == (0, 0)
    orc.close()
    eng.close()


def test_kat_occupy_waiting_and_prioritized_block():
    """ClusterFlowCheckerTest.testAcquireClusterTokenOccupyPass's requests (tests/golden/kat_ClusterFlowCheckerTest_
    testAcquireClusterTokenOccupyPass...) as one batch: a prioritized request occupies the next bucket (WAITING), a
    prioritized one is blocked (BLOCK_PRIO), plain ones are blocked (BLOCK)."""
    rules = [{"flow_id": 98765, "count": 5.0, "threshold_type": 1, "sample_count": 5, "window_interval_ms": 1000}]
    eng, orc = _engine(rules), Oracle(rules)
    steps = [(0, 0), (0, 0), (200, 0), (400, 1), (400, 0), (400, 1), (600, 0), (600, 0), (800, 0), (800, 1), (800, 0),
             (1000, 0)]
    t = np.array([T0 + s for s, _ in steps])
    p = np.array([q for _, q in steps], np.uint8)
    f, a = np.full(len(steps), 98765), np.ones(len(steps), np.int32)
    ref = orc.replay(f, a, p, t)
    assert ref[:, 0].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 1, 0] and ref[9, 2] == 200
    same_results(_svc(eng).request_tokens(f, a, p, t), ref)
    want = expected_tuples(reduce_rows({}, f, a, p, t, ref[:, 0]))
    assert want == [(T0, 98765, FLOW_BLOCK, 0, 4, 4), (T0, 98765, FLOW_BLOCK_PRIO, 0, 1, 1),
                    (T0, 98765, FLOW_WAITING, 0, 1, 1)]
    assert as_tuples(eng.server_log_rows()[0]) == want
    orc.close()
    eng.close()


# ------------------------------------------------------------------ wave and tile seams
_seam_case = itertools.count(1)


@pytest.fixture(scope="module")
def seam_pair():
    """One engine and one oracle for every seam case: each case drains everything it logged."""
    eng, orc = _engine(sc.seam_rules()), Oracle(sc.seam_rules())
    yield eng, orc
    orc.close()
    eng.close()


@pytest.mark.parametrize("pattern", sc.SEAM_PATTERNS)
@pytest.mark.parametrize("n", sc.SEAM_SIZES)
def test_seams(seam_pair, n, pattern):
    """Sizes around the wave (64), the block (256) and the pass's four tiles (1,024), five patterns
    (server_log_cases.seam_trace): the held tuple, a tuple per lane, two tuples in turn, a held tuple displaced in
    a later tile, a second boundary inside the wave with times going backwards."""
    eng, orc = seam_pair
    f, a, p, t = sc.seam_trace(n, pattern, T0 + 10_000 * next(_seam_case))
    ref = orc.replay(f, a, p, t)
    same_results(_svc(eng).request_tokens(f, a, p, t), ref, (n, pattern))
    acc = reduce_rows({}, f, a, p, t, ref[:, 0])
    assert (ref[f != 100, 0] == 1).all() and (ref[f == 100, 0] == 0).all()
    rows, le, lc = eng.server_log_rows()
    assert (le, lc) == (0, 0)
    assert as_tuples(rows) == expected_tuples(acc)
    assert sum(v[1] for v in acc.values()) == int((f != 100).sum())
    if pattern == "distinct":
        assert len(acc) == min(n, 64)
    if pattern == "second" and n >= 64:
        assert len({k[0] for k in acc}) >= 2, "the blocks straddle a second"
    if n >= 5:
        assert any(v[0] != v[1] for v in acc.values()), "count differs from events"
    assert len(eng.server_log_rows()[0]) == 0, "a drained log is empty"


# ------------------------------------------------------------------ paths and entries
@pytest.fixture(scope="module")
def path_expect():
    """The path trace's oracle results and rows, computed once."""
    orc = Oracle(sc.path_rules())
    acc, refs = {}, []
    for f, a, p, t in sc.path_trace():
        ref = orc.replay(f, a, p, t)
        refs.append(ref)
        reduce_rows(acc, f, a, p, t, ref[:, 0])
    orc.close()
    kinds = {k[2] for k in acc}
    assert {FLOW_BLOCK, FLOW_BLOCK_PRIO} <= kinds and any(v[0] != v[1] for v in acc.values())
    return refs, expected_tuples(acc)


# hot_min_requests = 64: rules 1..6 (about 160 requests a batch, acquire 1) become hot, the others (about 12) stay cold
_PATHS = {"hot": dict(hot_rules=True, hot_min_requests=64, small_batch=0),
          "sort": dict(hot_rules=False, small_batch=0), "small": dict(hot_rules=False, small_batch=4096)}


def _decode(o):
    from sentinel_amd.cluster import TOKEN_DTYPE
    return np.ascontiguousarray(o).view(TOKEN_DTYPE)


def _run_entry(eng, entry, f, a, p, t):
    """One batch through one entry; returns TOKEN_DTYPE results."""
    import torch
    from sentinel_amd import _lib
    from sentinel_amd.cluster import TOKEN_DTYPE
    L = _lib.load()
    n = len(f)
    if entry == "host":
        return _svc(eng).request_tokens(f, a, p, t)
    if entry == "queue":
        svc = _svc(eng)
        tickets = [svc.submit(int(f[i]), int(a[i]), bool(p[i]), int(t[i])) for i in range(n)]
        out = np.zeros(n, dtype=TOKEN_DTYPE)
        for i, tk in enumerate(tickets):
            r = svc.poll(tk)
            assert r is not None
            out[i] = (r.remaining, r.wait_in_ms, r.status, 0)
        return out
    dev = torch.device("cuda", 0)
    base = int(t.min())
    o = torch.zeros(n, dtype=torch.int64, device=dev)
    packed = None
    if entry == "packed":
        rec = np.zeros((n, 3), dtype=np.uint32)
        rec[:, 0] = f.astype(np.uint32)
        rec[:, 1] = (t - base).astype(np.uint32)
        rec[:, 2] = a.astype(np.uint32) | (p.astype(np.uint32) << 16)
        packed = torch.from_numpy(rec.view(np.int32)).to(dev)
    else:
        d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (f, a, p, (t - base).astype(np.int32))]
    torch.cuda.synchronize()  # the inputs and the zeroed output are there before the engine's stream reads them
    if packed is not None:
        rc = L.sga_request_tokens_packed_device(eng.handle, packed.data_ptr(), base, n, o.data_ptr(), None)
    else:
        fn = {"device": L.sga_request_tokens_device, "async": L.sga_request_tokens_device_async,
              "pipelined": L.sga_request_tokens_device_pipelined}[entry]
        stream = torch.cuda.Stream(device=dev) if entry == "pipelined" else None
        rc = fn(eng.handle, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), base, d[3].data_ptr(), n, o.data_ptr(),
                stream.cuda_stream if stream is not None else None)
        if stream is not None:
            assert L.sga_stream_wait(eng.handle, stream.cuda_stream) == 0
    assert rc == 0, L.sga_last_error(eng.handle)
    assert L.sga_sync(eng.handle) == 0
    torch.cuda.synchronize()
    return _decode(o.cpu().numpy())


@pytest.mark.parametrize("entry", ["host", "device", "packed", "async", "pipelined", "queue"])
@pytest.mark.parametrize("path", ["hot", "sort", "small"])
def test_paths_and_entries(path_expect, path, entry):
    """The same three batches give the oracle's results and the same rows through every entry on every path;
    sga_cluster_batch_info confirms the hot path ran (or did not)."""
    refs, want = path_expect
    eng = _engine(sc.path_rules(), **_PATHS[path])
    for k, (f, a, p, t) in enumerate(sc.path_trace()):
        same_results(_run_entry(eng, entry, f, a, p, t), refs[k], (path, entry, k))
    info = eng.batch_info()
    assert info["hot_mode"] == (1 if path == "hot" else 0), info
    if path == "hot":
        assert info["flags"] == 0 and info["n_hot_next"] >= 1, info  # the hot rules share one window length
    rows, le, lc = eng.server_log_rows()
    assert (le, lc) == (0, 0)
    assert as_tuples(rows) == want
    eng.close()


# ------------------------------------------------------------------ random trace
def test_random_trace_with_limiter():
    """About 50 rules of mixed geometry, 20,000 requests over three seconds in four batches, mixed prioritized, a
    namespace limiter (TOO_MANY_REQUEST), unknown flowIds and bad requests: rows are exactly the reduce."""
    rng = np.random.default_rng(11)
    rules = [{"flow_id": f, "count": float(rng.integers(0, 60)), "threshold_type": 1,
              "sample_count": int(rng.choice([1, 2, 5, 10])), "window_interval_ms": int(rng.choice([1000, 2000]))}
             for f in range(1, 51)]
    eng, orc = _engine(rules, limit=5000.0, max_batch=1 << 15), Oracle(rules, limit=5000.0)
    n = 20_000
    fid = rng.integers(1, 51, size=n).astype(np.int64)
    fid[rng.random(n) < 0.01] = 0
    fid[rng.random(n) < 0.01] = 4242
    acq = np.where(rng.random(n) < 0.8, 1, rng.integers(0, 5, size=n)).astype(np.int32)  # 0: BAD_REQUEST
    prio = (rng.random(n) < 0.3).astype(np.uint8)
    ts = (T0 + np.sort(rng.integers(0, 3000, size=n))).astype(np.int64)
    acc, seen = {}, set()
    for lo in range(0, n, 5000):
        s = slice(lo, lo + 5000)
        ref = orc.replay(fid[s], acq[s], prio[s], ts[s])
        same_results(_svc(eng).request_tokens(fid[s], acq[s], prio[s], ts[s]), ref, lo)
        reduce_rows(acc, fid[s], acq[s], prio[s], ts[s], ref[:, 0])
        seen |= set(ref[:, 0].tolist())
    assert {-4, -2, 0, 1, 2, 3} <= seen, seen
    assert {k[2] for k in acc} == {FLOW_BLOCK, FLOW_BLOCK_PRIO, FLOW_WAITING} and len({k[0] for k in acc}) == 3
    rows, le, lc = eng.server_log_rows()
    assert (le, lc) == (0, 0)
    assert as_tuples(rows) == expected_tuples(acc)
    orc.close()
    eng.close()


# ------------------------------------------------------------------ accumulation and drain
def test_accumulation_and_drain():
    from sentinel_amd import _lib
    rules = [{"flow_id": f, "count": 0.0, "threshold_type": 1} for f in (1, 2, 3)]
    eng, orc = _engine(rules), Oracle(rules)
    svc = _svc(eng)

    def batch(fids, t, acq=2):
        f, a = np.array(fids), np.full(len(fids), acq)
        p, ts = np.zeros(len(fids), np.uint8), np.full(len(fids), t)
        ref = orc.replay(f, a, p, ts)
        same_results(svc.request_tokens(f, a, p, ts), ref)
        return reduce_rows({}, f, a, p, ts, ref[:, 0])

    acc = {}
    for fids, t in (([1, 1, 2], T0 + 1), ([1, 3], T0 + 500), ([2, 2, 2], T0 + 1200)):  # several batches, one drain
        for k, v in batch(fids, t).items():
            acc[k] = [acc.get(k, [0, 0])[0] + v[0], acc.get(k, [0, 0])[1] + v[1]]
    want = expected_tuples(acc)
    assert eng.server_log_rows(T0 + 999)[0].size == 0, "no second is finished at T0 + 999"
    # SGA_ERANGE: *n = the number needed, nothing removed
    rc, n, _, _, _ = _raw_drain(eng, T0 + 1000, 1)
    assert (rc, n) == (ERANGE, 3)
    assert _lib.load().sga_server_log_enable(eng.handle, 128) == EINVAL, "rows pending"
    rows, le, lc = eng.server_log_rows(T0 + 1999)  # before_ms leaves the running second
    assert as_tuples(rows) == [r for r in want if r[0] == T0] and (le, lc) == (0, 0)
    late = batch([1], T0 + 700)  # a drained second that gets more events: new rows
    rows2, _, _ = eng.server_log_rows(T0 + 2000)
    assert as_tuples(rows2) == sorted(expected_tuples(late) + [r for r in want if r[0] == T0 + 1000])
    assert eng.server_log_rows()[0].size == 0
    assert _lib.load().sga_server_log_enable(eng.handle, 128) == 0, "an empty log may be resized"
    orc.close()
    eng.close()


# ------------------------------------------------------------------ overflow
def test_overflow_lost_counters():
    """max_rows = 64 and 300 distinct count-0 rules in one second: a key that has a slot never loses an update, the
    keys without one are counted in the lost counters."""
    rules = [{"flow_id": f, "count": 0.0, "threshold_type": 1} for f in range(1, 301)]
    eng, orc = _engine(rules, log=64), Oracle(rules)
    rng = np.random.default_rng(3)
    acc = {}
    for b in range(3):
        f = np.concatenate([np.arange(1, 301), rng.integers(1, 301, size=900)]).astype(np.int64)
        a = rng.integers(1, 4, size=len(f)).astype(np.int32)
        p, t = np.zeros(len(f), np.uint8), np.full(len(f), T0 + 10 + b)
        ref = orc.replay(f, a, p, t)
        same_results(_svc(eng).request_tokens(f, a, p, t), ref, b)
        reduce_rows(acc, f, a, p, t, ref[:, 0])
    assert len(acc) == 300
    rc, n, _, le0, lc0 = _raw_drain(eng, INT64_MAX, 8)
    assert rc == ERANGE and 8 < n <= 64 and (le0, lc0) == (77, 77), "SGA_ERANGE does not touch the lost counters"
    rows, le, lc = eng.server_log_rows()
    got = as_tuples(rows)
    assert len(got) == n
    want = {r[:4]: r for r in expected_tuples(acc)}
    for r in got:
        assert want[r[:4]] == r, "a returned row equals the expected row of its key exactly"
    missing = [want[k] for k in want if k not in {r[:4] for r in got}]
    assert len(missing) == 300 - n and le == sum(r[5] for r in missing) and lc == sum(r[4] for r in missing)
    rows, le, lc = eng.server_log_rows()
    assert len(rows) == 0 and (le, lc) == (0, 0), "a second drain returns zero lost"
    orc.close()
    eng.close()


# ------------------------------------------------------------------ RLS
def test_rls_both_entries():
    """SimpleClusterFlowChecker logs passes and blocks, knows no priority and no waiting; descriptors without a rule
    and requests with a negative hits_addend form nothing.  Batch 0 through the host entry, batch 1 the device's."""
    import torch
    from sentinel_amd import cluster
    rules = [{"flow_id": 1000 + f, "count": float(3 + f), "threshold_type": 1, "sample_count": 1} for f in range(8)]
    eng, orc = _engine(rules), Oracle(rules)
    svc = cluster.EnvoyRlsService(eng)
    rng = np.random.default_rng(19)
    dev = torch.device("cuda", 0)
    acc = {}
    for b in range(2):
        nreq = 300
        ndesc = rng.integers(1, 4, size=nreq)
        off = np.concatenate([[0], np.cumsum(ndesc)]).astype(np.uint32)
        dfid = (1000 + rng.integers(0, 8, size=int(off[-1]))).astype(np.int64)
        dfid[rng.random(len(dfid)) < 0.05] = 42  # no rule
        hits = rng.integers(0, 4, size=nreq).astype(np.int32)
        hits[rng.random(nreq) < 0.03] = -1
        ts = (T0 + 1500 * b + np.sort(rng.integers(0, 1500, size=nreq))).astype(np.int64)
        if b == 0:
            code, st = svc.should_rate_limit(off, dfid, hits, ts)
        else:
            base = int(ts.min())
            T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
            code, st, _ = svc.should_rate_limit_device(T(off.view(np.int32)), T(dfid), T(hits), base,
                                                       T((ts - base).astype(np.uint32).view(np.int32)))
            torch.cuda.synchronize()
            st = st.cpu().numpy()
        sel = np.nonzero(np.repeat(hits >= 0, ndesc))[0]
        f_s = dfid[sel]
        a_s = np.repeat(np.where(hits <= 0, 1, hits), ndesc)[sel]
        t_s = np.repeat(ts, ndesc)[sel]
        ref = orc.simple(f_s, a_s, t_s)
        want_st = np.full(len(dfid), 3)
        want_st[sel] = ref[:, 0]
        assert np.array_equal(np.asarray(st).astype(np.int64), want_st), b
        reduce_rows(acc, f_s, a_s, None, t_s, ref[:, 0], checker="simple")
    assert {k[2] for k in acc} == {FLOW_BLOCK, FLOW_PASS} and all(k[1] != 42 for k in acc)
    assert any(v[0] != v[1] for v in acc.values())
    rows, le, lc = eng.server_log_rows()
    assert (le, lc) == (0, 0)
    assert as_tuples(rows) == expected_tuples(acc)
    orc.close()
    eng.close()


# ------------------------------------------------------------------ parameters
# closed form: single values in ascending time, the default capacity.  50 and 51 always block, 60 after two passes
PARAM_RULE_FAST = {"flow_id": 1, "count": 1000.0, "threshold_type": 1, "hot": {50: 0, 51: 0, 60: 2}}
# sequential: its bucket maps hold 3 values (its namespace is loaded under sga_cluster_set_param_capacity(3)), the
# trace sends more, so it runs in LRU mode; it also gets the collections
PARAM_RULE_SLOW = {"flow_id": 2, "count": 1000.0, "threshold_type": 1, "hot": {50: 0, 51: 0}}


def _param_pair():
    from sentinel_amd import cluster
    from tests.test_cluster_param_gpu import to_param_rules
    eng = _engine(max_param_keys=1 << 12)
    mgr = cluster.ClusterParamFlowRuleManager(eng)
    orc = Oracle()
    L = orc.L

    def load(ns, rule):
        mgr.load_rules(ns, to_param_rules(cluster, [rule]))
        assert L.orc_cluster_load_param_rules(orc.h, ns.encode(), sc.H.cluster_param_rules_array([rule], orc.keep), 1) == 1

    load("fast", PARAM_RULE_FAST)
    mgr.set_param_capacity(3)
    L.orc_cluster_set_param_capacity(3)
    try:
        load("slow", PARAM_RULE_SLOW)
    finally:
        L.orc_cluster_set_param_capacity(0)
        mgr.set_param_capacity(0)
    return eng, orc


def _can_block(f, v):
    return v in (50, 51, 60)


def test_param_rows_both_paths():
    eng, orc = _param_pair()
    svc = _svc(eng)
    acc = {}

    def run(fid, values, ts, what):
        acq = np.ones(len(fid), np.int32)
        ref = orc.param(fid, acq, values, ts)
        got = svc.request_param_tokens(fid, acq, values, ts)
        bad = np.nonzero((got["status"] != ref[:, 0]) | (got["remaining"] != ref[:, 1]))[0]
        assert bad.size == 0, (what, bad[:5], got[bad[:5]], ref[bad[:5]])
        reduce_rows(acc, fid, acq, None, ts, ref[:, 0], checker="param", values=values, can_block=_can_block)
        return ref[:, 0]

    # batch 1, rule 1 on the closed form (single values, ascending time, capacity never passed: 3 distinct keys a
    # bucket at most); rule 2 passes its capacity with values 1..8 and is sequential from then on
    v1 = [1, 50, 60, 60, 60, 60, 2, 51, 50]
    fid = np.array([1] * len(v1) + [2] * 10)
    values = [[v] for v in v1] + [[v] for v in (1, 2, 3, 4, 5, 6, 7, 8, 50, 51)]
    st = run(fid, values, T0 + 10 + np.arange(len(fid)), "single values")
    assert st[:len(v1)].tolist() == [0, 1, 0, 0, 1, 1, 0, 1, 1]
    # batch 2, collections (the sequential path): [ok, A, B] with A and B both blocking -> the tag is A; a
    # multi-value pass; an empty list forms nothing (BAD_REQUEST); a single blocking value on the LRU rule
    fid = np.array([2, 2, 2, 2, 1, 1, 2])
    values = [[1, 50, 51], [1, 51, 50], [1, 2], [], [3, 51, 50], [4, 5, 6], [51]]
    st = run(fid, values, T0 + 1100 + np.arange(len(fid)), "collections")
    assert st.tolist() == [1, 1, 0, -4, 1, 0, 1]
    want = expected_tuples(acc)
    assert (T0 + 1000, 2, PARAM_BLOCK, 50, 1, 1) in want and (T0 + 1000, 2, PARAM_BLOCK, 51, 2, 2) in want
    assert (T0 + 1000, 1, PARAM_BLOCK, 51, 1, 1) in want and (T0, 1, PARAM_BLOCK, 60, 2, 2) in want
    assert (T0 + 1000, 2, PARAM_PASS, 0, 1, 1) in want
    rows, le, lc = eng.server_log_rows()
    assert (le, lc) == (0, 0)
    assert as_tuples(rows) == want
    orc.close()
    eng.close()


# ------------------------------------------------------------------ end to end
def _lines(acc, text, stamp):
    """The file's lines from the reduce, restating the fixed order of server_log.ServerLogWriter."""
    out = []
    for slot, fid in sorted({(k[0], k[1]) for k in acc}):
        g = {k[2:]: v for k, v in acc.items() if k[:2] == (slot, fid)}
        b, pb = g.get((FLOW_BLOCK, 0), [0, 0]), g.get((FLOW_BLOCK_PRIO, 0), [0, 0])
        s = stamp(slot)
        if b[1] or pb[1]:
            out += [f"{s}|1|flow|block|{fid}|{b[0] + pb[0]},0", f"{s}|1|flow|block_request|{fid}|{b[1] + pb[1]},0"]
            if pb[1]:
                out.append(f"{s}|1|flow|occupied_block|{fid}|{pb[1]},0")
        if (FLOW_WAITING, 0) in g:
            out.append(f"{s}|1|flow|waiting|{fid}|{g[(FLOW_WAITING, 0)][0]},0")
        if (FLOW_PASS, 0) in g:
            out += [f"{s}|1|flow|pass|{fid}|{g[(FLOW_PASS, 0)][0]},0",
                    f"{s}|1|flow|pass_request|{fid}|{g[(FLOW_PASS, 0)][1]},0"]
        if (PARAM_PASS, 0) in g:
            out.append(f"{s}|1|param|pass|{fid}|{g[(PARAM_PASS, 0)][0]},0")
        for (kind, tag), v in sorted(g.items()):
            if kind == PARAM_BLOCK:
                out.append(f"{s}|1|param|block|{fid}|{text(tag)}|{v[0]},0")
    return out


def test_end_to_end_file(tmp_path):
    """Engine -> ServerLogWriter.poll -> file bytes == the lines built from the oracle's statuses: flow blocks with
    prioritized requests, and a parameter rule whose blocking value is a string the token service recorded."""
    from sentinel_amd import cluster
    from sentinel_amd.server_log import ServerLogWriter
    alice = cluster.param_value_key("alice")
    frules = [{"flow_id": 7, "count": 3.0, "threshold_type": 1, "sample_count": 5}]
    prules = [{"flow_id": 20, "count": 100.0, "threshold_type": 1, "hot": {alice: 0, 50: 0}}]
    eng, orc = _engine(frules), Oracle(frules, prules)
    items = [cluster.ParamFlowItem(object="alice", count=0, class_type="java.lang.String"),
             cluster.ParamFlowItem(object=50, count=0, class_type="long")]
    cluster.ClusterParamFlowRuleManager(eng).load_rules("default", [cluster.ParamFlowRule(
        resource="p20", count=100.0, cluster_mode=True, param_flow_item_list=items,
        cluster_config=cluster.ParamFlowClusterConfig(flow_id=20, threshold_type=1))])
    w = ServerLogWriter(eng, str(tmp_path), tz=datetime.timezone.utc)
    svc = _svc(eng)
    acc = {}
    n = 40
    f, a = np.full(n, 7), np.where(np.arange(n) % 3 == 0, 2, 1).astype(np.int32)
    p, t = (np.arange(n) % 4 == 1).astype(np.uint8), T0 + np.arange(n) * 45
    ref = orc.replay(f, a, p, t)
    same_results(svc.request_tokens(f, a, p, t), ref)
    reduce_rows(acc, f, a, p, t, ref[:, 0])
    params = [["bob"], ["alice"], ["bob", "alice"], [50], ["carol"]]
    keys = [[cluster.param_value_key(v) for v in q] for q in params]
    pf, pa, pt = np.full(5, 20), np.ones(5, np.int32), T0 + 300 + np.arange(5)
    pref = orc.param(pf, pa, keys, pt)
    got = svc.request_param_tokens(pf, pa, params, pt)
    assert got["status"].tolist() == pref[:, 0].tolist() == [0, 1, 1, 1, 0]
    reduce_rows(acc, pf, pa, None, pt, pref[:, 0], checker="param", values=keys,
                can_block=lambda fl, v: v in (alice, 50))
    assert w.poll(T0 + 1000) > 0  # the first second only
    stamp = lambda slot: datetime.datetime.fromtimestamp(slot // 1000, datetime.timezone.utc).strftime(  # noqa: E731
        "%Y-%m-%d %H:%M:%S")
    text = lambda tag: "alice" if tag == alice & sc.M64 else str(tag)  # noqa: E731
    first = {k: v for k, v in acc.items() if k[0] == T0}
    with open(os.path.join(str(tmp_path), "sentinel-server.log"), "rb") as fh:
        assert fh.read() == ("\n".join(_lines(first, text, stamp)) + "\n").encode()
    w.close()
    with open(os.path.join(str(tmp_path), "sentinel-server.log"), "rb") as fh:
        lines = fh.read().decode().splitlines()
    assert lines == _lines(first, text, stamp) + _lines({k: v for k, v in acc.items() if k[0] != T0}, text, stamp)
    assert any("|param|block|20|alice|2,0" in x for x in lines) and any("|flow|block|7|" in x for x in lines)
    orc.close()
    eng.close()
