"""The front of a hot-path cluster batch: the precheck and the batch totals run inside
the key passes (no launch of their own: pass 0 adds each segment's counts to striped totals, pass 1's first
wave sums them; on a fallback batch the last workgroup of pass 1 to finish writes the batch's words), and
the fallback pass's few workgroups take the segments in turn.  Every TokenResult against the oracle replaying the same sequence from the start (ClusterFlowChecker.java:55-112 in
arrival order), the batch's path words (sga_cluster_batch_info) on normal and fallback batches -- the words
and tickets must come back clean for the batch after a fallback -- and the next hot set."""
import ctypes as C

import numpy as np
import pytest

from tests import oracle_harness as H

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000
N1000, N500 = 3000, 50          # rules with a 1000 ms window (S = 10), then 50 with a 500 ms window
SEG = 8192                      # requests per key-pass workgroup
N_MID = 3 * SEG + 17
SHAPES = [4097, N_MID, 65 * SEG + 5]
FLAG_UNSORTED, FLAG_MIXED, FLAG_BUCKET, FLAG_STATE = 1, 2, 4, 16


def rule_list(ids):
    ids = list(ids)
    rs = [{"flow_id": int(f), "count": float(3 + (k * 7) % 40), "threshold_type": 1, "sample_count": 10,
           "window_interval_ms": 1000} for k, f in enumerate(ids[:N1000])]
    rs += [{"flow_id": int(f), "count": float(2 + k % 9), "threshold_type": 1, "sample_count": 10,
            "window_interval_ms": 500} for k, f in enumerate(ids[N1000:])]
    rs[0]["count"] = 400.0  # the hottest rule passes a good share
    return rs


DENSE_IDS = list(range(1, N1000 + N500 + 1))
SPARSE_IDS = [1_000_003 + 7919 * k for k in range(N1000 + N500)]  # far apart: the hashed flowId table


def make_batch(rng, ids, n, t, span=250, pool=N1000, floor=0):
    """n requests at sorted times in [t, t + span): skewed over the first `pool` 1000 ms rules (the first by
    far the hottest, so the hot set takes its window length), a tenth on the 500 ms rules, a few invalid ones,
    1 % prioritized.  floor: every rule of the pool and every 500 ms rule gets at least that many requests."""
    ids = np.asarray(ids, np.int64)
    fixed = np.repeat(np.concatenate([np.arange(pool), N1000 + np.arange(N500)]), floor)
    m = n - len(fixed)
    z = rng.zipf(1.25, size=m)
    k = np.where(z <= pool, z - 1, rng.integers(0, pool, size=m))
    other = rng.random(m) < 0.1
    k[other] = N1000 + rng.integers(0, N500, size=int(other.sum()))
    fid = ids[rng.permutation(np.concatenate([fixed, k]))]
    if not floor:
        fid[3::211] = 0                      # BAD_REQUEST
        fid[5::223] = int(ids.max()) + 12345  # NO_RULE_EXISTS
    acq = np.ones(n, np.int32)
    prio = (rng.random(n) < 0.01).astype(np.uint8)
    ts = t + np.sort(rng.integers(0, span, size=n)).astype(np.int64)
    return fid, acq, prio, ts


def oracle_new(rules):
    L = H.lib()
    h = L.orc_cluster_new(1.0, 1.0)
    L.orc_cluster_load_rules(h, b"default", H.cluster_rules_array(rules), len(rules))
    return h


def oracle_replay(h, fid, acq, prio, ts):
    n = len(fid)
    out = (H.OrcTokenResult * n)()
    a = [np.ascontiguousarray(fid, np.int64), np.ascontiguousarray(acq, np.int32), np.ascontiguousarray(prio, np.uint8),
         np.ascontiguousarray(ts, np.int64)]
    H.lib().orc_cluster_replay(h, n, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, out)
    r = np.frombuffer(out, dtype=np.int32).reshape(n, 3)
    return r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy()


def assert_same(got, orc, ctx):
    st, rem, wait = orc
    bad = np.nonzero((got["status"] != st) | (got["remaining"] != rem) | (got["wait_in_ms"] != wait))[0]
    if bad.size:
        i = bad[0]
        raise AssertionError(f"{ctx}: {bad.size} mismatches; first at {i}: gpu=({got['status'][i]},"
                             f"{got['remaining'][i]},{got['wait_in_ms'][i]}) oracle=({st[i]},{rem[i]},{wait[i]})")


def assert_metrics(svc, oh, flow_ids, now):
    L = H.lib()
    for f in flow_ids:
        g = svc.metric_sums(int(f), now)
        o = [L.orc_cluster_metric_sum(oh, int(f), ev, now) for ev in range(7)]
        assert g == o, (f, g, o)


def make_engine(cluster, hot_min, max_batch):
    return cluster.Engine(max_batch=max_batch, max_rules=1 << 16, hot_rules=True, hot_min_requests=hot_min,
                          small_batch=0)


def load_rules(cluster, eng, rules):
    mgr = cluster.ClusterFlowRuleManager(eng)
    fr = [cluster.FlowRule(resource=f"r{r['flow_id']}", count=r["count"], cluster_mode=True,
                           cluster_config=cluster.ClusterFlowConfig(
                               flow_id=r["flow_id"], threshold_type=r["threshold_type"],
                               sample_count=r["sample_count"], window_interval_ms=r["window_interval_ms"]))
          for r in rules]
    mgr.load_rules("default", fr)
    return mgr


def n_valid(rules, fid):
    return int(np.isin(fid, [r["flow_id"] for r in rules]).sum())


def expected_hot_next(rules, fid, hot_min):
    """The rules the next batch decides on the hot path: those with at least max(hot_min, 1) requests in this
    batch and the window length of the rule with the most (fewer than 4096 rules: no count threshold beyond
    hot_min applies)."""
    win = {r["flow_id"]: r["window_interval_ms"] for r in rules}
    ids, cnt = np.unique(fid[np.isin(fid, list(win))], return_counts=True)
    wbest = win[int(ids[np.argmax(cnt)])]
    return int(sum(1 for f, c in zip(ids, cnt) if c >= max(hot_min, 1) and win[int(f)] == wbest))


@pytest.mark.parametrize("hot_min", [1, 64])
@pytest.mark.parametrize("n", SHAPES)
def test_front_shapes_match_oracle(n, hot_min):
    """Four consecutive batches per shape: one key workgroup, a short last segment, 66 segments (more than
    the 64 stripes of the totals).  With 3,050 rules the cold elements are LSD-sorted, so no cold partition runs
    here (tests/cluster_shapes.py group P has 65 segments over 30,000 rules: two partition groups).  From the
    second batch on the hot path is taken with no flag."""
    from sentinel_amd import cluster
    rules = rule_list(DENSE_IDS)
    rng = np.random.default_rng(1000 + n + hot_min)
    oh = oracle_new(rules)
    eng = make_engine(cluster, hot_min, max_batch=1 << 20)
    load_rules(cluster, eng, rules)
    svc = cluster.DefaultTokenService(eng)
    t = T0
    for b in range(4):
        fid, acq, prio, ts = make_batch(rng, DENSE_IDS, n, t)
        t = int(ts[-1]) + 20
        g = svc.request_tokens(fid, acq, prio, ts)
        info = eng.batch_info()
        assert_same(g, oracle_replay(oh, fid, acq, prio, ts), f"n={n} hot_min={hot_min} batch {b}")
        if b >= 1:
            assert info["hot_mode"] == 1 and info["flags"] == 0, (b, info)
            assert info["n_sort"] == info["n_cold"] and info["hot_err"] == 0, (b, info)
    assert_metrics(svc, oh, list(range(1, 33)) + list(range(N1000 - 15, N1000 + 17)), t)
    H.lib().orc_cluster_free(oh)
    eng.close()


@pytest.mark.parametrize("hot_min", [1, 64])
@pytest.mark.parametrize("kind", ["unsorted", "mixed", "bucket", "state"])
def test_front_fallback_batch_then_clean(kind, hot_min):
    """One fallback batch in the middle of normal ones: its flag, every valid request decided as cold, the
    oracle's results -- and the next batch on the hot path again with no flag (control words and tickets
    came back clean)."""
    from sentinel_amd import cluster
    rules = rule_list(DENSE_IDS)
    rng = np.random.default_rng(77)
    oh = oracle_new(rules)
    eng = make_engine(cluster, hot_min, max_batch=1 << 16)
    load_rules(cluster, eng, rules)
    svc = cluster.DefaultTokenService(eng)
    t = T0
    want = {"unsorted": FLAG_UNSORTED, "mixed": FLAG_MIXED, "bucket": FLAG_BUCKET, "state": FLAG_STATE}[kind]
    for b in range(5):
        fallback = b == 2
        if fallback and kind == "bucket":  # more than 64 of the hot rules' 100 ms buckets
            fid, acq, prio, ts = make_batch(rng, DENSE_IDS, N_MID, t, span=7000)
        elif fallback and kind == "state":  # starts before a bucket the hot rules already hold
            fid, acq, prio, ts = make_batch(rng, DENSE_IDS, N_MID, t - 320)
        else:
            fid, acq, prio, ts = make_batch(rng, DENSE_IDS, N_MID, t)
        if fallback and kind == "unsorted":
            ts[N_MID // 2] = ts[N_MID // 2 - 1] - 1  # one descending timestamp
        if fallback and kind == "mixed":
            k = int(np.nonzero(fid == 1)[0][5])  # the hottest rule is hot
            acq[k] = 2
        t = max(t, int(ts.max()) + 20)
        g = svc.request_tokens(fid, acq, prio, ts)
        info = eng.batch_info()
        assert_same(g, oracle_replay(oh, fid, acq, prio, ts), f"{kind} hot_min={hot_min} batch {b}")
        if fallback:
            assert info["flags"] & want, info
            assert info["hot_mode"] == 0 and info["n_cold"] == n_valid(rules, fid), (info, n_valid(rules, fid))
        elif b >= 1:
            assert info["hot_mode"] == 1 and info["flags"] == 0, (b, info)
    assert_metrics(svc, oh, range(1, 65), t)
    H.lib().orc_cluster_free(oh)
    eng.close()


@pytest.mark.parametrize("hot_min", [1, 64])
def test_front_next_hot_set(hot_min):
    """After each batch the next hot set holds exactly the rules it should (the 500 ms rules are candidates
    that leave holes in the picked ids), and the following batch decides like the oracle.  Every rule of the
    trace has at least 16 requests per batch, so no cold workgroup (2048 sorted elements, room for 256
    candidates) has more candidates than it can publish and the set is the one expected_hot_next names."""
    from sentinel_amd import cluster
    rules = rule_list(DENSE_IDS)
    rng = np.random.default_rng(5)
    oh = oracle_new(rules)
    eng = make_engine(cluster, hot_min, max_batch=1 << 16)
    load_rules(cluster, eng, rules)
    svc = cluster.DefaultTokenService(eng)
    t = T0
    for b in range(5):
        fid, acq, prio, ts = make_batch(rng, DENSE_IDS, N_MID, t, pool=1000, floor=16)
        t = int(ts[-1]) + 20
        g = svc.request_tokens(fid, acq, prio, ts)
        info = eng.batch_info()
        assert_same(g, oracle_replay(oh, fid, acq, prio, ts), f"hot_min={hot_min} batch {b}")
        assert info["n_hot_next"] == expected_hot_next(rules, fid, hot_min), (b, info)
    H.lib().orc_cluster_free(oh)
    eng.close()


def test_front_hashed_table():
    """Sparse flowIds: the hashed-table key kernels share the key pass's front."""
    from sentinel_amd import cluster
    rules = rule_list(SPARSE_IDS)
    rng = np.random.default_rng(9)
    oh = oracle_new(rules)
    eng = make_engine(cluster, 1, max_batch=1 << 16)
    load_rules(cluster, eng, rules)
    svc = cluster.DefaultTokenService(eng)
    t = T0
    for b in range(4):
        fid, acq, prio, ts = make_batch(rng, SPARSE_IDS, N_MID, t)
        if b == 2:
            ts[100] = ts[99] - 1  # a fallback batch on this path too
        t = int(ts.max()) + 20
        g = svc.request_tokens(fid, acq, prio, ts)
        info = eng.batch_info()
        assert_same(g, oracle_replay(oh, fid, acq, prio, ts), f"hashed batch {b}")
        if b == 2:
            assert info["flags"] & FLAG_UNSORTED and info["hot_mode"] == 0, info
        elif b >= 1:
            assert info["hot_mode"] == 1 and info["flags"] == 0, (b, info)
    assert_metrics(svc, oh, SPARSE_IDS[:32] + SPARSE_IDS[N1000 - 16:N1000 + 16], t)
    H.lib().orc_cluster_free(oh)
    eng.close()


def test_front_pipelined_entry_equals_sync():
    """sga_request_tokens_device_pipelined with two batches in flight (the next batch's key pass, with its
    precheck against the latest time of every earlier batch, beside this batch's decisions) decides like one
    synchronous call per batch; batch 3 goes back in time and must stay off the hot path either way."""
    import torch
    from sentinel_amd import _lib, cluster
    L = _lib.load()
    dev = torch.device("cuda", 0)
    rules = rule_list(DENSE_IDS)
    rng = np.random.default_rng(21)
    host, t = [], T0
    for b in range(6):
        fid, acq, prio, ts = make_batch(rng, DENSE_IDS, N_MID, t - 320 if b == 3 else t)
        t = max(t, int(ts[-1]) + 20)
        host.append((fid, acq, prio, ts))
    res = {}
    for mode in ("sync", "pipe"):
        eng = make_engine(cluster, 1, max_batch=1 << 16)
        load_rules(cluster, eng, rules)
        fn = L.sga_request_tokens_device if mode == "sync" else L.sga_request_tokens_device_pipelined
        inp = torch.cuda.Stream(dev)
        keep, outs = [], []
        for fid, acq, prio, ts in host:
            base = int(ts.min())
            with torch.cuda.stream(inp):
                d = (torch.from_numpy(fid).to(dev), torch.from_numpy(acq).to(dev), torch.from_numpy(prio).to(dev),
                     torch.from_numpy((ts - base).astype(np.int32)).to(dev))
                o = torch.zeros(len(fid), dtype=torch.int64, device=dev)
            rc = fn(eng.handle, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), base, d[3].data_ptr(), len(fid),
                    o.data_ptr(), C.c_void_p(inp.cuda_stream))
            assert rc == 0, (mode, rc, L.sga_last_error(eng.handle))
            keep.append(d)
            outs.append(o)
        assert L.sga_stream_wait(eng.handle, C.c_void_p(inp.cuda_stream)) == 0
        torch.cuda.synchronize()
        res[mode] = [o.cpu().numpy() for o in outs]
        svc = cluster.DefaultTokenService(eng)
        res[mode + "_metrics"] = [svc.metric_sums(f, t) for f in range(1, 33)]
        eng.close()
    for b in range(len(host)):
        assert np.array_equal(res["sync"][b], res["pipe"][b]), f"batch {b}"
    assert res["sync_metrics"] == res["pipe_metrics"]
    oh = oracle_new(rules)
    for b, (fid, acq, prio, ts) in enumerate(host):
        r = res["pipe"][b].view(np.uint64)
        got = {"status": ((r >> np.uint64(48)) & np.uint64(0xFF)).astype(np.int8).astype(np.int32),
               "remaining": (r & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32),
               "wait_in_ms": ((r >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16).astype(np.int32)}
        assert_same(got, oracle_replay(oh, fid, acq, prio, ts), f"pipelined batch {b}")
    H.lib().orc_cluster_free(oh)
