"""The compact decision line of a cluster rule's window record (cluster_line.hpp): a
record is decided from one 128-byte line of 32-bit fields while everything fits, and turns wide -- exactly,
never clamped -- when a bucket number or a counter outgrows its field, or when sampleCount is above ten.
Every TokenResult, all seven metric sums of every touched rule and the metric nodes against the oracle
replaying the same sequence from the start (ClusterFlowChecker.java:55-112 in arrival order)."""
import numpy as np
import pytest

from tests import oracle_harness as H

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000
SEG = 8192  # requests per key-pass workgroup
BIG = 1 << 30


def rule(fid, count, s=10, iv=1000):
    return {"flow_id": int(fid), "count": float(count), "threshold_type": 1, "sample_count": s,
            "window_interval_ms": iv}


def mixed_rules():
    """About 3,000 rules of four geometries; rule 1 is by far the hottest and passes a good share."""
    rs = [rule(1 + k, 3 + (k * 7) % 40) for k in range(2000)]                 # S = 10 / 1000 ms
    rs += [rule(2001 + k, 2 + k % 9, iv=500) for k in range(500)]             # S = 10 / 500 ms
    rs += [rule(2501 + k, 2 + k % 11, s=4) for k in range(300)]               # S = 4 (W = 250 ms)
    rs += [rule(2801 + k, 2 + k % 13, s=12, iv=1200) for k in range(200)]     # S = 12: wide from the start
    rs[0]["count"] = 400.0
    return rs


class Pair:
    """An engine and the oracle fed the same rules and requests."""

    def __init__(self, rules, **engine_args):
        from sentinel_amd import cluster
        self.cluster = cluster
        self.L = H.lib()
        self.oh = self.L.orc_cluster_new(1.0, 1.0)
        self.eng = cluster.Engine(max_batch=1 << 16, max_rules=1 << 16, **engine_args)
        self.mgr = cluster.ClusterFlowRuleManager(self.eng)
        self.svc = cluster.DefaultTokenService(self.eng)
        self.load(rules)

    def load(self, rules):
        self.rules = rules
        self.L.orc_cluster_load_rules(self.oh, b"default", H.cluster_rules_array(rules), len(rules))
        c = self.cluster
        self.mgr.load_rules("default", [
            c.FlowRule(resource=f"r{r['flow_id']}", count=r["count"], cluster_mode=True,
                       cluster_config=c.ClusterFlowConfig(flow_id=r["flow_id"], threshold_type=r["threshold_type"],
                                                          sample_count=r["sample_count"],
                                                          window_interval_ms=r["window_interval_ms"]))
            for r in rules])

    def batch(self, fid, acq, prio, ts, ctx):
        """One batch through both; every TokenResult compared."""
        n = len(fid)
        a = [np.ascontiguousarray(fid, np.int64), np.ascontiguousarray(acq, np.int32),
             np.ascontiguousarray(prio, np.uint8), np.ascontiguousarray(ts, np.int64)]
        got = self.svc.request_tokens(*a)
        out = (H.OrcTokenResult * n)()
        self.L.orc_cluster_replay(self.oh, n, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data,
                                  out)
        r = np.frombuffer(out, dtype=np.int32).reshape(n, 3)
        bad = np.nonzero((got["status"] != r[:, 0]) | (got["remaining"] != r[:, 1]) | (got["wait_in_ms"] != r[:, 2]))[0]
        if bad.size:
            i = bad[0]
            raise AssertionError(f"{ctx}: {bad.size} of {n} mismatch; first at {i} (flow {a[0][i]}, acquire {a[1][i]}, "
                                 f"prio {a[2][i]}, t {a[3][i]}): gpu=({got['status'][i]},{got['remaining'][i]},"
                                 f"{got['wait_in_ms'][i]}) oracle={tuple(r[i])}")
        return got

    def check_metrics(self, touched, now, ctx):
        """All seven sums of every touched rule, and the metric node of every rule, at `now`.  The node
        snapshot rotates every rule's window at `now`, so the oracle is asked about every rule too."""
        import torch
        from sentinel_amd.metrics import cluster_metric_snapshot
        for f in sorted(set(int(x) for x in touched)):
            g = self.svc.metric_sums(f, now)
            o = [self.L.orc_cluster_metric_sum(self.oh, f, ev, now) for ev in range(7)]
            assert g == o, (ctx, f, g, o)
        torch.cuda.set_device(0)
        nodes = cluster_metric_snapshot(self.eng, now)
        assert len(nodes) == len(self.rules), ctx
        by = {int(r["flow_id"]): r for r in nodes}
        for r in self.rules:
            f, isec = r["flow_id"], r["window_interval_ms"] / 1000.0
            m = by[f]
            # getAvg(BLOCK) then getAvg(PASS) at now (ClusterMetricNodeGenerator.java:75-91)
            assert m["block_qps"] == self.L.orc_cluster_metric_sum(self.oh, f, 1, now) / isec, (ctx, f)
            assert m["pass_qps"] == self.L.orc_cluster_metric_sum(self.oh, f, 0, now) / isec, (ctx, f)
            assert m["timestamp"] == now, (ctx, f)

    def close(self):
        self.L.orc_cluster_free(self.oh)
        self.eng.close()


def traffic(rng, ids, n, t, span=250, prio_share=0.01):
    """n acquire-1 requests at sorted times in [t, t + span), skewed over ids (the first the hottest), a few
    invalid ones."""
    ids = np.asarray(ids, np.int64)
    z = rng.zipf(1.25, size=n)
    k = np.where(z <= len(ids), z - 1, rng.integers(0, len(ids), size=n))
    fid = ids[k]
    fid[3::211] = 0                       # BAD_REQUEST
    fid[5::223] = int(ids.max()) + 12345  # NO_RULE_EXISTS
    acq = np.ones(n, np.int32)
    prio = (rng.random(n) < prio_share).astype(np.uint8)
    ts = t + np.sort(rng.integers(0, span, size=n)).astype(np.int64)
    return fid, acq, prio, ts


def valid_ids(p, fid):
    return np.unique(fid[np.isin(fid, [r["flow_id"] for r in p.rules])])


PATHS = {"hot": dict(hot_rules=True, hot_min_requests=8, small_batch=0),
         "sort": dict(hot_rules=False, small_batch=0)}


@pytest.mark.parametrize("path", ["hot", "sort"])
@pytest.mark.parametrize("n", [1500, 4097, 3 * SEG + 17])
def test_compact_forms_ordinary_traffic(n, path):
    """Four consecutive batches over rules of four geometries (S = 12 is wide from the start): the second
    continues the first's bucket (the cached group's tag hits), the third rotates, the fourth comes more than
    a whole interval later.  1 % prioritized (occupy transfer, SHOULD_WAIT); one rule reload between batches
    changes thresholds (the record's threshold copy).  1,500 requests take the small path."""
    args = dict(PATHS[path])
    if n == 1500:
        args["small_batch"] = 4096
    rules = mixed_rules()
    ids = [r["flow_id"] for r in rules]
    order = np.random.default_rng(3).permutation(ids[1:])
    ids = [ids[0]] + [int(x) for x in order]  # every geometry among the frequent rules
    p = Pair(rules, **args)
    rng = np.random.default_rng(100 + n)
    t = T0 + 10
    for b, gap in enumerate([0, 5, 130, 2600]):
        t += gap
        if b == 2:  # reload: every third rule gets another threshold, metrics stay
            rules = [dict(r, count=r["count"] + (2.0 if k % 3 == 0 else 0.0)) for k, r in enumerate(rules)]
            p.load(rules)
        fid, acq, prio, ts = traffic(rng, ids, n, t, span=60 if b < 2 else 250)
        p.batch(fid, acq, prio, ts, f"n={n} {path} batch {b}")
        t = int(ts[-1])
        if b in (1, 3) and path == "hot" and n > 1500:  # (a rule load empties the hot set: not batch 2)
            info = p.eng.batch_info()
            assert info["hot_mode"] == 1 and info["hot_err"] == 0, (b, info)
        p.check_metrics(valid_ids(p, fid), t, f"n={n} {path} batch {b}")
    p.close()


@pytest.mark.parametrize("path", ["hot", "sort"])
def test_widening_by_count(path):
    """Counters that outgrow 32 bits.  Rule 1 (the batch's hottest, so a hot-set rule turns wide) and rule 2:
    count 1e12, a handful of requests of acquire 2^30 take PASS past 2^32.  Rule 3: a small count, the same
    requests are blocked and take BLOCK past 2^32 (the cached group no longer fits: only its tag goes).
    Rule 4: prioritized requests of acquire 2^30 occupy the next bucket (counters with the top bit set, then
    the transfer into PASS).  Later batches of acquire-1 requests continue the same bucket and the next."""
    rules = [rule(1, 1e12), rule(2, 1e12), rule(3, 5), rule(4, 8.0 * BIG)] + [rule(10 + k, 3 + k % 17) for k in range(300)]
    p = Pair(rules, **PATHS[path])
    rng = np.random.default_rng(11)
    ids = [r["flow_id"] for r in rules]
    t = T0 + 10
    touched = set()

    def ordinary(n, t, span, ctx):
        fid, acq, prio, ts = traffic(rng, ids, n, t, span=span, prio_share=0.02)
        p.batch(fid, acq, prio, ts, ctx)
        touched.update(valid_ids(p, fid).tolist())
        return int(ts[-1])

    t = ordinary(4097, t, 40, "before")
    # rule 4: three passes of 2^30 in this bucket and three in the next (each bucket's PASS still fits)
    fid = np.array([4] * 6, np.int64)
    ts = np.array([t + 1] * 3 + [t + 101] * 3, np.int64)
    p.batch(fid, np.full(6, BIG, np.int32), np.zeros(6, np.uint8), ts, "rule 4 fill")
    t0 = t + 1
    # the big requests inside an ordinary batch, in the bucket the batch before ended in
    fid, acq, prio, ts = traffic(rng, ids, 4097, t + 2, span=30, prio_share=0.02)
    for f, k0 in ((1, 100), (2, 200), (3, 300)):
        sl = slice(k0, k0 + 6)
        fid[sl], acq[sl], prio[sl] = f, BIG, 0
    p.batch(fid, acq, prio, ts, "big acquires")
    touched.update(valid_ids(p, fid).tolist())
    t = int(ts[-1])
    t = ordinary(4097, t + 1, 30, "same bucket after")
    p.check_metrics(touched, t, "same bucket after")
    t = ordinary(4097, t + 100, 30, "next bucket after")
    p.check_metrics(touched, t, "next bucket after")
    # rule 4, nine buckets after its first: the head bucket holds 3 x 2^30, two more pass, then prioritized
    # requests occupy (SHOULD_WAIT) until the borrowed bucket is full, the rest is blocked
    t9 = t0 + 900
    assert t9 > t
    fid = np.array([4] * 8, np.int64)
    prio = np.array([0, 0, 1, 1, 1, 1, 1, 0], np.uint8)
    got = p.batch(fid, np.full(8, BIG, np.int32), prio, np.full(8, t9, np.int64), "rule 4 occupy")
    assert (got["status"] == 2).any(), got["status"]  # SHOULD_WAIT happened
    # the transfer of the occupied tokens into the next bucket's PASS, by ordinary traffic
    t = ordinary(4097, t9 + 100, 30, "after occupy")
    p.check_metrics(touched | {4}, t, "after occupy")
    if path == "hot":
        info = p.eng.batch_info()
        assert info["hot_mode"] == 1 and info["hot_err"] == 0, info
    p.close()


def test_widening_by_time_short_windows():
    """W = 1 ms (S = 10, interval 10 ms): a batch at T0, one 2^32 + 5 ms later (the bucket number no longer
    fits the 32-bit difference to the base), one far before T0 (the reference's detached bucket for the rules
    that hold newer buckets; for rules 200.. it is the first regression of a compact record, past its base)."""
    rules = [rule(1 + k, 2 + k % 7, iv=10) for k in range(400)]
    p = Pair(rules, hot_rules=True, hot_min_requests=8, small_batch=0)
    rng = np.random.default_rng(21)
    ids = [r["flow_id"] for r in rules]
    plan = [(T0, ids), (T0 + 3, ids), (T0 + (1 << 32) + 5, ids[:200]), (T0 + (1 << 32) + 9, ids[:200]),
            (T0 - 100_000, ids), (T0 - 100_000 + 4, ids), (T0 + (1 << 32) + 12, ids)]
    for b, (t, pool) in enumerate(plan):
        fid, acq, prio, ts = traffic(rng, pool, 4097, t, span=6)
        p.batch(fid, acq, prio, ts, f"batch {b} at {t}")
        p.check_metrics(valid_ids(p, fid), int(ts[-1]), f"batch {b} at {t}")
    p.close()


def test_widening_by_time_bucket_number_near_2_47():
    """W = 100 ms at times whose bucket number is just below 2^47, crosses it, and (rules 200.., first touched
    there) lies so far above it that no base below 2^47 reaches the bucket."""
    rules = [rule(1 + k, 2 + k % 7) for k in range(400)]
    p = Pair(rules, hot_rules=True, hot_min_requests=8, small_batch=0)
    rng = np.random.default_rng(22)
    ids = [r["flow_id"] for r in rules]
    q47 = 1 << 47
    plan = [((q47 - 3) * 100, ids[:200]), ((q47 - 2) * 100 + 50, ids[:200]), (q47 * 100 + 10, ids[:200]),
            ((q47 + 70_000) * 100, ids), ((q47 + 70_001) * 100 + 20, ids)]
    for b, (t, pool) in enumerate(plan):
        fid, acq, prio, ts = traffic(rng, pool, 4097, t, span=150)
        p.batch(fid, acq, prio, ts, f"batch {b} at {t}")
        p.check_metrics(valid_ids(p, fid), int(ts[-1]), f"batch {b} at {t}")
    p.close()


def test_fresh_slot_after_widening():
    """A rule whose record turned wide is dropped by a rule load and loaded again: the new metric's slot is
    initialised afresh (compact again; the form itself is not visible through the API, the results are)."""
    rules = [rule(1, 1e12), rule(2, 7)] + [rule(10 + k, 3 + k % 17) for k in range(100)]
    p = Pair(rules, hot_rules=True, hot_min_requests=8, small_batch=0)
    rng = np.random.default_rng(31)
    ids = [r["flow_id"] for r in rules]
    t = T0 + 10
    fid, acq, prio, ts = traffic(rng, ids, 4097, t, span=40)
    fid[50:56], acq[50:56], prio[50:56] = 1, BIG, 0  # PASS of rule 1 past 2^32
    p.batch(fid, acq, prio, ts, "widen")
    t = int(ts[-1])
    p.load(rules[1:])  # rule 1 and its metric go
    p.load(rules)      # a new metric for rule 1
    for b in range(2):
        fid, acq, prio, ts = traffic(rng, ids, 4097, t + 1 + 100 * b, span=40)
        p.batch(fid, acq, prio, ts, f"fresh batch {b}")
        t = int(ts[-1])
        p.check_metrics(valid_ids(p, fid), t, f"fresh batch {b}")
    p.close()
