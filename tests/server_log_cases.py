"""Shared by the token server log tests: the reference reduce and the traces.

Expected rows never come from the engine: reduce_rows forms them from the C oracle's statuses of the same trace,
restating the call sites of ClusterServerStatLogUtil.log (ClusterFlowChecker.java:91,102-107,
ClusterParamFlowChecker.java:77-79, SimpleClusterFlowChecker.java:49-61).  count and events are integer sums, so rows
are compared exactly everywhere."""
import ctypes as C

import numpy as np

from tests import oracle_harness as H

T0 = 1_700_000_000_000  # a whole second
FLOW_BLOCK, FLOW_BLOCK_PRIO, FLOW_WAITING, FLOW_PASS, PARAM_PASS, PARAM_BLOCK = range(6)
OK, BLOCKED, SHOULD_WAIT = 0, 1, 2
M64 = (1 << 64) - 1

SEAM_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1025)
SEAM_PATTERNS = ("one", "distinct", "alternate", "displace", "second")
SEAM_RULES = 64  # count-0 rules 1..64: every request on them is blocked


def reduce_rows(acc, flow_id, acquire, prio, ts, status, checker="default", values=None, can_block=None):
    """Adds one batch to acc {(time_slot, flow_id, kind, tag): [count, events]} and returns it.  checker: "default"
    (ClusterFlowChecker), "simple" (the RLS SimpleClusterFlowChecker: prio ignored) or "param"
    (ClusterParamFlowChecker: values[i] is request i's collection; can_block(flow_id, value) says whether a value
    can be the blockObject -- the traces give thresholds under which that is known -- and the tag is the first such
    value in collection order)."""
    for i in range(len(flow_id)):
        f, a, t, st = int(flow_id[i]), int(acquire[i]), int(ts[i]), int(status[i])
        kind, tag, add = None, 0, 1
        if checker == "param":
            vals = values[i]
            if len(vals) and st == OK:
                kind = PARAM_PASS
            elif len(vals) and st == BLOCKED:
                kind = PARAM_BLOCK
                tag = next(int(v) & M64 for v in vals if can_block(f, int(v)))
        elif st == BLOCKED:
            kind = FLOW_BLOCK_PRIO if (checker == "default" and prio is not None and prio[i]) else FLOW_BLOCK
            add = a
        elif st == SHOULD_WAIT:
            kind = FLOW_WAITING
        elif st == OK and checker == "simple":
            kind, add = FLOW_PASS, a
        if kind is None:
            continue
        row = acc.setdefault((t - t % 1000, f, kind, tag), [0, 0])
        row[0] += add
        row[1] += 1
    return acc


def expected_tuples(acc):
    """acc as the drain orders it: (time_slot, flow_id, kind, tag, count, events)."""
    return [k + (v[0], v[1]) for k, v in sorted(acc.items())]


def as_tuples(rows):
    assert not np.asarray(rows["reserved"]).any()
    return [(int(r["time_slot"]), int(r["flow_id"]), int(r["kind"]), int(r["tag"]), int(r["count"]),
             int(r["events"])) for r in rows]


def rows_array(tuples):
    """(time_slot, flow_id, kind, tag, count, events) tuples as drained rows."""
    from sentinel_amd.server_log import SERVER_LOG_ROW_DTYPE
    a = np.zeros(len(tuples), dtype=SERVER_LOG_ROW_DTYPE)
    for i, (slot, fid, kind, tag, count, events) in enumerate(tuples):
        a[i] = (slot, fid, tag, count, events, kind, (0, 0, 0))
    return a


# ---------------------------------------------------------------- oracle
class Oracle:
    """One oracle token server: flow rules as dicts (oracle_harness.cluster_rules_array)."""

    def __init__(self, rules=(), param_rules=(), ns="default", limit=None):
        self.L = H.lib()
        self.h = self.L.orc_cluster_new(1.0, 1.0)
        self.keep = []
        if rules:
            arr = H.cluster_rules_array(list(rules))
            assert self.L.orc_cluster_load_rules(self.h, ns.encode(), arr, len(rules)) == len(rules)
        if param_rules:
            arr = H.cluster_param_rules_array(list(param_rules), self.keep)
            assert self.L.orc_cluster_load_param_rules(self.h, ns.encode(), arr, len(param_rules)) == len(param_rules)
        if limit is not None:
            self.L.orc_cluster_set_namespace_limit(self.h, ns.encode(), float(limit))

    @staticmethod
    def _arr(x, dt):
        return np.ascontiguousarray(x, dtype=dt)

    def replay(self, fid, acq, prio, ts):
        """orc_cluster_replay: (status, remaining, wait) int32 columns."""
        n = len(fid)
        f, a, p, t = self._arr(fid, np.int64), self._arr(acq, np.int32), self._arr(prio, np.uint8), \
            self._arr(ts, np.int64)
        out = (H.OrcTokenResult * max(1, n))()
        self.L.orc_cluster_replay(self.h, n, f.ctypes.data, a.ctypes.data, p.ctypes.data, t.ctypes.data, out)
        return np.frombuffer(out, dtype=np.int32).reshape(-1, 3)[:n].copy()

    def simple(self, fid, acq, ts):
        """orc_cluster_request_token_simple per request: (status, remaining, wait)."""
        out = np.zeros((len(fid), 3), np.int32)
        for i in range(len(fid)):
            r = self.L.orc_cluster_request_token_simple(self.h, int(fid[i]), int(acq[i]), int(ts[i]))
            out[i] = (r.status, r.remaining, r.wait_in_ms)
        return out

    def param(self, fid, acq, values, ts):
        """orc_cluster_request_param_token per request: (status, remaining, wait)."""
        out = np.zeros((len(fid), 3), np.int32)
        for i in range(len(fid)):
            v = (C.c_int64 * max(1, len(values[i])))(*[int(x) for x in values[i]])
            r = self.L.orc_cluster_request_param_token(self.h, int(fid[i]), int(acq[i]), v, len(values[i]), int(ts[i]))
            out[i] = (r.status, r.remaining, r.wait_in_ms)
        return out

    def close(self):
        self.L.orc_cluster_free(self.h)


def same_results(got, ref, what=""):
    """The engine's TOKEN_DTYPE results against the oracle's (status, remaining, wait) columns."""
    bad = np.nonzero((got["status"] != ref[:, 0]) | (got["remaining"] != ref[:, 1]) |
                     (got["wait_in_ms"] != ref[:, 2]))[0]
    assert bad.size == 0, (what, bad[:5], got[bad[:5]], ref[bad[:5]])


# ---------------------------------------------------------------- traces
def seam_rules():
    """Rules 1..64 of count 0 (always blocked), rule 100 of count 1e9 (never blocked)."""
    r = [{"flow_id": f, "count": 0.0, "threshold_type": 1} for f in range(1, SEAM_RULES + 1)]
    return r + [{"flow_id": 100, "count": 1e9, "threshold_type": 1}]


def seam_trace(n, pattern, t0):
    """n requests of one seam pattern: (flow_id, acquire, prio, ts).  acquire in {1, 3}: count differs from events.
      one        every request on rule 1: the wave's held tuple
      distinct   lane l of every wave on rule l + 1: every lane has a tuple of its own
      alternate  rules 1 and 2 in turn
      displace   tile 0 of a block's wave: rule 1 on a few lanes (held), rule 2 once; the later tiles of the same
                 wave: rule 3 on most lanes, which displaces the held tuple
      second     one rule; times 999 up to lane 31 and 1000 from lane 32 of every wave, and every fourth wave a
                 second earlier than the one before: time goes backwards inside the batch"""
    i = np.arange(n)
    fid = np.ones(n, np.int64)
    ts = np.full(n, t0 + 5, np.int64)
    if pattern == "distinct":
        fid = (i % 64 + 1).astype(np.int64)
    elif pattern == "alternate":
        fid = (i % 2 + 1).astype(np.int64)
    elif pattern == "displace":
        first = (i // 256) % 4 == 0
        fid = np.where(first, np.where(i % 64 < 3, 1, np.where(i % 64 == 3, 2, 100)),
                       np.where(i % 64 < 50, 3, 1)).astype(np.int64)
    elif pattern == "second":
        ts = t0 + 2000 + np.where(i % 64 < 32, 999, 1000) - 1000 * ((i // 64) % 4 == 3)
    acq = np.where(i % 5 == 0, 3, 1).astype(np.int32)
    prio = np.zeros(n, np.uint8)
    return fid, acq, prio, ts.astype(np.int64)


PATH_RULES = 40


def path_rules():
    """40 rules: small counts so most requests block, sample counts 1 / 2 / 10."""
    return [{"flow_id": f, "count": float(1 + f % 7), "threshold_type": 1, "sample_count": (1, 2, 10)[f % 3],
             "window_interval_ms": 1000} for f in range(1, PATH_RULES + 1)]


def path_trace(seed=5, n=1400, batches=3):
    """Three batches of 1,400 requests over two seconds each, times ascending: rules 1..6 frequent with acquire 1
    (the hot path's rules once a scratch set has seen a batch: the second batch, or the third through the pipelined
    entry, whose batches alternate between two sets), the rest with acquire 1..3; 10 % prioritized; some flowId 0
    (BAD_REQUEST) and unknown flowIds (NO_RULE_EXISTS)."""
    rng = np.random.default_rng(seed)
    out = []
    t = T0
    for _ in range(batches):
        hot = rng.random(n) < 0.7
        fid = np.where(hot, rng.integers(1, 7, size=n), rng.integers(7, PATH_RULES + 1, size=n)).astype(np.int64)
        acq = np.where(hot, 1, rng.integers(1, 4, size=n)).astype(np.int32)
        fid[rng.random(n) < 0.01] = 0
        fid[rng.random(n) < 0.01] = 777_777
        prio = (rng.random(n) < 0.1).astype(np.uint8)
        ts = (t + np.sort(rng.integers(0, 2000, size=n))).astype(np.int64)
        t = int(ts[-1]) + 1
        out.append((fid, acq, prio, ts))
    return out
