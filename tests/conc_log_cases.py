"""Shared by the concurrency server log tests: the reference reduce, the engine / oracle pair and the traces.

Expected rows never come from the engine: reduce_conc restates the four call sites of ClusterServerStatLogUtil.log in
ConcurrentClusterFlowChecker (java:58,67 block, :73 pass, :99 release) over the C oracle's statuses
(orc_cluster_concurrent_acquire / _release), and a release's (flowId, acquireCount) is read from the oracle's token
node before the release is applied.  As in tests/test_concurrent_gpu.py the oracle is handed the token ids the engine
issued.  count and events are integer sums, so rows are compared exactly everywhere."""
import ctypes as C

import numpy as np

from tests import oracle_harness as H
from tests import server_log_cases as sc

T0 = sc.T0
CONC_PASS, CONC_BLOCK, CONC_RELEASE = 6, 7, 8
OK, BLOCKED, NO_RULE_EXISTS, BAD_REQUEST, RELEASE_OK, ALREADY_RELEASE = 0, 1, 3, -4, 6, 7
ACQUIRE, RELEASE = 0, 1
CLIENT_NONE = 0xFFFFFFFF

SEAM_SIZES = sc.SEAM_SIZES
SEAM_PATTERNS = ("one", "distinct", "alternate", "displace", "second", "release")
WIDE = 100  # seam_rules' rule that never blocks


def reduce_conc(acc, op, ids, acquire, ts, status, token_info):
    """Adds one batch to acc {(time_slot, flow_id, kind, 0): [count, events]} and returns it.  op 0: ids are flowIds,
    op 1: tokenIds; token_info[token] = (flow_id, acquire) of the token's node before its release."""
    for i in range(len(op)):
        t, st = int(ts[i]), int(status[i])
        if int(op[i]) == ACQUIRE:
            if st == OK:
                key, add = (int(ids[i]), CONC_PASS), int(acquire[i])
            elif st == BLOCKED:
                key, add = (int(ids[i]), CONC_BLOCK), int(acquire[i])
            else:
                continue
        elif st == RELEASE_OK:
            fid, add = token_info[int(ids[i])]  # the node's, not what the release call carries
            key = (int(fid), CONC_RELEASE)
        else:
            continue
        row = acc.setdefault((t - t % 1000,) + key + (0,), [0, 0])
        row[0] += add
        row[1] += 1
    return acc


def conc_rule(fid, count, threshold_type=1, resource_timeout=2000, client_offline_time=2000):
    return {"flow_id": fid, "count": float(count), "threshold_type": threshold_type,
            "resource_timeout": resource_timeout, "client_offline_time": client_offline_time}


def level_of(rule, connected):
    """ConcurrentClusterFlowChecker.calcGlobalThreshold: count (GLOBAL, 1) or count * connectedCount (AVG_LOCAL, 0)."""
    return rule["count"] if rule["threshold_type"] == 1 else rule["count"] * float(connected)


class ConcPair:
    """One engine and one oracle fed the same concurrency operations.  log: None = off, else max_rows."""

    def __init__(self, rules, log=0, ns="ns", connected=None, max_batch=1 << 12):
        from sentinel_amd import cluster
        self.cl, self.ns, self.connected = cluster, ns, connected
        self.L = H.lib()
        self.oh = self.L.orc_cluster_new(1.0, 1.0)
        self.eng = cluster.Engine(max_batch=max_batch)
        self.svc = cluster.DefaultTokenService(self.eng)
        self.mgr = cluster.ClusterFlowRuleManager(self.eng)
        if connected is not None:
            self.set_connected(connected)
        self.rules = {}
        self.load(rules)
        if log is not None:
            self.eng.server_log_enable(log)

    def set_connected(self, n):
        self.connected = n
        self.mgr.set_connected_count(self.ns, n)
        self.L.orc_cluster_set_connected_count(self.oh, self.ns.encode(), n)

    def load(self, rules):
        cl = self.cl
        rules = list(rules)
        self.rules = {r["flow_id"]: r for r in rules}
        self.mgr.load_rules(self.ns, [cl.FlowRule(
            resource=f"r{r['flow_id']}", count=r["count"], grade=0, cluster_mode=True,
            cluster_config=cl.ClusterFlowConfig(flow_id=r["flow_id"], threshold_type=r["threshold_type"],
                                                resource_timeout=r["resource_timeout"],
                                                client_offline_time=r["client_offline_time"])) for r in rules])
        self.L.orc_cluster_load_rules(self.oh, self.ns.encode(), H.cluster_rules_array(rules), len(rules))

    def run(self, op, client, ids, acquire, ts, acc=None):
        """One sga_concurrent_ops call and the oracle's sequential replay of it: asserts equal statuses, adds the
        reduce over the oracle's statuses to acc and returns (engine results, oracle statuses)."""
        got = self.svc.concurrent_ops(op, client, ids, acquire, ts)
        n = len(op)
        status = np.zeros(n, np.int32)
        info = {}
        f, cd, rd, aq = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        for i in range(n):
            if int(op[i]) == ACQUIRE:
                status[i] = self.L.orc_cluster_concurrent_acquire(self.oh, int(client[i]), int(ids[i]), int(acquire[i]),
                                                                  int(ts[i]), int(got["token_id"][i])).status
            else:
                tok = int(ids[i])
                if self.L.orc_cluster_concurrent_get(self.oh, tok, C.byref(f), C.byref(cd), C.byref(rd), C.byref(aq)):
                    info[tok] = (f.value, aq.value)
                status[i] = self.L.orc_cluster_concurrent_release(self.oh, tok)
        bad = np.nonzero(got["status"] != status)[0]
        assert bad.size == 0, (bad[:5], got["status"][bad[:5]], status[bad[:5]])
        if acc is not None:
            reduce_conc(acc, op, ids, acquire, ts, status, info)
        return got, status

    def acquire(self, fids, acq, ts, acc=None, client=0):
        n = len(fids)
        return self.run(np.zeros(n, np.uint8), np.full(n, client, np.uint32), np.asarray(fids, np.int64),
                        np.asarray(acq, np.int32), np.asarray(ts, np.int64), acc)

    def release(self, tokens, ts, acc=None, junk=0):
        n = len(tokens)
        return self.run(np.ones(n, np.uint8), np.full(n, CLIENT_NONE, np.uint32), np.asarray(tokens, np.int64),
                        np.full(n, junk, np.int32), np.asarray(ts, np.int64), acc)

    def oracle_now_calls(self, fid):
        v = C.c_int32()
        return v.value if self.L.orc_cluster_concurrent_now_calls(self.oh, int(fid), C.byref(v)) else None

    def oracle_tokens(self):
        return int(self.L.orc_cluster_concurrent_tokens(self.oh))

    def expected_gauges(self):
        """[(flow_id, level, nowCalls)] by flowId over the loaded rules whose nowCalls != 0 in the oracle."""
        out = []
        for fid in sorted(self.rules):
            v = self.oracle_now_calls(fid)
            if v:
                out.append((fid, level_of(self.rules[fid], self.connected or 0), v))
        return out

    def gauges(self):
        rows, size = self.eng.concurrent_gauges()
        assert not np.asarray(rows["reserved"]).any()
        return [(int(r["flow_id"]), float(r["level"]), int(r["now_calls"])) for r in rows], size

    def close(self):
        self.L.orc_cluster_free(self.oh)
        self.eng.close()


def seam_rules():
    """server_log_cases.seam_rules as concurrency rules: 1..64 of threshold 0 (every acquire is blocked), 100 wide."""
    return [conc_rule(r["flow_id"], r["count"]) for r in sc.seam_rules()]


def seam_acquires(n, pattern, t0):
    """(flow_id, acquire, ts) of n acquires: server_log_cases.seam_trace's rules and times (one / distinct /
    alternate / displace / second), acquire alternating 1 and 3 so that count differs from events."""
    fid, _, _, ts = sc.seam_trace(n, pattern, t0)
    acq = np.where(np.arange(n) % 2 == 1, 3, 1).astype(np.int32)
    return fid, acq, ts


def release_batch(tokens, t0, rng):
    """The second batch of the `release` pattern: every token released once in shuffled order, interleaved with
    blocked acquires (rule 1) and repeated releases; every release carries a junk acquire field; the times cross a
    second inside the batch.  Returns (op, client, ids, acquire, ts)."""
    n = len(tokens)
    order = rng.permutation(n)
    op, ids, acq = [], [], []
    for j, k in enumerate(order):
        op.append(RELEASE)
        ids.append(int(tokens[k]))
        acq.append(int(rng.integers(-5, 1000)))
        if j % 3 == 0:
            op.append(ACQUIRE)
            ids.append(1)
            acq.append(2)
        if j % 4 == 1:  # a token released earlier in this batch: ALREADY_RELEASE
            op.append(RELEASE)
            ids.append(int(tokens[order[int(rng.integers(0, j + 1))]]))
            acq.append(int(rng.integers(-5, 1000)))
    m = len(op)
    ts = t0 + 990 + (np.arange(m) * 20) // max(m, 1)  # 990 .. 1009: the batch straddles a second
    return (np.asarray(op, np.uint8), np.zeros(m, np.uint32), np.asarray(ids, np.int64), np.asarray(acq, np.int32),
            ts.astype(np.int64))
