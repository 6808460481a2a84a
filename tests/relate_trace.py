"""TEST INFRASTRUCTURE: expected values for FlowRules with strategy RELATE.

The oracle serves strategy DIRECT only, so a stream with RELATE rules is decided by driving the oracle
event by event (FlowRuleChecker.java:83-116, DefaultController.java:49-78):

  * the oracle holds every rule except the RELATE ones this helper evaluates itself;
  * an entry on a resource with such rules evaluates them in list order.  A rule whose refResource has not
    been entered yet selects a null node and is skipped (FlowRuleChecker.java:86-89).  Otherwise the rule reads
    the referenced node through the oracle's getter -- (int) passQps() at the entry's time, which rotates the
    node's window exactly as the rule's read does, or curThreadNum() -- and blocks iff cur + acquire > count;
  * a block is handed to the oracle as a kind-2 event: StatisticSlot's BlockException branch on the entered
    resource's own node, which is all a FlowException does there.  The expected block detail is the rule's
    index.  A pass goes on to the oracle as a normal entry (the resource's remaining rules, breakers, ...);
    a FLOW block detail from there is shifted by the number of RELATE rules ahead of it;
  * ClusterBuilderSlot creates a resource's node at its first kind 0 / 2 / 3 event, ahead of every check.

The helper's RELATE rules must be DefaultController rules (QPS or THREAD grade) listed ahead of the resource's
other rules.  With self_direct=True a rule that references its own resource goes to the oracle as a DIRECT
rule instead (the node is the same and never null), which admits every controller.
"""
import ctypes as C
import heapq

import numpy as np

from tests import local_trace as lt

REF_NONE = 0xFFFFFFFF


def is_relate(r):
    return r.get("strategy", 0) == 1


class RelateTrace:
    def __init__(self, n_res, flow_rules=(), param_rules=(), degrade_rules=(), self_direct=False, system=None):
        self.n_res = n_res
        self.self_direct = self_direct
        self.orc = lt.Oracle(n_res, [], list(param_rules), list(degrade_rules))
        if system is not None:
            self.orc.system(system)
        self.L = self.orc.L
        self.entered = set()
        self.ev = []       # the stream the engine gets
        self.exp = []      # (decision, wait) per event
        self.heap = []
        self.seq = 0
        self.n_block = self.n_pass = self.n_null = 0
        self.load(flow_rules)

    def _mine(self, r):
        return is_relate(r) and not (self.self_direct and r.get("ref") == r["resource"])

    def load(self, flow_rules):
        """FlowRuleManager.loadRules: raters reset, node statistics and the entered set kept."""
        self.relate = {}
        direct = []
        seen_direct = set()
        for r in flow_rules:
            if self._mine(r):
                assert r["resource"] not in seen_direct, "RELATE rules go ahead of the resource's other rules"
                assert r.get("grade", 1) == 0 or r.get("control_behavior", 0) == 0, "DefaultController only"
                self.relate.setdefault(r["resource"], []).append(r)
            else:
                seen_direct.add(r["resource"])
                d = dict(r)
                d["strategy"] = 0
                d.pop("ref", None)
                direct.append(d)
        self.orc.load(flow_rules=direct)

    # ---- one event each
    def _drive(self, kind, rid, ts, acq, fl, rt, pv):
        a = [np.array([kind], np.uint8), np.array([rid], np.uint32), np.array([ts], np.int64),
             np.array([acq], np.int32), np.array([fl], np.uint8), np.array([rt], np.int64), np.array([pv], np.uint64)]
        dec = np.zeros(1, np.int8)
        wait = np.zeros(1, np.int32)
        self.L.orc_flow_replay_p(self.orc.h, 1, *[x.ctypes.data for x in a], dec.ctypes.data, wait.ctypes.data)
        return int(dec[0]), int(wait[0])

    def _record(self, kind, rid, ts, acq, fl, rt, pv, exp):
        self.ev.append((kind, rid, ts, acq, fl, rt, pv))
        self.exp.append(exp)

    def entry(self, rid, ts, acq=1, prio=0, hp=0, pv=0, inb=0):
        fl = (1 if prio else 0) | (4 if hp else 0) | (8 if inb else 0)
        self.entered.add(rid)
        live = null = False
        for k, r in enumerate(self.relate.get(rid, ())):
            ref = r.get("ref", REF_NONE)
            if ref is None or ref >= self.n_res or ref not in self.entered:
                null = True
                continue
            node = self.L.orc_flow_node(self.orc.h, ref)
            if r.get("grade", 1) == 1:
                cur = int(self.L.orc_node_pass_qps(node, ts))
            else:
                cur = int(self.L.orc_node_cur_thread_num(node))
            live = True
            if cur + acq > r["count"]:
                assert not (prio and r.get("grade", 1) == 1), "occupy on the referenced node is not modelled"
                self._drive(2, rid, ts, acq, fl & 8, 0, 0)
                self._record(0, rid, ts, acq, fl, 0, pv, (1, k))
                self.n_block += 1
                return 1, k
        d, w = self._drive(0, rid, ts, acq, fl, 0, pv)
        if d == 1:
            w += len(self.relate.get(rid, ()))
        self._record(0, rid, ts, acq, fl, 0, pv, (d, w))
        self.n_pass += 1 if live else 0
        self.n_null += 1 if null else 0
        return d, w

    def other(self, kind, rid, ts, acq=1, fl=0, rt=0, pv=0):
        """An exit (1), a block outside the engine (2) or a revoke (3): straight to the oracle."""
        if kind != 1:
            self.entered.add(rid)
        self._drive(kind, rid, ts, acq, fl, rt, pv)
        self._record(kind, rid, ts, acq, fl, rt, pv, (0, 0))

    # ---- streams
    def pop_exits(self, now=None):
        while self.heap and (now is None or self.heap[0][0] <= now):
            te, _, rid, acq, fl, rt, pv = heapq.heappop(self.heap)
            self.other(1, rid, te, acq, fl, rt, pv)

    def pop_one(self):
        te, _, rid, acq, fl, rt, pv = heapq.heappop(self.heap)
        self.other(1, rid, te, acq, fl, rt, pv)
        return rid

    def step(self, rid, now, ts, acq=1, rt=0, prio=0, hp=0, pv=0, inb=0, err=0, pop=True):
        """Exits due by `now` (pop), then an entry stamped ts; a passed entry exits at ts + rt."""
        if pop:
            self.pop_exits(now)
        d, w = self.entry(rid, ts, acq, prio, hp, pv, inb)
        if d in (0, 4):
            fl = (2 if err else 0) | (4 if hp else 0) | (8 if inb else 0)
            heapq.heappush(self.heap, (ts + rt, self.seq, rid, acq, fl, rt, pv))
            self.seq += 1
        return d, w

    def generate(self, n_entries, seed, t0, weights, *, gap_mean=2.0, acq_max=2, rt_max=39, regress_pct=0.0,
                 warm=0, warm_weights=None, inbound=False, prio_pct=0.0, err_pct=0.0, params=0, param_res=()):
        """As local_trace.generate: n_entries entries on resources drawn by `weights` (the first `warm` by
        warm_weights), exponential gaps, acquire 1..acq_max, rt 0..rt_max, regress_pct of the entries stamped
        up to 800 ms back.  Pending exits stay pending: flush() ends the stream."""
        rng = np.random.default_rng(seed)
        w = np.asarray(weights, float)
        w = w / w.sum()
        res = rng.choice(len(w), size=n_entries, p=w)
        if warm:
            ww = np.asarray(warm_weights, float)
            res[:warm] = rng.choice(len(ww), size=warm, p=ww / ww.sum())
        gaps = rng.exponential(gap_mean, size=n_entries)
        t = float(getattr(self, "t", t0))
        for i in range(n_entries):
            t += gaps[i]
            now = int(t)
            ts = now
            if regress_pct and rng.random() < regress_pct:
                ts = now - int(rng.integers(1, 800))
            rid = int(res[i])
            acq = int(rng.integers(1, acq_max + 1))
            prio = prio_pct > 0 and rng.random() < prio_pct
            hp = params > 0 and rid in param_res and rng.random() < 0.9
            pv = int(rng.integers(0, params)) if hp else 0
            err = err_pct > 0 and rng.random() < err_pct
            self.step(rid, now, ts, acq, int(rng.integers(0, rt_max + 1)), prio, hp, pv, 1 if inbound else 0, err)
        self.t = t

    def flush(self):
        self.pop_exits(None)

    def mark(self):
        return len(self.ev)

    def stream(self, a=0, b=None):
        """(stream, expected decisions, expected waits) of events [a, b)."""
        ev = self.ev[a:b]
        x = np.array(ev, dtype=np.int64).reshape(-1, 7)
        st = {"kind": x[:, 0].astype(np.uint8), "resource": x[:, 1].astype(np.uint32), "ts": x[:, 2].copy(),
              "acquire": x[:, 3].astype(np.int32), "flags": x[:, 4].astype(np.uint8), "rt": x[:, 5].copy(),
              "param": x[:, 6].astype(np.uint64)}
        e = np.array(self.exp[a:b], dtype=np.int64).reshape(-1, 2)
        return st, e[:, 0].astype(np.int8), e[:, 1].astype(np.int32)

    def counts(self):
        return {"blocks": self.n_block, "passes": self.n_pass, "null": self.n_null}

    def node(self, rid, now):
        return self.orc.node(rid, now)

    def close(self):
        self.orc.close()
