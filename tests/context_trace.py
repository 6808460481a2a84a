"""TEST INFRASTRUCTURE: expected values for events that carry a context (and maybe a caller origin).

tests/origin_trace.py drives a main oracle instance and a shadow instance whose resources stand for the origin
nodes.  This helper adds a second shadow instance with one resource per (resource, context) pair: its
ClusterNode stands for that pair's DefaultNode (NodeSelectorSlot.java:158-177), which receives what the
ClusterNode receives from StatisticSlot -- DefaultNode's overrides count on the DefaultNode and forward to the
ClusterNode.  Everything about origins is OriginTrace's, unchanged.

  * NodeSelectorSlot creates the DefaultNode at the pair's first kind 0 / 2 / 3 event; an exit of a pair without
    a node leaves the context shadow alone.  Context 0 is "no tracked context": nothing is mirrored.
  * A FlowRule with "strategy": 2 (CHAIN) and "ref": c applies only to entries in context c and reads their
    DefaultNode (FlowRuleChecker.java:96-116).  The CHAIN rules of resource R for context c are loaded as DIRECT
    rules on the pair's context-shadow resource and decided there first, with their own rater state: a block is
    mirrored to R (and to the origin shadow) as a kind-2 event; a pass goes on to R as a normal entry, and if R
    then blocks, the shadow pass is taken back with a kind-3 event at the same time, which nets to the block
    StatisticSlot counts.  "ref": None is a context name nobody registered: the rule keeps its place and never
    applies.

What the helper cannot model it refuses:
  * a CHAIN rule listed after a DIRECT or RELATE default rule of the same resource (FlowRuleComparator keeps
    the list order among default-limitApp rules, and the shadow entry decides the CHAIN rules first);
  * a prioritized entry on a resource with CHAIN rules (its occupy counters live on the DefaultNode);
  * CHAIN in cluster mode;
  * CHAIN together with a limitApp, or on a resource that also has limitApp rules.
The GPU tests hold hand-computed cases for those.
"""
import heapq

import numpy as np

from tests import local_trace as lt
from tests import origin_trace as ot


class ContextTrace(ot.OriginTrace):
    def __init__(self, n_res, n_origins, n_contexts, flow_rules=(), param_rules=(), degrade_rules=(), system=None):
        self.n_contexts = n_contexts
        self.cshadow = lt.Oracle(max(1, n_res * n_contexts))
        self.ccreated = set()
        self.cx = []  # per event: its context
        self.rule_pass, self.rule_block = {}, {}  # per CHAIN rule (resource, index): entries it passed / blocked
        self.real_origins = n_origins
        super().__init__(n_res, max(1, n_origins), flow_rules, param_rules, degrade_rules, system)

    def load(self, flow_rules):
        chain = [r for r in flow_rules if r.get("strategy") == 2]
        rest = [r for r in flow_rules if r.get("strategy") != 2]
        self.csmap, self.n_chain = {}, {}
        cshadow = []
        for rid in range(self.n_res):
            mine = [r for r in flow_rules if r["resource"] == rid]
            ch = [r for r in mine if r.get("strategy") == 2]
            self.n_chain[rid] = len(ch)
            if not ch:
                continue
            assert rid not in self.param_res, "a CHAIN-ruled resource carries no parameter rules here"
            assert all(not r.get("limit_app") for r in mine), "CHAIN beside a limitApp is not modelled"
            assert all(not r.get("cluster_mode") for r in ch), "CHAIN in cluster mode is not modelled"
            assert all(r.get("strategy") == 2 for r in mine[:len(ch)]), "CHAIN rules come first in the list"
            for c in range(1, self.n_contexts + 1):
                ks = [k for k, r in enumerate(ch) if r.get("ref") == c]
                self.csmap[(rid, c)] = ks
                for k in ks:
                    d = {x: v for x, v in ch[k].items() if x not in ("strategy", "ref")}
                    d["resource"] = self.csid(rid, c)
                    cshadow.append(d)
        super().load(rest)
        for rid, n in self.n_chain.items():
            if n:
                self.n_nd[rid] = n  # a block detail of the main instance counts the CHAIN rules ahead of it
        self.cshadow.load(flow_rules=cshadow)

    def csid(self, rid, c):
        return rid * self.n_contexts + (c - 1)

    def _mirror(self, rid, c, kind, ts, acq, fl=0, rt=0):
        if kind != 1:
            self.ccreated.add((rid, c))
        if (rid, c) in self.ccreated:
            return self._drive(self.cshadow, kind, self.csid(rid, c), ts, acq, fl, rt, 0)
        return 0, 0

    # ---- one event each
    def entry(self, rid, o, ts, acq=1, prio=0, hp=0, pv=0, inb=0, c=0):
        self.cx.append(c)
        assert not (prio and (c or self.n_chain.get(rid))), "a prioritized entry with a context is not modelled"
        ks = self.csmap.get((rid, c)) if c else None
        if ks:  # the context's CHAIN rules first, on the shadow DefaultNode
            ds, ws = self._mirror(rid, c, 0, ts, acq)
            if ds == 1:
                fl = (4 if hp else 0) | (8 if inb else 0)
                self._drive(self.main, 2, rid, ts, acq, fl & 8, 0, 0)
                if o:
                    self.created.add((rid, o))
                    self._drive(self.shadow, 2, self.sid(rid, o), ts, acq, 0, 0, 0)
                key = (rid, ks[ws])
                self.rule_block[key] = self.rule_block.get(key, 0) + 1
                self.ev.append((0, rid, ts, acq, fl, 0, pv, o))
                self.exp.append((1, ks[ws]))
                return 1, ks[ws]
            assert ds == 0
            for k in ks:
                self.rule_pass[(rid, k)] = self.rule_pass.get((rid, k), 0) + 1
            d, w = super().entry(rid, o, ts, acq, 0, hp, pv, inb)
            if d == 0:
                w += ws
                self.exp[-1] = (d, w)
                self.rule_pass[(rid, -1)] = self.rule_pass.get((rid, -1), 0) + 1
            else:
                self._mirror(rid, c, 3, ts, acq)
                if d == 1:
                    key = (rid, w)
                    self.rule_block[key] = self.rule_block.get(key, 0) + 1
            return d, w
        d, w = super().entry(rid, o, ts, acq, prio, hp, pv, inb)
        if self.n_chain.get(rid):
            key = (rid, w if d == 1 else -1)
            book = self.rule_block if d == 1 else self.rule_pass
            book[key] = book.get(key, 0) + 1
        if c:
            if d == 0:
                assert self._mirror(rid, c, 0, ts, acq)[0] == 0
            else:
                assert d != 4
                self._mirror(rid, c, 2, ts, acq)
        return d, w

    def other(self, kind, rid, o, ts, acq=1, fl=0, rt=0, pv=0, c=0):
        """An exit (1), a block outside the engine (2) or a revoke (3)."""
        self.cx.append(c)
        super().other(kind, rid, o, ts, acq, fl, rt, pv)
        if c:
            self._mirror(rid, c, kind, ts, acq, fl & 2, rt)

    # ---- streams
    def pop_exits(self, now=None):
        while self.heap and (now is None or self.heap[0][0] <= now):
            te, _, rid, o, acq, fl, rt, pv, c = heapq.heappop(self.heap)
            self.other(1, rid, o, te, acq, fl, rt, pv, c)

    def step(self, rid, o, now, ts, acq=1, rt=0, hp=0, pv=0, inb=0, err=0, c=0):
        """Exits due by `now`, then an entry stamped ts; a passed entry exits at ts + rt with its origin and
        context."""
        self.pop_exits(now)
        d, w = self.entry(rid, o, ts, acq, 0, hp, pv, inb, c)
        if d in (0, 4):
            fl = (2 if err else 0) | (4 if hp else 0) | (8 if inb else 0)
            heapq.heappush(self.heap, (ts + rt, self.seq, rid, o, acq, fl, rt, pv, c))
            self.seq += 1
        return d, w

    def generate(self, n_entries, seed, t0, weights, origin_weights, context_weights, *, gap_mean=2.0, acq_max=2,
                 rt_max=39, regress_pct=0.0, inbound=False, err_pct=0.0, params=0, param_res=()):
        """OriginTrace.generate with each entry's context drawn by `context_weights` (index 0: no context)."""
        rng = np.random.default_rng(seed)
        w = np.asarray(weights, float)
        res = rng.choice(len(w), size=n_entries, p=w / w.sum())
        ow = np.asarray(origin_weights, float)
        org = rng.choice(len(ow), size=n_entries, p=ow / ow.sum())
        cw = np.asarray(context_weights, float)
        ctx = rng.choice(len(cw), size=n_entries, p=cw / cw.sum())
        gaps = rng.exponential(gap_mean, size=n_entries)
        t = float(t0)
        for i in range(n_entries):
            t += gaps[i]
            now = int(t)
            ts = now
            if regress_pct and rng.random() < regress_pct:
                ts = now - int(rng.integers(1, 800))
            rid = int(res[i])
            hp = params > 0 and rid in param_res and rng.random() < 0.9
            pv = int(rng.integers(0, params)) if hp else 0
            err = err_pct > 0 and rng.random() < err_pct
            self.step(rid, int(org[i]), now, ts, int(rng.integers(1, acq_max + 1)), int(rng.integers(0, rt_max + 1)),
                      hp, pv, 1 if inbound else 0, err, int(ctx[i]))

    def stream(self):
        st, ed, ew = super().stream()
        assert len(self.cx) == len(ed)
        st["context"] = np.array(self.cx, dtype=np.uint32)
        return st, ed, ew

    def finish(self, times=None, entry=False):
        """OriginTrace.finish, plus "cnodes": {(resource, context): [getters per time]} for the created pairs and
        "rule_pass" / "rule_block": per (resource, rule index in FlowRuleComparator order; -1: the resource's
        default rules together) how many entries of a CHAIN-ruled resource it let pass / blocked."""
        self.flush()
        st, ed, ew = self.stream()
        t_end = int(st["ts"].max())
        times = list(times) if times else [t_end, t_end + 400, t_end + 1700]
        cnodes = {p: [self.cshadow.node(self.csid(*p), t) for t in times] for p in sorted(self.ccreated)}
        tr = super().finish(times, entry)
        tr["st"]["context"] = st["context"]
        tr["cnodes"] = cnodes
        tr["rule_pass"], tr["rule_block"] = dict(self.rule_pass), dict(self.rule_block)
        if not self.real_origins:
            assert not tr["onodes"]
        return tr

    def close(self):
        super().close()
        self.cshadow.close()
