"""TEST INFRASTRUCTURE: expected values for events that carry a caller origin.

The oracle has no notion of an origin, so a stream with origins is decided by driving two oracle instances
event by event:

  * the main instance holds the resources with their `default` rules, parameter rules and breakers;
  * a second, rule-free instance has one resource per (resource, origin) pair.  Its ClusterNode stands for
    that pair's origin node, which StatisticSlot counts next to the resource's ClusterNode
    (StatisticSlot.java:81-84 pass, :123-125 block, :160-161 exit).  A pass of the main instance is a normal
    entry there (nothing can block it), a block a kind-2 event (the BlockException branch: the block count and
    nothing else), exits, kind-2 and kind-3 events are mirrored as they are;
  * a FlowRule with "limit_app" (an origin id, or "other") applies only to entries from that origin -- "other": from
    every origin no rule of the resource names (FlowRuleChecker.java:136-166, FlowRuleManager.java:137-153) -- and
    reads the origin node.  The rules of resource R that apply to origin o are loaded as DIRECT rules on the
    pair's shadow resource, where the shadow entry decides them on the shadow node with their own rater state.
    A block there is mirrored to R as a kind-2 event; a pass goes on to R as a normal entry; if R then blocks,
    the shadow pass is taken back with a kind-3 event at the same time, which nets to the block StatisticSlot
    counts.  FlowRuleComparator puts these rules ahead of R's default ones: a block detail is the index in
    that order;
  * ClusterBuilderSlot creates the origin node at the pair's first kind 0 / 2 / 3 event
    (ClusterBuilderSlot.java:104-107); an exit of a pair without a node leaves the shadow alone.

What the helper cannot model it refuses: parameter rules on a resource with such rules (ParamFlowSlot runs ahead
of FlowSlot, the shadow entry would not), such rules in cluster mode or with a strategy, a prioritized entry
with an origin (PriorityWaitException counts a
thread and no pass on the origin node, StatisticSlot.java:101-104, which a rule-free node cannot restate --
the GPU tests hold a hand-computed case for it).
"""
import heapq

import numpy as np

from tests import local_trace as lt


class OriginTrace:
    def __init__(self, n_res, n_origins, flow_rules=(), param_rules=(), degrade_rules=(), system=None):
        self.n_res, self.n_origins = n_res, n_origins
        self.main = lt.Oracle(n_res, [], list(param_rules), list(degrade_rules))
        self.param_res = {r.get("resource", 0) for r in param_rules}
        if system is not None:
            self.main.system(system)
        self.shadow = lt.Oracle(n_res * n_origins)
        self.L = self.main.L
        self.created = set()
        self.ev = []   # (kind, resource, ts, acquire, flags, rt, param, origin): the stream the engine gets
        self.exp = []  # (decision, wait) per event
        self.heap = []
        self.seq = 0
        self.n_origin_block = self.n_default_block = 0
        self.n_full_pass = {}
        self.load(flow_rules)

    def load(self, flow_rules):
        """FlowRuleManager.loadRules: raters reset on both instances, every node kept."""
        default = [r for r in flow_rules if not r.get("limit_app")]
        self.n_nd, self.smap = {}, {}
        shadow = []
        for rid in range(self.n_res):
            nd = [r for r in flow_rules if r["resource"] == rid and r.get("limit_app")]
            self.n_nd[rid] = len(nd)
            if not nd:
                continue
            assert rid not in self.param_res, "an origin-ruled resource carries no parameter rules"
            assert all(not r.get("cluster_mode") and not r.get("strategy") for r in nd)
            named = {r["limit_app"] for r in nd}
            for o in range(1, self.n_origins + 1):
                ks = [k for k, r in enumerate(nd)
                      if r["limit_app"] == o or (r["limit_app"] == "other" and o not in named)]
                self.smap[(rid, o)] = ks
                for k in ks:
                    d = {x: v for x, v in nd[k].items() if x != "limit_app"}
                    d["resource"] = self.sid(rid, o)
                    shadow.append(d)
        self.main.load(flow_rules=default)
        self.shadow.load(flow_rules=shadow)

    def sid(self, rid, o):
        return rid * self.n_origins + (o - 1)

    def _drive(self, orc, kind, rid, ts, acq, fl, rt, pv):
        a = [np.array([kind], np.uint8), np.array([rid], np.uint32), np.array([ts], np.int64),
             np.array([acq], np.int32), np.array([fl], np.uint8), np.array([rt], np.int64), np.array([pv], np.uint64)]
        dec = np.zeros(1, np.int8)
        wait = np.zeros(1, np.int32)
        self.L.orc_flow_replay_p(orc.h, 1, *[x.ctypes.data for x in a], dec.ctypes.data, wait.ctypes.data)
        return int(dec[0]), int(wait[0])

    # ---- one event each
    def entry(self, rid, o, ts, acq=1, prio=0, hp=0, pv=0, inb=0):
        assert not (o and prio), "a prioritized entry with an origin is not modelled"
        fl = (1 if prio else 0) | (4 if hp else 0) | (8 if inb else 0)
        ks = self.smap.get((rid, o)) if o else None
        if ks:  # the origin's rules first, on the shadow node
            self.created.add((rid, o))
            ds, ws = self._drive(self.shadow, 0, self.sid(rid, o), ts, acq, 0, 0, 0)
            if ds == 1:
                self._drive(self.main, 2, rid, ts, acq, fl & 8, 0, 0)
                d, w = 1, ks[ws]
                self.n_origin_block += 1
            else:
                assert ds == 0
                d, w = self._drive(self.main, 0, rid, ts, acq, fl, 0, pv)
                assert d != 4
                if d == 0:
                    w += ws
                    self.n_full_pass[o] = self.n_full_pass.get(o, 0) + 1
                else:
                    self._drive(self.shadow, 3, self.sid(rid, o), ts, acq, 0, 0, 0)
                    if d == 1:
                        w += self.n_nd[rid]
                        self.n_default_block += 1
        else:
            d, w = self._drive(self.main, 0, rid, ts, acq, fl, 0, pv)
            if d == 1:
                w += self.n_nd[rid]
            if o:
                self.created.add((rid, o))
                if d == 0:
                    assert self._drive(self.shadow, 0, self.sid(rid, o), ts, acq, 0, 0, 0)[0] == 0
                else:
                    assert d != 4
                    self._drive(self.shadow, 2, self.sid(rid, o), ts, acq, 0, 0, 0)
        self.ev.append((0, rid, ts, acq, fl, 0, pv, o))
        self.exp.append((d, w))
        return d, w

    def other(self, kind, rid, o, ts, acq=1, fl=0, rt=0, pv=0):
        """An exit (1), a block outside the engine (2) or a revoke (3)."""
        self._drive(self.main, kind, rid, ts, acq, fl, rt, pv)
        if o:
            if kind != 1:
                self.created.add((rid, o))
            if (rid, o) in self.created:
                self._drive(self.shadow, kind, self.sid(rid, o), ts, acq, fl & 2, rt, 0)
        self.ev.append((kind, rid, ts, acq, fl, rt, pv, o))
        self.exp.append((0, 0))

    # ---- streams
    def pop_exits(self, now=None):
        while self.heap and (now is None or self.heap[0][0] <= now):
            te, _, rid, o, acq, fl, rt, pv = heapq.heappop(self.heap)
            self.other(1, rid, o, te, acq, fl, rt, pv)

    def step(self, rid, o, now, ts, acq=1, rt=0, hp=0, pv=0, inb=0, err=0):
        """Exits due by `now`, then an entry stamped ts; a passed entry exits at ts + rt with its origin."""
        self.pop_exits(now)
        d, w = self.entry(rid, o, ts, acq, 0, hp, pv, inb)
        if d in (0, 4):
            fl = (2 if err else 0) | (4 if hp else 0) | (8 if inb else 0)
            heapq.heappush(self.heap, (ts + rt, self.seq, rid, o, acq, fl, rt, pv))
            self.seq += 1
        return d, w

    def generate(self, n_entries, seed, t0, weights, origin_weights, *, gap_mean=2.0, acq_max=2, rt_max=39,
                 regress_pct=0.0, inbound=False, err_pct=0.0, params=0, param_res=()):
        """n_entries entries on resources drawn by `weights` from origins drawn by `origin_weights` (index 0: no
        origin), exponential gaps, acquire 1..acq_max, rt 0..rt_max, regress_pct of the entries stamped up to
        800 ms back.  flush() ends the stream."""
        rng = np.random.default_rng(seed)
        w = np.asarray(weights, float)
        res = rng.choice(len(w), size=n_entries, p=w / w.sum())
        ow = np.asarray(origin_weights, float)
        org = rng.choice(len(ow), size=n_entries, p=ow / ow.sum())
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
                      hp, pv, 1 if inbound else 0, err)

    def flush(self):
        self.pop_exits(None)

    def stream(self):
        """(stream with its "origin" column, expected decisions, expected waits)."""
        x = np.array(self.ev, dtype=np.int64).reshape(-1, 8)
        st = {"kind": x[:, 0].astype(np.uint8), "resource": x[:, 1].astype(np.uint32), "ts": x[:, 2].copy(),
              "acquire": x[:, 3].astype(np.int32), "flags": x[:, 4].astype(np.uint8), "rt": x[:, 5].copy(),
              "param": x[:, 6].astype(np.uint64), "origin": x[:, 7].astype(np.uint32)}
        e = np.array(self.exp, dtype=np.int64).reshape(-1, 2)
        return st, e[:, 0].astype(np.int8), e[:, 1].astype(np.int32)

    def node(self, rid, now):
        return self.main.node(rid, now)

    def origin_node(self, rid, o, now):
        """The pair's node getters, or None while the pair has no node."""
        return self.shadow.node(self.sid(rid, o), now) if (rid, o) in self.created else None

    def finish(self, times=None, entry=False):
        """Ends the stream and reads every node once, at each of `times` in order (default: the last timestamp,
        400 ms and 1700 ms later -- inside the same bucket, past the second window).  Returns the trace the
        cases share: stream, expected decisions / waits, {resource: [getters per time]}, {(resource, origin):
        [getters per time]} for the created pairs."""
        self.flush()
        st, ed, ew = self.stream()
        t_end = int(st["ts"].max())
        times = list(times) if times else [t_end, t_end + 400, t_end + 1700]
        rids = list(range(self.n_res)) + ([0xFFFFFFFF] if entry else [])
        nodes = {rid: [self.main.node(rid, t) for t in times] for rid in rids}
        onodes = {p: [self.shadow.node(self.sid(*p), t) for t in times] for p in sorted(self.created)}
        self.close()
        return {"st": st, "ed": ed, "ew": ew, "times": times, "nodes": nodes, "onodes": onodes,
                "counts": {"origin_block": self.n_origin_block, "default_block": self.n_default_block,
                           "full_pass": dict(self.n_full_pass)}}

    def close(self):
        self.main.close()
        self.shadow.close()
