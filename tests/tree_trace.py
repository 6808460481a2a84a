"""TEST INFRASTRUCTURE: expected values for events that carry a context and the enclosing entry (the invocation tree).

tests/context_trace.py mirrors every (resource, context) pair's DefaultNode in a shadow oracle instance.  This helper
keeps, beside it, each event's parent -- the resource of the entry that encloses it in its context, or ENTRANCE --
and restates the one thing the tree adds to those nodes, the edge:

  * NodeSelectorSlot.entry (NodeSelectorSlot.java:158-177) creates the pair's DefaultNode at its first kind 0 / 2 / 3
    event and, then only, calls ((DefaultNode) context.getLastNode()).addChild(node).  Later entries of the pair
    under another parent add no edge.
  * context.getLastNode() (Context.java:180-186, CtEntry.java:157-159) is the enclosing entry's node, or the
    context's EntranceNode when there is none: an edge to a parent that had no DefaultNode in this context before
    the child's birth resolves to ENTRANCE (a self-parent and a parent born later included).
  * EntranceNode's getters (EntranceNode.java:45-126) are sums over its direct children; Constants.ROOT is an
    EntranceNode over the contexts' EntranceNodes.  Children are taken in ascending resource id, contexts in
    ascending id (the reference's order is a HashSet's), doubles summed sequentially in that order.

Decisions, waits and every node's counts are ContextTrace's, unchanged: the parent changes none of them.
"""
import functools
import heapq

import numpy as np

from tests import context_trace as ct
from tests import local_trace as lt

ENTRANCE = 0xFFFFFFFF
ROOT_NAME = "machine-root"
G = {g: k for k, g in enumerate(lt.NODE_GETTERS)}


def entrance_getters(children, max_rt=5000):
    """EntranceNode's getters, in lt.NODE_GETTERS order, over its direct children's getter lists in the given
    order.  The overridden ones are sums (avgRt the passQps-weighted mean, divided by 1 when no child passes);
    the others read a StatisticNode nothing adds to: zeros, minRt = statistic_max_rt, maxSuccessQps = 1 * 2 / 1."""
    total = total_qps = 0.0
    out = [0.0 if g.endswith("qps") or g in ("avg_rt", "min_rt") else 0 for g in lt.NODE_GETTERS]
    for c in children:
        total += c[G["avg_rt"]] * c[G["pass_qps"]]
        total_qps += c[G["pass_qps"]]
        for g in ("block_qps", "success_qps", "pass_qps", "total_pass", "total_block", "cur_thread_num"):
            out[G[g]] += c[G[g]]
    out[G["avg_rt"]] = total / (1 if total_qps == 0 else total_qps)
    out[G["min_rt"]] = float(max_rt)
    out[G["max_success_qps"]] = 2.0
    return out


def resolve(births):
    """{(resource, context): parent} from {(resource, context): (birth sequence, birth parent)}: the birth parent
    stands when its pair in the same context was born strictly earlier, else ENTRANCE."""
    out = {}
    for (rid, c), (seq, p) in births.items():
        pb = births.get((p, c))
        out[(rid, c)] = p if p != ENTRANCE and pb is not None and pb[0] < seq else ENTRANCE
    return out


def expected_tree(edges, views, res_names, ctx_names, max_rt=5000):
    """(name, getters, entrance, children) from ROOT down: `views` {(resource, context): getters} at one query
    time, `edges` as resolve() gives them."""
    def node(rid, c):
        kids = [node(r, c) for (r, cc), p in sorted(edges.items()) if cc == c and p == rid]
        return (res_names[rid], views[(rid, c)], False, kids)

    contexts = []
    for c in sorted({c for _, c in edges}):
        top = [node(r, c) for (r, cc), p in sorted(edges.items()) if cc == c and p == ENTRANCE]
        contexts.append((ctx_names[c - 1], entrance_getters([t[1] for t in top], max_rt), True, top))
    return (ROOT_NAME, entrance_getters([t[1] for t in contexts], max_rt), True, contexts)


class TreeTrace(ct.ContextTrace):
    def __init__(self, *a, **kw):
        self.px = []      # per event: its parent
        self.births = {}  # (resource, context): (sequence of the pair's first kind 0 / 2 / 3 event, its parent)
        self.reparented = set()  # pairs entered again under a parent other than their birth parent
        super().__init__(*a, **kw)

    def _note(self, kind, rid, c, p):
        seq = len(self.px)
        self.px.append(p)
        if not c or kind == 1:
            return
        if (rid, c) not in self.births:
            self.births[(rid, c)] = (seq, p)
        elif kind == 0 and self.births[(rid, c)][1] != p:
            self.reparented.add((rid, c))

    def entry(self, rid, o, ts, acq=1, prio=0, hp=0, pv=0, inb=0, c=0, p=ENTRANCE):
        self._note(0, rid, c, p)
        return super().entry(rid, o, ts, acq, prio, hp, pv, inb, c)

    def other(self, kind, rid, o, ts, acq=1, fl=0, rt=0, pv=0, c=0, p=ENTRANCE):
        self._note(kind, rid, c, p)
        super().other(kind, rid, o, ts, acq, fl, rt, pv, c)

    def step(self, rid, o, now, ts, acq=1, rt=0, hp=0, pv=0, inb=0, err=0, c=0, p=ENTRANCE):
        self.pop_exits(now)
        d, w = self.entry(rid, o, ts, acq, 0, hp, pv, inb, c, p)
        if d in (0, 4):
            fl = (2 if err else 0) | (4 if hp else 0) | (8 if inb else 0)
            heapq.heappush(self.heap, (ts + rt, self.seq, rid, o, acq, fl, rt, pv, c))
            self.seq += 1
        return d, w

    def generate(self, n_entries, seed, t0, weights, origin_weights, context_weights, *, gap_mean=2.0, acq_max=2,
                 rt_max=39, regress_pct=0.0, err_pct=0.0, nest_pct=0.75, depth=4):
        """ContextTrace.generate with a small stack of open entries per context: an entry is nested, with
        probability nest_pct, in the context's most recent entry that is still open (its parent is that entry's
        resource), else it is outermost; a passed entry is pushed while the stack holds fewer than `depth`."""
        rng = np.random.default_rng(seed)
        w = np.asarray(weights, float)
        res = rng.choice(len(w), size=n_entries, p=w / w.sum())
        ow = np.asarray(origin_weights, float)
        org = rng.choice(len(ow), size=n_entries, p=ow / ow.sum())
        cw = np.asarray(context_weights, float)
        ctx = rng.choice(len(cw), size=n_entries, p=cw / cw.sum())
        gaps = rng.exponential(gap_mean, size=n_entries)
        stacks = {}
        t = float(t0)
        for i in range(n_entries):
            t += gaps[i]
            now = int(t)
            ts = now
            if regress_pct and rng.random() < regress_pct:
                ts = now - int(rng.integers(1, 800))
            rid, c = int(res[i]), int(ctx[i])
            err = err_pct > 0 and rng.random() < err_pct
            rt = int(rng.integers(0, rt_max + 1))
            stack = stacks.setdefault(c, [])
            stack[:] = [e for e in stack if e[0] > now]  # exits due by now leave (pop_exits(now) sends them)
            p = stack[-1][1] if c and stack and rng.random() < nest_pct else ENTRANCE
            d, _ = self.step(rid, int(org[i]), now, ts, int(rng.integers(1, acq_max + 1)), rt, 0, 0, 0, err, c, p)
            if d in (0, 4) and c and len(stack) < depth and ts + rt > now:
                stack.append((ts + rt, rid))

    def edges(self):
        return resolve(self.births)

    def stream(self):
        st, ed, ew = super().stream()
        assert len(self.px) == len(ed)
        st["parent"] = np.array(self.px, dtype=np.uint32)
        return st, ed, ew

    def finish(self, times=None, entry=False, max_rt=5000):
        """ContextTrace.finish, plus "edges" {(resource, context): resolved parent}, "births", "reparented", and
        per query time "trees": expected_tree over resource names r0.. and context names c1.. ."""
        self.flush()
        parent = self.stream()[0]["parent"]
        tr = super().finish(times, entry)
        tr["st"]["parent"] = parent
        tr["edges"], tr["births"], tr["reparented"] = self.edges(), dict(self.births), set(self.reparented)
        assert set(tr["edges"]) == set(tr["cnodes"])
        res_names = [f"r{i}" for i in range(self.n_res)]
        ctx_names = [f"c{i + 1}" for i in range(self.n_contexts)]
        tr["trees"] = [expected_tree(tr["edges"], {p: v[k] for p, v in tr["cnodes"].items()}, res_names, ctx_names,
                                     max_rt) for k in range(len(tr["times"]))]
        return tr


def depth_of(edges, c):
    """Levels of DefaultNodes under context c's EntranceNode."""
    def d(rid):
        return 1 + max([d(r) for (r, cc), p in edges.items() if cc == c and p == rid], default=0)
    return max([d(r) for (r, cc), p in edges.items() if cc == c and p == ENTRANCE], default=0)


# ------------------------------------------------------------------ the traces the tree tests share
T0 = 1_700_000_000_000
A, B, C_ = 0, 1, 2


@functools.lru_cache(maxsize=None)
def hand_trace():
    """Contexts c1, c2 and resources A, B, C, no rules.  In c1: A outermost, B under A, C under B, then B again
    under C (no new edge); in c2: B outermost.  A's entry exits after 10 ms, c2's B after 30 ms.
    Edges: (A, c1) -> ENTRANCE, (B, c1) -> A, (C, c1) -> B, (B, c2) -> ENTRANCE."""
    h = TreeTrace(3, 0, 2)
    h.entry(A, 0, T0 + 1, c=1)
    h.entry(B, 0, T0 + 2, c=1, p=A)
    h.entry(C_, 0, T0 + 3, c=1, p=B)
    h.entry(B, 0, T0 + 4, c=1, p=C_)
    h.entry(B, 0, T0 + 5, c=2)
    h.other(1, A, 0, T0 + 11, 1, 0, 10, c=1)
    h.other(1, B, 0, T0 + 35, 1, 0, 30, c=2)
    return h.finish(times=[T0 + 40])


PARITY_SEED = 1
PARITY_RES, PARITY_ORG, PARITY_CTX = 8, 2, 3
PARITY_FLOW = [{"resource": 0, "count": 60},
               {"resource": 1, "count": 80, "control_behavior": 1, "warm_up_period_sec": 3},
               {"resource": 2, "count": 120, "control_behavior": 2, "max_queueing_time_ms": 30},
               {"resource": 3, "count": 90, "control_behavior": 3, "warm_up_period_sec": 2, "max_queueing_time_ms": 20},
               {"resource": 4, "count": 6, "grade": 0},
               {"resource": 7, "count": 30, "strategy": 2, "ref": 1}, {"resource": 7, "count": 40}]


@functools.lru_cache(maxsize=None)
def parity_trace(seed=PARITY_SEED):
    """About 20,000 events: 8 resources under the four controllers, a thread rule and a CHAIN rule, 3 contexts and
    none, 2 origins and none, 2 % of the entries stamped back in time."""
    h = TreeTrace(PARITY_RES, PARITY_ORG, PARITY_CTX, PARITY_FLOW)
    h.generate(14000, seed, T0, [3, 2, 2, 2, 1, 2, 2, 2], [2, 2, 1], [1, 3, 2, 2], gap_mean=1.0, acq_max=2, rt_max=39,
               regress_pct=0.02, err_pct=0.1)
    return h.finish()


def coverage(tr):
    """The three properties the parity trace must have, as (name, holds) pairs."""
    deep = all(depth_of(tr["edges"], c) >= 2 for c in range(1, PARITY_CTX + 1))
    differ = False
    for tree in tr["trees"]:
        for ctx in tree[3]:
            kids = [(k[1][G["pass_qps"]], k[1][G["avg_rt"]]) for k in ctx[3] if k[1][G["pass_qps"]] != 0]
            differ = differ or (len(kids) >= 2 and len({rt for _, rt in kids}) >= 2)
    return [("every context at least two levels deep", deep),
            ("a pair re-entered under a different parent", bool(tr["reparented"])),
            ("an EntranceNode with two passing children of different avgRt", differ)]
