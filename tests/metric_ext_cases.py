"""Shared cases of the metric extension tests (tests/test_metric_ext_host.py, tests/test_metric_ext_gpu.py).

The reference of the sums is add_reference: a Python restatement of MetricEntryCallback / MetricExitCallback behind
StatisticSlot.entry / exit (StatisticSlot.java:65-175) over a call's own input columns and the decision and wait
arrays that same call returned.  Decision parity itself is covered elsewhere; everything here is integer sums, so
every comparison is an equality."""
import ctypes as C

import numpy as np

from tests.block_log_cases import T0

BLOCKS = (1, 2, 3, 5, 6)  # FLOW, PARAM, DEGRADE, SYSTEM, AUTHORITY
PASSES = (0, 4)           # SGA_PASS and SGA_PASS_WAIT: onPass runs in the PriorityWaitException branch too
EV_PRIORITIZED, EV_ERROR = 1, 2
ERANGE, EINVAL = -34, -22

# 1,024 / 1,025: k_lsmall over page-locked memory against the pipeline; 64 the wave, 256 the tile
SEAM_SIZES = [1, 63, 64, 65, 255, 256, 257, 1024, 1025, 4097]
R_ONE, R_PACE, R_FIRST = 0, 1, 8
SEAM_RES = R_FIRST + max(SEAM_SIZES)
RES_FIELDS = ("pass", "pass_events", "success", "exits", "exception", "exception_events", "rt_sum", "rt_max")


def new_acc():
    return {"res": {}, "block": {}}


def add_reference(acc, nres, kind, resource, acquire, flags, rt, decision, wait, origin=None):
    """Adds one call's events to acc: acc["res"][resource] = the eight sums in RES_FIELDS order, acc["block"][(resource,
    origin, decision, detail)] = [sum of acquire, events]."""
    for i in range(len(kind)):
        d, r, k, a = int(decision[i]), int(resource[i]), int(kind[i]), int(acquire[i])
        if d < 0 or r >= nres:  # a refused chunk; an unknown resource has no node, no rules and no callbacks
            continue
        o = int(origin[i]) if origin is not None else 0
        line = acc["res"].setdefault(r, [0] * 8)
        blk = None
        if k == 0:
            if d in PASSES:
                line[0] += a
                line[1] += 1
            elif d in BLOCKS:
                blk = (r, o, d, int(wait[i]))
        elif k == 1:
            line[2] += a
            line[3] += 1
            if int(flags[i]) & EV_ERROR:
                line[4] += a
                line[5] += 1
            line[6] += int(rt[i])
            line[7] = max(line[7], int(rt[i]))
        elif k == 2:
            blk = (r, o, 0, 0)
        elif k == 3:
            blk = (r, o, 0, 0)
            line[0] -= a
            line[1] -= 1
        if blk is not None:
            e = acc["block"].setdefault(blk, [0, 0])
            e[0] += a
            e[1] += 1
    return acc


def expected_res(acc):
    """acc's resource lines as the drain returns them: sorted by resource, all-zero lines left out."""
    return [(r,) + tuple(v) for r, v in sorted(acc["res"].items()) if any(v)]


def expected_block(acc):
    return [k + tuple(v) for k, v in sorted(acc["block"].items())]


def res_tuples(rows):
    return [(int(r["resource"]),) + tuple(int(r[f]) for f in RES_FIELDS) for r in rows]


def block_tuples(rows):
    return [(int(b["resource"]), int(b["origin"]), int(b["decision"]), int(b["detail"]), int(b["block"]),
             int(b["block_events"])) for b in rows]


def stream(n, pattern, acq_hi=3):
    """n events in time order, 400 ms .. 1,100 ms into T0's second, acquire in {1, acq_hi}.  Of every 8 events four
    are entries (one of them always prioritized, another every second round), two exits (one with SGA_EV_ERROR),
    one more entry, and one a kind 2 or a kind 3 event.  Pattern "one": everything on R_ONE, whose rule lets
    about a quarter of the stream pass each second, so passes, flow blocks and priority waits all appear on one
    resource.  Pattern "distinct": a resource of its own for every event (every third with a rule that never
    passes), but the always-prioritized entries, which go to R_PACE (5 a second)."""
    kind = np.zeros(n, np.uint8)
    res = np.zeros(n, np.uint32)
    flags = np.zeros(n, np.uint8)
    rt = np.zeros(n, np.int64)
    ts = T0 + 400 + (np.arange(n, dtype=np.int64) * 700) // max(n, 1)
    acq = np.where((np.arange(n) * 7 // 3) % 2 == 0, 1, acq_hi).astype(np.int32)
    for i in range(n):
        m = i % 8
        res[i] = R_ONE if pattern == "one" else R_FIRST + i
        if m == 2 and (i // 8) % 2:
            flags[i] = EV_PRIORITIZED
        elif m == 3:
            flags[i] = EV_PRIORITIZED
            acq[i] = 1
            if pattern != "one":
                res[i] = R_PACE
        elif m in (4, 5):
            kind[i] = 1
            rt[i] = 3 + i % 5
            if m == 5:
                flags[i] = EV_ERROR
        elif m == 7:
            kind[i] = 2 if (i // 8) % 2 else 3
            acq[i] = 1
    return {"kind": kind, "resource": res, "ts": ts, "acquire": acq, "flags": flags, "rt": rt,
            "param": np.zeros(n, np.uint64)}


def rules(n):
    """FlowRules of the streams as (resource id, count)."""
    return [(R_ONE, float(max(5, n // 4))), (R_PACE, 5.0)] + [(R_FIRST + i, 0.0) for i in range(0, n, 3)]


def drain_raw(s, res_cap, block_cap):
    """sga_metric_ext_drain with explicit caps: (rc, n_res, n_block, res_rows, block_rows, lost_events, lost_count)."""
    from sentinel_amd import _lib
    from sentinel_amd.metric_extension import METRIC_BLOCK_ROW_DTYPE, METRIC_RES_ROW_DTYPE
    res = np.zeros(max(1, res_cap), dtype=METRIC_RES_ROW_DTYPE)
    blk = np.zeros(max(1, block_cap), dtype=METRIC_BLOCK_ROW_DTYPE)
    nr, nb, le, lc = C.c_size_t(), C.c_size_t(), C.c_uint64(), C.c_int64()
    rc = _lib.load().sga_metric_ext_drain(s.engine.handle, res.ctypes.data, res_cap, C.byref(nr), blk.ctypes.data,
                                          block_cap, C.byref(nb), C.byref(le), C.byref(lc))
    return (rc, int(nr.value), int(nb.value), res[:min(int(nr.value), res_cap)], blk[:min(int(nb.value), block_cap)],
            int(le.value), int(lc.value))


def make_res_rows(items):
    """A METRIC_RES_ROW_DTYPE array from (resource, pass, pass_events, success, exits, exception, exception_events,
    rt_sum, rt_max)."""
    from sentinel_amd.metric_extension import METRIC_RES_ROW_DTYPE
    rows = np.zeros(len(items), dtype=METRIC_RES_ROW_DTYPE)
    for r, it in zip(rows, items):
        r["resource"] = it[0]
        for f, v in zip(RES_FIELDS, it[1:]):
            r[f] = v
    return rows


def make_block_rows(items):
    """A METRIC_BLOCK_ROW_DTYPE array from (resource, origin, decision, detail, block, block_events)."""
    from sentinel_amd.metric_extension import METRIC_BLOCK_ROW_DTYPE
    rows = np.zeros(len(items), dtype=METRIC_BLOCK_ROW_DTYPE)
    for r, it in zip(rows, items):
        r["resource"], r["origin"], r["decision"], r["detail"], r["block"], r["block_events"] = it
    return rows


class StubSentinel:
    """What metric_extension.dispatch needs of a sentinel, with hand-made tables: no engine."""
    _PARAM_TEXTS_MAX = 16

    def __init__(self, resources, origins, rules=None):
        self.resources, self.origins = list(resources), list(origins)
        self.rules = dict(rules or {})  # {(decision, resource id, detail): rule object}
        self.param_texts = {}

    def block_rule(self, decision, resource, detail):
        return self.rules.get((decision, resource, detail))


class Recorder:
    """Mixin: every call as (method name, positional args, sorted keyword items)."""

    def __init__(self):
        self.calls = []

    def _rec(self, name, *a, **kw):
        self.calls.append((name, a, tuple(sorted(kw.items()))))
