"""Shared cases of the block-log tests (tests/test_block_log_host.py, tests/test_block_log_gpu.py).

The reference of the aggregation is reference_rows: a Python dict over a call's own input columns and the decision
and wait arrays that same call returned -- (time_slot, resource, decision, detail, origin, tag_kind, tag) ->
[sum of acquire, entries] for the caller's entries that ended in a BlockException.  Decision parity itself is
covered elsewhere."""
import ctypes as C

import numpy as np

T0 = 1_700_000_000_000  # 2023-11-14 22:13:20 UTC, a whole second
STAMP = "2023-11-14 22:13:20"
BLOCKS = (1, 2, 3, 5, 6)  # FLOW, PARAM, DEGRADE, SYSTEM, AUTHORITY; 4 is SGA_PASS_WAIT: no BlockException
SEAM_SIZES = [1, 63, 64, 65, 256, 257, 1024, 1025, 4097]  # <= 1024: k_lsmall over page-locked memory; above: pipeline

# resources of the seam streams
R_HOT, R_PACE, R_FREE, R_FIRST = 0, 1, 2, 8  # count-0 rule; count-5 rule; no rule; first of the distinct count-0 ones
SEAM_RES = R_FIRST + max(SEAM_SIZES)


def add_reference(acc, kind, resource, ts, acquire, decision, wait, origin=None, tags=None):
    """Adds one call's blocks to acc.  tags: {event index: (tag_kind, tag)} for SGA_BLOCK_PARAM events."""
    for i in range(len(kind)):
        d = int(decision[i])
        if int(kind[i]) != 0 or d not in BLOCKS:
            continue
        t = int(ts[i])
        tk, tg = (tags or {}).get(i, (0, 0))
        key = (t - t % 1000, int(resource[i]), d, int(wait[i]), int(origin[i]) if origin is not None else 0, tk, tg)
        e = acc.setdefault(key, [0, 0])
        e[0] += int(acquire[i])
        e[1] += 1
    return acc


def as_tuples(rows):
    """Drained rows as (key..., count, events) tuples in the order they came back."""
    return [(int(r["time_slot"]), int(r["resource"]), int(r["decision"]), int(r["detail"]), int(r["origin"]),
             int(r["tag_kind"]), int(r["tag"]), int(r["count"]), int(r["events"])) for r in rows]


def expected_tuples(acc, lo=None, hi=None):
    """acc in the drain's order: sorted by (time_slot, resource, decision, detail, origin, tag_kind, tag);
    lo <= time_slot < hi when given."""
    return [k + (v[0], v[1]) for k, v in sorted(acc.items())
            if (lo is None or k[0] >= lo) and (hi is None or k[0] < hi)]


def seam_stream(n, pattern):
    """n events in time order, 400 ms .. 1,100 ms into T0's second (so they straddle 999 / 1000 ms), acquire in
    {1, 3}.  Of every 8 events five are entries that block -- on R_HOT (pattern "one": one key per second) or on a
    resource of their own (pattern "distinct") -- one an entry on R_PACE (5 a second: passes, blocks, and prioritized
    ones that may wait, SGA_PASS_WAIT), one an entry or an exit on R_FREE, one a kind 2 event on R_HOT or a kind 3
    event on R_FREE."""
    kind = np.zeros(n, np.uint8)
    res = np.zeros(n, np.uint32)
    flags = np.zeros(n, np.uint8)
    rt = np.zeros(n, np.int64)
    ts = T0 + 400 + (np.arange(n, dtype=np.int64) * 700) // max(n, 1)
    acq = np.where((np.arange(n) * 7 // 3) % 2 == 0, 1, 3).astype(np.int32)
    for i in range(n):
        m = i % 8
        if m < 5:
            res[i] = R_HOT if pattern == "one" else R_FIRST + i
        elif m == 5:
            res[i] = R_PACE
            flags[i] = 1 if (i // 8) % 2 else 0  # SGA_EV_PRIORITIZED
            acq[i] = 1
        elif m == 6:
            res[i] = R_FREE
            kind[i] = (i // 8) % 2  # entry, then its exit
            acq[i] = 1
            rt[i] = 3
        else:
            kind[i] = 2 if (i // 8) % 2 else 3
            res[i] = R_HOT if kind[i] == 2 else R_FREE
            acq[i] = 1
    return {"kind": kind, "resource": res, "ts": ts, "acquire": acq, "flags": flags, "rt": rt,
            "param": np.zeros(n, np.uint64)}


def seam_rules(n):
    """FlowRules of the seam streams as (resource id, count): R_HOT and the distinct resources never pass."""
    return [(R_HOT, 0.0), (R_PACE, 5.0)] + [(R_FIRST + i, 0.0) for i in range(n)]


def drain_raw(s, before_ms, cap):
    """sga_block_log_drain with an explicit cap: (rc, n, rows, lost_events, lost_count)."""
    from sentinel_amd import _lib
    from sentinel_amd.block_log import BLOCK_ROW_DTYPE
    out = np.zeros(max(1, cap), dtype=BLOCK_ROW_DTYPE)
    n, le, lc = C.c_size_t(), C.c_uint64(), C.c_int64()
    rc = _lib.load().sga_block_log_drain(s.engine.handle, int(before_ms), out.ctypes.data, cap, C.byref(n),
                                         C.byref(le), C.byref(lc))
    return rc, int(n.value), out[:min(int(n.value), cap)], int(le.value), int(lc.value)


class StubSentinel:
    """What BlockLogWriter needs of a sentinel, with hand-made tables: no engine."""

    def __init__(self, resources, origins, rules, param_texts=None):
        self.resources, self.origins = list(resources), list(origins)
        self.rules = rules  # {(decision, resource id, detail): rule object}
        self.param_texts = dict(param_texts or {})
        self.pending = []   # [(rows, lost_events, lost_count)] handed out by block_rows in order

    def block_rule(self, decision, resource, detail):
        return self.rules.get((decision, resource, detail))

    def block_rows(self, before_ms=None):
        return self.pending.pop(0)


def make_rows(items):
    """A BLOCK_ROW_DTYPE array from (time_slot, resource, decision, detail, origin, tag_kind, tag, count, events)."""
    from sentinel_amd.block_log import BLOCK_ROW_DTYPE
    rows = np.zeros(len(items), dtype=BLOCK_ROW_DTYPE)
    for r, it in zip(rows, items):
        (r["time_slot"], r["resource"], r["decision"], r["detail"], r["origin"], r["tag_kind"], r["tag"], r["count"],
         r["events"]) = it
    return rows
