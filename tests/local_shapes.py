"""TEST INFRASTRUCTURE: deterministic event streams aimed at the size and time seams of the local path.

flow.hip decides a chunk of local events by about a dozen code paths, picked per resource from its rule shape
and from how many events it has in the chunk (DESIGN.md section 5 has the table).  The builders here put named
resources exactly at those switches -- 127 / 128 / 129 events, a run of 63 / 64 / 65 entries, a flow that ends
at sorted position 4095 / 4096 / 4097, an exit flow of 16383 / 16384 / 16385 events, ... -- instead of leaving
the counts to a seed.  Plain numpy, no GPU: tests/test_local_shapes_host.py checks the shapes against the
arrays and the oracle, tests/test_local_shapes_gpu.py replays them on the engine.

Every builder returns a Case:
  chunks   the engine calls, in order; each one is one submit with max_batch >= its length
  flow / param / degrade   the rules
  table    one row per (targeted resource, chunk): its events in the chunk, its entries per 500 ms run (a run =
           a maximal stretch of the resource's events, in arrival order, inside one 500 ms bucket), the seam the
           resource is there for, and which of pass / block its rule can produce there
  meta     what else the host test recomputes for the case (trip positions, colliding timestamps, ...)

Rules the builders keep (the host test asserts them): exits come from the oracle's decisions -- an entry that
passed (decision 0 or 4) is what a later exit takes its resource, acquire count and parameter from; every chunk
has more than 1024 events unless the case is about the small path; at least 300 rule-free filler resources widen
the sort key past one 8-bit digit; T0 is a multiple of 1000 and every targeted resource has events at
t % 500 == 0, t % 500 == 499 and t % 1000 == 0 and at least two runs per chunk (the single-run resources of
group B say so in their row); a chunk begins in the 500 ms bucket in which the previous one ended.
"""
from fractions import Fraction

import numpy as np

from tests import local_trace as lt

T0 = 1_700_000_000_000
EV_PRIO, EV_ERROR, EV_HAS_PARAM, EV_INBOUND = 1, 2, 4, 8
ALL_ONES = 0xFFFFFFFFFFFFFFFF
ENTRY_NODE = 0xFFFFFFFF
N_FILLER = 320
COLS = ("kind", "resource", "ts", "acquire", "flags", "rt", "param")
DTYPES = {"kind": np.uint8, "resource": np.uint32, "ts": np.int64, "acquire": np.int32, "flags": np.uint8,
          "rt": np.int64, "param": np.uint64}
# the switches of flow.hip / flow.hpp the cases are aimed at (restated: a test must not read them from the code
# it checks)
K_SMALL, K_WAVE, K_HEAVY, K_PSEG_LONG, K_CB_SHORT, K_CB_ROUND, K_CB_TILE_MIN = 1024, 128, 1024, 64, 4096, 8192, 16384
K_TILE, K_EN_TILE, K_EN_BUCKETS = 4096, 1024, 64
FORM_KEYS = ("heavy", "wave", "lru", "pseg", "segments", "long", "cb", "groups", "tiled", "small", "events", "chunks")


def events(kind, res, ts, acq=1, flags=0, rt=0, param=0):
    ts = np.asarray(ts, np.int64)
    n = len(ts)
    vals = {"kind": kind, "resource": res, "ts": ts, "acquire": acq, "flags": flags, "rt": rt, "param": param}
    return {k: np.ascontiguousarray(np.broadcast_to(np.asarray(vals[k], DTYPES[k]), (n,))).copy() for k in COLS}


def concat(parts):
    parts = [p for p in parts if len(p["kind"])]
    if not parts:
        return events(0, 0, [])
    return {k: np.concatenate([p[k] for p in parts]) for k in COLS}


def arrival(st):
    """Time order, exits before entries at equal time, otherwise the order given (stable)."""
    o = np.lexsort((1 - st["kind"].astype(np.int64), st["ts"]))
    return {k: np.ascontiguousarray(v[o]) for k, v in st.items()}


def offsets(n, lo=0, hi=499, burst=25):
    """n non-decreasing offsets in [lo, hi], the first at lo and the last at hi, the others in bursts at multiples
    of `burst` ms (several entries per millisecond: a rate limit both passes and blocks)."""
    if n <= 0:
        return np.zeros(0, np.int64)
    if n == 1:
        return np.array([lo], np.int64)
    o = lo + (np.arange(n, dtype=np.int64) * (hi - lo)) // (n - 1)
    if burst > 1:
        o = np.maximum(o // burst * burst, lo)
    o[0], o[-1] = lo, hi
    return o


def frame(b0, nb):
    """The run windows of a chunk that starts at offset 250 of bucket b0 and ends at offset 249 of bucket
    b0 + nb: [(bucket, lo, hi)].  The next chunk's frame starts at b0 + nb: in the bucket this one ended in."""
    return [(b0, 250, 499)] + [(b, 0, 499) for b in range(b0 + 1, b0 + nb)] + [(b0 + nb, 0, 249)]


def run_ts(windows, counts, burst=25):
    """Timestamps of counts[i] entries in windows[i]."""
    return np.concatenate([T0 + 500 * b + offsets(c, lo, hi, burst) for (b, lo, hi), c in zip(windows, counts)]
                          + [np.zeros(0, np.int64)])


def spread(total, n):
    """total split into n near-equal parts, each at least 2 (first and last offset of a run)."""
    q, r = divmod(total, n)
    out = [q + (1 if i < r else 0) for i in range(n)]
    assert min(out) >= 2, (total, n)
    return out


def filler(first_res, n, t_lo, t_hi):
    """n entries over the N_FILLER rule-free resources from first_res on, a few each, spread over [t_lo, t_hi]."""
    i = np.arange(n, dtype=np.int64)
    return events(0, first_res + i % N_FILLER, t_lo + (i * (t_hi - t_lo)) // max(n - 1, 1))


class Case:
    def __init__(self, name, n_targets, flow=(), param=(), degrade=()):
        self.name = name
        self.first_filler = n_targets
        self.n_res = n_targets + N_FILLER
        self.flow, self.param, self.degrade = list(flow), list(param), list(degrade)
        self.chunks, self.table, self.meta = [], [], {}
        self.max_batch = None      # engine max_batch (default: the longest chunk)
        self.small_ok = False      # group F: chunks of at most 1024 events are the point
        self.entry_node = False    # group E: ENTRY_NODE is compared too
        self.sorted_chunks = True  # chunks are in time order (group E and F build regressions on purpose)

    @property
    def targets(self):
        return sorted({r["res"] for r in self.table})

    def row(self, res, chunk, events_, run_entries, seam, can=("pass", "block"), single_run=False):
        self.table.append({"res": res, "chunk": chunk, "events": int(events_), "run_entries": list(run_entries),
                           "seam": seam, "can": tuple(can), "single_run": single_run})

    def oracle(self):
        return lt.Oracle(self.n_res, self.flow, self.param, self.degrade)


class Stage:
    """Builds a case's chunks against a generating oracle: the entries that pass queue up per resource, and an
    exit is always taken from that queue (oldest first)."""

    def __init__(self, case):
        self.case = case
        self.gen = case.oracle()
        self.pending = {}

    def npending(self, res):
        return len(self.pending.get(res, ()))

    def exits(self, res, ts, rt=None, err=None):
        """Exits of the oldest len(ts) passed entries of res at ts; rt defaults to the time since the entry."""
        ts = np.asarray(ts, np.int64)
        q = self.pending.get(res, [])
        k = len(ts)
        assert k <= len(q), (res, k, len(q))
        take = q[:k]
        del q[:k]
        if k == 0:
            return events(1, res, ts)
        ets = np.array([e[0] for e in take], np.int64)
        fl = np.array([e[2] & (EV_HAS_PARAM | EV_INBOUND) for e in take], np.uint8)
        if err is not None:
            fl = fl | (np.asarray(err, bool).astype(np.uint8) * EV_ERROR)
        return events(1, res, ts, acq=[e[1] for e in take], flags=fl,
                      rt=np.maximum(ts - ets, 1) if rt is None else rt, param=[e[3] for e in take])

    def add(self, parts, sort=True):
        # "_key": the time a part's events are sorted by, where it is not their timestamp (a clock that goes back)
        key = [p.get("_key", p["ts"]) for p in parts if len(p["kind"])]
        st = concat(parts)
        if sort and key:
            o = np.lexsort((1 - st["kind"].astype(np.int64), np.concatenate(key)))
            st = {k: np.ascontiguousarray(v[o]) for k, v in st.items()}
        dec, _ = self.gen.replay(st)
        for i in np.nonzero((st["kind"] == 0) & ((dec == 0) | (dec == 4)))[0]:
            self.pending.setdefault(int(st["resource"][i]), []).append(
                (int(st["ts"][i]), int(st["acquire"][i]), int(st["flags"][i]), int(st["param"][i])))
        self.case.chunks.append(st)
        return st, dec

    def drain(self, t_lo, t_hi, skip_filler=True):
        """The exits of every entry still in flight, at t_lo .. t_hi (filler entries stay in flight)."""
        parts = []
        for res in sorted(self.pending):
            n = self.npending(res)
            if n == 0 or (skip_filler and res >= self.case.first_filler):
                continue
            parts.append(self.exits(res, t_lo + (np.arange(n, dtype=np.int64) * (t_hi - t_lo)) // max(n - 1, 1)))
        return parts

    def close(self):
        self.gen.close()


def counted_row(st, res):
    """(events, entries per run) of `res` counted from a chunk's arrays."""
    m = st["resource"] == res
    bucket = st["ts"][m] // 500
    ent = st["kind"][m] == 0
    if not m.any():
        return 0, []
    cut = np.nonzero(np.diff(bucket) != 0)[0] + 1
    return int(m.sum()), [int(x.sum()) for x in np.split(ent, cut)]


def _auto_rows(case, ci, seams, can=None, single_run=()):
    """Table rows for chunk ci of every resource in seams, their sizes as built (the host test counts again)."""
    for res, seam in seams.items():
        n, runs = counted_row(case.chunks[ci], res)
        if n:
            case.row(res, ci, n, runs, seam, (can or {}).get(res, ("pass", "block")), res in single_run)


# ---------------------------------------------------------------------------------------------- dispatch model
def rule_shape(case, res):
    """(fast bits, n FlowRules, n ParamFlowRules, n DegradeRules) as FlowEngine::upload_res sets them."""
    fr = [r for r in case.flow if r["resource"] == res]
    pr = [r for r in case.param if r["resource"] == res]
    cb = [r for r in case.degrade if r["resource"] == res]
    fast = 0
    if len(fr) == 1 and not pr and not cb and fr[0].get("grade", 1) == 1:
        b = fr[0].get("control_behavior", 0)
        fast = 1 if b in (0, 1) else 4 if b == 2 else 0
    return fast, len(fr), len(pr), len(cb)


def predict_forms(case, ci, cb_state):
    """The dispatch counts the shape of chunk ci predicts (k_lflows restated over the arrays).  cb_state(res):
    the state of the resource's first breaker before the chunk."""
    st = case.chunks[ci]
    n = len(st["kind"])
    out = dict.fromkeys(FORM_KEYS, 0)
    out["events"] = n
    out["chunks"] = 1
    cpc = case.meta.get("chunks_per_call")
    if cpc and cpc[ci] == 2:  # the host cut the call: the read-back is of its tail, one event here
        out.update(small=1, events=1, chunks=2)
        return out
    if n <= K_SMALL:
        out["small"] = 1
        return out
    for res in np.unique(st["resource"]):
        res = int(res)
        m = st["resource"] == res
        nev = int(m.sum())
        fast, nf, npr, ncb = rule_shape(case, res)
        kinds = st["kind"][m]
        ent, ex = bool((kinds == 0).any()), bool((kinds == 1).any())
        if ncb == 1 and not nf and not npr and not (ent and ex):
            out["pseg"] += 1
            state = cb_state(res)
            if not (ent and state == 0):
                out["cb"] += 1
                if nev >= K_CB_TILE_MIN and (ent or state in (0, 1)):
                    out["tiled"] += 1
            continue
        if npr == 1 and not nf and not ncb:
            out["pseg"] += 1
            vals = st["param"][m]
            for v in np.unique(vals):
                s = vals == v
                out["segments"] += 1
                regular = (kinds[s] == 0).all() and len(np.unique(st["acquire"][m][s])) == 1 and \
                    (np.diff(st["ts"][m][s]) >= 0).all()
                if regular and int(s.sum()) >= K_PSEG_LONG:
                    out["long"] += 1
            continue
        if fast == 0 and nev >= K_HEAVY:
            out["heavy"] += 1
        elif fast and nev >= K_WAVE:
            out["wave"] += 1
    return out


# ------------------------------------------------------------------------------------------------------ group A
FAST_SHAPES = [  # name, rule, acquire pattern period, what the rule can do
    ("default", {"count": 20.0}, 1, ("pass", "block")),                       # uniform acquire: the closed form
    ("greedy", {"count": 20.0}, 3, ("pass", "block")),                        # acquire 1..3: k_lwave's greedy windows
    ("warmup", {"count": 30.0, "control_behavior": 1, "warm_up_period_sec": 2}, 3, ("pass", "block")),
    ("rl200", {"count": 200.0, "control_behavior": 2, "max_queueing_time_ms": 20}, 1, ("pass", "block")),
    ("rl_cost0", {"count": 2500.0, "control_behavior": 2, "max_queueing_time_ms": 500}, 1, ("pass",)),
    ("rl_count0", {"count": 0.0, "control_behavior": 2, "max_queueing_time_ms": 20}, 1, ("block",)),
]
# a RateLimiter that passes one entry per 250 ms: every other entry blocks and moves nothing, the interior
# windows of its runs are decided from their summaries.  Cost 250 ms, queue 25 ms, bursts every 25 ms: the entry
# that passes is the first of the burst 225 ms after the last pass time -- it waits exactly the queueing limit,
# and one of the two per run lies deep inside the run (the summary test "no entry of the window can pass" at
# equality)
SATURATED = ("rl_saturated", {"count": 4.0, "control_behavior": 2, "max_queueing_time_ms": 25}, 1, ("pass", "block"))
NONFAST_SHAPES = ["norule", "two_rules", "thread", "warmup_rl", "rules17", "cbs17"]
FAST_SIZES, NONFAST_SIZES = (127, 128, 129), (1023, 1024, 1025, 1535, 1536, 1537)
RUN_ENTRIES = (63, 64, 65, 511, 512, 513, 128)


def _nonfast_rules(shape, res):
    flow, degrade = [], []
    if shape == "two_rules":
        flow = [{"resource": res, "count": 20.0}, {"resource": res, "count": 25.0}]
    elif shape == "thread":
        flow = [{"resource": res, "count": 15.0, "grade": 0}]
    elif shape == "warmup_rl":
        flow = [{"resource": res, "count": 30.0, "control_behavior": 3, "warm_up_period_sec": 2,
                 "max_queueing_time_ms": 20}]
    elif shape == "rules17":  # above kHeavyRules = 16: k_lheavy keeps the rules in global memory
        flow = [{"resource": res, "count": float(20 + k)} for k in range(17)]
    elif shape == "cbs17":  # above kHeavyCbs = 16; the breakers never trip (an RT no exit reaches)
        flow = [{"resource": res, "count": 20.0}]
        degrade = [{"resource": res, "grade": 0, "count": 100000.0 + k, "slow_ratio_threshold": 0.5,
                    "min_request_amount": 5, "stat_interval_ms": 1000, "time_window": 1} for k in range(17)]
    return flow, degrade


def build_a():
    """Lane / wave / heavy.  Chunk 0 warms every resource up (80 entries each), chunk 1 is the chunk under test
    (nine runs per resource; the exits of chunk 0's passes come first in it), chunk 2 takes every exit left."""
    specs = []  # (res, seam, period, can, size or None)
    flow, degrade = [], []
    res = 0
    for name, rule, period, can in FAST_SHAPES:
        for size in FAST_SIZES:
            flow.append(dict(rule, resource=res))
            specs.append((res, f"{name}:{size} lane/wave", period, can, size))
            res += 1
    for shape in NONFAST_SHAPES:
        for size in NONFAST_SIZES:
            f, d = _nonfast_rules(shape, res)
            flow += f
            degrade += d
            specs.append((res, f"{shape}:{size} lane/heavy", 3, ("pass",) if shape == "norule" else ("pass", "block"),
                          size))
            res += 1
    for name, rule, period, can in FAST_SHAPES + [SATURATED]:
        flow.append(dict(rule, resource=res))
        specs.append((res, f"{name}: runs of {RUN_ENTRIES} entries", period, can, None))
        res += 1
    case = Case("A", res, flow=flow, degrade=degrade)
    stg = Stage(case)

    def acq(n, period):
        return 1 + np.arange(n) % period

    w0 = [(0, 0, 499), (1, 0, 200)]
    parts = [events(0, r, run_ts(w0, [40, 40]), acq=acq(80, p)) for r, _, p, _, _ in specs]
    stg.add(parts + [filler(case.first_filler, 1280, T0, T0 + 700)])
    w1 = frame(1, 8)  # buckets 1 (from 250) .. 9 (to 249)
    parts = []
    for r, _, p, _, size in specs:
        if size is not None:
            k = min(stg.npending(r), size // 4)
            counts = spread(size - k, len(w1))
        else:  # the measured runs hold entries only: the exits go into the first run
            k = min(stg.npending(r), 10)
            counts = [8] + list(RUN_ENTRIES) + [8]
        # few entries per run: all of a run's in two bursts, so that a rate limit blocks some of them
        ts = run_ts(w1, counts, burst=25 if size is None or size > 1000 else 250)
        parts += [stg.exits(r, T0 + 750 + offsets(k, 0, 249, 1)), events(0, r, ts, acq=acq(len(ts), p))]
    stg.add(parts + [filler(case.first_filler, 1280, T0 + 750, T0 + 4749)])
    stg.add(stg.drain(T0 + 4850, T0 + 4990) + [filler(case.first_filler, 1280, T0 + 4850, T0 + 4990)])
    stg.close()
    seams = {r: s for r, s, _, _, _ in specs}
    cans = {r: c for r, _, _, c, _ in specs}
    _auto_rows(case, 0, seams, cans)
    _auto_rows(case, 1, seams, cans)
    case.meta["sizes"] = {r: size for r, _, _, _, size in specs if size is not None}
    case.meta["run_resources"] = [r for r, _, _, _, size in specs if size is None]
    return case


# ------------------------------------------------------------------------------------------------------ group B
def build_b():
    """Run segmentation.  Resource 0 sorts first, so its event count is the sorted position at which resource 1
    starts.  Chunks: resource 0 with 4095 / 4096 / 4097 events (resource 1's first run has one event, so its
    second run -- a bucket change inside a flow -- starts one position later: at 4096 in the first chunk); one
    run of 8193 events in one bucket; chunk totals of 8192, 8193, 4096 and 4097 events."""
    flow = [{"resource": 0, "count": 2000.0},
            {"resource": 1, "count": 200.0, "control_behavior": 2, "max_queueing_time_ms": 20},
            {"resource": 2, "count": 20.0}, {"resource": 2, "count": 30.0}]
    case = Case("B", 3, flow=flow)
    stg = Stage(case)
    seams = {0: "flow end / tile seam", 1: "first run at the seam", 2: "two rules behind the seam"}
    plan = [(4095, 8192, False), (4096, 8193, False), (4097, 8192, False), (8193, 8193 + 1400, True),
            (2000, 4096, False), (2001, 4097, False)]
    for ci, (n0, total, one_run) in enumerate(plan):
        w = frame(2 * ci, 2)
        t_lo, t_hi = T0 + 1000 * ci + 250, T0 + 1000 * ci + 1249
        k = min(stg.npending(0), n0 // 3)
        w0 = [w[1]] if one_run else w
        ex_lo = T0 + 500 * w0[0][0] + w0[0][1]
        p0 = [stg.exits(0, ex_lo + offsets(k, 0, 200, 1)),
              events(0, 0, run_ts(w0, [n0 - k] if one_run else spread(n0 - k, 3), burst=5), acq=3 if ci >= 4 else 1)]
        k1 = min(stg.npending(1), 20)
        p1 = [events(0, 1, run_ts(w, [1, 150 - k1, 49])), stg.exits(1, t_lo + 300 + offsets(k1, 0, 100, 1))]
        p2 = [events(0, 2, run_ts(w, [30, 60, 30]), acq=1 + np.arange(120) % 3)]
        nfill = total - n0 - 200 - 120
        assert nfill >= 2 * N_FILLER
        stg.add(p0 + p1 + p2 + [filler(case.first_filler, nfill, t_lo, t_hi)])
        _auto_rows(case, ci, seams, single_run={0} if one_run else ())
    case.meta["plan"] = plan
    stg.close()
    return case


# ------------------------------------------------------------------------------------------------------ group C
PARAM_RULES = [  # name, rule, can
    ("bucket", {"count": 5.0}, ("pass", "block")),
    ("burst", {"count": 5.0, "burst_count": 3}, ("pass", "block")),
    ("throttle", {"count": 20.0, "control_behavior": 2, "max_queueing_time_ms": 150}, ("pass", "block")),
    ("throttle_cost0", {"count": 5000.0, "control_behavior": 2, "max_queueing_time_ms": 0}, ("pass",)),
]
V_SEG = {63: 1, 64: 2, 65: 3, 129: 4}  # regular entry segments: value by length
V_ACQ, V_BACK, V_EX1, V_EX2, V_EX64, V_REFILL, V_QUEUE = 5, 6, 7, 8, 9, 10, 11
HOT = {V_EX1: 100, V_EX2: 100, V_EX64: 100}  # these values pass often enough to have 64 entries in flight


def _param_resource(res):
    """The chunk-1 events of one parameter resource: segments by value."""
    P = EV_HAS_PARAM
    t1 = T0 + 1000  # bucket 2: every regular segment starts on a multiple of 1000
    parts = []
    # the segment of 64 comes first, at T0 + 1000: chunk 0 left the value's lastAddTokenTime at T0 with an empty
    # bucket, so its first entries have passTime == duration (no refill: blocked) and the next burst refills --
    # the refill equality inside a long segment (k_pseg_long's search for the next refill)
    for slot, n in enumerate((64, 63, 65, 129)):
        parts.append(events(0, res, t1 + 500 * slot + offsets(n), flags=P, param=V_SEG[n]))
    # irregular at the 64th entry: another acquire count there; the clock 1 ms back there
    a = np.ones(100, np.int32)
    a[63] = 2
    parts.append(events(0, res, t1 + 2000 + offsets(100), acq=a, flags=P, param=V_ACQ))
    tb = t1 + 2500 + np.arange(100, dtype=np.int64) * 4
    key = tb.copy()
    tb[63] = tb[62] - 1
    key[63] = key[62]  # it arrives right after the 63rd entry
    parts.append(dict(events(0, res, tb, flags=P, param=V_BACK), _key=key))
    # refill equality (token bucket, duration 1 s): six entries at ta (the first sets lastAddTokenTime = ta and the
    # bucket runs dry), then ta + 1000 (passTime == duration: no refill) and ta + 1001 (refill)
    ta = T0 + 760
    parts.append(events(0, res, [ta] * 6 + [ta + 1000, ta + 1001, ta + 1001], flags=P, param=V_REFILL))
    # throttle equality (cost 50 ms, queue 150 ms): entries pile up behind latestPassedTime until one waits
    # exactly 150 ms (blocked: the test is wait < max), then 149 ms and 151 ms
    tq = T0 + 770
    parts.append(events(0, res, [tq, tq, tq, tq, tq + 1, tq + 49, tq + 50, tq + 51], flags=P, param=V_QUEUE))
    # the values 0 and all ones (64 entries of all ones: one more long segment)
    parts.append(events(0, res, t1 + 3000 + offsets(20), flags=P, param=0))
    parts.append(events(0, res, t1 + 3000 + offsets(64), flags=P, param=ALL_ONES))
    return parts


def build_c():
    """Parameter segments.  Resources 0..3: one QPS ParamFlowRule each (PARAM_RULES).  Resource 4: the bucket rule
    beside a FlowRule with at least 1024 events and 1100 distinct values, the all-ones value among them
    (k_lheavy, past its kHeavySlots = 1024 LDS cache); resource 5 the same below 1024 events (its lane)."""
    param = [dict(rule, resource=r, hot=HOT) for r, (_, rule, _) in enumerate(PARAM_RULES)]
    param += [dict(PARAM_RULES[0][1], resource=r, hot=HOT) for r in (4, 5)]
    flow = [{"resource": r, "count": 400.0} for r in (4, 5)]
    case = Case("C", 6, flow=flow, param=param)
    stg = Stage(case)
    P = EV_HAS_PARAM
    # chunk 0: the thread-count maps come to exist, the exit-only values get their entries in flight
    parts = []
    for r in range(6):
        parts.append(events(0, r, T0 + offsets(70, 0, 700, 1), flags=P, param=V_EX64))
        parts.append(events(0, r, T0 + offsets(4, 0, 499, 1), flags=P, param=V_EX2))
        parts.append(events(0, r, T0 + 500 + offsets(3, 0, 200, 1), flags=P, param=V_EX1))
        parts.append(events(0, r, T0 + offsets(12, 0, 499, 500), flags=P, param=V_SEG[64]))
        parts.append(events(0, r, T0 + 500 + offsets(6, 0, 200), flags=P, param=ALL_ONES))
    stg.add(parts + [filler(case.first_filler, 1280, T0, T0 + 700)])
    w1 = frame(1, 8)
    parts = []
    for r in range(6):
        if r < 4:
            parts += _param_resource(r)
        else:
            n = 1100 if r == 4 else 800
            vals = np.arange(n, dtype=np.uint64) + 100
            vals[::50] = ALL_ONES
            vals[1::50] = 0
            parts.append(events(0, r, run_ts(w1, spread(n, len(w1)), burst=5), flags=P, param=vals))
            parts.append(events(0, r, T0 + 1000 + offsets(60), flags=P, param=V_SEG[64]))
        # exit-only segments of 1, 2 and 64 events
        assert stg.npending(r) >= 64 + 2 + 1
        byval = {}
        for i, e in enumerate(stg.pending[r]):
            byval.setdefault(e[3], []).append(i)
        assert len(byval[V_EX64]) >= 64 and len(byval[V_EX2]) >= 2 and len(byval[V_EX1]) >= 1, r
        take = byval[V_EX64][:64] + byval[V_EX2][:2] + byval[V_EX1][:1]
        q = stg.pending[r]
        stg.pending[r] = [q[i] for i in take] + [e for i, e in enumerate(q) if i not in set(take)]
        parts.append(stg.exits(r, T0 + 4000 + offsets(67, 0, 499, 1)))
    stg.add(parts + [filler(case.first_filler, 1280, T0 + 750, T0 + 4749)])
    stg.add(stg.drain(T0 + 4850, T0 + 4990) + [filler(case.first_filler, 1280, T0 + 4850, T0 + 4990)] +
            [events(0, r, T0 + 4900 + offsets(30, 0, 90, 10), flags=P, param=np.arange(30) % 3) for r in range(6)])
    stg.close()
    seams = {r: f"{PARAM_RULES[r][0]}: segments of 63/64/65/129, irregular, exit-only, equalities" for r in range(4)}
    seams[4] = "param + flow rule, k_lheavy, all-ones bypass, > 1024 values"
    seams[5] = "param + flow rule below kHeavyEvents"
    cans = {r: PARAM_RULES[r][2] for r in range(4)}
    _auto_rows(case, 0, seams, cans)
    _auto_rows(case, 1, seams, cans)
    case.meta["regressions"] = {1: 4}  # one per parameter-only resource
    return case


# ------------------------------------------------------------------------------------------------------ group D
def cb_rule(res, grade, thr, min_req=20, stat_ms=1000):
    if grade == 0:  # slow-request ratio: an exit is slow when rt > count
        return {"resource": res, "grade": 0, "count": 50.0, "slow_ratio_threshold": float(thr),
                "min_request_amount": min_req, "stat_interval_ms": stat_ms, "time_window": 2}
    # error ratio (1) or error count (2)
    return {"resource": res, "grade": grade, "count": float(thr), "min_request_amount": min_req,
            "stat_interval_ms": stat_ms, "time_window": 2}


def plan_bad(ts, grade, thr, min_req, stat_ms, trip_at):
    """Which exits are bad so that a CLOSED breaker trips exactly at exit trip_at (None: never): before it as
    many bad exits as keep the window's figure at or under the threshold (so it touches the threshold whenever
    it can), then a bad one.  Returns (bad mask, the exits at which the figure equals the threshold)."""
    n = len(ts)
    bad = np.zeros(n, bool)
    equal = []
    thr = Fraction(thr).limit_denominator(1000)
    win, s, tot = None, 0, 0
    for i in range(n if trip_at is None else trip_at + 1):
        w = int(ts[i]) - int(ts[i]) % stat_ms
        if w != win:
            win, s, tot = w, 0, 0
        tot += 1
        fig = (lambda s_: Fraction(s_, tot)) if grade < 2 else (lambda s_: Fraction(s_))
        if i == trip_at:
            s += 1
            bad[i] = True
            assert tot >= min_req and fig(s) > thr, (i, s, tot, thr)
        elif fig(s + 1) <= thr:
            s += 1
            bad[i] = True
        if i != trip_at and tot >= min_req and fig(s) == thr:
            equal.append(i)
    return bad, equal


def pick_threshold(ts, grade, min_req, stat_ms, trip_at):
    for thr in ([Fraction(1, 2), Fraction(1, 4), Fraction(1, 5), Fraction(1, 8)] if grade < 2 else [Fraction(7)]):
        try:
            plan_bad(ts, grade, thr, min_req, stat_ms, trip_at)
            return thr
        except AssertionError:
            continue
    raise AssertionError(("no threshold trips at", trip_at))


def build_d(which):
    """Breaker-only flows.  Chunk 0: N entries per resource (CLOSED: all pass).  Chunk 1: their N exits, the
    exit-only flows under test, each tripping at its planned exit (or never).  Chunk 2: entries against the OPEN
    breakers -- for the flows that tripped, either an entry exactly at the retry time (the probe) or entries up to
    1 ms before it (all blocked).  Chunk 3: the probes' exits.
    which: "4k" (k_cb_flows<1> / <8>), "8k" (k_cb_flows<8>, two rounds), "16k" (k_cbt_* tiles)."""
    # (events, grade, trip exit or None, min_request_amount or None)
    flows = {
        "4k": [(4095, 0, 1023, None), (4095, 1, 1024, None), (4095, 2, 4094, None),
               (4096, 0, 4095, None), (4096, 1, None, None), (4096, 2, 2047, None),
               (4097, 0, 4096, None), (4097, 1, 3000, None), (4097, 2, None, None),
               (1500, 1, 1023, 1024), (1500, 0, 1024, 1025)],  # all bad: trips when the count reaches the minimum
        "8k": [(8191, 0, 8190, None), (8192, 1, 8191, None), (8193, 2, 8192, None), (8193, 0, 8191, None),
               (8192, 2, None, None)],
        "16k": [(16383, 0, 8192, None), (16384, 1, 8191, None), (16385, 2, 16384, None), (16384, 0, 8192, None)],
    }[which]
    degrade, info = [], []
    t_exit0 = T0 + 999
    for res, (n, grade, trip, min_eq) in enumerate(flows):
        ts = t_exit0 + (np.arange(n, dtype=np.int64) * 1500) // n
        min_req = min_eq or 20
        if min_eq:  # every exit bad: the figure is over the threshold from the start, the minimum holds it back
            thr = Fraction(1, 2) if grade < 2 else Fraction(7)
            bad, equal = np.ones(n, bool), []
            stat_ms = 10000
        else:
            stat_ms = 1000
            thr = pick_threshold(ts, grade, min_req, stat_ms, trip)
            bad, equal = plan_bad(ts, grade, thr, min_req, stat_ms, trip)
        degrade.append(cb_rule(res, grade, thr, min_req, stat_ms))
        info.append({"res": res, "n": n, "grade": grade, "trip": trip, "ts": ts, "bad": bad, "equal": equal,
                     "min_eq": min_eq})
    case = Case("D" + which, len(flows), degrade=degrade)
    stg = Stage(case)
    stg.add([events(0, f["res"], T0 + (np.arange(f["n"], dtype=np.int64) * 999) // (f["n"] - 1)) for f in info] +
            [filler(case.first_filler, 1280, T0, T0 + 999)])
    parts = []
    for f in info:
        # a good exit's rt is exactly the slow-RT count (50: not slow, the test is rt > count)
        rt = np.where(f["bad"] & (f["grade"] == 0), 51, 50)
        parts.append(stg.exits(f["res"], f["ts"], rt=rt, err=f["bad"] & (f["grade"] > 0)))
    stg.add(parts + [filler(case.first_filler, 1280, t_exit0, t_exit0 + 1499)])
    # chunk 2: entries around the retry time (the trip's exit time + time_window s); a CLOSED breaker's pass
    t2 = t_exit0 + 1499
    parts = []
    for k, f in enumerate(info):
        if f["trip"] is None:
            parts.append(events(0, f["res"], t2 + offsets(40, 0, 3000, 1)))
            f["retry"] = None
            continue
        retry = int(f["ts"][f["trip"]]) + 2000
        f["retry"] = retry
        f["probe"] = k % 2 == 0
        before = t2 + (np.arange(30, dtype=np.int64) * (retry - 1 - t2)) // 29  # the last one at retry - 1
        after = [retry, retry, retry + 1] if f["probe"] else []
        parts.append(events(0, f["res"], np.concatenate([before, np.array(after, np.int64)])))
    t2_hi = t2 + 3000
    stg.add(parts + [filler(case.first_filler, 1280, t2, t2_hi)])
    # chunk 3: the probes' exits (good and bad alternate: HALF_OPEN -> CLOSED or back to OPEN), and the rest
    parts = []
    for k, f in enumerate(info):
        n = stg.npending(f["res"])
        if n:
            badp = (k % 4 == 0)
            parts.append(stg.exits(f["res"], t2_hi + offsets(n, 0, 400, 1), rt=np.full(n, 51 if badp else 50),
                                   err=np.full(n, badp and f["grade"] > 0)))
    stg.add(parts + [filler(case.first_filler, 1280, t2_hi, t2_hi + 400)])
    stg.close()
    for f in info:
        seam = f"grade {f['grade']}: {f['n']} exits, trip at {f['trip']}" + (" (count == minRequestAmount)" if f["min_eq"] else "")
        for ci in range(4):
            n, runs = counted_row(case.chunks[ci], f["res"])
            can = ("pass",)  # chunks 0, 1 and 3: entries of a CLOSED breaker, exits
            if ci == 2 and f["trip"] is not None:
                can = ("pass", "block") if f["probe"] else ("block",)
            if n:  # chunk 3: a probe's exit, or a CLOSED breaker's 40 exits, in one bucket
                case.row(f["res"], ci, n, runs, seam, can, single_run=ci == 3)
    case.meta["flows"] = info
    return case


# ------------------------------------------------------------------------------------------------------ group E
def build_e():
    """ENTRY_NODE tiles (k_entry_stats walks the chunk in tiles of 1024 events in arrival order).  Resources 0..3
    are inbound (their events carry EV_INBOUND), 4..7 are not; no system rule is loaded.  Chunks, in order:
    1023 / 1024 / 1025 / 2049 inbound events with as many other events between them; a chunk whose first tile
    spans 64 buckets (the most the bucketed form takes) and whose second spans 65; a chunk whose time goes back by
    1 ms exactly between events 1023 and 1024 (a tile boundary) and once inside the third tile; a last chunk that
    lies wholly before the first one (detached buckets: its adds are lost)."""
    flow = [{"resource": r, "count": 40.0 + 10 * r} for r in range(8)]
    case = Case("E", 8, flow=flow)
    case.entry_node = True
    case.sorted_chunks = False
    stg = Stage(case)
    tiles = {}

    def mixed(ts, n_in, back=False):
        """len(ts) events in the order given: entries round-robin over the resources, the first n_in inbound
        ones on resources 0..3; every third event an exit while entries are in flight."""
        n = len(ts)
        inb = np.zeros(n, bool)
        inb[np.round(np.linspace(0, n - 1, n_in)).astype(int)] = True
        assert inb.sum() == n_in
        parts, cnt = [], 0
        for i in range(n):
            r = (cnt % 4) + (0 if inb[i] else 4)
            if i % 3 == 2 and stg.npending(r) > 0 and (back or stg.pending[r][0][0] <= ts[i]):
                parts.append(stg.exits(r, [ts[i]], err=[i % 21 == 2]))
            else:
                parts.append(events(0, r, [ts[i]], flags=EV_INBOUND if inb[i] else 0, acq=1 + i % 2))
            cnt += 1
        return parts

    t = T0
    for ci, n_in in enumerate((1023, 1024, 1025, 2049)):
        ts = t + 250 + (np.arange(2 * n_in, dtype=np.int64) * 999) // (2 * n_in - 1)
        stg.add(mixed(ts, n_in) + [filler(case.first_filler, 700, t + 250, t + 1249)], sort=True)
        tiles[ci] = n_in
        t += 1000
    # tile spans: events 0..1023 over buckets b .. b+63, events 1024..2047 over b+63 .. b+127 (65 buckets)
    b = (t + 250) // 500
    ts0 = np.concatenate([[t + 250], (b + 1) * 500 + (np.arange(1022, dtype=np.int64) * (62 * 500 + 498)) // 1021,
                          [(b + 63) * 500 + 499]])
    ts1 = np.concatenate([[(b + 63) * 500 + 499], (b + 64) * 500 + (np.arange(1022, dtype=np.int64) * (62 * 500)) // 1021,
                          [(b + 127) * 500 + 250]])
    def tail(t_last):  # the filler of a chunk built in arrival order: behind the events under test, at their last time
        return [filler(case.first_filler, 2 * N_FILLER, t_last, t_last)]

    stg.add(mixed(np.concatenate([ts0, ts1]), 1500) + tail(ts1[-1]), sort=False)
    case.meta["span_chunk"] = 4
    t = (b + 127) * 500
    # time back by 1 ms between events 1023 and 1024, and once inside the third tile (event 2500)
    ts = t + 250 + (np.arange(3200, dtype=np.int64) * 999) // 3199
    ts[1024:] = ts[1024:] - (ts[1024] - ts[1023]) - 1
    ts[2500:2520] -= 300
    stg.add(mixed(ts, 2000) + tail(ts[-1]), sort=False)
    case.meta["back_chunk"] = 5
    # wholly before the first chunk
    ts = T0 - 5000 + (np.arange(1400, dtype=np.int64) * 1999) // 1399
    stg.add(mixed(ts, 900, back=True) + tail(ts[-1]), sort=False)
    case.meta["past_chunk"] = 6
    case.meta["inbound"] = tiles
    stg.close()
    seams = {r: "inbound" if r < 4 else "not inbound" for r in range(8)}
    for ci in range(len(case.chunks)):  # the chunk in the past reads windows that hold newer buckets: all blocked
        _auto_rows(case, ci, seams, {r: () if ci == case.meta["past_chunk"] else ("pass",) for r in range(8)})
    return case


# ------------------------------------------------------------------------------------------------------ group F
def _f_content(stg, case, n, t):
    """n events at t .. t + 999: five ruled resources (entries and the exits of earlier passes), the rest filler."""
    parts = []
    for r in range(5):
        k = min(stg.npending(r), 10)
        parts += [events(0, r, t + offsets(60, 0, 999, 250), acq=1 + np.arange(60) % 2),
                  stg.exits(r, t + 500 + offsets(k, 0, 400, 1))]
    m = sum(len(p["kind"]) for p in parts)
    # the filler first: at equal times the ruled resources' events come last, so a cut after n - 1 events falls
    # inside a ruled resource's run
    return [filler(case.first_filler, n - m, t, t + 999)] + parts


F_FLOW = [{"resource": 0, "count": 20.0}, {"resource": 1, "count": 200.0, "control_behavior": 2,
                                            "max_queueing_time_ms": 20},
          {"resource": 2, "count": 20.0}, {"resource": 2, "count": 30.0}, {"resource": 3, "count": 10.0, "grade": 0},
          {"resource": 4, "count": 30.0, "control_behavior": 1, "warm_up_period_sec": 2}]


def build_f(which):
    """Host chunking.  "small": one call of 1024 events (k_lsmall).  "pipe": the same 1024 events and one more
    (the pipeline).  "cut": max_batch 2048; calls of 2048 events (one chunk) and of 2049 events (cut after 2048,
    inside a 500 ms run).  "span": a call whose times span exactly 0xFFFFFFFF ms (one chunk), then one that spans
    0x100000000 ms (cut before its last event)."""
    case = Case("F" + which, 5, flow=F_FLOW)
    case.small_ok = True
    stg = Stage(case)
    seams = {r: "host chunking" for r in range(5)}
    if which in ("small", "pipe"):
        parts = _f_content(stg, case, 1024, T0)
        if which == "pipe":
            parts.append(events(0, 0, [T0 + 999]))
        stg.add(parts)
        stg.add(_f_content(stg, case, 1024 if which == "small" else 1025, T0 + 999))
        case.meta["chunks_per_call"] = [1, 1]
    elif which == "cut":
        case.max_batch = 2048
        stg.add(_f_content(stg, case, 2048, T0))
        stg.add(_f_content(stg, case, 2049, T0 + 999))
        case.meta["chunks_per_call"] = [1, 2]
        case.meta["cut_at"] = 2048
    else:
        stg.add(_f_content(stg, case, 1100, T0) + [events(0, 0, [T0 + 0xFFFFFFFF])])
        t1 = T0 + 0xFFFFFFFF
        stg.add(_f_content(stg, case, 1100, t1) + [events(0, 0, [t1 + 0x100000000])])
        case.meta["chunks_per_call"] = [1, 2]
        case.meta["spans"] = [0xFFFFFFFF, 0x100000000]
    stg.close()
    for ci in range(len(case.chunks)):
        _auto_rows(case, ci, seams)
    return case


# ------------------------------------------------------------------------------------------------------ group G
BIG = 1 << 29
INT32_MAX = (1 << 31) - 1


def build_g():
    """Acquire extremes.  Rules of count 3e9: entries of 2^29 pass until the second's pass sum is past INT32_MAX
    (the guard of lane_run's closed form and of k_lwave's WarmUp windows), a single entry of INT32_MAX, entries of
    acquire 0 -- on a lane (< 128 events), a wave (>= 128) and k_lheavy (two rules, >= 1024 events)."""
    shapes = [("default", {"count": 3e9}), ("warmup", {"count": 3e9, "control_behavior": 1, "warm_up_period_sec": 2})]
    flow, specs, res = [], [], 0
    for name, rule in shapes:
        for size, mix in ((100, "uniform"), (100, "mixed"), (300, "uniform"), (300, "mixed")):
            flow.append(dict(rule, resource=res))
            specs.append((res, f"{name} {mix} {size}", size, mix))
            res += 1
    for size in (900, 1100):
        flow += [{"resource": res, "count": 3e9}, {"resource": res, "count": 2.9e9}]
        specs.append((res, f"two rules mixed {size}", size, "mixed"))
        res += 1
    case = Case("G", res, flow=flow)
    stg = Stage(case)

    def acquires(n, mix, per_run):
        a = np.full(n, BIG, np.int64)
        if mix == "mixed":
            a[1::4] = 1
            a[2::4] = 0          # acquire == 0
            a[per_run + 3] = INT32_MAX  # a single entry of INT32_MAX, in the second run
        return a

    seams, cans = {}, {}
    for ci in range(2):
        w = frame(2 * ci, 2)
        parts = []
        for r, seam, size, mix in specs:
            k = min(stg.npending(r), size // 10)
            counts = spread(size - k, 3)
            if mix == "uniform":
                # one run of acquire 0 only, one of 2^29 only, one of INT32_MAX only: uniform runs (closed form)
                a = np.concatenate([np.zeros(counts[0], np.int64), np.full(counts[1], BIG, np.int64),
                                    np.full(counts[2], INT32_MAX, np.int64)])
            else:
                a = acquires(size - k, mix, counts[0])
            t_lo = T0 + 1000 * ci + 250
            parts += [events(0, r, run_ts(w, counts, burst=50), acq=a), stg.exits(r, t_lo + 10 + offsets(k, 0, 200, 1))]
            seams[r] = seam
            # DefaultController adds the acquire count to an int: past INT32_MAX the sum wraps and never exceeds
            # the count, so these rules pass everything; WarmUpController compares longs and blocks
            cans[r] = ("pass", "block") if seam.startswith("warmup") else ("pass",)
        stg.add(parts + [filler(case.first_filler, 1280, T0 + 1000 * ci + 250, T0 + 1000 * ci + 1249)])
        _auto_rows(case, ci, seams, cans)
    stg.close()
    case.meta["specs"] = specs
    return case


BUILDERS = {"A": build_a, "B": build_b, "C": build_c, "D4k": lambda: build_d("4k"), "D8k": lambda: build_d("8k"),
            "D16k": lambda: build_d("16k"), "E": build_e, "Fsmall": lambda: build_f("small"),
            "Fpipe": lambda: build_f("pipe"), "Fcut": lambda: build_f("cut"), "Fspan": lambda: build_f("span"),
            "G": build_g}
GROUPS = {"A": ["A"], "B": ["B"], "C": ["C"], "D": ["D4k", "D8k", "D16k"], "E": ["E"],
          "F": ["Fsmall", "Fpipe", "Fcut", "Fspan"], "G": ["G"]}
_cache = {}


def case(name):
    """Each case is built once per process and shared; nobody changes it."""
    if name not in _cache:
        _cache[name] = BUILDERS[name]()
    return _cache[name]
