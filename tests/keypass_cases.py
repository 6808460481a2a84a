"""Token batches that sit on the seams of the cluster batch's key pass (k_hot_key_*, DESIGN.md section 3,
sentinel_amd/csrc/cluster.hip): a round is 64 requests (one per lane), a chunk 4 rounds, a sub 1024 requests
(one wave), a segment 8192 (one workgroup).  Each case is a list of batches for one fresh engine: the first
makes the hot set (every rule is cold in it), the others run the key pass with hot rules.

1,000 rules with a 1000 ms window (100 ms buckets; rule 1 by far the busiest, so the hot set takes that bucket
length) and 40 with a 500 ms window (50 ms buckets: cold in every batch).  Every rule has at least FLOOR requests
in every batch, so no cold workgroup (2048 sorted elements) holds more than the 256 candidates it can publish and
the next hot set is every rule of the busiest rule's bucket length (hot_min_requests = 1).

predict() restates what the key pass must report (sga_cluster_batch_info) from the arrays alone;
tests/test_cluster_keypass_host.py proves the cases' claims on the oracle, tests/test_cluster_keypass_gpu.py
runs them on the engine."""
import numpy as np

T0 = 1_700_000_000_000  # a multiple of every bucket length used here
WH, WC = 100, 50        # bucket length of the hot rules and of the 500 ms rules
ROUND, CHUNK, SUB, SEG = 64, 256, 1024, 8192
K_HOT_BUCKETS, K_BD_ESC = 64, 63
FLAG_UNSORTED, FLAG_MIXED, FLAG_BUCKET = 1, 2, 4
POOL = np.arange(1, 1001)      # logical ids of the 1000 ms rules
COLD = np.arange(1101, 1141)   # ... of the 500 ms rules
HOLE, BEYOND = 1050, 5000      # no rule: inside the dense flowId range, and beyond it
FLOOR = 10
N_SHORT = 2 * SEG + 1          # 16,385: three segments, the last sub holds one request


def fmap(x, sparse):
    """Logical id -> flowId: itself (the dense flowId table), or far apart (the hashed table); 0 stays 0."""
    x = np.asarray(x, np.int64)
    return np.where(x > 0, 1_000_003 + 7919 * x, x) if sparse else x


def rules(sparse):
    """(flowId, count, sampleCount, windowIntervalMs) of every rule, in load order."""
    lid = np.concatenate([POOL, COLD])
    count = np.concatenate([3.0 + (np.arange(len(POOL)) * 7) % 40, 2.0 + np.arange(len(COLD)) % 9])
    count[0] = 400.0
    interval = np.concatenate([np.full(len(POOL), 1000), np.full(len(COLD), 500)]).astype(np.int32)
    return fmap(lid, sparse), count, np.full(len(lid), 10, np.int32), interval


def bucket_len(lid):
    return np.where(np.isin(lid, COLD), WC, WH)


class Batch:
    """lid: logical ids (0 = flowId 0); acq: what the four-array entry and the oracle see; resv: indices whose
    packed record carries a reserved flag bit (acq is 0 there); base: ts_base of the device entries (default: the
    earliest time).  claims: what the batch is built to hold, proven by the host test."""

    def __init__(self, lid, acq, prio, ts, resv=(), base=None, **claims):
        self.lid = np.ascontiguousarray(lid, np.int64)
        self.acq = np.ascontiguousarray(acq, np.int32)
        self.prio = np.ascontiguousarray(prio, np.uint8)
        self.ts = np.ascontiguousarray(ts, np.int64)
        self.resv = np.asarray(list(resv), np.int64)
        self.base = int(self.ts.min()) if base is None else int(base)
        self.claims = claims
        self.expect = None  # set by predict()

    @property
    def n(self):
        return len(self.lid)

    def end(self):
        return int(self.ts.max())


def fill(seed, n, toff, t0, fixed=None):
    """n requests at t0 + toff: `fixed` ({index: (lid, acq, prio)}) where given, elsewhere FLOOR requests of every
    rule and a skewed draw over the 1000 ms rules (rule 1 the busiest), 1 % prioritized, in a seeded order."""
    rng = np.random.default_rng(seed)
    fixed = fixed or {}
    free = np.setdiff1d(np.arange(n), np.fromiter(fixed.keys(), np.int64, len(fixed)))
    base = np.repeat(np.concatenate([POOL, COLD]), FLOOR)
    m = len(free) - len(base)
    assert m >= 0, (n, len(fixed))
    z = rng.zipf(1.25, size=m)
    k = np.where(z <= len(POOL), z, rng.integers(1, len(POOL) + 1, size=m))
    lid = np.zeros(n, np.int64)
    acq = np.ones(n, np.int32)
    prio = np.zeros(n, np.uint8)
    lid[free] = rng.permutation(np.concatenate([base, k]))
    prio[free] = rng.random(len(free)) < 0.01
    for i, (f, a, p) in fixed.items():
        lid[i], acq[i], prio[i] = f, a, p
    return lid, acq, prio, t0 + np.asarray(toff, np.int64)


def hot_round(fixed, r, lane=None, rare=None):
    """Round r (requests 64 r .. 64 r + 63) full of requests of 1000 ms rules, acquire 1, not prioritized; `rare`
    (lid, acq) at `lane`."""
    for l in range(ROUND):
        fixed[r * ROUND + l] = (int(POOL[(r * 13 + l * 7) % len(POOL)]), 1, 0)
    if rare is not None:
        fixed[r * ROUND + lane] = (rare[0], rare[1], 0)


def steps(n, starts):
    """Time offsets of n requests in hot buckets 0, 1, ...: bucket j + 1 starts at request starts[j]; inside a
    bucket the times rise by a few ms."""
    i = np.arange(n, dtype=np.int64)
    b = np.searchsorted(np.asarray(sorted(starts)), i, side="right")
    return b * WH + (i * 40) // n


def normal(seed, t0, n=N_SHORT):
    """A plain hot-path batch over 250 ms."""
    return Batch(*fill(seed, n, (np.arange(n, dtype=np.int64) * 250) // n, t0), path="hot")


def next_t0(b):
    """The start of the batch after b: the next multiple of 100 ms after b's last request."""
    return (b.end() // WH + 1) * WH


# ------------------------------------------------------------------------------------------------ the cases
def first(seed):
    n = N_SHORT
    return Batch(*fill(seed, n, (np.arange(n, dtype=np.int64) * 90) // n, T0), path="first")


def case_boundary(which):
    """Bucket boundaries whose first request sits on / next to the round, chunk, sub and segment edges, and at
    lane 1 and lane 62 of a round."""
    starts = {"a": [63, 255, 1023, 40 * ROUND + 1, 8191], "b": [64, 256, 1024, 50 * ROUND + 62, 8192],
              "c": [65, 257, 1025, 8193]}[which]
    b0 = first(10)
    n = N_SHORT
    return [b0, Batch(*fill(11 + ord(which), n, steps(n, starts), next_t0(b0)), path="hot", boundaries=starts)]


def case_multi():
    """Two boundaries in one round by a jump of two buckets between neighbouring lanes (at lane 0, inside a round
    and at lane 63), then a batch whose first round spans two buckets."""
    b0 = first(20)
    n = N_SHORT
    jumps = [3 * ROUND, 9 * ROUND + 30, 20 * ROUND + 63, SEG + 5]
    i = np.arange(n, dtype=np.int64)
    toff = 2 * WH * np.searchsorted(np.asarray(jumps), i, side="right") + (i * 40) // n
    b1 = Batch(*fill(21, n, toff, next_t0(b0)), path="hot", boundaries=jumps, jump=2)
    b2 = Batch(*fill(22, n + 62, steps(n + 62, [5, 2000]), next_t0(b1)), path="hot", boundaries=[5, 2000])
    return [b0, b1, b2]


def case_backward():
    """One descending timestamp at lane 0 (across a round edge), lane 1 and lane 63 of a round, across a sub edge
    and across a segment edge: kFlagUnsorted, the batch decided as cold; each followed by a plain hot-path batch."""
    out = [first(30)]
    for j, at in enumerate([5 * ROUND, 7 * ROUND + 1, 11 * ROUND + 63, 3 * SUB, SEG]):
        n = N_SHORT
        toff = (np.arange(n, dtype=np.int64) * 250) // n + 5
        toff[at] = toff[at - 1] - 1
        out.append(Batch(*fill(31 + 2 * j, n, toff, next_t0(out[-1])), path="unsorted", backward=at))
        out.append(normal(32 + 2 * j, next_t0(out[-1])))
    return out


def case_over64():
    """65 hot buckets (kFlagBucket), then the hot path again; 64 buckets stay hot."""
    b0 = first(40)
    n = N_SHORT
    i = np.arange(n, dtype=np.int64)
    b1 = Batch(*fill(41, n, (i * 64 // n) * WH + 3, next_t0(b0)), path="hot", span=64)
    b2 = Batch(*fill(42, n, (i * 65 // n) * WH + 3, next_t0(b1)), path="bucket", span=65)
    return [b0, b1, b2, normal(43, next_t0(b2))]


RARE_KINDS = ("fid0", "acq0", "resv", "hole", "beyond", "acq128")
DELTA_ROUND0 = 200  # the first of the six rounds that hold the 500 ms rule at bucket delta 62 / 63 / 64


def case_rare(sparse=False):
    """Rare lanes that leave the batch on the hot path, each the only one of a round of hot requests, once at lane
    0 and once at lane 63: flowId 0, acquire 0, a reserved flag bit, an unknown flowId, a flowId beyond the dense
    range, acquire 128 on a 500 ms rule, and a 500 ms rule at bucket delta 62 / 63 / 64 of its own 50 ms buckets."""
    b0 = first(50)
    n = N_SHORT
    fixed, resv, where = {}, [], {}
    r = 10
    for kind in RARE_KINDS:
        for lane in (0, 63):
            rare = {"fid0": (0, 1), "acq0": (7, 0), "resv": (9, 0), "hole": (HOLE, 1), "beyond": (BEYOND, 1),
                    "acq128": (int(COLD[3]), 128)}[kind]
            hot_round(fixed, r, lane, rare)
            where[(kind, lane)] = r * ROUND + lane
            if kind == "resv":
                resv.append(r * ROUND + lane)
            r += 1
    toff = (np.arange(n, dtype=np.int64) * 40) // n
    r = DELTA_ROUND0
    for d in (K_BD_ESC - 1, K_BD_ESC, K_BD_ESC + 1):
        for lane in (0, 63):
            hot_round(fixed, r, lane, (int(COLD[5 + lane % 2]), 1))
            where[(f"delta{d}", lane)] = r * ROUND + lane
            toff[r * ROUND:(r + 1) * ROUND] = d * WC + lane % 2
            r += 1
    toff[r * ROUND:] = (K_BD_ESC + 2) * WC + (np.arange(n - r * ROUND, dtype=np.int64) * 40) // n
    b1 = Batch(*fill(51, n, toff, next_t0(b0), fixed), resv=resv, path="hot", rare=where)
    return [b0, b1]


def case_mixed():
    """acquire 2 and acquire 128 on a hot rule (kFlagMixed), at lane 0 and lane 63 of a round of hot requests, each
    followed by a plain hot-path batch."""
    out = [first(60)]
    for j, (a, lane) in enumerate([(2, 0), (2, 63), (128, 0)]):
        fixed = {}
        hot_round(fixed, 17, lane, (1, a))
        n = N_SHORT
        out.append(Batch(*fill(61 + 2 * j, n, (np.arange(n, dtype=np.int64) * 250) // n, next_t0(out[-1]), fixed),
                         path="mixed", rare={("mixed", lane): 17 * ROUND + lane}))
        out.append(normal(62 + 2 * j, next_t0(out[-1])))
    return out


def case_overflow():
    """Time offsets just below 2^32 from a ts_base 50 ms into a hot bucket: r0 + t crosses 2^32 between lane 12
    and lane 13 of a round.  Such a batch is more than 64 buckets from its ts_base: kFlagBucket, decided as cold
    with every bucket delta an escape; then the hot path again."""
    b0 = first(70)
    n = N_SHORT
    t0 = next_t0(b0) + 56  # with the offsets below, ts_base is 50 ms into a bucket
    cross = 16 * ROUND + 13
    toff = np.where(np.arange(n) < cross, (1 << 32) - 90, (1 << 32) - 10).astype(np.int64)
    base = t0 - ((1 << 32) - 90)
    lid, acq, prio, ts = fill(71, n, toff, base)
    assert base % WH == 50 and (base % WH + toff[cross - 1] < 1 << 32 <= base % WH + toff[cross])
    b1 = Batch(lid, acq, prio, ts, base=base, path="bucket", cross=cross)
    return [b0, b1, normal(72, next_t0(b1))]


def case_tail():
    """n = 1, 63 and 0 (mod 64): a last sub of one request, a last round of 63, and whole segments only."""
    out = [first(80)]
    for j, n in enumerate([N_SHORT, 2 * SEG + 63, 2 * SEG + 64, 3 * SEG]):
        out.append(normal(81 + j, next_t0(out[-1]), n))
    return out


def case_sparse():
    """The hashed-table key kernels: boundaries, a backward step, rare lanes."""
    b0 = first(90)
    n = N_SHORT
    starts = [63, 256, 1025, 40 * ROUND + 1, 8192]
    b1 = Batch(*fill(91, n, steps(n, starts), next_t0(b0)), path="hot", boundaries=starts)
    toff = (np.arange(n, dtype=np.int64) * 250) // n + 5
    at = 11 * ROUND + 63
    toff[at] = toff[at - 1] - 1
    b2 = Batch(*fill(92, n, toff, next_t0(b1)), path="unsorted", backward=at)
    rare = case_rare()[1]
    shift = next_t0(b2) - int(rare.ts.min())
    b3 = Batch(rare.lid, rare.acq, rare.prio, rare.ts + shift, resv=rare.resv, **rare.claims)
    return [b0, b1, b2, b3]


BUILDERS = {
    "boundary_a": lambda: case_boundary("a"),
    "boundary_b": lambda: case_boundary("b"),
    "boundary_c": lambda: case_boundary("c"),
    "multi": case_multi,
    "backward": case_backward,
    "over64": case_over64,
    "rare": case_rare,
    "mixed": case_mixed,
    "overflow": case_overflow,
    "tail": case_tail,
    "sparse": case_sparse,
}
SPARSE = {"sparse"}
PATH_FLAG = {"unsorted": FLAG_UNSORTED, "mixed": FLAG_MIXED, "bucket": FLAG_BUCKET}


def predict(batches):
    """Sets every batch's expect: the words sga_cluster_batch_info must report, from the arrays alone.  A batch
    with a hot set stays on the hot path unless a time decreases, a hot bucket delta from ts_base reaches 64 or a
    valid request of a hot rule has an acquire count other than 1; a fallback batch keeps the flags and the first
    request's bucket delta (clipped to 63) and counts every valid request as cold.  Returns the hot sets."""
    known = np.concatenate([POOL, COLD])
    hot = np.zeros(0, np.int64)
    sets = []
    for b in batches:
        valid = np.isin(b.lid, known) & (b.acq >= 1)
        q = b.ts // WH - b.base // WH
        ishot = valid & np.isin(b.lid, hot)
        sets.append(hot)
        flags = 0
        if len(hot):
            flags |= FLAG_UNSORTED if (np.diff(b.ts) < 0).any() else 0
            flags |= FLAG_BUCKET if (q >= K_HOT_BUCKETS).any() else 0
            flags |= FLAG_MIXED if (ishot & (b.acq != 1)).any() else 0
        if not len(hot):
            b.expect = dict(hot_mode=0, flags=0, bd_lo=0, bd_hi=0, n_cold=int(valid.sum()))
        elif flags:
            b.expect = dict(hot_mode=0, flags=flags, bd_lo=int(min(q[0], K_HOT_BUCKETS - 1)), bd_hi=0,
                            n_cold=int(valid.sum()))
        else:
            b.expect = dict(hot_mode=1, flags=0, bd_lo=int(q[0]), bd_hi=int(q.max()), n_cold=int((valid & ~ishot).sum()))
        ids, cnt = np.unique(b.lid[valid], return_counts=True)
        busiest = ids[np.lexsort((ids, cnt))[-1]]
        hot = ids[bucket_len(ids) == bucket_len(busiest)]
    return sets


_cases = {}


def case(name):
    """(batches with their expectations, hot set per batch), built once."""
    if name not in _cases:
        bs = BUILDERS[name]()
        _cases[name] = (bs, predict(bs))
    return _cases[name]


_replays = {}


def replay(name):
    """The oracle's (status, remaining, wait) per batch and, at the end, all seven metric sums of every rule:
    computed once per case and shared."""
    if name in _replays:
        return _replays[name]
    import ctypes as C

    from sentinel_amd.cluster import CLUSTER_RULE_DTYPE
    from tests import oracle_harness as H
    sparse = name in SPARSE
    bs, _ = case(name)
    fid, count, sample, interval = rules(sparse)
    a = np.zeros(len(fid), dtype=CLUSTER_RULE_DTYPE)
    a["flow_id"], a["count"], a["threshold_type"], a["sample_count"] = fid, count, 1, sample
    a["window_interval_ms"], a["grade"], a["resource_timeout_ms"], a["client_offline_time_ms"] = interval, 1, 2000, 2000
    L = H.lib()
    oh = L.orc_cluster_new(1.0, 1.0)
    L.orc_cluster_load_rules(oh, b"default", a.ctypes.data_as(C.POINTER(H.OrcClusterRule)), len(a))
    res = []
    try:
        for b in bs:
            out = (H.OrcTokenResult * b.n)()
            f = np.ascontiguousarray(fmap(b.lid, sparse))
            L.orc_cluster_replay(oh, b.n, f.ctypes.data, b.acq.ctypes.data, b.prio.ctypes.data, b.ts.ctypes.data, out)
            r = np.frombuffer(out, dtype=np.int32).reshape(b.n, 3)
            res.append((r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy()))
        now = max(b.end() for b in bs) + 1
        sums = {int(f): [int(L.orc_cluster_metric_sum(oh, int(f), ev, now)) for ev in range(7)] for f in fid}
    finally:
        L.orc_cluster_free(oh)
    _replays[name] = dict(results=res, now=now, sums=sums)
    return _replays[name]
