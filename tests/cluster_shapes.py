"""Deterministic cluster token batches that sit on the size seams of the cluster batch (DESIGN.md section 3,
sentinel_amd/csrc/cluster.hip): each named case gives rules, engine arguments, a list of steps (token batches,
an RLS batch, a hot-rules switch) and a shape table naming, per targeted rule, the seam it sits on.

tests/test_cluster_shapes_host.py proves on the oracle alone that every case has the shape its table claims;
tests/test_cluster_shapes_gpu.py compares the engine with the oracle on every request of every batch.

Rules are loaded in one call on a fresh engine with flowId = load index + 1, so slot s holds flowId s + 1: the
LSD sort orders a batch by flowId, and the cold partition's bin b (30,000 rules: 5 slot bits below the bin)
holds flowIds 32 b + 1 .. 32 b + 32.

Cold-stage modes:
  sort   hot_rules off, small_batch 0: k_classify, the LSD sort, k_cold_fused<chunk>
  small  small_batch 4096 and batches of at most 4096 requests: k_small_sort, k_cold_fused<chunk>
  hot    hot rules on with a hot_min_requests nothing reaches, 3,000 rules: key passes, LSD sort, k_cold_fused<chunk>
  bin    the same with 30,000 rules: key passes, cold partition, k_cold_fused<bin>

Groups (one or more cases each):
  R  run length and answer form: 31/32/33 (kFzDirect), 63/64/65 (one wave step), 511/512/513, 2047/2048/2049
     (kFzHuge), with 0 / 1 / 4 / 5 / 65 prioritized requests (prio_before's four loads against its search),
     first block at 0, at n - 1, never; a rule with three runs in one batch and an occupy transfer
  L  the long-run list (kFzLong = 512): bins with 511 / 512 / 513 runs of 33 requests, a huge run among the 513
     (bin form only: a chunk-form workgroup owns 2048 elements of whole rules and one continuing rule of at most
     63 closed-form runs, so its list never fills)
  C  chunk ownership (kFzChunk = 2048): heads and ends on chunk edges, rules continuing 2047 .. 5 * 2048 + 1
     past their chunk, run records on both sides of the LDS / global split, 255 / 256 / 257 / 2048 rules per
     chunk, the invalid suffix
  B  bins: 1, 2559 / 2560 / 2561 (kBinLds), 3071 / 3072 / 3073 (bin_order's register rounds), more than 65,536
     elements, 32 rules or one rule per bin, the R sizes in an LDS bin and in a global bin
  E  escapes to the per-request replay: acquire 126 / 127 / 128 / 2^30, mixed acquire, bucket delta 62 / 63 / 64,
     sampleCount 12, 500 ms rules crossing delta 63 beside hot 1000 ms rules
  S  batch sizes around the small path and the tile: 1, 63 / 64 / 65, 4095 / 4096 / 4097, 1000 / 1001
  P  key segments: 1, 8, 9, 16, 17, 64, 65 (30,000 rules: the partition runs), 256, 257
     (a case that picks a hot set from an all-cold first batch gives every rule of that batch at least 8
     requests: no 2048-element chunk then holds more than the 256 candidates a workgroup can publish)
  H  hot side: 64 and 65 hot buckets, buckets starting at request 8191 / 8192 / 8193, a hot rule owning a
     whole segment, prioritized hot requests 0 / 1 / 64 / 65 / 4097 per rule and 16,383 / 16,385 per batch,
     sampleCount 1 / 2 / 64 / 65 among the busiest rules, 4095 / 4096 / 4097 candidates in one log2 count bin,
     a cold workgroup with 257 candidates
  M  a hot-path batch, an RLS batch, a sort-path batch and a hot-path batch on one engine of 30,000 rules"""
import numpy as np

T0 = 1_700_000_000_000  # a multiple of every window length used here
W = 100                 # bucket length of the 1000 ms / sampleCount 10 rules
SEG, CHUNK = 8192, 2048
K_DIRECT, K_LONG, K_HUGE, K_BIN_LDS, K_BO = 32, 512, 2048, 2560, 768
K_ACQ_MAX, K_BD_ESC, K_HOT, K_HOT_BUCKETS = 127, 63, 4096, 64
NEVER_HOT = 1 << 30     # hot_min_requests no rule reaches
N_CHUNK_RULES, N_BIN_RULES, BIN_LB = 3000, 30000, 5
FLAG_BUCKET = 4

MODES = {
    "sort": dict(hot_rules=False, small_batch=0),
    "small": dict(hot_rules=True, hot_min_requests=64, small_batch=4096),
    "hot": dict(hot_rules=True, hot_min_requests=NEVER_HOT, small_batch=0),
    "bin": dict(hot_rules=True, hot_min_requests=NEVER_HOT, small_batch=0),
}
R_SIZES = [31, 32, 33, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049]
R_PRIO = {31: 1, 32: 4, 33: 5, 63: 5, 64: 4, 65: 1, 511: 65, 512: 5, 513: 4, 2047: 65, 2048: 1, 2049: 65}
R_PRIME = 3  # passes in the head bucket of a rule that is to answer SHOULD_WAIT nine buckets later


class Case:
    def __init__(self, name, mode, n_rules, engine_args, max_batch=1 << 17):
        self.name, self.mode, self.n_rules = name, mode, n_rules
        self.engine_args, self.max_batch = dict(engine_args), max_batch
        self.count = np.full(n_rules, 3.0)          # filler: three tokens per second
        self.sample = np.full(n_rules, 10, np.int32)
        self.interval = np.full(n_rules, 1000, np.int32)
        self.steps = []    # {"kind": "token", fid, acq, prio, ts, "info": {...}} | {"kind": "rls", fid, ts} |
                           # {"kind": "hot", "on": bool}
        self.table = []    # rows: see row()
        self.fillers = []  # three filler rules whose metric sums are compared too

    @property
    def flow_id(self):
        return np.arange(1, self.n_rules + 1, dtype=np.int64)

    @property
    def n_requests(self):
        return sum(len(s["fid"]) for s in self.steps if s["kind"] != "hot")

    def bucket_len(self, rule):
        return int(self.interval[rule - 1]) // int(self.sample[rule - 1])

    def set_rule(self, rule, count, sample=10, interval=1000):
        self.count[rule - 1], self.sample[rule - 1], self.interval[rule - 1] = count, sample, interval

    def row(self, rule, step, seam, runs, prio=None, **expect):
        """A targeted rule in one step: the run lengths (per bucket, in time order) and the prioritized
        requests per run that the arrays must hold, and what the oracle must answer (expect):
          mix          "both" (passes and blocks), "pass", "block"
          wait         True / False: SHOULD_WAIT among the answers
          first_block  position in the rule's requests of this step of the first answer that is not OK
          escape       "acquire" / "mixed" / "delta": why the run is replayed per request
          head, end    positions of the rule's first element and past its last one in the sorted batch
          bin, bin_n   its partition bin and that bin's population"""
        self.table.append(dict(rule=rule, step=step, seam=seam, runs=list(runs),
                               prio=list(prio) if prio is not None else [0] * len(runs), **expect))

    def token(self, fid, acq, prio, ts, **info):
        self.steps.append(dict(kind="token", fid=np.ascontiguousarray(fid, np.int64),
                               acq=np.ascontiguousarray(acq, np.int32), prio=np.ascontiguousarray(prio, np.uint8),
                               ts=np.ascontiguousarray(ts, np.int64), info=info))
        return len(self.steps) - 1

    @property
    def watched(self):
        """The rules whose seven metric sums are compared after every step."""
        return self.targets + [f for f in self.fillers if f not in self.targets]

    @property
    def sum_touched(self):
        """A case whose table names no rule (S, P, M, some of H): at the end, the seven sums of every touched rule."""
        return not self.targets

    def touched(self):
        """Every rule that a step of the case names (valid flowIds), but for the watched ones."""
        ids = np.unique(np.concatenate([s["fid"] for s in self.steps if s["kind"] != "hot"]))
        ids = ids[(ids >= 1) & (ids <= self.n_rules)]
        return [int(f) for f in ids[~np.isin(ids, self.watched)]]

    @property
    def targets(self):
        return sorted({r["rule"] for r in self.table if r["rule"] > 0})

    def seam_of(self, rule):
        return "; ".join(dict.fromkeys(r["seam"] for r in self.table if r["rule"] == rule)) or "filler"

    def rules_array(self):
        """The rules as the oracle's orc_cluster_rule records (the engine's bulk load has the same layout)."""
        from sentinel_amd.cluster import CLUSTER_RULE_DTYPE
        a = np.zeros(self.n_rules, dtype=CLUSTER_RULE_DTYPE)
        a["flow_id"], a["count"], a["threshold_type"] = self.flow_id, self.count, 1
        a["sample_count"], a["window_interval_ms"], a["grade"] = self.sample, self.interval, 1
        a["resource_timeout_ms"], a["client_offline_time_ms"] = 2000, 2000
        return a


def run(rule, k, n, prio=(), acq=1):
    """n requests of one rule in bucket k of a batch (prio: positions in the run; acq: one value or n values)."""
    return dict(rule=int(rule), k=int(k), n=int(n), prio=tuple(int(p) for p in prio), acq=acq)


def assemble(runs, t0, seed, w=W, span=None):
    """The batch that holds `runs`: bucket after bucket (k * w from t0), within a bucket the runs interleaved by
    a seeded permutation with every run's own order kept, timestamps non-decreasing over span = (lo, hi)
    milliseconds of the bucket."""
    rng = np.random.default_rng(seed)
    lo, hi = span if span else (0, w - 1)
    out = [[], [], [], []]
    for k in sorted({r["k"] for r in runs}):
        rs = [r for r in runs if r["k"] == k and r["n"] > 0]
        lens = np.array([r["n"] for r in rs])
        m = int(lens.sum())
        lab = rng.permutation(np.repeat(np.arange(len(rs)), lens))
        order = np.argsort(lab, kind="stable")   # positions of run 0 ascending, then of run 1, ...
        f = np.empty(m, np.int64)
        a = np.ones(m, np.int32)
        p = np.zeros(m, np.uint8)
        f[order] = np.repeat(np.array([r["rule"] for r in rs], np.int64), lens)
        start = np.concatenate([[0], np.cumsum(lens)])
        for j, r in enumerate(rs):
            if r["prio"]:
                p[order[start[j] + np.array(r["prio"])]] = 1
            if not np.isscalar(r["acq"]) or r["acq"] != 1:
                a[order[start[j]:start[j + 1]]] = r["acq"]
        t = t0 + k * w + lo + (np.arange(m, dtype=np.int64) * (hi - lo)) // max(m, 1)
        for o, x in zip(out, (f, a, p, t)):
            o.append(x)
    return [np.concatenate(o) for o in out]


def filler_runs(ids, ks, seed, lo=1, hi=6):
    """A few requests (lo .. hi, by a seeded draw) of every filler rule in every bucket of ks."""
    rng = np.random.default_rng(seed)
    ids = np.asarray(list(ids))
    return [run(r, k, c) for k in ks for r, c in zip(ids, rng.integers(lo, hi + 1, size=len(ids)))]


def spread_prio(n, first_blocked, cp):
    """cp prioritized positions: every second one from the run's end (inside the blocked part), and for
    cp >= 4 the run's first request instead of the earliest of them (a prioritized pass)."""
    pos = [n - 1 - 2 * j for j in range(cp)]
    assert pos[-1] > first_blocked, (n, first_blocked, cp)
    if cp >= 4:
        pos[-1] = 0
    return sorted(pos)


# ------------------------------------------------------------------------------------------------ R
def r_specs(c, ids, sizes=R_SIZES, where=""):
    """Per size two rules from ids: one without prioritized requests (passes, then blocks) and one whose head
    bucket holds R_PRIME passes, so that nine buckets later prioritized requests behind the last pass answer
    SHOULD_WAIT (cw > 0).  Then a rule blocked from position 0, one blocked at n - 1 only, one that passes
    everything.  Returns (prime runs for bucket q0, main runs for bucket q0 + 9, rows without step)."""
    ids = iter(ids)
    prime, main, rows = [], [], []
    for n in sizes:
        a, b = next(ids), next(ids)
        ka = n - n // 3
        c.set_rule(a, ka)
        main.append(run(a, 0, n))
        rows.append(dict(rule=a, seam=f"run of {n}, no prioritized request{where}", runs=[n], prio=[0], mix="both",
                         wait=False, first_block=ka))
        kb, cp = n // 2, R_PRIO[n]
        c.set_rule(b, kb)
        prime.append(run(b, 0, R_PRIME))
        pp = spread_prio(n, kb - R_PRIME, cp)
        main.append(run(b, 0, n, prio=pp))
        rows.append(dict(rule=b, seam=f"run of {n}, {cp} prioritized, waits{where}", runs=[n], prio=[cp], mix="both",
                         wait=True, first_block=kb - R_PRIME, waits=min(R_PRIME, cp - (1 if cp >= 4 else 0))))
    z, l, al = next(ids), next(ids), next(ids)
    c.set_rule(z, 5)
    prime.append(run(z, 0, 8))
    main.append(run(z, 0, 40))
    rows.append(dict(rule=z, seam=f"blocked from position 0{where}", runs=[40], prio=[0], mix="block", wait=False,
                     first_block=0))
    c.set_rule(l, 39)
    main.append(run(l, 0, 40))
    rows.append(dict(rule=l, seam=f"first block at n - 1{where}", runs=[40], prio=[0], mix="both", wait=False,
                     first_block=39))
    c.set_rule(al, 100)
    main.append(run(al, 0, 40, prio=(3, 20)))
    rows.append(dict(rule=al, seam=f"passes everything{where}", runs=[40], prio=[2], mix="pass", wait=False,
                     first_block=None))
    return prime, main, rows


def build_R(mode):
    n_rules = N_BIN_RULES if mode == "bin" else N_CHUNK_RULES
    c = Case(f"R_{mode}", mode, n_rules, MODES[mode])
    # targets three flowIds apart from 100 on, filler on the flowIds between and around them
    tids = list(range(100, 100 + 3 * 40, 3))
    prime, main, rows = r_specs(c, tids[:27])
    t3 = tids[27]  # three runs in one batch, after SHOULD_WAIT answers in the batch before (occupy transfer)
    c.set_rule(t3, 20)
    prime.append(run(t3, 0, R_PRIME))
    main.append(run(t3, 0, 30, prio=(24, 25, 26, 27, 28, 29)))
    rows.append(dict(rule=t3, seam="waits, then three runs in the next batch", runs=[30], prio=[6], mix="both", wait=True,
                     first_block=20 - R_PRIME, waits=R_PRIME))
    near = [f for f in range(60, 260) if f not in tids]
    far = list(range(300, n_rules, 9 if mode != "bin" else 61))
    c.fillers = near[:3]
    c.token(*assemble(prime + filler_runs(near + far, [0], 1), T0, 11))
    if mode == "small":  # at most 4096 requests per batch: the small runs in two batches, every big run alone
        big = [m for m in main if m["n"] > 600]
        small = [m for m in main if m["n"] <= 600]
        parts = [small[0::2], small[1::2]] + [[m] for m in big]
    else:
        parts = [main]
    for j, part in enumerate(parts):
        fid, acq, prio, ts = assemble(part + filler_runs(near + far[::4], [0], 20 + j), T0 + 9 * W, 30 + j,
                                      span=(10 * j, 10 * j + 9) if len(parts) > 1 else None)
        assert mode != "small" or len(fid) <= 4096
        step = c.token(fid, acq, prio, ts)
        for r in rows:
            if any(m["rule"] == r["rule"] for m in part):
                c.row(step=step, **r)
    # bucket q0 + 10 takes the occupied tokens (the window still holds q0 + 9: all blocked); q0 + 19 and q0 + 20
    # come after q0 + 9 has left the window
    ks = [0, 9, 10]
    last = [run(t3, k, 40, prio=(5, 35)) for k in ks]
    step = c.token(*assemble(last + filler_runs(near + far[::4], ks, 40), T0 + 10 * W, 41))
    c.row(t3, step, "three runs (three buckets) in one batch, the first takes the occupied tokens", [40, 40, 40], [2, 2, 2],
          mix="both", wait=True)
    return c


# ------------------------------------------------------------------------------------------------ L
def build_L():
    """Bins of 32 rules x 16 buckets of 33 requests: 511, 512 and 513 runs for the long-run list of one
    workgroup (kFzLong = 512); among the 513 one run of 2048 requests that passes and blocks without a wait."""
    c = Case("L_bin", "bin", N_BIN_RULES, MODES["bin"])
    runs = []
    for b, total in ((10, K_LONG - 1), (20, K_LONG), (30, K_LONG + 1)):
        ids = list(range(32 * b + 1, 32 * b + 33))
        left = total
        for j, f in enumerate(ids):
            nb = 16 if j < 31 else left  # the last rule takes what is left: 15, 16 or 17 buckets
            huge = total == K_LONG + 1 and j == 0
            c.set_rule(f, 1500 if huge else 20)
            lens = [(K_HUGE if huge and k == 0 else K_DIRECT + 1) for k in range(nb)]
            runs += [run(f, k, n) for k, n in enumerate(lens)]
            left -= nb
            c.table.append(dict(rule=f, step=0, seam=f"bin {b}: {total} listed runs" + (", one of them huge" if huge else ""),
                                runs=lens, prio=[0] * nb, mix="both", wait=False, bin=b,
                                bin_n=total * (K_DIRECT + 1) + (K_HUGE - K_DIRECT - 1 if total == K_LONG + 1 else 0),
                                bin_runs=total))
    far = list(range(2000, N_BIN_RULES, 37))
    c.fillers = far[:3]
    c.token(*assemble(runs + filler_runs(far, range(17), 2, hi=2), T0, 51))
    return c


# ------------------------------------------------------------------------------------------------ C
class Layout:
    """Rules in flowId order with chosen request counts, so that each rule's first element lands on a chosen
    position of the sorted batch (every request valid: position = requests of the flowIds before it)."""

    def __init__(self, c, first=1):
        self.c, self.next, self.pos, self.runs, self.rows = c, first, 0, [], []

    def filler(self, n):
        f = self.next
        self.next += 1
        self.pos += n
        self.runs.append(run(f, 0, n))
        return f

    def pad_to(self, pos, each=5):
        """Filler rules of `each` requests (the last one of what is left) up to position pos."""
        assert pos >= self.pos, (pos, self.pos)
        while self.pos < pos:
            self.filler(min(each, pos - self.pos))

    def rule(self, lens, seam, count=None, **expect):
        """A targeted rule with one run per entry of lens (buckets 0, 1, ...)."""
        f = self.next
        self.next += 1
        n = sum(lens)
        self.c.set_rule(f, count if count is not None else max(1, lens[0] // 2))
        self.runs += [run(f, k, m) for k, m in enumerate(lens)]
        c1 = (self.pos // CHUNK + 1) * CHUNK
        self.rows.append(dict(rule=f, seam=seam, runs=list(lens), prio=[0] * len(lens), head=self.pos,
                              end=self.pos + n, past=max(0, self.pos + n - c1), **expect))
        self.pos += n
        return f


def build_C(mode, invalid):
    """invalid: requests of flowId 0 and of an unknown flowId that form the sorted batch's suffix."""
    c = Case(f"C_{mode}_inv{invalid}", mode, 20000, MODES[mode])
    lay = Layout(c)
    k = CHUNK
    lay.pad_to(k - 1)
    lay.rule([1 + 2047], "head on the last element of its chunk, continues 2047 past c1 (one chunk ahead)", mix="both")
    lay.pad_to(3 * k - 7)
    lay.rule([7], "ends exactly at its chunk's end", count=3, mix="both")
    lay.rule([4], "head on the first element of a chunk", count=2, mix="both")
    lay.pad_to(4 * k - 6)
    lay.rule([7], "ends one past its chunk's end", count=3, mix="both")
    lay.pad_to(5 * k - 5)
    lay.rule([5 + 2048], "continues 2048 past c1: ends with the chunk ahead (first gallop probe at n or a new rule)",
             mix="both")
    lay.pad_to(7 * k - 3)
    lay.rule([3 + 2049], "continues 2049 past c1 (gallop, then bisect)", mix="both")
    for x in (4095, 4096, 4097):
        lay.pad_to((lay.pos // k + 2) * k - 9)
        lay.rule([9 + x], f"continues {x} past c1 (first gallop probe)", mix="both")
    for x in (5 * k - 1, 5 * k + 1):
        lay.pad_to((lay.pos // k + 2) * k - 2)
        lay.rule([2 + x], f"continues {x} past c1 (second gallop probe, bisect); chunks without a rule head", mix="both")
    # run records on both sides of the LDS / global split: the chunk's first head is h0 = its first element,
    # the continuing rule's runs start 2047, 2048 and 2049 positions after h0
    c0 = (lay.pos // k + 2) * k
    lay.pad_to(c0 - 4)
    lay.filler(4)
    assert lay.pos == c0
    lay.pad_to(c0 + 1500)
    lay.rule([547, 1, 1, 600, 40], "runs starting 2047 / 2048 / 2049 after h0 (LDS and global run records)",
             count=100, mix="both", run_starts_after_h0=[1500, 2047, 2048, 2049, 2649], h0=c0)
    # rules per chunk: 255, 256, 257 and 2048 (rules past the first 256 are taken from the workgroup counter)
    c0 = (lay.pos // k + 2) * k
    lay.pad_to(c0 - 4)
    lay.filler(4)
    for nr in (255, 256, 257):
        first = lay.next
        lens = [8] * nr
        if nr == 255:
            lens[:8] = [9] * 8
        if nr == 257:
            lens[-2:] = [4, 4]
        for m in lens:
            lay.filler(m)
        c.table.append(dict(rule=-1, step=0, seam=f"{nr} rules in one chunk", runs=[], prio=[], chunk=lay.pos // k - 1,
                            chunk_rules=nr, first_rule=first))
        assert lay.pos % k == 0
    first = lay.next
    for _ in range(k):
        lay.filler(1)
    c.table.append(dict(rule=-1, step=0, seam="2048 rules of one request in one chunk", runs=[], prio=[],
                        chunk=lay.pos // k - 1, chunk_rules=k, first_rule=first))
    # the batch ends inside a continuing rule: with no invalid request that rule ends exactly at n
    lay.pad_to(lay.pos + k - 3)
    lay.rule([3 + 2500], "continues past c1 to the end of the valid elements" + (" = n" if not invalid else ""), mix="both")
    assert lay.next <= c.n_rules
    for r in lay.rows:
        c.table.append(dict(step=0, **r))
    c.fillers = [1, 2, 3]
    fid, acq, prio, ts = assemble(lay.runs, T0, 61)
    if invalid:  # spread over the batch in arrival order
        at = np.linspace(7, len(fid) - 1, invalid).astype(np.int64)
        fid = np.insert(fid, at, np.where(np.arange(invalid) % 2 == 0, 0, c.n_rules + 12345))
        acq = np.insert(acq, at, 1)
        prio = np.insert(prio, at, 0)
        ts = np.insert(ts, at, ts[at])
    c.token(fid, acq, prio, ts, n_valid=lay.pos, n_invalid=invalid)
    # a second batch in the next bucket: the continuing rules again, on their carried state
    second = [dict(m, k=0) for m in lay.runs if m["k"] == 0 and 2000 < m["n"] < 2100]
    c.token(*assemble(second + filler_runs(range(1, 300), [0], 62), T0 + 5 * W, 63))
    return c


def build_C_small(extra):
    """The small path's two chunks: a rule whose head is the last element of the first chunk and that continues
    2047 (the batch has 4095 requests) or 2048 (4096: the second chunk's end) elements, ending exactly at n."""
    c = Case(f"C_small{4095 + extra}", "small", N_CHUNK_RULES, MODES["small"])
    lay = Layout(c)
    lay.pad_to(CHUNK - 1)
    lay.rule([1 + 2047 + extra], f"head on the last element of the first chunk, continues {2047 + extra} past c1 to n (small path)",
             mix="both")
    for r in lay.rows:
        c.table.append(dict(step=0, **r))
    c.fillers = [1, 2, 3]
    c.token(*assemble(lay.runs, T0, 65 + extra), n_valid=lay.pos, n_invalid=0)
    assert lay.pos == 4095 + extra
    c.token(*assemble([run(lay.next - 1, 0, 50)] + filler_runs(range(1, 300), [0], 66), T0 + 5 * W, 67))
    return c


# ------------------------------------------------------------------------------------------------ B
def build_B():
    c = Case("B_bins", "bin", N_BIN_RULES, MODES["bin"])
    prime, main = [], []

    def ids(b):
        return list(range(32 * b + 1, 32 * b + 33))

    def fill_bin(b, total, seam, rules=32, used=0, first=0):
        """Filler rules first .. of bin b up to `total` elements in the bin."""
        fl = ids(b)[first:first + rules]
        left = total - used
        per = max(1, left // len(fl))
        for j, f in enumerate(fl):
            m = per if j < len(fl) - 1 else left - per * (len(fl) - 1)
            if m > 0:
                c.set_rule(f, max(1, m // 2))
                main.append(run(f, 0, m))
                c.table.append(dict(rule=f, step=1, seam=seam, runs=[m], prio=[0], mix="both" if m > 1 else "pass",
                                    wait=False, bin=b, bin_n=total))

    fill_bin(40, 1, "a bin of one element", rules=1)
    for j, total in enumerate((K_BIN_LDS - 1, K_BIN_LDS, K_BIN_LDS + 1)):
        fill_bin(50 + j, total, f"a bin of {total} elements (LDS image up to {K_BIN_LDS}), all 32 rules present")
    for j, total in enumerate((4 * K_BO - 1, 4 * K_BO, 4 * K_BO + 1)):
        fill_bin(60 + j, total, f"a bin of {total} elements (a wave's share in registers up to {K_BO}), a single rule",
                 rules=1, first=j)
    # the R sizes in a bin that fits the LDS image (u16 run records) ...
    p, m, rows = r_specs(c, ids(80)[:11], sizes=[31, 32, 33, 63], where=" (LDS bin)")
    pz, mz, rz = r_specs(c, ids(81)[:9], sizes=[64, 65, 511], where=" (LDS bin)")
    py, my, ry = r_specs(c, ids(82)[:5], sizes=[512], where=" (LDS bin)")
    px, mx, rx = r_specs(c, ids(83)[:5], sizes=[513], where=" (LDS bin)")
    prime += p + pz + py + px
    main += m + mz + my + mx
    lds_rows = rows + rz + ry + rx
    for j, n in enumerate((2047, 2048, 2049)):
        f = ids(84 + j)[3]
        ka = n - n // 3
        c.set_rule(f, ka)
        main.append(run(f, 0, n))
        main.append(run(ids(84 + j)[9], 0, 5))
        lds_rows.append(dict(rule=f, seam=f"run of {n}, no prioritized request (LDS bin)", runs=[n], prio=[0], mix="both",
                             wait=False, first_block=ka))
    # ... and all of them in one bin that does not
    pg, mg, rows_g = r_specs(c, ids(90)[:27], where=" (global bin)")
    prime += pg
    main += mg
    far = list(range(32 * 100 + 1, N_BIN_RULES, 53))
    c.fillers = far[:3]
    c.token(*assemble(prime + filler_runs(far, [0], 3), T0, 71))
    step = c.token(*assemble(main + filler_runs(far, [0], 4), T0 + 9 * W, 72))
    assert step == 1
    bins = {}
    for m in main:
        bins[(m["rule"] - 1) >> BIN_LB] = bins.get((m["rule"] - 1) >> BIN_LB, 0) + m["n"]
    for r in lds_rows + rows_g:
        b = (r["rule"] - 1) >> BIN_LB
        assert (bins[b] <= K_BIN_LDS) == ("LDS" in r["seam"]), (r, bins[b])
        c.row(step=1, bin=b, bin_n=bins[b], **r)
    return c


def build_B_big():
    """One bin of more than 65,536 elements (what a fallback batch concentrated on 32 rules leaves the cold
    partition): ordered in global memory, every run record in the global arrays."""
    c = Case("B_big", "bin", N_BIN_RULES, MODES["bin"])
    main = []
    for j, f in enumerate(range(32 * 70 + 1, 32 * 70 + 33)):
        m = 2050 + j
        c.set_rule(f, m // 2)
        main.append(run(f, 0, m))
        c.row(f, 0, "a bin of more than 65,536 elements", [m], mix="both", wait=False, first_block=m // 2, bin=70,
              bin_n=32 * 2050 + 31 * 16)
    far = list(range(32 * 100 + 1, N_BIN_RULES, 53))
    c.fillers = far[:3]
    c.token(*assemble(main + filler_runs(far, [0], 5), T0, 75))
    return c


# ------------------------------------------------------------------------------------------------ E
def e_targets(c, ids, k_hi):
    """Escapes on the sort and the small path.  The batch starts in bucket 0 and ends in bucket k_hi."""
    ids = iter(ids)
    main, rows = [], []
    for a in (126, 127, 128):
        f = next(ids)
        c.set_rule(f, 6 * a)
        main.append(run(f, 0, 10, acq=a))
        rows.append(dict(rule=f, seam=f"acquire {a} (closed form up to {K_ACQ_MAX})", runs=[10], prio=[0], mix="both",
                         wait=False, first_block=6, escape="acquire" if a > K_ACQ_MAX else None))
    f = next(ids)
    c.set_rule(f, 3.0 * (1 << 30))
    main.append(run(f, 0, 5, acq=1 << 30))
    rows.append(dict(rule=f, seam="acquire 2^30", runs=[5], prio=[0], mix="both", wait=False, first_block=3, escape="acquire"))
    f = next(ids)
    c.set_rule(f, 30)
    acq = np.ones(40, np.int32)
    acq[20] = 2
    main.append(run(f, 0, 40, acq=acq))
    rows.append(dict(rule=f, seam="one differing acquire in the middle of a run", runs=[40], prio=[0], mix="both", wait=False,
                     first_block=29, escape="mixed"))
    for n in (32, 33):
        for cp in (0, 2):
            f = next(ids)
            c.set_rule(f, n // 2, sample=12, interval=1200)
            main.append(run(f, 0, n, prio=(n - 3, n - 1)[:cp]))
            rows.append(dict(rule=f, seam=f"sampleCount 12 (wide record), run of {n}, {cp} prioritized", runs=[n], prio=[cp],
                             mix="both", wait=False))
    for d in (K_BD_ESC - 1, K_BD_ESC, K_BD_ESC + 1):
        if d > k_hi:
            continue
        f = next(ids)
        c.set_rule(f, 4)
        main += [run(f, 0, 6), run(f, d, 9)]
        rows.append(dict(rule=f, seam=f"bucket delta {d} from the batch's base (escape from {K_BD_ESC})", runs=[6, 9],
                         prio=[0, 0], mix="both", wait=False, delta=d, escape="delta" if d >= K_BD_ESC else None))
    return main, rows


def build_E(mode):
    c = Case(f"E_{mode}", mode, N_CHUNK_RULES, MODES[mode])
    main, rows = e_targets(c, range(100, 160, 3), K_BD_ESC + 1)
    wide = {r["rule"] for r in rows if "delta" in r}  # the rules of the batch that spans 65 buckets
    near = [f for f in range(60, 200) if f not in {m["rule"] for m in main}]
    far = list(range(300, N_CHUNK_RULES, 7))
    c.fillers = near[:3]
    cut = slice(None, 60) if mode == "small" else slice(None)
    # one bucket: acquire counts, mixed acquire, sampleCount 12 (their sums are read while the bucket is in the window)
    fid, acq, prio, ts = assemble([m for m in main if m["rule"] not in wide] + filler_runs(near + far, [0], 5), T0, 81)
    assert mode != "small" or len(fid) <= 4096
    step = c.token(fid, acq, prio, ts)
    for r in rows:
        if r["rule"] not in wide:
            c.row(step=step, **r)
    # 65 buckets: bucket deltas 62 / 63 / 64 from the batch's base
    fill = filler_runs((near + far)[cut], [0, K_BD_ESC - 1, K_BD_ESC, K_BD_ESC + 1], 6)
    fid, acq, prio, ts = assemble([m for m in main if m["rule"] in wide] + fill, T0 + 2 * W, 83)
    assert mode != "small" or len(fid) <= 4096
    step = c.token(fid, acq, prio, ts)
    for r in rows:
        if r["rule"] in wide:
            c.row(step=step, **r)
    # the same rules again three buckets later: every record (wide or compact) carries what the replay left
    c.token(*assemble([dict(m, k=0) for m in main if m["k"] == 0] + filler_runs(near, [0], 7), T0 + (K_BD_ESC + 6) * W, 82))
    return c


def build_E_hot():
    """A hot-path batch of 3.3 s: the hot 1000 ms rules stay inside 64 buckets, the cold 500 ms rules (50 ms
    buckets) cross bucket delta 63 and escape to the replay."""
    c = Case("E_hotmix", "hot", N_CHUNK_RULES, dict(hot_rules=True, hot_min_requests=1, small_batch=0))
    cold = list(range(2001, 2101))
    for f in cold:
        c.set_rule(f, 4, sample=10, interval=500)
    hot = list(range(1, 1200))
    c.count[0] = 400.0
    c.fillers = [2, 3, 4]
    w = 50
    c.token(*assemble([run(1, 0, 3000), run(1, 1, 3000)] + filler_runs(hot[1:], [0, 1], 8, lo=4) + filler_runs(cold, [0, 1], 9, lo=4),
                      T0, 91, w=w))
    ks = [0, 1, 30, 31, 61, 62, 63, 64, 65]
    main = [run(f, k, 3 + (f + k) % 5) for f in cold[:12] for k in ks]
    fill = [run(1, k, 400) for k in ks] + filler_runs(hot[1:], ks[::2], 10, hi=3) + filler_runs(cold[12:], ks[:3], 11)
    step = c.token(*assemble(main + fill, T0 + 10 * W, 92, w=w), hot_mode=1, flags=0)
    for f in cold[:12]:
        c.row(f, step, f"500 ms rule beside hot 1000 ms rules: bucket deltas 61 .. 65 (escape from {K_BD_ESC})",
              [3 + (f + k) % 5 for k in ks], mix="both", wait=False, delta=65, escape="delta")
    c.row(1, step, "hot rule, 33 buckets of 100 ms in the batch", [800, 800, 400, 800, 800], mix="both", wait=False, hot=True)
    return c


# ------------------------------------------------------------------------------------------------ S
def sized_batch(c, n, t, seed, pool=400, span=20):
    """Exactly n requests at sorted times in [t, t + span] over the first `pool` rules (rule 1 the busiest)."""
    rng = np.random.default_rng(seed)
    fid = 1 + np.minimum(rng.geometric(0.02, size=n) - 1, rng.integers(0, pool, size=n)).astype(np.int64)
    if n > 40:
        fid[5::97] = 0
        fid[9::101] = c.n_rules + 999
    prio = (rng.random(n) < 0.03).astype(np.uint8)
    ts = t + (np.arange(n, dtype=np.int64) * span) // max(n, 1)
    return fid, np.ones(n, np.int32), prio, ts


def build_S(name, engine_args, sizes):
    c = Case(name, "small" if engine_args["small_batch"] else "sort", N_CHUNK_RULES, engine_args)
    c.count[0] = 60.0
    c.fillers = [2, 3, 4]
    small_max = min(engine_args["small_batch"], 4096)
    for j, n in enumerate(sizes):
        step = c.token(*sized_batch(c, n, T0 + 30 * j, 100 + j), n=n)
        c.table.append(dict(rule=-1, step=step, seam=f"batch of {n} requests: " + ("small path" if n <= small_max else "sort path"),
                            runs=[], prio=[], n=n, small=n <= small_max))
    return c


# ------------------------------------------------------------------------------------------------ P
def zipf_batch(c, n, t, seed, span=60):
    rng = np.random.default_rng(seed)
    z = rng.zipf(1.2, size=n)
    fid = np.where(z <= c.n_rules, z, rng.integers(1, c.n_rules + 1, size=n)).astype(np.int64)
    fid[3::211] = 0
    fid[5::223] = c.n_rules + 12345
    prio = (rng.random(n) < 0.01).astype(np.uint8)
    ts = t + (np.arange(n, dtype=np.int64) * span) // n
    return fid, np.ones(n, np.int32), prio, ts


def build_P(name, n_rules, nsegs):
    """Key segments of 8192 requests: every nseg once full and once with a last segment of one request.  The
    first batch only picks the hot set; from the second on the batch is on the hot path with no flag."""
    c = Case(name, "bin" if n_rules >= 28671 else "hot", n_rules, dict(hot_rules=True, hot_min_requests=64, small_batch=0),
             max_batch=max(nsegs) * SEG)
    c.count[:64] = 500.0
    c.fillers = [2, 3, 4]
    # (a one-request batch leaves no hot set behind, so it comes last)
    sizes = [3 * SEG] + [x for s in nsegs for x in (SEG * s, SEG * (s - 1) + 1) if x > 1] + ([1] if 1 in nsegs else [])
    for j, n in enumerate(sizes):
        info = dict(hot_mode=1, flags=0) if j else {}
        step = c.token(*zipf_batch(c, n, T0 + 70 * j, 200 + j), **info)
        c.table.append(dict(rule=-1, step=step, seam=f"{-(-n // SEG)} key segments, the last of {(n - 1) % SEG + 1}",
                            runs=[], prio=[], n=n, nseg=-(-n // SEG)))
    return c


# ------------------------------------------------------------------------------------------------ H
def build_H_span(nb):
    """The hot rules' buckets span nb = 64 (the batch stays hot, bd_hi - bd_lo = 63) or 65 (bucket fallback)."""
    c = Case(f"H_span{nb}", "hot", N_CHUNK_RULES, dict(hot_rules=True, hot_min_requests=1, small_batch=0))
    hot = list(range(1, 600))
    c.count[0] = 300.0
    c.fillers = [2, 3, 4]
    c.token(*assemble([run(1, 0, 2000)] + filler_runs(hot[1:], [0], 12, lo=8, hi=12), T0, 111))
    ks = [0, 1, 31, nb - 2, nb - 1]
    step = c.token(*assemble([run(1, k, 700) for k in ks] + filler_runs(hot[1:], ks, 13, hi=3), T0 + 10 * W, 112),
                   **(dict(hot_mode=1, flags=0, bd_span=K_HOT_BUCKETS - 1) if nb <= K_HOT_BUCKETS else
                      dict(hot_mode=0, flag_set=FLAG_BUCKET)))
    c.row(1, step, f"hot rule over {nb} buckets", [700] * 5, mix="both", wait=False, hot=True)
    c.token(*assemble([run(1, 0, 900)] + filler_runs(hot[1:], [0, 1], 14, hi=3), T0 + (12 + nb) * W, 113), hot_mode=1, flags=0)
    return c


def build_H_seg():
    """Prioritized requests per hot rule of 0, 1, 64, 65 and 4097 (the head bucket holds R_PRIME passes, so the
    first R_PRIME of them behind the last pass answer SHOULD_WAIT); hot buckets whose first request is request
    8191, 8192 and 8193 of the batch (k_hot_flows treats a bucket that starts on a segment boundary
    differently); a hot rule that owns all 8192 requests of a key segment and one with 8193 across two.  A rule is
    hot in a batch when the batch before held a request of it."""
    c = Case("H_seg", "hot", N_CHUNK_RULES, dict(hot_rules=True, hot_min_requests=1, small_batch=0))
    own, own2 = 10, 11
    pr = {20: 0, 21: 1, 22: 64, 23: 65, 24: 4097}
    fl = list(range(31, 400))
    c.set_rule(1, 4000)
    for f in (own, own2):
        c.set_rule(f, 5000)
    for f in pr:
        c.set_rule(f, 1500)
    c.fillers = [31, 32, 33]
    c.token(*assemble([run(f, 0, R_PRIME) for f in pr] + [run(1, 0, 50)] + filler_runs(fl, [0], 15, lo=8, hi=12), T0, 121))
    runs = [run(f, 0, 2 * cp + 1700, prio=list(range(cp + 1700, 2 * cp + 1700))) for f, cp in pr.items()]
    step = c.token(*assemble(runs + [run(1, 0, 50)] + filler_runs(fl, [0], 38, hi=3), T0 + 9 * W, 141), hot_mode=1, flags=0)
    for f, cp in pr.items():
        c.row(f, step, f"hot rule with {cp} prioritized requests", [2 * cp + 1700], [cp], mix="both", wait=cp > 0, hot=True,
              first_block=1500 - R_PRIME, waits=min(cp, R_PRIME))
    # the batch's first bucket holds exactly 8191 / 8192 / 8193 requests, so the second starts at that request
    for j, first in enumerate((SEG - 1, SEG, SEG + 1)):
        fill = filler_runs(fl, [0], 16 + j, hi=3)
        left = first - sum(m["n"] for m in fill)
        nxt = [run(own, 1, 5), run(own2, 1, 5)] if j == 2 else []
        step = c.token(*assemble(fill + [run(1, 0, left)] + filler_runs(fl, [1], 26 + j, hi=3) + [run(1, 1, 300)] + nxt,
                                 T0 + (10 + 11 * j) * W, 122 + j), hot_mode=1, flags=0, second_bucket_at=first)
        c.row(1, step, f"a hot bucket's first request is request {first} of the batch", [left, 300], mix="both", wait=False,
              hot=True)
    # one rule alone in the batch's second key segment, one over 8193 requests of the third and the fourth
    t = T0 + 45 * W
    a = [x[:SEG] for x in assemble(filler_runs(fl, [0], 36, lo=22, hi=24), t, 131, span=(0, 9))]
    assert len(a[0]) == SEG
    b = assemble([run(own, 0, SEG)], t, 132, span=(10, 19))
    d = assemble([run(own2, 0, SEG + 1)], t, 133, span=(20, 29))
    e = assemble(filler_runs(fl, [0], 37, hi=3), t, 134, span=(30, 39))
    step = c.token(*(np.concatenate(x) for x in zip(a, b, d, e)), hot_mode=1, flags=0)
    c.row(own, step, "a hot rule owning all 8192 requests of a key segment", [SEG], mix="both", wait=False, hot=True,
          at=(SEG, 2 * SEG))
    c.row(own2, step, "a hot rule with 8193 requests across two segments", [SEG + 1], mix="both", wait=False, hot=True,
          at=(2 * SEG, 3 * SEG + 1))
    return c


def build_H_pick():
    """4095, 4096 and 4097 candidate rules in one log2 count bin (8 .. 15 requests each, so no chunk of 2048 sorted
    elements holds more than 256 of them): k_hot_pick admits at most 4096 rules by a power-of-two threshold, so
    the first two batches make every rule hot and the third none (threshold 16); the fourth picks again, with the
    cold candidates' floor at half that threshold."""
    c = Case("H_pick", "hot", 6000, dict(hot_rules=True, hot_min_requests=1, small_batch=0))
    c.count[:] = 5.0
    c.fillers = [5001, 5002, 5003]
    for j, k in enumerate((K_HOT - 1, K_HOT, K_HOT + 1, 500, 500)):
        runs = [run(f, 0, 8 + (f + j) % 8) for f in range(1, k + 1)]
        step = c.token(*assemble(runs, T0 + 2 * j * W, 150 + j), **(dict(hot_mode=0 if j == 3 else 1, flags=0) if j else {}))
        c.table.append(dict(rule=-1, step=step, seam=f"{k} candidate rules in one log2 count bin", runs=[], prio=[],
                            candidates=k, hot_next=(k if k <= K_HOT else 0)))
    return c


def build_H_sample():
    """sampleCount 1, 2, 64 and 65 among the busiest rules (all with 100 ms buckets): only 2 and 64 may turn hot --
    the hot runs keep one bucket per lane and the occupy wait is 1000 / sampleCount."""
    c = Case("H_sample", "hot", N_CHUNK_RULES, dict(hot_rules=True, hot_min_requests=1, small_batch=0))
    geo = {10: 1, 11: 2, 12: 64, 13: 65}
    size = {10: 500, 11: 400, 12: 300, 13: 450}
    for f, sc in geo.items():
        c.set_rule(f, 100 if sc <= 2 else 20, sample=sc, interval=100 * sc)
    fl = list(range(31, 400))
    c.fillers = [31, 32, 33]
    for j in range(3):
        runs = [run(f, 0, n, prio=(n - 1, n - 3)) for f, n in size.items()]
        step = c.token(*assemble(runs + filler_runs(fl, [0], 160 + j, lo=8, hi=12), T0 + 70 * j * W, 165 + j),  # (7 s apart: every window starts empty)
                       **(dict(hot_mode=1, flags=0) if j else {}))
        for f, sc in geo.items():
            c.row(f, step, f"sampleCount {sc} among the busiest rules" + (": may turn hot" if 1 < sc <= 64 else ": stays cold"),
                  [size[f]], [2], mix="both", hot=bool(j and 1 < sc <= 64), sample=sc)
    return c


def build_H_prio():
    """16,383 and 16,385 prioritized hot requests in one batch (four hot rules of about 4096 each)."""
    c = Case("H_prio", "hot", N_CHUNK_RULES, dict(hot_rules=True, hot_min_requests=1, small_batch=0))
    pr = [20, 21, 22, 23]
    fl = list(range(31, 400))
    for f in pr:
        c.set_rule(f, 1500)
    c.fillers = [31, 32, 33]
    c.token(*assemble([run(f, 0, R_PRIME) for f in pr] + filler_runs(fl, [0], 170, lo=8, hi=12), T0, 171))
    for j, last in enumerate((K_HOT - 1, K_HOT + 1)):
        cps = [K_HOT, K_HOT, K_HOT, last]
        # (the second batch is eleven buckets after the first: its head bucket holds the first one's passes)
        runs = [run(f, 0, cp + 1700, prio=list(range(1700, cp + 1700))) for f, cp in zip(pr, cps)]
        step = c.token(*assemble(runs + filler_runs(fl, [0], 172 + j, hi=3), T0 + (9 + 9 * j) * W, 174 + j), hot_mode=1, flags=0,
                       n_prio=sum(cps))
        for f, cp in zip(pr, cps):
            c.row(f, step, f"{sum(cps)} prioritized hot requests in the batch", [cp + 1700], [cp], mix="both", wait=True, hot=True)
    return c


def build_H_drop():
    """A cold workgroup with 257 candidates for the next hot set (hot_min_requests = 1: every rule of the chunk):
    it publishes 256, so the next hot set holds one rule fewer than the candidates; decisions stay exact."""
    c = Case("H_drop", "hot", N_CHUNK_RULES, dict(hot_rules=True, hot_min_requests=1, small_batch=0))
    lay = Layout(c)
    for nr in (256, 257, 256):
        lens = [8] * nr
        if nr == 257:
            lens[-2:] = [4, 4]
        first = lay.next
        for m in lens:
            lay.filler(m)
        c.table.append(dict(rule=-1, step=0, seam=f"{nr} candidates in one chunk", runs=[], prio=[], chunk=lay.pos // CHUNK - 1,
                            chunk_rules=nr, first_rule=first))
    c.count[:lay.next] = 4.0
    c.fillers = [1, 2, 3]
    c.token(*assemble(lay.runs + [run(lay.next, 0, 3)], T0, 181))  # (a last rule, so that the third chunk ends on a head)
    for j in (1, 2):
        c.token(*assemble([dict(m) for m in lay.runs], T0 + 4 * j * W, 181 + j), hot_mode=1, flags=0)
    return c


# ------------------------------------------------------------------------------------------------ M
def build_M():
    """One engine of 30,000 rules: a hot-path batch (the key passes choose the cold partition), an RLS batch and a
    token batch with the hot rules off (both sorted: their cold stage must take the chunk form whatever the
    batch before chose), then the hot path again."""
    c = Case("M_mixed", "bin", N_BIN_RULES, dict(hot_rules=True, hot_min_requests=8, small_batch=0))
    c.count[:64] = 300.0
    c.fillers = [2, 3, 4]
    c.token(*zipf_batch(c, 3 * SEG + 17, T0, 301))
    rng = np.random.default_rng(302)
    z = rng.zipf(1.2, size=5000)
    fid = np.where(z <= c.n_rules, z, rng.integers(1, c.n_rules + 1, size=5000)).astype(np.int64)
    fid[7::331] = c.n_rules + 777
    c.steps.append(dict(kind="rls", fid=fid, ts=T0 + 70 + (np.arange(5000, dtype=np.int64) * 40) // 5000, info={}))
    c.steps.append(dict(kind="hot", on=False, info={}))
    c.token(*zipf_batch(c, 6001, T0 + 120, 303), hot_mode=0)
    c.steps.append(dict(kind="hot", on=True, info={}))
    c.token(*zipf_batch(c, 3 * SEG + 17, T0 + 190, 304))
    c.token(*zipf_batch(c, 2 * SEG + 5, T0 + 260, 305), hot_mode=1, flags=0)
    for s in (0, 1, 3, 5, 6):
        c.table.append(dict(rule=-1, step=s, seam="mixed paths on one engine: " +
                            {0: "hot path", 1: "RLS (sort path, simple)", 3: "sort path, hot rules off", 5: "hot path again",
                             6: "hot path with a hot set"}[s], runs=[], prio=[]))
    return c


BUILDERS = {
    **{f"R_{m}": (lambda m=m: build_R(m)) for m in MODES},
    "L_bin": build_L,
    **{f"C_{m}_inv{i}": (lambda m=m, i=i: build_C(m, i)) for m in ("sort", "hot") for i in (0, 37, 2500)},
    "C_small4095": lambda: build_C_small(0),
    "C_small4096": lambda: build_C_small(1),
    "B_bins": build_B,
    "B_big": build_B_big,
    "E_sort": lambda: build_E("sort"),
    "E_small": lambda: build_E("small"),
    "E_hotmix": build_E_hot,
    "S_small": lambda: build_S("S_small", dict(hot_rules=False, small_batch=4096), [1, 63, 64, 65, 4095, 4096, 4097]),
    "S_sort": lambda: build_S("S_sort", dict(hot_rules=False, small_batch=0), [4095, 4096, 4097]),
    "S_1000": lambda: build_S("S_1000", dict(hot_rules=False, small_batch=1000), [1000, 1001]),
    "P_part": lambda: build_P("P_part", N_BIN_RULES, [1, 8, 9, 16, 17, 64, 65]),
    "P_256": lambda: build_P("P_256", N_CHUNK_RULES, [256, 257]),
    "H_span64": lambda: build_H_span(64),
    "H_span65": lambda: build_H_span(65),
    "H_seg": build_H_seg,
    "H_pick": build_H_pick,
    "H_sample": build_H_sample,
    "H_prio": build_H_prio,
    "H_drop": build_H_drop,
    "M_mixed": build_M,
}
GROUPS = {g: [n for n in BUILDERS if n[0] == g] for g in "RLCBESPHM"}

_cases = {}


def case(name):
    """The named case, built once (a case of more than 2^20 requests: on every call, see replay)."""
    if name in _cases:
        return _cases[name]
    c = BUILDERS[name]()
    if name[0] == "H" or name == "E_hotmix":  # the next hot set, wherever the restatement reaches
        for si, s in enumerate(c.steps):
            if s["kind"] == "token" and hot_next(c, si) is not None:
                s["info"]["n_hot_next"] = hot_next(c, si)
    if c.n_requests <= 1 << 20:
        _cases[name] = c
    return c


def sorted_layout(c, step):
    """What the cold stage sees of a token batch when nothing is hot: the valid requests in a stable order by
    flowId (= slot + 1).  Returns (flowIds sorted, arrival index of each)."""
    s = c.steps[step]
    valid = (s["fid"] >= 1) & (s["fid"] <= c.n_rules) & (s["acq"] >= 1)
    idx = np.nonzero(valid)[0]
    o = np.argsort(s["fid"][idx], kind="stable")
    return s["fid"][idx][o], idx[o]


def oracle_replay(c):
    """The oracle over the case's steps, from the start: per step the (status, remaining, wait) arrays (None for
    a switch) and, read right after the step at its last request time + 1, the seven metric sums of the watched
    rules (a read rotates the rule's window as ClusterMetric.getSum does, so the engine is read at the same
    points).  Then at `now` (the last of those times) the seven sums of every other touched rule where the case
    asks for them, and BLOCK and PASS sums of every rule (the metric nodes)."""
    import ctypes as C

    from tests import oracle_harness as H
    L = H.lib()
    oh = L.orc_cluster_new(1.0, 1.0)
    arr = c.rules_array()
    L.orc_cluster_load_rules(oh, b"default", arr.ctypes.data_as(C.POINTER(H.OrcClusterRule)), len(arr))
    res, step_sums, now = [], [], T0

    def sums(rules, t):
        return {f: [int(L.orc_cluster_metric_sum(oh, f, ev, t)) for ev in range(7)] for f in rules}

    try:
        for s in c.steps:
            if s["kind"] == "hot":
                res.append(None)
                step_sums.append(None)
                continue
            n = len(s["fid"])
            out = (H.OrcTokenResult * n)()
            if s["kind"] == "rls":
                acq = np.ones(n, np.int32)
                L.orc_cluster_replay_simple(oh, n, s["fid"].ctypes.data, acq.ctypes.data, s["ts"].ctypes.data, out)
            else:
                L.orc_cluster_replay(oh, n, s["fid"].ctypes.data, s["acq"].ctypes.data, s["prio"].ctypes.data,
                                     s["ts"].ctypes.data, out)
            r = np.frombuffer(out, dtype=np.int32).reshape(n, 3)
            res.append((r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy()))
            now = max(now, int(s["ts"].max()) + 1)
            step_sums.append((now, sums(c.watched, now)))
        final = sums(c.touched(), now) if c.sum_touched else {}
        node = np.array([[L.orc_cluster_metric_sum(oh, f, 1, now), L.orc_cluster_metric_sum(oh, f, 0, now)]
                         for f in range(1, c.n_rules + 1)], np.int64)
    finally:
        L.orc_cluster_free(oh)
    return dict(results=res, step_sums=step_sums, now=now, sums=final, node=node)


_replays = {}


def replay(name):
    """oracle_replay of the named case, computed once and shared (nothing changes it); the cases of more than 2^20
    requests are computed on every call instead of being held for the whole session."""
    if name in _replays:
        return _replays[name]
    c = case(name)
    r = oracle_replay(c)
    if c.n_requests <= 1 << 20:
        _replays[name] = r
    return r


# ------------------------------------------------------------------------------------------------ dispatch forms
# the words of sga_test_cluster_dispatch (test-only build), in their order
FORM_KEYS = ("chunk", "bin", "bin_lds", "bin_global", "direct", "wave", "wg", "replay", "listfull", "global_rec", "cont",
             "gallop", "psearch", "counter", "dropped", "hot_runs", "hot_cw")


def derived_forms(got):
    """The read-back with the sums and flags predict_forms names where a single count depends on the order in
    which a workgroup's lanes reach a full list, or on how often a run's closed form asks for a prioritized count."""
    got = dict(got)
    got["wave+wg"] = got["wave"] + got["wg"]
    got["psearch>0"] = got["psearch"] > 0
    return got


def hot_history(c):
    """A restatement of the next-hot-set rule (k_hot_next_a / k_hot_pick): per step the rules hot in the NEXT token
    step, the pick threshold, and the candidates the cold workgroups dropped -- (ids, thr, dropped), or None where
    the restatement does not reach (once a workgroup dropped a candidate: which one is a matter of lane order).
    Candidates are the rules with at least hot_min_requests requests in the batch and 1 < sampleCount <= 64: the
    hot ones with their totals, the cold ones as far as a cold workgroup (2048 sorted cold elements, or a bin)
    publishes them -- at most 256 each, and only counts of at least half the last threshold.  The threshold is the
    smallest power of two that admits at most 4096 candidates (at least hot_min_requests); of those the rules with
    the bucket length of the busiest candidate are picked."""
    hist, cur, thr, known = [], np.zeros(0, np.int64), 0, True
    ea = c.engine_args
    hot_min = ea.get("hot_min_requests", 64)
    w_all = c.interval // c.sample
    for si, s in enumerate(c.steps):
        if s["kind"] == "hot":  # a switch empties the hot set
            cur = np.zeros(0, np.int64)
        if s["kind"] != "token" or not step_hot_on(c, si) or len(s["fid"]) <= min(ea["small_batch"], 4096):
            hist.append((cur, thr, 0, 0) if known else None)  # off the hot path: no pick, the set stays
            continue
        if not known:
            hist.append(None)
            continue
        ok = (s["fid"] >= 1) & (s["fid"] <= c.n_rules) & (s["acq"] >= 1)
        ids, cnt = np.unique(s["fid"][ok], return_counts=True)
        fallback = s["info"].get("hot_mode") == 0 and len(cur) > 0
        ishot = np.isin(ids, cur) & (not fallback)
        floor = max(hot_min, 1, thr >> 1)
        cand = ishot | (cnt >= floor)
        # what the cold workgroups publish
        cold_ids = ids[~ishot]
        if c.n_rules + K_HOT + 2 > 1 << 15:
            per_wg = np.zeros(1, np.int64)
        else:
            head = np.concatenate([[0], np.cumsum(cnt[~ishot])[:-1]]) if len(cold_ids) else np.zeros(0, np.int64)
            per_wg = np.bincount((head // CHUNK)[(cnt[~ishot] >= floor)], minlength=1)
        dropped = int(np.maximum(per_wg - 256, 0).sum())
        elig = (c.sample[ids - 1] > 1) & (c.sample[ids - 1] <= 64) & (cnt >= max(hot_min, 1)) & cand
        if dropped:
            known = False
            hist.append((None, None, dropped, int(elig.sum())))
            continue
        bins = np.bincount(np.floor(np.log2(cnt[elig])).astype(int), minlength=32) if elig.any() else np.zeros(32, np.int64)
        t, cum = 0xFFFFFFFF, 0
        for b in range(31, -1, -1):
            cum += int(bins[b])
            if cum <= K_HOT:
                t = 1 << b
        thr = max(t, hot_min, 1)
        if elig.any():
            k = np.lexsort((ids[elig], cnt[elig]))[-1]  # the busiest: the highest count, then the highest slot
            wbest = w_all[ids[elig][k] - 1]
            cur = ids[elig & (cnt >= thr) & (w_all[ids - 1] == wbest)]
        else:
            cur = np.zeros(0, np.int64)
        hist.append((cur, thr, 0, int(elig.sum())))
    return hist


_hist = {}


def hot_set(c, step):
    """The rules decided on the hot path in this token step (hot_history of the step before), or None."""
    if step == 0:
        return np.zeros(0, np.int64)
    if c.name not in _hist:
        _hist[c.name] = hot_history(c)
    h = _hist[c.name][step - 1]
    return None if h is None or h[0] is None else h[0]


def hot_next(c, step):
    """n_hot_next after this token step (see hot_history); with a dropped candidate, one fewer per drop where
    every candidate would have been picked."""
    if c.name not in _hist:
        _hist[c.name] = hot_history(c)
    h = _hist[c.name][step]
    if h is None:
        return None
    return len(h[0]) if h[0] is not None else h[3] - h[2]


def predict_forms(c, step, answers):
    """What sga_test_cluster_dispatch must report after the step, derived from the step's arrays and the oracle's
    answers (cw of a run = its SHOULD_WAIT answers).  Only the keys this restatement can name are returned: on a
    batch with hot rules the cold form and the hot runs; on a batch where everything is cold the whole cold stage."""
    s = c.steps[step]
    n = len(s["fid"])
    simple = s["kind"] == "rls"
    acq = np.ones(n, np.int32) if simple else s["acq"]
    prio = np.zeros(n, np.uint8) if simple else s["prio"]
    small = not simple and n <= min(c.engine_args["small_batch"], 4096)
    hot_path = not simple and not small and c.engine_args["hot_rules"] and step_hot_on(c, step)
    binned = hot_path and c.n_rules + K_HOT + 2 > 1 << 15
    out = dict(chunk=0 if binned else 1, bin=1 if binned else 0)
    valid = (s["fid"] >= 1) & (s["fid"] <= c.n_rules) & (acq >= 1)
    hs = hot_set(c, step) if hot_path and c.engine_args["hot_min_requests"] < NEVER_HOT else np.zeros(0, np.int64)
    if s["info"].get("hot_mode") == 0 and hs is not None and len(hs):
        out.update(hot_runs=0, hot_cw=0)
        return out
    if hot_path and (hs is None or len(hs)):
        if hs is not None and "hot_mode" in s["info"]:
            ishot = valid & np.isin(s["fid"], hs)
            if s["info"]["hot_mode"] == 0:
                out.update(hot_runs=0, hot_cw=0)
            else:
                key = s["fid"][ishot] * (1 << 20) + (s["ts"][ishot] // W - int(s["ts"].min()) // W)
                runs, inv = np.unique(key, return_inverse=True)
                waits = np.bincount(inv, weights=(answers[0][ishot] == 2), minlength=len(runs))
                out.update(hot_runs=len(runs), hot_cw=int((waits > 0).sum()))
        return out
    out.update(hot_runs=0, hot_cw=0)
    if not hot_path or c.engine_args["hot_min_requests"] >= NEVER_HOT:
        out["dropped"] = 0  # no rule is a candidate for the next hot set
    elif hot_next(c, step) is not None:
        out["dropped"] = _hist[c.name][step][2]
    # ---- everything is cold: the sorted elements
    idx = np.nonzero(valid)[0]
    o = np.argsort(s["fid"][idx], kind="stable")
    idx = idx[o]
    slot = s["fid"][idx] - 1
    w = (c.interval // c.sample)[slot].astype(np.int64)
    bd = np.minimum(s["ts"][idx] // w - int(s["ts"].min()) // w, K_BD_ESC)
    a7 = np.where((acq[idx] <= K_ACQ_MAX) & (bd < K_BD_ESC), acq[idx], 0)
    nv = len(idx)
    n_arr = nv if hot_path else n  # the sort and the small path keep the invalid requests as the suffix
    rk = slot * 64 + bd
    rhead = np.concatenate([[0], np.nonzero(np.diff(rk))[0] + 1])          # run heads
    rlen = np.diff(np.concatenate([rhead, [nv]]))
    fhead = np.concatenate([[0], np.nonzero(np.diff(slot))[0] + 1])        # rule heads
    fend = np.concatenate([fhead[1:], [nv]])
    amin = np.minimum.reduceat(a7, rhead)
    amax = np.maximum.reduceat(a7, rhead)
    fast = (amin == amax) & (amin > 0)
    cp = np.add.reduceat(prio[idx].astype(np.int64), rhead)
    s_run = c.sample[slot[rhead]]
    fast &= ~((cp > 0) & ((s_run <= 1) | (1000 // s_run <= 0)))  # no occupy wait to name: replayed
    wt = np.add.reduceat((answers[0][idx] == 2).astype(np.int64), rhead)
    notok = np.add.reduceat((answers[0][idx] != 0).astype(np.int64), rhead)
    if binned:
        wg_of_rule = slot[fhead] >> BIN_LB
        pop = np.bincount(slot >> BIN_LB)
        out.update(bin_lds=int(((pop > 0) & (pop <= K_BIN_LDS)).sum()), bin_global=int((pop > K_BIN_LDS).sum()), cont=0, gallop=0)
        wg_of_run = slot[rhead] >> BIN_LB
        h0 = np.zeros(int(wg_of_run.max()) + 1, np.int64)
        first = np.concatenate([[0], np.nonzero(np.diff(slot >> BIN_LB))[0] + 1])
        h0[(slot >> BIN_LB)[first]] = first
        cap = np.where(pop <= K_BIN_LDS, K_BIN_LDS, 0)[wg_of_run]
        out["global_rec"] = int((rhead - h0[wg_of_run] >= cap).sum())
    else:
        wg_of_rule = fhead // CHUNK
        out.update(bin_lds=0, bin_global=0)
        rule_of_run = np.searchsorted(fhead, rhead, side="right") - 1
        wg_of_run = wg_of_rule[rule_of_run]
        nwg = -(-nv // CHUNK)
        h0 = np.full(nwg, -1, np.int64)
        for f in fhead[::-1]:
            h0[f // CHUNK] = f
        out["global_rec"] = int((rhead - h0[wg_of_run] >= CHUNK).sum())
        cont = gallop = 0
        for g in range(nwg):
            c1 = (g + 1) * CHUNK
            if h0[g] < 0 or c1 >= nv or slot[c1] != slot[c1 - 1]:
                continue
            cont += 1
            end = fend[np.searchsorted(fhead, c1, side="right") - 1]
            gallop += 1 if end >= min(n_arr, c1 + CHUNK) else 0
        out.update(cont=cont, gallop=gallop)
    nf = np.bincount(wg_of_rule)
    out["counter"] = int(np.maximum(nf - 256, 0).sum())
    out["replay"] = int((~fast).sum())
    out["direct"] = int((fast & (rlen <= K_DIRECT)).sum())
    longer = fast & (rlen > K_DIRECT)
    listed = np.bincount(wg_of_run[longer], minlength=1)
    out["listfull"] = int(np.maximum(listed - K_LONG, 0).sum())
    out["wave+wg"] = int(np.minimum(listed, K_LONG).sum())
    huge = longer & (rlen >= K_HUGE) & (wt == 0)
    full = np.nonzero(listed > K_LONG)[0]
    if not np.isin(wg_of_run[huge], full).any():  # (which runs a full list turns away depends on the lanes' order)
        out["wg"] = int(huge.sum())
        out["wave"] = out["wave+wg"] - out["wg"]
    if not (fast & (cp > 4)).any():
        out["psearch>0"] = False
    elif (fast & (cp > 4) & (notok > 0) & (notok < rlen)).any():
        out["psearch>0"] = True
    return out


def step_hot_on(c, step):
    on = c.engine_args["hot_rules"]
    for s in c.steps[:step]:
        if s["kind"] == "hot":
            on = s["on"]
    return on
