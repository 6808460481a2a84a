#!/usr/bin/env python3
"""Usage (GPU box): python3 tools/metric_ext_bench.py [--shape a|b|ab] [--legs all|off] [--rounds R] [--steps S]
                                                     [--out DIR]

The metric extension measurements of DESIGN.md section 5 (profiles/metric_ext/ab.jsonl, summary.txt), after
tools/blocklog_bench.py.

Shapes, one device-entry chunk of 2^20 events each, entries and exits alternating (an exit follows its entry, with
SGA_EV_ERROR on one exit in sixteen and rt in 0..8,191 ms; the chunk is formed before its decisions are known, so in
shape b a blocked entry is followed by an exit too -- load, not a faithful caller):
  a  one resource, no rule: every entry passes, every event lands on one line -- the contention case
  b  2^16 resources under Zipf(1.1), a QPS rule per resource at half its expected entries a second, four seconds:
     a large share of the entries blocks

Legs, each on an engine of its own fed the same chunks, alternating step by step in this one process:
  off   the sums off
  on    the sums on (k_mx_add after k_lfail); the drain is timed apart (drain_ms)
  host  the sums off, then decision and wait copied to the host and reduced there with numpy together with the
        input columns -- the only way to have these sums without the feature (the input columns are taken as
        already on the host, which favours this leg)
Host clock around the call and the stream wait.  One warm-up round, then R rounds of S steps a leg (2 S for shape a,
whose one draw serves every step -- but whose chunk takes the engine over a second, sums on or off: the recorded run
used --steps 2 for it and --steps 10 for shape b); a leg's figure is the median over its steps, its spread the range of its per-round medians.
--legs off runs the first leg alone: with SGA_LIB_VARIANT=parent (a build of the parent commit) that is the
disabled path's comparison."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sentinel_amd import _lib  # noqa: E402
from sentinel_amd.cluster import Engine  # noqa: E402
from sentinel_amd.local import FlowRuleManager, LocalSentinel  # noqa: E402
from sentinel_amd.rules import FlowRule  # noqa: E402

N, T0 = 1 << 20, 1_700_000_000_000
H = N // 2
BLOCKS = np.asarray([1, 2, 3, 5, 6], dtype=np.int8)


def shape(name, rng):
    """(n_res, rules, span_ms, draw): draw() -> (resource int32, ts_off int32 sorted) of one chunk; event 2k is an
    entry, event 2k + 1 its exit."""
    if name == "a":  # one draw serves every step (the chunks differ in their base time only)
        once = (np.zeros(N, np.int32), np.sort(rng.integers(0, 1000, size=N)).astype(np.int32))
        return 1, [], 1000, lambda: once
    n_res, span = 1 << 16, 4000
    p = 1.0 / np.arange(1, n_res + 1) ** 1.1
    p /= p.sum()
    perm = rng.permutation(n_res)
    per_sec = H * p / (span / 1000)
    rules = [FlowRule(resource=f"r{perm[k]}", count=float(np.floor(per_sec[k] / 2))) for k in range(n_res)]
    return n_res, rules, span, lambda: (
        np.repeat(perm[rng.choice(n_res, size=H, p=p)], 2).astype(np.int32),
        np.sort(rng.integers(0, span, size=N)).astype(np.int32))


def host_reduce(n_res, kind, res, acq, flags, rt, d, w):
    """The sums formed on the host: the eight per-resource sums and the block rows."""
    ent, ex = kind == 0, kind == 1
    ps = ent & ((d == 0) | (d == 4))
    er = ex & ((flags & 2) != 0)
    out = np.zeros((8, n_res), np.int64)
    out[0] = np.bincount(res[ps], weights=acq[ps], minlength=n_res)
    out[1] = np.bincount(res[ps], minlength=n_res)
    out[2] = np.bincount(res[ex], weights=acq[ex], minlength=n_res)
    out[3] = np.bincount(res[ex], minlength=n_res)
    out[4] = np.bincount(res[er], weights=acq[er], minlength=n_res)
    out[5] = np.bincount(res[er], minlength=n_res)
    out[6] = np.bincount(res[ex], weights=rt[ex], minlength=n_res)
    if ex.any():  # the largest rt per resource: a stable sort by resource, then a segmented maximum
        o = np.argsort(res[ex], kind="stable")
        rs, rv = res[ex][o], rt[ex][o]
        starts = np.flatnonzero(np.r_[True, rs[1:] != rs[:-1]])
        out[7][rs[starts]] = np.maximum(0, np.maximum.reduceat(rv, starts))
    m = ent & np.isin(d, BLOCKS)
    key = (res[m].astype(np.int64) << 24) | (d[m].astype(np.int64) << 20) | w[m].astype(np.int64)
    uniq, inv = np.unique(key, return_inverse=True)
    return out, uniq, np.bincount(inv, weights=acq[m]).astype(np.int64), np.bincount(inv)


def run(name, legs, rounds, steps, out):
    import torch
    rng = np.random.default_rng(2024)
    n_res, rules, span, draw = shape(name, rng)
    if name == "a":
        steps *= 2  # no draw between the steps: more of them for the same wall time
    dev = torch.device("cuda", 0)
    sents = {}
    for leg in legs:
        eng = Engine(max_batch=N)
        eng.set_small_batch(0)
        s = LocalSentinel(eng, [f"r{i}" for i in range(n_res)], metric_extensions=(1 << 20) if leg == "on" else False)
        assert FlowRuleManager(s).load_rules(rules) == len(rules)
        sents[leg] = (eng, s)
    i = np.arange(N)
    kind_h = (i % 2).astype(np.uint8)
    acq_h = np.where((i // 2) % 3 == 0, 3, 1).astype(np.int32)
    flags_h = np.where((i % 2 == 1) & ((i // 2) % 16 == 0), 2, 0).astype(np.uint8)
    rt_h = np.where(i % 2 == 1, (i * 2654435761) % 8192, 0).astype(np.int64)
    kind, acq = torch.from_numpy(kind_h).to(dev), torch.from_numpy(acq_h).to(dev)
    flags, rt = torch.from_numpy(flags_h).to(dev), torch.from_numpy(rt_h).to(dev)
    ms = {leg: [] for leg in legs}
    drain_ms, rows_n, info = [], [], {}
    for step in range((rounds + 1) * steps):
        res_h, off_h = draw()
        res, off = torch.from_numpy(res_h).to(dev), torch.from_numpy(off_h).to(dev)
        base = T0 + span * step
        if step % steps == 0:
            print(f"shape {name}: round {step // steps} of {rounds} + 1", file=sys.stderr, flush=True)
        for leg in legs:
            s = sents[leg][1]
            torch.cuda.synchronize()
            t = time.perf_counter()
            d, w = s.submit_device(kind, res, base, off, acq, flags=flags, rt=rt)
            s.device_status()
            if leg == "host":
                agg = host_reduce(n_res, kind_h, res_h, acq_h, flags_h, rt_h, d.cpu().numpy(), w.cpu().numpy())
            ms[leg].append((time.perf_counter() - t) * 1e3)
            if leg == "on":
                t = time.perf_counter()
                rr, br, le, lc = s.metric_ext_rows()
                drain_ms.append((time.perf_counter() - t) * 1e3)
                rows_n.append((len(rr), len(br)))
                info.update({"res_rows": len(rr), "block_rows": len(br), "lost_events": le,
                             "pass": int(rr["pass"].sum()), "success": int(rr["success"].sum()),
                             "rt_sum": int(rr["rt_sum"].sum()), "block": int(br["block"].sum()) + lc})
            elif leg == "host":
                info.update({"host_res_rows": int((agg[0] != 0).any(axis=0).sum()), "host_block_rows": len(agg[1]),
                             "host_pass": int(agg[0][0].sum()), "host_success": int(agg[0][2].sum()),
                             "host_rt_sum": int(agg[0][6].sum()), "host_block": int(agg[2].sum())})
            else:
                dh = d.cpu().numpy()
                info["blocked_share_of_entries"] = round(float(np.isin(dh[kind_h == 0], BLOCKS).mean()), 4)
    res = {"shape": name, "lib": os.path.basename(_lib.LIB_PATH), "events": N, "rounds": rounds, "steps": steps}
    for leg in legs:
        x = np.asarray(ms[leg][steps:]).reshape(rounds, steps)
        per_round = np.median(x, axis=1)
        res[leg] = {"median_ms": round(float(np.median(x)), 3),
                    "round_medians_ms": [round(float(v), 3) for v in per_round],
                    "spread_ms": round(float(per_round.max() - per_round.min()), 3),
                    "timed_s": round(float(x.sum()) / 1e3, 3)}
    if "on" in legs:
        res["on"]["drain_median_ms"] = round(float(np.median(drain_ms[steps:])), 3)
        res["on"]["res_rows_per_drain"] = int(np.median([r[0] for r in rows_n[steps:]]))
        res["on"]["block_rows_per_drain"] = int(np.median([r[1] for r in rows_n[steps:]]))
    res["last_chunk"] = info
    for eng, _ in sents.values():
        eng.close()
    line = json.dumps(res)
    print(line, flush=True)
    with open(os.path.join(out, "ab.jsonl"), "a") as f:
        f.write(line + "\n")
    return res


def summary(results, out):
    lines = []
    for r in results:
        lines.append(f"shape {r['shape']} ({r['lib']}): {r['events']} events a chunk, {r['rounds']} rounds x "
                     f"{r['steps']} steps a leg; last chunk {r['last_chunk']}")
        for leg in ("off", "on", "host"):
            if leg in r:
                lines.append(f"  {leg:4s} median {r[leg]['median_ms']:8.3f} ms   spread of round medians "
                             f"{r[leg]['spread_ms']:.3f} ms   timed {r[leg]['timed_s']} s")
        if "on" in r and "host" in r:
            lines.append(f"  on - off = {r['on']['median_ms'] - r['off']['median_ms']:.3f} ms (+ drain "
                         f"{r['on']['drain_median_ms']:.3f} ms for {r['on']['res_rows_per_drain']} + "
                         f"{r['on']['block_rows_per_drain']} rows);  host - off = "
                         f"{r['host']['median_ms'] - r['off']['median_ms']:.3f} ms")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(os.path.join(out, "summary.txt"), "a") as f:
        f.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ab")
    ap.add_argument("--legs", default="all", choices=["all", "off"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "metric_ext"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    legs = ["off", "on", "host"] if a.legs == "all" else ["off"]
    summary([run(sh, legs, a.rounds, a.steps, a.out) for sh in a.shape], a.out)
