#!/usr/bin/env python3
"""Usage (GPU box): python3 tools/blocklog_bench.py [--shape a|b|ab] [--legs all|off] [--rounds R] [--steps S]
                                                   [--out DIR]

The block-log measurements of DESIGN.md section 5 (profiles/blocklog/ab.jsonl, summary.txt).

Shapes, one device-entry chunk of 2^20 entries each:
  a  one resource, one count-0 QPS rule, one second: every entry blocks on one key -- the contention case
  b  2^16 resources under Zipf(1.1), a QPS rule per resource at half its expected entries a second, four seconds

Legs, each on an engine of its own fed the same chunks, alternating step by step in this one process:
  off   the log off
  on    the log on (k_blog_add after k_lfail); the drain of the finished seconds is timed apart (drain_ms)
  host  the log off, then decision and wait copied to the host and aggregated there with numpy -- the only way to
        keep a block log without the feature (the input columns are taken as already on the host, which favours
        this leg)
Host clock around the call and the stream wait.  One warm-up round, then R rounds of S steps a leg (5 S for shape a,
whose chunk is a third of a millisecond); a leg's figure
is the median over its steps, its spread the range of its per-round medians.  --legs off runs the first leg alone:
with SGA_LIB_VARIANT=parent (a build of the parent commit) that is the disabled path's comparison."""
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
BLOCKS = np.asarray([1, 2, 3, 5, 6], dtype=np.int8)


def shape(name, rng):
    """(n_res, rules, span_ms, draw): draw() -> (resource int32, ts_off int32 sorted) of one chunk."""
    if name == "a":  # one draw serves every step (the chunks differ in their base time only); 5 x the steps
        once = (np.zeros(N, np.int32), np.sort(rng.integers(0, 1000, size=N)).astype(np.int32))
        return 1, [FlowRule(resource="r0", count=0.0)], 1000, lambda: once
    n_res, span = 1 << 16, 4000
    p = 1.0 / np.arange(1, n_res + 1) ** 1.1
    p /= p.sum()
    perm = rng.permutation(n_res)
    per_sec = N * p / (span / 1000)
    rules = [FlowRule(resource=f"r{perm[k]}", count=float(np.floor(per_sec[k] / 2))) for k in range(n_res)]
    return n_res, rules, span, lambda: (
        perm[rng.choice(n_res, size=N, p=p)].astype(np.int32), np.sort(rng.integers(0, span, size=N)).astype(np.int32))


def host_aggregate(res, ts_base, off, acq, d, w):
    """The block log formed on the host: (time_slot, resource, decision, detail) -> (count, events)."""
    m = np.isin(d, BLOCKS)
    slot = (ts_base + off[m].astype(np.int64)) // 1000
    key = (((slot - slot.min()) << 48) | (res[m].astype(np.int64) << 24) | (d[m].astype(np.int64) << 20) |
           w[m].astype(np.int64))
    uniq, inv = np.unique(key, return_inverse=True)
    return uniq, np.bincount(inv, weights=acq[m]).astype(np.int64), np.bincount(inv)


def run(name, legs, rounds, steps, out):
    import torch
    rng = np.random.default_rng(2024)
    n_res, rules, span, draw = shape(name, rng)
    if name == "a":
        steps *= 5  # a sub-millisecond chunk: more of them for the same timed window
    dev = torch.device("cuda", 0)
    sents = {}
    for leg in legs:
        eng = Engine(max_batch=N)
        eng.set_small_batch(0)
        s = LocalSentinel(eng, [f"r{i}" for i in range(n_res)], block_log=(1 << 20) if leg == "on" else False)
        assert FlowRuleManager(s).load_rules(rules) == n_res
        sents[leg] = (eng, s)
    kind = torch.zeros(N, dtype=torch.uint8, device=dev)
    acq_h = np.where(np.arange(N) % 3 == 0, 3, 1).astype(np.int32)
    acq = torch.from_numpy(acq_h).to(dev)
    ms = {leg: [] for leg in legs}
    drain_ms, rows_n, info = [], [], {}
    for step in range((rounds + 1) * steps):
        res_h, off_h = draw()
        res, off = torch.from_numpy(res_h).to(dev), torch.from_numpy(off_h).to(dev)
        base = T0 + span * step
        for leg in legs:
            s = sents[leg][1]
            torch.cuda.synchronize()
            t = time.perf_counter()
            d, w = s.submit_device(kind, res, base, off, acq)
            s.device_status()
            if leg == "host":
                agg = host_aggregate(res_h, base, off_h, acq_h, d.cpu().numpy(), w.cpu().numpy())
            ms[leg].append((time.perf_counter() - t) * 1e3)
            if leg == "on":
                t = time.perf_counter()
                rows, le, lc = s.block_rows(base + span)
                drain_ms.append((time.perf_counter() - t) * 1e3)
                rows_n.append(len(rows))
                info.update({"rows": len(rows), "lost_events": le, "count": int(rows["count"].sum()) + lc})
            elif leg == "host":
                info.update({"host_rows": len(agg[0]), "host_count": int(agg[1].sum())})
            else:
                info["blocked_share"] = round(float(np.isin(d.cpu().numpy(), BLOCKS).mean()), 4)
    res = {"shape": name, "lib": os.path.basename(_lib.LIB_PATH), "events": N, "rounds": rounds, "steps": steps}
    for leg in legs:
        x = np.asarray(ms[leg][steps:]).reshape(rounds, steps)
        per_round = np.median(x, axis=1)
        res[leg] = {"median_ms": round(float(np.median(x)), 3), "round_medians_ms": [round(float(v), 3) for v in per_round],
                    "spread_ms": round(float(per_round.max() - per_round.min()), 3),
                    "timed_s": round(float(x.sum()) / 1e3, 3)}
    if "on" in legs:
        res["on"]["drain_median_ms"] = round(float(np.median(drain_ms[steps:])), 3)
        res["on"]["rows_per_drain"] = int(np.median(rows_n[steps:]))
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
        lines.append(f"shape {r['shape']} ({r['lib']}): {r['events']} entries a chunk, {r['rounds']} rounds x "
                     f"{r['steps']} steps a leg; last chunk {r['last_chunk']}")
        for leg in ("off", "on", "host"):
            if leg in r:
                lines.append(f"  {leg:4s} median {r[leg]['median_ms']:8.3f} ms   spread of round medians "
                             f"{r[leg]['spread_ms']:.3f} ms   timed {r[leg]['timed_s']} s")
        if "on" in r and "host" in r:
            lines.append(f"  on - off = {r['on']['median_ms'] - r['off']['median_ms']:.3f} ms (+ drain "
                         f"{r['on']['drain_median_ms']:.3f} ms for {r['on']['rows_per_drain']} rows);  host - off = "
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
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "blocklog"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    legs = ["off", "on", "host"] if a.legs == "all" else ["off"]
    summary([run(sh, legs, a.rounds, a.steps, a.out) for sh in a.shape], a.out)
