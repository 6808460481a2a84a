#!/usr/bin/env python3
"""Usage (GPU box): python3 tools/cb_events_bench.py [--shape a|b|ab] [--legs all|off] [--rounds R] [--steps S]
                                                    [--out DIR]

The breaker-event measurements of DESIGN.md section 5 (profiles/cb_events/ab.jsonl, summary.txt).

Shapes, one device-entry chunk of 2^20 events each:
  a  breaker-only: 2^12 resources, one exception-ratio breaker each (threshold 0.5), every step a chunk of entries
     followed by a chunk of their exits, 1 % of which fail -- almost nothing transitions
  b  the worst case: one resource with two breakers, both OPEN, the first due for retry and the second not; every
     entry of the chunk moves the first to HALF_OPEN and, blocked by the second, back to OPEN: two records an entry.
     The resource is decided in arrival order by one lane (two breakers: the generic replay), so the chunk is 2^14
     entries; the log's capacity is twice that

Legs, each on an engine of its own fed the same chunks, alternating step by step in this one process:
  off   the log off
  on    the log on; the drain after the chunk is timed apart (drain_ms)
Host clock around the call and the stream wait.  One warm-up round, then R rounds of S steps a leg (20 S for shape a,
whose step is two thirds of a millisecond); a leg's figure is
the median over its steps, its spread the range of its per-round medians.  --legs off runs the first leg alone: with
SGA_LIB_VARIANT=parent (a build of the parent commit) that is the disabled path's comparison."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sentinel_amd import _lib  # noqa: E402
from sentinel_amd.cluster import Engine  # noqa: E402
from sentinel_amd.local import DegradeRuleManager, LocalSentinel  # noqa: E402
from sentinel_amd.rules import DegradeRule  # noqa: E402

T0 = 1_700_000_000_000


def make(name, leg, n):
    """An engine of shape `name` ready for its timed chunks; shape b's breakers are opened here."""
    n_res = 1 << 12 if name == "a" else 1
    eng = Engine(max_batch=n)
    eng.set_small_batch(0)
    s = LocalSentinel(eng, [f"r{i}" for i in range(n_res)])
    if name == "a":
        rules = [DegradeRule(resource=f"r{i}", grade=1, count=0.5, time_window=10, min_request_amount=5,
                             stat_interval_ms=1000) for i in range(n_res)]
    else:  # one failing request opens both; the first retries after 1 s, the second after an hour
        rules = [DegradeRule(resource="r0", grade=2, count=0, time_window=w, min_request_amount=1,
                             stat_interval_ms=1000) for w in (1, 3600)]
    assert DegradeRuleManager(s).load_rules(rules) == len(rules)
    if name == "b":
        s.submit([0, 1], [0, 0], [T0, T0 + 1], [1, 1], [0, 2], [0, 1])
        assert [s.circuit_breaker_state(0, k) for k in range(2)] == [1, 1]
    if leg == "on" and hasattr(s, "enable_breaker_events"):
        s.enable_breaker_events(max(1 << 16, 2 * n))
    return eng, s


def run(name, legs, rounds, steps, out):
    import torch
    rng = np.random.default_rng(2024)
    n = 1 << 20 if name == "a" else 1 << 14
    if name == "a":
        steps *= 20  # a sub-millisecond step: more of them for the same timed window
    dev = torch.device("cuda", 0)
    sents = {leg: make(name, leg, n) for leg in legs}
    acq = torch.ones(n, dtype=torch.int32, device=dev)
    ent = torch.zeros(n, dtype=torch.uint8, device=dev)
    ext = torch.ones(n, dtype=torch.uint8, device=dev)
    rt = torch.ones(n, dtype=torch.int64, device=dev)
    ms = {leg: [] for leg in legs}
    drain_ms, recs_n, info = [], [], {}
    for step in range((rounds + 1) * steps):
        base = T0 + 2000 + 1000 * step
        if name == "a":
            res = torch.from_numpy(rng.integers(0, 1 << 12, size=n).astype(np.int32)).to(dev)
            off = torch.from_numpy(np.sort(rng.integers(0, 400, size=n)).astype(np.int32)).to(dev)
            fl = torch.from_numpy(((rng.random(n) < 0.01) * 2).astype(np.uint8)).to(dev)
            chunks = [(ent, off, None), (ext, off + 500, fl)]
        else:
            res = torch.zeros(n, dtype=torch.int32, device=dev)
            off = torch.from_numpy(np.sort(rng.integers(0, 1000, size=n)).astype(np.int32)).to(dev)
            chunks = [(ent, off, None)]
        for leg in legs:
            s = sents[leg][1]
            torch.cuda.synchronize()
            t = time.perf_counter()
            for kind, o, f in chunks:
                d, w = s.submit_device(kind, res, base, o, acq, flags=f, rt=rt)
            s.device_status()
            ms[leg].append((time.perf_counter() - t) * 1e3)
            if leg == "on":
                t = time.perf_counter()
                recs, lost = s.breaker_event_records()
                drain_ms.append((time.perf_counter() - t) * 1e3)
                recs_n.append(len(recs))
                info.update({"records": len(recs), "lost": lost})
            else:
                info["blocked_share"] = round(float((d.cpu().numpy() == 3).mean()), 4)
    res = {"shape": name, "lib": os.path.basename(_lib.LIB_PATH), "events": n * len(chunks), "rounds": rounds,
           "steps": steps}
    for leg in legs:
        x = np.asarray(ms[leg][steps:]).reshape(rounds, steps)
        per_round = np.median(x, axis=1)
        res[leg] = {"median_ms": round(float(np.median(x)), 3), "round_medians_ms": [round(float(v), 3) for v in per_round],
                    "spread_ms": round(float(per_round.max() - per_round.min()), 3),
                    "timed_s": round(float(x.sum()) / 1e3, 3)}
    if "on" in legs:
        res["on"]["drain_median_ms"] = round(float(np.median(drain_ms[steps:])), 3)
        res["on"]["records_per_drain"] = int(np.median(recs_n[steps:]))
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
        lines.append(f"shape {r['shape']} ({r['lib']}): {r['events']} events a step, {r['rounds']} rounds x "
                     f"{r['steps']} steps a leg; last chunk {r['last_chunk']}")
        for leg in ("off", "on"):
            if leg in r:
                lines.append(f"  {leg:4s} median {r[leg]['median_ms']:8.3f} ms   spread of round medians "
                             f"{r[leg]['spread_ms']:.3f} ms   timed {r[leg]['timed_s']} s")
        if "on" in r:
            lines.append(f"  on - off = {r['on']['median_ms'] - r['off']['median_ms']:.3f} ms (+ drain "
                         f"{r['on']['drain_median_ms']:.3f} ms for {r['on']['records_per_drain']} records)")
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
                                                  "profiles", "cb_events"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    legs = ["off", "on"] if a.legs == "all" else ["off"]
    summary([run(sh, legs, a.rounds, a.steps, a.out) for sh in a.shape], a.out)
