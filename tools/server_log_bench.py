#!/usr/bin/env python3
"""Usage (GPU box): python3 tools/server_log_bench.py [--shape hot|spread|both] [--legs all|off] [--rounds R]
                                                     [--steps S] [--out DIR] [--tag NAME]

The token server log measurements of DESIGN.md section 3 (profiles/server_log/*.jsonl, summary.txt).

Shapes, one packed device batch (sga_request_tokens_packed_device) of 2^22 requests each, C3's rule geometry
(GLOBAL, sampleCount 10, 1000 ms) and 1 % prioritized requests:
  hot     2^17 rules, flowId ~ Zipf(1.1), counts U{10..10000}: the blocks concentrate on the few hot rules
  spread  2^17 rules, flowId uniform, count 8: about 32 requests a rule and batch, blocks on about 10^5 rules

Legs, each on an engine of its own fed the same batches, alternating step by step in this one process:
  off   the log off
  on    the log on (k_slog_add behind the batch); the drain of the finished seconds is timed apart (drain_ms)
  host  the log off, then the 8-byte results copied to the host and reduced there with numpy -- the only way to
        keep a server log without the feature (the request columns are taken as already on the host, which favours
        this leg)
Host clock around the call and sga_sync.  One warm-up round, then R rounds of S steps a leg; a leg's figure is the
median over its steps, its spread the range of its per-round medians.  --legs off runs the first leg alone: with
SGA_LIB_VARIANT=parent (a build of the parent commit as sentinel_amd/libsentinel_amd_parent.so) that is the disabled
path's comparison, run as alternating processes (--tag names the process in off_<lib>.jsonl)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sentinel_amd import _lib  # noqa: E402
from sentinel_amd.cluster import ClusterFlowRuleManager, Engine  # noqa: E402

N, T0, N_RULES, SPAN = 1 << 22, 1_700_000_000_000, 1 << 17, 1000


def shape(name, rng):
    """(rule counts, flowId per request uint32): one draw serves every step (the batches differ in base time)."""
    if name == "hot":
        p = 1.0 / np.arange(1, N_RULES + 1) ** 1.1
        p /= p.sum()
        perm = rng.permutation(N_RULES)
        fid = perm[rng.choice(N_RULES, size=N, p=p)] + 1
        return rng.integers(10, 10001, size=N_RULES).astype(np.float64), fid.astype(np.uint32)
    return np.full(N_RULES, 8.0), rng.integers(1, N_RULES + 1, size=N).astype(np.uint32)


def host_reduce(fid, prio, acq, ts, res):
    """The server log formed on the host: (second, flowId, kind) -> (count, events) over the copied-back results."""
    st = (res >> np.uint64(48)).astype(np.uint8).view(np.int8)
    m = (st == 1) | (st == 2)
    kind = np.where(st[m] == 2, 2, prio[m].astype(np.int64))
    slot = ts[m] // 1000
    key = ((slot - slot.min()) << 40) | (fid[m].astype(np.int64) << 8) | kind
    uniq, inv = np.unique(key, return_inverse=True)
    add = np.where(kind == 2, 1, acq[m])
    return uniq, np.bincount(inv, weights=add).astype(np.int64), np.bincount(inv)


def run(name, legs, rounds, steps, out, tag):
    import torch
    L = _lib.load()
    rng = np.random.default_rng(2025)
    counts, fid_h = shape(name, rng)
    dev = torch.device("cuda", 0)
    engs = {}
    for leg in legs:
        eng = Engine(max_batch=N, max_rules=2 * N_RULES)
        ClusterFlowRuleManager(eng).load_rule_arrays("default", np.arange(1, N_RULES + 1, dtype=np.int64), counts)
        if leg == "on":
            eng.server_log_enable(1 << 20)
        engs[leg] = eng
    off_h = np.sort(rng.integers(0, SPAN, size=N)).astype(np.uint32)
    prio_h = (rng.random(N) < 0.01).astype(np.uint32)
    acq_h = np.ones(N, np.int64)
    rec = np.stack([fid_h, off_h, np.uint32(1) | (prio_h << 16)], axis=1).astype(np.uint32)
    d_req = torch.from_numpy(rec.view(np.int32)).to(dev)
    d_out = {leg: torch.zeros(N, dtype=torch.int64, device=dev) for leg in legs}
    ms = {leg: [] for leg in legs}
    drain_ms, rows_n, info = [], [], {}
    for step in range((rounds + 1) * steps):
        base = T0 + SPAN * step
        for leg in legs:
            eng = engs[leg]
            torch.cuda.synchronize()
            t = time.perf_counter()
            rc = L.sga_request_tokens_packed_device(eng.handle, d_req.data_ptr(), base, N, d_out[leg].data_ptr(), None)
            assert rc == 0 and L.sga_sync(eng.handle) == 0
            if leg == "host":
                agg = host_reduce(fid_h, prio_h, acq_h, base + off_h.astype(np.int64),
                                  d_out[leg].cpu().numpy().view(np.uint64))
            ms[leg].append((time.perf_counter() - t) * 1e3)
            if leg == "on":
                t = time.perf_counter()
                rows, le, lc = eng.server_log_rows(base + SPAN)
                drain_ms.append((time.perf_counter() - t) * 1e3)
                rows_n.append(len(rows))
                info.update({"rows": len(rows), "lost_events": le, "events": int(rows["events"].sum()) + le})
            elif leg == "host":
                info.update({"host_rows": len(agg[0]), "host_events": int(agg[2].sum())})
            else:
                st = (d_out[leg].cpu().numpy().view(np.uint64) >> np.uint64(48)).astype(np.uint8).view(np.int8)
                info["logged_share"] = round(float(((st == 1) | (st == 2)).mean()), 4)
    res = {"shape": name, "lib": os.path.basename(_lib.LIB_PATH), "tag": tag, "requests": N, "rounds": rounds,
           "steps": steps}
    for leg in legs:
        x = np.asarray(ms[leg][steps:]).reshape(rounds, steps)
        per_round = np.median(x, axis=1)
        res[leg] = {"median_ms": round(float(np.median(x)), 3),
                    "round_medians_ms": [round(float(v), 3) for v in per_round],
                    "spread_ms": round(float(per_round.max() - per_round.min()), 3)}
    if "on" in legs:
        res["on"]["drain_median_ms"] = round(float(np.median(drain_ms[steps:])), 3)
        res["on"]["rows_per_drain"] = int(np.median(rows_n[steps:]))
    res["last_batch"] = info
    for eng in engs.values():
        eng.close()
    line = json.dumps(res)
    print(line, flush=True)
    fname = "ab.jsonl" if len(legs) > 1 else "off_%s.jsonl" % os.path.basename(_lib.LIB_PATH)[:-3]
    with open(os.path.join(out, fname), "a") as f:
        f.write(line + "\n")
    return res


def summary(results, out):
    lines = []
    for r in results:
        lines.append(f"shape {r['shape']} ({r['lib']} {r['tag']}): {r['requests']} requests a batch, {r['rounds']} "
                     f"rounds x {r['steps']} steps a leg; last batch {r['last_batch']}")
        for leg in ("off", "on", "host"):
            if leg in r:
                lines.append(f"  {leg:4s} median {r[leg]['median_ms']:8.3f} ms   round medians "
                             f"{r[leg]['round_medians_ms']}   spread {r[leg]['spread_ms']:.3f} ms")
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
    ap.add_argument("--shape", default="both", choices=["hot", "spread", "both"])
    ap.add_argument("--legs", default="all", choices=["all", "off"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "server_log"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    legs = ["off", "on", "host"] if a.legs == "all" else ["off"]
    shapes = ["hot", "spread"] if a.shape == "both" else [a.shape]
    summary([run(sh, legs, a.rounds, a.steps, a.out, a.tag) for sh in shapes], a.out)
