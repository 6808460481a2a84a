#!/usr/bin/env python3
"""Usage (GPU box): python3 tools/authority_bench.py kernel | chunk rules|premarked|norules

The AuthoritySlot measurements of DESIGN.md section 5 (profiles/authority/).

kernel: sga_authority_check over 2^20 (resource, origin) pairs -- one full chunk of k_authority -- with every
        resource black-listing 1, 8 and then 1024 origins: 3 warm-ups and 10 timed launches per list length, in that
        order.  The kernel's time is read from the trace of
            rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/authority_bench.py kernel
        (the k_authority rows in dispatch order, 13 per list length); the host clock printed here includes the two
        copies in and the copy out.
chunk:  a C2-like device-entry chunk with origins: 100,000 resources under C2's rule mix (40 % Default, 30 %
        RateLimiter 500 ms, 30 % WarmUp 10 s; bench_local.py _cfg_c2), Zipf(1.1) over the resources, 2^20 entries a
        chunk, 4 origins of which the last carries about 1 % of the entries.
          rules:     every resource black-lists the last origin; the events are all kind 0
          premarked: no AuthorityRule; the host has marked the last origin's entries kind 2 (what a caller had to do
                     before the engine ran the slot: runs on a build without it, SGA_LIB_VARIANT=parent)
          norules:   no AuthorityRule, all kind 0 (the launch guard: the kernels of a build without the slot)
        Host clock around the call and the stream wait, 3 warm-ups, then 7 timed chunks: one JSON line.  Alternate
        the processes of the builds under comparison and take medians over the processes."""
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


def kernel():
    from sentinel_amd.local import AuthorityRuleManager
    from sentinel_amd.rules import AuthorityRule
    n_res, n_org = 1024, 2048
    eng = Engine(max_batch=N)
    s = LocalSentinel(eng, [f"r{i}" for i in range(n_res)], [f"o{i}" for i in range(1, n_org + 1)], max_origin_nodes=64)
    rng = np.random.default_rng(7)
    res = rng.integers(0, n_res, size=N).astype(np.uint32)
    org = rng.integers(1, n_org + 1, size=N).astype(np.uint32)
    for length in (1, 8, 1024):
        # every resource lists `length` distinct origins of its own, in a shuffled order
        rules = [AuthorityRule(f"r{r}", ",".join(f"o{i}" for i in rng.choice(n_org, size=length, replace=False) + 1), 1)
                 for r in range(n_res)]
        assert AuthorityRuleManager(s).load_rules(rules) == n_res
        times = []
        for _ in range(13):
            t = time.perf_counter()
            ok = s.authority_check(res, org)
            times.append((time.perf_counter() - t) * 1e3)
        print(json.dumps({"mode": "kernel", "list": length, "blocked": int((~ok).sum()),
                          "host_ms_median_of_last_10": round(float(np.median(times[3:])), 3)}), flush=True)
    eng.close()


def chunk(mode):
    import torch
    n_res, n_org = 100_000, 4
    rng = np.random.default_rng(102)
    beh, cnt = rng.random(n_res), rng.integers(5, 5001, size=n_res)
    flow = [FlowRule(resource=f"r{r}", count=float(cnt[r])) if beh[r] < 0.4 else
            FlowRule(resource=f"r{r}", count=float(cnt[r]), control_behavior=2, max_queueing_time_ms=500) if beh[r] < 0.7
            else FlowRule(resource=f"r{r}", count=float(cnt[r]), control_behavior=1, warm_up_period_sec=10)
            for r in range(n_res)]
    eng = Engine(max_batch=N)
    eng.set_small_batch(0)
    s = LocalSentinel(eng, [f"r{i}" for i in range(n_res)], [f"o{i}" for i in range(1, n_org + 1)],
                      max_origin_nodes=1 << 19)
    assert FlowRuleManager(s).load_rules(flow) == n_res
    if mode == "rules":
        from sentinel_amd.local import AuthorityRuleManager
        from sentinel_amd.rules import AuthorityRule
        assert AuthorityRuleManager(s).load_rules([AuthorityRule(f"r{r}", f"o{n_org}", 1) for r in range(n_res)]) == n_res
    p = 1.0 / np.arange(1, n_res + 1) ** 1.1
    p /= p.sum()
    perm = rng.permutation(n_res)
    dev = torch.device("cuda", 0)
    acq = torch.ones(N, dtype=torch.int32, device=dev)
    times, turned = [], 0
    for step in range(10):
        res = perm[rng.choice(n_res, size=N, p=p)].astype(np.int32)
        org = np.where(rng.random(N) < 0.01, n_org, rng.integers(1, n_org, size=N)).astype(np.int32)
        kind = np.where((org == n_org) & (mode == "premarked"), 2, 0).astype(np.uint8)
        off = np.sort(rng.integers(0, 100, size=N)).astype(np.int32)  # lambda = 1e7 / virtual s, as C2
        a = [torch.from_numpy(x).to(dev) for x in (kind, res, off, org)]
        torch.cuda.synchronize()
        t = time.perf_counter()
        d, w = s.submit_device(a[0], a[1], T0 + 100 * step, a[2], acq, origin=a[3])
        s.device_status()
        times.append((time.perf_counter() - t) * 1e3)
        turned = int((d == 6).sum())
        blocks = int((d == 1).sum())
    print(json.dumps({"mode": mode, "lib": os.path.basename(_lib.LIB_PATH), "ms": [round(x, 3) for x in times[3:]],
                      "median_ms": round(float(np.median(times[3:])), 3), "authority_blocks_last_chunk": turned,
                      "flow_blocks_last_chunk": blocks, "last_origin_entries": int((org == n_org).sum())}), flush=True)
    eng.close()


if __name__ == "__main__":
    if sys.argv[1] == "kernel":
        kernel()
    else:
        chunk(sys.argv[2])
