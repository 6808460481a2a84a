#!/usr/bin/env python3
"""Usage (GPU box): python3 tools/relate_bench.py relate|direct

The RELATE path's measurement of DESIGN.md section 5: device-entry chunks of 2^20 entries over 10,000 resources
in 5,000 pairs, under RELATE rules (A_k -> B_k, Default QPS count 50) or the equivalent DIRECT rules;
SGA_LIB_VARIANT=X times another build of the library (direct only for one that predates RELATE).  Kernel
times: rocprofv3 --kernel-trace --stats -- python3 tools/relate_bench.py relate, in a run of its own."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sentinel_amd.cluster import Engine
from sentinel_amd.local import FlowRuleManager, LocalSentinel
from sentinel_amd.rules import FlowRule

mode = sys.argv[1]
N, R, T0 = 1 << 20, 10_000, 1_700_000_000_000
eng = Engine(max_batch=N)
eng.set_small_batch(0)
s = LocalSentinel(eng, [f"r{i}" for i in range(R)])
rules = []
for k in range(0, R, 2):
    if mode == "relate":
        rules.append(FlowRule(resource=f"r{k}", count=50, strategy=1, ref_resource=f"r{k + 1}"))
    else:
        rules.append(FlowRule(resource=f"r{k}", count=50))
    rules.append(FlowRule(resource=f"r{k + 1}", count=50))
assert FlowRuleManager(s).load_rules(rules) == len(rules)
rng = np.random.default_rng(7)
dev = torch.device("cuda", 0)
kind = torch.zeros(N, dtype=torch.uint8, device=dev)
acq = torch.ones(N, dtype=torch.int32, device=dev)
times = []
blocks = 0
for step in range(8):
    res = torch.from_numpy(rng.integers(0, R, size=N).astype(np.int32)).to(dev)
    off = torch.from_numpy(np.sort(rng.integers(0, 1000, size=N)).astype(np.int32)).to(dev)
    torch.cuda.synchronize()
    t = time.perf_counter()
    d, w = s.submit_device(kind, res, T0 + 1000 * step, off, acq)
    s.device_status()
    times.append((time.perf_counter() - t) * 1e3)
    blocks = int((d == 1).sum())
print(f"{mode}: ms per 2^20-event chunk (8 steps, first 3 are warm-up): " + " ".join(f"{x:.3f}" for x in times),
      f"median of last 5 {np.median(times[3:]):.3f}; FLOW blocks in the last chunk {blocks}")
eng.close()
