#!/usr/bin/env python3
"""Usage (GPU box): python3 tools/context_bench.py wide|mid|hot [off|origin|context|both|ruled]...

The context nodes' measurement of DESIGN.md section 5, by the method of tools/origin_bench.py (same shapes, same
clock): device-entry chunks of 2^20 entries, host clock around the call and the stream wait, median
of 5 after 3 warm-ups.  16 contexts and 16 origins, both uniform.
  wide: 10,000 resources (Default QPS count 50 each): 160,000 pairs of 6-7 events a chunk and kind of pair
  mid:  1,024 resources: 16,384 pairs of about 64 events
  hot:  64 resources: 1,024 pairs of about 1,024 events
off: no id array.  origin: the origin array alone (origin_bench's "on").  context: the context array alone.
both: both arrays (two sort elements an event).  ruled: the context array, and every resource CHAIN-ruled (a
second rule, CHAIN on context c0, Default QPS count 5: each resource is replayed in arrival order).
Kernel times: rocprofv3 --kernel-trace --stats -- python3 tools/context_bench.py wide both, in a run of its own."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sentinel_amd.cluster import Engine
from sentinel_amd.local import FlowRuleManager, LocalSentinel
from sentinel_amd.rules import FlowRule, RuleConstant

shape = sys.argv[1]
modes = sys.argv[2:] or ["off", "origin", "context", "both"]
N, O, T0 = 1 << 20, 16, 1_700_000_000_000
R = {"wide": 10_000, "mid": 1024, "hot": 64}[shape]
for mode in modes:
    eng = Engine(max_batch=N)
    eng.set_small_batch(0)
    s = LocalSentinel(eng, [f"r{i}" for i in range(R)], [f"o{i}" for i in range(O)], max_origin_nodes=1 << 18,
                      contexts=[f"c{i}" for i in range(O)], max_context_nodes=1 << 18)
    rules = []
    if mode == "ruled":  # CHAIN rules first: the order FlowRuleComparator keeps
        rules += [FlowRule(resource=f"r{k}", count=5, strategy=RuleConstant.STRATEGY_CHAIN, ref_resource="c0")
                  for k in range(R)]
    rules += [FlowRule(resource=f"r{k}", count=50) for k in range(R)]
    assert FlowRuleManager(s).load_rules(rules) == len(rules)
    rng = np.random.default_rng(7)
    dev = torch.device("cuda", 0)
    kind = torch.zeros(N, dtype=torch.uint8, device=dev)
    acq = torch.ones(N, dtype=torch.int32, device=dev)
    times = []
    for step in range(8):
        res = torch.from_numpy(rng.integers(0, R, size=N).astype(np.int32)).to(dev)
        org = torch.from_numpy(rng.integers(1, O + 1, size=N).astype(np.int32)).to(dev)
        off = torch.from_numpy(np.sort(rng.integers(0, 1000, size=N)).astype(np.int32)).to(dev)
        ctx = torch.from_numpy(rng.integers(1, O + 1, size=N).astype(np.int32)).to(dev)
        torch.cuda.synchronize()
        t = time.perf_counter()
        d, w = s.submit_device(kind, res, T0 + 1000 * step, off, acq,
                               origin=org if mode in ("origin", "both") else None,
                               context=ctx if mode in ("context", "both", "ruled") else None)
        s.device_status()
        times.append((time.perf_counter() - t) * 1e3)
    npairs = sum(len(s.default_nodes(r)) for r in range(min(R, 64)))
    print(f"{shape} {mode}: ms per 2^20-event chunk (8 steps, first 3 are warm-up): " +
          " ".join(f"{x:.3f}" for x in times), f"median of last 5 {np.median(times[3:]):.3f};",
          f"context nodes on the first {min(R, 64)} resources {npairs}; FLOW blocks in the last chunk {int((d == 1).sum())}")
    eng.close()
