#!/usr/bin/env python3
"""Usage (GPU box): python3 tools/nodes_bench.py bulk|single|socket N

The bulk node views' measurement of DESIGN.md section 5 ("Bulk node views and the command center"): N resources under the C2 rule mix (Default / RateLimiter /
WarmUp FlowRules, count 5..500), every node entered by one warming chunk, host clock around the call, median of 5
after 3 warm-ups, each call 700 ms of virtual time after the last so that every node rotates.  One JSON line.
  bulk:   sga_query_nodes over all N nodes (one launch, one wait)
  single: the same nodes read by sga_query_node one at a time -- at most 4,096 of them, evenly spaced ids: above
          that the figure is a sample, and "nodes" says how many were read.  SGA_LIB_VARIANT=parent times the
          parent commit's build (sentinel_amd/libsentinel_amd_parent.so), which has no bulk entry.
  socket: one clusterNode request through a SimpleHttpCommandCenter on 127.0.0.1, end to end
Kernel time and bytes: rocprofv3 --kernel-trace --stats -- python3 tools/nodes_bench.py bulk N, in a run of its
own (k_node_views must read 4,032 B a node)."""
import ctypes as C
import json
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sentinel_amd import _lib
from sentinel_amd.cluster import Engine
from sentinel_amd.local import FlowRuleManager, LocalSentinel
from sentinel_amd.rules import FlowRule

mode, N = sys.argv[1], int(sys.argv[2])
T0 = 1_700_000_000_000
CHUNK = 1 << 17
rng = np.random.default_rng(7)
eng = Engine(max_batch=CHUNK)
s = LocalSentinel(eng, [f"r{i}" for i in range(N)])
fm = FlowRuleManager(s)
assert fm.load_rules([FlowRule(resource=f"r{r}", count=float(rng.integers(5, 500)), control_behavior=[0, 2, 1][r % 3],
                               max_queueing_time_ms=500, warm_up_period_sec=10) for r in range(N)]) == N
for lo in range(0, N, CHUNK):  # one entry a resource
    ids = np.arange(lo, min(lo + CHUNK, N), dtype=np.uint32)
    s.submit(np.zeros(len(ids), np.uint8), ids, np.full(len(ids), T0 + lo // CHUNK, np.int64),
             np.ones(len(ids), np.int32))
L = _lib.load()
now = T0 + 1000
times = []
nodes = N
if mode == "bulk":
    from sentinel_amd.local import NODE_ROW_DTYPE
    out = np.zeros(N, dtype=NODE_ROW_DTYPE)
    n = C.c_size_t()
    for _ in range(8):
        now += 700
        t = time.perf_counter()
        rc = L.sga_query_nodes(eng.handle, 0, None, 0, now, 0, out.ctypes.data, N, C.byref(n))
        times.append((time.perf_counter() - t) * 1e3)
        assert rc == 0 and n.value == N, (rc, n.value)
elif mode == "single":
    ids = np.linspace(0, N - 1, min(N, 4096)).astype(np.uint32)
    nodes = len(ids)
    v = _lib.SgaNodeView()
    for _ in range(8):
        now += 700
        t = time.perf_counter()
        for r in ids:
            rc = L.sga_query_node(eng.handle, int(r), now, C.byref(v))
        times.append((time.perf_counter() - t) * 1e3)
        assert rc == 0
else:
    from sentinel_amd.command_center import CommandCenter, SimpleHttpCommandCenter
    clock = {"now": now}
    srv = SimpleHttpCommandCenter(CommandCenter(s, {"flow": fm}, clock=lambda: clock["now"]), port=18760)
    port = srv.start()
    for _ in range(8):
        clock["now"] += 700
        t = time.perf_counter()
        with socket.create_connection(("127.0.0.1", port)) as c:
            c.sendall(b"GET /clusterNode HTTP/1.0\r\n\r\n")
            size = 0
            while True:
                b = c.recv(1 << 20)
                if not b:
                    break
                size += len(b)
        times.append((time.perf_counter() - t) * 1e3)
    srv.stop()
    nodes = N
print(json.dumps({"mode": mode, "lib": os.environ.get("SGA_LIB_VARIANT") or "this", "resources": N, "nodes": nodes,
                  "ms": [round(x, 3) for x in times], "median_ms_last5": round(float(np.median(times[3:])), 3),
                  "us_per_node": round(float(np.median(times[3:])) * 1e3 / nodes, 3)}))
eng.close()
