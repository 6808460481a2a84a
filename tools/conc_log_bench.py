#!/usr/bin/env python3
"""Usage (GPU box): python3 tools/conc_log_bench.py [--mode alternate|legs|gauges] [--legs off,on] [--rounds R]
                                                   [--steps S] [--procs P] [--out DIR] [--tag NAME]

The concurrency server log measurements of DESIGN.md section 3 (profiles/conc_log/*.jsonl, summary.txt).

Shapes, one sga_concurrent_ops call of 2^20 operations each: acquires (acquire 1, never blocked) and releases of the
previous call's tokens in turn, times ascending inside one second, flowIds uniform over
  spread  2^14 rules
  hot     4 rules (k_conc_runs walks a rule's operations with one lane: 2^18 operations a lane)

Legs, each on an engine of its own fed the same operations, alternating step by step in one process:
  off   the log off
  on    the log on (k_slog_conc behind k_conc_runs); the finished seconds are drained outside the timed call
Host clock around the call, which ends in a synchronise.  One warm-up round, then R rounds of S steps a leg; a leg's
figure is the median over its steps, its spread the range of its per-round medians.

--mode alternate (the default) is the whole record in one command: P times in turn a fresh process of this build
with the legs off,on (for on - off), one of this build with the leg off alone and one with SGA_LIB_VARIANT=parent (a
build of the parent commit as sentinel_amd/libsentinel_amd_parent.so) with the leg off alone, then one process for
the gauges, then summary.txt.  The disabled path's criterion is that the two off-alone figures differ by no more than
two processes of one build do.  A process that also holds the `on` engine is not compared with one that does not:
its off leg measured 2 to 5 % slower than the same leg alone (a second engine's token table and buffers in the same
caches is the supposed cause; not measured apart).

--mode gauges times one sga_concurrent_gauges call (and Engine.concurrent_gauges, which first asks with 1,024 rows
and repeats with the size SGA_ERANGE names) at 2^14 and 2^20 loaded rules, with nowCalls != 0 on every rule and on
64 rules."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, T0 = 1 << 20, 1_700_000_000_000
SHAPES = {"spread": 1 << 14, "hot": 4}


def _engine(n_rules, log):
    from sentinel_amd.cluster import ClusterFlowRuleManager, Engine
    eng = Engine(max_batch=N, max_rules=max(2 * n_rules, 1 << 16))
    ClusterFlowRuleManager(eng).load_rule_arrays("default", np.arange(1, n_rules + 1, dtype=np.int64),
                                                 np.full(n_rules, 1e12))
    if log:
        eng.server_log_enable(1 << 16)
    return eng


def run_legs(name, legs, rounds, steps, out, tag):
    from sentinel_amd import _lib
    from sentinel_amd.cluster import CONC_RESULT_DTYPE
    L = _lib.load()
    rng = np.random.default_rng(2026)
    n_rules, half = SHAPES[name], N // 2
    engs = {leg: _engine(n_rules, leg == "on") for leg in legs}
    fid = rng.integers(1, n_rules + 1, size=half).astype(np.int64)
    op = (np.arange(N) % 2).astype(np.uint8)  # acquire, release, acquire, ...
    cli = np.zeros(N, np.uint32)
    acq = np.ones(N, np.int32)
    off = np.sort(rng.integers(0, 1000, size=N)).astype(np.int64)
    res = {leg: np.zeros(N, dtype=CONC_RESULT_DTYPE) for leg in legs}
    held = {}

    def call(eng, o, ids, ts, dst, n):
        t = time.perf_counter()
        rc = L.sga_concurrent_ops(eng.handle, o.ctypes.data, cli.ctypes.data, ids.ctypes.data, acq.ctypes.data,
                                  ts.ctypes.data, n, dst.ctypes.data)
        dt = (time.perf_counter() - t) * 1e3
        assert rc == 0, rc
        return dt

    for leg in legs:  # priming: the tokens the first timed call releases
        call(engs[leg], np.zeros(half, np.uint8), fid, T0 + off[:half], res[leg], half)
        assert (res[leg]["status"][:half] == 0).all()
        held[leg] = res[leg]["token_id"][:half].copy()
    ms = {leg: [] for leg in legs}
    info = {}
    ids = np.zeros(N, np.int64)
    for step in range((rounds + 1) * steps):
        ts = T0 + 1000 * (step + 1) + off
        for leg in legs:
            ids[0::2] = fid
            ids[1::2] = held[leg]
            ms[leg].append(call(engs[leg], op, ids, ts, res[leg], N))
            st = res[leg]["status"]
            assert (st[0::2] == 0).all() and (st[1::2] == 6).all()
            held[leg] = res[leg]["token_id"][0::2].copy()
            if leg == "on":
                rows, le, lc = engs[leg].server_log_rows(int(ts[0]) + 1000)
                info = {"rows": len(rows), "events": int(rows["events"].sum()) + le, "lost_events": le}
    out_rec = {"shape": name, "rules": n_rules, "lib": os.path.basename(_lib.LIB_PATH), "tag": tag, "operations": N,
               "rounds": rounds, "steps": steps}
    for leg in legs:
        x = np.asarray(ms[leg][steps:]).reshape(rounds, steps)
        per_round = np.median(x, axis=1)
        out_rec[leg] = {"median_ms": round(float(np.median(x)), 3),
                        "round_medians_ms": [round(float(v), 3) for v in per_round],
                        "spread_ms": round(float(per_round.max() - per_round.min()), 3)}
    if info:
        out_rec["last_drain"] = info
    for eng in engs.values():
        eng.close()
    line = json.dumps(out_rec)
    print(line, flush=True)
    with open(os.path.join(out, "legs.jsonl"), "a") as f:
        f.write(line + "\n")


def run_gauges(out, reps=9):
    from sentinel_amd import _lib
    from sentinel_amd.cluster import CONC_GAUGE_DTYPE, DefaultTokenService
    L = _lib.load()
    for n_rules in (1 << 14, 1 << 20):
        eng = _engine(n_rules, False)
        svc = DefaultTokenService(eng)
        buf = np.zeros(n_rules, dtype=CONC_GAUGE_DTYPE)
        for listed in (64, n_rules):
            ids = np.arange(1, n_rules + 1, n_rules // listed, dtype=np.int64)
            if listed == n_rules:  # the 64 of the first filling hold a token already
                ids = np.setdiff1d(ids, np.arange(1, n_rules + 1, n_rules // 64))
            got = svc.concurrent_ops(np.zeros(len(ids), np.uint8), np.zeros(len(ids), np.uint32), ids,
                                     np.ones(len(ids), np.int32), np.full(len(ids), T0))
            assert (got["status"] == 0).all()
            raw, py = [], []
            for _ in range(reps + 1):
                n, size = C.c_size_t(), C.c_uint64()
                t = time.perf_counter()
                rc = L.sga_concurrent_gauges(eng.handle, buf.ctypes.data, n_rules, C.byref(n), C.byref(size))
                raw.append((time.perf_counter() - t) * 1e3)
                assert rc == 0 and n.value == listed and size.value == listed
                t = time.perf_counter()
                rows, _ = eng.concurrent_gauges()
                py.append((time.perf_counter() - t) * 1e3)
                assert len(rows) == listed
            rec = {"gauges": True, "rules": n_rules, "listed": listed, "reps": reps,
                   "call_median_ms": round(float(np.median(raw[1:])), 3),
                   "call_range_ms": [round(min(raw[1:]), 3), round(max(raw[1:]), 3)],
                   "python_median_ms": round(float(np.median(py[1:])), 3)}
            line = json.dumps(rec)
            print(line, flush=True)
            with open(os.path.join(out, "gauges.jsonl"), "a") as f:
                f.write(line + "\n")
        eng.close()


def summary(out):
    lines = []
    legs = [json.loads(x) for x in open(os.path.join(out, "legs.jsonl"))]
    for r in legs:
        lines.append(f"shape {r['shape']} ({r['rules']} rules; {r['lib']} {r['tag']}): {r['operations']} operations a "
                     f"call, {r['rounds']} rounds x {r['steps']} steps a leg" +
                     (f"; last drain {r['last_drain']}" if "last_drain" in r else ""))
        for leg in ("off", "on"):
            if leg in r:
                lines.append(f"  {leg:4s} median {r[leg]['median_ms']:9.3f} ms   round medians "
                             f"{r[leg]['round_medians_ms']}   spread {r[leg]['spread_ms']:.3f} ms")
        if "on" in r and "off" in r:
            lines.append(f"  on - off = {r['on']['median_ms'] - r['off']['median_ms']:.3f} ms")
    for shape in SHAPES:
        alone = [r for r in legs if r["shape"] == shape and "on" not in r]  # processes that ran the off leg alone
        here = [r["off"]["median_ms"] for r in alone if "parent" not in r["lib"]]
        par = [r["off"]["median_ms"] for r in alone if "parent" in r["lib"]]
        if here and par:
            lines.append(f"off alone, shape {shape}: this build's processes {here} ms (range {max(here) - min(here):.3f}), "
                         f"the parent's {par} ms (range {max(par) - min(par):.3f}); medians "
                         f"{float(np.median(here)):.3f} against {float(np.median(par)):.3f} ms")
    gpath = os.path.join(out, "gauges.jsonl")
    if os.path.exists(gpath):
        for r in (json.loads(x) for x in open(gpath)):
            lines.append(f"gauges, {r['rules']} rules, {r['listed']} listed: sga_concurrent_gauges median "
                         f"{r['call_median_ms']:.3f} ms (range {r['call_range_ms']}) over {r['reps']} calls; "
                         f"Engine.concurrent_gauges {r['python_median_ms']:.3f} ms")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(os.path.join(out, "summary.txt"), "w") as f:
        f.write(text)


def alternate(a):
    """Fresh processes in turn: this build (off, on), the parent build (off); then the gauges; then the summary.
    A child that fails or overruns its limit ends the run."""
    me = os.path.abspath(__file__)
    common = ["--rounds", str(a.rounds), "--steps", str(a.steps), "--out", a.out]
    for p in range(a.procs):
        for variant, legs in (("", "off,on"), ("", "off"), ("parent", "off")):
            env = dict(os.environ)
            env.pop("SGA_LIB_VARIANT", None)
            if variant:
                env["SGA_LIB_VARIANT"] = variant
            subprocess.run([sys.executable, me, "--mode", "legs", "--legs", legs, "--tag", f"p{p}"] + common, env=env,
                           check=True, timeout=a.child_timeout)
    subprocess.run([sys.executable, me, "--mode", "gauges", "--out", a.out], check=True, timeout=a.child_timeout)
    summary(a.out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="alternate", choices=["alternate", "legs", "gauges", "summary"])
    ap.add_argument("--legs", default="off,on")
    ap.add_argument("--shape", default="both", choices=["spread", "hot", "both"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--procs", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conc_log"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.mode == "alternate":
        alternate(a)
    elif a.mode == "legs":
        for sh in (["spread", "hot"] if a.shape == "both" else [a.shape]):
            run_legs(sh, a.legs.split(","), a.rounds, a.steps, a.out, a.tag)
    elif a.mode == "gauges":
        run_gauges(a.out)
    else:
        summary(a.out)
