#!/usr/bin/env python3
"""Usage (GPU box): python3 tools/gateway_bench.py [n_log2] [--regex device|host] [--pattern P] [--skip-decide]

The gateway parse measurement of DESIGN.md section 5 (profiles/gateway/): 2^20 entries (n_log2: another size) over
1,024 routes, Zipf(1.1); per route three gateway rules -- the client IP, a header with an EXACT pattern, a rule
without a paramItem -- so every entry gets three arguments; values of 7 to 40 bytes at whatever offset the packer
leaves them.  The batch lives on the device.  Per timed step:

  parse   sga_gateway_parse_device on a side stream, device events around 20 calls (3 warm-ups before), 5 rounds
  decide  sga_submit_events_device of the parsed batch: a host clock around the call and the status wait, chunk by
          chunk at advancing timestamps (3 warm-ups, 7 timed)

and the bytes the parse step has to move, counted from the shapes: per entry the resource, mode, flags (read and
written) and param word, per item slot the field's offset and length and its bytes, per argument two value words.
One JSON line.  The kernel's own time: rocprofv3 --kernel-trace --stats -- python3 tools/gateway_bench.py.

--regex swaps the header's EXACT rule for one REGEX rule per route with the same pattern (--pattern, default
[a-z]+-\\d{2,4}-gold: the quarter of the headers that equalled the EXACT pattern match it):
  device  a manager with device_regex=True: the kernel walks the pattern's DFA, no word is passed
  host    a default manager, the only way without programs: per step GatewayRuleManager.regex_bits over the 2^20
          requests on the host (2 timed passes), the upload of the word (5 timed), then the parse with the word
--skip-decide leaves the submit step out."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sentinel_amd import gateway as G  # noqa: E402
from sentinel_amd.cluster import Engine  # noqa: E402
from sentinel_amd.local import LocalSentinel, param_value  # noqa: E402

T0 = 1_700_000_000_000
HBM_TBS = 8.0  # MI355X_MICROARCH.md, the figure of DESIGN.md section 3


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("n_log2", nargs="?", type=int, default=20)
    ap.add_argument("--regex", choices=["device", "host"])
    ap.add_argument("--pattern", default=r"[a-z]+-\d{2,4}-gold")
    ap.add_argument("--skip-decide", action="store_true")
    opt = ap.parse_args()
    n = 1 << opt.n_log2
    n_res = 1024
    rng = np.random.default_rng(2024)
    names = [f"route{r}" for r in range(n_res)]
    eng = Engine(max_batch=n)
    eng.set_small_batch(0)
    s = LocalSentinel(eng, names)
    m = G.GatewayRuleManager(s, device_regex=opt.regex == "device")
    rules = []
    for r, name in enumerate(names):
        header = G.GatewayParamFlowItem(parse_strategy=2, field_name="X-Tenant", pattern=opt.pattern, match_strategy=2) \
            if opt.regex else G.GatewayParamFlowItem(parse_strategy=2, field_name="X-Tenant",
                                                   pattern=f"tenant-{r % 50:04d}-gold", match_strategy=0)
        rules += [G.GatewayFlowRule(name, count=float(rng.integers(5, 500)),
                                    param_item=G.GatewayParamFlowItem(parse_strategy=0)),
                  G.GatewayFlowRule(name, count=float(rng.integers(5, 500)), param_item=header),
                  G.GatewayFlowRule(name, count=float(rng.integers(500, 5000)))]
    assert m.load_rules(rules) == 3 * n_res and m.max_args == 3 and m.fields() == [("client_ip", ""), ("header", "X-Tenant")]
    assert len(m.regex_host_items()) == (n_res if opt.regex == "host" else 0)
    p = 1.0 / np.arange(1, n_res + 1) ** 1.1
    p /= p.sum()
    res = rng.permutation(n_res)[rng.choice(n_res, size=n, p=p)].astype(np.int32)
    # the field table built with numpy (a Python loop over 2^20 requests is not what is measured): client IPs of 7 to
    # 15 bytes, tenant headers of 16 to 40 bytes of which about a quarter equal the route's pattern
    ip = rng.integers(0, 1024, size=n)  # 2,048 distinct addresses, under a rule's CacheMap capacity (4,000 keys): the maps stay in free mode
    ips = np.char.add(np.char.add("10.", (ip >> 8).astype(str)), np.char.add(".", ((ip & 255) * 97 % 256).astype(str)))
    ips = np.char.add(ips, np.where(rng.random(n) < 0.5, ".1", ".123"))
    gold = rng.random(n) < 0.25
    pad = np.array(["", "-eu-west-1", "-ap-southeast-2-blue"])[rng.integers(0, 3, size=n)]
    ten = np.where(gold, np.char.add(np.char.add("tenant-", np.char.zfill((res % 50).astype(str), 4)), "-gold"),
                   np.char.add(np.char.add("tenant-", np.char.zfill(rng.integers(0, 5000, size=n).astype(str), 4)),
                               np.char.add("-std", pad)))
    both = np.char.add(ips, ten)
    l_ip, l_ten = np.char.str_len(ips).astype(np.uint32), np.char.str_len(ten).astype(np.uint32)
    assert l_ip.min() >= 7 and l_ten.max() <= 40
    start = np.concatenate([[0], np.cumsum(l_ip + l_ten)[:-1]]).astype(np.uint32)
    off = np.stack([start, start + l_ip], axis=1).reshape(-1)
    ln = np.stack([l_ip, l_ten], axis=1).reshape(-1)
    blob = np.frombuffer("".join(both.tolist()).encode("ascii"), np.uint8)
    assert len(blob) == int((l_ip + l_ten).sum())

    dev = torch.device("cuda", eng.device)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731
    d_res, d_mode = t(res), torch.zeros(n, dtype=torch.uint8, device=dev)
    d_off, d_ln, d_blob = t(off.view(np.int32)), t(ln.view(np.int32)), t(blob)
    d_flags = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_param = torch.zeros(n, dtype=torch.int64, device=dev)
    d_vals = torch.zeros(2 * m.max_args * n, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(device=dev)  # torch's default stream is handle 0, which the engine reads as its own

    extra, d_bits = {}, None
    if opt.regex == "host":  # what a build without programs pays before it can parse: the host pass and the upload
        rqs = [{("header", "X-Tenant"): v} for v in ten.tolist()]
        host_ms, up_ms = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            bits = m.regex_bits(res, rqs)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        for _ in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d_bits = torch.from_numpy(bits.view(np.int64)).to(dev)
            torch.cuda.synchronize()
            up_ms.append((time.perf_counter() - t0) * 1e3)
        extra = {"host_regex_bits_ms": round(float(np.median(host_ms[1:])), 1),
                 "host_regex_bits_ms_passes": [round(x, 1) for x in host_ms[1:]],
                 "word_upload_ms": round(float(np.median(up_ms[1:])), 3),
                 "matching": int((bits >> np.uint64(1) & np.uint64(1)).sum())}

    def parse():
        m.parse_device(d_res, d_mode, d_off, d_ln, d_blob, d_flags, d_param, d_vals, regex_bits=d_bits, stream=stream)

    for _ in range(3):
        parse()
    torch.cuda.synchronize()
    reps, rounds = 20, []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(reps):
            parse()
        b.record(stream)
        b.synchronize()
        rounds.append(a.elapsed_time(b) / reps)
    s.device_status()
    parse_ms = float(np.median(rounds))
    nbytes_r = n * (4 + 1 + 1) + 2 * n * 8 + len(blob)
    nbytes_w = n * (1 + 8) + n * m.max_args * 16
    kind = torch.zeros(n, dtype=torch.uint8, device=dev)
    acq = torch.ones(n, dtype=torch.int32, device=dev)
    ts_off = t(np.sort(rng.integers(0, 100, size=n)).astype(np.int32))
    decide = []
    nm_key = int(np.array([param_value("$NM")], np.uint64).view(np.int64)[0])
    not_matched = int((d_vals.view(n, 6)[:, 3] == nm_key).sum().item())  # the header slot's "$NM" answers
    out = {"entries": n, "routes": n_res, "args": m.max_args, "blob_bytes": int(len(blob)),
           "header_rule": "EXACT" if not opt.regex else f"REGEX {opt.pattern} ({opt.regex})", "header_not_matched": not_matched,
           "parse_ms": round(parse_ms, 4), "parse_ms_rounds": [round(x, 4) for x in rounds],
           "parse_bytes_read": int(nbytes_r), "parse_bytes_written": int(nbytes_w),
           "parse_gb_s": round((nbytes_r + nbytes_w) / parse_ms / 1e6, 1), "hbm_gb_s": HBM_TBS * 1000, **extra}
    if not opt.skip_decide:
        for step in range(10):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d, w = s.submit_device(kind, d_res, T0 + 100 * step, ts_off, acq, d_flags, None, d_param, d_vals)
            s.device_status()
            decide.append((time.perf_counter() - t0) * 1e3)
        dec = d.cpu().numpy()
        out.update({"decide_ms": round(float(np.median(decide[3:])), 3),
                    "decide_ms_steps": [round(x, 3) for x in decide[3:]],
                    "last_chunk": {"pass": int((dec == 0).sum()), "param_blocks": int((dec == 2).sum())}})
    print(json.dumps(out), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
