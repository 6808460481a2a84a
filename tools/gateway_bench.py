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
--skip-decide leaves the submit step out.

--api device|global|host is another workload ("Gateway API groups"): 2^20 requests with paths of
8 to 40 bytes against 64 API groups -- each an EXACT pattern and a /svcNN/** prefix, one of them a REGEX besides --
and 16 routes:
  device  sga_gateway_api_match_device and sga_gateway_api_expand_device (with the gather of a two-column field
          table), each timed like the parse step; the table is staged in LDS
  global  the same table behind a blob padded past the staging limit: the walk reads global memory (the A/B)
  host    the only way without the table: matching_apis_one per request on the host, timed over --host-sample
          requests of the same data (2^14 by default) and scaled to the batch"""
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


def api_main(opt):
    import ctypes as C

    import torch
    from sentinel_amd import _lib
    from sentinel_amd import gateway_api as A
    n, n_api, n_route = 1 << opt.n_log2, 64, 16
    rng = np.random.default_rng(2025)
    names = [f"route{r}" for r in range(n_route)] + [f"svc{k:02d}" for k in range(n_api)]
    eng = Engine(max_batch=n)
    s = LocalSentinel(eng, names)
    m = A.GatewayApiDefinitionManager(s)
    defs = []
    for k in range(n_api):
        items = [A.ApiPathPredicateItem(f"/svc{k:02d}/health", 0), A.ApiPathPredicateItem(f"/svc{k:02d}/**", 1)]
        if k == 7:
            items.append(A.ApiPathPredicateItem(r"/user/\d+/orders(?:/\d+)?", 2))
        defs.append(A.ApiDefinition(f"svc{k:02d}", items))
    m.load_api_definitions(defs)
    assert m.host_predicates() == [] and m.words == 1
    # the paths with numpy: /svcNN/health, /svcNN/<8..30 bytes>, /user/<id>/orders[/<id>], and paths nobody claims
    svc = np.char.add("/svc", np.char.zfill(rng.integers(0, n_api + 8, size=n).astype(str), 2))  # 8 of 72 unknown
    tails = np.array(["/health", "/v1/items", "/v1/items/4711", "/v2/orders/2024/10/21/open", "/static/app.js",
                      "/v1/customers/8812/address"])[rng.integers(0, 6, size=n)]
    users = np.char.add(np.char.add("/user/", rng.integers(1, 10 ** 6, size=n).astype(str)),
                        np.where(rng.random(n) < 0.5, "/orders", "/orders/77"))
    paths = np.where(rng.random(n) < 0.1, users, np.char.add(svc, tails))
    plen = np.char.str_len(paths).astype(np.uint32)
    assert plen.min() >= 8 and plen.max() <= 40
    off = np.concatenate([[0], np.cumsum(plen)[:-1]]).astype(np.uint32)
    blob = np.frombuffer("".join(paths.tolist()).encode("ascii"), np.uint8)
    routes = rng.integers(0, n_route + 1, size=n).astype(np.uint32)
    routes[routes == n_route] = A.ROUTE_NULL
    out = {"workload": "api", "mode": opt.api, "requests": n, "apis": n_api, "routes": n_route,
           "blob_bytes": int(len(blob)), "hbm_gb_s": HBM_TBS * 1000}
    if opt.api == "host":
        k = min(n, opt.host_sample)
        sample = paths[:k].tolist()
        passes = []
        for _ in range(2):
            t0 = time.perf_counter()
            hits = sum(len(m.matching_apis_one(v)) for v in sample)
            passes.append((time.perf_counter() - t0) * 1e3)
        out.update({"host_sample": k, "host_sample_ms_passes": [round(x, 1) for x in passes],
                    "host_us_per_request": round(min(passes) * 1e3 / k, 2),
                    "host_ms_scaled_to_batch": round(min(passes) * n / k, 1), "sample_matches": hits})
        print(json.dumps(out), flush=True)
        eng.close()
        return
    if opt.api == "global":  # the same predicates, the blob padded past kApiLdsBytes
        arr, n_preds, res, buf, blob_len = m._sent
        pad = (C.c_uint8 * (blob_len + 70000)).from_buffer_copy(bytes(buf[:blob_len]) + bytes(70000))
        assert _lib.load().sga_gateway_api_load(eng.handle, arr, n_preds, res.ctypes.data, len(res), pad, len(pad)) == 0
    dev = torch.device("cuda", eng.device)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731
    nf = 2
    d_off, d_len, d_blob = t(off.view(np.int32)), t(plen.view(np.int32)), t(blob)
    d_routes = t(routes.view(np.int32))
    d_match = torch.zeros(n, dtype=torch.int64, device=dev)
    d_fo, d_fl = t(rng.integers(0, 1 << 30, size=n * nf).astype(np.int32)), t(rng.integers(0, 40, size=n * nf).astype(np.int32))
    cap = 3 * n
    i32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)  # noqa: E731
    src, pos, d_res, d_total = i32(cap), i32(cap), i32(cap), i32(1)
    d_mode = torch.zeros(cap, dtype=torch.uint8, device=dev)
    fo_out, fl_out = i32(cap * nf), i32(cap * nf)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def match():
        m.match_device(d_off, d_len, d_blob, d_match, stream=stream)

    def expand():
        m.expand_device(d_routes, d_match, cap, src, pos, d_res, d_mode, d_total, field_off=d_fo, field_len=d_fl,
                        n_fields=nf, field_off_out=fo_out, field_len_out=fl_out, stream=stream)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps, rounds = 20, []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(reps):
                fn()
            b.record(stream)
            b.synchronize()
            rounds.append(a.elapsed_time(b) / reps)
        return rounds

    mr = timed(match)
    er = timed(expand)
    s.device_status()
    total = int(d_total.item())
    rows = d_match.cpu().numpy().view(np.uint64)
    matched = int((rows != 0).sum())
    # a sample against the host model
    for i in rng.integers(0, n, size=200).tolist():
        want = m.matching_apis_one(str(paths[i]))
        got = [m.columns()[k] for k in range(n_api) if (int(rows[i]) >> k) & 1]
        assert got == want, (paths[i], got, want)
    assert total == int((routes != A.ROUTE_NULL).sum()) + int(np.unpackbits(rows.view(np.uint8)).sum())
    match_ms, expand_ms = float(np.median(mr)), float(np.median(er))
    mb_r, mb_w = n * 8 + len(blob), n * 8
    eb_r = n * 4 + n * 8 * 2 + n * 4 * 4 + total * nf * 8
    eb_w = n * 4 * 2 + total * (4 + 4 + 4 + 1) + total * nf * 8
    out.update({"in_lds": opt.api == "device", "requests_matching": matched, "entries": total,
                "match_ms": round(match_ms, 4), "match_ms_rounds": [round(x, 4) for x in mr],
                "match_bytes_read": int(mb_r), "match_bytes_written": int(mb_w),
                "match_gb_s": round((mb_r + mb_w) / match_ms / 1e6, 1),
                "expand_ms": round(expand_ms, 4), "expand_ms_rounds": [round(x, 4) for x in er],
                "expand_bytes_read": int(eb_r), "expand_bytes_written": int(eb_w),
                "expand_gb_s": round((eb_r + eb_w) / expand_ms / 1e6, 1)})
    print(json.dumps(out), flush=True)
    eng.close()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("n_log2", nargs="?", type=int, default=20)
    ap.add_argument("--regex", choices=["device", "host"])
    ap.add_argument("--pattern", default=r"[a-z]+-\d{2,4}-gold")
    ap.add_argument("--skip-decide", action="store_true")
    ap.add_argument("--api", choices=["device", "global", "host"])
    ap.add_argument("--host-sample", type=int, default=1 << 14)
    opt = ap.parse_args()
    if opt.api:
        return api_main(opt)
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
