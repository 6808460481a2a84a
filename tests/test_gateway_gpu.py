"""Gateway rules on the GPU: the parse kernel (sga_gateway_parse / sga_gateway_parse_device) against
local.param_value and tests/gateway_trace.py, and the decisions of parsed gateway traffic against the oracle
replaying the stream whose argument vectors gateway_trace produced."""
import ctypes as C
import heapq

import numpy as np
import pytest

from sentinel_amd import _lib
from sentinel_amd import gateway as G
from sentinel_amd.local import (EV_ARGS, Decision, LocalSentinel, ParamFlowException, ParamFlowRuleManager,
                                encode_args, param_value)
from sentinel_amd.rules import ParamFlowRule
from tests import gateway_trace as gt
from tests import local_trace as lt
from tests.test_local_parity_gpu import T0, _assert_same, _engine

pytestmark = pytest.mark.gpu
NULL = 0xFFFFFFFF
REFUSED = 0xFFFFFFFF << 32  # the param word of an event the parser refused


def _sentinel(names, rules, max_batch=1 << 14, **kw):
    eng = _engine(max_batch)
    s = LocalSentinel(eng, names, **kw)
    m = G.GatewayRuleManager(s)
    m.load_rules([gt.to_product(r) for r in rules])
    return eng, s, m


def _raw_parse(s, res, mode, off, ln, blob, n_fields, regex=None, flags=None, param=None, value_base=0,
               n_values=None, max_args=None, fill=0):
    """sga_gateway_parse over a field table laid out by the test: (rc, flags, param, values)."""
    n = len(res)
    ma = C.c_uint32()
    assert _lib.load().sga_gateway_max_args(s.engine.handle, C.byref(ma)) == 0
    if max_args is not None:
        assert ma.value == max_args
    res = np.ascontiguousarray(res, np.uint32)
    mode = np.ascontiguousarray(mode, np.uint8)
    off = np.ascontiguousarray(off, np.uint32)
    ln = np.ascontiguousarray(ln, np.uint32)
    blob = np.frombuffer(bytes(blob) or b"\0", np.uint8)
    assert len(off) == len(ln) == n * n_fields
    f = np.zeros(n, np.uint8) if flags is None else np.array(flags, np.uint8)
    p = np.zeros(n, np.uint64) if param is None else np.array(param, np.uint64)
    nv = value_base + 2 * ma.value * n if n_values is None else n_values
    vals = np.full(max(1, nv), fill, np.uint64)
    rg = None if regex is None else np.ascontiguousarray(regex, np.uint64)
    rc = _lib.load().sga_gateway_parse(s.engine.handle, res.ctypes.data, mode.ctypes.data, off.ctypes.data,
                                       ln.ctypes.data, blob.ctypes.data, len(bytes(blob)) if len(off) else 0,
                                       rg.ctypes.data if rg is not None else None, n, f.ctypes.data, p.ctypes.data,
                                       vals.ctypes.data, nv, value_base)
    return rc, f, p, vals


def _vector(p, vals, i):
    """Event i's argument words as a list."""
    off, na = int(p[i]) >> 32, int(p[i]) & 0xFFFFFFFF
    return [int(x) for x in vals[off:off + 2 * na]]


def _expected(args):
    pv = []
    word = encode_args(args, pv)
    assert word == len(args)
    return pv


def _string_of(nbytes):
    """A string of exactly nbytes UTF-8 bytes with 2-, 3- and 4-byte characters in it where they fit."""
    out, used = [], 0
    for ch in "é€\U0001D11Ea" * (nbytes // 4 + 1):
        b = len(ch.encode())
        if used + b > nbytes:
            break
        out.append(ch)
        used += b
    return "".join(out) + "x" * (nbytes - used)


# ---- 1. hash seams
HASH_LENGTHS = [0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 31, 32, 33, 63, 64, 65, 255, 1000]


def test_keys_equal_param_value_at_every_length_and_offset():
    """XXH64's 32-byte stripe seam and its 8 / 4 / 1 byte tails, each value at byte offsets 0..7 of the blob."""
    assert param_value("$NM") == 0xa8199fa79222e5de and param_value("$D") == 0xb0cc5c973684564a
    assert param_value("") == 0x4211740c33556dfb
    eng, s, m = _sentinel(["r"], [gt.rule(resource="r", count=1, item={"parse_strategy": 0})])
    blob, off, ln, strings = bytearray(), [], [], []
    for nb in HASH_LENGTHS:
        v = _string_of(nb)
        assert len(v.encode()) == nb
        for shift in range(8):
            blob += b"#" * (-len(blob) % 8 + shift)
            off.append(len(blob))
            ln.append(nb)
            blob += v.encode()
            strings.append(v)
    n = len(strings)
    rc, f, p, vals = _raw_parse(s, np.zeros(n), np.zeros(n), off, ln, blob, 1, max_args=1)
    assert rc == 0 and (f == EV_ARGS).all()
    for i, v in enumerate(strings):
        assert _vector(p, vals, i) == [0, param_value(v)], (len(v.encode()), off[i] % 8)
    eng.close()


# ---- 2. match seams
MATCH_RULES = [
    gt.rule(resource="m", count=1, item={"parse_strategy": 2, "field_name": "E", "pattern": "abc", "match_strategy": 0}),
    gt.rule(resource="m", count=2, item={"parse_strategy": 3, "field_name": "C", "pattern": "aab", "match_strategy": 3}),
    gt.rule(resource="m", count=3, item={"parse_strategy": 4, "field_name": "P", "pattern": "zz", "match_strategy": 1}),
    gt.rule(resource="m", count=4, item={"parse_strategy": 2, "field_name": "U", "pattern": "zz", "match_strategy": 7}),
    gt.rule(resource="m", count=5, item={"parse_strategy": 2, "field_name": "R", "pattern": "\\d+", "match_strategy": 2}),
    gt.rule(resource="m", count=6, item={"parse_strategy": 2, "field_name": "Z", "pattern": "", "match_strategy": 0}),
    gt.rule(resource="m", count=7, item={"parse_strategy": 1, "pattern": "é€", "match_strategy": 3}),
]
MATCH_VALUES = {
    ("header", "E"): ["abc", "ab", "abcd", "", None, "abd"],            # equal, proper prefix, longer, empty, null
    ("url_param", "C"): ["aabxx", "xxaab", "aaab", "aa", "aab", "xyz", None, ""],  # start, end, partial overlap, ...
    ("cookie", "P"): ["zzz", "azz", None],
    ("header", "U"): ["zz", "q"],
    ("header", "R"): ["123", "12a", None, ""],
    ("header", "Z"): ["anything", ""],
    ("host", ""): ["xé€y", "é", "€é", None],
}


def test_match_strategies_equal_the_trace():
    eng, s, m = _sentinel(["m"], MATCH_RULES)
    by_res, _ = gt.assign(MATCH_RULES)
    conv = m.get_converted_param_rules("m")
    assert [len(c.param_flow_item_list) for c in conv] == [1] * 7  # the empty pattern adds "$NM" too
    assert conv[5].param_flow_item_list[0].object == "$NM" and conv[5].param_flow_item_list[0].count == 10_000_000
    n = 48
    rqs = [{k: v[i % len(v)] for k, v in MATCH_VALUES.items() if v[i % len(v)] is not None} for i in range(n)]
    f, p, vals = m.parse(np.zeros(n, np.uint32), np.zeros(n, np.uint8), rqs)
    seen = set()
    for i, rq in enumerate(rqs):
        args = gt.parse(by_res["m"], 0, rq)
        assert f[i] == EV_ARGS and _vector(p, vals, i) == _expected(args), (rq, args)
        seen.update((k, a) for k, a in enumerate(args))
    for want in [(0, "abc"), (0, "$NM"), (0, None), (1, "aabxx"), (1, "xxaab"), (1, "aaab"), (1, "aab"), (1, "$NM"),
                 (2, "azz"), (3, "q"), (4, "123"), (4, "$NM"), (4, None), (5, "anything"), (5, ""), (6, "xé€y"),
                 (6, "$NM")]:
        assert want in seen, want
    # REGEX follows the bit word: all zeros turns every non-null REGEX value into "$NM"; no word matches all
    off, ln, blob = G.pack_requests(rqs, m.fields())
    for bits, expect in ((np.zeros(n, np.uint64), "$NM"), (None, None)):
        rc, f, p, vals = _raw_parse(s, np.zeros(n), np.zeros(n), off, ln, blob.tobytes(), len(m.fields()), regex=bits)
        assert rc == 0
        for i, rq in enumerate(rqs):
            args = gt.parse(by_res["m"], 0, rq)
            if args[4] is not None:
                args[4] = expect or rq[("header", "R")]
            assert _vector(p, vals, i) == _expected(args), (i, bits is None)
    eng.close()


# ---- 3. the shape of the array
def test_array_shapes():
    rules = [gt.rule(resource="mix", count=1, item={"parse_strategy": 0}),
             gt.rule(resource="mix", count=2, resource_mode=1, item={"parse_strategy": 2, "field_name": "H"}),
             gt.rule(resource="mix", count=3),
             gt.rule(resource="np", count=4), gt.rule(resource="np", count=5, interval_sec=2),
             gt.rule(resource="api", resource_mode=1, count=6, item={"parse_strategy": 2, "field_name": "H"})]
    eng, s, m = _sentinel(["mix", "np", "plain", "api"], rules)
    rq = {("client_ip", ""): "9.9.9.9", ("header", "H"): "hv"}
    res = np.array([0, 0, 1, 1, 2, 3, 3, 2], np.uint32)
    mode = np.array([0, 1, 0, 1, 0, 0, 1, 1], np.uint8)
    flags = np.array([1, 0, 8, 0, 4, 2, 0, 16 | 4], np.uint8)
    param = np.array([5, 5, 5, 5, 77, 5, 5, (3 << 32) | 2], np.uint64)
    f, p, vals = m.parse(res, mode, [rq] * 8, flags=flags, param=param, value_base=5)
    assert m.max_args == 3
    by_res, _ = gt.assign(rules)
    for i, name in ((0, "mix"), (1, "mix"), (2, "np"), (3, "np"), (5, "api"), (6, "api")):
        args = gt.parse(by_res[name], int(mode[i]), rq)
        assert f[i] == flags[i] | EV_ARGS and _vector(p, vals, i) == _expected(args), (i, args)
        assert int(p[i]) >> 32 == 5 + i * 6
    # one rule of "mix" has the other mode whatever the request's: no arguments, the flag still set
    assert int(p[0]) & 0xFFFFFFFF == 0 and int(p[1]) & 0xFFFFFFFF == 0
    assert _vector(p, vals, 2) == [0, param_value("$D")] and _vector(p, vals, 6) == [0, param_value("hv")]
    assert int(p[5]) & 0xFFFFFFFF == 0
    # the resource without gateway rules keeps its flags and param
    assert (f[4], int(p[4]), f[7], int(p[7])) == (4, 77, 16 | 4, (3 << 32) | 2)
    # and the value words nobody writes stay the caller's: other resources' strides, the tails of shorter vectors
    off, ln, blob = G.pack_requests([rq] * 8, m.fields())
    rc, f, p, vals = _raw_parse(s, res, mode, off, ln, blob.tobytes(), len(m.fields()), value_base=5, fill=7)
    assert rc == 0 and (vals[:5] == 7).all() and (vals[5 + 4 * 6:5 + 5 * 6] == 7).all()
    assert [int(x) for x in vals[5 + 2 * 6:5 + 3 * 6]] == [0, param_value("$D"), 7, 7, 7, 7]
    eng.close()


def _items(rows):
    arr = (_lib.SgaGatewayItem * len(rows))()
    for a, (res, index, fld) in zip(arr, rows):
        a.resource, a.index, a.field = res, index, fld
    return arr


def test_items_sharing_an_index_leave_a_null_slot():
    """A table loaded through the C ABI with two items on index 0: the array has two slots, the later item writes
    slot 0 and slot 1 stays null."""
    eng = _engine(1 << 12)
    s = LocalSentinel(eng, ["r"])
    L = _lib.load()
    assert L.sga_gateway_load(eng.handle, _items([(0, 0, 0), (0, 0, 1)]), 2, None, 0, 2) == 0
    rc, f, p, vals = _raw_parse(s, [0], [0], [0, 1], [1, 2], b"abc", 2, max_args=2)
    assert rc == 0 and _vector(p, vals, 0) == [0, param_value("bc"), 1 << 62, 0]
    # an index past the resource's items, a field past n_fields, a resource past the engine's: refused
    assert L.sga_gateway_load(eng.handle, _items([(0, 1, 0)]), 1, None, 0, 1) == _lib.SGA_EINVAL
    assert L.sga_gateway_load(eng.handle, _items([(0, 0, 1)]), 1, None, 0, 1) == _lib.SGA_EINVAL
    assert L.sga_gateway_load(eng.handle, _items([(1, 0, 0)]), 1, None, 0, 1) == _lib.SGA_EINVAL
    # the refused loads left the table; clearing it makes parse a no-op
    assert L.sga_gateway_load(eng.handle, None, 0, None, 0, 0) == 0
    rc, f, p, vals = _raw_parse(s, [0], [0], [], [], b"", 0, max_args=0)
    assert rc == 0 and f[0] == 0 and p[0] == 0
    eng.close()


def test_64_arguments_are_served_and_65_refused():
    rules = [gt.rule(resource="r", count=k + 1, item={"parse_strategy": 2, "field_name": f"h{k % 3}"})
             for k in range(63)] + [gt.rule(resource="r", count=100)]
    eng, s, m = _sentinel(["r"], rules)
    assert m.max_args == 64
    rq = {("header", "h0"): "a", ("header", "h1"): "b"}
    f, p, vals = m.parse([0, 0], [0, 0], [rq, {}])
    by_res, _ = gt.assign(rules)
    assert _vector(p, vals, 0) == _expected(gt.parse(by_res["r"], 0, rq)) and int(p[1]) == (128 << 32) | 64
    assert _vector(p, vals, 1) == [1 << 62, 0] * 63 + [0, param_value("$D")]
    with pytest.raises(ValueError, match="65 arguments"):
        m.load_rules([gt.to_product(r) for r in rules] + [G.GatewayFlowRule("r", count=1, param_item=G.GatewayParamFlowItem())])
    assert _lib.load().sga_gateway_load(eng.handle, _items([(0, k, 0) for k in range(64)] + [(0, -1, 0)]), 65, None,
                                        0, 1) == _lib.SGA_ERANGE
    assert m.parse([0], [0], [rq])[1][0] == 64  # the refused loads changed nothing
    eng.close()


# ---- 4. decisions end to end
E2E_NAMES = [f"route{k}" for k in range(6)] + ["plain"]
E2E_RULES = [
    gt.rule(resource="route0", count=3, burst=2, item={"parse_strategy": 0}),
    gt.rule(resource="route1", count=5, control_behavior=2, max_queueing_timeout_ms=200,
            item={"parse_strategy": 2, "field_name": "X-Tier", "pattern": "tier-3", "match_strategy": 0}),
    gt.rule(resource="route2", count=2, item={"parse_strategy": 3, "field_name": "q", "pattern": "ab",
                                              "match_strategy": 3}),
    gt.rule(resource="route3", count=4, interval_sec=2),
    gt.rule(resource="route4", grade=0, count=1, item={"parse_strategy": 4, "field_name": "sid"}),
    gt.rule(resource="route5", count=4, item={"parse_strategy": 0}),
    gt.rule(resource="route5", count=6, item={"parse_strategy": 2, "field_name": "X-Tier"}),
]
E2E_OWN = [{"resource": 5, "count": 3.0, "param_idx": -1}, {"resource": 6, "count": 2.0, "param_idx": 0}]


def _e2e_request(rng):
    return {("client_ip", ""): f"10.0.{rng.integers(0, 4)}.{rng.integers(0, 5)}",
            ("header", "X-Tier"): f"tier-{rng.integers(0, 20)}",
            ("url_param", "q"): ["ab", "xab", "cab-é", "none", "b", ""][rng.integers(0, 6)] + str(rng.integers(0, 4)),
            ("cookie", "sid"): f"session-{rng.integers(0, 20):04d}-€"}


@pytest.fixture(scope="module")
def e2e():
    """The stream, generated once by driving an oracle entry by entry (passed entries get exits with the same
    arguments), and the expected decisions of a fresh oracle replaying it."""
    ids = {n: i for i, n in enumerate(E2E_NAMES)}
    by_res, conv = gt.assign(E2E_RULES)
    orules = []
    for name in by_res:
        for c in conv[name]:
            orules.append(dict(c, resource=ids[name], hot={param_value(k): v for k, v in c["hot"].items()}))
    orules += E2E_OWN
    rng = np.random.default_rng(11)
    gen = lt.Oracle(len(E2E_NAMES), [], orules)
    pvals, ev, rqs, heap, seq = [], [], [], [], 0

    def drive(kind, rid, t, rt, args):
        loc = []
        word = lt.encode_args([None if a is None else param_value(a) for a in args], loc)
        cols = [np.array([kind], np.uint8), np.array([rid], np.uint32), np.array([t], np.int64),
                np.array([1], np.int32), np.array([32], np.uint8), np.array([rt], np.int64),
                np.array([word], np.uint64)]
        lv = np.ascontiguousarray(loc or [0], dtype=np.uint64)
        dec, wt = np.zeros(1, np.int8), np.zeros(1, np.int32)
        gen.L.orc_flow_replay_args(gen.h, 1, *[a.ctypes.data for a in cols], lv.ctypes.data, dec.ctypes.data,
                                   wt.ctypes.data)
        return int(dec[0])

    def record(kind, rid, t, rt, args, rq):
        word = lt.encode_args([None if a is None else param_value(a) for a in args], pvals)
        ev.append((kind, rid, t, 1, 32, rt, word))
        rqs.append(rq)

    t = float(T0)
    for _ in range(4000):
        t += rng.exponential(0.5)
        now = int(t)
        while heap and heap[0][0] <= now:
            te, _, rid, rt, args, rq = heapq.heappop(heap)
            drive(1, rid, te, rt, args)
            record(1, rid, te, rt, args, rq)
        rid = int(rng.integers(0, len(E2E_NAMES)))
        rq = _e2e_request(rng)
        name = E2E_NAMES[rid]
        args = gt.parse(by_res[name], 0, rq) if name in by_res else [rq[("client_ip", "")]]
        d = drive(0, rid, now, 0, args)
        record(0, rid, now, 0, args, rq)
        if d in (0, 4):
            rt = int(rng.integers(0, 40))
            heapq.heappush(heap, (now + rt, seq, rid, rt, args, rq))
            seq += 1
    while heap:
        te, _, rid, rt, args, rq = heapq.heappop(heap)
        drive(1, rid, te, rt, args)
        record(1, rid, te, rt, args, rq)
    gen.close()
    a = np.array(ev, dtype=np.uint64).reshape(-1, 7)
    st = {"kind": a[:, 0].astype(np.uint8), "resource": a[:, 1].astype(np.uint32), "ts": a[:, 2].astype(np.int64),
          "acquire": a[:, 3].astype(np.int32), "flags": a[:, 4].astype(np.uint8), "rt": a[:, 5].astype(np.int64),
          "param": a[:, 6].copy(), "param_values": np.array(pvals, dtype=np.uint64)}
    orc = lt.Oracle(len(E2E_NAMES), [], orules)
    exp = orc.replay(st)
    end = int(st["ts"].max())
    views = [orc.node(r, end) for r in range(len(E2E_NAMES))]
    orc.close()
    d = exp[0][st["kind"] == 0]
    assert (d == 0).sum() > 50 and (d == 2).sum() > 50
    assert (exp[1][(st["kind"] == 0) & (st["resource"] == 1)] > 0).sum() > 5  # the throttling rule queued some
    for r in range(6):  # every route blocks some and passes some
        dr = exp[0][(st["kind"] == 0) & (st["resource"] == r)]
        assert (dr == 2).any() and np.isin(dr, (0, 4)).any(), r
    return st, rqs, exp, views, end


def _e2e_sentinel(max_batch):
    eng, s, m = _sentinel(E2E_NAMES, E2E_RULES, max_batch)
    ParamFlowRuleManager(s).load_rules([ParamFlowRule(resource=E2E_NAMES[r["resource"]], count=r["count"],
                                                      param_idx=r["param_idx"]) for r in E2E_OWN])
    return eng, s, m


def _plain_columns(st, rqs):
    """The stream as a front end hands it over: the gateway routes' events bare, the ordinary resource's events
    with their one argument as the param column."""
    plain = st["resource"] == 6
    flags = np.where(plain, 4, 0).astype(np.uint8)
    param = np.array([param_value(rq[("client_ip", "")]) if pl else 0 for rq, pl in zip(rqs, plain)], np.uint64)
    return flags, param


def _assert_views(s, views, end):
    for rid, exp in enumerate(views):
        v = s.node(rid, end)
        assert [getattr(v, g) for g in lt.NODE_GETTERS] == exp, rid


@pytest.mark.parametrize("max_batch", [1 << 14, 2048])
def test_parsed_traffic_decides_like_the_oracle(e2e, max_batch):
    """parse + submit; with max_batch 2048 the parse call splits the batch itself (n > max_batch)."""
    st, rqs, exp, views, end = e2e
    assert len(st["kind"]) > 2048
    eng, s, m = _e2e_sentinel(max_batch)
    flags, param = _plain_columns(st, rqs)
    f, p, vals = m.parse(st["resource"], np.zeros(len(rqs), np.uint8), rqs, flags=flags, param=param)
    got = s.submit(st["kind"], st["resource"], st["ts"], st["acquire"], f, st["rt"], p, vals)
    _assert_same(st, got, exp, f"gateway traffic, max_batch {max_batch}")
    _assert_views(s, views, end)
    eng.close()


def test_parsed_traffic_on_the_device_entry(e2e):
    """parse_device + submit_device over torch tensors, the vectors behind 1,000 words of other values."""
    import torch
    st, rqs, exp, views, end = e2e
    eng, s, m = _e2e_sentinel(1 << 14)
    n, base = len(rqs), 1000
    dev = torch.device("cuda", eng.device)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731
    flags, param = _plain_columns(st, rqs)
    off, ln, blob = G.pack_requests(rqs, m.fields())
    d_flags, d_param = t(flags), t(param.view(np.int64))
    d_vals = torch.zeros(base + 2 * m.max_args * n, dtype=torch.int64, device=dev)
    d_res = t(st["resource"].view(np.int32))
    m.parse_device(d_res, t(np.zeros(n, np.uint8)), t(off.view(np.int32)), t(ln.view(np.int32)), t(blob), d_flags,
                   d_param, d_vals, value_base=base)
    ts_base = int(st["ts"].min())
    dec, wait = s.submit_device(t(st["kind"]), d_res, ts_base, t((st["ts"] - ts_base).astype(np.int32)),
                                t(st["acquire"]), d_flags, t(st["rt"]), d_param, d_vals)
    s.device_status()
    first = int(np.nonzero(st["resource"] != 6)[0][0])
    assert int(d_param[first].item()) >> 32 == base + 2 * m.max_args * first
    _assert_same(st, (dec.cpu().numpy(), wait.cpu().numpy()), exp, "gateway traffic, device entry")
    _assert_views(s, views, end)
    eng.close()


# ---- 5. attribution
def test_blocked_gateway_entry_names_the_converted_rule():
    rules = [gt.rule(resource="route", count=1, item={"parse_strategy": 0}),
             gt.rule(resource="route", count=0, item={"parse_strategy": 2, "field_name": "X", "pattern": "vip",
                                                      "match_strategy": 0})]
    eng, s, m = _sentinel(["other", "route"], rules, 1 << 12, block_log=True)
    conv = m.get_converted_param_rules("route")
    # the header rule's hot item lets "$NM" through; "vip" meets count 0
    rq = {("client_ip", ""): "7.7.7.7", ("header", "X"): "guest"}
    e = s.gateway_entry("route", 0, rq, T0)
    assert e.args == ("7.7.7.7", "$NM")
    with pytest.raises(ParamFlowException) as x:
        s.gateway_entry("route", 0, rq, T0 + 1)
    assert x.value.rule is conv[0] and x.value.rule_limit_app == "7.7.7.7"
    with pytest.raises(ParamFlowException) as y:
        s.gateway_entry("route", 0, {("client_ip", ""): "8.8.8.8", ("header", "X"): "vip"}, T0 + 2)
    assert y.value.rule is conv[1] and y.value.rule_limit_app == "vip"
    e.exit(T0 + 3)
    rows, lost, _ = s.block_rows()
    assert lost == 0 and len(rows) == 2
    got = {(int(r["tag"]), s.block_rule_index(Decision.BLOCK_PARAM, int(r["resource"]), int(r["detail"])))
           for r in rows}
    assert got == {(param_value("7.7.7.7"), 0), (param_value("vip"), 1)}
    assert s.param_texts[(param_value("vip"), 0)] == "vip"
    # a route-mode rule under an API request: no arguments, nothing to limit
    s.gateway_entry("route", 1, rq, T0 + 4).exit(T0 + 4)
    eng.close()


# ---- 6. bad input
def test_bad_slices_and_short_buffers_are_reported_not_applied():
    import torch
    rules = [gt.rule(resource="r", count=1, item={"parse_strategy": 0}),
             gt.rule(resource="r", count=2, item={"parse_strategy": 2, "field_name": "H"})]
    eng, s, m = _sentinel(["r", "plain"], rules, 1 << 12)
    n = 4
    res = np.array([0, 1, 0, 0], np.uint32)
    blob = b"0123456789"
    off = np.array([0, 2, 0, 0, 4, 8, 1, 9], np.uint32)
    ln = np.array([2, 2, 0, 0, 2, 3, NULL, 1], np.uint32)  # event 2's header slice ends one byte past the blob
    rc, f, p, vals = _raw_parse(s, res, np.zeros(n), off, ln, blob, 2, max_args=2)
    assert rc == _lib.SGA_EINVAL
    assert int(p[2]) == REFUSED and f[2] == EV_ARGS and f[1] == 0
    assert _vector(p, vals, 0) == [0, param_value("01"), 0, param_value("23")]
    assert _vector(p, vals, 3) == [1 << 62, 0, 0, param_value("9")]
    kind, ts, acq = np.zeros(n, np.uint8), np.full(n, T0, np.int64), np.ones(n, np.int32)
    with pytest.raises(_lib.EngineError):
        s.submit(kind, res, ts, acq, f, None, p, vals)
    # a value buffer one word short of the last event's vector
    ln[5] = 2
    rc, f, p, vals = _raw_parse(s, res, np.zeros(n), off, ln, blob, 2, n_values=4 * n - 1)
    assert rc == _lib.SGA_EINVAL and int(p[3]) == REFUSED and int(p[2]) == (8 << 32) | 2
    rc, f, p, vals = _raw_parse(s, res, np.zeros(n), off, ln, blob, 2, n_values=4 * n)
    assert rc == 0
    # the device form reports through the status call, and the poisoned chunk is refused by the device entry
    dev = torch.device("cuda", eng.device)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731
    ln[5] = 3
    d_flags, d_param = t(np.zeros(n, np.uint8)), t(np.zeros(n, np.int64))
    d_vals = torch.zeros(4 * n, dtype=torch.int64, device=dev)
    d_res = t(res.view(np.int32))
    m.parse_device(d_res, t(np.zeros(n, np.uint8)), t(off.view(np.int32)), t(ln.view(np.int32)),
                   t(np.frombuffer(blob, np.uint8)), d_flags, d_param, d_vals)
    with pytest.raises(_lib.EngineError):
        s.device_status()
    s.device_status()  # reported once
    dec, _ = s.submit_device(t(kind), d_res, T0, t(np.zeros(n, np.int32)), t(acq), d_flags, None, d_param, d_vals)
    with pytest.raises(_lib.EngineError):
        s.device_status()
    assert (dec.cpu().numpy() == -1).all()
    d_small = torch.zeros(4 * n - 1, dtype=torch.int64, device=dev)
    ln[5] = 2
    m.parse_device(d_res, t(np.zeros(n, np.uint8)), t(off.view(np.int32)), t(ln.view(np.int32)),
                   t(np.frombuffer(blob, np.uint8)), d_flags, d_param, d_small)
    with pytest.raises(_lib.EngineError):
        s.device_status()
    for rid in (0, 1):  # nothing was applied
        v = s.node(rid, T0)
        assert v.total_pass == 0 and v.total_block == 0 and v.cur_thread_num == 0
    eng.close()
