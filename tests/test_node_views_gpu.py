"""GPU parity of the bulk node views (sga_query_nodes / sga_query_nodes_device, the k_node_views kernel: one wave
per node).

Bar: every row equals sga_query_node on a second engine fed the same stream, all 16 fields bit for bit, and both
equal the oracle's getters (tests/local_trace.py, tests/origin_trace.py, tests/context_trace.py -- no new model);
traffic after a query is decided alike on both engines, so the query's rotations are the single query's."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import context_trace as ct
from tests import local_trace as lt

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000  # a multiple of 60,000: second, minute-bucket and minute-window starts coincide
ENTRY = 0xFFFFFFFF
RES, ORG, CTX = 0, 1, 2  # SGA_NODES_*
NOT_ZERO = 1
N_RES = 300


# ------------------------------------------------------------------ helpers
def _sentinel(n_res, rules=None, origins=0, contexts=0, max_batch=1 << 14, max_nodes=0):
    from sentinel_amd.cluster import Engine
    from sentinel_amd.local import LocalSentinel
    from tests.test_local_parity_gpu import _load
    eng = Engine(max_batch=max_batch)
    s = LocalSentinel(eng, [f"r{i}" for i in range(n_res)],
                      [f"o{i + 1}" for i in range(origins)] or None, max_nodes,
                      [f"c{i + 1}" for i in range(contexts)] or None, max_nodes)
    if rules:
        _load(s, rules)
    return eng, s


def _submit(s, st):
    if not len(st["kind"]):
        return np.zeros(0, np.int8), np.zeros(0, np.int32)
    return s.submit(st["kind"], st["resource"], st["ts"], st["acquire"], st["flags"], st["rt"], st["param"],
                    origin=st.get("origin"), context=st.get("context"))


def _views(rows):
    """{(resource, other): the 16 getters} of a NODE_ROW_DTYPE array; the rows must come sorted."""
    keys = [(int(r["resource"]), int(r["other"])) for r in rows]
    assert keys == sorted(keys) and len(set(keys)) == len(keys), keys
    return {k: [r[g].item() for g in lt.NODE_GETTERS] for k, r in zip(keys, rows)}


def _single(s, rid, now):
    v = s.node(rid, now)
    return [getattr(v, g) for g in lt.NODE_GETTERS]


def _ev(rows):
    """(kind, resource, ts, acquire, flags, rt) rows."""
    x = np.array(rows, dtype=np.int64).reshape(-1, 6)
    return {"kind": x[:, 0].astype(np.uint8), "resource": x[:, 1].astype(np.uint32), "ts": x[:, 2].copy(),
            "acquire": x[:, 3].astype(np.int32), "flags": x[:, 4].astype(np.uint8), "rt": x[:, 5].copy(),
            "param": np.zeros(len(x), np.uint64)}


def _raw(s, table, ids, now, flags, cap):
    """sga_query_nodes as the C ABI gives it: (rc, n_out, rows)."""
    from sentinel_amd import _lib
    from sentinel_amd.local import NODE_ROW_DTYPE
    out = np.zeros(max(1, cap), dtype=NODE_ROW_DTYPE)
    a = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32)
    n = C.c_size_t(12345)
    rc = _lib.load().sga_query_nodes(s.engine.handle, table, None if a is None else a.ctypes.data,
                                     0 if a is None else len(a), now, flags, out.ctypes.data, cap, C.byref(n))
    return rc, n.value, out


# ------------------------------------------------------------------ 1: node counts around the block's 4 waves
COUNTS = [0, 1, 3, 4, 5, 63, 64, 65, 257]
RULES = [{"resource": r, "count": 2} for r in range(N_RES)]


@functools.lru_cache(maxsize=None)
def _count_trace(n):
    """n of 300 resources entered (ids drawn at random), QPS 2 each: two chunks, about 4 entries a resource each,
    with exits and errors; the second starts 700 ms after the first ends.  Expected: the oracle's getters of the
    n nodes at `now1` (read once, so that the oracle rotates as the engines do), its decisions of the second
    chunk, and the getters at `now2`."""
    rng = np.random.default_rng(100 + n)
    chosen = np.sort(rng.choice(N_RES, size=n, replace=False)).astype(np.uint32)
    orc = lt.Oracle(N_RES, RULES)
    if n == 0:
        orc.close()
        return chosen, [lt.empty_stream()] * 2, [T0 + 10, T0 + 20], [{}, {}], None
    gen = lt.Oracle(n, RULES[:n])
    first = _ev([(0, r, T0 - 5, 1, 0, 0) for r in range(n)])  # one pass each ahead of the drawn traffic, never
    gen.replay(first)                                         # exited: all n are entered by the first chunk
    chunks = []
    for k in range(2):
        st = lt.generate(gen, n, 4 * n + 3, 7 + k, T0, gap_mean=400.0 / n, acq_max=2, err_pct=0.2, rt_max=30,
                         zipf=False, t_start=T0 if k == 0 else int(chunks[0]["ts"].max()) + 700)
        if k == 0:
            st = lt.concat(first, st)
        st["resource"] = chosen[st["resource"]]
        chunks.append(st)
    gen.close()
    nows, exp, dec = [], [], None
    for k, st in enumerate(chunks):
        d = orc.replay(st)
        if k == 1:
            dec = d
        nows.append(int(st["ts"].max()) + 130)
        exp.append({(int(r), 0): orc.node(int(r), nows[k]) for r in chosen})
    orc.close()
    # the draw must have entered every chosen resource in the first chunk: the counts are what the case is about
    assert set(chunks[0]["resource"][chunks[0]["kind"] == 0]) == set(chosen)
    assert any(v[lt.NODE_GETTERS.index("total_block")] for v in exp[0].values()) or n < 3
    return chosen, chunks, nows, exp, dec


@pytest.mark.parametrize("n", COUNTS)
def test_rows_equal_single_queries_and_rotate_alike(n):
    chosen, chunks, nows, exp, dec = _count_trace(n)
    ea, a = _sentinel(N_RES, RULES)
    eb, b = _sentinel(N_RES, RULES)
    for k in range(2):
        da, db = _submit(a, chunks[k]), _submit(b, chunks[k])
        assert (da[0] == db[0]).all() and (da[1] == db[1]).all(), ("decisions differ after the bulk query", k)
        if k == 1 and dec is not None:
            assert (da[0] == dec[0]).all() and (da[1] == dec[1]).all()
        got = _views(a.query_nodes(RES, nows[k]))
        assert sorted(got) == [(int(r), 0) for r in chosen], (n, k)
        for key, v in got.items():
            assert v == _single(b, key[0], nows[k]), ("bulk != single", key, list(zip(lt.NODE_GETTERS, v)))
            assert v == exp[k][key], ("bulk != oracle", key, list(zip(lt.NODE_GETTERS, v, exp[k][key])))
    ea.close()
    eb.close()


# ------------------------------------------------------------------ 2: bucket ages and special nodes
@functools.lru_cache(maxsize=None)
def _edge_trace():
    """One stream; each resource is read once, at its own `now`, by an explicit one-id list.
    0-2: a pass at T0 (minute bucket and second bucket start T0) and one at T0 + 1000, read when the first minute
         bucket is 59,999 / 60,000 / 60,001 ms old;
    3-5: a pass at T0, read when its second bucket is 999 / 1,000 / 1,001 ms old; 6-8: the same for the second
         bucket of T0 + 500;
    9:   a pass and an exit in every second of a minute (all 60 minute buckets live), read in the 60th;
    10:  QPS 1: a pass, then a prioritized entry that borrows from the next window (PASS_WAIT): waiting = 1.  A
         lone prioritized entry either passes outright or is refused, so the pass ahead of it is needed;
    11:  passes without an exit: min_rt stays statistic_max_rt;
    12:  inbound passes and exits (ENTRY_NODE receives them);
    13:  never touched; 14: only an exit."""
    rows, reads = [], {}
    for k, age in enumerate((59_999, 60_000, 60_001)):
        rows += [(0, k, T0, 1, 0, 0), (0, k, T0 + 1000, 2, 0, 0), (1, k, T0 + 1010, 2, 0, 10)]
        reads[k] = T0 + age
    for k, age in enumerate((999, 1000, 1001)):
        rows += [(0, 3 + k, T0, 1, 0, 0), (1, 3 + k, T0 + 7, 1, 2, 7)]
        reads[3 + k] = T0 + age
        rows += [(0, 6 + k, T0 + 20, 1, 0, 0), (0, 6 + k, T0 + 500, 2, 0, 0), (1, 6 + k, T0 + 510, 2, 0, 10)]
        reads[6 + k] = T0 + 500 + age
    for sec in range(60):
        rows += [(0, 9, T0 + 1000 * sec + 5, 1 + sec % 3, 0, 0), (1, 9, T0 + 1000 * sec + 45, 1 + sec % 3, 0, 40)]
    reads[9] = T0 + 59_700
    rows += [(0, 10, T0 + 100, 1, 0, 0), (0, 10, T0 + 600, 1, 1, 0)]
    reads[10] = T0 + 601
    rows += [(0, 11, T0 + 50, 1, 0, 0), (0, 11, T0 + 60, 1, 0, 0)]
    reads[11] = T0 + 300
    rows += [(0, 12, T0 + 30, 1, 8, 0), (1, 12, T0 + 50, 1, 8, 20), (0, 12, T0 + 70, 2, 8, 0)]
    reads[12] = T0 + 200
    reads[13] = T0 + 200
    rows += [(1, 14, T0 + 90, 1, 0, 9)]
    reads[14] = T0 + 200
    rows.sort(key=lambda r: r[2])
    st = _ev(rows)
    rules = [{"resource": r, "count": 1000} for r in range(15) if r != 10] + [{"resource": 10, "count": 1}]
    orc = lt.Oracle(15, rules)
    dec = orc.replay(st)
    assert dec[0][(st["resource"] == 10) & (st["flags"] == 1)][0] == 4  # PASS_WAIT
    exp = {r: orc.node(r, now) for r, now in reads.items()}
    exp[ENTRY] = orc.node(ENTRY, T0 + 200)
    orc.close()
    G = lt.NODE_GETTERS.index
    assert exp[0][G("total_pass")] == 3 and exp[2][G("total_pass")] == 2  # the old bucket counts, then does not
    assert exp[3][G("pass_qps")] == 1.0 and exp[4][G("pass_qps")] == 0.0
    assert exp[9][G("total_pass")] == sum(1 + s % 3 for s in range(60))
    assert exp[10][G("waiting")] == 1 and exp[11][G("min_rt")] == 5000.0 and exp[ENTRY][G("total_pass")] == 3
    return st, rules, reads, exp


def test_bucket_ages_and_special_nodes():
    st, rules, reads, exp = _edge_trace()
    ea, a = _sentinel(15, rules)
    eb, b = _sentinel(15, rules)
    _submit(a, st)
    _submit(b, st)
    for rid, now in reads.items():
        rows = a.query_nodes(RES, now, [rid])
        assert len(rows) == 1 and int(rows[0]["entered"]) == (0 if rid in (13, 14) else 1), rid
        got = _views(rows)[(rid, 0)]
        assert got == exp[rid], ("bulk != oracle", rid, list(zip(lt.NODE_GETTERS, got, exp[rid])))
        assert got == _single(b, rid, now), ("bulk != single", rid)
    # ENTRY_NODE by explicit id, beside a resource; absent from "all", like the two that were never entered
    rows = a.query_nodes(RES, T0 + 200, [ENTRY, 12])
    assert [int(r["resource"]) for r in rows] == [12, ENTRY]
    assert _views(rows)[(ENTRY, 0)] == exp[ENTRY] == _single(b, ENTRY, T0 + 200)
    assert a.nodes(T0 + 200, ["__total_inbound_traffic__"])[0][0] == "__total_inbound_traffic__"
    assert [int(r["resource"]) for r in a.query_nodes(RES, T0 + 60_001)] == list(range(13))
    ea.close()
    eb.close()


# ------------------------------------------------------------------ 3: notZero
def test_not_zero_keeps_the_nodes_with_requests():
    """Resources 0-2 pass or block at T0 + 61,500; 3-4 only at T0: entered, and totalRequest() == 0 a minute later;
    5 is never entered.  The expected set is read from the oracle's views."""
    rules = [{"resource": r, "count": 1} for r in range(6)]
    rows = [(0, r, T0 + 10 * r, 2 if r == 4 else 1, 0, 0) for r in (3, 4)]
    rows += [(0, r, T0 + 61_500 + j, 1, 0, 0) for r in (0, 1, 2) for j in range(1 + r)]
    rows.sort(key=lambda r: r[2])
    st = _ev(rows)
    now = T0 + 61_900
    orc = lt.Oracle(6, rules)
    orc.replay(st)
    exp = {(r, 0): orc.node(r, now) for r in range(5)}
    orc.close()
    G = lt.NODE_GETTERS.index
    total = {k: v[G("total_pass")] + v[G("total_block")] for k, v in exp.items()}
    keep = sorted(k for k, t in total.items() if t > 0)
    assert keep == [(0, 0), (1, 0), (2, 0)] and total[(3, 0)] == 0 and total[(4, 0)] == 0  # both kinds are there
    assert exp[(2, 0)][G("total_block")] == 2
    ea, a = _sentinel(6, rules)
    eb, b = _sentinel(6, rules)
    _submit(a, st)
    _submit(b, st)
    got = _views(a.query_nodes(RES, now, None, NOT_ZERO))
    assert sorted(got) == keep and all(got[k] == exp[k] for k in keep)
    assert [n for n, _ in a.nodes(now, not_zero=True)] == ["r0", "r1", "r2"]
    # a dropped node was rotated like a kept one: the full views agree with the other engine's and the oracle's
    allv = _views(a.query_nodes(RES, now))
    assert sorted(allv) == sorted(exp) and all(allv[k] == exp[k] == _single(b, k[0], now) for k in exp)
    got = _views(a.query_nodes(RES, now, [4, 1, 5], NOT_ZERO))
    assert sorted(got) == [(1, 0)]
    ea.close()
    eb.close()


# ------------------------------------------------------------------ 4: pair tables
P_RES, P_ORG, P_CTX = 7, 5, 3
P_RULES = [{"resource": 0, "count": 20}, {"resource": 3, "count": 5, "grade": 0}]


@functools.lru_cache(maxsize=None)
def _pair_trace():
    h = ct.ContextTrace(P_RES, P_ORG, P_CTX, P_RULES)
    h.generate(1500, 3, T0, [3, 2, 2, 2, 1, 1, 1], [1, 2, 2, 2, 1, 1], [1, 2, 2, 1], gap_mean=1.5, rt_max=39,
               err_pct=0.1)
    t_end = int(max(e[2] for e in h.ev)) + 60
    tr = h.finish(times=[t_end + 300])
    assert len(tr["onodes"]) == P_RES * P_ORG and len(tr["cnodes"]) == P_RES * P_CTX
    return tr


def _pair_sentinel(tr):
    eng, s = _sentinel(P_RES, P_RULES, P_ORG, P_CTX)
    d, w = _submit(s, tr["st"])
    assert (d == tr["ed"]).all() and (w == tr["ew"]).all()
    return eng, s


def test_pair_tables_all_rows_sorted_and_filtered():
    tr = _pair_trace()
    now = tr["times"][0]
    eng, s = _pair_sentinel(tr)
    for table, want in ((ORG, tr["onodes"]), (CTX, tr["cnodes"])):
        rows = s.query_nodes(table, now)
        assert all(int(r["entered"]) == 1 for r in rows)
        got = _views(rows)
        assert sorted(got) == sorted(want)
        for k, v in got.items():
            assert v == want[k][0], (table, k, list(zip(lt.NODE_GETTERS, v, want[k][0])))
        sub = _views(s.query_nodes(table, now, [5, 2]))  # the filter; rotations at one `now` are idempotent
        assert sorted(sub) == [k for k in sorted(want) if k[0] in (2, 5)]
        assert all(sub[k] == want[k][0] for k in sub)
    ov = s.origin_node_views("r2", now)
    assert [o for o, _ in ov] == [f"o{o}" for o in range(1, P_ORG + 1)]
    assert [getattr(ov[3][1], g) for g in lt.NODE_GETTERS] == tr["onodes"][(2, 4)][0]
    single = s.origin_node(2, 4, now)
    assert [getattr(single, g) for g in lt.NODE_GETTERS] == tr["onodes"][(2, 4)][0]
    dv = s.default_node_views(6, now)
    assert [c for c, _ in dv] == ["c1", "c2", "c3"]
    assert [getattr(dv[0][1], g) for g in lt.NODE_GETTERS] == tr["cnodes"][(6, 1)][0]
    # the resource table of the same engine
    got = _views(s.query_nodes(RES, now))
    assert all(got[(r, 0)] == tr["nodes"][r][0] for r in range(P_RES))
    eng.close()


def test_engine_without_pairs_gives_no_rows():
    eng, s = _sentinel(3)
    _submit(s, _ev([(0, 1, T0, 1, 0, 0)]))
    for table in (ORG, CTX):
        assert _raw(s, table, None, T0 + 5, 0, 8)[:2] == (0, 0)
        assert _raw(s, table, [1], T0 + 5, 0, 8)[:2] == (0, 0)
        assert len(s.query_nodes(table, T0 + 5)) == 0
    eng.close()


def test_pair_rolled_back_by_a_refused_chunk_is_absent():
    """max_origin_nodes = 4 and a chunk that needs a fifth record: refused (SGA_ENOMEM), the pair it named keeps a
    table slot without a node and appears in no bulk view."""
    from sentinel_amd._lib import EngineError
    eng, s = _sentinel(3, None, 3, 0, 1 << 12, 4)
    o = lambda st, org: dict(st, origin=np.array(org, np.uint32))  # noqa: E731
    four = o(_ev([(0, 0, T0, 1, 0, 0), (0, 0, T0 + 1, 1, 0, 0), (0, 1, T0 + 2, 1, 0, 0), (0, 2, T0 + 3, 1, 0, 0)]),
             [1, 2, 1, 3])
    assert list(_submit(s, four)[0]) == [0, 0, 0, 0]
    with pytest.raises(EngineError, match="rc=-12"):
        _submit(s, o(_ev([(0, 0, T0 + 5, 1, 0, 0), (0, 1, T0 + 6, 1, 0, 0)]), [1, 2]))
    rows = s.query_nodes(ORG, T0 + 20)
    assert [(int(r["resource"]), int(r["other"])) for r in rows] == [(0, 1), (0, 2), (1, 1), (2, 3)]
    assert all(int(r["total_pass"]) == 1 for r in rows)
    assert [(int(r["resource"]), int(r["other"])) for r in s.query_nodes(ORG, T0 + 20, [1])] == [(1, 1)]
    eng.close()


# ------------------------------------------------------------------ 5: errors
def test_bad_lists_are_refused_and_a_short_buffer_reports_the_count():
    from sentinel_amd._lib import SGA_EINVAL, SGA_ERANGE
    st = _ev([(0, r, T0 + r, 1, 0, 0) for r in range(5)])
    ea, a = _sentinel(6)
    eb, b = _sentinel(6)
    _submit(a, st)
    _submit(b, st)
    now = T0 + 2000  # past the second window: a rotation that had happened would show below
    for ids in ([1, 3, 1], [2, 6], [ENTRY, ENTRY]):
        assert _raw(a, RES, ids, now, 0, 8)[0] == SGA_EINVAL
    assert _raw(a, ORG, [0, 0], now, 0, 8)[0] == SGA_EINVAL  # checked ahead of "no such table"
    assert _raw(a, CTX, [ENTRY], now, 0, 8)[0] == SGA_EINVAL
    assert _raw(a, 3, None, now, 0, 8)[0] == SGA_EINVAL and _raw(a, RES, None, -1, 0, 8)[0] == SGA_EINVAL
    assert _raw(a, RES, None, now, 2, 8)[0] == SGA_EINVAL
    # nothing was launched: read at an earlier time, the nodes are what the other engine's are
    early = _views(a.query_nodes(RES, T0 + 10))
    assert sorted(early) == [(r, 0) for r in range(5)]
    assert all(early[(r, 0)] == _single(b, r, T0 + 10) for r in range(5))
    rc, n, _ = _raw(a, RES, None, T0 + 10, 0, 4)
    assert (rc, n) == (SGA_ERANGE, 5)
    rc, n, _ = _raw(a, RES, None, T0 + 10, 0, 0)
    assert (rc, n) == (SGA_ERANGE, 5)
    rc, n, rows = _raw(a, RES, None, T0 + 10, 0, 5)
    assert (rc, n) == (0, 5) and _views(rows[:5]) == early
    ea.close()
    eb.close()


# ------------------------------------------------------------------ 6: device entry
def test_device_entry_gives_the_same_rows():
    import torch
    from sentinel_amd import _lib
    from sentinel_amd.local import NODE_ROW_DTYPE
    tr = _pair_trace()
    now = tr["times"][0]
    eng, s = _pair_sentinel(tr)
    for table, want in ((RES, {(r, 0): v for r, v in tr["nodes"].items()}), (ORG, tr["onodes"]), (CTX, tr["cnodes"])):
        rows, count = s.nodes_device(now, table, stream=torch.cuda.current_stream())  # torch's reads follow it
        n = int(count.cpu()[0])
        assert n == len(want)
        host = rows.cpu().numpy().view(NODE_ROW_DTYPE).reshape(-1)[:n]
        host = host[np.lexsort((host["other"], host["resource"]))]
        assert host.tobytes() == s.query_nodes(table, now).tobytes()
        got = _views(host)
        assert all(got[k] == want[k][0] for k in want)
        # a buffer below the count: the full count, the first cap rows only
        rows, count = s.nodes_device(now, table, cap=3)  # on the engine stream: wait for it on the host
        assert _lib.load().sga_sync(s.engine.handle) == 0
        assert int(count.cpu()[0]) == len(want)
        part = rows.cpu().numpy().view(NODE_ROW_DTYPE).reshape(-1)
        assert len(part) == 3 and all(got[(int(r["resource"]), int(r["other"]))] ==
                                      [r[g].item() for g in lt.NODE_GETTERS] for r in part)
    rows, count = s.nodes_device(T0 + 70_000, RES, not_zero=True)
    assert _lib.load().sga_sync(s.engine.handle) == 0
    assert int(count.cpu()[0]) == 0
    eng.close()
