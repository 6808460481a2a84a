"""The concurrency checker's lines and gauges on the GPU: k_slog_conc behind every chunk of sga_concurrent_ops
(rows of kinds SGA_SLOG_CONC_PASS / _BLOCK / _RELEASE in the token server log) and k_conc_gauges
(sga_concurrent_gauges).

Expected rows never come from the engine: tests/conc_log_cases.reduce_conc forms them from the C oracle's statuses
of the same operations, and every call also asserts that the engine's statuses equal the oracle's.  Expected gauges
come from the oracle's nowCalls and the rule dicts.  count, events and nowCalls are integers and a level is the
rule's count or count * connectedCount formed by the same double product: every comparison is exact."""
import ctypes as C
import datetime
import itertools
import os

import numpy as np
import pytest

from tests import conc_log_cases as cc
from tests.conc_log_cases import CONC_BLOCK, CONC_PASS, CONC_RELEASE, T0, ConcPair, conc_rule
from tests.server_log_cases import as_tuples, expected_tuples

pytestmark = pytest.mark.gpu

ERANGE, EINVAL = -34, -22
INT64_MAX = (1 << 63) - 1


def _raw_gauges(eng, cap):
    """sga_concurrent_gauges as the C caller sees it: (rc, n, buffer, token_size)."""
    from sentinel_amd import _lib
    from sentinel_amd.cluster import CONC_GAUGE_DTYPE
    out = np.zeros(max(cap, 1), dtype=CONC_GAUGE_DTYPE)
    out.view(np.uint8)[:] = 0xA5
    n, size = C.c_size_t(), C.c_uint64(77)
    rc = _lib.load().sga_concurrent_gauges(eng.handle, out.ctypes.data, cap, C.byref(n), C.byref(size))
    return rc, int(n.value), out, int(size.value)


# ------------------------------------------------------------------ known answer
def test_kat_checker_sequence():
    """ConcurrentClusterFlowCheckerTest's sequence as test_concurrent_kat_sequences drives it, log on: ten passes,
    ten blocks, ten releases, one ALREADY_RELEASE; the rejected requests add nothing."""
    p = ConcPair([conc_rule(111, 10, 1, 500, 1000)], ns="1-name")
    svc, cid = p.svc, p.eng.client_id("127.0.0.1")
    acc, toks = {}, []
    for _ in range(10):
        got, st = p.acquire([111], [1], [T0], acc, client=cid)
        assert st[0] == cc.OK
        toks.append(int(got["token_id"][0]))
    for _ in range(10):
        assert p.acquire([111], [1], [T0], acc, client=cid)[1][0] == cc.BLOCKED
    for t in toks:
        assert p.release([t], [T0], acc)[1][0] == cc.RELEASE_OK
    assert svc.concurrent_now_calls(111) == 0 and svc.concurrent_token_count() == 0
    assert p.release([toks[0]], [T0], acc)[1][0] == cc.ALREADY_RELEASE
    assert p.acquire([111], [1], [T0], acc, client=cc.CLIENT_NONE)[1][0] == cc.BAD_REQUEST
    assert p.acquire([5], [1], [T0], acc, client=cid)[1][0] == cc.NO_RULE_EXISTS
    want = [(T0, 111, CONC_PASS, 0, 10, 10), (T0, 111, CONC_BLOCK, 0, 10, 10), (T0, 111, CONC_RELEASE, 0, 10, 10)]
    assert expected_tuples(acc) == want
    rows, le, lc = p.eng.server_log_rows()
    assert as_tuples(rows) == want and (le, lc) == (0, 0)
    p.close()


# ------------------------------------------------------------------ off by default
def test_off_by_default_and_log_changes_no_result():
    """The same seeded trace on two engines, log on and off: identical statuses, tokens issued at the same
    operations (the ids themselves come from each engine's random base, so each engine releases its own), nowCalls
    and token count; the drain of the engine without the log answers SGA_EINVAL."""
    from sentinel_amd import _lib
    rules = [conc_rule(f, 3 + f % 5) for f in range(1, 21)]
    on, off = ConcPair(rules), ConcPair(rules, log=None)
    rng = np.random.default_rng(11)
    held = []  # (token of `on`, token of `off`): an engine draws its token ids from a random base of its own
    for b in range(4):
        n = 700
        op = (rng.random(n) < 0.4).astype(np.uint8) if held else np.zeros(n, np.uint8)
        ids = np.where(op == 0, rng.integers(0, 23, size=n), 0).astype(np.int64)
        ids_off = ids.copy()
        for i in np.nonzero(op)[0]:
            ids[i], ids_off[i] = held[int(rng.integers(0, len(held)))]
        acq = rng.integers(0, 4, size=n).astype(np.int32)
        ts = T0 + 400 * b + np.sort(rng.integers(0, 400, size=n))
        g_on, _ = on.run(op, np.zeros(n, np.uint32), ids, acq, ts)
        g_off = off.svc.concurrent_ops(op, np.zeros(n, np.uint32), ids_off, acq, ts)
        assert g_on["status"].tobytes() == g_off["status"].tobytes(), b
        assert ((g_on["token_id"] != 0) == (g_off["token_id"] != 0)).all() and not g_off["reserved"].any()
        ok = g_on["status"] == 0
        held += list(zip(g_on["token_id"][ok].tolist(), g_off["token_id"][ok].tolist()))
        assert [on.svc.concurrent_now_calls(f) for f in range(1, 21)] == \
            [off.svc.concurrent_now_calls(f) for f in range(1, 21)]
        assert on.svc.concurrent_token_count() == off.svc.concurrent_token_count() == on.oracle_tokens()
    out = np.zeros(16, dtype=np.uint8)
    n = C.c_size_t()
    assert _lib.load().sga_server_log_drain(off.eng.handle, INT64_MAX, out.ctypes.data, 0, C.byref(n), None,
                                            None) == EINVAL
    assert len(on.eng.server_log_rows()[0]) > 0
    on.close()
    off.close()


# ------------------------------------------------------------------ wave and tile seams
_seam_case = itertools.count(1)


@pytest.fixture(scope="module")
def seam_pair():
    """One engine and one oracle for every seam case: each case drains everything it logged."""
    p = ConcPair(cc.seam_rules())
    yield p
    p.close()


@pytest.mark.parametrize("pattern", cc.SEAM_PATTERNS)
@pytest.mark.parametrize("n", cc.SEAM_SIZES)
def test_seams(seam_pair, n, pattern):
    """Sizes around the wave (64), the block (256) and the pass's four tiles (1,024); the held tuple, a tuple per
    lane, two tuples in turn, a held tuple displaced in a later tile, a second boundary inside the wave with times
    going backwards, and releases whose flowId and count come from the token's node."""
    p = seam_pair
    t0 = T0 + 10_000 * next(_seam_case)
    acc = {}
    if pattern == "release":
        rng = np.random.default_rng(n)
        acq = rng.integers(1, 4, size=n)
        got, st = p.acquire(np.full(n, cc.WIDE), acq, np.full(n, t0 + 5), acc)
        assert (st == cc.OK).all()
        op, cli, ids, junk, ts = cc.release_batch(got["token_id"], t0, rng)
        _, st = p.run(op, cli, ids, junk, ts, acc)
        assert int((st == cc.RELEASE_OK).sum()) == n and int((st == cc.BLOCKED).sum()) == (n + 2) // 3
        assert int((st == cc.ALREADY_RELEASE).sum()) == int((op == 1).sum()) - n
        rel = {k: v for k, v in acc.items() if k[2] == CONC_RELEASE}
        assert sum(v[0] for v in rel.values()) == int(acq.sum()) and sum(v[1] for v in rel.values()) == n
        assert all(k[1] == cc.WIDE and k[0] >= t0 for k in rel), "the token's flowId, the release's second"
        if n >= 65:
            assert len(rel) == 2, "the releases straddle a second"
    else:
        f, a, t = cc.seam_acquires(n, pattern, t0)
        _, st = p.acquire(f, a, t, acc)
        assert (st[f != cc.WIDE] == cc.BLOCKED).all() and (st[f == cc.WIDE] == cc.OK).all()
        assert sum(v[1] for v in acc.values()) == n
        if pattern == "distinct":
            assert len(acc) == min(n, 64)
        if pattern == "second" and n >= 64:
            assert len({k[0] for k in acc}) >= 2, "the acquires straddle a second"
        if n >= 2:
            assert any(v[0] != v[1] for v in acc.values()), "count differs from events"
    rows, le, lc = p.eng.server_log_rows()
    assert (le, lc) == (0, 0)
    assert as_tuples(rows) == expected_tuples(acc)
    assert len(p.eng.server_log_rows()[0]) == 0, "a drained log is empty"


# ------------------------------------------------------------------ chunks
def test_calls_longer_than_a_chunk():
    """max_batch = 4096 and calls of 4,097 and 9,000 operations: sga_concurrent_ops stages them in chunks and every
    chunk gets its pass.  A call's second chunk cannot release what its first acquired (the caller has no token
    yet), so the calls are acquire-only and release-only; the rows equal the reduce over the whole call."""
    rules = [conc_rule(f, 1e6 if f <= 4 else 40) for f in range(1, 9)]
    p = ConcPair(rules, max_batch=4096)
    rng = np.random.default_rng(21)
    acc, held = {}, []
    for k, n in enumerate((4097, 9000)):
        f = rng.integers(1, 9, size=n)
        got, st = p.acquire(f, rng.integers(1, 4, size=n), T0 + 2000 * k + np.sort(rng.integers(0, 1500, size=n)), acc)
        held.append(got["token_id"][st == cc.OK])
        assert (st == cc.BLOCKED).any()
    for k, n in enumerate((4097, 9000)):
        toks = held[k]
        ids = np.concatenate([toks, rng.choice(toks, size=n - len(toks))]) if len(toks) < n else toks[:n]
        ids = rng.permutation(ids)
        _, st = p.release(ids, T0 + 5000 + 2000 * k + np.sort(rng.integers(0, 1500, size=n)), acc, junk=9)
        assert (st == cc.RELEASE_OK).any() and (st == cc.ALREADY_RELEASE).any()
    rows, le, lc = p.eng.server_log_rows()
    assert (le, lc) == (0, 0) and as_tuples(rows) == expected_tuples(acc)
    assert {k[2] for k in acc} == {CONC_PASS, CONC_BLOCK, CONC_RELEASE}
    p.close()


# ------------------------------------------------------------------ random parity: rows and gauges
@pytest.mark.parametrize("dense", [True, False], ids=["dense", "hash"])
def test_random_parity_rows_and_gauges(dense):
    """The trace of test_concurrent_random_parity with the log on: invalid clients, ids and counts, unknown tokens,
    repeated releases, the expiry passes, the reloads and the clear-all at batch 20.  The union of the rows drained
    after every fourth batch (before_ms = the batch's last second) and at the end equals the reduce; expiry passes
    form no rows and releases of tokens whose rule a reload dropped (NO_RULE_EXISTS) none.  After every batch the
    gauges equal the oracle's nowCalls != 0 over the loaded rules with the test's own level, and token_size the
    oracle's cache size."""
    rng = np.random.default_rng(7 if dense else 8)
    base = 0 if dense else 10 ** 12
    ids = [base + 1 + k * (1 if dense else 7919) for k in range(60)]

    def mk(fid):
        return conc_rule(fid, float(rng.integers(1, 25)) + (0.5 if rng.random() < 0.3 else 0.0),
                         int(rng.random() < 0.7), int(rng.integers(200, 3000)), int(rng.integers(100, 2000)))

    rules = {fid: mk(fid) for fid in ids[:50]}
    p = ConcPair(list(rules.values()), connected=3)
    clients = [f"10.0.0.{i}:{4000 + i}" for i in range(8)]
    cids = [p.eng.client_id(a) for a in clients]
    outstanding, acc, drained = [], {}, []
    seen = {"neg": False, "dropped": False, "norule_release": False}
    now = T0
    for batch in range(36):
        n = int(rng.integers(500, 2500))
        op = np.zeros(n, np.uint8)
        cli = np.zeros(n, np.uint32)
        x = np.zeros(n, np.int64)
        a = np.zeros(n, np.int32)
        ts = now + np.sort(rng.integers(0, 300, size=n))
        for i in range(n):
            u = rng.random()
            if u < 0.5 or not outstanding:
                cli[i] = cids[int(rng.integers(0, 8))] if rng.random() > 0.01 else cc.CLIENT_NONE
                x[i] = ids[int(rng.integers(0, 60))] if rng.random() > 0.02 else int(rng.integers(-1, 2))
                a[i] = int(rng.integers(1, 4)) if rng.random() > 0.01 else 0
            elif u < 0.95:
                op[i] = 1
                x[i] = outstanding[int(rng.integers(0, len(outstanding)))]  # may repeat: ALREADY_RELEASE
            else:
                op[i] = 1
                x[i] = int(rng.integers(-(1 << 62), 1 << 62))
        got, st = p.run(op, cli, x, a, ts, acc)
        outstanding += [int(t) for t in got["token_id"][(op == 0) & (st == cc.OK)]]
        seen["norule_release"] |= bool(((op == 1) & (st == cc.NO_RULE_EXISTS)).any())
        want = p.expected_gauges()
        got_g, size = p.gauges()
        assert got_g == want, batch
        assert size == p.oracle_tokens() == p.svc.concurrent_token_count(), batch
        seen["neg"] |= any(g[2] < 0 for g in want)
        if outstanding:  # the draw the original spends on its cached-node samples: the traces stay the same
            rng.choice(outstanding, size=min(5, len(outstanding)), replace=False)
        now = int(ts[-1]) + 1
        if batch % 4 == 3:
            rows, le, lc = p.eng.server_log_rows(int(ts[-1]) - int(ts[-1]) % 1000)
            assert (le, lc) == (0, 0)
            drained += as_tuples(rows)
            now += int(rng.integers(0, 2500))
            online = [i for i in range(8) if rng.random() < 0.6]
            bits = np.zeros(1, np.uint32)
            for c in online:
                bits[0] |= np.uint32(1 << cids[c])
            removed = p.svc.expire_concurrent_tokens(now, [clients[c] for c in online])
            assert removed == p.L.orc_cluster_concurrent_expire(p.oh, now, bits.ctypes.data, len(cids))
            assert p.gauges() == (p.expected_gauges(), p.oracle_tokens()), "after the expiry pass"
        if batch % 9 == 8:  # reload: drop some rules, add others, change thresholds
            keep = [f for f in rules if rng.random() < 0.8]
            seen["dropped"] |= any(f not in keep and p.oracle_now_calls(f) for f in rules)
            rules = {f: dict(rules[f], count=float(rng.integers(1, 25))) for f in keep}
            for f in ids:
                if f not in rules and rng.random() < 0.3:
                    rules[f] = mk(f)
            p.load(list(rules.values()))
            assert p.gauges() == (p.expected_gauges(), p.oracle_tokens()), "after the reload"
        if batch == 20:  # clear-all, then back
            p.load([])
            assert p.gauges() == ([], p.oracle_tokens()) and p.oracle_tokens() > 0
            p.load(list(rules.values()))
            assert p.gauges() == ([], p.oracle_tokens()), "listed again only once something is acquired"
    rows, le, lc = p.eng.server_log_rows()
    assert (le, lc) == (0, 0)
    drained += as_tuples(rows)
    assert len(drained) == len(set(r[:4] for r in drained)), "a drain cuts at whole seconds"
    assert sorted(drained) == expected_tuples(acc)
    assert {k[2] for k in acc} == {CONC_PASS, CONC_BLOCK, CONC_RELEASE}
    assert seen == {"neg": True, "dropped": True, "norule_release": True}, seen
    p.close()


# ------------------------------------------------------------------ overflow
def test_overflow_lost_counters():
    """max_rows = 64 and 300 threshold-0 rules blocked in one second: a tuple that has a row never loses an update,
    the tuples without one are counted in the lost counters."""
    p = ConcPair([conc_rule(f, 0) for f in range(1, 301)], log=64)
    rng = np.random.default_rng(3)
    acc = {}
    for b in range(3):
        f = np.concatenate([np.arange(1, 301), rng.integers(1, 301, size=900)])
        _, st = p.acquire(f, rng.integers(1, 4, size=len(f)), np.full(len(f), T0 + 10 + b), acc)
        assert (st == cc.BLOCKED).all()
    assert len(acc) == 300
    rows, le, lc = p.eng.server_log_rows()
    got = as_tuples(rows)
    assert 8 < len(got) <= 64
    want = {r[:4]: r for r in expected_tuples(acc)}
    for r in got:
        assert want[r[:4]] == r, "a returned row equals the expected row of its key exactly"
    missing = [want[k] for k in want if k not in {r[:4] for r in got}]
    assert len(missing) == 300 - len(got)
    assert le == sum(r[5] for r in missing) and lc == sum(r[4] for r in missing)
    rows, le, lc = p.eng.server_log_rows()
    assert len(rows) == 0 and (le, lc) == (0, 0)
    p.close()


# ------------------------------------------------------------------ gauges
def test_gauges_before_any_concurrency_state():
    from sentinel_amd import cluster
    eng = cluster.Engine(max_batch=1 << 12)
    assert _raw_gauges(eng, 4)[:2] == (0, 0) and _raw_gauges(eng, 4)[3] == 0
    rows, size = eng.concurrent_gauges()
    assert len(rows) == 0 and size == 0
    eng.close()


@pytest.mark.parametrize("nrules", (1, 63, 64, 65, 257))
def test_gauge_compaction_seams(nrules):
    """Rule counts around the wave and past a block, with nonzero nowCalls on no slot, on the last slot only, on
    every 64th and on all: the ballot's prefix count and the per-wave append."""
    rules = [conc_rule(f, 1e6, threshold_type=f % 2) for f in range(1, nrules + 1)]
    p = ConcPair(rules, log=None, connected=3)
    assert p.gauges() == ([], 0)
    got, _ = p.acquire([nrules], [2], [T0])
    want = [(nrules, 1e6 if nrules % 2 else 3e6, 2)]
    assert p.expected_gauges() == want and p.gauges() == (want, 1)
    p.release(got["token_id"], [T0])
    assert p.gauges() == ([], 0)
    every = np.arange(1, nrules + 1, 64)
    got, _ = p.acquire(every, np.full(len(every), 3), np.full(len(every), T0))
    assert p.gauges() == (p.expected_gauges(), len(every)) and len(p.expected_gauges()) == len(every)
    p.release(got["token_id"], np.full(len(every), T0))
    allr = np.arange(1, nrules + 1)
    p.acquire(allr, 1 + allr % 3, np.full(nrules, T0))
    want = p.expected_gauges()
    assert len(want) == nrules and p.gauges() == (want, nrules)
    # one short: SGA_ERANGE, *n right, the buffer untouched
    rc, n, buf, size = _raw_gauges(p.eng, nrules - 1)
    assert (rc, n) == (ERANGE, nrules) and (buf.view(np.uint8) == 0xA5).all()
    rc, n, buf, size = _raw_gauges(p.eng, nrules)
    assert (rc, n, size) == (0, nrules, nrules)
    assert [(int(r["flow_id"]), float(r["level"]), int(r["now_calls"])) for r in buf[:n]] == want
    assert p.gauges() == (want, nrules), "the call changes no state"
    p.close()


def test_gauges_reload_clear_and_connected_count():
    """A rule dropped by a reload while it holds tokens is not listed and its tokens still count in token_size;
    after clear-all and reload a rule is listed again only once something is acquired; an AVG_LOCAL rule's level
    follows set_connected_count."""
    r1, r2 = conc_rule(10 ** 10 + 1, 5, threshold_type=0), conc_rule(10 ** 10 + 9, 7, threshold_type=1)
    p = ConcPair([r1, r2], log=None, connected=3)
    f1, f2 = r1["flow_id"], r2["flow_id"]
    p.acquire([f1, f1, f2], [2, 1, 4], [T0, T0, T0])
    assert p.gauges() == ([(f1, 15.0, 3), (f2, 7.0, 4)], 3) and p.expected_gauges() == p.gauges()[0]
    p.set_connected(4)
    assert p.gauges() == ([(f1, 20.0, 3), (f2, 7.0, 4)], 3) and p.expected_gauges() == p.gauges()[0]
    p.load([r1])  # r2 dropped while it holds a token
    assert p.gauges() == ([(f1, 20.0, 3)], 3) and p.oracle_tokens() == 3
    p.load([])
    assert p.gauges() == ([], 3)
    p.load([r1, r2])
    assert p.gauges() == ([], 3) and p.expected_gauges() == []
    p.acquire([f2], [1], [T0 + 1])
    assert p.gauges() == ([(f2, 7.0, 1)], 4) and p.expected_gauges() == p.gauges()[0]
    p.close()


# ------------------------------------------------------------------ end to end
def test_end_to_end_file(tmp_path):
    """One engine, two seconds with all three kinds, sample_gauges in each second, poll, close: the file's lines
    equal lines built from the reduce and the oracle's nowCalls."""
    from sentinel_amd.server_log import ServerLogWriter
    utc = datetime.timezone.utc
    rules = [conc_rule(3, 4), conc_rule(8, 2.5, threshold_type=0)]
    p = ConcPair(rules, connected=3)
    w = ServerLogWriter(p.eng, str(tmp_path), tz=utc)
    stamp = lambda slot: datetime.datetime.fromtimestamp(slot // 1000, utc).strftime("%Y-%m-%d %H:%M:%S")  # noqa: E731

    def row_lines(acc, slot):
        word = {CONC_PASS: "pass", CONC_BLOCK: "block", CONC_RELEASE: "release"}
        return [f"{stamp(slot)}|1|concurrent|{word[k[2]]}|{k[1]}|{v[0]},0" for k, v in sorted(acc.items())
                if k[0] == slot]

    def gauge_lines(slot):
        out = [f"{stamp(slot)}|1|concurrent|resource:r{fid}|flowId:{fid}l|concurrencyLevel:{level:.6f}l|"
               f"currentConcurrency|{calls},0" for fid, level, calls in p.expected_gauges()]
        return out + [f"{stamp(slot)}|1|flow|totalTokenSize|{p.oracle_tokens()},0"]

    acc = {}
    got, st = p.acquire([3, 3, 3, 8, 8, 3], [2, 2, 1, 7, 3, 1], T0 + np.arange(6) * 100, acc)
    assert st.tolist() == [0, 0, 1, 0, 1, 1]
    toks = got["token_id"]
    w.sample_gauges(T0 + 900)
    want = row_lines(acc, T0) + gauge_lines(T0)
    assert any("concurrencyLevel:7.500000l" in x for x in want) and want[-1].endswith("totalTokenSize|3,0")
    op, cli, ids, junk, ts = [1, 0, 1, 1], [cc.CLIENT_NONE, 0, cc.CLIENT_NONE, cc.CLIENT_NONE], \
        [toks[0], 3, toks[3], toks[0]], [50, 2, 50, 50], [T0 + 1000, T0 + 1100, T0 + 1200, T0 + 1300]
    _, st = p.run(np.array(op, np.uint8), np.array(cli, np.uint32), np.array(ids, np.int64), np.array(junk, np.int32),
                  np.array(ts, np.int64), acc)
    assert st.tolist() == [cc.RELEASE_OK, cc.OK, cc.RELEASE_OK, cc.ALREADY_RELEASE]
    assert w.poll(T0 + 1999) == len(want)
    with open(os.path.join(str(tmp_path), "sentinel-server.log"), "rb") as fh:
        assert fh.read() == ("\n".join(want) + "\n").encode()
    w.sample_gauges(T0 + 1900)
    want += row_lines(acc, T0 + 1000) + gauge_lines(T0 + 1000)
    w.close()
    with open(os.path.join(str(tmp_path), "sentinel-server.log"), "rb") as fh:
        assert fh.read().decode().splitlines() == want
    assert f"{stamp(T0 + 1000)}|1|concurrent|release|8|7,0" in want
    assert {k[2] for k in acc} == {CONC_PASS, CONC_BLOCK, CONC_RELEASE}
    p.close()
