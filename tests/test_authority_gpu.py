"""GPU parity of AuthoritySlot in the engine: AuthorityRules by origin (AuthorityRuleManager.java:110-164,
AuthorityRuleChecker.java:30-66), checked after the pair nodes are claimed and ahead of SystemSlot.

Bar: decisions and waits equal tests/authority_trace.py (the C oracle behind OriginTrace, failing entries driven as
kind 2 events); every node getter of every resource, origin node, DefaultNode and ENTRY_NODE identical at three
query times; metric rows and breaker states identical.  Checked against the trace and against a twin: a fresh
engine with the same rules minus authority, fed the pre-marked stream (the turned events as kind 2), which must
agree everywhere except 6 against 0 at the turned positions.  Each stream is built once and asserts on the CPU
that it holds authority blocks, authority passes and at least one other kind of block."""
import functools
import heapq
import json
from urllib.parse import quote

import numpy as np
import pytest

from tests import authority_trace as at
from tests import local_trace as lt
from tests import origin_trace as ot
from tests.test_origin_gpu import (MIX_DEGRADE, MIX_FLOW, MIX_ORG, MIX_PARAM, MIX_RES, _load, _load_flow, _mix_trace,
                                   _nodes, _same, _sentinel)

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000
ENTRY = 0xFFFFFFFF
EINVAL = "rc=-22"
WHITE, BLACK = at.WHITE, at.BLACK


# ------------------------------------------------------------------ engine side
def _names(n, p):
    return [f"{p}{i + (p == 'o')}" for i in range(n)]


def _load_auth(s, rules):
    from sentinel_amd.local import AuthorityRuleManager
    from sentinel_amd.rules import AuthorityRule
    return AuthorityRuleManager(s).load_rules([AuthorityRule(*r) for r in rules])


def _submit(s, st, origins=True):
    kw = {}
    if "context" in st:
        kw["context"] = st["context"]
    if "parent" in st:
        kw["parent"] = st["parent"]
    return s.submit(st["kind"], st["resource"], st["ts"], st["acquire"], st["flags"], st["rt"], st["param"],
                    st.get("param_values"), origin=st["origin"] if origins else None, **kw)


def _device(s, st):
    import torch
    dev = torch.device("cuda", 0)
    base = int(st["ts"].min())
    off = (st["ts"] - base).astype(np.uint32).view(np.int32)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    kind = t(st["kind"], np.uint8)
    keep = kind.clone()
    d, w = s.submit_device(kind, t(st["resource"], np.int32), base, t(off, np.int32), t(st["acquire"], np.int32),
                           flags=t(st["flags"], np.uint8), rt=t(st["rt"], np.int64), param=t(st["param"], np.int64),
                           origin=t(st["origin"], np.int32))
    s.device_status()
    assert bool((kind == keep).all()), "the device entry wrote the caller's kind buffer"
    return d.cpu().numpy(), w.cpu().numpy()


def _state(s, times, n_res, degrade=()):
    """Everything the bar names, read in bulk: rows of the three node tables at each time, then the metric rows
    and the breaker states."""
    from sentinel_amd import _lib
    out = []
    for now in times:
        out.append(s.query_nodes(_lib.SGA_NODES_RESOURCE, now, list(range(n_res)) + [ENTRY]).tobytes())
        out.append(s.query_nodes(_lib.SGA_NODES_ORIGIN, now).tobytes())
        out.append(s.query_nodes(_lib.SGA_NODES_CONTEXT, now).tobytes())
    out.append([(m.timestamp, m.resource, m.pass_qps, m.block_qps, m.success_qps, m.exception_qps, m.rt,
                 m.occupied_pass_qps) for m in s.metrics(times[-1] + 2000)])
    out.append([s.circuit_breaker_state(r["resource"], 0) for r in degrade])
    return out


def _twin_same(got, twin, turned, what):
    (gd, gw, gs), (td, tw, ts) = got, twin
    want = td.copy()
    assert (want[turned] == 0).all(), (what, "the twin answers 0 for its kind 2 events")
    want[turned] = 6
    bad = np.nonzero((gd != want) | (gw != tw))[0]
    assert not len(bad), (what, "twin decisions", len(bad), int(bad[0]), gd[bad[0]], want[bad[0]])
    for k, (a, b) in enumerate(zip(gs, ts)):
        assert a == b, (what, "twin state differs at part", k)


def _play(s, tr, key, calls, auth, submit=_submit):
    """calls: [(lo, hi, authority rules to load first or None)] over tr[key]."""
    gd, gw = [], []
    for lo, hi, rules in calls:
        if auth and rules is not None:
            _load_auth(s, rules)
        d, w = submit(s, lt.slice_stream(tr[key], lo, hi))
        gd.append(d)
        gw.append(w)
    return np.concatenate(gd), np.concatenate(gw)


# ------------------------------------------------------------------ 1: the kernel alone
LENS = [0, 1, 2, 3, 64, 65, 1000]
N_ORIGINS = 2100


@functools.lru_cache(maxsize=None)
def _kernel_case():
    """Resource k < 21: a rule whose resolved list has LENS[k % 7] ids (every other id from 3 on, written in a
    shuffled order with repeats and names nobody registered), strategy white / black / 2 by k // 7.  Resource 21: no
    rule.  Resource 22, the last id: a black list of one.  Probes per resource: origin 0, the first id, the last, the
    middle, below the first, above the last, absent between two ids, the largest registered id."""
    rng = np.random.default_rng(7)
    origins = [f"app{i}" for i in range(1, N_ORIGINS + 1)]
    resources = [f"r{i}" for i in range(23)]
    rules, lists = [], {}
    for k in range(21):
        ids = [3 + 2 * j for j in range(LENS[k % 7])]
        lists[k] = ids
        names = [f"app{i}" for i in ids] * 2 + ["nobody", "app", "app1x"]
        rng.shuffle(names)
        rules.append((f"r{k}", ",".join(names), [WHITE, BLACK, 2][k // 7]))
    rules.append(("r22", "app5", BLACK))
    rules.append(("r22", "app6", BLACK))  # the second rule of a resource is ignored
    lists[21], lists[22] = [], [5]
    pairs = []
    for k in range(23):
        ids = lists[k]
        probe = {0, 1, 2, N_ORIGINS}
        if ids:
            probe |= {ids[0], ids[-1], ids[len(ids) // 2], ids[0] - 1, ids[-1] + 1, ids[len(ids) // 2] + 1}
        pairs += [(k, o) for o in sorted(probe)]
    conf = at.load_authority_conf(rules)
    exp = [at.check(conf, resources[r], origins[o - 1] if o else "") for r, o in pairs]
    assert 40 < sum(exp) < len(exp) - 40
    return resources, origins, rules, pairs, exp


def test_authority_check_against_the_restatement():
    from sentinel_amd._lib import EngineError
    from sentinel_amd.cluster import Engine
    from sentinel_amd.local import LocalSentinel
    resources, origins, rules, pairs, exp = _kernel_case()
    eng = Engine(max_batch=1 << 12)
    s = LocalSentinel(eng, resources, origins, max_origin_nodes=64)
    assert s.authority_check([0, 22], [3, 5]).tolist() == [True, True]  # no rule loaded: no launch, all pass
    assert _load_auth(s, rules) == 22
    r = np.array([p[0] for p in pairs], np.uint32)
    o = np.array([p[1] for p in pairs], np.uint32)
    assert s.authority_check(r, o).tolist() == exp
    assert len(pairs) > 150
    rep_r, rep_o, rep_e = np.tile(r, 40), np.tile(o, 40), exp * 40
    assert len(rep_e) > 5000
    for n in (1, 63, 64, 65, 255, 256, 257, 1025):  # a lane an event: wave and workgroup seams, several workgroups
        assert s.authority_check(rep_r[:n], rep_o[:n]).tolist() == rep_e[:n], n
    assert s.authority_check(np.roll(rep_r, 5)[:5000], np.roll(rep_o, 5)[:5000]).tolist() == \
        (rep_e[-5:] + rep_e[:-5])[:5000]  # more than one piece of the batch capacity
    for bad_r, bad_o in (([23], [1]), ([0], [N_ORIGINS + 1]), ([ENTRY], [0])):
        with pytest.raises(EngineError, match=EINVAL):
            s.authority_check(bad_r, bad_o)
    # a load that names a resource, a strategy or an id out of range loads nothing
    from sentinel_amd import _lib
    L = _lib.load()
    for res, strat, ids in (([23], [0], [1]), ([0], [-1], [1]), ([0], [0], [0]), ([0], [0], [N_ORIGINS + 1])):
        a = [np.array(x, dt) for x, dt in ((res, np.uint32), (strat, np.int32), ([0, 1], np.uint32), (ids, np.uint32))]
        assert L.sga_load_authority_rules(eng.handle, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, 1,
                                          a[3].ctypes.data) == -22
    dec = np.array([0, 1], np.uint32)[::-1].copy()
    assert L.sga_load_authority_rules(eng.handle, a[0].ctypes.data, a[1].ctypes.data, dec.ctypes.data, 1,
                                      a[3].ctypes.data) == -22  # a decreasing list_off
    assert s.authority_check(r, o).tolist() == exp  # the table stands
    assert _load_auth(s, []) == 0
    assert s.authority_check(r, o).all()
    eng.close()


# ------------------------------------------------------------------ 2: each dispatch form
AUTH_1 = [("r0", "o4,o2", BLACK), ("r5", "o1", BLACK), ("r2", "o3,nobody,o1,o2", WHITE),
          ("r0", "o1", BLACK), ("r7", "o5", 2)]  # the fourth is redundant, the fifth passes everybody
AUTH_2 = [("r0", "o1", BLACK), ("r3", "o1,o2,o3,o4", WHITE)]
ORIGINS = _names(MIX_ORG, "o")
RES = _names(MIX_RES, "r")
SYSTEM = [{"qps": 150}]


def _generate(a, n, seed, t0, inbound):
    a.generate(n, seed, t0, [3, 2, 2, 2, 1, 2, 2, 2], [2, 3, 2, 1, 1, 0.5], gap_mean=1.0, acq_max=2, rt_max=39,
               regress_pct=0.02, inbound=inbound, err_pct=0.1, params=6, param_res=(5,))


def _holds_every_outcome(tr, inbound):
    st, ed = tr["st"], tr["ed"]
    d = ed[st["kind"] == 0]
    need = (0, 5, 6) if inbound else (0, 1, 2, 3, 6)  # under the SystemRule the later slots see fewer entries
    assert all((d == c).sum() >= 50 for c in need), np.bincount(d)
    assert tr["n_auth_pass"] >= 1000 and len(tr["turned"]) >= 300
    for rid in (0, 2, 5):  # every listed resource passes some origins and blocks others
        sel = (st["kind"] == 0) & (st["resource"] == rid) & (st["origin"] != 0)
        assert (ed[sel] == 6).sum() >= 30 and (ed[sel] != 6).sum() >= 30, rid
    assert (ed[(st["origin"] == 0)] != 6).all() and (ed[st["resource"] == 7] != 6).all()


@functools.lru_cache(maxsize=None)
def _auth_trace(kind):
    """The mixed workload of test_origin_gpu.py under AUTH_1.  "plain": 10,000 entries.  "reload": 5,000 entries, then
    AUTH_2 replaces AUTH_1 (tr["mark"]), then 5,000 more.  "inbound": every event EntryType.IN under a SystemRule of
    150 QPS, which blocks: the arrival-order lane."""
    inbound = kind == "inbound"
    h = ot.OriginTrace(MIX_RES, MIX_ORG, MIX_FLOW, MIX_PARAM, MIX_DEGRADE, system=SYSTEM if inbound else None)
    a = at.AuthorityTrace(h, RES, ORIGINS, AUTH_1)
    if kind == "reload":
        _generate(a, 5000, 21, T0, False)
        mark = len(h.ev)
        a.load(AUTH_2)
        _generate(a, 5000, 22, int(h.ev[-1][2]) + 5, False)
    else:
        _generate(a, 10000, 23 + inbound, T0, inbound)
        mark = None
    tr = a.finish(entry=inbound)
    tr["mark"] = mark
    st, ed = tr["st"], tr["ed"]
    if kind == "reload":
        first = tr["turned"] < mark
        assert first.sum() >= 100 and (~first).sum() >= 100
        late = st["resource"][tr["turned"][~first]]
        assert set(late.tolist()) == {0, 3}  # after the reload only AUTH_2 blocks
        d = ed[st["kind"] == 0]
        assert all((d == c).sum() >= 50 for c in (0, 1, 2, 3, 6)), np.bincount(d)
    else:
        _holds_every_outcome(tr, inbound)
    if inbound:
        # an authority-blocked entry is not system-checked: had it been, the ones right after a system block, in
        # the same saturated second, would have answered 5, and the twin (kind 2 there) could not agree
        ent = np.nonzero(st["kind"] == 0)[0]
        prev5 = np.zeros(len(ed), bool)
        prev5[ent[1:]] = ed[ent[:-1]] == 5
        assert prev5[tr["turned"]].sum() >= 20
        assert tr["nodes"][ENTRY][0][lt.NODE_GETTERS.index("total_block")] > len(tr["turned"])
    return tr


def _form(tr, max_batch, small, calls, degrade=MIX_DEGRADE, system=None, submit=_submit, what=""):
    out = []
    for auth in (True, False):
        eng, s = _sentinel(MIX_RES, MIX_ORG, max_batch, small)
        _load(s, MIX_FLOW, MIX_PARAM, MIX_DEGRADE, system)
        d, w = _play(s, tr, "st" if auth else "pre", calls, auth, submit)
        # both engines against the trace (the twin was fed what the oracle was driven with), by the same reads
        # in the same order: a read rotates the windows of what it reads
        _same(tr["st"], (d, w), tr["ed"] if auth else tr["twin_ed"], tr["ew"], what + ("" if auth else " twin"))
        _nodes(s, tr, MIX_RES, MIX_ORG, what)
        out.append((d, w, _state(s, tr["times"], MIX_RES, degrade)))
        eng.close()
    _twin_same(out[0], out[1], tr["turned"], what)


def test_host_pipeline_one_chunk():
    tr = _auth_trace("plain")
    _form(tr, 1 << 15, 0, [(0, len(tr["ed"]), AUTH_1)], what="pipeline")


@pytest.mark.parametrize("path,chunk,small", [("pipeline_chunks", 3000, 0), ("small", 1000, None)])
def test_chunks_and_a_reload_between_two_calls(path, chunk, small):
    """Chunks of 3000 through the pipeline and of 1000 through k_lsmall; AUTH_2 is loaded between two calls and
    takes effect on the next call only."""
    tr = _auth_trace("reload")
    n, mark = len(tr["ed"]), tr["mark"]
    calls = [(a, min(a + chunk, mark), AUTH_1 if a == 0 else None) for a in range(0, mark, chunk)]
    calls += [(a, min(a + chunk, n), AUTH_2 if a == mark else None) for a in range(mark, n, chunk)]
    _form(tr, 3000, small, calls, what=path)


def test_device_entry():
    tr = _auth_trace("plain")
    _form(tr, 1 << 15, 0, [(0, len(tr["ed"]), AUTH_1)], submit=_device, what="device")


def test_arrival_order_lane_counts_entry_node_and_is_not_system_checked():
    tr = _auth_trace("inbound")
    _form(tr, 1 << 15, 0, [(0, len(tr["ed"]), AUTH_1)], system=SYSTEM, what="seq")


# ------------------------------------------------------------------ 2b: the three host lanes in one call
LANES = (2048, 2048, 500)  # events per chunk at max_batch 2048: the pipeline, k_lseq (inbound events), k_lsmall


@functools.lru_cache(maxsize=None)
def _lanes_trace():
    """The mixed workload under AUTH_1 and the blocking SystemRule, one event per step so that the chunk borders
    fall where LANES puts them: no inbound event in the first and the third chunk, every other entry of the second
    inbound.  The second chunk's last 150 events (80 ms, rt <= 39) hold no inbound entry, so no inbound exit is
    left for the third; the exits still due when the stream ends are not part of it.
    tests/test_authority_host.py asserts what each chunk holds."""
    h = ot.OriginTrace(MIX_RES, MIX_ORG, MIX_FLOW, MIX_PARAM, MIX_DEGRADE, system=SYSTEM)
    a = at.AuthorityTrace(h, RES, ORIGINS, AUTH_1)
    rng = np.random.default_rng(31)
    w, ow = np.array([3, 2, 2, 2, 1, 2, 2, 2], float), np.array([2, 3, 2, 1, 1, 0.5])
    ends = np.cumsum(LANES)
    t = T0 + rng.exponential(1.0)
    while len(h.ev) < ends[-1]:
        n, now = len(h.ev), int(t)
        if h.heap and h.heap[0][0] <= now:  # one exit per step
            te, _, rid, o, acq, fl, rt, pv = heapq.heappop(h.heap)
            h.other(1, rid, o, te, acq, fl, rt, pv)
            continue
        rid, o = int(rng.choice(len(w), p=w / w.sum())), int(rng.choice(len(ow), p=ow / ow.sum()))
        hp = rid == 5 and rng.random() < 0.9
        inb = bool(ends[0] <= n < ends[1] - 150 and rng.random() < 0.5)
        a.step(rid, o, now, now, int(rng.integers(1, 3)), int(rng.integers(0, 40)), hp,
               int(rng.integers(0, 6)) if hp else 0, 1 if inb else 0, rng.random() < 0.1)
        t += rng.exponential(1.0)
    h.heap.clear()
    return a.finish(entry=True)


def _run_lanes(hook=None):
    """One host call whose chunks take the pipeline, the arrival-order lane and the small path in turn: what a
    shared prologue or epilogue could leak from one chunk into the next (the overflow word, the dispatch counts,
    the effective kind, the epoch, the sequence numbers) would show in the decisions or the nodes."""
    tr = _lanes_trace()
    eng, s = _sentinel(MIX_RES, MIX_ORG, LANES[0])  # the small limit stays at its default
    _load(s, MIX_FLOW, MIX_PARAM, MIX_DEGRADE, SYSTEM)
    _load_auth(s, AUTH_1)
    got = _submit(s, tr["st"])
    forms = hook() if hook else None
    _same(tr["st"], got, tr["ed"], tr["ew"], "lanes")
    _nodes(s, tr, MIX_RES, MIX_ORG, "lanes")
    eng.close()
    return forms


def lanes_child():
    """Runs in the child process of test_three_lanes_dispatch (the test-only build is loaded)."""
    import ctypes as C

    from sentinel_amd import _lib
    fn = _lib.load().sga_test_local_dispatch  # the product library does not have it
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_uint32), C.c_size_t]

    def hook():
        out = (C.c_uint32 * 12)()
        assert fn(out, 12) == 12
        return [int(x) for x in out]

    print("LANES", json.dumps(_run_lanes(hook)))


def test_three_lanes_in_one_call():
    _run_lanes()


def test_three_lanes_dispatch():
    """The same call under the test-only build: three host chunks since the process began, the last one decided
    by k_lsmall, 500 events."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"import sys; sys.path.insert(0, {root!r}); from tests.test_authority_gpu import lanes_child; lanes_child()"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SGA_LIB_VARIANT="testhooks"),
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    forms = json.loads([x for x in r.stdout.splitlines() if x.startswith("LANES ")][-1][6:])
    assert forms[9:12] == [1, LANES[2], 3], forms


# ------------------------------------------------------------------ 3: edges
def _ev(rows, extra=()):
    """(kind, resource, ts, acquire, flags, rt, param, origin[, context, parent]) per event."""
    cols = ["kind", "resource", "ts", "acquire", "flags", "rt", "param", "origin"] + list(extra)
    dts = {"kind": np.uint8, "resource": np.uint32, "ts": np.int64, "acquire": np.int32, "flags": np.uint8,
           "rt": np.int64, "param": np.uint64, "origin": np.uint32, "context": np.uint32, "parent": np.uint32}
    x = np.array(rows, dtype=np.int64).reshape(-1, len(cols))
    return {c: x[:, i].astype(dts[c]) for i, c in enumerate(cols)}


def _premark(st, resources, origins, rules):
    """The restatement over a hand-written stream: (pre-marked stream, turned positions)."""
    conf = at.load_authority_conf(rules)
    turned = [i for i in range(len(st["kind"])) if st["kind"][i] == 0 and st["resource"][i] < len(resources) and
              not at.check(conf, resources[st["resource"][i]], origins[st["origin"][i] - 1] if st["origin"][i] else "")]
    pre = dict(st, kind=st["kind"].copy())
    pre["kind"][turned] = 2
    return pre, np.array(turned, np.int64)


@pytest.mark.parametrize("small", [None, 0], ids=["small", "pipeline"])
def test_edges_against_the_trace(small):
    """A blocked entry that is the first event ever of its resource and of its pair; a black-listed origin's exit,
    kind 2 and kind 3 events; a blocked prioritized entry with a parameter."""
    flow = [{"resource": 0, "count": 2}, {"resource": 1, "count": 5}]
    rules = [("r0", "o1", BLACK), ("r1", "o2", WHITE), ("r2", "o1,o2", BLACK)]
    h = ot.OriginTrace(3, 3, flow)
    a = at.AuthorityTrace(h, _names(3, "r"), _names(3, "o"), rules)
    t = T0
    assert a.entry(2, 1, t, 3) == (6, 0)               # first event of r2 and of (r2, o1): blocked
    for k in range(4):                                  # o2 on r0: two passes, two flow blocks
        a.entry(0, 2, t + 1 + k, 1)
    assert a.entry(0, 1, t + 6, 2, prio=1, hp=1, pv=7) == (6, 0)   # blocked, prioritized, with a parameter
    h.other(2, 0, 1, t + 7, 1)                          # the black-listed origin's own kind 2 event
    h.other(3, 0, 1, t + 8, 1)                          # and its revoke
    h.other(1, 0, 1, t + 40, 1, 2, 30)                  # and its exit
    assert a.entry(1, 1, t + 41, 1) == (6, 0) and a.entry(1, 2, t + 42, 1)[0] == 0 and a.entry(1, 0, t + 43, 1)[0] == 0
    h.other(1, 0, 2, t + 50, 1, 0, 45)
    tr = a.finish()
    assert len(tr["turned"]) == 3 and (tr["ed"] == 1).sum() == 2 and (2, 1) in tr["onodes"]
    blocked_first = tr["onodes"][(2, 1)][0]
    assert blocked_first[lt.NODE_GETTERS.index("total_block")] == 3
    assert blocked_first[lt.NODE_GETTERS.index("cur_thread_num")] == 0
    out = []
    for auth in (True, False):
        eng, s = _sentinel(3, 3, 1 << 12, small)
        _load(s, flow)
        if auth:
            assert _load_auth(s, rules) == 3
        d, w = _submit(s, tr["st"] if auth else tr["pre"])
        _same(tr["st"], (d, w), tr["ed"] if auth else tr["twin_ed"], tr["ew"], "edges")
        _nodes(s, tr, 3, 3, "edges")  # the same reads in the same order on both: a read rotates windows
        if auth:
            assert [n for n, _ in s.nodes(tr["times"][-1])] == ["r0", "r1", "r2"]  # r2: by its blocked entry alone
            assert tr["nodes"][0][0][lt.NODE_GETTERS.index("waiting")] == 0  # the blocked prioritized entry
            assert tr["nodes"][0][0][lt.NODE_GETTERS.index("occupied_pass_qps")] == 0.0  # occupied nothing
        out.append((d, w, _state(s, tr["times"], 3)))
        eng.close()
    _twin_same(out[0], out[1], tr["turned"], "edges")


EDGE_RES, EDGE_ORG = 6, 3
EDGE_FLOW = [{"resource": 0, "count": 3}, {"resource": 2, "count": 2, "ref": 3}, {"resource": 3, "count": 50},
             {"resource": 4, "count": 1, "limit_app": 2}, {"resource": 4, "count": 4}]
EDGE_PARAM = [{"resource": 1, "count": 2}]
EDGE_AUTH = [("r0", "o1", BLACK), ("r1", "o1,o3", BLACK), ("r2", "o2", WHITE), ("r4", "o1", BLACK),
             ("r5", "o9", WHITE)]


@functools.lru_cache(maxsize=None)
def _edge_stream():
    """r0 plain; r1 parameter-only; r2 RELATE to r3; r4 with a limitApp rule; r5 without rules, white-listed to a
    name nobody registered (every origin but "" fails); resource 99 is no resource.  Entries carry an argument
    vector (SGA_EV_ARGS) or a plain parameter, one in four is prioritized; passed entries of the first half exit."""
    rng = np.random.default_rng(3)
    rows, vals = [], []
    from sentinel_amd.local import encode_args
    for i in range(600):
        rid = int(rng.choice([0, 1, 2, 3, 4, 5, 99]))
        o = int(rng.integers(0, EDGE_ORG + 1))
        fl, pv = 0, 0
        if rid == 1:
            if i % 2:
                fl, pv = 32, encode_args((int(rng.integers(0, 3)),), vals)
            else:
                fl, pv = 4, int(rng.integers(0, 3))
        if i % 4 == 0 and rid != 1:
            fl |= 1
        rows.append((0, rid, T0 + 2 * i, 1 + i % 2, fl, 0, pv, o))
        if i % 3 == 0:
            rows.append((int(rng.choice([1, 2, 3])), rid, T0 + 2 * i + 1, 1, fl & ~1, 5, pv, o))
    st = _ev(rows)
    st["param_values"] = np.array(vals, np.uint64)
    pre, turned = _premark(st, _names(EDGE_RES, "r"), _names(EDGE_ORG, "o"), EDGE_AUTH)
    res_t = st["resource"][turned]
    assert all((res_t == r).sum() >= 10 for r in (0, 1, 2, 4, 5)) and not (res_t == 3).any() and not (res_t == 99).any()
    assert (st["flags"][turned] & 32).sum() >= 5 and (st["flags"][turned] & 1).sum() >= 10
    assert ((st["resource"] == 99) & (st["origin"] == 1) & (st["kind"] == 0)).sum() >= 5
    return st, pre, turned


@pytest.mark.parametrize("small,chunk", [(None, 300), (0, 1 << 12)], ids=["small", "pipeline"])
def test_edges_against_the_twin(small, chunk):
    """Argument vectors and prioritized entries, a parameter-only resource, a RELATE group, a limitApp rule, an
    unknown resource, exits / kind 2 / kind 3 events of black-listed origins: equal to the twin everywhere."""
    st, pre, turned = _edge_stream()
    out = []
    for auth in (True, False):
        eng, s = _sentinel(EDGE_RES, EDGE_ORG, 1 << 12, small)
        _load_flow(s, EDGE_FLOW)
        _load(s, param=EDGE_PARAM)
        if auth:
            assert _load_auth(s, EDGE_AUTH) == 5
            assert s.group_of(2) != 0xFFFFFFFF and s.group_of(4) != 0xFFFFFFFF
        src = st if auth else pre
        gd, gw = [], []
        for lo in range(0, len(src["kind"]), chunk):
            part = lt.slice_stream(src, lo, min(lo + chunk, len(src["kind"])))
            part["param_values"] = src["param_values"]
            d, w = _submit(s, part)
            gd.append(d)
            gw.append(w)
        d, w = np.concatenate(gd), np.concatenate(gw)
        if auth:
            assert (d[turned] == 6).all() and (w[turned] == 0).all() and (d != 6).sum() == len(d) - len(turned)
            assert (d[src["resource"] == 99] == 0).all()
            assert {1, 2} <= set(d.tolist())  # flow and parameter blocks beside the authority ones
        out.append((d, w, _state(s, [T0 + 1300, T0 + 1700, T0 + 3000], EDGE_RES)))
        eng.close()
    _twin_same(out[0], out[1], turned, "edges twin")


@pytest.mark.parametrize("small", [None, 0], ids=["small", "pipeline"])
def test_chain_rule_contexts_and_the_birth_parent_of_a_blocked_entry(small):
    """A sentinel with contexts and tree=True, a CHAIN rule on r1: the DefaultNode a blocked entry creates keeps the
    parent the entry named, counts one block and no thread; the twin agrees on the tree and every node."""
    from sentinel_amd.cluster import Engine
    from sentinel_amd.local import FlowRuleManager, LocalSentinel
    from sentinel_amd.rules import FlowRule
    E = ENTRY
    rows = [(0, 0, T0 + 1, 1, 0, 0, 0, 2, 1, E),    # r0 in c1 from o2: passes
            (0, 1, T0 + 2, 2, 0, 0, 0, 1, 1, 0),    # r1 under r0 from o1: blocked by authority; births (r1, c1) under r0
            (0, 1, T0 + 3, 1, 0, 0, 0, 2, 1, E),    # r1 again, another parent: no new edge; CHAIN rule count 1: passes
            (0, 1, T0 + 4, 1, 0, 0, 0, 2, 1, 0),    # CHAIN rule blocks
            (0, 2, T0 + 5, 1, 0, 0, 0, 1, 2, 1),    # r2 in c2 from o1: not listed, passes
            (1, 0, T0 + 9, 1, 0, 8, 0, 2, 1, E)]
    st = _ev(rows, ("context", "parent"))
    rules = [("r1", "o1", BLACK)]
    pre, turned = _premark(st, _names(3, "r"), _names(2, "o"), rules)
    assert turned.tolist() == [1]
    out = []
    for auth in (True, False):
        eng = Engine(max_batch=1 << 12)
        if small is not None:
            eng.set_small_batch(small)
        s = LocalSentinel(eng, _names(3, "r"), _names(2, "o"), contexts=["c1", "c2"], tree=True)
        FlowRuleManager(s).load_rules([FlowRule(resource="r1", count=1, strategy=2, ref_resource="c1")])
        if auth:
            _load_auth(s, rules)
        d, w = _submit(s, st if auth else pre)
        now = T0 + 20
        if auth:
            assert d.tolist() == [0, 6, 0, 1, 0, 0] and w[1] == 0
            edges = {(int(r["resource"]), int(r["context"])): int(r["parent"]) for r in s.tree_rows(now)}
            assert edges == {(0, 1): E, (1, 1): 0, (2, 2): E}
            v = s.default_node(1, 1, now)
            assert (v.total_block, v.total_pass, v.cur_thread_num) == (3, 1, 1)
            o = s.origin_node(1, 1, now)
            assert (o.total_block, o.total_pass, o.cur_thread_num) == (2, 0, 0)
        out.append((d, w, [s.tree_rows(now).tobytes()] + _state(s, [now, now + 400, now + 1700], 3)))
        eng.close()
    _twin_same(out[0], out[1], turned, "chain")


# ------------------------------------------------------------------ 4: the guard
@pytest.mark.parametrize("case", ["rules_without_an_origin_column", "origin_column_with_rules_cleared"])
def test_guard(case):
    """Rules loaded but no origin column, and an origin column but the rules cleared: what the engine answered
    before it ran the slot."""
    tr = _mix_trace(False)
    eng, s = _sentinel(MIX_RES, MIX_ORG)
    _load(s, MIX_FLOW, MIX_PARAM, MIX_DEGRADE)
    import sentinel_amd.local as local
    origins = case != "rules_without_an_origin_column"
    if hasattr(local, "AuthorityRuleManager"):  # an engine from before the slot has nothing to load or clear
        _load_auth(s, AUTH_1)
        if origins:
            _load_auth(s, [])
    st = tr["st"]
    got = s.submit(st["kind"], st["resource"], st["ts"], st["acquire"], st["flags"], st["rt"], st["param"],
                   origin=st["origin"] if origins else None)
    _same(st, got, tr["ed"], tr["ew"], case)
    _nodes(s, tr if origins else dict(tr, onodes={}), MIX_RES, MIX_ORG, case)
    eng.close()


# ------------------------------------------------------------------ 5: the socket
def test_authority_commands_over_the_socket():
    from sentinel_amd import command_center as cc
    from sentinel_amd.cluster import Engine
    from sentinel_amd.local import AuthorityException, AuthorityRuleManager, FlowRuleManager, LocalSentinel
    from tests.test_command_center_gpu import _get
    eng = Engine(max_batch=1 << 12)
    s = LocalSentinel(eng, ["svc/pay", "svc/user"], ["appA", "appB"])
    center = cc.CommandCenter(s, {"flow": FlowRuleManager(s), "authority": AuthorityRuleManager(s)},
                              clock=lambda: T0 + 100)
    server = cc.SimpleHttpCommandCenter(center, port=18760)
    port = server.start()
    try:
        rules = [{"resource": "svc/pay", "limitApp": "appAB,appB", "strategy": 1},
                 {"resource": "not-registered", "limitApp": "appA", "strategy": 0}]
        post = ("type=authority&data=" + quote(quote(json.dumps(rules)))).encode()
        assert _get(port, "setRules", post=post) == ("HTTP/1.0 200 OK", "success")
        with center.lock:
            s.entry("svc/pay", T0 + 1, origin="appA")          # appA is not contained in "appAB,appB"
            for k in range(3):
                with pytest.raises(AuthorityException):
                    s.entry("svc/pay", T0 + 2 + k, 2, origin="appB")
            s.entry("svc/user", T0 + 6, origin="appB")
        assert json.loads(_get(port, "getRules?type=authority")[1]) == \
            [{"limitApp": "appAB,appB", "resource": "svc/pay", "strategy": 1},
             {"limitApp": "appA", "resource": "not-registered", "strategy": 0}]
        with center.lock:
            views = [(n, s.node(n, T0 + 100)) for n in ("svc/pay", "svc/user")]
        assert (views[0][1].total_block, views[0][1].total_pass, views[1][1].total_block) == (6, 1, 0)
        assert _get(port, "cnode?id=svc")[1] == cc.format_cnode(views)
        assert _get(port, "origin?id=svc/pay")[1].count("\n") == 5  # both origins have a node
    finally:
        server.stop()
        eng.close()
