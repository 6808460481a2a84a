"""GPU parity of the invocation tree: events submitted with a parent array (sga_submit_events_tree*) record each
DefaultNode's parent at its creation (NodeSelectorSlot.java:158-177: addChild once, when the node is made), and
sga_query_tree answers the DefaultNodes with their resolved edges; EntranceNode and Constants.ROOT values are the
host's sums over those rows (EntranceNode.java:45-126).

Bar: edges equal tests/tree_trace.py's restatement; decisions, waits and every row's view bit-identical to the
context-shadow oracle at three query times; EntranceNode and ROOT views equal the helper's, field by field (both
sides sum bit-equal inputs in the same stated order).  The birth pass is tested where it can go wrong: first events
at the wave and workgroup seams of one chunk, a second chunk that names another parent, refused chunks."""
import json

import numpy as np
import pytest

from tests import local_trace as lt
from tests import tree_trace as tt

pytestmark = pytest.mark.gpu

T0 = tt.T0
ENT = tt.ENTRANCE
ENOMEM, EINVAL = "rc=-12", "rc=-22"
KT = 256  # the claim and birth passes' workgroup (flow.hip kT)


# ------------------------------------------------------------------ engine side
def _sentinel(n_res, n_origins, n_contexts, max_batch=1 << 12, small=0, max_cnodes=0, max_onodes=0, tree=True):
    from sentinel_amd.cluster import Engine
    from sentinel_amd.local import LocalSentinel
    eng = Engine(max_batch=max_batch)
    if small is not None:
        eng.set_small_batch(small)
    return eng, LocalSentinel(eng, [f"r{i}" for i in range(n_res)], [f"o{i + 1}" for i in range(n_origins)] or None,
                              max_origin_nodes=max_onodes, contexts=[f"c{i + 1}" for i in range(n_contexts)],
                              max_context_nodes=max_cnodes, tree=tree)


def _submit(s, st, parent=True):
    return s.submit(st["kind"], st["resource"], st["ts"], st["acquire"], st["flags"], st["rt"], st["param"],
                    origin=st["origin"] if s.origins else None, context=st["context"],
                    parent=st["parent"] if parent else None)


def _device(s, st):
    """One chunk through submit_device with the context and parent columns; status not read."""
    import torch
    dev = torch.device("cuda", 0)
    base = int(st["ts"].min())
    off = (st["ts"] - base).astype(np.uint32).view(np.int32)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)  # noqa: E731
    return s.submit_device(t(st["kind"], np.uint8), t(st["resource"], np.int32), base, t(off, np.int32),
                           t(st["acquire"], np.int32), flags=t(st["flags"], np.uint8), rt=t(st["rt"], np.int64),
                           param=t(st["param"], np.int64), origin=t(st["origin"], np.int32) if s.origins else None,
                           context=t(st["context"], np.int32), parent=t(st["parent"], np.int32))


def _ev(rows):
    """(kind, resource, ts, acquire, flags, rt, origin, context, parent) per event."""
    x = np.array(rows, dtype=np.int64).reshape(-1, 9)
    return {"kind": x[:, 0].astype(np.uint8), "resource": x[:, 1].astype(np.uint32), "ts": x[:, 2].copy(),
            "acquire": x[:, 3].astype(np.int32), "flags": x[:, 4].astype(np.uint8), "rt": x[:, 5].copy(),
            "param": np.zeros(len(x), dtype=np.uint64), "origin": x[:, 6].astype(np.uint32),
            "context": x[:, 7].astype(np.uint32), "parent": x[:, 8].astype(np.uint32)}


def _entry(rid, t, c, p, o=0):
    return (0, rid, T0 + t, 1, 0, 0, o, c, p)


def _edges(rows):
    return {(int(r["resource"]), int(r["context"])): int(r["parent"]) for r in rows}


def _views(rows):
    return {(int(r["resource"]), int(r["context"])): [r[g].item() for g in lt.NODE_GETTERS] for r in rows}


def _same_tree(got, exp, what):
    """A TreeNode against the helper's (name, getters, entrance, children)."""
    name, getters, entrance, kids = exp
    assert (got.name, got.entrance) == (name, entrance), (what, got.name, name)
    mine = [getattr(got.view, g) for g in lt.NODE_GETTERS]
    assert mine == getters, (what, name, [x for x in zip(lt.NODE_GETTERS, mine, getters) if x[1] != x[2]])
    assert [k.name for k in got.children] == [k[0] for k in kids], (what, name)
    for g, e in zip(got.children, kids):
        _same_tree(g, e, what + "/" + name)


def _same(got, ed, ew, what):
    gd, gw = got
    bad = np.nonzero((gd != ed) | (gw != ew))[0]
    assert not len(bad), (what, len(bad), int(bad[0]), gd[bad[0]], gw[bad[0]], ed[bad[0]], ew[bad[0]])


def _refused(s, entry, st, rc):
    from sentinel_amd._lib import EngineError
    if entry == "device":
        d, _ = _device(s, st)
        with pytest.raises(EngineError, match=rc):
            s.device_status()
        assert (d.cpu().numpy() == -1).all()
    else:
        with pytest.raises(EngineError, match=rc):
            _submit(s, st)


def _state(s, now):
    """Everything a chunk can change that a query shows: the tree's rows and every ClusterNode and origin node."""
    from sentinel_amd import _lib
    every = list(range(len(s.resources)))
    return (s.tree_rows(now).tobytes(), s.query_nodes(_lib.SGA_NODES_RESOURCE, now, every).tobytes(),
            s.query_nodes(_lib.SGA_NODES_ORIGIN, now).tobytes())


ENTRIES = [("host", 0), ("small", None), ("device", 0)]


# ------------------------------------------------------------------ 1: the hand case
@pytest.mark.parametrize("small", [0, None], ids=["pipeline", "small"])
def test_hand_case(small):
    tr = tt.hand_trace()
    eng, s = _sentinel(3, 0, 2, small=small)
    _same(_submit(s, tr["st"]), tr["ed"], tr["ew"], "hand")
    now = tr["times"][0]
    rows = s.tree_rows(now)
    assert [(int(r["context"]), int(r["resource"])) for r in rows] == [(1, 0), (1, 1), (1, 2), (2, 1)]  # sorted
    assert _edges(rows) == {(0, 1): ENT, (1, 1): 0, (2, 1): 1, (1, 2): ENT} == tr["edges"]
    assert _views(rows) == {p: v[0] for p, v in tr["cnodes"].items()}
    for r in rows:  # the row's view is sga_query_context_node's
        v = s.default_node(int(r["resource"]), int(r["context"]), now)
        assert [getattr(v, g) for g in lt.NODE_GETTERS] == [r[g].item() for g in lt.NODE_GETTERS]
    tree = s.invocation_tree(now)
    _same_tree(tree, tr["trees"][0], "hand")
    c1, c2 = tree.children
    assert (c1.view.pass_qps, c1.view.avg_rt, c2.view.avg_rt, tree.view.pass_qps, tree.view.avg_rt) == \
        (1.0, 10.0, 30.0, 2.0, 20.0)
    eng.close()


def test_single_entries_carry_their_parent():
    """LocalSentinel.entry(parent=): the enclosing Entry's resource is the parent; the Entry keeps it."""
    eng, s = _sentinel(3, 0, 1, small=None)
    a = s.entry("r0", T0 + 1, context="c1")
    b = s.entry("r1", T0 + 2, context="c1", parent=a)
    c = s.entry("r2", T0 + 3, context="c1", parent=b)
    s.entry("r1", T0 + 4, context="c1", parent=c)
    assert c.parent is b and b.parent is a and a.parent is None
    c.exit(T0 + 5)
    assert _edges(s.tree_rows(T0 + 6)) == {(0, 1): ENT, (1, 1): 0, (2, 1): 1}
    eng.close()


# ------------------------------------------------------------------ 2: births inside one chunk
FIRST = [0, 63, 64, KT - 1, KT, 4 * KT]     # where the six pairs' first events sit: wave and workgroup seams
BIRTH_PARENT = [7, 0, 1, 2, 0, 4]           # their parents: (7, c1) exists before the chunk, the others by then
N_CHUNK = 4 * KT + 1


def _birth_chunk():
    """One chunk of 4 kT + 1 entries in context c1, no rules.  Pair (k, c1) is created by event FIRST[k] under
    BIRTH_PARENT[k]; every other event re-enters a pair already created, chosen round-robin, under another parent
    (the EntranceNode, or r7 where r7 is not the birth parent) -- so each pair's later events lie in other waves
    and workgroups than its first, except the pair created by the chunk's last event, which has none."""
    rows, born = [], 0
    for i in range(N_CHUNK):
        if born < len(FIRST) and i == FIRST[born]:
            rows.append(_entry(born, 10 + i // 16, 1, BIRTH_PARENT[born]))
            born += 1
        else:
            k = i % born
            rows.append(_entry(k, 10 + i // 16, 1, ENT if (BIRTH_PARENT[k] == 7 or i % 2) else 7))
    st = _ev(rows)
    for k, f in enumerate(FIRST):
        mine = np.nonzero(st["resource"] == k)[0]
        assert mine[0] == f and (k == 5 or ((mine[1:] // 64 != f // 64).any() and (mine[1:] // KT != f // KT).any()))
        assert (st["parent"][mine[1:]] != BIRTH_PARENT[k]).all()
    return st


BIRTH_EDGES = {(7, 1): ENT, (0, 1): 7, (1, 1): 0, (2, 1): 1, (3, 1): 2, (4, 1): 0, (5, 1): 4}


@pytest.mark.parametrize("entry", ["host", "device"])
def test_birth_inside_one_chunk(entry):
    """The first event's parent wins for each pair, wherever the event sits in the grid; the device entry gives
    the host entry's rows."""
    st = _birth_chunk()
    eng, s = _sentinel(8, 0, 1, max_batch=1 << 11)
    assert list(_submit(s, _ev([_entry(7, 0, 1, ENT)]))[0]) == [0]
    if entry == "device":
        d, _ = _device(s, st)
        s.device_status()
        assert (d.cpu().numpy() == 0).all()
    else:
        assert (_submit(s, st)[0] == 0).all()
    rows = s.tree_rows(T0 + 200)
    assert _edges(rows) == BIRTH_EDGES
    counts = {k: int((st["resource"] == k).sum()) for k in range(6)}
    assert {(int(r["resource"]), int(r["total_pass"])) for r in rows} == {(7, 1)} | set(counts.items())
    eng.close()


# ------------------------------------------------------------------ 3: across chunks
@pytest.mark.parametrize("small", [0, None], ids=["pipeline", "small"])
def test_a_later_chunk_does_not_move_the_edge(small):
    """max_batch 4096: one call of 4096 + 64 events is two chunks (the second one the small path's when that is
    on).  (2, c1) is created in the first under r0; the second enters it under r1 and under the EntranceNode, and
    creates (3, c1) under r1."""
    cap = 1 << 12
    rows = [_entry(0, 1, 1, ENT), _entry(1, 1, 1, 0), _entry(2, 1, 1, 0)]
    rows += [_entry(0, 1 + i // 64, 1, ENT) for i in range(3, cap)]
    rows += [_entry(2, 70, 1, 1), _entry(2, 71, 1, ENT), _entry(3, 72, 1, 1)] + [_entry(2, 73, 1, 1) for i in range(61)]
    assert len(rows) == cap + 64
    eng, s = _sentinel(4, 0, 1, max_batch=cap, small=small)
    assert (_submit(s, _ev(rows))[0] == 0).all()
    assert _edges(s.tree_rows(T0 + 200)) == {(0, 1): ENT, (1, 1): 0, (2, 1): 0, (3, 1): 1}
    eng.close()


# ------------------------------------------------------------------ 4: refusals
@pytest.mark.parametrize("entry,small", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_chunk_refused_for_a_context_id_leaves_no_edge(entry, small):
    eng, s = _sentinel(4, 0, 2, small=small)
    _submit(s, _ev([_entry(0, 1, 1, ENT), _entry(2, 2, 1, 0)]))
    before = _state(s, T0 + 50)
    bad = _ev([_entry(1, 3, 1, 0), _entry(3, 4, 2, ENT), _entry(0, 5, 3, ENT)])   # context 3 of 2
    _refused(s, entry, bad, EINVAL)
    assert _state(s, T0 + 50) == before and s.default_node(1, 1, T0 + 50) is None
    # the pair is created by a later chunk, under that chunk's parent
    assert list(_submit(s, _ev([_entry(1, 6, 1, 2), _entry(1, 7, 1, 0)]))[0]) == [0, 0]
    assert _edges(s.tree_rows(T0 + 50)) == {(0, 1): ENT, (2, 1): 0, (1, 1): 2}
    eng.close()


@pytest.mark.parametrize("entry,small", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_chunk_refused_for_a_full_table_leaves_no_edge(entry, small):
    """The origin table holds one record: a chunk that needs a second is refused (SGA_ENOMEM) after the context
    table has handed (1, c1) its record; the claim is taken back, and with it the birth."""
    eng, s = _sentinel(4, 2, 1, small=small, max_onodes=1)
    _submit(s, _ev([_entry(0, 1, 1, ENT, o=1), _entry(2, 2, 1, 0)]))
    before = _state(s, T0 + 50)
    _refused(s, entry, _ev([_entry(1, 3, 1, 0, o=2)]), ENOMEM)
    assert _state(s, T0 + 50) == before and s.default_node(1, 1, T0 + 50) is None
    assert list(_submit(s, _ev([_entry(1, 6, 1, 2), _entry(1, 7, 1, 0)]))[0]) == [0, 0]
    assert _edges(s.tree_rows(T0 + 50)) == {(0, 1): ENT, (2, 1): 0, (1, 1): 2}
    eng.close()


@pytest.mark.parametrize("entry,small", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_bad_parent_refuses_the_chunk(entry, small):
    """A parent equal to n_resources on an event that may create a DefaultNode: SGA_EINVAL, nothing applied.  On
    an exit, or on an event without a context, the parent is not read."""
    n_res = 4
    eng, s = _sentinel(n_res, 1, 1, small=small)
    _submit(s, _ev([_entry(0, 1, 1, ENT, o=1), _entry(2, 2, 1, 0)]))
    before = _state(s, T0 + 50)
    bad = _ev([_entry(1, 3, 1, 0, o=1), _entry(3, 4, 1, n_res), _entry(0, 5, 1, ENT)])
    _refused(s, entry, bad, EINVAL)
    assert _state(s, T0 + 50) == before and s.default_node(1, 1, T0 + 50) is None
    ok = _ev([(1, 0, T0 + 6, 1, 0, 5, 1, 1, n_res), _entry(3, 7, 0, n_res), _entry(1, 8, 1, 2)])
    assert list(_submit(s, ok)[0]) == [0, 0, 0]
    assert _edges(s.tree_rows(T0 + 50)) == {(0, 1): ENT, (2, 1): 0, (1, 1): 2}
    eng.close()


# ------------------------------------------------------------------ 5: resolution
@pytest.mark.parametrize("small", [0, None], ids=["pipeline", "small"])
def test_edges_that_resolve_to_the_entrance_node(small):
    eng, s = _sentinel(6, 0, 2, small=small)
    st = _ev([_entry(5, 1, 2, ENT),     # r5 has a DefaultNode in c2 only
              _entry(0, 2, 1, 5),       # a parent without a DefaultNode in c1
              _entry(1, 3, 1, 1),       # a self-parent
              _entry(2, 4, 1, 3),       # a parent born later
              _entry(3, 5, 1, ENT),
              _entry(4, 6, 1, 3)])      # born after its parent: the edge stands
    assert (_submit(s, st)[0] == 0).all()
    assert _edges(s.tree_rows(T0 + 50)) == {(5, 2): ENT, (0, 1): ENT, (1, 1): ENT, (2, 1): ENT, (3, 1): ENT, (4, 1): 3}
    tree = s.invocation_tree(T0 + 50)
    assert [(c.name, [k.name for k in c.children]) for c in tree.children] == \
        [("c1", ["r0", "r1", "r2", "r3"]), ("c2", ["r5"])]
    assert [k.name for k in tree.children[0].children[3].children] == ["r4"]
    eng.close()


def test_query_tree_capacity_and_no_contexts():
    import ctypes as C
    from sentinel_amd import _lib
    from sentinel_amd.cluster import Engine
    from sentinel_amd.local import TREE_ROW_DTYPE, LocalSentinel
    eng, s = _sentinel(3, 0, 1)
    _submit(s, _ev([_entry(0, 1, 1, ENT), _entry(1, 2, 1, 0), _entry(2, 3, 1, 1)]))
    out, n = np.zeros(2, dtype=TREE_ROW_DTYPE), C.c_size_t()
    assert _lib.load().sga_query_tree(eng.handle, T0 + 9, out.ctypes.data, 2, C.byref(n)) == _lib.SGA_ERANGE
    assert n.value == 3
    eng.close()
    eng = Engine(max_batch=1 << 12)
    LocalSentinel(eng, ["r0"])
    assert _lib.load().sga_query_tree(eng.handle, T0, out.ctypes.data, 2, C.byref(n)) == 0 and n.value == 0
    eng.close()


# ------------------------------------------------------------------ 6: the parity trace
def _load_flow(s, rules):
    from tests.test_context_gpu import _load_flow as load
    return load(s, rules)


def _parity_engine(parent=True, chunk=3000):
    tr = tt.parity_trace()
    st = tr["st"]
    eng, s = _sentinel(tt.PARITY_RES, tt.PARITY_ORG, tt.PARITY_CTX, max_batch=1 << 12)
    assert _load_flow(s, tt.PARITY_FLOW) == len(tt.PARITY_FLOW)
    gd, gw = [], []
    for a in range(0, len(tr["ed"]), chunk):
        d, w = _submit(s, lt.slice_stream(st, a, min(a + chunk, len(tr["ed"]))), parent)
        gd.append(d)
        gw.append(w)
    return tr, eng, s, (np.concatenate(gd), np.concatenate(gw))


def test_parity_with_the_oracle():
    tr, eng, s, got = _parity_engine()
    _same(got, tr["ed"], tr["ew"], "parity")
    for k, now in enumerate(tr["times"]):
        rows = s.tree_rows(now)
        assert _views(rows) == {p: v[k] for p, v in tr["cnodes"].items()}, (k, now)
        assert _edges(rows) == tr["edges"], (k, now)
        _same_tree(s.invocation_tree(now), tr["trees"][k], f"t{k}")
    eng.close()


def test_no_parent_array_hangs_every_node_under_its_entrance_node():
    """The same stream through sga_submit_events_ctx: same decisions and waits, same views on every node of the
    three tables, every edge to the EntranceNode."""
    tr, eng, s, got = _parity_engine()
    tr, eng2, s2, got2 = _parity_engine(parent=False)
    assert (got[0] == got2[0]).all() and (got[1] == got2[1]).all()
    now = tr["times"][0]
    a, b = s.tree_rows(now), s2.tree_rows(now)
    assert (b["parent"] == ENT).all() and (a["parent"] != ENT).any()
    b["parent"] = a["parent"]
    assert a.tobytes() == b.tobytes()
    assert _state(s, now)[1:] == _state(s2, now)[1:]
    tree = s2.invocation_tree(now)
    assert all(not k.children for c in tree.children for k in c.children)
    eng.close()
    eng2.close()


# ------------------------------------------------------------------ 7: over a socket
def _tree_node(exp):
    from sentinel_amd.local import NodeView, TreeNode
    name, getters, entrance, kids = exp
    return TreeNode(name, NodeView(*getters), entrance, [_tree_node(k) for k in kids])


def test_tree_commands_over_the_socket():
    from sentinel_amd import command_center as cc
    from tests.test_command_center_gpu import _get
    tr, eng, s, _ = _parity_engine()
    now = tr["times"][0]
    want = _tree_node(tr["trees"][0])
    center = cc.CommandCenter(s, {}, clock=lambda: now)
    server = cc.SimpleHttpCommandCenter(center, port=18760)
    port = server.start()
    try:
        assert _get(port, "tree") == ("HTTP/1.0 200 OK", cc.format_tree(want))
        assert _get(port, "tree?id=c2") == ("HTTP/1.0 200 OK", cc.format_tree(want, "c2"))
        sub = cc.format_tree(want, "c")     # no context is named "c": every one that contains it
        assert sub.count("EntranceNode: ") == tt.PARITY_CTX and _get(port, "tree?id=c") == ("HTTP/1.0 200 OK", sub)
        ids = iter(f"n{k}" for k in range(1000))
        center.new_id = lambda: next(ids)
        exp = iter(f"n{k}" for k in range(1000))
        status, body = _get(port, "jsonTree")
        assert (status, body) == ("HTTP/1.0 200 OK", cc.to_json(cc.tree_node_vos(want, now, lambda: next(exp))))
        vos = json.loads(body)
        assert len(vos) == 1 + tt.PARITY_CTX + len(tr["edges"]) and "parentId" not in vos[0]
        api = json.loads(_get(port, "api")[1])
        assert len(api) == 13
    finally:
        server.stop()
    eng.close()
