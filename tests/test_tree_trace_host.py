"""The invocation tree without a GPU: the helper the GPU tests take their expected values from
(tests/tree_trace.py) against a case computed by hand, the properties the fixed-seed parity trace must have, and
the two texts (FetchTreeCommandHandler, FetchJsonTreeCommandHandler) against strings worked out from the Java
format strings over fabricated trees."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from sentinel_amd import command_center as cc
from sentinel_amd.local import ROOT_NAME, NodeView, TreeNode, entrance_view
from tests import local_trace as lt
from tests import tree_trace as tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENT = tt.ENTRANCE
A, B, C_ = tt.A, tt.B, tt.C_


def _g(getters, *names):
    return tuple(getters[tt.G[n]] for n in names)


# ------------------------------------------------------------------ the ABI
SYMBOLS = ["sga_submit_events_tree", "sga_submit_events_tree_device", "sga_query_tree"]


def test_header_mirror_and_library_declare_the_tree_entry_points():
    """Entry points and one constant only: no struct changed, the ABI version stays.  Loading the library needs
    no GPU."""
    from sentinel_amd import _lib
    from sentinel_amd.local import TREE_ROW_DTYPE
    with open(os.path.join(ROOT, "include", "sentinel_amd.h")) as f:
        h = f.read()
    lib = _lib.load()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", h), s
        assert s in _lib.SIGNATURES and getattr(lib, s) is not None, s
    m = re.search(r"#define\s+SGA_PARENT_ENTRANCE\s+(0x[0-9A-Fa-f]+)u", h)
    assert m and int(m.group(1), 0) == 0xFFFFFFFF == _lib.SGA_PARENT_ENTRANCE == ENT
    assert re.search(r"#define\s+SGA_ABI_VERSION\s+3\b", h) and lib.sga_abi_version() == 3
    # the parent array sits after the context array: one argument more than the _ctx entries
    for a, b in (("sga_submit_events_tree", "sga_submit_events_ctx"),
                 ("sga_submit_events_tree_device", "sga_submit_events_ctx_device")):
        assert len(_lib.SIGNATURES[a][1]) == len(_lib.SIGNATURES[b][1]) + 1
    # sga_tree_row: four ids, then the view -- the layout of a sga_node_row
    assert C.sizeof(_lib.SgaTreeRow) == TREE_ROW_DTYPE.itemsize == C.sizeof(_lib.SgaNodeRow) == 144
    assert TREE_ROW_DTYPE.names[:4] == ("resource", "context", "parent", "reserved")
    assert TREE_ROW_DTYPE.fields["pass_qps"][1] == _lib.SgaTreeRow.view.offset == 16


def test_parent_needs_a_tree_sentinel():
    """LocalSentinel refuses `parent` unless it was created with tree=True (checked before any engine call)."""
    from sentinel_amd.local import LocalSentinel
    s = LocalSentinel.__new__(LocalSentinel)
    s.tree = False
    with pytest.raises(ValueError, match="tree=True"):
        s.submit([0], [0], [0], [1], context=[1], parent=[ENT])
    with pytest.raises(ValueError, match="tree=True"):
        s.tree_rows(0)
    s.tree = True
    with pytest.raises(ValueError, match="context array"):
        s.submit([0], [0], [0], [1], parent=[ENT])


# ------------------------------------------------------------------ the helper
def test_hand_case_edges_and_sums():
    tr = tt.hand_trace()
    assert list(tr["ed"]) == [0] * 7
    assert list(tr["st"]["parent"]) == [ENT, A, B, C_, ENT, ENT, ENT]
    assert tr["births"] == {(A, 1): (0, ENT), (B, 1): (1, A), (C_, 1): (2, B), (B, 2): (4, ENT)}
    assert tr["edges"] == {(A, 1): ENT, (B, 1): A, (C_, 1): B, (B, 2): ENT}
    assert tr["reparented"] == {(B, 1)}                       # B under C: entered again, no edge
    assert [tt.depth_of(tr["edges"], c) for c in (1, 2)] == [3, 1]
    # at T0 + 40 every event is inside the second window: (passQps, successQps, avgRt, threads, totalPass)
    want = {(A, 1): (1.0, 1.0, 10.0, 0, 1), (B, 1): (2.0, 0.0, 0.0, 2, 2), (C_, 1): (1.0, 0.0, 0.0, 1, 1),
            (B, 2): (1.0, 1.0, 30.0, 0, 1)}
    views = {p: v[0] for p, v in tr["cnodes"].items()}
    for pair, exp in want.items():
        assert _g(views[pair], "pass_qps", "success_qps", "avg_rt", "cur_thread_num", "total_pass") == exp, pair
    root = tr["trees"][0]
    assert root[0] == tt.ROOT_NAME and root[2] and [c[0] for c in root[3]] == ["c1", "c2"]
    c1, c2 = root[3]
    # c1's only child is A (B and C hang below it): the EntranceNode sums direct children only
    assert [k[0] for k in c1[3]] == ["r0"] and [k[0] for k in c1[3][0][3]] == ["r1"]
    assert [k[0] for k in c1[3][0][3][0][3]] == ["r2"] and c1[3][0][3][0][3][0][3] == []
    assert [k[0] for k in c2[3]] == ["r1"] and c2[3][0][3] == []
    names = ("pass_qps", "block_qps", "success_qps", "avg_rt", "cur_thread_num", "total_pass", "total_block")
    assert _g(c1[1], *names) == (1.0, 0.0, 1.0, 10.0, 0, 1, 0)
    assert _g(c2[1], *names) == (1.0, 0.0, 1.0, 30.0, 0, 1, 0)
    assert _g(root[1], *names) == (2.0, 0.0, 2.0, (10.0 * 1.0 + 30.0 * 1.0) / 2.0, 0, 2, 0)
    # the getters EntranceNode does not override read a StatisticNode nothing adds to
    assert _g(c1[1], "exception_qps", "total_exception", "total_success", "min_rt", "max_success_qps", "waiting",
              "occupied_pass_qps", "previous_pass_qps", "previous_block_qps") == \
        (0.0, 0, 0, 5000.0, 2.0, 0, 0.0, 0.0, 0.0)


def test_resolution_rule():
    """A parent without a node, a self-parent and a parent born later fall to the EntranceNode; a parent born
    earlier in another context does not count."""
    births = {(0, 1): (5, 3), (1, 1): (6, 1), (2, 1): (7, 4), (4, 1): (9, ENT), (5, 1): (10, 4), (4, 2): (1, ENT),
              (6, 2): (2, 5)}
    assert tt.resolve(births) == {(0, 1): ENT, (1, 1): ENT, (2, 1): ENT, (4, 1): ENT, (5, 1): 4, (4, 2): ENT,
                                  (6, 2): ENT}


def test_entrance_getters_without_passing_children_divide_by_one():
    kid = [0.0] * len(lt.NODE_GETTERS)
    kid[tt.G["avg_rt"]], kid[tt.G["block_qps"]] = 7.0, 3.0
    got = tt.entrance_getters([kid, kid])
    assert _g(got, "avg_rt", "pass_qps", "block_qps") == (0.0, 0.0, 6.0)
    assert _g(tt.entrance_getters([]), "avg_rt", "pass_qps", "min_rt") == (0.0, 0.0, 5000.0)


def test_host_entrance_view_is_the_helpers_restatement():
    """sentinel_amd.local.entrance_view against the helper's independent restatement, field by field, on views
    whose products do not sum exactly in another order."""
    kids = [NodeView(3.0, 1.0, 2.0, 0.5, 0.0, 0.1, 1.0, 0.0, 30, 4, 20, 1, 2, 0, 4.0, 0.0),
            NodeView(7.0, 0.0, 6.0, 0.0, 0.0, 0.7, 1.0, 0.0, 70, 0, 60, 0, 1, 0, 8.0, 0.0),
            NodeView(11.0, 2.0, 9.0, 0.0, 0.0, 1.3, 1.0, 0.0, 110, 9, 90, 2, 5, 0, 6.0, 0.0)]
    got = entrance_view(kids, 5000)
    want = tt.entrance_getters([[getattr(k, g) for g in lt.NODE_GETTERS] for k in kids])
    assert [getattr(got, g) for g in lt.NODE_GETTERS] == want
    assert got.avg_rt == ((0.0 + 0.1 * 3.0) + 0.7 * 7.0 + 1.3 * 11.0) / ((0.0 + 3.0) + 7.0 + 11.0)


def test_parity_trace_coverage_conditions():
    """The fixed-seed trace the GPU parity test replays (seed picked here, with the oracles alone)."""
    tr = tt.parity_trace()
    for name, holds in tt.coverage(tr):
        assert holds, name
    st = tr["st"]
    assert 19000 <= len(tr["ed"]) <= 23000 and len(tr["cnodes"]) == tt.PARITY_RES * tt.PARITY_CTX
    assert (st["origin"] != 0).sum() > 5000 and (st["context"] == 0).sum() > 1000
    assert (np.diff(st["ts"]) < 0).sum() > 50                      # timestamps that decrease
    nested = (st["parent"] != ENT) & (st["kind"] == 0)
    assert nested.sum() > 3000 and ((st["parent"] == ENT) & (st["kind"] == 0) & (st["context"] != 0)).sum() > 1000
    d = tr["ed"][st["kind"] == 0]
    assert (d == 0).sum() > 1000 and (d == 1).sum() > 1000
    assert any(p != ENT for p in tr["edges"].values()) and any(p == ENT for p in tr["edges"].values())


# ------------------------------------------------------------------ the texts
def _view(pass_qps=0.0, block_qps=0.0, success_qps=0.0, avg_rt=0.0, total_pass=0, total_block=0, threads=0,
          exception_qps=0.0, total_exception=0):
    return NodeView(pass_qps, block_qps, success_qps, exception_qps, 0.0, avg_rt, 1.0, 0.0, total_pass, total_block, 0,
                    total_exception, threads, 0, 2.0, 0.0)


def _fabricated():
    """ROOT -> web (a -> b, c), web-admin (a), job (nothing passing)."""
    b = TreeNode("b", _view(1.0, 0.0, 1.0, 2.5, 10, 0, 1), False, [])
    a = TreeNode("a", _view(1.0E7, 3.0, 9999999.0, 0.25, 12345678, 3, 2, 1.0, 4), False, [b])
    c = TreeNode("c", _view(0.0, 2.0, 0.0, 0.0, 0, 2, 0), False, [])
    web = TreeNode("web", entrance_view([a.view, c.view], 5000), True, [a, c])
    a2 = TreeNode("a", _view(4.0, 0.0, 4.0, 1.5, 4, 0, 0), False, [])
    admin = TreeNode("web-admin", entrance_view([a2.view], 5000), True, [a2])
    job = TreeNode("job", entrance_view([], 5000), True, [])
    kids = [web, admin, job]
    return TreeNode(ROOT_NAME, entrance_view([k.view for k in kids], 5000), True, kids)


LEGEND = ("\r\n\r\nt:threadNum  pq:passQps  bq:blockQps  tq:totalQps  rt:averageRt  prq: passRequestQps 1mp:1m-pass "
          "1mb:1m-block 1mt:1m-total\r\n")
WEB = ("EntranceNode: web(t:2 pq:1.0E7 bq:5.0 tq:1.0000005E7 rt:0.25 prq:9999999.0 1mp:12345678 1mb:5 1mt:12345683)\n",
       "a(t:2 pq:1.0E7 bq:3.0 tq:1.0000003E7 rt:0.25 prq:9999999.0 1mp:12345678 1mb:3 1mt:12345681)\n",
       "b(t:1 pq:1.0 bq:0.0 tq:1.0 rt:2.5 prq:1.0 1mp:10 1mb:0 1mt:10)\n",
       "c(t:0 pq:0.0 bq:2.0 tq:2.0 rt:0.0 prq:0.0 1mp:0 1mb:2 1mt:2)\n")
ADMIN = ("EntranceNode: web-admin(t:0 pq:4.0 bq:0.0 tq:4.0 rt:1.5 prq:4.0 1mp:4 1mb:0 1mt:4)\n",
         "a(t:0 pq:4.0 bq:0.0 tq:4.0 rt:1.5 prq:4.0 1mp:4 1mb:0 1mt:4)\n")
JOB = "EntranceNode: job(t:0 pq:0.0 bq:0.0 tq:0.0 rt:0.0 prq:0.0 1mp:0 1mb:0 1mt:0)\n"


def _walk(level, lines):
    """A subtree's lines with their dashes: lines[0] at `level`, the given nesting below."""
    return "".join("-" * (level + d) + ln for d, ln in lines)


def test_format_tree():
    tree = _fabricated()
    # rt of ROOT: (0.25 * 1.0E7 + 1.5 * 4.0 + 0.0 * 0.0) / (1.0E7 + 4.0 + 0.0), as Double.toString prints it
    root_rt = (0.25 * 1.0E7 + 1.5 * 4.0) / (1.0E7 + 4.0)
    root = ("EntranceNode: machine-root(t:2 pq:1.0000004E7 bq:5.0 tq:1.0000009E7 rt:%s prq:1.0000003E7 "
            "1mp:12345682 1mb:5 1mt:12345687)\n" % cc.double_to_string(root_rt))
    web = [(0, WEB[0]), (1, WEB[1]), (2, WEB[2]), (1, WEB[3])]
    admin = [(0, ADMIN[0]), (1, ADMIN[1])]
    assert cc.format_tree(tree) == root + _walk(1, web) + _walk(1, admin) + "-" + JOB + LEGEND
    assert cc.format_tree(tree, "web") == _walk(0, web) + LEGEND                  # equals: that child alone
    assert cc.format_tree(tree, "web-admin") == _walk(0, admin) + LEGEND
    assert cc.format_tree(tree, "eb") == _walk(0, web) + _walk(0, admin) + LEGEND   # none equals: every one containing
    assert cc.format_tree(tree, "o") == JOB + LEGEND
    assert cc.format_tree(tree, "nobody") == LEGEND                               # the legend always ends the body
    assert cc.format_tree(tree, "machine-root") == LEGEND                         # id names ROOT's children only
    assert cc.format_tree(TreeNode(ROOT_NAME, entrance_view([], 5000), True, [])) == \
        "EntranceNode: machine-root(t:0 pq:0.0 bq:0.0 tq:0.0 rt:0.0 prq:0.0 1mp:0 1mb:0 1mt:0)\n" + LEGEND


def test_tree_node_vos():
    tree = _fabricated()
    ids = iter(f"id-{k}" for k in range(100))
    vos = cc.tree_node_vos(tree, 1234, lambda: next(ids))
    assert [v["resource"] for v in vos] == [ROOT_NAME, "web", "a", "b", "c", "web-admin", "a", "job"]   # preorder
    assert [v["id"] for v in vos] == [f"id-{k}" for k in range(8)]
    keys = ["averageRt", "blockQps", "exceptionQps", "id", "oneMinuteBlock", "oneMinuteException", "oneMinutePass",
            "oneMinuteTotal", "parentId", "passQps", "resource", "successQps", "threadNum", "timestamp", "totalQps"]
    assert list(vos[0]) == [k for k in keys if k != "parentId"]          # ROOT: null parentId left out
    assert all(list(v) == keys for v in vos[1:])
    assert [v["parentId"] for v in vos[1:]] == ["id-0", "id-1", "id-2", "id-1", "id-0", "id-5", "id-0"]
    for k, v in enumerate(vos[1:], 1):
        assert v["parentId"] in [u["id"] for u in vos[:k]]                # every parent earlier in the walk
    text = cc.to_json(vos)
    assert text.startswith('[{"averageRt":0,"blockQps":5,"exceptionQps":0,"id":"id-0","oneMinuteBlock":5,'
                           '"oneMinuteException":0,"oneMinutePass":12345682,"oneMinuteTotal":12345687,'
                           '"passQps":10000004,"resource":"machine-root","successQps":10000003,"threadNum":2,'
                           '"timestamp":1234,"totalQps":10000009},{"averageRt":0,"blockQps":5,"exceptionQps":0,'
                           '"id":"id-1","oneMinuteBlock":5,"oneMinuteException":0,"oneMinutePass":12345678,'
                           '"oneMinuteTotal":12345683,"parentId":"id-0","passQps":10000000,"resource":"web",')
    a = json.loads(text)[2]
    # (long) truncation; exceptionQps / oneMinuteException are the DefaultNode's own
    assert (a["averageRt"], a["exceptionQps"], a["oneMinuteException"], a["totalQps"]) == (0, 1, 4, 10000003)
    # the default id source: random UUID strings
    got = cc.tree_node_vos(tree, 1)
    assert len({v["id"] for v in got}) == 8 and all(len(v["id"]) == 36 and v["id"].count("-") == 4 for v in got)


# ------------------------------------------------------------------ the commands
class _Sentinel:
    tree = True
    resources, ids, origins = [], {}, []

    def __init__(self):
        self.calls = []

    def invocation_tree(self, now):
        self.calls.append(now)
        return _fabricated()


def test_command_center_registers_tree_commands_over_a_tree_sentinel():
    s = _Sentinel()
    c = cc.CommandCenter(s, {}, clock=lambda: 777)
    ids = iter("abcdefgh")
    c.new_id = lambda: next(ids)
    api = json.loads(c.handle("api", {})[1])
    assert len(api) == 13
    assert {"url": "/tree", "desc": "get metrics in tree mode, use id to specify detailed tree root"} in api
    assert {"url": "/jsonTree", "desc": "get tree node VO start from root node"} in api
    assert c.handle("tree", {}) == (True, cc.format_tree(_fabricated()))
    assert c.handle("tree", {"id": "web"}) == (True, cc.format_tree(_fabricated(), "web"))
    ok, text = c.handle("jsonTree", {})
    vos = json.loads(text)
    assert ok and [v["id"] for v in vos] == list("abcdefgh") and all(v["timestamp"] == 777 for v in vos)
    assert s.calls == [777, 777, 777]

    class Plain(_Sentinel):
        tree = False
    assert len(json.loads(cc.CommandCenter(Plain(), {}).handle("api", {})[1])) == 11
