"""The command center's host code, without a GPU: request parsing against HttpEventTaskTest's vectors
(tests/golden/kat_HttpEventTaskTest_*.json), Double.toString, the cnode / origin tables against strings worked
out by hand from the Java format strings, the clusterNode JSON, and the rule commands."""
import io
import json
import os
import socket

import pytest

from sentinel_amd import command_center as cc
from sentinel_amd.javautil import double_to_string
from sentinel_amd.local import NodeView

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _kat(name):
    with open(os.path.join(GOLDEN, f"kat_HttpEventTaskTest_{name}.json"), encoding="utf-8") as f:
        return json.load(f)


def _view(thread=0, pass_qps=0.0, block=0.0, success=0.0, exc=0.0, rt=0.0, m_pass=0, m_block=0, m_exc=0):
    return NodeView(pass_qps, block, success, exc, 0.0, rt, 1.0, 0.0, m_pass, m_block, 0, m_exc, thread, 0, 2.0, 0.0)


# ------------------------------------------------------------------ HttpEventTask
def test_process_query_string_vectors():
    for c in _kat("query")["processQueryString"]:
        r = cc.parse_request(c["line"])
        assert r.target == c["target"] and r.parameters == c["params"], c


def test_remove_anchor_vectors():
    for c in _kat("query")["removeAnchor"]:
        assert cc.remove_anchor(c["in"]) == c["out"], c


def test_parse_single_param_and_parse_params_vectors():
    kat = _kat("query")
    for c in kat["parseSingleParam"]:
        r = cc.CommandRequest()
        cc.parse_single_param(c["in"], r)
        assert r.parameters == c["params"], c
    for c in kat["parseParams"]:
        r = cc.CommandRequest()
        cc.parse_params(c["in"], r)
        assert r.parameters == c["params"], c
    assert sum(1 for c in kat["parseParams"] if not c["params"]) == 3  # the malformed ones yield nothing


def test_post_header_and_body_vectors():
    kat = _kat("post")
    for c in kat["parsePostHeaders"]:
        assert cc.parse_post_headers(io.BytesIO(c["in"].encode("utf-8"))) == c["headers"], c
    seen = set()
    for c in kat["processPostRequest"]:
        r = cc.CommandRequest()
        r.parameters.update(c["before"])
        raw = c["in"].replace("{padding}", "&" * c.get("padding", 0)).encode("utf-8")
        status = 200
        try:
            cc.process_post_request(io.BytesIO(raw), r)
        except cc.RequestException as e:
            status = e.status
            assert e.message == {415: "Only form-encoded post request is supported",
                                 411: "No legal Content-Length"}[status]
        assert status == c["status"] and r.parameters == c["params"], c["what"]
        seen.add(status)
    assert seen == {200, 411, 415}


def test_response_is_http_1_0_with_the_byte_length():
    assert cc.format_response(200, "的x") == \
        b"HTTP/1.0 200 OK\r\nContent-Length: 4\r\nConnection: close\r\n\r\n" + "的x".encode("utf-8")
    assert cc.format_response(400, None) == b"HTTP/1.0 400 Bad Request\r\nContent-Length: 0\r\nConnection: close\r\n\r\n"


# ------------------------------------------------------------------ Double.toString
def test_double_to_string():
    cases = [(9999999.0, "9999999.0"), (1.0e7, "1.0E7"), (0.001, "0.001"), (1.0e-4, "1.0E-4"), (0.0, "0.0"),
             (12.5, "12.5"), (-0.0, "-0.0"), (1.0, "1.0"), (123456.789, "123456.789"), (1.25e10, "1.25E10"),
             (9.99e-4, "9.99E-4"), (100.0, "100.0"), (-3.5e-7, "-3.5E-7"), (0.1 + 0.2, "0.30000000000000004")]
    for x, want in cases:
        assert double_to_string(x) == want, (x, double_to_string(x))
    assert double_to_string(float("nan")) == "NaN" and double_to_string(float("-inf")) == "-Infinity"


# ------------------------------------------------------------------ cnode / origin tables
CNODE_COLS = (10, 10, 10, 11, 9, 6, 10, 11, 9, 11)  # "%-10s%-10s%-10s%-11s%-9s%-6s%-10s%-11s%-9s%-11s" after idx, id


def _cnode_line(idx, name, width, cells):
    return str(idx).ljust(4) + name.ljust(width) + "".join(c.ljust(w) for c, w in zip(cells, CNODE_COLS)) + "\n"


V = _view(thread=2, pass_qps=3.0, block=1.0, success=2.0, exc=0.0, rt=12.5, m_pass=10, m_block=5)
V_CELLS = ("2", "3.0", "1.0", "2.0", "4.0", "12.5", "10", "5", "15", "0.0")
HEAD = ("thread", "pass", "blocked", "success", "total", "aRt", "1m-pass", "1m-block", "1m-all", "exception")


def test_cnode_one_short_name_spelled_out():
    # width of "id" = 3 + 1; the width loop counted one match, so the row is number 2
    want = ("idx id  thread    pass      blocked   success    total    aRt   1m-pass   1m-block   1m-all   exception  \n"
            "2   abc 2         3.0       1.0       2.0        4.0      12.5  10        5          15       0.0        \n")
    assert cc.format_cnode([("abc", V)]) == want


@pytest.mark.parametrize("n", [79, 80, 159])
def test_cnode_long_names_wrap_at_79(n):
    name = "".join(chr(ord("a") + k % 26) for k in range(n))
    want = _cnode_line("idx", "id", 80, HEAD) + _cnode_line(2, name[:79], 80, V_CELLS)
    if n > 79:
        want += _cnode_line("", name[79:158], 80, [""] * 10)
    if n > 158:
        want += _cnode_line("", name[158:], 80, [""] * 10)
    got = cc.format_cnode([(name, V)])
    assert got == want
    assert got.count("\n") == {79: 2, 80: 3, 159: 4}[n]


@pytest.mark.parametrize("n,rows", [(29, [30]), (30, list(range(31, 61))), (31, list(range(31, 62))),
                                    (20, list(range(21, 31)))])
def test_cnode_row_cap_and_carried_index(n, rows):
    """The reference counts matches up to 30 in its width loop and keeps counting in its row loop, which stops
    when the counter reaches 30: 29 matches print one row, numbered 30; 30 and 31 print all, from 31 on."""
    names = [f"res{k:02d}" for k in range(n)]
    got = cc.format_cnode([(m, V) for m in names]).splitlines(keepends=True)
    want = [_cnode_line("idx", "id", 6, HEAD)] + [_cnode_line(i, names[k], 6, V_CELLS) for k, i in enumerate(rows)]
    assert got == want


def test_cnode_name_width_is_taken_over_the_first_30():
    names = ["ab"] * 30 + ["abcdefghij"]
    lines = cc.format_cnode([(m, V) for m in names]).splitlines()
    assert lines[0].startswith("idx id ") and lines[0][7:13] == "thread"
    # the 31st name is cut to the width of 2 and wraps
    assert lines[-5].startswith("61  ab 2") and [ln[4:6] for ln in lines[-4:]] == ["cd", "ef", "gh", "ij"]


def test_origin_table():
    o1 = _view(thread=1, pass_qps=2.0, block=0.0, rt=0.5, m_pass=7, m_block=0)
    # the origin column is as wide as the longest name + 1: 8 here
    want = ("id: svc\n\n"
            "idx origin  threadNum passQps   blockQps   totalQps aRt   1m-pass   1m-block   1m-total \n"
            "1   app-one 1         2.0       0.0        2.0      0.5   7         0          7        \n"
            "2   b       2         3.0       1.0        4.0      12.5  10        5          15       \n")
    assert cc.format_origin("svc", [("app-one", o1), ("b", V)]) == want
    many = [(f"o{k:03d}", o1) for k in range(31)]
    lines = cc.format_origin("svc", many).splitlines()
    assert len(lines) == 3 + 30 and lines[-1].startswith("30  o029 ")
    # no origin: "%-1s" is a minimum width, the heading runs into the next one as in the reference
    assert cc.format_origin("svc", []) == \
        "id: svc\n\nidx originthreadNum passQps   blockQps   totalQps aRt   1m-pass   1m-block   1m-total \n"


# ------------------------------------------------------------------ commands over a stand-in sentinel
class _Sentinel:
    """What the handlers read of a LocalSentinel, from fixed views."""

    def __init__(self, views, origins=None, entry=None):
        self.views = views  # [(name, NodeView, entered)]
        self.resources = [n for n, _, _ in views]
        self.ids = {n: i for i, n in enumerate(self.resources)}
        self.origin_views = origins or {}
        self.origins = sorted({o for v in self.origin_views.values() for o, _ in v})
        self.entry = entry
        self.calls = []

    def nodes(self, now, resources=None, not_zero=False):
        self.calls.append(("nodes", now, resources, not_zero))
        if resources is not None:
            return [("__total_inbound_traffic__", self.entry)]
        return [(n, v) for n, v, e in self.views if e and (not not_zero or v.total_pass + v.total_block > 0)]

    def origin_node_views(self, rid, now):
        self.calls.append(("origin", now, rid))
        return self.origin_views.get(rid, [])


def _center(**kw):
    views = [("alpha", _view(thread=1, pass_qps=2.9, block=0.99, success=2.0, exc=1.5, rt=7.9, m_pass=40, m_block=2,
                             m_exc=3), True),
             ("beta", _view(), True), ("gamma", _view(m_pass=5), False), ("x-alpha", _view(m_block=1), True)]
    s = _Sentinel(views, {0: [("app", V)]}, entry=_view(thread=4, pass_qps=1.0e7, block=0.0, success=12.5, rt=0.25))
    return s, cc.CommandCenter(s, kw.get("managers", {}), clock=lambda: 1_700_000_123_456)


def test_cluster_node_json():
    s, c = _center()
    ok, text = c.handle("clusterNode", {})
    assert ok and " " not in text
    rows = json.loads(text)
    assert rows[0] == {"averageRt": 7, "blockQps": 0, "exceptionQps": 1, "oneMinuteBlock": 2, "oneMinuteException": 3,
                       "oneMinutePass": 40, "oneMinuteTotal": 42, "passQps": 2, "resource": "alpha", "successQps": 2,
                       "threadNum": 1, "timestamp": 1_700_000_123_456, "totalQps": 3}
    assert [r["resource"] for r in rows] == ["alpha", "beta", "x-alpha"]
    keys = [k for k, _ in json.loads(text, object_pairs_hook=list)[0]]
    assert keys == sorted(keys) and "id" not in keys and "parentId" not in keys
    ok, text = c.handle("clusterNode", {"type": "NotZero"})
    assert ok and [r["resource"] for r in json.loads(text)] == ["alpha", "x-alpha"]
    assert [x[3] for x in s.calls] == [False, True]  # one bulk read per command


def test_cnode_origin_and_system_status_commands():
    s, c = _center()
    ok, text = c.handle("cnode", {"id": "alpha"})
    assert ok and [ln[:12].rstrip() for ln in text.splitlines()] == ["idx id", "3   alpha", "4   x-alpha"]
    assert c.handle("cnode", {}) == (False, "Invalid parameter: empty clusterNode name")
    assert c.handle("origin", {"id": "alpha"})[1].startswith("id: alpha\n\nidx origin")
    assert c.handle("origin", {"id": "lph"})[1].startswith("id: alpha\n")       # indexOf(name) > 0
    assert c.handle("origin", {"id": "alp"})[1].startswith("id: x-alpha\n\n")   # not at index 0: the next name
    assert c.handle("origin", {"id": "nope"}) == (True, "Not find cNode with id nope")
    ok, text = c.handle("systemStatus", {})
    assert ok and text == '{"b":0.0,"r":0.25,"t":4,"qps":1.0E7,"rqps":12.5}'
    assert c.handle("version", {})[0]
    api = json.loads(c.handle("api", {})[1])
    assert {"url": "/cnode", "desc": "get clusterNode metrics by id, request param: id={resourceName}"} in api
    assert len(api) == 11


class _Lib:
    """The loaders of the engine library, standing in without a GPU: every rule offered counts as loaded."""

    def __getattr__(self, name):
        assert name.startswith("sga_load_"), name
        return lambda handle, *a: a[-1]


class _Engine:
    handle = None


@pytest.fixture
def managers(monkeypatch):
    from sentinel_amd import local
    monkeypatch.setattr(local._lib, "load", lambda: _Lib())
    s = _Sentinel([("alpha", _view(), True)])
    s.engine = _Engine()
    return s, {"flow": local.FlowRuleManager(s), "degrade": local.DegradeRuleManager(s),
               "system": local.SystemRuleManager(s), "param": local.ParamFlowRuleManager(s)}


def test_set_rules_get_rules_round_trip(managers):
    from urllib.parse import quote
    s, m = managers
    c = cc.CommandCenter(s, m, clock=lambda: 0)
    assert c.handle("getRules", {"type": "flow"}) == (True, "[]")
    flow = [{"resource": "alpha", "count": 20.0, "grade": 1, "limitApp": "default", "strategy": 0,
             "controlBehavior": 2, "maxQueueingTimeMs": 300, "warmUpPeriodSec": 10, "clusterMode": False},
            {"resource": "nobody-has-this", "count": 1.5, "someFutureField": 1}]
    # the simple-http transport has decoded the parameter once already; the handler decodes again
    assert c.handle("setRules", {"type": "flow", "data": quote(json.dumps(flow))}) == (True, "success")
    got = json.loads(c.handle("getRules", {"type": "FLOW"})[1])
    assert [r["resource"] for r in got] == ["alpha", "nobody-has-this"]  # the unknown resource is kept and listed
    assert {k: got[0][k] for k in flow[0]} == flow[0] and got[1]["count"] == 1.5 and got[1]["grade"] == 1
    assert "someFutureField" not in got[1] and "refResource" not in got[0]
    assert list(got[0]) == sorted(got[0]) and got[0]["clusterConfig"]["fallbackToLocalWhenFail"] is True
    assert [r.resource for r in m["flow"].get_rules()] == ["alpha", "nobody-has-this"]

    degrade = [{"resource": "alpha", "grade": 2, "count": 4.0, "timeWindow": 10, "minRequestAmount": 3,
                "slowRatioThreshold": 0.5, "statIntervalMs": 2000}]
    assert c.handle("setRules", {"type": "degrade", "data": json.dumps(degrade)}) == (True, "success")
    assert json.loads(c.handle("getRules", {"type": "degrade"})[1]) == degrade
    system = [{"highestSystemLoad": -1.0, "highestCpuUsage": 0.8, "qps": 1.0e7, "avgRt": 50, "maxThread": -1}]
    assert c.handle("setRules", {"type": "system", "data": json.dumps(system)}) == (True, "success")
    text = c.handle("getRules", {"type": "system"})[1]
    assert json.loads(text) == system and '"qps":1.0E7' in text
    param = [{"resource": "alpha", "paramIdx": 1, "count": 5.0, "durationInSec": 2,
              "paramFlowItemList": [{"object": "7", "count": 9, "classType": "int"}]}]
    assert c.handle("setParamFlowRules", {"data": json.dumps(param)}) == (True, "success")
    got = json.loads(c.handle("getParamFlowRules", {})[1])
    assert got[0]["paramFlowItemList"] == param[0]["paramFlowItemList"] and got[0]["paramIdx"] == 1


def test_rule_type_texts(managers):
    s, m = managers
    c = cc.CommandCenter(s, m, clock=lambda: 0)
    assert c.handle("getRules", {"type": "authority"}) == (True, "[]")
    assert c.handle("getRules", {"type": "nonsense"}) == (False, "invalid type")
    assert c.handle("getRules", {}) == (False, "invalid type")
    assert c.handle("setRules", {"type": "nonsense", "data": "[]"}) == (False, "invalid type")
    ok, text = c.handle("setRules", {"type": "authority", "data": "[]"})
    assert not ok and "AuthoritySlot" in text
    ok, text = c.handle("setRules", {"type": "flow", "data": "{not json"})
    assert not ok and m["flow"].get_rules() == []


# ------------------------------------------------------------------ the socket server
def _http(port, raw: bytes) -> bytes:
    with socket.create_connection(("127.0.0.1", port), timeout=5) as s:
        s.sendall(raw)
        out = b""
        while True:
            b = s.recv(65536)
            if not b:
                return out
            out += b


def test_socket_server_answers_as_the_reference_and_takes_the_next_free_port():
    s, c = _center()
    a = cc.SimpleHttpCommandCenter(c, port=18719)
    b = cc.SimpleHttpCommandCenter(c, port=18719)
    pa, pb = a.start(), b.start()
    try:
        assert pb > pa >= 18719
        body = b'{"b":0.0,"r":0.25,"t":4,"qps":1.0E7,"rqps":12.5}'
        assert _http(pa, b"GET /systemStatus HTTP/1.1\r\nHost: x\r\n\r\n") == \
            b"HTTP/1.0 200 OK\r\nContent-Length: %d\r\nConnection: close\r\n\r\n" % len(body) + body
        assert _http(pb, b"GET /nope?a=1 HTTP/1.0\r\n\r\n").endswith(b"\r\n\r\nUnknown command `nope`")
        assert _http(pa, b"GET / HTTP/1.0\r\n\r\n") == \
            b"HTTP/1.0 400 Bad Request\r\nContent-Length: 15\r\nConnection: close\r\n\r\nInvalid command"
        assert _http(pa, b"GET /cnode HTTP/1.0\r\n\r\n").endswith(b"Invalid parameter: empty clusterNode name")
        assert _http(pa, b"GET /origin HTTP/1.0\r\n\r\n") == \
            b"HTTP/1.0 500 Internal Server Error\r\nContent-Length: 20\r\nConnection: close\r\n\r\nCommand server error"
        post = b"id=alpha"
        got = _http(pa, b"POST /cnode HTTP/1.0\r\nContent-Type: application/x-www-form-urlencoded\r\n"
                        b"Content-Length: %d\r\n\r\n" % len(post) + post)
        assert got.startswith(b"HTTP/1.0 200 OK\r\n") and b"\n3   alpha" in got
        assert _http(pa, b"POST /cnode HTTP/1.0\r\nContent-Type: application/json\r\nContent-Length: 2\r\n\r\n{}") \
            .startswith(b"HTTP/1.0 415 Unsupported Media Type\r\n")
        assert _http(pa, b"POST /cnode HTTP/1.0\r\n\r\n").startswith(b"HTTP/1.0 411 Length Required\r\n")
    finally:
        a.stop()
        b.stop()
    with pytest.raises(OSError):
        socket.create_connection(("127.0.0.1", pa), timeout=1).close()
