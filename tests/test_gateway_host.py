"""Gateway rules on the host, no GPU: validity, index assignment, conversion and parseParameterFor against the
reference's own test cases (GatewayRuleConverterTest, GatewayRuleManagerTest, GatewayParamParserTest: the last as
data in tests/golden/gateway_param_parser.json) and against tests/gateway_trace.py; the effective parameter rule
list of a sentinel with both managers, over a stand-in library; the two commands; the request field packer."""
import json
import os
from urllib.parse import quote

import numpy as np
import pytest

from sentinel_amd import command_center as cc
from sentinel_amd import gateway as G
from sentinel_amd import local
from sentinel_amd.rules import ParamFlowItem, ParamFlowRule
from tests import gateway_trace as gt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gateway_param_parser.json")


class _Lib:
    """The loaders of the engine library, standing in without a GPU; records what each was given."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        assert name.startswith("sga_load_") or name == "sga_gateway_load", name

        def fn(handle, arr, n, *rest):
            rows = []
            if name == "sga_load_param_rules":
                rows = [(arr[i].resource, arr[i].param_idx, arr[i].count, arr[i].n_hot,
                         arr[i].hot_values[0] if arr[i].n_hot else None) for i in range(n)]
            elif name == "sga_gateway_load":
                pat = bytes(rest[0][:rest[1]])
                rows = [(a.resource, a.resource_mode, a.index, a.field, a.match_strategy,
                         pat[a.pattern_off:a.pattern_off + a.pattern_len].decode(), a.has_pattern)
                        for a in arr[:n]] + [("n_fields", rest[2])]
            self.calls.append((name, rows))
            return 0
        return fn


class _Engine:
    handle = None


class _Sentinel:
    def __init__(self, resources):
        self.resources = list(resources)
        self.ids = {n: i for i, n in enumerate(self.resources)}
        self.engine = _Engine()
        self._loaded = {}

    block_rule = local.LocalSentinel.block_rule


@pytest.fixture
def lib(monkeypatch):
    L = _Lib()
    monkeypatch.setattr(local._lib, "load", lambda: L)
    return L


def _request(triples):
    return {(k, n): v for k, n, v in triples}


def _manager(lib, rules, resources=None):
    names = resources if resources is not None else list(dict.fromkeys(r["resource"] for r in rules if r["resource"]))
    s = _Sentinel(names)
    m = G.GatewayRuleManager(s)
    prod = [gt.to_product(r) for r in rules]
    m.load_rules(prod)
    return s, m, prod


# ---- the reference's tests
def test_converter_apply_to_param_rule():
    """GatewayRuleConverterTest.testConvertAndApplyToParamRule."""
    r = G.GatewayFlowRule("routeId1", count=2, interval_sec=2, burst=2,
                          param_item=G.GatewayParamFlowItem(parse_strategy=G.PARAM_PARSE_STRATEGY_CLIENT_IP))
    p = G.to_param_rule(r, 1)
    assert (p.resource, p.count, p.control_behavior, p.duration_in_sec, p.burst_count, p.param_idx) == \
        ("routeId1", 2, 0, 2, 2, 1)
    assert r.param_item.index == 1 and p.param_flow_item_list == []
    assert p.grade == 1 and p.max_queueing_time_ms == 500


def test_manager_load_and_get(lib):
    """GatewayRuleManagerTest.testLoadAndGetGatewayRules."""
    rules = [gt.rule(resource="ahas_route", count=500, interval_sec=1),
             gt.rule(resource="ahas_route", count=20, interval_sec=2, burst=5, item={"parse_strategy": 0}),
             gt.rule(resource="complex_route_ZZZ", count=10, interval_sec=1, control_behavior=2,
                     max_queueing_timeout_ms=600, item={"parse_strategy": 2, "field_name": "X-Sentinel-Flag"})]
    s, m, prod = _manager(lib, rules)
    assert m.get_converted_param_rules("ahas_route")
    assert prod[1].param_item.index == 0 and prod[2].param_item.index == 0
    assert prod[0] in m.get_rules_for_resource("ahas_route") and prod[1] in m.get_rules_for_resource("ahas_route")
    assert m.get_converted_param_rules(" ") == [] and len(m.get_rules()) == 3
    # the rule without a paramItem takes the next free index
    assert sorted(p.param_idx for p in m.get_converted_param_rules("ahas_route")) == [0, 1]


def test_is_valid_rule():
    """GatewayRuleManagerTest.testIsValidRule."""
    I = G.GatewayParamFlowItem
    bad = [G.GatewayFlowRule(), G.GatewayFlowRule("abc", interval_sec=0),
           G.GatewayFlowRule("abc", param_item=I(parse_strategy=3)),
           G.GatewayFlowRule("abc", param_item=I(parse_strategy=3, field_name="p", pattern="def", match_strategy=-1))]
    good = [G.GatewayFlowRule("abc"), G.GatewayFlowRule("abc", param_item=I(parse_strategy=0)),
            G.GatewayFlowRule("abc", param_item=I(match_strategy=2, field_name="Origin", pattern="def"))]
    assert [G.GatewayRuleManager.is_valid_rule(r) for r in bad] == [False] * 4
    assert [G.is_valid_rule(r) for r in good] == [True] * 3
    assert not G.is_valid_rule(None)


def test_validity_compares_the_grade_with_rate_limiter():
    """GatewayRuleManager.java:122: `grade == CONTROL_BEHAVIOR_RATE_LIMITER`, not the control behaviour."""
    assert G.is_valid_rule(G.GatewayFlowRule("r", control_behavior=2, max_queueing_timeout_ms=-1))
    assert not G.is_valid_rule(G.GatewayFlowRule("r", grade=2, max_queueing_timeout_ms=-1))
    assert G.is_valid_rule(G.GatewayFlowRule("r", grade=2, max_queueing_timeout_ms=0))


@pytest.mark.parametrize("case", json.load(open(GOLDEN))["cases"], ids=lambda c: c["name"])
def test_param_parser_cases(lib, case):
    """GatewayParamParserTest: sizes 1 and 6, the API rule under the route predicate, the empty pattern, pattern
    matching -- through the manager's parse_one and through gateway_trace."""
    rules = [gt.rule(**r) for r in case["rules"]]
    s, m, prod = _manager(lib, rules)
    by_res, _ = gt.assign(rules)
    for call in case["calls"]:
        rq = _request(call["request"])
        got = m.parse_one(call["resource"], call["mode"], rq)
        assert got == gt.parse(by_res[call["resource"]], call["mode"], rq)
        assert len(got) == call["length"]
        for k, v in call["by_rule"].items():
            assert got[prod[int(k)].param_item.index] == v, (call, k)
        if "last" in call:
            assert got[-1] == call["last"]


# ---- the quirks
def test_shared_index(lib):
    """:207-209 advances the index only when the converted rule is new to the set.  paramIdx is part of
    ParamFlowRule.equals, so rules that differ only in their item still convert apart and take successive indices;
    the rules without a paramItem are the ones that share an index, the next free one; a rule listed twice counts
    once, as in the Set the reference is handed."""
    rules = [gt.rule(resource="r", count=5, item={"parse_strategy": 0}),
             gt.rule(resource="r", count=5, item={"parse_strategy": 2, "field_name": "H"}),
             gt.rule(resource="r", count=7), gt.rule(resource="r", count=8), gt.rule(resource="r", count=7)]
    rules.append(rules[1])
    s, m, prod = _manager(lib, rules)
    prod[5] = prod[1]
    m.load_rules(prod)
    assert [p.param_item.index for p in prod[:2]] == [0, 1]
    assert [(p.param_idx, p.count) for p in m.get_converted_param_rules("r")] == [(0, 5), (1, 5), (2, 7), (2, 8)]
    assert len(m.get_rules_for_resource("r")) == 4 and m.max_args == 3
    rq = {("client_ip", ""): "1.1.1.1"}
    by_res, conv = gt.assign(rules)
    assert [r["item"]["index"] for r in rules[:2]] == [0, 1]
    assert [(c["param_idx"], c["count"]) for c in conv["r"]] == [(0, 5), (1, 5), (2, 7), (2, 8)]
    assert m.parse_one("r", 0, rq) == gt.parse(by_res["r"], 0, rq) == ["1.1.1.1", None, "$D"]


def test_pattern_adds_the_not_match_item_and_prefix_keeps(lib):
    rules = [gt.rule(resource="r", count=1, item={"parse_strategy": 2, "field_name": "H", "pattern": "ab",
                                                  "match_strategy": 1}),
             gt.rule(resource="r", count=2, item={"parse_strategy": 2, "field_name": "H", "pattern": "",
                                                  "match_strategy": 0}),
             gt.rule(resource="r", count=3, item={"parse_strategy": 2, "field_name": "H"}),
             gt.rule(resource="r", count=4, item={"parse_strategy": 2, "field_name": "H", "pattern": "ab",
                                                  "match_strategy": 9}),
             gt.rule(resource="r", count=5, item={"parse_strategy": 2, "field_name": "H", "pattern": "(",
                                                  "match_strategy": 2}),
             gt.rule(resource="r", count=6, item={"parse_strategy": 7})]
    s, m, prod = _manager(lib, rules)
    conv = m.get_converted_param_rules("r")
    nm = ParamFlowItem("$NM", 10_000_000, "java.lang.String")
    assert [c.param_flow_item_list for c in conv] == [[nm], [nm], [], [nm], [nm], []]
    # PREFIX (1) and the unknown strategy 9 keep a value that does not start with the pattern; the pattern that
    # does not compile keeps it too; the unknown parse strategy 7 is null
    assert m.parse_one("r", 0, {("header", "H"): "zz"}) == ["zz"] * 5 + [None]
    assert m.fields() == [("header", "H"), ("strategy7", "")]


def test_conversion_matches_the_trace(lib):
    rules = [gt.rule(resource="a", count=3, interval_sec=2, burst=4, control_behavior=2, max_queueing_timeout_ms=70,
                     grade=1, item={"parse_strategy": 4, "field_name": "c", "pattern": "x", "match_strategy": 3}),
             gt.rule(resource="a", count=9, grade=0), gt.rule(resource="a", count=9, grade=0),
             gt.rule(resource="b", count=1), gt.rule(resource="", count=1)]
    s, m, prod = _manager(lib, rules, ["a", "b"])
    _, conv = gt.assign(rules)
    for name in ("a", "b"):
        got = [{"resource": p.resource, "grade": p.grade, "param_idx": p.param_idx, "count": p.count,
                "control_behavior": p.control_behavior, "max_queueing_time_ms": p.max_queueing_time_ms,
                "burst_count": p.burst_count, "duration_in_sec": p.duration_in_sec,
                "hot": {i.object: i.count for i in p.param_flow_item_list}}
               for p in m.get_converted_param_rules(name)]
        assert got == conv[name]
    assert len(m.get_converted_param_rules("a")) == 2 and len(m.get_rules()) == 3  # equal rules once


# ---- the effective parameter rule list
def test_effective_list_is_gateway_rules_then_param_rules(lib):
    rules = [gt.rule(resource="a", count=3, item={"parse_strategy": 0, "pattern": "1.2.3.4"}),
             gt.rule(resource="b", count=4), gt.rule(resource="elsewhere", count=4)]
    s = _Sentinel(["a", "b", "c"])
    pm = local.ParamFlowRuleManager(s)
    own = [ParamFlowRule(resource="c", count=8.0, param_idx=2), ParamFlowRule(resource="a", count=9.0, param_idx=-1)]
    pm.load_rules(own)
    assert lib.calls[-1] == ("sga_load_param_rules", [(2, 2, 8.0, 0, None), (0, -1, 9.0, 0, None)])
    assert s._loaded[local.Decision.BLOCK_PARAM] == own
    m = G.GatewayRuleManager(s)
    m.load_rules([gt.to_product(r) for r in rules])
    nm = local.param_value("$NM")
    assert nm == 0xa8199fa79222e5de
    assert lib.calls[-1] == ("sga_load_param_rules", [(0, 0, 3.0, 1, nm), (1, 0, 4.0, 0, None), (2, 2, 8.0, 0, None),
                                                       (0, -1, 9.0, 0, None)])
    conv = m.get_converted_param_rules("a") + m.get_converted_param_rules("b")
    assert s._loaded[local.Decision.BLOCK_PARAM] == conv + own
    assert lib.calls[-2] == ("sga_gateway_load", [(0, 0, 0, 0, 0, "1.2.3.4", 1), (1, 0, -1, 0, 0, "", 0),
                                                  ("n_fields", 1)])
    # the other manager re-sends the concatenation too
    pm.load_rules(own[:1])
    assert lib.calls[-1][1] == [(0, 0, 3.0, 1, nm), (1, 0, 4.0, 0, None), (2, 2, 8.0, 0, None)]
    assert s._loaded[local.Decision.BLOCK_PARAM] == conv + own[:1]
    assert pm.get_rules() == own[:1] and len(m.get_rules()) == 3
    # clearing the gateway rules leaves the parameter rules
    m.load_rules([])
    assert lib.calls[-1] == ("sga_load_param_rules", [(2, 2, 8.0, 0, None)])
    assert lib.calls[-2] == ("sga_gateway_load", [("n_fields", 0)])


def test_sentinel_without_a_gateway_manager_sends_what_it_sent(lib):
    s = _Sentinel(["a"])
    own = [ParamFlowRule(resource="a", count=2.0, param_flow_item_list=[ParamFlowItem(5, 7)])]
    local.ParamFlowRuleManager(s).load_rules(own)
    assert lib.calls == [("sga_load_param_rules", [(0, 0, 2.0, 1, 5)])]
    assert s._loaded[local.Decision.BLOCK_PARAM] == own


def test_refusals(lib):
    s = _Sentinel(["r"])
    m = G.GatewayRuleManager(s)
    many = [gt.to_product(gt.rule(resource="r", count=k, item={"parse_strategy": 0})) for k in range(64)]
    assert m.load_rules(many) == 64 and m.max_args == 64
    with pytest.raises(ValueError, match="65 arguments"):
        m.load_rules(many + [G.GatewayFlowRule("r", count=1)])
    assert len(m.get_rules()) == 64  # the refused load changed nothing
    clustered = G.GatewayFlowRule("r", count=1)
    clustered.cluster_mode = True
    with pytest.raises(ValueError, match="cluster-mode"):
        m.load_rules([clustered])


# ---- commands
def test_gateway_commands(lib):
    s = _Sentinel(["route"])
    m = G.GatewayRuleManager(s)
    plain = cc.CommandCenter(s, {}, clock=lambda: 0)
    assert "gateway/getRules" not in plain.handlers and len(plain.handlers) == 11
    c = cc.CommandCenter(s, {"gateway": m}, clock=lambda: 0)
    assert len(c.handlers) == 13
    assert c.handle("gateway/getRules", {}) == (True, "[]")
    data = [{"resource": "route", "resourceMode": 0, "grade": 1, "count": 5, "intervalSec": 2, "controlBehavior": 0,
             "burst": 1, "maxQueueingTimeoutMs": 500,
             "paramItem": {"parseStrategy": 2, "fieldName": "X-Flag", "pattern": "a b", "matchStrategy": 3}},
            {"resource": "route", "count": 9.5}]
    assert c.handle("gateway/updateRules", {"data": quote(json.dumps(data))}) == (True, "success")
    ok, text = c.handle("gateway/getRules", {})
    assert ok and json.loads(text) == [
        {"burst": 1, "controlBehavior": 0, "count": 5.0, "grade": 1, "intervalSec": 2, "maxQueueingTimeoutMs": 500,
         "paramItem": {"fieldName": "X-Flag", "index": 0, "matchStrategy": 3, "parseStrategy": 2, "pattern": "a b"},
         "resource": "route", "resourceMode": 0},
        {"burst": 0, "controlBehavior": 0, "count": 9.5, "grade": 1, "intervalSec": 1, "maxQueueingTimeoutMs": 500,
         "resource": "route", "resourceMode": 0}]
    assert [p.param_idx for p in m.get_converted_param_rules("route")] == [0, 1]
    assert c.handle("gateway/updateRules", {}) == (False, "Bad data")
    assert c.handle("gateway/updateRules", {"data": "  "}) == (False, "Bad data")
    assert c.handle("gateway/updateRules", {"data": "%7Bnot json"}) == (False, "decode gateway rule data error")
    assert len(m.get_rules()) == 2
    ok, text = c.handle("gateway/updateRules", {"data": quote(json.dumps([{"resource": "route", "clusterMode": True}]))})
    assert not ok and "cluster-mode" in text and len(m.get_rules()) == 2


def test_a_refused_table_leaves_the_manager_as_it_was(lib, monkeypatch):
    s = _Sentinel(["r"])
    m = G.GatewayRuleManager(s)
    assert m.regex_bits([0], [{}]) is None and m.parse_one("r", 0, {}) == [] and m.fields() == []  # before any load
    m.load_rules([G.GatewayFlowRule("r", count=1)])
    sent = len(lib.calls)
    monkeypatch.setattr(G, "check", lambda rc, *a: (_ for _ in ()).throw(local._lib.EngineError("refused")))
    with pytest.raises(local._lib.EngineError):
        m.load_rules([G.GatewayFlowRule("r", count=2), G.GatewayFlowRule("r", count=3)])
    assert [r.count for r in m.get_rules()] == [1] and m.max_args == 1
    assert [c[0] for c in lib.calls[sent:]] == ["sga_gateway_load"]  # the parameter rules were not re-sent


# ---- the packer
def test_pack_requests():
    fields = [("client_ip", ""), ("header", "X"), ("host", "")]
    rqs = [{("client_ip", ""): "1.2.3.4", ("header", "X"): ""},
           {("header", "X"): "hé", ("header", "Host"): "example.org"},
           {("host", ""): "own", ("header", "Host"): "ignored", ("cookie", "c"): "unused"}]
    off, ln, blob = G.pack_requests(rqs, fields)
    assert off.dtype == np.uint32 and ln.dtype == np.uint32 and blob.dtype == np.uint8
    N = G.FIELD_NULL
    assert ln.tolist() == [7, 0, N, N, 3, 11, N, N, 3]
    got = [None if l == N else bytes(blob[o:o + l]).decode() for o, l in zip(off.tolist(), ln.tolist())]
    assert got == ["1.2.3.4", "", None, None, "hé", "example.org", None, None, "own"]
    off, ln, blob = G.pack_requests([], fields)
    assert len(off) == 0 and len(blob) == 0
