"""RELATE FlowRules without a GPU: the event-by-event construction of tests/relate_trace.py pinned against
the oracle where both apply, and the ABI additions (sga_flow_rule.ref_resource, SGA_REF_NONE,
sga_flow_group_of)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import local_trace as lt
from tests import relate_trace as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = 1_700_000_000_000


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("regress", [0.0, 0.05])
@pytest.mark.parametrize("grade,count", [(1, 20), (0, 3)])
def test_self_reference_equals_direct(seed, regress, grade, count):
    """A RELATE rule whose refResource is its own resource selects the resource's own ClusterNode, which exists
    before its flow check: the helper's reading of the node through the getters must reproduce the oracle's
    DIRECT DefaultController exactly -- decisions, details and every node getter."""
    n_res = 2
    h = rt.RelateTrace(n_res, [{"resource": 0, "count": count, "grade": grade, "strategy": 1, "ref": 0}])
    h.generate(5000, seed, T0, [0.8, 0.2], gap_mean=2.0, acq_max=2, rt_max=39, regress_pct=regress)
    h.flush()
    st, ed, ew = h.stream()
    c = h.counts()
    assert c["blocks"] >= 100 and c["passes"] >= 100 and c["null"] == 0, c
    orc = lt.Oracle(n_res, [{"resource": 0, "count": count, "grade": grade}])
    od, ow = orc.replay(st)
    assert (od == ed).all() and (ow == ew).all(), int(((od != ed) | (ow != ew)).sum())
    t_end = int(st["ts"].max())
    for rid in range(n_res):
        assert orc.node(rid, t_end) == h.node(rid, t_end), rid
    orc.close()
    h.close()


def test_null_node_passes_until_first_entry():
    """count = 0 blocks everything -- once the referenced resource has been entered; a kind-2 event enters it."""
    h = rt.RelateTrace(3, [{"resource": 0, "count": 0, "strategy": 1, "ref": 1},
                           {"resource": 0, "count": 0, "strategy": 1, "ref": None}])
    assert h.entry(0, T0)[0] == 0
    h.other(2, 1, T0 + 1)
    assert h.entry(0, T0 + 2) == (1, 0)
    assert h.counts() == {"blocks": 1, "passes": 0, "null": 1}
    h.close()


def _header():
    text = open(os.path.join(ROOT, "include", "sentinel_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_relate_api():
    text = _header()
    assert re.search(r"#define\s+SGA_REF_NONE\s+0xFFFFFFFFu", text)
    assert re.search(r"\bint\s+sga_flow_group_of\s*\(\s*sga_engine\s*\*\s*\w*\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s*\*\s*\w+\s*\)",
                     text)
    body = re.search(r"typedef struct sga_flow_rule \{(.*?)\} sga_flow_rule;", text, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields[-1] == "ref_resource" and re.search(r"uint32_t\s+ref_resource\s*;", body)
    assert "reserved" not in fields


def test_ctypes_mirror_has_ref_resource():
    from sentinel_amd import _lib
    names = [f for f, _ in _lib.SgaFlowRule._fields_]
    assert names[-1] == "ref_resource" and "reserved" not in names
    assert _lib.SgaFlowRule.ref_resource.offset == 60 and _lib.SgaFlowRule.ref_resource.size == 4
    assert ctypes.sizeof(_lib.SgaFlowRule) == 64
    assert _lib.SGA_REF_NONE == 0xFFFFFFFF
    assert "sga_flow_group_of" in _lib.SIGNATURES


def test_rule_manager_maps_ref_names():
    """FlowRuleManager.load_rules: a blank refResource is invalid (strategy -1), an unknown name SGA_REF_NONE."""
    from sentinel_amd import _lib, local
    from sentinel_amd.rules import FlowRule, RuleConstant

    got = {}

    class FakeLib:
        def sga_load_flow_rules(self, handle, arr, n):
            got["rules"] = [(arr[i].resource, arr[i].strategy, arr[i].ref_resource) for i in range(n)]
            return n

    class FakeSentinel:
        ids = {"a": 0, "b": 1}

        class engine:
            handle = None

    real = _lib.load
    _lib.load = lambda: FakeLib()
    try:
        R = RuleConstant.STRATEGY_RELATE
        local.FlowRuleManager(FakeSentinel()).load_rules([
            FlowRule(resource="a", count=1, strategy=R, ref_resource="b"),
            FlowRule(resource="a", count=1, strategy=R, ref_resource="zzz"),
            FlowRule(resource="a", count=1, strategy=R, ref_resource=" "),
            FlowRule(resource="a", count=1, strategy=R),
            FlowRule(resource="b", count=1, strategy=RuleConstant.STRATEGY_CHAIN, ref_resource="a"),
            FlowRule(resource="b", count=1, strategy=R, ref_resource="a", limit_app="other"),
            FlowRule(resource="b", count=1)])
    finally:
        _lib.load = real
    assert got["rules"] == [(0, 1, 1), (0, 1, 0xFFFFFFFF), (0, -1, 0), (0, -1, 0), (1, 2, 0), (1, -1, 0), (1, 0, 0)]
