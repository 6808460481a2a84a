"""Caller origins, host side: the C header and its ctypes mirror, FlowRuleManager's limitApp mapping, and a
self-check of tests/origin_trace.py.  No GPU."""
import os
import re

import numpy as np

from tests import local_trace as lt
from tests import origin_trace as ot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = 1_700_000_000_000

SYMBOLS = ["sga_flow_set_origins", "sga_load_flow_rules_origin", "sga_submit_events_origin",
           "sga_submit_events_origin_device", "sga_query_origin_node", "sga_origin_nodes_of"]
CONSTANTS = {"SGA_LIMIT_DEFAULT": 0, "SGA_LIMIT_OTHER": 0xFFFFFFFE, "SGA_LIMIT_UNKNOWN": 0xFFFFFFFF, "SGA_ENOENT": -2}


def _header():
    with open(os.path.join(ROOT, "include", "sentinel_amd.h")) as f:
        return f.read()


def test_header_declares_the_origin_entry_points():
    h = _header()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", h), s
    for name, val in CONSTANTS.items():
        m = re.search(r"#define\s+" + name + r"\s+\(?(-?[0-9A-Fa-fx]+)u?\)?", h)
        assert m, name
        assert int(m.group(1), 0) == val, (name, m.group(1))
    # new entry points only: the struct the existing loader takes keeps its layout, the ABI version stays
    assert re.search(r"#define\s+SGA_ABI_VERSION\s+3\b", h)


def test_ctypes_mirror_binds_them():
    import ctypes as C

    from sentinel_amd import _lib
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES, s
    for name, val in CONSTANTS.items():
        assert getattr(_lib, name) == val, name
    # the origin array sits after `param` (host entry) / `d_param` (device entry): one argument more each
    assert len(_lib.SIGNATURES["sga_submit_events_origin"][1]) == len(_lib.SIGNATURES["sga_submit_events_ex"][1]) + 1
    assert len(_lib.SIGNATURES["sga_submit_events_origin_device"][1]) == \
        len(_lib.SIGNATURES["sga_submit_events_device"][1]) + 1
    assert C.sizeof(_lib.SgaFlowRule) == 64


class _FakeSentinel:
    ids = {"a": 0, "b": 1}

    class engine:
        handle = None


def _with_fake(fake, fn):
    from sentinel_amd import _lib
    real = _lib.load
    _lib.load = lambda: fake
    try:
        return fn()
    finally:
        _lib.load = real


def test_rule_manager_maps_limit_app_names_to_ids():
    """On a sentinel with registered origins FlowRuleManager.load_rules names every limitApp by id and calls the
    origin loader: default 0, a registered name its id, "other" and an unregistered name the two constants."""
    from sentinel_amd import _lib, local
    from sentinel_amd.rules import FlowRule, RuleConstant

    got = {}

    class FakeLib:
        def sga_load_flow_rules_origin(self, handle, arr, lim, n):
            got["rules"] = [(arr[i].resource, arr[i].strategy, arr[i].ref_resource, lim[i]) for i in range(n)]
            return n

    class S(_FakeSentinel):
        origin_ids = {"appA": 1, "appB": 2}

    R = RuleConstant.STRATEGY_RELATE
    _with_fake(FakeLib(), lambda: local.FlowRuleManager(S()).load_rules([
        FlowRule(resource="a", count=1),
        FlowRule(resource="a", count=1, limit_app="appB"),
        FlowRule(resource="b", count=1, limit_app="appA", strategy=R, ref_resource="a"),
        FlowRule(resource="b", count=1, limit_app=RuleConstant.LIMIT_APP_OTHER),
        FlowRule(resource="b", count=1, limit_app="nobody"),
        FlowRule(resource="b", count=1, limit_app="appA", strategy=R, ref_resource=" "),
        FlowRule(resource="zzz", count=1, limit_app="appA"),
    ]))
    assert got["rules"] == [(0, 0, 0, 0), (0, 0, 0, 2), (1, 1, 0, 1), (1, 0, 0, _lib.SGA_LIMIT_OTHER),
                            (1, 0, 0, _lib.SGA_LIMIT_UNKNOWN), (1, -1, 0, 1)]


def test_rule_manager_without_origins_keeps_the_plain_loader():
    """A sentinel without origins calls sga_load_flow_rules alone, a non-default limitApp as strategy -1."""
    from sentinel_amd import local
    from sentinel_amd.rules import FlowRule

    got = {}

    class FakeLib:  # has the plain loader only: any other call fails
        def sga_load_flow_rules(self, handle, arr, n):
            got["rules"] = [(arr[i].resource, arr[i].strategy) for i in range(n)]
            return n

    class Empty(_FakeSentinel):
        origin_ids = {}

    for sentinel in (_FakeSentinel(), Empty()):
        got.clear()
        _with_fake(FakeLib(), lambda: local.FlowRuleManager(sentinel).load_rules([
            FlowRule(resource="a", count=1), FlowRule(resource="b", count=1, limit_app="appA"),
            FlowRule(resource="b", count=1, limit_app="other")]))
        assert got["rules"] == [(0, 0), (1, -1), (1, -1)]


def test_reserved_origin_names_are_refused():
    import pytest

    from sentinel_amd import local

    class E:
        handle = None

    for bad in (["default"], ["other"], ["a", ""], ["a", "a"]):
        with pytest.raises(ValueError):
            local.LocalSentinel(E(), ["r"], origins=bad)


def test_origin_trace_shadow_equals_the_resource_node():
    """Every event of a rule-free resource carries one origin: the pair's shadow node must read as the
    resource's own ClusterNode, getter by getter, at several times (clock regressions and errors included)."""
    h = ot.OriginTrace(2, 2)
    h.generate(1500, 7, T0, [1.0, 0.0], [0.0, 0.0, 1.0], gap_mean=3.0, acq_max=3, rt_max=60, regress_pct=0.05,
               err_pct=0.2)
    h.other(2, 0, 2, h.ev[-1][2] + 1, 2)                  # a block outside the engine
    d, _ = h.entry(0, 2, h.ev[-1][2] + 2, 1)
    assert d == 0
    h.other(3, 0, 2, h.ev[-1][2], 1)                      # that entry revoked
    h.other(1, 1, 1, h.ev[-1][2] + 3, 1, 0, 5)            # an exit of a pair never entered
    assert h.created == {(0, 2)}
    assert h.origin_node(1, 1, T0) is None
    tr = h.finish()
    assert len(tr["times"]) >= 3 and list(tr["onodes"]) == [(0, 2)]
    for k in range(len(tr["times"])):
        assert tr["onodes"][(0, 2)][k] == tr["nodes"][0][k], (k, list(zip(lt.NODE_GETTERS, tr["onodes"][(0, 2)][k],
                                                                          tr["nodes"][0][k])))
    assert tr["nodes"][0][0][lt.NODE_GETTERS.index("total_pass")] > 1000
    assert sorted(np.unique(tr["st"]["origin"], return_counts=True)[1]) == [1, len(tr["ed"]) - 1]
    assert np.count_nonzero(tr["ed"]) == 0
