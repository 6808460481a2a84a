"""Contexts, host side: the C header, its ctypes mirror and the built library, FlowRuleManager's mapping of a
CHAIN rule's refResource, and self-checks of tests/context_trace.py.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import context_trace as ct
from tests import local_trace as lt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = 1_700_000_000_000

SYMBOLS = ["sga_flow_set_contexts", "sga_load_flow_rules_ctx", "sga_submit_events_ctx",
           "sga_submit_events_ctx_device", "sga_query_context_node", "sga_context_nodes_of"]


def test_header_and_ctypes_mirror_declare_the_context_entry_points():
    from sentinel_amd import _lib
    with open(os.path.join(ROOT, "include", "sentinel_amd.h")) as f:
        h = f.read()
    for s in SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", h), s
        assert s in _lib.SIGNATURES, s
    m = re.search(r"#define\s+SGA_CONTEXT_UNKNOWN\s+(0x[0-9A-Fa-f]+)u", h)
    assert m and int(m.group(1), 0) == 0xFFFFFFFF == _lib.SGA_CONTEXT_UNKNOWN
    # entry points and constants only: no struct changed, the ABI version stays
    assert re.search(r"#define\s+SGA_ABI_VERSION\s+3\b", h)
    assert C.sizeof(_lib.SgaFlowRule) == 64
    # the context array sits after the origin array: one argument more than the _origin entries
    for a, b in (("sga_submit_events_ctx", "sga_submit_events_origin"),
                 ("sga_submit_events_ctx_device", "sga_submit_events_origin_device")):
        assert len(_lib.SIGNATURES[a][1]) == len(_lib.SIGNATURES[b][1]) + 1


def test_built_library_exports_the_context_entry_points():
    """Opens the shared library without creating an engine (no GPU needed) and looks each symbol up."""
    from sentinel_amd import _lib
    lib = _lib.load()
    for s in SYMBOLS:
        assert getattr(lib, s) is not None, s


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


def test_rule_manager_maps_a_chain_rule_s_context_name_to_its_id():
    """On a sentinel with registered contexts: a registered name -> its id, an unregistered one ->
    SGA_CONTEXT_UNKNOWN, a blank one -> strategy -1; the _ctx loader, limit_app NULL without origins."""
    from sentinel_amd import _lib, local
    from sentinel_amd.rules import FlowRule, RuleConstant

    got = {}

    class FakeLib:
        def sga_load_flow_rules_ctx(self, handle, arr, lim, n):
            got["rules"] = [(arr[i].resource, arr[i].strategy, arr[i].ref_resource) for i in range(n)]
            got["lim"] = None if lim is None else [lim[i] for i in range(n)]
            return n

    class S(_FakeSentinel):
        context_ids = {"web": 1, "job": 2}

    class Both(S):
        origin_ids = {"appA": 1}

    CH, RL = RuleConstant.STRATEGY_CHAIN, RuleConstant.STRATEGY_RELATE
    rules = [FlowRule(resource="a", count=1, strategy=CH, ref_resource="job"),
             FlowRule(resource="a", count=1, strategy=CH, ref_resource="nobody"),
             FlowRule(resource="a", count=1, strategy=CH, ref_resource=" "),
             FlowRule(resource="a", count=1, strategy=CH),
             FlowRule(resource="b", count=1),
             FlowRule(resource="b", count=1, strategy=RL, ref_resource="a"),
             FlowRule(resource="b", count=1, strategy=CH, ref_resource="web", limit_app="appA")]
    _with_fake(FakeLib(), lambda: local.FlowRuleManager(S()).load_rules(rules))
    # (without registered origins a non-default limitApp stays invalid, as on the plain loader)
    assert got["rules"] == [(0, 2, 2), (0, 2, _lib.SGA_CONTEXT_UNKNOWN), (0, -1, 0), (0, -1, 0), (1, 0, 0), (1, 1, 0),
                            (1, -1, 0)]
    assert got["lim"] is None
    _with_fake(FakeLib(), lambda: local.FlowRuleManager(Both()).load_rules(rules))
    assert got["rules"][-1] == (1, 2, 1) and got["lim"] == [0, 0, 0, 0, 0, 0, 1]


def test_rule_manager_without_contexts_is_unchanged():
    """No registered contexts: the plain loader (or the origin loader) gets a CHAIN rule as (strategy 2, ref 0),
    which the engine rejects itself."""
    from sentinel_amd import local
    from sentinel_amd.rules import FlowRule, RuleConstant

    got = {}

    class FakeLib:  # any _ctx call fails: the attribute does not exist
        def sga_load_flow_rules(self, handle, arr, n):
            got["rules"] = [(arr[i].resource, arr[i].strategy, arr[i].ref_resource) for i in range(n)]
            return n

        def sga_load_flow_rules_origin(self, handle, arr, lim, n):
            return self.sga_load_flow_rules(handle, arr, n)

    class Empty(_FakeSentinel):
        context_ids = {}

    class Origins(_FakeSentinel):
        origin_ids = {"appA": 1}

    for sentinel in (_FakeSentinel(), Empty(), Origins()):
        got.clear()
        _with_fake(FakeLib(), lambda: local.FlowRuleManager(sentinel).load_rules([
            FlowRule(resource="b", count=1, strategy=RuleConstant.STRATEGY_CHAIN, ref_resource="a"),
            FlowRule(resource="a", count=1)]))
        assert got["rules"] == [(1, 2, 0), (0, 0, 0)]


def test_duplicate_and_blank_context_names_are_refused():
    from sentinel_amd import local

    class E:
        handle = None

    for bad in (["a", "a"], ["a", ""]):
        with pytest.raises(ValueError):
            local.LocalSentinel(E(), ["r"], contexts=bad)


def test_helper_without_chain_rules_and_contexts_gives_the_plain_oracle_s_decisions():
    flow = [{"resource": 0, "count": 40}, {"resource": 1, "count": 60, "control_behavior": 2, "max_queueing_time_ms": 30}]
    h = ct.ContextTrace(2, 0, 0, flow)
    h.generate(1500, 3, T0, [1, 1], [1.0], [1.0], gap_mean=3.0, err_pct=0.1, regress_pct=0.02)
    tr = h.finish()
    assert not tr["cnodes"] and not tr["onodes"] and not tr["st"]["context"].any()
    orc = lt.Oracle(2, flow)
    od, ow = orc.replay({k: v for k, v in tr["st"].items() if k not in ("origin", "context")})
    orc.close()
    assert (od == tr["ed"]).all() and (ow == tr["ew"]).all()
    assert (tr["ed"] == 1).sum() > 50


def test_helper_s_context_shadow_equals_the_resource_node():
    """Every event of a rule-free resource carries one context: the pair's shadow DefaultNode must read as the
    resource's own ClusterNode, getter by getter; kind 2 / 3 events create, an orphan exit does not."""
    h = ct.ContextTrace(2, 0, 2)
    h.generate(1200, 7, T0, [1.0, 0.0], [1.0], [0.0, 0.0, 1.0], gap_mean=3.0, acq_max=3, rt_max=60, regress_pct=0.05,
               err_pct=0.2)
    h.other(2, 0, 0, h.ev[-1][2] + 1, 2, c=2)
    assert h.entry(0, 0, h.ev[-1][2] + 2, 1, c=2)[0] == 0
    h.other(3, 0, 0, h.ev[-1][2], 1, c=2)
    h.other(1, 1, 0, h.ev[-1][2] + 3, 1, 0, 5, c=1)  # an exit of a pair never entered
    assert h.ccreated == {(0, 2)}
    tr = h.finish()
    assert list(tr["cnodes"]) == [(0, 2)]
    for k in range(len(tr["times"])):
        assert tr["cnodes"][(0, 2)][k] == tr["nodes"][0][k], k
    assert tr["nodes"][0][0][lt.NODE_GETTERS.index("total_pass")] > 800


def test_helper_refuses_what_it_cannot_model():
    chain = {"resource": 0, "count": 5, "strategy": 2, "ref": 1}
    for rules in ([{"resource": 0, "count": 9}, chain],                     # CHAIN after a default rule
                  [dict(chain, cluster_mode=True)],                         # CHAIN in cluster mode
                  [dict(chain, limit_app=1)],                               # CHAIN with a limitApp
                  [chain, {"resource": 0, "count": 9, "limit_app": 1}]):    # ... or beside one
        with pytest.raises(AssertionError):
            ct.ContextTrace(1, 1, 1, rules)
    h = ct.ContextTrace(1, 0, 1, [chain])
    with pytest.raises(AssertionError):
        h.entry(0, 0, T0, 1, prio=1, c=1)                                   # a prioritized entry under CHAIN
    h.close()
