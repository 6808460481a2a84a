"""AuthorityRules on the host, without a GPU: the string-level restatement of the reference's loader and checker
(tests/authority_trace.py) at its traps, AuthorityRuleManager's id resolution over a stand-in for the engine
library, the command center's authority commands, and LocalSentinel.entry raising AuthorityException."""
import ctypes as C
import json

import pytest

from sentinel_amd import command_center as cc
from sentinel_amd.rules import AuthorityRule, RuleConstant
from tests import authority_trace as at

WHITE, BLACK = RuleConstant.AUTHORITY_WHITE, RuleConstant.AUTHORITY_BLACK


# ------------------------------------------------------------------ the restatement's traps
def test_constants():
    assert (WHITE, BLACK) == (0, 1) == (at.WHITE, at.BLACK)


@pytest.mark.parametrize("limit_app,contained", [
    ("appAB", False),         # indexOf finds it, no element equals it
    ("xappA", False),
    ("appA,appB", True),
    ("appB, appA", False),    # the blank is not trimmed: " appA" is not "appA"
    ("appB,appA", True),
    ("appAB,x", False),
    ("appA", True),
    ("appA,,", True),         # split drops the trailing empty strings
    ("x", False)])
def test_contain_is_an_exact_match_of_one_element(limit_app, contained):
    assert at.pass_check(limit_app, BLACK, "appA") == (not contained)
    assert at.pass_check(limit_app, WHITE, "appA") == contained


def test_empty_origin_comma_origin_and_other_strategies():
    assert at.pass_check("appA", WHITE, "") and at.pass_check("appA", BLACK, "")
    assert at.pass_check("appA", WHITE, None)
    # an origin that holds a comma: indexOf may find it, no element of split(",") can equal it
    assert at.pass_check("a,b", BLACK, "a,b") and not at.pass_check("a,b", WHITE, "a,b")
    assert at.pass_check("appA", 2, "appA") and at.pass_check("appA", 2, "other")
    assert at.pass_check("", WHITE, "appA")  # an empty limitApp passes (never loaded: the rule is invalid)


def test_load_authority_conf():
    rules = [("r0", "  ", WHITE),         # blank limitApp: dropped
             ("", "a", WHITE),            # blank resource: dropped
             ("r0", "a", -1),             # negative strategy: dropped
             None,
             ("r0", "a", BLACK),          # the first valid rule of r0
             ("r0", "b", WHITE),          # the second rule of a resource is ignored
             ("r1", "b", 2)]              # any strategy >= 0 is valid
    conf = at.load_authority_conf(rules)
    assert conf == {"r0": ("r0", "a", BLACK), "r1": ("r1", "b", 2)}
    assert not at.check(conf, "r0", "a") and at.check(conf, "r0", "b") and at.check(conf, "r1", "a")
    assert at.check(conf, "r2", "a")  # no rule
    # a reload replaces; an empty list clears
    conf = at.load_authority_conf([("r0", "b", WHITE)])
    assert at.check(conf, "r0", "b") and not at.check(conf, "r0", "a") and "r1" not in conf
    assert at.load_authority_conf([]) == {} and at.load_authority_conf(None) == {}


def test_wrapper_turns_failing_entries_without_an_oracle():
    """AuthorityTrace over a stand-in trace: a failing entry becomes other(2, ...) with the inbound flag alone, keeps
    its flags and argument in the stream, answers 6 and schedules no exit."""
    class Inner:
        def __init__(self):
            self.ev, self.exp, self.calls = [], [], []

        def entry(self, rid, o, ts, acq=1, prio=0, hp=0, pv=0, inb=0):
            self.calls.append(("entry", rid, o))
            self.ev.append((0, rid, ts, acq, (1 if prio else 0) | (4 if hp else 0) | (8 if inb else 0), 0, pv, o))
            self.exp.append((0, 0))
            return 0, 0

        def other(self, kind, rid, o, ts, acq=1, fl=0, rt=0, pv=0):
            self.calls.append(("other", kind, rid, o, fl))
            self.ev.append((kind, rid, ts, acq, fl, rt, pv, o))
            self.exp.append((0, 0))

        def step(self, rid, o, now, ts, **kw):
            return self.entry(rid, o, ts, **kw)

    h = Inner()
    a = at.AuthorityTrace(h, ["r0", "r1"], ["appA", "appB"], [("r0", "appA", BLACK)])
    assert a.step(0, 1, 5, 5, prio=1, hp=1, pv=9, inb=1) == (6, 0)
    assert a.step(0, 2, 6, 6) == (0, 0) and a.step(0, 0, 7, 7) == (0, 0) and a.step(1, 1, 8, 8) == (0, 0)
    assert h.calls == [("other", 2, 0, 1, 8), ("entry", 0, 2), ("entry", 0, 0), ("entry", 1, 1)]
    assert h.ev[0] == (2, 0, 5, 1, 13, 0, 9, 1) and h.exp[0] == (6, 0) and a.turned == [0]
    a.load([])
    assert a.step(0, 1, 9, 9) == (0, 0)


def test_three_lane_call_holds_what_each_chunk_must_decide():
    """The stream of test_authority_gpu.py's three-lane case, chunk by chunk as the engine cuts it: inbound events
    in the second chunk alone (the arrival-order lane; the third stays small), and in every chunk passes, flow
    blocks, parameter-rule entries and authority-turned entries; system blocks in the second."""
    import numpy as np

    from tests.test_authority_gpu import LANES, _lanes_trace
    tr = _lanes_trace()
    st, ed = tr["st"], tr["ed"]
    assert len(ed) == sum(LANES) and LANES[0] == LANES[1] > 1024 >= LANES[2]
    turned = np.zeros(len(ed), bool)
    turned[tr["turned"]] = True
    lo = 0
    for k, n in enumerate(LANES):
        sl = slice(lo, lo + n)
        ent = st["kind"][sl] == 0
        d = ed[sl][ent]
        inbound = (st["flags"][sl] & 8) != 0
        assert inbound.any() == (k == 1), k
        assert (d == 0).sum() >= 50 and (d == 1).sum() >= 10 and turned[sl].sum() >= 10, (k, np.bincount(d))
        assert (ent & (st["resource"][sl] == 5) & ((st["flags"][sl] & 4) != 0)).sum() >= 10, k
        assert (st["kind"][sl] == 1).sum() >= 50 and (st["origin"][sl] != 0).sum() >= 100, k
        assert ((d == 5).sum() >= 10) == (k == 1), (k, np.bincount(d))
        lo += n
    assert tr["nodes"][0xFFFFFFFF][0] != [0] * len(tr["nodes"][0xFFFFFFFF][0])  # ENTRY_NODE counted something


# ------------------------------------------------------------------ the manager over a stand-in library
class _Lib:
    """The engine library's entry points the host side calls here, recording the authority load."""

    def __init__(self):
        self.loads = []
        self.decision = 0

    def sga_config_default(self, cfg):
        return None

    def sga_flow_set_resources(self, handle, n):
        return 0

    def sga_flow_set_origins(self, handle, n, m):
        return 0

    def sga_load_authority_rules(self, handle, resource, strategy, list_off, n, origin_ids):
        u32 = lambda p, k: list((C.c_uint32 * k).from_address(p)) if k else []  # noqa: E731
        off = u32(list_off, n + 1)
        self.loads.append({"resource": u32(resource, n), "strategy": list((C.c_int32 * n).from_address(strategy)) if n
                           else [], "list_off": off, "origin_ids": u32(origin_ids, off[-1])})
        return n

    def sga_submit_events_origin(self, handle, kind, resource, ts, acquire, flags, rt, param, origin, n, vals, nvals,
                                 dec, wait):
        (C.c_int8 * n).from_address(dec)[0] = self.decision
        return 0

    def sga_submit_events_ex(self, handle, kind, resource, ts, acquire, flags, rt, param, n, vals, nvals, dec, wait):
        return 0


class _Engine:
    handle = None


@pytest.fixture
def sentinel(monkeypatch):
    from sentinel_amd import local
    lib = _Lib()
    monkeypatch.setattr(local._lib, "load", lambda: lib)
    s = local.LocalSentinel(_Engine(), ["alpha", "beta", "gamma"], ["appA", "appB", "appC", " appA"])
    return s, lib, local


def test_manager_validity_and_first_rule_wins(sentinel):
    s, lib, local = sentinel
    m = local.AuthorityRuleManager(s)
    assert m.is_valid_rule(AuthorityRule("alpha", "appA")) and not m.is_valid_rule(None)
    assert not m.is_valid_rule(AuthorityRule("alpha", " ")) and not m.is_valid_rule(AuthorityRule(" ", "appA"))
    assert not m.is_valid_rule(AuthorityRule("alpha", "appA", -1)) and m.is_valid_rule(AuthorityRule("alpha", "a", 7))
    rules = [AuthorityRule("alpha", "", BLACK), AuthorityRule("alpha", "appB,appA,appB", BLACK),
             AuthorityRule("alpha", "appC", WHITE), AuthorityRule("nobody-has-this", "appA", WHITE),
             AuthorityRule("gamma", "appB, appA,nobody,appA,", WHITE), AuthorityRule("beta", "appC", 2)]
    assert m.load_rules(rules) == 4
    assert m.get_rules() == [rules[1], rules[3], rules[4], rules[5]]  # kept, in load order, the unknown resource too
    # the restatement keeps the same rules
    conf = at.load_authority_conf([(r.resource, r.limit_app, r.strategy) for r in rules])
    assert [conf[r.resource] for r in m.get_rules()] == [(r.resource, r.limit_app, r.strategy) for r in m.get_rules()]
    # the CSR arrays: the unknown resource is not sent; names resolve one by one, exactly; " appA" is its own origin
    unk = 0xFFFFFFFF
    assert lib.loads[-1] == {"resource": [0, 2, 1], "strategy": [BLACK, WHITE, 2], "list_off": [0, 3, 8, 9],
                             "origin_ids": [2, 1, 2, 2, 4, unk, 1, unk, 3]}


def test_manager_reload_replaces_and_empty_clears(sentinel):
    s, lib, local = sentinel
    m = local.AuthorityRuleManager(s)
    assert m.load_rules([AuthorityRule("alpha", "appA", BLACK)]) == 1
    assert m.load_rules([AuthorityRule("beta", "nobody", WHITE)]) == 1
    assert [r.resource for r in m.get_rules()] == ["beta"]
    assert lib.loads[-1] == {"resource": [1], "strategy": [WHITE], "list_off": [0, 1], "origin_ids": [0xFFFFFFFF]}
    assert m.load_rules([]) == 0 and m.get_rules() == []
    assert lib.loads[-1] == {"resource": [], "strategy": [], "list_off": [0], "origin_ids": []}


def test_entry_raises_authority_exception(sentinel):
    s, lib, local = sentinel
    assert local.Decision.BLOCK_AUTHORITY == 6 and issubclass(local.AuthorityException, local.BlockException)
    lib.decision = 6
    with pytest.raises(local.AuthorityException) as e:
        s.entry("alpha", 1_700_000_000_000, origin="appA")
    assert e.value.resource == "alpha"
    lib.decision = 0
    assert s.entry("alpha", 1_700_000_000_001, origin="appA").origin == "appA"


# ------------------------------------------------------------------ the command center
def test_command_center_round_trip_with_an_authority_manager(sentinel):
    from urllib.parse import quote
    s, lib, local = sentinel
    m = {"authority": local.AuthorityRuleManager(s)}
    c = cc.CommandCenter(s, m, clock=lambda: 0)
    assert c.handle("getRules", {"type": "authority"}) == (True, "[]")
    rules = [{"resource": "alpha", "limitApp": "appA,appB", "strategy": 1},
             {"resource": "alpha", "limitApp": "appC", "strategy": 0, "someFutureField": 1},
             {"resource": "nobody-has-this", "limitApp": "appC"}]
    assert c.handle("setRules", {"type": "authority", "data": quote(json.dumps(rules))}) == (True, "success")
    text = c.handle("getRules", {"type": "AUTHORITY"})[1]
    assert text == ('[{"limitApp":"appA,appB","resource":"alpha","strategy":1},'
                    '{"limitApp":"appC","resource":"nobody-has-this","strategy":0}]')  # keys sorted, defaults filled
    assert lib.loads[-1]["resource"] == [0] and lib.loads[-1]["origin_ids"] == [1, 2]
    n = len(lib.loads)
    ok, text = c.handle("setRules", {"type": "authority", "data": "{not json"})
    assert not ok and text.startswith("parse rule data error") and len(lib.loads) == n
    assert [r.resource for r in m["authority"].get_rules()] == ["alpha", "nobody-has-this"]  # the old rules stand
    assert c.handle("setRules", {"type": "authority", "data": "[]"}) == (True, "success")
    assert c.handle("getRules", {"type": "authority"}) == (True, "[]")


def test_command_center_without_an_authority_manager_answers_as_before(sentinel):
    s, lib, local = sentinel
    c = cc.CommandCenter(s, {"flow": local.FlowRuleManager(s)}, clock=lambda: 0)
    assert c.handle("getRules", {"type": "authority"}) == (True, "[]")
    ok, text = c.handle("setRules", {"type": "authority", "data": "[]"})
    assert not ok and text == "authority rules are not served: the engine does not run AuthoritySlot"
    assert lib.loads == []
