"""Gateway API groups on the host (sentinel_amd/gateway_api.py): the Ant matcher's restatement, its translation to
the DFA compiler's subset checked exhaustively, the reference's quirks, the manager over a recording library, the
numpy model of the expansion the GPU tests import, the reference's own cases and the two commands."""
import itertools
import json
import os
import re

import numpy as np
import pytest

from sentinel_amd import _lib, command_center as CC, gateway_api as A, gateway_regex as GR, local

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gateway_api_filter_cases.json")

ANT_CASES = [
    ("/product/**", "/product", True), ("/product/**", "/product/", True), ("/product/**", "/product/a", True),
    ("/product/**", "/product/a/b", True), ("/product/**", "/products", False), ("/product/**", "/produc", False),
    ("/product/**", "product/a", False),
    ("/**", "/", True), ("/**", "/x/y", True),
    ("/a/*", "/a/b", True), ("/a/*", "/a/", True), ("/a/*", "/a//b", True), ("/a/*", "/a", False),
    ("/a/*", "/a/b/", False), ("/a/*", "/a/b/c", False),
    ("/a/?c", "/a/bc", True), ("/a/?c", "/a/c", False),
    ("/a/*/b", "/a//b", False),
    ("/a/*/", "/a/b/", True), ("/a/*/", "/a/b", False),
    ("/é/?", "/é/€", True),
]
# the patterns the translation was designed on
SKETCH = ["/**", "/a/**", "/a/*", "/*", "/a/?", "/a/*/b", "/**/b", "/a/**/b", "/a/**/b/**", "/*/", "/a/*/", "/a*",
          "/a**b", "/***", "/a/**/", "/**/a/*", "/?", "/a/b?/**", "/**/**", "/a/**/**/b", "/*a/**/b*", "//a/*", "/a//*"]
STRINGS = ["".join(t) for n in range(9) for t in itertools.product("/ab", repeat=n)]


@pytest.mark.parametrize("pattern,path,want", ANT_CASES)
def test_ant_match_table(pattern, path, want):
    assert A.ant_match(pattern, path) is want


@pytest.mark.parametrize("pattern", SKETCH)
def test_translated_dfa_equals_ant_match_on_every_short_string(pattern):
    assert len(STRINGS) == 9841
    rx = A.ant_to_regex(pattern)
    assert rx is not None
    d = GR.compile_dfa(rx)
    assert d is not None, rx  # a silent fallback to the host would hide a translator bug
    assert re.compile(rx) is not None
    bad = [s for s in STRINGS if d.match(s.encode()) != A.ant_match(pattern, s)]
    assert not bad, (rx, bad[:8])


def test_translated_dfa_on_the_table_and_multibyte_tokens():
    for pattern, path, want in ANT_CASES:
        d = GR.compile_dfa(A.ant_to_regex(pattern))
        assert d is not None and d.match(path.encode()) is want, (pattern, path)
    d = GR.compile_dfa(A.ant_to_regex("/é/?"))
    assert not d.match("/é/€€".encode()) and not d.match("/é/".encode()) and d.match("/é/\U0001D11E".encode())
    d = GR.compile_dfa(A.ant_to_regex("/a.b/(x)/$*"))  # the regex's own punctuation is literal
    assert d.match(b"/a.b/(x)/$1") and not d.match(b"/aXb/(x)/$1") and not d.match(b"/a.b/x/$1")


@pytest.mark.parametrize("pattern", ["a/**", "", "*", "/a/{id}", "/a/{id", "/a/id}", "/{x:[a-z]+}/**", "/a\n/*"])
def test_translator_declines(pattern):
    assert A.ant_to_regex(pattern) is None


def test_is_pattern():
    assert [A.ant_is_pattern(p) for p in ("/a", "/a*", "/a?", "/{x}", "/}x{", "/{x", "")] == \
        [False, True, True, True, False, False, False]


# ---- the manager over a library that records the table
class _Lib:
    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def __getattr__(self, name):
        if name == "sga_last_error":
            return lambda h: b""

        def fn(handle, arr, n, res, n_apis, blob, blob_len):
            assert name == "sga_gateway_api_load"
            self.calls.append(([(a.api, a.kind, a.a, a.b, a.c, a.d, a.e) for a in arr[:n]], n_apis,
                               bytes(blob[:blob_len])))
            return self.rc
        return fn


class _Engine:
    handle = None


class _Sentinel:
    def __init__(self, resources):
        self.ids = {n: i for i, n in enumerate(resources)}
        self.engine = _Engine()


def _manager(monkeypatch, resources, defs, **kw):
    L = _Lib()
    monkeypatch.setattr(local._lib, "load", lambda: L)
    m = A.GatewayApiDefinitionManager(_Sentinel(resources), **kw)
    m.load_api_definitions(defs)
    return m, L


def _api(name, *items):
    return A.ApiDefinition(name, [A.ApiPathPredicateItem(p, st) for p, st in items])


def test_prefix_without_a_wildcard_matches_nothing(monkeypatch):
    m, L = _manager(monkeypatch, ["c"], [_api("c", ("/comments", 1))])
    assert m.matching_apis_one("/comments") == [] and m.matching_apis_one("/comments/1") == []
    assert L.calls[-1][0] == []  # no predicate reaches the engine either


def test_blank_pattern_unknown_strategy_and_null_path(monkeypatch):
    m, L = _manager(monkeypatch, ["c"], [_api("c", ("", 1), ("   ", 2), (None, 0), ("/x*", 7), ("/y", -1))])
    assert [p.kind for p in m._preds["c"]] == ["exact", "exact"]
    assert m.matching_apis_one("/x*") == ["c"] and m.matching_apis_one("/xy") == [] and m.matching_apis_one("/y") == ["c"]
    assert m.matching_apis_one(None) == []
    preds, n_apis, blob = L.calls[-1]
    assert [(p[0], p[1]) for p in preds] == [(0, _lib.SGA_GW_API_EXACT)] * 2 and n_apis == 1
    assert [blob[p[2]:p[2] + p[3]] for p in preds] == [b"/x*", b"/y"]


def test_a_regex_re_rejects_ends_its_definition_and_never_accepts_all(monkeypatch):
    assert GR.compile_dfa("a**").match(b"anything")  # what the parameter items do with it: not wanted here
    defs = [_api("c", ("/keep", 0), ("a**", 2), ("/lost/**", 1), ("/lost", 0)), _api("d", ("(", 2)),
            _api("e", ("/e/\\d+", 2))]
    m, L = _manager(monkeypatch, ["c", "d", "e"], defs)
    assert [p.pattern for p in m._preds["c"]] == ["/keep"] and m._preds["d"] == []
    for path in ("/keep", "/lost", "/lost/x", "anything", "a", ""):
        assert m.matching_apis_one(path) == (["c"] if path == "/keep" else []), path
    preds, n_apis, _ = L.calls[-1]
    assert n_apis == 3 and [(p[0], p[1]) for p in preds] == [(0, _lib.SGA_GW_API_EXACT), (2, _lib.SGA_GW_API_DFA)]
    assert m.host_predicates() == [] and m.host_bits(["/e/1"]) is None


def test_is_valid_api_and_replacement(monkeypatch):
    ok = A.is_valid_api
    assert not ok(None) and not ok(A.ApiDefinition()) and not ok(A.ApiDefinition("foo")) and \
        not ok(A.ApiDefinition("  ", [])) and ok(A.ApiDefinition("foo", []))
    m, L = _manager(monkeypatch, ["a", "b"], [_api("a", ("/1", 0)), _api("b", ("/b", 0)), A.ApiDefinition("bad"),
                                              _api("a", ("/2", 0))])
    assert [d.api_name for d in m.get_api_definitions()] == ["a", "b"]
    assert m.get_api_definition("a").predicate_items[0].pattern == "/2" and m.get_api_definition(None) is None
    assert m.get_api_definition("bad") is None
    assert m.matching_apis_one("/1") == [] and m.matching_apis_one("/2") == ["a"]
    m.load_api_definitions(None)
    assert m.get_api_definitions() == [] and L.calls[-1][0] == [] and m.matching_apis_one("/2") == []
    m.load_api_definitions([_api("a", ("/1", 0))])
    m.load_api_definitions([])
    assert m.get_api_definitions() == []


def test_unregistered_names_are_kept_without_a_column(monkeypatch):
    m, L = _manager(monkeypatch, ["b"], [_api("ghost", ("/g/**", 1)), _api("b", ("/b/**", 1))])
    assert m.columns() == ["b"] and [d.api_name for d in m.get_api_definitions()] == ["ghost", "b"]
    assert m.matching_apis_one("/g/1") == ["ghost"]
    preds, n_apis, _ = L.calls[-1]
    assert n_apis == 1 and [p[0] for p in preds] == [0]


def test_device_form_tables_and_host_predicates(monkeypatch):
    defs = [_api("a", ("/a/**", 1), ("/a/{id}/*", 1), (r"/r/\d+", 2), (r"/(x)\1", 2)), _api("b", ("/a/**", 1))]
    m, L = _manager(monkeypatch, ["a", "b"], defs)
    preds, n_apis, blob = L.calls[-1]
    K = _lib
    assert [(p[0], p[1]) for p in preds] == [(0, K.SGA_GW_API_DFA), (0, K.SGA_GW_API_HOST), (0, K.SGA_GW_API_DFA),
                                             (0, K.SGA_GW_API_HOST), (1, K.SGA_GW_API_DFA)]
    assert preds[0][2:] == preds[4][2:]  # one table for one pattern
    for p, rx in ((preds[0], A.ant_to_regex("/a/**")), (preds[2], r"/r/\d+")):
        d = GR.compile_dfa(rx)
        _, _, ns, nc, co, to, ao = p
        assert (ns, nc) == (d.n_states, d.n_classes) and to % 2 == 0
        assert blob[co:co + 256] == d.class_map.tobytes() and blob[to:to + 2 * ns * nc] == d.trans.tobytes()
        assert blob[ao:ao + (ns + 7) // 8] == d.accept.tobytes()
    assert m.host_predicates() == [("a", 0, "ant", "/a/{id}/*"), ("a", 1, "regex", r"/(x)\1")]
    assert [preds[1][2], preds[3][2]] == [0, 1]
    paths = ["/a/{id}/7", "/xx", "/a/1", None, "/a/{id}/7/8"]
    assert m.host_bits(paths).tolist() == [1, 2, 0, 0, 0]
    # braces are literals for the default host matcher: a documented divergence
    assert m.matching_apis_one("/q/{id}/7") == [] and m.matching_apis_one("/a/{id}/7") == ["a", "b"]
    # a caller's matcher replaces it
    m2, _ = _manager(monkeypatch, ["a", "b"], defs, ant_host=lambda pat, path: pat == "/a/{id}/*" and path == "/zz")
    assert m2.host_bits(["/zz", "/a/{id}/7"]).tolist() == [1, 0]
    # device=False: every PREFIX and REGEX predicate is the host's
    m3, L3 = _manager(monkeypatch, ["a", "b"], defs, device=False)
    assert [p[1] for p in L3.calls[-1][0]] == [K.SGA_GW_API_HOST] * 5 and len(m3.host_predicates()) == 5
    for path in paths + ["/r/12", "/r/x"]:
        assert m3.matching_apis_one(path) == m.matching_apis_one(path)
    # small caps reach the compiler
    m4, _ = _manager(monkeypatch, ["a", "b"], defs, regex_max_states=4)
    assert len(m4.host_predicates()) == 5


def test_more_than_64_host_predicates_are_refused_and_the_manager_stays(monkeypatch):
    m, L = _manager(monkeypatch, ["a"], [_api("a", ("/ok", 0))])
    with pytest.raises(ValueError):
        m.load_api_definitions([_api("a", *[(f"/h{k}/{{v}}/*", 1) for k in range(65)])])
    assert m.matching_apis_one("/ok") == ["a"] and len(L.calls) == 1
    # a table the engine refuses leaves it too
    L.rc = _lib.SGA_EINVAL
    with pytest.raises(_lib.EngineError):
        m.load_api_definitions([_api("a", ("/other", 0))])
    assert m.matching_apis_one("/ok") == ["a"] and m.matching_apis_one("/other") == []


def test_expected_entries_model():
    NULL = A.ROUTE_NULL
    match = np.array([[0b101, 0], [0, 0], [0, 1], [1 << 63, 0]], dtype=np.uint64)
    api_res = np.arange(100, 228, dtype=np.uint32)
    fo = np.arange(8, dtype=np.uint32)
    e = A.expected_entries([7, NULL, NULL, 9], match, api_res, fo, fo + 50, 2)
    assert e["total"] == 6
    assert e["src"].tolist() == [0, 0, 0, 2, 3, 3] and e["pos"].tolist() == [0, 1, 2, 0, 0, 1]
    assert e["resource"].tolist() == [7, 100, 102, 164, 9, 163] and e["mode"].tolist() == [0, 1, 1, 1, 0, 1]
    assert e["field_off"].tolist() == [0, 1, 0, 1, 0, 1, 4, 5, 6, 7, 6, 7]
    assert e["field_len"].tolist() == [50, 51, 50, 51, 50, 51, 54, 55, 56, 57, 56, 57]
    assert A.expected_entries([], np.zeros((0, 2), np.uint64), api_res)["total"] == 0


# ---- the reference's own cases
def _golden():
    with open(GOLDEN, encoding="utf-8") as f:
        return json.load(f)


def test_reference_is_valid_api_cases():
    for case in _golden()["is_valid_api"]:
        assert A.is_valid_api(CC.rule_from_bean(A.ApiDefinition, case["definition"])) is case["valid"]


@pytest.mark.parametrize("device", [True, False])
def test_reference_filter_cases(monkeypatch, device):
    g = _golden()
    defs = [CC.rule_from_bean(A.ApiDefinition, o) for o in g["definitions"]]
    m, L = _manager(monkeypatch, [d.api_name for d in defs], defs, device=device)
    for case in g["paths"]:
        assert m.matching_apis_one(case["path"]) == case["apis"], case
    assert len(m.host_predicates()) == (0 if device else 2)


def test_predicate_struct_layout_matches_the_c_compiler(tmp_path):
    """sizeof / offsetof of sga_gateway_api_pred as gcc lays it out == the ctypes mirror, and the constants."""
    import ctypes
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cls = _lib.SgaGatewayApiPred
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sentinel_amd.h"', "int main(void) {",
             'printf("%zu\\n", sizeof(sga_gateway_api_pred));']
    expect = [ctypes.sizeof(cls)]
    for f, _ in cls._fields_:
        lines.append(f'printf("%zu\\n", offsetof(sga_gateway_api_pred, {f}));')
        expect.append(getattr(cls, f).offset)
    lines.append('printf("%d\\n%d\\n%d\\n%d\\n", SGA_GW_API_EXACT, SGA_GW_API_DFA, SGA_GW_API_HOST, SGA_GW_API_MAX);')
    expect += [_lib.SGA_GW_API_EXACT, _lib.SGA_GW_API_DFA, _lib.SGA_GW_API_HOST, _lib.SGA_GW_API_MAX]
    lines.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == expect and expect[0] == 28


# ---- the command center
def test_api_definition_commands_round_trip(monkeypatch):
    from urllib.parse import quote
    m, L = _manager(monkeypatch, ["x"], [])
    cc = CC.CommandCenter(_Sentinel(["x"]), {"gateway_api": m})
    assert "gateway/getApiDefinitions" in cc.handlers and "gateway/updateApiDefinitions" in cc.handlers
    assert "gateway/getApiDefinitions" not in CC.CommandCenter(_Sentinel(["x"]), {}).handlers
    assert cc.handle("gateway/getApiDefinitions", {}) == (True, "[]")
    for bad in ({}, {"data": ""}, {"data": "   "}):
        assert cc.handle("gateway/updateApiDefinitions", bad) == (False, "Bad data")
    assert cc.handle("gateway/updateApiDefinitions", {"data": "{not json"}) == \
        (False, "decode gateway API definition data error")
    data = _golden()["definitions"] + [{"apiName": "x"}, {"predicateItems": [{"pattern": "/nameless"}]}]
    assert cc.handle("gateway/updateApiDefinitions", {"data": quote(json.dumps(data))}) == (True, "success")
    ok, text = cc.handle("gateway/getApiDefinitions", {})
    got = json.loads(text)
    assert ok and got == _golden()["definitions"] + [{"apiName": "x", "predicateItems": []}]
    assert text.startswith('[{"apiName":"some_customized_api","predicateItems":[{"matchStrategy":1,"pattern":"/product/**"}]}')
    assert m.matching_apis_one("/product/1") == ["some_customized_api"] and m.columns() == ["x"]
    assert cc.handle("gateway/updateApiDefinitions", {"data": "[]"}) == (True, "success")
    assert cc.handle("gateway/getApiDefinitions", {}) == (True, "[]")
