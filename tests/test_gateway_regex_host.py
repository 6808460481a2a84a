"""The REGEX pattern compiler (sentinel_amd/gateway_regex.py) on the host, no GPU: its DFAs against re.fullmatch over
a fixed corpus and seeded random strings, the probed shorthand sets against re itself, the constructs that must fall
back to the host word, the caps, the table invariants the C loader enforces, and what a manager built with
device_regex=True hands to the library."""
import ctypes as C
import re
import warnings

import numpy as np
import pytest

from sentinel_amd import _lib
from sentinel_amd import gateway as G
from sentinel_amd import gateway_regex as GR
from sentinel_amd import local
from tests import gateway_regex_cases as rc
from tests import gateway_trace as gt


@pytest.fixture(scope="module")
def dfas():
    return {p: GR.compile_dfa(p) for p in rc.PATTERNS}


def test_the_pattern_list_is_taken_whole(dfas):
    assert len(rc.PATTERNS) >= 60 and len(set(rc.PATTERNS)) == len(rc.PATTERNS)
    assert [p for p, d in dfas.items() if d is None] == []


def test_dfa_equals_fullmatch(dfas):
    values = rc.VALUES + rc.random_values()
    sizes = {len(v.encode()) for v in values}
    assert {0, 1, 2, 3, 4} <= sizes and max(sizes) == 255
    pairs = hits = 0
    for p, d in dfas.items():
        rx = re.compile(p)
        for v in values:
            want = bool(rx.fullmatch(v))
            assert d.match(v.encode()) == want, (p, v)
            pairs += 1
            hits += want
    share = hits / pairs
    print(f"{pairs} pairs, {hits} matches: {share:.3f}")
    assert 0.2 <= share <= 0.8, share


def test_the_named_edges(dfas):
    """The cases the corpus exists for, spelled out."""
    def m(p, v):
        got = dfas[p].match(v.encode())
        assert got == bool(re.fullmatch(p, v)), (p, v)
        return got
    assert m(r"x*", "") and not m(r"a+", "")
    assert not m(r".", "\n") and m(r".", rc.CLEF) and m(r"(?:.|\n)*", "a\nb")
    assert m(r"\d+", "1" + rc.DIGIT3) and m(r"\w", "é") and m(r"\s", rc.EMSPACE) and not m(r"\S*", rc.EMSPACE)
    assert m("[é€" + rc.CLEF + "]+", "é€" + rc.CLEF) and not m("[é€" + rc.CLEF + "]", "a")
    assert m(r"[^a]", "\n") and m(r"[^a]", "€") and not m(r"[^a]", "a")
    assert m(r"a{0}", "") and not m(r"a{0}", "a") and m(r"a{0,1}", "a") and not m(r"a{2,}", "a") and m(r"a{2,}", "aaaaa")
    assert m(r"a{2,4}", "aaaa") and not m(r"a{2,4}", "aaaaa")
    assert m(r"a|ab|abb|", "") and m(r"a|ab|abb|", "abb") and m(r"(a|ab)(b|)", "abb")
    # a byte automaton answers malformed UTF-8 too, and never leaves its tables
    for p in (r".*", r"[^a]*", r"\W+"):
        assert dfas[p].match(b"\xff") is False and dfas[p].match(b"\xc3") is False and dfas[p].match(b"\xe2\x82") is False


@pytest.mark.parametrize("letter", ["d", "w", "s"])
def test_shorthand_sets_are_res_own(letter):
    rx = re.compile("\\" + letter)
    want = {cp for cp in range(0x110000) if not 0xD800 <= cp <= 0xDFFF and rx.fullmatch(chr(cp))}
    got = GR.shorthand_ranges(letter)
    assert all(lo <= hi for lo, hi in got) and all(a[1] + 1 < b[0] for a, b in zip(got, got[1:]))
    assert sum(hi - lo + 1 for lo, hi in got) == len(want)
    assert all(cp in want for lo, hi in got for cp in range(lo, hi + 1))
    neg = GR.shorthand_ranges(letter.upper())
    assert sum(hi - lo + 1 for lo, hi in neg) == 0x110000 - 2048 - len(want)
    assert not any(cp in want for lo, hi in neg for cp in (lo, hi))


@pytest.mark.parametrize("p", rc.FALLBACKS)
def test_excluded_constructs_fall_back(p):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            re.compile(p)
        except re.error:
            pytest.fail(f"{p!r} does not compile: it belongs to the uncompilable list")
    assert GR.compile_dfa(p) is None


@pytest.mark.parametrize("p", rc.DIALECT)
def test_other_dialects_forms_fall_back(p):
    assert GR.compile_dfa(p) is None


def test_a_brace_that_opens_no_repeat():
    """`a{` is the literal language in re; the compiler may decline it, but may not answer anything else."""
    d = GR.compile_dfa(r"a{")
    assert d is None or all(d.match(v.encode()) == bool(re.fullmatch(r"a{", v)) for v in ("a{", "a", "", "a{{", "{"))


@pytest.mark.parametrize("p", rc.UNCOMPILABLE)
def test_uncompilable_patterns_accept_everything(p):
    assert G._compile(p) is None
    d = GR.compile_dfa(p)
    assert (d.n_states, d.n_classes) == (2, 1)
    for v in (b"", b"a", "é€".encode(), b"\xff", b"x" * 300):
        assert d.match(v)


def test_caps():
    assert GR.compile_dfa(r"(a|b)*a(a|b){14}") is None  # 2^15 subsets
    assert GR.compile_dfa(r"(a|b)*a(a|b){3}") is not None
    assert GR.compile_dfa(r"abcdef") is not None and GR.compile_dfa(r"abcdef", max_states=4) is None
    assert GR.compile_dfa(r"abcdef", max_states=8).n_states == 8  # dead, start, five inner, accept
    d = GR.compile_dfa(r"abcdef")
    assert GR.compile_dfa(r"abcdef", max_table_bytes=d.table_bytes) is not None
    assert GR.compile_dfa(r"abcdef", max_table_bytes=d.table_bytes - 1) is None
    assert GR.MAX_STATES == 4096 and GR.MAX_TABLE_BYTES == 1 << 20


def test_table_invariants(dfas):
    """What sga_gateway_load_regex checks before it uploads a program."""
    for p, d in list(dfas.items()) + [("a**", GR.compile_dfa("a**"))]:
        assert 2 <= d.n_states <= 65535 and 1 <= d.n_classes <= 256, p
        assert d.class_map.dtype == np.uint8 and d.class_map.shape == (256,) and int(d.class_map.max()) < d.n_classes, p
        assert d.trans.dtype == np.uint16 and d.trans.shape == (d.n_states * d.n_classes,), p
        assert int(d.trans.max()) < d.n_states and not d.trans[:d.n_classes].any(), p
        assert d.accept.dtype == np.uint8 and len(d.accept) == (d.n_states + 7) // 8 and not d.accepts(0), p
        assert set(d.class_map.tolist()) == set(range(d.n_classes)), p  # no class without a byte
        assert d.table_bytes <= GR.MAX_TABLE_BYTES and d.n_states <= GR.MAX_STATES, p


def test_minimal_automata():
    """Minimisation and class merging give the textbook sizes."""
    d = GR.compile_dfa(r"(a|b)*a(a|b){3}")
    assert d.n_states == 17 and d.n_classes == 3  # dead + 2^4 suffix states; a, b, everything else
    d = GR.compile_dfa(r"(?:a*)*")
    assert d.n_states == 2 and d.n_classes == 2
    assert GR.compile_dfa(r"a|a|a").n_states == 3


# ---- the manager over a stand-in library
class _Lib:
    def __init__(self, refuse_regex=False):
        self.calls, self.refuse_regex = [], refuse_regex

    def __getattr__(self, name):
        assert name in ("sga_load_param_rules", "sga_gateway_load", "sga_gateway_load_regex", "sga_last_error"), name

        def fn(handle, arr, n, *rest):
            if name == "sga_gateway_load_regex":
                blob = bytes(rest[0][:rest[1]])
                self.calls.append((name, [(a.item, a.n_states, a.n_classes, a.class_off, a.trans_off, a.accept_off)
                                          for a in arr[:n]], blob))
                return _lib.SGA_EINVAL if self.refuse_regex else 0
            self.calls.append((name, n))
            return 0
        if name == "sga_last_error":
            return lambda h: b""
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


def _regex_rule(resource, header, pattern, strategy=2):
    return gt.to_product(gt.rule(resource=resource, count=1, item={"parse_strategy": 2, "field_name": header,
                                                                   "pattern": pattern, "match_strategy": strategy}))


RULES = [("r", "A", r"\d+", 2), ("r", "B", r"(a)\1", 2), ("r", "C", r"abc", 0), ("q", "A", r"a**", 2),
         ("q", "D", r"", 2), ("r", "E", r"[a-z]+-\d{2,4}", 2)]


def test_manager_compiles_loads_and_remembers(monkeypatch):
    L = _Lib()
    monkeypatch.setattr(local._lib, "load", lambda: L)
    s = _Sentinel(["r", "q"])
    m = G.GatewayRuleManager(s, device_regex=True)
    m.load_rules([_regex_rule(*r) for r in RULES])
    names = [c[0] for c in L.calls]
    assert names.index("sga_gateway_load") < names.index("sga_gateway_load_regex") and names.count("sga_gateway_load_regex") == 1
    _, progs, blob = [c for c in L.calls if c[0] == "sga_gateway_load_regex"][0]
    # items are numbered as sga_gateway_load got them: r's four, then q's two; the empty pattern has no program
    assert [p[0] for p in progs] == [0, 3, 4]
    for (item, ns, nc, co, to, ao), pat in zip(progs, (r"\d+", r"[a-z]+-\d{2,4}", r"a**")):
        d = GR.compile_dfa(pat)
        assert (ns, nc) == (d.n_states, d.n_classes) and to % 2 == 0
        assert blob[co:co + 256] == d.class_map.tobytes() and blob[to:to + 2 * ns * nc] == d.trans.tobytes()
        assert blob[ao:ao + (ns + 7) // 8] == d.accept.tobytes()
    assert m.regex_host_items() == [("r", 1, r"(a)\1")]
    rqs = [{("header", "A"): "12", ("header", "B"): "aa"}, {("header", "A"): "x", ("header", "B"): "ab"},
           {("header", "A"): "x"}]
    bits = m.regex_bits([0, 0, 0], rqs)
    assert bits.tolist() == [2, 0, 2]  # only the backreference's bit; a null field keeps its bit as before
    assert m.regex_bits([1], [{("header", "A"): "zz"}]).tolist() == [0]


def test_no_host_items_means_no_word(monkeypatch):
    L = _Lib()
    monkeypatch.setattr(local._lib, "load", lambda: L)
    m = G.GatewayRuleManager(_Sentinel(["r"]), device_regex=True)
    m.load_rules([_regex_rule("r", "A", r"\d+"), _regex_rule("r", "B", r"zz", 3)])
    assert m.regex_host_items() == [] and m.regex_bits([0], [{("header", "A"): "1"}]) is None
    # small caps given to the manager reach the compiler: the item stays on the host
    m = G.GatewayRuleManager(_Sentinel(["r"]), device_regex=True, regex_max_states=4)
    m.load_rules([_regex_rule("r", "A", r"abcdef")])
    assert m.regex_host_items() == [("r", 0, r"abcdef")]
    m = G.GatewayRuleManager(_Sentinel(["r"]), device_regex=True, regex_max_table_bytes=300)
    m.load_rules([_regex_rule("r", "A", r"abcdef")])
    assert m.regex_host_items() == [("r", 0, r"abcdef")]
    # rules without a REGEX item: the programs of an earlier table are dropped by the table load alone
    n = len(L.calls)
    m.load_rules([_regex_rule("r", "B", r"zz", 3)])
    assert [c[0] for c in L.calls[n:]] == ["sga_gateway_load", "sga_load_param_rules"]


def test_default_manager_calls_no_new_entry(monkeypatch):
    L = _Lib()
    monkeypatch.setattr(local._lib, "load", lambda: L)
    m = G.GatewayRuleManager(_Sentinel(["r", "q"]))
    m.load_rules([_regex_rule(*r) for r in RULES])
    assert "sga_gateway_load_regex" not in [c[0] for c in L.calls]
    assert m.regex_host_items() == [("r", 0, r"\d+"), ("r", 1, r"(a)\1"), ("r", 3, r"[a-z]+-\d{2,4}"), ("q", 0, r"a**")]
    assert m.regex_bits([0], [{("header", "A"): "12", ("header", "B"): "ab", ("header", "E"): "ab-12"}]).tolist() == [9]


def test_refused_programs_leave_the_manager(monkeypatch):
    L = _Lib(refuse_regex=True)
    monkeypatch.setattr(local._lib, "load", lambda: L)
    m = G.GatewayRuleManager(_Sentinel(["r"]), device_regex=True)
    with pytest.raises(_lib.EngineError):
        m.load_rules([_regex_rule("r", "A", r"\d+")])
    assert m.get_rules() == [] and m.fields() == [] and m.max_args == 0 and m.regex_host_items() == []
    assert "sga_load_param_rules" not in [c[0] for c in L.calls]


def test_program_struct_layout():
    assert C.sizeof(_lib.SgaGatewayRegex) == 24
    assert [f for f, _ in _lib.SgaGatewayRegex._fields_] == ["item", "n_states", "n_classes", "class_off", "trans_off",
                                                             "accept_off"]
