"""REGEX gateway items decided on the GPU (sga_gateway_load_regex, k_gateway_parse's walk) against re.fullmatch
through tests/gateway_trace.py: the host corpus at every blob offset and the dword reader's seams, the precedence of
a program over the bit word, the two parse entries, the default manager's unchanged path, the programs' lifetimes and
the loader's refusals."""
import ctypes as C

import numpy as np
import pytest

from sentinel_amd import _lib
from sentinel_amd import gateway as G
from sentinel_amd import gateway_regex as GR
from sentinel_amd.local import EV_ARGS, LocalSentinel, param_value
from tests import gateway_regex_cases as rc
from tests import gateway_trace as gt
from tests.test_gateway_gpu import NULL, _expected, _raw_parse, _string_of, _vector
from tests.test_local_parity_gpu import _engine

pytestmark = pytest.mark.gpu

SEAM_LENGTHS = [0, 1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 255]
DEVICE_PATTERNS = [r"\d+", r"[a-z]+-\d{2,4}", r"a+", r"[ab]*", r".*", r"\w*", r"[^\n]*", r"(?:é|€|a)+", r"a{2,4}",
                   r"\S*\s?", r"x*", r"x?1*x?", "[é€" + rc.CLEF + "a]+x*", r"(a|ab)(b|)", r".{0,3}", r"\W+"]


def _rules(patterns, resource="m", extra=()):
    return [gt.rule(resource=resource, count=k + 1, item={"parse_strategy": 2, "field_name": f"H{k}", "pattern": p,
                                                         "match_strategy": 2}) for k, p in enumerate(patterns)] + \
        list(extra)


def _sentinel(names, rules, max_batch=1 << 14, **kw):
    eng = _engine(max_batch)
    s = LocalSentinel(eng, names)
    m = G.GatewayRuleManager(s, **kw)
    m.load_rules([gt.to_product(r) for r in rules])
    return eng, s, m


def _count(eng):
    n = C.c_uint32(77)
    assert _lib.load().sga_gateway_regex_count(eng.handle, C.byref(n)) == 0
    return n.value


def _seam_values():
    """Per length: all one letter, all digits, a digit run broken at its last and at its first byte, and the 1- to
    4-byte mix -- so a walk that drops or repeats a byte at the head or the tail of the dword stream answers wrong."""
    out = []
    for nb in SEAM_LENGTHS:
        out += ["a" * nb, "1" * nb, _string_of(nb)]
        if nb:
            out += ["1" * (nb - 1) + "x", "x" + "1" * (nb - 1)]
    assert {len(v.encode()) for v in out} == set(SEAM_LENGTHS)
    return out


def _corpus():
    vals = list(dict.fromkeys(_seam_values() + rc.VALUES + rc.random_values(120) +
                              ["abc-12", "abc-1", "abc-12345", "tenant-0042", "Abc-123"]))
    assert "" in vals
    return vals


def test_device_equals_re_at_every_offset():
    """Every REGEX slot of one resource reads the same value; each value sits at byte offsets 0..7 of the blob.  No
    word is given: a slot that fell back to the host would keep everything."""
    rules = _rules(DEVICE_PATTERNS)
    eng, s, m = _sentinel(["m"], rules, device_regex=True)
    assert m.regex_host_items() == [] and _count(eng) == len(DEVICE_PATTERNS)
    assert m.fields() == [("header", f"H{k}") for k in range(len(DEVICE_PATTERNS))]
    by_res, _ = gt.assign(rules)
    nf = len(DEVICE_PATTERNS)
    blob, off, ln, rqs = bytearray(), [], [], []
    for v in _corpus():
        b = v.encode()
        for shift in range(8):
            blob += b"#" * (-len(blob) % 8 + shift)
            off += [len(blob)] * nf
            ln += [len(b)] * nf
            blob += b
            rqs.append({("header", f"H{k}"): v for k in range(nf)})
    # null fields: the first header, every header, all but the first
    for nulls in ([0], list(range(nf)), list(range(1, nf))):
        off += [0] * nf
        ln += [NULL if k in nulls else 3 for k in range(nf)]
        rqs.append({("header", f"H{k}"): bytes(blob[:3]).decode() for k in range(nf) if k not in nulls})
    n = len(rqs)
    assert 1000 < n < 4000
    rc_, f, p, vals = _raw_parse(s, np.zeros(n), np.zeros(n), off, ln, blob, nf, max_args=nf)
    assert rc_ == 0 and (f == EV_ARGS).all()
    kept = np.zeros(nf, int)
    for i, rq in enumerate(rqs):
        args = gt.parse(by_res["m"], 0, rq)
        assert _vector(p, vals, i) == _expected(args), (i, rq.get(("header", "H1")), off[i * nf] % 8, args)
        kept += [a is not None and a != "$NM" for a in args]
    assert (kept > 8).all() and (kept < n - 8).all(), kept  # every program both keeps and refuses
    eng.close()


MIX_RULES = [
    gt.rule(resource="m", count=1, item={"parse_strategy": 2, "field_name": "A", "pattern": r"\d+", "match_strategy": 2}),
    gt.rule(resource="m", count=2, item={"parse_strategy": 2, "field_name": "B", "pattern": r"(a)\1", "match_strategy": 2}),
    gt.rule(resource="m", count=3, item={"parse_strategy": 2, "field_name": "C", "pattern": "abc", "match_strategy": 0}),
]
MIX_A = ["123", "12a", "", "٣1", None, "1" * 40]
MIX_B = ["aa", "ab", None, "", "aa"]
MIX_C = ["abc", "abd", None, "abcd"]


def _mix_requests(n):
    return [{k: v for k, v in ((("header", "A"), MIX_A[i % 6]), (("header", "B"), MIX_B[i % 5]),
                               (("header", "C"), MIX_C[i % 4])) if v is not None} for i in range(n)]


def test_program_goes_before_the_word_and_host_items_follow_it():
    eng, s, m = _sentinel(["m"], MIX_RULES, device_regex=True)
    assert m.regex_host_items() == [("m", 1, r"(a)\1")] and _count(eng) == 1
    n = 240
    rqs = _mix_requests(n)
    own = m.regex_bits(np.zeros(n, np.uint32), rqs)
    assert set(own.tolist()) == {0, 2}  # only the host item's bit
    off, ln, blob = G.pack_requests(rqs, m.fields())
    rng = np.random.default_rng(5)
    garbage = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, size=n).astype(np.uint64)
    assert {int(g) & 3 for g in garbage} == {0, 1, 2, 3}
    for word in (garbage, ~garbage):
        rc_, f, p, vals = _raw_parse(s, np.zeros(n), np.zeros(n), off, ln, blob.tobytes(), 3, regex=word, max_args=3)
        assert rc_ == 0
        seen = set()
        for i, rq in enumerate(rqs):
            a, b, c = (rq.get(("header", h)) for h in "ABC")
            want = [None if a is None else a if gt.re.fullmatch(r"\d+", a) else "$NM",
                    None if b is None else b if (int(word[i]) >> 1) & 1 else "$NM",
                    None if c is None else c if c == "abc" else "$NM"]
            assert _vector(p, vals, i) == _expected(want), (i, rq, hex(int(word[i])))
            seen.add((want[0] == a, int(word[i]) & 1, want[1] == b, (int(word[i]) >> 1) & 1))
        assert {(x[0], x[1]) for x in seen} >= {(True, 0), (True, 1), (False, 0), (False, 1)}
    # with the manager's own word the answers are re's for all three
    by_res, _ = gt.assign(MIX_RULES)
    f, p, vals = m.parse(np.zeros(n, np.uint32), np.zeros(n, np.uint8), rqs)
    for i, rq in enumerate(rqs):
        assert _vector(p, vals, i) == _expected(gt.parse(by_res["m"], 0, rq)), (i, rq)
    eng.close()


def test_host_and_device_entries_agree():
    import torch
    n = 600
    rqs = _mix_requests(n)
    res, mode = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    eng, s, m = _sentinel(["m"], MIX_RULES, 1 << 12, device_regex=True)
    f, p, vals = m.parse(res, mode, rqs)
    by_res, _ = gt.assign(MIX_RULES)
    for i, rq in enumerate(rqs):
        assert _vector(p, vals, i) == _expected(gt.parse(by_res["m"], 0, rq)), (i, rq)
    dev = torch.device("cuda", eng.device)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731
    off, ln, blob = G.pack_requests(rqs, m.fields())
    d_flags, d_param = t(np.zeros(n, np.uint8)), t(np.zeros(n, np.int64))
    d_vals = torch.zeros(2 * m.max_args * n, dtype=torch.int64, device=dev)
    m.parse_device(t(res.view(np.int32)), t(mode), t(off.view(np.int32)), t(ln.view(np.int32)), t(blob), d_flags,
                   d_param, d_vals, regex_bits=t(m.regex_bits(res, rqs).view(np.int64)))
    s.device_status()
    assert (d_flags.cpu().numpy() == f).all() and (d_param.cpu().numpy().view(np.uint64) == p).all()
    assert (d_vals.cpu().numpy().view(np.uint64) == vals).all()
    eng.close()
    # the host form in chunks of max_batch
    eng, s, m = _sentinel(["m"], MIX_RULES, 256, device_regex=True)
    f2, p2, vals2 = m.parse(res, mode, rqs)
    assert (f2 == f).all() and (p2 == p).all() and (vals2 == vals).all()
    eng.close()


def test_a_default_manager_ignores_nothing():
    """Without device_regex the same rules follow the word: zeros turn every non-null REGEX value into "$NM"."""
    rules = _rules([r"\d+", r"a+", r"a**"])
    eng, s, m = _sentinel(["m"], rules)
    assert _count(eng) == 0 and len(m.regex_host_items()) == 3
    vals_in = ["12", "aa", "", "x"]
    rqs = [{("header", f"H{k}"): vals_in[(i + k) % 4] for k in range(3) if (i + k) % 5} for i in range(40)]
    n = len(rqs)
    off, ln, blob = G.pack_requests(rqs, m.fields())
    rc_, f, p, vals = _raw_parse(s, np.zeros(n), np.zeros(n), off, ln, blob.tobytes(), 3, regex=np.zeros(n, np.uint64))
    assert rc_ == 0
    for i, rq in enumerate(rqs):
        want = [None if rq.get(("header", f"H{k}")) is None else "$NM" for k in range(3)]
        assert _vector(p, vals, i) == _expected(want), i
    eng.close()


def _parse_one_header(s, values, word=None):
    """The first slot's strings for one-field events."""
    blob, off, ln = bytearray(), [], []
    for v in values:
        off.append(len(blob))
        ln.append(len(v.encode()))
        blob += v.encode()
    n = len(values)
    rc_, f, p, vals = _raw_parse(s, np.zeros(n), np.zeros(n), off, ln, blob, 1, regex=word)
    assert rc_ == 0
    return [int(vals[(int(p[i]) >> 32) + 1]) for i in range(n)]


def _keys(strings):
    return [param_value(x) for x in strings]


def _one_item_table(L, eng, pattern=b"\\d+", strategy=2):
    arr = (_lib.SgaGatewayItem * 1)()
    arr[0].resource, arr[0].index, arr[0].field, arr[0].match_strategy = 0, 0, 0, strategy
    arr[0].has_pattern, arr[0].pattern_off, arr[0].pattern_len = 1, 0, len(pattern)
    pat = (C.c_uint8 * len(pattern)).from_buffer_copy(pattern)
    return L.sga_gateway_load(eng.handle, arr, 1, pat, len(pattern), 1)


def _program(d, item=0, pad=0):
    """(programs, blob) of one DFA: the transitions first (even), then the class map and the accept bits."""
    blob = bytearray(b"\0" * pad) + d.trans.tobytes()
    a = (_lib.SgaGatewayRegex * 1)()
    a[0].item, a[0].n_states, a[0].n_classes, a[0].trans_off = item, d.n_states, d.n_classes, pad
    a[0].class_off = len(blob)
    blob += d.class_map.tobytes()
    a[0].accept_off = len(blob)
    blob += d.accept.tobytes()
    return a, blob


def _load_program(L, eng, a, blob, n=1):
    buf = (C.c_uint8 * max(1, len(blob))).from_buffer_copy(bytes(blob) or b"\0")
    return L.sga_gateway_load_regex(eng.handle, a, n, buf, len(blob))


def test_programs_live_and_die_with_their_table():
    L = _lib.load()
    probe = ["12", "ab", "1a", ""]
    eng, s, m = _sentinel(["m"], _rules([r"\d+"]), 1 << 12, device_regex=True)
    assert _count(eng) == 1
    assert _parse_one_header(s, probe) == _keys(["12", "$NM", "$NM", "$NM"])
    # another pattern on the same slot
    m.load_rules([gt.to_product(r) for r in _rules([r"[a-z]*"])])
    assert _count(eng) == 1 and _parse_one_header(s, probe) == _keys(["$NM", "ab", "$NM", ""])
    # rules without a REGEX item
    m.load_rules([gt.to_product(gt.rule(resource="m", count=1, item={"parse_strategy": 2, "field_name": "H0",
                                                                      "pattern": "12", "match_strategy": 0}))])
    assert _count(eng) == 0 and _parse_one_header(s, probe) == _keys(["12", "$NM", "$NM", "$NM"])
    # sga_gateway_load alone drops the programs: the slot is back on the word
    m.load_rules([gt.to_product(r) for r in _rules([r"\d+"])])
    assert _count(eng) == 1
    assert _one_item_table(L, eng) == 0
    assert _count(eng) == 0
    assert _parse_one_header(s, probe) == _keys(probe)  # no word: every value kept
    assert _parse_one_header(s, probe, np.zeros(4, np.uint64)) == _keys(["$NM"] * 4)
    # programs attached by hand, then dropped with n_programs = 0
    a, blob = _program(GR.compile_dfa(r"\d+"))
    assert _load_program(L, eng, a, blob) == 0 and _count(eng) == 1
    assert _parse_one_header(s, probe, np.zeros(4, np.uint64)) == _keys(["12", "$NM", "$NM", "$NM"])
    assert L.sga_gateway_load_regex(eng.handle, None, 0, None, 0) == 0 and _count(eng) == 0
    assert _parse_one_header(s, probe) == _keys(probe)
    # clearing the table clears them too, and programs need a table
    assert _load_program(L, eng, a, blob) == 0 and _count(eng) == 1
    assert L.sga_gateway_load(eng.handle, None, 0, None, 0, 0) == 0 and _count(eng) == 0
    assert _load_program(L, eng, a, blob) == _lib.SGA_EINVAL
    eng.close()


def test_malformed_programs_are_refused_and_the_loaded_ones_stay():
    """Loads only: no parse runs over a table the loader refused; the parse at the end runs over the programs that
    were there before."""
    L = _lib.load()
    eng = _engine(1 << 12)
    s = LocalSentinel(eng, ["m"])
    assert _one_item_table(L, eng) == 0
    good = GR.compile_dfa(r"\d+")
    a, blob = _program(good)
    assert _load_program(L, eng, a, blob) == 0 and _count(eng) == 1
    nc, ns = good.n_classes, good.n_states

    def refused(edit_dfa=None, edit_rec=None, pad=0):
        d = GR.Dfa(ns, nc, good.class_map.copy(), good.trans.copy(), good.accept.copy())
        if edit_dfa:
            edit_dfa(d)
        a, blob = _program(d, 0, pad)
        if edit_rec:
            edit_rec(a[0], len(blob))
        assert _load_program(L, eng, a, blob) == _lib.SGA_EINVAL
        assert _count(eng) == 1

    def trans(q, v):
        return lambda d: d.trans.__setitem__(q, v)

    def rec(field, value):
        return lambda a, blob_len: setattr(a, field, value(blob_len) if callable(value) else value)

    refused(trans(nc + 1, ns))                                       # a transition equal to n_states
    refused(trans(ns * nc - 1, 0xFFFF))
    refused(lambda d: d.class_map.__setitem__(200, nc))              # a class equal to n_classes
    refused(None, rec("accept_off", lambda n: n))                    # slices that end past the blob
    refused(None, rec("class_off", lambda n: n - 255))
    refused(None, rec("trans_off", lambda n: (n - 2 * ns * nc + 2) & ~1))
    refused(None, rec("trans_off", 0xFFFFFFFE))
    refused(None, None, pad=1)                                       # an odd trans_off
    refused(trans(0, 1))                                             # row 0 leaves the dead state
    refused(trans(nc - 1, 1))
    refused(lambda d: d.accept.__setitem__(0, d.accept[0] | 1))      # state 0 accepts
    refused(None, rec("item", 1))                                    # no such item
    refused(None, rec("n_states", 1))
    refused(None, rec("n_states", 65536))
    refused(None, rec("n_classes", 0))
    refused(None, rec("n_classes", 257))
    # the second of two programs is bad: neither is taken
    two = (_lib.SgaGatewayRegex * 2)()
    for k in (0, 1):
        for fld, _ in _lib.SgaGatewayRegex._fields_:
            setattr(two[k], fld, getattr(a[0], fld))
    two[1].n_states = 1
    assert _load_program(L, eng, two, blob, 2) == _lib.SGA_EINVAL and _count(eng) == 1
    assert _parse_one_header(s, ["12", "ab"], np.array([2, 1], np.uint64)) == _keys(["12", "$NM"])
    # an item that is not a REGEX item with a pattern
    assert _one_item_table(L, eng, b"12", strategy=0) == 0
    assert _load_program(L, eng, a, blob) == _lib.SGA_EINVAL and _count(eng) == 0
    assert _parse_one_header(s, ["12", "ab"]) == _keys(["12", "$NM"])
    eng.close()


def test_an_uncompilable_pattern_keeps_every_value():
    eng, s, m = _sentinel(["m"], _rules([r"a**"]), 1 << 12, device_regex=True)
    assert m.regex_host_items() == [] and _count(eng) == 1 and m.regex_bits([0], [{}]) is None
    probe = ["", "a", "zz", "é€" + rc.CLEF, "x" * 255]
    assert _parse_one_header(s, probe) == _keys(probe)
    assert _parse_one_header(s, probe, np.zeros(len(probe), np.uint64)) == _keys(probe)
    eng.close()
