"""Gateway API groups on the GPU (sga_gateway_api_*): the match kernel against matching_apis_one at the dword reader's
seams and the bitmap's word seams, the expansion against the numpy model at the block's and the scan's tile
boundaries, the table's lifetimes and the loader's refusals, the front-end chain end to end, and the two commands."""
import ctypes as C
import json

import numpy as np
import pytest

from sentinel_amd import _lib
from sentinel_amd import command_center as CC
from sentinel_amd import gateway as G
from sentinel_amd import gateway_api as A
from sentinel_amd import gateway_regex as GR
from sentinel_amd.local import BlockException, LocalSentinel
from tests import gateway_trace as gt
from tests.test_gateway_gpu import _string_of
from tests.test_gateway_regex_gpu import SEAM_LENGTHS
from tests.test_local_parity_gpu import T0, _engine

pytestmark = pytest.mark.gpu
NULL = 0xFFFFFFFF
ONES = 0xFFFFFFFFFFFFFFFF
K = _lib


def _api(name, *items):
    return A.ApiDefinition(name, [A.ApiPathPredicateItem(p, st) for p, st in items])


def _sentinel(names, defs, max_batch=1 << 14, **kw):
    eng = _engine(max_batch)
    s = LocalSentinel(eng, names)
    m = A.GatewayApiDefinitionManager(s, **kw)
    m.load_api_definitions(defs)
    return eng, s, m


def _counts(eng):
    a, b = C.c_uint32(77), C.c_uint32(77)
    assert _lib.load().sga_gateway_api_count(eng.handle, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def _raw_match(eng, off, ln, blob, words, host=None, n_bytes=None):
    """sga_gateway_api_match over a layout the test made: (rc, rows), the rows pre-filled with ones."""
    off, ln = np.ascontiguousarray(off, np.uint32), np.ascontiguousarray(ln, np.uint32)
    buf = np.frombuffer(bytes(blob) or b"\0", np.uint8)
    rows = np.full((len(off), words), ONES, np.uint64)
    hb = None if host is None else np.ascontiguousarray(host, np.uint64)
    rc = _lib.load().sga_gateway_api_match(eng.handle, off.ctypes.data, ln.ctypes.data, buf.ctypes.data,
                                           len(blob) if n_bytes is None else n_bytes,
                                           hb.ctypes.data if hb is not None else None, len(off), rows.ctypes.data)
    return rc, rows


def _layout(paths):
    """Every path at byte offsets 0..7 of the blob (None: a null path): (paths per row, off, len, blob)."""
    blob, off, ln, rows = bytearray(), [], [], []
    for v in paths:
        for shift in range(8):
            blob += b"#" * (-len(blob) % 8 + shift)
            off.append(len(blob))
            if v is None:
                ln.append(NULL)
            else:
                ln.append(len(v.encode()))
                blob += v.encode()
            rows.append(v)
    return rows, off, ln, blob


def _names_of(row, columns):
    return [name for k, name in enumerate(columns) if (int(row[k >> 6]) >> (k & 63)) & 1]


# ---- 1. the match against the host model
EXACT_SEAMS = ["/" + "e" * (nb - 1) for nb in SEAM_LENGTHS if nb]
MATCH_DEFS = [
    _api("exacts", *[(p, 0) for p in EXACT_SEAMS], ("/é/€" + "\U0001D11E", 0)),
    _api("prefix", ("/p/**", 1), ("/q/*/z", 1), ("/comments", 1)),
    _api("regex", (r"/r/\d+", 2), (r"(?:/[a-zé€]+)+", 2)),
    _api("mixed", ("/m", 0), ("/m/?x", 1), (r"/m/[ab]*", 2), ("", 1)),
    _api("hostonly", (r"/(h)\1.*", 2), ("/v/{id}/*", 1)),
    _api("tail", ("/**/tail", 1), ("/**/*.jsp", 1)),
    _api("empty"),
]
MATCH_NAMES = [d.api_name for d in MATCH_DEFS]


def _match_corpus():
    out = [None, "", "/", "/m", "/m/", "/m/ax", "/m/x", "/m/abab", "/m/abc", "/q/1/z", "/q//z", "/q/1/2/z", "/comments",
           "/hh", "/hhzz", "/hz", "/v/{id}/7", "/v/3/7", "/a/b/tail", "/tail", "/tail/x", "/x/y/index.jsp", "/é/€\U0001D11E",
           "/é/€", "/r/12", "/r/1x", "/r/", "/abc/é€/x", "/abc/É", "p/x"]
    for nb in SEAM_LENGTHS:
        out += ["/" * nb, _string_of(nb), ("/" + _string_of(nb - 1)) if nb else ""]
        if nb >= 1:
            out += ["/" + "e" * (nb - 1), "/" + "e" * (nb - 2) + "f" if nb >= 2 else "e", "x" + "e" * (nb - 1)]
        if nb >= 3:
            out += ["/p/" + "a" * (nb - 3), "/r/" + "1" * (nb - 3), "/pp" + "a" * (nb - 3)]
        if nb >= 4:
            out += ["/r/" + "1" * (nb - 4) + "x", "/r/x" + "1" * (nb - 4), "/" + "a" * (nb - 2) + "é"]
        if nb >= 6:
            out += ["/" + "z" * (nb - 6) + "/tail", "/" + "z" * (nb - 6) + "/tai1"]
    out = list(dict.fromkeys(out))
    assert {len(v.encode()) for v in out if v is not None} >= set(SEAM_LENGTHS)
    return out


def test_match_equals_the_host_model_at_every_offset():
    eng, s, m = _sentinel(MATCH_NAMES, MATCH_DEFS)
    assert m.columns() == MATCH_NAMES and m.words == 1
    assert [(h[0], h[2]) for h in m.host_predicates()] == [("hostonly", "regex"), ("hostonly", "ant")]
    n_dev = sum(p.where == "device" for lst in m._preds.values() for p in lst)
    assert _counts(eng) == (len(MATCH_NAMES), n_dev) and n_dev == len(EXACT_SEAMS) + 1 + 2 + 2 + 3 + 2
    rows, off, ln, blob = _layout(_match_corpus())
    assert 1000 < len(rows) < 3000
    rc, got = _raw_match(eng, off, ln, blob, 1, host=m.host_bits(rows))
    assert rc == 0
    hits = {name: 0 for name in MATCH_NAMES}
    for i, v in enumerate(rows):
        want = m.matching_apis_one(v)
        assert _names_of(got[i], MATCH_NAMES) == want, (i, v, off[i] % 8)
        for name in want:
            hits[name] += 1
    assert hits.pop("empty") == 0 and all(8 <= h < len(rows) - 8 for h in hits.values()), hits
    # no host word: the host predicates do not match -- a missing answer enters nothing
    rc, bare = _raw_match(eng, off, ln, blob, 1)
    assert rc == 0
    for i, v in enumerate(rows):
        want = [name for name, lst in m._preds.items()
                if v is not None and any(p.where == "device" and m._test(p, v) for p in lst)]
        assert _names_of(bare[i], MATCH_NAMES) == want, (i, v)
    assert (bare != got).any() and not ((bare >> np.uint64(4)) & np.uint64(1)).any()
    # the manager's own entry fills the word itself
    assert (m.match(rows) == got).all() and (m.match(rows, host_bits=None) == bare).all()
    eng.close()


def test_device_false_and_device_true_give_the_same_bitmaps():
    rows = _match_corpus()
    maps = []
    for device in (True, False):
        eng, s, m = _sentinel(MATCH_NAMES, MATCH_DEFS, device=device)
        assert (len(m.host_predicates()) == 2) is device
        maps.append(m.match(rows))
        eng.close()
    assert (maps[0] == maps[1]).all() and maps[0].any()


def test_match_device_equals_the_host_entry():
    import torch
    eng, s, m = _sentinel(MATCH_NAMES, MATCH_DEFS)
    rows, off, ln, blob = _layout(_match_corpus())
    rc, want = _raw_match(eng, off, ln, blob, 1, host=m.host_bits(rows))
    dev = torch.device("cuda", eng.device)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731
    d_match = torch.full((len(rows),), -1, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    host = t(m.host_bits(rows).view(np.int64))
    torch.cuda.synchronize(dev)  # the inputs are in place before another stream reads them
    m.match_device(t(np.array(off, np.uint32).view(np.int32)), t(np.array(ln, np.uint32).view(np.int32)),
                   t(np.frombuffer(bytes(blob), np.uint8)), d_match,
                   host_bits=host, stream=side)
    s.device_status()
    assert (d_match.cpu().numpy().view(np.uint64) == want[:, 0]).all()
    eng.close()


# ---- 2. the bitmap's word seams
@pytest.mark.parametrize("n_apis", [1, 63, 64, 65, 129])
def test_bitmap_seams(n_apis):
    names = [f"api{k}" for k in range(n_apis)]
    marked = sorted({k for k in (0, 63, 64, n_apis - 1) if k < n_apis})
    defs = [_api(name, (f"/only{k}", 0), *([("/seam/**", 1)] if k in marked else [])) for k, name in enumerate(names)]
    eng, s, m = _sentinel(names, defs)
    words = (n_apis + 63) // 64
    assert m.words == words and _counts(eng) == (n_apis, n_apis + len(marked))
    paths = ["/seam/x", "/none", f"/only{n_apis - 1}", "/only0", None, "/seam"]
    off, ln, blob = A.pack_paths(paths)
    rc, rows = _raw_match(eng, off, ln, blob.tobytes(), words)  # the rows arrive full of ones
    assert rc == 0

    def row(ks):
        out = [0] * words
        for k in ks:
            out[k >> 6] |= 1 << (k & 63)
        return out
    assert rows.tolist() == [row(marked), row([]), row([n_apis - 1]), row([0]), row([]), row(marked)]
    eng.close()


# ---- 3. the expansion
N_APIS_X = 65
EXPAND_N = [1, 255, 256, 257, 4095, 4096, 4097]  # the kernels' 256-thread blocks, the scan's 4,096-element tile


def _expand_table(eng_names=N_APIS_X):
    names = ["routeA", "routeB"] + [f"g{k}" for k in range(eng_names)]
    defs = [_api(f"g{k}", (f"/g{k}", 0)) for k in range(eng_names)]
    return names, defs


def _expand_inputs(n, seed):
    """Routes, a bitmap and a two-column field table: requests without a route and without a match, route-only
    requests, one that matches every API, sparse ones."""
    rng = np.random.default_rng(seed)
    routes = rng.choice(np.array([0, 1, NULL], np.uint32), size=n)
    match = np.zeros((n, 2), np.uint64)
    kind = rng.integers(0, 4, size=n)
    for i in np.nonzero(kind >= 2)[0]:
        for k in rng.integers(0, N_APIS_X, size=int(rng.integers(1, 4))):
            match[i, int(k) >> 6] |= np.uint64(1 << (int(k) & 63))
    match[n // 2] = (ONES, 1)
    if n > 2:
        routes[0], match[0] = NULL, 0
        routes[n - 1], match[n - 1] = 1, (1 << 63, 1)
    fo = rng.integers(0, 1 << 31, size=2 * n).astype(np.uint32)
    fl = rng.integers(0, 1 << 31, size=2 * n).astype(np.uint32)
    return routes, match, fo, fl


@pytest.fixture(scope="module")
def expand_engine():
    names, defs = _expand_table()
    eng, s, m = _sentinel(names, defs, 1 << 13)
    yield eng, s, m
    eng.close()


@pytest.mark.parametrize("n", EXPAND_N)
def test_expand_device_equals_the_model(expand_engine, n):
    import torch
    eng, s, m = expand_engine
    api_res = np.arange(2, 2 + N_APIS_X, dtype=np.uint32)
    routes, match, fo, fl = _expand_inputs(n, n)
    want = A.expected_entries(routes, match, api_res, fo, fl, 2)
    total = want["total"]
    assert total >= 1 + N_APIS_X or n == 1
    dev = torch.device("cuda", eng.device)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731
    d_routes, d_match = t(routes.view(np.int32)), t(match.view(np.int64))
    d_fo, d_fl = t(fo.view(np.int32)), t(fl.view(np.int32))
    for cap in (total, total - 1):
        room = total + 8
        out = {k: torch.full((room * w,), 0x5A, dtype=dt, device=dev)
               for k, w, dt in (("src", 1, torch.int32), ("pos", 1, torch.int32), ("resource", 1, torch.int32),
                                ("mode", 1, torch.uint8), ("field_off", 2, torch.int32), ("field_len", 2, torch.int32))}
        d_total = torch.full((1,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        m.expand_device(d_routes, d_match, cap, out["src"], out["pos"], out["resource"], out["mode"], d_total,
                        field_off=d_fo, field_len=d_fl, n_fields=2, field_off_out=out["field_off"],
                        field_len_out=out["field_len"])
        s.device_status()
        assert int(d_total.item()) == total
        for k, v in out.items():
            w = 2 if k.startswith("field_") else 1
            got = v.cpu().numpy()
            got = got.view(np.uint32) if got.dtype == np.int32 else got
            assert (got[:cap * w] == want[k][:cap * w]).all(), (k, cap)
            assert (got[cap * w:] == 0x5A).all(), (k, cap)  # nothing at or past cap
    # without the gather
    d_total = torch.zeros(1, dtype=torch.int32, device=dev)
    src = torch.zeros(total, dtype=torch.int32, device=dev)
    pos, res = torch.zeros_like(src), torch.zeros_like(src)
    mode = torch.zeros(total, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    m.expand_device(d_routes, d_match, total, src, pos, res, mode, d_total)
    s.device_status()
    assert (src.cpu().numpy().view(np.uint32) == want["src"]).all() and (mode.cpu().numpy() == want["mode"]).all()


@pytest.mark.parametrize("n,max_batch", [(257, 1 << 13), (4097, 1 << 13), (2 * 64 + 3, 64)])
def test_expand_host_form_and_its_chunks(n, max_batch):
    names, defs = _expand_table()
    eng, s, m = _sentinel(names, defs, max_batch)
    api_res = np.arange(2, 2 + N_APIS_X, dtype=np.uint32)
    routes, match, fo, fl = _expand_inputs(n, 100 + n)
    want = A.expected_entries(routes, match, api_res, fo, fl, 2)
    got = m.expand(routes, match, fo, fl, 2)
    assert got["total"] == want["total"]
    for k in ("src", "pos", "resource", "mode", "field_off", "field_len"):
        assert (got[k] == want[k]).all(), k
    bare = m.expand(routes, match)
    assert (bare["src"] == want["src"]).all() and "field_off" not in bare
    # one entry short: SGA_ERANGE, the need reported, the entries that fit written
    total = want["total"]
    src, pos, res = (np.full(total, 0x5A5A5A5A, np.uint32) for _ in range(3))
    mode = np.full(total, 0x5A, np.uint8)
    need = C.c_size_t(0)
    rc = _lib.load().sga_gateway_api_expand(eng.handle, routes.ctypes.data, match.ctypes.data, n, None, None, 0,
                                            total - 1, src.ctypes.data, pos.ctypes.data, res.ctypes.data,
                                            mode.ctypes.data, None, None, C.byref(need))
    assert rc == K.SGA_ERANGE and need.value == total
    assert (src[:-1] == want["src"][:-1]).all() and (res[:-1] == want["resource"][:-1]).all()
    assert src[-1] == 0x5A5A5A5A and mode[-1] == 0x5A
    with pytest.raises(ValueError, match=str(total)):
        m.expand(routes, match, cap=total - 1)
    eng.close()


def test_host_match_in_chunks():
    eng, s, m = _sentinel(MATCH_NAMES, MATCH_DEFS, 64)
    rows = (_match_corpus() * 2)[:2 * 64 + 3]
    got = m.match(rows)
    for i, v in enumerate(rows):
        assert _names_of(got[i], MATCH_NAMES) == m.matching_apis_one(v), (i, v)
    eng.close()


# ---- 4. lifetimes and refusals
def _preds(rows):
    arr = (K.SgaGatewayApiPred * max(1, len(rows)))()
    for a, row in zip(arr, rows):
        a.api, a.kind, a.a, a.b, a.c, a.d, a.e = tuple(row) + (0,) * (7 - len(row))
    return arr


def _load(eng, rows, api_res, blob):
    res = np.ascontiguousarray(api_res, np.uint32)
    buf = (C.c_uint8 * max(1, len(blob))).from_buffer_copy(bytes(blob) or b"\0")
    return _lib.load().sga_gateway_api_load(eng.handle, _preds(rows), len(rows), res.ctypes.data if len(res) else None,
                                            len(res), buf, len(blob))


def _dfa_row(api, d, blob, pad=0):
    """Appends d's tables to blob (the transitions first, at an even offset + pad) and returns its predicate row."""
    blob += b"\0" * ((len(blob) & 1) + pad)
    t_off = len(blob)
    blob += d.trans.tobytes()
    c_off = len(blob)
    blob += d.class_map.tobytes()
    a_off = len(blob)
    blob += d.accept.tobytes()
    return [api, K.SGA_GW_API_DFA, d.n_states, d.n_classes, c_off, t_off, a_off]


def test_without_a_table_nothing_is_launched():
    eng = _engine(1 << 12)
    LocalSentinel(eng, ["a", "b"])
    assert _counts(eng) == (0, 0)
    rc, rows = _raw_match(eng, [0, 0], [1, 1], b"/", 1)
    assert rc == 0 and (rows == ONES).all()
    src = np.full(4, 0x5A5A5A5A, np.uint32)
    total = C.c_size_t(99)
    routes, match = np.zeros(2, np.uint32), np.zeros(2, np.uint64)
    rc = _lib.load().sga_gateway_api_expand(eng.handle, routes.ctypes.data, match.ctypes.data, 2, None, None, 0, 4,
                                            src.ctypes.data, src.ctypes.data, src.ctypes.data, src.ctypes.data, None,
                                            None, C.byref(total))
    assert rc == 0 and total.value == 99 and (src == 0x5A5A5A5A).all()
    eng.close()


def test_reload_clear_and_refusals_leave_the_previous_table_answering():
    eng = _engine(1 << 12)
    s = LocalSentinel(eng, ["a", "b", "c"])
    good = GR.compile_dfa(r"/r/\d+")
    ns, nc = good.n_states, good.n_classes
    probe = ["/x", "/r/12", "/y", "/r/", None]
    off, ln, pblob = A.pack_paths(probe)

    def answers(words=1, host=None):
        rc, rows = _raw_match(eng, off, ln, pblob.tobytes(), words, host=host)
        assert rc == 0
        return rows[:, 0].tolist()

    blob = bytearray(b"/x")
    table1 = [[0, K.SGA_GW_API_EXACT, 0, 2], _dfa_row(1, good, blob), [1, K.SGA_GW_API_HOST, 5]]
    assert _load(eng, table1, [0, 2], blob) == 0 and _counts(eng) == (2, 2)
    first = [1, 2, 0, 0, 0]
    assert answers() == first and answers(host=[1 << 5] * 5) == [3, 2, 2, 2, 0]
    # a reload replaces the table
    assert _load(eng, [[2, K.SGA_GW_API_EXACT, 0, 2], [0, K.SGA_GW_API_EXACT, 1, 1]], [0, 1, 2], b"/y") == 0
    assert _counts(eng) == (3, 2) and answers() == [0, 0, 4, 0, 0]
    assert _load(eng, table1, [0, 2], blob) == 0 and answers() == first

    def refused(rows, api_res=(0, 2), data=None, rc=K.SGA_EINVAL):
        assert _load(eng, rows, list(api_res), blob if data is None else data) == rc
        assert _counts(eng) == (2, 2) and answers() == first

    refused([[2, K.SGA_GW_API_EXACT, 0, 2]])                         # an api equal to n_apis
    refused([[0, K.SGA_GW_API_EXACT, 0, 2]], api_res=(0, 3))         # a resource equal to the resource count
    refused([[0, 3, 0, 0]])                                          # no such kind
    refused([[0, K.SGA_GW_API_EXACT, len(blob) - 1, 2]])             # a pattern that ends past the blob
    refused([[0, K.SGA_GW_API_EXACT, 0xFFFFFFFF, 2]])
    refused([[0, K.SGA_GW_API_HOST, 64]])                            # no such bit
    refused([[0, K.SGA_GW_API_EXACT, 0, 2]], api_res=())             # predicates without APIs
    refused(table1 + [[0, K.SGA_GW_API_HOST, k % 64] for k in range(64)], rc=K.SGA_ERANGE)  # 65 host predicates
    refused([[0, K.SGA_GW_API_EXACT, 0, 2]], api_res=[0] * (K.SGA_GW_API_MAX + 1), rc=K.SGA_ERANGE)

    def bad_dfa(edit_dfa=None, edit_row=None, pad=0):
        d = GR.Dfa(ns, nc, good.class_map.copy(), good.trans.copy(), good.accept.copy())
        if edit_dfa:
            edit_dfa(d)
        data = bytearray(b"/x")
        row = _dfa_row(1, d, data, pad)
        if edit_row:
            edit_row(row, len(data))
        refused([row], data=data)

    def trans(q, v):
        return lambda d: d.trans.__setitem__(q, v)

    def rec(idx, value):
        return lambda row, n: row.__setitem__(idx, value(n) if callable(value) else value)

    bad_dfa(trans(nc + 1, ns))                                       # a transition equal to n_states
    bad_dfa(trans(ns * nc - 1, 0xFFFF))
    bad_dfa(lambda d: d.class_map.__setitem__(200, nc))              # a class equal to n_classes
    bad_dfa(None, rec(6, lambda n: n))                               # slices that end past the blob
    bad_dfa(None, rec(4, lambda n: n - 255))
    bad_dfa(None, rec(5, lambda n: (n - 2 * ns * nc + 2) & ~1))
    bad_dfa(None, rec(5, 0xFFFFFFFE))
    bad_dfa(None, None, pad=1)                                       # an odd trans_off
    bad_dfa(trans(0, 1))                                             # row 0 leaves the dead state
    bad_dfa(trans(nc - 1, 1))
    bad_dfa(lambda d: d.accept.__setitem__(0, d.accept[0] | 1))      # state 0 accepts
    bad_dfa(None, rec(2, 1))
    bad_dfa(None, rec(2, 65536))
    bad_dfa(None, rec(3, 0))
    bad_dfa(None, rec(3, 257))
    # clearing: nothing is launched any more
    assert _load(eng, [], [], b"") == 0 and _counts(eng) == (0, 0)
    rc, rows = _raw_match(eng, off, ln, pblob.tobytes(), 1)
    assert rc == 0 and (rows == ONES).all()
    eng.close()


def test_a_table_too_big_for_lds_walks_global_memory_to_the_same_answers():
    """The same definitions behind a blob padded past the staging limit."""
    eng, s, m = _sentinel(MATCH_NAMES, MATCH_DEFS)
    paths = _match_corpus()
    want = m.match(paths, host_bits=None)
    d = GR.compile_dfa(r"/r/\d+")
    blob = bytearray(70000)
    rows = [_dfa_row(2, d, blob), [0, K.SGA_GW_API_EXACT, len(blob), 1]]
    blob += b"/"
    assert _load(eng, rows, list(range(len(MATCH_NAMES))), blob) == 0
    off, ln, pblob = A.pack_paths(paths)
    rc, got = _raw_match(eng, off, ln, pblob.tobytes(), 1)
    assert rc == 0
    for i, v in enumerate(paths):
        exp = ([] if v != "/" else ["exacts"]) + (["regex"] if v is not None and gt.re.fullmatch(r"/r/\d+", v) else [])
        assert _names_of(got[i], MATCH_NAMES) == exp, v
    assert got.any() and want.any()
    eng.close()


def test_a_path_slice_past_the_blob_zeroes_its_row_and_is_reported():
    import torch
    eng, s, m = _sentinel(["a"], [_api("a", ("/**", 1), ("", 2))])
    off, ln = [0, 2, 4, 6], [2, 2, 3, 0]  # request 2 ends one byte past the blob; an empty slice at its end is fine
    rc, rows = _raw_match(eng, off, ln, b"/a/b/c", 1)
    assert rc == K.SGA_EINVAL and rows[:, 0].tolist() == [1, 1, 0, 0]
    dev = torch.device("cuda", eng.device)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731
    d_match = torch.full((4,), -1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    m.match_device(t(np.array(off, np.int32)), t(np.array(ln, np.int32)), t(np.frombuffer(b"/a/b/c", np.uint8)), d_match)
    with pytest.raises(_lib.EngineError):
        s.device_status()
    s.device_status()  # reported once
    assert d_match.cpu().numpy().tolist() == [1, 1, 0, 0]
    eng.close()


# ---- 5. end to end
E2E_NAMES = ["route0", "route1", "api_a", "api_b", "api_c", "plain"]
E2E_DEFS = [_api("api_a", ("/a/**", 1), ("/both", 0)), _api("api_b", (r"/b/\d+", 2), ("/both", 0)),
            _api("api_c", ("/**/c", 1))]
E2E_RULES = [
    gt.rule(resource="route0", count=3, item={"parse_strategy": 0}),
    gt.rule(resource="route1", count=4),
    gt.rule(resource="api_a", resource_mode=1, count=2, item={"parse_strategy": 2, "field_name": "X-Tier"}),
    gt.rule(resource="api_b", resource_mode=1, count=50, control_behavior=2, max_queueing_timeout_ms=300),
    gt.rule(resource="api_c", resource_mode=0, count=1, item={"parse_strategy": 0}),  # a route-mode rule on an API
]
E2E_PATHS = ["/a/1", "/both", "/b/7", "/a/x/c", "/nothing", "/b/x", "/c", None]


def _e2e_sentinel():
    eng = _engine(1 << 12)
    s = LocalSentinel(eng, E2E_NAMES)
    g = G.GatewayRuleManager(s)
    g.load_rules([gt.to_product(r) for r in E2E_RULES])
    m = A.GatewayApiDefinitionManager(s)
    m.load_api_definitions(E2E_DEFS)
    return eng, s, g, m


def test_front_end_chain_on_the_device_decides_like_the_host_chain():
    import torch
    rng = np.random.default_rng(3)
    n = 48
    paths = [E2E_PATHS[i % len(E2E_PATHS)] for i in range(n)]
    routes = [None if i % 7 == 6 else f"route{i % 2}" for i in range(n)]
    rqs = [{("client_ip", ""): f"10.0.0.{rng.integers(0, 3)}", ("header", "X-Tier"): f"t{rng.integers(0, 2)}"}
           for _ in range(n)]
    # the host chain: the entry list from matching_apis_one, GatewayRuleManager.parse, submit
    eng, s, g, m = _e2e_sentinel()
    ent = [(i, s.ids[routes[i]], 0) for i in range(n) if routes[i] is not None]
    ent = sorted(ent + [(i, s.ids[name], 1) for i in range(n) for name in m.matching_apis_one(paths[i])],
                 key=lambda e: (e[0], e[2]))  # stable: the route first, the APIs in definition order
    res = np.array([e[1] for e in ent], np.uint32)
    mode = np.array([e[2] for e in ent], np.uint8)
    ne = len(ent)
    assert ne > n and len({e[1] for e in ent}) == 5
    f, p, vals = g.parse(res, mode, [rqs[e[0]] for e in ent])
    kind, ts, acq = np.zeros(ne, np.uint8), np.full(ne, T0, np.int64), np.ones(ne, np.int32)
    want = s.submit(kind, res, ts, acq, f, None, p, vals)
    assert (want[0] == 0).sum() > 5 and (want[0] == 2).sum() > 5 and (want[1] > 0).sum() > 2
    eng.close()
    # the device chain: match_device, expand_device with the gather, parse_device, the device entry
    eng, s, g, m = _e2e_sentinel()
    dev = torch.device("cuda", eng.device)
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731
    off, ln, blob = A.pack_paths(paths)
    fo, fl, fblob = G.pack_requests(rqs, g.fields())
    nf = len(g.fields())
    cap = n * 4
    i32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)  # noqa: E731
    d_match = torch.zeros(n * m.words, dtype=torch.int64, device=dev)
    d_flags = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_param = torch.zeros(cap, dtype=torch.int64, device=dev)
    d_vals = torch.zeros(2 * g.max_args * cap, dtype=torch.int64, device=dev)
    src, pos, d_res, d_total, ts_off = i32(cap), i32(cap), i32(cap), i32(1), i32(ne)
    d_mode = torch.zeros(cap, dtype=torch.uint8, device=dev)
    fo_out, fl_out = i32(cap * nf), i32(cap * nf)
    d_routes = t(np.array([NULL if r is None else s.ids[r] for r in routes], np.uint32).view(np.int32))
    d_off, d_ln, d_blob, d_fo, d_fl, d_fblob = (t(off.view(np.int32)), t(ln.view(np.int32)), t(blob),
                                                t(fo.view(np.int32)), t(fl.view(np.int32)), t(fblob))
    d_kind, d_acq = t(kind), t(acq)
    torch.cuda.synchronize(dev)  # every buffer is filled before the engine's stream touches it
    m.match_device(d_off, d_ln, d_blob, d_match)
    m.expand_device(d_routes, d_match, cap, src, pos, d_res, d_mode, d_total, field_off=d_fo, field_len=d_fl,
                    n_fields=nf, field_off_out=fo_out, field_len_out=fl_out)
    s.device_status()
    total = int(d_total.item())
    assert total == ne
    assert (d_res[:ne].cpu().numpy().view(np.uint32) == res).all() and (d_mode[:ne].cpu().numpy() == mode).all()
    assert src[:ne].cpu().numpy().tolist() == [e[0] for e in ent]
    g.parse_device(d_res[:ne], d_mode[:ne], fo_out[:ne * nf], fl_out[:ne * nf], d_fblob, d_flags[:ne], d_param[:ne],
                   d_vals[:2 * g.max_args * ne])
    dec, wait = s.submit_device(d_kind, d_res[:ne], T0, ts_off, d_acq, d_flags[:ne], None, d_param[:ne],
                                d_vals[:2 * g.max_args * ne])
    s.device_status()
    got = (dec.cpu().numpy(), wait.cpu().numpy())
    bad = np.nonzero((got[0] != want[0]) | (got[1] != want[1]))[0]
    assert not len(bad), [(int(i), E2E_NAMES[res[i]], int(mode[i]), (int(got[0][i]), int(got[1][i])),
                           (int(want[0][i]), int(want[1][i]))) for i in bad[:12]]
    eng.close()


def test_gateway_request_stops_at_the_first_block():
    eng, s, g, m = _e2e_sentinel()
    g.load_rules([gt.to_product(r) for r in (gt.rule(resource="api_a", resource_mode=1, count=1),
                                             gt.rule(resource="api_b", resource_mode=1, count=5))])
    rq = {("client_ip", ""): "1.1.1.1"}
    entries, block = s.gateway_request("route0", "/both", rq, T0)
    assert block is None and [e.rid for e in entries] == [s.ids[k] for k in ("route0", "api_a", "api_b")]
    entries2, block = s.gateway_request("route0", "/both", rq, T0 + 1)
    assert isinstance(block, BlockException) and [e.rid for e in entries2] == [s.ids["route0"]]
    view = {name: s.node(s.ids[name], T0 + 2) for name in E2E_NAMES}
    assert (view["route0"].total_pass, view["api_a"].total_pass, view["api_a"].total_block) == (2, 1, 1)
    assert (view["api_b"].total_pass, view["api_b"].total_block) == (1, 0)  # no later entry was made
    # a blank route enters the APIs only; a path nobody claims enters the route only
    entries3, block = s.gateway_request("  ", "/b/9", rq, T0 + 2)
    assert block is None and [e.rid for e in entries3] == [s.ids["api_b"]]
    entries4, block = s.gateway_request("route1", "/nothing", rq, T0 + 2)
    assert block is None and [e.rid for e in entries4] == [s.ids["route1"]]
    for e in entries + entries2 + entries3 + entries4:
        e.exit(T0 + 3)
    eng.close()


# ---- 6. the command center
def test_update_then_get_api_definitions():
    from urllib.parse import quote
    eng, s, m = _sentinel(["some_customized_api", "another_customized_api"], [])
    cc = CC.CommandCenter(s, {"gateway_api": m})
    data = [{"apiName": "some_customized_api", "predicateItems": [{"pattern": "/product/**", "matchStrategy": 1}]},
            {"apiName": "another_customized_api",
             "predicateItems": [{"pattern": "/something", "matchStrategy": 0}, {"pattern": "/other/**", "matchStrategy": 1}]}]
    assert cc.handle("gateway/updateApiDefinitions", {"data": quote(json.dumps(data))}) == (True, "success")
    ok, text = cc.handle("gateway/getApiDefinitions", {})
    assert ok and json.loads(text) == data
    assert _counts(eng) == (2, 3)
    assert m.match(["/product/123", "/products", "/something", "/other/foo/3"])[:, 0].tolist() == [1, 0, 2, 2]
    assert cc.handle("gateway/updateApiDefinitions", {"data": " "}) == (False, "Bad data")
    assert _counts(eng) == (2, 3)
    eng.close()
