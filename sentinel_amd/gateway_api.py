"""Gateway API groups: which ApiDefinitions a request path enters, for one request on the host and a batch on the GPU.

GW = sentinel-adapter/sentinel-api-gateway-adapter-common/src/main/java/com/alibaba/csp/sentinel/adapter/gateway/common
  ApiDefinition, ApiPathPredicateItem     GW/api/ApiDefinition.java, ApiPathPredicateItem.java
  URL_MATCH_STRATEGY_*                    GW/SentinelGatewayConstants.java:35-37
  GatewayApiDefinitionManager             GW/api/GatewayApiDefinitionManager.java:86-151
  AbstractApiMatcher                      GW/api/matcher/AbstractApiMatcher.java:45-49 (a constructor that swallows
                                          what initializeMatchers throws), :60-70 (test: any matcher)
  RequestContextApiMatcher                sentinel-zuul-adapter .../api/matcher/RequestContextApiMatcher.java:58-71 ->
                                          predicates_of (the SCG and zuul2 twins are the same)
  PrefixRoutePathMatcher                  sentinel-zuul-adapter .../api/route/PrefixRoutePathMatcher.java: matches only
                                          a pattern with a wildcard (isPattern) -- restated as written
  the filters                             SentinelZuulPreFilter.run:118-134 and its twins: the route id, then every
                                          matching API name -> LocalSentinel.gateway_request (one request),
                                          match / expand (a batch: sga_gateway_api_*)

Spring's AntPathMatcher is not part of the reference tree; the adapters call it with its defaults (separator "/", case
sensitive, no token trimming).  ant_match restates its documented algorithm; parity beyond the cases the tests list is
unpinned -- among them `{...}` URI variables (here literal braces), whether `?` and `*` cross a line terminator (here
they do) and whether a `{...}` pair alone makes a pattern a pattern (here it does).

Orders the reference leaves to a HashSet are list order here (parity-unpinned): the predicates of a definition --
which matters only for a REGEX item `re` cannot compile, whose exception ends the definition's matcher list where it
stands -- and the APIs of one request, which the device lists in table order.
"""
import ctypes as C
import re
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from . import _lib, gateway_regex
from ._lib import (SGA_GW_API_DFA, SGA_GW_API_EXACT, SGA_GW_API_HOST, SGA_GW_API_MAX, SgaGatewayApiPred, check)
from .gateway import FIELD_NULL, RESOURCE_MODE_CUSTOM_API_NAME, RESOURCE_MODE_ROUTE_ID, _blank

URL_MATCH_STRATEGY_EXACT = 0
URL_MATCH_STRATEGY_PREFIX = 1
URL_MATCH_STRATEGY_REGEX = 2
MAX_HOST_PREDICATES = 64  # the bits of the per-request host word
ROUTE_NULL = FIELD_NULL   # SGA_GW_NULL as a route id: the request enters no route


@dataclass
class ApiPathPredicateItem:
    pattern: Optional[str] = None
    match_strategy: int = URL_MATCH_STRATEGY_EXACT


@dataclass
class ApiDefinition:
    api_name: Optional[str] = None
    predicate_items: Optional[list] = None


def is_valid_api(d: Optional[ApiDefinition]) -> bool:
    """GatewayApiDefinitionManager.isValidApi (:147-150)."""
    return d is not None and not _blank(d.api_name) and d.predicate_items is not None


# ---- AntPathMatcher, default settings
def _tokens(s: str) -> List[str]:
    return [t for t in s.split("/") if t]


def ant_is_pattern(pattern: str) -> bool:
    """AntPathMatcher.isPattern: a `*`, a `?`, or a `{` with a `}` after it."""
    brace = False
    for c in pattern:
        if c in "*?":
            return True
        if c == "{":
            brace = True
        elif c == "}" and brace:
            return True
    return False


def _token_match(pat: str, s: str) -> bool:
    """One path token against one pattern token: `?` one character, `*` any run, everything else itself."""
    rx = "".join("." if c == "?" else ".*" if c == "*" else re.escape(c) for c in pat)
    return re.fullmatch(rx, s, re.S) is not None


def ant_match(pattern: str, path: str) -> bool:
    """AntPathMatcher.match(pattern, path) (doMatch with fullMatch) restated from its documented algorithm."""
    if path.startswith("/") != pattern.startswith("/"):
        return False
    pat, seg = _tokens(pattern), _tokens(path)
    p0, p1, s0, s1 = 0, len(pat) - 1, 0, len(seg) - 1
    while p0 <= p1 and s0 <= s1:  # up to the first **
        if pat[p0] == "**":
            break
        if not _token_match(pat[p0], seg[s0]):
            return False
        p0 += 1
        s0 += 1
    if s0 > s1:  # the path is exhausted
        if p0 > p1:
            return pattern.endswith("/") == path.endswith("/")
        if p0 == p1 and pat[p0] == "*" and path.endswith("/"):
            return True
        return all(t == "**" for t in pat[p0:p1 + 1])
    if p0 > p1:
        return False  # the pattern is exhausted, the path is not
    while p0 <= p1 and s0 <= s1:  # from the end back to the last **
        if pat[p1] == "**":
            break
        if not _token_match(pat[p1], seg[s1]):
            return False
        p1 -= 1
        s1 -= 1
    if s0 > s1:
        return all(t == "**" for t in pat[p0:p1 + 1])
    while p0 != p1 and s0 <= s1:  # between two **: the first place the tokens between them fit
        nxt = next((i for i in range(p0 + 1, p1 + 1) if pat[i] == "**"), -1)
        if nxt == p0 + 1:
            p0 += 1  # **/**
            continue
        plen, slen = nxt - p0 - 1, s1 - s0 + 1
        found = -1
        for i in range(slen - plen + 1):
            if all(_token_match(pat[p0 + j + 1], seg[s0 + i + j]) for j in range(plen)):
                found = s0 + i
                break
        if found < 0:
            return False
        p0, s0 = nxt, found + plen
    return all(t == "**" for t in pat[p0:p1 + 1])


_RX_META = set(".^$*+?{}[]\\|()")
_SEG = "[^/]"


def _token_regex(tok: str) -> str:
    if set(tok) == {"*"}:
        return _SEG + "+"  # a path token is never empty
    out, prev_star = [], False
    for c in tok:
        if c == "*":
            if not prev_star:
                out.append(_SEG + "*")
            prev_star = True
            continue
        prev_star = False
        out.append(_SEG if c == "?" else "\\" + c if c in _RX_META else c)
    return "".join(out)


def ant_to_regex(pattern: str) -> Optional[str]:
    """The language ant_match(pattern, .) accepts as a regular expression of the subset gateway_regex.compile_dfa
    takes, or None -- declined, the predicate stays on the host -- for a pattern that does not start with "/", holds
    `{` or `}`, or holds a character the compiler's subset has no plain spelling for.  It never guesses.

    A plain token is `/+` and its segment (`?` -> [^/], `*` -> [^/]*, a token of nothing but `*` -> [^/]+); a `**`
    token is (?:/+[^/]+)*.  With a `**` any run of slashes may follow.  Without one, a slash run follows iff the
    pattern ends in "/"; and when the last token is exactly `*`, the path may instead end in a slash run where that
    token would stand (the matcher's "one `*` left and the path ends in /")."""
    if not pattern.startswith("/") or "{" in pattern or "}" in pattern:
        return None
    if any(ord(c) < 0x20 or 0xD800 <= ord(c) <= 0xDFFF for c in pattern):
        return None
    toks = _tokens(pattern)
    if not toks:
        return "/+"
    if all(t == "**" for t in toks):
        return "/+(?:" + _SEG + "+/+)*(?:" + _SEG + "+)?"
    parts = ["(?:/+" + _SEG + "+)*" if t == "**" else "/+" + _token_regex(t) for t in toks]
    if "**" in toks:
        return "".join(parts) + "/*"
    full = "".join(parts) + ("/+" if pattern.endswith("/") else "")
    if toks[-1] == "*":
        return "(?:" + full + "|" + "".join(parts[:-1]) + "/+)"
    return full


# ---- a definition's matchers
@dataclass(eq=False)
class Predicate:
    """One matcher of a definition.  kind: "exact", "regex", "ant", or "never" (a PREFIX pattern without a wildcard).
    where: "device" or "host" once a manager placed it; bit: its bit of the host word."""
    kind: str
    pattern: str
    compiled: object = None
    where: str = "host"
    bit: int = -1
    dfa: object = field(default=None, repr=False)


def predicates_of(d: ApiDefinition) -> List[Predicate]:
    """RequestContextApiMatcher.initializeMatchers in list order.  A blank pattern gives none; REGEX is
    Pattern.matches (re.fullmatch); PREFIX the Ant matcher, which answers only for a pattern with a wildcard; every
    other strategy is EXACT.  A REGEX pattern that does not compile throws in the reference and the constructor keeps
    the matchers made so far: that item and the later ones are dropped."""
    out: List[Predicate] = []
    for it in d.predicate_items or []:
        if not isinstance(it, ApiPathPredicateItem) or _blank(it.pattern):
            continue
        if it.match_strategy == URL_MATCH_STRATEGY_REGEX:
            try:
                out.append(Predicate("regex", it.pattern, re.compile(it.pattern)))
            except (re.error, RecursionError, OverflowError):
                break
        elif it.match_strategy == URL_MATCH_STRATEGY_PREFIX:
            out.append(Predicate("ant" if ant_is_pattern(it.pattern) else "never", it.pattern))
        else:
            out.append(Predicate("exact", it.pattern))
    return out


def pack_paths(paths: Sequence[Optional[str]]):
    """(path_off, path_len, blob) of sga_gateway_api_match: uint32 arrays and the UTF-8 bytes; None has length
    FIELD_NULL."""
    off = np.zeros(len(paths), dtype=np.uint32)
    ln = np.full(len(paths), FIELD_NULL, dtype=np.uint32)
    blob = bytearray()
    for i, p in enumerate(paths):
        if p is None:
            continue
        b = p.encode("utf-8")
        off[i], ln[i] = len(blob), len(b)
        blob += b
    if len(blob) >= 1 << 32:
        raise ValueError("request paths of one batch exceed 4 GiB")
    return off, ln, np.frombuffer(bytes(blob), dtype=np.uint8)


class GatewayApiDefinitionManager:
    """GatewayApiDefinitionManager of one LocalSentinel.  load_api_definitions keeps the valid definitions and loads
    the engine's table (sga_gateway_api_load): one column per definition whose name is a registered resource of the
    sentinel, in definition order -- a definition of another name is kept and listed but has no column, like a rule
    of a resource nobody enters."""

    def __init__(self, sentinel, device: bool = True, ant_host: Callable[[str, str], bool] = ant_match,
                 regex_max_states: int = gateway_regex.MAX_STATES,
                 regex_max_table_bytes: int = gateway_regex.MAX_TABLE_BYTES):
        """device: compile PREFIX and REGEX predicates into byte DFAs the match kernel walks; what the compilers
        decline -- and with device=False every PREFIX and REGEX predicate -- is a host predicate: host_bits answers it
        with re.fullmatch or ant_host(pattern, path) and hands it over as a bit.  ant_host: the caller's Ant matcher
        (one that knows `{...}` variables, say); the default treats braces as literals."""
        self.s = sentinel
        sentinel._gateway_api = self
        self.device = bool(device)
        self.ant_host = ant_host
        self.regex_max_states, self.regex_max_table_bytes = regex_max_states, regex_max_table_bytes
        self._defs: Dict[str, ApiDefinition] = {}
        self._preds: Dict[str, List[Predicate]] = {}
        self._columns: List[str] = []  # API index -> name
        self._host: List[Predicate] = []
        self._table = False  # the engine holds a table
        self._sent = None

    is_valid_api = staticmethod(is_valid_api)

    def get_api_definitions(self) -> List[ApiDefinition]:
        return list(self._defs.values())

    def get_api_definition(self, name: Optional[str]) -> Optional[ApiDefinition]:
        return None if name is None else self._defs.get(name)

    def columns(self) -> List[str]:
        """The API names of the bitmap's bits, in order."""
        return list(self._columns)

    @property
    def words(self) -> int:
        return (len(self._columns) + 63) // 64

    def load_api_definitions(self, definitions) -> bool:
        """applyApiUpdateInternal: an empty or None set clears; a later definition of a name replaces the earlier."""
        defs: Dict[str, ApiDefinition] = {}
        for d in definitions or []:
            if is_valid_api(d):
                defs[d.api_name] = d
        preds = {name: predicates_of(d) for name, d in defs.items()}
        columns = [name for name in defs if name in self.s.ids]
        if len(columns) > SGA_GW_API_MAX:
            raise ValueError(f"{len(columns)} API definitions; the engine serves {SGA_GW_API_MAX}")
        blob = bytearray()
        rows, host = [], []
        dfas: Dict[tuple, object] = {}
        where: Dict[tuple, tuple] = {}
        for k, name in enumerate(columns):
            for p in preds[name]:
                if p.kind == "never":
                    continue
                if p.kind == "exact":
                    b = p.pattern.encode("utf-8")
                    rows.append((k, SGA_GW_API_EXACT, len(blob), len(b), 0, 0, 0))
                    blob += b
                    p.where = "device"
                    continue
                key = (p.kind, p.pattern)
                if self.device and key not in dfas:
                    rx = p.pattern if p.kind == "regex" else ant_to_regex(p.pattern)
                    dfas[key] = d = None if rx is None else gateway_regex.compile_dfa(
                        rx, max_states=self.regex_max_states, max_table_bytes=self.regex_max_table_bytes)
                    if d is not None:
                        blob += b"\0" * (len(blob) & 1)
                        t_off = len(blob)
                        blob += d.trans.tobytes()
                        where[key] = (len(blob), t_off, len(blob) + 256)
                        blob += d.class_map.tobytes() + d.accept.tobytes()
                d = dfas.get(key)
                if d is None:
                    if len(host) >= MAX_HOST_PREDICATES:
                        raise ValueError(f"more than {MAX_HOST_PREDICATES} predicates stay on the host")
                    p.where, p.bit = "host", len(host)
                    rows.append((k, SGA_GW_API_HOST, p.bit, 0, 0, 0, 0))
                    host.append(p)
                else:
                    p.where, p.dfa = "device", d
                    rows.append((k, SGA_GW_API_DFA, d.n_states, d.n_classes) + where[key])
        # unregistered definitions still answer matching_apis_one on the host
        for name in defs:
            if name not in columns:
                for p in preds[name]:
                    p.where = "host"
        arr = (SgaGatewayApiPred * max(1, len(rows)))()
        for a, row in zip(arr, rows):
            a.api, a.kind, a.a, a.b, a.c, a.d, a.e = row
        res = np.array([self.s.ids[name] for name in columns], dtype=np.uint32)
        buf = (C.c_uint8 * max(1, len(blob))).from_buffer_copy(bytes(blob) or b"\0")
        h = self.s.engine.handle
        check(_lib.load().sga_gateway_api_load(h, arr, len(rows), res.ctypes.data if len(res) else None, len(res), buf,
                                               len(blob)), h, "GatewayApiDefinitionManager.loadApiDefinitions")
        self._defs, self._preds, self._columns, self._host = defs, preds, columns, host
        self._table = bool(rows)
        self._sent = (arr, len(rows), res, buf, len(blob))  # the table as the engine got it
        return True

    def host_predicates(self) -> List[tuple]:
        """(api name, bit, kind, pattern) of the predicates host_bits answers."""
        by_pred = {id(p): name for name, lst in self._preds.items() for p in lst}
        return [(by_pred[id(p)], p.bit, p.kind, p.pattern) for p in self._host]

    def _test(self, p: Predicate, path: str) -> bool:
        if p.kind == "exact":
            return path == p.pattern
        if p.kind == "regex":
            return p.compiled.fullmatch(path) is not None
        if p.kind == "ant":
            return bool(self.ant_host(p.pattern, path))
        return False

    def matching_apis_one(self, path: Optional[str]) -> List[str]:
        """pickMatchingApiDefinitions for one path, on the host: the matching names in definition order."""
        if path is None:
            return []
        return [name for name, lst in self._preds.items() if any(self._test(p, path) for p in lst)]

    def host_bits(self, paths: Sequence[Optional[str]]) -> Optional[np.ndarray]:
        """One uint64 per request: bit j = host predicate j matches the path.  None when no predicate is on the
        host."""
        if not self._host:
            return None
        bits = np.zeros(len(paths), dtype=np.uint64)
        for i, path in enumerate(paths):
            if path is None:
                continue
            w = 0
            for p in self._host:
                if self._test(p, path):
                    w |= 1 << p.bit
            bits[i] = w
        return bits

    def _need_table(self):
        if not self._table:
            raise ValueError("no API table is loaded (no registered definition has a predicate)")

    # ---- batches
    def match(self, paths: Sequence[Optional[str]], host_bits="auto") -> np.ndarray:
        """sga_gateway_api_match: the (n, words) uint64 bitmap of `paths` (str or None).  host_bits: "auto" fills
        the host word with host_bits(paths); None hands none over (host predicates then do not match)."""
        self._need_table()
        off, ln, blob = pack_paths(paths)
        hb = self.host_bits(paths) if isinstance(host_bits, str) else host_bits
        if hb is not None:
            hb = np.ascontiguousarray(hb, dtype=np.uint64)
        out = np.zeros((len(paths), self.words), dtype=np.uint64)
        h = self.s.engine.handle
        check(_lib.load().sga_gateway_api_match(h, off.ctypes.data, ln.ctypes.data,
                                                blob.ctypes.data if len(blob) else None, len(blob),
                                                hb.ctypes.data if hb is not None else None, len(paths),
                                                out.ctypes.data), h, "gatewayApiMatch")
        return out

    def match_device(self, path_off, path_len, blob, match, host_bits=None, stream=None):
        """sga_gateway_api_match_device over torch tensors on the engine's GPU, asynchronous on `stream`: one chunk
        of at most max_batch requests; match (n x words, 64-bit) is written in place."""
        self._need_table()
        n = path_off.numel()
        for name, x, size in (("path_off", path_off, 4), ("path_len", path_len, 4), ("blob", blob, 1),
                              ("match", match, 8), ("host_bits", host_bits, 8)):
            if x is None:
                continue
            if not x.is_cuda or not x.is_contiguous() or x.element_size() != size:
                raise ValueError(f"{name}: a contiguous device tensor of {size}-byte elements expected")
        if path_len.numel() != n or match.numel() != n * self.words or \
                (host_bits is not None and host_bits.numel() != n):
            raise ValueError("gateway API tensors differ in length")
        h = self.s.engine.handle
        check(_lib.load().sga_gateway_api_match_device(
            h, path_off.data_ptr(), path_len.data_ptr(), blob.data_ptr() if blob.numel() else None, blob.numel(),
            host_bits.data_ptr() if host_bits is not None else None, n, match.data_ptr(),
            stream.cuda_stream if stream is not None else None), h, "gatewayApiMatchDevice")
        return match

    def expand(self, routes, match, field_off=None, field_len=None, n_fields: int = 0, cap: Optional[int] = None):
        """sga_gateway_api_expand: the entry list of a batch as a dict of numpy arrays -- src, pos, resource, mode,
        total, and field_off / field_len when the request field table (n x n_fields) is given.  routes: resource ids,
        ROUTE_NULL for a request without a route.  cap: room for entries (None: as many as needed); a smaller one
        raises ValueError naming the need."""
        self._need_table()
        r = np.ascontiguousarray(routes, dtype=np.uint32)
        m = np.ascontiguousarray(match, dtype=np.uint64).reshape(len(r), self.words)
        if cap is None:
            cap = int((r != ROUTE_NULL).sum()) + sum(bin(int(w)).count("1") for w in m.reshape(-1))
        gather = field_off is not None
        room = max(1, cap)
        out = {"src": np.zeros(room, np.uint32), "pos": np.zeros(room, np.uint32),
               "resource": np.zeros(room, np.uint32), "mode": np.zeros(room, np.uint8)}
        fo = fl = None
        if gather:
            fo = np.ascontiguousarray(field_off, dtype=np.uint32)
            fl = np.ascontiguousarray(field_len, dtype=np.uint32)
            if len(fo) != len(r) * n_fields or len(fl) != len(fo) or n_fields == 0:
                raise ValueError("the request field table is n x n_fields")
            out["field_off"] = np.zeros(room * n_fields, np.uint32)
            out["field_len"] = np.zeros(room * n_fields, np.uint32)
        total = C.c_size_t(0)
        h = self.s.engine.handle
        rc = _lib.load().sga_gateway_api_expand(
            h, r.ctypes.data, m.ctypes.data, len(r), fo.ctypes.data if gather else None,
            fl.ctypes.data if gather else None, n_fields if gather else 0, cap, out["src"].ctypes.data,
            out["pos"].ctypes.data, out["resource"].ctypes.data, out["mode"].ctypes.data,
            out["field_off"].ctypes.data if gather else None, out["field_len"].ctypes.data if gather else None,
            C.byref(total))
        if rc == _lib.SGA_ERANGE and total.value > cap:
            raise ValueError(f"gatewayApiExpand: {total.value} entries, room for {cap}")
        check(rc, h, "gatewayApiExpand")
        k = min(cap, total.value)
        out = {key: v[:k * n_fields] if key.startswith("field_") else v[:k] for key, v in out.items()}
        out["total"] = int(total.value)
        return out

    def expand_device(self, routes, match, cap: int, src, pos, resource, mode, total, field_off=None, field_len=None,
                      n_fields: int = 0, field_off_out=None, field_len_out=None, stream=None):
        """sga_gateway_api_expand_device over torch tensors, asynchronous on `stream`: one chunk of at most
        max_batch requests.  src / pos / resource (32-bit), mode (uint8) hold cap entries, total one 32-bit word; the
        four field tensors are given together or not at all."""
        self._need_table()
        n = routes.numel()
        sizes = (("routes", routes, 4, n), ("match", match, 8, n * self.words), ("src", src, 4, cap),
                 ("pos", pos, 4, cap), ("resource", resource, 4, cap), ("mode", mode, 1, cap), ("total", total, 4, 1),
                 ("field_off", field_off, 4, n * n_fields), ("field_len", field_len, 4, n * n_fields),
                 ("field_off_out", field_off_out, 4, cap * n_fields),
                 ("field_len_out", field_len_out, 4, cap * n_fields))
        for name, x, size, count in sizes:
            if x is None:
                continue
            if not x.is_cuda or not x.is_contiguous() or x.element_size() != size:
                raise ValueError(f"{name}: a contiguous device tensor of {size}-byte elements expected")
            if x.numel() < count:
                raise ValueError(f"{name}: {count} elements needed")
        ptr = (lambda x: x.data_ptr() if x is not None else None)
        h = self.s.engine.handle
        check(_lib.load().sga_gateway_api_expand_device(
            h, routes.data_ptr(), match.data_ptr(), n, ptr(field_off), ptr(field_len), int(n_fields), int(cap),
            src.data_ptr(), pos.data_ptr(), resource.data_ptr(), mode.data_ptr(), ptr(field_off_out),
            ptr(field_len_out), total.data_ptr(), stream.cuda_stream if stream is not None else None),
            h, "gatewayApiExpandDevice")
        return src, pos, resource, mode, total


def expected_entries(routes, match, api_resource, field_off=None, field_len=None, n_fields: int = 0):
    """The numpy model of the expansion: per request in input order the route entry (mode 0) unless the route is
    ROUTE_NULL, then one entry per set bit in ascending API index (mode 1)."""
    routes = np.asarray(routes, dtype=np.uint32)
    match = np.asarray(match, dtype=np.uint64).reshape(len(routes), -1) if len(routes) else np.zeros((0, 1), np.uint64)
    src, pos, res, mode = [], [], [], []
    for i, r in enumerate(routes.tolist()):
        q = 0
        if r != ROUTE_NULL:
            src.append(i), pos.append(q), res.append(r), mode.append(RESOURCE_MODE_ROUTE_ID)
            q += 1
        for w, word in enumerate(match[i].tolist()):
            while word:
                k = w * 64 + (word & -word).bit_length() - 1
                word &= word - 1
                src.append(i), pos.append(q), res.append(int(api_resource[k])), mode.append(
                    RESOURCE_MODE_CUSTOM_API_NAME)
                q += 1
    out = {"src": np.array(src, np.uint32), "pos": np.array(pos, np.uint32), "resource": np.array(res, np.uint32),
           "mode": np.array(mode, np.uint8), "total": len(src)}
    if field_off is not None:
        fo = np.asarray(field_off, np.uint32).reshape(len(routes), n_fields)
        fl = np.asarray(field_len, np.uint32).reshape(len(routes), n_fields)
        out["field_off"] = fo[out["src"].astype(np.int64)].reshape(-1)
        out["field_len"] = fl[out["src"].astype(np.int64)].reshape(-1)
    return out
