"""API-gateway flow control (sentinel-api-gateway-adapter-common) in front of the engine.

GW = sentinel-adapter/sentinel-api-gateway-adapter-common/src/main/java/com/alibaba/csp/sentinel/adapter/gateway/common
  GatewayFlowRule, GatewayParamFlowItem   GW/rule/GatewayFlowRule.java, GatewayParamFlowItem.java
  SentinelGatewayConstants                GW/SentinelGatewayConstants.java:26-49
  GatewayRuleManager.isValidRule          GW/rule/GatewayRuleManager.java:117-145
  applyGatewayRuleInternal                GW/rule/GatewayRuleManager.java:179-237 -> assign_indices
  GatewayRuleConverter                    GW/rule/GatewayRuleConverter.java:49-86 -> to_param_rule
  GatewayParamParser.parseParameterFor    GW/param/GatewayParamParser.java:51-174 -> GatewayRuleManager.parse_one (one
                                          request, on the host) / parse, parse_device (a batch, on the device:
                                          sga_gateway_parse, sga_gateway_parse_device)
  GatewayFlowSlot                         GW/slot/GatewayFlowSlot.java:36-71: ParamFlowChecker over the converted
                                          rules, ahead of ParamFlowSlot -> the converted rules lead the sentinel's
                                          parameter rule list

A gateway rule becomes a ParamFlowRule and a request an argument vector; the engine's ParamFlowSlot decides both.
What this module adds is the step before: per request and rule, pick a field, match it against the rule's pattern
and key the resulting string -- done for a whole batch by one kernel.

Orders the reference leaves to a HashSet are list order here (parity-unpinned): the index a rule gets, and -- for a
table loaded through the C ABI with two items on one index, which the manager never produces -- which of them
writes the slot (the later one).  REGEX patterns are evaluated on the host with
Python's `re` (re.fullmatch for Matcher.matches); the Java and Python dialects differ in places (possessive
quantifiers before Python 3.11, \\p{...} classes, inline-flag placement): a pattern Python cannot compile matches
everything, as a pattern Java cannot compile does in the reference.  A manager built with device_regex=True
compiles the patterns of a regular subset into byte DFAs (gateway_regex.py) that the parse kernel walks; those
items need no host pass and no regex_bits word, the rest keep it item by item.
"""
import ctypes as C
import re
from dataclasses import dataclass
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from . import _lib, gateway_regex
from ._lib import SgaGatewayItem, SgaGatewayRegex, check
from .rules import ParamFlowItem, ParamFlowRule, RuleConstant

RESOURCE_MODE_ROUTE_ID = 0
RESOURCE_MODE_CUSTOM_API_NAME = 1
PARAM_PARSE_STRATEGY_CLIENT_IP = 0
PARAM_PARSE_STRATEGY_HOST = 1
PARAM_PARSE_STRATEGY_HEADER = 2
PARAM_PARSE_STRATEGY_URL_PARAM = 3
PARAM_PARSE_STRATEGY_COOKIE = 4
PARAM_MATCH_STRATEGY_EXACT = 0
PARAM_MATCH_STRATEGY_PREFIX = 1
PARAM_MATCH_STRATEGY_REGEX = 2
PARAM_MATCH_STRATEGY_CONTAINS = 3
GATEWAY_NOT_MATCH_PARAM = "$NM"
GATEWAY_DEFAULT_PARAM = "$D"
NOT_MATCH_PASS_COUNT = 10_000_000  # GatewayRuleConverter.generateNonMatchPassParamItem
MAX_ARGS = 64                      # the engine's param_idx < 64
FIELD_NULL = 0xFFFFFFFF            # SGA_GW_NULL
_FIELD_REQUIRED = (PARAM_PARSE_STRATEGY_HEADER, PARAM_PARSE_STRATEGY_URL_PARAM, PARAM_PARSE_STRATEGY_COOKIE)
_FIELD_KIND = {PARAM_PARSE_STRATEGY_CLIENT_IP: "client_ip", PARAM_PARSE_STRATEGY_HOST: "host",
               PARAM_PARSE_STRATEGY_HEADER: "header", PARAM_PARSE_STRATEGY_URL_PARAM: "url_param",
               PARAM_PARSE_STRATEGY_COOKIE: "cookie"}


@dataclass(eq=False)  # no equals() in the reference: identity
class GatewayParamFlowItem:
    index: Optional[int] = None  # set by the manager (GatewayRuleConverter.applyToParamRule)
    parse_strategy: int = PARAM_PARSE_STRATEGY_CLIENT_IP
    field_name: Optional[str] = None
    pattern: Optional[str] = None
    match_strategy: int = PARAM_MATCH_STRATEGY_EXACT


@dataclass
class GatewayFlowRule:
    resource: Optional[str] = None
    resource_mode: int = RESOURCE_MODE_ROUTE_ID
    grade: int = RuleConstant.FLOW_GRADE_QPS
    count: float = 0.0
    interval_sec: int = 1
    control_behavior: int = RuleConstant.CONTROL_BEHAVIOR_DEFAULT
    burst: int = 0
    max_queueing_timeout_ms: int = 500
    param_item: Optional[GatewayParamFlowItem] = None


def _blank(s: Optional[str]) -> bool:
    return s is None or not s.strip()


def is_valid_param_item(item: GatewayParamFlowItem) -> bool:
    """GatewayRuleManager.isValidParamItem (:136-145)."""
    if item.parse_strategy < 0:
        return False
    if item.parse_strategy in _FIELD_REQUIRED and _blank(item.field_name):
        return False
    return not item.pattern or item.match_strategy >= 0


def is_valid_rule(rule: Optional[GatewayFlowRule]) -> bool:
    """GatewayRuleManager.isValidRule (:117-134).  Line 122 compares the *grade* with
    CONTROL_BEHAVIOR_RATE_LIMITER (2) before it looks at maxQueueingTimeoutMs: a throttling rule (controlBehavior 2,
    grade 1) with a negative timeout is valid, restated as written."""
    if (rule is None or _blank(rule.resource) or rule.resource_mode < 0 or rule.grade < 0 or rule.count < 0 or
            rule.burst < 0 or rule.control_behavior < 0):
        return False
    if rule.grade == RuleConstant.CONTROL_BEHAVIOR_RATE_LIMITER and rule.max_queueing_timeout_ms < 0:
        return False
    if rule.interval_sec <= 0:
        return False
    return rule.param_item is None or is_valid_param_item(rule.param_item)


def to_param_rule(rule: GatewayFlowRule, idx: int) -> ParamFlowRule:
    """GatewayRuleConverter.applyToParamRule / applyNonParamToParamRule: the rule's item (if any) gets idx; a
    pattern that is not null -- an empty one included -- adds the hot item {"$NM", String, 10,000,000}."""
    out = ParamFlowRule(resource=rule.resource, count=rule.count, grade=rule.grade,
                        duration_in_sec=rule.interval_sec, burst_count=rule.burst,
                        control_behavior=rule.control_behavior, max_queueing_time_ms=rule.max_queueing_timeout_ms,
                        param_idx=idx)
    item = rule.param_item
    if item is not None:
        item.index = idx
        if item.pattern is not None:
            out.param_flow_item_list.append(ParamFlowItem(GATEWAY_NOT_MATCH_PARAM, NOT_MATCH_PASS_COUNT,
                                                          "java.lang.String"))
    return out


def assign_indices(rules: Sequence[GatewayFlowRule]):
    """applyGatewayRuleInternal over `rules` in list order: (rule_map, converted) -- per resource the valid
    rules, and the converted ParamFlowRules (equal ones once): those of rules with a paramItem in list order, then
    those of the rules without.  The reference is handed a Set: a rule equal to an earlier one of the list counts
    once (GatewayFlowRule.equals; items compare by identity).  A resource's rules with a paramItem take indices 0,
    1, ...; the index advances only when the converted rule was new to the set (:207-209) -- which it always is,
    since paramIdx is part of ParamFlowRule.equals and no earlier rule of the resource carries the index in hand;
    the test is restated as written.  Every rule without a paramItem gets the next free index of its resource:
    they all share it."""
    rule_map: Dict[str, List[GatewayFlowRule]] = {}
    converted: Dict[str, List[ParamFlowRule]] = {}
    idx: Dict[str, int] = {}
    no_param: Dict[str, List[GatewayFlowRule]] = {}
    for rule in rules or []:
        if not is_valid_rule(rule):
            continue
        name = rule.resource
        seen = rule_map.setdefault(name, [])
        if rule in seen:
            continue
        seen.append(rule)
        if rule.param_item is None:
            no_param.setdefault(name, []).append(rule)
            continue
        i = idx.setdefault(name, 0)
        pr = to_param_rule(rule, i)
        have = converted.setdefault(name, [])
        if pr not in have:
            have.append(pr)
            idx[name] = i + 1
    for name, lst in no_param.items():
        for rule in lst:
            pr = to_param_rule(rule, idx.setdefault(name, 0))
            have = converted.setdefault(name, [])
            if pr not in have:
                have.append(pr)
    return rule_map, converted


def field_key(item: GatewayParamFlowItem) -> Tuple[str, str]:
    """What a front end extracts for an item: ("client_ip", ""), ("host", ""), ("header", name), ("url_param", name)
    or ("cookie", name).  Client IP and Host ignore fieldName; an unknown parse strategy names a field no request
    has (parseInternal's default: null)."""
    kind = _FIELD_KIND.get(item.parse_strategy)
    if kind is None:
        return (f"strategy{item.parse_strategy}", "")
    if item.parse_strategy in _FIELD_REQUIRED:
        return (kind, item.field_name)
    return (kind, "")


def request_field(request: Mapping, key: Tuple[str, str]) -> Optional[str]:
    """A request's value of a field; the Host strategy reads the "Host" header when the request has no host key."""
    v = request.get(key)
    if v is None and key == ("host", ""):
        v = request.get(("header", "Host"))
    return v


def _compile(pattern: str):
    try:
        return re.compile(pattern)
    except re.error:
        return None  # GatewayRegexCache holds no entry: the value is kept


def match_value(item: GatewayParamFlowItem, value: Optional[str]) -> Optional[str]:
    """parseWithMatchStrategyInternal behind the StringUtil.isEmpty(pattern) test of its callers (:86-174).
    PREFIX and every unknown strategy keep the value (the switch's default branch)."""
    if not item.pattern or value is None:
        return value
    if item.match_strategy == PARAM_MATCH_STRATEGY_EXACT:
        return value if value == item.pattern else GATEWAY_NOT_MATCH_PARAM
    if item.match_strategy == PARAM_MATCH_STRATEGY_CONTAINS:
        return value if item.pattern in value else GATEWAY_NOT_MATCH_PARAM
    if item.match_strategy == PARAM_MATCH_STRATEGY_REGEX:
        rx = _compile(item.pattern)
        return value if rx is None or rx.fullmatch(value) else GATEWAY_NOT_MATCH_PARAM
    return value


def pack_requests(requests: Sequence[Mapping], fields: Sequence[Tuple[str, str]]):
    """The request field table of sga_gateway_parse: (field_off, field_len, blob) -- uint32 arrays of
    len(requests) * len(fields) entries, row-major by request, and the UTF-8 bytes.  A missing field has length
    FIELD_NULL; the empty string has length 0."""
    n, nf = len(requests), len(fields)
    off = np.zeros(n * nf, dtype=np.uint32)
    ln = np.full(n * nf, FIELD_NULL, dtype=np.uint32)
    blob = bytearray()
    for i, rq in enumerate(requests):
        for k, key in enumerate(fields):
            v = request_field(rq, key)
            if v is None:
                continue
            b = v.encode("utf-8")
            off[i * nf + k] = len(blob)
            ln[i * nf + k] = len(b)
            blob += b
    if len(blob) >= 1 << 32:
        raise ValueError("request fields of one batch exceed 4 GiB")
    return off, ln, np.frombuffer(bytes(blob), dtype=np.uint8)


class GatewayRuleManager:
    """GatewayRuleManager of one LocalSentinel.  load_rules converts the rules, re-sends the sentinel's effective
    parameter rule list -- the converted gateway rules, in the order their resources first appear, then the rules
    last given to ParamFlowRuleManager -- and loads the parser's table (sga_gateway_load)."""

    def __init__(self, sentinel, device_regex: bool = False, regex_max_states: int = gateway_regex.MAX_STATES,
                 regex_max_table_bytes: int = gateway_regex.MAX_TABLE_BYTES):
        """device_regex: compile every REGEX item's pattern into a byte DFA at load_rules (gateway_regex.compile_dfa
        under the two caps) and have the parse kernel decide it; the items the compiler declines stay on the
        regex_bits word (regex_host_items).  False: every REGEX item follows the word, as a front end fills it."""
        self.s = sentinel
        sentinel._gateway = self
        self.device_regex = bool(device_regex)
        self.regex_max_states, self.regex_max_table_bytes = regex_max_states, regex_max_table_bytes
        self._sent = None  # what the engine's table was loaded from: put back when a program load is refused
        self._rules: List[GatewayFlowRule] = []
        self._rule_map: Dict[str, List[GatewayFlowRule]] = {}
        self._converted: Dict[str, List[ParamFlowRule]] = {}
        self._fields: List[Tuple[str, str]] = []
        self._slots: Dict[int, list] = {}  # resource id -> per argument slot: the item, None, or "$D"
        self._regex: Dict[int, object] = {}  # id(item) -> compiled pattern (None: does not compile) of REGEX items
        self.max_args = 0

    is_valid_rule = staticmethod(is_valid_rule)

    def get_rules(self) -> List[GatewayFlowRule]:
        """Every valid rule of the last load (GatewayRuleManager.getRules), resources in first-appearance order."""
        return [r for lst in self._rule_map.values() for r in lst]

    def get_rules_for_resource(self, name: str) -> List[GatewayFlowRule]:
        return [] if _blank(name) else list(self._rule_map.get(name, []))

    def get_converted_param_rules(self, name: str) -> List[ParamFlowRule]:
        return [] if _blank(name) else list(self._converted.get(name, []))

    def converted_rules(self) -> List[ParamFlowRule]:
        """The head of the sentinel's effective parameter rule list."""
        return [r for lst in self._converted.values() for r in lst]

    def fields(self) -> List[Tuple[str, str]]:
        """The distinct (kind, name) pairs the loaded rules read, in first-appearance order: the columns of the
        request field table, and the list of things a front end extracts from each request."""
        return list(self._fields)

    def load_rules(self, rules: Sequence[GatewayFlowRule]) -> int:
        rules = list(rules or [])
        for r in rules:
            if getattr(r, "cluster_mode", False):
                raise ValueError("cluster-mode gateway rules do not exist in the reference: refused")
        rule_map, converted = assign_indices(rules)
        fields: List[Tuple[str, str]] = []
        slots: Dict[int, list] = {}
        items = []
        for name, lst in rule_map.items():
            with_item = [r for r in lst if r.param_item is not None]
            nargs = len(with_item) + (1 if len(with_item) < len(lst) else 0)
            if nargs > MAX_ARGS:
                raise ValueError(f"gateway rules of {name!r} need {nargs} arguments; the engine serves {MAX_ARGS} "
                                 f"(param_idx < {MAX_ARGS})")
            rid = self.s.ids.get(name)
            if rid is None:
                continue  # applies to nothing, like a rule of a resource nobody enters
            row: list = [None] * nargs
            for r in lst:
                it = r.param_item
                if it is None:
                    row[nargs - 1] = GATEWAY_DEFAULT_PARAM
                    items.append((rid, r, None))
                    continue
                key = field_key(it)
                if key not in fields:
                    fields.append(key)
                row[it.index] = (r, it)
                items.append((rid, r, fields.index(key)))
            slots[rid] = row
        arr = (SgaGatewayItem * max(1, len(items)))()
        blob = bytearray()
        for a, (rid, r, col) in zip(arr, items):
            a.resource = rid
            a.resource_mode = r.resource_mode
            a.index = -1
            if col is None:
                continue
            it = r.param_item
            a.index = it.index
            a.field = col
            a.match_strategy = it.match_strategy
            if it.pattern:
                pb = it.pattern.encode("utf-8")
                a.has_pattern, a.pattern_off, a.pattern_len = 1, len(blob), len(pb)
                blob += pb
        # the table first: a refused table leaves the manager, the engine's table and its parameter rules as they were
        pat = (C.c_uint8 * max(1, len(blob))).from_buffer_copy(bytes(blob) or b"\0")
        table = (arr, len(items), pat, len(blob), len(fields))
        programs = self._compile_programs(items) if self.device_regex else None
        L, h = _lib.load(), self.s.engine.handle
        check(L.sga_gateway_load(h, *table), h, "GatewayRuleManager.loadRules")
        if programs is not None and programs[1]:
            rc = L.sga_gateway_load_regex(h, *programs[:4])
            if rc < 0:  # the engine goes back to the table the manager still describes
                old_table, old_programs = self._sent or (((SgaGatewayItem * 1)(), 0, None, 0, 0), None)
                L.sga_gateway_load(h, *old_table)
                if old_programs is not None and old_programs[1]:
                    L.sga_gateway_load_regex(h, *old_programs[:4])
                check(rc, h, "GatewayRuleManager.loadRules (REGEX programs)")
        self._sent = (table, programs)
        on_device = programs[4] if programs is not None else set()
        self._rules, self._rule_map, self._converted = rules, rule_map, converted
        self._fields, self._slots = fields, slots
        from .local import send_param_rules
        send_param_rules(self.s)
        self.max_args = max((len(v) for v in slots.values()), default=0)
        self._regex = {id(it): _compile(it.pattern) for row in slots.values() for e in row
                       if isinstance(e, tuple) for it in [e[1]]
                       if it.pattern and it.match_strategy == PARAM_MATCH_STRATEGY_REGEX and id(it) not in on_device}
        return len(self.get_rules())

    def _compile_programs(self, items):
        """The arguments of sga_gateway_load_regex for a table's items -- (programs, n, blob, blob_len) -- and the
        ids of the items they decide.  One table per distinct pattern: items that share a pattern share its slices."""
        dfas: Dict[str, object] = {}
        where: Dict[str, Tuple[int, int, int]] = {}
        blob = bytearray()
        rows, on_device = [], set()
        for j, (rid, r, col) in enumerate(items):
            it = r.param_item
            if col is None or not it.pattern or it.match_strategy != PARAM_MATCH_STRATEGY_REGEX:
                continue
            if it.pattern not in dfas:
                dfas[it.pattern] = d = gateway_regex.compile_dfa(it.pattern, max_states=self.regex_max_states,
                                                                 max_table_bytes=self.regex_max_table_bytes)
                if d is not None:
                    blob += b"\0" * (len(blob) & 1)
                    t_off = len(blob)
                    blob += d.trans.tobytes()
                    where[it.pattern] = (len(blob), t_off, len(blob) + 256)
                    blob += d.class_map.tobytes() + d.accept.tobytes()
            d = dfas[it.pattern]
            if d is None:
                continue
            rows.append((j, d.n_states, d.n_classes) + where[it.pattern])
            on_device.add(id(it))
        arr = (SgaGatewayRegex * max(1, len(rows)))()
        for a, row in zip(arr, rows):
            a.item, a.n_states, a.n_classes, a.class_off, a.trans_off, a.accept_off = row
        buf = (C.c_uint8 * max(1, len(blob))).from_buffer_copy(bytes(blob) or b"\0")
        return arr, len(rows), buf, len(blob), on_device

    def regex_host_items(self) -> List[Tuple[str, int, str]]:
        """(resource, index, pattern) of the REGEX items that follow the regex_bits word: all of them without
        device_regex, with it those the compiler declined.  Empty: parse_device needs no regex_bits."""
        names = {rid: name for name, rid in self.s.ids.items()}
        return [(names[rid], e[1].index, e[1].pattern) for rid, row in self._slots.items() for e in row
                if isinstance(e, tuple) and id(e[1]) in self._regex]

    # ---- one request on the host (gateway_entry)
    def parse_one(self, resource: str, mode: int, request: Mapping) -> list:
        """parseParameterFor(resource, request, rule -> rule.resourceMode == mode) for a registered resource."""
        row = self._slots.get(self.s.ids.get(resource, -1))
        if not row:
            return []
        if any(r.param_item is not None and r.resource_mode != mode for r in self._rule_map.get(resource, [])):
            return []
        out = []
        for e in row:
            if isinstance(e, tuple):
                out.append(match_value(e[1], request_field(request, field_key(e[1]))))
            else:
                out.append(e)  # None or "$D"
        return out

    # ---- batches on the device
    def regex_bits(self, resources, requests) -> Optional[np.ndarray]:
        """One uint64 per event: bit k = the REGEX item that writes slot k matches the event's value (re.fullmatch;
        a pattern that does not compile matches).  Bits are set for the items of regex_host_items only -- an item
        the device decides has none, the kernel ignores its bit; None when there is no such item."""
        if not self._regex:
            return None
        bits = np.zeros(len(requests), dtype=np.uint64)
        for i, (rid, rq) in enumerate(zip(resources, requests)):
            w = 0
            for k, e in enumerate(self._slots.get(int(rid), ())):
                if not isinstance(e, tuple) or id(e[1]) not in self._regex:
                    continue
                rx, v = self._regex[id(e[1])], request_field(rq, field_key(e[1]))
                if rx is None or v is None or rx.fullmatch(v):
                    w |= 1 << k
            bits[i] = w
        return bits

    def parse(self, resources, modes, requests, flags=None, param=None, value_base: int = 0):
        """sga_gateway_parse: (flags, param, param_values) numpy arrays for any submit entry.  resources: ids;
        modes: each request's resource mode; requests: one mapping per event, {("header", "X-Flag"): "v",
        ("client_ip", ""): "1.2.3.4", ...}.  flags / param: the events' columns so far (copied; None: zeros) --
        events of resources without gateway rules keep theirs.  The vectors start at param_values[value_base]."""
        r = np.ascontiguousarray(resources, dtype=np.uint32)
        n = len(r)
        m = np.ascontiguousarray(modes, dtype=np.uint8)
        if len(m) != n or len(requests) != n:
            raise ValueError("event arrays differ in length")
        f = np.zeros(n, np.uint8) if flags is None else np.array(flags, dtype=np.uint8)
        p = np.zeros(n, np.uint64) if param is None else np.array(param, dtype=np.uint64)
        off, ln, blob = pack_requests(requests, self._fields)
        rb = self.regex_bits(r, requests)
        vals = np.zeros(max(1, value_base + 2 * self.max_args * n), dtype=np.uint64)
        check(_lib.load().sga_gateway_parse(self.s.engine.handle, r.ctypes.data, m.ctypes.data, off.ctypes.data,
                                            ln.ctypes.data, blob.ctypes.data if len(blob) else None, len(blob),
                                            rb.ctypes.data if rb is not None else None, n, f.ctypes.data,
                                            p.ctypes.data, vals.ctypes.data, len(vals), int(value_base)),
              self.s.engine.handle, "gatewayParse")
        return f, p, vals

    def parse_device(self, resource, mode, field_off, field_len, blob, flags, param, param_values,
                     value_base: int = 0, regex_bits=None, stream=None):
        """sga_gateway_parse_device over torch tensors on the engine's GPU, asynchronous on `stream` (None: the
        engine stream): one chunk of at most max_batch events.  field_off / field_len / blob: pack_requests' arrays
        on the device; flags (uint8), param and param_values (64-bit) are written in place -- param_values holds
        value_base + 2 * max_args * n words.  LocalSentinel.device_status reports a refused event."""
        n = resource.numel()
        for x in (resource, mode, field_off, field_len, blob, flags, param, param_values, regex_bits):
            if x is not None and (not x.is_cuda or not x.is_contiguous()):
                raise ValueError("gateway tensors must be contiguous device tensors")
        nf = len(self._fields)
        if mode.numel() != n or flags.numel() != n or param.numel() != n or field_off.numel() != n * nf or \
                field_len.numel() != n * nf or (regex_bits is not None and regex_bits.numel() != n):
            raise ValueError("gateway tensors differ in length")
        for name, x, size in (("resource", resource, 4), ("mode", mode, 1), ("field_off", field_off, 4),
                              ("field_len", field_len, 4), ("blob", blob, 1), ("flags", flags, 1), ("param", param, 8),
                              ("param_values", param_values, 8), ("regex_bits", regex_bits, 8)):
            if x is not None and x.element_size() != size:
                raise ValueError(f"{name}: {size}-byte elements expected")
        check(_lib.load().sga_gateway_parse_device(
            self.s.engine.handle, resource.data_ptr(), mode.data_ptr(), field_off.data_ptr(), field_len.data_ptr(),
            blob.data_ptr() if blob.numel() else None, blob.numel(),
            regex_bits.data_ptr() if regex_bits is not None else None, n, flags.data_ptr(), param.data_ptr(),
            param_values.data_ptr(), param_values.numel(), int(value_base),
            stream.cuda_stream if stream is not None else None), self.s.engine.handle, "gatewayParseDevice")
        return flags, param, param_values
