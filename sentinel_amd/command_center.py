"""The reference's simple-HTTP command center for a LocalSentinel (host code, standard library only).

  HttpEventTask (request line, parameters, POST headers and body, HTTP/1.0 responses)
      sentinel-transport-simple-http/.../command/http/HttpEventTask.java -> parse_request & helpers, serve_connection
  SimpleHttpCommandCenter (server socket, next free port)              -> SimpleHttpCommandCenter
  CommandHandler implementations of sentinel-transport-common          -> CommandCenter's handlers:
      version, api, getRules, setRules, clusterNode, cnode, origin, systemStatus, metric
  and of the parameter-flow extension: getParamFlowRules, setParamFlowRules;
      tree, jsonTree over a sentinel that records the invocation tree (LocalSentinel(tree=True)).

The read commands rest on LocalSentinel.query_nodes (sga_query_nodes: one kernel launch per command).  Where the
reference iterates a HashMap of resources or origins, rows come in ascending id (parity-unpinned: DESIGN.md); so do
a tree node's children, where it iterates a HashSet.  tree and jsonTree rest on LocalSentinel.invocation_tree
(sga_query_tree: one launch) and are registered only over a sentinel whose `tree` attribute is true.
Not served: getSwitch / setSwitch, the cluster-mode commands, AuthoritySlot's rules.
"""
import dataclasses
import json
import math
import socket
import threading
import time
import uuid
from typing import Callable, Dict, List, Optional, Tuple
from urllib.parse import unquote_plus

from .gateway import GatewayFlowRule, GatewayParamFlowItem
from .gateway_api import ApiDefinition, ApiPathPredicateItem
from .javautil import double_to_string, is_blank
from .local import ENTRY_NODE, MetricNode, NodeView, SystemRule
from .rules import (AuthorityRule, ClusterFlowConfig, DegradeRule, FlowRule, ParamFlowClusterConfig, ParamFlowItem,
                    ParamFlowRule)

SERVER_ERROR_MESSAGE = "Command server error"
INVALID_COMMAND_MESSAGE = "Invalid command"
STATUS_TEXT = {200: "200 OK", 400: "400 Bad Request", 411: "411 Length Required",
               415: "415 Unsupported Media Type", 500: "500 Internal Server Error"}
REQUEST_TARGET = "command-target"  # HttpCommandUtils.REQUEST_TARGET
SYSTEM_LOAD_RESOURCE_NAME = "__system_load__"  # Constants.SYSTEM_LOAD_RESOURCE_NAME
CPU_USAGE_RESOURCE_NAME = "__cpu_usage__"      # Constants.CPU_USAGE_RESOURCE_NAME
VERSION = "1.8.4"  # Constants.SENTINEL_VERSION of the reference this restates


class RequestException(Exception):
    """transport/command/exception/RequestException: a status code and its text."""

    def __init__(self, status: int, message: str):
        super().__init__(message)
        self.status = status
        self.message = message


class CommandRequest:
    """CommandRequest: parameters (a later duplicate replaces an earlier one) and metadata."""

    def __init__(self):
        self.parameters: Dict[str, str] = {}
        self.metadata: Dict[str, str] = {}

    def get_param(self, key: str, default=None):
        return self.parameters.get(key, default)

    @property
    def target(self) -> Optional[str]:
        return self.metadata.get(REQUEST_TARGET)


# ------------------------------------------------------------------ HttpEventTask
def remove_anchor(s: Optional[str]) -> Optional[str]:
    """"a=1&b=2#mark" -> "a=1&b=2"."""
    if not s:
        return s
    anchor = s.find("#")
    return "" if anchor == 0 else s[:anchor] if anchor > 0 else s


def _java_trim(s: str) -> str:
    return s.strip("".join(chr(c) for c in range(0x21)))  # String.trim: code points <= ' '


def parse_single_param(single: Optional[str], request: CommandRequest) -> None:
    if single is None or len(single) < 3:
        return
    index = single.find("=")
    if index <= 0 or index >= len(single) - 1:
        return
    value = _java_trim(single[index + 1:])
    key = _java_trim(single[:index])
    request.parameters[unquote_plus(key, encoding="utf-8")] = unquote_plus(value, encoding="utf-8")


def parse_params(query: Optional[str], request: CommandRequest) -> None:
    if not query:
        return
    query = remove_anchor(query)
    pos = -1
    while True:
        offset = pos + 1
        pos = query.find("&", offset)
        if offset == pos:
            continue
        parse_single_param(query[offset:len(query) if pos == -1 else pos], request)
        if pos < 0:
            break


def parse_request(line: Optional[str]) -> CommandRequest:
    """HttpEventTask.processQueryString: the request line "GET /name?a=1&b=2 HTTP/1.0"."""
    request = CommandRequest()
    if is_blank(line):
        return request
    start = line.find("/")
    ask = line.rfind(" ") if line.find("?") == -1 else line.find("?")
    space = line.rfind(" ")
    request.metadata[REQUEST_TARGET] = line[start + 1 if start != -1 else 0:ask if ask != -1 else len(line)]
    if ask == -1 or ask == space:
        return request
    parse_params(line[ask + 1:space if space != -1 else len(line)], request)
    return request


def _read_line(stream) -> str:
    """HttpEventTask.readLine: up to '\\n' or the end of the stream, one trailing '\\r' dropped."""
    buf = bytearray()
    while True:
        b = stream.read(1)
        if not b or b == b"\n":
            break
        buf += b
    if buf.endswith(b"\r"):
        del buf[-1]
    return buf.decode("utf-8", "replace")


def parse_post_headers(stream) -> Dict[str, str]:
    headers: Dict[str, str] = {}
    while True:
        line = _read_line(stream)
        if not line:
            return headers
        index = line.find(":")
        if index < 1:
            continue
        name = _java_trim(line[:index]).lower()
        value = _java_trim(line[index + 1:])
        if value:
            headers[name] = value


def _content_type_supported(content_type: str) -> bool:
    idx = content_type.find(";")
    kind = _java_trim(content_type[:idx].lower()) if idx > 0 else content_type.lower()
    return "application/x-www-form-urlencoded" in kind


def process_post_request(stream, request: CommandRequest) -> None:
    """HttpEventTask.processPostRequest: headers, then a form-encoded body of Content-Length bytes."""
    headers = parse_post_headers(stream)
    if "content-type" in headers and not _content_type_supported(headers["content-type"]):
        raise RequestException(415, "Only form-encoded post request is supported")
    try:
        length = int(headers.get("content-length"))
    except (TypeError, ValueError):
        length = 0
    if length < 1:
        raise RequestException(411, "No legal Content-Length")
    body = bytearray()
    while len(body) < length:  # a partial body is allowed
        chunk = stream.read(min(512, length - len(body)))
        if not chunk:
            break
        body += chunk
    parse_params(body.decode("utf-8", "replace"), request)


def format_response(status: int, message: Optional[str]) -> bytes:
    """HttpEventTask.writeResponse."""
    body = b"" if message is None else message.encode("utf-8")
    head = f"HTTP/1.0 {STATUS_TEXT[status]}\r\nContent-Length: {len(body)}\r\nConnection: close\r\n\r\n"
    return head.encode("utf-8") + body


# ------------------------------------------------------------------ formatting the reference's way
def java_format(fmt_widths, *args) -> str:
    """String.format of a run of "%-Ns" conversions: each argument's toString, left-justified to its width."""
    return "".join(_jstr(a).ljust(w) for w, a in zip(fmt_widths, args))


def _jstr(x) -> str:
    if isinstance(x, bool):
        return "true" if x else "false"
    if isinstance(x, float):
        return double_to_string(x)
    return str(x)


def _j_long(x: float) -> int:
    """(long) of a double: truncation, NaN -> 0, saturating."""
    if math.isnan(x):
        return 0
    return max(-(1 << 63), min((1 << 63) - 1, int(x)))


def to_json(x) -> str:
    """fastjson's compact output for what the handlers serialize: doubles as Double.toString, no spaces."""
    if x is None:
        return "null"
    if isinstance(x, bool):
        return "true" if x else "false"
    if isinstance(x, float):
        return double_to_string(x)
    if isinstance(x, int):
        return str(x)
    if isinstance(x, str):
        return json.dumps(x, ensure_ascii=False)
    if isinstance(x, dict):
        return "{" + ",".join(json.dumps(k, ensure_ascii=False) + ":" + to_json(v) for k, v in x.items()) + "}"
    return "[" + ",".join(to_json(v) for v in x) + "]"


def _camel(name: str) -> str:
    head, *rest = name.split("_")
    return head + "".join(p.capitalize() for p in rest)


_NESTED = {(FlowRule, "cluster_config"): ClusterFlowConfig, (ParamFlowRule, "cluster_config"): ParamFlowClusterConfig,
           (ParamFlowRule, "param_flow_item_list"): ParamFlowItem,
           (GatewayFlowRule, "param_item"): GatewayParamFlowItem,
           (ApiDefinition, "predicate_items"): ApiPathPredicateItem}


def rule_to_bean(rule) -> dict:
    """A rule as its Java bean serializes: camelCase keys in alphabetical order (fastjson's default), null
    fields left out."""
    out = {}
    for f in dataclasses.fields(rule):
        v = getattr(rule, f.name)
        if v is None:
            continue
        if dataclasses.is_dataclass(v):
            v = rule_to_bean(v)
        elif isinstance(v, list):
            v = [rule_to_bean(i) if dataclasses.is_dataclass(i) else i for i in v]
        out[_camel(f.name)] = v
    return dict(sorted(out.items()))


def rule_from_bean(cls, obj: dict):
    """JSON.parseObject into a rule: known camelCase keys set, unknown ones ignored, numbers coerced to the
    field's type."""
    if not isinstance(obj, dict):
        raise ValueError("a rule must be a JSON object")
    rule = cls()
    for f in dataclasses.fields(cls):
        key = _camel(f.name)
        if key not in obj or obj[key] is None:
            continue
        v = obj[key]
        nested = _NESTED.get((cls, f.name))
        cur = getattr(rule, f.name)
        if nested is not None:
            v = [rule_from_bean(nested, i) for i in v] if isinstance(v, list) else rule_from_bean(nested, v)
        elif isinstance(cur, bool):
            v = bool(v)
        elif isinstance(cur, float):
            v = float(v)
        elif isinstance(cur, int):
            v = int(v)
        setattr(rule, f.name, v)
    return rule


def _node_rows(fmt_widths, names_views, first_index: int, cols) -> List[str]:
    """The rows of cnode / origin: the name wrapped at the name width, the counters on its first line."""
    width = fmt_widths[1] - 1
    lines = []
    for k, (name, v) in enumerate(names_views):
        wraps = int(math.ceil(len(name) / width)) - 1 if width else 0
        lines.append(java_format(fmt_widths, first_index + k, name if wraps == 0 else name[:width], *cols(v)))
        for j in range(1, wraps + 1):
            end = len(name) if j == wraps else width * (j + 1)
            lines.append(java_format(fmt_widths, "", name[width * j:end], *[""] * len(cols(v))))
    return lines


def format_cnode(matches: List[Tuple[str, NodeView]]) -> str:
    """FetchClusterNodeHumanCommandHandler over the matching (name, view) pairs in map order.  The name width is
    the longest of the first 30 names, at most 79.  The reference never resets its counter between the width
    loop and the row loop: rows are numbered on from the width loop's count, and the row loop stops when the
    counter reaches 30 -- so 29 matches print one row (30), and 30 or more print every match (31, 32, ...)."""
    widths = [4, 80, 10, 10, 10, 11, 9, 6, 10, 11, 9, 11]
    i = min(len(matches), 30)
    name_len = min(max((len(n) for n, _ in matches[:30]), default=0), 79)
    widths[1] = name_len + 1
    head = java_format(widths, "idx", "id", "thread", "pass", "blocked", "success", "total", "aRt", "1m-pass",
                       "1m-block", "1m-all", "exception")
    shown = matches[:30 - i] if i < 30 else matches
    rows = _node_rows(widths, shown, i + 1, lambda v: (
        v.cur_thread_num, v.pass_qps, v.block_qps, v.success_qps, v.pass_qps + v.block_qps, v.avg_rt, v.total_pass,
        v.total_block, v.total_pass + v.total_block, v.exception_qps))
    return "".join(line + "\n" for line in [head] + rows)


def format_origin(show_name: str, origins: List[Tuple[str, NodeView]]) -> str:
    """FetchOriginCommandHandler for a found resource: the name width over the first 120 origins (at most 79),
    at most 30 rows."""
    widths = [4, 80, 10, 10, 11, 9, 6, 10, 11, 9]
    name_len = min(max((len(n) for n, _ in origins[:120]), default=0), 79)
    widths[1] = name_len + 1
    head = java_format(widths, "idx", "origin", "threadNum", "passQps", "blockQps", "totalQps", "aRt", "1m-pass",
                       "1m-block", "1m-total")
    rows = _node_rows(widths, origins[:30], 1, lambda v: (
        v.cur_thread_num, v.pass_qps, v.block_qps, v.pass_qps + v.block_qps, v.avg_rt, v.total_pass, v.total_block,
        v.total_pass + v.total_block))
    return "id: " + show_name + "\n\n" + "".join(line + "\n" for line in [head] + rows)


def node_vo(name: str, v: NodeView, timestamp: int) -> dict:
    """NodeVo.fromClusterNode: (long) truncation of the doubles, keys in alphabetical order, no id / parentId."""
    total = v.total_pass + v.total_block
    return {"averageRt": _j_long(v.avg_rt), "blockQps": _j_long(v.block_qps),
            "exceptionQps": _j_long(v.exception_qps), "oneMinuteBlock": v.total_block,
            "oneMinuteException": v.total_exception, "oneMinutePass": total - v.total_block,
            "oneMinuteTotal": total, "passQps": _j_long(v.pass_qps), "resource": name,
            "successQps": _j_long(v.success_qps), "threadNum": v.cur_thread_num, "timestamp": timestamp,
            "totalQps": _j_long(v.pass_qps + v.block_qps)}


TREE_LEGEND = ("t:threadNum  pq:passQps  bq:blockQps  tq:totalQps  rt:averageRt  prq: passRequestQps 1mp:1m-pass "
               "1mb:1m-block 1mt:1m-total")


def format_tree(tree, id: Optional[str] = None) -> str:
    """FetchTreeCommandHandler over LocalSentinel.invocation_tree's ROOT: a preorder walk, `level` dashes before
    each line, an EntranceNode's line (ROOT is one) prefixed.  With id, the walk starts at level 0 from the ROOT
    child whose name equals id, or, when none does, from every ROOT child whose name contains it."""
    out: List[str] = []

    def visit(level: int, node) -> None:
        v = node.view
        total = v.total_pass + v.total_block
        out.append("-" * level + ("EntranceNode: " if node.entrance else "") +
                   "%s(t:%s pq:%s bq:%s tq:%s rt:%s prq:%s 1mp:%s 1mb:%s 1mt:%s)" % tuple(_jstr(x) for x in (
                       node.name, v.cur_thread_num, v.pass_qps, v.block_qps, v.pass_qps + v.block_qps, v.avg_rt,
                       v.success_qps, total - v.total_block, v.total_block, total)) + "\n")
        for child in node.children:
            visit(level + 1, child)

    if id is None:
        visit(0, tree)
    else:
        exact = next((c for c in tree.children if c.name == id), None)
        for c in ([exact] if exact is not None else [c for c in tree.children if id in c.name]):
            visit(0, c)
    return "".join(out) + "\r\n\r\n" + TREE_LEGEND + "\r\n"


def tree_node_vos(tree, timestamp: int, new_id: Callable[[], object] = uuid.uuid4) -> List[dict]:
    """FetchJsonTreeCommandHandler: NodeVo.fromDefaultNode of every node in preorder from ROOT -- node_vo's
    counters plus id (str(new_id()): a random UUID) and parentId (the parent's id; null for ROOT, and fastjson
    leaves nulls out), keys in alphabetical order."""
    out: List[dict] = []

    def visit(node, parent_id: Optional[str]) -> None:
        vo = node_vo(node.name, node.view, timestamp)
        vo["id"] = str(new_id())
        if parent_id is not None:
            vo["parentId"] = parent_id
        out.append(dict(sorted(vo.items())))
        for child in node.children:
            visit(child, vo["id"])

    visit(tree, None)
    return out


def format_system_status(v: NodeView) -> str:
    """FetchSystemStatusCommandHandler: a HashMap of five keys, written in that HashMap's iteration order."""
    return to_json({"b": v.block_qps, "r": v.avg_rt, "t": v.cur_thread_num, "qps": v.pass_qps,
                    "rqps": v.success_qps})


# ------------------------------------------------------------------ the command center
_RULE_TYPES = {"flow": FlowRule, "degrade": DegradeRule, "system": SystemRule}


class CommandCenter:
    """The handlers over one LocalSentinel.  managers: {"flow": FlowRuleManager, "degrade": DegradeRuleManager,
    "system": SystemRuleManager, "param": ParamFlowRuleManager, "authority": AuthorityRuleManager} (a missing one
    answers as an empty list and refuses setRules); metric_searcher: the MetricSearcher over the files MetricTimerListener writes; clock: the
    engine's `now` in ms (the mocked TimeUtil of the tests, the wall clock by default)."""

    def __init__(self, sentinel, managers: Dict[str, object], metric_searcher=None,
                 clock: Callable[[], int] = lambda: int(time.time() * 1000)):
        self.s = sentinel
        self.managers = dict(managers)
        self.searcher = metric_searcher
        self.clock = clock
        self.lock = threading.Lock()  # the sentinel's host side is not reentrant
        self.handlers: Dict[str, Tuple[str, Callable[[Dict[str, str]], str]]] = {}
        for name, desc, fn in (
                ("version", "get sentinel version", self._version),
                ("api", "get all available command handlers", self._api),
                ("getRules", "get all active rules by type, request param: type={ruleType}", self._get_rules),
                ("setRules", "modify the rules, accept param: type={ruleType}&data={ruleJson}", self._set_rules),
                ("getParamFlowRules", "Get all parameter flow rules", self._get_param_rules),
                ("setParamFlowRules", "Set parameter flow rules, while previous rules will be replaced.",
                 self._set_param_rules),
                ("clusterNode", "get all clusterNode VO, use type=notZero to ignore those nodes with totalRequest <=0",
                 self._cluster_node),
                ("cnode", "get clusterNode metrics by id, request param: id={resourceName}", self._cnode),
                ("origin", "get origin clusterNode by id, request param: id={resourceName}", self._origin),
                ("systemStatus", "get system status", self._system_status),
                ("metric", "get and aggregate metrics, accept param: startTime={startTime}&endTime={endTime}"
                           "&maxLines={maxLines}&identify={resourceName}", self._metric)):
            self.register(name, desc, fn)
        if getattr(sentinel, "tree", False):  # the sentinel records the invocation tree's edges
            self.register("tree", "get metrics in tree mode, use id to specify detailed tree root", self._tree)
            self.register("jsonTree", "get tree node VO start from root node", self._json_tree)
        if "gateway" in self.managers:  # a gateway.GatewayRuleManager: the api-gateway adapter's two handlers
            self.register("gateway/getRules", "Fetch all gateway rules", self._gateway_get_rules)
            self.register("gateway/updateRules", "Update gateway rules", self._gateway_update_rules)
        if "gateway_api" in self.managers:  # a gateway_api.GatewayApiDefinitionManager: the API group handlers
            self.register("gateway/getApiDefinitions", "Fetch all customized gateway API groups",
                          self._gateway_get_api_definitions)
            self.register("gateway/updateApiDefinitions", "", self._gateway_update_api_definitions)
        self.new_id: Callable[[], object] = uuid.uuid4  # NodeVo's UUID.randomUUID()

    def register(self, name: str, desc: str, fn: Callable[[Dict[str, str]], str]) -> None:
        """@CommandMapping(name, desc) on a handler: fn(params) returns the text or raises ValueError (ofFailure)."""
        self.handlers[name] = (desc, fn)

    def handle(self, name: str, params: Dict[str, str]) -> Tuple[bool, str]:
        """(success, text) of CommandHandler.handle; KeyError for a name nobody registered."""
        _, fn = self.handlers[name]
        with self.lock:
            try:
                return True, fn(params)
            except ValueError as e:
                return False, str(e)

    # ---- handlers
    def _version(self, p):
        return VERSION

    def _api(self, p):
        return to_json([{"url": "/" + n, "desc": d} for n, (d, _) in self.handlers.items()])

    def _rules_json(self, key):
        m = self.managers.get(key)
        return to_json([rule_to_bean(r) for r in (m.get_rules() if m is not None else [])])

    def _get_rules(self, p):
        kind = (p.get("type") or "").lower()
        if kind == "authority":  # served by an AuthorityRuleManager; without one, as before the engine ran the slot
            return self._rules_json("authority") if "authority" in self.managers else "[]"
        if kind not in _RULE_TYPES:
            raise ValueError("invalid type")
        return self._rules_json(kind)

    def _load(self, key, cls, data):
        m = self.managers.get(key)
        if m is None:
            raise ValueError(f"no {key} rule manager")
        try:
            arr = json.loads(data) if data else None
            rules = [rule_from_bean(cls, o) for o in (arr or [])]
        except (ValueError, TypeError) as e:
            raise ValueError(f"parse rule data error: {e}")
        m.load_rules(rules)
        return "success"

    def _set_rules(self, p):
        kind = (p.get("type") or "").lower()
        data = p.get("data")
        if data:
            data = unquote_plus(data, encoding="utf-8")  # the handler decodes once more
        if kind == "authority":
            if "authority" in self.managers:
                return self._load("authority", AuthorityRule, data)
            raise ValueError("authority rules are not served: the engine does not run AuthoritySlot")
        if kind not in _RULE_TYPES:
            raise ValueError("invalid type")
        return self._load(kind, _RULE_TYPES[kind], data)

    def _get_param_rules(self, p):
        return self._rules_json("param")

    def _set_param_rules(self, p):
        data = p.get("data")
        if data:
            data = unquote_plus(data, encoding="utf-8")
        return self._load("param", ParamFlowRule, data)

    def _gateway_get_rules(self, p):
        """GetGatewayRuleCommandHandler: JSON.toJSONString(GatewayRuleManager.getRules())."""
        return self._rules_json("gateway")

    def _gateway_update_rules(self, p):
        """UpdateGatewayRuleCommandHandler: a blank data is "Bad data"; data that does not decode or parse answers
        "decode gateway rule data error" (the reference lets fastjson's exception reach the server, which answers
        a failure too); otherwise the rules are loaded and the answer is "success"."""
        data = p.get("data")
        if data is None or not data.strip():
            raise ValueError("Bad data")
        try:
            arr = json.loads(unquote_plus(data, encoding="utf-8", errors="strict"))
            rules = [rule_from_bean(GatewayFlowRule, o) for o in (arr or [])]
        except (ValueError, TypeError):
            raise ValueError("decode gateway rule data error")
        if any(isinstance(o, dict) and o.get("clusterMode") for o in (arr or [])):
            raise ValueError("cluster-mode gateway rules do not exist in the reference: refused")
        self.managers["gateway"].load_rules(rules)
        return "success"

    def _gateway_get_api_definitions(self, p):
        """GetGatewayApiDefinitionGroupCommandHandler: JSON.toJSONString(GatewayApiDefinitionManager.getApiDefinitions())."""
        return to_json([rule_to_bean(d) for d in self.managers["gateway_api"].get_api_definitions()])

    def _gateway_update_api_definitions(self, p):
        """UpdateGatewayApiDefinitionGroupCommandHandler (:47-96): a blank data is "Bad data", data that does not
        decode or parse "decode gateway API definition data error"; every element becomes an ApiDefinition whose
        predicateItems are ApiPathPredicateItems (a missing array: an empty set).  The write-data-source branch is
        not served."""
        data = p.get("data")
        if data is None or not data.strip():
            raise ValueError("Bad data")
        try:
            arr = json.loads(unquote_plus(data, encoding="utf-8", errors="strict"))
            defs = []
            for o in arr:
                d = rule_from_bean(ApiDefinition, o)
                if d.predicate_items is None:
                    d.predicate_items = []
                defs.append(d)
        except (ValueError, TypeError):
            raise ValueError("decode gateway API definition data error")
        self.managers["gateway_api"].load_api_definitions(defs)
        return "success"

    def _cluster_node(self, p):
        now = self.clock()
        not_zero = (p.get("type") or "").lower() == "notzero"
        return to_json([node_vo(n, v, now) for n, v in self.s.nodes(now, not_zero=not_zero)])

    def _cnode(self, p):
        name = p.get("id")
        if not name:
            raise ValueError("Invalid parameter: empty clusterNode name")
        return format_cnode([(n, v) for n, v in self.s.nodes(self.clock()) if name in n])

    def _origin(self, p):
        name = p["id"]  # a missing id is the reference's NullPointerException: a server error
        # the resource is looked up among the registered names (resources are registered up front; one nobody
        # has entered answers like an entered one without origins), then one launch on the origin table
        rid = self.s.ids.get(name)
        if rid is None:
            rid = next((i for i, n in enumerate(self.s.resources) if n.find(name) > 0), None)
        if rid is None:
            return "Not find cNode with id " + name
        origins = self.s.origin_node_views(rid, self.clock()) if self.s.origins else []
        return format_origin(self.s.resources[rid], origins)

    def _tree(self, p):
        return format_tree(self.s.invocation_tree(self.clock()), p.get("id"))

    def _json_tree(self, p):
        now = self.clock()
        return to_json(tree_node_vos(self.s.invocation_tree(now), now, self.new_id))

    def _system_status(self, p):
        return format_system_status(self.s.nodes(self.clock(), [ENTRY_NODE])[0][1])

    def _metric(self, p):
        start_s, end_s, lines_s, identity = (p.get(k) for k in ("startTime", "endTime", "maxLines", "identity"))
        if is_blank(start_s):
            return ""
        if self.searcher is None:
            raise ValueError("Error when retrieving metrics")
        try:
            start = int(start_s)
            if not is_blank(end_s):
                found = self.searcher.find_by_time_and_resource(start, int(end_s), identity)
            else:
                found = self.searcher.find(start, min(int(lines_s) if not is_blank(lines_s) else 6000, 12000))
        except (OSError, ValueError):
            raise ValueError("Error when retrieving metrics")
        found = list(found or [])
        if is_blank(identity):  # the current load and cpu usage, x 10000, as two more rows
            ts = self.clock() // 1000 * 1000
            sysm = self.managers.get("system")
            for value, res in ((getattr(sysm, "avg_load", -1.0), SYSTEM_LOAD_RESOURCE_NAME),
                               (getattr(sysm, "cpu_usage", -1.0), CPU_USAGE_RESOURCE_NAME)):
                if value > 0:
                    found.append(MetricNode(ts, res, _j_long(value * 10000), 0, 0, 0, 0, 0))
        return "".join(n.to_thin_string() + "\n" for n in found)


# ------------------------------------------------------------------ the socket server
def serve_connection(center: CommandCenter, conn: socket.socket) -> None:
    """HttpEventTask.run: one request, one response, close."""
    stream = conn.makefile("rb")
    try:
        try:
            first = _read_line(stream)
            request = parse_request(first)
            if len(first) > 4 and first[:4].upper() == "POST":
                process_post_request(stream, request)
            name = request.target
            if is_blank(name):
                out = format_response(400, INVALID_COMMAND_MESSAGE)
            elif name not in center.handlers:
                out = format_response(400, "Unknown command `" + name + "`")
            else:
                ok, text = center.handle(name, request.parameters)
                out = format_response(200 if ok else 400, text)
        except RequestException as e:
            out = format_response(e.status, e.message)
        except Exception:  # whatever a handler throws: the reference's catch (Throwable)
            out = format_response(500, SERVER_ERROR_MESSAGE)
        conn.sendall(out)
    except OSError:
        pass
    finally:
        stream.close()
        conn.close()


class SimpleHttpCommandCenter:
    """SimpleHttpCommandCenter: one request per connection on host:port; when the port is busy the next one is
    taken (getServerSocketFromBasePort).  Binds the given address only."""

    def __init__(self, center: CommandCenter, host: str = "127.0.0.1", port: int = 8719):
        self.center = center
        self.host = host
        self.base_port = port
        self.port: Optional[int] = None
        self._sock: Optional[socket.socket] = None
        self._thread: Optional[threading.Thread] = None

    def start(self) -> int:
        """Binds and starts serving; returns the port in use."""
        port = self.base_port
        while True:
            sock = socket.socket(socket.AF_INET6 if ":" in self.host else socket.AF_INET, socket.SOCK_STREAM)
            try:
                sock.bind((self.host, port))
                break
            except OSError:
                sock.close()
                if port >= 65535:
                    raise
                port += 1
        sock.listen(100)
        self._sock = sock
        self.port = sock.getsockname()[1]
        self._thread = threading.Thread(target=self._serve, name="sentinel-command-center", daemon=True)
        self._thread.start()
        return self.port

    def _serve(self):
        while True:
            try:
                conn, _ = self._sock.accept()
            except OSError:
                return  # stop() closed the socket
            conn.settimeout(3.0)  # the reference's SO_TIMEOUT on an accepted socket
            threading.Thread(target=serve_connection, args=(self.center, conn), daemon=True).start()

    def stop(self) -> None:
        if self._sock is not None:
            try:
                self._sock.shutdown(socket.SHUT_RDWR)
            except OSError:
                pass
            self._sock.close()
        if self._thread is not None:
            self._thread.join(timeout=2.0)
        self._sock = self._thread = None
        self.port = None
