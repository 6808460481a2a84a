"""Host-side mirror of the reference's local (in-process) decision path.

Same names and argument meaning as the Java API the engine replaces:
  SphU.entry(resource, EntryType, batchCount, args...)  CORE/SphU.java:84-208  -> LocalSentinel.entry / submit
  Entry.exit(count, args...)                              CORE/Entry.java:86-111  -> Entry.exit
  Tracer.traceEntry(Throwable, Entry)                     CORE/Tracer.java:86-110 -> Entry.trace_error
  FlowRuleManager.loadRules       CORE/slots/block/flow/FlowRuleManager.java:125-127 (strategy DIRECT / RELATE)
  ParamFlowRuleManager.loadRules  PF/slots/block/flow/param/ParamFlowRuleManager.java:52
  DegradeRuleManager.loadRules    CORE/slots/block/degrade/DegradeRuleManager.java:108
  SystemRuleManager.loadRules     CORE/slots/system/SystemRuleManager.java:114-300 (SystemSlot, inbound only)
  AuthorityRuleManager.loadRules  CORE/slots/block/authority/AuthorityRuleManager.java:110-164 (AuthoritySlot: entries
                                  submitted with an origin; AuthorityRuleChecker.passCheck -> authority_check)
  Constants.ENTRY_NODE            CORE/Constants.java:66 -> LocalSentinel.node(ENTRY_NODE), metrics rows
  ClusterNode statistics          CORE/node/StatisticNode.java:185-250 -> LocalSentinel.node
  ContextUtil.enter(name, origin) CORE/context/ContextUtil.java:116-160 -> the `origin` of entry / submit
  ClusterNode.getOriginCountMap   CORE/node/ClusterNode.java:116-118 -> LocalSentinel.origin_node / origin_nodes
  ContextUtil.enter(name, ...)    the `context` of entry / submit; NodeSelectorSlot's DefaultNode per (resource,
                                  context), CORE/slots/nodeselector/NodeSelectorSlot.java:158-177
                                  -> LocalSentinel.default_node / default_nodes
  ClusterBuilderSlot.getClusterNodeMap, getOriginCountMap read whole (the command center's clusterNode, cnode,
                                  origin) -> LocalSentinel.nodes / origin_node_views / default_node_views /
                                  nodes_device (sga_query_nodes: one launch for any number of nodes)
  NodeSelectorSlot's addChild edge, EntranceNode, Constants.ROOT (CORE/node/EntranceNode.java:45-126) as the
                                  command center's tree / jsonTree walk them -> the `parent` of entry / submit on a
                                  LocalSentinel(tree=True), LocalSentinel.tree_rows / invocation_tree
  FlowRuleManager.getRules and its siblings -> the managers' get_rules
  EventObserverRegistry.addStateChangeObserver  CORE/slots/block/degrade/circuitbreaker/EventObserverRegistry.java
                                  -> LocalSentinel.observers (fed by the engine's breaker event log, sga_cb_events_*)
BlockException subclasses as in CORE/slots/block/BlockException.java and its subclasses.

Every decision is computed by the HIP engine (libsentinel_amd.so).  The mocked
TimeUtil clock of the reference tests is the explicit `now` / `ts` argument.
Resources are registered up front (dense ids), like CtSph's chain map keys.
"""
import ctypes as C
import struct
from dataclasses import dataclass
from enum import IntEnum
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import SGA_PARENT_ENTRANCE, SgaConfig, SgaDegradeRule, SgaFlowRule, SgaNodeView, SgaParamRule, check
from .cluster import Engine  # noqa: F401  (one engine serves both paths)
from .rules import AuthorityRule, DegradeRule, FlowRule, ParamFlowRule, RuleConstant  # noqa: F401


class Decision:
    PASS = 0
    BLOCK_FLOW = 1
    BLOCK_PARAM = 2
    BLOCK_DEGRADE = 3
    PASS_WAIT = 4
    BLOCK_SYSTEM = 5
    BLOCK_AUTHORITY = 6


EV_PRIORITIZED = 1
EV_ERROR = 2
EV_HAS_PARAM = 4
EV_INBOUND = 8          # EntryType.IN
EV_PARAM_LIST = 16      # args[0] is a Collection / array (param = offset << 32 | count into param_values)
EV_ARGS = 32            # the whole argument vector (param = offset << 32 | nargs into param_values)
ARG_SCALAR, ARG_NULL, ARG_LIST = 0, 1, 2
ENTRY_NODE = 0xFFFFFFFF  # resource id of Constants.ENTRY_NODE
TOTAL_IN_RESOURCE_NAME = "__total_inbound_traffic__"  # Constants.TOTAL_IN_RESOURCE_NAME
KIND_ENTRY = 0
KIND_EXIT = 1


class BlockException(Exception):
    """rule: the loaded rule object that blocked (None for a SystemBlockException, and while the rule's manager
    has not loaded through this sentinel); rule_limit_app: BlockException.getRuleLimitApp() as each subclass's
    constructor sets it -- what LogSlot writes into sentinel-block.log."""

    def __init__(self, resource: str, rule=None, rule_limit_app: str = RuleConstant.LIMIT_APP_DEFAULT):
        super().__init__(resource)
        self.resource = resource
        self.rule = rule
        self.rule_limit_app = rule_limit_app


class FlowException(BlockException):
    pass


class ParamFlowException(BlockException):
    pass


class DegradeException(BlockException):
    pass


class SystemBlockException(BlockException):
    pass


class AuthorityException(BlockException):
    pass


_EXC = {Decision.BLOCK_FLOW: FlowException, Decision.BLOCK_PARAM: ParamFlowException,
        Decision.BLOCK_DEGRADE: DegradeException, Decision.BLOCK_SYSTEM: SystemBlockException,
        Decision.BLOCK_AUTHORITY: AuthorityException}


def param_value(x) -> int:
    """64-bit key of a hot parameter (ParameterMetric maps compare args[idx] by equals()).

    Integral values (Java byte/short/int/long, boolean) map to their two's-complement
    long bits, floats to their IEEE-754 bits, strings to a 64-bit hash of the UTF-8 bytes
    (distinct strings that collide would share a counter: documented divergence)."""
    if isinstance(x, bool):
        return 1 if x else 0
    if isinstance(x, (int, np.integer)):
        return int(x) & 0xFFFFFFFFFFFFFFFF
    if isinstance(x, (float, np.floating)):
        return struct.unpack("<Q", struct.pack("<d", float(x)))[0]
    if isinstance(x, str):
        import xxhash
        return xxhash.xxh64_intdigest(x.encode("utf-8"), seed=0x5E47)
    raise TypeError(f"unsupported parameter type {type(x).__name__}")


def encode_args(args, pvals: List[int]) -> int:
    """SGA_EV_ARGS encoding of SphU.entry's `Object... args` appended to `pvals` (include/sentinel_amd.h):
    two words per argument -- kind << 62 | list length, then the scalar's key or the offset of the
    list's elements in pvals.  None is a null argument; a list / tuple is a Collection or array (its
    elements in iteration order; ParamFlowChecker.passLocalCheck checks every one).  Returns the event's
    param word, offset << 32 | nargs."""
    off = len(pvals)
    pvals.extend([0] * (2 * len(args)))
    for k, a in enumerate(args):
        if a is None:
            pvals[off + 2 * k] = ARG_NULL << 62
        elif isinstance(a, (list, tuple)):
            vals = [param_value(x) for x in a]
            pvals[off + 2 * k] = (ARG_LIST << 62) | len(vals)
            pvals[off + 2 * k + 1] = len(pvals)
            pvals.extend(vals)
        else:
            pvals[off + 2 * k] = ARG_SCALAR << 62
            pvals[off + 2 * k + 1] = param_value(a)
    return (off << 32) | len(args)


@dataclass
class NodeView:
    pass_qps: float
    block_qps: float
    success_qps: float
    exception_qps: float
    occupied_pass_qps: float
    avg_rt: float
    min_rt: float
    previous_pass_qps: float
    total_pass: int
    total_block: int
    total_success: int
    total_exception: int
    cur_thread_num: int
    waiting: int
    max_success_qps: float
    previous_block_qps: float


# one sga_node_row (sga_query_nodes): the row's ids, then the NodeView fields under their names
NODE_ROW_DTYPE = np.dtype([("resource", "<u4"), ("other", "<u4"), ("entered", "<u4"), ("reserved", "<u4")] +
                          [(f, "<f8" if t is C.c_double else "<i8") for f, t in SgaNodeView._fields_])


# one sga_tree_row (sga_query_tree): the DefaultNode's ids and resolved parent, then the NodeView fields
TREE_ROW_DTYPE = np.dtype([("resource", "<u4"), ("context", "<u4"), ("parent", "<u4"), ("reserved", "<u4")] +
                          [(f, "<f8" if t is C.c_double else "<i8") for f, t in SgaNodeView._fields_])
ROOT_NAME = "machine-root"  # Constants.ROOT_ID


@dataclass
class TreeNode:
    """One node of LocalSentinel.invocation_tree: Constants.ROOT, a context's EntranceNode (entrance = True for
    both) or a DefaultNode, with its children in the order the command center walks them."""
    name: str
    view: NodeView
    entrance: bool
    children: List["TreeNode"]


def entrance_view(children: Sequence[NodeView], statistic_max_rt: int) -> NodeView:
    """EntranceNode's getters over its direct children in the given order (EntranceNode.java:45-126): plain
    doubles, summed sequentially.  blockQps, successQps, passQps, totalQps, curThreadNum, blockRequest,
    totalRequest and totalPass are sums (totalQps is pass_qps + block_qps here: integer-valued doubles, exact in
    any order); avgRt = sum(child.avgRt * child.passQps) / (sum(child.passQps) or 1).  Every other getter reads
    the EntranceNode's own StatisticNode, which nothing ever adds to: zeros, minRt = statistic_max_rt,
    maxSuccessQps = 1 x sampleCount / intervalInSec = 2."""
    total = total_qps = block_qps = success_qps = pass_qps = 0.0
    threads = total_pass = total_block = 0
    for c in children:
        total += c.avg_rt * c.pass_qps
        total_qps += c.pass_qps
        block_qps += c.block_qps
        success_qps += c.success_qps
        pass_qps += c.pass_qps
        threads += c.cur_thread_num
        total_pass += c.total_pass
        total_block += c.total_block
    return NodeView(pass_qps=pass_qps, block_qps=block_qps, success_qps=success_qps, exception_qps=0.0,
                    occupied_pass_qps=0.0, avg_rt=total / (1 if total_qps == 0 else total_qps),
                    min_rt=float(statistic_max_rt), previous_pass_qps=0.0, total_pass=total_pass,
                    total_block=total_block, total_success=0, total_exception=0, cur_thread_num=threads, waiting=0,
                    max_success_qps=2.0, previous_block_qps=0.0)


@dataclass
class MetricNode:
    """CORE/node/metric/MetricNode.java:28-51 (one resource, one second)."""
    timestamp: int
    resource: str
    pass_qps: int
    block_qps: int
    success_qps: int
    exception_qps: int
    rt: int
    occupied_pass_qps: int
    concurrency: int = 0
    classification: int = 0

    def to_thin_string(self) -> str:
        """MetricNode.toThinString (:160-176): the metric log line the dashboard reads."""
        return "|".join(str(x) for x in (self.timestamp, self.resource.replace("|", "_"), self.pass_qps,
                                         self.block_qps, self.success_qps, self.exception_qps, self.rt,
                                         self.occupied_pass_qps, self.concurrency, self.classification))


class Entry:
    """A passed entry; exit() records RT / success (StatisticSlot.exit) and breaker completion."""

    def __init__(self, owner: "LocalSentinel", rid: int, create_ts: int, count: int, param: Optional[int],
                 wait_ms: int, inbound: bool = False, args=(), origin: str = "", context: str = "",
                 parent: Optional["Entry"] = None):
        self._owner = owner
        self.origin = origin
        self.context = context
        self.parent = parent  # the enclosing Entry (CtEntry.parent), None for an outermost one
        self.args = tuple(args)
        self.inbound = inbound
        self.rid = rid
        self.create_timestamp = create_ts
        self.count = count
        self.param = param
        self.wait_ms = wait_ms
        self.error = False
        self.exited = False

    def trace_error(self):
        self.error = True

    def exit(self, now: int):
        if self.exited:
            return
        self.exited = True
        # Entry.exit(count, args): ParamFlowStatisticExitCallback decreases the thread counts of the args
        pvals: List[int] = []
        word = encode_args(self.args, pvals)
        fl = (EV_ERROR if self.error else 0) | EV_ARGS | (EV_INBOUND if self.inbound else 0)
        self._owner.submit([KIND_EXIT], [self.rid], [now], [self.count], [fl], [now - self.create_timestamp],
                           [word], pvals, origin=[self._owner.origin_id(self.origin)] if self.origin else None,
                           context=[self._owner.context_id(self.context)] if self.context else None)


class CircuitBreakerState(IntEnum):
    """CircuitBreaker.State, numbered as sga_circuit_breaker_state and sga_cb_event do."""
    CLOSED = 0
    OPEN = 1
    HALF_OPEN = 2


@dataclass
class BreakerEvent:
    """One sga_cb_event with its rule resolved: the DegradeRule object the manager loaded (None while nothing was
    loaded through this sentinel).  snapshot_value is None exactly when the reference passes null (new_state is
    not OPEN)."""
    seq: int
    sub: int
    ts: int
    resource: int
    breaker: int
    epoch: int
    prev_state: CircuitBreakerState
    new_state: CircuitBreakerState
    rule: object
    snapshot_value: Optional[float]


BREAKER_EVENT_DTYPE = np.dtype([("ts", "<i8"), ("value", "<f8"), ("seq", "<u8"), ("resource", "<u4"),
                                ("breaker", "<u4"), ("epoch", "<u4"), ("sub", "<u2"), ("prev", "u1"), ("next", "u1")])


class EventObserverRegistry:
    """EventObserverRegistry's state-change observers of one LocalSentinel (sentinel.observers).  The first observer
    turns the engine's breaker event log on; from then on every host call of the sentinel that can move a breaker
    drains the log and calls fn(prev_state, new_state, rule, snapshot_value) per transition, in the reference's
    order, every observer in registration order."""

    def __init__(self, sentinel: "LocalSentinel"):
        self._s = sentinel
        self._observers: Dict[str, object] = {}

    def add_state_change_observer(self, name: str, fn) -> None:
        if name is None or fn is None:
            raise ValueError("name and observer cannot be null")
        self._s.enable_breaker_events()
        self._observers[name] = fn

    def remove_state_change_observer(self, name: str) -> bool:
        return self._observers.pop(name, None) is not None

    def get_state_change_observers(self) -> list:
        return list(self._observers.values())

    def dispatch(self, events) -> None:
        """Every event to every observer.  An observer that raises ends the delivery of its event; the events after
        it are not lost: they stay with the sentinel and go out with the next delivery, ahead of newer ones.  The
        exception surfaces from the call that delivered (entry, exit, submit, load_rules, ...), as the reference's
        observers throw into the thread that moved the breaker."""
        events = list(events)
        for i, ev in enumerate(events):
            try:
                for fn in list(self._observers.values()):
                    fn(ev.prev_state, ev.new_state, ev.rule, ev.snapshot_value)
            except BaseException:
                held = getattr(self._s, "_held_events", None)
                if held is not None:
                    held[:0] = events[i + 1:]
                raise


class LocalSentinel:
    """The local slot chain (StatisticSlot, ParamFlowSlot, FlowSlot, DegradeSlot) on one engine."""

    def __init__(self, engine: Engine, resources: Sequence[str], origins: Optional[Sequence[str]] = None,
                 max_origin_nodes: int = 0, contexts: Optional[Sequence[str]] = None, max_context_nodes: int = 0,
                 tree: bool = False, block_log=False, metric_extensions=False):
        """origins: the caller names events may carry (ContextUtil.enter's origin), registered up front like
        the resources; None = no origin tracking.  max_origin_nodes sizes the engine's table of (resource,
        origin) nodes (0: the engine's default).  contexts: the context names events may carry
        (ContextUtil.enter's name), registered the same way and independently; None = no DefaultNodes, no CHAIN
        rules.  max_context_nodes sizes the table of (resource, context) DefaultNodes.  tree (needs contexts):
        submit, submit_device and entry take `parent`, the enclosing entry, and each DefaultNode keeps the parent
        of its first entry (NodeSelectorSlot's addChild); tree_rows and invocation_tree read the result.  The
        default context (sentinel_default_context) appears in the tree only if the caller registers that name and
        submits its entries with that id: context 0 stays untracked.  block_log: True (the engine's default of 65,536
        rows) or a row count turns on the engine's block log (LogSlot: sga_block_log_enable); block_rows drains it
        and block_log.BlockLogWriter writes sentinel-block.log from it.  metric_extensions: True (the engine's default
        of 65,536 block rows) or a block-row capacity turns on the engine's metric extension sums
        (StatisticSlot's callbacks: sga_metric_ext_enable); `metric_extensions` is then the registry of
        metric_extension.MetricExtension objects, metric_ext_rows drains the sums and poll_metric_extensions
        drains and dispatches them."""
        self.engine = engine
        if tree and not contexts:
            raise ValueError("tree=True needs registered contexts")
        self.tree = bool(tree)
        cfg = SgaConfig()
        _lib.load().sga_config_default(C.byref(cfg))
        self.statistic_max_rt = int(cfg.statistic_max_rt)  # Engine creates its engine with the default
        self.resources: List[str] = list(resources)
        self.ids: Dict[str, int] = {r: i for i, r in enumerate(self.resources)}
        if len(self.ids) != len(self.resources):
            raise ValueError("duplicate resource names")
        self.origins: List[str] = list(origins) if origins else []
        # origin ids are 1-based: 0 is the empty origin
        self.origin_ids: Dict[str, int] = {o: i + 1 for i, o in enumerate(self.origins)}
        if len(self.origin_ids) != len(self.origins):
            raise ValueError("duplicate origin names")
        for o in self.origins:  # the names FlowRule.limitApp reserves (AuthorityRuleChecker / filterOrigin)
            if o in (RuleConstant.LIMIT_APP_DEFAULT, RuleConstant.LIMIT_APP_OTHER) or not o:
                raise ValueError(f"origin name {o!r} is reserved")
        self.contexts: List[str] = list(contexts) if contexts else []
        # context ids are 1-based: 0 is "no tracked context" (the default context, whose DefaultNodes nobody reads)
        self.context_ids: Dict[str, int] = {c: i + 1 for i, c in enumerate(self.contexts)}
        if len(self.context_ids) != len(self.contexts):
            raise ValueError("duplicate context names")
        if any(not c for c in self.contexts):
            raise ValueError("context name '' is reserved")
        # records of the two pair tables (0 = the engine's default of 16,384): the most rows a bulk view can give
        self._max_pair_nodes = (max_origin_nodes or 1 << 14, max_context_nodes or 1 << 14)
        check(_lib.load().sga_flow_set_resources(engine.handle, len(self.resources)), engine.handle, "setResources")
        if self.origins:
            check(_lib.load().sga_flow_set_origins(engine.handle, len(self.origins), max_origin_nodes),
                  engine.handle, "setOrigins")
        if self.contexts:
            check(_lib.load().sga_flow_set_contexts(engine.handle, len(self.contexts), max_context_nodes),
                  engine.handle, "setContexts")
        # what the rule managers last sent to the engine, by decision code: a list in the order of the array the
        # loader was given (sga_block_rule_index answers an index into it); AuthorityRules by resource id
        self._loaded: Dict[int, object] = {}
        # String.valueOf(args[paramIdx]) of the parameter blocks entry() raised, by (tag, tag_kind): bounded
        self.param_texts: Dict[tuple, str] = {}
        self.observers = EventObserverRegistry(self)
        self.breaker_event_cap = 0  # 0: the breaker event log is off
        self.breaker_events_lost = 0  # transitions that found the log full, over all drains
        self._held_events: List[BreakerEvent] = []  # drained ahead of a rule reload, not yet handed out
        self.block_log_rows = 0
        if block_log:
            rows = 0 if block_log is True else int(block_log)
            check(_lib.load().sga_block_log_enable(engine.handle, rows), engine.handle, "blockLogEnable")
            self.block_log_rows = max(64, 1 << (rows - 1).bit_length()) if rows else 1 << 16
        self.metric_ext_block_rows = 0  # 0: the metric extension sums are off
        self.metric_extensions = None
        if metric_extensions:
            from .metric_extension import MetricExtensionProvider
            rows = 0 if metric_extensions is True else int(metric_extensions)
            check(_lib.load().sga_metric_ext_enable(engine.handle, rows), engine.handle, "metricExtEnable")
            self.metric_ext_block_rows = max(64, 1 << (rows - 1).bit_length()) if rows else 1 << 16
            self.metric_extensions = MetricExtensionProvider()

    def context_id(self, name: str) -> int:
        """Dense id of a registered context; "" is 0 (no tracked context)."""
        return self.context_ids[name] if name else 0

    def origin_id(self, name: str) -> int:
        """Dense id of a registered origin; "" is 0."""
        return self.origin_ids[name] if name else 0

    def resource_id(self, name: str) -> int:
        return self.ids[name]

    # ---- breaker events (EventObserverRegistry)
    def enable_breaker_events(self, max_events: int = 0) -> None:
        """sga_cb_events_enable: turns the engine's breaker event log on (0: its default of 65,536 records), or
        resizes it while it is empty."""
        if self.breaker_event_cap and not max_events:
            return
        check(_lib.load().sga_cb_events_enable(self.engine.handle, int(max_events)), self.engine.handle,
              "cbEventsEnable")
        self.breaker_event_cap = max(64, 1 << (int(max_events) - 1).bit_length()) if max_events else 1 << 16

    def breaker_event_records(self):
        """sga_cb_events_drain: (records, lost) -- a BREAKER_EVENT_DTYPE array sorted by (seq, sub), and the
        transitions that found the log full since the last drain."""
        n, lost = C.c_size_t(), C.c_uint64()
        cap = self.breaker_event_cap
        while True:
            out = np.zeros(max(1, cap), dtype=BREAKER_EVENT_DTYPE)
            rc = _lib.load().sga_cb_events_drain(self.engine.handle, out.ctypes.data, cap, C.byref(n), C.byref(lost))
            if rc != _lib.SGA_ERANGE:
                break
            cap = int(n.value)  # the log was resized behind this sentinel's back: take what it needs
        check(rc, self.engine.handle, "cbEventsDrain")
        return out[:n.value].copy(), int(lost.value)

    def breaker_events(self) -> List[BreakerEvent]:
        """Drains the log: the pending transitions in the reference's notification order, each with the
        DegradeRule its (resource, breaker) named in the list loaded when it happened."""
        out, self._held_events = self._held_events + self._drain_breaker_events(), []
        return out

    def _drain_breaker_events(self) -> List[BreakerEvent]:
        recs, lost = self.breaker_event_records()
        self.breaker_events_lost += lost
        out = []
        for r in recs:
            nxt = CircuitBreakerState(int(r["next"]))
            out.append(BreakerEvent(int(r["seq"]), int(r["sub"]), int(r["ts"]), int(r["resource"]), int(r["breaker"]),
                                    int(r["epoch"]), CircuitBreakerState(int(r["prev"])), nxt,
                                    self.block_rule(Decision.BLOCK_DEGRADE, int(r["resource"]), int(r["breaker"])),
                                    float(r["value"]) if nxt == CircuitBreakerState.OPEN else None))
        return out

    def _notify(self) -> None:
        """After a host call that waited for its decisions: deliver what the log holds to the observers."""
        if self.breaker_event_cap and self.observers._observers:
            self.observers.dispatch(self.breaker_events())

    # ---- batched form: the engine's native interface
    def submit(self, kind, resource, ts, acquire, flags=None, rt=None, param=None, param_values=None, origin=None,
               context=None, parent=None):
        """Events in arrival order (see _submit); with state-change observers registered, the breaker transitions
        of the call are delivered before it returns."""
        out = self._submit(kind, resource, ts, acquire, flags, rt, param, param_values, origin, context, parent)
        self._notify()
        return out

    def _submit(self, kind, resource, ts, acquire, flags=None, rt=None, param=None, param_values=None, origin=None,
                context=None, parent=None):
        """Events in arrival order.  param_values: the values of Collection / array arguments
        (events flagged SGA_EV_PARAM_LIST = 16 carry param = offset << 32 | count into it).
        origin: each event's origin id (origin_id; 0 = none), on a sentinel with registered origins.
        context: each event's context id (context_id; 0 = none), on a sentinel with registered contexts.
        parent (tree=True, with context): each event's enclosing entry's resource id, SGA_PARENT_ENTRANCE for an
        outermost one (sga_submit_events_tree)."""
        if parent is not None and (not self.tree or context is None):
            raise ValueError("parent needs a LocalSentinel(tree=True) and a context array")
        k = np.ascontiguousarray(kind, dtype=np.uint8)
        r = np.ascontiguousarray(resource, dtype=np.uint32)
        t = np.ascontiguousarray(ts, dtype=np.int64)
        a = np.ascontiguousarray(acquire, dtype=np.int32)
        n = len(k)
        if not (len(r) == len(t) == len(a) == n):
            raise ValueError("event arrays differ in length")
        f = np.ascontiguousarray(flags, dtype=np.uint8) if flags is not None else None
        rtv = np.ascontiguousarray(rt, dtype=np.int64) if rt is not None else None
        pv = np.ascontiguousarray(param, dtype=np.uint64) if param is not None else None
        for x in (f, rtv, pv):
            if x is not None and len(x) != n:
                raise ValueError("event arrays differ in length")
        dec = np.zeros(n, dtype=np.int8)
        wait = np.zeros(n, dtype=np.int32)
        vals = np.ascontiguousarray(param_values, dtype=np.uint64) if param_values is not None else None
        if context is not None:
            og = np.ascontiguousarray(origin, dtype=np.uint32) if origin is not None else None
            cx = np.ascontiguousarray(context, dtype=np.uint32)
            if len(cx) != n or (og is not None and len(og) != n):
                raise ValueError("event arrays differ in length")
            if parent is not None:
                pa = np.ascontiguousarray(parent, dtype=np.uint32)
                if len(pa) != n:
                    raise ValueError("event arrays differ in length")
                rc = _lib.load().sga_submit_events_tree(
                    self.engine.handle, k.ctypes.data, r.ctypes.data, t.ctypes.data, a.ctypes.data,
                    f.ctypes.data if f is not None else None, rtv.ctypes.data if rtv is not None else None,
                    pv.ctypes.data if pv is not None else None, og.ctypes.data if og is not None else None,
                    cx.ctypes.data, pa.ctypes.data, n, vals.ctypes.data if vals is not None and len(vals) else None,
                    len(vals) if vals is not None else 0, dec.ctypes.data, wait.ctypes.data)
                check(rc, self.engine.handle, "submitEvents")
                return dec, wait
            rc = _lib.load().sga_submit_events_ctx(
                self.engine.handle, k.ctypes.data, r.ctypes.data, t.ctypes.data, a.ctypes.data,
                f.ctypes.data if f is not None else None, rtv.ctypes.data if rtv is not None else None,
                pv.ctypes.data if pv is not None else None, og.ctypes.data if og is not None else None,
                cx.ctypes.data, n, vals.ctypes.data if vals is not None and len(vals) else None,
                len(vals) if vals is not None else 0, dec.ctypes.data, wait.ctypes.data)
            check(rc, self.engine.handle, "submitEvents")
            return dec, wait
        if origin is not None:
            og = np.ascontiguousarray(origin, dtype=np.uint32)
            if len(og) != n:
                raise ValueError("event arrays differ in length")
            rc = _lib.load().sga_submit_events_origin(
                self.engine.handle, k.ctypes.data, r.ctypes.data, t.ctypes.data, a.ctypes.data,
                f.ctypes.data if f is not None else None, rtv.ctypes.data if rtv is not None else None,
                pv.ctypes.data if pv is not None else None, og.ctypes.data, n,
                vals.ctypes.data if vals is not None and len(vals) else None, len(vals) if vals is not None else 0,
                dec.ctypes.data, wait.ctypes.data)
            check(rc, self.engine.handle, "submitEvents")
            return dec, wait
        rc = _lib.load().sga_submit_events_ex(
            self.engine.handle, k.ctypes.data, r.ctypes.data, t.ctypes.data, a.ctypes.data,
            f.ctypes.data if f is not None else None, rtv.ctypes.data if rtv is not None else None,
            pv.ctypes.data if pv is not None else None, n,
            vals.ctypes.data if vals is not None and len(vals) else None, len(vals) if vals is not None else 0,
            dec.ctypes.data, wait.ctypes.data)
        check(rc, self.engine.handle, "submitEvents")
        return dec, wait

    # ---- one event at a time through the coalescing queue (sga_event_submit / sga_event_poll): what a
    # synchronous SphU.entry / Entry.exit of one application thread calls; concurrent callers share a batch
    def event_submit(self, kind, resource, ts, acquire, flags=0, rt=0, param=0, param_values=None) -> int:
        """Enqueue one event (kind, flags, param as in submit; param_values: this event's argument words only).
        Returns a ticket for event_poll."""
        pv = None if param_values is None else np.ascontiguousarray(param_values, dtype=np.uint64)
        t = C.c_uint64()
        rc = _lib.load().sga_event_submit(self.engine.handle, int(kind), int(resource), int(ts), int(acquire),
                                          int(flags), int(rt), int(param), pv.ctypes.data if pv is not None else None,
                                          0 if pv is None else len(pv), C.byref(t))
        check(rc, self.engine.handle, "eventSubmit")
        self._notify()
        return int(t.value)

    def event_poll(self, ticket):
        """(decision, wait_ms) once the ticket's event is decided (each ticket answers once), else None."""
        d, w = C.c_int8(), C.c_int32()
        rc = _lib.load().sga_event_poll(self.engine.handle, int(ticket), C.byref(d), C.byref(w))
        if rc == -11:  # SGA_EAGAIN
            return None
        check(rc, self.engine.handle, "eventPoll")
        self._notify()
        return int(d.value), int(w.value)

    def event_post(self, kind, resource, ts, acquire, flags=0, rt=0, param=0, param_values=None) -> int:
        """Queue an exit / block / revoke (kinds 1-3) without waiting (sga_event_post): decided in ticket order
        before anything queued or called later.  Returns its ticket (~0: decided on its own)."""
        pv = None if param_values is None else np.ascontiguousarray(param_values, dtype=np.uint64)
        t = C.c_uint64()
        rc = _lib.load().sga_event_post(self.engine.handle, int(kind), int(resource), int(ts), int(acquire), int(flags),
                                        int(rt), int(param), pv.ctypes.data if pv is not None else None,
                                        0 if pv is None else len(pv), C.byref(t))
        check(rc, self.engine.handle, "eventPost")
        self._notify()
        return int(t.value)

    def event_one(self, kind, resource, ts, acquire, flags=0, rt=0, param=0, param_values=None):
        """event_submit + event_poll until decided: (decision, wait_ms)."""
        pv = None if param_values is None else np.ascontiguousarray(param_values, dtype=np.uint64)
        d, w = C.c_int8(), C.c_int32()
        rc = _lib.load().sga_event_one(self.engine.handle, int(kind), int(resource), int(ts), int(acquire), int(flags),
                                       int(rt), int(param), pv.ctypes.data if pv is not None else None,
                                       0 if pv is None else len(pv), C.byref(d), C.byref(w))
        check(rc, self.engine.handle, "eventOne")
        self._notify()
        return int(d.value), int(w.value)

    def submit_device(self, kind, resource, ts_base, ts_off, acquire, flags=None, rt=None, param=None,
                      param_values=None, decision=None, wait=None, stream=None, origin=None, context=None,
                      parent=None):
        """submit over device tensors (torch, on the engine's GPU), asynchronous on `stream` (torch stream or
        None = the engine stream): one chunk of at most max_batch events with timestamps ts_base + ts_off.
        Returns (decision int8, wait int32) device tensors; device_status() reports a chunk the device
        checks rejected (rc -EINVAL) or a full parameter map (rc -ENOMEM) as EngineError.  parent (tree=True, with
        context): the enclosing entries' resource ids (sga_submit_events_tree_device)."""
        import torch
        if parent is not None and (not self.tree or context is None):
            raise ValueError("parent needs a LocalSentinel(tree=True) and a context tensor")
        n = kind.numel()
        for x in (resource, ts_off, acquire) + tuple(v for v in (flags, rt, param, origin, context, parent)
                                                     if v is not None):
            if x.numel() != n or not x.is_cuda or not x.is_contiguous():
                raise ValueError("event tensors must be contiguous device tensors of one length")
        want = {"kind": (kind, torch.uint8), "resource": (resource, torch.int32), "ts_off": (ts_off, torch.int32),
                "acquire": (acquire, torch.int32), "flags": (flags, torch.uint8), "rt": (rt, torch.int64),
                "param": (param, torch.int64), "param_values": (param_values, torch.int64),
                "origin": (origin, torch.int32), "context": (context, torch.int32), "parent": (parent, torch.int32)}
        for name, (x, dt) in want.items():
            if x is not None and x.element_size() != torch.empty(0, dtype=dt).element_size():
                raise ValueError(f"{name}: element size of {dt} expected")
        if decision is None:
            decision = torch.empty(n, dtype=torch.int8, device=kind.device)
        if wait is None:
            wait = torch.empty(n, dtype=torch.int32, device=kind.device)
        ptr = (lambda x: x.data_ptr() if x is not None else None)
        if parent is not None:  # the _ctx entry below with the enclosing entry per event
            rc = _lib.load().sga_submit_events_tree_device(
                self.engine.handle, kind.data_ptr(), resource.data_ptr(), int(ts_base), ts_off.data_ptr(),
                acquire.data_ptr(), ptr(flags), ptr(rt), ptr(param), ptr(origin), context.data_ptr(),
                parent.data_ptr(), n, ptr(param_values), param_values.numel() if param_values is not None else 0,
                decision.data_ptr(), wait.data_ptr(), stream.cuda_stream if stream is not None else None)
            check(rc, self.engine.handle, "submitEventsDevice")
            return decision, wait
        if context is not None:  # context (and origin) ids per event; a full table: device_status, rc -ENOMEM
            rc = _lib.load().sga_submit_events_ctx_device(
                self.engine.handle, kind.data_ptr(), resource.data_ptr(), int(ts_base), ts_off.data_ptr(),
                acquire.data_ptr(), ptr(flags), ptr(rt), ptr(param), ptr(origin), context.data_ptr(), n,
                ptr(param_values), param_values.numel() if param_values is not None else 0, decision.data_ptr(),
                wait.data_ptr(), stream.cuda_stream if stream is not None else None)
            check(rc, self.engine.handle, "submitEventsDevice")
            return decision, wait
        if origin is not None:  # origin ids per event (a full origin table: device_status, rc -ENOMEM)
            rc = _lib.load().sga_submit_events_origin_device(
                self.engine.handle, kind.data_ptr(), resource.data_ptr(), int(ts_base), ts_off.data_ptr(),
                acquire.data_ptr(), ptr(flags), ptr(rt), ptr(param), origin.data_ptr(), n, ptr(param_values),
                param_values.numel() if param_values is not None else 0, decision.data_ptr(), wait.data_ptr(),
                stream.cuda_stream if stream is not None else None)
            check(rc, self.engine.handle, "submitEventsDevice")
            return decision, wait
        rc = _lib.load().sga_submit_events_device(
            self.engine.handle, kind.data_ptr(), resource.data_ptr(), int(ts_base), ts_off.data_ptr(),
            acquire.data_ptr(), ptr(flags), ptr(rt), ptr(param), n, ptr(param_values),
            param_values.numel() if param_values is not None else 0, decision.data_ptr(), wait.data_ptr(),
            stream.cuda_stream if stream is not None else None)
        check(rc, self.engine.handle, "submitEventsDevice")
        return decision, wait

    def device_status(self):
        """Waits for the engine stream; EngineError for a rejected device chunk or a full parameter map."""
        check(_lib.load().sga_events_device_status(self.engine.handle), self.engine.handle, "submitEventsDevice")

    # ---- SphU-style single entry
    def entry(self, resource: str, now: int, batch_count: int = 1, prioritized: bool = False, args=(),
              entry_type: str = "OUT", origin: str = "", context: str = "",
              parent: Optional[Entry] = None) -> Entry:
        """SphU.entry(resource, entryType, batchCount, args); entry_type "IN" marks inbound traffic; origin:
        the caller the context was entered with (a registered origin name), context: that context's name (a
        registered context; "" = the default context, untracked), both kept by the Entry for its exit.  parent
        (tree=True): the Entry this one is nested in (the context's current entry, CtEntry.parent); its resource
        is what context.getLastNode() answers, None = the context's EntranceNode.  The Entry keeps it."""
        if parent is not None and not self.tree:
            raise ValueError("parent needs a LocalSentinel(tree=True)")
        pa = None
        if self.tree and context:
            pa = [parent.rid if parent is not None else SGA_PARENT_ENTRANCE]
        rid = self.ids[resource]
        inbound = entry_type == "IN"
        # the whole argument vector (SGA_EV_ARGS): ParamFlowSlot indexes args by each rule's paramIdx
        pvals: List[int] = []
        word = encode_args(tuple(args), pvals)
        fl = (EV_PRIORITIZED if prioritized else 0) | EV_ARGS | (EV_INBOUND if inbound else 0)
        dec, wait = self.submit([KIND_ENTRY], [rid], [now], [batch_count], [fl], None, [word], pvals,
                                origin=[self.origin_id(origin)] if origin else None,
                                context=[self.context_id(context)] if context else None, parent=pa)
        d = int(dec[0])
        if d in _EXC:
            raise self._block_exception(d, resource, rid, int(wait[0]), tuple(args), origin)
        param = param_value(args[0]) if len(args) > 0 and args[0] is not None and \
            not isinstance(args[0], (list, tuple)) else None
        return Entry(self, rid, now, batch_count, param, int(wait[0]), inbound, args, origin, context, parent)

    def gateway_entry(self, resource: str, mode: int, request, now: int, **kw) -> Entry:
        """A gateway filter's entry of one route or API group (a sentinel with a gateway.GatewayRuleManager):
        GatewayParamParser.parseParameterFor(resource, request, rule -> rule.resourceMode == mode) on the host, then
        entry(resource, now, args=...).  request: {("header", "X-Flag"): "v", ("client_ip", ""): "1.2.3.4", ...}.
        A block by a gateway rule raises ParamFlowException whose rule is the converted ParamFlowRule and whose
        rule_limit_app is String.valueOf of the parsed value ("$NM" for a value that missed its pattern)."""
        gw = getattr(self, "_gateway", None)
        if gw is None:
            raise ValueError("gateway_entry needs a GatewayRuleManager on this sentinel")
        return self.entry(resource, now, args=tuple(gw.parse_one(resource, mode, request)), **kw)

    def gateway_request(self, route: Optional[str], path: Optional[str], request, now: int, **kw):
        """A gateway filter's sequence for one request (SentinelZuulPreFilter.run:118-134 and its twins; a sentinel
        with a gateway.GatewayRuleManager and a gateway_api.GatewayApiDefinitionManager): gateway_entry on the route
        (mode 0) unless it is blank, then on every API group matching_apis_one(path) names (mode 1), in definition
        order, stopping at the first block.  Returns (entries, block): the entries made, for the caller to exit, and
        the BlockException that ended the sequence or None.  A matching definition whose name is no registered
        resource is not entered."""
        apis = getattr(self, "_gateway_api", None)
        if apis is None:
            raise ValueError("gateway_request needs a GatewayApiDefinitionManager on this sentinel")
        todo = [] if route is None or not route.strip() else [(route, 0)]
        todo += [(name, 1) for name in apis.matching_apis_one(path) if name in self.ids]
        entries: List[Entry] = []
        for name, mode in todo:
            try:
                entries.append(self.gateway_entry(name, mode, request, now, **kw))
            except BlockException as e:
                return entries, e
        return entries, None

    # ---- block attribution (LogSlot)
    _PARAM_TEXTS_MAX = 4096

    def block_rule_index(self, decision: int, resource, detail: int) -> int:
        """sga_block_rule_index: the position, in the array the matching loader was last given, of the rule a FLOW /
        PARAM / DEGRADE block detail names (the _origin / _ctx flow loaders reorder as FlowRuleComparator does)."""
        rid = resource if isinstance(resource, int) else self.ids[resource]
        idx = C.c_uint32()
        check(_lib.load().sga_block_rule_index(self.engine.handle, int(decision), rid, int(detail), C.byref(idx)),
              self.engine.handle, "blockRuleIndex")
        return int(idx.value)

    def block_rule(self, decision: int, resource, detail: int):
        """The loaded rule object a block names: the FlowRule / ParamFlowRule / DegradeRule at block_rule_index, the
        resource's AuthorityRule, None for a system block or while the manager has not loaded through this sentinel."""
        rid = resource if isinstance(resource, int) else self.ids[resource]
        loaded = self._loaded.get(int(decision))
        if decision == Decision.BLOCK_AUTHORITY:
            return None if loaded is None else loaded.get(rid)
        if loaded is None or decision == Decision.BLOCK_SYSTEM:
            return None
        return loaded[self.block_rule_index(decision, rid, detail)]

    def _block_exception(self, d: int, resource: str, rid: int, detail: int, args: tuple, origin: str):
        from . import block_log as BL
        rule = self.block_rule(d, rid, detail)
        if d == Decision.BLOCK_SYSTEM:  # SystemBlockException(resourceName, limitType)
            lim = BL.SYSTEM_LIMIT_TYPE[detail] if detail < len(BL.SYSTEM_LIMIT_TYPE) else str(detail)
        elif d == Decision.BLOCK_AUTHORITY:  # AuthorityException(context.getOrigin(), rule)
            lim = origin
        elif d == Decision.BLOCK_PARAM:  # ParamFlowException(resourceName, String.valueOf(args[paramIdx]), rule)
            # a negative paramIdx counts from the end (ParamFlowSlot.applyRealParamIdx, fixed on the rule at its
            # first check; resolved here against this call's args)
            idx = getattr(rule, "param_idx", 0)
            if idx < 0:
                idx = len(args) + idx if -idx <= len(args) else -idx
            arg = args[idx] if 0 <= idx < len(args) else None
            lim = BL.java_text(arg)
            if arg is not None:
                if isinstance(arg, (list, tuple)):
                    key = (BL.list_tag([param_value(x) for x in arg]), BL.TAG_LIST)
                else:
                    key = (param_value(arg), BL.TAG_SCALAR)
                if key not in self.param_texts and len(self.param_texts) >= self._PARAM_TEXTS_MAX:
                    self.param_texts.pop(next(iter(self.param_texts)))  # the oldest text goes
                self.param_texts[key] = lim
        else:  # FlowException(rule.getLimitApp(), rule), DegradeException(rule.getLimitApp(), rule)
            lim = getattr(rule, "limit_app", None) or RuleConstant.LIMIT_APP_DEFAULT
        return _EXC[d](resource, rule, lim)

    def block_rows(self, before_ms: Optional[int] = None):
        """sga_block_log_drain: (rows, lost_events, lost_count).  rows: a block_log.BLOCK_ROW_DTYPE array of the
        aggregated keys whose second is finished at before_ms (None: every row), sorted by (time_slot, resource,
        decision, detail, origin, tag_kind, tag); the lost counters: entries, and their acquire sum, that found no
        room in the table since the last drain."""
        from .block_log import BLOCK_ROW_DTYPE
        before = (1 << 63) - 1 if before_ms is None else int(before_ms)
        cap = self.block_log_rows
        n, le, lc = C.c_size_t(), C.c_uint64(), C.c_int64()
        out = np.zeros(max(1, cap), dtype=BLOCK_ROW_DTYPE)
        check(_lib.load().sga_block_log_drain(self.engine.handle, before, out.ctypes.data, cap, C.byref(n),
                                              C.byref(le), C.byref(lc)), self.engine.handle, "blockLogDrain")
        return out[:n.value].copy(), int(le.value), int(lc.value)

    # ---- metric extensions (StatisticSlot's callbacks)
    def metric_ext_rows(self):
        """sga_metric_ext_drain: (res_rows, block_rows, lost_events, lost_count) -- everything summed since the last
        drain.  res_rows: a metric_extension.METRIC_RES_ROW_DTYPE array of the resources with any non-zero sum, sorted
        by resource; block_rows: a METRIC_BLOCK_ROW_DTYPE array sorted by (resource, origin, decision, detail); the
        lost counters: blocked entries, and their acquire sum, that found no room in the block table.  The sums are
        signed deltas: a revoke drained apart from its entry shows as a negative pass."""
        from .metric_extension import METRIC_BLOCK_ROW_DTYPE, METRIC_RES_ROW_DTYPE
        if not self.metric_ext_block_rows:
            raise ValueError("metric_ext_rows needs LocalSentinel(metric_extensions=...)")
        rcap, bcap = len(self.resources), self.metric_ext_block_rows
        res = np.zeros(max(1, rcap), dtype=METRIC_RES_ROW_DTYPE)
        blk = np.zeros(max(1, bcap), dtype=METRIC_BLOCK_ROW_DTYPE)
        nr, nb, le, lc = C.c_size_t(), C.c_size_t(), C.c_uint64(), C.c_int64()
        check(_lib.load().sga_metric_ext_drain(self.engine.handle, res.ctypes.data, rcap, C.byref(nr),
                                               blk.ctypes.data, bcap, C.byref(nb), C.byref(le), C.byref(lc)),
              self.engine.handle, "metricExtDrain")
        return res[:nr.value].copy(), blk[:nb.value].copy(), int(le.value), int(lc.value)

    def poll_metric_extensions(self) -> int:
        """Drains the sums and hands them to the registered extensions (metric_extension.dispatch: resource order,
        registration order, the reference's order inside each callback).  Returns the number of calls made; with no
        extension registered nothing is drained."""
        from .metric_extension import dispatch
        if self.metric_extensions is None:
            raise ValueError("poll_metric_extensions needs LocalSentinel(metric_extensions=...)")
        if not len(self.metric_extensions):
            return 0
        res, blk, le, lc = self.metric_ext_rows()
        return dispatch(self, self.metric_extensions, res, blk, le, lc)

    def node(self, resource, now: int) -> NodeView:
        """ClusterNode views; resource ENTRY_NODE (or TOTAL_IN_RESOURCE_NAME) is Constants.ENTRY_NODE."""
        if resource == TOTAL_IN_RESOURCE_NAME:
            resource = ENTRY_NODE
        rid = resource if isinstance(resource, int) else self.ids[resource]
        v = SgaNodeView()
        check(_lib.load().sga_query_node(self.engine.handle, rid, now, C.byref(v)), self.engine.handle, "node")
        return NodeView(*[getattr(v, f) for f, _ in SgaNodeView._fields_])

    def origin_node(self, resource, origin, now: int) -> Optional[NodeView]:
        """ClusterNode.getOriginCountMap().get(origin): the origin node's views, None while the resource has
        not been entered from that origin."""
        rid = resource if isinstance(resource, int) else self.ids[resource]
        oid = origin if isinstance(origin, int) else self.origin_ids[origin]
        v = SgaNodeView()
        rc = _lib.load().sga_query_origin_node(self.engine.handle, rid, oid, now, C.byref(v))
        if rc == _lib.SGA_ENOENT:
            return None
        check(rc, self.engine.handle, "originNode")
        return NodeView(*[getattr(v, f) for f, _ in SgaNodeView._fields_])

    def origin_nodes(self, resource) -> List[str]:
        """The origins with a node on the resource (the keys of getOriginCountMap), sorted by id."""
        rid = resource if isinstance(resource, int) else self.ids[resource]
        buf = (C.c_uint32 * max(1, len(self.origins)))()
        n = C.c_size_t()
        check(_lib.load().sga_origin_nodes_of(self.engine.handle, rid, buf, len(self.origins), C.byref(n)),
              self.engine.handle, "originNodes")
        return [self.origins[i - 1] for i in sorted(buf[:n.value])]

    def default_node(self, resource, context, now: int) -> Optional[NodeView]:
        """The DefaultNode of the resource in the context (NodeSelectorSlot's map): its views, None while the
        resource has not been entered in that context."""
        rid = resource if isinstance(resource, int) else self.ids[resource]
        cid = context if isinstance(context, int) else self.context_ids[context]
        v = SgaNodeView()
        rc = _lib.load().sga_query_context_node(self.engine.handle, rid, cid, now, C.byref(v))
        if rc == _lib.SGA_ENOENT:
            return None
        check(rc, self.engine.handle, "defaultNode")
        return NodeView(*[getattr(v, f) for f, _ in SgaNodeView._fields_])

    def default_nodes(self, resource) -> List[str]:
        """The contexts with a DefaultNode on the resource, sorted by id."""
        rid = resource if isinstance(resource, int) else self.ids[resource]
        buf = (C.c_uint32 * max(1, len(self.contexts)))()
        n = C.c_size_t()
        check(_lib.load().sga_context_nodes_of(self.engine.handle, rid, buf, len(self.contexts), C.byref(n)),
              self.engine.handle, "defaultNodes")
        return [self.contexts[i - 1] for i in sorted(buf[:n.value])]

    # ---- node views in bulk (sga_query_nodes: one launch, one wave a node)
    def query_nodes(self, table: int, now: int, resources=None, flags: int = 0) -> np.ndarray:
        """Rows of sga_query_nodes as a NODE_ROW_DTYPE array sorted by (resource, other).  resources: ids of this
        table's resources (None: every node of the table)."""
        ids = None if resources is None else np.ascontiguousarray(resources, dtype=np.uint32)
        if table == _lib.SGA_NODES_RESOURCE:
            cap = len(self.resources) if ids is None else len(ids)
        else:
            reg, most = ((self.origins, self._max_pair_nodes[0]) if table == _lib.SGA_NODES_ORIGIN else
                         (self.contexts, self._max_pair_nodes[1]))
            cap = 0 if not reg else most if ids is None else min(most, len(ids) * len(reg))
        n = C.c_size_t()
        for _ in range(2):  # the first cap holds every row the table can give
            out = np.zeros(max(1, cap), dtype=NODE_ROW_DTYPE)
            rc = _lib.load().sga_query_nodes(self.engine.handle, table, None if ids is None else ids.ctypes.data,
                                             0 if ids is None else len(ids), now, flags, out.ctypes.data, cap,
                                             C.byref(n))
            if rc != _lib.SGA_ERANGE:
                break
            cap = n.value
        check(rc, self.engine.handle, "nodes")
        return out[:n.value]

    @staticmethod
    def _view_of(row) -> NodeView:
        return NodeView(*[row[f].item() for f, _ in SgaNodeView._fields_])

    def nodes(self, now: int, resources=None, not_zero: bool = False):
        """[(name, NodeView)] in ascending resource id.  resources None: the ClusterNodes that exist
        (ClusterBuilderSlot.getClusterNodeMap: entered resources, without ENTRY_NODE); a list of names / ids
        (ENTRY_NODE allowed): exactly those, entered or not.  not_zero: only nodes with totalRequest() > 0."""
        ids = None
        if resources is not None:
            ids = [ENTRY_NODE if r == TOTAL_IN_RESOURCE_NAME else r if isinstance(r, int) else self.ids[r]
                   for r in resources]
        rows = self.query_nodes(_lib.SGA_NODES_RESOURCE, now, ids, _lib.SGA_NODES_NOT_ZERO if not_zero else 0)
        return [(TOTAL_IN_RESOURCE_NAME if int(r["resource"]) == ENTRY_NODE else self.resources[int(r["resource"])],
                 self._view_of(r)) for r in rows]

    def origin_node_views(self, resource, now: int):
        """[(origin name, NodeView)] of the resource's origin nodes (getOriginCountMap), ascending origin id."""
        rid = resource if isinstance(resource, int) else self.ids[resource]
        rows = self.query_nodes(_lib.SGA_NODES_ORIGIN, now, [rid])
        return [(self.origins[int(r["other"]) - 1], self._view_of(r)) for r in rows]

    def default_node_views(self, resource, now: int):
        """[(context name, NodeView)] of the resource's DefaultNodes, ascending context id."""
        rid = resource if isinstance(resource, int) else self.ids[resource]
        rows = self.query_nodes(_lib.SGA_NODES_CONTEXT, now, [rid])
        return [(self.contexts[int(r["other"]) - 1], self._view_of(r)) for r in rows]

    # ---- the invocation tree (sga_query_tree: one launch, one wave a DefaultNode)
    def tree_rows(self, now: int) -> np.ndarray:
        """One TREE_ROW_DTYPE row per DefaultNode, sorted by (context, resource): its view at `now` and its
        resolved parent -- a resource id of the same context, or SGA_PARENT_ENTRANCE."""
        if not self.tree:
            raise ValueError("tree_rows needs a LocalSentinel(tree=True)")
        cap = min(self._max_pair_nodes[1], len(self.resources) * len(self.contexts))
        n = C.c_size_t()
        out = np.zeros(max(1, cap), dtype=TREE_ROW_DTYPE)
        check(_lib.load().sga_query_tree(self.engine.handle, now, out.ctypes.data, cap, C.byref(n)),
              self.engine.handle, "treeRows")
        return out[:n.value]

    def invocation_tree(self, now: int) -> TreeNode:
        """Constants.ROOT -> the EntranceNodes of the registered contexts that have a DefaultNode, ascending
        context id -> their DefaultNodes, children in ascending resource id under every node (the reference's
        child order is a HashSet's: parity-unpinned).  DefaultNode views are the engine's; EntranceNode and ROOT
        views are entrance_view over their direct children in that order.  The default context appears only if
        the caller registered its name and submitted its entries with that id (context 0 is untracked), and a
        context nobody has entered has no EntranceNode here."""
        rows = self.tree_rows(now)
        root_children: List[TreeNode] = []
        for cid in sorted({int(c) for c in rows["context"]}):
            mine = [r for r in rows if int(r["context"]) == cid]  # ascending resource id
            made = {int(r["resource"]): TreeNode(self.resources[int(r["resource"])], self._view_of(r), False, [])
                    for r in mine}
            top: List[TreeNode] = []
            for r in mine:
                p = int(r["parent"])
                (top if p == SGA_PARENT_ENTRANCE else made[p].children).append(made[int(r["resource"])])
            root_children.append(TreeNode(self.contexts[cid - 1],
                                          entrance_view([t.view for t in top], self.statistic_max_rt), True, top))
        return TreeNode(ROOT_NAME, entrance_view([t.view for t in root_children], self.statistic_max_rt), True,
                        root_children)

    def nodes_device(self, now: int, table: int = 0, not_zero: bool = False, cap: Optional[int] = None, stream=None):
        """Every node of the table into device memory (sga_query_nodes_device), asynchronous on `stream` (a torch
        stream; None = the engine stream): (rows, count) torch tensors on the engine's GPU -- rows uint8 of shape
        (cap, 144), one sga_node_row each (NODE_ROW_DTYPE once on the host), in no particular order; count int32
        of shape (1,), the full number of rows, of which min(count, cap) are written (the rest of `rows` is not
        initialised).  Work on another stream must wait for `stream`; with the engine stream, sga_sync
        waits for it on the host."""
        import torch
        if cap is None:
            cap = len(self.resources) if table == _lib.SGA_NODES_RESOURCE else self._max_pair_nodes[table - 1]
        dev = torch.device("cuda", self.engine.device)
        # empty, not zeros: a fill on torch's stream would race with the engine's writes on another
        rows = torch.empty((max(1, cap), NODE_ROW_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        check(_lib.load().sga_query_nodes_device(self.engine.handle, table, now,
                                                 _lib.SGA_NODES_NOT_ZERO if not_zero else 0, rows.data_ptr(), cap,
                                                 count.data_ptr(), stream.cuda_stream if stream is not None else None),
              self.engine.handle, "nodesDevice")
        return rows, count

    def metrics(self, now: int, cap: int = 1 << 16) -> List[MetricNode]:
        """MetricTimerListener.run (CORE/node/metric/MetricTimerListener.java:44-65): StatisticNode.metrics()
        of every resource at `now`, ordered by timestamp then resource (the TreeMap the reference writes)."""
        buf = (_lib.SgaMetricNode * max(1, cap))()
        n = C.c_size_t()
        rc = _lib.load().sga_metrics_snapshot(self.engine.handle, now, buf, cap, C.byref(n))
        _lib.check(rc, self.engine.handle, "metrics")
        def name(r):
            return TOTAL_IN_RESOURCE_NAME if r == ENTRY_NODE else self.resources[r]

        out = [MetricNode(b.timestamp, name(b.resource), b.pass_qps, b.block_qps, b.success_qps,
                          b.exception_qps, b.rt, b.occupied_pass_qps, b.concurrency)
               for b in buf[:n.value]]
        out.sort(key=lambda m: (m.timestamp, self.ids.get(m.resource, ENTRY_NODE)))
        return out

    def group_of(self, resource) -> int:
        """Leader (smallest resource id) of the group the loaded RELATE FlowRules put `resource` in, or
        SGA_REF_NONE when none couples it.  A group's events are decided in arrival order by one lane."""
        rid = resource if isinstance(resource, int) else self.ids[resource]
        leader = C.c_uint32()
        check(_lib.load().sga_flow_group_of(self.engine.handle, rid, C.byref(leader)), self.engine.handle, "groupOf")
        return int(leader.value)

    def circuit_breaker_state(self, resource, k: int = 0) -> int:
        rid = resource if isinstance(resource, int) else self.ids[resource]
        return _lib.load().sga_circuit_breaker_state(self.engine.handle, rid, k)

    def authority_check(self, resources, origins) -> np.ndarray:
        """AuthorityRuleChecker.passCheck of the loaded AuthorityRules for (resource id, origin id) pairs, in one
        launch of the kernel the slot runs (sga_authority_check): a bool array, True = passes.  Touches no state."""
        r = np.ascontiguousarray(resources, dtype=np.uint32)
        o = np.ascontiguousarray(origins, dtype=np.uint32)
        if len(r) != len(o):
            raise ValueError("resources and origins differ in length")
        out = np.zeros(max(1, len(r)), dtype=np.uint8)
        check(_lib.load().sga_authority_check(self.engine.handle, r.ctypes.data, o.ctypes.data, len(r),
                                              out.ctypes.data), self.engine.handle, "authorityCheck")
        return out[:len(r)].astype(bool)


class ClusterStateManager:
    """ClusterStateManager (CORE/cluster/ClusterStateManager.java) as the local path sees it:
    CLUSTER_SERVER = the embedded token server is this engine (sga_set_cluster_server 1);
    CLUSTER_NOT_STARTED = no token service, cluster-mode rules fall back.  The client mode (a
    remote token server over the network) is outside the decision path."""
    CLUSTER_NOT_STARTED, CLUSTER_SERVER = 0, 1

    def __init__(self, sentinel: "LocalSentinel"):
        self.s = sentinel

    def set_to_server(self):
        check(_lib.load().sga_set_cluster_server(self.s.engine.handle, 1), self.s.engine.handle, "setToServer")

    def stop(self):
        check(_lib.load().sga_set_cluster_server(self.s.engine.handle, 0), self.s.engine.handle, "stop")


class FlowRuleManager:
    def __init__(self, sentinel: LocalSentinel):
        self.s = sentinel

    def get_rules(self) -> list:
        """The list last loaded (the reference's getRules()); a rule naming a resource this sentinel does not
        have stays in it and applies to nothing, like a rule of a resource nobody enters."""
        return list(getattr(self, "_rules", []))

    def load_rules(self, rules: List[FlowRule]) -> int:
        """FlowRuleManager.loadRules.  Cluster-mode rules ask the token service when checked
        (FlowRuleChecker.passClusterCheck): with ClusterStateManager set to server the engine's own
        cluster rules (ClusterFlowRuleManager on the same Engine) decide their flowId, otherwise
        they fall back (fallbackToLocalWhenFail: the local rater, else pass)."""
        self._rules = list(rules)
        rules = [r for r in rules if r.resource in self.s.ids]
        arr = (SgaFlowRule * max(1, len(rules)))()
        # a sentinel with registered origins names each rule's limitApp by id (sga_load_flow_rules_origin: the rule
        # then applies to that origin's entries, or "other" to the origins no rule of the resource names, and
        # reads the origin node); one without keeps the plain loader and its mapping
        oids = getattr(self.s, "origin_ids", None) or None
        # one with registered contexts names a CHAIN rule's refResource, a context name, by id
        # (sga_load_flow_rules_ctx: the rule then applies to that context's entries and reads their DefaultNode)
        cids = getattr(self.s, "context_ids", None) or None
        lim = (C.c_uint32 * max(1, len(rules)))()
        for i, r in enumerate(rules):
            a = arr[i]
            a.resource = self.s.ids[r.resource]
            a.grade = r.grade
            a.count = r.count
            a.control_behavior = r.control_behavior
            a.warm_up_period_sec = r.warm_up_period_sec
            a.max_queueing_time_ms = r.max_queueing_time_ms
            # CHAIN is not served on a sentinel without registered contexts (the plain loaders refuse strategy 2
            # themselves), nor a non-default limitApp on a
            # sentinel without registered origins: rejected as invalid.  RELATE (FlowRuleChecker.java:96-116) names its refResource by dense
            # id -- SGA_REF_NONE for a name this sentinel has no resource for: its ClusterNode never exists, so
            # the rule never blocks; a blank refResource is invalid (FlowRuleUtil.checkStrategyField)
            a.strategy = r.strategy if r.limit_app == RuleConstant.LIMIT_APP_DEFAULT or oids else -1
            if oids:  # an unregistered name: no event can carry it (valid, never applies)
                lim[i] = (_lib.SGA_LIMIT_DEFAULT if r.limit_app == RuleConstant.LIMIT_APP_DEFAULT else
                          _lib.SGA_LIMIT_OTHER if r.limit_app == RuleConstant.LIMIT_APP_OTHER else
                          oids.get(r.limit_app, _lib.SGA_LIMIT_UNKNOWN))
            if a.strategy == RuleConstant.STRATEGY_RELATE:
                if r.ref_resource is None or not r.ref_resource.strip():
                    a.strategy = -1
                else:
                    a.ref_resource = self.s.ids.get(r.ref_resource, _lib.SGA_REF_NONE)
            elif a.strategy == RuleConstant.STRATEGY_CHAIN and cids:
                # an unregistered context name: no event can carry it (valid, never applies); blank: invalid
                if r.ref_resource is None or not r.ref_resource.strip():
                    a.strategy = -1
                else:
                    a.ref_resource = cids.get(r.ref_resource, _lib.SGA_CONTEXT_UNKNOWN)
            if r.cluster_mode:
                cc = r.cluster_config
                a.cluster_mode = 1
                a.cluster_fallback = 1 if cc is None or cc.fallback_to_local_when_fail else 0
                a.cluster_flow_id = -1 if cc is None or cc.flow_id is None else int(cc.flow_id)
                a.cluster_sample_count = 0 if cc is None else cc.sample_count
                a.cluster_window_ms = 0 if cc is None else cc.window_interval_ms
                a.cluster_strategy = 0 if cc is None else cc.strategy
        if hasattr(self.s, "_loaded"):
            self.s._loaded[Decision.BLOCK_FLOW] = rules
        if cids:
            return check(_lib.load().sga_load_flow_rules_ctx(self.s.engine.handle, arr, lim if oids else None,
                                                             len(rules)),
                         self.s.engine.handle, "FlowRuleManager.loadRules")
        if oids:
            return check(_lib.load().sga_load_flow_rules_origin(self.s.engine.handle, arr, lim, len(rules)),
                         self.s.engine.handle, "FlowRuleManager.loadRules")
        return check(_lib.load().sga_load_flow_rules(self.s.engine.handle, arr, len(rules)), self.s.engine.handle,
                     "FlowRuleManager.loadRules")


class ParamFlowRuleManager:
    def __init__(self, sentinel: LocalSentinel):
        self.s = sentinel
        self._keep = []

    def get_rules(self) -> list:
        """The list last loaded (the reference's getRules()); a rule naming a resource this sentinel does not
        have stays in it and applies to nothing, like a rule of a resource nobody enters."""
        return list(getattr(self, "_rules", []))

    def load_rules(self, rules: List[ParamFlowRule]) -> int:
        self._rules = list(rules)
        if hasattr(self.s, "_loaded"):
            self.s._param_own = self._rules
        rc, self._keep = _send_param_rules(self.s, self._rules)
        return check(rc, self.s.engine.handle, "ParamFlowRuleManager.loadRules")


def _send_param_rules(s, own: List[ParamFlowRule]):
    """sga_load_param_rules of a sentinel's effective parameter rule list: the converted rules of its
    GatewayRuleManager (none without one) -- GatewayFlowSlot runs ahead of ParamFlowSlot -- then `own`, the list
    last given to ParamFlowRuleManager.  Returns (rc, the arrays the call borrowed)."""
    gw = getattr(s, "_gateway", None)
    rules = (gw.converted_rules() if gw is not None else []) + list(own)
    rules = [r for r in rules if r.resource in s.ids]
    arr = (SgaParamRule * max(1, len(rules)))()
    keep = []
    for i, r in enumerate(rules):
        a = arr[i]
        a.resource = s.ids[r.resource]
        a.grade = r.grade
        a.count = r.count
        a.control_behavior = r.control_behavior
        a.max_queueing_time_ms = r.max_queueing_time_ms
        a.burst_count = r.burst_count
        a.param_idx = r.param_idx
        a.duration_in_sec = r.duration_in_sec
        if r.cluster_mode:  # ParamFlowRule.clusterMode + ParamFlowClusterConfig
            cc = r.cluster_config
            a.cluster_mode = 1
            a.cluster_flow_id = cc.flow_id if cc and cc.flow_id is not None else 0
            a.cluster_fallback = 1 if cc and cc.fallback_to_local_when_fail else 0
            a.cluster_sample_count = cc.sample_count if cc else 0
            a.cluster_window_ms = cc.window_interval_ms if cc else 0
        # ParamFlowRuleUtil.parseHotItems: later items with the same value win
        hot: Dict[int, int] = {}
        for it in r.param_flow_item_list:
            hot[param_value(it.object)] = int(it.count)
        hv = (C.c_uint64 * max(1, len(hot)))(*hot.keys())
        ht = (C.c_int32 * max(1, len(hot)))(*hot.values())
        keep += [hv, ht]
        a.n_hot = len(hot)
        a.hot_values = C.cast(hv, C.POINTER(C.c_uint64))
        a.hot_thresholds = C.cast(ht, C.POINTER(C.c_int32))
    rc = _lib.load().sga_load_param_rules(s.engine.handle, arr, len(rules))
    if hasattr(s, "_loaded"):
        s._loaded[Decision.BLOCK_PARAM] = rules
    return rc, keep


def send_param_rules(s) -> int:
    """Re-sends the effective list after the gateway rules changed (GatewayRuleManager.load_rules)."""
    rc, s._param_keep = _send_param_rules(s, getattr(s, "_param_own", []))
    return check(rc, s.engine.handle, "GatewayRuleManager.loadRules")


class DegradeRuleManager:
    def __init__(self, sentinel: LocalSentinel):
        self.s = sentinel

    def get_rules(self) -> list:
        """The list last loaded (the reference's getRules()); a rule naming a resource this sentinel does not
        have stays in it and applies to nothing, like a rule of a resource nobody enters."""
        return list(getattr(self, "_rules", []))

    def load_rules(self, rules: List[DegradeRule]) -> int:
        # pending breaker events name breakers of the list still loaded: deliver (or hold) them against it first
        if getattr(self.s, "breaker_event_cap", 0):
            self.s._held_events += self.s._drain_breaker_events()
            self.s._notify()
        self._rules = list(rules)
        rules = [r for r in rules if r.resource in self.s.ids]
        arr = (SgaDegradeRule * max(1, len(rules)))()
        for i, r in enumerate(rules):
            a = arr[i]
            a.resource = self.s.ids[r.resource]
            a.grade = r.grade
            a.count = r.count
            a.time_window = r.time_window
            a.min_request_amount = r.min_request_amount
            a.slow_ratio_threshold = r.slow_ratio_threshold
            a.stat_interval_ms = r.stat_interval_ms
        if hasattr(self.s, "_loaded"):
            self.s._loaded[Decision.BLOCK_DEGRADE] = rules
        return check(_lib.load().sga_load_degrade_rules(self.s.engine.handle, arr, len(rules)), self.s.engine.handle,
                     "DegradeRuleManager.loadRules")


class AuthorityRuleManager:
    """AuthorityRuleManager.loadRules (CORE/slots/block/authority/AuthorityRuleManager.java:110-164): one rule per
    resource, the first valid one in list order.  The engine's AuthoritySlot then checks every entry submitted with
    an origin (sga_load_authority_rules); a blocked entry answers Decision.BLOCK_AUTHORITY."""

    def __init__(self, sentinel: LocalSentinel):
        self.s = sentinel
        self._kept: List[AuthorityRule] = []

    @staticmethod
    def is_valid_rule(rule: Optional[AuthorityRule]) -> bool:
        """AuthorityRuleManager.isValidRule: resource and limitApp not blank, strategy >= 0."""
        return (rule is not None and bool(rule.resource) and bool(rule.resource.strip()) and rule.strategy >= 0 and
                bool(rule.limit_app) and bool(rule.limit_app.strip()))

    def get_rules(self) -> list:
        """The rules kept by the last load, in load order (the reference's getRules() walks a map); a rule naming
        a resource this sentinel does not have stays in it and applies to nothing."""
        return list(self._kept)

    def load_rules(self, rules: List[AuthorityRule]) -> int:
        """Replaces the whole set (an empty list clears it); returns the number of rules kept.  Each rule's
        limitApp.split(",") is resolved to origin ids name by name, exactly (no trimming: AuthorityRuleChecker
        compares with equals); a name that is no registered origin is sent as SGA_LIMIT_UNKNOWN, which the engine
        drops, since no event can carry it."""
        kept: List[AuthorityRule] = []
        seen = set()
        for r in rules or []:
            if not self.is_valid_rule(r) or r.resource in seen:
                continue
            seen.add(r.resource)
            kept.append(r)
        send = [r for r in kept if r.resource in self.s.ids]
        oids = self.s.origin_ids
        res = np.zeros(max(1, len(send)), dtype=np.uint32)
        strat = np.zeros(max(1, len(send)), dtype=np.int32)
        off = np.zeros(len(send) + 1, dtype=np.uint32)
        ids: List[int] = []
        for i, r in enumerate(send):
            res[i] = self.s.ids[r.resource]
            strat[i] = r.strategy
            ids.extend(oids.get(name, _lib.SGA_LIMIT_UNKNOWN) for name in r.limit_app.split(","))
            off[i + 1] = len(ids)
        idv = np.asarray(ids if ids else [0], dtype=np.uint32)
        check(_lib.load().sga_load_authority_rules(self.s.engine.handle, res.ctypes.data, strat.ctypes.data,
                                                   off.ctypes.data, len(send), idv.ctypes.data),
              self.s.engine.handle, "AuthorityRuleManager.loadRules")
        self._kept = kept
        if hasattr(self.s, "_loaded"):
            self.s._loaded[Decision.BLOCK_AUTHORITY] = {self.s.ids[r.resource]: r for r in send}
        return len(kept)


@dataclass
class SystemRule:
    """CORE/slots/system/SystemRule.java:43-50 (negative = not set)."""
    highest_system_load: float = -1.0
    highest_cpu_usage: float = -1.0
    qps: float = -1.0
    avg_rt: int = -1
    max_thread: int = -1


class SystemRuleManager:
    """SystemRuleManager.loadRules + the SystemStatusListener readings the host measures."""

    def __init__(self, sentinel: LocalSentinel):
        self.s = sentinel

    def get_rules(self) -> list:
        """The list last loaded (the reference's getRules()); a rule naming a resource this sentinel does not
        have stays in it and applies to nothing, like a rule of a resource nobody enters."""
        return list(getattr(self, "_rules", []))

    def load_rules(self, rules: List[SystemRule]) -> int:
        self._rules = list(rules)
        arr = (_lib.SgaSystemRule * max(1, len(rules)))()
        for i, r in enumerate(rules):
            arr[i].highest_system_load = r.highest_system_load
            arr[i].highest_cpu_usage = r.highest_cpu_usage
            arr[i].qps = r.qps
            arr[i].avg_rt = r.avg_rt
            arr[i].max_thread = r.max_thread
        return check(_lib.load().sga_load_system_rules(self.s.engine.handle, arr, len(rules)), self.s.engine.handle,
                     "SystemRuleManager.loadRules")

    avg_load, cpu_usage = -1.0, -1.0  # SystemRuleManager.getCurrentSystemAvgLoad / getCurrentCpuUsage (-1: not measured)

    def set_system_status(self, avg_load: float, cpu_usage: float):
        self.avg_load, self.cpu_usage = float(avg_load), float(cpu_usage)
        check(_lib.load().sga_set_system_status(self.s.engine.handle, avg_load, cpu_usage), self.s.engine.handle)
