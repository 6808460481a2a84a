"""Metric extensions: StatisticSlot's callbacks, fed from sums the engine forms.

  MetricCallbackInit        CORE/metric/extension/MetricCallbackInit.java: registers the two callbacks below with
                            StatisticSlotCallbackRegistry; StatisticSlot (StatisticSlot.java:65-175) calls them on
                            every pass (the PriorityWaitException branch included), every block and every exit
  MetricEntryCallback       .../callback/MetricEntryCallback.java:35-58: onPass -> increaseThreadNum + addPass (or
                            AdvancedMetricExtension.onPass); onBlocked -> addBlock (or onBlocked)
  MetricExitCallback        .../callback/MetricExitCallback.java:36-69: addRt(completeTime - createTimestamp),
                            addSuccess, decreaseThreadNum, addException if the entry holds an error (or onComplete,
                            then onError)
  MetricExtensionProvider   the list of extensions (SPI-loaded in the reference; add / remove / clear here)

The engine keeps exact 64-bit sums of what those calls would have added (sga_metric_ext_enable /
sga_metric_ext_drain); LocalSentinel.poll_metric_extensions drains them and dispatch() below turns each drained row
into calls.

Divergences from the reference, all following from summing on the device:
  * Merged calls.  One call per key and drain stands for N reference calls: it carries the summed count and, as
    events= / times=, how many calls it stands for.  That is equivalent for any extension that sums or gauges --
    what the interface is for (Prometheus / Micrometer / JMX counters).  A histogram of single response times cannot
    be rebuilt: add_rt gets the sum, the number of exits and the largest single rt (at least 0).
  * No args: the engine holds 64-bit keys, never the objects, so no method takes them; the parameter that a
    ParamFlowException blocked on is not part of a block row either (its rule_limit_app reads "null").
  * The Throwable of add_exception / on_error is None: the engine only holds the exit's ERROR flag.
  * An AdvancedMetricExtension's ResourceWrapper is the resource's name.
  * Sums are signed deltas.  A revoke (an entry a slot behind the engine's checks blocked) takes the entry's pass
    back; drained apart from its entry it arrives as a negative add_pass / increase_thread_num.
"""
from typing import List

import numpy as np

LOST_RESOURCE = "__lost__"  # the extra add_block of blocks that found no room in the engine's table

# one sga_metric_res_row / sga_metric_block_row (sga_metric_ext_drain)
METRIC_RES_ROW_DTYPE = np.dtype([("pass", "<i8"), ("pass_events", "<i8"), ("success", "<i8"), ("exits", "<i8"),
                                 ("exception", "<i8"), ("exception_events", "<i8"), ("rt_sum", "<i8"),
                                 ("rt_max", "<i8"), ("resource", "<u4"), ("reserved", "<u4")])
METRIC_BLOCK_ROW_DTYPE = np.dtype([("block", "<i8"), ("block_events", "<i8"), ("resource", "<u4"),
                                   ("origin", "<u4"), ("detail", "<u4"), ("decision", "u1"),
                                   ("reserved", "u1", (3,))])


class MetricExtension:
    """MetricExtension.java with merged calls; every method a no-op, for subclasses to override."""

    def add_pass(self, resource: str, n: int, events: int = 1) -> None:
        """n: the summed acquire of `events` passed entries (priority waits included)."""

    def add_block(self, resource: str, n: int, origin: str, block_exception, events: int = 1) -> None:
        """n: the summed acquire of `events` entries blocked for the same reason from the same origin."""

    def add_success(self, resource: str, n: int, events: int = 1) -> None:
        """n: the summed acquire of `events` exits."""

    def add_exception(self, resource: str, n: int, throwable=None, events: int = 1) -> None:
        """n: the summed acquire of `events` exits that carried a business error; throwable is None."""

    def add_rt(self, resource: str, rt_sum: int, events: int = 1, rt_max: int = 0) -> None:
        """rt_sum: the summed response time of `events` exits, uncapped; rt_max: the largest of them, at least 0."""

    def increase_thread_num(self, resource: str, times: int = 1) -> None:
        pass

    def decrease_thread_num(self, resource: str, times: int = 1) -> None:
        pass


class AdvancedMetricExtension(MetricExtension):
    """AdvancedMetricExtension.java with merged calls.  Like the reference's callbacks, the dispatcher calls only the
    four methods below on such an extension: no thread calls, none of MetricExtension's."""

    def on_pass(self, resource: str, batch_count: int, events: int = 1) -> None:
        pass

    def on_blocked(self, resource: str, batch_count: int, origin: str, block_exception, events: int = 1) -> None:
        pass

    def on_complete(self, resource: str, rt_sum: int, batch_count: int, events: int = 1, rt_max: int = 0) -> None:
        pass

    def on_error(self, resource: str, throwable, batch_count: int, events: int = 1) -> None:
        pass


class MetricExtensionProvider:
    """MetricExtensionProvider.java: the extensions in registration order."""

    def __init__(self):
        self._extensions: List[MetricExtension] = []

    def add(self, extension: MetricExtension) -> None:
        if extension is None:
            raise ValueError("extension is None")
        self._extensions.append(extension)

    def remove(self, extension: MetricExtension) -> bool:
        for i, e in enumerate(self._extensions):
            if e is extension:
                del self._extensions[i]
                return True
        return False

    def clear(self) -> None:
        self._extensions.clear()

    def list(self) -> List[MetricExtension]:
        return list(self._extensions)

    def __len__(self) -> int:
        return len(self._extensions)

    def __iter__(self):
        return iter(list(self._extensions))


def block_exception(sentinel, decision: int, resource: str, rid: int, detail: int, origin: str):
    """The BlockException of a block row, built as LocalSentinel.entry builds it (class by decision, .rule through
    block_rule, .rule_limit_app); decision 0 -- the exception was thrown outside the engine -- gives a plain
    BlockException."""
    from .local import BlockException, LocalSentinel
    if decision == 0:
        return BlockException(resource)
    return LocalSentinel._block_exception(sentinel, int(decision), resource, rid, int(detail), (), origin)


def dispatch(sentinel, extensions, res_rows, block_rows, lost_events: int = 0, lost_count: int = 0) -> int:
    """One drain (rows as sga_metric_ext_drain sorts them) as calls, in resource order; for each resource every
    extension in registration order, and inside an extension the reference's order: the pass callback, the block
    callback once per block row, the exit callback.  Lost blocks go out last as one add_block / on_blocked on
    LOST_RESOURCE.  sentinel: anything with resources, origins and block_rule (and param_texts).  Returns the number
    of calls made."""
    from .local import BlockException
    extensions = list(extensions)
    if not extensions:
        return 0
    calls = 0
    by_res = {}
    for r in res_rows:
        by_res.setdefault(int(r["resource"]), [None, []])[0] = r
    for b in block_rows:
        by_res.setdefault(int(b["resource"]), [None, []])[1].append(b)
    for rid in sorted(by_res):
        row, blocks = by_res[rid]
        name = sentinel.resources[rid]
        excs = []
        for b in blocks:
            oid = int(b["origin"])
            origin = sentinel.origins[oid - 1] if oid else ""
            excs.append((int(b["block"]), origin,
                         block_exception(sentinel, int(b["decision"]), name, rid, int(b["detail"]), origin),
                         int(b["block_events"])))
        p = pe = su = ex = ec = ee = rs = rm = 0
        if row is not None:
            p, pe, su, ex = int(row["pass"]), int(row["pass_events"]), int(row["success"]), int(row["exits"])
            ec, ee, rs, rm = (int(row["exception"]), int(row["exception_events"]), int(row["rt_sum"]),
                              int(row["rt_max"]))
        for m in extensions:
            adv = isinstance(m, AdvancedMetricExtension)
            if p or pe:
                if adv:
                    m.on_pass(name, p, events=pe)
                    calls += 1
                else:
                    m.increase_thread_num(name, times=pe)
                    m.add_pass(name, p, events=pe)
                    calls += 2
            for n, origin, e, ev in excs:
                if adv:
                    m.on_blocked(name, n, origin, e, events=ev)
                else:
                    m.add_block(name, n, origin, e, events=ev)
                calls += 1
            if ex:
                if adv:
                    m.on_complete(name, rs, su, events=ex, rt_max=rm)
                    calls += 1
                    if ee:
                        m.on_error(name, None, ec, events=ee)
                        calls += 1
                else:
                    m.add_rt(name, rs, events=ex, rt_max=rm)
                    m.add_success(name, su, events=ex)
                    m.decrease_thread_num(name, times=ex)
                    calls += 3
                    if ee:
                        m.add_exception(name, ec, None, events=ee)
                        calls += 1
    if lost_events or lost_count:
        for m in extensions:
            e = BlockException(LOST_RESOURCE)
            if isinstance(m, AdvancedMetricExtension):
                m.on_blocked(LOST_RESOURCE, int(lost_count), "", e, events=int(lost_events))
            else:
                m.add_block(LOST_RESOURCE, int(lost_count), "", e, events=int(lost_events))
            calls += 1
    return calls
