"""sentinel-server.log from the engine's token server log.

  ClusterServerStatLogUtil.log(msg[, count])   CS/../server/log/ClusterServerStatLogUtil.java: stat(msg).count(count)
                           -- a StatLogger "sentinel-cluster-server-record", one-second interval, entry delimiter
                           '|', 300 MB files, 3 backups.  Called by ClusterFlowChecker (flow|waiting, flow|block,
                           flow|block_request, flow|occupied_block), ClusterParamFlowChecker (param|pass,
                           param|block|<id>|<value>) and the RLS SimpleClusterFlowChecker (flow|pass,
                           flow|pass_request, flow|block, flow|block_request) and ConcurrentClusterFlowChecker
                           (concurrent|pass|<id>, concurrent|block|<id>, concurrent|release|<id>)
  ClusterConcurrentCheckerLogListener   CS/flow/statistic/concurrent/ClusterConcurrentCheckerLogListener.java:39-54,
                           scheduled once a second: concurrent|resource:..|flowId:..|concurrencyLevel:..|
                           currentConcurrency with count = nowCalls for every flowId whose nowCalls != 0, and
                           flow|totalTokenSize with count = the token cache's size when it is not empty
  StatLogController        CORE/eagleeye/StatLogController.java:126-152 (StatLogWriteTask): one line per key,
                           "yyyy-MM-dd HH:mm:ss|1|<msg>|count,sum\\n" -- the key is the message itself, bars
                           included; stat type 1, the value sum 0 because only count() is called

The sums per (second, flowId, kind, blocking value) are formed on the device (sga_server_log_enable /
sga_server_log_drain); ServerLogWriter drains the finished seconds of one engine or of every shard's engine, turns
the rows into the reference's messages and appends the lines.  The listener's gauges are state, not events:
ServerLogWriter.sample_gauges reads them from the engines (sga_concurrent_gauges) when the caller's once-a-second
tick says so.
"""
import decimal
import math
import os
from typing import Callable, Dict, List, Optional

import numpy as np

from .block_log import BlockLogWriter

SERVER_LOG_FILE = "sentinel-server.log"
LOST_KEY = "__lost__"  # the extra line of tuples that found no room in an engine's table

# one sga_server_log_row (sga_server_log_drain)
SERVER_LOG_ROW_DTYPE = np.dtype([("time_slot", "<i8"), ("flow_id", "<i8"), ("tag", "<u8"), ("count", "<i8"),
                                 ("events", "<u4"), ("kind", "u1"), ("reserved", "u1", (3,))])
FLOW_BLOCK, FLOW_BLOCK_PRIO, FLOW_WAITING, FLOW_PASS, PARAM_PASS, PARAM_BLOCK = range(6)  # SGA_SLOG_*
CONC_PASS, CONC_BLOCK, CONC_RELEASE = 6, 7, 8
_CONC_WORD = {CONC_PASS: "pass", CONC_BLOCK: "block", CONC_RELEASE: "release"}
TOKEN_SIZE_MESSAGE = "flow|totalTokenSize"


def default_value_text(tag: int) -> str:
    """The text of a blocking value nobody recorded: its 64-bit key as a signed Java long."""
    tag = int(tag) & 0xFFFFFFFFFFFFFFFF
    return str(tag - (1 << 64) if tag >> 63 else tag)


def java_fixed6(x: float) -> str:
    """String.format("%f", x) for a double: six fraction digits.  Formed from the double's shortest decimal text
    (repr, what Double.toString's digits are) rounded HALF_UP, which is how the JDK's Formatter is read to work
    (FormattedFloatingDecimal, then BigDecimal.setScale(6, HALF_UP)) -- not Python's %f, which rounds the exact
    binary value half-even.  The two agree whenever the shortest text has at most six fraction digits; beyond that
    the HALF_UP-over-shortest-digits rule is a reading of the JDK that no reference test confirms (DESIGN.md
    section 9: parity-unpinned)."""
    x = float(x)
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "Infinity" if x > 0 else "-Infinity"
    with decimal.localcontext() as ctx:
        ctx.prec = 400  # a double has at most 309 integer digits
        return format(decimal.Decimal(repr(x)).quantize(decimal.Decimal("0.000001"),
                                                        rounding=decimal.ROUND_HALF_UP), "f")


def gauge_message(resource: str, flow_id: int, level: float) -> str:
    """ClusterConcurrentCheckerLogListener's key.  The 'l' after each number is the reference's own format string
    ("flowId:%dl|concurrencyLevel:%fl")."""
    return "concurrent|resource:%s|flowId:%dl|concurrencyLevel:%sl|currentConcurrency" % (
        resource, int(flow_id), java_fixed6(level))


class ServerLogWriter(BlockLogWriter):
    """Writes sentinel-server.log under base_dir from the token server log of `engines`.

    engines: one cluster.Engine after server_log_enable() or a list of them -- anything with
    server_log_rows(before_ms) -> (rows, lost_events, lost_count) and (optionally) a param_texts dict {key: text}
    that DefaultTokenService.request_param_tokens fills.  A multi-GPU server has one engine per shard with disjoint
    flowIds; rows that come to the same message in one second are one line.  The text of a param|block line's value
    is param_text(tag) when given and not None, then the engines' dicts, then the key as a signed decimal.  tz,
    newline, max_file_size and max_backup_index as block_log.BlockLogWriter (the rolling file is the same
    EagleEyeRollingFileAppender).  poll(now) writes the seconds finished at `now`; close() writes everything.

    sample_gauges(now) adds the concurrency listener's lines of second `now` from every engine that has
    concurrent_gauges() -> (rows, token_size); nothing calls it on its own: the caller's once-a-second tick does,
    next to poll.  The resource of a gauge line is resource_of(flow_id) when given and not None, then the engines'
    flow_resources dicts (ClusterFlowRuleManager.load_rules fills them), then the decimal flowId -- a divergence
    only for rules loaded without names, which a valid reference rule always has."""

    def __init__(self, engines, base_dir: str, param_text: Optional[Callable[[int], Optional[str]]] = None,
                 tz=None, max_file_size: int = 300 << 20, max_backup_index: int = 3, newline: str = "\n",
                 resource_of: Optional[Callable[[int], Optional[str]]] = None):
        self.engines: List = list(engines) if isinstance(engines, (list, tuple)) else [engines]
        self.newline = newline
        self.param_text = param_text
        self.resource_of = resource_of
        # pending gauge sums: (second, message) -> [order key, count]; the order key sorts a second's lines
        self._gauges: Dict[tuple, list] = {}
        self.tz = tz
        self.max_file_size = int(max_file_size)
        self.max_backup_index = int(max_backup_index)
        os.makedirs(base_dir, exist_ok=True)
        self.path = os.path.join(base_dir, SERVER_LOG_FILE)
        self._f = open(self.path, "ab")
        self._size = self._f.tell()

    def _value_text(self, tag: int) -> str:
        text = self.param_text(tag) if self.param_text else None
        if text is None:
            signed = tag - (1 << 64) if tag >> 63 else tag  # param_value_key's keys are signed
            for e in self.engines:
                texts = getattr(e, "param_texts", None) or {}
                text = texts.get(signed, texts.get(tag))
                if text is not None:
                    break
        return default_value_text(tag) if text is None else text

    def messages(self, rows) -> List[tuple]:
        """(time_slot, message, count) per line, in the order of the file: by second, then flowId, then
        flow|block, flow|block_request, flow|occupied_block (only when prioritized requests were blocked),
        flow|waiting, flow|pass, flow|pass_request, param|pass, param|block|<id>|<text> by value key,
        concurrent|pass, concurrent|block, concurrent|release."""
        rows = np.sort(np.asarray(rows, dtype=SERVER_LOG_ROW_DTYPE), order=["time_slot", "flow_id", "kind", "tag"])
        groups: Dict[tuple, dict] = {}
        for r in rows:
            g = groups.setdefault((int(r["time_slot"]), int(r["flow_id"])),
                                  {"bc": 0, "be": 0, "pe": 0, "w": 0, "pc": 0, "pr": 0, "pp": 0, "pb": {},
                                   "conc": {}, "kinds": set()})
            kind, count, events = int(r["kind"]), int(r["count"]), int(r["events"])
            g["kinds"].add(kind)
            if kind in (FLOW_BLOCK, FLOW_BLOCK_PRIO):
                g["bc"] += count
                g["be"] += events
                if kind == FLOW_BLOCK_PRIO:
                    g["pe"] += events
            elif kind == FLOW_WAITING:
                g["w"] += count
            elif kind == FLOW_PASS:
                g["pc"] += count
                g["pr"] += events
            elif kind == PARAM_PASS:
                g["pp"] += count
            elif kind == PARAM_BLOCK:
                text = self._value_text(int(r["tag"]))
                g["pb"][text] = g["pb"].get(text, 0) + count
            elif kind in _CONC_WORD:
                g["conc"][kind] = g["conc"].get(kind, 0) + count
            else:
                raise ValueError("unknown server log row kind %d" % kind)
        out = []
        for (slot, fid), g in groups.items():
            kinds = g["kinds"]
            if FLOW_BLOCK in kinds or FLOW_BLOCK_PRIO in kinds:
                out.append((slot, "flow|block|%d" % fid, g["bc"]))
                out.append((slot, "flow|block_request|%d" % fid, g["be"]))
                if g["pe"]:
                    out.append((slot, "flow|occupied_block|%d" % fid, g["pe"]))
            if FLOW_WAITING in kinds:
                out.append((slot, "flow|waiting|%d" % fid, g["w"]))
            if FLOW_PASS in kinds:
                out.append((slot, "flow|pass|%d" % fid, g["pc"]))
                out.append((slot, "flow|pass_request|%d" % fid, g["pr"]))
            if PARAM_PASS in kinds:
                out.append((slot, "param|pass|%d" % fid, g["pp"]))
            for text, count in g["pb"].items():
                out.append((slot, "param|block|%d|%s" % (fid, text), count))
            for kind in (CONC_PASS, CONC_BLOCK, CONC_RELEASE):
                if kind in g["conc"]:
                    out.append((slot, "concurrent|%s|%d" % (_CONC_WORD[kind], fid), g["conc"][kind]))
        return out

    # ---- the listener's gauges
    def _resource_text(self, flow_id: int) -> str:
        text = self.resource_of(flow_id) if self.resource_of else None
        if text is None:
            for e in self.engines:
                text = (getattr(e, "flow_resources", None) or {}).get(flow_id)
                if text is not None:
                    break
        return str(flow_id) if text is None else text

    def sample_gauges(self, now: int) -> int:
        """One run of ClusterConcurrentCheckerLogListener at `now` (ms): reads concurrent_gauges() of every engine
        that has it and adds the lines to the pending sums of second now - now % 1000 -- two samples in one second
        add, as stat(msg).count(v) does when the task fires twice inside a StatLogger slot.  The token cache sizes
        are summed over the engines into one flow|totalTokenSize, left out when the sum is 0.  poll / close write
        the lines.  Returns the number of messages sampled."""
        now = int(now)
        slot = now - now % 1000
        total, lines = 0, 0
        for e in self.engines:
            read = getattr(e, "concurrent_gauges", None)
            if read is None:
                continue
            rows, size = read()
            total += int(size)
            for r in rows:
                fid = int(r["flow_id"])
                msg = gauge_message(self._resource_text(fid), fid, float(r["level"]))
                self._gauges.setdefault((slot, msg), [(0, fid), 0])[1] += int(r["now_calls"])
                lines += 1
        if total:
            self._gauges.setdefault((slot, TOKEN_SIZE_MESSAGE), [(1, 0), 0])[1] += total
            lines += 1
        return lines

    def _take_gauges(self, before_ms: Optional[int]) -> List[tuple]:
        """The pending gauge lines of the seconds finished at before_ms (None: all), removed: (time_slot, message,
        count) by second, the per-flow lines by flowId, then flow|totalTokenSize."""
        due = [k for k in self._gauges if before_ms is None or k[0] + 1000 <= before_ms]
        due.sort(key=lambda k: (k[0], self._gauges[k][0], k[1]))
        return [(k[0], k[1], self._gauges.pop(k)[1]) for k in due]

    def write_rows(self, rows, lost_events: int = 0, lost_count: int = 0, lost_slot: Optional[int] = None,
                   gauges=()) -> int:
        """Appends the lines of drained rows (of one engine or several concatenated).  gauges: (time_slot, message,
        count) lines of the listener, written after the row lines of their second (a second without rows too).
        Nonzero lost counters add a line __lost__|events=<n> carrying the lost count at lost_slot (the last second
        of the rows when None).  Returns the number of lines."""
        msgs = self.messages(rows)
        if gauges:  # a stable sort by second: a second's rows, then its gauges
            msgs = sorted(msgs + list(gauges), key=lambda m: m[0])
        for slot, msg, count in msgs:
            self._append(("%s|1|%s|%d,0%s" % (self._stamp(slot), msg, count, self.newline)).encode("utf-8"))
        lines = len(msgs)
        if lost_events or lost_count:
            slot = lost_slot if lost_slot is not None else (msgs[-1][0] if msgs else 0)
            self._append(("%s|1|%s|events=%d|%d,0%s" % (self._stamp(slot), LOST_KEY, lost_events, lost_count,
                                                        self.newline)).encode("utf-8"))
            lines += 1
        self._f.flush()
        return lines

    def _drain(self, before_ms):
        parts, lost_events, lost_count = [], 0, 0
        for e in self.engines:
            rows, le, lc = e.server_log_rows(before_ms)
            parts.append(rows)
            lost_events += le
            lost_count += lc
        rows = np.concatenate(parts) if parts else np.zeros(0, dtype=SERVER_LOG_ROW_DTYPE)
        return rows, lost_events, lost_count

    def poll(self, now: int) -> int:
        """Drains the seconds finished at `now` (ms) from every engine and appends their lines; returns the number
        of lines."""
        now = int(now)
        rows, lost_events, lost_count = self._drain(now)
        return self.write_rows(rows, lost_events, lost_count, lost_slot=(now - now % 1000) - 1000,
                               gauges=self._take_gauges(now))

    def close(self) -> int:
        """Drains everything, appends it and closes the file."""
        rows, lost_events, lost_count = self._drain(None)
        n = self.write_rows(rows, lost_events, lost_count, gauges=self._take_gauges(None))
        self._f.close()
        return n
