"""sentinel-block.log from the engine's block log.

  LogSlot.entry            CORE/slots/logger/LogSlot.java:34-47: every BlockException goes to
  EagleEyeLogUtil.log      CORE/slots/logger/EagleEyeLogUtil.java: statLogger.stat(resource, exceptionName,
                           ruleLimitApp, origin).count(count) -- a StatLogger "sentinel-block-log", one-second
                           interval, entry delimiter '|', key delimiter ','
  StatLogController        CORE/eagleeye/StatLogController.java:126-152 (StatLogWriteTask): one line per key,
                           "yyyy-MM-dd HH:mm:ss|1|k0,k1,k2,k3|count,sum\\n" -- stat type 1, the value sum 0 because
                           only count() is called
  EagleEyeRollingFileAppender.rollOver: base -> base.1 -> ... -> base.maxBackupIndex, the oldest deleted

The sum per (second, key) is formed on the device (sga_block_log_enable / sga_block_log_drain); BlockLogWriter
drains the finished seconds, turns ids and block details into the reference's texts and appends the lines.
"""
import datetime
import os
from typing import Callable, Dict, Optional

import numpy as np

BLOCK_LOG_FILE = "sentinel-block.log"
LOST_RESOURCE = "__lost__"  # the extra line of entries that found no room in the engine's table

# one sga_block_row (sga_block_log_drain)
BLOCK_ROW_DTYPE = np.dtype([("time_slot", "<i8"), ("tag", "<u8"), ("count", "<i8"), ("resource", "<u4"),
                            ("origin", "<u4"), ("detail", "<u4"), ("events", "<u4"), ("decision", "u1"),
                            ("tag_kind", "u1"), ("reserved", "u1", (6,))])
TAG_SCALAR, TAG_LIST = 0, 1

# decision code -> BlockException subclass simple name (LogSlot logs e.getClass().getSimpleName())
EXCEPTION_NAME = {1: "FlowException", 2: "ParamFlowException", 3: "DegradeException", 5: "SystemBlockException",
                  6: "AuthorityException"}
# SystemBlockException's limitType per block detail (SystemRuleManager.checkSystem, SystemRuleManager.java:317-342)
SYSTEM_LIMIT_TYPE = ("qps", "thread", "rt", "load", "cpu")

_M64 = 0xFFFFFFFFFFFFFFFF


def _splitmix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def list_tag(keys) -> int:
    """The engine's 64-bit fold of a Collection / array argument (flow.hip blog_list_tag): its length, then its
    element keys (param_value) in order."""
    h = _splitmix64(len(keys))
    for k in keys:
        h = _splitmix64(h ^ (int(k) & _M64))
    return h


def java_text(x) -> str:
    """String.valueOf of a Python stand-in for a Java argument: true / false, decimal integers, Double.toString
    for the common cases, strings as they are, lists as AbstractCollection.toString writes them ([a, b])."""
    if x is None:
        return "null"
    if isinstance(x, (bool, np.bool_)):
        return "true" if x else "false"
    if isinstance(x, (int, np.integer)):
        return str(int(x))
    if isinstance(x, (float, np.floating)):
        return repr(float(x))
    if isinstance(x, (list, tuple)):
        return "[" + ", ".join(java_text(v) for v in x) + "]"
    return str(x)


def default_param_text(tag: int, tag_kind: int) -> str:
    """The text of a parameter tag nobody recorded: a scalar's key as a signed Java long, a list's fold as '#' and
    16 hex digits (the engine only ever saw 64-bit keys)."""
    tag = int(tag) & _M64
    if tag_kind == TAG_LIST:
        return "#%016x" % tag
    return str(tag - (1 << 64) if tag >> 63 else tag)


class BlockLogWriter:
    """Writes sentinel-block.log under base_dir from `sentinel`'s block log.

    sentinel: a LocalSentinel(block_log=...) -- anything with block_rows(before_ms) -> (rows, lost_events,
    lost_count), resources, origins, block_rule(decision, resource, detail) and (optionally) a param_texts dict
    {(tag, tag_kind): text} filled by its entry().  param_text(tag, tag_kind) -> str or None is asked first for a
    ParamFlowException's limitApp, then the sentinel's dict, then default_param_text.  tz: the zone of the line's
    time (None: the local zone, as FastDateFormat).  newline ends a line: the reference's appender writes
    EagleEyeCoreUtils.NEWLINE, "\\r\\n" -- pass that for byte parity with a Java-written file.  poll(now) writes the
    seconds finished at `now`; close() writes everything (StatLogController.stop)."""

    def __init__(self, sentinel, base_dir: str, param_text: Optional[Callable[[int, int], Optional[str]]] = None,
                 tz: Optional[datetime.tzinfo] = None, max_file_size: int = 300 << 20, max_backup_index: int = 3,
                 newline: str = "\n"):
        self.s = sentinel
        self.newline = newline
        self.param_text = param_text
        self.tz = tz
        self.max_file_size = int(max_file_size)
        self.max_backup_index = int(max_backup_index)
        os.makedirs(base_dir, exist_ok=True)
        self.path = os.path.join(base_dir, BLOCK_LOG_FILE)
        self._f = open(self.path, "ab")
        self._size = self._f.tell()

    # ---- texts
    def _limit_app(self, row) -> str:
        d, detail = int(row["decision"]), int(row["detail"])
        if d == 5:
            return SYSTEM_LIMIT_TYPE[detail] if detail < len(SYSTEM_LIMIT_TYPE) else str(detail)
        if d == 6:  # AuthorityException(context.getOrigin(), rule)
            return self._origin(row)
        if d == 2:  # ParamFlowException(resource, String.valueOf(args[paramIdx]), rule)
            tag, kind = int(row["tag"]), int(row["tag_kind"])
            text = self.param_text(tag, kind) if self.param_text else None
            if text is None:
                text = getattr(self.s, "param_texts", {}).get((tag, kind))
            return default_param_text(tag, kind) if text is None else text
        rule = self.s.block_rule(d, int(row["resource"]), detail)
        return getattr(rule, "limit_app", None) or "default"

    def _origin(self, row) -> str:
        o = int(row["origin"])
        return self.s.origins[o - 1] if o else ""

    def _stamp(self, time_slot: int) -> str:
        t = datetime.datetime.fromtimestamp(time_slot // 1000, tz=self.tz)
        return t.strftime("%Y-%m-%d %H:%M:%S")

    # ---- file
    def _roll_over(self):
        """EagleEyeRollingFileAppender.rollOver: drop .maxBackupIndex, shift the rest up, base -> .1"""
        self._f.close()
        if self.max_backup_index > 0:
            oldest = "%s.%d" % (self.path, self.max_backup_index)
            if os.path.exists(oldest):
                os.remove(oldest)
            for i in range(self.max_backup_index - 1, 0, -1):
                src = "%s.%d" % (self.path, i)
                if os.path.exists(src):
                    os.replace(src, "%s.%d" % (self.path, i + 1))
            os.replace(self.path, self.path + ".1")
        self._f = open(self.path, "wb")
        self._size = 0

    def _append(self, line: bytes):
        if self._size >= self.max_file_size:  # checked before a write, like the appender's size check
            self._roll_over()
        self._f.write(line)
        self._size += len(line)

    # ---- rows -> lines
    def write_rows(self, rows, lost_events: int = 0, lost_count: int = 0, lost_slot: Optional[int] = None) -> int:
        """Appends the lines of drained rows (sorted as the drain sorts them): rows that come to the same text key
        in one second -- details that share a limitApp -- are one line.  Nonzero lost counters add a line of
        resource __lost__ at lost_slot (the last row's second when None).  Returns the number of lines."""
        merged: Dict[tuple, int] = {}
        for row in rows:
            key = (int(row["time_slot"]), self.s.resources[int(row["resource"])], EXCEPTION_NAME[int(row["decision"])],
                   self._limit_app(row), self._origin(row))
            merged[key] = merged.get(key, 0) + int(row["count"])
        lines = 0
        for (slot, res, exc, lim, org), count in merged.items():
            self._append(("%s|1|%s,%s,%s,%s|%d,0%s" % (self._stamp(slot), res, exc, lim, org, count,
                                                      self.newline)).encode("utf-8"))
            lines += 1
        if lost_events or lost_count:
            slot = lost_slot if lost_slot is not None else (int(rows[-1]["time_slot"]) if len(rows) else 0)
            self._append(("%s|1|%s,%s,%s,%s|%d,0%s" % (self._stamp(slot), LOST_RESOURCE, "BlockException",
                                                      "events=%d" % lost_events, "", lost_count,
                                                      self.newline)).encode("utf-8"))
            lines += 1
        self._f.flush()
        return lines

    def poll(self, now: int) -> int:
        """Drains the seconds finished at `now` (ms) and appends their lines; returns the number of lines."""
        rows, lost_events, lost_count = self.s.block_rows(now)
        return self.write_rows(rows, lost_events, lost_count, lost_slot=(now - now % 1000) - 1000)

    def close(self) -> int:
        """Drains everything, appends it and closes the file."""
        rows, lost_events, lost_count = self.s.block_rows(None)
        n = self.write_rows(rows, lost_events, lost_count)
        self._f.close()
        return n
