"""sentinel-server.log on the host: rows -> StatLogWriteTask's lines (server_log.ServerLogWriter), the row's two
Python mirrors against the C compiler's layout, and the reduce helper the GPU tests take their expected rows from.
No GPU: the rows are hand-made."""
import ctypes
import datetime
import os
import subprocess

import numpy as np

from tests import server_log_cases as sc
from tests.server_log_cases import (FLOW_BLOCK, FLOW_BLOCK_PRIO, FLOW_PASS, FLOW_WAITING, PARAM_BLOCK, PARAM_PASS, T0,
                                    rows_array)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UTC = datetime.timezone.utc
STAMP = "2023-11-14 22:13:20"  # T0 in UTC


class FakeEngine:
    """What ServerLogWriter asks of an engine: server_log_rows and (optionally) param_texts."""

    def __init__(self, tuples, lost=(0, 0), param_texts=None):
        self.tuples, self.lost = list(tuples), lost
        if param_texts is not None:
            self.param_texts = param_texts

    def server_log_rows(self, before_ms=None):
        due = [t for t in self.tuples if before_ms is None or t[0] + 1000 <= before_ms]
        self.tuples = [t for t in self.tuples if t not in due]
        lost, self.lost = self.lost, (0, 0)
        return rows_array(sorted(due)), lost[0], lost[1]


def _writer(tmp_path, engines=(), **kw):
    from sentinel_amd.server_log import ServerLogWriter
    kw.setdefault("tz", UTC)
    return ServerLogWriter(list(engines), str(tmp_path), **kw)


def _read(tmp_path, suffix=""):
    with open(os.path.join(str(tmp_path), "sentinel-server.log" + suffix), "rb") as f:
        return f.read()


def test_every_kind_exact_bytes(tmp_path):
    """One flowId with every kind in one second: the fixed order of the lines, count against events."""
    w = _writer(tmp_path)
    rows = rows_array([(T0, 7, FLOW_BLOCK, 0, 12, 5), (T0, 7, FLOW_BLOCK_PRIO, 0, 6, 2), (T0, 7, FLOW_WAITING, 0, 3, 3),
                       (T0, 7, FLOW_PASS, 0, 40, 9), (T0, 7, PARAM_PASS, 0, 4, 4), (T0, 7, PARAM_BLOCK, 55, 2, 2),
                       (T0, 7, PARAM_BLOCK, (1 << 64) - 3, 1, 1)])
    assert w.write_rows(rows) == 9
    w.close()
    assert _read(tmp_path) == (
        f"{STAMP}|1|flow|block|7|18,0\n{STAMP}|1|flow|block_request|7|7,0\n{STAMP}|1|flow|occupied_block|7|2,0\n"
        f"{STAMP}|1|flow|waiting|7|3,0\n{STAMP}|1|flow|pass|7|40,0\n{STAMP}|1|flow|pass_request|7|9,0\n"
        f"{STAMP}|1|param|pass|7|4,0\n{STAMP}|1|param|block|7|55|2,0\n{STAMP}|1|param|block|7|-3|1,0\n").encode()


def test_block_and_prio_merge_and_occupied_only_when_nonzero(tmp_path):
    w = _writer(tmp_path)
    w.write_rows(rows_array([(T0, 1, FLOW_BLOCK, 0, 10, 4),                                     # no PRIO row
                             (T0, 2, FLOW_BLOCK_PRIO, 0, 9, 3),                                 # PRIO only
                             (T0 + 1000, 1, FLOW_BLOCK, 0, 1, 1), (T0 + 1000, 1, FLOW_BLOCK_PRIO, 0, 2, 1)]))
    w.close()
    s2 = "2023-11-14 22:13:21"
    assert _read(tmp_path).decode().splitlines() == [
        f"{STAMP}|1|flow|block|1|10,0", f"{STAMP}|1|flow|block_request|1|4,0",
        f"{STAMP}|1|flow|block|2|9,0", f"{STAMP}|1|flow|block_request|2|3,0", f"{STAMP}|1|flow|occupied_block|2|3,0",
        f"{s2}|1|flow|block|1|3,0", f"{s2}|1|flow|block_request|1|2,0", f"{s2}|1|flow|occupied_block|1|1,0"]


def test_crlf_and_time_zones(tmp_path):
    rows = rows_array([(T0, 9, FLOW_WAITING, 0, 1, 1)])
    w = _writer(tmp_path / "a", newline="\r\n")
    w.write_rows(rows)
    w.close()
    assert _read(tmp_path / "a") == f"{STAMP}|1|flow|waiting|9|1,0\r\n".encode()
    plus8 = datetime.timezone(datetime.timedelta(hours=8))
    w = _writer(tmp_path / "b", tz=plus8)
    w.write_rows(rows)
    w.close()
    assert _read(tmp_path / "b") == b"2023-11-15 06:13:20|1|flow|waiting|9|1,0\n"
    w = _writer(tmp_path / "c", tz=None)  # the local zone, as FastDateFormat
    w.write_rows(rows)
    w.close()
    local = datetime.datetime.fromtimestamp(T0 // 1000).strftime("%Y-%m-%d %H:%M:%S")
    assert _read(tmp_path / "c") == f"{local}|1|flow|waiting|9|1,0\n".encode()


def test_lost_line(tmp_path):
    e = FakeEngine([(T0, 3, FLOW_BLOCK, 0, 2, 2)], lost=(5, 11))
    w = _writer(tmp_path, [e])
    assert w.poll(T0 + 1000) == 3
    assert w.poll(T0 + 2000) == 0  # the counters were cleared
    w.close()
    assert _read(tmp_path).decode().splitlines() == [
        f"{STAMP}|1|flow|block|3|2,0", f"{STAMP}|1|flow|block_request|3|2,0", f"{STAMP}|1|__lost__|events=5|11,0"]


def test_poll_leaves_the_running_second_and_close_writes_it(tmp_path):
    e = FakeEngine([(T0, 3, FLOW_WAITING, 0, 1, 1), (T0 + 1000, 3, FLOW_WAITING, 0, 2, 2)])
    w = _writer(tmp_path, [e])
    assert w.poll(T0 + 1999) == 1
    assert _read(tmp_path) == f"{STAMP}|1|flow|waiting|3|1,0\n".encode()
    assert w.close() == 1
    assert _read(tmp_path).decode().splitlines()[1] == "2023-11-14 22:13:21|1|flow|waiting|3|2,0"


def test_rolling(tmp_path):
    """EagleEyeRollingFileAppender: the size is checked before a write; base -> .1 -> .2, the oldest dropped."""
    line = len(f"{STAMP}|1|flow|waiting|1|1,0\n")
    w = _writer(tmp_path, max_file_size=2 * line, max_backup_index=2)
    for k in range(7):
        w.write_rows(rows_array([(T0, k + 1, FLOW_WAITING, 0, 1, 1)]))
    w.close()
    ids = lambda b: [int(x.split("|")[4]) for x in b.decode().splitlines()]  # noqa: E731
    assert ids(_read(tmp_path)) == [7]
    assert ids(_read(tmp_path, ".1")) == [5, 6]
    assert ids(_read(tmp_path, ".2")) == [3, 4]
    assert not os.path.exists(os.path.join(str(tmp_path), "sentinel-server.log.3"))


def test_param_block_text_resolution_order(tmp_path):
    """param_text(tag), then the engines' recorded texts, then the key as a signed decimal."""
    neg = (1 << 64) - 9
    e = FakeEngine([(T0, 4, PARAM_BLOCK, 10, 1, 1), (T0, 4, PARAM_BLOCK, 11, 1, 1), (T0, 4, PARAM_BLOCK, 12, 1, 1),
                    (T0, 4, PARAM_BLOCK, neg, 1, 1)], param_texts={10: "engine-ten", 11: "engine-eleven", -9: "minus"})
    w = _writer(tmp_path, [e], param_text=lambda tag: {10: "callback-ten"}.get(tag))
    w.close()
    assert [x.split("|", 2)[2] for x in _read(tmp_path).decode().splitlines()] == [
        "param|block|4|callback-ten|1,0", "param|block|4|engine-eleven|1,0", "param|block|4|12|1,0",
        "param|block|4|minus|1,0"]


def test_param_texts_filled_by_the_token_service():
    """DefaultTokenService.request_param_tokens records java_text of what it hashes, only with the log on."""
    from sentinel_amd import cluster
    from sentinel_amd.block_log import java_text
    assert java_text(True) == "true" and java_text("abc") == "abc" and java_text(12) == "12"
    assert cluster.PARAM_TEXTS_MAX >= 1024
    assert cluster.param_value_key("abc") != cluster.param_value_key("abd")


def test_rows_of_two_engines_merge(tmp_path):
    """Shards hold disjoint flowIds; rows that still come to one message in one second are one line, and two
    values with one text too."""
    a = FakeEngine([(T0, 1, FLOW_BLOCK, 0, 4, 2), (T0, 5, PARAM_BLOCK, 70, 1, 1)], lost=(1, 2))
    b = FakeEngine([(T0, 1, FLOW_BLOCK, 0, 6, 3), (T0, 2, FLOW_PASS, 0, 8, 8), (T0, 5, PARAM_BLOCK, 71, 2, 2)],
                   lost=(2, 3))
    w = _writer(tmp_path, [a, b], param_text=lambda tag: "same")
    assert w.poll(T0 + 1000) == 6
    w.close()
    assert _read(tmp_path).decode().splitlines() == [
        f"{STAMP}|1|flow|block|1|10,0", f"{STAMP}|1|flow|block_request|1|5,0", f"{STAMP}|1|flow|pass|2|8,0",
        f"{STAMP}|1|flow|pass_request|2|8,0", f"{STAMP}|1|param|block|5|same|3,0",
        f"{STAMP}|1|__lost__|events=3|5,0"]


def test_one_engine_is_accepted_without_a_list(tmp_path):
    from sentinel_amd.server_log import ServerLogWriter
    w = ServerLogWriter(FakeEngine([(T0, 1, FLOW_WAITING, 0, 1, 1)]), str(tmp_path), tz=UTC)
    assert w.close() == 1


def test_row_layout_matches_the_c_compiler(tmp_path):
    """sizeof / offsetof of sga_server_log_row as gcc lays it out == the ctypes mirror == the numpy dtype."""
    from sentinel_amd import _lib
    from sentinel_amd.server_log import SERVER_LOG_ROW_DTYPE
    cls = _lib.SgaServerLogRow
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sentinel_amd.h"', "int main(void) {",
             'printf("%zu\\n", sizeof(sga_server_log_row));']
    lines += [f'printf("%zu\\n", offsetof(sga_server_log_row, {f}));' for f, _ in cls._fields_]
    lines += ['printf("%d %d %d %d %d %d\\n", SGA_SLOG_FLOW_BLOCK, SGA_SLOG_FLOW_BLOCK_PRIO, SGA_SLOG_FLOW_WAITING, '
              'SGA_SLOG_FLOW_PASS, SGA_SLOG_PARAM_PASS, SGA_SLOG_PARAM_BLOCK);', "return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    names = [f for f, _ in cls._fields_]
    assert got[0] == 40 == ctypes.sizeof(cls) == SERVER_LOG_ROW_DTYPE.itemsize
    assert got[1:1 + len(names)] == [getattr(cls, f).offset for f in names]
    assert got[1:1 + len(names)] == [SERVER_LOG_ROW_DTYPE.fields[f][1] for f in names]
    assert tuple(SERVER_LOG_ROW_DTYPE.names) == tuple(names)
    assert got[1 + len(names):] == [FLOW_BLOCK, FLOW_BLOCK_PRIO, FLOW_WAITING, FLOW_PASS, PARAM_PASS, PARAM_BLOCK]
    from sentinel_amd import server_log as SL
    assert (SL.FLOW_BLOCK, SL.FLOW_BLOCK_PRIO, SL.FLOW_WAITING, SL.FLOW_PASS, SL.PARAM_PASS, SL.PARAM_BLOCK) == \
        tuple(range(6))


def test_reduce_helper_three_requests():
    """A blocked request of acquire 2, a prioritized one that waits and a prioritized one that is blocked, the
    last in the next second; a pass forms nothing under the default checker."""
    fid = np.array([7, 7, 7, 7])
    acq = np.array([2, 1, 3, 1])
    prio = np.array([0, 1, 1, 0])
    ts = np.array([T0 + 10, T0 + 999, T0 + 1000, T0 + 1001])
    acc = sc.reduce_rows({}, fid, acq, prio, ts, [1, 2, 1, 0])
    assert sc.expected_tuples(acc) == [(T0, 7, FLOW_BLOCK, 0, 2, 1), (T0, 7, FLOW_WAITING, 0, 1, 1),
                                       (T0 + 1000, 7, FLOW_BLOCK_PRIO, 0, 3, 1)]
    # the RLS checker logs passes and knows no priority; TOO_MANY_REQUEST / NO_RULE_EXISTS / BAD_REQUEST: nothing
    acc = sc.reduce_rows({}, fid, acq, prio, ts, [1, 0, -2, 3], checker="simple")
    assert sc.expected_tuples(acc) == [(T0, 7, FLOW_BLOCK, 0, 2, 1), (T0, 7, FLOW_PASS, 0, 1, 1)]
    # parameters: the first value in collection order that can block; an empty collection forms nothing
    acc = sc.reduce_rows({}, fid, acq, None, ts, [1, 0, 0, -4], checker="param",
                         values=[[5, 8, 9], [5, 6], [], []], can_block=lambda f, v: v in (8, 9))
    assert sc.expected_tuples(acc) == [(T0, 7, PARAM_PASS, 0, 1, 1), (T0, 7, PARAM_BLOCK, 8, 1, 1)]
    assert sc.as_tuples(rows_array(sc.expected_tuples(acc))) == sc.expected_tuples(acc)


class _Polls:
    """A writer stand-in: records the times it is polled at."""

    def __init__(self):
        self.at = []

    def poll(self, now):
        self.at.append(now)
        return 0


def test_rls_batcher_polls_once_a_second():
    """RlsBatcher(server_log=...) polls the writer when the clock's second changes, and once more on close; without
    the argument nothing is polled."""
    from sentinel_amd import rls_server as R

    class Mgr(R.EnvoyRlsRuleManager):
        def _push(self, flow):
            pass

    clock = iter([T0 + 10, T0 + 500, T0 + 1200, T0 + 1300])

    def decide(off, fids, hits, ts):
        n = len(fids)
        return np.ones(len(hits), np.int32), np.full(n, 3, np.int8), np.zeros(n, np.int32)

    w = _Polls()
    b = R.RlsBatcher(Mgr(None), window_us=1, clock=lambda: next(clock), decide=decide, server_log=w)
    for _ in range(3):
        assert b.submit("web", [[("path", "/a")]], 1)[0] == 1
    b.close()
    assert w.at == [T0 + 10, T0 + 1200, T0 + 1300]
    assert R.RlsBatcher(Mgr(None), decide=decide).server_log is None


def test_token_server_takes_a_writer():
    import inspect

    from sentinel_amd.token_server import ClusterTokenServer
    assert inspect.signature(ClusterTokenServer.__init__).parameters["server_log"].default is None
