"""The concurrency checker's part of sentinel-server.log on the host: the three concurrent|... messages, the
listener's gauge lines (server_log.ServerLogWriter.sample_gauges), the gauge row's Python mirrors against the C
compiler's layout, and the reduce helper the GPU tests take their expected rows from.  No GPU: rows and gauges are
hand-made."""
import ctypes
import datetime
import os
import subprocess

import numpy as np
import pytest

from tests import conc_log_cases as cc
from tests.conc_log_cases import CONC_BLOCK, CONC_PASS, CONC_RELEASE, T0
from tests.server_log_cases import FLOW_BLOCK, PARAM_BLOCK, PARAM_PASS, expected_tuples, rows_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UTC = datetime.timezone.utc
STAMP = "2023-11-14 22:13:20"  # T0 in UTC
STAMP1 = "2023-11-14 22:13:21"


class GaugeEngine:
    """What ServerLogWriter asks of an engine with concurrency gauges."""

    def __init__(self, gauges=(), size=0, tuples=(), flow_resources=None):
        self.g, self.size, self.tuples = list(gauges), size, list(tuples)
        if flow_resources is not None:
            self.flow_resources = flow_resources

    def concurrent_gauges(self):
        from sentinel_amd.cluster import CONC_GAUGE_DTYPE
        a = np.zeros(len(self.g), dtype=CONC_GAUGE_DTYPE)
        for i, (fid, level, calls) in enumerate(sorted(self.g)):
            a[i] = (fid, level, calls, 0)
        return a, self.size

    def server_log_rows(self, before_ms=None):
        due = [t for t in self.tuples if before_ms is None or t[0] + 1000 <= before_ms]
        self.tuples = [t for t in self.tuples if t not in due]
        return rows_array(sorted(due)), 0, 0


class PlainEngine:
    """An engine without concurrent_gauges (the server log host tests' FakeEngine): sample_gauges skips it."""

    def server_log_rows(self, before_ms=None):
        return rows_array([]), 0, 0


def _writer(tmp_path, engines=(), **kw):
    from sentinel_amd.server_log import ServerLogWriter
    kw.setdefault("tz", UTC)
    return ServerLogWriter(list(engines), str(tmp_path), **kw)


def _lines(tmp_path):
    with open(os.path.join(str(tmp_path), "sentinel-server.log"), "rb") as f:
        return f.read().decode().splitlines()


def _gauge(res, fid, level):
    return f"concurrent|resource:{res}|flowId:{fid}l|concurrencyLevel:{level}l|currentConcurrency"


# ------------------------------------------------------------------ the three kinds
def test_concurrent_messages_and_their_place(tmp_path):
    """concurrent|pass, |block, |release carry the row's count and come after the flow's param lines, in that
    order; another flowId's lines follow."""
    w = _writer(tmp_path)
    rows = rows_array([(T0, 7, CONC_RELEASE, 0, 9, 4), (T0, 7, CONC_BLOCK, 0, 6, 2), (T0, 7, CONC_PASS, 0, 12, 5),
                       (T0, 7, FLOW_BLOCK, 0, 3, 1), (T0, 7, PARAM_PASS, 0, 4, 4), (T0, 7, PARAM_BLOCK, 55, 2, 2),
                       (T0, 8, CONC_BLOCK, 0, 1, 1), (T0 + 1000, 7, CONC_RELEASE, 0, 2, 1)])
    assert w.write_rows(rows) == 9
    w.close()
    assert _lines(tmp_path) == [
        f"{STAMP}|1|flow|block|7|3,0", f"{STAMP}|1|flow|block_request|7|1,0", f"{STAMP}|1|param|pass|7|4,0",
        f"{STAMP}|1|param|block|7|55|2,0", f"{STAMP}|1|concurrent|pass|7|12,0", f"{STAMP}|1|concurrent|block|7|6,0",
        f"{STAMP}|1|concurrent|release|7|9,0", f"{STAMP}|1|concurrent|block|8|1,0",
        f"{STAMP1}|1|concurrent|release|7|2,0"]


def test_kind_nine_raises(tmp_path):
    w = _writer(tmp_path)
    with pytest.raises(ValueError):
        w.messages(rows_array([(T0, 7, 9, 0, 1, 1)]))
    w.close()


def test_constants():
    from sentinel_amd import server_log as SL
    assert (SL.CONC_PASS, SL.CONC_BLOCK, SL.CONC_RELEASE) == (6, 7, 8) == (CONC_PASS, CONC_BLOCK, CONC_RELEASE)


# ------------------------------------------------------------------ gauges
def test_gauge_line_bytes_for_three_levels(tmp_path):
    """Java's %f: six fraction digits; 0.1 * 3 = 0.30000000000000004 prints as 0.300000.  The literal l after each
    number is the reference's format string."""
    e = GaugeEngine([(5, 31.5, 4), (3, 10.0, 1), (6, 0.1 * 3, -2)], size=0, flow_resources={5: "res5", 3: "a|b", 6: "r6"})
    w = _writer(tmp_path, [e])
    assert w.sample_gauges(T0 + 10) == 3
    assert w.poll(T0 + 999) == 0, "the second is not finished"
    assert w.poll(T0 + 1000) == 3
    w.close()
    with open(os.path.join(str(tmp_path), "sentinel-server.log"), "rb") as f:
        assert f.read() == (
            f"{STAMP}|1|concurrent|resource:a|b|flowId:3l|concurrencyLevel:10.000000l|currentConcurrency|1,0\n"
            f"{STAMP}|1|concurrent|resource:res5|flowId:5l|concurrencyLevel:31.500000l|currentConcurrency|4,0\n"
            f"{STAMP}|1|concurrent|resource:r6|flowId:6l|concurrencyLevel:0.300000l|currentConcurrency|-2,0\n").encode()


def test_fixed6_is_half_up_over_the_shortest_text():
    from sentinel_amd.server_log import java_fixed6
    assert [java_fixed6(x) for x in (10.0, 31.5, 0.1 * 3, 0.0, 2.0 ** 40, 0.000001, 1e22)] == [
        "10.000000", "31.500000", "0.300000", "0.000000", "1099511627776.000000", "0.000001",
        "10000000000000000000000.000000"]
    assert java_fixed6(0.0000005) == "0.000001", "HALF_UP where Python's %f gives 0.000000"


def test_resource_fallbacks(tmp_path):
    """resource_of(flow_id), then the engines' flow_resources, then the decimal flowId."""
    a = GaugeEngine([(1, 2.0, 1), (2, 2.0, 1)], flow_resources={1: "engine-one", 2: "engine-two"})
    b = GaugeEngine([(3, 2.0, 1), (4, 2.0, 1)], flow_resources={3: "b-three"})
    w = _writer(tmp_path, [a, b], resource_of=lambda fid: {1: "callback-one"}.get(fid))
    w.sample_gauges(T0)
    w.close()
    assert [x.split("|", 2)[2] for x in _lines(tmp_path)] == [
        _gauge("callback-one", 1, "2.000000") + "|1,0", _gauge("engine-two", 2, "2.000000") + "|1,0",
        _gauge("b-three", 3, "2.000000") + "|1,0", _gauge("4", 4, "2.000000") + "|1,0"]


def test_two_samples_in_one_second_add_and_seconds_stay_apart(tmp_path):
    e = GaugeEngine([(5, 8.0, 4)], size=3, flow_resources={5: "r"})
    w = _writer(tmp_path, [e])
    w.sample_gauges(T0 + 1)
    e.g, e.size = [(5, 8.0, 6)], 2
    w.sample_gauges(T0 + 999)
    w.sample_gauges(T0 + 1000)
    assert w.poll(T0 + 1000) == 2
    assert w.close() == 2
    g = _gauge("r", 5, "8.000000")
    assert _lines(tmp_path) == [f"{STAMP}|1|{g}|10,0", f"{STAMP}|1|flow|totalTokenSize|5,0",
                                f"{STAMP1}|1|{g}|6,0", f"{STAMP1}|1|flow|totalTokenSize|2,0"]


def test_total_token_size_sums_engines_and_is_left_out_at_zero(tmp_path):
    a, b = GaugeEngine([(1, 1.0, 1)], size=4, flow_resources={1: "x"}), GaugeEngine([], size=7)
    w = _writer(tmp_path, [a, b])
    assert w.sample_gauges(T0) == 2
    a.size = b.size = 0
    assert w.sample_gauges(T0 + 1000) == 1
    w.close()
    g = _gauge("x", 1, "1.000000")
    assert _lines(tmp_path) == [f"{STAMP}|1|{g}|1,0", f"{STAMP}|1|flow|totalTokenSize|11,0", f"{STAMP1}|1|{g}|1,0"]


def test_gauges_follow_their_seconds_rows_and_a_second_without_rows_is_written(tmp_path):
    e = GaugeEngine([(9, 3.0, 2)], size=1, tuples=[(T0, 9, CONC_PASS, 0, 2, 1), (T0, 12, CONC_BLOCK, 0, 1, 1),
                                                   (T0 + 2000, 9, CONC_RELEASE, 0, 2, 1)], flow_resources={9: "nine"})
    w = _writer(tmp_path, [e])
    w.sample_gauges(T0 + 500)
    w.sample_gauges(T0 + 1500)  # a second with gauges and no rows
    assert w.poll(T0 + 3000) == 7
    assert w.close() == 0
    g = _gauge("nine", 9, "3.000000")
    assert _lines(tmp_path) == [
        f"{STAMP}|1|concurrent|pass|9|2,0", f"{STAMP}|1|concurrent|block|12|1,0", f"{STAMP}|1|{g}|2,0",
        f"{STAMP}|1|flow|totalTokenSize|1,0", f"{STAMP1}|1|{g}|2,0", f"{STAMP1}|1|flow|totalTokenSize|1,0",
        "2023-11-14 22:13:22|1|concurrent|release|9|2,0"]


def test_engine_without_gauges_is_skipped(tmp_path):
    w = _writer(tmp_path, [PlainEngine(), GaugeEngine([(2, 1.0, 1)], size=1)])
    assert w.sample_gauges(T0) == 2
    assert w.close() == 2
    w = _writer(tmp_path / "plain", [PlainEngine()])
    assert w.sample_gauges(T0) == 0 and w.close() == 0


def test_load_rules_records_resources_and_arrays_do_not(monkeypatch):
    """ClusterFlowRuleManager.load_rules keeps rule.resource per flowId on the engine object (non-cluster rules are
    skipped as the loader skips them); load_rule_arrays has no names.  The native loader is replaced: no GPU."""
    from sentinel_amd import cluster

    class Lib:
        def sga_load_cluster_flow_rules(self, handle, ns, arr, n):
            return n

    class Eng:
        handle = None
        flow_resources = {}

    monkeypatch.setattr(cluster._lib, "load", lambda: Lib())
    eng = Eng()
    mgr = cluster.ClusterFlowRuleManager(eng)
    rule = lambda res, fid, mode=True: cluster.FlowRule(  # noqa: E731
        resource=res, count=1.0, cluster_mode=mode, cluster_config=cluster.ClusterFlowConfig(flow_id=fid))
    assert mgr.load_rules("ns", [rule("alpha", 5), rule("beta", 6), rule("local", 7, mode=False)]) == 2
    assert eng.flow_resources == {5: "alpha", 6: "beta"}
    assert mgr.load_rule_arrays("ns", np.array([8, 9]), np.array([1.0, 1.0])) == 2
    assert eng.flow_resources == {5: "alpha", 6: "beta"}
    assert "second 0" in cluster.DefaultTokenService.release_concurrent_token.__doc__


# ------------------------------------------------------------------ layout
def test_gauge_layout_matches_the_c_compiler(tmp_path):
    """sizeof / offsetof of sga_concurrent_gauge as gcc lays it out == the ctypes mirror == the numpy dtype, and the
    three new SGA_SLOG_* values."""
    from sentinel_amd import _lib
    from sentinel_amd.cluster import CONC_GAUGE_DTYPE
    cls = _lib.SgaConcurrentGauge
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sentinel_amd.h"', "int main(void) {",
             'printf("%zu\\n", sizeof(sga_concurrent_gauge));']
    lines += [f'printf("%zu\\n", offsetof(sga_concurrent_gauge, {f}));' for f, _ in cls._fields_]
    lines += ['printf("%d %d %d %zu\\n", SGA_SLOG_CONC_PASS, SGA_SLOG_CONC_BLOCK, SGA_SLOG_CONC_RELEASE, '
              'sizeof(sga_server_log_row));', "return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    names = [f for f, _ in cls._fields_]
    assert got[0] == 24 == ctypes.sizeof(cls) == CONC_GAUGE_DTYPE.itemsize
    assert got[1:1 + len(names)] == [getattr(cls, f).offset for f in names]
    assert got[1:1 + len(names)] == [CONC_GAUGE_DTYPE.fields[f][1] for f in names]
    assert tuple(CONC_GAUGE_DTYPE.names) == tuple(names)
    assert got[1 + len(names):] == [CONC_PASS, CONC_BLOCK, CONC_RELEASE, 40]
    assert "sga_concurrent_gauges" in _lib.SIGNATURES


# ------------------------------------------------------------------ the reduce helper
def test_reduce_conc_hand_worked():
    """A pass of 2, a block of 3, a release whose call carries acquire 7 of a token acquired with 2 (count 2), a
    second release of it, a BAD_REQUEST, a NO_RULE_EXISTS (acquire and release), and a release one second after its
    acquire: it counts in the release's second."""
    op = [0, 0, 1, 1, 0, 0, 1, 1]
    ids = [11, 11, 900, 900, 0, 77, 901, 902]
    acq = [2, 3, 7, 7, 1, 1, 0, 5]
    ts = [T0 + 5, T0 + 6, T0 + 7, T0 + 8, T0 + 9, T0 + 10, T0 + 11, T0 + 1001]
    status = [cc.OK, cc.BLOCKED, cc.RELEASE_OK, cc.ALREADY_RELEASE, cc.BAD_REQUEST, cc.NO_RULE_EXISTS,
              cc.NO_RULE_EXISTS, cc.RELEASE_OK]
    info = {900: (11, 2), 901: (55, 1), 902: (12, 4)}
    acc = cc.reduce_conc({}, op, ids, acq, ts, status, info)
    assert expected_tuples(acc) == [(T0, 11, CONC_PASS, 0, 2, 1), (T0, 11, CONC_BLOCK, 0, 3, 1),
                                    (T0, 11, CONC_RELEASE, 0, 2, 1), (T0 + 1000, 12, CONC_RELEASE, 0, 4, 1)]
    cc.reduce_conc(acc, [0, 0], [11, 11], [1, 3], [T0 + 20, T0 + 21], [cc.OK, cc.OK], {})
    assert acc[(T0, 11, CONC_PASS, 0)] == [6, 3]
