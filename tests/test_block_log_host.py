"""Block log, host side (no GPU): the C ABI additions and their ctypes mirror, and block_log.BlockLogWriter driven
with hand-made rows -- the exact bytes of sentinel-block.log as StatLogController.StatLogWriteTask writes them
(StatLogController.java:126-152) with EagleEyeLogUtil's delimiters, the host merge, the lost line and the rolling
of EagleEyeRollingFileAppender.rollOver."""
import ctypes
import datetime
import os
import re
import subprocess

from tests.block_log_cases import STAMP, T0, StubSentinel, make_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UTC = datetime.timezone.utc
NEW_SYMBOLS = ("sga_block_log_enable", "sga_block_log_drain", "sga_block_rule_index")


def _header():
    text = open(os.path.join(ROOT, "include", "sentinel_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_block_log_api():
    text = _header()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, text), sym
    assert re.search(r"typedef\s+struct\s+sga_block_row\b", text)
    assert "#define SGA_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "sentinel_amd.h")).read()


def test_mirror_binds_the_block_log_api():
    from sentinel_amd import _lib
    L = _lib.load()
    for sym in NEW_SYMBOLS:
        assert sym in _lib.SIGNATURES, sym
        fn = getattr(L, sym)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib.SIGNATURES[sym][1]
    assert len(_lib.SIGNATURES["sga_block_log_drain"][1]) == 7
    assert len(_lib.SIGNATURES["sga_block_rule_index"][1]) == 5


def test_block_row_layout_matches_the_c_compiler(tmp_path):
    """sizeof / offsetof of sga_block_row as gcc lays it out == the ctypes mirror == the numpy dtype."""
    from sentinel_amd import _lib
    from sentinel_amd.block_log import BLOCK_ROW_DTYPE
    cls = _lib.SgaBlockRow
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sentinel_amd.h"', "int main(void) {",
             'printf("%zu\\n", sizeof(sga_block_row));']
    expect = [ctypes.sizeof(cls)]
    for f, _ in cls._fields_:
        lines.append(f'printf("%zu\\n", offsetof(sga_block_row, {f}));')
        expect.append(getattr(cls, f).offset)
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == expect
    assert got[0] == 48 and got[0] % 8 == 0
    assert BLOCK_ROW_DTYPE.itemsize == got[0]
    assert [BLOCK_ROW_DTYPE.fields[f][1] for f, _ in cls._fields_] == got[1:]


# ------------------------------------------------------------------ the writer
class _Rule:
    def __init__(self, limit_app):
        self.limit_app = limit_app


def _stub():
    resources = ["GET:/a", "GET:/b", "sys", "auth", "par"]
    origins = ["appA", "appB"]
    rules = {(1, 0, 0): _Rule("appA"), (1, 0, 1): _Rule("default"), (1, 0, 2): _Rule("default"),
             (3, 1, 0): _Rule("default")}
    return StubSentinel(resources, origins, rules, param_texts={(0xDEAD, 0): "bob"})


def _read(d, name="sentinel-block.log"):
    with open(os.path.join(d, name), "rb") as f:
        return f.read()


def test_one_line_of_each_exception_class(tmp_path):
    from sentinel_amd.block_log import BlockLogWriter
    s = _stub()
    s.pending.append((make_rows([
        (T0, 0, 1, 0, 1, 0, 0, 7, 3),          # FlowException, rule limited to appA, from appA
        (T0, 1, 3, 0, 2, 0, 0, 2, 2),          # DegradeException from appB
        (T0, 2, 5, 0, 0, 0, 0, 4, 4),          # SystemBlockException, limitType qps, no origin
        (T0, 3, 6, 0, 2, 0, 0, 1, 1),          # AuthorityException: limitApp = the origin
        (T0, 4, 2, 0, 0, 0, 0xDEAD, 5, 5),     # ParamFlowException: the recorded text of the tag
    ]), 0, 0))
    w = BlockLogWriter(s, str(tmp_path), tz=UTC)
    assert w.poll(T0 + 1000) == 5
    assert _read(tmp_path) == (
        f"{STAMP}|1|GET:/a,FlowException,appA,appA|7,0\n"
        f"{STAMP}|1|GET:/b,DegradeException,default,appB|2,0\n"
        f"{STAMP}|1|sys,SystemBlockException,qps,|4,0\n"
        f"{STAMP}|1|auth,AuthorityException,appB,appB|1,0\n"
        f"{STAMP}|1|par,ParamFlowException,bob,|5,0\n").encode()
    s.pending.append((make_rows([]), 0, 0))
    assert w.close() == 0


def test_system_limit_types_and_param_text_defaults(tmp_path):
    from sentinel_amd.block_log import BlockLogWriter, default_param_text, java_text
    s = _stub()
    s.pending.append((make_rows(
        [(T0, 2, 5, k, 0, 0, 0, 1, 1) for k in range(5)] +
        [(T0, 4, 2, 0, 0, 0, 42, 1, 1), (T0, 4, 2, 0, 0, 0, (1 << 64) - 2, 1, 1), (T0, 4, 2, 0, 0, 1, 0xAB, 1, 1),
         (T0, 4, 2, 0, 0, 0, 9, 1, 1)]), 0, 0))
    w = BlockLogWriter(s, str(tmp_path), param_text=lambda tag, kind: "nine" if tag == 9 else None, tz=UTC)
    w.poll(T0 + 1000)
    lims = [line.split("|")[2].split(",")[2] for line in _read(tmp_path).decode().splitlines()]
    assert lims == ["qps", "thread", "rt", "load", "cpu", "42", "-2", "#00000000000000ab", "nine"]
    assert default_param_text(5, 0) == "5" and default_param_text((1 << 63), 0) == str(-(1 << 63))
    assert java_text(True) == "true" and java_text(False) == "false" and java_text([1, "a", [2]]) == "[1, a, [2]]"
    assert java_text(17) == "17" and java_text("x,y") == "x,y"


def test_details_that_share_a_limit_app_merge(tmp_path):
    from sentinel_amd.block_log import BlockLogWriter
    s = _stub()
    s.pending.append((make_rows([
        (T0, 0, 1, 1, 1, 0, 0, 4, 2), (T0, 0, 1, 2, 1, 0, 0, 6, 3),        # two default rules: one line of 10
        (T0, 0, 1, 0, 1, 0, 0, 1, 1),                                      # the appA rule: its own line
        (T0 + 1000, 0, 1, 1, 1, 0, 0, 9, 9),                               # another second: its own line
    ]), 0, 0))
    w = BlockLogWriter(s, str(tmp_path), tz=UTC)
    assert w.poll(T0 + 2000) == 3
    assert _read(tmp_path) == (
        f"{STAMP}|1|GET:/a,FlowException,default,appA|10,0\n"
        f"{STAMP}|1|GET:/a,FlowException,appA,appA|1,0\n"
        f"{STAMP[:-2]}21|1|GET:/a,FlowException,default,appA|9,0\n").encode()


def test_empty_origin_leaves_nothing_after_the_last_comma(tmp_path):
    from sentinel_amd.block_log import BlockLogWriter
    s = _stub()
    s.pending.append((make_rows([(T0, 1, 3, 0, 0, 0, 0, 3, 3)]), 0, 0))
    w = BlockLogWriter(s, str(tmp_path), tz=UTC)
    w.poll(T0 + 1000)
    assert _read(tmp_path) == f"{STAMP}|1|GET:/b,DegradeException,default,|3,0\n".encode()


def test_newline_of_the_reference_appender(tmp_path):
    """EagleEyeCoreUtils.NEWLINE is "\\r\\n": the writer takes it for byte parity with a Java-written file."""
    from sentinel_amd.block_log import BlockLogWriter
    s = _stub()
    s.pending.append((make_rows([(T0, 1, 3, 0, 0, 0, 0, 3, 3)]), 0, 0))
    w = BlockLogWriter(s, str(tmp_path), tz=UTC, newline="\r\n")
    w.poll(T0 + 1000)
    assert _read(tmp_path) == f"{STAMP}|1|GET:/b,DegradeException,default,|3,0\r\n".encode()


def test_lost_counters_get_a_line(tmp_path):
    from sentinel_amd.block_log import BlockLogWriter
    s = _stub()
    s.pending.append((make_rows([(T0, 1, 3, 0, 0, 0, 0, 3, 3)]), 12, 30))
    s.pending.append((make_rows([]), 0, 0))
    s.pending.append((make_rows([]), 2, 2))
    w = BlockLogWriter(s, str(tmp_path), tz=UTC)
    assert w.poll(T0 + 1000) == 2
    assert w.poll(T0 + 1000) == 0          # no counters, no line
    assert w.poll(T0 + 2000) == 1          # counters alone still get theirs, at the second just finished
    assert _read(tmp_path) == (
        f"{STAMP}|1|GET:/b,DegradeException,default,|3,0\n"
        f"{STAMP}|1|__lost__,BlockException,events=12,|30,0\n"
        f"{STAMP[:-2]}21|1|__lost__,BlockException,events=2,|2,0\n").encode()


def test_rolling_keeps_max_backup_index_files(tmp_path):
    """EagleEyeRollingFileAppender.rollOver: .1 is the newest backup, .3 the oldest kept, no .4 ever."""
    from sentinel_amd.block_log import BlockLogWriter
    s = _stub()
    w = BlockLogWriter(s, str(tmp_path), tz=UTC, max_file_size=300, max_backup_index=3)
    per_poll = 4
    polls = 12
    for k in range(polls):  # every poll appends 4 lines (~215 bytes): a roll every second poll
        s.pending.append((make_rows([(T0 + 1000 * k, j, 5, 0, 0, 0, 0, 1, 1) for j in range(per_poll)]), 0, 0))
        assert w.poll(T0 + 1000 * (k + 1)) == per_poll
    names = sorted(os.listdir(tmp_path))
    assert names == ["sentinel-block.log", "sentinel-block.log.1", "sentinel-block.log.2", "sentinel-block.log.3"]
    # the files hold the newest lines in order, oldest file first, and the oldest lines are gone
    kept = b"".join(_read(tmp_path, n) for n in ["sentinel-block.log.3", "sentinel-block.log.2",
                                                 "sentinel-block.log.1", "sentinel-block.log"])
    assert 0 < len(kept.splitlines()) < polls * per_poll
    assert kept.decode().splitlines()[-1].startswith(f"{STAMP[:-2]}31|1|")   # T0 + 11 s
    for n in names[1:]:
        assert os.path.getsize(os.path.join(tmp_path, n)) >= 300
    s.pending.append((make_rows([]), 0, 0))
    w.close()
