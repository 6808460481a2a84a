"""Metric extensions without a GPU: the two row layouts, the registry, and the dispatcher over a stub sentinel with
hand-made rows -- the exact call sequence, and the reference's own vectors (MetricEntryCallbackTest,
MetricExitCallbackTest) through both extension kinds."""
import ctypes
import os
import subprocess

import pytest

from tests import metric_ext_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ layouts and bindings
@pytest.mark.parametrize("name,cls_name,dtype_name,size", [
    ("sga_metric_res_row", "SgaMetricResRow", "METRIC_RES_ROW_DTYPE", 72),
    ("sga_metric_block_row", "SgaMetricBlockRow", "METRIC_BLOCK_ROW_DTYPE", 32)])
def test_row_layout_matches_the_c_compiler(tmp_path, name, cls_name, dtype_name, size):
    """sizeof / offsetof as gcc lays the struct out == the ctypes mirror == the numpy dtype."""
    from sentinel_amd import _lib, metric_extension
    cls, dtype = getattr(_lib, cls_name), getattr(metric_extension, dtype_name)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sentinel_amd.h"', "int main(void) {",
             f'printf("%zu\\n", sizeof({name}));']
    expect = [ctypes.sizeof(cls)]
    for f, _ in cls._fields_:
        lines.append(f'printf("%zu\\n", offsetof({name}, {f.rstrip("_")}));')  # pass_: `pass` is a Python keyword
        expect.append(getattr(cls, f).offset)
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == expect
    assert got[0] == size and got[0] % 8 == 0
    assert dtype.itemsize == got[0]
    assert [f.rstrip("_") for f, _ in cls._fields_] == list(dtype.names)
    assert [dtype.fields[f][1] for f in dtype.names] == got[1:]


def test_the_two_calls_are_declared_and_bound():
    from sentinel_amd import _lib
    header = open(os.path.join(ROOT, "include", "sentinel_amd.h")).read()
    for sym, nargs in (("sga_metric_ext_enable", 2), ("sga_metric_ext_drain", 9)):
        assert f"int {sym}(" in header
        assert _lib.SIGNATURES[sym][0] is ctypes.c_int and len(_lib.SIGNATURES[sym][1]) == nargs
    assert "#define SGA_ABI_VERSION 3" in header


# ------------------------------------------------------------------ the dispatcher
def _basic():
    from sentinel_amd.metric_extension import MetricExtension

    class Basic(mc.Recorder, MetricExtension):
        def add_pass(self, *a, **k): self._rec("add_pass", *a, **k)
        def add_block(self, *a, **k): self._rec("add_block", *a, **k)
        def add_success(self, *a, **k): self._rec("add_success", *a, **k)
        def add_exception(self, *a, **k): self._rec("add_exception", *a, **k)
        def add_rt(self, *a, **k): self._rec("add_rt", *a, **k)
        def increase_thread_num(self, *a, **k): self._rec("increase_thread_num", *a, **k)
        def decrease_thread_num(self, *a, **k): self._rec("decrease_thread_num", *a, **k)
    return Basic()


def _advanced():
    from sentinel_amd.metric_extension import AdvancedMetricExtension

    class Advanced(mc.Recorder, AdvancedMetricExtension):
        def on_pass(self, *a, **k): self._rec("on_pass", *a, **k)
        def on_blocked(self, *a, **k): self._rec("on_blocked", *a, **k)
        def on_complete(self, *a, **k): self._rec("on_complete", *a, **k)
        def on_error(self, *a, **k): self._rec("on_error", *a, **k)
        # an advanced extension must never get these
        def add_pass(self, *a, **k): raise AssertionError("add_pass on an advanced extension")
        def add_block(self, *a, **k): raise AssertionError("add_block on an advanced extension")
        def add_rt(self, *a, **k): raise AssertionError("add_rt on an advanced extension")
        def add_success(self, *a, **k): raise AssertionError("add_success on an advanced extension")
        def add_exception(self, *a, **k): raise AssertionError("add_exception on an advanced extension")
        def increase_thread_num(self, *a, **k): raise AssertionError("thread call on an advanced extension")
        def decrease_thread_num(self, *a, **k): raise AssertionError("thread call on an advanced extension")
    return Advanced()


def _names(calls):
    return [c[0] for c in calls]


def test_the_exact_call_sequence():
    """Two resources, two extensions: resource order outside, registration order inside, and inside an extension the
    pass callback, the block rows in their order, then the exit callback with the exception last."""
    from sentinel_amd.local import BlockException, DegradeException, FlowException
    from sentinel_amd.metric_extension import dispatch
    from sentinel_amd.rules import DegradeRule, FlowRule
    flow = FlowRule(resource="b", count=0, limit_app="o2")
    deg = DegradeRule(resource="b", count=0, time_window=1)
    s = mc.StubSentinel(["a", "b"], ["o1", "o2"], {(1, 1, 0): flow, (3, 1, 2): deg})
    res = mc.make_res_rows([(0, 5, 3, 0, 0, 0, 0, 0, 0),            # a: passes only
                            (1, 7, 2, 9, 4, 3, 1, 7100, 7000)])     # b: passes, exits, one error
    blk = mc.make_block_rows([(1, 0, 0, 0, 1, 1),                   # b: a kind 2 event, no origin
                              (1, 2, 1, 0, 4, 2),                   # b: FlowException from o2
                              (1, 2, 3, 2, 1, 1)])                  # b: DegradeException from o2
    basic, adv = _basic(), _advanced()
    n = dispatch(s, [basic, adv], res, blk)
    assert _names(basic.calls) == ["increase_thread_num", "add_pass",                         # a
                                   "increase_thread_num", "add_pass", "add_block", "add_block", "add_block",
                                   "add_rt", "add_success", "decrease_thread_num", "add_exception"]
    assert _names(adv.calls) == ["on_pass", "on_pass", "on_blocked", "on_blocked", "on_blocked", "on_complete",
                                 "on_error"]
    assert n == len(basic.calls) + len(adv.calls)
    c = basic.calls
    assert c[0] == ("increase_thread_num", ("a",), (("times", 3),))
    assert c[1] == ("add_pass", ("a", 5), (("events", 3),))
    assert c[2] == ("increase_thread_num", ("b",), (("times", 2),))
    assert c[3] == ("add_pass", ("b", 7), (("events", 2),))
    assert c[7] == ("add_rt", ("b", 7100), (("events", 4), ("rt_max", 7000)))
    assert c[8] == ("add_success", ("b", 9), (("events", 4),))
    assert c[9] == ("decrease_thread_num", ("b",), (("times", 4),))
    assert c[10] == ("add_exception", ("b", 3, None), (("events", 1),))
    (_, (r0, n0, o0, e0), k0), (_, (r1, n1, o1, e1), k1), (_, (r2, n2, o2, e2), k2) = c[4:7]
    assert (r0, n0, o0, k0) == ("b", 1, "", (("events", 1),)) and type(e0) is BlockException and e0.rule is None
    assert (r1, n1, o1, k1) == ("b", 4, "o2", (("events", 2),)) and type(e1) is FlowException
    assert e1.rule is flow and e1.rule_limit_app == "o2" and e1.resource == "b"
    assert (r2, n2, o2, k2) == ("b", 1, "o2", (("events", 1),)) and type(e2) is DegradeException and e2.rule is deg
    a = adv.calls
    assert a[0] == ("on_pass", ("a", 5), (("events", 3),))
    assert a[3][1][:3] == ("b", 4, "o2") and a[3][1][3].rule is flow
    assert a[5] == ("on_complete", ("b", 7100, 9), (("events", 4), ("rt_max", 7000)))
    assert a[6] == ("on_error", ("b", None, 3), (("events", 1),))
    # the interleaving across extensions: all of a, then all of b
    order = []
    basic.calls.clear(), adv.calls.clear()
    basic._rec = lambda name, *a, **k: order.append(("basic", a[0]))
    adv._rec = lambda name, *a, **k: order.append(("adv", a[0]))
    dispatch(s, [basic, adv], res, blk)
    assert [k for k, _ in order] == ["basic"] * 2 + ["adv"] + ["basic"] * 9 + ["adv"] * 6
    assert [r for _, r in order] == ["a"] * 3 + ["b"] * 15


def _fakes():
    """The reference's FakeMetricExtension / FakeAdvancedMetricExtension as sums over merged calls."""
    from sentinel_amd.metric_extension import AdvancedMetricExtension, MetricExtension

    class Fake(MetricExtension):
        def __init__(self): self.pass_ = self.block = self.success = self.exception = self.rt = self.thread = 0
        def add_pass(self, resource, n, events=1): self.pass_ += n
        def add_block(self, resource, n, origin, block_exception, events=1): self.block += n
        def add_success(self, resource, n, events=1): self.success += n
        def add_exception(self, resource, n, throwable=None, events=1): self.exception += n
        def add_rt(self, resource, rt_sum, events=1, rt_max=0): self.rt += rt_sum
        def increase_thread_num(self, resource, times=1): self.thread += times
        def decrease_thread_num(self, resource, times=1): self.thread -= times

    class FakeAdvanced(AdvancedMetricExtension):
        def __init__(self): self.pass_ = self.block = self.complete = self.exception = self.rt = self.concurrency = 0

        def on_pass(self, resource, batch_count, events=1):
            self.pass_ += batch_count
            self.concurrency += events

        def on_blocked(self, resource, batch_count, origin, block_exception, events=1): self.block += batch_count

        def on_complete(self, resource, rt_sum, batch_count, events=1, rt_max=0):
            self.complete += batch_count
            self.rt += rt_sum
            self.concurrency -= events

        def on_error(self, resource, throwable, batch_count, events=1): self.exception += batch_count
    return Fake(), FakeAdvanced()


def test_the_reference_vectors_of_the_entry_callback():
    """MetricEntryCallbackTest: onPass with count 2 gives pass 2 and thread 1; onBlocked with a FlowException from
    origin1 and count 2 gives block 2 -- for both extension kinds."""
    from sentinel_amd.local import FlowException
    from sentinel_amd.metric_extension import dispatch
    s = mc.StubSentinel(["resource"], ["origin1"])
    fake, adv = _fakes()
    dispatch(s, [fake, adv], mc.make_res_rows([(0, 2, 1, 0, 0, 0, 0, 0, 0)]), mc.make_block_rows([]))
    assert (fake.pass_, fake.thread) == (2, 1)
    assert (adv.pass_, adv.concurrency) == (2, 1)
    seen = []
    fake.add_block = lambda res, n, origin, e, events=1: seen.append((res, n, origin, type(e), events))
    dispatch(s, [fake], mc.make_res_rows([]), mc.make_block_rows([(0, 1, 1, 0, 2, 1)]))
    assert seen == [("resource", 2, "origin1", FlowException, 1)]
    fake, adv = _fakes()
    dispatch(s, [fake, adv], mc.make_res_rows([]), mc.make_block_rows([(0, 1, 1, 0, 2, 1)]))
    assert fake.block == 2 and adv.block == 2
    assert (fake.pass_, fake.thread, adv.pass_, adv.concurrency) == (0, 0, 0, 0)


def test_the_reference_vectors_of_the_exit_callback():
    """MetricExitCallbackTest: from rt 20, success 6, thread 10, one exit of count 2 after 100 ms gives rt 20 + 100,
    success 6 + 2, thread 10 - 1 -- for both extension kinds (complete / concurrency on the advanced one)."""
    from sentinel_amd.metric_extension import dispatch
    s = mc.StubSentinel(["resource"], [])
    fake, adv = _fakes()
    fake.rt, fake.success, fake.thread = 20, 6, 10
    adv.rt, adv.complete, adv.concurrency = 20, 6, 10
    dispatch(s, [fake, adv], mc.make_res_rows([(0, 0, 0, 2, 1, 0, 0, 100, 100)]), mc.make_block_rows([]))
    assert (fake.rt, fake.success, fake.thread, fake.exception) == (20 + 100, 6 + 2, 10 - 1, 0)
    assert (adv.rt, adv.complete, adv.concurrency, adv.exception) == (20 + 100, 6 + 2, 10 - 1, 0)


def test_the_lost_call():
    from sentinel_amd.local import BlockException
    from sentinel_amd.metric_extension import LOST_RESOURCE, dispatch
    assert LOST_RESOURCE == "__lost__"
    s = mc.StubSentinel(["a"], [])
    basic, adv = _basic(), _advanced()
    n = dispatch(s, [basic, adv], mc.make_res_rows([(0, 1, 1, 0, 0, 0, 0, 0, 0)]), mc.make_block_rows([]), 7, 19)
    assert n == 5
    name, (res, cnt, origin, e), kw = basic.calls[-1]
    assert (name, res, cnt, origin, kw) == ("add_block", "__lost__", 19, "", (("events", 7),))
    assert type(e) is BlockException
    name, (res, cnt, origin, e), kw = adv.calls[-1]
    assert (name, res, cnt, origin, kw) == ("on_blocked", "__lost__", 19, "", (("events", 7),))


def test_the_registry():
    from sentinel_amd.metric_extension import MetricExtension, MetricExtensionProvider
    p = MetricExtensionProvider()
    a, b, c = MetricExtension(), MetricExtension(), MetricExtension()
    p.add(a), p.add(b), p.add(c)
    assert p.list() == [a, b, c] and len(p) == 3
    assert p.remove(b) and not p.remove(b)
    assert p.list() == [a, c]
    p.add(b)
    assert list(p) == [a, c, b], "registration order"
    with pytest.raises(ValueError):
        p.add(None)
    p.clear()
    assert p.list() == [] and len(p) == 0


def test_no_call_for_an_empty_drain():
    from sentinel_amd.metric_extension import MetricExtension, dispatch
    s = mc.StubSentinel(["a"], [])
    basic, adv = _basic(), _advanced()
    assert dispatch(s, [basic, adv], mc.make_res_rows([]), mc.make_block_rows([])) == 0
    assert basic.calls == [] and adv.calls == []
    assert dispatch(s, [], mc.make_res_rows([(0, 1, 1, 0, 0, 0, 0, 0, 0)]), mc.make_block_rows([])) == 0
    # the base classes are no-ops: nothing raises
    from sentinel_amd.metric_extension import AdvancedMetricExtension
    assert dispatch(s, [MetricExtension(), AdvancedMetricExtension()],
                    mc.make_res_rows([(0, 1, 1, 2, 1, 2, 1, 5, 5)]), mc.make_block_rows([(0, 0, 0, 0, 1, 1)])) == 11
