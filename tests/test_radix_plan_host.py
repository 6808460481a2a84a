"""The pass plan and scratch budget of every sort in radix_sort.hip, on the host (no GPU): the words the
kernels index never exceed the words the sizing functions promise.  One child per SGA_RADIX_BITS, because
the knob is read once per process; the child calls only sgat_sort_plan (tests/sort_cases.py plan)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sentinel_amd", "libsga_sorttest.so")

MAX_PASSES = 3
MAX_DIGIT = 11
PAIRS_LOOKBACK_TAIL = 3 * 2048 + 64  # digit totals of three passes + tile counters, kept in hist_scan


@pytest.fixture(scope="module")
def sorttest_lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return LIB


@pytest.mark.parametrize("knob", [None, "8", "9", "10", "11"])
def test_plan_fits_the_scratch_sizing(sorttest_lib, knob):
    env = {k: v for k, v in os.environ.items() if k not in ("SGA_RADIX_MODE", "SGA_RADIX_BITS")}
    if knob is not None:
        env["SGA_RADIX_BITS"] = knob
    width = int(knob) if knob else 8
    r = subprocess.run([sys.executable, "-m", "tests.sort_cases", "plan"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    plans = {tuple(x["plan"]): x["out"] for x in rows if "plan" in x}
    summary = [x for x in rows if x.get("summary")]
    assert len(summary) == 1 and summary[0]["cases"] == len(plans) == 3 * 32 * 4
    assert summary[0]["digit_cap"] == width
    for bits in range(1, 33):
        for n in (1, 4096, 4097, 1 << 20):
            tiles = -(-n // 4096)
            for kind in (0, 1, 2):
                npass, digit, hist_idx, hist_size, part_idx, part_size, gh_idx, gh_size = plans[(kind, bits, n)]
                where = "kind %d bits %d n %d: %s" % (kind, bits, n, plans[(kind, bits, n)])
                assert (npass <= MAX_PASSES) == (bits <= MAX_PASSES * width), where
                assert 1 <= digit <= min(MAX_DIGIT, width), where
                assert npass * digit >= bits and (npass - 1) * digit < bits, where
                if npass > MAX_PASSES:
                    continue  # refused: nothing is launched
                status = (1 << digit) * tiles
                assert hist_idx == status + (PAIRS_LOOKBACK_TAIL if kind == 0 else 0), where
                assert hist_idx <= hist_size, where
                assert part_idx <= part_size, where
                assert gh_idx <= gh_size, where
                assert npass << digit <= 3 * 2048, where
            assert plans[(2, bits, n)] == plans[(1, bits, n)]
