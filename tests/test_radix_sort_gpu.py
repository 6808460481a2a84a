"""radix_sort.hip tested directly: every sort entry point and the scan against numpy's stable sort,
exact equality, with guard zones behind every scratch and output buffer (sentinel_amd/csrc/sort_hooks.hip).

The sort reads SGA_RADIX_MODE / SGA_RADIX_BITS once per process, so each configuration is a fresh child
running tests/sort_cases.py.  A child that dies by a signal or at its time limit fails its test and makes
the remaining configurations skip: nothing more is started on a device that may have faulted."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sentinel_amd", "libsga_sorttest.so")
CHILD_TIMEOUT_S = 120  # a cap, not a measurement: HIP start-up plus a few hundred small sorts take seconds

pytestmark = pytest.mark.gpu

# (id, environment, which cases)
CONFIGS = [
    ("default", {}, "full"),
    ("mode2", {"SGA_RADIX_MODE": "2"}, "std"),
    ("bits9", {"SGA_RADIX_BITS": "9"}, "std"),
    ("bits10", {"SGA_RADIX_BITS": "10"}, "std"),
    ("bits11", {"SGA_RADIX_BITS": "11"}, "std"),
    # look-back: the contiguous u64 sort only (the pairs sort's look-back wait has no bound)
    ("mode0", {"SGA_RADIX_MODE": "0"}, "u64"),
    ("mode0_bits11", {"SGA_RADIX_MODE": "0", "SGA_RADIX_BITS": "11"}, "u64"),
]

_device_suspect = []  # set once a child died by a signal or at its time limit


@pytest.fixture(scope="module")
def sorttest_lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    return LIB


def run_child(env_extra, which):
    env = {k: v for k, v in os.environ.items() if k not in ("SGA_RADIX_MODE", "SGA_RADIX_BITS")}
    env.update(env_extra)
    return subprocess.run([sys.executable, "-m", "tests.sort_cases", which], cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=CHILD_TIMEOUT_S)


@pytest.mark.parametrize("name,env_extra,which", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_sort_and_scan_match_stable_host_sort(sorttest_lib, name, env_extra, which):
    if _device_suspect:
        pytest.skip("an earlier configuration's child died (%s): not starting more GPU work" % _device_suspect[0])
    try:
        r = run_child(env_extra, which)
    except subprocess.TimeoutExpired:
        _device_suspect.append("%s: time limit" % name)
        pytest.fail("child exceeded %d s" % CHILD_TIMEOUT_S)
    if r.returncode < 0:
        _device_suspect.append("%s: signal %d" % (name, -r.returncode))
        pytest.fail("child died by signal %d\n%s" % (-r.returncode, r.stderr[-2000:]))
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    if r.returncode == 3:  # the runner stopped at a HIP error
        _device_suspect.append("%s: HIP error" % name)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, "\n".join(r.stdout.splitlines()[-5:]),
                                                  r.stderr[-2000:])
    announce = [x for x in rows if "announce" in x]
    summary = [x for x in rows if x.get("summary")]
    cases = [x for x in rows if "case" in x]
    assert len(announce) == 1 and len(summary) == 1
    assert announce[0]["announce"] > 0
    # a runner that stopped early cannot pass
    assert summary[0]["cases"] == announce[0]["announce"] == len(cases)
    assert not summary[0]["aborted"]
    wrong = [(x["case"], x["msg"]) for x in cases if not x["ok"]]
    assert not wrong, "%d of %d cases differ from the stable host sort: %s" % (len(wrong), len(cases), wrong[:10])
    guards = [(x["case"], x["guard"]) for x in cases if x["guard"]]
    assert not guards, "guard zones overwritten (case, buffer bit mask): %s" % guards[:10]
    assert summary[0]["failed"] == 0 and summary[0]["guards"] == 0
    kinds = {x["case"].split()[0] for x in cases}
    assert kinds == ({"u64"} if which == "u64" else {"pairs", "u64", "tiled", "scan"})
