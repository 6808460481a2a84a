"""GPU parity of the local path at its dispatch seams: the streams of tests/local_shapes.py on the HIP engine
against lt.Oracle replaying the same chunks, bit for bit -- every decision and wait, every node getter of every
targeted resource (and of ENTRY_NODE in group E), the metrics rows at now + 2000 and every breaker state.

Groups (tests/local_shapes.py has the builders, tests/test_local_shapes_host.py proves their shapes):
  A  lane / wave / heavy: k_lflows, lane_run, k_lwave<0>, k_lwave<1>, k_lwsum, k_lheavy
  B  run segmentation: k_lruns_up, k_lruns_tiles, k_lruns_down, k_lexits
  C  parameter segments: k_pseg_key, k_pseg_heads, k_pseg_solve, k_pseg_long, k_lheavy's parameter cache
  D  breaker flows: k_cb_flows<1>, k_cb_flows<8>, k_cbt_*
  E  ENTRY_NODE tiles: k_entry_stats
  F  host chunking: FlowEngine::submit, k_lsmall
  G  acquire extremes on the closed form, the wave and the heavy path

test_dispatch_forms runs each group once more in a child process under the test-only build
(SGA_LIB_VARIANT=testhooks), where sga_test_local_dispatch reads back how the last chunk was dispatched: the
counts must equal what local_shapes.predict_forms derives from the shape table's arrays.  The engine keeps no
count of the windows k_lwave<1> decided from k_lwsum's summaries, of the form (bucketed or serial) a
k_entry_stats tile took, or of the closed form against the per-event replay inside lane_run: for those the
input shapes asserted in tests/test_local_shapes_host.py are the evidence, and parity here is the check."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import local_shapes as ls
from tests import local_trace as lt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_case(name, hook=None):
    """One engine call per chunk against the oracle; returns the dispatch counts per chunk when hook is given."""
    from sentinel_amd import EngineError
    from tests.test_configs_fullsize_gpu import _local
    c = ls.case(name)
    seam = {}
    for r in c.table:
        seam.setdefault(r["res"], r["seam"])
    orc = c.oracle()
    eng, s = _local(c.n_res, c.flow, c.param, c.degrade,
                    max_batch=c.max_batch or max(len(ch["kind"]) for ch in c.chunks))
    cb_res = sorted({r["resource"] for r in c.degrade})
    forms = []
    try:
        for ci, ch in enumerate(c.chunks):
            before = {r: orc.cb_state(r, 0) for r in cb_res}
            exp_d, exp_w = orc.replay(ch)
            try:
                got_d, got_w = s.submit(ch["kind"], ch["resource"], ch["ts"], ch["acquire"], ch["flags"], ch["rt"],
                                        ch["param"])
            except EngineError as e:  # a device error: nothing more is started on that GPU by this run
                pytest.exit(f"{name} chunk {ci}: the engine call failed: {e}", returncode=3)
            bad = np.nonzero((got_d != exp_d) | (got_w != exp_w))[0]
            if len(bad):
                i = int(bad[0])
                res = int(ch["resource"][i])
                pos = int((ch["resource"][:i] == res).sum())
                raise AssertionError(
                    f"{name} chunk {ci}: {len(bad)} of {len(got_d)} events differ; first at {i}: resource {res} "
                    f"({seam.get(res, 'filler')}), its event {pos} of {int((ch['resource'] == res).sum())}, "
                    f"kind={ch['kind'][i]} ts={ch['ts'][i]} acq={ch['acquire'][i]} flags={ch['flags'][i]} "
                    f"param={ch['param'][i]} gpu=({got_d[i]},{got_w[i]}) oracle=({exp_d[i]},{exp_w[i]}); "
                    f"resources that differ: {sorted(set(ch['resource'][bad].tolist()))[:20]}")
            for r in cb_res:
                for k in range(sum(1 for d in c.degrade if d["resource"] == r)):
                    assert s.circuit_breaker_state(r, k) == orc.cb_state(r, k), (name, ci, r, k, seam.get(r))
            if hook is not None:
                got = hook()
                exp = ls.predict_forms(c, ci, before.get)
                assert got == exp, (name, ci, {k: (got[k], exp[k]) for k in got if got[k] != exp[k]})
                forms.append(got)
        now = max(int(ch["ts"].max()) for ch in c.chunks) + 1
        nodes = c.targets + list(range(c.first_filler, c.first_filler + 3)) + ([ls.ENTRY_NODE] if c.entry_node else [])
        for rid in nodes:
            v = s.node(rid, now)
            got = [getattr(v, g) for g in lt.NODE_GETTERS]
            exp = orc.node(rid, now)
            assert got == exp, (name, rid, seam.get(rid), [x for x in zip(lt.NODE_GETTERS, got, exp) if x[1] != x[2]])
        got = [(m.timestamp, ls.ENTRY_NODE if m.resource == "__total_inbound_traffic__" else s.resource_id(m.resource),
                m.pass_qps, m.block_qps, m.success_qps, m.exception_qps, m.rt, m.occupied_pass_qps)
               for m in s.metrics(now + 2000, cap=1 << 16)]
        exp = orc.metrics(now + 2000, cap=1 << 16)
        if got != exp:
            diff = [(g, e) for g, e in zip(got, exp) if g != e][:3]
            raise AssertionError(f"{name}: metrics rows differ ({len(got)} against {len(exp)}); first: {diff}")
        assert not c.entry_node or any(row[1] == ls.ENTRY_NODE for row in exp)
    finally:
        orc.close()
        eng.close()
    return forms


@pytest.mark.parametrize("name", list(ls.BUILDERS))
def test_parity(name):
    run_case(name)


def child(group):
    """Runs in the child process of test_dispatch_forms (the test-only build is loaded)."""
    import ctypes as C

    from sentinel_amd import _lib
    L = _lib.load()
    fn = L.sga_test_local_dispatch  # the product library does not have it
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_uint32), C.c_size_t]

    def hook():
        out = (C.c_uint32 * 12)()
        assert fn(out, 12) == 12
        return dict(zip(ls.FORM_KEYS, [int(x) for x in out]))

    print("FORMS", json.dumps({name: run_case(name, hook) for name in ls.GROUPS[group]}))


@pytest.mark.parametrize("group", list(ls.GROUPS))
def test_dispatch_forms(group):
    """Which form decided what: the counts of FlowScratch::counters and cbt_ctl after each chunk equal the shape
    table's prediction, and the parity holds in the test-only build too.  The product library must not export the
    read-back."""
    import ctypes as C

    from sentinel_amd import _lib
    assert not hasattr(C.CDLL(_lib.LIB_PATH), "sga_test_local_dispatch")
    assert "sga_test_local_dispatch" not in _lib.SIGNATURES
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_local_shapes_gpu import child; child({group!r})"
    env = dict(os.environ, SGA_LIB_VARIANT="testhooks")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("FORMS ")][-1]
    forms = json.loads(line[6:])
    print(group, line)
    # what each group is there for did happen (the exact counts were compared in the child)
    tot = {k: sum(f[k] for fs in forms.values() for f in fs) for k in ls.FORM_KEYS}
    if group == "A":
        assert forms["A"][1]["wave"] == 2 * 6 + 7 and forms["A"][1]["heavy"] == 5 * 6
    if group == "C":
        assert forms["C"][1]["pseg"] == 4 and forms["C"][1]["long"] == 4 * 4 and forms["C"][1]["heavy"] == 1
    if group == "D":
        assert tot["tiled"] == 3 and tot["cb"] > 20
    if group == "F":
        assert [f["small"] for f in forms["Fsmall"]] == [1, 1] and [f["small"] for f in forms["Fpipe"]] == [0, 0]
        assert [f["chunks"] for f in forms["Fcut"]] == [1, 2] and [f["chunks"] for f in forms["Fspan"]] == [1, 2]
    if group == "G":
        assert forms["G"][0]["wave"] == 4 and forms["G"][0]["heavy"] == 1
