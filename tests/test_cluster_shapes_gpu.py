"""GPU parity of the cluster batch at its size seams: the cases of tests/cluster_shapes.py on the HIP engine against
the oracle replaying the same steps from the start (ClusterFlowChecker.java:55-112 in arrival order), bit for bit
-- every TokenResult (status, remaining, wait) of every request of every batch, all seven metric sums of every
targeted rule and three fillers after every step (of every touched rule at the end, where a case targets none),
the metric node of every rule, and the batch_info words a case names.

tests/cluster_shapes.py has the builders and the groups, tests/test_cluster_shapes_host.py proves their shapes.

test_dispatch_forms runs each group once more in a child process under the test-only build
(SGA_LIB_VARIANT=testhooks), where sga_test_cluster_dispatch reads back how the last batch's cold stage and hot
runs were dispatched: the counts must equal what cluster_shapes.predict_forms derives from the case's arrays and
the oracle's answers, and the form each group exists for must have occurred."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cluster_shapes as cs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO_WORDS = ("hot_mode", "flags", "n_sort", "n_cold", "n_prio", "n_hot_next", "bd_lo", "bd_hi", "hot_err")


def run_case(name, hook=None):
    """Every step of the case on a fresh engine against the shared oracle replay; returns the dispatch counts per
    step when hook is given."""
    import torch
    from sentinel_amd import EngineError, cluster
    from sentinel_amd.metrics import cluster_metric_snapshot
    c = cs.case(name)
    rep = cs.replay(name)
    eng = cluster.Engine(max_batch=c.max_batch, max_rules=1 << 16, **c.engine_args)
    forms = []
    try:
        cluster.ClusterFlowRuleManager(eng).load_rule_arrays("default", c.flow_id, c.count, threshold_type=1,
                                                             sample_count=c.sample, window_interval_ms=c.interval)
        svc = cluster.DefaultTokenService(eng)
        for si, s in enumerate(c.steps):
            ctx = f"{name} step {si}"
            if s["kind"] == "hot":
                eng.set_hot_rules(s["on"], c.engine_args.get("hot_min_requests", 64))
                forms.append(None)
                continue
            exp = rep["results"][si]
            n = len(s["fid"])
            try:
                if s["kind"] == "rls":
                    dev = torch.device("cuda", 0)
                    base = int(s["ts"].min())
                    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
                    _, st, rem = cluster.EnvoyRlsService(eng).should_rate_limit_device(
                        T(np.arange(n + 1, dtype=np.int32)), T(s["fid"]), T(np.ones(n, np.int32)), base,
                        T((s["ts"] - base).astype(np.uint32).view(np.int32)))
                    torch.cuda.synchronize()
                    got = (st.cpu().numpy().astype(np.int32), rem.cpu().numpy().astype(np.int32), np.zeros(n, np.int32))
                else:
                    g = svc.request_tokens(s["fid"], s["acq"], s["prio"], s["ts"])
                    got = (g["status"].astype(np.int32), g["remaining"].astype(np.int32), g["wait_in_ms"].astype(np.int32))
            except (EngineError, RuntimeError) as e:  # a device error: nothing more is started on that GPU by this run
                pytest.exit(f"{ctx}: the engine call failed: {e}", returncode=3)
            bad = np.nonzero((got[0] != exp[0]) | (got[1] != exp[1]) | (got[2] != exp[2]))[0]
            if len(bad):
                i = int(bad[0])
                rule = int(s["fid"][i])
                pos = int((s["fid"][:i] == rule).sum())
                raise AssertionError(
                    f"{ctx}: {len(bad)} of {n} requests differ; first at {i}: rule {rule} ({c.seam_of(rule)}), its request "
                    f"{pos} of {int((s['fid'] == rule).sum())}, t={s['ts'][i]} gpu=({got[0][i]},{got[1][i]},{got[2][i]}) "
                    f"oracle=({exp[0][i]},{exp[1][i]},{exp[2][i]}); rules that differ: "
                    f"{[(int(f), c.seam_of(int(f))) for f in np.unique(s['fid'][bad])[:8]]}")
            if s["kind"] == "token":
                info = eng.batch_info()
                want = s["info"]
                for k in INFO_WORDS:
                    if k in want:
                        assert info[k] == want[k], (ctx, k, info)
                if "bd_span" in want:
                    assert info["bd_hi"] - info["bd_lo"] == want["bd_span"], (ctx, info)
                if "flag_set" in want:
                    assert info["flags"] & want["flag_set"], (ctx, info)
            if hook is not None:
                got_f = hook()
                want_f = cs.predict_forms(c, si, exp)
                assert all(got_f[k] == v for k, v in want_f.items()), \
                    (ctx, {k: (got_f[k], v) for k, v in want_f.items() if got_f[k] != v})
                forms.append(got_f)
            # all seven sums of the watched rules right after the step, while its buckets are in the window
            t, want_s = rep["step_sums"][si]
            for f, o in want_s.items():
                g = svc.metric_sums(f, t)
                assert g == o, (ctx, f, c.seam_of(f), g, o)
        now = rep["now"]
        for f, o in rep["sums"].items():  # (a case without targeted rules: every rule its steps touched)
            g = svc.metric_sums(f, now)
            assert g == o, (name, f, g, o)
        torch.cuda.set_device(0)
        nodes = cluster_metric_snapshot(eng, now)
        assert len(nodes) == c.n_rules, name
        order = np.argsort(nodes["flow_id"])
        assert np.array_equal(nodes["flow_id"][order], c.flow_id), name
        isec = c.interval / 1000.0
        # getAvg(BLOCK) then getAvg(PASS) at now (ClusterMetricNodeGenerator.java:75-91)
        for col, k in (("block_qps", 0), ("pass_qps", 1)):
            bad = np.nonzero(nodes[col][order] != rep["node"][:, k] / isec)[0]
            assert not len(bad), (name, col, [(int(b) + 1, c.seam_of(int(b) + 1)) for b in bad[:8]])
        assert (nodes["timestamp"] == now).all(), name
    finally:
        eng.close()
    return forms


@pytest.mark.parametrize("name", list(cs.BUILDERS))
def test_parity(name):
    run_case(name)


def child(group):
    """Runs in the child process of test_dispatch_forms (the test-only build is loaded)."""
    import ctypes as C

    import torch
    from sentinel_amd import _lib
    assert torch.cuda.device_count() > 0  # torch's HIP runtime first, as under pytest: the engine library shares it
    L = _lib.load()
    fn = L.sga_test_cluster_dispatch  # the product library does not have it
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(C.c_uint32), C.c_size_t]
    nk = len(cs.FORM_KEYS)

    def hook():
        out = (C.c_uint32 * nk)()
        assert fn(out, nk) == nk
        return cs.derived_forms(dict(zip(cs.FORM_KEYS, [int(x) for x in out])))

    print("FORMS", json.dumps({name: run_case(name, hook) for name in cs.GROUPS[group]}))


@pytest.mark.parametrize("group", list(cs.GROUPS))
def test_dispatch_forms(group):
    """Which form decided what: after every batch the counts of the test-only build equal the prediction from the
    case's arrays (compared in the child, with the parity), and the form the group exists for did occur.  The
    product library must not export the read-back."""
    import ctypes as C

    from sentinel_amd import _lib
    assert not hasattr(C.CDLL(_lib.LIB_PATH), "sga_test_cluster_dispatch")
    assert "sga_test_cluster_dispatch" not in _lib.SIGNATURES
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_cluster_shapes_gpu import child; child({group!r})"
    env = dict(os.environ, SGA_LIB_VARIANT="testhooks")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    if r.returncode == 3:  # the child met a device error: nothing more is started on that GPU by this session
        pytest.exit(f"dispatch forms of group {group}: {r.stderr[-2000:]}", returncode=3)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = [x for x in r.stdout.splitlines() if x.startswith("FORMS ")][-1]
    forms = json.loads(line[6:])
    print(group, line[:4000])

    def tot(name, key):
        return sum(f[key] for f in forms[name] if f)

    if group == "R":
        for m in cs.MODES:
            # the runs of 2048 and 2049 without a wait: the whole workgroup; those with waits (cw > 0): one wave
            assert tot(f"R_{m}", "wg") == 2 and tot(f"R_{m}", "direct") > 0 and tot(f"R_{m}", "psearch") > 0, m
            assert tot(f"R_{m}", "bin" if m == "bin" else "chunk") == len(forms[f"R_{m}"]), m
            assert tot(f"R_{m}", "chunk" if m == "bin" else "bin") == 0, m
        assert tot("R_bin", "bin_global") > 0 and tot("R_sort", "global_rec") > 0
    if group == "L":
        assert tot("L_bin", "listfull") >= 1 and tot("L_bin", "wave+wg") == 3 * cs.K_LONG - 1
    if group == "C":
        for n in (4095, 4096):
            f = forms[f"C_small{n}"][0]
            assert (f["cont"], f["gallop"]) == (1, 1) and f["wg"] == 1, n
        for name in [n for n in forms if "small" not in n]:
            f = forms[name][0]
            assert f["cont"] > 8 and f["gallop"] >= 5 and f["global_rec"] >= 3 and f["counter"] >= 1 + 2048 - 256, name
    if group == "B":
        f = forms["B_bins"][1]
        assert f["bin_lds"] > 10 and f["bin_global"] >= 5 and f["wg"] >= 2 and f["global_rec"] > 0
        assert forms["B_big"][0]["bin_global"] == 1 and forms["B_big"][0]["wg"] == 32
    if group == "E":
        assert forms["E_sort"][0]["replay"] == 3 and forms["E_sort"][1]["replay"] > 5 and forms["E_small"][1]["replay"] > 5 and forms["E_hotmix"][1]["replay"] >= 12
        assert forms["E_hotmix"][1]["hot_runs"] > 0
    if group == "S":
        assert all(f["chunk"] == 1 and f["bin"] == 0 for fs in forms.values() for f in fs)
    if group == "P":
        assert all(f["bin"] == 1 and f["chunk"] == 0 for f in forms["P_part"])
        assert all(f["chunk"] == 1 for f in forms["P_256"]) and tot("P_part", "hot_runs") > 0
    if group == "H":
        assert forms["H_span64"][1]["hot_runs"] > 0 and forms["H_span65"][1]["hot_runs"] == 0
        assert forms["H_seg"][1]["hot_cw"] == 4
        assert forms["H_drop"][0]["dropped"] == 1 and forms["H_pick"][2]["hot_runs"] == cs.K_HOT
        assert forms["H_pick"][3]["hot_runs"] == 0 and forms["H_prio"][2]["hot_cw"] == 4
    if group == "M":
        f = forms["M_mixed"]
        assert (f[0]["bin"], f[0]["chunk"]) == (1, 0) and (f[1]["bin"], f[1]["chunk"]) == (0, 1)
        assert (f[3]["bin"], f[3]["chunk"]) == (0, 1) and (f[5]["bin"], f[6]["bin"]) == (1, 1)
