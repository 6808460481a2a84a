"""The cluster batch's key pass (k_hot_key_dense / k_hot_key_hash) at its seams: the cases
of tests/keypass_cases.py -- hot bucket boundaries on the round, chunk, sub and segment edges, two boundaries in
one round, a first round over two buckets, backward steps, more than 64 buckets, rare lanes alone in a round of
hot requests, time offsets crossing 2^32, short tails, the fallback pass followed by the hot path, sparse
flowIds -- through the four-array and the packed device entries.  Every TokenResult of every batch and all seven
metric sums of every rule against the oracle replaying the same batches from the start
(ClusterFlowChecker.java:55-112 in arrival order), and the batch's path words (sga_cluster_batch_info) against
keypass_cases.predict.  tests/test_cluster_keypass_host.py proves the cases."""
import numpy as np
import pytest

from tests import keypass_cases as kc

pytestmark = pytest.mark.gpu

WORDS = ("hot_mode", "flags", "bd_lo", "bd_hi", "n_cold")


def submit(L, eng, dev, b, sparse, packed):
    import torch
    fid = kc.fmap(b.lid, sparse)
    off = (b.ts - b.base).astype(np.uint32)
    o = torch.zeros(b.n, dtype=torch.int64, device=dev)
    if packed:  # 12-byte records: flowId, time offset, acquireCount | flags << 16 (bit 0 prioritized)
        rec = np.zeros((b.n, 3), dtype=np.uint32)
        rec[:, 0] = fid.astype(np.uint32)
        rec[:, 1] = off
        rec[:, 2] = b.acq.astype(np.uint32) | (b.prio.astype(np.uint32) << 16)
        for k, i in enumerate(b.resv):  # a valid acquire count under a reserved flag bit
            rec[i, 2] = 1 | (2 << (k % 15)) << 16
        d = torch.from_numpy(rec.view(np.int32)).to(dev)
        rc = L.sga_request_tokens_packed_device(eng.handle, d.data_ptr(), b.base, b.n, o.data_ptr(), None)
    else:
        d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (fid, b.acq, b.prio, off.view(np.int32))]
        rc = L.sga_request_tokens_device(eng.handle, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), b.base,
                                         d[3].data_ptr(), b.n, o.data_ptr(), None)
    if rc != 0 or L.sga_sync(eng.handle) != 0:  # a device error: nothing more is started on that GPU by this run
        pytest.exit(f"the engine call failed: {L.sga_last_error(eng.handle)}", returncode=3)
    r = o.cpu().numpy().view(np.uint64)
    return (((r >> np.uint64(48)) & np.uint64(0xFF)).astype(np.int8).astype(np.int32),
            (r & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32),
            ((r >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.uint16).view(np.int16).astype(np.int32))


@pytest.mark.parametrize("packed", [False, True], ids=["arrays", "packed"])
@pytest.mark.parametrize("name", list(kc.BUILDERS))
def test_keypass_case(name, packed):
    import torch
    from sentinel_amd import _lib, cluster
    L = _lib.load()
    dev = torch.device("cuda", 0)
    sparse = name in kc.SPARSE
    bs, _ = kc.case(name)
    rep = kc.replay(name)
    fid, count, sample, interval = kc.rules(sparse)
    eng = cluster.Engine(max_batch=1 << 16, max_rules=1 << 16, hot_rules=True, hot_min_requests=1, small_batch=0)
    try:
        cluster.ClusterFlowRuleManager(eng).load_rule_arrays("default", fid, count, threshold_type=1, sample_count=sample,
                                                             window_interval_ms=interval)
        for bi, b in enumerate(bs):
            ctx = f"{name} batch {bi} ({b.claims['path']})"
            got = submit(L, eng, dev, b, sparse, packed)
            info = eng.batch_info()
            exp = rep["results"][bi]
            bad = np.nonzero((got[0] != exp[0]) | (got[1] != exp[1]) | (got[2] != exp[2]))[0]
            if len(bad):
                i = int(bad[0])
                raise AssertionError(f"{ctx}: {len(bad)} of {b.n} requests differ; first at {i} (round {i // 64} lane "
                                     f"{i % 64}): rule {b.lid[i]} gpu=({got[0][i]},{got[1][i]},{got[2][i]}) "
                                     f"oracle=({exp[0][i]},{exp[1][i]},{exp[2][i]}) info={info}")
            assert {k: info[k] for k in WORDS} == b.expect, (ctx, info)
            assert info["hot_err"] == 0, (ctx, info)
        svc = cluster.DefaultTokenService(eng)
        for f, o in rep["sums"].items():
            g = svc.metric_sums(f, rep["now"])
            assert g == o, (name, f, g, o)
    finally:
        eng.close()
