"""The cases of tests/keypass_cases.py against the oracle alone (no GPU): each batch holds what its case names
and takes the path it names, so tests/test_cluster_keypass_gpu.py is not vacuous."""
import numpy as np
import pytest

from tests import keypass_cases as kc

STATUS_OK_BLOCK_WAIT = {0, 1, 2}


@pytest.mark.parametrize("name", list(kc.BUILDERS))
def test_case_holds_what_it_names(name):
    bs, sets = kc.case(name)
    rep = kc.replay(name)
    known = np.concatenate([kc.POOL, kc.COLD])
    last = 0
    assert bs[0].claims["path"] == "first" and bs[0].expect["hot_mode"] == 0 and bs[0].expect["flags"] == 0
    for bi, (b, hot) in enumerate(zip(bs, sets)):
        ctx = (name, bi)
        cl, ex = b.claims, b.expect
        st = rep["results"][bi][0]
        assert 2 * kc.SEG < b.n <= 3 * kc.SEG, ctx  # two or three key segments
        assert b.ts[0] >= last and b.base <= b.ts.min(), ctx
        last = b.end()
        # every rule has FLOOR requests: the next hot set is every 1000 ms rule
        ids, cnt = np.unique(b.lid[np.isin(b.lid, known) & (b.acq >= 1)], return_counts=True)
        assert len(ids) == len(known) and cnt.min() >= kc.FLOOR - 1 and ids[np.argmax(cnt)] == 1, ctx
        if bi:
            assert np.array_equal(hot, kc.POOL), ctx
        # ---- the path
        path = cl["path"]
        if path in ("hot", "first"):
            assert ex["flags"] == 0 and ex["hot_mode"] == (1 if path == "hot" else 0), ctx
            assert (np.diff(b.ts) >= 0).all(), ctx
        else:
            assert ex["hot_mode"] == 0 and ex["flags"] == kc.PATH_FLAG[path], (ctx, ex)
            assert ex["n_cold"] == int((np.isin(b.lid, known) & (b.acq >= 1)).sum()), ctx
            assert bs[bi + 1].claims["path"] == "hot" or name == "sparse", ctx  # pass 1, then the hot path again
        if path == "hot":
            assert 0 < ex["n_cold"] < b.n // 4, ctx  # most requests are hot
        q = b.ts // kc.WH - b.base // kc.WH
        starts = (np.nonzero(np.diff(q))[0] + 1).tolist()
        if "boundaries" in cl:
            assert starts == sorted(cl["boundaries"]), (ctx, starts)
            assert (np.diff(q)[np.array(starts) - 1] == cl.get("jump", 1)).all(), ctx
            assert ex["bd_lo"] == 0 and ex["bd_hi"] == cl.get("jump", 1) * len(starts), (ctx, ex)
        if "backward" in cl:
            at = cl["backward"]
            assert (np.nonzero(np.diff(b.ts) < 0)[0] + 1).tolist() == [at], ctx
        if "span" in cl:
            assert q.max() - q.min() + 1 == cl["span"] and (np.diff(b.ts) >= 0).all(), ctx
            assert (cl["span"] > kc.K_HOT_BUCKETS) == (path == "bucket"), ctx
        if "cross" in cl:
            x = b.base % kc.WH + (b.ts - b.base)
            at = cl["cross"]
            assert (b.ts - b.base).max() < 1 << 32 and at % kc.ROUND not in (0, 63), ctx
            assert (x[:at] < 1 << 32).all() and (x[at:] >= 1 << 32).all(), ctx
            assert ex["bd_lo"] == kc.K_HOT_BUCKETS - 1, ctx
        # ---- rare lanes: alone in a round of valid hot requests, and answered as the kind says
        for (kind, lane), i in cl.get("rare", {}).items():
            r0 = i - lane
            assert i % kc.ROUND == lane and lane in (0, 63), (ctx, kind)
            others = np.delete(np.arange(r0, r0 + kc.ROUND), lane)
            assert np.isin(b.lid[others], hot).all() and (b.acq[others] == 1).all() and not b.prio[others].any(), (ctx, kind)
            assert set(st[others]) <= STATUS_OK_BLOCK_WAIT, (ctx, kind)
            if kind in ("fid0", "acq0", "resv"):
                assert st[i] == st[cl["rare"][("fid0", 0)]] and st[i] not in STATUS_OK_BLOCK_WAIT, (ctx, kind, st[i])
                assert (i in b.resv) == (kind == "resv"), (ctx, kind)
            elif kind in ("hole", "beyond"):
                assert b.lid[i] not in known and st[i] == st[cl["rare"][("hole", 0)]], (ctx, kind)
                assert st[i] not in STATUS_OK_BLOCK_WAIT and st[i] != st[cl["rare"][("fid0", 0)]], (ctx, kind)
                assert (b.lid[i] > known.max()) == (kind == "beyond"), (ctx, kind)
            elif kind == "acq128":
                assert b.lid[i] in kc.COLD and b.acq[i] == 128 and st[i] in STATUS_OK_BLOCK_WAIT, (ctx, kind)
            elif kind.startswith("delta"):
                d = int(kind[5:])
                assert b.lid[i] in kc.COLD and b.ts[i] // kc.WC - b.base // kc.WC == d, (ctx, kind)
                assert st[i] in STATUS_OK_BLOCK_WAIT, (ctx, kind)
            elif kind == "mixed":
                assert b.lid[i] in hot and b.acq[i] not in (0, 1) and path == "mixed", (ctx, kind)
            else:
                raise AssertionError((ctx, kind))
    # the sums the GPU test compares are not all zero
    assert sum(sum(v) for v in rep["sums"].values()) > 0, name


def test_seams_are_covered():
    """Every position the key pass treats differently is named by some case."""
    starts = sorted({s for name in ("boundary_a", "boundary_b", "boundary_c") for b in kc.case(name)[0]
                     for s in b.claims.get("boundaries", [])})
    for edge in (kc.ROUND, kc.CHUNK, kc.SUB, kc.SEG):
        assert {edge - 1, edge, edge + 1} <= set(starts), edge
    assert {s % kc.ROUND for s in starts} >= {1, 62}
    back = [b.claims["backward"] for b in kc.case("backward")[0] if "backward" in b.claims]
    assert {a % kc.ROUND for a in back} >= {0, 1, 63} and any(a % kc.SUB == 0 for a in back)
    assert any(a % kc.SEG == 0 for a in back)
    rare = kc.case("rare")[0][1].claims["rare"]
    kinds = set(kc.RARE_KINDS) | {f"delta{d}" for d in (62, 63, 64)}
    assert {(k, l) for k in kinds for l in (0, 63)} == set(rare)
    assert set(kc.case("sparse")[0][3].claims["rare"]) == set(rare)
    assert {l for (_, l) in [k for b in kc.case("mixed")[0] for k in b.claims.get("rare", {})]} == {0, 63}
    assert sorted(b.n % kc.ROUND for b in kc.case("tail")[0][1:]) == [0, 0, 1, 63]
    assert any(b.n % kc.SUB == 1 for b in kc.case("tail")[0][1:])
    first_round = kc.case("multi")[0][2]
    assert first_round.claims["boundaries"][0] < kc.ROUND
