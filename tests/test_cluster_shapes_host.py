"""The cases of tests/cluster_shapes.py against the oracle alone (no GPU): what keeps
tests/test_cluster_shapes_gpu.py from being vacuous.

* every row of a case's shape table equals what is counted from the arrays: after a stable sort by (rule, bucket)
  the run lengths and prioritized counts, the positions relative to the 2048-element chunks, the bin populations,
  the batch sizes and key-segment counts are the named numbers;
* every targeted rule has the outcome mix its row names in the oracle's answers: passes and blocks, SHOULD_WAIT
  present or absent (and how many), the position of the first answer that is not OK, and the escapes (acquire
  above 127, mixed acquire, bucket delta from 63) are in the arrays exactly where the row says; the metric sums
  read after the step still hold the rule's last run;
* per group, the seams the group exists for are all in its tables."""
import numpy as np
import pytest

from tests import cluster_shapes as cs

CASES = list(cs.BUILDERS)


def rule_view(c, step, rule):
    """(arrival indices, bucket numbers, run lengths, prioritized per run) of a rule's requests in a step."""
    s = c.steps[step]
    idx = np.nonzero(s["fid"] == rule)[0]
    q = s["ts"][idx] // c.bucket_len(rule)
    cut = np.nonzero(np.diff(q))[0] + 1
    parts = np.split(np.arange(len(idx)), cut)
    return idx, q, [len(p) for p in parts], [int(s["prio"][idx[p]].sum()) for p in parts]


@pytest.mark.parametrize("name", CASES)
def test_batches_are_well_formed(name):
    c = cs.case(name)
    assert c.table and len(c.fillers) == 3 and not set(c.fillers) & set(c.targets)
    assert cs.T0 % 1000 == 0
    last = 0
    for s in c.steps:
        if s["kind"] == "hot":
            continue
        n = len(s["fid"])
        assert 0 < n <= c.max_batch and n <= 1 << 22
        assert (np.diff(s["ts"]) >= 0).all(), "sorted clock"
        assert s["ts"][0] >= last, "steps in time order"
        last = int(s["ts"][0])
        if s["kind"] == "token":
            assert len(s["acq"]) == len(s["prio"]) == len(s["ts"]) == n
            if c.mode == "small" and not c.name.startswith("S_"):
                assert n <= 4096
            elif c.mode != "small":
                assert n > 4096 or c.engine_args["small_batch"] == 0
    if c.mode == "bin":
        assert c.n_rules >= 28671 and c.engine_args["hot_rules"]
    if c.mode == "hot":
        assert c.n_rules < 28671 and c.engine_args["hot_rules"]
    # a case of fewer than 100k requests per batch, but for group P
    if not name.startswith("P_"):
        assert max(len(s["fid"]) for s in c.steps if s["kind"] != "hot") < 100_000


@pytest.mark.parametrize("name", CASES)
def test_shape_table_is_what_the_arrays_hold(name):
    c = cs.case(name)
    rep = cs.replay(name)
    layouts = {}

    def layout(step):
        if step not in layouts:
            layouts[step] = cs.sorted_layout(c, step)
        return layouts[step]

    for r in c.table:
        step, rule, ctx = r["step"], r["rule"], (name, r["rule"], r["seam"])
        s = c.steps[step]
        if rule < 0:  # a row about the batch
            if "n" in r:
                assert len(s["fid"]) == r["n"], ctx
            if "nseg" in r:
                assert -(-len(s["fid"]) // cs.SEG) == r["nseg"], ctx
            if "small" in r:
                assert (len(s["fid"]) <= min(c.engine_args["small_batch"], 4096)) == r["small"], ctx
            if "candidates" in r:
                assert len(np.unique(s["fid"])) == r["candidates"] and s["fid"].min() >= 1, ctx
                cnt = np.bincount(s["fid"])[1:]
                assert cnt.min() >= 8 and cnt.max() <= 15, ctx  # one log2 bin, at most 256 rule heads per chunk
                assert cs.hot_next(c, step) == r["hot_next"], (ctx, cs.hot_next(c, step))
            if "chunk_rules" in r:
                f, _ = layout(step)
                lo = r["chunk"] * cs.CHUNK
                heads = np.concatenate([[0], np.nonzero(np.diff(f))[0] + 1])
                assert int(((heads >= lo) & (heads < lo + cs.CHUNK)).sum()) == r["chunk_rules"], ctx
                assert lo in heads and lo + cs.CHUNK in heads and f[lo] == r["first_rule"], ctx
            continue
        idx, q, runs, prio = rule_view(c, step, rule)
        assert runs == r["runs"] and prio == r["prio"], (ctx, runs, prio)
        st = rep["results"][step][0][idx]
        # ---- what the oracle answers
        mix = r.get("mix")
        if mix == "both":
            assert (st == 0).any() and (st == 1).any(), ctx
        elif mix == "pass":
            assert (st == 0).all(), ctx
        elif mix == "block":
            assert (st == 1).all(), ctx
        else:
            raise AssertionError(ctx)
        assert set(np.unique(st)) <= {0, 1, 2}, ctx
        if "wait" in r:
            assert bool((st == 2).any()) == r["wait"], (ctx, int((st == 2).sum()))
        if "waits" in r:
            assert int((st == 2).sum()) == r["waits"], (ctx, int((st == 2).sum()))
        if "first_block" in r:
            nz = np.nonzero(st != 0)[0]
            assert (int(nz[0]) if len(nz) else None) == r["first_block"], (ctx, nz[:3])
        # ---- the sums read after the step still hold the rule's last run of it (the GPU comparison is not 0 == 0)
        t, sums = rep["step_sums"][step]
        last = st[len(st) - runs[-1]:]
        assert t == int(s["ts"].max()) + 1 and t - int(s["ts"][idx[-1]]) <= c.interval[rule - 1], ctx
        assert sums[rule][2] >= int((last == 0).sum()) and sums[rule][3] >= int((last == 1).sum()), (ctx, sums[rule])
        assert sums[rule][6] >= int((last == 2).sum()) and sum(sums[rule]) > 0, (ctx, sums[rule])
        # ---- escapes to the per-request replay: exactly where the row says
        acq = s["acq"][idx]
        w = c.bucket_len(rule)
        delta = q - int(s["ts"].min()) // w
        parts = np.split(acq, np.cumsum(runs)[:-1])
        found = ("acquire" if (acq > cs.K_ACQ_MAX).any() else
                 "mixed" if any(len(set(p.tolist())) > 1 for p in parts) else
                 "delta" if (delta >= cs.K_BD_ESC).any() else None)
        if not r.get("hot"):  # (a hot rule's requests are not packed into sort elements)
            assert found == r.get("escape"), (ctx, found)
        if "delta" in r:
            assert int(delta.max()) == r["delta"], (ctx, int(delta.max()))
        # ---- where the rule lies in the sorted batch
        if "head" in r or "bin" in r:
            f, _ = layout(step)
            at = np.nonzero(f == rule)[0]
            assert len(at) == len(idx) and (np.diff(at) == 1).all(), ctx
        if "head" in r:
            assert (int(at[0]), int(at[-1]) + 1) == (r["head"], r["end"]), ctx
            c1 = (r["head"] // cs.CHUNK + 1) * cs.CHUNK
            assert max(0, r["end"] - c1) == r["past"], ctx
            if "run_starts_after_h0" in r:
                lo = r["head"] // cs.CHUNK * cs.CHUNK
                assert r["h0"] == lo and f[lo] != f[lo - 1], ctx  # the chunk's first element is a rule head
                starts = r["head"] + np.concatenate([[0], np.cumsum(runs)[:-1]]) - lo
                assert starts.tolist() == r["run_starts_after_h0"], (ctx, starts)
        if "bin" in r:
            assert (rule - 1) >> cs.BIN_LB == r["bin"], ctx
            inbin = (f - 1) >> cs.BIN_LB == r["bin"]
            assert int(inbin.sum()) == r["bin_n"], (ctx, int(inbin.sum()))
            if "bin_runs" in r:
                key = f[inbin] * 1000 + s["ts"][layout(step)[1][inbin]] // w % 1000
                assert len(np.unique(key)) == r["bin_runs"], ctx
        if "second_bucket_at" in s["info"]:
            first = np.nonzero(s["ts"] // cs.W != s["ts"][0] // cs.W)[0][0]
            assert int(first) == s["info"]["second_bucket_at"] and s["fid"][first] >= 1, ctx
        if "at" in r:
            assert idx.tolist() == list(range(*r["at"])), ctx
        if r.get("hot"):  # in the hot set the batch before picked (the restatement of k_hot_pick's rule)
            hs = cs.hot_set(c, step)
            assert hs is not None and rule in hs, ctx
        elif "hot" in r and c.engine_args["hot_min_requests"] < cs.NEVER_HOT and step:
            assert rule not in cs.hot_set(c, step), ctx


def seams(names):
    return " | ".join(r["seam"] for n in names for r in cs.case(n).table)


@pytest.mark.parametrize("mode", list(cs.MODES))
def test_group_R_covers_its_seams(mode):
    c = cs.case(f"R_{mode}")
    rows = [r for r in c.table if len(r["runs"]) == 1]
    for n in cs.R_SIZES:
        assert sum(1 for r in rows if r["runs"] == [n] and r["prio"] == [0] and not r["wait"]) == 1, n
        assert sum(1 for r in rows if r["runs"] == [n] and r["wait"] and r["waits"] >= 1) == 1, n
    assert {r["prio"][0] for r in rows} >= {0, 1, 4, 5, 65}
    assert {0, 39, None} <= {r["first_block"] for r in rows if r["runs"] == [40]}
    assert any(len(r["runs"]) == 3 for r in c.table)
    # a prioritized count above 4 takes prio_before's search, up to 4 its four loads
    assert any(r["prio"][0] == 4 and r["wait"] for r in rows) and any(r["prio"][0] == 5 and r["wait"] for r in rows)


def test_group_L_covers_its_seams():
    c = cs.case("L_bin")
    assert {r["bin_runs"] for r in c.table} == {cs.K_LONG - 1, cs.K_LONG, cs.K_LONG + 1}
    assert all(n > cs.K_DIRECT for r in c.table for n in r["runs"])
    huge = [r for r in c.table if cs.K_HUGE in r["runs"]]
    assert len(huge) == 1 and huge[0]["bin_runs"] == cs.K_LONG + 1
    for b in {r["bin"] for r in c.table}:
        assert sum(1 for r in c.table if r["bin"] == b) == 32  # every rule of the bin


def test_group_C_small_path():
    for n in (4095, 4096):
        c = cs.case(f"C_small{n}")
        r = c.table[0]
        assert len(c.steps[0]["fid"]) == n and (r["head"], r["end"], r["past"]) == (cs.CHUNK - 1, n, n - cs.CHUNK)


@pytest.mark.parametrize("name", [n for n in cs.GROUPS["C"] if "small" not in n])
def test_group_C_covers_its_seams(name):
    c = cs.case(name)
    k = cs.CHUNK
    rows = [r for r in c.table if r["rule"] > 0]
    assert {r["past"] for r in rows} >= {0, 1, 2047, 2048, 2049, 4095, 4096, 4097, 5 * k - 1, 5 * k + 1}
    assert any(r["head"] % k == k - 1 for r in rows) and any(r["head"] % k == 0 for r in rows)
    assert any(r["end"] % k == 0 and r["past"] == 0 for r in rows)
    assert {r["chunk_rules"] for r in c.table if r["rule"] < 0} == {255, 256, 257, k}
    f, _ = cs.sorted_layout(c, 0)
    s = c.steps[0]
    assert len(f) == s["info"]["n_valid"] and len(s["fid"]) - len(f) == s["info"]["n_invalid"]
    heads = np.concatenate([[0], np.nonzero(np.diff(f))[0] + 1])
    assert len(set(range(len(f) // k)) - set((heads // k).tolist())) >= 4, "chunks without a rule head"
    last = max(rows, key=lambda r: r["end"])
    assert last["end"] == len(f) and last["past"] > 0  # the last rule continues to the end of the valid elements
    assert ((s["fid"] == 0).sum() > 0) == (s["info"]["n_invalid"] > 0)


def test_group_B_covers_its_seams():
    c = cs.case("B_bins")
    pops = {r["bin_n"] for r in c.table}
    b = cs.K_BIN_LDS
    assert pops >= {1, b - 1, b, b + 1, 4 * cs.K_BO - 1, 4 * cs.K_BO, 4 * cs.K_BO + 1}
    per_bin = {}
    for r in c.table:
        per_bin.setdefault(r["bin"], set()).add(r["rule"])
    f, _ = cs.sorted_layout(c, 1)
    used = set(((f - 1) >> cs.BIN_LB).tolist())
    assert any(len(v) == 32 for v in per_bin.values())
    assert any(len(v) == 1 and int(((f - 1) >> cs.BIN_LB == bn).sum()) > 3000 for bn, v in per_bin.items())
    assert len(used) < (c.n_rules >> cs.BIN_LB), "empty bins"
    for where, sizes in (("LDS", cs.R_SIZES), ("global", cs.R_SIZES)):
        got = {r["runs"][0] for r in c.table if where + " bin" in r["seam"] and r["prio"] == [0]}
        assert got >= set(sizes), (where, got)
    assert any("LDS bin" in r["seam"] and r["wait"] for r in c.table)
    assert any("global bin" in r["seam"] and r["wait"] for r in c.table)
    big = cs.case("B_big")
    assert big.table[0]["bin_n"] > 65536


def test_group_E_covers_its_seams():
    for name in ("E_sort", "E_small"):
        t = cs.case(name).table
        assert [r.get("escape") for r in t] == [None, None, "acquire", "acquire", "mixed", None, None, None, None, None,
                                                "delta", "delta"]
        assert [r["delta"] for r in t if "delta" in r] == [62, 63, 64]
    h = cs.case("E_hotmix")
    assert sum(1 for r in h.table if r.get("escape") == "delta") == 12 and h.table[-1]["hot"]
    s = h.steps[1]
    assert (int(s["ts"].max()) // 100 - int(s["ts"].min()) // 100) < cs.K_HOT_BUCKETS  # the hot rules stay inside


def test_group_S_P_sizes():
    assert [r["n"] for r in cs.case("S_small").table] == [1, 63, 64, 65, 4095, 4096, 4097]
    assert [r["small"] for r in cs.case("S_small").table] == [True] * 6 + [False]
    assert [r["small"] for r in cs.case("S_sort").table] == [False] * 3
    assert [(r["n"], r["small"]) for r in cs.case("S_1000").table] == [(1000, True), (1001, False)]
    p = cs.case("P_part")
    assert p.n_rules >= 28671
    got = sorted((r["nseg"], (r["n"] - 1) % cs.SEG + 1) for r in p.table[1:])
    assert got == sorted([(s, cs.SEG) for s in (1, 8, 9, 16, 17, 64, 65)] + [(s, 1) for s in (1, 8, 9, 16, 17, 64, 65)])
    q = cs.case("P_256")
    assert sorted(r["n"] for r in q.table[1:]) == sorted([256 * cs.SEG, 255 * cs.SEG + 1, 257 * cs.SEG, 256 * cs.SEG + 1])


def test_group_H_spans():
    for nb in (64, 65):
        c = cs.case(f"H_span{nb}")
        s = c.steps[1]
        assert int(s["ts"].max()) // cs.W - int(s["ts"].min()) // cs.W == nb - 1
    c = cs.case("H_seg")
    assert sorted(r["prio"][0] for r in c.table if "prioritized" in r["seam"]) == [0, 1, 64, 65, 4097]
    assert [s["info"].get("second_bucket_at") for s in c.steps[2:5]] == [cs.SEG - 1, cs.SEG, cs.SEG + 1]


def test_group_M_steps():
    c = cs.case("M_mixed")
    assert [s["kind"] for s in c.steps] == ["token", "rls", "hot", "token", "hot", "token", "token"]
    assert c.n_rules == 30000 and len(c.steps[0]["fid"]) == 3 * cs.SEG + 17 and len(c.steps[1]["fid"]) == 5000
    assert len(c.steps[3]["fid"]) > 4096 and not c.steps[2]["on"] and c.steps[4]["on"]
    rep = cs.replay("M_mixed")
    for r in rep["results"]:
        if r is not None:
            assert (r[0] == 0).any() and (r[0] == 1).any()


@pytest.mark.parametrize("name", ["E_hotmix"] + [n for n in cs.GROUPS["H"] if n != "H_drop"])
def test_first_batch_drops_no_hot_candidate(name):
    """With hot_min_requests = 1 every rule of the all-cold first batch is a candidate for the hot set, and a cold
    workgroup publishes at most 256: no chunk of 2048 sorted elements may hold more rule heads, or the hot set the
    rows rely on (and cluster_shapes.hot_set restates) would not be the one the engine picks."""
    c = cs.case(name)
    assert c.engine_args["hot_min_requests"] == 1
    f, _ = cs.sorted_layout(c, 0)
    heads = np.concatenate([[0], np.nonzero(np.diff(f))[0] + 1])
    assert np.bincount(heads // cs.CHUNK).max() <= 256


def test_group_H_next_hot_set():
    """The restatement of the pick rule on the cases built for it: 4095 / 4096 candidates are all picked, 4097 none;
    257 candidates in one chunk lose one; sampleCount 1 and 65 never turn hot."""
    assert [cs.hot_next(cs.case("H_pick"), j) for j in range(5)] == [cs.K_HOT - 1, cs.K_HOT, 0, 500, 500]
    d = cs.case("H_drop")
    h = cs.hot_history(d)[0]
    assert h[0] is None and h[2] == 1 and cs.hot_next(d, 0) == h[3] - 1 == d.steps[0]["info"]["n_hot_next"]
    sm = cs.case("H_sample")
    for step in (1, 2):
        hs = set(cs.hot_set(sm, step).tolist())
        assert {11, 12} <= hs and not {10, 13} & hs
    assert {r["sample"] for r in sm.table} == {1, 2, 64, 65}
    p = cs.case("H_prio")
    assert [int(s["prio"].sum()) for s in p.steps[1:]] == [4 * cs.K_HOT - 1, 4 * cs.K_HOT + 1]
