"""The streams of tests/local_shapes.py against the oracle alone (no GPU): what keeps
tests/test_local_shapes_gpu.py from being vacuous.

* the shape table equals what is counted from the arrays (events per resource and chunk, entries per run,
  chunk sizes), and the builders' common rules hold (filler, time seams, carried buckets, legal exits);
* every targeted resource whose rule can block has at least one pass and at least one block in every chunk;
* every breaker reaches the states its case names, tripping at the planned exit and not one earlier;
* every equality case hits its equality: the colliding values are recomputed here from the stream and the rule.

The engine keeps no count of the windows k_lwave walked by summaries, of the form a k_entry_stats tile took, or
of the closed form inside lane_run; for those the input shapes asserted here are the evidence."""
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest

from tests import local_shapes as ls

CASES = list(ls.BUILDERS)
_replays = {}


def replay(name):
    """[(decisions, waits)] per chunk of the case, from one oracle replay shared by the tests."""
    if name not in _replays:
        c = ls.case(name)
        orc = c.oracle()
        _replays[name] = [orc.replay(ch) for ch in c.chunks]
        orc.close()
    return _replays[name]


def passed(dec):
    return (dec == 0) | (dec == 4)


@pytest.mark.parametrize("name", CASES)
def test_shape_table_is_what_the_arrays_hold(name):
    c = ls.case(name)
    assert c.table and len(c.chunks) >= 2
    assert ls.T0 % 1000 == 0
    ruled = {r["resource"] for r in c.flow + c.param + c.degrade}
    assert all(r < c.first_filler for r in ruled), "filler resources carry no rule"
    for ci, ch in enumerate(c.chunks):
        n = len(ch["kind"])
        assert all(len(ch[k]) == n for k in ls.COLS)
        assert n <= (c.max_batch or n) or c.meta.get("chunks_per_call", [1] * 9)[ci] == 2, "one call per chunk"
        if not c.small_ok:
            assert n > ls.K_SMALL, (ci, n)
        # at least 300 filler resources, a few events each; the sort key is wider than one 8-bit digit
        fill = ch["resource"][ch["resource"] >= c.first_filler]
        cnt = np.bincount(fill - c.first_filler)
        assert (cnt > 0).sum() >= 300 and cnt.max() <= 16, (ci, (cnt > 0).sum(), cnt.max())
        assert c.n_res > 256
        if c.sorted_chunks:
            assert int((np.diff(ch["ts"]) < 0).sum()) == c.meta.get("regressions", {}).get(ci, 0), ci
            if ci:  # carried state: the chunk begins in the bucket in which the previous one ended
                assert ch["ts"].min() // 500 == c.chunks[ci - 1]["ts"].max() // 500, ci
    rows = {(r["res"], r["chunk"]): r for r in c.table}
    assert len(rows) == len(c.table)
    for (res, ci), r in rows.items():
        n, runs = ls.counted_row(c.chunks[ci], res)
        assert (n, runs) == (r["events"], r["run_entries"]), (res, ci, r["seam"])
        assert len(runs) >= 2 or r["single_run"], (res, ci, r["seam"])
    # every targeted resource's events of every chunk are in the table (A and C end with a chunk that only
    # takes the exits left over)
    for ci, ch in enumerate(c.chunks[:-1] if name in ("A", "C") else c.chunks):
        for res in np.unique(ch["resource"][ch["resource"] < c.first_filler]):
            assert (int(res), ci) in rows, (res, ci)
    if name != "E":  # group E's target is ENTRY_NODE (its own test below)
        for res in c.targets:
            t = np.concatenate([ch["ts"][ch["resource"] == res] for ch in c.chunks])
            assert (t % 500 == 0).any() and (t % 500 == 499).any() and (t % 1000 == 0).any(), res


@pytest.mark.parametrize("name", CASES)
def test_exits_are_of_entries_the_oracle_passed(name):
    """In arrival order, per resource: an exit takes the acquire count, the parameter and the parameter / inbound
    flags of an entry that passed before it and has not exited yet."""
    c = ls.case(name)
    flight = Counter()
    for ch, (dec, _) in zip(c.chunks, replay(name)):
        sel = np.nonzero((ch["resource"] < c.first_filler) & ((ch["kind"] == 1) | passed(dec)))[0]
        for i in sel:
            key = (int(ch["resource"][i]), int(ch["acquire"][i]), int(ch["param"][i]), int(ch["flags"][i]) & 12)
            if ch["kind"][i] == 1:
                flight[key] -= 1
                assert flight[key] >= 0, (name, key, int(i))
            else:
                flight[key] += 1
        assert not ((ch["kind"] == 1) & (ch["resource"] >= c.first_filler)).any()


@pytest.mark.parametrize("name", CASES)
def test_every_row_passes_and_blocks(name):
    c = ls.case(name)
    rep = replay(name)
    for r in c.table:
        ch, (dec, _) = c.chunks[r["chunk"]], rep[r["chunk"]]
        m = (ch["resource"] == r["res"]) & (ch["kind"] == 0)
        if not m.any():
            continue  # an exit-only flow
        if "pass" in r["can"]:
            assert passed(dec[m]).any(), (r["res"], r["chunk"], r["seam"])
        if "block" in r["can"]:
            assert (~passed(dec[m])).any(), (r["res"], r["chunk"], r["seam"])
    # the rules that cannot do both are the ones the builders say: no rule, a cost of 0 ms, a count of 0, a
    # CLOSED breaker, entries that all lie before an OPEN breaker's retry time; group E targets ENTRY_NODE
    lopsided = {r["seam"].split(":")[0].split(" ")[0] for r in c.table if len(r["can"]) < 2}
    assert lopsided <= {"rl_cost0", "rl_count0", "norule", "throttle_cost0", "grade", "inbound", "not",
                        "default", "two"}, lopsided


def runs_of(ch, res):
    """[(indices into the chunk)] per run of the resource."""
    idx = np.nonzero(ch["resource"] == res)[0]
    cut = np.nonzero(np.diff(ch["ts"][idx] // 500) != 0)[0] + 1
    return np.split(idx, cut)


def test_a_sizes_and_runs():
    c = ls.case("A")
    ch, (dec, _) = c.chunks[1], replay("A")[1]
    sizes = sorted(Counter(c.meta["sizes"].values()).items())
    assert sizes == [(s, 6) for s in ls.FAST_SIZES + ls.NONFAST_SIZES]  # six shapes at every size
    for res, size in c.meta["sizes"].items():
        assert int((ch["resource"] == res).sum()) == size
        can_pass = "pass" in next(r["can"] for r in c.table if r["res"] == res)
        assert (ch["kind"][ch["resource"] == res] == 1).any() or not can_pass, "exits among the events"
        fast = ls.rule_shape(c, res)[0]
        assert (fast != 0) == (size in ls.FAST_SIZES), res
    assert len(c.meta["run_resources"]) == 7
    for res in c.meta["run_resources"]:
        assert ls.rule_shape(c, res)[0] != 0 and int((ch["resource"] == res).sum()) >= ls.K_WAVE
        runs = runs_of(ch, res)
        assert all((ch["kind"][r] == 0).all() for r in runs[1:-1])  # the measured runs hold entries only
        assert [len(r) for r in runs[1:-1]] == list(ls.RUN_ENTRIES), res
    # the saturated RateLimiter: its long runs pass one entry and block the rest
    sat = c.meta["run_resources"][-1]
    rule = next(f for f in c.flow if f["resource"] == sat)
    wait = replay("A")[1][1]
    at_limit = 0
    for r in runs_of(ch, sat):
        if len(r) >= 511:
            assert passed(dec[r]).sum() <= 2 and (~passed(dec[r])).sum() >= 509
            p = r[passed(dec[r])]
            # the pass waits exactly maxQueueingTimeMs, and it lies in the interior of the run (not within its
            # first or last 64 events, whichever way the 64-event windows fall)
            at_limit += int(((wait[p] == rule["max_queueing_time_ms"]) & (p >= r[64]) & (p < r[-64])).sum())
    assert at_limit >= 3, at_limit
    # greedy and WarmUp resources mix acquire counts inside a run, the closed-form ones do not
    for res in c.meta["sizes"]:
        name = next(r["seam"] for r in c.table if r["res"] == res)
        a = ch["acquire"][(ch["resource"] == res) & (ch["kind"] == 0)]
        assert (len(np.unique(a)) == 1) == name.startswith(("default", "rl")), name


def test_b_positions():
    c = ls.case("B")
    for ci, (n0, total, one_run) in enumerate(c.meta["plan"]):
        ch = c.chunks[ci]
        assert len(ch["kind"]) == total and int((ch["resource"] == 0).sum()) == n0
        r1 = runs_of(ch, 1)
        assert len(r1[0]) == 1 and len(r1) == 3  # resource 1's second run starts at sorted position n0 + 1
        assert (len(runs_of(ch, 0)) == 1) == one_run
        assert (ch["kind"][ch["resource"] == 0] == 1).any() or ci == 0
    plan = c.meta["plan"]
    assert [p[0] for p in plan[:3]] == [ls.K_TILE - 1, ls.K_TILE, ls.K_TILE + 1]
    assert plan[0][0] + 1 == ls.K_TILE, "a bucket change inside resource 1's flow at sorted position 4096"
    assert plan[3][0] == 2 * ls.K_TILE + 1 and plan[3][2]
    assert sorted(p[1] for p in plan if not p[2]) == [4096, 4097, 8192, 8192, 8193]


def _param_rule(c, res):
    return next(r for r in c.param if r["resource"] == res)


def test_c_segments_and_equalities():
    c = ls.case("C")
    ch, (dec, wait) = c.chunks[1], replay("C")[1]
    for res in range(4):
        m = ch["resource"] == res
        assert (ch["flags"][m] & ls.EV_HAS_PARAM).all()
        seg = {int(v): np.nonzero(m & (ch["param"] == v))[0] for v in np.unique(ch["param"][m])}
        for n, v in ls.V_SEG.items():  # regular: entries only, one acquire count, times that do not go back
            i = seg[v]
            assert len(i) == n and (ch["kind"][i] == 0).all() and (ch["acquire"][i] == 1).all()
            assert (np.diff(ch["ts"][i]) >= 0).all()
        i = seg[ls.V_ACQ]
        assert list(np.nonzero(ch["acquire"][i] != 1)[0]) == [63] and (np.diff(ch["ts"][i]) >= 0).all()
        i = seg[ls.V_BACK]
        assert list(np.nonzero(np.diff(ch["ts"][i]) < 0)[0] + 1) == [63] and ch["ts"][i][63] - ch["ts"][i][62] == -1
        for v, n in ((ls.V_EX1, 1), (ls.V_EX2, 2), (ls.V_EX64, 64)):
            assert len(seg[v]) == n and (ch["kind"][seg[v]] == 1).all()
        assert 0 in seg and len(seg[ls.ALL_ONES]) == 64
        rule = _param_rule(c, res)
        if rule.get("control_behavior", 0) == 0:
            # token bucket: the entries passTime == duration (no refill: blocked, the bucket is dry) and + 1 ms
            i = seg[ls.V_REFILL]
            dur = rule.get("duration_in_sec", 1) * 1000
            last_add = ch["ts"][i][0]  # the value's first entry ever (not in chunk 0)
            assert not (c.chunks[0]["param"][c.chunks[0]["resource"] == res] == ls.V_REFILL).any()
            eq = [k for k in i if ch["ts"][k] - last_add == dur]
            nx = [k for k in i if ch["ts"][k] - last_add == dur + 1]
            assert len(eq) == 1 and len(nx) >= 1
            room = int(rule["count"]) + rule.get("burst_count", 0)
            n_first = int((ch["ts"][i] == last_add).sum())
            if n_first > room:  # dry: only a refill lets the next one pass
                assert dec[eq[0]] == 2 and dec[nx[0]] == 0, (res, dec[i])
            else:
                assert dec[eq[0]] == 0 and dec[nx[0]] == 0
            # the same equality inside a long regular segment: the value's first entry ever was at T0 (chunk 0,
            # which drained its tokens), the segment of 64 starts at T0 + duration
            i = seg[ls.V_SEG[64]]
            c0 = c.chunks[0]
            first = c0["ts"][(c0["resource"] == res) & (c0["param"] == ls.V_SEG[64])]
            assert first.min() == ls.T0 and (first == ls.T0).sum() > room
            eq = i[ch["ts"][i] - ls.T0 == dur]
            later = i[ch["ts"][i] - ls.T0 > dur]
            assert len(eq) >= 1 and (dec[eq] == 2).all() and dec[later[0]] == 0, (res, dec[i][:8])
        elif rule["max_queueing_time_ms"] > 0:
            # throttle: replay the value's entries; the waits that equal the queueing limit block (wait < limit)
            cost = int(Fraction(1000 * rule.get("duration_in_sec", 1), int(rule["count"])) + Fraction(1, 2))
            maxq = rule["max_queueing_time_ms"]

            def walk(i):
                """The value's entries (its first ever) replayed: {wait - limit: [passed]}."""
                latest, hits = None, {}
                for k in i:
                    t = int(ch["ts"][k])
                    if latest is None:
                        latest, ok, w = t, True, 0
                    else:
                        exp = latest + cost
                        ok = exp <= t or exp - t < maxq
                        w = max(exp - t, 0) if ok else 0
                        hits.setdefault(exp - t - maxq, []).append(ok)
                        if ok:
                            latest = max(exp, t)
                    assert (dec[k] == 0) == ok and wait[k] == w, (res, k, dec[k], wait[k], ok, w)
                return hits

            hits = walk(seg[ls.V_QUEUE])
            assert hits.get(0) and not any(hits[0]) and hits.get(-1) and all(hits[-1]) and hits.get(1) \
                and not any(hits[1]), hits
            # and inside the long regular segments (k_pseg_long's search for the next entry that may queue)
            for n in (63, 65, 129):
                hits = walk(seg[ls.V_SEG[n]])
                assert hits.get(0) and not any(hits[0]), (n, sorted(hits))
    for res, heavy in ((4, True), (5, False)):
        m = ch["resource"] == res
        assert (int(m.sum()) >= ls.K_HEAVY) == heavy and ls.rule_shape(c, res)[0] == 0
        vals = ch["param"][m]
        assert (vals == ls.ALL_ONES).sum() >= 10 and (vals == 0).any()
        assert len(np.unique(vals)) > 1024 or not heavy


def test_d_trips_states_and_equalities():
    for name in ls.GROUPS["D"]:
        c = ls.case(name)
        flows = c.meta["flows"]
        ch = c.chunks[1]
        orc = c.oracle()
        orc.replay(c.chunks[0])
        assert all(orc.cb_state(f["res"], 0) == 0 for f in flows)
        # the trip's exit and the one before it, found in the chunk; the chunk replayed in pieces between them
        marks = []
        for f in flows:
            i = np.nonzero(ch["resource"] == f["res"])[0]
            assert len(i) == f["n"] and (ch["kind"][i] == 1).all()
            f["idx"] = i
            if f["trip"] is not None:
                marks.append((int(i[f["trip"]]), f))
        lo = 0
        for g, f in sorted(marks, key=lambda x: x[0]):
            orc.replay({k: np.ascontiguousarray(v[lo:g]) for k, v in ch.items()})
            assert orc.cb_state(f["res"], 0) == 0, (name, f["res"], "tripped early")
            orc.replay({k: np.ascontiguousarray(v[g:g + 1]) for k, v in ch.items()})
            assert orc.cb_state(f["res"], 0) == 1, (name, f["res"], "no trip at the planned exit")
            lo = g + 1
        orc.replay({k: np.ascontiguousarray(v[lo:]) for k, v in ch.items()})
        for f in flows:
            assert orc.cb_state(f["res"], 0) == (0 if f["trip"] is None else 1)
        # the equalities, recomputed from the exits and the rule
        for f in flows:
            rule = next(r for r in c.degrade if r["resource"] == f["res"])
            i, si = f["idx"], rule["stat_interval_ms"]
            thr = Fraction(rule["slow_ratio_threshold"] if rule["grade"] == 0 else rule["count"]).limit_denominator(1000)
            bad = (ch["rt"][i] > rule["count"]) if rule["grade"] == 0 else (ch["flags"][i] & ls.EV_ERROR) != 0
            if rule["grade"] == 0 and not f["min_eq"]:
                assert (ch["rt"][i] == rule["count"]).any(), "an rt exactly at the slow-RT count (not slow)"
            win, s, tot, equal, at_trip = None, 0, 0, 0, None
            for k in range(f["n"] if f["trip"] is None else f["trip"] + 1):
                w = int(ch["ts"][i[k]]) // si
                if w != win:
                    win, s, tot = w, 0, 0
                tot += 1
                s += int(bad[k])
                fig = Fraction(s, tot) if rule["grade"] < 2 else Fraction(s)
                if k == f["trip"]:
                    at_trip = (tot, fig)
                elif tot >= rule["min_request_amount"]:
                    assert fig <= thr, (name, f["res"], k)
                    equal += fig == thr
            if f["trip"] is not None:
                assert at_trip[0] >= rule["min_request_amount"] and at_trip[1] > thr
            if f["min_eq"]:
                assert at_trip[0] == rule["min_request_amount"], "the request count equals minRequestAmount"
            else:
                assert equal > 0, "the figure touches the threshold without tripping"
        # the round / tile seams the trips sit on
        trips = {(f["n"], f["trip"]) for f in flows}
        S, R, M = ls.K_CB_SHORT, ls.K_CB_ROUND, ls.K_CB_TILE_MIN
        if name == "D4k":  # k_cb_flows<1> below S (rounds of 1024 exits), k_cb_flows<8> from S on
            assert {(S - 1, 1023), (S - 1, 1024), (S - 1, S - 2), (S, S - 1), (S + 1, S)} <= trips
        if name == "D8k":  # k_cb_flows<8>: the last exit of its first round, the first of its second, the last
            assert {(R - 1, R - 2), (R, R - 1), (R + 1, R), (R + 1, R - 1)} <= trips
        if name == "D16k":  # the tile kernels from M on, tiles of one round
            assert {(M - 1, R), (M, R - 1), (M + 1, M), (M, R)} <= trips
        # chunk 2: the retry time against the entries' timestamps
        ch2 = c.chunks[2]
        dec2, _ = orc.replay(ch2)
        for f in flows:
            j = np.nonzero(ch2["resource"] == f["res"])[0]
            assert (ch2["kind"][j] == 0).all()
            if f["trip"] is None:
                assert (dec2[j] == 0).all() and orc.cb_state(f["res"], 0) == 0
                continue
            rule = next(r for r in c.degrade if r["resource"] == f["res"])
            retry = int(ch["ts"][f["idx"][f["trip"]]]) + 1000 * rule["time_window"]
            before = j[ch2["ts"][j] < retry]
            assert ch2["ts"][before].max() == retry - 1 and (dec2[before] == 3).all()
            if f["probe"]:
                at = j[ch2["ts"][j] == retry]
                assert len(at) == 2 and dec2[at[0]] == 0 and dec2[at[1]] == 3
                assert orc.cb_state(f["res"], 0) == 2
            else:
                assert ch2["ts"][j].max() == retry - 1 and orc.cb_state(f["res"], 0) == 1
        orc.replay(c.chunks[3])
        states = {orc.cb_state(f["res"], 0) for f in flows if f["trip"] is not None and f["probe"]}
        assert states == {0, 1} or name != "D4k", "a probe's exit closes one breaker and reopens another"
        orc.close()


def test_e_entry_node_tiles():
    c = ls.case("E")
    T = ls.K_EN_TILE
    for ci, n_in in c.meta["inbound"].items():
        ch = c.chunks[ci]
        inb = (ch["flags"] & ls.EV_INBOUND) != 0
        assert int(inb.sum()) == n_in and int((~inb).sum()) > n_in  # other events between them
        assert (np.diff(np.nonzero(inb)[0]) > 1).any()
        assert (ch["resource"][inb] < 4).all()
    assert sorted(c.meta["inbound"].values()) == [T - 1, T, T + 1, 2 * T + 1]
    ch = c.chunks[c.meta["span_chunk"]]
    assert (np.diff(ch["ts"]) >= 0).all()
    span = [int(ch["ts"][lo:lo + T].max() // 500 - ch["ts"][lo] // 500) + 1 for lo in (0, T)]
    assert span == [ls.K_EN_BUCKETS, ls.K_EN_BUCKETS + 1], span
    ch = c.chunks[c.meta["back_chunk"]]
    back = np.nonzero(np.diff(ch["ts"]) < 0)[0] + 1
    assert list(back) == [T, 2500] and ch["ts"][T] - ch["ts"][T - 1] == -1 and 2 * T < 2500 < 3 * T
    ch = c.chunks[c.meta["past_chunk"]]
    assert ch["ts"].max() < min(x["ts"].min() for x in c.chunks[:-1])
    assert ((ch["flags"] & ls.EV_INBOUND) != 0).any() and (ch["kind"] == 1).any()
    for ch in c.chunks:
        inb = (ch["flags"] & ls.EV_INBOUND) != 0
        assert (ch["kind"][inb] == 1).any() or ch is c.chunks[0]
    t = np.concatenate([x["ts"][(x["flags"] & ls.EV_INBOUND) != 0] for x in c.chunks])
    assert (t % 500 == 0).any() and (t % 500 == 499).any() and (t % 1000 == 0).any()
    assert not c.degrade and not c.param  # and no system rule: Case has none


def test_f_chunking():
    small, pipe = ls.case("Fsmall"), ls.case("Fpipe")
    for k in ls.COLS:  # the same content, and one event more
        assert (small.chunks[0][k] == pipe.chunks[0][k][:-1]).all() or k == "ts"
    assert [len(x["kind"]) for x in small.chunks] == [1024, 1024]
    assert [len(x["kind"]) for x in pipe.chunks] == [1025, 1025]
    cut = ls.case("Fcut")
    assert cut.max_batch == 2048 and [len(x["kind"]) for x in cut.chunks] == [2048, 2049]
    ch = cut.chunks[1]
    k = cut.meta["cut_at"]
    res = ch["resource"][k]
    same = (ch["resource"][:k] == res) & (ch["ts"][:k] // 500 == ch["ts"][k] // 500)
    assert res < cut.first_filler and same.any(), "the cut falls inside a ruled resource's 500 ms run"
    span = ls.case("Fspan")
    assert [int(x["ts"].max() - x["ts"].min()) for x in span.chunks] == [0xFFFFFFFF, 0x100000000]
    assert span.max_batch is None and all(len(x["kind"]) > 1024 for x in span.chunks)


def test_g_acquire_extremes():
    c = ls.case("G")
    rep = replay("G")
    over = 0
    for res, seam, size, mix in c.meta["specs"]:
        for ch, (dec, _) in zip(c.chunks, rep):
            m = (ch["resource"] == res) & (ch["kind"] == 0)
            a = ch["acquire"][m].astype(np.int64)
            assert (a == 0).any() and (a == ls.BIG).any() and (a == ls.INT32_MAX).any(), seam
            for r in runs_of(ch, res):
                e = r[ch["kind"][r] == 0]
                if mix == "uniform":
                    assert len(np.unique(ch["acquire"][e])) == 1, seam
                over += int(ch["acquire"][e][passed(dec[e])].astype(np.int64).sum() > ls.INT32_MAX)
        n = int((c.chunks[0]["resource"] == res).sum())
        assert n == size and (n >= ls.K_WAVE) == (size >= 300)
    assert over >= 4, "runs whose pass sum goes past INT32_MAX"
