"""TEST INFRASTRUCTURE: expected circuit breaker notifications.

The oracle has no notion of an observer (it exposes orc_flow_cb_state only), so this restates, from the Java,

  * AbstractCircuitBreaker (AbstractCircuitBreaker.java:62-164): tryPass, fromCloseToOpen, fromOpenToHalfOpen with
    its whenTerminate hook, fromHalfOpenToOpen, fromHalfOpenToClose, and the notifyObservers call of each;
  * ExceptionCircuitBreaker.onRequestComplete (ExceptionCircuitBreaker.java:70-128) and
    ResponseTimeCircuitBreaker.onRequestComplete (ResponseTimeCircuitBreaker.java:65-128), each over its
    LeapArray(1, statIntervalMs) -- one bucket: currentWindow(t) resets it when t's window is newer, and hands out a
    detached bucket that nobody reads when it is older (LeapArray.java:118-190); values(t) skips a bucket with
    t - windowStart > intervalInMs (LeapArray.java:193-195, 320-340);
  * DegradeSlot.entry / exit over a resource's breakers in DegradeRuleManager list order (DegradeSlot.java:52-88);
  * the revoke of an entry a later slot blocked: the probe's whenTerminate hook with a block error set.

Nothing here knows of kernels, chunks or scans: one event at a time, in arrival order.  A notification is the dict
the engine's record must equal field by field: seq, sub, ts, resource, breaker, prev, next, value (None for null).
Python's bad / total on ints is the IEEE double division the Java performs, so values compare for equality.
"""
CLOSED, OPEN, HALF_OPEN = 0, 1, 2
GRADE_RT, GRADE_EXCEPTION_RATIO, GRADE_EXCEPTION_COUNT = 0, 1, 2


def java_round(x):
    """Math.round(double): floor(x + 0.5)."""
    import math
    return int(math.floor(x + 0.5))


def is_valid_rule(r):
    """DegradeRuleManager.isValidRule (DegradeRuleManager.java:210-240) over a rule dict."""
    ok = r["count"] >= 0 and r.get("time_window", 1) > 0 and r.get("min_request_amount", 5) > 0 and \
        r.get("stat_interval_ms", 1000) > 0
    if not ok:
        return False
    g = r.get("grade", 0)
    if g == GRADE_RT:
        return 0 <= r.get("slow_ratio_threshold", 1.0) <= 1
    if g == GRADE_EXCEPTION_RATIO:
        return r["count"] <= 1
    return g == GRADE_EXCEPTION_COUNT


class Breaker:
    """One AbstractCircuitBreaker with its subclass's counters.  rule: {grade, count, time_window,
    min_request_amount, slow_ratio_threshold, stat_interval_ms} with the oracle harness's defaults."""

    def __init__(self, rule, notify):
        self.rule = rule
        self.grade = rule.get("grade", 0)
        self.threshold = rule["count"]
        self.recovery_ms = rule.get("time_window", 1) * 1000
        self.min_request_amount = rule.get("min_request_amount", 5)
        self.max_slow_ratio = rule.get("slow_ratio_threshold", 1.0)
        self.interval = rule.get("stat_interval_ms", 1000)
        self.max_allowed_rt = java_round(rule["count"])
        self.state = CLOSED
        self.next_retry = 0
        self.win_start = None  # the one bucket of LeapArray(1, interval): its start, bad and total counts
        self.bad = 0
        self.total = 0
        self.probe_t = None  # time of the entry whose whenTerminate hook is pending
        self._notify = notify

    # -- LeapArray(1, interval)
    def _current_window(self, t):
        """currentWindow(t): True when the array's own bucket is handed out, False for a detached one."""
        ws = t - t % self.interval
        if self.win_start is None or ws > self.win_start:
            self.win_start, self.bad, self.total = ws, 0, 0
            return True
        return ws == self.win_start

    def _values(self, t):
        if self.win_start is None or t - self.win_start > self.interval:
            return 0, 0
        return self.bad, self.total

    # -- AbstractCircuitBreaker
    def try_pass(self, t):
        """tryPass; a passing probe registers its hook (probe_t)."""
        if self.state == CLOSED:
            return True
        if self.state == OPEN:
            if t >= self.next_retry:  # retryTimeoutArrived() && fromOpenToHalfOpen(context)
                self.state = HALF_OPEN
                self._notify(self, OPEN, HALF_OPEN, None)
                self.probe_t = t
                return True
            return False
        return False

    def when_terminate_blocked(self):
        """The probe's whenTerminate hook with entry.getBlockError() != null.  The reference notifies whether or
        not its compareAndSet succeeded; the engine reports real moves only, and here the state is HALF_OPEN
        whenever the hook runs (nothing runs between the probe and its block inside one entry, and a revoke
        names its entry by time)."""
        if self.state == HALF_OPEN:
            self.state = OPEN
            self._notify(self, HALF_OPEN, OPEN, 1.0)

    def _to_open(self, t, value):
        """transformToOpen."""
        if self.state == CLOSED:
            self.state = OPEN
            self.next_retry = t + self.recovery_ms
            self._notify(self, CLOSED, OPEN, value)
        elif self.state == HALF_OPEN:
            self._half_open_to_open(t, value)

    def _half_open_to_open(self, t, value):
        self.state = OPEN
        self.next_retry = t + self.recovery_ms
        self._notify(self, HALF_OPEN, OPEN, value)

    def _half_open_to_close(self, t):
        self.state = CLOSED
        if self._current_window(t):  # resetStat(): stat.currentWindow().value().reset()
            self.bad, self.total = 0, 0
        self._notify(self, HALF_OPEN, CLOSED, None)

    def on_request_complete(self, t, rt, error):
        bad = rt > self.max_allowed_rt if self.grade == GRADE_RT else bool(error)
        if self._current_window(t):
            if bad:
                self.bad += 1
            self.total += 1
        # handleStateChangeWhenThresholdExceeded
        if self.state == OPEN:
            return
        if self.state == HALF_OPEN:
            if bad:
                self._half_open_to_open(t, 1.0)
            else:
                self._half_open_to_close(t)
            return
        badc, total = self._values(t)
        if total < self.min_request_amount:
            return
        if self.grade == GRADE_RT:
            ratio = badc * 1.0 / total
            if ratio > self.max_slow_ratio or (ratio == self.max_slow_ratio and self.max_slow_ratio == 1.0):
                self._to_open(t, ratio)
            return
        cur = float(badc)
        if self.grade == GRADE_EXCEPTION_RATIO:
            cur = badc * 1.0 / total
        if cur > self.threshold:
            self._to_open(t, cur)


class BreakerTrace:
    """The breakers of every resource and the notifications of a sequence of events.

    rules: dicts as the oracle harness takes them ({resource, grade, count, ...}), in DegradeRuleManager list order;
    invalid ones are dropped as the manager drops them.  Every event takes its seq (its position in the stream
    since the log was enabled) and returns what the slot answers."""

    def __init__(self, rules, epoch=1):
        self.events = []
        self.epoch = epoch
        self._seq = self._ts = self._res = None
        self._sub = 0
        self.breakers = {}
        for r in rules:
            if is_valid_rule(r):
                self.breakers.setdefault(r.get("resource", 0), []).append(Breaker(r, self._note))

    def _note(self, breaker, prev, nxt, value):
        k = self.breakers[self._res].index(breaker)
        self.events.append({"seq": self._seq, "sub": self._sub, "ts": self._ts, "resource": self._res, "breaker": k,
                            "epoch": self.epoch, "prev": prev, "next": nxt, "value": value})
        self._sub += 1

    def _begin(self, seq, r, t):
        self._seq, self._res, self._ts, self._sub = seq, r, t, 0

    def entry(self, seq, r, t):
        """DegradeSlot.entry: -1 when every breaker passes, else the index of the one that blocks; the hooks of
        the probes before it run after the block."""
        self._begin(seq, r, t)
        bs = self.breakers.get(r, [])
        probes = []
        for k, b in enumerate(bs):
            was_open = b.state == OPEN
            if not b.try_pass(t):
                for p in probes:
                    p.when_terminate_blocked()
                return k
            if was_open:
                probes.append(b)
        return -1

    def exit(self, seq, r, t, rt, error):
        """DegradeSlot.exit of a passed entry: onRequestComplete of every breaker in order."""
        self._begin(seq, r, t)
        for b in self.breakers.get(r, []):
            b.on_request_complete(t, rt, error)

    def revoke(self, seq, r, t):
        """An entry the slot passed at time t was blocked further down the chain: the hooks of its probes."""
        self._begin(seq, r, t)
        for b in self.breakers.get(r, []):
            if b.state == HALF_OPEN and b.probe_t == t:
                b.when_terminate_blocked()

    def state(self, r, k):
        return self.breakers[r][k].state

    def states(self, r):
        return [b.state for b in self.breakers.get(r, [])]


KIND_ENTRY, KIND_EXIT, KIND_BLOCKED, KIND_REVOKE = 0, 1, 2, 3
EV_ERROR = 2
BLOCK_DEGRADE = 3


def replay_stream(trace, s, seq0=0, decisions=None, reach=None):
    """Drives a BreakerTrace with a stream (arrays kind, resource, ts, flags, rt).  An exit, like the engine's, is
    the exit of an entry that passed.  reach (optional): every event's decision by the oracle -- an entry that an
    earlier slot answered (anything but PASS or a degrade block) never reaches DegradeSlot, and what the
    restatement answers for the others must be what the oracle did.  decisions (optional list) receives 0 / 3 per
    entry and None for the rest.  Returns the trace's events."""
    for i in range(len(s["kind"])):
        k, r, t = int(s["kind"][i]), int(s["resource"][i]), int(s["ts"][i])
        d = None
        if k == KIND_ENTRY and reach is not None and int(reach[i]) not in (0, BLOCK_DEGRADE):
            pass
        elif k == KIND_ENTRY:
            d = 0 if trace.entry(seq0 + i, r, t) < 0 else BLOCK_DEGRADE
            assert reach is None or int(reach[i]) == d, (i, int(reach[i]), d)
        elif k == KIND_EXIT:
            trace.exit(seq0 + i, r, t, int(s["rt"][i]), bool(int(s["flags"][i]) & EV_ERROR))
        elif k == KIND_REVOKE:
            trace.revoke(seq0 + i, r, t)
        if decisions is not None:
            decisions.append(d)
    return trace.events


def scenario_events(sc, base):
    """A transcribed CircuitBreakingIntegrationTest scenario (the oracle harness's ops: flow_load_degrade,
    flow_entry_sleep, flow_entry_error, sleep, set_time) through the restatement.  Returns (events, results,
    states): the notifications, each entry op's pass / block, and the breaker states after each op."""
    now = base
    tr = None
    seq = 0
    results, states = [], []
    for op in sc["ops"]:
        k = op["op"]
        if k == "set_time":
            now = base + op["t"]
        elif k == "sleep":
            now += op["ms"]
        elif k == "flow_load_degrade":
            tr = BreakerTrace(op["rules"])
        elif k in ("flow_entry_sleep", "flow_entry_error"):
            passed = tr.entry(seq, op["resource"], now) < 0
            seq += 1
            if passed:
                t_in = now
                now += op["ms"]
                tr.exit(seq, op["resource"], now, now - t_in, k == "flow_entry_error")
                seq += 1
            results.append(passed)
        states.append(tr.states(0) if tr else [])
    return tr.events, results, states


# ------------------------------------------------------------------ seeded traces
def random_rules(rng, n_res, max_per_res=3):
    """1 to max_per_res breakers per resource, grades drawn from all three, small thresholds so that traces of a
    few hundred events trip, probe, close and reopen them."""
    rules = []
    for r in range(n_res):
        for _ in range(int(rng.integers(1, max_per_res + 1))):
            g = int(rng.integers(0, 3))
            rule = {"resource": r, "grade": g, "time_window": int(rng.integers(1, 3)),
                    "min_request_amount": int(rng.integers(1, 5)), "stat_interval_ms": int(rng.choice([200, 1000])),
                    "slow_ratio_threshold": float(rng.choice([0.5, 1.0]))}
            rule["count"] = [20, float(rng.choice([0.25, 0.5])), int(rng.integers(1, 4))][g]
            rules.append(rule)
    return rules


def random_stream(rng, rules, n, n_res, t0=1_700_000_000_000, revoke=True):
    """n events over n_res breaker-only resources, written while a private restatement runs so that the stream can
    aim: entries at exactly an OPEN breaker's nextRetry and at nextRetry - 1, timestamps that step back across a
    stat window, exits (slow, failed or good) of entries that passed, revokes of a probe that passed.  Returns the
    stream as numpy arrays (kind, resource, ts, acquire, flags, rt, param)."""
    import numpy as np
    tr = BreakerTrace(rules)
    now = t0
    live = {r: [] for r in range(n_res)}  # passed entries not yet exited: their times
    ev = []
    for i in range(n):
        r = int(rng.integers(0, n_res))
        bs = tr.breakers.get(r, [])
        u = rng.random()
        opened = [b for b in bs if b.state == OPEN]
        if u < 0.25 and opened:  # aim at a retry time
            b = opened[int(rng.integers(0, len(opened)))]
            now = max(t0, b.next_retry - int(rng.integers(0, 2)))
        elif u < 0.29:  # back across a stat window
            now = max(t0, now - int(rng.choice([250, 1100])))
        elif u < 0.36:
            now += int(rng.integers(100, 700))
        else:
            now += int(rng.integers(0, 12))
        v = rng.random()
        if live[r] and v < 0.45:
            t_in = live[r].pop(int(rng.integers(0, len(live[r]))))
            rt = int(rng.choice([1, 20, 21, 60, 90]))
            err = rng.random() < 0.55
            tr.exit(i, r, now, rt, err)
            ev.append((KIND_EXIT, r, now, EV_ERROR if err else 0, rt))
        elif revoke and live[r] and v < 0.52:
            t_in = live[r].pop()  # the latest passed entry: a probe's revoke names it by its time
            tr.revoke(i, r, t_in)
            ev.append((KIND_REVOKE, r, t_in, 0, 0))
        else:
            if tr.entry(i, r, now) < 0:
                live[r].append(now)
            ev.append((KIND_ENTRY, r, now, 0, 0))
    a = np.array(ev, dtype=np.int64).reshape(-1, 5)
    return {"kind": a[:, 0].astype(np.uint8), "resource": a[:, 1].astype(np.uint32), "ts": a[:, 2].copy(),
            "acquire": np.ones(len(a), np.int32), "flags": a[:, 3].astype(np.uint8), "rt": a[:, 4].copy(),
            "param": np.zeros(len(a), np.uint64)}
