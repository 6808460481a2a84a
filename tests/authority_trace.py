"""TEST INFRASTRUCTURE: expected values for events under AuthorityRules.

Two parts.

  * A string-level restatement of AuthorityRuleManager.loadAuthorityConf (AuthorityRuleManager.java:110-164) and
    AuthorityRuleChecker.passCheck (AuthorityRuleChecker.java:30-66), over names, as the reference runs them:
    indexOf, then split(","), then equals.  Nothing here knows of origin ids, sorted lists or binary searches.
  * AuthorityTrace, a wrapper around an OriginTrace or a ContextTrace by composition: every entry the wrapped trace
    is asked for is first put to the restatement.  AuthoritySlot runs after ClusterBuilderSlot and ahead of
    SystemSlot and every other check, and what StatisticSlot then counts for the AuthorityException is its
    BlockException branch, which is what a kind 2 event is.  So a failing entry is driven as other(2, ...) with the
    entry's inbound flag and no exit is scheduled; a passing one is driven as entry(...).
    finish() returns the usual trace with ed = 6 and ew = 0 at the turned positions, its stream "st" with the
    entries as the caller submits them (kind 0), and "pre", the pre-marked stream, in which the turned events
    carry kind 2: what a caller had to submit while the slot stayed outside the engine.
"""
import numpy as np

WHITE, BLACK = 0, 1
BLOCK_AUTHORITY = 6


# ------------------------------------------------------------------ the restatement
def is_blank(s):
    """StringUtil.isBlank."""
    return s is None or all(ch.isspace() for ch in s)


def java_split_comma(s):
    """String.split(","): trailing empty strings are removed."""
    parts = s.split(",")
    while parts and parts[-1] == "":
        parts.pop()
    return parts


def is_valid_rule(rule):
    """AuthorityRuleManager.isValidRule over (resource, limit_app, strategy)."""
    if rule is None:
        return False
    resource, limit_app, strategy = rule
    return not is_blank(resource) and strategy >= 0 and not is_blank(limit_app)


def load_authority_conf(rules):
    """{resource: (resource, limit_app, strategy)}: the first valid rule of a resource in list order."""
    out = {}
    for rule in rules or []:
        if not is_valid_rule(rule):
            continue
        if rule[0] in out:
            continue  # "Ignoring redundant rule"
        out[rule[0]] = tuple(rule)
    return out


def pass_check(limit_app, strategy, origin):
    """AuthorityRuleChecker.passCheck."""
    if not origin or not limit_app:
        return True
    contain = limit_app.find(origin) > -1
    if contain:
        contain = any(origin == app for app in java_split_comma(limit_app))
    if strategy == BLACK and contain:
        return False
    if strategy == WHITE and not contain:
        return False
    return True


def check(conf, resource, origin):
    """AuthoritySlot.checkBlackWhiteAuthority: a resource without a rule passes."""
    rule = conf.get(resource)
    return True if rule is None else pass_check(rule[1], rule[2], origin)


# ------------------------------------------------------------------ the wrapper
class AuthorityTrace:
    """inner: an OriginTrace or ContextTrace; resources / origins: the names behind its ids (origin id k is
    origins[k - 1], 0 the empty origin); rules: (resource, limit_app, strategy) in list order.  The wrapper takes
    the place of inner.entry, so inner.step and inner.generate route every entry through the restatement."""

    def __init__(self, inner, resources, origins, rules=()):
        self.h = inner
        self.resources, self.origins = list(resources), list(origins)
        self.turned = []
        self.n_pass = 0
        self._inner_entry = inner.entry
        inner.entry = self.entry
        self.load(rules)

    def load(self, rules):
        """AuthorityRuleManager.loadRules: replaces the set, touches no node and no rater."""
        self.conf = load_authority_conf(rules)

    def entry(self, rid, o, ts, acq=1, prio=0, hp=0, pv=0, inb=0, c=None):
        kw = {} if c is None else {"c": c}
        name = self.origins[o - 1] if o else ""
        if check(self.conf, self.resources[rid], name):
            self.n_pass += 1
            return self._inner_entry(rid, o, ts, acq, prio, hp, pv, inb, **kw)
        fl = (1 if prio else 0) | (4 if hp else 0) | (8 if inb else 0)
        self.h.other(2, rid, o, ts, acq, fl & 8, 0, 0, **kw)
        # the event as submitted keeps the entry's flags and argument; the oracle saw the block alone
        self.h.ev[-1] = (2, rid, ts, acq, fl, 0, pv, o)
        self.h.exp[-1] = (BLOCK_AUTHORITY, 0)
        self.turned.append(len(self.h.ev) - 1)
        return BLOCK_AUTHORITY, 0

    def __getattr__(self, name):  # step, generate, other, pop_exits, ...: the wrapped trace's
        return getattr(self.h, name)

    def finish(self, times=None, entry=False):
        tr = self.h.finish(times, entry)
        turned = np.array(self.turned, dtype=np.int64)
        pre = tr["st"]
        assert (pre["kind"][turned] == 2).all() and (tr["ed"][turned] == BLOCK_AUTHORITY).all()
        st = dict(pre, kind=pre["kind"].copy())
        st["kind"][turned] = 0
        twin_ed = tr["ed"].copy()
        twin_ed[turned] = 0
        tr.update(st=st, pre=pre, turned=turned, twin_ed=twin_ed, n_auth_pass=self.n_pass)
        return tr
