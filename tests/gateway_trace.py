"""TEST INFRASTRUCTURE: the api-gateway adapter's rule handling restated in plain Python over dicts, the expected
side of the gateway tests (independent of sentinel_amd.gateway).

GW = sentinel-adapter/sentinel-api-gateway-adapter-common/src/main/java/com/alibaba/csp/sentinel/adapter/gateway/common
  valid          GatewayRuleManager.isValidRule / isValidParamItem   GW/rule/GatewayRuleManager.java:117-145
  assign         applyGatewayRuleInternal                            GW/rule/GatewayRuleManager.java:179-237
  convert        GatewayRuleConverter                                GW/rule/GatewayRuleConverter.java:49-86
  parse          GatewayParamParser.parseParameterFor                GW/param/GatewayParamParser.java:51-174

A rule is a dict: resource, resource_mode (0), grade (1), count (0), interval_sec (1), control_behavior (0), burst
(0), max_queueing_timeout_ms (500), item (None, or a dict: parse_strategy (0), field_name, pattern, match_strategy
(0); `index` is written by assign).  Where the reference walks a HashSet this walks the list.
"""
import re

NM, D = "$NM", "$D"
KINDS = {0: "client_ip", 1: "host", 2: "header", 3: "url_param", 4: "cookie"}
DEFAULTS = {"resource": None, "resource_mode": 0, "grade": 1, "count": 0.0, "interval_sec": 1, "control_behavior": 0,
            "burst": 0, "max_queueing_timeout_ms": 500, "item": None}
ITEM_DEFAULTS = {"parse_strategy": 0, "field_name": None, "pattern": None, "match_strategy": 0}


def rule(**kw):
    r = dict(DEFAULTS)
    r.update(kw)
    if r["item"] is not None:
        it = dict(ITEM_DEFAULTS)
        it.update(r["item"])
        r["item"] = it
    return r


def _blank(s):
    return s is None or s.strip() == ""


def valid(r):
    if r is None or _blank(r["resource"]) or r["resource_mode"] < 0 or r["grade"] < 0 or r["count"] < 0 \
            or r["burst"] < 0 or r["control_behavior"] < 0:
        return False
    if r["grade"] == 2 and r["max_queueing_timeout_ms"] < 0:  # :122 compares the grade with RATE_LIMITER
        return False
    if r["interval_sec"] <= 0:
        return False
    it = r["item"]
    if it is None:
        return True
    if it["parse_strategy"] < 0:
        return False
    if it["parse_strategy"] in (2, 3, 4) and _blank(it["field_name"]):
        return False
    return it["pattern"] in (None, "") or it["match_strategy"] >= 0


def convert(r, idx):
    """The ParamFlowRule as a tuple that compares like ParamFlowRule.equals, then readable through as_param_rule."""
    hot = ()
    if r["item"] is not None:
        r["item"]["index"] = idx
        if r["item"]["pattern"] is not None:
            hot = ((NM, 10_000_000),)
    return (r["resource"], r["grade"], idx, float(r["count"]), r["control_behavior"], r["max_queueing_timeout_ms"],
            r["burst"], r["interval_sec"], hot)


def as_param_rule(c):
    return {"resource": c[0], "grade": c[1], "param_idx": c[2], "count": c[3], "control_behavior": c[4],
            "max_queueing_time_ms": c[5], "burst_count": c[6], "duration_in_sec": c[7], "hot": dict(c[8])}


def assign(rules):
    """(by_resource, converted): the valid rules per resource, and the converted rules per resource (param rules in
    list order, then the non-param ones), as as_param_rule dicts."""
    by_res, conv, idx, no_param = {}, {}, {}, {}
    for r in rules:
        if not valid(r):
            continue
        name = r["resource"]
        mine = by_res.setdefault(name, [])
        # the reference is handed a Set: an equal rule counts once (items compare by identity)
        if any(q is r or (q["item"] is None and q == r) for q in mine):
            continue
        mine.append(r)
        if r["item"] is None:
            no_param.setdefault(name, []).append(r)
            continue
        i = idx.setdefault(name, 0)
        c = convert(r, i)
        if c not in conv.setdefault(name, []):  # :207-209: always new, paramIdx is part of equals
            conv[name].append(c)
            idx[name] = i + 1
    for name, lst in no_param.items():
        for r in lst:
            c = convert(r, idx.setdefault(name, 0))
            if c not in conv.setdefault(name, []):
                conv[name].append(c)
    return by_res, {k: [as_param_rule(c) for c in v] for k, v in conv.items()}


def field_of(item, request):
    kind = KINDS.get(item["parse_strategy"])
    if kind is None:
        return None
    v = request.get((kind, item["field_name"] if item["parse_strategy"] in (2, 3, 4) else ""))
    if v is None and kind == "host":
        v = request.get(("header", "Host"))
    return v


def match(item, value):
    pat = item["pattern"]
    if pat is None or pat == "" or value is None:
        return value
    ms = item["match_strategy"]
    if ms == 0:
        return value if value == pat else NM
    if ms == 3:
        return value if pat in value else NM
    if ms == 2:
        try:
            rx = re.compile(pat)
        except re.error:
            return value
        return value if rx.fullmatch(value) else NM
    return value  # PREFIX and anything else: the switch's default


def parse(rules_of_resource, mode, request):
    """parseParameterFor with the predicate rule.resourceMode == mode; rules that share an index: the later wins."""
    g = [r for r in rules_of_resource if r["item"] is not None]
    non_param = len(g) < len(rules_of_resource)
    if not g and not non_param:
        return []
    if any(r["resource_mode"] != mode for r in g):
        return []
    arr = [None] * (len(g) + (1 if non_param else 0))
    for r in g:
        arr[r["item"]["index"]] = match(r["item"], field_of(r["item"], request))
    if non_param:
        arr[-1] = D
    return arr


def to_product(r):
    """The dict as sentinel_amd's GatewayFlowRule."""
    from sentinel_amd.gateway import GatewayFlowRule, GatewayParamFlowItem
    it = r["item"]
    return GatewayFlowRule(resource=r["resource"], resource_mode=r["resource_mode"], grade=r["grade"],
                           count=r["count"], interval_sec=r["interval_sec"], control_behavior=r["control_behavior"],
                           burst=r["burst"], max_queueing_timeout_ms=r["max_queueing_timeout_ms"],
                           param_item=None if it is None else GatewayParamFlowItem(
                               parse_strategy=it["parse_strategy"], field_name=it["field_name"],
                               pattern=it["pattern"], match_strategy=it["match_strategy"]))
