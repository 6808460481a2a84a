"""The command center over a live engine, everything through the socket: a SimpleHttpCommandCenter on 127.0.0.1 over
a LocalSentinel that has run a few thousand events with origins.  Expected texts are built from the oracle's
views (tests/origin_trace.py) with the module's formatters, whose own output tests/test_command_center.py pins."""
import json
import socket
from urllib.parse import quote

import numpy as np
import pytest

from tests import local_trace as lt
from tests import origin_trace as ot

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000
ENTRY = 0xFFFFFFFF
N_RES, N_ORG = 6, 3
NAMES = ["svc/orders", "svc/orders/list", "svc/pay", "idle", "svc/stock", "svc/user"]  # "idle" is never entered
RULES_1 = [{"resource": 0, "count": 30}, {"resource": 2, "count": 50, "control_behavior": 2, "max_queueing_time_ms": 20}]
RULES_2 = [{"resource": 0, "count": 3}, {"resource": 4, "count": 2, "grade": 0}, {"resource": 5, "count": 8}]
SYSTEM = [{"qps": 1e9}]  # never blocks: inbound traffic is counted on ENTRY_NODE


def _get(port, path, post=None):
    """(status line, body) of one request; post: a form-encoded body."""
    with socket.create_connection(("127.0.0.1", port), timeout=10) as s:
        if post is None:
            s.sendall(f"GET /{path} HTTP/1.1\r\nHost: localhost\r\n\r\n".encode())
        else:
            s.sendall(f"POST /{path} HTTP/1.1\r\nContent-Type: application/x-www-form-urlencoded\r\n"
                      f"Content-Length: {len(post)}\r\n\r\n".encode() + post)
        raw = b""
        while True:
            b = s.recv(1 << 16)
            if not b:
                break
            raw += b
    head, _, body = raw.partition(b"\r\n\r\n")
    lines = head.decode().split("\r\n")
    assert lines[1] == f"Content-Length: {len(body)}" and lines[2] == "Connection: close"
    return lines[0], body.decode("utf-8")


def _json_rules(rules):
    """The dashboard's FlowRule JSON for the oracle's rule dicts."""
    return json.dumps([{"resource": NAMES[r["resource"]], "count": float(r["count"]), "grade": r.get("grade", 1),
                        "controlBehavior": r.get("control_behavior", 0),
                        "maxQueueingTimeMs": r.get("max_queueing_time_ms", 500), "limitApp": "default"}
                       for r in rules] + [{"resource": "not-registered", "count": 1.0}])


def _view(getters):
    from sentinel_amd.local import NodeView
    return NodeView(*getters)


def test_dashboard_commands_over_the_socket(tmp_path):
    from sentinel_amd.cluster import Engine
    from sentinel_amd.local import LocalSentinel
    st, ed, ew, m1, now1, entered, views, entry_view, origin_views = _trace()

    # ---- the engine's side
    eng = Engine(max_batch=1 << 14)
    s = LocalSentinel(eng, NAMES, [f"caller-{o}" for o in range(1, N_ORG + 1)])
    _engine_side(tmp_path, eng, s, st, ed, ew, m1, now1, entered, views, entry_view, origin_views)


def _trace():
    """The oracle's side: chunk 1 under RULES_1, the views at now1, chunk 2 under RULES_2."""
    h = ot.OriginTrace(N_RES, N_ORG, RULES_1, system=SYSTEM)
    weights = [4, 2, 3, 0, 2, 2]
    h.generate(1500, 5, T0, weights, [1, 3, 2, 2], gap_mean=1.2, rt_max=39, inbound=True, err_pct=0.1)
    h.flush()
    m1 = len(h.ev)
    now1 = int(max(e[2] for e in h.ev)) + 150
    entered = [r for r in range(N_RES) if r != 3]
    views = {r: _view(h.node(r, now1)) for r in entered}
    entry_view = _view(h.main.node(ENTRY, now1))
    origin_views = [(f"caller-{o}", _view(h.origin_node(0, o, now1))) for o in range(1, N_ORG + 1)
                    if (0, o) in h.created]
    assert len(origin_views) == N_ORG and views[0].total_block > 0 and entry_view.total_pass > 300
    h.load(RULES_2)
    h.generate(1200, 6, now1 + 20, weights, [1, 3, 2, 2], gap_mean=1.2, rt_max=39, inbound=True, err_pct=0.1)
    h.flush()
    st, ed, ew = h.stream()
    h.close()
    assert len(ed) > 4000
    d2 = ed[m1:][st["kind"][m1:] == 0]
    assert (d2 == 1).sum() > 200 and (d2 == 0).sum() > 200  # the new rules block and pass
    return st, ed, ew, m1, now1, entered, views, entry_view, origin_views


def _engine_side(tmp_path, eng, s, st, ed, ew, m1, now1, entered, views, entry_view, origin_views):
    from sentinel_amd import command_center as cc
    from sentinel_amd import metric_log as ml
    from sentinel_amd.local import (DegradeRuleManager, FlowRuleManager, ParamFlowRuleManager, SystemRule,
                                    SystemRuleManager)
    managers = {"flow": FlowRuleManager(s), "degrade": DegradeRuleManager(s), "system": SystemRuleManager(s),
                "param": ParamFlowRuleManager(s)}
    managers["system"].load_rules([SystemRule(qps=1e9)])
    clock = {"now": now1}
    writer = ml.MetricWriter(str(tmp_path), app_name="gpu-app", pid=7, now_ms=T0 - 1000)
    searcher = ml.MetricSearcher(str(tmp_path), ml.form_metric_file_name("gpu-app", 7))
    center = cc.CommandCenter(s, managers, searcher, clock=lambda: clock["now"])
    server = cc.SimpleHttpCommandCenter(center, port=18740)
    port = server.start()
    try:
        # the first rules arrive as the dashboard pushes them
        assert _get(port, "setRules", post=("type=flow&data=" + quote(quote(_json_rules(RULES_1)))).encode()) == \
            ("HTTP/1.0 200 OK", "success")
        first = lt.slice_stream(st, 0, m1)
        d, w = s.submit(first["kind"], first["resource"], first["ts"], first["acquire"], first["flags"], first["rt"],
                        first["param"], origin=first["origin"])
        assert (d == ed[:m1]).all() and (w == ew[:m1]).all()

        # ---- the read commands at now1
        status, body = _get(port, "clusterNode")
        assert status == "HTTP/1.0 200 OK"
        assert body == cc.to_json([cc.node_vo(NAMES[r], views[r], now1) for r in entered])
        status, body = _get(port, "clusterNode?type=notZero")
        assert body == cc.to_json([cc.node_vo(NAMES[r], views[r], now1) for r in entered
                                   if views[r].total_pass + views[r].total_block > 0])
        assert _get(port, "cnode?id=orders")[1] == cc.format_cnode([(NAMES[r], views[r]) for r in (0, 1)])
        assert _get(port, "cnode?id=svc%2F")[1] == cc.format_cnode([(NAMES[r], views[r]) for r in entered])
        assert _get(port, "cnode", post=b"id=idle")[1] == cc.format_cnode([])  # registered, never entered
        assert _get(port, "origin?id=svc/orders")[1] == cc.format_origin(NAMES[0], origin_views)
        assert _get(port, "origin?id=nothing-like-it")[1] == "Not find cNode with id nothing-like-it"
        assert _get(port, "systemStatus")[1] == cc.format_system_status(entry_view)

        # ---- setRules changes the next chunk's decisions
        status, body = _get(port, "setRules", post=("type=flow&data=" + quote(quote(_json_rules(RULES_2)))).encode())
        assert (status, body) == ("HTTP/1.0 200 OK", "success")
        listed = json.loads(_get(port, "getRules?type=flow")[1])
        assert [r["resource"] for r in listed] == [NAMES[r["resource"]] for r in RULES_2] + ["not-registered"]
        second = lt.slice_stream(st, m1, len(ed))
        d, w = s.submit(second["kind"], second["resource"], second["ts"], second["acquire"], second["flags"],
                        second["rt"], second["param"], origin=second["origin"])
        bad = np.nonzero((d != ed[m1:]) | (w != ew[m1:]))[0]
        assert not len(bad), (len(bad), int(bad[0]) if len(bad) else None)

        # ---- metric: the lines MetricTimerListener wrote, then the load and cpu rows
        wrote = []
        real_write = writer.write
        writer.write = lambda t, nodes: (wrote.extend(nodes), real_write(t, nodes))[1]
        now2 = int(st["ts"].max()) + 1500
        clock["now"] = now2
        ml.MetricTimerListener(s, writer).run(now2)
        writer.close()
        assert len(wrote) > 10
        managers["system"].set_system_status(1.5, 0.25)
        sec = now2 // 1000 * 1000
        tail = f"{sec}|__system_load__|15000|0|0|0|0|0|0|0\n{sec}|__cpu_usage__|2500|0|0|0|0|0|0|0\n"
        status, body = _get(port, f"metric?startTime={T0}&endTime={now2}")
        assert status == "HTTP/1.0 200 OK"
        assert body == "".join(n.to_thin_string() + "\n" for n in wrote) + tail
        one = [n for n in wrote if n.resource == NAMES[2]]
        assert _get(port, f"metric?startTime={T0}&endTime={now2}&identity=svc/pay")[1] == \
            "".join(n.to_thin_string() + "\n" for n in one) and one
        assert _get(port, f"metric?startTime={T0}&maxLines=3")[1].endswith(tail)
        assert _get(port, "metric")[1] == ""

        # ---- commands nobody registered, and none
        assert _get(port, "jsonTree") == ("HTTP/1.0 400 Bad Request", "Unknown command `jsonTree`")
        assert _get(port, "") == ("HTTP/1.0 400 Bad Request", "Invalid command")
        assert _get(port, "getRules?type=nope") == ("HTTP/1.0 400 Bad Request", "invalid type")
    finally:
        server.stop()
        eng.close()
