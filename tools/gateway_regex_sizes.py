#!/usr/bin/env python3
"""Usage: python3 tools/gateway_regex_sizes.py [pattern ...]

The DFA gateway_regex.compile_dfa makes of each pattern under the default caps: states, byte classes, table bytes
(class map + transitions + accept bits) and the compile time on this host.  Without arguments: the patterns of the
device-REGEX tests (tests/gateway_regex_cases.py, tests/test_gateway_regex_gpu.py) and a few Unicode-heavy ones.
No GPU needed.  profiles/gateway/regex_dfa_sizes.txt is this tool's output."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sentinel_amd import gateway_regex as GR  # noqa: E402

EXTRA = [r"[a-z]+-\d{2,4}", r"[a-z]+-\d{2,4}-gold", r"\w+", r"[\w-]+", r"\w{2,4}", r"\w{1,16}", r"\w{1,32}", r"\W\w",
         r"[\w.+-]+@[\w-]+\.[\w.-]+", r"(a|b)*a(a|b){10}", r"(a|b)*a(a|b){14}"]


def main():
    pats = sys.argv[1:]
    if not pats:
        from tests import gateway_regex_cases as rc
        pats = list(dict.fromkeys(rc.PATTERNS + EXTRA))
    GR.shorthand_ranges("d")  # the probe of re's shorthand sets, once per process
    print(f"caps: {GR.MAX_STATES} states, {GR.MAX_TABLE_BYTES} table bytes")
    print(f"{'pattern':<34} {'states':>6} {'classes':>7} {'bytes':>8} {'ms':>8}")
    worst = (0, "")
    for p in pats:
        t0 = time.perf_counter()
        d = GR.compile_dfa(p)
        ms = (time.perf_counter() - t0) * 1e3
        shown = "".join(c if " " <= c < "\x7f" else c.encode("unicode_escape").decode() for c in p)
        if d is None:
            print(f"{shown:<34} {'-- None: past a cap or outside the subset':<24} {ms:8.1f}")
            continue
        print(f"{shown:<34} {d.n_states:6d} {d.n_classes:7d} {d.table_bytes:8d} {ms:8.1f}")
        worst = max(worst, (d.table_bytes, shown))
    print(f"largest table: {worst[0]} bytes ({worst[1]})")


if __name__ == "__main__":
    main()
