"""Direct cases for radix_sort.hip, run as a child process:  python -m tests.sort_cases <which>

The sort reads SGA_RADIX_MODE and SGA_RADIX_BITS once per process, so every configuration gets a
fresh child (tests/test_radix_sort_gpu.py, tests/test_radix_plan_host.py).  <which> is

  full   every case below plus the large ones (default configuration only)
  std    pairs, u64, hist0_ready, tiled and scan cases
  u64    the contiguous u64 sort only (the only sort SGA_RADIX_MODE=0 may run here)
  plan   host only: the pass plan and scratch budget of every sort, no device call

Output: {"announce": N}, one JSON line per case, then {"summary": ...}.  The runner stops at the
first HIP error; the summary then counts fewer cases than announced.

The reference is numpy's stable argsort of the key field; every comparison is exact equality of whole
elements (bits outside the field are random and must ride along unchanged).
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sentinel_amd", "libsga_sorttest.so")

TILE = 4096
SEG = 1024
MAX_PASSES = 3
FILL8 = 0xCD
POISON = np.uint64(0xDEADBEEFDEADBEEF)

SIZES = [1, 63, 64, 65, 1023, 1025, 4095, 4096, 4097, 3 * 4096 + 1, 64 * 4096 + 17]
DIST_SIZES = [65, 4097, 64 * 4096 + 17]
DISTS = ["uniform", "equal", "two", "ascending", "descending", "zipf", "top"]
SHIFTS = [0, 24, 32, 40]
ROW_SCAN_N = 2049 * 4096 + 3          # second round of k_row_scan (above 2048 tiles)
SCAN_LARGE = [4096 * 4096, 4096 * 4096 + 5]  # the latter: second round of k_scan_partials


def digit_cap():
    e = os.environ.get("SGA_RADIX_BITS")
    b = int(e) if e else 8
    return min(max(b, 8), 11)


def radix_mode():
    e = os.environ.get("SGA_RADIX_MODE")
    return int(e) if e else 1


def bit_counts():
    w = digit_cap()
    """(bit counts to sort, bit counts past the last: 25 or 33, then -- should that one still fit
    three passes, as 33 does with 11-bit digits -- the first that does not)"""
    w = digit_cap()
    if "SGA_RADIX_BITS" not in os.environ or w == 8:
        return [1, 7, 8, 9, 12, 16, 17, 21, 24], [25]
    return [9, 10, 11, 20, 22], ([33] if 33 > MAX_PASSES * w else [33, MAX_PASSES * w + 1])


def load():
    L = ctypes.CDLL(LIB)
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    pi, pu = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint32)
    L.sgat_last_error.restype = ctypes.c_char_p
    L.sgat_sort_pairs.argtypes = [vp, vp, u64, i32, vp, vp, vp, vp, pi, pu]
    L.sgat_sort_u64.argtypes = [vp, u64, i32, i32, vp, vp, vp, pi, pu, pu]
    L.sgat_sort_u64_tiled.argtypes = [vp, vp, u32, u64, i32, i32, vp, vp, vp, vp, pi, pu]
    L.sgat_exclusive_scan.argtypes = [vp, u64, vp, pu]
    L.sgat_sort_plan.argtypes = [i32, i32, u64, vp]
    L.sgat_sort_plan.restype = None
    return L


def ptr(a):
    return None if a is None else a.ctypes.data


class HipFailure(Exception):
    pass


def plan(L, kind, bits, n):
    out = np.zeros(8, np.int64)
    L.sgat_sort_plan(kind, bits, n, ptr(out))
    return [int(x) for x in out]


# ---- inputs ---------------------------------------------------------------------------------------
def make_field(rng, dist, n, bits, digit):
    """n values below 2**bits (uint64)."""
    hi = 1 << bits
    if dist == "uniform":
        f = rng.integers(0, hi, n, dtype=np.uint64)
    elif dist == "equal":  # one digit fills whole waves and tiles: every lane of a ballot matches
        f = np.full(n, int(rng.integers(0, hi)), np.uint64)
    elif dist == "two":
        a, b = int(rng.integers(0, hi)), int(rng.integers(0, hi))
        f = np.where(np.arange(n) % 2 == 0, a, b).astype(np.uint64)
    elif dist == "ascending":
        f = np.sort(rng.integers(0, hi, n, dtype=np.uint64))
    elif dist == "descending":
        f = np.sort(rng.integers(0, hi, n, dtype=np.uint64))[::-1].copy()
    elif dist == "zipf":
        f = (rng.zipf(1.3, n).astype(np.uint64) - np.uint64(1)) % np.uint64(hi)
    elif dist == "top":  # keys that differ only in the top digit of the field
        low = int(rng.integers(0, 1 << (bits - digit))) if bits > digit else 0
        f = (rng.integers(0, 1 << digit, n, dtype=np.uint64) << np.uint64(bits - digit)) | np.uint64(low)
    else:
        raise ValueError(dist)
    return f


def stable_perm(field, bits):
    dt = np.uint8 if bits <= 8 else (np.uint16 if bits <= 16 else (np.uint32 if bits <= 32 else np.uint64))
    return np.argsort(field.astype(dt), kind="stable")


def embed(rng, field, shift, bits):
    """u64 elements: the field at [shift, shift + bits), every other bit random."""
    n = len(field)
    m = np.uint64(((1 << bits) - 1) << shift)
    rnd = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    return (rnd & ~m) | (field << np.uint64(shift))


def first_diff(got, want):
    if got.shape != want.shape:
        return "shape %s != %s" % (got.shape, want.shape)
    if len(got) == 0:
        return ""
    bad = np.nonzero((got.reshape(len(got), -1) != want.reshape(len(want), -1)).any(axis=1))[0]
    return "" if len(bad) == 0 else "%d of %d elements differ, first at %d" % (len(bad), len(got), bad[0])


def untouched(buf):
    return bool((buf.view(np.uint8) == FILL8).all())


def check_rc(L, rc, name):
    if rc != 0:
        raise HipFailure("%s: hook returned %d: %s" % (name, rc, (L.sgat_last_error() or b"").decode()))


# ---- one case each ----------------------------------------------------------------------------------
def run_pairs(L, rng, n, bits, dist):
    digit = plan(L, 0, max(bits, 1), max(n, 1))[1]
    field = make_field(rng, dist, n, bits, digit) if bits > 0 else np.zeros(n, np.uint64)
    keys = ((rng.integers(0, 1 << 32, n, dtype=np.uint64) << np.uint64(bits)) | field).astype(np.uint32) \
        if bits < 32 else field.astype(np.uint32)
    pay = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    pay[:, 0] = np.arange(n, dtype=np.uint32)
    k = [np.empty(n, np.uint32), np.empty(n, np.uint32)]
    p = [np.empty((n, 4), np.uint32), np.empty((n, 4), np.uint32)]
    npass, guard = ctypes.c_int(-99), ctypes.c_uint32(0)
    rc = L.sgat_sort_pairs(ptr(keys), ptr(pay), n, bits, ptr(k[0]), ptr(k[1]), ptr(p[0]), ptr(p[1]),
                           ctypes.byref(npass), ctypes.byref(guard))
    check_rc(L, rc, "pairs")
    np_ = npass.value
    want_np = 0 if (n == 0 or bits <= 0) else -(-bits // digit)
    if want_np > MAX_PASSES:
        want_np = -1
    msg = "" if np_ == want_np else "pass count %d, expected %d" % (np_, want_np)
    if np_ <= 0:  # nothing sorted: nothing written
        msg = msg or first_diff(k[0], keys) or first_diff(p[0], pay)
        if not (untouched(k[1]) and untouched(p[1])):
            msg = msg or "alt buffers written"
    else:
        perm = stable_perm(keys.astype(np.uint64) & np.uint64((1 << bits) - 1), bits)
        r = np_ & 1  # radix_sort.hpp: in (keys, pay) when even, in the alt buffers when odd
        msg = msg or first_diff(k[r], keys[perm]) or first_diff(p[r], pay[perm])
    return msg, guard.value, np_


def hist0_of(el, shift, digit, nt):
    """digit-major per-tile histogram of the first digit: hist[d * ntiles + tile]."""
    R = 1 << digit
    d0 = ((el >> np.uint64(shift)) & np.uint64(R - 1)).astype(np.int64)
    tile = np.arange(len(el), dtype=np.int64) // TILE
    h = np.bincount(tile * R + d0, minlength=nt * R).reshape(nt, R)
    return np.ascontiguousarray(h.T).astype(np.uint32).reshape(-1)


def run_u64(L, rng, n, bits, shift, dist, with_hist0=False):
    digit = plan(L, 1, max(bits, 1), max(n, 1))[1]
    field = make_field(rng, dist, n, bits, digit) if bits > 0 else np.zeros(n, np.uint64)
    el = embed(rng, field, shift, bits) if bits > 0 else rng.integers(0, 1 << 64, n, dtype=np.uint64)
    hist0 = hist0_of(el, shift, digit, -(-n // TILE)) if with_hist0 else None
    out = [np.empty(n, np.uint64), np.empty(n, np.uint64)]
    npass, guard, err = ctypes.c_int(-99), ctypes.c_uint32(0), ctypes.c_uint32(0)
    rc = L.sgat_sort_u64(ptr(el), n, shift, bits, ptr(hist0), ptr(out[0]), ptr(out[1]), ctypes.byref(npass),
                         ctypes.byref(err), ctypes.byref(guard))
    check_rc(L, rc, "u64")
    np_ = npass.value
    want_np = 0 if (n == 0 or bits <= 0) else -(-bits // digit)
    if want_np > MAX_PASSES:
        want_np = -1
    msg = "" if np_ == want_np else "pass count %d, expected %d" % (np_, want_np)
    if err.value != 0:
        msg = msg or "look-back error word %d" % err.value
    if np_ <= 0:
        msg = msg or first_diff(out[0], el)
        if not untouched(out[1]):
            msg = msg or "alt buffer written"
    else:
        perm = stable_perm(field, bits)
        msg = msg or first_diff(out[np_ & 1], el[perm])  # in `a` when even, in `alt` when odd
    return msg, guard.value, np_


def tile_fills(rng, scenario):
    """(fills[tiles, 4], n_host)"""
    T = 5
    if scenario == "full":
        f = np.full((T, 4), SEG)
    elif scenario == "quarter":
        f = np.full((T, 4), SEG // 4)
    elif scenario == "random":
        f = rng.integers(0, SEG + 1, (T, 4))
    elif scenario == "random65":
        T = 65
        f = rng.integers(0, SEG + 1, (T, 4))
    elif scenario == "some_empty":
        f = rng.integers(0, SEG + 1, (T, 4)) * (rng.random((T, 4)) < 0.6)
    elif scenario == "tile_empty":
        f = rng.integers(0, SEG + 1, (T, 4))
        f[2, :] = 0
    elif scenario == "trailing":  # n_host = 5 * 4096 above dn = 2 * 4096 + 17
        f = np.zeros((T, 4), np.int64)
        f[0:2, :] = SEG
        f[2, 0] = 17
    elif scenario == "ragged_bound":  # the host bound is no multiple of the tile
        T = 4
        f = rng.integers(0, 3 * SEG // 4 + 1, (T, 4))
        return f.astype(np.uint32), 3 * TILE + 1
    else:
        raise ValueError(scenario)
    return f.astype(np.uint32), T * TILE


def run_tiled(L, rng, scenario, bits, shift, with_hist0):
    fills, n_host = tile_fills(rng, scenario)
    T = len(fills)
    assert T == -(-n_host // TILE)
    dn = int(fills.sum())
    assert 0 < dn <= n_host
    digit = plan(L, 2, bits, n_host)[1]
    field = make_field(rng, "uniform", dn, bits, digit)
    seq = embed(rng, field, shift, bits)  # logical arrival sequence
    outside = shift + bits if shift + bits < 64 else 0  # a bit outside the field
    seq[seq == POISON] ^= np.uint64(1 << outside)
    src = np.full(T * TILE, POISON, np.uint64)  # unused slots hold the poison value
    R = 1 << digit
    hist0 = np.zeros((T, R), np.int64)
    at = 0
    for t in range(T):
        for w in range(4):
            c = int(fills[t, w])
            src[t * TILE + w * SEG: t * TILE + w * SEG + c] = seq[at: at + c]
            d0 = ((seq[at: at + c] >> np.uint64(shift)) & np.uint64(R - 1)).astype(np.int64)
            hist0[t] += np.bincount(d0, minlength=R)
            at += c
    h0 = np.ascontiguousarray(hist0.T).astype(np.uint32).reshape(-1) if with_hist0 else None
    tile_n0 = np.ascontiguousarray(fills.reshape(-1))
    out = [np.empty(n_host, np.uint64), np.empty(n_host, np.uint64)]
    src_after = np.empty_like(src)
    npass, guard = ctypes.c_int(-99), ctypes.c_uint32(0)
    rc = L.sgat_sort_u64_tiled(ptr(src), ptr(tile_n0), dn, n_host, shift, bits, ptr(h0), ptr(out[0]), ptr(out[1]),
                               ptr(src_after), ctypes.byref(npass), ctypes.byref(guard))
    check_rc(L, rc, "tiled")
    np_ = npass.value
    want_np = -(-bits // digit)
    msg = "" if np_ == want_np else "pass count %d, expected %d" % (np_, want_np)
    if np_ > 0:
        perm = stable_perm(field, bits)
        res = out[0] if (np_ & 1) else out[1]  # pass p writes `a` when even: in `a` when the count is odd
        msg = msg or first_diff(res[:dn], seq[perm])
        if not (untouched(out[0][dn:]) and untouched(out[1][dn:])):
            msg = msg or "output written past the device-side count"
        if (res[:dn] == POISON).any():
            msg = msg or "an unused slot's value reached the output"
    if not msg and first_diff(src_after, src):
        msg = "src changed: " + first_diff(src_after, src)
    return msg, guard.value, np_


def run_scan(L, rng, n, kind):
    v = np.ones(n, np.uint32) if kind == "ones" else rng.integers(0, 256, n, dtype=np.uint64).astype(np.uint32)
    out = np.empty(n, np.uint32)
    guard = ctypes.c_uint32(0)
    rc = L.sgat_exclusive_scan(ptr(v), n, ptr(out), ctypes.byref(guard))
    check_rc(L, rc, "scan")
    c = np.cumsum(v, dtype=np.uint64)
    assert n == 0 or int(c[-1]) < 1 << 32
    want = np.zeros(n, np.uint32)
    want[1:] = c[:-1].astype(np.uint32)
    return first_diff(out, want), guard.value, 0


# ---- the case list --------------------------------------------------------------------------------
def u64_cases(add):
    bits_list, past = bit_counts()
    i = 0
    for n in SIZES:
        for bits in bits_list:
            shift = SHIFTS[i % len(SHIFTS)]
            i += 1
            add("u64 n=%d bits=%d shift=%d uniform" % (n, bits, shift),
                lambda L, r, n=n, b=bits, s=shift: run_u64(L, r, n, b, s, "uniform"))
    for bits in bits_list:  # the field ends at bit 64
        add("u64 n=4097 bits=%d shift=%d top-of-word" % (bits, 64 - bits),
            lambda L, r, b=bits: run_u64(L, r, 4097, b, 64 - b, "uniform"))
    for j, dist in enumerate(DISTS[1:]):
        for n in DIST_SIZES:
            bits = bits_list[(j + 3) % len(bits_list)] if dist != "top" else bits_list[-1]
            shift = SHIFTS[(j + 1) % len(SHIFTS)]
            add("u64 n=%d bits=%d shift=%d %s" % (n, bits, shift, dist),
                lambda L, r, n=n, b=bits, s=shift, d=dist: run_u64(L, r, n, b, s, d))
    add("u64 n=0 bits=8", lambda L, r: run_u64(L, r, 0, 8, 40, "uniform"))
    add("u64 n=4097 bits=0", lambda L, r: run_u64(L, r, 4097, 0, 40, "uniform"))
    for b in past:
        add("u64 n=4097 bits=%d %s" % (b, "refused" if b > MAX_PASSES * digit_cap() else "three full passes"),
            lambda L, r, b=b: run_u64(L, r, 4097, b, 0, "uniform"))


def pairs_cases(add):
    bits_list, past = bit_counts()
    for n in SIZES:
        for bits in bits_list:
            add("pairs n=%d bits=%d uniform" % (n, bits), lambda L, r, n=n, b=bits: run_pairs(L, r, n, b, "uniform"))
    for j, dist in enumerate(DISTS[1:]):
        for n in DIST_SIZES:
            bits = bits_list[(j + 2) % len(bits_list)] if dist != "top" else bits_list[-1]
            add("pairs n=%d bits=%d %s" % (n, bits, dist),
                lambda L, r, n=n, b=bits, d=dist: run_pairs(L, r, n, b, d))
    add("pairs n=0 bits=8", lambda L, r: run_pairs(L, r, 0, 8, "uniform"))
    add("pairs n=4097 bits=0", lambda L, r: run_pairs(L, r, 4097, 0, "uniform"))
    for b in past:  # past 32 bits the whole key is the field
        add("pairs n=4097 bits=%d %s" % (b, "refused" if b > MAX_PASSES * digit_cap() else "three full passes"),
            lambda L, r, b=b: run_pairs(L, r, 4097, b, "uniform"))


def hist0_cases(add):
    bits_list, _ = bit_counts()
    i = 0
    for n in [1, 4095, 4097, 3 * 4096 + 1, 64 * 4096 + 17]:
        for bits in bits_list:
            shift = SHIFTS[(i + 3) % len(SHIFTS)]
            i += 1
            add("u64 hist0 n=%d bits=%d shift=%d" % (n, bits, shift),
                lambda L, r, n=n, b=bits, s=shift: run_u64(L, r, n, b, s, "uniform", True))
    add("u64 hist0 n=%d equal" % (64 * 4096 + 17),
        lambda L, r: run_u64(L, r, 64 * 4096 + 17, bits_list[-1], 40, "equal", True))


def tiled_cases(add):
    bits_list, _ = bit_counts()
    scenarios = ["full", "quarter", "random", "some_empty", "tile_empty", "trailing", "ragged_bound", "random65"]
    i = 0
    for sc in scenarios:
        for bits in (bits_list if sc == "random" else [bits_list[i % len(bits_list)], bits_list[-1], bits_list[-2]]):
            shift = SHIFTS[i % len(SHIFTS)]
            i += 1
            for h in (False, True):
                add("tiled %s bits=%d shift=%d hist0=%d" % (sc, bits, shift, h),
                    lambda L, r, sc=sc, b=bits, s=shift, h=h: run_tiled(L, r, sc, b, s, h))


def scan_cases(add):
    for n in [0, 1, 4095, 4096, 4097]:
        for kind in ("ones", "random"):
            add("scan n=%d %s" % (n, kind), lambda L, r, n=n, k=kind: run_scan(L, r, n, k))


def large_cases(add):
    add("u64 n=%d bits=8 shift=40 (k_row_scan second round)" % ROW_SCAN_N,
        lambda L, r: run_u64(L, r, ROW_SCAN_N, 8, 40, "uniform"))
    for n in SCAN_LARGE:
        for kind in ("ones", "random"):
            add("scan n=%d %s" % (n, kind), lambda L, r, n=n, k=kind: run_scan(L, r, n, k))


def build_cases(which):
    cases = []
    add = lambda name, fn: cases.append((name, fn))
    mode = radix_mode()
    if which == "u64":
        u64_cases(add)
        return cases
    if mode == 0:
        # radix_sort_pairs would run k_rs_onesweep<D, true>, whose look-back wait has no bound
        raise SystemExit("refused: SGA_RADIX_MODE=0 runs only the 'u64' cases")
    pairs_cases(add)
    u64_cases(add)
    hist0_cases(add)  # the producer contract of modes 1 and 2
    tiled_cases(add)
    scan_cases(add)
    if which == "full":
        large_cases(add)
    return cases


def run_plan(L):
    rows = 0
    for kind in (0, 1, 2):
        for bits in range(1, 33):
            for n in (1, 4096, 4097, 1 << 20):
                print(json.dumps({"plan": [kind, bits, n], "out": plan(L, kind, bits, n)}))
                rows += 1
    print(json.dumps({"summary": True, "cases": rows, "digit_cap": digit_cap()}))
    return 0


def main(argv):
    which = argv[1] if len(argv) > 1 else "std"
    if which not in ("full", "std", "u64", "plan"):
        raise SystemExit("usage: python -m tests.sort_cases full|std|u64|plan")
    L = load()
    if which == "plan":
        return run_plan(L)
    cases = build_cases(which)
    print(json.dumps({"announce": len(cases), "mode": radix_mode(), "digit_cap": digit_cap()}), flush=True)
    done = failed = guards = 0
    for i, (name, fn) in enumerate(cases):
        rng = np.random.default_rng([20240607, i])
        try:
            msg, guard, npass = fn(L, rng)
        except HipFailure as e:  # stop here: launch nothing more on a device that reported an error
            print(json.dumps({"case": name, "ok": False, "hip_error": str(e)}), flush=True)
            print(json.dumps({"summary": True, "cases": done, "failed": failed + 1, "guards": guards,
                              "aborted": True}), flush=True)
            return 3
        done += 1
        failed += bool(msg)
        guards += bool(guard)
        print(json.dumps({"case": name, "ok": not msg, "guard": guard, "npass": npass, "msg": msg}), flush=True)
    print(json.dumps({"summary": True, "cases": done, "failed": failed, "guards": guards, "aborted": False}),
          flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
