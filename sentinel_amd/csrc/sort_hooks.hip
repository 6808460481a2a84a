// Test-only C entry points onto radix_sort.hip (libsga_sorttest.so; nothing here is linked into
// libsentinel_amd.so).  Each hook allocates every scratch and output buffer at exactly the size the
// engine's callers use, puts a guard zone of kGuardBytes behind each, runs one sort or scan, and
// copies back the buffers and a bit mask of the guard zones that changed.  The hooks never pick a
// result buffer: the caller applies the rule written in radix_sort.hpp to the pass count.
//
// Return value of every hook: 0, or a positive hipError_t / -5 (see sgat_last_error) after which the
// caller must stop using the device.  The sort's own return value goes to *npass.
#include "radix_sort.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace {

using namespace sga;

constexpr size_t kGuardBytes = 256;
constexpr uint8_t kGuardFill = 0xA5;

std::string g_err;

struct Check {
    void operator()(hipError_t e, const char *what) const {
        if (e != hipSuccess) throw HipError(std::string(what) + ": " + hipGetErrorString(e), __FILE__, __LINE__);
    }
};
#define SGAT_CHECK(expr) Check()((expr), #expr)

// Device buffer of exactly `bytes` bytes followed by a guard zone.
struct Guarded {
    uint8_t *p = nullptr;
    size_t bytes = 0;
    Guarded() = default;
    Guarded(const Guarded &) = delete;
    Guarded &operator=(const Guarded &) = delete;
    ~Guarded() {
        if (p) (void)hipFree(p);
    }
    void alloc(size_t nbytes, int fill) {
        bytes = nbytes;
        SGAT_CHECK(hipMalloc((void **)&p, bytes + kGuardBytes));
        if (bytes) SGAT_CHECK(hipMemset(p, fill, bytes));
        SGAT_CHECK(hipMemset(p + bytes, kGuardFill, kGuardBytes));
    }
    void upload(const void *src, size_t nbytes) {
        if (nbytes) SGAT_CHECK(hipMemcpy(p, src, nbytes, hipMemcpyHostToDevice));
    }
    void download(void *dst) const {
        if (dst && bytes) SGAT_CHECK(hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost));
    }
    bool guard_intact() const {
        uint8_t g[kGuardBytes];
        SGAT_CHECK(hipMemcpy(g, p + bytes, kGuardBytes, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < kGuardBytes; ++i)
            if (g[i] != kGuardFill) return false;
        return true;
    }
    template <typename T>
    T *as() const {
        return (T *)p;
    }
};

uint32_t guard_mask(std::initializer_list<const Guarded *> bufs) {
    uint32_t m = 0;
    int i = 0;
    for (const Guarded *b : bufs) {
        if (!b->guard_intact()) m |= 1u << i;
        ++i;
    }
    return m;
}

void finish() {
    SGAT_CHECK(hipDeviceSynchronize());
    SGAT_CHECK(hipGetLastError());
}

template <typename F>
int guarded_call(F &&f) {
    try {
        f();
        return 0;
    } catch (const HipError &e) {
        g_err = e.what;
        const hipError_t last = hipGetLastError();
        return last != hipSuccess ? (int)last : -5;
    } catch (const std::exception &e) {
        g_err = e.what();
        return -5;
    }
}

// scratch of the u64 sorts, sized as cluster.hip / concurrent.hip / flow.hip size theirs
struct Scratch64 {
    Guarded hist, hist_scan, partial, ghist, err;
    RadixScratch sc;
    size_t hist_words = 0;
    void alloc(size_t n, int bits) {
        hist_words = ((size_t)1 << radix64_digit_bits(bits)) * radix64_tiles(n);
        hist.alloc(hist_words * 4, 0xCD);
        hist_scan.alloc(hist_words * 4, 0xCD);
        partial.alloc(scan_partials_needed(hist_words) * 4, 0xCD);
        ghist.alloc(kRadixGhistWords * 4, 0xCD);
        err.alloc(4, 0);
        sc.hist = hist.as<uint32_t>();
        sc.hist_scan = hist_scan.as<uint32_t>();
        sc.partial = partial.as<uint32_t>();
        sc.ghist = ghist.as<uint32_t>();
        sc.err = err.as<uint32_t>();
    }
};

}  // namespace

extern "C" {

const char *sgat_last_error() { return g_err.c_str(); }

int sgat_guard_bytes() { return (int)kGuardBytes; }

// 1 when SGA_RADIX_MODE=0 selects the look-back sweeps in this process
int sgat_lookback() { return radix64_lookback(); }

// Guard bits: 0 keys, 1 pay, 2 keys_alt, 3 pay_alt, 4 hist, 5 hist_scan, 6 partial.
// The alt buffers start filled with 0xCD bytes.
int sgat_sort_pairs(const uint32_t *keys, const void *pay, uint64_t n, int bits, uint32_t *out_keys0,
                    uint32_t *out_keys1, void *out_pay0, void *out_pay1, int *npass, uint32_t *guard_bad) {
    // the look-back variant of the pairs sweep waits without a bound: never run from a test
    if (radix64_lookback()) return -22;
    return guarded_call([&] {
        Guarded k0, p0, k1, p1, hist, hist_scan, partial;
        k0.alloc(n * 4, 0);
        p0.alloc(n * sizeof(Payload), 0);
        k1.alloc(n * 4, 0xCD);
        p1.alloc(n * sizeof(Payload), 0xCD);
        const size_t hw = radix_hist_entries(n, bits);
        hist.alloc(hw * 4, 0xCD);
        hist_scan.alloc(hw * 4, 0xCD);
        partial.alloc(scan_partials_needed(hw) * 4, 0xCD);
        k0.upload(keys, n * 4);
        p0.upload(pay, n * sizeof(Payload));
        RadixScratch sc;
        sc.hist = hist.as<uint32_t>();
        sc.hist_scan = hist_scan.as<uint32_t>();
        sc.partial = partial.as<uint32_t>();
        *npass = radix_sort_pairs(k0.as<uint32_t>(), p0.as<Payload>(), k1.as<uint32_t>(), p1.as<Payload>(), n, bits,
                                  sc, nullptr);
        finish();
        k0.download(out_keys0);
        k1.download(out_keys1);
        p0.download(out_pay0);
        p1.download(out_pay1);
        *guard_bad = guard_mask({&k0, &p0, &k1, &p1, &hist, &hist_scan, &partial});
    });
}

// hist0: null, or the first pass's digit-major per-tile histogram ((1 << digit bits) * tiles words),
// uploaded to sc.hist and announced with hist0_ready.  *err: the look-back error word.
// Guard bits: 0 a, 1 alt, 2 hist, 3 hist_scan, 4 partial, 5 ghist, 6 err.  alt starts as 0xCD bytes.
int sgat_sort_u64(const uint64_t *el, uint64_t n, int key_shift, int bits, const uint32_t *hist0, uint64_t *out0,
                  uint64_t *out1, int *npass, uint32_t *err, uint32_t *guard_bad) {
    return guarded_call([&] {
        Guarded a, alt;
        Scratch64 s;
        a.alloc(n * 8, 0);
        alt.alloc(n * 8, 0xCD);
        s.alloc(n, bits);
        a.upload(el, n * 8);
        if (hist0) s.hist.upload(hist0, s.hist_words * 4);
        *npass = radix_sort_u64(a.as<uint64_t>(), alt.as<uint64_t>(), n, key_shift, bits, s.sc, nullptr,
                                hist0 != nullptr);
        finish();
        a.download(out0);
        alt.download(out1);
        SGAT_CHECK(hipMemcpy(err, s.err.p, 4, hipMemcpyDeviceToHost));
        *guard_bad = guard_mask({&a, &alt, &s.hist, &s.hist_scan, &s.partial, &s.ghist, &s.err});
    });
}

// src: radix64_tiles(n_host) * 4096 slots; tile_n0: 4 fills per tile; dn: element count kept on the
// device.  out0 / out1: `a` / `alt` (n_host elements each, both start as 0xCD bytes); src_after: src
// read back after the sort.
// Guard bits: 0 a, 1 alt, 2 hist, 3 hist_scan, 4 partial, 5 ghist, 6 err, 7 src, 8 tile_n0, 9 dn.
int sgat_sort_u64_tiled(const uint64_t *src, const uint32_t *tile_n0, uint32_t dn, uint64_t n_host, int key_shift,
                        int bits, const uint32_t *hist0, uint64_t *out0, uint64_t *out1, uint64_t *src_after,
                        int *npass, uint32_t *guard_bad) {
    return guarded_call([&] {
        const size_t tiles = radix64_tiles(n_host);
        Guarded a, alt, dsrc, dtn, ddn;
        Scratch64 s;
        a.alloc(n_host * 8, 0xCD);
        alt.alloc(n_host * 8, 0xCD);
        dsrc.alloc(tiles * kRadix64Tile * 8, 0);
        dtn.alloc(tiles * 4 * 4, 0);
        ddn.alloc(4, 0);
        s.alloc(n_host, bits);
        dsrc.upload(src, dsrc.bytes);
        dtn.upload(tile_n0, dtn.bytes);
        ddn.upload(&dn, 4);
        if (hist0) s.hist.upload(hist0, s.hist_words * 4);
        *npass = radix_sort_u64_tiled(dsrc.as<uint64_t>(), dtn.as<uint32_t>(), ddn.as<uint32_t>(), a.as<uint64_t>(),
                                      alt.as<uint64_t>(), n_host, key_shift, bits, s.sc, nullptr, hist0 != nullptr);
        finish();
        a.download(out0);
        alt.download(out1);
        dsrc.download(src_after);
        *guard_bad =
            guard_mask({&a, &alt, &s.hist, &s.hist_scan, &s.partial, &s.ghist, &s.err, &dsrc, &dtn, &ddn});
    });
}

// Guard bits: 0 out, 1 partial, 2 in.  out starts as 0xCD bytes.
int sgat_exclusive_scan(const uint32_t *in, uint64_t n, uint32_t *out, uint32_t *guard_bad) {
    return guarded_call([&] {
        Guarded din, dout, partial;
        din.alloc(n * 4, 0);
        dout.alloc(n * 4, 0xCD);
        partial.alloc(scan_partials_needed(n) * 4, 0xCD);
        din.upload(in, n * 4);
        exclusive_scan_u32(din.as<uint32_t>(), dout.as<uint32_t>(), n, partial.as<uint32_t>(), nullptr);
        finish();
        dout.download(out);
        *guard_bad = guard_mask({&dout, &partial, &din});
    });
}

// Host only: the pass plan of one sort and its scratch budget, in 32-bit words.
// kind 0 radix_sort_pairs, 1 radix_sort_u64, 2 radix_sort_u64_tiled.
// out[0] passes (above kRadixMaxPasses: the sort refuses), out[1] digit bits,
// out[2] hist words the kernels index, out[3] hist words the sizing function promises,
// out[4] / out[5] the same for `partial`, out[6] / out[7] for `ghist`.
// The pairs sort's look-back mode keeps its digit totals and tile counters in the first
// kRadixGhistWords of hist_scan and its status words in hist; out[2] counts both.
void sgat_sort_plan(int kind, int bits, uint64_t n, int64_t *out) {
    const int d = kind == 0 ? radix_pairs_digit_bits(bits) : radix64_digit_bits(bits);
    const int npass = (bits + d - 1) / d;
    const size_t status = ((size_t)1 << d) * (kind == 0 ? radix_tiles(n) : radix64_tiles(n));
    out[0] = npass;
    out[1] = d;
    if (kind == 0) {
        out[2] = (int64_t)(status + kRadixGhistWords);
        out[3] = (int64_t)radix_hist_entries(n, bits);
        out[4] = (int64_t)scan_partials_needed(status);
        out[5] = (int64_t)scan_partials_needed(radix_hist_entries(n, bits));
        out[6] = out[7] = 0;
    } else {
        out[2] = (int64_t)status;
        out[3] = (int64_t)(((size_t)1 << radix64_digit_bits(bits)) * radix64_tiles(n));
        out[4] = 0;  // the u64 sorts scan row by row: no partial sums
        out[5] = (int64_t)scan_partials_needed((size_t)out[3]);
        // per-digit totals (k_row_scan) or every pass's digit totals plus one tile counter per pass
        const int64_t lb = (int64_t)kRadixMaxPasses * 2048 + npass;
        out[6] = std::max<int64_t>((int64_t)npass << d, lb);
        out[7] = (int64_t)kRadixGhistWords;
    }
}

}  // extern "C"
