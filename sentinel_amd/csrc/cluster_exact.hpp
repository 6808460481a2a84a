// Device restatement of one cluster token request against a rule's window record: the exact
// per-request replay of ClusterFlowChecker.acquireClusterToken / SimpleClusterFlowChecker (used by
// the cluster kernels for runs the closed form does not cover, and by the local path's FlowSlot for
// cluster-mode rules decided by the embedded token server, FlowRuleChecker.passClusterCheck).
#pragma once
#include <hip/hip_runtime.h>

#include "cluster.hpp"
#include "cluster_line.hpp"

namespace sga {

enum : int8_t { TRS_BAD_REQUEST = -4, TRS_TOO_MANY_REQUEST = -2, TRS_FAIL = -1, TRS_OK = 0, TRS_BLOCKED = 1,
                TRS_SHOULD_WAIT = 2, TRS_NO_RULE_EXISTS = 3 };

// TokenResult packed as sga_token_result: remaining | waitInMs << 32 | status << 48
__device__ __forceinline__ uint64_t pack_result(int8_t status, int32_t remaining, int32_t wait) {
    return (uint64_t)(uint32_t)remaining | ((uint64_t)(uint16_t)(int16_t)wait << 32) |
           ((uint64_t)(uint8_t)status << 48);
}

// ---------------------------------------------------------------- exact per-request replay (device)
// Window state of a rule lives in one contiguous record: the 128-byte decision line (cluster_line.hpp)
// and behind it the 64-bit part of 8 x S + 12 int64, padded to an even number of 64-byte units
// (rec_units: 14 units = 896 bytes for S = 10, so every record starts on a 128-byte line):
//   line    ten (bucket number - base, PASS) pairs, base word with the flags, threshold, occupy counters,
//           the cached counter group -- all in 32-bit fields
//   header  [per bucket j: start, PASS] [occupy state: occupyCounter PASS, PASS_REQUEST, hasOccupied]
//           [cache: the six other counters of one bucket] [cache tag: that bucket's start] [threshold]
//   array   [per bucket j: WAITING, BLOCK, PASS_REQUEST, BLOCK_REQUEST, OCCUPIED_PASS, OCCUPIED_BLOCK]
// A record is compact or wide (kLnWide in the line's base word).  Compact (sampleCount <= 10 and every
// value fits its 32-bit field): the line is authoritative for the starts, PASS, the occupy state and the
// cache with its tag; the 64-bit header is unused.  Wide: the 64-bit header is authoritative and the line
// is ignored.  A compact record turns wide the moment a value does not fit (Rec::widen copies the line's
// state over unchanged), and stays wide until k_init_slots initialises the slot again: widening costs
// speed only, never a result.  The threshold copy (SlotParam::thr, written at every rule load by
// k_rec_thr) is kept in both places.  The array is authoritative and always written in both forms; the
// cache is only read by the closed forms, and a writer that changes a bucket's array counters without
// refreshing the cache clears the tag (Rec::cache_drop, from metric_add).
// A cold rule's closed form (k_cold_fused) so reads one 128-byte line of a compact record.
constexpr int kOccWords = 4;  // SlotOcc inside the record
static_assert(sizeof(SlotOcc) <= kOccWords * 8, "occupy state fits its words");
constexpr int kCacheWords = 6;  // the cached counter group (array order)
__host__ __device__ constexpr int rec_hdr_words(int S) { return 2 * S + kOccWords + kCacheWords + 2; }
__host__ __device__ constexpr uint32_t rec_units(int S) {
    // 64-byte units: the line (2) and the 64-bit part, even (128-byte aligned records)
    return 2u + (((uint32_t)(8 * S + 12 + 7) / 8 + 1u) & ~1u);
}
static_assert(rec_hdr_words(10) == 32 && rec_units(10) == 14, "S = 10: line, two-line header, 896-byte record");
static_assert(kLnWords64 * 8 == 128, "the decision line is one 128-byte line");
struct Rec {
    int64_t *r;  // the 64-bit part; the line lies in front of it
    int S;
    int32_t W;
    __device__ __forceinline__ uint32_t *ln() const { return reinterpret_cast<uint32_t *>(r - kLnWords64); }
    __device__ __forceinline__ uint64_t &bw() const { return *reinterpret_cast<uint64_t *>(ln() + LN_BASE); }
    __device__ __forceinline__ bool wide() const { return (bw() & kLnWide) != 0; }
    // ---- the 64-bit header (authoritative in a wide record)
    __device__ __forceinline__ int64_t &w_start(int j) const { return r[2 * j]; }
    __device__ __forceinline__ int64_t &w_pass(int j) const { return r[2 * j + 1]; }
    __device__ __forceinline__ SlotOcc &w_occ() const { return *reinterpret_cast<SlotOcc *>(r + 2 * S); }
    __device__ __forceinline__ int64_t *w_cache() const { return r + 2 * S + kOccWords; }
    __device__ __forceinline__ int64_t &w_tag() const { return r[2 * S + kOccWords + kCacheWords]; }
    __device__ __forceinline__ double &w_thr() const {
        return *reinterpret_cast<double *>(r + 2 * S + kOccWords + kCacheWords + 1);
    }
    // ---- the array (both forms)
    __device__ __forceinline__ int64_t *group(int j) const { return r + rec_hdr_words(S) + 6 * j; }
    __device__ __forceinline__ int64_t &cnt(int ev, int j) const {  // ev != CEV_PASS
        if (ev == CEV_WAITING) return group(j)[0];
        return group(j)[ev];  // BLOCK..OCCUPIED_BLOCK = ordinals 1..5
    }
    // ---- either form
    __device__ inline void widen() const {
        const uint64_t b = bw();
        if (b & kLnWide) return;
        const uint32_t *l = ln();
        const int64_t base = ln_base(b);
        for (int j = 0; j < S && j < kLnPairs; ++j) {
            const uint32_t d = l[2 * j];
            w_start(j) = d == kLnNoBucket ? kAbsent : ln_dec_bucket(d, base) * (int64_t)W;
            w_pass(j) = (int64_t)l[2 * j + 1];
        }
        w_occ() = SlotOcc{(int64_t)l[LN_OCC], (int64_t)l[LN_OCC + 1], (b & kLnHasOcc) ? 1 : 0, 0};
        const int tg = ln_tag(b);
        if (tg >= 0) {
            for (int k = 0; k < kCacheWords; ++k) w_cache()[k] = (int64_t)l[LN_CACHE + k];
            w_tag() = w_start(tg);
        } else {
            w_tag() = kAbsent;
        }
        bw() = b | kLnWide;
    }
    __device__ inline int64_t start(int j) const {
        const uint64_t b = bw();
        if (b & kLnWide) return w_start(j);
        const uint32_t d = ln()[2 * j];
        return d == kLnNoBucket ? kAbsent : ln_dec_bucket(d, ln_base(b)) * (int64_t)W;
    }
    // ws: a window start (t - t % W); rotating a bucket takes the cache from it
    __device__ inline void set_start(int j, int64_t ws) const {
        uint64_t b = bw();
        if (!(b & kLnWide)) {
            const int64_t q = ws / W;
            bool fits = ws >= 0 && q * (int64_t)W == ws;
            if (fits && !(b & kLnBaseSet)) {
                const int64_t nb = ln_pick_base(q);
                fits = ln_base_fits(nb);
                if (fits) b = (b & ~kLnBaseMask) | kLnBaseSet | (uint64_t)nb;
            }
            fits = fits && ln_delta_fits(q, ln_base(b));
            if (fits) {
                if (ln_tag(b) == j) b = ln_with_tag(b, -1);
                bw() = b;
                ln()[2 * j] = ln_enc_delta(q, ln_base(b));
                return;
            }
            widen();
        }
        w_start(j) = ws;
    }
    __device__ inline int64_t pass(int j) const { return wide() ? w_pass(j) : (int64_t)ln()[2 * j + 1]; }
    __device__ inline void set_pass(int j, int64_t v) const {
        if (!wide()) {
            if (ln_count_fits(v)) {
                ln()[2 * j + 1] = (uint32_t)v;
                return;
            }
            widen();
        }
        w_pass(j) = v;
    }
    __device__ inline SlotOcc occ() const {
        const uint64_t b = bw();
        if (b & kLnWide) return w_occ();
        return SlotOcc{(int64_t)ln()[LN_OCC], (int64_t)ln()[LN_OCC + 1], (b & kLnHasOcc) ? 1 : 0, 0};
    }
    __device__ inline void set_occ(const SlotOcc &o) const {
        const uint64_t b = bw();
        if (!(b & kLnWide)) {
            if (ln_count_fits(o.occ_pass) && ln_count_fits(o.occ_preq)) {
                ln()[LN_OCC] = (uint32_t)o.occ_pass;
                ln()[LN_OCC + 1] = (uint32_t)o.occ_preq;
                bw() = o.has_occ ? (b | kLnHasOcc) : (b & ~kLnHasOcc);
                return;
            }
            widen();
        }
        w_occ() = o;
    }
    // bucket j's array counters change without the cache following: the cached group is stale if it is j's
    __device__ inline void cache_drop(int j) const {
        const uint64_t b = bw();
        if (b & kLnWide) {
            if (w_tag() == w_start(j)) w_tag() = kAbsent;
        } else if (ln_tag(b) == j) {
            bw() = ln_with_tag(b, -1);
        }
    }
    // bucket j's six array counters (array order) as they were just written to the array
    __device__ inline void set_cache(int j, const int64_t (&g)[kCacheWords]) const {
        const uint64_t b = bw();
        if (b & kLnWide) {
            for (int k = 0; k < kCacheWords; ++k) w_cache()[k] = g[k];
            w_tag() = w_start(j);
            return;
        }
        bool fits = true;  // a cached counter that does not fit only takes the tag away
        for (int k = 0; k < kCacheWords; ++k) fits = fits && ln_count_fits(g[k]);
        if (fits)
            for (int k = 0; k < kCacheWords; ++k) ln()[LN_CACHE + k] = (uint32_t)g[k];
        bw() = ln_with_tag(b, fits ? j : -1);
    }
    __device__ inline double thr() const { return *reinterpret_cast<const double *>(ln() + LN_THR); }
    __device__ inline void set_thr(double v) const {
        *reinterpret_cast<double *>(ln() + LN_THR) = v;
        w_thr() = v;
    }
    // a slot's first state: no buckets, no base; sampleCount above the line's pairs is wide from here on
    __device__ inline void init(double thr_v) const {
        uint32_t *l = ln();
        for (int j = 0; j < kLnPairs; ++j) {
            l[2 * j] = kLnNoBucket;
            l[2 * j + 1] = 0;
        }
        bw() = S > kLnPairs ? kLnWide : 0ull;
        for (int k = LN_OCC; k < 2 * kLnWords64; ++k) l[k] = 0;
        for (int j = 0; j < S; ++j) {
            w_start(j) = kAbsent;
            w_pass(j) = 0;
            for (int k = 0; k < 6; ++k) group(j)[k] = 0;
        }
        w_occ() = SlotOcc{0, 0, 0, 0};
        w_tag() = kAbsent;
        set_thr(thr_v);
    }
};

__device__ __forceinline__ Rec rec_of(const ClusterState &st, const SlotParam &P) {
    return Rec{st.rec + (size_t)P.boff * 8 + kLnWords64, P.S, (int32_t)P.W};
}

struct WinRef {
    int j;
    bool detached;
};

__device__ __forceinline__ void bucket_zero(const Rec &R, int j) {
#pragma unroll
    for (int k = 1; k < CEV_N; ++k) R.cnt(k, j) = 0;
    R.set_pass(j, 0);
}

// LeapArray.currentWindow(t) on a ClusterMetricLeapArray (t >= 0)
__device__ inline WinRef cur_window(const ClusterState &st, const SlotParam &P, uint32_t s, int64_t t) {
    const Rec R = rec_of(st, P);
    const int j = (int)((t / P.W) % P.S);
    const int64_t ws = t - t % P.W;
    const int64_t old = R.start(j);
    if (old == kAbsent) {  // newEmptyBucket: no occupy transfer
        R.set_start(j, ws);
        bucket_zero(R, j);
        return WinRef{j, false};
    }
    if (ws == old) return WinRef{j, false};
    if (ws > old) {  // resetWindowTo + transferOccupyToBucket
        R.set_start(j, ws);
        bucket_zero(R, j);
        SlotOcc o = R.occ();
        if (o.has_occ) {
            R.cnt(CEV_OCCUPIED_PASS, j) += o.occ_pass;
            R.set_pass(j, R.pass(j) + o.occ_pass);
            o.occ_pass = 0;
            R.cnt(CEV_PASS_REQUEST, j) += o.occ_preq;
            o.occ_preq = 0;
            o.has_occ = 0;
            R.set_occ(o);
        }
        return WinRef{j, false};
    }
    return WinRef{j, true};  // time went backwards: detached bucket, adds lost
}

__device__ inline int64_t values_sum(const ClusterState &st, const SlotParam &P, int64_t t, int ev) {
    const Rec R = rec_of(st, P);
    int64_t s = 0;
    for (int j = 0; j < P.S; ++j) {
        const int64_t w = R.start(j);
        if (w != kAbsent && !(t - w > (int64_t)P.interval)) s += ev == CEV_PASS ? R.pass(j) : R.cnt(ev, j);
    }
    return s;
}

__device__ __forceinline__ double get_avg(const ClusterState &st, const SlotParam &P, uint32_t s, int64_t t, int ev) {
    cur_window(st, P, s, t);
    return (double)values_sum(st, P, t, ev) / P.isec;
}

__device__ __forceinline__ void metric_add(const ClusterState &st, const SlotParam &P, uint32_t s, int64_t t, int ev,
                                           int64_t n) {
    const WinRef w = cur_window(st, P, s, t);
    if (w.detached) return;
    const Rec R = rec_of(st, P);
    if (ev == CEV_PASS) {
        R.set_pass(w.j, R.pass(w.j) + n);
    } else {
        R.cnt(ev, w.j) += n;
        R.cache_drop(w.j);  // the cached group is stale now
    }
}

// ClusterMetricLeapArray.getFirstCountOfWindow(PASS) = getValidHead(now).value().get(PASS)
__device__ __forceinline__ int64_t head_pass(const ClusterState &st, const SlotParam &P, int64_t t) {
    const Rec R = rec_of(st, P);
    const int j = (int)(((t + P.W) / P.W) % P.S);
    const int64_t w = R.start(j);
    return (w != kAbsent && !(t - w > (int64_t)P.interval)) ? R.pass(j) : 0;
}

// ClusterFlowChecker.acquireClusterToken / SimpleClusterFlowChecker.acquireClusterToken for one request
__device__ inline uint64_t request_exact(const ClusterState &st, uint32_t s, int64_t t, int32_t a, bool p, int simple) {
    const SlotParam P = st.param[s];
    const double thr = simple ? P.thr_simple : P.thr;
    const double latest = get_avg(st, P, s, t, CEV_PASS);
    const double rem = thr - latest - (double)a;
    if (rem >= 0) {
        metric_add(st, P, s, t, CEV_PASS, a);
        metric_add(st, P, s, t, CEV_PASS_REQUEST, 1);
        if (p) metric_add(st, P, s, t, CEV_OCCUPIED_PASS, a);
        return pack_result(TRS_OK, j_d2i(rem), 0);
    }
    if (p) {
        const double occupy_avg = get_avg(st, P, s, t, CEV_WAITING);
        if (occupy_avg <= st.max_occupy_ratio * thr) {
            // ClusterMetric.tryOccupyNext(PASS, a, thr)
            const double latest2 = get_avg(st, P, s, t, CEV_PASS);
            const int64_t head = head_pass(st, P, t);
            const Rec R = rec_of(st, P);
            SlotOcc o = R.occ();
            if (latest2 + (double)((int64_t)a + o.occ_pass) - (double)head <= thr) {
                o.occ_pass += a;
                o.occ_preq += 1;
                o.has_occ = 1;
                R.set_occ(o);
                metric_add(st, P, s, t, CEV_WAITING, a);
                const int32_t wait = 1000 / P.S;
                if (wait > 0) return pack_result(TRS_SHOULD_WAIT, 0, wait);
            }
        }
    }
    metric_add(st, P, s, t, CEV_BLOCK, a);
    metric_add(st, P, s, t, CEV_BLOCK_REQUEST, 1);
    if (p) metric_add(st, P, s, t, CEV_OCCUPIED_BLOCK, a);
    return pack_result(TRS_BLOCKED, 0, 0);
}


}  // namespace sga
