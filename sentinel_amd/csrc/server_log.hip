// Token server log: ClusterServerStatLogUtil's per-second sums formed behind every token batch (server_log.hpp).
#include "server_log.hpp"

#include <algorithm>

namespace sga {
namespace {

constexpr int kSlogThreads = 256;
constexpr int kSlogTiles = 4;  // tiles a block at least: a wave's held tuple gathers what its tiles share

// TokenResultStatus as the engine packs it: bits 48..55 of the 8-byte result
__device__ __forceinline__ int slog_status(uint64_t r) { return (int)(int8_t)(r >> 48); }

struct SlogKey {
    int64_t time_slot;
    int64_t flow_id;
    uint64_t tag;
    uint32_t kind;
};

// The claim word of a row: a mix of the whole tuple, never 0
__device__ __forceinline__ uint64_t slog_hash(const SlogKey &k) {
    uint64_t h = splitmix64((uint64_t)k.time_slot);
    h = splitmix64(h ^ (uint64_t)k.flow_id);
    h = splitmix64(h ^ (uint64_t)k.kind);
    h = splitmix64(h ^ k.tag);
    return h ? h : 1ull;
}

// One lane adds a wave's combined (count, events) to the tuple's row: linear probing from the hash, a free slot
// claimed by one compare-and-swap (the winner stores the key fields -- never count or events, which others may
// already be adding to), a slot holding the same hash shared.  No probe waits for anybody; a tuple that finds
// neither within the probe limit goes to the lost counters.
__device__ __forceinline__ void slog_update(const SlogTab &tb, const SlogKey &k, uint64_t h, int64_t sum,
                                            uint32_t cnt) {
    const uint32_t limit = min(tb.mask + 1u, kSlogProbe);
    uint32_t s = (uint32_t)(h >> 20) & tb.mask;
    for (uint32_t p = 0; p < limit; ++p, s = (s + 1u) & tb.mask) {
        unsigned long long cur = __atomic_load_n(&tb.hash[s], __ATOMIC_RELAXED);
        if (cur == 0ull) {
            cur = atomicCAS(&tb.hash[s], 0ull, (unsigned long long)h);
            if (cur == 0ull) {
                sga_server_log_row &r = tb.row[s];
                r.time_slot = k.time_slot;
                r.flow_id = k.flow_id;
                r.tag = k.tag;
                r.kind = (uint8_t)k.kind;
                atomicAdd(&tb.ctl[2], 1ull);
                cur = h;
            }
        }
        if (cur == h) {
            atomicAdd((unsigned long long *)&tb.row[s].count, (unsigned long long)sum);
            atomicAdd(&tb.row[s].events, cnt);
            return;
        }
    }
    atomicAdd(&tb.ctl[0], (unsigned long long)cnt);
    atomicAdd(&tb.ctl[1], (unsigned long long)sum);
}

// The wave's combine, shared by k_slog_add and k_slog_conc: the kernels differ only in how a lane forms its tuple.
// Every lane of the wave calls add() once a tile with (has, key, hash, add) and flush() once at the end.  While a
// lane holds an unmerged tuple, the first such lane's hash is broadcast and the lanes holding the same one sum their
// counts and count themselves -- registers only, as k_blog_add does.  After that loop the first lanes of all the
// tuples update the table side by side.  A tuple that at least two lanes share can become the wave's held tuple
// instead: its sums stay in registers over the wave's later tiles, which merge into it first, and reach the table
// once, at the end or when a tuple with more lanes in a tile takes its place.  A batch of blocks on one hot rule
// costs two atomics a wave, not two a lane.
struct SlogWave {
    // the held tuple: hash, sums and owner lane are wave-uniform, the key fields stay in lane hl's hk
    bool held = false;
    uint64_t hh = 0;
    int64_t hsum = 0;
    uint32_t hcnt = 0;
    int hl = 0;
    SlogKey hk{};

    __device__ __forceinline__ void add(const SlogTab &tb, int lane, bool has, const SlogKey &k, uint64_t h,
                                        int64_t add) {
        unsigned long long pend = __ballot(has);
        uint32_t hm = 0;  // lanes of this tile that merged into the held tuple
        if (held && pend) {
            const bool same = has && h == hh;
            const unsigned long long sm = __ballot(same);
            if (sm) {
                hsum += wave_sum_i64(same ? add : 0);
                hm = (uint32_t)__popcll(sm);
                hcnt += hm;
                has = has && !same;
                pend &= ~sm;
            }
        }
        bool first = false;  // this lane is the first of a tuple that goes to the table after the loop
        int64_t gsum = 0;
        uint32_t gcnt = 0;
        while (pend) {
            const int lead = __ffsll(pend) - 1;
            const uint64_t lh = (uint64_t)readlane_i64((int64_t)h, lead);
            const bool same = has && h == lh;
            const unsigned long long sm = __ballot(same);
            int64_t sum = add;
            uint32_t cnt = 1;
            if (sm & (sm - 1ull)) {  // wave-uniform: more than one lane holds the tuple
                sum = wave_sum_i64(same ? add : 0);
                cnt = (uint32_t)__popcll(sm);
            }
            if (cnt >= 2 && cnt > hm) {  // wave-uniform: the tuple becomes the held one, the old one goes out
                if (held && lane == hl) slog_update(tb, hk, hh, hsum, hcnt);
                held = true;
                hh = lh;
                hsum = sum;
                hcnt = hm = cnt;
                hl = lead;
                if (lane == lead) hk = k;
            } else if (lane == lead) {
                first = true;
                gsum = sum;
                gcnt = cnt;
            }
            has = has && !same;
            pend &= ~sm;
        }
        if (first) slog_update(tb, k, h, gsum, gcnt);
    }

    __device__ __forceinline__ void flush(const SlogTab &tb, int lane) {
        if (held && lane == hl) slog_update(tb, hk, hh, hsum, hcnt);
    }
};

// One lane a request, grid-stride over whole blocks (every lane of a wave stays in the loop: the combine is
// wave-wide).  The lane reads the request's 8-byte result and forms at most one tuple (the table in the header:
// which one depends on the checker that decided the batch); SlogWave does the rest.
__global__ __launch_bounds__(kSlogThreads) void k_slog_add(SlogTab tb, ReqIn in, int64_t ts_base, uint32_t n,
                                                           int checker, const uint64_t *__restrict__ res,
                                                           SlogBatch b) {
    if (b.fail && (*b.fail & b.fail_mask)) return;  // the batch failed: nothing is logged
    const int lane = (int)(threadIdx.x & 63u);
    SlogWave w;
    for (uint32_t i0 = blockIdx.x * kSlogThreads; i0 < n; i0 += gridDim.x * kSlogThreads) {
        const uint32_t i = i0 + threadIdx.x;
        bool has = false;
        SlogKey k{};
        int64_t add = 1;
        uint64_t h = 0;
        if (i < n) {
            const int st = slog_status(res[i]);
            if (checker == kSlogParam) {
                const uint32_t v0 = b.voff[i], nv = b.voff[i + 1] - v0;
                if (nv && st == SGA_TOKEN_OK) {
                    has = true;
                    k.kind = SGA_SLOG_PARAM_PASS;
                } else if (nv && st == SGA_TOKEN_BLOCKED) {
                    has = true;
                    k.kind = SGA_SLOG_PARAM_BLOCK;
                    uint32_t pos = b.bpos ? b.bpos[i] : 0u;
                    if (pos >= nv) pos = 0;
                    k.tag = (uint64_t)b.values[v0 + pos];
                }
            } else if (st == SGA_TOKEN_BLOCKED) {
                has = true;
                k.kind = (checker == kSlogDefault && in.prio_at(i)) ? SGA_SLOG_FLOW_BLOCK_PRIO : SGA_SLOG_FLOW_BLOCK;
                add = (int64_t)in.acq_at(i);
            } else if (st == SGA_TOKEN_SHOULD_WAIT) {
                has = true;
                k.kind = SGA_SLOG_FLOW_WAITING;
            } else if (st == SGA_TOKEN_OK && checker == kSlogSimple) {
                has = true;
                k.kind = SGA_SLOG_FLOW_PASS;
                add = (int64_t)in.acq_at(i);
            }
            if (has) {
                const int64_t t = ts_base + (int64_t)in.ts_at(i);
                k.time_slot = t - t % 1000;
                k.flow_id = in.flow_at(i);
                h = slog_hash(k);
            }
        }
        w.add(tb, lane, has, k, h, add);
    }
    w.flush(tb, lane);
}

// The concurrency checker's lines (ConcurrentClusterFlowChecker.java:58,67,73,99), behind k_conc_runs of one staged
// chunk: one lane an operation.  The lane reads the operation and its 16-byte result's status; an acquire answered
// OK or BLOCKED forms (second of ts, id, CONC_PASS / CONC_BLOCK) with its acquireCount, a release answered
// RELEASE_OK forms CONC_RELEASE under the flowId and acquireCount of its token's node: tok[aux[i]], a tombstone of
// the current epoch that nothing overwrites until a later batch.  Every other status forms nothing.
__global__ __launch_bounds__(kSlogThreads) void k_slog_conc(SlogTab tb, SlogConc c, uint32_t n) {
    const int lane = (int)(threadIdx.x & 63u);
    SlogWave w;
    for (uint32_t i0 = blockIdx.x * kSlogThreads; i0 < n; i0 += gridDim.x * kSlogThreads) {
        const uint32_t i = i0 + threadIdx.x;
        bool has = false;
        SlogKey k{};
        int64_t add = 0;
        uint64_t h = 0;
        if (i < n) {
            const int st = c.res[i].status;
            if (c.op[i] == SGA_CONCURRENT_ACQUIRE) {
                if (st == SGA_TOKEN_OK || st == SGA_TOKEN_BLOCKED) {
                    has = true;
                    k.kind = st == SGA_TOKEN_OK ? SGA_SLOG_CONC_PASS : SGA_SLOG_CONC_BLOCK;
                    k.flow_id = c.id[i];
                    add = (int64_t)c.acquire[i];
                }
            } else if (st == SGA_TOKEN_RELEASE_OK) {
                const uint32_t ix = c.aux[i];
                if (ix <= c.tmask) {
                    has = true;
                    k.kind = SGA_SLOG_CONC_RELEASE;
                    k.flow_id = c.tok[ix].flow_id;
                    add = (int64_t)c.tok[ix].acquire;
                }
            }
            if (has) {
                const int64_t t = c.ts[i];
                k.time_slot = t - t % 1000;
                h = slog_hash(k);
            }
        }
        w.add(tb, lane, has, k, h, add);
    }
    w.flush(tb, lane);
}

// Drain, first half: the rows of finished seconds (time_slot <= limit) copied out, counted, nothing removed yet
__global__ __launch_bounds__(kSlogThreads) void k_slog_drain(SlogTab tb, uint32_t slots, int64_t limit,
                                                             sga_server_log_row *out, uint32_t *count) {
    const uint32_t i = blockIdx.x * kSlogThreads + threadIdx.x;
    if (i >= slots || !tb.hash[i]) return;
    const sga_server_log_row r = tb.row[i];
    if (r.time_slot > limit) return;
    out[atomicAdd(count, 1u)] = r;  // out holds `slots` rows
}

// Drain, second half: the survivors rehashed into the other (empty) table, which then becomes the live one.  The
// hashes of one table are distinct, so every survivor claims a slot of its own; the table is as large as the old
// one, so the probe ends.
__global__ __launch_bounds__(kSlogThreads) void k_slog_rebuild(SlogTab from, SlogTab to, uint32_t slots,
                                                               int64_t limit) {
    const uint32_t i = blockIdx.x * kSlogThreads + threadIdx.x;
    if (i >= slots) return;
    const unsigned long long h = from.hash[i];
    if (!h) return;
    const sga_server_log_row r = from.row[i];
    if (r.time_slot <= limit) return;
    uint32_t s = (uint32_t)(h >> 20) & to.mask;
    for (uint32_t p = 0; p < slots; ++p, s = (s + 1u) & to.mask)
        if (atomicCAS(&to.hash[s], 0ull, h) == 0ull) {
            to.row[s] = r;
            atomicAdd(&to.ctl[2], 1ull);
            return;
        }
}

}  // namespace

int ServerLog::enable(uint32_t max_rows, hipStream_t stream) {
    if (max_rows == 0) max_rows = 1u << 16;  // the default: a choice, not a measurement
    if (max_rows > (1u << 26)) return SGA_EINVAL;
    uint32_t want = 64;
    while (want < max_rows) want <<= 1;
    if (on) {  // an empty log may be resized
        unsigned long long used = 0;
        SGA_HIP_CHECK(hipMemcpyAsync(&used, ctl.p + 2, 8, hipMemcpyDeviceToHost, stream));
        SGA_HIP_CHECK(hipStreamSynchronize(stream));
        if (used) return SGA_EINVAL;
        if (want == slots) return SGA_OK;
    }
    SGA_HIP_CHECK(hipStreamSynchronize(stream));
    for (int k = 0; k < 2; ++k) {
        hash[k].alloc(want);
        row[k].alloc(want);
        SGA_HIP_CHECK(hipMemsetAsync(hash[k].p, 0, hash[k].bytes(), stream));
        SGA_HIP_CHECK(hipMemsetAsync(row[k].p, 0, row[k].bytes(), stream));
    }
    out.alloc(want);
    if (!ctl.p) {
        ctl.alloc(4);
        cnt.alloc(1);
        SGA_HIP_CHECK(hipMemsetAsync(ctl.p, 0, ctl.bytes(), stream));
    }
    SGA_HIP_CHECK(hipStreamSynchronize(stream));
    slots = want;
    live = 0;
    on = true;
    return SGA_OK;
}

// blocks of a pass over n requests: kSlogTiles tiles a block at least
static uint32_t slog_blocks(uint32_t n) {
    const uint32_t per = kSlogTiles * kSlogThreads;
    return std::min<uint32_t>((n + per - 1) / per, 512);
}

void ServerLog::pass(const ReqIn &in, int64_t ts_base, uint32_t n, int checker, const void *results,
                     const SlogBatch &b, hipStream_t s) {
    if (!on || n == 0) return;
    const uint32_t nb = slog_blocks(n);
    hipLaunchKernelGGL(k_slog_add, dim3(nb), dim3(kSlogThreads), 0, s, tab(live), in, ts_base, n, checker,
                       (const uint64_t *)results, b);
    SGA_HIP_CHECK(hipGetLastError());
}

void ServerLog::pass_conc(const SlogConc &c, uint32_t n, hipStream_t s) {
    if (!on || n == 0) return;
    hipLaunchKernelGGL(k_slog_conc, dim3(slog_blocks(n)), dim3(kSlogThreads), 0, s, tab(live), c, n);
    SGA_HIP_CHECK(hipGetLastError());
}

int ServerLog::drain(int64_t before_ms, sga_server_log_row *rows, size_t cap, size_t *n, uint64_t *lost_events,
                     int64_t *lost_count, hipStream_t stream) {
    if (!on || !n || (cap && !rows)) return SGA_EINVAL;
    *n = 0;
    const int64_t limit = before_ms < 1000 ? -1 : before_ms - 1000;  // due: time_slot + 1000 <= before_ms
    const uint32_t nb = (slots + kSlogThreads - 1) / kSlogThreads;
    const SlogTab lv = tab(live), other = tab(live ^ 1);
    SGA_HIP_CHECK(hipMemsetAsync(cnt.p, 0, 4, stream));
    hipLaunchKernelGGL(k_slog_drain, dim3(nb), dim3(kSlogThreads), 0, stream, lv, slots, limit, out.p, cnt.p);
    SGA_HIP_CHECK(hipGetLastError());
    uint32_t c = 0;
    unsigned long long w[3] = {0, 0, 0};
    SGA_HIP_CHECK(hipMemcpyAsync(&c, cnt.p, 4, hipMemcpyDeviceToHost, stream));
    SGA_HIP_CHECK(hipMemcpyAsync(w, ctl.p, sizeof(w), hipMemcpyDeviceToHost, stream));
    SGA_HIP_CHECK(hipStreamSynchronize(stream));
    *n = c;
    if (c > cap) return SGA_ERANGE;  // nothing removed, the lost counters kept
    if (c) {
        SGA_HIP_CHECK(hipMemcpyAsync(rows, out.p, (size_t)c * sizeof(sga_server_log_row), hipMemcpyDeviceToHost, stream));
        // the survivors move to the other table (empty: zeroed when it was left), which becomes the live one
        SGA_HIP_CHECK(hipMemsetAsync(ctl.p + 2, 0, 8, stream));
        if (c < w[2]) {
            hipLaunchKernelGGL(k_slog_rebuild, dim3(nb), dim3(kSlogThreads), 0, stream, lv, other, slots, limit);
            SGA_HIP_CHECK(hipGetLastError());
            live ^= 1;
        }
        SGA_HIP_CHECK(hipMemsetAsync(lv.hash, 0, (size_t)slots * 8, stream));
        SGA_HIP_CHECK(hipMemsetAsync(lv.row, 0, (size_t)slots * sizeof(sga_server_log_row), stream));
    }
    if (w[0] || w[1]) SGA_HIP_CHECK(hipMemsetAsync(ctl.p, 0, 16, stream));
    SGA_HIP_CHECK(hipStreamSynchronize(stream));
    if (lost_events) *lost_events = w[0];
    if (lost_count) *lost_count = (int64_t)w[1];
    std::sort(rows, rows + c, [](const sga_server_log_row &x, const sga_server_log_row &y) {
        if (x.time_slot != y.time_slot) return x.time_slot < y.time_slot;
        if (x.flow_id != y.flow_id) return x.flow_id < y.flow_id;
        if (x.kind != y.kind) return x.kind < y.kind;
        return x.tag < y.tag;
    });
    return SGA_OK;
}

}  // namespace sga
