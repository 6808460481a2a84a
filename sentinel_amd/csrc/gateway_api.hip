// Gateway API groups: paths -> bitmap of matching ApiDefinitions -> entry list (gateway_api.hpp).
#include "gateway_api.hpp"

#include <algorithm>
#include <array>
#include <cstring>
#include <map>

#include "radix_sort.hpp"

namespace sga {

namespace {

constexpr int kT = 256;
constexpr int kTLds = 1024;  // the staging workgroup: two of them fill a CU's wave slots beside 2 x 64 KiB of LDS

// The bytes of a path at any byte offset of the blob, taken from the aligned dwords that hold them (Guideline 13: no
// byte loads on the request bytes).  words: the blob's address rounded down to a dword, as a pointer derived from the
// kernel argument so the loads stay global_load; at: the path's byte offset from there.  next() is called at most
// len times, so only dwords that hold a byte of the path are read -- the contract of sga_gateway_parse_device.
struct PathBytes {
    const uint32_t *w;
    uint32_t word, have;
    __device__ __forceinline__ PathBytes(const uint32_t *words, uint64_t at, uint32_t len) {
        const uint32_t sh = ((uint32_t)at & 3u) * 8u;
        w = words + (at >> 2);
        word = 0;
        have = 0;
        if (len) {
            word = *w >> sh;
            have = 4 - (sh >> 3);
        }
    }
    __device__ __forceinline__ uint32_t next() {
        if (have == 0) {
            word = *++w;
            have = 4;
        }
        const uint32_t b = word & 0xFFu;
        word >>= 8;
        --have;
        return b;
    }
};

// One lane per request, every lane of a wave on the same predicate at the same time: the predicate record is
// wave-uniform (scalar loads, a uniform branch on its kind) and all 64 lanes walk one table, which is why the tables
// can sit in LDS -- kLds: the workgroup copies the blob there once and then serves tiles of kBlock requests in a grid
// stride; otherwise the walk reads the blob in global memory as k_gateway_parse does.  A lane writes its request's
// whole row itself (preds are sorted by api, so the row's words fill in order): no atomics, no zeroing pass, no
// stale bits.  The request's dwords are re-read per predicate from the L1; a predicate of an API that already
// matched is skipped (the OR is decided).  GatewayApiEngine::load checked every slice, class and transition.
template <bool kLds, int kBlock>
__global__ __launch_bounds__(kBlock) void k_gateway_api_match(ApiTable t, const uint32_t *__restrict__ path_off,
                                                          const uint32_t *__restrict__ path_len,
                                                          const uint8_t *__restrict__ bytes, uint64_t n_bytes,
                                                          const uint64_t *__restrict__ host_bits, uint32_t n,
                                                          uint64_t *__restrict__ match, uint32_t *status) {
    extern __shared__ uint32_t smem32[];
    const uint8_t *tab = t.blob;
    if (kLds) {
        const uint32_t *src = (const uint32_t *)t.blob;
        for (uint32_t o = threadIdx.x; o < t.blob_words; o += kBlock) smem32[o] = src[o];
        __syncthreads();
        tab = (const uint8_t *)smem32;
    }
    const uint32_t mis = (uint32_t)(uintptr_t)bytes & 3u;
    const uint32_t *words = (const uint32_t *)(bytes - mis);
    const uint32_t ntiles = (n + kBlock - 1) / kBlock;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t i = tile * kBlock + threadIdx.x;
        if (i >= n) continue;
        const uint32_t len = path_len[i], off = path_off[i];
        bool live = len != SGA_GW_NULL;
        if (live && (uint64_t)off + len > n_bytes) {
            live = false;
            atomicOr(status, 1u);
        }
        const uint64_t at = (uint64_t)off + mis;
        const uint64_t hb = host_bits ? host_bits[i] : 0ull;  // no word: a host predicate does not match
        uint64_t *row = match + (size_t)i * t.words;
        uint64_t acc = 0;
        uint32_t cw = 0;
        for (uint32_t p = 0; p < t.n_preds; ++p) {
            const ApiPred P = t.pred[p];
            const uint32_t wi = P.api >> 6;
            while (cw < wi) {
                row[cw++] = acc;
                acc = 0;
            }
            const uint64_t bit = 1ull << (P.api & 63u);
            if (!live || (acc & bit)) continue;
            bool m;
            if (P.kind == SGA_GW_API_HOST) {
                m = (hb >> P.a) & 1ull;
            } else if (P.kind == SGA_GW_API_EXACT) {
                m = len == P.b;  // the length before the bytes
                if (m) {
                    const uint8_t *pat = tab + P.a;
                    PathBytes rd(words, at, len);
                    for (uint32_t j = 0; j < len; ++j)
                        if (rd.next() != pat[j]) {
                            m = false;
                            break;
                        }
                }
            } else {
                const uint8_t *cls = tab + P.b;
                const uint16_t *trans = (const uint16_t *)(tab + P.c);
                PathBytes rd(words, at, len);
                uint32_t s = 1;
                for (uint32_t left = len; left && s; --left) s = trans[s * P.a + cls[rd.next()]];
                m = (tab[P.d + (s >> 3)] >> (s & 7u)) & 1u;
            }
            if (m) acc |= bit;
        }
        while (cw < t.words) {
            row[cw++] = acc;
            acc = 0;
        }
    }
}

// A row's word w without the bits past the last API: a bitmap the caller made itself cannot index past api_res.
__device__ __forceinline__ uint64_t api_row_word(const uint64_t *row, uint32_t w, uint32_t words, uint32_t n_apis) {
    const uint64_t bits = row[w];
    return w + 1 == words && (n_apis & 63u) ? bits & ((1ull << (n_apis & 63u)) - 1) : bits;
}

__global__ __launch_bounds__(kT) void k_gateway_api_count(const uint32_t *__restrict__ route,
                                                          const uint64_t *__restrict__ match, uint32_t words,
                                                          uint32_t n_apis, uint32_t n, uint32_t *__restrict__ cnt) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    uint32_t c = route[i] != SGA_GW_NULL;
    const uint64_t *row = match + (size_t)i * words;
    for (uint32_t w = 0; w < words; ++w) c += (uint32_t)__popcll(api_row_word(row, w, words, n_apis));
    cnt[i] = c;
}

// One lane per request writes its entries at off[i] .. off[i] + cnt[i]: the route (mode 0), then the set bits in
// ascending API index (mode 1); an entry at or past cap is counted, not written.  The last request's lane stores the
// total.
__global__ __launch_bounds__(kT) void k_gateway_api_scatter(
    const uint32_t *__restrict__ route, const uint64_t *__restrict__ match, uint32_t words, uint32_t n_apis,
    uint32_t n, const uint32_t *__restrict__ api_res, const uint32_t *__restrict__ off, const uint32_t *__restrict__ cnt,
    const uint32_t *__restrict__ field_off, const uint32_t *__restrict__ field_len, uint32_t nf, uint64_t cap,
    uint32_t src_base, uint32_t *__restrict__ src, uint32_t *__restrict__ pos, uint32_t *__restrict__ resource,
    uint8_t *__restrict__ mode, uint32_t *__restrict__ fo_out, uint32_t *__restrict__ fl_out,
    uint32_t *__restrict__ total) {
    const uint32_t i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    uint64_t j = off[i];
    if (i == n - 1) *total = off[i] + cnt[i];
    uint32_t q = 0;
    auto emit = [&](uint32_t r, uint8_t m) {
        if (j < cap) {
            src[j] = src_base + i;
            pos[j] = q;
            resource[j] = r;
            mode[j] = m;
            if (fo_out)
                for (uint32_t f = 0; f < nf; ++f) {
                    fo_out[j * nf + f] = field_off[(size_t)i * nf + f];
                    fl_out[j * nf + f] = field_len[(size_t)i * nf + f];
                }
        }
        ++j;
        ++q;
    };
    if (route[i] != SGA_GW_NULL) emit(route[i], 0);
    const uint64_t *row = match + (size_t)i * words;
    for (uint32_t w = 0; w < words; ++w) {
        uint64_t bits = api_row_word(row, w, words, n_apis);
        while (bits) {
            const uint32_t k = w * 64 + (uint32_t)__builtin_ctzll(bits);
            bits &= bits - 1;
            emit(api_res[k], 1);
        }
    }
}

}  // namespace

int GatewayApiEngine::load(const sga_gateway_api_pred *preds, size_t np, const uint32_t *api_resource, size_t na,
                           const uint8_t *blob, size_t blob_len, uint32_t nres, hipStream_t s, std::string *err) {
    if (np == 0) {
        // as GatewayEngine::load: the engine stream's end is past every match and expand issued so far
        SGA_HIP_CHECK(hipStreamSynchronize(s));
        d_pred.release();
        d_blob.release();
        d_api_res.release();
        n_apis = n_preds = n_device_preds = blob_words = 0;
        return SGA_OK;
    }
    if (!preds || !api_resource || na == 0 || (blob_len && !blob)) return SGA_EINVAL;
    if (blob_len > 0xFFFFFFFFull) return SGA_EINVAL;  // the offsets are 32 bits
    if (na > kApiMax) {
        if (err) *err = "gateway API table: " + std::to_string(na) + " APIs, the engine serves " + std::to_string(kApiMax);
        return SGA_ERANGE;
    }
    for (size_t k = 0; k < na; ++k)
        if (api_resource[k] >= nres) return SGA_EINVAL;
    std::vector<ApiPred> recs;
    recs.reserve(np);
    std::map<std::array<uint32_t, 5>, bool> seen;  // DFA slices already checked
    uint32_t n_host = 0;
    for (size_t j = 0; j < np; ++j) {
        const sga_gateway_api_pred &P = preds[j];
        if (P.api >= na) return SGA_EINVAL;
        if (P.kind == SGA_GW_API_EXACT) {
            if ((uint64_t)P.a + P.b > blob_len) return SGA_EINVAL;
            recs.push_back(ApiPred{P.api, P.kind, P.a, P.b, 0, 0});
        } else if (P.kind == SGA_GW_API_HOST) {
            if (P.a >= kApiHostMax) return SGA_EINVAL;
            ++n_host;
            recs.push_back(ApiPred{P.api, P.kind, P.a, 0, 0, 0});
        } else if (P.kind == SGA_GW_API_DFA) {
            // sga_gateway_regex's contract, as GatewayEngine::load_regex checks it
            const uint32_t ns = P.a, nc = P.b, class_off = P.c, trans_off = P.d, accept_off = P.e;
            if (ns < 2 || ns > 65535 || nc < 1 || nc > 256) return SGA_EINVAL;
            const uint64_t nt = (uint64_t)ns * nc, nacc = (ns + 7) / 8;
            if ((uint64_t)class_off + 256 > blob_len || (uint64_t)trans_off + 2 * nt > blob_len ||
                (uint64_t)accept_off + nacc > blob_len || (trans_off & 1u))
                return SGA_EINVAL;
            const std::array<uint32_t, 5> key{ns, nc, class_off, trans_off, accept_off};
            if (!seen.count(key)) {
                for (uint32_t b = 0; b < 256; ++b)
                    if (blob[class_off + b] >= nc) return SGA_EINVAL;
                for (uint64_t q = 0; q < nt; ++q) {
                    uint16_t to;
                    std::memcpy(&to, blob + trans_off + 2 * q, 2);
                    if (to >= ns || (q < nc && to != 0)) return SGA_EINVAL;  // row 0 is dead
                }
                if (blob[accept_off] & 1u) return SGA_EINVAL;  // state 0 accepts nothing
                seen[key] = true;
            }
            recs.push_back(ApiPred{P.api, P.kind, nc, class_off, trans_off, accept_off});
        } else {
            return SGA_EINVAL;
        }
    }
    if (n_host > kApiHostMax) {
        if (err) *err = "gateway API table: " + std::to_string(n_host) + " host predicates, the word holds " +
                        std::to_string(kApiHostMax);
        return SGA_ERANGE;
    }
    std::stable_sort(recs.begin(), recs.end(), [](const ApiPred &x, const ApiPred &y) { return x.api < y.api; });
    if (!cus) {
        int dev = 0;
        hipDeviceProp_t prop;
        SGA_HIP_CHECK(hipGetDevice(&dev));
        SGA_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
        cus = std::max(1, prop.multiProcessorCount);
    }
    const size_t words4 = (blob_len + 3) / 4;
    std::vector<uint8_t> padded(std::max<size_t>(words4, 1) * 4, 0);
    if (blob_len) std::memcpy(padded.data(), blob, blob_len);
    SGA_HIP_CHECK(hipStreamSynchronize(s));
    d_pred.alloc(recs.size());
    d_blob.alloc(padded.size());
    d_api_res.alloc(na);
    SGA_HIP_CHECK(hipMemcpyAsync(d_pred.p, recs.data(), recs.size() * sizeof(ApiPred), hipMemcpyHostToDevice, s));
    SGA_HIP_CHECK(hipMemcpyAsync(d_blob.p, padded.data(), padded.size(), hipMemcpyHostToDevice, s));
    SGA_HIP_CHECK(hipMemcpyAsync(d_api_res.p, api_resource, na * 4, hipMemcpyHostToDevice, s));
    SGA_HIP_CHECK(hipStreamSynchronize(s));
    n_apis = (uint32_t)na;
    n_preds = (uint32_t)recs.size();
    n_device_preds = n_preds - n_host;
    blob_words = (uint32_t)words4;
    return SGA_OK;
}

void GatewayApiEngine::launch_match(const uint32_t *d_path_off, const uint32_t *d_path_len, const uint8_t *d_bytes,
                                    uint64_t n_bytes, const uint64_t *d_host_bits, uint32_t n, uint64_t *d_match,
                                    uint32_t *d_status, hipStream_t s) const {
    if (in_lds()) {
        const uint32_t ntiles = (n + kTLds - 1) / kTLds;
        const unsigned grid = std::min<uint32_t>(ntiles, (uint32_t)cus * 2u);
        hipLaunchKernelGGL((k_gateway_api_match<true, kTLds>), dim3(grid), dim3(kTLds), (size_t)blob_words * 4, s, table(),
                           d_path_off, d_path_len, d_bytes, n_bytes, d_host_bits, n, d_match, d_status);
    } else {
        const uint32_t ntiles = (n + kT - 1) / kT;
        const unsigned grid = std::min<uint32_t>(ntiles, (uint32_t)cus * 8u);
        hipLaunchKernelGGL((k_gateway_api_match<false, kT>), dim3(grid), dim3(kT), 0, s, table(), d_path_off, d_path_len,
                           d_bytes, n_bytes, d_host_bits, n, d_match, d_status);
    }
    SGA_HIP_CHECK(hipGetLastError());
}

void GatewayApiEngine::ensure_scratch(size_t max_batch) {
    if (d_cnt.n >= max_batch) return;
    d_cnt.alloc(max_batch);
    d_off.alloc(max_batch);
    d_partial.alloc(scan_partials_needed(max_batch) + 16);
}

void GatewayApiEngine::launch_count_scan(const uint32_t *d_route, const uint64_t *d_match, uint32_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_gateway_api_count, dim3((n + kT - 1) / kT), dim3(kT), 0, s, d_route, d_match, words(), n_apis,
                       n, d_cnt.p);
    exclusive_scan_u32(d_cnt.p, d_off.p, n, d_partial.p, s);
    SGA_HIP_CHECK(hipGetLastError());
}

void GatewayApiEngine::launch_scatter(const uint32_t *d_route, const uint64_t *d_match, uint32_t n,
                                      const uint32_t *d_field_off, const uint32_t *d_field_len, uint32_t n_fields,
                                      uint64_t cap, uint32_t src_base, uint32_t *d_src, uint32_t *d_pos,
                                      uint32_t *d_resource, uint8_t *d_mode, uint32_t *d_field_off_out,
                                      uint32_t *d_field_len_out, uint32_t *d_total, hipStream_t s) {
    hipLaunchKernelGGL(k_gateway_api_scatter, dim3((n + kT - 1) / kT), dim3(kT), 0, s, d_route, d_match, words(), n_apis,
                       n, d_api_res.p, d_off.p, d_cnt.p, d_field_off, d_field_len, n_fields, cap, src_base, d_src, d_pos,
                       d_resource, d_mode, d_field_off_out, d_field_len_out, d_total);
    SGA_HIP_CHECK(hipGetLastError());
}

template <class T>
static void at_least(DevBuf<T> &b, size_t n) {
    if (b.n < std::max<size_t>(n, 1)) b.alloc(std::max<size_t>(n, 1));
}

int GatewayApiEngine::match_host(const uint32_t *path_off, const uint32_t *path_len, const uint8_t *bytes,
                                 size_t n_bytes, const uint64_t *host_bits, size_t n, uint64_t *match,
                                 size_t max_batch, hipStream_t s) {
    const size_t cap = std::min(n, max_batch), W = words();
    at_least(h_off, cap);
    at_least(h_len, cap);
    at_least(h_bits, cap);
    at_least(h_match, cap * W);
    at_least(h_bytes, std::max<size_t>(n_bytes, 4));
    at_least(h_status, 1);
    SGA_HIP_CHECK(hipMemsetAsync(h_status.p, 0, 4, s));
    if (n_bytes) SGA_HIP_CHECK(hipMemcpyAsync(h_bytes.p, bytes, n_bytes, hipMemcpyHostToDevice, s));
    for (size_t b = 0; b < n; b += cap) {
        const size_t m = std::min(cap, n - b);
        SGA_HIP_CHECK(hipMemcpyAsync(h_off.p, path_off + b, m * 4, hipMemcpyHostToDevice, s));
        SGA_HIP_CHECK(hipMemcpyAsync(h_len.p, path_len + b, m * 4, hipMemcpyHostToDevice, s));
        if (host_bits) SGA_HIP_CHECK(hipMemcpyAsync(h_bits.p, host_bits + b, m * 8, hipMemcpyHostToDevice, s));
        launch_match(h_off.p, h_len.p, h_bytes.p, n_bytes, host_bits ? h_bits.p : nullptr, (uint32_t)m, h_match.p,
                     h_status.p, s);
        SGA_HIP_CHECK(hipMemcpyAsync(match + b * W, h_match.p, m * W * 8, hipMemcpyDeviceToHost, s));
        SGA_HIP_CHECK(hipStreamSynchronize(s));
    }
    uint32_t st = 0;
    SGA_HIP_CHECK(hipMemcpy(&st, h_status.p, 4, hipMemcpyDeviceToHost));
    return st ? SGA_EINVAL : SGA_OK;
}

int GatewayApiEngine::expand_host(const uint32_t *route, const uint64_t *match, size_t n, const uint32_t *field_off,
                                  const uint32_t *field_len, uint32_t nf, size_t cap, uint32_t *src, uint32_t *pos,
                                  uint32_t *resource, uint8_t *mode, uint32_t *field_off_out, uint32_t *field_len_out,
                                  size_t *total, size_t max_batch, hipStream_t s) {
    const size_t chunk = std::min(n, max_batch), W = words();
    const bool gather = field_off_out != nullptr;
    ensure_scratch(chunk);
    at_least(h_route, chunk);
    at_least(h_match, chunk * W);
    at_least(h_total, 1);
    if (gather) {
        at_least(h_foff, chunk * nf);
        at_least(h_flen, chunk * nf);
    }
    size_t done = 0;
    for (size_t b = 0; b < n; b += chunk) {
        const size_t m = std::min(chunk, n - b);
        SGA_HIP_CHECK(hipMemcpyAsync(h_route.p, route + b, m * 4, hipMemcpyHostToDevice, s));
        SGA_HIP_CHECK(hipMemcpyAsync(h_match.p, match + b * W, m * W * 8, hipMemcpyHostToDevice, s));
        launch_count_scan(h_route.p, h_match.p, (uint32_t)m, s);
        uint32_t last[2];
        SGA_HIP_CHECK(hipMemcpyAsync(&last[0], d_off.p + (m - 1), 4, hipMemcpyDeviceToHost, s));
        SGA_HIP_CHECK(hipMemcpyAsync(&last[1], d_cnt.p + (m - 1), 4, hipMemcpyDeviceToHost, s));
        SGA_HIP_CHECK(hipStreamSynchronize(s));
        const size_t need = (size_t)last[0] + last[1];
        // the entries of this chunk that still fit the caller's arrays: the rest are counted only
        const size_t room = cap > done ? std::min(need, cap - done) : 0;
        if (room) {
            at_least(h_src, room);
            at_least(h_pos, room);
            at_least(h_res, room);
            at_least(h_mode, room);
            if (gather) {
                at_least(h_foff_out, room * nf);
                at_least(h_flen_out, room * nf);
                SGA_HIP_CHECK(hipMemcpyAsync(h_foff.p, field_off + b * nf, m * nf * 4, hipMemcpyHostToDevice, s));
                SGA_HIP_CHECK(hipMemcpyAsync(h_flen.p, field_len + b * nf, m * nf * 4, hipMemcpyHostToDevice, s));
            }
            launch_scatter(h_route.p, h_match.p, (uint32_t)m, gather ? h_foff.p : nullptr, gather ? h_flen.p : nullptr,
                           nf, room, (uint32_t)b, h_src.p, h_pos.p, h_res.p, h_mode.p, gather ? h_foff_out.p : nullptr,
                           gather ? h_flen_out.p : nullptr, h_total.p, s);
            SGA_HIP_CHECK(hipMemcpyAsync(src + done, h_src.p, room * 4, hipMemcpyDeviceToHost, s));
            SGA_HIP_CHECK(hipMemcpyAsync(pos + done, h_pos.p, room * 4, hipMemcpyDeviceToHost, s));
            SGA_HIP_CHECK(hipMemcpyAsync(resource + done, h_res.p, room * 4, hipMemcpyDeviceToHost, s));
            SGA_HIP_CHECK(hipMemcpyAsync(mode + done, h_mode.p, room, hipMemcpyDeviceToHost, s));
            if (gather) {
                SGA_HIP_CHECK(hipMemcpyAsync(field_off_out + done * nf, h_foff_out.p, room * nf * 4,
                                             hipMemcpyDeviceToHost, s));
                SGA_HIP_CHECK(hipMemcpyAsync(field_len_out + done * nf, h_flen_out.p, room * nf * 4,
                                             hipMemcpyDeviceToHost, s));
            }
            SGA_HIP_CHECK(hipStreamSynchronize(s));
        }
        done += need;
    }
    *total = done;
    return done > cap ? SGA_ERANGE : SGA_OK;
}

}  // namespace sga
