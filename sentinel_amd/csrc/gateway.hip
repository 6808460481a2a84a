// Gateway flow rules: request fields -> argument vectors (gateway.hpp).
#include "gateway.hpp"

#include <algorithm>
#include <array>
#include <cstring>
#include <map>

namespace sga {

constexpr int kT = 256;
// The param word of a refused event: an empty vector at offset 2^32 - 1, past any value buffer (n_values stays
// below that).  Every submit entry refuses it under SGA_EV_ARGS by its range check, and an empty vector gives the
// passes that read arguments ahead of the device entry's verdict (the CacheMap count pass) nothing to dereference.
constexpr uint64_t kPoison = 0xFFFFFFFFull << 32;

struct HostRd {
    const uint8_t *b;
    uint64_t u64(uint32_t o) const {
        uint64_t v;
        std::memcpy(&v, b + o, 8);
        return v;
    }
    uint32_t u32(uint32_t o) const {
        uint32_t v;
        std::memcpy(&v, b + o, 4);
        return v;
    }
    uint32_t u8(uint32_t o) const { return b[o]; }
};

// A string at any byte address of the blob, read as aligned dwords (Guideline 13: no byte loads on the
// 32-byte stripes): base = the address rounded down to a dword, sh = the bits to drop from its first dword.  A
// read touches only dwords that hold at least one byte of the string, so it never leaves the memory the
// slice check admitted by more than the rest of a dword it already owns a byte of.
struct DevRd {
    const uint32_t *base;
    uint32_t sh;  // 0, 8, 16, 24
    const uint8_t *bytes;
    __device__ __forceinline__ DevRd(const uint8_t *p)
        : base((const uint32_t *)((uintptr_t)p & ~(uintptr_t)3)), sh(((uint32_t)(uintptr_t)p & 3u) * 8u), bytes(p) {}
    __device__ __forceinline__ uint32_t u32(uint32_t o) const {  // o is a multiple of 4
        const uint32_t *w = base + (o >> 2);
        const uint32_t a = w[0];
        if (sh == 0) return a;
        return (a >> sh) | (w[1] << (32 - sh));
    }
    __device__ __forceinline__ uint64_t u64(uint32_t o) const {
        const uint32_t *w = base + (o >> 2);
        const uint32_t a = w[0], b = w[1];
        if (sh == 0) return (uint64_t)b << 32 | a;
        const uint32_t c = w[2];
        return (uint64_t)((b >> sh) | (c << (32 - sh))) << 32 | ((a >> sh) | (b << (32 - sh)));
    }
    __device__ __forceinline__ uint32_t u8(uint32_t o) const { return bytes[o]; }
};

// String.equals / String.contains over UTF-8 bytes: on valid UTF-8 a byte substring is a char substring,
// since no character's encoding is a suffix or an infix of another's (UTF-8 is self-synchronising).
__device__ __forceinline__ bool bytes_equal(const uint8_t *a, const uint8_t *b, uint32_t n) {
    for (uint32_t j = 0; j < n; ++j)
        if (a[j] != b[j]) return false;
    return true;
}
__device__ __forceinline__ bool bytes_contain(const uint8_t *v, uint32_t vn, const uint8_t *p, uint32_t pn) {
    if (pn > vn) return false;
    for (uint32_t s = 0; s + pn <= vn; ++s)
        if (bytes_equal(v + s, p, pn)) return true;
    return false;
}

// A REGEX program over the value: s = 1; per byte s = trans[s * n_classes + class_map[byte]] until s == 0 (the dead
// state); the accept bit of s answers, for an empty value that of the start state.  The value is read as the aligned
// dwords that hold a byte of it, one load for up to four bytes (Guideline 13, as DevRd does for the hash; the
// tables' own bytes and halfwords are what they are).  load_regex checked every class and transition against the
// table's sizes, so whatever the bytes -- malformed UTF-8 included -- the walk stays inside the tables.
__device__ __forceinline__ bool regex_walk(const GwRegex P, const uint8_t *__restrict__ blob, const uint8_t *v,
                                           uint32_t len) {
    const uint8_t *cls = blob + P.class_off;
    const uint16_t *trans = (const uint16_t *)(blob + P.trans_off);
    const DevRd rd(v);
    const uint32_t *w = rd.base;
    uint32_t s = 1, word = 0, have = 0;  // have: bytes of the value left in word
    if (len) {
        word = *w >> rd.sh;
        have = 4 - (rd.sh >> 3);
    }
    for (uint32_t left = len; left && s; --left) {
        if (have == 0) {
            word = *++w;
            have = 4;
        }
        s = trans[s * P.n_classes + cls[word & 0xFFu]];
        word >>= 8;
        --have;
    }
    return (blob[P.accept_off + (s >> 3)] >> (s & 7u)) & 1u;
}

// One lane per (event, argument slot).  Slot 0's lane also owns the event's flags and param words and checks
// every slice of the event, so a refused event is poisoned by one writer; the other lanes check their own slice
// and the event's room again and write nothing when either fails.
__global__ __launch_bounds__(kT) void k_gateway_parse(GwTable t, const uint32_t *__restrict__ resource,
                                                      const uint8_t *__restrict__ mode,
                                                      const uint32_t *__restrict__ field_off,
                                                      const uint32_t *__restrict__ field_len,
                                                      const uint8_t *__restrict__ bytes, uint64_t n_bytes,
                                                      const uint64_t *__restrict__ regex_bits, uint32_t n,
                                                      uint8_t *__restrict__ flags, uint64_t *__restrict__ param,
                                                      uint64_t *__restrict__ values, uint64_t n_values,
                                                      uint64_t value_base, uint64_t bias, uint32_t *status) {
    const uint64_t tid = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (tid >= (uint64_t)n * t.max_args) return;
    const uint32_t i = (uint32_t)(tid / t.max_args), k = (uint32_t)(tid % t.max_args);
    const uint32_t r = resource[i];
    if (r >= t.nres) return;
    const GwRes R = t.res[r];
    if (R.nargs == 0) return;  // no gateway rule: the event stays as given
    const int32_t md = mode[i];
    const bool mode_ok = R.mode_min > R.mode_max || (R.mode_min == md && R.mode_max == md);
    const uint32_t nargs = mode_ok ? R.nargs : 0;
    const uint64_t off = value_base + (uint64_t)i * 2 * t.max_args;
    const bool room = off + 2 * (uint64_t)nargs <= n_values && off <= 0xFFFFFFFFull;
    const size_t frow = (size_t)i * t.n_fields;
    if (k == 0) {
        bool ok = room;
        for (uint32_t q = 0; q < nargs && ok; ++q) {
            const GwSlot S = t.slot[R.slot_off + q];
            if (S.kind != kGwItem) continue;
            const uint32_t fl = field_len[frow + S.field];
            if (fl != SGA_GW_NULL && (uint64_t)field_off[frow + S.field] + fl > n_bytes) ok = false;
        }
        flags[i] |= (uint8_t)SGA_EV_ARGS;
        param[i] = ok ? (off << 32 | nargs) : kPoison;
        if (!ok) atomicOr(status, 1u);
    }
    if (k >= nargs || !room) return;
    const GwSlot S = t.slot[R.slot_off + k];
    uint64_t head = (uint64_t)SGA_ARG_SCALAR << 62, key = 0;
    if (S.kind == kGwDefault) {
        key = t.key_d;
    } else if (S.kind == kGwNull) {
        head = (uint64_t)SGA_ARG_NULL << 62;
    } else {
        const uint32_t fl = field_len[frow + S.field], fo = field_off[frow + S.field];
        if (fl == SGA_GW_NULL) {
            head = (uint64_t)SGA_ARG_NULL << 62;
        } else {
            if ((uint64_t)fo + fl > n_bytes) return;  // slot 0's lane refused the event
            const uint8_t *v = bytes + fo;
            bool keep = true;
            if (S.has_pattern) {
                const uint8_t *p = t.pat + S.pat_off;
                if (S.match == SGA_GW_EXACT) keep = fl == S.pat_len && bytes_equal(v, p, fl);
                else if (S.match == SGA_GW_CONTAINS) keep = bytes_contain(v, fl, p, S.pat_len);
                else if (S.match == SGA_GW_REGEX)  // a program goes before the word
                    keep = S.program ? regex_walk(t.rx[S.pat_off], t.rx_blob, v, fl)
                                     : !regex_bits || ((regex_bits[i] >> k) & 1ull);
            }
            key = keep ? xxh64(DevRd(v), fl, SGA_GW_SEED) : t.key_nm;
        }
    }
    values[off - bias + 2 * k] = head;  // bias: where the buffer starts in the caller's numbering (host chunks)
    values[off - bias + 2 * k + 1] = key;
}

uint64_t gateway_string_key(const uint8_t *bytes, size_t len) {
    return xxh64(HostRd{bytes}, (uint32_t)len, SGA_GW_SEED);
}

int GatewayEngine::load(const sga_gateway_item *items, size_t n_items, const uint8_t *blob, size_t blob_len,
                        uint32_t nf, uint32_t nres_now, hipStream_t s, std::string *err) {
    if (n_items && (!items || !nres_now)) return SGA_EINVAL;
    if (blob_len && !blob) return SGA_EINVAL;
    std::vector<GwRes> res(nres_now, GwRes{0, 0, INT32_MAX, INT32_MIN});
    std::vector<uint32_t> n_param(nres_now, 0);
    std::vector<uint8_t> non_param(nres_now, 0);
    for (size_t j = 0; j < n_items; ++j) {
        const sga_gateway_item &it = items[j];
        if (it.resource >= nres_now || it.index < -1 || it.index >= 64) return SGA_EINVAL;
        if (it.index < 0) {
            non_param[it.resource] = 1;
            continue;
        }
        if (it.field >= nf) return SGA_EINVAL;
        if (it.has_pattern && (uint64_t)it.pattern_off + it.pattern_len > blob_len) return SGA_EINVAL;
        n_param[it.resource]++;
        GwRes &R = res[it.resource];
        R.mode_min = std::min(R.mode_min, it.resource_mode);
        R.mode_max = std::max(R.mode_max, it.resource_mode);
    }
    uint32_t total = 0, most = 0;
    for (uint32_t r = 0; r < nres_now; ++r) {
        const uint32_t na = n_param[r] + non_param[r];
        if (na > 64) {
            if (err) *err = "gateway rules: resource " + std::to_string(r) + " needs " + std::to_string(na) +
                            " arguments, the engine serves 64";
            return SGA_ERANGE;
        }
        res[r].slot_off = total;
        res[r].nargs = na;
        total += na;
        most = std::max(most, na);
    }
    std::vector<GwSlot> slots(total, GwSlot{0, 0, 0, kGwNull, 0, 0, 0});
    std::vector<int64_t> winner(total, -1);  // the item that writes each slot
    for (uint32_t r = 0; r < nres_now; ++r)
        if (non_param[r]) slots[res[r].slot_off + res[r].nargs - 1].kind = kGwDefault;
    for (size_t j = 0; j < n_items; ++j) {
        const sga_gateway_item &it = items[j];
        if (it.index < 0) continue;
        if ((uint32_t)it.index >= n_param[it.resource]) return SGA_EINVAL;  // indices are dense per resource
        GwSlot &S = slots[res[it.resource].slot_off + it.index];
        const uint8_t m = it.match_strategy == SGA_GW_EXACT || it.match_strategy == SGA_GW_REGEX ||
                                  it.match_strategy == SGA_GW_CONTAINS
                              ? (uint8_t)it.match_strategy
                              : (uint8_t)1;
        S = GwSlot{it.field, it.pattern_off, it.pattern_len, kGwItem, m, (uint8_t)(it.has_pattern ? 1 : 0), 0};
        winner[res[it.resource].slot_off + it.index] = (int64_t)j;
    }
    // the slot each REGEX item with a pattern decides (load_regex): -1 not such an item, -2 shadowed
    std::vector<int32_t> rslot(n_items, -1);
    for (size_t j = 0; j < n_items; ++j) {
        const sga_gateway_item &it = items[j];
        if (it.index < 0 || it.match_strategy != SGA_GW_REGEX || !it.has_pattern) continue;
        const uint32_t q = res[it.resource].slot_off + it.index;
        rslot[j] = winner[q] == (int64_t)j ? (int32_t)q : -2;
    }
    // No parse in flight reads the old table: a parse on a caller stream ends with the engine stream waiting for
    // that stream (Engine::leave_stream), so the engine stream's end is past every parse issued so far.
    SGA_HIP_CHECK(hipStreamSynchronize(s));
    max_args = 0;
    // the programs belonged to the table that goes
    d_rx.release();
    d_rx_blob.release();
    n_regex_slots = 0;
    slots0.clear();
    regex_slot.clear();
    if (!most) {
        d_res.release();
        d_slot.release();
        d_pat.release();
        return SGA_OK;
    }
    d_res.alloc(nres_now);
    d_slot.alloc(total);
    d_pat.alloc(std::max<size_t>(blob_len, 4));
    SGA_HIP_CHECK(hipMemcpyAsync(d_res.p, res.data(), res.size() * sizeof(GwRes), hipMemcpyHostToDevice, s));
    SGA_HIP_CHECK(hipMemcpyAsync(d_slot.p, slots.data(), slots.size() * sizeof(GwSlot), hipMemcpyHostToDevice, s));
    if (blob_len) SGA_HIP_CHECK(hipMemcpyAsync(d_pat.p, blob, blob_len, hipMemcpyHostToDevice, s));
    SGA_HIP_CHECK(hipStreamSynchronize(s));
    nres = nres_now;
    n_fields = nf;
    max_args = most;
    key_nm = gateway_string_key((const uint8_t *)"$NM", 3);
    key_d = gateway_string_key((const uint8_t *)"$D", 2);
    slots0 = std::move(slots);
    regex_slot = std::move(rslot);
    return SGA_OK;
}

int GatewayEngine::load_regex(const sga_gateway_regex *programs, size_t n_programs, const uint8_t *blob,
                              size_t blob_len, hipStream_t s) {
    if (n_programs && (!programs || !blob)) return SGA_EINVAL;
    if (blob_len > 0xFFFFFFFFull) return SGA_EINVAL;  // the offsets are 32 bits
    std::vector<GwSlot> slots = slots0;
    std::vector<GwRegex> recs;
    std::map<std::array<uint32_t, 5>, uint32_t> seen;  // slices already checked -> their record
    for (size_t j = 0; j < n_programs; ++j) {
        const sga_gateway_regex &P = programs[j];
        if (P.item >= regex_slot.size() || regex_slot[P.item] == -1) return SGA_EINVAL;
        if (P.n_states < 2 || P.n_states > 65535 || P.n_classes < 1 || P.n_classes > 256) return SGA_EINVAL;
        const uint64_t nt = (uint64_t)P.n_states * P.n_classes, na = (P.n_states + 7) / 8;
        if ((uint64_t)P.class_off + 256 > blob_len || (uint64_t)P.trans_off + 2 * nt > blob_len ||
            (uint64_t)P.accept_off + na > blob_len || (P.trans_off & 1u))
            return SGA_EINVAL;
        const std::array<uint32_t, 5> key{P.n_states, P.n_classes, P.class_off, P.trans_off, P.accept_off};
        auto it = seen.find(key);
        if (it == seen.end()) {
            for (uint32_t b = 0; b < 256; ++b)
                if (blob[P.class_off + b] >= P.n_classes) return SGA_EINVAL;
            for (uint64_t q = 0; q < nt; ++q) {
                uint16_t to;
                std::memcpy(&to, blob + P.trans_off + 2 * q, 2);
                if (to >= P.n_states || (q < P.n_classes && to != 0)) return SGA_EINVAL;  // row 0 is dead
            }
            if (blob[P.accept_off] & 1u) return SGA_EINVAL;  // state 0 accepts nothing
            it = seen.emplace(key, (uint32_t)recs.size()).first;
            recs.push_back(GwRegex{P.class_off, P.trans_off, P.accept_off, P.n_classes});
        }
        if (regex_slot[P.item] < 0) continue;  // shadowed: checked, decides nothing
        GwSlot &S = slots[(size_t)regex_slot[P.item]];
        S.program = 1;
        S.pat_off = it->second;
    }
    uint32_t count = 0;
    for (const GwSlot &S : slots) count += S.program;
    // as in load(): the engine stream's end is past every parse issued so far
    SGA_HIP_CHECK(hipStreamSynchronize(s));
    if (!count) {
        if (d_rx.p && d_slot.p)
            SGA_HIP_CHECK(hipMemcpyAsync(d_slot.p, slots0.data(), slots0.size() * sizeof(GwSlot), hipMemcpyHostToDevice, s));
        SGA_HIP_CHECK(hipStreamSynchronize(s));
        d_rx.release();
        d_rx_blob.release();
        n_regex_slots = 0;
        return SGA_OK;
    }
    d_rx.alloc(recs.size());
    d_rx_blob.alloc(std::max<size_t>(blob_len, 4));
    SGA_HIP_CHECK(hipMemcpyAsync(d_rx.p, recs.data(), recs.size() * sizeof(GwRegex), hipMemcpyHostToDevice, s));
    SGA_HIP_CHECK(hipMemcpyAsync(d_rx_blob.p, blob, blob_len, hipMemcpyHostToDevice, s));
    SGA_HIP_CHECK(hipMemcpyAsync(d_slot.p, slots.data(), slots.size() * sizeof(GwSlot), hipMemcpyHostToDevice, s));
    SGA_HIP_CHECK(hipStreamSynchronize(s));
    n_regex_slots = count;
    return SGA_OK;
}

void GatewayEngine::launch(const uint32_t *d_resource, const uint8_t *d_mode, const uint32_t *d_field_off,
                           const uint32_t *d_field_len, const uint8_t *d_bytes, uint64_t n_bytes,
                           const uint64_t *d_regex_bits, uint32_t n, uint8_t *d_flags, uint64_t *d_param,
                           uint64_t *d_values, uint64_t n_values, uint64_t value_base, uint64_t bias,
                           uint32_t *d_status, hipStream_t s) const {
    const uint64_t lanes = (uint64_t)n * max_args;
    hipLaunchKernelGGL(k_gateway_parse, dim3((unsigned)((lanes + kT - 1) / kT)), dim3(kT), 0, s, table(), d_resource,
                       d_mode, d_field_off, d_field_len, d_bytes, n_bytes, d_regex_bits, n, d_flags, d_param, d_values,
                       n_values, value_base, bias, d_status);
    SGA_HIP_CHECK(hipGetLastError());
}

int GatewayEngine::parse_host(const uint32_t *resource, const uint8_t *mode, const uint32_t *field_off,
                              const uint32_t *field_len, const uint8_t *bytes, size_t n_bytes,
                              const uint64_t *regex_bits, size_t n, uint8_t *flags, uint64_t *param, uint64_t *values,
                              size_t n_values, size_t value_base, size_t max_batch, hipStream_t s) {
    if (!loaded() || n == 0) return SGA_OK;
    const size_t cap = std::min(n, max_batch), stride = 2 * (size_t)max_args;
    if (h_res.n < cap) {
        h_res.alloc(cap);
        h_mode.alloc(cap);
        h_flags.alloc(cap);
        h_regex.alloc(cap);
        h_param.alloc(cap);
    }
    if (h_foff.n < cap * n_fields) {
        h_foff.alloc(cap * n_fields);
        h_flen.alloc(cap * n_fields);
    }
    if (h_values.n < cap * stride) h_values.alloc(cap * stride);
    if (h_bytes.n < std::max<size_t>(n_bytes, 4)) h_bytes.alloc(std::max<size_t>(n_bytes, 4));
    if (!h_status.p) h_status.alloc(1);
    SGA_HIP_CHECK(hipMemsetAsync(h_status.p, 0, 4, s));
    if (n_bytes) SGA_HIP_CHECK(hipMemcpyAsync(h_bytes.p, bytes, n_bytes, hipMemcpyHostToDevice, s));
    for (size_t b = 0; b < n; b += cap) {
        const size_t m = std::min(cap, n - b);
        // the chunk's vectors go to values[value_base + b * stride ..): the room left there, capped at the staging
        const size_t base = value_base + b * stride;
        const size_t room = n_values > base ? std::min(n_values - base, m * stride) : 0;
        SGA_HIP_CHECK(hipMemcpyAsync(h_res.p, resource + b, m * 4, hipMemcpyHostToDevice, s));
        SGA_HIP_CHECK(hipMemcpyAsync(h_mode.p, mode + b, m, hipMemcpyHostToDevice, s));
        SGA_HIP_CHECK(hipMemcpyAsync(h_flags.p, flags + b, m, hipMemcpyHostToDevice, s));
        SGA_HIP_CHECK(hipMemcpyAsync(h_param.p, param + b, m * 8, hipMemcpyHostToDevice, s));
        SGA_HIP_CHECK(hipMemcpyAsync(h_foff.p, field_off + b * n_fields, m * n_fields * 4, hipMemcpyHostToDevice, s));
        SGA_HIP_CHECK(hipMemcpyAsync(h_flen.p, field_len + b * n_fields, m * n_fields * 4, hipMemcpyHostToDevice, s));
        if (regex_bits) SGA_HIP_CHECK(hipMemcpyAsync(h_regex.p, regex_bits + b, m * 8, hipMemcpyHostToDevice, s));
        // the words nobody writes (shorter vectors, events of other resources) go back as the caller had them,
        // as the device form leaves them
        if (room) SGA_HIP_CHECK(hipMemcpyAsync(h_values.p, values + base, room * 8, hipMemcpyHostToDevice, s));
        launch(h_res.p, h_mode.p, h_foff.p, h_flen.p, h_bytes.p, n_bytes, regex_bits ? h_regex.p : nullptr, (uint32_t)m,
               h_flags.p, h_param.p, h_values.p, n_values, base, base, h_status.p, s);
        SGA_HIP_CHECK(hipMemcpyAsync(flags + b, h_flags.p, m, hipMemcpyDeviceToHost, s));
        SGA_HIP_CHECK(hipMemcpyAsync(param + b, h_param.p, m * 8, hipMemcpyDeviceToHost, s));
        if (room) SGA_HIP_CHECK(hipMemcpyAsync(values + base, h_values.p, room * 8, hipMemcpyDeviceToHost, s));
        SGA_HIP_CHECK(hipStreamSynchronize(s));
    }
    uint32_t st = 0;
    SGA_HIP_CHECK(hipMemcpy(&st, h_status.p, 4, hipMemcpyDeviceToHost));
    return st ? SGA_EINVAL : SGA_OK;
}

}  // namespace sga
