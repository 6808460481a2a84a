// Gateway flow rules: request fields -> SGA_EV_ARGS argument vectors on the device (sga_gateway_*).
// GW = sentinel-adapter/sentinel-api-gateway-adapter-common/src/main/java/com/alibaba/csp/sentinel/adapter/
// gateway/common.  GatewayParamParser.parseParameterFor (GW/param/GatewayParamParser.java:51-174) restated over a
// table the host built from the loaded GatewayFlowRules (sentinel_amd/gateway.py).
#pragma once
#include "../../include/sentinel_amd.h"
#include "common.hpp"

#include <vector>

namespace sga {

// ---- XXH64 (the public xxHash specification), seed SGA_GW_SEED.  Rd reads little-endian words at a byte
// offset of the string: the host passes a memcpy reader, the kernel one that assembles aligned dwords.
constexpr uint64_t kXP1 = 0x9E3779B185EBCA87ull, kXP2 = 0xC2B2AE3D27D4EB4Full, kXP3 = 0x165667B19E3779F9ull,
                   kXP4 = 0x85EBCA77C2B2AE63ull, kXP5 = 0x27D4EB2F165667C5ull;
SGA_HD uint64_t xrotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
SGA_HD uint64_t xround(uint64_t acc, uint64_t in) { return xrotl(acc + in * kXP2, 31) * kXP1; }
SGA_HD uint64_t xmerge(uint64_t h, uint64_t v) { return (h ^ xround(0, v)) * kXP1 + kXP4; }

template <class Rd>
SGA_HD uint64_t xxh64(const Rd &rd, uint32_t len, uint64_t seed) {
    uint32_t p = 0;
    uint64_t h;
    if (len >= 32) {
        uint64_t v1 = seed + kXP1 + kXP2, v2 = seed + kXP2, v3 = seed, v4 = seed - kXP1;
        for (; p + 32 <= len; p += 32) {
            v1 = xround(v1, rd.u64(p));
            v2 = xround(v2, rd.u64(p + 8));
            v3 = xround(v3, rd.u64(p + 16));
            v4 = xround(v4, rd.u64(p + 24));
        }
        h = xrotl(v1, 1) + xrotl(v2, 7) + xrotl(v3, 12) + xrotl(v4, 18);
        h = xmerge(xmerge(xmerge(xmerge(h, v1), v2), v3), v4);
    } else {
        h = seed + kXP5;
    }
    h += len;
    for (; p + 8 <= len; p += 8) h = xrotl(h ^ xround(0, rd.u64(p)), 27) * kXP1 + kXP4;
    if (p + 4 <= len) {
        h = xrotl(h ^ ((uint64_t)rd.u32(p) * kXP1), 23) * kXP2 + kXP3;
        p += 4;
    }
    for (; p < len; ++p) h = xrotl(h ^ ((uint64_t)rd.u8(p) * kXP5), 11) * kXP1;
    h ^= h >> 33;
    h *= kXP2;
    h ^= h >> 29;
    h *= kXP3;
    h ^= h >> 32;
    return h;
}

uint64_t gateway_string_key(const uint8_t *bytes, size_t len);  // host

// Per resource: its argument slots are slot[slot_off .. slot_off + nargs); the last one is "$D" when the resource
// has a rule without a paramItem.  nargs == 0: no gateway rule, its events are left alone.  mode_min / mode_max:
// over the rules with a paramItem (min > max: none) -- parseParameterFor answers [] unless every one equals the
// request's mode.
struct GwRes {
    uint32_t slot_off, nargs;
    int32_t mode_min, mode_max;
};
enum : uint8_t { kGwItem = 0, kGwNull = 1, kGwDefault = 2 };
// One argument slot: the item that writes it (the last in load order among those sharing the index), none
// (kGwNull: the slot stays null), or the "$D" constant (kGwDefault).  program != 0: a REGEX slot decided on the
// device; pat_off is then its index into GwTable::rx (the kernel never reads a REGEX slot's pattern bytes).
struct GwSlot {
    uint32_t field, pat_off, pat_len;
    uint8_t kind, match, has_pattern, program;
};
// One REGEX program (sga_gateway_regex, checked by GatewayEngine::load_regex): byte offsets into GwTable::rx_blob of
// the 256-byte class map, the n_states x n_classes uint16 transitions (even) and the accept bits.
struct GwRegex {
    uint32_t class_off, trans_off, accept_off, n_classes;
};
struct GwTable {
    const GwRes *res;
    const GwSlot *slot;
    const uint8_t *pat;
    uint32_t nres, n_fields, max_args;
    uint64_t key_nm, key_d;  // "$NM", "$D"
    const GwRegex *rx;       // null unless programs are loaded
    const uint8_t *rx_blob;
};

struct GatewayEngine {
    DevBuf<GwRes> d_res;
    DevBuf<GwSlot> d_slot;
    DevBuf<uint8_t> d_pat;
    uint32_t nres = 0, n_fields = 0, max_args = 0;
    uint64_t key_nm = 0, key_d = 0;
    bool loaded() const { return max_args != 0; }
    GwTable table() const {
        return GwTable{d_res.p, d_slot.p, d_pat.p, nres, n_fields, max_args, key_nm, key_d, d_rx.p, d_rx_blob.p};
    }
    int load(const sga_gateway_item *items, size_t n_items, const uint8_t *blob, size_t blob_len, uint32_t n_fields,
             uint32_t nres, hipStream_t s, std::string *err);
    // REGEX programs of the loaded table (sga_gateway_load_regex).  The host keeps the slots as load() made them
    // and, per item, the slot it won if it is a REGEX item with a pattern (-1 otherwise): attaching programs patches
    // a copy and uploads it, dropping them uploads the original.
    DevBuf<GwRegex> d_rx;
    DevBuf<uint8_t> d_rx_blob;
    std::vector<GwSlot> slots0;
    std::vector<int32_t> regex_slot;  // per item of the last load; -2: a REGEX item a later item shadows
    uint32_t n_regex_slots = 0;
    int load_regex(const sga_gateway_regex *programs, size_t n_programs, const uint8_t *blob, size_t blob_len,
                   hipStream_t s);
    // one launch over n events x max_args slots; status: a device word, bit 0 set for a refused event; bias: the
    // offset d_values[0] has in the caller's numbering (0 unless d_values is a chunk's staging buffer)
    void launch(const uint32_t *d_resource, const uint8_t *d_mode, const uint32_t *d_field_off,
                const uint32_t *d_field_len, const uint8_t *d_bytes, uint64_t n_bytes, const uint64_t *d_regex_bits,
                uint32_t n, uint8_t *d_flags, uint64_t *d_param, uint64_t *d_values, uint64_t n_values,
                uint64_t value_base, uint64_t bias, uint32_t *d_status, hipStream_t s) const;
    // host form: staging
    DevBuf<uint32_t> h_res, h_foff, h_flen, h_status;
    DevBuf<uint8_t> h_mode, h_bytes, h_flags;
    DevBuf<uint64_t> h_regex, h_param, h_values;
    int parse_host(const uint32_t *resource, const uint8_t *mode, const uint32_t *field_off, const uint32_t *field_len,
                   const uint8_t *bytes, size_t n_bytes, const uint64_t *regex_bits, size_t n, uint8_t *flags,
                   uint64_t *param, uint64_t *values, size_t n_values, size_t value_base, size_t max_batch,
                   hipStream_t s);
};

}  // namespace sga
