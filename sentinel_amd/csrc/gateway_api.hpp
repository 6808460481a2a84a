// Gateway API groups: request paths -> matching ApiDefinitions -> entry lists on the device (sga_gateway_api_*).
// GW = sentinel-adapter/sentinel-api-gateway-adapter-common/src/main/java/com/alibaba/csp/sentinel/adapter/
// gateway/common.  What every adapter's filter does per request (pickMatchingApiDefinitions, then one entry per
// matching API name) restated for a batch over a table the host built from the loaded ApiDefinitions
// (sentinel_amd/gateway_api.py): a predicate is an EXACT pattern, a byte DFA in sga_gateway_regex's format (REGEX
// patterns and translated Ant patterns), or a bit the host answers.
#pragma once
#include "../../include/sentinel_amd.h"
#include "common.hpp"

#include <string>
#include <vector>

namespace sga {

constexpr uint32_t kApiMax = 4096;        // design limit: 64 bitmap words per request
constexpr uint32_t kApiHostMax = 64;      // the host word's bits
constexpr uint32_t kApiLdsBytes = 65536;  // a table blob up to this size is staged in LDS (two workgroups per CU)

// One predicate as the kernel reads it, sorted by api.  EXACT: a = pattern offset, b = its length.  DFA: a =
// n_classes, b = class_off, c = trans_off, d = accept_off.  HOST: a = the bit.
struct ApiPred {
    uint32_t api, kind, a, b, c, d;
};
struct ApiTable {
    const ApiPred *pred;
    const uint8_t *blob;
    uint32_t n_preds, n_apis, words, blob_words;  // words: u64 words per bitmap row; blob_words: dwords of the blob
};

struct GatewayApiEngine {
    DevBuf<ApiPred> d_pred;
    DevBuf<uint8_t> d_blob;
    DevBuf<uint32_t> d_api_res;
    uint32_t n_apis = 0, n_preds = 0, n_device_preds = 0, blob_words = 0;
    int cus = 0;
    bool loaded() const { return n_apis != 0; }
    uint32_t words() const { return (n_apis + 63) / 64; }
    bool in_lds() const { return (size_t)blob_words * 4 <= kApiLdsBytes; }
    ApiTable table() const { return ApiTable{d_pred.p, d_blob.p, n_preds, n_apis, words(), blob_words}; }
    int load(const sga_gateway_api_pred *preds, size_t n_preds, const uint32_t *api_resource, size_t n_apis,
             const uint8_t *blob, size_t blob_len, uint32_t nres, hipStream_t s, std::string *err);
    // one launch: n bitmap rows; status: a device word, bit 0 set for a path slice that leaves the blob
    void launch_match(const uint32_t *d_path_off, const uint32_t *d_path_len, const uint8_t *d_bytes, uint64_t n_bytes,
                      const uint64_t *d_host_bits, uint32_t n, uint64_t *d_match, uint32_t *d_status,
                      hipStream_t s) const;
    // Expansion: per-request counts and their exclusive scan (exclusive_scan_u32) into d_cnt / d_off, then the
    // scatter: entry j of the chunk goes to index j of the outputs when j < cap; src = src_base + i.
    DevBuf<uint32_t> d_cnt, d_off, d_partial;
    void ensure_scratch(size_t max_batch);
    void launch_count_scan(const uint32_t *d_route, const uint64_t *d_match, uint32_t n, hipStream_t s);
    void launch_scatter(const uint32_t *d_route, const uint64_t *d_match, uint32_t n, const uint32_t *d_field_off,
                        const uint32_t *d_field_len, uint32_t n_fields, uint64_t cap, uint32_t src_base,
                        uint32_t *d_src, uint32_t *d_pos, uint32_t *d_resource, uint8_t *d_mode,
                        uint32_t *d_field_off_out, uint32_t *d_field_len_out, uint32_t *d_total, hipStream_t s);
    // host forms: staging
    DevBuf<uint32_t> h_off, h_len, h_status, h_route, h_foff, h_flen, h_src, h_pos, h_res, h_foff_out, h_flen_out,
        h_total;
    DevBuf<uint8_t> h_bytes, h_mode;
    DevBuf<uint64_t> h_bits, h_match;
    int match_host(const uint32_t *path_off, const uint32_t *path_len, const uint8_t *bytes, size_t n_bytes,
                   const uint64_t *host_bits, size_t n, uint64_t *match, size_t max_batch, hipStream_t s);
    int expand_host(const uint32_t *route, const uint64_t *match, size_t n, const uint32_t *field_off,
                    const uint32_t *field_len, uint32_t n_fields, size_t cap, uint32_t *src, uint32_t *pos,
                    uint32_t *resource, uint8_t *mode, uint32_t *field_off_out, uint32_t *field_len_out, size_t *total,
                    size_t max_batch, hipStream_t s);
};

}  // namespace sga
