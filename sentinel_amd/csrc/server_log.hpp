// Token server log (ClusterServerStatLogUtil -> StatLogger "sentinel-cluster-server-record"): the per-second sums
// of sentinel-server.log kept on the device (sga_server_log_enable / sga_server_log_drain).
#pragma once
#include "../../include/sentinel_amd.h"
#include "cluster.hpp"
#include "common.hpp"
#include "concurrent.hpp"

namespace sga {

// An open-addressing table of sga_server_log_row in HBM, one row per (time_slot, flow_id, kind, tag).  hash[s] is
// the slot's claim word -- a 64-bit mix of the whole tuple, never 0 (0: empty) -- and the only thing a lookup
// compares: tuples whose hashes collide share a row.  A slot is claimed by one compare-and-swap; the winner stores
// the key fields, everybody adds count and events with integer atomics, and nobody ever waits for another wave
// (the block log's scheme, flow.hpp BlogTab).
struct SlogTab {
    unsigned long long *hash;
    sga_server_log_row *row;
    unsigned long long *ctl;  // [0] lost_events [1] lost_count [2] rows claimed in the live table
    uint32_t mask;
};
constexpr uint32_t kSlogProbe = 128;  // linear probes before a tuple counts as lost

// Which checker decided the batch: the tuple a status forms depends on it
enum : int { kSlogDefault = 0, kSlogSimple = 1, kSlogParam = 2 };

// What a batch hands to the pass beside its requests: the parameter entry's value lists and the position of the
// blocking value in each (null off that entry; bpos null: position 0), and a device word whose masked bits mean the
// batch failed (null: none) -- the pass then adds nothing.
struct SlogBatch {
    const uint32_t *voff = nullptr;
    const int64_t *values = nullptr;
    const uint32_t *bpos = nullptr;
    const uint32_t *fail = nullptr;
    uint32_t fail_mask = 0;
};

// What a concurrency chunk hands to its pass (k_slog_conc): the staged operations, their results, and where a
// release finds its token's node -- aux[i] is the entry k_conc_classify found, a tombstone of the current epoch once
// k_conc_runs answered RELEASE_OK.
struct SlogConc {
    const uint8_t *op;
    const int64_t *id;
    const int32_t *acquire;
    const int64_t *ts;
    const sga_concurrent_result *res;
    const uint32_t *aux;
    const TokenEntry *tok;
    uint32_t tmask;
};

struct ServerLog {
    bool on = false;
    uint32_t slots = 0;
    int live = 0;
    DevBuf<unsigned long long> hash[2];
    DevBuf<sga_server_log_row> row[2], out;
    DevBuf<unsigned long long> ctl;
    DevBuf<uint32_t> cnt;
    SlogTab tab(int which) const { return SlogTab{hash[which].p, row[which].p, ctl.p, slots - 1}; }

    int enable(uint32_t max_rows, hipStream_t stream);
    // The last kernel of a token batch, on the batch's stream.  Nothing when the log is off.
    void pass(const ReqIn &in, int64_t ts_base, uint32_t n, int checker, const void *results, const SlogBatch &b,
              hipStream_t s);
    // The last kernel of a concurrency chunk, behind k_conc_runs on the engine stream.  Nothing when the log is off.
    void pass_conc(const SlogConc &c, uint32_t n, hipStream_t s);
    int drain(int64_t before_ms, sga_server_log_row *rows, size_t cap, size_t *n, uint64_t *lost_events,
              int64_t *lost_count, hipStream_t stream);
};

}  // namespace sga
