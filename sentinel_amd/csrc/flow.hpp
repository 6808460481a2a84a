// Local path (StatisticSlot + ParamFlowSlot + FlowSlot + DegradeSlot) -- device engine.
#pragma once
#include <functional>

#include "cluster.hpp"
#include "../../include/sentinel_amd.h"
#include "common.hpp"
#include "radix_sort.hpp"

#include <vector>

namespace sga {

// FlowState::overflow bits: any other bit = a parameter map filled (SGA_ENOMEM); kOvfMissingEntry = a
// parameter event of a per-value segment flow found no thread-count entry, which every such event had
// claimed before (never expected: the batch fails with SGA_EIO instead of leaving the event undecided)
constexpr uint32_t kOvfMissingEntry = 0x80000000u;
constexpr const char *kMissingEntryText =
    "parameter event without its thread-count map entry (k_pseg_key device check); the batch failed";


// ---- node record (one ClusterNode per resource), int64 words -------------------
// second window: OccupiableBucketLeapArray(2, 1000)  (StatisticNode.java:99-100)
// borrow window: FutureBucketLeapArray(2, 1000)      (OccupiableBucketLeapArray.java:33-37)
// minute window: BucketLeapArray(60, 60000)          (StatisticNode.java:106)
// MetricBucket fields: start, PASS, BLOCK, EXCEPTION, SUCCESS, RT, OCCUPIED_PASS, minRt
constexpr int kMB = 8;
enum : int { MB_START = 0, MB_PASS, MB_BLOCK, MB_EXC, MB_SUCC, MB_RT, MB_OPASS, MB_MINRT };
constexpr int kNodeSec = 0;                       // 2 x 8
constexpr int kNodeBor = kNodeSec + 2 * kMB;      // 2 x 2 (start, PASS)
constexpr int kNodeMin = kNodeBor + 4;            // 60 x 8
constexpr int kNodeThreads = kNodeMin + 60 * kMB; // curThreadNum
constexpr int kNodeLastFetch = kNodeThreads + 1;  // StatisticNode.lastFetchTime (-1 initially)
// nonzero once ClusterBuilderSlot.entry has run for the resource (its ClusterNode exists: a kind 0 / 2 / 3
// event, whatever its outcome; ClusterBuilderSlot.java:70-100).  RELATE rules on other resources read it.
constexpr int kNodeEntered = kNodeThreads + 2;
constexpr int kNodeWords = kNodeThreads + 4;      // 504 words = 4032 B (64-B aligned)

struct FlowRuleDev {    // one rater (TrafficShapingController) + its FlowRule fields
    int32_t behavior, grade;
    double count;
    int32_t max_queue, cold_factor;
    int32_t warning_token, max_token;
    double slope;
    int64_t latest_passed;   // RateLimiterController / WarmUpRateLimiterController latestPassedTime
    int64_t stored_tokens;   // WarmUpController.storedTokens
    int64_t last_filled;     // WarmUpController.lastFilledTime
    // FlowRule.clusterMode (FlowRuleChecker.passClusterCheck): the token server's rule slot for the
    // rule's flowId (-1: no such cluster rule -> NO_RULE_EXISTS), resolved on the host before a batch
    int32_t cluster, cfallback;
    int64_t cflow;
    int32_t cslot;
    // FlowRule.strategy (FlowRuleChecker.selectNodeByRequesterAndStrategy, FlowRuleChecker.java:96-116): 0 =
    // DIRECT, the rater reads the resource's own node; otherwise RELATE, refResource's dense id + 1 -- nres + 1
    // for a refResource that is no resource of the engine (its ClusterNode never exists: the rule passes), and for
    // a rule whose limitApp or CHAIN context no event can carry.  A CHAIN rule's context is not here: PairCtx::rule_ctx
    uint32_t rel;
};

struct ParamRuleDev {
    int32_t grade, behavior;
    double count;
    int32_t max_queue, burst;
    int32_t param_idx, n_hot;
    int64_t duration;
    uint32_t hot_off, id;   // id: global param-rule id (hash-table key part)
    // ParamFlowSlot.applyRealParamIdx (ParamFlowSlot.java:56-66) rewrites a negative index on the rule at
    // its first check: the index in force (kIdxUnresolved until then), kept by equal rules on reload
    int32_t idx_res;
    // ParamFlowRule.clusterMode (QPS grade): decided by the embedded server's parameter path
    int32_t cluster, cfallback;
    int32_t cpad;
    int64_t cflow;
    uint32_t cap;   // ParameterMetric: the rule's time / token CacheMap capacity, min(4000 * durationInSec, 200000)
    uint32_t pad2;
};
constexpr int32_t kIdxUnresolved = INT32_MIN;
constexpr int kMaxParamIdx = 64;  // thread-count maps exist for argument indices 0..63

struct CbDev {
    int32_t grade, min_req;
    double count, slow_ratio;
    int32_t stat_interval, state;   // state: 0 CLOSED, 1 OPEN, 2 HALF_OPEN
    int64_t recovery_ms, max_allowed_rt, next_retry;
    int64_t st_start, st_bad, st_total;  // LeapArray(1, statIntervalMs) bucket
    int64_t probe_t;  // time of the entry that moved it OPEN -> HALF_OPEN (its revoke moves it back)
};

struct ResDev {
    uint32_t rule_off, n_rules;
    uint32_t prule_off, n_prules;
    uint32_t cb_off, n_cbs;
    uint32_t fast;   // bit0: single QPS Default/WarmUp rule, no param rules, no breakers;
                     // bit1: the resource has a parameter thread-count map (sticky)
    uint32_t group;  // leader (smallest member id) of the resource's RELATE group, kNoGroup: ungrouped
};
constexpr uint32_t kNoGroup = 0xFFFFFFFFu;  // SGA_REF_NONE

// (rule, value) -> {time, tokens} for ParameterMetric rule maps; (resource, value) -> thread count
struct alignas(32) PEntry {
    uint64_t value;
    uint32_t owner;   // rule id + 1 (param maps) or resource + 1 (thread counts); 0 = empty
    uint32_t pad;
    int64_t a;        // time counter / thread count
    int64_t b;        // token counter
};
constexpr int64_t kPAbsent = INT64_MIN;

// ParameterMetric's CacheMaps (ConcurrentLinkedHashMapWrapper, strict LRU; ParameterMetric.java:37-39,95-121).
// Every key access stamps the key's map slot with ((event sequence) << 16 | element index): within an
// owner (a rule's time/token map, or a resource's thread-count map of one argument index) stamps grow
// with the access order.  An owner whose keys cannot exceed its capacity in a batch (count pass) stays in
// free mode (any kernel, sizes kept exactly); one that could is switched to LRU mode for good: its
// present keys go into a recency queue (records {value, stamp}, oldest first), its resource is decided
// in arrival order by one lane, every access appends a record, and an insert into a full map evicts the
// oldest record whose stamp still matches its key.
struct LruRec {
    uint64_t value;
    uint64_t stamp;  // the queue area's first record holds {head, tail}
};
constexpr uint64_t kNoQueue = ~0ull;        // free mode
constexpr uint32_t kNoTBase = 0xFFFFFFFFu;  // a resource without thread-count map owner slots
constexpr uint32_t kThreadMapCap = 4000;    // ParameterMetric.THREAD_COUNT_MAX_CAPACITY
constexpr uint64_t kStampMark = 1ull << 63;  // count pass: an absent key first met in this batch

// SystemRuleManager thresholds (SystemRuleManager.java:62-74) + SystemStatusListener readings
struct SysDev {
    int32_t check, load_set, cpu_set, pad;
    double load, cpu, qps;
    int64_t max_rt, max_thread;
    double cur_load, cur_cpu;
};

// Pair nodes: one StatisticNode per (resource, origin) pair (sga_flow_set_origins) and one per (resource,
// context) pair (sga_flow_set_contexts), two instances of one table behind the same kernels.
// Origin nodes are created at the pair's first entry (ClusterBuilderSlot.java:104-107) and counted by
// StatisticSlot next to the resource's ClusterNode (StatisticSlot.java:81-84, 101-104, 123-125, 160-161).
// A context's DefaultNode is created by NodeSelectorSlot.entry (NodeSelectorSlot.java:158-177), ahead of
// ClusterBuilderSlot and every check, and receives the same adds: DefaultNode's overrides (addPassRequest,
// increaseBlockQps, increaseExceptionQps, addRtAndSuccess, increaseThreadNum, decreaseThreadNum) count on the
// DefaultNode and on the ClusterNode.  An open-addressing table maps the pair to its node
// record: key[h] = (resource + 1) << 32 | id (0: empty; bit 63: a slot a refused chunk left without a
// record, matched by nobody), idx[h] = the record, born[h] = the event sequence of the pair's first kind 0 / 2 /
// 3 event (~0: reserved by a refused chunk, not created).  The context table keeps one more word per slot, parent[h]:
// the resource id of the entry that enclosed the pair's first event (context.getLastNode() when NodeSelectorSlot
// created the DefaultNode and called addChild, NodeSelectorSlot.java:158-177), SGA_PARENT_ENTRANCE for an
// outermost one and for every pair born through an entry point without a parent array.
struct PairState {
    int64_t *node;             // max_nodes records of kNodeWords words, initialised like a resource's node;
                               // null: this kind of pair is not registered
    unsigned long long *key, *born;
    uint32_t *idx;
    uint32_t *cnt;             // records handed out
    uint32_t mask, max_nodes, n_ids;
    uint32_t *parent;          // context table only (null in the origin table): the birth parent per slot
};
constexpr int kPairOrigin = 0, kPairContext = 1, kPairKinds = 2;
constexpr uint32_t kPairNone = 0xFFFFFFFFu;
constexpr unsigned long long kPairDead = 1ull << 63, kPairUnborn = ~0ull;
constexpr uint32_t kPairFull = 1, kPairBadId = 2;
// Both tables as the pair-node kernels see them.  The statistics pass sorts by one key over both: an origin
// record q sorts under q, a context record q under base1 + q (base1 = the origin table's records, 0 without
// one), an element without a node under total.
struct PairTabs {
    PairState t[kPairKinds];
    uint32_t *ctl;             // [0] this chunk's error bits (kPairFull, kPairBadId) [1] its long segments
    uint32_t base1, total;
};
// What the arrival-order replay of a pair-ruled resource needs of the chunk (FlowState::octx, the pair-node
// state pointer; device memory, rewritten per chunk): a resource with a FlowRule whose limitApp is an origin or
// "other", or whose strategy is CHAIN, is decided in arrival order as a RELATE group of its own, the rule's
// controller reading the origin node or the context's DefaultNode
// (FlowRuleChecker.selectNodeByRequesterAndStrategy, FlowRuleChecker.java:96-116, 136-166).
struct PairCtx {
    PairTabs pt;
    const uint32_t *id[kPairKinds];    // per event (null: every event has id 0)
    const uint32_t *slot[kPairKinds];  // per event: the claim pass's table slot
    const uint32_t *rule_lim;  // per rule (FlowState::rules order): SGA_LIMIT_*
    const uint32_t *rule_ctx;  // per rule: a CHAIN rule's context id (refResource), 0 for any other strategy
    const uint8_t *oruled;     // per resource: pair-ruled
    uint64_t seq_base;
};

// AuthoritySlot (sga_load_authority_rules): per resource the one AuthorityRule the reference keeps
// (AuthorityRuleManager.java:110-143) -- its strategy (kAuthNone: no rule) and its limitApp names as a slice of one
// pool of origin ids, sorted and distinct inside a slice, so AuthorityRuleChecker.passCheck's contain test is a
// binary search whatever the order the names were written in.
struct AuthRuleDev {
    uint32_t off, n;     // pool[off .. off + n)
    int32_t strategy;    // SGA_AUTHORITY_WHITE / SGA_AUTHORITY_BLACK; kAuthNone
    uint32_t pad;
};
constexpr int32_t kAuthNone = -1;
struct AuthState {
    const AuthRuleDev *rule;   // per resource
    const uint32_t *pool;
    uint32_t nres;
};

// Block log (LogSlot, sga_block_log_enable): an open-addressing table of sga_block_row in HBM, one row per
// (time_slot, resource, decision, detail, origin, tag_kind, tag).  hash[s] is the slot's claim word -- a 64-bit mix
// of the whole tuple, never 0 (0: empty) -- and the only thing a lookup compares: tuples whose hashes collide
// share a row.  A slot is claimed by one compare-and-swap; the winner stores the key fields, everybody adds count
// and events with integer atomics, and nobody ever waits for another wave.
struct BlogTab {
    unsigned long long *hash;
    sga_block_row *row;
    unsigned long long *ctl;  // [0] lost_events [1] lost_count [2] rows claimed in the live table
    uint32_t mask;
};
constexpr uint32_t kBlogProbe = 128;  // linear probes before a tuple counts as lost
constexpr uint8_t kBlogScalar = 0, kBlogList = 1;  // sga_block_row::tag_kind

// Metric extensions (StatisticSlot's callbacks, sga_metric_ext_enable).  res: one 64-byte line of eight signed sums
// per resource, in sga_metric_res_row's order (pass, pass_events, success, exits, exception, exception_events, rt_sum,
// rt_max) -- dense, so it cannot overflow and the drain is one streaming scan.  The block rows live in an
// open-addressing table claimed as the block log's is: hash[s] is a mix of (resource, origin, decision, detail),
// never 0, and the only thing a lookup compares.  Integer atomics only; nobody waits for another wave.
struct MxRes {
    long long v[8];
};
enum : int { kMxPass = 0, kMxPassEv, kMxSuccess, kMxExits, kMxExc, kMxExcEv, kMxRtSum, kMxRtMax };
struct MxTab {
    MxRes *res;
    unsigned long long *hash;
    sga_metric_block_row *row;
    unsigned long long *ctl;  // [0] lost_events [1] lost_count
    uint32_t nres, mask;
};

// Breaker events (sga_cb_events_enable): an append buffer of sga_cb_event in HBM behind one atomic counter.  The
// kernels that write a breaker's state append one record per transition (flow.hip cb_emit); a record that finds
// the buffer full only counts in ctl[1].  The header lives in device memory (rewritten when the log is enabled or
// resized and when the degrade rules are loaded); FlowState carries one pointer to it, null while the log is off.
struct CbLog {
    sga_cb_event *rec;
    unsigned long long *ctl;  // [0] records claimed (may pass cap) [1] lost
    uint32_t cap, epoch;      // epoch: sga_load_degrade_rules calls so far
};

struct FlowState {
    int64_t *node;
    FlowRuleDev *rules;
    ParamRuleDev *prules;
    const uint64_t *hot_v;
    const int32_t *hot_t;
    CbDev *cbs;
    const ResDev *res;
    PEntry *ptab;      // param time/token maps
    PEntry *ttab;      // thread-count maps
    uint32_t pmask, tmask;
    uint32_t nres;
    uint32_t has_groups;  // the loaded FlowRules couple resources (RELATE): ResDev::group is read
    uint32_t *overflow;  // set when a param table is full (bit kOvfMissingEntry: a device check failed)
    // embedded cluster token server for cluster-mode FlowRules (sga_set_cluster_server 1)
    ClusterState cst;
    int32_t cluster_on;
    int32_t lru_ps;              // k_llru_ps takes LRU-mode parameter-only resources (SGA_LRU_PS=0: k_llru)
    // device entry (sga_submit_events_device): the chunk's gate word, written by k_lgate; nullptr on
    // the host entry, which chooses the kernels itself
    const uint32_t *gate;
    // per resource: bit k set once a parameter rule with (resolved) index k was checked -- the
    // ParameterMetric thread-count map of argument k exists (ParameterMetric.initialize, :113-121)
    uint64_t *tmapmask;
    // embedded cluster server's parameter path for cluster-mode parameter rules (ctl null: no rules)
    CParamState cpst;
    // CacheMap capacity (LruRec above)
    uint64_t *pstamp, *tstamp;   // per map slot: stamp of the key's last access
    uint32_t *psize;             // per parameter-rule id: keys present in its time/token map
    uint64_t *pq;                // per parameter-rule id: LRU queue area in lpool (kNoQueue: free mode)
    const uint32_t *pcap, *pres; // per parameter-rule id: capacity, resource
    const uint32_t *tbase;       // per resource: first of its kMaxParamIdx thread-map owner slots
    const uint32_t *tres;        // per thread-slot base (tbase / kMaxParamIdx): its resource
    uint32_t *tsize;             // per thread-map owner slot: keys present
    uint64_t *tq;                // per thread-map owner slot: LRU queue area (kNoQueue: free mode)
    LruRec *lpool;
    uint64_t lpool_cap;
    unsigned long long *lcursor; // next free record of lpool
    uint32_t *pnew, *tnew;       // count pass: distinct absent keys the batch may insert, per owner
    uint8_t *lru_res;            // per resource: an owner in LRU mode (its events replay in arrival order)
    uint32_t *lru_ctl;           // [0] owners switched this batch [1] error bits (1 queue pool full, 2 queue check)
                                 // [2] events in lneed
    uint32_t *lru_list;          // owners switched this batch: param id, or kLruThread | thread slot
    uint32_t *lneed;             // count pass input: the batch's events with a key absent at its start ([2] of lru_ctl)
    uint32_t nprid, ntslot;      // parameter-rule ids, thread-map owner slots
    uint64_t seq_base;           // event sequence of the batch's first event
    const PairCtx *octx;         // null unless the loaded FlowRules hold one limited to an origin or "other", or a CHAIN one
    const CbLog *cbl;            // breaker events (null: off)
    uint64_t cbl_seq;            // the chunk's first event: events submitted since the log was enabled
};
constexpr uint32_t kLruThread = 1u << 31;

// A RateLimiter window's state-independent summary (flow.hip k_lwsum): its entries with a nonzero
// cost block while latestPassedTime L is past kmax + maxQueueingTime (kmax: the largest ts_off - cost),
// and its zero-cost entries pass with L unchanged while L - maxQueueingTime <= t0min and t0max <= L;
// n0 / a0: the entries that then pass (zero cost or acquireCount 0), their count and acquire sum; has0: any
// zero-cost entry with a positive acquireCount (t0min / t0max hold)
struct WinSum {
    int64_t kmax;
    int64_t a0;
    uint32_t t0min, t0max, n0, has0;
};

struct CbAgg {
    int64_t ws, bad, tot;  // a breaker stat window's counts: the last window's start (kCbNone: no exit), bad, total
};
struct CbTile {  // one tile of a long exit-only breaker flow (k_cbt_*)
    CbAgg agg, carry;
    int64_t first, last;  // windows
    int64_t tbad, ttot;   // k_cbt_tiles<1>: the window's counts at the tile's first tripping exit (breaker events)
    uint32_t bad;         // a window went back inside the tile
};

struct FlowScratch {
    uint32_t *keys[2];
    Payload *pay[2];
    uint32_t *ev_run, *ev_eidx;
    uint32_t *run_start, *run_end, *run_slot, *run_t0off, *run_nent, *run_cp;
    int32_t *run_amin, *run_amax;
    int64_t *run_asum;            // entries' acquire counts per run (k_lwave's saturated tail: blocks = sum - passes)
    uint64_t *run_exc, *run_exerr;
    int64_t *run_exrt, *run_exmin;
    uint32_t *run_nexit;
    uint32_t *run_f;
    uint8_t *run_mode;
    uint32_t *flow_first_run;
    uint32_t *heavy;  // flows replayed by k_lheavy (count in counters[8])
    uint32_t *pace;   // long single-rule fast-path flows decided by k_lwave (count in counters[9])
    uint32_t *lru;    // flows of resources with a map in LRU mode, replayed by k_llru (count in counters[10])
    // parameter-only resources decided per (rule, value) segment (flow.hip k_pseg_*): their flows (count in
    // counters[11]), the events as (thread-count map slot << 32 | sorted position), sorted by slot, the
    // segments' first elements (count in counters[12]), and each run's pass / block acquire sums and passes
    uint32_t *pseg;
    uint32_t *plong;  // long regular entry segments (first element, length; count in counters[14], k_pseg_long)
    uint32_t *cbf;       // the breaker-only flows that move their breaker (count in counters[13], k_cb_flows)
    int64_t *rt_sorted;  // each exit's response time at its sorted position (k_lexits; k_cb_flows reads it in order)
    // long exit-only breaker flows over the whole GPU (k_cbt_*): per taken flow its cbf index, first tile, first
    // tripping exit, state and total; per tile its flow, counts and carry; [0] flows [1] tiles
    uint32_t *cbt_flow, *cbt_off, *cbt_trip, *cbt_state, *cbt_tile, *cbt_ctl;
    CbTile *cbt;
    CbAgg *cbt_total;
    uint64_t *pel[2];
    Payload *spay;  // the per-value segments' payloads in sorted order (k_pseg_gather): one gather, then streams
    uint32_t *seg;
    int64_t *run_pa, *run_ba;
    uint32_t *run_np;
    WinSum *wsum;     // per 64-event window (j / 64) of a RateLimiter k_lwave run (k_lwsum)
    int64_t *wstate;  // per window: the state k_lwave skipped it at, or kWinWalked (flow.hip RUN_WIN)
    void *tile_agg, *tile_carry;
    uint32_t *tile_valid;
    uint32_t *counters;
    RadixScratch radix;
    size_t cap = 0;
    const uint32_t *gate = nullptr;  // as FlowState::gate
    // Events the slot chain replays with their original arguments (F_SPECIAL: kind 2 / 3 events, argument
    // vectors and Collection arguments k_lclassify could not restate as one value): their resources are
    // marked res_special[r] == epoch for this chunk and go to the per-resource replay.  ev_param: every
    // event's parameter after that restatement (what the parallel kernels read as param_in).
    uint64_t *ev_param = nullptr;
    uint32_t *res_special = nullptr;
    uint32_t epoch = 0;
    const uint8_t *in_kind = nullptr, *in_flags = nullptr;
    const uint64_t *in_param = nullptr, *pvals = nullptr;
    // every event's resource as submitted: a RELATE group's events are sorted under the group's leader, and
    // its replay takes each event's own resource from here
    const uint32_t *in_resource = nullptr;
    uint32_t *group = nullptr;  // flows of RELATE groups too long for their k_lflows lane (count in counters[15], k_lgroup)
};

void print_heavy_prof();  // SGA_HEAVY_PROF=1 diagnostics (flow.hip)

// One chunk of the local path as every host-side stage sees it (never passed to a kernel): device columns of m
// events.  flags, rt and param are never null (an absent column is a zero-filled staging buffer).
struct Chunk {
    const uint8_t *kind_in = nullptr;  // the caller's kind
    const uint8_t *kind = nullptr;     // the effective kind (AuthoritySlot), set by chunk_prologue
    const uint32_t *resource = nullptr, *ts_off = nullptr;
    int64_t ts_base = 0;
    const int32_t *acquire = nullptr;
    const uint8_t *flags = nullptr;
    const int64_t *rt = nullptr;
    const uint64_t *param = nullptr, *pvals = nullptr;  // pvals: null when no event of the chunk names a list
    const uint32_t *ids[kPairKinds] = {nullptr, nullptr};  // null: every event has id 0 of that kind
    const uint32_t *parent = nullptr;                      // enclosing resources of the DefaultNodes it creates
    int8_t *decision = nullptr;
    int32_t *wait_ms = nullptr;
    uint32_t m = 0;
    uint32_t *gate = nullptr;  // device entry: FlowEngine::d_gate; null on the host entries
    hipStream_t s = nullptr;
    bool pairs() const { return ids[0] || ids[1]; }
    bool turned() const { return kind != kind_in; }  // k_authority ran: authority_answer writes its decisions
};

struct FlowEngine {
    sga_config cfg{};
    hipStream_t stream = nullptr;
    uint32_t nres = 0;
    DevBuf<int64_t> d_node;
    DevBuf<FlowRuleDev> d_rules;
    DevBuf<ParamRuleDev> d_prules;
    DevBuf<uint64_t> d_hot_v;
    DevBuf<int32_t> d_hot_t;
    DevBuf<CbDev> d_cbs;
    DevBuf<ResDev> d_res;
    DevBuf<PEntry> d_ptab, d_ttab;
    DevBuf<uint32_t> d_overflow;
    DevBuf<uint32_t> d_keycount;
    DevBuf<uint64_t> d_tmapmask;  // FlowState::tmapmask
    DevBuf<uint32_t> d_res_special;  // FlowScratch::res_special (per resource, the chunk epoch that marked it)
    uint32_t epoch = 0;
    // CacheMap capacity (FlowState: pstamp .. seq_base)
    DevBuf<uint64_t> d_pstamp, d_tstamp, d_pq, d_tq;
    DevBuf<uint32_t> d_psize, d_pcap, d_pres, d_pnew, d_tbase, d_tres, d_tsize, d_tnew, d_lru_ctl, d_lru_list, d_lneed;
    DevBuf<uint8_t> d_lru_res;
    DevBuf<LruRec> d_lpool;
    DevBuf<unsigned long long> d_lcursor;
    std::vector<uint32_t> h_tbase;  // per resource (kNoTBase until it gets parameter rules)
    uint32_t ntbase = 0;            // resources given thread-map owner slots
    uint64_t seq = 0;               // events submitted so far (stamps)
    void lru_sync_rules();          // per-id / per-slot arrays after a parameter-rule load
    // parameter-only resources per (rule, value) segment, after k_lflows took their flows (flow.hip k_pseg_*)
    void launch_pseg(const Chunk &c, const FlowState &st, const FlowScratch &g, const Payload *pay,
                     const uint32_t *keys);
    void debug_size_check();  // SGA_SIZE_CHECK=1 diagnostics
    bool lru_counts() const { return d_psize.p && !h_prules.empty(); }  // lru_prepare launches its count pass
    void lru_prepare(const Chunk &c);  // count pass + switches, before a batch
    int lru_error(hipStream_t s);   // sticky queue errors (host wait)
    CParamState cparam_st{};      // set before each batch (the engine's cluster parameter state)
    bool has_cluster_prules = false;
    // after the count pass (which creates the cluster-mode rules' keys): the engine switches cluster
    // parameter rules past their CacheMap capacity to LRU mode and refreshes cparam_st (host wait)
    std::function<void(hipStream_t)> cparam_hook;
    // upper bounds of the keys held by the parameter / thread-count maps (exact after a count);
    // the maps are rehashed into more room before a batch could fill them past a quarter
    size_t pkeys_ub = 0, tkeys_ub = 0;
    int ensure_maps(size_t m);
    void grow_map(DevBuf<PEntry> &tab, DevBuf<uint64_t> &stamp, size_t &ub, size_t add);
    DevBuf<uint8_t> d_scratch;
    FlowScratch sc;
    size_t scratch_cap = 0;
    // host mirrors for rule reloads
    std::vector<FlowRuleDev> h_rules;
    std::vector<sga_flow_rule> h_flow_src;
    std::vector<ParamRuleDev> h_prules;
    std::vector<sga_param_rule> h_prule_src;
    std::vector<std::vector<uint64_t>> h_prule_hot_v;
    std::vector<std::vector<int32_t>> h_prule_hot_t;
    std::vector<CbDev> h_cbs;
    std::vector<sga_degrade_rule> h_cb_src;
    std::vector<ResDev> h_res;
    // RELATE groups (load_flow_rules): each resource's leader or kNoGroup; any: a launch of k_lgroup per chunk
    std::vector<uint32_t> h_group;
    bool has_groups = false;
    int group_of(uint32_t resource, uint32_t *leader) const;
    uint32_t next_prule_id = 0;
    // staging for host API
    DevBuf<uint8_t> d_kind, d_flags;
    DevBuf<uint32_t> d_resid, d_ts;
    DevBuf<int32_t> d_acq;
    DevBuf<int64_t> d_rt;
    DevBuf<uint64_t> d_param;
    DevBuf<int8_t> d_dec;
    DevBuf<int32_t> d_wait;
    DevBuf<int64_t> d_view;

    void init(const sga_config &c, hipStream_t s) {
        cfg = c;
        stream = s;
    }
    void release() { print_heavy_prof(); }
    FlowState state() const;
    // cluster-mode FlowRules: the engine's cluster state and ClusterStateManager mode, set before
    // each batch (sga_set_cluster_server); resolve_cluster fills every cluster rule's slot
    ClusterState cluster_st{};
    int32_t cluster_on = 0;
    bool has_cluster_rules = false;
    uint64_t cluster_resolved_gen = ~0ull;
    int resolve_cluster(const std::function<int32_t(int64_t)> &slot_of_flow, uint64_t gen);
    int set_resources(uint32_t n);
    // limit_app (sga_load_flow_rules_origin / _ctx): null = every rule's limitApp is "default"; chain
    // (sga_load_flow_rules_ctx): strategy 2 is valid, ref_resource its context id
    int load_flow_rules(const sga_flow_rule *r, size_t n, const uint32_t *limit_app = nullptr, bool chain = false);
    int load_param_rules(const sga_param_rule *r, size_t n);
    int load_degrade_rules(const sga_degrade_rule *r, size_t n);
    void upload_res();
    int submit(const uint8_t *kind, const uint32_t *resource, const int64_t *ts, const int32_t *acquire,
               const uint8_t *flags, const int64_t *rt, const uint64_t *param, size_t n, int8_t *decision,
               int32_t *wait_ms, const uint64_t *pvals = nullptr, size_t npvals = 0,
               const uint32_t *origin = nullptr, const uint32_t *context = nullptr, const uint32_t *parent = nullptr);
    DevBuf<uint64_t> d_pvals;  // values of Collection / array arguments (SGA_EV_PARAM_LIST)
    // The stages of a chunk, each written once for the three entries.  chunk_prologue: the
    // authority pass (the one place that decides c.kind), the pair claim (its refusal is returned), the control
    // word clears, pair_ctx, lru_prepare; small: k_lsmall decides the chunk (no dispatch counts to clear).
    // chunk_pipeline: special_scratch to k_entry_stats (gate null: k_entry_stats only when inbound); with a gate
    // it ends in chunk_seq, for the gate to choose.  chunk_seq: k_lseq.  chunk_epilogue: pair_apply
    // (seq_lane: k_oseq), then authority_answer.  host_result: the host entries' rule for the overflow word.
    int chunk_prologue(Chunk &c, bool small);
    void chunk_pipeline(const Chunk &c, bool inbound);
    void chunk_seq(const Chunk &c);
    void chunk_epilogue(const Chunk &c, bool seq_lane);
    static int host_result(uint32_t ovf);
    FlowScratch special_scratch(const Chunk &c);  // advances epoch: once per pipeline chunk, in no other lane
    // small host batches (<= kSmallEvents events, <= kSmallWords argument words, no SystemRule check): one
    // packed page-locked copy each way and one replay kernel (k_lsmall) instead of the pipeline
    static constexpr uint32_t kSmallEvents = 1024, kSmallWords = 16384;
    uint32_t small_max = kSmallEvents;  // sga_set_small_batch (0: off)
    PinnedBuf h_small;
    // c: the chunk's ids, parent, ts_base, m and stream; its columns are set here, to the packed buffer's
    int submit_small(Chunk c, const uint8_t *kind, const uint32_t *resource, const int32_t *acquire,
                     const uint8_t *flags, const int64_t *rt, const uint64_t *param, const uint32_t *ts_off,
                     int8_t *decision, int32_t *wait_ms, const uint64_t *pvals, size_t npvals);
    // the same as submit over device buffers, asynchronous on s: one chunk of n <= max_batch events
    int submit_device(const uint8_t *d_kind, const uint32_t *d_resource, int64_t ts_base, const uint32_t *d_ts_off,
                      const int32_t *d_acquire, const uint8_t *d_flags, const int64_t *d_rt_in,
                      const uint64_t *d_param_in, size_t n, const uint64_t *d_param_values, size_t n_values,
                      int8_t *d_decision, int32_t *d_wait, hipStream_t s, const uint32_t *d_origin = nullptr,
                      const uint32_t *d_context = nullptr, const uint32_t *d_parent = nullptr);
    // pair nodes (PairState): a kind is off until set_pairs, and for every call that passes no id array of it
    struct PairTable {
        uint32_t n_ids = 0, max_nodes = 0, slots = 0;
        DevBuf<int64_t> node;
        DevBuf<unsigned long long> key, born;
        DevBuf<uint32_t> idx, ids, slot;  // ids: the host entries' copy of the chunk's array
        DevBuf<uint32_t> parent, parents; // context table: the birth parent per slot; the host entries' copy of
                                          // the chunk's parent array
    } ptab[kPairKinds];
    DevBuf<uint32_t> d_pctl;   // [0] error bits [1] long segments [2 + kind] records handed out
    DevBuf<uint32_t> d_olong;
    // the statistics pass of a chunk that carries both arrays sorts two elements per event: buffers of its own,
    // twice the pipeline's (allocated once both kinds are registered)
    DevBuf<uint32_t> d_pkeys[2], d_phist[2], d_ppart;
    DevBuf<Payload> d_ppay[2];
    // FlowRules limited to an origin or "other", or of strategy CHAIN (load_flow_rules): each rule's limitApp and
    // context, the pair-ruled resources, and the chunk's PairCtx
    std::vector<uint32_t> h_rule_lim, h_rule_ctx;
    DevBuf<uint32_t> d_rule_lim, d_rule_ctx;
    DevBuf<uint8_t> d_oruled;
    DevBuf<PairCtx> d_octx;
    DevBuf<uint32_t> d_olist;  // pair_nodes_of: [0] count, then the ids
    bool has_pair_rules = false;
    void pair_ctx(const Chunk &c);  // before a chunk's decisions
    int set_pairs(int kind, uint32_t n, uint32_t max_nodes);
    PairTabs pstate() const;
    // the claim pass of a chunk (ahead of every check): the chunk's pairs find or claim their records.  Host
    // entry (gate null): waits, SGA_ENOMEM when a table is full -- the chunk's claims are then taken back.
    // c.parent (may be null): the chunk's enclosing resources; the pairs the chunk creates record theirs
    int pair_claim(const Chunk &c);
    // the statistics pass of a chunk, after its decisions (seq_lane: one lane in arrival order, small chunks)
    void pair_apply(const Chunk &c, bool seq_lane);
    int query_pair(int kind, uint32_t resource, uint32_t id, int64_t now, sga_node_view *out);
    int pair_nodes_of(int kind, uint32_t resource, uint32_t *ids, size_t cap, size_t *n);
    // sga_query_tree: k_tree_rows over the context table, rows sorted by (context, resource)
    DevBuf<sga_tree_row> d_trows;
    int query_tree(int64_t now, sga_tree_row *out, size_t cap, size_t *n_out);
    int device_status();  // sticky error of the device entry since the last call (host wait)
    int ensure_scratch();
    DevBuf<uint32_t> d_gate;  // [0] gate word of the running chunk, [1] sticky error bits
    int query(uint32_t resource, int64_t now, sga_node_view *out);
    int query_at(int64_t *nodes, uint32_t index, int64_t now, sga_node_view *out);
    // sga_query_nodes / sga_query_nodes_device: k_node_views over one table.  launch_views returns the number of
    // rows the launch can produce at most (0: nothing launched, *d_count zeroed)
    DevBuf<sga_node_row> d_rows;
    DevBuf<uint32_t> d_vlist;  // [0] the row counter, then the explicit list or the pair filter
    size_t launch_views(int table, const uint32_t *d_list, uint32_t n, int64_t now, uint32_t flags,
                        sga_node_row *d_out, uint32_t cap, uint32_t *d_count, hipStream_t s);
    int query_nodes(int table, const uint32_t *resources, size_t n, int64_t now, uint32_t flags, sga_node_row *out,
                    size_t cap, size_t *n_out);
    int cb_state(uint32_t resource, uint32_t k);
    int metrics(int64_t now, sga_metric_node *out, size_t cap, size_t *n);
    int load_system_rules(const sga_system_rule *r, size_t n);
    // AuthoritySlot.  auth_dev: rules of strategy 0 / 1 on the device (0: no chunk launches anything for the slot);
    // auth_kept: what loadAuthorityConf keeps (any strategy >= 0, one per resource).  A chunk that carries an origin
    // array runs k_authority over its events first: d_ekind takes the chunk's effective kind (the caller's, failing
    // entries turned into SGA_KIND_BLOCKED), which every later step reads in place of the caller's, d_aturned which
    // events were turned; authority_answer writes their decisions last.
    DevBuf<AuthRuleDev> d_auth_rule;
    DevBuf<uint32_t> d_auth_pool, d_auth_q[2];
    DevBuf<uint8_t> d_ekind, d_aturned;
    uint32_t auth_dev = 0, auth_kept = 0;
    AuthState auth_state() const { return AuthState{d_auth_rule.p, d_auth_pool.p, nres}; }
    int load_authority_rules(const uint32_t *resource, const int32_t *strategy, const uint32_t *list_off, size_t n,
                             const uint32_t *origin_ids);
    int authority_check(const uint32_t *resource, const uint32_t *origin, size_t n, uint8_t *pass);
    // sets c.kind: the chunk's effective kind (c.kind_in when no rule is on the device or it has no origin array)
    void authority_pass(Chunk &c);
    void authority_answer(const Chunk &c);
    // Block log (BlogTab): off until block_log_enable -- no chunk launches or allocates anything for it before.
    // Two tables: a drain moves the rows of finished seconds out and rehashes the survivors into the other one
    // (deleting in place would break probe chains).  block_log_pass is the chunk's last stage on every entry.
    struct BlockLog {
        bool on = false;
        uint32_t slots = 0;
        int live = 0;
        DevBuf<unsigned long long> hash[2], ctl;
        DevBuf<sga_block_row> row[2], out;
        DevBuf<uint32_t> cnt;
    } blog;
    BlogTab blog_tab(int which) const {
        return BlogTab{blog.hash[which].p, blog.row[which].p, blog.ctl.p, blog.slots - 1};
    }
    int block_log_enable(uint32_t max_rows);
    void block_log_pass(const Chunk &c);
    int block_log_drain(int64_t before_ms, sga_block_row *rows, size_t cap, size_t *n, uint64_t *lost_events,
                        int64_t *lost_count);
    // Metric extensions (MxTab): off until metric_ext_enable -- no chunk launches or allocates anything for them
    // before.  metric_ext_pass follows block_log_pass as the chunk's last stage on every entry; a drain copies out
    // and zeroes everything, so the block table needs no second copy.
    struct MetricExt {
        bool on = false;
        uint32_t slots = 0;
        DevBuf<MxRes> res;
        DevBuf<unsigned long long> hash, ctl;
        DevBuf<sga_metric_block_row> row, out_block;
        DevBuf<sga_metric_res_row> out_res;
        DevBuf<uint32_t> cnt;  // [0] resource rows [1] block rows of the drain under way
    } mext;
    MxTab metric_ext_tab() const {
        return MxTab{mext.res.p, mext.hash.p, mext.row.p, mext.ctl.p, nres, mext.slots - 1};
    }
    void metric_ext_collect(uint32_t counts[2], unsigned long long lost[2]);
    int metric_ext_enable(uint32_t max_block_rows);
    void metric_ext_pass(const Chunk &c);
    int metric_ext_drain(sga_metric_res_row *res_rows, size_t res_cap, size_t *n_res, sga_metric_block_row *block_rows,
                         size_t block_cap, size_t *n_block, uint64_t *lost_events, int64_t *lost_count);
    // Breaker events (CbLog): off until cb_events_enable -- no chunk launches or allocates anything for it.  The
    // deciding kernels append; the drain copies out and sorts by (seq, sub) on the host.
    struct CbEvents {
        bool on = false;
        uint32_t cap = 0, epoch = 0;
        uint64_t seq = 0;  // events submitted since the log was enabled (every entry point)
        DevBuf<sga_cb_event> rec;
        DevBuf<unsigned long long> ctl;
        DevBuf<CbLog> dev;  // FlowState::cbl
    } cbev;
    void cb_events_sync();
    int cb_events_enable(uint32_t max_events);
    int cb_events_drain(sga_cb_event *ev, size_t cap, size_t *n, uint64_t *lost);
    // per rule in device order (FlowState::rules / prules / cbs): its index in the array the loader was given
    std::vector<uint32_t> h_flow_idx, h_prule_idx, h_cb_idx;
    int block_rule_index(int8_t decision, uint32_t resource, uint32_t detail, uint32_t *index) const;
    SysDev sys{0, 0, 0, 0, 1.7976931348623157e308, 1.7976931348623157e308, 1.7976931348623157e308, INT64_MAX,
               INT64_MAX, -1.0, -1.0};
    DevBuf<sga_metric_node> d_metrics;
    DevBuf<uint32_t> d_mcount;
};

}  // namespace sga
