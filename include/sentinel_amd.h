/*
 * sentinel_amd.h -- C-ABI of the MI355X-native admission engine for Sentinel's
 * statistics-and-decision hot path.  Drop-in boundary: these are the calls a
 * JNI shim (GpuTokenService / GpuStatisticSlot / rule-manager hooks, see
 * INTEGRATION.md) binds.  Plain pointers and sizes only; every function
 * returns 0 or a negative errno-style code; no exception crosses the ABI.
 *
 * Reference interfaces replaced (paths relative to the reference root; aliases
 * CORE / CS / RLS as in SURVEY.md):
 *   sga_request_tokens*       <- TokenService.requestToken(Long, int, boolean)
 *                                CORE/cluster/TokenService.java:36 ;
 *                                DefaultTokenService.requestToken CS/flow/DefaultTokenService.java:39-50
 *   sga_load_cluster_flow_rules <- ClusterFlowRuleManager.loadRules(String, List<FlowRule>)
 *                                CS/flow/rule/ClusterFlowRuleManager.java:254-260 (apply :310-364)
 *   sga_set_namespace_limit   <- GlobalRequestLimiter.initIfAbsent / applyMaxQpsChange
 *                                CS/flow/statistic/limit/GlobalRequestLimiter.java:32-80
 *   sga_set_connected_count   <- ConnectionManager.getConnectedCount (AVG_LOCAL thresholds)
 *                                CS/flow/rule/ClusterFlowRuleManager.java:333-343
 *   sga_cluster_metric_sums   <- ClusterMetric.getSum(ClusterFlowEvent)  CS/flow/statistic/metric/ClusterMetric.java:53-62
 *   sga_load_cluster_param_rules <- ClusterParamFlowRuleManager.loadRules(String, List<ParamFlowRule>)
 *                                CS/flow/rule/ClusterParamFlowRuleManager.java:270-276 (apply :318-368)
 *   sga_request_param_tokens  <- TokenService.requestParamToken(Long, int, Collection<Object>)
 *                                CORE/cluster/TokenService.java:46 ; DefaultTokenService.requestParamToken
 *                                CS/flow/DefaultTokenService.java:52-64
 *   sga_rls_should_rate_limit <- SentinelEnvoyRlsServiceImpl.shouldRateLimit -> SimpleClusterFlowChecker
 *                                RLS/SentinelEnvoyRlsServiceImpl.java:51-134, RLS/flow/SimpleClusterFlowChecker.java:33-65
 *   sga_submit_events         <- SphU.entry(String, EntryType, int, Object...) / Entry.exit(int, Object...)
 *                                CORE/SphU.java:84-208, CORE/Entry.java:86-111 through the slot chain
 *                                StatisticSlot (CORE/slots/statistic/StatisticSlot.java:64-187) ->
 *                                ParamFlowSlot (PF/slots/block/flow/param/ParamFlowSlot.java:34-93) ->
 *                                FlowSlot (CORE/slots/block/flow/FlowSlot.java:161-189) ->
 *                                DegradeSlot (CORE/slots/block/degrade/DegradeSlot.java:41-89)
 *   sga_load_flow_rules       <- FlowRuleManager.loadRules(List<FlowRule>)  CORE/slots/block/flow/FlowRuleManager.java:125-127
 *   sga_load_param_rules      <- ParamFlowRuleManager.loadRules(List<ParamFlowRule>)  PF/slots/block/flow/param/ParamFlowRuleManager.java:52
 *   sga_load_degrade_rules    <- DegradeRuleManager.loadRules(List<DegradeRule>)  CORE/slots/block/degrade/DegradeRuleManager.java:108
 *   sga_query_node            <- Node views (ClusterNode) CORE/node/Node.java:40-203, StatisticNode.java:185-250
 *   sga_metrics_snapshot      <- StatisticNode.metrics() as polled by MetricTimerListener.run
 *                                CORE/node/StatisticNode.java:120-157, CORE/node/metric/MetricTimerListener.java:44-65
 *   sga_cluster_metric_nodes* <- ClusterMetricNodeGenerator.flowToMetricNode
 *                                CS/flow/statistic/ClusterMetricNodeGenerator.java:75-91
 */
#ifndef SENTINEL_AMD_H
#define SENTINEL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGA_ABI_VERSION 3

/* error codes (negated errno values) */
#define SGA_OK 0
#define SGA_EINVAL (-22)
#define SGA_ENOMEM (-12)
#define SGA_EIO (-5)      /* HIP/device error; sga_last_error() has the text */
#define SGA_ENODEV (-19)  /* no usable gfx950 device */
#define SGA_ERANGE (-34)  /* batch larger than the configured capacity */
#define SGA_ENOSYS (-38)  /* feature not available on this build */
#define SGA_EAGAIN (-11)  /* sga_poll: the request is not decided yet */
#define SGA_ENOENT (-2)   /* sga_query_origin_node / sga_query_context_node: the pair has no node yet */

/* TokenResultStatus codes, CORE/cluster/TokenResultStatus.java:27-60 */
#define SGA_TOKEN_BAD_REQUEST (-4)
#define SGA_TOKEN_TOO_MANY_REQUEST (-2)
#define SGA_TOKEN_FAIL (-1)
#define SGA_TOKEN_OK 0
#define SGA_TOKEN_BLOCKED 1
#define SGA_TOKEN_SHOULD_WAIT 2
#define SGA_TOKEN_NO_RULE_EXISTS 3
#define SGA_TOKEN_RELEASE_OK 6
#define SGA_TOKEN_ALREADY_RELEASE 7

/* ClusterFlowEvent ordinals, CS/flow/statistic/data/ClusterFlowEvent.java:22-52 */
#define SGA_CEV_PASS 0
#define SGA_CEV_BLOCK 1
#define SGA_CEV_PASS_REQUEST 2
#define SGA_CEV_BLOCK_REQUEST 3
#define SGA_CEV_OCCUPIED_PASS 4
#define SGA_CEV_OCCUPIED_BLOCK 5
#define SGA_CEV_WAITING 6

typedef struct sga_engine sga_engine;

typedef struct sga_config {
    int32_t device;            /* HIP device ordinal */
    uint32_t max_batch;        /* events per submit (device scratch is sized for it) */
    uint32_t max_rules;        /* initial rule-slot capacity (grows on load) */
    int32_t cold_factor;       /* csp.sentinel.flow.cold.factor, SentinelConfig.java:68 (3) */
    int32_t statistic_max_rt;  /* csp.sentinel.statistic.max.rt, SentinelConfig.java:69 (5000) */
    uint32_t max_param_keys;   /* cluster parameter flow: (rule, value) keys kept on the device
                                  (0 = 1M; at most 4M) */
    double exceed_count;       /* ServerFlowConfig.DEFAULT_EXCEED_COUNT (1.0), ServerFlowConfig.java:26 */
    double max_occupy_ratio;   /* ServerFlowConfig.DEFAULT_MAX_OCCUPY_RATIO (1.0), ServerFlowConfig.java:27 */
} sga_config;

/* Cluster flow rule = FlowRule{count, grade, strategy, clusterMode=true} +
 * ClusterFlowConfig{flowId, thresholdType, sampleCount, windowIntervalMs, resourceTimeout,
 * clientOfflineTime} (CORE/slots/block/flow/FlowRule.java:52-95,
 * CORE/slots/block/flow/ClusterFlowConfig.java:34-105). */
typedef struct sga_cluster_flow_rule {
    int64_t flow_id;
    double count;
    int32_t threshold_type;     /* ClusterRuleConstant: AVG_LOCAL = 0, GLOBAL = 1 */
    int32_t sample_count;       /* default 10 (ClusterRuleConstant.DEFAULT_CLUSTER_SAMPLE_COUNT) */
    int32_t window_interval_ms; /* default 1000 */
    int32_t grade;              /* RuleConstant.FLOW_GRADE_QPS = 1 (THREAD = 0: concurrency tokens) */
    int32_t strategy;           /* ClusterFlowConfig.strategy, NORMAL = 0 */
    int32_t reserved;
    int64_t resource_timeout_ms;     /* ClusterFlowConfig.resourceTimeout (default 2000) */
    int64_t client_offline_time_ms;  /* ClusterFlowConfig.clientOfflineTime (default 2000) */
} sga_cluster_flow_rule;

/* TokenResult as the engine writes it: 8 bytes per decision.
 * (CORE/cluster/TokenResult.java: status, remaining, waitInMs) */
typedef struct sga_token_result {
    int32_t remaining;
    int16_t wait_in_ms;
    int8_t status;
    int8_t reserved;
} sga_token_result;

void sga_config_default(sga_config *cfg);
int sga_create(const sga_config *cfg, sga_engine **out);
int sga_destroy(sga_engine *e);
const char *sga_last_error(const sga_engine *e);
int sga_abi_version(void);

/* ClusterFlowRuleManager.loadRules(namespace, rules): invalid rules dropped
 * (FlowRuleUtil.isValidRule), metrics of flowIds that stay are kept, metrics of
 * dropped flowIds removed, new flowIds get a fresh ClusterMetric. Returns the
 * number of rules applied (>= 0) or an error. */
int sga_load_cluster_flow_rules(sga_engine *e, const char *ns, const sga_cluster_flow_rule *rules, size_t n);
int sga_set_namespace_limit(sga_engine *e, const char *ns, double max_allowed_qps);
int sga_set_connected_count(sga_engine *e, const char *ns, int32_t connected);

/* Engine tuning, no reference counterpart (decisions never depend on it): the cluster token
 * path decides the requests of its hottest rules (at most 4096, each with at least `min_requests`
 * requests in the previous batch, one window length) in input order without sorting them: each
 * request's rank among its rule's requests comes from a per-segment count and a column prefix
 * (DESIGN.md section 3).  enabled = 0 sends every request through the radix sort.  Default:
 * enabled, min_requests 64. */
int sga_set_hot_rules(sga_engine *e, int32_t enabled, uint32_t min_requests);
/* Engine tuning (no reference counterpart): token batches of at most max_requests requests (capped
 * at 4096, 0 = off; default 4096) are classified and ordered by one workgroup instead of the
 * multi-launch sort pipeline -- the latency path of a single requestToken.  Decisions are the same
 * either way.  The same setting (capped at 1024) sends host chunks of local events (sga_submit_events,
 * the sga_event_* queue) of at most that many events, without inbound events under SystemRules, to one
 * replay kernel instead of the local pipeline. */
int sga_set_small_batch(sga_engine *e, uint32_t max_requests);

/* Batched DefaultTokenService.requestToken over host buffers; synchronous.
 * Requests are decided in array order as if issued one by one under a mocked
 * TimeUtil returning ts[i] (epoch ms).  Host-pinned or pageable buffers. */
int sga_request_tokens(sga_engine *e, const int64_t *flow_id, const int32_t *acquire, const uint8_t *prioritized,
                       const int64_t *ts, size_t n, sga_token_result *out);

/* Engine tuning (no reference counterpart): page-lock a long-lived host buffer of the caller (a front
 * end's request / result pool) for this engine's DMA.  sga_request_tokens batches of at least 2^20
 * requests whose arrays all lie in registered buffers are copied straight from / to them; other large
 * batches are staged through the engine's own page-locked slots by host threads.  Decisions are the
 * same either way.  Unregister before freeing the memory. */
int sga_host_register(sga_engine *e, void *ptr, size_t bytes);
int sga_host_unregister(sga_engine *e, void *ptr);

/* Coalescing queue for single requests.  TokenService.requestToken is called once per request from
 * many threads (FlowRequestProcessor.java:43 -> DefaultTokenService.requestToken,
 * CS/flow/DefaultTokenService.java:39-54); calling sga_request_tokens with n = 1 from each would
 * launch one pipeline per request.  sga_token_submit enqueues one request (lock-free, any thread)
 * and returns a ticket; sga_poll returns SGA_OK with its TokenResult once decided, SGA_EAGAIN before
 * (a poller that finds no batch running decides every queued request as one batch, so concurrent
 * callers share a launch); each ticket is polled to SGA_OK exactly once.  sga_request_token_one =
 * submit + poll until decided (the drop-in for a synchronous requestToken).  Decisions equal one
 * sga_request_tokens batch per request in ticket order.  A batch that fails answers
 * TokenResultStatus.FAIL (-1). */
int sga_token_submit(sga_engine *e, int64_t flow_id, int32_t acquire, uint8_t prioritized, int64_t ts,
                     uint64_t *ticket);
int sga_poll(sga_engine *e, uint64_t ticket, sga_token_result *out);
int sga_request_token_one(sga_engine *e, int64_t flow_id, int32_t acquire, uint8_t prioritized, int64_t ts,
                          sga_token_result *out);

/* Same over DEVICE buffers, asynchronous on `hip_stream` (NULL = engine stream).
 * Timestamps are ts_base + ts_off[i].  Inputs must stay valid until the stream
 * reaches the end of the call's work.  A caller stream first waits for all earlier engine work
 * and the engine stream then waits for the batch, so later engine calls (rule loads, other
 * batches on any stream) never overlap it. */
int sga_request_tokens_device(sga_engine *e, const int64_t *d_flow_id, const int32_t *d_acquire,
                              const uint8_t *d_prioritized, int64_t ts_base, const uint32_t *d_ts_off, size_t n,
                              sga_token_result *d_out, void *hip_stream);

/* One token request in the packed 12-byte form (SURVEY.md 8(d) E_in: flowId u32, ts offset u32,
 * acquireCount u16, flags u16): what a front end that decodes Netty frames (FlowRequestData:
 * flowId, count, priority -- CS/server/codec/data/FlowRequestDataDecoder.java:35-48) into a device
 * batch writes, for engines whose flowIds fit 32 bits.  flow_id = 0 and acquire = 0 answer
 * BAD_REQUEST as flowId <= 0 / acquireCount <= 0 do (DefaultTokenService.notValidRequest, :87-89);
 * flags bit 0 = prioritized, the other bits are reserved: a request with any of them set answers
 * BAD_REQUEST. */
typedef struct sga_token_request {
    uint32_t flow_id;
    uint32_t ts_off;   /* time = ts_base + ts_off (ms) */
    uint16_t acquire;
    uint16_t flags;
} sga_token_request;
#define SGA_REQ_PRIORITIZED 1u

/* sga_request_tokens_device over packed requests (12 B each, 4-byte aligned): same decisions as the
 * unpacked entry on the same requests (DefaultTokenService.requestToken in arrival order,
 * CS/flow/DefaultTokenService.java:39-50); the hot path reads the records directly, every other path
 * unpacks them on the device first. */
int sga_request_tokens_packed_device(sga_engine *e, const sga_token_request *d_req, int64_t ts_base, size_t n,
                                     sga_token_result *d_out, void *hip_stream);

/* Round-1 name of sga_request_tokens_device (kept for its callers): the device entry already
 * returns once the batch is queued on the engine stream, and batches run in submission order. */
int sga_request_tokens_device_async(sga_engine *e, const int64_t *d_flow_id, const int32_t *d_acquire,
                                    const uint8_t *d_prio, int64_t ts_base, const uint32_t *d_ts_off, size_t n,
                                    sga_token_result *d_out, void *hip_stream);
/* Pipelined form of sga_request_tokens_device for a stream of hot-path batches: the batch's classification
 * (key pass, count scans, sorts) starts once the inputs are ready on hip_stream, beside the previous batch's
 * decisions; decisions still run in submission order after every earlier engine call.  The outputs are
 * ready on hip_stream only after sga_stream_wait(e, hip_stream) (or sga_sync).  A batch the hot path does
 * not take runs as sga_request_tokens_device.  Same decisions as one sga_request_tokens_device per batch
 * (DefaultTokenService.requestToken in arrival order, CS/flow/DefaultTokenService.java:39-50). */
int sga_request_tokens_device_pipelined(sga_engine *e, const int64_t *d_flow_id, const int32_t *d_acquire,
                                        const uint8_t *d_prioritized, int64_t ts_base, const uint32_t *d_ts_off,
                                        size_t n, sga_token_result *d_out, void *hip_stream);
/* Make `hip_stream` wait for every queued engine batch (no host wait). */
int sga_stream_wait(sga_engine *e, void *hip_stream);
/* Host wait for every queued batch. */
int sga_sync(sga_engine *e);

/* ClusterMetric.getSum(event) for every ClusterFlowEvent at virtual time `now`
 * (rotation side effects included, as in the reference). out[7]. */
int sga_cluster_metric_sums(sga_engine *e, int64_t flow_id, int64_t now, int64_t *out7);

/* Cluster parameter flow rule = ParamFlowRule{count, grade, paramIdx, burstCount, controlBehavior,
 * durationInSec, maxQueueingTimeMs, parsed hot items, clusterMode=true} + ParamFlowClusterConfig
 * {flowId, thresholdType, sampleCount, windowIntervalMs}
 * (PF/slots/block/flow/param/ParamFlowRule.java:45-83, ParamFlowClusterConfig.java:32-44).
 * Fields other than flow_id / count / threshold_type / window geometry / hot items only take part
 * in ParamFlowRuleUtil.isValidRule (PF/.../ParamFlowRuleUtil.java:46-70). */
typedef struct sga_cluster_param_rule {
    int64_t flow_id;
    double count;
    int32_t threshold_type;       /* AVG_LOCAL = 0 (ParamFlowClusterConfig default), GLOBAL = 1 */
    int32_t sample_count;         /* default 10 */
    int32_t window_interval_ms;   /* default 1000 */
    int32_t grade;                /* QPS = 1 */
    int32_t burst_count;          /* default 0 */
    int32_t control_behavior;     /* default 0 */
    int32_t max_queueing_time_ms; /* default 0 */
    int32_t param_idx_set;        /* paramIdx != null */
    int64_t duration_in_sec;      /* default 1 */
    int32_t n_hot;                /* parsed hot items (value -> count), later entries win */
    int32_t reserved;
    const int64_t *hot_values;
    const int32_t *hot_counts;
} sga_cluster_param_rule;

/* ClusterParamFlowRuleManager.loadRules(namespace, rules)  CS/flow/rule/ClusterParamFlowRuleManager.java:270-368:
 * invalid rules dropped, metrics of flowIds that stay are kept (geometry fixed at creation), metrics
 * of dropped flowIds removed.  Returns the number of rules applied or an error. */
int sga_load_cluster_param_rules(sga_engine *e, const char *ns, const sga_cluster_param_rule *rules, size_t n);

/* Batched DefaultTokenService.requestParamToken(flowId, acquireCount, params)
 * (CS/flow/DefaultTokenService.java:52-64 -> ClusterParamFlowChecker.acquireClusterToken):
 * request i carries the parameter values values[value_offsets[i] .. value_offsets[i+1]) (Java
 * Objects as 64-bit values: the caller maps each parameter to a stable int64, e.g. the long value
 * or a 64-bit hash of a String).  Decided in array order under a mocked clock ts[i].  Host buffers,
 * synchronous.  -ENOMEM when the device key store (sga_config.max_param_keys) is exhausted. */
int sga_request_param_tokens(sga_engine *e, const int64_t *flow_id, const int32_t *acquire,
                             const uint32_t *value_offsets, const int64_t *values, const int64_t *ts, size_t n,
                             sga_token_result *out);

/* Each bucket map's capacity of the ClusterParamMetrics created from now on (the maxCapacity argument of
 * ClusterParamMetric(sampleCount, intervalInMs, maxCapacity), ClusterParamMetric.java:44-49; 0 restores
 * DEFAULT_CLUSTER_MAX_CAPACITY = 4000).  Existing metrics keep theirs.  A map at capacity evicts its least
 * recently accessed value (getSum's get and addValue's putIfAbsent are accesses). */
int sga_cluster_set_param_capacity(sga_engine *e, uint32_t capacity);

/* ClusterParamMetric.getSum(value) of a flow at `now` (rotation side effect included; the gets are
 * accesses in LRU order). */
int sga_cluster_param_sum(sga_engine *e, int64_t flow_id, int64_t value, int64_t now, int64_t *out);

/* ClusterParamMetric.getTopValues(number) of a param flow at `now` (rotation side effect included):
 * up to `number` (1..1024) values with the largest sums over the valid buckets, as value keys and
 * qps = sum / intervalInSecond, largest first (equal sums: smaller value key first; the reference's
 * order among equal sums is its HashMap's).  *n_out = 0 when the flow has no metric. */
int sga_cluster_param_top_values(sga_engine *e, int64_t flow_id, int64_t now, uint32_t number, int64_t *values,
                                 double *qps, uint32_t *n_out);

/* Number of flow slots and device bytes of window state (for roofline tools). */
int sga_cluster_stats(sga_engine *e, uint64_t *n_active_rules, uint64_t *state_bytes);
/* Host-side event routing for a node of G engines (no reference
 * counterpart -- the reference runs one token server): order[] receives the request indices of a
 * global batch grouped by shard = splitmix64(flowId) mod G, arrival order kept inside a shard (a
 * stable counting sort); shard g's requests are order[shard_off[g] .. shard_off[g + 1]).
 * n_threads host threads (slices counted in parallel, one offset scan).  n < 2^32. */
int sga_route_shards(const int64_t *flow_id, size_t n, uint32_t n_shards, uint32_t n_threads, uint32_t *order,
                     uint64_t *shard_off);

/* Diagnostics of the last token batch (no reference counterpart): out[0] 1 when it ran the hot
 * path, [1] fallback flags, [2] sorted elements, [3] cold elements, [4] prioritized hot requests,
 * [5] hot rules for the next batch, [6..7] first / last hot bucket delta, [8] hot runs that
 * needed a replay (always 0), [9] in-segment bucket boundaries, [10] 1 when the device passed the
 * LDS lane-order probe the hot path's ranking relies on (else the hot path stays off).
 * Synchronous. */
int sga_cluster_batch_info(sga_engine *e, uint32_t *out, size_t n);

/* ---------------------------------------------------------------------------
 * Cluster concurrency tokens: TokenService.requestConcurrentToken / releaseConcurrentToken
 * (CORE/cluster/TokenService.java:58-73) -> DefaultTokenService.java:67-86 ->
 * ConcurrentClusterFlowChecker.java:37-104, TokenCacheNodeManager, CurrentConcurrencyManager,
 * RegularExpireStrategy.java:78-134 (CS = sentinel-cluster-server-default/.../cluster).
 * Client addresses are dense ids of a host table (SGA_CLIENT_NONE = null or "").
 * ------------------------------------------------------------------------- */
#define SGA_CONCURRENT_ACQUIRE 0
#define SGA_CONCURRENT_RELEASE 1
#define SGA_CLIENT_NONE 0xFFFFFFFFu

typedef struct sga_concurrent_result {
    int64_t token_id;  /* TokenResult.tokenId (acquire OK; 0 otherwise) */
    int32_t status;    /* TokenResultStatus: OK, BLOCKED, NO_RULE_EXISTS, BAD_REQUEST, RELEASE_OK,
                          ALREADY_RELEASE */
    int32_t reserved;
} sga_concurrent_result;

/* TokenCacheNode (TokenCacheNode.java:25-60); the timeouts are absolute, as the setters store them. */
typedef struct sga_token_cache_node {
    int64_t token_id;
    int64_t flow_id;
    int64_t client_timeout;    /* clientOfflineTime + creation time */
    int64_t resource_timeout;  /* resourceTimeout + creation time */
    int32_t acquire_count;
    uint32_t client;
} sga_token_cache_node;

/* A batch of acquire / release operations decided in arrival order.  op[i] = SGA_CONCURRENT_*;
 * acquire: id = flowId (ruleId), client[i], acquire[i], ts[i] = TimeUtil/System time of the call;
 * release: id = tokenId (client / acquire ignored).  Token ids are 64-bit values unique per engine
 * (the reference draws UUID.randomUUID().getMostSignificantBits()). */
int sga_concurrent_ops(sga_engine *e, const uint8_t *op, const uint32_t *client, const int64_t *id,
                       const int32_t *acquire, const int64_t *ts, size_t n, sga_concurrent_result *out);

/* One RegularExpireStrategy pass at `now` over every cached token.  online_bits: bit c set when
 * client c is connected (ConnectionManager.isClientOnline).  *n_removed = tokens removed. */
int sga_concurrent_expire(sga_engine *e, int64_t now, const uint32_t *online_bits, uint32_t n_clients,
                          uint64_t *n_removed);

/* CurrentConcurrencyManager.get(flowId): returns 1 and *now_calls when present, 0 when absent. */
int sga_concurrent_now_calls(sga_engine *e, int64_t flow_id, int32_t *now_calls);

/* TokenCacheNodeManager.getSize() */
int sga_concurrent_token_count(sga_engine *e, uint64_t *n);

/* TokenCacheNodeManager.getTokenCacheNode(tokenId): 1 and *out when cached, 0 when absent. */
int sga_concurrent_get_token(sga_engine *e, int64_t token_id, sga_token_cache_node *out);

/* Envoy RLS: SentinelEnvoyRlsServiceImpl.shouldRateLimit over a batch of
 * requests.  Each request has desc_count descriptors; descriptor d has flowId
 * d_flow_id (= Integer.MAX_VALUE + key.hashCode(), EnvoySentinelRuleConverter.java:67-72)
 * and hitsAddend.  Every descriptor consumes (no short-circuit).  code[r]:
 * 1 = OK, 2 = OVER_LIMIT (envoy RateLimitResponse.Code), -1 = hitsAddend < 0 (onError).
 * Optional per-descriptor outputs: desc_status = the TokenResult status of
 * SimpleClusterFlowChecker.acquireClusterToken (NO_RULE_EXISTS for an absent rule -- the
 * descriptor's Code is then OK and it carries no current_limit, :65-83) and desc_remaining =
 * TokenResult.remaining (DescriptorStatus.limit_remaining). */
int sga_rls_should_rate_limit(sga_engine *e, const uint32_t *desc_offsets, size_t n_requests,
                              const int64_t *desc_flow_id, const int32_t *hits_addend, const int64_t *ts,
                              int8_t *desc_status, int32_t *desc_remaining, int32_t *code);
/* The same over DEVICE buffers, asynchronous on `hip_stream` with the stream ordering of
 * sga_request_tokens_device: desc_offsets[n_requests + 1] (offsets[n_requests] = n_descriptors
 * <= max_batch), request times ts_base + ts_off[r].  d_desc_status / d_desc_remaining may be NULL. */
int sga_rls_should_rate_limit_device(sga_engine *e, const uint32_t *d_desc_offsets, size_t n_requests,
                                     size_t n_descriptors, const int64_t *d_desc_flow_id,
                                     const int32_t *d_hits_addend, int64_t ts_base, const uint32_t *d_ts_off,
                                     int8_t *d_desc_status, int32_t *d_desc_remaining, int32_t *d_code,
                                     void *hip_stream);

/* ---------------------------------------------------------------------------
 * Local path: resources are dense ids 0..n_resources-1 (the host keeps the
 * name table, like CtSph's chain map keys).  One ClusterNode per resource
 * (FlowRuleChecker.selectNodeByRequesterAndStrategy, FlowRuleChecker.java:96-116, 136-166: every limitApp,
 * and strategy DIRECT, RELATE or CHAIN, each through the loader that knows it).
 * Caller origins (ContextUtil.enter(name, origin)) are opt-in per engine: after
 * sga_flow_set_origins, events submitted with an origin array (sga_submit_events_origin*)
 * create and count one origin StatisticNode per (resource, origin) pair beside the
 * ClusterNode (ClusterBuilderSlot.java:104-107, StatisticSlot.java:81-84, 101-104, 123-125,
 * 160-161).  Every other call, and every engine that never registers origins, behaves as
 * without them.  FlowRules limited to one origin or to "other" (sga_load_flow_rules_origin) read the origin
 * node; a resource with such a rule is decided in arrival order by one lane, like a RELATE group.
 * Contexts (the name of ContextUtil.enter(name, origin)) are opt-in the same way and independent of origins:
 * after sga_flow_set_contexts, events submitted with a context array (sga_submit_events_ctx*) create and
 * count one DefaultNode per (resource, context) pair (NodeSelectorSlot.java:158-177; DefaultNode's overrides
 * count on it and on the ClusterNode), and a CHAIN rule (sga_load_flow_rules_ctx) reads the entry's
 * DefaultNode when its refResource is the entry's context.  Context id 0 is "no tracked context" -- the
 * default sentinel_default_context, whose DefaultNodes nobody reads: such an event creates and counts no
 * context node (a deployment that wants a rule on the default context registers that name like any other).
 * An entry under NullContext (past 2,000 context names, ContextUtil.trueEnter) skips the slot chain
 * altogether: such entries are simply never submitted.  The invocation tree is opt-in per call: events
 * submitted with a parent array (sga_submit_events_tree*) record each DefaultNode's parent at its creation, and
 * sga_query_tree answers the DefaultNodes with their edges; EntranceNodes and Constants.ROOT hold no counters of
 * their own (sums over their children, formed by the host).
 * ------------------------------------------------------------------------- */

/* Coalescing queue of single local events (SphU.entry / Entry.exit from many application threads, one
 * synchronous call each: CtSph.entryWithPriority, CORE/CtSph.java:117-168).  sga_event_submit enqueues one
 * event (lock-free, any thread; kind, flags, param as in sga_submit_events_ex, param_values holding this
 * event's argument words only, at most 64 of them -- SGA_ERANGE otherwise) and returns a ticket;
 * sga_event_poll returns SGA_OK with its decision and wait once decided, SGA_EAGAIN before (a poller that
 * finds no batch running decides every queued event as ONE batch, so concurrent callers share a launch);
 * each ticket is polled to SGA_OK exactly once.  Decisions equal one sga_submit_events_ex call per event in
 * ticket order.  A batch that fails answers decision -1 and SGA_EIO.  sga_event_one = submit + poll until
 * decided (an event with more argument words than a slot holds is decided on its own). */
int sga_event_submit(sga_engine *e, uint8_t kind, uint32_t resource, int64_t ts, int32_t acquire, uint8_t flags,
                     int64_t rt, uint64_t param, const uint64_t *param_values, size_t n_values, uint64_t *ticket);
int sga_event_poll(sga_engine *e, uint64_t ticket, int8_t *decision, int32_t *wait_ms);
int sga_event_one(sga_engine *e, uint8_t kind, uint32_t resource, int64_t ts, int32_t acquire, uint8_t flags,
                  int64_t rt, uint64_t param, const uint64_t *param_values, size_t n_values, int8_t *decision,
                  int32_t *wait_ms);
/* An event whose caller needs no decision -- Entry.exit, a block counted by a slot before the engine, a revoke
 * (kinds 1-3; an entry is refused with SGA_EINVAL) -- queued like sga_event_submit and returned at once: nobody
 * polls its ticket (written to *ticket when not NULL, ~0 for an event decided on its own), the combining round
 * that decides it frees its slot.  Ticket order holds: it is decided before every event this thread queues later,
 * and every other call on the engine (batches, queries, snapshots, rule loads) first waits for the events queued
 * before it.  A round that failed holding posted events makes the next sga_event_post return SGA_EIO. */
int sga_event_post(sga_engine *e, uint8_t kind, uint32_t resource, int64_t ts, int32_t acquire, uint8_t flags,
                   int64_t rt, uint64_t param, const uint64_t *param_values, size_t n_values, uint64_t *ticket);

/* decision codes of sga_submit_events.  wait_ms of an entry: the sleep of a pass (RateLimiter pacing,
 * SHOULD_WAIT, parameter throttle) or of SGA_PASS_WAIT; for a block, the block detail the exception
 * carries: SGA_BLOCK_FLOW the blocking FlowRule's index in the resource's rules (FlowRuleComparator
 * order), SGA_BLOCK_PARAM the ParamFlowRule's index (list order), SGA_BLOCK_DEGRADE the breaker's
 * index (DegradeRuleManager list order), SGA_BLOCK_SYSTEM the SystemRule check (SystemBlockException
 * limitType: 0 qps, 1 thread, 2 rt, 3 load, 4 cpu). */
#define SGA_PASS 0
#define SGA_BLOCK_FLOW 1     /* FlowException */
#define SGA_BLOCK_PARAM 2    /* ParamFlowException */
#define SGA_BLOCK_DEGRADE 3  /* DegradeException */
#define SGA_PASS_WAIT 4      /* PriorityWaitException: passed after wait_ms, not counted as pass */
#define SGA_BLOCK_SYSTEM 5   /* SystemBlockException (SystemSlot, inbound entries only) */
#define SGA_BLOCK_AUTHORITY 6   /* AuthorityException; wait_ms 0 */

/* event kinds: 0 entry, 1 exit of a passed entry, 2 an entry blocked by a slot outside the engine
 * (a custom slot ahead of the checks, or an AuthoritySlot the caller keeps -- the engine's own runs through
 * sga_load_authority_rules): StatisticSlot's BlockException branch only --
 * increaseBlockQps on the node and, inbound, on ENTRY_NODE (StatisticSlot.java:121-135).  Kind 2 events
 * report SGA_PASS and are decided in arrival order by one lane. */
#define SGA_KIND_ENTRY 0
#define SGA_KIND_EXIT 1
#define SGA_KIND_BLOCKED 2
/* kind 3: an entry the engine passed (decision SGA_PASS) that a slot after the engine's checks then blocked
 * (a custom slot sorted after DegradeSlot).  In the reference StatisticSlot fires those slots before its pass
 * accounting (StatisticSlot.java:71-84), so such an entry only counts a block: the revoke undoes the entry's
 * pass, thread count and parameter thread counts and counts the block (node and, inbound, ENTRY_NODE), at the
 * entry's time, with the entry's flags and arguments.  Decided in arrival order by one lane; reports SGA_PASS. */
#define SGA_KIND_REVOKE 3

/* event flags */
#define SGA_EV_PRIORITIZED 1u
#define SGA_EV_ERROR 2u      /* exit of an entry that recorded a business error (Tracer.traceEntry) */
#define SGA_EV_HAS_PARAM 4u  /* args[0] present (param field) */
#define SGA_EV_INBOUND 8u    /* EntryType.IN (on entries and their exits): Constants.ENTRY_NODE + SystemSlot */
#define SGA_EV_PARAM_LIST 16u /* with HAS_PARAM: args[0] is a Collection / array; param = offset << 32 | count
                               * into sga_submit_events_ex's param_values (every element is checked,
                               * ParamFlowChecker.passLocalCheck, and counted by ParameterMetric) */
#define SGA_EV_ARGS 32u       /* the event's whole argument vector (SphU.entry(..., Object... args)):
                               * param = offset << 32 | nargs into param_values, two words per argument:
                               * param_values[offset + 2k] = kind << 62 | list length, param_values[offset
                               * + 2k + 1] = the argument's 64-bit key (SGA_ARG_SCALAR) or the offset of its
                               * elements in param_values (SGA_ARG_LIST: a Collection / array); SGA_ARG_NULL
                               * is a null argument.  HAS_PARAM / PARAM_LIST are ignored on such events.
                               * Chunks holding them are decided in arrival order by one lane. */
#define SGA_ARG_SCALAR 0u
#define SGA_ARG_NULL 1u
#define SGA_ARG_LIST 2u

/* resource id of Constants.ENTRY_NODE ("__total_inbound_traffic__") in sga_query_node and metric rows */
#define SGA_ENTRY_NODE 0xFFFFFFFFu

/* resource id that names no resource (a RELATE rule's refResource outside the engine; "no group") */
#define SGA_REF_NONE 0xFFFFFFFFu

/* FlowRule, CORE/slots/block/flow/FlowRule.java:52-95 (limitApp default; strategy DIRECT or RELATE, the node
 * the rule's controller reads chosen as in FlowRuleChecker.java:96-116) */
typedef struct sga_flow_rule {
    uint32_t resource;
    int32_t grade;                 /* FLOW_GRADE_THREAD 0 / QPS 1 */
    double count;
    int32_t control_behavior;      /* 0 default, 1 warm up, 2 rate limiter, 3 warm up + rate limiter */
    int32_t warm_up_period_sec;    /* default 10 */
    int32_t max_queueing_time_ms;  /* default 500 */
    int32_t strategy;              /* STRATEGY_DIRECT 0 or STRATEGY_RELATE 1; STRATEGY_CHAIN 2 through
                                    * sga_load_flow_rules_ctx only (the other loaders: invalid rule, like negatives) */
    /* FlowRule.clusterMode (FlowRuleChecker.passClusterCheck, FlowRuleChecker.java:168-230): the
     * rule asks the token service; with the embedded server (sga_set_cluster_server) that is this
     * engine's cluster rules (sga_load_cluster_flow_rules, keyed by flowId) */
    int32_t cluster_mode;
    int32_t cluster_fallback;      /* ClusterFlowConfig.fallbackToLocalWhenFail (default 1) */
    int64_t cluster_flow_id;       /* ClusterFlowConfig.flowId (> 0 for a valid cluster rule) */
    int32_t cluster_sample_count;  /* ClusterFlowConfig.sampleCount / windowIntervalMs / strategy: */
    int32_t cluster_window_ms;     /*   validity only (FlowRuleUtil.checkClusterField) */
    int32_t cluster_strategy;
    /* RELATE: refResource as a dense resource id.  The rule's controller reads that resource's ClusterNode
     * (passQps / curThreadNum / occupy), the entered resource's own node still counts the pass or block.  The
     * rule passes untouched until the referenced resource has been entered once (its ClusterNode is null before:
     * FlowRuleChecker.java:86-89); an id >= n_resources (SGA_REF_NONE) names a resource that never is, so the
     * rule is valid, counted as loaded and never blocks.  A blank refResource is invalid (FlowRuleUtil.java:246-251):
     * the caller passes strategy -1.  Ignored with DIRECT.  CHAIN (sga_load_flow_rules_ctx): the context id. */
    uint32_t ref_resource;
} sga_flow_rule;

/* ParamFlowRule, PF/slots/block/flow/param/ParamFlowRule.java:45-83 */
typedef struct sga_param_rule {
    uint32_t resource;
    int32_t grade;                 /* QPS 1 / THREAD 0 */
    double count;
    int32_t control_behavior;      /* 0 token bucket, 2 throttle (RATE_LIMITER) */
    int32_t max_queueing_time_ms;  /* default 0 */
    int32_t burst_count;           /* default 0 */
    int32_t param_idx;             /* args index; negative counts from the end, fixed on the rule at its first
                                    * check (ParamFlowSlot.applyRealParamIdx, ParamFlowSlot.java:56-66);
                                    * -64 <= param_idx < 64 */
    int64_t duration_in_sec;       /* default 1 */
    uint32_t n_hot;                /* parsed hot items: value -> threshold */
    uint32_t reserved;
    const uint64_t *hot_values;
    const int32_t *hot_thresholds;
    /* ParamFlowRule.clusterMode + ParamFlowClusterConfig (ParamFlowClusterConfig.java:32-44): with the
     * embedded token server on (sga_set_cluster_server 1) a QPS rule asks this engine's cluster parameter
     * path (TokenService.requestParamToken -> ClusterParamFlowChecker) in event order: OK passes,
     * BLOCKED blocks, anything else falls back (ParamFlowChecker.passClusterCheck, :305-343) */
    int32_t cluster_mode;
    int32_t cluster_fallback;      /* fallbackToLocalWhenFail, default 0 */
    int64_t cluster_flow_id;
    int32_t cluster_sample_count;  /* validity only (ParamFlowRuleUtil.checkCluster): default 10 */
    int32_t cluster_window_ms;     /* default 1000 */
} sga_param_rule;

/* DegradeRule, CORE/slots/block/degrade/DegradeRule.java:59-84 */
typedef struct sga_degrade_rule {
    uint32_t resource;
    int32_t grade;                 /* RT 0, EXCEPTION_RATIO 1, EXCEPTION_COUNT 2 */
    double count;
    int32_t time_window;           /* seconds */
    int32_t min_request_amount;    /* default 5 */
    double slow_ratio_threshold;   /* default 1.0 */
    int32_t stat_interval_ms;      /* default 1000 */
    int32_t reserved;
} sga_degrade_rule;

/* Node view at virtual time `now` (StatisticNode getters; reads rotate windows like the reference). */
typedef struct sga_node_view {
    double pass_qps, block_qps, success_qps, exception_qps, occupied_pass_qps;
    double avg_rt, min_rt, previous_pass_qps;
    int64_t total_pass, total_block, total_success, total_exception;  /* minute window */
    int64_t cur_thread_num;
    int64_t waiting;                                                /* borrowed (occupied) tokens */
    double max_success_qps;     /* StatisticNode.maxSuccessQps (StatisticNode.java:225-230): max bucket success
                                 * of the second window (>= 1) x sampleCount / intervalInSec */
    double previous_block_qps;  /* StatisticNode.previousBlockQps (StatisticNode.java:180-182): the minute
                                 * window's previous bucket's block count */
} sga_node_view;

int sga_flow_set_resources(sga_engine *e, uint32_t n_resources);
int sga_load_flow_rules(sga_engine *e, const sga_flow_rule *rules, size_t n);
/* Resources linked by RELATE rules (a rule's resource and its refResource, transitively) form a group whose
 * events are decided in arrival order by one lane; everything else stays parallel per resource.  *leader = the
 * smallest resource id of `resource`'s group, or SGA_REF_NONE when no loaded RELATE rule couples it.  A
 * multi-GPU deployment must route a group's resources to one engine. */
int sga_flow_group_of(sga_engine *e, uint32_t resource, uint32_t *leader);
/* ClusterStateManager for the local path's cluster-mode FlowRules (FlowRuleChecker.pickClusterService):
 * 0 = neither client nor server (cluster-mode rules fall back: fallbackToLocalOrPass), 1 = embedded
 * token server -- the rule's flowId is decided by this engine's cluster path in event order
 * (DefaultTokenService.requestToken, then applyTokenResult: OK pass, SHOULD_WAIT pass after waitInMs,
 * BLOCKED block, NO_RULE_EXISTS / BAD_REQUEST / FAIL / TOO_MANY_REQUEST fall back).  A cluster
 * flowId must belong to one resource's rules, and its namespace must have no GlobalRequestLimiter
 * (-ENOSYS otherwise). */
int sga_set_cluster_server(sga_engine *e, int32_t mode);
int sga_load_param_rules(sga_engine *e, const sga_param_rule *rules, size_t n);
int sga_load_degrade_rules(sga_engine *e, const sga_degrade_rule *rules, size_t n);

/* A time-ordered stream of entries (kind 0) and exits of passed entries (kind 1),
 * decided as if SphU.entry / Entry.exit were called one by one under a mocked
 * TimeUtil returning ts[i].  acquire = batchCount; rt[i] = exit - entry time
 * (exits); param[i] = args[0] when SGA_EV_HAS_PARAM.  decision[i] / wait_ms[i]
 * for entries (exits report SGA_PASS).  Host buffers, synchronous. */
int sga_submit_events(sga_engine *e, const uint8_t *kind, const uint32_t *resource, const int64_t *ts,
                      const int32_t *acquire, const uint8_t *flags, const int64_t *rt, const uint64_t *param,
                      size_t n, int8_t *decision, int32_t *wait_ms);
/* sga_submit_events with Collection / array arguments: events flagged SGA_EV_PARAM_LIST take their
 * values from param_values[param >> 32 .. (param >> 32) + (param & 0xffffffff)). */
int sga_submit_events_ex(sga_engine *e, const uint8_t *kind, const uint32_t *resource, const int64_t *ts,
                         const int32_t *acquire, const uint8_t *flags, const int64_t *rt, const uint64_t *param,
                         size_t n, const uint64_t *param_values, size_t n_values, int8_t *decision,
                         int32_t *wait_ms);
/* sga_submit_events_ex over DEVICE buffers, asynchronous on `hip_stream` (NULL = engine stream), with
 * the stream ordering of sga_request_tokens_device.  One chunk: n <= max_batch.  Timestamps are
 * ts_base + ts_off[i]; d_flags, d_rt, d_param, d_param_values and d_wait_ms may be NULL (zeros /
 * not written).  The checks the host entry makes by scanning the events (SystemSlot or Collection
 * arguments -> arrival-order replay, inbound statistics, acquire >= 0, value ranges inside
 * param_values) run on the device; a chunk that fails them is not applied and answers -1 for
 * every event.  sga_events_device_status waits for the engine stream and reports SGA_EINVAL for
 * such a chunk or SGA_ENOMEM when a parameter map filled, since its last call. */
int sga_submit_events_device(sga_engine *e, const uint8_t *d_kind, const uint32_t *d_resource, int64_t ts_base,
                             const uint32_t *d_ts_off, const int32_t *d_acquire, const uint8_t *d_flags,
                             const int64_t *d_rt, const uint64_t *d_param, size_t n, const uint64_t *d_param_values,
                             size_t n_values, int8_t *d_decision, int32_t *d_wait_ms, void *hip_stream);
int sga_events_device_status(sga_engine *e);
int sga_query_node(sga_engine *e, uint32_t resource, int64_t now, sga_node_view *out);

/* ---- caller origins (no struct changes: new entry points only) ---- */
/* FlowRule.limitApp as an id: RuleConstant.LIMIT_APP_DEFAULT, a registered origin 1..n_origins,
 * RuleConstant.LIMIT_APP_OTHER, or a name no event can carry */
#define SGA_LIMIT_DEFAULT 0u
#define SGA_LIMIT_OTHER 0xFFFFFFFEu
#define SGA_LIMIT_UNKNOWN 0xFFFFFFFFu

/* Registers the origins (after sga_flow_set_resources, once): dense ids 1..n_origins, the host keeps the
 * names; 0 is the empty origin "".  max_origin_nodes sizes the device table of (resource, origin) node
 * records (4,032 bytes each, initialised like a resource's node; the pair table beside it stays at most half
 * full); 0 picks the default of 16,384 records (66 MB). */
int sga_flow_set_origins(sga_engine *e, uint32_t n_origins, uint32_t max_origin_nodes);

/* sga_load_flow_rules with a parallel limit_app[n] (SGA_LIMIT_*; NULL = all default, the old call).
 * FlowRuleChecker.selectNodeByRequesterAndStrategy (FlowRuleChecker.java:136-166) for an entry of origin o: a
 * rule with limit_app == o (o != 0) applies and its controller reads the pair's origin node (DIRECT) or
 * ref_resource's ClusterNode (RELATE, the null rule included); a default rule behaves as ever; an "other" rule
 * applies iff o != 0 and no rule of the resource names o (FlowRuleManager.isOtherOrigin,
 * FlowRuleManager.java:137-153), and then reads like a matching rule; every other rule does not apply to the
 * entry and no rater state is touched.  SGA_LIMIT_UNKNOWN, a name no event can carry, is valid and counted,
 * never applies and names nobody for "other".  A cluster-mode rule asks the token service whatever its
 * limit_app; only its local fallback selects a node.  Occupy and waiting counters go to the node the rule
 * selected.  An id past n_origins that is neither constant: SGA_EINVAL.  Strategy 2 (CHAIN) stays invalid here (sga_load_flow_rules_ctx).
 * A resource with a rule limited to an origin or to "other" is coupled through the ClusterNode its default
 * rules read: its events are decided in arrival order by one lane, as a RELATE group of its own
 * (sga_flow_group_of reports it).  This loader orders each resource's rules as FlowRuleComparator does
 * (FlowRuleComparator.java:30-55, a stable sort by (cluster mode, limit_app == default): non-default first,
 * cluster mode last), and a FLOW block detail is the index in that order; sga_load_flow_rules keeps the list
 * order.  A reload resets the raters and keeps the origin nodes. */
int sga_load_flow_rules_origin(sga_engine *e, const sga_flow_rule *rules, const uint32_t *limit_app, size_t n);

/* sga_submit_events_ex / sga_submit_events_device with the caller's origin per event (origin[n], NULL = the
 * old call).  Entries, exits, kind 2 and kind 3 events carry the origin of their entry, as they carry
 * SGA_EV_INBOUND.  A kind 0 / 2 / 3 event with origin != 0 on a known resource creates the pair's origin node
 * ahead of every check; the node then receives what the resource's node receives for the event: a pass adds a
 * thread and PASS, SGA_PASS_WAIT a thread only, a block BLOCK; an exit adds rt and success, releases the
 * thread and adds EXCEPTION on SGA_EV_ERROR; kind 2 adds BLOCK; kind 3 takes the pass and the thread back and
 * adds BLOCK.  An exit of a pair without a node leaves origin nodes alone.  Decisions equal those of the
 * same events without origins.  An id above n_origins refuses the whole call (SGA_EINVAL; device entry: the
 * chunk, -1 for every event).  A chunk that would need more than max_origin_nodes records is refused
 * before anything of it is applied (SGA_ENOMEM; device entry: through sga_events_device_status); the pairs it
 * named keep the records it reserved, still without a node. */
int sga_submit_events_origin(sga_engine *e, const uint8_t *kind, const uint32_t *resource, const int64_t *ts,
                             const int32_t *acquire, const uint8_t *flags, const int64_t *rt, const uint64_t *param,
                             const uint32_t *origin, size_t n, const uint64_t *param_values, size_t n_values,
                             int8_t *decision, int32_t *wait_ms);
int sga_submit_events_origin_device(sga_engine *e, const uint8_t *d_kind, const uint32_t *d_resource,
                                    int64_t ts_base, const uint32_t *d_ts_off, const int32_t *d_acquire,
                                    const uint8_t *d_flags, const int64_t *d_rt, const uint64_t *d_param,
                                    const uint32_t *d_origin, size_t n, const uint64_t *d_param_values,
                                    size_t n_values, int8_t *d_decision, int32_t *d_wait_ms, void *hip_stream);
/* The origin node's view (ClusterNode.getOriginCountMap().get(origin)); SGA_ENOENT while the pair has none. */
int sga_query_origin_node(sga_engine *e, uint32_t resource, uint32_t origin, int64_t now, sga_node_view *out);
/* The origins with a node on the resource (the keys of getOriginCountMap), in no particular order: up to
 * cap ids, *n = number written; SGA_ERANGE when there are more. */
int sga_origin_nodes_of(sga_engine *e, uint32_t resource, uint32_t *origins, size_t cap, size_t *n);

/* ---- contexts (no struct changes: new entry points only) ---- */
/* A CHAIN rule's refResource that is the name of no registered context: no event can carry it */
#define SGA_CONTEXT_UNKNOWN 0xFFFFFFFFu

/* Registers the contexts (after sga_flow_set_resources, once; independent of sga_flow_set_origins: an engine
 * may register either, both or neither): dense ids 1..n_contexts, the host keeps the names; 0 is "no tracked
 * context".  max_context_nodes sizes the device table of (resource, context) DefaultNode records, a second
 * instance of the origin table (4,032 bytes a record); 0 picks the same default of 16,384 records (66 MB),
 * a choice, not a measurement. */
int sga_flow_set_contexts(sga_engine *e, uint32_t n_contexts, uint32_t max_context_nodes);

/* sga_load_flow_rules_origin with strategy 2 (CHAIN) valid; limit_app NULL = every rule "default", legal on an
 * engine without origins.  A CHAIN rule's ref_resource is its refResource as a context id: 1..n_contexts, or
 * SGA_CONTEXT_UNKNOWN (valid, counted, keeps its place, never applies); 0 or any other id: invalid rule.
 * FlowRuleChecker.selectNodeByRequesterAndStrategy / selectReferenceNode (FlowRuleChecker.java:96-116,
 * 136-166): a CHAIN rule applies to an entry iff its limitApp test passes (the three-way test of
 * sga_load_flow_rules_origin, so a CHAIN rule limited to an origin or to "other" is legal) and its
 * refResource equals the entry's context; its controller then reads the entry's DefaultNode -- occupy and
 * waiting counters go there only, DefaultNode forwards none of them.  Otherwise the rule does not apply and
 * touches no rater state.  A cluster-mode CHAIN rule asks the token service; only its local fallback selects
 * a node.  A resource with a CHAIN rule is decided in arrival order by one lane, as a group of its own
 * (sga_flow_group_of reports it).  Rules are ordered as FlowRuleComparator does; a reload resets the raters and
 * keeps the context nodes.  sga_load_flow_rules and sga_load_flow_rules_origin keep rejecting strategy 2. */
int sga_load_flow_rules_ctx(sga_engine *e, const sga_flow_rule *rules, const uint32_t *limit_app, size_t n);

/* The _origin entries with the entry's context per event (context[n]; either array may be NULL).  A kind 0 / 2 /
 * 3 event with context != 0 on a known resource creates the pair's DefaultNode ahead of every check
 * (NodeSelectorSlot.entry runs before ClusterBuilderSlot); the node then receives exactly what the origin node
 * receives (above), so an event with an origin and a context counts on three nodes.  An exit creates nothing;
 * an exit of a pair without a node -- one that arrives ahead of the pair's first entry in the same chunk
 * included -- leaves context nodes alone.  ENTRY_NODE, breakers and parameter metrics know no context.
 * Refusals are those of the origin entries: an id above n_contexts refuses the whole call or chunk
 * (SGA_EINVAL), a full context table refuses it before anything is applied (SGA_ENOMEM), and the claims of
 * both tables are taken back.  The sga_event_* queue and the JNI shim carry context 0, as they carry origin 0. */
int sga_submit_events_ctx(sga_engine *e, const uint8_t *kind, const uint32_t *resource, const int64_t *ts,
                          const int32_t *acquire, const uint8_t *flags, const int64_t *rt, const uint64_t *param,
                          const uint32_t *origin, const uint32_t *context, size_t n, const uint64_t *param_values,
                          size_t n_values, int8_t *decision, int32_t *wait_ms);
int sga_submit_events_ctx_device(sga_engine *e, const uint8_t *d_kind, const uint32_t *d_resource, int64_t ts_base,
                                 const uint32_t *d_ts_off, const int32_t *d_acquire, const uint8_t *d_flags,
                                 const int64_t *d_rt, const uint64_t *d_param, const uint32_t *d_origin,
                                 const uint32_t *d_context, size_t n, const uint64_t *d_param_values, size_t n_values,
                                 int8_t *d_decision, int32_t *d_wait_ms, void *hip_stream);
/* The DefaultNode's view; SGA_ENOENT while the pair has none. */
int sga_query_context_node(sga_engine *e, uint32_t resource, uint32_t context, int64_t now, sga_node_view *out);
/* The contexts with a DefaultNode on the resource, in no particular order: up to cap ids, *n = number written;
 * SGA_ERANGE when there are more. */
int sga_context_nodes_of(sga_engine *e, uint32_t resource, uint32_t *contexts, size_t cap, size_t *n);

/* ---- node views in bulk (new entry points only): what the command center's clusterNode, cnode, origin and
 * systemStatus commands read ---- */
#define SGA_NODES_RESOURCE 0 /* ClusterNodes (ClusterBuilderSlot.getClusterNodeMap) and Constants.ENTRY_NODE */
#define SGA_NODES_ORIGIN   1 /* origin nodes (ClusterNode.getOriginCountMap) */
#define SGA_NODES_CONTEXT  2 /* DefaultNodes */
#define SGA_NODES_NOT_ZERO 1u /* keep the rows with total_pass + total_block > 0 (clusterNode?type=notZero) */
typedef struct sga_node_row {
    uint32_t resource, other;   /* other = origin / context id, 0 for a resource row */
    uint32_t entered, reserved; /* entered: the node exists (always 1 for a pair row) */
    sga_node_view view;
} sga_node_row;

/* sga_query_node's view of many nodes of one table at `now`, in one launch (one wave a node) and one wait.
 * resources == NULL: every node of the table -- SGA_NODES_RESOURCE: the resources ClusterBuilderSlot.entry has
 * run for, without SGA_ENTRY_NODE; a pair table: every pair with a node.  SGA_NODES_RESOURCE with a list: exactly
 * those resources, entered or not (`entered` says which; SGA_ENTRY_NODE is allowed); a pair table with a list: the
 * pairs of those resources.  Ids must be distinct and in range (SGA_EINVAL, checked before any launch).  Rows come
 * back sorted by (resource, other).  More rows than cap: SGA_ERANGE, *n_out = the number needed, the first cap
 * rows in `out` unsorted.  A pair table that was never registered: SGA_OK, 0 rows.  Every candidate node receives
 * the window rotations of sga_query_node at `now` -- also one SGA_NODES_NOT_ZERO then drops, where the reference's
 * totalRequest() rotates the minute window only; rotations at one `now` are idempotent. */
int sga_query_nodes(sga_engine *e, int table, const uint32_t *resources, size_t n, int64_t now, uint32_t flags,
                    sga_node_row *out, size_t cap, size_t *n_out);
/* Every node of the table into DEVICE memory on `hip_stream` (NULL = engine stream), no host wait: min(count,
 * cap) rows in no particular order, the full count in *d_count (uint32, device). */
int sga_query_nodes_device(sga_engine *e, int table, int64_t now, uint32_t flags, sga_node_row *d_out, size_t cap,
                           uint32_t *d_count, void *hip_stream);

/* ---- invocation tree (new entry points only): what the command center's tree and jsonTree commands read ---- */
/* "no enclosing DefaultNode": the pair hangs under its context's EntranceNode */
#define SGA_PARENT_ENTRANCE 0xFFFFFFFFu

/* The _ctx entries with the enclosing entry per event (parent[n], after context; NULL = every event is
 * outermost): parent[i] is the resource id of the entry that encloses event i in its context, or
 * SGA_PARENT_ENTRANCE.  It is the edge NodeSelectorSlot.entry takes when it creates a DefaultNode --
 * ((DefaultNode) context.getLastNode()).addChild(node), NodeSelectorSlot.java:158-177, once, at creation -- so it
 * is read only for a kind 0 / 2 / 3 event with context != 0 on a known resource, and kept only from the pair's
 * first such event in arrival order; later entries of the pair under another parent add no edge, exits ignore it.
 * On such an event an id >= n_resources that is not SGA_PARENT_ENTRANCE refuses the whole call or chunk as an
 * origin id above n_origins does (SGA_EINVAL, nothing applied, claims taken back; device entry: -1 for every event
 * and sga_events_device_status).  Decisions, waits and every node's counts equal those of the same events through
 * sga_submit_events_ctx*; a DefaultNode born through any entry point without a parent array hangs under its
 * EntranceNode. */
int sga_submit_events_tree(sga_engine *e, const uint8_t *kind, const uint32_t *resource, const int64_t *ts,
                           const int32_t *acquire, const uint8_t *flags, const int64_t *rt, const uint64_t *param,
                           const uint32_t *origin, const uint32_t *context, const uint32_t *parent, size_t n,
                           const uint64_t *param_values, size_t n_values, int8_t *decision, int32_t *wait_ms);
int sga_submit_events_tree_device(sga_engine *e, const uint8_t *d_kind, const uint32_t *d_resource, int64_t ts_base,
                                  const uint32_t *d_ts_off, const int32_t *d_acquire, const uint8_t *d_flags,
                                  const int64_t *d_rt, const uint64_t *d_param, const uint32_t *d_origin,
                                  const uint32_t *d_context, const uint32_t *d_parent, size_t n,
                                  const uint64_t *d_param_values, size_t n_values, int8_t *d_decision,
                                  int32_t *d_wait_ms, void *hip_stream);

typedef struct sga_tree_row {
    uint32_t resource, context;
    uint32_t parent;   /* the resolved edge: a resource id of the same context, or SGA_PARENT_ENTRANCE */
    uint32_t reserved;
    sga_node_view view;
} sga_tree_row;

/* One row per DefaultNode, sorted by (context, resource), in one launch (one wave a node) and one wait.  view is
 * sga_query_context_node's at `now`, with the rotations of sga_query_nodes.  parent is the birth parent's resource
 * id when the pair (parent, context) has a DefaultNode born strictly before this one, else SGA_PARENT_ENTRANCE:
 * Context.getLastNode's fallback to the EntranceNode when the enclosing entry has no node (Context.java:180-186,
 * CtEntry.java:157-159).  The rule makes the edges a forest for any input: a self-parent and a parent born later
 * both fall to the EntranceNode.  More rows than cap: SGA_ERANGE, *n_out = the number needed, the first cap rows
 * in `out` unsorted.  No contexts registered: SGA_OK, 0 rows.  EntranceNode and Constants.ROOT values are sums
 * over these rows (EntranceNode.java:45-126), formed by the host. */
int sga_query_tree(sga_engine *e, int64_t now, sga_tree_row *out, size_t cap, size_t *n_out);

/* ---- AuthoritySlot (no struct changes: new entry points only) ---- */
#define SGA_AUTHORITY_WHITE 0
#define SGA_AUTHORITY_BLACK 1

/* AuthorityRuleManager.loadAuthorityConf (AuthorityRuleManager.java:110-143) over ids.
 * n rules in CSR form: rule k is on resource[k] with strategy[k] and the origin ids
 * origin_ids[list_off[k] .. list_off[k+1]).  Ids are 1..n_origins or SGA_LIMIT_UNKNOWN (dropped); anything
 * else, a resource >= n_resources, a strategy < 0 or a decreasing list_off: SGA_EINVAL, nothing loaded.
 * The first rule of a resource wins; n == 0 clears.  Returns the number of rules kept.
 * A load replaces the whole set and touches no node and no rater.  AuthorityRuleChecker.passCheck
 * (AuthorityRuleChecker.java:30-66) then runs for every kind 0 event of every entry point that takes an origin
 * array (host and device, _origin, _ctx and _tree), after the pair nodes' claim and ahead of SystemSlot: origin 0
 * passes; SGA_AUTHORITY_BLACK blocks an origin in the list, SGA_AUTHORITY_WHITE one that is not; any other strategy
 * passes.  A blocked entry is counted exactly as a SGA_KIND_BLOCKED event of the caller's (its resource replays in
 * arrival order that chunk) and answers SGA_BLOCK_AUTHORITY, wait_ms 0.  The caller's kind array is never written.
 * Entry points without an origin array, the sga_event_* queue and the JNI shim carry origin 0: never blocked. */
int sga_load_authority_rules(sga_engine *e, const uint32_t *resource, const int32_t *strategy,
                             const uint32_t *list_off, size_t n, const uint32_t *origin_ids);

/* AuthorityRuleChecker.passCheck for n (resource, origin) pairs in one launch of the same kernel:
 * pass[i] = 1 / 0.  Touches no state.  Ids out of range: SGA_EINVAL. */
int sga_authority_check(sga_engine *e, const uint32_t *resource, const uint32_t *origin, size_t n, uint8_t *pass);

/* ---- block log (LogSlot; new entry points only) ---- */
/* LogSlot (CORE/slots/logger/LogSlot.java:34-47) hands every BlockException to EagleEyeLogUtil.log(resource,
 * exceptionSimpleName, ruleLimitApp, origin, count), which a StatLogger sums per second into sentinel-block.log.
 * The engine keeps that sum on the device: once enabled, every chunk of every submit entry (host and device) ends
 * with one pass that adds the chunk's blocked entries to an engine-resident table of rows.  Logged: events the
 * caller submitted as SGA_KIND_ENTRY whose decision is SGA_BLOCK_FLOW, _PARAM, _DEGRADE, _SYSTEM or _AUTHORITY.
 * Not logged: SGA_PASS_WAIT (PriorityWaitException is no BlockException), exits, kind 2 / 3 events (the slot that
 * threw their block has a LogSlot of its own in front of it), and chunks the device entry refused (-1).
 * Off by default: an engine that never enables the log launches and allocates nothing for it. */
#define SGA_TAG_SCALAR 0u  /* tag = the argument's 64-bit key */
#define SGA_TAG_LIST 1u    /* tag = a 64-bit fold of the list's length and its element keys in order */
typedef struct sga_block_row {
    int64_t time_slot;   /* ts - ts % 1000 of the entries (StatLogger's rolling slot at intervalSeconds(1)) */
    uint64_t tag;        /* SGA_BLOCK_PARAM: args[paramIdx] of the blocking rule (tag_kind); 0 for every other decision */
    int64_t count;       /* sum of acquire (StatEntry.count(count)) */
    uint32_t resource;
    uint32_t origin;     /* 0 when the call had no origin array */
    uint32_t detail;     /* the block detail wait_ms carried */
    uint32_t events;     /* number of entries */
    uint8_t decision;    /* SGA_BLOCK_* */
    uint8_t tag_kind;    /* SGA_TAG_SCALAR / SGA_TAG_LIST */
    uint8_t reserved[6]; /* zero: sizeof == 48 */
} sga_block_row;

/* Turns the log on with room for max_rows rows (0: the default of 65,536; at least 64; rounded up to a power of
 * two).  Two tuples whose 64-bit hashes collide share a row (as two strings whose 64-bit keys collide share a parameter counter).
 * Calling it again resizes an empty log; with rows pending: SGA_EINVAL. */
int sga_block_log_enable(sga_engine *e, uint32_t max_rows);

/* Moves out every row with time_slot + 1000 <= before_ms (INT64_MAX: all), sorted by (time_slot, resource,
 * decision, detail, origin, tag_kind, tag); *n = their number.  More than cap: SGA_ERANGE, *n = the number needed,
 * nothing removed, the lost counters neither returned nor cleared.  A drained second that receives further events
 * gets new rows.  *lost_events / *lost_count (either may be NULL): entries and their acquire sum that found no room
 * in the table since the last successful drain -- returned and cleared.  Waits for the engine stream.  An engine
 * without the log: SGA_EINVAL. */
int sga_block_log_drain(sga_engine *e, int64_t before_ms, sga_block_row *rows, size_t cap, size_t *n,
                        uint64_t *lost_events, int64_t *lost_count);

/* The rule a block detail names, as its index in the array the caller last passed to the matching loader
 * (SGA_BLOCK_FLOW: sga_load_flow_rules*, whose _origin / _ctx forms reorder; SGA_BLOCK_PARAM: sga_load_param_rules;
 * SGA_BLOCK_DEGRADE: sga_load_degrade_rules).  Any other decision, an unknown resource or a detail past the
 * resource's rules: SGA_EINVAL. */
int sga_block_rule_index(sga_engine *e, int8_t decision, uint32_t resource, uint32_t detail, uint32_t *index);

/* ---- metric extensions (StatisticSlotCallbackRegistry; new entry points only) ---- */
/* MetricCallbackInit registers MetricEntryCallback and MetricExitCallback with StatisticSlotCallbackRegistry;
 * StatisticSlot (CORE/slots/statistic/StatisticSlot.java:65-175) calls them on every pass, block and exit, and they
 * fan out to every MetricExtension (CORE/metric/extension/): cumulative counters per resource, as opposed to the
 * nodes' sliding windows.  The engine keeps what those calls would have summed: once enabled, every chunk of every
 * submit entry (host and device, the sga_event_* queue included) ends with one pass that adds the chunk's events to
 * engine-resident 64-bit sums, exact and kept until drained.  By the caller's kind and the final decision:
 *   SGA_KIND_ENTRY, SGA_PASS or SGA_PASS_WAIT     pass += acquire, pass_events += 1 (onPass runs in the
 *                                                 PriorityWaitException branch too, where the node's second
 *                                                 window gets the pass only in the second it was borrowed from)
 *   SGA_KIND_ENTRY, SGA_BLOCK_*                   a block row (resource, origin, decision, wait_ms as detail)
 *   SGA_KIND_EXIT                                 success += acquire, exits += 1, rt_sum += rt, rt_max = max(rt) --
 *                                                 rt as given, neither capped at statistic_max_rt nor made positive;
 *                                                 with SGA_EV_ERROR also exception += acquire, exception_events += 1
 *   SGA_KIND_BLOCKED                              a block row (resource, origin, 0, 0): the exception was thrown
 *                                                 outside the engine
 *   SGA_KIND_REVOKE                               the same block row, and the entry's pass taken back:
 *                                                 pass -= acquire, pass_events -= 1
 * A revoke drained apart from its entry shows as a negative pass: the sums are signed deltas.  Counted for nothing: a
 * resource id >= n_resources, and every event of a chunk the device entry refused (-1).  The parameter of a
 * SGA_BLOCK_PARAM is not part of a block row's key.  Off by default: an engine that never enables the sums launches
 * and allocates nothing for them. */
typedef struct sga_metric_res_row {   /* sizeof == 72 */
    int64_t pass;              /* MetricExtension.addPass: sum of acquire */
    int64_t pass_events;       /* onPass calls = increaseThreadNum calls */
    int64_t success;           /* addSuccess: sum of acquire over exits */
    int64_t exits;             /* onExit calls = decreaseThreadNum calls */
    int64_t exception;         /* addException: sum of acquire over exits with SGA_EV_ERROR */
    int64_t exception_events;
    int64_t rt_sum;            /* addRt: sum of rt over exits */
    int64_t rt_max;            /* the largest rt of an exit, at least 0 (0 without exits) */
    uint32_t resource;
    uint32_t reserved;
} sga_metric_res_row;

typedef struct sga_metric_block_row {   /* sizeof == 32 */
    int64_t block;             /* addBlock: sum of acquire */
    int64_t block_events;      /* onBlocked calls */
    uint32_t resource;
    uint32_t origin;           /* 0 when the call had no origin array */
    uint32_t detail;           /* the block detail wait_ms carried (sga_block_rule_index names the rule) */
    uint8_t decision;          /* SGA_BLOCK_*; 0: a kind 2 / 3 event (a plain BlockException) */
    uint8_t reserved[3];
} sga_metric_block_row;

/* Turns the sums on (after sga_flow_set_resources) with room for max_block_rows block rows (0: the default of
 * 65,536; at least 64; rounded up to a power of two); the per-resource sums are one 64-byte line per resource and
 * cannot overflow.  Two block keys whose 64-bit hashes collide share a row.  Events submitted before the call are not
 * counted.  Calling it again resizes the block table while nothing is pending; with sums pending: SGA_EINVAL. */
int sga_metric_ext_enable(sga_engine *e, uint32_t max_block_rows);

/* Moves out everything summed since the last drain: the resources with any non-zero sum, sorted by resource, and all
 * block rows, sorted by (resource, origin, decision, detail); *n_res / *n_block = their numbers.  If either cap is too
 * small: SGA_ERANGE, both numbers as needed, nothing removed, the lost counters neither returned nor cleared.
 * *lost_events / *lost_count (either may be NULL): blocked entries and their acquire sum that found no room in the
 * block table since the last successful drain -- returned and cleared.  Waits for the event queue and the engine
 * stream.  An engine without the sums: SGA_EINVAL. */
int sga_metric_ext_drain(sga_engine *e, sga_metric_res_row *res_rows, size_t res_cap, size_t *n_res,
                         sga_metric_block_row *block_rows, size_t block_cap, size_t *n_block, uint64_t *lost_events,
                         int64_t *lost_count);

/* ---- token server log (ClusterServerStatLogUtil; new entry points only) ---- */
/* The cluster checkers record what they refused through ClusterServerStatLogUtil.log(msg[, count])
 * (CS/flow/ClusterFlowChecker.java:91,102-107, ClusterParamFlowChecker.java:77-79, RLS SimpleClusterFlowChecker.java:49-61),
 * which a StatLogger sums per second into sentinel-server.log.  The engine keeps those sums on the device: once
 * enabled, every token batch of every entry (sga_request_tokens and its device, packed, async and pipelined forms,
 * the coalescing queue, sga_request_param_tokens, sga_rls_should_rate_limit and its device form) ends with one pass
 * that adds the batch's requests to an engine-resident table of rows.  One request forms one tuple or none:
 *   SGA_SLOG_FLOW_BLOCK       BLOCKED, not prioritized (or an RLS descriptor)   count += acquire, events += 1
 *   SGA_SLOG_FLOW_BLOCK_PRIO  BLOCKED, prioritized                              count += acquire, events += 1
 *   SGA_SLOG_FLOW_WAITING     SHOULD_WAIT                                       count += 1,       events += 1
 *   SGA_SLOG_FLOW_PASS        OK, RLS descriptors only                          count += acquire, events += 1
 *   SGA_SLOG_PARAM_PASS       requestParamToken OK with a non-empty value list  count += 1,       events += 1
 *   SGA_SLOG_PARAM_BLOCK      requestParamToken BLOCKED; tag = the first value  count += 1,       events += 1
 *                             in collection order whose nextRemaining < 0
 * Nothing is formed for TOO_MANY_REQUEST, FAIL, NO_RULE_EXISTS and BAD_REQUEST (an empty value list among them)
 * nor for a batch that failed.
 * The concurrency checker writes to the same file (CS/flow/ConcurrentClusterFlowChecker.java:58,67,73,99), so every
 * staged chunk of sga_concurrent_ops ends with a pass of its own behind the kernel that decided it.  One operation
 * forms one tuple or none, in the second of the operation itself (a release counts in the second of the release):
 *   SGA_SLOG_CONC_PASS        acquire answered OK                               count += acquire, events += 1
 *   SGA_SLOG_CONC_BLOCK       acquire answered BLOCKED                          count += acquire, events += 1
 *   SGA_SLOG_CONC_RELEASE     release answered RELEASE_OK; flow_id and the      count += the token's acquire,
 *                             count are those of the token's node, not the call's                events += 1
 * with tag 0.  BAD_REQUEST, NO_RULE_EXISTS and ALREADY_RELEASE (the second release of one token inside a batch among
 * them) form nothing, and neither does an expiry pass (RegularExpireStrategy writes to RecordLog only).  This path
 * has no failed batches: the pass is unconditional.
 * Off by default: an engine that never enables the log launches and allocates nothing for it. */
#define SGA_SLOG_FLOW_BLOCK 0
#define SGA_SLOG_FLOW_BLOCK_PRIO 1
#define SGA_SLOG_FLOW_WAITING 2
#define SGA_SLOG_FLOW_PASS 3
#define SGA_SLOG_PARAM_PASS 4
#define SGA_SLOG_PARAM_BLOCK 5
#define SGA_SLOG_CONC_PASS 6
#define SGA_SLOG_CONC_BLOCK 7
#define SGA_SLOG_CONC_RELEASE 8
typedef struct sga_server_log_row {   /* sizeof == 40 */
    int64_t time_slot;   /* t - t % 1000 of the requests (StatLogger's rolling slot at intervalSeconds(1)) */
    int64_t flow_id;
    uint64_t tag;        /* SGA_SLOG_PARAM_BLOCK: the blocking value's 64-bit key; 0 for every other kind */
    int64_t count;
    uint32_t events;
    uint8_t kind;        /* SGA_SLOG_* */
    uint8_t reserved[3]; /* zero */
} sga_server_log_row;

/* Turns the log on with room for max_rows rows (0: the default of 65,536; at least 64; rounded up to a power of
 * two; at most 2^26).  Two tuples whose 64-bit hashes collide share a row, as in the block log.  Calling it again
 * resizes an empty log; with rows pending: SGA_EINVAL. */
int sga_server_log_enable(sga_engine *e, uint32_t max_rows);

/* Moves out every row with time_slot + 1000 <= before_ms (INT64_MAX: all), sorted by (time_slot, flow_id, kind,
 * tag); *n = their number.  More than cap: SGA_ERANGE, *n = the number needed, nothing removed, the lost counters
 * neither returned nor cleared.  A drained second that receives further events gets new rows.  *lost_events /
 * *lost_count (either may be NULL): tuples and their count sum that found no room in the table since the last
 * successful drain -- returned and cleared.  Waits for the queued batches.  An engine without the log: SGA_EINVAL. */
int sga_server_log_drain(sga_engine *e, int64_t before_ms, sga_server_log_row *rows, size_t cap, size_t *n,
                         uint64_t *lost_events, int64_t *lost_count);

/* The gauges ClusterConcurrentCheckerLogListener writes once a second (CS/flow/statistic/concurrent/
 * ClusterConcurrentCheckerLogListener.java:39-54): one row for every loaded cluster flow rule that is active, is in
 * CurrentConcurrencyManager's map and has nowCalls != 0 (negative values are listed), sorted by flow_id; *n = their
 * number.  *token_size (may be NULL): TokenCacheNodeManager.getSize().  The rows are compacted on the device, so the
 * call copies back what it returns and nothing else.  More rows than cap: SGA_ERANGE, *n = the number needed, nothing
 * written.  Waits for the engine stream, changes no state and does not need the log enabled.  An engine without
 * concurrency state yet: *n = 0, *token_size = 0. */
typedef struct sga_concurrent_gauge {   /* sizeof == 24 */
    int64_t flow_id;
    double  level;       /* ConcurrentClusterFlowChecker.calcGlobalThreshold(rule): count, or count * connectedCount */
    int32_t now_calls;   /* CurrentConcurrencyManager value, != 0 */
    int32_t reserved;    /* zero */
} sga_concurrent_gauge;
int sga_concurrent_gauges(sga_engine *e, sga_concurrent_gauge *rows, size_t cap, size_t *n, uint64_t *token_size);

/* ---- circuit breaker events (EventObserverRegistry; new entry points only) ---- */
/* AbstractCircuitBreaker notifies every CircuitBreakerStateChangeObserver of each transition with (prevState,
 * newState, rule, snapshotValue) (CORE/slots/block/degrade/circuitbreaker/AbstractCircuitBreaker.java:102-164).
 * Once enabled, the kernels that decide a breaker append one record per transition to an engine-resident buffer,
 * on every submit entry (host and device, _origin, _ctx, _tree, the sga_event_* queue).  Off by default: an engine
 * that never enables the log launches and allocates nothing for it. */
#define SGA_CB_CLOSED 0u
#define SGA_CB_OPEN 1u
#define SGA_CB_HALF_OPEN 2u
typedef struct sga_cb_event {
    int64_t ts;        /* time of the event that caused the transition */
    double value;      /* snapshotValue when next is SGA_CB_OPEN (the reference passes null otherwise), else 0 */
    uint64_t seq;      /* events submitted to the engine since the log was enabled and before this one */
    uint32_t resource; /* dense resource id */
    uint32_t breaker;  /* index k in DegradeRuleManager list order (as sga_circuit_breaker_state) */
    uint32_t epoch;    /* sga_load_degrade_rules calls so far: the rule list k indexes */
    uint16_t sub;      /* emission order within one event */
    uint8_t prev, next; /* SGA_CB_*; sizeof == 40 */
} sga_cb_event;

/* Turns the log on with room for max_events records (0: the default of 65,536; at least 64; rounded up to a power
 * of two); seq counts from the first call.  Calling it again resizes an empty log; with records pending:
 * SGA_EINVAL.  Also SGA_EINVAL: an engine without resources (sga_flow_set_resources comes first), and max_events
 * above 2^26.  A transition that finds the buffer full is counted as lost and changes no breaker. */
int sga_cb_events_enable(sga_engine *e, uint32_t max_events);

/* Moves out every pending record, sorted by (seq, sub): the order in which the reference would have called the
 * observers; *n = their number.  More than cap: SGA_ERANGE, *n = the number needed, nothing removed, lost neither
 * returned nor cleared.  *lost (may be NULL): transitions that found no room since the last successful drain --
 * returned and cleared.  Waits for the engine stream.  An engine without the log: SGA_EINVAL. */
int sga_cb_events_drain(sga_engine *e, sga_cb_event *ev, size_t cap, size_t *n, uint64_t *lost);

/* SystemRule (CORE/slots/system/SystemRule.java:43-50); negative = not set. */
typedef struct sga_system_rule {
    double highest_system_load;
    double highest_cpu_usage;  /* > 1 is ignored as invalid */
    double qps;
    int64_t avg_rt;
    int64_t max_thread;
} sga_system_rule;

/* SystemRuleManager.loadRules (SystemPropertyListener.configUpdate + loadSystemConf,
 * SystemRuleManager.java:191-300): the minimum of every field over the rules; the check is on
 * when the LAST rule sets any field (the reference sets the switch per rule); an empty list turns
 * it off.  While on, inbound entries (SGA_EV_INBOUND) pass SystemRuleManager.checkSystem against
 * ENTRY_NODE before the other slots -- a global order dependency: such batches are decided by
 * one sequential lane (exact).  Returns the number of rules that set a field. */
int sga_load_system_rules(sga_engine *e, const sga_system_rule *rules, size_t n);

/* SystemStatusListener readings (system load average, CPU usage 0..1; -1 = not measured yet). */
int sga_set_system_status(sga_engine *e, double avg_load, double cpu_usage);
/* circuit breaker k of a resource: 0 CLOSED, 1 OPEN, 2 HALF_OPEN (negative = no such breaker) */
int sga_circuit_breaker_state(sga_engine *e, uint32_t resource, uint32_t k);

/* ---------------------------------------------------------------------------
 * Once-per-second metrics
 * ------------------------------------------------------------------------- */

/* MetricNode, CORE/node/metric/MetricNode.java:28-51 (thin-format fields); resource = dense id */
typedef struct sga_metric_node {
    int64_t timestamp;        /* second-window start (minute LeapArray bucket) */
    int64_t pass_qps, block_qps, success_qps, exception_qps;
    int64_t rt;               /* rt sum / success (ArrayMetric.fromBucket, :203-218) */
    int64_t occupied_pass_qps;
    uint32_t resource;
    int32_t concurrency;      /* not filled by StatisticNode.metrics() (0) */
} sga_metric_node;

/* StatisticNode.metrics() of every resource's ClusterNode at `now` (CORE/node/StatisticNode.java:120-157):
 * minute buckets with lastFetchTime < start < now - now % 1000 and a non-zero field, each node's
 * lastFetchTime advanced as in the reference.  Up to `cap` nodes; *n = number written (the order
 * between resources is unspecified, like the reference's ClusterNode map).  -ERANGE if more than
 * `cap` nodes were due (the first `cap` are written, lastFetchTime still advanced). */
int sga_metrics_snapshot(sga_engine *e, int64_t now, sga_metric_node *out, size_t cap, size_t *n);

/* ClusterMetricNodeGenerator.flowToMetricNode for every active cluster flow rule
 * (CS/flow/statistic/ClusterMetricNodeGenerator.java:75-91): passQps / blockQps =
 * ClusterMetric.getAvg(PASS / BLOCK) at `now` (rotation side effect included). */
typedef struct sga_cluster_metric_node {
    int64_t flow_id;
    double pass_qps;
    double block_qps;
    int64_t timestamp;
} sga_cluster_metric_node;

int sga_cluster_metric_nodes(sga_engine *e, int64_t now, sga_cluster_metric_node *out, size_t cap, size_t *n);
/* Same into DEVICE memory on `hip_stream` (NULL = engine stream), count into *d_n (uint32, device):
 * the input of the once-per-second RCCL all-gather across the node's GPUs. */
int sga_cluster_metric_nodes_device(sga_engine *e, int64_t now, sga_cluster_metric_node *d_out, size_t cap,
                                    uint32_t *d_n, void *hip_stream);

/* ---- gateway flow rules: request fields -> argument vectors (no struct changes: new entry points only) ----
 * GatewayParamParser.parseParameterFor (GW = sentinel-adapter/sentinel-api-gateway-adapter-common/src/main/java/
 * com/alibaba/csp/sentinel/adapter/gateway/common; GW/param/GatewayParamParser.java:51-174) for a whole batch:
 * per event and rule of its resource, pick a request field, match it against the rule's pattern, and hash the
 * resulting string into the 64-bit key the parameter maps use.  The converted ParamFlowRules
 * (GW/rule/GatewayRuleConverter.java:49-86) are loaded through sga_load_param_rules like any other; this table
 * only says how each resource's argument vector is made.
 *
 * One item per valid GatewayFlowRule.  index: the rule's paramItem index as GatewayRuleManager assigned it
 * (GW/rule/GatewayRuleManager.java:179-237), -1 for a rule without a paramItem.  field: a column of the request
 * field table.  Items of one resource that share an index: the last in array order wins the slot.  A resource's
 * argument count is (its items with index >= 0) + (1 if it has an item of index -1): at most 64. */
typedef struct sga_gateway_item {
    uint32_t resource;
    int32_t index;
    uint32_t field;
    int32_t match_strategy; /* 0 EXACT, 2 REGEX, 3 CONTAINS; 1 (PREFIX) and everything else keep the value */
    uint32_t pattern_off;   /* the pattern's UTF-8 bytes in patterns_blob */
    uint32_t pattern_len;
    int32_t resource_mode;  /* 0 route id, 1 custom API name */
    uint8_t has_pattern;    /* 0: pattern null or empty -- no matching */
    uint8_t reserved[3];
} sga_gateway_item;
#define SGA_GW_EXACT 0
#define SGA_GW_REGEX 2
#define SGA_GW_CONTAINS 3
#define SGA_GW_NULL 0xFFFFFFFFu /* a field length: the request has no such field (0 is the empty string) */
#define SGA_GW_SEED 0x5E47ull   /* a string's key: XXH64 of its UTF-8 bytes with this seed */

/* Replaces the table (n_items = 0 clears it: sga_gateway_parse* then launch nothing).  After
 * sga_flow_set_resources.  SGA_EINVAL: a resource or field out of range, an index outside [-1, 64), a pattern
 * outside the blob; SGA_ERANGE: a resource with more than 64 arguments. */
int sga_gateway_load(sga_engine *e, const sga_gateway_item *items, size_t n_items, const uint8_t *patterns_blob,
                     size_t blob_len, uint32_t n_fields);
/* The largest argument count of a loaded resource (0: no table).  sga_gateway_parse* write each event's vector
 * at value_base + i * 2 * max_args: the value buffer holds value_base + 2 * max_args * n words. */
int sga_gateway_max_args(sga_engine *e, uint32_t *out);
/* XXH64(bytes, SGA_GW_SEED): the key sga_gateway_parse* give a string ("$NM" and "$D" included). */
uint64_t sga_gateway_string_key(const uint8_t *bytes, size_t len);

/* REGEX items decided on the device: a program is a DFA over the bytes of the value, compiled by the caller (the
 * Python front end compiles Python's `re` dialect, sentinel_amd/gateway_regex.py; a front end that wants
 * java.util.regex's answers compiles its own tables).  The kernel walks s = 1; for each byte
 * s = trans[s * n_classes + class_map[byte]], leaving at s == 0; the value matches iff bit (s & 7) of
 * accept[s >> 3] is set (the empty value is answered by state 1).  State 0 is dead: row 0 is all zeros and it does
 * not accept.  item: an index into the item array of the last sga_gateway_load.  class_off (256 bytes), trans_off
 * (n_states * n_classes uint16, row-major; a multiple of 2) and accept_off ((n_states + 7) / 8 bytes) point into
 * the blob; programs may share slices. */
typedef struct sga_gateway_regex {
    uint32_t item;
    uint32_t n_states, n_classes;
    uint32_t class_off, trans_off, accept_off;
} sga_gateway_regex;
/* Attaches programs to the table last loaded (n_programs = 0 drops them all; sga_gateway_load drops them too: they
 * belong to the table they were compiled for).  The slot a program's item writes is then decided by the program:
 * its bit of the regex_bits word is ignored, and so is a NULL word.  An item shadowed by a later one on its index
 * decides nothing, with or without a program; of two programs for one item the later counts.  Everything is
 * checked on the host before anything is uploaded, so the walk needs no bounds checks: SGA_EINVAL, with the
 * engine's programs left as they were, unless every program names a REGEX item with a pattern, has
 * 2 <= n_states <= 65535 and 1 <= n_classes <= 256, slices inside the blob, an even trans_off, class values below
 * n_classes, transitions below n_states, an all-zero row 0 and a state 0 that does not accept. */
int sga_gateway_load_regex(sga_engine *e, const sga_gateway_regex *programs, size_t n_programs, const uint8_t *blob,
                           size_t blob_len);
/* How many argument slots are decided by a program. */
int sga_gateway_regex_count(sga_engine *e, uint32_t *out);
/* Over DEVICE buffers, asynchronous on `hip_stream` with the ordering of sga_submit_events_device; n <= max_batch.
 * d_mode[i]: the request's resource mode.  The values are read as aligned 4-byte words: d_bytes must be readable from
 * the 4-byte boundary at or below it to the one at or above d_bytes + n_bytes (any hipMalloc'd buffer is).
 *  Field k of event i is d_bytes[d_field_off[i * n_fields + k] ..
 * + d_field_len[i * n_fields + k]) (any offset, any length; SGA_GW_NULL: null).  d_regex_bits (may be NULL: every
 * REGEX item matches): bit `index` of word i = the REGEX item at that index matches event i's value.  A REGEX item
 * with a program (sga_gateway_load_regex, below) is matched on the device and reads no bit.
 * For every event whose resource has items: the SGA_EV_ARGS words of parseParameterFor's array go to
 * d_param_values[value_base + i * 2 * max_args ..), d_param[i] = offset << 32 | nargs, d_flags[i] |= SGA_EV_ARGS
 * (nargs 0 when a rule's resource mode differs from d_mode[i]).  Null fields and unwritten slots are
 * SGA_ARG_NULL; strings are SGA_ARG_SCALAR with sga_gateway_string_key.  Every other event is left as given.
 * An event whose field slice leaves the blob or whose vector leaves the value buffer (n_values words, fewer than
 * 2^32 - 1) gets d_param[i] = 0xFFFFFFFF << 32 with SGA_EV_ARGS -- an empty vector past the buffer, which every
 * submit entry refuses with its chunk -- and sga_events_device_status reports SGA_EINVAL. */
int sga_gateway_parse_device(sga_engine *e, const uint32_t *d_resource, const uint8_t *d_mode,
                             const uint32_t *d_field_off, const uint32_t *d_field_len, const uint8_t *d_bytes,
                             size_t n_bytes, const uint64_t *d_regex_bits, size_t n, uint8_t *d_flags,
                             uint64_t *d_param, uint64_t *d_param_values, size_t n_values, size_t value_base,
                             void *hip_stream);
/* The same over HOST buffers, synchronous, any n (chunks of max_batch inside); like the device form it leaves the
 * words of param_values it does not write as they were.  SGA_EINVAL for what the device
 * form reports through the status call (the outputs then hold the poisoned events). */
int sga_gateway_parse(sga_engine *e, const uint32_t *resource, const uint8_t *mode, const uint32_t *field_off,
                      const uint32_t *field_len, const uint8_t *bytes, size_t n_bytes, const uint64_t *regex_bits,
                      size_t n, uint8_t *flags, uint64_t *param, uint64_t *param_values, size_t n_values,
                      size_t value_base);

/* ---- gateway API groups: request paths -> matching ApiDefinitions -> entries (new entry points only) ----
 * What every adapter's filter does per request (pickMatchingApiDefinitions: the path against every loaded
 * ApiDefinition, GW/api/matcher/AbstractApiMatcher.java; then one entry per matching API name with
 * RESOURCE_MODE_CUSTOM_API_NAME) for a whole batch.  The table is a list of predicates; API k matches a request iff
 * any predicate with api == k does.  kind EXACT: the path equals blob[a .. a + b).  kind DFA: a byte DFA walked over
 * the path, a = n_states, b = n_classes, c = class_off, d = trans_off, e = accept_off -- sga_gateway_regex's format and
 * contract (REGEX patterns, and Ant path patterns translated to the same tables by the front end).  kind HOST: bit a
 * (< 64) of the request's host word, for what the front end decides itself. */
typedef struct sga_gateway_api_pred {
    uint32_t api;  /* < n_apis */
    uint32_t kind; /* SGA_GW_API_* */
    uint32_t a, b, c, d, e;
} sga_gateway_api_pred;
#define SGA_GW_API_EXACT 0
#define SGA_GW_API_DFA 1
#define SGA_GW_API_HOST 2
#define SGA_GW_API_MAX 4096 /* design limit: APIs per table (64 bitmap words per request) */

/* Replaces the table (n_preds = 0 clears it: the match and expand entries then launch nothing).  After
 * sga_flow_set_resources.  api_resource[k] (< the resource count): the resource id API k is entered as.  Everything
 * is checked on the host before anything is uploaded, so the walk carries no bounds checks.  SGA_EINVAL, with the
 * loaded table left in place: an api >= n_apis, a resource out of range, an unknown kind, a slice outside the blob,
 * a DFA that breaks sga_gateway_load_regex's rules, a host bit >= 64, n_apis = 0.  SGA_ERANGE, likewise: more than
 * 64 HOST predicates, more than SGA_GW_API_MAX APIs. */
int sga_gateway_api_load(sga_engine *e, const sga_gateway_api_pred *preds, size_t n_preds,
                         const uint32_t *api_resource, size_t n_apis, const uint8_t *blob, size_t blob_len);
/* The loaded table's API count (0: no table) and the predicates decided on the device (EXACT and DFA). */
int sga_gateway_api_count(sga_engine *e, uint32_t *n_apis, uint32_t *n_device_preds);
/* Over DEVICE buffers, asynchronous on `hip_stream` with the ordering of sga_submit_events_device; n <= max_batch.
 * Request i's path is d_bytes[d_path_off[i] .. + d_path_len[i]) (SGA_GW_NULL: no path -- matches nothing), read as
 * aligned 4-byte words under sga_gateway_parse_device's contract.  d_host_bits (may be NULL: every HOST predicate
 * answers no match -- a missing answer must not enter a resource): one word per request.  d_match: n x W uint64,
 * W = (n_apis + 63) / 64, bit k % 64 of word k / 64 of row i = API k matches request i; every row is written in full.
 * A path slice that leaves the blob zeroes its row and sga_events_device_status reports SGA_EINVAL. */
int sga_gateway_api_match_device(sga_engine *e, const uint32_t *d_path_off, const uint32_t *d_path_len,
                                 const uint8_t *d_bytes, size_t n_bytes, const uint64_t *d_host_bits, size_t n,
                                 uint64_t *d_match, void *hip_stream);
/* The entry list of a batch, same ordering and n <= max_batch: request i contributes, in input order, the route entry
 * (resource d_route[i], mode 0) unless d_route[i] == SGA_GW_NULL, then one entry per set bit of its row in ascending
 * API index (resource api_resource[k], mode 1; the reference collects a HashSet: the order among one request's APIs
 * is parity-unpinned).  Entry j: d_src[j] = its request, d_pos[j] = its position inside the request (a caller that
 * wants the filter's stop-at-first-block submits position 0 of every request, then position 1 of the unblocked ones,
 * and so on: that loop is the caller's).  d_field_off / d_field_len (n x n_fields) with the two _out arrays
 * (cap x n_fields), all four or none: entry j gets row d_src[j] of the request field table, ready for
 * sga_gateway_parse_device.  *d_total (uint32, device) = the entries needed; entries at or past cap are not written.
 * SGA_ERANGE: n * (1 + n_apis) >= 2^32. */
int sga_gateway_api_expand_device(sga_engine *e, const uint32_t *d_route, const uint64_t *d_match, size_t n,
                                  const uint32_t *d_field_off, const uint32_t *d_field_len, uint32_t n_fields,
                                  size_t cap, uint32_t *d_src, uint32_t *d_pos, uint32_t *d_resource, uint8_t *d_mode,
                                  uint32_t *d_field_off_out, uint32_t *d_field_len_out, uint32_t *d_total,
                                  void *hip_stream);
/* The same over HOST buffers, synchronous, any n (chunks of max_batch inside, entry offsets continued across
 * chunks).  sga_gateway_api_match: SGA_EINVAL for what the device form reports through the status call.
 * sga_gateway_api_expand: *total = the entries needed; SGA_ERANGE when cap is smaller (the first cap are written). */
int sga_gateway_api_match(sga_engine *e, const uint32_t *path_off, const uint32_t *path_len, const uint8_t *bytes,
                          size_t n_bytes, const uint64_t *host_bits, size_t n, uint64_t *match);
int sga_gateway_api_expand(sga_engine *e, const uint32_t *route, const uint64_t *match, size_t n,
                           const uint32_t *field_off, const uint32_t *field_len, uint32_t n_fields, size_t cap,
                           uint32_t *src, uint32_t *pos, uint32_t *resource, uint8_t *mode, uint32_t *field_off_out,
                           uint32_t *field_len_out, size_t *total);

/* Optional helper for tools: HIP stream of the engine (hipStream_t as void*). */
void *sga_engine_stream(sga_engine *e);

#ifdef __cplusplus
}
#endif
#endif
