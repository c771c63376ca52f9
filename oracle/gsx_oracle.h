/*
 * gsx_oracle.h — CPU restatement of the reference's peer-scoring semantics.
 *
 * TEST INFRASTRUCTURE ONLY.  This is the parity checker for the HIP engine in
 * go-libp2p-pubsub_amd/.  Only tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg may load it; the product path never links or calls it.
 *
 * It restates, in plain C over an array-of-structs model that follows the
 * reference's own structs, the functions of /root/reference/score.go and
 * score_params.go (each function cites the file:line it follows).  It shares
 * only the parameter/event/state-view TYPE definitions with include/gsx.h
 * (data layout of the boundary), none of its logic.
 *
 * Pinning: the reference is Go and no Go toolchain exists in this container
 * (SURVEY.md §8c), so the reference cannot be built or run here.  The oracle
 * is pinned against the known-answer values held by the reference's own tests
 * (score_test.go, score_params_test.go), restated as fixtures in
 * tests/golden/ by tests/golden/make_golden.py.
 *
 * Determinism contract: the reference iterates Go maps in
 * random order; the oracle uses ascending topic index for the topic sum of
 * score() and applies events in the order given.  Floating point is IEEE
 * binary64 with no contraction (-ffp-contract=off), matching Go on amd64.
 */
#ifndef GSX_ORACLE_H
#define GSX_ORACLE_H

#include "../include/gsx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orc_engine orc_engine;

orc_engine* orc_create(uint32_t n_topics);
void orc_destroy(orc_engine* o);

int orc_validate_peer_params(const gsx_peer_score_params* p);
int orc_validate_topic_params(const gsx_topic_score_params* p);
int orc_validate_thresholds(const gsx_thresholds* p);
double orc_score_parameter_decay_with_base(int64_t decay_ns, int64_t base_ns, double decay_to_zero);
double orc_score_parameter_decay(int64_t decay_ns);

int orc_set_peer_params(orc_engine* o, const gsx_peer_score_params* p);
int orc_set_topic_params(orc_engine* o, uint32_t topic, const gsx_topic_score_params* p);
int orc_load_overlay(orc_engine* o, uint32_t n_nodes, const int64_t* row_ptr, const int32_t* col,
                     const uint8_t* edge_flags, const uint32_t* node_ips);
int orc_set_thresholds(orc_engine* o, const gsx_thresholds* t);
/* Propagation (floodsub.go:76-100, gossipsub.go:943-1013, randomsub.go:99-160
 * under the synchronous-hop contract of gsx.h), one message at a time.
 * hop/from: optional [m][n_nodes] outputs. */
int orc_propagate(orc_engine* o, const gsx_msg* msgs, size_t m, const gsx_prop_config* cfg, gsx_prop_out* out,
                  uint8_t* hop, int32_t* from);
/* With dup tracking on, orc_propagate records which copies were duplicates
 * (the DuplicateMessage tracer calls, pubsub.go:1052-1056) per receiving
 * pair, laid out as gsx_prop_duplicates' rows. */
int orc_prop_set_dup_tracking(orc_engine* o, int on);
int orc_prop_duplicates(orc_engine* o, uint64_t* rows, size_t n_words);
/* Heartbeat round (gossipsub.go:1303-1604, 718-859) under the contract of gsx.h. */
int orc_default_gossipsub_params(gsx_gossipsub_params* p);
int orc_heartbeat(orc_engine* o, const gsx_gossipsub_params* gp, uint64_t tick, int64_t now_ns, uint64_t seed,
                  gsx_heartbeat_out* out);
/* gsx_hb_trace_words of the last orc_heartbeat (always recorded). */
int orc_set_gossipsub_params(orc_engine* o, const gsx_gossipsub_params* gp);
int orc_set_subscriptions(orc_engine* o, const uint64_t* joined);
int orc_export_membership(orc_engine* o, uint64_t* joined, uint64_t* fanout, int64_t* lastpub);
int orc_join(orc_engine* o, const uint32_t* nodes, const uint32_t* topics, size_t n, int64_t now, uint64_t seed,
             gsx_heartbeat_out* out);
int orc_leave(orc_engine* o, const uint32_t* nodes, const uint32_t* topics, size_t n, int64_t now,
              gsx_heartbeat_out* out);
int orc_hb_trace_words(orc_engine* o, uint64_t* sent_graft, uint64_t* sent_prune, uint64_t* acc_graft,
                       uint64_t* handled_prune);
/* gsx_hb_px_records of the last orc_heartbeat (every candidate is kept). */
int orc_hb_px_records(orc_engine* o, uint32_t* out, size_t cap, size_t* n);
int orc_export_backoff(orc_engine* o, int64_t* out);
int orc_import_backoff(orc_engine* o, const int64_t* in);
int orc_gossip_results(orc_engine* o, uint32_t* len, uint64_t* hash);
/* the gossipTracer's promises (gossip_tracer.go:48-185; gsx.h gsx_promise_*) */
int orc_promise_add(orc_engine* o, uint64_t pair, const uint64_t* handles, uint32_t n, int64_t expire, uint64_t seed);
int orc_promise_broken(orc_engine* o, int64_t now, uint32_t* counts, uint64_t* total);
int orc_promise_fulfill(orc_engine* o, uint32_t node, uint64_t handle);
int orc_promise_throttle(orc_engine* o, uint64_t pair);
int orc_promise_count(orc_engine* o, uint64_t* n);
/* Rejected Int31n draws (Go's `for v > max` redraw) since the last reset, per
 * draw tag of the counter hash: process-wide, every engine and thread adds to
 * them.  For tests that must know a run took the redraw branch. */
#define ORC_RNG_TAGS 16
void orc_rng_rejections(uint64_t* out); /* ORC_RNG_TAGS counts */
void orc_rng_rejections_reset(void);
int orc_mcache_clear(orc_engine* o);
int orc_mcache_last(orc_engine* o, uint32_t* n_msgs);
/* hop_rows (may be NULL): the set's arrival hops ([node][message] bytes, the
 * validation codes of a propagated set) */
int orc_mcache_copy_last(orc_engine* o, uint8_t* cache_rows, uint8_t* set_rows, uint8_t* hop_rows);
int orc_mcache_pop(orc_engine* o);
int orc_mcache_put(orc_engine* o, const gsx_msg* msgs, size_t m, const gsx_prop_config* cfg, uint32_t n_parts,
                   const uint32_t* part_msgs, const uint8_t* const* cache_parts, const uint8_t* const* set_parts,
                   const uint8_t* const* hop_parts);
int orc_mcache_ids(orc_engine* o, uint32_t node, uint32_t topic, uint32_t n_windows, uint64_t* out, size_t cap,
                   size_t* n_out);
int orc_set_ip_whitelist(orc_engine* o, const uint32_t* ip_ids, size_t n);
int orc_set_app_scores(orc_engine* o, const double* app, size_t n_pairs);
int orc_set_pair_ips(orc_engine* o, const uint64_t* pairs, const uint32_t* ips, size_t n);
int orc_ip_colocation_factors(orc_engine* o, double* out);

int orc_apply_events(orc_engine* o, const gsx_event* ev, size_t n);

int orc_trace_validate(orc_engine* o, uint64_t pair, uint64_t msg_id, uint32_t topic, int64_t now_ns);
int orc_trace_deliver(orc_engine* o, uint64_t pair, uint64_t msg_id, uint32_t topic, int64_t now_ns);
int orc_trace_reject(orc_engine* o, uint64_t pair, uint64_t msg_id, uint32_t topic, int32_t reason,
                     int64_t now_ns);
int orc_trace_duplicate(orc_engine* o, uint64_t pair, uint64_t msg_id, uint32_t topic, int64_t now_ns);
int orc_gc_deliveries(orc_engine* o, int64_t now_ns);
uint64_t orc_num_delivery_records(orc_engine* o);

/* refreshScores (score.go:497-558) */
int orc_refresh(orc_engine* o, int64_t now_ns);
/* score() for every pair / one pair (score.go:258-335) */
int orc_scores(orc_engine* o, double* out, size_t n_pairs);
double orc_score(orc_engine* o, uint64_t pair);
/* Refresh + score restricted to pairs [p0, p1) (bench sample); returns 0. */
int orc_refresh_scores_range(orc_engine* o, int64_t now_ns, uint64_t p0, uint64_t p1, double* out);
/* refresh + score of every pair on n_threads OpenMP threads (bench CPU baseline) */
int orc_refresh_scores_parallel(orc_engine* o, int64_t now_ns, double* out, int n_threads);

int orc_import_state(orc_engine* o, const gsx_state_view* s);
int orc_export_state(orc_engine* o, gsx_state_view* s);
uint64_t orc_num_pairs(orc_engine* o);

#ifdef __cplusplus
}
#endif
#endif
