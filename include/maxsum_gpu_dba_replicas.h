/* DBA's seeded restarts as replicas of one engine, ranked by the violations counted on the device: the declarations.
 * #included by maxsum_gpu.h at the end of its DBA block (inside its extern "C"); not meant to be included alone.
 * Exported by the same library under the same mxs_version: a binding that needs these looks the symbols up
 * (pydcop_amd/dba.py does, and says which are missing). */
#ifndef MAXSUM_GPU_DBA_REPLICAS_H
#define MAXSUM_GPU_DBA_REPLICAS_H

/* REPLICAS: n_replicas seeded runs of the instance in ONE engine, 1 <= n_replicas <= 4096 (else MXS_E_INVALID; null
 * seeds: MXS_E_INVALID; a stop_policy other than 0 / 1: MXS_E_INVALID; a grid of more than 2^31 - 1 blocks -- the
 * largest launch of one run times n_replicas --: MXS_E_INVALID -- all of these, and the refusals of mxs_dba_create,
 * before anything is allocated; device memory that does not suffice: MXS_E_NOMEM, nothing stays allocated).  The
 * violation bit rows, their offsets and strides, the slot view, the domains and the name ranks are stored once; the
 * dynamic state is [replica][variable] (values, held costs and their flags, counters, flags, improvement records: 30
 * bytes per variable and replica) and [replica][slot] (weights, violated flags: 5 bytes).  A round of all replicas is
 * the two launches one run needs; a block is one wave of one replica.  Replica r is bit for bit mxs_dba_create with
 * seed seeds[r] for as long as it runs: state, weights and stop round.
 * stop_policy 0 (EACH): a replica that stops is frozen in the state of its stop round, the others run on; the engine
 * has ENDED once every replica has stopped, in the round of the last stop.  stop_policy 1 (FIRST): the engine ends
 * with the round F in which the first replica stops; every replica completes round F, nothing runs after it -- the
 * state of replica r is the single run's after min(its own stop round, F) rounds.  No read-back per round under
 * either policy.  mxs_dba_run after the end does nothing; mxs_dba_rounds is the rounds the engine has run, the end
 * round once it has ended; mxs_dba_finished reports whether it has ended, and in which round.  mxs_dba_reset / _run
 * act on all replicas (the int32 bound on the rounds stays); mxs_dba_get_state, mxs_dba_get_weights and
 * mxs_dba_eval_cost(idx = NULL) mean replica 0.  The sticky "improves with no best value" error is per replica:
 * _run fails with MXS_E_STATE and names the lowest such replica.  An engine of mxs_dba_create has one replica and
 * answers every call below. */
int mxs_dba_create_replicas(const mxs_graph *g, const mxs_params *p, const int32_t *name_rank, double infinity,
                            int32_t max_distance, const uint64_t *seeds, int32_t n_replicas, int32_t stop_policy,
                            int64_t mask_budget_bytes, int32_t device, mxs_dba **out);
int mxs_dba_replicas(const mxs_dba *e, int32_t *n);
int mxs_dba_get_state_replica(mxs_dba *e, int32_t replica, int32_t *idx, int32_t *cost, uint8_t *has_cost,
                              int32_t *eval, int32_t *improve, int32_t *new_value, int32_t *counter,
                              uint8_t *consistent);
int mxs_dba_get_weights_replica(mxs_dba *e, int32_t replica, int32_t *out /* [n_slots] */);
/* per replica: stop_round = the round in which it stopped (0: it is running, or the engine ended before it stopped),
 * rounds = the rounds it ran.  Either pointer may be NULL. */
int mxs_dba_stop_rounds(mxs_dba *e, int64_t *stop_round /* [n_replicas] */, int64_t *rounds /* [n_replicas] */);
/* per replica: the constraints whose entry under the replica's current assignment is >= `infinity` (the engine's,
 * compared as the bit rows were filled: NaN is not violated; NOT the `== infinity` of mxs_dba_eval_cost), the
 * constraints of variables that never play included.  Counted on the device from the bit rows, in a fixed shape
 * without atomics. */
int mxs_dba_replica_violations(mxs_dba *e, int64_t *violations /* [n_replicas] */);
/* the lexicographic minimum of (violations, stop round with running = +infinity, index) over the replicas' current
 * states: a stop does not imply a solution when max_distance is below the graph's diameter, so the violations come
 * first.  Any out pointer may be NULL. */
int mxs_dba_best_replica(mxs_dba *e, int32_t *replica, int64_t *stop_round, int64_t *violations);

#endif /* MAXSUM_GPU_DBA_REPLICAS_H */
