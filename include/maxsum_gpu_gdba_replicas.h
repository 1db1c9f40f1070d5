/* GDBA's seeded restarts as replicas of one engine, best state kept on the device: the declarations.
 * #included by maxsum_gpu.h at the end of its GDBA block (inside its extern "C"); not meant to be included alone.
 * Exported by the same library under the same mxs_version: a binding that needs these looks the symbols up
 * (pydcop_amd/gdba.py does, and says which are missing). */
#ifndef MAXSUM_GPU_GDBA_REPLICAS_H
#define MAXSUM_GPU_GDBA_REPLICAS_H

/* REPLICAS: n_replicas seeded runs of the instance in ONE engine, 1 <= n_replicas <= 4096 (else MXS_E_INVALID; null
 * seeds: MXS_E_INVALID; a grid of more than 2^31 - 1 blocks -- the largest launch of one run times n_replicas --:
 * MXS_E_INVALID; n_replicas times the bytes of one run's modifier tables above `pool_budget_bytes` (0: 4 GiB):
 * MXS_E_INVALID, the message gives both numbers and the replica count -- all of these before anything is allocated;
 * device memory that does not suffice: MXS_E_NOMEM, nothing stays allocated).  The slot view, the tables, the
 * violation references, the offsets of the modifier tables, the domains, the name ranks and the variable costs are
 * stored once; the dynamic state is [replica][variable] (values, held costs and their flags, improvement
 * records: 17 bytes per variable and replica in f32 mode, 29 in f64), [replica][slot] (violated flags; the cumulative variable costs where some variable cost
 * is non-zero) and [replica][modifier] (the pool: what slot -1 of the single run reports, per replica).  A round of all
 * replicas is the two launches one run needs; a block is one wave of one replica.  Replica r is bit for bit
 * mxs_gdba_create with seed seeds[r], the start included: a variable with an initial value keeps it in every replica,
 * the others take draw 6 under their replica's seed, a variable without neighbours its optimal_cost_value.  mxs_gdba_reset
 * / _run act on all replicas (the refusal past 65535 rounds stays); mxs_gdba_get_state, mxs_gdba_get_modifiers and
 * mxs_gdba_eval_cost(idx = NULL) mean replica 0; mxs_gdba_get_modifiers with slot = -1 reports the bytes of the whole
 * pool, all replicas.  An engine of mxs_gdba_create has one replica (its replica costs are mxs_gdba_eval_cost of its
 * state) and tracks no best state: _track_best and _get_best answer MXS_E_STATE there. */
int mxs_gdba_create_replicas(const mxs_graph *g, const mxs_params *p, const int32_t *name_rank,
                             const int32_t *value_rank, int32_t modifier, int32_t violation, int32_t increase_mode,
                             const uint64_t *seeds, int32_t n_replicas, int64_t pool_budget_bytes, int32_t device,
                             mxs_gdba **out);
int mxs_gdba_replicas(const mxs_gdba *e, int32_t *n);
int mxs_gdba_get_state_replica(mxs_gdba *e, int32_t replica, int32_t *idx, double *cost, uint8_t *has_cost,
                               double *improve, int32_t *new_value);
int mxs_gdba_get_modifiers_replica(mxs_gdba *e, int32_t replica, int32_t slot, int32_t *out, int64_t capacity,
                                   int64_t *n_entries);
/* DCOP.solution_cost of every replica's current assignment, reduced on the device: as mxs_dsa_replica_costs (the
 * same kernels; in f32 mode the cost of the narrowed tables) */
int mxs_gdba_replica_costs(mxs_gdba *e, double infinity, double *cost, int64_t *violations);
/* BEST STATE.  A GDBA run is not monotone: the breakout raises the weights of violated constraints and the assignment
 * wanders, so the state a run ends in is usually not the best one it passed through.  The semantics are those of
 * mxs_dsa_track_best / mxs_dsa_get_best with rounds in place of cycles: every > 0 keeps, per replica, the best state
 * seen at the call and after every `every`-th round (counted from the engine's round 0), on the device -- replaced on
 * STRICT improvement only, compared on (violations, cost; the cost negated with MXS_MODE_MAX) as mxs_gdba_replica_costs
 * computes them with this `infinity`; no atomics, the same bits from run to run.  every = 0: no records, _get_best
 * ranks the CURRENT states (its round is the engine's).  Every call clears the records, and so does mxs_gdba_reset
 * (the first record is then the start state).  _get_best: r = -1: the lexicographic minimum of (violations, cost,
 * index) over the replicas' records, else the record of replica r; any out pointer may be NULL; idx [n_vars] in
 * graph order.  MXS_E_STATE before the first _track_best; every < 0: MXS_E_INVALID. */
int mxs_gdba_track_best(mxs_gdba *e, int32_t every, double infinity);
int mxs_gdba_get_best(mxs_gdba *e, int32_t r, int32_t *replica, int64_t *round, double *cost, int64_t *violations,
                      int32_t *idx);

#endif /* MAXSUM_GPU_GDBA_REPLICAS_H */
