/* Max-Sum's best assignment and cost trace, kept on the device: the declarations.
 * #included by maxsum_gpu.h at the end of its engine block (inside its extern "C"); not meant to be included alone.
 * Exported by the same library under the same mxs_version: a binding that needs these looks the symbols up
 * (pydcop_amd/engine.py does, and says which are missing). */
#ifndef MAXSUM_GPU_ANYTIME_H
#define MAXSUM_GPU_ANYTIME_H

/* BEST STATE AND COST TRACE.  Max-Sum on a loopy graph is not monotone: the assignment it ends with is usually not
 * the best one it passed through.  every > 0 switches tracking on: any record and trace are cleared, the FIRST RECORD
 * is taken from the state as it is now, at the engine's cycle count (unconditionally, whatever its cost), and from
 * then on the cost and the violations of the selected values are evaluated on the device after every cycle c with
 * c % every == 0 (c: the engine's cycle count, not a per-call count) -- the cost of mxs_eval_cost(idx = NULL) with this
 * `infinity`, bit for bit: always f64 on the un-narrowed tables, in f32 engines too.  The record (a snapshot of the
 * selection with its cycle, cost and violations) is replaced on STRICT improvement only: fewer violations, or as many
 * and a lower cost (higher with MXS_MODE_MAX); a NaN cost never replaces a record.  Every evaluation, the first record
 * included, appends (cycle, cost, violations) to a device trace of `trace_capacity` entries; later evaluations are
 * counted, not stored.  Nothing is read back before _get_best / _get_cost_trace.  The result depends on the sequence
 * of cycles alone: not on how the cycles are split over calls, not on which of mxs_run / _run_async / _run_timed /
 * _run_reps made them, not on mxs_params.graph_chunk.  No atomics: the same bits from run to run.
 *   every == 0 switches tracking off and frees the buffers.  mxs_reset clears the record and the trace and takes the
 * first record at cycle 0.  mxs_set_state, mxs_update_factor_table, mxs_set_parent_table and mxs_slice_factor change
 * the state or the cost function: each restarts the record from the current state at the current cycle (one more
 * evaluation, appended to the trace, which is kept).
 *   MXS_E_INVALID: every < 0 or trace_capacity < 0.  MXS_E_STATE: a sharded engine (mxs_halo_setup, mxs_comm_init or
 * mxs_peer_connect has been called: the ownership masks make a shard's cost partial).  While tracking,
 * mxs_debug_timeline, mxs_step_compute / _pack / _unpack and mxs_halo_setup (so the engine cannot become a shard:
 * mxs_comm_init and mxs_peer_connect need mxs_halo_setup first) answer MXS_E_STATE.  A refused call changes nothing. */
int mxs_track_best(mxs_engine *e, int32_t every, double infinity, int32_t trace_capacity);
/* The record; any out pointer may be NULL; idx [n_vars] in the caller's variable order.  MXS_E_STATE when not tracking. */
int mxs_get_best(mxs_engine *e, int64_t *cycle, double *cost, int64_t *violations, int32_t *idx);
/* The first min(evaluations, trace_capacity, capacity) trace entries, their number in *n, and the number of
 * evaluations made since the trace was cleared in *evaluations.  The arrays may be NULL when capacity is 0.
 * MXS_E_STATE when not tracking; capacity < 0: MXS_E_INVALID. */
int mxs_get_cost_trace(mxs_engine *e, int64_t *cycle, double *cost, int64_t *violations, int32_t capacity, int32_t *n,
                       int64_t *evaluations);

#endif /* MAXSUM_GPU_ANYTIME_H */
