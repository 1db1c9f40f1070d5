/* Max-Sum's end condition, detected on the device: the declarations.
 * A header of its own on top of maxsum_gpu.h (which it includes).  Exported by the same library under the same
 * mxs_version: a binding that needs these looks the symbols up (pydcop_amd/engine.py does, and says which are missing). */
#ifndef MAXSUM_GPU_QUIESCENCE_H
#define MAXSUM_GPU_QUIESCENCE_H

#include "maxsum_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* QUIESCENCE.  The send rule silences a directed edge once its message has matched SAME_COUNT (4) times.  A cycle in
 * which NO directed edge sends leaves every message, counter, selection and belief as it was, so every later cycle is
 * that cycle again: the run has ended.  A send counter is 4 after a silent cycle and after a fourth send alike, so the
 * criterion takes two consecutive looks and is exact:
 *     cycle c sent nothing  <=>  all 2*E send counters are 4 after cycle c-1 and after cycle c.
 * every = W > 0 switches watching on: a CHECK (the number of counters != 4, `active`) is made on the device after every
 * cycle c with c % W == 0 or c % W == 1 (c: the engine's cycle count; W = 1: every cycle), with no read-back.  The first
 * check at a cycle c with active == 0 whose predecessor c-1 was checked with active == 0 too sets the quiescent cycle to
 * c; it is never overwritten.  With t* the first cycle that sent nothing, that is t* for W <= 2 and the smallest
 * c >= t* with c % W == 1 otherwise.  The state as it is when watching is switched on is not checked.  The result
 * depends on the sequence of cycles alone: not on how the cycles are split over calls, not on which of mxs_run /
 * _run_async / _run_timed / _run_reps made them, not on mxs_params.graph_chunk.  No atomics: the same bits from run to
 * run.  Cycles after the quiescent one are still computed when asked for (they change nothing).
 *   every == 0 switches watching off and frees the buffers; every > 0 on a watching engine starts again (checks = 0).
 * mxs_reset, mxs_set_state, mxs_update_factor_table, mxs_set_parent_table and mxs_slice_factor end the fixed point:
 * each clears the quiescent cycle (the number of checks is kept) and detection starts again from there.
 *   MXS_E_INVALID: every < 0.  MXS_E_STATE: a sharded engine (mxs_halo_setup, mxs_comm_init or mxs_peer_connect has been
 * called: a shard sees its own edges only).  While watching, mxs_debug_timeline, mxs_step_compute / _pack / _unpack and
 * mxs_halo_setup answer MXS_E_STATE.  A refused call changes nothing. */
int mxs_watch_quiescence(mxs_engine *e, int32_t every);
/* One small copy from the device and nothing else; any out pointer may be NULL.  *quiescent: 0 / 1; *cycle: the
 * quiescent cycle, -1 while there is none; *checks: checks made since watching was switched on; *active: the counters
 * != 4 at the last check; *last_check_cycle: its cycle, -1 before the first.  MXS_E_STATE when not watching. */
int mxs_quiescence(mxs_engine *e, int32_t *quiescent, int64_t *cycle, int64_t *checks, int64_t *active,
                   int64_t *last_check_cycle);
/* Runs spans of `poll` cycles (poll <= 0: the larger of 64 and twice the captured chunk) and reads the state after each;
 * stops at the first span end with a quiescent cycle, or after max_cycles.  *cycles_run: the cycles this call ran,
 * min(max_cycles, the smallest multiple of poll >= the detection cycle - the cycle count at the call); 0, running
 * nothing, when the engine is quiescent already.  MXS_E_STATE when not watching; max_cycles < 0: MXS_E_INVALID. */
int mxs_run_until_quiescent(mxs_engine *e, int32_t max_cycles, int32_t poll, int32_t *quiescent, int64_t *cycle,
                            int64_t *cycles_run);

#ifdef __cplusplus
}
#endif

#endif /* MAXSUM_GPU_QUIESCENCE_H */
