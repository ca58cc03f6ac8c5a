/*
 * g2048_eval.h -- the part of the C ABI of libg2048.so (include/g2048.h, which includes this file) that plays
 * score-only rollouts: the episodes of the persistent rollout kernels without their trajectory rows.  Include
 * g2048.h, not this file: it uses the types and constants declared there.  Additive: the ABI is still 17.
 */
#ifndef G2048_EVAL_H
#define G2048_EVAL_H

#ifndef G2048_H
#error "include g2048.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* What a score-only rollout keeps of an episode (the per-episode fields of g2048_traj, same meaning): lengths (steps
 * played), totals (fp64 running sum of the rewards in step order, src/reinforce_agent.py:233), max_tile (log2 of
 * max_tile_seen), final_board.  Each [n]; g2048_sized_eval's final_board is [W, n] planes of stride n.  Only the
 * entries of episodes that end in the call are written. */
typedef struct g2048_eval_out {
    int32_t* lengths;
    double* totals;
    uint8_t* max_tile;
    uint64_t* final_board;
} g2048_eval_out;

/* g2048_rollout without the trajectory: the same kernel with its row stores compiled out (a second instantiation), so
 * the same episodes -- forward, choice, draws, env step and the fp64 total in step order -- and memory that does not
 * depend on the episodes' lengths.  Arguments and rules are g2048_rollout's minus the row buffers and cap: obs_mode
 * log2 / raw and cfg->max_steps >= 0 (the launch is bounded by max_steps: every episode ends by then); queue: one
 * uint32, zero before the call.  G2048_EINVAL before any HIP call for whatever g2048_rollout rejects that still
 * applies and for a NULL out or field of out; n == 0 returns G2048_OK without a launch. */
int g2048_rollout_eval(const float* packed, int h1, int h2, int activation, const g2048_env_cfg* cfg, int greedy,
                       const uint64_t* env_state, const uint64_t* env_inc, const uint64_t* env_buf,
                       const uint64_t* pol_state, const uint64_t* pol_inc, const uint64_t* pol_buf, uint32_t* queue,
                       int64_t n, const g2048_eval_out* out, void* stream);

/* g2048_deep_rollout without the trajectory (the score-only instantiations of its 32-slot and 64-slot kernels).
 * step_limit (1 .. 2^31 - 1) takes cap's place and is no row count: an episode whose absolute step count reaches
 * step_limit in this call without ending is suspended exactly as g2048_deep_rollout suspends at row cap -- streams
 * written back into env_* / pol_*, board, meta and total into *sus, the episode listed -- and a later call with
 * resume = 1, order = the suspended list and a larger step_limit plays it on.  Every launch is therefore bounded,
 * also for an episode that would never end, and nothing has to grow between launches.  There is no n * step_limit
 * limit.  Every other argument and rule, the grid included, is g2048_deep_rollout's.  G2048_EINVAL before any HIP call
 * for whatever that rejects that still applies, for a NULL out or field of out and for step_limit < 1; n_order == 0
 * returns G2048_OK without a launch. */
int g2048_deep_eval(const float* packed, int n_hidden, const int32_t* hidden, int activation, const g2048_env_cfg* cfg,
                    int greedy, uint64_t* env_state, const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state,
                    const uint64_t* pol_inc, uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order,
                    int resume, const g2048_suspend* sus, int64_t n, int64_t step_limit, const g2048_eval_out* out,
                    void* stream);

#ifdef __cplusplus
}
#endif

#endif /* G2048_EVAL_H */
