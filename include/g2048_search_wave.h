/*
 * g2048_search_wave.h -- the part of the C ABI of libg2048.so (include/g2048.h, which includes this file after
 * g2048_search.h) that plays the expectimax player of g2048_search.h wave-cooperatively: one episode, or one board, per
 * wave of 64 lanes instead of per lane, the chance children of its four moves spread over the lanes.  Include g2048.h,
 * not this file.  Additive: the ABI is still 17.
 *
 * The player is all integers and a chance node is a sum, so these calls give bit for bit what their per-lane siblings
 * give: the same rows, per-episode outputs, suspend state, actions and q.  What differs is the time.  A launch of few
 * episodes or boards (tens to a few thousand) finishes sooner here, because a step's chain of dependent work is
 * ceil(items / 64) children instead of all of them (items <= 8 (N^2 - 1)); a launch that fills the device one episode
 * per lane is faster through g2048_search.h.
 *
 * Each call has its sibling's exact signature and checks, and additionally returns G2048_EINVAL, before any HIP call,
 * for depth 0: there is no chance level to spread, so callers use the per-lane call.
 */
#ifndef G2048_SEARCH_WAVE_H
#define G2048_SEARCH_WAVE_H

#ifndef G2048_SEARCH_H
#error "include g2048.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* g2048_search_rollout / g2048_search_eval / g2048_sized_search_rollout / g2048_sized_search_eval with one episode per
 * wave: workgroups of G2048_SCRIPT_BLOCK threads play G2048_SCRIPT_BLOCK / 64 episodes at a time, and the grid is
 * min(ceil(n_order / 4), 8 per CU, max_workgroups when > 0).  n_order == 0 returns G2048_OK without a launch. */
int g2048_search_wave_rollout(const g2048_search* search, const g2048_env_cfg* cfg, uint64_t* env_state,
                              const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                              uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                              const g2048_suspend* sus, int64_t n, int64_t cap, const g2048_traj* traj,
                              int max_workgroups, void* stream);
int g2048_search_wave_eval(const g2048_search* search, const g2048_env_cfg* cfg, uint64_t* env_state,
                           const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                           uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                           const g2048_suspend* sus, int64_t n, int64_t step_limit, const g2048_eval_out* out,
                           int max_workgroups, void* stream);
int g2048_sized_search_wave_rollout(int size, const g2048_search* search, const g2048_env_cfg* cfg, uint64_t* env_state,
                                    const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state,
                                    const uint64_t* pol_inc, uint64_t* pol_buf, uint32_t* queue, const int32_t* order,
                                    int64_t n_order, int resume, const g2048_suspend* sus, int64_t n, int64_t cap,
                                    const g2048_traj* traj, int64_t board_stride, int max_workgroups, void* stream);
int g2048_sized_search_wave_eval(int size, const g2048_search* search, const g2048_env_cfg* cfg, uint64_t* env_state,
                                 const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state,
                                 const uint64_t* pol_inc, uint64_t* pol_buf, uint32_t* queue, const int32_t* order,
                                 int64_t n_order, int resume, const g2048_suspend* sus, int64_t n, int64_t step_limit,
                                 const g2048_eval_out* out, int max_workgroups, void* stream);

/* g2048_search_choose / g2048_sized_search_choose with one board per wave (a grid-stride loop over the boards).
 * n == 0 returns G2048_OK without a launch. */
int g2048_search_wave_choose(const g2048_search* search, const uint64_t* boards, int64_t n, uint8_t* actions,
                             int64_t* q, void* stream);
int g2048_sized_search_wave_choose(int size, const g2048_search* search, const uint64_t* boards, int64_t n,
                                   uint8_t* actions, int64_t* q, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* G2048_SEARCH_WAVE_H */
