/*
 * g2048_scripted.h -- the part of the C ABI of libg2048.so (include/g2048.h, which includes this file) that plays
 * whole episodes for a scripted player instead of a net: ReinforceAgent.run_episode(env_seed, policy_seed,
 * action_gen=...) (src/reinforce_agent.py:126-252) for the generators of tools/simple_action_gen.py and for the
 * random-valid baseline.  Include g2048.h, not this file: it uses the types and constants declared there.  Additive:
 * the ABI is still 17.
 */
#ifndef G2048_SCRIPTED_H
#define G2048_SCRIPTED_H

#ifndef G2048_H
#error "include g2048.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* PRIORITY: the action is the first entry of `order` (a permutation of 0..3) whose bit is set in the board's action
 * mask -- action_gen_1 is order (0, 1, 2, 3), action_gen_2 (0, 1, 3, 2).  select_action takes a valid candidate as it
 * is, so the episode's policy stream is never drawn from: pol_state / pol_buf are left byte for byte as they were.
 * Needs cfg->use_action_mask.
 * UNIFORM: select_action for a net whose logits are all equal: p[a] = fp32(1) / fp32(k) on the k actions the mask
 * allows (all four without an action mask), 0 elsewhere; one Generator.random() of the episode's policy stream per
 * step (also when k = 1); the action is Generator.choice(4, p).  `order` is not read. */
#define G2048_SCRIPT_PRIORITY 0
#define G2048_SCRIPT_UNIFORM 1
typedef struct g2048_script {
    int32_t kind;        /* G2048_SCRIPT_* */
    uint8_t order[4];
} g2048_script;

/* threads, and so episodes in flight, of one workgroup of the scripted kernels (max_workgroups below counts these) */
#define G2048_SCRIPT_BLOCK 256

/* g2048_deep_rollout for a script: the same episodes' rows (boards pre-step, actions, fp64 rewards, flags), per-episode
 * outputs, suspension at row cap (streams written back, state in *sus, the episode listed), resume = 1 continuation
 * and queue (one uint32, zero before each call); traj->probs must be NULL.  One episode per lane of a persistent
 * launch; max_workgroups > 0 caps the grid (0: as many workgroups of G2048_SCRIPT_BLOCK lanes as n_order needs, at most
 * what is resident at once).  The move is computed in registers (no row table: g2048_init is not needed).
 * G2048_EINVAL before any HIP call for whatever g2048_deep_rollout rejects that still applies, and for a NULL script, a
 * kind outside {0, 1}, an order that is no permutation, PRIORITY with cfg->use_action_mask == 0, a non-NULL
 * traj->probs and max_workgroups < 0; n_order == 0 returns G2048_OK without a launch. */
int g2048_scripted_rollout(const g2048_script* script, const g2048_env_cfg* cfg, uint64_t* env_state,
                           const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                           uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                           const g2048_suspend* sus, int64_t n, int64_t cap, const g2048_traj* traj, int max_workgroups,
                           void* stream);

/* g2048_deep_eval for a script (the same kernel with its row stores compiled out): step_limit takes cap's place. */
int g2048_scripted_eval(const g2048_script* script, const g2048_env_cfg* cfg, uint64_t* env_state,
                        const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                        uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                        const g2048_suspend* sus, int64_t n, int64_t step_limit, const g2048_eval_out* out,
                        int max_workgroups, void* stream);

/* g2048_sized_rollout / g2048_sized_eval for a script: board sizes 2..8, boards as [W, cap, n] planes of stride
 * board_stride >= cap * n, final_board / sus->board [W, n] planes of stride n; otherwise as the two above. */
int g2048_sized_scripted_rollout(int size, const g2048_script* script, const g2048_env_cfg* cfg, uint64_t* env_state,
                                 const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state,
                                 const uint64_t* pol_inc, uint64_t* pol_buf, uint32_t* queue, const int32_t* order,
                                 int64_t n_order, int resume, const g2048_suspend* sus, int64_t n, int64_t cap,
                                 const g2048_traj* traj, int64_t board_stride, int max_workgroups, void* stream);
int g2048_sized_scripted_eval(int size, const g2048_script* script, const g2048_env_cfg* cfg, uint64_t* env_state,
                              const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                              uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                              const g2048_suspend* sus, int64_t n, int64_t step_limit, const g2048_eval_out* out,
                              int max_workgroups, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* G2048_SCRIPTED_H */
