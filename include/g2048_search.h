/*
 * g2048_search.h -- the part of the C ABI of libg2048.so (include/g2048.h, which includes this file) that plays an
 * expectimax lookahead player: whole episodes in persistent launches (the calls of g2048_scripted.h with a search
 * player in the script's place) and the player's choice on arbitrary boards.  Include g2048.h, not this file: it uses
 * the types and constants declared there.  Additive: the ABI is still 17.
 *
 * The player (all integers; int64, every value >= 0 and below 2^37).  A board is N x N exponents e[r][c], 0 = empty;
 * actions 0 up, 1 right, 2 down, 3 left; move(b, a) is the env's slide / merge without the spawn; a is valid iff
 * move(b, a) != b.
 *   gain(b, a) = sum of log2(v) over the tiles v created by merges in move(b, a)
 *   H(b)       = w_empty #empty(b)
 *                + w_smooth sum over horizontally and vertically adjacent cell pairs of (15 - |e_i - e_j|)
 *                + w_corner sum_{r,c} e[r][c] ((N-1-r) + (N-1-c))
 *   C_0(m)     = H(m)
 *   C_d(m)     = floor(sum over the empty cells c of m of [9 V_{d-1}(m with exponent 1 at c)
 *                                                          + V_{d-1}(m with exponent 2 at c)] / (10 #empty(m)))
 *   Q_d(b, a)  = w_merge gain(b, a) + C_d(move(b, a))    for valid a
 *   V_d(b)     = max over valid a of Q_d(b, a), 0 when no action is valid
 * The choice is the valid action with the largest Q_depth(b, a); ties go to the lowest action.  The player computes
 * validity itself (cfg->use_action_mask may be 0 or 1), never chooses an invalid action and never draws from the
 * policy stream: pol_state / pol_buf are left byte for byte as they were.  Boards holding a 2^15 tile are outside the
 * pinned domain (a 15 + 15 merge saturates here).
 */
#ifndef G2048_SEARCH_H
#define G2048_SEARCH_H

#ifndef G2048_H
#error "include g2048.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define G2048_SEARCH_MAX_DEPTH 2
#define G2048_SEARCH_MAX_WEIGHT 4096
typedef struct g2048_search {
    int32_t depth;                                  /* 0..G2048_SEARCH_MAX_DEPTH */
    uint32_t w_merge, w_empty, w_smooth, w_corner;  /* each 0..G2048_SEARCH_MAX_WEIGHT */
} g2048_search;

/* g2048_scripted_rollout / g2048_scripted_eval / g2048_sized_scripted_rollout / g2048_sized_scripted_eval with the
 * search player in the script's place: the same rows, per-episode outputs, queue, order, resume, suspension at cap /
 * step_limit, traj->probs == NULL and max_workgroups (workgroups of G2048_SCRIPT_BLOCK lanes, one episode per lane).
 * G2048_EINVAL before any HIP call for a NULL search, a depth outside 0..2, a weight above 4096 and for whatever the
 * scripted calls reject that still applies; n_order == 0 returns G2048_OK without a launch. */
int g2048_search_rollout(const g2048_search* search, const g2048_env_cfg* cfg, uint64_t* env_state,
                         const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                         uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                         const g2048_suspend* sus, int64_t n, int64_t cap, const g2048_traj* traj, int max_workgroups,
                         void* stream);
int g2048_search_eval(const g2048_search* search, const g2048_env_cfg* cfg, uint64_t* env_state,
                      const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                      uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                      const g2048_suspend* sus, int64_t n, int64_t step_limit, const g2048_eval_out* out,
                      int max_workgroups, void* stream);
int g2048_sized_search_rollout(int size, const g2048_search* search, const g2048_env_cfg* cfg, uint64_t* env_state,
                               const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                               uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                               const g2048_suspend* sus, int64_t n, int64_t cap, const g2048_traj* traj,
                               int64_t board_stride, int max_workgroups, void* stream);
int g2048_sized_search_eval(int size, const g2048_search* search, const g2048_env_cfg* cfg, uint64_t* env_state,
                            const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                            uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                            const g2048_suspend* sus, int64_t n, int64_t step_limit, const g2048_eval_out* out,
                            int max_workgroups, void* stream);

/* The player's choice on n boards, one board per thread: actions[i] = the choice on boards[i], q[4 i + a] = Q_depth
 * (boards[i], a), -1 for an invalid a (q may be NULL).  A board with no valid action gives action 0 and q all -1.
 * boards: n bitboards; the sized form takes [W, n] planes of stride n (W = g2048_sized_words(size)).
 * G2048_EINVAL before any HIP call for a NULL search / boards / actions, a bad depth or weight, n outside 0..2^31-1
 * and a size outside 2..8; n == 0 returns G2048_OK without a launch. */
int g2048_search_choose(const g2048_search* search, const uint64_t* boards, int64_t n, uint8_t* actions, int64_t* q,
                        void* stream);
int g2048_sized_search_choose(int size, const g2048_search* search, const uint64_t* boards, int64_t n, uint8_t* actions,
                              int64_t* q, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* G2048_SEARCH_H */
