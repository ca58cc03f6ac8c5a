/*
 * g2048_ntuple.h -- the part of the C ABI of libg2048.so (include/g2048.h, which includes this file) that plays and
 * trains an n-tuple value network: whole episodes in persistent launches (the calls of g2048_scripted.h with the
 * network's player in the script's place), the player's choice and the network's value on arbitrary boards, and the
 * batched afterstate TD(0) update on a recorded trajectory.  Include g2048.h, not this file: it uses the types and
 * constants declared there.  Additive: the ABI is still 17.
 *
 * The model (all integers).  A board is N x N exponents e[cell], cell = r N + c, 0 = empty, 2 <= N <= 8; actions 0 up,
 * 1 right, 2 down, 3 left; move(b, a) is the env's slide / merge without the spawn; a is valid iff move(b, a) != b;
 * g(b, a) = the sum of the merged tiles' values (the game's score gain), 0 for an invalid move.
 *   fixed point   F = G2048_NTUPLE_FRAC_BITS = 10 fractional bits: a reward in value units is g << F
 *   feature f     (offset_f, k_f, cells_f[k_f]): k_f distinct cells, 2 <= k_f <= 6, and a table of 16^k_f int32 weights
 *                 at w[offset_f ..].  The device knows nothing of symmetry: the caller lists every feature (the 8
 *                 dihedral images of a base tuple share its offset), at most G2048_NTUPLE_MAX_FEATURES of them.
 *   index_f(m)    = sum_j e[cells_f[j]] 16^j
 *   V(m)          = sum_f w[offset_f + index_f(m)]                                        (int64)
 *   Q_0(b, a)     = (g(b, a) << F) + V(move(b, a))                                        for valid a
 *   V'(s)         = max over valid a' of Q_0(s, a'), 0 when none is valid
 *   Q_1(b, a)     = (g << F) + floor(sum over the empty cells c of m of [9 V'(m + 2 at c) + V'(m + 4 at c)]
 *                                    / (10 #empty(m))),  m = move(b, a); floor rounds toward minus infinity
 * The choice is the valid action with the largest Q_depth(b, a); ties go to the lowest action; a board with no valid
 * action gives action 0.  Invalid entries of q are INT64_MIN (Q may be negative).  The player computes validity itself
 * (cfg->use_action_mask may be 0 or 1), never chooses an invalid action and never draws from the policy stream:
 * pol_state / pol_buf are left byte for byte as they were.
 *
 * TD(0) on afterstates, for a time-major trajectory batch (row t of episode i at t n + i, valid iff t < lengths[i]);
 * every V below is taken with the weights as they were before the call:
 *   m_t = move(board_t, a_t), g_t = g(board_t, a_t)            (an invalid recorded action: m_t = board_t, g_t = 0)
 *   y_t = (g_{t+1} << F) + V(m_{t+1})  for t < L_i - 1;  y_t = 0 for t = L_i - 1 when that row's flags have
 *         G2048_F_TERMINATED;  a last row without it (truncated) is skipped
 *   d_t = y_t - V(m_t);  step_t = clamp(floor(d_t lr_num / 2^lr_shift), -2^30, 2^30)
 *   for every feature f: w[offset_f + index_f(m_t)] += step_t                    (an int32 add that wraps)
 * Integer adds commute, so the result does not depend on the order in which rows arrive.
 */
#ifndef G2048_NTUPLE_H
#define G2048_NTUPLE_H

#ifndef G2048_H
#error "include g2048.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define G2048_NTUPLE_FRAC_BITS 10
#define G2048_NTUPLE_MAX_DEPTH 1
#define G2048_NTUPLE_MIN_CELLS 2
#define G2048_NTUPLE_MAX_CELLS 6
#define G2048_NTUPLE_MAX_FEATURES 128
#define G2048_NTUPLE_MAX_LR_NUM 65536
#define G2048_NTUPLE_MAX_LR_SHIFT 40

typedef struct g2048_ntuple_feature {
    uint32_t offset;                          /* first weight of the feature's table */
    uint8_t k;                                /* cells used: 2..6 */
    uint8_t cells[G2048_NTUPLE_MAX_CELLS];    /* distinct, each < N^2; entries past k are ignored */
    uint8_t reserved;
} g2048_ntuple_feature;

typedef struct g2048_ntuple {
    int32_t depth;                            /* 0..G2048_NTUPLE_MAX_DEPTH (the update and values ignore it) */
    int32_t n_features;                       /* 1..G2048_NTUPLE_MAX_FEATURES */
    const g2048_ntuple_feature* features;     /* HOST memory: read and checked by the call, copied into the launch */
    int32_t* weights;                         /* DEVICE memory: n_weights int32 */
    int64_t n_weights;
} g2048_ntuple;

/* g2048_scripted_rollout / g2048_scripted_eval / g2048_sized_scripted_rollout / g2048_sized_scripted_eval with the
 * network's player in the script's place: the same rows, per-episode outputs, queue, order, resume, suspension at cap /
 * step_limit, traj->probs == NULL and max_workgroups.  G2048_EINVAL before any HIP call for a NULL descriptor, feature
 * list or weight pointer, a depth outside 0..1, n_features outside 1..128, a k outside 2..6, a cell >= N^2, a repeated
 * cell in a tuple, an offset + 16^k beyond n_weights, a size outside 2..8 and for whatever the scripted calls reject
 * that still applies; n_order == 0 returns G2048_OK without a launch. */
int g2048_ntuple_rollout(const g2048_ntuple* net, const g2048_env_cfg* cfg, uint64_t* env_state,
                         const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                         uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                         const g2048_suspend* sus, int64_t n, int64_t cap, const g2048_traj* traj, int max_workgroups,
                         void* stream);
int g2048_ntuple_eval(const g2048_ntuple* net, const g2048_env_cfg* cfg, uint64_t* env_state,
                      const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                      uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                      const g2048_suspend* sus, int64_t n, int64_t step_limit, const g2048_eval_out* out,
                      int max_workgroups, void* stream);
int g2048_sized_ntuple_rollout(int size, const g2048_ntuple* net, const g2048_env_cfg* cfg, uint64_t* env_state,
                               const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                               uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                               const g2048_suspend* sus, int64_t n, int64_t cap, const g2048_traj* traj,
                               int64_t board_stride, int max_workgroups, void* stream);
int g2048_sized_ntuple_eval(int size, const g2048_ntuple* net, const g2048_env_cfg* cfg, uint64_t* env_state,
                            const uint64_t* env_inc, uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc,
                            uint64_t* pol_buf, uint32_t* queue, const int32_t* order, int64_t n_order, int resume,
                            const g2048_suspend* sus, int64_t n, int64_t step_limit, const g2048_eval_out* out,
                            int max_workgroups, void* stream);

/* The player's choice on n boards, one board per thread: actions[i] = the choice on boards[i], q[4 i + a] = Q_depth
 * (boards[i], a), INT64_MIN for an invalid a (q may be NULL).  boards: n bitboards; the sized form takes [W, n] planes
 * of stride n (W = g2048_sized_words(size)).  G2048_EINVAL before any HIP call for a bad descriptor (above), NULL
 * boards / actions, n outside 0..2^31-1 and a size outside 2..8; n == 0 returns G2048_OK without a launch. */
int g2048_ntuple_choose(const g2048_ntuple* net, const uint64_t* boards, int64_t n, uint8_t* actions, int64_t* q,
                        void* stream);
int g2048_sized_ntuple_choose(int size, const g2048_ntuple* net, const uint64_t* boards, int64_t n, uint8_t* actions,
                              int64_t* q, void* stream);

/* values[i] = V(boards[i]) for n boards (the board itself, no move), one board per thread; arguments and errors as
 * the choose calls' (values must not be NULL; net->depth must still be valid). */
int g2048_ntuple_values(const g2048_ntuple* net, const uint64_t* boards, int64_t n, int64_t* values, void* stream);
int g2048_sized_ntuple_values(int size, const g2048_ntuple* net, const uint64_t* boards, int64_t n, int64_t* values,
                              void* stream);

/* One TD(0) update of net->weights, in place, from a time-major batch of n episodes and T rows: boards [T, n]
 * bitboards (sized: [W, T, n] planes, board_stride >= T n elements apart), actions [T, n] uint8, flags [T, n] uint8
 * (G2048_F_*), lengths [n] int32 (each 0..T).  scratch: 2 T n int64 of device memory (the first pass writes V(m_t) and
 * (g_t << F) + V(m_t) of every row there; the second pass reads them and no weight, so no V sees a write of the same
 * call).  stats: 2 int64 of device memory, written by the call: the number of rows updated and the sum of |d_t|.
 * G2048_EINVAL before any HIP call for a bad descriptor (above), a NULL buffer, lr_num outside 1..65536, lr_shift
 * outside 0..40, n or T outside 0..2^31-1, T n above 2^40, a board_stride below T n and a size outside 2..8; n == 0 or
 * T == 0 returns G2048_OK without a launch (stats is then not written). */
int g2048_ntuple_td_update(const g2048_ntuple* net, const uint64_t* boards, const uint8_t* actions,
                           const uint8_t* flags, const int32_t* lengths, int64_t n, int64_t T, int32_t lr_num,
                           int32_t lr_shift, int64_t* scratch, int64_t* stats, void* stream);
int g2048_sized_ntuple_td_update(int size, const g2048_ntuple* net, const uint64_t* boards, int64_t board_stride,
                                 const uint8_t* actions, const uint8_t* flags, const int32_t* lengths, int64_t n,
                                 int64_t T, int32_t lr_num, int32_t lr_shift, int64_t* scratch, int64_t* stats,
                                 void* stream);

#ifdef __cplusplus
}
#endif

#endif /* G2048_NTUPLE_H */
