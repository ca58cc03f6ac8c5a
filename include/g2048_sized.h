/*
 * g2048_sized.h -- the part of the C ABI of libg2048.so (include/g2048.h, which includes this file) that serves
 * board sizes other than 4.  Include g2048.h, not this file: it uses the types and constants declared there.
 */
#ifndef G2048_SIZED_H
#define G2048_SIZED_H

#ifndef G2048_H
#error "include g2048.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- board sizes 2..8 (g2048_sized.hip; ABI 17) -------------------------------------------------------------------
 * Game2048 / Game2048Env for Game2048EnvConfig.size = N, 2 <= N <= 8 (src/game2048.py never assumes 4).  Board
 * encoding: cell k = r*N + c lives in nibble (k & 15) of word (k >> 4), W = g2048_sized_words(N) = ceil(N*N / 16)
 * uint64 words per board (1 for N <= 4, 2 for 5, 3 for 6, 4 for 7 and 8); unused high nibbles are 0; saturation at
 * 2**15 and G2048_F_OVERFLOW as above.  Board buffers are plane-major: word w of lane i at buf[w * plane_stride + i],
 * plane_stride >= n given per buffer (so prev_board can be row t of a [W, cap, n] trajectory tensor with
 * plane_stride = cap * n).  Lines move in plain ALU (no row table; g2048_init is not needed).  The lane state word,
 * flag bits, seeds, PCG64 arrays, Philox counter / key scheme and every other argument are those of the 4 x 4
 * counterparts.  obs buffers are [n * N*N] (raw / log2) or [n * N*N*17] (one-hot, channel e of cell r*N+c at
 * (r*N+c)*17 + e) and must be 16-byte aligned.  Every entry point accepts N = 4 too (W = 1, same results as the 4 x 4
 * entry points; the product path does not use them).  A size outside 2..8, a plane_stride below the lanes it must
 * hold or n > 2^30 return G2048_EINVAL before any launch.
 *
 * The fused policy (g2048_sized_policy.hip; additive, ABI still 17): g2048_sized_policy is g2048_deep_policy for
 * these boards -- forward of 1..G2048_DEEP_MAX_HIDDEN hidden layers of 1..256 units on raw / log2 / one-hot obs,
 * masked softmax and the action choice, straight from the board planes (no obs buffer, no GEMM) -- on a net packed
 * by g2048_sized_pack.  Only layer 0 depends on the size: N*N features (raw / log2) or N*N cells of 17 one-hot
 * features against W_0's three exact bf16 planes, accumulated cell by cell; at N = 4 the results are
 * g2048_deep_policy's bit for bit. */
int g2048_sized_words(int size);   /* W, or -1 for an unsupported size */

/* g2048_step_out for sized boards: the same fields, except */
typedef struct g2048_sized_step_out {
    float* reward;
    uint8_t* flags;
    int8_t* mask;
    float* obs;
    uint8_t* merged;       /* [n][N*(N/2)] the exponent log2(v) of each merged tile of this step in the reference's
                              list order (board rotated clockwise 3 - action times, rows top to bottom, each left to
                              right: src/game2048.py:120-165), 0-terminated when shorter than N*(N/2) */
    uint64_t* prev_board;  /* planes of the board before the step, word w of lane i at [w * prev_stride + i] */
    double* reward64;
    uint32_t* score_add;
    uint8_t* mask_bits;
    int64_t prev_stride;   /* plane stride of prev_board (>= n; ignored when prev_board is NULL) */
} g2048_sized_step_out;

/* g2048_reset for size N: lanes->board holds W planes of plane_stride lanes. */
int g2048_sized_reset(int size, const g2048_lanes* lanes, int64_t plane_stride, const uint64_t* seeds,
                      const uint8_t* reset_mask, const g2048_env_cfg* cfg, int rng_mode, uint64_t philox_key,
                      int8_t* mask_out, float* obs_out, int64_t n, void* stream);
/* g2048_step for size N (one kernel: move, spawn, done, fp64 reward, flags, truncation, max_tile_seen, auto-reset). */
int g2048_sized_step(int size, const g2048_lanes* lanes, int64_t plane_stride, const uint8_t* actions,
                     const g2048_env_cfg* cfg, const g2048_sized_step_out* out, int rng_mode, uint64_t philox_key,
                     int auto_reset, uint64_t reset_stride, int64_t n, void* stream);
/* g2048_obs for size N. */
int g2048_sized_obs(int size, const uint64_t* boards, int64_t plane_stride, int obs_mode, float obs_log2_scale,
                    float* obs, int8_t* mask, int64_t n, void* stream);
/* g2048_move for size N: out_board planes of out_stride lanes; merged [n][N*(N/2)] as in g2048_sized_step_out. */
int g2048_sized_move(int size, const uint64_t* boards, int64_t plane_stride, const uint8_t* actions,
                     uint64_t* out_board, int64_t out_stride, uint8_t* merged, uint8_t* flags, int64_t n,
                     void* stream);
/* g2048_symmetries for size N: word w of symmetry k of lane i at out_boards[w * out_stride + k*n + i]
 * (out_stride >= 8n); out_actions [8n] symmetry-major (NULL ok). */
int g2048_sized_symmetries(int size, const uint64_t* boards, int64_t plane_stride, const uint8_t* actions,
                           uint64_t* out_boards, int64_t out_stride, uint8_t* out_actions, int64_t n, void* stream);


/* Floats in the packed net of g2048_sized_pack, or -1 when the shape is not covered (size 2..8; obs_mode raw, log2 or
 * one-hot; 1..G2048_DEEP_MAX_HIDDEN hidden layers of 1..256 units).  Host arithmetic only: it never touches the
 * device. */
int g2048_sized_policy_packed_size(int size, int obs_mode, int n_hidden, const int32_t* hidden);
/* g2048_deep_pack for size N: W_l [in, out] row-major (the reference layout), W_0 with N*N rows (raw / log2) or
 * N*N*17 rows (one-hot: row 17 k + e = cell k = r*N + c, exponent e); out_dim 4 (actor) or 1 (a value head, packed
 * as output 0). */
int g2048_sized_pack(int size, const float* const* W, const float* const* b, int obs_mode, int n_hidden,
                     const int32_t* hidden, int out_dim, float* packed, int64_t packed_len, void* stream);
/* g2048_deep_policy for size N on plane-major boards (word w of lane i at boards[w * plane_stride + i]); every other
 * argument and rule is g2048_deep_policy's: lane_index compaction (entry j -> lane lane_index[j]), lane_state
 * (lanes without G2048_LS_ACTIVE are left untouched; the Philox counter is the step count), use_mask, greedy,
 * rng_mode PCG64 / Philox, probs_out / logits_out [lanes][4], actions == NULL = forward only (logits_out; a value
 * head in column 0).  G2048_EINVAL before any launch for a size outside 2..8, plane_stride < n, n > 2^30 or a net
 * that g2048_sized_policy_packed_size does not cover; n == 0 returns G2048_OK without a launch. */
int g2048_sized_policy(int size, const float* packed, int n_hidden, const int32_t* hidden, int activation,
                       const uint64_t* boards, int64_t plane_stride, const uint32_t* lane_state,
                       const int32_t* lane_index, int obs_mode, float obs_scale, int use_mask, int greedy, int rng_mode,
                       uint64_t* rng_state, const uint64_t* rng_inc, const uint64_t* rng_buf, uint64_t philox_key,
                       const uint64_t* lane_seed, float* probs_out, float* logits_out, uint8_t* actions, int64_t n,
                       void* stream);

/* g2048_deep_rollout for size N (g2048_sized_rollout.hip; additive, ABI still 17): the whole batched rollout in
 * persistent launches for a net packed by g2048_sized_pack.  The contract is g2048_deep_rollout's: obs mode, obs
 * scale, use_action_mask, the reward config and max_steps come from cfg; both streams of every episode are numpy
 * PCG64 (g2048_seed_pcg64); episodes order[0 .. n_order) (NULL: 0 .. n-1, n_order = n) run to their end inside the
 * launch; one that reaches row cap without ending is suspended -- streams written back into env_* / pol_*, board,
 * meta and total into *sus, the episode listed in sus->list -- and is resumed by a later call with resume = 1, order
 * = the suspended list and the trajectory buffers grown (same n, larger cap; rows below the old cap kept).  queue:
 * one uint32, zero before each call.  A new episode starts from two spawns on an empty board with max tile exponent
 * 2, step count 0 and total 0.0.
 * Board buffers are plane-major: traj->boards holds word w of row t of episode e at [w * board_stride + t * n + e]
 * (board_stride >= cap * n: a [W, cap, n] tensor); traj->final_board and sus->board are [W, n] planes of stride n;
 * sus->meta and sus->total stay per episode.
 * max_workgroups: 0 = two workgroups per CU, further capped by ceil(n_order / 32); a positive value caps the grid
 * below that (a tuning knob: every workgroup runs 32 episode slots that refill from the queue).
 * G2048_EINVAL before any HIP call for a size outside 2..8, a net g2048_sized_policy_packed_size does not cover,
 * board_stride < cap * n, bad n / cap / order (g2048_deep_rollout's rules), a NULL required buffer or a negative
 * max_workgroups; n_order == 0 returns G2048_OK without a launch. */
int g2048_sized_rollout(int size, const float* packed, int n_hidden, const int32_t* hidden, int activation,
                        const g2048_env_cfg* cfg, int greedy, uint64_t* env_state, const uint64_t* env_inc,
                        uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc, uint64_t* pol_buf,
                        uint32_t* queue, const int32_t* order, int64_t n_order, int resume, const g2048_suspend* sus,
                        int64_t n, int64_t cap, const g2048_traj* traj, int64_t board_stride, int max_workgroups,
                        void* stream);
/* g2048_deep_eval for size N (g2048_sized_eval.hip; additive, ABI still 17): g2048_sized_rollout's kernels with the
 * trajectory row stores compiled out, so the same episodes and memory that does not depend on their lengths.
 * step_limit (1 .. 2^31 - 1) is the absolute step count at which an episode still running is suspended in this call
 * (g2048_eval.h); there is no board_stride and no n * step_limit limit.  out->final_board and sus->board are [W, n]
 * planes of stride n.  Every other argument and rule, max_workgroups and the grid included, is g2048_sized_rollout's;
 * G2048_EINVAL before any HIP call for whatever that rejects that still applies, for a NULL out or field of out and
 * for step_limit < 1; n_order == 0 returns G2048_OK without a launch.
 * g2048_eval_out is declared in g2048_eval.h, which g2048.h includes before this file. */
int g2048_sized_eval(int size, const float* packed, int n_hidden, const int32_t* hidden, int activation,
                     const g2048_env_cfg* cfg, int greedy, uint64_t* env_state, const uint64_t* env_inc,
                     uint64_t* env_buf, uint64_t* pol_state, const uint64_t* pol_inc, uint64_t* pol_buf,
                     uint32_t* queue, const int32_t* order, int64_t n_order, int resume, const g2048_suspend* sus,
                     int64_t n, int64_t step_limit, const g2048_eval_out* out, int max_workgroups, void* stream);

/* The fused gradient for size N (g2048_sized_grad.hip; additive, ABI still 17): g2048_deep_grad and g2048_onehot_dw1
 * for these boards -- update_batch's actor or critic gradient of n samples in one launch, straight from the board
 * planes, on a net packed by g2048_sized_pack (forward) and g2048_deep_grad_pack (the dense layers' backward
 * fragments: layers l >= 1 only, so they do not depend on the size).
 *
 * Coverage (g2048_sized_grad_slab >= 0): size 2..8; raw / log2 / one-hot obs; ReLU / Sigmoid; 1..4 hidden layers of
 * 1..256 units whose dense 32 x 32 weight-gradient tiles, sum over l >= 1 of ceil(H_{l-1} / 32) ceil(H_l / 32), number
 * at most 40 on one-hot obs (e.g. [256, 128, 64]) and at most 32 on raw / log2 (e.g. [256, 128]), and whose LDS bill
 * fits 160 KiB.  One launch only: there is no multi-launch form, and every other net returns -1 / G2048_EINVAL.
 *
 * Partial slab (floats; H_l p = H_l rounded up to 32; g2048_deep_grad's with layer 0 sized to the board):
 *   dW_0  [rows0][H_0 p]  raw / log2 only: rows0 = 32 ceil(N*N / 32) feature rows (32 for N <= 5, 64 for N >= 6), the
 *                         rows >= N*N zero; one-hot: absent (g2048_sized_onehot_dw1 forms it from d0_out)
 *   db_0  [H_0 p]
 *   dW_l  [H_{l-1} p][H_l p], db_l [H_l p]    for l = 1 .. L-1
 *   dW_out [H_{L-1} p][4], db_out [4]
 * g2048_sized_grad_layout returns these offsets.  Raw / log2 dW_0 is formed inside the kernel at every size (no
 * d0_out fall-back was needed: 0 spilled registers with both feature tiles held). */
/* Floats per partial slab, or -1 when the net is not covered.  Host arithmetic only. */
int g2048_sized_grad_slab(int size, int obs_mode, int n_hidden, const int32_t* hidden);
/* The workgroup count (nparts) that fills the device: one 8-wave workgroup per CU; -1 when not covered.  Unlike the
 * slab and layout queries this one touches the HIP runtime for a covered net (hipGetDevice / hipDeviceGetAttribute on
 * the current device's CU count) and answers 256 where no device can be asked. */
int g2048_sized_grad_parts(int size, int obs_mode, int n_hidden, const int32_t* hidden);
/* The slab layout: w_off[l] / b_off[l] (n_hidden + 1 entries each, NULL ok) = float offsets of dW_l / db_l, entry
 * n_hidden the output layer's; *dw0_rows = rows0 (0 on one-hot obs), *dw0_ld = H_0 p (NULL ok).  Returns the slab size
 * or -1 when not covered.  Host arithmetic only. */
int g2048_sized_grad_layout(int size, int obs_mode, int n_hidden, const int32_t* hidden, int32_t* w_off,
                            int32_t* b_off, int32_t* dw0_rows, int32_t* dw0_ld);
/* g2048_deep_grad for size N on plane-major boards (word w of sample j at boards[w * plane_stride + j]); the contract
 * is g2048_deep_grad's: critic = 0 the policy-gradient branch (actions, coef = advantage x step weight, the mask of
 * each board when use_mask), critic = 1 the value loss (loss 0 = MSE, 1 = Huber with huber_delta; coef = step weight;
 * target = r + gamma V(s') m; delta_out = target - V and value_out = V, [n], NULL ok); every one of the nparts
 * workgroups writes a complete slab into partials [nparts][slab], zeros when it gets no group of 32 samples, to be
 * summed by g2048_fold_partials.  There is no TD-row argument.  d0_out [n][H_0 p] is required on one-hot obs (layer
 * 0's deltas for g2048_sized_onehot_dw1) and ignored otherwise.
 * hidden_out (NULL ok; production calls pass NULL): n_hidden pointers, entry l (NULL ok) receives hidden layer l's
 * activations [n][H_l p] exactly as the kernel's forward computed them (stored after the forward, before the deltas
 * overwrite them) -- the kernel's own ReLU pattern, for tests and diagnostics.
 * G2048_EINVAL before any HIP call for a size outside 2..8, plane_stride < n, n < 0 or n > 2^30, a net
 * g2048_sized_grad_slab does not cover, a bad activation / obs mode / loss, nparts outside 1..65535 or a NULL
 * required buffer (packed, partials; grad_packed when n_hidden > 1; with n > 0: boards, coef, actions (actor), target
 * (critic), d0_out (one-hot)).  n == 0 returns G2048_OK without a launch: partials is left untouched. */
int g2048_sized_grad(int size, const float* packed, const float* grad_packed, int n_hidden, const int32_t* hidden,
                     int activation, int obs_mode, float obs_scale, int use_mask, const uint64_t* boards,
                     int64_t plane_stride, const uint8_t* actions, const float* coef, int critic, int loss,
                     float huber_delta, const float* target, float* delta_out, float* value_out, float* d0_out,
                     float* const* hidden_out, int64_t n, float* partials, int64_t nparts, void* stream);
/* Floats per partial slab of g2048_sized_onehot_dw1: (17 N*N + 1) h1 (17 N*N rows of dW_0, then db_0), or -1 for a
 * size outside 2..8 or h1 outside 1..256. */
int g2048_sized_onehot_dw1_slab(int size, int h1);
/* g2048_onehot_dw1 for size N: dW_0 / db_0 of a one-hot first layer from the board planes and the layer's deltas d1
 * [m][ld] (units < h1 <= ld).  Row 17 k + e of a slab is cell k = r*N + c, exponent e (g2048_sized_pack's row order;
 * rows 17 k + 16 are zero); workgroups (i, w) take samples [i per, (i + 1) per) and board word w, nparts = ceil(m /
 * per) slabs, summed by g2048_fold_partials.  Same arithmetic as g2048_onehot_dw1 (the exact one-hot operand against
 * each delta's three exact bf16 planes, fp32 accumulation in a fixed order: deterministic, no atomics).
 * G2048_EINVAL for a size outside 2..8, plane_stride < m, m > 2^30 and by g2048_onehot_dw1's rules; m == 0 returns
 * G2048_OK without a launch. */
int g2048_sized_onehot_dw1(int size, const uint64_t* boards, int64_t plane_stride, const float* d1, int h1, int64_t m,
                           int64_t ld, int64_t per, float* partials, int64_t nparts, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* G2048_SIZED_H */
