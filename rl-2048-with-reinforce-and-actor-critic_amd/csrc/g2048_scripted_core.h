// g2048_scripted_core.h -- scripted play (ReinforceAgent.run_episode with an action_gen, src/reinforce_agent.py:126-252,
// for the generators of tools/simple_action_gen.py): the scripted choice and one iteration of the episode loop, on top
// of g2048_core.h (4 x 4) and g2048_sized_core.h (sizes 2..8).  Shared by the gfx950 kernels (g2048_scripted_kernel.h)
// and the CPU test harness (tests/native/scripted_host.cpp, test-only).  Nothing here allocates or launches.
//
// A scripted episode needs no net: the action comes from the board's action mask alone (PRIORITY: the first action of
// a fixed order that the mask allows -- select_action accepts a valid candidate as it is and never draws), or from the
// mask and one draw of the episode's policy stream (UNIFORM: select_action's Generator.choice on the probabilities of
// a net whose logits are all equal).
#pragma once
#include "g2048_core.h"
#include "g2048_sized_core.h"

// G2048_HD for a static member function (the host form of G2048_HD is itself `static inline`)
#ifdef __HIPCC__
#define G2048_HDM __host__ __device__ static inline
#else
#define G2048_HDM static inline
#endif

namespace g2048 {
namespace scripted {

constexpr int32_t kPriority = 0, kUniform = 1;   // G2048_SCRIPT_* of include/g2048_scripted.h

// the four actions of a priority order in one word, entry i in byte i
G2048_HD uint32_t order_word(const uint8_t o[4]) {
    return (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24);
}

// a permutation of (0, 1, 2, 3)
G2048_HD bool order_ok(const uint8_t o[4]) {
    uint32_t seen = 0;
    for (int i = 0; i < 4; i++) {
        if (o[i] > 3) return false;
        seen |= 1u << o[i];
    }
    return seen == 15u;
}

// action_gen_1 / action_gen_2 (tools/simple_action_gen.py): the first entry of the order whose bit is set in the mask
// (bit a = action a changes the board).  A live episode's board always has a valid move; mask 0 gives entry 0.
G2048_HD uint32_t priority_choice(uint32_t ow, uint32_t mask_bits) {
    uint32_t act = ow & 3u;
#pragma unroll
    for (int i = 3; i >= 0; i--) {
        const uint32_t a = (ow >> (8 * i)) & 3u;
        act = ((mask_bits >> a) & 1u) ? a : act;
    }
    return act;
}

// select_action (src/reinforce_agent.py:178-190) for equal logits: p[a] = fp32(1) / fp32(k) on the k allowed actions
// (all four without a mask), 0 elsewhere -- what logits_to_probs (src/MLP.py:139-156) gives in fp32 -- then
// Generator.choice(4, p) on the draw u: softmax_select's cdf arithmetic.
G2048_HD uint32_t uniform_choice(uint32_t mask_bits, bool has_mask, double u, float p[4]) {
    const uint32_t mb = has_mask ? (mask_bits & 15u) : 15u;
    const float q = 1.0f / (float)popc64((uint64_t)mb);
#pragma unroll
    for (int k = 0; k < 4; k++) p[k] = ((mb >> k) & 1u) ? q : 0.0f;
    double cdf[4], acc = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        acc += (double)p[k];
        cdf[k] = acc;
    }
    uint32_t act = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) act += (cdf[k] / cdf[3] <= u) ? 1u : 0u;
    return act;
}

// ---------------------------------------------------------------------------------------------------------------
// The two games behind one interface: kWords board words, fresh (Game2048.reset: two spawns on the env stream), mask
// (bit a = action a changes the board), step (one Game2048Env.step; sc = the step count before it), and the two pieces
// of a step a lookahead needs on their own: move and put.
// ---------------------------------------------------------------------------------------------------------------

// 4 x 4: the bitboard of g2048_core.h.  The move is board_move_alu -- no row table, so no LDS and no g2048_init --
// followed by env_step_pcg's own sequence (spawn if changed, done, reward, truncation).
struct Game4 {
    static constexpr int kWords = 1;
    static constexpr int kSize = 4;
    G2048_HDM void fresh(uint64_t (&bw)[1], Pcg64& g) { bw[0] = spawn_pcg(spawn_pcg(0ull, g), g); }
    G2048_HDM uint32_t mask(const uint64_t (&bw)[1]) { return bits_mask(board_bits(bw[0])); }
    G2048_HDM void step(uint64_t (&bw)[1], uint32_t a, uint32_t sc, uint32_t& mt, Pcg64& g, const RewardCfg& rc,
                              int64_t max_steps, double& reward, uint32_t& flags) {
        const uint64_t b = bw[0];
        MoveSummary s;
        uint64_t m = board_move_alu<false>(b, a, s);
        const bool changed = m != b;
        if (changed) m = spawn_pcg(m, g);
        const BoardBits bits = board_bits(m);
        const bool done = bits_done(bits);
        const bool invalid = !changed && !done;
        reward = env_reward(rc, s, m, done, invalid, mt);
        const bool trunc = max_steps >= 0 && (int64_t)(sc + 1u) >= max_steps && !done;
        flags = (changed ? kFChanged : 0u) | (done ? kFTerminated : 0u) | (trunc ? kFTruncated : 0u) |
                (invalid ? kFInvalid : 0u) | (s.overflow ? kFOverflow : 0u);
        bw[0] = m;
    }
    // the slide / merge alone (no spawn): out = move(bw, a), sum_e = the log2 sum of the merged tiles; true iff the
    // board changed.  put: exponent e into the empty cell `cell`.  (The search player, g2048_search_core.h.)
    G2048_HDM bool move(const uint64_t (&bw)[1], uint32_t a, uint64_t (&out)[1], uint32_t& sum_e) {
        MoveSummary s;
        out[0] = board_move_alu<false>(bw[0], a, s);
        sum_e = s.sum_e;
        return out[0] != bw[0];
    }
    G2048_HDM void put(uint64_t (&bw)[1], uint32_t cell, uint32_t e) { bw[0] |= (uint64_t)e << (4u * cell); }
};

// N x N, 2 <= N <= 8: the word planes of g2048_sized_core.h
template <int N>
struct GameN {
    static constexpr int kWords = sized::Dim<N>::kWords;
    static constexpr int kSize = N;
    G2048_HDM sized::Board<N> load(const uint64_t (&bw)[kWords]) {
        sized::Board<N> b;
#pragma unroll
        for (int w = 0; w < kWords; w++) b.w[w] = bw[w];
        return b;
    }
    G2048_HDM void fresh(uint64_t (&bw)[kWords], Pcg64& g) {
        sized::Board<N> b;
#pragma unroll
        for (int w = 0; w < kWords; w++) b.w[w] = 0ull;
        sized::spawn_pcg<N>(b, g);
        sized::spawn_pcg<N>(b, g);
#pragma unroll
        for (int w = 0; w < kWords; w++) bw[w] = b.w[w];
    }
    G2048_HDM uint32_t mask(const uint64_t (&bw)[kWords]) { return sized::action_mask<N>(load(bw)); }
    G2048_HDM void step(uint64_t (&bw)[kWords], uint32_t a, uint32_t sc, uint32_t& mt, Pcg64& g,
                              const RewardCfg& rc, int64_t max_steps, double& reward, uint32_t& flags) {
        const sized::StepValues<N> o =
            sized::env_step<N, 0, false>(load(bw), a, sc + 1u, mt, g, 0ull, 0ull, rc, max_steps, nullptr);
#pragma unroll
        for (int w = 0; w < kWords; w++) bw[w] = o.board.w[w];
        reward = o.reward;
        flags = o.flags;
    }
    // as Game4's
    G2048_HDM bool move(const uint64_t (&bw)[kWords], uint32_t a, uint64_t (&out)[kWords], uint32_t& sum_e) {
        MoveSummary s;
        const sized::Board<N> m = sized::board_move<N, false>(load(bw), a, s, nullptr);
        bool changed = false;
#pragma unroll
        for (int w = 0; w < kWords; w++) {
            out[w] = m.w[w];
            changed = changed || m.w[w] != bw[w];
        }
        sum_e = s.sum_e;
        return changed;
    }
    G2048_HDM void put(uint64_t (&bw)[kWords], uint32_t cell, uint32_t e) {
        const uint32_t word = cell >> 4, sh = 4u * (cell & 15u);
#pragma unroll
        for (int w = 0; w < kWords; w++) bw[w] |= word == (uint32_t)w ? (uint64_t)e << sh : 0ull;
    }
};

// the script of a launch: kind and, for PRIORITY, order_word of its order
struct Script {
    int32_t kind;
    uint32_t order;
};

// an episode in values: the board, the steps played (t: rows written, sc: Game2048Env._step_count -- equal here),
// log2(max_tile_seen), the fp64 total in step order and the two streams of run_episode
template <class G>
struct Episode {
    uint64_t bw[G::kWords];
    uint32_t t, sc, mt;
    double total;
    Pcg64 ge, gp;
};

// one trajectory row: the board before the step, the action, the fp64 reward and the step's flags
template <class G>
struct Row {
    uint64_t bw[G::kWords];
    uint32_t action, flags;
    double reward;
};

// env.reset(seed=env_seed) of run_episode (src/reinforce_agent.py:209): ge / gp hold default_rng(env_seed) /
// default_rng(policy_seed)
template <class G>
G2048_HD void episode_reset(Episode<G>& e) {
    G::fresh(e.bw, e.ge);
    e.t = 0;
    e.sc = 0;
    e.mt = 2;      // max_tile_seen = 4 (src/env.py:188)
    e.total = 0.0;
}

// One iteration of run_episode's loop (src/reinforce_agent.py:214-238): choose (PRIORITY: the mask alone, the policy
// stream untouched; UNIFORM: one Generator.random() of the policy stream, also when one action is allowed), step, add
// the reward to the total.  Returns true when the episode ended (terminated or truncated) with this step.
template <class G>
G2048_HD bool episode_step(Episode<G>& e, const Script& s, const RewardCfg& rc, int64_t max_steps, bool use_mask,
                           Row<G>& row) {
    const uint32_t mb = G::mask(e.bw);
    uint32_t act;
    if (s.kind == kPriority) {
        act = priority_choice(s.order, mb);
    } else {
        float p[4];
        act = uniform_choice(mb, use_mask, pcg_random(e.gp), p);
    }
#pragma unroll
    for (int w = 0; w < G::kWords; w++) row.bw[w] = e.bw[w];
    G::step(e.bw, act, e.sc, e.mt, e.ge, rc, max_steps, row.reward, row.flags);
    row.action = act;
    e.sc += 1u;
    e.t += 1u;
    e.total += row.reward;      // total_reward += float(reward) (src/reinforce_agent.py:233)
    return (row.flags & (kFTerminated | kFTruncated)) != 0u;
}

}  // namespace scripted
}  // namespace g2048
