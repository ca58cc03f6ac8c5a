// TEST-ONLY host build of csrc/g2048_scripted_core.h (the scripted choice and the episode loop body the gfx950 scripted
// kernels run), for tests/test_scripted_host.py: a shared library for ctypes.  "Play episode e for at most k steps from
// this state": the caller holds the episode's state (ScState: board words, counters, total, both PCG64 streams) the way
// the kernels' suspend protocol does, and sc_play continues it, writing one row per step.
#include <stdint.h>
#include <string.h>

#include "g2048_scripted_core.h"

using namespace g2048;
namespace sc = g2048::scripted;

namespace {

struct EpCfg {   // tests/native/sized_host.cpp's
    int32_t reward_mode, bonus_mode, use_action_mask, pad;
    double base_reward_scale, empty_tile_reward, merge_reward, bonus_scale, step_reward, endgame_penalty,
        invalid_action_penalty;
    int64_t max_steps;
};

RewardCfg reward_cfg(const EpCfg& c) {
    RewardCfg r;
    r.reward_mode = c.reward_mode;
    r.bonus_mode = c.bonus_mode;
    r.use_action_mask = c.use_action_mask;
    r.base_reward_scale = c.base_reward_scale;
    r.empty_tile_reward = c.empty_tile_reward;
    r.merge_reward = c.merge_reward;
    r.bonus_scale = c.bonus_scale;
    r.step_reward = c.step_reward;
    r.endgame_penalty = c.endgame_penalty;
    r.invalid_action_penalty = c.invalid_action_penalty;
    r.terms = reward_terms(r);
    return r;
}

struct ScStream {
    uint64_t s_lo, s_hi, i_lo, i_hi;
    uint32_t has_uint32, uinteger;
};

struct ScState {
    uint64_t board[4];
    uint32_t t, sc, mt, ended;
    double total;
    ScStream env, pol;
};

Pcg64 to_pcg(const ScStream& s) {
    Pcg64 g;
    g.s_lo = s.s_lo; g.s_hi = s.s_hi; g.i_lo = s.i_lo; g.i_hi = s.i_hi;
    g.has_uint32 = s.has_uint32; g.uinteger = s.uinteger;
    return g;
}

ScStream from_pcg(const Pcg64& g) { return ScStream{g.s_lo, g.s_hi, g.i_lo, g.i_hi, g.has_uint32, g.uinteger}; }

// fresh != 0: seed both streams (default_rng(env_seed) / default_rng(policy_seed)) and reset; else continue *st.
// Plays until the episode ends or k steps were played in this call; rows t0 .. t0 + played - 1 go to boards
// [k][kWords], actions, rewards, flags [k].  Returns the steps played; st->ended says whether the episode ended.
template <class G>
int64_t play(int kind, const uint8_t* order, const EpCfg* cfg, int fresh, uint64_t env_seed, uint64_t pol_seed,
             ScState* st, int64_t k, uint64_t* boards, uint8_t* actions, double* rewards, uint8_t* flags) {
    const RewardCfg rc = reward_cfg(*cfg);
    sc::Script s;
    s.kind = kind;
    s.order = kind == sc::kPriority ? sc::order_word(order) : 0u;
    sc::Episode<G> e{};
    if (fresh) {
        e.ge = pcg_seed(env_seed);
        e.gp = pcg_seed(pol_seed);
        sc::episode_reset<G>(e);
    } else {
        for (int w = 0; w < G::kWords; w++) e.bw[w] = st->board[w];
        e.t = st->t; e.sc = st->sc; e.mt = st->mt; e.total = st->total;
        e.ge = to_pcg(st->env);
        e.gp = to_pcg(st->pol);
    }
    int64_t played = 0;
    bool ended = false;
    while (!ended && played < k) {
        sc::Row<G> row;
        ended = sc::episode_step<G>(e, s, rc, cfg->max_steps, cfg->use_action_mask != 0, row);
        for (int w = 0; w < G::kWords; w++) boards[played * G::kWords + w] = row.bw[w];
        actions[played] = (uint8_t)row.action;
        rewards[played] = row.reward;
        flags[played] = (uint8_t)row.flags;
        played++;
    }
    memset(st->board, 0, sizeof(st->board));
    for (int w = 0; w < G::kWords; w++) st->board[w] = e.bw[w];
    st->t = e.t; st->sc = e.sc; st->mt = e.mt; st->ended = ended ? 1u : 0u; st->total = e.total;
    st->env = from_pcg(e.ge);
    st->pol = from_pcg(e.gp);
    return played;
}

}  // namespace

extern "C" {

int sc_order_ok(const uint8_t* order) { return sc::order_ok(order) ? 1 : 0; }

uint32_t sc_priority_choice(const uint8_t* order, uint32_t mask_bits) {
    return sc::priority_choice(sc::order_word(order), mask_bits);
}

uint32_t sc_uniform_choice(uint32_t mask_bits, int has_mask, double u, float* p) {
    return sc::uniform_choice(mask_bits, has_mask != 0, u, p);
}

void sc_seed(uint64_t seed, ScStream* out) { *out = from_pcg(pcg_seed(seed)); }

// the 4 x 4 game (g2048_core.h)
int64_t sc_play4(int kind, const uint8_t* order, const EpCfg* cfg, int fresh, uint64_t env_seed, uint64_t pol_seed,
                 ScState* st, int64_t k, uint64_t* boards, uint8_t* actions, double* rewards, uint8_t* flags) {
    return play<sc::Game4>(kind, order, cfg, fresh, env_seed, pol_seed, st, k, boards, actions, rewards, flags);
}

// size N (g2048_sized_core.h), 2 <= N <= 8; -1 for another size
int64_t sc_play_sized(int size, int kind, const uint8_t* order, const EpCfg* cfg, int fresh, uint64_t env_seed,
                      uint64_t pol_seed, ScState* st, int64_t k, uint64_t* boards, uint8_t* actions, double* rewards,
                      uint8_t* flags) {
#define SC_PLAY(NN) \
    return play<sc::GameN<NN>>(kind, order, cfg, fresh, env_seed, pol_seed, st, k, boards, actions, rewards, flags)
    switch (size) {
        case 2: SC_PLAY(2);
        case 3: SC_PLAY(3);
        case 4: SC_PLAY(4);
        case 5: SC_PLAY(5);
        case 6: SC_PLAY(6);
        case 7: SC_PLAY(7);
        case 8: SC_PLAY(8);
        default: return -1;
    }
#undef SC_PLAY
}

}  // extern "C"
