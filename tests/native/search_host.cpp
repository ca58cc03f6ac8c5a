// TEST-ONLY host build of csrc/g2048_search_core.h (the expectimax player and the episode loop body the gfx950 search
// kernels run), for tests/test_search_host.py: a shared library for ctypes.  sr_choose labels boards; sr_play continues
// an episode for at most k steps from a caller-held state, as tests/native/scripted_host.cpp's sc_play does (the same
// EpCfg / ScStream / ScState layouts).
#include <stdint.h>
#include <string.h>

#include "g2048_search_core.h"

using namespace g2048;
namespace sc = g2048::scripted;
namespace sr = g2048::search;

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

sr::Weights weights_of(const uint32_t* w) { return sr::Weights{w[0], w[1], w[2], w[3]}; }

// boards: [kWords, n] planes; actions [n]; q [n, 4]
template <class G>
int choose(int depth, const uint32_t* w, const uint64_t* boards, int64_t n, uint8_t* actions, int64_t* q) {
    const sr::Weights ws = weights_of(w);
    for (int64_t i = 0; i < n; i++) {
        uint64_t b[G::kWords];
        for (int k = 0; k < G::kWords; k++) b[k] = boards[k * n + i];
        int64_t qv[4];
        actions[i] = (uint8_t)sr::choose_at<G>(depth, b, ws, qv);
        for (int k = 0; k < 4; k++) q[4 * i + k] = qv[k];
    }
    return 0;
}

template <class G, int D>
int64_t play_d(const sr::Weights& ws, const EpCfg* cfg, int fresh, uint64_t env_seed, uint64_t pol_seed, ScState* st,
               int64_t k, uint64_t* boards, uint8_t* actions, double* rewards, uint8_t* flags) {
    const RewardCfg rc = reward_cfg(*cfg);
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
        ended = sr::episode_step<G, D>(e, ws, rc, cfg->max_steps, row);
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

template <class G>
int64_t play(int depth, const uint32_t* w, const EpCfg* cfg, int fresh, uint64_t env_seed, uint64_t pol_seed,
             ScState* st, int64_t k, uint64_t* boards, uint8_t* actions, double* rewards, uint8_t* flags) {
    const sr::Weights ws = weights_of(w);
    switch (depth) {
        case 0: return play_d<G, 0>(ws, cfg, fresh, env_seed, pol_seed, st, k, boards, actions, rewards, flags);
        case 1: return play_d<G, 1>(ws, cfg, fresh, env_seed, pol_seed, st, k, boards, actions, rewards, flags);
        case 2: return play_d<G, 2>(ws, cfg, fresh, env_seed, pol_seed, st, k, boards, actions, rewards, flags);
        default: return -1;
    }
}

}  // namespace

#define SR_SIZES(CALL)   \
    switch (size) {      \
        case 2: CALL(2); \
        case 3: CALL(3); \
        case 4: CALL(4); \
        case 5: CALL(5); \
        case 6: CALL(6); \
        case 7: CALL(7); \
        case 8: CALL(8); \
        default: return -1; \
    }

extern "C" {

// the 4 x 4 game (g2048_core.h); -1 for a depth outside 0..2
int sr_choose4(int depth, const uint32_t* w, const uint64_t* boards, int64_t n, uint8_t* actions, int64_t* q) {
    if (depth < 0 || depth > sr::kMaxDepth) return -1;
    return choose<sc::Game4>(depth, w, boards, n, actions, q);
}

// size N (g2048_sized_core.h), 2 <= N <= 8; -1 for another size or depth
int sr_choose_sized(int size, int depth, const uint32_t* w, const uint64_t* boards, int64_t n, uint8_t* actions,
                    int64_t* q) {
    if (depth < 0 || depth > sr::kMaxDepth) return -1;
#define SR_CHOOSE(NN) return choose<sc::GameN<NN>>(depth, w, boards, n, actions, q)
    SR_SIZES(SR_CHOOSE)
#undef SR_CHOOSE
}

int64_t sr_play4(int depth, const uint32_t* w, const EpCfg* cfg, int fresh, uint64_t env_seed, uint64_t pol_seed,
                 ScState* st, int64_t k, uint64_t* boards, uint8_t* actions, double* rewards, uint8_t* flags) {
    return play<sc::Game4>(depth, w, cfg, fresh, env_seed, pol_seed, st, k, boards, actions, rewards, flags);
}

int64_t sr_play_sized(int size, int depth, const uint32_t* w, const EpCfg* cfg, int fresh, uint64_t env_seed,
                      uint64_t pol_seed, ScState* st, int64_t k, uint64_t* boards, uint8_t* actions, double* rewards,
                      uint8_t* flags) {
#define SR_PLAY(NN) \
    return play<sc::GameN<NN>>(depth, w, cfg, fresh, env_seed, pol_seed, st, k, boards, actions, rewards, flags)
    SR_SIZES(SR_PLAY)
#undef SR_PLAY
}

}  // extern "C"
