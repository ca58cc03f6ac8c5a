// TEST-ONLY host build of csrc/g2048_ntuple_core.h (the n-tuple value network: V, the players of depth 0 and 1, the
// episode loop body and the per-row TD(0) arithmetic the gfx950 kernels run), for tests/test_ntuple_host.py: a shared
// library for ctypes.  nt_values / nt_choose label boards; nt_play continues an episode for at most k steps from a
// caller-held state, as tests/native/search_host.cpp's sr_play does (the same EpCfg / ScStream / ScState layouts);
// nt_td is the update in the kernels' two passes.  A feature is ntuple::Feature: uint32 offset, uint32 k, uint64 cells
// (cell j in byte j).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "g2048_ntuple_core.h"

using namespace g2048;
namespace sc = g2048::scripted;
namespace nt = g2048::ntuple;

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

// boards: [kWords, n] planes
template <class G>
int values(const nt::Net& net, const uint64_t* boards, int64_t n, int64_t* out) {
    for (int64_t i = 0; i < n; i++) {
        uint64_t b[G::kWords];
        for (int k = 0; k < G::kWords; k++) b[k] = boards[k * n + i];
        out[i] = nt::value<G>(b, net);
    }
    return 0;
}

template <class G>
int choose(int depth, const nt::Net& net, const uint64_t* boards, int64_t n, uint8_t* actions, int64_t* q) {
    for (int64_t i = 0; i < n; i++) {
        uint64_t b[G::kWords];
        for (int k = 0; k < G::kWords; k++) b[k] = boards[k * n + i];
        int64_t qv[4];
        actions[i] = (uint8_t)nt::choose_at<G>(depth, b, net, qv);
        for (int k = 0; k < 4; k++) q[4 * i + k] = qv[k];
    }
    return 0;
}

template <class G, int D>
int64_t play_d(const nt::Net& net, const EpCfg* cfg, int fresh, uint64_t env_seed, uint64_t pol_seed, ScState* st,
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
        ended = nt::episode_step<G, D>(e, net, rc, cfg->max_steps, row);
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
int64_t play(int depth, const nt::Net& net, const EpCfg* cfg, int fresh, uint64_t env_seed, uint64_t pol_seed,
             ScState* st, int64_t k, uint64_t* boards, uint8_t* actions, double* rewards, uint8_t* flags) {
    return depth == 0 ? play_d<G, 0>(net, cfg, fresh, env_seed, pol_seed, st, k, boards, actions, rewards, flags)
                      : play_d<G, 1>(net, cfg, fresh, env_seed, pol_seed, st, k, boards, actions, rewards, flags);
}

struct WrapAdd {
    void operator()(int32_t* p, int32_t v) const { *p = (int32_t)((uint32_t)*p + (uint32_t)v); }
};

// The update on [kWords, T, n] planes, in the kernels' two passes; w: the weights, updated in place; stats: rows, sum |d|
template <class G>
int td(const nt::Net& net, int32_t* w, const uint64_t* boards, const uint8_t* actions, const uint8_t* flags,
       const int32_t* lengths, int64_t n, int64_t T, int32_t lr_num, int32_t lr_shift, int64_t* stats) {
    const int64_t rows = n * T;
    std::vector<int64_t> v(rows, 0), q(rows, 0);
    std::vector<uint64_t> ms(rows * G::kWords, 0);
    std::vector<int64_t> len(n, 0);      // lengths clamped to 0..T, as pass 2 of the kernels clamps them
    for (int64_t i = 0; i < n; i++) len[i] = lengths[i] < 0 ? 0 : lengths[i] > T ? T : lengths[i];
    for (int64_t r = 0; r < rows; r++) {
        const int64_t t = r / n, i = r % n;
        if (t >= len[i]) continue;
        uint64_t b[G::kWords], m[G::kWords];
        for (int k = 0; k < G::kWords; k++) b[k] = boards[k * rows + r];
        nt::td_row_values<G>(b, actions[r], net, m, v[r], q[r]);
        for (int k = 0; k < G::kWords; k++) ms[r * G::kWords + k] = m[k];
    }
    stats[0] = stats[1] = 0;
    for (int64_t r = 0; r < rows; r++) {
        const int64_t t = r / n, i = r % n;
        if (t >= len[i]) continue;
        int64_t y;
        if (!nt::td_target((uint32_t)t, (uint32_t)len[i], flags[r], t + 1 < len[i] ? q[r + n] : 0, y)) continue;
        const int64_t d = y - v[r];
        stats[0] += 1;
        stats[1] += d < 0 ? -d : d;
        uint64_t m[G::kWords];
        for (int k = 0; k < G::kWords; k++) m[k] = ms[r * G::kWords + k];
        nt::td_apply<G>(m, net, w, nt::td_step(d, lr_num, lr_shift), WrapAdd{});
    }
    return 0;
}

}  // namespace

#define NT_GAMES(CALL)                      \
    if (native4) {                          \
        if (size != 4) return -1;           \
        return CALL(sc::Game4);             \
    }                                       \
    switch (size) {                         \
        case 2: return CALL(sc::GameN<2>);  \
        case 3: return CALL(sc::GameN<3>);  \
        case 4: return CALL(sc::GameN<4>);  \
        case 5: return CALL(sc::GameN<5>);  \
        case 6: return CALL(sc::GameN<6>);  \
        case 7: return CALL(sc::GameN<7>);  \
        case 8: return CALL(sc::GameN<8>);  \
        default: return -1;                 \
    }

extern "C" {

// native4: the 4 x 4 game of g2048_core.h (size must be 4); else the sized game at `size`.  -1 for a bad size / depth.
int nt_values(int size, int native4, const nt::Feature* f, uint32_t nf, const int32_t* w, const uint64_t* boards,
              int64_t n, int64_t* out) {
    const nt::Net net{w, f, nf};
#define NT_CALL(G) values<G>(net, boards, n, out)
    NT_GAMES(NT_CALL)
#undef NT_CALL
}

int nt_choose(int size, int native4, int depth, const nt::Feature* f, uint32_t nf, const int32_t* w,
              const uint64_t* boards, int64_t n, uint8_t* actions, int64_t* q) {
    if (depth < 0 || depth > nt::kMaxDepth) return -1;
    const nt::Net net{w, f, nf};
#define NT_CALL(G) choose<G>(depth, net, boards, n, actions, q)
    NT_GAMES(NT_CALL)
#undef NT_CALL
}

int64_t nt_play(int size, int native4, int depth, const nt::Feature* f, uint32_t nf, const int32_t* w, const EpCfg* cfg,
                int fresh, uint64_t env_seed, uint64_t pol_seed, ScState* st, int64_t k, uint64_t* boards,
                uint8_t* actions, double* rewards, uint8_t* flags) {
    if (depth < 0 || depth > nt::kMaxDepth) return -1;
    const nt::Net net{w, f, nf};
#define NT_CALL(G) play<G>(depth, net, cfg, fresh, env_seed, pol_seed, st, k, boards, actions, rewards, flags)
    NT_GAMES(NT_CALL)
#undef NT_CALL
}

int nt_td(int size, int native4, const nt::Feature* f, uint32_t nf, int32_t* w, const uint64_t* boards,
          const uint8_t* actions, const uint8_t* flags, const int32_t* lengths, int64_t n, int64_t T, int32_t lr_num,
          int32_t lr_shift, int64_t* stats) {
    const nt::Net net{w, f, nf};
#define NT_CALL(G) td<G>(net, w, boards, actions, flags, lengths, n, T, lr_num, lr_shift, stats)
    NT_GAMES(NT_CALL)
#undef NT_CALL
}

int32_t nt_td_step(int64_t delta, int32_t lr_num, int32_t lr_shift) { return nt::td_step(delta, lr_num, lr_shift); }

int64_t nt_floor_div(int64_t a, int64_t d) { return nt::floor_div(a, d); }

}  // extern "C"
