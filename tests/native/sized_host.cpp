// TEST-ONLY host build of csrc/g2048_sized_core.h (the N x N arithmetic the gfx950 kernels run), for
// tests/test_sized_host.py.  Two builds of this file:
//   * a shared library (ctypes): the exported sh_* functions, checked against the reference fixtures;
//   * with -DSIZED_HOST_MAIN a stand-alone program (own main) that runs the fixture-free checks -- the sized
//     functions against a plain array implementation of the game written here, and against g2048_core.h at N = 4 --
//     and is meant to be built with -fsanitize=address,undefined (a shift count of 64 or more in the multi-word
//     nibble code is undefined behaviour that can pass unnoticed on one target).
#include <initializer_list>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "g2048_sized_core.h"

using namespace g2048;
namespace sz = g2048::sized;

#define SIZED_SWITCH(size, CALL) \
    switch (size) {              \
        case 2: CALL(2); break;  \
        case 3: CALL(3); break;  \
        case 4: CALL(4); break;  \
        case 5: CALL(5); break;  \
        case 6: CALL(6); break;  \
        case 7: CALL(7); break;  \
        case 8: CALL(8); break;  \
        default: break;          \
    }

namespace {

template <int N>
sz::Board<N> from_words(const uint64_t* w) {
    sz::Board<N> b;
    for (int i = 0; i < sz::Dim<N>::kWords; i++) b.w[i] = w[i];
    return b;
}
template <int N>
void to_words(const sz::Board<N>& b, uint64_t* w) {
    for (int i = 0; i < sz::Dim<N>::kWords; i++) w[i] = b.w[i];
}

template <int N>
void t_move(const uint64_t* b, uint32_t a, uint64_t* out, uint8_t* list, uint32_t* sum) {
    MoveSummary s;
    const sz::Board<N> m = sz::board_move<N, true>(from_words<N>(b), a, s, list);
    MoveSummary s2;
    const sz::Board<N> m2 = sz::board_move<N, false>(from_words<N>(b), a, s2, nullptr);
    to_words<N>(m, out);
    sum[0] = s.count; sum[1] = s.sum_e; sum[2] = s.score; sum[3] = s.max_e; sum[4] = s.overflow;
    // the list-free instantiation must agree
    sum[5] = sz::board_eq<N>(m, m2) && s.count == s2.count && s.sum_e == s2.sum_e && s.score == s2.score &&
             s.max_e == s2.max_e && s.overflow == s2.overflow;
}

struct EpCfg {
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

// Game2048Env.reset(seed) + steps on the numpy PCG64 stream.  boards [steps + 1][W] (row 0 = the reset board),
// lists [steps][kListLen]; per step reward (fp64), flags, score_add, mask, max tile exponent.  start (W words, or
// NULL): a board that replaces the reset board before the first step (the stream stays where reset left it).
template <int N>
void t_episode(uint64_t seed, const uint64_t* start, const uint8_t* actions, int64_t steps, const EpCfg* cfg, uint64_t* boards,
               uint8_t* lists, double* rewards, uint32_t* flags, uint32_t* score_add, uint32_t* masks,
               uint32_t* max_tile, uint32_t* reset_mask) {
    constexpr int W = sz::Dim<N>::kWords, LEN = sz::Dim<N>::kListLen;
    const RewardCfg rc = reward_cfg(*cfg);
    Pcg64 g;
    sz::Board<N> b = sz::fresh_board<N, 0>(seed, 0, g);
    if (start) b = from_words<N>(start);
    to_words<N>(b, boards);
    *reset_mask = sz::action_mask<N>(b);
    uint32_t mt = 2;
    for (int64_t t = 0; t < steps; t++) {
        const sz::StepValues<N> o =
            sz::env_step<N, 0, true>(b, actions[t], (uint32_t)(t + 1), mt, g, 0, 0, rc, cfg->max_steps, lists + t * LEN);
        b = o.board;
        to_words<N>(b, boards + (t + 1) * W);
        rewards[t] = o.reward;
        flags[t] = o.flags;
        score_add[t] = o.score_add;
        masks[t] = o.mask;
        max_tile[t] = mt;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// a plain array implementation of the game (src/game2048.py restated on exponents), for the fixture-free checks
struct Naive {
    int n;
    int c[8][8];
};

uint64_t rnd(uint64_t& s) {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
}

Naive naive_rot_cw(const Naive& a) {   // np.rot90(k=-1): out[i][j] = in[n-1-j][i]
    Naive r;
    r.n = a.n;
    for (int i = 0; i < a.n; i++)
        for (int j = 0; j < a.n; j++) r.c[i][j] = a.c[a.n - 1 - j][i];
    return r;
}

// rotate clockwise 3 - a times, move every row left, rotate back; merged exponents appended in order
Naive naive_move(Naive b, int a, int* merged, int& nm, bool& ovf) {
    const int rot = 3 - a;
    for (int t = 0; t < rot; t++) b = naive_rot_cw(b);
    nm = 0;
    ovf = false;
    for (int r = 0; r < b.n; r++) {
        int cells[8], k = 0, out[8] = {0, 0, 0, 0, 0, 0, 0, 0}, w = 0;
        for (int j = 0; j < b.n; j++)
            if (b.c[r][j]) cells[k++] = b.c[r][j];
        for (int i = 0; i < k;) {
            if (i + 1 < k && cells[i] == cells[i + 1]) {
                merged[nm++] = cells[i] + 1;
                if (cells[i] == 15) ovf = true;
                out[w++] = cells[i] == 15 ? 15 : cells[i] + 1;
                i += 2;
            } else {
                out[w++] = cells[i];
                i += 1;
            }
        }
        for (int j = 0; j < b.n; j++) b.c[r][j] = out[j];
    }
    for (int t = 0; t < (4 - rot) % 4; t++) b = naive_rot_cw(b);
    return b;
}

bool naive_eq(const Naive& a, const Naive& b) {
    for (int i = 0; i < a.n; i++)
        for (int j = 0; j < a.n; j++)
            if (a.c[i][j] != b.c[i][j]) return false;
    return true;
}

bool naive_done(const Naive& b) {
    for (int i = 0; i < b.n; i++)
        for (int j = 0; j < b.n; j++) {
            if (!b.c[i][j]) return false;
            if (i + 1 < b.n && b.c[i + 1][j] == b.c[i][j]) return false;
            if (j + 1 < b.n && b.c[i][j + 1] == b.c[i][j]) return false;
        }
    return true;
}

template <int N>
sz::Board<N> pack(const Naive& a) {
    sz::Board<N> b;
    for (int w = 0; w < sz::Dim<N>::kWords; w++) b.w[w] = 0;
    for (int k = 0; k < N * N; k++) b.w[k >> 4] |= (uint64_t)a.c[k / N][k % N] << (4 * (k & 15));
    return b;
}

template <int N>
int64_t t_selfcheck(int64_t count, uint64_t seed) {
    constexpr int LEN = sz::Dim<N>::kListLen;
    int64_t bad = 0;
    uint64_t s = seed | 1;
    for (int64_t it = 0; it < count; it++) {
        Naive a;
        a.n = N;
        const uint64_t kind = rnd(s) % 5;   // empties / small exponents (many merges) / full / high tiles
        for (int i = 0; i < N; i++)
            for (int j = 0; j < N; j++) {
                const uint64_t r = rnd(s);
                int e = kind == 1 ? 1 + (int)(r % 2) : kind == 3 ? 13 + (int)(r % 3) : 1 + (int)(r % 15);
                if (kind != 2 && kind != 1 && (r >> 32) % 8 < (kind == 4 ? 6u : 3u)) e = 0;
                a.c[i][j] = e;
            }
        const sz::Board<N> b = pack<N>(a);
        uint32_t mask = 0;
        for (int act = 0; act < 4; act++) {
            int merged[64], nm;
            bool ovf;
            const Naive m = naive_move(a, act, merged, nm, ovf);
            uint8_t list[LEN + 1];
            MoveSummary sm;
            const sz::Board<N> g = sz::board_move<N, true>(b, (uint32_t)act, sm, list);
            bool ok = sz::board_eq<N>(g, pack<N>(m)) && (int)sm.count == nm && (bool)sm.overflow == ovf;
            uint32_t se = 0, sc = 0, mx = 0;
            for (int k = 0; k < nm; k++) {
                ok = ok && list[k] == merged[k];
                se += merged[k];
                sc += 1u << merged[k];
                mx = (uint32_t)merged[k] > mx ? merged[k] : mx;
            }
            for (int k = nm; k < LEN; k++) ok = ok && list[k] == 0;
            ok = ok && sm.sum_e == se && sm.score == sc && sm.max_e == mx;
            if (!naive_eq(m, a)) mask |= 1u << act;
            bad += !ok;
        }
        bad += sz::action_mask<N>(b) != mask;
        bad += sz::is_done<N>(b) != naive_done(a);
        // empty cells in row-major order
        const sz::Bits<N> bits = sz::board_bits<N>(b);
        uint32_t ne = 0;
        for (int k = 0; k < N * N; k++)
            if (!a.c[k / N][k % N]) {
                bad += sz::kth_empty<N>(bits.z, ne) != (uint32_t)k;
                ne++;
            }
        bad += sz::bits_empty<N>(bits) != ne;
        // symmetries: k quarter turns counter-clockwise (three clockwise ones each), after fliplr for k >= 4
        for (int k = 0; k < 8; k++) {
            Naive x = a;
            if (k >= 4)
                for (int i = 0; i < N; i++)
                    for (int j = 0; j < N; j++) x.c[i][j] = a.c[i][N - 1 - j];
            for (int t = 0; t < 3 * (k & 3); t++) x = naive_rot_cw(x);
            bad += !sz::board_eq<N>(sz::symmetry_board<N>(b, k), pack<N>(x));
        }
        // spawns keep every old tile and add one 2 or 4 in an empty cell; the PCG64 and Philox paths on this board
        if (ne) {
            Pcg64 g = pcg_seed(rnd(s));
            sz::Board<N> p = b, q = b;
            sz::spawn_pcg<N>(p, g);
            sz::spawn_philox<N>(q, (uint32_t)rnd(s), (uint32_t)rnd(s));
            for (const sz::Board<N>* y : {&p, &q}) {
                int diff = 0;
                for (int k = 0; k < N * N; k++) {
                    const uint32_t o = sz::get_cell<N>(b, k), v = sz::get_cell<N>(*y, k);
                    if (o != v) {
                        diff++;
                        bad += !(o == 0 && (v == 1 || v == 2));
                    }
                }
                bad += diff != 1;
            }
        }
    }
    return bad;
}

// at N = 4 the sized move / mask / done / PCG64 spawn equal the g2048_core.h functions
int64_t check_n4(int64_t count, uint64_t seed) {
    int64_t bad = 0;
    uint64_t s = seed | 1;
    const auto lut = [](uint32_t o) { return line_move_left(o); };
    for (int64_t it = 0; it < count; it++) {
        uint64_t b = 0;
        const uint64_t kind = rnd(s) % 4;
        for (int k = 0; k < 16; k++) {
            const uint64_t r = rnd(s);
            uint64_t e = kind == 1 ? 1 + r % 3 : 1 + r % 15;
            if (kind != 2 && (r >> 32) % 8 < 3) e = 0;
            b |= e << (4 * k);
        }
        sz::Board<4> sb;
        sb.w[0] = b;
        for (uint32_t a = 0; a < 4; a++) {
            MoveSummary s0, s1;
            const uint64_t m0 = board_move(b, a, lut, s0);
            uint8_t list[8];
            const sz::Board<4> m1 = sz::board_move<4, true>(sb, a, s1, list);
            bool ok = m0 == m1.w[0] && s0.count == s1.count && s0.sum_e == s1.sum_e && s0.score == s1.score &&
                      s0.max_e == s1.max_e && s0.overflow == s1.overflow;
            // the 4 x 4 list holds nibbles e - 1, the sized one bytes e
            for (uint32_t k = 0; k < s0.count; k++) ok = ok && ((s0.list >> (4 * k)) & 15u) == ((list[k] - 1u) & 15u);
            bad += !ok;
        }
        bad += action_mask(b) != sz::action_mask<4>(sb);
        bad += is_done(b) != sz::is_done<4>(sb);
        const uint64_t sd = rnd(s);
        Pcg64 g0 = pcg_seed(sd), g1 = g0;
        if (it & 1) (void)pcg_next32(g0), (void)pcg_next32(g1);   // half of the streams start with a full buffer
        const uint64_t p0 = spawn_pcg(b, g0);
        sz::Board<4> p1 = sb;
        sz::spawn_pcg<4>(p1, g1);
        bad += p0 != p1.w[0] || g0.s_lo != g1.s_lo || g0.s_hi != g1.s_hi || g0.has_uint32 != g1.has_uint32 ||
               g0.uinteger != g1.uinteger;
    }
    return bad;
}

}  // namespace

extern "C" {

int sh_words(int size) { return size < 2 || size > 8 ? -1 : (size * size + 15) / 16; }

// one line: new line, merged bytes (position order), and the summary count / sum_e / score / max_e
uint32_t sh_line_move(int size, uint32_t line, uint32_t* ml, uint32_t* sum) {
    MoveSummary s;
    s.count = s.sum_e = s.score = s.max_e = s.list = s.overflow = 0;
    uint32_t r = 0;
#define CALL(NN) r = sz::line_move<NN>(line, s, *ml)
    SIZED_SWITCH(size, CALL)
#undef CALL
    sum[0] = s.count; sum[1] = s.sum_e; sum[2] = s.score; sum[3] = s.max_e;
    return r;
}

void sh_move(int size, const uint64_t* b, uint32_t a, uint64_t* out, uint8_t* list, uint32_t* sum) {
#define CALL(NN) t_move<NN>(b, a, out, list, sum)
    SIZED_SWITCH(size, CALL)
#undef CALL
}

uint32_t sh_mask(int size, const uint64_t* b) {
    uint32_t r = 0;
#define CALL(NN) r = sz::action_mask<NN>(from_words<NN>(b))
    SIZED_SWITCH(size, CALL)
#undef CALL
    return r;
}

int sh_done(int size, const uint64_t* b) {
    int r = 0;
#define CALL(NN) r = sz::is_done<NN>(from_words<NN>(b))
    SIZED_SWITCH(size, CALL)
#undef CALL
    return r;
}

void sh_symmetry(int size, const uint64_t* b, int k, uint64_t* out) {
#define CALL(NN) to_words<NN>(sz::symmetry_board<NN>(from_words<NN>(b), k), out)
    SIZED_SWITCH(size, CALL)
#undef CALL
}

uint32_t sh_symmetry_action(uint32_t a, int k) { return symmetry_action(a, k); }

void sh_philox(uint64_t key, uint64_t seed, uint32_t ctr, uint32_t tag, uint32_t* out) {
    const U4 r = sz::philox_draw(key, seed, ctr, tag);
    out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}

void sh_spawn_philox(int size, const uint64_t* b, uint32_t rx, uint32_t ry, uint64_t* out) {
#define CALL(NN)                                   \
    {                                              \
        sz::Board<NN> x = from_words<NN>(b);       \
        sz::spawn_philox<NN>(x, rx, ry);           \
        to_words<NN>(x, out);                      \
    }
    SIZED_SWITCH(size, CALL)
#undef CALL
}

// Philox reset board (counter 0, tag 1) and one Philox step of it
void sh_fresh_philox(int size, uint64_t key, uint64_t seed, uint64_t* out) {
    Pcg64 g;
#define CALL(NN) to_words<NN>(sz::fresh_board<NN, 1>(seed, key, g), out)
    SIZED_SWITCH(size, CALL)
#undef CALL
}

void sh_episode(int size, uint64_t seed, const uint8_t* actions, int64_t steps, const EpCfg* cfg, uint64_t* boards,
                uint8_t* lists, double* rewards, uint32_t* flags, uint32_t* score_add, uint32_t* masks,
                uint32_t* max_tile, uint32_t* reset_mask) {
#define CALL(NN)                                                                                              \
    t_episode<NN>(seed, nullptr, actions, steps, cfg, boards, lists, rewards, flags, score_add, masks, max_tile, \
                  reset_mask)
    SIZED_SWITCH(size, CALL)
#undef CALL
}

// sh_episode from an injected board: reset(seed), the board overwritten with `start`, then the steps
void sh_episode_from(int size, uint64_t seed, const uint64_t* start, const uint8_t* actions, int64_t steps,
                     const EpCfg* cfg, uint64_t* boards, uint8_t* lists, double* rewards, uint32_t* flags,
                     uint32_t* score_add, uint32_t* masks, uint32_t* max_tile, uint32_t* reset_mask) {
#define CALL(NN)                                                                                            \
    t_episode<NN>(seed, start, actions, steps, cfg, boards, lists, rewards, flags, score_add, masks, max_tile, \
                  reset_mask)
    SIZED_SWITCH(size, CALL)
#undef CALL
}

int64_t sh_selfcheck(int size, int64_t count, uint64_t seed) {
    int64_t r = -1;
#define CALL(NN) r = t_selfcheck<NN>(count, seed)
    SIZED_SWITCH(size, CALL)
#undef CALL
    return r;
}

int64_t sh_check_n4(int64_t count, uint64_t seed) { return check_n4(count, seed); }

}  // extern "C"

#ifdef SIZED_HOST_MAIN
int main() {
    int64_t bad = check_n4(200000, 7);
    printf("n4 vs g2048_core.h: %lld mismatches\n", (long long)bad);
    for (int size = 2; size <= 8; size++) {
        const int64_t b = sh_selfcheck(size, 20000, 11 + size);
        printf("size %d vs array game: %lld mismatches\n", size, (long long)b);
        bad += b;
        // whole episodes on the PCG64 stream (reset spawns, Lemire draws for every empty count, truncation)
        EpCfg cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.use_action_mask = 1;
        cfg.base_reward_scale = 1.0;
        cfg.empty_tile_reward = 0.1;
        cfg.max_steps = 400;
        static uint8_t actions[400];
        static uint64_t boards[401 * 4];
        static uint8_t lists[400 * 32];
        static double rewards[400];
        static uint32_t flags[400], score_add[400], masks[400], max_tile[400];
        uint32_t reset_mask;
        for (uint64_t seed = 0; seed < 8; seed++) {
            uint64_t s = seed * 77 + 5;
            for (int t = 0; t < 400; t++) actions[t] = (uint8_t)(rnd(s) >> 20 & 3);
            sh_episode(size, seed, actions, 400, &cfg, boards, lists, rewards, flags, score_add, masks, max_tile,
                       &reset_mask);
            // invariants: flags agree with the mask of the previous board
            uint32_t pm = reset_mask;
            for (int t = 0; t < 400; t++) {
                bad += ((flags[t] & kFChanged) != 0) != ((pm >> actions[t] & 1u) != 0);
                bad += ((flags[t] & kFTerminated) != 0) != (masks[t] == 0);
                pm = masks[t];
            }
        }
    }
    printf("total: %lld mismatches\n", (long long)bad);
    return bad ? 1 : 0;
}
#endif
