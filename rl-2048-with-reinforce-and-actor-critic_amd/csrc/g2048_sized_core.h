// g2048_sized_core.h -- the 2048 arithmetic for N x N boards, 2 <= N <= 8, shared by the gfx950 kernels
// (g2048_sized.hip) and the CPU unit-test harness (tests/native/sized_host.cpp, test-only).  The 4 x 4 hot path
// stays in g2048_core.h (uint64 bitboard, row tables); nothing there changes.  Nothing here allocates or launches.
//
// Board: cell k = r*N + c lives in nibble (k & 15) of word (k >> 4) and holds log2(tile) (0 = empty);
// W = ceil(N*N / 16) words (1 for N <= 4, 2 for N = 5, 3 for N = 6, 4 for N = 7, 8); the unused high nibbles of the
// last word are always 0.  A "line" is N nibbles (<= 32 bits) in move-left frame order (nibble 0 = destination
// edge).  A 15+15 merge saturates at 15 and raises kFOverflow, as on the 4 x 4 path.
//
// Every per-thread array is indexed by loop counters of fully unrolled loops only (compile-time constants on the
// device: registers, no scratch).  Every shift count is < the operand width for every N (the multi-word code
// guards each cross-word shift), which the sanitizer build of the host harness checks.
#pragma once
#include "g2048_core.h"

namespace g2048 {
namespace sized {

template <int N>
struct Dim {
    static_assert(N >= 2 && N <= 8, "board sizes 2..8");
    static constexpr int kCells = N * N;
    static constexpr int kWords = (N * N + 15) / 16;
    static constexpr int kListLen = N * (N / 2);   // most merges one move can make
    static constexpr uint32_t kLineMask = N == 8 ? 0xFFFFFFFFu : ((1u << (4 * (N & 7))) - 1u);
};

template <int N>
struct Board {
    uint64_t w[Dim<N>::kWords];
};

// nibble-LSB masks per word: every cell / cells with a right-hand neighbour (c < N-1) / with a lower one (r < N-1)
template <int N>
struct Masks {
    uint64_t cell[4], h[4], v[4];
};

template <int N>
constexpr Masks<N> make_masks() {
    Masks<N> m{};
    for (int k = 0; k < N * N; k++) {
        const uint64_t bit = 1ull << (4 * (k & 15));
        m.cell[k >> 4] |= bit;
        if (k % N < N - 1) m.h[k >> 4] |= bit;
        if (k / N < N - 1) m.v[k >> 4] |= bit;
    }
    return m;
}

template <int N>
G2048_HD bool board_eq(const Board<N>& a, const Board<N>& b) {
    bool e = true;
#pragma unroll
    for (int w = 0; w < Dim<N>::kWords; w++) e = e && a.w[w] == b.w[w];
    return e;
}

// the board as one bit string shifted right by S bits, 0 < S < 64 (4 = the right-hand neighbour, 4N = the lower one)
template <int N, int S>
G2048_HD Board<N> shr(const Board<N>& b) {
    static_assert(S > 0 && S < 64, "cross-word shift counts stay below 64");
    constexpr int W = Dim<N>::kWords;
    Board<N> r;
#pragma unroll
    for (int w = 0; w < W; w++) {
        uint64_t v = b.w[w] >> S;
        if (w + 1 < W) v |= b.w[w + 1 < W ? w + 1 : w] << (64 - S);
        r.w[w] = v;
    }
    return r;
}

template <int N>
G2048_HD uint32_t get_cell(const Board<N>& b, int k) {
    return (uint32_t)(b.w[k >> 4] >> (4 * (k & 15))) & 15u;
}

// row j as a line (cell c in nibble c): N contiguous nibbles of the bit string, at most across two words
template <int N>
G2048_HD uint32_t get_row(const Board<N>& b, int j) {
    constexpr int W = Dim<N>::kWords;
    const int off = 4 * N * j, w = off >> 6, s = off & 63;
    uint64_t v = b.w[w] >> s;
    if (s + 4 * N > 64 && w + 1 < W) v |= b.w[w + 1 < W ? w + 1 : w] << ((64 - s) & 63);   // then s > 32
    return (uint32_t)v & Dim<N>::kLineMask;
}

// column j as a line (cell r in nibble r)
template <int N>
G2048_HD uint32_t get_col(const Board<N>& b, int j) {
    uint32_t x = 0;
#pragma unroll
    for (int p = 0; p < N; p++) x |= get_cell<N>(b, p * N + j) << (4 * p);
    return x;
}

template <int N>
G2048_HD void or_row(Board<N>& b, int j, uint32_t line) {
    constexpr int W = Dim<N>::kWords;
    const int off = 4 * N * j, w = off >> 6, s = off & 63;
    b.w[w] |= (uint64_t)line << s;
    if (s + 4 * N > 64 && w + 1 < W) b.w[w + 1 < W ? w + 1 : w] |= (uint64_t)line >> ((64 - s) & 63);
}

template <int N>
G2048_HD void or_col(Board<N>& b, int j, uint32_t line) {
#pragma unroll
    for (int p = 0; p < N; p++) {
        const int k = p * N + j;
        b.w[k >> 4] |= (uint64_t)((line >> (4 * p)) & 15u) << (4 * (k & 15));
    }
}

// reverse the N nibbles of a line
template <int N>
G2048_HD uint32_t rev_line(uint32_t x) {
    x = ((x & 0x0F0F0F0Fu) << 4) | ((x >> 4) & 0x0F0F0F0Fu);
    x = ((x & 0x00FF00FFu) << 8) | ((x >> 8) & 0x00FF00FFu);
    x = (x << 16) | (x >> 16);
    return x >> (4 * (8 - N));
}

// 1 where the nibble-sized value x (0..15) is nonzero, else 0; no compare (see line_move)
G2048_HD uint32_t nz1(uint32_t x) { return (x + 15u) >> 4; }

// _row_move_left (src/game2048.py:120-137) of one N-nibble line in plain ALU (the pass of line_move_alu): the
// pending tile either merges with the next equal tile or is placed at the write position.  Returns the new line;
// ml = the merged exponents of this line in position order, one byte each (true value: 16 = a saturated 15+15);
// the summary fields count / sum_e / score / max_e are accumulated into s.
// Written without compares or selects: on the device every compare of a lane value yields a 64-bit lane mask in
// scalar registers, and enough of them stay live across the unrolled steps to spill scalar registers; sums and
// masks of 0 / all-ones words stay in vector registers.
template <int N>
G2048_HD uint32_t line_move(uint32_t o, MoveSummary& s, uint32_t& ml) {
    uint32_t out = 0u, sh = 0u, pend = o & 15u, msh = 0u;
    ml = 0u;
#pragma unroll
    for (int k = 1; k < N; k++) {
        const uint32_t v = (o >> (4 * k)) & 15u;
        const uint32_t nzm = 0u - nz1(v);                       // tile here
        const uint32_t mgm = nzm & (nz1(v ^ pend) - 1u);        // ... equal to the pending one: merge
        const uint32_t e = mgm & (v + 1u);                      // merged exponent (16 = saturated), 0 if none
        const uint32_t emit = (e - (e >> 4)) | (~mgm & nzm & pend);
        out |= emit << sh;                                      // sh <= 4 (N - 2) here
        sh += 4u * nz1(emit);
        ml |= e << (msh & 31u);                                 // at most N/2 merges: msh <= 24 whenever e != 0
        msh += mgm & 8u;
        s.count += mgm & 1u;
        s.sum_e += e;
        s.score += (1u << e) & ~1u;
        s.max_e = e > s.max_e ? e : s.max_e;
        pend = (~mgm & ((nzm & v) | (~nzm & pend)));
    }
    return out | (pend << sh);                                  // sh <= 4 (N - 1)
}

// cell (r, c) <-> (c, r)
template <int N>
G2048_HD Board<N> transpose(const Board<N>& b) {
    Board<N> r;
#pragma unroll
    for (int w = 0; w < Dim<N>::kWords; w++) r.w[w] = 0ull;
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++) {
            const int d = j * N + i;
            r.w[d >> 4] |= (uint64_t)get_cell<N>(b, i * N + j) << (4 * (d & 15));
        }
    return r;
}

// reverse the cells of every row: (r, c) -> (r, N-1-c)
template <int N>
G2048_HD Board<N> reverse_rows(const Board<N>& b) {
    Board<N> r;
#pragma unroll
    for (int w = 0; w < Dim<N>::kWords; w++) r.w[w] = 0ull;
#pragma unroll
    for (int j = 0; j < N; j++) or_row<N>(r, j, rev_line<N>(get_row<N>(b, j)));
    return r;
}

// reverse the order of the rows: (r, c) -> (N-1-r, c)
template <int N>
G2048_HD Board<N> flip_rows(const Board<N>& b) {
    Board<N> r;
#pragma unroll
    for (int w = 0; w < Dim<N>::kWords; w++) r.w[w] = 0ull;
#pragma unroll
    for (int j = 0; j < N; j++) or_row<N>(r, N - 1 - j, get_row<N>(b, j));
    return r;
}

// m all-ones: y, m zero: x
template <int N>
G2048_HD Board<N> select(const Board<N>& x, const Board<N>& y, uint64_t m) {
    Board<N> r;
#pragma unroll
    for (int w = 0; w < Dim<N>::kWords; w++) r.w[w] = x.w[w] ^ ((x.w[w] ^ y.w[w]) & m);
    return r;
}

// Game2048._move (src/game2048.py:158-165) for action a.  The reference rotates clockwise (3 - a) times and moves
// every row left, top to bottom.  Here the board is brought into a frame whose rows are those lines in that order --
// left: the board; right: rows reversed, bottom row first; up: columns, last column first; down: columns reversed
// -- with transposes and reversals selected by masks (no rotation), and taken back afterwards.  The lines are
// then moved one per iteration of a loop that is NOT unrolled: each iteration takes the frame's lowest row and
// shifts the frame down by one row (compile-time shifts, so no array is indexed by the loop counter); unrolled, the
// N independent line moves are interleaved by the scheduler and their live values spill vector registers at N >= 5.
// WANT_LIST: list[0 .. kListLen) receives the merged exponents in the reference's order (frame rows top to bottom,
// each left to right) followed by zeros.  The summary does not depend on the order of the merges.
template <int N, bool WANT_LIST>
G2048_HD Board<N> board_move(const Board<N>& b, uint32_t a, MoveSummary& s, uint8_t* list) {
    constexpr int W = Dim<N>::kWords;
    // 0 / all-ones words of the action (0 up, 1 right, 2 down, 3 left): vertical, reversed, lines taken backwards
    const uint64_t mvert = 0ull - (uint64_t)(~a & 1u), mrev = 0ull - (uint64_t)(((a >> 1) ^ a) & 1u),
                   mback = 0ull - (uint64_t)(~(a >> 1) & 1u);
    s.count = s.sum_e = s.score = s.max_e = s.list = s.overflow = 0u;
    Board<N> f = select<N>(b, transpose<N>(b), mvert);
    f = select<N>(f, reverse_rows<N>(f), mrev);
    f = select<N>(f, flip_rows<N>(f), mback);
    Board<N> g;
#pragma unroll
    for (int w = 0; w < W; w++) g.w[w] = 0ull;
    uint32_t cnt = 0;
#pragma unroll 1
    for (int j = 0; j < N; j++) {
        const uint32_t o = (uint32_t)f.w[0] & Dim<N>::kLineMask;
        f = shr<N, 4 * N>(f);
        uint32_t ml;
        const uint32_t nl = line_move<N>(o, s, ml);
        g = shr<N, 4 * N>(g);
        or_row<N>(g, N - 1, nl);   // N - 1 further shifts bring the first line to row 0
        if (WANT_LIST) {
#pragma unroll
            for (int q = 0; q < N / 2; q++) {
                const uint32_t e = (ml >> (8 * q)) & 255u;
                if (e) {
                    list[cnt] = (uint8_t)e;
                    cnt++;
                }
            }
        }
    }
    if (WANT_LIST)
        for (uint32_t k = cnt; k < (uint32_t)Dim<N>::kListLen; k++) list[k] = 0;
    s.overflow = s.max_e >> 4;
    g = select<N>(g, flip_rows<N>(g), mback);
    g = select<N>(g, reverse_rows<N>(g), mrev);
    return select<N>(g, transpose<N>(g), mvert);
}

// nz / empty / equal-neighbour bits of a board (bit 4 (k & 15) of word k >> 4 = cell k)
template <int N>
struct Bits {
    Board<N> nz, z, eqh, eqv;
};

template <int N>
G2048_HD Bits<N> board_bits(const Board<N>& b) {
    constexpr int W = Dim<N>::kWords;
    constexpr Masks<N> M = make_masks<N>();
    Bits<N> r;
    const Board<N> bh = shr<N, 4>(b), bv = shr<N, 4 * N>(b);
#pragma unroll
    for (int w = 0; w < W; w++) {
        r.nz.w[w] = nz_bits(b.w[w]);
        r.z.w[w] = ~r.nz.w[w] & M.cell[w];
        r.eqh.w[w] = ~nz_bits(b.w[w] ^ bh.w[w]) & r.nz.w[w] & M.h[w];
        r.eqv.w[w] = ~nz_bits(b.w[w] ^ bv.w[w]) & r.nz.w[w] & M.v[w];
    }
    return r;
}

// number of empty cells
template <int N>
G2048_HD uint32_t bits_empty(const Bits<N>& r) {
    uint32_t n = 0;
#pragma unroll
    for (int w = 0; w < Dim<N>::kWords; w++) n += (uint32_t)popc64(r.z.w[w]);
    return n;
}

// Game2048._is_done (src/game2048.py:172-187): no empty cell and no equal horizontal / vertical neighbours
template <int N>
G2048_HD bool bits_done(const Bits<N>& r) {
    uint64_t any = 0;
#pragma unroll
    for (int w = 0; w < Dim<N>::kWords; w++) any |= r.z.w[w] | r.eqh.w[w] | r.eqv.w[w];
    return any == 0;
}

// Game2048.get_action_mask (src/game2048.py:95-99, :233-237): bit a set iff action a changes the board -- a line
// changes under move-left iff an empty cell precedes a tile or two adjacent tiles are equal
template <int N>
G2048_HD uint32_t bits_mask(const Bits<N>& r) {
    constexpr int W = Dim<N>::kWords;
    constexpr Masks<N> M = make_masks<N>();
    const Board<N> nzh = shr<N, 4>(r.nz), nzv = shr<N, 4 * N>(r.nz), zh = shr<N, 4>(r.z), zv = shr<N, 4 * N>(r.z);
    uint64_t up = 0, down = 0, left = 0, right = 0;
#pragma unroll
    for (int w = 0; w < W; w++) {
        up |= (r.z.w[w] & nzv.w[w] & M.v[w]) | r.eqv.w[w];
        down |= (r.nz.w[w] & zv.w[w] & M.v[w]) | r.eqv.w[w];
        left |= (r.z.w[w] & nzh.w[w] & M.h[w]) | r.eqh.w[w];
        right |= (r.nz.w[w] & zh.w[w] & M.h[w]) | r.eqh.w[w];
    }
    return (uint32_t)(up != 0) | ((uint32_t)(right != 0) << 1) | ((uint32_t)(down != 0) << 2) |
           ((uint32_t)(left != 0) << 3);
}

template <int N>
G2048_HD bool is_done(const Board<N>& b) { return bits_done<N>(board_bits<N>(b)); }
template <int N>
G2048_HD uint32_t action_mask(const Board<N>& b) { return bits_mask<N>(board_bits<N>(b)); }

// index of the k-th empty cell in row-major order (np.argwhere(board == 0)[k], src/game2048.py:109); z = Bits::z
template <int N>
G2048_HD uint32_t kth_empty(const Board<N>& z, uint32_t k) {
    uint32_t cell = 0;
    bool found = false;
#pragma unroll
    for (int w = 0; w < Dim<N>::kWords; w++) {
        const uint32_t c = (uint32_t)popc64(z.w[w]);
        const bool hit = !found && k < c;
        cell = hit ? 16u * w + kth_empty_cell(z.w[w], k) : cell;
        k = (!found && !hit) ? k - c : k;
        found = found || hit;
    }
    return cell;
}

// put exponent e into (empty) cell `cell`
template <int N>
G2048_HD void put_cell(Board<N>& b, uint32_t cell, uint32_t e) {
    const uint32_t word = cell >> 4, sh = 4u * (cell & 15u);
#pragma unroll
    for (int w = 0; w < Dim<N>::kWords; w++) b.w[w] |= word == (uint32_t)w ? (uint64_t)e << sh : 0ull;
}

// Game2048._spawn (src/game2048.py:108-118) on the numpy PCG64 stream: integers(len(empties)) -- 32-bit Lemire,
// n <= 64, n == 1 draws nothing -- then random() < 0.9
template <int N>
G2048_HD void spawn_pcg(Board<N>& b, Pcg64& g) {
    const Bits<N> r = board_bits<N>(b);
    const uint32_t n = bits_empty<N>(r);
    if (n == 0u) return;
    const uint32_t k = pcg_bounded(g, n);
    const uint32_t cell = kth_empty<N>(r.z, k);
    put_cell<N>(b, cell, pcg_random(g) < 0.9 ? 1u : 2u);
}

// Philox spawn, as spawn_philox_z: rx picks the cell (Lemire, no rejection), ry < 0.9 * 2**32 picks the 2
template <int N>
G2048_HD void spawn_philox(Board<N>& b, uint32_t rx, uint32_t ry) {
    const Bits<N> r = board_bits<N>(b);
    const uint32_t n = bits_empty<N>(r);
    if (n == 0u) return;
    const uint32_t k = (uint32_t)(((uint64_t)rx * n) >> 32);
    put_cell<N>(b, kth_empty<N>(r.z, k), ry < 3865470566u ? 1u : 2u);
}

// the Philox draw of (key, lane seed, counter, tag): the 4 x 4 path's counter / key scheme
G2048_HD U4 philox_draw(uint64_t key, uint64_t seed, uint32_t ctr, uint32_t tag) {
    U4 c{(uint32_t)seed, (uint32_t)(seed >> 32), ctr, tag};
    return philox4x32(c, (uint32_t)key, (uint32_t)(key >> 32));
}

// Game2048.reset (src/game2048.py:26-34): empty board, two spawns from a fresh stream.  RNG 0 = numpy PCG64
// (default_rng(seed), g receives the stream), 1 = Philox (counter 0, tag 1: x, y the first spawn, z, w the second).
template <int N, int RNG>
G2048_HD Board<N> fresh_board(uint64_t seed, uint64_t key, Pcg64& g) {
    Board<N> b;
#pragma unroll
    for (int w = 0; w < Dim<N>::kWords; w++) b.w[w] = 0ull;
    if (RNG == 0) {
        g = pcg_seed(seed);
        spawn_pcg<N>(b, g);
        spawn_pcg<N>(b, g);
    } else {
        const U4 r = philox_draw(key, seed, 0u, 1u);
        spawn_philox<N>(b, r.x, r.y);
        spawn_philox<N>(b, r.z, r.w);
    }
    return b;
}

// Game2048Env._compute_reward (src/env.py:197-261): env_reward_nz's arithmetic and fp64 operation order, with the
// number of empty cells of the final board passed as a number.  Every term is an exact integer times a config
// constant, so the order of the merges does not enter.
G2048_HD double env_reward_ne(const RewardCfg& c, const MoveSummary& s, uint32_t n_empty, bool done, bool invalid,
                              uint32_t& max_tile_e) {
    const uint32_t t = c.terms;
    if ((t & kRwInvalidPenalty) && invalid) return c.invalid_action_penalty;
    double r = (t & kRwLog2) ? (double)s.sum_e : (double)s.score;
    r *= c.base_reward_scale;
    if (t & kRwEmpty) r += c.empty_tile_reward * (double)n_empty;
    if (t & kRwMerge) r += c.merge_reward * (double)s.count;
    if (s.max_e >= 3u && s.max_e > max_tile_e) {
        double bonus = 0.0;
        if (t & kRwBonusRaw) bonus = (double)(1u << s.max_e);
        else if (t & kRwBonusLog2) bonus = (double)s.max_e;
        max_tile_e = s.max_e;
        bonus *= c.bonus_scale;
        r += bonus;
    }
    r += c.step_reward;
    if (done && (t & kRwEndgame)) r += c.endgame_penalty;
    return r;
}

// One Game2048Env.step (src/env.py:264-302) on a lane held in values: move, spawn only if the board changed
// (src/game2048.py:40-70), done and action mask of the final board, fp64 reward, truncation at max_steps (< 0 =
// None).  sc = the step count after this step (also the Philox counter); max_tile_e and g are updated in place.
template <int N>
struct StepValues {
    Board<N> board;
    double reward;
    uint32_t flags, score_add, mask;
};

template <int N, int RNG, bool WANT_LIST>
G2048_HD StepValues<N> env_step(const Board<N>& b, uint32_t a, uint32_t sc, uint32_t& max_tile_e, Pcg64& g,
                                uint64_t key, uint64_t seed, const RewardCfg& rc, int64_t max_steps, uint8_t* list) {
    MoveSummary s;
    Board<N> m = board_move<N, WANT_LIST>(b, a, s, list);
    const bool changed = !board_eq<N>(m, b);
    if (changed) {
        if (RNG == 0) {
            spawn_pcg<N>(m, g);
        } else {
            const U4 r = philox_draw(key, seed, sc, 0u);
            spawn_philox<N>(m, r.x, r.y);
        }
    }
    const Bits<N> bits = board_bits<N>(m);
    const bool done = bits_done<N>(bits);
    const bool invalid = !changed && !done;
    StepValues<N> o;
    o.reward = env_reward_ne(rc, s, bits_empty<N>(bits), done, invalid, max_tile_e);
    const bool trunc = max_steps >= 0 && (int64_t)sc >= max_steps && !done;
    o.flags = (changed ? kFChanged : 0u) | (done ? kFTerminated : 0u) | (trunc ? kFTruncated : 0u) |
              (invalid ? kFInvalid : 0u) | (s.overflow ? kFOverflow : 0u);
    o.board = m;
    o.score_add = s.score;
    o.mask = bits_mask<N>(bits);
    return o;
}

// Dihedral symmetry k of a board (Game2048Env.get_symmetries order, src/env.py:355-396) as a nibble permutation:
// k = 0..3: k counter-clockwise quarter turns (out[i][j] = in[j][N-1-i] per turn); k = 4..7: fliplr, then (k - 4)
// turns.  sym_src = the source cell of output cell (i, j).  The action maps are symmetry_action of g2048_core.h.
constexpr int sym_src(int n, int k, int i, int j) {
    for (int t = 0; t < (k & 3); t++) {
        const int ni = j, nj = n - 1 - i;
        i = ni;
        j = nj;
    }
    if (k >= 4) j = n - 1 - j;
    return i * n + j;
}

template <int N>
G2048_HD Board<N> symmetry_board(const Board<N>& b, int k) {
    Board<N> r;
#pragma unroll
    for (int w = 0; w < Dim<N>::kWords; w++) r.w[w] = 0ull;
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++) {
            const int d = i * N + j;
            r.w[d >> 4] |= (uint64_t)get_cell<N>(b, sym_src(N, k, i, j)) << (4 * (d & 15));
        }
    return r;
}

// all 8 symmetries as a chain -- each the previous one turned once more (k = 1 on it), k = 4 the flip (k = 4 on the
// board) -- so that no two of the nibble permutations are independent work for the scheduler to interleave
template <int N, class Emit>
G2048_HD void symmetry_chain(const Board<N>& b, const Emit& emit) {
    Board<N> x = b;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if (k == 4) x = symmetry_board<N>(b, 4);
        else if (k) x = symmetry_board<N>(x, 1);
        emit(k, x);
    }
}

}  // namespace sized
}  // namespace g2048
