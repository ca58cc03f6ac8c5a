// g2048_search_core.h -- the expectimax player (include/g2048_search.h, rl2048_amd.ExpectimaxPolicy): the afterstate
// heuristic H, the chance node C_d, the move values Q_d and the choice, written once against the game interface of
// g2048_scripted_core.h (Game4 / GameN<N>), and the sibling of episode_step that plays it.  Shared by the gfx950
// kernels (g2048_search_kernel.h) and the CPU test harness (tests/native/search_host.cpp, test-only).  Nothing here
// allocates or launches.
//
// The player, all in integers (so the host build, the kernels and the Python statement of it agree bit for bit):
//   gain(b, a) = sum of log2(v) over the tiles v that move(b, a) creates by merging      (MoveSummary::sum_e)
//   H(b)       = w_empty #empty(b) + w_smooth sum over adjacent cell pairs (15 - |e_i - e_j|)
//                + w_corner sum_{r,c} e[r][c] ((N-1-r) + (N-1-c))
//   C_0(m)     = H(m)
//   C_d(m)     = floor(sum over empty cells c of m [9 V_{d-1}(m + 2 at c) + V_{d-1}(m + 4 at c)] / (10 #empty(m)))
//   Q_d(b, a)  = w_merge gain(b, a) + C_d(move(b, a))   for valid a (move(b, a) != b)
//   V_d(b)     = max over valid a of Q_d(b, a), 0 when no action is valid
//   choice     = the valid action of the largest Q_depth(b, a), the lowest index among equals
// Every value is >= 0 and, with weights <= 4096, below 2^37: int64 throughout, and C's truncating division is the
// floor.
//
// The depth is a template parameter (compile-time recursion: no stack, no per-thread array of levels).  The loops over
// the four actions and over the empty cells are kept rolled, so a depth-d player holds d + 1 inlined moves and one H,
// not 4^d of them; no per-thread array is indexed by a run-time value (the Q values leave through selects).
#pragma once
#include "g2048_scripted_core.h"

namespace g2048 {
namespace search {

constexpr int kMaxDepth = 2;              // include/g2048_search.h: depth in 0..2
constexpr uint32_t kMaxWeight = 4096u;    // ... and every weight in 0..4096

struct Weights {
    uint32_t merge, empty, smooth, corner;
};

// sum over the 16 nibbles of |x_n - y_n|
G2048_HD uint32_t sad_nibbles(uint64_t x, uint64_t y) {
    constexpr uint64_t kLo = 0x0F0F0F0F0F0F0F0Full;
    const uint64_t xl = x & kLo, xh = (x >> 4) & kLo, yl = y & kLo, yh = (y >> 4) & kLo;
#ifdef __HIP_DEVICE_COMPILE__
    uint32_t acc = __builtin_amdgcn_sad_u8((uint32_t)xl, (uint32_t)yl, 0u);
    acc = __builtin_amdgcn_sad_u8((uint32_t)(xl >> 32), (uint32_t)(yl >> 32), acc);
    acc = __builtin_amdgcn_sad_u8((uint32_t)xh, (uint32_t)yh, acc);
    return __builtin_amdgcn_sad_u8((uint32_t)(xh >> 32), (uint32_t)(yh >> 32), acc);
#else
    uint32_t acc = 0;
    for (int i = 0; i < 8; i++) {
        const int a = (int)((xl >> (8 * i)) & 255u) - (int)((yl >> (8 * i)) & 255u);
        const int b = (int)((xh >> (8 * i)) & 255u) - (int)((yh >> (8 * i)) & 255u);
        acc += (uint32_t)(a < 0 ? -a : a) + (uint32_t)(b < 0 ? -b : b);
    }
    return acc;
#endif
}

// H(b).  Smoothness: 15 per adjacent pair (2 N (N - 1) of them) minus the sum of |e_i - e_j|, taken nibble-parallel
// against the board shifted by one cell / one row on the cells that have that neighbour (Masks::h / Masks::v).
template <class G>
G2048_HD int64_t heuristic(const uint64_t (&bw)[G::kWords], const Weights& w) {
    constexpr int N = G::kSize, W = G::kWords;
    static_assert(W == sized::Dim<N>::kWords, "Game4 and GameN<4> share the nibble layout");
    constexpr sized::Masks<N> M = sized::make_masks<N>();
    sized::Board<N> b;
#pragma unroll
    for (int i = 0; i < W; i++) b.w[i] = bw[i];
    const sized::Board<N> bh = sized::shr<N, 4>(b), bv = sized::shr<N, 4 * N>(b);
    uint32_t empty = 0, rough = 0, corner = 0;
#pragma unroll
    for (int i = 0; i < W; i++) {
        const uint64_t hm = M.h[i] * 15ull, vm = M.v[i] * 15ull;
        empty += (uint32_t)popc64(~nz_bits(b.w[i]) & M.cell[i]);
        rough += sad_nibbles(b.w[i] & hm, bh.w[i] & hm) + sad_nibbles(b.w[i] & vm, bv.w[i] & vm);
    }
#pragma unroll
    for (int k = 0; k < N * N; k++) corner += sized::get_cell<N>(b, k) * (uint32_t)((N - 1 - k / N) + (N - 1 - k % N));
    const uint32_t smooth = 15u * (uint32_t)(2 * N * (N - 1)) - rough;
    return (int64_t)w.empty * empty + (int64_t)w.smooth * smooth + (int64_t)w.corner * corner;
}

// the lowest empty cell of z (bit 4 (k & 15) of word k >> 4 = cell k is empty; z != 0), removed from z
template <int W>
G2048_HD uint32_t take_empty(uint64_t (&z)[W]) {
    uint32_t cell = 0;
    bool found = false;
#pragma unroll
    for (int i = 0; i < W; i++) {
        const bool hit = !found && z[i] != 0ull;
        cell = hit ? 16u * (uint32_t)i + ((uint32_t)__builtin_ctzll(z[i] | (1ull << 63)) >> 2) : cell;
        z[i] = hit ? z[i] & (z[i] - 1ull) : z[i];
        found = found || hit;
    }
    return cell;
}

template <class G, int D>
G2048_HD int64_t value(const uint64_t (&b)[G::kWords], const Weights& w);

// C_D(m)
template <class G, int D>
G2048_HD int64_t chance(const uint64_t (&m)[G::kWords], const Weights& w) {
    if constexpr (D == 0) {
        return heuristic<G>(m, w);
    } else {
        constexpr int W = G::kWords;
        constexpr sized::Masks<G::kSize> M = sized::make_masks<G::kSize>();
        uint64_t z[W];
        uint32_t ne = 0;
#pragma unroll
        for (int i = 0; i < W; i++) {
            z[i] = ~nz_bits(m[i]) & M.cell[i];
            ne += (uint32_t)popc64(z[i]);
        }
        int64_t tot = 0;
#pragma unroll 1
        for (uint32_t i = 0; i < ne; i++) {
            const uint32_t cell = take_empty<W>(z);
#pragma unroll 1
            for (uint32_t e = 1; e <= 2; e++) {      // a 2 with weight 9, a 4 with weight 1
                uint64_t c[W];
#pragma unroll
                for (int k = 0; k < W; k++) c[k] = m[k];
                G::put(c, cell, e);
                tot += (int64_t)(e == 1u ? 9 : 1) * value<G, D - 1>(c, w);
            }
        }
        return ne ? (int64_t)((uint64_t)tot / (10u * ne)) : 0;   // a valid move always leaves an empty cell
    }
}

// V_D(b)
template <class G, int D>
G2048_HD int64_t value(const uint64_t (&b)[G::kWords], const Weights& w) {
    int64_t best = 0;      // every Q is >= 0, so the maximum from 0 is also the "no valid action" value
#pragma unroll 1
    for (uint32_t a = 0; a < 4; a++) {
        uint64_t m[G::kWords];
        uint32_t gain;
        if (G::move(b, a, m, gain)) {
            const int64_t q = (int64_t)w.merge * gain + chance<G, D>(m, w);
            best = q > best ? q : best;
        }
    }
    return best;
}

// The choice on board b at depth D: q[a] = Q_D(b, a), -1 for an invalid a; returns the valid action of the largest q
// (the lowest index among equals), 0 when no action is valid.
template <class G, int D>
G2048_HD uint32_t choose(const uint64_t (&b)[G::kWords], const Weights& w, int64_t (&q)[4]) {
    uint32_t act = 0;
    int64_t best = -1;
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = -1;
#pragma unroll 1
    for (uint32_t a = 0; a < 4; a++) {
        uint64_t m[G::kWords];
        uint32_t gain;
        if (G::move(b, a, m, gain)) {
            const int64_t v = (int64_t)w.merge * gain + chance<G, D>(m, w);
#pragma unroll
            for (int k = 0; k < 4; k++) q[k] = a == (uint32_t)k ? v : q[k];
            act = v > best ? a : act;
            best = v > best ? v : best;
        }
    }
    return act;
}

// choose for a depth known at run time (0..kMaxDepth; the caller has checked it)
template <class G>
G2048_HD uint32_t choose_at(int depth, const uint64_t (&b)[G::kWords], const Weights& w, int64_t (&q)[4]) {
    return depth == 0 ? choose<G, 0>(b, w, q) : depth == 1 ? choose<G, 1>(b, w, q) : choose<G, 2>(b, w, q);
}

// episode_step (g2048_scripted_core.h) for the search player: the choice is computed from the board alone -- no action
// mask is read, so it plays with use_action_mask on or off, and it is always a valid action -- and the policy stream
// is not touched (select_action takes a valid candidate as it is).
template <class G, int D>
G2048_HD bool episode_step(scripted::Episode<G>& e, const Weights& w, const RewardCfg& rc, int64_t max_steps,
                           scripted::Row<G>& row) {
    int64_t q[4];
    const uint32_t act = choose<G, D>(e.bw, w, q);
#pragma unroll
    for (int k = 0; k < G::kWords; k++) row.bw[k] = e.bw[k];
    G::step(e.bw, act, e.sc, e.mt, e.ge, rc, max_steps, row.reward, row.flags);
    row.action = act;
    e.sc += 1u;
    e.t += 1u;
    e.total += row.reward;
    return (row.flags & (kFTerminated | kFTruncated)) != 0u;
}

}  // namespace search
}  // namespace g2048
