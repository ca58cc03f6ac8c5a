// g2048_search_wave_core.h -- the expectimax player of g2048_search_core.h with choose<G, D>, D >= 1, split at its top
// chance level so that the 64 lanes of a wave can share one board's work.  Written once against Game4 / GameN<N>, host
// and device, like the core it splits.  Shared by the gfx950 kernels (g2048_search_wave_kernel.h) and the CPU test
// harness (tests/native/search_wave_host.cpp, test-only).  Nothing here allocates or launches.
//
// Work items of board b: the triples (a, c, e) -- a valid action a, an empty cell c of move(b, a), an exponent e in
// {1, 2} -- numbered by a, then by c ascending, then by e: item off(a) + 2 rank(c) + (e - 1), off(a) = the items of the
// valid actions below a.  At most 8 (N^2 - 1) of them: 120 at N = 4, 504 at N = 8.  Item i belongs to lane i mod 64.
//   wave_partial<G, D>(b, w, lane, tot)  tot[a] = sum over the lane's items (a, c, e) of (e == 1 ? 9 : 1) V_{D-1}(child)
//   -- the caller sums tot[0..3] over the 64 lanes (integers: any order gives the same bits; every term is below
//      10 * 2^37 and there are at most 504, so int64 holds it) --
//   wave_finish<G>(b, w, tot, q)         Q_D(b, a) = w_merge gain + tot[a] / (10 #empty(move(b, a))) and choose's choice
// Every lane slides the four top moves itself (4 moves against the hundreds below them) and keeps the four afterstates;
// as in g2048_search_core.h no per-thread array is indexed by a run-time value: an item's afterstate is taken, and the
// totals are written, through selects.
#pragma once
#include "g2048_search_core.h"

namespace g2048 {
namespace search {

constexpr uint32_t kWaveLanes = 64;

// the empty cells of m as bits (bit 4 (k & 15) of word k >> 4 = cell k is empty) and their count
template <class G>
G2048_HD uint32_t empty_bits(const uint64_t (&m)[G::kWords], uint64_t (&z)[G::kWords]) {
    constexpr sized::Masks<G::kSize> M = sized::make_masks<G::kSize>();
    uint32_t ne = 0;
#pragma unroll
    for (int i = 0; i < G::kWords; i++) {
        z[i] = ~nz_bits(m[i]) & M.cell[i];
        ne += (uint32_t)popc64(z[i]);
    }
    return ne;
}

// the cell of the k-th (from 0) empty cell of z; k < the number of bits set in z
template <int W>
G2048_HD uint32_t kth_empty(const uint64_t (&z)[W], uint32_t k) {
    uint64_t zw = z[0];
    uint32_t word = 0;
    bool found = false;
#pragma unroll
    for (int i = 0; i < W; i++) {          // the word that holds it: k becomes the rank inside that word
        const uint32_t c = (uint32_t)popc64(z[i]);
        const bool hit = !found && k < c;
        zw = hit ? z[i] : zw;
        word = hit ? (uint32_t)i : word;
        k = (found || hit) ? k : k - c;
        found = found || hit;
    }
    uint32_t sh = 0;
#pragma unroll
    for (uint32_t half = 32; half >= 4; half >>= 1) {   // bisect the word: 32, 16, 8, 4 bits
        const uint32_t c = (uint32_t)popc64((zw >> sh) & ((1ull << half) - 1ull));
        const bool up = k >= c;
        k = up ? k - c : k;
        sh = up ? sh + half : sh;
    }
    return 16u * word + (sh >> 2);
}

// The four afterstates of b, each with its count of empty cells (0 for an invalid action: it then has no items).
template <class G>
struct TopMoves {
    uint64_t m[4][G::kWords];
    uint32_t ne[4];
};

template <class G>
G2048_HD void top_moves(const uint64_t (&b)[G::kWords], TopMoves<G>& t) {
    constexpr int W = G::kWords;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        t.ne[k] = 0;
#pragma unroll
        for (int i = 0; i < W; i++) t.m[k][i] = 0ull;
    }
#pragma unroll 1
    for (uint32_t a = 0; a < 4; a++) {
        uint64_t m[W], z[W];
        uint32_t gain;
        const bool ok = G::move(b, a, m, gain);
        const uint32_t ne = ok ? empty_bits<G>(m, z) : 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            t.ne[k] = a == (uint32_t)k ? ne : t.ne[k];
#pragma unroll
            for (int i = 0; i < W; i++) t.m[k][i] = a == (uint32_t)k ? m[i] : t.m[k][i];
        }
    }
}

// f(a, cell, e, child) for the items of `lane`, in ascending item order; child = move(b, a) with exponent e at cell
template <class G, class F>
G2048_HD void for_lane_items(const uint64_t (&b)[G::kWords], uint32_t lane, F&& f) {
    constexpr int W = G::kWords;
    TopMoves<G> t;
    top_moves<G>(b, t);
    const uint32_t off1 = 2u * t.ne[0], off2 = off1 + 2u * t.ne[1], off3 = off2 + 2u * t.ne[2];
    const uint32_t items = off3 + 2u * t.ne[3];
#pragma unroll 1
    for (uint32_t i = lane; i < items; i += kWaveLanes) {
        // an invalid action has no items, so its offset equals the next one's and the count below skips it
        const uint32_t a = (i >= off1 ? 1u : 0u) + (i >= off2 ? 1u : 0u) + (i >= off3 ? 1u : 0u);
        const uint32_t j = i - (a == 0u ? 0u : a == 1u ? off1 : a == 2u ? off2 : off3);
        uint64_t c[W], z[W];
#pragma unroll
        for (int k = 0; k < W; k++) c[k] = a == 0u ? t.m[0][k] : a == 1u ? t.m[1][k] : a == 2u ? t.m[2][k] : t.m[3][k];
        empty_bits<G>(c, z);
        const uint32_t cell = kth_empty<W>(z, j >> 1), e = (j & 1u) + 1u;
        G::put(c, cell, e);
        f(a, cell, e, c);
    }
}

template <class G, int D>
G2048_HD void wave_partial(const uint64_t (&b)[G::kWords], const Weights& w, uint32_t lane, int64_t (&tot)[4]) {
    static_assert(D >= 1, "depth 0 has no chance level to spread");
#pragma unroll
    for (int k = 0; k < 4; k++) tot[k] = 0;
    for_lane_items<G>(b, lane, [&](uint32_t a, uint32_t, uint32_t e, const uint64_t (&c)[G::kWords]) {
        const int64_t v = (int64_t)(e == 1u ? 9 : 1) * value<G, D - 1>(c, w);
#pragma unroll
        for (int k = 0; k < 4; k++) tot[k] += a == (uint32_t)k ? v : 0;
    });
}

// choose's result from the wave-wide totals: q[a] = Q_D(b, a), -1 for an invalid a; returns the valid action of the
// largest q (the lowest index among equals), 0 when no action is valid
template <class G>
G2048_HD uint32_t wave_finish(const uint64_t (&b)[G::kWords], const Weights& w, const int64_t (&tot)[4],
                              int64_t (&q)[4]) {
    uint32_t act = 0;
    int64_t best = -1;
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = -1;
#pragma unroll 1
    for (uint32_t a = 0; a < 4; a++) {
        uint64_t m[G::kWords], z[G::kWords];
        uint32_t gain;
        if (G::move(b, a, m, gain)) {
            const uint32_t ne = empty_bits<G>(m, z);      // a valid move always leaves an empty cell
            const int64_t t = a == 0u ? tot[0] : a == 1u ? tot[1] : a == 2u ? tot[2] : tot[3];
            const int64_t v = (int64_t)w.merge * gain + (int64_t)((uint64_t)t / (10u * ne));
#pragma unroll
            for (int k = 0; k < 4; k++) q[k] = a == (uint32_t)k ? v : q[k];
            act = v > best ? a : act;
            best = v > best ? v : best;
        }
    }
    return act;
}

// The host's form of the whole choice: the lanes one after another (the kernels reduce with a wave butterfly instead).
template <class G, int D>
G2048_HD uint32_t wave_choose_serial(const uint64_t (&b)[G::kWords], const Weights& w, int64_t (&q)[4]) {
    int64_t sum[4] = {0, 0, 0, 0};
    for (uint32_t lane = 0; lane < kWaveLanes; lane++) {
        int64_t tot[4];
        wave_partial<G, D>(b, w, lane, tot);
#pragma unroll
        for (int k = 0; k < 4; k++) sum[k] += tot[k];
    }
    return wave_finish<G>(b, w, sum, q);
}

}  // namespace search
}  // namespace g2048
