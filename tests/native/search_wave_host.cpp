// TEST-ONLY host build of csrc/g2048_search_wave_core.h (the expectimax player split over the lanes of a wave, as the
// gfx950 search_wave kernels run it), for tests/test_search_wave_host.py: a shared library for ctypes.  sw_choose labels
// boards through wave_partial for lanes 0..63, a sum and wave_finish; sw_items lists the work items each lane visits.
#include <stdint.h>

#include "g2048_search_wave_core.h"

using namespace g2048;
namespace sc = g2048::scripted;
namespace sr = g2048::search;

namespace {

// boards: [kWords, n] planes; actions [n]; q [n, 4]
template <class G, int D>
int choose_d(const sr::Weights& ws, const uint64_t* boards, int64_t n, uint8_t* actions, int64_t* q) {
    for (int64_t i = 0; i < n; i++) {
        uint64_t b[G::kWords];
        for (int k = 0; k < G::kWords; k++) b[k] = boards[k * n + i];
        int64_t sum[4] = {0, 0, 0, 0}, qv[4];
        for (uint32_t lane = 0; lane < sr::kWaveLanes; lane++) {
            int64_t tot[4];
            sr::wave_partial<G, D>(b, ws, lane, tot);
            for (int k = 0; k < 4; k++) sum[k] += tot[k];
        }
        actions[i] = (uint8_t)sr::wave_finish<G>(b, ws, sum, qv);
        for (int k = 0; k < 4; k++) q[4 * i + k] = qv[k];
    }
    return 0;
}

template <class G>
int choose(int depth, const uint32_t* w, const uint64_t* boards, int64_t n, uint8_t* actions, int64_t* q) {
    const sr::Weights ws{w[0], w[1], w[2], w[3]};
    if (depth == 1) return choose_d<G, 1>(ws, boards, n, actions, q);
    if (depth == 2) return choose_d<G, 2>(ws, boards, n, actions, q);
    return -1;      // depth 0 has no wave form
}

// board: kWords words.  items: [64, cap, 3] (action, cell, exponent) in the order the lane visits them; counts: [64].
// Returns the total number of items, or -2 when a lane has more than cap.
template <class G>
int items(const uint64_t* board, int cap, int32_t* out, int32_t* counts) {
    uint64_t b[G::kWords];
    for (int k = 0; k < G::kWords; k++) b[k] = board[k];
    int total = 0;
    bool over = false;
    for (uint32_t lane = 0; lane < sr::kWaveLanes; lane++) {
        int k = 0;
        sr::for_lane_items<G>(b, lane, [&](uint32_t a, uint32_t cell, uint32_t e, const uint64_t (&)[G::kWords]) {
            if (k < cap) {
                int32_t* o = out + ((int64_t)lane * cap + k) * 3;
                o[0] = (int32_t)a;
                o[1] = (int32_t)cell;
                o[2] = (int32_t)e;
            } else {
                over = true;
            }
            k++;
        });
        counts[lane] = k;
        total += k;
    }
    return over ? -2 : total;
}

}  // namespace

#define SW_SIZES(CALL)   \
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

// the 4 x 4 game (g2048_core.h); -1 for a depth outside 1..2
int sw_choose4(int depth, const uint32_t* w, const uint64_t* boards, int64_t n, uint8_t* actions, int64_t* q) {
    return choose<sc::Game4>(depth, w, boards, n, actions, q);
}

// size N (g2048_sized_core.h), 2 <= N <= 8; -1 for another size or depth
int sw_choose_sized(int size, int depth, const uint32_t* w, const uint64_t* boards, int64_t n, uint8_t* actions,
                    int64_t* q) {
#define SW_CHOOSE(NN) return choose<sc::GameN<NN>>(depth, w, boards, n, actions, q)
    SW_SIZES(SW_CHOOSE)
#undef SW_CHOOSE
}

int sw_items4(const uint64_t* board, int cap, int32_t* out, int32_t* counts) {
    return items<sc::Game4>(board, cap, out, counts);
}

int sw_items_sized(int size, const uint64_t* board, int cap, int32_t* out, int32_t* counts) {
#define SW_ITEMS(NN) return items<sc::GameN<NN>>(board, cap, out, counts)
    SW_SIZES(SW_ITEMS)
#undef SW_ITEMS
}

}  // extern "C"
