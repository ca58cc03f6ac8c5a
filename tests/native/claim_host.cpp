// TEST-ONLY host build of the step kernel's chunk-ticket map (csrc/g2048_core.h claim_lane_base), for
// tests/test_step_claim_host.py.  Not part of the library.
#include <cstdint>
#include <vector>

#include "g2048_core.h"

using namespace g2048;

// Walks every workgroup's tickets in order -- all the valid ones and the 3 * 16 void ones its waves can draw after
// them -- and returns 0, or a negative code: -1 a base differs from its exact 64-bit value (32-bit overflow), -2 bases
// do not grow with the ticket, -3 a chunk is drawn twice, -4 a chunk below ceil(n / 64) is never drawn, -5 a valid
// ticket follows a void one.
extern "C" int64_t claim_check(uint32_t grid, uint32_t n) {
    const uint64_t chunks = ((uint64_t)n + 63u) / 64u;
    std::vector<uint8_t> seen(chunks, 0);
    for (uint32_t block = 0; block < grid; block++) {
        uint64_t prev = 0;
        uint32_t voids = 0;
        for (uint32_t t = 0; voids < 3u * kClaimWaves; t++) {
            const uint64_t exact =
                ((uint64_t)block * kClaimWaves + (t % kClaimWaves) + (uint64_t)(t / kClaimWaves) * grid * kClaimWaves) * 64u;
            const uint32_t base = claim_lane_base(t, block * 1024u, grid * 1024u);
            if ((uint64_t)base != exact || exact + 63u > UINT32_MAX) return -1;   // base + lane is formed too
            if (t > 0 && exact <= prev) return -2;
            prev = exact;
            if (base >= n) {
                voids++;
                continue;
            }
            if (voids) return -5;
            if (seen[base / 64u]++) return -3;
        }
    }
    for (uint64_t c = 0; c < chunks; c++)
        if (!seen[c]) return -4;
    return 0;
}
