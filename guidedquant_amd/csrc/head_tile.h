// head_tile.h -- what the scoring heads (head_nll.hip, head_kl.hip) agree on: the tile of a block, the neutral elements of the online
// softmax, and the rule that cuts the vocabulary into ranges.  Constants and host code only: no kernel text lives here.
#pragma once
#include <stdint.h>

#include "gq_internal.h"

namespace gqh {
constexpr uint32_t BS = 128, BV = 128, BKK = 64;  // sequence rows and vocabulary rows of a tile, columns of a K step
constexpr uint32_t LD = BKK + 8;                 // halves per LDS row: 16 bytes of padding
constexpr float NEG = -1.0e30f;                  // below every fp16 value and finite: NEG - NEG = 0, never Inf - Inf
constexpr float LOG2E = 1.4426950408889634f;
constexpr int NO_ID = 0x7FFFFFFF;
constexpr uint32_t MAX_SPLITS = 65535u;

// the vocabulary splits of a launch: the caller's, or enough blocks for two per compute unit with at least 8 tiles each
inline uint32_t pick_splits(uint32_t S, uint32_t V, uint32_t splits) {
    if (splits) return splits;
    const uint32_t row_tiles = (S + BS - 1u) / BS, ntiles = (V + BV - 1u) / BV;
    const uint32_t want = (2u * (uint32_t)gq_cu_count() + row_tiles - 1u) / row_tiles;
    const uint32_t cap = ntiles / 8u < MAX_SPLITS ? ntiles / 8u : MAX_SPLITS;
    const uint32_t n = want < cap ? want : cap;
    return n > 1u ? n : 1u;
}
}  // namespace gqh
