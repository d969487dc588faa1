// The index arithmetic of the stable segmented radix sort (sort.hip), as plain functions of integers so that
// a host program can drive them without a GPU (scripts/sort_emulate.cpp walks the tiles, waves and rounds of every shape
// of tests/test_sort_gpu.py under the address and undefined-behaviour sanitizers and holds the result to std::stable_sort).
//
// One pass orders the pairs of every segment by one digit of SG_SORT_DIGIT_BITS key bits.  A segment of `len` elements is cut
// into tiles of SG_SORT_TILE; a tile belongs to one workgroup of SORT_WAVES waves; wave w of the tile owns the elements
// [w * SORT_WAVE_ELEMS, (w + 1) * SORT_WAVE_ELEMS) and walks them in SORT_ROUNDS rounds of 64, lane l taking element
// r * 64 + l of the wave's share.  So (tile, wave, round, lane) in lexicographic order IS the input order, and an element's
// place in the output is
//   digit_base[d]              elements of the segment whose digit is smaller           (scan of the table's row totals)
// + table[seg][d][tile]        elements of digit d in earlier tiles                      (exclusive scan along the row)
// + wave_base[w][d]            elements of digit d in earlier waves of the tile          (prefix over the waves' counts)
// + seen[w][d]                 elements of digit d in earlier rounds of the wave         (the wave's running count)
// + sort_lane_rank(peers, l)   lanes below l of this round that hold digit d             (ballots, mbcnt)
// None of the five depends on the order in which anything lands.
#pragma once
#include <stdint.h>
#include "../../include/segengine.h"

#if defined(__HIPCC__)
#define SG_HD __host__ __device__ inline
#else
#define SG_HD inline
#endif

constexpr int SORT_RADIX = 1 << SG_SORT_DIGIT_BITS;
constexpr int SORT_WAVES = 4;                                          // 256 threads
constexpr int SORT_WAVE_ELEMS = SG_SORT_TILE / SORT_WAVES;             // 512
constexpr int SORT_ROUNDS = SORT_WAVE_ELEMS / 64;                      // 8
static_assert(SORT_RADIX == 256, "thread d of a 256-thread workgroup owns digit d");
static_assert(SORT_ROUNDS * 64 * SORT_WAVES == SG_SORT_TILE, "a tile is waves x rounds x 64 lanes");

SG_HD int sort_passes(int key_bits) { return (key_bits + SG_SORT_DIGIT_BITS - 1) / SG_SORT_DIGIT_BITS; }

SG_HD int64_t sort_tiles(int64_t len) { return (len + SG_SORT_TILE - 1) / SG_SORT_TILE; }

// the digit of pass `pass`: the last pass of a key_bits that is no multiple of the digit width compares fewer bits
SG_HD uint32_t sort_digit_mask(int pass, int key_bits) {
  const int left = key_bits - pass * SG_SORT_DIGIT_BITS;
  return left >= SG_SORT_DIGIT_BITS ? (uint32_t)(SORT_RADIX - 1) : ((1u << left) - 1u);
}

SG_HD uint32_t sort_digit(uint32_t key, int pass, uint32_t mask) { return (key >> (pass * SG_SORT_DIGIT_BITS)) & mask; }

// element of the segment that (tile, wave, round, lane) holds; >= len: nothing
SG_HD int64_t sort_elem(int64_t tile, int wave, int round, int lane) {
  return tile * SG_SORT_TILE + (int64_t)wave * SORT_WAVE_ELEMS + round * 64 + lane;
}

// table[seg][digit][tile]: digit-major, so that a row's exclusive scan counts the earlier tiles
SG_HD int64_t sort_table_index(int64_t seg, int digit, int64_t tile, int64_t ntiles) {
  return (seg * SORT_RADIX + digit) * ntiles + tile;
}

// lanes below `lane` among the round's lanes with the same digit
SG_HD int sort_lane_rank(uint64_t peers, int lane) {
  return __builtin_popcountll(peers & ((1ull << lane) - 1ull));
}

// the highest lane of the peers adds the round's count to the wave's running count: one writer per digit and round
SG_HD bool sort_is_last_peer(uint64_t peers, int lane) { return (peers >> lane) == 1ull; }

// pass i writes buffer (i even ? 0 : 1) of the two it alternates between and reads the other (pass 0: the caller's input).
// The public call wants the last pass in the caller's output: which of the two is that?
SG_HD int sort_final_buffer(int passes) { return (passes - 1) & 1; }

// place of an element in the whole output array from base = digit_base + tile_base, wave_base and place = seen + lane rank;
// -1 if the terms left the segment (they cannot: the caller then drops the store instead of writing outside the tensor)
SG_HD int64_t sort_out_index(int64_t seg, int64_t len, uint32_t base, uint32_t wave_base, uint32_t place) {
  const int64_t pos = (int64_t)base + wave_base + place;
  return pos < len ? seg * len + pos : -1;
}

// the table, the row totals and, for more than one pass, one spare pair of buffers
SG_HD size_t sort_ws_words(int64_t segments, int64_t len, int key_bits) {
  const size_t tab = (size_t)segments * SORT_RADIX * ((size_t)sort_tiles(len) + 1);
  return tab + (sort_passes(key_bits) > 1 ? 2 * (size_t)segments * (size_t)len : 0);
}
