// What lovasz.hip calls of sort.hip beside the public entry points: the passes themselves, on buffers the caller owns.
#pragma once
#include "sg_common.h"
#include "sort_rank.h"

// 0, or SG_EINVAL with the error text set: segments, len >= 1, segments * len <= 2^31 - 1, 1 <= key_bits <= 32
int sort_pairs_shape_ok(const char* who, int64_t segments, int64_t len, int key_bits);

// Pass 0 reads (k_src, v_src); pass i writes the even pair for even i and the odd pair for odd i and reads what pass i - 1
// wrote, so the result lies in the pair sort_final_buffer(sort_passes(key_bits)) names.  The source may be the odd pair (it
// is then overwritten by pass 1).  table: SORT_RADIX * (sort_tiles(len) + 1) words per segment, in any state.
int sort_pairs_run(hipStream_t st, int64_t segments, int64_t len, int key_bits, const uint32_t* k_src, const uint32_t* v_src,
                   uint32_t* k_even, uint32_t* v_even, uint32_t* k_odd, uint32_t* v_odd, uint32_t* table);
