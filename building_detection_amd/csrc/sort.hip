// Stable segmented least-significant-digit radix sort of (key, value) pairs of uint32: `segments` contiguous
// segments of `len` elements, ascending by the low key_bits bits, equal keys in input order.  ceil(key_bits / 8) passes of
//   sort_hist_kernel     one workgroup per tile of SG_SORT_TILE elements: the tile's count of every digit -> table[seg][d][tile].
//                        The workgroup counts in LDS (integer adds, exact in any order) and WRITES all 256 words, so the table
//                        needs no clearing at all (neither a kernel nor a memset node: DESIGN 4.10)
//   sort_scan_kernel     one workgroup per (segment, digit): the row's exclusive scan over the tiles in place, its total to
//                        rowtot[seg][d]
//   sort_scatter_kernel  one workgroup per tile: the exclusive scan of the segment's 256 row totals, then every element's place
//                        from the five terms of sort_rank.h.  Inside the tile the place comes from ballots, an mbcnt prefix and
//                        the fixed order wave -> round -> lane; no atomic is issued, so no place depends on an arrival order:
//                        the sort is stable and gives the same bits every run
// The index arithmetic lives in sort_rank.h as host/device functions; scripts/sort_emulate.cpp drives it on the host.
// No allocation, no synchronisation; every launch is a kernel node.  4-byte alignment is enough for every pointer.
#include "sort_impl.h"

namespace {

__device__ __forceinline__ uint64_t ballot64(bool v) { return __ballot(v); }

// the lanes of the round that hold the same digit as this one (invalid lanes: 0)
__device__ __forceinline__ uint64_t digit_peers(uint32_t d, bool valid) {
  uint64_t peers = ballot64(valid);
#pragma unroll
  for (int b = 0; b < SG_SORT_DIGIT_BITS; ++b) {
    const bool bit = (d >> b) & 1u;
    const uint64_t m = ballot64(bit);
    peers &= bit ? m : ~m;
  }
  return valid ? peers : 0ull;
}

__global__ __launch_bounds__(256) void sort_hist_kernel(int64_t len, int64_t ntiles, int pass, uint32_t mask,
                                                        const uint32_t* __restrict__ keys, uint32_t* __restrict__ table) {
  __shared__ uint32_t h[SORT_RADIX];
  const int64_t seg = blockIdx.x / ntiles, tile = blockIdx.x - seg * ntiles;
  h[threadIdx.x] = 0u;
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t* __restrict__ src = keys + seg * len;
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    const int64_t e = sort_elem(tile, wave, r, lane);
    if (e < len) atomicAdd(&h[sort_digit(src[e], pass, mask)], 1u);
  }
  __syncthreads();
  table[sort_table_index(seg, threadIdx.x, tile, ntiles)] = h[threadIdx.x];
}

// grid = segments * 256; thread t owns the tiles [t * per, (t + 1) * per) of the row
__global__ __launch_bounds__(256) void sort_scan_kernel(int64_t ntiles, uint32_t* __restrict__ table, uint32_t* __restrict__ rowtot) {
  __shared__ uint32_t ws[SORT_WAVES];
  uint32_t* __restrict__ row = table + (int64_t)blockIdx.x * ntiles;
  const int64_t per = (ntiles + 255) / 256;
  const int64_t t0 = (int64_t)threadIdx.x * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
  uint32_t s = 0u;
  for (int64_t t = t0; t < t1; ++t) s += row[t];
  // exclusive prefix of the 256 thread sums: inside the wave by shuffles, across the waves in wave order
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t inc = s;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t v = __shfl_up(inc, off, 64);
    if (lane >= off) inc += v;
  }
  if (lane == 63) ws[wave] = inc;
  __syncthreads();
  uint32_t base = 0u;
  for (int w = 0; w < wave; ++w) base += ws[w];
  uint32_t run = base + inc - s;
  for (int64_t t = t0; t < t1; ++t) {
    const uint32_t v = row[t];
    row[t] = run;
    run += v;
  }
  if (threadIdx.x == 255) rowtot[blockIdx.x] = base + inc;
}

__global__ __launch_bounds__(256) void sort_scatter_kernel(int64_t len, int64_t ntiles, int pass, uint32_t mask,
                                                           const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                           const uint32_t* __restrict__ table, const uint32_t* __restrict__ rowtot,
                                                           uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out) {
  __shared__ uint32_t seen[SORT_WAVES][SORT_RADIX];   // a wave's running count of every digit; after the rounds its total
  __shared__ uint32_t dbase[SORT_RADIX];              // digit_base + tile_base
  __shared__ uint32_t wsum[SORT_WAVES];
  const int64_t seg = blockIdx.x / ntiles, tile = blockIdx.x - seg * ntiles;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, d = threadIdx.x;
#pragma unroll
  for (int w = 0; w < SORT_WAVES; ++w) seen[w][d] = 0u;
  {  // thread d: the exclusive scan of the segment's 256 row totals, plus the row's count in earlier tiles
    const uint32_t s = rowtot[seg * SORT_RADIX + d];
    uint32_t inc = s;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t v = __shfl_up(inc, off, 64);
      if (lane >= off) inc += v;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t base = 0u;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    dbase[d] = base + inc - s + table[sort_table_index(seg, d, tile, ntiles)];
  }
  __syncthreads();
  const uint32_t* __restrict__ ksrc = keys + seg * len;
  const uint32_t* __restrict__ vsrc = vals + seg * len;
  uint32_t k[SORT_ROUNDS], v[SORT_ROUNDS], place[SORT_ROUNDS];   // place: seen + lane rank, the two terms a wave knows alone
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    const int64_t e = sort_elem(tile, wave, r, lane);
    const bool valid = e < len;
    k[r] = valid ? ksrc[e] : 0u;
    v[r] = valid ? vsrc[e] : 0u;
    const uint32_t dg = sort_digit(k[r], pass, mask);
    const uint64_t peers = digit_peers(dg, valid);
    uint32_t pl = 0u;
    if (valid) {
      const uint32_t before = seen[wave][dg];
      pl = before + (uint32_t)sort_lane_rank(peers, lane);
      // one lane per digit writes; the LDS keeps a wave's accesses in program order, so the next round reads the new count
      if (sort_is_last_peer(peers, lane)) seen[wave][dg] = before + (uint32_t)__popcll(peers);
    }
    place[r] = pl;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  uint32_t wbase[SORT_WAVES];   // thread d: digit d's count in the waves before w
  {
    uint32_t run = 0u;
#pragma unroll
    for (int w = 0; w < SORT_WAVES; ++w) {
      wbase[w] = run;
      run += seen[w][d];
    }
  }
#pragma unroll
  for (int w = 0; w < SORT_WAVES; ++w) seen[w][d] = wbase[w];   // column d is this thread's alone
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    const int64_t e = sort_elem(tile, wave, r, lane);
    if (e < len) {
      const uint32_t dg = sort_digit(k[r], pass, mask);
      const int64_t o = sort_out_index(seg, len, dbase[dg], seen[wave][dg], place[r]);
      if (o >= 0) {
        keys_out[o] = k[r];
        vals_out[o] = v[r];
      }
    }
  }
}

}  // namespace

int sort_pairs_run(hipStream_t st, int64_t segments, int64_t len, int key_bits, const uint32_t* k_src, const uint32_t* v_src,
                   uint32_t* k_even, uint32_t* v_even, uint32_t* k_odd, uint32_t* v_odd, uint32_t* table) {
  const int64_t ntiles = sort_tiles(len);
  const int passes = sort_passes(key_bits);
  uint32_t* rowtot = table + segments * SORT_RADIX * ntiles;
  const unsigned tiles = (unsigned)(segments * ntiles), rows = (unsigned)(segments * SORT_RADIX);
  const uint32_t *ks = k_src, *vs = v_src;
  for (int pass = 0; pass < passes; ++pass) {
    const uint32_t mask = sort_digit_mask(pass, key_bits);
    uint32_t* kd = (pass & 1) ? k_odd : k_even;
    uint32_t* vd = (pass & 1) ? v_odd : v_even;
    hipLaunchKernelGGL(sort_hist_kernel, dim3(tiles), dim3(256), 0, st, len, ntiles, pass, mask, ks, table);
    SG_LAUNCH_CHECK("sort_hist_kernel");
    hipLaunchKernelGGL(sort_scan_kernel, dim3(rows), dim3(256), 0, st, ntiles, table, rowtot);
    SG_LAUNCH_CHECK("sort_scan_kernel");
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(tiles), dim3(256), 0, st, len, ntiles, pass, mask, ks, vs, (const uint32_t*)table,
                       (const uint32_t*)rowtot, kd, vd);
    SG_LAUNCH_CHECK("sort_scatter_kernel");
    ks = kd, vs = vd;
  }
  return 0;
}

int sort_pairs_shape_ok(const char* who, int64_t segments, int64_t len, int key_bits) {
  SG_CHECK_ARG(segments >= 1 && len >= 1, "%s: segments = %lld, len = %lld must be >= 1", who, (long long)segments, (long long)len);
  SG_CHECK_ARG(len <= INT32_MAX && segments <= INT32_MAX / len, "%s: segments * len = %lld * %lld exceeds 2^31 - 1", who,
               (long long)segments, (long long)len);
  SG_CHECK_ARG(segments * sort_tiles(len) <= INT32_MAX / SORT_RADIX, "%s: %lld segments of %lld tiles: too many table rows", who,
               (long long)segments, (long long)sort_tiles(len));
  SG_CHECK_ARG(key_bits >= 1 && key_bits <= 32, "%s: key_bits = %d outside [1, 32]", who, key_bits);
  return 0;
}

extern "C" {

size_t sg_sort_pairs_ws_bytes(const sg_ctx*, int64_t segments, int64_t len, int key_bits) {
  if (sort_pairs_shape_ok("sg_sort_pairs_ws_bytes", segments, len, key_bits)) return 0;
  return sort_ws_words(segments, len, key_bits) * sizeof(uint32_t);
}

int sg_sort_pairs_u32(sg_ctx* ctx, void* stream, int64_t segments, int64_t len, int key_bits, const void* keys_in,
                      const void* vals_in, void* keys_out, void* vals_out, void* ws, size_t ws_bytes) {
  SG_CHECK_ARG(ctx && keys_in && vals_in && keys_out && vals_out, "sg_sort_pairs_u32: bad argument");
  if (const int rc = sort_pairs_shape_ok("sg_sort_pairs_u32", segments, len, key_bits)) return rc;
  SG_CHECK_ARG(keys_out != keys_in && keys_out != vals_in && vals_out != keys_in && vals_out != vals_in && keys_out != vals_out,
               "sg_sort_pairs_u32: an output aliases another operand");
  const size_t need = sort_ws_words(segments, len, key_bits) * sizeof(uint32_t);
  if (!ws || ws_bytes < need) {
    sg_set_error("sg_sort_pairs_u32: workspace %zu < %zu", ws_bytes, need);
    return SG_EWORKSPACE;
  }
  uint32_t* table = (uint32_t*)ws;
  uint32_t* tk = table + (size_t)segments * SORT_RADIX * ((size_t)sort_tiles(len) + 1);   // the spare pair: more than one pass only
  uint32_t* tv = tk + segments * len;
  uint32_t *ko = (uint32_t*)keys_out, *vo = (uint32_t*)vals_out;
  const bool out_is_odd = sort_final_buffer(sort_passes(key_bits)) == 1;
  return sort_pairs_run((hipStream_t)stream, segments, len, key_bits, (const uint32_t*)keys_in, (const uint32_t*)vals_in,
                        out_is_odd ? tk : ko, out_is_odd ? tv : vo, out_is_odd ? ko : tk, out_is_odd ? vo : tv, table);
}

}  // extern "C"
