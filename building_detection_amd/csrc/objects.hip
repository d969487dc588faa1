// Per-building evaluation on label maps: deterministic connected-component labelling of a u8 mask or class map
// (sg_objects_label) and the intersection counts of two label maps (sg_objects_overlap).  What the host does with them -
// IoU matching, precision / recall per building - is exact integer work in building_detection_amd/objects.py.
//
//   sg_objects_label    1. parent array: every non-zero pixel its own root;
//                       2. union-find merge of neighbours of EQUAL value (4- or 8-connected), larger root under smaller: the
//                          root of a component ends as its smallest pixel index, whatever the order of the unions;
//                       3. flatten (every pixel points at its root) and count the roots of each 256-pixel block;
//                       4. exclusive scan of the block counts in two levels (SCAN_ITEMS counts per workgroup, then one
//                          workgroup over the at most TOP_ITEMS segment totals): the object number of a root is its rank
//                          among all roots in raster order - no ticket, so the numbering is the same in every run;
//                       5. number the roots, start their table rows; 6. labels + per-object area / bounding box, one
//                          set of integer atomics per run of equal labels inside a wave.
//   sg_objects_overlap  an open-addressing table (64-bit keys a << 32 | b, 32-bit counts) in caller memory; a run of
//                       equal keys inside a wave inserts once, adding its length; at most `slots` probes, then the run is
//                       counted as lost; a second kernel compacts the occupied slots into the pair list.
//
// HBM / atomic-bound integer work, no float anywhere.  No loop waits for another workgroup: a find follows strictly decreasing
// parents, a union retries only after somebody else's union succeeded, a probe sequence ends after `slots` steps.
#include "sg_common.h"

namespace {

constexpr int OBJ_COLS = 8;        // table row: first pixel, area, x0, y0, x1, y1, value, 0
constexpr int NT = 256;            // threads per workgroup = pixels per workgroup
constexpr int SCAN_THREAD = 16;    // block counts per thread of the first scan level
constexpr int SCAN_ITEMS = NT * SCAN_THREAD;  // 4096 block counts (= 2^20 pixels) per workgroup of the first scan level
constexpr int TOP_THREAD = 8;
constexpr int TOP_ITEMS = NT * TOP_THREAD;    // 2048 segment totals in the one workgroup of the second level: 2^31 pixels
static_assert((int64_t)NT * SCAN_ITEMS * TOP_ITEMS >= (1ll << 31), "the two scan levels must cover every image the ABI admits");

constexpr unsigned long long EMPTY_KEY = ~0ull;  // a, b >= 0: no real key has the top bit set

// ------------------------------------------------------------------------------------------------ union-find (as morph.hip)
__device__ __forceinline__ int uf_find(const int* L, int x) {
  while (true) {
    const int p = __atomic_load_n(&L[x], __ATOMIC_RELAXED);  // other workgroups hang roots under smaller ones meanwhile
    if (p == x) return x;
    x = p;
  }
}

__device__ __forceinline__ void uf_union(int* L, int a, int b) {
  while (true) {
    a = uf_find(L, a);
    b = uf_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }  // a > b: hang a under b
    const int old = atomicMin(&L[a], b);
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(NT) void obj_init_kernel(const unsigned char* __restrict__ m, int* __restrict__ L, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i < n) L[i] = m[i] ? (int)i : -1;
}

// the left, upper and (conn8) the two upper diagonal neighbours, where they hold the pixel's own value
__global__ __launch_bounds__(NT) void obj_merge_kernel(const unsigned char* __restrict__ m, int* __restrict__ L, int H, int W,
                                                       int conn8) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  const int64_t n = (int64_t)H * W;
  if (i >= n) return;
  const unsigned char v = m[i];
  if (!v) return;
  const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
  if (x > 0 && m[i - 1] == v) uf_union(L, (int)i, (int)i - 1);
  if (y > 0) {
    if (m[i - W] == v) uf_union(L, (int)i, (int)(i - W));
    if (conn8) {
      if (x > 0 && m[i - W - 1] == v) uf_union(L, (int)i, (int)(i - W - 1));
      if (x < W - 1 && m[i - W + 1] == v) uf_union(L, (int)i, (int)(i - W + 1));
    }
  }
}

// L[i] <- root of i (roots stay self-parented: concurrent finds of other pixels still end there); cnt[block] = its roots
__global__ __launch_bounds__(NT) void obj_flatten_count_kernel(int* __restrict__ L, int64_t n, int* __restrict__ cnt) {
  __shared__ int wsum[NT / 64];
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  bool root = false;
  if (i < n && L[i] >= 0) {
    const int r = uf_find(L, (int)i);
    if (r != (int)i) L[i] = r;
    root = r == (int)i;
  }
  const unsigned long long bal = __ballot(root);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// exclusive prefix of v over the workgroup's threads; *total = the workgroup's sum
__device__ __forceinline__ int block_excl_scan(int v, int* sm, int* total) {
  const int t = threadIdx.x;
  sm[t] = v;
  __syncthreads();
  for (int off = 1; off < NT; off <<= 1) {
    const int x = t >= off ? sm[t - off] : 0;
    __syncthreads();
    sm[t] += x;
    __syncthreads();
  }
  const int incl = sm[t];
  *total = sm[NT - 1];
  __syncthreads();
  return incl - v;
}

// a[0 .. na) in segments of NT * PER items, one workgroup each: exclusive scan in place inside the segment, the segment's
// sum to seg[block] (seg == nullptr: one segment only, the sum goes to *total_out)
template <int PER>
__global__ __launch_bounds__(NT) void obj_scan_kernel(int* __restrict__ a, int na, int* __restrict__ seg, int* __restrict__ total_out) {
  __shared__ int sm[NT];
  const int base = blockIdx.x * (NT * PER) + threadIdx.x * PER;
  int v[PER];
  int s = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    v[j] = base + j < na ? a[base + j] : 0;
    s += v[j];
  }
  int total;
  int run = block_excl_scan(s, sm, &total);
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (base + j < na) a[base + j] = run;
    run += v[j];
  }
  if (threadIdx.x == 0) {
    if (seg) seg[blockIdx.x] = total;
    else *total_out = total;
  }
}

// every root takes its rank among all roots (cnt / seg hold the exclusive scans) and keeps it as -(number + 2)
__global__ __launch_bounds__(NT) void obj_number_kernel(const unsigned char* __restrict__ m, int* __restrict__ L, int64_t n,
                                                        const int* __restrict__ cnt, const int* __restrict__ seg,
                                                        int* __restrict__ table, int max_objs) {
  __shared__ int wsum[NT / 64];
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  const bool root = i < n && L[i] == (int)i;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(root);
  if (lane == 0) wsum[wave] = __popcll(bal);
  __syncthreads();
  if (!root) return;
  int k = cnt[blockIdx.x] + seg[blockIdx.x / SCAN_ITEMS] + __popcll(bal & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) k += wsum[w];
  if (k < max_objs) {
    int* row = table + (int64_t)k * OBJ_COLS;
    row[0] = (int)i; row[1] = 0; row[2] = 0x7fffffff; row[3] = 0x7fffffff; row[4] = -1; row[5] = -1; row[6] = m[i]; row[7] = 0;
  }
  L[i] = -(k + 2);
}

__device__ __forceinline__ int obj_of(const int* __restrict__ L, int64_t i) {
  const int p = L[i];
  if (p == -1) return -1;       // background
  if (p < -1) return -(p + 2);  // a root
  return -(L[p] + 2);           // its root carries the number
}

// Lanes of a wave hold consecutive pixels; `head` marks the lanes whose key differs from the previous lane's (lane 0 always).
// Returns the length of the run that starts at a head lane (up to the next head or the end of the wave).
__device__ __forceinline__ int run_length(bool head, int lane) {
  const unsigned long long bal = __ballot(head);
  const unsigned long long after = lane == 63 ? 0ull : bal & ~((2ull << lane) - 1ull);
  return (after ? __builtin_ctzll(after) : 64) - lane;
}

// labels[i] = object number or -1; area and bounding box of every object by one set of atomics per run of equal labels
__global__ __launch_bounds__(NT) void obj_stats_kernel(const int* __restrict__ L, int H, int W, int* __restrict__ table,
                                                       int max_objs, int* __restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  const int64_t n = (int64_t)H * W;
  const int lane = threadIdx.x & 63;
  const int o = i < n ? obj_of(L, i) : -1;
  if (i < n) labels[i] = o;
  const int prev = __shfl_up(o, 1);
  const bool head = lane == 0 || o != prev;
  const int len = run_length(head, lane);
  if (!head || o < 0 || o >= max_objs) return;
  const int64_t j = i + len - 1;  // last pixel of the run; a run that wraps a row end touches both image edges
  const int y0 = (int)(i / W), xa = (int)(i - (int64_t)y0 * W);
  const int y1 = (int)(j / W), xb = (int)(j - (int64_t)y1 * W);
  int* row = table + (int64_t)o * OBJ_COLS;
  atomicAdd(&row[1], len);
  atomicMin(&row[2], y0 == y1 ? xa : 0);
  atomicMin(&row[3], y0);
  atomicMax(&row[4], y0 == y1 ? xb : W - 1);
  atomicMax(&row[5], y1);
}

// ------------------------------------------------------------------------------------------------ overlaps
__global__ __launch_bounds__(NT) void ovl_init_kernel(unsigned long long* __restrict__ keys, int* __restrict__ counts, int64_t slots,
                                                      int* __restrict__ stat) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i < slots) { keys[i] = EMPTY_KEY; counts[i] = 0; }
  if (i == 0) { stat[0] = 0; stat[1] = 0; }
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long k) {  // the 64-bit finaliser of MurmurHash3
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return k;
}

__global__ __launch_bounds__(NT) void ovl_count_kernel(const int* __restrict__ la, const int* __restrict__ lb, int64_t n,
                                                       unsigned long long* __restrict__ keys, int* __restrict__ counts,
                                                       int64_t slots, int* __restrict__ stat) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int a = -1, b = -1;
  if (i < n) { a = la[i]; b = lb[i]; }
  if (a < 0 || b < 0) { a = -1; b = -1; }  // one key for "nothing to count"
  const int pa = __shfl_up(a, 1), pb = __shfl_up(b, 1);
  const bool head = lane == 0 || a != pa || b != pb;
  const int len = run_length(head, lane);
  if (!head || a < 0) return;
  const unsigned long long key = ((unsigned long long)(unsigned)a << 32) | (unsigned)b;
  const unsigned long long mask = (unsigned long long)slots - 1ull;
  unsigned long long h = mix64(key) & mask;
  for (int64_t probe = 0; probe < slots; ++probe) {
    unsigned long long cur = __atomic_load_n(&keys[h], __ATOMIC_RELAXED);
    if (cur == EMPTY_KEY) cur = atomicCAS(&keys[h], EMPTY_KEY, key);  // returns what the slot held
    if (cur == EMPTY_KEY || cur == key) {
      atomicAdd(&counts[h], len);
      return;
    }
    h = (h + 1ull) & mask;
  }
  atomicAdd(&stat[1], len);  // table full of other pairs: the caller repeats with more slots
}

// at most `slots` slots are occupied, so the ticket stays inside the list's `slots` rows
__global__ __launch_bounds__(NT) void ovl_compact_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ counts,
                                                         int64_t slots, int* __restrict__ pairs, int* __restrict__ stat) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= slots) return;
  const unsigned long long key = keys[i];
  if (key == EMPTY_KEY) return;
  const int k = atomicAdd(&stat[0], 1);
  int* row = pairs + (int64_t)k * 3;
  row[0] = (int)(key >> 32); row[1] = (int)(key & 0xffffffffull); row[2] = counts[i];
}

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + NT - 1) / NT); }
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

size_t sg_objects_label_ws_bytes(int H, int W) {
  const int64_t n = (int64_t)H * W;
  if (H <= 0 || W <= 0) return 0;
  const int64_t nb = (n + NT - 1) / NT;
  // parent array, root count per 256-pixel block, total per segment of the first scan level
  return align256((size_t)n * sizeof(int)) + align256((size_t)nb * sizeof(int)) + align256((size_t)TOP_ITEMS * sizeof(int));
}

int sg_objects_label(sg_ctx* ctx, void* stream, int H, int W, const void* map_u8, int conn8, void* ws, size_t ws_bytes,
                     void* labels_i32, void* table_i32, int max_objs, void* count_i32) {
  SG_CHECK_ARG(ctx && map_u8 && ws && labels_i32 && table_i32 && count_i32 && H > 0 && W > 0 && max_objs > 0,
               "sg_objects_label: bad argument");
  SG_CHECK_ARG(conn8 == 0 || conn8 == 1, "sg_objects_label: conn8 %d (0 = 4-connected, 1 = 8-connected)", conn8);
  const int64_t n = (int64_t)H * W;
  SG_CHECK_ARG(n < (1ll << 31) - 2, "sg_objects_label: image exceeds 2^31 pixels");
  if (ws_bytes < sg_objects_label_ws_bytes(H, W)) {
    sg_set_error("sg_objects_label: workspace %zu < %zu", ws_bytes, sg_objects_label_ws_bytes(H, W));
    return SG_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t nb = (n + NT - 1) / NT;
  const int nseg = (int)((nb + SCAN_ITEMS - 1) / SCAN_ITEMS);  // <= TOP_ITEMS by the static_assert above
  int* L = (int*)ws;
  int* cnt = (int*)((char*)ws + align256((size_t)n * sizeof(int)));
  int* seg = (int*)((char*)cnt + align256((size_t)nb * sizeof(int)));
  const unsigned char* m = (const unsigned char*)map_u8;
  hipLaunchKernelGGL(obj_init_kernel, dim3((unsigned)nb), dim3(NT), 0, st, m, L, n);
  hipLaunchKernelGGL(obj_merge_kernel, dim3((unsigned)nb), dim3(NT), 0, st, m, L, H, W, conn8);
  hipLaunchKernelGGL(obj_flatten_count_kernel, dim3((unsigned)nb), dim3(NT), 0, st, L, n, cnt);
  hipLaunchKernelGGL(obj_scan_kernel<SCAN_THREAD>, dim3((unsigned)nseg), dim3(NT), 0, st, cnt, (int)nb, seg, (int*)nullptr);
  hipLaunchKernelGGL(obj_scan_kernel<TOP_THREAD>, dim3(1), dim3(NT), 0, st, seg, nseg, (int*)nullptr, (int*)count_i32);
  hipLaunchKernelGGL(obj_number_kernel, dim3((unsigned)nb), dim3(NT), 0, st, m, L, n, (const int*)cnt, (const int*)seg,
                     (int*)table_i32, max_objs);
  hipLaunchKernelGGL(obj_stats_kernel, dim3((unsigned)nb), dim3(NT), 0, st, (const int*)L, H, W, (int*)table_i32, max_objs,
                     (int*)labels_i32);
  SG_LAUNCH_CHECK("sg_objects_label");
  return 0;
}

size_t sg_objects_overlap_ws_bytes(int64_t slots) {
  if (slots <= 0) return 0;
  return align256((size_t)slots * sizeof(unsigned long long)) + align256((size_t)slots * sizeof(int));  // keys, counts
}

int sg_objects_overlap(sg_ctx* ctx, void* stream, int H, int W, const void* labels_a_i32, const void* labels_b_i32, int64_t slots,
                       void* ws, size_t ws_bytes, void* pairs_i32, void* stat_i32) {
  SG_CHECK_ARG(ctx && labels_a_i32 && labels_b_i32 && ws && pairs_i32 && stat_i32 && H > 0 && W > 0,
               "sg_objects_overlap: bad argument");
  SG_CHECK_ARG(slots > 0 && slots <= (1ll << 30) && (slots & (slots - 1)) == 0,
               "sg_objects_overlap: slots %lld is not a power of two in 1 ... 2^30", (long long)slots);
  const int64_t n = (int64_t)H * W;
  SG_CHECK_ARG(n < (1ll << 31) - 2, "sg_objects_overlap: image exceeds 2^31 pixels");
  if (ws_bytes < sg_objects_overlap_ws_bytes(slots)) {
    sg_set_error("sg_objects_overlap: workspace %zu < %zu", ws_bytes, sg_objects_overlap_ws_bytes(slots));
    return SG_EWORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)ws;
  int* counts = (int*)((char*)ws + align256((size_t)slots * sizeof(unsigned long long)));
  hipLaunchKernelGGL(ovl_init_kernel, dim3(blocks_for(slots)), dim3(NT), 0, st, keys, counts, slots, (int*)stat_i32);
  hipLaunchKernelGGL(ovl_count_kernel, dim3(blocks_for(n)), dim3(NT), 0, st, (const int*)labels_a_i32, (const int*)labels_b_i32, n,
                     keys, counts, slots, (int*)stat_i32);
  hipLaunchKernelGGL(ovl_compact_kernel, dim3(blocks_for(slots)), dim3(NT), 0, st, (const unsigned long long*)keys,
                     (const int*)counts, slots, (int*)pairs_i32, (int*)stat_i32);
  SG_LAUNCH_CHECK("sg_objects_overlap");
  return 0;
}

}  // extern "C"
