// Host emulation of csrc/sort.hip's passes, driven by the very index functions the kernels call (csrc/sort_rank.h): tiles,
// waves, rounds and lanes are walked in loops, a ballot is a loop over the 64 lanes.  Every buffer is a heap block of exactly
// the size the entry point is given (the workspace: sort_ws_words), so an index slip is an AddressSanitizer report here
// instead of an out-of-bounds store on a GPU.  Over the shape list of tests/test_sort_gpu.py the result is held to
// std::stable_sort and every output slot must be written exactly once per pass.  A development aid, not a pytest test:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I. scripts/sort_emulate.cpp -o sort_emulate
//   ./sort_emulate
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>
#include "building_detection_amd/csrc/sort_rank.h"

static int fails = 0;
#define REQUIRE(cond, ...)                \
  do {                                    \
    if (!(cond)) {                        \
      std::printf("FAIL: " __VA_ARGS__);  \
      std::printf("\n");                  \
      if (++fails > 20) std::exit(1);     \
    }                                     \
  } while (0)

static void hist_pass(int64_t segments, int64_t len, int pass, uint32_t mask, const uint32_t* keys, uint32_t* table) {
  const int64_t ntiles = sort_tiles(len);
  for (int64_t blk = 0; blk < segments * ntiles; ++blk) {
    const int64_t seg = blk / ntiles, tile = blk - seg * ntiles;
    uint32_t h[SORT_RADIX] = {0};
    for (int wave = 0; wave < SORT_WAVES; ++wave)
      for (int r = 0; r < SORT_ROUNDS; ++r)
        for (int lane = 0; lane < 64; ++lane) {
          const int64_t e = sort_elem(tile, wave, r, lane);
          if (e < len) ++h[sort_digit(keys[seg * len + e], pass, mask)];
        }
    for (int d = 0; d < SORT_RADIX; ++d) table[sort_table_index(seg, d, tile, ntiles)] = h[d];
  }
}

static void scan_pass(int64_t segments, int64_t ntiles, uint32_t* table, uint32_t* rowtot) {
  for (int64_t row = 0; row < segments * SORT_RADIX; ++row) {   // thread t owns [t * per, (t + 1) * per)
    const int64_t per = (ntiles + 255) / 256;
    uint32_t run = 0;
    for (int t = 0; t < 256; ++t) {
      const int64_t t0 = (int64_t)t * per, t1 = std::min(t0 + per, ntiles);
      for (int64_t i = t0; i < t1; ++i) {
        const uint32_t v = table[row * ntiles + i];
        table[row * ntiles + i] = run;
        run += v;
      }
    }
    rowtot[row] = run;
  }
}

static void scatter_pass(int64_t segments, int64_t len, int pass, uint32_t mask, const uint32_t* keys, const uint32_t* vals,
                         const uint32_t* table, const uint32_t* rowtot, uint32_t* keys_out, uint32_t* vals_out,
                         std::vector<uint8_t>& written) {
  const int64_t ntiles = sort_tiles(len);
  std::fill(written.begin(), written.end(), 0);
  for (int64_t blk = 0; blk < segments * ntiles; ++blk) {
    const int64_t seg = blk / ntiles, tile = blk - seg * ntiles;
    uint32_t dbase[SORT_RADIX], seen[SORT_WAVES][SORT_RADIX] = {{0}};
    uint32_t run = 0;
    for (int d = 0; d < SORT_RADIX; ++d) {
      dbase[d] = run + table[sort_table_index(seg, d, tile, ntiles)];
      run += rowtot[seg * SORT_RADIX + d];
    }
    REQUIRE(run == (uint32_t)len, "the row totals of segment %lld add up to %u, not %lld", (long long)seg, run, (long long)len);
    static uint32_t place[SORT_WAVES][SORT_ROUNDS][64];
    for (int wave = 0; wave < SORT_WAVES; ++wave)
      for (int r = 0; r < SORT_ROUNDS; ++r) {
        uint32_t dg[64];
        bool valid[64];
        for (int lane = 0; lane < 64; ++lane) {
          const int64_t e = sort_elem(tile, wave, r, lane);
          valid[lane] = e < len;
          dg[lane] = sort_digit(valid[lane] ? keys[seg * len + e] : 0u, pass, mask);
        }
        uint32_t before[64];
        uint64_t peers[64];
        for (int lane = 0; lane < 64; ++lane) {   // digit_peers: the ballots
          uint64_t m = 0;
          for (int o = 0; o < 64; ++o)
            if (valid[o] && dg[o] == dg[lane]) m |= 1ull << o;
          peers[lane] = valid[lane] ? m : 0ull;
          before[lane] = seen[wave][dg[lane]];      // every lane reads before any lane writes
        }
        for (int lane = 0; lane < 64; ++lane) {
          if (!valid[lane]) continue;
          place[wave][r][lane] = before[lane] + (uint32_t)sort_lane_rank(peers[lane], lane);
          if (sort_is_last_peer(peers[lane], lane)) seen[wave][dg[lane]] = before[lane] + (uint32_t)__builtin_popcountll(peers[lane]);
        }
      }
    for (int d = 0; d < SORT_RADIX; ++d) {   // the waves' totals -> the count in earlier waves
      uint32_t w0 = 0;
      for (int w = 0; w < SORT_WAVES; ++w) {
        const uint32_t t = seen[w][d];
        seen[w][d] = w0;
        w0 += t;
      }
    }
    for (int wave = 0; wave < SORT_WAVES; ++wave)
      for (int r = 0; r < SORT_ROUNDS; ++r)
        for (int lane = 0; lane < 64; ++lane) {
          const int64_t e = sort_elem(tile, wave, r, lane);
          if (e >= len) continue;
          const uint32_t k = keys[seg * len + e], d = sort_digit(k, pass, mask);
          const int64_t o = sort_out_index(seg, len, dbase[d], seen[wave][d], place[wave][r][lane]);
          REQUIRE(o >= 0, "an element left its segment (len %lld pass %d)", (long long)len, pass);
          if (o < 0) continue;
          REQUIRE(!written[o], "output slot %lld written twice", (long long)o);
          written[o] = 1;
          keys_out[o] = k;
          vals_out[o] = vals[seg * len + e];
        }
  }
  for (size_t i = 0; i < written.size(); ++i) REQUIRE(written[i], "output slot %zu never written", i);
}

// what sg_sort_pairs_u32 does with its operands
static void sort_pairs(int64_t segments, int64_t len, int key_bits, const uint32_t* kin, const uint32_t* vin, uint32_t* kout,
                       uint32_t* vout, uint32_t* ws) {
  const int64_t ntiles = sort_tiles(len), n = segments * len;
  const int passes = sort_passes(key_bits);
  uint32_t* table = ws;
  uint32_t* rowtot = table + segments * SORT_RADIX * ntiles;
  uint32_t* tk = table + (size_t)segments * SORT_RADIX * ((size_t)ntiles + 1);
  uint32_t* tv = tk + n;
  const bool out_is_odd = sort_final_buffer(passes) == 1;
  uint32_t *ke = out_is_odd ? tk : kout, *ve = out_is_odd ? tv : vout, *ko = out_is_odd ? kout : tk, *vo = out_is_odd ? vout : tv;
  std::vector<uint8_t> written((size_t)n);
  const uint32_t *ks = kin, *vs = vin;
  for (int pass = 0; pass < passes; ++pass) {
    const uint32_t mask = sort_digit_mask(pass, key_bits);
    uint32_t *kd = (pass & 1) ? ko : ke, *vd = (pass & 1) ? vo : ve;
    hist_pass(segments, len, pass, mask, ks, table);
    scan_pass(segments, ntiles, table, rowtot);
    scatter_pass(segments, len, pass, mask, ks, vs, table, rowtot, kd, vd, written);
    ks = kd, vs = vd;
  }
  REQUIRE(ks == kout && vs == vout, "the last pass did not write the caller's output (%d passes)", passes);
}

static const char* KEYSETS[] = {"equal", "two_values", "random30", "top_digit", "low_digit", "junk_above", "sorted", "reversed"};

static std::vector<uint32_t> make_keys(int set, int64_t n, int key_bits, std::mt19937& rng) {
  std::vector<uint32_t> k((size_t)n);
  const int top = (sort_passes(key_bits) - 1) * SG_SORT_DIGIT_BITS;
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t r = rng();
    switch (set) {
      case 0: k[i] = 0x2a5a5a5au; break;
      case 1: k[i] = (r & 1) ? 0x00000001u : 0x20000100u; break;
      case 2: k[i] = r & 0x3fffffffu; break;
      case 3: k[i] = ((r & 0xffu) << top) | 0x15u; break;
      case 4: k[i] = 0x12345600u | (r & 0xffu); break;
      case 5: k[i] = r; break;   // junk above key_bits: carried along, not compared
      case 6: k[i] = (uint32_t)i; break;
      default: k[i] = (uint32_t)(n - 1 - i); break;
    }
  }
  return k;
}

int main() {
  const int T = SG_SORT_TILE, W = SG_SORT_DIGIT_BITS;
  const int64_t lens[] = {1, 63, 64, 65, 255, 257, T - 1, T, T + 1, 3 * T + 17};
  const int64_t segs[] = {1, 3};
  const int bits[] = {1, W, W + 1, 30, 32};
  std::mt19937 rng(12345);
  int cases = 0;
  for (int64_t len : lens)
    for (int64_t segments : segs)
      for (int key_bits : bits)
        for (int set = 0; set < 8; ++set) {
          const int64_t n = segments * len;
          const std::vector<uint32_t> keys = make_keys(set, n, key_bits, rng);
          uint32_t* kin = new uint32_t[n];
          uint32_t* vin = new uint32_t[n];
          uint32_t* kout = new uint32_t[n];
          uint32_t* vout = new uint32_t[n];
          const size_t words = sort_ws_words(segments, len, key_bits);
          uint32_t* ws = new uint32_t[words];
          std::memset(ws, 0xff, words * 4);   // the workspace may hold anything
          for (int64_t i = 0; i < n; ++i) kin[i] = keys[i], vin[i] = 0x80000000u ^ (uint32_t)(i * 2654435761u);
          sort_pairs(segments, len, key_bits, kin, vin, kout, vout, ws);
          const uint32_t cmp = key_bits == 32 ? 0xffffffffu : ((1u << key_bits) - 1u);
          for (int64_t s = 0; s < segments; ++s) {
            std::vector<int64_t> order((size_t)len);
            std::iota(order.begin(), order.end(), (int64_t)0);
            std::stable_sort(order.begin(), order.end(),
                             [&](int64_t a, int64_t b) { return (kin[s * len + a] & cmp) < (kin[s * len + b] & cmp); });
            for (int64_t i = 0; i < len; ++i) {
              const int64_t src = s * len + order[i];
              REQUIRE(kout[s * len + i] == kin[src] && vout[s * len + i] == vin[src],
                      "len %lld segments %lld key_bits %d %s: segment %lld slot %lld", (long long)len, (long long)segments, key_bits,
                      KEYSETS[set], (long long)s, (long long)i);
            }
          }
          delete[] kin; delete[] vin; delete[] kout; delete[] vout; delete[] ws;
          ++cases;
        }
  std::printf("%d cases, %d failures\n", cases, fails);
  return fails ? 1 : 0;
}
