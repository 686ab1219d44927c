// Host-only check of gemm_plan.hpp (tests/test_gemm_plan_host.py builds it with -fsanitize=address,undefined and runs it): the tile
// list of the similarity GEMMs in both forms and the cut of the list into a main launch and a split-K tail.  The sweep holds what
// the rule promises (every tile once, whole rounds in front of a tail, a power-of-two split); the literals are the plans of the
// shipped workloads at 512 workgroup slots and of the small shapes tests/test_gpu_gemm_plans.py pins, recorded from the rule as it
// stood inside build_plan before it moved into the header.  Exit status 0 = every check held.
#include <cstdint>
#include <cstdio>

#include "../gemm_plan.hpp"

using namespace pvs;

static int g_fail = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      if (g_fail++ < 20) {                       \
        fprintf(stderr, "FAIL %s: ", #cond);     \
        fprintf(stderr, __VA_ARGS__);            \
        fprintf(stderr, "\n");                   \
      }                                          \
    }                                            \
  } while (0)

static void properties(int tiles_m, int tiles_n, bool symm, int slots) {
  std::vector<GemmTile> t;
  gemm_plan_tiles(tiles_m, tiles_n, symm, t);
  const int tn_count = symm ? tiles_m : tiles_n;
  const size_t want = symm ? (size_t)tiles_m * (tiles_m + 1) / 2 : (size_t)tiles_m * tiles_n;
  CHECK(t.size() == want, "%d x %d symm %d: %zu tiles listed, %zu exist", tiles_m, tiles_n, (int)symm, t.size(), want);
  std::vector<int> hit((size_t)tiles_m * tn_count, 0);
  for (const GemmTile& x : t) {
    const bool inside = x.tm >= 0 && x.tm < tiles_m && x.tn >= 0 && x.tn < tn_count && (!symm || x.tn >= x.tm);
    CHECK(inside, "%d x %d symm %d: tile (%d, %d) does not exist", tiles_m, tiles_n, (int)symm, x.tm, x.tn);
    if (inside) ++hit[(size_t)x.tm * tn_count + x.tn];
  }
  for (int tm = 0; tm < tiles_m; ++tm)
    for (int tn = 0; tn < tn_count; ++tn) {
      const int expect = (!symm || tn >= tm) ? 1 : 0;
      CHECK(hit[(size_t)tm * tn_count + tn] == expect, "%d x %d symm %d: tile (%d, %d) listed %d times", tiles_m, tiles_n, (int)symm, tm,
            tn, hit[(size_t)tm * tn_count + tn]);
    }
  const int total = (int)t.size();
  const GemmCut c = gemm_plan_cut(total, slots);
  CHECK(c.n_main >= 0 && c.n_tail >= 0 && c.n_main + c.n_tail == total, "total %d slots %d: n_main %d n_tail %d", total, slots, c.n_main,
        c.n_tail);
  if (c.n_tail > 0 && c.n_main > 0)
    CHECK(c.n_main % slots == 0 && c.n_tail < slots, "total %d slots %d: %d whole tiles in front of a tail of %d", total, slots, c.n_main,
          c.n_tail);
  CHECK(c.splitk >= 1 && c.splitk <= 32 && (c.splitk & (c.splitk - 1)) == 0, "total %d slots %d: split %d", total, slots, c.splitk);
  CHECK((c.n_tail == 0) == (c.splitk == 1), "total %d slots %d: split %d with a tail of %d", total, slots, c.splitk, c.n_tail);
  if (total >= 4 * slots) CHECK(c.n_main > 0, "total %d slots %d: four rounds and more keep a main launch", total, slots);
}

static uint64_t order_hash(const std::vector<GemmTile>& t) {   // FNV-1a over (tm, tn) in list order
  uint64_t h = 1469598103934665603ull;
  for (const GemmTile& x : t) {
    h = (h ^ (uint32_t)x.tm) * 1099511628211ull;
    h = (h ^ (uint32_t)x.tn) * 1099511628211ull;
  }
  return h;
}

static void expect_cut(const char* what, int tiles_m, int tiles_n, bool symm, int slots, int n_main, int n_tail, int splitk) {
  std::vector<GemmTile> t;
  gemm_plan_tiles(tiles_m, tiles_n, symm, t);
  const GemmCut c = gemm_plan_cut((int)t.size(), slots);
  CHECK(c.n_main == n_main && c.n_tail == n_tail && c.splitk == splitk, "%s at %d slots: %d + %d split %d", what, slots, c.n_main, c.n_tail,
        c.splitk);
}

int main() {
  const int slot_values[] = {1, 2, 4, 7, 64, 256, 512};
  for (int tm = 1; tm <= 40; ++tm)
    for (int tn = 1; tn <= 40; ++tn)
      for (int s : slot_values) {
        properties(tm, tn, false, s);
        if (tn == tm) properties(tm, tm, true, s);
      }

  // ---- the shipped workloads at 512 slots (256 CUs x 2 workgroups)
  std::vector<GemmTile> t;
  gemm_plan_tiles(64, 64, true, t);   // 8192 x 8192 self-similarity: 2080 tiles of the upper triangle
  CHECK(t.size() == 2080 && order_hash(t) == 2067039801184119939ull, "64 x 64 symmetric: %zu tiles, order hash %llu", t.size(),
        (unsigned long long)order_hash(t));
  if (t.size() == 2080) {
    const int at[8] = {0, 1, 8, 35, 36, 63, 64, 2079};
    const GemmTile lit[8] = {{0, 0}, {0, 1}, {2, 3}, {7, 7}, {0, 8}, {3, 11}, {4, 11}, {63, 63}};
    for (int i = 0; i < 8; ++i)
      CHECK(t[(size_t)at[i]].tm == lit[i].tm && t[(size_t)at[i]].tn == lit[i].tn, "64 x 64 symmetric: entry %d is (%d, %d)", at[i],
            t[(size_t)at[i]].tm, t[(size_t)at[i]].tn);
  }
  expect_cut("64 x 64 symmetric", 64, 64, true, 512, 2048, 32, 16);
  gemm_plan_tiles(16, 64, false, t);   // 2048 queries against 8192 rows
  CHECK(t.size() == 1024 && order_hash(t) == 6714423518916470147ull, "16 x 64 general: %zu tiles, order hash %llu", t.size(),
        (unsigned long long)order_hash(t));
  if (t.size() == 1024) {
    const int at[8] = {0, 1, 8, 35, 36, 63, 64, 1023};
    const GemmTile lit[8] = {{0, 0}, {1, 0}, {0, 1}, {3, 4}, {4, 4}, {7, 7}, {0, 8}, {15, 63}};
    for (int i = 0; i < 8; ++i)
      CHECK(t[(size_t)at[i]].tm == lit[i].tm && t[(size_t)at[i]].tn == lit[i].tn, "16 x 64 general: entry %d is (%d, %d)", at[i],
            t[(size_t)at[i]].tm, t[(size_t)at[i]].tn);
  }
  expect_cut("16 x 64 general", 16, 64, false, 512, 1024, 0, 1);

  // ---- the small plans the GPU tests pin by slot count
  expect_cut("3 x 3", 3, 3, false, 1, 9, 0, 1);
  expect_cut("3 x 3", 3, 3, false, 2, 8, 1, 2);
  expect_cut("3 x 3", 3, 3, false, 4, 8, 1, 4);
  expect_cut("3 x 3", 3, 3, false, 7, 7, 2, 16);
  expect_cut("3 x 3", 3, 3, false, 64, 0, 9, 16);
  expect_cut("3 x 3", 3, 3, false, 512, 0, 9, 32);
  expect_cut("3 x 3 symmetric", 3, 3, true, 1, 6, 0, 1);
  expect_cut("3 x 3 symmetric", 3, 3, true, 4, 4, 2, 2);
  expect_cut("3 x 3 symmetric", 3, 3, true, 64, 0, 6, 8);
  expect_cut("3 x 4", 3, 4, false, 5, 10, 2, 2);
  expect_cut("3 x 4", 3, 4, false, 7, 7, 5, 4);
  expect_cut("3 x 4", 3, 4, false, 64, 0, 12, 16);
  expect_cut("1 x 3", 1, 3, false, 2, 2, 1, 2);
  expect_cut("1 x 3", 1, 3, false, 6, 0, 3, 2);
  expect_cut("1 x 3", 1, 3, false, 64, 0, 3, 16);

  if (g_fail) {
    fprintf(stderr, "gemm_plan_check: %d checks failed\n", g_fail);
    return 1;
  }
  printf("gemm_plan_check: ok\n");
  return 0;
}
