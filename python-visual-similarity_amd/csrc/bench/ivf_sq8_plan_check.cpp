// Host-only check of ivf_sq8_plan.hpp and of the two rules of list_common.hpp it builds on (tests/test_ivf_sq8_host.py builds it
// with -fsanitize=address,undefined and runs it): the width of a candidate row, the query block and the slices of the probed int8
// scan.  The expected values are
// literals worked out by hand from the rules as the section states them, not a restatement of the formulas; the sweep then holds what
// the rule promises: the slices tile [0, W) exactly once, S is a multiple of 16, and a slice the host chose has at least 64 slots.
// Exit status 0 = every check held.
#include <cstdio>

#include "../ivf_sq8_plan.hpp"

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

static void expect_slices(const char* what, int num_cu, int64_t QB, int64_t W, int64_t slice_rows, int64_t S, int64_t G) {
  const IsqSlices s = isq_slices(num_cu, QB, W, slice_rows);
  CHECK(s.S == S && s.G == G, "%s: S %lld G %lld", what, (long long)s.S, (long long)s.G);
}

// the slices walked the way the kernel walks them: slice g is [g S, min((g + 1) S, W)), wave w of it takes p0 + w, p0 + w + 16, ...
static void properties(int num_cu, int64_t QB, int64_t W, int64_t slice_rows) {
  const IsqSlices s = isq_slices(num_cu, QB, W, slice_rows);
  CHECK(s.S >= 16 && s.S % 16 == 0 && s.G >= 1, "cu=%d QB=%lld W=%lld slice=%lld: S %lld G %lld", num_cu, (long long)QB, (long long)W,
        (long long)slice_rows, (long long)s.S, (long long)s.G);
  if (s.S < 1 || s.G < 1) return;
  if (slice_rows == 0) CHECK(s.S >= ISQ_MIN_SLICE, "cu=%d QB=%lld W=%lld: chosen slice %lld", num_cu, (long long)QB, (long long)W, (long long)s.S);
  else CHECK(s.S >= slice_rows && s.S < slice_rows + 16, "W=%lld slice=%lld: rounded to %lld", (long long)W, (long long)slice_rows, (long long)s.S);
  int64_t end = 0;
  for (int64_t g = 0; g < s.G; ++g) {
    const int64_t p0 = g * s.S, p1 = std::min(p0 + s.S, W);
    CHECK(p0 == end && p1 > p0, "cu=%d QB=%lld W=%lld slice=%lld: slice %lld is [%lld, %lld)", num_cu, (long long)QB, (long long)W,
          (long long)slice_rows, (long long)g, (long long)p0, (long long)p1);
    end = p1;
    if (s.G > 4096 && g == 2) g = s.G - 3, end = (s.G - 2) * s.S;   // long rows of small slices: both ends
  }
  CHECK(end == W, "cu=%d QB=%lld W=%lld slice=%lld: covered %lld", num_cu, (long long)QB, (long long)W, (long long)slice_rows, (long long)end);
  if (W <= 4096) {   // every slot belongs to exactly one (slice, wave, step)
    std::vector<int> hit((size_t)W, 0);
    for (int64_t g = 0; g < s.G; ++g)
      for (int w = 0; w < ISQ_WAVES; ++w)
        for (int64_t p = g * s.S + w; p < std::min((g + 1) * s.S, W); p += ISQ_WAVES) ++hit[(size_t)p];
    for (int64_t p = 0; p < W; ++p) CHECK(hit[(size_t)p] == 1, "W=%lld slice=%lld: slot %lld served %d times", (long long)W, (long long)slice_rows, (long long)p, hit[(size_t)p]);
  }
}

int main() {
  CHECK(ISQ_THREADS == 1024 && ISQ_WAVES == 16 && ISQ_MAX_PROBE == 1024 && ISQ_MIN_SLICE == 64 && IVF_CAND_BYTES == 67108864, "constants");

  // ---- W: the nprobe longest lists, rounded up to 64, at least 64
  const int64_t off_a[] = {0, 10, 10, 110, 115, 415};   // lengths 10, 0, 100, 5, 300
  CHECK(ivf_candidate_width(off_a, 5, 1) == 320, "W of the longest list");
  CHECK(ivf_candidate_width(off_a, 5, 2) == 448, "W of the two longest (400 -> 448)");
  CHECK(ivf_candidate_width(off_a, 5, 3) == 448, "W of the three longest (410 -> 448)");
  CHECK(ivf_candidate_width(off_a, 5, 5) == 448, "W of all lists (415 -> 448)");
  const int64_t off_b[] = {0, 0, 0, 0};
  CHECK(ivf_candidate_width(off_b, 3, 1) == 64 && ivf_candidate_width(off_b, 3, 3) == 64, "W of empty lists");
  const int64_t off_c[] = {0, 64, 128};
  CHECK(ivf_candidate_width(off_c, 2, 1) == 64 && ivf_candidate_width(off_c, 2, 2) == 128, "W on a multiple of 64");
  const int64_t off_d[] = {0, 2147483647};
  CHECK(ivf_candidate_width(off_d, 1, 1) == 2147483648LL, "W of the largest index");

  // ---- the query block: all queries up to 65535, within 64 MiB of 8-byte slots, at least one
  CHECK(ivf_query_block(1, 64) == 1 && ivf_query_block(100, 64) == 100, "query block, small");
  CHECK(ivf_query_block(100000, 64) == 65535, "query block, grid.y");
  CHECK(ivf_query_block(100000, 1024) == 8192, "query block, 64 MiB / (8 * 1024)");
  CHECK(ivf_query_block(64, 100032) == 64 && ivf_query_block(64, 1000000) == 8, "query block at W = 10^5 and 10^6");
  CHECK(ivf_query_block(5, 2147483648LL) == 1, "query block, one row over the budget");

  // ---- slices, 256 compute units
  expect_slices("one query, W = 100032", 256, 1, 100032, 0, 208, 481);          // want 512, G0 512, ceil(100032 / 512) = 196 -> 208
  expect_slices("64 queries, W = 100032", 256, 64, 100032, 0, 12512, 8);        // want 8, ceil(100032 / 8) = 12504 -> 12512
  expect_slices("one query, W = 448", 256, 1, 448, 0, 64, 7);                   // W / 64 = 7 bounds G0
  expect_slices("one query, W = 64", 256, 1, 64, 0, 64, 1);
  expect_slices("1024 queries, W = 4096", 256, 1024, 4096, 0, 4096, 1);         // want 1
  expect_slices("300 queries, W = 4096", 256, 300, 4096, 0, 2048, 2);           // want 2
  expect_slices("seam 16", 256, 1, 448, 16, 16, 28);
  expect_slices("seam 48", 256, 1, 448, 48, 48, 10);
  expect_slices("seam 17 -> 32", 256, 1, 448, 17, 32, 14);
  expect_slices("seam 4096", 256, 1, 448, 4096, 4096, 1);
  expect_slices("seam 1 -> 16", 256, 1, 64, 1, 16, 4);

  // ---- generic properties
  const int cus[] = {1, 8, 256, 304};
  const int64_t QBs[] = {1, 2, 3, 17, 64, 511, 512, 513, 8192, 65535};
  const int64_t Ws[] = {64, 128, 192, 448, 1024, 4032, 4096, 100032, 1000000 / 64 * 64, 2147483648LL};
  const int64_t seams[] = {0, 1, 15, 16, 17, 48, 64, 100, 4096, 2147483647};
  for (int cu : cus)
    for (int64_t QB : QBs)
      for (int64_t W : Ws)
        for (int64_t s : seams) properties(cu, QB, W, s);

  if (g_fail) {
    fprintf(stderr, "ivf_sq8_plan_check: %d checks failed\n", g_fail);
    return 1;
  }
  printf("ivf_sq8_plan_check: ok\n");
  return 0;
}
