// Host-only check of subset_common.hpp (tests/test_subset_host.py builds it with -fsanitize=address,undefined and runs it; nothing is
// loaded into Python).  The mask words against a bit-by-bit loop; the 64-column window for every col0 % 32, every lane and every tail of
// the mask against single-bit reads; the chunks of the listed path tiling [0, ns) exactly once; the empty-panel test and the panel's
// id range against a linear scan; the id check; the auto rule at its edge.  Exit status 0 = every check held.
#include <cstdio>
#include <vector>

#include "../subset_common.hpp"

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

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t next_u64() {   // xorshift64*
  g_rng ^= g_rng >> 12;
  g_rng ^= g_rng << 25;
  g_rng ^= g_rng >> 27;
  return g_rng * 0x2545f4914f6cdd1dull;
}

// every `keep_one_in`-th row on average, ascending
static std::vector<int64_t> random_ids(int64_t N, int keep_one_in) {
  std::vector<int64_t> ids;
  for (int64_t i = 0; i < N; ++i)
    if (next_u64() % (uint64_t)keep_one_in == 0) ids.push_back(i);
  if (ids.empty()) ids.push_back(N / 2);
  return ids;
}

static bool bit_of(const std::vector<int64_t>& ids, int64_t col) {   // the linear scan everything is held against
  for (int64_t i : ids)
    if (i == col) return true;
  return false;
}

static void check_mask_and_window(int64_t N, int keep_one_in) {
  const std::vector<int64_t> ids = random_ids(N, keep_one_in);
  const int64_t nwords = subset_words(N);
  CHECK(nwords == (N + 31) / 32, "N=%lld: %lld words", (long long)N, (long long)nwords);
  std::vector<uint32_t> words((size_t)nwords, 0xffffffffu);   // build must clear what it is given
  subset_build_mask(ids.data(), (int64_t)ids.size(), N, words.data());
  std::vector<char> want((size_t)(32 * nwords), 0);
  for (int64_t i : ids) want[(size_t)i] = 1;
  for (int64_t c = 0; c < 32 * nwords; ++c)
    CHECK(((words[(size_t)(c >> 5)] >> (c & 31)) & 1u) == (uint32_t)want[(size_t)c], "N=%lld: bit %lld", (long long)N, (long long)c);
  // windows: every start up to two words past the end, so every col0 % 32 meets every position of the tail
  for (int64_t col0 = 0; col0 < 32 * nwords + 64; ++col0) {
    const uint64_t w = subset_window64(words.data(), nwords, col0);
    for (int lane = 0; lane < 64; ++lane) {
      const int64_t c = col0 + lane;
      const bool expect = c < 32 * nwords && want[(size_t)c];
      CHECK((((w >> lane) & 1ull) != 0) == expect, "N=%lld col0=%lld (mod 32 = %lld) lane=%d", (long long)N, (long long)col0,
            (long long)(col0 & 31), lane);
    }
  }
}

static void check_panels(int64_t N, int keep_one_in, int64_t NC) {
  const std::vector<int64_t> ids = random_ids(N, keep_one_in);
  const int64_t ns = (int64_t)ids.size();
  int64_t seen = 0;
  for (int64_t c0 = 0; c0 < N; c0 += NC) {
    const int64_t cn = std::min(NC, N - c0);
    int64_t count = 0;
    for (int64_t c = c0; c < c0 + cn; ++c) count += bit_of(ids, c);
    int64_t a = -1, b = -1;
    subset_panel_range(ids.data(), ns, c0, cn, &a, &b);
    CHECK(b - a == count && a == seen, "N=%lld NC=%lld c0=%lld: range [%lld, %lld), %lld ids", (long long)N, (long long)NC, (long long)c0,
          (long long)a, (long long)b, (long long)count);
    CHECK(subset_panel_empty(ids.data(), ns, c0, cn) == (count == 0), "N=%lld NC=%lld c0=%lld: empty", (long long)N, (long long)NC, (long long)c0);
    seen += count;
  }
  CHECK(seen == ns, "N=%lld NC=%lld: panels hold %lld of %lld ids", (long long)N, (long long)NC, (long long)seen, (long long)ns);
}

static void check_chunks(int64_t ns, int64_t row_bytes, int tile, int64_t want_rows) {
  const int64_t rows = subset_chunk_rows(ns, row_bytes, tile);
  CHECK(rows == want_rows, "chunk rows ns=%lld row_bytes=%lld tile=%d: %lld", (long long)ns, (long long)row_bytes, tile, (long long)rows);
  CHECK(rows >= 1 && rows <= ns && (rows == 1 || rows * row_bytes <= SUBSET_STAGE_BYTES) && (tile == 0 || rows <= tile), "chunk bound");
  if (rows < 1) return;
  int64_t end = 0, chunks = 0;
  for (int64_t p0 = 0; p0 < ns; p0 += rows) {       // the loop of subset_listed_path
    const int64_t pn = std::min(rows, ns - p0);
    CHECK(p0 == end && pn >= 1 && pn <= rows, "chunk at %lld", (long long)p0);
    end = p0 + pn;
    ++chunks;
  }
  CHECK(end == ns && chunks == (ns + rows - 1) / rows, "chunks cover %lld of %lld", (long long)end, (long long)ns);
}

int main() {
  CHECK(SUBSET_STAGE_BYTES == 268435456 && SUBSET_MAX_K == 1024 && SUBSET_MAX_TILE == 32768, "constants");

  for (int64_t N : {1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 200})
    for (int keep : {1, 2, 5}) check_mask_and_window(N, keep);

  for (int64_t N : {1, 5, 47, 48, 49, 100, 333})
    for (int keep : {1, 3, 40})
      for (int64_t NC : {1, 7, 48, 64, 1000}) check_panels(N, keep, NC);

  // literals worked out by hand: 256 MiB / 131072 B = 2048 rows; one row when a row exceeds the budget; tile caps; ns caps
  check_chunks(100000, 131072, 0, 2048);
  check_chunks(100000, 131072, 48, 48);
  check_chunks(1000, 131072, 0, 1000);
  check_chunks(7, (int64_t)1 << 30, 0, 1);
  check_chunks(7, (int64_t)1 << 30, 48, 1);
  check_chunks(1, 64, 0, 1);
  check_chunks(5000000, 64, 0, 4194304);
  check_chunks(1000, 4000, 64, 64);
  check_chunks(48, 64, 48, 48);
  check_chunks(49, 64, 48, 48);

  // ids: strictly ascending within [0, N)
  {
    const int64_t good[] = {0, 3, 4, 9}, unsorted[] = {0, 4, 3}, twice[] = {1, 1}, high[] = {2, 10}, negative[] = {-1, 2};
    CHECK(subset_first_bad_id(good, 4, 10) == 0, "good ids");
    CHECK(subset_first_bad_id(unsorted, 3, 10) == 3, "unsorted ids");
    CHECK(subset_first_bad_id(twice, 2, 10) == 2, "a repeated id");
    CHECK(subset_first_bad_id(high, 2, 10) == 2, "an id equal to N");
    CHECK(subset_first_bad_id(negative, 2, 10) == 1, "a negative id");
  }

  // auto: the listed path iff 4 ns <= N
  CHECK(subset_auto_listed(25, 100) && !subset_auto_listed(26, 100) && subset_auto_listed(1, 4) && !subset_auto_listed(1, 3), "auto rule");

  if (g_fail) {
    fprintf(stderr, "subset_plan_check: %d checks failed\n", g_fail);
    return 1;
  }
  printf("subset_plan_check: ok\n");
  return 0;
}
