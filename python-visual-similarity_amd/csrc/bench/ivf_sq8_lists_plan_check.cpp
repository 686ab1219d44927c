// Host-only check of the scan-by-list rules of ivf_sq8_plan.hpp (tests/test_ivf_sq8_lists_host.py builds it with
// -fsanitize=address,undefined and runs it): the query block, the row tiles and the pair capacity against
// literal values worked out by hand from the rules as the section states them, then over a sweep of ragged lists and probes that
// row tiles x query tiles, walked the way the tile kernel walks them, write every live (query, slot) exactly once and no other slot.
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

static void expect_plan(const char* what, const std::vector<int64_t>& len, int nprobe, int64_t nq, int64_t query_block, int64_t W, int64_t QB,
                        int64_t row_tiles, int64_t pairs) {
  std::vector<int64_t> off(len.size() + 1, 0);
  for (size_t l = 0; l < len.size(); ++l) off[l + 1] = off[l] + len[l];
  const IsqlPlan p = isql_plan(off.data(), (int)len.size(), nprobe, nq, query_block);
  CHECK(p.W == W && p.QB == QB && p.row_tiles == row_tiles && p.pairs == pairs, "%s: W %lld QB %lld row_tiles %lld pairs %lld", what, (long long)p.W,
        (long long)p.QB, (long long)p.row_tiles, (long long)p.pairs);
}

static uint64_t g_state = 88172645463325252ull;
static uint32_t next_u32() {   // xorshift64: the sweep is the same on every run
  g_state ^= g_state << 13;
  g_state ^= g_state >> 7;
  g_state ^= g_state << 17;
  return (uint32_t)(g_state >> 32);
}

// one case: nlist ragged lists, qn queries of nprobe distinct probes each (some replaced by -1 or nlist), grouped by a stable
// counting sort on the list, then every row tile against every query tile of its group
static void coverage(int nlist, int nprobe, int qn, int max_len) {
  std::vector<int64_t> off((size_t)nlist + 1, 0);
  const int64_t shapes[] = {0, 1, 127, 128, 129, 257};
  for (int l = 0; l < nlist; ++l) {
    const uint32_t u = next_u32();
    const int64_t len = (u & 3) == 0 ? shapes[(u >> 2) % 6] : (int64_t)((u >> 2) % (uint32_t)(max_len + 1));
    off[(size_t)l + 1] = off[(size_t)l] + len;
  }
  const IsqlPlan plan = isql_plan(off.data(), nlist, nprobe, qn, 0);
  const int64_t W = plan.W;
  CHECK(plan.QB >= 1 && plan.QB <= qn && plan.pairs == plan.QB * nprobe && plan.pairs <= std::max<int64_t>(ISQL_MAX_PAIRS, nprobe), "plan of nlist=%d nprobe=%d qn=%d",
        nlist, nprobe, qn);
  // probes: the first nprobe entries of a shuffle of the lists
  std::vector<int64_t> probe((size_t)qn * nprobe);
  std::vector<int> perm((size_t)nlist);
  for (int q = 0; q < qn; ++q) {
    for (int l = 0; l < nlist; ++l) perm[(size_t)l] = l;
    for (int j = 0; j < nprobe; ++j) {
      std::swap(perm[(size_t)j], perm[(size_t)j + next_u32() % (uint32_t)(nlist - j)]);
      int64_t l = perm[(size_t)j];
      const uint32_t u = next_u32() % 16;
      if (u == 0) l = -1;
      if (u == 1) l = nlist;
      probe[(size_t)q * nprobe + j] = l;
    }
  }
  // base, total
  std::vector<int64_t> base((size_t)qn * nprobe), total((size_t)qn, 0);
  for (int q = 0; q < qn; ++q)
    for (int j = 0; j < nprobe; ++j) {
      const int64_t l = probe[(size_t)q * nprobe + j];
      base[(size_t)q * nprobe + j] = total[(size_t)q];
      if (l >= 0 && l < nlist) total[(size_t)q] += off[(size_t)l + 1] - off[(size_t)l];
    }
  // the stable grouping
  std::vector<int64_t> goff((size_t)nlist + 2, 0);
  for (int64_t l : probe)
    if (l >= 0 && l < nlist) ++goff[(size_t)l + 1];
  for (int l = 0; l < nlist; ++l) goff[(size_t)l + 1] += goff[(size_t)l];
  std::vector<int64_t> fill(goff.begin(), goff.end() - 1), gq((size_t)goff[(size_t)nlist]), gbase((size_t)goff[(size_t)nlist]);
  for (int64_t s = 0; s < (int64_t)probe.size(); ++s) {
    const int64_t l = probe[(size_t)s];
    if (l < 0 || l >= nlist) continue;
    gq[(size_t)fill[(size_t)l]] = s / nprobe;
    gbase[(size_t)fill[(size_t)l]++] = base[(size_t)s];
  }
  // the tiles
  std::vector<int> hit((size_t)qn * (size_t)W, 0);
  int64_t tiles = 0;
  for (int l = 0; l < nlist; ++l) {
    const int64_t first = off[(size_t)l], end = off[(size_t)l + 1];
    CHECK(isql_list_tiles(end - first) == (end - first + 127) / 128, "tiles of a list of %lld", (long long)(end - first));
    for (int64_t t = 0; t < isql_list_tiles(end - first); ++t, ++tiles) {
      const int64_t d0 = first + t * ISQL_ROWS;
      const int64_t g0 = goff[(size_t)l], g1 = goff[(size_t)l + 1];
      for (int64_t qt = 0; qt < isql_query_tiles(g1 - g0); ++qt)
        for (int64_t p = g0 + qt * ISQL_PAIRS; p < std::min(g0 + (qt + 1) * ISQL_PAIRS, g1); ++p)
          for (int64_t row = d0; row < std::min(d0 + ISQL_ROWS, end); ++row) {
            const int64_t slot = gbase[(size_t)p] + (row - first);
            CHECK(slot >= 0 && slot < W, "slot %lld of W %lld", (long long)slot, (long long)W);
            if (slot >= 0 && slot < W) ++hit[(size_t)(gq[(size_t)p] * W + slot)];
          }
    }
  }
  CHECK(tiles == plan.row_tiles, "nlist=%d: %lld tiles walked, the plan says %lld", nlist, (long long)tiles, (long long)plan.row_tiles);
  for (int q = 0; q < qn; ++q) {
    CHECK(total[(size_t)q] <= W, "query %d: %lld live slots of W %lld", q, (long long)total[(size_t)q], (long long)W);
    for (int64_t s = 0; s < W; ++s)
      CHECK(hit[(size_t)(q * W + s)] == (s < total[(size_t)q] ? 1 : 0), "nlist=%d nprobe=%d qn=%d: slot (%d, %lld) written %d times, %lld live", nlist,
            nprobe, qn, q, (long long)s, hit[(size_t)(q * W + s)], (long long)total[(size_t)q]);
  }
}

int main() {
  CHECK(ISQL_ROWS == 128 && ISQL_PAIRS == 128 && ISQL_MAX_PAIRS == 1048576 && ISQL_GROUP_BYTES == 33554432, "constants");
  CHECK(isql_list_tiles(0) == 0 && isql_list_tiles(1) == 1 && isql_list_tiles(128) == 1 && isql_list_tiles(129) == 2 && isql_list_tiles(257) == 3,
        "row tiles of a list");
  CHECK(isql_query_tiles(0) == 0 && isql_query_tiles(127) == 1 && isql_query_tiles(130) == 2 && isql_query_tiles(257) == 3, "query tiles of a group");

  // ---- the plan, by hand
  expect_plan("five ragged lists", {10, 0, 100, 5, 300}, 2, 64, 0, 448, 64, 6, 128);          // tiles 1 + 0 + 1 + 1 + 3; W 400 -> 448
  expect_plan("one query", {10, 0, 100, 5, 300}, 5, 1, 0, 448, 1, 6, 5);
  expect_plan("empty index", {0, 0, 0}, 3, 7, 0, 64, 7, 0, 21);
  expect_plan("tile seams", {128, 129, 0}, 1, 3, 0, 192, 3, 3, 3);                             // W 129 -> 192
  expect_plan("query_block below the rule", {10, 0, 100, 5, 300}, 2, 64, 5, 448, 5, 6, 10);
  expect_plan("query_block above the rule", {10, 0, 100, 5, 300}, 2, 64, 1000000, 448, 64, 6, 128);
  expect_plan("the pair budget", std::vector<int64_t>(1024, 1), 1024, 100000, 0, 1024, 1024, 1024, 1048576);   // 8192 by the slots, 2^20 / 1024 by the pairs
  expect_plan("the slot budget", std::vector<int64_t>(256, 3907), 256, 1024, 0, 1000192, 8, 7936, 2048);       // 64 MiB / (8 x 1000192) = 8; 31 tiles a list
  expect_plan("the timing record's shape", std::vector<int64_t>(256, 391), 256, 64, 0, 100096, 64, 1024, 16384);
  expect_plan("one long list", {2147483647}, 1, 4, 0, 2147483648LL, 1, 16777216, 1);

  // ---- row tiles x query tiles cover every live (query, slot) once
  const int nlists[] = {1, 2, 7, 64, 300};
  const int qns[] = {1, 3, 17, 130, 257};
  for (int nlist : nlists)
    for (int qn : qns) {
      const int nprobes[] = {1, std::min(2, nlist), std::min(nlist, 9), nlist > 64 ? 40 : nlist};
      for (int nprobe : nprobes) coverage(nlist, nprobe, qn, nlist >= 64 ? 20 : 300);
    }

  if (g_fail) {
    fprintf(stderr, "ivf_sq8_lists_plan_check: %d checks failed\n", g_fail);
    return 1;
  }
  printf("ivf_sq8_lists_plan_check: ok\n");
  return 0;
}
