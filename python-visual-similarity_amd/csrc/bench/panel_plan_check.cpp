// Host-only check of the host part of panel_plan.hpp (tests/test_topk_host.py builds it with -fsanitize=address,undefined and runs it).
// The expected block sizes are literals worked out by hand from the rules as DESIGN.md section 23 states them, not a restatement of
// the formulas; the sweep then holds what every rule promises: the blocks tile [0, nq) x [0, N) exactly once, QT >= 1, NC >= 1, and a
// panel stays within the 1 GiB budget unless it is one complete row.  Exit status 0 = every check held.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../panel_plan.hpp"

using namespace pvs;

static char g_error[256];
void pvs::set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
}

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

constexpr int64_t P27 = 134217728, P28 = 268435456, GIB = 1073741824;

// QT and NC, and the number and the last size of the blocks on either axis, walked the way the driver walks them
static void expect(const char* what, const PanelPlan& p, int64_t QT, int64_t NC, int64_t qblocks, int64_t last_q, int64_t cblocks,
                   int64_t last_c) {
  CHECK(p.QT == QT && p.NC == NC, "%s: QT %lld NC %lld", what, (long long)p.QT, (long long)p.NC);
  int64_t nqb = 0, ncb = 0, lq = 0, lc = 0;
  for (int64_t q0 = 0; q0 < p.nq; q0 += p.QT) ++nqb, lq = p.qn(q0);
  for (int64_t c0 = 0; c0 < p.N; c0 += p.NC) ++ncb, lc = p.cn(c0);
  CHECK(nqb == qblocks && lq == last_q && ncb == cblocks && lc == last_c, "%s: %lld query blocks (last %lld), %lld column blocks (last %lld)",
        what, (long long)nqb, (long long)lq, (long long)ncb, (long long)lc);
}

static PanelPlan ranking(PanelPlan (*rule)(int64_t, int64_t), int64_t nq, int64_t N, int k, int merge, int want_rc) {
  PanelPlan p{-1, -1, -1, -1};
  g_error[0] = 0;
  const int rc = panel_ranking_plan(rule, nq, N, k, merge, &p);
  CHECK(rc == want_rc, "ranking plan nq=%lld N=%lld k=%d merge=%d: status %d", (long long)nq, (long long)N, k, merge, rc);
  if (want_rc == PVS_OK) {
    CHECK(g_error[0] == 0 && p.nq == nq && p.N == N, "ranking plan nq=%lld N=%lld k=%d: message or problem size", (long long)nq, (long long)N, k);
  } else {
    char msg[64];
    snprintf(msg, sizeof msg, "ranking depth %d needs a single panel", k);
    CHECK(strcmp(g_error, msg) == 0 && p.QT == -1, "refusal at k=%d: message '%s'", k, g_error);
  }
  return p;
}

// ---- the generic properties of one plan over `elems` scores; `one_row_may_exceed`: a complete-row plan
static void properties(const char* what, const PanelPlan& p, int64_t elems, bool one_row_may_exceed) {
  CHECK(p.QT >= 1 && p.NC >= 1 && p.QT <= p.nq && p.NC <= p.N, "%s nq=%lld N=%lld: QT %lld NC %lld", what, (long long)p.nq, (long long)p.N,
        (long long)p.QT, (long long)p.NC);
  if (p.QT < 1 || p.NC < 1) return;
  const bool within = p.QT <= elems / p.NC;   // QT * NC <= elems without the product
  CHECK(within || (one_row_may_exceed && p.QT == 1 && p.NC == p.N), "%s nq=%lld N=%lld: %lld x %lld scores", what, (long long)p.nq,
        (long long)p.N, (long long)p.QT, (long long)p.NC);
  // exactly once: the query blocks follow each other from 0 to nq, the column blocks from 0 to N, none empty, none beyond its size
  int64_t q_end = 0, c_end = 0;
  for (int64_t q0 = 0; q0 < p.nq; q0 += p.QT) {
    CHECK(q0 == q_end && p.qn(q0) >= 1 && p.qn(q0) <= p.QT, "%s nq=%lld: query block at %lld", what, (long long)p.nq, (long long)q0);
    q_end = q0 + p.qn(q0);
  }
  for (int64_t c0 = 0; c0 < p.N; c0 += p.NC) {
    CHECK(c0 == c_end && p.cn(c0) >= 1 && p.cn(c0) <= p.NC, "%s N=%lld: column block at %lld", what, (long long)p.N, (long long)c0);
    c_end = c0 + p.cn(c0);
  }
  CHECK(q_end == p.nq && c_end == p.N, "%s nq=%lld N=%lld: covered %lld x %lld", what, (long long)p.nq, (long long)p.N, (long long)q_end,
        (long long)c_end);
}

int main() {
  CHECK(PANEL_BUDGET_BYTES == GIB && panel_elems<float>() == P28 && panel_elems<double>() == P27 && PANEL_PAGED_K == 1024, "budget");

  // ---- dense
  expect("dense 1x1", ranking(panel_dense, 1, 1, 1, 0, PVS_OK), 1, 1, 1, 1, 1, 1);
  const PanelPlan d2 = ranking(panel_dense, 8193, 32769, 10, 0, PVS_OK);
  expect("dense 8193x32769", d2, 8192, 32768, 2, 1, 2, 1);
  CHECK(panel_bytes<float>(d2) == (size_t)GIB, "dense panel bytes %zu", panel_bytes<float>(d2));
  expect("dense merge, k=1024", ranking(panel_dense, 9000, 40000, 1024, 1, PVS_OK), 8192, 32768, 2, 808, 2, 7232);
  expect("dense deep 5x5000", ranking(panel_dense, 5, 5000, 1025, 0, PVS_OK), 5, 5000, 1, 5, 1, 5000);
  const PanelPlan d4 = ranking(panel_dense, 3, P28, 2000, 0, PVS_OK);
  expect("dense deep 3x2^28", d4, 1, P28, 3, 1, 1, P28);
  CHECK(panel_bytes<float>(d4) == (size_t)GIB, "deep row bytes %zu", panel_bytes<float>(d4));
  expect("dense deep 8193x32768", ranking(panel_dense, 8193, 32768, 1025, 0, PVS_OK), 8192, 32768, 2, 1, 1, 32768);
  expect("dense deep 4097x65536", ranking(panel_dense, 4097, 65536, 1025, 0, PVS_OK), 4096, 65536, 2, 1, 1, 65536);
  ranking(panel_dense, 3, P28 + 1, 1025, 0, PVS_ERR_UNSUPPORTED);
  ranking(panel_dense, 5, 5000, 1025, 1, PVS_ERR_UNSUPPORTED);
  ranking(panel_dense, 5, 5000, 5000, 7, PVS_ERR_UNSUPPORTED);

  // ---- scan (ADC and Int8)
  const PanelPlan s1 = ranking(panel_scan, 1100, 4099, 10, 0, PVS_OK);
  expect("scan 1100x4099", s1, 1024, 4096, 2, 76, 2, 3);
  CHECK(panel_bytes<float>(s1) == (size_t)16777216, "scan panel bytes %zu", panel_bytes<float>(s1));
  expect("scan 1024x4100", ranking(panel_scan, 1024, 4100, 10, 1, PVS_OK), 1024, 4096, 1, 1024, 2, 4);
  expect("scan 3x5000000", ranking(panel_scan, 3, 5000000, 10, 0, PVS_OK), 3, 1398101, 1, 3, 4, 805697);
  expect("scan 1x10^7", ranking(panel_scan, 1, 10000000, 1, 0, PVS_OK), 1, 4194304, 1, 1, 3, 1611392);
  expect("scan 2000x100", ranking(panel_scan, 2000, 100, 100, 0, PVS_OK), 1024, 100, 2, 976, 1, 100);
  expect("scan deep 5x5000", ranking(panel_scan, 5, 5000, 1025, 0, PVS_OK), 5, 5000, 1, 5, 1, 5000);
  expect("scan deep 3x2^28", ranking(panel_scan, 3, P28, 2000, 0, PVS_OK), 1, P28, 3, 1, 1, P28);
  ranking(panel_scan, 3, P28 + 1, 1025, 0, PVS_ERR_UNSUPPORTED);
  ranking(panel_scan, 5, 5000, 1025, 1, PVS_ERR_UNSUPPORTED);

  // ---- complete rows of float64
  expect("f64 100x3000000", panel_full_rows(100, 3000000, panel_elems<double>()), 44, 3000000, 3, 12, 1, 3000000);
  const PanelPlan f2 = panel_full_rows(8193, 16384, panel_elems<double>());
  expect("f64 8193x16384", f2, 8192, 16384, 2, 1, 1, 16384);
  CHECK(panel_bytes<double>(f2) == (size_t)GIB, "f64 panel bytes %zu", panel_bytes<double>(f2));
  const PanelPlan f3 = panel_full_rows(2, P27 + 1, panel_elems<double>());
  expect("f64 2x(2^27+1)", f3, 1, P27 + 1, 2, 1, 1, P27 + 1);
  CHECK(panel_bytes<double>(f3) == (size_t)GIB + 8, "f64 single row bytes %zu", panel_bytes<double>(f3));
  expect("f64 7x50", panel_full_rows(7, 50, panel_elems<double>()), 7, 50, 1, 7, 1, 50);

  // ---- filtered top-k
  expect("filter square 4096", panel_filter(4096, 4096, true), 4096, 4096, 1, 4096, 1, 4096);
  expect("filter 600x40000", panel_filter(600, 40000, false), 600, 32768, 1, 600, 2, 7232);
  expect("filter 10000x32768", panel_filter(10000, 32768, false), 8192, 32768, 2, 1808, 1, 32768);
  expect("filter same 20000 (over the budget)", panel_filter(20000, 20000, true), 13421, 20000, 2, 6579, 1, 20000);
  expect("filter same 40000 (two column blocks)", panel_filter(40000, 40000, true), 8192, 32768, 5, 7232, 2, 7232);
  expect("filter 100x100", panel_filter(100, 100, false), 100, 100, 1, 100, 1, 100);
  expect("filter 3000000x100", panel_filter(3000000, 100, false), 2684354, 100, 2, 315646, 1, 100);
  CHECK(panel_full_rows(7, 100000000, panel_elems<float>()).QT == 2, "filter overflow batch of 7 rows, N = 10^8");
  CHECK(panel_full_rows(0, 1000, panel_elems<float>()).QT == 1, "filter overflow batch of no rows");

  // ---- bit mask of the int8 threshold join: 8192 x 262144 bits, rows in whole 128-row tiles, 4 words per 128 columns
  expect("mask 1x1", panel_mask(1, 1), 1, 1, 1, 1, 1, 1);
  CHECK(panel_mask_bytes(panel_mask(1, 1)) == (size_t)2048, "mask 1x1 bytes %zu", panel_mask_bytes(panel_mask(1, 1)));
  const PanelPlan m1 = panel_mask(8189, 32768);
  expect("mask 8189x32768", m1, 8189, 32768, 1, 8189, 1, 32768);
  CHECK(panel_mask_bytes(m1) == (size_t)33554432, "mask 8189x32768 bytes %zu", panel_mask_bytes(m1));
  const PanelPlan m2 = panel_mask(8193, 262145);
  expect("mask 8193x262145", m2, 8192, 262144, 2, 1, 2, 1);
  CHECK(panel_mask_bytes(m2) == (size_t)268435456, "mask 8193x262145 bytes %zu", panel_mask_bytes(m2));
  expect("mask 1000000x1000000", panel_mask(1000000, 1000000), 8192, 262144, 123, 576, 4, 213568);
  CHECK(panel_mask_words(1) == 4 && panel_mask_words(128) == 4 && panel_mask_words(129) == 8 && panel_mask_words(100) == 4 &&
            panel_mask_words(262144) == 8192,
        "mask words");
  CHECK(panel_mask_bytes(PanelPlan{129, 160, 129, 160}) == (size_t)256 * 8 * 4, "mask bytes of a 129 x 160 tile");
  CHECK(panel_mask_bytes(PanelPlan{40000, 40000, 32768, 32768}) == (size_t)134217728, "mask bytes of the largest test tile");

  // ---- query block of the host float64 entry
  CHECK(host_f64_query_block(1000, 1000000, 1000000, false) == 134, "host f64 block, 10^6 x 10^6");
  CHECK(host_f64_query_block(1000, 1000000, 2000000, false) == 134, "host f64 block, the panel bounds it");
  CHECK(host_f64_query_block(1000, 1000000, 4000000, false) == 67, "host f64 block, 2 GiB of rows bound it");
  CHECK(host_f64_query_block(50, 1000, 1000, false) == 50, "host f64 block, all queries");
  CHECK(host_f64_query_block(5, P27 + 1, 2, false) == 1, "host f64 block, one row over the budget");
  CHECK(host_f64_query_block(100000, 100000, 64, true) == 100000, "host f64 block, same operands: uncapped, as it always was");

  // ---- generic properties
  const int64_t nqs[] = {1, 2, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193, 20000, 100000, 3000000};
  const int64_t Ns[] = {1, 3, 4095, 4096, 4097, 32767, 32768, 32769, 65536, 1398101, 4194305, 10000000, P27, P27 + 1, P28 - 1, P28};
  const int ks[] = {1, 1024, 1025, 5000};
  for (int64_t nq : nqs)
    for (int64_t N : Ns) {
      for (int k : ks) {
        properties("dense", ranking(panel_dense, nq, N, k, 0, PVS_OK), panel_elems<float>(), k > 1024);
        properties("scan", ranking(panel_scan, nq, N, k, 0, PVS_OK), k > 1024 ? panel_elems<float>() : (int64_t)1 << 22, k > 1024);
      }
      properties("full rows f64", panel_full_rows(nq, N, panel_elems<double>()), panel_elems<double>(), true);
      properties("full rows f32", panel_full_rows(nq, N, panel_elems<float>()), panel_elems<float>(), true);
      properties("mask", panel_mask(nq, N), 8 * GIB, false);   // one bit per pair
      CHECK(panel_mask_bytes(panel_mask(nq, N)) <= (size_t)PANEL_BUDGET_BYTES / 4, "mask nq=%lld N=%lld: %zu bytes", (long long)nq, (long long)N,
            panel_mask_bytes(panel_mask(nq, N)));
      properties("filter", panel_filter(nq, N, false), panel_elems<float>(), false);
      if (nq == N) properties("filter, same operands", panel_filter(nq, N, true), panel_elems<float>(), false);
      for (int64_t L : {(int64_t)2, (int64_t)32768, (int64_t)300000000}) {
        const int64_t QB = host_f64_query_block(nq, N, L, false);
        CHECK(QB >= 1 && QB <= nq && (QB == 1 || (QB <= panel_elems<double>() / N && QB <= 268435456 / L)), "host f64 block nq=%lld N=%lld L=%lld: %lld",
              (long long)nq, (long long)N, (long long)L, (long long)QB);
      }
    }

  if (g_fail) {
    fprintf(stderr, "panel_plan_check: %d checks failed\n", g_fail);
    return 1;
  }
  printf("panel_plan_check: ok\n");
  return 0;
}
