// Host-only check of the host part of pq_common.hpp (tests/test_pq_host.py builds it with -fsanitize=address,undefined and runs it):
// scan_plan against the arithmetic the two scans carried inline before they shared it -- the segment size and LDS bytes in their
// launchers, the load-width predicates in their kernels -- for both entry budgets, code bases at byte offsets 0, 4 and 1, and the
// (m, ksub) of the segment-limit cases of tests/test_gpu_pq.py and tests/test_gpu_ivf.py.  Exit status 0 = every check held.
#include <cstdio>

#include "../pq_common.hpp"

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

// the closed forms, as plain integers (al = the code base modulo 16)
static void one_case(int m, int ksub, int entries, const char* base, int al, bool flat_case) {
  const int seg_m = entries / ksub > 1 ? entries / ksub : 1;
  const size_t lds = (size_t)(m < seg_m ? m : seg_m) * ksub * 4;
  const bool one_seg = seg_m >= m;
  const bool vec = m % 16 == 0 && (one_seg || seg_m % 16 == 0) && al % 16 == 0;   // the probed scan's 16-byte rule
  const bool dw = m % 4 == 0 && (one_seg || seg_m % 4 == 0) && al % 4 == 0;       // the probed scan's 4-byte rule
  const ScanPlan p = scan_plan(m, ksub, entries, base + al);
  CHECK(p.seg_m == seg_m && p.lds == lds, "m=%d ksub=%d entries=%d: seg_m %d lds %zu against %d %zu", m, ksub, entries, p.seg_m, p.lds, seg_m,
        lds);
  CHECK(p.width == (vec ? 16 : dw ? 4 : 1), "m=%d ksub=%d entries=%d offset=%d: width %d", m, ksub, entries, al, p.width);
  if (flat_case) {
    // The flat scan asked for seg_m % 4 == 0 of a single segment too, where no segment starts inside a dword.  scan_plan follows
    // the probed scan there: ONE DIFFERENCE from what the flat scan computed -- a single segment whose seg_m is no multiple of 4
    // now takes 4-byte loads (aligned, same order of additions) where it took bytes.  Everything else is equal.
    const bool flat_dw = m % 4 == 0 && seg_m % 4 == 0 && al % 4 == 0;
    const bool widened = one_seg && seg_m % 4 != 0 && m % 4 == 0 && al % 4 == 0;
    CHECK((p.width >= 4) == (flat_dw || widened), "m=%d ksub=%d entries=%d offset=%d: flat 4-byte rule", m, ksub, entries, al);
    CHECK((p.width >= 4 && m <= 64) == (m % 4 == 0 && m <= 64 && al % 4 == 0), "m=%d offset=%d: register path", m, al);
  }
}

int main() {
  alignas(16) static const char buf[32] = {};
  const int budgets[] = {40960, 36864}, offsets[] = {0, 4, 1};
  // test_gpu_pq.py: the segment-limit cases, the shapes of the scan cases and of the load-width cases
  const int flat[][2] = {{160, 256}, {369, 111}, {161, 256}, {370, 111}, {200, 256}, {8, 256}, {64, 256}, {3, 255}, {5, 16},
                         {80, 256},  {176, 256}, {68, 256},  {67, 256},  {4, 4},     {1, 1},     {372, 100}};
  // test_gpu_ivf.py: above the limit, and more than one segment on each load width
  const int probed[][2] = {{161, 256}, {160, 256}, {148, 256}, {372, 100}, {16, 256}, {6, 255}, {7, 64}, {32, 256}};
  for (int entries : budgets)
    for (int al : offsets) {
      for (const auto& c : flat) one_case(c[0], c[1], entries, buf, al, true);
      for (const auto& c : probed) one_case(c[0], c[1], entries, buf, al, false);
    }
  // what the GPU tests rely on, spelled out
  CHECK(scan_plan(80, 256, 40960, buf).width == 16 && scan_plan(80, 256, 40960, buf + 4).width == 4 && scan_plan(80, 256, 40960, buf + 1).width == 1,
        "m = 80 at offsets 0, 4, 1");
  CHECK(scan_plan(176, 256, 40960, buf).seg_m == 160 && scan_plan(176, 256, 40960, buf).width == 16, "m = 176: segments of 160 + 16");
  CHECK(scan_plan(68, 256, 40960, buf).width == 4 && scan_plan(67, 256, 40960, buf).width == 1, "m = 68, 67");
  CHECK(scan_plan(160, 256, 36864, buf).seg_m == 144 && scan_plan(160, 256, 36864, buf).lds == 144 * 1024, "probed budget: 144 KiB");
  // the difference spelled out: (372, 100) is one segment of the flat budget with seg_m = 409; the flat scan read it by bytes
  CHECK(scan_plan(372, 100, 40960, buf).seg_m == 409 && scan_plan(372, 100, 40960, buf).width == 4, "(372, 100): the widened case");
  CHECK(scan_plan(1, 1, 40960, buf).seg_m == 40960 && scan_plan(1, 1, 40960, buf).lds == 4, "m = ksub = 1");

  CHECK(scan_shape_ok(1, 1) && scan_shape_ok(1 << 24, 256), "range: the corners");
  CHECK(!scan_shape_ok(0, 16) && !scan_shape_ok((1 << 24) + 1, 16) && !scan_shape_ok(4, 0) && !scan_shape_ok(4, 257) && !scan_shape_ok(-1, -1),
        "range: just outside");

  if (g_fail) {
    fprintf(stderr, "scan_plan_check: %d checks failed\n", g_fail);
    return 1;
  }
  printf("scan_plan_check: ok\n");
  return 0;
}
