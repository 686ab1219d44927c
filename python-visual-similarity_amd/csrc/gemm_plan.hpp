// The launch plan of the similarity GEMMs as a host-only rule (no HIP types): which tiles exist and in what order, and how
// the list is cut into a main launch of whole tiles and a split-K tail.  cosine.hip caches and uploads what this header
// decides; bench/gemm_plan_check.cpp (tests/test_gemm_plan_host.py) sweeps the rule on the CPU.
#pragma once
#include <algorithm>
#include <vector>

namespace pvs {

struct GemmTile {
  int tm, tn;
};

// how the tile list is cut into launches: entries [0, n_main) run whole, entries [n_main, n_main + n_tail) split along K
struct GemmCut {
  int n_main, n_tail, splitk;
};

// Tile order: 8x8 super-tiles for L2 panel sharing; the upper triangle (tn >= tm) only when A == B (symm, tiles_n unused).
inline void gemm_plan_tiles(int tiles_m, int tiles_n, bool symm, std::vector<GemmTile>& t) {
  t.clear();
  if (symm) {
    const int TS = (tiles_m + 7) / 8;
    for (int si = 0; si < TS; ++si)
      for (int sj = si; sj < TS; ++sj)
        for (int w = 0; w < 64; ++w) {
          const int tm = si * 8 + (w & 7), tn = sj * 8 + (w >> 3);
          if (tm < tiles_m && tn < tiles_m && tn >= tm) t.push_back({tm, tn});
        }
  } else {
    for (int g0 = 0; g0 < tiles_m; g0 += 8) {
      const int gsz = std::min(8, tiles_m - g0);
      for (int tn = 0; tn < tiles_n; ++tn)
        for (int dm = 0; dm < gsz; ++dm) t.push_back({g0 + dm, tn});
    }
  }
}

// How to cut the work into launches.  One tile takes the same time T whether the chip is full or not, so a problem of
// few tiles (a rank's share in the multi-GPU scheme, a query batch) is fast only when its tiles are split along K into
// s slices (whole 1024-k chains each; the reduce adds the chain images in chain order, so the scores do not change).
// Cost in units of T:  rounds(blocks) * (1/s + eps) + the reduce's traffic;  candidates: full rounds unsplit + the last
// partial round split (A), or every tile split (B).
inline GemmCut gemm_plan_cut(int total, int slots) {
  GemmCut P;
  const double eps = 0.02, red = 3.0e-4;
  auto rounds = [&](long blocks) { return (double)((blocks + slots - 1) / slots); };
  const int full = total / slots, rem = total % slots;
  double best = rounds(total);            // nothing split
  P.n_main = total;
  P.n_tail = 0;
  P.splitk = 1;
  for (int sk = 2; sk <= 32; sk *= 2) {
    if (rem > 0) {
      const double a = full + rounds((long)rem * sk) * (1.0 / sk + eps) + red * rem;
      if (a < best - 1e-9) { best = a; P.n_main = total - rem; P.n_tail = rem; P.splitk = sk; }
    }
    if (total < 4 * slots) {
      const double b = rounds((long)total * sk) * (1.0 / sk + eps) + red * total;
      if (b < best - 1e-9) { best = b; P.n_main = 0; P.n_tail = total; P.splitk = sk; }
    }
  }
  return P;
}

}  // namespace pvs
