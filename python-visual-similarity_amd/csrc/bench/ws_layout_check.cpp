// Host-only check of workspace.hpp (tests/test_workspace_host.py builds it with -fsanitize=address,undefined and runs it):
// the generic properties of WsLayout, then four call sites held offset for offset against the closed-form byte arithmetic those sites
// carried inline before they were written with the layout, and the blocks of update.hip and asmk_update.hip against theirs.  Exit status 0 = every check held.
#include <cstdio>
#include <memory>

#include "../workspace.hpp"

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

template <size_t S>
struct Elem {
  char b[S];
};

// three pieces of (c0, c1, c2) elements of S bytes in a layout of alignment A
template <size_t A, size_t S>
static void generic_case(size_t c0, size_t c1, size_t c2) {
  WsLayout<A> lay;
  const size_t cnt[3] = {c0, c1, c2};
  size_t off[3];
  const WsPiece<Elem<S>> p0 = lay.template add<Elem<S>>(c0), p1 = lay.template add<Elem<S>>(c1), p2 = lay.template add<Elem<S>>(c2);
  off[0] = p0.off, off[1] = p1.off, off[2] = p2.off;
  CHECK(off[0] == 0, "first piece at %zu", off[0]);
  for (int i = 0; i < 3; ++i) {
    const size_t next = i < 2 ? off[i + 1] : lay.bytes();
    CHECK(off[i] % A == 0, "A=%zu S=%zu piece %d at %zu", A, S, i, off[i]);
    CHECK(next >= off[i] + cnt[i] * S, "A=%zu S=%zu piece %d: %zu elements at %zu, next at %zu", A, S, i, cnt[i], off[i], next);
    CHECK(next - off[i] < cnt[i] * S + A, "A=%zu S=%zu piece %d takes %zu bytes for %zu", A, S, i, next - off[i], cnt[i] * S);
  }
  // the typed pointers land inside a real block of bytes() (the sanitizers watch the writes)
  const std::unique_ptr<char[]> block(new char[lay.bytes()]);
  if (c0) p0(block.get())[c0 - 1].b[S - 1] = 1;
  if (c1) p1(block.get())[c1 - 1].b[S - 1] = 2;
  if (c2) p2(block.get())[c2 - 1].b[S - 1] = 3;
  CHECK(reinterpret_cast<char*>(p2(block.get())) == block.get() + off[2], "pointer of piece 2");
}

template <size_t A, size_t S>
static void generic_sweep() {
  const size_t counts[] = {0, 1, A - 1, A, A + 1, 3 * A + 7};
  for (size_t a : counts)
    for (size_t b : counts)
      for (size_t c : counts) generic_case<A, S>(a, b, c);
}

template <size_t A>
static void generic_align() {
  CHECK(WsLayout<A>().bytes() == 0, "empty layout of alignment %zu", A);
  generic_sweep<A, 1>();
  generic_sweep<A, 2>();
  generic_sweep<A, 4>();
  generic_sweep<A, 8>();
  generic_sweep<A, 16>();
}

// ---- the closed forms, as plain integers
static size_t al(size_t b) { return (b + 255) / 256 * 256; }

static void filter_site(size_t nq, size_t N, size_t QT, size_t k, size_t cap) {
  const size_t o_invq = 0, o_invd = o_invq + al(nq * 4), o_stats = o_invd + al(N * 4), o_aidx = o_stats + 256, o_aval = o_aidx + al(QT * k * 8),
               o_cidx = o_aval + al(QT * k * 4), o_cval = o_cidx + al(QT * cap * 8), o_cnt = o_cval + al(QT * cap * 4), o_end = o_cnt + al(QT * 4);
  const FilterListsLayout f = filter_lists_layout(nq, N, QT, k, cap);
  CHECK(f.invq.off == o_invq && f.invdb.off == o_invd && f.stats.off == o_stats && f.aidx.off == o_aidx && f.aval.off == o_aval &&
            f.cidx.off == o_cidx && f.cval.off == o_cval && f.cnt.off == o_cnt && f.bytes == o_end,
        "filtered top-k lists nq=%zu N=%zu QT=%zu k=%zu cap=%zu", nq, N, QT, k, cap);
}

static void knn_site(size_t N, size_t QT, size_t k, size_t cap) {
  const size_t hy_b = al(N * 4), ai_b = al(QT * k * 8), av_b = al(QT * k * 4), c_b = al(QT * cap * 8), n_b = al(QT * 4), k_b = al(QT * cap * 8);
  const KnnF32Layout f = knn_f32_layout(N, QT, k, cap);
  CHECK(f.hy.off == 0 && f.aidx.off == hy_b && f.aval.off == hy_b + ai_b && f.cand.off == hy_b + ai_b + av_b &&
            f.count.off == hy_b + ai_b + av_b + c_b && f.key.off == hy_b + ai_b + av_b + c_b + n_b &&
            f.ovf.off == hy_b + ai_b + av_b + c_b + n_b + k_b && f.bytes == hy_b + ai_b + av_b + c_b + n_b + k_b + 256,
        "f32 kNN lists N=%zu QT=%zu k=%zu cap=%zu", N, QT, k, cap);
}

static void kmeanspp_site(size_t total, size_t D, size_t n_clusters, size_t trials) {
  const size_t nblk = (total + 4095) / 4096;
  const size_t mind_b = al(total * 4), dist_b = al(trials * total * 4), cand_b = al(trials * D * 4), bs_b = al(nblk * 8),
               uni_b = al((n_clusters > 1 ? n_clusters - 1 : 1) * trials * 8), idx_b = al(n_clusters * 8), small_b = 512;
  const KmeansppLayout f = kmeanspp_layout(total, nblk, D, n_clusters, trials);
  CHECK(f.mind.off == 0 && f.dist.off == mind_b && f.cand.off == mind_b + dist_b && f.block_sums.off == mind_b + dist_b + cand_b &&
            f.uniform.off == mind_b + dist_b + cand_b + bs_b && f.indices.off == mind_b + dist_b + cand_b + bs_b + uni_b &&
            f.small.off == mind_b + dist_b + cand_b + bs_b + uni_b + idx_b &&
            f.bytes == mind_b + dist_b + cand_b + bs_b + uni_b + idx_b + small_b,
        "k-means++ block total=%zu D=%zu n_clusters=%zu trials=%zu", total, D, n_clusters, trials);
}

// The closed form left the last piece (72 bytes per candidate) unrounded, so its total is a multiple of 16 only for an even n_cand; the
// layout rounds every piece.  Offsets are equal always, totals are equal for even n_cand and 8 bytes apart for odd n_cand.
static void sift_site(size_t nc) {
  const size_t max_peaks = 18;
  const size_t cand_b = nc * 16, kp_b = nc * 32, int_b = ((nc + 1) * 4 + 15) & ~(size_t)15, bins_b = nc * max_peaks * 4;
  const auto f = sift_cand_layout<Elem<16>, Elem<32>>(nc, max_peaks);
  CHECK(f.cand.off == 0 && f.kp.off == cand_b && f.npeaks.off == cand_b + kp_b && f.nkeep.off == cand_b + kp_b + int_b &&
            f.row_off.off == cand_b + kp_b + 2 * int_b && f.bins.off == cand_b + kp_b + 3 * int_b,
        "SIFT candidate block offsets n_cand=%zu", nc);
  const size_t closed = cand_b + kp_b + 3 * int_b + bins_b;
  CHECK(f.bytes == closed + (nc % 2 ? 8 : 0), "SIFT candidate block n_cand=%zu: %zu bytes against %zu", nc, f.bytes, closed);
}

// the index-maintenance blocks (update.hip): scan partials, and the stored-order mask and positions in front of them
static void update_sites(size_t n, size_t tile) {
  const size_t ntiles = (n + tile - 1) / tile;
  const UpdateScanLayout u = update_scan_layout(ntiles, tile);
  CHECK(u.tile.off == 0 && u.block.off == al(ntiles * 8) && u.top.off == al(ntiles * 8) + al(tile * 8) &&
            u.bytes == al(ntiles * 8) + al(tile * 8) + 256,
        "scan partials n=%zu tile=%zu", n, tile);
  const IvfRemoveLayout r = ivf_remove_layout(n, ntiles, tile);
  const size_t o_pos = al(n), o_tile = o_pos + al((n + 1) * 8), o_block = o_tile + al(ntiles * 8), o_top = o_block + al(tile * 8);
  CHECK(r.keep.off == 0 && r.pos.off == o_pos && r.tile.off == o_tile && r.block.off == o_block && r.top.off == o_top && r.bytes == o_top + 256,
        "list-remove block n=%zu tile=%zu", n, tile);
  CHECK(update_stage_bytes(n, 3) == al(n * 3), "staging block of %zu rows", n);
}

// the partial lists of the top-m assignment (assign_topm.hip): indices, then values, [row][split][m] each
static void topm_site(size_t total, size_t splits, size_t m) {
  const TopmPartialLayout t = topm_partial_layout(total, splits, m);
  const size_t piece = al(total * splits * m * 4);
  CHECK(t.idx.off == 0 && t.val.off == piece && t.bytes == 2 * piece, "top-m partial lists total=%zu splits=%zu m=%zu", total, splits, m);
}

// the ASMK maintenance blocks (asmk_update.hip): the sort's two item arrays, digit counts and scan partials; the survivor flags
static void asmk_update_sites(size_t total, size_t ntiles) {
  const size_t ncounts = 257 * ntiles, nscan = (ncounts + 2047) / 2048;
  const AsmkInvertLayout a = asmk_invert_layout(total, ncounts, nscan);
  CHECK(a.items_a.off == 0 && a.items_b.off == al(total * 8) && a.counts.off == 2 * al(total * 8) &&
            a.partials.off == 2 * al(total * 8) + al(ncounts * 4) && a.bytes == 2 * al(total * 8) + al(ncounts * 4) + al(nscan * 4),
        "ASMK inversion block total=%zu ntiles=%zu", total, ntiles);
  const AsmkRemoveLayout r = asmk_remove_layout(total, (total + 1 + 2047) / 2048);
  CHECK(r.spos.off == 0 && r.partials.off == al((total + 1) * 4) && r.bytes == al((total + 1) * 4) + al((total + 1 + 2047) / 2048 * 4),
        "ASMK remove block entries=%zu", total);
}

// the block of the ASMK query expansion (asmk_expand.hip): hit masks of every word, then chunk counts and chunk weight sums
static void asmk_expand_site(size_t queries, size_t nchunks) {
  const AsmkExpandLayout e = asmk_expand_layout(queries, nchunks);
  const size_t mask_b = al(queries * nchunks * 64 * 4), small_b = al(queries * nchunks * 4);
  CHECK(e.mask.off == 0 && e.cnt.off == mask_b && e.wsum.off == mask_b + small_b && e.bytes == mask_b + 2 * small_b,
        "ASMK expansion block queries=%zu chunks=%zu", queries, nchunks);
}

// the grouping block of the probed int8 scan by list (ivf_sq8.hip): tile prefix, base, total, goff, gq, gbase, then the sort's arrays
static void ivf_sq8_group_site(size_t queries, size_t nprobe, size_t nlist) {
  const size_t pairs = queries * nprobe, ntiles = (pairs + 4095) / 4096, ncounts = 257 * ntiles, nscan = (ncounts + 2047) / 2048;
  const IvfSq8GroupLayout g = ivf_sq8_group_layout(queries, pairs, nlist, ncounts, nscan);
  const size_t off_b = al((nlist + 1) * 4), pair_b = al(pairs * 4), item_b = al(pairs * 8);
  CHECK(g.tile_off.off == 0 && g.base.off == off_b && g.total.off == off_b + pair_b && g.goff.off == off_b + pair_b + al(queries * 4) &&
            g.gq.off == 2 * off_b + pair_b + al(queries * 4) && g.gbase.off == g.gq.off + pair_b && g.items_a.off == g.gbase.off + pair_b &&
            g.items_b.off == g.items_a.off + item_b && g.counts.off == g.items_b.off + item_b && g.partials.off == g.counts.off + al(ncounts * 4) &&
            g.bytes == g.partials.off + al(nscan * 4),
        "IVF int8 grouping block queries=%zu nprobe=%zu nlist=%zu", queries, nprobe, nlist);
}

int main() {
  generic_align<256>();
  generic_align<16>();
  generic_align<8>();

  const size_t ks[] = {1, 5, 128}, caps[] = {64, 260, 2048}, rows[] = {1, 63, 64, 65, 8192}, Ns[] = {1, 255, 32768, 100001};
  for (size_t k : ks)
    for (size_t cap : caps)
      for (size_t QT : rows)
        for (size_t N : Ns) {
          knn_site(N, QT, k, cap);
          for (size_t nq : rows) filter_site(nq, N, QT, k, cap);
        }
  const size_t dims[] = {1, 63, 128}, clusters[] = {1, 2, 5, 128, 2048}, trials[] = {1, 5, 8};
  for (size_t total : Ns)
    for (size_t total2 : rows)
      for (size_t D : dims)
        for (size_t c : clusters)
          for (size_t t : trials) {
            kmeanspp_site(total, D, c, t);
            kmeanspp_site(total2, D, c, t);
          }
  for (size_t N : Ns) update_sites(N, 2048);
  for (size_t N : rows) update_sites(N, 64);
  for (size_t N : Ns) asmk_update_sites(N, (N + 255) / 256);
  for (size_t N : rows) asmk_update_sites(N, (N + 4095) / 4096);
  for (size_t nq : {(size_t)1, (size_t)3, (size_t)128})
    for (size_t nchunks : {(size_t)1, (size_t)5, (size_t)1024}) asmk_expand_site(nq, nchunks);
  for (size_t nq : rows)
    for (size_t nprobe : {(size_t)1, (size_t)7, (size_t)1024})
      for (size_t nlist : {(size_t)1, (size_t)1024, (size_t)65536})
        if (nprobe <= nlist) ivf_sq8_group_site(nq, nprobe, nlist);
  for (size_t nc : rows) sift_site(nc);
  for (size_t nc : Ns) sift_site(nc);
  const size_t splits[] = {2, 3, 64, 256}, ms[] = {1, 5, 8};
  for (size_t total : Ns)
    for (size_t sp : splits)
      for (size_t m : ms) topm_site(total, sp, m);

  if (g_fail) {
    fprintf(stderr, "ws_layout_check: %d checks failed\n", g_fail);
    return 1;
  }
  printf("ws_layout_check: ok\n");
  return 0;
}
