// Host-only check of list_common.hpp (tests/test_update_host.py builds it with -fsanitize=address,undefined and runs it): the
// overlap tests, the two offset predicates, and the three launch-shape rules held against the expressions their entry points carried
// inline before the header took them, over a grid of inputs, with the invariants the kernels rely on.  Exit status 0 = every check held.
#include <cstdio>

#include "../list_common.hpp"

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

static void overlap_cases() {
  char buf[64];
  CHECK(!ranges_overlap(buf, 8, buf + 8, 8), "adjacent ranges");
  CHECK(!ranges_overlap(buf + 8, 8, buf, 8), "adjacent ranges, swapped");
  CHECK(ranges_overlap(buf, 9, buf + 8, 8), "one byte shared");
  CHECK(ranges_overlap(buf + 8, 8, buf, 9), "one byte shared, swapped");
  CHECK(ranges_overlap(buf, 64, buf + 20, 1) && ranges_overlap(buf + 20, 1, buf, 64), "a range inside another");
  CHECK(ranges_overlap(buf, 8, buf, 8), "the same range");
  CHECK(!ranges_overlap(nullptr, 8, buf, 8) && !ranges_overlap(buf, 8, nullptr, 8) && !ranges_overlap(nullptr, 8, nullptr, 8), "a null pointer");
  CHECK(!ranges_overlap(buf, 0, buf, 8) && !ranges_overlap(buf, 8, buf + 4, 0) && !ranges_overlap(buf, -1, buf, 8), "an empty range");

  const ByteRange ins[] = {{buf, 16}, {nullptr, 16}, {buf + 16, 0}};
  const ByteRange apart[] = {{buf + 16, 16}, {buf + 32, 16}, {buf + 48, 16}};
  CHECK(outputs_overlap(apart, 3, ins, 3) == 0, "disjoint outputs and inputs");
  const ByteRange on_input[] = {{buf + 16, 16}, {buf + 32, 16}, {buf + 15, 1}};
  CHECK(outputs_overlap(on_input, 3, ins, 3) == 1, "the last output on the first input");
  const ByteRange twice[] = {{buf + 16, 16}, {buf + 32, 16}, {buf + 47, 16}};
  CHECK(outputs_overlap(twice, 3, ins, 3) == 2, "outputs 1 and 2 share a byte");
  const ByteRange first_last[] = {{buf + 16, 16}, {buf + 40, 8}, {buf + 31, 2}};
  CHECK(outputs_overlap(first_last, 3, ins, 3) == 2, "outputs 0 and 2 share a byte");
  const ByteRange both[] = {{buf, 1}, {buf + 32, 16}, {buf + 32, 16}};
  CHECK(outputs_overlap(both, 3, ins, 3) == 1, "an input overlap is reported before an output overlap");
  CHECK(outputs_overlap(apart, 0, ins, 3) == 0 && outputs_overlap(apart, 3, ins, 0) == 0, "no outputs, no inputs");
}

static void offset_cases() {
  const int64_t good[] = {0, 0, 3, 3, 7}, one[] = {0}, nonzero[] = {1, 2, 3}, last_step[] = {0, 2, 5, 4}, middle[] = {0, 5, 4, 9};
  CHECK(offsets_first_break(good, 4) == -1, "good offsets");
  CHECK(offsets_first_break(one, 0) == -1, "offsets of no list");
  CHECK(offsets_first_break(nonzero, 2) == 0, "first element non-zero");
  CHECK(offsets_first_break(last_step, 3) == 3, "a decrease at the last step");
  CHECK(offsets_first_break(last_step, 2) == -1, "the decrease lies beyond count");
  CHECK(offsets_first_break(middle, 3) == 2, "a decrease in the middle");

  const int64_t q_good[] = {4, 4, 9, 12}, q_neg[] = {-1, 0, 3}, q_neg_later[] = {0, -2, 3}, q_last[] = {0, 6, 5};
  CHECK(query_offsets_first_break(q_good, 3) == -1, "query offsets need not start at 0");
  CHECK(query_offsets_first_break(q_good, 0) == -1, "no query");
  CHECK(query_offsets_first_break(q_neg, 2) == 0, "a negative query offset");
  CHECK(query_offsets_first_break(q_neg_later, 2) == 0, "a decrease into a negative offset is query 0's");
  CHECK(query_offsets_first_break(q_last, 2) == 1, "a decrease at the last step");
}

static void shape_cases() {
  for (int bits = -32; bits <= 160; ++bits) CHECK(sig_bits_ok(bits) == (bits == 32 || bits == 64 || bits == 96 || bits == 128), "bits %d", bits);
  CHECK(sig_align(1) == 4 && sig_align(2) == 8 && sig_align(3) == 4 && sig_align(4) == 16, "signature alignment");
  CHECK(!word_count_ok(0) && word_count_ok(1) && word_count_ok(65536) && !word_count_ok(65537) && !word_count_ok(-1), "K range");
}

// ---- the rules as pvs_asmk_score_dev, pvs_asmk_expand_dev and pvs_asmk_invert_dev carried them inline
static int64_t inline_score_slice(int num_cu, int64_t qn, int64_t N, int slice_images) {
  int64_t S = slice_images;
  if (S == 0) {
    const int64_t want = (2 * (int64_t)num_cu + qn - 1) / qn;
    const int64_t G0 = std::max<int64_t>(1, std::min<int64_t>(want, N / 1024));
    S = std::min<int64_t>(32768, ((N + G0 - 1) / G0 + 63) / 64 * 64);
  }
  return S;
}

static int inline_tile_chunks(int num_cu, int nchunks, int64_t qn, int tile_words) {
  int tile_chunks = tile_words / 64;
  if (tile_chunks == 0) {
    const int64_t want = (int64_t)num_cu * 8;
    tile_chunks = (int)std::min<int64_t>(4096 / 64, std::max<int64_t>(4, ((int64_t)nchunks * qn + want - 1) / want));
  }
  return tile_chunks;
}

static int64_t inline_invert_tile(int tile_entries, int64_t total) {
  int64_t tile = tile_entries == 0 ? 4096 : std::min<int64_t>(std::max<int64_t>((tile_entries + 255) / 256 * 256, 256), 65536);
  const int64_t need = ((total + 65536 - 1) / 65536 + 255) / 256 * 256;
  tile = std::max(tile, need);
  return tile;
}

static void launch_shape_cases() {
  const int64_t last = ((int64_t)1 << 31) - 1;
  const int num_cus[] = {1, 256};
  const int64_t qns[] = {1, 127, 128};
  const int64_t Ns[] = {1, 63, 64, 1023, 1024, 1025, (int64_t)32768 * 300, last};
  const int slices[] = {0, 64, 1024, 32768};
  const int nchunks_all[] = {1, 4, 5, 1024};
  const int tile_words_all[] = {0, 64, 256, 4096};
  const int64_t totals[] = {1, 256, 257, (int64_t)65536 * 256 + 1, last};
  const int tile_entries_all[] = {0, 1, 256, 257, 65536, 70000};
  for (int num_cu : num_cus)
    for (int64_t qn : qns) {
      for (int64_t N : Ns)
        for (int slice : slices) {
          const int64_t S = score_slice(num_cu, qn, N, slice);
          CHECK(S == inline_score_slice(num_cu, qn, N, slice), "score_slice(%d, %lld, %lld, %d) = %lld", num_cu, (long long)qn, (long long)N,
                slice, (long long)S);
          CHECK(S % 64 == 0 && S >= 64 && S <= 32768, "slice %lld", (long long)S);
          CHECK((N + S - 1) / S * S >= N, "slices of %lld do not cover %lld", (long long)S, (long long)N);
          if (slice != 0) CHECK(S == slice, "a given slice is kept");
        }
      for (int nchunks : nchunks_all)
        for (int tile_words : tile_words_all) {
          const int tc = expand_tile_chunks(num_cu, nchunks, qn, tile_words);
          CHECK(tc == inline_tile_chunks(num_cu, nchunks, qn, tile_words), "expand_tile_chunks(%d, %d, %lld, %d) = %d", num_cu, nchunks,
                (long long)qn, tile_words, tc);
          if (tile_words == 0) CHECK(tc >= 4 && tc <= 64, "tile_chunks %d", tc);
          else CHECK(tc == tile_words / 64, "a given tile is kept");
        }
    }
  for (int64_t total : totals)
    for (int tile_entries : tile_entries_all) {
      const int64_t tile = invert_tile(tile_entries, total);
      CHECK(tile == inline_invert_tile(tile_entries, total), "invert_tile(%d, %lld) = %lld", tile_entries, (long long)total, (long long)tile);
      CHECK(tile % 256 == 0 && tile >= 256, "tile %lld", (long long)tile);
      CHECK((total + tile - 1) / tile <= 65536, "%lld tiles", (long long)((total + tile - 1) / tile));
    }
  CHECK(flat_grid(256, 0) == 1 && flat_grid(256, 1) == 1 && flat_grid(256, 256) == 1 && flat_grid(256, 257) == 2, "small flat grids");
  CHECK(flat_grid(256, last) == 2048 && flat_grid(1, last) == 8, "a flat grid holds at most eight workgroups per compute unit");
  CHECK(flat_grid(256, 1025, 1024) == 2 && flat_grid(256, 1024, 1024) == 1, "a flat grid over blocks of 1024");
}

int main() {
  overlap_cases();
  offset_cases();
  shape_cases();
  launch_shape_cases();
  if (g_fail) fprintf(stderr, "%d checks failed\n", g_fail);
  else printf("list_common: all checks held\n");
  return g_fail ? 1 : 0;
}
