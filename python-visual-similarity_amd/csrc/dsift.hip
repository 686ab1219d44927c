// Dense SIFT: SIFT descriptors on a regular grid at fixed bin sizes, from pixels to 128-byte rows, one
// workgroup per (image, bin size, tile of the descriptor grid).  Nothing between the pixels and the finished rows touches HBM:
//
//   stage 1  gray tile + halo (replicated borders)                    -> LDS  G  [Hr][Wr]
//   stage 2  horizontal Gaussian                                      -> LDS  T  [Hr][Wg]
//   stage 3  vertical Gaussian                                        -> LDS  S  [Hg][Wg]   (over G)
//   stage 4  gradient: magnitude m and soft orientation t = 8 theta / 2 pi -> LDS  M, Th [Hp][Wp]
//            (m, t) IS the eight orientation planes: plane o at a pixel is m (1 - frac t), m frac t or 0, so the planes cost two
//            floats per pixel instead of eight and are expanded in registers by the next stage
//   stage 5  triangular convolution along x, only at the bin-centre columns, all eight planes per thread -> LDS Hb [8][ncx][Hp] (over G/S)
//   stage 6  triangular convolution along y, only at the bin-centre rows                                -> LDS Bn [ncy][ncx][8] (over T)
//   stage 7  normalise, clamp, renormalise, quantise: eight lanes per descriptor, one 16-byte store per lane
//
// Every sum runs in a fixed order (taps ascending, then a fixed butterfly over eight lanes) and no atomics are used, so a row's bits
// depend on the image, the bin size and the step only: not on the batch, the tile it fell into or the run.
#include <algorithm>

#include "sift_common.hpp"

namespace pvs {

constexpr int DS_THREADS = 256;
constexpr int DS_MAX_SIZES = 16;
constexpr int DS_MAX_RADIUS = 32;
constexpr int DS_MAX_TILE = 8;                 // descriptors per tile edge
constexpr size_t DS_LDS_TARGET = 64 * 1024;    // tiles grow while they stay under this (two workgroups per CU)
constexpr size_t DS_LDS_LIMIT = 160 * 1024;    // one workgroup per CU: the slow path of the large bin sizes

struct DsiftImage {
  int H, W;
  int64_t pix_off;    // first element of the image in the pixel buffer (elements of the pixel type)
  int64_t row_base;   // first output row of the image
};

struct DsiftArgs {
  const void* pixels;
  const DsiftImage* img;
  void* out;
  int pix_kind, out_kind, step, n_sizes, which, s, radius, tx, ty;
  float thr;
  int sizes[DS_MAX_SIZES];
  float taps[2 * DS_MAX_RADIUS + 1];
};

__host__ __device__ inline int ds_grid(int extent, int s, int step) {
  return extent >= 5 * s - 1 ? (extent - 5 * s + 1) / step + 1 : 0;
}

// LDS floats of a tile of tx x ty descriptors; the same arithmetic places the regions in the kernel
struct DsiftLayout {
  int Wp, Hp, Wg, Hg, Wr, Hr, WpS, HpS;
  int r1, r2, r3, tw;   // region offsets in floats
  int total;
};
__host__ __device__ inline DsiftLayout ds_layout(int s, int step, int radius, int tx, int ty) {
  DsiftLayout L;
  L.Wp = (tx - 1) * step + 5 * s - 1;
  L.Hp = (ty - 1) * step + 5 * s - 1;
  L.Wg = L.Wp + 2;
  L.Hg = L.Hp + 2;
  L.Wr = L.Wg + 2 * radius;
  L.Hr = L.Hg + 2 * radius;
  L.WpS = L.Wp | 1;   // odd strides: threads that walk down a column hit distinct banks
  L.HpS = L.Hp | 1;
  const int g1 = L.Hr * L.Wr, h1 = 8 * 4 * tx * L.HpS;   // gray (then S) | Hb
  const int g2 = L.Hr * L.Wg, h2 = 4 * ty * 4 * tx * 8;   // T | Bn
  const int n1 = g1 > h1 ? g1 : h1;
  const int n2 = g2 > h2 ? g2 : h2;
  const int n3 = 2 * L.Hp * L.WpS;
  L.r1 = 0;
  L.r2 = (n1 + 3) & ~3;
  L.r3 = L.r2 + ((n2 + 3) & ~3);
  L.tw = L.r3 + ((n3 + 3) & ~3);
  L.total = L.tw + ((2 * s - 1 + 3) & ~3);
  return L;
}

__global__ __launch_bounds__(DS_THREADS) void dsift_kernel(const DsiftArgs a, const int img0) {
  extern __shared__ float lds[];
  const DsiftImage im = a.img[img0 + blockIdx.y];
  const int s = a.s, step = a.step, R = a.radius;
  const int H = im.H, W = im.W;
  const int nx = ds_grid(W, s, step), ny = ds_grid(H, s, step);
  if (nx == 0 || ny == 0) return;
  const int tiles_x = (nx + a.tx - 1) / a.tx, tiles_y = (ny + a.ty - 1) / a.ty;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;
  const int ta = ((int)blockIdx.x % tiles_x) * a.tx, tb = ((int)blockIdx.x / tiles_x) * a.ty;   // first descriptor of the tile
  const int cntx = min(a.tx, nx - ta), cnty = min(a.ty, ny - tb);
  int64_t row0 = im.row_base;
  for (int k = 0; k < a.which; ++k) row0 += (int64_t)ds_grid(W, a.sizes[k], step) * ds_grid(H, a.sizes[k], step);

  // regions are placed for the full tile; an edge tile uses a corner of each
  const DsiftLayout LM = ds_layout(s, step, R, a.tx, a.ty);
  const DsiftLayout L = ds_layout(s, step, R, cntx, cnty);
  float* G = lds + LM.r1;     // gray, then S, then Hb
  float* T = lds + LM.r2;     // horizontal Gaussian, then Bn
  float* M = lds + LM.r3;     // magnitude
  float* Th = M + L.Hp * L.WpS;   // soft orientation index t in [0, 8]
  float* tw = lds + LM.tw;    // triangular weights w(d), d = -(s-1) .. s-1
  const int tid = threadIdx.x;
  const int px0 = ta * step, py0 = tb * step;   // image pixel of the plane region's corner: x0 - s + 1 with x0 = s - 1 + ta step
  const int ncx = 4 * cntx, ncy = 4 * cnty;

  for (int d = tid; d < 2 * s - 1; d += DS_THREADS) tw[d] = 1.0f - (float)abs(d - (s - 1)) / (float)s;

  // ---- stage 1: gray with replicated borders
  for (int idx = tid; idx < L.Hr * L.Wr; idx += DS_THREADS) {
    const int y = idx / L.Wr, x = idx - y * L.Wr;
    const int iy = min(max(py0 - 1 - R + y, 0), H - 1), ix = min(max(px0 - 1 - R + x, 0), W - 1);
    G[idx] = gray_at(a.pixels, a.pix_kind, im.pix_off, W, iy, ix);
  }
  __syncthreads();
  // ---- stage 2: T[y][x] = sum_k taps[k] G[y][x + k]
  for (int idx = tid; idx < L.Hr * L.Wg; idx += DS_THREADS) {
    const int y = idx / L.Wg, x = idx - y * L.Wg;
    const float* g = G + y * L.Wr + x;
    float acc = 0.f;
    for (int k = 0; k <= 2 * R; ++k) acc = fmaf(a.taps[k], g[k], acc);
    T[idx] = acc;
  }
  __syncthreads();
  // ---- stage 3: S[y][x] = sum_k taps[k] T[y + k][x]   (S overwrites G)
  float* S = G;
  for (int idx = tid; idx < L.Hg * L.Wg; idx += DS_THREADS) {
    const int y = idx / L.Wg, x = idx - y * L.Wg;
    const float* t = T + y * L.Wg + x;
    float acc = 0.f;
    for (int k = 0; k <= 2 * R; ++k) acc = fmaf(a.taps[k], t[k * L.Wg], acc);
    S[idx] = acc;
  }
  __syncthreads();
  // ---- stage 4: gradient of S at the plane region (S has a one-pixel ring around it)
  for (int idx = tid; idx < L.Hp * L.Wp; idx += DS_THREADS) {
    const int y = idx / L.Wp, x = idx - y * L.Wp;
    const int ix = px0 + x, iy = py0 + y;
    const float* c = S + (y + 1) * L.Wg + (x + 1);
    float gx, gy;
    if (ix == 0) gx = c[1] - c[0];
    else if (ix == W - 1) gx = c[0] - c[-1];
    else gx = 0.5f * (c[1] - c[-1]);
    if (iy == 0) gy = c[L.Wg] - c[0];
    else if (iy == H - 1) gy = c[0] - c[-L.Wg];
    else gy = 0.5f * (c[L.Wg] - c[-L.Wg]);
    const float m = sqrtf(gx * gx + gy * gy);
    float th = atan2f(gy, gx);
    if (th < 0.f) th += 6.283185307179586f;
    M[y * L.WpS + x] = m;
    Th[y * L.WpS + x] = th * 1.2732395447351628f;   // 8 / 2 pi
  }
  __syncthreads();
  // ---- stage 5: Hb[o][cx][y] = sum_d w(d) plane_o[y][xc + d]; consecutive threads take consecutive y
  float* Hb = G;
  for (int idx = tid; idx < L.Hp * ncx; idx += DS_THREADS) {
    const int cx = idx / L.Hp, y = idx - cx * L.Hp;
    const int xl = (cx >> 2) * step + (cx & 3) * s;   // xc - (s - 1)
    const float* mp = M + y * L.WpS + xl;
    const float* tp = Th + y * L.WpS + xl;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int d = 0; d < 2 * s - 1; ++d) {
      const float m = mp[d], t = tp[d], w = tw[d];
      const int b = (int)t;                 // t >= 0: truncation is the floor
      const float f = t - (float)b;
      const float hi = m * f, lo = m * (1.0f - f);
      const int b0 = b & 7, b1 = (b + 1) & 7;
      const float wlo = w * lo, whi = w * hi;
#pragma unroll
      for (int o = 0; o < 8; ++o) acc[o] += (b0 == o) ? wlo : ((b1 == o) ? whi : 0.f);
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) Hb[(o * ncx + cx) * L.HpS + y] = acc[o];
  }
  __syncthreads();
  // ---- stage 6: Bn[cy][cx][o] = sum_d w(d) Hb[o][cx][yc + d]; consecutive threads take consecutive cx
  float* Bn = T;
  for (int idx = tid; idx < 8 * ncx * ncy; idx += DS_THREADS) {
    const int cx = idx % ncx, r = idx / ncx, o = r & 7, cy = r >> 3;
    const float* h = Hb + (o * ncx + cx) * L.HpS + (cy >> 2) * step + (cy & 3) * s;
    float acc = 0.f;
    for (int d = 0; d < 2 * s - 1; ++d) acc = fmaf(tw[d], h[d], acc);
    Bn[(cy * ncx + cx) * 8 + o] = acc;
  }
  __syncthreads();
  // ---- stage 7: eight lanes per descriptor, sixteen consecutive elements (two spatial cells x eight planes) per lane
  const int q = tid & 7;
  const int n_desc = cntx * cnty;
  for (int d0 = 0; d0 < n_desc; d0 += DS_THREADS / 8) {
    const int dsc = d0 + (tid >> 3);
    const bool live = dsc < n_desc;           // every lane takes part in the shuffles
    const int da = live ? dsc % cntx : 0, db = live ? dsc / cntx : 0;
    const int j = q >> 1, i0 = (q & 1) * 2;   // cells 2q and 2q + 1 = (j, i0) and (j, i0 + 1): sixteen consecutive floats of Bn
    const float* src = Bn + ((db * 4 + j) * ncx + da * 4 + i0) * 8;
    const int64_t row = row0 + (int64_t)(tb + db) * nx + (ta + da);
    sift_row_tail(src, a.thr, a.out_kind, a.out, row, q, live);
  }
}

static int ds_check_grid(int step, const int32_t* sizes, int n_sizes) {
  if (step < 1) PVS_FAIL(PVS_ERR_INVALID, "dense SIFT: step must be >= 1 (got %d)", step);
  if (!sizes || n_sizes < 1) PVS_FAIL(PVS_ERR_INVALID, "dense SIFT: at least one bin size is needed");
  if (n_sizes > DS_MAX_SIZES) PVS_FAIL(PVS_ERR_UNSUPPORTED, "dense SIFT: at most %d bin sizes (got %d)", DS_MAX_SIZES, n_sizes);
  for (int k = 0; k < n_sizes; ++k) {
    if (sizes[k] < 1) PVS_FAIL(PVS_ERR_INVALID, "dense SIFT: bin sizes must be >= 1 (got %d)", sizes[k]);
    if (sizes[k] > (1 << 24)) PVS_FAIL(PVS_ERR_INVALID, "dense SIFT: bin size %d is out of range", sizes[k]);   // 5 s stays an int
  }
  return PVS_OK;
}

static int ds_radius(int s) { return (4 * s + 5) / 6; }   // ceil(4 sigma), sigma = s / 6

// the largest tile (up to DS_MAX_TILE per edge, grown alternately) that stays under the LDS target; 1 x 1 may use the whole LDS
static int ds_pick_tile(int s, int step, int radius, int* tx, int* ty, size_t* bytes) {
  int bx = 1, by = 1;
  size_t b = (size_t)ds_layout(s, step, radius, 1, 1).total * 4;
  if (b > DS_LDS_LIMIT)
    PVS_FAIL(PVS_ERR_UNSUPPORTED, "dense SIFT: bin size %d needs %zu bytes of LDS per descriptor tile (limit %zu)", s, b, DS_LDS_LIMIT);
  for (bool grew = true; grew;) {
    grew = false;
    for (int axis = 0; axis < 2; ++axis) {
      const int cx = bx + (axis == 0), cy = by + (axis == 1);
      if (cx > DS_MAX_TILE || cy > DS_MAX_TILE) continue;
      // a tile with two descriptors along an axis spans more than `step` pixels: beyond this step it cannot fit the target, and
      // refusing it here keeps ds_layout's int arithmetic far from overflow for any step the entry point accepts
      if (step > 16384) continue;
      const size_t c = (size_t)ds_layout(s, step, radius, cx, cy).total * 4;
      if (c <= DS_LDS_TARGET) {
        bx = cx, by = cy, b = c;
        grew = true;
      }
    }
  }
  *tx = bx, *ty = by, *bytes = b;
  return PVS_OK;
}

}  // namespace pvs

using namespace pvs;

PVS_EXPORT int pvs_dsift_count(int H, int W, int step, const int32_t* sizes, int n_sizes, int64_t* count) {
  PVS_TRY(ds_check_grid(step, sizes, n_sizes));
  if (H < 0 || W < 0) PVS_FAIL(PVS_ERR_INVALID, "dense SIFT: negative image size");
  if (!count) PVS_FAIL(PVS_ERR_INVALID, "pvs_dsift_count: null count");
  int64_t n = 0;
  for (int k = 0; k < n_sizes; ++k) n += (int64_t)ds_grid(W, sizes[k], step) * ds_grid(H, sizes[k], step);
  *count = n;
  return PVS_OK;
}

PVS_EXPORT int pvs_dsift_frames(int H, int W, int step, const int32_t* sizes, int n_sizes, float* frames, int64_t capacity) {
  int64_t n = 0;
  PVS_TRY(pvs_dsift_count(H, W, step, sizes, n_sizes, &n));
  if (n > capacity) PVS_FAIL(PVS_ERR_INVALID, "pvs_dsift_frames: %lld frames do not fit %lld rows", (long long)n, (long long)capacity);
  if (n && !frames) PVS_FAIL(PVS_ERR_INVALID, "pvs_dsift_frames: null frames");
  float* f = frames;
  for (int k = 0; k < n_sizes; ++k) {
    const int s = sizes[k], nx = ds_grid(W, s, step), ny = ds_grid(H, s, step);
    for (int b = 0; b < ny; ++b)
      for (int a = 0; a < nx; ++a, f += 3) {
        f[0] = (float)(s - 1 + a * step) + 1.5f * (float)s;
        f[1] = (float)(s - 1 + b * step) + 1.5f * (float)s;
        f[2] = (float)s;
      }
  }
  return PVS_OK;
}

PVS_EXPORT int pvs_dsift_dev(pvs_ctx* ctx, const void* d_pixels, int pixel_kind, const int32_t* h_hw, const int64_t* h_pix_offsets,
                             int64_t n_images, int step, const int32_t* sizes, int n_sizes, double contrast_threshold, int out_kind,
                             void* d_out, int64_t out_rows, int64_t* d_row_offsets) {
  if (!ctx) PVS_FAIL(PVS_ERR_INVALID, "pvs_dsift_dev: null ctx");
  PVS_TRY(ds_check_grid(step, sizes, n_sizes));
  ImageIntake in{"dense SIFT", "pvs_dsift_dev", h_hw, h_pix_offsets};
  PVS_TRY(in.open(pixel_kind, out_kind, n_images));
  if (!(contrast_threshold >= 0.0)) PVS_FAIL(PVS_ERR_INVALID, "dense SIFT: contrast_threshold must be >= 0");
  if (n_images == 0) return PVS_OK;
  if (!d_row_offsets) PVS_FAIL(PVS_ERR_INVALID, "pvs_dsift_dev: null row offsets");
  PVS_HIP(hipSetDevice(ctx->device));

  // tiles first: an unsupported bin size fails before anything is queued
  int tx[DS_MAX_SIZES], ty[DS_MAX_SIZES];
  size_t lds_bytes[DS_MAX_SIZES];
  for (int k = 0; k < n_sizes; ++k) {
    if (ds_radius(sizes[k]) > DS_MAX_RADIUS) PVS_FAIL(PVS_ERR_UNSUPPORTED, "dense SIFT: bin size %d is not supported", sizes[k]);
    PVS_TRY(ds_pick_tile(sizes[k], step, ds_radius(sizes[k]), &tx[k], &ty[k], &lds_bytes[k]));
  }

  // per-image table and row offsets, built in a pinned block of a small ring (the call does not wait for the stream: a block is
  // reused only after the copies that read it have finished)
  const size_t meta_bytes = (size_t)n_images * sizeof(DsiftImage);
  const size_t off_bytes = (size_t)(n_images + 1) * sizeof(int64_t);
  const size_t need = meta_bytes + off_bytes;
  const int slot = ctx->dsift_next;
  ctx->dsift_next = (slot + 1) % pvs_ctx::DSIFT_RING;
  if (ctx->dsift_ev[slot]) PVS_HIP(hipEventSynchronize(ctx->dsift_ev[slot]));
  else PVS_HIP(hipEventCreateWithFlags(&ctx->dsift_ev[slot], hipEventDisableTiming));
  if (ctx->dsift_h_bytes[slot] < need) {
    if (ctx->dsift_h[slot]) (void)hipHostFree(ctx->dsift_h[slot]);
    ctx->dsift_h[slot] = nullptr;
    ctx->dsift_h_bytes[slot] = 0;
    const size_t want = std::max<size_t>(need + need / 4, 4096);
    PVS_HIP(hipHostMalloc(&ctx->dsift_h[slot], want, hipHostMallocDefault));
    ctx->dsift_h_bytes[slot] = want;
  }
  DsiftImage* h_meta = static_cast<DsiftImage*>(ctx->dsift_h[slot]);
  int64_t* h_off = reinterpret_cast<int64_t*>(static_cast<char*>(ctx->dsift_h[slot]) + meta_bytes);
  int64_t rows = 0;
  std::vector<int> max_tiles(n_sizes, 0);
  for (int64_t i = 0; i < n_images; ++i) {
    int H, W;
    int64_t po;
    PVS_TRY(in.next(i, &H, &W, &po));
    h_meta[i] = DsiftImage{H, W, po, rows};
    h_off[i] = rows;
    for (int k = 0; k < n_sizes; ++k) {
      const int nx = ds_grid(W, sizes[k], step), ny = ds_grid(H, sizes[k], step);
      rows += (int64_t)nx * ny;
      max_tiles[k] = std::max(max_tiles[k], ((nx + tx[k] - 1) / tx[k]) * ((ny + ty[k] - 1) / ty[k]));
    }
  }
  h_off[n_images] = rows;
  if (rows > out_rows) PVS_FAIL(PVS_ERR_INVALID, "dense SIFT: %lld rows do not fit the output of %lld rows", (long long)rows, (long long)out_rows);
  if (rows > 0 && (!d_pixels || !d_out)) PVS_FAIL(PVS_ERR_INVALID, "pvs_dsift_dev: null pixels or output");
  DsiftImage* d_meta = nullptr;
  PVS_TRY(ws_reserve(ctx, WS_DSIFT_TABLE, meta_bytes, &d_meta));
  PVS_HIP(hipMemcpyAsync(d_meta, h_meta, meta_bytes, hipMemcpyHostToDevice, ctx->stream));
  PVS_HIP(hipMemcpyAsync(d_row_offsets, h_off, off_bytes, hipMemcpyHostToDevice, ctx->stream));
  PVS_HIP(hipEventRecord(ctx->dsift_ev[slot], ctx->stream));
  if (rows == 0) return PVS_OK;

  ScopedTimer tm(ctx, T_MISC);
  for (int k = 0; k < n_sizes; ++k) {
    if (max_tiles[k] == 0) continue;
    DsiftArgs a;
    memset(&a, 0, sizeof(a));
    a.pixels = d_pixels;
    a.img = d_meta;
    a.out = d_out;
    a.pix_kind = pixel_kind;
    a.out_kind = out_kind;
    a.step = step;
    a.n_sizes = n_sizes;
    a.which = k;
    a.s = sizes[k];
    a.radius = ds_radius(sizes[k]);
    a.tx = tx[k];
    a.ty = ty[k];
    a.thr = (float)contrast_threshold;
    for (int j = 0; j < n_sizes; ++j) a.sizes[j] = sizes[j];
    gaussian_taps((double)a.s / 6.0, a.radius, a.taps);   // sigma = s / 6
    PVS_TRY(ensure_lds(ctx, reinterpret_cast<const void*>(dsift_kernel), lds_bytes[k]));
    for (int64_t i0 = 0; i0 < n_images; i0 += 65535) {
      const dim3 grid((unsigned)max_tiles[k], (unsigned)std::min<int64_t>(65535, n_images - i0));
      hipLaunchKernelGGL(dsift_kernel, grid, dim3(DS_THREADS), lds_bytes[k], ctx->stream, a, (int)i0);
      PVS_HIP(hipGetLastError());
    }
  }
  return PVS_OK;
}
