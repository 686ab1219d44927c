// Keypoint SIFT: Gaussian pyramid, DoG extrema, sub-pixel refinement, contrast and edge tests, orientation
// assignment and rotated 4 x 4 x 8 descriptors, from pixels to 128-byte rows, for a batch of images of mixed sizes.
//
//   sift_base     gray (+ 2x bilinear enlargement)                                   -> layer 1 of octave 0 (scratch)
//   sift_blur     separable Gaussian of one layer through an LDS tile (32 x 32 + halo) -> the next layer (HBM)
//   sift_down     every second pixel of layer L                                      -> layer 0 of the next octave
//   sift_detect   DoG (computed from the Gaussian layers, never stored) + pre-threshold + strict 3 x 3 x 3 extremum;
//                 run twice: per-block counts, exclusive scan, then the candidates written in (image, octave, layer, y, x) order
//   sift_refine   one thread per candidate: quadratic refinement, contrast and edge tests
//   sift_orient   one wave per candidate: 36-bin histogram (lane-private columns in LDS, summed over the lanes in a fixed order)
//   sift_rank     nfeatures > 0 only: rows kept per candidate among the strongest of its image
//   sift_desc     one wave per candidate, one pass per kept orientation: 128 lane-private columns in LDS, the eight-lane tail
//
// The row count is data dependent; everything variable is compacted by counts + exclusive scans, and every sum runs in an order
// fixed by the keypoint alone.  No atomics: a row's bits and its place among its image's rows depend on the image and the
// parameters only, not on the batch, the chunking or the run.
#include <algorithm>

#include "sift_common.hpp"

namespace pvs {

constexpr int SF_MAX_RADIUS = 32;
constexpr int SF_MAX_LAYERS = 8;                 // n_octave_layers
constexpr int SF_MAX_OCT = 24;
constexpr int SF_TILE = 32;                      // blur tile edge
constexpr int SF_BORDER = 5;
constexpr int SF_MIN_OCTAVE = 16;
constexpr int SF_MAX_PEAKS = 18;                 // local maxima of 36 circular bins
constexpr int SF_CHUNK_IMAGES = 1024;
constexpr size_t SF_PYRAMID_BUDGET = 256u << 20; // bytes of Gaussian pyramids per chunk (a single larger image runs alone)
constexpr int SF_HSTRIDE = 65;                   // lane-private histogram columns: bin * 65 + lane (conflict-free both ways)

struct SiftImage {
  int H, W;          // input
  int H0, W0;        // octave 0
  int n_oct, pad;
  int64_t pix_off;   // first element of the image in the pixel buffer
  int64_t ws_off;    // first float of the image's pyramid in the workspace
};

struct SiftKp {
  int alive, i, y, x;          // final integer position of the refinement
  float Xx, Xy, Xs, contr;
};

__host__ __device__ inline int sf_octaves(int h0, int w0) {
  const int m = h0 < w0 ? h0 : w0;
  int n = 0;
  while (n < SF_MAX_OCT && (m >> n) >= SF_MIN_OCTAVE) ++n;
  return n;
}
// floats in front of octave o of an image's pyramid (nl layers per octave)
__host__ __device__ inline int64_t sf_oct_off(int h0, int w0, int o, int nl) {
  int64_t off = 0;
  for (int k = 0; k < o; ++k) off += (int64_t)nl * (h0 >> k) * (w0 >> k);
  return off;
}

struct SiftArgs {
  const void* pixels;
  const SiftImage* img;     // the chunk's table
  float* pyr;
  int pix_kind, upsample, L, nl;
  float pre, thr_c, edge_r, edge_r1sq, sigma;
};

__device__ inline float* sf_layer(const SiftArgs& a, const SiftImage& im, int o, int layer) {
  const int h = im.H0 >> o, w = im.W0 >> o;
  return a.pyr + im.ws_off + sf_oct_off(im.H0, im.W0, o, a.nl) + (int64_t)layer * h * w;
}

// ---- gray (+ enlargement) into layer 1 of octave 0
__global__ __launch_bounds__(256) void sift_base_kernel(const SiftArgs a) {
  const SiftImage im = a.img[blockIdx.y];
  if (im.n_oct == 0) return;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)im.H0 * im.W0) return;
  const int y = (int)(idx / im.W0), x = (int)(idx - (int64_t)y * im.W0);
  const auto gray = [&](int py, int px) { return gray_at(a.pixels, a.pix_kind, im.pix_off, im.W, py, px); };
  float v;
  if (a.upsample) {
    const float sy = fminf(fmaxf((float)y * 0.5f - 0.25f, 0.f), (float)(im.H - 1));
    const float sx = fminf(fmaxf((float)x * 0.5f - 0.25f, 0.f), (float)(im.W - 1));
    const int y0 = (int)floorf(sy), x0 = (int)floorf(sx);
    const int y1 = min(y0 + 1, im.H - 1), x1 = min(x0 + 1, im.W - 1);
    const float fy = sy - (float)y0, fx = sx - (float)x0;
    const float top = (1.0f - fx) * gray(y0, x0) + fx * gray(y0, x1);
    const float bot = (1.0f - fx) * gray(y1, x0) + fx * gray(y1, x1);
    v = (1.0f - fy) * top + fy * bot;
  } else {
    v = gray(y, x);
  }
  sf_layer(a, im, 0, 1)[idx] = v;
}

// ---- separable Gaussian: layer `src` -> layer `dst` of octave o, replicated borders, taps ascending
struct SiftBlurArgs {
  int o, src, dst, R;
  float taps[2 * SF_MAX_RADIUS + 1];
};
__global__ __launch_bounds__(256) void sift_blur_kernel(const SiftArgs a, const SiftBlurArgs b) {
  extern __shared__ float lds[];
  const SiftImage im = a.img[blockIdx.y];
  if (b.o >= im.n_oct) return;
  const int h = im.H0 >> b.o, w = im.W0 >> b.o;
  const int tiles_x = (w + SF_TILE - 1) / SF_TILE, tiles_y = (h + SF_TILE - 1) / SF_TILE;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;
  const int tx0 = ((int)blockIdx.x % tiles_x) * SF_TILE, ty0 = ((int)blockIdx.x / tiles_x) * SF_TILE;
  const int R = b.R, Wr = SF_TILE + 2 * R;
  float* G = lds;                 // [Wr][Wr]
  float* T = lds + Wr * Wr;       // [Wr][SF_TILE]
  const float* s = sf_layer(a, im, b.o, b.src);
  float* d = sf_layer(a, im, b.o, b.dst);
  const int tid = threadIdx.x;
  for (int idx = tid; idx < Wr * Wr; idx += 256) {
    const int y = idx / Wr, x = idx - y * Wr;
    const int iy = min(max(ty0 - R + y, 0), h - 1), ix = min(max(tx0 - R + x, 0), w - 1);
    G[idx] = s[(int64_t)iy * w + ix];
  }
  __syncthreads();
  for (int idx = tid; idx < Wr * SF_TILE; idx += 256) {
    const int y = idx / SF_TILE, x = idx - y * SF_TILE;
    const float* g = G + y * Wr + x;
    float acc = 0.f;
    for (int k = 0; k <= 2 * R; ++k) acc = fmaf(b.taps[k], g[k], acc);
    T[idx] = acc;
  }
  __syncthreads();
  for (int idx = tid; idx < SF_TILE * SF_TILE; idx += 256) {
    const int y = idx / SF_TILE, x = idx - y * SF_TILE;
    if (ty0 + y >= h || tx0 + x >= w) continue;
    const float* t = T + y * SF_TILE + x;
    float acc = 0.f;
    for (int k = 0; k <= 2 * R; ++k) acc = fmaf(b.taps[k], t[k * SF_TILE], acc);
    d[(int64_t)(ty0 + y) * w + tx0 + x] = acc;
  }
}

// ---- layer 0 of octave o = every second pixel of layer L of octave o - 1
__global__ __launch_bounds__(256) void sift_down_kernel(const SiftArgs a, const int o) {
  const SiftImage im = a.img[blockIdx.y];
  if (o >= im.n_oct) return;
  const int h = im.H0 >> o, w = im.W0 >> o, wp = im.W0 >> (o - 1);
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)h * w) return;
  const int y = (int)(idx / w), x = (int)(idx - (int64_t)y * w);
  sf_layer(a, im, o, 0)[idx] = sf_layer(a, im, o - 1, a.L)[(int64_t)(2 * y) * wp + 2 * x];
}

// ---- DoG extrema.  Block b of (image, octave, layer) covers 256 consecutive pixels of the octave in raster order; the count (or,
// with WRITE, the scanned offset) of block b sits at img * stride + base + (layer - 1) * gridDim.x + b, which is the defined order.
struct SiftDetectArgs {
  int o, base, stride;
  int* counts;           // per-block counts (pass 1) / exclusive offsets (pass 2)
  int4* cand;            // (image in chunk, octave | layer << 8, y, x)
};
template <bool WRITE>
__global__ __launch_bounds__(256) void sift_detect_kernel(const SiftArgs a, const SiftDetectArgs d) {
  __shared__ int wave_n[4];
  const SiftImage im = a.img[blockIdx.y];
  const int i = (int)blockIdx.z + 1;
  const int slot = (int)blockIdx.y * d.stride + d.base + (i - 1) * (int)gridDim.x + (int)blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  bool hit = false;
  int y = 0, x = 0;
  if (d.o < im.n_oct) {
    const int h = im.H0 >> d.o, w = im.W0 >> d.o;
    const int64_t idx = (int64_t)blockIdx.x * 256 + tid;
    if (idx < (int64_t)h * w) {
      y = (int)(idx / w), x = (int)(idx - (int64_t)y * w);
      if (y >= SF_BORDER && y < h - SF_BORDER && x >= SF_BORDER && x < w - SF_BORDER) {
        const int64_t plane = (int64_t)h * w;
        const float* g = sf_layer(a, im, d.o, 0) + (int64_t)y * w + x;
        const float v = g[(i + 1) * plane] - g[i * plane];
        if (fabsf(v) > a.pre) {
          bool is_max = v > 0.f, is_min = v < 0.f;
          for (int di = -1; di <= 1 && (is_max || is_min); ++di)
            for (int dy = -1; dy <= 1; ++dy)
              for (int dx = -1; dx <= 1; ++dx) {
                if (di == 0 && dy == 0 && dx == 0) continue;
                const float* q = g + (i + di) * plane + dy * w + dx;
                const float n = q[plane] - q[0];
                is_max = is_max && v > n;
                is_min = is_min && v < n;
              }
          hit = is_max || is_min;
        }
      }
    }
  }
  const unsigned long long m = __ballot(hit);
  if (lane == 0) wave_n[wv] = __popcll(m);
  __syncthreads();
  if (!WRITE) {
    if (tid == 0) d.counts[slot] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
  } else if (hit) {
    int pos = d.counts[slot] + __popcll(m & ((1ull << lane) - 1ull));
    for (int k = 0; k < wv; ++k) pos += wave_n[k];
    d.cand[pos] = make_int4((int)blockIdx.y, d.o | (i << 8), y, x);
  }
}

// ---- exclusive scan of n ints by one workgroup; out[n] = total
__global__ __launch_bounds__(1024) void sift_scan_kernel(const int* in, int* out, const int n) {
  __shared__ int wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int carry = 0;
  for (int base = 0; base < n; base += 1024) {
    const int i = base + tid;
    const int v = i < n ? in[i] : 0;
    int x = v;
    for (int dd = 1; dd < 64; dd <<= 1) {
      const int t = __shfl_up(x, dd);
      if (lane >= dd) x += t;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int woff = 0, tot = 0;
    for (int k = 0; k < 16; ++k) {
      if (k < w) woff += wsum[k];
      tot += wsum[k];
    }
    if (i < n) out[i] = carry + woff + x - v;
    carry += tot;
    __syncthreads();
  }
  if (tid == 0) out[n] = carry;
}

// ---- refinement: up to five steps of the 3-D quadratic, then the contrast and edge tests
__global__ __launch_bounds__(256) void sift_refine_kernel(const SiftArgs a, const int4* cand, SiftKp* kp, const int n) {
  const int c = (int)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const int4 cd = cand[c];
  const SiftImage im = a.img[cd.x];
  const int o = cd.y & 255;
  int i = cd.y >> 8, y = cd.z, x = cd.w;
  const int h = im.H0 >> o, w = im.W0 >> o;
  const int64_t plane = (int64_t)h * w;
  const float* g0 = sf_layer(a, im, o, 0);
  SiftKp k;
  k.alive = 0;
  k.i = i, k.y = y, k.x = x;
  k.Xx = k.Xy = k.Xs = k.contr = 0.f;
  bool ok = false;
  float v = 0.f, dx = 0.f, dy = 0.f, dz = 0.f, dxx = 0.f, dyy = 0.f, dxy = 0.f, X0 = 0.f, X1 = 0.f, X2 = 0.f;
  for (int step = 0; step < 5; ++step) {
    const float* g = g0 + (int64_t)y * w + x;
#define SF_D(di, ddy, ddx) (g[(i + (di) + 1) * plane + (ddy) * w + (ddx)] - g[(i + (di)) * plane + (ddy) * w + (ddx)])
    v = SF_D(0, 0, 0);
    const float xp = SF_D(0, 0, 1), xm = SF_D(0, 0, -1), yp = SF_D(0, 1, 0), ym = SF_D(0, -1, 0), sp = SF_D(1, 0, 0), sm = SF_D(-1, 0, 0);
    dx = (xp - xm) * 0.5f;
    dy = (yp - ym) * 0.5f;
    dz = (sp - sm) * 0.5f;
    dxx = xp + xm - 2.0f * v;
    dyy = yp + ym - 2.0f * v;
    const float dss = sp + sm - 2.0f * v;
    dxy = (SF_D(0, 1, 1) - SF_D(0, 1, -1) - SF_D(0, -1, 1) + SF_D(0, -1, -1)) * 0.25f;
    const float dxs = (SF_D(1, 0, 1) - SF_D(1, 0, -1) - SF_D(-1, 0, 1) + SF_D(-1, 0, -1)) * 0.25f;
    const float dys = (SF_D(1, 1, 0) - SF_D(1, -1, 0) - SF_D(-1, 1, 0) + SF_D(-1, -1, 0)) * 0.25f;
#undef SF_D
    const float c00 = dyy * dss - dys * dys, c01 = dxs * dys - dxy * dss, c02 = dxy * dys - dxs * dyy;
    const float c11 = dxx * dss - dxs * dxs, c12 = dxy * dxs - dxx * dys, c22 = dxx * dyy - dxy * dxy;
    const float det = dxx * c00 + dxy * c01 + dxs * c02;
    if (det == 0.f) break;
    const float inv = -1.0f / det;
    X0 = (c00 * dx + c01 * dy + c02 * dz) * inv;
    X1 = (c01 * dx + c11 * dy + c12 * dz) * inv;
    X2 = (c02 * dx + c12 * dy + c22 * dz) * inv;
    if (fabsf(X0) < 0.5f && fabsf(X1) < 0.5f && fabsf(X2) < 0.5f) {
      ok = true;
      break;
    }
    if (!(fabsf(X0) <= 1048576.f && fabsf(X1) <= 1048576.f && fabsf(X2) <= 1048576.f)) break;   // also refuses NaN
    x += (int)floorf(X0 + 0.5f);
    y += (int)floorf(X1 + 0.5f);
    i += (int)floorf(X2 + 0.5f);
    if (i < 1 || i > a.L || x < SF_BORDER || x > w - 1 - SF_BORDER || y < SF_BORDER || y > h - 1 - SF_BORDER) break;
  }
  if (ok) {
    const float contr = v + 0.5f * (dx * X0 + dy * X1 + dz * X2);
    const float tr = dxx + dyy, det2 = dxx * dyy - dxy * dxy;
    const float q = tr * tr * a.edge_r - a.edge_r1sq * det2;
    if (fabsf(contr) >= a.thr_c && det2 > 0.f && q < 0.f) {
      k.alive = 1;
      k.i = i, k.y = y, k.x = x;
      k.Xx = X0, k.Xy = X1, k.Xs = X2, k.contr = contr;
    }
  }
  kp[c] = k;
}

__device__ inline void sf_grad(const float* G, int w, int py, int px, float& mag, float& th) {
  const float* c = G + (int64_t)py * w + px;
  const float gx = c[1] - c[-1], gy = c[w] - c[-w];
  mag = sqrtf(gx * gx + gy * gy);
  th = atan2f(gy, gx);
  if (th < 0.f) th += 6.283185307179586f;
}

// ---- orientation: one wave per candidate
__global__ __launch_bounds__(64) void sift_orient_kernel(const SiftArgs a, const int4* cand, const SiftKp* kp, int* npeaks, float* bins) {
  __shared__ float col[36 * SF_HSTRIDE];
  __shared__ float raw[36], sm[36];
  const int c = blockIdx.x, lane = threadIdx.x;
  const SiftKp k = kp[c];
  if (!k.alive) {
    if (lane == 0) npeaks[c] = 0;
    return;
  }
  const int4 cd = cand[c];
  const SiftImage im = a.img[cd.x];
  const int o = cd.y & 255, h = im.H0 >> o, w = im.W0 >> o;
  const float* G = sf_layer(a, im, o, k.i);
  const float scl = a.sigma * exp2f(((float)k.i + k.Xs) / (float)a.L);
  const int rad = (int)floorf(4.5f * scl + 0.5f);
  const float sw = 1.5f * scl, cw = -1.0f / (2.0f * sw * sw);
  for (int b = 0; b < 36; ++b) col[b * SF_HSTRIDE + lane] = 0.f;
  const int side = 2 * rad + 1;
  for (int idx = lane; idx < side * side; idx += 64) {
    const int dy = idx / side - rad, dx = idx - (dy + rad) * side - rad;
    const int py = k.y + dy, px = k.x + dx;
    if (py < 1 || py > h - 2 || px < 1 || px > w - 2) continue;
    float mag, th;
    sf_grad(G, w, py, px, mag, th);
    const float wgt = expf((float)(dx * dx + dy * dy) * cw);
    const float t = th * 5.729577951308232f;   // 36 / 2 pi
    const float fl = floorf(t), f = t - fl;
    const int b0 = ((int)fl) % 36, b1 = (b0 + 1) % 36;
    const float wm = wgt * mag;
    col[b0 * SF_HSTRIDE + lane] += wm * (1.0f - f);
    col[b1 * SF_HSTRIDE + lane] += wm * f;
  }
  __syncthreads();
  if (lane < 36) {
    float s = 0.f;
    for (int l = 0; l < 64; ++l) s += col[lane * SF_HSTRIDE + l];
    raw[lane] = s;
  }
  __syncthreads();
  if (lane < 36) {
    const int i = lane;
    sm[i] = (raw[(i + 34) % 36] + raw[(i + 2) % 36]) * (1.0f / 16.0f) + (raw[(i + 35) % 36] + raw[(i + 1) % 36]) * (4.0f / 16.0f) +
            raw[i] * (6.0f / 16.0f);
  }
  __syncthreads();
  if (lane == 0) {
    float top = sm[0];
    for (int i = 1; i < 36; ++i) top = fmaxf(top, sm[i]);
    int n = 0;
    for (int i = 0; i < 36; ++i) {
      const float l = sm[(i + 35) % 36], r = sm[(i + 1) % 36], m = sm[i];
      if (m > l && m > r && m >= 0.8f * top && n < SF_MAX_PEAKS) {
        float b = (float)i + 0.5f * (l - r) / (l - 2.0f * m + r);
        if (b < 0.f) b += 36.0f;
        if (b >= 36.0f) b -= 36.0f;
        bins[(int64_t)c * SF_MAX_PEAKS + n++] = b;
      }
    }
    npeaks[c] = n;
  }
}

// ---- nfeatures: rows kept per candidate.  Rank of a candidate's first row = rows of its image with a larger |response|, or an equal
// one earlier in the order; cand_start[img] .. cand_start[img + 1] are the image's candidates
__global__ __launch_bounds__(256) void sift_rank_kernel(const int4* cand, const SiftKp* kp, const int* npeaks, const int* cand_start,
                                                        int* nkeep, const int n, const int nfeatures) {
  const int c = (int)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const int np = npeaks[c];
  if (np == 0) {
    nkeep[c] = 0;
    return;
  }
  const int img = cand[c].x;
  const float r = fabsf(kp[c].contr);
  int rank = 0;
  for (int j = cand_start[img]; j < cand_start[img + 1]; ++j) {
    const int nj = npeaks[j];
    if (nj == 0 || j == c) continue;
    const float rj = fabsf(kp[j].contr);
    if (rj > r || (rj == r && j < c)) rank += nj;
  }
  nkeep[c] = max(0, min(np, nfeatures - rank));
}

// rows in front of each image of the chunk: img_rows[i] = row_off[cand_start[i]], i = 0 .. n_img
__global__ void sift_img_rows_kernel(const int* row_off, const int* cand_start, int* img_rows, const int n_img) {
  const int i = (int)blockIdx.x * 256 + threadIdx.x;
  if (i <= n_img) img_rows[i] = row_off[cand_start[i]];
}
// cand_start[i] = scanned block offset at the image's first block (i = n_img: the total)
__global__ void sift_cand_start_kernel(const int* block_off, int* cand_start, const int n_img, const int stride) {
  const int i = (int)blockIdx.x * 256 + threadIdx.x;
  if (i <= n_img) cand_start[i] = block_off[(int64_t)i * stride];
}

// ---- descriptors: one wave per candidate
struct SiftDescArgs {
  const int4* cand;
  const SiftKp* kp;
  const int* nkeep;
  const int* row_off;
  const float* bins;
  void* out;
  float* frames;
  int64_t row_base, capacity;
  int out_kind;
};
__global__ __launch_bounds__(64) void sift_desc_kernel(const SiftArgs a, const SiftDescArgs d) {
  __shared__ float col[128 * SF_HSTRIDE];
  __shared__ float acc[128];
  const int c = blockIdx.x, lane = threadIdx.x;
  const int nk = d.nkeep[c];
  if (nk == 0) return;
  const SiftKp k = d.kp[c];
  const int4 cd = d.cand[c];
  const SiftImage im = a.img[cd.x];
  const int o = cd.y & 255, h = im.H0 >> o, w = im.W0 >> o;
  const float* G = sf_layer(a, im, o, k.i);
  const float scl = a.sigma * exp2f(((float)k.i + k.Xs) / (float)a.L);
  const float hw = 3.0f * scl;
  const int rad = (int)floorf(hw * 3.5355339059327378f + 0.5f);   // sqrt(2) * 2.5
  const int side = 2 * rad + 1;
  for (int p = 0; p < nk; ++p) {
    const int64_t row = d.row_base + d.row_off[c] + p;
    if (row >= d.capacity) return;                                  // uniform over the wave
    const float b = d.bins[(int64_t)c * SF_MAX_PEAKS + p];
    const float theta = b * 0.17453292519943295f;                   // 2 pi / 36
    const float ct = cosf(theta), st = sinf(theta);
    for (int e = 0; e < 128; ++e) col[e * SF_HSTRIDE + lane] = 0.f;
    for (int idx = lane; idx < side * side; idx += 64) {
      const int dy = idx / side - rad, dx = idx - (dy + rad) * side - rad;
      const int py = k.y + dy, px = k.x + dx;
      if (py < 1 || py > h - 2 || px < 1 || px > w - 2) continue;
      const float c_rot = ((float)dx * ct + (float)dy * st) / hw;
      const float r_rot = ((float)dy * ct - (float)dx * st) / hw;
      const float rbin = r_rot + 1.5f, cbin = c_rot + 1.5f;
      if (!(rbin > -1.f && rbin < 4.f && cbin > -1.f && cbin < 4.f)) continue;
      float mag, th;
      sf_grad(G, w, py, px, mag, th);
      const float wgt = expf((c_rot * c_rot + r_rot * r_rot) * -0.125f);
      float ob = (th - theta) * 1.2732395447351628f;                // 8 / 2 pi
      if (ob < 0.f) ob += 8.0f;
      if (ob >= 8.0f) ob -= 8.0f;
      const float r0f = floorf(rbin), c0f = floorf(cbin), o0f = floorf(ob);
      const float fr = rbin - r0f, fc = cbin - c0f, fo = ob - o0f;
      const int r0 = (int)r0f, c0 = (int)c0f, o0 = (int)o0f;
      const float v = wgt * mag;
#pragma unroll
      for (int dr = 0; dr < 2; ++dr) {
        const int rr = r0 + dr;
        if (rr < 0 || rr > 3) continue;
        const float vr = v * (dr ? fr : 1.0f - fr);
#pragma unroll
        for (int dc = 0; dc < 2; ++dc) {
          const int cc = c0 + dc;
          if (cc < 0 || cc > 3) continue;
          const float vc = vr * (dc ? fc : 1.0f - fc);
          col[((rr * 4 + cc) * 8 + (o0 & 7)) * SF_HSTRIDE + lane] += vc * (1.0f - fo);
          col[((rr * 4 + cc) * 8 + ((o0 + 1) & 7)) * SF_HSTRIDE + lane] += vc * fo;
        }
      }
    }
    __syncthreads();
    for (int e = lane; e < 128; e += 64) {
      float s = 0.f;
      for (int l = 0; l < 64; ++l) s += col[e * SF_HSTRIDE + l];
      acc[e] = s;
    }
    __syncthreads();
    // the row tail: eight lanes per row, sixteen consecutive elements per lane; the wave holds eight identical copies and lanes
    // 0..7 store.  A row is zeroed only when its norm is 0
    const int q = lane & 7;
    sift_row_tail(acc + q * 16, 0.f, d.out_kind, d.out, row, q, lane < 8);
    if (lane == 0 && d.frames) {
      const float scale = (float)(1 << o), u = a.upsample ? 2.0f : 1.0f, off = a.upsample ? 0.25f : 0.0f;
      float* f = d.frames + row * 6;
      f[0] = ((float)k.x + k.Xx) * scale / u - off;
      f[1] = ((float)k.y + k.Xy) * scale / u - off;
      f[2] = 2.0f * scl * scale / u;
      f[3] = b * 10.0f;
      f[4] = fabsf(k.contr);
      f[5] = (float)o;
    }
    __syncthreads();
  }
}

static void sf_taps(double sigma, int* R, float* taps) {
  const int r = (int)std::ceil(4.0 * sigma - 1e-12);
  *R = r;
  if (r <= SF_MAX_RADIUS) gaussian_taps(sigma, r, taps);
}

static int sf_check(int nfeatures, int L, double contrast, double edge, double sigma, int upsample, double* base, double* inc) {
  if (nfeatures < 0) PVS_FAIL(PVS_ERR_INVALID, "SIFT: nfeatures must be >= 0 (got %d)", nfeatures);
  if (L < 1) PVS_FAIL(PVS_ERR_INVALID, "SIFT: n_octave_layers must be >= 1 (got %d)", L);
  if (L > SF_MAX_LAYERS) PVS_FAIL(PVS_ERR_UNSUPPORTED, "SIFT: at most %d octave layers (got %d)", SF_MAX_LAYERS, L);
  if (!(contrast >= 0.0)) PVS_FAIL(PVS_ERR_INVALID, "SIFT: contrast_threshold must be >= 0");
  if (!(edge > 0.0)) PVS_FAIL(PVS_ERR_INVALID, "SIFT: edge_threshold must be > 0");
  if (!(sigma > 0.0) || !std::isfinite(sigma)) PVS_FAIL(PVS_ERR_INVALID, "SIFT: sigma must be > 0");
  const double assumed = upsample ? 1.0 : 0.5;
  *base = std::sqrt(std::max(sigma * sigma - assumed * assumed, 0.01));
  const double k = std::pow(2.0, 1.0 / L);
  double worst = *base;
  for (int i = 1; i <= L + 2; ++i) {
    const double s1 = sigma * std::pow(k, i), s0 = sigma * std::pow(k, i - 1);
    inc[i] = std::sqrt(s1 * s1 - s0 * s0);
    worst = std::max(worst, inc[i]);
  }
  if ((int)std::ceil(4.0 * worst - 1e-12) > SF_MAX_RADIUS)
    PVS_FAIL(PVS_ERR_UNSUPPORTED, "SIFT: sigma %g needs a blur radius above %d", sigma, SF_MAX_RADIUS);
  return PVS_OK;
}

}  // namespace pvs

using namespace pvs;

PVS_EXPORT int pvs_sift_workspace(int H, int W, int n_octave_layers, int upsample, size_t* bytes, int64_t* max_rows) {
  if (H < 1 || W < 1) PVS_FAIL(PVS_ERR_INVALID, "SIFT: image size %d x %d", H, W);
  if (n_octave_layers < 1 || n_octave_layers > SF_MAX_LAYERS) PVS_FAIL(PVS_ERR_INVALID, "SIFT: n_octave_layers out of range");
  if (H > (1 << 28) || W > (1 << 28)) PVS_FAIL(PVS_ERR_INVALID, "SIFT: image too large");
  const int h0 = upsample ? 2 * H : H, w0 = upsample ? 2 * W : W;
  const int n = sf_octaves(h0, w0);
  if (bytes) *bytes = (size_t)sf_oct_off(h0, w0, n, n_octave_layers + 3) * sizeof(float);
  if (max_rows) {
    // a strict extremum excludes its 26 neighbours, so at most every second pixel per axis and layer; SF_MAX_PEAKS rows each
    int64_t m = 0;
    for (int o = 0; o < n; ++o) m += (int64_t)(((h0 >> o) + 1) / 2) * (((w0 >> o) + 1) / 2) * ((n_octave_layers + 1) / 2);
    *max_rows = m * SF_MAX_PEAKS;
  }
  return PVS_OK;
}

PVS_EXPORT int pvs_sift_dev(pvs_ctx* ctx, const void* d_pixels, int pixel_kind, const int32_t* h_hw, const int64_t* h_pix_offsets,
                            int64_t n_images, int nfeatures, int n_octave_layers, double contrast_threshold, double edge_threshold,
                            double sigma, int upsample, int out_kind, void* d_rows, int64_t capacity_rows, float* d_frames,
                            int64_t* d_row_offsets, int64_t* h_total_rows) {
  if (!ctx) PVS_FAIL(PVS_ERR_INVALID, "pvs_sift_dev: null ctx");
  double base_sigma = 0.0, inc[SF_MAX_LAYERS + 3] = {0};
  PVS_TRY(sf_check(nfeatures, n_octave_layers, contrast_threshold, edge_threshold, sigma, upsample, &base_sigma, inc));
  ImageIntake in{"SIFT", "pvs_sift_dev", h_hw, h_pix_offsets};
  PVS_TRY(in.open(pixel_kind, out_kind, n_images));
  if (capacity_rows < 0) PVS_FAIL(PVS_ERR_INVALID, "SIFT: negative capacity");
  if (n_images == 0) return PVS_OK;
  if (!d_row_offsets || !h_total_rows) PVS_FAIL(PVS_ERR_INVALID, "pvs_sift_dev: null row offsets or total");
  if (!d_pixels) PVS_FAIL(PVS_ERR_INVALID, "pvs_sift_dev: null pixels");
  if (capacity_rows > 0 && !d_rows) PVS_FAIL(PVS_ERR_INVALID, "pvs_sift_dev: null rows");
  PVS_HIP(hipSetDevice(ctx->device));

  const int L = n_octave_layers, nl = L + 3;
  std::vector<SiftImage> table((size_t)n_images);
  for (int64_t i = 0; i < n_images; ++i) {
    int H, W;
    int64_t po;
    PVS_TRY(in.next(i, &H, &W, &po));
    if (H > 16384 || W > 16384) PVS_FAIL(PVS_ERR_UNSUPPORTED, "SIFT: image %lld is larger than 16384 pixels per side", (long long)i);
    SiftImage& im = table[(size_t)i];
    im.H = H, im.W = W;
    im.H0 = upsample ? 2 * H : H, im.W0 = upsample ? 2 * W : W;
    im.n_oct = sf_octaves(im.H0, im.W0);
    im.pad = 0;
    im.pix_off = po;
    im.ws_off = 0;
  }

  SiftArgs a;
  memset(&a, 0, sizeof(a));
  a.pixels = d_pixels;
  a.pix_kind = pixel_kind;
  a.upsample = upsample ? 1 : 0;
  a.L = L, a.nl = nl;
  a.pre = (float)(0.5 * contrast_threshold / L * 255.0);
  a.thr_c = (float)(255.0 * contrast_threshold / L);
  a.edge_r = (float)edge_threshold;
  a.edge_r1sq = (float)((edge_threshold + 1.0) * (edge_threshold + 1.0));
  a.sigma = (float)sigma;

  std::vector<int64_t> counts((size_t)n_images, 0);
  std::vector<int> h_img_rows;
  int64_t total = 0;
  ScopedTimer tm(ctx, T_MISC);
  for (int64_t c0 = 0; c0 < n_images;) {
    // ---- the chunk: images whose pyramids fit the budget together (at least one)
    int64_t c1 = c0, floats = 0;
    int max_oct = 0;
    int64_t max_px[SF_MAX_OCT] = {0};
    while (c1 < n_images && c1 - c0 < SF_CHUNK_IMAGES) {
      SiftImage& im = table[(size_t)c1];
      const int64_t need = sf_oct_off(im.H0, im.W0, im.n_oct, nl);
      if (c1 > c0 && (size_t)(floats + need) * sizeof(float) > SF_PYRAMID_BUDGET) break;
      im.ws_off = floats;
      floats += need;
      max_oct = std::max(max_oct, im.n_oct);
      for (int o = 0; o < im.n_oct; ++o) max_px[o] = std::max<int64_t>(max_px[o], (int64_t)(im.H0 >> o) * (im.W0 >> o));
      ++c1;
    }
    const int n_img = (int)(c1 - c0);
    c0 = c1;
    if (max_oct == 0) continue;                       // nothing in this chunk has an octave
    const int64_t first = c1 - n_img;
    int gx[SF_MAX_OCT], base[SF_MAX_OCT], stride = 0;
    for (int o = 0; o < max_oct; ++o) {
      gx[o] = (int)((max_px[o] + 255) / 256);
      base[o] = stride;
      stride += L * gx[o];
    }
    const int64_t n_blocks = (int64_t)n_img * stride;
    if (n_blocks > (1ll << 30)) PVS_FAIL(PVS_ERR_UNSUPPORTED, "SIFT: chunk too large");

    float* d_pyr = nullptr;
    char* d_meta = nullptr;
    PVS_TRY(ws_reserve(ctx, WS_SIFT_PYRAMID, (size_t)floats * sizeof(float), &d_pyr));
    WsLayout<16> meta;
    const auto table_p = meta.add<SiftImage>((size_t)n_img);
    const auto cnt_p = meta.add<int>((size_t)n_blocks + 1), off_p = meta.add<int>((size_t)n_blocks + 1);
    const auto cand_start_p = meta.add<int>((size_t)n_img + 1), img_rows_p = meta.add<int>((size_t)n_img + 1);
    PVS_TRY(ws_reserve(ctx, WS_SIFT_TABLES, meta.bytes(), &d_meta));
    SiftImage* d_table = table_p(d_meta);
    int* d_cnt = cnt_p(d_meta);
    int* d_off = off_p(d_meta);
    int* d_cand_start = cand_start_p(d_meta);
    int* d_img_rows = img_rows_p(d_meta);
    PVS_HIP(hipMemcpyAsync(d_table, table.data() + first, (size_t)n_img * sizeof(SiftImage), hipMemcpyHostToDevice, ctx->stream));
    a.img = d_table;
    a.pyr = d_pyr;

    // ---- pyramid
    hipLaunchKernelGGL(sift_base_kernel, dim3((unsigned)gx[0], (unsigned)n_img), dim3(256), 0, ctx->stream, a);
    PVS_HIP(hipGetLastError());
    for (int o = 0; o < max_oct; ++o) {
      const unsigned tiles = (unsigned)((max_px[o] + SF_TILE * SF_TILE - 1) / (SF_TILE * SF_TILE)) + 0u;
      // tiles of the largest image by area may be fewer than another image needs along one axis: size by the worst case per axis
      unsigned need_tiles = tiles;
      for (int64_t i = first; i < c1; ++i) {
        const SiftImage& im = table[(size_t)i];
        if (o >= im.n_oct) continue;
        const unsigned t = (unsigned)((((im.W0 >> o) + SF_TILE - 1) / SF_TILE) * (((im.H0 >> o) + SF_TILE - 1) / SF_TILE));
        need_tiles = std::max(need_tiles, t);
      }
      if (o > 0) {
        hipLaunchKernelGGL(sift_down_kernel, dim3((unsigned)gx[o], (unsigned)n_img), dim3(256), 0, ctx->stream, a, o);
        PVS_HIP(hipGetLastError());
      }
      for (int layer = (o == 0 ? 0 : 1); layer < nl; ++layer) {
        SiftBlurArgs b;
        memset(&b, 0, sizeof(b));
        b.o = o;
        b.src = layer == 0 ? 1 : layer - 1;      // octave 0, layer 0: the base blur of the scratch image held in layer 1
        b.dst = layer;
        sf_taps(layer == 0 ? base_sigma : inc[layer], &b.R, b.taps);
        const int Wr = SF_TILE + 2 * b.R;
        const size_t lds = (size_t)(Wr * Wr + Wr * SF_TILE) * sizeof(float);
        hipLaunchKernelGGL(sift_blur_kernel, dim3(need_tiles, (unsigned)n_img), dim3(256), lds, ctx->stream, a, b);
        PVS_HIP(hipGetLastError());
      }
    }

    // ---- candidates: count, scan, write
    SiftDetectArgs d;
    d.counts = d_cnt;
    d.cand = nullptr;
    d.stride = stride;
    for (int o = 0; o < max_oct; ++o) {
      d.o = o, d.base = base[o];
      hipLaunchKernelGGL(sift_detect_kernel<false>, dim3((unsigned)gx[o], (unsigned)n_img, (unsigned)L), dim3(256), 0, ctx->stream, a, d);
      PVS_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(sift_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_cnt, d_off, (int)n_blocks);
    PVS_HIP(hipGetLastError());
    int n_cand = 0;
    PVS_HIP(hipMemcpyAsync(&n_cand, d_off + n_blocks, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PVS_HIP(hipStreamSynchronize(ctx->stream));
    if (n_cand == 0) continue;

    char* d_kp_block = nullptr;
    const auto kl = sift_cand_layout<int4, SiftKp>((size_t)n_cand, SF_MAX_PEAKS);
    PVS_TRY(ws_reserve(ctx, WS_SIFT_KEYPOINTS, kl.bytes, &d_kp_block));
    int4* d_cand = kl.cand(d_kp_block);
    SiftKp* d_kp = kl.kp(d_kp_block);
    int* d_npeaks = kl.npeaks(d_kp_block);
    int* d_nkeep = kl.nkeep(d_kp_block);
    int* d_row_off = kl.row_off(d_kp_block);
    float* d_bins = kl.bins(d_kp_block);
    d.counts = d_off;
    d.cand = d_cand;
    for (int o = 0; o < max_oct; ++o) {
      d.o = o, d.base = base[o];
      hipLaunchKernelGGL(sift_detect_kernel<true>, dim3((unsigned)gx[o], (unsigned)n_img, (unsigned)L), dim3(256), 0, ctx->stream, a, d);
      PVS_HIP(hipGetLastError());
    }
    const unsigned cb = (unsigned)((n_cand + 255) / 256), ib = (unsigned)((n_img + 256) / 256);
    hipLaunchKernelGGL(sift_cand_start_kernel, dim3(ib), dim3(256), 0, ctx->stream, d_off, d_cand_start, n_img, stride);
    hipLaunchKernelGGL(sift_refine_kernel, dim3(cb), dim3(256), 0, ctx->stream, a, d_cand, d_kp, n_cand);
    hipLaunchKernelGGL(sift_orient_kernel, dim3((unsigned)n_cand), dim3(64), 0, ctx->stream, a, d_cand, d_kp, d_npeaks, d_bins);
    PVS_HIP(hipGetLastError());
    const int* d_keep = d_npeaks;
    if (nfeatures > 0) {
      hipLaunchKernelGGL(sift_rank_kernel, dim3(cb), dim3(256), 0, ctx->stream, d_cand, d_kp, d_npeaks, d_cand_start, d_nkeep, n_cand, nfeatures);
      PVS_HIP(hipGetLastError());
      d_keep = d_nkeep;
    }
    hipLaunchKernelGGL(sift_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_keep, d_row_off, n_cand);
    hipLaunchKernelGGL(sift_img_rows_kernel, dim3(ib), dim3(256), 0, ctx->stream, d_row_off, d_cand_start, d_img_rows, n_img);
    PVS_HIP(hipGetLastError());
    h_img_rows.resize((size_t)n_img + 1);
    PVS_HIP(hipMemcpyAsync(h_img_rows.data(), d_img_rows, ((size_t)n_img + 1) * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PVS_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n_img; ++i) counts[(size_t)(first + i)] = h_img_rows[(size_t)i + 1] - h_img_rows[(size_t)i];
    const int64_t chunk_rows = h_img_rows[(size_t)n_img];
    if (chunk_rows > 0 && total < capacity_rows) {
      SiftDescArgs e;
      e.cand = d_cand, e.kp = d_kp, e.nkeep = d_keep, e.row_off = d_row_off, e.bins = d_bins;
      e.out = d_rows, e.frames = d_frames;
      e.row_base = total, e.capacity = capacity_rows;
      e.out_kind = out_kind;
      hipLaunchKernelGGL(sift_desc_kernel, dim3((unsigned)n_cand), dim3(64), 0, ctx->stream, a, e);
      PVS_HIP(hipGetLastError());
    }
    total += chunk_rows;
  }

  std::vector<int64_t> h_off((size_t)n_images + 1, 0);
  for (int64_t i = 0; i < n_images; ++i) h_off[(size_t)i + 1] = h_off[(size_t)i] + counts[(size_t)i];
  PVS_HIP(hipMemcpyAsync(d_row_offsets, h_off.data(), h_off.size() * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  PVS_HIP(hipStreamSynchronize(ctx->stream));
  *h_total_rows = total;
  if (total > capacity_rows)
    PVS_FAIL(PVS_ERR_CAPACITY, "SIFT: %lld rows do not fit the output of %lld rows", (long long)total, (long long)capacity_rows);
  return PVS_OK;
}
