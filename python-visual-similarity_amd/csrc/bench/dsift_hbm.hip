// Measurement only: dense SIFT with the eight orientation planes kept in HBM, next to the product kernel (dsift.hip), which
// keeps every intermediate in LDS.  The straightforward whole-image form of DESIGN.md section 9, one kernel per step:
//   k1 gray + horizontal Gaussian -> T;  k2 vertical Gaussian -> S;  k3 gradient -> eight planes P [y][x][8];
//   k4 triangular sums along x -> A;  k5 along y -> B;  k6 gather the 4 x 4 bin centres, normalise, quantise -> uint8 rows.
// Same tap order and the same eight-lane normalisation as the product, so the rows are compared byte for byte.
// Usage: dsift_hbm [images=256] [H=500] [W=600] [step=16] [sizes=4,8] [steps=20]   -> one JSON line
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../../include/pvsim.h"

#define CK(e)                                                                      \
  do {                                                                             \
    hipError_t r__ = (e);                                                          \
    if (r__ != hipSuccess) {                                                       \
      fprintf(stderr, "%s: %s (line %d)\n", #e, hipGetErrorString(r__), __LINE__); \
      return 2;                                                                    \
    }                                                                              \
  } while (0)
#define PK(e)                                                              \
  do {                                                                     \
    if ((e) != PVS_OK) {                                                   \
      fprintf(stderr, "%s: %s (line %d)\n", #e, pvs_last_error(), __LINE__); \
      return 2;                                                            \
    }                                                                      \
  } while (0)

struct Taps {
  int radius;
  float t[65];
};

__global__ void k_hsmooth(const unsigned char* pix, int H, int W, Taps tp, float* T) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  const unsigned char* row = pix + ((size_t)blockIdx.z * H + y) * W * 3;
  float acc = 0.f;
  for (int k = 0; k <= 2 * tp.radius; ++k) {
    const unsigned char* q = row + 3 * min(max(x + k - tp.radius, 0), W - 1);
    acc = fmaf(tp.t[k], 0.299f * (float)q[0] + 0.587f * (float)q[1] + 0.114f * (float)q[2], acc);
  }
  T[((size_t)blockIdx.z * H + y) * W + x] = acc;
}

__global__ void k_vsmooth(const float* T, int H, int W, Taps tp, float* S) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  const float* im = T + (size_t)blockIdx.z * H * W;
  float acc = 0.f;
  for (int k = 0; k <= 2 * tp.radius; ++k) acc = fmaf(tp.t[k], im[(size_t)min(max(y + k - tp.radius, 0), H - 1) * W + x], acc);
  S[((size_t)blockIdx.z * H + y) * W + x] = acc;
}

__global__ void k_planes(const float* S, int H, int W, float* P) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  const float* c = S + ((size_t)blockIdx.z * H + y) * W + x;
  float gx, gy;
  if (x == 0) gx = c[1] - c[0];
  else if (x == W - 1) gx = c[0] - c[-1];
  else gx = 0.5f * (c[1] - c[-1]);
  if (y == 0) gy = c[W] - c[0];
  else if (y == H - 1) gy = c[0] - c[-W];
  else gy = 0.5f * (c[W] - c[-W]);
  const float m = sqrtf(gx * gx + gy * gy);
  float th = atan2f(gy, gx);
  if (th < 0.f) th += 6.283185307179586f;
  const float t = th * 1.2732395447351628f;
  const int b = (int)t;
  const float f = t - (float)b;
  const float hi = m * f, lo = m * (1.0f - f);
  const int b0 = b & 7, b1 = (b + 1) & 7;
  float p[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) p[o] = (b0 == o) ? lo : ((b1 == o) ? hi : 0.f);
  float4* dst = reinterpret_cast<float4*>(P + (((size_t)blockIdx.z * H + y) * W + x) * 8);
  dst[0] = make_float4(p[0], p[1], p[2], p[3]);
  dst[1] = make_float4(p[4], p[5], p[6], p[7]);
}

// out[y][x][o] = sum_d w(d) in[y + d dy][x + d dx][o], zero outside the image (no support the grid allows reaches there)
__global__ void k_tri(const float* in, int H, int W, int s, int along_y, float* out) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  const float* im = in + (size_t)blockIdx.z * H * W * 8;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int d = -(s - 1); d <= s - 1; ++d) {
    const int xx = along_y ? x : x + d, yy = along_y ? y + d : y;
    if (xx < 0 || xx >= W || yy < 0 || yy >= H) continue;
    const float w = 1.0f - (float)abs(d) / (float)s;
    const float4* q = reinterpret_cast<const float4*>(im + ((size_t)yy * W + xx) * 8);
    const float4 a = q[0], b = q[1];
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    if (along_y) {
#pragma unroll
      for (int o = 0; o < 8; ++o) acc[o] = fmaf(w, v[o], acc[o]);
    } else {
#pragma unroll
      for (int o = 0; o < 8; ++o) acc[o] = __fadd_rn(acc[o], __fmul_rn(w, v[o]));
    }
  }
  float4* dst = reinterpret_cast<float4*>(out + (((size_t)blockIdx.z * H + y) * W + x) * 8);
  dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
  dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
}

// eight lanes per descriptor, as stage 7 of the product kernel
__global__ void k_rows(const float* B, int H, int W, int s, int step, int nx, int ny, long long rows_per_image, long long row_off,
                       unsigned char* out) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int q = (int)(gid & 7);
  const long long dsc = gid >> 3;
  const long long per = (long long)nx * ny;
  const int img = blockIdx.y;
  const bool live = dsc < per;
  const int da = live ? (int)(dsc % nx) : 0, db = live ? (int)(dsc / nx) : 0;
  const int j = q >> 1, i0 = (q & 1) * 2;
  const int y = s - 1 + db * step + j * s, x = s - 1 + da * step + i0 * s;
  const float* im = B + (size_t)img * H * W * 8;
  float v[16];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const float4* src = reinterpret_cast<const float4*>(im + ((size_t)y * W + x + c * s) * 8);
    const float4 a = src[0], b = src[1];
    v[8 * c + 0] = a.x, v[8 * c + 1] = a.y, v[8 * c + 2] = a.z, v[8 * c + 3] = a.w;
    v[8 * c + 4] = b.x, v[8 * c + 5] = b.y, v[8 * c + 6] = b.z, v[8 * c + 7] = b.w;
  }
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) ss = fmaf(v[k], v[k], ss);
  ss += __shfl_xor(ss, 1);
  ss += __shfl_xor(ss, 2);
  ss += __shfl_xor(ss, 4);
  const float n1 = sqrtf(ss);
  const bool zero = !(n1 > 0.f);
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = zero ? 0.f : fminf(v[k] / n1, 0.2f);
  float s2 = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) s2 = fmaf(v[k], v[k], s2);
  s2 += __shfl_xor(s2, 1);
  s2 += __shfl_xor(s2, 2);
  s2 += __shfl_xor(s2, 4);
  const float n2 = sqrtf(s2);
  if (!live) return;
  unsigned int w[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    unsigned int word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float r = fminf(floorf(fmaf(512.f, zero ? 0.f : v[4 * g + k] / n2, 0.5f)), 255.f);
      word |= (unsigned int)r << (8 * k);
    }
    w[g] = word;
  }
  const long long row = (long long)img * rows_per_image + row_off + dsc;
  reinterpret_cast<uint4*>(out + row * 128)[q] = make_uint4(w[0], w[1], w[2], w[3]);
}

static int grid1(int extent, int s, int step) { return extent >= 5 * s - 1 ? (extent - 5 * s + 1) / step + 1 : 0; }

int main(int argc, char** argv) {
  const int B = argc > 1 ? atoi(argv[1]) : 256, H = argc > 2 ? atoi(argv[2]) : 500, W = argc > 3 ? atoi(argv[3]) : 600;
  const int step = argc > 4 ? atoi(argv[4]) : 16;
  std::vector<int32_t> sizes;
  {
    char buf[128];
    strncpy(buf, argc > 5 ? argv[5] : "4,8", sizeof(buf) - 1);
    buf[sizeof(buf) - 1] = 0;
    for (char* tok = strtok(buf, ","); tok; tok = strtok(nullptr, ",")) sizes.push_back(atoi(tok));
  }
  const int steps = argc > 6 ? atoi(argv[6]) : 20;
  if (B < 1 || H < 8 || W < 8 || step < 1 || sizes.empty()) return 1;

  pvs_ctx* ctx = nullptr;
  PK(pvs_init(0, nullptr, &ctx));
  hipStream_t st = static_cast<hipStream_t>(pvs_stream(ctx));
  int64_t per = 0;
  PK(pvs_dsift_count(H, W, step, sizes.data(), (int)sizes.size(), &per));
  const size_t npix = (size_t)B * H * W, total = (size_t)per * B;
  std::vector<unsigned char> h_pix(npix * 3);
  unsigned int lcg = 12345u;
  for (size_t i = 0; i < h_pix.size(); ++i) {   // blocky noise: gradients of every orientation, a few flat blocks
    const size_t p = i / 3, y = (p / W) % H, x = p % W;
    lcg = lcg * 1664525u + 1013904223u;
    h_pix[i] = (unsigned char)(((x / 7 + y / 5) * 37 + (lcg >> 27)) & 255);
  }
  unsigned char *d_pix, *d_out1, *d_out2;
  float *d_T, *d_S, *d_P, *d_A;
  int64_t* d_off;
  CK(hipMalloc(&d_pix, npix * 3));
  CK(hipMalloc(&d_out1, total * 128));
  CK(hipMalloc(&d_out2, total * 128));
  CK(hipMalloc(&d_T, npix * 4));
  CK(hipMalloc(&d_S, npix * 4));
  CK(hipMalloc(&d_P, npix * 32));
  CK(hipMalloc(&d_A, npix * 32));
  CK(hipMalloc(&d_off, (size_t)(B + 1) * 8));
  CK(hipMemcpy(d_pix, h_pix.data(), npix * 3, hipMemcpyHostToDevice));
  CK(hipMemset(d_out1, 0xee, total * 128));
  CK(hipMemset(d_out2, 0xdd, total * 128));
  std::vector<int32_t> hw(2 * (size_t)B);
  for (int i = 0; i < B; ++i) hw[2 * i] = H, hw[2 * i + 1] = W;

  auto product = [&]() -> int {
    return pvs_dsift_dev(ctx, d_pix, PVS_PIX_U8_RGB, hw.data(), nullptr, B, step, sizes.data(), (int)sizes.size(), 0.0, PVS_DSIFT_U8,
                         d_out1, (int64_t)total, d_off);
  };
  auto variant = [&]() -> int {
    const dim3 blk(128), grd((W + 127) / 128, H, B);
    long long row_off = 0;
    for (int s : sizes) {
      const int nx = grid1(W, s, step), ny = grid1(H, s, step);
      if (nx == 0 || ny == 0) continue;
      Taps tp;
      tp.radius = (4 * s + 5) / 6;
      if (tp.radius > 32) return 1;
      const double sigma = s / 6.0;
      double t[65], sum = 0.0;
      for (int d = -tp.radius; d <= tp.radius; ++d) sum += t[d + tp.radius] = std::exp(-(double)d * d / (2.0 * sigma * sigma));
      for (int d = 0; d <= 2 * tp.radius; ++d) tp.t[d] = (float)(t[d] / sum);
      hipLaunchKernelGGL(k_hsmooth, grd, blk, 0, st, d_pix, H, W, tp, d_T);
      hipLaunchKernelGGL(k_vsmooth, grd, blk, 0, st, d_T, H, W, tp, d_S);
      hipLaunchKernelGGL(k_planes, grd, blk, 0, st, d_S, H, W, d_P);
      hipLaunchKernelGGL(k_tri, grd, blk, 0, st, d_P, H, W, s, 0, d_A);
      hipLaunchKernelGGL(k_tri, grd, blk, 0, st, d_A, H, W, s, 1, d_P);
      const long long lanes = (long long)nx * ny * 8;
      hipLaunchKernelGGL(k_rows, dim3((unsigned)((lanes + 255) / 256), B), dim3(256), 0, st, d_P, H, W, s, step, nx, ny, (long long)per,
                         row_off, d_out2);
      row_off += (long long)nx * ny;
    }
    return hipGetLastError() == hipSuccess ? 0 : 1;
  };
  auto time_ms = [&](auto& fn, double* med, double* lo, double* hi) -> int {
    for (int i = 0; i < 3; ++i)
      if (fn()) return 1;
    if (pvs_sync(ctx) != PVS_OK) return 1;
    std::vector<double> ms;
    for (int i = 0; i < steps; ++i) {
      const auto t0 = std::chrono::steady_clock::now();
      if (fn()) return 1;
      if (pvs_sync(ctx) != PVS_OK) return 1;
      ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    *med = ms[ms.size() / 2], *lo = ms.front(), *hi = ms.back();
    return 0;
  };
  double pm, pl, ph, vm, vl, vh;
  if (time_ms(product, &pm, &pl, &ph)) {
    fprintf(stderr, "product path failed: %s\n", pvs_last_error());
    return 2;
  }
  if (time_ms(variant, &vm, &vl, &vh)) {
    fprintf(stderr, "variant failed\n");
    return 2;
  }
  std::vector<unsigned char> o1(total * 128), o2(total * 128);
  CK(hipMemcpy(o1.data(), d_out1, o1.size(), hipMemcpyDeviceToHost));
  CK(hipMemcpy(o2.data(), d_out2, o2.size(), hipMemcpyDeviceToHost));
  size_t differ = 0, nonzero = 0;
  int maxdiff = 0;
  for (size_t i = 0; i < o1.size(); ++i) {
    const int d = abs((int)o1[i] - (int)o2[i]);
    differ += d != 0;
    nonzero += o1[i] != 0;
    if (d > maxdiff) maxdiff = d;
  }
  // bytes the variant moves through HBM per size: T w, T r + S w, S r (x ~3 rows, cached) + P w, P r + A w, A r + P w, gather
  const double plane_bytes = (double)npix * 32.0;
  const double variant_bytes = (double)sizes.size() * ((double)npix * (3 + 4 + 8 + 4) + 5.0 * plane_bytes) + (double)total * 128 * 5;
  printf("{\"tool\": \"csrc/bench/dsift_hbm\", \"images\": %d, \"H\": %d, \"W\": %d, \"step\": %d, \"n_sizes\": %zu, \"rows\": %zu, "
         "\"planes_in_lds_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}, \"planes_in_hbm_ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}, "
         "\"hbm_over_lds\": %.3f, \"variant_hbm_bytes_estimate\": %.0f, \"bytes_differ\": %zu, \"max_byte_diff\": %d, \"nonzero_bytes\": %zu, "
         "\"steps\": %d}\n",
         B, H, W, step, sizes.size(), total, pm, pl, ph, vm, vl, vh, vm / pm, variant_bytes, differ, maxdiff, nonzero, steps);
  pvs_destroy(ctx);
  return 0;
}
