// What dense SIFT (dsift.hip) and keypoint SIFT (sift.hip) must agree on, defined once: how a pixel becomes gray, how sixteen
// accumulators per lane become a stored row, how Gaussian taps are filled and how a batch of images is taken in.  The encoders
// (DESC_U8_ROOTSIFT), match.hip and the shipped vocabularies read rows of either extractor: a row is what this file says it is.
#pragma once

#include "common.hpp"

namespace pvs {

// gray value of pixel (y, x) of a W-wide image that starts at element `base` of `pixels` (a pvs_pixel_kind)
__device__ inline float gray_at(const void* pixels, int pix_kind, int64_t base, int W, int y, int x) {
  const int64_t p = (int64_t)y * W + x;
  switch (pix_kind) {
    case PVS_PIX_U8_RGB: {
      const unsigned char* q = static_cast<const unsigned char*>(pixels) + base + 3 * p;
      return 0.299f * (float)q[0] + 0.587f * (float)q[1] + 0.114f * (float)q[2];
    }
    case PVS_PIX_U8_GRAY:
      return (float)static_cast<const unsigned char*>(pixels)[base + p];
    case PVS_PIX_F32_RGB: {
      const float* q = static_cast<const float*>(pixels) + base + 3 * p;
      return 0.299f * q[0] + 0.587f * q[1] + 0.114f * q[2];
    }
    default:
      return static_cast<const float*>(pixels)[base + p];
  }
}

// The row tail: normalise, clamp at 0.2, renormalise, quantise, store.  Eight consecutive lanes hold one row; lane q of them passes
// its sixteen accumulators acc[0 .. 15], elements 16 q .. 16 q + 15 of the row.  A row whose norm is not above `thr` is all zeros;
// PVS_DSIFT_F32_RAW stores the accumulators as they came.  Every lane of the eight must call this (the sums cross the lanes in a
// fixed butterfly); `store` gates the stores alone.
__device__ __forceinline__ void sift_row_tail(const float* acc, float thr, int out_kind, void* out, int64_t row, int q, bool store) {
  float v[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) v[k] = acc[k];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) ss = fmaf(v[k], v[k], ss);
  ss += __shfl_xor(ss, 1);
  ss += __shfl_xor(ss, 2);
  ss += __shfl_xor(ss, 4);
  const float n1 = sqrtf(ss);
  if (out_kind != PVS_DSIFT_F32_RAW) {
    const bool zero = !(n1 > thr);
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = zero ? 0.f : fminf(v[k] / n1, 0.2f);
    float s2 = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s2 = fmaf(v[k], v[k], s2);
    s2 += __shfl_xor(s2, 1);
    s2 += __shfl_xor(s2, 2);
    s2 += __shfl_xor(s2, 4);
    const float n2 = sqrtf(s2);
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = zero ? 0.f : v[k] / n2;
  }
  if (!store) return;
  if (out_kind == PVS_DSIFT_U8) {
    unsigned int w[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      unsigned int word = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float r = fminf(floorf(fmaf(512.f, v[4 * g + k], 0.5f)), 255.f);
        word |= (unsigned int)r << (8 * k);
      }
      w[g] = word;
    }
    uint4* dst = reinterpret_cast<uint4*>(static_cast<unsigned char*>(out) + row * 128) + q;
    *dst = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    if (out_kind == PVS_DSIFT_F32_QUANT) {
#pragma unroll
      for (int k = 0; k < 16; ++k) v[k] = fminf(floorf(fmaf(512.f, v[k], 0.5f)), 255.f);
    }
    float4* dst = reinterpret_cast<float4*>(static_cast<float*>(out) + row * 128) + q * 4;
#pragma unroll
    for (int g = 0; g < 4; ++g) dst[g] = make_float4(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]);
  }
}

// taps[0 .. 2 radius] = exp(-d^2 / 2 sigma^2), d = -radius .. radius, summed ascending and normalised to sum 1 in float64
inline void gaussian_taps(double sigma, int radius, float* taps) {
  const auto g = [sigma](int d) { return std::exp(-(double)d * d / (2.0 * sigma * sigma)); };
  double sum = 0.0;
  for (int d = -radius; d <= radius; ++d) sum += g(d);
  for (int d = -radius; d <= radius; ++d) taps[d + radius] = (float)(g(d) / sum);
}

// The batch as both entry points take it: h_hw = (H, W) per image, h_pix_offsets = first element of each image in the pixel
// buffer or null for images packed back to back.  `what` starts every message ("dense SIFT" / "SIFT"), `entry` those about
// the call itself.  Limits that only one extractor has stay with that extractor.
struct ImageIntake {
  const char* what;
  const char* entry;
  const int32_t* hw;
  const int64_t* offs;
  int chan = 1;       // interleaved channels of the pixel kind
  int64_t pix = 0;    // elements in front of the next packed image

  int open(int pixel_kind, int out_kind, int64_t n_images) {
    if (pixel_kind < PVS_PIX_U8_RGB || pixel_kind > PVS_PIX_F32_GRAY) PVS_FAIL(PVS_ERR_INVALID, "%s: unknown pixel kind %d", what, pixel_kind);
    if (out_kind < PVS_DSIFT_U8 || out_kind > PVS_DSIFT_F32_QUANT) PVS_FAIL(PVS_ERR_INVALID, "%s: unknown output kind %d", what, out_kind);
    if (n_images < 0) PVS_FAIL(PVS_ERR_INVALID, "%s: negative image count", what);
    if (n_images > 0 && !hw) PVS_FAIL(PVS_ERR_INVALID, "%s: null image sizes", entry);
    chan = (pixel_kind == PVS_PIX_U8_RGB || pixel_kind == PVS_PIX_F32_RGB) ? 3 : 1;
    return PVS_OK;
  }
  // image i, in ascending i
  int next(int64_t i, int* H, int* W, int64_t* pix_off) {
    *H = hw[2 * i], *W = hw[2 * i + 1];
    if (*H < 1 || *W < 1) PVS_FAIL(PVS_ERR_INVALID, "%s: image %lld has size %d x %d", what, (long long)i, *H, *W);
    *pix_off = offs ? offs[i] : pix;
    if (*pix_off < 0) PVS_FAIL(PVS_ERR_INVALID, "%s: negative pixel offset", what);
    pix += (int64_t)*H * *W * chan;
    return PVS_OK;
  }
};

}  // namespace pvs
