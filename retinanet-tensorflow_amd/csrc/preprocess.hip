// Input pipeline on the device: convert_image_dtype (uint8 -> [0,1] float), bilinear resize with
// align_corners=True (dataset.py:145-151 rescale_image -> tf.image.resize_images, the ResizeBilinear kernel with
// half_pixel_centers = false) and the mean / std normalisation of train.py:48-49, fused in one pass.
// Compiled with -ffp-contract=off: every operation rounds separately, in the order of the TF kernel
//   in = dst * scale;  lo = floor(in);  hi = min(ceil(in), size-1);  lerp = in - lo
//   top = tl + (tr - tl) * xl;  bot = bl + (br - bl) * xl;  out = top + (bot - top) * yl
// HBM-bound: 4 gathered reads (cached) + 1 write per output element.
#include "rn_common.h"

namespace {
struct ResizeArgs {
  const void* x; float* y;
  int n, h, w, c, oh, ow, in_u8, normalize;
  float hs, ws;  // (in-1)/(out-1) with align_corners, 0 when out == 1
  float mean[8], stdv[8];
};

__device__ __forceinline__ float fetch(const ResizeArgs& a, size_t idx) {
  if (a.in_u8) return (float)reinterpret_cast<const uint8_t*>(a.x)[idx] * (1.0f / 255.0f);  // convert_image_dtype
  return reinterpret_cast<const float*>(a.x)[idx];
}

__global__ __launch_bounds__(256) void resize_bilinear_kernel(const ResizeArgs a) {
  const int64_t total = (int64_t)a.n * a.oh * a.ow * a.c;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    int64_t q = i;
    const int ch = (int)(q % a.c); q /= a.c;
    const int ox = (int)(q % a.ow); q /= a.ow;
    const int oy = (int)(q % a.oh);
    const int n_ = (int)(q / a.oh);
    const float iny = (float)oy * a.hs, inx = (float)ox * a.ws;
    const float fy = floorf(iny), fx = floorf(inx);
    const int y0 = max((int)fy, 0), x0 = max((int)fx, 0);
    const int y1 = min((int)ceilf(iny), a.h - 1), x1 = min((int)ceilf(inx), a.w - 1);
    const float yl = iny - fy, xl = inx - fx;
    const size_t base = (size_t)n_ * a.h * a.w;
    const float tl = fetch(a, ((base + (size_t)y0 * a.w + x0) * a.c) + ch), tr = fetch(a, ((base + (size_t)y0 * a.w + x1) * a.c) + ch);
    const float bl = fetch(a, ((base + (size_t)y1 * a.w + x0) * a.c) + ch), br = fetch(a, ((base + (size_t)y1 * a.w + x1) * a.c) + ch);
    const float top = tl + (tr - tl) * xl;
    const float bot = bl + (br - bl) * xl;
    float v = top + (bot - top) * yl;
    if (a.normalize) v = (v - a.mean[ch]) / a.stdv[ch];
    a.y[i] = v;
  }
}
}  // namespace

extern "C" int rn_resize_bilinear_normalize(const void* x, int in_u8, float* y, int n, int h, int w, int c, int oh, int ow,
                                            const float* mean, const float* stdv, rn_stream_t stream) {
  RN_CHECK_ARG(x && y && n >= 1 && h >= 1 && w >= 1 && c >= 1 && oh >= 1 && ow >= 1, "resize: bad argument");
  RN_UNSUPPORTED(c > 8, "resize: c = %d (at most 8 channels)", c);
  RN_CHECK_ARG((mean == nullptr) == (stdv == nullptr), "resize: mean and std go together");
  ResizeArgs a = {};
  a.x = x; a.y = y; a.n = n; a.h = h; a.w = w; a.c = c; a.oh = oh; a.ow = ow; a.in_u8 = in_u8 ? 1 : 0;
  a.hs = oh > 1 ? (float)(h - 1) / (float)(oh - 1) : 0.f;
  a.ws = ow > 1 ? (float)(w - 1) / (float)(ow - 1) : 0.f;
  a.normalize = mean ? 1 : 0;
  for (int i = 0; i < c && mean; ++i) { a.mean[i] = mean[i]; a.stdv[i] = stdv[i]; }
  const int64_t total = (int64_t)n * oh * ow * c;
  int64_t b = (total + 255) / 256;
  if (b > 16384) b = 16384;
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3((unsigned)b), dim3(256), 0, (hipStream_t)stream, a);
  RN_LAUNCH_CHECK();
  return RN_OK;
}

// ---------------------------------------------------------------------------------------------------------------- ragged pair
// One pass from a raw uint8 [h, w, 3] image of any size (read from a device descriptor at run time) to the reference's batch of
// two [image, hflip(image)] (dataset.py:182-204, augmentation.py:5-22): the arithmetic of resize_bilinear_kernel, channel by
// channel, one work item per output pixel, written to slot 0 at (oy, ox) and to slot 1 at (oy, ow-1-ox).  Since h, w, hs, ws
// come from `desc`, one captured graph serves every raw size that maps to the same (oh, ow).  Every read is bounded by
// raw_capacity: a bad descriptor gives wrong pixels, never an access outside the buffer.
namespace {
struct PairArgs {
  const uint8_t* raw; int64_t cap;
  const rn_resize_desc* desc;
  float* y;
  int oh, ow, normalize;
  float mean[3], stdv[3];
};

__device__ __forceinline__ float fetch_u8(const uint8_t* raw, int64_t cap, int64_t idx) {
  return (idx >= 0 && idx < cap) ? (float)raw[idx] * (1.0f / 255.0f) : 0.0f;  // convert_image_dtype
}

__global__ __launch_bounds__(256) void resize_pair_u8_kernel(const PairArgs a) {
  const int h = a.desc->h, w = a.desc->w;
  const float hs = a.desc->hs, ws = a.desc->ws;
  const int64_t total = (int64_t)a.oh * a.ow;
  const int64_t plane = total * 3;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int ox = (int)(i % a.ow), oy = (int)(i / a.ow);
    const float iny = (float)oy * hs, inx = (float)ox * ws;
    const float fy = floorf(iny), fx = floorf(inx);
    // the clamps to [0, size-1] change nothing for a valid descriptor (the TF index arithmetic stays inside the image)
    const int y0 = min(max((int)fy, 0), h - 1), x0 = min(max((int)fx, 0), w - 1);
    const int y1 = max(min((int)ceilf(iny), h - 1), 0), x1 = max(min((int)ceilf(inx), w - 1), 0);
    const float yl = iny - fy, xl = inx - fx;
    const int64_t r0 = (int64_t)y0 * w, r1 = (int64_t)y1 * w;
    const int64_t itl = (r0 + x0) * 3, itr = (r0 + x1) * 3, ibl = (r1 + x0) * 3, ibr = (r1 + x1) * 3;
    float* o0 = a.y + i * 3;
    float* o1 = a.y + plane + ((int64_t)oy * a.ow + (a.ow - 1 - ox)) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float tl = fetch_u8(a.raw, a.cap, itl + ch), tr = fetch_u8(a.raw, a.cap, itr + ch);
      const float bl = fetch_u8(a.raw, a.cap, ibl + ch), br = fetch_u8(a.raw, a.cap, ibr + ch);
      const float top = tl + (tr - tl) * xl;
      const float bot = bl + (br - bl) * xl;
      float v = top + (bot - top) * yl;
      if (a.normalize) v = (v - a.mean[ch]) / a.stdv[ch];
      o0[ch] = v;
      o1[ch] = v;
    }
  }
}
}  // namespace

extern "C" int rn_resize_pair_u8(const uint8_t* raw, int64_t raw_capacity, const rn_resize_desc* desc, float* pair, int oh,
                                 int ow, const float* mean, const float* stdv, rn_stream_t stream) {
  RN_CHECK_ARG(raw && desc && pair && raw_capacity >= 3 && oh >= 1 && ow >= 1, "resize_pair_u8: bad argument");
  RN_CHECK_ARG((mean == nullptr) == (stdv == nullptr), "resize_pair_u8: mean and std go together");
  PairArgs a = {};
  a.raw = raw; a.cap = raw_capacity; a.desc = desc; a.y = pair; a.oh = oh; a.ow = ow;
  a.normalize = mean ? 1 : 0;
  for (int i = 0; i < 3 && mean; ++i) { a.mean[i] = mean[i]; a.stdv[i] = stdv[i]; }
  const int64_t total = (int64_t)oh * ow;
  int64_t b = (total + 255) / 256;
  if (b > 16384) b = 16384;
  hipLaunchKernelGGL(resize_pair_u8_kernel, dim3((unsigned)b), dim3(256), 0, (hipStream_t)stream, a);
  RN_LAUNCH_CHECK();
  return RN_OK;
}
