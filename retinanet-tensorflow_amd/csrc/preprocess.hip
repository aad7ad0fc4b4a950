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

// the pair of ONE sample, by the blocks (bx of nbx) that share it: the single-image kernel and the batched one run this body
__device__ __forceinline__ void resize_pair_u8_body(const PairArgs& a, unsigned bx, unsigned nbx) {
  const int h = a.desc->h, w = a.desc->w;
  const float hs = a.desc->hs, ws = a.desc->ws;
  const int64_t total = (int64_t)a.oh * a.ow;
  const int64_t plane = total * 3;
  for (int64_t i = (int64_t)bx * 256 + threadIdx.x; i < total; i += (int64_t)nbx * 256) {
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

__global__ __launch_bounds__(256) void resize_pair_u8_kernel(const PairArgs a) { resize_pair_u8_body(a, blockIdx.x, gridDim.x); }

// K samples in one launch, grid (output pixel blocks of one sample, sample): sample i is a PairArgs of its own -- raw slot i of
// `cap` bytes (the slot stride, which is also its read bound), descriptor i, slots 2i / 2i+1 of the output -- run through the
// single-image body.
__global__ __launch_bounds__(256) void resize_pair_u8_batch_kernel(const PairArgs first) {
  const int64_t s = blockIdx.y;
  PairArgs a = first;
  a.raw += s * a.cap;
  a.desc += s;
  a.y += s * 2 * ((int64_t)a.oh * a.ow * 3);
  resize_pair_u8_body(a, blockIdx.x, gridDim.x);
}

constexpr int PAIR_BATCH_MAX = 65535;   // samples per launch: gridDim.y
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

extern "C" int rn_resize_pair_u8_batch(const uint8_t* raw, int64_t sample_stride_bytes, const rn_resize_desc* desc, int k,
                                       float* pairs, int oh, int ow, const float* mean, const float* stdv, rn_stream_t stream) {
  RN_CHECK_ARG(raw && desc && pairs && sample_stride_bytes >= 3 && oh >= 1 && ow >= 1, "resize_pair_u8_batch: bad argument");
  RN_CHECK_ARG(k >= 1 && k <= PAIR_BATCH_MAX, "resize_pair_u8_batch: k = %d (1 .. %d samples)", k, PAIR_BATCH_MAX);
  RN_CHECK_ARG((mean == nullptr) == (stdv == nullptr), "resize_pair_u8_batch: mean and std go together");
  PairArgs a = {};
  a.raw = raw; a.cap = sample_stride_bytes; a.desc = desc; a.y = pairs; a.oh = oh; a.ow = ow;
  a.normalize = mean ? 1 : 0;
  for (int i = 0; i < 3 && mean; ++i) { a.mean[i] = mean[i]; a.stdv[i] = stdv[i]; }
  const int64_t total = (int64_t)oh * ow;
  int64_t b = (total + 255) / 256;      // per sample: the single-image grid, so every thread meets the pixels it meets there
  if (b > 16384) b = 16384;
  hipLaunchKernelGGL(resize_pair_u8_batch_kernel, dim3((unsigned)b, (unsigned)k), dim3(256), 0, (hipStream_t)stream, a);
  RN_LAUNCH_CHECK();
  return RN_OK;
}

// ---------------------------------------------------------------------------------------------------------------- augmented pair
// Training-time augmentation of the ragged pair (the transforms the reference names and leaves as a TODO in augment_sample,
// dataset.py:206-212, asked for by train_input_fn's augment=True, train.py:190-198).  TensorFlow's kernels are not the yardstick
// here (the reference has no live code): THE CONTRACT IS THIS COMMENT.  For one sample, with a crop window (y0, x0, ch, cw) in raw
// pixels, a contrast factor f > 0, a brightness delta d, a saturation factor k >= 0 and the output size (oh, ow):
//   1. r = the pipeline of resize_pair_u8_kernel applied to raw[y0:y0+ch, x0:x0+cw]: convert_image_dtype (* 1/255), bilinear
//      resize with align_corners=True to (oh, ow), operation for operation.  hs = (ch-1)/(oh-1), ws = (cw-1)/(ow-1) come from the
//      descriptor (fp32, computed on the host); the window offset is added to the INTEGER indices only; index clamps are to the
//      window; reads stay inside raw[0, raw_capacity) whatever the descriptor holds.
//   2. contrast: m_c = mean of r[..., c] over the oh*ow pixels, accumulated in fp64, rounded once to fp32;
//      a = (r - m_c) * f + m_c            (f == 1: a = r, not the formula -- (r - m) * 1 + m is no identity in fp32)
//   3. brightness and clip: b = clamp(a + d, 0, 1)
//   4. saturation, closed form, no hue: M = max_c b, n = min_c b;  M == n: s = b;  else s_c = M - (M - b_c) * min(k, M / (M - n))
//      (k == 1: s = b, not the formula, for the same reason).  This is HSV with S scaled by k and clamped to 1:
//        V = M, S = (M - n) / M, and every channel is b_c = V - V S g_c with g_c = (M - b_c) / (M - n) a function of the hue alone;
//        S' = min(k S, 1) gives s_c = M - M S' g_c = M - (M - b_c) S'/S, and S'/S = min(k, 1/S) = min(k, M / (M - n)).
//   5. (s - MEAN) / STD when normalising
//   6. slot 0 at (oy, ox), slot 1 at (oy, ow-1-ox): both halves of the pair get the same parameters (the reference would apply
//      augment_sample to the stacked pair, and the flipped image has the same channel means).
// With the full window and f = 1, d = 0, k = 1 the result is rn_resize_pair_u8's bit for bit (r lies in [0, 1], so the clip
// changes nothing); with only a window it is rn_resize_pair_u8 of a contiguous copy of the crop.
//
// Two launches, because the contrast needs the mean of the whole resized image before any pixel can be written and nothing here
// waits grid-wide: (1) augment_stats_kernel -- block j covers the fixed pixel range [j * ppb, (j+1) * ppb) and leaves three fp64
// channel sums in partial[3j..3j+2]: every thread adds its pixels in a fixed order, the block adds its threads in a fixed tree;
// (2) augment_apply_kernel -- every block adds the partials in index order (the same value in every block), then steps 2-6.  No
// atomics, nothing to zero between replays: bit-identical run to run and graph to eager.  The grids depend on (oh, ow) only and
// everything else is read from the device descriptor, so one capture serves every raw size, window and parameter draw.
namespace {
constexpr int AUG_MAX_BLOCKS = 256;      // partial sums (and stats blocks) at most: the apply pass re-adds all of them per block
constexpr int AUG_STATS_THREADS = 256;

struct AugArgs {
  const uint8_t* raw; int64_t cap;
  const rn_augment_desc* desc;
  float* y;
  double* partial;
  int oh, ow, normalize, nblk;
  int64_t ppb;                          // pixels per stats block (a multiple of AUG_STATS_THREADS, see aug_geometry)
  float mean[3], stdv[3];
};

// r of one output pixel: resize_pair_u8_kernel's arithmetic with the window's size in the clamps and its origin in the indices
__device__ __forceinline__ void aug_resized(const AugArgs& a, int oy, int ox, float r[3]) {
  const rn_augment_desc* q = a.desc;
  const int w = q->w, wy = q->y0, wx = q->x0, ch = q->ch, cw = q->cw;
  const float iny = (float)oy * q->hs, inx = (float)ox * q->ws;
  const float fy = floorf(iny), fx = floorf(inx);
  const int y0 = min(max((int)fy, 0), ch - 1), x0 = min(max((int)fx, 0), cw - 1);
  const int y1 = max(min((int)ceilf(iny), ch - 1), 0), x1 = max(min((int)ceilf(inx), cw - 1), 0);
  const float yl = iny - fy, xl = inx - fx;
  const int64_t r0 = ((int64_t)wy + y0) * w + wx, r1 = ((int64_t)wy + y1) * w + wx;
  const int64_t itl = (r0 + x0) * 3, itr = (r0 + x1) * 3, ibl = (r1 + x0) * 3, ibr = (r1 + x1) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float tl = fetch_u8(a.raw, a.cap, itl + c), tr = fetch_u8(a.raw, a.cap, itr + c);
    const float bl = fetch_u8(a.raw, a.cap, ibl + c), br = fetch_u8(a.raw, a.cap, ibr + c);
    const float top = tl + (tr - tl) * xl;
    const float bot = bl + (br - bl) * xl;
    r[c] = top + (bot - top) * yl;
  }
}

// (measured 11.0 us at 375 x 500 -> 512 x 683 with these 256-thread blocks, profiles/augment_cost.txt; larger blocks for the
// <= AUG_MAX_BLOCKS ranges are untried)
__device__ __forceinline__ void augment_stats_body(const AugArgs& a, unsigned bx) {
  __shared__ double red[3][AUG_STATS_THREADS];
  const int64_t total = (int64_t)a.oh * a.ow;
  const int64_t lo = (int64_t)bx * a.ppb;
  const int64_t hi = min(lo + a.ppb, total);
  if (a.desc->f == 1.0f) return;         // (uniform) no contrast: the apply pass does not read the sums
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += AUG_STATS_THREADS) {
    float r[3];
    aug_resized(a, (int)(i / a.ow), (int)(i % a.ow), r);
    s0 += (double)r[0]; s1 += (double)r[1]; s2 += (double)r[2];
  }
  red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
  __syncthreads();
  for (int step = AUG_STATS_THREADS / 2; step >= 1; step >>= 1) {
    if ((int)threadIdx.x < step) {
#pragma unroll
      for (int c = 0; c < 3; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + step];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) a.partial[(int64_t)bx * 3 + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(AUG_STATS_THREADS) void augment_stats_kernel(const AugArgs a) { augment_stats_body(a, blockIdx.x); }

__device__ __forceinline__ void augment_apply_body(const AugArgs& a, unsigned bx, unsigned nbx) {
  __shared__ double part[3 * AUG_MAX_BLOCKS];
  __shared__ float mean_c[3];
  const int64_t total = (int64_t)a.oh * a.ow;
  const float f = a.desc->f, d = a.desc->d, k = a.desc->k;
  if (f != 1.0f) {                       // (uniform over the grid: the descriptor is one value for all threads)
    for (int i = threadIdx.x; i < 3 * a.nblk; i += 256) part[i] = a.partial[i];
    __syncthreads();
    if (threadIdx.x < 3) {
      double s = 0.0;
      for (int j = 0; j < a.nblk; ++j) s += part[3 * j + threadIdx.x];      // index order
      mean_c[threadIdx.x] = (float)(s / (double)total);                     // the one rounding to fp32
    }
    __syncthreads();
  }
  const int64_t plane = total * 3;
  for (int64_t i = (int64_t)bx * 256 + threadIdx.x; i < total; i += (int64_t)nbx * 256) {
    const int ox = (int)(i % a.ow), oy = (int)(i / a.ow);
    float v[3];
    aug_resized(a, oy, ox, v);
    if (f != 1.0f) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = (v[c] - mean_c[c]) * f + mean_c[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float t = v[c] + d;
      v[c] = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
    }
    const float M = fmaxf(fmaxf(v[0], v[1]), v[2]), n = fminf(fminf(v[0], v[1]), v[2]);
    if (k != 1.0f && M != n) {
      const float t = fminf(k, M / (M - n));
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = M - (M - v[c]) * t;
    }
    float* o0 = a.y + i * 3;
    float* o1 = a.y + plane + ((int64_t)oy * a.ow + (a.ow - 1 - ox)) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float u = v[c];
      if (a.normalize) u = (u - a.mean[c]) / a.stdv[c];
      o0[c] = u;
      o1[c] = u;
    }
  }
}

__global__ __launch_bounds__(256) void augment_apply_kernel(const AugArgs a) { augment_apply_body(a, blockIdx.x, gridDim.x); }

// K samples per launch, grids (blocks of one sample, sample): sample i is an AugArgs of its own -- raw slot i of `cap` bytes,
// descriptor i, its own nblk partial sums, slots 2i / 2i+1 -- run through the single-image bodies.  The sums of a sample are
// formed by its own stats blocks and read by its own apply blocks only: nothing is added across samples.
__device__ __forceinline__ AugArgs aug_sample(const AugArgs& first, int64_t s) {
  AugArgs a = first;
  a.raw += s * a.cap;
  a.desc += s;
  a.partial += s * 3 * a.nblk;
  a.y += s * 2 * ((int64_t)a.oh * a.ow * 3);
  return a;
}

__global__ __launch_bounds__(AUG_STATS_THREADS) void augment_stats_batch_kernel(const AugArgs first) {
  augment_stats_body(aug_sample(first, blockIdx.y), blockIdx.x);
}

__global__ __launch_bounds__(256) void augment_apply_batch_kernel(const AugArgs first) {
  augment_apply_body(aug_sample(first, blockIdx.y), blockIdx.x, gridDim.x);
}

// stats blocks of (oh, ow): 1024 pixels each (four strides of a block's 256 threads), or -- beyond AUG_MAX_BLOCKS of those --
// ceil(total / AUG_MAX_BLOCKS) rounded up to a multiple of 256, i.e. to whole strides
void aug_geometry(int oh, int ow, int* nblk, int64_t* ppb) {
  const int64_t total = (int64_t)oh * ow;
  int64_t p = 1024;
  if ((total + p - 1) / p > AUG_MAX_BLOCKS) p = ((total + AUG_MAX_BLOCKS - 1) / AUG_MAX_BLOCKS + 255) / 256 * 256;
  *ppb = p;
  *nblk = (int)((total + p - 1) / p);
}
}  // namespace

extern "C" size_t rn_resize_pair_u8_augment_workspace(int oh, int ow) {
  if (oh < 1 || ow < 1) return 0;
  int nblk; int64_t ppb;
  aug_geometry(oh, ow, &nblk, &ppb);
  return (size_t)nblk * 3 * sizeof(double);
}

extern "C" int rn_resize_pair_u8_augment(const uint8_t* raw, int64_t raw_capacity, const rn_augment_desc* desc, float* pair,
                                         int oh, int ow, const float* mean, const float* stdv, void* workspace,
                                         size_t workspace_bytes, rn_stream_t stream) {
  RN_CHECK_ARG(raw && desc && pair && workspace && raw_capacity >= 3 && oh >= 1 && ow >= 1, "resize_pair_u8_augment: bad argument");
  RN_CHECK_ARG((mean == nullptr) == (stdv == nullptr), "resize_pair_u8_augment: mean and std go together");
  RN_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && workspace_bytes >= rn_resize_pair_u8_augment_workspace(oh, ow),
               "resize_pair_u8_augment: workspace of %zu bytes, need %zu (8-byte aligned)", workspace_bytes,
               rn_resize_pair_u8_augment_workspace(oh, ow));
  AugArgs a = {};
  a.raw = raw; a.cap = raw_capacity; a.desc = desc; a.y = pair; a.partial = (double*)workspace; a.oh = oh; a.ow = ow;
  aug_geometry(oh, ow, &a.nblk, &a.ppb);
  a.normalize = mean ? 1 : 0;
  for (int i = 0; i < 3 && mean; ++i) { a.mean[i] = mean[i]; a.stdv[i] = stdv[i]; }
  hipLaunchKernelGGL(augment_stats_kernel, dim3((unsigned)a.nblk), dim3(AUG_STATS_THREADS), 0, (hipStream_t)stream, a);
  RN_LAUNCH_CHECK();
  const int64_t total = (int64_t)oh * ow;
  int64_t b = (total + 255) / 256;
  if (b > 16384) b = 16384;
  hipLaunchKernelGGL(augment_apply_kernel, dim3((unsigned)b), dim3(256), 0, (hipStream_t)stream, a);
  RN_LAUNCH_CHECK();
  return RN_OK;
}

extern "C" size_t rn_resize_pair_u8_augment_batch_workspace(int k, int oh, int ow) {
  if (k < 1 || k > PAIR_BATCH_MAX) return 0;
  return (size_t)k * rn_resize_pair_u8_augment_workspace(oh, ow);
}

extern "C" int rn_resize_pair_u8_augment_batch(const uint8_t* raw, int64_t sample_stride_bytes, const rn_augment_desc* desc, int k,
                                               float* pairs, int oh, int ow, const float* mean, const float* stdv, void* workspace,
                                               size_t workspace_bytes, rn_stream_t stream) {
  RN_CHECK_ARG(raw && desc && pairs && workspace && sample_stride_bytes >= 3 && oh >= 1 && ow >= 1,
               "resize_pair_u8_augment_batch: bad argument");
  RN_CHECK_ARG(k >= 1 && k <= PAIR_BATCH_MAX, "resize_pair_u8_augment_batch: k = %d (1 .. %d samples)", k, PAIR_BATCH_MAX);
  RN_CHECK_ARG((mean == nullptr) == (stdv == nullptr), "resize_pair_u8_augment_batch: mean and std go together");
  RN_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && workspace_bytes >= rn_resize_pair_u8_augment_batch_workspace(k, oh, ow),
               "resize_pair_u8_augment_batch: workspace of %zu bytes, need %zu (8-byte aligned)", workspace_bytes,
               rn_resize_pair_u8_augment_batch_workspace(k, oh, ow));
  AugArgs a = {};
  a.raw = raw; a.cap = sample_stride_bytes; a.desc = desc; a.y = pairs; a.partial = (double*)workspace; a.oh = oh; a.ow = ow;
  aug_geometry(oh, ow, &a.nblk, &a.ppb);
  a.normalize = mean ? 1 : 0;
  for (int i = 0; i < 3 && mean; ++i) { a.mean[i] = mean[i]; a.stdv[i] = stdv[i]; }
  hipLaunchKernelGGL(augment_stats_batch_kernel, dim3((unsigned)a.nblk, (unsigned)k), dim3(AUG_STATS_THREADS), 0,
                     (hipStream_t)stream, a);
  RN_LAUNCH_CHECK();
  const int64_t total = (int64_t)oh * ow;
  int64_t b = (total + 255) / 256;      // per sample: the single-image grid
  if (b > 16384) b = 16384;
  hipLaunchKernelGGL(augment_apply_batch_kernel, dim3((unsigned)b, (unsigned)k), dim3(256), 0, (hipStream_t)stream, a);
  RN_LAUNCH_CHECK();
  return RN_OK;
}
