// fp16-storage inference of the DenseNet-BC backbones (densenet.py:50-80 BottleneckCompositeFunction, :117-121 the growth concat,
// :124-151 TransitionLayer): the dense block on ONE fp16 buffer [n, hw, ld] and the transition's average pool.
//
//   rn_dense_f16_put       a dense [n, hw, c] tensor -> the channel slice [coff, coff + c) of the buffer, and in the same pass the
//                          sums of x and x^2 of the values as stored, per (sample, pixel chunk, channel), into the caller's table
//                          [2][n][rows][ld].  A chunk is CHUNK consecutive pixels of one sample, so rows = ceil(hw / CHUNK) depends
//                          on hw alone and every slice of a block lands in one layout.  The statistics of a channel never change
//                          once its slice is written: no layer of the block reads the prefix for statistics again.
//   rn_dense_f16_finalize  mean / rstd [n][groups] of the channel prefix [0, c) from the table: fp64, fixed order.  Group sizes are
//                          c / 32 = 2, 3, 4 ... 51 as the block grows, so a thread addresses single floats of the table.
//   rn_dense_f16_norm      a = act(GN(prefix)) from the buffer (row stride ld) into a dense [n, hw, c] fp16 tensor: the operand of
//                          the layer's 1 x 1 conv.  (scale, shift) per channel in LDS; the expression of gn_apply_f16x8_kernel.
//   rn_avgpool_gn_fwd_f16  2 x 2 / 2 average pool, TF SAME (the sum divided by the number of in-bounds cells, avgpool_fwd_kernel),
//                          optionally of act(GN(x)) of the raw x in one pass: every tap is formed in fp32 and rounded to fp16 as
//                          rn_group_norm_apply_f16 stores it, summed in fp32, scaled, rounded once -- bit-equal to the apply pass
//                          followed by the plain pool.
// All four are memory-bound: 16-byte vectors (8 halfs) along the channel axis, no atomics, every reduction in a fixed order.
#include "rn_common.h"

namespace {
constexpr int T = 256;
constexpr int CHUNK = 256;          // pixels per statistic row
constexpr int MAX_OB = 32;          // channel octets a put block spans (256 channels)
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

struct PutArgs {
  const _Float16* src; _Float16* buf; float* partial;
  int n, hw, c, c8, ld, coff, rows;
  int ob;           // octets per block (a power of two <= MAX_OB)
  int lanes;        // pixel lanes per block: T / ob
  int copy;         // 0: src == buf (the sums of a finished tensor): nothing is stored
};

// block = (chunk, sample, octet span); thread = (pixel lane, octet) with the octet fastest: a wave's 16-byte accesses are
// contiguous along the channel axis.  A lane walks the chunk's pixels lane, lane + lanes, ... in order; the lanes are folded
// pairwise through LDS, the same pairs in the same order at every launch.
__global__ __launch_bounds__(T) void dense_put_kernel(const PutArgs a) {
  __shared__ __attribute__((aligned(16))) float red[T * 16];
  const int tid = threadIdx.x;
  const int lane = tid / a.ob, oct = tid - lane * a.ob;
  const int chunk = blockIdx.x, smp = blockIdx.y;
  const int go = blockIdx.z * a.ob + oct;
  const bool active = go < a.c8;
  float s1[8], s2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { s1[i] = 0.f; s2[i] = 0.f; }
  if (active) {
    const int p0 = chunk * CHUNK, p1 = min(p0 + CHUNK, a.hw);
    const _Float16* src = a.src + (size_t)smp * a.hw * a.c + go * 8;
    _Float16* dst = a.buf + (size_t)smp * a.hw * a.ld + a.coff + go * 8;
#pragma unroll 4
    for (int p = p0 + lane; p < p1; p += a.lanes) {
      const half8 v = *reinterpret_cast<const half8*>(src + (size_t)p * a.c);
      if (a.copy) *reinterpret_cast<half8*>(dst + (size_t)p * a.ld) = v;
#pragma unroll
      for (int i = 0; i < 8; ++i) { const float f = (float)v[i]; s1[i] += f; s2[i] = fmaf(f, f, s2[i]); }
    }
  }
  float* mine = red + tid;          // component i of thread t at red[i * T + t]: a wave's accesses fall on consecutive banks
#pragma unroll
  for (int i = 0; i < 8; ++i) { mine[i * T] = s1[i]; mine[(8 + i) * T] = s2[i]; }
  __syncthreads();
  for (int off = a.lanes >> 1; off >= 1; off >>= 1) {
    if (lane < off) {
      const float* other = mine + off * a.ob;
#pragma unroll
      for (int i = 0; i < 16; ++i) mine[i * T] += other[i * T];
    }
    __syncthreads();
  }
  if (lane == 0 && active) {
    float* q1 = a.partial + ((size_t)smp * a.rows + chunk) * a.ld + a.coff + go * 8;
    float* q2 = q1 + (size_t)a.n * a.rows * a.ld;
    *reinterpret_cast<float4*>(q1) = make_float4(mine[0], mine[T], mine[2 * T], mine[3 * T]);
    *reinterpret_cast<float4*>(q1 + 4) = make_float4(mine[4 * T], mine[5 * T], mine[6 * T], mine[7 * T]);
    *reinterpret_cast<float4*>(q2) = make_float4(mine[8 * T], mine[9 * T], mine[10 * T], mine[11 * T]);
    *reinterpret_cast<float4*>(q2 + 4) = make_float4(mine[12 * T], mine[13 * T], mine[14 * T], mine[15 * T]);
  }
}

struct FinArgs { const float* partial; float* mean; float* rstd; int n, hw, c, ld, rows, groups, cpg; float eps; };

// block = (group, sample).  The group's sums are rows x cpg floats per plane; thread t takes the elements t, t + 256, ... (row
// major) in fp64, the threads are folded pairwise through LDS.
__global__ __launch_bounds__(T) void dense_finalize_kernel(const FinArgs a) {
  __shared__ double red[T][2];
  const int tid = threadIdx.x, g = blockIdx.x, smp = blockIdx.y;
  const float* __restrict__ p1 = a.partial + (size_t)smp * a.rows * a.ld + g * a.cpg;
  const float* __restrict__ p2 = p1 + (size_t)a.n * a.rows * a.ld;
  const int total = a.rows * a.cpg;
  double s1 = 0.0, s2 = 0.0;
  for (int e = tid; e < total; e += T) {
    const int r = e / a.cpg, j = e - r * a.cpg;
    const size_t at = (size_t)r * a.ld + j;
    s1 += (double)p1[at]; s2 += (double)p2[at];
  }
  red[tid][0] = s1; red[tid][1] = s2;
  __syncthreads();
  for (int off = T >> 1; off >= 1; off >>= 1) {
    if (tid < off) { red[tid][0] += red[tid + off][0]; red[tid][1] += red[tid + off][1]; }
    __syncthreads();
  }
  if (tid == 0) {
    const double m = (double)a.hw * (double)a.cpg;
    const double mean = red[0][0] / m;
    double var = red[0][1] / m - mean * mean;
    if (var < 0.0) var = 0.0;
    a.mean[smp * a.groups + g] = (float)mean;
    a.rstd[smp * a.groups + g] = (float)(1.0 / sqrt(var + (double)a.eps));
  }
}

struct NormArgs {
  const _Float16* buf; _Float16* y; const float* mean; const float* rstd; const float* gamma; const float* beta;
  int n, hw, c, c8, ld, groups, cpg, act;
};

// block.y = sample; grid-stride over (pixel, octet) with the octet fastest.  An octet may straddle groups (odd group sizes):
// every channel has its own (scale, shift).
__global__ __launch_bounds__(T) void dense_norm_kernel(const NormArgs a) {
  __shared__ float2 tab[2048];
  const int smp = blockIdx.y, tid = threadIdx.x;
  for (int c = tid; c < a.c; c += T) {
    const int g = c / a.cpg;
    const float sc = a.rstd[smp * a.groups + g] * a.gamma[c];
    tab[c] = make_float2(sc, a.beta[c] - a.mean[smp * a.groups + g] * sc);
  }
  __syncthreads();
  const _Float16* __restrict__ x = a.buf + (size_t)smp * a.hw * a.ld;
  _Float16* __restrict__ y = a.y + (size_t)smp * a.hw * a.c;
  const int64_t total = (int64_t)a.hw * a.c8;
#pragma unroll 2
  for (int64_t i = (int64_t)blockIdx.x * T + tid; i < total; i += (int64_t)gridDim.x * T) {
    const int p = (int)(i / a.c8);
    const int q = (int)(i - (int64_t)p * a.c8);
    const half8 v = *reinterpret_cast<const half8*>(x + (size_t)p * a.ld + q * 8);
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float2 t = tab[q * 8 + j];
      o[j] = (_Float16)rn::act_fwd(fmaf((float)v[j], t.x, t.y), a.act);
    }
    *reinterpret_cast<half8*>(y + (size_t)i * 8) = o;
  }
}

struct AvgArgs {
  const _Float16* x; _Float16* out; const float* mean; const float* rstd; const float* gamma; const float* beta;
  int n, h, w, c, oh, ow, groups, act;
};

// thread = (output pixel, 8 channels).  k = 2, stride 2: SAME pads at the bottom / right only, so window (oy, ox) is the in-bounds
// cells of rows 2 oy, 2 oy + 1 and columns 2 ox, 2 ox + 1, summed in that order (avgpool_fwd_kernel's).
template <bool GN>
__global__ __launch_bounds__(T) void avgpool_gn_f16_kernel(const AvgArgs a) {
  __shared__ float2 tab[GN ? 2048 : 1];
  const int smp = blockIdx.y, tid = threadIdx.x;
  if (GN) {
    const int cpg = a.c / a.groups;
    for (int c = tid; c < a.c; c += T) {
      const int g = c / cpg;
      const float sc = a.rstd[smp * a.groups + g] * a.gamma[c];
      tab[c] = make_float2(sc, a.beta[c] - a.mean[smp * a.groups + g] * sc);
    }
    __syncthreads();
  }
  const int C8 = a.c >> 3;
  const int64_t total = (int64_t)a.oh * a.ow * C8;
  const _Float16* __restrict__ x = a.x + (size_t)smp * a.h * a.w * a.c;
  _Float16* __restrict__ out = a.out + (size_t)smp * a.oh * a.ow * a.c;
  for (int64_t i = (int64_t)blockIdx.x * T + tid; i < total; i += (int64_t)gridDim.x * T) {
    const int q = (int)(i % C8);
    const int p = (int)(i / C8);
    const int ox = p % a.ow, oy = p / a.ow;
    float sum[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sum[j] = 0.f;
    int cnt = 0;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      const int ih = oy * 2 + kh;
      if (ih >= a.h) continue;
#pragma unroll
      for (int kw = 0; kw < 2; ++kw) {
        const int iw = ox * 2 + kw;
        if (iw >= a.w) continue;
        const half8 v = *reinterpret_cast<const half8*>(x + ((size_t)ih * a.w + iw) * a.c + q * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (GN) {
            const float2 t = tab[q * 8 + j];
            sum[j] += (float)(_Float16)rn::act_fwd(fmaf((float)v[j], t.x, t.y), a.act);   // the tap as the apply pass stores it
          } else {
            sum[j] += (float)v[j];
          }
        }
        ++cnt;
      }
    }
    const float inv = 1.f / (float)cnt;
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (_Float16)(sum[j] * inv);
    *reinterpret_cast<half8*>(out + (size_t)i * 8) = o;
  }
}

// blocks (per sample) of a grid-stride loop: at least four items per thread, and about 2048 blocks over the n samples (256 CUs x
// 8): every block rebuilds the (scale, shift) table of up to 2048 channels, so more, thinner blocks only repeat that work
unsigned stride_grid(int64_t items, int n) {
  int64_t b = (items + (int64_t)T * 4 - 1) / ((int64_t)T * 4);
  const int64_t cap = n >= 32 ? 64 : 2048 / n;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (unsigned)b;
}

// The ONE host decision of the three dense-block entry points: they launch what this fills in, rn_dense_f16_plan reports it.
int decide(int op, int n, int hw, int c, int ld, int coff, int groups, rn_dense_plan* pl) {
  RN_CHECK_ARG(pl, "dense f16: null plan");
  *pl = rn_dense_plan{};
  RN_CHECK_ARG(op == RN_DENSE_F16_PUT || op == RN_DENSE_F16_FINALIZE || op == RN_DENSE_F16_NORM, "dense f16: unknown op %d", op);
  RN_CHECK_ARG(n >= 1 && hw >= 1 && c >= 1 && ld >= 1 && coff >= 0, "dense f16: bad shape n=%d hw=%d c=%d ld=%d coff=%d", n, hw, c, ld, coff);
  RN_CHECK_ARG((int64_t)coff + c <= ld, "dense f16: the slice [%d, %d) does not fit ld=%d", coff, coff + c, ld);
  RN_UNSUPPORTED(c % 8 != 0, "dense f16: c=%d must be a multiple of 8", c);
  RN_UNSUPPORTED(ld % 8 != 0 || coff % 8 != 0, "dense f16: ld=%d and coff=%d must be multiples of 8", ld, coff);
  RN_UNSUPPORTED(n > 65535, "dense f16: n=%d above 65535", n);
  const int rows = rn::ceil_div(hw, CHUNK);
  if (op != RN_DENSE_F16_PUT) {
    RN_CHECK_ARG(coff == 0, "dense f16: finalize and norm take the prefix [0, c) (coff=%d)", coff);
    RN_CHECK_ARG(groups >= 1 && c % groups == 0, "dense f16: groups=%d does not divide c=%d", groups, c);
    RN_UNSUPPORTED(groups > 65535, "dense f16: groups=%d above 65535", groups);
    RN_UNSUPPORTED(op == RN_DENSE_F16_FINALIZE && (int64_t)rows * (c / groups) >= 2147483648LL, "dense f16 finalize: %d rows of %d channels per group",
                   rows, c / groups);
    RN_UNSUPPORTED(op == RN_DENSE_F16_NORM && c > 2048, "dense f16 norm: c=%d above 2048", c);
  } else {
    RN_UNSUPPORTED(c / 8 > 65535 * MAX_OB, "dense f16 put: c=%d too wide", c);
  }
  pl->op = op; pl->chunk = CHUNK; pl->rows = rows; pl->threads = T;      // (nothing below refuses: a refused call's plan stays zeroed)
  if (op == RN_DENSE_F16_PUT) {
    const int c8 = c / 8;
    int ob = 1;
    while (ob * 2 <= c8 && ob * 2 <= MAX_OB) ob *= 2;
    pl->vec = 8; pl->octets_per_block = ob; pl->lanes = T / ob;
    pl->grid_x = rows; pl->grid_y = n; pl->grid_z = rn::ceil_div(c8, ob);
  } else if (op == RN_DENSE_F16_FINALIZE) {
    pl->vec = 1; pl->grid_x = groups; pl->grid_y = n; pl->grid_z = 1;
  } else {
    pl->vec = 8; pl->grid_x = (int)stride_grid((int64_t)hw * (c / 8), n); pl->grid_y = n; pl->grid_z = 1;
  }
  return RN_OK;
}
}  // namespace

extern "C" int rn_dense_f16_rows(int hw) { return hw >= 1 ? rn::ceil_div(hw, CHUNK) : 0; }

extern "C" int rn_dense_f16_plan(int op, int n, int hw, int c, int ld, int coff, int groups, rn_dense_plan* plan) {
  return decide(op, n, hw, c, ld, coff, groups, plan);
}

extern "C" int rn_dense_f16_put(const void* src, void* buf, float* partial, int n, int hw, int c, int ld, int coff, rn_stream_t stream) {
  RN_CHECK_ARG(src && buf && partial, "dense f16 put: null pointer (src, buf, partial)");
  RN_CHECK_ARG((((uintptr_t)src | (uintptr_t)buf | (uintptr_t)partial) & 15) == 0, "dense f16 put: src, buf and partial must be 16-byte aligned");
  rn_dense_plan pl;
  if (int e = decide(RN_DENSE_F16_PUT, n, hw, c, ld, coff, 0, &pl)) return e;
  PutArgs a = {};
  a.src = (const _Float16*)src; a.buf = (_Float16*)buf; a.partial = partial;
  a.n = n; a.hw = hw; a.c = c; a.c8 = c / 8; a.ld = ld; a.coff = coff; a.rows = pl.rows; a.ob = pl.octets_per_block; a.lanes = pl.lanes; a.copy = src != buf;
  hipLaunchKernelGGL(dense_put_kernel, dim3((unsigned)pl.grid_x, (unsigned)pl.grid_y, (unsigned)pl.grid_z), dim3(T), 0, (hipStream_t)stream, a);
  RN_LAUNCH_CHECK();
  return RN_OK;
}

extern "C" int rn_dense_f16_finalize(const float* partial, int n, int hw, int c, int ld, int groups, float eps, float* mean, float* rstd,
                                     rn_stream_t stream) {
  RN_CHECK_ARG(partial && mean && rstd, "dense f16 finalize: null pointer (partial, mean, rstd)");
  rn_dense_plan pl;
  if (int e = decide(RN_DENSE_F16_FINALIZE, n, hw, c, ld, 0, groups, &pl)) return e;
  FinArgs a = {partial, mean, rstd, n, hw, c, ld, pl.rows, groups, c / groups, eps};
  hipLaunchKernelGGL(dense_finalize_kernel, dim3((unsigned)pl.grid_x, (unsigned)pl.grid_y), dim3(T), 0, (hipStream_t)stream, a);
  RN_LAUNCH_CHECK();
  return RN_OK;
}

extern "C" int rn_dense_f16_norm(const void* buf, void* y, int n, int hw, int c, int ld, int groups, const float* mean, const float* rstd,
                                 const float* gamma, const float* beta, int act, rn_stream_t stream) {
  RN_CHECK_ARG(buf && y && mean && rstd && gamma && beta, "dense f16 norm: null pointer (buf, y, mean, rstd, gamma, beta)");
  RN_CHECK_ARG((((uintptr_t)buf | (uintptr_t)y) & 15) == 0, "dense f16 norm: buf and y must be 16-byte aligned");
  RN_CHECK_ARG(act >= RN_ACT_NONE && act <= RN_ACT_SIGMOID, "dense f16 norm: unknown act=%d", act);
  rn_dense_plan pl;
  if (int e = decide(RN_DENSE_F16_NORM, n, hw, c, ld, 0, groups, &pl)) return e;
  NormArgs a = {};
  a.buf = (const _Float16*)buf; a.y = (_Float16*)y; a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta;
  a.n = n; a.hw = hw; a.c = c; a.c8 = c / 8; a.ld = ld; a.groups = groups; a.cpg = c / groups; a.act = act;
  hipLaunchKernelGGL(dense_norm_kernel, dim3((unsigned)pl.grid_x, (unsigned)pl.grid_y), dim3(T), 0, (hipStream_t)stream, a);
  RN_LAUNCH_CHECK();
  return RN_OK;
}

extern "C" int rn_avgpool_gn_fwd_f16(const void* x, void* y, int n, int h, int w, int c, int k, int stride, const float* mean,
                                     const float* rstd, const float* gamma, const float* beta, int groups, int act, rn_stream_t stream) {
  RN_CHECK_ARG(x && y, "avgpool gn fwd f16: null pointer (x, y)");
  RN_CHECK_ARG(n >= 1 && h >= 1 && w >= 1 && c >= 1, "avgpool gn fwd f16: bad shape n=%d h=%d w=%d c=%d", n, h, w, c);
  RN_CHECK_ARG((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "avgpool gn fwd f16: x and y must be 16-byte aligned");
  RN_UNSUPPORTED(k != 2 || stride != 2, "avgpool gn fwd f16: k=%d stride=%d (2 x 2 / 2 only)", k, stride);
  RN_UNSUPPORTED(c % 8 != 0, "avgpool gn fwd f16: c=%d must be a multiple of 8", c);
  RN_UNSUPPORTED(n > 65535, "avgpool gn fwd f16: n=%d above 65535", n);
  AvgArgs a = {};
  a.x = (const _Float16*)x; a.out = (_Float16*)y;
  a.n = n; a.h = h; a.w = w; a.c = c; a.oh = (h + 1) / 2; a.ow = (w + 1) / 2;
  const unsigned bx = stride_grid((int64_t)a.oh * a.ow * (c / 8), n);
  if (mean) {
    RN_CHECK_ARG(rstd && gamma && beta && groups >= 1 && c % groups == 0, "avgpool gn fwd f16: the GroupNorm needs rstd, gamma, beta and groups dividing c");
    RN_CHECK_ARG(act >= RN_ACT_NONE && act <= RN_ACT_SIGMOID, "avgpool gn fwd f16: unknown act=%d", act);
    RN_UNSUPPORTED(c > 2048, "avgpool gn fwd f16: c=%d above 2048 behind a GroupNorm", c);
    a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.beta = beta; a.groups = groups; a.act = act;
    hipLaunchKernelGGL(avgpool_gn_f16_kernel<true>, dim3(bx, (unsigned)n), dim3(T), 0, (hipStream_t)stream, a);
  } else {
    hipLaunchKernelGGL(avgpool_gn_f16_kernel<false>, dim3(bx, (unsigned)n), dim3(T), 0, (hipStream_t)stream, a);
  }
  RN_LAUNCH_CHECK();
  return RN_OK;
}
