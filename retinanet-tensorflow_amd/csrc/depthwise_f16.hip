// fp16-storage depthwise 3x3 for inference (rn_depthwise_fwd_f16, rn_hip.h): MobileNetV2's DepthwiseConv2D
// (mobilenet_v2.py:15-38) between the GroupNorms of its bottleneck (mobilenet_v2.py:57-73).  NHWC fp16 in and out, the fp32
// kernel [3,3,c] as the parameter is stored, fp32 accumulation, stride 1 or 2, TF SAME padding.
//
// Memory-bound: x is read once from memory (the taps' re-reads hit the caches), y is written once.  A block is 256 threads laid
// out as (pixel lane, channel octet) with the octet fastest, so the 16-byte loads of a wave are contiguous along the channel
// axis and, across pixel lanes, along w.  A thread owns ONE octet for the whole launch: its 72 weights and, with an input fold,
// its 8 (scale, shift) pairs sit in registers.  Its unit of work is a strip: P output pixels along w, R output rows tall.  It walks
// down the strip with a window of three input rows in registers (fp16, already folded): every output row loads S new input rows
// of (P - 1) S + 3 columns, so at stride 1 an input vector is loaded -- and its GroupNorm + activation formed -- 1.5 (R + 2) / R
// times per strip instead of 4.5 times, and feeds up to nine outputs from registers.  (The fold, not the nine multiply-adds, is
// the arithmetic that counts here: a conversion, an fma, the activation with its exponential, a conversion per element.)
//   input fold   x is the RAW output of the conv in front: act(GN(x)) is formed in fp32 and rounded to fp16 exactly as
//                rn_group_norm_apply_f16 stores it (the expression of conv3x3_sg32_f16_kernel's FIN = 1 path), zero at the padding
//                taps AFTER the activation
//   statistics   a block is one pixel chunk of one sample = one row of `partial` [2][n rows][c]: every thread sums y and y^2 of the
//                values as stored over its strips, the pixel lanes are folded by a fixed-order tree through LDS, no atomics
#include "rn_common.h"

namespace {
constexpr int T = 256;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

struct DwHArgs {
  const _Float16* x; const float* wgt; _Float16* y; float* partial;
  const float* in_mean; const float* in_rstd; const float* in_gamma; const float* in_beta;
  int in_groups, in_cpg, in_act;
  int n, h, w, c, c8, oh, ow, pad_t, pad_l;
  int pt;          // pixel lanes of a block: T / c8
  int tree;        // the power of two >= pt
  int rpt;         // output rows of a strip (R)
  int spr;         // strips side by side along w
  int strips;      // per sample: ceil(oh / R) * spr
  int rows;        // chunks per sample: a chunk is pt strips
};

template <int S, int P, bool FIN, bool FOUT>
__global__ __launch_bounds__(T) void dw_f16_kernel(const DwHArgs a) {
  constexpr int NW = (P - 1) * S + 3;                         // input columns of a strip
  __shared__ __attribute__((aligned(16))) float red[FOUT ? T * 16 : 1];
  const int tid = threadIdx.x;
  const int pl = tid / a.c8, oct = tid - pl * a.c8;
  const bool active = pl < a.pt;
  const int smp = blockIdx.x / a.rows, chunk = blockIdx.x - smp * a.rows;
  const int C = a.c, H = a.h, W = a.w, OW = a.ow;
  const int c0 = oct * 8;
  float wk[9][8];
  float sc[FIN ? 8 : 1], sh[FIN ? 8 : 1];
  float s1[FOUT ? 8 : 1], s2[FOUT ? 8 : 1];
  if (FOUT) {
#pragma unroll
    for (int i = 0; i < 8; ++i) { s1[i] = 0.f; s2[i] = 0.f; }
  }
  if (active) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const float4 lo = *reinterpret_cast<const float4*>(a.wgt + (size_t)t * C + c0);
      const float4 hi = *reinterpret_cast<const float4*>(a.wgt + (size_t)t * C + c0 + 4);
      wk[t][0] = lo.x; wk[t][1] = lo.y; wk[t][2] = lo.z; wk[t][3] = lo.w;
      wk[t][4] = hi.x; wk[t][5] = hi.y; wk[t][6] = hi.z; wk[t][7] = hi.w;
    }
    if (FIN) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {       // (an octet may straddle groups: the group of every channel on its own)
        const int c = c0 + i, g_ = c / a.in_cpg;
        const float scv = a.in_rstd[smp * a.in_groups + g_] * a.in_gamma[c];
        sc[i] = scv;
        sh[i] = a.in_beta[c] - a.in_mean[smp * a.in_groups + g_] * scv;
      }
    }
    const _Float16* __restrict__ xs = a.x + (size_t)smp * H * W * C + c0;
    _Float16* __restrict__ ys = a.y + (size_t)smp * a.oh * OW * C + c0;
    const int u = chunk * a.pt + pl;                        // strip of the sample
    if (u < a.strips) {
      const int ob = u / a.spr, ox0 = (u - ob * a.spr) * P;
      const int oy0 = ob * a.rpt, oy1 = min(oy0 + a.rpt, a.oh);
      const int ix0 = ox0 * S - a.pad_l;
      half8 win[3][NW];                                     // the input rows iy .. iy + 2 of the output row in hand
      auto load_row = [&](int iy, half8 (&dst)[NW]) {
        const bool rowok = (unsigned)iy < (unsigned)H;
#pragma unroll
        for (int j = 0; j < NW; ++j) {
          const int ix = ix0 + j;
          const bool ok = rowok && (unsigned)ix < (unsigned)W;
          half8 v = {};
          if (ok) v = *reinterpret_cast<const half8*>(xs + ((size_t)iy * W + ix) * C);
          if (FIN) {      // zero where the tap lies in the padding: SAME pads the ACTIVATED tensor
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = ok ? (_Float16)rn::act_fwd(fmaf((float)v[i], sc[i], sh[i]), a.in_act) : (_Float16)0.f;
          }
          dst[j] = v;
        }
      };
      int iy = oy0 * S - a.pad_t;
#pragma unroll
      for (int j = 0; j < 3 - S; ++j) load_row(iy + j, win[j]);
      for (int oy = oy0; oy < oy1; ++oy, iy += S) {
#pragma unroll
        for (int j = 3 - S; j < 3; ++j) load_row(iy + j, win[j]);
        float acc[P][8];
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[p][i] = 0.f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int p = 0; p < P; ++p)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
#pragma unroll
              for (int i = 0; i < 8; ++i) acc[p][i] = fmaf((float)win[kh][p * S + kw][i], wk[kh * 3 + kw][i], acc[p][i]);
#pragma unroll
        for (int p = 0; p < P; ++p) {
          if (ox0 + p < OW) {
            half8 o;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              o[i] = (_Float16)acc[p][i];
              if (FOUT) { const float fv = (float)o[i]; s1[i] += fv; s2[i] = fmaf(fv, fv, s2[i]); }
            }
            *reinterpret_cast<half8*>(ys + ((size_t)oy * OW + ox0 + p) * C) = o;
          }
        }
#pragma unroll
        for (int j = 0; j < 3 - S; ++j)                     // the rows the next output row shares with this one
#pragma unroll
          for (int jj = 0; jj < NW; ++jj) win[j][jj] = win[j + S][jj];
      }
    }
  }
  if (FOUT) {
    // pixel lanes folded pairwise, the same pairs in the same order at every launch; lanes beyond a.pt hold no sums and are never read
    float* mine = red + tid * 16;
#pragma unroll
    for (int i = 0; i < 8; ++i) { mine[i] = s1[i]; mine[8 + i] = s2[i]; }
    __syncthreads();
    for (int off = a.tree >> 1; off >= 1; off >>= 1) {
      if (active && pl < off && pl + off < a.pt) {
        const float* other = red + (tid + off * a.c8) * 16;
#pragma unroll
        for (int i = 0; i < 16; ++i) mine[i] += other[i];
      }
      __syncthreads();
    }
    if (pl == 0) {     // tid = oct < c8
      float* p1 = a.partial + (size_t)(smp * a.rows + chunk) * C + c0;
      float* p2 = p1 + (size_t)a.n * a.rows * C;
      *reinterpret_cast<float4*>(p1) = *reinterpret_cast<const float4*>(mine);
      *reinterpret_cast<float4*>(p1 + 4) = *reinterpret_cast<const float4*>(mine + 4);
      *reinterpret_cast<float4*>(p2) = *reinterpret_cast<const float4*>(mine + 8);
      *reinterpret_cast<float4*>(p2 + 4) = *reinterpret_cast<const float4*>(mine + 12);
    }
  }
}

// The ONE host decision of this file: rn_depthwise_fwd_f16 launches what this fills in, rn_depthwise_f16_plan reports it.
//   strip width P      stride 1: 4 outputs along w, stride 2: 2 (a window of 3 x 6 / 3 x 5 input vectors in registers); 1 where
//                      the output row is shorter than that
//   strip height R     4 output rows on maps of 32 rows and more, 2 from 8 rows on, else 1: small maps keep their parallelism
//   pixel lanes        256 / (c / 8): every thread one octet (c <= 2048)
//   chunk              the strips of a block's pixel lanes, one each (= one statistic row); a chunk never leaves its sample:
//                      the grid is n x rows_per_sample blocks, not capped
int decide(const rn_dw_f16* d, DwHArgs* a, rn_dw_f16_plan* pl) {
  *pl = rn_dw_f16_plan{};
  RN_CHECK_ARG(d, "depthwise f16: null descriptor");
  RN_CHECK_ARG(d->x && d->wgt && d->y, "depthwise f16: null pointer (x, wgt, y)");
  const int given = (d->in_mean != nullptr) + (d->in_rstd != nullptr) + (d->in_gamma != nullptr) + (d->in_beta != nullptr);
  RN_CHECK_ARG(given == 0 || given == 4, "depthwise f16: the input fold needs in_mean, in_rstd, in_gamma and in_beta (%d of 4 given)", given);
  RN_CHECK_ARG(d->n >= 1 && d->h >= 1 && d->w >= 1 && d->c >= 1, "depthwise f16: bad shape n=%d h=%d w=%d c=%d", d->n, d->h, d->w, d->c);
  RN_CHECK_ARG(d->c % 8 == 0, "depthwise f16: c=%d must be a multiple of 8", d->c);
  RN_CHECK_ARG(d->stride == 1 || d->stride == 2, "depthwise f16: stride=%d (1 or 2)", d->stride);
  if (given) {
    RN_CHECK_ARG(d->in_groups >= 1 && d->c % d->in_groups == 0, "depthwise f16: in_groups=%d does not divide c=%d", d->in_groups, d->c);
    RN_CHECK_ARG(d->in_act >= RN_ACT_NONE && d->in_act <= RN_ACT_SIGMOID, "depthwise f16: unknown in_act=%d", d->in_act);
  } else {
    RN_CHECK_ARG(d->in_groups == 0 && d->in_act == 0, "depthwise f16: in_groups / in_act given without the input fold's pointers");
  }
  RN_CHECK_ARG(((uintptr_t)d->x & 15) == 0 && ((uintptr_t)d->y & 15) == 0 && ((uintptr_t)d->wgt & 15) == 0,
               "depthwise f16: x, wgt and y must be 16-byte aligned");
  RN_CHECK_ARG(((uintptr_t)d->partial & 15) == 0, "depthwise f16: partial must be 16-byte aligned");
  RN_CHECK_ARG((((uintptr_t)d->in_mean | (uintptr_t)d->in_rstd | (uintptr_t)d->in_gamma | (uintptr_t)d->in_beta) & 3) == 0,
               "depthwise f16: in_mean, in_rstd, in_gamma and in_beta must be 4-byte aligned");
  RN_UNSUPPORTED(d->k != 3, "depthwise f16: k=%d (3 x 3 only)", d->k);
  RN_UNSUPPORTED(d->c > 2048, "depthwise f16: c=%d above 2048", d->c);
  RN_UNSUPPORTED((double)d->n * d->h * d->w * d->c >= 2147483648.0, "depthwise f16: tensors of 2^31 elements and more are not supported");
  a->x = (const _Float16*)d->x; a->wgt = d->wgt; a->y = (_Float16*)d->y; a->partial = d->partial;
  a->in_mean = d->in_mean; a->in_rstd = d->in_rstd; a->in_gamma = d->in_gamma; a->in_beta = d->in_beta;
  a->in_groups = d->in_groups; a->in_cpg = given ? d->c / d->in_groups : 1; a->in_act = d->in_act;
  a->n = d->n; a->h = d->h; a->w = d->w; a->c = d->c; a->c8 = d->c / 8;
  rn::same_pad(d->h, 3, d->stride, &a->oh, &a->pad_t);
  rn::same_pad(d->w, 3, d->stride, &a->ow, &a->pad_l);
  const int wide = d->stride == 1 ? 4 : 2;
  const int P = a->ow >= wide ? wide : 1;
  a->rpt = a->oh >= 32 ? 4 : a->oh >= 8 ? 2 : 1;
  a->pt = T / a->c8;
  a->tree = 1;
  while (a->tree < a->pt) a->tree *= 2;
  a->spr = rn::ceil_div(a->ow, P);
  a->strips = rn::ceil_div(a->oh, a->rpt) * a->spr;
  a->rows = rn::ceil_div(a->strips, a->pt);
  RN_UNSUPPORTED((double)d->n * a->rows >= 2147483648.0, "depthwise f16: grid too large");
  pl->oh = a->oh; pl->ow = a->ow; pl->pad_t = a->pad_t; pl->pad_l = a->pad_l;
  pl->kernel = d->stride == 1 ? RN_DW_F16_S1 : RN_DW_F16_S2;
  pl->pixels_per_thread = P;
  pl->pixel_lanes = a->pt;
  pl->rows_per_thread = a->rpt;
  pl->strips_per_sample = a->strips;
  pl->strips_per_chunk = a->pt;
  pl->pixels_per_chunk = a->pt * P * a->rpt;
  pl->rows_per_sample = a->rows;
  pl->blocks = d->n * a->rows;
  pl->fold = given ? 1 : 0;
  pl->stats = d->partial ? 1 : 0;
  return RN_OK;
}

template <int S, int P>
void launch(const DwHArgs& a, const rn_dw_f16_plan& pl, hipStream_t st) {
  const dim3 grid((unsigned)pl.blocks), block(T);
  if (pl.fold) {
    if (pl.stats) hipLaunchKernelGGL((dw_f16_kernel<S, P, true, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((dw_f16_kernel<S, P, true, false>), grid, block, 0, st, a);
  } else {
    if (pl.stats) hipLaunchKernelGGL((dw_f16_kernel<S, P, false, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((dw_f16_kernel<S, P, false, false>), grid, block, 0, st, a);
  }
}
}  // namespace

extern "C" int rn_depthwise_f16_plan(const rn_dw_f16* d, rn_dw_f16_plan* plan) {
  RN_CHECK_ARG(plan, "depthwise f16 plan: null plan");
  DwHArgs a = {};
  return decide(d, &a, plan);
}

extern "C" int rn_depthwise_f16_rows(int n, int h, int w, int c, int stride) {
  static const uint64_t word[2] __attribute__((aligned(16))) = {0, 0};      // (the decision only compares the pointers with NULL)
  rn_dw_f16 d = {};
  d.x = word; d.wgt = (const float*)word; d.y = (void*)word;
  d.n = n; d.h = h; d.w = w; d.c = c; d.k = 3; d.stride = stride;
  DwHArgs a = {};
  rn_dw_f16_plan pl;
  return decide(&d, &a, &pl) == RN_OK ? pl.rows_per_sample : 0;
}

extern "C" int rn_depthwise_fwd_f16(const rn_dw_f16* d, rn_stream_t stream) {
  DwHArgs a = {};
  rn_dw_f16_plan pl;
  if (int e = decide(d, &a, &pl)) return e;
  hipStream_t st = (hipStream_t)stream;
  if (pl.kernel == RN_DW_F16_S1) {
    if (pl.pixels_per_thread == 4) launch<1, 4>(a, pl, st);
    else launch<1, 1>(a, pl, st);
  } else {
    if (pl.pixels_per_thread == 2) launch<2, 2>(a, pl, st);
    else launch<2, 1>(a, pl, st);
  }
  RN_LAUNCH_CHECK();
  return RN_OK;
}
