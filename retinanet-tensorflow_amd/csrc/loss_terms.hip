// Classification loss as a weighted sum of the terms of the reference's classification_loss (losses.py:113-141), the list its
// author edits by commenting lines in and out; regression loss, #fg, masking rule and NaN rule exactly those of loss.hip.
// All sums run over the M trainable rows; p = sigmoid(z), per class I = sum l p, L = sum l, P = sum p:
//   bce          : mean_{M,C} bce(z, l)                                                                    (losses.py:124-125)
//   balanced_bce : (1/(M C)) sum_c (wp_c B1_c + wn_c B0_c), wp_c = (M - L_c)/M, wn_c = L_c/M,
//                  B1_c = sum_{l == 1} bce, B0_c = sum_{l != 1} bce                                        (losses.py:96-110, axis 0)
//   dice         : mean_c 1 - (2 I + s)/(L + P + s)                                                        (losses.py:50-60, axis 0)
//   fixed_iou    : mean_c 1 - (I + s)/D, D = L + P - I + s  (the reference's union L + sum (1 - l) p = L + P - I)  (losses.py:63-73)
//   jaccard      : mean_c (1 - (I + s)/D) s: fixed_iou times s -- ONE device term (smooth, scale) in two slots  (losses.py:37-47, axis 0)
//   focal        : sum focal / max(#fg, 1), focus 2, alpha 0.25, eps 1e-7                                  (losses.py:6-15, 119-122)
// focal_softmax_cross_entropy_with_logits (losses.py:18-34, marked "check if this is correct") is not covered.
//
// Same two layouts and the same fixed-order reduction as loss.hip (registers -> LDS -> one partial row per block -> fp64 sum ->
// fp64 finalize; no atomics: bitwise reproducible).  The term set and the weights are wave-uniform launch arguments: one
// instantiation per quads-per-lane count.  A partial row is NSCAL + 3 C floats, NSCAL + 5 C (then B1_c, B0_c) only in a launch
// with balanced_bce.  The gradient pass is elementwise given the statistics: every overlap term is p(1-p)(l A_c + B_c) and the
// balanced weights depend on the labels only, so a lane hoists four constants per class it owns.
// The descriptors {bce:1, dice:1:0} and {focal:1} run loss.hip's kernels (rn_loss_fwd / rn_loss_bwd): same bits, same cost.
#include <stdlib.h>

#include <cmath>

#include "rn_common.h"

namespace {

constexpr int T = 256;
constexpr int WAVES = T / 64;
constexpr int MAXJ = 4;          // classes per lane => C <= 256
constexpr int NSCAL = 5;         // M, fg, bce, focal, huber (loss.hip's)
constexpr int BLOCKS = 2048;
constexpr int RPW = 16;          // four-lane layout: rows per wave and pass
constexpr int H = RN_LOSS_STATS_HEADER;
constexpr uint32_t ALL_TERMS = RN_LT_BCE | RN_LT_BALANCED_BCE | RN_LT_DICE | RN_LT_JACCARD | RN_LT_FIXED_IOU | RN_LT_FOCAL;

struct LossSeg {
  const float* zl; const float* ll; const float* rp; const float* rl; const uint8_t* tm;
  float* dz; float* dr;
  int64_t rows; int64_t row_start;
};
struct TermsDev {
  uint32_t terms;
  float w_bce, w_bal, w_dice, w_focal, s_dice;
  float iou_smooth[2], iou_scale[2];   // slot k live iff terms & (RN_LT_JACCARD << k): jaccard (s, w s), fixed_iou (s, w)
};
struct TermsArgs {
  LossSeg seg[RN_MAX_SEG];
  int nseg, C, width;            // width of a partial row: NSCAL + 3 C, or NSCAL + 5 C with balanced_bce
  int64_t total_rows;
  TermsDev t;
  float* partial;  // [BLOCKS][width]
  float* stats;
  float* cls_out; float* reg_out;
  const float* g_cls; const float* g_reg;
};

__device__ __forceinline__ int seg_of_row(const TermsArgs& a, int64_t r) {
  int s = 0;
  while (s + 1 < a.nseg && r >= a.seg[s + 1].row_start) ++s;
  return s;
}
__device__ __forceinline__ float sigmoidf(float z) { return 1.f / (1.f + expf(-z)); }
// the same three as loss.hip: compares keep a NaN target NaN; the mask is a select, the foreground weight a multiply
__device__ __forceinline__ float clip1(float e) { return e < -1.f ? -1.f : (e > 1.f ? 1.f : e); }
__device__ __forceinline__ float huber1(float e) {
  const float a = fabsf(e), q = fminf(a, 1.f);
  return 0.5f * q * q + (a - q);
}
__device__ __forceinline__ float bce_of(float z, float l) { return fmaxf(z, 0.f) - z * l + log1pf(expf(-fabsf(z))); }
__device__ __forceinline__ float focal_of(float l, float p) {
  const bool pos = (l == 1.f);
  const float pt = pos ? p : 1.f - p;
  const float om = 1.f - pt;
  return -(pos ? 0.25f : 0.75f) * om * om * logf(pt + 1e-7f);
}
// d focal / dz: f = -al (1-pt)^2 log(pt+eps); dpt/dz = +-p(1-p)
__device__ __forceinline__ float focal_grad_of(float l, float p) {
  const bool pos = (l == 1.f);
  const float pt = pos ? p : 1.f - p;
  const float al = pos ? 0.25f : 0.75f;
  const float om = 1.f - pt;
  const float dfdpt = -al * (-2.f * om * logf(pt + 1e-7f) + om * om / (pt + 1e-7f));
  return dfdpt * (pos ? 1.f : -1.f) * p * (1.f - p);
}

// block-level end of both reduce kernels: red[wave][i] -> partial[block][i], waves added in order
template <int N>
__device__ __forceinline__ void store_partial(const TermsArgs& a, float (&red)[WAVES][N]) {
  __syncthreads();
  for (int i = threadIdx.x; i < a.width; i += T) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) v += red[w][i];
    a.partial[(size_t)blockIdx.x * a.width + i] = v;
  }
}

// one wave per row (any C <= 256)
__global__ __launch_bounds__(T) void terms_reduce_kernel(const TermsArgs a) {
  __shared__ float red[WAVES][NSCAL + 5 * 64 * MAXJ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.C;
  const bool bal = a.t.terms & RN_LT_BALANCED_BCE, any_bce = a.t.terms & (RN_LT_BCE | RN_LT_BALANCED_BCE);
  const bool focal = a.t.terms & RN_LT_FOCAL;
  float I[MAXJ], L[MAXJ], P[MAXJ], B1[MAXJ], B0[MAXJ];
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) I[j] = L[j] = P[j] = B1[j] = B0[j] = 0.f;
  float s_m = 0.f, s_fg = 0.f, s_bce = 0.f, s_focal = 0.f, s_hub = 0.f;

  const int64_t wave_id = (int64_t)blockIdx.x * WAVES + wave, nwaves = (int64_t)gridDim.x * WAVES;
  for (int64_t r = wave_id; r < a.total_rows; r += nwaves) {
    const LossSeg& sg = a.seg[seg_of_row(a, r)];
    const int64_t lr = r - sg.row_start;
    if (!sg.tm[lr]) continue;  // wave-uniform
    const float* __restrict__ zrow = sg.zl + lr * C;
    const float* __restrict__ lrow = sg.ll + lr * C;
    float lmax = -1e30f;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
      const int c = lane + 64 * j;
      if (c < C) {
        const float z = zrow[c], l = lrow[c];
        const float p = sigmoidf(z);
        lmax = fmaxf(lmax, l);
        I[j] += l * p; L[j] += l; P[j] += p;
        if (any_bce) {
          const float b = bce_of(z, l);
          s_bce += b;
          if (bal) { if (l == 1.f) B1[j] += b; else B0[j] += b; }
        }
        if (focal) s_focal += focal_of(l, p);
      }
    }
    lmax = rn::wave_max(lmax);
    const bool fg = lmax > 0.5f;
    if (lane == 0) { s_m += 1.f; s_fg += fg ? 1.f : 0.f; }
    if (lane < 4) s_hub = fmaf(fg ? 1.f : 0.f, huber1(sg.rl[lr * 4 + lane] - sg.rp[lr * 4 + lane]), s_hub);
  }
  s_m = rn::wave_sum(s_m); s_fg = rn::wave_sum(s_fg); s_bce = rn::wave_sum(s_bce);
  s_focal = rn::wave_sum(s_focal); s_hub = rn::wave_sum(s_hub);
  if (lane == 0) { red[wave][0] = s_m; red[wave][1] = s_fg; red[wave][2] = s_bce; red[wave][3] = s_focal; red[wave][4] = s_hub; }
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int c = lane + 64 * j;
    if (c < C) {
      red[wave][NSCAL + 3 * c + 0] = I[j];
      red[wave][NSCAL + 3 * c + 1] = L[j];
      red[wave][NSCAL + 3 * c + 2] = P[j];
      if (bal) { red[wave][NSCAL + 3 * C + c] = B1[j]; red[wave][NSCAL + 4 * C + c] = B0[j]; }
    }
  }
  store_partial(a, red);
}

// C % 4 == 0, 4 <= C <= 128: four lanes per row, 16 rows per wave and pass, two row groups per pass; lane (row, j) owns the class
// quads j, j + 4, ..  All 4 NK 16-byte loads of a pass are issued before the first is used (the pass is latency-bound).
template <int NK>
__global__ __launch_bounds__(T) void terms_reduce4_kernel(const TermsArgs a) {
  __shared__ float red[WAVES][NSCAL + 5 * 16 * NK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.C, CQ = C >> 2, j = lane & 3, r16 = lane >> 2;
  const bool bal = a.t.terms & RN_LT_BALANCED_BCE, any_bce = a.t.terms & (RN_LT_BCE | RN_LT_BALANCED_BCE);
  const bool focal = a.t.terms & RN_LT_FOCAL;
  float I[NK][4], L[NK][4], P[NK][4], B1[NK][4], B0[NK][4];
#pragma unroll
  for (int k = 0; k < NK; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) I[k][e] = L[k][e] = P[k][e] = B1[k][e] = B0[k][e] = 0.f;
  float s_m = 0.f, s_fg = 0.f, s_bce = 0.f, s_focal = 0.f, s_hub = 0.f;
  const int64_t ngroups = (a.total_rows + RPW - 1) / RPW;
  const int64_t wave_id = (int64_t)blockIdx.x * WAVES + wave, nwaves = (int64_t)gridDim.x * WAVES;
  for (int64_t g0 = wave_id * 2; g0 < ngroups; g0 += nwaves * 2) {
    float4 z[2][NK], l[2][NK];
    float rl[2], rp[2], tmv[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t r = min((g0 + u) * RPW + r16, a.total_rows - 1);
      const bool live = (g0 + u) * RPW + r16 < a.total_rows;
      const LossSeg& sg = a.seg[seg_of_row(a, r)];
      const int64_t lr = r - sg.row_start;
      tmv[u] = (live && sg.tm[lr]) ? 1.f : 0.f;
      rl[u] = sg.rl[lr * 4 + j]; rp[u] = sg.rp[lr * 4 + j];
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int q = min(j + 4 * k, CQ - 1);
        z[u][k] = *reinterpret_cast<const float4*>(sg.zl + lr * C + q * 4);
        l[u][k] = *reinterpret_cast<const float4*>(sg.ll + lr * C + q * 4);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float lmax = -1e30f, bce = 0.f, foc = 0.f;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const float w = (j + 4 * k < CQ) ? tmv[u] : 0.f;        // 0: the quad does not exist, or the row is not trainable
        const float zz[4] = {z[u][k].x, z[u][k].y, z[u][k].z, z[u][k].w}, ll[4] = {l[u][k].x, l[u][k].y, l[u][k].z, l[u][k].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          // select, not multiply: what a removed row holds (NaN, inf) must not reach a sum as NaN * 0
          const float zv = w != 0.f ? zz[e] : 0.f, lv = w != 0.f ? ll[e] : 0.f;
          const float p = sigmoidf(zv);
          if (j + 4 * k < CQ) lmax = fmaxf(lmax, ll[e]);
          I[k][e] = fmaf(w, lv * p, I[k][e]); L[k][e] = fmaf(w, lv, L[k][e]); P[k][e] = fmaf(w, p, P[k][e]);
          if (any_bce) {
            const float b = w * bce_of(zv, lv);
            bce += b;
            if (bal) { if (lv == 1.f) B1[k][e] += b; else B0[k][e] += b; }
          }
          if (focal) foc = fmaf(w, focal_of(lv, p), foc);
        }
      }
      lmax = fmaxf(lmax, __shfl_xor(lmax, 1, 64));
      lmax = fmaxf(lmax, __shfl_xor(lmax, 2, 64));
      const float fgw = (lmax > 0.5f) ? 1.f : 0.f;
      const float fg = fgw * tmv[u];
      s_bce += bce; s_focal += foc;
      if (j == 0) { s_m += tmv[u]; s_fg += fg; }
      const float hub = fgw * huber1(rl[u] - rp[u]);             // multiply: the foreground weight
      s_hub += (tmv[u] != 0.f) ? hub : 0.f;                      // select: the trainable mask
    }
  }
  s_m = rn::wave_sum(s_m); s_fg = rn::wave_sum(s_fg); s_bce = rn::wave_sum(s_bce);
  s_focal = rn::wave_sum(s_focal); s_hub = rn::wave_sum(s_hub);
  if (lane == 0) { red[wave][0] = s_m; red[wave][1] = s_fg; red[wave][2] = s_bce; red[wave][3] = s_focal; red[wave][4] = s_hub; }
  // per-class sums: over the 16 row lanes that share j
#pragma unroll
  for (int k = 0; k < NK; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float vi = I[k][e], vl = L[k][e], vp = P[k][e], v1 = B1[k][e], v0 = B0[k][e];
#pragma unroll
      for (int m = 4; m < 64; m <<= 1) { vi += __shfl_xor(vi, m, 64); vl += __shfl_xor(vl, m, 64); vp += __shfl_xor(vp, m, 64); }
      if (bal) {
#pragma unroll
        for (int m = 4; m < 64; m <<= 1) { v1 += __shfl_xor(v1, m, 64); v0 += __shfl_xor(v0, m, 64); }
      }
      const int c = 4 * (j + 4 * k) + e;
      if (lane < 4 && j + 4 * k < CQ) {
        red[wave][NSCAL + 3 * c + 0] = vi; red[wave][NSCAL + 3 * c + 1] = vl; red[wave][NSCAL + 3 * c + 2] = vp;
        if (bal) { red[wave][NSCAL + 3 * C + c] = v1; red[wave][NSCAL + 4 * C + c] = v0; }
      }
    }
  store_partial(a, red);
}

// stage 1: sums[i] = sum over blocks of partial[b][i]; 16 values x 16 row lanes per block, fixed order
__global__ __launch_bounds__(256) void terms_sum_kernel(const TermsArgs a, int nblocks, double* __restrict__ sums) {
  __shared__ double sh[16][16];
  const int n = a.width;
  const int il = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + il;
  double v = 0.0;
  if (i < n) {
    int b = rl;
    for (; b + 16 * 7 < nblocks; b += 16 * 8) {  // eight loads in flight, added in row order
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = a.partial[(size_t)(b + 16 * u) * n + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) v += (double)t[u];
    }
    for (; b < nblocks; b += 16) v += (double)a.partial[(size_t)b * n + i];
  }
  sh[rl][il] = v;
  __syncthreads();
  if (rl == 0 && i < n) {
    double t = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) t += sh[r][il];
    sums[i] = t;
  }
}

// stage 2: the class loss as the weighted sum of its terms, and the statistics the gradient pass reads
__global__ void terms_finalize_kernel(const TermsArgs a, const double* __restrict__ sh) {
  __shared__ double part[256];
  const int C = a.C;
  const TermsDev& t = a.t;
  const bool bal = t.terms & RN_LT_BALANCED_BCE;
  const double M = sh[0], fg = sh[1];
  for (int i = threadIdx.x; i < 3 * C; i += blockDim.x) a.stats[H + i] = (float)sh[NSCAL + i];
  for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) a.stats[H + 3 * C + i] = bal ? (float)sh[NSCAL + 3 * C + i] : 0.f;
  double d = 0.0;                 // C times the per-class terms
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const double I = sh[NSCAL + 3 * c], L = sh[NSCAL + 3 * c + 1], P = sh[NSCAL + 3 * c + 2];
    if (t.terms & RN_LT_DICE) d += (double)t.w_dice * (1.0 - (2.0 * I + (double)t.s_dice) / (L + P + (double)t.s_dice));
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (t.terms & (RN_LT_JACCARD << k)) {
        const double s = (double)t.iou_smooth[k];
        d += (double)t.iou_scale[k] * (1.0 - (I + s) / (L + P - I + s));
      }
    if (bal) d += (double)t.w_bal * (((M - L) / M) * sh[NSCAL + 3 * C + c] + (L / M) * sh[NSCAL + 4 * C + c]) / M;
  }
  part[threadIdx.x] = d;
  __syncthreads();
  if (threadIdx.x == 0) {
    double cls = 0.0;
    for (int i = 0; i < (int)blockDim.x; ++i) cls += part[i];
    cls /= C;
    if (t.terms & RN_LT_BCE) cls += (double)t.w_bce * sh[2] / (M * C);
    if (t.terms & RN_LT_FOCAL) cls += (double)t.w_focal * sh[3] / (fg > 1.0 ? fg : 1.0);
    const double reg = fg > 0.0 ? sh[4] / (4.0 * fg) : 0.0;
    a.stats[0] = (float)cls; a.stats[1] = (float)reg; a.stats[2] = (float)M; a.stats[3] = (float)fg;
    if (a.cls_out) *a.cls_out = (float)cls;
    if (a.reg_out) *a.reg_out = (float)reg;
    a.stats[4] = (float)sh[2]; a.stats[5] = (float)sh[3]; a.stats[6] = (float)sh[4]; a.stats[7] = 0.f;
  }
}

// What the gradient pass needs of class c, upstream gradient included:
//   dz = (p - l) (k_bce + (l == 1 ? wp : wn)) + p (1 - p) (l A + B) + k_focal focal'
//   dice: -(w/C) p' (2 l U - (2I+s))/U^2, U = L+P+s       => A -= 2 k/U,          B += k (2I+s)/U^2
//   iou : -(k) p' (l D - (I+s)(1-l))/D^2, D = L+P-I+s     => A -= k (D + I+s)/D^2, B += k (I+s)/D^2
struct ClassConst { float A, B, wp, wn; };
__device__ __forceinline__ ClassConst class_const(const TermsArgs& a, int c, float gc, float M) {
  const TermsDev& t = a.t;
  const float fC = (float)a.C;
  const float I = a.stats[H + 3 * c], L = a.stats[H + 3 * c + 1], P = a.stats[H + 3 * c + 2];
  ClassConst k = {0.f, 0.f, 0.f, 0.f};
  if (t.terms & RN_LT_DICE) {
    const float U = L + P + t.s_dice, kd = gc * t.w_dice / fC;
    k.A -= 2.f * kd / U;
    k.B += kd * (2.f * I + t.s_dice) / (U * U);
  }
#pragma unroll
  for (int s = 0; s < 2; ++s)
    if (t.terms & (RN_LT_JACCARD << s)) {
      const float N = I + t.iou_smooth[s], D = L + P - I + t.iou_smooth[s], ki = gc * t.iou_scale[s] / fC;
      k.A -= ki * (D + N) / (D * D);
      k.B += ki * N / (D * D);
    }
  if (t.terms & RN_LT_BALANCED_BCE) {
    const float kb = gc * t.w_bal / (M * fC);
    k.wp = kb * ((M - L) / M);
    k.wn = kb * (L / M);
  }
  return k;
}
__device__ __forceinline__ float elem_grad(const TermsDev& t, const ClassConst& k, float k_bce, float k_focal, float z, float l) {
  const float p = sigmoidf(z);
  float g = (p - l) * (k_bce + (l == 1.f ? k.wp : k.wn)) + p * (1.f - p) * fmaf(l, k.A, k.B);
  if (t.terms & RN_LT_FOCAL) g = fmaf(k_focal, focal_grad_of(l, p), g);
  return g;
}

template <int NK>
__global__ __launch_bounds__(T) void terms_grad4_kernel(const TermsArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.C, CQ = C >> 2, j = lane & 3, r16 = lane >> 2;
  const float M = a.stats[2], nfg = a.stats[3];
  const float gc = a.g_cls[0], gr = a.g_reg[0];
  const float k_bce = (a.t.terms & RN_LT_BCE) ? gc * a.t.w_bce / (M * (float)C) : 0.f;
  const float k_focal = gc * a.t.w_focal / fmaxf(nfg, 1.f);
  const float k_reg = nfg > 0.f ? gr / (4.f * nfg) : 0.f;
  ClassConst kc[NK][4];
#pragma unroll
  for (int k = 0; k < NK; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) kc[k][e] = class_const(a, min(4 * (j + 4 * k) + e, C - 1), gc, M);
  const int64_t ngroups = (a.total_rows + RPW - 1) / RPW;
  const int64_t wave_id = (int64_t)blockIdx.x * WAVES + wave, nwaves = (int64_t)gridDim.x * WAVES;
  for (int64_t g0 = wave_id * 2; g0 < ngroups; g0 += nwaves * 2) {
    float4 z[2][NK], l[2][NK];
    float rl[2], rp[2], tmv[2];
    float* dzp[2]; float* drp[2]; bool live[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t r = min((g0 + u) * RPW + r16, a.total_rows - 1);
      live[u] = (g0 + u) * RPW + r16 < a.total_rows;
      const LossSeg& sg = a.seg[seg_of_row(a, r)];
      const int64_t lr = r - sg.row_start;
      tmv[u] = (live[u] && sg.tm[lr]) ? 1.f : 0.f;
      rl[u] = sg.rl[lr * 4 + j]; rp[u] = sg.rp[lr * 4 + j];
      dzp[u] = sg.dz + lr * C; drp[u] = sg.dr + lr * 4 + j;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int q = min(j + 4 * k, CQ - 1);
        z[u][k] = *reinterpret_cast<const float4*>(sg.zl + lr * C + q * 4);
        l[u][k] = *reinterpret_cast<const float4*>(sg.ll + lr * C + q * 4);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float lmax = -1e30f;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const float zz[4] = {z[u][k].x, z[u][k].y, z[u][k].z, z[u][k].w}, ll[4] = {l[u][k].x, l[u][k].y, l[u][k].z, l[u][k].w};
        float g[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (j + 4 * k < CQ) lmax = fmaxf(lmax, ll[e]);
          g[e] = elem_grad(a.t, kc[k][e], k_bce, k_focal, zz[e], ll[e]);
          g[e] = tmv[u] != 0.f ? g[e] : 0.f;
        }
        if (live[u] && j + 4 * k < CQ) *reinterpret_cast<float4*>(dzp[u] + (j + 4 * k) * 4) = make_float4(g[0], g[1], g[2], g[3]);
      }
      lmax = fmaxf(lmax, __shfl_xor(lmax, 1, 64));
      lmax = fmaxf(lmax, __shfl_xor(lmax, 2, 64));
      if (live[u]) {
        float g = 0.f;
        if (tmv[u] != 0.f) g = ((lmax > 0.5f) ? 1.f : 0.f) * (k_reg * clip1(rp[u] - rl[u]));
        *drp[u] = g;
      }
    }
  }
}

__global__ __launch_bounds__(T) void terms_grad_kernel(const TermsArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.C;
  const float M = a.stats[2], nfg = a.stats[3];
  const float gc = a.g_cls[0], gr = a.g_reg[0];
  const float k_bce = (a.t.terms & RN_LT_BCE) ? gc * a.t.w_bce / (M * (float)C) : 0.f;
  const float k_focal = gc * a.t.w_focal / fmaxf(nfg, 1.f);
  const float k_reg = nfg > 0.f ? gr / (4.f * nfg) : 0.f;
  ClassConst kc[MAXJ];
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) kc[j] = class_const(a, min(lane + 64 * j, C - 1), gc, M);
  const int64_t wave_id = (int64_t)blockIdx.x * WAVES + wave, nwaves = (int64_t)gridDim.x * WAVES;
  for (int64_t r = wave_id; r < a.total_rows; r += nwaves) {
    const LossSeg& sg = a.seg[seg_of_row(a, r)];
    const int64_t lr = r - sg.row_start;
    float* __restrict__ dzrow = sg.dz + lr * C;
    if (!sg.tm[lr]) {
#pragma unroll
      for (int j = 0; j < MAXJ; ++j) { const int c = lane + 64 * j; if (c < C) dzrow[c] = 0.f; }
      if (lane < 4) sg.dr[lr * 4 + lane] = 0.f;
      continue;
    }
    const float* __restrict__ zrow = sg.zl + lr * C;
    const float* __restrict__ lrow = sg.ll + lr * C;
    float lmax = -1e30f;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
      const int c = lane + 64 * j;
      if (c < C) {
        const float z = zrow[c], l = lrow[c];
        lmax = fmaxf(lmax, l);
        dzrow[c] = elem_grad(a.t, kc[j], k_bce, k_focal, z, l);
      }
    }
    lmax = rn::wave_max(lmax);
    if (lane < 4) {
      const float e = sg.rp[lr * 4 + lane] - sg.rl[lr * 4 + lane];    // d huber(l - p)/dp = clip(p - l)
      sg.dr[lr * 4 + lane] = ((lmax > 0.5f) ? 1.f : 0.f) * (k_reg * clip1(e));
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ host
struct TermField { uint32_t bit; const char* name; float weight; bool has_smooth; float smooth; };

int validate(const rn_loss_terms* t) {
  RN_CHECK_ARG(t, "loss terms: null descriptor");
  RN_CHECK_ARG(t->terms != 0, "loss terms: no term set");
  RN_CHECK_ARG((t->terms & ~ALL_TERMS) == 0, "loss terms: unknown term bits 0x%x", t->terms & ~ALL_TERMS);
  const TermField f[6] = {{RN_LT_BCE, "bce", t->w_bce, false, 0.f},
                          {RN_LT_BALANCED_BCE, "balanced_bce", t->w_balanced_bce, false, 0.f},
                          {RN_LT_DICE, "dice", t->w_dice, true, t->s_dice},
                          {RN_LT_JACCARD, "jaccard", t->w_jaccard, true, t->s_jaccard},
                          {RN_LT_FIXED_IOU, "fixed_iou", t->w_fixed_iou, true, t->s_fixed_iou},
                          {RN_LT_FOCAL, "focal", t->w_focal, false, 0.f}};
  for (const TermField& x : f) {
    if (t->terms & x.bit) {
      RN_CHECK_ARG(std::isfinite(x.weight) && x.weight > 0.f, "loss terms: weight of %s must be finite and > 0 (got %g)", x.name, x.weight);
      RN_CHECK_ARG(!x.has_smooth || (std::isfinite(x.smooth) && x.smooth >= 0.f), "loss terms: smooth of %s must be finite and >= 0 (got %g)",
                   x.name, x.smooth);
    } else {
      RN_CHECK_ARG(x.weight == 0.f, "loss terms: weight of the clear term %s must be 0 (got %g)", x.name, x.weight);
      RN_CHECK_ARG(!x.has_smooth || x.smooth == 0.f, "loss terms: smooth of the clear term %s must be 0 (got %g)", x.name, x.smooth);
    }
  }
  // jaccard's device scale is weight * smooth
  RN_CHECK_ARG(std::isfinite(t->w_jaccard * t->s_jaccard), "loss terms: weight * smooth of jaccard overflows (%g * %g)", t->w_jaccard,
               t->s_jaccard);
  return RN_OK;
}

// {bce:1, dice:1:0} and {focal:1} are loss.hip's two modes (RN_LOSS_TERMS_GENERAL=1: the general kernels for them too, measurements)
int legacy_mode(const rn_loss_terms* t) {
  static const bool general = getenv("RN_LOSS_TERMS_GENERAL") && atoi(getenv("RN_LOSS_TERMS_GENERAL"));
  if (general) return -1;
  if (t->terms == (RN_LT_BCE | RN_LT_DICE) && t->w_bce == 1.f && t->w_dice == 1.f && t->s_dice == 0.f) return RN_LOSS_BCE_DICE;
  if (t->terms == RN_LT_FOCAL && t->w_focal == 1.f) return RN_LOSS_FOCAL;
  return -1;
}

int build(const rn_loss_seg* segs, int nseg, int C, const rn_loss_terms* t, TermsArgs* a, bool bwd) {
  RN_CHECK_ARG(segs && nseg >= 1 && nseg <= RN_MAX_SEG, "loss terms: bad segments");
  RN_UNSUPPORTED(C < 1 || C > 64 * MAXJ, "loss terms: num_classes %d outside [1,%d]", C, 64 * MAXJ);
  a->nseg = nseg; a->C = C;
  a->width = NSCAL + ((t->terms & RN_LT_BALANCED_BCE) ? 5 : 3) * C;
  a->t.terms = t->terms;
  a->t.w_bce = t->w_bce; a->t.w_bal = t->w_balanced_bce; a->t.w_dice = t->w_dice; a->t.w_focal = t->w_focal; a->t.s_dice = t->s_dice;
  a->t.iou_smooth[0] = t->s_jaccard; a->t.iou_scale[0] = t->w_jaccard * t->s_jaccard;
  a->t.iou_smooth[1] = t->s_fixed_iou; a->t.iou_scale[1] = t->w_fixed_iou;
  int64_t rows = 0;
  for (int s = 0; s < nseg; ++s) {
    RN_CHECK_ARG(segs[s].cls_logit && segs[s].cls_label && segs[s].reg_pred && segs[s].reg_label && segs[s].trainable &&
                 segs[s].rows >= 0, "loss terms: null pointer in segment %d", s);
    if (bwd) RN_CHECK_ARG(segs[s].d_cls_logit && segs[s].d_reg_pred, "loss terms bwd: null gradient buffer in segment %d", s);
    LossSeg& d = a->seg[s];
    d.zl = segs[s].cls_logit; d.ll = segs[s].cls_label; d.rp = segs[s].reg_pred; d.rl = segs[s].reg_label;
    d.tm = segs[s].trainable; d.dz = segs[s].d_cls_logit; d.dr = segs[s].d_reg_pred;
    d.rows = segs[s].rows; d.row_start = rows;
    rows += segs[s].rows;
  }
  a->total_rows = rows;
  return RN_OK;
}

// the layout choice and the grids of loss.hip
bool use4(int C) {
  static const bool off = getenv("RN_LOSS_WAVE_PER_ROW") && atoi(getenv("RN_LOSS_WAVE_PER_ROW"));
  return !off && C % 4 == 0 && C >= 4 && C <= 128;
}
int nblocks4(int64_t rows) {      // one pass of two row groups per wave
  int64_t b = (rows + RPW * 2 * WAVES - 1) / (RPW * 2 * WAVES);
  return (int)(b > BLOCKS ? BLOCKS : (b < 1 ? 1 : b));
}
int nblocks1(int64_t rows) {
  int64_t b = (rows + WAVES * 4 - 1) / (WAVES * 4);
  return (int)(b > BLOCKS ? BLOCKS : (b < 1 ? 1 : b));
}
template <bool REDUCE, int NK>
void launch4_nk(const TermsArgs& a, hipStream_t st) {
  const dim3 grid(nblocks4(a.total_rows)), block(T);
  if (REDUCE) hipLaunchKernelGGL((terms_reduce4_kernel<NK>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((terms_grad4_kernel<NK>), grid, block, 0, st, a);
}
template <bool REDUCE>
void launch4(const TermsArgs& a, hipStream_t st) {
  switch ((a.C / 4 + 3) / 4) {
    case 1: launch4_nk<REDUCE, 1>(a, st); break;
    case 2: launch4_nk<REDUCE, 2>(a, st); break;
    case 3: launch4_nk<REDUCE, 3>(a, st); break;
    case 4: launch4_nk<REDUCE, 4>(a, st); break;
    case 5: launch4_nk<REDUCE, 5>(a, st); break;
    case 6: launch4_nk<REDUCE, 6>(a, st); break;
    case 7: launch4_nk<REDUCE, 7>(a, st); break;
    default: launch4_nk<REDUCE, 8>(a, st); break;
  }
}
size_t partial_bytes(int width) { return rn::align_up((size_t)BLOCKS * (size_t)width * sizeof(float), 256); }
}  // namespace

extern "C" size_t rn_loss_terms_stats_floats(int num_classes) { return (size_t)H + 5 * (size_t)(num_classes > 0 ? num_classes : 0); }

extern "C" size_t rn_loss_terms_workspace(const rn_loss_seg* segs, int nseg, int num_classes, const rn_loss_terms* t) {
  if (validate(t) != RN_OK) return 0;
  if (legacy_mode(t) >= 0) return rn_loss_workspace(segs, nseg, num_classes);
  const int width = NSCAL + ((t->terms & RN_LT_BALANCED_BCE) ? 5 : 3) * (num_classes > 0 ? num_classes : 0);
  return partial_bytes(width) + (size_t)width * sizeof(double);
}

extern "C" int rn_loss_terms_fwd(const rn_loss_seg* segs, int nseg, int num_classes, const rn_loss_terms* t, float* stats,
                                 float* class_loss_out, float* regr_loss_out, void* workspace, size_t workspace_bytes,
                                 rn_stream_t stream) {
  if (int e = validate(t)) return e;
  const int mode = legacy_mode(t);
  if (mode >= 0) return rn_loss_fwd(segs, nseg, num_classes, mode, stats, class_loss_out, regr_loss_out, workspace, workspace_bytes, stream);
  TermsArgs a = {};
  if (int e = build(segs, nseg, num_classes, t, &a, false)) return e;
  RN_CHECK_ARG(stats && workspace, "loss terms fwd: null stats/workspace");
  if (workspace_bytes < rn_loss_terms_workspace(segs, nseg, num_classes, t)) {
    rn::set_error("loss terms fwd: workspace too small");
    return RN_EWORKSPACE;
  }
  a.partial = (float*)workspace; a.stats = stats; a.cls_out = class_loss_out; a.reg_out = regr_loss_out;
  hipStream_t st = (hipStream_t)stream;
  const bool four = use4(num_classes);
  const int nb = four ? nblocks4(a.total_rows) : nblocks1(a.total_rows);
  if (four) launch4<true>(a, st);
  else hipLaunchKernelGGL(terms_reduce_kernel, dim3(nb), dim3(T), 0, st, a);
  double* sums = (double*)((char*)workspace + partial_bytes(a.width));
  hipLaunchKernelGGL(terms_sum_kernel, dim3(rn::ceil_div(a.width, 16)), dim3(256), 0, st, a, nb, sums);
  hipLaunchKernelGGL(terms_finalize_kernel, dim3(1), dim3(256), 0, st, a, (const double*)sums);
  RN_LAUNCH_CHECK();
  return RN_OK;
}

extern "C" int rn_loss_terms_bwd(const rn_loss_seg* segs, int nseg, int num_classes, const rn_loss_terms* t, const float* stats,
                                 const float* g_cls, const float* g_reg, rn_stream_t stream) {
  if (int e = validate(t)) return e;
  const int mode = legacy_mode(t);
  if (mode >= 0) return rn_loss_bwd(segs, nseg, num_classes, mode, stats, g_cls, g_reg, stream);
  TermsArgs a = {};
  if (int e = build(segs, nseg, num_classes, t, &a, true)) return e;
  RN_CHECK_ARG(stats && g_cls && g_reg, "loss terms bwd: null stats/upstream gradient");
  a.stats = const_cast<float*>(stats); a.g_cls = g_cls; a.g_reg = g_reg;
  hipStream_t st = (hipStream_t)stream;
  if (use4(num_classes)) launch4<false>(a, st);
  else hipLaunchKernelGGL(terms_grad_kernel, dim3(nblocks1(a.total_rows)), dim3(T), 0, st, a);
  RN_LAUNCH_CHECK();
  return RN_OK;
}
