// Box regression loss as a weighted sum of terms over the foreground (fg) rows: fg = trainable and max_c label[row, c] > 0.5, the
// rule of loss.hip.  Prediction p and label l of a row are anchor-relative (ty, tx, th, tw) (the reference's dataset.py:102-112,
// utils.py:100-117); in anchor units
//   box(t) = (ty - e^th/2, tx - e^tw/2, ty + e^th/2, tx + e^tw/2)
//   iy = max(0, min(P2, L2) - max(P0, L0)), ix likewise, I = iy ix, U = area(p) + area(l) - I, IoU = I/U
//   cy = max(P2, L2) - min(P0, L0),         cx likewise, E = cy cx, GIoU = IoU - (E - U)/E
//   huber : w sum_fg huber_delta(l - p) / (4 #fg)       (regression_loss, losses.py:144-152; delta = tf.losses.huber_loss's)
//   iou   : w sum_fg (1 - IoU) / #fg
//   giou  : w sum_fg (1 - GIoU) / #fg
// Both boxes of a row share the anchor: their image-space versions (regression_postprocess, utils.py:108-117) are the anchor-unit
// ones under ONE translation and ONE positive per-axis scaling, which ratios of areas do not see -- no anchor table is read.
// DIoU / CIoU hold centre distance over diagonal, which an anisotropic scaling changes: they need per-row anchor aspect ratios
// and are not covered.
// Subgradients: max(P, L) follows P where P >= L, min(P, L) where P <= L, max(0, d) where d > 0.  The area of a box is formed
// from its own edges, (P2 - P0)(P3 - P1), so that identical boxes give IoU = GIoU = 1 exactly.
// Masking: huber is the fg weight TIMES the term on every trainable row (a NaN there reaches the loss, as in loss.hip and the
// reference); the overlap terms SELECT (a row that is not fg adds exactly 0 and gets gradient exactly 0, whatever it holds:
// nothing constrains exp(th) of a background prediction).  Rows outside the trainable mask are never read into a sum.
// Forward: four lanes per row take the label row's maximum (16-byte loads when C % 4 == 0, scalar loads otherwise), lane 0 of
// the four evaluates the row; registers -> wave -> LDS -> one partial row per block; one block adds the partial rows in fixed
// order in fp64 and writes loss and statistics.  No atomics: bitwise reproducible.  Backward: one lane per row over [rows, 4].
// The term set is a wave-uniform launch argument; without an overlap term no expf is evaluated.
#include <stdlib.h>

#include <cmath>

#include "rn_common.h"

namespace {

constexpr int T = 256;
constexpr int WAVES = T / 64;
constexpr int RPW = 16;                    // forward: rows per wave and pass (four lanes per row)
constexpr int RPB = RPW * WAVES;           // forward: rows per block and pass
constexpr int FWD_BLOCKS = 2048;           // the forward grid-strides past FWD_BLOCKS * RPB = 131072 rows
constexpr int BWD_BLOCKS = 512;            // the backward past BWD_BLOCKS * T = 131072 rows
constexpr int NP = 5;                      // partial row: #fg, sum huber, sum (1 - IoU), sum (1 - GIoU), sum IoU
constexpr int PW = 8;                      // its stride in floats
constexpr uint32_t ALL_TERMS = RN_RT_HUBER | RN_RT_IOU | RN_RT_GIOU;
constexpr uint32_t OVERLAP = RN_RT_IOU | RN_RT_GIOU;

struct RegrSeg {
  const float* ll; const float* rp; const float* rl; const uint8_t* tm;
  float* dr;
  int64_t row_start;
};
struct RegrArgs {
  RegrSeg seg[RN_MAX_SEG];
  int nseg, C;
  int64_t total_rows;
  uint32_t terms;
  float w_huber, w_iou, w_giou, delta;
  float* partial;        // [FWD_BLOCKS][PW]
  float* stats;
  float* reg_out;
  uint8_t* fg_rows;      // [total_rows], segment order
  const float* g_reg;
};

__device__ __forceinline__ int seg_of_row(const RegrArgs& a, int64_t r) {
  int s = 0;
  while (s + 1 < a.nseg && r >= a.seg[s + 1].row_start) ++s;
  return s;
}
__device__ __forceinline__ float huber_d(float e, float d) {      // tf.losses.huber_loss: 0.5 q^2 + delta (|e| - q), q = min(|e|, delta)
  const float a = fabsf(e), q = fminf(a, d);
  return 0.5f * q * q + d * (a - q);
}
__device__ __forceinline__ float clip_d(float e, float d) { return e < -d ? -d : (e > d ? d : e); }

// what both passes need of a pair of boxes
struct Overlap {
  float ph, pw;            // e^th, e^tw of the prediction
  float iy, ix, cy, cx;    // intersection and enclosure extents
  float ap;                // area of the prediction
  float I, U, E;
  bool sy_hi, sy_lo, sx_hi, sx_lo;   // min / max of the intersection follow the prediction
  bool ty_hi, ty_lo, tx_hi, tx_lo;   // max / min of the enclosure follow the prediction
  bool py, px;                       // the clamp at 0 passes
};
__device__ __forceinline__ Overlap overlap_of(const float4 p, const float4 l) {
  Overlap o;
  o.ph = expf(p.z); o.pw = expf(p.w);
  const float lh = expf(l.z), lw = expf(l.w);
  const float P0 = p.x - 0.5f * o.ph, P2 = p.x + 0.5f * o.ph, P1 = p.y - 0.5f * o.pw, P3 = p.y + 0.5f * o.pw;
  const float L0 = l.x - 0.5f * lh, L2 = l.x + 0.5f * lh, L1 = l.y - 0.5f * lw, L3 = l.y + 0.5f * lw;
  o.sy_hi = P2 <= L2; o.sy_lo = P0 >= L0; o.sx_hi = P3 <= L3; o.sx_lo = P1 >= L1;
  o.ty_hi = P2 >= L2; o.ty_lo = P0 <= L0; o.tx_hi = P3 >= L3; o.tx_lo = P1 <= L1;
  const float dy = (o.sy_hi ? P2 : L2) - (o.sy_lo ? P0 : L0), dx = (o.sx_hi ? P3 : L3) - (o.sx_lo ? P1 : L1);
  o.py = dy > 0.f; o.px = dx > 0.f;
  o.iy = o.py ? dy : 0.f; o.ix = o.px ? dx : 0.f;
  o.cy = (o.ty_hi ? P2 : L2) - (o.ty_lo ? P0 : L0); o.cx = (o.tx_hi ? P3 : L3) - (o.tx_lo ? P1 : L1);
  o.ap = (P2 - P0) * (P3 - P1);
  const float al = (L2 - L0) * (L3 - L1);
  o.I = o.iy * o.ix;
  o.U = o.ap + al - o.I;
  o.E = o.cy * o.cx;
  return o;
}

// VEC: C % 4 == 0, 16-byte label loads; otherwise scalar loads (any C >= 1)
template <bool VEC>
__global__ __launch_bounds__(T) void regr_reduce_kernel(const RegrArgs a) {
  __shared__ float red[WAVES][NP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.C, j = lane & 3, r16 = lane >> 2;
  const bool huber = a.terms & RN_RT_HUBER, overlap = a.terms & OVERLAP;
  float s_fg = 0.f, s_hub = 0.f, s_iou_l = 0.f, s_giou_l = 0.f, s_iou = 0.f;
  for (int64_t r0 = (int64_t)blockIdx.x * RPB + wave * RPW; r0 < a.total_rows; r0 += (int64_t)gridDim.x * RPB) {
    const int64_t r = r0 + r16;
    const bool live = r < a.total_rows;
    const RegrSeg& sg = a.seg[seg_of_row(a, live ? r : a.total_rows - 1)];
    const int64_t lr = r - sg.row_start;
    const bool tm = live && sg.tm[lr];
    float lmax = -1e30f;
    if (tm) {
      if (VEC) {
        const float4* __restrict__ lrow = reinterpret_cast<const float4*>(sg.ll + lr * C);
        const int CQ = C >> 2;
#pragma unroll 4
        for (int q = j; q < CQ; q += 4) {
          const float4 v = lrow[q];
          lmax = fmaxf(lmax, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
        }
      } else {
        const float* __restrict__ lrow = sg.ll + lr * C;
#pragma unroll 4
        for (int c = j; c < C; c += 4) lmax = fmaxf(lmax, lrow[c]);
      }
    }
    lmax = fmaxf(lmax, __shfl_xor(lmax, 1, 64));
    lmax = fmaxf(lmax, __shfl_xor(lmax, 2, 64));
    const bool fg = tm && lmax > 0.5f;
    if (j == 0 && live) {
      a.fg_rows[r] = fg ? 1 : 0;
      if (tm && (huber || fg)) {
        const float4 p = *reinterpret_cast<const float4*>(sg.rp + lr * 4), l = *reinterpret_cast<const float4*>(sg.rl + lr * 4);
        if (huber) {      // multiply: the foreground weight
          const float h = (huber_d(l.x - p.x, a.delta) + huber_d(l.y - p.y, a.delta)) + (huber_d(l.z - p.z, a.delta) + huber_d(l.w - p.w, a.delta));
          s_hub = fmaf(fg ? 1.f : 0.f, h, s_hub);
        }
        if (overlap && fg) {   // select
          const Overlap o = overlap_of(p, l);
          const float iou = o.I / o.U;
          s_iou += iou; s_iou_l += 1.f - iou;
          s_giou_l += (1.f - iou) + (o.E - o.U) / o.E;
        }
      }
      s_fg += fg ? 1.f : 0.f;
    }
  }
  s_fg = rn::wave_sum(s_fg); s_hub = rn::wave_sum(s_hub); s_iou_l = rn::wave_sum(s_iou_l);
  s_giou_l = rn::wave_sum(s_giou_l); s_iou = rn::wave_sum(s_iou);
  if (lane == 0) { red[wave][0] = s_fg; red[wave][1] = s_hub; red[wave][2] = s_iou_l; red[wave][3] = s_giou_l; red[wave][4] = s_iou; }
  __syncthreads();
  if (tid < NP) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) v += red[w][tid];
    a.partial[(size_t)blockIdx.x * PW + tid] = v;
  }
}

// one block: thread t adds the partial rows t, t + T, .. in fp64, then the T sums are added in order
__global__ __launch_bounds__(T) void regr_finalize_kernel(const RegrArgs a, int nblocks) {
  __shared__ double sh[NP][T];
  const int tid = threadIdx.x;
  double v[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) v[i] = 0.0;
  for (int b = tid; b < nblocks; b += T)
#pragma unroll
    for (int i = 0; i < NP; ++i) v[i] += (double)a.partial[(size_t)b * PW + i];
#pragma unroll
  for (int i = 0; i < NP; ++i) sh[i][tid] = v[i];
  __syncthreads();
  if (tid < NP) {
    double t = 0.0;
    for (int k = 0; k < T; ++k) t += sh[tid][k];
    sh[tid][0] = t;
  }
  __syncthreads();
  if (tid == 0) {
    const double fg = sh[0][0];
    double loss = 0.0;
    if (fg > 0.0) {
      if (a.terms & RN_RT_HUBER) loss += (double)a.w_huber * sh[1][0] / (4.0 * fg);
      if (a.terms & RN_RT_IOU) loss += (double)a.w_iou * sh[2][0] / fg;
      if (a.terms & RN_RT_GIOU) loss += (double)a.w_giou * sh[3][0] / fg;
    }
    a.stats[0] = (float)loss; a.stats[1] = (float)fg; a.stats[2] = (float)sh[1][0]; a.stats[3] = (float)sh[2][0];
    a.stats[4] = (float)sh[3][0]; a.stats[5] = (float)sh[4][0]; a.stats[6] = 0.f; a.stats[7] = 0.f;
    if (a.reg_out) *a.reg_out = (float)loss;
  }
}

// d(g_reg * regr_loss)/d reg_pred.  With a = g w_iou / #fg, b = g w_giou / #fg the row's overlap loss is
// (a + b)(1 - IoU) + b (E - U)/E, and with dU = dA - dI (A = area(p)):
//   d = cI dI + cA dA + cE dE,  cI = -(a + b)(U + I)/U^2 + b/E,  cA = (a + b) I/U^2 - b/E,  cE = b U/E^2
//   dI = d(iy) ix + iy d(ix), dE likewise; d(P0, P2)/d(ty) = (1, 1), d(P0, P2)/d(th) = (-e^th/2, e^th/2), dA/d(th) = A
__global__ __launch_bounds__(T) void regr_grad_kernel(const RegrArgs a) {
  const float nfg = a.stats[1], g = a.g_reg[0];
  const float k_hub = nfg > 0.f ? g * a.w_huber / (4.f * nfg) : 0.f;
  const float ka = nfg > 0.f ? g * (a.w_iou + a.w_giou) / nfg : 0.f;     // the weights of clear terms are 0
  const float kb = nfg > 0.f ? g * a.w_giou / nfg : 0.f;
  const bool huber = a.terms & RN_RT_HUBER, overlap = a.terms & OVERLAP, giou = a.terms & RN_RT_GIOU;
  for (int64_t r = (int64_t)blockIdx.x * T + threadIdx.x; r < a.total_rows; r += (int64_t)gridDim.x * T) {
    const RegrSeg& sg = a.seg[seg_of_row(a, r)];
    const int64_t lr = r - sg.row_start;
    float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.fg_rows[r]) {
      const float4 p = *reinterpret_cast<const float4*>(sg.rp + lr * 4), l = *reinterpret_cast<const float4*>(sg.rl + lr * 4);
      if (huber) {        // d huber(l - p)/dp = clip(p - l)
        d.x = k_hub * clip_d(p.x - l.x, a.delta); d.y = k_hub * clip_d(p.y - l.y, a.delta);
        d.z = k_hub * clip_d(p.z - l.z, a.delta); d.w = k_hub * clip_d(p.w - l.w, a.delta);
      }
      if (overlap) {
        const Overlap o = overlap_of(p, l);
        const float u2 = o.U * o.U;
        float cI = -ka * (o.U + o.I) / u2, cA = ka * o.I / u2;
        const float hy = 0.5f * o.ph, hx = 0.5f * o.pw;
        const float sy_hi = o.sy_hi ? 1.f : 0.f, sy_lo = o.sy_lo ? 1.f : 0.f, sx_hi = o.sx_hi ? 1.f : 0.f, sx_lo = o.sx_lo ? 1.f : 0.f;
        if (giou) {
          const float cE = kb * o.U / (o.E * o.E);
          cI += kb / o.E; cA -= kb / o.E;
          const float ty_hi = o.ty_hi ? 1.f : 0.f, ty_lo = o.ty_lo ? 1.f : 0.f, tx_hi = o.tx_hi ? 1.f : 0.f, tx_lo = o.tx_lo ? 1.f : 0.f;
          const float ey = cE * o.cx, ex = cE * o.cy;
          d.x += ey * (ty_hi - ty_lo); d.z += ey * (ty_hi + ty_lo) * hy;
          d.y += ex * (tx_hi - tx_lo); d.w += ex * (tx_hi + tx_lo) * hx;
        }
        const float gy = o.py ? cI * o.ix : 0.f, gx = o.px ? cI * o.iy : 0.f;
        const float ga = cA * o.ap;
        d.x += gy * (sy_hi - sy_lo); d.z += gy * (sy_hi + sy_lo) * hy + ga;
        d.y += gx * (sx_hi - sx_lo); d.w += gx * (sx_hi + sx_lo) * hx + ga;
      }
    }
    *reinterpret_cast<float4*>(sg.dr + lr * 4) = d;
  }
}

// ------------------------------------------------------------------------------------------------------------------ host
int validate(const rn_regr_terms* t) {
  RN_CHECK_ARG(t, "regr terms: null descriptor");
  RN_CHECK_ARG(t->terms != 0, "regr terms: no term set");
  RN_CHECK_ARG((t->terms & ~ALL_TERMS) == 0, "regr terms: unknown term bits 0x%x", t->terms & ~ALL_TERMS);
  const struct { uint32_t bit; const char* name; float weight; } f[3] = {
      {RN_RT_HUBER, "huber", t->w_huber}, {RN_RT_IOU, "iou", t->w_iou}, {RN_RT_GIOU, "giou", t->w_giou}};
  for (const auto& x : f) {
    if (t->terms & x.bit)
      RN_CHECK_ARG(std::isfinite(x.weight) && x.weight > 0.f, "regr terms: w_%s must be finite and > 0 (got %g)", x.name, x.weight);
    else
      RN_CHECK_ARG(x.weight == 0.f, "regr terms: w_%s of the clear term must be 0 (got %g)", x.name, x.weight);
  }
  if (t->terms & RN_RT_HUBER)
    RN_CHECK_ARG(std::isfinite(t->delta_huber) && t->delta_huber > 0.f, "regr terms: delta_huber must be finite and > 0 (got %g)", t->delta_huber);
  else
    RN_CHECK_ARG(t->delta_huber == 0.f, "regr terms: delta_huber of the clear term must be 0 (got %g)", t->delta_huber);
  return RN_OK;
}

int build(const rn_loss_seg* segs, int nseg, const rn_regr_terms* t, RegrArgs* a, bool bwd) {
  RN_CHECK_ARG(nseg >= 1 && nseg <= RN_MAX_SEG, "regr terms: nseg %d outside [1,%d]", nseg, RN_MAX_SEG);
  RN_CHECK_ARG(segs, "regr terms: null segs");
  a->nseg = nseg;
  a->terms = t->terms; a->w_huber = t->w_huber; a->w_iou = t->w_iou; a->w_giou = t->w_giou; a->delta = t->delta_huber;
  int64_t rows = 0;
  for (int s = 0; s < nseg; ++s) {
    RN_CHECK_ARG(segs[s].rows >= 0, "regr terms: rows of segment %d is negative", s);
    RN_CHECK_ARG(segs[s].reg_pred && segs[s].reg_label, "regr terms: null reg_pred / reg_label in segment %d", s);
    if (bwd) RN_CHECK_ARG(segs[s].d_reg_pred, "regr terms bwd: null d_reg_pred in segment %d", s);
    else RN_CHECK_ARG(segs[s].cls_label && segs[s].trainable, "regr terms fwd: null cls_label / trainable in segment %d", s);
    RegrSeg& d = a->seg[s];
    d.ll = segs[s].cls_label; d.rp = segs[s].reg_pred; d.rl = segs[s].reg_label; d.tm = segs[s].trainable; d.dr = segs[s].d_reg_pred;
    d.row_start = rows;
    rows += segs[s].rows;
  }
  a->total_rows = rows;
  return RN_OK;
}

int fwd_blocks(int64_t rows) {
  const int64_t b = (rows + RPB - 1) / RPB;
  return (int)(b > FWD_BLOCKS ? FWD_BLOCKS : (b < 1 ? 1 : b));
}
int bwd_blocks(int64_t rows) {
  const int64_t b = (rows + T - 1) / T;
  return (int)(b > BWD_BLOCKS ? BWD_BLOCKS : (b < 1 ? 1 : b));
}
}  // namespace

extern "C" size_t rn_regr_terms_workspace(const rn_loss_seg*, int, int, const rn_regr_terms* t) {
  if (validate(t) != RN_OK) return 0;
  return (size_t)FWD_BLOCKS * PW * sizeof(float);
}

extern "C" int rn_regr_terms_fwd(const rn_loss_seg* segs, int nseg, int num_classes, const rn_regr_terms* t, float* stats,
                                 float* regr_loss_out, uint8_t* fg_rows, void* workspace, size_t workspace_bytes, rn_stream_t stream) {
  if (int e = validate(t)) return e;
  RegrArgs a = {};
  if (int e = build(segs, nseg, t, &a, false)) return e;
  RN_CHECK_ARG(num_classes >= 1, "regr terms fwd: num_classes %d < 1", num_classes);
  RN_CHECK_ARG(stats && fg_rows && workspace, "regr terms fwd: null stats / fg_rows / workspace");
  if (workspace_bytes < rn_regr_terms_workspace(segs, nseg, num_classes, t)) {
    rn::set_error("regr terms fwd: workspace too small");
    return RN_EWORKSPACE;
  }
  a.C = num_classes; a.partial = (float*)workspace; a.stats = stats; a.reg_out = regr_loss_out; a.fg_rows = fg_rows;
  hipStream_t st = (hipStream_t)stream;
  const int nb = fwd_blocks(a.total_rows);
  if (num_classes % 4 == 0) hipLaunchKernelGGL(regr_reduce_kernel<true>, dim3(nb), dim3(T), 0, st, a);
  else hipLaunchKernelGGL(regr_reduce_kernel<false>, dim3(nb), dim3(T), 0, st, a);
  hipLaunchKernelGGL(regr_finalize_kernel, dim3(1), dim3(T), 0, st, a, nb);
  RN_LAUNCH_CHECK();
  return RN_OK;
}

extern "C" int rn_regr_terms_bwd(const rn_loss_seg* segs, int nseg, const rn_regr_terms* t, const float* stats, const uint8_t* fg_rows,
                                 const float* g_reg, rn_stream_t stream) {
  if (int e = validate(t)) return e;
  RegrArgs a = {};
  if (int e = build(segs, nseg, t, &a, true)) return e;
  RN_CHECK_ARG(stats && fg_rows && g_reg, "regr terms bwd: null stats / fg_rows / g_reg");
  a.stats = const_cast<float*>(stats); a.fg_rows = const_cast<uint8_t*>(fg_rows); a.g_reg = g_reg;
  if (a.total_rows == 0) return RN_OK;
  hipLaunchKernelGGL(regr_grad_kernel, dim3(bwd_blocks(a.total_rows)), dim3(T), 0, (hipStream_t)stream, a);
  RN_LAUNCH_CHECK();
  return RN_OK;
}
