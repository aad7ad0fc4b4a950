// Running training metrics inside the captured step (build_metrics, train.py:137-161): the class confusion counts of
// tf.metrics.mean_iou(labels, sigmoid(logits) > 0.5, 2 classes) over the trainable anchors, the box IoU between the label box and
// the predicted box decoded at the ground-truth foreground anchors (utils.py:62-97,108-117,183-195), and the window sums of the
// step's losses.  Compiled with -ffp-contract=off: decode and IoU are rn::decode_one / rn::iou_corners (box_math.h), float32 op
// for op what rn_decode_boxes and rn_iou compute.
//
//   pass : ONE launch over every pyramid level (segments, as loss.hip).  FOUR lanes per row, 16 rows per wave and pass: the row's
//          lanes split its C logits / labels, lane 0 of a foreground row decodes both boxes.  C % 4 == 0, C <= 128 (every row then
//          starts on a 16-byte boundary): NK 16-byte loads per tensor and lane, two row groups in flight, all issued before the
//          first is used and before the row's mask is known (loss.hip's reduce4 shape: the same bytes, just read by the loss).
//          Any other C: 16-byte loads where the row's address allows them, a scalar head and tail otherwise.  Integer counts and
//          the fp64 IoU sum go lane -> wave (shuffles) -> block (LDS, wave order) -> one row of `partial` per block.  No atomics,
//          fixed order: eager and graph runs give the same bits.
//   fold : one block at the end of the step: the partial rows (integers: exact in any order; the IoU sums: index order inside 64
//          contiguous chunks, then the chunks in order), the step's loss scalars, the finiteness gate, the window state
//          (rn_hip.h: layout).  Plain stores.
#include "box_math.h"
#include "rn_common.h"

namespace {

constexpr int T = 256;
constexpr int WAVES = T / 64;
constexpr int RPW = 16;            // rows per wave and pass (4 lanes each)
constexpr int MAX_BLOCKS = 1024;   // partial rows (the fold reads MAX_BLOCKS / T of them per thread)
constexpr int NCOL = 6;            // tn, fp, fn, tp, iou_rows (int64), sum_iou (double)
constexpr int ROW_SLOTS = 8;       // 64-byte partial rows
constexpr int HEADER_SLOTS = 8;    // [0] = rows the last pass wrote
constexpr int CHUNKS = 64;         // of the fold's ordered IoU sum
static_assert((HEADER_SLOTS + MAX_BLOCKS * ROW_SLOTS) * sizeof(int64_t) == RN_TRAIN_METRICS_MAX_WORKSPACE_BYTES, "rn_hip.h");

struct MetSeg {
  const float* zl; const float* ll; const float* rp; const float* rl; const uint8_t* tm; const float* anch;
  int h, w, A;
  int64_t rows, row_start;
};
struct MetArgs {
  MetSeg seg[RN_MAX_SEG];
  int nseg, C;
  int64_t total_rows;
  int64_t* ws;                     // header + gridDim.x partial rows
};

__device__ __forceinline__ int seg_of_row(const MetArgs& a, int64_t r) {
  int s = 0;
  while (s + 1 < a.nseg && r >= a.seg[s + 1].row_start) ++s;
  return s;
}

struct Counts {
  int tn, fp, fn, tp, nbox;
  double iou_sum;
};

// one element of a trainable row: label positive iff > 0.5, prediction positive iff logit > 0 (rn_hip.h: the sigmoid note)
__device__ __forceinline__ void count_one(float z, float l, Counts& c, float& lmax) {
  const bool lab = l > 0.5f, pred = z > 0.f;
  c.tn += (!lab && !pred) ? 1 : 0; c.fp += (!lab && pred) ? 1 : 0;
  c.fn += (lab && !pred) ? 1 : 0;  c.tp += (lab && pred) ? 1 : 0;
  lmax = fmaxf(lmax, l);
}

// a trainable foreground row (utils.classmap_decode, utils.py:171-179): the label box and the predicted box at this anchor
__device__ __forceinline__ void box_iou(const MetSeg& sg, int64_t lr, Counts& c) {
  int64_t q = lr;
  const int an = (int)(q % sg.A); q /= sg.A;
  const int x_ = (int)(q % sg.w); q /= sg.w;
  const int y_ = (int)(q % sg.h);
  const float ah = sg.anch[an * 2], aw = sg.anch[an * 2 + 1];
  const float4 t = rn::decode_one(*reinterpret_cast<const float4*>(sg.rl + lr * 4), ah, aw, y_, x_, sg.h, sg.w);
  const float4 p = rn::decode_one(*reinterpret_cast<const float4*>(sg.rp + lr * 4), ah, aw, y_, x_, sg.h, sg.w);
  const float v = rn::iou_corners(t.x, t.y, t.z, t.w, (t.z - t.x) * (t.w - t.y), p.x, p.y, p.z, p.w);
  c.iou_sum += (double)v;
  c.nbox += 1;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// lane -> wave -> block -> this block's partial row; block 0 also leaves the row count in the header
__device__ __forceinline__ void store_partial(const MetArgs& a, Counts c) {
  __shared__ long long red_i[WAVES][NCOL - 1];
  __shared__ double red_d[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  c.tn = wave_sum_i(c.tn); c.fp = wave_sum_i(c.fp); c.fn = wave_sum_i(c.fn); c.tp = wave_sum_i(c.tp); c.nbox = wave_sum_i(c.nbox);
  c.iou_sum = rn::wave_sum_d(c.iou_sum);
  if (lane == 0) {
    red_i[wave][0] = c.tn; red_i[wave][1] = c.fp; red_i[wave][2] = c.fn; red_i[wave][3] = c.tp; red_i[wave][4] = c.nbox;
    red_d[wave] = c.iou_sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t* row = a.ws + HEADER_SLOTS + (size_t)blockIdx.x * ROW_SLOTS;
#pragma unroll
    for (int k = 0; k < NCOL - 1; ++k) {
      long long v = 0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) v += red_i[w][k];
      row[k] = v;
    }
    double d = 0.0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) d += red_d[w];
    reinterpret_cast<double*>(row)[NCOL - 1] = d;
    if (blockIdx.x == 0) a.ws[0] = (int64_t)gridDim.x;
  }
}

// any C
__global__ __launch_bounds__(T) void metrics_pass_kernel(const MetArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = a.C, j = lane & 3, r16 = lane >> 2;
  Counts c = {0, 0, 0, 0, 0, 0.0};
  const int64_t ngroups = (a.total_rows + RPW - 1) / RPW;
  const int64_t wave_id = (int64_t)blockIdx.x * WAVES + wave, nwaves = (int64_t)gridDim.x * WAVES;
  for (int64_t g = wave_id; g < ngroups; g += nwaves) {
    const int64_t r = min(g * RPW + r16, a.total_rows - 1);       // (a lane past the last row looks at it and counts nothing)
    const bool live = g * RPW + r16 < a.total_rows;
    const MetSeg& sg = a.seg[seg_of_row(a, r)];
    const int64_t lr = r - sg.row_start;
    const bool trainable = live && sg.tm[lr] != 0;
    float lmax = -1e30f;
    if (trainable) {
      const float* __restrict__ zrow = sg.zl + lr * C;
      const float* __restrict__ lrow = sg.ll + lr * C;
      // both rows start at the same element offset lr * C of 16-byte aligned tensors (checked by the entry): one split serves both
      const int mis = (int)((reinterpret_cast<uintptr_t>(zrow) >> 2) & 3);
      const int head = min(C, (4 - mis) & 3), nq = (C - head) >> 2, tail = C - head - 4 * nq;
      if (j < head) count_one(zrow[j], lrow[j], c, lmax);
#pragma unroll 4
      for (int q = j; q < nq; q += 4) {
        const float4 z = *reinterpret_cast<const float4*>(zrow + head + 4 * q);
        const float4 l = *reinterpret_cast<const float4*>(lrow + head + 4 * q);
        count_one(z.x, l.x, c, lmax); count_one(z.y, l.y, c, lmax); count_one(z.z, l.z, c, lmax); count_one(z.w, l.w, c, lmax);
      }
      if (j < tail) count_one(zrow[head + 4 * nq + j], lrow[head + 4 * nq + j], c, lmax);
    }
    lmax = fmaxf(lmax, __shfl_xor(lmax, 1, 64));
    lmax = fmaxf(lmax, __shfl_xor(lmax, 2, 64));
    if (trainable && j == 0 && lmax > 0.5f) box_iou(sg, lr, c);
  }
  store_partial(a, c);
}

// C % 4 == 0, C <= 16 * NK: lane (row, j) owns the class quads j, j + 4, ..; a lane past the row's last quad, or past the last row,
// re-reads a quad that exists (the clamp) and does not count it
template <int NK>
__global__ __launch_bounds__(T) void metrics_pass4_kernel(const MetArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = a.C, CQ = C >> 2, j = lane & 3, r16 = lane >> 2;
  Counts c = {0, 0, 0, 0, 0, 0.0};
  const int64_t ngroups = (a.total_rows + RPW - 1) / RPW;
  const int64_t wave_id = (int64_t)blockIdx.x * WAVES + wave, nwaves = (int64_t)gridDim.x * WAVES;
  for (int64_t g0 = wave_id * 2; g0 < ngroups; g0 += nwaves * 2) {
    float4 z[2][NK], l[2][NK];
    bool trainable[2];
    int segs[2];
    int64_t lrs[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t r = min((g0 + u) * RPW + r16, a.total_rows - 1);
      const bool live = (g0 + u) * RPW + r16 < a.total_rows;
      segs[u] = seg_of_row(a, r);
      const MetSeg& sg = a.seg[segs[u]];
      const int64_t lr = r - sg.row_start;
      lrs[u] = lr;
      trainable[u] = live && sg.tm[lr] != 0;
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
        if (trainable[u] && j + 4 * k < CQ) {
          count_one(z[u][k].x, l[u][k].x, c, lmax); count_one(z[u][k].y, l[u][k].y, c, lmax);
          count_one(z[u][k].z, l[u][k].z, c, lmax); count_one(z[u][k].w, l[u][k].w, c, lmax);
        }
      }
      lmax = fmaxf(lmax, __shfl_xor(lmax, 1, 64));
      lmax = fmaxf(lmax, __shfl_xor(lmax, 2, 64));
      if (trainable[u] && j == 0 && lmax > 0.5f) box_iou(a.seg[segs[u]], lrs[u], c);
    }
  }
  store_partial(a, c);
}

__device__ __forceinline__ bool finite_d(double v) { return v - v == 0.0; }

// state: doubles [sum_total, sum_class, sum_regr, sum_reg, sum_iou], int64 [steps, nonfinite_steps, tn, fp, fn, tp, iou_rows]
__global__ __launch_bounds__(T) void metrics_fold_kernel(const int64_t* __restrict__ ws, int max_rows, const float* class_loss,
                                                         const float* regr_loss, const float* reg_loss, int64_t* state) {
  __shared__ double iou_row[MAX_BLOCKS];
  __shared__ double iou_chunk[CHUNKS];
  __shared__ long long red_i[WAVES][NCOL - 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int n = (int)min((long long)ws[0], (long long)max_rows);     // (never more rows than the workspace the caller handed in holds)
  if (n < 0) n = 0;
  long long v[NCOL - 1] = {0, 0, 0, 0, 0};
#pragma unroll
  for (int u = 0; u < MAX_BLOCKS / T; ++u) {                    // every load of the block issued at once
    const int r = tid + u * T;
    if (r < n) {
      const int64_t* row = ws + HEADER_SLOTS + (size_t)r * ROW_SLOTS;
#pragma unroll
      for (int k = 0; k < NCOL - 1; ++k) v[k] += row[k];
      iou_row[r] = reinterpret_cast<const double*>(row)[NCOL - 1];
    }
  }
#pragma unroll
  for (int k = 0; k < NCOL - 1; ++k) {                          // integers: exact in any order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    if (lane == 0) red_i[wave][k] = v[k];
  }
  __syncthreads();
  if (tid < CHUNKS) {                                           // chunk t: rows [t * per, (t + 1) * per) in index order
    const int per = (n + CHUNKS - 1) / CHUNKS;
    double d = 0.0;
    for (int r = tid * per; r < min(n, (tid + 1) * per); ++r) d += iou_row[r];
    iou_chunk[tid] = d;
  }
  __syncthreads();
  if (tid == 0) {
    double iou = 0.0;
    for (int t = 0; t < CHUNKS; ++t) iou += iou_chunk[t];       // the chunks in order
    long long tot[NCOL - 1];
#pragma unroll
    for (int k = 0; k < NCOL - 1; ++k) {
      tot[k] = 0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) tot[k] += red_i[w][k];
    }
    const double cl = (double)class_loss[0], rl = (double)regr_loss[0], rg = (double)reg_loss[0];
    double* sd = reinterpret_cast<double*>(state);
    int64_t* si = state + 5;
    if (finite_d(cl) && finite_d(rl) && finite_d(rg) && finite_d(iou)) {
      sd[0] += (cl + rl) + rg; sd[1] += cl; sd[2] += rl; sd[3] += rg; sd[4] += iou;
      si[0] += 1;
      si[2] += tot[0]; si[3] += tot[1]; si[4] += tot[2]; si[5] += tot[3]; si[6] += tot[4];
    } else {
      si[1] += 1;
    }
  }
}

bool use4(int C) { return C % 4 == 0 && C >= 4 && C <= 128; }

int nblocks_for(int64_t rows, int C) {   // one pass per wave: 16 rows, or two groups of 16 in the four-aligned kernels
  const int per_block = RPW * WAVES * (use4(C) ? 2 : 1);
  int64_t b = (rows + per_block - 1) / per_block;
  if (b > MAX_BLOCKS) b = MAX_BLOCKS;
  if (b < 1) b = 1;
  return (int)b;
}

template <int NK>
void launch4(const MetArgs& a, int nb, hipStream_t st) {
  hipLaunchKernelGGL((metrics_pass4_kernel<NK>), dim3(nb), dim3(T), 0, st, a);
}

int build(const rn_metrics_seg* segs, int nseg, int C, MetArgs* a) {
  RN_CHECK_ARG(segs && nseg >= 1 && nseg <= RN_MAX_SEG, "train_metrics: bad segments");
  RN_CHECK_ARG(C >= 1, "train_metrics: num_classes %d", C);
  a->nseg = nseg; a->C = C;
  int64_t rows = 0;
  for (int s = 0; s < nseg; ++s) {
    const rn_metrics_seg& g = segs[s];
    RN_CHECK_ARG(g.cls_logit && g.cls_label && g.reg_pred && g.reg_label && g.trainable && g.anchor_sizes,
                 "train_metrics: null pointer in segment %d", s);
    RN_CHECK_ARG(g.n >= 1 && g.h >= 1 && g.w >= 1 && g.anchors >= 1, "train_metrics: bad shape in segment %d", s);
    RN_CHECK_ARG(((uintptr_t)g.cls_logit | (uintptr_t)g.cls_label | (uintptr_t)g.reg_pred | (uintptr_t)g.reg_label) % 16 == 0,
                 "train_metrics: segment %d: tensors must be 16-byte aligned", s);
    MetSeg& d = a->seg[s];
    d.zl = g.cls_logit; d.ll = g.cls_label; d.rp = g.reg_pred; d.rl = g.reg_label; d.tm = g.trainable; d.anch = g.anchor_sizes;
    d.h = g.h; d.w = g.w; d.A = g.anchors;
    d.rows = (int64_t)g.n * g.h * g.w * g.anchors; d.row_start = rows;
    rows += d.rows;
  }
  // lane and wave counters are 32-bit: with MAX_BLOCKS blocks a wave counts rows * C / (WAVES * MAX_BLOCKS) elements, < 2^28 here
  RN_UNSUPPORTED(rows * (int64_t)C >= (1ll << 40), "train_metrics: %lld rows x %d classes: too large", (long long)rows, C);
  a->total_rows = rows;
  return RN_OK;
}
}  // namespace

extern "C" size_t rn_train_metrics_workspace(const rn_metrics_seg* segs, int nseg, int num_classes) {
  MetArgs a = {};
  if (build(segs, nseg, num_classes, &a)) return 0;
  return (size_t)(HEADER_SLOTS + (size_t)nblocks_for(a.total_rows, num_classes) * ROW_SLOTS) * sizeof(int64_t);
}

extern "C" int rn_train_metrics_pass(const rn_metrics_seg* segs, int nseg, int num_classes, void* workspace,
                                     size_t workspace_bytes, rn_stream_t stream) {
  MetArgs a = {};
  if (int e = build(segs, nseg, num_classes, &a)) return e;
  RN_CHECK_ARG(workspace && (uintptr_t)workspace % 8 == 0, "train_metrics: null or misaligned workspace");
  const int nb = nblocks_for(a.total_rows, num_classes);
  if (workspace_bytes < (size_t)(HEADER_SLOTS + (size_t)nb * ROW_SLOTS) * sizeof(int64_t)) {
    rn::set_error("train_metrics: workspace too small");
    return RN_EWORKSPACE;
  }
  a.ws = (int64_t*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (use4(num_classes)) {
    switch ((num_classes / 4 + 3) / 4) {
      case 1: launch4<1>(a, nb, st); break;
      case 2: launch4<2>(a, nb, st); break;
      case 3: launch4<3>(a, nb, st); break;
      case 4: launch4<4>(a, nb, st); break;
      case 5: launch4<5>(a, nb, st); break;
      case 6: launch4<6>(a, nb, st); break;
      case 7: launch4<7>(a, nb, st); break;
      default: launch4<8>(a, nb, st); break;
    }
  } else {
    hipLaunchKernelGGL(metrics_pass_kernel, dim3(nb), dim3(T), 0, st, a);
  }
  RN_LAUNCH_CHECK();
  return RN_OK;
}

extern "C" int rn_train_metrics_fold(const void* workspace, size_t workspace_bytes, const float* class_loss,
                                     const float* regr_loss, const float* reg_loss, void* state, rn_stream_t stream) {
  RN_CHECK_ARG(workspace && class_loss && regr_loss && reg_loss && state, "train_metrics fold: null pointer");
  RN_CHECK_ARG((uintptr_t)workspace % 8 == 0 && (uintptr_t)state % 16 == 0,
               "train_metrics fold: workspace must be 8-byte and state 16-byte aligned");
  RN_CHECK_ARG(workspace_bytes >= HEADER_SLOTS * sizeof(int64_t), "train_metrics fold: workspace too small");
  int64_t max_rows = (int64_t)(workspace_bytes / sizeof(int64_t) - HEADER_SLOTS) / ROW_SLOTS;
  if (max_rows > MAX_BLOCKS) max_rows = MAX_BLOCKS;
  hipLaunchKernelGGL(metrics_fold_kernel, dim3(1), dim3(T), 0, (hipStream_t)stream, (const int64_t*)workspace, (int)max_rows,
                     class_loss, regr_loss, reg_loss, (int64_t*)state);
  RN_LAUNCH_CHECK();
  return RN_OK;
}

extern "C" int rn_train_metrics_reset(void* state, rn_stream_t stream) {
  RN_CHECK_ARG(state && (uintptr_t)state % 16 == 0, "train_metrics reset: null or misaligned state");
  return rn_zero((float*)state, RN_TRAIN_METRICS_STATE_BYTES / 4, stream);
}
