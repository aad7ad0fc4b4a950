// Box arithmetic shared by the kernels that must agree bit for bit: the anchor grid's cell centres (dataset.py:16-25), the
// anchor decode (utils.regression_postprocess, utils.py:100-117) and utils.iou (utils.py:62-97).  The ONLY copy of each:
// assign.hip, decode_nms.hip and train_metrics.hip include this header and are all compiled with -ffp-contract=off, so every
// float32 operation is rounded on its own, in the reference's order, whichever kernel runs it.
#pragma once
#include <hip/hip_runtime.h>

namespace rn {

// cell centre i of `size` cells: tf.linspace(cell/2, 1-cell/2, size)[i] in float32
// (dataset.py:16-25; [TF-sem] value = start + step*i, step = (stop-start)/(size-1))
__device__ __forceinline__ float cell_center(int i, int size) {
  const float cell = (float)(1.0 / (double)size);
  const float start = cell / 2.0f;
  if (size == 1) return start;
  const float stop = 1.0f - start;
  const float step = (stop - start) / (float)(size - 1);
  const float t = step * (float)i;
  return start + t;
}

// one anchor's box from its raw regression (utils.regression_postprocess, utils.py:100-117): the full-map kernel of
// rn_decode_boxes, the candidate-only path of det_emit_kernel and the training metrics' pass all call it (same bits)
__device__ __forceinline__ float4 decode_one(const float4 r, float ah, float aw, int y_, int x_, int h, int w) {
  const float sy = r.x * ah, sx = r.y * aw;
  const float bh = expf(r.z) * ah, bw = expf(r.w) * aw;
  const float cy = sy + cell_center(y_, h), cx = sx + cell_center(x_, w);
  const float hh = bh / 2.0f, hw = bw / 2.0f;
  return make_float4(cy - hh, cx - hw, cy + hh, cx + hw);
}

// utils.iou (utils.py:62-97) of two corner boxes, every float32 operation rounded on its own and in the reference's order
__device__ __forceinline__ float iou_corners(float a0, float a1, float a2, float a3, float area_a,
                                             float b0, float b1, float b2, float b3) {
  const float yt = fmaxf(a0, b0), xl = fmaxf(a1, b1), yb = fminf(a2, b2), xr = fminf(a3, b3);
  const bool invalid = (yb < yt) || (xr < xl);
  const float inter = (yb - yt) * (xr - xl);
  const float area_b = (b2 - b0) * (b3 - b1);
  const float den = (area_a + area_b) - inter;
  const float v = inter / den;
  return invalid ? 0.f : v;
}

}  // namespace rn
