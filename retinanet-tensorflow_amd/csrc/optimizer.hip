// Optimizer apply on one flat fp32 parameter arena (train.py:111-134,221):
//   g' = grad*grad_scale + wd*w            (L2 regulariser gradient, scale per parameter)
//   g' *= clip/max(||g'||, clip)           (tf.clip_by_global_norm, optional)
//   Momentum(0.9) | RMSProp(0.9, 0.9, 1e-10) | Adam(0.9, 0.999, 1e-8)   [TF-sem]
// HBM-bound: one pass, float4 accesses; 16-20 B/element (+8 with the moving average of the weights kept by the same pass).
#include "rn_common.h"

namespace {
constexpr int T = 256;
constexpr int NB = 1024;  // reduction blocks

__global__ __launch_bounds__(T) void norm_reg_kernel(const float* __restrict__ w, const float* __restrict__ g,
                                                     const float* __restrict__ wd, int64_t count, float gs,
                                                     double* __restrict__ partial) {
  __shared__ double red[2][T / 64];
  double n2 = 0.0, rg = 0.0;
  const int64_t nquad = count / 4;  // count is a multiple of RN_OPT_BLOCK
  for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < nquad; i += (int64_t)gridDim.x * T) {
    const float d = wd[(i * 4) / RN_OPT_BLOCK];
    const float4 wv = *reinterpret_cast<const float4*>(w + i * 4);
    const float4 gv = *reinterpret_cast<const float4*>(g + i * 4);
    const float t0 = gv.x * gs + d * wv.x, t1 = gv.y * gs + d * wv.y, t2 = gv.z * gs + d * wv.z, t3 = gv.w * gs + d * wv.w;
    n2 += (double)(t0 * t0 + t1 * t1 + t2 * t2 + t3 * t3);
    rg += (double)(0.5f * d * (wv.x * wv.x + wv.y * wv.y + wv.z * wv.z + wv.w * wv.w));
  }
  n2 = rn::wave_sum_d(n2); rg = rn::wave_sum_d(rg);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[0][wave] = n2; red[1][wave] = rg; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, b = 0.0;
    for (int i = 0; i < T / 64; ++i) { a += red[0][i]; b += red[1][i]; }
    partial[blockIdx.x * 2] = a; partial[blockIdx.x * 2 + 1] = b;
  }
}

__global__ void norm_reg_finalize_kernel(const double* __restrict__ partial, int nb, float* __restrict__ out2) {
  // one wave; lane-strided fixed-order sums
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nb; i += 64) { a += partial[2 * i]; b += partial[2 * i + 1]; }
  a = rn::wave_sum_d(a); b = rn::wave_sum_d(b);
  if (threadIdx.x == 0) { out2[0] = (float)a; out2[1] = (float)b; }
}

// NORM: the pass that applies the update also forms this launch's share of (sum g'^2, L2 regulariser value) -- both at the
// weights BEFORE the update, as rn_grad_norm_l2reg does -- into partial[block] (no clipping then: the norm is not an input)
// EMA: the pass also keeps the exponential moving average of the weights (tf.train.ExponentialMovingAverage): with w' the
// weight this launch stores and om = ema_dev[1] = 1 - d(n), what rn_step_control_eval left on the device, e <- e - (e - w') * om.
// The two EMA arguments are not read by the EMA = false instantiations.
// ACC (RN_OPT_F_ACCUM): the pass sums the gradients of A launches in `acc` and applies their mean on the A-th.  Every wave
// reads accum_dev = [p, applying], what rn_step_control_eval left on the device, once (a uniform load, like lr_dev[1]) and runs ONE
// of three loops: p == 0 and not applying, acc = g * gs (acc is not read); 0 < p and not applying, acc += g * gs; applying, the
// update from G = (acc + g * gs) * inv_accum in the place of g * gs (acc is not written: the next cycle's first launch overwrites
// it).  The two accumulating loops touch nothing but acc and leave the block's `partial` pair as the last update wrote it; the
// dropout counter advances in every launch.  The three accumulation arguments are not read by the ACC = false instantiations.
// GATE (RN_OPT_F_GATE; never with ACC): `accum_dev` carries gate_dev = [0, finite], what rn_step_control_eval left on the
// device in accum_dev's layout.  Every wave reads its second word once (a uniform load, like lr_dev[1]); on 0 the launch returns
// behind the dropout counter's bump and touches neither w nor the slots nor ema.  No argument was added for it: the argument
// block, and with it the code of the GATE = false instantiations, is what it was without the parameter.
template <int KIND, bool NORM, bool EMA, bool ACC, bool GATE = false>
__global__ __launch_bounds__(T) void opt_step_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                     float* __restrict__ s1, float* __restrict__ s2,
                                                     const float* __restrict__ wd, int64_t count, float lr, float gs,
                                                     float clip, const float* __restrict__ norm_sq, unsigned long long* advance, unsigned long long advance_by,
                                                     double* __restrict__ partial, const float* __restrict__ lr_dev,
                                                     float* __restrict__ ema, const float* __restrict__ ema_dev,
                                                     float* __restrict__ acc, float inv_accum, const int* __restrict__ accum_dev) {
  __shared__ double red[2][T / 64];
  double n2 = 0.0, rg = 0.0;
  if (lr_dev) lr = lr_dev[1];  // the rate rn_step_control_eval left on the device: one uniform load per wave, ahead of the loop
  float om = 0.f;
  if (EMA) om = ema_dev[1];  // 1 - d(n) of this update, likewise
  if (advance && blockIdx.x == 0 && threadIdx.x == 0) *advance += advance_by;  // the step counter the dropout masks hash (fresh masks next step)
  static_assert(!(GATE && ACC), "the gate and the accumulation phase share one argument");
  if (GATE) {
    if (accum_dev[1] == 0) return;  // gate_dev[1]: a non-finite gradient norm, this step's update does not happen
  }
  float cs = 1.f;
  if (clip > 0.f) {
    const float gn = sqrtf(norm_sq[0]);
    cs = clip / fmaxf(gn, clip);
  }
  const int64_t nquad = count / 4;
  if (ACC) {
    const int phase = accum_dev[0];
    if (accum_dev[1] == 0) {  // not the cycle's last launch: the sum only
      if (phase == 0) {
        for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < nquad; i += (int64_t)gridDim.x * T) {
          const float4 gv = *reinterpret_cast<const float4*>(g + i * 4);
          *reinterpret_cast<float4*>(acc + i * 4) = make_float4(gv.x * gs, gv.y * gs, gv.z * gs, gv.w * gs);
        }
      } else {
        for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < nquad; i += (int64_t)gridDim.x * T) {
          const float4 gv = *reinterpret_cast<const float4*>(g + i * 4);
          const float4 cv = *reinterpret_cast<const float4*>(acc + i * 4);
          *reinterpret_cast<float4*>(acc + i * 4) = make_float4(cv.x + gv.x * gs, cv.y + gv.y * gs, cv.z + gv.z * gs, cv.w + gv.w * gs);
        }
      }
      return;
    }
  }
  const float sc = ACC ? 1.f : gs;  // applying an accumulated gradient: G below carries the scale already
  for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < nquad; i += (int64_t)gridDim.x * T) {
    const float d = wd[(i * 4) / RN_OPT_BLOCK];
    float4 wv = *reinterpret_cast<float4*>(w + i * 4);
    float4 gv = *reinterpret_cast<const float4*>(g + i * 4);
    if (ACC) {  // G, the mean of the cycle's gradients, stands where g * gs stood
      const float4 cv = *reinterpret_cast<const float4*>(acc + i * 4);
      gv.x = (cv.x + gv.x * gs) * inv_accum; gv.y = (cv.y + gv.y * gs) * inv_accum;
      gv.z = (cv.z + gv.z * gs) * inv_accum; gv.w = (cv.w + gv.w * gs) * inv_accum;
    }
    float4 av = *reinterpret_cast<float4*>(s1 + i * 4);
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (KIND != RN_OPT_MOMENTUM) bv = *reinterpret_cast<float4*>(s2 + i * 4);
    float4 ev = make_float4(0.f, 0.f, 0.f, 0.f);
    if (EMA) ev = *reinterpret_cast<float4*>(ema + i * 4);
    float* wp = &wv.x; const float* gp = &gv.x; float* ap = &av.x; float* bp = &bv.x; float* ep = &ev.x;
    if (NORM) {
      const float t0 = gv.x * sc + d * wv.x, t1 = gv.y * sc + d * wv.y, t2 = gv.z * sc + d * wv.z, t3 = gv.w * sc + d * wv.w;
      n2 += (double)(t0 * t0 + t1 * t1 + t2 * t2 + t3 * t3);
      rg += (double)(0.5f * d * (wv.x * wv.x + wv.y * wv.y + wv.z * wv.z + wv.w * wv.w));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gg = (gp[j] * sc + d * wp[j]) * cs;
      if (KIND == RN_OPT_MOMENTUM) {
        ap[j] = 0.9f * ap[j] + gg;
        wp[j] -= lr * ap[j];
      } else if (KIND == RN_OPT_RMSPROP) {
        ap[j] = 0.9f * ap[j] + 0.1f * gg * gg;
        bp[j] = 0.9f * bp[j] + lr * gg / sqrtf(ap[j] + 1e-10f);
        wp[j] -= bp[j];
      } else {
        ap[j] = 0.9f * ap[j] + 0.1f * gg;
        bp[j] = 0.999f * bp[j] + 0.001f * gg * gg;
        wp[j] -= lr * ap[j] / (sqrtf(bp[j]) + 1e-8f);  // lr already carries the bias correction
      }
      if (EMA) ep[j] -= (ep[j] - wp[j]) * om;
    }
    *reinterpret_cast<float4*>(w + i * 4) = wv;
    *reinterpret_cast<float4*>(s1 + i * 4) = av;
    if (KIND != RN_OPT_MOMENTUM) *reinterpret_cast<float4*>(s2 + i * 4) = bv;
    if (EMA) *reinterpret_cast<float4*>(ema + i * 4) = ev;
  }
  if (NORM) {
    n2 = rn::wave_sum_d(n2); rg = rn::wave_sum_d(rg);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[0][wave] = n2; red[1][wave] = rg; }
    __syncthreads();
    if (threadIdx.x == 0) {
      double a = 0.0, b = 0.0;
      for (int i = 0; i < T / 64; ++i) { a += red[0][i]; b += red[1][i]; }
      partial[blockIdx.x * 2] = a; partial[blockIdx.x * 2 + 1] = b;
    }
  }
}

unsigned grid_for(int64_t nquad) {
  int64_t b = (nquad + T - 1) / T;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (unsigned)b;
}
}  // namespace

extern "C" size_t rn_optimizer_workspace(int64_t) { return (size_t)NB * 2 * sizeof(double); }

extern "C" int rn_grad_norm_l2reg(const float* w, const float* grad, const float* wd_per_block, int64_t count,
                                  float grad_scale, float* out2, void* workspace, size_t workspace_bytes,
                                  rn_stream_t stream) {
  RN_CHECK_ARG(w && grad && wd_per_block && out2 && workspace, "grad_norm: null pointer");
  RN_CHECK_ARG(count > 0 && count % RN_OPT_BLOCK == 0, "grad_norm: count %lld not a multiple of %d", (long long)count,
               RN_OPT_BLOCK);
  if (workspace_bytes < rn_optimizer_workspace(count)) { rn::set_error("grad_norm: workspace too small"); return RN_EWORKSPACE; }
  unsigned nb = grid_for(count / 4);
  if (nb > NB) nb = NB;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(norm_reg_kernel, dim3(nb), dim3(T), 0, st, w, grad, wd_per_block, count, grad_scale, (double*)workspace);
  hipLaunchKernelGGL(norm_reg_finalize_kernel, dim3(1), dim3(64), 0, st, (const double*)workspace, (int)nb, out2);
  RN_LAUNCH_CHECK();
  return RN_OK;
}

extern "C" int rn_grad_norm_partial(const float* w, const float* grad, const float* wd_per_block, int64_t count, float grad_scale,
                                    double* partial, rn_stream_t stream) {
  RN_CHECK_ARG(w && grad && wd_per_block && partial, "grad_norm_partial: null pointer");
  RN_CHECK_ARG(count > 0 && count % RN_OPT_BLOCK == 0, "grad_norm_partial: count %lld not a multiple of %d", (long long)count,
               RN_OPT_BLOCK);
  // grid_for's grid, not the NB-capped one of rn_grad_norm_l2reg: one pair per block = rn_optimizer_norm_pairs(count) pairs
  hipLaunchKernelGGL(norm_reg_kernel, dim3(grid_for(count / 4)), dim3(T), 0, (hipStream_t)stream, w, grad, wd_per_block, count,
                     grad_scale, partial);
  RN_LAUNCH_CHECK();
  return RN_OK;
}

extern "C" int64_t rn_optimizer_norm_pairs(int64_t count) { return count > 0 ? (int64_t)grid_for(count / 4) : 0; }

// The one update entry: `features` says which instantiation runs and which fields must be set -- a pointer that is null (or set)
// by mistake is refused, it does not select another kernel.  Every check stands ahead of the launch (include/rn_hip.h lists them).
extern "C" int rn_optimizer_update(const rn_opt_update* u, rn_stream_t stream) {
  RN_CHECK_ARG(u, "optimizer: null descriptor");
  const uint32_t f = u->features;
  const bool norm = f & RN_OPT_F_NORM, lrdev = f & RN_OPT_F_LRDEV, ema = f & RN_OPT_F_EMA, clip = f & RN_OPT_F_CLIP,
             accum = f & RN_OPT_F_ACCUM, gate = f & RN_OPT_F_GATE;
  const int kind = u->kind;
  const int64_t count = u->count;
  RN_CHECK_ARG(u->w && u->grad && u->state1 && u->wd_per_block, "optimizer: null pointer");
  RN_CHECK_ARG(count > 0 && count % RN_OPT_BLOCK == 0, "optimizer: count %lld not a multiple of %d", (long long)count, RN_OPT_BLOCK);
  RN_CHECK_ARG(kind == RN_OPT_MOMENTUM || kind == RN_OPT_RMSPROP || kind == RN_OPT_ADAM, "optimizer: unknown kind %d", kind);
  RN_CHECK_ARG(kind == RN_OPT_MOMENTUM || u->state2, "optimizer: state2 required for rmsprop/adam");
  RN_CHECK_ARG(!(f & ~(uint32_t)(RN_OPT_F_NORM | RN_OPT_F_LRDEV | RN_OPT_F_EMA | RN_OPT_F_CLIP | RN_OPT_F_ACCUM | RN_OPT_F_GATE)),
               "optimizer: unknown feature bit in 0x%x", (unsigned)f);
  RN_CHECK_ARG(!norm || (!clip && !gate), "optimizer: NORM (the fused norm) goes with neither CLIP nor GATE: the norm is their input");
  RN_CHECK_ARG(!accum || (norm && !clip && !gate), "optimizer: ACCUM needs NORM and goes with neither CLIP nor GATE");
  RN_CHECK_ARG((u->partial != nullptr) == norm, "optimizer: partial is set with NORM and only with it");
  RN_CHECK_ARG((u->lr_dev != nullptr) == lrdev, "optimizer: lr_dev (the device rate) is set with LRDEV and only with it");
  RN_CHECK_ARG((u->ema != nullptr) == ema && (u->ema_dev != nullptr) == ema, "optimizer: ema and ema_dev go together, with EMA and only with it");
  RN_CHECK_ARG(((uintptr_t)u->ema & 15) == 0, "optimizer: ema is not 16-byte aligned");
  RN_CHECK_ARG((u->acc != nullptr) == accum && (u->accum_dev != nullptr) == accum,
               "optimizer: acc and accum_dev go together, with ACCUM and only with it");
  RN_CHECK_ARG(((uintptr_t)u->acc & 15) == 0, "optimizer: acc is not 16-byte aligned");
  RN_CHECK_ARG(!accum || (u->inv_accum > 0.f && u->inv_accum <= 1.f), "optimizer: inv_accum %g outside (0, 1]", (double)u->inv_accum);
  RN_CHECK_ARG((u->gate_dev != nullptr) == gate, "optimizer: gate_dev is set with GATE and only with it");
  RN_CHECK_ARG(((uintptr_t)u->gate_dev & 3) == 0, "optimizer: gate_dev is not 4-byte aligned");
  RN_CHECK_ARG(clip ? u->clip_norm > 0.f : u->clip_norm == 0.f, "optimizer: clip_norm %g (above 0 with CLIP, 0 without)", (double)u->clip_norm);
  RN_CHECK_ARG((u->norm_sq != nullptr) == clip, "optimizer: norm_sq is set with CLIP and only with it");
  float lr_eff = u->lr;  // LRDEV: the kernel reads its rate from lr_dev[1] -- bias correction included -- and `lr` / `step` are not used
  if (kind == RN_OPT_ADAM && !lrdev) {
    RN_CHECK_ARG(u->step >= 1, "optimizer: adam step must be >= 1");
    lr_eff = (float)((double)u->lr * sqrt(1.0 - pow(0.999, (double)u->step)) / (1.0 - pow(0.9, (double)u->step)));
  }
  const unsigned nb = grid_for(count / 4);
  hipStream_t st = (hipStream_t)stream;
  // the gate travels in accum_dev's slot (never both); inv_accum is 1 without ACCUM
#define RN_OPT_ARGS                                                                                                              \
  u->w, u->grad, u->state1, u->state2, u->wd_per_block, count, lr_eff, u->grad_scale, u->clip_norm, u->norm_sq,                   \
      (unsigned long long*)u->advance_counter, (unsigned long long)u->advance_by, u->partial, u->lr_dev, u->ema, u->ema_dev, u->acc, \
      accum ? u->inv_accum : 1.f, (const int*)(gate ? u->gate_dev : u->accum_dev)
#define RN_OPT_LAUNCH(KIND_)                                                                                                    \
  do {                                                                                                                          \
    if (gate && ema) hipLaunchKernelGGL((opt_step_kernel<KIND_, false, true, false, true>), dim3(nb), dim3(T), 0, st, RN_OPT_ARGS); \
    else if (gate) hipLaunchKernelGGL((opt_step_kernel<KIND_, false, false, false, true>), dim3(nb), dim3(T), 0, st, RN_OPT_ARGS); \
    else if (accum && ema) hipLaunchKernelGGL((opt_step_kernel<KIND_, true, true, true>), dim3(nb), dim3(T), 0, st, RN_OPT_ARGS);   \
    else if (accum) hipLaunchKernelGGL((opt_step_kernel<KIND_, true, false, true>), dim3(nb), dim3(T), 0, st, RN_OPT_ARGS);     \
    else if (ema && norm) hipLaunchKernelGGL((opt_step_kernel<KIND_, true, true, false>), dim3(nb), dim3(T), 0, st, RN_OPT_ARGS); \
    else if (ema) hipLaunchKernelGGL((opt_step_kernel<KIND_, false, true, false>), dim3(nb), dim3(T), 0, st, RN_OPT_ARGS);      \
    else if (norm) hipLaunchKernelGGL((opt_step_kernel<KIND_, true, false, false>), dim3(nb), dim3(T), 0, st, RN_OPT_ARGS);     \
    else hipLaunchKernelGGL((opt_step_kernel<KIND_, false, false, false>), dim3(nb), dim3(T), 0, st, RN_OPT_ARGS);              \
  } while (0)
  if (kind == RN_OPT_MOMENTUM) RN_OPT_LAUNCH(RN_OPT_MOMENTUM);
  else if (kind == RN_OPT_RMSPROP) RN_OPT_LAUNCH(RN_OPT_RMSPROP);
  else RN_OPT_LAUNCH(RN_OPT_ADAM);
#undef RN_OPT_LAUNCH
#undef RN_OPT_ARGS
  RN_LAUNCH_CHECK();
  return RN_OK;
}

namespace {
// d(n) of the EMA feature of rn_step_control (include/rn_hip.h) and its complement, each formed in double and rounded to float once
__device__ void ema_decay_eval(double decay, int warmup, unsigned long long* num_updates_dev, float* ema_dev) {
  const unsigned long long n = *num_updates_dev;
  double d = decay;
  if (warmup) d = fmin(decay, (1.0 + (double)n) / (10.0 + (double)n));
  ema_dev[0] = (float)d;
  ema_dev[1] = (float)(1.0 - d);
  *num_updates_dev = n + 1;
}

// lr(s) of rn_lr_schedule (include/rn_hip.h), in double; the caller rounds it to float once
__device__ double lr_schedule_value(const rn_lr_schedule& d, uint64_t s) {
  const double base = d.base_lr;
  if (s < (uint64_t)d.warmup_steps) return base * (d.warmup_factor + (1.0 - d.warmup_factor) * (double)s / (double)d.warmup_steps);
  if (d.kind == RN_LR_STEP) {
    int passed = 0;
    for (int i = 0; i < d.n_boundaries; ++i) passed += ((uint64_t)d.boundaries[i] <= s) ? 1 : 0;
    return base * pow(d.decay_factor, (double)passed);
  }
  if (d.kind == RN_LR_COSINE) {
    const double span = (double)(d.total_steps - d.warmup_steps);
    const double frac = fmin(1.0, (double)(s - (uint64_t)d.warmup_steps) / span);
    return base * (d.final_factor + (1.0 - d.final_factor) * 0.5 * (1.0 + cos(3.14159265358979323846 * frac)));
  }
  return base;
}

__device__ void lr_schedule_eval(const rn_lr_schedule& d, unsigned long long* step_dev, float* lr_dev, int opt_kind) {
  const unsigned long long s = *step_dev;
  const float lr = (float)lr_schedule_value(d, (uint64_t)s);
  float eff = lr;
  if (opt_kind == RN_OPT_ADAM) {
    const double t = (double)(s + 1);
    eff = (float)((double)lr * sqrt(1.0 - pow(0.999, t)) / (1.0 - pow(0.9, t)));
  }
  lr_dev[0] = lr;
  lr_dev[1] = eff;
  *step_dev = s + 1;
}

// The step's control words, one thread: the phase or the finite gate first (never both), then the schedule and the average's
// decay behind the gate either of them left -- a closed gate leaves lr_dev, ema_dev and the two words they count in untouched.
//   accum_dev   = [p, p == A - 1], p = micro-steps seen so far mod A; the word advances
//   gate_dev    = [0, sum g'^2 finite]: accum_dev's layout (opt_step_kernel reads either through one argument)
//   skipped_dev = [updates skipped in all, updates skipped in a row] (the second word starts again at an applied update)
__global__ void step_control_kernel(rn_step_control c) {
  int gate = 1;
  if (c.features & RN_CTL_F_ACCUM) {
    unsigned long long* micro_dev = (unsigned long long*)c.micro_dev;
    const unsigned long long m = *micro_dev;
    const int p = (int)(m % (unsigned long long)c.accumulate_steps);
    gate = (p == c.accumulate_steps - 1) ? 1 : 0;
    c.accum_dev[0] = p;
    c.accum_dev[1] = gate;
    *micro_dev = m + 1;
  }
  if (c.features & RN_CTL_F_GUARD) {
    unsigned long long* skipped_dev = (unsigned long long*)c.skipped_dev;
    const bool finite = isfinite(c.norm_sq[0]);
    gate = finite ? 1 : 0;
    c.gate_dev[0] = 0;
    c.gate_dev[1] = gate;
    if (finite) {
      skipped_dev[1] = 0ull;
    } else {
      skipped_dev[0] += 1ull;
      skipped_dev[1] += 1ull;
    }
  }
  if (!gate) return;
  if (c.features & RN_CTL_F_LR) lr_schedule_eval(c.schedule, (unsigned long long*)c.step_dev, c.lr_dev, c.optimizer_kind);
  if (c.features & RN_CTL_F_EMA) ema_decay_eval(c.ema_decay, c.ema_warmup, (unsigned long long*)c.ema_updates_dev, c.ema_dev);
}

int check_lr_schedule(const rn_lr_schedule& d) {
  RN_CHECK_ARG(d.kind == RN_LR_CONSTANT || d.kind == RN_LR_STEP || d.kind == RN_LR_COSINE, "step_control: unknown schedule kind %d", d.kind);
  RN_CHECK_ARG(d.warmup_steps >= 0, "step_control: warmup_steps %lld < 0", (long long)d.warmup_steps);
  RN_CHECK_ARG(d.warmup_factor >= 0.0 && d.warmup_factor <= 1.0 && d.final_factor >= 0.0 && d.final_factor <= 1.0,
               "step_control: warmup_factor %g / final_factor %g outside [0, 1]", d.warmup_factor, d.final_factor);
  RN_CHECK_ARG(d.n_boundaries >= 0 && d.n_boundaries <= RN_LR_MAX_BOUNDARIES, "step_control: %d boundaries, at most %d",
               d.n_boundaries, RN_LR_MAX_BOUNDARIES);
  for (int i = 0; i < d.n_boundaries; ++i)
    RN_CHECK_ARG(d.boundaries[i] >= 0 && (i == 0 || d.boundaries[i] > d.boundaries[i - 1]),
                 "step_control: boundaries must be non-negative and strictly increasing (entry %d)", i);
  RN_CHECK_ARG(d.total_steps > d.warmup_steps || (d.kind != RN_LR_COSINE && d.total_steps == 0),
               "step_control: total_steps %lld is not above warmup_steps %lld", (long long)d.total_steps, (long long)d.warmup_steps);
  return RN_OK;
}
}  // namespace

// The one control entry: `features` says which words the launch forms and which fields must be set -- a pointer that is null (or
// set) by mistake is refused, it does not select another behaviour.  Every check stands ahead of the launch.
extern "C" int rn_step_control_eval(const rn_step_control* c, rn_stream_t stream) {
  RN_CHECK_ARG(c, "step_control: null descriptor");
  const uint32_t f = c->features;
  const bool accum = f & RN_CTL_F_ACCUM, guard = f & RN_CTL_F_GUARD, lr = f & RN_CTL_F_LR, ema = f & RN_CTL_F_EMA;
  RN_CHECK_ARG(!(f & ~(uint32_t)(RN_CTL_F_ACCUM | RN_CTL_F_GUARD | RN_CTL_F_LR | RN_CTL_F_EMA)), "step_control: unknown feature bit in 0x%x",
               (unsigned)f);
  RN_CHECK_ARG(f != 0, "step_control: no feature set, nothing to launch");
  RN_CHECK_ARG(!(accum && guard), "step_control: ACCUM goes with no GUARD: the schedule and the average run behind ONE gate");
  RN_CHECK_ARG((c->micro_dev != nullptr) == accum && (c->accum_dev != nullptr) == accum,
               "step_control: micro_dev and accum_dev go together, with ACCUM and only with it");
  RN_CHECK_ARG(!accum || c->accumulate_steps >= 1, "step_control: accumulate_steps %d < 1", (int)c->accumulate_steps);
  RN_CHECK_ARG((c->norm_sq != nullptr) == guard && (c->gate_dev != nullptr) == guard && (c->skipped_dev != nullptr) == guard,
               "step_control: norm_sq, gate_dev and skipped_dev go together, with GUARD and only with it");
  RN_CHECK_ARG(((uintptr_t)c->norm_sq & 3) == 0 && ((uintptr_t)c->gate_dev & 3) == 0 && ((uintptr_t)c->skipped_dev & 7) == 0,
               "step_control: misaligned pointer (norm_sq 4, gate_dev 4, skipped_dev 8 bytes)");
  RN_CHECK_ARG((c->step_dev != nullptr) == lr && (c->lr_dev != nullptr) == lr, "step_control: step_dev and lr_dev go together, with LR and only with it");
  RN_CHECK_ARG(c->optimizer_kind == RN_OPT_MOMENTUM || c->optimizer_kind == RN_OPT_RMSPROP || c->optimizer_kind == RN_OPT_ADAM,
               "step_control: unknown optimizer kind %d", (int)c->optimizer_kind);
  if (lr)
    if (int rc = check_lr_schedule(c->schedule)) return rc;
  RN_CHECK_ARG((c->ema_updates_dev != nullptr) == ema && (c->ema_dev != nullptr) == ema,
               "step_control: ema_updates_dev and ema_dev go together, with EMA and only with it");
  RN_CHECK_ARG(!ema || (c->ema_decay > 0.0 && c->ema_decay < 1.0), "step_control: ema_decay %g outside (0, 1)", c->ema_decay);
  hipLaunchKernelGGL(step_control_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, *c);
  RN_LAUNCH_CHECK();
  return RN_OK;
}

extern "C" int rn_norm_reg_finalize(const double* partial, int64_t npairs, float* out2, rn_stream_t stream) {
  RN_CHECK_ARG(partial && out2 && npairs >= 1 && npairs < (1 << 30), "norm_reg_finalize: bad argument");
  hipLaunchKernelGGL(norm_reg_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partial, (int)npairs, out2);
  RN_LAUNCH_CHECK();
  return RN_OK;
}

namespace {
__global__ void counter_add_kernel(unsigned long long* c, unsigned long long inc) { *c += inc; }
}  // namespace

extern "C" int rn_counter_add(uint64_t* counter, uint64_t inc, rn_stream_t stream) {
  RN_CHECK_ARG(counter, "counter_add: null pointer");
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (unsigned long long*)counter, (unsigned long long)inc);
  RN_LAUNCH_CHECK();
  return RN_OK;
}

namespace {
__global__ __launch_bounds__(T) void zero_kernel(float* __restrict__ p, int64_t count) {
  const int64_t nquad = count / 4;
  for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < nquad; i += (int64_t)gridDim.x * T)
    *reinterpret_cast<float4*>(p + i * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
  if (blockIdx.x == 0 && threadIdx.x < (int)(count - nquad * 4)) p[nquad * 4 + threadIdx.x] = 0.f;
}
}  // namespace

extern "C" int rn_zero(float* p, int64_t count, rn_stream_t stream) {
  RN_CHECK_ARG(p && count >= 0 && ((uintptr_t)p & 15) == 0, "zero: null / unaligned pointer");
  if (count == 0) return RN_OK;
  hipLaunchKernelGGL(zero_kernel, dim3(grid_for(count / 4 + 1)), dim3(T), 0, (hipStream_t)stream, p, count);
  RN_LAUNCH_CHECK();
  return RN_OK;
}
