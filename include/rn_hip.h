/*
 * rn_hip.h -- C ABI of librn_hip.so: the MI355X (gfx950) kernels behind the RetinaNet hot path.
 *
 * The reference (vshmyhlo/retinanet-tensorflow) has no FFI seam: its model/loss code calls
 * TensorFlow kernels directly.  This library is the drop-in for exactly those kernels; every
 * entry point cites the reference call site(s) whose TF op it replaces.  The Python host side
 * (retinanet-tensorflow_amd/) binds it with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; `stream` is a hipStream_t passed as void*.
 *   - all tensors are dense fp32, NHWC activations, HWIO conv kernels, [kh,kw,C] depthwise.
 *   - the caller owns every buffer (including workspaces); the library never allocates device
 *     memory, never synchronises and keeps no pointer after a call returns: every call only
 *     enqueues work on `stream` (hipGraph-capturable).
 *   - return value: 0 (RN_OK) or a negative rn_status; rn_last_error() has the text.
 *   - "segments": several independent problems that share one weight / one parameter set are
 *     passed as an array and run in ONE launch (the shared heads over P3..P7,
 *     reference retinanet.py:283-291).
 */
#ifndef RN_HIP_H
#define RN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* rn_stream_t;

enum rn_status {
  RN_OK = 0,
  RN_EINVAL = -1,       /* bad argument */
  RN_EUNSUPPORTED = -2, /* shape outside what the kernels cover */
  RN_EHIP = -3,         /* HIP runtime error at launch */
  RN_EWORKSPACE = -4    /* workspace too small */
};

enum rn_act { RN_ACT_NONE = 0, RN_ACT_RELU = 1, RN_ACT_ELU = 2, RN_ACT_RELU6 = 3, RN_ACT_SIGMOID = 4 };
enum rn_loss_mode { RN_LOSS_BCE_DICE = 0, RN_LOSS_FOCAL = 1 };
enum rn_opt { RN_OPT_MOMENTUM = 0, RN_OPT_RMSPROP = 1, RN_OPT_ADAM = 2 };

#define RN_MAX_SEG 16

/* caller-owned list that collects deferred row reductions (see "deferred gradient reductions" below) */
typedef struct rn_reduce_list rn_reduce_list;

/* Version of this header's ABI: bumped whenever an entry point's arguments or a struct layout change.  rn_version() returns
 * the value the library was built with; a caller built against another value must not call anything else. */
#define RN_API_VERSION 427
int rn_version(void);
const char* rn_last_error(void);

/* TF 'SAME' padding rule: out = ceil(n/s); before = max((out-1)s+k-n,0)/2. */
void rn_same_pad(int n, int k, int s, int* out, int* pad_before);

/* ------------------------------------------------------------------ dense convolution
 * Replaces tf.layers.Conv2D (Conv2D / Conv2DBackpropInput / Conv2DBackpropFilter kernels):
 * retinanet.py:39-46,55-62,87-94,100-106,127-145,170-201; mobilenet_v2.py:57-59,75-77,
 * 112-114,179-181; resnet.py:32-49,67-69,147-149; densenet.py:37,61-70,137,168.
 * padding='same' always (the reference never uses 'valid'); implicit GEMM on
 * v_mfma_f32_32x32x2_f32, fp32 in / fp32 accumulate.
 */
typedef struct rn_conv_seg {
  const float* x;    /* fwd,wgrad: input  [n,h,w,cin]                       */
  const float* wgt;  /* fwd,dgrad: kernel [kh,kw,cin,cout]                  */
  const float* bias; /* fwd: [cout] or NULL                                 */
  float* y;          /* fwd: output [n,oh,ow,cout]                          */
  const float* dy;   /* dgrad,wgrad: grad of output [n,oh,ow,cout]          */
  float* dx;         /* dgrad: grad of input [n,h,w,cin]                    */
  int32_t n, h, w;   /* input batch / height / width                        */
  int32_t cout;      /* may differ per segment in fwd/dgrad                 */
  int32_t x_ld;      /* 0: x (and dx) are dense [n,h,w,cin].  > 0: x / dx are the channel slice
                        [x_coff, x_coff+cin) of a buffer with x_ld channels per pixel (x, dx point at the
                        buffer's first element): lets two convs consume / fill halves of one tensor      */
  int32_t x_coff;
  int64_t wgt_bytes; /* fp16 convs (rn_conv2d_fwd_f16*): bytes of the packed-kernel buffer `wgt` points at.  The fragment-ordered
                        copy behind Wt is read only when this proves it is there (>= rn_pack_weights_f16_bytes); 0 = unknown:
                        a Wt-only buffer is assumed.  Ignored by the fp32 entry points. */
} rn_conv_seg;

typedef struct rn_conv_geom {
  int32_t kh, kw, stride, cin;
  int32_t groups; /* 0 or 1 = dense.  G > 1: grouped conv (ResNeXt cardinality, resnet.py:53-59): kernel
                     [kh,kw,cin/G,cout], output channels [g*cout/G,(g+1)*cout/G) read input channels
                     [g*cin/G,(g+1)*cin/G) */
} rn_conv_geom;

/* workspace: optional scratch for split-K (rn_conv2d_*_workspace bytes, 0 when the launch is large enough not to
 * want it): grids of a few tiles with a long reduction -- the stride-2 convs that make P6 / P7, the 4x4 and 8x8
 * pyramid maps -- are otherwise latency-bound on a handful of CUs.  NULL / too small => no split (never an error). */
size_t rn_conv2d_fwd_workspace(const rn_conv_seg* segs, int nseg, const rn_conv_geom* g);
size_t rn_conv2d_dgrad_workspace(const rn_conv_seg* segs, int nseg, const rn_conv_geom* g);
int rn_conv2d_fwd(const rn_conv_seg* segs, int nseg, const rn_conv_geom* g, void* workspace, size_t workspace_bytes,
                  rn_stream_t stream);
int rn_conv2d_dgrad(const rn_conv_seg* segs, int nseg, const rn_conv_geom* g, void* workspace, size_t workspace_bytes,
                    rn_stream_t stream);
/* ------------------------------------------------------------------ GroupNorm statistics from the producer
 * normalization.py:30 takes the moments of a conv output that this library has just had in registers: the conv /
 * depthwise forward can emit partial sums as a by-product -- per block, a row of (sum, sum of squares) pairs -- and the
 * GroupNorm that follows (rn_gn_params.stat_rows) merges the rows of its sample in a fixed order (fp64) while its
 * activations are in flight, then applies: one elementwise pass instead of a reduction + exchange + apply.  No block
 * waits for another, no atomics, bitwise reproducible.
 *   rows            : [n][rows_per_sample][width] pairs of floats, written by the producer, read by the GroupNorm
 *   rows_per_sample : m-tiles of a sample (conv) / pixel chunks of a sample (depthwise)
 *   per_group       : 0: width = channels (the conv's tiles cut through groups); 1: width = groups (a depthwise block owns
 *                     all channels of its pixels and folds them into groups itself)
 * The *_stats_rows functions return the bytes of `rows` and fill the layout fields, or return 0 when the shape cannot
 * produce rows (several segments, grouped conv, bias, split-K plan, a sample's pixels not a multiple of the tile height)
 * or the GroupNorm could not merge them cheaply (rn_group_norm_rows_ok): use the stand-alone GroupNorm then. */
typedef struct rn_gn_rows {
  void* rows;
  int32_t rows_per_sample, per_group, groups;
} rn_gn_rows;
size_t rn_conv2d_stats_rows(const rn_conv_seg* segs, int nseg, const rn_conv_geom* g, size_t workspace_bytes, int groups,
                            rn_gn_rows* layout);
/* rn_conv2d_fwd + the rows of y (one dense segment, no bias) */
int rn_conv2d_fwd_stats(const rn_conv_seg* segs, int nseg, const rn_conv_geom* g, void* workspace, size_t workspace_bytes,
                        const rn_gn_rows* rows, rn_stream_t stream);

/* Conv2D -> Dropout (-> the statistics of the GroupNorm behind it) as ONE launch: y = dropout(conv(x)), and `rows` (may be NULL) = the
 * partial sums of the DROPPED y in the layout rn_conv2d_dropout_rows reports -- DenseNet's composite function runs
 * 1x1 conv -> Dropout -> GroupNorm (densenet.py:61-67, 70-77, dropout: densenet.py:23): the conv's output is never stored un-dropped and
 * the GroupNorm does not read it twice.  The mask is rn_dropout's (keep element i of y iff hash(seed + *seed_dev, i) >= rate, scaled by
 * 1 / (1 - rate)): bit-identical to rn_conv2d_fwd followed by rn_dropout.  Dense 1x1 / stride-1 convs of one segment without bias, in
 * product mode 1 (rn_set_product_mode): rn_conv2d_dropout_rows sets *fused_ok = 0 and the call returns RN_EUNSUPPORTED elsewhere -- the
 * caller then runs rn_conv2d_fwd + rn_dropout.  rn_conv2d_dropout_rows returns the rows' bytes (0: no rows for this shape). */
size_t rn_conv2d_dropout_rows(const rn_conv_seg* segs, int nseg, const rn_conv_geom* g, int groups, rn_gn_rows* layout, int* fused_ok);
int rn_conv2d_fwd_dropout(const rn_conv_seg* segs, int nseg, const rn_conv_geom* g, float rate, uint64_t seed, const uint64_t* seed_dev,
                          const rn_gn_rows* rows, rn_stream_t stream);

/* dw[kh,kw,cin,cout] = sum over all segments (they share the kernel: shared heads);
 * split-K partial slabs go to `workspace`, reduced in fixed order (bitwise reproducible).
 * If accumulate != 0 the result is added to dw instead of overwriting it. */
size_t rn_conv2d_wgrad_workspace(const rn_conv_seg* segs, int nseg, const rn_conv_geom* g);
int rn_conv2d_wgrad(const rn_conv_seg* segs, int nseg, const rn_conv_geom* g, float* dw, int accumulate,
                    void* workspace, size_t workspace_bytes, rn_stream_t stream, rn_reduce_list* defer);

/* Both gradients of one convolution (segments: x, wgt, dy, dx as for the two calls above; dw overwritten).  Small
 * problems -- the backbone's 1x1 convs -- run as ONE launch whose blocks are of two kinds (data-gradient tiles and
 * weight-gradient splits); anything else falls back to rn_conv2d_dgrad (without split-K) + rn_conv2d_wgrad.
 * workspace: rn_conv2d_wgrad_workspace bytes. */
int rn_conv2d_bwd(const rn_conv_seg* segs, int nseg, const rn_conv_geom* g, float* dw, void* workspace,
                  size_t workspace_bytes, rn_stream_t stream, rn_reduce_list* defer);

/* dbias[cout] = sum over all segments / pixels of dy (the out_conv biases, retinanet.py:46-53). */
size_t rn_conv2d_bias_grad_workspace(int cout);
int rn_conv2d_bias_grad(const rn_conv_seg* segs, int nseg, const rn_conv_geom* g, float* dbias, void* workspace,
                        size_t workspace_bytes, rn_stream_t stream, rn_reduce_list* defer);

/* ------------------------------------------------------------------ what a convolution call launches (host only)
 * rn_conv2d_plan reports the kernels one rn_conv2d_fwd / _fwd_stats / _dgrad / _wgrad / _bwd call with the same arguments
 * launches.  It is the decision the entry points launch from: conv_fwd_impl, conv_dgrad_impl, conv_wgrad_impl and the body of
 * rn_conv2d_bwd (csrc/conv_gemm.hip) fill an rn_conv_plan_call and launch from it; the query stops them before the first
 * launch.  It runs on the host, touches no device and follows no data pointer: segs[].x / wgt / y / dy / dx / bias, dw and
 * workspace are only compared with NULL where the entry point does that.  Returns what the launch would return for the same
 * arguments (RN_EINVAL / RN_EUNSUPPORTED / RN_EWORKSPACE), RN_EINVAL for a NULL plan or an unknown op.
 *   op               RN_CONV_FWD, RN_CONV_FWD_STATS (stats_groups = the GroupNorm's group count; RN_EUNSUPPORTED where
 *                    rn_conv2d_stats_rows returns 0), RN_CONV_DGRAD, RN_CONV_WGRAD (accumulate, defer != 0: a defer list is
 *                    passed), RN_CONV_BWD (defer likewise)
 *   workspace[_bytes] what the caller will pass to the entry point (split-K and the patch matrix are declined without it)
 * Environment switches, as the entry points read them.  At every call: RN_CONV_CFG, RN_WGRAD_CFG, RN_WGRAD_SPLITS,
 * RN_NO_SPLITK, RN_NO_PHASE_DGRAD.  Once per process (first use): RN_STEM_DIRECT, RN_X3_CONV1X1, RN_X3_IM2COL,
 * RN_GCONV_DIRECT, RN_NO_MERGED_BWD, RN_X3_IM2COL_PIECE_MB.  The product mode (rn_set_product_mode) is read at every call.
 * rn_gemm_batched_plan: the same for rn_gemm_batched (the fp32 kernels in batched mode, or the split-bf16 product). */
enum rn_conv_op { RN_CONV_FWD = 0, RN_CONV_FWD_STATS = 1, RN_CONV_DGRAD = 2, RN_CONV_WGRAD = 3, RN_CONV_BWD = 4 };
enum rn_conv_path {
  RN_CONV_PATH_NONE = 0,
  RN_CONV_PATH_DIRECT_GROUPED = 1, /* grouped_conv.hip: 3x3 / stride 1, 4 / 8 / 16 / 32 channels per group */
  RN_CONV_PATH_STEM = 2,           /* stem_conv_fwd_kernel */
  RN_CONV_PATH_X3_1X1 = 3,         /* split-bf16 product on x itself (gemm_x3.hip) */
  RN_CONV_PATH_X3_PATCH = 4,       /* split-bf16 product of a patch matrix (im2col.hip) */
  RN_CONV_PATH_FP32 = 5,           /* the fp32 implicit GEMM of conv_gemm.hip */
  RN_CONV_PATH_MERGED_BWD = 6      /* conv_bwd_kernel: data-gradient tiles and weight-gradient splits in one launch */
};
enum rn_conv_load { RN_CONV_LOAD_SCALAR = 0, RN_CONV_LOAD_VEC4 = 1, RN_CONV_LOAD_VEC4_TAP = 2 /* tap-uniform K tiles */ };
enum rn_conv_reduce { RN_CONV_REDUCE_NONE = 0, RN_CONV_REDUCE_LAUNCHED = 1, RN_CONV_REDUCE_DEFERRED = 2 };
/* why rn_conv2d_bwd runs as two calls */
enum rn_conv_unmerged {
  RN_CONV_MERGED = 0,
  RN_CONV_UNMERGED_SWITCH = 1, /* RN_NO_MERGED_BWD */
  RN_CONV_UNMERGED_X3_1X1 = 2, /* the split-bf16 1x1 kernels take the conv */
  RN_CONV_UNMERGED_DIRECT = 3, /* the direct grouped kernels take it */
  RN_CONV_UNMERGED_PATCH = 4,  /* the patch-matrix path takes it */
  RN_CONV_UNMERGED_SHAPE = 5   /* the fp32 plans do not fit the merged kernel: more than 4 (pseudo-)segments, scalar loads, a
                                  data-gradient tile other than 64 x 64, phase decomposition */
};
typedef struct rn_conv_plan_call {
  int32_t path;            /* enum rn_conv_path */
  /* fp32 kernels (path FP32, and both halves of MERGED_BWD) */
  int32_t cfg;             /* tile shape: 0 128x128, 1 128x64, 2 64x64, 3 128x32 */
  int32_t load;            /* enum rn_conv_load */
  int32_t nsplit;          /* fwd / dgrad: split-K ranges (1: none).  wgrad: splits of the pixel range, all segments */
  int32_t ksplit;          /* fwd / dgrad: K tiles per range (0: no split-K).  wgrad: `chunk`, pixels per split */
  int32_t blocks;          /* grid size of the conv kernel */
  int32_t grouped;         /* groups > 1 */
  int32_t batched;         /* number of batched products (rn_gemm_batched; 1 otherwise) */
  /* data gradient */
  int32_t phases;          /* stride 2: phase pseudo-segments (0: not decomposed) */
  int32_t phases_no_taps;  /* ... of which see no filter tap (they store zeros) */
  /* weight gradient */
  int32_t windows;         /* a split is longer than the kernel's 1024-pixel table and walks its range in windows */
  int32_t direct;          /* one split, written straight into dw (no slab, no reduction) */
  int32_t reduce;          /* enum rn_conv_reduce: the final row reduction */
  /* split-bf16 paths */
  int32_t m_tile;          /* m-tile rows: 64 or 128 */
  int32_t n_piece;         /* patch matrix, forward: samples per piece (n / n_piece pieces) */
  int64_t patch_bytes;     /* patch matrix: its bytes (of one piece) */
  /* RN_CONV_FWD_STATS */
  int32_t rows_per_sample;
  int32_t reserved_;
} rn_conv_plan_call;
typedef struct rn_conv_plan {
  rn_conv_plan_call call;         /* the call (RN_CONV_BWD: path MERGED_BWD with blocks = both halves', or NONE when not merged) */
  rn_conv_plan_call dgrad, wgrad; /* RN_CONV_BWD: the two halves (merged) / the two calls it runs instead */
  int32_t unmerged;               /* RN_CONV_BWD: enum rn_conv_unmerged */
  int32_t reserved_;
} rn_conv_plan;
int rn_conv2d_plan(const rn_conv_seg* segs, int nseg, const rn_conv_geom* g, int op, int stats_groups, int accumulate, int defer,
                   const float* dw, const void* workspace, size_t workspace_bytes, rn_conv_plan* plan);
int rn_gemm_batched_plan(const float* A, const float* B, const float* C, int M, int K, int N, int nbatch, int b_nk, rn_conv_plan* plan);

/* ------------------------------------------------------------------ deferred gradient reductions
 * Every weight-gradient entry point (rn_conv2d_wgrad, rn_conv2d_bwd, rn_depthwise_wgrad, rn_depthwise_bwd,
 * rn_conv2d_bias_grad, the GroupNorm parameter gradients of rn_group_norm_bwd, rn_reduce_rows) ends with a
 * fixed-order row reduction of per-block partial results.  A training step has ~130 of them, each a
 * launch-latency-bound kernel.  Each of those entry points therefore takes a trailing `rn_reduce_list* defer`:
 * NULL = reduce now; otherwise the reduction is only RECORDED in the caller's list (host memory the caller owns:
 * the library keeps nothing between calls) and rn_flush_reductions(list, stream) runs everything recorded as one
 * launch (per 140) and empties the list.  While deferring, the `workspace` handed to those entry points must stay
 * untouched until the flush (give each call its own buffer), and the gradients are only valid after the flush.
 * Results are bitwise identical to immediate mode, except the GroupNorm dgamma / dbeta of maps too large for the
 * single-kernel path, whose chunk rows are then summed in fp32 (fixed order) instead of fp64.
 * A full list is an error (RN_EWORKSPACE), never a silent immediate launch. */
typedef struct rn_reduce_desc {
  const float* in;   /* [nrows][count] partial rows */
  float* out;        /* [count] */
  int32_t count;
  uint16_t nrows, accumulate;
} rn_reduce_desc;
struct rn_reduce_list {
  rn_reduce_desc* desc; /* caller-owned array of `capacity` entries */
  int32_t capacity;
  int32_t count;        /* entries recorded so far */
};
int rn_flush_reductions(rn_reduce_list* list, rn_stream_t stream);

/* ------------------------------------------------------------------ Winograd F(m x m, 3x3) convolution
 * The 3x3 / stride-1 / SAME dense convolutions of the head towers and FPN merges (retinanet.py:39-46,87-94,
 * 138-145) with 2.25x (tile = 2) or 4x (tile = 4) fewer multiply-adds: input transform -> (tile+2)^2 batched
 * GEMMs on the fp32 matrix cores -> output transform (+ bias).  Segment fields as rn_conv2d_fwd (x, y, n, h, w;
 * dense NHWC).  w is always the forward kernel [3,3,cin,cout]; with dgrad != 0 the call computes
 * dx = conv(dy, rot180(w)^T) from the segments' dy / dx instead (the weight gradient keeps the direct
 * rn_conv2d_wgrad).  cin and cout multiples of 4.  Results differ from the direct kernels only by the fp32
 * rounding of the transforms (about 1e-6 of the output range for tile 2, 1e-5 for tile 4; tests: <= 1e-4). */
size_t rn_conv3x3_winograd_workspace(const rn_conv_seg* segs, int nseg, int cin, int cout, int tile);
/* v_buf / urot_buf (optional, caller-owned, sizes from rn_conv3x3_winograd_keep_bytes) let a training step reuse two
 * intermediates instead of recomputing them in the backward pass: a forward call (dgrad == 0) writes the transformed
 * input into v_buf (rn_conv3x3_winograd_wgrad then skips its input transform) and the transformed ROTATED kernel into
 * urot_buf (same launch as the forward kernel transform); a data-gradient call (dgrad != 0) that is handed urot_buf
 * skips its weight transform.  NULL = compute everything in the workspace. */
int rn_conv3x3_winograd_keep_bytes(const rn_conv_seg* segs, int nseg, int cin, int cout, int tile, size_t* v_bytes,
                                   size_t* urot_bytes);
int rn_conv3x3_winograd(const rn_conv_seg* segs, int nseg, int cin, int cout, const float* w, const float* bias,
                        int dgrad, int tile, void* workspace, size_t workspace_bytes, float* v_buf, float* urot_buf,
                        rn_stream_t stream);
/* The batched product the Winograd stages run on the fp32 matrix cores, exposed for measurement (bench.py times
 * the head-tower layer's instance: 36 x [682 x 256] x [256 x 256]) and reuse:
 *   C_b [M x N] = A_b [M x K] * B_b,  b = 0..nbatch-1, matrices of a batch stored back to back;
 *   b_nk == 0: B_b is [K x N];  b_nk != 0: B_b is [N x K] (the data-gradient layout).  K and N multiples of 4. */
int rn_gemm_batched(const float* A, const float* B, float* C, int M, int K, int N, int nbatch, int b_nk, rn_stream_t stream);
/* The merged backward products of such a layer (what rn_conv3x3_winograd_bwd launches between its transforms), exposed
 * for measurement (bench.py times the head-tower instance: the largest kernel of the training step): ONE launch with
 * blocks of two kinds -- the data-gradient products Cd_b [M x Nd] = Ad_b [M x Kd] * Bd_b^T (Bd_b stored [Nd x Kd]) and
 * the split partial products of the weight gradient Aw_b^T [Kw x M] * Bw_b [M x Nw], left in `workspace` as *nsplit
 * slabs (rn_winograd_bwd_products_workspace bytes). */
size_t rn_winograd_bwd_products_workspace(int M, int Kw, int Nw, int nbatch);
int rn_winograd_bwd_products(const float* Ad, const float* Bd, float* Cd, int M, int Kd, int Nd, const float* Aw,
                             const float* Bw, int Kw, int Nw, int nbatch, void* workspace, size_t workspace_bytes,
                             int* nsplit, rn_stream_t stream);
/* Weight gradient of the same convolution in the Winograd domain: dU_xi = sum over tiles of
 * (B^T d B)_xi^T (A dY A^T)_xi as (tile+2)^2 batched GEMMs with the reduction split across blocks (fixed-order
 * sum), then dw[3,3,cin,cout] (+)= G^T dU G.  Segments: x, dy, n, h, w. */
size_t rn_conv3x3_winograd_wgrad_workspace(const rn_conv_seg* segs, int nseg, int cin, int cout, int tile);
int rn_conv3x3_winograd_wgrad(const rn_conv_seg* segs, int nseg, int cin, int cout, float* dw, int accumulate, int tile,
                              void* workspace, size_t workspace_bytes, const float* v_buf, rn_stream_t stream);

/* The whole backward pass of such a layer -- dx for every segment and dw -- in three launches whose blocks are of two
 * kinds each: [B^T dy B | A dy A^T], [data-gradient products | weight-gradient partial products],
 * [output transform -> dx | G^T dU G -> dw].  Same results as rn_conv3x3_winograd(dgrad = 1) followed by
 * rn_conv3x3_winograd_wgrad.  Segments: x, dy, dx.  v_buf / urot_buf: the buffers a forward call kept (either may be
 * NULL: then it is rebuilt here; say so in the workspace query). */
size_t rn_conv3x3_winograd_bwd_workspace(const rn_conv_seg* segs, int nseg, int cin, int cout, int tile, int have_v, int have_urot);
int rn_conv3x3_winograd_bwd(const rn_conv_seg* segs, int nseg, int cin, int cout, const float* w, float* dw, int accumulate, int tile,
                            void* workspace, size_t workspace_bytes, const float* v_buf, const float* urot_buf, rn_stream_t stream);

/* How the batched fp32 products of the Winograd convolutions are evaluated (process-wide; default 1, or the environment's
 * RN_PROD_X3 at first use):
 *   0  the exact fp32 matrix-core instruction (v_mfma_f32_32x32x2_f32): a k-ordered fmaf chain
 *   1  every fp32 operand split exactly into three bf16 values, six bf16 matrix-core products with fp32 accumulation
 *      (csrc/gemm_x3.hip): relative error <= ~2^-23 per elementary product, 2.7 x less matrix-core time.  Storage stays fp32.
 * Shapes the split kernels do not take (K or N not a multiple of 4, matrices >= 2 GiB) use mode 0 regardless. */
int rn_set_product_mode(int mode);
int rn_get_product_mode(void);
/* Product mode 1, the kernel operand of the head towers' FORWARD products (the reference's conv kernels of retinanet.py:37-62,85-106)
 * pre-split by its PRODUCER: the Winograd kernel transform of rn_conv3x3_winograd_gn writes U as the three bf16 planes the product
 * kernel needs, in the order its matrix-core instruction reads them -- [32-column block][16-k step][plane][lane][8 bf16], 6 bytes
 * per element -- and the product kernel loads its B fragments straight from global memory (no split, no LDS for that operand).
 * Same values, same order of operations: results are bit-identical to the fp32-operand kernel.  Process-wide switch (default on,
 * RN_X3_BFRAG=0 at first use: off).
 *   rn_x3_bfrag_ok     1 when [M x K] x [K x N] can take such an operand now (mode 1, switch on, K % 16 == 0, N % 4 == 0)
 *   rn_x3_bfrag_bytes  bytes of the images of `nbatch` [K x N] operands (the columns padded to 32)
 *   rn_x3_pack_bfrag   fp32 B_b ([K x N], or [N x K] when b_nk) -> images: for stand-alone products (tests, bench.py)
 *   rn_gemm_batched_bfrag   rn_gemm_batched with B given as images (fwd_name: which of two identical kernel instantiations runs) */
int rn_set_x3_bfrag(int on);
int rn_get_x3_bfrag(void);
int rn_x3_bfrag_ok(int M, int K, int N);
size_t rn_x3_bfrag_bytes(int K, int N, int nbatch);
int rn_x3_pack_bfrag(const float* B, void* out, int K, int N, int nbatch, int b_nk, rn_stream_t stream);
int rn_gemm_batched_bfrag(const float* A, const void* Bfrag, float* C, int M, int K, int N, int nbatch, int fwd_name, rn_stream_t stream);

/* ------------------------------------------------------------------ fp16 inference convolution
 * BASELINE configs[4] ("Inference-only ResNeXt-50-FPN 1024x1024 bs=16, fp16"): forward conv on the f16
 * matrix cores (v_mfma_f32_32x32x16_f16, fp32 accumulate).  Segment fields as rn_conv2d_fwd but x is
 * fp16 NHWC, wgt is the PACKED kernel (fp16, written by rn_pack_weights_f16 into a buffer of rn_pack_weights_f16_bytes
 * bytes), bias fp32, y fp16 (out_f32 = 0) or fp32 (out_f32 = 1).  cin/G must be a multiple of 4.
 * The packed kernel is Wt[cout][kh*kw*cin/G] and, when kh*kw*cin/G is a multiple of 16, 256-byte aligned behind it, the
 * same values once more in matrix-core fragment order Wf[ceil(cout/32)][K/16][64 lanes][8] (channels padded with zeros):
 * the large-tile kernel reads its weight operand from that copy straight into registers.
 * A 3 x 3 kernel with 4 / 8 / 16 / 32 input channels per group and cout % 32 == 0 carries a THIRD copy, 256-byte aligned behind
 * the others: Ws[cout/32][9 taps][2][64 lanes][8], the block-diagonal 32 x 32 kernel of every super-group of 32 consecutive
 * channels in fragment order (lane l: output channel l & 31, input channels 16 step + 8 (l >> 5) .. + 7 of the super-group; zero
 * where the two belong to different groups of cin_g channels).  Grouped 3 x 3 convs with as many input as output channels per
 * group on maps of whole 16 x 16 (stride 1) / 32 x 32 (stride 2) pixel tiles -- ResNeXt's conv 2, resnet.py:36-49 -- run from it:
 * a block keeps the input patch of a 16 x 16 (8 x 16) output tile of one super-group in LDS and the kernel in registers; with
 * rn_conv2d_fwd_f16_fold a GroupNorm + activation in front is applied once per patch element on its way into LDS. */
size_t rn_pack_weights_f16_bytes(int kh, int kw, int cin_g, int cout);
int rn_pack_weights_f16(const float* w, void* wt, int kh, int kw, int cin_g, int cout, rn_stream_t stream);
int rn_cast_f32_to_f16(const float* x, void* y, int64_t count, rn_stream_t stream);
/* image [pixels,3] fp32 -> [pixels,4] fp16 with a zero 4th channel (the stem then gathers 8 bytes per tap) */
int rn_pad_cast_rgb_f16(const float* x, void* y, int64_t pixels, rn_stream_t stream);
int rn_conv2d_fwd_f16(const rn_conv_seg* segs, int nseg, const rn_conv_geom* g, int out_f32, rn_stream_t stream);
/* The same convolution with the GroupNorms around it folded in (Sequential([Conv2D, Normalization, activation]) of the
 * backbones, e.g. resnet.py:53-64,88-101, normalization.py:20-35), fp16 output, one segment:
 *   input side (in_mean != NULL): x is the RAW output of the previous conv; the kernel loads act(GN(x)) -- scale / shift per
 *     (sample, channel) from in_mean / in_rstd [n][in_groups] and in_gamma / in_beta [cin] -- and pads with zeros AFTER
 *     the activation, exactly what a stand-alone GroupNorm + activation pass would have stored;
 *   output side (partial != NULL): per (m-tile, channel) sums of y and y^2, of the values as stored in fp16, in the
 *     layout [2][n * rows][cout] with rows = rn_conv2d_f16_fold_rows(...) m-tiles per sample; rn_group_norm_finalize turns
 *     them into mean / rstd [n][groups]; the conv must have no bias.  (The input side alone is not built: a conv whose
 *     input is a pending GroupNorm is followed by one itself in every network here.)
 * rn_conv2d_f16_fold_rows returns 0 when the shape cannot fold (several segments, fp32 output, oh*ow not a whole number of
 * m-tiles, cout/groups not a multiple of 8): the caller then uses rn_conv2d_fwd_f16 + rn_group_norm_fwd. */
typedef struct rn_f16_fold {
  const float* in_mean; const float* in_rstd; const float* in_gamma; const float* in_beta;
  int in_groups; int in_act;
  float* partial;
  /* several segments in one launch (the head towers' pyramid levels, retinanet.py:37-62,85-106; output side only): `partial` is ONE
   * array [2][total_chunks][cout]; segment s writes its rows (n_s x tiles per sample, rn_conv2d_f16_stats_tiles) from row
   * seg_chunk_start[s] on; a segment with 0 tiles per sample (its m-tiles straddle samples) writes none.  NULL: one segment, as above. */
  const int32_t* seg_chunk_start;
  int32_t total_chunks;
} rn_f16_fold;
int rn_conv2d_f16_fold_rows(const rn_conv_seg* segs, int nseg, const rn_conv_geom* g);
/* m-tiles per sample each segment of such a launch would write statistics rows for (0: none); RN_EUNSUPPORTED where the several-segment
 * layout is not possible: fp32 output, cout/groups % 8 != 0, groups, and a shape the super-group kernel takes */
int rn_conv2d_f16_stats_tiles(const rn_conv_seg* segs, int nseg, const rn_conv_geom* g, int32_t* tiles_per_sample);
int rn_conv2d_fwd_f16_fold(const rn_conv_seg* segs, int nseg, const rn_conv_geom* g, const rn_f16_fold* fold, rn_stream_t stream);
/* What one rn_conv2d_fwd_f16 (fold == NULL) / rn_conv2d_fwd_f16_fold call with the same arguments launches (host only).  It is the
 * decision the launch is made from: conv_f16_impl (csrc/conv_f16.hip) fills an rn_f16_plan and launches from it; the query is the
 * same function stopped before the first launch and before the pipelined kernels' dynamic-LDS attribute is requested.  It touches
 * no device and follows no data pointer: segs[].x / wgt / y / bias and the fold's in_* / partial are only compared with NULL where
 * the entry point does that (fold->seg_chunk_start is a host array and is read as the entry point reads it).  Returns what the
 * launch would return for the same arguments (RN_EINVAL / RN_EUNSUPPORTED; RN_EINVAL for a NULL plan or an empty fold); the plan
 * of a refused call is not meaningful.  rn_conv2d_f16_fold_rows and rn_conv2d_f16_stats_tiles read rows_per_sample /
 * tiles_per_sample of the plan of the plain fp16-output call.
 * Environment switches, as the entry points read them.  At every call: RN_CONV_CFG.  Once per process (first use): RN_F16_SG,
 * RN_F16_PIPE, RN_F16_NT, RN_F16_PIPE_MIN_K.
 * `pipe` is the K loop the host asks for; the pipelined kernels need 147 KB of dynamic LDS, an attribute only a device can grant:
 * rn_conv2d_f16_pipe_available (device side: the same one-time request the first pipelined launch makes) returns 1 when it was
 * granted, 0 when every launch with pipe != 0 silently runs the plain loop (the same template F, PIPE = 0) instead. */
enum rn_f16_kernel { RN_F16_KERNEL_IGEMM = 1 /* conv_f16_kernel */, RN_F16_KERNEL_SG = 2 /* conv3x3_sg32_f16_kernel */ };
enum rn_f16_epilogue { RN_F16_EPI_STAGED = 0 /* fp16 through LDS, 16-byte stores */, RN_F16_EPI_SCALAR_F16 = 1, RN_F16_EPI_SCALAR_F32 = 2 };
typedef struct rn_f16_plan {
  int32_t kernel;          /* enum rn_f16_kernel */
  int32_t cfg;             /* implicit GEMM: tile 0 128x128, 1 128x64, 2 64x64, 3 128x32, 4 256x128, 5 256x256; super-group: the stride 1 / 2 */
  int32_t vec;             /* halfs per operand gather: 4 or 8 */
  int32_t tap_uniform;     /* every K tile lies inside one filter tap (cin/G % 64 == 0) */
  int32_t fold;            /* implicit GEMM: the template's F (0, 2 statistics, 3 input fold + statistics, 7 the same with ReLU);
                              super-group: FIN (0 none, 1 any activation, 2 ReLU) */
  int32_t stats;           /* the epilogue writes statistic rows (implicit GEMM: F & 2) */
  int32_t pipe;            /* 0 the plain loop, 1 pipelined with both operands through LDS, 2 weight fragments from the packed copy */
  int32_t epilogue;        /* enum rn_f16_epilogue */
  int32_t a_nt;            /* non-temporal loads of the activation operand */
  int32_t frag_copy;       /* every segment's wgt_bytes proves the fragment-ordered copy */
  int32_t blocks;          /* grid size */
  int32_t k_tiles;         /* K tiles of 64 halfs (super-group: 18 matrix-core steps, reported as 0) */
  int32_t rows_per_sample; /* statistic rows per sample of a one-segment fold (rn_conv2d_f16_fold_rows; 0: the shape cannot fold) */
  int32_t multi_stats;     /* the several-segment statistics layout is possible (fp16 output, cout % 8 == 0, no groups) */
  int32_t tiles_per_sample[RN_MAX_SEG]; /* ... and the rows per sample each segment writes there (rn_conv2d_f16_stats_tiles) */
} rn_f16_plan;
int rn_conv2d_f16_plan(const rn_conv_seg* segs, int nseg, const rn_conv_geom* g, int out_f32, const rn_f16_fold* fold /* NULL: rn_conv2d_fwd_f16 */,
                       rn_f16_plan* plan);
int rn_conv2d_f16_pipe_available(void);
/* mean / rstd [n][groups] from the partial sums above (fp64, fixed order); hw = oh * ow */
int rn_group_norm_finalize(const float* partial, int n, int rows_per_sample, int hw, int c, int groups, float eps, float* mean,
                           float* rstd, rn_stream_t stream);
/* y = act(GN(x)) + residual, or act(GN(x) + residual) (act_after_residual), fp16 x / residual / y, from given statistics */
int rn_group_norm_apply_f16(const void* x, const void* residual, void* y, int n, int hw, int c, int groups, const float* mean,
                            const float* rstd, const float* gamma, const float* beta, int act, int act_after_residual,
                            rn_stream_t stream);
/* The same with a residual that is itself the RAW fp16 output of a conv whose activation-free GroupNorm has not been applied yet
 * (ResNeXt's projection branch, resnet.py:62-71: identity = normalization(conv(input))): residual' = GN_r(residual) is formed
 * in fp32 inside this pass and never written -- y = act(GN(x) + GN_r(residual)) (act_after_residual) or act(GN(x)) + GN_r(..). */
typedef struct rn_gn_residual_norm {
  const float* mean; const float* rstd;       /* [n][groups] */
  const float* gamma; const float* beta;      /* [c] */
  int groups;
} rn_gn_residual_norm;
int rn_group_norm_apply_res_f16(const void* x, const void* residual, const rn_gn_residual_norm* residual_norm, void* y, int n, int hw, int c,
                                int groups, const float* mean, const float* rstd, const float* gamma, const float* beta, int act,
                                int act_after_residual, rn_stream_t stream);

/* ------------------------------------------------------------------ depthwise 3x3
 * Replaces tf.nn.depthwise_conv2d (DepthwiseConv2dNative + its two backprops),
 * mobilenet_v2.py:35-36.  Kernel [kh,kw,C] (channel multiplier 1), padding SAME.
 */
int rn_depthwise_fwd(const float* x, const float* wgt, float* y, int n, int h, int w, int c, int k, int stride,
                     rn_stream_t stream);
/* the same with the GroupNorm partial-sum rows of y (rn_gn_rows above); k == 3, c % 4 == 0, c <= 1024 */
size_t rn_depthwise_stats_rows(int n, int h, int w, int c, int k, int stride, int groups, rn_gn_rows* layout);
int rn_depthwise_fwd_stats(const float* x, const float* wgt, float* y, int n, int h, int w, int c, int k, int stride,
                           const rn_gn_rows* rows, rn_stream_t stream);
int rn_depthwise_dgrad(const float* dy, const float* wgt, float* dx, int n, int h, int w, int c, int k,
                       int stride, rn_stream_t stream);
size_t rn_depthwise_wgrad_workspace(int n, int h, int w, int c, int k, int stride);
/* both gradients of a 3x3 depthwise conv in one launch (workspace: rn_depthwise_wgrad_workspace bytes) */
int rn_depthwise_bwd(const float* x, const float* dy, const float* wgt, float* dx, float* dw, int n, int h, int w, int c, int k,
                     int stride, void* workspace, size_t workspace_bytes, rn_stream_t stream, rn_reduce_list* defer);
int rn_depthwise_wgrad(const float* x, const float* dy, float* dw, int n, int h, int w, int c, int k, int stride,
                       void* workspace, size_t workspace_bytes, rn_stream_t stream, rn_reduce_list* defer);

/* Which kernels the rn_depthwise_* calls of this shape launch, and with which grids -- for tests that must know which
 * implementation a shape takes.  It is the decision the entry points themselves run before they launch (one function).  Host
 * only: touches no device, launches nothing.  groups: of the GroupNorm behind rn_depthwise_fwd_stats (< 1: the stats_* fields
 * stay 0).  Returns what rn_depthwise_fwd / _dgrad would return for the same shape (RN_EINVAL / RN_EUNSUPPORTED: the plan is
 * zeroed), RN_EINVAL for a NULL plan. */
enum rn_dw_fwd {
  RN_DW_FWD_K3 = 1,      /* dw_fwd_kernel<true>: unrolled, branch-free 3x3 */
  RN_DW_FWD_GENERIC = 2  /* dw_fwd_kernel<false>: any k                    */
};
enum rn_dw_dgrad {
  RN_DW_DGRAD_K3_PARITY = 1, /* dw_dgrad_kernel<true> at stride 2: the 2 x 2 taps whose parity matches the pixel's */
  RN_DW_DGRAD_K3 = 2,        /* dw_dgrad_kernel<true> at any other stride: nine taps under divisibility masks       */
  RN_DW_DGRAD_GENERIC = 3    /* dw_dgrad_kernel<false>: any k                                                       */
};
typedef struct rn_dw_plan {
  int32_t oh, ow, pad_t, pad_l;         /* SAME geometry: output size, padding before                                       */
  int32_t fwd_kernel, fwd_blocks;       /* rn_dw_fwd; blocks of 256 threads (at most 8192: grid-stride)                     */
  int32_t dgrad_kernel, dgrad_blocks;   /* rn_dw_dgrad; likewise                                                            */
  int32_t wgrad_ok;                     /* 0: rn_depthwise_wgrad and rn_depthwise_bwd return RN_EUNSUPPORTED (k != 3)       */
  int32_t wgrad_chunks, wgrad_ppc;      /* blocks of dw_wgrad_partial_kernel (at most 4096) and output pixels of each       */
  int32_t bwd_blocks;                   /* dw_bwd_kernel: dgrad_blocks + wgrad_chunks (0 where wgrad_ok is 0)               */
  int32_t stats_r;                      /* dw_fwd_stats_kernel<R>: 4, 8, 16; 0: rn_depthwise_stats_rows returns 0           */
  int32_t stats_ppc;                    /* output pixels per block                                                          */
  int32_t stats_rows_per_sample;        /* = rn_gn_rows.rows_per_sample                                                     */
  int32_t stats_blocks;                 /* n * stats_rows_per_sample                                                        */
  uint64_t wgrad_workspace_bytes;       /* = rn_depthwise_wgrad_workspace                                                   */
} rn_dw_plan;
int rn_depthwise_plan(int n, int h, int w, int c, int k, int stride, int groups, rn_dw_plan* plan);

/* ------------------------------------------------------------------ fp16 inference depthwise 3x3
 * The DepthwiseConv2D of MobileNetV2's bottleneck at inference (mobilenet_v2.py:15-38, tf.nn.depthwise_conv2d at :35-36; built
 * into the block at :66-68 between the Normalization + activation of the expand conv, :57-61, and its own, :69-70;
 * normalization.py:20-35): x, y fp16 NHWC, wgt the fp32 kernel [3,3,c] as the parameter is stored (9 c floats, no packing), fp32
 * accumulation, stride 1 or 2, TF SAME padding, c a multiple of 8 (at most 2048).
 *   input side (in_mean .. in_beta all non-NULL; all NULL and in_groups = in_act = 0: x is a finished activation): rn_f16_fold's
 *     semantics -- x is the RAW fp16 output of the conv in front; the kernel loads act(GN(x)), formed in fp32 and rounded to fp16
 *     exactly as rn_group_norm_apply_f16 would have stored it, and pads with zeros AFTER the activation.  in_mean / in_rstd
 *     [n][in_groups], in_gamma / in_beta [c]; any channels per group (an octet of channels may straddle groups).
 *   output side (partial != NULL): sums of y and y^2, of the values as stored in fp16, per (pixel chunk, channel) in the layout
 *     [2][n * rows][c], rows = rn_depthwise_f16_rows(n, h, w, c, stride) chunks per sample (a chunk never straddles samples): what
 *     rn_group_norm_finalize reads.  Fixed-order reduction through LDS, no atomics.
 * Checked before any launch.  RN_EINVAL: a NULL descriptor, x, wgt or y; in_* given partly (or in_groups / in_act without them);
 * c % 8 != 0; stride outside {1, 2}; x, wgt, y or partial not 16-byte aligned, an in_* pointer not 4-byte aligned.
 * RN_EUNSUPPORTED: k != 3, c > 2048, 2^31 elements and more. */
typedef struct rn_dw_f16 {
  const void* x; const float* wgt; void* y;
  int32_t n, h, w, c, k, stride;
  const float* in_mean; const float* in_rstd; const float* in_gamma; const float* in_beta;
  int32_t in_groups, in_act;
  float* partial;
} rn_dw_f16;
int rn_depthwise_f16_rows(int n, int h, int w, int c, int stride);       /* 0: a shape rn_depthwise_fwd_f16 refuses */
int rn_depthwise_fwd_f16(const rn_dw_f16* d, rn_stream_t stream);
/* What rn_depthwise_fwd_f16 launches for the same descriptor: the launch decision stopped before the launch (one function).
 * Host only: touches no device; the descriptor's pointers are compared with NULL and checked for alignment, never followed.
 * Returns what the launch would return (a refused call's plan is zeroed), RN_EINVAL for a NULL plan.
 * A block of 256 threads is pixel_lanes x (c / 8) threads (the rest idle); a thread owns one channel octet and computes one strip
 * of pixels_per_thread outputs along w by rows_per_thread output rows; a block is one chunk = one statistic row. */
enum rn_dw_f16_kernel { RN_DW_F16_S1 = 1 /* dw_f16_kernel<1, P, ..> */, RN_DW_F16_S2 = 2 /* dw_f16_kernel<2, P, ..> */ };
typedef struct rn_dw_f16_plan {
  int32_t oh, ow, pad_t, pad_l;      /* SAME geometry                                                                  */
  int32_t kernel;                    /* enum rn_dw_f16_kernel                                                          */
  int32_t pixels_per_thread;         /* P, the strip's width: 4 at stride 1, 2 at stride 2; 1 where ow is smaller     */
  int32_t pixel_lanes;               /* 256 / (c / 8)                                                                  */
  int32_t rows_per_thread;           /* R, the strip's height: 4 (oh >= 32), 2 (oh >= 8), 1                            */
  int32_t strips_per_sample;         /* ceil(oh / R) * ceil(ow / P)                                                    */
  int32_t strips_per_chunk;          /* = pixel_lanes                                                                  */
  int32_t pixels_per_chunk;          /* strips_per_chunk * P * R (strips at the right / bottom edge may hold fewer)    */
  int32_t rows_per_sample;           /* = rn_depthwise_f16_rows                                                        */
  int32_t blocks;                    /* n * rows_per_sample (not capped)                                               */
  int32_t fold;                      /* the input side is applied                                                      */
  int32_t stats;                     /* statistic rows are written                                                     */
} rn_dw_f16_plan;
int rn_depthwise_f16_plan(const rn_dw_f16* d, rn_dw_f16_plan* plan);

/* ------------------------------------------------------------------ fp16 inference dense block (DenseNet-BC)
 * The reference's dense block (densenet.py:117-121: output = composite_function(input); input = concat([input, output]))
 * on ONE fp16 buffer [n, hw, ld], ld = c_in + depth * k, for inference: no concat, and the GroupNorm in front of every layer's
 * 1 x 1 conv (densenet.py:61-66, normalization.py:20-35) takes its statistics from per-channel sums that are formed ONCE, when a
 * channel slice is written -- the statistics of a channel prefix do not change inside a block.
 *   rn_dense_f16_put       buf[:, :, coff : coff + c] = src (dense fp16 [n, hw, c]); in the same pass partial[0 | 1][sample][row][coff + j]
 *                          = sum of x | x^2 (of the values as stored, fp32, fixed order) over the pixels of chunk `row` of the sample.
 *                          partial is the caller's table [2][n][rows][ld] (fp32), rows = rn_dense_f16_rows(hw): a function of hw
 *                          alone, so every slice of a block shares the layout.  Bytes of buf and partial outside the slice are not
 *                          touched.  src == buf (with ld == c, coff == 0) asks for the sums of a finished tensor: nothing is stored to buf.
 *   rn_dense_f16_finalize  mean / rstd [n][groups] of the prefix [0, c) from the table (fp64, fixed order); c / groups is any size
 *                          (2, 3, 4 ... 51 in DenseNet-121 / -169 with groups = 32).
 *   rn_dense_f16_norm      y (dense fp16 [n, hw, c]) = act(GN(buf[:, :, 0 : c])), formed in fp32 and rounded to fp16 exactly as
 *                          rn_group_norm_apply_f16 stores it; c <= 2048.  A launch of its own behind the finalise.
 * Checked before any launch.  RN_EINVAL: a NULL or misaligned (16 bytes) pointer, a shape < 1, ld < coff + c, coff != 0 or groups
 * not dividing c for finalize / norm, an unknown act.  RN_EUNSUPPORTED: c, ld or coff not a multiple of 8, c > 2048 (norm),
 * n > 65535. */
int rn_dense_f16_rows(int hw);      /* statistic rows per sample; 0 for hw < 1 */
int rn_dense_f16_put(const void* src, void* buf, float* partial, int n, int hw, int c, int ld, int coff, rn_stream_t stream);
int rn_dense_f16_finalize(const float* partial, int n, int hw, int c, int ld, int groups, float eps, float* mean, float* rstd,
                          rn_stream_t stream);
int rn_dense_f16_norm(const void* buf, void* y, int n, int hw, int c, int ld, int groups, const float* mean, const float* rstd,
                      const float* gamma, const float* beta, int act, rn_stream_t stream);
/* What the three entry points launch for a shape: their launch decision stopped before the launch (one function).  Host only.
 * Returns what the launch would return for valid pointers (a refused call's plan is zeroed), RN_EINVAL for a NULL plan.
 * groups is read by finalize / norm only. */
enum rn_dense_f16_op { RN_DENSE_F16_PUT = 1, RN_DENSE_F16_FINALIZE = 2, RN_DENSE_F16_NORM = 3 };
typedef struct rn_dense_plan {
  int32_t op;                  /* enum rn_dense_f16_op                                                                      */
  int32_t vec;                 /* elements per memory access: 8 halfs (put, norm), 1 float (finalize)                        */
  int32_t chunk;               /* pixels per statistic row                                                                   */
  int32_t rows;                /* = rn_dense_f16_rows(hw)                                                                    */
  int32_t octets_per_block;    /* put: channel octets a block spans (a power of two, at most 32)                             */
  int32_t lanes;               /* put: pixel lanes of a block = threads / octets_per_block; lane l walks pixels l, l + lanes .. */
  int32_t grid_x, grid_y, grid_z; /* put: (rows, n, octet spans); finalize: (groups, n, 1); norm: (grid-stride blocks, n, 1) */
  int32_t threads;             /* 256                                                                                        */
} rn_dense_plan;
int rn_dense_f16_plan(int op, int n, int hw, int c, int ld, int coff, int groups, rn_dense_plan* plan);

/* ------------------------------------------------------------------ GroupNorm (+act, +dropout, +residual)
 * Replaces normalization.py:20-35 (reshape + tf.nn.moments + affine), the activation that
 * follows it in every reference Sequential (tf.nn.elu train.py:214 / tf.nn.relu resnet.py:85),
 * tf.layers.Dropout (mobilenet_v2.py:62,71,79) and the residual add (mobilenet_v2.py:91-92).
 *   y = dropout(act((x-mean_g)*rstd_g*gamma_c+beta_c)) + residual
 * Segments share gamma/beta (heads: one layer applied to P3..P7).
 * mean / rstd ([n, groups] per segment) are outputs of fwd and inputs of bwd.
 */
typedef struct rn_gn_seg {
  const float* x;        /* [n, hw, c] conv output                         */
  float* y;              /* fwd out                                         */
  const float* residual; /* fwd: optional, same shape as y, or NULL         */
  const float* dy;       /* bwd in                                          */
  float* dx;             /* bwd out                                         */
  float* dresidual;      /* bwd out, only with act_after_residual: grad w.r.t. residual */
  float* mean;           /* [n, groups]                                     */
  float* rstd;           /* [n, groups]                                     */
  int32_t n, hw;
  /* Channel-prefix views (concat-free DenseNet blocks, densenet.py:117-121: layer i normalises the first c channels of
   * the block's one [n, hw, c_total] buffer instead of a concatenated copy).  0 = dense. */
  int32_t x_ld;          /* floats between consecutive pixels of x (fwd and bwd reads)                     */
  int32_t dx_ld;         /* the same for dx                                                                 */
  int32_t dx_accumulate; /* != 0: dx += (every later layer of the block adds to the same gradient buffer)   */
} rn_gn_seg;

typedef struct rn_gn_params {
  int32_t c, groups, act;
  int32_t act_after_residual; /* 0: y = drop(act(GN(x))) + residual (MobileNetV2, mobilenet_v2.py:91-92);
                                 1: y = drop(act(GN(x) + residual))  (ResNeXt, resnet.py:99-101)          */
  int32_t in_f16, out_f16;    /* forward only (inference): x is fp16 / y and residual are fp16           */
  float eps;
  float drop_rate;    /* 0 => no dropout                                    */
  uint64_t drop_seed; /* counter-based mask: keep iff hash(seed, elem) >= rate            */
  const uint64_t* drop_seed_dev; /* optional DEVICE counter added to drop_seed (so a replayed
                                    hipGraph draws a fresh mask every step); may be NULL    */
  void* sync; /* optional: rn_group_norm_sync_bytes() zero-initialised DEVICE bytes owned by the caller, private to the
                 stream, written by these kernels only; enables the single-kernel path for mid-sized maps (<= 128 blocks
                 exchange tagged per-group sums through it, bounded polling).  Word 0 is left at zero, word 1 counts the
                 calls, word 2 becomes 1 if a wait ever timed out.  NULL = not used. */
  const rn_gn_rows* stat_rows; /* forward, one dense fp32 segment: the partial-sum rows its producer wrote for x
                                  (rn_conv2d_fwd_stats / rn_depthwise_fwd_stats): merged here instead of reading x twice.
                                  Ignored (statistics computed from x) where rn_group_norm_rows_ok says no.  NULL = none. */
} rn_gn_params;

size_t rn_group_norm_sync_bytes(void);
/* can rn_group_norm_fwd merge rows of this layout for c channels in `groups` groups? (channel slabs of whole groups must
 * tile c, and a block's share of the rows must stay small) */
int rn_group_norm_rows_ok(int c, int groups, int rows_per_sample, int per_group);
size_t rn_group_norm_workspace(const rn_gn_seg* segs, int nseg, const rn_gn_params* p);
int rn_group_norm_fwd(const rn_gn_seg* segs, int nseg, const rn_gn_params* p, const float* gamma,
                      const float* beta, void* workspace, size_t workspace_bytes, rn_stream_t stream);
/* fp16 inference, several segments (the head towers' pyramid levels: the GroupNorm + activation behind the tower convs of
 * retinanet.py:37-62,85-106): y = act(GN(x)) with the statistics taken from the conv's epilogue rows (rn_conv2d_fwd_f16_fold with
 * seg_chunk_start; `partial` and `tiles_per_sample` as there / as rn_conv2d_f16_stats_tiles returned them) instead of a pass over x;
 * a segment with 0 tiles per sample (<= 4096 pixels per sample) is summed from x by the finalise blocks.  fp16 x and y, dense,
 * c % 64 == 0, no dropout, no residual.  Two launches (finalise, apply). */
int rn_group_norm_fwd_f16_tiles(const rn_gn_seg* segs, int nseg, const rn_gn_params* p, const float* gamma, const float* beta,
                                const float* partial, const int32_t* tiles_per_sample, rn_stream_t stream);
/* dgamma/dbeta [c] are OVERWRITTEN with the sum over all segments. */
int rn_group_norm_bwd(const rn_gn_seg* segs, int nseg, const rn_gn_params* p, const float* gamma,
                      const float* beta, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                      rn_stream_t stream, rn_reduce_list* defer);
/* Which kernels one rn_group_norm_fwd (backward == 0) or rn_group_norm_bwd (backward != 0) call with these segments, parameters
 * and workspace size launches -- for tests that must know which implementation a shape takes.  It is the decision the two
 * entry points themselves run before they launch (one function: the same constants, RN_GN_NO_SLICE / RN_GN_NO_ROWS /
 * RN_GN_NO_COOP / RN_GN_SLICE_WC read at the call, RN_GN_ROWS_FIRST / RN_GN_SLICE_BIG / RN_GN_F16_STATS read once per process).
 * Host only: touches no device, launches nothing.  Of the segments only n, hw, x_ld, dx_ld and dx_accumulate are read (data
 * pointers may be NULL); of the parameters the pointers sync, stat_rows and stat_rows->rows are compared with NULL, never
 * followed into device memory.  Returns what the launch would return for the same shapes: RN_EINVAL / RN_EUNSUPPORTED /
 * RN_EWORKSPACE (workspace_bytes below rn_group_norm_workspace), RN_EINVAL for a NULL plan. */
enum rn_gn_path {
  RN_GN_PATH_PRODUCER_ROWS = 1, /* fwd: the producer's statistic rows (rn_gn_params.stat_rows) merged by gn_apply_rows_kernel   */
  RN_GN_PATH_SLICE = 2,         /* gn_slice_{fwd,bwd}_kernel: one kernel, two-pass statistics in registers                      */
  RN_GN_PATH_GRID_RESIDENT = 3, /* gn_coop_{fwd,bwd}_kernel: one kernel, blocks exchange tagged sums through rn_gn_params.sync  */
  RN_GN_PATH_NARROW_SLICE = 4,  /* the slice kernels on runs narrower than 32 bytes, after the grid-resident path has declined  */
  RN_GN_PATH_ROWS = 5,          /* gn_rows_partial_kernel + gn_[bwd_]apply_rows_kernel                                          */
  RN_GN_PATH_THREE_KERNELS = 6  /* partial, finalize, apply                                                                     */
};
enum rn_gn_kernel { /* the three-kernel path's choices */
  RN_GN_K_NONE = 0,
  RN_GN_K_PARTIAL = 1, RN_GN_K_PARTIAL_F16X8 = 2,       /* statistics */
  RN_GN_K_FINALIZE = 3, RN_GN_K_FINALIZE_COLS_SEGS = 4, /* finalize   */
  RN_GN_K_APPLY = 5, RN_GN_K_APPLY_F16X8 = 6            /* apply      */
};
enum rn_gn_param_grad { /* backward: how dgamma / dbeta are formed */
  RN_GN_PGRAD_NONE = 0,            /* forward */
  RN_GN_PGRAD_FINALIZE_BLOCKS = 1, /* blocks appended to the gn_finalize_kernel launch sum the chunk partial planes     */
  RN_GN_PGRAD_KERNEL = 2,          /* gn_param_grad_kernel sums the slice kernels' per-sample rows                      */
  RN_GN_PGRAD_REDUCE_ROWS = 3      /* two rn_reduce_rows column sums (launched now, or recorded in the call's defer list) */
};
typedef struct rn_gn_plan {
  int32_t path;                                 /* rn_gn_path */
  int32_t slice_wc, slice_r, slice_blocks;      /* slice paths: channels per block, the kernels' template R, blocks; else 0 */
  int32_t coop_r, coop_ppc, coop_blocks;        /* grid-resident path: float4 values per thread, pixels per block, blocks; else 0 */
  int32_t rows_sw, rows_per_group;              /* rows paths: channel slab of the apply kernel; 1: rows hold per-group sums */
  int32_t rows_apply_r, rows_apply_blocks;      /* rows paths: the apply kernel's template R and its pixel chunks (grid.x) */
  int32_t rows_per_sample[RN_MAX_SEG];          /* rows paths: chunk rows per sample of every segment */
  int32_t stats_kernel, finalize_kernel, apply_kernel;  /* three-kernel path: rn_gn_kernel; else RN_GN_K_NONE */
  int32_t apply_blocks;                         /* three-kernel path: blocks per sample of the apply kernel */
  int32_t param_grad, param_grad_deferred;      /* rn_gn_param_grad without / with a defer list given to rn_group_norm_bwd */
  int32_t total_chunks;                         /* partial rows of the path taken (producer rows: the producer's) */
} rn_gn_plan;
int rn_group_norm_plan(const rn_gn_seg* segs, int nseg, const rn_gn_params* p, int backward, size_t workspace_bytes,
                       rn_gn_plan* plan);

/* ------------------------------------------------------------------ small elementwise ops
 * activation alone (retinanet.py:180-181 `activation` before the P7 conv) */
int rn_act_fwd(const float* x, float* y, int64_t count, int act, rn_stream_t stream);
int rn_act_bwd(const float* x, const float* dy, float* dx, int64_t count, int act, rn_stream_t stream);
/* y = lateral + nearest_resize(top -> lateral size, align_corners=True); retinanet.py:153-157
 * (ResizeNearestNeighbor) and its gradient w.r.t. top (sum over the children). */
int rn_upsample_add_fwd(const float* lateral, const float* top, float* y, int n, int h, int w, int th, int tw, int c,
                        rn_stream_t stream);
int rn_upsample_add_bwd_top(const float* dy, float* dtop, int n, int h, int w, int th, int tw, int c,
                            rn_stream_t stream);

/* stand-alone inverted dropout (DenseNet puts tf.layers.Dropout after a conv: densenet.py:44,67,77,143);
 * the same counter-based mask in forward and backward: dx = rn_dropout(dy) with the same seed.
 *
 * THE MASK FUNCTION (every dropout of this library: rn_dropout*, rn_gn_params, rn_mb_norm).  Element e (flat
 * index into the dense NHWC tensor the dropout acts on) with s = seed + (seed_dev ? *seed_dev : 0), all arithmetic mod 2^32:
 *     h  = lo32(e) * 0x9E3779B1 + lo32(s);   h ^= hi32(e) * 0x85EBCA77 + hi32(s);
 *     h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16;
 *     u  = (float)(h >> 8) * 2^-24;          y = u >= rate ? x * (1.f / (1.f - rate)) : 0
 * Nothing else enters it (not the launch shape, not the kernel that applies it), so a checker can be handed the very masks
 * a step draws: oracle/dropout_ref.py restates it, tests/test_gpu_dropout.py compares the two bit for bit. */
int rn_dropout(const float* x, float* y, int64_t count, float rate, uint64_t seed, const uint64_t* seed_dev,
               rn_stream_t stream);
/* The same between channel slices: y[p, y_coff + ch] = dropout(x[p, x_coff + ch]), ch < c, rows x_ld / y_ld floats apart; the
 * mask is that of the dense [pixels, c] tensor (element p * c + ch), so slice and dense forms agree.  rate 0 = a copy.
 * Concat-free DenseNet blocks (densenet.py:117-121): a growth layer's output goes straight into its channel slice of the
 * block's buffer; in the backward pass its gradient slice is read out of the block's gradient buffer. */
int rn_dropout_strided(const float* x, float* y, int64_t pixels, int c, int x_ld, int x_coff, int y_ld, int y_coff, float rate,
                       uint64_t seed, const uint64_t* seed_dev, rn_stream_t stream);
/* tf.layers.MaxPooling2D(k, stride, 'same') (resnet.py:200, densenet.py:180): padded cells never win; the
 * gradient goes to the first maximum of each window.  tf.layers.AveragePooling2D(k, stride, 'same')
 * (densenet.py:144): divides by the number of valid cells. */
/* argmax (optional, uint8 [n,oh,ow,c]): tap index kh*k+kw of each window's first maximum, for rn_maxpool_bwd_arg */
int rn_maxpool_fwd(const float* x, float* y, uint8_t* argmax, int n, int h, int w, int c, int k, int stride,
                   rn_stream_t stream);
/* fp16-storage forward variants for the inference path (same semantics) */
int rn_act_fwd_f16(const void* x, void* y, int64_t count, int act, rn_stream_t stream);
int rn_maxpool_fwd_f16(const void* x, void* y, int n, int h, int w, int c, int k, int stride, rn_stream_t stream);
/* fp16 inference: y = maxpool_kxk/stride(act(GroupNorm(x))) from the RAW conv output x [n,h,w,c] (fp16) and the GroupNorm's
 * per-(sample, group) mean / rstd (rn_group_norm_finalize): ResNeXt's stem (resnet.py:192-201: conv, normalization, relu,
 * max_pooling2d) without writing the normalised tensor.  Bit-equal to rn_group_norm_apply_f16 followed by rn_maxpool_fwd_f16. */
int rn_maxpool_gn_fwd_f16(const void* x, void* y, int n, int h, int w, int c, int k, int stride, const float* mean, const float* rstd,
                          const float* gamma, const float* beta, int groups, int act, rn_stream_t stream);
/* fp16 inference: the 2 x 2 / 2 average pool of DenseNet's transition layer (densenet.py:124-151), TF SAME: the sum over the
 * in-bounds cells divided by their number (rn_avgpool_fwd's rule), fp16 NHWC in and out, fp32 accumulation.  mean == NULL: the
 * plain pool.  Otherwise y = avgpool(act(GroupNorm(x))) of the RAW x in one pass, the normalised tensor never written; every tap is
 * rounded to fp16 as rn_group_norm_apply_f16 would store it: bit-equal to that apply pass followed by the plain pool.
 * RN_EUNSUPPORTED: k != 2, stride != 2, c % 8 != 0, c > 2048 behind a GroupNorm.  RN_EINVAL: NULL x / y, a partly given GroupNorm. */
int rn_avgpool_gn_fwd_f16(const void* x, void* y, int n, int h, int w, int c, int k, int stride, const float* mean, const float* rstd,
                          const float* gamma, const float* beta, int groups, int act, rn_stream_t stream);
int rn_upsample_add_fwd_f16(const void* lateral, const void* top, void* y, int n, int h, int w, int th, int tw, int c,
                            rn_stream_t stream);
/* two forms of the same gradient: from x (re-scans every window) or from the forward pass's argmax bytes (5 bytes
 * read per window; what the autograd carrier uses) */
int rn_maxpool_bwd(const float* x, const float* dy, float* dx, int n, int h, int w, int c, int k, int stride,
                   rn_stream_t stream);
int rn_maxpool_bwd_arg(const uint8_t* argmax, const float* dy, float* dx, int n, int h, int w, int c, int k, int stride,
                       rn_stream_t stream);
int rn_avgpool_fwd(const float* x, float* y, int n, int h, int w, int c, int k, int stride, rn_stream_t stream);
int rn_avgpool_bwd(const float* dy, float* dx, int n, int h, int w, int c, int k, int stride, rn_stream_t stream);

/* augmentation.flip (augmentation.py:5-22): y[o, W-1-j, i] = x[o, j, i] for an [outer, W, inner] tensor of
 * 4-byte (fp32) or 1-byte (mask) elements; neg_mod > 0 also negates element neg_idx of every group of
 * neg_mod values along `inner` (the x shift of the [.., A, 4] regression maps: neg_mod 4, neg_idx 1). */
int rn_flip_width(const void* x, void* y, int64_t outer, int w, int64_t inner, int elem_bytes, int neg_mod, int neg_idx,
                  rn_stream_t stream);

/* Input pipeline: tf.image.convert_image_dtype (in_u8: uint8 * 1/255) -> bilinear resize with
 * align_corners=True (dataset.py:145-151 rescale_image; the TF ResizeBilinear arithmetic, operation by operation)
 * -> optional (v - mean[c]) / std[c] (train.py:48-49 preprocess_image; mean / std are HOST arrays of c floats, both
 * NULL = no normalisation).  x [n,h,w,c] uint8 or fp32, y [n,oh,ow,c] fp32, c <= 8. */
int rn_resize_bilinear_normalize(const void* x, int in_u8, float* y, int n, int h, int w, int c, int oh, int ow,
                                 const float* mean, const float* stdv, rn_stream_t stream);

/* The same input pipeline for one raw uint8 image of ANY size, straight into the reference's batch of two (dataset.py:145-151,
 * 182-204 rescale + [image, hflip]; augmentation.py:5-22 flip; train.py:48-49 preprocess_image): pair [2, oh, ow, 3] fp32,
 * slot 0 = rn_resize_bilinear_normalize of the image (bit for bit), slot 1 = its h-flip.  The raw size and the resize ratios
 * come from `desc`, a DEVICE struct uploaded with the sample; the caller computes hs = (h-1)/(oh-1) (0 when oh == 1) and
 * ws = (w-1)/(ow-1) in fp32 as rn_resize_bilinear_normalize does, so no division happens on the device.  One capture of
 * this call therefore serves every raw size that maps to (oh, ow).  Reads stay inside raw[0, raw_capacity) whatever `desc`
 * holds.  mean / std: HOST arrays of 3 floats, both NULL = no normalisation. */
typedef struct rn_resize_desc {
  int32_t h, w;
  float hs, ws;
} rn_resize_desc;
int rn_resize_pair_u8(const uint8_t* raw, int64_t raw_capacity, const rn_resize_desc* desc, float* pair, int oh, int ow,
                      const float* mean, const float* stdv, rn_stream_t stream);

/* rn_resize_pair_u8 with the training-time augmentation the reference names in augment_sample and leaves as a TODO
 * (dataset.py:206-212: random_contrast(0.8, 1.2), random_brightness(0.2), random_saturation(0.8, 1.0); asked for by
 * train_input_fn's augment=True, train.py:190-198) plus a crop window, all driven by a DEVICE descriptor uploaded with the
 * sample: r = the pair's resize of raw[y0:y0+ch, x0:x0+cw] (hs = (ch-1)/(oh-1), ws = (cw-1)/(ow-1) in fp32 from the host, 0
 * when the output extent is 1);  a = (r - m_c) * f + m_c with m_c the fp64-accumulated channel mean of r;  b = clamp(a + d, 0, 1);
 * s_c = M - (M - b_c) * min(k, M / (M - n)) with M / n the channel max / min of b (HSV saturation times k, clamped to 1; s = b
 * when M == n);  then the normalisation and the two slots as in rn_resize_pair_u8.  The full contract is the comment in front
 * of the kernels (csrc/preprocess.hip).  f == 1 and k == 1 skip their step, so the full window with f = 1, d = 0, k = 1 gives
 * rn_resize_pair_u8's output bit for bit, and a window alone gives rn_resize_pair_u8 of a contiguous copy of the crop.
 * Two launches (per-block fp64 channel sums, then the transform), grids a function of (oh, ow) only, no atomics, nothing to
 * clear between replays: one capture serves every raw size, window and parameter draw, bit-identical run to run.  h and w are
 * the raw image's size; reads stay inside raw[0, raw_capacity) whatever `desc` holds.
 * workspace: rn_resize_pair_u8_augment_workspace(oh, ow) bytes, 8-byte aligned (the partial sums). */
typedef struct rn_augment_desc {
  int32_t h, w;            /* raw image */
  int32_t y0, x0, ch, cw;  /* crop window in raw pixels */
  float hs, ws;            /* the window's resize ratios */
  float f, d, k;           /* contrast factor (> 0), brightness delta, saturation factor (>= 0) */
  int32_t reserved;
} rn_augment_desc;
size_t rn_resize_pair_u8_augment_workspace(int oh, int ow);
int rn_resize_pair_u8_augment(const uint8_t* raw, int64_t raw_capacity, const rn_augment_desc* desc, float* pair, int oh, int ow,
                              const float* mean, const float* stdv, void* workspace, size_t workspace_bytes,
                              rn_stream_t stream);

/* Several samples per step (dataset.py:145-151 rescale, 182-204 [image, hflip] and the batch of samples the reference's
 * tf.data pipeline would form, train.py:48-49 preprocess_image): rn_resize_pair_u8 of k raw images in ONE launch.  Raw image i
 * starts at raw + i * sample_stride_bytes and has the DEVICE descriptor desc[i]; pairs [2k, oh, ow, 3] fp32 gets
 * pairs[2i] = the rescaled + normalised sample i and pairs[2i+1] = its h-flip, bit for bit what rn_resize_pair_u8(raw + i * stride,
 * stride, desc + i, pairs + 2i * oh*ow*3, ...) writes: the same arithmetic in the same order, the grid is (that call's blocks,
 * sample).  All raw sizes are read from the descriptors at run time: one capture serves every group of k raw sizes that map to
 * (oh, ow).  sample_stride_bytes is every sample's raw_capacity: reads of sample i stay inside its own slot
 * raw[i * stride, (i+1) * stride) whatever desc[i] holds (a descriptor with h*w*3 > stride gives wrong pixels, never a read
 * of the next slot or past the buffer).  1 <= k <= 65535. */
int rn_resize_pair_u8_batch(const uint8_t* raw, int64_t sample_stride_bytes, const rn_resize_desc* desc, int k, float* pairs,
                            int oh, int ow, const float* mean, const float* stdv, rn_stream_t stream);

/* rn_resize_pair_u8_augment of k raw images (dataset.py:206-212 augment_sample per sample, then the calls above), laid out as for
 * rn_resize_pair_u8_batch with desc[i] an rn_augment_desc.  TWO launches whatever k is: the per-block fp64 channel sums of every
 * sample (sample i's in its own part of the workspace), then the transform of every sample from its own sums -- nothing is added
 * across samples, no atomics, nothing to clear between replays.  Slots 2i / 2i+1 are bit for bit rn_resize_pair_u8_augment's of
 * sample i alone.  workspace: rn_resize_pair_u8_augment_batch_workspace(k, oh, ow) bytes (k times the single-image query),
 * 8-byte aligned. */
size_t rn_resize_pair_u8_augment_batch_workspace(int k, int oh, int ow);
int rn_resize_pair_u8_augment_batch(const uint8_t* raw, int64_t sample_stride_bytes, const rn_augment_desc* desc, int k,
                                    float* pairs, int oh, int ow, const float* mean, const float* stdv, void* workspace,
                                    size_t workspace_bytes, rn_stream_t stream);

/* ------------------------------------------------------------------ loss
 * Replaces utils.process_labels_and_logits/postprocess_and_mask (utils.py:240-284; the
 * boolean_mask compaction becomes a 0/1 row weight, result-identical) and losses.loss
 * (losses.py:155-175): class loss = BCE+dice (live, :124-139) or focal (:6-15,:119-122),
 * regression loss = Huber(delta 1) over fg rows / (4*#fg) (:144-152).
 * Segment = one pyramid level, rows = n*h*w*anchors.
 */
typedef struct rn_loss_seg {
  const float* cls_logit; /* [rows, C]                                      */
  const float* cls_label; /* [rows, C] one-hot / zeros                      */
  const float* reg_pred;  /* [rows, 4]                                      */
  const float* reg_label; /* [rows, 4]                                      */
  const uint8_t* trainable; /* [rows] 0/1                                   */
  float* d_cls_logit;     /* bwd out [rows, C]                              */
  float* d_reg_pred;      /* bwd out [rows, 4]                              */
  int64_t rows;
} rn_loss_seg;

/* stats layout (float32, device): [0]=class_loss [1]=regr_loss [2]=M (trainable rows)
 * [3]=#fg [4]=sum bce [5]=sum focal [6]=sum huber [7]=reserved, then per class c:
 * [8+3c]=I_c=sum l*sigmoid, [9+3c]=L_c=sum l, [10+3c]=P_c=sum sigmoid (the dice term's sums: RN_LOSS_BCE_DICE; in
 * RN_LOSS_FOCAL mode, which does not use them, they may be zero). */
#define RN_LOSS_STATS_HEADER 8
size_t rn_loss_workspace(const rn_loss_seg* segs, int nseg, int num_classes);
/* class_loss_out / regr_loss_out (optional, one float each): the two losses also as stand-alone device scalars */
int rn_loss_fwd(const rn_loss_seg* segs, int nseg, int num_classes, int mode, float* stats, float* class_loss_out,
                float* regr_loss_out, void* workspace, size_t workspace_bytes, rn_stream_t stream);
/* d(g_cls*class_loss + g_reg*regr_loss)/d(logits); g_* are device scalars (upstream grads). */
int rn_loss_bwd(const rn_loss_seg* segs, int nseg, int num_classes, int mode, const float* stats,
                const float* g_cls, const float* g_reg, rn_stream_t stream);

/* ------------------------------------------------------------------ loss as a weighted sum of terms
 * Replaces classification_loss (losses.py:113-141) as a LIST of terms, the one the reference's author edits by commenting lines in
 * and out: class loss = sum over the set terms of weight * term.  Over the M trainable rows, p = sigmoid(z), per class I = sum l p,
 * L = sum l, P = sum p, s = the term's smooth:
 *   RN_LT_BCE           mean_{M,C} sigmoid_cross_entropy_with_logits                                (losses.py:124-125)
 *   RN_LT_BALANCED_BCE  (1/(M C)) sum_c (wp_c B1_c + wn_c B0_c), wp_c = (M - L_c)/M, wn_c = L_c/M, B1_c / B0_c = the sum of the
 *                       cross entropy where l == 1 / l != 1       (balanced_sigmoid_cross_entropy_with_logits, losses.py:96-110, axis 0)
 *   RN_LT_DICE          mean_c 1 - (2 I + s)/(L + P + s)                                            (dice_loss, losses.py:50-60, :130)
 *   RN_LT_FIXED_IOU     mean_c 1 - (I + s)/(L + P - I + s)                                          (fixed_iou_loss, losses.py:63-73, :136)
 *   RN_LT_JACCARD       mean_c (1 - (I + s)/(L + P - I + s)) s: s times fixed_iou(s); 0 for s = 0   (jaccard_loss, losses.py:37-47, :133)
 *   RN_LT_FOCAL         sum focal / max(#fg, 1), focus 2, alpha 0.25, eps 1e-7                      (losses.py:6-15, :119-122)
 * The smooths of the reference's call sites (:130, :133, :136): dice 0, jaccard 1, fixed_iou 1e-7.
 * focal_softmax_cross_entropy_with_logits (losses.py:18-34, "check if this is correct") is not covered.
 * Regression loss, #fg, masking rule, segments and the two-pass structure are those of rn_loss_fwd / rn_loss_bwd above.
 * With M = 0 the two cross-entropy terms are NaN (0/0), as in the reference and in rn_loss_fwd.
 *
 * The descriptor is read before the call returns.  RN_EINVAL: null descriptor; no term or an unknown bit set; the weight of a
 * set term not finite or <= 0; a smooth not finite or < 0; weight or smooth of a clear term not 0; jaccard's weight * smooth
 * not finite.
 * A descriptor equal to {BCE 1, DICE 1, s_dice 0} or {FOCAL 1} runs the kernels of rn_loss_fwd / rn_loss_bwd in that mode:
 * losses, stats [0, 8 + 3C) and gradients are bit-identical to them (stats [8 + 3C, 8 + 5C) are not written then); the
 * environment variable RN_LOSS_TERMS_GENERAL=1 runs the general kernels for these two as well (measurements).
 * stats: the layout above, then [8 + 3C + c] = B1_c and [8 + 4C + c] = B0_c; the general kernels write zeros there without
 * RN_LT_BALANCED_BCE, the two descriptors that run the kernels of rn_loss_fwd leave these 2C entries as the caller passed them. */
enum rn_loss_term { RN_LT_BCE = 1, RN_LT_BALANCED_BCE = 2, RN_LT_DICE = 4, RN_LT_JACCARD = 8, RN_LT_FIXED_IOU = 16, RN_LT_FOCAL = 32 };
typedef struct rn_loss_terms {
  uint32_t terms;        /* OR of rn_loss_term */
  float w_bce, w_balanced_bce, w_dice, w_jaccard, w_fixed_iou, w_focal;   /* > 0 for a set term, 0 for a clear one */
  float s_dice, s_jaccard, s_fixed_iou;                                   /* >= 0; 0 for a clear term */
} rn_loss_terms;
size_t rn_loss_terms_stats_floats(int num_classes);     /* RN_LOSS_STATS_HEADER + 5 C */
/* 0 (and rn_last_error) for a descriptor rn_loss_terms_fwd would refuse */
size_t rn_loss_terms_workspace(const rn_loss_seg* segs, int nseg, int num_classes, const rn_loss_terms* t);
int rn_loss_terms_fwd(const rn_loss_seg* segs, int nseg, int num_classes, const rn_loss_terms* t, float* stats,
                      float* class_loss_out, float* regr_loss_out, void* workspace, size_t workspace_bytes, rn_stream_t stream);
int rn_loss_terms_bwd(const rn_loss_seg* segs, int nseg, int num_classes, const rn_loss_terms* t, const float* stats,
                      const float* g_cls, const float* g_reg, rn_stream_t stream);

/* ------------------------------------------------------------------ box regression loss as a weighted sum of terms
 * Replaces regression_loss (losses.py:144-152) by a sum over the set terms of weight * term, over the foreground rows (fg:
 * trainable and max_c cls_label[row, c] > 0.5, the rule of rn_loss_fwd).  Prediction p and label l of a row are the anchor-relative
 * (ty, tx, th, tw) of dataset.py:102-112 / utils.py:100-117; in anchor units box(t) = (ty - e^th/2, tx - e^tw/2, ty + e^th/2,
 * tx + e^tw/2), I = the area of the intersection, U = area(p) + area(l) - I, E = the area of the smallest enclosing box:
 *   RN_RT_HUBER  sum_fg huber_delta(l - p) / (4 #fg)      (regression_loss, losses.py:144-152; delta: tf.losses.huber_loss's)
 *   RN_RT_IOU    sum_fg (1 - I/U) / #fg
 *   RN_RT_GIOU   sum_fg (1 - (I/U - (E - U)/E)) / #fg
 * Both boxes of a row share the anchor, so regression_postprocess (utils.py:108-117) maps them to the image by one translation and
 * one positive per-axis scaling, under which ratios of areas (utils.iou, utils.py:62-97) do not change: no anchor table is read.
 * DIoU / CIoU (centre distance over diagonal) are not invariant under an anisotropic scaling, would need per-row anchor aspect
 * ratios, and are not covered.  The loss is 0 with #fg = 0.  th / tw are not clamped (regression_postprocess does not clamp).
 * Subgradients: max(P, L) follows P where P >= L, min(P, L) where P <= L, max(0, d) passes where d > 0.
 * Masking: HUBER is the fg weight times the term on every trainable row (a NaN on a trainable row reaches the loss, as in
 * rn_loss_fwd); IOU and GIOU select: a row that is not fg adds exactly 0 and gets gradient exactly 0 whatever it holds.  Rows
 * outside the trainable mask are never read into a sum.  Sums: per-block partials, fixed-order fp64 finalize, no atomics.
 *
 * rn_regr_terms_fwd reads cls_label (for the fg rule only), reg_pred, reg_label and trainable of each segment (cls_logit and the
 * d_* fields may be null) and writes stats, regr_loss_out (optional) and fg_rows (caller-owned, sum of rows bytes, segment order:
 * 1 for a fg row, else 0).  rn_regr_terms_bwd reads reg_pred, reg_label, fg_rows, stats and the device scalar g_reg and writes
 * every element of d_reg_pred = d(g_reg * regr_loss)/d(reg_pred), zeros on rows that are not fg; it touches no class tensor.
 * Zero-row segments are allowed, as in rn_loss_fwd.  No allocation, no synchronisation, no host read: both record into a graph.
 * The descriptor is read before the call returns.  RN_EINVAL (rn_last_error names the field): null descriptor; no term or an
 * unknown bit set; w_* / delta_huber of a set term not finite or <= 0; w_* / delta_huber of a clear term not 0; nseg outside
 * 1..RN_MAX_SEG. */
enum rn_regr_term { RN_RT_HUBER = 1, RN_RT_IOU = 2, RN_RT_GIOU = 4 };
typedef struct rn_regr_terms {
  uint32_t terms;                    /* OR of rn_regr_term */
  float w_huber, w_iou, w_giou;      /* > 0 for a set term, 0 for a clear one */
  float delta_huber;                 /* > 0 with RN_RT_HUBER, else 0 */
} rn_regr_terms;
#define RN_REGR_STATS_FLOATS 8   /* [0] regr_loss [1] #fg [2] sum huber [3] sum (1-IoU) [4] sum (1-GIoU) [5] sum IoU [6,7] reserved */
/* 0 (and rn_last_error) for a descriptor rn_regr_terms_fwd would refuse */
size_t rn_regr_terms_workspace(const rn_loss_seg* segs, int nseg, int num_classes, const rn_regr_terms* t);
int rn_regr_terms_fwd(const rn_loss_seg* segs, int nseg, int num_classes, const rn_regr_terms* t, float* stats,
                      float* regr_loss_out, uint8_t* fg_rows, void* workspace, size_t workspace_bytes, rn_stream_t stream);
int rn_regr_terms_bwd(const rn_loss_seg* segs, int nseg, const rn_regr_terms* t, const float* stats, const uint8_t* fg_rows,
                      const float* g_reg, rn_stream_t stream);

/* ------------------------------------------------------------------ running training metrics
 * Replaces build_metrics (train.py:137-161): the streaming tf.metrics of a training run -- the means of the total, class,
 * regression and regularisation losses, class_iou = tf.metrics.mean_iou(labels, sigmoid(logits) > 0.5, num_classes=2) over the
 * trainable anchors, regr_iou = the mean of utils.iou (utils.py:62-97) between the label box and the predicted box, both decoded
 * (utils.regression_postprocess, utils.py:108-117) at the ground-truth foreground anchors (utils.boxes_decode, utils.py:183-195).
 * Device-resident: the host reads nothing per step.
 * Segment = one pyramid level, rows = n*h*w*anchors in [n,h,w,anchors] order; at most RN_MAX_SEG segments. */
typedef struct rn_metrics_seg {
  const float* cls_logit;    /* [rows, C]                                       */
  const float* cls_label;    /* [rows, C] one-hot / zeros                       */
  const float* reg_pred;     /* [rows, 4] raw (dy, dx, log h, log w)            */
  const float* reg_label;    /* [rows, 4]                                       */
  const uint8_t* trainable;  /* [rows] 0/1                                      */
  const float* anchor_sizes; /* [anchors, 2] (h, w) / image size: rn_decode_boxes' table of this level */
  int32_t n, h, w, anchors;
} rn_metrics_seg;
/* rn_train_metrics_pass: ONE launch over all segments.  For every row with trainable != 0:
 *   class confusion over the row's C elements: label positive iff label > 0.5, prediction positive iff logit > 0.  `logit > 0`
 *     stands for the reference's float32 sigmoid(logit) > 0.5: the two differ only for 0 < logit <~ 1.2e-7, where the float32
 *     sigmoid rounds to exactly 0.5 (the reference then predicts negative, this kernel positive).  Four integer counts.
 *   box IoU, if the row is foreground (max_c label > 0.5): reg_label and reg_pred decoded with rn_decode_boxes' device function,
 *     the IoU formed as rn_iou forms it element-wise (float32 op for op; 0 where the intersection is inverted; NaN where the
 *     reference's is NaN), converted to double and added.
 * Counts and the IoU sum are reduced wave -> block -> one 64-byte row per block of `workspace` (int64 [tn, fp, fn, tp, iou_rows],
 * double sum_iou, 2 unused; behind a 64-byte header whose first int64 is the number of rows written).  No atomics, fixed order:
 * the same bits eagerly and from a graph.  The cls / reg tensors must be 16-byte aligned (16-byte loads where a row's address
 * allows them, a scalar head and tail otherwise: any C >= 1; C % 4 == 0 up to 128 takes kernels of their own, with every load of
 * two row groups in flight at once).  workspace: rn_train_metrics_workspace() bytes, 8-byte aligned,
 * owned by the caller -- it lives from the pass to the fold, so it is NOT the shared scratch arena. */
size_t rn_train_metrics_workspace(const rn_metrics_seg* segs, int nseg, int num_classes);
/* the largest value rn_train_metrics_workspace returns (header + 1024 partial rows): a caller whose launches are captured into
 * graphs allocates this much ONCE, so that every graph of every input shape holds the same pointer for as long as it lives */
#define RN_TRAIN_METRICS_MAX_WORKSPACE_BYTES 65600
int rn_train_metrics_pass(const rn_metrics_seg* segs, int nseg, int num_classes, void* workspace, size_t workspace_bytes,
                          rn_stream_t stream);
/* rn_train_metrics_fold: one block at the end of the step.  Sums the partial rows the last pass left in `workspace` (never more
 * than workspace_bytes holds) in a fixed order -- the integer columns exactly, the IoU sums in index order inside 64 contiguous
 * chunks of rows and then the chunks in order --, reads the device scalars class_loss, regr_loss and reg_loss (the regulariser:
 * norm_reg[1] of rn_norm_reg_finalize / rn_grad_norm_l2reg) and adds the step into `state` (RN_TRAIN_METRICS_STATE_BYTES, 16-byte
 * aligned -- checked by this entry and by rn_train_metrics_reset --, device):
 *   double  [0] sum_total = sum ((class + regr) + reg)  [1] sum_class  [2] sum_regr  [3] sum_reg  [4] sum_iou
 *   int64   [5] steps  [6] nonfinite_steps  [7] tn  [8] fp  [9] fn  [10] tp  [11] iou_rows
 * The step is added ONLY IF class_loss, regr_loss, reg_loss and the step's IoU sum are all finite; otherwise nonfinite_steps
 * advances and nothing else changes (a degenerate box gives NaN as in the reference; one such step must not poison a window's
 * means).  The gate is the metric's own, independent of the guard's (RN_CTL_F_GUARD).  Plain stores. */
#define RN_TRAIN_METRICS_STATE_BYTES 96
int rn_train_metrics_fold(const void* workspace, size_t workspace_bytes, const float* class_loss, const float* regr_loss,
                          const float* reg_loss, void* state, rn_stream_t stream);
/* state = 0 on the stream (rn_zero over its 96 bytes): a new window */
int rn_train_metrics_reset(void* state, rn_stream_t stream);

/* ------------------------------------------------------------------ GroupNorm folded into Winograd layers
 * A chain [conv3x3, GroupNorm, activation] x k -> conv3x3 (the class / box subnets, retinanet.py:37-71,85-115; the
 * GroupNorm is normalization.py:20-35) without GroupNorm kernels and without ever writing the normalised tensor:
 * the output transform of a layer emits, per chunk of 16 Winograd tiles of one sample, the per-group statistics
 * (count, mean, M2 = sum (y - mean)^2, unused) of the RAW conv output ("stat rows", rn_wino_gn_rows() rows of
 * [groups][4] floats); the input transform of the next layer merges its sample's rows (Chan et al.'s pairwise
 * update, fp64, chunk order: no E[y^2] - E[y]^2 cancellation) into mean / rstd and loads act(GN(y)) on the fly.  Backward likewise: the data gradient of the next layer leaves its output transform as
 * g = dA * act'(z) together with rows of (sum g, sum g xhat) -- per channel for dgamma / dbeta (rn_reduce_rows) and
 * gamma-weighted per group -- and the dy transforms of this layer load dy = rstd (gamma g - c1 - xhat c2) from g
 * and the raw y.  No exchange between blocks, no atomics: every sum runs over rows an earlier launch wrote.
 * Needs cin, cout multiples of 64 and 64 % (channels / groups) == 0 on a folded side (RN_EUNSUPPORTED otherwise).
 */
typedef struct rn_wino_gn {
  /* input side: segs[].x is the raw output of the previous conv; NULL in_rows = x is used as it is */
  const float* in_rows;   /* [rows][in_groups][4] written by the previous layer's call */
  const float* in_gamma;  /* [cin] */
  const float* in_beta;   /* [cin] */
  int32_t in_groups, in_act;
  float in_eps;
  /* output side: NULL out_rows = no statistics */
  float* out_rows;        /* [rows][out_groups][4] */
  int32_t out_groups;
  /* the kernel transforms prepared ahead of the layer by rn_conv3x3_winograd_gn_weights (train.Trainer: all tower layers once per
   * step on a side stream beside the backbone, off the layers' critical path): u_ready = its u_out (NULL: transformed inside this
   * call, in the workspace); urot_ready != 0: urot_buf already holds its urot_out and is only read */
  const void* u_ready;
  int32_t urot_ready;
} rn_wino_gn;
size_t rn_wino_gn_rows(const rn_conv_seg* segs, int nseg, int tile);
/* The kernel transforms of such a layer alone: U in the format the layer's forward product reads under the current switches
 * (fp32 [P][cin][cout], or the fragment image of rn_x3_pack_bfrag) -> u_out (rn_conv3x3_winograd_gn_u_bytes bytes), and the rotated
 * kernel's transform (fp32, the data gradient's operand) -> urot_out (urot_bytes of rn_conv3x3_winograd_keep_bytes; NULL: skipped).
 * Same kernels, same values as inside rn_conv3x3_winograd_gn.  The reference's conv kernels: retinanet.py:37-62,85-106. */
size_t rn_conv3x3_winograd_gn_u_bytes(int cin, int cout, int tile);
int rn_conv3x3_winograd_gn_weights(const float* w, int cin, int cout, int tile, void* u_out, size_t u_out_bytes, float* urot_out,
                                   rn_stream_t stream);
/* y = conv3x3_same(act(GN(x)), w) (+ bias).  Workspace / v_buf / urot_buf as rn_conv3x3_winograd. */
int rn_conv3x3_winograd_gn(const rn_conv_seg* segs, int nseg, int cin, int cout, const float* w, const float* bias, int tile,
                           const rn_wino_gn* gn, void* workspace, size_t workspace_bytes, float* v_buf, float* urot_buf,
                           rn_stream_t stream);
typedef struct rn_wino_gn_bwd {
  /* input side folded (in_rows != NULL): segs[].x = raw input tensor, segs[].dx receives g of the input's GroupNorm */
  const float* in_rows;
  const float* in_gamma;
  const float* in_beta;
  int32_t in_groups, in_act;
  float in_eps;
  float* in_g_rows_group; /* out: [rows][in_groups][2] (sum gamma g, sum gamma g xhat) */
  float* in_g_rows_chan;  /* out: [2][rows][cin]: plane 0 sum g (-> dbeta), plane 1 sum g xhat (-> dgamma) */
  /* output side folded (out_rows != NULL): segs[].y = raw conv output, segs[].dy = g of the GroupNorm after it */
  const float* out_rows;
  const float* out_g_rows_group;
  const float* out_gamma;
  int32_t out_groups;
  float out_eps;
  int32_t defer_wgrad;    /* != 0: this call leaves dw alone -- its weight-gradient half (the product V^T dM over the tiles and the
                             G^T dU G back-transform, nothing of which anybody needs before the optimizer step) is run later by
                             rn_conv3x3_winograd_gn_bwd_wgrad FROM THE SAME WORKSPACE, which the caller keeps untouched until then:
                             e.g. on a side stream beside the backbone's latency-bound backward pass */
} rn_wino_gn_bwd;
/* dx (or g, see above) for every segment and dw (+)=; workspace rn_conv3x3_winograd_bwd_workspace bytes. */
int rn_conv3x3_winograd_gn_bwd(const rn_conv_seg* segs, int nseg, int cin, int cout, const float* w, float* dw, int accumulate,
                               int tile, const rn_wino_gn_bwd* gn, void* workspace, size_t workspace_bytes, const float* v_buf,
                               const float* urot_buf, rn_stream_t stream);
/* The deferred half of a rn_conv3x3_winograd_gn_bwd call made with gn->defer_wgrad: same segments, cin, cout, tile, workspace
 * (untouched since), v_buf and the same urot_buf-was-given flag; dw (+)= as `accumulate` says. */
int rn_conv3x3_winograd_gn_bwd_wgrad(const rn_conv_seg* segs, int nseg, int cin, int cout, float* dw, int accumulate, int tile,
                                     void* workspace, size_t workspace_bytes, const float* v_buf, int urot_was_given, rn_stream_t stream);
/* Which kernels one layer's rn_conv3x3_winograd_gn ("fwd") and rn_conv3x3_winograd_gn_bwd ("bwd") calls launch, decided by the
 * planner the launches use (the same functions, the same constants, RN_WINO_GN_W / RN_WINO_W and the product switches read at
 * the call) -- for tests that must know which branch a shape takes.  Host only: touches no device, launches nothing; of the
 * segments only n, h, w are read.  in_groups / out_groups: the groups of the folded GroupNorm on the input / output side
 * (rn_wino_gn.in_groups / out_groups), 0: that side is not folded (in_rows / out_rows NULL).
 * A call has an input side (fwd: x, cin channels; bwd: dy, cout channels) and an output side (fwd: y, cout; bwd: dx, cin).
 * The CHUNK kernels (a block = 16 tiles of one sample x 16 lanes of W channels; `slabs` blocks side by side cover the
 * channels) run every folded side, the fwd input side and the bwd output side; a side that is not folded otherwise runs the
 * GRID-STRIDE kernels of rn_conv3x3_winograd (the fwd output transform of a layer that emits no rows, the dy transforms of
 * plain dy).  A chunk kernel on a folded side reads its sample's statistic rows: staged in LDS while groups per block x
 * chunks per sample <= 1024, from global memory otherwise. */
typedef struct rn_wino_gn_plan_call {
  int32_t in_chunked, out_chunked;  /* 1: chunk kernel, 0: grid-stride kernel */
  int32_t in_w, out_w;              /* channels per thread (1, 2, 4) of the side's chunk kernel; 0: not chunked */
  int32_t in_slabs, out_slabs;      /* channels / (16 W) of the side's chunk kernel; 0: not chunked */
  int32_t stride_w;                 /* channels per thread (1, 2, 4) of the call's grid-stride kernel; 0: it launches none */
  int32_t in_staged, out_staged;    /* 1: every segment's rows staged in LDS, 0: some segment reads them from global memory,
                                       -1: the side reads no rows (not folded; fwd output side: it writes them) */
} rn_wino_gn_plan_call;
typedef struct rn_wino_gn_plan {
  rn_wino_gn_plan_call fwd, bwd;
  int32_t tiles, chunks;            /* Winograd tiles and chunks (= statistic rows, rn_wino_gn_rows) of all segments */
  int32_t partial_chunk;            /* 1: some segment's tiles per sample are no multiple of 16 (its last chunk is partly empty) */
  int32_t u_frag;                   /* 1: the forward product reads U as the fragment image (rn_x3_bfrag_ok), 0: as fp32 */
} rn_wino_gn_plan;
int rn_conv3x3_winograd_gn_plan(const rn_conv_seg* segs, int nseg, int cin, int cout, int tile, int in_groups, int out_groups,
                                rn_wino_gn_plan* plan);
/* out[i] = (accumulate ? out[i] : 0) + sum_r in[r * count + i], r < nrows, fixed order (bit-reproducible); joins the
 * caller's deferred batch when `defer` is given.  Finishes dgamma / dbeta from in_g_rows_chan. */
int rn_reduce_rows(const float* in, float* out, int64_t count, int nrows, int accumulate, rn_stream_t stream, rn_reduce_list* defer);

/* ------------------------------------------------------------------ MobileNetV2 bottleneck chain
 * Replaces the chain  [conv1x1, Normalization, act, Dropout] -> [DepthwiseConv2D 3x3, Normalization, act, Dropout] ->
 * [conv1x1, Normalization, Dropout] (+ input)  of mobilenet_v2.py:41-94 (GroupNorm variant: normalization.py:20-35),
 * forward and backward, with every GroupNorm applied by its CONSUMER while it loads:
 *   - a conv / depthwise kernel writes its RAW output y and, as a by-product, rows of per-group (sum, sum of squares);
 *   - the next kernel merges the rows of its sample (fixed order, fp64) and computes dropout(act(GN(y))) [+ residual] on the
 *     fly in its operand load -- the normalised tensor is never written (a pointwise conv can also write it out once,
 *     `materialise`: the bottleneck's output is needed again as the next bottleneck's residual / as a pyramid tap);
 *   - backward: a data-gradient kernel turns its result into g = d * act'(z) * dropout mask of the GroupNorm block it enters
 *     from behind, stores it, and emits rows of (sum gamma g, sum gamma g xhat) + per-channel planes (sum g, sum g xhat);
 *     the kernel that needs dy = rstd (gamma g - c1 - xhat c2) of that GroupNorm computes it while loading g and y.
 * One bottleneck = 3 launches forward, 3 backward (13 through the layer-by-layer path).  No kernel waits for another
 * block, no atomics; results are bitwise reproducible.  fp32, NHWC; channels % 4 == 0; a sample's pixels are a multiple
 * of the pointwise kernels' tile height (RN_EUNSUPPORTED otherwise: use the layer-by-layer entry points).
 *
 * rn_mb_rows: [n][rows_per_sample][width] pairs of floats.  Entry (group g, producer N-tile t) of a row sits at position
 * g + t: a pointwise conv's N-tiles (bn channels each) cut through groups, consecutive tiles share at most one group, so
 * the positions are unique; a depthwise block owns whole groups (bn >= channels: t = 0).  Group g's total is the sum over
 * the rows and over t = (g cpg) / bn .. ((g + 1) cpg - 1) / bn.  The *_rows functions fill the layout and return the bytes. */
typedef struct rn_mb_rows {
  float* rows;
  int32_t rows_per_sample, width, bn;
} rn_mb_rows;

/* one GroupNorm (+ activation + dropout) block, described for the kernels on either side of it */
typedef struct rn_mb_norm {
  const float* y;             /* the raw conv output it normalises, [n, hw, c] */
  rn_mb_rows stat;            /* forward: y's (sum, sum sq) rows; stat.rows == NULL: mean / rstd below are READ, not written */
  float* mean; float* rstd;   /* [n, groups]; the forward consumer writes them, every backward kernel reads them */
  const float* gamma; const float* beta;   /* [c] */
  int32_t c, groups, act;     /* act: rn_act applied after the normalisation */
  float eps, drop_rate;       /* dropout after the activation: keep iff hash(seed, element index of y) >= rate (rn_gn_params) */
  uint64_t drop_seed; const uint64_t* drop_seed_dev;
} rn_mb_norm;

/* A consumer block merges at most rn_mb_rows_max() rows of its sample.  The largest maps produce more (one row per tile):
 * rn_mb_compact_rows sums consecutive rows (fp64, fixed order) into <= 8 per sample first -- one small launch. */
int rn_mb_rows_max(void);
size_t rn_mb_compact_rows_layout(int n, const rn_mb_rows* in, rn_mb_rows* out);   /* fills `out`'s layout, returns its bytes */
int rn_mb_compact_rows(const rn_mb_rows* in, const rn_mb_rows* out, int n, rn_stream_t stream);

/* y[n,hw,cout] = A w, w [cin, cout] (a 1x1 Conv2D kernel, HWIO), A = x (plain) or dropout(act(GN(in->y))) [+ residual];
 * `materialise` (optional, with `in`): A is also written out, [n,hw,cin].  stat_out (optional): y's rows (layout from
 * rn_mb_pointwise_rows with the GroupNorm's `groups` that follows y). */
size_t rn_mb_pointwise_rows(int n, int hw, int cin, int cout, int groups, rn_mb_rows* layout);
int rn_mb_pointwise_fwd(const float* x, const rn_mb_norm* in, const float* residual, float* materialise, const float* w, float* y,
                        int n, int hw, int cin, int cout, const rn_mb_rows* stat_out, int stat_groups, rn_stream_t stream);
/* y = depthwise3x3(dropout(act(GN(in->y)))), TF SAME padding, stride 1 or 2; w [3,3,c]; stat_out: y's rows */
size_t rn_mb_depthwise_rows(int n, int h, int w, int c, int stride, int groups, rn_mb_rows* layout);
int rn_mb_depthwise_fwd(const rn_mb_norm* in, const float* w, float* y, int n, int h, int wd, int stride, const rn_mb_rows* stat_out,
                        int stat_groups, rn_stream_t stream);
/* out = dropout(act(GN(in->y))) [+ residual]: writes a normalised tensor out (the end of a chain; tests) */
int rn_mb_apply(const rn_mb_norm* in, const float* residual, float* out, int n, int hw, rn_stream_t stream);

/* the gradient of a conv output y, as a backward kernel loads it */
typedef struct rn_mb_dy {
  const float* dy;            /* plain gradient [n,hw,c]; or NULL: computed from the fields below while loading */
  const rn_mb_norm* norm;     /* the GroupNorm block behind y (mean / rstd as the forward pass wrote them) */
  const float* g;             /* [n,hw,c] the gradient entering that block from behind */
  int32_t g_plain;            /* 0: g already carries act' and the dropout mask (a data-gradient epilogue wrote it);
                                 1: g is the gradient of the block's OUTPUT: the dropout mask is applied while loading
                                    (the block's activation must be RN_ACT_NONE) */
  rn_mb_rows grows;           /* the rows (sum gamma g, sum gamma g xhat) g's producer wrote */
} rn_mb_dy;
/* what a data-gradient kernel does with its result d = dL/d(input of the conv) */
typedef struct rn_mb_gout {
  float* out;                 /* [n,hw,c] */
  const float* add1; const float* add2;   /* optional, d += add1 + add2 (the residual path's gradient, a pyramid tap's gradient) */
  const rn_mb_norm* norm;     /* NULL: out = d.  Else the conv's input was norm's block output: g = d act'(z) mask */
  int32_t store_plain;        /* with norm: 1: out = d (its loader applies the mask: rn_mb_dy.g_plain), 0: out = g */
  rn_mb_rows grows;           /* out: rows of (sum gamma g, sum gamma g xhat) */
  float* planes;              /* out: [2][n * grows.rows_per_sample][c] per-channel (sum g | sum g xhat) of every row;
                                 rn_reduce_rows over the rows gives dbeta | dgamma */
} rn_mb_gout;
/* both gradients of rn_mb_pointwise_fwd in one launch: gout->out = dy w^T (+ ...), dw = A^T dy (A = x or the block of `in`).
 * workspace: rn_mb_pointwise_bwd_workspace bytes (weight-gradient partial sums, summed by the deferred reduction). */
size_t rn_mb_pointwise_bwd_rows(int n, int hw, int cin, int cout, int groups, rn_mb_rows* layout);   /* layout of gout->grows */
size_t rn_mb_pointwise_bwd_workspace(int n, int hw, int cin, int cout);
int rn_mb_pointwise_bwd(const float* x, const rn_mb_norm* in, const rn_mb_dy* dy, const float* w, float* dw, const rn_mb_gout* gout,
                        int n, int hw, int cin, int cout, void* workspace, size_t workspace_bytes, rn_stream_t stream,
                        rn_reduce_list* defer);
/* both gradients of rn_mb_depthwise_fwd in one launch: gout (norm = in) receives the data gradient, dw [3,3,c] */
size_t rn_mb_depthwise_bwd_rows(int n, int h, int w, int c, int stride, int groups, rn_mb_rows* layout);
size_t rn_mb_depthwise_bwd_workspace(int n, int h, int w, int c, int stride);
int rn_mb_depthwise_bwd(const rn_mb_norm* in, const rn_mb_dy* dy, const float* w, float* dw, const rn_mb_gout* gout, int n, int h,
                        int wd, int stride, void* workspace, size_t workspace_bytes, rn_stream_t stream, rn_reduce_list* defer);
/* Which 3x3 tap loops the two depthwise kernels run.  Process-wide switch (default on, RN_MB_DW_TAPS=0 at first use: off).
 *   on   one base address per pixel and block-uniform tap offsets; the backward data gradient reads no tap that is an exact
 *        zero (stride 2: 4, 2, 2 or 1 of the nine by the pixel's parity class) and needs no mask
 *   off  the earlier loops: every tap's index, validity and clamped address per pixel
 * Same terms in the same order: y, the data gradient, dw and gout->grows / planes are equal either way.  For comparing the
 * two in one process. */
int rn_set_mb_dw_taps(int on);
int rn_get_mb_dw_taps(void);

/* ------------------------------------------------------------------ IoU
 * Replaces utils.iou (utils.py:62-97; known answers utils_test.py:99-118): boxes are corners [y1, x1, y2, x2].
 * pairwise != 0: out[i * nb + j] = IoU(a[i], b[j]) -- the [O,1,1,1,4] x [1,H,W,A,4] -> [O,H,W,A] broadcast of
 * dataset.py:57-60; pairwise == 0 (na == nb): out[i] = IoU(a[i], b[i]).  Boxes that do not overlap give 0
 * (utils.py:82-86); `malformed` (one int32, zeroed by the caller) is set to 1 if any box has y2 < y1 or x2 < x1
 * (the reference's tf.assert_* at utils.py:65-68).  Same float32 operation order as the assignment kernel.
 */
int rn_iou(const float* a, int64_t na, const float* b, int64_t nb, int pairwise, float* out, int32_t* malformed,
           rn_stream_t stream);

/* ------------------------------------------------------------------ anchor assignment
 * Replaces dataset.level_labels / build_labels (dataset.py:43-142) for a batch of images:
 * IoU of every anchor with every object -> arg-max/max -> one-hot class (zero where IoU<0.5),
 * log-space regression target of the arg-max object, trainable = IoU<0.4 || IoU>=0.5.
 * Degenerate objects (zero / negative extent) behave as in the reference's reduce_sum(regression * one_hot, 0)
 * (dataset.py:118-121): the log-size component of every anchor NOT assigned to such an object is NaN (-inf * 0).
 * boxes [nimg, max_obj, 4] normalised corners, class_ids [nimg, max_obj], num_obj [nimg] (>=1).
 * anchor_sizes [A,2] already divided by the image size (levels.py:38-44, dataset.py:53).
 */
int rn_anchor_assign(const float* boxes, const int32_t* class_ids, const int32_t* num_obj, int nimg, int max_obj,
                     const float* anchor_sizes, int num_anchors, int grid_h, int grid_w, int num_classes,
                     float* cls_out, float* reg_out, uint8_t* trainable_out, int32_t* argmax_out,
                     rn_stream_t stream);
/* build_labels (dataset.py:126-142): the same for every pyramid level of the batch in one launch. */
#define RN_MAX_LEVELS 8
typedef struct rn_assign_level {
  const float* anchor_sizes; /* [A,2] of this level, normalised */
  int grid_h, grid_w;
  float* cls_out;            /* [nimg, grid_h, grid_w, A, C] */
  float* reg_out;            /* [nimg, grid_h, grid_w, A, 4] */
  uint8_t* trainable_out;    /* [nimg, grid_h, grid_w, A] */
  int32_t* argmax_out;       /* optional (NULL): index of the matched object */
} rn_assign_level;
int rn_anchor_assign_levels(const float* boxes, const int32_t* class_ids, const int32_t* num_obj, int nimg, int max_obj,
                            const rn_assign_level* levels, int nlevel, int num_anchors, int num_classes,
                            rn_stream_t stream);
/* The reference's batch of two (dataset.py:182-204: [sample, augmentation.flip(sample)], augmentation.py:5-22) straight from
 * the assignment: every source image i is assigned ONCE and written to two batch slots -- [2i] as is, [2i+1] with every
 * map reversed along W and the x shift (regression component 1) negated -- so the mirror image's labels are the flipped
 * MAPS bit for bit (assigning mirrored boxes rounds 1 - x differently).  Outputs hold 2 * nimg images. */
int rn_anchor_assign_levels_pair(const float* boxes, const int32_t* class_ids, const int32_t* num_obj, int nimg, int max_obj,
                                 const rn_assign_level* levels, int nlevel, int num_anchors, int num_classes,
                                 rn_stream_t stream);

/* ------------------------------------------------------------------ decode + NMS
 * rn_decode_boxes: utils.regression_postprocess (utils.py:108-117): exp, anchor scale, add
 *   cell centre, centre->corner.  reg [n,h,w,A,4] -> boxes [n,h,w,A,4].
 * rn_detect_*: utils.boxes_decode + merge_boxes_decoded + nms_classwise (utils.py:183-227,
 *   tf.image.non_max_suppression max 1000 / IoU>0.5) for a whole batch in one pass.
 */
int rn_decode_boxes(const float* reg, const float* anchor_sizes, float* boxes, int n, int h, int w, int num_anchors,
                    rn_stream_t stream);

typedef struct rn_det_level {
  const void* prob;   /* [n, rows_per_image, C] class probabilities (post-sigmoid), fp32 or fp16 (prob_f16) */
  const float* boxes; /* [n, rows_per_image, 4] decoded corner boxes, or NULL: decode on the fly from the fields below */
  int64_t rows_per_image;
  /* boxes == NULL: only the rows that become candidates are decoded (utils.regression_postprocess arithmetic,
   * utils.py:100-117, same bits as rn_decode_boxes) -- ~1 % of the rows instead of a full pass over the level */
  const void* regression;    /* [n, grid_h, grid_w, num_anchors, 4] raw network output, fp32 or fp16 (regression_f16) */
  const float* anchor_sizes; /* [num_anchors, 2] normalised (h, w)                      */
  int32_t grid_h, grid_w, num_anchors;
  /* BASELINE configs[4] (fp16 inference): the maps stay in the storage type the net wrote them in -- 2 bytes per
   * element through the scan instead of 4; all arithmetic (max, threshold, decode, IoU) is fp32 on the exact values. */
  int32_t prob_f16;        /* != 0: prob holds fp16                                                                */
  int32_t regression_f16;  /* != 0: regression holds fp16                                                           */
  /* != 0: prob holds the class LOGITS (classification.unscaled); the scan applies the sigmoid of train.py:74 /
   * utils.py:246 element by element on the fly (same expression as rn_act_fwd(RN_ACT_SIGMOID), so fp32 results
   * equal sigmoid-then-scan bit for bit) -- the probability map is never written or re-read */
  int32_t prob_is_logit;
} rn_det_level;

typedef struct rn_det_params {
  int32_t n, num_classes, max_per_class; /* 1000 = utils.NMS_MAX_OUTPUT_SIZE          */
  float score_threshold, iou_threshold;  /* 0.5 / 0.5                                  */
  int64_t max_candidates;                /* capacity of the candidate buffers          */
} rn_det_params;

size_t rn_detect_workspace(const rn_det_level* levels, int nlevels, const rn_det_params* p);
/* outputs (device): out_boxes [max_candidates,4], out_scores, out_class (int32), out_image (int32),
 * out_anchor (int64 flat index of the row inside its image, levels concatenated P3..P7):
 * survivors in (image, class, score-desc, index-asc) order; counts[0]=#candidates,
 * counts[1]=#survivors, counts[2..2+n) survivors per image. */
int rn_detect(const rn_det_level* levels, int nlevels, const rn_det_params* p, float* out_boxes, float* out_scores,
              int32_t* out_class, int32_t* out_image, int64_t* out_anchor, int64_t* counts, void* workspace,
              size_t workspace_bytes, rn_stream_t stream);

/* utils.boxes_decode alone (utils.py:183-195) for a batch: candidates (max prob > threshold) in
 * row-major anchor order, no sort / NMS.  Same outputs as rn_detect; counts[0]=counts[1]=#candidates. */
int rn_boxes_decode(const rn_det_level* levels, int nlevels, const rn_det_params* p, float* out_boxes,
                    float* out_scores, int32_t* out_class, int32_t* out_image, int64_t* out_anchor, int64_t* counts,
                    void* workspace, size_t workspace_bytes, rn_stream_t stream);
/* utils.nms_classwise / utils.nms (utils.py:198-220) on already decoded boxes: K = *count_dev
 * (device scalar) rows of boxes/scores/class_ids/image_ids; p->max_candidates >= K is the buffer
 * capacity.  Output order (image, class, score desc, index asc); out_index = row of the input. */
size_t rn_nms_classwise_workspace(const rn_det_params* p);
int rn_nms_classwise(const float* boxes, const float* scores, const int32_t* class_ids, const int32_t* image_ids,
                     const int64_t* count_dev, const rn_det_params* p, float* out_boxes, float* out_scores,
                     int32_t* out_class, int32_t* out_image, int64_t* out_index, int64_t* counts, void* workspace,
                     size_t workspace_bytes, rn_stream_t stream);

/* Which kernels one rn_detect / rn_boxes_decode call with these levels and parameters launches, and with which grids -- for
 * tests that must know which implementation a shape takes.  It is the decision the entry points themselves run before they
 * launch (one function: the same constants, RN_SCAN_LDS / RN_SCAN_NO_LDS read at the call, RN_SCAN_T / RN_SCAN_NT read once
 * per process).  Host only: touches no device, launches nothing; of the levels only rows_per_image, prob_f16 and
 * prob_is_logit decide (data pointers may be NULL).  nlevels == 0 (levels ignored): the plan of rn_nms_classwise, which runs
 * no scan, offsets or emit pass (scan == RN_DET_SCAN_NONE, their fields 0).  Returns what the launch would return for the
 * same shapes (RN_EINVAL / RN_EUNSUPPORTED), RN_EINVAL for a NULL plan. */
enum rn_det_scan {
  RN_DET_SCAN_NONE = 0,
  RN_DET_SCAN_T = 1,       /* det_scan_t_kernel: fp16 maps of 80 classes, transposed through LDS, non-temporal loads */
  RN_DET_SCAN_T_PLAIN = 2, /* the same with plain loads (RN_SCAN_NT=0)                                                */
  RN_DET_SCAN_Q = 3,       /* det_scan_q_kernel<scan_half, scan_logit, scan_q>: four lanes per row, q chunks per lane */
  RN_DET_SCAN_LDS = 4,     /* det_scan_lds_kernel (RN_SCAN_LDS): rows staged through scan_lds_per_wave bytes per wave  */
  RN_DET_SCAN_GENERIC = 5  /* det_scan_kernel: any class count, levels of mixed storage type / logit flag             */
};
enum rn_det_emit { RN_DET_EMIT_NONE = 0, RN_DET_EMIT_HIST = 1, RN_DET_EMIT_STRIDED = 2 };
enum rn_det_segments {
  RN_DET_SEG_LDS_SCATTER = 1,   /* det_seg_scatter_kernel: the segment scan in every block's LDS               */
  RN_DET_SEG_GLOBAL_SCATTER = 2 /* det_seg_scan_kernel + det_seg_scatter_global_kernel (more than 8192 segments) */
};
typedef struct rn_det_plan {
  int32_t scan;                             /* rn_det_scan */
  int32_t scan_half, scan_logit, scan_q;    /* RN_DET_SCAN_Q: the kernel's template arguments; else 0 */
  int32_t scan_lds_per_wave;                /* RN_DET_SCAN_LDS: bytes per wave; else 0 */
  int32_t scan_grid;                        /* blocks of the scan kernel */
  int32_t offsets_blocks;                   /* blocks of det_offsets_kernel */
  int32_t emit_mode, emit_grid;             /* rn_det_emit, blocks of det_emit_kernel */
  int32_t emit_lds_bytes;                   /* its dynamic LDS */
  int32_t segments;                         /* rn_det_segments (rn_boxes_decode stops before it) */
  int32_t nseg;                             /* n * num_classes: blocks of the sort, NMS and gather kernels */
  uint64_t workspace_bytes;                 /* = rn_detect_workspace / rn_nms_classwise_workspace */
} rn_det_plan;
int rn_detect_plan(const rn_det_level* levels, int nlevels, const rn_det_params* p, rn_det_plan* plan);

/* ------------------------------------------------------------------ optimizer
 * Replaces tf.train.{Momentum,RMSProp,Adam}Optimizer.apply + the L2 regulariser gradient
 * + tf.clip_by_global_norm (train.py:111-134,221) on ONE flat fp32 parameter arena.
 * The arena is cut into blocks of RN_OPT_BLOCK elements; wd_per_block[b] is the L2 scale of
 * the parameter that owns block b (0 for gamma/beta/bias and padding).
 *   g' = (grad*grad_scale + wd*w) * clip_scale  (grad_scale = 1/world_size; clip_scale = clip/max(||grad*grad_scale + wd*w||, clip):
 *                                                the norm includes the regulariser's gradient, as compute_gradients(loss) does)
 */
#define RN_OPT_BLOCK 1024
size_t rn_optimizer_workspace(int64_t count);
/* out[0] = sum(grad^2)*grad_scale^2 (global norm squared), out[1] = sum_b wd_b * 0.5*sum(w^2) */
int rn_grad_norm_l2reg(const float* w, const float* grad, const float* wd_per_block, int64_t count,
                       float grad_scale, float* out2, void* workspace, size_t workspace_bytes, rn_stream_t stream);
/* rn_optimizer_norm_pairs(count): the (double, double) pairs of (sum g'^2, L2 regulariser value) that a pass over a slice
 * [w, w + count) of the arena leaves in `partial` -- the update itself under RN_OPT_F_NORM (below), or rn_grad_norm_partial;
 * rn_norm_reg_finalize sums the pairs of all slices (fixed order) into out2[2] = what rn_grad_norm_l2reg writes. */
int64_t rn_optimizer_norm_pairs(int64_t count);
int rn_norm_reg_finalize(const double* partial, int64_t npairs, float* out2, rn_stream_t stream);

/* Learning-rate schedules evaluated ON THE DEVICE (the reference trains at one constant rate, train.py:114-119; its TODO list:
 * "try other scheduling schemes").  A rate that is a launch argument is a constant of a captured step: a schedule would capture
 * the step again for every rate.  Here the rate is a function of a device step word, so a replayed hipGraph advances it itself.
 * With s = updates already applied, W = warmup_steps, f0 = warmup_factor, T = total_steps, ff = final_factor:
 *   s <  W                 lr = base_lr * (f0 + (1 - f0) * s / W)
 *   s >= W  RN_LR_CONSTANT lr = base_lr
 *           RN_LR_STEP     lr = base_lr * decay_factor ^ #{i : boundaries[i] <= s}
 *           RN_LR_COSINE   lr = base_lr * (ff + (1 - ff) * 0.5 * (1 + cos(pi * min(1, (s - W) / (T - W)))))
 * all in double, rounded to float once.  Checked by rn_step_control_eval: kind; warmup_steps >= 0; f0, ff in [0, 1]; n_boundaries in
 * [0, RN_LR_MAX_BOUNDARIES], boundaries >= 0 and strictly increasing; total_steps > warmup_steps (RN_LR_COSINE needs it; the
 * other kinds do not read it and also take 0 = unset).  The rate is evaluated by rn_step_control_eval (RN_CTL_F_LR, below). */
enum rn_lr_kind { RN_LR_CONSTANT = 0, RN_LR_STEP = 1, RN_LR_COSINE = 2 };
#define RN_LR_MAX_BOUNDARIES 8
typedef struct rn_lr_schedule {
  int32_t kind;
  int32_t n_boundaries;
  double base_lr, warmup_factor, final_factor, decay_factor;
  int64_t warmup_steps, total_steps;
  int64_t boundaries[RN_LR_MAX_BOUNDARIES];
} rn_lr_schedule;
/* THE STEP'S CONTROL WORDS: one one-thread launch ahead of the update forms every device word the update kernels read, so that no
 * launch argument changes from step to step and a replayed hipGraph advances all of them by itself.  The descriptor lives in host
 * memory, is read before the call returns and travels to the kernel by value.  `features` says which of the four parts run -- in
 * this order -- and which fields are set; the fields of a clear feature stay 0 / null.
 * RN_CTL_F_ACCUM  gradient accumulation (the reference takes one optimizer step per batch, train.py:111-134; a larger effective
 *   batch than fits in memory is the usual reason to sum the gradients of A batches first).  A = accumulate_steps; a micro-step is
 *   one forward + backward pass, an update is applied on every A-th one, from the MEAN of the last A gradients (GroupNorm is per
 *   sample, so that is the gradient of the A-times-larger batch but for the dropout masks, drawn per micro-step).
 *     p = *micro_dev % A;  accum_dev[0] = p;  accum_dev[1] = (p == A - 1);  *micro_dev += 1
 * RN_CTL_F_GUARD  a guard against non-finite gradients (the reference trains on whatever its graph computes: a NaN regression
 *   target from a ground-truth box of zero extent reaches every weight).  The criterion is the float rn_norm_reg_finalize leaves,
 *   so the launch stands BEHIND it: sum g'^2 over the whole arena is not finite iff some g' is NaN or inf or the sum overflows.
 *     f = isfinite(norm_sq[0]);  gate_dev[0] = 0;  gate_dev[1] = f;  f ? (skipped_dev[1] = 0) : (skipped_dev[0] += 1, skipped_dev[1] += 1)
 *   so gate_dev has accum_dev's layout and skipped_dev = [updates skipped in all, updates skipped in a row].
 * The two parts below run behind the gate accum_dev[1] (ACCUM) or gate_dev[1] (GUARD), always without either.  A closed gate
 * leaves lr_dev, ema_dev, *step_dev and *ema_updates_dev as they are: both words, and Adam's bias correction, count APPLIED updates.
 * RN_CTL_F_LR     s = *step_dev;  lr_dev[0] = lr(s) of `schedule` (above);  lr_dev[1] = the rate the update kernel multiplies by --
 *   for optimizer_kind RN_OPT_ADAM lr(s) * sqrt(1 - 0.999^t) / (1 - 0.9^t), t = s + 1, formed in double from the rounded lr(s)
 *   exactly as rn_optimizer_update forms it from its float `lr`; lr(s) itself for the other kinds;  *step_dev = s + 1.
 * RN_CTL_F_EMA    an exponential moving average of the weights, kept by the pass that updates them
 *   (tf.train.ExponentialMovingAverage; the reference trains and evaluates the raw weights only).  With n = updates applied before
 *   this one and w' the weight after it:
 *     d(n) = min(ema_decay, (1 + n) / (10 + n))   ema_warmup != 0
 *          = ema_decay                            ema_warmup == 0
 *     e   <- e - (e - w') * (1 - d(n))            in fp32, per element (RN_OPT_F_EMA)
 *   n = *ema_updates_dev;  ema_dev[0] = d(n);  ema_dev[1] = 1 - d(n), each formed in double and rounded to float once;
 *   *ema_updates_dev = n + 1.  The count is the average's own word (a constant-rate step has no step word).
 * Checked before the launch, each RN_EINVAL with a message: non-null c; no unknown feature bit and at least one; never ACCUM with
 * GUARD (one gate; rn_optimizer_update refuses the pair too); a known optimizer_kind; micro_dev and accum_dev both given iff ACCUM,
 * accumulate_steps >= 1; norm_sq, gate_dev and skipped_dev all given iff GUARD, 4 / 4 / 8-byte aligned; step_dev and lr_dev both
 * given iff LR, and the schedule's own list (above); ema_updates_dev and ema_dev both given iff EMA, 0 < ema_decay < 1. */
enum rn_ctl_feature { RN_CTL_F_ACCUM = 1, RN_CTL_F_GUARD = 2, RN_CTL_F_LR = 4, RN_CTL_F_EMA = 8 };
typedef struct rn_step_control {
  uint32_t features; int32_t optimizer_kind;
  int32_t accumulate_steps; uint64_t* micro_dev; int32_t* accum_dev;               /* ACCUM */
  const float* norm_sq; int32_t* gate_dev; uint64_t* skipped_dev;                   /* GUARD */
  rn_lr_schedule schedule; uint64_t* step_dev; float* lr_dev;                       /* LR    */
  double ema_decay; int32_t ema_warmup; uint64_t* ema_updates_dev; float* ema_dev;  /* EMA   */
} rn_step_control;
int rn_step_control_eval(const rn_step_control* c, rn_stream_t stream);
/* The norm pass of rn_grad_norm_l2reg for a SLICE [w, w + count) of the arena (wd_per_block points at the slice's first block):
 * rn_optimizer_norm_pairs(count) (double, double) pairs of (sum g'^2, L2 regulariser value) into `partial`, in the layout
 * RN_OPT_F_NORM writes; rn_norm_reg_finalize over the pairs of all slices gives [sum g'^2, reg].  The caller owns
 * `partial`: no workspace, nothing a capture may not contain. */
int rn_grad_norm_partial(const float* w, const float* grad, const float* wd_per_block, int64_t count, float grad_scale,
                         double* partial, rn_stream_t stream);
/* THE UPDATE: one pass over a slice [w, w + count) of the arena (wd_per_block points at the slice's first block), fp32 per element,
 * float4 accesses, 16 B/element for RN_OPT_MOMENTUM and 20 for the other kinds (w, grad, state1 [, state2] read; all but grad
 * written).  With g' as above, lr the rate and state1 / state2 = momentum-acc | rms, mom | m, v:
 *   RN_OPT_MOMENTUM  a = 0.9 a + g';                                       w -= lr a
 *   RN_OPT_RMSPROP   a = 0.9 a + 0.1 g'^2;  b = 0.9 b + lr g' / sqrt(a + 1e-10);  w -= b
 *   RN_OPT_ADAM      a = 0.9 a + 0.1 g';    b = 0.999 b + 0.001 g'^2;      w -= lr_t a / (sqrt(b) + 1e-8),
 *                    lr_t = lr * sqrt(1 - 0.999^step) / (1 - 0.9^step), formed on the host in double; `step` is 1-based
 * The descriptor lives in host memory and is read before the call returns.  `features` says what the caller means: it selects the
 * kernel and says which of the fields below the first three lines are set -- the fields of a clear feature stay 0 / null.
 * Always: kind (enum rn_opt), w, grad, state1, state2 (RN_OPT_RMSPROP / RN_OPT_ADAM), wd_per_block, count, lr, grad_scale, step;
 *   advance_counter (optional): a device word incremented by advance_by in the same launch -- the per-step counter the fused
 *   dropouts hash (rn_gn_params.drop_seed_dev), so that the next step (or hipGraph replay) draws fresh masks (tf.layers.Dropout
 *   draws new noise every session.run, mobilenet_v2.py:62).
 * RN_OPT_F_NORM   the pass also forms the slice's share of (sum g'^2, L2 regulariser value), both at the weights BEFORE the update
 *   (one read of w and grad instead of two): rn_optimizer_norm_pairs(count) pairs into `partial`.  No clipping then: the norm is
 *   not an input.  A trainer can so update the heads + FPN slice while the backbone's backward pass runs.
 * RN_OPT_F_LRDEV  the rate is lr_dev[1], what rn_step_control_eval left there -- bias correction included -- instead of `lr`; `lr`
 *   and `step` are not read.  Same kernel, same grid, same `partial` layout.  Without it RN_OPT_ADAM needs step >= 1, an argument
 *   that DOES change from step to step.
 * RN_OPT_F_EMA    the pass also keeps the moving average `ema` (count floats, 16-byte aligned, laid out like w) with 1 - d(n) read
 *   from ema_dev[1], what rn_step_control_eval left there.  w, the slots, the pairs and the counter come out exactly as without it:
 *   the average is one more load, one fused multiply-add and one more store per element (+8 B/element).
 * RN_OPT_F_CLIP   clip_scale = clip_norm / max(sqrt(norm_sq[0]), clip_norm), formed by the kernel from the device scalar, so
 *   nothing step-dependent is among the launch arguments and the clipped update can be a node of a captured step like the
 *   unclipped one.  The norm is an INPUT of this pass, so the pass before it forms it (rn_grad_norm_partial +
 *   rn_norm_reg_finalize, or rn_grad_norm_l2reg): never with NORM.  Without CLIP clip_norm is 0 and norm_sq null.
 * RN_OPT_F_ACCUM  (with NORM; never with CLIP or GATE) the update on an accumulated gradient.  Every wave reads accum_dev[0..1] =
 *   [p, applying], what rn_step_control_eval left there, once and the launch runs ONE of three loops, gs = grad_scale:
 *     p == 0, not applying   acc  = grad * gs                 acc is not read                              8 B/element
 *     p  > 0, not applying   acc += grad * gs                                                              12 B/element
 *     applying               G = (acc + grad * gs) * inv_accum;  g' = G + wd*w;  the update, the average and the (sum g'^2,
 *                            regulariser) pair exactly as formed from g' without ACCUM; acc is not written (the next
 *                            cycle's first launch overwrites it)                                           +4 B/element
 *   A launch that does not apply leaves w, the slots, ema and its `partial` pairs untouched: rn_norm_reg_finalize then gives the
 *   LAST update's (sum g'^2, regulariser) again.  advance_counter is bumped by every launch (fresh dropout masks per micro-step).
 *   acc: count floats, 16-byte aligned, laid out like w; zero-filled at the start.  inv_accum: the caller passes 1 / A.
 * RN_OPT_F_GATE   (never with NORM or ACCUM) the update behind the guard's gate: every wave reads gate_dev[1], what
 *   rn_step_control_eval left there, once; on 0 the launch bumps advance_counter (fresh dropout masks next step) and returns without
 *   touching w, the slots or ema; otherwise it is the ungated update, bit for bit.
 * A launch on another stream that reads lr_dev / ema_dev / accum_dev must be ordered behind the control launch that wrote it.
 * Checked before any launch, each RN_EINVAL with a message: non-null u, w, grad, state1, wd_per_block; count > 0 and whole
 * blocks; a known kind; state2 for RN_OPT_RMSPROP / RN_OPT_ADAM; no unknown feature bit; NORM with neither CLIP nor GATE; ACCUM
 * with NORM and with neither CLIP nor GATE; partial non-null iff NORM; lr_dev non-null iff LRDEV; ema and ema_dev both given iff
 * EMA, ema 16-byte aligned; acc and accum_dev both given iff ACCUM, acc 16-byte aligned, 0 < inv_accum <= 1; gate_dev non-null iff
 * GATE, 4-byte aligned; clip_norm > 0 and norm_sq with CLIP, clip_norm == 0 and null norm_sq without (NaN refused either way);
 * step >= 1 for RN_OPT_ADAM without LRDEV.  A pointer that is null by mistake is so refused instead of selecting another kernel. */
enum rn_opt_feature { RN_OPT_F_NORM = 1, RN_OPT_F_LRDEV = 2, RN_OPT_F_EMA = 4, RN_OPT_F_CLIP = 8,
                      RN_OPT_F_ACCUM = 16, RN_OPT_F_GATE = 32 };
typedef struct rn_opt_update {
  int32_t kind; uint32_t features;
  float* w; const float* grad; float* state1; float* state2; const float* wd_per_block; int64_t count;
  float lr; float grad_scale; int64_t step;
  uint64_t* advance_counter; uint64_t advance_by;
  double* partial;                                        /* NORM  */
  const float* lr_dev;                                    /* LRDEV */
  float* ema; const float* ema_dev;                       /* EMA   */
  float clip_norm; const float* norm_sq;                  /* CLIP  */
  float* acc; float inv_accum; const int32_t* accum_dev;  /* ACCUM */
  const int32_t* gate_dev;                                /* GATE  */
} rn_opt_update;
int rn_optimizer_update(const rn_opt_update* u, rn_stream_t stream);
/* *counter += inc on the stream (the same counter, for callers that run backward passes without an optimizer step) */
int rn_counter_add(uint64_t* counter, uint64_t inc, rn_stream_t stream);
/* p[0..count) = 0 (16-byte aligned): the gradient arena before a backward pass (the reference's graph zero-initialises
 * its gradient accumulators, train.py:121-123) */
int rn_zero(float* p, int64_t count, rn_stream_t stream);

/* out = a + b for up to RN_MAX_SEG tensors in one launch (count floats each, 16-byte aligned): the sum autograd forms when
 * a tensor feeds two branches -- a bottleneck's input (expand conv + identity, mobilenet_v2.py:91-92), a pyramid level
 * (class + box subnet, retinanet.py:283-291), C5 (P5 + P6, retinanet.py:214-216). */
typedef struct rn_add_seg { const float* a; const float* b; float* out; int64_t count; } rn_add_seg;
int rn_add_segs(const rn_add_seg* segs, int nseg, rn_stream_t stream);

/* Measurement aid (bench.py `config.collective_standin`; not on the product path): what a ring all-reduce under the
 * backbone's backward pass would take from the compute stream on ONE GPU -- `blocks` workgroups of 256 threads (RCCL runs
 * one workgroup per channel) stream `bytes` from src to dst (16-byte aligned), paced by the constant 100 MHz clock so the
 * copy lasts ~target_us (2 (R-1)/R x slice bytes at the ~150 GB/s a ring gets from one xGMI link).  Launch it on a side
 * stream.  The reference's MirroredStrategy (train.py:261-267) has no counterpart: this replaces nothing. */
int rn_debug_collective_standin(const void* src, void* dst, int64_t bytes, int blocks, float target_us, rn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RN_HIP_H */
