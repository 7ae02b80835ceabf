/*
 * yolo2_hip.h — C ABI of libyolo2_hip.so: the MI355X (gfx950) YOLOv2 hot path.
 *
 * The reference (ruiminshen/yolo2-pytorch) has no FFI: its "operator API" for this path is a set of
 * Python call signatures.  This header is the boundary underneath the Python mirror of
 * those signatures (yolo2-pytorch_amd/model, utils.postprocess, utils.iou.torch): every entry point
 * names the reference interface (file:line under /root/reference) whose arithmetic it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers + sizes; no torch types.  All pointers are DEVICE pointers unless a
 *     parameter says "host".  All floating point is fp32; indices int32 unless stated.
 *   - Every call only ENQUEUES work on `stream` (a hipStream_t passed as void*); nothing here
 *     allocates, frees or synchronises.  The caller owns every buffer and keeps it alive until the
 *     stream has drained (PyTorch caching-allocator stream semantics).
 *   - Return value: 0 on success, a negative Y2_E* code on an argument error, or -(1000+hipError_t)
 *     when a launch failed.  Never throws.
 *   - Stateless and re-entrant per stream: safe under one-process-per-GPU data parallelism.
 *   - Activation layout inside the path is NHWC ("pixel-major"): element (b, y, x, c) of a tensor with
 *     pixel stride `ld` lives at ((b*H + y)*W + x)*ld + c.  The plugin boundary (NCHW in / NCHW out,
 *     model/yolo2.py:125-130) is handled by y2_conv0_fwd (reads NCHW) and by the head writing the
 *     [B, rows, cols, A*(5+C)] image that model/__init__.py:122 obtains with permute(0,2,3,1).
 */
#ifndef YOLO2_HIP_H
#define YOLO2_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Y2_OK 0
#define Y2_EINVAL (-1)    /* bad size / null pointer */
#define Y2_EALIGN (-2)    /* pointer or stride not aligned as required */
#define Y2_ENOSUP (-3)    /* combination not supported by this build */

/* Training-mode BN statistics are accumulated with fp64 atomics into Y2_STATS_REPL replicated copies of the
 * [sum | sum of squares] vector (copy = tile index mod Y2_STATS_REPL) to keep atomic contention off the critical
 * path; y2_bn_finalize adds the copies.  A stats buffer therefore holds Y2_STATS_REPL * 2 * C doubles. */
#define Y2_STATS_REPL 32

typedef void* y2_stream_t; /* hipStream_t */

/* Library/ABI version (bump when a signature changes) and the gfx target it was compiled for. */
int y2_abi_version(void);
const char* y2_build_info(void);

/* ------------------------------------------------------------------------------------------------
 * Weight preparation (replaces nothing in the reference: torch keeps [Cout,Cin,kh,kw], model/yolo2.py:57)
 * ------------------------------------------------------------------------------------------------ */

/* Repack a conv weight [Cout][Cin][k][k] (state_dict layout, model/yolo2.py:57) into the GEMM layouts
 * the kernels read.  mode 0 (fprop): dst[co][tap][ci];  mode 1 (dgrad): dst[ci][k*k-1-tap][co]
 * (filters rotated by 180 deg, in/out swapped).  dst holds Cout*Cin*k*k floats. */
int y2_pack_weight(const float* w, float* dst, int Cout, int Cin, int ksize, int mode, y2_stream_t stream);

/* Multi-tensor form for a whole network: ONE launch prepares every listed operand from the state_dict layout [Cout][Cin][k][k]
 * (a training step re-derives ~90 operands from the freshly updated weights; as separate launches they are launch-latency bound).
 * Modes: Y2_PREP_FPROP / Y2_PREP_DGRAD = y2_pack_weight modes 0 / 1;  Y2_PREP_WINO_FPROP / Y2_PREP_WINO_DGRAD = the Winograd
 * filter transform U[16][Cout][Cin] resp. U[16][Cin][Cout] (rotated, in/out swapped) of a 3x3 filter, bit-identical to
 * y2_pack_weight + y2_wino_weight;  Y2_PREP_WINO6_DGRAD = the F(4x4,3x3) data-gradient operand U6[36][Cin][Cout] (rotated, in/out
 * swapped), bit-identical to y2_pack_weight(mode 1) + y2_wino6_weight.
 * dst sizes: Cout*Cin*k*k floats (packs), 16*Cout*Cin floats (2x2-tile transforms), 36*Cout*Cin floats (4x4-tile transform). */
#define Y2_PREP_FPROP 0
#define Y2_PREP_DGRAD 1
#define Y2_PREP_WINO_FPROP 2
#define Y2_PREP_WINO_DGRAD 3
#define Y2_PREP_WINO6_DGRAD 4
#define Y2_PREP_MAX_ITEMS 96
typedef struct {
    const float* src;
    float* dst;
    int32_t Cout, Cin, ksize, mode;
} y2_prep_item;
int y2_prep_weights(const y2_prep_item* items, int32_t count, y2_stream_t stream);

/* Many small range operations in ONE launch (table in the kernel arguments): the zero fills of a training step's accumulation
 * buffers (autograd's zeros, train.py:350), the fp64 -> fp32 hand-out of the affine-parameter gradients, plain copies.
 * n counts ELEMENTS of dst (fp32); src is const double* for Y2_MULTI_F64_TO_F32, const float* for Y2_MULTI_COPY, ignored for ZERO. */
#define Y2_MULTI_ZERO 0
#define Y2_MULTI_F64_TO_F32 1
#define Y2_MULTI_COPY 2
#define Y2_MULTI_MAX_ITEMS 96
typedef struct {
    const void* src;
    float* dst;
    int64_t n;
    int32_t op, reserved;
} y2_multi_item;
int y2_multi(const y2_multi_item* items, int32_t count, y2_stream_t stream);

/* The weighted loss sum of train.py:348-349, `sum(loss[key] * hparam[key] for key in loss)`, over the n <= 64 loss terms in
 * device memory: out[0] = sum_k v[k]*w[k] (left to right); and its gradient out[k] = g[0]*w[k]. */
int y2_small_dot(const float* v, const float* w, int32_t n, float* out, y2_stream_t stream);
int y2_small_scale(const float* g, const float* w, int32_t n, float* out, y2_stream_t stream);

/* Inverse of mode 0 for a weight GRADIENT: src[co][tap][ci] -> dst[Cout][Cin][k][k]. */
int y2_unpack_weight_grad(const float* src, float* dst, int Cout, int Cin, int ksize, y2_stream_t stream);

/* Fold eval-mode BatchNorm (nn.BatchNorm2d eps=1e-5, model/yolo2.py:58) into a per-channel affine:
 * scale = gamma / sqrt(var + eps), shift = beta - mean*scale. */
int y2_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
               float* scale, float* shift, int C, y2_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Convolution forward: model.yolo2.Conv2d.forward (model/yolo2.py:61-65) = conv(k, stride 1,
 * pad (k-1)/2) -> per-channel affine (folded BN, or conv bias) -> LeakyReLU(slope), with the
 * following MaxPool2d(2) (model/yolo2.py:79,86,97), the passthrough `reorg` (model/yolo2.py:33-46)
 * and the `torch.cat` (model/yolo2.py:129) expressed as output addressing.
 * ------------------------------------------------------------------------------------------------ */
typedef struct y2_conv_params {
    const float* x;      /* input, NHWC, pixel stride ldx (>= Cin) */
    const float* w;      /* packed weights, y2_pack_weight mode 0: [Cout][k*k][Cin] */
    const float* scale;  /* [Cout] or NULL (= 1) */
    const float* shift;  /* [Cout] or NULL (= 0); conv bias goes here */
    float* y;            /* full-resolution output or NULL */
    float* y_pool;       /* 2x2/stride-2 max-pooled output or NULL (needs even H and W) */
    double* stats;       /* NULL, or [Y2_STATS_REPL][2*Cout] doubles (pre-zeroed): sum and sum of squares of the RAW
                            conv output per channel are atomically accumulated (training-mode BN statistics) */
    int32_t B, H, W;     /* INPUT spatial size; output = (H + 2*pad - k)/stride + 1 (equal to the input for stride 1 / same padding) */
    int32_t Cin, ldx;
    int32_t Cout;
    int32_t ksize;       /* 1..7 (1 and 3 with stride 1 / same padding take the specialised path) */
    int32_t ldy, coff;   /* y pixel stride and channel offset (concat write-through) */
    int32_t ldp, poff;   /* y_pool pixel stride and channel offset */
    int32_t out_mode;    /* 0: y[b,y,x,coff+n];  1: reorg(stride 2): y[b,y/2,x/2, coff + ((y&1)*2+(x&1))*Cout + n] */
    float slope;         /* LeakyReLU negative slope; 1.0f = no activation */
    int32_t tile;        /* 0 = auto; else force a tile config (see conv_fwd.hip; benchmarking only); an id that names no kernel of
                          * the problem's path is refused with Y2_ENOSUP.  With the fused Winograd algorithms:
                          * 3 = the third-generation kernel (32-tile x 64-channel units, two workgroups per CU) */
    float* workspace;    /* optional scratch (16-B aligned) for the split-K remainder scheme, or NULL */
    int64_t workspace_bytes; /* its size; y2_conv_fwd_workspace_bytes() tells how much a problem can use */
    const float* residual; /* optional [B,Ho,Wo,Cout] (pixel stride ldr) added before the activation (model/resnet.py:59,101) */
    int32_t ldr;
    int32_t stride;      /* 0 or 1 = stride 1; 2 = the strided convs of model/resnet.py:31,71,111 */
    int32_t pad_plus1;   /* 0 = "same" padding (k-1)/2; otherwise padding + 1 */
    int32_t transposed;  /* != 0: data gradient of a conv with this (ksize, stride, pad): x = dz [B,H,W,Cin=Cout_fwd], w = y2_pack_weight
                            mode 1 of the forward weight, result [B,out_h,out_w,Cout=Cin_fwd] (fractionally strided convolution) */
    int32_t out_h, out_w; /* transposed only: spatial size of the forward conv's input */
    int32_t algo;        /* Y2_ALGO_DIRECT (0): implicit GEMM, w = y2_pack_weight output.
                            Y2_ALGO_WINOGRAD (1): F(2x2,3x3) for 3x3 / stride 1 / same padding: w = y2_wino_weight output
                            [16][Cout][Cin]; `workspace` is REQUIRED (transformed input + products, y2_conv_fwd_workspace_bytes) */
    int64_t w_plane;     /* Y2_ALGO_WINOGRAD_SPLIT only: distance in ELEMENTS between the three bf16 planes of w (0 = 16*Cout*Cin, the layout
                            y2_split_bf16x3 gives one operand; larger when many operands were split as one array) */
} y2_conv_params;

#define Y2_ALGO_DIRECT 0
#define Y2_ALGO_WINOGRAD 1
#define Y2_ALGO_WINOGRAD_FUSED 2   /* same transforms, but GEMM + output transform in ONE kernel (no product tensor in memory); Cin % 32 == 0 */
#define Y2_ALGO_WINOGRAD_IMPLICIT 3 /* as FUSED, and the input transform B^T d B happens in that kernel's operand loader: the transformed input
                                      (4x the input) never goes to memory either.  Cin % 32 == 0, a batch chunk's input < 1 GB.
                                      Bit-identical results to FUSED.  (Leaves no transformed input behind for y2_wino_wgrad.) */
#define Y2_ALGO_WINOGRAD_SPLIT 4   /* as WINOGRAD (three kernels, fp32 transforms), but the 16 GEMMs run on the bf16 matrix pipe with every fp32 operand
                                      split into three bf16 planes and six plane products per multiply ("bf16x6", csrc/gemm_split.hip): fp32-level
                                      accuracy at 2.67x the fp32-MFMA rate.  w = y2_split_bf16x3 of the y2_wino_weight output; Cin % 32 == 0.
                                      Opt-in precision mode of the Python layer (Y2_SPLIT_BF16=1); never chosen by the library itself. */

#define Y2_ALGO_WINOGRAD_F43 6     /* three kernels like WINOGRAD, on 4x4 output tiles: Winograd F(4x4,3x3), 36 GEMMs, 2.25x fewer multiply-adds than
                                      F(2x2,3x3) on even maps; w = y2_wino6_weight output [36][Cout][Cin]; y only (no pool / statistics).  Error 8-9e-6 x rms
                                      per layer in an fp32 model (F(2x2,3x3): 1.3e-6): meant for GRADIENTS (the training step's data gradients), not
                                      for the inference path, whose tolerance it would use up */
#define Y2_ALGO_WINOGRAD_F43_PRE 7 /* as F43, but x IS the transformed input [36][T][Cin] (ldx == Cin, T = y2_wino6_tiles(B, H, W)), written by
                                      y2_bn_act_bwd_wino6: no input-transform launch, no transformed input in the workspace */
#define Y2_ALGO_WINOGRAD_SPLIT_F16 5 /* as SPLIT with fp16 plane PAIRS (hi = fp16(s x), lo = fp16(s x - hi): 2 x 11 bits + the residual's sign) and three
                                      products (hi x hi, hi x lo, lo x hi): half the matrix instructions and 4 instead of 6 operand bytes of SPLIT.
                                      fp16 has 5 exponent bits: the operands carry fixed power-of-two scales (V x 2^-4, w x 2^8 - pass 256 to
                                      y2_split_f16x2 for w; the product is rescaled exactly) so that |V| up to 10^6 and |w| up to 255 stay finite;
                                      beyond that the result is Inf / NaN, and operands far BELOW 1 (gradients) lose their low plane to fp16's subnormals - unlike every
                                      other algorithm.  For activations (inference, training forward).  Opt-in (Y2_SPLIT_F16=1). */

/* Two fp16 planes of src * scale (scale a power of two): dst = [2][n] fp16 (4 n bytes).  The weight operand of Y2_ALGO_WINOGRAD_SPLIT_F16 (scale 256). */
int y2_split_f16x2(const float* src, void* dst, long long n, float scale, y2_stream_t stream);
/* 1 if any value handed to the fp16 split since the last reset was outside fp16's range (the affected results hold Inf / NaN), else 0; reset != 0
 * clears the flag.  Synchronises the device (a check for the end of an epoch / a benchmark, not for the hot path). */
int y2_split_f16_overflow(int reset);
/* y2_gemm_split for fp16 plane pairs A = [2][groups][M][K], B = [2][groups][N][K]; C = (A B^T) * out_scale. */
int y2_gemm_split_f16(const void* A, const void* B, float* C, long long M, int32_t N, int32_t K, int32_t ldc, int32_t groups, float out_scale, y2_stream_t stream);

/* Three bf16 planes of an fp32 array (hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid), round to nearest even):
 * dst = [3][n] bf16 (6 n bytes), n % 4 == 0, src 16-B aligned.  The weight operand of Y2_ALGO_WINOGRAD_SPLIT. */
int y2_split_bf16x3(const float* src, void* dst, long long n, y2_stream_t stream);

/* C[g] (M x N, row stride ldc, fp32) = A[g] (M x K) * B[g]^T (N x K) for g < groups on the bf16 matrix pipe, operands as plane triples
 * A = [3][groups][M][K], B = [3][groups][N][K] (y2_split_bf16x3 of the fp32 arrays [groups][M][K] / [groups][N][K]); K % 32 == 0.
 * Two accumulator sets per output (hi x hi products / the five cross products) are added once at the end.
 * The GEMM stage of Y2_ALGO_WINOGRAD_SPLIT, exposed for tests and tools. */
int y2_gemm_split(const void* A, const void* B, float* C, long long M, int32_t N, int32_t K, int32_t ldc, int32_t groups, y2_stream_t stream);

/* Winograd F(2x2,3x3) filter transform U[p][co][ci] = (G g G^T)[p], p = 4*xi + nu, from a packed 3x3 weight
 * (y2_pack_weight mode 0 for the forward conv, mode 1 for the data gradient: [Cout][9][Cin]).  Same role as the cuDNN
 * WINOGRAD algorithm the reference's nn.Conv2d (model/yolo2.py:57) may pick for fp32 3x3 convolutions: 2.25x fewer
 * multiplications, results within fp32 rounding of the direct sum (tests state the tolerance). */
int y2_wino_weight(const float* w_packed, float* u, int32_t Cout, int32_t Cin, y2_stream_t stream);
/* ... and for Y2_ALGO_WINOGRAD_F43: u6[36][Cout][Cin] = G g G^T (G 6x3, interpolation points 0, 1, -1, 2, -1/2, inf). */
int y2_wino6_weight(const float* w_packed, float* u6, int32_t Cout, int32_t Cin, y2_stream_t stream);

/* Winograd form of y2_conv_wgrad for a 3x3 / stride-1 / same-padding convolution: dw_packed[Cout][9][Cin] = (not +=) the
 * weight gradient; 16 reductions over ceil(H/2)*ceil(W/2) tiles per image instead of 9 over H*W pixels.  Cin, Cout, ldx,
 * ldz multiples of 4; workspace of y2_wino_wgrad_workspace_bytes() bytes (transformed input, transformed gradient, dU). */
long long y2_wino_wgrad_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout);
/* The same for ONE form (native_layout as y2_wino_wgrad_ex takes it; what that entry point requires): the 4x4-tile form needs 36/64 of the 2x2-tile form's rows. */
long long y2_wino_wgrad_workspace_bytes_ex(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t native_layout);
int y2_wino_wgrad(const float* x, const float* dz, float* dw_packed, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t ldx,
                  int32_t Cout, int32_t ldz, const float* v_transformed, float* workspace, long long workspace_bytes, y2_stream_t stream);
/* ... native_layout bit 0: the result is written as dw[Cout][Cin][3][3] - nn.Conv2d.weight.grad's own layout (model/yolo2.py:57), no
 * y2_unpack_weight_grad pass behind it.  Bit 1: Winograd F(3x3, 4x4) - 36 reductions over 4x4 gradient tiles (1.78x fewer multiply-adds than
 * the 2x2 form on even maps); needs x (not v_transformed); its larger transform constants cost accuracy (1.2-1.4e-5 x rms of the gradient in
 * fp32 against 2.7e-6): for weight gradients only.  Bit 2 (with bit 1): `dz` IS the transformed gradient [36][T][Cout] that
 * y2_bn_act_bwd_wino6 wrote (T = y2_wino6_tiles(B, H, W)); ldz is ignored. */
int y2_wino_wgrad_ex(const float* x, const float* dz, float* dw, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t ldx,
                     int32_t Cout, int32_t ldz, const float* v_transformed, float* workspace, long long workspace_bytes, int32_t native_layout,
                     y2_stream_t stream);
/* v_transformed (optional): the transformed input V[16][B*ceil(H/2)*ceil(W/2)][Cin] of the SAME x, as y2_conv_fwd with
 * algo = Y2_ALGO_WINOGRAD leaves it at the start of its workspace when the batch fits one chunk (V + M <= Y2_WINO_CHUNK_MB,
 * default 4096 MB): the training graph keeps that workspace alive and the weight gradient skips the input transform. */

int y2_conv_fwd(const y2_conv_params* p, y2_stream_t stream);

/* Scratch bytes this problem can use (tiles that do not fill the last round of the 256 CUs are split along K into a
 * caller-provided workspace and combined by a fix-up kernel); 0 = none; negative = argument error. */
long long y2_conv_fwd_workspace_bytes(const y2_conv_params* p);

/* The same for `count` convolutions enqueued back to back (one host call for a whole Darknet stage chain;
 * model/yolo2.py:125-130 runs them as separate nn.Module calls). Stops at the first error. */
int y2_conv_fwd_batch(const y2_conv_params* params, int count, y2_stream_t stream);

/* y2_conv_fwd(p) for a raw 3x3 problem (scale == shift == NULL, slope == 1, y given, y_pool NULL) as a producer of z_sel (see y2_bn_act_fwd_sel): the same
 * launch also writes z_sel [B,H/2,W/2,Cout] (pixel stride ldzs) = per 2x2 window the first z_q in scan order that maximises sign(gamma[c]) * z_q (strict
 * comparison, gamma[c] == 0: q = 0; gamma = the BatchNorm weight).  Served only by the fused Winograd kernel of tile 3: p->algo is Y2_ALGO_WINOGRAD_FUSED or
 * Y2_ALGO_WINOGRAD_IMPLICIT with p->tile == 3, H and W even, z_sel 16-byte aligned, ldzs >= Cout a multiple of 4, outputs below 2 GB.  Anything else:
 * Y2_ENOSUP with nothing launched and nothing written (call y2_conv_fwd and y2_bn_act_fwd_sel instead); gamma or z_sel NULL: Y2_EINVAL.  p->stats may be NULL. */
int y2_conv_fwd_sel(const y2_conv_params* p, const float* gamma, float* z_sel, int ldzs, y2_stream_t stream);

/* First layer (model/yolo2.py:78, 'layers1.0'): reads the plugin's NCHW fp32 input [B,Cin<=4,H,W] directly,
 * conv3x3 pad 1 -> affine -> LeakyReLU -> (optional 2x2 max-pool), writes NHWC.
 * w is the UNPACKED state_dict weight [Cout][Cin][3][3]; Cout <= 64.  y (full res, pixel stride ldy) and/or
 * y_pool (pixel stride ldp) may be requested; stats as in y2_conv_params. */
int y2_conv0_fwd(const float* x_nchw, const float* w, const float* scale, const float* shift,
                 float* y, float* y_pool, double* stats,
                 int B, int H, int W, int Cin, int Cout, int ldy, int ldp, float slope, y2_stream_t stream);
/* The training forward of the first layer as a producer of z_sel (see y2_bn_act_fwd_sel): raw z (pixel stride ldz), its statistics, and z_sel
 * [B,H/2,W/2,Cout] (pixel stride ldzs) = per window the first z_q in scan order that maximises sign(gamma[c]) * z_q (strict comparison; gamma = the
 * BatchNorm weight, known before the batch statistics are).  z and stats are those of y2_conv0_fwd(x, w, NULL, NULL, z, NULL, stats, ..., 1.0).
 * gamma, z and z_sel are required (NULL: Y2_EINVAL); stats may be NULL (deterministic mode, where statistics are refused, passes NULL): z and z_sel
 * are then written all the same, for every Cin, Cout and row stride the plain entry accepts. */
int y2_conv0_fwd_sel(const float* x_nchw, const float* w, const float* gamma, float* z, float* z_sel, double* stats,
                     int B, int H, int W, int Cin, int Cout, int ldz, int ldzs, y2_stream_t stream);

/* nn.MaxPool2d(kernel_size=2) (model/yolo2.py:79,86,97) on NHWC; H, W even (16-B vector path when C, ldx, ldy are multiples of 4). */
int y2_maxpool2_fwd(const float* x, float* y, int B, int H, int W, int C, int ldx, int ldy, y2_stream_t stream);

/* General max-pool on NHWC with `pad` rows/cols of -inf before and `pad_end` after each spatial axis:
 * nn.MaxPool2d(3, 2, 1) of model/resnet.py:114 is (3, 2, 1, 1); ConstantPad2d((0,1,0,1), float32.min) + MaxPool2d(2, stride=1)
 * of model/yolo2.py:151-152 (Tiny) is (2, 1, 0, 1).  out = (H + pad + pad_end - k)/stride + 1. */
int y2_maxpool_fwd(const float* x, float* y, int B, int H, int W, int C, int ldx, int ldy, int ksize, int stride, int pad, int pad_end, y2_stream_t stream);

/* Plugin input boundary for backbones whose stem runs through y2_conv_fwd (model/resnet.py:111): NCHW [B,C,H,W] ->
 * NHWC with pixel stride ld >= C, padding channels zero-filled. */
int y2_nchw_to_nhwc(const float* x, float* y, int B, int C, int H, int W, int ld, y2_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Detection head decode: model.Inference.forward after self.dnn(x) (model/__init__.py:120-135),
 * softmax of the class logits (detect.py:152, eval.py:270) and the visibility filter
 * (detect.filter_visible, detect.py:51-63) in one pass over the head image.
 * ------------------------------------------------------------------------------------------------ */
/* feature: [B, cells, A, 5+C] (C may be 0: single class), i.e. the NHWC head image.
 * anchors: [A][2] (height, width) in cell units (utils/__init__.py:78-81).
 * Outputs (any may be NULL): iou [B,cells,A]; center_offset, size_norm, yx_min, yx_max [B,cells,A,2];
 * prob [B,cells,A,C] = softmax(logits); prob_cls [B,cells,A] = max_c prob and cls [B,cells,A] its first arg-max
 * (detect.py:52; 1.0 / 0 when C == 0, detect.py:43-48).  Cell k decodes to (k / rows, k % rows) (model/__init__.py:53-56). */
int y2_decode(const float* feature, const float* anchors, int B, int rows, int cols, int A, int C,
              float* iou, float* center_offset, float* size_norm, float* yx_min, float* yx_max, float* prob,
              float* prob_cls, int32_t* cls, y2_stream_t stream);

/* detect.filter_visible (detect.py:51-63): per image, candidates with score > thr in candidate order, where
 * score = iou*max_c prob (fix != 0, thr = threshold_cls) or iou (fix == 0, thr = threshold).
 * Inputs as produced by y2_decode for one batch: iou [B,n], prob [B,n,C] (C >= 1).
 * Outputs: count[B]; index[B,n] (first count[b] entries = surviving candidate indices, ascending);
 * prob_cls[B,n], cls[B,n] (max prob and its first arg-max for EVERY candidate).
 * If prob == NULL, prob_cls is an INPUT (already computed by y2_decode) and cls is not touched. */
int y2_filter_visible(const float* iou, const float* prob, int B, int n, int C, int fix, float thr,
                      int32_t* count, int32_t* index, float* prob_cls, int32_t* cls, y2_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * IoU: utils.iou.torch (utils/iou/torch.py:24-61, 116-153, 216-233).  Boxes are (y, x) min / max pairs.
 * Bit-exact to the fp32 operation order of the reference (no FMA contraction, IEEE division).
 * ------------------------------------------------------------------------------------------------ */
/* The tail of detect.postprocess after NMS (detect.py:69-79) for a whole batch in one launch: k_* = the surviving boxes of every image
 * (iou, yx_min, yx_max of candidate cand[b][keep[b][k]], k < keep_count[b]; cand NULL: keep holds box indices) and - e_count != NULL,
 * the `[detect] fix` branch (:73-77) - their expansion into detections: every (box, class) pair with iou * prob > threshold_cls in
 * row-major order: e_min / e_max [B][limit*C][2], e_score, e_cls (int64) [B][limit*C], e_count [B]. */
int y2_expand_classes(const float* iou, const float* prob, const float* yx_min, const float* yx_max, const int32_t* cand, const int32_t* keep,
                      const int32_t* keep_count, int32_t B, int32_t n, int32_t C, int32_t limit, float threshold_cls, float* k_iou, float* k_min, float* k_max,
                      float* e_min, float* e_max, float* e_score, long long* e_cls, int32_t* e_count, y2_stream_t stream);

/* eval.matching (eval.py:67-75): best[i], which[i] = max / first arg-max over j of IoU(box1 i, box2 j) (utils/iou/torch.py:47-61 arithmetic). */
int y2_iou_rowmax(const float* yx_min1, const float* yx_max1, const float* yx_min2, const float* yx_max2, int32_t N1, int32_t N2, float min_union,
                  float* best, long long* which, y2_stream_t stream);

/* The matching loop of the VOC evaluation (eval.py:278-292 with filter_valid :140-145, filter_cls_data / filter_cls_pred :148-162, matching and
 * _matching :57-75) for a batch of B images in ONE launch (one workgroup per image) - in place of one y2_iou_rowmax launch, two blocking copies and
 * a host claim loop per (image, predicted class).  A latency kernel: about M x G IoUs per image.
 * Detections (the batch form of detect.postprocess, detect.expand_batch): det_min / det_max [B][M][2] in (y, x) order, det_cls int64 [B][M],
 * det_count [B]: row i of image b takes part iff i < det_count[b] (clamped to [0, M]).  Ground truth padded to G boxes per image: gt_min / gt_max
 * [B][G][2], gt_cls int64 [B][G], gt_difficult uint8 [B][G].  A box is VALID iff ymin < ymax, xmin < xmax and difficult < 1 (zero padding is invalid).
 * cls_num [C] += the number of valid boxes per class (the caller zeroes it; a class id outside [0, C) is not counted).
 * tp [B][M] uint8: every row is written.  A participating row of class c takes the maximum IoU (the y2_iou_rowmax arithmetic: same device function,
 * same min_union clamp) over the valid boxes of class c in array order and its FIRST arg-max; it is positive iff that maximum > threshold (strict,
 * fp32; never without a valid box of its class); tp = positive and no EARLIER participating row of the image (array order - not score order: the
 * reference sorts only at the end, across images) is positive with the same arg-max box.  Integer atomics only: bit-reproducible.
 * M >= 0 unbounded, 0 <= G <= Y2_EVAL_MATCH_MAX_G (the image's labels are staged in LDS, 32 bytes per box; more: Y2_ENOSUP, nothing is written).
 * The det_* / tp pointers may be NULL when M == 0, the gt_* pointers when G == 0. */
#define Y2_EVAL_MATCH_MAX_G 1024
int y2_eval_match(const float* det_min, const float* det_max, const long long* det_cls, const int32_t* det_count,
                  const float* gt_min, const float* gt_max, const long long* gt_cls, const uint8_t* gt_difficult,
                  int32_t B, int32_t M, int32_t G, int32_t C, float threshold, float min_union, uint8_t* tp, int32_t* cls_num, y2_stream_t stream);

/* The collate step of the data pipeline (utils/data.py:114-133: cv2.resize of the cropped, possibly flipped image - transform/resize/label.py:25-74,
 * transform/augmentation.py:88-103 - then BGR2RGB, ToTensor, Normalize) for a ragged batch of uint8 images in ONE launch.
 * src: one packed byte buffer; image b starts at src + offset[b] (any byte alignment), 3 interleaved channels per pixel.
 * geom [B][8] int32: {row_stride_bytes, src_h, src_w, win_y0, win_x0, win_h, win_w, flip}.  The window is in the frame AFTER the optional horizontal
 * flip: with flip set, frame column x is source column src_w - 1 - x.  The whole image without flip is the reference's `rescale`.
 * lut [3][256] fp32, indexed by OUTPUT plane: the whole of ToTensor + Normalize (or any per-level map) as a table; no arithmetic on levels follows
 * the resize.  flags bit 0: output plane c reads source channel 2 - c (BGR2RGB).  out [B][3][H][W] fp32 (what y2_conv0_fwd / y2_nchw_to_nhwc read).
 * Resampling (per axis, window extent s -> output extent d, 8-bit INTER_LINEAR arithmetic): scale = (double)s / d;
 * f = (float)((i + 0.5) * scale - 0.5), k = floor(f), f -= k; horizontally only: k < 0 -> k = 0, f = 0 and k >= s - 1 -> k = s - 1, f = 0; taps
 * clamp(k, 0, s - 1) and clamp(k + 1, 0, s - 1); c1 = rint(f * 2048.f), c0 = rint((1.f - f) * 2048.f).  h = p0 * c0 + p1 * c1 per source row,
 * level = clamp((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2, 0, 255).  When win_h == 2 * H AND win_w == 2 * W the level is the
 * 2x2 box mean (a + b + c + d + 2) >> 2.  Integer after the coefficients: bit-identical on device and host.
 * B == 0: nothing is launched.  W <= Y2_COLLATE_MAX_W (the column taps are staged in LDS; more: Y2_EINVAL).  16-byte stores when W % 4 == 0 and
 * out is 16-byte aligned, 4-byte stores otherwise.  Never allocates, never synchronises.  The tables are DEVICE memory: the device entry point
 * cannot check a window against src_h / src_w (utils.data.to_device and the host function do); it only keeps every tap inside the image the
 * table names. */
#define Y2_COLLATE_MAX_W 4096
int y2_collate_images(const uint8_t* src, const int64_t* offset, const int32_t* geom, const float* lut,
                      int32_t B, int32_t H, int32_t W, int32_t flags, float* out, y2_stream_t stream);

/* The rotation of the data pipeline (transform/augmentation.py:28-75: cv2.warpAffine(image, M, dsize, INTER_LINEAR, BORDER_CONSTANT, fill) with the
 * matrix of cv2.getRotationMatrix2D on a grown canvas) for a ragged batch of uint8 images in ONE launch: the stage in front of y2_collate_images.
 * src / src_offset: as y2_collate_images.  src_geom [B][4] int32: {row_stride_bytes, src_h, src_w, flip}; with flip set, source column x is read at
 * src_w - 1 - x (a flip recorded BEFORE the rotation).  inv [B][6] double: A, the INVERSE map, destination (x, y) -> source
 * (A0 x + A1 y + A2, A3 x + A4 y + A5).  dst / dst_offset / dst_geom [B][8]: the destination images, in the layout of the tables y2_collate_images
 * reads next - columns 0-2 {row_stride_bytes, dst_h, dst_w} are read here, the rest is ignored.  Bytes of a destination row beyond 3 * dst_w are
 * not written.  max_h, max_w: the largest dst_h and dst_w of the batch (the grid; an image larger than that is cut there).
 * fill: the level outside the source, 0xC2C1C0 = one byte per source channel (channel c: fill >> 8c; the reference passes 0).
 * Resampling - cv2.warpAffine for 8-bit 3-channel images, INTER_LINEAR, BORDER_CONSTANT, restated.  For destination pixel (x, y), every double
 * operation rounded separately, lrint = round to nearest even:
 *   adelta = lrint((A0 * x) * 1024), bdelta = lrint((A3 * x) * 1024); X0 = lrint((A1 * y + A2) * 1024) + 16, Y0 = lrint((A4 * y + A5) * 1024) + 16;
 *   X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5 (arithmetic shifts); sx = X >> 5, ax = X & 31, sy = Y >> 5, ay = Y & 31, sx and sy saturated to
 *   [-32768, 32767].  Taps (sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1); a tap outside [0, src_h) x [0, src_w) reads the fill level; with
 *   flip an inside tap reads source column src_w - 1 - sx.  Per channel
 *   level = (p00 (32 - ax)(32 - ay) + p01 ax (32 - ay) + p10 (32 - ax) ay + p11 ax ay + 512) >> 10
 * (OpenCV's 15-bit table form (sum p w + 2^14) >> 15: its bilinear weights are exactly 32 x these products, so the table's sum correction never
 * fires).  Integer after the lrints: bit-identical on device and host.  The identity map is an exact copy.
 * All dimensions in [1, Y2_WARP_MAX_DIM]; |A0|, |A1|, |A3|, |A4| <= 4 and |A2|, |A5| <= 2^19, so every sum above fits int32.  The tables are DEVICE
 * memory: the device entry point cannot check them (utils.data.to_device and the host function do); it rounds through a saturating clamp, forms
 * the sums in 64 bits and reads no tap outside the image the table names.  B == 0: nothing is launched.  12-byte stores (4 pixels) where
 * dst + dst_offset[b] and the row stride are multiples of 4, byte stores otherwise and for the last dst_w % 4 pixels of a row.  Never allocates,
 * never synchronises. */
#define Y2_WARP_MAX_DIM 16384
int y2_warp_affine_images(const uint8_t* src, const int64_t* src_offset, const int32_t* src_geom, const double* inv,
                          uint8_t* dst, const int64_t* dst_offset, const int32_t* dst_geom,
                          int32_t B, int32_t max_h, int32_t max_w, int32_t fill, y2_stream_t stream);

/* The test-time `fixed` resize of the data pipeline (transform/resize/image.py:36-46: cv2.warpAffine(image, [[s, 0, 0], [0, s, 0]], (W, H), flags) -
 * the picture scaled by s into the top-left of a zero canvas, INTER_AREA (which warpAffine runs as INTER_LINEAR) when s < 1, INTER_CUBIC otherwise)
 * fused with BGR2RGB, ToTensor and Normalize, for a ragged batch of uint8 images in ONE launch, IN PLACE of y2_collate_images: packed source images
 * straight to out [B][3][H][W] fp32, no uint8 intermediate.
 * src / offset: as y2_collate_images.  geom [B][4] int32: {row_stride_bytes, src_h, src_w, mode}, mode 0 = linear, 1 = cubic.  inv [B][6] double: A,
 * the INVERSE map, destination (x, y) -> source (A0 x + A1 y + A2, A3 x + A4 y + A5), as y2_warp_affine_images takes it (any affine map is accepted,
 * not only a scale).  lut [3][256] fp32, flags bit 0 (BGR2RGB) and out: as y2_collate_images.  The level outside the source is 0.
 * Coordinates, both modes: those of y2_warp_affine_images above (adelta, bdelta, X0, Y0 with 10 fractional bits, X = (X0 + adelta) >> 5, sx = X >> 5,
 * ax = X & 31, sy and ay alike, sx and sy saturated to [-32768, 32767]).
 * Mode 0: the bilinear level of y2_warp_affine_images with fill 0 and no flip; out[b][c][y][x] = lut[c][that level] of the channel the flag selects -
 * bit for bit what y2_warp_affine_images into an H x W canvas followed by the table gives.
 * Mode 1 - cv2.warpAffine for 8-bit images, INTER_CUBIC, BORDER_CONSTANT 0, restated.  Taps: rows sy - 1 .. sy + 2 x columns sx - 1 .. sx + 2; a tap
 * outside [0, src_h) x [0, src_w) reads 0.  One-dimensional coefficients of a fraction a / 32, fp32, every operation rounded separately, A = -0.75f,
 * t = a * (1.f / 32.f):
 *   c0 = ((A (t + 1) - 5 A)(t + 1) + 8 A)(t + 1) - 4 A;  c1 = ((A + 2) t - (A + 3)) t t + 1;  c2 = ((A + 2)(1 - t) - (A + 3))(1 - t)(1 - t) + 1;
 *   c3 = 1.f - c0 - c1 - c2   (left to right).
 * Weights w[i][j] = saturate_int16(rint((cy[i] * cx[j]) * 32768.f)), i the row and j the column of the tap.  When they do not sum to 32768 the
 * difference d = sum - 32768 is taken out of ONE of the four central weights (i, j in {1, 2}): start with min = max = [1][1], visit [1][1], [1][2],
 * [2][1], [2][2]; an element strictly below the current minimum becomes the minimum, else one strictly above the current maximum becomes the maximum;
 * d < 0: max -= d, d > 0: min -= d (the result is not narrowed to 16 bits again: a = 0 on both axes gives 0, 32768, 0, 0 - the identity map is an
 * exact copy).  Per channel level = clamp((sum of p w + 16384) >> 15, 0, 255) (arithmetic shift).  The weights are computed per pixel by the one
 * function of csrc/fixed.h on device and host: bit-identical.
 * This is OpenCV's recipe restated from its description; agreement with a real cv2.warpAffine is UNVERIFIED (cv2 is not available to the tests).
 * H, W and all source dimensions in [1, Y2_WARP_MAX_DIM]; |A0|, |A1|, |A3|, |A4| <= 4 and |A2|, |A5| <= 2^19.  The tables are DEVICE memory: the
 * device entry point cannot check them (utils.data.to_device and the host function do); it rounds through saturating clamps, forms the sums in 64
 * bits and loads only from positions clamped into the image the table names (the value of a tap outside is dropped).  B == 0: nothing is launched;
 * B > 65535: Y2_ENOSUP.  16-byte stores when W % 4 == 0 and out is 16-byte aligned, 4-byte stores otherwise.  Never allocates, never synchronises. */
int y2_fixed_images(const uint8_t* src, const int64_t* offset, const int32_t* geom, const double* inv, const float* lut,
                    int32_t B, int32_t H, int32_t W, int32_t flags, float* out, y2_stream_t stream);

/* The collate step WITH the colour jitter of the data pipeline (utils/data.py:120-121: resize, then transform_image - transform/image.py: RandomBlur,
 * BGR2HSV, RandomHue / RandomSaturation / RandomBrightness, HSV2RGB, RandomGamma - then ToTensor, Normalize) for a ragged batch in ONE launch, in
 * place of y2_collate_images.  src / offset / geom, B, H, W, flags and out mean exactly what they mean there (so it reads the output of
 * y2_warp_affine_images unchanged).  jitter [B][4] int32: {kx, ky, hsv (0 / 1), 0}.  hsv_tab [B][3][256] uint8: the image's H, S and V tables (may be
 * NULL when no image sets hsv).  lut [B][3][256] fp32: PER IMAGE, indexed by output plane (gamma, ToTensor and Normalize composed by the host).
 * Per output image:
 * (a) Resize: the BGR level of every pixel of the H x W image by the resampling of y2_collate_images above (window, flip, taps, 11-bit coefficients,
 *     the 2x2 box mean at exactly 2:1).
 * (b) Blur - cv2.blur(image, (kx, ky)), restated: a normalised box filter per channel, anchor (kx / 2, ky / 2) in integer division, so the window of
 *     column x is x - kx / 2 .. x - kx / 2 + kx - 1 (rows alike); BORDER_REFLECT_101 on the RESIZED image's coordinates, borderInterpolate's loop:
 *     p < 0 -> -p, p >= n -> 2 n - 2 - p, repeated until 0 <= p < n, and n == 1 -> 0.  s = the integer sum of the kx * ky window;
 *     level = clamp(rint((double)s * (1.0 / (double)(kx * ky))), 0, 255), rint = round half to even (the ColumnSum<int, uchar> path).
 *     1 <= kx, ky <= Y2_JITTER_MAX_BLUR; kx == ky == 1 gives the level back untouched.
 * (c) Colour.  hsv == 0: output plane c takes source channel 2 - c with flags bit 0 (BGR2RGB), else channel c.  hsv == 1: 8-bit COLOR_BGR2HSV, the
 *     three tables applied to H, S and V, 8-bit COLOR_HSV2RGB; the planes are R, G, B whatever flags says.
 *     BGR2HSV, restated (integers, arithmetic right shifts, cvRound = round half to even): sdiv[i] = cvRound((255 << 12) / (1.0 * i)),
 *     hdiv[i] = cvRound((180 << 12) / (6.0 * i)), [0] = 0 in both; v = max(b, g, r), vmin = min(b, g, r), diff = v - vmin;
 *     s = (diff * sdiv[v] + 2048) >> 12; h = (v == r) ? g - b : (v == g) ? b - r + 2 * diff : r - g + 4 * diff; h = (h * hdiv[diff] + 2048) >> 12;
 *     if h < 0, h += 180; all three saturated to 0 .. 255.
 *     HSV2RGB, restated (fp32, every operation rounded separately, + - x and floorf only): hf = (float)h, sf = s * (1.f / 255.f),
 *     vf = v * (1.f / 255.f).  s == 0: r = g = b = vf.  Otherwise hf *= (6.f / 180.f); while hf >= 6, hf -= 6; sector = (int)floorf(hf), hf -= sector;
 *     a sector outside 0 .. 5 -> sector = 0, hf = 0; tab = {vf, vf * (1 - sf), vf * (1 - sf * hf), vf * (1 - sf * (1 - hf))};
 *     (b, g, r) = tab[{1,3,0}, {1,0,2}, {3,0,1}, {0,2,1}, {0,1,3}, {2,1,0}][sector].  Each output is clamp(cvRound(x * 255.f), 0, 255).
 * (d) out[b][c][y][x] = lut[b][c][level of plane c].
 * The recipes of (b) and (c) are restated from memory: agreement with a real cv2.blur / cv2.cvtColor is UNVERIFIED (OpenCV is not available where
 * this was written); what is tested is that device, host and an independent numpy restatement agree bit for bit, that the conversions are within
 * one level of the textbook HSV formulas in fp64, and that the blur is the fp64 box mean over reflect-101 padding.
 * Integer arithmetic, one fp64 product and exactly rounded fp32 operations: bit-identical on device and host.
 * B == 0: nothing is launched.  B > 65535: Y2_ENOSUP.  W > Y2_COLLATE_MAX_W: Y2_EINVAL.  16-byte stores when W % 4 == 0 and out is 16-byte aligned,
 * 4-byte stores otherwise.  Never allocates, never synchronises.  The tables are DEVICE memory: the device entry point cannot refuse a window
 * outside its image, a blur size outside 1 .. Y2_JITTER_MAX_BLUR or hsv without hsv_tab (utils.data.to_device and the host function do: Y2_EINVAL);
 * it keeps every tap inside the image the table names, brings a blur size into that range and takes the plain path when hsv_tab is NULL. */
#define Y2_JITTER_MAX_BLUR 7
int y2_collate_jitter_images(const uint8_t* src, const int64_t* offset, const int32_t* geom, const int32_t* jitter, const uint8_t* hsv_tab,
                             const float* lut, int32_t B, int32_t H, int32_t W, int32_t flags, float* out, y2_stream_t stream);

/* Baseline JPEG decoding of the data pipeline (utils/data.py:77: cv2.imread, whose decoder is libjpeg-turbo) for a ragged batch on the device: the
 * stage in front of y2_warp_affine_images / y2_collate_images / y2_collate_jitter_images (csrc/jpeg.hip; the decoder is csrc/jpeg.h, shared with the
 * host function).  A worker parses the headers of a file with y2_jpeg_probe_host and ships the file's bytes and the descriptor record.
 * Supported: baseline sequential DCT (SOF0), 8-bit, Huffman; ONE scan holding every component; three components Y Cb Cr with chroma sampled 1 x 1 and
 * luma 1 x 1, 2 x 1 or 2 x 2, or one component (written to all three channels); restart intervals; up to four 8-bit quantisation tables, two DC and
 * two AC Huffman tables; sides of 1 .. Y2_JPEG_MAX_DIM.  Everything else - progressive, extended, arithmetic, lossless, 12-bit, 16-bit quantisation
 * tables, Huffman table ids 2 / 3, more than one scan, other sampling, four components, RGB (an Adobe APP14 marker with transform 0 on three
 * components, or components named 'R' 'G' 'B' without a JFIF marker), DNL, an Exif orientation (tag 0x0112 of IFD0) of 2 .. 8, which cv2.imread would
 * apply - is Y2_ENOSUP from the probe: no error, the caller decodes that file on the host.
 *
 * The recipe - libjpeg-turbo's defaults (JDCT_ISLOW, fancy upsampling), restated.  VERIFIED bit for bit against Pillow's libjpeg-turbo on the
 * fixtures of tests/golden/jpeg (tools/make_golden_jpeg.py); agreement with cv2.imread itself is unverified (OpenCV was not available).
 * (a) Entropy decoding.  Canonical Huffman codes from the DHT counts and symbols.  Bytes FF 00 are one data byte FF.  Per block: a DC symbol t, t extra
 *     bits, diff = extend(bits, t), DC = prediction + diff per component (prediction 0 at the scan start and behind every restart marker); then AC
 *     symbols rs at zigzag position k = 1 ..: r = rs >> 4, n = rs & 15; n > 0: k += r, coefficient k = extend(n bits, n), k += 1; n == 0, r == 15
 *     (ZRL): k += 16; n == 0 otherwise (EOB): the block ends.  extend(v, n) = v < 2^(n-1) ? v - 2^n + 1 : v.  With a restart interval of R MCUs,
 *     behind every R MCUs less than 8 unread bits are dropped and the next two bytes must be FF D0+m (m counts the markers modulo 8).
 * (b) Dequantisation and IDCT.  coefficient x table entry in 32-bit integers; jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2, the constants
 *     2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172, a column pass descaled by 11 then a row pass descaled by 18 (descale(x, n) =
 *     (x + 2^(n-1)) >> n, arithmetic), + 128, clamped to 0 .. 255.  (libjpeg's all-zero-AC shortcuts give the same values and are not taken; its
 *     range-limit table wraps beyond +-512 where this clamps: outside what a valid stream produces.)  The arithmetic wraps modulo 2^32 instead of
 *     overflowing.
 * (c) Chroma upsampling, on the component's downsampled size cw x ch = ceil(size * samp / max_samp), not the block-padded one.  cw <= 2: replication.
 *     Otherwise 2 x 1: out[2i] = (3 in[i] + in[i-1] + 1) >> 2, out[2i+1] = (3 in[i] + in[i+1] + 2) >> 2, the first and last output samples of a row
 *     copies;  2 x 2: per output row s[i] = 3 near[i] + far[i] (far = the row above for the upper output row, below for the lower; beyond the first /
 *     last real row: that row itself), out[2i] = (3 s[i] + s[i-1] + 8) >> 4, out[2i+1] = (3 s[i] + s[i+1] + 7) >> 4, first column
 *     (4 s[0] + 8) >> 4, last column (4 s[cw-1] + 7) >> 4.
 * (d) Colour: x = level - 128; R = clamp(Y + ((91881 x_cr + 32768) >> 16)), B = clamp(Y + ((116130 x_cb + 32768) >> 16)),
 *     G = clamp(Y + ((-22554 x_cb - 46802 x_cr + 32768) >> 16)), arithmetic shifts; bytes are stored B, G, R (cv2.imread's order).
 *
 * y2_jpeg_probe_host(data, nbytes, desc): HOST function.  Parses the markers of one file and fills the descriptor record desc
 * [Y2_JPEG_DESC_BYTES] (zeroed when the file is refused).  Its first eight int32 are {height, width, components, luma h sampling, luma v sampling,
 * restart interval, byte offset of the entropy-coded segment in the file, its length up to the first marker that is no RSTn}; behind them the table
 * selectors, the quantisation tables and the Huffman tables in decoding form (csrc/jpeg.h: JpDesc).  0, Y2_ENOSUP (above) or Y2_EINVAL: no SOI,
 * a segment length past the end, table ids or sampling factors out of range, zero dimensions, Huffman counts that over-subscribe the code space, a
 * scan that names an undefined table, scan parameters other than 0 / 63 / 0.  Never reads outside [data, data + nbytes).
 * y2_jpeg_workspace_bytes(desc, B): HOST function; desc [B] records in host memory.  The scratch a batch needs: B times the largest image's
 * coefficient blocks (int16, in decoding order) and block-padded component planes (uint8), 3 bytes per padded component sample (4.5 per pixel at 4:2:0); Y2_EINVAL for a
 * record that is none.
 * y2_jpeg_decode_images: src: the packed file bytes, src_bytes long; file b starts at src + src_offset[b].  desc [B] records (4-byte aligned).
 * dst / dst_offset / dst_geom [B][8]: the tables y2_collate_images and y2_warp_affine_images read next; columns 0-2 {row_stride_bytes, h, w} are
 * read here and must be the descriptor's size; bytes of a row beyond 3 * w are not written.  ws: ws_bytes of scratch, 16-byte aligned; image b owns
 * [b * p, (b + 1) * p), p = (ws_bytes / B) rounded down to 16.  status [B] int32, written on the device: 0 decoded; 1 bits were needed beyond the end
 * of the segment; 2 no restart marker where an interval ends; 3 no such Huffman code, or a run past coefficient 63; 4 whole bytes left behind the last
 * MCU - in these four cases the image holds what decoding zero bits from that point on yields (deterministic, the same on device and host);
 * 5 the record is none, disagrees with dst_geom, or the image's source, destination or scratch lies outside src_bytes / dst_bytes / p: nothing is
 * written for that image.  The other images of the batch are not affected.
 * SAFETY, for ANY bytes in src and ANY contents of desc, src_offset, dst_offset and dst_geom: the device reads only inside [src, src + src_bytes) and
 * the tables, writes only inside [dst, dst + dst_bytes), [ws, ws + ws_bytes) and status, and takes a bounded number of steps.  Every geometry value
 * is derived in one place from range-checked descriptor fields (jp_layout) and checked against the three extents before an image is touched; a
 * table selector is range-checked; a Huffman symbol's run cannot move past coefficient 63; a symbol index is masked to the table; a block takes at
 * most 64 symbols and the block count comes from the checked size; reads past the segment's end yield zero bits.
 * Three launches (entropy decoding: one workgroup per image; IDCT; upsampling + colour + store with 12-byte stores where dst + dst_offset[b] and
 * the row stride are multiples of 4).  B == 0: nothing is launched.  B > 65535: Y2_ENOSUP.  Never allocates, never synchronises. */
#define Y2_JPEG_MAX_DIM 16384
#define Y2_JPEG_DESC_BYTES 4096
int y2_jpeg_decode_images(const uint8_t* src, int64_t src_bytes, const int64_t* src_offset, const uint8_t* desc,
                          uint8_t* dst, int64_t dst_bytes, const int64_t* dst_offset, const int32_t* dst_geom,
                          uint8_t* ws, int64_t ws_bytes, int32_t* status, int32_t B, y2_stream_t stream);

/* Choosing a dataset's anchors (dimension_cluster.py): k-means on the distance 1 - IoU over box sizes, R restarts ("trials") in one launch, one
 * workgroup per trial (csrc/kmeans.hip; the arithmetic is csrc/kmeans.h, shared with the host functions).  The reference runs
 * nltk.cluster.kmeans.KMeansClusterer with distance(a, b) = 1 - utils.iou.numpy.iou(-a, a, -b, b) on float64 data.  nltk was not available: the
 * algorithm below is KMeansClusterer RESTATED FROM MEMORY, agreement with a real nltk run is UNVERIFIED, and this text is the contract.
 * All arithmetic is fp64, one rounding per operation (-ffp-contract=off).  size [N][2]: (height, width) per box, like yx - the half-extents a of a box
 * centred on the origin.
 * (a) IoU, in the operation order of utils/iou/numpy.py:iou with its default `min`: ih = 2 min(a.h, b.h), iw = 2 min(a.w, b.w) (the difference
 *     min(a, b) - max(-a, -b) is exactly that); inter = ih iw; area1 = (2 a.h)(2 a.w), area2 likewise; union = max((area1 + area2) - inter,
 *     DBL_EPSILON); iou = inter / union; dist = 1 - iou.  min and max are numpy's: a NaN operand is the result.
 * (b) Classification (classify_vectorspace): best = dist(x, mean[0]) unconditionally; mean k = 1 .. K-1 replaces it only when dist < best (strict):
 *     ties and NaN stay with the lower index.
 * (c) Centroid.  nltk adds a cluster's members one after the other, which no parallel reduction reproduces, so the order is fixed HERE, independently
 *     of how a kernel is launched: per cluster and component 256 lane partials, each starting at +0.0 and adding the members i = l (mod 256) in
 *     increasing i; then the tree for s = 128, 64 .. 1: p[l] += p[l + s] for l < s; centroid = p[0] / (double)count.  (Adding +0.0 for a non-member
 *     is bit-identical to skipping it.)
 * (d) One iteration (_cluster_vectorspace): classify all N boxes; if a cluster is empty the trial ends with status 1 (the reference aborts on an
 *     assertion there) and the means stay those the iteration started from; otherwise the new means, difference = sum_k dist(old_k, new_k) added in
 *     increasing k from 0.0, the means become the new means, and the trial has converged when difference < conv_test (the reference: 1e-6).
 * (e) max_iter iterations without convergence: status 2 (nltk has no limit).  K >= N: no iteration runs (nltk's num_means < len(vectors) guard), the
 *     initial means are the result, iters 0, status 0.
 * (f) Initial means of trial r: size[init[r][k]].  An index outside [0, N) is never dereferenced: the trial ends with status 3 and zeroed outputs.
 * (g) Final pass: one more classification against the final means gives counts [K] and cost = sum of dist in the lane / tree order of (c); the mean
 *     IoU of the anchors is 1 - cost / N.
 * iters[r]: the iterations that replaced the means (the one that found an empty cluster is not counted).
 * Y2_EINVAL: N, K, R or max_iter <= 0, a null pointer.  Y2_ENOSUP: K > Y2_KMEANS_MAX_K (the paper explores up to 15; YOLOv2 uses 5, its successors
 * 9), R > 65535.  Y2_EALIGN: size, means or cost not 8-byte aligned.  One launch; never allocates, never synchronises.
 * SAFETY for ANY values in size and init: a box index is a loop counter, an initial index is range-checked, a winner is an integer in [0, K).  The
 * Python layer rejects NaN, zero and negative sizes and out-of-range indices before they reach the library.
 * y2_anchor_assign: classification (b) of N boxes against arbitrary means [K][2] (device memory): index [N] int32 and / or iou [N] double (the IoU
 * with the winning mean), either may be NULL.  A grid-stride kernel. */
#define Y2_KMEANS_MAX_K 16
int y2_anchor_kmeans(const double* size, int32_t N, int32_t K, const int32_t* init, int32_t R, int32_t max_iter, double conv_test,
                     double* means, int32_t* iters, int32_t* status, double* cost, int32_t* counts, y2_stream_t stream);
int y2_anchor_assign(const double* size, int32_t N, const double* means, int32_t K, int32_t* index, double* iou, y2_stream_t stream);

/* batch_iou_matrix: [Bt,N1,2]x2, [Bt,N2,2]x2 -> out [Bt,N1,N2]; iou_matrix is Bt = 1.  min_union = eps32.
 * mode 0: IoU (utils/iou/torch.py:47-61, 139-153);  mode 1: intersection area only (:24-44, 116-136). */
int y2_iou_matrix(const float* yx_min1, const float* yx_max1, const float* yx_min2, const float* yx_max2,
                  int Bt, int N1, int N2, float min_union, int mode, float* out, y2_stream_t stream);
/* batch_iou_pair: [n,2]x4 -> out [n]. */
int y2_iou_pair(const float* yx_min1, const float* yx_max1, const float* yx_min2, const float* yx_max2,
                int n, float min_union, float* out, y2_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * NMS: utils.postprocess.nms (utils/postprocess.py:23-49): class-agnostic greedy NMS on `score`,
 * top-`limit` after a descending sort, keep j iff IoU(head, j) <= overlap.  Batched: image b owns
 * candidates [b*stride, b*stride + n[b]); with cand != NULL (the index list of y2_filter_visible) candidate i of
 * image b is element cand[b*stride + i] of the image's score/box rows (no gather pass).  Ties: lower index first.
 * keep [B, limit] receives, in descending-score order, indices RELATIVE to the image's first candidate;
 * keep_count[B] their number.  limit <= 1024.  One workgroup per image.  order_ws: [B, limit] int32 workspace
 * (receives the top-`limit` candidate indices in descending-score order).
 * ------------------------------------------------------------------------------------------------ */
int y2_nms(const float* score, const float* yx_min, const float* yx_max, const int32_t* cand, const int32_t* n, int B, int stride,
           float overlap, int limit, int32_t* order_ws, int32_t* keep, int32_t* keep_count, y2_stream_t stream);

/* HOST-memory forms of the same algorithms (all pointers are HOST pointers, no stream, no HIP call: safe in a forked child).
 * utils.postprocess.nms is called on CPU tensors by the reference's summary worker (train.py:209) and the utils.iou.torch unit
 * tests run on CPU tensors (utils/iou/torch.py:64-113).  Same ordering rule (score descending, ties -> lower index, NaN last),
 * same fp32 IoU operation sequence: keep lists and IoU values are bit-identical to the device entry points. */
int y2_nms_host(const float* score, const float* yx_min, const float* yx_max, const int32_t* cand, const int32_t* n, int B, int stride,
                float overlap, int limit, int32_t* keep, int32_t* keep_count);
int y2_iou_matrix_host(const float* yx_min1, const float* yx_max1, const float* yx_min2, const float* yx_max2,
                       int Bt, int N1, int N2, float min_union, int mode, float* out);
int y2_iou_pair_host(const float* yx_min1, const float* yx_max1, const float* yx_min2, const float* yx_max2,
                     int n, float min_union, float* out);
/* y2_eval_match on host memory (eval.match_batch on CPU tensors): the same semantics, the same fp32 IoU sequence, the same G cap - tp and
 * cls_num are bit-identical to the device entry point. */
int y2_eval_match_host(const float* det_min, const float* det_max, const long long* det_cls, const int32_t* det_count,
                       const float* gt_min, const float* gt_max, const long long* gt_cls, const uint8_t* gt_difficult,
                       int32_t B, int32_t M, int32_t G, int32_t C, float threshold, float min_union, uint8_t* tp, int32_t* cls_num);
/* y2_collate_images on host memory (utils.data.to_device on 'cpu'): the same arithmetic, bit-identical output.  The tables are checked first
 * (offset >= 0, row_stride_bytes >= 3 * src_w, the window inside the image, flip 0 or 1): Y2_EINVAL, nothing is written. */
int y2_collate_images_host(const uint8_t* src, const int64_t* offset, const int32_t* geom, const float* lut,
                           int32_t B, int32_t H, int32_t W, int32_t flags, float* out);
/* y2_warp_affine_images on host memory: the same arithmetic, bit-identical output.  The tables are checked first (offsets >= 0, source dimensions
 * in [1, Y2_WARP_MAX_DIM], dst_h <= max_h, dst_w <= max_w, row strides >= 3 * width, flip 0 or 1, the ranges of A above): Y2_EINVAL, nothing is
 * written. */
int y2_warp_affine_images_host(const uint8_t* src, const int64_t* src_offset, const int32_t* src_geom, const double* inv,
                               uint8_t* dst, const int64_t* dst_offset, const int32_t* dst_geom,
                               int32_t B, int32_t max_h, int32_t max_w, int32_t fill);
/* y2_fixed_images on host memory (utils.data.to_device on 'cpu'): the same arithmetic, bit-identical output.  The tables are checked first
 * (offset >= 0, source dimensions in [1, Y2_WARP_MAX_DIM], row_stride_bytes >= 3 * src_w, mode 0 or 1, the ranges of A above; a NaN is out of
 * range): Y2_EINVAL, nothing is written. */
int y2_fixed_images_host(const uint8_t* src, const int64_t* offset, const int32_t* geom, const double* inv, const float* lut,
                         int32_t B, int32_t H, int32_t W, int32_t flags, float* out);
/* y2_collate_jitter_images on host memory (utils.data.to_device on 'cpu'): the same arithmetic, bit-identical output.  The tables are checked first
 * (those of y2_collate_images_host; kx and ky in 1 .. Y2_JITTER_MAX_BLUR, hsv 0 or 1, jitter[b][3] == 0, hsv_tab present when an image sets hsv):
 * Y2_EINVAL, nothing is written. */
int y2_collate_jitter_images_host(const uint8_t* src, const int64_t* offset, const int32_t* geom, const int32_t* jitter, const uint8_t* hsv_tab,
                                  const float* lut, int32_t B, int32_t H, int32_t W, int32_t flags, float* out);
/* The JPEG functions that run on the host (see y2_jpeg_decode_images).  y2_jpeg_decode_images_host: the same arguments as host pointers, the same
 * bytes and the same status 0 .. 4.  The tables are checked first: an image that the device would give status 5 is Y2_EINVAL here, nothing is
 * written. */
int y2_jpeg_probe_host(const uint8_t* data, int64_t nbytes, uint8_t* desc);
long long y2_jpeg_workspace_bytes(const uint8_t* desc, int32_t B);
int y2_jpeg_decode_images_host(const uint8_t* src, int64_t src_bytes, const int64_t* src_offset, const uint8_t* desc,
                               uint8_t* dst, int64_t dst_bytes, const int64_t* dst_offset, const int32_t* dst_geom,
                               uint8_t* ws, int64_t ws_bytes, int32_t* status, int32_t B);
/* y2_anchor_kmeans / y2_anchor_assign on host memory (dimension_cluster.cluster on CPU data): the same functions of csrc/kmeans.h, the trials one
 * after the other on the calling thread; every output is bit-identical to the device entry point. */
int y2_anchor_kmeans_host(const double* size, int32_t N, int32_t K, const int32_t* init, int32_t R, int32_t max_iter, double conv_test,
                          double* means, int32_t* iters, int32_t* status, double* cost, int32_t* counts);
int y2_anchor_assign_host(const double* size, int32_t N, const double* means, int32_t K, int32_t* index, double* iou);

/* ------------------------------------------------------------------------------------------------
 * Deterministic mode (opt-in, process-global; one process per GPU, one stream).  By default the split-K weight gradient, the
 * BatchNorm-backward sums, the BatchNorm statistics and the loss sums combine partial results with atomics, in completion order:
 * run-to-run differences of ~1e-6 relative.  y2_set_deterministic(1, ws, bytes) makes y2_conv_wgrad / _ex / y2_wino_wgrad /
 * y2_conv0_wgrad / y2_bn_act_bwd / _ex / y2_region_loss_fwd write their partials into the scratch area `ws` (device memory, 16-B
 * aligned, >= 1 MiB; 256 MiB covers Darknet-19 at batch 64; a call that needs more returns Y2_EINVAL) and add them in a fixed
 * tree.  y2_conv_fwd / y2_conv0_fwd then refuse `stats` (Y2_ENOSUP): the forward statistics are taken by y2_colstats_det over the
 * raw convolution output z [M, C] (row stride ld): stats = [sum z | sum z^2] in fp64, written (not added) to stats[0 .. 2C) -
 * copy 0 of the Y2_STATS_REPL layout y2_bn_finalize reads (the caller keeps the other copies zero).  `workspace` of
 * y2_colstats_det: min(1024, ceil(M / 256)) * 2 * C doubles.  NOT covered: y2_opt_grad_sumsq (gradient-norm clipping) and y2_colsum.
 * ------------------------------------------------------------------------------------------------ */
int y2_set_deterministic(int on, float* workspace, long long workspace_bytes);
int y2_get_deterministic(void);
int y2_colstats_det(const float* z, long long M, int32_t C, int32_t ld, double* stats, float* workspace, long long workspace_bytes, y2_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Measurement hooks (bench.py, tools/): y2_prof_enable(1) clears the record table and starts bracketing EVERY kernel launch of
 * this library with a HIP event pair on the launch stream; y2_prof_enable(0) stops.  Record i = (kernel name, milliseconds
 * between its two events, multiply-add FLOPs the launch executes: 2*M*N*K of the GEMM it runs, 0 for non-GEMM kernels).
 * y2_prof_get synchronises that record's end event.  Not for use during hipGraph capture.  Process-global tooling state
 * (the only host state of the library besides per-device attribute caches); one process per GPU.
 * ------------------------------------------------------------------------------------------------ */
int y2_prof_enable(int on);
int y2_prof_count(void);
int y2_prof_get(int i, char* name, int name_cap, float* ms, double* flops);
/* Caller-defined non-negative tag stamped on every record made until the next call (e.g. the layer being executed), and its readback. */
int y2_prof_set_tag(int tag);
int y2_prof_get_tag(int i);

/* ------------------------------------------------------------------------------------------------
 * Training path.  The reference trains through torch autograd (train.py:344-357): conv / BN / LeakyReLU /
 * MaxPool backward are PyTorch's; the kernels below are their MI355X-native equivalents, orchestrated by
 * yolo2-pytorch_amd/model/train_graph.py behind the same Python surface (Darknet.forward, model.loss).
 * ------------------------------------------------------------------------------------------------ */

/* Weight gradient of a stride-1 "same" conv (autograd of nn.Conv2d, model/yolo2.py:57):
 * dw[co][tap][ci] = sum_pixels dz[pixel][co] * x[pixel + tap][ci], written in the PACKED layout [Cout][k*k][Cin]
 * (y2_unpack_weight_grad converts to [Cout,Cin,k,k]).  dw must be zero-filled (split-K partials are added atomically).
 * Requires Cin, ldx, Cout, ldz multiples of 4 and 16-B aligned bases (else Y2_EALIGN). */
int y2_conv_wgrad(const float* x, const float* dz, float* dw, int B, int H, int W, int Cin, int ldx, int Cout, int ldz,
                  int ksize, y2_stream_t stream);

/* The same for any kernel size <= 7, stride and padding (model/resnet.py:31,71,79,111): x [B,Hi,Wi,Cin] is the conv INPUT, dz the
 * gradient of its output [B,(Hi+2p-k)/s+1,(Wi+2p-k)/s+1,Cout]. */
int y2_conv_wgrad_ex(const float* x, const float* dz, float* dw, int B, int Hi, int Wi, int Cin, int ldx, int Cout, int ldz,
                     int ksize, int stride, int pad, y2_stream_t stream);

/* Weight gradient of the first layer (model/yolo2.py:78): x is the plugin's NCHW input [B,Cin<=3,H,W], dz NHWC with pixel
 * stride ldz, Cout <= 64.  dw is the state_dict layout [Cout][Cin][3][3], pre-zeroed (partials are added atomically). */
int y2_conv0_wgrad(const float* x_nchw, const float* dz, float* dw, int B, int H, int W, int Cin, int Cout, int ldz, y2_stream_t stream);

/* The first layer's weight gradient WITHOUT a materialised dz (model/yolo2.py:78-79: Conv2d(3, 32) + MaxPool2d(2)): the BatchNorm / LeakyReLU /
 * max-pool backward of y2_bn_act_bwd's second pass runs in this kernel's loader from (z, dy_pool) and the pass-1 sums (call y2_bn_act_bwd
 * with dz = NULL first: it then computes only `sums`).  Same arguments as y2_bn_act_bwd / y2_conv0_wgrad; H, W even; dw pre-zeroed. */
int y2_conv0_wgrad_fused(const float* x_nchw, const float* z, const float* scale, const float* shift, const float* mean, const float* invstd,
                         const float* gamma, float slope, const float* dy_pool, int32_t ldp, const double* sums, float* dw,
                         int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ldz, int32_t has_bn, y2_stream_t stream);

/* Training-mode nn.BatchNorm2d(momentum 0.01, eps 1e-5) statistics (model/yolo2.py:58): stats = Y2_STATS_REPL copies of
 * [sum z | sum z^2] per channel (fp64, accumulated by y2_conv_fwd / y2_conv0_fwd), count = B*H*W.  Writes the affine (scale, shift) used for
 * normalisation (biased variance), saves mean / invstd for backward and updates the running statistics in place
 * (unbiased variance) when running_mean != NULL; num_batches_tracked (int64 scalar in device memory, may be NULL) is the module's
 * step counter, incremented by one (torch/nn/modules/batchnorm.py, as called at model/yolo2.py:58). */
int y2_bn_finalize(const double* stats, double count, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, float momentum, float eps,
                   float* scale, float* shift, float* mean, float* invstd, int C, long long* num_batches_tracked, y2_stream_t stream);

/* y = LeakyReLU(z*scale + shift) on NHWC (scale/shift NULL = identity), optionally with the following MaxPool2d(2)
 * (y_pool) and/or the reorg/concat output addressing of y2_conv_params (out_mode, ldy, coff). */
int y2_bn_act_fwd(const float* z, const float* scale, const float* shift, float slope, float* y, float* y_pool,
                  int B, int H, int W, int C, int ldz, int ldy, int coff, int ldp, int poff, int out_mode, y2_stream_t stream);

/* Backward of (BN train) -> LeakyReLU -> [MaxPool2d(2)]: from dy_full (gradient of the full-resolution activation;
 * fmode 1: stored reorg'ed in a [B,H/2,W/2,ldf] buffer at channel foff) and/or dy_pool (gradient of the pooled
 * activation, routed to the first maximal window element like nn.MaxPool2d) to dz (gradient of the raw conv output).
 * sums [2C] (pre-zeroed fp64) receives sum(g) = d beta (or d bias) and sum(g*zhat) = d gamma.  has_bn = 0: plain
 * bias + LeakyReLU block (dz = g); dz = NULL: only the sums (pass 1; see y2_conv0_wgrad_fused); has_bn = 2: BatchNorm with FROZEN statistics (eval()-mode module with autograd recording,
 * receptive_field_analyzer.py:67,87): mean / invstd are the running statistics, dz = g * gamma * invstd. */
int y2_bn_act_bwd(const float* z, const float* scale, const float* shift, const float* mean, const float* invstd, const float* gamma,
                  float slope, const float* dy_full, int ldf, int foff, int fmode, const float* dy_pool, int ldp, int poff,
                  double* sums, float* dz, int ldd, int B, int H, int W, int C, int ldz, int has_bn, y2_stream_t stream);

/* Extended forms for residual networks (model/resnet.py:29-104): `residual` (pixel stride ldr) is added before the
 * activation in the forward; the backward takes an optional second full-resolution gradient source dy_full2 (fan-out),
 * uses the residual to rebuild the activation mask and can emit dres = gradient w.r.t. the residual input.
 * Aliasing: dz may be one of the gradient inputs (the op is element-wise); a dense dz (ldd == C) that overlaps NO input
 * additionally serves as scratch for the per-workgroup partial sums of pass 1 (an overlapping dz falls back to atomics). */
int y2_bn_act_fwd_ex(const float* z, const float* scale, const float* shift, float slope, const float* residual, int ldr, float* y, float* y_pool,
                     int B, int H, int W, int C, int ldz, int ldy, int coff, int ldp, int poff, int out_mode, y2_stream_t stream);
int y2_bn_act_bwd_ex(const float* z, const float* scale, const float* shift, const float* mean, const float* invstd, const float* gamma,
                     float slope, const float* dy_full, int ldf, int foff, int fmode, const float* dy_pool, int ldp, int poff,
                     const float* dy_full2, int ld2, const float* residual, int ldr, float* dres, int lddr,
                     double* sums, float* dz, int ldd, int B, int H, int W, int C, int ldz, int has_bn, y2_stream_t stream);

/* Pooled blocks without a full-resolution consumer (conv -> BatchNorm(batch statistics) -> LeakyReLU -> MaxPool2d(2), model/yolo2.py:78-96): the
 * quarter-resolution companion z_sel [B,H/2,W/2,C] (pixel stride ldzs) holds, per window and channel, the pre-activation z of the element the pool
 * selects: with s = sign(gamma[c]) the FIRST q in scan order that maximises s*z_q (strict comparison; s = 0: q = 0).  The activation is monotone in z,
 * so LeakyReLU(z_sel*scale + shift) IS the pooled activation, bit for bit (y2_bn_act_fwd over z_sel as an un-pooled [B,H/2,W/2,C] map), and the pooled
 * gradient is non-zero at that element only, so the backward's sums need no other z.
 * y2_bn_act_fwd_sel: y2_bn_act_fwd's pooled form (y = NULL) that also writes z_sel = z at the window's first maximal ACTIVATION (exactly the element
 * y2_bn_act_bwd routes the gradient to; it differs from the definition above only where two different z round to one activation).
 * y2_bn_act_bwd_sel: y2_bn_act_bwd for dy_pool only and has_bn = 1 whose pass 1 (sums) reads (z_sel, dy_pool) - a quarter of z - while pass 2 (dz, NULL:
 * sums only) reads the full z as before. */
int y2_bn_act_fwd_sel(const float* z, const float* scale, const float* shift, float slope, float* y_pool, float* z_sel,
                      int B, int H, int W, int C, int ldz, int ldp, int poff, int ldzs, y2_stream_t stream);
int y2_bn_act_bwd_sel(const float* z, const float* z_sel, int ldzs, const float* scale, const float* shift, const float* mean, const float* invstd,
                      const float* gamma, float slope, const float* dy_pool, int ldp, int poff, double* sums, float* dz, int ldd,
                      int B, int H, int W, int C, int ldz, y2_stream_t stream);

/* Tile count T of the 4x4-tile Winograd forms for a batch of B maps of H x W (per-image grid, or the batch mosaic where that is smaller: csrc/common.h,
 * Wino6Grid) - the row count of the transformed operands [36][T][C] of Y2_ALGO_WINOGRAD_F43(_PRE) / y2_wino_wgrad_ex (bits 1, 2). */
long long y2_wino6_tiles(int32_t B, int32_t H, int32_t W);
/* y2_bn_act_bwd for a block whose gradient dz is consumed ONLY through the two 4x4-tile Winograd transforms (autograd of conv -> BatchNorm(batch
 * statistics) -> LeakyReLU, model/yolo2.py:57-65, in front of a 3x3 convolution whose weight gradient runs F(3x3,4x4) and whose data gradient runs
 * F(4x4,3x3)): pass 1 (sums [2C], pre-zeroed) as y2_bn_act_bwd, then ONE kernel forms dz per pixel and stores v6 = B^T dz B [36][T][C] (the operand of
 * Y2_ALGO_WINOGRAD_F43_PRE) and / or m6 = G dz G^T [36][T][C] (the operand of y2_wino_wgrad_ex bit 2) - bit-identical to y2_bn_act_bwd followed by the
 * transform kernels of those two entry points, without the dz tensor (written once, read twice) and two launches.  Un-pooled gradient source with plain
 * addressing only (dy_full, pixel stride ldf, channel offset foff).  dz: optional plain gradient [B,H,W,C] (pixel stride ldd) for a third consumer, or NULL.
 * The buffer of v6 (else m6) is scratch for pass 1 before it is written.  Not available in deterministic mode. */
int y2_bn_act_bwd_wino6(const float* z, const float* scale, const float* shift, const float* mean, const float* invstd, const float* gamma,
                        float slope, const float* dy_full, int ldf, int foff, double* sums, float* v6, float* m6, float* dz, int ldd,
                        int B, int H, int W, int C, int ldz, int has_bn, y2_stream_t stream);

/* Backward of y2_maxpool_fwd (overlapping windows allowed): dx[B,H,W,C] from dy (+ optional dy2) [B,Ho,Wo,C]; the gradient of a
 * window goes to its first maximum (ATen semantics). */
int y2_maxpool_bwd(const float* x, const float* dy, const float* dy2, float* dx, int B, int H, int W, int C, int ldx, int ldy, int lddx,
                   int ksize, int stride, int pad, int pad_end, y2_stream_t stream);

/* out[c] += sum_m x[m*ld + c] (fp64; conv-bias gradient of the head, model/yolo2.py:112).  out pre-zeroed. */
int y2_colsum(const float* x, long long M, int C, int ld, double* out, y2_stream_t stream);
/* dst[i] = (float)(src[i] * mul) */
int y2_f64_to_f32(const double* src, float* dst, int n, double mul, y2_stream_t stream);

/* Gradient of the decode (model/__init__.py:122-135) w.r.t. the head image [boxes, 5+C] from the gradients of
 * iou [boxes], center_offset / size_norm [boxes,2], logits [boxes,C] (any may be NULL = zero); yx_min / yx_max carry
 * no gradient (the reference's loss detaches them, model/__init__.py:142). */
int y2_decode_bwd(const float* iou, const float* center_offset, const float* d_iou, const float* d_center_offset, const float* d_size_norm,
                  const float* d_logits, float* d_feature, int boxes, int C, y2_stream_t stream);

/* model.loss (model/__init__.py:138-167) = iou_match (:59-73) + fit_positive (:76-95) + fill_norm (:98-103) + the five
 * terms, each divided by cnt = B*cells*A; cls is the MEAN cross entropy over positives (gt_cls int64 [B,N]) or the
 * summed squared error on softmax (gt_onehot [B,N,C]); C = 0: no cls term.  GT boxes [B,N,2] in cell units, zero rows =
 * padding.  Outputs: loss_out[5] = foreground, background, center, size, cls; saved for backward: best_iou [B,n],
 * best_idx [B,n], positive [B,n] (uint8), sums[6] (fp64: the five sums and the number of positives). n = rows*cols*A. */
int y2_region_loss_fwd(const float* iou, const float* center_offset, const float* size_norm, const float* logits,
                       const float* yx_min, const float* yx_max,
                       const float* gt_yx_min, const float* gt_yx_max, const int64_t* gt_cls, const float* gt_onehot,
                       const float* anchors, int B, int rows, int cols, int A, int C, int N, float threshold,
                       float* best_iou, int32_t* best_idx, uint8_t* positive, double* sums, float* loss_out, y2_stream_t stream);

/* Data-parallel training: after sums[5] (number of positives) has been summed over ranks, recompute loss_out so that
 * the mean-over-positives of the cls term uses the GLOBAL count (cnt stays the local B*cells*A). */
int y2_region_loss_finalize(const double* sums, double cnt, int cross_entropy, float* loss_out, y2_stream_t stream);

/* Gradients of sum_k weights[k]*loss[k] (train.py:348-349) w.r.t. iou, center_offset, size_norm, logits. */
int y2_region_loss_bwd(const float* iou, const float* center_offset, const float* size_norm, const float* logits,
                       const float* gt_yx_min, const float* gt_yx_max, const int64_t* gt_cls, const float* gt_onehot,
                       const float* anchors, int B, int rows, int cols, int A, int C, int N, float threshold,
                       const float* best_iou, const int32_t* best_idx, const uint8_t* positive, const double* sums, const float* weights,
                       float* d_iou, float* d_center_offset, float* d_size_norm, float* d_logits, y2_stream_t stream);

/* ---- fused multi-tensor optimizer -------------------------------------------------------------------
 * One launch updates up to Y2_OPT_MAX_TENSORS parameter tensors (the pointer table is passed by value in the kernel
 * arguments).  Replaces the per-tensor loops of `self.optimizer.step()` (train.py:357; optimizer from the ini lambda,
 * config.ini:72) and `nn.utils.clip_grad_norm` (train.py:352-354).  All tensors fp32, contiguous. */
#define Y2_OPT_MAX_TENSORS 48
typedef struct {
    float* param;
    float* grad;
    float* state1;   /* SGD: momentum buffer (NULL when momentum == 0); Adam: exp_avg; RMSprop: square_avg */
    float* state2;   /* Adam: exp_avg_sq; SGD: NULL; RMSprop: momentum buffer (NULL when momentum == 0) */
    int64_t numel;
} y2_opt_tensor;

/* torch.optim.SGD: d = g + wd*p; buf = first_step ? d : momentum*buf + (1-dampening)*d; d = nesterov ? d + momentum*buf : buf; p -= lr*d */
int y2_opt_sgd(const y2_opt_tensor* tensors, int32_t count, float lr, float momentum, float dampening, float weight_decay,
               int32_t nesterov, int32_t first_step, y2_stream_t stream);
/* torch.optim.Adam (no amsgrad), `step` = 1-based step count of these tensors (bias corrections computed in double on the host) */
int y2_opt_adam(const y2_opt_tensor* tensors, int32_t count, float lr, float beta1, float beta2, float eps, float weight_decay,
                int32_t step, y2_stream_t stream);
/* torch.optim.RMSprop (its single-tensor formula, statement by statement, unfused):
 *   d = g + weight_decay*p (when weight_decay != 0);  square_avg = square_avg*alpha + (1-alpha)*d*d;
 *   centered: grad_avg += (1-alpha)*(d - grad_avg), avg = sqrt(square_avg - grad_avg^2);  otherwise avg = sqrt(square_avg);
 *   avg += eps;  momentum != 0: buf = buf*momentum + d/avg, p -= lr*buf;  otherwise p -= lr*d/avg.
 * state1 = square_avg (required), state2 = momentum_buffer (required iff momentum != 0, not read otherwise).  grad_avg: HOST array of `count`
 * device pointers, required (every entry) iff centered, not read otherwise - centred RMSprop with momentum has three states, y2_opt_tensor two.
 * Rounding: one fp32 rounding per operation, and ONE for each of g + weight_decay*p, square_avg*alpha [rounded] + (1-alpha)*(d*d [rounded]),
 * grad_avg + (1-alpha)*(d - grad_avg [rounded]) and p - lr*x (fused multiply-adds, as torch's element-wise GPU kernels compute them).
 * New states start as zeros (the caller's).  alpha is a double: 1 - alpha is formed in double and then rounded to fp32, as torch does with the Python float.  Same chunking and 16-B / scalar paths as the others
 * (a tensor takes the 16-B path when param, grad and every state it uses are 16-B aligned); no allocation, no synchronisation, capturable.
 * Y2_EINVAL (nothing launched): count outside 1..Y2_OPT_MAX_TENSORS, a NULL param / grad / required state, numel <= 0. */
int y2_opt_rmsprop(const y2_opt_tensor* tensors, int32_t count, float* const* grad_avg, float lr, double alpha, float eps, float weight_decay,
                   float momentum, int32_t centered, y2_stream_t stream);
/* *sumsq (fp64, pre-zeroed, accumulated across calls) += sum of squares of all gradients; then y2_opt_clip_grads scales every
 * gradient by max_norm / (sqrt(*sumsq) + 1e-6) when that is < 1 (torch.nn.utils.clip_grad_norm_, L2).  No host sync. */
int y2_opt_grad_sumsq(const y2_opt_tensor* tensors, int32_t count, double* sumsq, y2_stream_t stream);
int y2_opt_clip_grads(const y2_opt_tensor* tensors, int32_t count, const double* sumsq, float max_norm, y2_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Depthwise 3x3 convolution (model/mobilenet.py conv_dw: nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False)), csrc/dwconv.hip.
 * NHWC fp32, pad 1, stride 1 or 2, output Ho = (H-1)/stride + 1, Wo alike.  The filter w is read in its state_dict layout
 * [C][1][3][3] (no packing).  16-B vector path when C and both pixel strides are multiples of 4 and the two activation bases are
 * 16-B aligned; otherwise a scalar path (any width).  B*H*W < 2^31.  FLOPs = 2*9*B*Ho*Wo*C.
 * ------------------------------------------------------------------------------------------------ */
/* y[b,yo,xo,c] = LeakyReLU_slope(scale[c] * conv + shift[c]) from x [B,H,W] (pixel stride ldx) into y [B,Ho,Wo] (pixel stride ldy);
 * scale / shift NULL = identity, slope 1 = no activation, 0 = ReLU.  stats: NULL, or [Y2_STATS_REPL][2*C] doubles (pre-zeroed)
 * receiving the per-channel sum and sum of squares of the RAW convolution output (as y2_conv_params.stats); Y2_ENOSUP in
 * deterministic mode (take them with y2_colstats_det). */
int y2_dwconv_fwd(const float* x, const float* w, const float* scale, const float* shift, float slope, float* y, double* stats,
                  int B, int H, int W, int C, int ldx, int ldy, int stride, y2_stream_t stream);
/* Data gradient, gather form: dx [B,H,W,C] (pixel stride lddx; H, W = the forward's INPUT size) from dz [B,Ho,Wo,C] (pixel stride
 * ldz).  Every element sums its contributing taps in a fixed order: no atomics, bit-reproducible. */
int y2_dwconv_dgrad(const float* dz, const float* w, float* dx, int B, int H, int W, int C, int ldz, int lddx, int stride, y2_stream_t stream);
/* Weight gradient dw [C][1][3][3] (state_dict layout, overwritten) from the forward input x [B,H,W,C] (pixel stride ldx) and dz
 * [B,Ho,Wo,C] (pixel stride ldz).  Two fixed-order stages, no atomics: per-workgroup partial sums go to `workspace` (16-B aligned, at
 * least y2_dwconv_wgrad_workspace_bytes(B, H, W, C, stride) bytes; else Y2_EALIGN / Y2_EINVAL), one reduce launch adds them.
 * Bit-reproducible in both library modes. */
int y2_dwconv_wgrad(const float* x, const float* dz, float* dw, float* workspace, long long workspace_bytes,
                    int B, int H, int W, int C, int ldx, int ldz, int stride, y2_stream_t stream);
long long y2_dwconv_wgrad_workspace_bytes(int B, int H, int W, int C, int stride);

/* ------------------------------------------------------------------------------------------------
 * Pre-activation kernels of the DenseNet plugin (model/densenet.py; torchvision's _DenseLayer / _Transition: BatchNorm -> ReLU -> 1x1
 * convolution [-> AvgPool2d(2, 2)]), csrc/dense.hip.  NHWC fp32.  The input is a channel slice of a block buffer: x points at the slice's
 * first channel, ldx is the buffer's pixel stride.  pre_scale / pre_shift [K] are the per-INPUT-channel affine (NULL = identity: 1 / 0),
 * pre_slope the LeakyReLU slope behind it (0 = ReLU, 1 = none).  pool = 1: 2x2 / stride-2 average of the pre-activated input (H, W even),
 * everything downstream at [B, H/2, W/2].  16-B vector path when the channel count and the pixel strides of the operands read are multiples
 * of 4 and their bases 16-B aligned; otherwise a scalar path (any width).  B*H*W < 2^31.
 * ------------------------------------------------------------------------------------------------ */
/* out[m][coff + n] = LeakyReLU_slope(scale[n] * sum_k act_pre(pre_scale[k] * x[m][k] + pre_shift[k]) * w[n][k] + shift[n]) for the M = B*Ho*Wo
 * output pixels: the pre-activation runs in the operand loader of an fp32-MFMA GEMM, nothing but the result goes to memory.
 * w: [N][K], a 1x1 weight in its state_dict layout (no packing).  scale / shift [N] or NULL, slope, ldy / coff: as y2_conv_params.
 * stats: NULL, or [Y2_STATS_REPL][2*N] doubles (pre-zeroed) receiving the sum and the sum of squares of the RAW products per output channel;
 * Y2_ENOSUP in deterministic mode (take them with y2_colstats_det).  pool = 1: the window mean is formed in the loader and the GEMM
 * runs at half resolution (average pooling and a 1x1 convolution commute).  FLOPs = 2*M*N*K. */
int y2_preact_conv1x1_fwd(const float* x, const float* w, const float* pre_scale, const float* pre_shift, float pre_slope,
                          const float* scale, const float* shift, float slope, float* y, double* stats,
                          int B, int H, int W, int K, int ldx, int N, int ldy, int coff, int pool, y2_stream_t stream);
/* The materialising form: out[m][c] = act_pre(pre_scale[c] * x[m][c] + pre_shift[c]) (pool = 1: its 2x2 window mean, summed in the order
 * the GEMM loader uses) into out [B,Ho,Wo] with pixel stride ldo: the operand of the 1x1 weight gradient (y2_conv_wgrad, ksize 1). */
int y2_preact_fwd(const float* x, const float* pre_scale, const float* pre_shift, float pre_slope, float* out,
                  int B, int H, int W, int C, int ldx, int ldo, int pool, y2_stream_t stream);
/* Backward of (BatchNorm with batch statistics | frozen BatchNorm | nothing) -> LeakyReLU [-> AvgPool 2x2] on a channel slice: has_bn = 1 / 2 / 0
 * as y2_bn_act_bwd.  pre_scale / pre_shift: the forward's affine (rebuilds the activation mask; zero gradient at 0 like torch); mean, invstd,
 * gamma [C] (has_bn != 0).  dA: gradient of the forward's output, [B,Ho,Wo] with pixel stride ldda (pool = 1: every element of a window
 * receives dA / 4).  With g = the gradient behind the mask and xhat = (x - mean) * invstd:
 *   sums [2C] fp64 = [sum g | sum g * xhat] = [d beta | d gamma] - pre-zeroed by the caller (fp64 atomics); in deterministic mode written
 *   through a fixed tree of per-workgroup partial sums;
 *   dx = gamma * invstd * (g - sum g / M - xhat * sum g xhat / M), M = B*H*W (has_bn 1);  g * gamma * invstd (has_bn 2);  g (has_bn 0),
 * WRITTEN (accumulate = 0) or ADDED (accumulate = 1) to dx [B,H,W] with pixel stride lddx - the slice of the block's gradient buffer. */
int y2_preact_bwd(const float* x, const float* pre_scale, const float* pre_shift, float pre_slope, const float* mean, const float* invstd,
                  const float* gamma, const float* dA, int ldda, double* sums, float* dx, int lddx, int accumulate,
                  int B, int H, int W, int C, int ldx, int pool, int has_bn, y2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* YOLO2_HIP_H */
