/*
 * slfp.h -- C ABI of libslfp_hip.so: the MI355X (gfx950) SLFP<3,4> / SFP<3,3> quantized
 * conv2d forward path.
 *
 * This is the drop-in boundary for the hot path of happyxtt/CNNs_SLFP_quantization:
 *   utils/sfp_quant.py    quantize_act / quantize_weight (fake-quant codecs)
 *   utils/conv2d_func.py  Conv2d_Q.forward (conv2d_Q, conv2d_Q_bias), Linear_Q.forward
 * Every entry point takes plain device pointers and sizes (no torch types), is
 * asynchronous on the hipStream_t passed as `void* stream` (NULL = the default stream),
 * never allocates, never synchronises, never throws, and returns an int status
 * (0 = ok, < 0 = error; slfp_last_error() gives the text).  The reference raises Python
 * exceptions (an assert at sfp_quant.py:138 and shape errors from F.conv2d); the host
 * binding maps non-zero statuses to the same exception types.
 *
 * Threading: no mutable state on the launch path except a thread-local last-error string and lock-protected caches of
 * derived constants (threshold tables per scale, occupancy / CU count per device); safe to call from any host thread; one
 * device per process is assumed (multi-GPU = one process per GPU, as torch.distributed/RCCL launches them).
 * Environment: a handful of SLFP_* experiment switches (csrc/slfp_host.hpp: Switches) are read ONCE when the library is
 * loaded -- never per launch; slfp_debug_reload_switches() re-reads them (profiling tools only).
 */
#ifndef SLFP_H_
#define SLFP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLFP_ABI_VERSION 1

/* status codes */
#define SLFP_OK 0
#define SLFP_ERR_BAD_ARG (-1)     /* null pointer, bad enum, non-positive size, bad Qbits */
#define SLFP_ERR_SHAPE (-2)       /* inconsistent conv geometry (what F.conv2d would reject) */
#define SLFP_ERR_UNSUPPORTED (-3) /* valid but not implemented on this path (e.g. dilation with NCHW) */
#define SLFP_ERR_ALIGNMENT (-4)   /* a pointer is not aligned as the kernel needs (16 B) */
#define SLFP_ERR_HIP (-5)         /* a HIP runtime call failed (launch error etc.) */

/* codec formats (the `fmt` argument) */
#define SLFP_FMT_ACT8 0 /* quantize_act(8):    SLFP<3,4> activations, utils/sfp_quant.py:80-96 */
#define SLFP_FMT_W8 1   /* quantize_weight(8): SLFP<3,4> weights,     utils/sfp_quant.py:32-47 */
#define SLFP_FMT_SFP7 2 /* quantize_{act,weight}(7): SFP<3,3>,        utils/sfp_quant.py:14-30,63-78 */
#define SLFP_FMT_EXT 4  /* OR-able: extended code points (exact zero = 0x01, clamp literal =
                           sign|0x02) so that decode(encode(x)) == quantize(x) bit for bit */

/* tensor layouts */
#define SLFP_LAYOUT_NCHW 0 /* the reference's layout (contiguous NCHW) */
#define SLFP_LAYOUT_NHWC 1 /* channels-last: the native layout of the HIP kernels */

/* pointwise/implicit-GEMM MFMA operand precision (slfp_conv2d_desc.mfma_passes) */
#define SLFP_MFMA_DEFAULT 0 /* library default = SLFP_MFMA_F16X1 (meets the 1e-3 parity bar) */
#define SLFP_MFMA_F16X1 1   /* one fp16 MFMA pass: ~2.5e-4 tensor-relative error on SLFP<3,4> */
#define SLFP_MFMA_F16X3 3   /* hi/lo split, three passes: float32-equivalent (~1e-6) */

int slfp_version(void);
/* Re-reads the SLFP_* experiment switches from the environment (profiles/variants.py); not for production use. */
void slfp_debug_reload_switches(void);
/* Text of the last error on the calling thread ("" if none). Never NULL. */
const char* slfp_last_error(void);
/* Number of visible HIP devices (0 if none / runtime unavailable). */
int slfp_device_count(void);

/* ---- codec: replaces quantize_act(k) / quantize_weight(k) .forward ------------------
 * q = x[i] / scale_div is an IEEE float32 division, exactly as `input/self.Ka`
 * (utils/conv2d_func.py:21-22) with the float64 0-dim scale cast to float32.           */

/* code[i] = canonical code of Q_fmt(q): sign<<7 | (E+4)<<4 | m  (Qbits 8)
 *                                        sign<<6 | (E+4)<<3 | m  (Qbits 7)
 * (bit layout from the comments at utils/sfp_quant.py:95 and :125). */
int slfp_encode_f32(const float* x, uint8_t* code, size_t n, float scale_div, int fmt, void* stream);
/* y[i] = float32 value of code[i] (inverse of the above; with SLFP_FMT_EXT exact). */
int slfp_decode_f32(const uint8_t* code, float* y, size_t n, int fmt, void* stream);
/* y[i] = Q_fmt(q) as float32: bit-identical to what qfn.forward returns
 * (utils/sfp_quant.py:10-48, :59-97).  x == y (in place) is allowed. */
int slfp_quantize_f32(const float* x, float* y, size_t n, float scale_div, int fmt, void* stream);

/* y[i] = SFP<4,4> layer-output quantizer: replaces quantize_layerout(k <= 8).forward
 * (utils/sfp_quant.py:108-127), bit-identical including its quirks (the reference's `2^(-8)` is an
 * integer XOR, so only RNE to 5 significant bits, the >= 248 clamp and NaN-for-exact-zero are live). */
int slfp_quantize_layerout_f32(const float* x, float* y, size_t n, void* stream);
/* *out = max_i |x[i]| (device pointer to one float32): the per-layer statistic of the reference's
 * calibration pass get_scale_factor (cifar100_train_eval.py:261-271); Ka = max / 15.5. */
int slfp_absmax_f32(const float* x, size_t n, float* out, void* stream);

/* ---- conv2d: replaces Conv2d_Q.forward (utils/conv2d_func.py:20-25 and :41-47) ------ */

typedef struct slfp_conv2d_desc {
    int64_t n, c_in, h, w;    /* input  N x C_in x H x W (logical NCHW sizes)              */
    int64_t c_out, kh, kw;    /* weight C_out x (C_in/groups) x KH x KW                     */
    int32_t stride_h, stride_w, pad_h, pad_w, dil_h, dil_w, groups;
    int32_t x_layout, y_layout; /* SLFP_LAYOUT_*: memory layout of x and of y                 */
    int32_t qbits;            /* 8 = SLFP<3,4>, 7 = SFP<3,3>  (32 is a host-side passthrough) */
    float ka, kw_scale;       /* float32(Ka), float32(Kw): the module's calibration scales    */
    int32_t mfma_passes;      /* SLFP_MFMA_*                                                   */
    int32_t reserved;
} slfp_conv2d_desc;

/* Validates the geometry; writes the output spatial size. */
int slfp_conv2d_out_shape(const slfp_conv2d_desc* d, int64_t* h_out, int64_t* w_out);
/* Which kernel family slfp_conv2d_fwd will run for this descriptor (for logs/tests):
 * a static string such as "dw3x3_nhwc", "pw_mfma_f16x3", "dense_mfma_f16x1", "direct_nhwc". */
const char* slfp_conv2d_kernel_name(const slfp_conv2d_desc* d);
/* Which depthwise 3x3 kernel slfp_conv2d_fwd (has_post == 0) / slfp_conv2d_fwd_post (has_post != 0; no layer-output
 * quantizer) will run for this bias-free descriptor under the switches read at load (tests, logs): "rows" (csrc/conv_dw3.hip),
 * "tile" (csrc/conv_dw2.hip), "general" (csrc/conv_dw.hip), or "none" when the descriptor is not of the dw3x3 family.
 * Host only: no device is touched. */
const char* slfp_debug_dw3x3_variant(const slfp_conv2d_desc* d, int has_post);
/* Which dense k x k kernel (csrc/conv_dense.hip) a forward of this descriptor launches under the switches read at load, with
 * float32 (x_codes == 0) or 1-byte codes (x_codes != 0) on the input side; "none" when the descriptor is not of the dense_mfma_*
 * family.  Per-tile kernels: "<wm><wn><mt>/<body>/nwb<N>/ns<N>/p<N>" = tiling, body ("k3x3": the unrolled 3x3 stride-1
 * kernel, "gen": the general one), weight buffers, halo slots per wave, operand planes, e.g. "424/k3x3/nwb3/ns6/p1".  The
 * weights-resident persistent kernel: "res/mt<N>/ns<N>", with "/encx" when it encodes the float32 input itself.  The string
 * is printed from the selection the launch consumes.  Host only: no device is touched.  The pointer stays valid
 * until the next call on the same thread. */
const char* slfp_debug_dense_variant(const slfp_conv2d_desc* d, int x_codes);
/* Which pointwise (1x1) kernel instance (csrc/conv_pw.hip, csrc/conv_pw_codes.hip) the matching forward entry point launches for
 * this descriptor under the switches read at load; "none" outside the pw_mfma_* family or where that entry point refuses the
 * call.  io (NULL: float32 on both sides) says whether codes come in and go out and describes the reader of output codes; has_res:
 * slfp_conv2d_fwd_res; has_res_codes (with has_res): slfp_conv2d_fwd_res_codes, io->y_ka / y_qbits describing the reader of the second
 * output; y_ld != 0: slfp_conv2d_fwd_codes_slice.  The string names the kernel and every template argument the launcher chose:
 *   stream/ks<N>/<kfull|kpart|a8>/<tab|long>/<stg|dir>/p<1|3>/<act8|sfp7>[/res|/yc][/grid<n>]      k_pw_stream
 *   tiled/<wm><wn><mt>/<kfull|kpart>/<tab|long>/<stg|dir>/p<1|3>/<act8|sfp7>[/res|/yc]             k_pw_tiled
 *   pwc-stream/ks<N>/<xw|dw|half>/<act8|sfp7>/<f32|yc|res|res/dual>[/grid<n>]                      k_pwc_stream
 *   slice/nts<4|8>/<act8|sfp7>/<f32|yc|res|res/dual>[/grid<n>]                                     k_pwc_slice
 *   pwc-tiled/<wm><wn><mt>/<act8|sfp7>/<f32|yc|res|res/dual>                                       k_pwc_tiled
 * (/grid<n>: SLFP_PW_GRID caps the persistent grid.)  It is printed from the selection the launch consumes (DESIGN.md section
 * 19).  Host only: no device is touched.  The pointer stays valid until the next call on the same thread. */
struct slfp_conv2d_io;   /* defined below */
/* Which depthwise 3x3 template instance (csrc/conv_dw.hip, conv_dw2.hip, conv_dw3.hip, conv_dwc.hip) the matching forward entry
 * point launches for this descriptor under the switches read at load; "none" outside the dw3x3 family or where that entry point
 * refuses the call.  io == NULL (or codes on neither side): slfp_conv2d_fwd / slfp_conv2d_fwd_post; codes on the input side:
 * slfp_conv2d_fwd_codes, or, with SLFP_POST_LAYEROUT in post_flags, slfp_conv2d_fwd_codes_lut (the layer-output quantizer on codes
 * is the table epilogue).  has_bias / has_post: a bias / a post_scale + post_shift pair is passed; post_flags: the `relu` argument
 * (SLFP_POST_RELU | SLFP_POST_LAYEROUT).  One word per template argument the launcher chooses:
 *   general/s<1|2>/<cb32iw16|cb64iw9|cb32iw15|gen>/v<4|2>/<tab|long>/<act8|sfp7>[/lo]        k_dw3x3<FMT, S, CBT, IWT, V, LO, TAB>
 *   tile/s<1|2>/<plain|post>                                                                k_dw3x3_tile<S, 14 | 7, 14 | 7, POST>
 *   rows/<plain|post>                                                                       k_dw3x3_rows<7, POST>
 *   dwc/s<1|2>/lc<3|4|5>/<f32|yc|yc-signed|lut>/<plain|post>/<act8|sfp7>                     k_dwc<S, LCS, 7 | 4, 2 | 1, YC, POST, SIGNED, LUTQ>
 * (cb<N>iw<N>: the geometry-specialised channel-group / halo-width forms, gen: the generic one; v<N>: floats per lane; tab / long:
 * threshold-table / long-form input quantizer; /lo: the fused layer-output quantizer; f32 / yc / yc-signed / lut: float32 out,
 * codes with the ReLU folded into the quantizer, signed codes, the table epilogue; the last word of a dwc string is the format
 * of the input codes, a runtime argument of that kernel.)  The string is printed from the selection the launch consumes
 * (DESIGN.md section 26).  Host only: no device is touched.  The pointer stays valid until the next call on the same thread.
 *
 * Arithmetic of the depthwise 3x3 kernels.  All five kernels compute every output element by the same float32 steps, so their
 * results are equal bit for bit (a NaN equals a NaN) to one another and to the CPU restatement oracle/slfp_oracle.c:
 * slfp_oracle_dw3x3_f32:
 *   1. xq = QA(x / Ka) (code input: the decoded code), wq = QW(w / Kw);
 *   2. acc = +0, or bq = (bias / Ka) / Kw -- two IEEE float32 divisions -- when there is a bias;
 *   3. nine acc = fmaf(xq, wq, acc) in (kh, kw) order; a padded tap contributes fmaf(+0, wq, acc);
 *   4. t = (acc * Ka) * Kw, two roundings;
 *   5. with post_scale / post_shift: t = fmaf(t, scale[c], shift[c]);
 *   6. with SLFP_POST_LAYEROUT: t = the layer-output quantizer of t (slfp_quantize_layerout_f32);
 *   7. with SLFP_POST_RELU: t = fmaxf(t, 0) (a NaN gives 0).
 * Code output is the extended code of QA(t / y_ka) of that float32 t; the table epilogue is the byte table's entry for step 6's class. */
const char* slfp_debug_dw3x3_instance(const slfp_conv2d_desc* d, const struct slfp_conv2d_io* io, int has_bias, int post_flags, int has_post);
const char* slfp_debug_pw_variant(const slfp_conv2d_desc* d, const struct slfp_conv2d_io* io, int has_res, int has_res_codes, int64_t y_ld);
/* Which image-stem or direct kernel instance (csrc/conv_direct.hip, conv_stem_small.hip, conv_stem_mfma.hip) the matching forward
 * entry point launches for this descriptor under the switches read at load; "none" for a null descriptor, outside the direct_nhwc /
 * stem_nhwc / stem_small_mfma_* / stem_mfma_* families, on channel-padded copies, or where that entry point refuses the call.
 * io == NULL (or codes on neither side): slfp_conv2d_fwd / slfp_conv2d_fwd_post; io->y_codes: slfp_conv2d_fwd_codes[_ws], or, with
 * SLFP_POST_LAYEROUT in post_flags, slfp_conv2d_fwd_codes_lut (these kernels read float32: io->x_codes gives "none").  has_bias /
 * has_post / post_flags as for slfp_debug_dw3x3_instance.  One word per template argument or runtime form a launcher chooses:
 *   direct/<act8|sfp7>/cc<CC>/oc<chunks>/<vec|scalar|mixed>     k_direct<FMT>; CC input channels per LDS chunk, 64-channel output
 *                                                               chunks per group, and what the threads decide from C_out and
 *                                                               C_out / groups: 16-byte weight loads and stores in every live
 *                                                               thread, in none (C_out % 4 != 0), or in some (C_out / groups % 4 != 0)
 *   stem/gen/<act8|sfp7>/p<2|4|8>                               k_stem<FMT>, P output rows per thread (C_out = 16 / 32 / 64)
 *   stem/fixed/<act8|sfp7>/long                                 k_stem_fixed<FMT, 3, 3, 3, 2, 32>: the long-form quantizer
 *   stem/fixed/tab/<f32|yc|yc-signed|lut>                       k_stem_fixed<Act8, 3, 3, 3, 2, 32, TAB, 16, YC, LUTQ>
 *   stem/mx/<f32|yc|yc-signed|lut>                              k_stem_mx<YC, LUTQ>
 *   small/nt<1|2|3|4>/<act8|sfp7>/<f32|yc|yc-signed|lut>        k_stem_small<FMT, NT, LUTQ>
 *   rows/nt<4|6>/<act8|sfp7>/<f32|yc|yc-signed>                 k_stem_rows<FMT, NT, YC>
 *   im2row/nt<4|6>/<act8|sfp7>/<f32|yc|yc-signed>               k_stem_im2row<FMT> + k_stem_mfma<NT, 8, YC>
 * (f32 / yc / yc-signed / lut as for the dwc strings; yc against yc-signed is a runtime argument of the YC instance.)  k_stem_mx is
 * selected only where its aligned 16-byte halo loads are valid: W * 3 a multiple of 4 AND pad_w = 1 (mod 4); every other 3x3 stride-2
 * 3 -> 32 layer with a threshold table runs stem/fixed/tab.  The string is printed from the selection the launch consumes, and
 * slfp_conv2d_codes_supported / slfp_conv2d_codes_lut_supported ask the same selection.  Host only: no device is touched.  The pointer
 * stays valid until the next call on the same thread.
 *
 * Arithmetic of the float32 kernels (k_direct, k_stem, k_stem_fixed, k_stem_mx).  They compute every output element by the same
 * float32 steps, so their results equal the CPU restatement oracle/slfp_oracle.c: slfp_oracle_conv_f32 bit for bit (a NaN equals a NaN):
 *   1. xq = QA(x / Ka) as float32, wq = QW(w / Kw);
 *   2. acc = +0; one acc = fmaf(xq, wq, acc) per tap: k_direct in input-channel chunks of CC outermost, then (kh, kw, c) inside a
 *      chunk; the stems in (kh, kw, c) order; a padded tap contributes fmaf(+0, wq, acc).  k_stem_mx (the float32 matrix core, which
 *      multiplies exactly and accumulates in k order) appends a 28th tap fmaf(+0, +0, acc).  That tap changes no bit: it could only
 *      turn a -0 accumulator into +0, and an accumulator that starts at +0 is never -0 (in round-to-nearest a -0 product added to
 *      +0 gives +0, an exact cancellation gives +0, and the quantized operands are too large for a non-zero sum to underflow);
 *      a NaN stays a NaN;
 *   3. t = ((acc + (bias / Ka) / Kw) * Ka) * Kw -- two IEEE float32 divisions, one addition (no bias: acc + +0), two roundings;
 *   4. with post_scale / post_shift: t = fmaf(t, scale[c], shift[c]);
 *   5. with SLFP_POST_LAYEROUT (and the affine): t = the layer-output quantizer of t (slfp_quantize_layerout_f32);
 *   6. with SLFP_POST_RELU: t = fmaxf(t, 0) (a NaN gives 0);
 *   7. code output as for the depthwise family: the extended code of QA(t / y_ka) of step 5's float32 t, the ReLU folded into the
 *      quantizer; the table epilogue is the byte table's entry for the class of step 5's value.
 * The fp16 matrix-core stems (small, rows, im2row) contract float16(16 xq) with float16(16 wq) on the matrix cores, whose internal
 * order is not specified: they are held to an operand-level reference within a rounding-count bound (tests/test_gpu_stem_variants.py). */
const char* slfp_debug_stem_instance(const slfp_conv2d_desc* d, const struct slfp_conv2d_io* io, int has_bias, int post_flags, int has_post);

/* Bytes of the prepared-weight blob for this layer (device memory the caller owns). */
size_t slfp_conv2d_wprep_bytes(const slfp_conv2d_desc* d);
/* Quantize the float32 OIHW weights once: weight_q = QW(w / Kw) (conv2d_func.py:22) and
 * lay them out for the kernel this descriptor selects.  weight_q_oihw (optional, may be
 * NULL) receives the reference's `self.weight_q` tensor (float32, OIHW).  The reference
 * re-quantizes the weights on every forward; callers cache the blob and call this again
 * whenever the weight tensor changes. */
int slfp_conv2d_prepare_weights(const slfp_conv2d_desc* d, const float* w_oihw, void* wprep,
                                float* weight_q_oihw, void* stream);
/* The same blob from the weights' 1-byte codes: codes_oihw[i] = slfp_encode_f32(w, Kw, fmt | SLFP_FMT_EXT)[i] with fmt =
 * SLFP_FMT_W8 (qbits 8) or SLFP_FMT_SFP7 (qbits 7).  decode(encode(x)) == quantize(x) bit for bit, so the blob is
 * identical to slfp_conv2d_prepare_weights' -- this is what a rank builds from the broadcast of SURVEY 8(e)
 * (quantized weights travel as u8 codes, 1 B per weight; each rank lays them out for its own kernels). */
int slfp_conv2d_prepare_weights_codes(const slfp_conv2d_desc* d, const uint8_t* codes_oihw, void* wprep,
                                      float* weight_q_oihw, void* stream);
/* Bytes of scratch slfp_conv2d_fwd needs for this descriptor: 0 for the HBM-bound NHWC families
 * (depthwise, pointwise, 3x3 stems); non-zero when a layout conversion is involved and for the
 * two MFMA families of compute-bound layers ("dense_mfma_*": k x k with C_in >= 16,
 * "stem_mfma_*": C_in <= 4 with KH*KW >= 25), which encode the input once to fp16 into it.
 * The contents are scratch: nothing persists between calls. */
size_t slfp_conv2d_workspace_bytes(const slfp_conv2d_desc* d);
/* y = conv2d(QA(x/Ka), weight_q, bias/Ka/Kw) * Ka * Kw.
 * bias: NULL for conv2d_Q (conv2d_func.py:20-25), float32[C_out] for conv2d_Q_bias (:41-47).
 * input_q (optional, may be NULL): receives QA(x/Ka) in x's layout (the reference's
 * `self.input_q`).  workspace: slfp_conv2d_workspace_bytes(d) bytes or NULL if that is 0. */
int slfp_conv2d_fwd(const slfp_conv2d_desc* d, const float* x, const void* wprep, const float* bias,
                    float* y, float* input_q, void* workspace, void* stream);

/* Same, with the eval-mode BatchNorm2d (+ ReLU) that follows every Conv2d_Q in the reference
 * nets (nets_imgnet/mobilenetv1.py:24-41, resnet50.py:74-88) fused into the epilogue (SURVEY 8f
 * rank 1):   y = act(conv_q_out * post_scale[c] + post_shift[c]),  act = max(., 0) if relu.
 * post_scale = gamma / sqrt(running_var + eps), post_shift = beta - running_mean * post_scale,
 * float32[C_out], 16-byte aligned; both NULL = no affine.  The conv result itself keeps the
 * reference's (out * Ka) * Kw roundings; the affine is one fused multiply-add on top. */
#define SLFP_POST_RELU 1      /* `relu` argument of slfp_conv2d_fwd_post: max(., 0) last                         */
#define SLFP_POST_LAYEROUT 2  /* SFP<4,4> layer-output quantizer (slfp_quantize_layerout_f32) between the affine
                                 and the ReLU: the [Conv2d_Q, BatchNorm2d, layerout_quantize_func, ReLU] blocks of
                                 MobileNetV1_swish / VGG16_gelu / ShuffleNetV2 (nets_cifar/mobilenetv1.py:196-231);
                                 needs post_scale / post_shift                                                  */
int slfp_conv2d_fwd_post(const slfp_conv2d_desc* d, const float* x, const void* wprep, const float* bias,
                         const float* post_scale, const float* post_shift, int relu, float* y,
                         float* input_q, void* workspace, void* stream);

/* ---- one MobileNet block in one launch (second half) ---------------------------------------------
 * nets_imgnet/mobilenetv1.py:24-41's conv_dw block -- Conv2d_Q(3x3, groups = C) -> BatchNorm2d -> ReLU -> Conv2d_Q(1x1)
 * -> BatchNorm2d -> ReLU -- with the depthwise result quantized for the pointwise layer where it is produced and handed
 * to the matrix cores through LDS as fp16: the intermediate tensor never goes to HBM.  Bit-identical to
 * slfp_conv2d_fwd_post(dw) followed by slfp_conv2d_fwd_post(pw) in the single-pass MFMA mode.  `dw` / `pw` are the two
 * layers' descriptors (NHWC; pw's input size = dw's output size), wprep_* their prepared weights, post1_* the folded
 * BatchNorm of the depthwise layer (required), post2_* that of the pointwise layer (or NULL), relu*: 0 / 1 (anything else:
 * SLFP_ERR_BAD_ARG before any other argument is looked at).
 * slfp_dwpw_supported: 1 if the pair can be fused (3x3 depthwise stride 1 / 2, C in {32, 64, 128}, N in {64, 128, 256},
 * C * N * 2 B <= 64 KiB, single-pass mode, threshold tables available for both Ka), else 0. */
int slfp_dwpw_supported(const slfp_conv2d_desc* dw, const slfp_conv2d_desc* pw);
int slfp_dwpw_fwd(const slfp_conv2d_desc* dw, const slfp_conv2d_desc* pw, const float* x, const void* wprep_dw,
                  const float* post1_scale, const float* post1_shift, int relu1, const void* wprep_pw,
                  const float* bias_pw, const float* post2_scale, const float* post2_shift, int relu2, float* y,
                  void* stream);

/* ---- inter-layer activations as 1-byte codes ("... + next layer's encode") ---------------------------
 * Every Conv2d_Q of the reference nets feeds BatchNorm2d -> ReLU -> the next Conv2d_Q, whose first step is
 * input_q = quantize_act(input / Ka) (utils/conv2d_func.py:21; nets_imgnet/mobilenetv1.py:24-33).  With `y_codes` the
 * producer applies the CONSUMER's quantizer in its epilogue and stores, per element, the byte
 *     slfp_encode_f32(out, y_ka, fmt(y_qbits) | SLFP_FMT_EXT)
 * instead of the float32 value; with `x_codes` a layer reads such bytes (written for ITS Ka and qbits) in place of the
 * float32 tensor and skips its own quantizer.  Classes and values are the same as on the float32 interface, so a chain
 * of layers linked this way returns bit for bit what slfp_conv2d_fwd_post returns layer by layer (single-pass MFMA mode /
 * SFP<3,3>), while activations cross HBM as 1 B per element instead of 4.  NaN has no code (it becomes 0x00, as in
 * slfp_encode_f32).  Both tensors are NHWC; x, y and wprep 16-byte aligned; wprep is the blob of
 * slfp_conv2d_prepare_weights for the same descriptor.  Supported: 3x3 depthwise (x_codes), 1x1 (x_codes; C_in a
 * multiple of 32, or 16 or 48; C_out a multiple of 16 with y_codes), and the 3x3 stride-2 RGB stem -> 32 channels (float32 in, y_codes):
 * every layer of nets_imgnet/mobilenetv1.py:43-57; the 3x3 RGB stem -> 64 channels of VGG-16 (float32 in, y_codes); the
 * large-kernel image stems of the "stem_mfma_*" family (float32 in, y_codes; C_out a multiple of 16: ResNet-50's 7x7 s2 3 -> 64,
 * SqueezeNet's 7x7 s2 3 -> 96, AlexNet's 11x11 s4 3 -> 64) -- the stems that keep their encoded rows in LDS here, the others
 * (AlexNet's, odd stride * C_in) through slfp_conv2d_fwd_codes_ws; dense k x k layers through slfp_conv2d_fwd_codes_ws (below).
 * slfp_conv2d_codes_supported answers 1 / 0 without device work. */
typedef struct slfp_conv2d_io {
    int32_t x_codes;  /* 0: x is float32 (as slfp_conv2d_fwd); 1: x is uint8 codes of QA(. / d->ka), format of d->qbits */
    int32_t y_codes;  /* 0: y is float32; 1: y receives uint8 codes of QA(out / y_ka) in the format of y_qbits        */
    float y_ka;       /* float32(Ka) of the layer that will read y                                                   */
    int32_t y_qbits;  /* its q_bit: 8 = SLFP<3,4>, 7 = SFP<3,3>                                                       */
} slfp_conv2d_io;
int slfp_conv2d_codes_supported(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int relu);
/* post_scale / post_shift / relu as in slfp_conv2d_fwd_post (SLFP_POST_LAYEROUT is not supported here). */
int slfp_conv2d_fwd_codes(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, const void* x, const void* wprep,
                          const float* bias, const float* post_scale, const float* post_shift, int relu, void* y,
                          void* stream);
/* The same with a workspace, for the layers whose float32 form needs one: dense k x k convolutions on the matrix cores
 * (VGG-16 / ResNet-50 3x3, SqueezeNet expand3x3; x_codes and / or y_codes; C_out a multiple of 16 with y_codes) and the
 * large-kernel image stems that run as two kernels (the im2row copy lies in it; float32 in, y_codes).  `workspace`:
 * slfp_conv2d_workspace_bytes(d) bytes, 16-byte aligned; may be NULL for the layers slfp_conv2d_fwd_codes takes.  The codes
 * are decoded into the same fp16 operand copy the float32 interface builds from its input: results are bit-identical. */
int slfp_conv2d_fwd_codes_ws(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, const void* x, const void* wprep,
                             const float* bias, const float* post_scale, const float* post_shift, int relu, void* y,
                             void* workspace, void* stream);
/* ---- one MobileNet block in one launch, on codes ------------------------------------------------------------------------------
 * slfp_dwpw_fwd's pair of layers inside a chain of codes: x holds the depthwise layer's input codes (io->x_codes must be 1: codes
 * of QA(. / dw->ka) in the format of dw->qbits), y receives float32 (io->y_codes = 0) or the codes of the reader io->y_ka /
 * io->y_qbits describe (io->y_codes = 1).  The depthwise result goes through the pointwise layer's quantizer straight into the
 * matrix cores' fp16 operand in LDS: no code is formed for it and it never reaches HBM.  Bit-identical to slfp_conv2d_fwd_codes(dw, codes ->
 * codes for pw->ka) followed by slfp_conv2d_fwd_codes(pw, codes -> y).  The other arguments are slfp_dwpw_fwd's (post1_* required;
 * bias_pw / post2_* may be NULL; relu*: 0 / 1; every pointer 16-byte aligned).
 * slfp_dwpw_codes_supported answers 1 / 0 without device work: 1 where slfp_dwpw_supported takes the pair (3x3 depthwise, stride
 * 1 / 2, C in {32, 64, 128}, N in {64, 128, 256}, C * N * 2 B <= 64 KiB, NHWC, single-pass mode or SFP<3,3>, one q_bit), the
 * depthwise layer alone is one slfp_conv2d_fwd_codes takes, the reader's quantizer is valid (y_qbits 8 or 7, y_ka > 0 with a code
 * table), relu1 / relu2 are 0 or 1 (no SLFP_POST_LAYEROUT) and the kernel's LDS (<= 160 KiB) and offsets fit; K >= 256 blocks,
 * float32 input, the three-pass mode and everything else: 0, and slfp_dwpw_fwd_codes then returns SLFP_ERR_UNSUPPORTED. */
int slfp_dwpw_codes_supported(const slfp_conv2d_desc* dw, const slfp_conv2d_desc* pw, const slfp_conv2d_io* io,
                              int has_bias_pw, int relu1, int relu2);
int slfp_dwpw_fwd_codes(const slfp_conv2d_desc* dw, const slfp_conv2d_desc* pw, const slfp_conv2d_io* io, const void* x,
                        const void* wprep_dw, const float* post1_scale, const float* post1_shift, int relu1,
                        const void* wprep_pw, const float* bias_pw, const float* post2_scale, const float* post2_shift,
                        int relu2, void* y, void* stream);
/* Which template instance of the one-kernel block a call would run.  io == NULL: slfp_dwpw_fwd's k_dwpw<S, KS, NT>, as
 *   f32/s<1|2>/k<1|2|4>/n<4|8|16>
 * otherwise slfp_dwpw_fwd_codes' k_dwpw_codes<S, KS, NT, FMT, YC>, as
 *   codes/s<1|2>/k<1|2|4>/n<4|8|16>/<act8|sfp7>/<f32|yc>
 * (s: the depthwise stride; k: C / 32; n: pointwise C_out / 16; act8 / sfp7: the format of the input codes; f32 / yc: float32 or
 * code output).  "none" wherever slfp_dwpw_supported / slfp_dwpw_codes_supported answers 0 (null descriptors and relu bits other
 * than 0 / 1 included).  The string is printed from the selection the queries and the launchers consume, so a query answers 1
 * exactly where its launcher has an instance.  Host only: no device is touched.  The pointer stays valid until the next call on
 * the same thread. */
const char* slfp_debug_dwpw_instance(const slfp_conv2d_desc* dw, const slfp_conv2d_desc* pw, const slfp_conv2d_io* io,
                                     int has_bias_pw, int relu1, int relu2);
/* ---- code output into a channel slice: a concat without the copy ------------------------------------------------------------
 * slfp_conv2d_fwd_codes_ws with the code output written into a channel slice of a WIDER NHWC code tensor: y points at the
 * slice's first channel of pixel 0, y_ld is the wider tensor's channel count = the byte distance between two pixels.  The two
 * expand layers of a SqueezeNet Fire module (nets_imgnet/squeezenet1_0.py:41-46) write the two halves of the concatenated
 * tensor this way, so torch.cat never runs.  Requires io->y_codes == 1, y_ld >= c_out, y_ld a multiple of 16 and y 16-byte
 * aligned (so the channel offset is a multiple of 16).  The bytes written are exactly those slfp_conv2d_fwd_codes_ws writes for
 * the same arguments, pixel by pixel; nothing outside the slice is touched; y_ld == c_out is slfp_conv2d_fwd_codes_ws.
 * Supported (slfp_conv2d_codes_slice_supported: 1 / 0, host only): the 1x1 layers on codes of the pw_mfma_* family and the dense
 * k x k layers (codes or float32 in), wherever slfp_conv2d_codes_supported says yes; depthwise and stem layers return
 * SLFP_ERR_UNSUPPORTED.  1x1 layers on codes take C_in = 16 and 48 next to the multiples of 32 (Fire 3/4 and 8/9 squeeze to
 * 16 and 48 channels), and 96 among those (the squeeze behind the stem).  workspace: as slfp_conv2d_fwd_codes_ws. */
int slfp_conv2d_codes_slice_supported(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int relu, int64_t y_ld);
int slfp_conv2d_fwd_codes_slice(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, const void* x, const void* wprep,
                                const float* bias, const float* post_scale, const float* post_shift, int relu, void* y,
                                int64_t y_ld, void* workspace, void* stream);
/* ---- entry: the layer at which a chain of codes begins, for the 1x1 layers of the pw_mfma_* family ------------------------------
 * slfp_conv2d_fwd_entry reads the float32 tensor x (as slfp_conv2d_fwd_post does) and writes, per output element, the byte
 *     slfp_encode_f32(y, io->y_ka, fmt(io->y_qbits) | SLFP_FMT_EXT)
 * of the float32 value y that slfp_conv2d_fwd_post writes for the same d, x, wprep, bias, post_scale, post_shift and relu -- bit
 * for bit, in ONE launch: conv1 of a ResNet-50 Bottleneck (nets_imgnet/resnet50.py:76-80) reads the float32 trunk and hands conv2
 * 1-byte codes; the first Fire squeeze of SqueezeNet reads the pooled float32 stem output.  Requires io->x_codes == 0 and
 * io->y_codes == 1.  wprep: the blob of slfp_conv2d_prepare_weights, unchanged.  y_codes: uint8 NHWC, C_out bytes per pixel.  x,
 * y_codes, wprep, bias, post_scale and post_shift 16-byte aligned; post_scale / post_shift given together or both NULL.
 * Supported (slfp_conv2d_entry_supported: 1 / 0, host only): 1x1, groups 1, any stride the float32 interface takes, both layouts
 * NHWC, C_out a multiple of 16, C_in a multiple of 4, the single-pass operand modes (F16X1 / default, SFP<3,3>), relu 0 or
 * SLFP_POST_RELU, y_qbits 8 or 7, y_ka > 0 with a code table.  Everything else -- F16X3, NCHW, SLFP_POST_LAYEROUT, other channel
 * counts, dense / depthwise / stem layers -- returns SLFP_ERR_UNSUPPORTED.  slfp_conv2d_codes_supported and slfp_conv2d_fwd_codes
 * keep refusing this combination: the two interfaces do not overlap. */
int slfp_conv2d_entry_supported(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int relu);
int slfp_conv2d_fwd_entry(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, const float* x, const void* wprep,
                          const float* bias, const float* post_scale, const float* post_shift, int relu,
                          void* y_codes, void* stream);
/* ---- float32-equivalent (three-pass) mode on codes, for the 1x1 layers of the pw_mfma_f16x3 family -------------------------------
 * slfp_conv2d_fwd_codes_x3 reads the uint8 codes slfp_conv2d_fwd_codes takes (io->x_codes == 1: QA(x / d->ka) as SLFP<3,4> extended
 * codes) and writes float32 (io->y_codes == 0) or the reader's codes (io->y_codes == 1, io->y_ka / io->y_qbits as for
 * slfp_conv2d_fwd_codes) with a descriptor whose mfma_passes is SLFP_MFMA_F16X3.  Each code expands to the hi + lo fp16 pair of its
 * class (hi = fp16(16 v), lo = fp16(16 v - hi)); every 32-deep k-step issues (w_lo, x_hi), (w_hi, x_lo), (w_hi, x_hi) in the order of
 * the float32-interface three-pass kernels and the epilogue is theirs, so the float32 output equals, bit for bit, what
 * slfp_conv2d_fwd_post writes for the same descriptor on the decoded tensor, and the code output is slfp_encode_f32 of that.
 * wprep: the blob of slfp_conv2d_prepare_weights for the same descriptor (both planes), unchanged.  x, y, wprep, bias, post_scale and
 * post_shift 16-byte aligned; post_scale / post_shift given together or both NULL.
 * Supported (slfp_conv2d_codes_x3_supported: 1 / 0, host only): qbits 8 with SLFP_MFMA_F16X3, 1x1, groups 1, stride 1 or 2 as the
 * single-pass kernels take it, both layouts NHWC, no channel re-padding, relu 0 or SLFP_POST_RELU, C_in a multiple of 32 (a multiple
 * of 64 where both planes of W exceed the LDS-resident kernel: C_in / 32 not in {1, 2, 3, 4, 8} or 4 * C_in * C_out(padded to 64) >
 * 128 KiB), C_out a multiple of 4 (float32 out) or 16 (code out); code out needs y_qbits 8 or 7 and y_ka > 0 with a code table.
 * There is no residual, second-output, table-epilogue (SLFP_POST_LAYEROUT), channel-slice, float32-in or C_in = 16 / 48 form: those
 * return SLFP_ERR_UNSUPPORTED and the caller stays on slfp_conv2d_fwd_post.  The older queries and entry points keep refusing
 * three-pass descriptors on 1x1 layers: the interfaces do not overlap.
 * slfp_debug_pwc_x3_variant names what runs ("none" where the query says 0), from the selection the launcher dispatches on:
 *   pwc-stream/ks<KS>/<xw|dw>/act8/<f32|yc>/p3      k_pwc_stream<kFmtAct8, KS, XW, YC, ..., PASSES = 3> (/grid<N> under SLFP_PW_GRID)
 *   pwc-tiled/<WM><WN><MT>/act8/<f32|yc>/p3         k_pwc_tiled<kFmtAct8, WM, WN, MT, YC, ..., PASSES = 3>: 144, 222 or 411 */
int slfp_conv2d_codes_x3_supported(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int relu);
int slfp_conv2d_fwd_codes_x3(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, const void* x, const void* wprep,
                             const float* bias, const float* post_scale, const float* post_shift, int relu,
                             void* y, void* stream);
const char* slfp_debug_pwc_x3_variant(const slfp_conv2d_desc* d, const slfp_conv2d_io* io);
/* ---- residual operand: y = relu?(affine(conv(x)) + res) in ONE launch -------------------------------------------------
 * The tail of every residual block, out = relu(bn3(conv3(h)) + identity) (nets_imgnet/resnet50.py:82-88), for the 1x1
 * stride-1 layers of the pw_mfma_* family.  Per output element, in this order, every step rounded to float32:
 *     r = the conv result with the reference's (out * Ka) * Kw roundings, exactly as slfp_conv2d_fwd_post computes it
 *     t = fma(r, post_scale[c], post_shift[c])      when post_scale / post_shift are given
 *     t = t + res[i]                                one float32 add; res is indexed like y
 *     y[i] = (relu & SLFP_POST_RELU) ? max(t, 0) : t
 * which is what slfp_conv2d_fwd_post(relu = 0) followed by a float32 add and a ReLU pass computes: the result is
 * bit-identical to that sequence on NaN-free data, with 8 B per output element through HBM instead of 24.
 * io->x_codes 0 / 1: x is float32, or the uint8 codes slfp_conv2d_fwd_codes takes; io->y_codes must be 0.  res and y: float32
 * NHWC tensors of the output shape, 16-byte aligned, not overlapping (SLFP_ERR_BAD_ARG otherwise).  Supported: 1x1, stride 1,
 * groups 1, both layouts NHWC, C_in and C_out multiples of 4, in the F16X1, F16X3 and SFP<3,3> operand modes with float32
 * input, and wherever slfp_conv2d_codes_supported says yes with code input.  Everything else -- dense, depthwise and stem
 * layers, strided 1x1, NCHW, SLFP_POST_LAYEROUT, y_codes -- returns SLFP_ERR_UNSUPPORTED.  `workspace` is reserved (no
 * supported layer needs one; pass NULL).  slfp_conv2d_res_supported answers 1 / 0 without device work. */
int slfp_conv2d_res_supported(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int relu);
int slfp_conv2d_fwd_res(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, const void* x, const void* wprep,
                        const float* bias, const float* post_scale, const float* post_shift, int relu,
                        const float* res, float* y, void* workspace, void* stream);
/* ---- the residual epilogue also writes the next block's codes ------------------------------------------------------------
 * slfp_conv2d_fwd_res on codes (io->x_codes == 1) with a second output: y is written exactly as slfp_conv2d_fwd_res writes it for
 * the same arguments with io->y_codes = 0, and y_codes (uint8 NHWC, C_out bytes per pixel) receives, per element, the byte
 *     slfp_encode_f32(y, io->y_ka, fmt(io->y_qbits) | SLFP_FMT_EXT)
 * of that y -- in the same launch, from the value the kernel holds after the add and the ReLU: the float32 trunk of a ResNet
 * goes on to the next block's residual add, its codes to the next block's conv1 (and downsample.0), which then never read the
 * float32 tensor.  Both hold for every input, NaN, +-inf and -0.0 in res included (NaN has no code: 0x00).  Requires
 * io->x_codes == 1 and io->y_codes == 1 (y_ka / y_qbits describe the reader of y_codes); y_codes non-NULL, 16-byte aligned and not
 * overlapping y or res (SLFP_ERR_BAD_ARG / SLFP_ERR_ALIGNMENT as for y).  Supported (slfp_conv2d_res_codes_supported: 1 / 0, host
 * only) exactly where slfp_conv2d_res_supported says yes for {x_codes = 1, y_codes = 0}, C_out is a multiple of 16 and the reader's
 * quantizer is valid (y_qbits 8 or 7, y_ka > 0 with a code table).  Everything else -- float32 input, SLFP_POST_LAYEROUT, NCHW,
 * strided, dense, depthwise and stem layers, F16X3 at qbits 8 -- returns SLFP_ERR_UNSUPPORTED before any device work.
 * slfp_conv2d_res_supported keeps refusing y_codes.  `workspace` is reserved; pass NULL. */
int slfp_conv2d_res_codes_supported(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int relu);
int slfp_conv2d_fwd_res_codes(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, const void* x, const void* wprep,
                              const float* bias, const float* post_scale, const float* post_shift, int relu,
                              const float* res, float* y, void* y_codes, void* workspace, void* stream);

/* ---- codes behind the layer-output quantizer: the activation as a byte table ------------------------------------------------
 * The blocks of MobileNetV1_swish / VGG16_gelu are [Conv2d_Q, BatchNorm2d, layerout_quantize_func, ReLU | Swish | GELU]
 * (nets_cifar/mobilenetv1.py:196-231, nets_cifar/vgg16.py:186-293).  After the layer-output quantizer a float32 has 5 significant
 * bits and |v| <= 248: slfp_layerout_lut_classes() values in all (NaN, which the quantizer returns for an exact zero, is one of
 * them).  Whatever lies between that value and the next layer's code -- a ReLU, any elementwise activation module, the reader's
 * quantize_act(. / Ka) -- is a function of it, so slfp_conv2d_fwd_codes_lut stores, per output element, the byte
 *     lut[class(layerout(fma(r, post_scale[c], post_shift[c])))]
 * with r exactly what slfp_conv2d_fwd_post computes, layerout = slfp_quantize_layerout_f32 and class the index documented in
 * csrc/slfp_layerout_lut.hpp.  The caller builds the table: slfp_layerout_lut_values gives the float32 value of every index
 * (index 0: NaN; indices from slfp_layerout_lut_classes() on: padding, 0), the caller applies the activation and
 * slfp_encode_f32(., Ka, fmt | SLFP_FMT_EXT) to them (fusion.link_layerout).  The result is then bit-identical to
 * slfp_conv2d_fwd_post(relu = SLFP_POST_LAYEROUT) + activation + slfp_encode_f32 for ANY elementwise activation.
 * lut: device memory, SLFP_LAYEROUT_LUT_BYTES bytes, 16-byte aligned.  io->y_codes must be 1, io->x_codes 0 or 1 as the layer's
 * family allows on slfp_conv2d_fwd_codes; io->y_ka / y_qbits are validated as there, though the kernel reads only the table.
 * post_scale / post_shift are required.  y_ld == C_out: a dense code tensor; otherwise a channel slice under the rules of
 * slfp_conv2d_fwd_codes_slice.  workspace: as slfp_conv2d_fwd_codes_ws.
 * Supported (slfp_conv2d_codes_lut_supported: 1 / 0, host only): 3x3 depthwise on codes, 1x1 on codes (C_in 32 / 64 / 128 / 256
 * and, with C_out > 256, the multiples of 64 above), dense 3x3 stride 1 (codes or float32 in) and the two 3x3 RGB stems
 * (3 -> 32 stride 2, 3 -> 64 stride 1; float32 in) -- the layers of the two nets above.  The residual forms, the entry kernel
 * and the large-kernel stems have no table form: SLFP_ERR_UNSUPPORTED.  The older entry points keep refusing SLFP_POST_LAYEROUT.
 * slfp_layerout_lut_index (host): the index of a value of the quantizer, -1 for any other float32.
 * slfp_debug_layerout_lut_mismatches sweeps ALL 2^32 float32 inputs on the device: *out1 (device memory) = inputs whose
 * layer-output value differs in bits from the value of its class (all NaNs counted as equal).  Must be 0. */
#define SLFP_LAYEROUT_LUT_BYTES 4928
int slfp_layerout_lut_classes(void);
int slfp_layerout_lut_values(float* out, int n);
int slfp_layerout_lut_index(float v);
int slfp_conv2d_codes_lut_supported(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int64_t y_ld);
int slfp_conv2d_fwd_codes_lut(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, const void* x, const void* wprep,
                              const float* bias, const float* post_scale, const float* post_shift, const uint8_t* lut, void* y,
                              int64_t y_ld, void* workspace, void* stream);
int slfp_debug_layerout_lut_mismatches(unsigned long long* out1, void* stream);

/* ---- Image stems that read uint8 pixels ----
 * A decoded image is HWC bytes; ToTensor() + Normalize(mean, std) -- or any per-channel elementwise preprocessing -- maps byte v of
 * channel c to one of 256 float32 values, pix_table[c][v].  slfp_conv2d_fwd_u8 takes the bytes and that table.
 * Contract: the result is bit for bit what the matching float32 entry point (slfp_conv2d_fwd_post, or slfp_conv2d_fwd_codes[_ws]
 * with io->y_codes == 1) returns for the float32 tensor x32[n,h,w,c] = pix_table[c][x[n,h,w,c]], from the same kernel instance
 * family, the same prepared blob (slfp_conv2d_prepare_weights) and the same epilogue.  Each workgroup applies the kernel's own
 * per-element encode to the 256 * C_in table entries once (LDS) and the fill step becomes a byte load and a lookup; a padded tap
 * contributes the operand +0 as before (not pix_table[c][0]); NaN / inf entries follow the float32 kernels' rules.
 *   x          NHWC bytes, N*H*W*C_in, dense, ANY byte alignment (plain byte loads; nothing outside [x, x + N*H*W*C_in) is read)
 *   pix_table  device float32 [C_in][256], 16-byte aligned
 *   io         NULL or io->y_codes == 0: float32 out, post_flags as slfp_conv2d_fwd_post (SLFP_POST_LAYEROUT included);
 *              io->y_codes == 1: the reader's codes (ReLU folded, or signed), y_qbits 8 or 7
 *   workspace  as the float32 entry point of the layer (slfp_conv2d_workspace_bytes); NULL where that is 0
 * Supported (slfp_conv2d_u8_supported: 1 / 0, host only): the 3x3 s2 3 -> 32 stem on k_stem_fixed's threshold-table form (the byte
 * entry sends k_stem_mx's geometry there too: both equal the CPU restatement bit for bit), the small-K matrix-core stems
 * (k_stem_small) and the large-kernel stems (k_stem_rows; k_stem_im2row's pre-pass reads the bytes).  Refused with
 * SLFP_ERR_UNSUPPORTED before any device work: io->x_codes == 1, the table epilogue, SLFP_POST_LAYEROUT with code output, NCHW on
 * either side, groups != 1, C_in > 4, every layer whose float32 form runs k_direct, the generic k_stem or k_stem_fixed without a
 * threshold table, and qbits 8 with SLFP_MFMA_F16X3.  NULL x / pix_table / y / wprep: SLFP_ERR_BAD_ARG.
 * slfp_debug_stem_u8_instance: the instance the launch consumes, from the same selection, in slfp_debug_stem_instance's grammar
 * with a `u8` word in front of the output form ("stem/fixed/tab/u8/yc", "small/nt4/act8/u8/f32", "rows/nt6/sfp7/u8/yc-signed",
 * "im2row/nt4/act8/u8/f32"); "none" where the query says 0.
 * slfp_image_u8_expand_f32: y[p][c] = pix_table[c][x[p][c]] for n_pixels pixels of c = 1..4 channels in one pass (x: any alignment;
 * y: 16-byte aligned, 16-byte stores) -- the float32 tensor of the contract above, for every layer without a byte form and for
 * training. */
int slfp_conv2d_u8_supported(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int post_flags);
int slfp_conv2d_fwd_u8(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, const uint8_t* x, const float* pix_table,
                       const void* wprep, const float* bias, const float* post_scale, const float* post_shift,
                       int post_flags, void* y, void* workspace, void* stream);
const char* slfp_debug_stem_u8_instance(const slfp_conv2d_desc* d, const slfp_conv2d_io* io, int has_bias, int post_flags, int has_post);
int slfp_image_u8_expand_f32(const uint8_t* x, const float* pix_table, float* y, int64_t n_pixels, int c, void* stream);

/* nn.MaxPool2d (floor mode, dilation 1) on a tensor of activation codes (NHWC, C a multiple of 4; 16-byte aligned): the class
 * of a window's largest input is the highest class among its codes in the order of the classes' pre-images (the clamp literal
 * of Qbits 8 ranks above the top regular code, "tiny" above exact zero, signed codes by decreasing magnitude), so
 * y == slfp_encode_f32(max_pool2d(t), ka, fmt | SLFP_FMT_EXT) wherever x == slfp_encode_f32(t, ka, fmt | SLFP_FMT_EXT), bit for
 * bit -- the pools between VGG-16's stages (nets_cifar/vgg16.py:39,49,63,78,92) can stay inside a code chain. */
int slfp_maxpool2d_codes(const uint8_t* x, uint8_t* y, int64_t n, int64_t h, int64_t w, int64_t c, int kh, int kw, int sh, int sw,
                         int ph, int pw, int qbits, void* stream);
/* The same with nn.MaxPool2d's ceil_mode (0 / 1; SqueezeNet's three pools, nets_imgnet/squeezenet1_0.py:60-71): with 1 the
 * output size per axis is ceil((in + 2 p - k) / s) + 1, minus one if the last window would start past the input and its left
 * padding -- ATen's rule; windows that hang over the edge take the maximum of the taps inside the image.  ceil_mode == 0 is
 * slfp_maxpool2d_codes.  slfp_maxpool2d_out_shape answers the size on the host (SLFP_ERR_SHAPE: bad geometry). */
int slfp_maxpool2d_codes_ex(const uint8_t* x, uint8_t* y, int64_t n, int64_t h, int64_t w, int64_t c, int kh, int kw, int sh, int sw,
                            int ph, int pw, int qbits, int ceil_mode, void* stream);
int slfp_maxpool2d_out_shape(int64_t h, int64_t w, int kh, int kw, int sh, int sw, int ph, int pw, int ceil_mode, int64_t* h_out,
                             int64_t* w_out);
/* Self-check of the producer side: sweeps ALL 2^32 float32 inputs on the device; out3[0] = inputs whose table-driven code
 * (enc4_code_fmt, signed variant) differs from slfp_encode_f32(.., fmt | SLFP_FMT_EXT), out3[1] = the same for its unsigned
 * variant (inputs >= +0 and -0; the callers apply the sign themselves), out3[2] = code bytes whose decode-table entries (float32
 * and fp16 operand) differ from slfp_decode_f32.  All three must be 0.  fmt: SLFP_FMT_ACT8 or SLFP_FMT_SFP7.  The encoder with the
 * ReLU folded in, which the ReLU-epilogue producers run, is swept by slfp_debug_code_relu_mismatches. */
int slfp_debug_code_mismatches(float scale_div, int fmt, unsigned long long* out3, void* stream);
/* The same sweep for the ReLU-folded encoder (enc4_code_relu: the depthwise code kernel, the tile epilogue, the stems, the dense
 * epilogue): out2[0] = inputs x whose code differs from the extended code of max(x, 0) -- NaN gives 0x00 as slfp_encode_f32 does;
 * -0, negatives and -inf give the code of exact zero; out2[1] = the same behind relu_of_nan4 and for the encoder's own NaN-to-zero
 * form (the forms the kernels run), where a NaN gives the code of exact zero as well.  Both must be 0. */
int slfp_debug_code_relu_mismatches(float scale_div, int fmt, unsigned long long* out2, void* stream);

/* ---- linear: replaces Linear_Q.forward (utils/conv2d_func.py:60-65) -------------------
 * out = linear(QA(x/Ka), QW(w/Kw), bias/Kw/Ka) * Kw * Ka   (note the Kw-first order).
 * x: [batch, in_f] row-major, w: [out_f, in_f] row-major, bias: [out_f] or NULL.  The weights
 * are re-quantized on every call (as the reference does) into `workspace`
 * (slfp_linear_workspace_bytes bytes of device memory).                                   */
size_t slfp_linear_workspace_bytes(int64_t batch, int64_t in_f, int64_t out_f);
int slfp_linear_fwd(const float* x, const float* w, const float* bias, float* y, int64_t batch,
                    int64_t in_f, int64_t out_f, float ka, float kw_scale, int qbits, int mfma_passes,
                    void* workspace, void* stream);
/* The same with the weights quantized ONCE (inference: AlexNet's 9216x4096 and VGG-16's 25088x4096
 * fully-connected layers would otherwise be re-encoded on every forward):
 * slfp_linear_prepare_weights fills `wprep` (slfp_linear_workspace_bytes(1, in_f, out_f) bytes; the
 * blob depends on kw_scale, qbits and mfma_passes, not on the batch), slfp_linear_fwd_prepared
 * consumes it.  slfp_linear_fwd == prepare + fwd_prepared on the caller's workspace. */
int slfp_linear_prepare_weights(const float* w, void* wprep, int64_t in_f, int64_t out_f, float kw_scale,
                                int qbits, int mfma_passes, void* stream);
int slfp_linear_fwd_prepared(const float* x, const void* wprep, const float* bias, float* y, int64_t batch,
                             int64_t in_f, int64_t out_f, float ka, float kw_scale, int qbits,
                             int mfma_passes, void* stream);

/* ---- linear on 1-byte codes: the weight-streaming kernel (csrc/linear_fc.hip) ----------------------------------------
 * Linear_Q.forward (utils/conv2d_func.py:60-65) for classifier layers, whose cost is the stream of W rather than of the
 * activations: one wave per workgroup owns 1, 2 or 4 of the blob's 16-channel tiles and 16, 32 or 64 rows and streams its share of W
 * (the blob of slfp_linear_prepare_weights, unchanged) straight into registers with two chunks of k-steps in flight; the grid is
 * sized from (batch, out_f) so that it covers the compute units wherever out_f allows, and is never split over in_f.
 *   io->x_codes 0: x is float32 [batch, in_f]; it is encoded once -- slfp_encode_f32(x, ka, fmt(qbits) | SLFP_FMT_EXT) -- into
 *                  `workspace` (slfp_linear_fc_workspace_bytes bytes of device memory)
 *   io->x_codes 1: x holds those codes, as for slfp_conv2d_fwd_codes; `workspace` may be NULL (0 bytes)
 *   io->y_codes 0: y is float32 [batch, out_f]:  t = linear(QA(x/Ka), QW(w/Kw), bias/Kw/Ka) * Kw * Ka, bit for bit what
 *                  slfp_linear_fwd_prepared writes for the same arguments;  y = (relu & SLFP_POST_RELU) ? max(t, 0) : t
 *   io->y_codes 1: y is uint8 [batch, out_f] = slfp_encode_f32(that y, io->y_ka, fmt(io->y_qbits) | SLFP_FMT_EXT): what the
 *                  Linear_Q behind this one (its Ka, its q_bit) reads with x_codes = 1
 * relu: 0 or SLFP_POST_RELU.  x, wprep, y, bias and workspace 16-byte aligned.  Supported (slfp_linear_fc_supported: 1 / 0, host
 * only): qbits 8 in the single-pass operand modes (SLFP_MFMA_DEFAULT / SLFP_MFMA_F16X1) and qbits 7, in_f a multiple of 32, out_f a
 * multiple of 4 (of 16 with y_codes), batch >= 1, y_qbits 8 or 7 and y_ka > 0 with a code table.  Everything else -- SLFP_MFMA_F16X3
 * at qbits 8, feature counts that take the direct kernel, other qbits -- returns SLFP_ERR_UNSUPPORTED before any device work.  NaN
 * inputs are outside the bit-identity: codes have no NaN (slfp_encode_f32 gives 0x00), the float32 interface propagates it.
 * slfp_debug_linear_fc_tiles(n_tiles, row_tiles) forces the 16-channel tiles / 16-row tiles per workgroup (1, 2 or 4 each; 0: the
 * rule): measurements only (profiles/linear_fc_bench.py).  The switch is process-wide, not scoped to a thread or a stream: it changes
 * the tiling (never the result) of every later slfp_linear_fwd_fc call on every thread until it is set again, so a caller resets it
 * with slfp_debug_linear_fc_tiles(0, 0) when the measurement is done. */
int slfp_linear_fc_supported(int64_t batch, int64_t in_f, int64_t out_f, int qbits, int mfma_passes,
                             const slfp_conv2d_io* io, int has_bias, int relu);
size_t slfp_linear_fc_workspace_bytes(int64_t batch, int64_t in_f, int64_t out_f, const slfp_conv2d_io* io);
int slfp_linear_fwd_fc(const void* x, const void* wprep, const float* bias, void* y, int64_t batch, int64_t in_f,
                       int64_t out_f, float ka, float kw_scale, int qbits, int mfma_passes,
                       const slfp_conv2d_io* io, int relu, void* workspace, void* stream);
int slfp_debug_linear_fc_tiles(int n_tiles, int row_tiles);

/* ---- global average pool (csrc/pool_avg.hip) -------------------------------------------------------------------------
 * The pool between the last convolution and the classifier: nn.AdaptiveAvgPool2d((1, 1)) -> flatten -> Linear_Q
 * (nets_imgnet/resnet50.py:146-147, 244-245), nn.AdaptiveAvgPool2d(1) -> view(-1, 1024) -> Linear_Q
 * (nets_cifar/mobilenetv1.py:62-86, 248-272), nn.AvgPool2d(7) on a 7 x 7 map (nets_imgnet/mobilenetv1.py:58) and conv -> ReLU ->
 * nn.AdaptiveAvgPool2d((1, 1)) (nets_imgnet/squeezenet1_0.py:85).
 *   y[n, c] = mean over the h * w pixels of x[n, :, :, c],   x float32 in x_layout (SLFP_LAYOUT_NHWC or SLFP_LAYOUT_NCHW).
 * The summation runs in float32 in ONE fixed order, which is part of this interface:
 *   p   = row * w + col                        the row-major pixel index, 0 .. h * w - 1
 *   v_p = relu ? max(x_p, 0) : x_p
 *   s_j = the sum of v_p over p == j (mod 4), p ascending, each s_j starting from +0.0f        (j = 0, 1, 2, 3)
 *   y   = ((s_0 + s_1) + (s_2 + s_3)) / (float)(h * w)          IEEE float32 division, not a multiply by a reciprocal
 * so a row of y is a pure function of one image's values: the same bits whatever n, the grid, the stream or the layout (the two
 * layouts give the same bits for the same values).  No atomics.
 *   io->y_codes 0: y is float32 [n, c]
 *   io->y_codes 1: y is uint8 [n, c] = slfp_encode_f32(that float32 y, io->y_ka, fmt(io->y_qbits) | SLFP_FMT_EXT): what the
 *                  Linear_Q behind the pool (its Ka, its q_bit) reads with x_codes = 1; signed classes, no ReLU behind the pool
 * io->x_codes must be 0; relu is 0 or 1.  Supported (slfp_global_avgpool_supported: 1 / 0, host only): h, w >= 1, c >= 1; NHWC
 * needs c a multiple of 4 and 16-byte aligned x and y; NCHW takes any c and 4-byte alignment; code output needs c a multiple of
 * 4, y_qbits 8 or 7 and y_ka > 0 with a code table.  Null (SLFP_ERR_BAD_ARG), shape (SLFP_ERR_SHAPE), unsupported
 * (SLFP_ERR_UNSUPPORTED) and alignment (SLFP_ERR_ALIGNMENT) refusals happen before any device work and leave y untouched; n == 0
 * returns SLFP_OK.  NaN inputs are outside the code contract, as in slfp_linear_fwd_fc. */
int slfp_global_avgpool_supported(int64_t n, int64_t h, int64_t w, int64_t c, int x_layout, const slfp_conv2d_io* io);
int slfp_global_avgpool_f32(const float* x, void* y, int64_t n, int64_t h, int64_t w, int64_t c, int x_layout, int relu,
                            const slfp_conv2d_io* io, void* stream);

/* ---- training-mode BatchNorm2d (+ReLU), forward and backward (csrc/bn_train.hip) ---------------------------------------
 * The nn.BatchNorm2d behind every Conv2d_Q of the training nets and the nn.ReLU(inplace=True) that mostly follows it
 * (nets_cifar/mobilenetv1.py:30-45, nets_imgnet/mobilenetv1.py:24-41), in training mode: batch statistics, the running
 * statistics' update, and the gradients.  float32, x_layout SLFP_LAYOUT_NHWC only: x, y, gy, gx are [M][c] with M = n * h * w
 * rows; any c >= 1 (c % 4 == 0: 16-byte accesses; otherwise 4-byte ones).  Contiguous NCHW is not built.
 * No atomics.  Every result is a pure function of the inputs and of (M, c); two calls give the same bits.  The summation
 * contract (every operation float32 and rounded on its own unless float64 is named):
 *   split      slfp_debug_bn_split(M, c) cuts the rows into S <= 1024 slabs of R rows, R (S - 1) < M <= R S, the last one
 *              ragged.  With V = 4 if c % 4 == 0 else 1, TX = the power of two >= min(c / V, 64) and TY = 256 / TX, lane ty
 *              of a slab that begins at row r0 owns rows r0 + ty, r0 + ty + TY, ...
 *   statistics k = x[r0], the slab's first row.  Per lane, from +0.0f, rows ascending:  d = x - k;  s1 = s1 + d;
 *              s2 = s2 + d * d.  The lanes' partials are added ty = 0, 1, ..., TY - 1: one (count, k, s1, s2) per (slab, channel).
 *              (The shift by k keeps the variance where |mean| >> sigma, which a plain E[x^2] - E[x]^2 loses.)
 *   finalize   in float64, per slab  mean_b = k + s1 / n_b,  M2_b = s2 - s1 * s1 / n_b,  then Chan's formula in slab order
 *              with n_a rows in front:  n = n_a + n_b;  delta = mean_b - mean;  mean = mean + delta * (n_b / n);
 *              M2 = (M2 + M2_b) + (delta * delta) * (n_a * n_b / n).   var = M2 / M (biased), or 0 where rounding left it below 0.
 *              save_mean = f32(mean);  save_invstd = f32(1 / sqrt(var + eps)), computed in float64 and rounded once;
 *              lo = f32(mean - save_mean), the part of the mean that float32 cannot hold (kept in the workspace).
 *              running_mean = f32((1 - momentum) * running_mean + momentum * mean) and running_var = f32((1 - momentum) *
 *              running_var + momentum * (var * M / (M - 1))) in float64, in place; both NULL: no update.
 *   apply      sc = save_invstd * gamma;  y = (((x - save_mean) - lo) * sc) + beta;  relu: y = y < 0 ? 0 : y  (a NaN stays a
 *              NaN).  x - save_mean is exact for x within a factor 2 of the mean, so y keeps float32 accuracy relative to the
 *              centred value where |mean| >> sigma.
 *   backward   g = relu ? (y > 0 ? gy : 0) : gy  -- the mask is read from the forward's own output y, never recomputed from x.
 *              Per lane, from +0.0f, rows ascending:  d = x - save_mean;  sg = sg + g;  sx = sx + g * (d * save_invstd);
 *              sd = sd + d;  lanes added as above; the slabs' sums are added in slab order in float64 to SG, SX, SD.
 *              lo = SD / M is what the float32 save_mean lost of the mean;  SX = SX - (lo * save_invstd) * SG, the sum of g * xh
 *              for xh = ((x - save_mean) - lo) * save_invstd.   gbeta = f32(SG),  ggamma = f32(SX),  mb = f32(SG / M),
 *              mg = f32(SX / M).   a = gamma * save_invstd;  gx = a * ((g - mb) - (xh * mg))  with lo rounded to float32.
 *              ggamma and gbeta may be NULL (not needed); the sums are computed all the same, gx needs them.
 * relu is 0 or 1; with relu == 0 the backward does not read y (it must still be a valid pointer).  y may not alias x, gx neither
 * x nor y.  workspace: slfp_bn_train_workspace_bytes(n, h, w, c) bytes, 16-byte aligned, the same for both directions; its
 * contents need not survive from the forward to the backward.  Supported (slfp_bn_train_supported: 1 / 0, host only): NHWC,
 * h, w, c >= 1, M < 2^31, c <= 2^21, and M != 1 -- one value per channel has no variance ("Expected more than 1 value per
 * channel").  Refusals happen before any device work and leave the outputs untouched: null pointers, a bad layout enum or relu
 * (SLFP_ERR_BAD_ARG), bad geometry (SLFP_ERR_SHAPE), NCHW or M == 1 (SLFP_ERR_UNSUPPORTED), pointers not aligned to 16 bytes
 * (c % 4 == 0) or 4 bytes (SLFP_ERR_ALIGNMENT), a workspace that is NULL, misaligned or smaller than required
 * (SLFP_ERR_BAD_ARG, as the conv workspace).  n == 0 returns SLFP_OK.
 * slfp_bn_train_supported answers what the kernels can run, not what is worth running: measured against MIOpen's BatchNorm and
 * ATen's ReLU (profiles/bn_train_bench.json), forward + backward of tensors of fewer than about 16 M elements was not reliably
 * faster, and below 3.2 M elements slower; a caller of this interface gets 1 for those shapes all the same and applies a size rule
 * of its own, as the Python module does (batchnorm.MIN_ELEMENTS). */
int slfp_bn_train_supported(int64_t n, int64_t h, int64_t w, int64_t c, int x_layout);
size_t slfp_bn_train_workspace_bytes(int64_t n, int64_t h, int64_t w, int64_t c);
int slfp_bn_train_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                      float momentum, float eps, int relu, float* y, float* save_mean, float* save_invstd, int64_t n, int64_t h,
                      int64_t w, int64_t c, int x_layout, void* workspace, size_t ws_bytes, void* stream);
int slfp_bn_train_bwd(const float* x, const float* y, const float* gy, const float* gamma, const float* save_mean,
                      const float* save_invstd, int relu, float* gx, float* ggamma, float* gbeta, int64_t n, int64_t h, int64_t w,
                      int64_t c, int x_layout, void* workspace, size_t ws_bytes, void* stream);
/* host only: the split above for M = m rows of c channels (SLFP_ERR_SHAPE: m < 1 or c < 1 or beyond the supported range) */
int slfp_debug_bn_split(int64_t m, int64_t c, int64_t* rows_per_slab, int64_t* slabs);

/* ---- training-mode BatchNorm2d -> layer-output quantizer -> activation (csrc/bn_train.hip, the LUT forms) ------------------
 * The tail [BatchNorm2d, layerout_quantize_func, ReLU | Swish | GELU] of the training blocks of MobileNetV1_swish / VGG16_gelu
 * (nets_cifar/mobilenetv1.py:196-231, nets_cifar/vgg16.py:186-293), in training mode.  Behind the SFP<4,4> layer-output quantizer
 * a value is one of slfp_layerout_lut_classes() classes, so an elementwise activation is a float32 table over the class index and
 * its derivative another.  act_table, dact_table: device memory, SLFP_LAYEROUT_TABLE_FLOATS float32 each, 16-byte aligned; index i
 * is the class of slfp_layerout_lut_values / layerout_class (csrc/slfp_layerout_lut.hpp), index 0 the NaN class; the caller
 * builds both (act_table[i] = act(value_i), dact_table[i] = act'(value_i)).  The contract is exact:
 *   statistics save_mean, save_invstd and the running statistics are exactly those of slfp_bn_train_fwd on the same x: the same
 *              split, the same sums, the same finalize.  save_lo[c] = lo = f32(mean - save_mean), which slfp_bn_train_fwd keeps
 *              in its workspace, is an output here: the backward must reproduce the forward's values bit for bit.
 *   forward    t = (((x - save_mean) - save_lo) * (save_invstd * gamma)) + beta, the apply above with relu = 0;
 *              q = layerout_bits(t), what slfp_quantize_layerout_f32 computes;  y = act_table[layerout_class(q)].  So y is
 *              bit-identical to slfp_bn_train_fwd(relu = 0), then slfp_quantize_layerout_f32, then a gather from the table.
 *              The apply pass reads x once and writes y once.
 *   backward   the class of every element is recomputed from x, gamma, beta, save_mean, save_invstd and save_lo with the
 *              forward's expression; a saved y is never read (Swish and GELU are not injective: the class is what matters).
 *              g = gy * dact_table[class], one float32 multiply (the quantizer is a straight-through estimator: it passes the
 *              gradient unchanged).  From there on gx, ggamma and gbeta are bit-identical to slfp_bn_train_bwd(relu = 0) called
 *              with g in place of gy, the lo it recovers itself from SD / M included.  ggamma and gbeta may be NULL.  The
 *              reduce pass reads x and gy; the dx pass reads x and gy and writes gx.
 * No atomics; two calls give the same bits.  A NaN or an inf stays in its channel (a NaN's class is 0, an inf's +-248).  The
 * denormal branch of layerout_class stays a cold branch.  Both take the supported set of slfp_bn_train_supported and the
 * workspace of slfp_bn_train_workspace_bytes, and make the refusals of slfp_bn_train_fwd / slfp_bn_train_bwd in the same order
 * before any device work; save_lo counts among the per-channel arrays, a NULL act_table, dact_table or save_lo is
 * SLFP_ERR_BAD_ARG and a table address not aligned to 16 bytes SLFP_ERR_ALIGNMENT (after the per-channel arrays').  y may not
 * alias x, gx not x. */
#define SLFP_LAYEROUT_TABLE_FLOATS SLFP_LAYEROUT_LUT_BYTES   /* 4928 */
int slfp_bn_lut_train_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                          float momentum, float eps, const float* act_table, float* y, float* save_mean, float* save_invstd,
                          float* save_lo, int64_t n, int64_t h, int64_t w, int64_t c, int x_layout,
                          void* workspace, size_t ws_bytes, void* stream);
int slfp_bn_lut_train_bwd(const float* x, const float* gy, const float* gamma, const float* beta, const float* save_mean,
                          const float* save_invstd, const float* save_lo, const float* dact_table, float* gx,
                          float* ggamma, float* gbeta, int64_t n, int64_t h, int64_t w, int64_t c, int x_layout,
                          void* workspace, size_t ws_bytes, void* stream);

/* ---- training-mode BatchNorm2d -> residual add -> ReLU (csrc/bn_train.hip, the residual forms) -----------------------------
 * The tail of a Bottleneck, out = bn3(out); out += identity; out = relu(out) (nets_imgnet/resnet50.py:85-90), in training mode,
 * in the two passes slfp_bn_train_fwd / _bwd already make over the tensor.  res: the identity, float32 [M][c] like x.  The
 * contract is exact:
 *   statistics save_mean, save_invstd and the running statistics are exactly those of slfp_bn_train_fwd on the same x: the same
 *              split, the same sums, the same finalize.
 *   forward    t = (((x - save_mean) - lo) * (save_invstd * gamma)) + beta, the apply above with relu = 0;  z = t + res, one
 *              float32 add rounded on its own;  relu: y = z < 0 ? 0 : z  (a NaN stays a NaN);  otherwise y = z.  So y is
 *              bit-identical to slfp_bn_train_fwd(relu = 0), then a float32 add of res, then where(z < 0, 0, z).  The apply pass
 *              reads x and res once and writes y once.
 *   backward   g = relu ? (y > 0 ? gy : 0) : gy  with y the forward's own output (behind the add and the ReLU).  gx, ggamma
 *              and gbeta are bit-identical to slfp_bn_train_bwd(relu) given the same x, y, gy.  gres = g, the residual's
 *              gradient, is a second store of the dx pass; gres == NULL: not needed, the store is skipped and nothing else
 *              changes.  ggamma and gbeta may be NULL.  The reduce pass reads x, gy and (relu) y; the dx pass reads the same
 *              and writes gx and gres.
 * No atomics; two calls give the same bits; a NaN or an inf in res stays in its own element of y.  Both take the supported set
 * of slfp_bn_train_supported and the workspace of slfp_bn_train_workspace_bytes (no more), and make the refusals of
 * slfp_bn_train_fwd / slfp_bn_train_bwd in the same order before any device work; res counts among the big arrays (NULL:
 * SLFP_ERR_BAD_ARG; not aligned to 16 bytes (c % 4 == 0) or 4 bytes: SLFP_ERR_ALIGNMENT), a misaligned gres is
 * SLFP_ERR_ALIGNMENT (behind the workspace check, with ggamma / gbeta).  y may alias neither x nor res; gx and gres may alias
 * neither each other nor x, y or gy.  n == 0 returns SLFP_OK. */
int slfp_bn_res_train_fwd(const float* x, const float* res, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, float momentum, float eps, int relu,
                          float* y, float* save_mean, float* save_invstd,
                          int64_t n, int64_t h, int64_t w, int64_t c, int x_layout,
                          void* workspace, size_t ws_bytes, void* stream);
int slfp_bn_res_train_bwd(const float* x, const float* y, const float* gy, const float* gamma,
                          const float* save_mean, const float* save_invstd, int relu,
                          float* gx, float* gres, float* ggamma, float* gbeta,
                          int64_t n, int64_t h, int64_t w, int64_t c, int x_layout,
                          void* workspace, size_t ws_bytes, void* stream);

/* ---- training-mode BatchNorm2d (+ReLU) that writes the next Conv2d_Q's codes (csrc/bn_train.hip, the code forms) -------------
 * In conv -> BN -> ReLU -> conv (nets_imgnet/mobilenetv1.py:24-41) the next Conv2d_Q's first act is quantize_act(y / Ka)
 * (utils/conv2d_func.py:21), a pure function of y; its weight gradient reads the same quantized value (the quantizers are
 * straight-through estimators without a clipping mask, utils/sfp_quant.py:50-53, 99-102); and the BatchNorm backward needs of y
 * only the ReLU's mask.  So the forward stores, instead of the float32 y, one byte per element: the extended code of the reader's
 * quantizer (y_ka its Ka, y_qbits its q_bit, 8 or 7), and the backward recomputes the mask from x.  The contract is exact:
 *   statistics save_mean, save_invstd and the running statistics are exactly those of slfp_bn_train_fwd on the same x: the same
 *              split, the same sums, the same finalize.  save_lo[c] = f32(mean - save_mean) is an output, as in the LUT form.
 *   forward    t = (((x - save_mean) - save_lo) * (save_invstd * gamma)) + beta, then relu: t < 0 ? 0 : t -- the y of
 *              slfp_bn_train_fwd, bit for bit.  y_codes[i] = the byte slfp_encode_f32(y, y_ka, fmt(y_qbits) | SLFP_FMT_EXT) gives
 *              element i, through the reader's threshold table (slfp_enc_table_ok(y_ka, fmt) must hold).  A NaN takes code 0x00,
 *              as everywhere on the code path: the reader sees the tiny class where the float32 interface would hand it the NaN
 *              (save_mean, save_invstd and the running statistics are NaN in the same places as in the plain form).  The apply
 *              pass reads x once and writes one byte per element, a lane's four channels as one dword.
 *   backward   g = relu ? (t > 0 ? gy : 0) : gy  with t recomputed from x, gamma, beta, save_mean, save_invstd and save_lo by the
 *              forward's own expression; y > 0 holds exactly where t > 0, and no forward output is read.  From there gx, ggamma
 *              and gbeta are bit-identical to slfp_bn_train_bwd(relu) given the plain forward's y.
 *              ggamma and gbeta may be NULL.  The reduce pass reads x and gy; the dx pass reads x and gy and writes gx.
 * No atomics; two calls give the same bits; a NaN or an inf stays in its channel.  Supported (slfp_bn_codes_train_supported: 1 / 0,
 * host only): the set of slfp_bn_train_supported, and in addition c % 4 == 0, y_qbits 8 or 7, y_ka > 0 with a proven code table;
 * everything else is SLFP_ERR_UNSUPPORTED (the backward, which is not told the reader, refuses c % 4 != 0).  Both take the
 * workspace of slfp_bn_train_workspace_bytes and make the refusals of slfp_bn_train_fwd / slfp_bn_train_bwd in the same order
 * before any device work, leaving the outputs untouched; save_lo counts among the per-channel arrays; y_codes (NULL:
 * SLFP_ERR_BAD_ARG) needs 4-byte alignment (SLFP_ERR_ALIGNMENT, behind x).  y_codes may not alias x, gx not x.  n == 0 returns
 * SLFP_OK.  Algorithmic traffic per element (computed from the code, not measured): forward 4 + 4 + 1 = 9 B against 12 B,
 * backward 8 + 8 + 4 = 20 B against 28 B of the plain form. */
int slfp_bn_codes_train_supported(int64_t n, int64_t h, int64_t w, int64_t c, int x_layout, float y_ka, int y_qbits);
int slfp_bn_codes_train_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                            float momentum, float eps, int relu, float y_ka, int y_qbits, uint8_t* y_codes,
                            float* save_mean, float* save_invstd, float* save_lo,
                            int64_t n, int64_t h, int64_t w, int64_t c, int x_layout,
                            void* workspace, size_t ws_bytes, void* stream);
int slfp_bn_codes_train_bwd(const float* x, const float* gy, const float* gamma, const float* beta, const float* save_mean,
                            const float* save_invstd, const float* save_lo, int relu, float* gx, float* ggamma, float* gbeta,
                            int64_t n, int64_t h, int64_t w, int64_t c, int x_layout,
                            void* workspace, size_t ws_bytes, void* stream);

/* ---- training-mode BatchNorm2d + residual add (+ReLU) that writes the trunk AND its readers' codes (csrc/bn_train.hip, the
 * residual-and-codes form) ------------------------------------------------------------------------------------------------------
 * The trunk of a ResNet leaves a Bottleneck as relu(bn3(.) + identity) and is read by the next block's conv1 (and downsample.0 at a
 * stage boundary), whose first act is quantize_act(y / Ka), and by the next block's add, which needs float32.  So the forward of
 * slfp_bn_res_train_fwd stores, next to the float32 y, one byte per element: the extended code of the readers' quantizer (y_ka
 * their Ka, y_qbits their q_bit, 8 or 7).  The training twin of slfp_conv2d_fwd_res_codes.  The contract is exact:
 *   statistics save_mean, save_invstd and the running statistics are exactly those of slfp_bn_train_fwd on the same x.
 *   forward    y is slfp_bn_res_train_fwd's, bit for bit: t = the apply with relu = 0;  z = t + res, rounded on its own;  relu:
 *              y = z < 0 ? 0 : z.  y_codes[i] = the byte slfp_encode_f32(y, y_ka, fmt(y_qbits) | SLFP_FMT_EXT) gives element i,
 *              through the readers' threshold table, a lane's four channels as one dword.  A NaN in y takes code 0x00: the trunk's
 *              readers see the tiny class, the float32 trunk itself (and so the next add) still carries the NaN.  The apply pass
 *              reads x and res once and writes y and y_codes once: 4 + 4 + 4 + 1 = 13 B per element against 12 B (17 B against
 *              16 B with the statistics pass).
 *   backward   slfp_bn_res_train_bwd, as it is: it reads x and y.
 * No atomics; two calls give the same bits.  Supported (slfp_bn_res_codes_train_supported: 1 / 0, host only): the set of
 * slfp_bn_train_supported, and in addition c % 4 == 0, y_qbits 8 or 7, y_ka > 0 with a proven code table; everything else is
 * SLFP_ERR_UNSUPPORTED.  The workspace is that of slfp_bn_train_workspace_bytes.  The refusals of slfp_bn_res_train_fwd come
 * first, in its order, then those of slfp_bn_codes_train_fwd (y_codes NULL: SLFP_ERR_BAD_ARG; not 4-byte aligned:
 * SLFP_ERR_ALIGNMENT); y may alias neither x nor res, and y_codes may alias no other operand (x, res, y, the per-channel arrays,
 * the running statistics, the workspace): SLFP_ERR_BAD_ARG.  Every refusal is made before any device work and leaves y, y_codes,
 * the saves and the running statistics untouched.  n == 0 returns SLFP_OK. */
int slfp_bn_res_codes_train_supported(int64_t n, int64_t h, int64_t w, int64_t c, int x_layout, float y_ka, int y_qbits);
int slfp_bn_res_codes_train_fwd(const float* x, const float* res, const float* gamma, const float* beta, float* running_mean,
                                float* running_var, float momentum, float eps, int relu, float y_ka, int y_qbits,
                                float* y, uint8_t* y_codes, float* save_mean, float* save_invstd,
                                int64_t n, int64_t h, int64_t w, int64_t c, int x_layout,
                                void* workspace, size_t ws_bytes, void* stream);

/* ---- training-mode BatchNorm2d -> layer-output quantizer -> activation that writes the next Conv2d_Q's codes (csrc/bn_train.hip,
 * the table-and-codes form) ---------------------------------------------------------------------------------------------------
 * In Conv2d_Q -> BatchNorm2d -> layerout_quantize_func -> Swish | GELU -> Conv2d_Q (nets_cifar/mobilenetv1.py:176-250,
 * nets_cifar/vgg16.py:186-293) a value behind the layer-output quantizer is one of slfp_layerout_lut_classes() classes, so the
 * activation followed by the reader's quantize_act(. / Ka) is ONE byte per class: the training twin of slfp_conv2d_fwd_codes_lut.
 * code_table: device memory, SLFP_LAYEROUT_LUT_BYTES bytes, 16-byte aligned; index i is the class of slfp_layerout_lut_values /
 * layerout_class, index 0 the NaN class; the caller builds it (code_table[i] = the extended code, in the reader's Ka and q_bit, of
 * act(value_i); the NaN class and the padding 0x00).  The kernel is not told the reader's Ka or q_bit: the table holds them.  The
 * contract is exact:
 *   statistics save_mean, save_invstd, save_lo and the running statistics are bit-identical to slfp_bn_lut_train_fwd on the same x.
 *   forward    t = (((x - save_mean) - save_lo) * (save_invstd * gamma)) + beta, the LUT form's expression;
 *              y_codes[i] = code_table[layerout_class(layerout_bits(t_i))].  With a table built as above that is the byte
 *              slfp_encode_f32(fmt | SLFP_FMT_EXT) gives slfp_bn_lut_train_fwd's y, except where that y is a NaN (the exact-zero
 *              class): the float32 interface hands the reader the NaN, the codes hand it 0x00, the tiny class, as everywhere on the
 *              code path.  No float32 y is written.  The apply pass reads x once and writes one byte per element, a lane's four
 *              channels as one dword; each workgroup holds the byte table alone in LDS (4 928 B against the float table's 19 712 B).
 *   backward   there is no new entry point: the backward is slfp_bn_lut_train_bwd, unchanged, with the dact_table of the same
 *              activation.  It recomputes every class from x and the three saves and reads no forward output.
 * No atomics; two calls give the same bits; a NaN or an inf stays in its channel.  Supported (slfp_bn_lut_codes_train_supported:
 * 1 / 0, host only): the set of slfp_bn_train_supported, and in addition c % 4 == 0; everything else is SLFP_ERR_UNSUPPORTED.  The
 * workspace is that of slfp_bn_train_workspace_bytes.  The refusals are those of slfp_bn_lut_train_fwd, in its order, before any
 * device work, leaving the outputs untouched: y_codes stands where y stood (NULL: SLFP_ERR_BAD_ARG; not 4-byte aligned:
 * SLFP_ERR_ALIGNMENT, behind x), code_table where act_table stood (NULL: SLFP_ERR_BAD_ARG; not 16-byte aligned:
 * SLFP_ERR_ALIGNMENT, behind the per-channel arrays).  y_codes may not alias x.  n == 0 returns SLFP_OK.
 * Algorithmic traffic per element (computed from the code, not measured): forward 4 + 4 + 1 = 9 B against the LUT form's 12 B; the
 * reader's forward and its weight gradient read 1 B each against 4 B; the backward's 20 B are the LUT form's; saved for the
 * backward are x and the codes, 5 B against 8 B. */
int slfp_bn_lut_codes_train_supported(int64_t n, int64_t h, int64_t w, int64_t c, int x_layout);
int slfp_bn_lut_codes_train_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                float momentum, float eps, const uint8_t* code_table, uint8_t* y_codes,
                                float* save_mean, float* save_invstd, float* save_lo,
                                int64_t n, int64_t h, int64_t w, int64_t c, int x_layout,
                                void* workspace, size_t ws_bytes, void* stream);

/* ---- self-check ------------------------------------------------------------------------
 * The kernels compute x / scale_div with an FMA correction chain on a host-computed
 * reciprocal instead of the IEEE division macro (csrc/slfp_device.hpp, ScaleDiv).  This
 * sweeps ALL 2^32 float32 inputs on the device and writes to out2 (device memory, 2 x u64):
 * out2[0] = inputs with |x| and |x/scale| in [1e-20, 1e20] whose quotient differs from IEEE `/`,
 * out2[1] = inputs (all 2^32) for which any quantizer result would differ.  Both must be 0. */
int slfp_debug_div_mismatches(float scale_div, unsigned long long* out2, void* stream);

/* The conv kernels evaluate QA(x / Ka) through a per-Ka threshold table (csrc/slfp_enc.hpp: one approximate
 * multiply picks a bin, one exact compare in x-space picks the side) instead of the long form above.  The table is
 * built and proven on the host per (Ka, format); this sweeps ALL 2^32 float32 inputs on the device and writes
 * out2[0] = inputs whose float32 result differs from the long form, out2[1] = inputs whose fp16 MFMA-operand
 * result differs (+0 / -0 counted as equal).  Both must be 0.  fmt: SLFP_FMT_ACT8 or SLFP_FMT_SFP7.
 * Returns SLFP_ERR_UNSUPPORTED if no table can be proven for this scale (the kernels then use the long form). */
int slfp_debug_enc_mismatches(float scale_div, int fmt, unsigned long long* out2, void* stream);
/* The same for the hi / lo fp16 operand pair of the three-pass (float32-equivalent) pointwise mode (round 3): *out1 = inputs
 * (all 2^32) whose pair from the two tables differs from hi = fp16(16 Q), lo = fp16(16 Q - fp32(hi)).  Must be 0. */
int slfp_debug_enc_hl_mismatches(float scale_div, int fmt, unsigned long long* out1, void* stream);
/* 1 if the threshold table exists for this scale / format (host-only query, no device work). */
int slfp_enc_table_ok(float scale_div, int fmt);

/* ---- optimizer step: replaces DSGD / SSGD / NormalSGD.step (utils/optimizer.py) ---------------------------------------
 * For every tensor i (numel[i] float32 elements; param[i], grad[i] and momentum_buf[i] share one dense layout), in place:
 *     g = g + weight_decay * p                      (weight_decay != 0; grad[i] keeps the result, as p.grad does)
 *     buf = first_step[i] ? g : (buf * momentum) + damp_alpha * g      (momentum != 0; buf is not read on the first step)
 *     d = momentum != 0 ? (nesterov ? g + momentum * buf : buf) : g
 *     t = d * -lr;   wb = Q(p);   p = p + t
 *     SLFP_OPT_DSGD: s = |wb - Q(p)| < 1e-4f ? 2 : 0;   SLFP_OPT_SSGD: s = |p| + 1;   then p = p + t * s
 * Q = quantize_weight(qbits) at unit scale (32 = identity).  Every line is its own float32 rounding; `a + alpha * b` is one
 * fused multiply-add, as ATen's add(alpha=) computes it on gfx950.  lr, momentum, damp_alpha = float32(1 - dampening) (the
 * subtraction in double) and weight_decay are the float32 values ATen applies.  momentum_buf: NULL iff momentum == 0.  The
 * host arrays are read during the call only; tensors are grouped into launches of up to 48 (no device allocation, no copy). */
#define SLFP_OPT_SGD 0  /* NormalSGD */
#define SLFP_OPT_DSGD 1
#define SLFP_OPT_SSGD 2
typedef struct slfp_sgd_hparams {
    int32_t rule, qbits;                          /* SLFP_OPT_*, 8 / 7 / 32                        */
    float lr, momentum, damp_alpha, weight_decay; /* the float32 values ATen applies               */
    int32_t nesterov, reserved;                   /* nesterov: 0 / 1                               */
} slfp_sgd_hparams;
int slfp_sgd_step_f32(const slfp_sgd_hparams* h, size_t ntensors, float* const* param, float* const* grad,
                      float* const* momentum_buf, const int64_t* numel, const uint8_t* first_step, void* stream);

/* ---- backward of Conv2d_Q / Linear_Q (the reference's STE gradients, utils/conv2d_func.py) ----------------------------
 *     gx = conv_input(QW(w / Kw), gy) * Kw      gw = conv_weight(QA(x / Ka), gy) * Ka      gb = sum_{n,h,w} gy
 * accumulated in float32 (VALU FMAs for depthwise, float32 MFMA for pointwise); QA is applied on load, bit-identical to
 * slfp_quantize_f32.  Deterministic: partial sums go through the workspace and are added in a fixed order, no atomics.
 * Covered: 3x3 depthwise (groups == C_in == C_out, stride 1 or 2, pad 1, dilation 1) and 1x1 stride-1 pad-0 groups-1 layers
 * (a Linear_Q is the 1x1 case with n = rows, h = w = 1); everything else returns SLFP_ERR_UNSUPPORTED.
 * slfp_conv2d_bwd_kernel_name: "dw3x3_bwd", "pw_bwd_mfma_f32" or "composite" (not covered).  mfma_passes is ignored.
 * x / gx follow d->x_layout, gy follows d->y_layout, w_oihw and gw_oihw are contiguous OIHW.  gx / gw / gb may be NULL (not
 * needed); gb needs gw.  All tensors 16-byte aligned; workspace: slfp_conv2d_bwd_workspace_bytes(d, gx != NULL, gw != NULL)
 * bytes, 16-byte aligned (NULL if 0). */
int slfp_conv2d_bwd_supported(const slfp_conv2d_desc* d);
const char* slfp_conv2d_bwd_kernel_name(const slfp_conv2d_desc* d);
size_t slfp_conv2d_bwd_workspace_bytes(const slfp_conv2d_desc* d, int need_gx, int need_gw);
int slfp_conv2d_bwd(const slfp_conv2d_desc* d, const float* x, const float* w_oihw, const float* gy, float* gx, float* gw_oihw,
                    float* gb, void* workspace, void* stream);

/* The same four with a `flags` word; flags == 0 is exactly the functions above.  SLFP_BWD_DENSE adds the implicit-GEMM
 * family "dense_bwd_mfma_f32" (float32 MFMA, xq encoded on load and never materialised, deterministic) for every
 * groups == 1, dilation 1 layer the two families above do not take: any kernel size, stride and padding, any channel
 * count (3x3 / 5x5 / 7x7 / 11x11, strided 1x1, C_in = 3 stems).  Grouped non-depthwise and dilated layers stay
 * unsupported; unknown flag bits are SLFP_ERR_BAD_ARG (not supported / "composite" / 0 bytes in the queries). */
#define SLFP_BWD_DENSE 1u   /* also cover groups == 1, dilation 1 layers of any kernel size / stride / padding */
int slfp_conv2d_bwd_supported_ex(const slfp_conv2d_desc* d, unsigned flags);
const char* slfp_conv2d_bwd_kernel_name_ex(const slfp_conv2d_desc* d, unsigned flags);
size_t slfp_conv2d_bwd_workspace_bytes_ex(const slfp_conv2d_desc* d, unsigned flags, int need_gx, int need_gw);
int slfp_conv2d_bwd_ex(const slfp_conv2d_desc* d, unsigned flags, const float* x, const float* w_oihw, const float* gy,
                       float* gx, float* gw_oihw, float* gb, void* workspace, void* stream);

/* slfp_conv2d_bwd_ex with the activation operand as 1-byte codes: x_codes[i] = the byte slfp_encode_f32(x, d->ka,
 * fmt(d->qbits) | SLFP_FMT_EXT) gives element i -- this layer's own Ka and q_bit, as a producer such as slfp_bn_codes_train_fwd
 * stores them.  Both quantizers are pure straight-through estimators, so decode(code) is the operand of the weight gradient bit
 * for bit: in all three families the x load becomes a byte load (a dword of four channels where the float path loads a float4)
 * decoded through a 256-entry float32 table in LDS; the gx half never reads x.  gx, gw and gb are equal (as float32 values; +0
 * and -0 alike) to slfp_conv2d_bwd_ex on any float32 x with these codes, except where x holds a NaN, which has no code (0x00,
 * the tiny class).  New entry points, not a flag bit: `flags` means what it means for slfp_conv2d_bwd_ex, and the workspace and
 * kernel names are those of the _ex queries.  x_codes: NHWC only, C_in % 4 == 0, 4-byte aligned (the other tensors 16-byte);
 * NCHW x, C_in % 4 != 0 and whatever slfp_conv2d_bwd_ex refuses are SLFP_ERR_UNSUPPORTED / 0. */
int slfp_conv2d_bwd_codes_supported(const slfp_conv2d_desc* d, unsigned flags);
int slfp_conv2d_bwd_codes(const slfp_conv2d_desc* d, unsigned flags, const uint8_t* x_codes, const float* w_oihw,
                          const float* gy, float* gx, float* gw_oihw, float* gb, void* workspace, void* stream);

/* Which kernel instances of csrc/conv_bwd.hip slfp_conv2d_bwd_ex (x_codes == 0) or slfp_conv2d_bwd_codes (x_codes == 1) launches
 * for this descriptor and these flags under the switches read at load, when gx (need_gx) and / or gw with gb (need_gw) are asked
 * for.  One word per template argument a launcher chooses, then the runtime split the launch is sized by:
 *   dw/s<1|2>/<tab|long|codes>/<act8|sfp7>/b<blocks>                                 k_dw3x3_bwd<S, AF>: one kernel gives gx, gw and gb
 *   pw/gx/tm<1|2>tn<1|2>/<v4|v1>                                                     k_gemm_f32<TM, TN, false, kNoEnc, VEC>
 *   pw/gw/tm<1|2>tn<1|2>/<v4|v1>/<tab|long|codes>/<act8|sfp7>/p<splits>k<kps>        k_gemm_f32<TM, TN, true, AF, VEC>
 *   dense/gx/tn<1|2>/<v4|v1>                                                         k_dense_gx<TN, VEC>
 *   dense/gw/tm<1|2>tn<1|2>/<v4|v1>/<tab|long|codes>/<act8|sfp7>/p<splits>k<kps>     k_dense_gw<TM, TN, AF, VEC>
 * tab / long / codes: x is encoded on load through the threshold table or the long form, or arrives as codes and is decoded; the
 * format word names the long form's or the codes' template argument and, with `tab`, the table's contents (one instance serves
 * both formats).  v4 / v1: float4 or scalar loads (both channel counts multiples of 4, or not).  b: workgroups along x of the
 * depthwise kernel, which walk the image units grid-stride; p, k: the splits of the gw contraction over its rows and the rows per
 * split, p also being the partials k_reduce_parts sums (the pointwise family writes gw directly when p == 1).  With need_gx and
 * need_gw both set the pointwise and dense families give "<gx string>+<gw string>".  "composite" where the entry point refuses
 * (a null descriptor, unknown flag bits, an unsupported layer, codes that are not NHWC with C_in % 4 == 0); "none" when nothing is
 * asked for.  Printed from the selection the launch consumes (bwd_kind_ex, pw_shape, dense_shape, dw_geom / dw_blocks, act_form).
 * Host only: no device is touched.  The pointer stays valid until the next call on the same thread. */
const char* slfp_debug_bwd_instance(const slfp_conv2d_desc* d, unsigned flags, int x_codes, int need_gx, int need_gw);

/* ---- layout helpers (the reference is NCHW; the kernels are NHWC) -------------------- */
int slfp_nchw_to_nhwc_f32(const float* x, float* y, int64_t n, int64_t c, int64_t h, int64_t w, void* stream);
int slfp_nhwc_to_nchw_f32(const float* x, float* y, int64_t n, int64_t c, int64_t h, int64_t w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SLFP_H_ */
