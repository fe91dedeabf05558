// slfp_host.hpp -- host-side helpers shared by the translation units of libslfp_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include "../../include/slfp.h"
#include "slfp_device.hpp"
#include "slfp_enc.hpp"

namespace slfp {

// thread-local last-error text (slfp_last_error()).
void set_error(const char* fmt, ...);
int fail(int code, const char* fmt, ...);
// Returns SLFP_OK or SLFP_ERR_HIP (and records the HIP error string) after a launch.
int check_launch(const char* what);

// Kernels that need more than 64 KiB of dynamic LDS must opt in with hipFuncSetAttribute.  The attribute belongs to the
// (device, function) pair, so it is set once per pair, under a lock (any host thread may call the library; one process
// may drive several devices).  Returns SLFP_OK or an error status.
int raise_lds_limit(const void* fn, size_t lds_bytes);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Host side of ScaleDiv (slfp_device.hpp): r = RN(1/d) via double (1/d of a float is never
// within 2^-53 of a float rounding midpoint unless it is exact, so the double rounding is
// harmless).  scale_div_ok() is the range the FMA chain is valid for.
inline bool scale_div_ok(float d) { return std::isfinite(d) && d >= 1e-30f && d <= 1e30f; }

inline ScaleDiv make_scale_div(float d, int esh = 0) {
    ScaleDiv s;
    s.d = std::ldexp(d, -esh);  // dividing by d/2^esh == multiplying the quotient by 2^esh, exactly
    s.r = (float)(1.0 / (double)s.d);
    return s;
}

// Experiment switches (profiles/*.sh, profiles/variants.py).  They are environment variables read ONCE, when the library is
// first used (and again only on slfp_debug_reload_switches()): no getenv() is reachable from a launch.
//   SLFP_LONG_ENCODE    keep every kernel on the long-form quantizer (slfp_device.hpp) instead of the threshold table
//   SLFP_DW_OLD         keep every depthwise layer on conv_dw.hip
//   SLFP_PW_NOSTG       pointwise kernels without the LDS-staged whole-line stores
//   SLFP_PW_NOTAB       pointwise kernels on the long-form quantizer
//   SLFP_PW_STG_MAXKS   stream kernel: staged stores up to this many k-steps (default: 1, 2 and 8)
//   SLFP_PW_GRID=<n>    persistent pointwise kernels: at most n workgroups (k_pw_stream, k_pwc_stream) / n rank groups of 8 x n_slices
//                       workgroups (k_pwc_slice), so that a small layer runs several trips of the persistent loop (tests); unset: no cap
//   SLFP_PW_NT_MIN_MB / SLFP_DW_NT_MIN_MB   output size from which staged / depthwise stores carry the nt hint
//   SLFP_DW_ROWS        0: stride-2 depthwise layers stay on the tile kernel (conv_dw2.hip); unset: the measured rule
//                       (dw3x3_rows_applicable); any other value: a mask of size classes that take conv_dw3.hip (A/B runs)
struct Switches {
    bool long_encode, dw_old, pw_nostg, pw_notab;
    int pw_stg_maxks;         // -1: default rule
    long long pw_nt_min_mb;   // default 0
    long long dw_nt_min_mb;   // default 30
    bool stem_old;            // SLFP_STEM_OLD: the MobileNetV1 stem on the vector ALU (k_stem_fixed) instead of the float32 MFMA kernel (k_stem_mx)
    bool pwc_slice;           // SLFP_PWC_NOSLICE unsets it: deep code-path pointwise layers on k_pwc_tiled / k_pwc_stream instead of k_pwc_slice
    bool dense_generic;       // SLFP_DENSE_GENERIC: 3x3 stride-1 layers on the general k_dense_mfma instead of the unrolled k_dense3x3
    int dense_cfg;            // SLFP_DENSE_CFG=<wm><wn><mt> (e.g. 244): force a dense k x k tiling where it fits (sweeps); 0 = cost model
    int dense_nwb;            // SLFP_DENSE_NWB=2: keep two weight buffers everywhere (A/B of the three-buffer pipeline)
    bool dense_encx;          // SLFP_DENSE_NOENCX unsets it: k_dense3x3_res encodes the float32 halo on load (C_in == 64, C_out <= 64) instead of reading the pre-pass's fp16 copy
    bool dense_res;           // SLFP_DENSE_NORES unsets it: 3x3 stride-1 layers with C_in <= 64 on the persistent weights-resident k_dense3x3_res
    bool stem_im2row;         // SLFP_STEM_IM2ROW: large-kernel stems through the im2row workspace (the round-1 form; A/B of k_stem_rows)
    int dw_rows;              // SLFP_DW_ROWS: -1 (unset) the measured rule, 0 never, else bit k = size class k (dw_rows_class) on k_dw3x3_rows
    int pw_grid;              // SLFP_PW_GRID: cap of the persistent pointwise grids (0: unset, no cap)
    int pw_stream_max_kb;     // SLFP_PW_STREAM_MAX_KB: largest W (KiB, fp16) the float32-interface path gives to the LDS-resident stream kernel (default 30; its capacity is 128)
};
const Switches& switches();
void reload_switches();
inline bool long_encode_forced() { return switches().long_encode; }
inline bool dw_old_forced() { return switches().dw_old; }
// The table for the activation side of a layer, or nullptr when the long form has to be used.
inline const EncArgs* act_table(float ka, int fmt_act, int rep) {
    if (long_encode_forced()) return nullptr;
    const EncArgs* t = enc_table(ka, fmt_act, rep);
    return t->valid ? t : nullptr;
}

// Kernel families (slfp_conv2d_kernel_name reports them).
enum KernelFamily { kDw3x3 = 0, kPointwise = 1, kDirect = 2, kDenseMfma = 3, kStemMfma = 4, kStemSmall = 5 };

struct ConvPlan {
    KernelFamily family;
    int fmt_act;   // kFmtAct8 | kFmtSfp7
    int fmt_w;     // kFmtW8   | kFmtSfp7
    int passes;    // MFMA passes for the pointwise family (1 or 3)
    int64_t h_out, w_out;
    float s1, s2;  // epilogue: out = ((acc + bias/s1/s2) * s1) * s2  (conv: Ka,Kw; linear: Kw,Ka)
    // pointwise: padded K (multiple of 64) and N (multiple of 64) of the fragment-ordered blob
    int64_t k_pad, n_pad;
    size_t wprep_bytes;
    // Channel counts that are not a multiple of 4 (ShuffleNetV2's 58-channel branches) break the
    // 16-byte NHWC access the depthwise / pointwise kernels are built on.  Such layers run those
    // same kernels on channel-padded copies: x -> [..][cpi] (zeros appended: Q(0) = 0 and the
    // padded weights are 0, so results are unchanged), y <- [..][cpo].  `family` etc. describe
    // the inner (padded) launch.
    bool repad;
    int64_t cpi, cpo;
};

// Validates `d` and fills `plan`; returns SLFP_OK or an error status (error text recorded).
int make_plan(const slfp_conv2d_desc* d, ConvPlan* plan);

// ---- launchers implemented next to their kernels (all NHWC, all async on `stream`) ----
int launch_quantize(const float* x, float* y, size_t n, float scale, int fmt, hipStream_t stream);
int launch_dw3x3(const slfp_conv2d_desc& d, const ConvPlan& p, const float* x, const float* wq9c,
                 const float* bias, const PostOp& post, float* y, hipStream_t stream);
// the straight-line depthwise tile kernel (conv_dw2.hip): C a multiple of 32, threshold table available
bool dw3x3_tile_applicable(const slfp_conv2d_desc& d, const ConvPlan& p, const float* bias, const PostOp& post);
int launch_dw3x3_tile(const slfp_conv2d_desc& d, const ConvPlan& p, const float* x, const float* wq9c,
                      const PostOp& post, float* y, hipStream_t stream);
// the register-window depthwise kernel (conv_dw3.hip): the tile kernel's preconditions, stride 2, and the SLFP_DW_ROWS rule
bool dw3x3_rows_applicable(const slfp_conv2d_desc& d, const ConvPlan& p, const float* bias, const PostOp& post);
int launch_dw3x3_rows(const slfp_conv2d_desc& d, const ConvPlan& p, const float* x, const float* wq9c,
                      const PostOp& post, float* y, hipStream_t stream);
// which template instance launch_dw3x3 runs for this layer (the rows, tile or general kernel) under the switches read at load: each
// launcher maps its selection to a kernel pointer and launches it, and the name is printed only after the same lookup returned one
// (slfp_debug_dw3x3_instance; host only; grammar in include/slfp.h; what the four files share: conv_dw_core.hpp).  "none" outside
// the family, where the launch would be refused or where the selection has no instance; valid until the next call on the same thread.
const char* dw3x3_instance_name(const slfp_conv2d_desc& d, const ConvPlan& p, bool has_bias, const PostOp& post);
const char* dw3x3_tile_name(const slfp_conv2d_desc& d, const ConvPlan& p, const PostOp& post);
const char* dw3x3_rows_name(const slfp_conv2d_desc& d, const ConvPlan& p, const PostOp& post);
// SLFP_DW_ROWS as the environment gives it (nullptr: unset) -> Switches::dw_rows
inline int parse_dw_rows(const char* e) {
    if (!e || !*e) return -1;
    const long v = strtol(e, nullptr, 0);
    return v <= 0 ? 0 : (int)(v & 0xF);
}
// size class of a depthwise layer: 0 / 1 / 2 / 3 = output images of at least 56 x 56 / 28 x 28 / 14 x 14 / fewer pixels
inline int dw_rows_class(int64_t h_out, int64_t w_out) {
    const int64_t px = h_out * w_out;
    return px >= 56 * 56 ? 0 : (px >= 28 * 28 ? 1 : (px >= 14 * 14 ? 2 : 3));
}
// res: the residual operand of slfp_conv2d_fwd_res (float32 NHWC like y; needs pointwise_res_applicable) or nullptr
int launch_pointwise(const slfp_conv2d_desc& d, const ConvPlan& p, const float* x, const void* wfrag,
                     const float* bias, const PostOp& post, float* y, hipStream_t stream, const float* res = nullptr);
bool pointwise_res_applicable(const slfp_conv2d_desc& d, const ConvPlan& p);
// what launch_pointwise (has_res: with a residual operand) / launch_pointwise_entry (y_codes: for the reader y_ka, y_fmt) decide for
// this layer under the switches read at load, printed from the selection they consume (slfp_debug_pw_variant; host only).  "none"
// outside the family or where the launch would be refused; valid until the next call on the same thread.
const char* pw_variant_name(const slfp_conv2d_desc& d, const ConvPlan& p, bool has_res, bool y_codes, float y_ka, int y_fmt);
// ---- 1-byte activation codes between layers (slfp_codes.hpp; slfp_conv2d_fwd_codes) ----
// How a layer's input arrives and its output leaves: float32, or the extended codes of QA(. / ka) in format fmt.
struct CodeIo {
    bool x_codes;     // x holds uint8 codes of QA(x / d.ka) (format of d.qbits) instead of float32
    bool y_codes;     // y receives uint8 codes of QA(out / y_ka) in format y_fmt instead of float32
    float y_ka;
    int y_fmt;        // kFmtAct8 | kFmtSfp7
    int64_t y_ld = 0; // y_codes: channel count of the (wider) NHWC code tensor y is a channel slice of; 0: y is dense (C_out)
    const uint8_t* lut = nullptr;   // slfp_conv2d_fwd_codes_lut (y_codes, post_scale / post_shift): the byte table of the layer-output
                                    // classes (slfp_layerout_lut.hpp), device memory, 16-byte aligned; y_ka / y_fmt are then not read
};
// Workgroups of `fn` (block size, dynamic LDS) that fit one CU at once (hipOccupancyMaxActiveBlocksPerMultiprocessor, cached
// per device / function / LDS size): how persistent grids are sized.  >= 1.
int resident_blocks_per_cu(const void* fn, int block_threads, size_t dynamic_lds);
// Number of compute units of the current device (cached per device; 256 on MI355X): persistent grids are sized from it.
int device_cu_count();
// pointwise, float32 in -> codes out (conv_pw.hip's YC forms; slfp_conv2d_fwd_entry): the layer at which a chain of codes begins.
// Single-pass table forms, C_out a multiple of 16, C_in a multiple of 4, no channel re-padding, no layer-output quantizer.
bool pointwise_entry_applicable(const slfp_conv2d_desc& d, const ConvPlan& p, int post_flags, float y_ka, int y_fmt);
int launch_pointwise_entry(const slfp_conv2d_desc& d, const ConvPlan& p, const float* x, const void* wfrag, const float* bias,
                           const PostOp& post, void* y_codes, const CodeIo& io, hipStream_t stream);
// pointwise on codes (conv_pw_codes.hpp): codes in, codes or float32 out; the SAME prepared blob as launch_pointwise
bool pwc_applicable(const slfp_conv2d_desc& d, const ConvPlan& p, int post_flags, bool y_codes);
int launch_pwc(const slfp_conv2d_desc& d, const ConvPlan& p, const uint8_t* x, const void* wfrag, const float* bias,
               const PostOp& post, void* y, const CodeIo& io, hipStream_t stream, const float* res = nullptr, void* res_codes = nullptr);
// the same for launch_pwc (codes in): code or float32 output, residual operand, second (code) output
const char* pwc_variant_name(const slfp_conv2d_desc& d, const ConvPlan& p, bool y_codes, bool has_res, bool has_dual, bool lut = false);
// lut (y_codes only): the table-epilogue instance of the selected kernel (slfp_conv2d_fwd_codes_lut); "none" where none is built
// res_codes (with res, float32 y, C_out a multiple of 16; slfp_conv2d_fwd_res_codes): the uint8 tensor that receives, next to y, the codes
// of y for the reader io.y_ka / io.y_fmt describe
// pointwise on codes in the float32-equivalent (three-pass) mode (slfp_conv2d_fwd_codes_x3): SLFP<3,4> codes in, codes or float32 out,
// both planes of the SAME prepared blob; no residual, table-epilogue, channel-slice or half-live form.  The name comes from the
// selection the launcher dispatches on ("none" where the launch would be refused; valid until the next call on the same thread).
bool pwc_x3_applicable(const slfp_conv2d_desc& d, const ConvPlan& p, int post_flags, bool y_codes);
int launch_pwc_x3(const slfp_conv2d_desc& d, const ConvPlan& p, const uint8_t* x, const void* wfrag, const float* bias,
                  const PostOp& post, void* y, const CodeIo& io, hipStream_t stream);
const char* pwc_x3_variant_name(const slfp_conv2d_desc& d, const ConvPlan& p, bool y_codes);
// the MobileNetV1 image stem with code output (conv_direct.hip)
bool stem_codes_applicable(const slfp_conv2d_desc& d, const ConvPlan& p, int post_flags);
int launch_stem_codes(const slfp_conv2d_desc& d, const ConvPlan& p, const float* x, const float* wq_hwio, const float* bias,
                      const PostOp& post, void* y, const CodeIo& io, hipStream_t stream);
// depthwise 3x3 on codes (conv_dwc.hip): codes in, codes or float32 out
bool dwc_applicable(const slfp_conv2d_desc& d, const ConvPlan& p, const float* bias, int post_flags);
int launch_dwc(const slfp_conv2d_desc& d, const ConvPlan& p, const uint8_t* x, const float* wq9c, const PostOp& post,
               void* y, const CodeIo& io, hipStream_t stream);
// the k_dwc instance launch_dwc runs, printed from the selection it consumes (slfp_debug_dw3x3_instance; host only)
const char* dwc_instance_name(const slfp_conv2d_desc& d, const ConvPlan& p, const PostOp& post, const CodeIo& io);
// ---- one depthwise -> pointwise block in one kernel (conv_dwpw.hip: k_dwpw, conv_dwpw_codes.hip: k_dwpw_codes; their common
// geometry, LDS size, parameters and device steps: conv_dwpw_core.hpp) ----
// The (S, KS, NT) instances both kernels are built for.  The selections behind the queries (through dwpw_instance_built) and the two
// launchers' dispatch expand this one list, so a pair a query accepts always has a kernel to run.
#define SLFP_DWPW_INSTANCES(X)                                                                                   \
    X(1, 1, 4) X(1, 1, 8) X(1, 1, 16) X(1, 2, 4) X(1, 2, 8) X(1, 2, 16) X(1, 4, 4) X(1, 4, 8) X(1, 4, 16)        \
    X(2, 1, 4) X(2, 1, 8) X(2, 1, 16) X(2, 2, 4) X(2, 2, 8) X(2, 2, 16) X(2, 4, 4) X(2, 4, 8) X(2, 4, 16)
// What the launchers choose among the instances: slfp_dwpw_supported / slfp_dwpw_codes_supported answer 1 exactly where the
// selection below succeeds, slfp_dwpw_fwd / slfp_dwpw_fwd_codes dispatch on it, slfp_debug_dwpw_instance prints it.
struct DwPwSel {
    int s, ks, nt;   // S (depthwise stride), KS = K / 32, NT = N / 16
    int fmt_in;      // k_dwpw_codes: FMT, what the input codes are (kFmtAct8 | kFmtSfp7)
    bool yc;         // k_dwpw_codes: YC, code output
};
inline bool dwpw_instance_built(int s, int ks, int nt) {
#define SLFP_DWPW_HAS(SS, KK, NN) if (s == SS && ks == KK && nt == NN) return true;
    SLFP_DWPW_INSTANCES(SLFP_DWPW_HAS)
#undef SLFP_DWPW_HAS
    return false;
}
// the float32 interface's selection (conv_dwpw.hip); false: the pair does not run as one kernel.  Host only.
bool dwpw_select(const slfp_conv2d_desc* dw, const slfp_conv2d_desc* pw, DwPwSel* s);
// the code interface's (conv_dwpw_codes.hip)
bool dwpw_codes_select(const slfp_conv2d_desc* dw, const slfp_conv2d_desc* pw, const slfp_conv2d_io* io, int relu1, int relu2, DwPwSel* s);
int launch_direct(const slfp_conv2d_desc& d, const ConvPlan& p, const float* x, const float* wq_hwio,
                  const float* bias, const PostOp& post, float* y, hipStream_t stream);
bool stem_applicable(const slfp_conv2d_desc& d);  // direct family: the small-C_in stem kernel takes it
// which instance of k_direct / k_stem / k_stem_fixed / k_stem_mx launch_direct (io == nullptr) or launch_stem_codes runs, printed from
// the selection the launch consumes (slfp_debug_stem_instance; host only; grammar in include/slfp.h).  "none" outside the family or
// where the launch would be refused; valid until the next call on the same thread.
const char* direct_instance_name(const slfp_conv2d_desc& d, const ConvPlan& p, const PostOp& post, const CodeIo* io, bool u8 = false);
// ---- image stems on NHWC bytes + a float32 pixel table [C_in][256] (slfp_conv2d_fwd_u8): the U8 form of the four stem kernels' fill
// step.  `pix` / `u8` on the launchers and name functions of the stem families select it; `x` then points at bytes of any alignment.
bool stem_u8_applicable(const slfp_conv2d_desc& d, const ConvPlan& p, const PostOp& post, const CodeIo* io);
int launch_stem_u8(const slfp_conv2d_desc& d, const ConvPlan& p, const uint8_t* x, const float* pix, const float* wq_hwio,
                   const float* bias, const PostOp& post, void* y, const CodeIo* io, hipStream_t stream);
// pointwise: does W (padded) fit the LDS-resident stream kernel?  (that kernel also takes even channel
// counts that are not a multiple of 4, with 8-byte accesses)
bool pointwise_stream_fits(int64_t k_pad, int64_t n_pad, int passes);
// dense k x k implicit GEMM on MFMA (conv_dense.hip); wblob = [tap][n_tile][k_step][64][8] fp16;
// `workspace` (dense_mfma_workspace_bytes) receives the input encoded once to fp16
bool dense_mfma_applicable(const slfp_conv2d_desc& d, int passes);
size_t dense_mfma_workspace_bytes(const slfp_conv2d_desc& d, int passes);
int launch_dense_mfma(const slfp_conv2d_desc& d, const ConvPlan& p, const float* x, const void* wblob,
                      const float* bias, const PostOp& post, float* y, void* workspace, hipStream_t stream);
// the same with 1-byte codes in and / or out (x_any: float32 or uint8 codes of QA(x / d.ka); y_any: float32 or uint8 codes)
bool dense_codes_applicable(const slfp_conv2d_desc& d, const ConvPlan& p, int post_flags, bool y_codes);
int launch_dense_mfma_io(const slfp_conv2d_desc& d, const ConvPlan& p, const void* x_any, const void* wblob, const float* bias,
                         const PostOp& post, void* y_any, void* workspace, const CodeIo& io, hipStream_t stream);
// what launch_dense_mfma_io decides for this layer under the switches read at load, printed from the selection it consumes
// (slfp_debug_dense_variant; host only).  "none" outside the family; valid until the next call on the same thread.
const char* dense_variant_name(const slfp_conv2d_desc& d, const ConvPlan& p, bool x_codes);
// is there a table-epilogue instance (CodeIo::lut) of the kernel launch_dense_mfma_io picks for this layer?  Host only.
bool dense_lut_applicable(const slfp_conv2d_desc& d, const ConvPlan& p, bool x_codes);
// codes: `w_oihw` points at 1-byte extended weight codes (slfp_encode_f32 | SLFP_FMT_EXT) instead of float32 weights
int launch_prepare_weights(const slfp_conv2d_desc& d, const ConvPlan& p, const float* w_oihw, void* wprep,
                           float* weight_q_oihw, hipStream_t stream, bool codes = false);

// large-kernel image stems on MFMA (conv_stem_mfma.hip); wblob = [kh*ksub + sub][nt][64][8] fp16;
// `workspace` receives the im2row'ed, encoded input
bool stem_mfma_applicable(const slfp_conv2d_desc& d, int passes);
void stem_mfma_blob_shape(const slfp_conv2d_desc& d, int* ksub, int* nt);
size_t stem_mfma_workspace_bytes(const slfp_conv2d_desc& d, int64_t w_out);
int launch_stem_mfma(const slfp_conv2d_desc& d, const ConvPlan& p, const float* x, const void* wblob,
                     const float* bias, const PostOp& post, float* y, void* workspace, hipStream_t stream);
// float32 in -> codes out (the YC forms): C_out a multiple of 16, no channel re-padding, no layer-output quantizer
bool stem_mfma_codes_applicable(const slfp_conv2d_desc& d, const ConvPlan& p, int post_flags);
// does the call run k_stem_im2row + k_stem_mfma (workspace needed) instead of k_stem_rows?  The code table counts in the
// rows form's LDS, so the answer can differ between float32 and code output.
bool stem_mfma_uses_workspace(const slfp_conv2d_desc& d, bool y_codes, bool u8 = false);
int launch_stem_mfma_io(const slfp_conv2d_desc& d, const ConvPlan& p, const float* x, const void* wblob, const float* bias,
                        const PostOp& post, void* y_any, void* workspace, const CodeIo& io, hipStream_t stream, const float* pix = nullptr);
// the k_stem_rows or k_stem_im2row + k_stem_mfma instance it runs, printed from the selection it consumes (slfp_debug_stem_instance)
const char* stem_mfma_instance_name(const slfp_conv2d_desc& d, const ConvPlan& p, const PostOp& post, const CodeIo& io, bool u8 = false);

// 3x3-class image stems whose whole contraction is one MFMA k-step (conv_stem_small.hip);
// wblob = [o/16][64][8] fp16 with k = (kh*KW + kw)*C_in + c
bool stem_small_applicable(const slfp_conv2d_desc& d, int passes);
int stem_small_tiles(const slfp_conv2d_desc& d);
int launch_stem_small(const slfp_conv2d_desc& d, const ConvPlan& p, const float* x, const void* wblob,
                      const float* bias, const PostOp& post, float* y, hipStream_t stream);
bool stem_small_codes_applicable(const slfp_conv2d_desc& d, const ConvPlan& p, int post_flags);   // float32 in -> codes out (C_out == 64)
int launch_stem_small_io(const slfp_conv2d_desc& d, const ConvPlan& p, const float* x, const void* wblob, const float* bias,
                         const PostOp& post, void* y_any, const CodeIo& io, hipStream_t stream, const float* pix = nullptr);
// the k_stem_small instance it runs, printed from the selection it consumes (slfp_debug_stem_instance)
const char* stem_small_instance_name(const slfp_conv2d_desc& d, const ConvPlan& p, const PostOp& post, const CodeIo& io, bool u8 = false);

// XCD-aware block remap (MI355X: 8 XCDs, blocks are dealt round-robin over them, so
// blocks b and b+8 share an L2).  Maps the hardware block id to a logical id such that
// each XCD owns a CONTIGUOUS range of logical ids: neighbouring tiles (shared halos,
// shared X rows of a column-split GEMM) then hit the same L2.  Bijective for any grid.
__device__ __forceinline__ uint32_t xcd_remap(uint32_t bid, uint32_t nblocks) {
    const uint32_t xcd = bid & 7u, slot = bid >> 3;
    const uint32_t q = nblocks >> 3, r = nblocks & 7u;
    const uint32_t base = xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q;
    return base + slot;
}

}  // namespace slfp
