// Internal types shared by the graph builder, the executor and the HIP kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <vector>

namespace yp {

enum DType { DT_BF16 = 0, DT_F32 = 1 };
enum Act { ACT_NONE = 0, ACT_SILU = 1, ACT_RELU = 2 };   // (ReLU: conv_igemm only - the U^2-Net path)

enum OpKind {
    OP_STEM = 0,      // u8 BGR NHWC -> first 3x3 s2 conv (+/255, BGR->RGB fused)
    OP_CONV = 1,      // dense conv k in {1,3}, s in {1,2}: implicit GEMM on MFMA, fused bias/SiLU/residual
    OP_DWCONV = 2,    // depthwise k in {3,7}
    OP_POOL5 = 3,     // max-pool 5x5 s1 p2 (SPPF)
    OP_UPSAMPLE = 4,  // nearest x2
    OP_ATTN = 5,      // PSA attention core: softmax(q^T k * scale) applied to v
    OP_HEAD = 6,      // DFL decode + sigmoid + two-stage top-k
    OP_CONVT = 7,     // ConvTranspose2d k2 s2 (Proto) = 4 strided 1x1 GEMMs
    OP_AMAX = 9,      // per-level class-max of the head (sigmoid(max_c logit)) - runs on the level's class lane
    OP_POOL3 = 8,     // SPPF: three chained 5x5 max-pools in one launch (out = first pooled slice, 3*C channels written)
};

// Channel slice of an NHWC tensor: element (b,y,x,c) at ((b*H+y)*W+x)*pix_stride + coff + c
struct View {
    int t = -1;    // tensor id
    int coff = 0;  // first channel
    int C = 0;     // channels in the slice
};

struct TensorDesc {
    std::string name;
    int C = 0;
    int sdiv = 1;        // spatial size = input size / sdiv
    bool f32 = false;    // fp32 regardless of engine dtype (head logits)
    // resolved by the plan:
    int H = 0, W = 0;
    size_t bytes = 0;
    void* ptr = nullptr;
};

struct WeightDesc {
    std::string name;    // folded name, e.g. "model.2.cv1" ; parameters "<name>.weight" / "<name>.bias"
    int cout = 0, cin_g = 0, k = 1, groups = 1;
    int cin_pad = 0;           // dense convs: channels per tap in the PACKED matrix (= cin_g rounded up to 32 when that is not a multiple of 32
                               // and > 32; zero weights in the gap) - the conv kernels then run with Cin = cin_pad, see engine.hip conv_params
    bool transposed = false;   // ConvTranspose2d layout [Cin][Cout][k][k]
    bool is_stem = false;
    bool have_w = false, have_b = false;
    std::vector<float> w, b;   // host fp32 copies until finalize
    // device, packed
    void* d_w = nullptr;       // layout depends on the consumer kernel
    void* d_w2 = nullptr;      // stem only: bf16 [C0][32] GEMM layout for the MFMA stem
    float* d_b = nullptr;
    int Kpad = 0;
    size_t mat_bytes = 0;      // bytes of one packed GEMM matrix
};

// How a launching op runs (a plan decision). The ops whose work a fused form takes over are skipped. engine.hip's kForms has one record
// per value, in this order: candidates, admission, effective views and launch of a form are all there.
enum Form {
    FORM_PLAIN = 0,       // the op's own kernel
    FORM_DWPW,            // OP_CONV 1x1: the depthwise 3x3 in front (fuse_dw) and this conv as conv_dwpw_kernel
    FORM_DWPW_TAIL,       // OP_CONV 1x1 logits: dw -> pw (fuse_tail) -> this conv (+ the class-max keys of tail_amax) as conv_dwpw_kernel's TAIL form
    FORM_S2PW,            // OP_CONV 1x1: the 3x3 s2 conv in front (fuse_pre) and this conv as conv_halo_s2's PW2 form
    FORM_FRONTEND,        // OP_CONV 1x1: stem (stem_op) -> 3x3 s2 (fuse_pre) -> this conv as frontend_kernel
    FORM_C2F,             // OP_CONV 1x1: the bottleneck's two 3x3 convs (c2f_m1, c2f_m2) and this conv as c2f_fused_kernel
    FORM_SCDOWN,          // OP_DWCONV 3x3 s2: the 1x1 in front (scd_pre) and this op as scdown_fused_kernel
    FORM_PWSP,            // OP_DWCONV / OP_POOL3: the 1x1 in front (pw_pre) and this op as pwsp_kernel
    FORM_CLS_OUT,         // OP_CONV logits: logits and the class-max keys of amax_post in one cls_out_kernel launch
};

struct Op {
    int kind = OP_CONV;
    std::string name;
    View in, out, res;
    int widx = -1;
    int k = 1, s = 1, act = ACT_NONE;
    int gs = 0, gstride = 0;      // depthwise input channel gather: in_ch = coff + (c/gs)*gstride + c%gs (gs=0: identity)
    int nh = 0, kd = 0, hd = 0;   // attention
    View box[3], cls[3], cf[3];   // head inputs per level
    View amax[3];                 // head: per-level anchor-max keys (written by the OP_AMAX ops)
    int nlev = 0;
    double flops = 0, bytes = 0;  // algorithmic (filled by the plan)
    std::string kernel;           // device kernel symbol this op launches (filled by the plan)
    int cfg = -1;                 // autotuned conv_dma configuration (-1: heuristic)
    int fuse_dw = -1;             // OP_CONV 1x1: index of the depthwise 3x3 op feeding it that can be fused in (graph pass)
    Form form = FORM_PLAIN;       // plan decision: launch form
    bool skip = false;            // plan decision: this op's work is done by a fused consumer
    int fuse_pre = -1;            // OP_CONV 1x1: index of the 3x3 stride-2 conv feeding it that can run as the first stage of one kernel
    int stem_op = -1;             // OP_CONV 1x1 with fuse_pre: index of the stem op when that 3x3 is the only reader of the stem's output (graph pass)
    int fold_up = -1;             // OP_CONV 1x1 on a [upsampled | skip] concat: index of the nearest-x2 upsample op it can absorb
    bool folded = false;          // plan decision: the upsample is folded into this conv's input gather
    int c2f_m1 = -1, c2f_m2 = -1; // OP_CONV 1x1 closing a C2f with one plain bottleneck: indices of the bottleneck's two 3x3 convs
    int scd_pre = -1;             // OP_DWCONV 3x3 s2 closing an SCDown: index of the 1x1 conv in front of it
    int fuse_tail = -1, tail_amax = -1;   // OP_CONV 1x1 without activation (fp32 logits): index of the dw->pw pointwise conv feeding it that can take it
                                  // on as a third stage, and of the OP_AMAX op behind it (or -1)
    int amax_post = -1;           // OP_CONV 1x1 that writes a level's fp32 class logits: index of the OP_AMAX op that reads them (graph pass)
    int pw_pre = -1;              // OP_DWCONV (3x3 / 7x7, stride 1) / OP_POOL3: index of the 1x1 conv that produces its input and can run as the first stage of pwsp_kernel (graph pass)
    bool pw_store = false;        // FORM_PWSP: the 1x1's own output has other readers and is written as well
    int lane = 0;                 // capture lane: independent head branches run on their own streams inside the hipGraph
    bool nms = false;             // OP_HEAD: conf filter + class-aware NMS (YOLOv8 / YOLO11) instead of the two-stage top-k (v10)
    int hb_box[3][3] = {{-1, -1, -1}, {-1, -1, -1}, {-1, -1, -1}}, hb_cf[3][3] = {{-1, -1, -1}, {-1, -1, -1}, {-1, -1, -1}};   // OP_HEAD (v10): op indices of the box / coefficient branch convs per level ({0,1,2} = 3x3, 3x3, 1x1), -1 = none
    bool sparse_box = false, sparse_cf = false;   // plan decision: that branch runs on the stage-1 winners only (head_branch.hip); its dense ops are skipped
};

// ---------------------------------------------------------------------------------------------------------
// Kernel parameter blocks (passed by value)
// ---------------------------------------------------------------------------------------------------------
struct ConvParams {
    const void* x; int x_stride, x_coff;        // input view (elements)
    int H, W, Cin;
    const void* w; int Kpad;                    // packed [CoutPad][Kpad], k order (ky,kx,ci)
    const float* bias;
    void* y; int y_stride, y_coff; int Ho, Wo, Cout;
    const void* res; int res_stride, res_coff;  // nullable; added after the activation
    int M;                                      // B*Ho*Wo
    int ks, stride, pad;
    int act, out_f32;
    int up, oy, ox;                             // output pixel (ho,wo) -> (ho*up+oy, wo*up+ox) in an (Ho*up,Wo*up) image
    size_t x_bytes, w_bytes, y_bytes;           // extents of the x / packed-weight / y buffers (buffer descriptors)
    int cfg;                                    // conv_dma tile configuration (-1: heuristic)
    int dbg;                                    // timing ablations (tests/tools only): 1 = drop stores, 2 = drop pixel loads
    // folded nearest-x2 upsample (1x1 convs on a [upsampled | skip] concat): input channels [0, x2_C) are read from the
    // low-resolution tensor x2 at pixel (ho >> 1, wo >> 1) instead of from x; channels >= x2_C come from x as usual
    const void* x2; size_t x2_bytes; int x2_stride, x2_coff, x2_C, x2_H, x2_W;
    // fused trailing 1x1 (conv_halo_s2 PW2 form): y = act2(W2 . act(conv(x)) + bias2); Cout is then the intermediate width,
    // y / y_stride / y_coff / y_bytes describe the FINAL output of C2 channels
    const void* w2; const float* bias2; int C2, act2, Kpad2; size_t w2_bytes;
    unsigned long long* clk;                    // debug (YOLOP_LC_CLOCKS=1, conv_dma_lc only): per-wave phase clocks, else null
    int dil;                                    // dilation of a 3x3 (0 = 1); conv_igemm only - the U^2-Net path (pad = dil there)
    // conv_small only: x is the tensor IN FRONT OF a 2x2 / stride-2 / ceil-mode max pool (src_H x src_W pixels) and the pool is taken
    // while loading; H, W stay the pooled size the convolution sees
    int pool_in, src_H, src_W;
    // conv_small only: the x2 channels are a BILINEAR resize (align_corners = False) of x2 to H x W instead of the nearest x2 above
    int up_bilinear;
    // bf16 epilogues: 1 = the engine asks for the paired channel order (16-byte stores, kernel_util.h). A launcher passes it on to its
    // kernel only where wide_store_ok holds, so in a kernel it means "this launch is paired": weight fill and epilogue read the same flag
    int wide;
};

struct DwParams {
    const void* x; int x_stride, x_coff; int H, W, C;
    const void* w;             // packed [k*k][C]
    const float* bias;
    void* y; int y_stride, y_coff; int Ho, Wo;
    const void* res; int res_stride, res_coff;
    int B, ks, stride, pad, act;
    int gs, gstride;
    size_t x_bytes;            // extent of the x tensor (buffer descriptor of the row kernels)
};

struct StemParams {
    const uint8_t* x; int H, W;       // [B,H,W,3] BGR
    const float* w;                   // [3][3][3(bgr)][C0]
    const void* wpk;                  // bf16 [C0][32], k = (ky,kx,c_bgr), zero padded (MFMA stem); may be null
    const float* bias;
    void* y; int y_stride, y_coff; int Ho, Wo, C0; int B;
    int act;
};

// fused front end (frontend.hip): stem -> 3x3 s2 conv -> 1x1 conv
struct FrontParams {
    const uint8_t* img; int imgH, imgW, B;                               // [B,imgH,imgW,3] BGR u8
    const void* w0; const float* bias0; int act0, C0; int H1, W1;         // stem: bf16 [C0][32], output grid H1 x W1
    const void* w1; const float* bias1; int act1, C1, Kpad1; size_t w1_bytes;   // 3x3 s2: packed [C1^][9*C0]
    const void* w2; const float* bias2; int act2, C2, Kpad2; size_t w2_bytes;   // 1x1:    packed [C2^][C1]
    void* y; int y_stride, y_coff; size_t y_bytes; int Ho, Wo;           // final output view (Ho x Wo = H1/2 x W1/2)
    unsigned long long* clk;                                              // debug (YOLOP_FRONT_CLOCKS=1): per-wave stage clocks, else null
};
bool frontend_valid(const FrontParams& p);
hipError_t launch_frontend(const FrontParams& p, hipStream_t st);

// fused C2f tail (c2f_fused.hip): [a | b] -> 3x3 -> 3x3 (+ b) -> 1x1 over [a | b | c]
struct C2fParams {
    const void* x; int x_stride, x_coff; size_t x_bytes;                 // the concat buffer: a = channels [coff, coff+C), b = the next C
    int B, H, W, C;
    const void* w1; const float* bias1; int act1, Kpad1; size_t w1_bytes;   // m.0.cv1: packed [C^][9*C]
    const void* w2; const float* bias2; int act2, Kpad2; size_t w2_bytes;   // m.0.cv2: packed [C^][9*C]
    int shortcut;                                                         // c += b
    const void* w3; const float* bias3; int act3, Kpad3, Cout; size_t w3_bytes;   // cv2: packed [Cout^][3*C]
    void* y; int y_stride, y_coff; size_t y_bytes;
    unsigned long long* clk;                                              // debug (YOLOP_C2F_CLOCKS=1): per-wave stage clocks, else null
    int wide;                                                             // the final 1x1's paired channel order is asked for (ConvParams::wide); the launcher decides
};
bool c2f_fused_valid(const C2fParams& p);

// fused SCDown (scdown_fused.hip): 1x1 conv + act -> depthwise 3x3 stride 2
struct ScdParams {
    const void* x; int x_stride, x_coff; size_t x_bytes; int B, H, W, K;          // input view [B,H,W,K]
    const void* w1; const float* bias1; int act1, Kpad1, C; size_t w1_bytes;        // 1x1: packed [C^][K]
    const void* wd; const float* biasd; int actd;                                    // depthwise 3x3 s2: packed [9][C] bf16, bias fp32
    void* y; int y_stride, y_coff; size_t y_bytes; int Ho, Wo;
    unsigned long long* clk;                                                          // debug (YOLOP_SCD_CLOCKS=1), else null
};
bool scdown_fused_valid(const ScdParams& p);
const char* scdown_fused_kernel_name(const ScdParams& p);
bool scdown_stream_valid(const ScdParams& p);                     // the streaming form for 256 output channels (scdown_stream.hip)
const char* scdown_stream_kernel_name(const ScdParams& p);
hipError_t launch_scdown_stream(const ScdParams& p, hipStream_t st);
hipError_t launch_scdown_fused(const ScdParams& p, hipStream_t st);
hipError_t launch_c2f_fused(const C2fParams& p, hipStream_t st);

struct PoolParams {
    const void* x; int x_stride, x_coff;
    void* y; int y_stride, y_coff;
    int B, H, W, C;
};

struct UpParams {
    const void* x; int x_stride, x_coff;
    void* y; int y_stride, y_coff;
    int B, H, W, C;   // input dims; output 2H x 2W
};

struct AttnParams {
    const void* qkv; int q_stride, q_coff;   // [B,N,nh*(2kd+hd)]
    void* o; int o_stride, o_coff;           // [B,N,nh*hd]
    int B, N, nh, kd, hd;
    float scale;
};

struct HeadParams {
    const float* box[3]; const float* cls[3]; const float* cf[3];   // fp32 NHWC logits per level
    int hw[3][2]; int nlev;
    int B, nc, max_det, A;
    float* det; int32_t* idx; float* coeff;   // user outputs
    void* scratch;                            // device scratch, head_scratch_bytes(B, A)
    const unsigned* mk[3];                    // per-level anchor-max keys [B][HW_l] (bits of sigmoid(max_c logit)); when set, the
                                              // class-max pass already ran (OP_AMAX) and `scratch` is not used
    // NMS heads (YOLOv8 / YOLO11, head_nms.hip): device parameters [conf, iou] and per-image candidate scratch [B][A][8] floats
    const float* nms_params;
    float* nms_ws;
    // winners-only head (round 3): stage 1 leaves its winners in sp_sel / sp_wlist / sp_wcount / sp_thr, the branch kernel(s) fill
    // sp_box [B][max_det][64] (and sp_cf [B][max_det][32]), stage 2 + decode read those rows by rank instead of box[] / cf[]
    int* sp_sel; int* sp_wlist; int* sp_wcount; unsigned* sp_thr; float* sp_box; float* sp_cf;
    int* sp_plist; int* sp_pcount; int sp_plist_off[3], sp_plist_cap[3];   // needed positions per level (see HeadBranchParams); null = not wanted
};
hipError_t launch_head_stage1(const HeadParams& p, hipStream_t st);
hipError_t launch_head_stage2(const HeadParams& p, hipStream_t st);
constexpr int HEAD_MAXK = 512;
// The box / mask-coefficient branch of the v10 one-to-one head evaluated at the stage-1 winners only (head_branch.hip)
struct HeadBranchParams {
    const void* x[3]; int x_stride[3], x_coff[3], H[3], W[3], Cin[3]; size_t x_bytes[3];     // the levels' feature maps (bf16 NHWC views)
    const void* w0[3]; int Kpad0[3]; const float* b0[3];                                       // 3x3 Cin -> cmid, packed [cmid^][9*Cin]
    const void* w1[3]; int Kpad1[3]; const float* b1[3];                                       // 3x3 cmid -> cmid
    const void* w2[3]; int Kpad2[3]; const float* b2[3];                                       // 1x1 cmid -> cout, no activation
    int act0, act1;
    int B, max_det, maxk, cmid, cout;
    int A0, A1;                                   // anchors of level 0 / 1 (anchor id -> level-local pixel)
    const int* sel;                               // [B][maxk] stage-1 winners (anchor ids, rank order)
    const int* wlist;                             // [B][3][maxk] ranks of the winners that lie on a level
    const int* wcount;                            // [B][3]
    float* out;                                   // [B][max_det][cout] fp32 rows by rank
    // positions form (head_pos_kernel + head_win_kernel): the first 3x3 once per NEEDED position (the union of the winners' in-frame 3x3
    // neighbourhoods, listed by the stage-1 kernel), its output in a position-addressed map that the winners' second 3x3 gathers from
    const int* plist; const int* pcount;          // per level: entries image << 20 | level-local pixel; pcount[3]
    int plist_off[3], plist_cap[3];               // level l's list = plist + plist_off[l], at most plist_cap[l] entries
    void* t0; size_t t0_off[3], t0_bytes;         // bf16 [level][B][H_l*W_l][cmid]: element offset of level l
    int pos_grid;                                 // workgroups of the (persistent) position kernel
};
bool head_branch_valid(const HeadBranchParams& p);
hipError_t launch_head_branch(const HeadBranchParams& p, hipStream_t st);
// `options`: the forms that honour the class set, the agnostic flag and max_nms (yp_set_nms_options) - kernels of their own, so the
// default forms keep their registers and LDS. They read the words behind [conf, iou] in the device block `nms_params`:
constexpr int NMS_OPT_AGNOSTIC = 2, NMS_OPT_MAX_NMS = 3, NMS_OPT_USE_CLASSES = 4, NMS_OPT_MASK = 5;   // word indices (uint32)
constexpr int NMS_MASK_WORDS = 32;                                                                    // class bit mask: nc <= 1024
constexpr int NMS_PARAM_WORDS = NMS_OPT_MASK + NMS_MASK_WORDS;
constexpr int NMS_DEFAULT_MAX_NMS = 16384;                                                             // head_nms_common.h NCAP
hipError_t launch_head_nms(const HeadParams& p, hipStream_t st, bool options = false);
const char* head_nms_kernel_name(int A, bool options);
size_t head_nms_scratch_bytes(int B, int A);
hipError_t launch_head_nms_large(const HeadParams& p, hipStream_t st, bool options = false);    // head_large.hip: A > HEAD_LDS_ANCHORS

// Experiment switches (YOLOP_* environment variables). env_on: set and its first character is '1'; env_int: atoi of the value, dflt when
// unset. A launcher keeps the result in a function-local static, so a switch is read once, at the first use of that function.
inline bool env_on(const char* name) { const char* v = std::getenv(name); return v && *v == '1'; }
inline int env_int(const char* name, int dflt) { const char* v = std::getenv(name); return v ? atoi(v) : dflt; }

// Lets `kern` be launched with `bytes` of dynamic LDS. Nothing to do up to the 64 KiB every kernel may have, or when `granted` (the caller's
// `static size_t granted = 0`, one per kernel instantiation) already covers it; else the kernel's limit goes to the most the device has for
// it, once: 160 KiB less the kernel's static LDS, which comes out of the same 160 KiB (asking for more is an invalid value). The attribute
// only permits an allocation: a launch still gets just the LDS it asks for. The engine runs one process per GPU (parallel.py), so a
// per-process static is the right lifetime for `granted`.
inline hipError_t allow_dynamic_lds(const void* kern, size_t bytes, size_t& granted) {
    if (bytes <= 64 * 1024 || bytes <= granted) return hipSuccess;
    hipFuncAttributes fa;
    if (hipError_t e = hipFuncGetAttributes(&fa, kern)) return e;
    const size_t most = 160 * 1024 - fa.sharedSizeBytes;
    if (hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)most)) return e;
    granted = most;
    return hipSuccess;
}

// The paired (16-byte) store form of a bf16 conv epilogue, decided per launch from the parameters alone (no tuner decision, no
// configuration id): `frags` = 16-channel fragments per wave, `Cout` etc. of the kernel's FINAL store. It needs fragment pairs (even
// frags), Cout in whole pairs (32 channels) and 16-byte aligned channel slices of y and of the residual; anything else - v10-N's narrow
// layers, odd head widths, the fp32 outputs, YOLOP_NARROW_STORE=1 (want = 0) - takes the 8-byte form.
// Test hook (yp_debug_last_store_form): what the last launch that can take either form took. Recorded only once the hook has been called,
// so a production launch writes no shared state; atomics, as two engines may launch from two threads.
inline std::atomic<bool>& store_form_watched() { static std::atomic<bool> v{false}; return v; }
inline std::atomic<int>& last_store_form() { static std::atomic<int> v{-1}; return v; }
inline bool wide_store_ok(int want, int frags, int Cout, int y_stride, int y_coff, bool out_f32, const void* res = nullptr, int res_stride = 0, int res_coff = 0) {
    const bool ok = want && !out_f32 && frags > 0 && (frags & 1) == 0 && (Cout % 32) == 0 && (y_stride & 7) == 0 && (y_coff & 7) == 0 &&
                    (!res || ((res_stride & 7) == 0 && (res_coff & 7) == 0));
    if (store_form_watched().load(std::memory_order_relaxed)) last_store_form().store(ok ? 1 : 0, std::memory_order_relaxed);
    return ok;
}
inline ConvParams with_store_form(const ConvParams& p, int frags) {
    ConvParams q = p;
    q.wide = wide_store_ok(p.wide, frags, p.Cout, p.y_stride, p.y_coff, p.out_f32 != 0, p.res, p.res_stride, p.res_coff) ? 1 : 0;
    return q;
}

// Test hook (yp_debug_max_workgroups): an upper bound on the grid of the persistent kernels with a counted wait in front of a tile
// (conv_wres, conv_dwpw_stream, c2f_fused), 0 = none.
// With it a small input makes a workgroup walk several tiles - the counted vmcnt in front of a tile is exercised from the second tile on.
// Read by the launchers only; a kernel whose workgroup mapping needs whole rounds (conv_wres: 8 tile lanes per channel block) stops there.
inline std::atomic<int>& debug_max_workgroups_ref() { static std::atomic<int> v{0}; return v; }
inline int debug_max_workgroups() { return debug_max_workgroups_ref().load(std::memory_order_relaxed); }

// launches (implemented in the .hip files); dtype selects the template instance
hipError_t launch_conv(const ConvParams& p, int dtype, hipStream_t st);
hipError_t launch_conv_igemm(const ConvParams& p, int dtype, hipStream_t st);   // always the register-staged kernel (dilation, ReLU, any Cin % 8 == 0)
std::string conv_kernel_name(const ConvParams& p, int dtype);
bool conv_cfg_usable(const ConvParams& p, int dtype, int cfg);   // a configuration id from a cache file / yp_tuning_import is launchable for p
bool conv_dma_supported(const ConvParams& p);
int conv_dma_requested_cfg(const ConvParams& p);                 // conv_dma's configuration for p when forced or tuned (valid for p), else -1
int conv_launch_cfg(const ConvParams& p, int dtype);             // the configuration id launch_conv runs p with, -1 = a heuristic's pick
void conv_dma_force_cfg(int cfg);
int conv_dma_forced_cfg();
void conv_set_debug_ablation(int v);
int conv_debug_ablation();
bool tile_balance_enabled(int family);  // tiles sized to whole rounds of workgroups? family 1 = conv_pxd, 2 = conv_wres, 4 = cls_out; YOLOP_BALANCE=<mask> (A/B switch)

// One tile-kernel family of the dense conv. A configuration id (Op::cfg, ConvParams::cfg, the tune tables) in [base, base + num_cfgs) is
// configuration id - base of that family; -1 is the heuristic (conv_dma or conv_igemm) and PWSP_CFG is launched by the engine itself.
// conv_igemm.hip's kConvFamilies lists every family, in the order the autotuner times them.
struct ConvFamily {
    int base, num_cfgs;
    bool (*valid)(const ConvParams& p, int c);
    std::string (*symbol)(const ConvParams& p, int c);                    // the full kernel symbol launch() runs for p
    hipError_t (*launch)(const ConvParams& p, int c, hipStream_t st);
    bool two_source;                                                      // implements the folded-upsample gather (x2_C > 0)
    const char* tune_env;                                                 // the tuner's A/B switch, null = always a candidate
    bool opt_in;                                                          // tune_env = 1 adds the family instead of removing it
};
// Tile configurations (host side). A configuration is a type that states its kernel's leading template arguments ONCE: a family's
// `template <int...> struct X : Cfg<...>` with the tile sizes its valid() reads as constexpr members. A family is the CfgList of its
// configurations in id order; validity, the reported symbol and the launch all go through with_cfg, so they cannot name different instances.
template <int... V> struct Cfg {};
template <class... C> struct CfgList { static constexpr int size = (int)sizeof...(C); };
// f(C{}) for the c-th configuration of the list; c out of range: hipErrorInvalidValue for a launch, else an empty value (no name, not valid)
template <class F, class... C> auto with_cfg_of(CfgList<C...>, int c, F& f) {
    using R = std::common_type_t<decltype(f(C{}))...>;
    R r{};
    if constexpr (std::is_same_v<R, hipError_t>) r = hipErrorInvalidValue;
    int i = 0;
    ((i++ == c ? (void)(r = f(C{})) : (void)0), ...);
    return r;
}
template <class List, class F> auto with_cfg(int c, F f) { return with_cfg_of(List{}, c, f); }
// "256,128,4,2,32,4" of a Cfg<256,128,4,2,32,4>, ",true,false" of {true, false}
template <int... V> std::string cfg_args(Cfg<V...>) {
    std::string s;
    ((s += (s.empty() ? "" : ",") + std::to_string(V)), ...);
    return s;
}
inline std::string bool_args(std::initializer_list<bool> bs) {
    std::string s;
    for (bool b : bs) s += b ? ",true" : ",false";
    return s;
}
// the symbol kernel<V..., variant arguments>
template <class K> std::string cfg_symbol(const char* kernel, K k, const std::string& variant = "") { return std::string(kernel) + "<" + cfg_args(k) + variant + ">"; }
// HAS_RES, OUT_F32 of the persistent conv kernels: out_f32 first (fp32 logits never carry a residual), then res, else neither
template <class F> auto with_res_f32(const ConvParams& p, F f) {
    if (p.out_f32) return f(std::false_type{}, std::true_type{});
    if (p.res) return f(std::true_type{}, std::false_type{});
    return f(std::false_type{}, std::false_type{});
}
inline std::string res_f32_args(const ConvParams& p) { return with_res_f32(p, [](auto res, auto f32) { return bool_args({res, f32}); }); }
// store side of the kernels whose epilogue has only the 4-channel vector form, through buffer descriptors
inline bool conv_store_side_ok(const ConvParams& p) {
    if ((p.Cout & 3) || (p.y_stride & 3) || (p.y_coff & 3) || (p.res && ((p.res_stride & 3) || (p.res_coff & 3)))) return false;
    if (p.res && p.out_f32) return false;
    return p.x_bytes < (1ull << 31) && p.w_bytes < (1ull << 31) && p.y_bytes < (1ull << 31);
}
// conv_dma (ids 0..) picks its configuration from p.cfg / the forced id itself and ignores c; conv_halo_s2 launches its fused trailing 1x1
// form when p.C2 > 0 (configuration from conv_halo_s2_pw_cfg)
extern const ConvFamily conv_dma_family, conv_halo_family, conv_halo_p_family, conv_dma_p_family, conv_dma_lc_family, conv_halo_s2_family,
    conv_tile1_family, conv_wreg_family, conv_pxd_family, conv_ks_family, conv_wres_family, conv_wrs_family;
constexpr int kNumConvFamilies = 12;
extern const ConvFamily* const kConvFamilies[kNumConvFamilies];
int conv_halo_s2_pw_cfg(const ConvParams& p);          // configuration for the fused trailing-1x1 form, or -1
size_t conv_halo_s2_lds_bytes(const ConvParams& p, int c);   // dynamic LDS of the launch of configuration c (id - 500) of conv_halo_s2 for p, 0 = no such c
int conv_halo_s2_lds_weights(int on);                  // 1 = conv_halo_s2 keeps its weights in LDS everywhere (A/B, tests), 0 = off, < 0 = read; returns the previous value
hipError_t launch_dwconv(const DwParams& p, int dtype, hipStream_t st);
std::string dwconv_kernel_name(const DwParams& p, int dtype);    // the kernel launch_dwconv runs for p
hipError_t launch_stem(const StemParams& p, int dtype, hipStream_t st);
std::string stem_kernel_name(const StemParams& p, int dtype);    // the kernel launch_stem runs for p
hipError_t launch_pool5(const PoolParams& p, int dtype, hipStream_t st);
hipError_t launch_sppf_pool3(const PoolParams& p, int dtype, hipStream_t st);
bool sppf_pool3_fits(const PoolParams& p, int dtype);
bool dwconv_mfma_valid(const DwParams& p, int dtype);
hipError_t launch_dwconv_mfma(const DwParams& p, hipStream_t st);
const char* dwconv_mfma_kernel_name(const DwParams& p);
hipError_t launch_upsample(const UpParams& p, int dtype, hipStream_t st);
// wgs > 0: the matrix-core form's workgroup target for this call (0: YOLOP_ATTN_WGS, else 256); *kernel_out = 1 matrix-core form, 0 generic
// Attention form of an engine (yp_set_attention_form): AUTO = the resident matrix-core kernel up to 400 tokens, the generic kernel beyond;
// STREAM = calls in attention_stream_scope with more than 400 tokens take attention_stream_kernel (no token bound), the rest is AUTO.
// STREAM_WIDE = STREAM, and calls in attention_stream_wide_scope (key_dim 36, head_dim 72) take attention_stream_wide_kernel at every
// token count. The value is a bit set: bit 0 the streaming kernel for 32/64 heads, bit 1 the wide-head one, which is a streaming kernel
// too: bit 1 alone is no form.
enum AttnForm { ATTN_FORM_AUTO = 0, ATTN_FORM_STREAM = 1, ATTN_FORM_STREAM_WIDE = 3 };
inline bool attn_form_valid(int form) { return form == ATTN_FORM_AUTO || form == ATTN_FORM_STREAM || form == ATTN_FORM_STREAM_WIDE; }
constexpr int ATTN_RESIDENT_TOKENS = 400;
// kernel_out: 0 generic, 1 resident matrix-core, 2 streaming matrix-core, 3 streaming matrix-core for 36/72 heads, 4 streaming matrix-core
// in fp32, 5 streaming matrix-core in fp32 for 36/72 heads. f32_stream is an engine's fp32 switch (yp_set_attention_f32_stream),
// orthogonal to the form and a bit set like it: bit 0 (ATTN_F32_STREAM) - fp32 calls in attention_stream_f32_scope with more than 400
// tokens take attention_stream_f32_kernel (no token bound); bit 1 - fp32 calls in attention_stream_wide_f32_scope (key_dim 36, head_dim 72)
// with more than 400 tokens take attention_stream_wide_f32_kernel. Bit 1 alone is no value: 0, 1 and 3 (ATTN_F32_STREAM_WIDE) are. Off,
// nothing changes.
enum AttnF32 { ATTN_F32_GENERIC = 0, ATTN_F32_STREAM = 1, ATTN_F32_STREAM_WIDE = 3 };
inline bool attn_f32_valid(int v) { return v == ATTN_F32_GENERIC || v == ATTN_F32_STREAM || v == ATTN_F32_STREAM_WIDE; }
hipError_t launch_attention(const AttnParams& p, int dtype, hipStream_t st, int wgs = 0, int* kernel_out = nullptr, int form = ATTN_FORM_AUTO,
                            int f32_stream = ATTN_F32_GENERIC);
// the predicate of launch_attention, for the planner; *max_tokens = the generic kernel's bound for p's head sizes
bool attention_fits(const AttnParams& p, int dtype, int* max_tokens, int form = ATTN_FORM_AUTO, int f32_stream = ATTN_F32_GENERIC);
bool attention_takes_stream(const AttnParams& p, int dtype, int form);     // launch_attention would launch attention_stream_kernel
bool attention_takes_stream_wide(const AttnParams& p, int dtype, int form);    // ... attention_stream_wide_kernel
// attention_stream.hip
bool attention_stream_scope(const AttnParams& p, int dtype);
void attention_stream_split(int B, int N, int nh, int wgs, int* nsplit_out, int* gpw_out);
hipError_t launch_attention_stream(const AttnParams& p, hipStream_t st, int wgs);
// attention_stream_wide.hip
bool attention_stream_wide_scope(const AttnParams& p, int dtype);
hipError_t launch_attention_stream_wide(const AttnParams& p, hipStream_t st, int wgs);
// attention_stream_f32.hip
bool attention_takes_stream_f32(const AttnParams& p, int dtype, int f32_stream);    // launch_attention would launch attention_stream_f32_kernel
bool attention_stream_f32_scope(const AttnParams& p, int dtype);
hipError_t launch_attention_stream_f32(const AttnParams& p, hipStream_t st, int wgs);
// attention_stream_wide_f32.hip
bool attention_takes_stream_wide_f32(const AttnParams& p, int dtype, int f32_stream);    // ... attention_stream_wide_f32_kernel
bool attention_stream_wide_f32_scope(const AttnParams& p, int dtype);
hipError_t launch_attention_stream_wide_f32(const AttnParams& p, hipStream_t st, int wgs);
// conv_small.hip: fp32 3x3 for small maps (four waves split K, operands straight from L2)
bool conv_small_valid(const ConvParams& p, int dtype);
hipError_t launch_conv_small(const ConvParams& p, int dtype, hipStream_t st);
// conv_halo_f32.hip: fp32 3x3 for large maps (8 x 32 pixel tiles, halo patch + weights by LDS-DMA, 16-channel chunks)
bool conv_halo_f32_valid(const ConvParams& p, int dtype);
hipError_t launch_conv_halo_f32(const ConvParams& p, int dtype, hipStream_t st);
hipError_t launch_head(const HeadParams& p, hipStream_t st);
hipError_t launch_letterbox(const uint8_t* src, int h0, int w0, uint8_t* dst, int out_h, int out_w, int new_h, int new_w, int top,
                            int left, int pad, hipStream_t st);
hipError_t launch_letterbox_batch(const uint8_t* src, int n, int h0, int w0, uint8_t* dst, int out_h, int out_w, int new_h, int new_w,
                                  int top, int left, int pad, hipStream_t st);
size_t head_scratch_bytes(int B, int A);
// More anchors than one workgroup's LDS holds (head_large.hip): chunks of HEAD_LDS_ANCHORS select in parallel, one workgroup per image merges
// their winners - at most HEAD_LDS_ANCHORS of them, HEAD_MAXK per chunk, hence the bound on A.
constexpr int HEAD_LDS_ANCHORS = 12288;
constexpr int HEAD_MAX_ANCHORS = HEAD_LDS_ANCHORS * (HEAD_LDS_ANCHORS / HEAD_MAXK);
inline int head_large_chunks(int A) { return (A + HEAD_LDS_ANCHORS - 1) / HEAD_LDS_ANCHORS; }
inline size_t head_large_ckeys_offset(int B, int A) { return ((size_t)B * A * sizeof(unsigned) + 255) & ~(size_t)255; }      // in HeadParams::scratch
hipError_t launch_head_large(const HeadParams& p, int mode, hipStream_t st);      // mode 0: whole head, 1: stage 1 (winners hand-over)
const char* head_large_kernel_name(int mode);
hipError_t head_read_clocks(unsigned long long* out8);
hipError_t head_branch_read_clocks(unsigned long long* out8);
hipError_t launch_copy_out(const float* det, float* det_out, const int32_t* idx, int32_t* idx_out, const float* coeff, float* coeff_out,
                           size_t rows, hipStream_t st);
hipError_t launch_anchor_max_level(const float* cls, int B, int HW, int nc, unsigned* out, hipStream_t st);

struct DwPwParams {                              // fused depthwise 3x3 s1 -> pointwise 1x1 (conv_dwpw.hip)
    const void* x; int x_stride, x_coff; int B, H, W, C; size_t x_bytes;
    const void* w_dw; const float* b_dw; int act_dw;            // depthwise: packed [9][C] bf16, bias fp32
    const void* w_pw; int Kpad; size_t wpw_bytes; const float* b_pw; int act_pw;   // pointwise: packed [Cout^][Kpad]
    void* y; int y_stride, y_coff; size_t y_bytes; int Cout; int out_f32;
    unsigned long long* clk;                                    // debug (YOLOP_DWPW_CLOCKS=1): per-wave phase clocks, else null
    int wide;                                                   // conv_dwpw_stream: the paired channel order is asked for (ConvParams::wide); its launcher decides (wide_store_ok)
    // TAIL form (round 3): a trailing 1x1 (the class branch's logit conv, no activation, fp32 output) runs as a third stage on the tile
    // while it is still in LDS: y3 = W3 . act_pw(pointwise(...)) + b3; the pointwise result itself is NOT written (y is unused). When
    // `keys` is set, the per-pixel class maximum goes out as well: keys[b*H*W + pixel] = bits of sigmoid(max_c y3) (what OP_AMAX makes)
    const void* w3; int Kpad3; size_t w3_bytes; const float* b3; int C3;
    float* y3; int y3_stride, y3_coff; size_t y3_bytes;
    unsigned* keys;
};
bool dwpw_stream_valid(const DwPwParams& p);                    // the streaming form for 128-channel inputs (conv_dwpw_stream.hip)
hipError_t launch_dwpw_stream(const DwPwParams& p, hipStream_t st);
// pointwise 1x1 -> per-channel spatial operator, one workgroup per (image, channel slice) (pwsp.hip): the small-map layers
struct PwSpParams {
    const void* x; int x_stride, x_coff; size_t x_bytes; int B, H, W, K;           // input view [B,H,W,K]
    const void* w1; const float* bias1; int act1, Kpad1, C1; size_t w1_bytes;       // 1x1: packed [C1^][K]
    void* y1; int y1_stride, y1_coff;                                              // the pointwise result's own tensor (null: not stored)
    const void* res1; int res1_stride, res1_coff;                                   // added to the pointwise result after act1 (sp = 0 only; nullable)
    int sp;                                                                         // 0 none, 1 depthwise 3x3, 2 depthwise 7x7, 3 SPPF's three chained 5x5 max-pools
    int sp_c0, Csp;                                                                 // the spatial operator reads channels [sp_c0, sp_c0 + Csp) of the pointwise result
    const void* wd; const float* biasd; int actd;                                   // depthwise: packed [k*k][Csp] bf16, bias fp32 (indexed from sp_c0)
    const void* res; int res_stride, res_coff;                                      // added after actd (nullable)
    void* y2; int y2_stride, y2_coff;                                              // spatial result (pool: stage s at channel offset s * Csp)
    int dbg;                                                                        // timing ablations (tools only, results wrong): 1 no MFMAs, 2 no pixel loads, 4 no spatial stage
    int wide;                                                                       // sp = 0: the paired channel order for the stores to y1 is asked for (ConvParams::wide); the launcher decides
};
bool pwsp_valid(const PwSpParams& p);
const char* pwsp_kernel_name(const PwSpParams& p);
constexpr int PWSP_CFG = 1000;                                                       // Op::cfg of a plain 1x1 conv that runs as pwsp_kernel<NS,0> (a tuner candidate)
hipError_t launch_pwsp(const PwSpParams& p, hipStream_t st);
hipError_t pwsp_read_clocks(unsigned long long* out32);

// class logits + class-max keys in one kernel (cls_out.hip)
struct ClsOutParams {
    const void* x; int x_stride, x_coff; size_t x_bytes;      // bf16 [M][x_stride] view of K channels
    int M, K, nc;
    const void* w; int Kpad; size_t w_bytes; const float* bias;   // packed [nc^][K]
    float* y; int y_stride, y_coff;                           // fp32 logits [M][y_stride]
    unsigned* keys;                                           // [M]: bits of sigmoid(max_c y)
};
bool cls_out_valid(const ClsOutParams& p);
const char* cls_out_kernel_name(const ClsOutParams& p);
hipError_t launch_cls_out(const ClsOutParams& p, hipStream_t st);

bool conv_dwpw_valid(const DwPwParams& p);
const char* conv_dwpw_kernel_name(const DwPwParams& p);
hipError_t launch_conv_dwpw(const DwPwParams& p, hipStream_t st);

struct MaskParams {
    const void* proto; int Hp, Wp;        // [Hp,Wp,32] engine dtype (one image)
    const float* coeff; const float* boxes; int n;
    int oh, ow;                           // output size
    int t, l, ch, cw;                     // crop rectangle of the proto image that maps onto (oh,ow) (retina) or full
    float bsx, bsy;                       // box scale applied before cropping (process_mask: mw/iw, mh/ih ; retina: 1)
    int crop_before;                      // 1: process_mask (crop at proto res then upsample), 0: native (upsample then crop)
    uint8_t* masks; int64_t* ids; int32_t* kept; int32_t* area;
    int suppress_small, min_area;
    int rh, rw;                           // > 0: second, antialiased bilinear resize of the {0,1} masks to (rh,rw) before the area test and
                                          // the id paint (auto_segment with min_side > 0); ids is then [rh,rw]
};
hipError_t launch_masks(const MaskParams& p, int dtype, hipStream_t st);
size_t masks_workspace_bytes(const MaskParams& p);
// One mask per selected frame (yp_masks_frames: retina; yp_masks_frames_input: process_mask, p.crop_before = 1): p describes image 0 with
// n = 1 (proto, coeff = row 0 of frame 0, crop, oh, ow);
// mask j uses frame fidx[j] (device int32 [k]): proto + fidx[j] * proto_stride bytes, coeff + fidx[j] * coeff_stride floats, box
// boxes[4j..4j+4). M: float workspace [k, ch*cw]. masks uint8 [k,oh,ow], every byte written.
struct MaskFramesParams {
    MaskParams p;
    const int32_t* fidx; int k;
    size_t proto_stride; long coeff_stride;
};
hipError_t launch_masks_frames(const MaskFramesParams& f, float* M, int dtype, hipStream_t st);
// All masks of many frames -> one id image per frame (yp_id_masks_frames): p describes image 0 and ALL rows (proto of image 0, coeff
// [n_total,32], boxes [n_total,4], n = n_total, the crop, (oh,ow), (rh,rw) > 0 for the second resize, ids int64 [k,ph,pw], kept int32
// [n_total] or NULL, suppress_small, min_area; masks and area unused). Frame j: rows row_off[j] .. row_off[j+1] against image fidx[j]
// (proto + fidx[j] * proto_stride bytes). fidx / row_off are read from the head of the workspace (int32 fidx[k] | row_off[k+1]), where
// the caller has put them; launch_id_masks_frames sets the two pointers.
struct IdMaskFramesParams {
    MaskParams p;
    const int32_t* fidx; const int32_t* row_off; int k;
    size_t proto_stride;
};
size_t id_masks_frames_workspace_bytes(const MaskParams& p, int k);
hipError_t launch_id_masks_frames(const IdMaskFramesParams& f, int max_n, void* ws, int dtype, hipStream_t st);
hipError_t contour_read_clocks(unsigned long long* out12);
hipError_t launch_contours(const uint8_t* masks, int n, int H, int W, int strategy, int max_pts, int32_t* pts, int32_t* count, int32_t* parts, int parts_cap,
                           double* rect, hipStream_t st);
// the same contours; rect of the points after hostops.scale_coords((H,W) -> (H0,W0)) and int32 truncation ((-1, -1) when W0 >= 2048)
hipError_t launch_contours_scaled(const uint8_t* masks, int n, int H, int W, int H0, int W0, int strategy, int max_pts, int32_t* pts, int32_t* count,
                                  int32_t* parts, int parts_cap, double* rect, hipStream_t st);

// the large path (contour_large.hip): every table in a caller-provided workspace; H, W <= CL_MAXDIM, up to CL_MAXCAND border starts (and
// as many outer borders) per mask. H0 = W0 = 0: rectangle in mask pixels, else as launch_contours_scaled (any W0)
constexpr int CL_MAXDIM = 4096;              // = YP_CONTOURS_LARGE_MAX_DIM (engine.hip asserts both)
constexpr int CL_MAXCAND = 65536;            // = YP_CONTOURS_LARGE_MAX_STARTS
size_t contours_large_workspace_bytes(int n, int H, int W);            // 0 on bad sizes
hipError_t launch_contours_large(const uint8_t* masks, int n, int H, int W, int strategy, int max_pts, int32_t* pts, int32_t* count, int32_t* parts,
                                 int parts_cap, double* rect, int H0, int W0, int flags, void* workspace, hipStream_t st);

// the "all_merged" bridge (contour_merge.hip) on the buffers the contour calls fill: closest pairs of consecutive contours over a tile list
// derived on the device, then every piece copied to its place. Point indices below CM_MAX_PTS (19 bits each in the 64-bit key).
constexpr int CM_TILE = 256;                 // = YP_CONTOURS_MERGE_TILE: a-points per tile (one per lane) and b-points per LDS tile
constexpr int CM_SCAN = 1024;                // = YP_CONTOURS_MERGE_SCAN_BLOCK: contours per step of the scans
constexpr int CM_MAX_PTS = 1 << 19;          // = YP_CONTOURS_MERGE_MAX_PTS
constexpr int CM_MAX_CONTOURS = CL_MAXCAND;  // a parts row lists at most as many lengths as the large path has border starts
size_t contours_merge_workspace_bytes(int n, int parts_cap);           // 0 on bad sizes
unsigned long long contours_merge_tiles(const int32_t* lengths, int n);  // host: work tiles of one mask's contour list (0 on a bad length)
hipError_t launch_contours_merge(const int32_t* pts, const int32_t* count, const int32_t* parts, int n, int max_pts, int parts_cap, int32_t* out,
                                 int32_t* out_count, int out_cap, void* workspace, hipStream_t st);

// host-side float -> bf16 (round to nearest even), as the device's v_cvt_pk_bf16_f32
static inline uint16_t f2bf(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static inline float bf2f(uint16_t h) {
    uint32_t u = ((uint32_t)h) << 16;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

}  // namespace yp

#include "kernel_util.h"   // the device primitives shared by the kernel files (they name the enums above)
