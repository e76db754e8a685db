// U^2-Net / U^2-Net-P behind the C-ABI (yp_u2net_*): the second per-frame network of the reference's video loop
// (`unet_predict(unet_model, cropped_frame)`, yolo_seg/app.py:184; model yolo_seg/tasks/models/U2Net.py:424-526, loader and
// post-process yolo_seg/tasks/unet_segment.py:32-73).
//
// Graph builder (host): RSU-7/6/5/4/4F blocks from the (in, mid, out) table of U2NETP / U2NET; every `torch.cat` is a channel-slice
// view of a buffer allocated up front (the bilinear up-sample and the skip's producer write straight into their halves), the
// block residual `hx1d + hxin` rides in the last convolution's epilogue (added after the ReLU, as in the reference).
// Kernels: dilated 3x3 conv + folded BatchNorm + ReLU = conv_igemm (matrix cores; fp32 mode = exact fp32 FMA chains), plus the
// small ones below - u8 BGR -> RGB/255 (channel-padded to 8), ceil-mode 2x2 max-pool, PyTorch-exact bilinear resize-to-size, and
// the tail: six side maps -> bilinear to full size -> 1x1 fusion -> sigmoid -> min/max -> normPRED -> mask.
// Clip path (yp_u2net_forward_crops): the input op crops B windows straight from the uint8 frames on the device, the tail keeps one
// min/max per image (the reference's normPRED runs per `unet_predict` call, i.e. per frame) and the last kernel writes the crop mask and
// pastes it into the full-frame mask in the same pass.
#include "../../include/yolop.h"
#include "common.h"
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>

using namespace yp;

extern "C" int yp_fail_public(int code, const char* msg);
static int u2fail(int code, const char* fmt, ...) {
    char buf[400];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return yp_fail_public(code, buf);
}
#define U2HIP(x)                                                                                                   \
    do {                                                                                                           \
        hipError_t _e = (x);                                                                                       \
        if (_e != hipSuccess) return u2fail(YP_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

namespace {

enum U2Kind { U2_INPUT = 0, U2_CONV = 1, U2_POOL = 2, U2_UP = 3 };

struct U2Tensor {
    std::string name;
    int C = 0, lvl = 0;
    bool f32 = false;      // fp32 regardless of the engine dtype (side maps)
    int H = 0, W = 0;
    size_t bytes = 0;
    void* ptr = nullptr;
};
struct U2Weight {
    std::string name;
    int cout = 0, cin = 0, cin_pad = 0, k = 3;
    bool have_w = false, have_b = false;
    std::vector<float> w, b;
    void* d_w = nullptr;
    float* d_b = nullptr;
    int Kpad = 0;
    size_t mat_bytes = 0;
};
struct U2Op {
    int kind = U2_CONV;
    std::string name;
    View in, out, res;
    int widx = -1, dil = 1, act = ACT_RELU;
    int impl = -1;         // convs: -1 = not yet chosen for this plan, 0 = conv_igemm, 1 = conv_small, 2 = conv_small taking the max pool /
                           // bilinear up-sample in front of it while loading, 3 = conv_halo_f32 (tuned in the plan's first pass)
    int pool_op = -1;      // convs: index of the pool op that produces this conv's input and feeds nothing else (graph pass)
    int up_op = -1;        // convs: index of the bilinear up-sample op that produces the first channels of this conv's input (graph pass)
    int consumer = -1;     // pools / up-samples: index of that conv; the op does not launch while the conv runs with impl 2
};
// one crop of yp_u2net_forward_crops: the clipped window (x1,y1,x2,y2) of frame f
struct U2Win { int x1, y1, x2, y2, f; };

}  // namespace

struct yp_u2net {
    int variant = 'p', dtype = DT_F32, device = 0;
    std::vector<U2Tensor> tensors;
    std::vector<U2Weight> weights;
    std::vector<U2Op> ops;
    std::map<std::string, int> wmap;
    int side_t[6] = {-1, -1, -1, -1, -1, -1};
    int outconv_w = -1;
    bool finalized = false;
    // conv_small.hip vs conv_igemm.hip per convolution: small_max < 0 = timed per layer in a plan's first pass (default), otherwise
    // conv_small takes every layer it can run with at most small_max output pixels (YOLOP_U2_SMALL_MAX; 0 = never). Read at create.
    long small_max = -1;
    bool fuse_pool = true;              // conv_small may take a pool / up-sample while loading (YOLOP_U2_FUSE_POOL, 0 = never). Read at create.
    int pB = 0, pH = 0, pW = 0;
    void* arena = nullptr;
    size_t arena_bytes = 0;
    float* d_fuse = nullptr;            // [6 weights | bias | min bits | max bits]
    // hipGraph replay (the crop is launch-bound: ~170 small kernels): the graph reads an engine-owned copy of the frame and writes
    // engine-owned results, so neither the caller's input nor its output pointers are baked in; both copies ride the same stream
    bool use_graph = false, warmed = false;      // replay measured slower than eager launches on this net (2.29 vs 2.08 ms at 380^2): off by default
    hipStream_t own_stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    hipGraphExec_t gexec = nullptr;
    int gB = 0, gH = 0, gW = 0;
    uint8_t* in_buf = nullptr; float* o_prob = nullptr; float* o_norm = nullptr; uint8_t* o_mask = nullptr; size_t io_cap = 0;
    // conv choices of every (B, H, W) this engine has timed, restored when a plan returns to that shape (a clip alternates between
    // 380x380 chunks and edge groups; re-timing ~119 convolutions per switch would cost more than the forward)
    std::map<std::tuple<int, int, int>, std::vector<int>> tuned;
    // yp_u2net_forward_crops: windows (pinned staging -> device), per-image [min bits, max bits], prob scratch when the caller wants none
    U2Win* h_win = nullptr; U2Win* d_win = nullptr; unsigned* d_mm = nullptr; int win_cap = 0;
    hipEvent_t ev_win = nullptr; bool win_pending = false;
    float* d_prob = nullptr; size_t prob_cap = 0;
    int es() const { return dtype == DT_BF16 ? 2 : 4; }
};

namespace {

struct StageCfg { int n; bool flat; int cin, mid, co; };      // n = 7,6,5,4 ; flat = RSU-4F

struct U2Builder {
    yp_u2net& e;
    explicit U2Builder(yp_u2net& en) : e(en) {}
    int tensor(const std::string& name, int C, int lvl, bool f32 = false) {
        U2Tensor t;
        t.name = name; t.C = C; t.lvl = lvl; t.f32 = f32;
        e.tensors.push_back(t);
        return (int)e.tensors.size() - 1;
    }
    View full(int t) const { return View{t, 0, e.tensors[t].C}; }
    int weight(const std::string& name, int cout, int cin, int k) {
        U2Weight w;
        w.name = name; w.cout = cout; w.cin = cin; w.cin_pad = (cin + 7) / 8 * 8; w.k = k;
        w.Kpad = (k * k * w.cin_pad + 31) / 32 * 32;
        w.mat_bytes = (size_t)((cout + 127) / 128 * 128) * w.Kpad * e.es();
        e.weights.push_back(w);
        e.wmap[name] = (int)e.weights.size() - 1;
        return (int)e.weights.size() - 1;
    }
    void conv(const std::string& name, View in, View out, int cin_logical, int dil, int act = ACT_RELU, View res = View{}) {
        U2Op o;
        o.kind = U2_CONV; o.name = name; o.in = in; o.out = out; o.res = res; o.dil = dil; o.act = act;
        o.widx = weight(name, out.C, cin_logical, 3);
        e.ops.push_back(o);
    }
    void pool(const std::string& name, View in, View out) {
        U2Op o;
        o.kind = U2_POOL; o.name = name; o.in = in; o.out = out;
        e.ops.push_back(o);
    }
    void up(const std::string& name, View in, View out) {
        U2Op o;
        o.kind = U2_UP; o.name = name; o.in = in; o.out = out;
        e.ops.push_back(o);
    }
    int lvl_of(View v) const { return e.tensors[v.t].lvl; }

    // RSU-n / RSU-4F (U2Net.py:30-314): `in` at level L -> `out` (a view, usually half of the next concat buffer)
    void rsu(const std::string& p, const StageCfg& s, View in, View out, int cin_logical) {
        const int L = lvl_of(in);
        const int tin = tensor(p + ".hxin", s.co, L);
        conv(p + ".rebnconvin", in, full(tin), cin_logical, 1);
        const int n = s.n;
        // cat_i (i = 1..n-1): [ first half: hx_n (deepest) or the up-sampled decoder map | second half: hx_i ]
        std::vector<int> cat(n, -1);
        for (int i = 1; i <= n - 1; ++i) cat[i] = tensor(p + ".cat" + std::to_string(i), 2 * s.mid, s.flat ? L : L + i - 1);
        auto hx = [&](int i) { return View{cat[i], s.mid, s.mid}; };
        static const int fdil[5] = {0, 1, 2, 4, 8};
        conv(p + ".rebnconv1", full(tin), hx(1), s.co, 1);
        for (int i = 2; i <= n - 1; ++i) {
            if (s.flat) conv(p + ".rebnconv" + std::to_string(i), hx(i - 1), hx(i), s.mid, fdil[i]);
            else {
                const int pt = tensor(p + ".pool" + std::to_string(i - 1), s.mid, L + i - 1);
                pool(p + ".pool" + std::to_string(i - 1), hx(i - 1), full(pt));
                conv(p + ".rebnconv" + std::to_string(i), full(pt), hx(i), s.mid, 1);
            }
        }
        conv(p + ".rebnconv" + std::to_string(n), hx(n - 1), View{cat[n - 1], 0, s.mid}, s.mid, s.flat ? 8 : 2);
        for (int i = n - 1; i >= 1; --i) {
            const bool last = i == 1;
            const int dil = s.flat ? fdil[i] : 1;
            if (last) {
                conv(p + ".rebnconv1d", full(cat[1]), out, 2 * s.mid, dil, ACT_RELU, full(tin));
            } else {
                const View dst{cat[i - 1], 0, s.mid};
                if (s.flat) conv(p + ".rebnconv" + std::to_string(i) + "d", full(cat[i]), dst, 2 * s.mid, dil);
                else {
                    const int dt = tensor(p + ".hx" + std::to_string(i) + "d", s.mid, L + i - 1);
                    conv(p + ".rebnconv" + std::to_string(i) + "d", full(cat[i]), full(dt), 2 * s.mid, 1);
                    up(p + ".up" + std::to_string(i), full(dt), dst);
                }
            }
        }
    }
};

static int build_u2net(yp_u2net& e) {
    static const StageCfg enc_p[6] = {{7, false, 3, 16, 64}, {6, false, 64, 16, 64}, {5, false, 64, 16, 64}, {4, false, 64, 16, 64}, {4, true, 64, 16, 64}, {4, true, 64, 16, 64}};
    static const StageCfg dec_p[5] = {{4, true, 128, 16, 64}, {4, false, 128, 16, 64}, {5, false, 128, 16, 64}, {6, false, 128, 16, 64}, {7, false, 128, 16, 64}};
    static const StageCfg enc_f[6] = {{7, false, 3, 32, 64}, {6, false, 64, 32, 128}, {5, false, 128, 64, 256}, {4, false, 256, 128, 512}, {4, true, 512, 256, 512}, {4, true, 512, 256, 512}};
    static const StageCfg dec_f[5] = {{4, true, 1024, 256, 512}, {4, false, 1024, 128, 256}, {5, false, 512, 64, 128}, {6, false, 256, 32, 64}, {7, false, 128, 16, 64}};
    if (e.variant != 'p' && e.variant != 'f') return u2fail(YP_ERR_ARG, "unknown U^2-Net variant '%c' ('p' = U2NETP, 'f' = U2NET)", e.variant);
    const StageCfg* enc = e.variant == 'p' ? enc_p : enc_f;
    const StageCfg* dec = e.variant == 'p' ? dec_p : dec_f;
    U2Builder B(e);
    const int x8 = B.tensor("input", 8, 0);
    {
        U2Op o;
        o.kind = U2_INPUT; o.name = "input"; o.out = B.full(x8);
        e.ops.push_back(o);
    }
    // decoder concat buffers: dcat[i] = [ up(deeper decoder map) | stage(i+1) output ], i = 0..4 (levels 0..4)
    int dcat[5];
    for (int i = 0; i < 5; ++i) {
        const int cup = (i == 4) ? enc[5].co : dec[3 - i].co;            // what is up-sampled into the first half
        dcat[i] = B.tensor("dec" + std::to_string(i + 1) + ".cat", cup + enc[i].co, i);
        if (cup + enc[i].co != dec[4 - i].cin) return u2fail(YP_ERR_STATE, "internal: decoder %d channel table", i + 1);
    }
    auto skip = [&](int i) { const int cup = e.tensors[dcat[i]].C - enc[i].co; return View{dcat[i], cup, enc[i].co}; };
    View cur = B.full(x8);
    int cin_logical = 3;
    const int h6 = B.tensor("stage6", enc[5].co, 5);
    for (int i = 0; i < 6; ++i) {
        const View out = i < 5 ? skip(i) : B.full(h6);
        B.rsu("stage" + std::to_string(i + 1), enc[i], cur, out, cin_logical);
        if (i < 5) {
            const int pt = B.tensor("pool" + std::to_string(i + 1) + std::to_string(i + 2), enc[i].co, i + 1);
            B.pool("pool" + std::to_string(i + 1) + std::to_string(i + 2), out, B.full(pt));
            cur = B.full(pt);
            cin_logical = enc[i].co;
        }
    }
    // decoder: stage5d .. stage1d
    int feat[6];                                  // hx1d .. hx5d, hx6 (side inputs)
    feat[5] = h6;
    View d = B.full(h6);
    for (int j = 0; j < 5; ++j) {
        const int i = 4 - j;                      // decoder stage i+1 works at level i
        B.up("up" + std::to_string(i + 2) + "to" + std::to_string(i + 1), d, View{dcat[i], 0, d.C});
        const int dt = B.tensor("stage" + std::to_string(i + 1) + "d", dec[j].co, i);
        B.rsu("stage" + std::to_string(i + 1) + "d", dec[j], B.full(dcat[i]), B.full(dt), dec[j].cin);
        feat[i] = dt;
        d = B.full(dt);
    }
    for (int k = 0; k < 6; ++k) {                 // side1..6: conv3x3 -> 1 channel, fp32, no activation
        const int st = B.tensor("side" + std::to_string(k + 1), 1, k, true);
        B.conv("side" + std::to_string(k + 1), B.full(feat[k]), B.full(st), e.tensors[feat[k]].C, 1, ACT_NONE);
        e.side_t[k] = st;
    }
    e.outconv_w = B.weight("outconv", 1, 6, 1);
    // graph pass: a max pool whose output is read by exactly one op, a convolution over the whole pooled tensor, may be taken by that
    // convolution while loading (conv_small's POOL form); whether it is, is decided per plan (u2_tune_op)
    for (size_t i = 0; i < e.ops.size(); ++i) {
        if (e.ops[i].kind != U2_POOL) continue;
        const int t = e.ops[i].out.t;
        int readers = 0, conv = -1;
        for (size_t j = 0; j < e.ops.size(); ++j) {
            const U2Op& o = e.ops[j];
            if (j != i && (o.in.t == t || o.res.t == t)) { ++readers; conv = (int)j; }
        }
        bool side = false;
        for (int k = 0; k < 6; ++k) side = side || e.side_t[k] == t;
        if (readers != 1 || side || conv < (int)i) continue;
        U2Op& c = e.ops[conv];
        if (c.kind != U2_CONV || c.in.t != t || c.in.coff != 0 || c.in.C != e.tensors[t].C || c.res.t == t) continue;
        if (e.ops[i].out.coff != 0 || e.ops[i].out.C != e.tensors[t].C) continue;
        c.pool_op = (int)i;
        e.ops[i].consumer = conv;
    }
    // likewise a bilinear up-sample that fills the FIRST channels of a concat buffer whose only reader of those channels is a convolution
    // over the whole buffer (the decoder convolutions of every RSU and the first convolution of every decoder stage)
    for (size_t i = 0; i < e.ops.size(); ++i) {
        if (e.ops[i].kind != U2_UP) continue;
        const View uo = e.ops[i].out;
        if (uo.coff != 0 || (uo.C & 15)) continue;
        int readers = 0, conv = -1;
        for (size_t j = 0; j < e.ops.size(); ++j) {
            const U2Op& o = e.ops[j];
            if (j == i) continue;
            if (o.in.t == uo.t && o.in.coff < uo.C) { ++readers; conv = (int)j; }
            if (o.res.t == uo.t && o.res.coff < uo.C) { ++readers; conv = -2; }
        }
        bool side = false;
        for (int k = 0; k < 6; ++k) side = side || e.side_t[k] == uo.t;
        if (readers != 1 || conv < (int)i || side) continue;
        U2Op& c = e.ops[conv];
        if (c.kind != U2_CONV || c.in.coff != 0 || c.in.C != e.tensors[uo.t].C || c.pool_op >= 0) continue;
        c.up_op = (int)i;
        e.ops[i].consumer = conv;
    }
    return YP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void u2_input_kernel(const uint8_t* __restrict__ img, T* __restrict__ out, size_t npix) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const uint8_t* s = img + i * 3;
    // numpy2tensor (yolo_seg/utils/transform.py:15-20): BGR -> RGB, ToTensor = float(u8) / 255
    const float r = (float)s[2] / 255.0f, g = (float)s[1] / 255.0f, b = (float)s[0] / 255.0f;
    T* o = out + i * 8;
    o[0] = (T)r; o[1] = (T)g; o[2] = (T)b;
#pragma unroll
    for (int c = 3; c < 8; ++c) o[c] = (T)0.f;
}

// crop_frame + numpy2tensor on the device: crop pixel (y, x) of image b is frame[f][y1 + y][x1 + x] inside the window and 0 (the
// zero pad) elsewhere, the window at the top-left as in yolo_seg/utils/transform.py:45-49. Same float operations as u2_input_kernel,
// so an unpadded crop gives the same bits. The crop never exists as uint8. Thread 0 of each image also resets that image's normPRED
// range for the tail (stream order: the previous call's last kernel has read it).
template <typename T>
__global__ __launch_bounds__(256) void u2_crop_input_kernel(const uint8_t* __restrict__ frames, int H, int W, const U2Win* __restrict__ win,
                                                           T* __restrict__ out, int ch, int cw, unsigned* __restrict__ minmax) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { minmax[2 * b] = 0x7f800000u; minmax[2 * b + 1] = 0u; }
    if (i >= ch * cw) return;
    const int y = i / cw, x = i - y * cw;
    const U2Win w = win[b];
    float r = 0.f, g = 0.f, bl = 0.f;
    if (y < w.y2 - w.y1 && x < w.x2 - w.x1) {
        const uint8_t* s = frames + (((size_t)w.f * H + (w.y1 + y)) * W + (w.x1 + x)) * 3;
        r = (float)s[2] / 255.0f; g = (float)s[1] / 255.0f; bl = (float)s[0] / 255.0f;
    }
    T* o = out + ((size_t)b * ch * cw + i) * 8;
    o[0] = (T)r; o[1] = (T)g; o[2] = (T)bl;
#pragma unroll
    for (int c = 3; c < 8; ++c) o[c] = (T)0.f;
}

// nn.MaxPool2d(2, stride=2, ceil_mode=True): windows clipped at the border
template <typename T>
__global__ __launch_bounds__(256) void u2_pool_kernel(const T* __restrict__ x, int xs, int xc, T* __restrict__ y, int ys, int yc, int B, int H, int W,
                                                     int Ho, int Wo, int C) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int cg = C >> 2;
    if (i >= (size_t)B * Ho * Wo * cg) return;
    const int c = (int)(i % cg) * 4;
    size_t r = i / cg;
    const int wo = (int)(r % Wo); r /= Wo;
    const int ho = (int)(r % Ho);
    const int b = (int)(r / Ho);
    float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int hi = ho * 2 + dy, wi = wo * 2 + dx;
            if (hi < H && wi < W) {
                const T* p = x + ((size_t)(b * H + hi) * W + wi) * xs + xc + c;
#pragma unroll
                for (int q = 0; q < 4; ++q) m[q] = fmaxf(m[q], (float)p[q]);
            }
        }
    T* o = y + ((size_t)(b * Ho + ho) * Wo + wo) * ys + yc + c;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = (T)m[q];
}

template <typename T>
__global__ __launch_bounds__(256) void u2_up_kernel(const T* __restrict__ x, int xs, int xc, T* __restrict__ y, int ys, int yc, int B, int H, int W,
                                                   int Ho, int Wo, int C) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int cg = C >> 2;
    if (i >= (size_t)B * Ho * Wo * cg) return;
    const int c = (int)(i % cg) * 4;
    size_t r = i / cg;
    const int wo = (int)(r % Wo); r /= Wo;
    const int ho = (int)(r % Ho);
    const int b = (int)(r / Ho);
    T* o = y + ((size_t)(b * Ho + ho) * Wo + wo) * ys + yc + c;
    if (H == Ho && W == Wo) {                       // same size: PyTorch returns the values unchanged (weights are exactly 1 and 0)
        const T* p = x + ((size_t)(b * H + ho) * W + wo) * xs + xc + c;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = p[q];
        return;
    }
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    bilinear_tap(ho, H, Ho, y0, y1, ly0, ly1);
    bilinear_tap(wo, W, Wo, x0, x1, lx0, lx1);
    const T* p00 = x + ((size_t)(b * H + y0) * W + x0) * xs + xc + c;
    const T* p01 = x + ((size_t)(b * H + y0) * W + x1) * xs + xc + c;
    const T* p10 = x + ((size_t)(b * H + y1) * W + x0) * xs + xc + c;
    const T* p11 = x + ((size_t)(b * H + y1) * W + x1) * xs + xc + c;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        o[q] = (T)bilinear_blend((float)p00[q], (float)p01[q], (float)p10[q], (float)p11[q], ly0, ly1, lx0, lx1);
}

struct U2Tail {
    const float* side[6];
    int h[6], w[6];
    int B, H, W;
    const float* fuse;         // [6 weights | bias]
    unsigned* minmax;          // [min bits | max bits] of the positive floats: one pair for the call, or [B][2] with per_image
    int per_image;
    float* prob;
};
// d0 = outconv(cat(d1, up(d2), ..., up(d6))) ; sigmoid (U2Net.py:498-520) ; running min / max for normPRED
// grid (H*W / 256, B): a block never spans two images, so the wave reduction below is per image
__global__ __launch_bounds__(256) void u2_tail_kernel(const U2Tail t) {
    const int b = blockIdx.y;
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t hw = (size_t)t.H * t.W;
    float pr = 0.5f;
    const bool live = j < hw;
    if (live) {
        const int wo = (int)(j % t.W);
        const int ho = (int)(j / t.W);
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const float* s = t.side[k] + (size_t)b * t.h[k] * t.w[k];
            float v;
            if (t.h[k] == t.H && t.w[k] == t.W) v = s[(size_t)ho * t.W + wo];
            else {
                int y0, y1, x0, x1;
                float ly0, ly1, lx0, lx1;
                bilinear_tap(ho, t.h[k], t.H, y0, y1, ly0, ly1);
                bilinear_tap(wo, t.w[k], t.W, x0, x1, lx0, lx1);
                v = bilinear_blend(s[y0 * t.w[k] + x0], s[y0 * t.w[k] + x1], s[y1 * t.w[k] + x0], s[y1 * t.w[k] + x1], ly0, ly1, lx0, lx1);
            }
            acc = fmaf(t.fuse[k], v, acc);
        }
        acc += t.fuse[6];
        pr = 1.f / (1.f + expf(-acc));
        t.prob[(size_t)b * hw + j] = pr;
    }
    // sigmoid outputs are >= 0: their bit patterns order like unsigned integers
    unsigned lo = live ? __float_as_uint(pr) : 0x7f800000u, hi = live ? __float_as_uint(pr) : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, (unsigned)__shfl_xor((int)lo, o));
        hi = max(hi, (unsigned)__shfl_xor((int)hi, o));
    }
    // one atomic pair per block: every block of an image updates the same two words, and at B = 16 per-wave atomics on them cost more
    // than the fusion itself
    __shared__ unsigned red[2][4];
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = lo; red[1][threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned* mm = t.minmax + (t.per_image ? 2 * b : 0);
        atomicMin(&mm[0], min(min(red[0][0], red[0][1]), min(red[0][2], red[0][3])));
        atomicMax(&mm[1], max(max(red[1][0], red[1][1]), max(red[1][2], red[1][3])));
    }
}
// normPRED (unet_segment.py:24-30) + `> 0.5 -> 255` (:66-71)
__global__ __launch_bounds__(256) void u2_norm_kernel(const float* __restrict__ prob, const unsigned* __restrict__ minmax, float* __restrict__ norm,
                                                     uint8_t* __restrict__ mask, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float mi = __uint_as_float(minmax[0]), ma = __uint_as_float(minmax[1]);
    const float dn = (prob[i] - mi) / (ma - mi);
    if (norm) norm[i] = dn;
    if (mask) mask[i] = dn > 0.5f ? 255 : 0;
}

struct U2Paste {
    const float* prob;         // [B][ch][cw]
    const unsigned* minmax;    // [B][2]
    const U2Win* win;
    int ch, cw, H, W;
    uint8_t* crop_mask;        // [B][ch][cw] or null
    uint8_t* frame_mask;       // [N][H][W] or null
};
// per-image normPRED + `> 0.5 -> 255`, then the app's paste (yolo_seg/app.py:183-186): every pixel of frame f's mask is written, the
// crop mask's top-left (y2-y1) x (x2-x1) block at (y1, x1) and 0 elsewhere. grid (max(ch*cw, H*W) / 256, B).
__global__ __launch_bounds__(256) void u2_crop_norm_kernel(const U2Paste p) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const float mi = __uint_as_float(p.minmax[2 * b]), ma = __uint_as_float(p.minmax[2 * b + 1]);
    const float* pr = p.prob + (size_t)b * p.ch * p.cw;
    if (p.crop_mask && i < p.ch * p.cw) {
        const float dn = (pr[i] - mi) / (ma - mi);
        p.crop_mask[(size_t)b * p.ch * p.cw + i] = dn > 0.5f ? 255 : 0;
    }
    if (p.frame_mask && i < p.H * p.W) {
        const U2Win w = p.win[b];
        const int fy = i / p.W, fx = i - fy * p.W;
        uint8_t v = 0;
        if (fy >= w.y1 && fy < w.y2 && fx >= w.x1 && fx < w.x2) {
            const float dn = (pr[(fy - w.y1) * p.cw + (fx - w.x1)] - mi) / (ma - mi);
            v = dn > 0.5f ? 255 : 0;
        }
        p.frame_mask[(size_t)w.f * p.H * p.W + i] = v;
    }
}

// every activation offset of a plan fits in 32 bits (the widest level-0 tensor has 128 channels, at most 4 bytes each)
static bool u2_offsets_fit(int B, int H, int W) { return (size_t)B * H * W * 128 * 4 < (1ull << 31); }

static int plan_u2(yp_u2net& e, int B, int H, int W) {
    if (B <= 0 || H < 32 || W < 32) return u2fail(YP_ERR_ARG, "input must be [B,H,W,3] with H,W >= 32 (got %d,%d,%d)", B, H, W);
    if (e.pB == B && e.pH == H && e.pW == W && e.arena) return YP_OK;
    e.warmed = false;
    int lh[6], lw[6];
    lh[0] = H; lw[0] = W;
    for (int l = 1; l < 6; ++l) { lh[l] = (lh[l - 1] + 1) / 2; lw[l] = (lw[l - 1] + 1) / 2; }
    size_t total = 0;
    for (auto& t : e.tensors) {
        t.H = lh[t.lvl]; t.W = lw[t.lvl];
        t.bytes = (size_t)B * t.H * t.W * t.C * (t.f32 ? 4 : e.es());
        total += (t.bytes + 255) & ~(size_t)255;
    }
    if (!u2_offsets_fit(B, H, W)) return u2fail(YP_ERR_ARG, "input too large for 32-bit tensor offsets");
    U2HIP(hipSetDevice(e.device));
    if (total > e.arena_bytes) {
        U2HIP(hipDeviceSynchronize());
        if (e.arena) U2HIP(hipFree(e.arena));
        e.arena = nullptr; e.arena_bytes = 0;
        U2HIP(hipMalloc(&e.arena, total));
        e.arena_bytes = total;
    }
    size_t off = 0;
    for (auto& t : e.tensors) { t.ptr = (char*)e.arena + off; off += (t.bytes + 255) & ~(size_t)255; }
    e.pB = B; e.pH = H; e.pW = W;
    const auto memo = e.tuned.find(std::make_tuple(B, H, W));
    for (size_t i = 0; i < e.ops.size(); ++i) e.ops[i].impl = memo != e.tuned.end() ? memo->second[i] : -1;
    if (e.gexec) { (void)hipDeviceSynchronize(); (void)hipGraphExecDestroy(e.gexec); e.gexec = nullptr; }
    return YP_OK;
}

template <typename T>
static hipError_t run_small(const yp_u2net& e, const U2Op& o, const uint8_t* img, hipStream_t st) {
    const int B = e.pB;
    if (o.kind == U2_INPUT) {
        const U2Tensor& to = e.tensors[o.out.t];
        const size_t npix = (size_t)B * to.H * to.W;
        hipLaunchKernelGGL(u2_input_kernel<T>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, img, (T*)to.ptr, npix);
        return hipGetLastError();
    }
    const U2Tensor &ti = e.tensors[o.in.t], &to = e.tensors[o.out.t];
    const size_t n = (size_t)B * to.H * to.W * (o.out.C / 4);
    if (o.kind == U2_POOL)
        hipLaunchKernelGGL(u2_pool_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const T*)ti.ptr, ti.C, o.in.coff, (T*)to.ptr, to.C, o.out.coff,
                           B, ti.H, ti.W, to.H, to.W, o.out.C);
    else
        hipLaunchKernelGGL(u2_up_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const T*)ti.ptr, ti.C, o.in.coff, (T*)to.ptr, to.C, o.out.coff,
                           B, ti.H, ti.W, to.H, to.W, o.out.C);
    return hipGetLastError();
}

static ConvParams u2_conv_params(const yp_u2net& e, const U2Op& o, bool fuse_pool = false) {
    const U2Weight& w = e.weights[o.widx];
    const U2Tensor &ti = e.tensors[o.in.t], &to = e.tensors[o.out.t];
    ConvParams p{};
    p.x = ti.ptr; p.x_stride = ti.C; p.x_coff = o.in.coff; p.H = ti.H; p.W = ti.W; p.Cin = w.cin_pad;
    p.w = w.d_w; p.Kpad = w.Kpad; p.bias = w.d_b;
    p.y = to.ptr; p.y_stride = to.C; p.y_coff = o.out.coff; p.Ho = to.H; p.Wo = to.W; p.Cout = o.out.C;
    if (o.res.t >= 0) { p.res = e.tensors[o.res.t].ptr; p.res_stride = e.tensors[o.res.t].C; p.res_coff = o.res.coff; }
    p.M = e.pB * to.H * to.W; p.ks = 3; p.stride = 1; p.pad = o.dil; p.dil = o.dil; p.act = o.act;
    p.out_f32 = (to.f32 && e.dtype == DT_BF16) ? 1 : 0;
    p.up = 1; p.cfg = -1;
    p.x_bytes = ti.bytes; p.w_bytes = w.mat_bytes; p.y_bytes = to.bytes;
    if (fuse_pool && o.pool_op >= 0) {                 // read the pool's input instead; H, W stay the pooled size
        const U2Op& po = e.ops[o.pool_op];
        const U2Tensor& ts = e.tensors[po.in.t];
        p.x = ts.ptr; p.x_stride = ts.C; p.x_coff = po.in.coff; p.x_bytes = ts.bytes;
        p.pool_in = 1; p.src_H = ts.H; p.src_W = ts.W;
    } else if (fuse_pool && o.up_op >= 0) {            // the first channels come from the up-sample's low-resolution input
        const U2Op& uo = e.ops[o.up_op];
        const U2Tensor& ts = e.tensors[uo.in.t];
        p.x2 = ts.ptr; p.x2_bytes = ts.bytes; p.x2_stride = ts.C; p.x2_coff = uo.in.coff; p.x2_C = uo.out.C; p.x2_H = ts.H; p.x2_W = ts.W;
        p.up_bilinear = 1;
    }
    return p;
}

// untuned choice: the K-split kernel (conv_small.hip) up to `small_max` output pixels
static int u2_default_impl(const yp_u2net& e, const ConvParams& p) {
    const long cap = e.small_max >= 0 ? e.small_max : 40000L;
    return ((long)p.M <= cap && conv_small_valid(p, e.dtype)) ? 1 : 0;
}

static hipError_t run_u2_op(const yp_u2net& e, const U2Op& o, const uint8_t* img, hipStream_t st) {
    if ((o.kind == U2_POOL || o.kind == U2_UP) && o.consumer >= 0 && e.ops[o.consumer].impl == 2) return hipSuccess;   // taken by its consumer while loading
    if (o.kind != U2_CONV) return e.dtype == DT_BF16 ? run_small<__bf16>(e, o, img, st) : run_small<float>(e, o, img, st);
    const int impl = o.impl >= 0 ? o.impl : 0;
    const ConvParams p = u2_conv_params(e, o, impl == 2);
    if (impl == 3) return launch_conv_halo_f32(p, e.dtype, st);
    return impl >= 1 ? launch_conv_small(p, e.dtype, st) : launch_conv_igemm(p, e.dtype, st);
}

// First pass of a plan: every convolution that both kernels can run is timed with both on its real input (the ops before it have
// run), the faster one is kept for this plan. An op rewrites the same output from the same inputs, so repeating it is harmless.
static int u2_tune_op(yp_u2net& e, U2Op& o, hipStream_t st) {
    const ConvParams p = u2_conv_params(e, o);
    const bool can_small = conv_small_valid(p, e.dtype), can_halo = conv_halo_f32_valid(p, e.dtype);
    if (!can_small && !can_halo) { o.impl = 0; return YP_OK; }
    const int pre_op = o.pool_op >= 0 ? o.pool_op : o.up_op;      // the pool / up-sample this conv could take while loading (at most one)
    const bool can_fuse = can_small && e.fuse_pool && pre_op >= 0 && conv_small_valid(u2_conv_params(e, o, true), e.dtype);
    if (e.small_max >= 0) {                              // forced (tests): conv_small up to small_max pixels, the halo kernel above it
        o.impl = (can_small && u2_default_impl(e, p)) ? (can_fuse ? 2 : 1) : ((can_halo && e.small_max > 0) ? 3 : 0);
        return YP_OK;
    }
    hipEvent_t e0, e1;
    U2HIP(hipEventCreate(&e0));
    U2HIP(hipEventCreate(&e1));
    // variants: 0 igemm, 1 small, 2 small + pool, 3 halo_f32, 4 = the pool launch alone (added to the unfused variants when comparing)
    float best[5] = {1e30f, 1e30f, 1e30f, 1e30f, 1e30f};
    for (int v = 0; v < 5; ++v) {
        if ((v == 1 && !can_small) || ((v == 2 || v == 4) && !can_fuse) || (v == 3 && !can_halo)) continue;
        const ConvParams pv = u2_conv_params(e, o, v == 2);
        for (int rep = 0; rep < 4; ++rep) {              // rep 0 warms (code object, caches)
            U2HIP(hipEventRecord(e0, st));
            hipError_t err;
            if (v == 4) err = e.dtype == DT_BF16 ? run_small<__bf16>(e, e.ops[pre_op], nullptr, st) : run_small<float>(e, e.ops[pre_op], nullptr, st);
            else if (v == 3) err = launch_conv_halo_f32(pv, e.dtype, st);
            else err = v >= 1 ? launch_conv_small(pv, e.dtype, st) : launch_conv_igemm(pv, e.dtype, st);
            if (err != hipSuccess) return u2fail(YP_ERR_HIP, "tuning launch of op '%s' failed: %s", o.name.c_str(), hipGetErrorString(err));
            U2HIP(hipEventRecord(e1, st));
            U2HIP(hipEventSynchronize(e1));
            float ms = 0.f;
            U2HIP(hipEventElapsedTime(&ms, e0, e1));
            if (rep > 0 && ms < best[v]) best[v] = ms;
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    o.impl = 0;
    if (best[1] < best[o.impl]) o.impl = 1;
    if (best[3] < best[o.impl]) o.impl = 3;
    if (can_fuse && best[2] < best[o.impl] + best[4]) o.impl = 2;
    static const char* names[4] = {"igemm", "small", "small+pre", "halo_f32"};
    if (getenv("YOLOP_U2_TUNE_LOG")) fprintf(stderr, "[u2 tune] %-28s M %7d Cin %3d Cout %2d dil %d: igemm %.1f us, small %.1f us, small+pool/up %.1f us (pool/up alone %.1f us), halo_f32 %.1f us -> %s\n",
                                             o.name.c_str(), p.M, p.Cin, p.Cout, p.dil, best[0] * 1e3f, can_small ? best[1] * 1e3f : 0.f, can_fuse ? best[2] * 1e3f : 0.f,
                                             can_fuse ? best[4] * 1e3f : 0.f, can_halo ? best[3] * 1e3f : 0.f, names[o.impl]);
    return YP_OK;
}

static void u2_put(std::vector<unsigned char>& buf, size_t idx, float v, int dtype) {
    if (dtype == DT_BF16) { const uint16_t h = f2bf(v); memcpy(&buf[idx * 2], &h, 2); }
    else memcpy(&buf[idx * 4], &v, 4);
}
// dense [Cout][Cin][k][k] -> [Cout^128][Kpad], k order (ky,kx,ci) over the channel-padded input (pure host arithmetic)
static void u2_pack(const yp_u2net& e, const U2Weight& w, std::vector<unsigned char>& buf) {
    buf.assign(w.mat_bytes, 0);
    for (int co = 0; co < w.cout; ++co)
        for (int ci = 0; ci < w.cin; ++ci)
            for (int ky = 0; ky < w.k; ++ky)
                for (int kx = 0; kx < w.k; ++kx)
                    u2_put(buf, (size_t)co * w.Kpad + (size_t)(ky * w.k + kx) * w.cin_pad + ci, w.w[(((size_t)co * w.cin + ci) * w.k + ky) * w.k + kx], e.dtype);
}

}  // namespace

extern "C" {

int yp_u2net_create(int variant, int dtype, int device, yp_u2net** out) {
    if (!out) return u2fail(YP_ERR_ARG, "null argument");
    if (dtype != YP_BF16 && dtype != YP_F32) return u2fail(YP_ERR_ARG, "bad dtype");
    std::unique_ptr<yp_u2net> e(new yp_u2net());
    e->variant = variant; e->dtype = dtype; e->device = device;
    if (const char* sm = getenv("YOLOP_U2_SMALL_MAX")) e->small_max = atol(sm);
    if (const char* fp = getenv("YOLOP_U2_FUSE_POOL")) e->fuse_pool = fp[0] != '0';
    const int rc = build_u2net(*e);
    if (rc != YP_OK) return rc;
    *out = e.release();
    return YP_OK;
}

int yp_u2net_destroy(yp_u2net* e) {
    if (!e) return YP_OK;
    if (e->finalized || e->arena) { (void)hipSetDevice(e->device); (void)hipDeviceSynchronize(); }
    for (auto& w : e->weights) { if (w.d_w) (void)hipFree(w.d_w); if (w.d_b) (void)hipFree(w.d_b); }
    if (e->arena) (void)hipFree(e->arena);
    if (e->d_fuse) (void)hipFree(e->d_fuse);
    if (e->gexec) (void)hipGraphExecDestroy(e->gexec);
    if (e->in_buf) { (void)hipFree(e->in_buf); (void)hipFree(e->o_prob); (void)hipFree(e->o_norm); (void)hipFree(e->o_mask); }
    if (e->ev_in) (void)hipEventDestroy(e->ev_in);
    if (e->ev_out) (void)hipEventDestroy(e->ev_out);
    if (e->ev_win) (void)hipEventDestroy(e->ev_win);
    if (e->h_win) (void)hipHostFree(e->h_win);
    if (e->d_win) (void)hipFree(e->d_win);
    if (e->d_mm) (void)hipFree(e->d_mm);
    if (e->d_prob) (void)hipFree(e->d_prob);
    if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
    delete e;
    return YP_OK;
}

int yp_u2net_weight_count(const yp_u2net* e) { return e ? (int)e->weights.size() * 2 : u2fail(YP_ERR_ARG, "null engine"); }

int yp_u2net_weight_info(const yp_u2net* e, int i, char* name, int cap, int64_t shape[4], int* ndim) {
    if (!e || i < 0 || i >= (int)e->weights.size() * 2) return u2fail(YP_ERR_ARG, "bad weight index");
    const U2Weight& w = e->weights[i / 2];
    const bool is_bias = i & 1;
    if (name && cap > 0) snprintf(name, cap, "%s.%s", w.name.c_str(), is_bias ? "bias" : "weight");
    if (is_bias) { if (shape) { shape[0] = w.cout; shape[1] = shape[2] = shape[3] = 1; } if (ndim) *ndim = 1; }
    else { if (shape) { shape[0] = w.cout; shape[1] = w.cin; shape[2] = shape[3] = w.k; } if (ndim) *ndim = 4; }
    return YP_OK;
}

int yp_u2net_set_weight(yp_u2net* e, const char* name, const float* host, const int64_t* shape, int ndim) {
    if (!e || !name || !host || !shape) return u2fail(YP_ERR_ARG, "null argument");
    if (e->finalized) return u2fail(YP_ERR_STATE, "engine already finalized");
    std::string n(name);
    const bool is_bias = n.size() > 5 && n.compare(n.size() - 5, 5, ".bias") == 0;
    const bool is_w = n.size() > 7 && n.compare(n.size() - 7, 7, ".weight") == 0;
    if (!is_bias && !is_w) return u2fail(YP_ERR_WEIGHT, "parameter name '%s' must end in .weight or .bias", name);
    auto it = e->wmap.find(n.substr(0, n.size() - (is_bias ? 5 : 7)));
    if (it == e->wmap.end()) return u2fail(YP_ERR_WEIGHT, "unknown parameter '%s'", name);
    U2Weight& w = e->weights[it->second];
    if (is_bias) {
        if (ndim != 1 || shape[0] != w.cout) return u2fail(YP_ERR_WEIGHT, "'%s': expected shape [%d]", name, w.cout);
        w.b.assign(host, host + w.cout);
        w.have_b = true;
    } else {
        if (ndim != 4 || shape[0] != w.cout || shape[1] != w.cin || shape[2] != w.k || shape[3] != w.k)
            return u2fail(YP_ERR_WEIGHT, "'%s': expected shape [%d,%d,%d,%d]", name, w.cout, w.cin, w.k, w.k);
        w.w.assign(host, host + (size_t)w.cout * w.cin * w.k * w.k);
        w.have_w = true;
    }
    return YP_OK;
}

int yp_u2net_finalize(yp_u2net* e) {
    if (!e) return u2fail(YP_ERR_ARG, "null engine");
    if (e->finalized) return YP_OK;
    for (const auto& w : e->weights)
        if (!w.have_w || !w.have_b) return u2fail(YP_ERR_WEIGHT, "parameter '%s.%s' was never set", w.name.c_str(), w.have_w ? "bias" : "weight");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return u2fail(YP_ERR_HIP, "no HIP device: the MI355X kernels cannot run here (no CPU fallback exists)");
    if (e->device < 0 || e->device >= ndev) return u2fail(YP_ERR_ARG, "device %d out of range (%d devices)", e->device, ndev);
    U2HIP(hipSetDevice(e->device));
    std::vector<unsigned char> buf;
    for (size_t i = 0; i < e->weights.size(); ++i) {
        U2Weight& w = e->weights[i];
        if ((int)i == e->outconv_w) continue;
        u2_pack(*e, w, buf);
        U2HIP(hipMalloc(&w.d_w, buf.size()));
        U2HIP(hipMemcpy(w.d_w, buf.data(), buf.size(), hipMemcpyHostToDevice));
        U2HIP(hipMalloc((void**)&w.d_b, (size_t)w.cout * 4));
        U2HIP(hipMemcpy(w.d_b, w.b.data(), (size_t)w.cout * 4, hipMemcpyHostToDevice));
    }
    {
        const U2Weight& w = e->weights[e->outconv_w];
        float f[9] = {w.w[0], w.w[1], w.w[2], w.w[3], w.w[4], w.w[5], w.b[0], 0.f, 0.f};
        U2HIP(hipMalloc((void**)&e->d_fuse, sizeof(f)));
        U2HIP(hipMemcpy(e->d_fuse, f, sizeof(f), hipMemcpyHostToDevice));
    }
    e->finalized = true;
    return YP_OK;
}

// the crop path's extra state for u2_run (null: whole-frame input, normPRED over the whole call)
struct U2CropRun {
    const uint8_t* frames;
    int H, W;
    uint8_t* crop_mask;
    uint8_t* frame_mask;
};

static int u2_run(yp_u2net* e, const uint8_t* bgr, float* prob, float* norm, uint8_t* mask, hipStream_t st, const U2CropRun* cr = nullptr) {
    bool timed = false;
    for (U2Op& o : e->ops) {
        if (o.kind == U2_CONV && o.impl < 0) {             // (never under a capture: a plan's first pass is eager)
            const int rc = u2_tune_op(*e, o, st);
            if (rc != YP_OK) return rc;
            timed = true;
        }
        hipError_t err;
        if (cr && o.kind == U2_INPUT) {
            const U2Tensor& to = e->tensors[o.out.t];
            const dim3 grid((unsigned)((to.H * to.W + 255) / 256), (unsigned)e->pB);
            if (e->dtype == DT_BF16)
                hipLaunchKernelGGL(u2_crop_input_kernel<__bf16>, grid, dim3(256), 0, st, cr->frames, cr->H, cr->W, e->d_win, (__bf16*)to.ptr, to.H, to.W, e->d_mm);
            else
                hipLaunchKernelGGL(u2_crop_input_kernel<float>, grid, dim3(256), 0, st, cr->frames, cr->H, cr->W, e->d_win, (float*)to.ptr, to.H, to.W, e->d_mm);
            err = hipGetLastError();
        } else {
            err = run_u2_op(*e, o, bgr, st);
        }
        if (err != hipSuccess) return u2fail(YP_ERR_HIP, "launch of op '%s' failed: %s", o.name.c_str(), hipGetErrorString(err));
    }
    if (timed) {
        std::vector<int>& memo = e->tuned[std::make_tuple(e->pB, e->pH, e->pW)];
        memo.clear();
        for (const U2Op& o : e->ops) memo.push_back(o.impl);
    }
    U2Tail t{};
    for (int k = 0; k < 6; ++k) { const U2Tensor& s = e->tensors[e->side_t[k]]; t.side[k] = (const float*)s.ptr; t.h[k] = s.H; t.w[k] = s.W; }
    t.B = e->pB; t.H = e->pH; t.W = e->pW; t.fuse = e->d_fuse; t.prob = prob;
    const size_t hw = (size_t)e->pH * e->pW;
    const dim3 tgrid((unsigned)((hw + 255) / 256), (unsigned)e->pB);
    if (cr) {                                              // per-image range, reset by u2_crop_input_kernel
        t.minmax = e->d_mm; t.per_image = 1;
        hipLaunchKernelGGL(u2_tail_kernel, tgrid, dim3(256), 0, st, t);
        if (cr->crop_mask || cr->frame_mask) {
            const U2Paste p{prob, e->d_mm, e->d_win, e->pH, e->pW, cr->H, cr->W, cr->crop_mask, cr->frame_mask};
            const size_t n = std::max(cr->crop_mask ? hw : 0, cr->frame_mask ? (size_t)cr->H * cr->W : 0);
            hipLaunchKernelGGL(u2_crop_norm_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)e->pB), dim3(256), 0, st, p);
        }
    } else {
        t.minmax = (unsigned*)(e->d_fuse + 7); t.per_image = 0;
        U2HIP(hipMemsetD32Async((hipDeviceptr_t)t.minmax, (int)0x7f800000u, 1, st));
        U2HIP(hipMemsetD32Async((hipDeviceptr_t)(t.minmax + 1), 0, 1, st));
        const size_t n = (size_t)e->pB * hw;
        hipLaunchKernelGGL(u2_tail_kernel, tgrid, dim3(256), 0, st, t);
        if (norm || mask) hipLaunchKernelGGL(u2_norm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, prob, t.minmax, norm, mask, n);
    }
    U2HIP(hipGetLastError());
    return YP_OK;
}

int yp_u2net_forward(yp_u2net* e, const uint8_t* bgr_dev, int B, int H, int W, float* prob_out, float* norm_out, uint8_t* mask_out, void* stream) {
    if (!e || !bgr_dev || !prob_out) return u2fail(YP_ERR_ARG, "null argument");
    if (!e->finalized) return u2fail(YP_ERR_STATE, "yp_u2net_finalize has not been called");
    int rc = plan_u2(*e, B, H, W);
    if (rc != YP_OK) return rc;
    U2HIP(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    if (!e->use_graph || !e->warmed) {            // eager; the first pass of every shape always is (nothing is loaded or configured under a capture)
        rc = u2_run(e, bgr_dev, prob_out, norm_out, mask_out, st);
        if (rc == YP_OK) e->warmed = true;
        return rc;
    }
    const size_t n = (size_t)B * H * W;
    if (n > e->io_cap) {
        U2HIP(hipDeviceSynchronize());
        if (e->gexec) { (void)hipGraphExecDestroy(e->gexec); e->gexec = nullptr; }
        if (e->in_buf) { (void)hipFree(e->in_buf); (void)hipFree(e->o_prob); (void)hipFree(e->o_norm); (void)hipFree(e->o_mask); }
        e->in_buf = nullptr; e->io_cap = 0;
        U2HIP(hipMalloc((void**)&e->in_buf, n * 3));
        U2HIP(hipMalloc((void**)&e->o_prob, n * 4));
        U2HIP(hipMalloc((void**)&e->o_norm, n * 4));
        U2HIP(hipMalloc((void**)&e->o_mask, n));
        e->io_cap = n;
    }
    if (!e->own_stream) {
        U2HIP(hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking));
        U2HIP(hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming));
        U2HIP(hipEventCreateWithFlags(&e->ev_out, hipEventDisableTiming));
    }
    if (!e->gexec || e->gB != B || e->gH != H || e->gW != W) {
        if (e->gexec) { U2HIP(hipStreamSynchronize(e->own_stream)); (void)hipGraphExecDestroy(e->gexec); e->gexec = nullptr; }
        hipGraph_t g = nullptr;
        U2HIP(hipStreamBeginCapture(e->own_stream, hipStreamCaptureModeThreadLocal));
        rc = u2_run(e, e->in_buf, e->o_prob, e->o_norm, e->o_mask, e->own_stream);
        const hipError_t ce = hipStreamEndCapture(e->own_stream, &g);
        if (rc != YP_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
        if (ce != hipSuccess) return u2fail(YP_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(ce));
        U2HIP(hipGraphInstantiate(&e->gexec, g, nullptr, nullptr, 0));
        (void)hipGraphDestroy(g);
        e->gB = B; e->gH = H; e->gW = W;
    }
    U2HIP(hipEventRecord(e->ev_in, st));
    U2HIP(hipStreamWaitEvent(e->own_stream, e->ev_in, 0));
    U2HIP(hipMemcpyAsync(e->in_buf, bgr_dev, n * 3, hipMemcpyDeviceToDevice, e->own_stream));
    U2HIP(hipGraphLaunch(e->gexec, e->own_stream));
    U2HIP(hipMemcpyAsync(prob_out, e->o_prob, n * 4, hipMemcpyDeviceToDevice, e->own_stream));
    if (norm_out) U2HIP(hipMemcpyAsync(norm_out, e->o_norm, n * 4, hipMemcpyDeviceToDevice, e->own_stream));
    if (mask_out) U2HIP(hipMemcpyAsync(mask_out, e->o_mask, n, hipMemcpyDeviceToDevice, e->own_stream));
    U2HIP(hipEventRecord(e->ev_out, e->own_stream));
    U2HIP(hipStreamWaitEvent(st, e->ev_out, 0));
    return YP_OK;
}

int yp_u2net_forward_crops(yp_u2net* e, const uint8_t* frames_dev, int N, int H, int W, const int32_t* windows, const int32_t* frame_idx,
                           int B, int ch, int cw, float* prob_out, uint8_t* crop_mask_out, uint8_t* frame_mask_out, void* stream) {
    // every argument is checked before anything is launched or allocated
    if (!e || !frames_dev || !windows || !frame_idx) return u2fail(YP_ERR_ARG, "null argument");
    if (N <= 0 || H <= 0 || W <= 0) return u2fail(YP_ERR_ARG, "frames must be [N,H,W,3] with N,H,W >= 1 (got %d,%d,%d)", N, H, W);
    if (B <= 0 || ch < 32 || cw < 32) return u2fail(YP_ERR_ARG, "crops must be [B,ch,cw] with B >= 1 and ch,cw >= 32 (got %d,%d,%d)", B, ch, cw);
    if (!u2_offsets_fit(B, ch, cw)) return u2fail(YP_ERR_ARG, "%d crops of %dx%d are too many for 32-bit tensor offsets: split the call", B, ch, cw);
    std::vector<char> seen(frame_mask_out ? N : 0, 0);
    for (int b = 0; b < B; ++b) {
        const int32_t* w = windows + 4 * b;
        const int f = frame_idx[b];
        if (f < 0 || f >= N) return u2fail(YP_ERR_ARG, "crop %d: frame index %d outside [0,%d)", b, f, N);
        if (w[0] < 0 || w[1] < 0 || w[2] > W || w[3] > H || w[0] >= w[2] || w[1] >= w[3])
            return u2fail(YP_ERR_ARG, "crop %d: window (%d,%d,%d,%d) is empty or leaves the %dx%d frame", b, w[0], w[1], w[2], w[3], W, H);
        if (w[2] - w[0] > cw || w[3] - w[1] > ch)
            return u2fail(YP_ERR_ARG, "crop %d: window (%d,%d,%d,%d) is larger than the %dx%d crop", b, w[0], w[1], w[2], w[3], cw, ch);
        if (frame_mask_out) {                         // each frame mask is written whole by the one crop that names it
            if (seen[f]) return u2fail(YP_ERR_ARG, "crop %d: frame %d is named twice while a frame mask is requested", b, f);
            seen[f] = 1;
        }
    }
    if (!e->finalized) return u2fail(YP_ERR_STATE, "yp_u2net_finalize has not been called");
    U2HIP(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    if (B > e->win_cap) {
        U2HIP(hipDeviceSynchronize());
        if (e->h_win) { (void)hipHostFree(e->h_win); (void)hipFree(e->d_win); (void)hipFree(e->d_mm); }
        e->h_win = nullptr; e->d_win = nullptr; e->d_mm = nullptr; e->win_cap = 0; e->win_pending = false;
        U2HIP(hipHostMalloc((void**)&e->h_win, (size_t)B * sizeof(U2Win)));
        U2HIP(hipMalloc((void**)&e->d_win, (size_t)B * sizeof(U2Win)));
        U2HIP(hipMalloc((void**)&e->d_mm, (size_t)B * 2 * sizeof(unsigned)));
        e->win_cap = B;
    }
    if (!e->ev_win) U2HIP(hipEventCreateWithFlags(&e->ev_win, hipEventDisableTiming));
    float* prob = prob_out;
    if (!prob) {
        const size_t n = (size_t)B * ch * cw;
        if (n > e->prob_cap) {
            U2HIP(hipDeviceSynchronize());
            if (e->d_prob) (void)hipFree(e->d_prob);
            e->d_prob = nullptr; e->prob_cap = 0;
            U2HIP(hipMalloc((void**)&e->d_prob, n * sizeof(float)));
            e->prob_cap = n;
        }
        prob = e->d_prob;
    }
    int rc = plan_u2(*e, B, ch, cw);
    if (rc != YP_OK) return rc;
    // the staging buffer is rewritten only once the previous call's copy out of it has run
    if (e->win_pending) U2HIP(hipEventSynchronize(e->ev_win));
    for (int b = 0; b < B; ++b) e->h_win[b] = U2Win{windows[4 * b], windows[4 * b + 1], windows[4 * b + 2], windows[4 * b + 3], frame_idx[b]};
    U2HIP(hipMemcpyAsync(e->d_win, e->h_win, (size_t)B * sizeof(U2Win), hipMemcpyHostToDevice, st));
    U2HIP(hipEventRecord(e->ev_win, st));
    e->win_pending = true;
    const U2CropRun cr{frames_dev, H, W, crop_mask_out, frame_mask_out};
    return u2_run(e, nullptr, prob, nullptr, nullptr, st, &cr);
}

int yp_u2net_set_graph(yp_u2net* e, int enable) {
    if (!e) return u2fail(YP_ERR_ARG, "null engine");
    e->use_graph = enable != 0;
    return YP_OK;
}

int yp_u2net_tensor_count(const yp_u2net* e) { return e ? (int)e->tensors.size() : u2fail(YP_ERR_ARG, "null engine"); }

int yp_u2net_tensor_info(const yp_u2net* e, int i, char* name, int cap, int dims[4]) {
    if (!e || i < 0 || i >= (int)e->tensors.size()) return u2fail(YP_ERR_ARG, "bad tensor index");
    const U2Tensor& t = e->tensors[i];
    if (name && cap > 0) snprintf(name, cap, "%s", t.name.c_str());
    if (dims) { dims[0] = e->pB; dims[1] = t.H; dims[2] = t.W; dims[3] = t.C; }
    return YP_OK;
}

int yp_u2net_tensor_read(yp_u2net* e, int i, float* host_out) {
    if (!e || i < 0 || i >= (int)e->tensors.size() || !host_out) return u2fail(YP_ERR_ARG, "bad argument");
    if (!e->arena) return u2fail(YP_ERR_STATE, "no forward has run yet");
    const U2Tensor& t = e->tensors[i];
    U2HIP(hipSetDevice(e->device));
    U2HIP(hipDeviceSynchronize());
    const size_t n = (size_t)e->pB * t.H * t.W * t.C;
    if (t.f32 || e->dtype == DT_F32) {
        U2HIP(hipMemcpy(host_out, t.ptr, n * 4, hipMemcpyDeviceToHost));
    } else {
        std::vector<uint16_t> tmp(n);
        U2HIP(hipMemcpy(tmp.data(), t.ptr, n * 2, hipMemcpyDeviceToHost));
        for (size_t j = 0; j < n; ++j) host_out[j] = bf2f(tmp[j]);
    }
    return YP_OK;
}

int yp_u2net_op_count(const yp_u2net* e) { return e ? (int)e->ops.size() : u2fail(YP_ERR_ARG, "null engine"); }

int yp_u2net_op_info(const yp_u2net* e, int i, char* name, int cap, int32_t* info, int info_cap) {
    if (!e || i < 0 || i >= (int)e->ops.size()) return u2fail(YP_ERR_ARG, "bad op index");
    const U2Op& o = e->ops[i];
    if (name && cap > 0) snprintf(name, cap, "%s", o.name.c_str());
    const int32_t f[YP_U2_OP_INFO] = {o.kind, o.in.t, o.in.coff, o.in.C, o.out.t, o.out.coff, o.out.C, o.res.t, o.res.coff, o.res.C, o.dil, o.act,
                                      o.widx >= 0 ? e->weights[o.widx].cin : 0, o.impl, o.pool_op, o.up_op, o.consumer};
    for (int k = 0; info && k < info_cap && k < YP_U2_OP_INFO; ++k) info[k] = f[k];
    return YP_U2_OP_INFO;
}

}  // extern "C"
