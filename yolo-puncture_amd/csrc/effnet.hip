// EfficientNet-B3 needle classifier behind the C-ABI (yp_cls_*): the third network of the reference's video loop
// (`load_classify_net` + `predict_and_find_start_inserted`, yolo_seg/app.py:116-123 -> yolo_seg/tasks/needle_clasify.py:41-199;
// the network is efficientnet_pytorch's `EfficientNet.from_name('efficientnet-b3', num_classes=2)`).
//
// Graph builder (host): the 26 MBConv blocks from the (width 1.2, depth 1.4) coefficients, TF "SAME" static padding computed for the
// configured image size 300. Kernels (all NHWC, one image per grid z so that results do not depend on the batch):
//   cls_stem_kernel   uint8 frame + int32 box -> 380^2 crop window, pad, /255, normalise -> 3x3 s2 conv 3->40 + bias + swish
//   cls_pw_kernel     1x1 conv as a GEMM on the matrix cores (fp32: v_mfma_f32_16x16x4_f32, bf16: v_mfma_f32_16x16x32_bf16) with an
//                     optional per-image gate on the K operand (SE), bias, swish, residual, or a fused global-average-pool epilogue
//   cls_dw_kernel     depthwise k3/k5 s1/s2 + bias + swish, with the SE squeeze as per-(image, row chunk, channel) partial sums
//   cls_se_kernel     per image: partial sums -> mean -> reduce 1x1 + bias -> swish -> expand 1x1 + bias -> sigmoid = gate
//   cls_fc_kernel     per image: pool partials -> mean -> FC 1536->2 -> softmax -> max prob, argmax
// Every reduction runs in a fixed order without atomics: graph replay equals eager, B = 1 equals B = 8 bitwise.
#include "../../include/yolop.h"
#include "common.h"
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

using namespace yp;

extern "C" int yp_fail_public(int code, const char* msg);
static int clsfail(int code, const char* fmt, ...) {
    char buf[400];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return yp_fail_public(code, buf);
}
#define CLSHIP(x)                                                                                                  \
    do {                                                                                                           \
        hipError_t _e = (x);                                                                                       \
        if (_e != hipSuccess) return clsfail(YP_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

namespace {

constexpr int CLS_IN = 380;          // INPUT_IMG_SIZE of needle_clasify.py
constexpr int CLS_HALF = CLS_IN / 2;
constexpr int DW_ROWS = 1;           // output rows per depthwise workgroup (= the SE squeeze's row chunk)

// ---------------------------------------------------------------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float d_bf2f(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
__device__ __forceinline__ uint16_t d_f2bf(float f) {       // round to nearest even (NaN stays NaN)
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

template <typename T> __device__ __forceinline__ float ld(const T* p, size_t i);
template <> __device__ __forceinline__ float ld<float>(const float* p, size_t i) { return p[i]; }
template <> __device__ __forceinline__ float ld<uint16_t>(const uint16_t* p, size_t i) { return d_bf2f(p[i]); }
__device__ __forceinline__ void st(float* p, size_t i, float v) { p[i] = v; }
__device__ __forceinline__ void st(uint16_t* p, size_t i, float v) { p[i] = d_f2bf(v); }
__device__ __forceinline__ float rnd(float, float v) { return v; }           // the value the next op reads back
__device__ __forceinline__ float rnd(uint16_t, float v) { return d_bf2f(d_f2bf(v)); }

// The crop window of predict_and_find_start_inserted -> crop_frame(frame, xyxy, 380, need_padding=True) (restated in
// classify.crop_geometry, which this must equal bit for bit): centre = int((x1+x2)/2) (C integer division truncates toward zero like
// Python's int()), window [c-190, c+190) clipped to the frame, the clipped crop at the top-left of a zero 380x380 image.
struct Roi { int x0, y0, cw, ch; };
__host__ __device__ inline Roi roi_of(const int* box, int FH, int FW) {
    const int cx = (box[0] + box[2]) / 2, cy = (box[1] + box[3]) / 2;
    const int x1 = max(0, cx - CLS_HALF), y1 = max(0, cy - CLS_HALF);
    const int x2 = min(FW, cx + CLS_HALF), y2 = min(FH, cy + CLS_HALF);
    return Roi{x1, y1, max(0, x2 - x1), max(0, y2 - y1)};
}
// ToTensor (/255) then Normalize ((v - mean) / std) in fp32, the same op order as torchvision; crop padding is uint8 0 before it
__device__ __forceinline__ float roi_value(const uint8_t* frame, const Roi& r, int FW, int bgr, int py, int px, int c) {
    const float mean[3] = {0.485f, 0.456f, 0.406f};
    const float stdv[3] = {0.229f, 0.224f, 0.225f};
    uint8_t u = 0;
    if (py < r.ch && px < r.cw) u = frame[((size_t)(r.y0 + py) * FW + (r.x0 + px)) * 3 + (bgr ? 2 - c : c)];
    return ((float)u / 255.f - mean[c]) / stdv[c];
}

// sum of n partials p[0], p[stride], ... in index order; the loads go out 8 at a time (one dependent load per partial costs ~70 us
// on the 190^2 maps' 190 chunks), the additions keep the order
__device__ __forceinline__ float sum_chunks(const float* p, int n, size_t stride) {
    float t = 0.f;
    for (int r = 0; r < n; r += 8) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = r + i < n ? p[(size_t)(r + i) * stride] : 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) if (r + i < n) t += v[i];
    }
    return t;
}

// ---- ROI stem -------------------------------------------------------------------------------------------------------------------------
struct StemArgs {
    const uint8_t* frames; const int* boxes; int FH, FW, bgr;
    const float* w;        // [3][3][3 rgb][40]
    const float* bias;     // [40]
    void* y; int Ho, Wo;   // [B][Ho][Wo][40]
    int pt, pl;            // static SAME pad (top, left)
};
constexpr int STEM_C = 40;

template <typename T>
__global__ __launch_bounds__(256) void cls_stem_kernel(StemArgs a) {
    __shared__ float sw[27 * STEM_C];
    __shared__ float sb[STEM_C];
    for (int i = threadIdx.x; i < 27 * STEM_C; i += 256) sw[i] = a.w[i];
    if (threadIdx.x < STEM_C) sb[threadIdx.x] = a.bias[threadIdx.x];
    __syncthreads();
    const int b = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= a.Ho * a.Wo) return;
    const int oy = pix / a.Wo, ox = pix % a.Wo;
    const uint8_t* frame = a.frames + (size_t)b * a.FH * a.FW * 3;
    const Roi r = roi_of(a.boxes + 4 * b, a.FH, a.FW);
    float acc[STEM_C];
#pragma unroll
    for (int c = 0; c < STEM_C; ++c) acc[c] = 0.f;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * 2 - a.pt + ky;
        if (iy < 0 || iy >= CLS_IN) continue;                       // SAME padding: 0 after normalisation
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * 2 - a.pl + kx;
            if (ix < 0 || ix >= CLS_IN) continue;
            for (int c = 0; c < 3; ++c) {
                const float v = roi_value(frame, r, a.FW, a.bgr, iy, ix, c);
                const float* wp = sw + ((ky * 3 + kx) * 3 + c) * STEM_C;
#pragma unroll
                for (int o = 0; o < STEM_C; ++o) acc[o] = fmaf(v, wp[o], acc[o]);
            }
        }
    }
    T* y = (T*)a.y + ((size_t)b * a.Ho * a.Wo + pix) * STEM_C;
#pragma unroll
    for (int o = 0; o < STEM_C; ++o) st(y, o, silu_ieee(acc[o] + sb[o]));
}

// debug tap only (YOLOP_CLS_TAP_INPUT=1): the normalised 380^2 crop the stem reads, from the same roi_value
__global__ void cls_crop_kernel(const uint8_t* frames, const int* boxes, int FH, int FW, int bgr, float* out) {
    const int b = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= CLS_IN * CLS_IN) return;
    const Roi r = roi_of(boxes + 4 * b, FH, FW);
    const uint8_t* frame = frames + (size_t)b * FH * FW * 3;
    for (int c = 0; c < 3; ++c) out[((size_t)b * CLS_IN * CLS_IN + pix) * 3 + c] = roi_value(frame, r, FW, bgr, pix / CLS_IN, pix % CLS_IN, c);
}

// ---- 1x1 conv = GEMM on the matrix cores ----------------------------------------------------------------------------------------------
// y[b][p][n] = act(sum_k x[b][p][k] * gate[b][k] * w[n][k] + bias[n]) + res[b][p][n], p < HW. Workgroup = 4 waves = 64 pixels x 64
// channels of one image; each wave 32 x 32 as 2 x 2 MFMA tiles of 16 x 16. w is packed [Npad = N^32][Kpad = K^32] zero-padded, so only
// the activation operand needs bounds (K % 8 == 0 is checked by the builder). pool != null: nothing is stored; the wave writes its 32
// rows' column sums of act(...) to pool[b][row/32][n] (the head's global average pool, finished by cls_fc_kernel in a fixed order).
struct PwArgs {
    const void* x; const void* w; const float* bias; const float* gate; const void* res;
    void* y; float* pool;
    int HW, K, N, Kpad, act;
};

template <typename T>
__global__ __launch_bounds__(256) void cls_pw_kernel(PwArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z;
    const int row0 = blockIdx.x * 64 + (wave & 1) * 32;
    const int col0 = blockIdx.y * 64 + (wave >> 1) * 32;
    const int Npad = (a.N + 31) / 32 * 32;
    if (row0 >= a.HW || col0 >= Npad) return;                       // (no barrier in this kernel)
    const T* x = (const T*)a.x + (size_t)b * a.HW * a.K;
    const T* w = (const T*)a.w;
    const float* g = a.gate ? a.gate + (size_t)b * a.K : nullptr;
    f32x4 acc[2][2];
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int lr = lane & 15, lg = lane >> 4;
    if constexpr (sizeof(T) == 2) {
        for (int k0 = 0; k0 < a.Kpad; k0 += 32) {
            const int kk = k0 + 8 * lg;
            bf16x8 af[2], bfr[2];
            for (int i = 0; i < 2; ++i) {
                const int row = row0 + i * 16 + lr;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (row < a.HW && kk < a.K) {
                    v = *(const uint4*)(x + (size_t)row * a.K + kk);
                    if (g) {
                        uint16_t* h = (uint16_t*)&v;
                        for (int e = 0; e < 8; ++e) h[e] = d_f2bf(d_bf2f(h[e]) * g[kk + e]);
                    }
                }
                af[i] = __builtin_bit_cast(bf16x8, v);
            }
            for (int j = 0; j < 2; ++j) bfr[j] = __builtin_bit_cast(bf16x8, *(const uint4*)(w + (size_t)(col0 + j * 16 + lr) * a.Kpad + kk));
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
    } else {
        // f32: each lane loads 4 consecutive k (float4); step t of the four MFMAs takes element t, i.e. lane group lg supplies
        // k = k0 + 4 lg + t to both operands - an exact fp32 FMA chain over all 16 k of the chunk
        for (int k0 = 0; k0 < a.Kpad; k0 += 16) {
            const int kk = k0 + 4 * lg;
            float4 av[2], bv[2];
            for (int i = 0; i < 2; ++i) {
                const int row = row0 + i * 16 + lr;
                av[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < a.HW && kk < a.K) {
                    av[i] = *(const float4*)(x + (size_t)row * a.K + kk);
                    if (g) { av[i].x *= g[kk]; av[i].y *= g[kk + 1]; av[i].z *= g[kk + 2]; av[i].w *= g[kk + 3]; }
                }
            }
            for (int j = 0; j < 2; ++j) bv[j] = *(const float4*)(w + (size_t)(col0 + j * 16 + lr) * a.Kpad + kk);
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i].x, bv[j].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i].y, bv[j].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i].z, bv[j].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i].w, bv[j].w, acc[i][j], 0, 0, 0);
                }
        }
    }
    // epilogue: C/D map col = lane & 15, row = 4 (lane >> 4) + r
    for (int j = 0; j < 2; ++j) {
        const int col = col0 + j * 16 + lr;
        const bool cok = col < a.N;
        const float bias = cok ? a.bias[col] : 0.f;
        float colsum = 0.f;
        for (int i = 0; i < 2; ++i)
            for (int r = 0; r < 4; ++r) {
                const int row = row0 + i * 16 + 4 * lg + r;
                float v = acc[i][j][r] + bias;
                if (a.act) v = silu_ieee(v);
                if (a.pool) {
                    if (row < a.HW) colsum += v;
                } else if (cok && row < a.HW) {
                    const size_t o = ((size_t)b * a.HW + row) * a.N + col;
                    if (a.res) v += ld((const T*)a.res, o);
                    st((T*)a.y, o, v);
                }
            }
        if (a.pool) {
            colsum += __shfl_xor(colsum, 16);
            colsum += __shfl_xor(colsum, 32);
            if (lg == 0 && cok) a.pool[((size_t)b * ((a.HW + 31) / 32) + row0 / 32) * a.N + col] = colsum;
        }
    }
}

// ---- depthwise conv + SE squeeze ------------------------------------------------------------------------------------------------------
// Workgroup = DW_ROWS output rows x 32 channels of one image; thread = channel (tid & 31) x pixel lane (tid >> 5). Each thread sums
// the values it stores (as stored: bf16-rounded in bf16 mode) in pixel order, the 8 lanes are added in lane order: part[b][chunk][c].
struct DwArgs {
    const void* x; const float* w /*[k*k][C]*/; const float* bias;
    void* y; float* part;
    int H, W, C, Ho, Wo, k, s, pt, pl;
};

template <typename T>
__global__ __launch_bounds__(256) void cls_dw_kernel(DwArgs a) {
    __shared__ float red[8][32];
    const int c = blockIdx.y * 32 + (threadIdx.x & 31);
    const int p = threadIdx.x >> 5;
    const int b = blockIdx.z;
    const int oy0 = blockIdx.x * DW_ROWS;
    float sum = 0.f;
    if (c < a.C) {
        const T* x = (const T*)a.x + (size_t)b * a.H * a.W * a.C;
        T* y = (T*)a.y + (size_t)b * a.Ho * a.Wo * a.C;
        const float bias = a.bias[c];
        const int n = min(DW_ROWS, a.Ho - oy0) * a.Wo;
        for (int q = p; q < n; q += 8) {
            const int oy = oy0 + q / a.Wo, ox = q % a.Wo;
            float acc = 0.f;
            for (int ky = 0; ky < a.k; ++ky) {
                const int iy = oy * a.s - a.pt + ky;
                if (iy < 0 || iy >= a.H) continue;
                for (int kx = 0; kx < a.k; ++kx) {
                    const int ix = ox * a.s - a.pl + kx;
                    if (ix < 0 || ix >= a.W) continue;
                    acc = fmaf(ld(x, ((size_t)iy * a.W + ix) * a.C + c), a.w[(ky * a.k + kx) * a.C + c], acc);
                }
            }
            const float v = silu_ieee(acc + bias);
            st(y, ((size_t)oy * a.Wo + ox) * a.C + c, v);
            sum += rnd(T{}, v);
        }
    }
    red[p][threadIdx.x & 31] = sum;
    __syncthreads();
    if (p == 0 && c < a.C) {
        float t = red[0][threadIdx.x];
        for (int i = 1; i < 8; ++i) t += red[i][threadIdx.x];
        a.part[((size_t)b * gridDim.x + blockIdx.x) * a.C + c] = t;
    }
}

// ---- SE excite: one workgroup per image -----------------------------------------------------------------------------------------------
struct SeArgs {
    const float* part; int nchunk, HW, C, sq;
    const float* wr; const float* br;   // [sq][C], [sq]
    const float* we; const float* be;   // [C][sq], [C]
    float* gate;                        // [B][C]
};
constexpr int SE_MAXC = 2304, SE_MAXSQ = 96;

__global__ __launch_bounds__(256) void cls_se_kernel(SeArgs a) {
    __shared__ float mean[SE_MAXC];
    __shared__ float s[SE_MAXSQ];
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < a.C; c += 256) {
        mean[c] = sum_chunks(a.part + (size_t)b * a.nchunk * a.C + c, a.nchunk, a.C) / (float)a.HW;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = wave; j < a.sq; j += 4) {
        float t = 0.f;
        for (int c = lane; c < a.C; c += 64) t = fmaf(a.wr[(size_t)j * a.C + c], mean[c], t);
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
        if (lane == 0) s[j] = silu_ieee(t + a.br[j]);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < a.C; c += 256) {
        float t = 0.f;
        for (int j = 0; j < a.sq; ++j) t = fmaf(a.we[(size_t)c * a.sq + j], s[j], t);
        a.gate[(size_t)b * a.C + c] = sigmoid_ieee(t + a.be[c]);
    }
}

// ---- head tail: pool -> FC -> softmax -> max / argmax ---------------------------------------------------------------------------------
struct FcArgs {
    const float* part; int nchunk, HW, C;
    const float* w; const float* bias;  // [2][C], [2]
    float* pooled;                      // [B][C] (debug tap)
    float* logits; float* prob; int* cls;
};
constexpr int FC_MAXC = 1536;

__global__ __launch_bounds__(128) void cls_fc_kernel(FcArgs a) {
    __shared__ float pooled[FC_MAXC];
    __shared__ float lg[2];
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < a.C; c += 128) {
        pooled[c] = sum_chunks(a.part + (size_t)b * a.nchunk * a.C + c, a.nchunk, a.C) / (float)a.HW;
        a.pooled[(size_t)b * a.C + c] = pooled[c];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float t = 0.f;
    for (int c = lane; c < a.C; c += 64) t = fmaf(a.w[(size_t)wave * a.C + c], pooled[c], t);
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if (lane == 0) lg[wave] = t + a.bias[wave];
    __syncthreads();
    if (threadIdx.x == 0) {
        const float l0 = lg[0], l1 = lg[1], m = fmaxf(l0, l1);
        const float e0 = expf(l0 - m), e1 = expf(l1 - m), sum = e0 + e1;
        const float p0 = e0 / sum, p1 = e1 / sum;
        a.logits[2 * b] = l0; a.logits[2 * b + 1] = l1;
        a.prob[b] = p1 > p0 ? p1 : p0;
        a.cls[b] = p1 > p0 ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// host: network table, weights, tensors
// ---------------------------------------------------------------------------------------------------------------------------------------
enum WKind { W_STEM = 0, W_PW = 1, W_DW = 2, W_SE = 3, W_FC = 4 };
struct ClsWeight {
    std::string name;
    int kind = W_PW, cout = 0, cin = 0, k = 1;
    bool have_w = false, have_b = false;
    std::vector<float> w, b;
    void* d_w = nullptr; float* d_b = nullptr;
    int Kpad = 0;
};
struct ClsTensor {
    std::string name;
    int H = 0, W = 0, C = 0;
    bool f32 = false;     // fp32 in both modes (gates, pooled features, the input tap)
    void* ptr = nullptr;
};
struct ClsBlock {
    int k, s, cin, cout, cexp, sq, pt, pl, Hin, Hout;
    bool expand, residual;
    int w_exp = -1, w_dw, w_ser, w_see, w_proj;
    int t_exp = -1, t_dw, t_gate, t_out;
};

// efficientnet_pytorch 0.7.x: efficientnet-b0 block strings, scaled by (width, depth)
struct BaseStage { int r, k, s, e, i, o; };
const BaseStage kB0[7] = {{1, 3, 1, 1, 32, 16}, {2, 3, 2, 6, 16, 24}, {2, 5, 2, 6, 24, 40}, {3, 3, 2, 6, 40, 80},
                          {3, 5, 1, 6, 80, 112}, {4, 5, 2, 6, 112, 192}, {1, 3, 1, 6, 192, 320}};
int round_filters(int f, double width) {
    const double x = f * width;
    int nf = std::max(8, (int)(x + 4.0) / 8 * 8);
    if (nf < 0.9 * x) nf += 8;
    return nf;
}
// TF SAME static padding for input size i: (before, total)
void same_pad(int i, int k, int s, int* before, int* total) {
    const int o = (i + s - 1) / s;
    *total = std::max((o - 1) * s + k - i, 0);
    *before = *total / 2;
}

}  // namespace

struct yp_cls {
    int variant = 3, dtype = DT_F32, device = 0;
    std::vector<ClsWeight> weights;
    std::map<std::string, int> wmap;
    std::vector<ClsTensor> tensors;
    std::vector<ClsBlock> blocks;
    int w_stem = -1, w_head = -1, w_fc = -1;
    int stem_pt = 0, stem_pl = 0;
    int t_input = -1, t_stem = -1, t_pool = -1;
    int head_c = 0;
    bool tap_input = false, finalized = false;
    int pB = 0;
    void* arena = nullptr;
    float* d_part = nullptr; size_t part_elems = 0;
    bool use_graph = false;
    hipStream_t cap_stream = nullptr;
    hipGraphExec_t gexec = nullptr;
    const void* gkey[6] = {};
    int gB = 0, gH = 0, gW = 0, gbgr = 0;
    int es() const { return dtype == DT_BF16 ? 2 : 4; }
};

namespace {

int add_weight(yp_cls& e, const std::string& name, int kind, int cout, int cin, int k) {
    ClsWeight w;
    w.name = name; w.kind = kind; w.cout = cout; w.cin = cin; w.k = k;
    e.weights.push_back(w);
    e.wmap[name] = (int)e.weights.size() - 1;
    return (int)e.weights.size() - 1;
}
int add_tensor(yp_cls& e, const std::string& name, int H, int W, int C, bool f32 = false) {
    ClsTensor t;
    t.name = name; t.H = H; t.W = W; t.C = C; t.f32 = f32;
    e.tensors.push_back(t);
    return (int)e.tensors.size() - 1;
}

int build_cls(yp_cls& e) {
    if (e.variant != 3)
        return clsfail(YP_ERR_ARG, "efficientnet-b%d: only efficientnet-b3 is supported (b4/b5/b7 are registered by the reference's "
                                   "models/efficientnet.py but no caller selects them)", e.variant);
    const double width = 1.2, depth = 1.4;
    const int cfg_size = 300;                     // efficientnet-b3's configured image size: the static padding is computed for it
    int isz = cfg_size;                           // padding image size, threaded like calculate_output_image_size
    int H = CLS_IN;                               // actual map size
    const int c0 = round_filters(32, width);
    if (c0 != STEM_C) return clsfail(YP_ERR_STATE, "internal: stem width %d", c0);
    e.w_stem = add_weight(e, "_conv_stem", W_STEM, c0, 3, 3);
    int tot;
    same_pad(isz, 3, 2, &e.stem_pt, &tot);
    e.stem_pl = e.stem_pt;
    isz = (isz + 1) / 2;
    H = (H + 1) / 2;
    e.t_input = add_tensor(e, "input", CLS_IN, CLS_IN, 3, true);
    e.t_stem = add_tensor(e, "stem", H, H, c0);
    int idx = 0;
    for (int si = 0; si < 7; ++si) {
        const BaseStage& bs = kB0[si];
        const int cin0 = round_filters(bs.i, width), cout = round_filters(bs.o, width);
        const int reps = (int)std::ceil(depth * bs.r);
        for (int r = 0; r < reps; ++r, ++idx) {
            ClsBlock B{};
            B.k = bs.k; B.s = r == 0 ? bs.s : 1; B.cin = r == 0 ? cin0 : cout; B.cout = cout;
            B.cexp = B.cin * bs.e; B.sq = std::max(1, (int)(B.cin * 0.25));
            B.expand = bs.e != 1; B.residual = B.s == 1 && B.cin == B.cout;
            same_pad(isz, B.k, B.s, &B.pt, &tot);
            B.pl = B.pt;
            B.Hin = H; B.Hout = (H + B.s - 1) / B.s;
            const std::string p = "_blocks." + std::to_string(idx);
            if (B.cexp > SE_MAXC || B.sq > SE_MAXSQ || B.cin % 8 || B.cexp % 8) return clsfail(YP_ERR_STATE, "internal: block %d widths", idx);
            if (B.expand) B.w_exp = add_weight(e, p + "._expand_conv", W_PW, B.cexp, B.cin, 1);
            B.w_dw = add_weight(e, p + "._depthwise_conv", W_DW, B.cexp, 1, B.k);
            B.w_ser = add_weight(e, p + "._se_reduce", W_SE, B.sq, B.cexp, 1);
            B.w_see = add_weight(e, p + "._se_expand", W_SE, B.cexp, B.sq, 1);
            B.w_proj = add_weight(e, p + "._project_conv", W_PW, B.cout, B.cexp, 1);
            if (B.expand) B.t_exp = add_tensor(e, p + ".expand", B.Hin, B.Hin, B.cexp);
            B.t_dw = add_tensor(e, p + ".dw", B.Hout, B.Hout, B.cexp);
            B.t_gate = add_tensor(e, p + ".gate", 1, 1, B.cexp, true);
            B.t_out = add_tensor(e, p, B.Hout, B.Hout, B.cout);
            e.blocks.push_back(B);
            isz = (isz + B.s - 1) / B.s;
            H = B.Hout;
        }
    }
    e.head_c = round_filters(1280, width);
    if (e.head_c > FC_MAXC) return clsfail(YP_ERR_STATE, "internal: head width");
    e.w_head = add_weight(e, "_conv_head", W_PW, e.head_c, e.blocks.back().cout, 1);
    e.w_fc = add_weight(e, "_fc", W_FC, 2, e.head_c, 1);
    e.t_pool = add_tensor(e, "head.pool", 1, 1, e.head_c, true);
    return YP_OK;
}

size_t tensor_bytes(const yp_cls& e, const ClsTensor& t, int B) { return (size_t)B * t.H * t.W * t.C * (t.f32 ? 4 : e.es()); }

int plan_cls(yp_cls& e, int B) {
    if (B == e.pB && e.arena) return YP_OK;
    if (e.gexec) { (void)hipDeviceSynchronize(); (void)hipGraphExecDestroy(e.gexec); e.gexec = nullptr; }
    if (e.arena) { (void)hipDeviceSynchronize(); (void)hipFree(e.arena); e.arena = nullptr; }
    if (e.d_part) { (void)hipFree(e.d_part); e.d_part = nullptr; }
    size_t total = 0;
    std::vector<size_t> off(e.tensors.size());
    for (size_t i = 0; i < e.tensors.size(); ++i) {
        off[i] = total;
        if ((int)i == e.t_input && !e.tap_input) continue;
        total += (tensor_bytes(e, e.tensors[i], B) + 255) / 256 * 256;
    }
    CLSHIP(hipMalloc(&e.arena, total));
    for (size_t i = 0; i < e.tensors.size(); ++i)
        e.tensors[i].ptr = ((int)i == e.t_input && !e.tap_input) ? nullptr : (char*)e.arena + off[i];
    size_t part = 0;
    for (const ClsBlock& b : e.blocks) part = std::max(part, (size_t)((b.Hout + DW_ROWS - 1) / DW_ROWS) * b.cexp);
    const int hw = e.blocks.back().Hout * e.blocks.back().Hout;
    part = std::max(part, (size_t)((hw + 31) / 32) * e.head_c);
    e.part_elems = part * B;
    CLSHIP(hipMalloc((void**)&e.d_part, e.part_elems * 4));
    e.pB = B;
    return YP_OK;
}

template <typename T>
hipError_t launch_pw(const yp_cls& e, int widx, const void* x, int HW, const float* gate, const void* res, void* y, float* pool, int act, int B,
                     hipStream_t st) {
    const ClsWeight& w = e.weights[widx];
    PwArgs a{x, w.d_w, w.d_b, gate, res, y, pool, HW, w.cin, w.cout, w.Kpad, act};
    hipLaunchKernelGGL(cls_pw_kernel<T>, dim3((HW + 63) / 64, (w.cout + 63) / 64, B), dim3(256), 0, st, a);
    return hipGetLastError();
}

template <typename T>
int run_cls(yp_cls& e, const uint8_t* frames, int B, int FH, int FW, int bgr, const int* boxes, float* logits, float* prob, int* cls,
            hipStream_t st) {
    {
        const ClsWeight& w = e.weights[e.w_stem];
        const ClsTensor& t = e.tensors[e.t_stem];
        StemArgs a{frames, boxes, FH, FW, bgr, (const float*)w.d_w, w.d_b, t.ptr, t.H, t.W, e.stem_pt, e.stem_pl};
        hipLaunchKernelGGL(cls_stem_kernel<T>, dim3((t.H * t.W + 255) / 256, B), dim3(256), 0, st, a);
        if (e.tap_input)
            hipLaunchKernelGGL(cls_crop_kernel, dim3((CLS_IN * CLS_IN + 255) / 256, B), dim3(256), 0, st, frames, boxes, FH, FW, bgr,
                               (float*)e.tensors[e.t_input].ptr);
        CLSHIP(hipGetLastError());
    }
    const void* cur = e.tensors[e.t_stem].ptr;
    for (const ClsBlock& b : e.blocks) {
        const void* xin = cur;
        if (b.expand) {
            CLSHIP(launch_pw<T>(e, b.w_exp, cur, b.Hin * b.Hin, nullptr, nullptr, e.tensors[b.t_exp].ptr, nullptr, 1, B, st));
            xin = e.tensors[b.t_exp].ptr;
        }
        const int nchunk = (b.Hout + DW_ROWS - 1) / DW_ROWS;
        {
            const ClsWeight& w = e.weights[b.w_dw];
            DwArgs a{xin, (const float*)w.d_w, w.d_b, e.tensors[b.t_dw].ptr, e.d_part, b.Hin, b.Hin, b.cexp, b.Hout, b.Hout, b.k, b.s, b.pt, b.pl};
            hipLaunchKernelGGL(cls_dw_kernel<T>, dim3(nchunk, (b.cexp + 31) / 32, B), dim3(256), 0, st, a);
            CLSHIP(hipGetLastError());
        }
        {
            const ClsWeight& r = e.weights[b.w_ser];
            const ClsWeight& x = e.weights[b.w_see];
            SeArgs a{e.d_part, nchunk, b.Hout * b.Hout, b.cexp, b.sq, (const float*)r.d_w, r.d_b, (const float*)x.d_w, x.d_b,
                     (float*)e.tensors[b.t_gate].ptr};
            hipLaunchKernelGGL(cls_se_kernel, dim3(B), dim3(256), 0, st, a);
            CLSHIP(hipGetLastError());
        }
        CLSHIP(launch_pw<T>(e, b.w_proj, e.tensors[b.t_dw].ptr, b.Hout * b.Hout, (const float*)e.tensors[b.t_gate].ptr,
                            b.residual ? cur : nullptr, e.tensors[b.t_out].ptr, nullptr, 0, B, st));
        cur = e.tensors[b.t_out].ptr;
    }
    const int H = e.blocks.back().Hout, HW = H * H;
    CLSHIP(launch_pw<T>(e, e.w_head, cur, HW, nullptr, nullptr, nullptr, e.d_part, 1, B, st));
    const ClsWeight& fc = e.weights[e.w_fc];
    FcArgs a{e.d_part, (HW + 31) / 32, HW, e.head_c, (const float*)fc.d_w, fc.d_b, (float*)e.tensors[e.t_pool].ptr, logits, prob, cls};
    hipLaunchKernelGGL(cls_fc_kernel, dim3(B), dim3(128), 0, st, a);
    CLSHIP(hipGetLastError());
    return YP_OK;
}

int run_any(yp_cls& e, const uint8_t* frames, int B, int FH, int FW, int bgr, const int* boxes, float* logits, float* prob, int* cls, hipStream_t st) {
    return e.dtype == DT_BF16 ? run_cls<uint16_t>(e, frames, B, FH, FW, bgr, boxes, logits, prob, cls, st)
                              : run_cls<float>(e, frames, B, FH, FW, bgr, boxes, logits, prob, cls, st);
}

uint16_t h_f2bf(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
float h_bfround(float f) {
    const uint32_t u = (uint32_t)h_f2bf(f) << 16;
    float r;
    memcpy(&r, &u, 4);
    return r;
}

// device layouts: stem [ky][kx][c][40] fp32; 1x1 [N^32][K^32] in the storage type; depthwise [k*k][C] fp32; SE / FC as given.
// In bf16 mode the conv weights (stem, depthwise, 1x1) are rounded to bf16; the SE and FC weights stay fp32.
void pack_weight(const yp_cls& e, const ClsWeight& w, std::vector<unsigned char>& buf) {
    const bool bf = e.dtype == DT_BF16;
    auto cw = [&](float v) { return bf ? h_bfround(v) : v; };
    if (w.kind == W_PW) {
        const int Np = (w.cout + 31) / 32 * 32;
        buf.assign((size_t)Np * w.Kpad * e.es(), 0);
        for (int n = 0; n < w.cout; ++n)
            for (int k = 0; k < w.cin; ++k) {
                const size_t i = (size_t)n * w.Kpad + k;
                const float v = w.w[(size_t)n * w.cin + k];
                if (bf) ((uint16_t*)buf.data())[i] = h_f2bf(v);
                else ((float*)buf.data())[i] = v;
            }
        return;
    }
    std::vector<float> out(w.w.size());
    if (w.kind == W_STEM) {
        for (int o = 0; o < w.cout; ++o)
            for (int c = 0; c < 3; ++c)
                for (int ky = 0; ky < 3; ++ky)
                    for (int kx = 0; kx < 3; ++kx) out[((ky * 3 + kx) * 3 + c) * w.cout + o] = cw(w.w[((o * 3 + c) * 3 + ky) * 3 + kx]);
    } else if (w.kind == W_DW) {
        for (int c = 0; c < w.cout; ++c)
            for (int t = 0; t < w.k * w.k; ++t) out[(size_t)t * w.cout + c] = cw(w.w[(size_t)c * w.k * w.k + t]);
    } else {
        out = w.w;
    }
    buf.resize(out.size() * 4);
    memcpy(buf.data(), out.data(), buf.size());
}

void weight_shape(const ClsWeight& w, int64_t shape[4], int* nd) {
    if (w.kind == W_FC) { shape[0] = w.cout; shape[1] = w.cin; shape[2] = shape[3] = 1; *nd = 2; return; }
    shape[0] = w.cout; shape[1] = w.cin; shape[2] = shape[3] = w.k; *nd = 4;
}

}  // namespace

extern "C" {

int yp_cls_create(int variant, int dtype, int device, yp_cls** out) {
    if (!out) return clsfail(YP_ERR_ARG, "null argument");
    if (dtype != YP_BF16 && dtype != YP_F32) return clsfail(YP_ERR_ARG, "bad dtype");
    std::unique_ptr<yp_cls> e(new yp_cls());
    e->variant = variant; e->dtype = dtype; e->device = device;
    if (const char* t = getenv("YOLOP_CLS_TAP_INPUT")) e->tap_input = atoi(t) != 0;
    const int rc = build_cls(*e);
    if (rc != YP_OK) return rc;
    *out = e.release();
    return YP_OK;
}

int yp_cls_destroy(yp_cls* e) {
    if (!e) return YP_OK;
    if (e->finalized || e->arena) { (void)hipSetDevice(e->device); (void)hipDeviceSynchronize(); }
    for (auto& w : e->weights) { if (w.d_w) (void)hipFree(w.d_w); if (w.d_b) (void)hipFree(w.d_b); }
    if (e->arena) (void)hipFree(e->arena);
    if (e->d_part) (void)hipFree(e->d_part);
    if (e->gexec) (void)hipGraphExecDestroy(e->gexec);
    if (e->cap_stream) (void)hipStreamDestroy(e->cap_stream);
    delete e;
    return YP_OK;
}

int yp_cls_weight_count(const yp_cls* e) { return e ? (int)e->weights.size() * 2 : clsfail(YP_ERR_ARG, "null engine"); }

int yp_cls_weight_info(const yp_cls* e, int i, char* name, int cap, int64_t shape[4], int* ndim) {
    if (!e || i < 0 || i >= (int)e->weights.size() * 2) return clsfail(YP_ERR_ARG, "bad weight index");
    const ClsWeight& w = e->weights[i / 2];
    const bool is_bias = i & 1;
    if (name && cap > 0) snprintf(name, cap, "%s.%s", w.name.c_str(), is_bias ? "bias" : "weight");
    int64_t s[4];
    int nd;
    if (is_bias) { s[0] = w.cout; s[1] = s[2] = s[3] = 1; nd = 1; }
    else weight_shape(w, s, &nd);
    if (shape) memcpy(shape, s, sizeof(s));
    if (ndim) *ndim = nd;
    return YP_OK;
}

int yp_cls_set_weight(yp_cls* e, const char* name, const float* host, const int64_t* shape, int ndim) {
    if (!e || !name || !host || !shape) return clsfail(YP_ERR_ARG, "null argument");
    if (e->finalized) return clsfail(YP_ERR_STATE, "engine already finalized");
    std::string n(name);
    const bool is_bias = n.size() > 5 && n.compare(n.size() - 5, 5, ".bias") == 0;
    const bool is_w = n.size() > 7 && n.compare(n.size() - 7, 7, ".weight") == 0;
    if (!is_bias && !is_w) return clsfail(YP_ERR_WEIGHT, "parameter name '%s' must end in .weight or .bias", name);
    auto it = e->wmap.find(n.substr(0, n.size() - (is_bias ? 5 : 7)));
    if (it == e->wmap.end()) return clsfail(YP_ERR_WEIGHT, "unknown parameter '%s'", name);
    ClsWeight& w = e->weights[it->second];
    if (is_bias) {
        if (ndim != 1 || shape[0] != w.cout) return clsfail(YP_ERR_WEIGHT, "'%s': expected shape [%d]", name, w.cout);
        w.b.assign(host, host + w.cout);
        w.have_b = true;
    } else {
        int64_t s[4];
        int nd;
        weight_shape(w, s, &nd);
        bool ok = ndim == nd;
        for (int d = 0; ok && d < nd; ++d) ok = shape[d] == s[d];
        if (!ok) return clsfail(YP_ERR_WEIGHT, "'%s': expected shape [%lld,%lld,%lld,%lld] (rank %d)", name, (long long)s[0], (long long)s[1],
                                (long long)s[2], (long long)s[3], nd);
        w.w.assign(host, host + (size_t)w.cout * w.cin * w.k * w.k);
        w.have_w = true;
    }
    return YP_OK;
}

int yp_cls_finalize(yp_cls* e) {
    if (!e) return clsfail(YP_ERR_ARG, "null engine");
    if (e->finalized) return YP_OK;
    for (const auto& w : e->weights)
        if (!w.have_w || !w.have_b) return clsfail(YP_ERR_WEIGHT, "parameter '%s.%s' was never set", w.name.c_str(), w.have_w ? "bias" : "weight");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return clsfail(YP_ERR_HIP, "no HIP device: the MI355X kernels cannot run here (no CPU fallback exists)");
    if (e->device < 0 || e->device >= ndev) return clsfail(YP_ERR_ARG, "device %d out of range (%d devices)", e->device, ndev);
    CLSHIP(hipSetDevice(e->device));
    std::vector<unsigned char> buf;
    for (ClsWeight& w : e->weights) {
        w.Kpad = (w.cin + 31) / 32 * 32;
        pack_weight(*e, w, buf);
        CLSHIP(hipMalloc(&w.d_w, buf.size()));
        CLSHIP(hipMemcpy(w.d_w, buf.data(), buf.size(), hipMemcpyHostToDevice));
        CLSHIP(hipMalloc((void**)&w.d_b, (size_t)w.cout * 4));
        CLSHIP(hipMemcpy(w.d_b, w.b.data(), (size_t)w.cout * 4, hipMemcpyHostToDevice));
    }
    e->finalized = true;
    return YP_OK;
}

int yp_cls_forward(yp_cls* e, const uint8_t* frames_dev, int B, int H, int W, int bgr, const int32_t* boxes_dev, float* logits_out,
                   float* prob_out, int32_t* cls_out, void* stream) {
    if (!e || !frames_dev || !boxes_dev || !logits_out || !prob_out || !cls_out) return clsfail(YP_ERR_ARG, "null argument");
    if (!e->finalized) return clsfail(YP_ERR_STATE, "yp_cls_finalize has not been called");
    if (B <= 0 || H <= 0 || W <= 0) return clsfail(YP_ERR_ARG, "bad shape B=%d H=%d W=%d", B, H, W);
    CLSHIP(hipSetDevice(e->device));
    int rc = plan_cls(*e, B);
    if (rc != YP_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    bgr = bgr ? 1 : 0;
    const void* key[6] = {frames_dev, boxes_dev, logits_out, prob_out, cls_out, e->arena};
    if (!e->use_graph) return run_any(*e, frames_dev, B, H, W, bgr, boxes_dev, logits_out, prob_out, cls_out, st);
    // replay: the graph is specialised on the pointers and the shape; a change re-captures (the first forward of a plan runs eagerly)
    const bool same = e->gexec && e->gB == B && e->gH == H && e->gW == W && e->gbgr == bgr && memcmp(key, e->gkey, sizeof(key)) == 0;
    if (!same) {
        rc = run_any(*e, frames_dev, B, H, W, bgr, boxes_dev, logits_out, prob_out, cls_out, st);
        if (rc != YP_OK) return rc;
        if (!e->cap_stream) CLSHIP(hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking));
        CLSHIP(hipStreamSynchronize(st));
        if (e->gexec) { (void)hipGraphExecDestroy(e->gexec); e->gexec = nullptr; }
        hipGraph_t g = nullptr;
        CLSHIP(hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeThreadLocal));
        rc = run_any(*e, frames_dev, B, H, W, bgr, boxes_dev, logits_out, prob_out, cls_out, e->cap_stream);
        const hipError_t ce = hipStreamEndCapture(e->cap_stream, &g);
        if (rc != YP_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
        if (ce != hipSuccess) return clsfail(YP_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(ce));
        CLSHIP(hipGraphInstantiate(&e->gexec, g, nullptr, nullptr, 0));
        (void)hipGraphDestroy(g);
        e->gB = B; e->gH = H; e->gW = W; e->gbgr = bgr;
        memcpy(e->gkey, key, sizeof(key));
        return YP_OK;
    }
    CLSHIP(hipGraphLaunch(e->gexec, st));
    return YP_OK;
}

int yp_cls_set_graph(yp_cls* e, int enable) {
    if (!e) return clsfail(YP_ERR_ARG, "null engine");
    e->use_graph = enable != 0;
    return YP_OK;
}

int yp_cls_tensor_count(const yp_cls* e) { return e ? (int)e->tensors.size() : clsfail(YP_ERR_ARG, "null engine"); }

int yp_cls_tensor_info(const yp_cls* e, int i, char* name, int cap, int dims[4]) {
    if (!e || i < 0 || i >= (int)e->tensors.size()) return clsfail(YP_ERR_ARG, "bad tensor index");
    const ClsTensor& t = e->tensors[i];
    if (name && cap > 0) snprintf(name, cap, "%s", t.name.c_str());
    if (dims) { dims[0] = e->pB; dims[1] = t.H; dims[2] = t.W; dims[3] = t.C; }
    return YP_OK;
}

int yp_cls_tensor_read(yp_cls* e, int i, float* host_out) {
    if (!e || i < 0 || i >= (int)e->tensors.size() || !host_out) return clsfail(YP_ERR_ARG, "bad argument");
    if (!e->arena) return clsfail(YP_ERR_STATE, "no forward has run yet");
    const ClsTensor& t = e->tensors[i];
    if (!t.ptr) return clsfail(YP_ERR_STATE, "tensor '%s' is not kept (the input tap needs YOLOP_CLS_TAP_INPUT=1 at create)", t.name.c_str());
    CLSHIP(hipSetDevice(e->device));
    CLSHIP(hipDeviceSynchronize());
    const size_t n = (size_t)e->pB * t.H * t.W * t.C;
    if (t.f32 || e->dtype == DT_F32) {
        CLSHIP(hipMemcpy(host_out, t.ptr, n * 4, hipMemcpyDeviceToHost));
    } else {
        std::vector<uint16_t> tmp(n);
        CLSHIP(hipMemcpy(tmp.data(), t.ptr, n * 2, hipMemcpyDeviceToHost));
        for (size_t j = 0; j < n; ++j) host_out[j] = bf2f(tmp[j]);
    }
    return YP_OK;
}

}  // extern "C"
