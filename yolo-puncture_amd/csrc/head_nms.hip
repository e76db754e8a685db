// Post-process of the anchor-free heads that still need NMS (YOLOv8 / YOLO11 Detect + Segment - the checkpoints the reference's UI
// offers, yolo_seg/app.py:218-223): what `ops.non_max_suppression` does inside `.predict` [U], one workgroup per image:
//   candidates = anchors whose best class score exceeds conf (the per-level class-max keys of OP_AMAX)
//   -> sorted by (score desc, anchor asc) with a bitonic network in LDS
//   -> per candidate: class = first arg-max of the sigmoid scores, box = DFL expectation -> dist2bbox -> xywh -> xyxy (the
//      round trip of Detect._inference + xywh2xyxy is part of the reference's arithmetic)
//   -> greedy NMS on class-offset boxes (box + cls * 7680, IoU = inter / (a_i + a_j - inter) in fp32, drop when > iou): the scan over
//      the sorted list is sequential, the suppression by each KEPT box is one parallel sweep + one barrier (at most max_det of them)
//   -> rows [x1,y1,x2,y2,score,cls], anchor index, mask coefficients; rows past the kept count are zero / -1.
// A box never suppresses a higher-scoring one, so the rows above any conf' >= conf are the rows NMS at conf' would give.
#include "common.h"

#include "head_nms_common.h"
#include "head_nms_opt.h"

namespace yp {

// Kernel A (whole chip): for every anchor whose best score exceeds conf - class = first arg-max of the sigmoid scores, box = DFL
// expectation -> dist2bbox -> xywh -> xyxy - written at the ANCHOR's slot of the scratch [B][A][8]. One anchor per thread.
__global__ __launch_bounds__(256) void head_nms_decode_kernel(const HeadParams p) {
    const NmsLocate locate{p.hw[0][0] * p.hw[0][1], p.hw[1][0] * p.hw[1][1], p.hw[2][0] * p.hw[2][1]};
    const long item = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= (long)p.B * p.A) return;
    const int b = (int)(item / p.A), a = (int)(item - (long)b * p.A);
    int l, loc, HWl;
    locate(a, l, loc, HWl);
    const float conf = p.nms_params[0];
    if (!(p.mk[l][(size_t)b * HWl + loc] > __float_as_uint(fmaxf(conf, 0.f)))) return;
    const float* cp = p.cls[l] + ((size_t)b * HWl + loc) * p.nc;
    // `conf, j = cls.max(1)` takes the first maximum of the SIGMOID scores. sigmoid is monotone, so only classes whose logit is
    // within a hair of the largest logit - or, once that one saturates to 1.0f, any logit in the saturated range - can tie with it:
    // the sigmoid is evaluated for those alone
    float m = -INFINITY;
    for (int c = 0; c < p.nc; ++c) m = fmaxf(m, cp[c]);
    const float sm = sigmoid_ieee(m);
    const float lo = (sm >= 1.0f) ? 15.0f : m - fmaxf(1e-3f, 1e-4f * fabsf(m));
    float best = -1.f;
    int cls = 0;
    for (int c = 0; c < p.nc; ++c) {
        const float v = cp[c];
        if (v >= lo) {
            const float s = sigmoid_ieee(v);
            if (s > best) { best = s; cls = c; }
        }
    }
    const int Wl = p.hw[l][1];
    const int y = loc / Wl, x = loc - y * Wl;
    const float stride = (float)(8 << l);
    const float* bp = p.box[l] + ((size_t)b * HWl + loc) * 64;
    float dist[4];
#pragma unroll
    for (int sd = 0; sd < 4; ++sd) {
        float v[16], mx = -INFINITY;
#pragma unroll
        for (int q = 0; q < 16; ++q) { v[q] = bp[sd * 16 + q]; mx = fmaxf(mx, v[q]); }
        float sum = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) { v[q] = expf(v[q] - mx); sum += v[q]; }
        float e = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) e += (v[q] / sum) * (float)q;
        dist[sd] = e;
    }
    const float ax = (float)x + 0.5f, ay = (float)y + 0.5f;
    const float x1 = (ax - dist[0]) * stride, y1 = (ay - dist[1]) * stride, x2 = (ax + dist[2]) * stride, y2 = (ay + dist[3]) * stride;
    // dist2bbox(xywh=True) then xywh2xyxy
    const float cx = (x1 + x2) / 2.f, cy = (y1 + y2) / 2.f, w = x2 - x1, h = y2 - y1;
    float* o = p.nms_ws + ((size_t)b * p.A + a) * 8;
    o[0] = cx - w / 2.f; o[1] = cy - h / 2.f; o[2] = cx + w / 2.f; o[3] = cy + h / 2.f;
    o[4] = (float)cls;
}

// Kernel B (one workgroup per image): candidates -> sort -> greedy NMS -> rows
__global__ __launch_bounds__(NT) void head_nms_kernel(const HeadParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];     // [NCAP]
    __shared__ unsigned s_n;
    __shared__ unsigned s_dead[NCAP / 32];
    __shared__ int s_kept[NMAXK];
    const int b = blockIdx.x, tid = threadIdx.x;
    const NmsLocate locate{p.hw[0][0] * p.hw[0][1], p.hw[1][0] * p.hw[1][1], p.hw[2][0] * p.hw[2][1]};
    const float conf = p.nms_params[0], iou_thr = p.nms_params[1];
    const unsigned conf_bits = __float_as_uint(fmaxf(conf, 0.f));
    if (tid == 0) s_n = 0;
    for (int i = tid; i < NCAP / 32; i += NT) s_dead[i] = 0u;
    __syncthreads();
    // ---- candidates: score > conf (scores are sigmoids, >= 0: bit patterns order like the floats) ------------------------------
    {
        int off = 0;
        for (int l = 0; l < 3; ++l) {
            const int HWl = p.hw[l][0] * p.hw[l][1];
            const unsigned* src = p.mk[l] + (size_t)b * HWl;
            for (int a = tid; a < HWl; a += NT) {
                const unsigned sb = src[a];
                if (sb > conf_bits) keys[atomicAdd(&s_n, 1u)] = ((unsigned long long)sb << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)(off + a));
            }
            off += HWl;
        }
    }
    __syncthreads();
    nms_sort_sweep_rows(p, keys, (int)s_n, s_dead, s_kept, locate, iou_thr);
}

// Kernel B under yp_set_nms_options: candidates of the class set only (the class is in the scratch head_nms_decode_kernel filled), at most
// max_nms of them behind the sort, agnostic or class-offset sweep. A kernel of its own: head_nms_kernel keeps its registers.
__global__ __launch_bounds__(NT) void head_nms_opt_kernel(const HeadParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];     // [NCAP]
    __shared__ unsigned s_n;
    __shared__ unsigned s_dead[NCAP / 32];
    __shared__ int s_kept[NMAXK];
    const int b = blockIdx.x, tid = threadIdx.x;
    const NmsLocate locate{p.hw[0][0] * p.hw[0][1], p.hw[1][0] * p.hw[1][1], p.hw[2][0] * p.hw[2][1]};
    const float conf = p.nms_params[0], iou_thr = p.nms_params[1];
    const unsigned* opt = (const unsigned*)p.nms_params;
    const bool agnostic = opt[NMS_OPT_AGNOSTIC] != 0u;
    const int max_nms = (int)opt[NMS_OPT_MAX_NMS];
    const unsigned conf_bits = __float_as_uint(fmaxf(conf, 0.f));
    if (tid == 0) s_n = 0;
    __syncthreads();
    {
        const float* wsa = p.nms_ws + (size_t)b * p.A * 8;
        int off = 0;
        for (int l = 0; l < 3; ++l) {
            const int HWl = p.hw[l][0] * p.hw[l][1];
            const unsigned* src = p.mk[l] + (size_t)b * HWl;
            for (int a = tid; a < HWl; a += NT) {
                const unsigned sb = src[a];
                if (sb > conf_bits && nms_class_in_set(opt, wsa[(size_t)(off + a) * 8 + 4]))
                    keys[atomicAdd(&s_n, 1u)] = ((unsigned long long)sb << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)(off + a));
            }
            off += HWl;
        }
    }
    __syncthreads();
    const int n = (int)s_n;
    const int nk = nms_opt_round(p, keys, n, min(n, max_nms), s_dead, s_kept, nullptr, 0, locate, iou_thr, agnostic);
    nms_opt_empty_rows(p, nk);
}

const char* head_nms_kernel_name(int A, bool options) {
    if (A > HEAD_LDS_ANCHORS) return options ? "head_nms_gather_opt_kernel + head_nms_large_opt_kernel" : "head_nms_gather_kernel + head_nms_large_kernel";
    return options ? "head_nms_opt_kernel" : "head_nms_kernel";
}

// beyond HEAD_LDS_ANCHORS anchors (head_large.hip) the per-image candidate key lists [B][A] and their counters [B] follow the boxes
size_t head_nms_scratch_bytes(int B, int A) {
    const size_t boxes = (size_t)B * A * 8 * sizeof(float);
    return A <= HEAD_LDS_ANCHORS ? boxes : boxes + (size_t)B * A * sizeof(unsigned long long) + (((size_t)B * sizeof(unsigned) + 255) & ~(size_t)255);
}

hipError_t launch_head_nms(const HeadParams& p, hipStream_t st, bool options) {
    if (p.A > HEAD_MAX_ANCHORS || p.max_det > NMAXK || !p.mk[0] || !p.nms_params || !p.nms_ws) return hipErrorInvalidValue;
    const size_t sh = (size_t)NCAP * 8;
    static size_t granted = 0;
    if (hipError_t e = allow_dynamic_lds((const void*)head_nms_kernel, sh, granted)) return e;
    const long items = (long)p.B * p.A;
    hipLaunchKernelGGL(head_nms_decode_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, p);
    if (p.A > HEAD_LDS_ANCHORS) return launch_head_nms_large(p, st, options);      // (the LDS gather below has no room for them)
    if (options) {
        static size_t granted_opt = 0;
        if (hipError_t e = allow_dynamic_lds((const void*)head_nms_opt_kernel, sh, granted_opt)) return e;
        hipLaunchKernelGGL(head_nms_opt_kernel, dim3(p.B), dim3(NT), sh, st, p);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(head_nms_kernel, dim3(p.B), dim3(NT), sh, st, p);
    return hipGetLastError();
}

}  // namespace yp
