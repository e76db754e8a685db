// v10Detect one-to-one head epilogue + NMS-free post-process:
//   sigmoid -> per-anchor class max -> top-k anchors -> top-k of (k x nc) -> DFL decode of the winners only.
// Replaces Detect._inference (DFL, dist2bbox, make_anchors) + v10postprocess inside `.predict`
// (reference yolo_seg/app.py:91); spec SURVEY.md A.4 / A.6 [U]. The [B,8400,4+nc] decoded tensor of the
// reference is never materialised. Ordering rule: score descending, ties by flat index ascending
// (stage 1: anchor index; stage 2: stage-1 rank * nc + class) - encoded in unique 64-bit keys
//   key = float_bits(score) << 32 | (0xFFFFFFFF - flat_index)
// so "top-k by key" is exactly that rule. Two kernels:
//   anchor_max_kernel  (whole chip)   : coalesced pass over the class logits, one key per anchor
//   head_select_kernel (1 WG / image) : exact k-th-key radix select in LDS (8 x 8-bit passes over LDS histograms),
//                                       compaction, 512-key bitonic sort; stage 2 prefilters the k*nc candidates
//                                       with the stage-1 threshold and runs the same select in bounded rounds.
// The select and the kernel body live in head_select.h: head_large.hip (more than CAP anchors) shares them.
#include "common.h"

namespace yp {

// phase timestamps (s_memrealtime, 100 MHz) of image 0's workgroup in the last launch: tools read them through
// yp_debug_head_clocks to see where the select kernel's time goes
__device__ unsigned long long g_head_clk[8];
#define HEAD_STAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_head_clk[i] = wall_clock64(); } while (0)
#define HEAD_CLK7_RESET() do { if (blockIdx.x == 0 && threadIdx.x == 0) g_head_clk[7] = 0ull; } while (0)
#define HEAD_CLK7_ROUND(n) do { if (blockIdx.x == 0 && threadIdx.x == 0) g_head_clk[7] = (g_head_clk[7] & 0xffffffff00000000ull) + (1ull << 32) + (unsigned long long)(n); } while (0)

}  // namespace yp

#include "head_select.h"

namespace yp {

// ---------------------------------------------------------------------------------------------------------------
// kernel 1: m[a] = sigmoid(max_c logit[a][c]); 16 lanes per anchor, coalesced 64-B reads
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void anchor_max_kernel(const HeadParams p, unsigned* __restrict__ mkey) {
    const Locate locate{p.hw[0][0] * p.hw[0][1], p.hw[1][0] * p.hw[1][1], p.hw[2][0] * p.hw[2][1]};
    const int sub = threadIdx.x & 15;
    const long item = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;   // (image, anchor)
    const long total = (long)p.B * p.A;
    float mx = -INFINITY;
    if (item < total) {
        const int b = (int)(item / p.A), a = (int)(item - (long)b * p.A);
        int l, loc, HWl;
        locate(a, l, loc, HWl);
        const float* cp = p.cls[l] + ((size_t)b * HWl + loc) * p.nc;
        for (int c = sub; c < p.nc; c += 16) mx = fmaxf(mx, cp[c]);
    }
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 16));
    if (sub == 0 && item < total) mkey[item] = __float_as_uint(sigmoid_ieee(mx));
}

// nc % 4 == 0 form: a workgroup owns 64 consecutive anchors of one level of one image = 16*nc consecutive float4s, read
// with full-width coalesced loads; per-float4 maxima go through LDS and one thread per anchor finishes the row.
__global__ __launch_bounds__(256) void anchor_max4_kernel(const HeadParams p, unsigned* __restrict__ mkey, const int blocks_per_image,
                                                          const int nb0, const int nb1) {
    __shared__ float part[64 * 64];                    // [64 anchors][nc/4 <= 64]
    const int b = blockIdx.x / blocks_per_image, blk = blockIdx.x - b * blocks_per_image;
    const int A0 = p.hw[0][0] * p.hw[0][1], A1 = p.hw[1][0] * p.hw[1][1], A2 = p.hw[2][0] * p.hw[2][1];
    int l, a0, HWl, abase;
    if (blk < nb0) { l = 0; a0 = blk * 64; HWl = A0; abase = 0; }
    else if (blk < nb0 + nb1) { l = 1; a0 = (blk - nb0) * 64; HWl = A1; abase = A0; }
    else { l = 2; a0 = (blk - nb0 - nb1) * 64; HWl = A2; abase = A0 + A1; }
    const int na = min(64, HWl - a0);
    const int q = p.nc >> 2;                            // float4s per anchor
    const float4* src = (const float4*)(p.cls[l] + ((size_t)b * HWl + a0) * p.nc);
    const int n4 = na * q;
    for (int i = threadIdx.x; i < n4; i += 256) {
        const float4 v = src[i];
        part[i] = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
    }
    __syncthreads();
    // 4 threads per anchor
    const int a = threadIdx.x >> 2, sub = threadIdx.x & 3;
    float mx = -INFINITY;
    if (a < na)
        for (int j = sub; j < q; j += 4) mx = fmaxf(mx, part[a * q + j]);
    mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
    if (a < na && sub == 0) mkey[(size_t)b * p.A + abase + a0 + a] = __float_as_uint(sigmoid_ieee(mx));
}

// one level, one launch (OP_AMAX): the class-max pass of a level runs on that level's class lane as soon as its logits exist,
// so only the select kernel is left on the tail of the graph. Same arithmetic as anchor_max4_kernel.
__global__ __launch_bounds__(256) void anchor_max_level_kernel(const float* __restrict__ cls, const int B, const int HW, const int nc,
                                                               unsigned* __restrict__ out) {
    __shared__ float part[64 * 64];
    const int bpi = (HW + 63) / 64;
    const int b = blockIdx.x / bpi, a0 = (blockIdx.x - b * bpi) * 64;
    const int na = min(64, HW - a0);
    const int a = threadIdx.x >> 2, sub = threadIdx.x & 3;
    float mx = -INFINITY;
    if ((nc & 3) == 0 && nc <= 256) {
        const int q = nc >> 2;
        const float4* src = (const float4*)(cls + ((size_t)b * HW + a0) * nc);
        const int n4 = na * q;
        for (int i = threadIdx.x; i < n4; i += 256) {
            const float4 v = src[i];
            part[i] = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
        }
        __syncthreads();
        if (a < na)
            for (int j = sub; j < q; j += 4) mx = fmaxf(mx, part[a * q + j]);
    } else if (a < na) {
        const float* cp = cls + ((size_t)b * HW + a0 + a) * nc;
        for (int c = sub; c < nc; c += 4) mx = fmaxf(mx, cp[c]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
    if (a < na && sub == 0) out[(size_t)b * HW + a0 + a] = __float_as_uint(sigmoid_ieee(mx));
}

hipError_t launch_anchor_max_level(const float* cls, int B, int HW, int nc, unsigned* out, hipStream_t st) {
    hipLaunchKernelGGL(anchor_max_level_kernel, dim3((unsigned)(B * ((HW + 63) / 64))), dim3(256), 0, st, cls, B, HW, nc, out);
    return hipGetLastError();
}

template <int MODE>
__global__ __launch_bounds__(HT) void head_select_kernel(const HeadParams p, const unsigned* __restrict__ mkey) {
    head_select_body<MODE, false>(p, mkey, nullptr, 0);
}

hipError_t head_read_clocks(unsigned long long* out8) { return hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_head_clk), 8 * sizeof(unsigned long long)); }

// class-max keys of the mk == nullptr form; beyond CAP anchors the chunk winners of head_large.hip behind them
size_t head_scratch_bytes(int B, int A) {
    const size_t mkey = (size_t)B * A * sizeof(unsigned);
    return A <= CAP ? mkey : head_large_ckeys_offset(B, A) + (size_t)B * head_large_chunks(A) * MAXK * sizeof(unsigned long long);
}

static hipError_t head_attrs() {
    const size_t sh = (size_t)(CAP + 1536 + HT) * 8 + MAXK * 4 + MAXK * 8;
    static size_t granted[3] = {0, 0, 0};
    if (hipError_t e = allow_dynamic_lds((const void*)head_select_kernel<0>, sh, granted[0])) return e;
    if (hipError_t e = allow_dynamic_lds((const void*)head_select_kernel<1>, sh, granted[1])) return e;
    return allow_dynamic_lds((const void*)head_select_kernel<2>, sh, granted[2]);
}

hipError_t launch_head(const HeadParams& p, hipStream_t st) {
    if (p.A > HEAD_MAX_ANCHORS || p.max_det > MAXK || (p.scratch == nullptr && (p.mk[0] == nullptr || p.A > CAP))) return hipErrorInvalidValue;
    const size_t sh = (size_t)(CAP + 1536 + HT) * 8 + MAXK * 4 + MAXK * 8;
    hipError_t e = head_attrs();
    if (e != hipSuccess) return e;
    unsigned* mkey = (unsigned*)p.scratch;
    if (p.mk[0]) {
        // class-max keys were produced per level by OP_AMAX
    } else if ((p.nc & 3) == 0 && p.nc <= 256) {
        const int nb0 = (p.hw[0][0] * p.hw[0][1] + 63) / 64, nb1 = (p.hw[1][0] * p.hw[1][1] + 63) / 64, nb2 = (p.hw[2][0] * p.hw[2][1] + 63) / 64;
        const int bpi = nb0 + nb1 + nb2;
        hipLaunchKernelGGL(anchor_max4_kernel, dim3((unsigned)(p.B * bpi)), dim3(256), 0, st, p, mkey, bpi, nb0, nb1);
    } else {
        const long items = (long)p.B * p.A * 16;
        hipLaunchKernelGGL(anchor_max_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, p, mkey);
    }
    if (p.A > CAP) return launch_head_large(p, 0, st);
    hipLaunchKernelGGL(head_select_kernel<0>, dim3(p.B), dim3(HT), sh, st, p, mkey);
    return hipGetLastError();
}

// winners-only head: stage 1 (the per-level class-max keys must exist: p.mk), then the caller runs head_branch.hip, then stage 2 + decode
hipError_t launch_head_stage1(const HeadParams& p, hipStream_t st) {
    if (p.A > HEAD_MAX_ANCHORS || p.max_det > MAXK || p.mk[0] == nullptr || !p.sp_sel || !p.sp_wlist || !p.sp_wcount || !p.sp_thr) return hipErrorInvalidValue;
    if (p.A > CAP) return p.scratch ? launch_head_large(p, 1, st) : hipErrorInvalidValue;
    const size_t sh = (size_t)(CAP + 1536 + HT) * 8 + MAXK * 4 + MAXK * 8;
    hipError_t e = head_attrs();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(head_select_kernel<1>, dim3(p.B), dim3(HT), sh, st, p, (const unsigned*)nullptr);
    return hipGetLastError();
}
hipError_t launch_head_stage2(const HeadParams& p, hipStream_t st) {
    if (p.A > HEAD_MAX_ANCHORS || p.max_det > MAXK || !p.sp_sel || !p.sp_thr || !p.sp_box) return hipErrorInvalidValue;      // (nothing in stage 2 grows with A)
    const size_t sh = (size_t)(CAP + 1536 + HT) * 8 + MAXK * 4 + MAXK * 8;
    hipError_t e = head_attrs();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(head_select_kernel<2>, dim3(p.B), dim3(HT), sh, st, p, (const unsigned*)nullptr);
    return hipGetLastError();
}

}  // namespace yp
