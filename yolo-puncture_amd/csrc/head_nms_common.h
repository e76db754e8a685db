// Shared by head_nms.hip and head_large.hip: what the NMS kernel does once an image's candidate keys sit in LDS - sort, boxes into
// sorted order, greedy NMS, rows.
#pragma once
#include "common.h"

namespace yp {

constexpr int NT = 1024;
constexpr int NCAP = 16384;           // sorted-key capacity (power of two >= the 12288-anchor limit of the plan)
constexpr int NMAXK = 512;
static_assert(NMAXK == HEAD_MAXK, "one row bound for both heads: include/yolop.h YP_MAX_DET");

struct NmsLocate {
    int A0, A1, A2;
    __device__ __forceinline__ void operator()(int a, int& l, int& loc, int& HWl) const {
        if (a < A0) { l = 0; loc = a; HWl = A0; }
        else if (a < A0 + A1) { l = 1; loc = a - A0; HWl = A1; }
        else { l = 2; loc = a - A0 - A1; HWl = A2; }
    }
};

// keys[0..n) (n <= NCAP, unsorted, in the NCAP-slot dynamic LDS area) -> the image's rows. s_dead is cleared; a barrier separates the
// writes of keys from this call.
static __device__ __forceinline__ void nms_sort_sweep_rows(const HeadParams& p, unsigned long long* keys, const int n, unsigned* s_dead, int* s_kept,
                                                           const NmsLocate& locate, const float iou_thr) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int A = p.A;
    int np2 = 2;
    while (np2 < n) np2 <<= 1;
    for (int i = n + tid; i < np2; i += NT) keys[i] = 0ull;
    __syncthreads();
    // ---- bitonic sort, descending ---------------------------------------------------------------------------------------------
    for (int k = 2; k <= np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < np2; i += NT) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a = keys[i], c = keys[ixj];
                    const bool up = (i & k) == 0;           // descending blocks first
                    if (up ? (a < c) : (a > c)) { keys[i] = c; keys[ixj] = a; }
                }
            }
            __syncthreads();
        }
    // ---- per candidate: class and box were computed per anchor by head_nms_decode_kernel; bring them into sorted order -----------
    const float* wsa = p.nms_ws + (size_t)b * A * 8;      // by anchor
    // the first `ncache` boxes of the sorted list live in the part of the key area the sort did not need (5 floats each): the sweep of
    // a kept box then costs LDS latency instead of dependent trips to L2
    float* cache = (float*)(keys + np2);
    const int ncache = min(n, (int)(((size_t)(NCAP - np2) * 8) / 20));
    for (int i = tid; i < ncache; i += NT) {
        const int a = (int)(0xFFFFFFFFu - (unsigned)(keys[i] & 0xFFFFFFFFull));
        const float* src = wsa + (size_t)a * 8;
        float* c5 = cache + (size_t)i * 5;
        c5[0] = src[0]; c5[1] = src[1]; c5[2] = src[2]; c5[3] = src[3]; c5[4] = src[4];
    }
    __syncthreads();
    auto box_of = [&](int i) -> const float* {
        if (i < ncache) return cache + (size_t)i * 5;
        return wsa + (size_t)(int)(0xFFFFFFFFu - (unsigned)(keys[i] & 0xFFFFFFFFull)) * 8;
    };
    // ---- greedy NMS ----------------------------------------------------------------------------------------------------------------
    const int kmax = min(p.max_det, NMAXK);
    int nk = 0;
    // walk the sorted list word by word: the next survivor is the lowest clear bit at or after the cursor (every thread reads the same
    // LDS word: a broadcast, the branches are uniform); only KEPT boxes cost a sweep and a barrier
    for (int w = 0; w * 32 < n && nk < kmax; ++w) {
        unsigned done = 0u;                                   // bits of this word already handled (kept) in this pass over it
        for (;;) {
            const int lim = min(32, n - w * 32);
            const unsigned valid = lim == 32 ? 0xffffffffu : ((1u << lim) - 1u);
            const unsigned alive = ~s_dead[w] & ~done & valid;
            if (!alive || nk >= kmax) break;
            const int bit = __builtin_ctz(alive);
            const int i = w * 32 + bit;
            done |= 1u << bit;
            if (tid == 0) s_kept[nk] = i;
            ++nk;
            const float* bi = box_of(i);
            const float ci = bi[4];
            const float off = ci * 7680.0f;
            const float ix1 = bi[0] + off, iy1 = bi[1] + off, ix2 = bi[2] + off, iy2 = bi[3] + off;
            const float iarea = (ix2 - ix1) * (iy2 - iy1);
            for (int j = i + 1 + tid; j < n; j += NT) {
                if ((s_dead[j >> 5] >> (j & 31)) & 1u) continue;
                const float* bj = box_of(j);
                if (bj[4] != ci) continue;                   // other classes sit 7680 px away: no intersection
                const float jx1 = bj[0] + off, jy1 = bj[1] + off, jx2 = bj[2] + off, jy2 = bj[3] + off;
                const float xx1 = fmaxf(ix1, jx1), yy1 = fmaxf(iy1, jy1), xx2 = fminf(ix2, jx2), yy2 = fminf(iy2, jy2);
                const float inter = fmaxf(xx2 - xx1, 0.f) * fmaxf(yy2 - yy1, 0.f);
                const float ovr = inter / (iarea + (jx2 - jx1) * (jy2 - jy1) - inter);
                if (ovr > iou_thr) atomicOr(&s_dead[j >> 5], 1u << (j & 31));
            }
            __syncthreads();
        }
    }
    __syncthreads();
    // ---- rows ------------------------------------------------------------------------------------------------------------------------
    for (int r = tid; r < p.max_det; r += NT) {
        float* d = p.det + ((size_t)b * p.max_det + r) * 6;
        if (r >= nk) {
#pragma unroll
            for (int j = 0; j < 6; ++j) d[j] = 0.f;
            if (p.idx) p.idx[(size_t)b * p.max_det + r] = -1;
            if (p.coeff)
                for (int j = 0; j < 32; ++j) p.coeff[((size_t)b * p.max_det + r) * 32 + j] = 0.f;
            continue;
        }
        const int i = s_kept[r];
        const unsigned long long key = keys[i];
        const int a = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
        const float* bi = box_of(i);
        d[0] = bi[0]; d[1] = bi[1]; d[2] = bi[2]; d[3] = bi[3];
        d[4] = __uint_as_float((unsigned)(key >> 32));
        d[5] = bi[4];
        if (p.idx) p.idx[(size_t)b * p.max_det + r] = a;
        if (p.coeff) {
            int l, loc, HWl;
            locate(a, l, loc, HWl);
            const float* cf = p.cf[l] + ((size_t)b * HWl + loc) * 32;
            for (int j = 0; j < 32; ++j) p.coeff[((size_t)b * p.max_det + r) * 32 + j] = cf[j];
        }
    }
}

}  // namespace yp
