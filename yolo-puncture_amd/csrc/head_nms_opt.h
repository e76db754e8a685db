// The option forms of the NMS head (yp_set_nms_options: class set, class-agnostic NMS, max_nms): what head_nms_common.h does for the
// default form, cut into rounds. A round takes up to NCAP keys that all rank behind the keys of the rounds before it; boxes kept in
// earlier rounds suppress its candidates first, then the round's own greedy sweep appends to the kept rows. Over all rounds that is
// greedy NMS over the whole sorted list: a candidate stays iff no earlier KEPT box suppresses it.
// The default kernels do not include this file: their registers and LDS are what they were.
#pragma once
#include "head_nms_common.h"

namespace yp {

// the class set of the device block (common.h NMS_OPT_*): bit c of the mask words, or every class when no set is given
__device__ __forceinline__ bool nms_class_in_set(const unsigned* opt, const float cls) {
    if (!opt[NMS_OPT_USE_CLASSES]) return true;
    const unsigned c = (unsigned)cls;
    return c < (unsigned)(NMS_MASK_WORDS * 32) && ((opt[NMS_OPT_MASK + (c >> 5)] >> (c & 31)) & 1u);
}

// does kept box i (corners + class ci) suppress box bj? The arithmetic of nms_sort_sweep_rows: both boxes moved by the KEPT box's class
// offset (the other box has the same class, or the test is agnostic and nothing moves), fp32, `> iou` drops.
__device__ __forceinline__ bool nms_suppresses(const float* bi, const float* bj, const bool agnostic, const float iou_thr) {
    const float ci = bi[4];
    if (!agnostic && bj[4] != ci) return false;               // other classes sit 7680 px away: no intersection
    const float off = agnostic ? 0.f : ci * 7680.0f;
    const float ix1 = bi[0] + off, iy1 = bi[1] + off, ix2 = bi[2] + off, iy2 = bi[3] + off;
    const float iarea = (ix2 - ix1) * (iy2 - iy1);
    const float jx1 = bj[0] + off, jy1 = bj[1] + off, jx2 = bj[2] + off, jy2 = bj[3] + off;
    const float xx1 = fmaxf(ix1, jx1), yy1 = fmaxf(iy1, jy1), xx2 = fminf(ix2, jx2), yy2 = fminf(iy2, jy2);
    const float inter = fmaxf(xx2 - xx1, 0.f) * fmaxf(yy2 - yy1, 0.f);
    const float ovr = inter / (iarea + (jx2 - jx1) * (jy2 - jy1) - inter);
    return ovr > iou_thr;
}

// One round. keys[0..n) (n <= NCAP, unsorted, in the NCAP-slot dynamic LDS area; a barrier separates their writes from this call); the
// `ncut` (<= n) best of them take part. nk rows are kept so far (block-uniform); their boxes sit in s_kbox[0..nk) (null: a single round,
// nothing is carried). Writes rows [nk, nk') and returns nk'; ends with a barrier, after which keys may be overwritten.
static __device__ __forceinline__ int nms_opt_round(const HeadParams& p, unsigned long long* keys, int n, const int ncut, unsigned* s_dead, int* s_kept,
                                                    float (*s_kbox)[5], int nk, const NmsLocate& locate, const float iou_thr, const bool agnostic) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int A = p.A;
    const int nk0 = nk;
    int np2 = 2;
    while (np2 < n) np2 <<= 1;
    for (int i = n + tid; i < np2; i += NT) keys[i] = 0ull;
    for (int i = tid; i < NCAP / 32; i += NT) s_dead[i] = 0u;
    __syncthreads();
    // ---- bitonic sort, descending ---------------------------------------------------------------------------------------------
    for (int k = 2; k <= np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < np2; i += NT) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a = keys[i], c = keys[ixj];
                    const bool up = (i & k) == 0;
                    if (up ? (a < c) : (a > c)) { keys[i] = c; keys[ixj] = a; }
                }
            }
            __syncthreads();
        }
    n = min(n, ncut);                                         // the max_nms cut: the list is sorted, the tail leaves
    // ---- boxes into sorted order: the first `ncache` in the part of the key area the sort did not need ---------------------------
    const float* wsa = p.nms_ws + (size_t)b * A * 8;
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
    // ---- the boxes kept in earlier rounds all rank above this round's candidates: they suppress first ---------------------------
    if (s_kbox && nk > 0) {
        for (int j = tid; j < n; j += NT) {
            const float* bj = box_of(j);
            for (int k = 0; k < nk; ++k)
                if (nms_suppresses(s_kbox[k], bj, agnostic, iou_thr)) { atomicOr(&s_dead[j >> 5], 1u << (j & 31)); break; }
        }
        __syncthreads();
    }
    // ---- greedy NMS (the word walk of nms_sort_sweep_rows) ------------------------------------------------------------------------
    const int kmax = min(p.max_det, NMAXK);
    for (int w = 0; w * 32 < n && nk < kmax; ++w) {
        unsigned done = 0u;
        for (;;) {
            const int lim = min(32, n - w * 32);
            const unsigned valid = lim == 32 ? 0xffffffffu : ((1u << lim) - 1u);
            const unsigned alive = ~s_dead[w] & ~done & valid;
            if (!alive || nk >= kmax) break;
            const int bit = __builtin_ctz(alive);
            const int i = w * 32 + bit;
            done |= 1u << bit;
            const float* bsrc = box_of(i);
            const float bi[5] = {bsrc[0], bsrc[1], bsrc[2], bsrc[3], bsrc[4]};
            if (tid == 0) s_kept[nk] = i;
            if (s_kbox && tid < 5) s_kbox[nk][tid] = bsrc[tid];
            ++nk;
            for (int j = i + 1 + tid; j < n; j += NT) {
                if ((s_dead[j >> 5] >> (j & 31)) & 1u) continue;
                if (nms_suppresses(bi, box_of(j), agnostic, iou_thr)) atomicOr(&s_dead[j >> 5], 1u << (j & 31));
            }
            __syncthreads();
        }
    }
    __syncthreads();
    // ---- this round's rows -----------------------------------------------------------------------------------------------------------
    for (int r = nk0 + tid; r < nk; r += NT) {
        float* d = p.det + ((size_t)b * p.max_det + r) * 6;
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
    __syncthreads();
    return nk;
}

// rows past the kept count: zero / -1
static __device__ __forceinline__ void nms_opt_empty_rows(const HeadParams& p, const int nk) {
    const int b = blockIdx.x;
    for (int r = nk + (int)threadIdx.x; r < p.max_det; r += NT) {
        float* d = p.det + ((size_t)b * p.max_det + r) * 6;
#pragma unroll
        for (int j = 0; j < 6; ++j) d[j] = 0.f;
        if (p.idx) p.idx[(size_t)b * p.max_det + r] = -1;
        if (p.coeff)
            for (int j = 0; j < 32; ++j) p.coeff[((size_t)b * p.max_det + r) * 32 + j] = 0.f;
    }
}

}  // namespace yp
