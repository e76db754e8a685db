// The heads' post-process for inputs whose three levels hold more anchors than one workgroup's LDS (CAP = 12288): the same exact
// ordering rule (unique 64-bit keys) as head.hip / head_nms.hip, LDS use bounded by constants, no host read-back and no
// data-dependent launch dimension.
//   v10 top-k head: stage 1 is the only part whose storage grows with A.
//     head_chunk_topk_kernel     (1 WG / (image, chunk of <= CAP anchors), whole chip): the select of head.hip on the chunk; its
//                                min(k, chunk size) best keys - they carry the image-wide anchor index, so tie order survives - go to global memory
//     head_select_large_kernel   (1 WG / image): top k of the <= nchunks * k <= CAP chunk winners (a key outside its chunk's top k is
//                                outside the image's), then what head_select_kernel<0 / 1> does behind stage 1, from the same body
//   The "k-th largest per-thread maximum is a lower bound" prefilter of head.hip is used inside a chunk only: there its survivors are at
//   most the chunk, which is at most CAP; over a whole image nothing bounds them.
//   NMS heads (v8 / 11): head_nms_kernel gathers candidates straight into LDS, safe only while A <= NCAP.
//     head_nms_gather_kernel     (whole chip): anchors above conf -> a per-image key list in global memory (one atomic per wave)
//     head_nms_large_kernel      (1 WG / image): the list -> LDS; when it holds more than NCAP keys, exactly the NCAP largest take part
//                                (exact radix threshold over the global list); then the sort / sweep / rows of head_nms.hip
#include "common.h"

#define HEAD_STAMP(i) do { } while (0)
#define HEAD_CLK7_RESET() do { } while (0)
#define HEAD_CLK7_ROUND(n) do { } while (0)
#include "head_select.h"
#include "head_nms_common.h"
#include "head_nms_opt.h"

namespace yp {

static_assert(CAP == HEAD_LDS_ANCHORS && MAXK == HEAD_MAXK && NT == HT, "one set of bounds");
static_assert((HEAD_MAX_ANCHORS / CAP) * MAXK <= CAP, "the chunk winners of an image fit the merge kernel's key area");

// ---------------------------------------------------------------------------------------------------------------
// v10: chunk pass
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HT) void head_chunk_topk_kernel(const HeadParams p, const unsigned* __restrict__ mkey, unsigned long long* __restrict__ ckeys,
                                                             const int nchunks) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds[];
    unsigned long long* keys = lds;                 // [CAP]
    unsigned long long* best = lds + CAP;           // [512]
    unsigned long long* tmp = best + 512;           // [512]
    unsigned long long* tmaxs = tmp + 512;          // [HT]
    __shared__ SelectShared S;
    __shared__ unsigned nfill;
    const unsigned* const mk0 = p.mk[0]; const unsigned* const mk1 = p.mk[1]; const unsigned* const mk2 = p.mk[2];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / nchunks, c = blockIdx.x - b * nchunks;
    const int A = p.A, a0 = c * CAP, n = min(CAP, A - a0), kc = min(p.max_det, n);
    const Locate locate{p.hw[0][0] * p.hw[0][1], p.hw[1][0] * p.hw[1][1], p.hw[2][0] * p.hw[2][1]};
    // as stage 1 of head_select_kernel, on anchors [a0, a0 + n): keys in registers, the kc-th largest per-thread maximum T0 bounds the
    // kc-th largest key from below (kc <= min(n, HT) threads hold a key), the exact select looks at the keys >= T0 only
    constexpr int NPT = CAP / HT;
    unsigned long long kreg[NPT];
    unsigned sbits[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const int a = a0 + min(tid + i * HT, n - 1);
        if (mk0) {                                                // (uniform)
            int l, loc, HWl;
            locate(a, l, loc, HWl);
            sbits[i] = (l == 0 ? mk0 : l == 1 ? mk1 : mk2)[(size_t)b * HWl + loc];
        } else sbits[i] = mkey[(size_t)b * A + a];
    }
    unsigned long long tmx = 0ull;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const int j = tid + i * HT;
        kreg[i] = j < n ? (((unsigned long long)sbits[i] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)(a0 + j))) : 0ull;
        tmx = kreg[i] > tmx ? kreg[i] : tmx;
    }
    tmaxs[tid] = tmx;
    if (tid == 0) nfill = 0u;
    __syncthreads();
    const unsigned long long T0 = radix_kth(tmaxs, HT, kc, S, (unsigned)A);
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const bool have = kreg[i] != 0ull && kreg[i] >= T0;
        const unsigned pos = wave_append(have, &nfill);          // (<= n <= CAP survivors)
        if (have) keys[pos] = kreg[i];
    }
    __syncthreads();
    select_topk_sorted(keys, (int)nfill, kc, best, tmp, S, (unsigned)A);
    unsigned long long* dst = ckeys + ((size_t)b * nchunks + c) * MAXK;
    for (int r = tid; r < kc; r += HT) dst[r] = best[r];
}

template <int MODE>
__global__ __launch_bounds__(HT) void head_select_large_kernel(const HeadParams p, const unsigned long long* __restrict__ ckeys, const int nchunks) {
    head_select_body<MODE, true>(p, nullptr, ckeys, nchunks);
}

const char* head_large_kernel_name(int mode) {
    return mode == 0 ? "head_chunk_topk_kernel + head_select_large_kernel<0>" : "head_chunk_topk_kernel + head_select_large_kernel<1>";
}

// mode 0: the whole head (the class-max keys are p.mk, or the [B][A] array at the start of p.scratch); mode 1: stage 1 with the winners hand-over
hipError_t launch_head_large(const HeadParams& p, int mode, hipStream_t st) {
    if (p.A <= CAP || p.A > HEAD_MAX_ANCHORS || p.max_det > MAXK || p.max_det < 1 || !p.scratch || (mode != 0 && mode != 1)) return hipErrorInvalidValue;
    const size_t sh_chunk = (size_t)(CAP + 1024 + HT) * 8;
    const size_t sh = (size_t)(CAP + 1536 + HT) * 8 + MAXK * 4 + MAXK * 8;
    static size_t granted[3] = {0, 0, 0};
    if (hipError_t e = allow_dynamic_lds((const void*)head_chunk_topk_kernel, sh_chunk, granted[0])) return e;
    const int nchunks = head_large_chunks(p.A);
    unsigned long long* ckeys = (unsigned long long*)((char*)p.scratch + head_large_ckeys_offset(p.B, p.A));
    const unsigned* mkey = p.mk[0] ? nullptr : (const unsigned*)p.scratch;
    hipLaunchKernelGGL(head_chunk_topk_kernel, dim3((unsigned)(p.B * nchunks)), dim3(HT), sh_chunk, st, p, mkey, ckeys, nchunks);
    if (mode == 0) {
        if (hipError_t e = allow_dynamic_lds((const void*)head_select_large_kernel<0>, sh, granted[1])) return e;
        hipLaunchKernelGGL(head_select_large_kernel<0>, dim3(p.B), dim3(HT), sh, st, p, (const unsigned long long*)ckeys, nchunks);
    } else {
        if (hipError_t e = allow_dynamic_lds((const void*)head_select_large_kernel<1>, sh, granted[2])) return e;
        hipLaunchKernelGGL(head_select_large_kernel<1>, dim3(p.B), dim3(HT), sh, st, p, (const unsigned long long*)ckeys, nchunks);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// NMS heads
// ---------------------------------------------------------------------------------------------------------------
// grid (ceil(A / 256), B): a wave never spans two images, so one atomic per wave appends its candidates to the image's list
__global__ __launch_bounds__(256) void head_nms_gather_kernel(const HeadParams p, unsigned long long* __restrict__ glist, unsigned* __restrict__ gcount) {
    const NmsLocate locate{p.hw[0][0] * p.hw[0][1], p.hw[1][0] * p.hw[1][1], p.hw[2][0] * p.hw[2][1]};
    const int b = blockIdx.y, a = blockIdx.x * 256 + threadIdx.x;
    const unsigned conf_bits = __float_as_uint(fmaxf(p.nms_params[0], 0.f));
    unsigned sb = 0u;
    if (a < p.A) {
        int l, loc, HWl;
        locate(a, l, loc, HWl);
        sb = p.mk[l][(size_t)b * HWl + loc];
    }
    const bool have = a < p.A && sb > conf_bits;
    const unsigned pos = wave_append(have, gcount + b);          // (at most A per image: the list holds A keys)
    if (have) glist[(size_t)b * p.A + pos] = ((unsigned long long)sb << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)a);
}

__global__ __launch_bounds__(NT) void head_nms_large_kernel(const HeadParams p, const unsigned long long* __restrict__ glist, const unsigned* __restrict__ gcount) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];     // [NCAP]
    __shared__ SelectShared S;
    __shared__ unsigned s_n;
    __shared__ unsigned s_dead[NCAP / 32];
    __shared__ int s_kept[NMAXK];
    const int b = blockIdx.x, tid = threadIdx.x;
    const NmsLocate locate{p.hw[0][0] * p.hw[0][1], p.hw[1][0] * p.hw[1][1], p.hw[2][0] * p.hw[2][1]};
    const float iou_thr = p.nms_params[1];
    const unsigned long long* list = glist + (size_t)b * p.A;
    const int nall = (int)min(gcount[b], (unsigned)p.A);
    if (tid == 0) s_n = 0;
    for (int i = tid; i < NCAP / 32; i += NT) s_dead[i] = 0u;
    int n = nall;
    if (nall <= NCAP) {
        for (int i = tid; i < nall; i += NT) keys[i] = list[i];
    } else {
        // more candidates than the sort holds: the NCAP largest keys, exactly (keys are unique: NCAP of them reach the NCAP-th largest)
        const unsigned long long kth = radix_kth(list, nall, NCAP, S, (unsigned)p.A);
        for (int i = tid; i < nall; i += NT) {
            const unsigned long long key = list[i];
            const bool have = key >= kth;
            const unsigned pos = wave_append(have, &s_n);
            if (have && pos < (unsigned)NCAP) keys[pos] = key;
        }
        n = NCAP;
    }
    __syncthreads();
    nms_sort_sweep_rows(p, keys, n, s_dead, s_kept, locate, iou_thr);
}

// The two kernels under yp_set_nms_options. The gather leaves out the classes outside the set; the NMS kernel walks the max_nms best keys of
// the list in rounds of NCAP: round r takes the keys of rank [r * NCAP, min((r + 1) * NCAP, max_nms, nall)) - below the threshold the round
// before ended on, down to the exact radix threshold of its last rank (keys are unique: exactly r1 keys reach the r1-th largest). Still one
// workgroup per image, no read-back, no data-dependent launch dimension.
__global__ __launch_bounds__(256) void head_nms_gather_opt_kernel(const HeadParams p, unsigned long long* __restrict__ glist, unsigned* __restrict__ gcount) {
    const NmsLocate locate{p.hw[0][0] * p.hw[0][1], p.hw[1][0] * p.hw[1][1], p.hw[2][0] * p.hw[2][1]};
    const int b = blockIdx.y, a = blockIdx.x * 256 + threadIdx.x;
    const unsigned conf_bits = __float_as_uint(fmaxf(p.nms_params[0], 0.f));
    const unsigned* opt = (const unsigned*)p.nms_params;
    unsigned sb = 0u;
    if (a < p.A) {
        int l, loc, HWl;
        locate(a, l, loc, HWl);
        sb = p.mk[l][(size_t)b * HWl + loc];
    }
    // (the class slot of the scratch is written for the anchors above conf only: read it behind that test)
    const bool have = a < p.A && sb > conf_bits && nms_class_in_set(opt, p.nms_ws[((size_t)b * p.A + a) * 8 + 4]);
    const unsigned pos = wave_append(have, gcount + b);
    if (have) glist[(size_t)b * p.A + pos] = ((unsigned long long)sb << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)a);
}

__global__ __launch_bounds__(NT) void head_nms_large_opt_kernel(const HeadParams p, const unsigned long long* __restrict__ glist, const unsigned* __restrict__ gcount) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];     // [NCAP]
    __shared__ SelectShared S;
    __shared__ unsigned s_n;
    __shared__ unsigned s_dead[NCAP / 32];
    __shared__ int s_kept[NMAXK];
    __shared__ float s_kbox[NMAXK][5];                                            // boxes and classes of the rows kept so far
    const int b = blockIdx.x, tid = threadIdx.x;
    const NmsLocate locate{p.hw[0][0] * p.hw[0][1], p.hw[1][0] * p.hw[1][1], p.hw[2][0] * p.hw[2][1]};
    const float iou_thr = p.nms_params[1];
    const unsigned* opt = (const unsigned*)p.nms_params;
    const bool agnostic = opt[NMS_OPT_AGNOSTIC] != 0u;
    const unsigned long long* list = glist + (size_t)b * p.A;
    const int nall = (int)min(gcount[b], (unsigned)p.A);
    const int nuse = min(nall, (int)opt[NMS_OPT_MAX_NMS]);
    const int kmax = min(p.max_det, NMAXK);
    int nk = 0;
    unsigned long long hi = 0ull;                                 // the threshold the previous round ended on: this round's keys lie below it
    for (int r0 = 0; r0 < nuse && nk < kmax; r0 += NCAP) {
        const int r1 = min(r0 + NCAP, nuse);
        const unsigned long long lo = r1 < nall ? radix_kth(list, nall, r1, S, (unsigned)p.A) : 0ull;
        if (tid == 0) s_n = 0;
        __syncthreads();
        for (int i = tid; i < nall; i += NT) {
            const unsigned long long key = list[i];
            const bool have = key >= lo && (r0 == 0 || key < hi);
            const unsigned pos = wave_append(have, &s_n);
            if (have && pos < (unsigned)NCAP) keys[pos] = key;
        }
        __syncthreads();
        nk = nms_opt_round(p, keys, r1 - r0, r1 - r0, s_dead, s_kept, s_kbox, nk, locate, iou_thr, agnostic);
        hi = lo;
    }
    nms_opt_empty_rows(p, nk);
}

// (called by launch_head_nms behind head_nms_decode_kernel)
hipError_t launch_head_nms_large(const HeadParams& p, hipStream_t st, bool options) {
    if (p.A <= HEAD_LDS_ANCHORS || p.A > HEAD_MAX_ANCHORS || p.max_det > NMAXK || !p.mk[0] || !p.nms_params || !p.nms_ws) return hipErrorInvalidValue;
    const size_t sh = (size_t)NCAP * 8;
    static size_t granted = 0;
    if (hipError_t e = allow_dynamic_lds((const void*)head_nms_large_kernel, sh, granted)) return e;
    // behind the [B][A][8] boxes of head_nms_scratch_bytes: the key lists, then the counters (emptied for every forward)
    unsigned long long* glist = (unsigned long long*)(p.nms_ws + (size_t)p.B * p.A * 8);
    unsigned* gcount = (unsigned*)(glist + (size_t)p.B * p.A);
    if (hipError_t e = hipMemsetAsync(gcount, 0, (size_t)p.B * sizeof(unsigned), st)) return e;
    if (options) {
        static size_t granted_opt = 0;
        if (hipError_t e = allow_dynamic_lds((const void*)head_nms_large_opt_kernel, sh, granted_opt)) return e;
        hipLaunchKernelGGL(head_nms_gather_opt_kernel, dim3((unsigned)((p.A + 255) / 256), (unsigned)p.B), dim3(256), 0, st, p, glist, gcount);
        hipLaunchKernelGGL(head_nms_large_opt_kernel, dim3(p.B), dim3(NT), sh, st, p, (const unsigned long long*)glist, (const unsigned*)gcount);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(head_nms_gather_kernel, dim3((unsigned)((p.A + 255) / 256), (unsigned)p.B), dim3(256), 0, st, p, glist, gcount);
    hipLaunchKernelGGL(head_nms_large_kernel, dim3(p.B), dim3(NT), sh, st, p, (const unsigned long long*)glist, (const unsigned*)gcount);
    return hipGetLastError();
}

}  // namespace yp
