// PSA attention core, streaming matrix-core form in fp32 (key_dim 32, head_dim 64, any N >= 1): the strict-parity engines' kernel past the
// generic kernel's 2368 tokens, and from 401 tokens on where an engine asked for it (yp_set_attention_f32_stream). K and V pass through
// LDS in blocks of AF_KB keys, so a workgroup's LDS does not grow with N (attention.hip holds the generic fp32 kernel).
//
// Both products run on v_mfma_f32_16x16x4_f32, an exact fp32 FMA chain: no rounding point is added to the fp32 contract, only the order of
// the sums is the kernel's own (tests/attention_f32_stream_cases.py restates it on the CPU). Two passes, as the bf16
// streaming kernel takes them:
//   pass 1  streams K only: per query row the max m and the sum l of exp(s - m). Every lane keeps a running (m, l) over ITS keys
//           (rescaled when m grows: l enters the result only through 1/l) and the four lane groups of a row merge once at the end.
//   pass 2  streams K and V: recomputes S, P = exp(s - m) * (1/l), O += P.V. A key block accumulates in a fresh accumulator that is
//           added to the row's total behind the block: chains of AF_KB and of N / AF_KB additions, never one of N (whose rounding error
//           grows with sqrt(N): the comment in attention_kernel's P.V loop).
// The scale multiplies the finished dot product, as in the generic kernel.
//
// Fragments (A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15], D[row = 4 (lane >> 4) + reg][col = lane & 15]):
//   S^T = K.Q^T  K is the A operand, Q the B operand. Which key dimension a k-slot means is free as long as both sides agree: lane group g
//                holds d = 8g .. 8g+7 of its K row and of its query (two 16-byte reads each) and step s of the 8 takes d = 8g + s; steps
//                2c, 2c+1 form chain c of four, summed (c0 + c1) + (c2 + c3). D leaves a lane with ONE query (lane & 15) and keys 4g .. 4g+3 of a 16-key tile: the softmax reductions are in-lane
//                plus two shuffles.
//   O = P.V      that lane's four probabilities are the A operand of four steps: step r multiplies keys {r, 4+r, 8+r, 12+r} of the tile,
//                k-slot g = key 4g + r. The B operand of group g is V row 4g + r; column c of the MFMA means d = 4c + dt, so ONE
//                16-byte LDS read of the row-major V image feeds the four d tiles dt, and a lane ends up with four consecutive d of its
//                query rows 4g + reg: 16-byte stores, a 16-lane group writes one 256-byte output row.
//
// One workgroup = (image, head, a run of query groups); a query group = 4 waves x 16 queries (48 KB of LDS: three workgroups per CU).
// The matrix products run at the fp32 vector rate, so a wave's 16 queries are already ~27 us of matrix work per 1000 keys (128 MFMAs of
// 32 cycles per block of 64) and one image at 920 tokens needs the workgroups more than the K/V reuse: with 32 queries per wave
// (measured) one image and four heads at 920 tokens took 0.137 ms against the generic kernel's 0.085.
// K/V blocks are register-staged and double-buffered: the loads of block i+1 are issued in front of the MFMAs of block i and written to the other buffer behind them, one
// barrier per block. A query row is computed by one wave from the same blocks in the same order whatever the grid is: the output bits
// depend on neither batch nor split. No atomics.
#include "common.h"
#include <algorithm>

namespace yp {

constexpr int AF_KB = 64;                        // keys per block: 8 KB of K rows + 16 KB of V rows, twice
constexpr int AF_NW = 4;                         // waves per workgroup
constexpr int AF_TW = 1;                         // 16-query tiles per wave
constexpr int AF_QW = 16 * AF_TW;                // queries per wave
constexpr int AF_GROUP = AF_NW * AF_QW;          // queries per group
constexpr float AF_LOG2E = 1.44269504088896341f;
constexpr int AF_KBYTES = AF_KB * 128, AF_VBYTES = AF_KB * 256;
constexpr float AF_MIN = -3.0e38f;               // "no key yet": finite, so that (m_old - m_new) is never inf - inf

template <bool WITH_V> struct AfStage {
    static constexpr int NT = AF_NW * 64;
    static constexpr int NK = AF_KB * 8 / NT, NV = WITH_V ? AF_KB * 16 / NT : 0;
    u32x4 k[NK];
    u32x4 v[NV > 0 ? NV : 1];
    // rows of block kb (keys >= N: an offset no buffer holds = zeros; never whatever lies behind the tensor). K rows are 128 bytes,
    // their 16-byte chunks swizzled by cswz128(row); V rows are 256 bytes, as they lie in memory.
    __device__ __forceinline__ void load(const __amdgpu_buffer_rsrc_t rs, const AttnParams& p, size_t base_el, int kb, int tid) {
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            const int ch = tid + i * NT, row = ch >> 3, c = (ch & 7) ^ cswz128(row), key = kb * AF_KB + row;
            const unsigned off = key < p.N ? (unsigned)((base_el + (size_t)key * p.q_stride + 32 + c * 4) * 4) : kBufferOOB;
            k[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int ch = tid + i * NT, row = ch >> 4, c = ch & 15, key = kb * AF_KB + row;
            const unsigned off = key < p.N ? (unsigned)((base_el + (size_t)key * p.q_stride + 64 + c * 4) * 4) : kBufferOOB;
            v[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
        }
    }
    __device__ __forceinline__ void write(unsigned char* Ks, unsigned char* Vs, int tid) const {
#pragma unroll
        for (int i = 0; i < NK; ++i) *(u32x4*)(Ks + (tid + i * NT) * 16) = k[i];
#pragma unroll
        for (int i = 0; i < NV; ++i) *(u32x4*)(Vs + (tid + i * NT) * 16) = v[i];
    }
};

// exp(x) as the matrix-core kernels take it: one multiplication and v_exp_f32 (the accurate expf is ~10 instructions, and with the MFMAs
// at the fp32 vector rate the exponentials of a block cost as much issue time as its matrix products)
__device__ __forceinline__ float af_exp(float x) { return __builtin_amdgcn_exp2f(x * AF_LOG2E); }

// scaled scores of key tile j against the wave's query tiles: sc[t][reg] = (q_t[lane & 15] . k[16 j + 4 g + reg]) * scale, keys >= N
// at -inf (ragged: the block reaches past N, uniform)
__device__ __forceinline__ void af_scores(const unsigned char* Ks, unsigned koff0, unsigned koff1, int j, const float (&qf)[AF_TW][8], float scale,
                                          bool ragged, int key0, int N, f32x4 (&sc)[AF_TW]) {
    const f32x4 k0 = *(const f32x4*)(Ks + koff0 + j * 2048), k1 = *(const f32x4*)(Ks + koff1 + j * 2048);
    const float kf[8] = {k0[0], k0[1], k0[2], k0[3], k1[0], k1[1], k1[2], k1[3]};
#pragma unroll
    for (int t = 0; t < AF_TW; ++t) {
        // four chains of 8 key dimensions, added pairwise: one chain of 32 carries twice their rounding error, and on a row that one
        // key dominates the score's error is the output's; independent accumulators also hide the MFMA latency
        f32x4 part[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            part[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[2 * c], qf[t][2 * c], z, 0, 0, 0);
            part[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[2 * c + 1], qf[t][2 * c + 1], part[c], 0, 0, 0);
        }
        f32x4 acc = (part[0] + part[1]) + (part[2] + part[3]);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] *= scale;
        if (ragged) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (key0 + j * 16 + r >= N) acc[r] = -INFINITY;
        }
        sc[t] = acc;
    }
}

__global__ __launch_bounds__(AF_NW * 64) void attention_stream_f32_kernel(const AttnParams p, const int groups_per_wg, const unsigned qkv_bytes) {
    __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * (AF_KBYTES + AF_VBYTES)];
    constexpr int NW = AF_NW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, g = lane >> 4;
    const int bh = blockIdx.y, b = bh / p.nh, h = bh - b * p.nh;
    const size_t base_el = (size_t)b * p.N * p.q_stride + p.q_coff + h * 128;
    const float* base = (const float*)p.qkv + base_el;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.qkv, 0, (int)qkv_bytes, 0x00020000);
    const int nkb = (p.N + AF_KB - 1) / AF_KB;
    const int ngroups = (p.N + AF_GROUP - 1) / AF_GROUP;
    const int g0 = blockIdx.x * groups_per_wg, g1 = min(g0 + groups_per_wg, ngroups);

    // K fragment of key tile j: + j * 2048 (the chunk swizzle of a row depends on row & 15 only); chunks 2g and 2g + 1 of row fr
    const unsigned koff0 = fr * 128 + (((2 * g) ^ cswz128(fr)) * 16), koff1 = fr * 128 + (((2 * g + 1) ^ cswz128(fr)) * 16);
    // V fragment of key tile j, step r: + j * 4096 + r * 256; row 4g (+ r), d = 4 fr .. 4 fr + 3
    const unsigned voff = g * 1024 + fr * 16;

    for (int grp = g0; grp < g1; ++grp) {                       // (uniform: every wave meets every barrier)
        const int q0 = (grp * NW + wave) * AF_QW;
        float qf[AF_TW][8];
#pragma unroll
        for (int t = 0; t < AF_TW; ++t) {                            // query rows >= N: row N-1 again, never stored
            const float* qp = base + (size_t)min(q0 + t * 16 + fr, p.N - 1) * p.q_stride + g * 8;
            const f32x4 a = *(const f32x4*)qp, c = *(const f32x4*)(qp + 4);
#pragma unroll
            for (int s = 0; s < 4; ++s) { qf[t][s] = a[s]; qf[t][4 + s] = c[s]; }
        }

        // ---- pass 1: row max and sum ---------------------------------------------------------------------------------
        float m[AF_TW], l[AF_TW];
#pragma unroll
        for (int t = 0; t < AF_TW; ++t) { m[t] = AF_MIN; l[t] = 0.f; }
        {
            AfStage<false> sg;
            sg.load(rs, p, base_el, 0, tid);
            sg.write(lds, nullptr, tid);
            __syncthreads();
            for (int kb = 0; kb < nkb; ++kb) {
                const unsigned char* Ks = lds + (kb & 1) * AF_KBYTES;
                if (kb + 1 < nkb) sg.load(rs, p, base_el, kb + 1, tid);
                const bool ragged = (kb + 1) * AF_KB > p.N;
                f32x4 st[AF_KB / 16][AF_TW];
                float bm[AF_TW];
#pragma unroll
                for (int t = 0; t < AF_TW; ++t) bm[t] = AF_MIN;
#pragma unroll
                for (int j = 0; j < AF_KB / 16; ++j) {
                    af_scores(Ks, koff0, koff1, j, qf, p.scale, ragged, kb * AF_KB + g * 4, p.N, st[j]);
#pragma unroll
                    for (int t = 0; t < AF_TW; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) bm[t] = fmaxf(bm[t], st[j][t][r]);
                }
#pragma unroll
                for (int t = 0; t < AF_TW; ++t) {
                    const float mn = fmaxf(m[t], bm[t]);
                    float s = 0.f;
#pragma unroll
                    for (int j = 0; j < AF_KB / 16; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) s += af_exp(st[j][t][r] - mn);
                    l[t] = l[t] * af_exp(m[t] - mn) + s;
                    m[t] = mn;
                }
                if (kb + 1 < nkb) sg.write(lds + ((kb + 1) & 1) * AF_KBYTES, nullptr, tid);
                __syncthreads();
            }
        }
        float inv[AF_TW];
#pragma unroll
        for (int t = 0; t < AF_TW; ++t) {                            // the four lane groups of a query row
            float mm = fmaxf(m[t], __shfl_xor(m[t], 16, 64));
            mm = fmaxf(mm, __shfl_xor(mm, 32, 64));
            float s = l[t] * af_exp(m[t] - mm);
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            m[t] = mm;
            inv[t] = 1.0f / s;
        }

        // ---- pass 2: O = P.V ---------------------------------------------------------------------------------------------
        f32x4 o[AF_TW][4];
#pragma unroll
        for (int t = 0; t < AF_TW; ++t)
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        {
            AfStage<true> sg;
            unsigned char* const Kb = lds;
            unsigned char* const Vb = lds + 2 * AF_KBYTES;
            sg.load(rs, p, base_el, 0, tid);
            sg.write(Kb, Vb, tid);
            __syncthreads();
            for (int kb = 0; kb < nkb; ++kb) {
                const unsigned char* Ks = Kb + (kb & 1) * AF_KBYTES;
                const unsigned char* Vs = Vb + (kb & 1) * AF_VBYTES;
                if (kb + 1 < nkb) sg.load(rs, p, base_el, kb + 1, tid);
                const bool ragged = (kb + 1) * AF_KB > p.N;
                f32x4 ob[AF_TW][4];                                 // this block's share: a fresh accumulator
#pragma unroll
                for (int t = 0; t < AF_TW; ++t)
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) ob[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < AF_KB / 16; ++j) {
                    f32x4 sc[AF_TW];
                    af_scores(Ks, koff0, koff1, j, qf, p.scale, ragged, kb * AF_KB + g * 4, p.N, sc);
#pragma unroll
                    for (int t = 0; t < AF_TW; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) sc[t][r] = af_exp(sc[t][r] - m[t]) * inv[t];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const f32x4 vf = *(const f32x4*)(Vs + voff + j * 4096 + r * 256);
#pragma unroll
                        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                            for (int t = 0; t < AF_TW; ++t) ob[t][dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(sc[t][r], vf[dt], ob[t][dt], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int t = 0; t < AF_TW; ++t)
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) o[t][dt] += ob[t][dt];
                if (kb + 1 < nkb) sg.write(Kb + ((kb + 1) & 1) * AF_KBYTES, Vb + ((kb + 1) & 1) * AF_VBYTES, tid);
                __syncthreads();
            }
        }
        // D: col (lane & 15) = d 4 fr + dt, rows = queries g*4 + r: four consecutive d per lane and row
#pragma unroll
        for (int t = 0; t < AF_TW; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = q0 + t * 16 + g * 4 + r;
                if (q >= p.N) continue;
                float* op = (float*)p.o + ((size_t)b * p.N + q) * p.o_stride + p.o_coff + h * 64 + fr * 4;
                *(f32x4*)op = f32x4{o[t][0][r], o[t][1][r], o[t][2][r], o[t][3][r]};
            }
    }
}

// What the kernel takes: fp32, 32-wide keys and 64-wide heads, 16-byte fragments on both slices, 32-bit byte offsets into qkv.
bool attention_stream_f32_scope(const AttnParams& p, int dtype) {
    const size_t qkv_bytes = (size_t)p.B * p.N * p.q_stride * 4;
    return dtype == DT_F32 && p.kd == 32 && p.hd == 64 && p.N >= 1 && ((p.q_stride | p.q_coff | p.o_stride | p.o_coff) & 3) == 0 && qkv_bytes < (1ull << 31);
}

// (workgroups per head, query groups each walks): attention_stream_split's rule on this kernel's groups - runs as long as possible while
// the grid still reaches the workgroup target (wgs, else YOLOP_ATTN_WGS, else 1024). The default is four times the bf16 kernels': every
// group streams all of K and V, a run saves nothing but the launch of its workgroups, and a group here is 16 x the matrix time of a bf16
// one, so a short grid waits for its longest run (8 images x 1600 tokens x 4 heads, 25 groups a head: 0.409 ms as 7 runs of 4 a head
// under a target of 256, 0.307 ms as 25 workgroups a head). tests/attention_f32_stream_cases.py restates it.
static void attention_stream_f32_split(int B, int N, int nh, int wgs, int* nsplit_out, int* gpw_out) {
    static const int env_target = [] { const int v = env_int("YOLOP_ATTN_WGS", 0); return v > 0 ? v : 1024; }();
    const int target = wgs > 0 ? wgs : env_target;
    const int BH = B * nh;
    const int ngroups = (N + AF_GROUP - 1) / AF_GROUP;
    int nsplit = std::min(ngroups, std::max(1, (target + BH - 1) / BH));
    const int gpw = (ngroups + nsplit - 1) / nsplit;
    nsplit = (ngroups + gpw - 1) / gpw;
    *nsplit_out = nsplit; *gpw_out = gpw;
}

hipError_t launch_attention_stream_f32(const AttnParams& p, hipStream_t st, int wgs) {
    if (!attention_stream_f32_scope(p, DT_F32)) return hipErrorInvalidValue;
    const size_t qkv_bytes = (size_t)p.B * p.N * p.q_stride * 4;
    int nsplit, gpw;
    attention_stream_f32_split(p.B, p.N, p.nh, wgs, &nsplit, &gpw);
    hipLaunchKernelGGL(attention_stream_f32_kernel, dim3((unsigned)nsplit, (unsigned)(p.B * p.nh)), dim3(AF_NW * 64), 0, st, p, gpw, (unsigned)qkv_bytes);
    return hipGetLastError();
}

}  // namespace yp
