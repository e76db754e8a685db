// PSA attention core, streaming matrix-core form (bf16, key_dim 32, head_dim 64, any N >= 1): K and V pass through LDS in blocks of
// AS_KB keys, so a workgroup's LDS does not grow with N (attention.hip holds the resident form, N <= 400, and the generic fp32 one).
//
// Rounding points are the oracle's (oracle/yolov10_oracle.py::attention in bf16 mode, tests/attention_ref.py): P is the NORMALISED
// probability rounded to bf16, P.V accumulates in fp32 in a fixed key order, the output is rounded once. A one-pass flash form rounds
// exp(s - running max) and rescales O, i.e. rounds every probability somewhere else ("Streaming attention"); so two passes:
//   pass 1  streams K only: per query row the max m and the sum l of exp2((s - m) c). Every lane keeps a running (m, l) over ITS keys
//           (rescaled when m grows: l enters the result only through 1/l) and the four lane groups of a row merge once at the end.
//   pass 2  streams K and V: recomputes S, P = bf16(exp2((s - m) c) * (1/l)), O += P.V.
// Fragments are those of attention_mfma_kernel: S^T = K.Q^T (K the MFMA A operand, Q the B operand) leaves a lane with ONE query
// (lane & 15) and keys 4g .. 4g+3 of each 16-key tile, so P is already P.V's A operand under the k-slot permutation
// {4g..4g+3, 16+4g..16+4g+3} of a 32-key step; V's B operand comes from the row-major pair-swizzled V image through ds_read_b64_tr_b16.
//
// One workgroup = (image, head, a run of query groups); a query group = 4 waves x 32 queries (two 16-query tiles per wave: every K and
// V fragment read from LDS feeds two MFMAs; 48 KB of LDS, and 194 registers per lane: two workgroups per CU). K/V blocks are register-staged and
// double-buffered: the loads of block i+1 are issued in front of the MFMAs of block i and written to the other buffer behind them, one
// barrier per block. A query row is computed by one wave from the same blocks in the same order whatever the grid is: the output bits
// depend on neither batch nor split.
#include "common.h"
#include <algorithm>

namespace yp {

typedef __attribute__((ext_vector_type(4))) short ss16x4;
typedef __attribute__((address_space(3))) ss16x4 s_lds_s4;

constexpr int AS_KB = 128;                       // keys per block: 8 KB of K rows + 16 KB of V rows, twice
constexpr int AS_NW = 4;                         // waves per workgroup
constexpr int AS_QW = 32;                        // queries per wave
constexpr int AS_GROUP = AS_NW * AS_QW;          // queries per group
constexpr int AS_KBYTES = AS_KB * 64, AS_VBYTES = AS_KB * 128;
constexpr float AS_MIN = -3.0e38f;               // "no key yet": finite, so that (m_old - m_new) is never inf - inf

template <bool WITH_V> struct AsStage {
    static constexpr int NW = AS_NW;
    static constexpr int NK = AS_KB * 4 / (NW * 64), NV = WITH_V ? AS_KB * 8 / (NW * 64) : 0;
    u32x4 k[NK];
    u32x4 v[NV > 0 ? NV : 1];
    // rows of block kb (keys >= N: an offset no buffer holds = zeros; never whatever lies behind the tensor)
    __device__ __forceinline__ void load(const __amdgpu_buffer_rsrc_t rs, const AttnParams& p, size_t base_el, int kb, int tid) {
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            const int ch = tid + i * NW * 64, row = ch >> 2, c = (ch & 3) ^ cswz64(row), key = kb * AS_KB + row;
            const unsigned off = key < p.N ? (unsigned)((base_el + (size_t)key * p.q_stride + 32 + c * 8) * 2) : kBufferOOB;
            k[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int ch = tid + i * NW * 64, row = ch >> 3, c = (ch & 7) ^ vswz(row), key = kb * AS_KB + row;
            const unsigned off = key < p.N ? (unsigned)((base_el + (size_t)key * p.q_stride + 64 + c * 8) * 2) : kBufferOOB;
            v[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
        }
    }
    __device__ __forceinline__ void write(unsigned char* Ks, unsigned char* Vs, int tid) const {
#pragma unroll
        for (int i = 0; i < NK; ++i) *(u32x4*)(Ks + (tid + i * NW * 64) * 16) = k[i];
#pragma unroll
        for (int i = 0; i < NV; ++i) *(u32x4*)(Vs + (tid + i * NW * 64) * 16) = v[i];
    }
};

__global__ __launch_bounds__(AS_NW * 64) void attention_stream_kernel(const AttnParams p, const int groups_per_wg, const unsigned qkv_bytes) {
    __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * (AS_KBYTES + AS_VBYTES)];
    constexpr int NW = AS_NW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, g = lane >> 4;
    const int bh = blockIdx.y, b = bh / p.nh, h = bh - b * p.nh;
    const size_t base_el = (size_t)b * p.N * p.q_stride + p.q_coff + h * 128;
    const __bf16* base = (const __bf16*)p.qkv + base_el;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.qkv, 0, (int)qkv_bytes, 0x00020000);
    const int nkb = (p.N + AS_KB - 1) / AS_KB;
    const int ngroups = (p.N + NW * AS_QW - 1) / (NW * AS_QW);
    const int g0 = blockIdx.x * groups_per_wg, g1 = min(g0 + groups_per_wg, ngroups);
    const float cexp = p.scale * 1.44269504088896341f;          // exp((s - m) * scale) = exp2((s - m) * scale * log2 e)

    // K fragment of key tile j: + j * 1024 (the chunk swizzle of a row depends on row & 15 only)
    const unsigned koff = fr * 64 + ((g ^ cswz64(fr)) * 16);
    // transposed-read addresses as in attention_mfma_kernel: lane 4q+pp of group g supplies key row 4g+q (+16: the second half of a
    // 32-key step), d columns dt*16 + 4pp .. +3
    unsigned voff[4];
    {
        const int q = (lane >> 2) & 3, pp = lane & 3, row = 4 * g + q;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) voff[dt] = row * 128 + (((2 * dt + (pp >> 1)) ^ vswz(row)) * 16) + 8 * (pp & 1);
    }

    for (int grp = g0; grp < g1; ++grp) {                       // (uniform: every wave meets every barrier, EXEC all ones at the tr reads)
        const int q0 = (grp * NW + wave) * AS_QW;
        bf16x8 qf[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)                              // query rows >= N: row N-1 again, never stored
            qf[t] = *(const bf16x8*)(base + (size_t)min(q0 + t * 16 + fr, p.N - 1) * p.q_stride + g * 8);

        // ---- pass 1: row max and sum ---------------------------------------------------------------------------------
        float m[2] = {AS_MIN, AS_MIN}, l[2] = {0.f, 0.f};
        {
            AsStage<false> sg;
            sg.load(rs, p, base_el, 0, tid);
            sg.write(lds, nullptr, tid);
            __syncthreads();
            for (int kb = 0; kb < nkb; ++kb) {
                const unsigned char* Ks = lds + (kb & 1) * AS_KBYTES;
                if (kb + 1 < nkb) sg.load(rs, p, base_el, kb + 1, tid);
                f32x4 st[2][AS_KB / 16];
                float bm[2] = {AS_MIN, AS_MIN};
#pragma unroll
                for (int j = 0; j < AS_KB / 16; ++j) {
                    const bf16x8 kf = *(const bf16x8*)(Ks + koff + j * 1024);
                    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        st[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[t], z, 0, 0, 0);
                        if ((kb + 1) * AS_KB > p.N) {            // (uniform) the last block may be ragged
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (kb * AS_KB + j * 16 + g * 4 + r >= p.N) st[t][j][r] = -INFINITY;
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) bm[t] = fmaxf(bm[t], st[t][j][r]);
                    }
                }
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const float mn = fmaxf(m[t], bm[t]);
                    float s = 0.f;
#pragma unroll
                    for (int j = 0; j < AS_KB / 16; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) s += __builtin_amdgcn_exp2f((st[t][j][r] - mn) * cexp);
                    l[t] = l[t] * __builtin_amdgcn_exp2f((m[t] - mn) * cexp) + s;
                    m[t] = mn;
                }
                if (kb + 1 < nkb) sg.write(lds + ((kb + 1) & 1) * AS_KBYTES, nullptr, tid);
                __syncthreads();
            }
        }
        float inv[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {                            // the four lane groups of a query row
            float mm = fmaxf(m[t], __shfl_xor(m[t], 16, 64));
            mm = fmaxf(mm, __shfl_xor(mm, 32, 64));
            float s = l[t] * __builtin_amdgcn_exp2f((m[t] - mm) * cexp);
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            m[t] = mm;
            inv[t] = 1.0f / s;
        }

        // ---- pass 2: O = P.V ---------------------------------------------------------------------------------------------
        f32x4 o[2][4];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        {
            AsStage<true> sg;
            unsigned char* const Kb = lds;
            unsigned char* const Vb = lds + 2 * AS_KBYTES;
            sg.load(rs, p, base_el, 0, tid);
            sg.write(Kb, Vb, tid);
            __syncthreads();
            for (int kb = 0; kb < nkb; ++kb) {
                const unsigned char* Ks = Kb + (kb & 1) * AS_KBYTES;
                const unsigned char* Vs = Vb + (kb & 1) * AS_VBYTES;
                if (kb + 1 < nkb) sg.load(rs, p, base_el, kb + 1, tid);
#pragma unroll
                for (int s = 0; s < AS_KB / 32; ++s) {           // steps of 32 keys
                    bf16x8 pf[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int j = 2 * s + u;
                        const bf16x8 kf = *(const bf16x8*)(Ks + koff + j * 1024);
                        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int t = 0; t < 2; ++t) {
                            f32x4 sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[t], z, 0, 0, 0);
                            if ((kb + 1) * AS_KB > p.N) {
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                    if (kb * AS_KB + j * 16 + g * 4 + r >= p.N) sc[r] = -INFINITY;
                            }
#pragma unroll
                            for (int r = 0; r < 4; ++r) pf[t][4 * u + r] = (__bf16)(__builtin_amdgcn_exp2f((sc[r] - m[t]) * cexp) * inv[t]);
                        }
                    }
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) {
                        const ss16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s_lds_s4*)(Vs + voff[dt] + s * 4096));
                        const ss16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s_lds_s4*)(Vs + voff[dt] + s * 4096 + 2048));
                        union { ss16x4 h[2]; bf16x8 v; } u;
                        u.h[0] = lo; u.h[1] = hi;
#pragma unroll
                        for (int t = 0; t < 2; ++t) o[t][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[t], u.v, o[t][dt], 0, 0, 0);
                    }
                }
                if (kb + 1 < nkb) sg.write(Kb + ((kb + 1) & 1) * AS_KBYTES, Vb + ((kb + 1) & 1) * AS_VBYTES, tid);
                __syncthreads();
            }
        }
        // D: col = d (lane & 15), rows = queries g*4 + r
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = q0 + t * 16 + g * 4 + r;
                if (q >= p.N) continue;
                __bf16* op = (__bf16*)p.o + ((size_t)b * p.N + q) * p.o_stride + p.o_coff + h * 64;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) op[dt * 16 + fr] = (__bf16)o[t][dt][r];
            }
    }
}

// What the streaming kernel takes: the resident form's conditions without its token bound.
bool attention_stream_scope(const AttnParams& p, int dtype) {
    const size_t qkv_bytes = (size_t)p.B * p.N * p.q_stride * 2;
    return dtype == DT_BF16 && p.kd == 32 && p.hd == 64 && p.N >= 1 && (p.q_stride & 7) == 0 && (p.q_coff & 7) == 0 && qkv_bytes < (1ull << 31);
}

// (workgroups per head, query groups each walks): runs as long as possible - every group streams all of K and V, a run only saves the
// launch of its workgroups - while the grid still reaches the workgroup target. tests/attention_stream_cases.py restates it.
void attention_stream_split(int B, int N, int nh, int wgs, int* nsplit_out, int* gpw_out) {
    static const int env_target = [] { const int v = env_int("YOLOP_ATTN_WGS", 0); return v > 0 ? v : 256; }();
    const int target = wgs > 0 ? wgs : env_target;
    const int BH = B * nh;
    const int ngroups = (N + AS_GROUP - 1) / AS_GROUP;
    int nsplit = std::min(ngroups, std::max(1, (target + BH - 1) / BH));
    const int gpw = (ngroups + nsplit - 1) / nsplit;
    nsplit = (ngroups + gpw - 1) / gpw;
    *nsplit_out = nsplit; *gpw_out = gpw;
}

hipError_t launch_attention_stream(const AttnParams& p, hipStream_t st, int wgs) {
    if (!attention_stream_scope(p, DT_BF16) || (p.o_stride & 3) || (p.o_coff & 3)) return hipErrorInvalidValue;
    const size_t qkv_bytes = (size_t)p.B * p.N * p.q_stride * 2;
    int nsplit, gpw;
    attention_stream_split(p.B, p.N, p.nh, wgs, &nsplit, &gpw);
    hipLaunchKernelGGL(attention_stream_kernel, dim3((unsigned)nsplit, (unsigned)(p.B * p.nh)), dim3(AS_NW * 64), 0, st, p, gpw, (unsigned)qkv_bytes);
    return hipGetLastError();
}

}  // namespace yp
