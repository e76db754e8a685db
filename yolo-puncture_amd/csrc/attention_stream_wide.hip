// PSA attention core, streaming matrix-core form for YOLOv10-M's heads (bf16, key_dim 36, head_dim 72, any N >= 1). The two-pass form
// of attention_stream.hip with its rounding points and its fragments (read that file's header first): pass 1 streams K and leaves per
// query row the max m and the sum l of exp2((s - m) c); pass 2 streams K and V, recomputes S, P = bf16(exp2((s - m) c) * (1/l)),
// O += P.V in fp32 in a fixed key order; the output is rounded once. There is no resident sibling: this kernel takes every N.
//
// What 36 / 72 change ("Streaming attention for 36/72 heads"):
//   key dim 36   S^T = K.Q^T takes one 16x16x32 step (dims 0..31) and one 16x16x16 step whose lane group 0 holds dims 32..35; the k-slots
//                of groups 1..3 are true zeros in BOTH operands: Q's are zero registers, K's are read from the 8 zero bytes that end
//                every K row in LDS (what follows K's 36 elements in memory is V, and 0 x NaN is NaN).
//   head dim 72  five 16-column output tiles, the last one half dead: columns 72..79 of the V image are zeros, feed only their own
//                output columns and are never stored.
//   global       a head block [q(36) | k(36) | v(72)] starts 16-byte aligned; K rows start at +72 B = 8-byte aligned only and are
//                fetched as nine 8-byte pieces (+ one piece at kBufferOOB = the zero pad), V rows at +144 B as nine 16-byte pieces
//                (+ one at kBufferOOB). Rows of keys >= N are fetched at kBufferOOB too; their scores are masked to -inf.
//   LDS          K rows of 80 B, V rows of 160 B (AW_KB = 128 keys: 2 x (10 + 20) KB = 60 KB, two workgroups per CU). Every
//                ds_read_b128 is 16-byte aligned, every ds_read_b64 / ds_read_b64_tr_b16 8-byte aligned. Banks (256-B bank row):
//                K: 80 r mod 256 is a bijection of the sixteen 16-B slots over r = 0..15, but a ds_read_b128 lane group mixes lane
//                   group g of rows {0-3, 12-15} with g ^ 1 of rows {4-11}: rows 4..11 keep their first four 16-B pieces in the order
//                   1 0 3 2 (kswz), so a hardware group reads one piece position of 16 different rows. The fifth piece (dims 32..35 |
//                   zeros) is read 8 bytes per lane: groups 0 / 1 take the two halves of 16 different slots, groups 2 / 3 broadcast.
//                V: a 32-lane half of a transposed read covers 8 rows x 32 B; 160 r mod 256 in units of 32 B is a bijection over
//                   r = 0..7 (and 16 rows are 10 bank rows): conflict-free without a swizzle.
//
// One workgroup = (image, head, a run of query groups); a query group = 4 waves x 32 queries, as in attention_stream_kernel, so the
// split is attention_stream_split. A query row is computed by one wave from the same blocks in the same order whatever the grid is.
#include "common.h"
#include <algorithm>

namespace yp {

typedef __attribute__((ext_vector_type(4))) short aw_s16x4;
typedef __attribute__((address_space(3))) aw_s16x4 aw_lds_s4;

constexpr int AW_KD = 36, AW_HD = 72, AW_BLK = 2 * AW_KD + AW_HD;
constexpr int AW_KB = 128;                       // keys per block
constexpr int AW_NW = 4;                         // waves per workgroup
constexpr int AW_QW = 32;                        // queries per wave
constexpr int AW_KROW = 80, AW_VROW = 160;       // LDS row strides in bytes
constexpr int AW_KBYTES = AW_KB * AW_KROW, AW_VBYTES = AW_KB * AW_VROW;
constexpr int AW_DT = 5;                         // output tiles of 16 columns (the last: 8 live)
constexpr float AW_MIN = -3.0e38f;               // "no key yet": finite, so that (m_old - m_new) is never inf - inf

// XOR mask on the index of the first four 16-B pieces of K row `row` (see the header)
__device__ __forceinline__ int kswz(int row) { return (((row & 15) + 4) >> 3) & 1; }

template <bool WITH_V> struct AwStage {
    static constexpr int NK = AW_KB * 10 / (AW_NW * 64), NV = WITH_V ? AW_KB * 10 / (AW_NW * 64) : 0;
    u32x2 k[NK];
    u32x4 v[NV > 0 ? NV : 1];
    // rows of block kb: thread piece ch fills LDS bytes [ch * 8, +8) of the K image and [ch * 16, +16) of the V image
    __device__ __forceinline__ void load(const __amdgpu_buffer_rsrc_t rs, const AttnParams& p, size_t base_el, int kb, int tid) {
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            const int ch = tid + i * AW_NW * 64, row = ch / 10, pos = ch - row * 10, key = kb * AW_KB + row;
            const int c = pos < 8 ? pos ^ (kswz(row) << 1) : pos;        // the 8-byte piece of the source row that lives at pos
            const unsigned off = (key < p.N && c < 9) ? (unsigned)((base_el + (size_t)key * p.q_stride + AW_KD + c * 4) * 2) : kBufferOOB;
            k[i] = __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int ch = tid + i * AW_NW * 64, row = ch / 10, c = ch - row * 10, key = kb * AW_KB + row;
            const unsigned off = (key < p.N && c < 9) ? (unsigned)((base_el + (size_t)key * p.q_stride + 2 * AW_KD + c * 8) * 2) : kBufferOOB;
            v[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
        }
    }
    __device__ __forceinline__ void write(unsigned char* Ks, unsigned char* Vs, int tid) const {
#pragma unroll
        for (int i = 0; i < NK; ++i) *(u32x2*)(Ks + (tid + i * AW_NW * 64) * 8) = k[i];
#pragma unroll
        for (int i = 0; i < NV; ++i) *(u32x4*)(Vs + (tid + i * AW_NW * 64) * 16) = v[i];
    }
};

// scores of one 16-key tile against one 16-query tile: dims 0..31, then 32..35
__device__ __forceinline__ f32x4 aw_scores(bf16x8 kf, aw_s16x4 kt, bf16x8 qf, aw_s16x4 qt) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    const f32x4 s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, z, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(kt, qt, s, 0, 0, 0);
}

__global__ __launch_bounds__(AW_NW * 64) void attention_stream_wide_kernel(const AttnParams p, const int groups_per_wg, const unsigned qkv_bytes) {
    __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * (AW_KBYTES + AW_VBYTES)];
    constexpr int NW = AW_NW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, g = lane >> 4;
    const int bh = blockIdx.y, b = bh / p.nh, h = bh - b * p.nh;
    const size_t base_el = (size_t)b * p.N * p.q_stride + p.q_coff + h * AW_BLK;
    const __bf16* base = (const __bf16*)p.qkv + base_el;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.qkv, 0, (int)qkv_bytes, 0x00020000);
    const int nkb = (p.N + AW_KB - 1) / AW_KB;
    const int ngroups = (p.N + NW * AW_QW - 1) / (NW * AW_QW);
    const int g0 = blockIdx.x * groups_per_wg, g1 = min(g0 + groups_per_wg, ngroups);
    const float cexp = p.scale * 1.44269504088896341f;          // exp((s - m) * scale) = exp2((s - m) * scale * log2 e)

    // K fragments of key tile j: + j * 16 * AW_KROW. Dims 0..31: piece g of row fr; dims 32..35: the row's bytes 64..71 for lane group 0,
    // its zero bytes 72..79 for the others
    const unsigned koff = fr * AW_KROW + ((g ^ kswz(fr)) * 16);
    const unsigned ktoff = fr * AW_KROW + (g == 0 ? 64 : 72);
    // transposed-read addresses: lane 4q+pp of group g supplies key row 4g+q (+16: the second half of a 32-key step), d columns
    // dt*16 + 4pp .. +3
    const unsigned voff = (4 * g + ((lane >> 2) & 3)) * AW_VROW + (lane & 3) * 8;

    for (int grp = g0; grp < g1; ++grp) {                       // (uniform: every wave meets every barrier, EXEC all ones at the tr reads)
        const int q0 = (grp * NW + wave) * AW_QW;
        bf16x8 qf[2];
        aw_s16x4 qt[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {                            // query rows >= N: row N-1 again, never stored
            const __bf16* qp = base + (size_t)min(q0 + t * 16 + fr, p.N - 1) * p.q_stride;
            qf[t] = *(const bf16x8*)(qp + g * 8);
            qt[t] = aw_s16x4{0, 0, 0, 0};
            if (g == 0) qt[t] = *(const aw_s16x4*)(qp + 32);
        }

        // ---- pass 1: row max and sum ---------------------------------------------------------------------------------
        float m[2] = {AW_MIN, AW_MIN}, l[2] = {0.f, 0.f};
        {
            AwStage<false> sg;
            sg.load(rs, p, base_el, 0, tid);
            sg.write(lds, nullptr, tid);
            __syncthreads();
            for (int kb = 0; kb < nkb; ++kb) {
                const unsigned char* Ks = lds + (kb & 1) * AW_KBYTES;
                if (kb + 1 < nkb) sg.load(rs, p, base_el, kb + 1, tid);
                f32x4 st[2][AW_KB / 16];
                float bm[2] = {AW_MIN, AW_MIN};
#pragma unroll
                for (int j = 0; j < AW_KB / 16; ++j) {
                    const bf16x8 kf = *(const bf16x8*)(Ks + koff + j * 16 * AW_KROW);
                    const aw_s16x4 kt = *(const aw_s16x4*)(Ks + ktoff + j * 16 * AW_KROW);
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        st[t][j] = aw_scores(kf, kt, qf[t], qt[t]);
                        if ((kb + 1) * AW_KB > p.N) {            // (uniform) the last block may be ragged
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (kb * AW_KB + j * 16 + g * 4 + r >= p.N) st[t][j][r] = -INFINITY;
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
                    for (int j = 0; j < AW_KB / 16; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) s += __builtin_amdgcn_exp2f((st[t][j][r] - mn) * cexp);
                    l[t] = l[t] * __builtin_amdgcn_exp2f((m[t] - mn) * cexp) + s;
                    m[t] = mn;
                }
                if (kb + 1 < nkb) sg.write(lds + ((kb + 1) & 1) * AW_KBYTES, nullptr, tid);
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
        f32x4 o[2][AW_DT];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int dt = 0; dt < AW_DT; ++dt) o[t][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        {
            AwStage<true> sg;
            unsigned char* const Kb = lds;
            unsigned char* const Vb = lds + 2 * AW_KBYTES;
            sg.load(rs, p, base_el, 0, tid);
            sg.write(Kb, Vb, tid);
            __syncthreads();
            for (int kb = 0; kb < nkb; ++kb) {
                const unsigned char* Ks = Kb + (kb & 1) * AW_KBYTES;
                const unsigned char* Vs = Vb + (kb & 1) * AW_VBYTES;
                if (kb + 1 < nkb) sg.load(rs, p, base_el, kb + 1, tid);
#pragma unroll
                for (int s = 0; s < AW_KB / 32; ++s) {           // steps of 32 keys
                    bf16x8 pf[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int j = 2 * s + u;
                        const bf16x8 kf = *(const bf16x8*)(Ks + koff + j * 16 * AW_KROW);
                        const aw_s16x4 kt = *(const aw_s16x4*)(Ks + ktoff + j * 16 * AW_KROW);
#pragma unroll
                        for (int t = 0; t < 2; ++t) {
                            f32x4 sc = aw_scores(kf, kt, qf[t], qt[t]);
                            if ((kb + 1) * AW_KB > p.N) {
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                    if (kb * AW_KB + j * 16 + g * 4 + r >= p.N) sc[r] = -INFINITY;
                            }
#pragma unroll
                            for (int r = 0; r < 4; ++r) pf[t][4 * u + r] = (__bf16)(__builtin_amdgcn_exp2f((sc[r] - m[t]) * cexp) * inv[t]);
                        }
                    }
#pragma unroll
                    for (int dt = 0; dt < AW_DT; ++dt) {
                        const aw_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((aw_lds_s4*)(Vs + voff + dt * 32 + s * 32 * AW_VROW));
                        const aw_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((aw_lds_s4*)(Vs + voff + dt * 32 + s * 32 * AW_VROW + 16 * AW_VROW));
                        union { aw_s16x4 h[2]; bf16x8 v; } u;
                        u.h[0] = lo; u.h[1] = hi;
#pragma unroll
                        for (int t = 0; t < 2; ++t) o[t][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[t], u.v, o[t][dt], 0, 0, 0);
                    }
                }
                if (kb + 1 < nkb) sg.write(Kb + ((kb + 1) & 1) * AW_KBYTES, Vb + ((kb + 1) & 1) * AW_VBYTES, tid);
                __syncthreads();
            }
        }
        // D: col = d (lane & 15), rows = queries g*4 + r; of the fifth tile only columns 64..71 exist
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = q0 + t * 16 + g * 4 + r;
                if (q >= p.N) continue;
                __bf16* op = (__bf16*)p.o + ((size_t)b * p.N + q) * p.o_stride + p.o_coff + h * AW_HD;
#pragma unroll
                for (int dt = 0; dt < AW_DT; ++dt)
                    if (dt * 16 + fr < AW_HD) op[dt * 16 + fr] = (__bf16)o[t][dt][r];
            }
    }
}

// What the wide-head streaming kernel takes: any token count, the strides of the 16-byte Q and V fragments.
bool attention_stream_wide_scope(const AttnParams& p, int dtype) {
    const size_t qkv_bytes = (size_t)p.B * p.N * p.q_stride * 2;
    return dtype == DT_BF16 && p.kd == AW_KD && p.hd == AW_HD && p.N >= 1 && (p.q_stride & 7) == 0 && (p.q_coff & 7) == 0 && qkv_bytes < (1ull << 31);
}

hipError_t launch_attention_stream_wide(const AttnParams& p, hipStream_t st, int wgs) {
    if (!attention_stream_wide_scope(p, DT_BF16) || (p.o_stride & 3) || (p.o_coff & 3)) return hipErrorInvalidValue;
    const size_t qkv_bytes = (size_t)p.B * p.N * p.q_stride * 2;
    int nsplit, gpw;
    attention_stream_split(p.B, p.N, p.nh, wgs, &nsplit, &gpw);          // the query group is attention_stream_kernel's: 4 waves x 32 queries
    hipLaunchKernelGGL(attention_stream_wide_kernel, dim3((unsigned)nsplit, (unsigned)(p.B * p.nh)), dim3(AW_NW * 64), 0, st, p, gpw, (unsigned)qkv_bytes);
    return hipGetLastError();
}

}  // namespace yp
