// PSA attention core, streaming matrix-core form in fp32 for YOLOv10-M's heads (key_dim 36, head_dim 72, any N >= 1): the strict-parity M
// engine's kernel past the generic kernel's 2364 tokens, and from 401 tokens on where an engine asked for it (yp_set_attention_f32_stream,
// value 3). It is attention_stream_f32.hip's kernel - two passes, both products on v_mfma_f32_16x16x4_f32 (an exact fp32 FMA chain: no
// rounding point is added to the fp32 contract, only the order of the sums is the kernel's own), keys in blocks of AW_KB through a
// register-staged, double-buffered LDS image, one barrier per block, P.V of a block in a fresh accumulator - with what 36/72 change
// (tests/attention_f32_wide_cases.py restates the order on the CPU):
//
//   key dim 36   nine k-steps of four, no padding. In fp32 a head block is 576 bytes, K starts at +144 and V at +288: all 16-byte aligned,
//                so a K row is nine 16-byte loads. Lane group g holds d = 8g .. 8g+7 (two 16-byte LDS reads) and d = 32 + g (one 4-byte
//                read) of its K row and of its query; step s < 8 takes d = 8g + s, step 8 takes d = 32 + g. Steps 2c, 2c+1 form chain c
//                of four and step 8 a fifth chain: ((c0 + c1) + (c2 + c3)) + c4. The scale multiplies the finished sum.
//   head dim 72  five 16-column output tiles. Column c of tiles 0..3 means d = 4c + dt (one 16-byte LDS read of the row-major V image
//                feeds the four, and a lane stores 16 bytes of four consecutive d); column c of tile 4 means d = 64 + c, alive for c < 8.
//                Columns 72..79 of the V image are true zeros - staged from an offset no buffer holds, never what follows the row in
//                memory (0 x NaN = NaN) -, feed only their own dead output columns and are never stored.
//
// LDS (bank of byte a = (a / 4) mod 64 for 16-byte reads, mod 32 for 4-byte reads; a 16-byte read is served in the hardware lane groups
// {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... = rows {0-3,12-15} of lane group g with rows {4-11} of lane group g^1, a 4-byte read in halves
// of 32 lanes):
//   K rows of 144 bytes = nine 16-byte pieces. 9 r mod 16 is a bijection of the sixteen 16-byte slots of a 256-byte bank row over 16
//                consecutive rows, so sixteen lanes that read ONE piece position of 16 different rows do not collide. Rows 4..11 (mod 16)
//                keep pieces 0..7 at position c ^ 2: lane group g^1 of those rows then reads the position lane group g reads in the others.
//                Piece 8, read 4 bytes per lane: dword 36 r + 32 + g lies in bank (4 r + g) mod 32, rows r and r + 8 collide; rows 8..15
//                keep the four dwords of piece 8 in the order 2 3 0 1, so that in a half (g in {0, 1} or {2, 3}) row r takes dwords
//                {g} and row r + 8 dwords {g ^ 2} of the same four banks.
//   V rows of 384 bytes. 16 bytes per lane: lane (c, g) reads piece c of row 4g + r; four rows are 96 pieces = 0 mod 16, so a hardware
//                group reads pieces {0-3,12-15} of one row and {4-11} of another at the same bank-row phase: 16 different slots. 4 bytes
//                per lane (tile 4): dword 96 row + 64 + c, and 96 row = 0 mod 32: lane groups g and g + 1 of a half would meet in banks
//                0..15. Rows of odd lane groups ((row >> 2) & 1) keep d = 64..79 at dwords 80..95, banks 16..31. (288- and 320-byte rows
//                do not work: four rows of 288 are 8 mod 16 pieces, the two row sets of a hardware group overlap; 320 has no room for
//                the second position of d = 64..79.)
// 2 x (9 + 24) KB = 66 KB: two workgroups per CU.
//
// One workgroup = (image, head, a run of query groups); a query group = 4 waves x 16 queries; the split rule is the fp32 32/64 kernel's.
// Keys >= N are fetched as zeros and their scores masked to -inf before the max; query rows >= N read row N-1 again and are not stored.
// A query row is computed by one wave from the same blocks in the same order whatever the grid is: the output bits depend on neither
// batch nor split. No atomics.
#include "common.h"
#include <algorithm>

namespace yp {

constexpr int AW_KB = 64;                        // keys per block
constexpr int AW_NW = 4;                         // waves per workgroup
constexpr int AW_QW = 16;                        // queries per wave
constexpr int AW_GROUP = AW_NW * AW_QW;          // queries per group
constexpr int AW_KD = 36, AW_HD = 72, AW_HEAD = 2 * AW_KD + AW_HD;
constexpr int AW_KPITCH = 144, AW_VPITCH = 384;  // LDS row pitches, bytes
constexpr int AW_KCH = 9, AW_VCH = 20;           // staged 16-byte pieces per row: V's 18 and two of zeros (d = 72..79)
constexpr int AW_KBYTES = AW_KB * AW_KPITCH, AW_VBYTES = AW_KB * AW_VPITCH;
constexpr float AW_LOG2E = 1.44269504088896341f;
constexpr float AW_MIN = -3.0e38f;               // "no key yet": finite, so that (m_old - m_new) is never inf - inf
static_assert(2 * (AW_KBYTES + AW_VBYTES) <= 80 * 1024, "two workgroups per CU");

template <bool WITH_V> struct AwStage {
    static constexpr int NT = AW_NW * 64;
    static constexpr int NK = (AW_KB * AW_KCH + NT - 1) / NT, NV = WITH_V ? AW_KB * AW_VCH / NT : 0;
    static_assert(AW_KB * AW_VCH % NT == 0, "V pieces divide among the threads");
    u32x4 k[NK];
    u32x4 v[NV > 0 ? NV : 1];
    // rows of block kb (keys >= N, V's zero pieces and the K pieces past the block: an offset no buffer holds = zeros)
    __device__ __forceinline__ void load(const __amdgpu_buffer_rsrc_t rs, const AttnParams& p, size_t base_el, int kb, int tid) {
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            const int ch = tid + i * NT, row = ch / AW_KCH, c = ch - row * AW_KCH, key = kb * AW_KB + row;
            const unsigned off = (row < AW_KB && key < p.N) ? (unsigned)((base_el + (size_t)key * p.q_stride + AW_KD + c * 4) * 4) : kBufferOOB;
            k[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int ch = tid + i * NT, row = ch / AW_VCH, c = ch - row * AW_VCH, key = kb * AW_KB + row;
            const unsigned off = (c < AW_HD / 4 && key < p.N) ? (unsigned)((base_el + (size_t)key * p.q_stride + 2 * AW_KD + c * 4) * 4) : kBufferOOB;
            v[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
        }
    }
    // the LDS image (file comment): K pieces 0..7 of rows 4..11 (mod 16) at c ^ 2, the dwords of piece 8 of rows 8..15 as 2 3 0 1;
    // V pieces 16..19 of the rows of odd lane groups four pieces further
    __device__ __forceinline__ void write(unsigned char* Ks, unsigned char* Vs, int tid) const {
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            const int ch = tid + i * NT, row = ch / AW_KCH, c = ch - row * AW_KCH;
            if (row >= AW_KB) continue;
            const int pos = c < 8 ? c ^ ((((row + 12) & 15) < 8) ? 2 : 0) : c;
            const bool swap = c == 8 && (row & 8);
            const u32x4 x = k[i];
            *(u32x4*)(Ks + row * AW_KPITCH + pos * 16) = swap ? u32x4{x[2], x[3], x[0], x[1]} : x;
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int ch = tid + i * NT, row = ch / AW_VCH, c = ch - row * AW_VCH;
            const int pos = c < 16 ? c : c + 4 * ((row >> 2) & 1);
            *(u32x4*)(Vs + row * AW_VPITCH + pos * 16) = v[i];
        }
    }
};

// exp(x) as the matrix-core kernels take it: one multiplication and v_exp_f32
__device__ __forceinline__ float aw_exp(float x) { return __builtin_amdgcn_exp2f(x * AW_LOG2E); }

// scaled scores of key tile j against the wave's query tile: sc[reg] = (q[lane & 15] . k[16 j + 4 g + reg]) * scale, keys >= N at -inf
// (ragged: the block reaches past N, uniform)
__device__ __forceinline__ void aw_scores(const unsigned char* Ks, unsigned koff0, unsigned koff1, unsigned koff8, int j, const float (&qf)[9], float scale,
                                          bool ragged, int key0, int N, f32x4& sc) {
    const f32x4 k0 = *(const f32x4*)(Ks + koff0 + j * (16 * AW_KPITCH)), k1 = *(const f32x4*)(Ks + koff1 + j * (16 * AW_KPITCH));
    const float k8 = *(const float*)(Ks + koff8 + j * (16 * AW_KPITCH));
    const float kf[8] = {k0[0], k0[1], k0[2], k0[3], k1[0], k1[1], k1[2], k1[3]};
    // four chains of 8 key dimensions and one of 4, independent accumulators (they also hide the MFMA's dependent latency)
    f32x4 part[5];
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        part[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[2 * c], qf[2 * c], z, 0, 0, 0);
        part[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[2 * c + 1], qf[2 * c + 1], part[c], 0, 0, 0);
    }
    part[4] = __builtin_amdgcn_mfma_f32_16x16x4f32(k8, qf[8], z, 0, 0, 0);
    f32x4 acc = ((part[0] + part[1]) + (part[2] + part[3])) + part[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] *= scale;
    if (ragged) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (key0 + j * 16 + r >= N) acc[r] = -INFINITY;
    }
    sc = acc;
}

__global__ __launch_bounds__(AW_NW * 64, 2) void attention_stream_wide_f32_kernel(const AttnParams p, const int groups_per_wg, const unsigned qkv_bytes) {
    __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * (AW_KBYTES + AW_VBYTES)];
    constexpr int NW = AW_NW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, g = lane >> 4;
    const int bh = blockIdx.y, b = bh / p.nh, h = bh - b * p.nh;
    const size_t base_el = (size_t)b * p.N * p.q_stride + p.q_coff + h * AW_HEAD;
    const float* base = (const float*)p.qkv + base_el;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.qkv, 0, (int)qkv_bytes, 0x00020000);
    const int nkb = (p.N + AW_KB - 1) / AW_KB;
    const int ngroups = (p.N + AW_GROUP - 1) / AW_GROUP;
    const int g0 = blockIdx.x * groups_per_wg, g1 = min(g0 + groups_per_wg, ngroups);

    // K fragment of key tile j (+ j * 16 rows; the image of a row depends on row & 15 only): pieces 2g and 2g + 1 and dword g of piece 8
    const int kx = (((fr + 12) & 15) < 8) ? 2 : 0;
    const unsigned koff0 = fr * AW_KPITCH + (((2 * g) ^ kx) * 16), koff1 = fr * AW_KPITCH + (((2 * g + 1) ^ kx) * 16);
    const unsigned koff8 = fr * AW_KPITCH + 128 + ((g ^ ((fr & 8) ? 2 : 0)) * 4);
    // V fragment of key tile j, step r: + j * 16 rows + r rows; row 4g (+ r): d = 4 fr .. 4 fr + 3, and d = 64 + fr
    const unsigned voff = g * 4 * AW_VPITCH + fr * 16;
    const unsigned voff4 = g * 4 * AW_VPITCH + (64 + 16 * (g & 1) + fr) * 4;

    for (int grp = g0; grp < g1; ++grp) {                       // (uniform: every wave meets every barrier)
        const int q0 = (grp * NW + wave) * AW_QW;
        float qf[9];
        {                                                            // query rows >= N: row N-1 again, never stored
            const float* qp = base + (size_t)min(q0 + fr, p.N - 1) * p.q_stride;
            const f32x4 a = *(const f32x4*)(qp + g * 8), c = *(const f32x4*)(qp + g * 8 + 4);
#pragma unroll
            for (int s = 0; s < 4; ++s) { qf[s] = a[s]; qf[4 + s] = c[s]; }
            qf[8] = qp[32 + g];
        }

        // ---- pass 1: row max and sum ---------------------------------------------------------------------------------
        float m = AW_MIN, l = 0.f;
        {
            AwStage<false> sg;
            sg.load(rs, p, base_el, 0, tid);
            sg.write(lds, nullptr, tid);
            __syncthreads();
            for (int kb = 0; kb < nkb; ++kb) {
                const unsigned char* Ks = lds + (kb & 1) * AW_KBYTES;
                if (kb + 1 < nkb) sg.load(rs, p, base_el, kb + 1, tid);
                const bool ragged = (kb + 1) * AW_KB > p.N;
                f32x4 st[AW_KB / 16];
                float bm = AW_MIN;
#pragma unroll
                for (int j = 0; j < AW_KB / 16; ++j) {
                    aw_scores(Ks, koff0, koff1, koff8, j, qf, p.scale, ragged, kb * AW_KB + g * 4, p.N, st[j]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) bm = fmaxf(bm, st[j][r]);
                }
                const float mn = fmaxf(m, bm);
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < AW_KB / 16; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s += aw_exp(st[j][r] - mn);
                l = l * aw_exp(m - mn) + s;
                m = mn;
                if (kb + 1 < nkb) sg.write(lds + ((kb + 1) & 1) * AW_KBYTES, nullptr, tid);
                __syncthreads();
            }
        }
        float inv;
        {                                                            // the four lane groups of a query row
            float mm = fmaxf(m, __shfl_xor(m, 16, 64));
            mm = fmaxf(mm, __shfl_xor(mm, 32, 64));
            float s = l * aw_exp(m - mm);
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            m = mm;
            inv = 1.0f / s;
        }

        // ---- pass 2: O = P.V ---------------------------------------------------------------------------------------------
        f32x4 o[5];
#pragma unroll
        for (int dt = 0; dt < 5; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
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
                const bool ragged = (kb + 1) * AW_KB > p.N;
                f32x4 ob[5];                                         // this block's share: a fresh accumulator
#pragma unroll
                for (int dt = 0; dt < 5; ++dt) ob[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < AW_KB / 16; ++j) {
                    f32x4 sc;
                    aw_scores(Ks, koff0, koff1, koff8, j, qf, p.scale, ragged, kb * AW_KB + g * 4, p.N, sc);
#pragma unroll
                    for (int r = 0; r < 4; ++r) sc[r] = aw_exp(sc[r] - m) * inv;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const f32x4 vf = *(const f32x4*)(Vs + voff + (j * 16 + r) * AW_VPITCH);
                        const float v4 = *(const float*)(Vs + voff4 + (j * 16 + r) * AW_VPITCH);
#pragma unroll
                        for (int dt = 0; dt < 4; ++dt) ob[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(sc[r], vf[dt], ob[dt], 0, 0, 0);
                        ob[4] = __builtin_amdgcn_mfma_f32_16x16x4f32(sc[r], v4, ob[4], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int dt = 0; dt < 5; ++dt) o[dt] += ob[dt];
                if (kb + 1 < nkb) sg.write(Kb + ((kb + 1) & 1) * AW_KBYTES, Vb + ((kb + 1) & 1) * AW_VBYTES, tid);
                __syncthreads();
            }
        }
        // D: rows = queries g*4 + r; col (lane & 15) = d 4 fr + dt of tiles 0..3 (four consecutive d per lane and row), d = 64 + fr of
        // tile 4, whose columns 8..15 are dead
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = q0 + g * 4 + r;
            if (q >= p.N) continue;
            float* op = (float*)p.o + ((size_t)b * p.N + q) * p.o_stride + p.o_coff + h * AW_HD;
            *(f32x4*)(op + fr * 4) = f32x4{o[0][r], o[1][r], o[2][r], o[3][r]};
            if (fr < 8) op[64 + fr] = o[4][r];
        }
    }
}

// What the kernel takes: fp32, 36-wide keys and 72-wide heads, 16-byte fragments on both slices, 32-bit byte offsets into qkv.
bool attention_stream_wide_f32_scope(const AttnParams& p, int dtype) {
    const size_t qkv_bytes = (size_t)p.B * p.N * p.q_stride * 4;
    return dtype == DT_F32 && p.kd == AW_KD && p.hd == AW_HD && p.N >= 1 && ((p.q_stride | p.q_coff | p.o_stride | p.o_coff) & 3) == 0 && qkv_bytes < (1ull << 31);
}

// (workgroups per head, query groups each walks): attention_stream_f32_split's rule - runs as long as possible while the grid still
// reaches the workgroup target (wgs, else YOLOP_ATTN_WGS, else 1024). tests/attention_f32_wide_cases.py restates it.
static void attention_stream_wide_f32_split(int B, int N, int nh, int wgs, int* nsplit_out, int* gpw_out) {
    static const int env_target = [] { const int v = env_int("YOLOP_ATTN_WGS", 0); return v > 0 ? v : 1024; }();
    const int target = wgs > 0 ? wgs : env_target;
    const int BH = B * nh;
    const int ngroups = (N + AW_GROUP - 1) / AW_GROUP;
    int nsplit = std::min(ngroups, std::max(1, (target + BH - 1) / BH));
    const int gpw = (ngroups + nsplit - 1) / nsplit;
    nsplit = (ngroups + gpw - 1) / gpw;
    *nsplit_out = nsplit; *gpw_out = gpw;
}

hipError_t launch_attention_stream_wide_f32(const AttnParams& p, hipStream_t st, int wgs) {
    if (!attention_stream_wide_f32_scope(p, DT_F32)) return hipErrorInvalidValue;
    const size_t qkv_bytes = (size_t)p.B * p.N * p.q_stride * 4;
    int nsplit, gpw;
    attention_stream_wide_f32_split(p.B, p.N, p.nh, wgs, &nsplit, &gpw);
    hipLaunchKernelGGL(attention_stream_wide_f32_kernel, dim3((unsigned)nsplit, (unsigned)(p.B * p.nh)), dim3(AW_NW * 64), 0, st, p, gpw, (unsigned)qkv_bytes);
    return hipGetLastError();
}

}  // namespace yp
