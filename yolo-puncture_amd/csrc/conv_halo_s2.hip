// Stride-2 member of the halo family (see conv_halo_p.hip): 3x3, stride 2, pad 1, bf16, persistent, weights resident in LDS or, for
// Cin = 32 / 64 under ids 500 / 501, in registers.
//
// The im2col form of a stride-2 3x3 re-reads every input pixel 2.25 times through the 1-KiB LDS-DMA pieces and streams
// it a k-step at a time (model.1 / model.3 / model.17: 100 / 80 / 35 us at 3.1 / 2.0 / 1.9 TB/s). Here the input patch of
// an output tile - (2*TH+1) rows x 33 columns per 32-channel chunk - is staged ONCE. A lane of the MFMA B operand reads its
// own pixel, so the stride-2 gather is free in principle; what has to be arranged is the bank pattern: 16 lanes reading
// every second pixel of a row hit 2 of the 16-byte slots. The LDS image therefore stores the EVEN and the ODD input columns
// of a row as two planes (17 + 16 pixels): tap kx = 0 reads plane E at n, kx = 1 plane O at n, kx = 2 plane E at n+1 -
// always 16 consecutive LDS rows, conflict-free under the usual chunk swizzle. The LDS-DMA fill computes the source pixel of
// every LDS row from that layout (the destination of a piece is lane-linear, the source address is per lane).
// Rows: input row jr = 2r + ky serves output row r; an even input row feeds (r = jr/2, ky = 0) and (r = jr/2 - 1, ky = 2),
// an odd one (r = (jr-1)/2, ky = 1), so each fragment read still feeds up to 2*FN MFMAs.
// vmcnt accounting, persistence, epilogue: identical to conv_halo_p.hip.
//
// Register-weights forms (a ninth template argument = the number of 32-channel chunks). With the weights in LDS a wave reads 3 * FN
// weight fragments and 2 * FM + 1 pixel fragments per kx for 3 * FM * FN MFMAs: two thirds of the LDS read bytes of <1,2,4,2> are
// weights that are the same for every tile a workgroup walks. These forms stage the workgroup's slab once, a chunk at a time, through
// the (still unused) halo ring and keep each wave's 9 * chunks * FN fragments in registers (at most 144 VGPRs; one workgroup per CU =
// two waves per SIMD, as conv_wreg.hip). LDS then holds the ring alone, which admits tiles the weights excluded: 8 rows x 64 channels
// for Cin = 64, and 4 rows x 128 channels (<2,2,2,4>) - one channel block for a 128-wide layer, so every input tile is fetched by one
// workgroup instead of two. They are no configuration ids: a launch of id 500 / 501 with Cin = 32 / 64 takes them (halo_s2_form;
// YOLOP_S2_LDS_WEIGHTS=1 keeps the LDS forms). model.3 of v10-S under id 501: 60 us (LDS) -> 52-54 (<1,2,4,2>, registers) -> 46.5
// (<2,2,2,4>, what it launches now). The k order of every output element (chunk, kx, ky) is that of the LDS forms: the results are
// bit-identical (tests/test_gpu_halo_s2_wreg.py).
#include "common.h"

namespace yp {

constexpr int kS2WregMaxVgprs = 144;      // weight registers of a wave in a register-weights form (two waves per SIMD, 256 VGPRs each)

// The kernel body of both forms. NCH = 0: weights resident in LDS, the chunk count is p.Cin / 32; NCH > 0: register weights for NCH chunks.
template <int FM, int FN, int WGM, int WGN, int NSH, bool HAS_RES, bool OUT_F32, bool PW2, int NCH>
__device__ __forceinline__ void conv_halo_s2_body(const ConvParams& p, const int tiles_h, const int tiles_w, const int ntiles, const int G) {
    constexpr int NW = WGM * WGN;
    constexpr int TH = WGM * FM, BN = WGN * FN * 16;
    constexpr int HR = 2 * TH + 1;                     // input rows of the patch
    constexpr int HP = HR * 33;                        // LDS rows (pixels) per slot: [jr][E0..E16 | O0..O15]
    constexpr int H_INSTR = (HP * 4 + 63) / 64;
    constexpr int LH = (H_INSTR + NW - 1) / NW;
    constexpr int HB = H_INSTR * 1024;
    constexpr int S = FM * FN;                        // stores per wave per tile
    constexpr bool WREG = NCH > 0;                    // (the chunk count is then a constant: the register array is indexed by it)
    static_assert(!WREG || (!PW2 && 9 * NCH * FN * 4 <= kS2WregMaxVgprs), "register-weights form");
    static_assert(NSH == 3, "wait selection below is written for a 3-slot ring");
    static_assert((NSH - 2) * LH + 2 * S < 64, "vmcnt immediate");

    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    unsigned char* const Hs = smem;                   // NSH halo slots
    unsigned char* const dump = smem + NSH * HB;      // 1 KiB landing zone of padding loads
    unsigned char* const Wres = dump + 1024;          // resident weights: [(chunk*9 + tap)][BN][32] bf16 (not WREG)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WGM, wn = wave / WGM;
    const int fr = lane & 15, fc = lane >> 4;
    const int nchunk = WREG ? NCH : p.Cin >> 5;

    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int nt = bid % ntiles, j0 = bid / ntiles;
    const int n0 = nt * BN;
    const int B = p.M / (p.Ho * p.Wo);
    const int num_tiles = B * tiles_h * tiles_w;

    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (int)p.w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc((void*)p.y, 0, (int)p.y_bytes, 0x00020000);

    // bias first: its loads retire under the one-time vmcnt(0) below, so no compiler wait lands inside the tile loop
    float bias[FN][4];
#pragma unroll
    for (int a = 0; a < FN; ++a) {
        const int co = n0 + wn * (FN * 16) + a * 16 + fc * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) bias[a][r] = (co + r < p.Cout) ? p.bias[co + r] : 0.f;
    }

    // ---- resident weights: one pass of LDS-DMA pieces, row rg = (chunk*9 + tap)*BN + n -----------------------------
    if constexpr (!WREG) {
        const int rows = 9 * nchunk * BN;
        const int ninstr = rows >> 4;
        for (int ii = wave; ii < ninstr; ii += NW) {
            const int s = ii * 64 + lane;
            const int rg = s >> 2, pc = s & 3;
            const int c8 = pc ^ cswz64(rg);
            const int n = rg % BN, q = rg / BN;
            const int tap = q % 9, ch = q / 9;
            const unsigned voff = (unsigned)(((n0 + n) * p.Kpad + tap * p.Cin + ch * 32 + c8 * 8) * 2);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (lds_void*)(Wres + ii * 1024), 16, voff, 0, 0, 0);
        }
    }
    // ---- register weights: the slab goes through the halo ring a chunk at a time (rows tap*BN + n, the same pieces and swizzle), every
    //      wave then reads its own 9 * FN fragments (the launcher allots a chunk's bytes where the ring is smaller). Filled once per workgroup, before the first halo piece is issued; known complete
    //      (lgkmcnt(0)) and passed through empty asm statements, so that no wait for them lands in the tile loop ----
    bf16x8 wr[WREG ? NCH : 1][9][FN];
    if constexpr (WREG) {
        constexpr int W_INSTR = 9 * BN / 16;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            for (int ii = wave; ii < W_INSTR; ii += NW) {
                const int s = ii * 64 + lane;
                const int rg = s >> 2, pc = s & 3;
                const int c8 = pc ^ cswz64(rg);
                const int tap = rg / BN, n = rg - tap * BN;
                const unsigned voff = (unsigned)(((n0 + n) * p.Kpad + tap * p.Cin + c * 32 + c8 * 8) * 2);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (lds_void*)(Hs + ii * 1024), 16, voff, 0, 0, 0);
            }
            wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int a = 0; a < FN; ++a) {
                    const int rw = t * BN + wn * (FN * 16) + a * 16 + fr;
                    wr[c][t][a] = *(const bf16x8*)(Hs + swz64((unsigned)(rw * 64 + fc * 16)));
                }
            __builtin_amdgcn_s_waitcnt(0xc07f);               // lgkmcnt(0): the fragments are in registers before the image is overwritten
            __builtin_amdgcn_s_barrier();                     // (by the next chunk, or by the first halo pieces below)
        }
#pragma unroll
        for (int c = 0; c < NCH; ++c)
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int a = 0; a < FN; ++a) asm volatile("" : "+v"(wr[c][t][a]));
    }

    // ---- PW2: the trailing 1x1's weights [C2 = BN][BN] (128-B rows, 8-slot swizzle) stay in LDS behind the 3x3 weights ------
    unsigned char* const W2s = Wres + (size_t)9 * nchunk * BN * 64;
    float bias2[FN][4];
    if (PW2) {
        static_assert(!PW2 || BN == 64, "the fused trailing 1x1 is written for a 64-wide intermediate and output");
        const __amdgpu_buffer_rsrc_t w2rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.w2, 0, (int)p.w2_bytes, 0x00020000);
        for (int ii = wave; ii < BN * 8 / 64; ii += NW) {          // BN rows x 8 chunks of 16 B
            const int s = ii * 64 + lane;
            const int row = s >> 3, pc = s & 7;
            const int c8 = pc ^ ((row >> 1) & 7);
            const unsigned voff = (unsigned)((row * p.Kpad2 + c8 * 8) * 2);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(w2rs, (lds_void*)(W2s + ii * 1024), 16, voff, 0, 0, 0);
        }
#pragma unroll
        for (int a = 0; a < FN; ++a) {
            const int co = wn * (FN * 16) + a * 16 + fc * 4;
#pragma unroll
            for (int r = 0; r < 4; ++r) bias2[a][r] = (co + r < p.C2) ? p.bias2[co + r] : 0.f;
        }
    }

    // ---- issue side: halo pieces of (tile it_tile, chunk it_c) --------------------------------------------------------
    unsigned hconst[LH];
    auto set_tile = [&](int tile) {
        int t = tile;
        const int tw = t % tiles_w; t /= tiles_w;
        const int th = t % tiles_h;
        const int b = t / tiles_h;
        const int h0 = th * TH, w0 = tw * 16;
#pragma unroll
        for (int j = 0; j < LH; ++j) {
            const int ii = wave * LH + j;
            const int s = ii * 64 + lane;
            const int hp = s >> 2, pc = s & 3;
            const int c8 = pc ^ cswz64(hp);
            const int jr = hp / 33, e = hp - jr * 33;
            const int jc = (e < 17) ? 2 * e : 2 * (e - 17) + 1;            // column of the patch this LDS row holds
            const int hi = 2 * h0 - 1 + jr, wi = 2 * w0 - 1 + jc;
            const bool ok = (tile < num_tiles) && (ii < H_INSTR) && (hp < HP) && ((unsigned)hi < (unsigned)p.H) && ((unsigned)wi < (unsigned)p.W);
            hconst[j] = ok ? (unsigned)((((b * p.H + hi) * p.W + wi) * p.x_stride + p.x_coff) * 2 + c8 * 16) : kBufferOOB;
        }
    };
    int it_tile = j0, it_c = 0, it_slot = 0;
    set_tile(it_tile);
    auto issue_next = [&]() {
        unsigned char* dst = Hs + it_slot * HB;
        const unsigned coff = (unsigned)it_c * 64u;
#pragma unroll
        for (int j = 0; j < LH; ++j) {
            const int ii = wave * LH + j;
            const unsigned voff = (hconst[j] == kBufferOOB) ? kBufferOOB : hconst[j] + coff;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (lds_void*)((ii < H_INSTR) ? dst + ii * 1024 : dump), 16, voff, 0, 0, 0);
        }
        it_slot = (it_slot + 1 == NSH) ? 0 : it_slot + 1;
        if (++it_c == nchunk) {
            it_c = 0;
            it_tile += G;
            set_tile(it_tile);
        }
    };

#pragma unroll
    for (int s = 0; s < NSH - 1; ++s) issue_next();
    wait_vmcnt<0>();                      // weights + first chunks landed (once per workgroup)
    __builtin_amdgcn_s_barrier();

    int rd_slot = 0;
    unsigned epmask = 0;                // bit k: iteration (current-1-k) ended a tile
    bool first_iter = true;
    for (int tile = j0; tile < num_tiles; tile += G) {
        f32x4 acc[FN][FM];
#pragma unroll
        for (int a = 0; a < FN; ++a)
#pragma unroll
            for (int r = 0; r < FM; ++r) acc[a][r] = f32x4{bias[a][0], bias[a][1], bias[a][2], bias[a][3]};   // bias rides in the accumulator

        auto chunk = [&](const int c) {
            if (!first_iter) {
                const int k = __builtin_popcount(epmask & ((1u << (NSH - 1)) - 1u));
                if (k == 0) wait_vmcnt<(NSH - 2) * LH>();
                else if (k == 1) wait_vmcnt<(NSH - 2) * LH + S>();
                else wait_vmcnt<(NSH - 2) * LH + 2 * S>();
                __builtin_amdgcn_s_barrier();
            }
            first_iter = false;
            issue_next();
            epmask <<= 1;

            const unsigned char* hsl = Hs + rd_slot * HB;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                bf16x8 wf[3][FN];
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int a = 0; a < FN; ++a) {
                        if constexpr (WREG) {
                            wf[ky][a] = wr[c][ky * 3 + kx][a];
                        } else {
                            const int rw = (c * 9 + ky * 3 + kx) * BN + wn * (FN * 16) + a * 16 + fr;
                            wf[ky][a] = *(const bf16x8*)(Wres + swz64((unsigned)(rw * 64 + fc * 16)));
                        }
                    }
                const int eoff = (kx == 1) ? 17 + fr : fr + (kx >> 1);      // plane O at n, plane E at n / n+1
#pragma unroll
                for (int jj = 0; jj < 2 * FM + 1; ++jj) {
                    const int hp = (2 * wm * FM + jj) * 33 + eoff;
                    const bf16x8 xf = *(const bf16x8*)(hsl + swz64((unsigned)(hp * 64 + fc * 16)));
                    if (jj & 1) {
#pragma unroll
                        for (int a = 0; a < FN; ++a)
                            acc[a][jj >> 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[1][a], xf, acc[a][jj >> 1], 0, 0, 0);
                    } else {
                        if ((jj >> 1) < FM) {
#pragma unroll
                            for (int a = 0; a < FN; ++a)
                                acc[a][jj >> 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0][a], xf, acc[a][jj >> 1], 0, 0, 0);
                        }
                        if ((jj >> 1) >= 1) {
#pragma unroll
                            for (int a = 0; a < FN; ++a)
                                acc[a][(jj >> 1) - 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[2][a], xf, acc[a][(jj >> 1) - 1], 0, 0, 0);
                        }
                    }
                }
            }
            rd_slot = (rd_slot + 1 == NSH) ? 0 : rd_slot + 1;
        };
        if constexpr (WREG) {
#pragma unroll
            for (int c = 0; c < NCH; ++c) chunk(c);
        } else {
            for (int c = 0; c < nchunk; ++c) chunk(c);
        }

        if (PW2) {
            // the tile's intermediate (bias + SiLU, bf16 - exactly the tensor the unfused graph would store) goes through the
            // halo slot this tile just finished with (free until the ring refills it after the next iteration's barrier)
            // and is multiplied by the resident 64x64 weights; acc is then the trailing 1x1's accumulator
            unsigned char* tb = Hs + ((rd_slot == 0) ? NSH - 1 : rd_slot - 1) * HB;
            __builtin_amdgcn_s_barrier();                     // every wave is done reading that slot
#pragma unroll
            for (int r = 0; r < FM; ++r) {
                const int px = (wm * FM + r) * 16 + fr;
#pragma unroll
                for (int a = 0; a < FN; ++a) {
                    const int co = wn * (FN * 16) + a * 16 + fc * 4;
                    __attribute__((aligned(8))) __bf16 o[4];
                    float sv[4] = {acc[a][r][0], acc[a][r][1], acc[a][r][2], acc[a][r][3]};
                    if (p.act == ACT_SILU) silu4_packed(sv);
#pragma unroll
                    for (int i = 0; i < 4; ++i) o[i] = (__bf16)sv[i];
                    // (asm: a compiler-visible ds_write would first drain vmcnt to 0, i.e. wait for the next tile's halo DMA)
                    asm volatile("ds_write_b64 %0, %1" ::"v"((unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)(tb + px * 128 + (((co >> 3) ^ ((px >> 1) & 7)) * 16) + (co & 7) * 2)),
                                 "v"(*(const unsigned long long*)o) : "memory");
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
#pragma unroll
            for (int a = 0; a < FN; ++a)
#pragma unroll
                for (int r = 0; r < FM; ++r) acc[a][r] = f32x4{bias2[a][0], bias2[a][1], bias2[a][2], bias2[a][3]};
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                bf16x8 w2f[FN], t2f[FM];
#pragma unroll
                for (int a = 0; a < FN; ++a) {
                    const int rw = wn * (FN * 16) + a * 16 + fr;
                    w2f[a] = *(const bf16x8*)(W2s + rw * 128 + (((ss * 4 + fc) ^ ((rw >> 1) & 7)) * 16));
                }
#pragma unroll
                for (int r = 0; r < FM; ++r) {
                    const int px = (wm * FM + r) * 16 + fr;
                    t2f[r] = *(const bf16x8*)(tb + px * 128 + (((ss * 4 + fc) ^ ((px >> 1) & 7)) * 16));
                }
#pragma unroll
                for (int a = 0; a < FN; ++a)
#pragma unroll
                    for (int r = 0; r < FM; ++r) acc[a][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2f[a], t2f[r], acc[a][r], 0, 0, 0);
            }
        }
        // ---- epilogue of `tile`: exactly S buffer stores per wave ---------------------------------------------------------
        {
            int t = tile;
            const int tw = t % tiles_w; t /= tiles_w;
            const int th = t % tiles_h;
            const int b = t / tiles_h;
            const int wo = tw * 16 + fr;
            // residual tile first (ordinary loads, all in flight together; the compiler waits once before the first use)
            uint2 rres[FM][FN];
            if (HAS_RES) {
#pragma unroll
                for (int r = 0; r < FM; ++r) {
                    const int ho = th * TH + wm * FM + r;
                    const bool pix_ok = (ho < p.Ho) && (wo < p.Wo);
                    const unsigned m = (unsigned)((b * p.Ho + ho) * p.Wo + wo);
#pragma unroll
                    for (int a = 0; a < FN; ++a) {
                        const int co = n0 + wn * (FN * 16) + a * 16 + fc * 4;
                        rres[r][a] = (pix_ok && co < p.Cout)
                                         ? *(const uint2*)((const __bf16*)p.res + (size_t)m * p.res_stride + p.res_coff + co)
                                         : make_uint2(0u, 0u);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < FM; ++r) {
                const int ho = th * TH + wm * FM + r;
                const bool pix_ok = (ho < p.Ho) && (wo < p.Wo);
                const unsigned m = (unsigned)((b * p.Ho + ho) * p.Wo + wo);
#pragma unroll
                for (int a = 0; a < FN; ++a) {
                    const int co = n0 + wn * (FN * 16) + a * 16 + fc * 4;
                    const bool ok = pix_ok && (co < (PW2 ? p.C2 : p.Cout));
                    float v[4] = {acc[a][r][0], acc[a][r][1], acc[a][r][2], acc[a][r][3]};
                    if ((PW2 ? p.act2 : p.act) == ACT_SILU) silu4_packed(v);
                    if (HAS_RES) {
                        const uint2 rr = rres[r][a];
                        add_res_bf16x4(v, rr);
                    }
                    if (OUT_F32) {
                        const unsigned off = ok ? (m * (unsigned)p.y_stride + (unsigned)(p.y_coff + co)) * 4u : kBufferOOB;
                        store_f32x4(v, yrs, off);
                    } else {
                        const unsigned off = ok ? (m * (unsigned)p.y_stride + (unsigned)(p.y_coff + co)) * 2u : kBufferOOB;
                        store_bf16x4(v, yrs, off);
                    }
                }
            }
        }
        epmask |= 1u;
    }
    wait_vmcnt<0>();
}

// Two kernel templates of one name: eight template arguments = weights in LDS (ids 500-504, their symbols as they were), a ninth = the
// chunk count of a register-weights form.
template <int FM, int FN, int WGM, int WGN, int NSH, bool HAS_RES, bool OUT_F32, bool PW2>
__global__ __launch_bounds__(WGM * WGN * 64) void conv_halo_s2_kernel(const ConvParams p, const int tiles_h, const int tiles_w,
                                                                    const int ntiles, const int G) {
    conv_halo_s2_body<FM, FN, WGM, WGN, NSH, HAS_RES, OUT_F32, PW2, 0>(p, tiles_h, tiles_w, ntiles, G);
}
template <int FM, int FN, int WGM, int WGN, int NSH, bool HAS_RES, bool OUT_F32, bool PW2, int NCH>
__global__ __launch_bounds__(WGM * WGN * 64) void conv_halo_s2_kernel(const ConvParams p, const int tiles_h, const int tiles_w,
                                                                    const int ntiles, const int G) {
    static_assert(NCH > 0, "the ninth argument is a register-weights form's chunk count");
    conv_halo_s2_body<FM, FN, WGM, WGN, NSH, HAS_RES, OUT_F32, PW2, NCH>(p, tiles_h, tiles_w, ntiles, G);
}

// ---------------------------------------------------------------------------------------------------------------
enum { S2_PW2 = 1, S2_WREG = 2 };      // a configuration also has its fused trailing-1x1 (PW2) instance / keeps its weights in registers
template <int FM, int FN, int WGM, int WGN, int FORM = 0> struct S2 : Cfg<FM, FN, WGM, WGN, 3> {
    static constexpr int TH = WGM * FM, BN = WGN * FN * 16;
    static constexpr bool pw2 = FORM & S2_PW2, wreg = FORM & S2_WREG;
    // halo ring + landing zone, then the resident weights (and the fused 1x1's). A register-weights form stages its slab through the ring
    // before the ring is in use, 9 * BN * 64 bytes at a time (a chunk): no weight term, but at least that chunk.
    static constexpr size_t lds(int Cin, bool with_pw2 = false) {
        const size_t ring = (size_t)3 * (((2 * TH + 1) * 33 * 4 + 63) / 64) * 1024 + 1024;
        if (wreg) return std::max(ring, (size_t)9 * BN * 64);
        return ring + (size_t)9 * (Cin / 32) * BN * 64 + (with_pw2 ? (size_t)BN * 128 : 0);
    }
};
// Entries 0-4 are the family's configuration ids (500 + entry). Entries 5-7 are the register-weights instances a launch of id 500 / 501
// resolves to where they are valid (halo_s2_form): no ids of their own - tuner, tables and the forced id speak of tile requests.
using S2Forms = CfgList<
    S2<2, 2, 4, 2, S2_PW2>,     // 0: 8x16 out px x 64 ch, 8 waves
    S2<1, 2, 4, 2, S2_PW2>,     // 1: 4x16 out px x 64 ch, 8 waves
    S2<2, 2, 4, 1>,             // 2: 8x16 out px x 32 ch, 4 waves
    S2<1, 2, 4, 1>,             // 3: 4x16 out px x 32 ch, 4 waves
    S2<2, 4, 4, 2>,             // 4: 8x16 out px x 128 ch, 8 waves (Cin = 32; admitted by no shape)
    S2<1, 2, 4, 2, S2_WREG>,    // 5: 1 with the weights in registers
    S2<2, 2, 4, 2, S2_WREG>,    // 6: 0 with the weights in registers (so the 8-row tile fits for Cin = 64 too)
    S2<2, 2, 2, 4, S2_WREG>>;   // 7: 1 on a layer of more than 96 channels: the same 4x16 pixels, both 64-channel
                                //    blocks in one workgroup, so the input tile is fetched once, not twice
constexpr int kNumS2 = 5;

// A/B and test switch: 1 = every launch keeps its weights in LDS (YOLOP_S2_LDS_WEIGHTS=1, or yp_debug_conv_s2's argument for one call)
static std::atomic<int>& s2_lds_weights_ref() {
    static std::atomic<int> v{env_on("YOLOP_S2_LDS_WEIGHTS") ? 1 : 0};
    return v;
}
int conv_halo_s2_lds_weights(int on) { return on < 0 ? s2_lds_weights_ref().load() : s2_lds_weights_ref().exchange(on ? 1 : 0); }

// The S2Forms entry that configuration c launches p with, -1 = no such c. Register weights: 9 taps x chunks x FN = 2 fragments x 4 VGPRs <= 144
// per wave, i.e. Cin = 32 / 64; not with the fused trailing 1x1 (its weights stay in LDS anyway), not for the 4-wave tiles (ids 502 / 503: unmeasured).
static int halo_s2_form(const ConvParams& p, int c) {
    if (c < 0 || c >= kNumS2) return -1;
    if (c > 1 || p.C2 > 0 || s2_lds_weights_ref().load()) return c;
    if ((p.Cin % 32) != 0 || 9 * (p.Cin / 32) * 2 * 4 > kS2WregMaxVgprs) return c;
    if (c == 0) return 6;
    return p.Cout > 96 ? 7 : 5;
}
static std::string conv_halo_s2_symbol(const ConvParams& p, int c) {
    return with_cfg<S2Forms>(halo_s2_form(p, c), [&](auto k) {
        if (k.wreg) return cfg_symbol("conv_halo_s2_kernel", k, res_f32_args(p) + bool_args({false}) + "," + std::to_string(p.Cin / 32));
        return cfg_symbol("conv_halo_s2_kernel", k, p.C2 > 0 ? bool_args({false, false, true}) : res_f32_args(p) + bool_args({false}));
    });
}

static bool conv_halo_s2_cfg_valid(const ConvParams& p, int c) {
    if (p.ks != 3 || p.stride != 2 || p.pad != 1 || p.up != 1 || (p.Cin % 32) != 0 || (p.Kpad != 9 * p.Cin)) return false;
    if ((p.H & 1) || (p.W & 1) || p.Ho * 2 != p.H || p.Wo * 2 != p.W) return false;
    if (!conv_store_side_ok(p)) return false;
    return with_cfg<S2Forms>(halo_s2_form(p, c), [&](auto k) {                // (the instance that would launch: its LDS need decides)
        using K = decltype(k);
        const int cpad = (p.Cout + 31) / 32 * 32;
        if (K::BN > cpad) return false;
        if (K::lds(p.Cin) > 160 * 1024) return false;
        const long covered = (long)((p.Ho + K::TH - 1) / K::TH * K::TH) * ((p.Wo + 15) / 16 * 16);
        return covered * 2 <= (long)p.Ho * p.Wo * 3;
    });
}

// WCH: the chunk count of a register-weights form (the kernel's ninth argument), none for the weights in LDS
template <bool HAS_RES, bool OUT_F32, bool PW2, int... WCH, int FM, int FN, int WGM, int WGN, int FORM>
static hipError_t launch_halo_s2_var(S2<FM, FN, WGM, WGN, FORM> k, const ConvParams& p, hipStream_t st) {
    static_assert(sizeof...(WCH) == 0 || (FN == 2 && 9 * 2 * FN * 4 <= kS2WregMaxVgprs && 9 * 3 * FN * 4 > kS2WregMaxVgprs), "the chunk counts instantiated are those halo_s2_form admits");
    constexpr int TH = k.TH, BN = k.BN;
    const size_t sh = k.lds(p.Cin, PW2);
    const int B = p.M / (p.Ho * p.Wo);
    const int tiles_h = (p.Ho + TH - 1) / TH, tiles_w = (p.Wo + 15) / 16, ntiles = (p.Cout + BN - 1) / BN;
    const int num_tiles = B * tiles_h * tiles_w;
    // (a register-weights workgroup takes more than half of a CU's registers: one per CU whatever its LDS need)
    const int per_cu = sizeof...(WCH) > 0 ? 1 : (int)std::max<size_t>(1, std::min<size_t>(2, (160 * 1024) / sh));
    int G = (256 * per_cu) / ntiles;
    if (G < 1) G = 1;
    if (G > num_tiles) G = num_tiles;
    auto kern = conv_halo_s2_kernel<FM, FN, WGM, WGN, 3, HAS_RES, OUT_F32, PW2, WCH...>;
    static size_t granted = 0;
    if (hipError_t e = allow_dynamic_lds((const void*)kern, sh, granted)) return e;
    hipLaunchKernelGGL(kern, dim3(G * ntiles), dim3(WGM * WGN * 64), sh, st, p, tiles_h, tiles_w, ntiles, G);
    return hipGetLastError();
}

// ---- fused trailing 1x1 ------------------------------------------------------------------------------------------------
// valid when the 3x3 s2 conv and the 1x1 behind it are both 64 wide (model.1 -> model.2.cv1 of v10-S), nothing carries a residual,
// the intermediate has no other reader (the graph pass checks that), and LDS holds both weight sets beside the halo ring
int conv_halo_s2_pw_cfg(const ConvParams& p) {
    if (p.w2 == nullptr && p.C2 == 0) return -1;
    if (p.Cout != 64 || p.C2 != 64 || p.Kpad2 != 64 || p.res || p.out_f32) return -1;
    for (int c : {0, 1}) {
        ConvParams q = p;
        q.Cout = p.C2;                                          // the store-side checks of the plain form apply to the final view
        if (!conv_halo_s2_cfg_valid(q, c)) continue;
        if (with_cfg<S2Forms>(c, [&](auto k) { return k.lds(p.Cin, true); }) > 160 * 1024) continue;
        return c;
    }
    return -1;
}

size_t conv_halo_s2_lds_bytes(const ConvParams& p, int c) {
    return with_cfg<S2Forms>(halo_s2_form(p, c), [&](auto k) { return k.lds(p.Cin); });
}

static hipError_t launch_conv_halo_s2(const ConvParams& p, int c, hipStream_t st) {
    return with_cfg<S2Forms>(halo_s2_form(p, c), [&](auto k) {
        using K = decltype(k);
        if constexpr (K::wreg) {
            // register-weights forms: the chunk count is a template argument (1 or 2 with FN = 2: halo_s2_form's register bound)
            return with_res_f32(p, [&](auto res, auto f32) {
                if (p.Cin == 32) return launch_halo_s2_var<res, f32, false, 1>(k, p, st);
                if (p.Cin == 64) return launch_halo_s2_var<res, f32, false, 2>(k, p, st);
                return hipErrorInvalidValue;
            });
        } else {
            if (p.C2 > 0) {
                if constexpr (K::pw2) return launch_halo_s2_var<false, false, true>(k, p, st);
                else return hipErrorInvalidValue;
            }
            return with_res_f32(p, [&](auto res, auto f32) { return launch_halo_s2_var<res, f32, false>(k, p, st); });
        }
    });
}

#if !defined(__HIP_DEVICE_COMPILE__)      // (host data: the device pass must not reference the host functions)
const ConvFamily conv_halo_s2_family = {500, kNumS2, conv_halo_s2_cfg_valid, conv_halo_s2_symbol, launch_conv_halo_s2, false, "YOLOP_NO_S2", false};
#endif

}  // namespace yp
