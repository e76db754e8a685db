// Weights-resident streaming form of the bf16 1x1 convolution (configuration ids 1100+): y[px][co] = act(W . x[px] + b) (+ res).
// The 1x1 layers of C2f / SCDown / PSA / the heads (SURVEY.md Appendix A.2-A.4 [U]; run inside `.predict`, reference yolo_seg/app.py:91).
//
// Why: the 1x1 layers on the 80x80 and 40x40 maps are HBM-bound (AI 64-150 FLOP/B) and the k-stepped GEMM
// kernels run them at 2.5-3.6 TB/s: a k-step is a barrier, a ring slot and a handful of 1-KiB pieces per wave, and the pixel rows arrive
// 128 bytes at a time. `cls_out_kernel` (the logits layer, same idea) reaches 4.1 TB/s = 89 % of the chip's copy rate. Here, generalised:
//   * a persistent workgroup keeps ITS block of output channels' weights [NB][K] in LDS for its whole life (NB <= 128; wider layers are
//     split into blocks whose workgroups sit on the same XCD and walk the same pixel tiles at the same time: the second read of a tile is
//     an L2 hit);
//   * a pixel tile is [TP px][K] - whole pixel rows, K * 2 contiguous bytes each - double-buffered by LDS-DMA: ONE barrier per tile, the
//     next tile's rows in flight under this tile's MFMAs, SiLU and stores;
//   * a folded nearest-x2 upsample (1x1 on a [upsampled | skip] concat) is two row segments per pixel, each from its own tensor.
// 8 waves as WGM (pixels) x WGN (channel fragments); a lane ends with 4 consecutive channels of a pixel: bias rides in the accumulator,
// activation, optional residual, bf16, one 8-byte buffer store. A wave issues the same number of stores for every tile (masked ones go
// to an out-of-range offset), so the wait in front of the next tile is a counted `vmcnt`: the rows must have landed, the stores issued
// behind them may still be in flight (first form: `vmcnt(0)` there and four waves - 77 us on `model.4.cv2`, every store drain exposed).
#include "common.h"

namespace yp {

constexpr int WR_NW = 8;
constexpr int WR_MAXNF = 8;             // channel fragments of a block (NB <= 128)

// the fragment set (xs, ws) has landed once at most N younger LDS reads are outstanding; its registers pass through empty asm statements
// behind the wait, so no use of them moves above it (volatile asm statements keep their order)
template <int N, int FM, int NFW> __device__ __forceinline__ void wr_wait_lgkm(bf16x8 (&xs)[FM], bf16x8 (&ws)[NFW]) {
    static_assert(N >= 0 && N < 16, "lgkmcnt range");
    asm volatile("s_waitcnt lgkmcnt(%0)" : : "n"(N) : "memory");
#pragma unroll
    for (int f = 0; f < FM; ++f) asm volatile("" : "+v"(xs[f]));
#pragma unroll
    for (int i = 0; i < NFW; ++i) asm volatile("" : "+v"(ws[i]));
}

// Which instantiations carry the paired (16-byte) store form beside the 8-byte one (kernel and launcher ask the same function): those whose
// waves issue at least 8 stores per tile. Measured on the bench step against the parent build, kernel trace / per-op table: <128,2> (8 stores
// -> 4) 28.0 -> 26.0 us, while <64,2> (4 -> 2) and <32,4> (2 -> 1) came out 0.5 - 0.7 us SLOWER with both epilogues in them than with one, in
// either form - there is too little to halve. They compile to what they were (same instruction count and registers).
template <int TP, int WGN> constexpr bool wres_paired() { return (TP / (16 * (WR_NW / WGN))) * (WR_MAXNF / WGN) >= 8; }

// The kernel's body. CLK: the stamped form (debug, YOLOP_WRES_CLOCKS=1, conv_wres_clk_kernel below): per-wave s_memtime sums of prologue /
// wait + barrier / piece issue / k loop / epilogue, in the style of conv_wreg's; the production kernels carry none of it
template <int TP, int WGN, bool HAS_RES, bool CLK>
__device__ __forceinline__ void conv_wres_body(const ConvParams p, const int NB, const int nblk, const int G, const int TPe) {
    constexpr int WGM = WR_NW / WGN;
    constexpr int FM = TP / (16 * WGM);                            // pixel fragments per wave
    constexpr int NFW = WR_MAXNF / WGN;                            // channel fragments per wave at most
    static_assert(FM >= 1 && FM * 16 * WGM == TP, "pixel tile");
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    const int K = p.Cin, KA = p.x2_C, KB = K - KA;                 // KA channels from the low-resolution source (0: none), KB from x
    const int RBW = K * 2, RBA = KA * 2, RBB = KB * 2;             // row bytes: weights, segment A, segment B
    // swizzle: position pc of row r holds source chunk pc ^ (r & mask); mask = 15 where a row is a multiple of 256 bytes (a fragment read's 16
    // rows then fall into the 16 different 16-byte bank groups), else 7 (8 groups, two rows each)
    const int mA = (KA % 128) == 0 ? 15 : 7, mB = (KB % 128) == 0 ? 15 : 7, mW = ((K % 128) == 0 && (KA % 128) == 0) ? 15 : 7;
    const int nfb = (NB + 15) >> 4;                                // channel fragments of the block
    const int nfw = nfb / WGN;                                     // ... of a wave (nfb % WGN == 0)
    unsigned char* const Ws = smem;                                // [nfb * 16][K]
    const size_t xtile = (size_t)TP * RBW;                         // one pixel tile: [TP][KA] then [TP][KB]
    unsigned char* const Xs = smem + (size_t)nfb * 16 * RBW;       // 2 tiles
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WGM, wn = wave / WGM;
    const int fr = lane & 15, fc = lane >> 4;
    const bool wide = wres_paired<TP, WGN>() && p.wide != 0;       // paired channel order (kernel_util.h): weight rows, bias, residual, store and the counted wait
    // TPe <= TP rows of a tile are in use: the host sizes the tiles so that every tile lane gets the same number of pixels (a 40x40 map in
    // 64-pixel tiles is 3.1 tiles per lane = four rounds of which the last is mostly idle; four rounds of 50 pixels are not)
    const int ntiles = (p.M + TPe - 1) / TPe;
    const int HoWo = p.Ho * p.Wo;
    unsigned long long clk[5] = {0, 0, 0, 0, 0}, last = CLK ? __builtin_amdgcn_s_memtime() : 0ull;
#define WRES_STAMP(i) if constexpr (CLK) { const unsigned long long now = __builtin_amdgcn_s_memtime(); clk[i] += now - last; last = now; }

    // workgroup -> (channel block, tile lane): the blocks of one tile lane are neighbours on one XCD (G % (8 * nblk) == 0)
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int nb = slot % nblk, g = (slot / nblk) * 8 + xcd;
    const int Gt = G / nblk;                                       // tile lanes
    const int n0 = nb * NB;

    const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.x_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t x2rs = __builtin_amdgcn_make_buffer_rsrc((void*)(KA > 0 ? p.x2 : p.x), 0, (int)(KA > 0 ? p.x2_bytes : p.x_bytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (int)p.w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc((void*)p.y, 0, (int)p.y_bytes, 0x00020000);

    // rows are written 16 bytes per lane, whole rows per piece, swizzled as above
    auto issue_tile = [&](int tile, unsigned char* dst) {
        const long row0 = (long)tile * TPe;
        if (KA > 0) {                                              // segment A: channels [0, KA) of pixel (b, ho, wo) live at (b, ho >> 1, wo >> 1) of x2
            const int cpr = RBA >> 4, pieces = (TP * cpr) >> 6;
            for (int ii = wave; ii < pieces; ii += WR_NW) {
                const int s = ii * 64 + lane;
                const int r = s / cpr, pc = s - r * cpr;
                const int c = pc ^ (r & mA);
                const long m = row0 + r;
                unsigned voff = kBufferOOB;
                if (m < p.M && r < TPe) {
                    const int mi = (int)m;
                    const int b = mi / HoWo, q = mi - b * HoWo;
                    const int ho = q / p.Wo, wo = q - ho * p.Wo;
                    voff = (unsigned)((((b * p.x2_H + (ho >> 1)) * p.x2_W + (wo >> 1)) * p.x2_stride + p.x2_coff + c * 8) * 2);
                }
                __builtin_amdgcn_raw_ptr_buffer_load_lds(x2rs, (lds_void*)(dst + ii * 1024), 16, voff, 0, 0, 0);
            }
        }
        {
            unsigned char* const d2 = dst + (size_t)TP * RBA;
            const int cpr = RBB >> 4, pieces = (TP * cpr) >> 6;
            for (int ii = wave; ii < pieces; ii += WR_NW) {
                const int s = ii * 64 + lane;
                const int r = s / cpr, pc = s - r * cpr;
                const int c = pc ^ (r & mB);
                const long m = row0 + r;
                const unsigned voff = (m < p.M && r < TPe) ? (unsigned)((m * p.x_stride + p.x_coff + KA + c * 8) * 2) : kBufferOOB;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (lds_void*)(d2 + ii * 1024), 16, voff, 0, 0, 0);
            }
        }
    };
    {                                                              // the block's weights: rows n0 .. n0 + nfb * 16 (beyond Cout: the packed matrix's zero rows / beyond its end: zeros)
        const int cpr = RBW >> 4, pieces = (nfb * 16 * cpr) >> 6;
        for (int ii = wave; ii < pieces; ii += WR_NW) {
            const int s = ii * 64 + lane;
            const int r = s / cpr, pc = s - r * cpr;
            const int c = pc ^ (r & mW);
            const unsigned voff = (unsigned)(((n0 + weight_row_channel(r, wide)) * p.Kpad + c * 8) * 2);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wrs, (lds_void*)(Ws + ii * 1024), 16, voff, 0, 0, 0);
        }
    }
    int tile = g;
    if (tile < ntiles) issue_tile(tile, Xs);

    float bias[NFW][4];
#pragma unroll
    for (int i = 0; i < NFW; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = wres_paired<TP, WGN>() ? n0 + wn * nfw * 16 + acc_channel(i, fc, wide) + r : n0 + (wn * nfw + i) * 16 + fc * 4 + r;
            bias[i][r] = (i < nfw && co < p.Cout) ? p.bias[co] : 0.f;
        }
    // The bias loads must be KNOWN to be complete before the loop: the compiler cannot count the vector-memory operations of a loop
    // iteration (runtime piece counts) and otherwise puts `s_waitcnt vmcnt(0)` in front of the accumulators' initialisation - in every
    // iteration, behind the next tile's loads: no prefetch at all. Waited for here, then passed through an empty asm statement (a value
    // that comes out of one is no memory result to wait for).
    wait_vmcnt<0>();
#pragma unroll
    for (int i = 0; i < NFW; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) asm volatile("" : "+v"(bias[i][r]));

    WRES_STAMP(0)
    for (int it = 0; tile < ntiles; tile += Gt, ++it) {
        // this tile's rows (first time: the weights too) have landed; the FM * NFW stores of the previous tile (half as many in the paired
        // form), issued behind them, may still fly
        if (it == 0) wait_vmcnt<0>();
        else if (wide) wait_vmcnt<FM * NFW / 2>();
        else wait_vmcnt<FM * NFW>();
        __builtin_amdgcn_s_barrier();
        WRES_STAMP(1)
        if (tile + Gt < ntiles) issue_tile(tile + Gt, Xs + ((it & 1) ^ 1) * xtile);
        WRES_STAMP(2)
        const unsigned char* const XA = Xs + (it & 1) * xtile;
        const unsigned char* const XB = XA + (size_t)TP * RBA;
        f32x4 acc[NFW][FM];
#pragma unroll
        for (int i = 0; i < NFW; ++i)
#pragma unroll
            for (int f = 0; f < FM; ++f) acc[i][f] = f32x4{bias[i][0], bias[i][1], bias[i][2], bias[i][3]};
        // One segment's k loop, software-pipelined by hand: the fragment reads of substep ks + 1 are issued in front of the MFMAs of ks
        // (two register sets, inline-asm `ds_read_b128`, counted `lgkmcnt` waits whose statement the set's registers pass through - the
        // compiler's own schedule was read, wait, MFMA, read, wait, MFMA: four exposed LDS round trips per substep, 9.8 k cycles per
        // 64-pixel tile on `model.6.cv1`). nks is even (segments are multiples of 64 channels).
        auto run_segment = [&](const unsigned char* X, int rb, int kchunk0, int nks, int mX) {
            unsigned xrow[FM], wrow[NFW];
            const unsigned xl = (unsigned)(size_t)(const __attribute__((address_space(3))) unsigned char*)X;
            const unsigned wl = (unsigned)(size_t)(const __attribute__((address_space(3))) unsigned char*)Ws;
#pragma unroll
            for (int f = 0; f < FM; ++f) xrow[f] = xl + (unsigned)(((wm * FM + f) * 16 + fr) * rb);
#pragma unroll
            for (int i = 0; i < NFW; ++i) wrow[i] = wl + (unsigned)(((wn * nfw + min(i, nfw - 1)) * 16 + fr) * RBW + kchunk0 * 16);   // (fewer than NFW fragments: the last one again, multiplied for nothing)
            const unsigned swx = (unsigned)(fr & mX), sww = (unsigned)(fr & mW);      // (row & 15 = fr for both operands' fragments)
            auto rd = [&](bf16x8 (&xd)[FM], bf16x8 (&wd)[NFW], int ks) {
                const unsigned ch = (unsigned)(ks * 4 + fc);
                const unsigned offx = (ch ^ swx) << 4, offw = (ch ^ sww) << 4;
#pragma unroll
                for (int f = 0; f < FM; ++f) asm volatile("ds_read_b128 %0, %1" : "=v"(xd[f]) : "v"(xrow[f] + offx));
#pragma unroll
                for (int i = 0; i < NFW; ++i) asm volatile("ds_read_b128 %0, %1" : "=v"(wd[i]) : "v"(wrow[i] + offw));
            };
            auto mma = [&](bf16x8 (&xd)[FM], bf16x8 (&wd)[NFW]) {
#pragma unroll
                for (int i = 0; i < NFW; ++i)
#pragma unroll
                    for (int f = 0; f < FM; ++f) acc[i][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wd[i], xd[f], acc[i][f], 0, 0, 0);
            };
            bf16x8 xa[FM], wa[NFW], xb[FM], wb[NFW];
            rd(xa, wa, 0);
            for (int ks = 0; ks < nks; ks += 2) {
                rd(xb, wb, ks + 1);
                wr_wait_lgkm<FM + NFW>(xa, wa);
                mma(xa, wa);
                if (ks + 2 < nks) {
                    rd(xa, wa, ks + 2);
                    wr_wait_lgkm<FM + NFW>(xb, wb);
                } else {
                    wr_wait_lgkm<0>(xb, wb);
                }
                mma(xb, wb);
            }
        };
        if (KA > 0) run_segment(XA, RBA, 0, KA >> 5, mA);
        run_segment(XB, RBB, KA >> 3, KB >> 5, mB);
        WRES_STAMP(3)
        // ---- activation, residual, bf16 stores ----------------------------------------------------------------------------------
#pragma unroll
        for (int f = 0; f < FM; ++f) {
            const int ri = (wm * FM + f) * 16 + fr;
            const long m = (long)tile * TPe + ri;
            if (wide) {                                    // a fragment pair (2j, 2j+1) per step: one 16-byte store (and residual read) per lane; nfw is even
#pragma unroll
                for (int j = 0; j < NFW / 2; ++j) {
                    const int co = n0 + wn * nfw * 16 + acc_channel(2 * j, fc, true);           // 8 channels from here: fragment 2j's four, then 2j+1's
                    const bool ok = 2 * j < nfw && ri < TPe && m < p.M && co < p.Cout;          // (Cout % 32 == 0: a lane's eight channels exist together)
                    float v[2][4];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) v[h][q] = acc[2 * j + h][f][q];
                        if (p.act == ACT_SILU && 2 * j < nfw) silu4_packed(v[h]);
                    }
                    if (HAS_RES) {
                        uint2 rr[2];
                        load_res_bf16x8((const __bf16*)p.res + m * p.res_stride + p.res_coff + co, ok, rr[0], rr[1]);
                        add_res_bf16x4(v[0], rr[0]);
                        add_res_bf16x4(v[1], rr[1]);
                    }
                    store_bf16x8(v[0], v[1], yrs, ok ? (unsigned)((m * p.y_stride + p.y_coff + co) * 2) : kBufferOOB);
                }
                continue;
            }
            // the 8-byte form: one store per fragment, weight rows in natural order
#pragma unroll
            for (int i = 0; i < NFW; ++i) {
                const int co = n0 + (wn * nfw + i) * 16 + fc * 4;
                const bool ok = i < nfw && ri < TPe && m < p.M && co < p.Cout;                 // (Cout % 4 == 0: a lane's four channels exist together)
                float v[4] = {acc[i][f][0], acc[i][f][1], acc[i][f][2], acc[i][f][3]};
                if (p.act == ACT_SILU && i < nfw) silu4_packed(v);
                if (HAS_RES && ok) {
                    const uint2 rr = *(const uint2*)((const __bf16*)p.res + m * p.res_stride + p.res_coff + co);
                    v[0] += __uint_as_float(rr.x << 16); v[1] += __uint_as_float(rr.x & 0xffff0000u);
                    v[2] += __uint_as_float(rr.y << 16); v[3] += __uint_as_float(rr.y & 0xffff0000u);
                }
                __attribute__((aligned(8))) __bf16 o[4] = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
                const unsigned off = ok ? (unsigned)((m * p.y_stride + p.y_coff + co) * 2) : kBufferOOB;
                __builtin_amdgcn_raw_buffer_store_b64(*(const __attribute__((ext_vector_type(2))) unsigned*)o, yrs, off, 0, 0);
            }
        }
        WRES_STAMP(4)
    }
    wait_vmcnt<0>();
    if constexpr (CLK) {
        if (lane == 0)
            for (int i = 0; i < 5; ++i) p.clk[((size_t)blockIdx.x * WR_NW + wave) * 5 + i] = clk[i];
    }
#undef WRES_STAMP
}

template <int TP, int WGN, bool HAS_RES>
__global__ __launch_bounds__(WR_NW * 64) void conv_wres_kernel(const ConvParams p, const int NB, const int nblk, const int G, const int TPe) {
    conv_wres_body<TP, WGN, HAS_RES, false>(p, NB, nblk, G, TPe);
}
template <int TP, int WGN>
__global__ __launch_bounds__(WR_NW * 64) void conv_wres_clk_kernel(const ConvParams p, const int NB, const int nblk, const int G, const int TPe) {
    conv_wres_body<TP, WGN, false, true>(p, NB, nblk, G, TPe);
}

// ---------------------------------------------------------------------------------------------------------------------------------------
template <int TP_, int WGN_> struct Wres : Cfg<TP_, WGN_> {
    static constexpr int TP = TP_, WGN = WGN_;
    // channel block of a workgroup: as few blocks as 128 channels each allow, equal sizes, whole fragments (pairs of them for two channel waves)
    static void blocks(const ConvParams& p, int& NB, int& nblk) {
        nblk = (p.Cout + 127) / 128;
        const int q = 16 * WGN;
        NB = ((p.Cout + nblk - 1) / nblk + q - 1) / q * q;
    }
    // the block's resident weights + two pixel tiles
    static size_t lds(const ConvParams& p) {
        int NB, nblk;
        blocks(p, NB, nblk);
        return (size_t)NB * p.Cin * 2 + (size_t)2 * TP * p.Cin * 2;
    }
};
using WresCfgs = CfgList<Wres<64, 2>, Wres<128, 2>, Wres<32, 4>>;

static std::string conv_wres_symbol(const ConvParams& p, int c) {
    return with_cfg<WresCfgs>(c, [&](auto k) { return cfg_symbol("conv_wres_kernel", k, bool_args({p.res != nullptr})); });
}

static bool conv_wres_cfg_valid(const ConvParams& p, int c) {
    if (p.ks != 1 || p.stride != 1 || p.up != 1 || p.w2 || p.out_f32 || p.pool_in || p.up_bilinear) return false;
    if (p.act != ACT_SILU && p.act != ACT_NONE) return false;
    if (p.Cin < 64 || (p.Cin % 64) != 0 || p.Kpad != p.Cin || p.Cin > 1024) return false;
    if (p.x2_C > 0 && ((p.x2_C % 64) != 0 || p.x2_C >= p.Cin || (p.x2_stride & 7) || (p.x2_coff & 7) || p.x2_bytes >= (1ull << 31))) return false;
    if ((p.x_stride & 7) || (p.x_coff & 7)) return false;
    if (!conv_store_side_ok(p) || p.M <= 0 || p.Ho <= 0 || p.Wo <= 0) return false;
    return with_cfg<WresCfgs>(c, [&](auto k) {
        if ((((size_t)k.TP * (p.Cin - p.x2_C) * 2) & 1023) || (((size_t)k.TP * p.x2_C * 2) & 1023)) return false;       // whole 1-KiB pieces per segment
        return k.lds(p) <= 156 * 1024;
    });
}

template <bool HAS_RES, int TP, int WGN>
static hipError_t launch_wres_t(Wres<TP, WGN> k, const ConvParams& p_in, hipStream_t st) {
    int NB, nblk;
    k.blocks(p_in, NB, nblk);
    // paired stores: whole fragment pairs per wave (then NB, and every block's first channel, is a multiple of 32)
    const ConvParams p = with_store_form(p_in, wres_paired<TP, WGN>() ? NB / (16 * WGN) : 1);
    const size_t sh = k.lds(p);
    auto kern = conv_wres_kernel<TP, WGN, HAS_RES>;
    static size_t granted = 0;
    if (hipError_t e = allow_dynamic_lds((const void*)kern, sh, granted)) return e;
    const int ntiles = (p.M + TP - 1) / TP;
    // an HBM-bound kernel: as many workgroups as fit (two per CU when the tiles are small), tile lanes in whole XCD rounds
    const int gmax = sh <= 78 * 1024 ? 512 : 256;
    int lanes8 = gmax / (8 * nblk);                                // tile lanes / 8
    if (lanes8 < 1) lanes8 = 1;
    while (lanes8 > 1 && (lanes8 - 1) * 8 >= ntiles) --lanes8;
    if (const int cap = debug_max_workgroups()) while (lanes8 > 1 && lanes8 * 8 * nblk > cap) --lanes8;
    const int G = lanes8 * 8 * nblk;
    // equal pixels per tile lane: the rounds the full tiles need, then the tile height that fills exactly those rounds
    const long lanes = (long)lanes8 * 8;
    const int rounds = (int)((p.M + lanes * TP - 1) / (lanes * TP));
    const int TPe = tile_balance_enabled(2) ? (int)((p.M + lanes * rounds - 1) / (lanes * rounds)) : TP;
    if constexpr (TP == 128 && WGN == 2 && !HAS_RES) {
        static const bool clocks = env_on("YOLOP_WRES_CLOCKS");   // debug: per-phase s_memtime sums of the stamped instantiation
        if (clocks) {
            auto kc = conv_wres_clk_kernel<TP, WGN>;
            static size_t granted_c = 0;
            if (hipError_t e = allow_dynamic_lds((const void*)kc, sh, granted_c)) return e;
            ConvParams q = p;
            const size_t n = (size_t)G * WR_NW * 5;
            if (hipMalloc((void**)&q.clk, n * 8) != hipSuccess) return hipErrorOutOfMemory;
            hipLaunchKernelGGL(kc, dim3((unsigned)G), dim3(WR_NW * 64), sh, st, q, NB, nblk, G, TPe);
            (void)hipStreamSynchronize(st);
            std::vector<unsigned long long> h(n);
            (void)hipMemcpy(h.data(), q.clk, n * 8, hipMemcpyDeviceToHost);
            (void)hipFree(q.clk);
            double s5[5] = {0, 0, 0, 0, 0};
            for (size_t w = 0; w < n / 5; ++w)
                for (int i = 0; i < 5; ++i) s5[i] += (double)h[w * 5 + i];
            fprintf(stderr, "[wres clocks] %s G=%d tiles=%d  %s stores  per-wave mean cycles: prologue %.0f  wait+barrier %.0f  issue %.0f  k loop %.0f  epilogue %.0f\n",
                    ("conv_wres_kernel<" + cfg_args(k)).c_str(), G, (p.M + TPe - 1) / TPe, p.wide ? "16-byte" : "8-byte", s5[0] / (n / 5), s5[1] / (n / 5), s5[2] / (n / 5), s5[3] / (n / 5), s5[4] / (n / 5));
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)G), dim3(WR_NW * 64), sh, st, p, NB, nblk, G, TPe);
    return hipGetLastError();
}

static hipError_t launch_conv_wres(const ConvParams& p, int c, hipStream_t st) {
    if (!conv_wres_cfg_valid(p, c)) return hipErrorInvalidValue;
    return with_cfg<WresCfgs>(c, [&](auto k) { return p.res ? launch_wres_t<true>(k, p, st) : launch_wres_t<false>(k, p, st); });
}

#if !defined(__HIP_DEVICE_COMPILE__)      // (host data: the device pass must not reference the host functions)
const ConvFamily conv_wres_family = {1100, WresCfgs::size, conv_wres_cfg_valid, conv_wres_symbol, launch_conv_wres, true, "YOLOP_NO_WRES", false};
#endif

}  // namespace yp
