// Device primitives shared by the kernel files (gfx950 only), each defined once. A primitive that two kernel files use lives here;
// a kernel file defines only what is its own ("Shared device primitives"). Included at the end of common.h.
#pragma once
#include <hip/hip_runtime.h>

#if defined(__HIPCC__)
namespace yp {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) short short2v;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((address_space(3))) void lds_void;

// s_waitcnt vmcnt(N) only (gfx9 encoding: vmcnt[3:0] | expcnt[6:4]=7 | lgkmcnt[11:8]=15 | vmcnt_hi[15:14])
template <int N> __device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N < 64, "vmcnt range");
    __builtin_amdgcn_s_waitcnt((N & 0xF) | (7 << 4) | (0xF << 8) | (((N >> 4) & 3) << 14));
}

// XOR mask applied to the 16-B chunk index within an LDS row. 64-B rows: conflict-free for ds_read_b128 of ANY 16 consecutive rows;
// 128-B rows: conflict-free for 16-row aligned fragments. Derivations: DESIGN.md. cswz<BK> picks by the row's bf16 width.
__device__ __forceinline__ int cswz64(int row) { return ((row >> 2) & 1) << 1; }
__device__ __forceinline__ int cswz128(int row) { return (row >> 1) & 7; }
template <int BK> __device__ __forceinline__ int cswz(int row) {
    return BK == 32 ? cswz64(row) : cswz128(row);
}
// LDS byte offset of the 16-byte piece `c` of the 64-byte row `row` under the chunk swizzle c ^ cswz64(row), computed from the
// UNSWIZZLED offset L = row * 64 + c * 16: the swizzle flips bit 5 of L where bit 2 of row = bit 8 of L is set. Written on L, a fragment read
// costs one add (row offset of the tap, usually a constant) + two bit operations; written on `row`, the compiler spent ~9 VALU instructions per
// read (PMC on conv_tile1: VALU issue 48 % of the kernel's cycles, matrix pipe busy 30 %).
__device__ __forceinline__ unsigned swz64(unsigned L) { return L ^ ((L >> 3) & 32u); }
// The attention kernels' V image ([key][64] bf16, 128-B rows): XOR mask on the 16-B chunk index that moves 32-B pairs, under which the
// transposing ds_read_b64_tr_b16 of 4 key rows x 16 d per 16-lane group is conflict-free.
__device__ __forceinline__ int vswz(int row) { return ((row >> 1) & 3) << 1; }

// XCD-aware bijective remap of the linear block id `bid` of an `nwg`-workgroup launch (blocks b, b+8, ... share an XCD / L2): each XCD
// walks a contiguous run of the remapped ids.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, j = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
}

// SiLU and sigmoid. The three SiLU forms round differently - hardware v_rcp_f32 (1 ulp) against the IEEE division sequence (~12
// instructions), __expf (v_exp_f32 on a scaled argument) against the library expf - and the parity tests' tolerances were set per kernel
// against the form that kernel uses: a kernel must not switch form.
__device__ __forceinline__ float silu_rcp(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }   // bf16 epilogues
__device__ __forceinline__ float silu_fdiv(float x) { return x / (1.0f + __expf(-x)); }                       // fast exp, IEEE division
__device__ __forceinline__ float silu_ieee(float x) { return x / (1.0f + expf(-x)); }                         // fp32 parity mode: library expf, IEEE division
__device__ __forceinline__ float sigmoid_ieee(float x) { return 1.0f / (1.0f + expf(-x)); }
template <typename T> __device__ __forceinline__ float silu_t(float x) { return sizeof(T) == 2 ? silu_rcp(x) : silu_ieee(x); }
// ReLU / SiLU (silu_fdiv's form) / none by the Act code: the fp32-capable 3x3 kernels of the U^2-Net path
__device__ __forceinline__ float act_fdiv(float v, int act) {
    if (act == ACT_RELU) return fmaxf(v, 0.f);
    if (act == ACT_SILU) return silu_fdiv(v);
    return v;
}
// Four SiLUs with the two multiplies and the add as packed fp32 operations (v_pk_mul_f32 / v_pk_add_f32: two values per
// instruction). Same operations and roundings as  x * rcp(1 + exp2(-x * log2e))  element by element, so the same bits; the
// conv epilogues are VALU-bound on exactly this sequence (28 -> 22 cycles per element).
__device__ __forceinline__ void silu4_packed(float* v) {
#pragma unroll
    for (int i = 0; i < 4; i += 2) {
        f32x2 x = {v[i], v[i + 1]};
        f32x2 t = x * -1.4426950408889634f;
        t[0] = __builtin_amdgcn_exp2f(t[0]); t[1] = __builtin_amdgcn_exp2f(t[1]);
        t = t + 1.0f;
        t[0] = __builtin_amdgcn_rcpf(t[0]); t[1] = __builtin_amdgcn_rcpf(t[1]);
        x = x * t;
        v[i] = x[0]; v[i + 1] = x[1];
    }
}

// ---- paired channel order: 16-byte stores of the bf16 conv epilogues --------------------------------------------------------------
// A lane of a 16x16 MFMA accumulator holds A-rows fc*4 .. fc*4+3 of its pixel: with the weight rows in natural order that is 4
// consecutive output channels = one 8-byte store per fragment. The weights are the A operand, so WHICH channel sits in an A-row is
// chosen where the weight rows are fetched: in the paired order, row i of fragment a of the fragment pair (2j, 2j+1) holds channel
//   j*32 + (i >> 2)*8 + (a & 1)*4 + (i & 3),
// lane group fc then holds channels j*32 + fc*8 + 0..3 in fragment 2j and + 4..7 in fragment 2j+1: 8 consecutive bf16 = one 16-byte
// store per lane and fragment pair, 64 contiguous bytes per pixel and instruction. Every output element is the same dot product in the
// same k order (bit-identical); the LDS / register images keep their row positions (swizzles, bank behaviour unchanged); only the
// SOURCE row of the weight fill and the channel index of bias, residual and store change. ConvParams::wide and its conditions: common.h.
//
// paired_channel: row of a weight image whose 32-row blocks are fragment pairs -> the channel fetched into it (a bijection of each block;
// tests/test_wide_store_host.py restates it)
__host__ __device__ constexpr int paired_channel(int row) { return (row & ~31) | ((row & 12) << 1) | ((row & 16) >> 2) | (row & 3); }
__device__ __forceinline__ int weight_row_channel(int row, bool wide) { return wide ? paired_channel(row) : row; }
// first of the 4 channels that lane group fc holds of fragment a, relative to the first channel of the wave's fragment 0
__device__ __forceinline__ int acc_channel(int a, int fc, bool wide) { return wide ? (a >> 1) * 32 + fc * 8 + (a & 1) * 4 : a * 16 + fc * 4; }
// byte offset no buffer holds (every buffer here is below 2 GiB): a load at it returns zeros, a store at it is dropped
constexpr unsigned kBufferOOB = 0x80000000u;
// v[0..3] += four bf16 residual values
__device__ __forceinline__ void add_res_bf16x4(float* v, uint2 rr) {
    v[0] += __uint_as_float(rr.x << 16); v[1] += __uint_as_float(rr.x & 0xffff0000u);
    v[2] += __uint_as_float(rr.y << 16); v[3] += __uint_as_float(rr.y & 0xffff0000u);
}
// the 16-byte residual read of a fragment pair: lo = the 4 channels of fragment 2j, hi = those of fragment 2j+1
__device__ __forceinline__ void load_res_bf16x8(const __bf16* src, bool ok, uint2& lo, uint2& hi) {
    const uint4 q = ok ? *(const uint4*)src : make_uint4(0u, 0u, 0u, 0u);
    lo = make_uint2(q.x, q.y); hi = make_uint2(q.z, q.w);
}
// v[0..3] rounded to bf16: the 8 bytes a store of them writes
__device__ __forceinline__ u32x2 pack_bf16x4(const float* v) {
    __attribute__((aligned(8))) __bf16 o[4] = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
    return *(const u32x2*)o;
}
// (the stores convert in place and do not go through pack_bf16x4: routed through a uint2 value, conv_wreg<2,4,2,4,2,16> spills four registers more)
__device__ __forceinline__ void store_bf16x4(const float* v, __amdgpu_buffer_rsrc_t rs, unsigned off) {
    __attribute__((aligned(8))) __bf16 o[4] = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
    __builtin_amdgcn_raw_buffer_store_b64(*(const __attribute__((ext_vector_type(2))) unsigned*)o, rs, off, 0, 0);
}
__device__ __forceinline__ void store_f32x4(const float* v, __amdgpu_buffer_rsrc_t rs, unsigned off) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, make_float4(v[0], v[1], v[2], v[3])), rs, off, 0, 0);
}
// both fragments of a pair rounded to bf16: the 16 bytes a store of them writes
__device__ __forceinline__ u32x4 pack_bf16x8(const float* lo, const float* hi) {
    __attribute__((aligned(16))) __bf16 o[8] = {(__bf16)lo[0], (__bf16)lo[1], (__bf16)lo[2], (__bf16)lo[3], (__bf16)hi[0], (__bf16)hi[1], (__bf16)hi[2], (__bf16)hi[3]};
    return *(const u32x4*)o;
}
// both fragments of a pair as eight bf16 in one 16-byte store
__device__ __forceinline__ void store_bf16x8(const float* lo, const float* hi, __amdgpu_buffer_rsrc_t rs, unsigned off) {
    __attribute__((aligned(16))) __bf16 o[8] = {(__bf16)lo[0], (__bf16)lo[1], (__bf16)lo[2], (__bf16)lo[3], (__bf16)hi[0], (__bf16)hi[1], (__bf16)hi[2], (__bf16)hi[3]};
    __builtin_amdgcn_raw_buffer_store_b128(*(const __attribute__((ext_vector_type(4))) unsigned*)o, rs, off, 0, 0);
}
__device__ __forceinline__ uint2 load_res_bf16x4(const __bf16* src, bool ok) { return ok ? *(const uint2*)src : make_uint2(0u, 0u); }

// The conv epilogue of one accumulator fragment: SiLU (silu4_packed) when asked, then the residual, then round and store.
// Leaf pieces - add_res_bf16x4, load_res_bf16x4 / x8, pack_bf16x4 / x8, store_bf16x4 / store_f32x4 / store_bf16x8: a kernel that keeps its own
// statement order composes these; written that way a kernel compiles to the instructions of its former hand-written loop.
// Register layer - conv_out_x4: the residual words are already in registers (a kernel that preloads them keeps its own hoisting) and
// `elem` is the element index the caller computed, scaled here by the output's element size; !ok drops the store (the select sits behind
// the arithmetic, where the hand-written loops had it: ahead of it the register-tight kernels spill more). A call issues exactly ONE
// buffer store and nothing else on the vector-memory queue. It also moves the index arithmetic ahead of the SiLU, and register
// allocation notices (profiles/LAB_NOTES.md, "One conv epilogue"): a kernel takes this layer only where its resources and its time
// stay the parent's. load_res_bf16x4 has the same catch: its pointer is formed outside the conditional (conv_dma_p keeps a ternary).
__device__ __forceinline__ void conv_out_x4(f32x4 a, bool silu, bool has_res, uint2 rr, __amdgpu_buffer_rsrc_t rs, bool ok, unsigned elem, bool out_f32) {
    float v[4] = {a[0], a[1], a[2], a[3]};
    if (silu) silu4_packed(v);
    if (has_res) add_res_bf16x4(v, rr);
    if (out_f32) store_f32x4(v, rs, ok ? elem * 4u : kBufferOOB);
    else store_bf16x4(v, rs, ok ? elem * 2u : kBufferOOB);
}

// LDS accesses behind the compiler's back: it cannot tell them from the in-flight LDS-DMA of the next chunk apart and drains vmcnt to 0
// in front of them (= no prefetch at all). The caller orders the reads with explicit lgkmcnt waits before the first use.
__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(size_t)(const __attribute__((address_space(3))) unsigned char*)p; }
__device__ __forceinline__ void lds_write8(unsigned char* dst, unsigned long long v) {
    asm volatile("ds_write_b64 %0, %1" ::"v"((unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)dst), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_write8(unsigned char* dst, uint2 v) { lds_write8(dst, *(const unsigned long long*)&v); }
__device__ __forceinline__ void lds_write8(unsigned char* dst, u32x2 v) { lds_write8(dst, __builtin_bit_cast(unsigned long long, v)); }
__device__ __forceinline__ unsigned long long lds_read8_async(const unsigned char* src) {
    unsigned long long v;
    asm volatile("ds_read_b64 %0, %1" : "=v"(v) : "v"((unsigned)(size_t)(const __attribute__((address_space(3))) unsigned char*)src) : "memory");
    return v;
}
template <typename V = f32x4> __device__ __forceinline__ V lds_read16_async(const unsigned char* src) {
    V v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"((unsigned)(size_t)(const __attribute__((address_space(3))) unsigned char*)src) : "memory");
    return v;
}

// bf16 pair -> order-preserving int16 pair (k = x ^ ((x >> 15) & 0x7fff), an involution), so that one v_pk_max_i16 handles two channels
__device__ __forceinline__ unsigned bf16x2_key(unsigned d) {
    const unsigned s = (d >> 15) & 0x00010001u;
    return d ^ ((s << 15) - s);
}
__device__ __forceinline__ uint4 bf16x8_key(const uint4 v) { return make_uint4(bf16x2_key(v.x), bf16x2_key(v.y), bf16x2_key(v.z), bf16x2_key(v.w)); }
__device__ __forceinline__ unsigned pkmax(unsigned a, unsigned b) {
    const short2v r = __builtin_elementwise_max(__builtin_bit_cast(short2v, a), __builtin_bit_cast(short2v, b));
    return __builtin_bit_cast(unsigned, r);
}
__device__ __forceinline__ uint4 pkmax4(const uint4 a, const uint4 b) {
    return make_uint4(pkmax(a.x, b.x), pkmax(a.y, b.y), pkmax(a.z, b.z), pkmax(a.w, b.w));
}

// the value a tensor of element type T holds after x is stored to it
template <typename T> __device__ __forceinline__ float round_to(float x);
template <> __device__ __forceinline__ float round_to<__bf16>(float x) { return (float)(__bf16)x; }
template <> __device__ __forceinline__ float round_to<float>(float x) { return x; }

// F.upsample(size=..., mode='bilinear') = upsample_bilinear2d, align_corners=False: src = scale*(dst+0.5)-0.5 clamped at 0.
// Source indices i0, i1 and their weights l0, l1 for destination index dst of an n_in -> n_out resize.
// This and bilinear_blend are ONE fixed sequence of IEEE fp32 operations (no contraction into FMAs, which the compiler would choose per
// call site): every kernel that resizes - stand-alone, while loading a convolution's operand, in the tail - gets the same bits, and a host
// restatement with one rounding per operation gets them too (tests/perop_u2net.py: bilinear_f32).
__device__ __forceinline__ void bilinear_tap(int dst, int n_in, int n_out, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
    const float scale = (float)n_in / (float)n_out;
    float f = scale * ((float)dst + 0.5f) - 0.5f;
    f = fmaxf(f, 0.f);
    i0 = (int)f;
    i1 = i0 + ((i0 < n_in - 1) ? 1 : 0);
    l1 = f - (float)i0;
    l0 = 1.f - l1;
}
// the four taps (a b / c d) blended: along each row first, then the two rows
__device__ __forceinline__ float bilinear_blend(float a, float b, float c, float d, float ly0, float ly1, float lx0, float lx1) {
#pragma clang fp contract(off)
    const float top = lx0 * a + lx1 * b;
    const float bot = lx0 * c + lx1 * d;
    return ly0 * top + ly1 * bot;
}

}  // namespace yp
#endif
