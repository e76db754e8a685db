// The "all_merged" bridge of Masks.xy on the device (yp_mask_contours_merge): hostops.merge_contours - ultralytics' merge_multi_segment as
// the later 8.3.x masks2segments calls it - on the buffers the two contour calls fill (points, per-contour lengths, counts). The point set
// does not change, only the order; everything here is exact integer work. Per mask with contours c_0 .. c_{n-1} in list order:
//   plan      one workgroup per mask: checks the lengths against the count, exclusive scan of the lengths (contour offsets), tiles per
//             consecutive pair and their exclusive scan - the TILE LIST, kept as one offset per pair instead of one record per tile, so its
//             size is bounded by the number of contours whatever the lengths are -, keys preset to all ones, the merged count
//   masktiles exclusive scan of the per-mask tile totals over the masks of the call (64 bit)
//   closest   a FIXED grid walks the tile list (two binary searches per tile: mask, then pair): a tile is CM_TILE points of c_{i-1}, one per
//             lane in registers, against up to CM_BGROUP b-tiles of CM_TILE points of c_i, staged through LDS and read as broadcasts. A lane
//             keeps its first strict minimum while ib ascends; the key (d2 << 38 | ia << 19 | ib) is reduced over the wave and combined
//             with a 64-bit atomic minimum in global memory. Minimum of the key = lexicographic minimum of (d2, ia, ib) = the first minimum of
//             the table in row-major order, however the table is tiled and in whatever order the tiles arrive.
//   emitplan  one workgroup per mask: entry / exit index of every contour from the keys, the flip of a middle contour whose entry index is
//             greater than its exit index (the indices are swapped, NOT mirrored: as the reference), piece lengths, their scans
//   emit      one lane per slot of sum(n_i + 2): slot -> contour by binary search over the offsets, -> closed, rolled, possibly reversed index
//             -> its place on the way out or on the way back (the way-back pieces run in reverse contour order)
// No launch dimension depends on device data and nothing is read back between the trace and the bridge.
#include "common.h"
#include "../../include/yolop.h"

namespace yp {

constexpr int CM_BGROUP = 4;                 // b-tiles per work tile: 256 x 1024 distances, 1024 per lane
constexpr int CM_CLOSEST_GRID = 2048;        // workgroups of the closest-pair walk (8 per CU)
constexpr int CM_EMIT_GRID = 64;             // workgroups per mask of the emission
constexpr int CM_HDR = 8;                    // header words of a mask's slice: [0] state, [1] contours, [2] merged points, [3] tiles
constexpr int CM_ST_PASS = 0, CM_ST_SINGLE = 1, CM_ST_MERGE = 2, CM_ST_DECLINED = 3;
constexpr int CM_IDX_BITS = 19;              // 2^19 = CM_MAX_PTS indices; d2 < 2^26 above them
static_assert((1 << CM_IDX_BITS) == CM_MAX_PTS && 2 * CM_IDX_BITS + 26 == 64, "key = d2 | ia | ib in 64 bits");
static_assert(CM_TILE == YP_CONTOURS_MERGE_TILE && CM_SCAN == YP_CONTOURS_MERGE_SCAN_BLOCK && CM_MAX_PTS == YP_CONTOURS_MERGE_MAX_PTS,
              "include/yolop.h states the bridge's sizes");

// one call's workspace, in 4-byte words: [tile offsets of the masks, 64 bit, n + 1] then one slice per mask
struct MergeLayout {
    int P;                                   // contours a mask's parts row can list (parts_cap - 1)
    size_t o_slices;                         // first slice
    size_t o_off, o_ptile, o_key, o_plan;    // inside a slice: P + 1 offsets, P + 1 tile offsets, P 64-bit keys, P int4 plans
    size_t words;                            // per slice
};

static MergeLayout contours_merge_layout(int n, int parts_cap) {
    MergeLayout L{};
    L.P = parts_cap - 1;
    auto pad4 = [](size_t w) { return (w + 3) & ~(size_t)3; };
    L.o_slices = pad4(2 * ((size_t)n + 1));
    size_t o = CM_HDR;
    L.o_off = o; o += pad4((size_t)L.P + 1);
    L.o_ptile = o; o += pad4((size_t)L.P + 1);
    L.o_key = o; o += pad4(2 * (size_t)L.P);
    L.o_plan = o; o += 4 * (size_t)L.P;
    L.words = o;
    return L;
}

size_t contours_merge_workspace_bytes(int n, int parts_cap) {
    if (n <= 0 || n > 65535 || parts_cap < 2 || parts_cap > CM_MAX_CONTOURS + 1) return 0;
    const MergeLayout L = contours_merge_layout(n, parts_cap);
    return (L.o_slices + (size_t)n * L.words) * 4;
}

// work tiles of the |a| x |b| table of one pair: a-tiles x groups of CM_BGROUP b-tiles (never 0: a contour has a point)
__host__ __device__ static inline unsigned cm_pair_tiles(int la, int lb) {
    return (unsigned)((la + CM_TILE - 1) / CM_TILE) * (unsigned)((lb + CM_TILE * CM_BGROUP - 1) / (CM_TILE * CM_BGROUP));
}

unsigned long long contours_merge_tiles(const int32_t* lengths, int n) {
    unsigned long long t = 0;
    for (int i = 1; i < n; ++i) {
        if (lengths[i - 1] < 1 || lengths[i] < 1 || lengths[i - 1] > CM_MAX_PTS || lengths[i] > CM_MAX_PTS) return 0;
        t += cm_pair_tiles(lengths[i - 1], lengths[i]);
    }
    return t;
}

struct MergeParams {
    const int32_t* pts; const int32_t* count; const int32_t* parts;
    int n, max_pts, parts_cap;
    int32_t* out; int32_t* out_count; int out_cap;
    int* ws;
    MergeLayout L;
};

__device__ __forceinline__ int* cm_ws(const MergeParams& p, int mi) { return p.ws + p.L.o_slices + (size_t)mi * p.L.words; }

// inclusive scan of one value per thread over a CM_SCAN-thread workgroup; `total` = the sum of all of them. s_w: one word per wave.
__device__ __forceinline__ int cm_block_scan(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    __syncthreads();                                         // (s_w of the previous call is read no more)
    if (lane == 63) s_w[wave] = v;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < CM_SCAN / 64; ++k) {
        const int w = s_w[k];
        if (k < wave) before += w;
        all += w;
    }
    total = all;
    return v + before;
}

__global__ __launch_bounds__(CM_SCAN) void cm_plan_kernel(const MergeParams p) {
    __shared__ int s_w[CM_SCAN / 64];
    __shared__ int s_bad;
    const int mi = blockIdx.x, tid = threadIdx.x;
    int* ws = cm_ws(p, mi);
    int* off = ws + p.L.o_off;
    unsigned* ptile = (unsigned*)(ws + p.L.o_ptile);
    unsigned long long* key = (unsigned long long*)(ws + p.L.o_key);
    const int cnt = p.count[mi];
    auto finish = [&](int state, int nc, int total) {       // thread 0: a mask without tiles
        ws[0] = state; ws[1] = nc; ws[2] = total; ws[3] = 0;
        p.out_count[mi] = state == CM_ST_DECLINED ? -1 : total;
    };
    if (cnt <= 0) {                                          // empty, or declined by the trace: the code travels on
        if (tid == 0) finish(CM_ST_PASS, 0, cnt);
        return;
    }
    const int32_t* parts = p.parts + (size_t)mi * p.parts_cap;
    const int nc = parts[0];
    if (nc < 1 || nc > p.L.P || cnt > p.max_pts) {           // more contours than the row lists
        if (tid == 0) finish(CM_ST_DECLINED, 0, 0);
        return;
    }
    if (tid == 0) s_bad = 0;
    __syncthreads();
    // contour offsets
    long long carry = 0;
    for (int base = 0; base < nc; base += CM_SCAN) {
        const int i = base + tid;
        int v = 0;
        if (i < nc) {
            v = parts[1 + i];
            if (v < 1 || v > cnt) { s_bad = 1; v = 0; }
        }
        int total;
        const int inc = cm_block_scan(v, s_w, total);
        if (i < nc) off[i] = (int)min(carry + inc - v, (long long)cnt);
        carry += total;
    }
    __syncthreads();
    const long long merged = nc == 1 ? (long long)cnt : (long long)cnt + 2ll * nc - 2;
    if (s_bad || carry != cnt || merged > p.out_cap) {       // lengths that do not add up to the count, or a list beyond the capacity
        if (tid == 0) finish(CM_ST_DECLINED, 0, 0);
        return;
    }
    if (tid == 0) off[nc] = cnt;
    if (nc == 1) {
        if (tid == 0) finish(CM_ST_SINGLE, 1, cnt);
        return;
    }
    __syncthreads();
    // the tile list: tiles before each pair (pair j = contours j, j + 1)
    unsigned tcarry = 0;
    for (int base = 0; base < nc - 1; base += CM_SCAN) {
        const int j = base + tid;
        int v = 0;
        if (j < nc - 1) {
            v = (int)cm_pair_tiles(off[j + 1] - off[j], off[j + 2] - off[j + 1]);
            key[j] = ~0ull;
        }
        int total;
        const int inc = cm_block_scan(v, s_w, total);
        if (j < nc - 1) ptile[j] = tcarry + (unsigned)(inc - v);
        tcarry += (unsigned)total;
    }
    if (tid == 0) {
        ptile[nc - 1] = tcarry;
        ws[0] = CM_ST_MERGE; ws[1] = nc; ws[2] = (int)merged; ws[3] = (int)tcarry;
        p.out_count[mi] = (int)merged;
    }
}

__global__ __launch_bounds__(CM_SCAN) void cm_masktiles_kernel(const MergeParams p) {
    __shared__ int s_w[CM_SCAN / 64];
    unsigned long long* mto = (unsigned long long*)p.ws;
    const int tid = threadIdx.x;
    unsigned long long carry = 0;
    for (int base = 0; base < p.n; base += CM_SCAN) {
        const int mi = base + tid;
        const int v = mi < p.n ? cm_ws(p, mi)[3] : 0;      // < 2^19 per mask: 1024 of them stay below 2^31
        int total;
        const int inc = cm_block_scan(v, s_w, total);
        if (mi < p.n) mto[mi] = carry + (unsigned long long)(inc - v);
        carry += (unsigned long long)total;
    }
    if (tid == 0) mto[p.n] = carry;
}

__global__ __launch_bounds__(CM_TILE) void cm_closest_kernel(const MergeParams p) {
    __shared__ int2 s_b[CM_TILE];
    const unsigned long long* mto = (const unsigned long long*)p.ws;
    const int tid = threadIdx.x;
    const unsigned long long total = mto[p.n];
    for (unsigned long long t = blockIdx.x; t < total; t += gridDim.x) {
        int lo = 0, hi = p.n - 1;                           // the last mask whose first tile is <= t (masks without tiles share an offset
        while (lo < hi) {                                   // with their successor and are passed over)
            const int mid = (lo + hi + 1) >> 1;
            if (mto[mid] <= t) lo = mid; else hi = mid - 1;
        }
        const int mi = lo;
        const unsigned r = (unsigned)(t - mto[mi]);
        int* ws = cm_ws(p, mi);
        const int nc = ws[1];
        const int* off = ws + p.L.o_off;
        const unsigned* ptile = (const unsigned*)(ws + p.L.o_ptile);
        if (ws[0] != CM_ST_MERGE || r >= ptile[nc - 1]) continue;       // (uniform over the workgroup)
        lo = 0; hi = nc - 2;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (ptile[mid] <= r) lo = mid; else hi = mid - 1;
        }
        const int j = lo;
        const unsigned q = r - ptile[j];
        const int oa = off[j], ob = off[j + 1];
        const int la = ob - oa, lb = off[j + 2] - ob;
        const unsigned ngroups = (unsigned)((lb + CM_TILE * CM_BGROUP - 1) / (CM_TILE * CM_BGROUP));
        const int ia = (int)(q / ngroups) * CM_TILE + tid;
        const int b0 = (int)(q % ngroups) * (CM_TILE * CM_BGROUP), b1 = min(lb, b0 + CM_TILE * CM_BGROUP);
        const int2* pts = (const int2*)p.pts + (size_t)mi * p.max_pts;
        const bool valid = ia < la;
        const int2 a = valid ? pts[oa + ia] : make_int2(0, 0);
        unsigned best_d = 0xffffffffu;
        int best_ib = 0;
        for (int bb = b0; bb < b1; bb += CM_TILE) {
            const int nb = min(CM_TILE, b1 - bb);
            __syncthreads();
            if (tid < nb) s_b[tid] = pts[ob + bb + tid];
            __syncthreads();
            if (valid) {
#pragma unroll 4
                for (int k = 0; k < nb; ++k) {
                    const int2 b = s_b[k];
                    const int dx = a.x - b.x, dy = a.y - b.y;
                    const unsigned d = (unsigned)(dx * dx) + (unsigned)(dy * dy);
                    if (d < best_d) { best_d = d; best_ib = bb + k; }       // strict: the first ib of this row's minimum
                }
            }
        }
        unsigned long long k64 = ~0ull;
        if (valid) k64 = ((unsigned long long)(best_d & 0x3ffffffu) << (2 * CM_IDX_BITS)) | ((unsigned long long)ia << CM_IDX_BITS) | (unsigned)best_ib;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(k64, o);
            k64 = other < k64 ? other : k64;
        }
        if ((tid & 63) == 0 && k64 != ~0ull) atomicMin((unsigned long long*)(ws + p.L.o_key) + j, k64);
    }
}

__global__ __launch_bounds__(CM_SCAN) void cm_emitplan_kernel(const MergeParams p) {
    __shared__ int s_w[CM_SCAN / 64];
    const int mi = blockIdx.x, tid = threadIdx.x;
    int* ws = cm_ws(p, mi);
    if (ws[0] != CM_ST_MERGE) return;
    const int nc = ws[1];
    const int* off = ws + p.L.o_off;
    const unsigned long long* key = (const unsigned long long*)(ws + p.L.o_key);
    int4* plan = (int4*)(ws + p.L.o_plan);
    constexpr unsigned IDX = (1u << CM_IDX_BITS) - 1;
    int fcarry = 0, bcarry = 0;
    for (int base = 0; base < nc; base += CM_SCAN) {
        const int i = base + tid;
        int fwd = 0, back = 0, start = 0, d = 0, flip = 0;
        if (i < nc) {
            const int L = off[i + 1] - off[i];
            // entry: the b index of the pair with the contour before; exit: the a index of the pair with the contour behind
            const int e = i > 0 ? min((int)((unsigned)key[i - 1] & IDX), L - 1) : -1;
            const int x = i < nc - 1 ? min((int)((unsigned)(key[i] >> CM_IDX_BITS) & IDX), L - 1) : -1;
            if (i == 0 || i == nc - 1) {                     // walked whole from its one bridge point, and closed
                start = i == 0 ? x : e;
                fwd = L + 1;
            } else {                                         // out: entry .. exit; back: exit .. the closing point
                flip = e > x;
                start = min(e, x);
                d = abs(e - x);
                fwd = d + 1;
                back = L + 1 - d;
            }
        }
        int ftot, btot;
        const int finc = cm_block_scan(fwd, s_w, ftot);
        const int binc = cm_block_scan(back, s_w, btot);
        if (i < nc) plan[i] = make_int4((int)((unsigned)start | ((unsigned)flip << 31)), d, fcarry + finc - fwd, bcarry + binc);      // .w: way-back points up to and with this one
        fcarry += ftot; bcarry += btot;
    }
}

__global__ __launch_bounds__(256) void cm_emit_kernel(const MergeParams p) {
    const int mi = blockIdx.y;
    const int* ws = cm_ws(p, mi);
    const int state = ws[0];
    if (state != CM_ST_SINGLE && state != CM_ST_MERGE) return;
    const int2* pts = (const int2*)p.pts + (size_t)mi * p.max_pts;
    int2* out = (int2*)p.out + (size_t)mi * p.out_cap;
    const int total = ws[2];
    const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    if (state == CM_ST_SINGLE) {
        for (int s = first; s < total; s += stride) out[s] = pts[s];
        return;
    }
    const int nc = ws[1];
    const int* off = ws + p.L.o_off;
    const int4* plan = (const int4*)(ws + p.L.o_plan);
    const int slots = off[nc] + 2 * nc;                      // L + 2 per contour; a first / last contour leaves its last slot unused
    for (int s = first; s < slots; s += stride) {
        int lo = 0, hi = nc - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (off[mid] + 2 * mid <= s) lo = mid; else hi = mid - 1;
        }
        const int i = lo, r = s - off[i] - 2 * i, L = off[i + 1] - off[i];
        const int4 pl = plan[i];
        const int start = pl.x & 0x7fffffff, flip = (int)((unsigned)pl.x >> 31), d = pl.y;
        int k, dst;                                          // k: index in the rolled, closed contour (0 .. L)
        if (i == 0 || i == nc - 1) {
            if (r > L) continue;
            k = r; dst = pl.z + r;
        } else if (r <= d) {
            k = r; dst = pl.z + r;
        } else {
            k = r - 1; dst = total - pl.w + (k - d);         // the way back lists the later contours first
        }
        int jj = start + k;
        if (jj >= L) jj -= L;
        if (jj >= L) jj -= L;
        if (dst >= 0 && dst < total) out[dst] = pts[off[i] + (flip ? L - 1 - jj : jj)];
    }
}

hipError_t launch_contours_merge(const int32_t* pts, const int32_t* count, const int32_t* parts, int n, int max_pts, int parts_cap, int32_t* out,
                                 int32_t* out_count, int out_cap, void* workspace, hipStream_t st) {
    if (n == 0) return hipSuccess;
    MergeParams p{};
    p.pts = pts; p.count = count; p.parts = parts; p.n = n; p.max_pts = max_pts; p.parts_cap = parts_cap;
    p.out = out; p.out_count = out_count; p.out_cap = out_cap;
    p.ws = (int*)workspace;
    p.L = contours_merge_layout(n, parts_cap);
    hipLaunchKernelGGL(cm_plan_kernel, dim3(n), dim3(CM_SCAN), 0, st, p);
    hipLaunchKernelGGL(cm_masktiles_kernel, dim3(1), dim3(CM_SCAN), 0, st, p);
    hipLaunchKernelGGL(cm_closest_kernel, dim3(CM_CLOSEST_GRID), dim3(CM_TILE), 0, st, p);
    hipLaunchKernelGGL(cm_emitplan_kernel, dim3(n), dim3(CM_SCAN), 0, st, p);
    hipLaunchKernelGGL(cm_emit_kernel, dim3(CM_EMIT_GRID, n), dim3(256), 0, st, p);
    return hipGetLastError();
}

}  // namespace yp
