// The LARGE path of Masks.xy + the shaft-length rectangle (yp_mask_contours_large): the same definitions as contour.hip (its header comment
// and hostops.py "Masks.xy" are the contract) for the masks whose tables do not fit one workgroup's LDS - 4K frames, boxes above
// ~1400x700, more than 64 outer borders. Every table lives in a caller-provided workspace in HBM (the bit image of a 3840x2160 frame is
// 1.04 MB and stays L2-resident) and a mask's candidates are spread over as many workgroups as there are waves of them:
//   init      per mask: run / skip (YP_CONTOURS_ONLY_DECLINED) / rectangle only (points present, rectangle row at (-1, -1))
//   bits      bit image of the WHOLE frame (no bounding box: the column tables are indexed by mask column anyway), zero border included
//   candrow   candidate starts (set pixel, W / NW / N / NE clear) by word-parallel bit logic -> candidate bit image + per-row popcount
//   scan      exclusive scan of the row counts; candlist: per-row scan of the word popcounts -> the candidates IN RASTER ORDER, and for
//             every word the index of its first candidate (find(pixel) = that + popcount below the bit): no atomic decides an order
//   trace     one lane per candidate walks to the next checkpoint (contour.hip 3a, trace_segment) and records successor, moves, kept
//             points, first / last move, raster-first pixel. Nothing is emitted yet: the offsets are not known
//   cycles    borders = cycles of the successor pointers; the candidate with the lowest index LEADS (it alone walks the whole cycle, the
//             others stop at the first lower index). An outer border is a cycle whose raster-first pixel is its leader; the leader fixes each
//             segment's offset inside the contour and the joint points
//   order1    outer borders compacted in raster order (scan of the leader flags)
//   nest      RETR_EXTERNAL without a parity table: from a border's start pixel q go west to the nearest set pixel p. The background east
//             of p and west of q is one 4-connected run, so q's blob lies in the background component G on that side of p. A walker started
//             at p with its search at east follows the border between p's blob and G to the next checkpoint: a cycle that is an outer border
//             -> q is outside that blob and exactly as nested as it is (link); any other cycle, or a border without checkpoints, is a hole
//             border -> q is nested; no set pixel to the west -> external
//   order2    links resolved (they point to earlier borders only), the list bottom-up ("all") or the border with the most points, the later
//             start on a tie ("largest"), prefix offsets, count / parts
//   emit      every segment of a listed border is walked once more and writes its points straight to their final places (the walkers go
//             clockwise, the list runs the other way behind the start point: the index is mirrored while writing)
//   hull      per-column min / max by MASK column (at most W <= 4096 columns, whatever the scale: scale_coord is monotone per axis, columns
//             that scale to the same x are merged on the fly), Andrew's monotone chain, rotating calipers in float64 - as contour.hip
// Fixed visit and summation orders throughout: a mask gives the same bytes alone and inside a batch.
#include "common.h"
#include "contour_common.h"
#include "../../include/yolop.h"
#include <algorithm>

namespace yp {

constexpr int CL_THREADS = 1024;
constexpr int CL_ST_RUN = 0, CL_ST_SKIP = 1, CL_ST_RECT = 2, CL_ST_DONE = 3;   // header word 0
constexpr int CL_HDR = 16;                   // header words: [0] state, [1] candidates, [2] outer borders
constexpr int CL_LINK_EXT = -1, CL_LINK_NESTED = -2, CL_LINK_FAIL = -3;

// one mask's slice of the workspace, in 4-byte words
struct LargeLayout {
    int pitch, wpr, candcap;
    size_t nwords;                           // (H + 2) * pitch
    size_t o_bm, o_cbm, o_woff, o_rowcnt, o_rowoff, o_cand;
    size_t o_nxt, o_nkp, o_nmv, o_mvs, o_mnl, o_bid, o_rel, o_jkp, o_lnp, o_bno;     // per candidate
    size_t o_bk, o_blink, o_bbase, o_bext;                                          // per outer border
    size_t words;
};

LargeLayout contours_large_layout(int H, int W) {
    LargeLayout L{};
    L.wpr = (W + 31) / 32;
    L.pitch = L.wpr + 3;
    L.nwords = (size_t)(H + 2) * L.pitch;
    const size_t maxc = (size_t)H * ((W + 1) / 2);                       // a candidate's west neighbour is clear
    L.candcap = (int)std::min<size_t>((size_t)CL_MAXCAND, maxc);
    size_t o = CL_HDR;
    auto take = [&](size_t nw) { const size_t at = o; o += (nw + 3) & ~(size_t)3; return at; };
    L.o_bm = take(L.nwords); L.o_cbm = take(L.nwords); L.o_woff = take(L.nwords);
    L.o_rowcnt = take(H); L.o_rowoff = take(H);
    size_t* per[] = {&L.o_cand, &L.o_nxt, &L.o_nkp, &L.o_nmv, &L.o_mvs, &L.o_mnl, &L.o_bid, &L.o_rel, &L.o_jkp, &L.o_lnp, &L.o_bno,
                     &L.o_bk, &L.o_blink, &L.o_bbase, &L.o_bext};
    for (size_t* q : per) *q = take(L.candcap);
    L.words = o;
    return L;
}

size_t contours_large_workspace_bytes(int n, int H, int W) {
    if (n < 0 || H <= 0 || W <= 0 || H > CL_MAXDIM || W > CL_MAXDIM) return 0;
    return (size_t)n * contours_large_layout(H, W).words * 4;
}

struct LargeParams {
    const uint8_t* masks;      // [n][H][W], non-zero = set
    int n, H, W, max_pts;
    int32_t* pts; int32_t* count; int strategy;
    int32_t* parts; int parts_cap;
    double* rect;
    int flags, scaled, H0, W0;
    float gain, padx, pady;
    int* ws;
    LargeLayout L;
};

__device__ __forceinline__ int* cl_ws(const LargeParams& p, int mi) { return p.ws + (size_t)mi * p.L.words; }

__device__ __forceinline__ void cl_finish(const LargeParams& p, int mi, int* ws, int code) {      // one thread: nothing (more) to list
    p.count[mi] = code;
    if (p.rect) { p.rect[2 * mi] = 0.0; p.rect[2 * mi + 1] = 0.0; }
    if (p.parts) p.parts[(size_t)mi * p.parts_cap] = 0;
    ws[0] = CL_ST_DONE;
}

__global__ __launch_bounds__(256) void cl_init_kernel(const LargeParams p) {
    const int mi = blockIdx.x * 256 + threadIdx.x;
    if (mi >= p.n) return;
    int* ws = cl_ws(p, mi);
    int st = CL_ST_RUN;
    if (p.flags & YP_CONTOURS_ONLY_DECLINED) {
        const bool has_pts = p.count[mi] >= 0;
        const bool has_rect = !p.rect || p.rect[2 * mi] >= 0.0;
        st = has_pts ? (has_rect ? CL_ST_SKIP : CL_ST_RECT) : CL_ST_RUN;
    }
    ws[0] = st; ws[1] = 0; ws[2] = 0;
}

// bit image of the whole frame, its zero border included: one thread per stored word
__global__ __launch_bounds__(256) void cl_bits_kernel(const LargeParams p) {
    const int mi = blockIdx.y;
    int* ws = cl_ws(p, mi);
    if (ws[0] != CL_ST_RUN) return;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.L.nwords) return;
    const int r = (int)(i / p.L.pitch), j = (int)(i - (size_t)r * p.L.pitch);
    unsigned wv = 0u;
    if (r >= 1 && r <= p.H && j >= 1 && j <= p.L.wpr) {
        const int x0 = (j - 1) * 32;
        const uint8_t* src = p.masks + ((size_t)mi * p.H + (r - 1)) * p.W + x0;
        if (x0 + 32 <= p.W && ((uintptr_t)src & 15) == 0) {
            const uint4 a = ((const uint4*)src)[0], b = ((const uint4*)src)[1];
            const unsigned v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const unsigned u = v[q];
                const unsigned nib = ((u & 0xffu) ? 1u : 0u) | ((u & 0xff00u) ? 2u : 0u) | ((u & 0xff0000u) ? 4u : 0u) | ((u & 0xff000000u) ? 8u : 0u);
                wv |= nib << (4 * q);
            }
        } else {
            const int e = min(32, p.W - x0);
            for (int q = 0; q < e; ++q) wv |= (src[q] ? 1u : 0u) << q;
        }
    }
    ((unsigned*)ws)[p.L.o_bm + i] = wv;
}

// candidate starts of one row: set pixels whose W, NW, N, NE neighbours are clear
__global__ __launch_bounds__(256) void cl_candrow_kernel(const LargeParams p) {
    __shared__ int s_cnt[4];
    const int mi = blockIdx.y, y = blockIdx.x, tid = threadIdx.x;
    int* ws = cl_ws(p, mi);
    if (ws[0] != CL_ST_RUN) return;
    const unsigned* r = (const unsigned*)ws + p.L.o_bm + (size_t)(y + 1) * p.L.pitch;
    const unsigned* u = r - p.L.pitch;
    unsigned* cb = (unsigned*)ws + p.L.o_cbm + (size_t)(y + 1) * p.L.pitch;
    int cnt = 0;
    for (int j = 1 + tid; j <= p.L.wpr; j += 256) {
        const unsigned m = r[j];
        unsigned c = 0u;
        if (m) {
            const unsigned wb = (m << 1) | (r[j - 1] >> 31);
            const unsigned ub = u[j];
            const unsigned nwb = (ub << 1) | (u[j - 1] >> 31);
            const unsigned neb = (ub >> 1) | (u[j + 1] << 31);
            c = m & ~wb & ~ub & ~nwb & ~neb;
        }
        cb[j] = c;
        cnt += __popc(c);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) ws[p.L.o_rowcnt + y] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// exclusive scan of s[0 .. CL_THREADS) in place (Hillis-Steele on the inclusive sums), total returned to every thread
__device__ __forceinline__ int cl_block_scan(int* s, int v, int tid, int* total) {
    s[tid] = v;
    __syncthreads();
    for (int o = 1; o < CL_THREADS; o <<= 1) {
        const int a = tid >= o ? s[tid - o] : 0;
        __syncthreads();
        s[tid] += a;
        __syncthreads();
    }
    *total = s[CL_THREADS - 1];
    const int excl = s[tid] - v;
    __syncthreads();
    return excl;
}

__global__ __launch_bounds__(CL_THREADS) void cl_scan_kernel(const LargeParams p) {
    __shared__ int s[CL_THREADS];
    const int mi = blockIdx.x, tid = threadIdx.x;
    int* ws = cl_ws(p, mi);
    if (ws[0] != CL_ST_RUN) return;
    const int per = (p.H + CL_THREADS - 1) / CL_THREADS;          // (H <= 4096: at most 4 rows per thread)
    const int y0 = tid * per, y1 = min(p.H, y0 + per);
    int sum = 0;
    for (int y = y0; y < y1; ++y) sum += ws[p.L.o_rowcnt + y];
    int total;
    int run = cl_block_scan(s, sum, tid, &total);
    for (int y = y0; y < y1; ++y) { ws[p.L.o_rowoff + y] = run; run += ws[p.L.o_rowcnt + y]; }
    if (tid == 0) {
        ws[1] = total;
        if (total == 0) cl_finish(p, mi, ws, 0);                  // empty mask
        else if (total > p.L.candcap) cl_finish(p, mi, ws, -2);
    }
}

// the candidates of one row in raster order + the index of every word's first candidate
__global__ __launch_bounds__(256) void cl_candlist_kernel(const LargeParams p) {
    __shared__ int s[256];
    const int mi = blockIdx.y, y = blockIdx.x, tid = threadIdx.x;
    int* ws = cl_ws(p, mi);
    if (ws[0] != CL_ST_RUN) return;
    if (ws[p.L.o_rowcnt + y] == 0) return;
    const unsigned* cb = (const unsigned*)ws + p.L.o_cbm + (size_t)(y + 1) * p.L.pitch;
    int* wo = ws + p.L.o_woff + (size_t)(y + 1) * p.L.pitch;
    int base = ws[p.L.o_rowoff + y];
    for (int j0 = 1; j0 <= p.L.wpr; j0 += 256) {                  // (W <= 4096: one round)
        const int j = j0 + tid;
        unsigned c = j <= p.L.wpr ? cb[j] : 0u;
        const int pc = __popc(c);
        s[tid] = pc;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int a = tid >= o ? s[tid - o] : 0;
            __syncthreads();
            s[tid] += a;
            __syncthreads();
        }
        int at = base + s[tid] - pc;
        const int round_total = s[255];
        __syncthreads();
        if (j <= p.L.wpr) wo[j] = at;
        while (c) {
            const int b = __builtin_ctz(c);
            c &= c - 1;
            ws[p.L.o_cand + at++] = y * p.W + (j - 1) * 32 + b;
        }
        base += round_total;
    }
}

struct LargeView {
    Bitmap bm;
    const unsigned* cbm;
    const int* woff;
    int W;
    __device__ __forceinline__ bool is_cand(int rb, int x) const { return (cbm[rb + bm.pitch + 1 + (x >> 5)] >> (x & 31)) & 1u; }
    // index of the candidate at column x of the row whose row above starts at word rb
    __device__ __forceinline__ int find(int rb, int x) const {
        const int wi = rb + bm.pitch + 1 + (x >> 5);
        return woff[wi] + __popc(cbm[wi] & ((1u << (x & 31)) - 1u));
    }
};

__device__ __forceinline__ LargeView cl_view(const LargeParams& p, const int* ws) {
    return LargeView{Bitmap{(const unsigned*)ws + p.L.o_bm, p.L.pitch}, (const unsigned*)ws + p.L.o_cbm, ws + p.L.o_woff, p.W};
}

__device__ __forceinline__ int cl_fresh(unsigned nbm) { return (6 + __builtin_ctz(((nbm >> 6) | (nbm << 2)) & 0xffu)) & 7; }

// One segment of a border, as contour.hip's trace_segment: from candidate (sy,sx) to the next candidate on the same border that the walker
// is about to leave by the move a fresh trace would take there. EMIT: the interior kept point i goes to out[place(i)].
struct LSeg { int next, nkeep, nmoves, first_move, last_move, min_lin; };
template <bool EMIT, typename Place>
__device__ void cl_walk_segment(const LargeView& v, int sy, int sx, int max_steps, int32_t* out, Place place, LSeg& si) {
    const int pitch = v.bm.pitch, start_lin = sy * v.W + sx;
    int cy = sy, cx = sx, rb = sy * pitch, lin = start_lin;
    si.next = -1; si.nkeep = 0; si.nmoves = 0; si.first_move = 0; si.last_move = 0; si.min_lin = start_lin;
    int mn = start_lin;
    unsigned nbm = v.bm.ring(rb, cx);
    if (nbm == 0) { si.next = v.find(rb, cx); return; }             // isolated pixel: a border of its own, no moves
    int nd = cl_fresh(nbm);
    si.first_move = nd;
    int prev_move = nd, nkeep = 0, nmoves = 1;
    {
        const int dy = c_dy(nd), dx = c_dx(nd);
        cy += dy; cx += dx; rb += dy * pitch; lin += dy * v.W + dx;
    }
    int d = (nd + 6 - (nd & 1)) & 7;
    for (int step = 1; step < max_steps; ++step) {
        nbm = v.bm.ring(rb, cx);
        nd = (d + __builtin_ctz(((nbm >> d) | (nbm << (8 - d))) & 0xffu)) & 7;
        mn = min(mn, lin);
        if (v.is_cand(rb, cx) && nd == cl_fresh(nbm)) {
            si.next = v.find(rb, cx); si.nkeep = nkeep; si.nmoves = nmoves; si.last_move = prev_move; si.min_lin = mn;
            return;
        }
        if (nd != prev_move) {
            if (EMIT) { const int at = place(nkeep); if (at >= 0) { out[2 * at] = cx; out[2 * at + 1] = cy; } }
            ++nkeep;
        }
        prev_move = nd;
        const int dy = c_dy(nd), dx = c_dx(nd);
        cy += dy; cx += dx; rb += dy * pitch; lin += dy * v.W + dx;
        ++nmoves;
        d = (nd + 6 - (nd & 1)) & 7;
    }
}

__global__ __launch_bounds__(64) void cl_trace_kernel(const LargeParams p) {
    const int mi = blockIdx.y, k = blockIdx.x * 64 + threadIdx.x;
    int* ws = cl_ws(p, mi);
    if (ws[0] != CL_ST_RUN || k >= ws[1]) return;
    const LargeView v = cl_view(p, ws);
    const int lin = ws[p.L.o_cand + k];
    const int sy = lin / p.W, sx = lin - sy * p.W;
    LSeg si;
    cl_walk_segment<false>(v, sy, sx, 4 * p.H * p.W + 8, nullptr, [](int) { return -1; }, si);
    ws[p.L.o_nxt + k] = si.next; ws[p.L.o_nkp + k] = si.nkeep; ws[p.L.o_nmv + k] = si.nmoves;
    ws[p.L.o_mvs + k] = si.first_move | (si.last_move << 4); ws[p.L.o_mnl + k] = si.min_lin;
    ws[p.L.o_bid + k] = -1; ws[p.L.o_lnp + k] = 0;
}

// borders = cycles of the successor pointers. The lowest candidate of a cycle leads it: it walks the cycle twice (is it the lowest? then
// the sums, each segment's offset inside the contour and its joint point); every other candidate stops at the first lower index.
__global__ __launch_bounds__(64) void cl_cycles_kernel(const LargeParams p) {
    const int mi = blockIdx.y, k = blockIdx.x * 64 + threadIdx.x;
    int* ws = cl_ws(p, mi);
    if (ws[0] != CL_ST_RUN) return;
    const int ncand = ws[1];
    if (k >= ncand) return;
    const int* nxt = ws + p.L.o_nxt;
    const int* nkp = ws + p.L.o_nkp;
    const int* nmv = ws + p.L.o_nmv;
    const int* mvs = ws + p.L.o_mvs;
    const int* mnl = ws + p.L.o_mnl;
    {
        int j = k, len = 0;
        do {
            const int jn = nxt[j];
            if (jn < k) return;                                     // a broken walk (-1) or a lower candidate on the cycle
            j = jn;
        } while (j != k && ++len < ncand);
        if (j != k) return;
    }
    int j = k, prev = -1, off = 0, moves = 0, cmin = 0x7fffffff;
    do {
        const int joint = (prev >= 0 && (((mvs[prev] >> 4) & 15) != (mvs[j] & 15))) ? 1 : 0;     // the joint point at this segment's start
        off += joint;
        ws[p.L.o_bid + j] = k; ws[p.L.o_jkp + j] = joint; ws[p.L.o_rel + j] = off;
        off += nkp[j];
        moves += nmv[j];
        cmin = min(cmin, mnl[j]);
        prev = j;
        j = nxt[j];
    } while (j != k);
    // a border counts from its raster-first PIXEL only: a hole border whose first pixel is no local top has candidates but no survivor
    if (cmin != ws[p.L.o_cand + k]) return;
    const int start_kept = (((mvs[prev] >> 4) & 15) != (mvs[k] & 15)) ? 1 : 0;
    const int kept = off + start_kept;
    int np;
    if (moves == 0) np = 1;                                         // isolated pixel
    else if (moves <= 2) np = moves;                                // _compress keeps everything
    else np = kept > 0 ? kept : 1;
    const int sk = (moves <= 2) ? 1 : start_kept;
    ws[p.L.o_lnp + k] = (np << 1) | sk;
}

// outer borders in raster order: scan of the leader flags
__global__ __launch_bounds__(CL_THREADS) void cl_order1_kernel(const LargeParams p) {
    __shared__ int s[CL_THREADS];
    const int mi = blockIdx.x, tid = threadIdx.x;
    int* ws = cl_ws(p, mi);
    if (ws[0] != CL_ST_RUN) return;
    const int ncand = ws[1];
    const int per = (ncand + CL_THREADS - 1) / CL_THREADS;
    const int k0 = min(ncand, tid * per), k1 = min(ncand, k0 + per);
    int cnt = 0;
    for (int k = k0; k < k1; ++k) cnt += ws[p.L.o_lnp + k] != 0;
    int total;
    int at = cl_block_scan(s, cnt, tid, &total);
    for (int k = k0; k < k1; ++k)
        if (ws[p.L.o_lnp + k] != 0) { ws[p.L.o_bk + at] = k; ws[p.L.o_bno + k] = at; ++at; }
    if (tid == 0) {
        ws[2] = total;
        if (total == 0) cl_finish(p, mi, ws, -2);                   // (every walk broke: cannot happen on a bit image)
    }
}

// RETR_EXTERNAL, see the header comment: link of outer border b = CL_LINK_EXT, CL_LINK_NESTED or the earlier border it is as nested as
__global__ __launch_bounds__(64) void cl_nest_kernel(const LargeParams p) {
    const int mi = blockIdx.y, b = blockIdx.x * 64 + threadIdx.x;
    int* ws = cl_ws(p, mi);
    if (ws[0] != CL_ST_RUN) return;
    const int nb = ws[2];
    if (b >= nb) return;
    if (nb == 1) { ws[p.L.o_blink] = CL_LINK_EXT; return; }
    const LargeView v = cl_view(p, ws);
    const int pitch = p.L.pitch;
    const int qlin = ws[p.L.o_cand + ws[p.L.o_bk + b]];
    const int qy = qlin / p.W, qx = qlin - qy * p.W;
    // nearest set pixel west of q in its row
    const unsigned* row = v.bm.w + (size_t)(qy + 1) * pitch;
    int jw = 1 + (qx >> 5);
    unsigned m = row[jw] & ((1u << (qx & 31)) - 1u);
    while (m == 0u && jw > 1) m = row[--jw];
    if (m == 0u) { ws[p.L.o_blink + b] = CL_LINK_EXT; return; }
    const int px = (jw - 1) * 32 + 31 - __builtin_clz(m);
    int cy = qy, cx = px, rb = qy * pitch;
    const int max_steps = 4 * p.H * p.W + 8;
    int link = CL_LINK_FAIL, j = -1;
    unsigned nbm = v.bm.ring(rb, cx);
    if (nbm == 0) j = v.find(rb, cx);                               // p is an isolated pixel: its own outer border
    else {
        int d = 0, start_nd = -1;                                   // the search starts at east: the background run between p and q
        for (int step = 0; step < max_steps; ++step) {
            nbm = v.bm.ring(rb, cx);
            const int nd = (d + __builtin_ctz(((nbm >> d) | (nbm << (8 - d))) & 0xffu)) & 7;
            if (v.is_cand(rb, cx) && nd == cl_fresh(nbm)) { j = v.find(rb, cx); break; }
            if (step == 0) start_nd = nd;
            else if (cy == qy && cx == px && nd == start_nd) { link = CL_LINK_NESTED; break; }     // a border without checkpoints: a hole's
            const int dy = c_dy(nd), dx = c_dx(nd);
            cy += dy; cx += dx; rb += dy * pitch;
            d = (nd + 6 - (nd & 1)) & 7;
        }
    }
    if (j >= 0) {
        const int lead = ws[p.L.o_bid + j];
        if (lead >= 0) link = ws[p.L.o_lnp + lead] ? ws[p.L.o_bno + lead] : CL_LINK_NESTED;
    }
    ws[p.L.o_blink + b] = link;
}

// which borders are listed, where, and the counts
__global__ __launch_bounds__(CL_THREADS) void cl_order2_kernel(const LargeParams p) {
    __shared__ int s[CL_THREADS];
    __shared__ int s_fail;
    __shared__ unsigned long long s_best[CL_THREADS / 64];
    const int mi = blockIdx.x, tid = threadIdx.x;
    int* ws = cl_ws(p, mi);
    if (ws[0] != CL_ST_RUN) return;
    const int nb = ws[2];
    const int* bk = ws + p.L.o_bk;
    const int* lnp = ws + p.L.o_lnp;
    int* bext = ws + p.L.o_bext;
    int* bbase = ws + p.L.o_bbase;
    if (tid == 0) s_fail = 0;
    __syncthreads();
    for (int b = tid; b < nb; b += CL_THREADS) {
        int l = ws[p.L.o_blink + b];
        for (int it = 0; l >= 0 && it < nb; ++it) l = l < b ? ws[p.L.o_blink + l] : CL_LINK_FAIL;     // (links point to earlier borders)
        if (l != CL_LINK_EXT && l != CL_LINK_NESTED) s_fail = 1;
        bext[b] = l == CL_LINK_EXT ? 1 : 0;
        bbase[b] = -1;
    }
    __syncthreads();
    if (s_fail) { if (tid == 0) cl_finish(p, mi, ws, -2); return; }
    int no = 0, total = 0;
    if (p.strategy == 1) {
        // bottom-up: descending raster order of the start pixels = descending border index; thread t takes a run of them, highest first
        const int per = (nb + CL_THREADS - 1) / CL_THREADS;
        const int r0 = min(nb, tid * per), r1 = min(nb, r0 + per);      // r = nb - 1 - b
        int cnt = 0, sum = 0;
        for (int r = r0; r < r1; ++r) { const int b = nb - 1 - r; if (bext[b]) { ++cnt; sum += lnp[bk[b]] >> 1; } }
        int tot_cnt, tot_sum;
        int at = cl_block_scan(s, cnt, tid, &tot_cnt);
        // (a border's points are pixels of the frame, each on at most four visits: the sum stays far inside int range)
        int base = cl_block_scan(s, sum, tid, &tot_sum);
        if (tot_sum <= p.max_pts) {
            for (int r = r0; r < r1; ++r) {
                const int b = nb - 1 - r;
                if (!bext[b]) continue;
                const int np = lnp[bk[b]] >> 1;
                bbase[b] = base;
                if (p.parts && at + 1 < p.parts_cap) p.parts[(size_t)mi * p.parts_cap + at + 1] = np;
                base += np; ++at;
            }
        }
        no = tot_cnt; total = tot_sum;
    } else {
        // most points; on a tie the first of the bottom-up list = the later start
        unsigned long long best = 0ull;
        for (int b = tid; b < nb; b += CL_THREADS)
            if (bext[b]) best = max(best, ((unsigned long long)(unsigned)(lnp[bk[b]] >> 1) << 32) | (unsigned long long)(unsigned)(b + 1));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best = max(best, (unsigned long long)__shfl_xor((long long)best, o));
        if ((tid & 63) == 0) s_best[tid >> 6] = best;
        __syncthreads();
        for (int w = 0; w < CL_THREADS / 64; ++w) best = max(best, s_best[w]);
        if (best) {
            no = 1; total = (int)(best >> 32);
            if (tid == 0 && total <= p.max_pts) {
                bbase[(int)(best & 0xffffffffull) - 1] = 0;
                if (p.parts) p.parts[(size_t)mi * p.parts_cap + 1] = total;
            }
        }
    }
    if (tid == 0) {
        if (no == 0) cl_finish(p, mi, ws, 0);
        else if (total > p.max_pts) cl_finish(p, mi, ws, -2);
        else {
            p.count[mi] = total;
            if (p.parts) p.parts[(size_t)mi * p.parts_cap] = no;
        }
    }
}

__global__ __launch_bounds__(64) void cl_emit_kernel(const LargeParams p) {
    const int mi = blockIdx.y, k = blockIdx.x * 64 + threadIdx.x;
    int* ws = cl_ws(p, mi);
    if (ws[0] != CL_ST_RUN || k >= ws[1]) return;
    const int lead = ws[p.L.o_bid + k];
    if (lead < 0) return;
    const int e = ws[p.L.o_lnp + lead];
    if (!e) return;
    const int base = ws[p.L.o_bbase + ws[p.L.o_bno + lead]];
    if (base < 0) return;
    const int np = e >> 1, sk = e & 1;
    // clockwise index r of the contour (the start point first, when kept) -> its place in the list: the list runs the other way behind
    // the start point
    auto place = [&](int r) { return r >= np ? -1 : base + (r < sk ? r : sk + (np - 1 - r)); };
    int32_t* out = p.pts + (size_t)mi * p.max_pts * 2;
    const int lin = ws[p.L.o_cand + k];
    const int sy = lin / p.W, sx = lin - sy * p.W;
    const int rel = sk + ws[p.L.o_rel + k];
    if (k == lead && sk) { out[2 * base] = sx; out[2 * base + 1] = sy; }
    if (ws[p.L.o_jkp + k]) { const int at = place(rel - 1); if (at >= 0) { out[2 * at] = sx; out[2 * at + 1] = sy; } }
    if (ws[p.L.o_nkp + k] == 0) return;
    const LargeView v = cl_view(p, ws);
    LSeg si;
    cl_walk_segment<true>(v, sy, sx, 4 * p.H * p.W + 8, out, [&](int i) { return place(rel + i); }, si);
}

// ---- hull + calipers -----------------------------------------------------------------------------------------------------------------
constexpr int CL_HULL_LDS = (3 * CL_MAXDIM + 2 * (2 * CL_MAXDIM + 2) + 2 * (CL_MAXDIM + 2)) * (int)sizeof(int);

__global__ __launch_bounds__(CL_THREADS) void cl_hull_kernel(const LargeParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_xlo, s_xhi, s_chain_n[2], s_nuniq, s_first[2], s_last[2], s_nhull;
    const int mi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* ws = cl_ws(p, mi);
    const int st = ws[0];
    if (!p.rect || (st != CL_ST_RUN && st != CL_ST_RECT)) return;
    const int np = p.count[mi];
    if (np <= 0) { if (tid == 0) { p.rect[2 * mi] = 0.0; p.rect[2 * mi + 1] = 0.0; } return; }
    const int32_t* out = p.pts + (size_t)mi * p.max_pts * 2;
    int* colmin = (int*)smem;
    int* colmax = colmin + CL_MAXDIM;
    int* colx = colmax + CL_MAXDIM;             // the column's x as the rectangle sees it (scaled or not)
    int* hull = colx + CL_MAXDIM;               // up to 2 * W + 2 vertices, (x, y) interleaved; the lower chain is built in place
    int* chain_up = hull + 2 * (2 * CL_MAXDIM + 2);
    if (tid == 0) { s_xlo = p.W; s_xhi = -1; s_nhull = 0; }
    for (int i = tid; i < p.W; i += CL_THREADS) { colmin[i] = 0x7fffffff; colmax[i] = -1; }
    __syncthreads();
    for (int i = tid; i < np; i += CL_THREADS) {
        const int x = out[2 * i], y = out[2 * i + 1];
        if ((unsigned)x >= (unsigned)p.W) continue;                 // (cannot happen: the points are pixels of the mask)
        atomicMin(&colmin[x], y);
        atomicMax(&colmax[x], y);
    }
    __syncthreads();
    {
        int xl = p.W, xh = -1;
        for (int x = tid; x < p.W; x += CL_THREADS) {
            if (colmax[x] < 0) continue;
            xl = min(xl, x); xh = max(xh, x);
            if (p.scaled) {                                          // monotone per axis: the extremes stay the extremes
                colmin[x] = scale_coord(colmin[x], p.pady, p.gain, p.H0);
                colmax[x] = scale_coord(colmax[x], p.pady, p.gain, p.H0);
                colx[x] = scale_coord(x, p.padx, p.gain, p.W0);
            } else colx[x] = x;
        }
        if (xh >= 0) { atomicMin(&s_xlo, xl); atomicMax(&s_xhi, xh); }
    }
    __syncthreads();
    const int xlo = s_xlo, xhi = s_xhi;
    // Andrew's monotone chain over the groups of columns with one x, (x, lowest y) and (x, highest y) each, in (x, y) order: lower chain
    // left to right, upper chain right to left, pops on cross <= 0 - hostops._convex_hull on the unique points. Lane 0 of wave 0 builds the
    // lower chain, lane 0 of wave 1 the upper one, lane 0 of wave 2 counts the unique points; hull = lower[:-1] + upper[:-1].
    if (tid == 0 || tid == 64 || tid == 128) {
        const bool upper = tid == 64, count_only = tid == 128;
        int* const stk = upper ? chain_up : hull;
        int n = 0, ax = 0, ay = 0, bx = 0, by = 0;
        int nuniq = 0, fx = 0, fy = 0, gx = 0, gy = 0;
        auto push = [&](int qx, int qy) {
            while (n >= 2 && (long long)(bx - ax) * (qy - ay) - (long long)(by - ay) * (qx - ax) <= 0) {
                --n;
                bx = ax; by = ay;
                if (n >= 2) { ax = stk[2 * (n - 2)]; ay = stk[2 * (n - 2) + 1]; }
            }
            stk[2 * n] = qx; stk[2 * n + 1] = qy; ++n;
            ax = bx; ay = by; bx = qx; by = qy;
        };
        auto flush = [&](int x, int lo, int hi) {
            if (count_only) {
                if (nuniq == 0) { fx = x; fy = lo; }
                nuniq += (lo != hi) ? 2 : 1;
                gx = x; gy = hi;
            } else if (!upper) {
                push(x, lo);
                if (hi != lo) push(x, hi);
            } else {
                if (hi != lo) push(x, hi);
                push(x, lo);
            }
        };
        int cur = -1, lo = 0, hi = 0;
        const int step = upper ? -1 : 1;
        for (int x = upper ? xhi : xlo; x >= xlo && x <= xhi; x += step) {
            if (colmax[x] < 0) continue;
            const int sx = colx[x];
            if (sx != cur) {
                if (cur >= 0) flush(cur, lo, hi);
                cur = sx; lo = colmin[x]; hi = colmax[x];
            } else { lo = min(lo, colmin[x]); hi = max(hi, colmax[x]); }
        }
        if (cur >= 0) flush(cur, lo, hi);
        if (count_only) { s_nuniq = nuniq; s_first[0] = fx; s_first[1] = fy; s_last[0] = gx; s_last[1] = gy; }
        else s_chain_n[upper ? 1 : 0] = n;
    }
    __syncthreads();
    {
        const int nuniq = s_nuniq;
        if (nuniq <= 2) {
            if (tid == 0) {
                hull[0] = s_first[0]; hull[1] = s_first[1];
                if (nuniq == 2) { hull[2] = s_last[0]; hull[3] = s_last[1]; }
                s_nhull = nuniq < 2 ? 1 : 2;
            }
        } else {
            const int nlo = s_chain_n[0] - 1, nup = s_chain_n[1] - 1;     // lo[:-1], up[:-1]
            for (int i = tid; i < nup; i += CL_THREADS) { hull[2 * (nlo + i)] = chain_up[2 * i]; hull[2 * (nlo + i) + 1] = chain_up[2 * i + 1]; }
            if (tid == 0) s_nhull = nlo + nup;
        }
    }
    __syncthreads();
    const int nh = s_nhull;
    if (nh <= 2) {
        if (tid == 0) {
            double len = 0.0;
            if (nh == 2) { const double ddx = hull[2] - hull[0], ddy = hull[3] - hull[1]; len = hypot(ddx, ddy); }
            p.rect[2 * mi] = len; p.rect[2 * mi + 1] = 0.0;
        }
        return;
    }
    // rotating calipers: one hull edge per thread, float64 as hostops.min_area_rect_size; the smallest area wins, ties by the lower edge
    // index (the host loop keeps the first minimum)
    __shared__ double s_area[CL_THREADS / 64], s_w[CL_THREADS / 64], s_h[CL_THREADS / 64];
    __shared__ int s_idx[CL_THREADS / 64];
    double barea = 1e300, bwid = 0, bhei = 0;
    int bidx = 0x7fffffff;
    for (int i = tid; i < nh; i += CL_THREADS) {
        const int j = (i + 1 == nh) ? 0 : i + 1;
        const double ex = (double)(hull[2 * j] - hull[2 * i]), ey = (double)(hull[2 * j + 1] - hull[2 * i + 1]);
        const double nrm = hypot(ex, ey);
        const double ux = ex / nrm, uy = ey / nrm;
        const double vx = -uy, vy = ux;
        double amin = 1e300, amax = -1e300, bmin = 1e300, bmax = -1e300;
        for (int k = 0; k < nh; ++k) {
            const double hx = (double)hull[2 * k], hy = (double)hull[2 * k + 1];
            const double a = hx * ux + hy * uy, b = hx * vx + hy * vy;
            amin = fmin(amin, a); amax = fmax(amax, a); bmin = fmin(bmin, b); bmax = fmax(bmax, b);
        }
        const double w = amax - amin, h = bmax - bmin;
        if (w * h < barea || (w * h == barea && i < bidx)) { barea = w * h; bwid = w; bhei = h; bidx = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double oa = __shfl_xor(barea, o), ow = __shfl_xor(bwid, o), oh = __shfl_xor(bhei, o);
        const int oi = __shfl_xor(bidx, o);
        if (oa < barea || (oa == barea && oi < bidx)) { barea = oa; bwid = ow; bhei = oh; bidx = oi; }
    }
    if (lane == 0) { s_area[wave] = barea; s_w[wave] = bwid; s_h[wave] = bhei; s_idx[wave] = bidx; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < CL_THREADS / 64; ++k)
            if (s_area[k] < barea || (s_area[k] == barea && s_idx[k] < bidx)) { barea = s_area[k]; bwid = s_w[k]; bhei = s_h[k]; bidx = s_idx[k]; }
        p.rect[2 * mi] = fmax(bwid, bhei); p.rect[2 * mi + 1] = fmin(bwid, bhei);
    }
}

hipError_t launch_contours_large(const uint8_t* masks, int n, int H, int W, int strategy, int max_pts, int32_t* pts, int32_t* count, int32_t* parts,
                                 int parts_cap, double* rect, int H0, int W0, int flags, void* workspace, hipStream_t st) {
#pragma clang fp contract(off)
    if (n == 0) return hipSuccess;
    LargeParams p{};
    p.masks = masks; p.n = n; p.H = H; p.W = W; p.max_pts = max_pts; p.pts = pts; p.count = count; p.strategy = strategy;
    p.parts = parts; p.parts_cap = parts ? parts_cap : 0; p.rect = rect; p.flags = flags;
    p.ws = (int*)workspace;
    p.L = contours_large_layout(H, W);
    if (H0 > 0) {
        // hostops.scale_coords: gain and pads in double (Python floats), rounded to float32 where numpy meets the float32 polygon
        const double gain = std::min((double)H / H0, (double)W / W0);
        const double wg = W0 * gain, hg = H0 * gain;
        p.scaled = 1; p.H0 = H0; p.W0 = W0;
        p.gain = (float)gain; p.padx = (float)((W - wg) / 2); p.pady = (float)((H - hg) / 2);
    }
    static size_t granted = 0;
    if (hipError_t e = allow_dynamic_lds((const void*)cl_hull_kernel, (size_t)CL_HULL_LDS, granted)) return e;
    const unsigned cg = (unsigned)((p.L.candcap + 63) / 64);
    hipLaunchKernelGGL(cl_init_kernel, dim3((n + 255) / 256), dim3(256), 0, st, p);
    hipLaunchKernelGGL(cl_bits_kernel, dim3((unsigned)((p.L.nwords + 255) / 256), n), dim3(256), 0, st, p);
    hipLaunchKernelGGL(cl_candrow_kernel, dim3(H, n), dim3(256), 0, st, p);
    hipLaunchKernelGGL(cl_scan_kernel, dim3(n), dim3(CL_THREADS), 0, st, p);
    hipLaunchKernelGGL(cl_candlist_kernel, dim3(H, n), dim3(256), 0, st, p);
    hipLaunchKernelGGL(cl_trace_kernel, dim3(cg, n), dim3(64), 0, st, p);
    hipLaunchKernelGGL(cl_cycles_kernel, dim3(cg, n), dim3(64), 0, st, p);
    hipLaunchKernelGGL(cl_order1_kernel, dim3(n), dim3(CL_THREADS), 0, st, p);
    hipLaunchKernelGGL(cl_nest_kernel, dim3(cg, n), dim3(64), 0, st, p);
    hipLaunchKernelGGL(cl_order2_kernel, dim3(n), dim3(CL_THREADS), 0, st, p);
    hipLaunchKernelGGL(cl_emit_kernel, dim3(cg, n), dim3(64), 0, st, p);
    if (rect) hipLaunchKernelGGL(cl_hull_kernel, dim3(n), dim3(CL_THREADS), CL_HULL_LDS, st, p);
    return hipGetLastError();
}

}  // namespace yp
