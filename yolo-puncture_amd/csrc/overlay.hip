// The app's output frame on the device over a whole clip (yp_overlay_frames): loop #2 of the reference's video path pastes the U^2-Net
// crop mask into a zero H x W x 3 image, draws the ROI rectangle and the label into a second one (create_roi_mask,
// yolo_seg/utils/mask_tools.py:100-129) and adds both to the frame with two saturating cv2.addWeighted calls (yolo_seg/app.py:179-190).
// All terms are non-negative, so per byte
//     out = min(255, frame + M + R[c])
// with M the crop-mask byte inside the window (the same for the three channels, added as it is), R[c] = max(band ? col[c] : 0,
// (cov * col[c] + 127) / 255), band the thickness-2 rectangle and cov the label bitmap's coverage byte (hostops.overlay_frame is the
// numpy statement of the same arithmetic, with the band's pixel set written out).
//
// A frame is a byte stream of H*W*3 bytes whose first byte has any alignment. Its aligned body is cut into 16-byte vectors; vector v
// starts at channel (16 v + head) % 3 of pixel (16 v + head) / 3 and meets at most six pixels. The value to add is built for those six
// pixels as 18 bytes in five dwords, moved to the vector's phase with v_alignbyte, and added with a four-bytes-at-once saturating add, so
// that every global access is one aligned 16-byte load or store whatever W, H*W*3 and the base address are. The head before the first
// aligned byte and the tail after the last whole vector (fewer than 16 bytes each) go bytewise.
//   copy form (dst != src):  every vector of every frame is loaded once and stored once, lane-contiguous; a vector that meets none of the
//                            frame's six region rectangles (window, four band strips, label) is stored as loaded.
//   in-place form (dst == src): work items are (rectangle, row, vector of that row's byte span); an item does the read-modify-write
//                            only when it is the first (rectangle, row) that the vector's pixels meet, so a vector shared by two rows or two
//                            rectangles is still updated once.
#include "../../include/yolop.h"
#include "common.h"
#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>

extern "C" int yp_fail_public(int code, const char* msg);
static int ovfail(int code, const char* fmt, ...) {
    char buf[400];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return yp_fail_public(code, buf);
}
#define OVHIP(x)                                                                                                   \
    do {                                                                                                           \
        hipError_t _e = (x);                                                                                       \
        if (_e != hipSuccess) return ovfail(YP_ERR_HIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

namespace {

constexpr int OV_RECTS = 6;                       // window, band top / bottom / left / right, label
constexpr int OV_FRAMES = 64;                     // frames per launch: their rows travel as kernel arguments (64 x 52 bytes of the 4 KiB)
// one row of the caller's table (YP_OVERLAY_PARAMS ints)
struct OvPar {
    int x_lt, y_lt, x_rd, y_rd;                   // mask window, half open
    int x1, y1, x2, y2;                           // roi corners, both on the outline
    int lx, ly, lw, lh;                           // label bitmap: top-left in the frame, used width and height (0 = no label)
    int crop;                                     // index of the frame's crop in masks
};
static_assert(sizeof(OvPar) == YP_OVERLAY_PARAMS * sizeof(int), "OvPar is the caller's row");
// what both sides derive from a row: the frame's six region rectangles and, for the in-place form, the work items of each
struct OvRects {
    int rect[OV_RECTS][4];                        // (xa, ya, xb, yb) inclusive and clipped to the frame; xa > xb when empty
    int first[OV_RECTS + 1];                      // first work item of each rectangle, [OV_RECTS] = items of the frame
};

struct OvArgs {
    const uint8_t* src;
    uint8_t* dst;
    const uint8_t* masks;
    const uint8_t* labels;
    long frame_bytes;                             // H * W * 3
    int H, W, ch, cw, LH, LW;
    unsigned long long inv_w;                     // ceil(2^40 / W): p / W == (p * inv_w) >> 40 for p * W < 2^40 (checked on the host)
    unsigned col;                                 // col[0] | col[1] << 8 | col[2] << 16
    OvPar par[OV_FRAMES];                         // frame blockIdx.z of this launch
};
static_assert(sizeof(OvArgs) <= 4096, "kernel arguments");

__host__ __device__ inline int imin(int a, int b) { return a < b ? a : b; }
__host__ __device__ inline int imax(int a, int b) { return a > b ? a : b; }

__host__ __device__ inline void put_rect(int* r, int xa, int ya, int xb, int yb, int H, int W) {
    xa = imax(xa, 0); ya = imax(ya, 0); xb = imin(xb, W - 1); yb = imin(yb, H - 1);
    const bool empty = xa > xb || ya > yb;
    r[0] = empty ? 1 : xa; r[1] = empty ? 1 : ya; r[2] = empty ? 0 : xb; r[3] = empty ? 0 : yb;
}

// vectors one row of a rectangle can meet: its span of bytes plus one vector for each end that is not aligned
__host__ __device__ inline int rect_row_vectors(const int* r) { return r[0] > r[2] ? 0 : ((r[2] - r[0] + 1) * 3 + 15) / 16 + 1; }

__host__ __device__ inline void derive_rects(const OvPar& p, int H, int W, OvRects& o) {
    put_rect(o.rect[0], p.x_lt, p.y_lt, p.x_rd - 1, p.y_rd - 1, H, W);
    put_rect(o.rect[1], p.x1 - 1, p.y1 - 1, p.x2 + 1, p.y1 + 1, H, W);
    put_rect(o.rect[2], p.x1 - 1, p.y2 - 1, p.x2 + 1, p.y2 + 1, H, W);
    put_rect(o.rect[3], p.x1 - 1, p.y1 - 1, p.x1 + 1, p.y2 + 1, H, W);
    put_rect(o.rect[4], p.x2 - 1, p.y1 - 1, p.x2 + 1, p.y2 + 1, H, W);
    const bool lab = p.lw > 0 && p.lh > 0;
    put_rect(o.rect[5], lab ? p.lx : 1, lab ? p.ly : 1, lab ? p.lx + p.lw - 1 : 0, lab ? p.ly + p.lh - 1 : 0, H, W);
    int n = 0;                                    // < 6 * H * (W * 3 / 16 + 2) < 2^31 while H * W * 3 < 2^31
#pragma unroll
    for (int k = 0; k < OV_RECTS; ++k) {
        o.first[k] = n;
        n += (o.rect[k][3] - o.rect[k][1] + 1) * rect_row_vectors(o.rect[k]);       // an empty rectangle has yb - ya + 1 = 0 rows
    }
    o.first[OV_RECTS] = n;
}

// ---- device side ----------------------------------------------------------------------------------------------------------------------
struct Px { int y, x; };

__device__ __forceinline__ Px px_of(unsigned p, const OvArgs& a) {
    const unsigned y = (unsigned)(((unsigned long long)p * a.inv_w) >> 40);
    return Px{(int)y, (int)(p - y * (unsigned)a.W)};
}

// M + R[c] for the three channels of one pixel, each already clamped to 255, packed B | G << 8 | R << 16
__device__ __forceinline__ unsigned px_add(int y, int x, const OvPar& p, const OvArgs& a) {
    if (y >= a.H) return 0u;                       // a vector's six pixels may run past the frame's last one
    unsigned m = 0, cov = 0;
    if (x >= p.x_lt && x < p.x_rd && y >= p.y_lt && y < p.y_rd)
        m = a.masks[((size_t)p.crop * a.ch + (y - p.y_lt)) * a.cw + (x - p.x_lt)];
    const bool band = x >= p.x1 - 1 && x <= p.x2 + 1 && y >= p.y1 - 1 && y <= p.y2 + 1 &&
                      !(x >= p.x1 + 2 && x <= p.x2 - 2 && y >= p.y1 + 2 && y <= p.y2 - 2);
    const int u = x - p.lx, v = y - p.ly;
    if (u >= 0 && u < p.lw && v >= 0 && v < p.lh) cov = a.labels[((size_t)blockIdx.z * a.LH + v) * a.LW + u];
    unsigned out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned cc = (a.col >> (8 * c)) & 255u;
        const unsigned r = max(band ? cc : 0u, (cov * cc + 127u) / 255u);
        out |= min(255u, m + r) << (8 * c);
    }
    return out;
}

// four bytes at once: min(255, a + b) per byte
__device__ __forceinline__ unsigned sat_add_u8x4(unsigned a, unsigned b) {
    const unsigned low = (a & 0x7f7f7f7fu) + (b & 0x7f7f7f7fu);
    const unsigned sum = low ^ ((a ^ b) & 0x80808080u);
    const unsigned carry = ((a & b) | ((a | b) & ~sum)) & 0x80808080u;
    return sum | ((carry >> 7) * 255u);
}

__device__ __forceinline__ bool meets(const int* r, int xa, int ya, int xb, int yb) {
    return xb >= r[0] && xa <= r[2] && yb >= r[1] && ya <= r[3];
}

// does the run of pixels from q0 to q1 (row-major order, both in the frame) meet one of the rectangles? Exact within one row and over
// two rows; over more rows the run counts as full rows.
__device__ __forceinline__ bool run_meets(const OvRects& o, Px q0, Px q1, int W) {
    bool hit = false;
    if (q0.y == q1.y) {
#pragma unroll
        for (int r = 0; r < OV_RECTS; ++r) hit |= meets(o.rect[r], q0.x, q0.y, q1.x, q0.y);
    } else if (q0.y + 1 == q1.y) {
#pragma unroll
        for (int r = 0; r < OV_RECTS; ++r) hit |= meets(o.rect[r], q0.x, q0.y, W - 1, q0.y) || meets(o.rect[r], 0, q1.y, q1.x, q1.y);
    } else {
#pragma unroll
        for (int r = 0; r < OV_RECTS; ++r) hit |= meets(o.rect[r], 0, q0.y, W - 1, q1.y);
    }
    return hit;
}

// the sixteen bytes to add to the vector whose first byte is byte b of the frame
__device__ __forceinline__ uint4 vector_add(unsigned b, const OvPar& p, const OvArgs& a) {
    const unsigned p0 = b / 3u, ph = b - 3u * p0;
    Px q = px_of(p0, a);
    unsigned t[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        t[k] = px_add(q.y, q.x, p, a);
        if (++q.x == a.W) { q.x = 0; ++q.y; }
    }
    // 18 bytes B G R B G R ... as five dwords, then shifted down by the phase
    const unsigned s0 = t[0] | (t[1] << 24), s1 = (t[1] >> 8) | (t[2] << 16), s2 = (t[2] >> 16) | (t[3] << 8);
    const unsigned s3 = t[4] | (t[5] << 24), s4 = t[5] >> 8;
    uint4 r;
    r.x = __builtin_amdgcn_alignbyte(s1, s0, ph);
    r.y = __builtin_amdgcn_alignbyte(s2, s1, ph);
    r.z = __builtin_amdgcn_alignbyte(s3, s2, ph);
    r.w = __builtin_amdgcn_alignbyte(s4, s3, ph);
    return r;
}

// edge byte e of the frame (the head's bytes first, then the tail's), one byte per lane
__device__ __forceinline__ void edge_byte(const uint8_t* src, uint8_t* dst, long e, long head, long body_end, bool inplace,
                                          const OvPar& p, const OvArgs& a) {
    const unsigned b = (unsigned)(e < head ? e : body_end + (e - head));
    const unsigned p0 = b / 3u, c = b - 3u * p0;
    const Px q = px_of(p0, a);
    const unsigned add = (px_add(q.y, q.x, p, a) >> (8 * c)) & 255u;
    if (!inplace || add) dst[b] = (uint8_t)min(255u, (unsigned)src[b] + add);
}

// head bytes before the first 16-byte boundary of dst and the count of whole vectors after them; a frame whose src and dst differ in
// alignment has no vector body and goes bytewise as a whole
__device__ __forceinline__ void frame_split(const uint8_t* src, const uint8_t* dst, long frame_bytes, long& head, long& nvec) {
    head = (long)((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u);
    if (head > frame_bytes) head = frame_bytes;
    nvec = (frame_bytes - head) / 16;
    if (((uintptr_t)src ^ (uintptr_t)dst) & 15u) { head = frame_bytes; nvec = 0; }
}

constexpr int OV_UNROLL = 4;

// does the run of frame bytes from byte x0 of row y0 to byte x1 of row y1 meet one of the rectangles? Exact within one row; over more
// rows the run counts as full rows (it then takes the per-vector test, which is exact).
__device__ __forceinline__ bool span_meets(const OvRects& o, int y0, int x0, int y1, int x1) {
    bool hit = false;
#pragma unroll
    for (int r = 0; r < OV_RECTS; ++r) {
        const int* q = o.rect[r];
        hit |= y0 == y1 ? (y0 >= q[1] && y0 <= q[3] && x1 >= q[0] * 3 && x0 <= q[2] * 3 + 2) : (q[0] <= q[2] && y1 >= q[1] && y0 <= q[3]);
    }
    return hit;
}

__global__ __launch_bounds__(256) void overlay_copy_kernel(OvArgs a) {
    const OvPar& p = a.par[blockIdx.z];
    OvRects o;
    derive_rects(p, a.H, a.W, o);
    const uint8_t* src = a.src + (size_t)blockIdx.z * a.frame_bytes;
    uint8_t* dst = a.dst + (size_t)blockIdx.z * a.frame_bytes;
    long head, nvec;
    frame_split(src, dst, a.frame_bytes, head, nvec);
    const uint4* sv = reinterpret_cast<const uint4*>(src + head);
    uint4* dv = reinterpret_cast<uint4*>(dst + head);
    const int lane = threadIdx.x & 63;
    // A wave's 64 vectors are 1 KiB of the frame. Whether that span meets a region is one test on the scalar unit, in (row, byte of the
    // row) coordinates that advance by a constant from one span of the wave to its next: most waves copy and compute nothing per lane.
    const int pitch = a.W * 3;
    const int step = (int)(gridDim.x * blockDim.x);                                 // vectors between a wave's consecutive spans
    const int step_y = (16 * step) / pitch, step_x = 16 * step - step_y * pitch;
    const int span_y = 1023 / pitch, span_x = 1023 - span_y * pitch;
    int wv = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * blockDim.x + threadIdx.x) - lane);      // the wave's first vector (nvec < 2^27)
    const int nv = (int)nvec;
    const int wb = (int)head + 16 * wv;
    int wy = wb / pitch, wx = wb - wy * pitch;
    while (wv < nv) {
        uint4 d[OV_UNROLL];
#pragma unroll
        for (int k = 0; k < OV_UNROLL; ++k)
            if (wv + k * step + lane < nv) d[k] = sv[wv + k * step + lane];
#pragma unroll
        for (int k = 0; k < OV_UNROLL; ++k) {
            const int v = wv + k * step + lane;
            int ey = wy + span_y, ex = wx + span_x;
            if (ex >= pitch) { ex -= pitch; ++ey; }
            if (wv + k * step < nv && span_meets(o, wy, wx, ey, ex) && v < nv) {
                const unsigned b = (unsigned)(head + 16 * v);
                if (run_meets(o, px_of(b / 3u, a), px_of((b + 15u) / 3u, a), a.W)) {
                    const uint4 add = vector_add(b, p, a);
                    d[k].x = sat_add_u8x4(d[k].x, add.x); d[k].y = sat_add_u8x4(d[k].y, add.y);
                    d[k].z = sat_add_u8x4(d[k].z, add.z); d[k].w = sat_add_u8x4(d[k].w, add.w);
                }
            }
            if (v < nv) dv[v] = d[k];
            wy += step_y; wx += step_x;
            if (wx >= pitch) { wx -= pitch; ++wy; }
        }
        wv += OV_UNROLL * step;
    }
    const long n_edge = a.frame_bytes - 16 * nvec;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n_edge; e += step) edge_byte(src, dst, e, head, head + 16 * nvec, false, p, a);
}

__global__ __launch_bounds__(256) void overlay_inplace_kernel(OvArgs a) {
    const OvPar& p = a.par[blockIdx.z];
    OvRects o;
    derive_rects(p, a.H, a.W, o);
    uint8_t* dst = a.dst + (size_t)blockIdx.z * a.frame_bytes;
    long head, nvec;
    frame_split(dst, dst, a.frame_bytes, head, nvec);
    uint4* dv = reinterpret_cast<uint4*>(dst + head);
    if (blockIdx.x == 0)                          // one block takes the at most 30 edge bytes
        for (long e = threadIdx.x; e < a.frame_bytes - 16 * nvec; e += blockDim.x) edge_byte(dst, dst, e, head, head + 16 * nvec, true, p, a);
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= o.first[OV_RECTS]) return;
    // the item's rectangle: the last one that starts at or before it (an empty rectangle starts where the next one does)
    int r = 0, xa = o.rect[0][0], ya = o.rect[0][1], xb = o.rect[0][2], base = 0;
#pragma unroll
    for (int k = 1; k < OV_RECTS; ++k)
        if (item >= o.first[k]) { r = k; xa = o.rect[k][0]; ya = o.rect[k][1]; xb = o.rect[k][2]; base = o.first[k]; }
    const int per_row = ((xb - xa + 1) * 3 + 15) / 16 + 1;
    const int local = item - base;
    const int y = ya + local / per_row, i = local - (local / per_row) * per_row;
    // the row's byte span [b0, b1] of the frame, and the vectors it meets
    const long b0 = ((long)y * a.W + xa) * 3, b1 = ((long)y * a.W + xb) * 3 + 2;
    if (b1 < head) return;
    const long va = b0 < head ? 0 : (b0 - head) / 16, v = va + i;
    if (v >= nvec || head + 16 * v > b1) return;
    // owner = the first (rectangle, row) among those that the vector's pixels lie in
    const unsigned b = (unsigned)(head + 16 * v);
    const unsigned pa = b / 3u, pb = (b + 15u) / 3u;
    Px q = px_of(pa, a);
    long best = (long)OV_RECTS << 32;
    for (unsigned k = pa; k <= pb; ++k) {
        if (q.y < a.H) {
#pragma unroll
            for (int s = 0; s < OV_RECTS; ++s)
                if (meets(o.rect[s], q.x, q.y, q.x, q.y)) {
                    const long key = ((long)s << 32) | (long)q.y;
                    best = key < best ? key : best;
                }
        }
        if (++q.x == a.W) { q.x = 0; ++q.y; }
    }
    if (best != (((long)r << 32) | (long)y)) return;
    const uint4 add = vector_add(b, p, a);
    if ((add.x | add.y | add.z | add.w) == 0u) return;
    uint4 d = dv[v];
    d.x = sat_add_u8x4(d.x, add.x); d.y = sat_add_u8x4(d.y, add.y);
    d.z = sat_add_u8x4(d.z, add.z); d.w = sat_add_u8x4(d.w, add.w);
    dv[v] = d;
}

}  // namespace

extern "C" {

int yp_overlay_frames(const uint8_t* src_dev, uint8_t* dst_dev, int n, int H, int W, const uint8_t* masks_dev, int B, int ch, int cw,
                      const int32_t* params, const uint8_t* labels_dev, int LH, int LW, const uint8_t* col, void* stream) {
    // every argument is checked before the device is touched
    if (n < 0) return ovfail(YP_ERR_ARG, "yp_overlay_frames: n = %d is negative", n);
    if (n == 0) return YP_OK;
    if (!src_dev || !dst_dev || !params) return ovfail(YP_ERR_ARG, "yp_overlay_frames: null argument");
    if (H <= 0 || W <= 0) return ovfail(YP_ERR_ARG, "yp_overlay_frames: frames must be [n,H,W,3] with H,W >= 1 (got %d,%d)", H, W);
    const long frame_bytes = (long)H * W * 3;
    // px_of: (p * inv_w) >> 40 is p / W while p * W < 2^40, and p * inv_w stays below 2^64 while H < 2^22 (p runs a few pixels past H * W)
    if (frame_bytes >= (1l << 31) || ((long)H * W + 8) * W >= (1l << 40) || H >= (1 << 22))
        return ovfail(YP_ERR_ARG, "yp_overlay_frames: a %dx%d frame is too large (H*W*3 < 2^31, H*W*W < 2^40, H < 2^22)", H, W);
    if (B < 0 || ch < 0 || cw < 0 || LH < 0 || LW < 0)
        return ovfail(YP_ERR_ARG, "yp_overlay_frames: negative size (B %d, crop %dx%d, label %dx%d)", B, ch, cw, LH, LW);
    if (B > 0 && !masks_dev) return ovfail(YP_ERR_ARG, "yp_overlay_frames: %d crops but no masks", B);
    const uint8_t* s_end = src_dev + (size_t)n * frame_bytes;
    const uint8_t* d_end = dst_dev + (size_t)n * frame_bytes;
    if (src_dev != dst_dev && src_dev < d_end && dst_dev < s_end)
        return ovfail(YP_ERR_ARG, "yp_overlay_frames: src and dst overlap without being equal");
    constexpr int LIM = 1 << 24;
    for (int f = 0; f < n; ++f) {
        const int32_t* q = params + (size_t)f * YP_OVERLAY_PARAMS;
        const bool empty = q[0] == q[2] || q[1] == q[3];
        if (q[0] < 0 || q[1] < 0 || q[2] > W || q[3] > H || q[2] < q[0] || q[3] < q[1])
            return ovfail(YP_ERR_ARG, "yp_overlay_frames: frame %d: window (%d,%d,%d,%d) leaves the %dx%d frame", f, q[0], q[1], q[2], q[3], W, H);
        if (!empty && (q[2] - q[0] > cw || q[3] - q[1] > ch))
            return ovfail(YP_ERR_ARG, "yp_overlay_frames: frame %d: window (%d,%d,%d,%d) is larger than the %dx%d crop", f, q[0], q[1], q[2], q[3], cw, ch);
        if (!empty && (q[12] < 0 || q[12] >= B))
            return ovfail(YP_ERR_ARG, "yp_overlay_frames: frame %d: crop index %d outside [0,%d)", f, q[12], B);
        if (q[6] < q[4] || q[7] < q[5])
            return ovfail(YP_ERR_ARG, "yp_overlay_frames: frame %d: roi (%d,%d,%d,%d) has x2 < x1 or y2 < y1", f, q[4], q[5], q[6], q[7]);
        for (int k = 4; k < 10; ++k)
            if (q[k] < -LIM || q[k] > LIM) return ovfail(YP_ERR_ARG, "yp_overlay_frames: frame %d: coordinate %d outside +-2^24", f, q[k]);
        if (q[10] < 0 || q[11] < 0 || q[10] > LW || q[11] > LH)
            return ovfail(YP_ERR_ARG, "yp_overlay_frames: frame %d: label %dx%d outside the %dx%d bitmap", f, q[10], q[11], LW, LH);
        if (q[10] > 0 && q[11] > 0 && !labels_dev) return ovfail(YP_ERR_ARG, "yp_overlay_frames: frame %d has a label but labels is null", f);
    }

    hipStream_t st = (hipStream_t)stream;
    OvArgs a;
    a.masks = masks_dev;
    a.frame_bytes = frame_bytes;
    a.H = H; a.W = W; a.ch = ch; a.cw = cw; a.LH = LH; a.LW = LW;
    a.inv_w = ((1ull << 40) + (unsigned long long)W - 1) / (unsigned long long)W;
    a.col = col ? ((unsigned)col[0] | ((unsigned)col[1] << 8) | ((unsigned)col[2] << 16)) : (255u << 16);
    // the rows travel with the launch, OV_FRAMES frames at a time: nothing is staged, so the call neither waits nor keeps state
    for (int f0 = 0; f0 < n; f0 += OV_FRAMES) {
        const int nf = std::min(OV_FRAMES, n - f0);
        a.src = src_dev + (size_t)f0 * frame_bytes;
        a.dst = dst_dev + (size_t)f0 * frame_bytes;
        a.labels = labels_dev ? labels_dev + (size_t)f0 * LH * LW : nullptr;
        int items = 0;
        for (int f = 0; f < nf; ++f) {
            OvPar& r = a.par[f];
            memcpy(&r, params + (size_t)(f0 + f) * YP_OVERLAY_PARAMS, sizeof(OvPar));
            if (r.x_lt == r.x_rd || r.y_lt == r.y_rd) { r.x_rd = r.x_lt; r.y_rd = r.y_lt; r.crop = 0; }
            OvRects o;
            derive_rects(r, H, W, o);
            items = std::max(items, o.first[OV_RECTS]);
        }
        if (src_dev == dst_dev) {
            // launched over the regions: the widest frame of the launch sets the grid, the others' surplus items return at once
            const int gx = std::max(1, (items + 255) / 256);
            hipLaunchKernelGGL(overlay_inplace_kernel, dim3(gx, 1, nf), dim3(256), 0, st, a);
        } else {
            // memory bound: about 2048 blocks in all, each lane four vectors per turn, the rest by grid stride
            // (as many blocks as give each the same number of turns)
            const long turns = (frame_bytes / 16 + 256 * OV_UNROLL - 1) / (256 * OV_UNROLL);
            const long cap = std::max(8, 2048 / nf), per_block = (turns + cap - 1) / cap;
            const int gx = (int)std::max(1l, (turns + std::max(1l, per_block) - 1) / std::max(1l, per_block));
            hipLaunchKernelGGL(overlay_copy_kernel, dim3(gx, 1, nf), dim3(256), 0, st, a);
        }
        OVHIP(hipGetLastError());
    }
    return YP_OK;
}

}  // extern "C"
