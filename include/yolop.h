/* yolop.h - C-ABI of libyolop.so: the MI355X-native YOLOv10 predict hot path.
 *
 * The reference (daisy9542/yolo-puncture) has NO native/FFI layer for this path: its boundary is the Python call
 * `ultralytics.YOLO(path).predict(source, conf=, retina_masks=, device=)` (yolo_seg/app.py:45,49,91;
 * yolo_seg/yolo_with_deva.py:51,226; dev_tools/auto_speed_calc.py:40,62;
 * dev_tools/classify/cls_bbox_dataset_generate.py:48,66). Each entry point below names the part of that call
 * it replaces. The Python facade in yolo-puncture_amd/predictor.py binds these with ctypes.
 *
 * Conventions: every function returns 0 on success, <0 on error; yp_last_error() returns a thread-local
 * message. All device pointers are raw HIP device addresses owned by the CALLER (PyTorch tensors'
 * data_ptr()); the engine owns packed weights + its activation workspace. Work is enqueued on the stream
 * passed in (a hipStream_t cast to void*; NULL = default stream) with no hidden synchronisation.
 * An engine is bound to one device and is not re-entrant: one engine per GPU, one caller thread at a time.
 */
#ifndef YOLOP_H
#define YOLOP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YP_OK 0
#define YP_ERR_ARG -1      /* bad argument / shape                */
#define YP_ERR_STATE -2    /* call order (e.g. forward before finalize) */
#define YP_ERR_HIP -3      /* a HIP runtime call failed           */
#define YP_ERR_WEIGHT -4   /* unknown / missing / mis-shaped weight */

#define YP_BF16 0          /* activations+weights bf16 in HBM, fp32 accumulate (MFMA 16x16x32 bf16) */
#define YP_F32 1           /* everything fp32 (MFMA 16x16x4 f32): strict-parity mode               */

#define YP_TASK_DETECT 0
#define YP_TASK_SEGMENT 1

#define YP_NM 32           /* mask coefficients per detection */
#define YP_MAX_MASKS 480   /* masks per yp_masks / yp_id_mask_resized call (one frame's coefficients stay in LDS); a YP_TASK_SEGMENT engine
                              therefore takes max_det <= 480 - yp_create refuses more (ultralytics' default, and what every caller of the
                              reference leaves in place, is 300: yolo_seg/app.py:91, yolo_seg/yolo_with_deva.py:51) */
#define YP_ID_MASKS_FRAMES_BUDGET (1ull << 30)   /* bytes of workspace one yp_id_masks_frames call may ask of the engine before the Python facade
                                                    splits a chunk's frames over several calls (hostops.group_frames_by_workspace) */
#define YP_MAX_DET 512     /* rows per image the top-k and NMS head kernels rank in one step (csrc: MAXK, NMAXK, HEAD_MAXK) */

typedef struct yp_engine yp_engine;

/* What `YOLO(path)` learns from the checkpoint's yaml: which graph to build. */
typedef struct yp_model_desc {
    int variant; /* ASCII 'n','s','m','b','l','x'                                */
    int nc;      /* number of classes                                             */
    int task;    /* YP_TASK_DETECT | YP_TASK_SEGMENT (v10 trunk + Proto/cv4 head) */
    int dtype;   /* YP_BF16 | YP_F32                                              */
    int max_det; /* 300 (ultralytics default); top-k size of the one-to-one head and row cap of the NMS head; <= YP_MAX_DET (detect),
                    <= YP_MAX_MASKS (segment); yp_create refuses more */
    int family;  /* YP_FAMILY_V10 (0) | YP_FAMILY_V8 | YP_FAMILY_11: which ultralytics yaml the graph follows. The v8 / 11
                    families (the checkpoints the reference's UI offers, yolo_seg/app.py:218-223) are segment models: task must
                    be YP_TASK_SEGMENT; their head ends in conf filter + NMS (yp_set_nms) instead of the v10 top-k */
} yp_model_desc;

#define YP_FAMILY_V10 0
#define YP_FAMILY_V8 8
#define YP_FAMILY_11 11

const char* yp_last_error(void);

/* -- construction: replaces `YOLO(path)` (yolo_seg/app.py:45). Builds the op graph on the host; touches no GPU
 *    state, so it also works (for inspection) on a box without a GPU. device = HIP ordinal used later. */
int yp_create(const yp_model_desc* desc, int device, yp_engine** out);
int yp_destroy(yp_engine* e);

/* The folded (Conv+BN merged) parameters the graph expects, e.g. "model.0.weight" [32,3,3,3], "model.0.bias" [32]. */
int yp_weight_count(const yp_engine* e);
int yp_weight_info(const yp_engine* e, int i, char* name, int name_cap, int64_t shape[4], int* ndim);

/* Hand one folded fp32 parameter (HOST pointer) to the engine; it is repacked to the kernel layout
 * ([Cout][ky][kx][Cin], K padded) in the engine dtype. Replaces the state-dict load inside YOLO(path). */
int yp_set_weight(yp_engine* e, const char* name, const float* host, const int64_t* shape, int ndim);

/* Verify every parameter was set, upload packed weights to the device. After this the engine can run. */
int yp_finalize(yp_engine* e);

/* -- the forward + NMS-free post-process: replaces predictor inference + `v10postprocess` inside
 *    `.predict(...)` (yolo_seg/app.py:91). in_dev: uint8 NHWC **BGR**, already letterboxed, [B,H,W,3], H and W
 *    multiples of 32. Outputs (device, caller-owned):
 *      det_out   float [B,max_det,6] = x1,y1,x2,y2 (letterboxed-input pixels), score, class; rows sorted by
 *                score descending, ties by (stage-1 rank, class) ascending
 *      idx_out   int32 [B,max_det] anchor index of each row (may be NULL)
 *      coeff_out float [B,max_det,32] mask coefficients of each row (segment task; may be NULL)
 *    If the image has fewer than max_det anchors, k = #anchors rows are valid and the rest are zero. */
int yp_forward(yp_engine* e, const uint8_t* in_dev, int B, int H, int W, float* det_out, int32_t* idx_out,
               float* coeff_out, void* stream);

/* Engine-owned prototype tensor of the last forward (segment task): NHWC [B,Hp,Wp,32] in the engine dtype. */
int yp_proto(const yp_engine* e, const void** proto_dev, int* Hp, int* Wp);

/* -- segmentation tail: replaces ops.process_mask_native / process_mask + the id painting loop of
 *    `auto_segment` (yolo_seg/yolo_with_deva.py:54-86).
 *    image b of the last forward; n rows of coeff [n,32] (device float) and boxes [n,4] (device float):
 *    retina != 0: boxes in ORIGINAL-image pixels, masks at (oh,ow)      (process_mask_native)
 *    retina == 0: boxes in letterboxed-input pixels, masks at (oh,ow)=(H,W) of the forward (process_mask)
 *    masks_out: uint8 [n,oh,ow] in {0,1} (may be NULL)
 *    id_out:    int64 [oh,ow] painted ids (may be NULL): rows in order, later overwrite earlier, rows whose
 *               area < min_area are skipped when suppress_small != 0, ids consecutive over kept rows
 *    kept_out:  int32 [n] id assigned to each row (0 = suppressed) (may be NULL; needs id_out)          */
int yp_masks(yp_engine* e, int b, const float* coeff_dev, const float* boxes_dev, int n, int oh, int ow,
             int retina, uint8_t* masks_out, int64_t* id_out, int32_t* kept_out, int suppress_small,
             int min_area, void* stream);

/* `auto_segment` as the reference normally calls it, with min_side > 0 (yolo_seg/yolo_with_deva.py:45-48,118,140): the frame is
 * shrunk before predict, so the masks come out at (oh,ow) = the shrunk frame and each FLOAT {0,1} mask is resized to the original
 * frame (rh,rw) with torchvision `F.resize` (:71-72: bilinear, align_corners=False, antialias) before the area test
 * `mask.sum() < MIN_AREA_THRESHOLD` (:75, on the resized float mask) and the paint `output_mask[mask > 0.5] = id` (:79).
 * The resize repeats torch's CPU kernel operation by operation (fp32 weights, horizontal pass first, fused multiply-adds), so the
 * many exact 0.5 ties of e.g. a 2:3 upscale fall on the same side. boxes in (oh,ow) pixels; id_out int64 [rh,rw]; kept_out int32 [n].
 * With (rh,rw) == (oh,ow) this is yp_masks(retina=1) with id_out. */
int yp_id_mask_resized(yp_engine* e, int b, const float* coeff_dev, const float* boxes_dev, int n, int oh, int ow, int rh,
                       int rw, int64_t* id_out, int32_t* kept_out, int suppress_small, int min_area, void* stream);

/* The clip form of `results[0].masks` for the app's best row (yolo_seg/app.py:91-101): one retina mask per selected image of the last
 * forward. Mask j is process_mask_native of the coefficient row coeff_dev + frame_idx[j] * coeff_row_stride against image frame_idx[j]'s
 * prototypes, byte-equal to yp_masks(e, frame_idx[j], that row, boxes_dev + 4j, 1, oh, ow, retina=1, ...).
 *    frame_idx_host int32 [k] host array, each in [0,B) of the last forward (gaps and repeats allowed); copied to the device in the call
 *    coeff_dev      float, row 0 of image 0 (e.g. yp_forward's coeff_out with coeff_row_stride = max_det * YP_NM)
 *    boxes_dev      float [k,4] x1,y1,x2,y2 in original-image (oh,ow) pixels
 *    masks_out      uint8 [k,oh,ow] {0,1}; every byte is written (0 outside the box); k*oh*ow < 2^31
 * Every argument is checked before anything is launched. */
int yp_masks_frames(yp_engine* e, const int32_t* frame_idx_host, int k, const float* coeff_dev, long coeff_row_stride,
                    const float* boxes_dev, int oh, int ow, uint8_t* masks_out, void* stream);
/* The same for `predict(frame, conf)` without retina_masks (dev_tools/auto_speed_calc.py:62): ultralytics' process_mask at the letterboxed
 * input size. Mask j is byte-equal to yp_masks(e, frame_idx[j], that row, boxes_dev + 4j, 1, oh, ow, retina=0, ...).
 *    boxes_dev  float [k,4] x1,y1,x2,y2 in letterboxed-input pixels (the forward's rows, before scale_boxes)
 *    (oh,ow)    the (H,W) of the last forward; masks_out uint8 [k,oh,ow] {0,1}, every byte written
 * Other arguments and checks as yp_masks_frames. */
int yp_masks_frames_input(yp_engine* e, const int32_t* frame_idx_host, int k, const float* coeff_dev, long coeff_row_stride,
                          const float* boxes_dev, int oh, int ow, uint8_t* masks_out, void* stream);

/* The clip form of `auto_segment` (yolo_seg/yolo_with_deva.py:37-88): ALL masks of k images of the last forward -> one id image per image.
 * Frame j owns rows row_off[j] .. row_off[j+1] of coeff_dev / boxes_dev (n_j = their number, 0 <= n_j <= YP_MAX_MASKS) and image
 * frame_idx[j]. Its ids_out[j] and kept_out[row_off[j] .. row_off[j+1]) are byte-equal to
 *     yp_masks(e, frame_idx[j], coeff_dev + 32 * row_off[j], boxes_dev + 4 * row_off[j], n_j, oh, ow, 1, NULL, ids, kept, ...)   (rh,rw) == (oh,ow)
 *     yp_id_mask_resized(e, frame_idx[j], the same rows, n_j, oh, ow, rh, rw, ids, kept, ...)                                   otherwise
 * (float areas closer to min_area than their double sums' rounding excepted, as between two runs of yp_id_mask_resized itself).
 *    frame_idx_host int32 [k] host, each in [0,B) of the last forward (gaps and repeats allowed); row_off_host int32 [k+1] host, row_off[0] = 0,
 *                   non-decreasing; both are copied to the device in the call. k >= 1
 *    coeff_dev      float [n_total,32], boxes_dev float [n_total,4] x1,y1,x2,y2 in (oh,ow) pixels, n_total = row_off[k] (NULL allowed when 0)
 *    (oh,ow)        the size the masks are made at (retina); (rh,rw) the size of the id images, resized as yp_id_mask_resized when it differs
 *    ids_out        int64 [k,rh,rw], every byte written - zeros for a frame without rows; kept_out int32 [n_total], every byte written
 * Limits: k <= 65535, n_total <= 65535, each of oh*ow, oh*rw, rh*rw below 2^31 and n_total times the largest of them below 2^32 (a plane is
 * indexed with 32 bits, rows and frames with 64), the 16x downscale limit of yp_id_mask_resized. Every argument is checked before anything
 * is launched; on an error code nothing is written. The workspace is the engine's (grown when needed, as for yp_masks);
 * yp_id_masks_frames_workspace is its size in bytes for the engine's current plan - host arithmetic, 0 for sizes the call refuses or
 * before a plan - so that a caller can split frames over calls (YP_ID_MASKS_FRAMES_BUDGET). */
int yp_id_masks_frames(yp_engine* e, const int32_t* frame_idx_host, const int32_t* row_off_host, int k, const float* coeff_dev,
                       const float* boxes_dev, int oh, int ow, int rh, int rw, int64_t* ids_out, int32_t* kept_out, int suppress_small,
                       int min_area, void* stream);
size_t yp_id_masks_frames_workspace(const yp_engine* e, int n_total, int k, int oh, int ow, int rh, int rw);

/* `results[0].masks.xy[i]` and `get_coord_min_rect_len(...)` on the device (yolo_seg/app.py:101-103, yolo_seg/utils/mask_tools.py:12-22;
 * [U] Masks.xy = masks2segments(strategy): cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE), then "all" (the 8.3.x line the app's
 * YOLO11 weights need: every contour, concatenated) or "largest" (8.0-8.2: the contour with the most points, the first of them on a tie);
 * get_coord_min_rect_len = cv2.minAreaRect of that polygon -> (long side, long/short)). Engine-free. Per mask (one workgroup): bit image
 * of the mask's bounding box in LDS, Moore trace of every blob's outer border, RETR_EXTERNAL by crossing parity (a blob inside a hole of
 * another blob is skipped), run end points, convex hull, rotating calipers. cv2 is not available to pin this against; the definitions are
 * written out in yolo-puncture_amd/hostops.py ("Masks.xy") and restated three ways in the tests: a contour starts at its blob's raster-first
 * pixel and runs down first (a filled rectangle: top-left, bottom-left, bottom-right, top-right); contours are listed bottom-up
 * (descending raster order of the start pixels).
 *    masks_dev uint8 [n,H,W] (non-zero = set)
 *    strategy  YP_CONTOURS_LARGEST or YP_CONTOURS_ALL
 *    pts_out   int32 [n,max_pts,2] (x,y) polygon in mask pixels       count_out int32 [n]: number of points; 0 = empty mask;
 *              -1 = bounding box larger than the LDS image (1280x720 fits), -2 = more than max_pts points / 4096 border starts / 64 outer
 *              borders: use yp_mask_contours_large (below), or the host path (hostops.mask_polygon)
 *    parts_out int32 [n,parts_cap] or NULL: [0] = contours in the list, [1 .. ] = their point counts in list order (as many as fit)
 *    rect_out  double [n,2] = (long side, short side) of the minimum-area rectangle of the polygon (may be NULL) */
#define YP_CONTOURS_LARGEST 0
#define YP_CONTOURS_ALL 1
int yp_mask_contours(const uint8_t* masks_dev, int n, int H, int W, int strategy, int max_pts, int32_t* pts_out, int32_t* count_out,
                     int32_t* parts_out, int parts_cap, double* rect_out, void* stream);
/* yp_mask_contours of masks at the letterboxed input size (H,W) of a (H0,W0) frame, for `masks.xy[i]` without retina_masks: pts_out,
 * count_out and parts_out are byte-equal to yp_mask_contours' (mask pixels). rect_out is the minimum-area rectangle of the polygon after
 * hostops.scale_coords((H,W) -> (H0,W0)) and the int32 truncation of get_coord_min_rect_len - what get_coord_min_rect_len(masks.xy[i])
 * measures: per point x' = (int)min(max(((float)x - padx) / gain, 0), W0) in fp32 (same for y with pady, H0), with gain = min(H/H0, W/W0),
 * padx = (W - W0 * gain) / 2, pady = (H - H0 * gain) / 2 computed in double and rounded to float. When W0 >= 2048 (the hull's column
 * tables cover 0..W0) the device declines the rectangle only: rect_out row = (-1, -1), points as usual (yp_mask_contours_large measures
 * it for any W0). */
int yp_mask_contours_scaled(const uint8_t* masks_dev, int n, int H, int W, int strategy, int max_pts, int32_t* pts_out, int32_t* count_out,
                            int32_t* parts_out, int parts_cap, double* rect_out, int H0, int W0, void* stream);

/* The large path of the two calls above, for the masks they decline: 4K frames, bounding boxes beyond the LDS image, more than 64 outer
 * borders. Same definitions, same outputs in the same layout (so the calls can share one set of buffers); every table lives in the
 * caller's workspace (the bit image of the whole frame, the border starts in raster order, one record per border segment), and a mask's
 * border starts are walked by as many workgroups as there are waves of them. Limits: H, W <= YP_CONTOURS_LARGE_MAX_DIM; up to
 * YP_CONTOURS_LARGE_MAX_STARTS border starts per mask, and as many outer borders. Beyond them: H or W too large is an argument error
 * (YP_ERR_ARG, nothing launched); more border starts, or more than max_pts points, give count_out = -2 as above (host path).
 *    H0, W0     0, 0: rect_out in mask pixels (the large form of the plain call); both > 0: rect_out of the polygon scaled to the (H0,W0)
 *               frame exactly as the scaled call defines it, for any W0 (the column tables are indexed by mask column)
 *    flags      0, or YP_CONTOURS_ONLY_DECLINED: mask i is skipped - none of its rows is touched - when, on entry, count_out[i] >= 0 and
 *               (rect_out is NULL or rect_out[2 * i] >= 0); a mask with count_out[i] >= 0 and a rectangle row at (-1, -1) keeps its points
 *               and gets the rectangle only. So a second call on the buffers of a first fills in what that one declined.
 *    parts_out  as above; its rows hold as many contour lengths as parts_cap allows (not capped at 64)
 *    workspace_dev  device memory of at least the workspace query's size for (n, H, W), 16-byte aligned, owned by the caller;
 *               its contents need not survive the call. The query returns 0 for sizes the call would reject. n <= 65535. */
#define YP_CONTOURS_ONLY_DECLINED 1
#define YP_CONTOURS_LARGE_MAX_DIM 4096
#define YP_CONTOURS_LARGE_MAX_STARTS 65536
size_t yp_mask_contours_large_workspace(int n, int H, int W);
int yp_mask_contours_large(const uint8_t* masks_dev, int n, int H, int W, int strategy, int max_pts, int32_t* pts_out, int32_t* count_out,
                           int32_t* parts_out, int parts_cap, double* rect_out, int H0, int W0, int flags, void* workspace_dev,
                           size_t workspace_bytes, void* stream);

/* The "all_merged" polygon order on the device: masks2segments of the later 8.3.x releases joins a mask's contours with
 * merge_multi_segment (hostops.merge_contours is the definition) instead of laying them end to end. Runs on the buffers the three contour
 * calls above fill with YP_CONTOURS_ALL - same stream, nothing read back in between - and writes the bridged list to a second buffer:
 * consecutive contours of the list are bridged at their closest pair of points (first minimum of the squared integer distance in row-major
 * order of the (index in c_{i-1}, index in c_i) table), a middle contour whose entry index is greater than its exit index is reversed with
 * the indices swapped, every contour is rolled to its entry point and closed by repeating it; the first and the last contour are listed
 * whole, a middle one from entry to exit on the way out and the rest on the way back, the way-back pieces in reverse contour order. A list
 * of k > 1 contours with m points has m + 2k - 2 points afterwards; one contour is copied unchanged (not closed).
 *    pts_dev, count_dev, parts_dev   what a contour call wrote: int32 [n,max_pts,2], [n], [n,parts_cap]; pts_dev 8-byte aligned;
 *               coordinates below 4096; max_pts <= YP_CONTOURS_MERGE_MAX_PTS; 2 <= parts_cap <= YP_CONTOURS_LARGE_MAX_STARTS + 1
 *    merged_out int32 [n,out_cap,2], 8-byte aligned, no overlap with the inputs      merged_count_out int32 [n]: points of the bridged list;
 *               count_dev[i] <= 0 (empty, or declined by the trace) is passed on as it is; -1 = the bridged list has more than out_cap
 *               points, the parts row does not list every contour (parts_cap too small) or its lengths do not add up to the count: nothing
 *               of that mask's rows is written, the other masks of the call are not affected (bridge it on the host from pts_dev)
 *    workspace_dev  as for the large path: at least the query's bytes for (n, parts_cap), 16-byte aligned, the caller's, free to reuse
 *               once the stream's work is done. The query returns 0 for sizes the call rejects. n <= 65535.
 * The closest pairs are searched in tiles of YP_CONTOURS_MERGE_TILE points a side; the per-mask scans step through the contours
 * YP_CONTOURS_MERGE_SCAN_BLOCK at a time. The tiles query is host arithmetic: the number of work tiles the device derives for one mask
 * whose contours have these lengths (0 for fewer than two contours or a length outside 1 .. YP_CONTOURS_MERGE_MAX_PTS). */
#define YP_CONTOURS_MERGE_TILE 256
#define YP_CONTOURS_MERGE_SCAN_BLOCK 1024
#define YP_CONTOURS_MERGE_MAX_PTS 524288
size_t yp_mask_contours_merge_workspace(int n, int parts_cap);
unsigned long long yp_mask_contours_merge_tiles(const int32_t* lengths_host, int n_contours);
int yp_mask_contours_merge(const int32_t* pts_dev, const int32_t* count_dev, const int32_t* parts_dev, int n, int max_pts, int parts_cap,
                           int32_t* merged_out, int32_t* merged_count_out, int out_cap, void* workspace_dev, size_t workspace_bytes,
                           void* stream);
/* the two sizes above as the loaded library was built with them (tile, scan block) */
void yp_mask_contours_merge_sizes(int* tile, int* scan_block);

/* LetterBox on the device (the step before the network inside `.predict`; reference call sites yolo_seg/app.py:86-91,
 * [U] ultralytics LetterBox = cv2.resize INTER_LINEAR + cv2.copyMakeBorder(114)). Engine-free, pure function of its
 * arguments; bit-exact with the fixed-point 8-bit bilinear resize the oracle restates.
 *    src_dev: uint8 [h0,w0,3] (HWC, any channel order)      dst_dev: uint8 [out_h,out_w,3]
 *    the resized image (new_h x new_w; resize skipped when equal to h0 x w0) lands at (top,left), the rest is pad_value.
 *    The geometry is the caller's (LetterBox arithmetic is host integer math: predictor.py / hostops.letterbox_geometry). */
int yp_letterbox(const uint8_t* src_dev, int h0, int w0, uint8_t* dst_dev, int out_h, int out_w, int new_h, int new_w,
                 int top, int left, int pad_value, void* stream);
/* n frames of one geometry in one launch: src_dev uint8 [n,h0,w0,3] -> dst_dev uint8 [n,out_h,out_w,3], byte-equal to n calls of
 * yp_letterbox. 0 <= n <= 65535; n*h0*w0*3 and n*out_h*out_w*3 < 2^31. */
int yp_letterbox_batch(const uint8_t* src_dev, int n, int h0, int w0, uint8_t* dst_dev, int out_h, int out_w, int new_h,
                       int new_w, int top, int left, int pad_value, void* stream);

/* The app's output frame on the device, n frames in one launch (loop #2 of the video path: the crop-mask paste, create_roi_mask and the
 * two saturating cv2.addWeighted calls, yolo_seg/app.py:179-190, yolo_seg/utils/mask_tools.py:100-129). Engine-free; launches on the
 * current device. Per byte of frame f, pixel (y,x), channel c:   dst = min(255, src + M + R[c])
 *    M     masks_dev[crop][y - y_lt][x - x_lt] inside the window x_lt <= x < x_rd, y_lt <= y < y_rd, else 0: the byte as it is, the same
 *          for the three channels. masks_dev uint8 [B,ch,cw] (row stride cw, the window at the crop's top-left); a full-frame mask
 *          [n,H,W] is B = n, ch = H, cw = W with the window (0,0,W,H). An empty window (x_rd == x_lt or y_rd == y_lt) adds nothing.
 *    R[c]  max(band ? col[c] : 0, (cov * col[c] + 127) / 255): rectangle and label drawn into one image, as the reference does.
 *    band  cv2.rectangle((x1,y1),(x2,y2), thickness 2) stated as: every in-frame pixel at Chebyshev distance <= 1 from the one-pixel
 *          outline through the two corners; x2 == W and y2 == H clip to the frame (stated, not pinned against cv2: its round caps may
 *          leave out the four outer corner pixels).
 *    cov   labels_dev[f][y - ly][x - lx] for 0 <= x - lx < lw, 0 <= y - ly < lh, else 0. labels_dev uint8 [n,LH,LW] coverage bitmaps
 *          (may be NULL when no frame has a label); (lx,ly) may lie outside the frame, the bitmap is clipped to it.
 *    params  HOST int32 [n, YP_OVERLAY_PARAMS]: x_lt, y_lt, x_rd, y_rd, x1, y1, x2, y2, lx, ly, lw, lh, crop (lw or lh 0: no label). The
 *          rows travel to the device as kernel arguments, 64 frames per launch: the call stages nothing, waits for nothing and keeps
 *          no state, so it is safe from any thread and on any stream.
 *    col   HOST uint8 [3] (BGR), NULL = (0,0,255).
 * dst_dev != src_dev (no overlap): every byte of the n frames is read once and written once, 16 bytes per lane wherever the address
 * allows, whatever the alignment of the base, of W*3 and of H*W*3. dst_dev == src_dev: in place, only the 16-byte groups that meet the
 * window, the band or the label are loaded and stored. n >= 0, H*W*3 < 2^31; frame offsets are 64-bit.
 * Checked before anything is launched (YP_ERR_ARG): null pointers, a window outside the frame or larger than ch x cw, x2 < x1 or
 * y2 < y1, a crop index outside [0,B), a label larger than LH x LW. */
#define YP_OVERLAY_PARAMS 13
int yp_overlay_frames(const uint8_t* src_dev, uint8_t* dst_dev, int n, int H, int W, const uint8_t* masks_dev, int B, int ch, int cw,
                      const int32_t* params, const uint8_t* labels_dev, int LH, int LW, const uint8_t* col, void* stream);

/* -- U^2-Net-P / U^2-Net: the second per-frame network of the reference's video loop, `unet_predict(unet_model,
 *    cropped_frame)` at yolo_seg/app.py:184. Model: yolo_seg/tasks/models/U2Net.py:424-526 (U2NETP) / :318-420 (U2NET); loader and
 *    post-process: yolo_seg/tasks/unet_segment.py:32-73. variant 'p' = U2NETP, 'f' = U2NET. Weights are handed over folded (conv +
 *    eval-mode BatchNorm -> one weight/bias pair per REBNCONV, named like the reference modules: "stage1.rebnconvin.weight", ...,
 *    "side1.weight", "outconv.weight"), exactly like yp_set_weight.
 *    yp_u2net_forward: bgr_dev uint8 [B,H,W,3] BGR (what cv2 hands the reference; BGR->RGB and /255 of numpy2tensor happen on the device),
 *      prob_out float [B,H,W] = sigmoid(d0), the first of the model's seven outputs (required)
 *      norm_out float [B,H,W] = normPRED(prob) = (p - min) / (max - min) over the whole call (may be NULL)
 *      mask_out uint8 [B,H,W] = norm > 0.5 ? 255 : 0, the array `unet_predict` returns (may be NULL) */
typedef struct yp_u2net yp_u2net;
int yp_u2net_create(int variant, int dtype, int device, yp_u2net** out);
int yp_u2net_destroy(yp_u2net* e);
int yp_u2net_weight_count(const yp_u2net* e);
int yp_u2net_weight_info(const yp_u2net* e, int i, char* name, int name_cap, int64_t shape[4], int* ndim);
int yp_u2net_set_weight(yp_u2net* e, const char* name, const float* host, const int64_t* shape, int ndim);
int yp_u2net_finalize(yp_u2net* e);
int yp_u2net_forward(yp_u2net* e, const uint8_t* bgr_dev, int B, int H, int W, float* prob_out, float* norm_out,
                     uint8_t* mask_out, void* stream);
/*    yp_u2net_forward_crops: the clip form of crop_frame + unet_predict + the app's paste (yolo_seg/app.py:127,183-186). frames_dev
 *      uint8 [N,H,W,3] BGR; windows int32 [B,4] host array, each row the clipped (x1,y1,x2,y2) crop_frame returns; frame_idx int32 [B]
 *      host array, the frame of each crop; (ch, cw) the crop shape every window of the call shares (each window no larger). Crop pixel
 *      (y,x) is the frame pixel (y1+y, x1+x) inside the window and 0 elsewhere (the window sits at the top-left of the zero pad).
 *      prob_out float [B,ch,cw] = sigmoid(d0) (may be NULL); crop_mask_out uint8 [B,ch,cw] = normPRED(prob) > 0.5 ? 255 : 0 with min /
 *      max taken per crop, pad included, as the per-frame reference call does (may be NULL); frame_mask_out uint8 [N,H,W] (may be NULL):
 *      for every frame a crop names (at most once), the crop mask's top-left (y2-y1) x (x2-x1) block at (y1,x1) and 0 everywhere else.
 *      Windows, indices and sizes are checked before any launch (YP_ERR_ARG). Eager launches on `stream`, never graph replay. */
int yp_u2net_forward_crops(yp_u2net* e, const uint8_t* frames_dev, int N, int H, int W, const int32_t* windows, const int32_t* frame_idx,
                           int B, int ch, int cw, float* prob_out, uint8_t* crop_mask_out, uint8_t* frame_mask_out, void* stream);
int yp_u2net_set_graph(yp_u2net* e, int enable);   /* hipGraph replay of the forward (default off: measured slower than eager launches; the first pass of a shape is always eager) */
int yp_u2net_tensor_count(const yp_u2net* e);
int yp_u2net_tensor_info(const yp_u2net* e, int i, char* name, int name_cap, int dims[4] /*B,H,W,C*/);
int yp_u2net_tensor_read(yp_u2net* e, int i, float* host_out);   /* sync copy NHWC -> fp32 host (debug taps) */
/*    Read-only view of the plan (per-op tests): yp_u2net_op_info writes op i's name and up to info_cap of its YP_U2_OP_INFO = 17 fields
 *      [kind (0 input, 1 conv, 2 pool, 3 up), in (tensor, coff, C), out (tensor, coff, C), res (tensor or -1, coff, C), dil, act (0 none,
 *      2 ReLU), logical Cin, impl (-1 not chosen yet, 0 conv_igemm, 1 conv_small, 2 conv_small taking its pool / up-sample while loading,
 *      3 conv_halo_f32), pool_op, up_op, consumer (op indices or -1)] and returns 17. impl is that of the current plan: final once a
 *      forward of the shape has run. A pool / up op whose consumer has impl 2 does not launch (its output tensor is not written). */
#define YP_U2_OP_INFO 17
int yp_u2net_op_count(const yp_u2net* e);
int yp_u2net_op_info(const yp_u2net* e, int i, char* name, int name_cap, int32_t* info, int info_cap);

/* -- EfficientNet-B3 needle classifier: the third network of the reference's video loop, `load_classify_net` +
 *    `predict_and_find_start_inserted` (yolo_seg/app.py:116-123 -> yolo_seg/tasks/needle_clasify.py:41-199), efficientnet_pytorch's
 *    `EfficientNet.from_name('efficientnet-b3', num_classes=2)`. variant = 3 (b3; every other value is refused). Weights are handed over
 *    folded (conv + eval-mode BatchNorm, eps 1e-3 -> one weight/bias pair), named after the reference modules: "_conv_stem",
 *    "_blocks.{i}._expand_conv" / "._depthwise_conv" / "._project_conv", the SE convs "._se_reduce" / "._se_expand" (their own bias),
 *    "_conv_head" and "_fc" (weight [2,1536], rank 2).
 *    yp_cls_forward: frames_dev uint8 [B,H,W,3] (bgr = 1: BGR as cv2 reads them; 0: RGB), boxes_dev int32 [B,4] xyxy; the 380x380 crop
 *      window of crop_frame(frame, box, 380, need_padding=True) is read straight from the frame (never materialised),
 *      logits_out float [B,2], prob_out float [B] = max softmax, cls_out int32 [B] = argmax. */
typedef struct yp_cls yp_cls;
int yp_cls_create(int variant, int dtype, int device, yp_cls** out);
int yp_cls_destroy(yp_cls* e);
int yp_cls_weight_count(const yp_cls* e);
int yp_cls_weight_info(const yp_cls* e, int i, char* name, int name_cap, int64_t shape[4], int* ndim);
int yp_cls_set_weight(yp_cls* e, const char* name, const float* host, const int64_t* shape, int ndim);
int yp_cls_finalize(yp_cls* e);
int yp_cls_forward(yp_cls* e, const uint8_t* frames_dev, int B, int H, int W, int bgr, const int32_t* boxes_dev, float* logits_out,
                   float* prob_out, int32_t* cls_out, void* stream);
int yp_cls_set_graph(yp_cls* e, int enable);   /* hipGraph replay (default off); specialised on shape and pointers, a change re-captures */
int yp_cls_tensor_count(const yp_cls* e);
int yp_cls_tensor_info(const yp_cls* e, int i, char* name, int name_cap, int dims[4] /*B,H,W,C*/);
int yp_cls_tensor_read(yp_cls* e, int i, float* host_out);   /* sync copy NHWC -> fp32 host (debug taps) */

/* -- multi-GPU: frames are sharded over one process per GPU; the only data-path collective is ONE all-gather of
 *    the [B/G,max_det,6] detections per batch over RCCL (xGMI). The reference has no multi-GPU path (frames are independent inside
 *    `.predict`, yolo_seg/app.py:85-91). bench.py / parallel.py use torch.distributed's "nccl" backend for it; these entry points
 *    give a host without PyTorch the same collective. librccl.so is resolved at run time (dlopen).
 *      rank 0: yp_comm_unique_id(id) -> ship the 128 bytes to every rank (any channel) -> all ranks: yp_comm_create(id, rank, world, dev)
 *      yp_allgather: recv_dev holds world * bytes_per_rank bytes in rank order; enqueued on `stream`. */
typedef struct yp_comm yp_comm;
int yp_comm_unique_id(void* id128);
int yp_comm_create(const void* id128, int rank, int world, int device, yp_comm** out);
int yp_allgather(yp_comm* c, const void* send_dev, void* recv_dev, size_t bytes_per_rank, void* stream);
int yp_comm_destroy(yp_comm* c);

/* -- introspection (tests, bench): the planned op list for an input shape; host only. */
/* Input size limits. All of them are checked by yp_plan (and by everything that plans: yp_forward, yp_tuning_import), before any launch,
 * with a message that names the quantity and the largest value that fits (YP_ERR_ARG):
 *   anchors  (H/8 * W/8 + H/16 * W/16 + H/32 * W/32) <= YP_MAX_ANCHORS. Up to 12288 anchors the heads select inside one workgroup's LDS;
 *            beyond, chunks of 12288 anchors select in parallel and one workgroup per image merges the chunk winners (v10), or the
 *            candidates above `conf` are gathered into a global list first (NMS families; at most the max_nms best-scoring candidates of
 *            an image enter NMS: 16384 by default, ultralytics' 30000 through yp_set_nms_options).
 *   attention tokens (H/32 * W/32, v10 and 11 only): above 400 the PSA block runs a generic kernel that keeps 16 x tokens scores in LDS,
 *            which ends at 2368 tokens for 32-wide keys. v8 has no attention. An engine whose attention form is `stream`
 *            (yp_set_attention_form) runs bf16 PSA blocks with 32-wide keys and 64-wide heads - every v10 variant except M, every YOLO11
 *            variant - above 400 tokens on a matrix-core kernel that streams K and V through LDS: no token bound of its own, the anchor
 *            bound (anchors = 21 x tokens, so 14043 tokens) and the byte bound remain. v10-M (36-wide keys, 72-wide heads) does the same
 *            at every token count under the form `stream_wide`, which includes `stream`; under `auto` and `stream` it keeps the generic
 *            kernel and its bound of 2364 tokens. fp32 engines keep the generic kernel and its bound under every form; their
 *            streaming kernels have a switch of their own (yp_set_attention_f32_stream: value 1 - 32-wide keys and 64-wide heads, above
 *            400 tokens, no token bound; fp32 v10-M keeps the generic kernel and 2364 tokens under 0 and 1 and streams above 400 tokens
 *            under value 3).
 *   bytes    every activation stays below 2^31 bytes: yp_max_batch(e, H, W) is the largest B that plans at HxW (callers split to it). */
#define YP_MAX_ANCHORS 294912   /* 12288 * (12288 / 512): covers 3840x2176 (214200) */
int yp_max_batch(const yp_engine* e, int H, int W);
int yp_plan(yp_engine* e, int B, int H, int W);            /* (re)build the plan; returns #ops or <0 */
int yp_op_info(const yp_engine* e, int i, char* name, int name_cap, int* kind, double* flops,
               double* bytes);                                 /* algorithmic FLOPs / HBM bytes of op i */
int yp_op_kernel(const yp_engine* e, int i, char* name, int name_cap);   /* device kernel symbol op i launches */
int yp_op_output(const yp_engine* e, int i, int* tensor, int* coff, int* C); /* output channel slice of op i (tensor<0: user buffers) */
/* Input view of op i, and `c_read`: the channels a dense conv packed with padded taps actually reads per pixel (> C for 48- / 80-channel
   inputs: the surplus lanes meet zero weights; their bytes come from the next pixel or, at the very end, from the tensor's zeroed tail). */
int yp_op_input(const yp_engine* e, int i, int* tensor, int* coff, int* C, int* c_read);
/* Fused producer of op i under the current plan: *pre = index of the 1x1 conv that runs as the first stage of op i's kernel (pwsp_kernel:
   1x1 -> depthwise conv / SPPF pool chain, one workgroup per image and channel slice), or -1; *pre_stored = 1 when that kernel also writes
   the 1x1's own output tensor (it has other readers). The parity tests use it to teacher-force both results of such a launch. */
int yp_op_fusion(const yp_engine* e, int i, int* pre, int* pre_stored);
/* Launch form of op i under the current plan: *form = 0 when it launches as its own kernel (or not at all), else the fused form
   (1 dw -> pw, 2 dw -> pw -> logits, 3 3x3 s2 -> 1x1, 4 stem -> 3x3 s2 -> 1x1, 5 C2f bottleneck -> 1x1, 6 1x1 -> dw s2, 7 1x1 -> dw / pool
   chain, 8 logits + class-max keys). Returns the number of ops whose work that launch takes over - they launch nothing and report no
   FLOPs or bytes - and fills absorbed[0 .. min(n, cap)) with their indices (either pointer may be null); < 0 on a bad index. Host only. */
int yp_debug_op_form(const yp_engine* e, int i, int* form, int* absorbed, int cap);
/* Debug stepping for per-op parity tests ("teacher forcing"): run ONE op of the current plan, and overwrite a
 * channel slice of an engine tensor from fp32 host data [B,H,W,C] (converted to the tensor's storage type). */
int yp_run_op(yp_engine* e, int i, const uint8_t* in_dev, float* det_out, int32_t* idx_out, float* coeff_out, void* stream);
int yp_tensor_write(yp_engine* e, int tensor, int coff, int C, const float* host);
int yp_tensor_count(const yp_engine* e);
int yp_tensor_info(const yp_engine* e, int i, char* name, int name_cap, int dims[4] /*B,H,W,C*/, int* is_f32);
int yp_tensor_read(yp_engine* e, int i, float* host_out);  /* sync copy NHWC -> fp32 host (debug taps) */

/* Run the plan op by op with a HIP event pair around every launch on `stream`; ms_out[#ops]. */
int yp_profile(yp_engine* e, const uint8_t* in_dev, int B, int H, int W, float* det_out, int32_t* idx_out,
               float* coeff_out, float* ms_out, int iters, void* stream);

/* NMS heads (families v8 / 11): score threshold and IoU threshold of `ops.non_max_suppression` [U] as `.predict(conf=, iou=)` sets
 * them (defaults 0.25 / 0.7). Rows of yp_forward's det_out are the boxes NMS keeps, best first; may be changed between forwards
 * (the values live in device memory: a captured graph does not go stale). No effect on the v10 family. */
int yp_set_nms(yp_engine* e, float conf, float iou);

/* NMS heads (families v8 / 11): the other three arguments of `.predict` that steer `ops.non_max_suppression` [U] (multi_label=False):
 *   classes   n_classes class ids in [0, nc): only candidates of these classes take part - filtered before NMS and before the max_nms
 *             cut, as [U] does. NULL or n_classes == 0: all classes (the default).
 *   agnostic  != 0: no per-class box offset, a kept box suppresses overlapping boxes of every class (`agnostic_nms=True`). Default 0.
 *   max_nms   in [1, YP_MAX_ANCHORS]: the max_nms best candidates (score descending, lower anchor first among equal scores) enter NMS.
 *             Default 16384; ultralytics' own value is 30000 - pass it to get [U]'s rows when more than 16384 anchors pass `conf`
 *             (possible from 1024x800 on). Above 16384 the NMS kernel works through the sorted list in rounds of 16384 keys: exact
 *             greedy NMS over the whole list.
 * May be changed between forwards: the values live in device memory beside conf / iou. Any non-default value moves the head op to option
 * kernels of its own (yp_op_kernel names them); that step - and the step back - drops a captured graph and costs the next forward one
 * extra eager pass, a change among non-default values costs nothing. Host only (nothing is launched here).
 * YP_ERR_ARG: a class id outside [0, nc), n_classes < 0, max_nms out of range, or a v10 engine (its head is a top-k without NMS: filter its
 * rows on the host). */
int yp_set_nms_options(yp_engine* e, const int32_t* classes, int n_classes, int agnostic, int max_nms);

/* Attention form of the PSA block (v10 / 11): 0 auto - the default: the resident matrix-core kernel up to 400 tokens, the generic kernel up to
 * its LDS bound, refusal beyond -, 1 stream - bf16, key_dim 32, head_dim 64 above 400 tokens run attention_stream_kernel (two passes over K:
 * row max and sum, then P.V with the normalised bf16 probabilities; same rounding points as the other kernels, no token bound); whatever is
 * outside that scope runs and is refused as under 0 -, 3 stream_wide - form 1, and bf16, key_dim 36, head_dim 72 (YOLOv10-M) run
 * attention_stream_wide_kernel at every token count (the same two passes and rounding points). The value is a bit set - bit 0 the 32/64
 * streaming kernel, bit 1 the 36/72 one, itself a streaming kernel: 2 is no form. Any other value: YP_ERR_ARG. Allowed before or after
 * yp_finalize; a change drops the current plan (the next yp_plan / yp_forward plans again). An engine created while YOLOP_ATTN_FORM=stream
 * (stream_wide) is set starts in form 1 (3). */
int yp_set_attention_form(yp_engine* e, int form);

/* fp32 streaming attention, a switch of its own beside the attention form (which stays a bf16 matter): on = 1 lets an fp32 engine's PSA
 * block with key_dim 32 and head_dim 64 - every v10 variant except M, every YOLO11 variant - run attention_stream_f32_kernel above 400
 * tokens: K and V stream through LDS in blocks of 64 keys, both products on the fp32 matrix-core instruction (an exact fp32 FMA chain, so
 * the fp32 contract gains no rounding point), two passes over K (row max and sum, then P.V with the normalised probabilities). No token
 * bound of its own: the anchor bound and the byte bound (qkv below 2^31 bytes, yp_max_batch) remain. Up to 400 tokens, in bf16 engines and
 * for v10-M's 36/72 heads value 1 changes nothing: same plan, same refusals. on = 3 (stream_wide) is on = 1, and an fp32 engine's PSA
 * block with key_dim 36 and head_dim 72 (YOLOv10-M) runs attention_stream_wide_f32_kernel above 400 tokens: the same two passes and
 * instruction, nine k-steps over the 36 key dimensions, five 16-column output tiles whose eight dead columns are fed zeros and never
 * stored; no token bound of its own either. The value is a bit set like the attention form - bit 0 the 32/64 kernel, bit 1 the 36/72 one:
 * 2 is no value. on = 0 (the default) is the engine as it was: the generic kernel up to 2368 tokens (2364 for v10-M), refusal beyond; the
 * refusal of v10-M does not name the switch. Any other value, or a null engine: YP_ERR_ARG. Allowed before or after yp_finalize; a change
 * drops the current plan and keeps the per-shape tuning memo. An engine created while YOLOP_ATTN_F32=stream (stream_wide) is set starts
 * with value 1 (3); any other non-empty value of the variable fails yp_create. */
int yp_set_attention_f32_stream(yp_engine* e, int on);

/* Enable/disable the plan-time autotuner that picks the conv tile configuration per layer (default on). */
int yp_set_autotune(yp_engine* e, int enable);

/* Tile configurations of the current plan, one id per op (-1 = heuristic / not a tunable conv), as the plan-time autotuner (or an import) left
   them. bf16 results depend on them in the last bit (fp32 summation order), so a job that wants every rank - or every box - to return identical
   detections for a frame tunes once and hands the ids round: rank 0 exports after its first forward, the others import BEFORE theirs
   (yolo_puncture_amd.parallel.sync_tuning does this over torch.distributed; bench.py calls it at N > 1). The reference has no counterpart
   (one process, PyTorch picks its kernels: yolo_seg/app.py:45-50).
   yp_tuning_export: returns the number of ops; fills cfg_out[0..n) when it is non-null (cap >= n). Needs a forward on the current plan.
   yp_tuning_import: plans (B,H,W) and installs the ids for it; every id is validated against this build's configuration tables for its layer
   (all or nothing, YP_ERR_ARG otherwise). The next yp_forward of that shape neither tunes nor reads the tune cache. */
int yp_tuning_export(const yp_engine* e, int32_t* cfg_out, int cap);
int yp_tuning_import(yp_engine* e, int B, int H, int W, const int32_t* cfg, int n);

/* Test hook: force conv tile configuration `cfg` wherever it is valid (-1 = off). Returns the number of configurations. */
int yp_debug_force_conv_cfg(int cfg);
/* Test hook, host only (no GPU needed): the tile configuration id that yp_run_op(e, i) launches op i of the current plan with, under the
   forced id and the plan's own ids as they stand - a conv family's id (conv_dma's only when it was forced or tuned), 1000 for a 1x1 conv that
   runs as pwsp_kernel, -1 where a heuristic picks or the op has no configuration id (fused forms other than the 3x3 s2 -> 1x1 pair, non-conv
   ops), -2 for a folded upsample no configuration can run. */
int yp_debug_op_cfg(const yp_engine* e, int i, int* cfg);
/* Test hook: the store form of the last conv launch of this process whose kernel has both: 1 = 16-byte stores in the paired channel order,
   0 = the 8-byte form (a launch that misses the alignment or width conditions, or an engine created under YOLOP_NARROW_STORE=1, which keeps
   the 8-byte stores everywhere), -1 = no such launch since the last call (the call resets it; launches record their form only from the first call on, so call it once
   before the launch of interest). Read it right after yp_run_op. */
int yp_debug_last_store_form(void);
/* Test hook: at most n workgroups for the persistent kernels that wait for a tile with a counted vmcnt (conv_wres: in whole rounds of 8 tile
   lanes per channel block; conv_dwpw_stream, c2f_fused), 0 = no cap. A small input then makes a workgroup walk several tiles, which is where the counted wait in front of a tile
   comes into play. Host-side only: the launchers read it, device code is the same. Returns the previous value. */
int yp_debug_max_workgroups(int n);
/* Test hook: the conv tile families' configuration id ranges [base, base + num_cfgs), in the autotuner's order. Fills at most cap entries of
   each array (either may be null) and returns the number of families. */
int yp_debug_conv_families(int* base, int* num_cfgs, int cap);
/* Timing ablation for tools (results become wrong): 0 off, 1 conv kernels drop their stores, 2 drop their pixel loads. */
int yp_debug_ablation(int v);
/* Profiling hook: 100 MHz timestamps of the phases of the top-k kernel (image 0's workgroup, last launch):
   [0] start, [1] keys loaded, [2] stage-1 lower bound found, [3] stage-1 select done, [4] stage-2 candidates scanned,
   [5] stage-2 select done, [6] decoded; [7] = stage-2 rounds << 32 | candidates that entered the last round's select. */
int yp_debug_head_clocks(uint64_t* out8);
/* Test hook: the PSA attention core alone, o = softmax(q.k^T * kd^-0.5).v per image and head, through the launcher an OP_ATTN op takes (the same
   parameters, scale = 1/sqrt(kd)). qkv_dev: device [B][N][q_stride], head h of a token at channels q_coff + h*(2kd+hd): q(kd) | k(kd) | v(hd);
   o_dev: device [B][N][o_stride], head h at channels o_coff + h*hd; elements are bf16 (YP_BF16) or float (YP_F32). wgs > 0 replaces the
   matrix-core form's workgroup target (YOLOP_ATTN_WGS, else 256) for this call: it sets the query tiles a workgroup walks. *kernel_out:
   1 the matrix-core kernel took the call, 0 the generic one. Returns after the stream has drained. YP_ERR_ARG (nothing launched) on null
   pointers, non-positive sizes, a slice that does not fit its stride (q_coff + nh*(2kd+hd) > q_stride, o_coff + nh*hd > o_stride), strides
   or offsets that are not multiples of 4 elements, and shapes no kernel holds (more tokens than the generic kernel's LDS, kd or hd % 4). */
int yp_debug_attention(const void* qkv_dev, void* o_dev, int dtype, int B, int N, int nh, int kd, int hd, int q_stride, int q_coff, int o_stride,
                       int o_coff, int wgs, int* kernel_out, void* stream);
/* yp_debug_attention under an attention form (yp_set_attention_form's values; anything else is refused like the rest, on the host): with
   form 1 a bf16 call with kd 32, hd 64, q_stride and q_coff in multiples of 8 and more than 400 tokens takes the streaming kernel, *kernel_out
   = 2, and wgs sets the query groups its workgroups walk; every other call behaves as under form 0, the generic kernel's token bound included.
   Form 3 is form 1, and a bf16 call with kd 36, hd 72, q_stride and q_coff in multiples of 8 takes the wide-head streaming kernel at every
   token count, *kernel_out = 3. yp_debug_attention is this call with form 0. */
int yp_debug_attention_form(const void* qkv_dev, void* o_dev, int dtype, int B, int N, int nh, int kd, int hd, int q_stride, int q_coff, int o_stride,
                            int o_coff, int wgs, int form, int* kernel_out, void* stream);
/* yp_debug_attention on float elements under the fp32 switch (yp_set_attention_f32_stream's values; anything else is refused like the
   rest, on the host): with f32_stream = 1 a call with kd 32, hd 64, more than 400 tokens and qkv below 2^31 bytes takes the fp32 streaming
   kernel, *kernel_out = 4, and wgs replaces its workgroup target (YOLOP_ATTN_WGS, else 1024), which sets the runs of 64-query groups its
   workgroups walk; every other call behaves as with 0, which is
   yp_debug_attention with YP_F32, the generic kernel's token bound included. f32_stream = 3 is 1, and a call with kd 36, hd 72, more than
   400 tokens and qkv below 2^31 bytes takes the wide-head fp32 streaming kernel, *kernel_out = 5, under the same workgroup target. 2 is
   refused. */
int yp_debug_attention_f32(const void* qkv_dev, void* o_dev, int B, int N, int nh, int kd, int hd, int q_stride, int q_coff, int o_stride, int o_coff,
                           int wgs, int f32_stream, int* kernel_out, void* stream);
/* Test hook: one 3x3 / stride-2 / pad-1 bf16 convolution alone through the stride-2 halo family (conv_halo_s2.hip), y = act(W * x + bias)
   [+ res], under configuration id `cfg` of that family (500 ...). x_dev: device bf16 [B][H][W][Cin]; w_dev: device bf16 [Cout][3][3][Cin];
   bias_dev: device float [Cout]; res_dev: device bf16 [B][H/2][W/2][Cout] or null; y_dev: device [B][H/2][W/2][Cout], float when out_f32,
   else bf16; silu: 1 = SiLU, 0 = no activation. lds_weights: 1 = the launch keeps its weights in LDS (as under YOLOP_S2_LDS_WEIGHTS=1),
   0 = the launcher's own pick: the register-weights instance of ids 500 / 501 where Cin is 32 or 64. Returns after the stream has
   drained. YP_ERR_ARG (nothing launched) on non-positive sizes, an id outside the family and a shape the id's validity predicate
   refuses. With x_dev, w_dev, bias_dev and y_dev all null the call is host-only: it applies the same checks (res_dev null or not says
   whether a residual is asked for) and launches nothing. *lds_out (may be null) receives the dynamic LDS bytes of the launch whenever
   the id belongs to the family, kernel_out (may be null) the kernel symbol of an admitted launch. */
int yp_debug_conv_s2(const void* x_dev, const void* w_dev, const float* bias_dev, const void* res_dev, void* y_dev, int out_f32, int B, int H,
                     int W, int Cin, int Cout, int silu, int cfg, int lds_weights, int64_t* lds_out, char* kernel_out, int kernel_cap,
                     void* stream);
/* Test hook: stage 1 of the top-k head alone (the top k anchors by score descending, anchor index ascending) on caller-made class-max keys,
   through the kernels an engine takes for that anchor count: head_select_kernel<1> up to 12288 anchors, head_chunk_topk_kernel +
   head_select_large_kernel<1> beyond. mk_dev[l]: device uint32 [B][hw[l][0] * hw[l][1]], the bits of the anchors' best sigmoid scores as
   the class-max pass leaves them (non-negative floats); 1 <= k <= 512. sel_out_dev: device int32 [B][512], the winners' anchor ids in rank
   order in the first min(k, anchors) slots; thr_out_dev: device uint32 [B], the score bits of the last winner. Returns after the stream
   has drained. YP_ERR_ARG (nothing launched) on null pointers, B < 1, k out of range, an empty level or more than YP_MAX_ANCHORS anchors. */
int yp_debug_topk_anchors(const uint32_t* const mk_dev[3], int B, const int hw[3][2], int k, int32_t* sel_out_dev, uint32_t* thr_out_dev, void* stream);
/* The same for the position kernel of the winners-only head (workgroup 0's first tile, last launch): [0] tile start, [1] position list read,
   [2] first patch plane landed, [3] all channel chunks done, [4] activations stored; [5] = level << 32 | channel chunks of that tile,
   [6] = tiles of the launch (64 positions each), [7] = listed positions of the launch (all levels, all images). */
int yp_debug_head_branch_clocks(uint64_t* out8);
/* Winners-only head (the default for bf16 YOLOv10 engines whose branch width is 64 / 32 channels; YOLOP_DENSE_HEAD=1 at yp_create keeps
   every branch dense): the box branch `one2one_cv2.*` - and the coefficient branch `cv4.*` of the seg head - are evaluated only for the
   max_det anchors the class scores select, which are the only ones whose boxes the reference's v10postprocess gathers ([U] SURVEY A.6;
   inside `.predict`, yolo_seg/app.py:91): the first 3x3 once per distinct position of the winners' 3x3 neighbourhoods, the second 3x3 and
   the 1x1 at the winners. Same inputs, weights and rounding points as the dense convolutions, so the same numbers up to fp32 summation
   order. This hook copies what the last forward left: sel_host int32 [B][512] (stage-1 winners, anchor ids by rank),
   box_host float [B][max_det][64] and coeff_host float [B][max_det][32] (rows by rank; any may be NULL).
   Returns bit 0: box rows are winners-only, bit 1: coefficient rows are; 0 = dense head. */
int yp_debug_head_winners(yp_engine* e, int32_t* sel_host, float* box_host, float* coeff_host);
/* phase stamps of yp_mask_contours (mask 0): [0..6] 100-MHz ticks at box / bit image / candidates / trace / emit / hull / end, [8] candidates,
   [9] points of the winning contour, [10], [11] bounding box width, height */
int yp_debug_contour_clocks(uint64_t* out12);
/* phase stamps (core clock) of workgroup 0 in the last pwsp_kernel launch: [0] start, [1] prologue issued, [2] GEMM done, [3] epilogue done,
   [4] behind the barrier, [5] spatial stage done, [8 + g] top of k-step g (g < 16) */
int yp_debug_pwsp_clocks(uint64_t* out32);

/* Where the tile configurations of the current plan came from: 0 = this process's tuner (or the heuristics, with autotuning off),
 * 1 = a YOLOP_TUNE_CACHE file, 2 = a table packaged beside the library (tune_tables/tt_<key>.txt: the best of several tunings of that
 * shape; used when YOLOP_TUNE_CACHE is unset; YOLOP_NO_TUNE_TABLES=1 ignores them). */
int yp_tuning_source(const yp_engine* e);

/* Host-only self-check of the executor for the current plan (parameter blocks, kernel symbols, tune-cache round trip, lane
 * schedule invariants). Needs no GPU; returns the number of scheduled launches or <0. Used by the CPU sanitizer build. */
int yp_debug_host_selftest(yp_engine* e);
/* What the last capture built: out[0] captures + instantiations so far, [1] graph nodes, [2] graph edges, [3] edges into the first node
   of every op as the lane schedule prescribes them (for a chain: nodes - 1; [2] - [3] = the inner chains of ops that launch several
   kernels), [4] lanes that launched, [5] 1 while an executable exists. */
int yp_debug_graph_info(const yp_engine* e, int64_t* out6);
/* Winners-only head, last forward: out[0..3) distinct positions listed per level (P3, P4, P5; all images), out[3..6) winners per level.
   Returns 0 for a dense head (out zeroed). Synchronises the device. */
int yp_debug_head_positions(yp_engine* e, int64_t* out6);
/* Profiling hook: enqueue a one-thread kernel named op_marker_kernel (tools/op_traffic.py brackets the launches of one op with it so that
   per-dispatch counter rows can be attributed to ops). */
int yp_debug_marker(void* stream);

/* hipGraph capture + replay of the forward: 0 = eager launches on the caller's stream (the library default), 1 = one hipGraph whose
 * independent head branches are parallel branches of the graph, 2 = the graph as one chain (what a ring of several engines uses; A/B),
 * 3 = auto: per input shape, whichever of 0 and 1 a one-off timing inside the first yp_forward of that shape finds faster on this box
 * (what predictor.py uses: one frame per call - yolo_seg/app.py:85-91 - runs eagerly, batches replay). The first forward of every
 * input shape runs once eagerly inside yp_forward before anything is captured.
 * Stream contract: a replay is launched on the CALLER's stream (`stream` of yp_forward); a caller on the legacy NULL stream gets the
 * engine's own stream ordered in between by an event pair. Forwards of one engine never overlap: a call on another stream than the
 * engine's previous call first waits (on the device) for that call's completion event. The graph is specialised on the plan, the input
 * pointer and the output pointers; a caller that keeps them from call to call never re-captures (yp_debug_graph_info counts captures). */
int yp_set_graph(yp_engine* e, int enable);

#ifdef __cplusplus
}
#endif
#endif /* YOLOP_H */
