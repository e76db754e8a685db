// Host-side sanitizer driver (CPU container, no GPU): links libyolop_asan.so (`make -C yolo-puncture_amd/csrc asan`) and walks the
// part of the C-ABI that runs without a device for every variant x task x dtype: graph build, weight hand-over (host copies),
// planning for several input shapes, op / tensor introspection, kernel-symbol completion, tune-cache round trip, per-shape tuning
// memo and the lane schedule (yp_debug_host_selftest), error paths, destroy. AddressSanitizer + UBSan abort on the first finding.
#include "../include/yolop.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(x)                                                                                         \
    do {                                                                                                 \
        if (!(x)) { fprintf(stderr, "asan_host: CHECK failed: %s (%s:%d): %s\n", #x, __FILE__, __LINE__, yp_last_error()); exit(1); } \
    } while (0)

int main() {
    const char variants[] = {'n', 's', 'm', 'b', 'l', 'x'};
    const int shapes[][3] = {{1, 64, 64}, {2, 96, 128}, {1, 384, 640}, {32, 640, 640}, {8, 640, 640}, {3, 480, 608}, {1, 640, 480}, {5, 32, 32}};
    long launches = 0;
    const int families[] = {YP_FAMILY_V10, YP_FAMILY_V8, YP_FAMILY_11};
    for (int fam : families)
    for (char v : variants)
        for (int task = 0; task < 2; ++task)
            for (int dtype = 0; dtype < 2; ++dtype) {
                if (fam != YP_FAMILY_V10 && (task == 0 || v == 'b' || dtype == 1)) continue;     // the v8 / 11 families: n s m l x, segment
                yp_model_desc d{v, 80, task, dtype, 300, fam};
                yp_engine* e = nullptr;
                CHECK(yp_create(&d, 0, &e) == YP_OK);
                const int nw = yp_weight_count(e);
                CHECK(nw > 0);
                for (int i = 0; i < nw; ++i) {
                    char name[256];
                    int64_t shp[4];
                    int nd = 0;
                    CHECK(yp_weight_info(e, i, name, sizeof(name), shp, &nd) == YP_OK);
                    size_t n = 1;
                    for (int k = 0; k < nd; ++k) n *= (size_t)shp[k];
                    std::vector<float> w(n);
                    for (size_t k = 0; k < n; ++k) w[k] = (float)((k * 2654435761u) & 0xffff) / 65536.f - 0.5f;
                    CHECK(yp_set_weight(e, name, w.data(), shp, nd) == YP_OK);
                    if (i == 0) {                                       // error paths: wrong rank, wrong shape, unknown name
                        int64_t bad[4] = {shp[0] + 1, shp[1], shp[2], shp[3]};
                        CHECK(yp_set_weight(e, name, w.data(), bad, nd) < 0);
                        CHECK(yp_set_weight(e, name, w.data(), shp, 1) < 0);
                        CHECK(yp_set_weight(e, "model.99.weight", w.data(), shp, nd) < 0);
                    }
                }
                CHECK(yp_finalize(e) < 0);                              // no device here: must refuse, not fall back
                CHECK(yp_plan(e, 1, 100, 100) < 0);
                for (const auto& s : shapes) {
                    const int nops = yp_plan(e, s[0], s[1], s[2]);
                    CHECK(nops > 0);
                    for (int i = 0; i < nops; ++i) {
                        char name[8];                                   // deliberately short: snprintf must truncate
                        char kname[256];
                        int kind, t, co, c;
                        double fl, by;
                        CHECK(yp_op_info(e, i, name, sizeof(name), &kind, &fl, &by) == YP_OK);
                        CHECK(yp_op_kernel(e, i, kname, sizeof(kname)) == YP_OK);
                        CHECK(yp_op_output(e, i, &t, &co, &c) == YP_OK);
                    }
                    const int nt = yp_tensor_count(e);
                    for (int i = 0; i < nt; ++i) {
                        char name[256];
                        int dims[4], f32;
                        CHECK(yp_tensor_info(e, i, name, sizeof(name), dims, &f32) == YP_OK);
                    }
                    const int st = yp_debug_host_selftest(e);
                    CHECK(st > 0);
                    launches += st;
                }
                // back to the first shape: the per-shape memo path
                CHECK(yp_plan(e, shapes[0][0], shapes[0][1], shapes[0][2]) > 0);
                CHECK(yp_debug_host_selftest(e) > 0);
                // NMS options: the class list becomes mask words on the host; refusals are loud; only v8 / 11 have an NMS to steer
                {
                    const int32_t cls[3] = {0, d.nc - 1, d.nc / 2}, outside[2] = {1, d.nc}, negative[1] = {-1};
                    if (fam == YP_FAMILY_V10) {
                        CHECK(yp_set_nms_options(e, cls, 3, 1, 30000) == YP_ERR_ARG && strstr(yp_last_error(), "v10"));
                    } else {
                        CHECK(yp_set_nms_options(nullptr, cls, 3, 1, 30000) == YP_ERR_ARG);
                        CHECK(yp_set_nms_options(e, outside, 2, 0, 16384) == YP_ERR_ARG && strstr(yp_last_error(), "class id"));
                        CHECK(yp_set_nms_options(e, negative, 1, 0, 16384) == YP_ERR_ARG);
                        CHECK(yp_set_nms_options(e, cls, -1, 0, 16384) == YP_ERR_ARG);
                        CHECK(yp_set_nms_options(e, nullptr, 0, 0, 0) == YP_ERR_ARG && strstr(yp_last_error(), "max_nms"));
                        CHECK(yp_set_nms_options(e, nullptr, 0, 0, YP_MAX_ANCHORS + 1) == YP_ERR_ARG);
                        CHECK(yp_set_nms_options(e, cls, 3, 1, YP_MAX_ANCHORS) == YP_OK);
                        CHECK(yp_debug_host_selftest(e) > 0);
                        CHECK(yp_set_nms_options(e, nullptr, 0, 0, 16384) == YP_OK);
                    }
                }
                // beyond 12288 anchors: the heads' large forms plan; what no kernel holds is refused by yp_plan and leaves the plan as it was
                CHECK(yp_plan(e, 1, 800, 768) > 0);
                CHECK(yp_debug_host_selftest(e) > 0);
                CHECK(yp_plan(e, 1, 3776, 3840) == YP_ERR_ARG && strstr(yp_last_error(), "anchors"));                    // one row past YP_MAX_ANCHORS
                if (fam != YP_FAMILY_V8) CHECK(yp_plan(e, 1, 2560, 1472) == YP_ERR_ARG && strstr(yp_last_error(), "attention tokens"));
                else CHECK(yp_plan(e, 1, 2560, 1472) > 0);
                // the streaming attention form: 3680 tokens plan where the kernel's scope holds (bf16, 32-wide keys), the refusal stays elsewhere
                CHECK(yp_set_attention_form(e, 2) == YP_ERR_ARG && yp_set_attention_form(nullptr, 1) == YP_ERR_ARG);
                CHECK(yp_set_attention_form(e, 1) == YP_OK);
                {
                    const bool in_scope = fam != YP_FAMILY_V8 && d.dtype == YP_BF16 && !(fam == YP_FAMILY_V10 && d.variant == 'm');
                    const int rc = yp_plan(e, 1, 2560, 1472);
                    if (fam == YP_FAMILY_V8 || in_scope) {
                        CHECK(rc > 0);
                        bool named = false;
                        for (int i = 0; i < rc; ++i) {
                            char kname[256];
                            CHECK(yp_op_kernel(e, i, kname, sizeof(kname)) == YP_OK);
                            named |= !strcmp(kname, "attention_stream_kernel");
                        }
                        CHECK(named == in_scope);
                        CHECK(yp_debug_host_selftest(e) > 0);
                    } else CHECK(rc == YP_ERR_ARG && strstr(yp_last_error(), "attention tokens"));
                }
                // the wide-head form: form 1's scope, and bf16 v10-M (36-wide keys) on its own kernel
                CHECK(yp_set_attention_form(e, 3) == YP_OK);
                {
                    const bool narrow = fam != YP_FAMILY_V8 && d.dtype == YP_BF16 && !(fam == YP_FAMILY_V10 && d.variant == 'm');
                    const bool wide = fam == YP_FAMILY_V10 && d.variant == 'm' && d.dtype == YP_BF16;
                    const int rc = yp_plan(e, 1, 2560, 1472);
                    if (fam == YP_FAMILY_V8 || narrow || wide) {
                        CHECK(rc > 0);
                        bool named = false, named_wide = false;
                        for (int i = 0; i < rc; ++i) {
                            char kname[256];
                            CHECK(yp_op_kernel(e, i, kname, sizeof(kname)) == YP_OK);
                            named |= !strcmp(kname, "attention_stream_kernel");
                            named_wide |= !strcmp(kname, "attention_stream_wide_kernel");
                        }
                        CHECK(named == narrow && named_wide == wide);
                        CHECK(yp_debug_host_selftest(e) > 0);
                    } else CHECK(rc == YP_ERR_ARG && strstr(yp_last_error(), "attention tokens"));
                }
                CHECK(yp_set_attention_form(e, 0) == YP_OK);
                // the fp32 switch, a bit set too: under 1 fp32 engines with 32-wide keys plan 3680 tokens on the fp32 streaming kernel, under 3
                // those plan as under 1 and fp32 v10-M (36-wide keys) on its own kernel; bf16 engines ignore it
                CHECK(yp_set_attention_f32_stream(e, 2) == YP_ERR_ARG && yp_set_attention_f32_stream(nullptr, 3) == YP_ERR_ARG);
                for (int on : {1, 3}) {
                    CHECK(yp_set_attention_f32_stream(e, on) == YP_OK);
                    const bool m = fam == YP_FAMILY_V10 && d.variant == 'm';
                    const bool narrow = fam != YP_FAMILY_V8 && d.dtype == YP_F32 && !m;
                    const bool wide = m && d.dtype == YP_F32 && on == 3;
                    const int rc = yp_plan(e, 1, 2560, 1472);
                    if (fam == YP_FAMILY_V8 || narrow || wide) {
                        CHECK(rc > 0);
                        bool named = false, named_wide = false;
                        for (int i = 0; i < rc; ++i) {
                            char kname[256];
                            CHECK(yp_op_kernel(e, i, kname, sizeof(kname)) == YP_OK);
                            named |= !strcmp(kname, "attention_stream_f32_kernel");
                            named_wide |= !strcmp(kname, "attention_stream_wide_f32_kernel");
                        }
                        CHECK(named == narrow && named_wide == wide);
                        CHECK(yp_debug_host_selftest(e) > 0);
                    } else CHECK(rc == YP_ERR_ARG && strstr(yp_last_error(), "attention tokens"));
                    if (m && d.dtype == YP_F32) {                       // 2420 tokens: the first shape the generic kernel refuses for M
                        const int r2 = yp_plan(e, 1, 1408, 1760);
                        if (on == 3) CHECK(r2 > 0 && yp_debug_host_selftest(e) > 0);
                        else CHECK(r2 == YP_ERR_ARG && strstr(yp_last_error(), "at most 2364"));
                    }
                }
                CHECK(yp_set_attention_f32_stream(e, 0) == YP_OK);
                {
                    const int mb = yp_max_batch(e, 1280, 1280);
                    CHECK(mb >= 1 && yp_max_batch(e, 640, 640) >= mb);
                    CHECK(yp_plan(e, mb, 1280, 1280) > 0);
                    CHECK(yp_plan(e, mb + 1, 1280, 1280) == YP_ERR_ARG && strstr(yp_last_error(), "2^31"));
                    CHECK(yp_debug_host_selftest(e) > 0);                                                                  // (the plan at mb still stands)
                    CHECK(yp_max_batch(nullptr, 640, 640) == YP_ERR_ARG && yp_max_batch(e, 100, 640) == YP_ERR_ARG && yp_max_batch(e, 640, 0) == YP_ERR_ARG);
                }
                CHECK(yp_plan(e, shapes[0][0], shapes[0][1], shapes[0][2]) > 0);
                CHECK(yp_forward(e, nullptr, 1, 64, 64, nullptr, nullptr, nullptr, nullptr) < 0);
                CHECK(yp_destroy(e) == YP_OK);
            }
    {   // yp_debug_topk_anchors: every argument is checked before anything touches the device
        static uint32_t stub[4];
        const uint32_t* mk[3] = {stub, stub, stub};
        const uint32_t* mk_hole[3] = {stub, nullptr, stub};
        const int hw[3][2] = {{100, 96}, {50, 48}, {25, 24}};
        const int hw_zero[3][2] = {{100, 96}, {0, 48}, {25, 24}};
        const int hw_big[3][2] = {{512, 512}, {128, 256}, {1, 1}};                      // YP_MAX_ANCHORS + 1
        int32_t* sel = (int32_t*)stub;
        CHECK(yp_debug_topk_anchors(nullptr, 1, hw, 300, sel, stub, nullptr) == YP_ERR_ARG);
        CHECK(yp_debug_topk_anchors(mk, 1, nullptr, 300, sel, stub, nullptr) == YP_ERR_ARG);
        CHECK(yp_debug_topk_anchors(mk, 1, hw, 300, nullptr, stub, nullptr) == YP_ERR_ARG);
        CHECK(yp_debug_topk_anchors(mk, 1, hw, 300, sel, nullptr, nullptr) == YP_ERR_ARG);
        CHECK(yp_debug_topk_anchors(mk, 0, hw, 300, sel, stub, nullptr) == YP_ERR_ARG);
        CHECK(yp_debug_topk_anchors(mk, 1, hw, 0, sel, stub, nullptr) == YP_ERR_ARG);
        CHECK(yp_debug_topk_anchors(mk, 1, hw, 513, sel, stub, nullptr) == YP_ERR_ARG);
        CHECK(yp_debug_topk_anchors(mk_hole, 1, hw, 300, sel, stub, nullptr) == YP_ERR_ARG);
        CHECK(yp_debug_topk_anchors(mk, 1, hw_zero, 300, sel, stub, nullptr) == YP_ERR_ARG);
        CHECK(yp_debug_topk_anchors(mk, 1, hw_big, 300, sel, stub, nullptr) == YP_ERR_ARG);
    }
    yp_model_desc bad{'q', 80, 0, 0, 300, 0};
    yp_engine* e = nullptr;
    CHECK(yp_create(&bad, 0, &e) < 0);
    // EfficientNet-B3 classifier (yp_cls_*): create, weight table, set_weight with its error paths, refusal without a device, destroy
    for (int dtype = 0; dtype < 2; ++dtype) {
        yp_cls* c = nullptr;
        CHECK(yp_cls_create(3, dtype, 0, &c) == YP_OK);
        const int nw = yp_cls_weight_count(c);
        CHECK(nw > 0);
        for (int i = 0; i < nw; ++i) {
            char name[256];
            int64_t shp[4];
            int nd = 0;
            CHECK(yp_cls_weight_info(c, i, name, sizeof(name), shp, &nd) == YP_OK);
            size_t n = 1;
            for (int k = 0; k < nd; ++k) n *= (size_t)shp[k];
            std::vector<float> w(n, 0.25f);
            if (i < 2) {
                int64_t bad[4] = {shp[0] + 1, shp[1], shp[2], shp[3]};
                CHECK(yp_cls_set_weight(c, name, w.data(), bad, nd) < 0);
                CHECK(yp_cls_set_weight(c, "_blocks.99._fc.weight", w.data(), shp, nd) < 0);
                CHECK(yp_cls_finalize(c) < 0);                           // missing weights
            }
            CHECK(yp_cls_set_weight(c, name, w.data(), shp, nd) == YP_OK);
        }
        CHECK(yp_cls_weight_info(c, nw, nullptr, 0, nullptr, nullptr) < 0);
        char tn[8];
        int dims[4];
        for (int i = 0; i < yp_cls_tensor_count(c); ++i) CHECK(yp_cls_tensor_info(c, i, tn, sizeof(tn), dims) == YP_OK);
        float tmp[4];
        CHECK(yp_cls_tensor_read(c, 0, tmp) < 0);                         // no forward yet
        CHECK(yp_cls_finalize(c) < 0);                                    // no device here: must refuse, not fall back
        CHECK(yp_cls_destroy(c) == YP_OK);
    }
    for (int v : {0, 4, 5, 7}) {
        yp_cls* c = nullptr;
        CHECK(yp_cls_create(v, 1, 0, &c) < 0 && c == nullptr);
    }
    // U^2-Net-P clip path (yp_u2net_forward_crops): every argument check runs before the device is touched
    for (int dtype = 0; dtype < 2; ++dtype) {
        yp_u2net* u = nullptr;
        CHECK(yp_u2net_create('p', dtype, 0, &u) == YP_OK);
        static uint8_t frame_stub[16];                                   // never read: every call below is refused first
        const int32_t ok_win[8] = {0, 0, 380, 380, 900, 340, 1280, 720};
        const int32_t ok_idx[2] = {0, 1};
        uint8_t mask_stub[1];
        CHECK(yp_u2net_forward_crops(u, nullptr, 2, 720, 1280, ok_win, ok_idx, 2, 380, 380, nullptr, nullptr, nullptr, nullptr) == YP_ERR_ARG);
        CHECK(yp_u2net_forward_crops(u, frame_stub, 2, 720, 1280, ok_win, ok_idx, 2, 31, 380, nullptr, nullptr, nullptr, nullptr) == YP_ERR_ARG);
        CHECK(yp_u2net_forward_crops(u, frame_stub, 2, 720, 1280, ok_win, ok_idx, 30, 380, 380, nullptr, nullptr, nullptr, nullptr) == YP_ERR_ARG);
        const int32_t bad_idx[2] = {0, 2};
        CHECK(yp_u2net_forward_crops(u, frame_stub, 2, 720, 1280, ok_win, bad_idx, 2, 380, 380, nullptr, nullptr, nullptr, nullptr) == YP_ERR_ARG);
        const int32_t dup_idx[2] = {1, 1};
        CHECK(yp_u2net_forward_crops(u, frame_stub, 2, 720, 1280, ok_win, dup_idx, 2, 380, 380, nullptr, nullptr, mask_stub, nullptr) == YP_ERR_ARG);
        const int32_t outside[4] = {1000, 0, 1380, 380}, wide[4] = {0, 0, 381, 380}, empty[4] = {5, 5, 5, 100};
        for (const int32_t* w : {outside, wide, empty})
            CHECK(yp_u2net_forward_crops(u, frame_stub, 2, 720, 1280, w, ok_idx, 1, 380, 380, nullptr, nullptr, nullptr, nullptr) == YP_ERR_ARG);
        // valid arguments: refused only because no weights were finalized (no device here)
        CHECK(yp_u2net_forward_crops(u, frame_stub, 2, 720, 1280, ok_win, dup_idx, 2, 380, 380, nullptr, nullptr, nullptr, nullptr) == YP_ERR_STATE);
        // the plan's read-only view (yp_u2net_op_info): input + 112 REBNCONVs + 6 side convs + pools + up-samples, short buffers respected
        const int nops = yp_u2net_op_count(u);
        int nconv = 0;
        for (int i = 0; i < nops; ++i) {
            char on[8];
            int32_t info[YP_U2_OP_INFO + 1];
            info[YP_U2_OP_INFO] = 12345;
            CHECK(yp_u2net_op_info(u, i, on, sizeof(on), info, YP_U2_OP_INFO) == YP_U2_OP_INFO && info[YP_U2_OP_INFO] == 12345);
            CHECK(info[13] == -1);                                       // impl: nothing is chosen before a plan's first pass
            nconv += info[0] == 1;
            int32_t two[3] = {-7, -7, -7};
            CHECK(yp_u2net_op_info(u, i, nullptr, 0, two, 2) == YP_U2_OP_INFO && two[0] == info[0] && two[2] == -7);
        }
        CHECK(nconv == 118);
        CHECK(yp_u2net_op_info(u, nops, nullptr, 0, nullptr, 0) == YP_ERR_ARG && yp_u2net_op_info(u, -1, nullptr, 0, nullptr, 0) == YP_ERR_ARG);
        CHECK(yp_u2net_op_count(nullptr) == YP_ERR_ARG);
        CHECK(yp_u2net_destroy(u) == YP_OK);
    }
    // clip form of the YOLO segmentation pass (yp_masks_frames, yp_masks_frames_input, yp_letterbox_batch): bad arguments fail before
    // anything is launched
    for (int task = 0; task < 2; ++task) {
        yp_model_desc d{'n', 80, task, YP_F32, 300, YP_FAMILY_V10};
        yp_engine* eng = nullptr;
        CHECK(yp_create(&d, 0, &eng) == YP_OK);
        static float stub_f[8];                                          // never read: every call below is refused first
        static uint8_t stub_u8[16];
        const int32_t idx[3] = {0, 2, 2};
        CHECK(yp_masks_frames(nullptr, idx, 3, stub_f, 300 * 32, stub_f, 720, 1280, stub_u8, nullptr) == YP_ERR_ARG);
        CHECK(yp_masks_frames(eng, idx, -1, stub_f, 300 * 32, stub_f, 720, 1280, stub_u8, nullptr) == YP_ERR_ARG);
        CHECK(yp_masks_frames(eng, idx, 3, stub_f, 300 * 32, stub_f, 0, 1280, stub_u8, nullptr) == YP_ERR_ARG);
        CHECK(yp_masks_frames(eng, idx, 3, stub_f, 300 * 32, stub_f, 720, -5, stub_u8, nullptr) == YP_ERR_ARG);
        CHECK(yp_masks_frames(eng, idx, 3000, stub_f, 300 * 32, stub_f, 720, 1280, stub_u8, nullptr) == YP_ERR_ARG);   // k*oh*ow >= 2^31
        CHECK(yp_masks_frames(eng, nullptr, 3, stub_f, 300 * 32, stub_f, 720, 1280, stub_u8, nullptr) == YP_ERR_ARG);
        CHECK(yp_masks_frames(eng, idx, 3, nullptr, 300 * 32, stub_f, 720, 1280, stub_u8, nullptr) == YP_ERR_ARG);
        CHECK(yp_masks_frames(eng, idx, 3, stub_f, 300 * 32, nullptr, 720, 1280, stub_u8, nullptr) == YP_ERR_ARG);
        CHECK(yp_masks_frames(eng, idx, 3, stub_f, 300 * 32, stub_f, 720, 1280, nullptr, nullptr) == YP_ERR_ARG);
        CHECK(yp_masks_frames(eng, idx, 3, stub_f, 31, stub_f, 720, 1280, stub_u8, nullptr) == YP_ERR_ARG);
        // valid arguments: a detect engine has no prototypes, a segment engine has run no forward (no device here)
        CHECK(yp_masks_frames(eng, idx, 3, stub_f, 300 * 32, stub_f, 720, 1280, stub_u8, nullptr) == YP_ERR_STATE);
        CHECK(yp_masks_frames(eng, idx, 0, stub_f, 300 * 32, stub_f, 720, 1280, stub_u8, nullptr) == YP_ERR_STATE);
        // the process_mask form (yp_masks_frames_input): the same checks, in the same order
        CHECK(yp_masks_frames_input(nullptr, idx, 3, stub_f, 300 * 32, stub_f, 384, 640, stub_u8, nullptr) == YP_ERR_ARG);
        CHECK(yp_masks_frames_input(eng, idx, -1, stub_f, 300 * 32, stub_f, 384, 640, stub_u8, nullptr) == YP_ERR_ARG);
        CHECK(yp_masks_frames_input(eng, idx, 3, stub_f, 300 * 32, stub_f, 0, 640, stub_u8, nullptr) == YP_ERR_ARG);
        CHECK(yp_masks_frames_input(eng, idx, 3, stub_f, 300 * 32, stub_f, 384, -5, stub_u8, nullptr) == YP_ERR_ARG);
        CHECK(yp_masks_frames_input(eng, idx, 9000, stub_f, 300 * 32, stub_f, 384, 640, stub_u8, nullptr) == YP_ERR_ARG);   // k*oh*ow >= 2^31
        CHECK(yp_masks_frames_input(eng, idx, 70000, stub_f, 300 * 32, stub_f, 4, 4, stub_u8, nullptr) == YP_ERR_ARG);      // k > 65535
        CHECK(yp_masks_frames_input(eng, nullptr, 3, stub_f, 300 * 32, stub_f, 384, 640, stub_u8, nullptr) == YP_ERR_ARG);
        CHECK(yp_masks_frames_input(eng, idx, 3, nullptr, 300 * 32, stub_f, 384, 640, stub_u8, nullptr) == YP_ERR_ARG);
        CHECK(yp_masks_frames_input(eng, idx, 3, stub_f, 300 * 32, nullptr, 384, 640, stub_u8, nullptr) == YP_ERR_ARG);
        CHECK(yp_masks_frames_input(eng, idx, 3, stub_f, 300 * 32, stub_f, 384, 640, nullptr, nullptr) == YP_ERR_ARG);
        CHECK(yp_masks_frames_input(eng, idx, 3, stub_f, 31, stub_f, 384, 640, stub_u8, nullptr) == YP_ERR_ARG);
        CHECK(yp_masks_frames_input(eng, idx, 3, stub_f, 300 * 32, stub_f, 384, 640, stub_u8, nullptr) == YP_ERR_STATE);
        CHECK(yp_masks_frames_input(eng, idx, 0, stub_f, 300 * 32, stub_f, 384, 640, stub_u8, nullptr) == YP_ERR_STATE);
        CHECK(yp_destroy(eng) == YP_OK);
    }
    // the clip form of auto_segment (yp_id_masks_frames, yp_id_masks_frames_workspace): every check runs before the device is touched, the
    // query is host arithmetic on the engine's plan
    for (int task = 0; task < 2; ++task) {
        yp_model_desc d{'n', 80, task, YP_F32, 300, YP_FAMILY_V10};
        yp_engine* eng = nullptr;
        CHECK(yp_create(&d, 0, &eng) == YP_OK);
        static float stub_f[8];                                          // never read or written: every call below is refused first
        static int64_t stub_ids[2];
        static int32_t stub_kept[2];
        const int32_t idx[3] = {0, 3, 3}, off[4] = {0, 2, 2, 5};
        auto call = [&](yp_engine* e, const int32_t* fi, const int32_t* ro, int k, int oh, int ow, int rh, int rw) {
            return yp_id_masks_frames(e, fi, ro, k, stub_f, stub_f, oh, ow, rh, rw, stub_ids, stub_kept, 1, 100, nullptr);
        };
        CHECK(yp_id_masks_frames_workspace(eng, 5, 3, 96, 160, 96, 160) == 0);                       // no plan yet
        CHECK(call(eng, idx, off, 3, 96, 160, 96, 160) == YP_ERR_STATE);
        CHECK(yp_plan(eng, 4, 96, 160) > 0);
        CHECK(call(nullptr, idx, off, 3, 96, 160, 96, 160) == YP_ERR_ARG);
        CHECK(call(eng, idx, off, 0, 96, 160, 96, 160) == YP_ERR_ARG && strstr(yp_last_error(), "yp_id_masks_frames"));
        CHECK(call(eng, nullptr, off, 3, 96, 160, 96, 160) == YP_ERR_ARG);
        CHECK(call(eng, idx, nullptr, 3, 96, 160, 96, 160) == YP_ERR_ARG);
        CHECK(yp_id_masks_frames(eng, idx, off, 3, stub_f, stub_f, 96, 160, 96, 160, nullptr, stub_kept, 1, 100, nullptr) == YP_ERR_ARG);
        CHECK(yp_id_masks_frames(eng, idx, off, 3, nullptr, stub_f, 96, 160, 96, 160, stub_ids, stub_kept, 1, 100, nullptr) == YP_ERR_ARG);
        CHECK(yp_id_masks_frames(eng, idx, off, 3, stub_f, nullptr, 96, 160, 96, 160, stub_ids, stub_kept, 1, 100, nullptr) == YP_ERR_ARG);
        CHECK(yp_id_masks_frames(eng, idx, off, 3, stub_f, stub_f, 96, 160, 96, 160, stub_ids, nullptr, 1, 100, nullptr) == YP_ERR_ARG);
        const int32_t off_start[4] = {1, 2, 2, 5}, off_down[4] = {0, 2, 1, 5}, off_many[4] = {0, 2, 2 + YP_MAX_MASKS + 1, 2 + YP_MAX_MASKS + 1};
        for (const int32_t* ro : {off_start, off_down, off_many}) CHECK(call(eng, idx, ro, 3, 96, 160, 96, 160) == YP_ERR_ARG);
        CHECK(call(eng, idx, off, 3, 0, 160, 96, 160) == YP_ERR_ARG);
        CHECK(call(eng, idx, off, 3, 96, 160, 144, -1) == YP_ERR_ARG);
        CHECK(call(eng, idx, off, 3, 96, 160, 5, 160) == YP_ERR_ARG && strstr(yp_last_error(), "16x"));
        CHECK(call(eng, idx, off, 3, 46341, 46341, 46341, 46341) == YP_ERR_ARG && strstr(yp_last_error(), "2^31"));
        CHECK(call(eng, idx, off, 3, 65536, 4096, 4096, 32768) == YP_ERR_ARG);                       // oh * rw = 2^31
        {
            std::vector<int32_t> fi(140, 0), ro(141);
            for (int j = 0; j <= 140; ++j) ro[j] = YP_MAX_MASKS * j;                                  // 67200 masks in all
            CHECK(call(eng, fi.data(), ro.data(), 140, 96, 160, 96, 160) == YP_ERR_ARG && strstr(yp_last_error(), "65535"));
            const int32_t ro4[5] = {0, 300, 600, 900, 1200};
            CHECK(call(eng, fi.data(), ro4, 4, 2048, 2048, 2048, 2048) == YP_ERR_ARG && strstr(yp_last_error(), "2^32"));
            std::vector<int32_t> fk(65536, 0), rk(65537, 0);
            CHECK(call(eng, fk.data(), rk.data(), 65536, 96, 160, 96, 160) == YP_ERR_ARG);
        }
        if (task == YP_TASK_SEGMENT) {
            const int32_t idx_hi[3] = {0, 4, 3}, idx_lo[3] = {0, -1, 3};
            CHECK(call(eng, idx_hi, off, 3, 96, 160, 96, 160) == YP_ERR_ARG && call(eng, idx_lo, off, 3, 96, 160, 96, 160) == YP_ERR_ARG);
            // valid arguments, the 16x limit itself and a frame at the mask limit: a plan, but no forward (no device here)
            const int32_t off_full[4] = {0, YP_MAX_MASKS, YP_MAX_MASKS, YP_MAX_MASKS + 3};
            CHECK(call(eng, idx, off, 3, 96, 160, 96, 160) == YP_ERR_STATE && call(eng, idx, off, 3, 96, 160, 6, 10) == YP_ERR_STATE);
            CHECK(call(eng, idx, off_full, 3, 96, 160, 144, 240) == YP_ERR_STATE);
            const int32_t off_none[4] = {0, 0, 0, 0};
            CHECK(yp_id_masks_frames(eng, idx, off_none, 3, nullptr, nullptr, 96, 160, 96, 160, stub_ids, nullptr, 1, 100, nullptr) == YP_ERR_STATE);
            // the query: 256-byte blocks, growing with rows and frames, 0 for what the call refuses
            size_t prev = 0;
            for (int n : {0, 1, 17, 480, 5000}) {
                const size_t a = yp_id_masks_frames_workspace(eng, n, 1, 96, 160, 96, 160), b = yp_id_masks_frames_workspace(eng, n, 64, 96, 160, 144, 240);
                CHECK(a > prev && b > a && a % 256 == 0 && b % 256 == 0);
                prev = a;
            }
            CHECK(yp_id_masks_frames_workspace(eng, 5, 0, 96, 160, 96, 160) == 0 && yp_id_masks_frames_workspace(eng, 70000, 2, 96, 160, 96, 160) == 0);
            CHECK(yp_id_masks_frames_workspace(eng, 5, 2, 96, 160, 5, 10) == 0 && yp_id_masks_frames_workspace(eng, 5, 2, 46341, 46341, 46341, 46341) == 0);
            CHECK(yp_id_masks_frames_workspace(nullptr, 5, 2, 96, 160, 96, 160) == 0);
        } else {
            CHECK(call(eng, idx, off, 3, 96, 160, 96, 160) == YP_ERR_STATE);                         // a detect engine has no prototypes
            CHECK(yp_id_masks_frames_workspace(eng, 5, 2, 96, 160, 96, 160) == 0);
        }
        CHECK(yp_destroy(eng) == YP_OK);
    }
    {
        // yp_mask_contours_scaled: bad arguments fail before anything is launched; n = 0 launches nothing
        static uint8_t m[16];
        static int32_t pts[64], cnt[4], parts[8];
        static double rect[8];
        CHECK(yp_mask_contours_scaled(m, -1, 384, 640, YP_CONTOURS_ALL, 16, pts, cnt, parts, 4, rect, 720, 1280, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_scaled(m, 1, 0, 640, YP_CONTOURS_ALL, 16, pts, cnt, parts, 4, rect, 720, 1280, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_scaled(m, 1, 384, -1, YP_CONTOURS_ALL, 16, pts, cnt, parts, 4, rect, 720, 1280, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_scaled(m, 1, 384, 640, YP_CONTOURS_ALL, 1, pts, cnt, parts, 4, rect, 720, 1280, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_scaled(m, 1, 384, 640, YP_CONTOURS_ALL, 16, pts, cnt, parts, 4, rect, 0, 1280, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_scaled(m, 1, 384, 640, YP_CONTOURS_ALL, 16, pts, cnt, parts, 4, rect, 720, -3, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_scaled(m, 1, 384, 640, 7, 16, pts, cnt, parts, 4, rect, 720, 1280, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_scaled(nullptr, 1, 384, 640, YP_CONTOURS_ALL, 16, pts, cnt, parts, 4, rect, 720, 1280, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_scaled(m, 1, 384, 640, YP_CONTOURS_ALL, 16, nullptr, cnt, parts, 4, rect, 720, 1280, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_scaled(m, 1, 384, 640, YP_CONTOURS_ALL, 16, pts, nullptr, parts, 4, rect, 720, 1280, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_scaled(m, 1, 384, 640, YP_CONTOURS_ALL, 16, pts, cnt, parts, 1, rect, 720, 1280, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_scaled(m, 1, 50000, 50000, YP_CONTOURS_ALL, 16, pts, cnt, parts, 4, rect, 720, 1280, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_scaled(m, 0, 384, 640, YP_CONTOURS_ALL, 16, pts, cnt, parts, 4, rect, 720, 1280, nullptr) == YP_OK);
    }
    {
        // yp_mask_contours_merge: the tile-list sizes, the workspace arithmetic and the refusals are host code; nothing is launched
        const int T = YP_CONTOURS_MERGE_TILE, G = 4 * YP_CONTOURS_MERGE_TILE;
        int tile = 0, scan = 0;
        yp_mask_contours_merge_sizes(&tile, &scan);
        yp_mask_contours_merge_sizes(nullptr, nullptr);
        CHECK(tile == T && scan == YP_CONTOURS_MERGE_SCAN_BLOCK);
        {
            const int32_t two[2] = {T + 1, G + 1}, big[3] = {6000, 6000, 3000}, bad[3] = {3, 0, 3}, top[2] = {YP_CONTOURS_MERGE_MAX_PTS, YP_CONTOURS_MERGE_MAX_PTS};
            CHECK(yp_mask_contours_merge_tiles(two, 2) == 4 && yp_mask_contours_merge_tiles(two, 1) == 0 && yp_mask_contours_merge_tiles(nullptr, 2) == 0);
            CHECK(yp_mask_contours_merge_tiles(big, 3) == (unsigned long long)((6000 + T - 1) / T) * (((6000 + G - 1) / G) + ((3000 + G - 1) / G)));
            CHECK(yp_mask_contours_merge_tiles(bad, 3) == 0);
            CHECK(yp_mask_contours_merge_tiles(top, 2) == (unsigned long long)(YP_CONTOURS_MERGE_MAX_PTS / T) * (YP_CONTOURS_MERGE_MAX_PTS / G));
            std::vector<int32_t> many(YP_CONTOURS_LARGE_MAX_STARTS, 4);
            CHECK(yp_mask_contours_merge_tiles(many.data(), (int)many.size()) == (unsigned long long)many.size() - 1);
        }
        CHECK(yp_mask_contours_merge_workspace(0, 65) == 0 && yp_mask_contours_merge_workspace(-1, 65) == 0 && yp_mask_contours_merge_workspace(65536, 65) == 0);
        CHECK(yp_mask_contours_merge_workspace(1, 1) == 0 && yp_mask_contours_merge_workspace(1, YP_CONTOURS_LARGE_MAX_STARTS + 2) == 0);
        const size_t per = yp_mask_contours_merge_workspace(1, 65) - 16;
        CHECK(per > 0 && per % 16 == 0);
        for (int n : {1, 2, 7, 480, 65535})
            CHECK(yp_mask_contours_merge_workspace(n, 65) == (size_t)((2 * (n + 1) + 3) / 4) * 16 + (size_t)n * per);
        CHECK(yp_mask_contours_merge_workspace(65535, YP_CONTOURS_LARGE_MAX_STARTS + 1) > ((size_t)1 << 36));      // (size_t arithmetic: no 32-bit wrap)
        static int32_t pts[64], cnt[4], parts[8], out[80], outc[4];
        alignas(16) static int32_t ws[4096];
        const size_t need = yp_mask_contours_merge_workspace(2, 4);
        CHECK(need > 0 && need <= sizeof ws);
        CHECK(yp_mask_contours_merge(pts, cnt, parts, -1, 16, 4, out, outc, 20, ws, need, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_merge(pts, cnt, parts, 65536, 16, 4, out, outc, 20, ws, need, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_merge(pts, cnt, parts, 2, 1, 4, out, outc, 20, ws, need, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_merge(pts, cnt, parts, 2, YP_CONTOURS_MERGE_MAX_PTS + 1, 4, out, outc, 20, ws, need, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_merge(pts, cnt, parts, 2, 16, 1, out, outc, 20, ws, need, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_merge(pts, cnt, parts, 2, 16, YP_CONTOURS_LARGE_MAX_STARTS + 2, out, outc, 20, ws, need, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_merge(pts, cnt, parts, 2, 16, 4, out, outc, 0, ws, need, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_merge(nullptr, cnt, parts, 2, 16, 4, out, outc, 20, ws, need, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_merge(pts, nullptr, parts, 2, 16, 4, out, outc, 20, ws, need, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_merge(pts, cnt, nullptr, 2, 16, 4, out, outc, 20, ws, need, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_merge(pts, cnt, parts, 2, 16, 4, nullptr, outc, 20, ws, need, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_merge(pts, cnt, parts, 2, 16, 4, out, nullptr, 20, ws, need, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_merge((const int32_t*)((const char*)pts + 4), cnt, parts, 2, 16, 4, out, outc, 20, ws, need, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_merge(pts, cnt, parts, 2, 16, 4, out, outc, 20, nullptr, need, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_merge(pts, cnt, parts, 2, 16, 4, out, outc, 20, (char*)ws + 8, need, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_merge(pts, cnt, parts, 2, 16, 4, out, outc, 20, ws, need - 1, nullptr) == YP_ERR_ARG);
        CHECK(yp_mask_contours_merge(pts, cnt, parts, 0, 16, 4, out, outc, 20, nullptr, 0, nullptr) == YP_OK);       // nothing to do
    }
    {
        static uint8_t src[16], dst[16];                                 // never read: every call below is refused first or launches nothing
        CHECK(yp_letterbox_batch(nullptr, 2, 720, 1280, dst, 384, 640, 360, 640, 12, 0, 114, nullptr) == YP_ERR_ARG);
        CHECK(yp_letterbox_batch(src, 2, 720, 1280, nullptr, 384, 640, 360, 640, 12, 0, 114, nullptr) == YP_ERR_ARG);
        CHECK(yp_letterbox_batch(src, -1, 720, 1280, dst, 384, 640, 360, 640, 12, 0, 114, nullptr) == YP_ERR_ARG);
        CHECK(yp_letterbox_batch(src, 70000, 4, 4, dst, 4, 4, 4, 4, 0, 0, 114, nullptr) == YP_ERR_ARG);
        CHECK(yp_letterbox_batch(src, 2, 720, 1280, dst, 384, 640, 360, 640, 30, 0, 114, nullptr) == YP_ERR_ARG);     // past the bottom
        CHECK(yp_letterbox_batch(src, 2, 720, 1280, dst, 384, 640, 360, 640, 12, 0, 256, nullptr) == YP_ERR_ARG);
        CHECK(yp_letterbox_batch(src, 2, 0, 1280, dst, 384, 640, 360, 640, 12, 0, 114, nullptr) == YP_ERR_ARG);
        CHECK(yp_letterbox_batch(src, 800, 720, 1280, dst, 384, 640, 360, 640, 12, 0, 114, nullptr) == YP_ERR_ARG);  // > 2^31 bytes
        CHECK(yp_letterbox_batch(src, 0, 720, 1280, dst, 384, 640, 360, 640, 12, 0, 114, nullptr) == YP_OK);         // nothing to do
    }
    printf("asan_host: ok (%ld scheduled launches walked)\n", launches);
    return 0;
}
