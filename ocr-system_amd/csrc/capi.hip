// extern "C" surface of liblumina_ocr.so (declared in include/lumina_ocr.h). Nothing throws.
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/lumina_ocr.h"
#include "dbpost.h"
#include "deskew.h"
#include "engine.h"
#include "marks.h"
#include "barcodes.h"
#include "qrcodes.h"
#include "datamatrix.h"
#include "aztec.h"
#include "ops.h"
#include "orient.h"
#include "compose.h"
#include "resize.h"
#include "runs.h"
#include "jpeg.h"
#include "jpegdec.h"
#include "lzw.h"
#include "jp2dec.h"
#include "pngdec.h"
#include "vp8dec.h"
#include "webpdec.h"
#include "webp_parse.h"
#include "ccitt.h"
#include "jbig2.h"
#include "jbig2_parse.h"
#include "stem_conv.h"
#include "tables.h"

#define API_TRY try {
#define API_CATCH(h)                                                             \
    }                                                                            \
    catch (const std::exception& e) { return locr_fail(h, "exception", e.what()); } \
    catch (...) { return locr_fail(h, "exception", "unknown"); }

// every entry that allocates, copies or launches binds the calling thread to the handle's device first: provider threads
// (asyncio.to_thread workers) start on device 0 whatever device the handle was created on.  The thread's previous device is put
// back when the entry returns (a host that keeps its own current device — torch without an explicit device, a second engine on
// another GPU — is not silently rebound).
namespace {
struct DeviceGuard {
    int prev = -1;
    hipError_t err;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        err = hipSetDevice(dev);
        if (prev == dev) prev = -1;   // nothing to restore
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
}  // namespace
#define BIND(h)                                                                                              \
    if (!(h)) return 1;                                                                                      \
    DeviceGuard _device_guard((h)->device);                                                                  \
    if (_device_guard.err != hipSuccess) return locr_fail((h), "hipSetDevice", hipGetErrorString(_device_guard.err))

// an entry's last step: 0, or the HIP error recorded in the handle
static int hip_rc(lumina_ocr* h, const char* what, hipError_t e) { return e == hipSuccess ? 0 : locr_fail(h, what, hipGetErrorString(e)); }

// waits for the device, then hands every timed launch and its milliseconds to f and drops the records (and their events)
template <class F> static int drain_launches(lumina_ocr* h, const char* what, F&& f) {
    if (hipDeviceSynchronize() != hipSuccess) return locr_fail(h, what, "sync failed");
    for (const LaunchRecord& r : h->launches) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, r.e0.get(), r.e1.get()) != hipSuccess) t = 0.f;
        f(r, t);
    }
    h->launches.clear();
    return 0;
}

// Pages are processed in groups that bound the workspace, whose size for a group of nb pages is ws(nb).  for_page_groups reserves it
// and runs body(b0, nb) for every group of n pages (body returns 0, or 1 after locr_fail).  A group is the handle's post_group;
// passes whose worst case is large (run lists, run slots, masks) take fit_group of it: at most n, and halved until it fits 1 GiB.
template <class WS> static int fit_group(int group, int n, WS&& ws) {
    if (group > n) group = n;
    while (group > 1 && ws(group) > ((size_t)1 << 30)) group = (group + 1) / 2;
    return group;
}
template <class WS, class Body> static int for_page_groups(lumina_ocr* h, int n, int group, WS&& ws, Body&& body) {
    for (int b0 = 0; b0 < n; b0 += group) {
        const int nb = n - b0 < group ? n - b0 : group;
        if (eng_ws_reserve(h, ws(nb)) || body(b0, nb)) return 1;
    }
    return 0;
}

// What the five matrix-code entries share.  A page group's base pointers: rows of 12 ints, data rows of row_len elements of T, one count
// and (optionally) one finder or candidate count a page, the masks [H][ceil(W / 64)] a page.
template <class T> struct CodeGroup {
    const uint8_t* rgb; int nb; int32_t* codes; T* data; int32_t* counts; int32_t* slot_counts; const unsigned long long* mask_in; unsigned long long* mask_out;
    // the fields every reader's Params names alike
    template <class P> void bind(P& p) const { p.rgb = rgb; p.B = nb; p.codes = codes; p.counts = counts; p.mask_in = mask_in; p.mask_out = mask_out; }
};
// The checks in their order (handle, no pages, pointers, the caller's parameter message: nullptr when they are fine, the sides), the
// device, the page groups (ws(nb): the workspace of nb pages; the run list is sized for its worst case, 28 to 60 bytes per two pixels),
// and per group launch(group, workspace, its capacity).
template <class T, class WS, class Launch>
static int matrix_codes(lumina_ocr_t* h, const char* what, const char* bad_params, const uint8_t* pages_dev, int n, int height, int width, int max_codes,
                        int row_len, int32_t* codes_dev, T* data_dev, int32_t* counts_dev, int32_t* slot_counts_dev, const uint64_t* mask_in_dev,
                        uint64_t* mask_out_dev, WS ws, Launch launch) {
    if (!h) return 1;
    if (n == 0) return 0;
    if (!pages_dev || !codes_dev || !data_dev || !counts_dev || n < 0) return locr_fail(h, what, "bad arguments");
    if (bad_params) return locr_fail(h, what, bad_params);
    if (ws(1) == 0) return locr_fail(h, what, "bad dimensions (sides 1..65535)");
    BIND(h);
    API_TRY
    const size_t nw = ((size_t)width + 63) / 64;
    return for_page_groups(h, n, fit_group(h->post_group, n, ws), ws, [&](int b0, int nb) {
        CodeGroup<T> g{};
        g.rgb = pages_dev + (size_t)b0 * height * width * 3; g.nb = nb;
        g.codes = codes_dev + (size_t)b0 * max_codes * 12; g.data = data_dev + (size_t)b0 * max_codes * row_len; g.counts = counts_dev + b0;
        g.slot_counts = slot_counts_dev ? slot_counts_dev + b0 : nullptr;
        g.mask_in = mask_in_dev ? reinterpret_cast<const unsigned long long*>(mask_in_dev) + (size_t)b0 * height * nw : nullptr;
        g.mask_out = mask_out_dev ? reinterpret_cast<unsigned long long*>(mask_out_dev) + (size_t)b0 * height * nw : nullptr;
        return hip_rc(h, what, launch(g, h->ws.get(), h->ws.cap));
    });
    API_CATCH(h)
}

extern "C" {

const char* lumina_ocr_version(void) { return "lumina-ocr-mi355x 0.1 (gfx950)"; }

int lumina_ocr_create(int device, lumina_ocr_t** out) {
    if (!out) return 1;
    *out = nullptr;
    lumina_ocr* eng = new (std::nothrow) lumina_ocr();
    if (!eng) return 1;
    eng->device = device;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        eng->err = "no HIP device " + std::to_string(device) + " (device count " + std::to_string(ndev) + ")";
        *out = eng;  // handle is returned so the caller can read the error
        return 2;
    }
    if (hipSetDevice(device) != hipSuccess) { eng->err = "hipSetDevice failed"; *out = eng; return 2; }
    if (const char* e = getenv("LUMINA_RING_ORIENT")) eng->ring_orient = atoi(e) < 0 ? -1 : (atoi(e) != 0);   // developer A/B (profiler runs)
    if (getenv("LUMINA_CONV_NO_RING")) eng->conv_ring = false;
    if (getenv("LUMINA_BLOCKED")) eng->blocked_layout = atoi(getenv("LUMINA_BLOCKED")) != 0;
    *out = eng;
    return 0;
}

void lumina_ocr_destroy(lumina_ocr_t* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;   // (its device memory, pinned buffers and events are released by their owners)
}

const char* lumina_ocr_last_error(const lumina_ocr_t* h) { return h ? h->err.c_str() : "null handle"; }

int lumina_ocr_set_option(lumina_ocr_t* h, const char* key, int value) {
    if (!h || !key) return 1;
    if (!strcmp(key, "det_sub_batch")) h->det_sub_batch = value > 0 ? value : 1;
    else if (!strcmp(key, "rec_sub_batch")) h->rec_sub_batch = value > 0 ? value : 1;
    else if (!strcmp(key, "cls_sub_batch")) h->cls_sub_batch = value > 0 ? value : 1;
    else if (!strcmp(key, "keep_taps")) h->keep_taps = value < 0 || value > 2 ? 0 : value;
    else if (!strcmp(key, "time_convs")) h->time_convs = value != 0;
    else if (!strcmp(key, "fuse_head")) h->fuse_head = value != 0;
    else if (!strcmp(key, "fuse_mb")) h->fuse_mb = value != 0;
    else if (!strcmp(key, "fuse_xproj")) h->fuse_xproj = value != 0;
    else if (!strcmp(key, "fuse_conv2_pool")) h->fuse_conv2_pool = value != 0;
    else if (!strcmp(key, "lstm_waves")) h->lstm_waves = value == 3 ? 3 : 12;
    else if (!strcmp(key, "seq_gemm_min")) h->seq_gemm_min = value >= 0 ? value : 128;
    else if (!strcmp(key, "fuse_pool")) h->fuse_pool = value != 0;
    else if (!strcmp(key, "fuse_stem")) h->fuse_stem = value != 0;
    else if (!strcmp(key, "fpn_multi")) h->fpn_multi = value != 0;
    else if (!strcmp(key, "fpn_compose")) h->fpn_compose = value != 0;
    else if (!strcmp(key, "fuse_short")) h->fuse_short = value != 0;
    else if (!strcmp(key, "conv_ring")) h->conv_ring = value != 0;
    else if (!strcmp(key, "blocked_layout")) h->blocked_layout = value != 0;
    else if (!strcmp(key, "conv_big_min")) h->conv_big_min = value >= 0 ? value : 1024;
    else if (!strcmp(key, "ring_orient")) h->ring_orient = value < 0 ? -1 : (value != 0);
    else if (!strcmp(key, "post_group")) h->post_group = value > 0 ? value : 1;
    else if (!strcmp(key, "tail_group")) h->tail_group = value > 0 ? value : 0;
    else if (!strcmp(key, "svtr_f16")) h->svtr_f16 = value < 0 ? -1 : (value != 0);
    else if (!strcmp(key, "png_sub_batch_mb")) h->pd_sub_batch_mb = value > 0 ? value : 1;
    else if (!strcmp(key, "webp_sub_batch_mb")) h->wp_sub_batch_mb = value > 0 ? value : 1;
    else if (!strcmp(key, "jp2_sub_batch_mb")) h->jp_sub_batch_mb = value > 0 ? value : 1;
    else if (!strcmp(key, "conv2d_variant")) h->conv2d_variant = value < 0 || value > 2 ? 0 : value;
    else return locr_fail(h, "set_option: unknown key", key);
    return 0;
}

int lumina_ocr_load_det_weights(lumina_ocr_t* h, const void* blob, size_t nbytes) {
    if (!h || !blob) return 1;
    BIND(h);
    API_TRY return eng_load_det(h, blob, nbytes); API_CATCH(h)
}
int lumina_ocr_load_rec_weights(lumina_ocr_t* h, const void* blob, size_t nbytes) {
    if (!h || !blob) return 1;
    BIND(h);
    API_TRY return eng_load_rec(h, blob, nbytes); API_CATCH(h)
}
int lumina_ocr_num_classes(const lumina_ocr_t* h) { return h ? h->num_classes : 0; }
int lumina_ocr_model_loaded(const lumina_ocr_t* h, int kind) {
    if (!h) return 0;
    return kind == 0 ? h->det_loaded : kind == 1 ? h->rec_loaded : kind == 2 ? h->cls_loaded : kind == 3 ? h->svtr.loaded : false;
}

int lumina_ocr_normalize(lumina_ocr_t* h, const uint8_t* img_dev, int n, int height, int width, int hp, int wp, const float scale[3],
                         const float shift[3], int layout_nchw, uint16_t* out_dev, void* stream) {
    if (!h || !img_dev || !out_dev || hp < height || wp < width) return locr_fail(h, "normalize", "bad arguments");
    BIND(h);
    return hip_rc(h, "normalize", normalize_launch(img_dev, out_dev, n, height, width, hp, wp, height, width, scale, shift, layout_nchw, (hipStream_t)stream));
}

int lumina_ocr_det_forward(lumina_ocr_t* h, const uint8_t* pages_dev, int batch, int height, int width, int hp, int wp, uint16_t* prob_dev,
                           void* stream) {
    if (!h || !pages_dev || !prob_dev) return locr_fail(h, "det_forward", "null argument");
    BIND(h);
    API_TRY return eng_det_forward(h, pages_dev, batch, height, width, hp, wp, prob_dev, (hipStream_t)stream); API_CATCH(h)
}

int lumina_ocr_det_postprocess(lumina_ocr_t* h, const uint16_t* prob_dev, int batch, int hp, int wp, int valid_h, int valid_w, float thresh,
                               float box_thresh, float unclip_ratio, int min_size, int max_boxes, int32_t* boxes_dev, float* scores_dev,
                               int32_t* counts_dev, void* stream) {
    if (!h || !prob_dev || !boxes_dev || !scores_dev || !counts_dev) return locr_fail(h, "det_postprocess", "null argument");
    if (batch <= 0 || max_boxes <= 0 || valid_h > hp || valid_w > wp) return locr_fail(h, "det_postprocess", "bad dimensions");
    BIND(h);
    API_TRY
    // ~66 MB per A4 page: worst-case run list + row-extreme segments and hull scratch of max_boxes page-high candidates
    return for_page_groups(h, batch, h->post_group, [&](int nb) { return dbpost_workspace_bytes(nb, hp, wp, max_boxes); }, [&](int b0, int nb) {
        DbPostParams p{};
        p.prob = prob_dev + (size_t)b0 * hp * wp; p.B = nb; p.Hp = hp; p.Wp = wp; p.valid_h = valid_h; p.valid_w = valid_w;
        p.thresh = thresh; p.box_thresh = box_thresh; p.unclip_ratio = unclip_ratio; p.min_size = min_size; p.max_boxes = max_boxes;
        p.boxes = boxes_dev + (size_t)b0 * max_boxes * 8; p.scores = scores_dev + (size_t)b0 * max_boxes; p.counts = counts_dev + b0;
        return hip_rc(h, "det_postprocess", dbpost_launch(p, h->ws.get(), h->ws.cap, (hipStream_t)stream));
    });
    API_CATCH(h)
}

int lumina_ocr_rec_crop(lumina_ocr_t* h, const uint8_t* pages_dev, int batch, int height, int width, const int32_t* quads_dev,
                        const int32_t* page_idx_dev, int n_crops, uint8_t* crops_dev, int32_t* widths_dev, void* stream) {
    if (!h || !pages_dev || !quads_dev || !page_idx_dev || !crops_dev || !widths_dev) return locr_fail(h, "rec_crop", "null argument");
    BIND(h);
    (void)batch;
    return hip_rc(h, "rec_crop", rec_crop_launch(pages_dev, height, width, quads_dev, page_idx_dev, n_crops, crops_dev, widths_dev, (hipStream_t)stream));
}

int lumina_ocr_load_cls_weights(lumina_ocr_t* h, const void* blob, size_t nbytes) {
    if (!h || !blob) return locr_fail(h, "load_cls_weights", "null argument");
    BIND(h);
    API_TRY return eng_load_cls(h, blob, nbytes); API_CATCH(h)
}

int lumina_ocr_cls_forward(lumina_ocr_t* h, const uint8_t* crops_dev, const int32_t* widths_dev, int n_crops, float thresh, int32_t* label_dev,
                           float* score_dev, int32_t* flip_dev, void* stream) {
    if (!h) return 1;
    if (n_crops <= 0) return 0;
    if (!crops_dev || !label_dev || !score_dev || !flip_dev) return locr_fail(h, "cls_forward", "null argument");
    BIND(h);
    API_TRY return eng_cls_forward(h, crops_dev, widths_dev, n_crops, thresh, label_dev, score_dev, flip_dev, (hipStream_t)stream); API_CATCH(h)
}

int lumina_ocr_rec_crop_oriented(lumina_ocr_t* h, const uint8_t* pages_dev, int batch, int height, int width, const int32_t* quads_dev,
                                 const int32_t* page_idx_dev, int n_crops, const int32_t* flip_dev, uint8_t* crops_dev, int32_t* widths_dev,
                                 void* stream) {
    if (!h) return 1;
    if (n_crops <= 0) return 0;
    if (!pages_dev || !quads_dev || !page_idx_dev || !flip_dev || !crops_dev || !widths_dev) return locr_fail(h, "rec_crop_oriented", "null argument");
    BIND(h);
    (void)batch;
    return hip_rc(h, "rec_crop_oriented", rec_crop_launch(pages_dev, height, width, quads_dev, page_idx_dev, n_crops, crops_dev, widths_dev,
                                                         (hipStream_t)stream, flip_dev));
}

int lumina_ocr_cls_crop(lumina_ocr_t* h, const uint8_t* pages_dev, int batch, int height, int width, const int32_t* quads_dev,
                        const int32_t* page_idx_dev, int n_crops, uint8_t* crops_dev, int32_t* widths_dev, void* stream) {
    if (!h) return 1;
    if (n_crops <= 0) return 0;
    if (!pages_dev || !quads_dev || !page_idx_dev || !crops_dev || !widths_dev) return locr_fail(h, "cls_crop", "null argument");
    BIND(h);
    (void)batch;
    return hip_rc(h, "cls_crop", cls_crop_launch(pages_dev, height, width, quads_dev, page_idx_dev, n_crops, crops_dev, widths_dev, (hipStream_t)stream));
}

int lumina_ocr_rec_forward(lumina_ocr_t* h, const uint8_t* crops_dev, const int32_t* widths_dev, int n_crops, int32_t* idx_dev, float* prob_dev,
                           void* stream) {
    if (!h || !crops_dev || !idx_dev || !prob_dev) return locr_fail(h, "rec_forward", "null argument");
    BIND(h);
    API_TRY return eng_rec_forward(h, crops_dev, widths_dev, n_crops, idx_dev, prob_dev, (hipStream_t)stream); API_CATCH(h)
}

int lumina_ocr_load_svtr_weights(lumina_ocr_t* h, const void* blob, size_t nbytes) {
    if (!h || !blob) return locr_fail(h, "load_svtr_weights", "null argument");
    BIND(h);
    API_TRY return eng_load_svtr(h, blob, nbytes); API_CATCH(h)
}

int lumina_ocr_svtr_forward(lumina_ocr_t* h, const uint8_t* crops_dev, const int32_t* widths_dev, int n_crops, int32_t* idx_dev, float* prob_dev,
                            void* stream) {
    if (!h || !crops_dev || !idx_dev || !prob_dev) return locr_fail(h, "svtr_forward", "null argument");
    BIND(h);
    API_TRY return eng_svtr_forward(h, crops_dev, widths_dev, n_crops, idx_dev, prob_dev, (hipStream_t)stream); API_CATCH(h)
}

int lumina_ocr_ctc_decode(lumina_ocr_t* h, const int32_t* idx_dev, const float* prob_dev, int n, int32_t* text_dev, int32_t* len_dev,
                          float* score_dev, void* stream) {
    if (!h || !idx_dev || !prob_dev || !text_dev || !len_dev || !score_dev) return locr_fail(h, "ctc_decode", "null argument");
    BIND(h);
    if (n <= 0) return 0;
    return hip_rc(h, "ctc_decode", ctc_collapse_launch(idx_dev, prob_dev, text_dev, len_dev, score_dev, n, LUMINA_REC_T, (hipStream_t)stream));
}

int lumina_ocr_ctc_decode_words(lumina_ocr_t* h, const int32_t* idx_dev, const float* prob_dev, int n, const int32_t* quads_dev,
                                const int32_t* widths_dev, const int32_t* flip_dev, int space_id, int32_t* text_dev, int32_t* len_dev,
                                float* score_dev, int32_t* word_quads_dev, int32_t* word_span_dev, float* word_score_dev, int32_t* word_count_dev,
                                void* stream) {
    if (!h) return 1;
    if (n <= 0) return 0;
    if (!idx_dev || !prob_dev || !quads_dev || !widths_dev || !text_dev || !len_dev || !score_dev || !word_quads_dev || !word_span_dev ||
        !word_score_dev || !word_count_dev)
        return locr_fail(h, "ctc_decode_words", "null argument");
    BIND(h);
    return hip_rc(h, "ctc_decode_words", ctc_words_launch(idx_dev, prob_dev, quads_dev, widths_dev, flip_dev, space_id, text_dev, len_dev, score_dev,
                                                          word_quads_dev, word_span_dev, word_score_dev, word_count_dev, n, LUMINA_REC_T,
                                                          (hipStream_t)stream));
}

int lumina_ocr_conv2d(lumina_ocr_t* h, const uint16_t* x_dev, int n, int height, int width, int cin, const uint16_t* w_host,
                      const float* bias_host, int cout, int ks, int stride, int act, const uint16_t* res_dev, uint16_t* y_dev, void* stream) {
    if (!h || !x_dev || !w_host || !bias_host || !y_dev) return locr_fail(h, "conv2d", "null argument");
    if (cout % 8 != 0) return locr_fail(h, "conv2d", "cout must be a multiple of 8");
    BIND(h);
    API_TRY
    ConvLayer L;
    L.name = "conv2d"; L.ks = ks; L.stride = stride; L.cin = cin; L.cout = cout; L.act = act;
    if (!conv_pick_cfg(ks, stride, cin, cout, &L.cfg)) return locr_fail(h, "conv2d", "unsupported ks/stride/cin");
    std::vector<bf16_t> packed(conv_packed_weight_elems(cout, ks, cin, L.cfg.bn));
    pack_conv_weights(w_host, cout, ks, cin, L.cfg.bn, L.cfg.ck, packed.data(), L.cfg.nw == 6 ? 1 : 0);
    const int ntiles = (cout + L.cfg.bn - 1) / L.cfg.bn;
    std::vector<float> bias((size_t)ntiles * L.cfg.bn, 0.f);
    memcpy(bias.data(), bias_host, sizeof(float) * cout);
    // option conv2d_variant (parity tests): 1 = the LDS-DMA 16x32-tile kernel, 2 = the persistent ring kernel, for the layers
    // those kernels serve in the detector (3x3 / stride 1, >= 32 input channels in chunks of 16, output channels in tiles of 64)
    const bool big_ok = ks == 3 && stride == 1 && cin >= 32 && cin % 16 == 0 && cout % 64 == 0 && L.cfg.bn == 64;
    if (h->conv2d_variant > 0 && !big_ok) return locr_fail(h, "conv2d", "conv2d_variant 1/2 needs ks 3, stride 1, cin % 16 == 0, cin >= 32, cout % 64 == 0");
    // the layer's weights live for this call only
    DeviceMem dw, db, dw2;
    auto upload = [](DeviceMem* d, const void* host, size_t bytes) {
        hipError_t e = mem_alloc(d, bytes);
        return e == hipSuccess ? hipMemcpy(d->get(), host, bytes, hipMemcpyHostToDevice) : e;
    };
    if (upload(&dw, packed.data(), packed.size() * 2) != hipSuccess || upload(&db, bias.data(), bias.size() * 4) != hipSuccess) return locr_fail(h, "conv2d", "weight upload");
    L.wpk = static_cast<bf16_t*>(dw.get()); L.bias = static_cast<float*>(db.get());
    if (h->conv2d_variant > 0) {
        L.cfg_big = L.cfg; L.cfg_big.nw = 6; L.cfg_big.ck = 16;
        std::vector<bf16_t> packed2(conv_packed_weight_elems(cout, ks, cin, 64));
        pack_conv_weights(w_host, cout, ks, cin, 64, 16, packed2.data(), 1);
        if (upload(&dw2, packed2.data(), packed2.size() * 2) != hipSuccess) return locr_fail(h, "conv2d", "weight upload");
        L.wpk_big = static_cast<bf16_t*>(dw2.get());
    }
    Tensor4 x; x.p = const_cast<bf16_t*>(x_dev); x.n = n; x.h = height; x.w = width; x.c = cin;
    Tensor4 y; y.p = y_dev; y.n = n; y.c = cout;
    y.h = (ks == 3) ? (height - 1) / stride + 1 : height / stride;
    y.w = (ks == 3) ? (width - 1) / stride + 1 : width / stride;
    Tensor4 r; r.p = const_cast<bf16_t*>(res_dev); r.n = n; r.h = y.h; r.w = y.w; r.c = cout;
    ConvCall call;
    call.res = res_dev ? &r : nullptr; call.variant = h->conv2d_variant;
    int rc = eng_run_conv(h, L, x, &y, (hipStream_t)stream, call);
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (rc) return rc;
    return hip_rc(h, "conv2d sync", e);
    API_CATCH(h)
}

int lumina_ocr_read_tap(lumina_ocr_t* h, const char* name, uint16_t* out_host, size_t capacity_elems, int dims[4]) {
    if (!h || !name || !dims) return 1;
    auto it = h->taps.find(name);
    if (it == h->taps.end()) return locr_fail(h, "read_tap: unknown tap", name);
    BIND(h);
    const Tensor4& t = it->second;
    dims[0] = t.n; dims[1] = t.h; dims[2] = t.w; dims[3] = t.c;
    if (!out_host) return 0;
    if (capacity_elems < t.elems()) return locr_fail(h, "read_tap", "buffer too small");
    if (hipDeviceSynchronize() != hipSuccess) return locr_fail(h, "read_tap", "sync failed");
    return hip_rc(h, "read_tap", hipMemcpy(out_host, t.p, t.elems() * sizeof(bf16_t), hipMemcpyDeviceToHost));
}

int lumina_ocr_conv_timing(lumina_ocr_t* h, double* total_ms, double* total_flops, int* launches) {
    if (!h || !total_ms || !total_flops || !launches) return 1;
    BIND(h);
    double ms = 0, fl = 0;
    int count = 0;
    if (drain_launches(h, "conv_timing", [&](const LaunchRecord& r, float t) { ms += t; fl += r.flop; ++count; })) return 1;
    *total_ms = ms; *total_flops = fl; *launches = count;
    return 0;
}

static int get_coeffs(lumina_ocr* h, int in_size, int out_size, lumina_ocr::Coeffs* out) {
    auto key = std::make_pair(in_size, out_size);
    auto it = h->coeff_cache.find(key);
    if (it == h->coeff_cache.end()) {
        std::vector<int> bounds, kk;
        lumina_ocr::Coeffs c;
        lanczos_coeffs(in_size, out_size, &c.ksize, &bounds, &kk);
        c.bounds_host = std::make_shared<std::vector<int>>(bounds);
        c.bounds = static_cast<int*>(eng_upload(h, bounds.data(), bounds.size() * 4));
        c.kk = static_cast<int*>(eng_upload(h, kk.data(), kk.size() * 4));
        if (!c.bounds || !c.kk) return locr_fail(h, "resize", "coefficient table upload");
        it = h->coeff_cache.emplace(key, c).first;
    }
    *out = it->second;
    return 0;
}

/* image_preprocessing.py:81-110 on the device: two-pass 8-bit LANCZOS, byte-exact with PIL. */
int lumina_ocr_resize_lanczos(lumina_ocr_t* h, const uint8_t* in_dev, int n, int height, int width, int channels, uint8_t* out_dev,
                              int out_h, int out_w, void* stream) {
    if (!h || !in_dev || !out_dev || n <= 0 || height <= 0 || width <= 0 || out_h <= 0 || out_w <= 0 || channels <= 0)
        return locr_fail(h, "resize_lanczos", "bad arguments");
    BIND(h);
    API_TRY
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* src = in_dev;
    int cur_w = width;
    const bool need_h = out_w != width, need_v = out_h != height;
    if (!need_h && !need_v) {
        return hip_rc(h, "resize_lanczos", hipMemcpyAsync(out_dev, in_dev, (size_t)n * height * width * channels, hipMemcpyDeviceToDevice, st));
    }
    if (need_h) {
        lumina_ocr::Coeffs c;
        if (get_coeffs(h, width, out_w, &c)) return 1;
        uint8_t* dst = out_dev;
        if (need_v) {
            if (hip_rc(h, "resize_lanczos", h->aux.reserve((size_t)n * height * out_w * channels))) return 1;
            dst = h->aux.get();
        }
        if (hip_rc(h, "resize_lanczos", resample_launch(src, dst, c.bounds, c.kk, c.ksize, n, height, width, channels, out_w, 0, c.bounds_host->data(), st))) return 1;
        src = dst; cur_w = out_w;
    }
    if (need_v) {
        lumina_ocr::Coeffs c;
        if (get_coeffs(h, height, out_h, &c)) return 1;
        if (hip_rc(h, "resize_lanczos", resample_launch(src, out_dev, c.bounds, c.kk, c.ksize, n, height, cur_w, channels, out_h, 1, c.bounds_host->data(), st))) return 1;
    }
    return 0;
    API_CATCH(h)
}

/* image_preprocessing.py:132-158 (ImageEnhance.Contrast then .Sharpness) on RGB u8 [n,H,W,3]; tmp_dev: scratch, same size. */
int lumina_ocr_enhance(lumina_ocr_t* h, const uint8_t* img_dev, int n, int height, int width, float contrast, float sharpness,
                       uint8_t* tmp_dev, uint8_t* out_dev, void* stream) {
    if (!h || !img_dev || !tmp_dev || !out_dev || n <= 0) return locr_fail(h, "enhance", "bad arguments");
    BIND(h);
    if (hip_rc(h, "enhance", h->sums.reserve(sizeof(unsigned long long) * (size_t)n))) return 1;
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(h->sums.get());
    return hip_rc(h, "enhance", enhance_launch(img_dev, tmp_dev, out_dev, sums, n, height, width, contrast, sharpness, (hipStream_t)stream));
}

int lumina_ocr_binarize(lumina_ocr_t* h, const uint8_t* img_dev, int n, int height, int width, int adaptive, int threshold, uint8_t* out_dev, void* stream) {
    if (!h || !img_dev || !out_dev || n <= 0 || height <= 0 || width <= 0) return locr_fail(h, "binarize", "bad arguments");
    BIND(h);
    return hip_rc(h, "binarize", binarize_launch(img_dev, out_dev, n, height, width, adaptive != 0, threshold, (hipStream_t)stream));
}

int lumina_ocr_exif_transpose(lumina_ocr_t* h, const uint8_t* img_dev, int n, int height, int width, int orientation, uint8_t* out_dev, void* stream) {
    if (!h || !img_dev || !out_dev || n <= 0 || height <= 0 || width <= 0 || orientation < 1 || orientation > 8 || img_dev == out_dev)
        return locr_fail(h, "exif_transpose", "bad arguments (orientation 1..8, not in place)");
    BIND(h);
    return hip_rc(h, "exif_transpose", exif_transpose_launch(img_dev, out_dev, n, height, width, orientation, (hipStream_t)stream));
}

int lumina_ocr_grayscale(lumina_ocr_t* h, const uint8_t* img_dev, int n, int height, int width, uint8_t* out_dev, void* stream) {
    if (!h || !img_dev || !out_dev || n <= 0 || height <= 0 || width <= 0) return locr_fail(h, "grayscale", "bad arguments");
    BIND(h);
    return hip_rc(h, "grayscale", grayscale_launch(img_dev, out_dev, n, height, width, (hipStream_t)stream));
}

int lumina_ocr_denoise(lumina_ocr_t* h, const uint8_t* img_dev, int n, int height, int width, uint8_t* out_dev, void* stream) {
    if (!h || !img_dev || !out_dev || n <= 0 || height <= 0 || width <= 0 || img_dev == out_dev) return locr_fail(h, "denoise", "bad arguments (not in place)");
    BIND(h);
    return hip_rc(h, "denoise", median3_launch(img_dev, out_dev, n, height, width, (hipStream_t)stream));
}

int lumina_ocr_jpeg_encode(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int quality, int optimize,
                           uint8_t* out_dev, size_t out_stride, int32_t* sizes_dev, void* stream) {
    if (!h || !pages_dev || !out_dev || !sizes_dev || n <= 0 || height <= 0 || width <= 0) return locr_fail(h, "jpeg_encode", "bad arguments");
    BIND(h);
    API_TRY
    if (eng_ws_reserve(h, jpeg_workspace_bytes(n, height, width))) return 1;
    JpegParams p{};
    p.rgb = pages_dev; p.n = n; p.height = height; p.width = width; p.quality = quality; p.optimize = optimize != 0; p.out = out_dev; p.out_stride = out_stride; p.sizes = sizes_dev;
    return hip_rc(h, "jpeg_encode", jpeg_encode_launch(p, h->ws.get(), h->ws.cap, (hipStream_t)stream));
    API_CATCH(h)
}

int lumina_ocr_jpeg_probe(const uint8_t* file, size_t size, int info[6]) {
    if (!file || !info) return -1;
    JdInfo i{};
    const int rc = jpegdec_probe(file, size, &i);
    info[0] = i.width; info[1] = i.height; info[2] = i.ncomp; info[3] = i.hs; info[4] = i.vs; info[5] = i.restart;
    return rc;
}

int lumina_ocr_jpeg_decode(lumina_ocr_t* h, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev, int* status,
                           void* stream) {
    if (!h || !files || !sizes || !out_dev || !status || n <= 0 || height <= 0 || width <= 0) return locr_fail(h, "jpeg_decode", "bad arguments");
    BIND(h);
    API_TRY
    return jpegdec_run(h, files, sizes, n, height, width, out_dev, status, (hipStream_t)stream);
    API_CATCH(h)
}

int lumina_ocr_jpeg_decode_async(lumina_ocr_t* h, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev,
                                 int* status_pinned, int passes, void* stream) {
    if (!h || !files || !sizes || !out_dev || !status_pinned || n <= 0 || height <= 0 || width <= 0 || passes < 2) return locr_fail(h, "jpeg_decode_async", "bad arguments");
    BIND(h);
    API_TRY
    return jpegdec_run(h, files, sizes, n, height, width, out_dev, status_pinned, (hipStream_t)stream, passes);
    API_CATCH(h)
}

int lumina_ocr_jpeg_last_passes(const lumina_ocr_t* h) { return h ? h->jd_last_passes : 0; }

int lumina_ocr_jpeg_probe_progressive(const uint8_t* file, size_t size, int info[8]) {
    if (!file || !info) return -1;
    JdProgInfo i{};
    const int rc = jpegdec_probe_progressive(file, size, &i);
    info[0] = i.width; info[1] = i.height; info[2] = i.ncomp; info[3] = i.hs; info[4] = i.vs; info[5] = i.restart; info[6] = i.progressive; info[7] = i.nscans;
    return rc;
}

int lumina_ocr_jpeg_decode_progressive(lumina_ocr_t* h, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev,
                                       int* status, void* stream) {
    if (!h || !files || !sizes || !out_dev || !status || n <= 0 || height <= 0 || width <= 0) return locr_fail(h, "jpeg_decode_progressive", "bad arguments");
    BIND(h);
    API_TRY
    return jpegdec_run_progressive(h, files, sizes, n, height, width, out_dev, status, (hipStream_t)stream);
    API_CATCH(h)
}

int lumina_ocr_png_probe(const uint8_t* file, size_t size, int info[8]) {
    if (!file || !info) return -1;
    PdInfo i{};
    const int rc = pngdec_probe(file, size, &i);
    info[0] = i.width; info[1] = i.height; info[2] = i.color_type; info[3] = i.bit_depth; info[4] = i.interlace; info[5] = i.palette_size;
    info[6] = i.orientation; info[7] = 0;
    return rc;
}

int lumina_ocr_png_decode(lumina_ocr_t* h, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev, int* status,
                          void* stream) {
    if (!h || !files || !sizes || !out_dev || !status || n <= 0 || height <= 0 || width <= 0) return locr_fail(h, "png_decode", "bad arguments");
    BIND(h);
    API_TRY
    return pngdec_run(h, files, sizes, n, height, width, out_dev, status, (hipStream_t)stream);
    API_CATCH(h)
}

namespace {
thread_local int webp_last_code = 0;
thread_local const char* webp_last_reason = "";
}  // namespace

int lumina_ocr_webp_probe(const uint8_t* file, size_t size, int info[8]) {
    if (!file || !info) return -1;
    WpInfo i{};
    const int rc = webp_probe(file, size, &i);
    info[0] = i.width; info[1] = i.height; info[2] = i.alpha; info[3] = i.vp8x; info[4] = i.exif; info[5] = i.xmp; info[6] = 0; info[7] = 0;
    webp_last_code = rc; webp_last_reason = i.reason ? i.reason : "";
    return rc;
}

const char* lumina_ocr_webp_reason(int code) {
    if (code != 0 && code == webp_last_code && webp_last_reason[0]) return webp_last_reason;
    switch (code) {
        case 0: return "read";
        case -1: return "corrupt or irregular WebP file";
        case -2: return "valid WebP that is not read";
        case -4: return "another size than the batch";
    }
    return "unknown status";
}

int lumina_ocr_webp_decode(lumina_ocr_t* h, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev, int* status,
                           void* stream) {
    if (!h || !files || !sizes || !out_dev || !status || n <= 0 || height <= 0 || width <= 0) return locr_fail(h, "webp_decode", "bad arguments");
    BIND(h);
    API_TRY
    return webpdec_run(h, files, sizes, n, height, width, out_dev, status, (hipStream_t)stream);
    API_CATCH(h)
}

int lumina_ocr_webp_probe_lossy(const uint8_t* file, size_t size, int info[8]) {
    if (!file || !info) return -1;
    const char* reason = "";
    const int rc = vp8dec_probe(file, size, info, &reason);
    webp_last_code = rc; webp_last_reason = reason;
    return rc;
}

int lumina_ocr_webp_decode_lossy(lumina_ocr_t* h, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev,
                                 int* status, void* stream) {
    if (!h || !files || !sizes || !out_dev || !status || n <= 0 || height <= 0 || width <= 0) return locr_fail(h, "webp_decode_lossy", "bad arguments");
    BIND(h);
    API_TRY
    return vp8dec_run(h, files, sizes, n, height, width, out_dev, status, (hipStream_t)stream);
    API_CATCH(h)
}

namespace {
thread_local int jp2_last_code = 0;
thread_local const char* jp2_last_reason = "";
}  // namespace

namespace {
int jp2_probe_any(const uint8_t* file, size_t size, int info[8], unsigned flags) {
    if (!file || !info) return -1;
    Jp2Probe p{};
    int rc = -1;
    try {
        rc = jp2dec_probe(file, size, &p, flags);
    } catch (const std::exception&) {   // (allocation failure: the file is left to the host decoder)
        p.reason = "out of memory while reading the packet headers";
        rc = -2;
    }
    for (int i = 0; i < 8; ++i) info[i] = p.info[i];
    jp2_last_code = rc; jp2_last_reason = p.reason ? p.reason : "";
    return rc;
}
}  // namespace

int lumina_ocr_jp2_probe(const uint8_t* file, size_t size, int info[8]) { return jp2_probe_any(file, size, info, 0); }
int lumina_ocr_jp2_probe_irreversible(const uint8_t* file, size_t size, int info[8]) {
    return jp2_probe_any(file, size, info, LUMINA_OCR_JP2_F_IRREVERSIBLE);
}
int lumina_ocr_jp2_probe_ex(const uint8_t* file, size_t size, unsigned flags, int info[8]) {
    if (flags & ~(unsigned)(LUMINA_OCR_JP2_F_IRREVERSIBLE | LUMINA_OCR_JP2_F_TILES)) {
        jp2_last_code = -1; jp2_last_reason = "unknown flag bits";
        return -1;
    }
    return jp2_probe_any(file, size, info, flags);
}

const char* lumina_ocr_jp2_reason(int code) {
    if (code != 0 && code == jp2_last_code && jp2_last_reason[0]) return jp2_last_reason;
    switch (code) {
        case 0: return "read";
        case -1: return "corrupt or irregular JPEG 2000 file";
        case -2: return "valid JPEG 2000 outside the device subset";
        case -4: return "another size than the batch";
    }
    return "unknown status";
}

int lumina_ocr_jp2_decode(lumina_ocr_t* h, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev, int* status,
                          void* stream) {
    if (!h || !files || !sizes || !out_dev || !status || n <= 0 || height <= 0 || width <= 0) return locr_fail(h, "jp2_decode", "bad arguments");
    BIND(h);
    API_TRY
    return jp2dec_run(h, files, sizes, n, height, width, out_dev, status, (hipStream_t)stream);
    API_CATCH(h)
}

int lumina_ocr_jp2_decode_irreversible(lumina_ocr_t* h, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev,
                                       int* status, void* stream) {
    if (!h || !files || !sizes || !out_dev || !status || n <= 0 || height <= 0 || width <= 0) return locr_fail(h, "jp2_decode_irreversible", "bad arguments");
    BIND(h);
    API_TRY
    return jp2dec_run(h, files, sizes, n, height, width, out_dev, status, (hipStream_t)stream, LUMINA_OCR_JP2_F_IRREVERSIBLE);
    API_CATCH(h)
}

int lumina_ocr_jp2_decode_ex(lumina_ocr_t* h, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev,
                             int* status, unsigned flags, void* stream) {
    if (!h || !files || !sizes || !out_dev || !status || n <= 0 || height <= 0 || width <= 0 ||
        (flags & ~(unsigned)(LUMINA_OCR_JP2_F_IRREVERSIBLE | LUMINA_OCR_JP2_F_TILES)))
        return locr_fail(h, "jp2_decode_ex", "bad arguments");
    BIND(h);
    API_TRY
    return jp2dec_run(h, files, sizes, n, height, width, out_dev, status, (hipStream_t)stream, flags);
    API_CATCH(h)
}

int lumina_ocr_flate_image_decode(lumina_ocr_t* h, const uint8_t* const* streams, const size_t* sizes, int n, int height, int width,
                                  const int32_t* params, const uint8_t* const* palettes, uint8_t* out_dev, int* status, void* stream) {
    if (!h || !streams || !sizes || !params || !out_dev || !status || n <= 0 || height <= 0 || width <= 0) return locr_fail(h, "flate_image_decode", "bad arguments");
    BIND(h);
    API_TRY
    return flate_image_run(h, streams, sizes, n, height, width, params, palettes, out_dev, status, (hipStream_t)stream);
    API_CATCH(h)
}

int lumina_ocr_strip_image_decode(lumina_ocr_t* h, const uint8_t* const* strips, const size_t* sizes, int m, const int32_t* strip_counts, int n,
                                  int height, int width, int rows_per_strip, const int32_t* params, const uint8_t* const* palettes,
                                  uint8_t* out_dev, int* status, void* stream) {
    if (!h || !strips || !sizes || !strip_counts || !params || !out_dev || !status || m < 0 || n <= 0 || height <= 0 || width <= 0 || rows_per_strip <= 0)
        return locr_fail(h, "strip_image_decode", "bad arguments");
    BIND(h);
    API_TRY
    return strip_image_run(h, strips, sizes, m, strip_counts, n, height, width, rows_per_strip, params, palettes, out_dev, status, (hipStream_t)stream);
    API_CATCH(h)
}

int lumina_ocr_ccitt_decode(lumina_ocr_t* h, const uint8_t* const* streams, const size_t* sizes, int n, int rows, int columns,
                            const int32_t* params, uint8_t* out_dev, int* status, void* stream) {
    if (!h || !streams || !sizes || !params || !out_dev || !status || n <= 0 || rows <= 0 || columns <= 0) return locr_fail(h, "ccitt_decode", "bad arguments");
    BIND(h);
    API_TRY
    return ccitt_run(h, streams, sizes, n, rows, columns, params, out_dev, status, (hipStream_t)stream);
    API_CATCH(h)
}

int lumina_ocr_fax_decode(lumina_ocr_t* h, const uint8_t* const* streams, const size_t* sizes, int n, int rows, int columns,
                          const int32_t* params, uint8_t* out_dev, int* status, void* stream) {
    if (!h || !streams || !sizes || !params || !out_dev || !status || n <= 0 || rows <= 0 || columns <= 0) return locr_fail(h, "fax_decode", "bad arguments");
    BIND(h);
    API_TRY
    return fax_run(h, streams, sizes, n, rows, columns, params, out_dev, status, (hipStream_t)stream);
    API_CATCH(h)
}

namespace {
thread_local int jb2_last_code = 0;
thread_local const char* jb2_last_reason = "";
}  // namespace

int lumina_ocr_jbig2_probe(const uint8_t* stream, size_t size, const uint8_t* globals, size_t globals_size, int info[8]) {
    if (!stream || !info) return -1;
    Jb2Page p;
    int rc = -1;
    try {
        rc = jbig2_probe(stream, size, globals, globals ? globals_size : 0, &p);
    } catch (const std::exception&) {   // (allocation failure: the page is left to the host)
        p.reason = "out of memory while reading the segments";
        rc = -2;
    }
    for (int i = 0; i < 8; ++i) info[i] = p.info[i];
    jb2_last_code = rc; jb2_last_reason = p.reason ? p.reason : "";
    return rc;
}

const char* lumina_ocr_jbig2_reason(int code) {
    if (code != 0 && code == jb2_last_code && jb2_last_reason[0]) return jb2_last_reason;
    switch (code) {
        case 0: return "read";
        case -1: return "corrupt or irregular JBIG2 stream";
        case -2: return "valid JBIG2 outside the device subset";
        case -4: return "another size than the batch";
    }
    return "unknown status";
}

int lumina_ocr_jbig2_decode(lumina_ocr_t* h, const uint8_t* const* streams, const size_t* sizes, const uint8_t* const* globals,
                            const size_t* globals_sizes, int n, int height, int width, const int32_t* params, uint8_t* out_dev, int* status,
                            void* stream) {
    if (h && n == 0) return 0;
    if (!h || !streams || !sizes || !params || !out_dev || !status || n < 0 || height <= 0 || width <= 0 || (globals && !globals_sizes))
        return locr_fail(h, "jbig2_decode", "bad arguments");
    BIND(h);
    API_TRY
    return jbig2_run(h, streams, sizes, globals, globals_sizes, n, height, width, params, out_dev, status, (hipStream_t)stream);
    API_CATCH(h)
}

int lumina_ocr_jpeg_coefficients(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int quality, int16_t* coefs_dev,
                                 void* stream) {
    if (!h || !pages_dev || !coefs_dev || n <= 0 || height <= 0 || width <= 0) return locr_fail(h, "jpeg_coefficients", "bad arguments");
    BIND(h);
    return hip_rc(h, "jpeg_coefficients", jpeg_coefficients_launch(pages_dev, n, height, width, quality, coefs_dev, (hipStream_t)stream));
}

static int deskew_tables(lumina_ocr* h) {
    if (h->dk_trig && h->dk_wtab) return 0;
    float trig[360];
    std::vector<short> wtab(32 * 32 * 16);
    deskew_trig_table(trig);
    deskew_weight_table(wtab.data());
    h->dk_trig = static_cast<float*>(eng_upload(h, trig, sizeof(trig)));
    h->dk_wtab = static_cast<short*>(eng_upload(h, wtab.data(), wtab.size() * 2));
    return h->dk_trig && h->dk_wtab ? 0 : locr_fail(h, "deskew", "table upload");
}

int lumina_ocr_deskew(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, uint8_t* out_dev, double* rot_dev, int32_t* info_dev,
                      uint8_t* edges_dev, int32_t* segs_dev, int32_t* nsegs_dev, void* stream) {
    if (!h || !pages_dev || !rot_dev || !info_dev || n <= 0 || height <= 0 || width <= 0) return locr_fail(h, "deskew", "bad arguments");
    if ((segs_dev == nullptr) != (nsegs_dev == nullptr)) return locr_fail(h, "deskew", "segs_dev and nsegs_dev go together");
    BIND(h);
    API_TRY
    if (deskew_tables(h)) return 1;
    // ~16 bytes per pixel + the accumulators
    return for_page_groups(h, n, h->post_group, [&](int nb) { return deskew_workspace_bytes(nb, height, width); }, [&](int b0, int nb) {
        const size_t px = (size_t)height * width;
        DeskewParams p{};
        p.rgb = pages_dev + (size_t)b0 * px * 3; p.out = out_dev ? out_dev + (size_t)b0 * px * 3 : nullptr;
        p.B = nb; p.H = height; p.W = width; p.trig = h->dk_trig; p.wtab = h->dk_wtab;
        p.rot = rot_dev + (size_t)b0 * 3; p.info = info_dev + (size_t)b0 * 2;
        p.edges_out = edges_dev ? edges_dev + (size_t)b0 * px : nullptr;
        p.segs_out = segs_dev ? segs_dev + (size_t)b0 * DESKEW_MAX_PEAKS * DESKEW_SEG_PER_PEAK * 4 : nullptr;
        p.nsegs_out = nsegs_dev ? nsegs_dev + (size_t)b0 * DESKEW_MAX_PEAKS : nullptr;
        return hip_rc(h, "deskew", deskew_launch(p, h->ws.get(), h->ws.cap, (hipStream_t)stream));
    });
    API_CATCH(h)
}

int lumina_ocr_deskew_warp(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, const double* rot_dev, uint8_t* out_dev, void* stream) {
    if (!h || !pages_dev || !rot_dev || !out_dev || n <= 0 || height <= 0 || width <= 0) return locr_fail(h, "deskew_warp", "bad arguments");
    BIND(h);
    API_TRY
    if (deskew_tables(h)) return 1;
    return hip_rc(h, "deskew_warp", deskew_warp_launch(pages_dev, out_dev, rot_dev, h->dk_wtab, n, height, width, (hipStream_t)stream));
    API_CATCH(h)
}

// what is wrong with a table_rules / selection_marks argument set, or null.  rules_and_marks, which takes both sets, reports the table
// parameters in one text of its own (both_sets)
static const char* tables_bad_args(int height, int width, int gap, int min_len, int max_thick, int max_rules, bool both_sets) {
    const bool dims = table_workspace_bytes(1, height, width, gap, min_len, max_rules) == 0;
    if (both_sets)
        return dims || max_thick < 0 ? "bad dimensions or table parameters (sides 1..65535, gap >= 0, min_len >= 1, max_thick >= 0, max_rules 1..2048)" : nullptr;
    if (dims) return "bad dimensions or parameters (sides 1..65535, gap >= 0, min_len >= 1, max_rules 1..2048)";
    return max_thick < 0 ? "max_thick must be >= 0" : nullptr;
}
static const char* marks_bad_args(int height, int width, int min_side, int max_side, int max_marks) {
    if (min_side < MARK_MIN_SIDE || max_side > MARK_MAX_SIDE || max_side < min_side) return "sides must satisfy 4 <= min_side <= max_side <= 64";
    if (marks_workspace_bytes(1, height, width, max_marks) == 0) return "bad dimensions or parameters (sides 1..65535, max_marks 1..2048)";
    return nullptr;
}

int lumina_ocr_table_rules(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int gap, int min_len, int max_thick,
                           int max_rules, int32_t* hrules_dev, int32_t* vrules_dev, int32_t* counts_dev, uint64_t* hmask_dev, void* stream) {
    if (!h) return 1;
    if (n == 0) return 0;
    if (!pages_dev || !hrules_dev || !vrules_dev || !counts_dev || n < 0) return locr_fail(h, "table_rules", "bad arguments");
    if (const char* why = tables_bad_args(height, width, gap, min_len, max_thick, max_rules, false)) return locr_fail(h, "table_rules", why);
    BIND(h);
    API_TRY
    // the run slots: ~40 bytes per (min_len + gap + 1) pixels, both directions
    const auto ws = [&](int nb) { return table_workspace_bytes(nb, height, width, gap, min_len, max_rules); };
    const size_t nw = ((size_t)width + 63) / 64;
    return for_page_groups(h, n, fit_group(h->post_group, n, ws), ws, [&](int b0, int nb) {
        TableParams p{};
        p.rgb = pages_dev + (size_t)b0 * height * width * 3; p.B = nb; p.H = height; p.W = width;
        p.threshold = threshold; p.gap = gap; p.min_len = min_len; p.max_thick = max_thick; p.max_rules = max_rules;
        p.hrules = hrules_dev + (size_t)b0 * max_rules * 5; p.vrules = vrules_dev + (size_t)b0 * max_rules * 5; p.counts = counts_dev + (size_t)b0 * 2;
        p.hmask_out = hmask_dev ? reinterpret_cast<unsigned long long*>(hmask_dev) + (size_t)b0 * height * nw : nullptr;
        return hip_rc(h, "table_rules", table_rules_launch(p, h->ws.get(), h->ws.cap, (hipStream_t)stream));
    });
    API_CATCH(h)
}

// the round marks' parameters (marks.h: the band is at most 32 pixels, one lane per band row)
static const char* const ROUND_BAD_ARGS = "round parameters must satisfy out_max >= 0, ring_div >= 1, band_div >= 4, 0 <= band_min <= 16";

// selection_marks, and with round_dev / round_counts_dev the round marks (radio buttons) of the same components in a second list.
// Without them the pass, its workspace and its rows are the checkboxes' alone
static int selection_marks_impl(lumina_ocr_t* h, const char* what, const uint8_t* pages_dev, int n, int height, int width, int threshold, int min_side, int max_side,
                               int max_marks, int32_t* marks_dev, int32_t* counts_dev, uint64_t* mask_dev, int out_max, int ring_div, int band_div,
                                     int band_min, int32_t* round_dev, int32_t* round_counts_dev, void* stream) {
    if (!h) return 1;
    if (n == 0) return 0;
    if (!pages_dev || !marks_dev || !counts_dev || (round_dev == nullptr) != (round_counts_dev == nullptr) || n < 0) return locr_fail(h, what, "bad arguments");
    if (const char* why = marks_bad_args(height, width, min_side, max_side, max_marks)) return locr_fail(h, what, why);
    if (round_dev && !round_params_ok(out_max, ring_div, band_div, band_min)) return locr_fail(h, what, ROUND_BAD_ARGS);
    BIND(h);
    API_TRY
    // the run list is sized for its worst case (24 bytes per two pixels)
    const auto ws = [&](int nb) { return marks_workspace_bytes(nb, height, width, max_marks, round_dev != nullptr); };
    const size_t nw = ((size_t)width + 63) / 64;
    return for_page_groups(h, n, fit_group(h->post_group, n, ws), ws, [&](int b0, int nb) {
        MarkParams p{};
        p.rgb = pages_dev + (size_t)b0 * height * width * 3; p.B = nb; p.H = height; p.W = width;
        p.threshold = threshold; p.min_side = min_side; p.max_side = max_side; p.max_marks = max_marks;
        p.marks = marks_dev + (size_t)b0 * max_marks * 8; p.counts = counts_dev + b0;
        if (round_dev) { p.rounds = round_dev + (size_t)b0 * max_marks * 8; p.round_counts = round_counts_dev + b0; }
        p.out_max = out_max; p.ring_div = ring_div; p.band_div = band_div; p.band_min = band_min;
        p.mask_out = mask_dev ? reinterpret_cast<unsigned long long*>(mask_dev) + (size_t)b0 * height * nw : nullptr;
        return hip_rc(h, what, marks_launch(p, h->ws.get(), h->ws.cap, (hipStream_t)stream));
    });
    API_CATCH(h)
}

// rules_and_marks, with or without the round marks: one ink mask for all of them
static int rules_and_marks_impl(lumina_ocr_t* h, const char* what, const uint8_t* pages_dev, int n, int height, int width, int threshold, int gap, int min_len,
                               int max_thick, int max_rules, int32_t* hrules_dev, int32_t* vrules_dev, int32_t* rule_counts_dev, int min_side,
                               int max_side, int max_marks, int32_t* marks_dev, int32_t* mark_counts_dev, int out_max, int ring_div, int band_div,
                                     int band_min, int32_t* round_dev, int32_t* round_counts_dev, void* stream) {
    if (!h) return 1;
    if (n == 0) return 0;
    if (!pages_dev || !hrules_dev || !vrules_dev || !rule_counts_dev || !marks_dev || !mark_counts_dev || (round_dev == nullptr) != (round_counts_dev == nullptr) || n < 0) return locr_fail(h, what, "bad arguments");
    if (const char* why = tables_bad_args(height, width, gap, min_len, max_thick, max_rules, true)) return locr_fail(h, what, why);
    if (const char* why = marks_bad_args(height, width, min_side, max_side, max_marks)) return locr_fail(h, what, why);
    if (round_dev && !round_params_ok(out_max, ring_div, band_div, band_min)) return locr_fail(h, what, ROUND_BAD_ARGS);
    BIND(h);
    API_TRY
    // one group size for both (the marks limit, then the tables limit); the workspace is the group's mask, then room for the larger of
    // the two passes (they run one after the other on the stream)
    const auto wt = [&](int nb) { return table_workspace_bytes(nb, height, width, gap, min_len, max_rules); };
    const auto wm = [&](int nb) { return marks_workspace_bytes(nb, height, width, max_marks, round_dev != nullptr); };
    const size_t nw = ((size_t)width + 63) / 64;
    const auto rest_bytes = [&](int nb) { return wt(nb) > wm(nb) ? wt(nb) : wm(nb); };
    const auto ws = [&](int nb) {
        Arena sizes;
        sizes.take<unsigned long long>((size_t)nb * height * nw);
        sizes.take<uint8_t>(rest_bytes(nb));
        return sizes.off;
    };
    hipStream_t st = (hipStream_t)stream;
    return for_page_groups(h, n, fit_group(fit_group(h->post_group, n, wm), n, wt), ws, [&](int b0, int nb) {
        const size_t bytes = rest_bytes(nb);
        Arena a(h->ws.get(), h->ws.cap);
        unsigned long long* mask = a.take<unsigned long long>((size_t)nb * height * nw);
        uint8_t* rest = a.take<uint8_t>(bytes);
        if (a.overflow) return locr_fail(h, what, "workspace");
        const uint8_t* rgb = pages_dev + (size_t)b0 * height * width * 3;
        if (hip_rc(h, what, ink_mask_launch(rgb, mask, nb, height, width, threshold, st))) return 1;
        TableParams t{};
        t.rgb = rgb; t.B = nb; t.H = height; t.W = width; t.threshold = threshold; t.gap = gap; t.min_len = min_len; t.max_thick = max_thick;
        t.max_rules = max_rules; t.hrules = hrules_dev + (size_t)b0 * max_rules * 5; t.vrules = vrules_dev + (size_t)b0 * max_rules * 5;
        t.counts = rule_counts_dev + (size_t)b0 * 2; t.hmask_in = mask;
        if (hip_rc(h, what, table_rules_launch(t, rest, bytes, st))) return 1;
        MarkParams p{};
        p.rgb = rgb; p.B = nb; p.H = height; p.W = width; p.threshold = threshold; p.min_side = min_side; p.max_side = max_side; p.max_marks = max_marks;
        p.marks = marks_dev + (size_t)b0 * max_marks * 8; p.counts = mark_counts_dev + b0; p.mask_in = mask;
        if (round_dev) { p.rounds = round_dev + (size_t)b0 * max_marks * 8; p.round_counts = round_counts_dev + b0; }
        p.out_max = out_max; p.ring_div = ring_div; p.band_div = band_div; p.band_min = band_min;
        return hip_rc(h, what, marks_launch(p, rest, bytes, st));
    });
    API_CATCH(h)
}

int lumina_ocr_selection_marks(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int min_side, int max_side,
                               int max_marks, int32_t* marks_dev, int32_t* counts_dev, uint64_t* mask_dev, void* stream) {
    return selection_marks_impl(h, "selection_marks", pages_dev, n, height, width, threshold, min_side, max_side, max_marks, marks_dev, counts_dev, mask_dev,
                                0, 0, 0, 0, nullptr, nullptr, stream);
}

int lumina_ocr_selection_marks_round(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int min_side, int max_side,
                                     int max_marks, int32_t* marks_dev, int32_t* counts_dev, uint64_t* mask_dev, int out_max, int ring_div, int band_div,
                                     int band_min, int32_t* round_dev, int32_t* round_counts_dev, void* stream) {
    if (h && n != 0 && (!round_dev || !round_counts_dev)) return locr_fail(h, "selection_marks_round", "bad arguments");
    return selection_marks_impl(h, "selection_marks_round", pages_dev, n, height, width, threshold, min_side, max_side, max_marks, marks_dev, counts_dev,
                                mask_dev, out_max, ring_div, band_div, band_min, round_dev, round_counts_dev, stream);
}

int lumina_ocr_rules_and_marks(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int gap, int min_len,
                               int max_thick, int max_rules, int32_t* hrules_dev, int32_t* vrules_dev, int32_t* rule_counts_dev, int min_side,
                               int max_side, int max_marks, int32_t* marks_dev, int32_t* mark_counts_dev, void* stream) {
    return rules_and_marks_impl(h, "rules_and_marks", pages_dev, n, height, width, threshold, gap, min_len, max_thick, max_rules, hrules_dev, vrules_dev,
                                rule_counts_dev, min_side, max_side, max_marks, marks_dev, mark_counts_dev, 0, 0, 0, 0, nullptr, nullptr, stream);
}

int lumina_ocr_rules_and_marks_round(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int gap, int min_len,
                                     int max_thick, int max_rules, int32_t* hrules_dev, int32_t* vrules_dev, int32_t* rule_counts_dev, int min_side,
                                     int max_side, int max_marks, int32_t* marks_dev, int32_t* mark_counts_dev, int out_max, int ring_div, int band_div,
                                     int band_min, int32_t* round_dev, int32_t* round_counts_dev, void* stream) {
    if (h && n != 0 && (!round_dev || !round_counts_dev)) return locr_fail(h, "rules_and_marks_round", "bad arguments");
    return rules_and_marks_impl(h, "rules_and_marks_round", pages_dev, n, height, width, threshold, gap, min_len, max_thick, max_rules, hrules_dev,
                                vrules_dev, rule_counts_dev, min_side, max_side, max_marks, marks_dev, mark_counts_dev, out_max, ring_div, band_div, band_min,
                                round_dev, round_counts_dev, stream);
}

static int barcodes_impl(lumina_ocr_t* h, const char* what, const uint8_t* pages_dev, int n, int height, int width, int threshold, int quiet, int max_dist,
                         int min_rows, int row_gap, int max_codes, int kinds, int32_t* codes_dev, int32_t* syms_dev, int32_t* counts_dev,
                         const uint64_t* mask_in_dev, uint64_t* mask_out_dev, void* stream) {
    if (!h) return 1;
    if (n == 0) return 0;
    if (!pages_dev || !codes_dev || !syms_dev || !counts_dev || n < 0) return locr_fail(h, what, "bad arguments");
    if (!barcode_kinds_ok(kinds)) return locr_fail(h, what, "kinds must be a non-empty set of the bits 0..5 (1..63)");
    if (!barcode_params_ok(quiet, max_dist, min_rows, row_gap, max_codes))
        return locr_fail(h, what, "parameters must satisfy 0 <= quiet <= 64, 0 <= max_dist <= 256, min_rows >= 1, 1 <= row_gap <= 16, max_codes 1..256");
    if (barcodes_workspace_bytes(1, height, width, max_codes) == 0) return locr_fail(h, what, "bad dimensions (sides 1..65535)");
    BIND(h);
    API_TRY
    // the run list is sized for its worst case (8 bytes per two pixels); four read slots a row and a column
    const auto ws = [&](int nb) { return barcodes_workspace_bytes(nb, height, width, max_codes); };
    const size_t nw = ((size_t)width + 63) / 64;
    return for_page_groups(h, n, fit_group(h->post_group, n, ws), ws, [&](int b0, int nb) {
        BarcodeParams p{};
        p.rgb = pages_dev + (size_t)b0 * height * width * 3; p.B = nb; p.H = height; p.W = width;
        p.threshold = threshold; p.quiet = quiet; p.max_dist = max_dist; p.min_rows = min_rows; p.row_gap = row_gap; p.max_codes = max_codes;
        p.kinds = kinds;
        p.codes = codes_dev + (size_t)b0 * max_codes * 8; p.syms = syms_dev + (size_t)b0 * max_codes * BARCODE_MAX_SYMS; p.counts = counts_dev + b0;
        p.mask_in = mask_in_dev ? reinterpret_cast<const unsigned long long*>(mask_in_dev) + (size_t)b0 * height * nw : nullptr;
        p.mask_out = mask_out_dev ? reinterpret_cast<unsigned long long*>(mask_out_dev) + (size_t)b0 * height * nw : nullptr;
        return hip_rc(h, what, barcodes_launch(p, h->ws.get(), h->ws.cap, (hipStream_t)stream));
    });
    API_CATCH(h)
}

int lumina_ocr_barcodes(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int quiet, int max_dist, int min_rows,
                        int row_gap, int max_codes, int32_t* codes_dev, int32_t* syms_dev, int32_t* counts_dev, const uint64_t* mask_in_dev,
                        uint64_t* mask_out_dev, void* stream) {
    return barcodes_impl(h, "barcodes", pages_dev, n, height, width, threshold, quiet, max_dist, min_rows, row_gap, max_codes, BARCODE_KINDS_DEFAULT, codes_dev,
                         syms_dev, counts_dev, mask_in_dev, mask_out_dev, stream);
}

int lumina_ocr_barcodes_kinds(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int quiet, int max_dist, int min_rows,
                              int row_gap, int max_codes, int32_t* codes_dev, int32_t* syms_dev, int32_t* counts_dev, const uint64_t* mask_in_dev,
                              uint64_t* mask_out_dev, void* stream, int kinds) {
    return barcodes_impl(h, "barcodes_kinds", pages_dev, n, height, width, threshold, quiet, max_dist, min_rows, row_gap, max_codes, kinds, codes_dev, syms_dev,
                         counts_dev, mask_in_dev, mask_out_dev, stream);
}

// the scalar parameters both QR calls take
static QrCommon qr_common(int height, int width, int threshold, int min_module, int max_module, int quiet, int centre_tol, int ring_tol, int timing_max,
                          int max_finders, int max_codes) {
    QrCommon c{};
    c.H = height; c.W = width; c.threshold = threshold; c.min_module = min_module; c.max_module = max_module; c.quiet = quiet; c.centre_tol = centre_tol;
    c.ring_tol = ring_tol; c.timing_max = timing_max; c.max_finders = max_finders; c.max_codes = max_codes;
    return c;
}

int lumina_ocr_qrcodes(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int min_module, int max_module, int quiet,
                       int centre_tol, int ring_tol, int timing_max, int max_finders, int max_codes, int32_t* codes_dev, int32_t* data_dev, int32_t* counts_dev,
                       int32_t* finder_counts_dev, const uint64_t* mask_in_dev, uint64_t* mask_out_dev, void* stream) {
    const QrCommon c = qr_common(height, width, threshold, min_module, max_module, quiet, centre_tol, ring_tol, timing_max, max_finders, max_codes);
    const char* bad = qr_params_ok(c) ? nullptr
                                      : "parameters must satisfy 1 <= min_module <= max_module <= 64, 0 <= quiet <= 4, 0 <= centre_tol, ring_tol <= 64, "
                                        "0 <= timing_max <= 128, max_finders 1..64, max_codes 1..64";
    return matrix_codes(
        h, "qrcodes", bad, pages_dev, n, height, width, max_codes, QR_MAX_DATA, codes_dev, data_dev, counts_dev, finder_counts_dev, mask_in_dev, mask_out_dev,
        [&](int nb) { return qrcodes_workspace_bytes(nb, height, width, max_finders, max_codes); },
        [&](const CodeGroup<int32_t>& g, void* ws, size_t cap) {
            QrParams p{};
            static_cast<QrCommon&>(p) = c;
            g.bind(p); p.data = g.data; p.finder_counts = g.slot_counts;
            return qrcodes_launch(p, ws, cap, (hipStream_t)stream);
        });
}

int lumina_ocr_qrcodes_versions(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int min_module, int max_module,
                                int quiet, int centre_tol, int ring_tol, int timing_max, int max_finders, int max_codes, int max_version, int32_t* codes_dev,
                                uint8_t* data_dev, int32_t* counts_dev, int32_t* finder_counts_dev, const uint64_t* mask_in_dev, uint64_t* mask_out_dev,
                                void* stream) {
    const QrCommon c = qr_common(height, width, threshold, min_module, max_module, quiet, centre_tol, ring_tol, timing_max, max_finders, max_codes);
    const char* bad = qr_params_ok(c) && qr_max_version_ok(max_version)
                          ? nullptr
                          : "parameters must satisfy 1 <= min_module <= max_module <= 64, 0 <= quiet <= 4, 0 <= centre_tol, ring_tol <= 64, "
                            "0 <= timing_max <= 128, max_finders 1..64, max_codes 1..64, max_version 10..40";
    return matrix_codes(
        h, "qrcodes_versions", bad, pages_dev, n, height, width, max_codes, QR_VERSIONS_MAX_DATA, codes_dev, data_dev, counts_dev, finder_counts_dev, mask_in_dev,
        mask_out_dev, [&](int nb) { return qrcodes_versions_workspace_bytes(nb, height, width, max_finders, max_codes); },
        [&](const CodeGroup<uint8_t>& g, void* ws, size_t cap) {
            QrVersionsParams p{};
            static_cast<QrCommon&>(p) = c;
            g.bind(p); p.data = g.data; p.finder_counts = g.slot_counts; p.max_version = max_version;
            return qrcodes_versions_launch(p, ws, cap, (hipStream_t)stream);
        });
}

int lumina_ocr_datamatrix(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int min_module, int max_module, int quiet,
                          int timing_max, int solid_max, int max_candidates, int max_codes, int32_t* codes_dev, int32_t* data_dev, int32_t* counts_dev,
                          int32_t* candidate_counts_dev, const uint64_t* mask_in_dev, uint64_t* mask_out_dev, void* stream) {
    const char* bad = dm_params_ok(min_module, max_module, quiet, timing_max, solid_max, max_candidates, max_codes)
                          ? nullptr
                          : "parameters must satisfy 1 <= min_module <= max_module <= 64, 0 <= quiet <= 4, 0 <= timing_max, solid_max <= 128, "
                            "max_candidates 1..1024, max_codes 1..64";
    return matrix_codes(
        h, "datamatrix", bad, pages_dev, n, height, width, max_codes, DM_MAX_DATA, codes_dev, data_dev, counts_dev, candidate_counts_dev, mask_in_dev, mask_out_dev,
        [&](int nb) { return datamatrix_workspace_bytes(nb, height, width, max_candidates, max_codes); },
        [&](const CodeGroup<int32_t>& g, void* ws, size_t cap) {
            DmParams p{};
            g.bind(p); p.data = g.data; p.candidate_counts = g.slot_counts; p.H = height; p.W = width;
            p.threshold = threshold; p.min_module = min_module; p.max_module = max_module; p.quiet = quiet; p.timing_max = timing_max; p.solid_max = solid_max;
            p.max_candidates = max_candidates; p.max_codes = max_codes;
            return datamatrix_launch(p, ws, cap, (hipStream_t)stream);
        });
}

size_t lumina_ocr_datamatrix_sizes_workspace_bytes(int n, int height, int width, int max_candidates, int max_codes) {
    return n > 0 ? datamatrix_sizes_workspace_bytes(n, height, width, max_candidates, max_codes) : 0;
}

int lumina_ocr_datamatrix_placement(int side, uint16_t* out, int capacity) { return datamatrix_placement(side, out, capacity); }

int lumina_ocr_datamatrix_sizes(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int min_module, int max_module,
                                int quiet, int timing_max, int solid_max, int max_candidates, int max_codes, int max_size, int32_t* codes_dev,
                                uint8_t* data_dev, int32_t* counts_dev, int32_t* candidate_counts_dev, const uint64_t* mask_in_dev, uint64_t* mask_out_dev,
                                void* stream) {
    const char* bad = dm_params_ok(min_module, max_module, quiet, timing_max, solid_max, max_candidates, max_codes) && dm_max_size_ok(max_size)
                          ? nullptr
                          : "parameters must satisfy 1 <= min_module <= max_module <= 64, 0 <= quiet <= 4, 0 <= timing_max, solid_max <= 128, "
                            "max_candidates 1..1024, max_codes 1..64, max_size 52..144";
    return matrix_codes(
        h, "datamatrix_sizes", bad, pages_dev, n, height, width, max_codes, DM_MAX_DATA_ALL, codes_dev, data_dev, counts_dev, candidate_counts_dev, mask_in_dev,
        mask_out_dev, [&](int nb) { return datamatrix_sizes_workspace_bytes(nb, height, width, max_candidates, max_codes); },
        [&](const CodeGroup<uint8_t>& g, void* ws, size_t cap) {
            DmSizesParams p{};
            g.bind(p); p.data_all = g.data; p.candidate_counts = g.slot_counts; p.H = height; p.W = width;
            p.threshold = threshold; p.min_module = min_module; p.max_module = max_module; p.quiet = quiet; p.timing_max = timing_max; p.solid_max = solid_max;
            p.max_candidates = max_candidates; p.max_codes = max_codes; p.max_size = max_size;
            return datamatrix_sizes_launch(p, ws, cap, (hipStream_t)stream);
        });
}

size_t lumina_ocr_aztec_workspace_bytes(int n, int height, int width, int max_finders, int max_codes) {
    return n > 0 ? aztec_workspace_bytes(n, height, width, max_finders, max_codes) : 0;
}

// the scalar parameters both Aztec calls take
static void aztec_common(AztecParams& p, int height, int width, int threshold, int min_module, int max_module, int quiet, int centre_tol, int ring_tol,
                         int mark_max, int max_finders, int max_codes) {
    p.H = height; p.W = width; p.threshold = threshold; p.min_module = min_module; p.max_module = max_module; p.quiet = quiet; p.centre_tol = centre_tol;
    p.ring_tol = ring_tol; p.mark_max = mark_max; p.max_finders = max_finders; p.max_codes = max_codes;
}

int lumina_ocr_aztec(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int min_module, int max_module, int quiet,
                     int centre_tol, int ring_tol, int mark_max, int max_finders, int max_codes, int32_t* codes_dev, int32_t* data_dev, int32_t* counts_dev,
                     int32_t* finder_counts_dev, const uint64_t* mask_in_dev, uint64_t* mask_out_dev, void* stream) {
    const char* bad = aztec_params_ok(min_module, max_module, quiet, centre_tol, ring_tol, mark_max, max_finders, max_codes)
                          ? nullptr
                          : "parameters must satisfy 1 <= min_module <= max_module <= 64, 0 <= quiet <= 4, 0 <= centre_tol <= 64, 0 <= ring_tol <= 15, "
                            "0 <= mark_max <= 64, max_finders 1..64, max_codes 1..64";
    return matrix_codes(
        h, "aztec", bad, pages_dev, n, height, width, max_codes, AZ_MAX_DATA, codes_dev, data_dev, counts_dev, finder_counts_dev, mask_in_dev, mask_out_dev,
        [&](int nb) { return aztec_workspace_bytes(nb, height, width, max_finders, max_codes); },
        [&](const CodeGroup<int32_t>& g, void* ws, size_t cap) {
            AztecParams p{};
            aztec_common(p, height, width, threshold, min_module, max_module, quiet, centre_tol, ring_tol, mark_max, max_finders, max_codes);
            g.bind(p); p.data = g.data; p.finder_counts = g.slot_counts;
            return aztec_launch(p, ws, cap, (hipStream_t)stream);
        });
}

size_t lumina_ocr_aztec_layers_workspace_bytes(int n, int height, int width, int max_finders, int max_codes) {
    return n > 0 ? aztec_layers_workspace_bytes(n, height, width, max_finders, max_codes) : 0;
}

int lumina_ocr_aztec_layers(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int min_module, int max_module, int quiet,
                            int centre_tol, int ring_tol, int mark_max, int max_finders, int max_codes, int max_layers, int32_t* codes_dev, uint16_t* data_dev,
                            int32_t* counts_dev, int32_t* finder_counts_dev, const uint64_t* mask_in_dev, uint64_t* mask_out_dev, void* stream) {
    const char* bad = aztec_params_ok(min_module, max_module, quiet, centre_tol, ring_tol, mark_max, max_finders, max_codes) && aztec_max_layers_ok(max_layers)
                          ? nullptr
                          : "parameters must satisfy 1 <= min_module <= max_module <= 64, 0 <= quiet <= 4, 0 <= centre_tol <= 64, "
                            "0 <= ring_tol <= 15, 0 <= mark_max <= 64, max_finders 1..64, max_codes 1..64, max_layers 11..32";
    return matrix_codes(
        h, "aztec_layers", bad, pages_dev, n, height, width, max_codes, AZ_MAX_DATA_ALL, codes_dev, data_dev, counts_dev, finder_counts_dev, mask_in_dev,
        mask_out_dev, [&](int nb) { return aztec_layers_workspace_bytes(nb, height, width, max_finders, max_codes); },
        [&](const CodeGroup<uint16_t>& g, void* ws, size_t cap) {
            AztecLayersParams p{};
            aztec_common(p, height, width, threshold, min_module, max_module, quiet, centre_tol, ring_tol, mark_max, max_finders, max_codes);
            g.bind(p); p.data_all = g.data; p.finder_counts = g.slot_counts; p.max_layers = max_layers;
            return aztec_layers_launch(p, ws, cap, (hipStream_t)stream);
        });
}

size_t lumina_ocr_page_quarter_workspace_bytes(int n, int height, int width) { return n > 0 ? quarter_workspace_bytes(n, height, width) : 0; }

int lumina_ocr_page_quarter(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int ratio, int64_t* energies_dev,
                            int32_t* sideways_dev, void* stream) {
    if (!h) return 1;
    if (n == 0) return 0;
    if (!pages_dev || !energies_dev || !sideways_dev || n < 0) return locr_fail(h, "page_quarter", "bad arguments");
    if (quarter_workspace_bytes(1, height, width) == 0) return locr_fail(h, "page_quarter", "bad dimensions (sides 1..65535)");
    if (ratio < 1 || ratio > QUARTER_MAX_RATIO) return locr_fail(h, "page_quarter", "ratio must be 1..1024");
    BIND(h);
    API_TRY
    // two masks and the profiles (~1/12 of the page bytes)
    const auto ws = [&](int nb) { return quarter_workspace_bytes(nb, height, width); };
    return for_page_groups(h, n, fit_group(h->post_group, n, ws), ws, [&](int b0, int nb) {
        QuarterParams p{};
        p.rgb = pages_dev + (size_t)b0 * height * width * 3; p.B = nb; p.H = height; p.W = width; p.threshold = threshold; p.ratio = ratio;
        p.energies = reinterpret_cast<long long*>(energies_dev) + (size_t)b0 * 2; p.sideways = sideways_dev + b0;
        return hip_rc(h, "page_quarter", quarter_launch(p, h->ws.get(), h->ws.cap, (hipStream_t)stream));
    });
    API_CATCH(h)
}

int lumina_ocr_page_turn(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, const int32_t* index_dev, int m, int turn,
                         uint8_t* out_dev, void* stream) {
    if (!h) return 1;
    if (m == 0) return 0;
    if (!pages_dev || !index_dev || !out_dev || n <= 0 || m < 0 || height <= 0 || width <= 0 || height > 65535 || width > 65535 || turn < 0 || turn > 3 ||
        pages_dev == out_dev)
        return locr_fail(h, "page_turn", "bad arguments (sides 1..65535, turn 0..3, not in place)");
    BIND(h);
    hipStream_t st = (hipStream_t)stream;
    const size_t page = (size_t)height * width * 3;
    for (int j0 = 0; j0 < m; j0 += 32768) {   // (the page index is a grid dimension)
        const int mj = m - j0 < 32768 ? m - j0 : 32768;
        if (hip_rc(h, "page_turn", page_turn_launch(pages_dev, n, height, width, index_dev + j0, mj, turn, out_dev + (size_t)j0 * page, st))) return 1;
    }
    return 0;
}

int lumina_ocr_page_vote(lumina_ocr_t* h, const int32_t* flip_dev, const int32_t* page_idx_dev, int n, int pages, int32_t* counts_dev, void* stream) {
    if (!h) return 1;
    if (pages == 0) return 0;
    if (!counts_dev || pages < 0 || n < 0 || (n > 0 && (!flip_dev || !page_idx_dev))) return locr_fail(h, "page_vote", "bad arguments");
    BIND(h);
    return hip_rc(h, "page_vote", page_vote_launch(flip_dev, page_idx_dev, n, pages, counts_dev, (hipStream_t)stream));
}

int lumina_ocr_page_compose(lumina_ocr_t* h, const lumina_ocr_compose_layer* layers, int n_layers, int n, int height, int width, uint8_t* out_dev,
                            void* stream) {
    if (!h) return 1;
    if (n == 0) return 0;
    BIND(h);
    API_TRY
    return page_compose_run(h, layers, n_layers, n, height, width, out_dev, (hipStream_t)stream);
    API_CATCH(h)
}

int lumina_ocr_svtr_num_classes(const lumina_ocr_t* h) { return h ? h->svtr.num_classes : 0; }
int lumina_ocr_svtr_dtype(const lumina_ocr_t* h) { return h ? h->svtr.dtype : 0; }

int lumina_ocr_conv_timing_detail(lumina_ocr_t* h, char* buf, size_t cap) {
    if (!h || !buf || cap == 0) return 1;
    BIND(h);
    std::string out;
    if (drain_launches(h, "conv_timing_detail", [&](const LaunchRecord& r, float t) {
            char line[256];
            snprintf(line, sizeof(line), "%s %s %.4f %.4f %.4f\n", r.layer.c_str(), r.kernel.c_str(), t, r.flop * 1e-9, r.bytes * 1e-6);
            out += line;
        }))
        return 1;
    snprintf(buf, cap, "%s", out.c_str());
    return 0;
}

}  // extern "C"
