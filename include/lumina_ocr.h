/* lumina_ocr.h — C ABI of the MI355X-native det+rec OCR engine (liblumina_ocr.so).
 *
 * This is the drop-in boundary underneath the reference's OCR-provider interface.  The reference
 * has no FFI for this path: its provider is a Python module whose engine slot is one call,
 *   Azure : /root/reference/backend/services/ocr_service.py:213-246  (_analyze_with_azure)
 *   Paddle: /root/reference/backend/services/ocr_service_paddleocr_backup.py:285 (pipeline.predict)
 * and whose result is reshaped by ocr_service.py:248-376 (_extract_layout_boxes).  The entry
 * points below are what a ctypes binding inside that slot calls (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; it never throws and never
 *     aborts.  lumina_ocr_last_error() returns a description of the last failure on the handle
 *     (the reference's error convention is "errors are data": ocr_service.py:464-475).
 *   - all *_dev pointers are device pointers owned by the caller (e.g. torch-ROCm tensors,
 *     tensor.data_ptr()); `stream` is a hipStream_t passed as void* (NULL = default stream).
 *     Work is enqueued asynchronously on that stream unless stated otherwise.
 *   - a handle is bound to one device and must not be used from two threads at once (the
 *     reference serialises pages with a Semaphore(1): ocr_service.py:157, :404).  Every entry
 *     runs with the handle's device current and puts the calling thread's previous device back
 *     before it returns.
 *   - images are uint8 HWC RGB; activations are bf16 NHWC; the probability map is bf16.
 */
#ifndef LUMINA_OCR_H
#define LUMINA_OCR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lumina_ocr lumina_ocr_t;

#define LUMINA_REC_H 32
#define LUMINA_REC_W 320
#define LUMINA_REC_T 80
#define LUMINA_MAX_WORDS 40 /* words of one line: 80 steps hold at most 40 characters with a space between each two */
#define LUMINA_MAX_BOXES 1000 /* DB max_candidates; box buffers are [B][LUMINA_MAX_BOXES][8] */

/* lifecycle — replaces OCRService._ensure_client_initialized (ocr_service.py:166-207) */
int lumina_ocr_create(int device, lumina_ocr_t** out);
void lumina_ocr_destroy(lumina_ocr_t* h);
const char* lumina_ocr_last_error(const lumina_ocr_t* h);
const char* lumina_ocr_version(void);
/* options: "det_sub_batch", "rec_sub_batch", "cls_sub_batch", "post_group", "tail_group", "keep_taps", "time_convs"; developer A/B switches (results are
 * bit-identical either way): "fuse_head", "fuse_pool", "fuse_stem", "fuse_mb", "fpn_multi", "conv_ring", "ring_orient", "conv_big_min",
 * "blocked_layout" (experiment: fails loudly when a blocked tensor would reach a kernel other than the ring kernel);
 * "svtr_f16" (storage type of the next SVTR load), "conv2d_variant" (kernel choice of lumina_ocr_conv2d, parity tests);
 * "png_sub_batch_mb" (lumina_ocr_png_decode: MB of inflated scanlines per sub-batch, default 768 — bounds the workspace a PNG batch reserves);
 * "webp_sub_batch_mb" (lumina_ocr_webp_decode: MB of pixel planes and code tables per sub-batch, default 2048 — bounds the workspace a WebP batch
 * reserves);
 * "jp2_sub_batch_mb" (lumina_ocr_jp2_decode: MB of coefficient planes per sub-batch, default 4096) */
int lumina_ocr_set_option(lumina_ocr_t* h, const char* key, int value);

/* weights: "LOCW" container (ocr-system_amd/lumina_ocr/arch.py write_blob), host memory.
 * Replaces PaddleOCRVL(...) model construction (ocr_service_paddleocr_backup.py:204-253).
 *
 * Every lumina_ocr_load_*_weights first parses the whole container and checks every tensor the model reads (csrc/blob_check.h: name,
 * dtype, rank, every dimension, byte count = dims x element size) and only then touches the engine.  A REFUSED BLOB LEAVES THE
 * PREVIOUSLY LOADED MODEL OF THAT KIND INTACT AND RUNNABLE, BIT FOR BIT; on an engine that had none, the model stays "not loaded".
 * The call returns 1 and lumina_ocr_last_error() gives "load_<kind>_weights: <reason> (tensor <name>)".  Reasons:
 *   container : bad magic | unsupported version | truncated | truncated data | unknown dtype | rank out of range (1 .. 4) |
 *               implausible dimension (0, above 2^28, or a product above 2^34) | byte count does not match the dimensions |
 *               duplicate tensor name | trailing bytes
 *   model     : missing tensor | wrong dtype | wrong rank | wrong dimension | class count out of range (the CTC heads take 2 .. 65536
 *               classes; weight and bias must agree) | svtr.config value not a small whole number | svtr.config out of range (...)
 * Where several tensors are wrong, the one whose name sorts first is named.  Layout of every conv / linear weight: OHWI
 * [out][kh][kw][in] bf16 (depthwise [c][k][k][1], squeeze-excite [mid][1][1][c]); biases and LayerNorm vectors f32.
 * Choices: tensors the model does not read are ignored (a duplicate name is refused even then); bytes after the last tensor are
 * refused; the blob may lie at any address (one that is no multiple of 16 is copied to aligned storage for the duration of the call)
 * and is not referenced after the call returns.  If a device allocation or upload fails after the check has passed, the model of that
 * kind is not loaded on return and its forward refuses with "not loaded". */
int lumina_ocr_load_det_weights(lumina_ocr_t* h, const void* blob, size_t nbytes);
int lumina_ocr_load_rec_weights(lumina_ocr_t* h, const void* blob, size_t nbytes);
int lumina_ocr_num_classes(const lumina_ocr_t* h);
int lumina_ocr_model_loaded(const lumina_ocr_t* h, int kind);   /* 1 if the model is loaded: kind 0 det, 1 rec (CRNN), 2 cls, 3 SVTR */

/* image -> tensor: xn = bf16(u8 * scale[c] + shift[c]), zero outside (valid_h, valid_w).
 * layout_nchw = 1 writes [N,3,Hp,Wp], 0 writes [N,Hp,Wp,3]. */
int lumina_ocr_normalize(lumina_ocr_t* h, const uint8_t* img_dev, int n, int height, int width, int hp, int wp,
                         const float scale[3], const float shift[3], int layout_nchw, uint16_t* out_dev, void* stream);

/* DBNet (ResNet18_vd + DBFPN + DBHead): pages_dev uint8 [B,H,W,3] -> prob_dev bf16 [B,Hp,Wp],
 * Hp, Wp multiples of 32, >= H, W (the page is zero-padded in normalised space).
 * This is the arithmetic of the engine slot (ocr_service.py:231-238). */
int lumina_ocr_det_forward(lumina_ocr_t* h, const uint8_t* pages_dev, int batch, int height, int width, int hp, int wp,
                           uint16_t* prob_dev, void* stream);

/* DB post-process on device: prob -> integer quads (TL,TR,BR,BL) in page pixels.
 * boxes_dev int32 [B][max_boxes][8], scores_dev float [B][max_boxes], counts_dev int32 [B].
 * Output shape follows ocr_postprocessor.py:24 / ocr_service.py:295-301 (4 points / flat 8). */
int lumina_ocr_det_postprocess(lumina_ocr_t* h, const uint16_t* prob_dev, int batch, int hp, int wp, int valid_h, int valid_w,
                               float thresh, float box_thresh, float unclip_ratio, int min_size, int max_boxes,
                               int32_t* boxes_dev, float* scores_dev, int32_t* counts_dev, void* stream);

/* Recognition crops: for crop i, sample quad quads_dev[i] (8 int32) of page page_idx_dev[i] into
 * crops_dev uint8 [n][32][320][3]; widths_dev int32 [n] receives the valid width. */
int lumina_ocr_rec_crop(lumina_ocr_t* h, const uint8_t* pages_dev, int batch, int height, int width, const int32_t* quads_dev,
                        const int32_t* page_idx_dev, int n_crops, uint8_t* crops_dev, int32_t* widths_dev, void* stream);

/* lumina_ocr_rec_crop with a per-crop flag flip_dev int32 [n] (lumina_ocr_cls_forward's: the lines PaddleOCR's use_angle_cls reads as
 * upside down): a flagged crop is the 180-degree turn of the crop lumina_ocr_rec_crop makes, within its valid width —
 * out[i][j] = crop[31-i][wc-1-j] for j < wc; padding and widths are unchanged, an unflagged crop is byte-identical.
 * n_crops == 0 is a no-op (no pointer is read). */
int lumina_ocr_rec_crop_oriented(lumina_ocr_t* h, const uint8_t* pages_dev, int batch, int height, int width, const int32_t* quads_dev,
                                 const int32_t* page_idx_dev, int n_crops, const int32_t* flip_dev, uint8_t* crops_dev, int32_t* widths_dev,
                                 void* stream);

/* Text-line orientation classifier (PP-OCR `cls`, ch_ppocr_mobile_v2.0_cls; PaddleOCR's use_angle_cls): MobileNetV3-small x0.35 on
 * 48 x 192 crops -> conv 1x1 (200) -> 2x2 max pool -> mean -> FC(2) -> soft-max.  Blob: LOCW with the cls.* tensors of
 * lumina_ocr/arch.py make_cls_weights; checked before anything is touched, as lumina_ocr_load_det_weights states for every model:
 * a refused blob leaves the previously loaded classifier intact and runnable, bit for bit. */
int lumina_ocr_load_cls_weights(lumina_ocr_t* h, const void* blob, size_t nbytes);

/* Orientation-classifier crops (PP-OCR `cls` input): the sampling of lumina_ocr_rec_crop, 48 rows, into crops_dev
 * uint8 [n][48][192][3]; widths_dev int32 [n] receives the valid width min(192, ceil(48 * ratio)), columns past it are 0.
 * n_crops == 0 is a no-op. */
int lumina_ocr_cls_crop(lumina_ocr_t* h, const uint8_t* pages_dev, int batch, int height, int width, const int32_t* quads_dev,
                        const int32_t* page_idx_dev, int n_crops, uint8_t* crops_dev, int32_t* widths_dev, void* stream);

/* Orientation classifier: crops uint8 [n][48][192][3] (+ optional valid widths, as lumina_ocr_cls_crop writes them) ->
 * label_dev int32 [n] (0 = "0", 1 = "180"), score_dev float [n] (soft-max probability of the label), flip_dev int32 [n] =
 * label == 1 && score > thresh (PaddleOCR's cls_thresh, 0.9), the flags lumina_ocr_rec_crop_oriented takes.  Runs in sub-batches of
 * option "cls_sub_batch" crops (default 4096); no host synchronisation.  n_crops == 0 is a no-op. */
int lumina_ocr_cls_forward(lumina_ocr_t* h, const uint8_t* crops_dev, const int32_t* widths_dev, int n_crops, float thresh, int32_t* label_dev,
                           float* score_dev, int32_t* flip_dev, void* stream);

/* CRNN (MobileNetV3-small x0.5 + 2xBiLSTM(96) + FC) with the CTC FC, arg-max and soft-max fused:
 * crops uint8 [n][32][320][3] (+ optional valid widths) -> idx int32 [n][80], prob float [n][80]. */
int lumina_ocr_rec_forward(lumina_ocr_t* h, const uint8_t* crops_dev, const int32_t* widths_dev, int n_crops, int32_t* idx_dev,
                           float* prob_dev, void* stream);

/* CTC greedy decode: collapse repeats, drop blank(0). text int32 [n][80] (class ids, -1 padded),
 * len int32 [n], score float [n] (mean max-prob of kept steps) — the (text, confidence) pair of
 * ocr_postprocessor.py:73-93 and the "confidence" key of ocr_service.py:298. */
int lumina_ocr_ctc_decode(lumina_ocr_t* h, const int32_t* idx_dev, const float* prob_dev, int n, int32_t* text_dev, int32_t* len_dev,
                          float* score_dev, void* stream);

/* lumina_ocr_ctc_decode + the words of every line, from the same pass over the CTC alignment (PaddleOCR's return_word_box; Azure's
 * `word` entries with their own polygon and confidence, ocr_service.py:293-311).  text / len / score are bit-identical to
 * lumina_ocr_ctc_decode.  Step t of the recogniser covers columns [4t, 4t + 4) of the line's crop.
 *   kept character: a step t with idx[t] != 0 && idx[t] != idx[t-1]; its run ends at the last consecutive step with the same class.
 *   word: a maximal run of kept characters whose class is not space_id — the non-empty pieces of text.split(" "), in text order;
 *     space_id < 0: the whole line is one word (none when it is empty).  At most LUMINA_MAX_WORDS per line.
 *   columns: c0 = min(4 * t_first, wc), c1 = max(min(4 * (run end of the last character + 1), wc), c0), wc = widths_dev[i], the crop's
 *     valid width (lumina_ocr_rec_crop).  flip_dev (optional, the flags lumina_ocr_rec_crop_oriented took): a set flag means the crop
 *     was turned, so the word covers the source columns [wc - c1, wc - c0).  A line with wc <= 0 has no words.
 *   quad: the corners P0..P3 of quads_dev[i] in the order the crop used them (lumina_ocr_rec_crop rotates the corners by one when
 *     4 * height^2 >= 9 * width^2 of the quad's longer sides: a vertical line); a column c maps to P0 + R((P1 - P0) * c / wc) on the
 *     top edge and P3 + R((P2 - P3) * c / wc) on the bottom edge, per coordinate, in 64-bit integers, R = round half away from zero.
 *     The four points are written in the line quad's own corner order: point k lies on the side of corner k of the line (TL, TR,
 *     BR, BL for an unrotated line).
 *   score: the fp32 sum, in time order, of the kept probabilities of the word's characters, divided by their count (the rule of
 *     `score`).
 * word_quads_dev int32 [n][LUMINA_MAX_WORDS][8]; word_span_dev int32 [n][LUMINA_MAX_WORDS][2] = index of the word's first character
 * in text, character count; word_score_dev float [n][LUMINA_MAX_WORDS]; word_count_dev int32 [n]; rows past the count are left
 * untouched.  No workspace.  Defined bit for bit (tests/word_reference.py).  Asynchronous; n == 0 is a no-op. */
int lumina_ocr_ctc_decode_words(lumina_ocr_t* h, const int32_t* idx_dev, const float* prob_dev, int n, const int32_t* quads_dev,
                                const int32_t* widths_dev, const int32_t* flip_dev /* may be NULL */, int space_id, int32_t* text_dev,
                                int32_t* len_dev, float* score_dev, int32_t* word_quads_dev, int32_t* word_span_dev, float* word_score_dev,
                                int32_t* word_count_dev, void* stream);

/* Reference pre-processing on the device, byte-exact with the reference's PIL path:
 * resize_if_needed (image_preprocessing.py:81-110): 8-bit two-pass LANCZOS to (out_h, out_w); any channel count. */
int lumina_ocr_resize_lanczos(lumina_ocr_t* h, const uint8_t* in_dev, int n, int height, int width, int channels, uint8_t* out_dev,
                              int out_h, int out_w, void* stream);
/* enhance_contrast(contrast) then enhance_sharpness(sharpness) (image_preprocessing.py:132-158, :234-240) on RGB
 * uint8 [n,H,W,3]; tmp_dev is a scratch buffer of the same size. */
int lumina_ocr_enhance(lumina_ocr_t* h, const uint8_t* img_dev, int n, int height, int width, float contrast, float sharpness,
                       uint8_t* tmp_dev, uint8_t* out_dev, void* stream);

/* binarize (image_preprocessing.py:175-185) / adaptive_binarize (:462-494; settings.PREPROCESSING_APPLY_BINARIZE, off by default,
 * replaces contrast + sharpness when on: :613-622).  adaptive = 0: PIL L > threshold (what the reference's adaptive_binarize degrades
 * to without OpenCV, :473-475; byte-exact with it); adaptive = 1: cv2.adaptiveThreshold(GAUSSIAN_C, BINARY, blockSize 11, C 2)
 * restated ("parity unpinned").  RGB uint8 [n,H,W,3] in; the 0 / 255 value on all three channels out. */
int lumina_ocr_binarize(lumina_ocr_t* h, const uint8_t* img_dev, int n, int height, int width, int adaptive, int threshold, uint8_t* out_dev,
                        void* stream);

/* optimize_for_ocr's optional steps (image_preprocessing.py:225-231; both off by default in the reference's callers):
 * convert_to_grayscale (:167-169) = PIL convert('L'), written to all three channels of the page; denoise (:160-165) = PIL
 * MedianFilter(3), per channel, image edge-replicated.  uint8 [n,H,W,3] in and out (denoise: not in place); byte-exact with Pillow. */
/* auto_orient (image_preprocessing.py:171-173, first step of optimize_for_ocr :213) = PIL ImageOps.exif_transpose: EXIF orientation 1..8
 * applied on the device (the companion of lumina_ocr_jpeg_decode for camera / phone files); out_dev is [n][width][height][3] for 5..8. */
int lumina_ocr_exif_transpose(lumina_ocr_t* h, const uint8_t* img_dev, int n, int height, int width, int orientation, uint8_t* out_dev, void* stream);
int lumina_ocr_grayscale(lumina_ocr_t* h, const uint8_t* img_dev, int n, int height, int width, uint8_t* out_dev, void* stream);
int lumina_ocr_denoise(lumina_ocr_t* h, const uint8_t* img_dev, int n, int height, int width, uint8_t* out_dev, void* stream);

/* deskew (image_preprocessing.py:372-460; on by default in the provider: backend/config.py:85, ocr_service.py:412-417): Canny(50, 150)
 * -> Hough line segments (threshold 100, min length 100, max gap 10) -> median of the segment angles folded into [-45, 45] ->
 * unchanged below 0.5 / above 45 degrees -> cubic affine warp about (W / 2, H / 2) with replicated borders.  The reference does
 * this with OpenCV (absent offline: "parity unpinned"); the arithmetic is defined by oracle/csrc/deskew_oracle.c and reproduced
 * bit for bit.  pages_dev uint8 [n,H,W,3]; out_dev (same shape, may be NULL: estimate only) receives the rotated page or a copy;
 * rot_dev double [n][3] = sin, cos of the angle and a flag (0 no line found, 1 below 0.5 degrees, 2 above 45 degrees, 3 rotated);
 * info_dev int32 [n][2] = segments found, Hough peaks walked.  Optional parity hooks (NULL to skip): edges_dev uint8 [n,H,W]
 * (0 / 255), segs_dev int32 [n][512][8][4] (x1, y1, x2, y2) with nsegs_dev int32 [n][512] segments per peak slot.  Asynchronous. */
int lumina_ocr_deskew(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, uint8_t* out_dev, double* rot_dev,
                      int32_t* info_dev, uint8_t* edges_dev, int32_t* segs_dev, int32_t* nsegs_dev, void* stream);
/* The warp alone, for given (sin, cos, flag) triples: cv2.getRotationMatrix2D((w // 2, h // 2), angle, 1.0) + cv2.warpAffine(...,
 * flags=INTER_CUBIC, borderMode=BORDER_REPLICATE) (image_preprocessing.py:446-454) in OpenCV's fixed-point arithmetic. */
int lumina_ocr_deskew_warp(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, const double* rot_dev, uint8_t* out_dev,
                           void* stream);

/* Rules of ruled ("lattice") tables: the long thin ink lines of each page, the device half of the `table` / `table_cell` entries of
 * the reference's result (ocr_service.py:324-352; the host half is lumina_ocr/utils/tables.py).  ink = L < threshold with L = PIL
 * convert('L'); in every row the ink runs at most `gap` non-ink pixels apart merge and those at least min_len long are kept; kept
 * runs of adjacent rows whose x-intervals overlap form components; a component with bounding box x0, y0, x1, y1 and area (the sum
 * of its run lengths) is a horizontal rule when x1 - x0 + 1 >= min_len and area <= max_thick * (x1 - x0 + 1).  Vertical rules:
 * the same with x and y exchanged.  pages_dev uint8 [n,H,W,3]; hrules_dev / vrules_dev int32 [n][max_rules][5] = x0, y0, x1, y1,
 * area, sorted by (y0, x0, y1, x1) / (x0, y0, x1, y1), rows past the count untouched; counts_dev int32 [n][2] = the true numbers of
 * horizontal and vertical rules (a list whose count exceeds max_rules is not written).  hmask_dev: optional parity hook (NULL to
 * skip), the ink mask uint64 [n][H][ceil(W / 64)], bit x % 64 of word x / 64, bits past W zero.  max_rules <= 2048.  Integer
 * arithmetic throughout: the result is defined bit for bit (tests/table_reference.py).  Asynchronous; n == 0 is a no-op. */
int lumina_ocr_table_rules(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int gap, int min_len,
                           int max_thick, int max_rules, int32_t* hrules_dev, int32_t* vrules_dev, int32_t* counts_dev, uint64_t* hmask_dev,
                           void* stream);

/* Selection marks (checkboxes): the device half of the `selection_mark` entries of the reference's result (ocr_service.py:313-322;
 * the host half is lumina_ocr/utils/marks.py).  ink as in lumina_ocr_table_rules.  The 8-connected components of the ink with a
 * bounding box x0, y0, x1, y1 (inclusive; w, h its sides) are candidates when min_side <= w, h <= max_side and
 * 4 |w - h| <= min(w, h).  Frame test on the page's ink inside the box, t = 1 + min(w, h) / 8: top / bottom = the columns of the box
 * with ink in its first / last t rows, left / right = the rows with ink in its first / last t columns; a mark has top, bottom >=
 * w - w / 8 and left, right >= h - h / 8.  ink_in = the ink pixels of columns x0 + w / 4 .. x1 - w / 4, rows y0 + h / 4 .. y1 - h / 4,
 * area_in = the size of that interior, state = 1 (selected) when 16 ink_in >= area_in.  pages_dev uint8 [n,H,W,3]; marks_dev int32
 * [n][max_marks][8] = x0, y0, x1, y1, top + bottom + left + right, ink_in, area_in, state, sorted by (y0, x0, y1, x1, first run of the
 * component in raster order), rows past the count untouched; counts_dev int32 [n] = the true number of marks (a list whose count
 * exceeds max_marks is not written).  mask_dev: optional parity hook (NULL to skip), the ink mask as hmask_dev of
 * lumina_ocr_table_rules.  4 <= min_side <= max_side <= 64 (a box's window is one 64-bit word per row), max_marks <= 2048, sides
 * 1..65535.  Integer arithmetic throughout: the result is defined bit for bit (tests/mark_reference.py).  Asynchronous; n == 0 is a
 * no-op; bad arguments return a status before anything is written. */
int lumina_ocr_selection_marks(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int min_side,
                               int max_side, int max_marks, int32_t* marks_dev, int32_t* counts_dev, uint64_t* mask_dev, void* stream);

/* lumina_ocr_table_rules and lumina_ocr_selection_marks on the same pages with one threshold: the ink mask is computed once and both
 * read it.  Every output equals that of the two calls made one after the other. */
int lumina_ocr_rules_and_marks(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int gap, int min_len,
                               int max_thick, int max_rules, int32_t* hrules_dev, int32_t* vrules_dev, int32_t* rule_counts_dev, int min_side,
                               int max_side, int max_marks, int32_t* marks_dev, int32_t* mark_counts_dev, void* stream);

/* lumina_ocr_selection_marks plus the ROUND selection marks (radio buttons) of the same pages, in a second list of the same format,
 * order and capacity (round_dev int32 [n][max_marks][8], round_counts_dev int32 [n]; the host half is lumina_ocr/utils/marks.py).  The
 * checkbox outputs are those of lumina_ocr_selection_marks, bit for bit.  A candidate (as above) that passes the frame test is a
 * checkbox and never a round mark: the lists are disjoint.  Any other candidate is read in doubled coordinates about the centre of its
 * box: u = 2 x - (x0 + x1), v = 2 y - (y0 + y1), q = u^2 + v^2, D = max(w, h), T = 1 + D / ring_div.  Zones: outside q > (D + 1)^2; core
 * q <= D^2 / 4; ring zone inner < q <= (D + 1)^2 with inner = max((max(D - 2 T, 0))^2, D^2 / 4); moat = what lies between core and ring
 * zone.  It is a round mark when at most out_max ink pixels of the box lie outside; the ink of the ring zone covers top, bottom >=
 * w - w / 8 columns in the rows with v <= 0 / v >= 0 and left, right >= h - h / 8 rows in the columns with u <= 0 / u >= 0; the moat
 * holds no ink; and the band of band_min + min(w, h) / band_div pixels around the box, clipped to the page, holds no ink (what keeps
 * letters out: a glyph inside a word has a neighbour nearer than that).  Row: x0, y0, x1, y1, top + bottom + left + right, ink_in (the
 * ink of the core), area_in (the pixels of the core), state = 1 when 16 ink_in >= area_in.  out_max >= 0, ring_div >= 1, band_div >= 4,
 * 0 <= band_min <= 16 (the band is at most 32 pixels); defaults in lumina_ocr/arch.py ROUND_MARK_PARAMS.  Integer arithmetic
 * throughout (tests/radio_reference.py).  Asynchronous; n == 0 is a no-op; bad arguments return a status before anything is written. */
int lumina_ocr_selection_marks_round(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int min_side,
                                     int max_side, int max_marks, int32_t* marks_dev, int32_t* counts_dev, uint64_t* mask_dev, int out_max,
                                     int ring_div, int band_div, int band_min, int32_t* round_dev, int32_t* round_counts_dev, void* stream);

/* lumina_ocr_rules_and_marks with the round marks as well: one ink mask for the rules, the checkboxes and the round marks.  Every
 * output equals that of lumina_ocr_table_rules and lumina_ocr_selection_marks_round made one after the other. */
int lumina_ocr_rules_and_marks_round(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int gap,
                                     int min_len, int max_thick, int max_rules, int32_t* hrules_dev, int32_t* vrules_dev,
                                     int32_t* rule_counts_dev, int min_side, int max_side, int max_marks, int32_t* marks_dev,
                                     int32_t* mark_counts_dev, int out_max, int ring_div, int band_div, int band_min, int32_t* round_dev,
                                     int32_t* round_counts_dev, void* stream);

/* Barcodes: Code 128 and Code 39 strips of the pages, read on the device (the host half is lumina_ocr/utils/barcodes.py).  ink as in
 * lumina_ocr_table_rules.  A row of the ink is a list of runs; its elements are the run widths (bars) and the gaps between them.
 * Read from a bar to the right, or to the left (a strip printed upside down: flags bit 0), symbol k of a Code 128 is elements
 * 6 k .. 6 k + 5 (11 modules), of a Code 39 elements 10 k .. 10 k + 8 (15 modules, wide = 3) with element 10 k + 9 the gap between
 * characters.  A symbol of S pixels is matched against every pattern p of its table by d = sum |w_i M - p_i S|: the lowest d wins,
 * ties go to the lowest value, d > max_dist S M / 256 rejects.  A Code 128 reads when symbol 0 is a start (103-105), the first stop
 * (106: its first six elements, then a bar of 1.5 .. 2.5 modules) is symbol k >= 2, the symbols between are <= 102 and the mod-103
 * checksum holds; a Code 39 when symbol 0 is `*` (43), the first later `*` ends it, and every gap between characters is at most two
 * modules.  2..64 symbols; the gap before the start is at least `quiet` module widths of the start symbol (the page edge is quiet).
 * Scanning a row bar by bar to the right a read claims its bars, the same to the left; a read to the left that shares a bar with one
 * to the right is dropped, and the four leftmost reads are the row's.  Columns are read the same way on the transposed mask (flags
 * bit 1: top to bottom, or reversed).  Reads of one direction join when kind, reversal and symbols are equal, their ranges along the
 * code overlap and their rows are at most row_gap apart; a group of at least min_rows reads is a barcode, its box the hull.
 * codes_dev int32 [n][max_codes][8] = x0, y0, x1, y1 (inclusive), kind (0 Code 128, 1 Code 39), nsym, rows (the reads of the group),
 * flags, sorted by (y0, x0, y1, x1, first read in row-then-column raster order), rows past the count untouched; syms_dev int32
 * [n][max_codes][64] = the symbol values in reading order (Code 128: start, data, check, stop; Code 39: character indices with both
 * `*`), zero behind nsym; counts_dev int32 [n] = the true number (a list whose count exceeds max_codes is not written).  mask_in_dev:
 * optional, the ink mask of these pages at this threshold (as hmask_dev of lumina_ocr_table_rules), computed already; mask_out_dev:
 * optional parity hook, receives the mask.  0 <= quiet <= 64, 0 <= max_dist <= 256, min_rows >= 1, 1 <= row_gap <= 16, max_codes
 * 1..256, sides 1..65535; defaults in lumina_ocr/arch.py BARCODE_PARAMS.  Integer arithmetic throughout: the result is defined bit for
 * bit (tests/barcode_reference.py).  Asynchronous; n == 0 is a no-op; bad arguments return a status before anything is written. */
int lumina_ocr_barcodes(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int quiet, int max_dist,
                        int min_rows, int row_gap, int max_codes, int32_t* codes_dev, int32_t* syms_dev, int32_t* counts_dev,
                        const uint64_t* mask_in_dev, uint64_t* mask_out_dev, void* stream);

/* lumina_ocr_barcodes with the kinds to read: `kinds` is a bit mask, bit k = kind k, of 0 Code 128, 1 Code 39, 2 EAN-13 (UPC-A is an
 * EAN-13 whose first digit is 0), 3 EAN-8, 4 UPC-E, 5 ITF (Interleaved 2 of 5); 1 <= kinds <= 63, and kinds = 3 is lumina_ocr_barcodes
 * bit for bit.  At a bar the kinds of the set are tried in that order and the first that reads claims its bars; scan, directions,
 * slots, merge and outputs are lumina_ocr_barcodes'.  A GUARD of n elements beside a digit of S pixels holds when its elements match
 * n single modules by the measure (M = n) and its G pixels are n of the digit's seven modules within a quarter (4 |7 G - n S| <= n S).
 * EAN-13 (30 bars), EAN-8 (22), UPC-E (17): start guard = elements 0-2 beside digit 0; digit k = four elements (7 modules) from
 * element 3 + 4 k, behind the centre guard from 8 + 4 k; centre guard = five elements behind the left half (EAN-13: 6 digits, EAN-8: 4),
 * beside the digit before it; end guard = three elements (UPC-E: six) behind the last digit, beside it.  The gap before the first bar
 * is at least `quiet` modules of digit 0 and the gap behind the last bar the same of the last digit (the page edge is quiet).  A
 * left-half digit is matched against sets L and G, a right-half digit against set R.  EAN-13: the L / G pattern is the first digit
 * and the 13 digits pass the mod-10 check (nsym 13).  EAN-8: the left half is all L and the 8 digits pass mod 10 (nsym 8).  UPC-E: the
 * pattern gives number system and check digit, which is the mod-10 check digit of the UPC-A the six digits abbreviate; symbols =
 * number system, six digits, check digit (nsym 8).  ITF: start = elements 0-3, four single modules by the measure with a gap of
 * `quiet` of them before it; pair k = elements 4 + 10 k .. 13 + 10 k, its five bars one digit and its five spaces the next (two wide
 * of five, weights 1, 2, 4, 7, 0, digit 0 = 4 + 7), each matched on its own sum at M half-modules (narrow 2, wide (M - 6) / 2); M is
 * the one of 14, 16, 18 (wide : narrow = 2, 2.5, 3) whose best pattern for pair 0's bars has the lowest d * (1008 / M), ties to the
 * lower, and the start is 8 half-modules of that quintuple within a quarter; the stop behind pair k = its next three elements matched
 * against wide, narrow, narrow, M / 2 + 1 half-modules of the pair's bars within a quarter, with a gap of `quiet` modules (or the page
 * edge) behind it; the code ends at the first pair k >= 2 with a stop and every pair up to it matched: 6..64 digits, an even count
 * (nsym = the digits).  ITF has no check symbol; 14 digits that pass mod 10 set flags bit 2 (ITF-14).  The symbol values of kinds 2-5
 * are the digits.  Everything else as lumina_ocr_barcodes; kinds of 0 or with unknown bits is a bad-argument status before anything is
 * written.  Integer arithmetic throughout: the result is defined bit for bit (tests/linear_reference.py). */
int lumina_ocr_barcodes_kinds(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int quiet, int max_dist,
                              int min_rows, int row_gap, int max_codes, int32_t* codes_dev, int32_t* syms_dev, int32_t* counts_dev,
                              const uint64_t* mask_in_dev, uint64_t* mask_out_dev, void* stream, int kinds);

/* QR codes: QR Code Model 2 symbols (ISO/IEC 18004) of versions 1-10 on the pages, located, sampled and error-corrected on the device
 * (the host half is lumina_ocr/utils/qrcodes.py).  ink as in lumina_ocr_table_rules.  Of the 8-connected components of the ink a CORE
 * is a solid square (sides 3 min_module .. 3 max_module, 4 |w - h| <= min(w, h), 4 area >= 3 w h) whose centre row has, before and
 * after the core's run, two runs of one other component, the RING, concentric within centre_tol / 16 of a module and 7/3 of the
 * core's size within ring_tol / 16 of a module (the ring's w + h stands for 14 modules): a finder, its centre the ring's in doubled
 * pixel coordinates.  A finder A is a symbol's corner with the partners B (+x) and C (+y) when |AB|^2 and |AC|^2 agree within a
 * quarter, |cos| <= 1/8, cross(AB, AC) > 0 in image coordinates (all four rotations, no mirror images), the module estimates agree
 * within a quarter and a version lies within three modules of |AB|; the valid pairs are tried in the order of |AB|^2 + |AC|^2
 * (then the partners' roots), eight at most, and the first that decodes is the corner's symbol.  Module (col i, row j) is the ink
 * at A + ((i - 3) AB + (j - 3) AC) / (D - 7), rounded down to a pixel, clear off the page.  Of the versions in reach the one with the fewest timing-pattern mismatches is read (at most timing_max); the
 * `quiet` rings of modules round the symbol must be clear; the format information is the nearer of the 32 words within distance 3,
 * the first copy preferred; the codewords are unmasked, read in placement order, de-interleaved and corrected block by block over
 * GF(256) (0x11D, roots alpha^0 ..), and the syndromes of the corrected block must vanish.
 * codes_dev int32 [n][max_codes][12] = x0, y0, x1, y1 (the hull of the symbol's corners, inclusive), version, level (0..3 = L, M, Q,
 * H), mask, ndata, corrected errors, rotation (quarter turns clockwise), format distance (+ 16 when the second copy was read), timing
 * mismatches; sorted by (y0, x0, y1, x1, root of the corner finder's core), rows past the count untouched; data_dev int32
 * [n][max_codes][288] = the corrected data codewords, zero behind ndata; counts_dev int32 [n] = the true number (a list whose count
 * exceeds max_codes is not written); finder_counts_dev: optional, int32 [n] = the finders of each page (a page with more than
 * max_finders is not read: its count is 0).  mask_in_dev / mask_out_dev as in lumina_ocr_barcodes.  1 <= min_module <= max_module <= 64,
 * 0 <= quiet <= 4, 0 <= centre_tol, ring_tol <= 64, 0 <= timing_max <= 128, max_finders 1..64, max_codes 1..64, sides 1..65535;
 * defaults in lumina_ocr/arch.py QR_PARAMS.  Integer arithmetic throughout: the result is defined bit for bit
 * (tests/qr_reference.py).  Asynchronous; n == 0 is a no-op; bad arguments return a status before anything is written. */
int lumina_ocr_qrcodes(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int min_module, int max_module,
                       int quiet, int centre_tol, int ring_tol, int timing_max, int max_finders, int max_codes, int32_t* codes_dev,
                       int32_t* data_dev, int32_t* counts_dev, int32_t* finder_counts_dev, const uint64_t* mask_in_dev, uint64_t* mask_out_dev,
                       void* stream);

/* QR codes of every version: QR Code Model 2 symbols of versions 1 .. max_version (10 <= max_version <= 40) in two stages.  STAGE 1 is
 * lumina_ocr_qrcodes itself: the same ink, components, finders, pairs and decode of versions 1-10, with the same result bit for bit; at
 * max_version = 10 nothing else runs.  STAGE 2 runs for every finder A to which stage 1 gave no symbol.  A's pairs (B, C) pass stage 1's
 * geometric tests; version v in 11 .. max_version, n = 10 + 4 v modules between finder centres, is in reach when
 * (2 (n - w) M)^2 <= 882 (|AB|^2 + |AC|^2) <= (2 (n + w) M)^2 with w = 3 + n / 16 and M = meA + meB + meC (doubled pixels); the valid
 * pairs with a version in reach are tried in the order of |AB|^2 + |AC|^2 (then the partners' roots), eight at most, and the first that
 * decodes is the corner's symbol.  Per pair, for every version in reach only row 6 and column 6 are sampled on that version's grid
 * (the module formula of lumina_ocr_qrcodes with that n) and the version with the fewest timing mismatches is kept, the smaller on a
 * tie; more than timing_max * D / 57 mismatches (D = 17 + 4 v, rounded down) drop the candidate.  The version information must agree:
 * the top-right copy within Hamming distance 3 of the version's 18-bit word (generator 0x1F25), otherwise the bottom-left copy,
 * otherwise the candidate is dropped.  Then as stage 1: the whole grid is sampled once, the `quiet` rings must be clear, the format
 * information is read (first copy, then second), the codewords are unmasked, read in placement order (two-column strips from the right
 * edge, alternately up and down, column 6 skipped, function modules skipped: finders, separators, timing, format, version and
 * alignment patterns, the dark module), de-interleaved and corrected block by block over GF(256) (0x11D, roots alpha^0 ..), up to 81
 * blocks of up to 153 codewords, and the syndromes of every corrected block must vanish.  The grid is affine through the three
 * finders at every version: alignment patterns are function modules only, so a symbol must be flat and nearly upright.
 * codes_dev int32 [n][max_codes][12]: the twelve fields and the sort key of lumina_ocr_qrcodes, rows past the count untouched;
 * data_dev uint8 [n][max_codes][2956] = the corrected data codewords as bytes (40-L has 2956), zero behind ndata; counts_dev,
 * finder_counts_dev, mask_in_dev / mask_out_dev and the parameters' ranges as in lumina_ocr_qrcodes.  Integer arithmetic throughout:
 * the result is defined bit for bit (tests/qr_versions_reference.py).  Asynchronous; n == 0 is a no-op; bad arguments (max_version
 * outside 10..40 among them) return a status before anything is written. */
int lumina_ocr_qrcodes_versions(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int min_module,
                                int max_module, int quiet, int centre_tol, int ring_tol, int timing_max, int max_finders, int max_codes,
                                int max_version, int32_t* codes_dev, uint8_t* data_dev, int32_t* counts_dev, int32_t* finder_counts_dev,
                                const uint64_t* mask_in_dev, uint64_t* mask_out_dev, void* stream);

/* Data Matrix: ECC 200 symbols (ISO/IEC 16022) of the 21 sizes whose rows fit one 64-bit word (10 x 10 .. 52 x 52, 8 x 18 .. 16 x 48) on
 * the pages, located, sampled and error-corrected on the device (the host half is lumina_ocr/utils/datamatrix.py).  ink as in
 * lumina_ocr_table_rules.  Every 8-connected component of the ink has its box, its area and four diagonal extremes (the pixels that
 * minimise x + y, maximise x - y, maximise x + y, minimise x - y, ties by the smaller y); it is a CANDIDATE when its box sides lie in
 * 8 min_module .. 52 max_module and 32 area >= w h.  With nothing touching it, the component of a symbol's L finder has three of
 * its extremes at the L's outer corners at any residual skew; the fourth corner is completed as a parallelogram.  Every rotation
 * (quarter turns clockwise, the elbow at one extreme and the arms to its neighbours) and every size whose two module sizes lie in
 * min_module .. max_module and agree within a quarter is tried: a module is the ink at its centre on the affine grid, clear off the
 * page; the try with the fewest mismatches in the clock tracks and inner clock bars is read (ties: fewer clear modules in the L and
 * the inner solid bars, smaller area, smaller rotation), at most timing_max mismatches and solid_max clear modules; the `quiet`
 * rings of modules round the symbol must be clear; the codewords are read through the placement, de-interleaved (52 x 52) and
 * corrected block by block over GF(256) (0x12D, roots alpha^1 ..), and the syndromes of the corrected block must vanish.
 * codes_dev int32 [n][max_codes][12] = x0, y0, x1, y1 (the hull of the symbol's corners, inclusive), rows, cols, ndata, corrected
 * errors, rotation (quarter turns clockwise), timing mismatches, L misses, 0; sorted by (y0, x0, y1, x1, root of the component), rows
 * past the count untouched; data_dev int32 [n][max_codes][208] = the corrected data codewords, zero behind ndata; counts_dev int32 [n]
 * = the true number (a list whose count exceeds max_codes is not written); candidate_counts_dev: optional, int32 [n] = the candidates
 * of each page (a page with more than max_candidates is not read: its count is 0).  mask_in_dev / mask_out_dev as in
 * lumina_ocr_barcodes.  1 <= min_module <= max_module <= 64, 0 <= quiet <= 4, 0 <= timing_max, solid_max <= 128, max_candidates 1..1024,
 * max_codes 1..64, sides 1..65535; defaults in lumina_ocr/arch.py DM_PARAMS.  Not read: 64 x 64 and larger (lumina_ocr_datamatrix_sizes below reads them), ECC 000-140,
 * light-on-dark and mirrored symbols, perspective, a symbol that other ink touches.  Integer arithmetic throughout: the result is
 * defined bit for bit (tests/dm_reference.py).  Asynchronous; n == 0 is a no-op; bad arguments return a status before anything is
 * written. */
int lumina_ocr_datamatrix(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int min_module, int max_module,
                          int quiet, int timing_max, int solid_max, int max_candidates, int max_codes, int32_t* codes_dev, int32_t* data_dev,
                          int32_t* counts_dev, int32_t* candidate_counts_dev, const uint64_t* mask_in_dev, uint64_t* mask_out_dev, void* stream);

/* lumina_ocr_datamatrix_sizes: lumina_ocr_datamatrix for every ECC 200 size, up to max_size (52 .. 144) modules a side.  STAGE 1 is
 * lumina_ocr_datamatrix itself: the same candidates, rows and codewords, bit for bit, and max_size = 52 reads exactly what it reads.
 * STAGE 2 (max_size >= 64) reads the squares of 64 x 64 .. 144 x 144 (4 x 4 or 6 x 6 regions, 2 .. 10 interleaved blocks) whose side is
 * at most max_size.  It has a candidate list of its own, so that stage 1's count and its max_candidates cut-off do not move: the
 * roots that pass the area test and whose box sides lie in 64 min_module .. 144 max_module, up to max_candidates of them (a page
 * with more is not read by stage 2; stage 1's rows stand).  A root that gave a stage-1 row is skipped.  Tries, score (over all clock
 * and solid rows and columns of the regions), quiet rings, placement and Reed-Solomon as in stage 1; the blocks are dealt by stream
 * position: the codeword at position p of data + check belongs to block p mod blocks, which for 144 x 144 (1558 data codewords in ten
 * blocks, eight of 156 + 62 and two of 155 + 62) makes the check codewords carry on from block 8.  The nine size rows and this
 * interleave are written from recollection of the standard and pinned structurally and by this project's own encoder only.
 * Both stages' rows are sorted together by the key of lumina_ocr_datamatrix; codes_dev as there; data_dev uint8 [n][max_codes][1560]
 * = the corrected data codewords, zero behind ndata; candidate_counts_dev is stage 1's.  The other parameters, their ranges and
 * mask_in_dev / mask_out_dev as in lumina_ocr_datamatrix.  Integer arithmetic throughout: the result is defined bit for bit
 * (tests/dm_sizes_reference.py).  Asynchronous; n == 0 is a no-op; bad arguments (max_size outside 52..144 among them) return a
 * status before anything is written.  lumina_ocr_datamatrix_sizes_workspace_bytes: the workspace of n pages (0 for bad arguments). */
size_t lumina_ocr_datamatrix_sizes_workspace_bytes(int n, int height, int width, int max_candidates, int max_codes);
/* Host only, no device needed: the placement table the second stage uses for the side x side symbol (64 .. 144), built by the
 * library from the standard's walk: (row << 8 | col) of every codeword bit, the most significant bit of a codeword first, into
 * out[capacity] -> the number of entries, 0 for another side or too small a capacity. */
int lumina_ocr_datamatrix_placement(int side, uint16_t* out, int capacity);
int lumina_ocr_datamatrix_sizes(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int min_module,
                                int max_module, int quiet, int timing_max, int solid_max, int max_candidates, int max_codes, int max_size,
                                int32_t* codes_dev, uint8_t* data_dev, int32_t* counts_dev, int32_t* candidate_counts_dev,
                                const uint64_t* mask_in_dev, uint64_t* mask_out_dev, void* stream);

/* Aztec codes (ISO/IEC 24778, written from recollection of the public symbology): compact symbols of 1-4 layers and full-range
 * symbols of 1-11 layers (15 .. 61 modules: the symbols whose rows fit one 64-bit word) on the pages, located, sampled and
 * error-corrected on the device (the host half is lumina_ocr/utils/aztec.py).  ink as in lumina_ocr_table_rules.  The FINDER is the
 * bullseye's core: a component whose box sides lie in min_module .. max_module, square within a quarter and at least three quarters
 * ink, whose neighbours on its centre row both belong to one other component, the 5-module ring: sides five of the core's within
 * ring_tol / 16 of a module, concentric within centre_tol / 16, 12/25 .. 20/25 of its box ink.  A page with more than max_finders
 * finders is not read.  A FRAME is the ring's centre, a slope t / 128 and a pitch (the ring's box sides are ten modules) scaled by
 * (256 + 2 k) / 256; a point of it is a pixel by integer multiplications and shifts, clear off the page.  For either kind the frame
 * (k even in -12 .. 12, t in -4, 0, 4) with the fewest mismatches in the bullseye is taken, the rotation is the one with the fewest
 * mismatches in the mode ring's twelve corner modules, and the mode message is corrected over GF(16); the kind with the fewest
 * mismatches (at most mark_max) that corrects and is in scope is read (ties: fewer mode errors, compact).  The size known, the frame
 * (k in -12 .. 12, t in -6 .. 6) with no ink a quarter module outside the symbol's outline, the fewest mismatches on the centre
 * reference lines and the most ink a quarter module inside the outline is taken; the `quiet` rings of modules must be clear; the
 * codewords are read through the layer spiral and corrected as one block over GF(64) / GF(256) / GF(1024), and the syndromes of the
 * corrected block must vanish.
 * codes_dev int32 [n][max_codes][12] = x0, y0, x1, y1 (the hull of the symbol's corners, inclusive), layers, compact (0 / 1), codeword
 * width, ndata, corrected errors, rotation (quarter turns clockwise), mode-message errors, bullseye + corner + reference-line
 * mismatches; sorted by (y0, x0, y1, x1, root of the core), rows past the count untouched; data_dev int32 [n][max_codes][320] = the
 * corrected data codewords, still bit-stuffed, zero behind ndata; counts_dev int32 [n] = the true number (a list whose count exceeds
 * max_codes is not written); finder_counts_dev: optional, int32 [n] = the finders of each page.  mask_in_dev / mask_out_dev as in
 * lumina_ocr_barcodes.  1 <= min_module <= max_module <= 64, 0 <= quiet <= 4, 0 <= centre_tol <= 64, 0 <= ring_tol <= 15,
 * 0 <= mark_max <= 64, max_finders 1..64, max_codes 1..64, sides 1..65535; defaults in lumina_ocr/arch.py AZTEC_PARAMS.  Not read:
 * full-range symbols of 12-32 layers (lumina_ocr_aztec_layers below reads them), runes, light-on-dark and mirrored symbols,
 * perspective, a bullseye that other ink touches.
 * Integer arithmetic throughout: the result is defined bit for bit (tests/aztec_reference.py).  Asynchronous; n == 0 is a no-op; bad
 * arguments return a status before anything is written.  lumina_ocr_aztec_workspace_bytes: the workspace n pages of that size need
 * in one launch (0: bad arguments); the entry itself splits n into groups that fit the handle's workspace. */
size_t lumina_ocr_aztec_workspace_bytes(int n, int height, int width, int max_finders, int max_codes);
int lumina_ocr_aztec(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int min_module, int max_module,
                     int quiet, int centre_tol, int ring_tol, int mark_max, int max_finders, int max_codes, int32_t* codes_dev, int32_t* data_dev,
                     int32_t* counts_dev, int32_t* finder_counts_dev, const uint64_t* mask_in_dev, uint64_t* mask_out_dev, void* stream);

/* lumina_ocr_aztec_layers: lumina_ocr_aztec for full-range symbols of every size, up to max_layers (11 .. 32) layers and 151 modules a
 * side.  Stage 1 is lumina_ocr_aztec itself: every symbol it reads is in this list with the same 12 ints and the same data codewords
 * (max_layers = 11 gives exactly its list).  A full-range finder whose mode message says 12 .. max_layers layers, and that stage 1
 * gave no row for, goes to stage 2, one wave per finder.  Its frame is finer: the ring's centre, a slope t / 1024 and a pitch of
 * (1024 + k) / 1024 of the ring's tenth.  From the bullseye's frame it is refined outwards along the centre reference lines, at the
 * radii 16, 32, 64 modules and the symbol's half side with steps of 8, 4, 2, 1: of the 9 x 9 neighbouring frames the middle of those
 * with the fewest mismatches a quarter module round the lines' module centres is kept.  It is finished on the outline: of the 9 x 9
 * nearest frames with no ink a quarter module outside it and some ink a quarter module inside it, the one with the fewest mismatches
 * on the centre lines, then the nearest.  The `quiet` rings must be clear; module rows are three 64-bit words; the codewords are 10
 * bits over GF(1024) up to 22 layers and 12 bits over GF(4096) / 0x1069 from 23 layers; the hull is the box of the outline's corners,
 * each at its nearest pixel.
 * codes_dev and counts_dev as lumina_ocr_aztec, both stages' rows sorted together; data_dev uint16 [n][max_codes][1664], zero behind
 * ndata.  The parameters' ranges as lumina_ocr_aztec, and 11 <= max_layers <= 32; a finder whose mode message says more layers than
 * max_layers is dropped.  Not read: runes, light-on-dark and mirrored symbols, perspective, a bullseye that other ink touches.
 * Integer arithmetic throughout: the result is defined bit for bit (tests/aztec_layers_reference.py).  Asynchronous; n == 0 is a
 * no-op; bad arguments return a status before anything is written.  lumina_ocr_aztec_layers_workspace_bytes as
 * lumina_ocr_aztec_workspace_bytes. */
size_t lumina_ocr_aztec_layers_workspace_bytes(int n, int height, int width, int max_finders, int max_codes);
int lumina_ocr_aztec_layers(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int min_module, int max_module,
                            int quiet, int centre_tol, int ring_tol, int mark_max, int max_finders, int max_codes, int max_layers, int32_t* codes_dev,
                            uint16_t* data_dev, int32_t* counts_dev, int32_t* finder_counts_dev, const uint64_t* mask_in_dev, uint64_t* mask_out_dev,
                            void* stream);

/* ---- page orientation (optional; DESIGN.md: "Page orientation") ----
 * A page is upright after `turn` quarter turns: upright = np.rot90(page, turn) (counter-clockwise).  The three entries below are the
 * device half; which pages get which turn is decided on the host (lumina_ocr/utils/page_orient.py, OcrPipeline.run_oriented).
 *
 * lumina_ocr_page_quarter: is a page sideways?  ink as in lumina_ocr_table_rules (L < threshold, Pillow's luma); r[y] / c[x] = the ink
 * pixels of row y / column x; E_r = sum over y of (r[y+1] - r[y])^2, E_c likewise over x, in 64-bit integers: text lines make the
 * profile across them jagged and the one along them flat.  energies_dev int64 [n][2] = E_r, E_c; sideways_dev int32 [n] = 1 when
 * E_c > ratio * E_r (a blank page: 0).  pages_dev uint8 [n,H,W,3], sides 1..65535, ratio 1..1024.  A heuristic, not a model: a page
 * whose ink is mostly long vertical rules is misjudged.  Integer arithmetic throughout: defined bit for bit
 * (tests/page_orient_reference.py).  Asynchronous; n == 0 is a no-op; bad arguments return a status before anything is written.
 * lumina_ocr_page_quarter_workspace_bytes: the workspace n pages of that size need in one launch (0: bad dimensions); the entry itself
 * works in groups of pages bounded by 1 GiB.
 *
 * lumina_ocr_page_turn: out_dev uint8 [m][H'][W'][3], page j = np.rot90(pages[index[j]], turn) byte for byte; (H', W') = (W, H) for
 * turn 1 and 3.  index_dev int32 [m] on the device, entries in 0..n-1, in any order, with repeats (an entry outside the range leaves
 * its page unwritten).  Not in place.  Asynchronous; m == 0 is a no-op.
 *
 * lumina_ocr_page_vote: counts_dev int32 [pages][2] = the lines of each page and those among them whose flip flag is set, from
 * lumina_ocr_cls_forward's flip_dev int32 [n] and the lines' page_idx_dev int32 [n] (entries outside 0..pages-1 are not counted).
 * Asynchronous; n == 0 writes zeros. */
size_t lumina_ocr_page_quarter_workspace_bytes(int n, int height, int width);
int lumina_ocr_page_quarter(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int threshold, int ratio,
                            int64_t* energies_dev, int32_t* sideways_dev, void* stream);
int lumina_ocr_page_turn(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, const int32_t* index_dev, int m, int turn,
                         uint8_t* out_dev, void* stream);
int lumina_ocr_page_vote(lumina_ocr_t* h, const int32_t* flip_dev, const int32_t* page_idx_dev, int n, int pages, int32_t* counts_dev, void* stream);

/* ---- page composition (optional; DESIGN.md §3: "Layered PDF pages") ----
 * A scanned PDF page painted from several images (strips, a stencil over a background, images with a soft or an explicit mask) is
 * put together from its decoded layers.  lumina_ocr/utils/pdf_pages.py finds the layers and computes the integer canvas; the
 * device sees integers only.
 *
 * lumina_ocr_page_compose: out_dev uint8 [n][height][width][3].  layers: HOST array of n_layers records, the layers of page 0 first,
 * each page's in paint order (pages ascending; at most 64 layers a page; a page may have none).  A pixel starts at 255, 255, 255
 * and is painted once per layer of its page, in that order, for each layer whose rectangle x0 <= x < x1, y0 <= y < y1 holds it
 * (the rectangle may stick out of the canvas; it must meet it and |coordinate| <= 2^24):
 *   sampling  the sample that holds the pixel centre (PDF's rule without /Interpolate):
 *             u = floor((2 (x - x0) + 1) w / (2 (x1 - x0))), v likewise from y and h; for the mask the same with mw, mh over the
 *             same rectangle.  (x1 - x0 == w is the identity u = x - x0.)
 *   kind 0    opaque image:        c = src[v][u]
 *   kind 1    stencil:             c = fill where (mask[v][u] < 128) != flip            (fill = r | g << 8 | b << 16)
 *   kind 2    image with /SMask:   a = flip ? 255 - mask[v][u] : mask[v][u]; per channel c = div255(src * a + c * (255 - a)),
 *             div255(t) = (t + 128 + ((t + 128) >> 8)) >> 8  (= t / 255 rounded to nearest)
 *   kind 3    image with /Mask:    c = src[v][u] unless (mask[v][u] >= 128) != flip     (that sample is masked out)
 * src and mask are device images as the decoders write them, uint8 [h][w][3] and [mh][mw][3]; a mask is read from channel 0.
 * Pure integer arithmetic, every output byte written exactly once: defined byte for byte (tests/pdf_layers_reference.py).
 * The table is checked on the host before anything is launched (sides 1..65535, kinds 0..3, non-empty rectangles that meet the
 * canvas, a source for kinds 0 / 2 / 3 and a mask for kinds 1 / 2 / 3 with sides 1..65535, at most 64 layers a page): a table that
 * fails returns 1 with the reason in lumina_ocr_last_error and launches nothing.  The table is copied to the device through the
 * engine's own buffers: the caller may free it when the call returns.  Asynchronous; n == 0 is a no-op. */
typedef struct {
    int32_t page, kind;          /* page 0..n-1; kind 0..3 */
    int32_t x0, y0, x1, y1;      /* canvas rectangle */
    int32_t flip, fill;          /* polarity of the mask (0 | 1); fill colour of a stencil */
    const uint8_t* src;          /* device, [h][w][3] (kinds 0, 2, 3) */
    int32_t w, h;
    const uint8_t* mask;         /* device, [mh][mw][3] (kinds 1, 2, 3) */
    int32_t mw, mh;
} lumina_ocr_compose_layer;
int lumina_ocr_page_compose(lumina_ocr_t* h, const lumina_ocr_compose_layer* layers, int n_layers, int n, int height, int width,
                            uint8_t* out_dev, void* stream);

/* Second recogniser family (BASELINE configs[4]: "SVTR-base multilingual (Hindi dict), fp16 MFMA"): same slot and the same outputs as
 * lumina_ocr_load_rec_weights / lumina_ocr_rec_forward (the `rec` model of the engine call, ocr_service_paddleocr_backup.py:232-238,
 * :285), with an SVTR backbone (patch embedding, local / global mixing blocks, CTC head) instead of CRNN.  Blob: LOCW with the
 * `svtr.*` tensors of lumina_ocr/arch.py make_svtr_weights; the optional f32 tensor `svtr.config` = [dim0, dim1, dim2, depth0,
 * depth1, depth2, heads0, heads1, heads2, local_blocks, out_channels, dtype] selects the variant (absent: SVTR-Tiny, bf16;
 * Base = 128/256/384, 3/6/9, 4/8/12, 8 local blocks) and the storage / MFMA type (0 bf16, 1 fp16: v_mfma_f32_32x32x16_f16,
 * activations and weights stored as IEEE half); option "svtr_f16" (0 / 1, -1 = as the blob says) overrides the type at load time.  Every svtr.config value must be a
 * whole number 0 .. 65536 (checked before it is converted: NaN, infinities and fractions are refused); dims 64 / 128 / 256 / 384 with
 * 32-wide heads and dims[0] <= 128, depths 1 .. 32, local_blocks <= depth0 + depth1, out_channels 192, dtype 0 / 1.  The tensor list
 * is derived from these values; refusals as lumina_ocr_load_det_weights states. */
int lumina_ocr_load_svtr_weights(lumina_ocr_t* h, const void* blob, size_t nbytes);
int lumina_ocr_svtr_forward(lumina_ocr_t* h, const uint8_t* crops_dev, const int32_t* widths_dev, int n_crops, int32_t* idx_dev, float* prob_dev,
                            void* stream);
int lumina_ocr_svtr_num_classes(const lumina_ocr_t* h);   /* class count of the loaded SVTR head (lumina_ocr_num_classes: the CRNN's) */
int lumina_ocr_svtr_dtype(const lumina_ocr_t* h);         /* storage / MFMA type of the loaded SVTR model: 0 bf16, 1 fp16 */

/* JPEG hand-off of the processed page: replaces image.save(buffer, format='JPEG', quality=q, optimize=True) inside
 * ImagePreprocessor.compress_for_azure (backend/utils/image_preprocessing.py:526-538; the bytes become OCROutput.processed_image_bytes,
 * ocr_service.py:459, saved by backend/utils/file_manager.py:283-287).  Byte-identical to Pillow's output: JFIF 1.01, YCbCr 4:2:0,
 * integer DCT, optimised Huffman tables.  pages_dev: uint8 [n, height, width, 3]; out_dev: uint8 [n, out_stride] receives one complete
 * file per page; sizes_dev[i] = its length, or a negative number (-(length needed), saturated) when it does not fit out_stride — the
 * caller's cue to retry at a lower quality, as the reference's loop does when a file exceeds its 2 MB target.  optimize = 0 writes
 * the typical Huffman tables of T.81 Annex K.3 instead (the reference's size probe `image.save(buffer, 'JPEG', quality=min_quality)`,
 * :548).  Asynchronous on stream. */
int lumina_ocr_jpeg_encode(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int quality, int optimize,
                           uint8_t* out_dev, size_t out_stride, int32_t* sizes_dev, void* stream);
/* Parity hook for the encoder's first half: quantised DCT coefficients, int16 [n][ceil(w/16)*ceil(h/16)][6][64] in zig-zag order
 * (4 luma, Cb, Cr blocks per MCU; dummy edge blocks resolved). */
/* JPEG decode on the device — the pixel work of the reference's Image.open(path) / Image.open(BytesIO(bytes)) for .jpg inputs
 * (ImagePreprocessor.load_image / load_image_bytes, image_preprocessing.py:57-75).  The contract: status 0 => byte-identical to
 * Pillow's decode; any other status => the file is left to Pillow (damaged files Pillow would recover, or decode differently
 * depending on the host CPU's SIMD, are refused with -1: see the acceptance rule in DESIGN.md).
 * lumina_ocr_jpeg_probe (host only, no handle): info = {width, height, components, luma h, luma v, restart interval}; returns 0 for a
 * file the device decodes (sequential Huffman baseline, 8 bit, grey or YCbCr in one interleaved scan, 4:4:4 / 4:2:2 / 4:2:0),
 * -1 corrupt / not a JPEG, -2 valid but outside that subset (progressive, CMYK, ...): decode those with Pillow, as the reference does.
 * lumina_ocr_jpeg_decode: files / sizes are HOST arrays of n file images, all height x width; out_dev uint8 [n][height][width][3]
 * (a grey file: its value on all three channels); status HOST int [n]: 0 ok; -1 corrupt (header, Huffman table, entropy data, restart
 * markers or coefficient range); -2 outside the subset; -4 another size.  A page with a non-zero status is not written.
 * Synchronises `stream` (the parallel Huffman decode iterates to a fixed point). */
int lumina_ocr_jpeg_probe(const uint8_t* file, size_t size, int info[6]);
int lumina_ocr_jpeg_decode(lumina_ocr_t* h, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev,
                           int* status, void* stream);
/* The same without any host synchronisation (a pipeline decodes the next batch while the device still works on the previous one): `passes`
 * synchronisation passes are enqueued blindly (12 suffice for 1 KB chunks on busy A4 pages: 8 needed), `status_pinned` must be pinned host
 * memory and is valid once `stream` has run; -5 = the passes did not reach the fixed point (decode that batch again with the form above). */
int lumina_ocr_jpeg_decode_async(lumina_ocr_t* h, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev,
                                 int* status_pinned, int passes, void* stream);
/* synchronisation passes over the chunk decoders the last lumina_ocr_jpeg_decode call needed (diagnostic) */
int lumina_ocr_jpeg_last_passes(const lumina_ocr_t* h);
/* Progressive JPEG files (SOF2) as well.  The entries above keep their answers (-2 for a progressive file).
 * lumina_ocr_jpeg_probe_progressive (host only): 0 for every file lumina_ocr_jpeg_probe takes, and for progressive Huffman files: 8 bit,
 * grey or YCbCr, 4:4:4 / 4:2:2 / 4:2:0, any legal scan script of at most 32 scans (interleaved or single-component DC scans, any
 * spectral bands and successive-approximation depth, DHT and DRI between scans).  info = {width, height, components, luma h, luma v,
 * restart interval (of the first scan), 1 if progressive, number of scans}.  -2: arithmetic coding, 12 bit, 4 components, more than 32
 * scans, a DQT after the first scan, a first scan over a coefficient that is complete already, or scans that stop short of all 64 coefficients of every component at full precision (libjpeg smooths such a file across
 * blocks); -1: corrupt, an illegal progression included.
 * lumina_ocr_jpeg_decode_progressive: the contract and the status codes of lumina_ocr_jpeg_decode; sequential and progressive files may
 * be mixed in one batch, a sequential file takes the kernels and gives the bytes of lumina_ocr_jpeg_decode.  Synchronises `stream`. */
int lumina_ocr_jpeg_probe_progressive(const uint8_t* file, size_t size, int info[8]);
int lumina_ocr_jpeg_decode_progressive(lumina_ocr_t* h, const uint8_t* const* files, const size_t* sizes, int n, int height, int width,
                                       uint8_t* out_dev, int* status, void* stream);

/* PNG decode on the device — the pixel work of the reference's Image.open(...) + convert('RGB') for .png inputs and for the PNG pages
 * pdf2image returns (image_preprocessing.py:57-75).  The contract is the JPEG pair's: status 0 => byte-identical to Pillow's
 * Image.open(f).convert('RGB'); any other status => the file is left to Pillow (the device accepts a file only where every conformant
 * decoder agrees: see the acceptance rule in DESIGN.md).
 * lumina_ocr_png_probe (host only, no handle): a walk over the chunks before the first IDAT (no pixel data is read); info = {width,
 * height, colour type, bit depth, interlace, palette entries, EXIF orientation of an eXIf chunk before IDAT (0: none), 0}; returns 0 for
 * a file the device decodes (non-interlaced grey 1/2/4/8 bit, RGB 8, palette 1/2/4/8, grey+alpha 8, RGBA 8), -1 corrupt / not a PNG,
 * -2 valid but outside that subset (Adam7, 16 bit, compressed metadata, animation, chunks after the image data): decode those with
 * Pillow, as the reference does.
 * lumina_ocr_png_decode: files / sizes are HOST arrays of n file images, all height x width; out_dev uint8 [n][height][width][3] (a grey
 * file: its value on all three channels; alpha dropped; palette looked up); status HOST int [n]: 0 ok; -1 corrupt (chunk structure, zlib
 * header, DEFLATE stream, inflated size, Adler-32, filter byte or palette index); -2 outside the subset; -4 another size.  A page with a
 * non-zero status is not written.  Synchronises `stream`. */
int lumina_ocr_png_probe(const uint8_t* file, size_t size, int info[8]);
int lumina_ocr_png_decode(lumina_ocr_t* h, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev,
                          int* status, void* stream);

/* Lossless WebP decode on the device — the pixel work of the reference's Image.open(...) + convert('RGB') for .webp inputs
 * (image_preprocessing.py:57-75).  The contract is the JPEG pair's: status 0 => byte-identical to Pillow's (libwebp's)
 * Image.open(f).convert('RGB'); any other status => the file is left to Pillow (the device accepts a file only where every conformant
 * decoder agrees: see the acceptance rule in DESIGN.md).
 * lumina_ocr_webp_probe (host only, no handle): a walk over the RIFF chunks (no pixel data is read); info = {width, height, the VP8L
 * alpha bit, 1 inside a VP8X container, 1 with an EXIF chunk, 1 with an XMP chunk, 0, 0}; returns 0 for a file the device decodes
 * (RIFF / WEBP with one VP8L chunk, bare or inside VP8X; ICCP, EXIF, XMP and unknown chunks skipped), -2 valid WebP that is not read
 * (lossy VP8, an ALPH chunk, animation, more than 2^26 pixels, a VP8L chunk of 256 MB or more): decode those with Pillow, as the reference
 * does; -1 corrupt or irregular (signature byte other than 0x2F, version bits other than 0, a chunk or the RIFF size past the file, bytes
 * after the RIFF payload, chunks after the image of a file without VP8X, a VP8X canvas that differs from the VP8L header).
 * lumina_ocr_webp_reason: why the calling thread's last probe returned `code` (a static string; the generic meaning of the code otherwise).
 * lumina_ocr_webp_decode: files / sizes are HOST arrays of n file images, all height x width; out_dev uint8 [n][height][width][3] (alpha
 * dropped: the stored RGB, not pre-multiplied); status HOST int [n]: 0 ok; -1 corrupt (container, a prefix code that is over- or
 * under-subscribed, a copy before the first or past the last pixel, a transform repeated, colour-cache bits outside 1..11, reading past
 * the chunk); -2 outside the subset (as the probe; more than 4096 prefix-code groups); -4 another size.  A page with a non-zero status
 * is not written.  Synchronises `stream`. */
int lumina_ocr_webp_probe(const uint8_t* file, size_t size, int info[8]);
const char* lumina_ocr_webp_reason(int code);
int lumina_ocr_webp_decode(lumina_ocr_t* h, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev,
                           int* status, void* stream);

/* Lossy WebP (VP8 key frames) on the device, in one batch with lossless files.  The contract is the same: status 0 => byte-identical to
 * Pillow's Image.open(f).convert('RGB'); any other status => the file is left to Pillow.  lumina_ocr_webp_probe / _decode above keep
 * answering -2 for a lossy file.
 * lumina_ocr_webp_probe_lossy (host only, no handle): as lumina_ocr_webp_probe, with the same info fields, and 0 also for a still lossy
 * file: RIFF / WEBP with one `VP8 ` chunk, bare or inside VP8X, without ALPH; a key frame of profile 0..3 with show_frame 1 and start
 * code 9d 01 2a, any size up to 16383 x 16383 and 2^26 pixels (the scale bits are ignored, as libwebp ignores them); segments, both loop
 * filters, 1 / 2 / 4 / 8 token partitions.  info[6] = 1 for a lossy file, info[7] = its number of token partitions.  It reads the
 * frame header (a few hundred boolean-coded flags), no macroblock.  -2: a lossy file with an ALPH chunk, animation, more than 2^26
 * pixels, a chunk of 256 MB or more.  -1: the container cases; a VP8X canvas that differs from the frame header; both a VP8 and a VP8L
 * chunk; an inter frame; a profile above 3; show_frame 0; a wrong start code; a first-partition length, a partition-size table or a
 * partition past the chunk; an empty last partition; a frame header that reads past the first partition.
 * lumina_ocr_webp_reason serves both probes.
 * lumina_ocr_webp_decode_lossy: arguments and statuses as lumina_ocr_webp_decode; lossless files take its kernels and give its bytes.
 * -1 from the decode also covers: a read of the first partition or of a token partition past its end (a decision of the boolean decoder
 * that needs a byte the partition does not have: libwebp pads a truncated token partition with zeros, a strict reader need not), and a
 * block beyond the coefficient bound inside which no inverse transform leaves 16 bits (libwebp's C and SIMD paths differ beyond it): the
 * sum of the absolute values of a block's 16 dequantised coefficients above 19000, or of a macroblock's 16 Y2 values above 32764 (derived
 * in csrc/vp8_dec.h).  Sub-batched by "webp_sub_batch_mb"; synchronises `stream`. */
int lumina_ocr_webp_probe_lossy(const uint8_t* file, size_t size, int info[8]);
int lumina_ocr_webp_decode_lossy(lumina_ocr_t* h, const uint8_t* const* files, const size_t* sizes, int n, int height, int width,
                                 uint8_t* out_dev, int* status, void* stream);

/* JPEG 2000 decode on the device — the pixel work of the reference's Image.open(...) + convert('RGB') for .jp2 / .j2k inputs, and the
 * /JPXDecode pages of scanned PDFs.  The contract is the JPEG pair's: status 0 => byte-identical to Pillow's (OpenJPEG's) decode; any
 * other status => the file is left to Pillow.
 * Read: a raw codestream or a JP2 / JPX-baseline file (ihdr, one colr of method 1 with sRGB or grey, the first jp2c; box length 0 and
 * the 64-bit box length are honoured); one tile, origin 0, 1 or 3 components, 8 bit unsigned, no sub-sampling; the 5/3 reversible
 * transform with 0-6 levels, lossless or cut short by up to 32 quality layers; the five progression orders; one precinct per
 * resolution; code-blocks from 4 x 4 to 64 x 64; code-block style 0; with or without the reversible colour transform; COM, PLT and TLM
 * are skipped.
 * -2 (valid, outside the subset): the 9/7 irreversible transform, tiles, user precincts, a code-block side over 64, any code-block
 * style bit, SOP / EPH, POC / RGN / PPM / PPT / PLM / CRG, a COC or QCC that differs from COD / QCD (or any of the four in a tile-part
 * header), a non-zero origin, sub-sampling, 2 or 4+ components, another bit depth or signed samples, Rsiz other than 0, pclr / cmap /
 * cdef / opct / bpcc boxes, colr of method 2 or sYCC, more than 32 layers or 6 levels, a side over 16384, more than 15 magnitude
 * bit-planes in a sub-band.  -1: anything irregular — the decoder is strict where OpenJPEG is lenient (segments out of order or of the
 * wrong length, a packet header past its tile-part, more coding passes or zero bit-planes than Mb allows, data left over after the last
 * packet, a missing EOC, bytes after it).
 * lumina_ocr_jp2_probe (host only, no handle): the boxes, the headers and the walk over every packet header; no pixel is decoded.
 * info = {width, height, components, decomposition levels, layers, progression order (0 LRCP, 1 RLCP, 2 RPCL, 3 PCRL, 4 CPRL),
 * code-block width, code-block height}, filled as far as the headers were read.  Returns 0, -1 or -2.
 * lumina_ocr_jp2_reason: the reason behind the last non-zero lumina_ocr_jp2_probe result of the calling thread when `code` is that
 * result (a static string, for logs); otherwise the general meaning of `code`.
 * lumina_ocr_jp2_decode: files / sizes are HOST arrays of n file images, all height x width; out_dev uint8 [n][height][width][3] (a grey
 * file: its value on all three channels); status HOST int [n]: 0 ok, -1, -2, -4 another size.  A page with a non-zero status is not
 * written.  Synchronises `stream`. */
int lumina_ocr_jp2_probe(const uint8_t* file, size_t size, int info[8]);
const char* lumina_ocr_jp2_reason(int code);
int lumina_ocr_jp2_decode(lumina_ocr_t* h, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev,
                          int* status, void* stream);
/* 9/7 (irreversible, lossy) JPEG 2000 files as well.  The entries above keep their answers (-2 for a 9/7 file).
 * lumina_ocr_jp2_probe_irreversible (host only): 0 for every file lumina_ocr_jp2_probe takes, and for files of the 9/7 irreversible
 * transform inside the same subset with expounded step sizes (QCD style 2, one 16-bit step per sub-band), at most 15 magnitude
 * bit-planes in a sub-band (OpenJPEG's own files of up to 5 levels, its default) and no line of one sample in a resolution above the
 * lowest; with or without the irreversible colour transform.  -2 besides the list above: 9/7 with derived or no quantisation, 9/7
 * with 16 bit-planes (OpenJPEG's 6-level files), a one-sample line, 5/3 with step sizes.  info and lumina_ocr_jp2_reason as above.
 * lumina_ocr_jp2_decode_irreversible: the contract and the status codes of lumina_ocr_jp2_decode; 5/3 and 9/7 files may be mixed in
 * one batch, a 5/3 file takes the kernels and gives the bytes of lumina_ocr_jp2_decode.  The float arithmetic of the 9/7 path
 * (dequantisation, lifting, colour transform, rounding) is OpenJPEG's operation for operation in single precision, so status 0 =>
 * byte-identical to Pillow here too.  Synchronises `stream`. */
int lumina_ocr_jp2_probe_irreversible(const uint8_t* file, size_t size, int info[8]);
int lumina_ocr_jp2_decode_irreversible(lumina_ocr_t* h, const uint8_t* const* files, const size_t* sizes, int n, int height, int width,
                                       uint8_t* out_dev, int* status, void* stream);
/* Tiled JPEG 2000 files as well: what scanners, Acrobat scan profiles and archive masters write.  `flags` names what is read beyond
 * the first subset; the four entries above keep their answers (-2 for a tiled file, with their reasons).
 * LUMINA_OCR_JP2_F_IRREVERSIBLE: 9/7 files, as the _irreversible entries take them.
 * LUMINA_OCR_JP2_F_TILES: any XOsiz / YOsiz / XTOsiz / YTOsiz the standard allows (Xsiz, Ysiz up to 2^30); a grid of up to 4096
 * tiles, their tile-parts in any order and interleaved, TPsot counting up within each tile, Psot = 0 on the last tile-part; user
 * precinct sizes (COD with Scod & 1); all five progression orders over several precincts; code-blocks clipped to their precinct.
 * height / width, and info[0] / info[1], are those of the image area (Xsiz - XOsiz by Ysiz - YOsiz), which keeps the limits above.
 * Both inverse transforms run per tile-component, and a line whose first canvas coordinate is odd starts with a high-pass sample; the
 * 9/7 refusal of a one-sample line holds per tile-component resolution.  status 0 => byte-identical to Pillow, as everywhere.
 * Still -2: SOP / EPH, POC, coding parameters per tile (COD / COC / QCD / QCC / RGN in a tile-part header), PPM / PPT, sub-sampled
 * components, more than 4096 tiles.  -1 besides the list above: origins that leave the first tile empty, a tile without a tile-part
 * or with fewer than it announces, TPsot out of order within its tile, a tile index outside the grid, a precinct exponent of 0 above
 * resolution 0, a tile whose packets end early or leave data over.  Other flag bits: -1 from the probe, an error from the decode.
 * lumina_ocr_jp2_reason serves lumina_ocr_jp2_probe_ex too.  A one-tile file gives the bytes of the entries above.
 * lumina_ocr_jp2_decode_ex synchronises `stream`. */
#define LUMINA_OCR_JP2_F_IRREVERSIBLE 1u
#define LUMINA_OCR_JP2_F_TILES 2u
int lumina_ocr_jp2_probe_ex(const uint8_t* file, size_t size, unsigned flags, int info[8]);
int lumina_ocr_jp2_decode_ex(lumina_ocr_t* h, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev,
                             int* status, unsigned flags, void* stream);

/* Scanned PDF pages — the images of a PDF whose pages are one image each (utils/pdf_pages.py finds them), decoded at their own sample
 * grid instead of the rasterisation pdf2image / poppler does for the reference (ocr_service.py:508-660).  /DCTDecode streams are JPEG
 * files: lumina_ocr_jpeg_decode.  The two entries below take the other two filters; the batch contract is lumina_ocr_png_decode's:
 * HOST pointers to n same-size streams, out_dev uint8 [n][height][width][3], a HOST status per page (0: exact pixels, -1 corrupt,
 * -2 unsupported; the pixels of a page with a non-zero status are undefined), `stream` synchronised.
 * lumina_ocr_flate_image_decode: /FlateDecode image streams (plain zlib).  params int32 [n][5] = {Predictor (1 packed rows, 2 TIFF
 * horizontal differencing with 8-bit samples, 10..15 PNG row filters), components (1 | 3), bits per component (8; 1 / 2 / 4 with one
 * component), indexed (0 | 1), invert (/Decode [1 0]: one non-indexed component)}; palettes: per indexed stream 768 bytes of RGB (the
 * /Indexed lookup expanded to RGB, entries past hival filled by the caller), null entries elsewhere; may be null without indexed streams.
 * Grey samples map as v * 255 / (2^bits - 1).  -1: zlib header, DEFLATE stream, Adler-32, a PNG filter byte past 4, bytes after the
 * Adler-32, or an inflated length other than rows x row bytes.
 * lumina_ocr_ccitt_decode: /CCITTFaxDecode with K < 0 (ITU-T T.6, Group 4).  params int32 [n][4] = {K, EncodedByteAlign, BlackIs1,
 * invert}; -2 for K >= 0, EncodedByteAlign or columns > 8192 (CC_MAX_COLS, ccitt.h).  Decoding stops after `rows` lines or at
 * EOFB, whichever comes first; bytes after that are ignored.  A coded-white run is sample 1 unless BlackIs1; sample 1 is white (255)
 * unless invert.  -1: an unused code, a line whose a0 does not advance or passes `columns`, a pass code whose b2 is the line's end,
 * more than columns + 1 changing elements on a line, bits past the stream's end, or fewer than `rows` lines.
 * lumina_ocr_fax_decode: the same arguments with params int32 [n][5] = {K, EncodedByteAlign, BlackIs1, invert, path}: every
 * /CCITTFaxDecode coding, and the strips of TIFF Compression 2 (CCITT RLE), 3 (Group 3, TIFF-F) and 4.  K < 0 is decoded exactly as
 * by lumina_ocr_ccitt_decode.  K = 0: ITU-T T.4 one-dimensional lines; K > 0: the bit after each EOL says whether the line is one- or
 * two-dimensional.  EOLs are found, not announced: at each line's start zero bits are skipped (fill of any length), and 11 or more of
 * them followed by a 1 are an EOL; a stream has one in front of every line or of none (its first line decides).  EncodedByteAlign: in
 * a stream without EOLs every line begins on a byte boundary (Compression 2).  Decoding stops after `rows` lines; an RTC or anything
 * else behind them is ignored.  path: 0 automatic, 1 the serial walk; 2 is reserved for a line-parallel decode and answers -2.
 * -1 (the host's libtiff is lenient, this decoder is not): an unused code, a line whose runs do not add up to `columns` exactly, a run
 * of length 0 other than a line's first, the two-dimensional violations listed above, an EOL in front of some lines only, two EOLs
 * in a row before `rows` lines, bits other than 0 between a line's end and the next EOL, bits past the stream's end.  -2: K > 0 in a
 * stream without EOLs (PDF allows it; libtiff cannot express it, so nothing can serve as its oracle), EncodedByteAlign in a stream
 * with EOLs (the same), a path other than 0 / 1, columns > 8192.  T.4's uncompressed mode is not decoded. */
int lumina_ocr_flate_image_decode(lumina_ocr_t* h, const uint8_t* const* streams, const size_t* sizes, int n, int height, int width,
                                  const int32_t* params, const uint8_t* const* palettes, uint8_t* out_dev, int* status, void* stream);
int lumina_ocr_ccitt_decode(lumina_ocr_t* h, const uint8_t* const* streams, const size_t* sizes, int n, int rows, int columns,
                            const int32_t* params, uint8_t* out_dev, int* status, void* stream);
int lumina_ocr_fax_decode(lumina_ocr_t* h, const uint8_t* const* streams, const size_t* sizes, int n, int rows, int columns,
                          const int32_t* params, uint8_t* out_dev, int* status, void* stream);

/* JBIG2 (ITU-T T.88) page and mask streams of scanned PDFs, generic-region subset: PDF's /JBIG2Decode in the embedded organisation
 * (no file header; the segments of the optional /JBIG2Globals stream come first).  The contract follows lumina_ocr_fax_decode and
 * lumina_ocr_jp2_probe.
 * Read: page information (type 48), immediate generic regions (38, 39) coded arithmetically with templates 0-3, adaptive template
 * pixels anywhere T.88 allows (y in -128..0, x in -128..127, before the current pixel) and typical prediction, or coded as MMR (T.6
 * lines, 1 = black, EOFB optional); end of stripe (50: with a page height of 0xFFFFFFFF the height is the last stripe's y + 1), end of
 * page (49) and end of file (51), which end the reading; profiles (52) and extensions (62) are skipped.  Regions are combined onto
 * the page in segment order, each with its operator (OR, AND, XOR, XNOR, REPLACE), clipped to the page, over the default pixel.
 * -2 (valid, outside the subset), each with its reason: symbol dictionaries (0), text regions (4, 6, 7), pattern dictionaries (16),
 * halftone regions (20, 22, 23), intermediate generic regions (36), refinement regions (40, 42, 43), code tables (53), a data length
 * of 0xFFFFFFFF, EXTTEMPLATE, a region or page wider than 8192, more than 256 regions, a page association other than 0 or 1, a
 * second page information segment, a stream of 2^28 bytes or more.  -1: a header or length past the stream, a region before the page
 * information, a region that does not meet the page, an operator other than the page's where the page forbids overriding, reserved
 * flag bits, an adaptive pixel that is not before the current pixel, a type T.88 does not define, an unknown height without an end of
 * stripe, no page information, an MMR region the fax decoder refuses (lumina_ocr_ccitt_decode's list).
 * The segment syntax is written from recollection of T.88 and pinned to the project's own test encoder; no other JBIG2 coder was at
 * hand (README).  The arithmetic coder is pinned to the standard's test sequence (H.2), the MMR path to libtiff.
 * lumina_ocr_jbig2_probe (host only, no handle): the segments; no pixel is decoded (so an MMR region's -1 shows only in the decode).
 * globals may be null.  info = {width, height, regions, arithmetic regions, MMR regions, highest template, TPGDON anywhere, striped},
 * filled as far as the segments were read.  Returns 0, -1 or -2.
 * lumina_ocr_jbig2_reason: the reason behind the last non-zero lumina_ocr_jbig2_probe result of the calling thread when `code` is
 * that result (a static string, for logs); otherwise the general meaning of `code`.
 * lumina_ocr_jbig2_decode: streams / sizes and globals / globals_sizes are HOST arrays of n entries (globals, or any entry of it, may
 * be null), every page height x width; params int32 [n][1] = {invert}; out_dev uint8 [n][height][width][3] with bit 1 -> 0 (black)
 * and bit 0 -> 255, PDF's rule for /JBIG2Decode, swapped by invert (/Decode [1 0]); status HOST int [n]: 0 ok, -1, -2, -4 another
 * size.  A page with a non-zero status is not written.  n == 0 does nothing.  Synchronises `stream`. */
int lumina_ocr_jbig2_probe(const uint8_t* stream, size_t size, const uint8_t* globals, size_t globals_size, int info[8]);
const char* lumina_ocr_jbig2_reason(int code);
int lumina_ocr_jbig2_decode(lumina_ocr_t* h, const uint8_t* const* streams, const size_t* sizes, const uint8_t* const* globals,
                            const size_t* globals_sizes, int n, int height, int width, const int32_t* params, uint8_t* out_dev, int* status,
                            void* stream);

/* Strip-coded page images — the strips of a scanned TIFF page (utils/tiff_pages.py finds them) and PDF's /LZWDecode and
 * /RunLengthDecode image streams (one strip a page).  The batch contract is lumina_ocr_flate_image_decode's: HOST pointers, n pages of
 * one size, out_dev uint8 [n][height][width][3], a HOST status per page (0: exact pixels, the bytes of Pillow's
 * Image.open(f).convert('RGB'); any other status: the page is left to Pillow, its pixels are undefined), `stream` synchronised.
 * strips / sizes: m strips, those of page 0 first, each page's consecutive and in row order; strip k of a page covers rows
 * [k * rows_per_strip, min(height, (k + 1) * rows_per_strip)) as whole packed rows.  strip_counts int32 [n] must each equal
 * ceil(height / rows_per_strip) (else that page is -2) and add up to m (else the call fails).  params int32 [n][7] = {codec (1 none,
 * 5 LZW: MSB-first codes of 9..12 bits with early change, 256 Clear, 257 EOI; 32773 PackBits), predictor (1; 2: horizontal differencing,
 * 8-bit samples), components (1 | 3), bits per component (8; 1 / 2 / 4 with one component), indexed (0 | 1), invert (0 | 1: MinIsWhite
 * or /Decode [1 0], one non-indexed component), rle_eod (0 | 1: a PackBits header byte of 128 ends the data as in /RunLengthDecode;
 * 0 skips it as TIFF does)}; palettes as for lumina_ocr_flate_image_decode.  A page's status is the lowest of its strips':
 * 0 exactly when the strip produced its rows x row bytes (codes or bytes after that are ignored, no EOI is needed);
 * -1: an LZW code above the next free entry, a code >= 258 right after Clear, a full table followed by anything but Clear, EOI or the end
 * of the data before the strip is full, a PackBits literal or repeat that runs past the input, fewer raw bytes than the strip's rows;
 * -2: a combination outside this list, or an LZW strip whose first code is not Clear (old-style LSB-first LZW among them).
 * Output is clipped at the strip's end; a hostile stream ends in -1 after at most one step per 9 bits (LZW) or per byte (PackBits). */
int lumina_ocr_strip_image_decode(lumina_ocr_t* h, const uint8_t* const* strips, const size_t* sizes, int m, const int32_t* strip_counts, int n,
                                  int height, int width, int rows_per_strip, const int32_t* params, const uint8_t* const* palettes,
                                  uint8_t* out_dev, int* status, void* stream);

int lumina_ocr_jpeg_coefficients(lumina_ocr_t* h, const uint8_t* pages_dev, int n, int height, int width, int quality, int16_t* coefs_dev,
                                 void* stream);

/* ---- kernel-level entry points (parity tests, benchmarks) ---- */
/* Generic NHWC bf16 convolution through the MFMA implicit-GEMM kernel.  w_host: OHWI bf16 bits
 * [cout][ks][ks][cin], bias_host float [cout]; ks/stride in {1/1, 2/2, 3/1, 3/2}; cin % 16 == 0,
 * cout % 8 == 0; act: 0 none, 1 relu, 2 hswish, 3 hsigmoid, 4 sigmoid; res_dev optional [N,Ho,Wo,cout].
 * Synchronous (packs and uploads the weights, runs, waits). */
int lumina_ocr_conv2d(lumina_ocr_t* h, const uint16_t* x_dev, int n, int height, int width, int cin, const uint16_t* w_host,
                      const float* bias_host, int cout, int ks, int stride, int act, const uint16_t* res_dev, uint16_t* y_dev,
                      void* stream);
/* Copy an intermediate activation of the last det/rec forward (option keep_taps=1) to host memory.
 * dims receives n,h,w,c; returns non-zero when the tap is unknown or the buffer too small. */
int lumina_ocr_read_tap(lumina_ocr_t* h, const char* name, uint16_t* out_host, size_t capacity_elems, int dims[4]);
/* Sum of conv-kernel device time (ms) and algorithmic FLOPs since the last call (option time_convs=1). */
int lumina_ocr_conv_timing(lumina_ocr_t* h, double* total_ms, double* total_flops, int* launches);
/* Same, per launch, as text lines "name kernel ms gflop\n" written into buf (truncated to cap). Clears the records. */
int lumina_ocr_conv_timing_detail(lumina_ocr_t* h, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
