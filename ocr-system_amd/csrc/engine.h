// Host-side engine: weight loading/packing, workspace, and the det / rec layer schedules.
#pragma once
#include <map>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "blob_check.h"
#include "common.h"
#include "conv_mfma.h"
#include "mbconv.h"
#include "svtr.h"

struct Tensor4 {
    bf16_t* p = nullptr;
    int n = 0, h = 0, w = 0, c = 0;
    bool blk = false;  // channel-blocked layout [n][c/16][h][w][16] instead of NHWC (conv_mfma.h: ConvParams::x_blk)
    // virtual concat (ConvParams::n_src): the c channels are n_src tensors, source k at 1 / 2^shift[k] resolution contributing xs_c[k]
    // channels (0: c / n_src) out of pixels xs_cs[k] channels wide (0: xs_c[k])
    int n_src = 0; const bf16_t* xs[4] = {nullptr, nullptr, nullptr, nullptr}; int xs_shift[4] = {0, 0, 0, 0};
    int xs_c[4] = {0, 0, 0, 0}, xs_cs[4] = {0, 0, 0, 0};
    int src_c(int k) const { return xs_c[k] ? xs_c[k] : c / n_src; }
    int src_cs(int k) const { return xs_cs[k] ? xs_cs[k] : src_c(k); }
    size_t elems() const { return (size_t)n * h * w * c; }
};

struct ConvLayer {
    std::string name;
    int ks = 1, stride = 1, cin = 0, cout = 0;  // padded gemm dims
    int act = ACT_NONE;
    bool convt = false;
    int convt_c = 0;
    ConvKernelCfg cfg{};
    bf16_t* wpk = nullptr;  // device
    // second packing for the 16x32-tile / 4x2-register-tile kernel (3x3, stride 1, >= 64 input channels): picked per launch
    // when the grid is large enough to fill the chip with the bigger tiles
    ConvKernelCfg cfg_big{}; bf16_t* wpk_big = nullptr;
    bf16_t* fuse_w = nullptr; float fuse_b = 0.f;  // optional fused DBHead tail (see ConvParams)
    double alg_flop_per_px = 0;   // > 0: algorithmic FLOP per output pixel of the architecture's layers this launch replaces (a composed layer executes more)
    float* bias = nullptr;  // device, n_tiles*BN
};

struct DwLayer { int k = 3, c = 0; bf16_t* w = nullptr; float* bias = nullptr; };
struct SeLayer { int c = 0, mid = 0; bf16_t *w1 = nullptr, *w2 = nullptr; float *b1 = nullptr, *b2 = nullptr; };

struct RecBlock {
    int k, cin, exp, cout, se_mid, stride_h, act;
    bool se, res;
    ConvLayer expand, project;
    DwLayer dw;
    bf16_t* we_pk = nullptr; float* be_pk = nullptr;  // expand weights / bias in the fused expand+depthwise kernel's layout (mbconv.h)
    SeLayer sel;
};

// SVTR recogniser (arch.svtr_block_table; Tiny or Base: the dimensions travel in the blob's svtr.config tensor).  Every linear layer
// and every convolution is one svtr_gemm launch (svtr.h); proj / fc2 / the merging convs carry the LayerNorm that follows them.
struct SvtrLinear {
    int K = 0, N = 0, taps = 1, cin = 0, act = ACT_NONE;
    uint16_t* w = nullptr;   // device, [N][K] in the model's storage type
    float* bias = nullptr;
    float *gamma = nullptr, *beta = nullptr;   // LayerNorm fused into the epilogue (or null)
};
struct SvtrBlock { int dim = 0, heads = 0, gh = 0, gw = 0; bool local = false; SvtrLinear qkv, proj, fc1, fc2; };
struct SvtrModel {
    bool loaded = false;
    int dtype = 0;            // storage / MFMA type: 0 bf16, 1 fp16
    int dims[3] = {64, 128, 256}, depths[3] = {3, 6, 3}, heads[3] = {2, 4, 8}, local_blocks = 6, out_ch = 192;
    int num_classes = 0, ctc_ntiles = 0;
    SvtrLinear pe1, pe2, sub[2], last;
    uint16_t* pos = nullptr;  // [640][dims[0]]
    std::vector<SvtrBlock> blocks;
    bf16_t* ctc_wpk = nullptr; float* ctc_bias = nullptr;
};

// Owning handles (move-only, released by the destructor): the only places device memory, pinned host memory and events are freed
struct DeviceFree { void operator()(void* p) const { (void)hipFree(p); } };
struct PinnedFree { void operator()(void* p) const { (void)hipHostFree(p); } };
struct EventDestroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
using DeviceMem = std::unique_ptr<void, DeviceFree>;
using PinnedMem = std::unique_ptr<void, PinnedFree>;
using Event = std::unique_ptr<std::remove_pointer<hipEvent_t>::type, EventDestroy>;
inline hipError_t mem_alloc(DeviceMem* m, size_t bytes) { void* p = nullptr; hipError_t e = hipMalloc(&p, bytes); m->reset(p); return e; }
inline hipError_t mem_alloc(PinnedMem* m, size_t bytes) { void* p = nullptr; hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault); m->reset(p); return e; }

// A buffer that grows on demand and never shrinks (contents are not kept).  The old buffer is freed only once the GPU is done with it:
// after `in_use` (the work that reads it), or, without one, after the whole device has drained.
template <class Mem> struct Growable {
    Mem mem;
    size_t cap = 0;
    uint8_t* get() const { return static_cast<uint8_t*>(mem.get()); }
    hipError_t reserve(size_t bytes, hipEvent_t in_use = nullptr) {
        if (bytes <= cap) return hipSuccess;
        hipError_t e = in_use ? hipEventSynchronize(in_use) : hipDeviceSynchronize();
        if (e != hipSuccess) return e;
        mem.reset(); cap = 0;
        if ((e = mem_alloc(&mem, bytes)) != hipSuccess) return e;
        cap = bytes;
        return hipSuccess;
    }
};

// one timed launch (option time_convs): HIP events around it on its stream, its algorithmic work, and what ran
struct LaunchRecord { Event e0, e1; double flop, bytes; std::string layer, kernel; };

struct lumina_ocr {
    int device = 0;
    std::string err;
    // ---- det ----
    bool det_loaded = false;
    std::map<std::string, ConvLayer> det;
    bf16_t* stem_wpk = nullptr; float* stem_bias = nullptr;
    // ---- rec ----
    bool rec_loaded = false;
    int num_classes = 0, ctc_ntiles = 0;
    bf16_t* rstem_wpk = nullptr; float* rstem_bias = nullptr;
    std::vector<RecBlock> rblocks;
    ConvLayer rconv2, xproj[2];
    bf16_t* whh[2] = {nullptr, nullptr};
    bf16_t *xproj_spk[2] = {nullptr, nullptr}, *rconv2_spk = nullptr;  // the same weights in seq_gemm's tile order (bias: the layers' own)
    bf16_t* ctc_wpk = nullptr; float* ctc_bias = nullptr;
    SvtrModel svtr;
    // ---- orientation classifier (PP-OCR cls: MobileNetV3-small x0.35 on 48 x 192 crops, FC 200 -> 2) ----
    bool cls_loaded = false;
    bf16_t* cstem_wpk = nullptr; float* cstem_bias = nullptr;
    std::vector<RecBlock> cblocks;
    ConvLayer cconv2;
    float *cls_fc_w = nullptr, *cls_fc_b = nullptr;   // fp32 [2][200], [2]
    // ---- workspace ----
    Growable<DeviceMem> ws;
    Arena arena;  // carves ws for the forward in progress (null base: its dry run, which sizes ws)
    std::vector<DeviceMem> owned;  // weights and tables, freed at destroy
    bf16_t* zeros = nullptr;  // 256 B of zeros (out-of-image halo source of the LDS-DMA conv); zero_block() uploads it at first use
    int det_sub_batch = 16, rec_sub_batch = 4096, cls_sub_batch = 4096, post_group = 64;
    int tail_group = 16;   // pages per pass of the detector's 1/4-resolution tail (lateral in2 -> p2 -> head) inside one det forward
    std::map<std::string, Tensor4> taps;  // last forward's intermediates (debug / parity tests)
    int keep_taps = 0;   // 1: every intermediate (switches the fusions that would skip one off); 2: fusions stay on, tap what still exists
    bool fuse_head = true;  // head.convt3 fused into head.convt2's epilogue
    bool fuse_pool = true;  // stem.conv3's epilogue does the 3x3/s2 max pool
    int conv_big_min = 1024;  // 16x32-tile kernels once a full sub-batch gives at least this many work-groups
    bool blocked_layout = true;   // stage-0 activations between ring-kernel layers in channel-blocked layout (bit-identical)
    bool conv_ring = true;  // persistent ring kernel for the 3x3 / stride-1 layers (conv_ring.hip)
    int svtr_f16 = -1;      // storage type of the next SVTR load: -1 = what the blob's svtr.config says, 0 bf16, 1 fp16
    int conv2d_variant = 0; // lumina_ocr_conv2d passes it as ConvCall::variant (tests)
    int ring_orient = -1;   // its tile orientation: -1 auto, 0 / 1 forced (tests)
    bool fuse_short = true;   // stages 1-3: the block entry's 2x2 / stride-2 shortcut conv computed by its 3x3 / stride-2 conv0 kernel (one read of the input)
    bool fpn_compose = true;  // the lateral fpn.in2 composed into fpn.p2 (the 256-channel 1/4-resolution lateral is never computed); needs fpn_multi
    bool fpn_multi = true;  // head.conv1 reads p5 / p4 / p3 / p2 at their own resolution (ring kernel): the FPN concat is never written
    bool fuse_stem = true;  // stem.conv1 + stem.conv2 in one kernel (the first 32-channel tensor stays in LDS)
    bool fuse_mb = true;    // recogniser blocks: expand + depthwise in one kernel (the expanded tensor stays in LDS)
    bool fuse_xproj = true;       // LSTM x-projections on the A-stationary streaming GEMM (seq_gemm.h)
    bool fuse_conv2_pool = true;  // rec.conv2 + rec.pool in one seq_gemm launch (the [N,2,160,288] tensor is never written)
    int lstm_waves = 12;          // waves per work-group of the LSTM recurrence: 12, or 3 (the earlier kernel)
    // seq_gemm only once a sub-batch gives at least this many of its 128-row work-groups (as conv_big_min): a work-group walks all
    // column tiles one after the other, so row tiles are its only parallelism, and with few of them the tile-parallel kernels, which
    // spread 5 to 12 times as many work-groups over the chip, are faster (measured, both x-projections: 29 to 39 us against 44 to 47 at 4 to 82
    // work-groups, 62 against 49 us at 163)
    int seq_gemm_min = 128;
    // per-kernel event timing (bench roofline): the launches of the last det forward
    bool time_convs = false;
    std::vector<LaunchRecord> launches;
    // ---- pre-processing (resize / enhance) ----
    struct Coeffs { int ksize = 0; int* bounds = nullptr; int* kk = nullptr; std::shared_ptr<std::vector<int>> bounds_host; };
    std::map<std::pair<int, int>, Coeffs> coeff_cache;  // (in, out) -> device tables
    Growable<DeviceMem> aux;   // resize intermediate
    Growable<DeviceMem> sums;  // enhance: per-page grey sums
    int jd_last_passes = 0;   // synchronisation passes the last JPEG decode needed (incl. the one that found nothing to change)
    // pinned staging buffers of the JPEG decoder (jpegdec.hip), used in turn; `uploaded` is recorded after the uploads that read one
    struct Staging { Growable<PinnedMem> buf; Event uploaded; };
    Staging jd_stage[2];
    int jd_stage_next = 0;
    Staging pd_stage;   // pinned staging of the PNG decoder's gathered IDAT payloads (pngdec.hip)
    int pd_sub_batch_mb = 768;   // PNG decoder: filtered-scanline MB per sub-batch (64 A4 RGB pages at 300 dpi are 1.7 GB); sizes its workspace
    Staging jp_stage;   // pinned staging of the JPEG 2000 decoder's block records and coded bytes (jp2dec.hip)
    Staging wp_stage;   // pinned staging of the WebP decoder's gathered VP8L payloads (webpdec.hip)
    int wp_sub_batch_mb = 2048;   // WebP decoder: MB of planes and code tables per sub-batch (an A4 page at 200 dpi takes 69 MB, 37 of them tables)
    int jp_sub_batch_mb = 4096;   // JPEG 2000 decoder: MB of coefficient planes per sub-batch (an A4 RGB page at 200 dpi takes 93 MB)
    float* dk_trig = nullptr; short* dk_wtab = nullptr;   // de-skew tables (deskew.h), uploaded at first use
    Staging pc_stage;               // pinned copy of the page-composition layer table (compose.hip) ...
    Growable<DeviceMem> pc_table;   // ... and its device copy; `uploaded` is recorded after the kernel that reads it
};

int locr_fail(lumina_ocr* eng, const char* what, const char* detail);

int eng_load_det(lumina_ocr* eng, const void* blob, size_t n);
int eng_load_rec(lumina_ocr* eng, const void* blob, size_t n);
int eng_det_forward(lumina_ocr* eng, const uint8_t* pages, int B, int H, int W, int Hp, int Wp, bf16_t* prob, hipStream_t st);
int eng_rec_forward(lumina_ocr* eng, const uint8_t* crops, const int* widths, int N, int* idx, float* prob, hipStream_t st);
int eng_load_svtr(lumina_ocr* eng, const void* blob, size_t n);
int eng_load_cls(lumina_ocr* eng, const void* blob, size_t n);
int eng_cls_forward(lumina_ocr* eng, const uint8_t* crops, const int* widths, int N, float thresh, int* label, float* score, int* flip, hipStream_t st);
int eng_svtr_forward(lumina_ocr* eng, const uint8_t* crops, const int* widths, int N, int* idx, float* prob, hipStream_t st);
int eng_ws_reserve(lumina_ocr* eng, size_t bytes);
// a device copy of host data, owned by the engine until destroy (nullptr if the allocation or the copy fails)
void* eng_upload(lumina_ocr* eng, const void* host, size_t bytes);
// What an eng_run_conv call asks for beyond y = act(conv(L, x) + bias); a call site names only what differs from the defaults.
struct ConvCall {
    const Tensor4* res = nullptr; int res_shift = 0;   // residual / top-down tensor, read at (oy >> res_shift, ox >> res_shift)
    int out_mode = OUT_NORMAL, up_shift = 0;           // ConvOutMode; OUT_UPSAMPLE replicates every pixel (1 << up_shift)^2 times
    int y_cstride = 0, y_coff = 0;                     // y is the channel slice [y_coff, y_coff + cout) of pixels y_cstride wide (0: y->c)
    bool flat = false;                                 // 1x1 conv as one GEMM over all pixels of the batch
    const bf16_t* gate = nullptr;                      // squeeze-excite gate [n][cin] multiplied into the input (ConvParams::gate)
    const ConvLayer* short_l = nullptr; Tensor4* short_y = nullptr;   // the block's shortcut layer and its output, computed by the same launch (ConvParams::wpk2)
    int variant = 0;   // lumina_ocr_conv2d: 0 = the layer's own choice, 1 = LDS-DMA 16x32 tile and never the ring, 2 = ring kernel or an error
    ConvCall& residual(const Tensor4* r, int shift = 0) { res = r; res_shift = shift; return *this; }
    ConvCall& mode(int m) { out_mode = m; return *this; }
    ConvCall& upsample(int shift) { out_mode = OUT_UPSAMPLE; up_shift = shift; return *this; }
    ConvCall& channel_slice(int cstride, int coff) { y_cstride = cstride; y_coff = coff; return *this; }
    ConvCall& flat_gemm(bool on = true) { flat = on; return *this; }
    ConvCall& gated(const bf16_t* g) { gate = g; return *this; }
    ConvCall& shortcut(const ConvLayer* l, Tensor4* y) { short_l = l; short_y = y; return *this; }
};
int eng_run_conv(lumina_ocr* eng, const ConvLayer& L, const Tensor4& x, Tensor4* y, hipStream_t st, const ConvCall& c = {});
