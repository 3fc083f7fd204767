// Engine: LOCW weight-blob parsing + packing, device workspace, det (DBNet-R18vd) and rec
// (CRNN-MobileNetV3) layer schedules.  Layer names/shapes mirror lumina_ocr/arch.py.
#include "engine.h"

#include <cstdlib>
#include <cstring>

#include "ops.h"
#include "seq_gemm.h"
#include "stem_conv.h"

int locr_fail(lumina_ocr* eng, const char* what, const char* detail) {
    if (eng) eng->err = std::string(what) + ": " + (detail ? detail : "");
    return 1;
}

#define RUN(expr) do { if ((expr) != 0) return 1; } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize is per device: remember (device, kernel) pairs, not kernels
#include <mutex>
#include <set>
hipError_t locr_dyn_lds(const void* kernel, int bytes) {
    static std::mutex mu;
    static std::set<std::pair<int, const void*>> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(mu);
    if (done.count({dev, kernel})) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.insert({dev, kernel});
    return e;
}

// ------------------------------------------------------------------------------ blob
// What every eng_load_* does first (blob_check.h): parse, then check every tensor the loader will read.  On a refusal the engine is
// untouched: the error names the reason and the tensor, and the model loaded before stays as it was.  `storage` keeps the aligned copy
// of a blob that came at an address the loaders cannot read arrays from in place.
static bool checked_blob(lumina_ocr* eng, const char* what, BlobKind kind, const void* blob, size_t n, std::vector<uint64_t>* storage, BlobMap* m) {
    BlobError e;
    if (blob == nullptr) { locr_fail(eng, what, "null blob"); return false; }
    blob = blob_realign(blob, n, storage);
    if (!blob_parse(blob, n, m, &e) || !check_blob(kind, *m, &e)) {
        locr_fail(eng, what, (e.reason + (e.tensor.empty() ? "" : " (tensor " + e.tensor + ")")).c_str());
        return false;
    }
    return true;
}

// ------------------------------------------------------------------------------ memory
void* eng_upload(lumina_ocr* eng, const void* host, size_t bytes) {
    DeviceMem d;
    if (mem_alloc(&d, bytes ? bytes : 16) != hipSuccess) return nullptr;
    if (bytes && hipMemcpy(d.get(), host, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    eng->owned.push_back(std::move(d));
    return eng->owned.back().get();
}

int eng_ws_reserve(lumina_ocr* eng, size_t bytes) {
    LOCR_CHECK(eng->ws.reserve(bytes));
    return 0;
}

// the forward in progress takes its tensors from eng->arena: null pointers in its dry run (and past the reservation: see ws_null)
static Tensor4 ws_tensor(lumina_ocr* eng, int n, int h, int w, int c) {
    Tensor4 t; t.n = n; t.h = h; t.w = w; t.c = c;
    t.p = eng->arena.take<bf16_t>(t.elems());
    return t;
}

// a launch site found a null workspace pointer: the dry run (0), or a carve past the reservation, which is an error and never a dry run
static int ws_null(lumina_ocr* eng, const char* what) {
    return eng->arena.overflow ? locr_fail(eng, what, "workspace layout exceeds the reservation") : 0;
}

// 256 B of zeros, uploaded at first use (nullptr if that fails)
static const bf16_t* zero_block(lumina_ocr* eng) {
    if (eng->zeros == nullptr) {
        const uint32_t z[64] = {0};
        eng->zeros = static_cast<bf16_t*>(eng_upload(eng, z, sizeof(z)));
    }
    return eng->zeros;
}

static inline int rup(int v, int m) { return (v + m - 1) / m * m; }
constexpr int CLS_H = 48, CLS_W = 192;   // classifier crop (arch.CLS_*; CLS_FEAT, conv2's channels: blob_check.h)

// ------------------------------------------------------------------------------ layer construction
static bool get_wb(lumina_ocr* eng, const std::map<std::string, HostBlobTensor>& m, const std::string& name,
                   const HostBlobTensor** w, const HostBlobTensor** b) {
    auto iw = m.find(name + ".w"), ib = m.find(name + ".b");
    if (iw == m.end() || ib == m.end() || iw->second.dtype != 1 || ib->second.dtype != 0) {
        locr_fail(eng, "missing/ill-typed tensor", name.c_str());
        return false;
    }
    *w = &iw->second; *b = &ib->second;
    return true;
}

// Build a conv layer from blob tensor name.w [cout_r][ks][ks][cin_r] (bf16) / name.b [cout_r or bias_r] (f32).
static bool make_conv(lumina_ocr* eng, const std::map<std::string, HostBlobTensor>& m, const std::string& name, int ks, int stride,
                      int cin_r, int cout_r, int cin_p, int cout_p, int act, ConvLayer* L, int bias_repeat = 1) {
    const HostBlobTensor *w, *b;
    if (!get_wb(eng, m, name, &w, &b)) return false;
    if (w->dims.size() != 4 || w->dims[0] != cout_r || w->dims[1] != ks || w->dims[3] != cin_r ||
        (int)b->dims[0] * bias_repeat != cout_r) {
        locr_fail(eng, "unexpected tensor shape", name.c_str());
        return false;
    }
    L->name = name; L->ks = ks; L->stride = stride; L->cin = cin_p; L->cout = cout_p; L->act = act;
    if (!conv_pick_cfg(ks, stride, cin_p, cout_p, &L->cfg)) { locr_fail(eng, "no conv kernel config", name.c_str()); return false; }
    const int taps = ks * ks;
    std::vector<bf16_t> padded((size_t)cout_p * taps * cin_p, 0);
    const bf16_t* src = reinterpret_cast<const bf16_t*>(w->data);
    for (int co = 0; co < cout_r; ++co)
        for (int t = 0; t < taps; ++t)
            memcpy(&padded[((size_t)co * taps + t) * cin_p], &src[((size_t)co * taps + t) * cin_r], sizeof(bf16_t) * cin_r);
    std::vector<bf16_t> packed(conv_packed_weight_elems(cout_p, ks, cin_p, L->cfg.bn));
    pack_conv_weights(padded.data(), cout_p, ks, cin_p, L->cfg.bn, L->cfg.ck, packed.data());
    L->wpk = static_cast<bf16_t*>(eng_upload(eng, packed.data(), packed.size() * sizeof(bf16_t)));
    // 16x32-tile kernel: operands by LDS-DMA into a 2-deep ring (nw == 6, default: +3..5 % on the 128..256-channel layers) or
    // through registers (nw == 5, LUMINA_CONV_DMA=0)
    static const int dma = getenv("LUMINA_CONV_DMA") != nullptr ? atoi(getenv("LUMINA_CONV_DMA")) : 1;
    if (ks == 3 && stride == 1 && L->cfg.bn == 64 && (cin_p >= 64 || name == "stem.conv3") && L->cfg.nw == 4) {  // stem.conv3: for the fused max pool
        L->cfg_big = L->cfg; L->cfg_big.nw = dma ? 6 : 5; L->cfg_big.ck = 16;
        std::vector<bf16_t> packed2(conv_packed_weight_elems(cout_p, ks, cin_p, 64));
        pack_conv_weights(padded.data(), cout_p, ks, cin_p, 64, 16, packed2.data(), dma ? 1 : 0);
        L->wpk_big = static_cast<bf16_t*>(eng_upload(eng, packed2.data(), packed2.size() * sizeof(bf16_t)));
    }
    const int ntiles = (cout_p + L->cfg.bn - 1) / L->cfg.bn;
    std::vector<float> bias((size_t)ntiles * L->cfg.bn, 0.f);
    const float* bs = reinterpret_cast<const float*>(b->data);
    const int bn_r = b->dims[0];
    for (int i = 0; i < cout_r; ++i) bias[i] = bs[i % bn_r];
    L->bias = static_cast<float*>(eng_upload(eng, bias.data(), bias.size() * sizeof(float)));
    if (!L->wpk || !L->bias) { locr_fail(eng, "device upload failed", name.c_str()); return false; }
    return true;
}

static inline float host_bf16_to_f32(bf16_t b) { uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f; }
static inline bf16_t host_f32_to_bf16(float f) {   // round to nearest even (finite inputs)
    uint32_t u; memcpy(&u, &f, 4);
    return (bf16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

static inline uint16_t bf16_bits_to(uint16_t b, int dtype) {   // bf16 bits -> the model's storage type (fp16: exact for |w| >= 2^-14)
    if (!dtype) return b;
    uint32_t u = (uint32_t)b << 16;
    float f; memcpy(&f, &u, 4);
    const _Float16 hv = (_Float16)f;
    uint16_t o; memcpy(&o, &hv, 2);
    return o;
}

// The 3-channel stem conv name.w [cout][3][3][3] / name.b [cout] (cout <= 32) of the detector, the recogniser or the classifier, in the
// dedicated kernel's layout (stem_conv.h)
static int load_stem(lumina_ocr* eng, const std::map<std::string, HostBlobTensor>& m, const char* name, int cout, bf16_t** wpk, float** bias) {
    const HostBlobTensor *w, *b;
    if (!get_wb(eng, m, name, &w, &b)) return 1;
    if (w->dims.size() != 4 || w->dims[0] != cout || w->dims[1] != 3 || w->dims[2] != 3 || w->dims[3] != 3 || b->dims[0] != cout)
        return locr_fail(eng, name, "shape");
    bf16_t packed[2 * 2 * 32 * 8];
    pack_stem_weights(reinterpret_cast<const bf16_t*>(w->data), cout, packed);
    float padded[32] = {0};
    memcpy(padded, b->data, sizeof(float) * cout);
    *wpk = static_cast<bf16_t*>(eng_upload(eng, packed, sizeof(packed)));
    *bias = static_cast<float*>(eng_upload(eng, padded, sizeof(padded)));
    return *wpk && *bias ? 0 : locr_fail(eng, "upload", name);
}

// The CTC head name.w [classes][K] (bf16, stored as `dtype`) / name.b [classes] of the CRNN or of SVTR, in ctc_fc_argmax's layout; the
// bias of the padding classes is -1e30
static int load_ctc_head(lumina_ocr* eng, const std::map<std::string, HostBlobTensor>& m, const char* name, int K, int dtype, int* num_classes,
                         int* ntiles, bf16_t** wpk, float** bias) {
    auto w = m.find(std::string(name) + ".w"), b = m.find(std::string(name) + ".b");
    if (w == m.end() || b == m.end() || w->second.dims.size() != 2 || w->second.dims[1] != K || b->second.dims[0] != w->second.dims[0])
        return locr_fail(eng, name, "missing/shape");
    const int C = w->second.dims[0];
    *num_classes = C; *ntiles = (C + 63) / 64;
    std::vector<bf16_t> conv((size_t)C * K), packed(ctc_packed_weight_elems(C, K));
    const bf16_t* src = reinterpret_cast<const bf16_t*>(w->second.data);
    for (size_t i = 0; i < conv.size(); ++i) conv[i] = bf16_bits_to(src[i], dtype);
    pack_ctc_weights(conv.data(), C, K, packed.data());
    std::vector<float> padded((size_t)*ntiles * 64, -1.0e30f);
    memcpy(padded.data(), b->second.data, sizeof(float) * C);
    *wpk = static_cast<bf16_t*>(eng_upload(eng, packed.data(), packed.size() * sizeof(bf16_t)));
    *bias = static_cast<float*>(eng_upload(eng, padded.data(), padded.size() * sizeof(float)));
    return *wpk && *bias ? 0 : locr_fail(eng, "upload", name);
}

// The lateral fpn.in2 (1x1, 64 -> 256, no bias in DBFPN) composed into the smoothing conv fpn.p2 (3x3, 256 -> 64):
//     p2 = conv3x3(W_p2, W_in2 c2 + up2(out3)) = conv3x3(W_c, c2) + conv3x3(W_p2, up2(out3)),   W_c[co][tap][ci] = sum_m W_p2[co][tap][m] W_in2[m][ci]
// -> layer "fpn.p2c": ONE 3x3 conv over the 320 channels [c2 (64, full resolution) | out3 (256, half resolution, read nearest-upsampled)];
// the 256-channel 1/4-resolution lateral (1.5 GB per 16 A4 pages, written by one kernel and read back by the next) never exists.
// W_c is formed in fp64 in m order, rounded to fp32 and then to bf16 (oracle/nets.py compose_fpn_p2 does the same, bit for bit); the
// lateral sum is no longer rounded to bf16 on its way.  Exact with zero padding only for a lateral without bias — which is what
// DBFPN has; a blob with a non-zero fpn.in2 bias keeps the two-kernel path.
static int compose_fpn_p2(lumina_ocr* eng, const std::map<std::string, HostBlobTensor>& m) {
    const HostBlobTensor *wi, *bi, *wp, *bp;
    if (!get_wb(eng, m, "fpn.in2", &wi, &bi) || !get_wb(eng, m, "fpn.p2", &wp, &bp)) return 1;
    const float* b_in2 = reinterpret_cast<const float*>(bi->data);
    for (int i = 0; i < 256; ++i)
        if (b_in2[i] != 0.f) return 0;   // (no "fpn.p2c" entry: det_forward_sub keeps in2 -> p2)
    const bf16_t* Wi = reinterpret_cast<const bf16_t*>(wi->data);   // [256][1][1][64]
    const bf16_t* Wp = reinterpret_cast<const bf16_t*>(wp->data);   // [64][3][3][256]
    std::vector<bf16_t> w((size_t)64 * 9 * 320);
    std::vector<double> win((size_t)256 * 64);
    for (size_t i = 0; i < win.size(); ++i) win[i] = (double)host_bf16_to_f32(Wi[i]);
    for (int co = 0; co < 64; ++co)
        for (int t = 0; t < 9; ++t) {
            double acc[64] = {0};
            const bf16_t* row = Wp + ((size_t)co * 9 + t) * 256;
            for (int mm = 0; mm < 256; ++mm) {
                const double a = (double)host_bf16_to_f32(row[mm]);
                for (int ci = 0; ci < 64; ++ci) acc[ci] += a * win[(size_t)mm * 64 + ci];
            }
            bf16_t* dst = &w[((size_t)co * 9 + t) * 320];
            for (int ci = 0; ci < 64; ++ci) dst[ci] = host_f32_to_bf16((float)acc[ci]);
            memcpy(dst + 64, row, 256 * sizeof(bf16_t));
        }
    std::map<std::string, HostBlobTensor> mm;
    mm["fpn.p2c.w"] = HostBlobTensor{1, {64, 3, 3, 320}, reinterpret_cast<const uint8_t*>(w.data()), w.size() * sizeof(bf16_t)};
    mm["fpn.p2c.b"] = *bp;
    ConvLayer& L = eng->det["fpn.p2c"];
    if (!make_conv(eng, mm, "fpn.p2c", 3, 1, 320, 64, 320, 64, ACT_NONE, &L)) return 1;
    L.alg_flop_per_px = 2.0 * 64 * 256 + 2.0 * 9 * 256 * 64;   // the architecture's fpn.in2 + fpn.p2 (the composed conv executes 2 * 9 * 320 * 64)
    return 0;
}

int eng_load_det(lumina_ocr* eng, const void* blob, size_t n) {
    BlobMap m;
    std::vector<uint64_t> aligned;
    if (!checked_blob(eng, "load_det_weights", BLOB_DET, blob, n, &aligned, &m)) return 1;
    LOCR_CHECK(hipSetDevice(eng->device));
    eng->det_loaded = false;   // from here on only an upload can fail; the detector then stays unloaded
    eng->det.clear();
    RUN(load_stem(eng, m, "stem.conv1", 32, &eng->stem_wpk, &eng->stem_bias));   // (Cin = 3: dedicated kernel)
    auto add = [&](const std::string& name, int ks, int stride, int cin, int cout, int act) -> bool {
        return make_conv(eng, m, name, ks, stride, cin, cout, cin, cout, act, &eng->det[name]);
    };
    if (!add("stem.conv2", 3, 1, 32, 32, ACT_RELU) || !add("stem.conv3", 3, 1, 32, 64, ACT_RELU)) return 1;
    const int chs[4] = {64, 128, 256, 512};
    int cin = 64;
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 2; ++j) {
            const std::string p = "s" + std::to_string(i) + ".b" + std::to_string(j);
            const int stride = (i > 0 && j == 0) ? 2 : 1;
            if (!add(p + ".conv0", 3, stride, cin, chs[i], ACT_RELU)) return 1;
            if (!add(p + ".conv1", 3, 1, chs[i], chs[i], ACT_RELU)) return 1;
            if (j == 0) {
                if (i == 0) { if (!add(p + ".short", 1, 1, cin, chs[i], ACT_NONE)) return 1; }
                else { if (!add(p + ".short", 2, 2, cin, chs[i], ACT_NONE)) return 1; }
            }
            cin = chs[i];
        }
    }
    for (int l = 5; l >= 2; --l) {
        if (!add("fpn.in" + std::to_string(l), 1, 1, chs[l - 2], 256, ACT_NONE)) return 1;
        if (!add("fpn.p" + std::to_string(l), 3, 1, 256, 64, ACT_NONE)) return 1;
    }
    if (!add("head.conv1", 3, 1, 256, 64, ACT_RELU)) return 1;
    if (compose_fpn_p2(eng, m)) return 1;
    {
        ConvLayer& L = eng->det["head.convt2"];
        if (!make_conv(eng, m, "head.convt2", 1, 1, 64, 256, 64, 256, ACT_RELU, &L, 4)) return 1;
        L.convt = true; L.convt_c = 64;
        ConvLayer& L3 = eng->det["head.convt3"];
        if (!make_conv(eng, m, "head.convt3", 1, 1, 64, 4, 64, 4, ACT_SIGMOID, &L3, 4)) return 1;
        L3.convt = true; L3.convt_c = 1;
        // fused tail: raw convt3 weights [4][64] + scalar bias live next to convt2
        const HostBlobTensor *w3, *b3;
        if (!get_wb(eng, m, "head.convt3", &w3, &b3)) return 1;
        ConvLayer& Lf = eng->det["head.convt2.fused"];
        Lf = L;
        Lf.name = "head.convt2+3";
        {   // MFMA A-operand image [kstep 4][half 2][row 32][8]: rows 0..3 = convt3 weights, the rest zero
            const bf16_t* w3s = reinterpret_cast<const bf16_t*>(w3->data);
            std::vector<bf16_t> img(4 * 2 * 32 * 8, 0);
            for (int ks = 0; ks < 4; ++ks)
                for (int hh = 0; hh < 2; ++hh)
                    for (int row = 0; row < 4; ++row)
                        for (int j = 0; j < 8; ++j) img[((ks * 2 + hh) * 32 + row) * 8 + j] = w3s[row * 64 + ks * 16 + hh * 8 + j];
            Lf.fuse_w = static_cast<bf16_t*>(eng_upload(eng, img.data(), img.size() * sizeof(bf16_t)));
        }
        Lf.fuse_b = reinterpret_cast<const float*>(b3->data)[0];
        if (!Lf.fuse_w) return locr_fail(eng, "upload", "head.convt3 fused weights");
    }
    eng->det_loaded = true;
    return 0;
}

// ------------------------------------------------------------------------------ conv dispatch
// does a 3x3 / stride-1 layer on an ho x wo map take the 16x32-tile (LDS-DMA / ring) kernels?  Depends on the layer geometry and the
// configured sub-batch only, never on the number of images in the call (the variants sum in different orders)
static bool conv_takes_big(const lumina_ocr* eng, const ConvLayer& L, int n, int ho, int wo, bool flat) {
    static const bool no_big = getenv("LUMINA_CONV_NO_BIG") != nullptr;
    static const long long big_min_env = getenv("LUMINA_CONV_BIG_MIN") ? atoll(getenv("LUMINA_CONV_BIG_MIN")) : -1;
    const long long nb_eff = n > eng->det_sub_batch ? n : eng->det_sub_batch;
    const long long big_blocks = nb_eff * ((ho + 15) / 16) * ((wo + 31) / 32) * ((L.cout + L.cfg.bn - 1) / L.cfg.bn);
    const long long big_min = big_min_env >= 0 ? big_min_env : eng->conv_big_min;
    return !no_big && !flat && L.wpk_big != nullptr && big_blocks >= big_min;
}

// option time_convs: HIP events on the launch stream around ONE launch (the detector's convolutions, and the recogniser paths' launches
// too: bench.py --config 3 / 5); flop / bytes are the launch's algorithmic work (operands and results once).  The events of a launch
// that fails go with the timer.
struct LaunchTimer {
    lumina_ocr* eng; hipStream_t st; Event e0, e1;
    LaunchTimer(lumina_ocr* e, hipStream_t s, bool enabled = true) : eng(e), st(s) {
        if (!enabled || !e->time_convs) return;
        hipEvent_t a = nullptr, b = nullptr;
        if (hipEventCreate(&a) == hipSuccess) e0.reset(a);
        if (hipEventCreate(&b) == hipSuccess) e1.reset(b);
        if (!e0 || !e1 || hipEventRecord(e0.get(), st) != hipSuccess) { e0.reset(); e1.reset(); }
    }
    bool on() const { return e1 != nullptr; }
    void done(std::string layer, std::string kernel, double flop, double bytes) {
        if (!on() || hipEventRecord(e1.get(), st) != hipSuccess) return;
        eng->launches.push_back(LaunchRecord{std::move(e0), std::move(e1), flop, bytes, std::move(layer), std::move(kernel)});
    }
};

// the call's geometry as the kernels want it (the weight image is the kernel choice's: conv_choose)
static int conv_params(lumina_ocr* eng, const ConvLayer& L, const Tensor4& x, const Tensor4& y, const ConvCall& c, ConvParams* out) {
    ConvParams p{};
    p.zeros = zero_block(eng);
    if (!p.zeros) return locr_fail(eng, "conv", "zero block upload failed");
    p.gate = c.gate; p.gate_hw = x.h * x.w;
    p.x = x.p; p.wpk = L.wpk; p.bias = L.bias; p.res = c.res ? c.res->p : nullptr; p.y = y.p;
    p.Cin = L.cin; p.Cout = L.cout; p.act = L.act;
    p.out_mode = c.out_mode; p.up_shift = c.up_shift; p.convt_c = L.convt_c;
    p.fuse_w = (c.out_mode == OUT_CONVT) ? L.fuse_w : nullptr; p.fuse_b = L.fuse_b;
    if (c.flat) {  // 1x1 conv == GEMM over all pixels: re-tile as rows of 32 so every 8x32 tile is full
        const long long m = (long long)x.n * x.h * x.w;
        p.N = 1; p.W = 32; p.H = (int)((m + 31) / 32); p.pix_limit = (int)m;
        p.Ho = p.H; p.Wo = 32;
        p.res_h = p.H; p.res_w = 32;
    } else {
        p.N = x.n; p.H = x.h; p.W = x.w; p.pix_limit = 0;
        p.Ho = (L.ks == 3) ? (x.h - 1) / L.stride + 1 : x.h / L.stride;
        p.Wo = (L.ks == 3) ? (x.w - 1) / L.stride + 1 : x.w / L.stride;
        if (c.res) { p.res_h = c.res->h; p.res_w = c.res->w; }
    }
    p.res_shift = c.res_shift;
    p.x_blk = x.blk; p.y_blk = y.blk; p.res_blk = c.res ? c.res->blk : 0;
    p.n_src = x.n_src;
    for (int k = 0; k < 4; ++k) {
        p.xs[k] = x.xs[k]; p.xs_shift[k] = x.xs_shift[k];
        p.xs_nchunk[k] = k < x.n_src ? x.src_c(k) / 16 : 0; p.xs_cstride[k] = k < x.n_src ? x.src_cs(k) : 0;
    }
    p.res_cstride = c.res ? c.res->c : 0;
    p.y_cstride = c.y_cstride ? c.y_cstride : y.c;
    p.y_coff = c.y_coff;
    if (const ConvLayer* s = c.short_l) {
        const Tensor4* sy = c.short_y;
        if (sy == nullptr || s->cin != L.cin || s->cout != L.cout || s->cfg.bn != L.cfg.bn || s->cfg.ck != L.cfg.ck || s->ks != 2 || s->stride != 2 ||
            sy->c != L.cout || sy->h != y.h || sy->w != y.w)
            return locr_fail(eng, "fused shortcut: layer mismatch", L.name.c_str());
        p.wpk2 = s->wpk; p.bias2 = s->bias; p.y2 = sy->p; p.y2_cstride = sy->c;
    }
    if (x.c != L.cin) return locr_fail(eng, "conv input channels mismatch", L.name.c_str());
    *out = p;
    return 0;
}

// which kernel runs the call, with which configuration and weight image
enum ConvKernel { CONV_TILE_8X32, CONV_TILE_16X32, CONV_POINTWISE, CONV_RING };
struct ConvChoice { ConvKernel kernel; ConvKernelCfg cfg; const bf16_t* wpk; };

static int conv_choose(lumina_ocr* eng, const ConvLayer& L, const ConvParams& p, const ConvCall& c, ConvChoice* out) {
    if (p.out_mode == OUT_POOL && (L.wpk_big == nullptr || L.cfg_big.nw != 6)) return locr_fail(eng, "fused max pool needs the LDS-DMA conv kernel", L.name.c_str());
    const bool forced = c.variant != 0 && L.wpk_big != nullptr;   // (the conv2d hook)
    // 16x32 tiles (less LDS and L2 traffic per MFMA) once they still give >= 2 workgroups per CU on all 256 CUs twice over
    const bool big = forced || p.out_mode == OUT_POOL || p.n_src > 1 || conv_takes_big(eng, L, p.N, p.Ho, p.Wo, c.flat);   // (a multi-source input is the ring kernel's)
    if (forced && c.variant == 2 && !conv_ring_supported(L.cfg_big, p)) return locr_fail(eng, "conv2d_variant 2: the ring kernel does not take this layer", L.name.c_str());
    *out = big ? ConvChoice{CONV_TILE_16X32, L.cfg_big, L.wpk_big} : ConvChoice{CONV_TILE_8X32, L.cfg, L.wpk};
    static const bool no_pw = getenv("LUMINA_CONV_NO_PW") != nullptr;
    const bool ring_on = c.variant == 0 ? eng->conv_ring : c.variant == 2;
    if (!no_pw && !big && conv_pw_supported(out->cfg, p)) out->kernel = CONV_POINTWISE;
    else if (ring_on && big && conv_ring_supported(out->cfg, p)) out->kernel = CONV_RING;
    if (p.n_src > 1 && out->kernel != CONV_RING) return locr_fail(eng, "a multi-source input reached a kernel other than the ring kernel", L.name.c_str());
    if (out->kernel != CONV_RING && (p.x_blk || p.y_blk || p.res_blk)) return locr_fail(eng, "a channel-blocked tensor reached a kernel that cannot address it", L.name.c_str());
    return 0;
}

static hipError_t conv_dispatch(const lumina_ocr* eng, const ConvChoice& k, const ConvParams& p, hipStream_t st) {
    if (k.kernel == CONV_RING) return conv_ring_launch(p, eng->ring_orient, st);
    return k.kernel == CONV_POINTWISE ? conv_pw_launch(p, st) : conv_launch(k.cfg, p, st);
}

// the launch's algorithmic work and the name of the instantiation that ran, for option time_convs
static void conv_account(const lumina_ocr* eng, const ConvLayer& L, const Tensor4& x, const ConvCall& c, const ConvParams& p, const ConvChoice& k, LaunchTimer* tm) {
    const ConvLayer* s = c.short_l;
    const double px = c.flat ? (double)p.pix_limit : (double)p.N * p.Ho * p.Wo;
    const double flop = (L.alg_flop_per_px > 0 ? px * L.alg_flop_per_px : 2.0 * px * L.ks * L.ks * L.cin * L.cout) + (s ? 2.0 * px * 4 * s->cin * s->cout : 0.0);
    // algorithmic HBM bytes: input once + output once (+ residual) + weights once
    double in_elems = (double)x.elems();
    if (x.n_src > 1) { in_elems = 0; for (int i = 0; i < x.n_src; ++i) in_elems += (double)x.n * (x.h >> x.xs_shift[i]) * (x.w >> x.xs_shift[i]) * x.src_c(i); }
    const double bytes = 2.0 * (in_elems + px * (c.out_mode == OUT_CONVT && p.fuse_w ? 4.0 : (double)L.cout) * (c.out_mode == OUT_UPSAMPLE ? (double)(1 << (2 * c.up_shift)) : (c.out_mode == OUT_POOL ? 0.25 : 1.0)) + (c.res ? px * (double)L.cout / (double)(1 << (2 * c.res_shift)) : 0.0) + (double)L.ks * L.ks * L.cin * L.cout +
                                (s ? px * (double)s->cout + 4.0 * s->cin * s->cout : 0.0));
    std::string kname = k.kernel == CONV_POINTWISE ? (L.cin == 64 ? "conv_pw_kernel<64>" : "conv_pw_kernel<128>") : conv_kernel_name(k.cfg);
    if (k.kernel == CONV_RING) kname = conv_ring_kernel_name(p, eng->ring_orient);
    if (s) { const size_t pos = kname.rfind(",0,2>"); if (pos != std::string::npos) kname.replace(pos, 5, ",5,2>"); }   // the fused-shortcut instantiation
    if (c.out_mode == OUT_POOL && k.kernel != CONV_RING) { const size_t pos = kname.rfind(",3,4>"); if (pos != std::string::npos) kname.replace(pos, 5, ",4,4>"); }  // the fused-pool instantiation
    tm->done(s ? L.name + "+short" : L.name, kname, flop, bytes);
}

int eng_run_conv(lumina_ocr* eng, const ConvLayer& L, const Tensor4& x, Tensor4* y, hipStream_t st, const ConvCall& c) {
    ConvParams p;
    RUN(conv_params(eng, L, x, *y, c, &p));
    if (x.p == nullptr || y->p == nullptr) return ws_null(eng, L.name.c_str());  // dry run (workspace sizing)
    LaunchTimer tm(eng, st);
    ConvChoice k;
    RUN(conv_choose(eng, L, p, c, &k));
    p.wpk = k.wpk;
    hipError_t e = conv_dispatch(eng, k, p, st);
    if (e != hipSuccess) return locr_fail(eng, L.name.c_str(), hipGetErrorString(e));
    if (tm.on()) conv_account(eng, L, x, c, p, k, &tm);
    return 0;
}

static void tap(lumina_ocr* eng, const char* name, const Tensor4& t) { if (eng->keep_taps && t.p) eng->taps[name] = t; }

// The 3-channel stem conv (load_stem) of N H x W uint8 images -> y: pixel * scale[c] + shift[c], 3x3 / stride 2, act; widths: valid
// width per image (the rest reads as zero) or null.  conv2 (detector): that 3x3 / stride-1 layer computed by the same kernel.
static int run_stem(lumina_ocr* eng, const char* name, const uint8_t* x, const int* widths, int N, int H, int W, const bf16_t* wpk, const float* bias,
                    int act, const float scale[3], const float shift[3], const Tensor4& y, hipStream_t st, const ConvLayer* conv2 = nullptr) {
    if (eng->arena.counting() || y.p == nullptr) return 0;
    StemParams sp{};
    sp.x = x; sp.wpk = wpk; sp.bias = bias; sp.y = y.p; sp.valid_w_per_img = widths;
    sp.N = N; sp.H = H; sp.W = W; sp.valid_h = H; sp.valid_w = W; sp.Ho = y.h; sp.Wo = y.w; sp.Cout_store = y.c;
    sp.act = act;
    for (int c = 0; c < 3; ++c) { sp.scale[c] = scale[c]; sp.shift[c] = shift[c]; }
    hipError_t e = conv2 ? stem12_launch(sp, conv2->wpk, conv2->bias, st) : stem_conv_launch(sp, st);
    return e == hipSuccess ? 0 : locr_fail(eng, name, hipGetErrorString(e));
}
static const float STEM_SCALE_PM1[3] = {2.0f / 255.0f, 2.0f / 255.0f, 2.0f / 255.0f}, STEM_SHIFT_PM1[3] = {-1.0f, -1.0f, -1.0f};   // pixels to [-1, 1] (rec, cls)

// ------------------------------------------------------------------------------ det forward
static int det_forward_sub(lumina_ocr* eng, const uint8_t* pages, int B, int H, int W, int Hp, int Wp, bf16_t* prob, hipStream_t st) {
    const bool dry = eng->arena.counting();
    auto& D = eng->det;
    // stem.conv1 + stem.conv2 fused (the first half-resolution tensor stays in LDS) unless it is wanted as a tap
    ConvLayer& c2 = D["stem.conv2"];
    const bool fuse_stem = eng->fuse_stem && eng->keep_taps != 1 && c2.cfg.bn == 32 && c2.cfg.ck == 16 && c2.act == ACT_RELU;
    Tensor4 t1{};
    if (!fuse_stem || dry) t1 = ws_tensor(eng, B, Hp / 2, Wp / 2, 32);
    Tensor4 t2 = ws_tensor(eng, B, Hp / 2, Wp / 2, 32);
    {
        const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};   // ImageNet
        float scale[3], shift[3];
        for (int c = 0; c < 3; ++c) { scale[c] = 1.0f / (255.0f * stdv[c]); shift[c] = -mean[c] / stdv[c]; }
        RUN(run_stem(eng, "stem.conv1", pages, nullptr, B, H, W, eng->stem_wpk, eng->stem_bias, ACT_RELU, scale, shift, fuse_stem ? t2 : t1, st, fuse_stem ? &c2 : nullptr));
    }
    if (!fuse_stem) {
        tap(eng, "stem.conv1", t1);
        RUN(eng_run_conv(eng, c2, t1, &t2, st)); tap(eng, "stem.conv2", t2);
    }
    // stem.conv3 + 3x3/s2 max pool: fused (the 64-channel half-resolution tensor, 93 MB per page, is never written) unless the
    // intermediate is wanted as a tap
    const bool fuse_pool = eng->fuse_pool && eng->keep_taps != 1;
    Tensor4 t3{};
    if (!fuse_pool || dry) t3 = ws_tensor(eng, B, Hp / 2, Wp / 2, 64);
    Tensor4 x = ws_tensor(eng, B, Hp / 4, Wp / 4, 64);
    if (fuse_pool) {
        RUN(eng_run_conv(eng, D["stem.conv3"], t2, &x, st, ConvCall().mode(OUT_POOL)));
    } else {
        RUN(eng_run_conv(eng, D["stem.conv3"], t2, &t3, st)); tap(eng, "stem.conv3", t3);
        if (!dry && x.p) {
            hipError_t e = maxpool_launch(t3.p, x.p, B, t3.h, t3.w, 64, 3, 2, 1, x.h, x.w, st);
            if (e != hipSuccess) return locr_fail(eng, "stem.pool", hipGetErrorString(e));
        }
    }
    tap(eng, "stem.pool", x);
    const int chs[4] = {64, 128, 256, 512};
    Tensor4 feats[4];
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 2; ++j) {
            const std::string p = "s" + std::to_string(i) + ".b" + std::to_string(j);
            const int stride = (i > 0 && j == 0) ? 2 : 1;
            Tensor4 y = ws_tensor(eng, B, x.h / stride, x.w / stride, chs[i]);
            // stage-0 tensors that only the ring kernel touches are stored channel-blocked [n][C/16][H][W][16]: a 16-channel chunk
            // pass then reads / writes whole cache lines (NHWC: 32 of every 128 bytes per pass); same values, DESIGN.md 3.2
            const bool blk = i == 0 && eng->blocked_layout && eng->keep_taps == 0 && eng->conv_ring && !dry &&
                             conv_takes_big(eng, D[p + ".conv0"], B, x.h, x.w, false) && conv_takes_big(eng, D[p + ".conv1"], B, x.h, x.w, false);
            y.blk = blk;
            // stages 1-3, first block: conv0 (3x3 / s2) and the vd shortcut (2x2 / s2) read the same input — one launch computes both
            const ConvLayer& c0 = D[p + ".conv0"];
            const bool fuse_sc = eng->fuse_short && i > 0 && j == 0 && x.h % 2 == 0 && x.w % 2 == 0 && c0.cfg.bn == 64 && c0.cfg.ck == 16 && c0.cfg.nw == 4 &&
                                 D[p + ".short"].cfg.bn == 64 && D[p + ".short"].cfg.ck == 16;
            Tensor4 sc = x;
            if (j == 0) sc = ws_tensor(eng, B, y.h, y.w, chs[i]);
            if (fuse_sc) {
                RUN(eng_run_conv(eng, c0, x, &y, st, ConvCall().shortcut(&D[p + ".short"], &sc)));
            } else {
                RUN(eng_run_conv(eng, c0, x, &y, st));
                if (j == 0) RUN(eng_run_conv(eng, D[p + ".short"], x, &sc, st, ConvCall().flat_gemm(i == 0)));
            }
            Tensor4 o = ws_tensor(eng, B, y.h, y.w, chs[i]);
            o.blk = blk && j == 0;
            RUN(eng_run_conv(eng, D[p + ".conv1"], y, &o, st, ConvCall().residual(&sc)));
            tap(eng, p.c_str(), o);
            x = o;
        }
        feats[i] = x;
    }
    // FPN: laterals with fused top-down nearest-upsample add
    Tensor4 in5 = ws_tensor(eng, B, feats[3].h, feats[3].w, 256);
    RUN(eng_run_conv(eng, D["fpn.in5"], feats[3], &in5, st));
    Tensor4 out4 = ws_tensor(eng, B, feats[2].h, feats[2].w, 256);
    RUN(eng_run_conv(eng, D["fpn.in4"], feats[2], &out4, st, ConvCall().residual(&in5, 1)));
    Tensor4 out3 = ws_tensor(eng, B, feats[1].h, feats[1].w, 256);
    RUN(eng_run_conv(eng, D["fpn.in3"], feats[1], &out3, st, ConvCall().residual(&out4, 1)));
    // DBHead's first conv runs over the concat [up8(p5), up4(p4), up2(p3), p2].  Default: the smoothing convs write p5 .. p2 at their
    // own resolution and head.conv1 (ring kernel) reads them nearest-upsampled through its halo addressing — the 1/4-resolution
    // 256-channel concat (1.5 GB per 16 A4 pages, written 4 / 16 / 64-fold replicated) never exists.  Same products, same order.
    ConvLayer& hc1 = D["head.conv1"];
    const bool multi = eng->fpn_multi && eng->keep_taps != 1 && eng->conv_ring && conv_takes_big(eng, hc1, B, Hp / 4, Wp / 4, false) &&
                       (Hp / 4) % 8 == 0 && (Wp / 4) % 8 == 0;
    auto slice = [](const Tensor4& t, int b0, int nb) {
        Tensor4 r = t;
        r.n = nb;
        if (t.p) r.p = t.p + (size_t)b0 * t.h * t.w * t.c;
        return r;
    };
    // fpn.p2.  Default: ONE conv over [c2 | up2(out3)] with the lateral fpn.in2 composed into its weights (compose_fpn_p2; ring kernel,
    // multi-source input, whatever the page size: the arithmetic definition must not depend on which kernel a geometry selects) —
    // the 256-channel 1/4-resolution lateral is never computed.  Otherwise (option fpn_compose = 0, ring kernel off, a lateral with
    // a bias): in2 -> lateral tensor -> p2.
    const bool compose = eng->fpn_compose && eng->conv_ring && D.count("fpn.p2c") != 0;
    auto run_p2 = [&](const Tensor4& c2, const Tensor4& o3, Tensor4* lateral, Tensor4* dst, int y_cstride, int y_coff) -> int {
        if (compose) {
            Tensor4 in = c2;
            in.c = 320; in.n_src = 2;
            in.xs[0] = c2.p; in.xs[1] = o3.p; in.p = o3.p;
            in.xs_shift[0] = 0; in.xs_shift[1] = 1; in.xs_c[0] = 64; in.xs_c[1] = 256;
            return eng_run_conv(eng, D["fpn.p2c"], in, dst, st, ConvCall().channel_slice(y_cstride, y_coff));
        }
        RUN(eng_run_conv(eng, D["fpn.in2"], c2, lateral, st, ConvCall().residual(&o3, 1)));
        return eng_run_conv(eng, D["fpn.p2"], *lateral, dst, st, ConvCall().channel_slice(y_cstride, y_coff));
    };
    auto head_tail = [&](const Tensor4& h1, bf16_t* prob_g, int nb) -> int {
        Tensor4 pm; pm.p = dry ? nullptr : prob_g; pm.n = nb; pm.h = Hp; pm.w = Wp; pm.c = 1;
        if (eng->fuse_head && eng->keep_taps != 1)   // DBHead tail in one launch: the 64-channel 1/2-resolution tensor never exists
            return eng_run_conv(eng, D["head.convt2.fused"], h1, &pm, st, ConvCall().mode(OUT_CONVT));
        Tensor4 h2 = ws_tensor(eng, nb, Hp / 2, Wp / 2, 64);
        RUN(eng_run_conv(eng, D["head.convt2"], h1, &h2, st, ConvCall().mode(OUT_CONVT))); tap(eng, "head.convt2", h2);
        return eng_run_conv(eng, D["head.convt3"], h2, &pm, st, ConvCall().mode(OUT_CONVT1));
    };
    if (multi) {
        Tensor4 p5 = ws_tensor(eng, B, in5.h, in5.w, 64), p4 = ws_tensor(eng, B, out4.h, out4.w, 64), p3 = ws_tensor(eng, B, out3.h, out3.w, 64);
        RUN(eng_run_conv(eng, D["fpn.p5"], in5, &p5, st)); tap(eng, "fpn.p5", p5);
        RUN(eng_run_conv(eng, D["fpn.p4"], out4, &p4, st)); tap(eng, "fpn.p4", p4);
        RUN(eng_run_conv(eng, D["fpn.p3"], out3, &p3, st)); tap(eng, "fpn.p3", p3);
        // The 1/4-resolution tail — lateral in2 (1.5 GB per 16 pages), p2, head.conv1, DBHead tail — runs in groups of tail_group
        // pages: each consumer then finds part of its producer's output still in the 256 MB Infinity Cache (A/B on one device,
        // 64 A4 pages in one forward: p2 3.68 -> 3.47 ms, head.conv1 3.32 -> 3.12 ms), and the 256-channel lateral only ever exists for
        // one group.  Launch order only: results are per page.
        const int G = (eng->keep_taps == 0 && eng->tail_group > 0 && B > eng->tail_group) ? eng->tail_group : B;
        Tensor4 out2{};
        if (!compose) out2 = ws_tensor(eng, G, feats[0].h, feats[0].w, 256);
        Tensor4 p2 = ws_tensor(eng, G, feats[0].h, feats[0].w, 64);
        Tensor4 h1 = ws_tensor(eng, G, Hp / 4, Wp / 4, 64);
        for (int g0 = 0; g0 < B; g0 += G) {
            const int nb = B - g0 < G ? B - g0 : G;
            Tensor4 o2 = slice(out2, 0, nb), p2g = slice(p2, 0, nb), h1g = slice(h1, 0, nb), o3 = slice(out3, g0, nb);
            RUN(run_p2(slice(feats[0], g0, nb), o3, &o2, &p2g, 0, 0));
            tap(eng, "fpn.p2", p2g);
            Tensor4 cat = p2g;
            cat.c = 256; cat.n_src = 4;
            cat.xs[0] = slice(p5, g0, nb).p; cat.xs[1] = slice(p4, g0, nb).p; cat.xs[2] = slice(p3, g0, nb).p; cat.xs[3] = p2g.p;
            cat.xs_shift[0] = 3; cat.xs_shift[1] = 2; cat.xs_shift[2] = 1; cat.xs_shift[3] = 0;
            RUN(eng_run_conv(eng, hc1, cat, &h1g, st)); tap(eng, "head.conv1", h1g);
            RUN(head_tail(h1g, prob ? prob + (size_t)g0 * Hp * Wp : nullptr, nb));
        }
        return 0;
    }
    Tensor4 out2{};
    if (!compose) out2 = ws_tensor(eng, B, feats[0].h, feats[0].w, 256);
    // smooth convs write straight into the channel slices of the 1/4-resolution concat (replicated)
    Tensor4 fuse = ws_tensor(eng, B, Hp / 4, Wp / 4, 256);
    RUN(eng_run_conv(eng, D["fpn.p5"], in5, &fuse, st, ConvCall().upsample(3).channel_slice(256, 0)));
    RUN(eng_run_conv(eng, D["fpn.p4"], out4, &fuse, st, ConvCall().upsample(2).channel_slice(256, 64)));
    RUN(eng_run_conv(eng, D["fpn.p3"], out3, &fuse, st, ConvCall().upsample(1).channel_slice(256, 128)));
    RUN(run_p2(feats[0], out3, &out2, &fuse, 256, 192));
    tap(eng, "fpn.fuse", fuse);
    Tensor4 h1 = ws_tensor(eng, B, Hp / 4, Wp / 4, 64);
    RUN(eng_run_conv(eng, hc1, fuse, &h1, st)); tap(eng, "head.conv1", h1);
    return head_tail(h1, prob, B);
}

// A forward over n images in sub-batches of sb: run(b0, nb) -> 0 / 1 runs images b0 .. b0 + nb - 1, taking its tensors from eng->arena.
// A dry run of one full sub-batch on a counting arena (run(0, sb): no launch) sizes the workspace; every sub-batch then carves it afresh.
template <class Run> static int forward_sub_batched(lumina_ocr* eng, int n, int sb, Run&& run) {
    eng->arena = Arena();
    RUN(run(0, sb));
    RUN(eng_ws_reserve(eng, eng->arena.off + 4096));
    eng->taps.clear();
    for (int b0 = 0; b0 < n; b0 += sb) {
        eng->arena = Arena(eng->ws.get(), eng->ws.cap);
        RUN(run(b0, n - b0 < sb ? n - b0 : sb));
        if (eng->arena.overflow) return ws_null(eng, "forward");
    }
    return 0;
}

int eng_det_forward(lumina_ocr* eng, const uint8_t* pages, int B, int H, int W, int Hp, int Wp, bf16_t* prob, hipStream_t st) {
    if (!eng->det_loaded) return locr_fail(eng, "det_forward", "det weights not loaded");
    if (Hp % 32 || Wp % 32 || Hp < H || Wp < W || B <= 0) return locr_fail(eng, "det_forward", "Hp/Wp must be multiples of 32 and >= H/W");
    LOCR_CHECK(hipSetDevice(eng->device));
    return forward_sub_batched(eng, B, eng->det_sub_batch < B ? eng->det_sub_batch : B, [&](int b0, int nb) {
        return det_forward_sub(eng, pages + (size_t)b0 * H * W * 3, nb, H, W, Hp, Wp, prob + (size_t)b0 * Hp * Wp, st);
    });
}

// ------------------------------------------------------------------------------ rec
// (cp16, make_div and the MobileNetV3 rows: blob_check.h, which lists the tensors from them)
static bool make_dw(lumina_ocr* eng, const std::map<std::string, HostBlobTensor>& m, const std::string& name, int k, int c_r, int c_p, DwLayer* L) {
    const HostBlobTensor *w, *b;
    if (!get_wb(eng, m, name, &w, &b)) return false;
    if (w->dims.size() != 4 || w->dims[0] != c_r || w->dims[1] != k || w->dims[3] != 1) { locr_fail(eng, "dw shape", name.c_str()); return false; }
    std::vector<bf16_t> wt((size_t)k * k * c_p, 0);
    const bf16_t* src = reinterpret_cast<const bf16_t*>(w->data);
    for (int c = 0; c < c_r; ++c)
        for (int t = 0; t < k * k; ++t) wt[(size_t)t * c_p + c] = src[(size_t)c * k * k + t];
    std::vector<float> bias(c_p, 0.f);
    memcpy(bias.data(), b->data, sizeof(float) * c_r);
    L->k = k; L->c = c_p;
    L->w = static_cast<bf16_t*>(eng_upload(eng, wt.data(), wt.size() * sizeof(bf16_t)));
    L->bias = static_cast<float*>(eng_upload(eng, bias.data(), bias.size() * sizeof(float)));
    return L->w && L->bias;
}

static bool make_se(lumina_ocr* eng, const std::map<std::string, HostBlobTensor>& m, const std::string& pfx, int c_r, int c_p, int mid, SeLayer* L) {
    const HostBlobTensor *w1, *b1, *w2, *b2;
    if (!get_wb(eng, m, pfx + ".se1", &w1, &b1) || !get_wb(eng, m, pfx + ".se2", &w2, &b2)) return false;
    if (w1->dims[0] != mid || w1->dims[3] != c_r || w2->dims[0] != c_r || w2->dims[3] != mid) { locr_fail(eng, "se shape", pfx.c_str()); return false; }
    std::vector<bf16_t> a((size_t)mid * c_p, 0), bmat((size_t)c_p * mid, 0);
    const bf16_t* s1 = reinterpret_cast<const bf16_t*>(w1->data);
    const bf16_t* s2 = reinterpret_cast<const bf16_t*>(w2->data);
    for (int i = 0; i < mid; ++i) memcpy(&a[(size_t)i * c_p], &s1[(size_t)i * c_r], sizeof(bf16_t) * c_r);
    memcpy(bmat.data(), s2, sizeof(bf16_t) * (size_t)c_r * mid);
    std::vector<float> bb2(c_p, 0.f);
    memcpy(bb2.data(), b2->data, sizeof(float) * c_r);
    L->c = c_p; L->mid = mid;
    L->w1 = static_cast<bf16_t*>(eng_upload(eng, a.data(), a.size() * sizeof(bf16_t)));
    L->w2 = static_cast<bf16_t*>(eng_upload(eng, bmat.data(), bmat.size() * sizeof(bf16_t)));
    L->b1 = static_cast<float*>(eng_upload(eng, b1->data, sizeof(float) * mid));
    L->b2 = static_cast<float*>(eng_upload(eng, bb2.data(), bb2.size() * sizeof(float)));
    return L->w1 && L->w2 && L->b1 && L->b2;
}

// the 11 MobileNetV3-small blocks (arch._MV3_SMALL) of the recogniser ("rec") or the orientation classifier ("cls"): channel counts at
// `scale`, vertical strides sh[11], input channels cin
static int load_mv3_blocks(lumina_ocr* eng, const std::map<std::string, HostBlobTensor>& m, const std::string& prefix, double scale, const int* sh,
                           int cin, std::vector<RecBlock>* blocks) {
    const Mv3Row* rows = MV3_ROWS;   // (blob_check.h: the tensor list check_blob holds the blob to is written from the same rows)
    blocks->clear();
    blocks->resize(11);
    for (int i = 0; i < 11; ++i) {
        RecBlock& B = (*blocks)[i];
        B.k = rows[i].k; B.cin = cin; B.exp = make_div(rows[i].exp * scale); B.cout = make_div(rows[i].c * scale);
        B.se = rows[i].se; B.se_mid = B.exp / 4; B.stride_h = sh[i]; B.act = rows[i].hswish ? ACT_HSWISH : ACT_RELU;
        B.res = (B.stride_h == 1 && B.cin == B.cout);
        const std::string p = prefix + ".b" + std::to_string(i);
        if (!make_conv(eng, m, p + ".expand", 1, 1, B.cin, B.exp, cp16(B.cin), cp16(B.exp), B.act, &B.expand)) return 1;
        if (!make_dw(eng, m, p + ".dw", B.k, B.exp, cp16(B.exp), &B.dw)) return locr_fail(eng, "dw", p.c_str());
        {   // the same expand weights once more, in the fused kernel's fragment order
            const HostBlobTensor *w, *b;
            if (!get_wb(eng, m, p + ".expand", &w, &b)) return 1;
            const int ec = cp16(B.exp), cc = cp16(B.cin);
            std::vector<bf16_t> padded((size_t)ec * cc, 0), packed(mbconv_expand_packed_elems(ec, cc));
            const bf16_t* src = reinterpret_cast<const bf16_t*>(w->data);
            for (int r = 0; r < B.exp; ++r) memcpy(&padded[(size_t)r * cc], &src[(size_t)r * B.cin], sizeof(bf16_t) * B.cin);
            mbconv_pack_expand(padded.data(), ec, cc, packed.data());
            std::vector<float> bias((size_t)((ec + 31) / 32) * 32, 0.f);
            memcpy(bias.data(), b->data, sizeof(float) * B.exp);
            B.we_pk = static_cast<bf16_t*>(eng_upload(eng, packed.data(), packed.size() * sizeof(bf16_t)));
            B.be_pk = static_cast<float*>(eng_upload(eng, bias.data(), bias.size() * sizeof(float)));
            if (!B.we_pk || !B.be_pk) return locr_fail(eng, "upload", (p + ".expand (fused)").c_str());
        }
        if (B.se && !make_se(eng, m, p, B.exp, cp16(B.exp), B.se_mid, &B.sel)) return 1;
        if (!make_conv(eng, m, p + ".project", 1, 1, B.exp, B.cout, cp16(B.exp), cp16(B.cout), ACT_NONE, &B.project)) return 1;
        cin = B.cout;
    }
    return 0;
}

int eng_load_rec(lumina_ocr* eng, const void* blob, size_t n) {
    BlobMap m;
    std::vector<uint64_t> aligned;
    if (!checked_blob(eng, "load_rec_weights", BLOB_REC, blob, n, &aligned, &m)) return 1;
    LOCR_CHECK(hipSetDevice(eng->device));
    eng->rec_loaded = false;   // from here on only an upload can fail; the recogniser then stays unloaded
    const double scale = REC_SCALE;
    const int c0 = make_div(16 * scale);
    RUN(load_stem(eng, m, "rec.conv1", c0, &eng->rstem_wpk, &eng->rstem_bias));
    if (load_mv3_blocks(eng, m, "rec", scale, REC_STRIDES, c0, &eng->rblocks)) return 1;
    const int cin = eng->rblocks.back().cout;
    if (!make_conv(eng, m, "rec.conv2", 1, 1, cin, 288, cp16(cin), 288, ACT_HSWISH, &eng->rconv2)) return 1;
    eng->rconv2_spk = nullptr;
    if (cin == 48) {   // the same weights once more, in seq_gemm's tile order (conv2 + pool in one launch)
        std::vector<bf16_t> spk(seq_gemm_packed_elems(288, cin));
        seq_gemm_pack_weights(reinterpret_cast<const bf16_t*>(m.find("rec.conv2.w")->second.data), 288, cin, spk.data());
        eng->rconv2_spk = static_cast<bf16_t*>(eng_upload(eng, spk.data(), spk.size() * sizeof(bf16_t)));
        if (!eng->rconv2_spk) return locr_fail(eng, "upload", "rec.conv2 (seq_gemm)");
    }
    // LSTM: x-projection of both directions as one GEMM; recurrent weights [2][4H][H]
    // (check_blob has proved all six tensors of a layer: w_ih bf16 [4H][din], w_hh bf16 [4H][H], b f32 [4H], so the concatenations
    // below are exactly [8H][din], [8H] and [2][4H][H], which is what make_conv, seq_gemm_pack_weights and lstm_kernel read)
    const int Hh = LSTM_HIDDEN;
    for (int l = 0; l < 2; ++l) {
        const int din = l == 0 ? 288 : 2 * Hh;
        const std::string pf = "lstm.l" + std::to_string(l) + ".fw", pb = "lstm.l" + std::to_string(l) + ".bw";
        auto wf = m.find(pf + ".w_ih"), wb = m.find(pb + ".w_ih"), bf = m.find(pf + ".b"), bb = m.find(pb + ".b");
        auto hf = m.find(pf + ".w_hh"), hb = m.find(pb + ".w_hh");
        if (wf == m.end() || wb == m.end() || bf == m.end() || bb == m.end() || hf == m.end() || hb == m.end())
            return locr_fail(eng, "lstm tensors missing", pf.c_str());
        if (wf->second.nbytes != (size_t)4 * Hh * din * 2 || wb->second.nbytes != wf->second.nbytes || bf->second.nbytes != (size_t)4 * Hh * 4 ||
            bb->second.nbytes != bf->second.nbytes || hf->second.nbytes != (size_t)4 * Hh * Hh * 2 || hb->second.nbytes != hf->second.nbytes)
            return locr_fail(eng, "lstm shape", pf.c_str());   // (an assertion: check_blob has refused such a blob already)
        // synthesise a 1x1 conv blob entry [8H][1][1][din]
        std::vector<uint8_t> wcat(wf->second.nbytes + wb->second.nbytes), bcat(bf->second.nbytes + bb->second.nbytes);
        memcpy(wcat.data(), wf->second.data, wf->second.nbytes); memcpy(wcat.data() + wf->second.nbytes, wb->second.data, wb->second.nbytes);
        memcpy(bcat.data(), bf->second.data, bf->second.nbytes); memcpy(bcat.data() + bf->second.nbytes, bb->second.data, bb->second.nbytes);
        std::map<std::string, HostBlobTensor> mm;
        mm["x.w"] = HostBlobTensor{1, {8 * Hh, 1, 1, din}, wcat.data(), wcat.size()};
        mm["x.b"] = HostBlobTensor{0, {8 * Hh}, bcat.data(), bcat.size()};
        if (!make_conv(eng, mm, "x", 1, 1, din, 8 * Hh, din, 8 * Hh, ACT_NONE, &eng->xproj[l])) return 1;
        eng->xproj[l].name = "lstm.l" + std::to_string(l) + ".xproj";
        {   // and in seq_gemm's tile order
            std::vector<bf16_t> spk(seq_gemm_packed_elems(8 * Hh, din));
            seq_gemm_pack_weights(reinterpret_cast<const bf16_t*>(wcat.data()), 8 * Hh, din, spk.data());
            eng->xproj_spk[l] = static_cast<bf16_t*>(eng_upload(eng, spk.data(), spk.size() * sizeof(bf16_t)));
            if (!eng->xproj_spk[l]) return locr_fail(eng, "upload", "xproj (seq_gemm)");
        }
        std::vector<uint8_t> hcat(hf->second.nbytes + hb->second.nbytes);
        memcpy(hcat.data(), hf->second.data, hf->second.nbytes); memcpy(hcat.data() + hf->second.nbytes, hb->second.data, hb->second.nbytes);
        eng->whh[l] = static_cast<bf16_t*>(eng_upload(eng, hcat.data(), hcat.size()));
        if (!eng->whh[l]) return locr_fail(eng, "upload", "whh");
    }
    RUN(load_ctc_head(eng, m, "ctc.fc", 2 * Hh, 0, &eng->num_classes, &eng->ctc_ntiles, &eng->ctc_wpk, &eng->ctc_bias));
    eng->rec_loaded = true;
    return 0;
}

#define LAUNCH(name, expr)                                                                                        \
    do {                                                                                                          \
        if (!dry) {                                                                                               \
            if (eng->arena.overflow) return ws_null(eng, name);                                                   \
            hipError_t _e = (expr); if (_e != hipSuccess) return locr_fail(eng, name, hipGetErrorString(_e));     \
        }                                                                                                         \
    } while (0)

// one MobileNetV3 block (expand -> depthwise -> [squeeze-excite] -> project [+ residual]) of the recogniser or the classifier on *x, which
// becomes the block's output (tap `name`)
static int run_mv3_block(lumina_ocr* eng, const RecBlock& B, const std::string& name, Tensor4* x, hipStream_t st) {
    const bool dry = eng->arena.counting();
    const int N = x->n;
    const int ho = (x->h + 2 * (B.k / 2) - B.k) / B.stride_h + 1;
    MbParams mp{};
    mp.we = B.we_pk; mp.be = B.be_pk; mp.wd = B.dw.w; mp.bd = B.dw.bias;
    mp.N = N; mp.H = x->h; mp.W = x->w; mp.cin = x->c; mp.expc = cp16(B.exp); mp.Ho = ho; mp.act = B.act;
    const bool fused_mb = eng->fuse_mb && mbconv_supported(mp, B.k, B.stride_h);
    Tensor4 e1{};
    if (!fused_mb || dry) e1 = ws_tensor(eng, N, x->h, x->w, cp16(B.exp));   // (dry run sizes the arena for the unfused path too)
    Tensor4 d = ws_tensor(eng, N, ho, x->w, cp16(B.exp));
    float* pool = B.se ? eng->arena.take<float>((size_t)N * mb_strips(x->w) * d.c) : nullptr;
    if (fused_mb) {
        mp.x = x->p; mp.d = d.p; mp.pool = pool;   // squeeze-excite blocks: the pooled sums leave with the tile (the tensor is not read again for them)
        if (!dry && x->p && d.p) {
            LaunchTimer tm(eng, st);
            LAUNCH("mbconv", mbconv_launch(mp, B.k, B.stride_h, st));
            const double opx = (double)N * ho * x->w, ipx = (double)N * x->h * x->w;
            tm.done(name + ".expand+dw", "mbconv_kernel<" + std::to_string(B.k) + "," + std::to_string(B.stride_h) + "," + std::to_string(B.act) + ">",
                    2.0 * ipx * x->c * mp.expc + 2.0 * opx * B.k * B.k * mp.expc, 2.0 * (ipx * x->c + opx * mp.expc));
        }
    } else {
        RUN(eng_run_conv(eng, B.expand, *x, &e1, st, ConvCall().flat_gemm()));
        LAUNCH("dwconv", dwconv_launch(e1.p, B.dw.w, B.dw.bias, d.p, N, e1.h, e1.w, e1.c, B.k, B.stride_h, B.act, st));
        if (B.se) LAUNCH("se_pool", se_pool_launch(d.p, pool, N, d.h, d.w, d.c, st));   // the same sums in the same order
    }
    const bf16_t* se_gate_ptr = nullptr;
    if (B.se) {
        bf16_t* gate = eng->arena.take<bf16_t>((size_t)N * d.c);
        LAUNCH("se_fc", se_fc_launch(pool, mb_strips(d.w), B.sel.w1, B.sel.b1, B.sel.w2, B.sel.b2, gate, N, d.h * d.w, d.c, B.sel.mid, st));
        se_gate_ptr = gate;   // the scaling itself is fused into the project conv's operand staging
    }
    Tensor4 o = ws_tensor(eng, N, d.h, d.w, cp16(B.cout));
    RUN(eng_run_conv(eng, B.project, d, &o, st, ConvCall().flat_gemm().residual(B.res ? x : nullptr).gated(se_gate_ptr)));
    tap(eng, name.c_str(), o);
    *x = o;
    return 0;
}

static int rec_forward_sub(lumina_ocr* eng, const uint8_t* crops, const int* widths, int N, int* idx, float* prob, hipStream_t st) {
    const bool dry = eng->arena.counting();
    const int T = 80;
    Tensor4 x = ws_tensor(eng, N, 16, 160, 16);
    RUN(run_stem(eng, "rec.conv1", crops, widths, N, 32, 320, eng->rstem_wpk, eng->rstem_bias, ACT_HSWISH, STEM_SCALE_PM1, STEM_SHIFT_PM1, x, st));
    tap(eng, "rec.conv1", x);
    for (size_t bi = 0; bi < eng->rblocks.size(); ++bi) RUN(run_mv3_block(eng, eng->rblocks[bi], "rec.b" + std::to_string(bi), &x, st));
    // one seq_gemm launch (timed as `layer`) in place of a 1x1 conv [+ 2x2 pool]; the bias is the conv layer's own (64-column tiles)
    auto seq_gemm = [&](const char* layer, const ConvLayer& L, const bf16_t* spk, const Tensor4& in, Tensor4& out, int epi) -> int {
        SeqGemmParams sp{};
        sp.x = in.p; sp.wpk = spk; sp.bias = L.bias; sp.y = out.p;
        sp.M = N * T; sp.K = in.c; sp.Cout = out.c; sp.T = T; sp.epi = epi;
        if (dry) return 0;
        LaunchTimer tm(eng, st);
        LAUNCH(layer, seq_gemm_launch(sp, st));
        const double px = (double)N * in.h * in.w;
        tm.done(layer, seq_gemm_kernel_name(sp), 2.0 * px * in.c * out.c, 2.0 * (px * in.c + (double)sp.M * out.c + (double)in.c * out.c));
        return 0;
    };
    const bool seq_fills = (N * T + 127) / 128 >= eng->seq_gemm_min;   // enough row tiles for the A-stationary kernel (engine.h)
    const bool pool_fused = seq_fills && eng->fuse_conv2_pool && eng->keep_taps != 1 && eng->rconv2_spk != nullptr && eng->rconv2.cfg.bn == 64 &&
                            x.h == 2 && x.w == 2 * T && x.c == 48;
    Tensor4 f{};
    if (!pool_fused || dry) f = ws_tensor(eng, N, x.h, x.w, 288);   // (dry run sizes the arena for the unfused path too)
    Tensor4 seq = ws_tensor(eng, N, 1, T, 288);
    if (pool_fused) {
        RUN(seq_gemm("rec.conv2+pool", eng->rconv2, eng->rconv2_spk, x, seq, SEQ_POOL4));
    } else {
        RUN(eng_run_conv(eng, eng->rconv2, x, &f, st, ConvCall().flat_gemm())); tap(eng, "rec.conv2", f);
        LAUNCH("rec.pool", maxpool_launch(f.p, seq.p, N, f.h, f.w, 288, 2, 2, 0, 1, T, st));
    }
    tap(eng, "rec.feat", seq);
    for (int l = 0; l < 2; ++l) {
        Tensor4 xp = ws_tensor(eng, N, 1, T, 8 * 96);
        if (seq_fills && eng->fuse_xproj && eng->xproj_spk[l] != nullptr && eng->xproj[l].cfg.bn == 64 && (seq.c == 288 || seq.c == 192))
            RUN(seq_gemm(eng->xproj[l].name.c_str(), eng->xproj[l], eng->xproj_spk[l], seq, xp, SEQ_STORE));
        else
            RUN(eng_run_conv(eng, eng->xproj[l], seq, &xp, st, ConvCall().flat_gemm()));
        Tensor4 hs = ws_tensor(eng, N, 1, T, 2 * 96);
        {
            LaunchTimer tm(eng, st, !dry);
            LAUNCH("lstm", lstm_recurrent_launch(xp.p, eng->whh[l], hs.p, N, T, st, eng->lstm_waves));
            tm.done("lstm.l" + std::to_string(l), eng->lstm_waves == 3 ? "lstm3_kernel" : "lstm_kernel", 2.0 * N * T * 2 * 96 * 384, 2.0 * N * T * (768 + 192));
        }
        tap(eng, l == 0 ? "lstm.l0" : "lstm.l1", hs);
        seq = hs;
    }
    if (!dry) {
        CtcFcParams cp{};
        cp.seq = seq.p; cp.wpk = eng->ctc_wpk; cp.bias = eng->ctc_bias; cp.out_idx = idx; cp.out_prob = prob;
        cp.M = N * T; cp.K = 192; cp.C = eng->num_classes; cp.ntiles = eng->ctc_ntiles;
        LaunchTimer tm(eng, st);
        LAUNCH("ctc_fc_argmax", ctc_fc_argmax_launch(cp, st));
        tm.done("ctc.fc+argmax", "ctc_fc_argmax_kernel<0>", 2.0 * cp.M * cp.K * cp.C, 2.0 * cp.M * cp.K + 8.0 * cp.M + 2.0 * cp.K * cp.C);
    }
    return 0;
}

int eng_rec_forward(lumina_ocr* eng, const uint8_t* crops, const int* widths, int N, int* idx, float* prob, hipStream_t st) {
    if (!eng->rec_loaded) return locr_fail(eng, "rec_forward", "rec weights not loaded");
    if (N <= 0) return 0;
    LOCR_CHECK(hipSetDevice(eng->device));
    return forward_sub_batched(eng, N, eng->rec_sub_batch < N ? eng->rec_sub_batch : N, [&](int b0, int nb) {
        return rec_forward_sub(eng, crops + (size_t)b0 * 32 * 320 * 3, widths ? widths + b0 : nullptr, nb, idx + (size_t)b0 * 80, prob + (size_t)b0 * 80, st);
    });
}

// ------------------------------------------------------------------------------ orientation classifier (PP-OCR cls)
// MobileNetV3-small x0.35 (arch.cls_block_table: the recogniser's blocks, vertical strides 2 on blocks 0, 1, 3, 8) on 48 x 192 crops:
// 24 x 96 after the stem, 2 x 96 after block 10 -> conv2 (1x1, 200, hswish) -> 2x2 max pool -> 48 positions -> cls_head_kernel
int eng_load_cls(lumina_ocr* eng, const void* blob, size_t n) {
    BlobMap m;
    std::vector<uint64_t> aligned;
    if (!checked_blob(eng, "load_cls_weights", BLOB_CLS, blob, n, &aligned, &m)) return 1;
    LOCR_CHECK(hipSetDevice(eng->device));
    eng->cls_loaded = false;   // from here on only an upload can fail; the classifier then stays unloaded
    const double scale = CLS_SCALE;
    const int c0 = make_div(16 * scale);
    RUN(load_stem(eng, m, "cls.conv1", c0, &eng->cstem_wpk, &eng->cstem_bias));
    if (load_mv3_blocks(eng, m, "cls", scale, CLS_STRIDES, c0, &eng->cblocks)) return 1;
    const int cin = eng->cblocks.back().cout;
    if (!make_conv(eng, m, "cls.conv2", 1, 1, cin, CLS_FEAT, cp16(cin), cp16(CLS_FEAT), ACT_HSWISH, &eng->cconv2)) return 1;
    {
        auto w = m.find("cls.fc.w"), b = m.find("cls.fc.b");
        if (w == m.end() || b == m.end() || w->second.dtype != 1 || b->second.dtype != 0 || w->second.dims.size() != 2 || w->second.dims[0] != 2 ||
            w->second.dims[1] != CLS_FEAT || b->second.dims.size() != 1 || b->second.dims[0] != 2)
            return locr_fail(eng, "cls.fc", "missing/shape (w bf16 [2][200], b f32 [2])");
        std::vector<float> fw(2 * CLS_FEAT);
        const bf16_t* src = reinterpret_cast<const bf16_t*>(w->second.data);
        for (int i = 0; i < 2 * CLS_FEAT; ++i) fw[i] = host_bf16_to_f32(src[i]);
        eng->cls_fc_w = static_cast<float*>(eng_upload(eng, fw.data(), fw.size() * sizeof(float)));
        eng->cls_fc_b = static_cast<float*>(eng_upload(eng, b->second.data, 2 * sizeof(float)));
        if (!eng->cls_fc_w || !eng->cls_fc_b) return locr_fail(eng, "upload", "cls.fc");
    }
    eng->cls_loaded = true;
    return 0;
}

static int cls_forward_sub(lumina_ocr* eng, const uint8_t* crops, const int* widths, int N, float thresh, int* label, float* score, int* flip,
                           hipStream_t st) {
    const bool dry = eng->arena.counting();
    Tensor4 x = ws_tensor(eng, N, CLS_H / 2, CLS_W / 2, 16);
    RUN(run_stem(eng, "cls.conv1", crops, widths, N, CLS_H, CLS_W, eng->cstem_wpk, eng->cstem_bias, ACT_HSWISH, STEM_SCALE_PM1, STEM_SHIFT_PM1, x, st));
    tap(eng, "cls.conv1", x);
    for (size_t bi = 0; bi < eng->cblocks.size(); ++bi) RUN(run_mv3_block(eng, eng->cblocks[bi], "cls.b" + std::to_string(bi), &x, st));
    Tensor4 f = ws_tensor(eng, N, x.h, x.w, eng->cconv2.cout);
    RUN(eng_run_conv(eng, eng->cconv2, x, &f, st, ConvCall().flat_gemm())); tap(eng, "cls.conv2", f);
    if (f.h != 2 || f.w % 2) return locr_fail(eng, "cls_forward", "unexpected feature map");
    Tensor4 feat = ws_tensor(eng, N, 1, f.w / 2, f.c);
    LAUNCH("cls.pool", maxpool_launch(f.p, feat.p, N, f.h, f.w, f.c, 2, 2, 0, 1, feat.w, st));
    tap(eng, "cls.feat", feat);
    Tensor4 logits = ws_tensor(eng, N, 1, 1, 2);
    {
        LaunchTimer tm(eng, st, !dry);
        LAUNCH("cls.head", cls_head_launch(feat.p, eng->cls_fc_w, eng->cls_fc_b, N, feat.w, CLS_FEAT, feat.c, thresh, label, score, flip, logits.p, st));
        tm.done("cls.head", "cls_head_kernel", (double)N * (feat.w * CLS_FEAT + 4.0 * CLS_FEAT), 2.0 * N * feat.w * feat.c);
    }
    tap(eng, "cls.logits", logits);
    return 0;
}

int eng_cls_forward(lumina_ocr* eng, const uint8_t* crops, const int* widths, int N, float thresh, int* label, float* score, int* flip, hipStream_t st) {
    if (!eng->cls_loaded) return locr_fail(eng, "cls_forward", "cls weights not loaded");
    if (N <= 0) return 0;
    LOCR_CHECK(hipSetDevice(eng->device));
    return forward_sub_batched(eng, N, eng->cls_sub_batch < N ? eng->cls_sub_batch : N, [&](int b0, int nb) {
        return cls_forward_sub(eng, crops + (size_t)b0 * CLS_H * CLS_W * 3, widths ? widths + b0 : nullptr, nb, thresh, label + b0, score + b0,
                               flip + b0, st);
    });
}

// ------------------------------------------------------------------------------ SVTR recogniser (Tiny / Base, bf16 / fp16)
static float* upload_f32(lumina_ocr* eng, const std::map<std::string, HostBlobTensor>& m, const std::string& name, int n) {
    auto it = m.find(name);
    if (it == m.end() || it->second.dtype != 0 || (int)it->second.dims[0] != n) { locr_fail(eng, "missing/ill-shaped f32 tensor", name.c_str()); return nullptr; }
    return static_cast<float*>(eng_upload(eng, it->second.data, sizeof(float) * n));
}

// name.w [N][ks][ks][cin] bf16 (+ name.b) -> SvtrLinear with w [N][taps * cin_pad] in the storage type; ln != "" fuses that LayerNorm
static bool make_linear(lumina_ocr* eng, const std::map<std::string, HostBlobTensor>& m, const std::string& name, int ks, int cin, int cin_pad, int N, int act,
                        const std::string& ln, int dtype, bool flat_k, SvtrLinear* L) {
    const HostBlobTensor *w, *b;
    if (!get_wb(eng, m, name, &w, &b)) return false;
    if (w->dims.size() != 4 || w->dims[0] != N || w->dims[1] != ks || w->dims[2] != ks || w->dims[3] != cin || (int)b->dims[0] != N) {
        locr_fail(eng, "unexpected tensor shape", name.c_str());
        return false;
    }
    const int taps = ks * ks;
    const bf16_t* src = reinterpret_cast<const bf16_t*>(w->data);
    // flat_k: the taps * cin real values of a row are packed densely and the ROW is padded to cin_pad (patch embedding 1: 27 -> 32)
    const int K = flat_k ? cin_pad : taps * cin_pad;
    std::vector<uint16_t> packed((size_t)N * K, 0);
    for (int n = 0; n < N; ++n)
        for (int t = 0; t < taps; ++t)
            for (int c = 0; c < cin; ++c)
                packed[(size_t)n * K + (flat_k ? t * cin + c : t * cin_pad + c)] = bf16_bits_to(src[((size_t)n * taps + t) * cin + c], dtype);
    L->K = K; L->N = N; L->taps = flat_k ? 1 : taps; L->cin = cin_pad; L->act = act;
    L->w = static_cast<uint16_t*>(eng_upload(eng, packed.data(), packed.size() * 2));
    L->bias = static_cast<float*>(eng_upload(eng, b->data, sizeof(float) * N));
    if (!ln.empty()) {
        L->gamma = upload_f32(eng, m, ln + ".g", N); L->beta = upload_f32(eng, m, ln + ".b", N);
        if (!L->gamma || !L->beta) return false;
    }
    if (!L->w || !L->bias) { locr_fail(eng, "device upload failed", name.c_str()); return false; }
    return true;
}

int eng_load_svtr(lumina_ocr* eng, const void* blob, size_t n) {
    BlobMap m;
    std::vector<uint64_t> aligned;
    if (!checked_blob(eng, "load_svtr_weights", BLOB_SVTR, blob, n, &aligned, &m)) return 1;
    SvtrConfig cfg;
    BlobError ce;
    if (!blob_svtr_config(m, &cfg, &ce)) return locr_fail(eng, "load_svtr_weights", ce.reason.c_str());   // (check_blob has run it already)
    LOCR_CHECK(hipSetDevice(eng->device));
    SvtrModel& M = eng->svtr;
    M = SvtrModel();   // loaded = false: from here on only an upload can fail; the model then stays unloaded
    {   // variant + storage type, validated by blob_svtr_config before any cast (the tests below are assertions now)
        for (int i = 0; i < 3; ++i) { M.dims[i] = cfg.dims[i]; M.depths[i] = cfg.depths[i]; M.heads[i] = cfg.heads[i]; }
        M.local_blocks = cfg.local_blocks; M.out_ch = cfg.out_ch; M.dtype = cfg.dtype;
        if (eng->svtr_f16 >= 0) M.dtype = eng->svtr_f16;
        for (int i = 0; i < 3; ++i) {
            const int d = M.dims[i];
            if (!(d == 64 || d == 128 || d == 256 || d == 384) || M.heads[i] * 32 != d || M.depths[i] < 1 || M.depths[i] > 32)
                return locr_fail(eng, "svtr.config", "dims must be 64 / 128 / 256 / 384 with 32-wide heads");
        }
        if (M.out_ch != 192 || M.dims[0] > 128) return locr_fail(eng, "svtr.config", "out_channels must be 192 (CTC head K), dims[0] <= 128");
    }
    const int dt = M.dtype, d0 = M.dims[0];
    if (!make_linear(eng, m, "svtr.pe1", 3, 3, 32, d0 / 2, ACT_GELU, "", dt, true, &M.pe1)) return 1;
    if (!make_linear(eng, m, "svtr.pe2", 3, d0 / 2, d0 / 2, d0, ACT_GELU, "", dt, false, &M.pe2)) return 1;
    {
        auto it = m.find("svtr.pos.w");
        if (it == m.end() || it->second.dtype != 1 || it->second.dims.size() != 2 || it->second.dims[0] != 640 || it->second.dims[1] != d0)
            return locr_fail(eng, "svtr.pos", "missing/shape");
        const bf16_t* src = reinterpret_cast<const bf16_t*>(it->second.data);
        std::vector<uint16_t> pos((size_t)640 * d0);
        for (size_t i = 0; i < pos.size(); ++i) pos[i] = bf16_bits_to(src[i], dt);
        M.pos = static_cast<uint16_t*>(eng_upload(eng, pos.data(), pos.size() * 2));
        if (!M.pos) return locr_fail(eng, "upload", "svtr.pos");
    }
    int idx = 0, gh = 8;
    for (int s = 0; s < 3; ++s) {
        const int c = M.dims[s];
        for (int d = 0; d < M.depths[s]; ++d, ++idx) {
            M.blocks.emplace_back();
            SvtrBlock& B = M.blocks.back();
            B.dim = c; B.heads = M.heads[s]; B.gh = gh; B.gw = 80; B.local = idx < M.local_blocks;
            if (B.local && gh % 4 != 0) return locr_fail(eng, "svtr.config", "local mixing blocks need a token grid of at least 4 rows");
            const std::string p = "svtr.b" + std::to_string(idx);
            if (!make_linear(eng, m, p + ".qkv", 1, c, c, 3 * c, ACT_NONE, "", dt, false, &B.qkv)) return 1;
            if (!make_linear(eng, m, p + ".proj", 1, c, c, c, ACT_NONE, p + ".ln1", dt, false, &B.proj)) return 1;
            if (!make_linear(eng, m, p + ".fc1", 1, c, c, 4 * c, ACT_GELU, "", dt, false, &B.fc1)) return 1;
            if (!make_linear(eng, m, p + ".fc2", 1, 4 * c, 4 * c, c, ACT_NONE, p + ".ln2", dt, false, &B.fc2)) return 1;
        }
        if (s < 2) {
            const std::string p = "svtr.sub" + std::to_string(s);
            if (!make_linear(eng, m, p, 3, c, c, M.dims[s + 1], ACT_NONE, p + ".ln", dt, false, &M.sub[s])) return 1;
            gh /= 2;
        }
    }
    if (!make_linear(eng, m, "svtr.last", 1, M.dims[2], M.dims[2], M.out_ch, ACT_HSWISH, "", dt, false, &M.last)) return 1;
    RUN(load_ctc_head(eng, m, "svtr.ctc.fc", M.out_ch, dt, &M.num_classes, &M.ctc_ntiles, &M.ctc_wpk, &M.ctc_bias));
    M.loaded = true;
    return 0;
}

// What a run_linear call asks for beyond a plain linear layer without residual.
struct LinearCall {
    const bf16_t* res = nullptr; int res_mod = 0, res_post = 0;   // SvtrGemmParams: residual [M][N], or a table of res_mod rows added after the activation
    int hin = 1, win = 1, hout = 1, wout = 1, sh = 1, sw = 1;     // gather geometry of a 3x3 conv (1x1: none)
    LinearCall& residual(const bf16_t* r) { res = r; return *this; }
    LinearCall& add_table_after_act(const bf16_t* table, int rows) { res = table; res_mod = rows; res_post = 1; return *this; }
    LinearCall& conv3x3(const Tensor4& in, const Tensor4& out) { hin = in.h; win = in.w; hout = out.h; wout = out.w; sh = in.h / out.h; sw = in.w / out.w; return *this; }
};

// one svtr_gemm launch: y = epi(gather(x) w^T + b)
static int run_linear(lumina_ocr* eng, const SvtrLinear& L, const Tensor4& x, Tensor4* y, hipStream_t st, const LinearCall& c = {}) {
    if (x.p == nullptr || y->p == nullptr) return ws_null(eng, "svtr linear");  // dry run (workspace sizing)
    SvtrGemmParams p{};
    p.x = x.p; p.w = L.w; p.bias = L.bias; p.res = c.res; p.res_mod = c.res_mod; p.res_post = c.res_post; p.gamma = L.gamma; p.beta = L.beta; p.y = y->p;
    p.zeros = zero_block(eng); p.M = (int)(y->elems() / L.N); p.K = L.K; p.N = L.N; p.act = L.act; p.eps = 1e-6f;
    p.taps = L.taps; p.Cin = L.cin; p.Hin = c.hin; p.Win = c.win; p.Tout = c.hout * c.wout; p.Wout = c.wout; p.sh = c.sh; p.sw = c.sw;
    if (!p.zeros) return locr_fail(eng, "svtr", "zero block upload failed");
    if (x.c != L.cin || y->c != L.N) return locr_fail(eng, "svtr linear: channel mismatch", "");
    LaunchTimer tm(eng, st);
    hipError_t e = svtr_gemm_launch(p, eng->svtr.dtype, st);
    if (e != hipSuccess) return locr_fail(eng, "svtr_gemm", hipGetErrorString(e));
    // algorithmic bytes: the input tensor, the weights, the result and the residual once (a 9-tap gather re-reads its input from cache)
    tm.done("svtr.linear", svtr_gemm_kernel_name(p, eng->svtr.dtype), 2.0 * p.M * p.K * p.N,
            2.0 * ((double)x.elems() + (double)p.N * p.K + (double)p.M * p.N + (c.res && c.res_mod == 0 ? (double)p.M * p.N : 0.0)));
    return 0;
}

static int svtr_forward_sub(lumina_ocr* eng, const uint8_t* crops, const int* widths, int N, int* idx, float* prob, hipStream_t st) {
    const bool dry = eng->arena.counting();
    SvtrModel& M = eng->svtr;
    const int T = 80, dt = M.dtype, d0 = M.dims[0];
    Tensor4 patches = ws_tensor(eng, N, 16, 160, 32);
    LAUNCH("svtr.im2col", svtr_im2col_launch(crops, widths, patches.p, N, dt, st));
    Tensor4 e1 = ws_tensor(eng, N, 16, 160, d0 / 2);
    RUN(run_linear(eng, M.pe1, patches, &e1, st));
    Tensor4 x = ws_tensor(eng, N, 8, 80, d0);   // patch embedding 2 (3x3 / s2, GELU, rounded) + positional embedding (rounded again)
    RUN(run_linear(eng, M.pe2, e1, &x, st, LinearCall().conv3x3(e1, x).add_table_after_act(M.pos, 640)));
    tap(eng, "svtr.embed", x);
    int stage = 0;
    for (size_t bi = 0; bi < M.blocks.size(); ++bi) {
        SvtrBlock& B = M.blocks[bi];
        const int want_stage = (int)bi < M.depths[0] ? 0 : ((int)bi < M.depths[0] + M.depths[1] ? 1 : 2);
        if (want_stage != stage) {
            // height merging: 3x3 conv, stride (2, 1), + LayerNorm (fused epilogue)
            Tensor4 y = ws_tensor(eng, N, x.h / 2, x.w, M.dims[stage + 1]);
            RUN(run_linear(eng, M.sub[stage], x, &y, st, LinearCall().conv3x3(x, y)));
            tap(eng, stage == 0 ? "svtr.sub0" : "svtr.sub1", y);
            x = y; ++stage;
        }
        const int Tk = x.h * x.w, c = B.dim;
        Tensor4 qkv = ws_tensor(eng, N, x.h, x.w, 3 * c);
        RUN(run_linear(eng, B.qkv, x, &qkv, st));
        Tensor4 att = ws_tensor(eng, N, x.h, x.w, c);
        {
            LaunchTimer tm(eng, st, !dry);
            LAUNCH("svtr.attn", svtr_attention_launch(qkv.p, att.p, N, Tk, B.heads, B.gh, B.gw, B.local ? 1 : 0, dt, st));
            const double keys = B.local ? 77.0 : (double)Tk;   // keys a query attends (7 x 11 window / all)
            tm.done("svtr.attn", std::string("svtr_attn_kernel<") + (dt ? "1>" : "0>"), 4.0 * N * Tk * keys * c, 2.0 * N * Tk * 4.0 * c);
        }
        Tensor4 x1 = ws_tensor(eng, N, x.h, x.w, c);
        RUN(run_linear(eng, B.proj, att, &x1, st, LinearCall().residual(x.p)));   // + residual, LayerNorm 1
        Tensor4 f1 = ws_tensor(eng, N, x.h, x.w, 4 * c);
        RUN(run_linear(eng, B.fc1, x1, &f1, st));
        Tensor4 x2 = ws_tensor(eng, N, x.h, x.w, c);
        RUN(run_linear(eng, B.fc2, f1, &x2, st, LinearCall().residual(x1.p)));   // + residual, LayerNorm 2
        tap(eng, ("svtr.b" + std::to_string(bi)).c_str(), x2);
        x = x2;
    }
    Tensor4 pooled = ws_tensor(eng, N, 1, T, M.dims[2]);
    LAUNCH("svtr.pool", svtr_rowmean_launch(x.p, pooled.p, N, x.h, x.w, M.dims[2], dt, st));
    Tensor4 seq = ws_tensor(eng, N, 1, T, M.out_ch);
    RUN(run_linear(eng, M.last, pooled, &seq, st));
    tap(eng, "svtr.seq", seq);
    if (!dry) {
        CtcFcParams cp{};
        cp.seq = seq.p; cp.wpk = M.ctc_wpk; cp.bias = M.ctc_bias; cp.out_idx = idx; cp.out_prob = prob;
        cp.M = N * T; cp.K = M.out_ch; cp.C = M.num_classes; cp.ntiles = M.ctc_ntiles; cp.f16 = dt;
        LaunchTimer tm(eng, st);
        LAUNCH("svtr ctc_fc_argmax", ctc_fc_argmax_launch(cp, st));
        tm.done("svtr.ctc.fc+argmax", std::string("ctc_fc_argmax_kernel<") + (dt ? "1>" : "0>"), 2.0 * cp.M * cp.K * cp.C, 2.0 * cp.M * cp.K + 8.0 * cp.M + 2.0 * cp.K * cp.C);
    }
    return 0;
}

int eng_svtr_forward(lumina_ocr* eng, const uint8_t* crops, const int* widths, int N, int* idx, float* prob, hipStream_t st) {
    if (!eng->svtr.loaded) return locr_fail(eng, "svtr_forward", "SVTR weights not loaded");
    if (N <= 0) return 0;
    LOCR_CHECK(hipSetDevice(eng->device));
    int sb = eng->rec_sub_batch / (eng->svtr.dims[2] > 256 ? 4 : 2);   // ~3 MB (Tiny) / ~7 MB (Base) of activations per crop
    if (sb < 1) sb = 1;
    if (sb > N) sb = N;
    return forward_sub_batched(eng, N, sb, [&](int b0, int nb) {
        return svtr_forward_sub(eng, crops + (size_t)b0 * 32 * 320 * 3, widths ? widths + b0 : nullptr, nb, idx + (size_t)b0 * 80, prob + (size_t)b0 * 80, st);
    });
}
