// The LOCW weight container, host only (no device header: tests/blob_main.cpp compiles this file with the host compiler alone).
//   blob_parse  : bytes -> name -> (dtype, dims, data pointer); reads every field through memcpy, so the blob may lie at any address
//   blob_spec   : the tensors the loader of one model reads, written from the loaders' own constants (engine.hip uses the same ones)
//   check_blob  : every tensor of that list present once, with that dtype, rank and every dimension; byte count = dims x element size
// Every eng_load_* runs blob_parse + check_blob before it writes one engine field or uploads one byte, and afterwards reads only
// extents that check_blob has proved.  tests/blob_reference.py restates the rule from the shapes of arch.make_*_weights;
// tests/test_blob_check_sanitized.py holds this file to it, mutant by mutant.
//
// Choices (stated in include/lumina_ocr.h as well):
//   - tensors the loader does not read are ignored; a name that occurs twice is refused, whether the loader reads it or not;
//   - bytes after the last tensor are refused ("trailing bytes"): a count field that is too small would otherwise drop tensors unseen;
//   - a blob at an address that is no multiple of 16 is loaded correctly: the parser assumes no alignment, and the loader, which reads
//     bf16 / f32 arrays in place, first copies such a blob to aligned storage (blob_realign).
//
// CTC class count C (ctc.fc.w / svtr.ctc.fc.w dims[0]): BLOB_CTC_MIN_CLASSES <= C <= BLOB_CTC_MAX_CLASSES.
//   - lower bound 2: class 0 is the blank that ctc_collapse_row (ops.hip) drops, so a head needs one more class to emit anything;
//     ctc_fc_argmax_launch (ops.hip) itself refuses ntiles < 1.
//   - upper bound 65536: ctc_fc_argmax_kernel (ops.hip) walks ntiles = ceil(C / CT_BN) tiles of CT_BN = 64 classes with int tile and
//     class indices (run_i = t * CT_BN + ti) and size_t addresses, so its arithmetic holds far beyond this; the bound is what the loader
//     is willing to stage on the host (C x 192 bf16, twice) on the word of one header field, and is 3.5 times the largest published
//     PP-OCR dictionary (18 383 classes).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

struct HostBlobTensor { int dtype; std::vector<int> dims; const uint8_t* data; size_t nbytes; };
typedef std::map<std::string, HostBlobTensor> BlobMap;

struct BlobError { std::string reason, tensor; };   // tensor: "" where no tensor can be named (container header, a cut inside a name)

enum BlobKind { BLOB_DET = 0, BLOB_REC = 1, BLOB_CLS = 2, BLOB_SVTR = 3 };
constexpr int BLOB_F32 = 0, BLOB_BF16 = 1;
constexpr int BLOB_CTC_MIN_CLASSES = 2, BLOB_CTC_MAX_CLASSES = 65536;
constexpr int BLOB_CLASSES = -1;   // a BlobSpec dimension: the model's CTC class count (the head's weight and bias must agree on it)
constexpr int LSTM_HIDDEN = 96, REC_FEAT = 288, CTC_K = 192, CLS_FEAT = 200;   // arch.REC_HIDDEN, REC_FEAT, SVTR_OUT = 2 * REC_HIDDEN, CLS_FEAT
constexpr int DET_STAGE_CH[4] = {64, 128, 256, 512}, DET_FPN_CH = 256;

struct BlobSpec { std::string name; int dtype; std::vector<int> dims; bool required; };

static inline bool blob_fail(BlobError* e, const char* reason, const std::string& tensor) {
    if (e) { e->reason = reason; e->tensor = tensor; }
    return false;
}

inline bool blob_parse(const void* blob, size_t n, BlobMap* out, BlobError* err) {
    const uint8_t* b = static_cast<const uint8_t*>(blob);
    if (n < 12 || memcmp(b, "LOCW", 4) != 0) return blob_fail(err, "bad magic", "");
    uint32_t ver, cnt;
    memcpy(&ver, b + 4, 4); memcpy(&cnt, b + 8, 4);
    if (ver != 1) return blob_fail(err, "unsupported version", "");
    size_t off = 12;
    for (uint32_t i = 0; i < cnt; ++i) {
        if (n - off < 2) return blob_fail(err, "truncated", "");
        uint16_t ln; memcpy(&ln, b + off, 2); off += 2;
        if (n - off < (size_t)ln + 2) return blob_fail(err, "truncated", "");
        const std::string name(reinterpret_cast<const char*>(b + off), ln); off += ln;
        HostBlobTensor t;
        t.dtype = b[off]; const int nd = b[off + 1]; off += 2;
        if (t.dtype > 1) return blob_fail(err, "unknown dtype", name);
        if (nd < 1 || nd > 4) return blob_fail(err, "rank out of range", name);
        if (n - off < 4 * (size_t)nd + 8) return blob_fail(err, "truncated", name);
        uint64_t count = 1;
        for (int d = 0; d < nd; ++d) {
            uint32_t v; memcpy(&v, b + off, 4); off += 4;
            if (v == 0 || v > (1u << 28) || count * v > (1ull << 34)) return blob_fail(err, "implausible dimension", name);
            count *= v; t.dims.push_back((int)v);
        }
        uint64_t nb; memcpy(&nb, b + off, 8); off += 8;
        off += (16 - off % 16) % 16;
        if (nb != count * (t.dtype ? 2u : 4u)) return blob_fail(err, "byte count does not match the dimensions", name);
        if (off > n || nb > n - off) return blob_fail(err, "truncated data", name);   // (off + nb could wrap)
        t.data = b + off; t.nbytes = (size_t)nb; off += (size_t)nb;
        if (!out->emplace(name, t).second) return blob_fail(err, "duplicate tensor name", name);
    }
    if (off != n) return blob_fail(err, "trailing bytes", "");
    return true;
}

// ---- the loaders' constants ----
static inline int cp16(int c) { return (c + 15) / 16 * 16; }
static inline int make_div(double v, int d = 8) {   // arch._make_div
    int nv = (int)(v + d / 2.0) / d * d;
    if (nv < d) nv = d;
    if (nv < 0.9 * v) nv += d;
    return nv;
}
// MobileNetV3-small (arch._MV3_SMALL): kernel, expanded channels, output channels, squeeze-excite, hard-swish (else ReLU)
struct Mv3Row { int k, exp, c; bool se, hswish; };
constexpr Mv3Row MV3_ROWS[11] = {{3, 16, 16, true, false},  {3, 72, 24, false, false}, {3, 88, 24, false, false}, {5, 96, 40, true, true},
                                 {5, 240, 40, true, true},  {5, 240, 40, true, true},  {5, 120, 48, true, true},  {5, 144, 48, true, true},
                                 {5, 288, 96, true, true},  {5, 576, 96, true, true},  {5, 576, 96, true, true}};
constexpr double REC_SCALE = 0.5, CLS_SCALE = 0.35;
constexpr int REC_STRIDES[11] = {1, 2, 1, 2, 1, 1, 1, 1, 2, 1, 1}, CLS_STRIDES[11] = {2, 2, 1, 2, 1, 1, 1, 1, 2, 1, 1};

// svtr.config, validated: blob_svtr_config fills it (the SVTR-Tiny defaults where the blob has no svtr.config)
struct SvtrConfig { int dims[3] = {64, 128, 256}, depths[3] = {3, 6, 3}, heads[3] = {2, 4, 8}, local_blocks = 6, out_ch = CTC_K, dtype = 0; };

// Every value finite and integral before it is cast; dims 64 / 128 / 256 / 384 with 32-wide heads, dims[0] <= 128, depths 1 .. 32,
// out_channels 192, dtype 0 / 1, and 0 <= local_blocks <= depths[0] + depths[1] (a local block needs a token grid of at least 4 rows,
// which stage 2, 2 x 80 tokens, does not have).
inline bool blob_svtr_config(const BlobMap& m, SvtrConfig* cfg, BlobError* err) {
    *cfg = SvtrConfig();
    const auto it = m.find("svtr.config");
    if (it == m.end()) return true;
    const HostBlobTensor& t = it->second;
    if (t.dtype != BLOB_F32) return blob_fail(err, "wrong dtype", "svtr.config");
    if (t.dims.size() != 1) return blob_fail(err, "wrong rank", "svtr.config");
    if (t.dims[0] != 12 || t.nbytes != 48) return blob_fail(err, "wrong dimension", "svtr.config");
    int v[12];
    for (int i = 0; i < 12; ++i) {
        float f; memcpy(&f, t.data + 4 * i, 4);
        if (!std::isfinite(f) || f < 0.f || f > 65536.f || f != std::floor(f)) return blob_fail(err, "svtr.config value not a small whole number", "svtr.config");
        v[i] = (int)f;
    }
    for (int i = 0; i < 3; ++i) {
        cfg->dims[i] = v[i]; cfg->depths[i] = v[3 + i]; cfg->heads[i] = v[6 + i];
        const int d = v[i];
        if (!(d == 64 || d == 128 || d == 256 || d == 384) || cfg->heads[i] * 32 != d || cfg->depths[i] < 1 || cfg->depths[i] > 32)
            return blob_fail(err, "svtr.config out of range (dims 64 / 128 / 256 / 384 with 32-wide heads, depths 1 .. 32)", "svtr.config");
    }
    cfg->local_blocks = v[9]; cfg->out_ch = v[10]; cfg->dtype = v[11];
    if (cfg->out_ch != CTC_K || cfg->dims[0] > 128) return blob_fail(err, "svtr.config out of range (out_channels 192, dims[0] <= 128)", "svtr.config");
    if (cfg->local_blocks > cfg->depths[0] + cfg->depths[1]) return blob_fail(err, "svtr.config out of range (local blocks past stage 1)", "svtr.config");
    if (cfg->dtype > 1) return blob_fail(err, "svtr.config out of range (dtype 0 / 1)", "svtr.config");
    return true;
}

struct BlobSpecList {
    std::vector<BlobSpec> v;
    void add(const std::string& name, int dtype, std::vector<int> dims, bool required = true) { v.push_back(BlobSpec{name, dtype, std::move(dims), required}); }
    // name.w [cout][ks][ks][cin] bf16 + name.b [nbias] f32 (OHWI: what make_conv, make_dw, make_se, load_stem and make_linear read)
    void conv(const std::string& name, int cout, int ks, int cin, int nbias = 0) {
        add(name + ".w", BLOB_BF16, {cout, ks, ks, cin});
        add(name + ".b", BLOB_F32, {nbias ? nbias : cout});
    }
    void layer_norm(const std::string& name, int c) { add(name + ".g", BLOB_F32, {c}); add(name + ".b", BLOB_F32, {c}); }
    void ctc(const std::string& name) { add(name + ".w", BLOB_BF16, {BLOB_CLASSES, CTC_K}); add(name + ".b", BLOB_F32, {BLOB_CLASSES}); }
    int mv3(const std::string& prefix, double scale) {   // load_stem + load_mv3_blocks -> channels after block 10
        int cin = make_div(16 * scale);
        conv(prefix + ".conv1", cin, 3, 3);
        for (int i = 0; i < 11; ++i) {
            const int exp = make_div(MV3_ROWS[i].exp * scale), cout = make_div(MV3_ROWS[i].c * scale), k = MV3_ROWS[i].k;
            const std::string p = prefix + ".b" + std::to_string(i);
            conv(p + ".expand", exp, 1, cin);
            conv(p + ".dw", exp, k, 1);
            if (MV3_ROWS[i].se) { conv(p + ".se1", exp / 4, 1, exp); conv(p + ".se2", exp, 1, exp / 4); }
            conv(p + ".project", cout, 1, exp);
            cin = cout;
        }
        return cin;
    }
};

// The tensors eng_load_<kind> reads.  SVTR: from the blob's own (validated) svtr.config.
inline bool blob_spec(BlobKind kind, const BlobMap& m, std::vector<BlobSpec>* out, BlobError* err) {
    BlobSpecList L;
    if (kind == BLOB_DET) {
        L.conv("stem.conv1", 32, 3, 3); L.conv("stem.conv2", 32, 3, 32); L.conv("stem.conv3", 64, 3, 32);
        int cin = 64;
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 2; ++j) {
                const std::string p = "s" + std::to_string(i) + ".b" + std::to_string(j);
                const int c = DET_STAGE_CH[i];
                L.conv(p + ".conv0", c, 3, cin);
                L.conv(p + ".conv1", c, 3, c);
                if (j == 0) L.conv(p + ".short", c, i == 0 ? 1 : 2, cin);
                cin = c;
            }
        for (int l = 5; l >= 2; --l) {
            L.conv("fpn.in" + std::to_string(l), DET_FPN_CH, 1, DET_STAGE_CH[l - 2]);
            L.conv("fpn.p" + std::to_string(l), 64, 3, DET_FPN_CH);
        }
        L.conv("head.conv1", 64, 3, 256);
        L.conv("head.convt2", 256, 1, 64, 64);   // transposed 2x2: [4 taps x 64][1][1][64], one bias per output channel
        L.conv("head.convt3", 4, 1, 64, 1);
    } else if (kind == BLOB_REC) {
        const int cin = L.mv3("rec", REC_SCALE);
        L.conv("rec.conv2", REC_FEAT, 1, cin);
        for (int l = 0; l < 2; ++l)
            for (const char* dir : {"fw", "bw"}) {
                const std::string p = "lstm.l" + std::to_string(l) + "." + dir;
                L.add(p + ".w_ih", BLOB_BF16, {4 * LSTM_HIDDEN, l == 0 ? REC_FEAT : 2 * LSTM_HIDDEN});
                L.add(p + ".w_hh", BLOB_BF16, {4 * LSTM_HIDDEN, LSTM_HIDDEN});
                L.add(p + ".b", BLOB_F32, {4 * LSTM_HIDDEN});
            }
        L.ctc("ctc.fc");
    } else if (kind == BLOB_CLS) {
        const int cin = L.mv3("cls", CLS_SCALE);
        L.conv("cls.conv2", CLS_FEAT, 1, cin);
        L.add("cls.fc.w", BLOB_BF16, {2, CLS_FEAT});
        L.add("cls.fc.b", BLOB_F32, {2});
    } else {
        SvtrConfig c;
        if (!blob_svtr_config(m, &c, err)) return false;
        L.add("svtr.config", BLOB_F32, {12}, false);
        L.conv("svtr.pe1", c.dims[0] / 2, 3, 3);
        L.conv("svtr.pe2", c.dims[0], 3, c.dims[0] / 2);
        L.add("svtr.pos.w", BLOB_BF16, {640, c.dims[0]});
        int idx = 0;
        for (int s = 0; s < 3; ++s) {
            const int d = c.dims[s];
            for (int k = 0; k < c.depths[s]; ++k, ++idx) {
                const std::string p = "svtr.b" + std::to_string(idx);
                L.conv(p + ".qkv", 3 * d, 1, d);
                L.conv(p + ".proj", d, 1, d);
                L.layer_norm(p + ".ln1", d);
                L.conv(p + ".fc1", 4 * d, 1, d);
                L.conv(p + ".fc2", d, 1, 4 * d);
                L.layer_norm(p + ".ln2", d);
            }
            if (s < 2) {
                const std::string p = "svtr.sub" + std::to_string(s);
                L.conv(p, c.dims[s + 1], 3, d);
                L.layer_norm(p + ".ln", c.dims[s + 1]);
            }
        }
        L.conv("svtr.last", c.out_ch, 1, c.dims[2]);
        L.ctc("svtr.ctc.fc");
    }
    *out = std::move(L.v);
    return true;
}

// true, or false with the reason and the tensor: where several tensors are wrong, the one whose name sorts first.
inline bool check_blob(BlobKind kind, const BlobMap& m, BlobError* err) {
    std::vector<BlobSpec> spec;
    if (!blob_spec(kind, m, &spec, err)) return false;
    BlobError first;
    bool ok = true;
    auto fail = [&](const char* reason, const std::string& name) {
        if (ok || name < first.tensor) { first.reason = reason; first.tensor = name; }
        ok = false;
    };
    int classes = 0;   // of the first CTC tensor that states one
    for (const BlobSpec& s : spec) {
        const auto it = m.find(s.name);
        if (it == m.end()) {
            if (s.required) fail("missing tensor", s.name);
            continue;
        }
        const HostBlobTensor& t = it->second;
        if (t.dtype != s.dtype) { fail("wrong dtype", s.name); continue; }
        if (t.dims.size() != s.dims.size()) { fail("wrong rank", s.name); continue; }
        uint64_t count = 1;
        bool dims_ok = true;
        for (size_t d = 0; d < s.dims.size() && dims_ok; ++d) {
            int want = s.dims[d];
            if (want == BLOB_CLASSES) {
                if (t.dims[d] < BLOB_CTC_MIN_CLASSES || t.dims[d] > BLOB_CTC_MAX_CLASSES) { fail("class count out of range", s.name); dims_ok = false; break; }
                if (classes == 0) classes = t.dims[d];
                want = classes;
            }
            if (t.dims[d] != want) { fail("wrong dimension", s.name); dims_ok = false; }
            count *= (uint64_t)t.dims[d];
        }
        if (dims_ok && t.nbytes != count * (t.dtype ? 2u : 4u)) fail("byte count does not match the dimensions", s.name);
    }
    if (!ok) return blob_fail(err, first.reason.c_str(), first.tensor);
    return true;
}

// The blob at a 16-byte aligned address: itself, or a copy in `storage` (its data offsets are multiples of 16 from the blob's start,
// so every bf16 / f32 array of an aligned blob can be read in place).
inline const void* blob_realign(const void* blob, size_t n, std::vector<uint64_t>* storage) {
    if (reinterpret_cast<uintptr_t>(blob) % 16 == 0) return blob;
    storage->assign(n / 8 + 2, 0);
    uint8_t* p = reinterpret_cast<uint8_t*>(storage->data());
    p += (16 - reinterpret_cast<uintptr_t>(p) % 16) % 16;
    memcpy(p, blob, n);
    return p;
}
