// Lossless WebP (VP8L) decoder on the device (webpdec.h): what the reference's Image.open(...).convert('RGB') does for lossless .webp
// inputs, byte-identical to Pillow.
//
// The container walk (webp_parse.h: a few dozen bytes of chunk headers) is host code; it gathers each file's VP8L payload into one pinned
// staging buffer.  The device then runs, per sub-batch:
//   1. wp_entropy: one wave64 work-group per file runs wp_decode_stream (webp_dec.h): transform headers, the sub-resolution images, the
//      prefix codes of every group, and the walk of the ARGB stream into a u32 plane.  All decode state is wave-uniform; the bit reader
//      keeps 32..64 bits in registers; the code lengths, the code-length code, the colour cache and the current group's five first-level
//      tables sit in LDS, the groups' full codes in the workspace.  Backward references are copied by all 64 lanes (lane k copies
//      src + k mod distance) and the lanes insert the copied pixels into the colour cache, the later pixel winning a slot;
//   2. the inverse transforms, last to first, each its own kernel over all files, launched once per position a transform can take:
//      wp_palette (packed indices -> colours, into the file's second plane), wp_green, wp_cross (element-wise, in place) and
//      wp_predictor: bands of 64 rows as a skewed wavefront, lane i owns row band * 64 + i and runs two pixels behind lane i - 1, so
//      top-left, top and top-right come from lane i - 1 by cross-lane moves and left from the lane's own last step; row 63 of a band
//      is handed to the next band through LDS;
//   3. wp_rgb: ARGB words -> RGB u8, every output byte written once.
// A file whose stream breaks any rule (webp_dec.h) ends with err != 0 in its WpHead and is not written.
#include "webpdec.h"

#include <algorithm>
#include <cstring>
#include <vector>

#include "engine.h"
#include "webp_dec.h"
#include "webp_parse.h"

namespace {

constexpr int WP_MAX_ROW = 16384;   // the longest row the format has: the predictor's LDS hand-over row

struct WpFile {
    unsigned long long zoff;   // byte offset of the VP8L payload in the sub-batch's stream buffer (a multiple of 16)
    unsigned zlen;
    int valid, out_index;
};

__global__ __launch_bounds__(64) void wp_entropy(const WpFile* __restrict__ F, const uint8_t* __restrict__ z, uint32_t* __restrict__ planes,
                                                 uint32_t* __restrict__ sub, uint16_t* __restrict__ tab, WpHead* __restrict__ heads, int W, int H,
                                                 size_t plane_words, size_t sub_words) {
    __shared__ uint32_t cache[1 << WP_MAX_CACHE_BITS], stamp[1 << WP_MAX_CACHE_BITS];
    __shared__ uint16_t gfast[5 << WP_FAST], cl[WP_CL_WORDS + 1];
    __shared__ uint8_t lens[WP_LENS];
    const int k = blockIdx.x;
    const WpFile f = F[k];
    if (!f.valid) {
        if (threadIdx.x == 0) { heads[k].err = -1; heads[k].ntrans = 0; heads[k].width = W; }
        return;
    }
    WpCtx c;
    wp_bits_init(c.b, z + f.zoff, f.zlen, 5);   // the five header bytes were read by the host
    c.err = 0;
    c.lens = lens; c.cache = cache; c.stamp = stamp; c.cl = cl; c.gfast = gfast;
    c.tab = tab + (size_t)k * WP_TABLE_WORDS;
    c.sub = sub + (size_t)k * sub_words; c.sub_cap = (uint32_t)sub_words; c.sub_used = 0;
    wp_decode_stream(c, W, H, planes + (size_t)k * 2 * plane_words, &heads[k]);
}

// the transform a stage-2 launch of position `step` (0: the last in the stream) undoes for this file, or null; *second: the image is
// in the file's second plane (a palette has been undone before)
__device__ const WpTrans* wp_step(const WpFile& f, const WpHead& h, int step, int type, bool* second) {
    if (!f.valid || h.err) return nullptr;
    const int k = h.ntrans - 1 - step;
    if (k < 0 || h.t[k].type != type) return nullptr;
    bool s = false;
    for (int j = k + 1; j < h.ntrans; ++j) s |= h.t[j].type == WP_PALETTE;
    *second = s;
    return &h.t[k];
}

__global__ __launch_bounds__(256) void wp_palette(const WpFile* __restrict__ F, const WpHead* __restrict__ heads, uint32_t* __restrict__ planes,
                                                  const uint32_t* __restrict__ sub, int H, size_t plane_words, size_t sub_words, int step) {
    const int k = blockIdx.y;
    bool second;
    const WpTrans* T = wp_step(F[k], heads[k], step, WP_PALETTE, &second);
    if (!T) return;
    const int tw = T->width, pw = wp_subsize(tw, T->bits);
    const uint32_t* src = planes + (size_t)k * 2 * plane_words;
    uint32_t* dst = planes + (size_t)k * 2 * plane_words + plane_words;
    const uint32_t* pal = sub + (size_t)k * sub_words + T->sub;
    const size_t n = (size_t)tw * H;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256) {
        const int y = (int)(p / tw), x = (int)(p - (size_t)y * tw);
        dst[p] = wp_palette_px(src + (size_t)y * pw, x, T->bits, pal, T->count);
    }
}

__global__ __launch_bounds__(256) void wp_green(const WpFile* __restrict__ F, const WpHead* __restrict__ heads, uint32_t* __restrict__ planes, int H,
                                                size_t plane_words, int step) {
    const int k = blockIdx.y;
    bool second;
    const WpTrans* T = wp_step(F[k], heads[k], step, WP_GREEN, &second);
    if (!T) return;
    uint32_t* d = planes + (size_t)k * 2 * plane_words + (second ? plane_words : 0);
    const size_t n = (size_t)T->width * H;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256) d[p] = wp_green_px(d[p]);
}

__global__ __launch_bounds__(256) void wp_cross(const WpFile* __restrict__ F, const WpHead* __restrict__ heads, uint32_t* __restrict__ planes,
                                                const uint32_t* __restrict__ sub, int H, size_t plane_words, size_t sub_words, int step) {
    const int k = blockIdx.y;
    bool second;
    const WpTrans* T = wp_step(F[k], heads[k], step, WP_CROSS, &second);
    if (!T) return;
    uint32_t* d = planes + (size_t)k * 2 * plane_words + (second ? plane_words : 0);
    const uint32_t* m = sub + (size_t)k * sub_words + T->sub;
    const int tw = T->width, bits = T->bits, sw = wp_subsize(tw, bits);
    const size_t n = (size_t)tw * H;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256) {
        const int y = (int)(p / tw), x = (int)(p - (size_t)y * tw);
        d[p] = wp_cross_px(m[(size_t)(y >> bits) * sw + (x >> bits)], d[p]);
    }
}

__global__ __launch_bounds__(64) void wp_predictor(const WpFile* __restrict__ F, const WpHead* __restrict__ heads, uint32_t* __restrict__ planes,
                                                   const uint32_t* __restrict__ sub, int H, size_t plane_words, size_t sub_words, int step) {
    __shared__ uint32_t prevrow[WP_MAX_ROW];
    const int k = blockIdx.x;
    bool second;
    const WpTrans* T = wp_step(F[k], heads[k], step, WP_PREDICTOR, &second);
    if (!T) return;
    uint32_t* d = planes + (size_t)k * 2 * plane_words + (second ? plane_words : 0);
    const uint32_t* m = sub + (size_t)k * sub_words + T->sub;
    const int tw = T->width, bits = T->bits, sw = wp_subsize(tw, bits);
    const int lane = threadIdx.x;
    for (int band = 0; band * 64 < H; ++band) {
        const int r = band * 64 + lane;
        const bool rowok = r < H;
        uint32_t* row = d + (size_t)(rowok ? r : 0) * tw;
        const uint32_t* mrow = m + (size_t)((rowok ? r : 0) >> bits) * sw;
        uint32_t h1 = 0, h2 = 0, h3 = 0, left = 0, first = 0;   // h1..h3: this lane's last three outputs, the most recent first
        const int steps = tw + 2 * 63;
        for (int t = 0; t < steps; ++t) {
            const int x = t - 2 * lane;
            const bool act = rowok && x >= 0 && x < tw;
            // lane i - 1 stands two pixels ahead: its outputs of one, two and three steps ago are top-right, top and top-left
            uint32_t tr = (uint32_t)__shfl_up((int)h1, 1, 64), tp = (uint32_t)__shfl_up((int)h2, 1, 64), tl = (uint32_t)__shfl_up((int)h3, 1, 64);
            if (lane == 0 && band > 0 && act) {
                tp = prevrow[x];
                tl = x > 0 ? prevrow[x - 1] : 0u;
                tr = x + 1 < tw ? prevrow[x + 1] : 0u;
            }
            uint32_t o = 0;
            if (act) {
                uint32_t pred;
                if (r == 0) pred = x == 0 ? 0xFF000000u : left;
                else if (x == 0) pred = tp;
                else {
                    if (x == tw - 1) tr = first;   // the pixel after the row above's last one in memory: this row's first
                    pred = wp_predict((int)((mrow[x >> bits] >> 8) & 15u), left, tp, tl, tr);
                }
                o = wp_add(row[x], pred);
                row[x] = o;
                if (x == 0) first = o;
                left = o;
                if (lane == 63) prevrow[x] = o;   // (lane 0 reads positions 126 steps ahead of this one)
            }
            h3 = h2; h2 = h1; h1 = o;
        }
        __syncthreads();   // prevrow (row 63 of this band) -> lane 0 of the next band
    }
}

__global__ __launch_bounds__(256) void wp_rgb(const WpFile* __restrict__ F, const WpHead* __restrict__ heads, const uint32_t* __restrict__ planes,
                                              uint8_t* __restrict__ out, int W, int H, size_t plane_words) {
    const int k = blockIdx.y;
    const WpFile f = F[k];
    const WpHead& h = heads[k];
    if (!f.valid || h.err) return;
    bool second = false;
    for (int j = 0; j < h.ntrans; ++j) second |= h.t[j].type == WP_PALETTE;
    const uint32_t* d = planes + (size_t)k * 2 * plane_words + (second ? plane_words : 0);
    uint8_t* o = out + (size_t)f.out_index * H * W * 3;
    const size_t n = (size_t)W * H;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256) {
        const uint32_t v = d[p];
        o[3 * p] = (uint8_t)(v >> 16); o[3 * p + 1] = (uint8_t)(v >> 8); o[3 * p + 2] = (uint8_t)v;
    }
}

struct WpWorkspace { WpFile* F; WpHead* heads; uint8_t* z; uint32_t *planes, *sub; uint16_t* tab; };
size_t wp_plane_words(int height, int width) { return (((size_t)height * width) + 63) & ~(size_t)63; }
WpWorkspace wp_layout(Arena& a, int n, int height, int width, size_t z_total) {
    WpWorkspace w;
    w.F = a.take<WpFile>(n); w.heads = a.take<WpHead>(n); w.z = a.take<uint8_t>(z_total);
    w.planes = a.take<uint32_t>((size_t)n * 2 * wp_plane_words(height, width));
    w.sub = a.take<uint32_t>((size_t)n * wp_sub_words(width, height));
    w.tab = a.take<uint16_t>((size_t)n * WP_TABLE_WORDS);
    return w;
}

}  // namespace

size_t webpdec_workspace_bytes(int n, int height, int width, size_t z_total) {
    Arena a;
    wp_layout(a, n, height, width, z_total);
    return a.off;
}

int webpdec_run(lumina_ocr* eng, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev, int* status,
                hipStream_t st) {
    std::vector<WpInfo> I((size_t)n);
    for (int i = 0; i < n; ++i) {
        int rc = files[i] ? webp_probe(files[i], sizes[i], &I[(size_t)i]) : -1;
        if (rc == 0 && (I[(size_t)i].width != width || I[(size_t)i].height != height)) rc = -4;
        status[i] = rc;
    }
    if (width > WP_MAX_ROW || (long long)width * height > WP_MAX_PIXELS) {   // (no file of such a size has status 0)
        for (int i = 0; i < n; ++i)
            if (status[i] == 0) status[i] = -2;
        return 0;
    }
    lumina_ocr::Staging& stage = eng->wp_stage;
    if (!stage.uploaded) {
        hipEvent_t ev = nullptr;
        LOCR_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        stage.uploaded.reset(ev);
    }
    // sub-batches of at most eng->wp_sub_batch_mb MB of planes, sub-resolution images and code tables (at least one file each)
    const size_t pw = wp_plane_words(height, width), sw = wp_sub_words(width, height);
    const size_t per_file = 2 * pw * 4 + sw * 4 + WP_TABLE_WORDS * 2;
    const int per_batch = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)eng->wp_sub_batch_mb << 20) / per_file));
    for (int i0 = 0; i0 < n; i0 += per_batch) {
        const int nb = std::min(per_batch, n - i0);
        std::vector<WpFile> F((size_t)nb);
        size_t z_total = 0;
        int any = 0;
        for (int k = 0; k < nb; ++k) {
            WpFile& f = F[(size_t)k];
            memset(&f, 0, sizeof(f));
            const int i = i0 + k;
            if (status[i] != 0) continue;
            f.valid = 1; ++any;
            f.out_index = i;
            f.zlen = (unsigned)I[(size_t)i].len;
            f.zoff = z_total; z_total += (I[(size_t)i].len + 15 + 16) & ~(size_t)15;
        }
        if (!any) continue;
        LOCR_CHECK(hipEventSynchronize(stage.uploaded.get()));
        LOCR_CHECK(stage.buf.reserve(z_total, stage.uploaded.get()));
        uint8_t* zs = stage.buf.get();
        for (int k = 0; k < nb; ++k) {
            const WpFile& f = F[(size_t)k];
            if (!f.valid) continue;
            const WpInfo& info = I[(size_t)(i0 + k)];
            memcpy(zs + f.zoff, files[i0 + k] + info.off, info.len);
            memset(zs + f.zoff + info.len, 0, ((info.len + 15 + 16) & ~(size_t)15) - info.len);
        }
        Arena sizing;
        wp_layout(sizing, nb, height, width, z_total);
        if (eng_ws_reserve(eng, sizing.off)) return 1;
        Arena a(eng->ws.get(), eng->ws.cap);
        const WpWorkspace w = wp_layout(a, nb, height, width, z_total);
        if (a.overflow) return locr_fail(eng, "webp_decode", "workspace layout exceeds the reservation");
        LOCR_CHECK(hipMemcpyAsync(w.F, F.data(), sizeof(WpFile) * nb, hipMemcpyHostToDevice, st));
        LOCR_CHECK(hipMemcpyAsync(w.z, zs, z_total, hipMemcpyHostToDevice, st));
        LOCR_CHECK(hipEventRecord(stage.uploaded.get(), st));
        hipLaunchKernelGGL(wp_entropy, dim3(nb), dim3(64), 0, st, w.F, w.z, w.planes, w.sub, w.tab, w.heads, width, height, pw, sw);
        const size_t npx = (size_t)width * height;
        const dim3 grid((unsigned)std::min<size_t>((npx + 255) / 256, 4096), nb);
        for (int step = 0; step < 4; ++step) {
            hipLaunchKernelGGL(wp_palette, grid, dim3(256), 0, st, w.F, w.heads, w.planes, w.sub, height, pw, sw, step);
            hipLaunchKernelGGL(wp_green, grid, dim3(256), 0, st, w.F, w.heads, w.planes, height, pw, step);
            hipLaunchKernelGGL(wp_cross, grid, dim3(256), 0, st, w.F, w.heads, w.planes, w.sub, height, pw, sw, step);
            hipLaunchKernelGGL(wp_predictor, dim3(nb), dim3(64), 0, st, w.F, w.heads, w.planes, w.sub, height, pw, sw, step);
        }
        hipLaunchKernelGGL(wp_rgb, grid, dim3(256), 0, st, w.F, w.heads, w.planes, out_dev, width, height, pw);
        std::vector<WpHead> heads((size_t)nb);
        LOCR_CHECK(hipMemcpyAsync(heads.data(), w.heads, sizeof(WpHead) * nb, hipMemcpyDeviceToHost, st));
        LOCR_CHECK(hipStreamSynchronize(st));
        LOCR_CHECK(hipGetLastError());
        for (int k = 0; k < nb; ++k)
            if (F[(size_t)k].valid) status[i0 + k] = heads[(size_t)k].err;
    }
    return 0;
}
