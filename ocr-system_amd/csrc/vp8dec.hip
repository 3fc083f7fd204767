// Lossy WebP (VP8 key frame) decoder on the device (vp8dec.h): what the reference's Image.open(...).convert('RGB') does for lossy .webp
// inputs, byte-identical to Pillow (libwebp).  Lossless files of the same batch take webpdec.hip's kernels.
//
// The host (vp8_parse.h) walks the container and reads the boolean-coded frame header, whose work does not grow with the page, and
// gathers each file's VP8 payload into one pinned staging buffer.  The device then runs, per sub-batch (functions in vp8_dec.h):
//   1. vp8_modes: one wave64 work-group per file; lane 0 walks the first partition (segment id, skip flag, luma mode with its 16
//      sub-modes in context, chroma mode) into one Vp8Mb record per macroblock.  The row of above modes sits in LDS;
//   2. vp8_tokens: one wave64 work-group per file.  All lanes copy the frame header into LDS and clear the file's coefficient plane
//      with 16-byte stores; lane 0 then walks the token partitions one macroblock row after another (row r from partition r & (P - 1),
//      the decoder states of the partitions in LDS), writes dequantised coefficients, undoes the WHT, and records each block's
//      non-zero bit and the inner-edge decision.  The partitions of a file are walked in turn, not side by side: row r needs the
//      contexts of row r - 1, and lanes of one wave must not wait on each other;
//   3. vp8_recon: one work-group of 256 per file walks the diagonals x + 2y of the macroblock grid, VP8_RECON_MBS = 16 macroblocks at a
//      time, 16 lanes a macroblock.  A lane owns the 4x4 luma block (bx, by) and runs it at sub-step bx + 2 by of ten (prediction from
//      the unfiltered frame, inverse DCT, add); lanes 0..7 also own the eight chroma blocks;
//   4. vp8_filter: the same walk over the finished unfiltered frame, a lane per line of an edge (16 luma lines; 8 U and 8 V lines):
//      left edge, inner vertical edges, top edge, inner horizontal edges.  A file whose frame level is 0 returns at once;
//   5. vp8_rgb: fancy up-sampling, YUV -> RGB, crop; every output byte written once.
// A file whose walk breaks a rule ends with err != 0 in its head and is not written.
#include "vp8dec.h"

#include <algorithm>
#include <cstring>
#include <vector>

#include "engine.h"
#include "vp8_dec.h"
#include "vp8_parse.h"
#include "webpdec.h"

namespace {

constexpr int VP8_RECON_MBS = 16;   // macroblocks of a diagonal a work-group handles at a time
constexpr int VP8_MAX_MBW = 1024;   // 16383 pixels
static_assert(sizeof(Vp8Frame) % 4 == 0, "the frame header is copied in words");

struct Vp8File {
    unsigned long long zoff;   // byte offset of the VP8 payload in the sub-batch's stream buffer (a multiple of 16)
    int out_index;
};

struct Vp8Planes {   // one file's share of the workspace, in elements
    size_t mbs, coefs, y, uv;
};
__host__ __device__ inline Vp8Planes vp8_planes(int mbw, int mbh) {
    Vp8Planes p;
    p.mbs = (size_t)mbw * mbh;
    p.coefs = p.mbs * VP8_MB_COEFS;
    p.y = p.mbs * 256;
    p.uv = p.mbs * 64;
    return p;
}

__global__ __launch_bounds__(64) void vp8_modes(const Vp8File* __restrict__ F, const Vp8Frame* __restrict__ frames, const uint8_t* __restrict__ z,
                                                Vp8Mb* __restrict__ mbs, int* __restrict__ err) {
    __shared__ uint8_t top[4 * VP8_MAX_MBW];
    const int k = blockIdx.x;
    if (threadIdx.x != 0) return;
    const Vp8Frame& fr = frames[k];
    err[k] = vp8_mode_walk(fr, z + F[k].zoff, mbs + (size_t)k * fr.mbw * fr.mbh, top);
}

__global__ __launch_bounds__(64) void vp8_tokens(const Vp8File* __restrict__ F, const Vp8Frame* __restrict__ frames, const uint8_t* __restrict__ z,
                                                 Vp8Mb* __restrict__ mbs, int16_t* __restrict__ coefs, int* __restrict__ err) {
    __shared__ Vp8Frame fr;
    __shared__ uint8_t tnz[VP8_MAX_MBW], tdc[VP8_MAX_MBW];
    __shared__ Vp8Bool pb[8];
    __shared__ int16_t y2[16];
    const int k = blockIdx.x;
    if (err[k]) return;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(frames + k);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&fr);
        for (unsigned i = threadIdx.x; i < sizeof(Vp8Frame) / 4; i += 64) dst[i] = src[i];
    }
    __syncthreads();
    const Vp8Planes P = vp8_planes(fr.mbw, fr.mbh);
    {
        uint4* c = reinterpret_cast<uint4*>(coefs + (size_t)k * P.coefs);   // (a macroblock's coefficients are 768 bytes)
        const size_t n16 = P.coefs * sizeof(int16_t) / 16;
        for (size_t i = threadIdx.x; i < n16; i += 64) c[i] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    err[k] = vp8_token_walk(fr, z + F[k].zoff, mbs + (size_t)k * P.mbs, coefs + (size_t)k * P.coefs, tnz, tdc, pb, y2);
}

// macroblock j of diagonal d (x + 2y = d), counted from the smallest y; n: macroblocks on the diagonal
__device__ inline int vp8_diagonal(int d, int mbw, int mbh, int* y0) {
    const int lo = d - (mbw - 1) > 0 ? (d - (mbw - 1) + 1) >> 1 : 0;
    const int hi = (d >> 1) < mbh - 1 ? (d >> 1) : mbh - 1;
    *y0 = lo;
    return hi - lo + 1;
}

__global__ __launch_bounds__(256) void vp8_recon(const Vp8Frame* __restrict__ frames, const Vp8Mb* __restrict__ mbs, const int16_t* __restrict__ coefs,
                                                 uint8_t* __restrict__ ybuf, uint8_t* __restrict__ ubuf, uint8_t* __restrict__ vbuf,
                                                 const int* __restrict__ err) {
    const int k = blockIdx.x;
    if (err[k]) return;
    const Vp8Frame& fr = frames[k];
    const int mbw = fr.mbw, mbh = fr.mbh, ys = 16 * mbw, uvs = 8 * mbw;
    const Vp8Planes P = vp8_planes(mbw, mbh);
    const Vp8Mb* M = mbs + (size_t)k * P.mbs;
    const int16_t* C = coefs + (size_t)k * P.coefs;
    uint8_t *Y = ybuf + (size_t)k * P.y, *U = ubuf + (size_t)k * P.uv, *V = vbuf + (size_t)k * P.uv;
    const int slot = threadIdx.x >> 4, lane = threadIdx.x & 15;
    const int luma_step = (lane & 3) + 2 * (lane >> 2), chroma_step = luma_step == 0 ? 1 : 0;
    for (int d = 0; d <= mbw - 1 + 2 * (mbh - 1); ++d) {
        int y0;
        const int n = vp8_diagonal(d, mbw, mbh, &y0);
        for (int j0 = 0; j0 < n; j0 += VP8_RECON_MBS) {
            const int j = j0 + slot;
            const bool on = j < n;
            const int y = y0 + (on ? j : 0), x = d - 2 * y;
            const size_t i = (size_t)y * mbw + x;
            for (int s = 0; s < 10; ++s) {
                if (on) {
                    if (s == luma_step) vp8_recon_luma(fr, M[i], C + i * VP8_MB_COEFS, x, y, lane, Y, ys);
                    if (s == chroma_step && lane < 8) vp8_recon_chroma(M[i], C + i * VP8_MB_COEFS, x, y, lane, U, V, uvs);
                }
                __syncthreads();   // the blocks of this sub-step (and, after the last one, of this diagonal) -> their neighbours
            }
        }
    }
}

__global__ __launch_bounds__(256) void vp8_filter(const Vp8Frame* __restrict__ frames, const Vp8Mb* __restrict__ mbs, uint8_t* __restrict__ ybuf,
                                                  uint8_t* __restrict__ ubuf, uint8_t* __restrict__ vbuf, const int* __restrict__ err) {
    const int k = blockIdx.x;
    if (err[k]) return;
    const Vp8Frame& fr = frames[k];
    if (fr.filter_type == 0) return;
    const int mbw = fr.mbw, mbh = fr.mbh, ys = 16 * mbw, uvs = 8 * mbw;
    const Vp8Planes P = vp8_planes(mbw, mbh);
    const Vp8Mb* M = mbs + (size_t)k * P.mbs;
    uint8_t *Y = ybuf + (size_t)k * P.y, *U = ubuf + (size_t)k * P.uv, *V = vbuf + (size_t)k * P.uv;
    const int slot = threadIdx.x >> 4, lane = threadIdx.x & 15;
    for (int d = 0; d <= mbw - 1 + 2 * (mbh - 1); ++d) {
        int y0;
        const int n = vp8_diagonal(d, mbw, mbh, &y0);
        for (int j0 = 0; j0 < n; j0 += VP8_RECON_MBS) {
            const int j = j0 + slot;
            const bool on = j < n;
            const int y = y0 + (on ? j : 0), x = d - 2 * y;
            for (int s = 0; s < 4; ++s) {
                if (on) vp8_filter_step(fr, M[(size_t)y * mbw + x], x, y, s, lane, Y, U, V, ys, uvs);
                __syncthreads();
            }
        }
    }
}

__global__ __launch_bounds__(256) void vp8_rgb(const Vp8File* __restrict__ F, const Vp8Frame* __restrict__ frames, const uint8_t* __restrict__ ybuf,
                                               const uint8_t* __restrict__ ubuf, const uint8_t* __restrict__ vbuf, const int* __restrict__ err,
                                               uint8_t* __restrict__ out) {
    const int k = blockIdx.y;
    if (err[k]) return;
    const Vp8Frame& fr = frames[k];
    const int W = fr.width, H = fr.height, ys = 16 * fr.mbw, uvs = 8 * fr.mbw;
    const Vp8Planes P = vp8_planes(fr.mbw, fr.mbh);
    const uint8_t *Y = ybuf + (size_t)k * P.y, *U = ubuf + (size_t)k * P.uv, *V = vbuf + (size_t)k * P.uv;
    uint8_t* o = out + (size_t)F[k].out_index * H * W * 3;
    const size_t n = (size_t)W * H;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (size_t)gridDim.x * 256) {
        const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
        uint8_t rgb[3];
        vp8_rgb_px(Y, U, V, ys, uvs, W, H, x, y, rgb);
        o[3 * p] = rgb[0]; o[3 * p + 1] = rgb[1]; o[3 * p + 2] = rgb[2];
    }
}

struct Vp8Workspace { Vp8File* F; Vp8Frame* frames; int* err; uint8_t* z; Vp8Mb* mbs; int16_t* coefs; uint8_t *y, *u, *v; };
Vp8Workspace vp8_layout(Arena& a, int n, int height, int width, size_t z_total) {
    const Vp8Planes P = vp8_planes((width + 15) >> 4, (height + 15) >> 4);
    Vp8Workspace w;
    w.F = a.take<Vp8File>(n); w.frames = a.take<Vp8Frame>(n); w.err = a.take<int>(n); w.z = a.take<uint8_t>(z_total);
    w.mbs = a.take<Vp8Mb>((size_t)n * P.mbs);
    w.coefs = a.take<int16_t>((size_t)n * P.coefs);
    w.y = a.take<uint8_t>((size_t)n * P.y); w.u = a.take<uint8_t>((size_t)n * P.uv); w.v = a.take<uint8_t>((size_t)n * P.uv);
    return w;
}
size_t vp8_padded(size_t len) { return (len + 15 + 16) & ~(size_t)15; }

}  // namespace

size_t vp8dec_workspace_bytes(int n, int height, int width, size_t z_total) {
    Arena a;
    vp8_layout(a, n, height, width, z_total);
    return a.off;
}

int vp8dec_probe(const uint8_t* file, size_t size, int info[8], const char** reason) {
    Vp8Info i;
    const int rc = vp8_probe(file, size, &i, nullptr);
    info[0] = i.wp.width; info[1] = i.wp.height; info[2] = i.wp.alpha; info[3] = i.wp.vp8x; info[4] = i.wp.exif; info[5] = i.wp.xmp;
    info[6] = i.lossy; info[7] = i.parts;
    *reason = i.wp.reason ? i.wp.reason : "";
    return rc;
}

int vp8dec_run(lumina_ocr* eng, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev, int* status,
               hipStream_t st) {
    std::vector<Vp8Info> I((size_t)n);
    std::vector<Vp8Frame> frames((size_t)n);
    std::vector<const uint8_t*> lossless((size_t)n, nullptr);
    std::vector<int> lossy;
    int n_lossless = 0;
    for (int i = 0; i < n; ++i) {
        int rc = files[i] ? vp8_probe(files[i], sizes[i], &I[(size_t)i], &frames[(size_t)i]) : -1;
        if (rc == 0 && (I[(size_t)i].wp.width != width || I[(size_t)i].wp.height != height)) rc = -4;
        status[i] = rc;
        if (rc) continue;
        if (I[(size_t)i].lossy) lossy.push_back(i);
        else { lossless[(size_t)i] = files[i]; ++n_lossless; }
    }
    if (n_lossless) {   // the lossless files take the existing kernels; the other entries are absent to that call
        std::vector<int> st2((size_t)n);
        if (webpdec_run(eng, lossless.data(), sizes, n, height, width, out_dev, st2.data(), st)) return 1;
        for (int i = 0; i < n; ++i)
            if (lossless[(size_t)i]) status[i] = st2[(size_t)i];
    }
    if (lossy.empty()) return 0;
    lumina_ocr::Staging& stage = eng->wp_stage;
    if (!stage.uploaded) {
        hipEvent_t ev = nullptr;
        LOCR_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        stage.uploaded.reset(ev);
    }
    // sub-batches of at most eng->wp_sub_batch_mb MB of records, coefficients and planes (at least one file each)
    const size_t per_file = vp8dec_workspace_bytes(1, height, width, 0);
    const int total = (int)lossy.size();
    const int per_batch = (int)std::max<size_t>(1, std::min<size_t>((size_t)total, ((size_t)eng->wp_sub_batch_mb << 20) / per_file));
    for (int i0 = 0; i0 < total; i0 += per_batch) {
        const int nb = std::min(per_batch, total - i0);
        std::vector<Vp8File> F((size_t)nb);
        std::vector<Vp8Frame> fr((size_t)nb);
        size_t z_total = 0;
        for (int k = 0; k < nb; ++k) {
            const int i = lossy[(size_t)(i0 + k)];
            F[(size_t)k].zoff = z_total; F[(size_t)k].out_index = i;
            fr[(size_t)k] = frames[(size_t)i];
            z_total += vp8_padded(I[(size_t)i].wp.len);
        }
        LOCR_CHECK(hipEventSynchronize(stage.uploaded.get()));
        LOCR_CHECK(stage.buf.reserve(z_total, stage.uploaded.get()));
        uint8_t* zs = stage.buf.get();
        for (int k = 0; k < nb; ++k) {
            const int i = lossy[(size_t)(i0 + k)];
            const WpInfo& info = I[(size_t)i].wp;
            memcpy(zs + F[(size_t)k].zoff, files[i] + info.off, info.len);
            memset(zs + F[(size_t)k].zoff + info.len, 0, vp8_padded(info.len) - info.len);
        }
        Arena sizing;
        vp8_layout(sizing, nb, height, width, z_total);
        if (eng_ws_reserve(eng, sizing.off)) return 1;
        Arena a(eng->ws.get(), eng->ws.cap);
        const Vp8Workspace w = vp8_layout(a, nb, height, width, z_total);
        if (a.overflow) return locr_fail(eng, "webp_decode_lossy", "workspace layout exceeds the reservation");
        LOCR_CHECK(hipMemcpyAsync(w.F, F.data(), sizeof(Vp8File) * nb, hipMemcpyHostToDevice, st));
        LOCR_CHECK(hipMemcpyAsync(w.frames, fr.data(), sizeof(Vp8Frame) * nb, hipMemcpyHostToDevice, st));
        LOCR_CHECK(hipMemcpyAsync(w.z, zs, z_total, hipMemcpyHostToDevice, st));
        LOCR_CHECK(hipEventRecord(stage.uploaded.get(), st));
        hipLaunchKernelGGL(vp8_modes, dim3(nb), dim3(64), 0, st, w.F, w.frames, w.z, w.mbs, w.err);
        hipLaunchKernelGGL(vp8_tokens, dim3(nb), dim3(64), 0, st, w.F, w.frames, w.z, w.mbs, w.coefs, w.err);
        hipLaunchKernelGGL(vp8_recon, dim3(nb), dim3(256), 0, st, w.frames, w.mbs, w.coefs, w.y, w.u, w.v, w.err);
        hipLaunchKernelGGL(vp8_filter, dim3(nb), dim3(256), 0, st, w.frames, w.mbs, w.y, w.u, w.v, w.err);
        const size_t npx = (size_t)width * height;
        const dim3 grid((unsigned)std::min<size_t>((npx + 255) / 256, 4096), nb);
        hipLaunchKernelGGL(vp8_rgb, grid, dim3(256), 0, st, w.F, w.frames, w.y, w.u, w.v, w.err, out_dev);
        std::vector<int> err((size_t)nb);
        LOCR_CHECK(hipMemcpyAsync(err.data(), w.err, sizeof(int) * nb, hipMemcpyDeviceToHost, st));
        LOCR_CHECK(hipStreamSynchronize(st));
        LOCR_CHECK(hipGetLastError());
        for (int k = 0; k < nb; ++k) status[lossy[(size_t)(i0 + k)]] = err[(size_t)k];
    }
    return 0;
}
