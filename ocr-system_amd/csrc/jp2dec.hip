// JPEG 2000 decoder on the device (see jp2dec.h).  The host reads the boxes and headers and walks the packet headers (jp2_parse.h:
// tier 2, kilobytes per page, no pixel).  The device does the rest:
//   j2_tier1   one wave64 per code-block, every block of every page of the sub-batch in one launch: the MQ decoder and the three
//              coding passes per bit-plane (jp2_t1.h).  The decision walk is serial and runs on one lane over row bit-maps in LDS
//              (64-bit words, one per block row); the wave clears the state and writes the coefficients out.  10.5 KB of LDS per
//              wave: 15 waves per CU.
//   j2_dwt_h / j2_dwt_v   the inverse 5/3 lifting, level by level, horizontal then vertical, between two int32 planes: one launch per
//              level and direction over every tile-component of every page (J2Tile; a one-tile page is one tile-component a plane)
//   j2_dwt97_h / j2_dwt97_v   the inverse 9/7 lifting of the irreversible pages, beside them, over the same two planes read as float
//   j2_finish  inverse colour transform (reversible or irreversible), level shift, clamp -> RGB u8
// A 9/7 page (J2Page::kind 1) differs from a 5/3 page in the value tier 1 writes (the half-unit magnitude times half the step size,
// as float), in its lifting kernels and in the branch of j2_finish; both kinds share a batch and the tier-1 launch.  All of the float
// arithmetic is in jp2_t1.h, one rounding per operation in OpenJPEG's order, so the bytes are Pillow's.
// A component plane is [height][width] of the image area.  Each tile-component owns its rectangle of the plane and keeps its sub-bands
// inside it as the transform reads them, low-pass part top left; tier 1 writes a block where the host's record says, so it does not
// know tiles.  Sizes and the parity of a line's first sample come from the tile's corners on the canvas.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "engine.h"
#include "jp2_parse.h"
#include "jp2_t1.h"
#include "jp2dec.h"

namespace {

struct J2Block {
    unsigned long long data_off;   // its coded bytes (the segments of all layers, concatenated) in the sub-batch's byte buffer
    unsigned data_len;
    int plane;                     // index of its component plane in the sub-batch
    int x, y;                      // rectangle in the plane
    unsigned char w, h, orient, nbps;
    int passes;
    float hs;                      // 9/7: half the step size of its sub-band; 0: the integer (5/3) path
};
struct J2Page { int levels, comps, mct, out_index, plane0, kind; };   // kind: 0 = 5/3 (int32 planes), 1 = 9/7 (float planes)

__global__ __launch_bounds__(64) void j2_tier1(const J2Block* __restrict__ blocks, const uint8_t* __restrict__ bytes, int* __restrict__ coef,
                                               int height, int width) {
    __shared__ Jp2T1State S;
    const J2Block b = blocks[blockIdx.x];
    const int lane = threadIdx.x;
    unsigned* words = reinterpret_cast<unsigned*>(&S);
    for (unsigned i = lane; i < sizeof(Jp2T1State) / 4; i += 64) words[i] = 0;
    __syncthreads();
    jp2_t1_tables(S, lane, 64);
    __syncthreads();
    if (lane == 0) jp2_t1_walk(S, bytes + b.data_off, b.data_len, b.w, b.h, b.orient, b.nbps, b.passes);
    __syncthreads();
    int* dst = coef + (size_t)b.plane * height * width;
    const int n = (int)b.w * b.h;
    for (int i = lane; i < n; i += 64) {
        const int y = i / b.w, x = i - y * b.w;
        dst[(size_t)(b.y + y) * width + b.x + x] = b.hs != 0.0f ? __float_as_int(jp2_t1_value_f(S, y, x, b.hs)) : jp2_t1_value(S, y, x);
    }
}

// A tile-component: its rectangle of its component plane (px, py, x1 - x0 wide, y1 - y0 high), its corners on the canvas, and what to
// run on it.  Sizes on a resolution come from the canvas corners, ceil(x1 / 2^s) - ceil(x0 / 2^s), and so does the parity of a line's
// first sample: a line that starts on an odd coordinate starts with a high-pass sample (jp2_t1.h).
struct J2Tile { int plane, px, py, x0, y0, x1, y1, levels, kind; };

__device__ inline int j2_cdivp(int a, int sh) { return (a + (1 << sh) - 1) >> sh; }

// One step of the inverse transform: every tile-component whose `levels` reach `step` rebuilds its resolution `step` (top left of its
// rectangle).  blockIdx.x = tile-component * per + share: `per` work-groups split a tile-component's samples between them.
__global__ __launch_bounds__(256) void j2_dwt_h(const J2Tile* __restrict__ tiles, const int* __restrict__ src, int* __restrict__ dst, int height,
                                                int width, int step, unsigned per) {
    const J2Tile T = tiles[blockIdx.x / per];
    if (T.kind != 0 || step > T.levels) return;
    const int sh = T.levels - step, rx0 = j2_cdivp(T.x0, sh), rw = j2_cdivp(T.x1, sh) - rx0, rh = j2_cdivp(T.y1, sh) - j2_cdivp(T.y0, sh);
    const int cas = rx0 & 1, np = (rw + 1) / 2;
    const size_t base = ((size_t)T.plane * height + T.py) * width + T.px;
    for (long long i = (long long)(blockIdx.x % per) * 256 + threadIdx.x; i < (long long)rh * np; i += (long long)per * 256) {
        const int y = (int)(i / np), k = (int)(i - (long long)y * np);
        const int* line = src + base + (size_t)y * width;
        int* o = dst + base + (size_t)y * width;
        o[2 * k] = jp2_lift_at(line, 1, rw, cas, 2 * k);
        if (2 * k + 1 < rw) o[2 * k + 1] = jp2_lift_at(line, 1, rw, cas, 2 * k + 1);
    }
}

__global__ __launch_bounds__(256) void j2_dwt_v(const J2Tile* __restrict__ tiles, const int* __restrict__ src, int* __restrict__ dst, int height,
                                                int width, int step, unsigned per) {
    const J2Tile T = tiles[blockIdx.x / per];
    if (T.kind != 0 || step > T.levels) return;
    const int sh = T.levels - step, ry0 = j2_cdivp(T.y0, sh), rw = j2_cdivp(T.x1, sh) - j2_cdivp(T.x0, sh), rh = j2_cdivp(T.y1, sh) - ry0;
    const int cas = ry0 & 1, np = (rh + 1) / 2;
    const size_t base = ((size_t)T.plane * height + T.py) * width + T.px;
    for (long long i = (long long)(blockIdx.x % per) * 256 + threadIdx.x; i < (long long)np * rw; i += (long long)per * 256) {
        const int k = (int)(i / rw), x = (int)(i - (long long)k * rw);
        const int* line = src + base + x;
        int* o = dst + base + x;
        o[(size_t)(2 * k) * width] = jp2_lift_at(line, width, rh, cas, 2 * k);
        if (2 * k + 1 < rh) o[(size_t)(2 * k + 1) * width] = jp2_lift_at(line, width, rh, cas, 2 * k + 1);
    }
}

// ---- the 9/7 lifting.  An output sample depends on four input samples to either side through the four steps, so a work-group holds a
// window of a line in LDS (jp2_lift97_at): the samples it owns and JP2_LIFT97_HALO more a side, interleaved and scaled as they are
// loaded, then one step per barrier interval.  The expression tree of a sample is fixed, so neither the windows nor the tiling of the
// launch show in the bits.
constexpr int J2_HSEG = 256;    // samples of a row a work-group of j2_dwt97_h owns (a sample pair per thread and step; 3 % of halo)
constexpr int J2_VSEG = 56;     // rows of a 64-column strip a work-group of j2_dwt97_v owns: 64 x 64 floats, 16 KB of LDS

// blockIdx.x = tile-component * per + share; a tile-component's units are (window of the row, row), shared out between its `per`
// work-groups.  Lanes read the two halves of the row alternately (two runs of 32 floats per wave) and write the row out contiguously;
// the steps touch every other float of the window, a 2-way bank conflict that four short passes over 1 KB do not repay removing.
__global__ __launch_bounds__(128) void j2_dwt97_h(const J2Tile* __restrict__ tiles, const float* __restrict__ src, float* __restrict__ dst, int height,
                                                  int width, int step, unsigned per) {
    __shared__ float w[J2_HSEG + 2 * JP2_LIFT97_HALO];
    const J2Tile T = tiles[blockIdx.x / per];
    if (T.kind != 1 || step > T.levels) return;
    const int sh = T.levels - step, rx0 = j2_cdivp(T.x0, sh), rw = j2_cdivp(T.x1, sh) - rx0, rh = j2_cdivp(T.y1, sh) - j2_cdivp(T.y0, sh);
    const int cas = rx0 & 1, tid = threadIdx.x;
    const long long units = rh > 0 ? (long long)((rw + J2_HSEG - 1) / J2_HSEG) * rh : 0;
    const size_t base = ((size_t)T.plane * height + T.py) * width + T.px;
    for (long long u = blockIdx.x % per; u < units; u += per) {
        const int y = (int)(u % rh), seg0 = (int)(u / rh) * J2_HSEG;
        const int lo = seg0 - JP2_LIFT97_HALO < 0 ? 0 : seg0 - JP2_LIFT97_HALO;
        const int end = seg0 + J2_HSEG < rw ? seg0 + J2_HSEG : rw, hi = end + JP2_LIFT97_HALO < rw ? end + JP2_LIFT97_HALO : rw;
        const size_t row = base + (size_t)y * width;
        for (int i = lo + tid; i < hi; i += 128) w[i - lo] = jp2_lift97_load(src + row, 1, rw, i, cas);
        __syncthreads();
        for (int s = 0; s < 4; ++s) {
            const float c = jp2_lift97_coef(s);
            for (int i = jp2_lift97_first(lo, s, cas) + 2 * tid; i < hi; i += 256) jp2_lift97_at(w, 1, lo, hi, rw, i, c);
            __syncthreads();
        }
        for (int i = seg0 + tid; i < end; i += 128) dst[row + i] = w[i - lo];
        __syncthreads();   // the next unit loads over the window
    }
}

// A tile-component's units are (window of the columns, 64-column strip).  A wave is 64 neighbouring columns of one row: its loads and
// stores are 256 contiguous bytes and its LDS accesses one bank row.
__global__ __launch_bounds__(256) void j2_dwt97_v(const J2Tile* __restrict__ tiles, const float* __restrict__ src, float* __restrict__ dst, int height,
                                                  int width, int step, unsigned per) {
    __shared__ float w[(J2_VSEG + 2 * JP2_LIFT97_HALO) * 64];
    const J2Tile T = tiles[blockIdx.x / per];
    if (T.kind != 1 || step > T.levels) return;
    const int sh = T.levels - step, ry0 = j2_cdivp(T.y0, sh), rw = j2_cdivp(T.x1, sh) - j2_cdivp(T.x0, sh), rh = j2_cdivp(T.y1, sh) - ry0;
    const int cas = ry0 & 1, strips = (rw + 63) / 64;
    const long long units = (long long)strips * ((rh + J2_VSEG - 1) / J2_VSEG);
    const int cx = threadIdx.x & 63, q = threadIdx.x >> 6;
    const size_t base = ((size_t)T.plane * height + T.py) * width + T.px;
    for (long long u = blockIdx.x % per; u < units; u += per) {
        const int x0 = (int)(u % strips) * 64, seg0 = (int)(u / strips) * J2_VSEG;
        const int lo = seg0 - JP2_LIFT97_HALO < 0 ? 0 : seg0 - JP2_LIFT97_HALO;
        const int end = seg0 + J2_VSEG < rh ? seg0 + J2_VSEG : rh, hi = end + JP2_LIFT97_HALO < rh ? end + JP2_LIFT97_HALO : rh;
        const int x = x0 + cx;
        const bool live = x < rw;
        const size_t col = base + (size_t)(live ? x : x0);
        if (live)
            for (int i = lo + q; i < hi; i += 4) w[(i - lo) * 64 + cx] = jp2_lift97_load(src + col, width, rh, i, cas);
        __syncthreads();
        for (int s = 0; s < 4; ++s) {
            const float c = jp2_lift97_coef(s);
            if (live)
                for (int i = jp2_lift97_first(lo, s, cas) + 2 * q; i < hi; i += 8) jp2_lift97_at(w + cx, 64, lo, hi, rh, i, c);
            __syncthreads();
        }
        if (live)
            for (int i = seg0 + q; i < end; i += 4) dst[col + (size_t)i * width] = w[(i - lo) * 64 + cx];
        __syncthreads();   // the next unit loads over the window
    }
}

__device__ inline uint8_t j2_sample(int v) { v += 128; return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

__global__ __launch_bounds__(256) void j2_finish(const J2Page* __restrict__ pages, const int* __restrict__ coef, uint8_t* __restrict__ out, int height, int width) {
    const J2Page pg = pages[blockIdx.y];
    const size_t npx = (size_t)height * width;
    const int* p0 = coef + (size_t)pg.plane0 * npx;
    uint8_t* o = out + (size_t)pg.out_index * npx * 3;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (size_t)gridDim.x * 256) {
        if (pg.kind == 1) {
            const float* f0 = reinterpret_cast<const float*>(p0);
            uint8_t rgb[3];
            if (pg.comps == 1) rgb[0] = rgb[1] = rgb[2] = jp2_sample97(f0[i]);
            else jp2_finish97(f0[i], f0[npx + i], f0[2 * npx + i], pg.mct, rgb);
            o[3 * i] = rgb[0]; o[3 * i + 1] = rgb[1]; o[3 * i + 2] = rgb[2];
            continue;
        }
        int r, g, b;
        if (pg.comps == 1) {
            r = g = b = p0[i];
        } else if (pg.mct) {
            const int y = p0[i], u = p0[npx + i], v = p0[2 * npx + i];
            g = y - ((u + v) >> 2); r = v + g; b = u + g;
        } else {
            r = p0[i]; g = p0[npx + i]; b = p0[2 * npx + i];
        }
        o[3 * i] = j2_sample(r); o[3 * i + 1] = j2_sample(g); o[3 * i + 2] = j2_sample(b);
    }
}

struct J2Workspace { J2Block* blocks; J2Page* pages; J2Tile* tiles; uint8_t* bytes; int *a, *b; };
J2Workspace j2_layout(Arena& a, size_t nblocks, size_t nbytes, int pages, size_t planes, int height, int width, size_t ntiles) {
    J2Workspace w;
    w.blocks = a.take<J2Block>(nblocks); w.pages = a.take<J2Page>((size_t)pages); w.tiles = a.take<J2Tile>(ntiles); w.bytes = a.take<uint8_t>(nbytes);
    w.a = a.take<int>(planes * height * width); w.b = a.take<int>(planes * height * width);
    return w;
}

inline int h_cdivp(int a, int sh) { return (a + (1 << sh) - 1) >> sh; }

}  // namespace

size_t jp2dec_workspace_bytes(size_t nblocks, size_t nbytes, int pages, size_t planes, int height, int width, size_t tile_components) {
    Arena a;
    j2_layout(a, nblocks, nbytes, pages, planes, height, width, tile_components);
    return a.off;
}

int jp2dec_probe(const uint8_t* file, size_t n, Jp2Probe* out, unsigned flags) {
    Jp2File f;
    const int rc = jp2_parse(file, n, &f, flags);
    memcpy(out->info, f.info, sizeof(f.info));
    out->reason = f.reason;
    return rc;
}

int jp2dec_run(lumina_ocr* eng, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev, int* status,
               hipStream_t st, unsigned flags) {
    lumina_ocr::Staging& stage = eng->jp_stage;
    if (!stage.uploaded) {
        hipEvent_t ev = nullptr;
        LOCR_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        stage.uploaded.reset(ev);
    }
    const size_t npx = (size_t)height * width;
    const size_t budget = (size_t)eng->jp_sub_batch_mb << 20;
    constexpr size_t MAX_PAGES = 65535;   // a sub-batch's pages are a grid dimension of the colour launch
    int i0 = 0;
    Jp2File held;          // the page that did not fit the last sub-batch: it opens the next one and is not parsed again
    bool holding = false;
    while (i0 < n) {
        // a sub-batch: pages until their coefficient planes (two int32 copies) pass the budget, at least one page
        std::vector<Jp2File> F;
        std::vector<int> index;
        size_t planes = 0, nblocks = 0, nbytes = 0, ntc = 0;
        int i1 = i0;
        for (; i1 < n; ++i1) {
            Jp2File f;
            if (holding) {
                f = std::move(held);
                holding = false;
            } else {
                int rc = jp2_parse(files[i1], sizes[i1], &f, flags);
                if (rc == 0 && (f.width != width || f.height != height)) rc = -4;
                status[i1] = rc;
                if (rc) continue;
            }
            if (!index.empty() && ((planes + (size_t)f.comps) * npx * 8 > budget || index.size() == MAX_PAGES)) {
                held = std::move(f);
                holding = true;
                break;
            }
            planes += (size_t)f.comps;
            ntc += f.tiles.size() * (size_t)f.comps;
            for (const Jp2Block& K : f.blocks)
                if (K.passes) {
                    ++nblocks;
                    size_t len = 0;
                    for (int s = K.seg_head; s >= 0; s = f.segs[(size_t)s].next) len += f.segs[(size_t)s].len;
                    nbytes += len;
                }
            F.push_back(std::move(f));
            index.push_back(i1);
        }
        const int np = (int)index.size();
        if (np) {
            // staging: [J2Block x nblocks][J2Page x np][J2Tile x ntc][bytes]
            const size_t blocks_b = (sizeof(J2Block) * nblocks + 255) & ~(size_t)255, pages_b = (sizeof(J2Page) * np + 255) & ~(size_t)255;
            const size_t tiles_b = (sizeof(J2Tile) * ntc + 255) & ~(size_t)255;
            LOCR_CHECK(hipEventSynchronize(stage.uploaded.get()));
            LOCR_CHECK(stage.buf.reserve(blocks_b + pages_b + tiles_b + nbytes + 256, stage.uploaded.get()));
            J2Block* hb = reinterpret_cast<J2Block*>(stage.buf.get());
            J2Page* hp = reinterpret_cast<J2Page*>(stage.buf.get() + blocks_b);
            J2Tile* ht = reinterpret_cast<J2Tile*>(stage.buf.get() + blocks_b + pages_b);
            uint8_t* hbytes = stage.buf.get() + blocks_b + pages_b + tiles_b;
            size_t bi = 0, ti = 0, off = 0;
            int plane0 = 0, max_levels = 0;
            for (int k = 0; k < np; ++k) {
                const Jp2File& f = F[(size_t)k];
                hp[k] = J2Page{f.levels, f.comps, f.mct, index[(size_t)k], plane0, f.irreversible};
                max_levels = std::max(max_levels, f.levels);
                for (int c = 0; c < f.comps; ++c)
                    for (const Jp2Tile& T : f.tiles) ht[ti++] = J2Tile{plane0 + c, T.x0 - f.x0, T.y0 - f.y0, T.x0, T.y0, T.x1, T.y1, f.levels, f.irreversible};
                for (const Jp2Block& K : f.blocks) {
                    if (!K.passes) continue;
                    J2Block& b = hb[bi++];
                    b.data_off = off; b.plane = plane0 + K.comp; b.x = K.x; b.y = K.y;
                    b.w = (unsigned char)K.w; b.h = (unsigned char)K.h; b.orient = (unsigned char)K.orient; b.nbps = (unsigned char)(K.mb - K.zbp);
                    b.passes = K.passes; b.hs = K.hs;
                    for (int s = K.seg_head; s >= 0; s = f.segs[(size_t)s].next) {
                        memcpy(hbytes + off, files[index[(size_t)k]] + f.segs[(size_t)s].off, f.segs[(size_t)s].len);
                        off += f.segs[(size_t)s].len;
                    }
                    b.data_len = (unsigned)(off - b.data_off);
                }
                plane0 += f.comps;
            }
            Arena sizing;
            j2_layout(sizing, nblocks, nbytes + 256, np, planes, height, width, ntc);
            if (eng_ws_reserve(eng, sizing.off)) return 1;
            Arena a(eng->ws.get(), eng->ws.cap);
            const J2Workspace w = j2_layout(a, nblocks, nbytes + 256, np, planes, height, width, ntc);
            if (a.overflow) return locr_fail(eng, "jp2_decode", "workspace layout exceeds the reservation");
            if (nblocks) LOCR_CHECK(hipMemcpyAsync(w.blocks, hb, sizeof(J2Block) * nblocks, hipMemcpyHostToDevice, st));
            LOCR_CHECK(hipMemcpyAsync(w.pages, hp, sizeof(J2Page) * np, hipMemcpyHostToDevice, st));
            LOCR_CHECK(hipMemcpyAsync(w.tiles, ht, sizeof(J2Tile) * ntc, hipMemcpyHostToDevice, st));
            if (nbytes) LOCR_CHECK(hipMemcpyAsync(w.bytes, hbytes, nbytes, hipMemcpyHostToDevice, st));
            LOCR_CHECK(hipEventRecord(stage.uploaded.get(), st));
            LOCR_CHECK(hipMemsetAsync(w.a, 0, planes * npx * sizeof(int), st));   // blocks no layer includes are zero
            if (nblocks) hipLaunchKernelGGL(j2_tier1, dim3((unsigned)nblocks), dim3(64), 0, st, w.blocks, w.bytes, w.a, height, width);
            float* const fa = reinterpret_cast<float*>(w.a);
            float* const fb = reinterpret_cast<float*>(w.b);
            // one launch per step and direction over all tile-components: blockIdx.x = tile-component * per + share, `per` from the
            // largest tile-component of the step (a grid's x dimension holds 2^31 - 1 work-groups; the kernels stride over what is left)
            const size_t most = (size_t)0x7FFFFFFF / ntc;
            for (int step = 1; step <= max_levels; ++step) {
                size_t work = 0;               // the largest resolution any 5/3 tile-component rebuilds at this step
                size_t units_h = 0, units_v = 0;   // the most windows any 9/7 tile-component has, along the rows and along the columns
                for (const Jp2File& f : F)
                    if (step <= f.levels) {
                        const int sh = f.levels - step;
                        for (const Jp2Tile& T : f.tiles) {
                            const size_t rw = (size_t)(h_cdivp(T.x1, sh) - h_cdivp(T.x0, sh)), rh = (size_t)(h_cdivp(T.y1, sh) - h_cdivp(T.y0, sh));
                            if (f.irreversible) {
                                units_h = std::max(units_h, (rw + J2_HSEG - 1) / J2_HSEG * rh);
                                units_v = std::max(units_v, (rw + 63) / 64 * ((rh + J2_VSEG - 1) / J2_VSEG));
                            } else {
                                work = std::max(work, rh * rw);
                            }
                        }
                    }
                if (work) {
                    const unsigned per = (unsigned)std::min<size_t>(std::min<size_t>((work / 2 + 255) / 256 + 1, 2048), most);
                    hipLaunchKernelGGL(j2_dwt_h, dim3((unsigned)(ntc * per)), dim3(256), 0, st, w.tiles, w.a, w.b, height, width, step, per);
                    hipLaunchKernelGGL(j2_dwt_v, dim3((unsigned)(ntc * per)), dim3(256), 0, st, w.tiles, w.b, w.a, height, width, step, per);
                }
                if (units_h) {
                    const unsigned per_h = (unsigned)std::min(units_h, most), per_v = (unsigned)std::min(units_v, most);
                    hipLaunchKernelGGL(j2_dwt97_h, dim3((unsigned)(ntc * per_h)), dim3(128), 0, st, w.tiles, fa, fb, height, width, step, per_h);
                    hipLaunchKernelGGL(j2_dwt97_v, dim3((unsigned)(ntc * per_v)), dim3(256), 0, st, w.tiles, fb, fa, height, width, step, per_v);
                }
            }
            hipLaunchKernelGGL(j2_finish, dim3((unsigned)std::min<size_t>((npx + 255) / 256, 2048), (unsigned)np), dim3(256), 0, st, w.pages, w.a, out_dev,
                               height, width);
            LOCR_CHECK(hipStreamSynchronize(st));
            LOCR_CHECK(hipGetLastError());
        }
        i0 = i1;
    }
    return 0;
}
