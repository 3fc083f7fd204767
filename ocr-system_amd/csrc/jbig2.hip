// JBIG2 generic regions on the device (jbig2.h).  The host parser (jbig2_parse.h) turns each page into region records; three kernels
// do the pixel work of a whole batch:
//   jb2_generic  one wave64 per arithmetic-coded region, every region of every page in one launch.  An arithmetic-coded region is one
//                serial stream: each decision depends on the one before through the coder's registers and through the context, so
//                lane 0 walks (jbig2_dec.h, the text the host tests run) and the wave does what is parallel: it clears the contexts,
//                copies typical rows and writes each finished row to the region's 1-bit plane.  The adaptive contexts, a byte each
//                (64 KB for template 0, 8 KB for template 1, 1 KB for 2 and 3), the three live rows and the coder's state table sit in
//                dynamic LDS, sized per launch by the largest template present; two template-0 regions fit a CU's 160 KB.
//   jb2_mmr      one wave64 per MMR region: T.6 lines through the fax decoder's line stages (ccitt_lines.h) into the same planes.
//   jb2_page     pixel-parallel, one work-group per page row and one lane per 32-pixel word: the default pixel, then every region
//                in segment order with its operator, clipped to the page, then the row as RGB bytes.  Every output byte is written once.
// Hostile streams: past the end of its data the arithmetic decoder reads 0xFF (jp2_mq_byte), so a region costs at most
// rows x (columns + 1) decisions whatever its bytes are, and rows are clipped to the page before anything is sized; the MMR walk
// has the fax decoder's checks.  Each region's data is copied to a slot of its own with a zero tail, as the fax decoder's streams are.
#include "jbig2.h"

#include <cstring>
#include <vector>

#include "ccitt_lines.h"
#include "engine.h"
#include "jbig2_dec.h"
#include "jbig2_parse.h"

static_assert(JB2_MAX_COLS == CC_MAX_COLS, "the MMR regions use the fax decoder's line arrays");

namespace {

struct Jb2DevRegion {
    unsigned long long zoff, plane;   // byte offset of the coded data in the batch's buffer; word offset of the region's plane
    unsigned zlen;
    int page, w, rows, x, y, op;      // rows: the region's height clipped to the page's bottom
    int mmr, tmpl, tpgd, nominal;
    int8_t at[8];
};
struct Jb2DevPage { int first, count, default_pixel, valid, invert; };

constexpr int JB2_LDS_ROW = (JB2_MAX_COLS >> 5) + 2;                 // words of one live row (jb2_row_words of the widest region)
constexpr int JB2_LDS_FIXED = (3 * JB2_LDS_ROW + 48 + 4) * 4;        // three rows, the state table, the row's LTP flag
constexpr int JB2_LDS_MAX = JB2_LDS_FIXED + (1 << 16);

__global__ __launch_bounds__(64) void jb2_generic(const Jb2DevRegion* __restrict__ R, const uint8_t* __restrict__ z, uint32_t* planes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Jb2DevRegion& r = R[blockIdx.x];
    if (r.mmr) return;
    const int lane = threadIdx.x;
    uint32_t* rows = reinterpret_cast<uint32_t*>(smem);
    uint32_t* mq = rows + 3 * JB2_LDS_ROW;
    int* flag = reinterpret_cast<int*>(mq + 48);
    uint8_t* cx = reinterpret_cast<uint8_t*>(flag + 4);
    const int ncx = 1 << jb2_context_bits(r.tmpl);
    for (int i = lane; i < 3 * JB2_LDS_ROW; i += 64) rows[i] = 0;
    for (int i = lane; i < ncx / 4; i += 64) reinterpret_cast<uint32_t*>(cx)[i] = 0;   // state 0, MPS 0
    for (int i = lane; i < 47; i += 64) mq[i] = jp2_mq_states[i];
    __syncthreads();
    Jp2Mq m;
    m.cx[0] = m.cx[1] = m.cx[2] = 0;   // (unused: the contexts are bytes of LDS here)
    jp2_mq_init(m, z + r.zoff, r.zlen);
    const int W = r.w, pw = jb2_plane_words(W), rw = jb2_row_words(W);
    uint32_t* plane = planes + r.plane;
    int ltp = 0;
    for (int y = 0; y < r.rows; ++y) {
        uint32_t* r0 = rows + (y % 3) * JB2_LDS_ROW;
        const uint32_t* r1 = rows + ((y + 2) % 3) * JB2_LDS_ROW;
        const uint32_t* r2 = rows + ((y + 1) % 3) * JB2_LDS_ROW;
        for (int j = lane; j < rw; j += 64) r0[j] = 0;   // (it held row y - 3)
        __syncthreads();
        if (lane == 0) {
            if (r.tpgd) ltp ^= jb2_sltp(m, mq, cx, r.tmpl);
            *flag = ltp;
            if (!ltp) {
                const Jb2Rows rr{r0, r1, r2, plane, pw, W, y};
                if (r.nominal) jb2_row_nominal(m, mq, cx, rr, r.tmpl);
                else jb2_row_general(m, mq, cx, rr, r.tmpl, r.at);
            }
        }
        __syncthreads();
        const bool typical = *flag != 0;   // a typical row is the row above (zeros above the region)
        for (int j = lane; j < pw; j += 64) {
            const uint32_t v = typical ? r1[j] : r0[j];
            if (typical) r0[j] = v;
            plane[(size_t)y * pw + j] = v;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void jb2_mmr(const Jb2DevRegion* __restrict__ R, const uint8_t* __restrict__ z, uint32_t* __restrict__ planes,
                                              int* __restrict__ status) {
    __shared__ CcLds L;
    const Jb2DevRegion& r = R[blockIdx.x];
    if (!r.mmr) return;
    const int lane = threadIdx.x, W = r.w, pw = jb2_plane_words(W);
    cc_tables(L, W, lane);
    CcBits b;
    b.z32 = reinterpret_cast<const uint32_t*>(z + r.zoff); b.zlen = r.zlen; b.pos = 0; b.bad = false;
    b.load(lane);
    const unsigned limit = r.zlen * 8u;
    uint32_t* plane = planes + r.plane;
    int y = 0, sel = 0;
    bool bad = false;
    for (; y < r.rows; ++y) {
        if ((b.peek(lane) >> 8) == 0x001001u) break;   // EOFB before all the rows are there
        unsigned short* cur = L.ce[sel ^ 1];
        const int n = cc_line_2d(L, b, L.ce[sel], cur, W, limit, lane);
        if (n < 0) { bad = true; break; }
        cc_line_words(L, cur, n, W, lane);
        for (int j = lane; j < pw; j += 64) plane[(size_t)y * pw + j] = L.bits[j];   // (jb2_page masks the last word's bits past W)
        __syncthreads();
        sel ^= 1;
    }
    if (lane == 0 && (bad || b.bad || y < r.rows)) status[r.page] = -1;   // (every region that fails writes the same value)
}

__global__ __launch_bounds__(256) void jb2_page(const Jb2DevPage* __restrict__ P, const Jb2DevRegion* __restrict__ R, const uint32_t* __restrict__ planes,
                                                const int* __restrict__ status, uint8_t* __restrict__ out, int H, int W) {
    __shared__ uint32_t words[JB2_MAX_COLS / 32];
    const Jb2DevPage& p = P[blockIdx.y];
    if (!p.valid || status[blockIdx.y] != 0) return;
    const int y = blockIdx.x, t = threadIdx.x;
    if (t * 32 < W) {
        uint32_t v = p.default_pixel ? 0xFFFFFFFFu : 0u;
        for (int k = 0; k < p.count; ++k) {
            const Jb2DevRegion& r = R[p.first + k];
            const int ry = y - r.y, lx0 = 32 * t - r.x;   // lx0: the region's column under bit 0 of this word
            if (ry < 0 || ry >= r.rows || lx0 <= -32 || lx0 >= r.w) continue;
            const int rpw = jb2_plane_words(r.w), wj = lx0 >> 5, sh = lx0 & 31;
            const uint32_t* row = planes + r.plane + (size_t)ry * rpw;
            const uint32_t lo = wj >= 0 && wj < rpw ? row[wj] : 0u, hi = wj + 1 >= 0 && wj + 1 < rpw ? row[wj + 1] : 0u;
            const uint32_t src = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
            uint32_t mask = 0xFFFFFFFFu;   // the bits of this word the region covers
            if (lx0 < 0) mask &= 0xFFFFFFFFu << (-lx0);
            if (r.w - lx0 < 32) mask &= (1u << (r.w - lx0)) - 1u;
            switch (r.op) {
                case 0: v |= src & mask; break;
                case 1: v &= src | ~mask; break;
                case 2: v ^= src & mask; break;
                case 3: v = (v & ~mask) | (~(v ^ src) & mask); break;
                default: v = (v & ~mask) | (src & mask); break;
            }
        }
        words[t] = v;
    }
    __syncthreads();
    uint8_t* row = out + ((size_t)blockIdx.y * H + y) * W * 3;
    const uint8_t one = p.invert ? 255 : 0, zero = (uint8_t)(255 - one);   // /JBIG2Decode: bit 1 is black
    for (int bx = t; bx < W * 3; bx += 256) {
        const int px = bx / 3;
        row[bx] = ((words[px >> 5] >> (px & 31)) & 1u) ? one : zero;
    }
}

struct Jb2Workspace { Jb2DevRegion* R; Jb2DevPage* P; int* status; uint8_t* z; uint32_t* planes; };
Jb2Workspace jb2_layout(Arena& a, int n, size_t regions, size_t z_total, size_t plane_words) {
    Jb2Workspace w;
    w.R = a.take<Jb2DevRegion>(regions); w.P = a.take<Jb2DevPage>(n); w.status = a.take<int>(n); w.z = a.take<uint8_t>(z_total);
    w.planes = a.take<uint32_t>(plane_words);
    return w;
}

}  // namespace

int jbig2_probe(const uint8_t* stream, size_t size, const uint8_t* globals, size_t globals_size, Jb2Page* page) {
    return jbig2_parse(stream, size, globals, globals_size, page);
}

int jbig2_run(lumina_ocr* eng, const uint8_t* const* streams, const size_t* sizes, const uint8_t* const* globals, const size_t* globals_sizes,
              int n, int height, int width, const int* params, uint8_t* out_dev, int* status, hipStream_t st) {
    std::vector<Jb2DevPage> P((size_t)n);
    std::vector<Jb2DevRegion> R;
    std::vector<const uint8_t*> src;   // where each region's coded data lies on the host
    size_t z_total = 0, plane_words = 0;
    int any = 0, any_arith = 0, any_mmr = 0, top_bits = 0;
    for (int i = 0; i < n; ++i) {
        Jb2DevPage& p = P[(size_t)i];
        memset(&p, 0, sizeof(p));
        if (!streams[i] || sizes[i] == 0) { status[i] = -1; continue; }
        const uint8_t* g = globals ? globals[i] : nullptr;
        const size_t gs = g && globals_sizes ? globals_sizes[i] : 0;
        Jb2Page page;
        const int rc = jbig2_parse(streams[i], sizes[i], g, gs, &page);
        if (rc) { status[i] = rc; continue; }
        if (page.width != width || page.height != height) { status[i] = -4; continue; }
        status[i] = 0;
        p.valid = 1; ++any;
        p.default_pixel = page.default_pixel;
        p.invert = params[i] != 0;
        p.first = (int)R.size(); p.count = (int)page.regions.size();
        for (const Jb2Region& q : page.regions) {
            Jb2DevRegion r;
            memset(&r, 0, sizeof(r));
            r.page = i; r.w = (int)q.w; r.x = (int)q.x; r.y = (int)q.y; r.op = q.op;   // (w <= 8192, x < width, y < height: the parser)
            r.rows = (int)(q.h < (uint32_t)(height - r.y) ? q.h : (uint32_t)(height - r.y));
            r.mmr = q.mmr; r.tmpl = q.tmpl; r.tpgd = q.tpgd; r.nominal = q.nominal;
            memcpy(r.at, q.at, 8);
            r.zlen = q.len;
            r.zoff = z_total; z_total += (((size_t)q.len + 255) & ~(size_t)255) + CC_Z_PAD;
            r.plane = plane_words; plane_words += (size_t)jb2_plane_words(r.w) * (size_t)r.rows;
            if (q.mmr) ++any_mmr;
            else { ++any_arith; if (jb2_context_bits(q.tmpl) > top_bits) top_bits = jb2_context_bits(q.tmpl); }
            R.push_back(r);
            src.push_back((q.from_globals ? g : streams[i]) + q.off);
        }
    }
    if (!any) return 0;
    if (n > 65535) return locr_fail(eng, "jbig2_decode", "more than 65535 pages in one call");
    const size_t nr = R.size() ? R.size() : 1;
    lumina_ocr::Staging& stage = eng->pd_stage;
    if (!stage.uploaded) {
        hipEvent_t ev = nullptr;
        LOCR_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        stage.uploaded.reset(ev);
    }
    LOCR_CHECK(hipEventSynchronize(stage.uploaded.get()));
    LOCR_CHECK(stage.buf.reserve(z_total ? z_total : 256, stage.uploaded.get()));
    uint8_t* zs = stage.buf.get();
    for (size_t k = 0; k < R.size(); ++k) {
        const size_t slot = (((size_t)R[k].zlen + 255) & ~(size_t)255) + CC_Z_PAD;
        memcpy(zs + R[k].zoff, src[k], R[k].zlen);
        memset(zs + R[k].zoff + R[k].zlen, 0, slot - R[k].zlen);
    }
    Arena sizing;
    jb2_layout(sizing, n, nr, z_total, plane_words);
    if (eng_ws_reserve(eng, sizing.off)) return 1;
    Arena a(eng->ws.get(), eng->ws.cap);
    const Jb2Workspace w = jb2_layout(a, n, nr, z_total, plane_words);
    if (a.overflow) return locr_fail(eng, "jbig2_decode", "workspace layout exceeds the reservation");
    if (!R.empty()) LOCR_CHECK(hipMemcpyAsync(w.R, R.data(), sizeof(Jb2DevRegion) * R.size(), hipMemcpyHostToDevice, st));
    LOCR_CHECK(hipMemcpyAsync(w.P, P.data(), sizeof(Jb2DevPage) * n, hipMemcpyHostToDevice, st));
    if (z_total) LOCR_CHECK(hipMemcpyAsync(w.z, zs, z_total, hipMemcpyHostToDevice, st));
    LOCR_CHECK(hipEventRecord(stage.uploaded.get(), st));
    LOCR_CHECK(hipMemsetAsync(w.status, 0, sizeof(int) * n, st));   // (0 until an MMR region of the page says otherwise)
    if (any_arith) {
        LOCR_CHECK(locr_dyn_lds(reinterpret_cast<const void*>(jb2_generic), JB2_LDS_MAX));
        hipLaunchKernelGGL(jb2_generic, dim3((unsigned)R.size()), dim3(64), (size_t)JB2_LDS_FIXED + ((size_t)1 << top_bits), st, w.R, w.z, w.planes);
    }
    if (any_mmr) hipLaunchKernelGGL(jb2_mmr, dim3((unsigned)R.size()), dim3(64), 0, st, w.R, w.z, w.planes, w.status);
    hipLaunchKernelGGL(jb2_page, dim3((unsigned)height, (unsigned)n), dim3(256), 0, st, w.P, w.R, w.planes, w.status, out_dev, height, width);
    std::vector<int> dev_status((size_t)n);
    LOCR_CHECK(hipMemcpyAsync(dev_status.data(), w.status, sizeof(int) * n, hipMemcpyDeviceToHost, st));
    LOCR_CHECK(hipStreamSynchronize(st));
    LOCR_CHECK(hipGetLastError());
    for (int i = 0; i < n; ++i)
        if (P[(size_t)i].valid) status[i] = dev_status[(size_t)i];
    return 0;
}
