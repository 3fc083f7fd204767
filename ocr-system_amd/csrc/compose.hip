// Page composition on the device: the kernel behind lumina_ocr_page_compose (definition: compose.h, include/lumina_ocr.h).
//
// Memory-bound: a page is written once and every pixel reads the three bytes of each layer that holds it.  The work of one
// work-group is a band of whole rows of one page (about PC_TILE pixels).
//   * Wave 0 first lists in LDS, in paint order (ballot + prefix count), the layers of the page whose rectangles meet the band's rows.
//     The layer loop of every pixel then runs over that list alone, with a trip count and records that are the same for the whole
//     work-group: a page cut into strips reads one layer per pixel, not one rectangle test per strip.
//   * A band is a run of consecutive bytes of the output.  Its pixels are painted one per lane, neighbouring lanes on neighbouring
//     pixels, so that the byte loads of a source row fall into two or three cache lines per wave instruction, and the colours go to an
//     LDS tile of 4096 pixels (12 KB).  The tile leaves with 16-byte stores, neighbouring lanes 16 bytes apart.  Rows of 3 W bytes are
//     aligned to nothing, so the tiles are cut where the byte offset in the whole output is a multiple of 48 (16 pixels, three 16-byte
//     words); the up to 15 pixels of a band before the first and after the last cut are written bytewise by the band that owns them.
//     Every byte is written exactly once, by the band its row belongs to.
//   * Pixel coordinates cost one 32-bit division per thread and tile (the 16 pixels of a thread are 256 apart: stepped); the sample
//     maps cost none when a layer is shown sample for pixel, one 32-bit division each otherwise (compose_map).
// No register array, no scratch; LDS 4 KB of layer records + 12 KB tile.
#include "compose.h"

#include <cstring>
#include <vector>

#include "common.h"
#include "engine.h"

namespace {

constexpr int PC_THREADS = 256, PC_PER_THREAD = 16, PC_TILE = PC_THREADS * PC_PER_THREAD;

__device__ __forceinline__ uint32_t pc_paint(const ComposeLayer* lay, int nl, int x, int y) {
    uint32_t c = 0xffffff;
    for (int k = 0; k < nl; ++k) c = compose_pixel(c, lay[k], x, y);
    return c;
}

__global__ __launch_bounds__(PC_THREADS) void pc_compose_kernel(const ComposeLayer* __restrict__ layers, const int* __restrict__ first, int p0, int H,
                                                                 int W, int rows, int vec, uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) ComposeLayer lay[COMPOSE_MAX_LAYERS];
    __shared__ uint4 tile[PC_TILE * 3 / 16];
    __shared__ int nl_s;
    const int t = threadIdx.x, p = p0 + blockIdx.y;
    const int r0 = blockIdx.x * rows, r1 = min(H, r0 + rows);
    if (t < 64) {   // wave 0: the layers that meet rows r0 .. r1 - 1, kept in paint order
        const int f = first[p], cnt = min(first[p + 1] - f, COMPOSE_MAX_LAYERS);
        const bool touch = t < cnt && layers[f + t].y0 < r1 && layers[f + t].y1 > r0;
        const unsigned long long b = __ballot(touch);
        if (touch) {   // the 64-byte record as four 16-byte words, global to LDS
            static_assert(sizeof(ComposeLayer) == 64, "a layer record is four 16-byte words");
            const uint4* g = reinterpret_cast<const uint4*>(layers + f + t);
            uint4* d = reinterpret_cast<uint4*>(&lay[__popcll(b & ((1ull << t) - 1ull))]);
            for (int k = 0; k < 4; ++k) d[k] = g[k];
        }
        if (t == 0) nl_s = __popcll(b);
    }
    __syncthreads();
    const int nl = nl_s;

    const uint64_t page_px = (uint64_t)p * (uint64_t)H * (uint64_t)W;
    uint8_t* const po = out + page_px * 3;
    // positions along the page are counted from `o` pixels before its first one, so that a multiple of 16 is a 48-byte boundary of out
    const uint32_t o = vec ? (uint32_t)(page_px & 15) : 0u;
    const uint32_t a = o + (uint32_t)r0 * (uint32_t)W, b = o + (uint32_t)r1 * (uint32_t)W;   // < 65535^2 + 16
    uint32_t v0 = (a + 15u) & ~15u, v1 = b & ~15u;
    if (!vec || v0 > v1) v0 = v1 = b;   // no 48-byte boundary inside the band, or an output that is not 16-byte aligned: all bytewise

    const int step_y = PC_THREADS / W, step_x = PC_THREADS % W;
    uint8_t* const tl = reinterpret_cast<uint8_t*>(tile);
    for (uint32_t tb = v0; tb < v1; tb += PC_TILE) {
        const uint32_t cnt = min((uint32_t)PC_TILE, v1 - tb);   // a multiple of 16
        const uint32_t q = tb - o + (uint32_t)t;
        int y = (int)(q / (uint32_t)W), x = (int)(q - (uint32_t)y * (uint32_t)W);
#pragma unroll 4
        for (int j = 0; j < PC_PER_THREAD; ++j) {
            const uint32_t i = (uint32_t)t + (uint32_t)(PC_THREADS * j);
            if (i < cnt) {   // (then y < r1: the pixel is inside the band)
                const uint32_t c = pc_paint(lay, nl, x, y);
                tl[3 * i] = (uint8_t)c; tl[3 * i + 1] = (uint8_t)(c >> 8); tl[3 * i + 2] = (uint8_t)(c >> 16);
            }
            x += step_x; y += step_y;
            if (x >= W) { x -= W; ++y; }
        }
        __syncthreads();
        uint4* const dst = reinterpret_cast<uint4*>(po + (size_t)(tb - o) * 3);
        const uint32_t words = cnt * 3 / 16;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t wd = (uint32_t)t + (uint32_t)(PC_THREADS * k);
            if (wd < words) dst[wd] = tile[wd];
        }
        __syncthreads();
    }
    // the pixels before the first and after the last boundary (at most 15 each; the whole band when there is none)
    for (int part = 0; part < 2; ++part) {
        const uint32_t s = part ? max(v1, v0) : a, e = part ? b : min(v0, b);
        for (uint32_t q = s + (uint32_t)t; q < e; q += PC_THREADS) {
            const uint32_t pp = q - o;
            const int y = (int)(pp / (uint32_t)W), x = (int)(pp - (uint32_t)y * (uint32_t)W);
            const uint32_t c = pc_paint(lay, nl, x, y);
            uint8_t* d = po + (size_t)pp * 3;
            d[0] = (uint8_t)c; d[1] = (uint8_t)(c >> 8); d[2] = (uint8_t)(c >> 16);
        }
    }
}

}  // namespace

hipError_t page_compose_launch(const ComposeLayer* layers, const int* first, int n, int H, int W, uint8_t* out, hipStream_t st) {
    if (!first || !out || n <= 0 || H <= 0 || W <= 0 || H > COMPOSE_MAX_SIDE || W > COMPOSE_MAX_SIDE) return hipErrorInvalidValue;
    const int rows = W >= PC_TILE ? 1 : PC_TILE / W;
    const int vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    for (int p0 = 0; p0 < n; p0 += 32768) {   // (the page is a grid dimension)
        const int np = n - p0 < 32768 ? n - p0 : 32768;
        hipLaunchKernelGGL(pc_compose_kernel, dim3((unsigned)((H + rows - 1) / rows), (unsigned)np), dim3(PC_THREADS), 0, st, layers, first, p0, H, W, rows,
                           vec, out);
    }
    return hipGetLastError();
}

int page_compose_run(lumina_ocr* eng, const ComposeLayer* layers, int m, int n, int H, int W, uint8_t* out, hipStream_t st) {
    if (n == 0) return 0;
    if (!out) return locr_fail(eng, "page_compose", "null output");
    if (const char* why = compose_params_why(layers, m, n, H, W)) return locr_fail(eng, "page_compose", why);
    if ((size_t)n >= ((size_t)1 << 24)) return locr_fail(eng, "page_compose", "too many pages");
    // first[p]: the first layer of page p (the table is grouped by page, ascending)
    std::vector<int> first((size_t)n + 1, m);
    {
        int at = 0;
        for (int p = 0; p <= n; ++p) {
            while (at < m && layers[at].page < p) ++at;
            first[(size_t)p] = at;
        }
    }
    lumina_ocr::Staging& stage = eng->pc_stage;
    if (!stage.uploaded) {
        hipEvent_t ev = nullptr;
        LOCR_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        stage.uploaded.reset(ev);
    }
    // one layout for the pinned copy and the device copy: the records, then the page index
    const size_t lay_bytes = (sizeof(ComposeLayer) * (size_t)m + 255) & ~(size_t)255, total = lay_bytes + sizeof(int) * ((size_t)n + 1);
    // (the event is recorded after the kernel: it guards the pinned buffer and the device table of the previous call alike)
    LOCR_CHECK(hipEventSynchronize(stage.uploaded.get()));
    LOCR_CHECK(stage.buf.reserve(total, stage.uploaded.get()));
    LOCR_CHECK(eng->pc_table.reserve(total, stage.uploaded.get()));
    uint8_t* hs = stage.buf.get();
    if (m) memcpy(hs, layers, sizeof(ComposeLayer) * (size_t)m);
    memset(hs + sizeof(ComposeLayer) * (size_t)m, 0, lay_bytes - sizeof(ComposeLayer) * (size_t)m);
    memcpy(hs + lay_bytes, first.data(), sizeof(int) * ((size_t)n + 1));
    uint8_t* dv = eng->pc_table.get();
    LOCR_CHECK(hipMemcpyAsync(dv, hs, total, hipMemcpyHostToDevice, st));
    const hipError_t e = page_compose_launch(reinterpret_cast<const ComposeLayer*>(dv), reinterpret_cast<const int*>(dv + lay_bytes), n, H, W, out, st);
    LOCR_CHECK(hipEventRecord(stage.uploaded.get(), st));
    if (e != hipSuccess) return locr_fail(eng, "page_compose", hipGetErrorString(e));
    return 0;
}
