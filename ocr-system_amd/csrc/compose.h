// Page composition (lumina_ocr_page_compose; the definition is restated in tests/pdf_layers_reference.py): a scanned PDF page painted
// from several images (strips, a stencil over a background, images with soft or explicit masks; utils/pdf_pages.py finds them) is put
// together on the device from the decoded layers.  The layer check (compose_params_ok) and the function that paints one layer onto one
// pixel (compose_pixel) are plain functions: compose.hip runs the second on the device, tests/compose_main.cpp compiles both for the
// host, where the sanitizers can see them.  Integer arithmetic throughout: the result does not depend on the order anything runs in.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/lumina_ocr.h"

#ifdef __HIPCC__
#define COMPOSE_HD __host__ __device__
#else
#define COMPOSE_HD
#endif

typedef lumina_ocr_compose_layer ComposeLayer;

constexpr int COMPOSE_MAX_LAYERS = 64;        // layers of one page (the kernel lists them in LDS, one lane of a wave each)
constexpr int COMPOSE_MAX_SIDE = 65535;       // canvas, source and mask sides
constexpr int COMPOSE_MAX_COORD = 1 << 24;    // |rectangle coordinate|: (2 * (x - x0) + 1) * w then stays below 2^42

// The sample that holds a pixel centre (PDF's rule without /Interpolate): pixel d of a span of `span` pixels that shows `w` samples
// -> floor((2 d + 1) w / (2 span)), 0 <= d < span.  A span of exactly w pixels is the identity and pays for no division; the
// quotient needs 64 bits only when 2 * span * w does not fit 32 (the numerator is below that product).
COMPOSE_HD inline int compose_map(int d, int span, int w) {
    if (span == w) return d;
    const uint64_t num = (uint64_t)(2 * (int64_t)d + 1) * (uint64_t)w, den = 2 * (uint64_t)span;
    if (den * (uint64_t)w <= 0xffffffffull) return (int)((uint32_t)num / (uint32_t)den);
    return (int)(num / den);
}

COMPOSE_HD inline uint32_t compose_div255(uint32_t t) { return (t + 128 + ((t + 128) >> 8)) >> 8; }

// Layer L painted onto pixel (x, y) of its page, whose colour so far is c (r | g << 8 | b << 16) -> the colour after it.  Sources
// and masks are [h][w][3] RGB as the decoders write them; a mask is read from channel 0.  An index is formed only inside the
// rectangle, where compose_params_ok's limits keep every one inside its image.
COMPOSE_HD inline uint32_t compose_pixel(uint32_t c, const ComposeLayer& L, int x, int y) {
    if (x < L.x0 || x >= L.x1 || y < L.y0 || y >= L.y1) return c;
    const int dx = x - L.x0, dy = y - L.y0, sx = L.x1 - L.x0, sy = L.y1 - L.y0;
    uint32_t m = 0;
    if (L.kind != 0) {
        const int mu = compose_map(dx, sx, L.mw), mv = compose_map(dy, sy, L.mh);
        m = L.mask[((size_t)mv * (size_t)L.mw + (size_t)mu) * 3];
        if (L.flip) m = 255 - m;
        if (L.kind == 1) return m < 128 ? (uint32_t)L.fill : c;
        if (L.kind == 3 && m >= 128) return c;
    }
    const int u = compose_map(dx, sx, L.w), v = compose_map(dy, sy, L.h);
    const uint8_t* s = L.src + ((size_t)v * (size_t)L.w + (size_t)u) * 3;
    const uint32_t r = s[0], g = s[1], b = s[2];
    if (L.kind != 2) return r | g << 8 | b << 16;
    const uint32_t a = m, na = 255 - m;
    return compose_div255(r * a + (c & 255) * na) | compose_div255(g * a + (c >> 8 & 255) * na) << 8 |
           compose_div255(b * a + (c >> 16 & 255) * na) << 16;
}

// nullptr, or what is wrong with the table: the reason the entry reports before it launches anything
inline const char* compose_params_why(const ComposeLayer* layers, int m, int n, int H, int W) {
    if (n < 0 || m < 0 || (m > 0 && !layers)) return "negative counts or a null table";
    if (H <= 0 || W <= 0 || H > COMPOSE_MAX_SIDE || W > COMPOSE_MAX_SIDE) return "canvas sides must be 1..65535";
    int page = -1, on_page = 0;
    for (int i = 0; i < m; ++i) {
        const ComposeLayer& L = layers[i];
        if (L.page < 0 || L.page >= n) return "a layer's page is outside 0..n-1";
        if (L.page < page) return "layers are not grouped by page in ascending order";
        on_page = L.page == page ? on_page + 1 : 1;
        page = L.page;
        if (on_page > COMPOSE_MAX_LAYERS) return "more than 64 layers on one page";
        if (L.kind < 0 || L.kind > 3) return "layer kind must be 0..3";
        if (L.flip != 0 && L.flip != 1) return "layer polarity must be 0 or 1";
        if (L.fill < 0 || L.fill > 0xffffff) return "fill colour must be 0..0xffffff";
        const int32_t co[4] = {L.x0, L.y0, L.x1, L.y1};
        for (int k = 0; k < 4; ++k)
            if (co[k] < -COMPOSE_MAX_COORD || co[k] > COMPOSE_MAX_COORD) return "rectangle coordinate beyond +-2^24";
        if (L.x0 >= L.x1 || L.y0 >= L.y1) return "empty rectangle";
        if (L.x0 >= W || L.x1 <= 0 || L.y0 >= H || L.y1 <= 0) return "rectangle outside the canvas";
        if (L.kind != 1 && (!L.src || L.w <= 0 || L.h <= 0 || L.w > COMPOSE_MAX_SIDE || L.h > COMPOSE_MAX_SIDE))
            return "an image layer needs a source of 1..65535 samples a side";
        if (L.kind != 0 && (!L.mask || L.mw <= 0 || L.mh <= 0 || L.mw > COMPOSE_MAX_SIDE || L.mh > COMPOSE_MAX_SIDE))
            return "a masked layer needs a mask of 1..65535 samples a side";
    }
    return nullptr;
}
inline bool compose_params_ok(const ComposeLayer* layers, int m, int n, int H, int W) { return compose_params_why(layers, m, n, H, W) == nullptr; }

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
// out [n][H][W][3]; layers: DEVICE, the table compose_params_ok accepted; first: DEVICE int [n + 1], layers first[p] .. first[p + 1] - 1
// are page p's, in paint order.  Launches nothing for a table it has not been shown to be safe: the caller checks.
hipError_t page_compose_launch(const ComposeLayer* layers, const int* first, int n, int H, int W, uint8_t* out, hipStream_t st);
struct lumina_ocr;
// the entry behind lumina_ocr_page_compose: checks the HOST table, copies it through the engine's pinned staging and workspace, launches
int page_compose_run(lumina_ocr* eng, const ComposeLayer* layers, int m, int n, int H, int W, uint8_t* out, hipStream_t st);
#endif
