// The WebP host parser (csrc/webp_parse.h) and the functions the kernels run (csrc/webp_dec.h, compiled here with one "lane") as a
// stand-alone program, so that the sanitizers can see them: tests/test_webp_sanitized.py builds this with -fsanitize=address,undefined.
//   webp_main PACK [RGB_OUT]
// PACK: files one after another, each a little-endian u32 length and its bytes.  One line per file on stdout:
//   status width height alpha vp8x exif xmp
// RGB_OUT: the RGB pixels of every file of status 0, one after another.  Every buffer is sized exactly (no slack), as far as the
// functions allow, so that a read or write past one is a report.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "webp_dec.h"
#include "webp_parse.h"

static int decode(const uint8_t* f, size_t n, WpInfo* I, std::vector<uint8_t>* rgb) {
    int rc = webp_probe(f, n, I);
    if (rc) return rc;
    const int w = I->width, h = I->height;
    std::vector<uint8_t> payload(f + I->off, f + I->off + I->len);   // (its own allocation: a read past the chunk is a report)
    std::vector<uint8_t> lens(WP_LENS);
    std::vector<uint32_t> cache(1 << WP_MAX_CACHE_BITS), stamp(1 << WP_MAX_CACHE_BITS);
    std::vector<uint16_t> cl(WP_CL_WORDS);
    static std::vector<uint16_t> tab(WP_TABLE_WORDS);   // (37 MB: once for all files; a group index is below WP_MAX_GROUPS by construction)
    std::vector<uint32_t> sub(wp_sub_words(w, h));
    std::vector<uint32_t> a((size_t)w * h), b((size_t)w * h);
    WpCtx c{};
    wp_bits_init(c.b, payload.data(), (uint32_t)payload.size(), 5);
    c.lens = lens.data(); c.cache = cache.data(); c.stamp = stamp.data(); c.cl = cl.data(); c.gfast = nullptr;
    c.tab = tab.data(); c.sub = sub.data(); c.sub_cap = (uint32_t)sub.size();
    WpHead H;
    wp_decode_stream(c, w, h, a.data(), &H);
    if (H.err) return H.err;
    const uint32_t* px = wp_untransform_host(H, sub.data(), w, h, a.data(), b.data());
    if (rgb) {
        rgb->resize((size_t)w * h * 3);
        for (size_t i = 0; i < (size_t)w * h; ++i) {
            (*rgb)[3 * i] = (uint8_t)(px[i] >> 16); (*rgb)[3 * i + 1] = (uint8_t)(px[i] >> 8); (*rgb)[3 * i + 2] = (uint8_t)px[i];
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: webp_main PACK [RGB_OUT]\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    FILE* out = argc > 2 ? fopen(argv[2], "wb") : nullptr;
    if (argc > 2 && !out) { perror(argv[2]); return 2; }
    uint8_t lb[4];
    while (fread(lb, 1, 4, in) == 4) {
        const size_t n = wp_le32(lb);
        std::vector<uint8_t> file(n);
        if (n && fread(file.data(), 1, n, in) != n) { fprintf(stderr, "short pack\n"); return 2; }
        WpInfo I;
        std::vector<uint8_t> rgb;
        const int rc = decode(file.data(), n, &I, out ? &rgb : nullptr);
        printf("%d %d %d %d %d %d %d\n", rc, I.width, I.height, I.alpha, I.vp8x, I.exif, I.xmp);
        if (rc == 0 && out) fwrite(rgb.data(), 1, rgb.size(), out);
    }
    fclose(in);
    if (out) fclose(out);
    return 0;
}
