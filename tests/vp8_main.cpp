// The lossy-WebP host parser (csrc/vp8_parse.h) and the functions the kernels run (csrc/vp8_dec.h), in raster order, as a stand-alone
// program, so that the sanitizers can see them: tests/test_vp8_sanitized.py builds this with -fsanitize=address,undefined.
//   vp8_main PACK [RGB_OUT]
// PACK: files one after another, each a little-endian u32 length and its bytes.  One line per file on stdout:
//   status width height lossy parts vp8x exif xmp
// RGB_OUT: the RGB pixels of every lossy file of status 0, one after another (a lossless file is probed, not decoded).  Every buffer is
// sized exactly, so that a read or write past one is a report.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vp8_dec.h"
#include "vp8_parse.h"

static int decode(const uint8_t* f, size_t n, Vp8Info* I, std::vector<uint8_t>* rgb) {
    Vp8Frame F;
    int rc = vp8_probe(f, n, I, &F);
    if (rc || !I->lossy) return rc;
    std::vector<uint8_t> s(f + I->wp.off, f + I->wp.off + I->wp.len);   // (its own allocation: a read past the chunk is a report)
    const int mbw = F.mbw, mbh = F.mbh, ys = 16 * mbw, uvs = 8 * mbw;
    std::vector<Vp8Mb> mbs((size_t)mbw * mbh);
    std::vector<uint8_t> top(4 * (size_t)mbw), tnz(mbw), tdc(mbw);
    if ((rc = vp8_mode_walk(F, s.data(), mbs.data(), top.data())) != 0) return rc;
    std::vector<int16_t> coefs((size_t)mbw * mbh * VP8_MB_COEFS, 0);
    Vp8Bool pb[8];
    int16_t y2[16];
    if ((rc = vp8_token_walk(F, s.data(), mbs.data(), coefs.data(), tnz.data(), tdc.data(), pb, y2)) != 0) return rc;
    std::vector<uint32_t> yb((size_t)ys * 16 * mbh / 4), ub((size_t)uvs * 8 * mbh / 4), vb((size_t)uvs * 8 * mbh / 4);   // (aligned for the word stores)
    uint8_t *Y = (uint8_t*)yb.data(), *U = (uint8_t*)ub.data(), *V = (uint8_t*)vb.data();
    for (int y = 0; y < mbh; ++y)
        for (int x = 0; x < mbw; ++x) {
            const Vp8Mb& m = mbs[(size_t)y * mbw + x];
            const int16_t* c = coefs.data() + ((size_t)y * mbw + x) * VP8_MB_COEFS;
            for (int k = 0; k < 16; ++k) vp8_recon_luma(F, m, c, x, y, k, Y, ys);
            for (int k = 0; k < 8; ++k) vp8_recon_chroma(m, c, x, y, k, U, V, uvs);
        }
    if (F.filter_type)
        for (int y = 0; y < mbh; ++y)
            for (int x = 0; x < mbw; ++x)
                for (int step = 0; step < 4; ++step)
                    for (int lane = 0; lane < 16; ++lane) vp8_filter_step(F, mbs[(size_t)y * mbw + x], x, y, step, lane, Y, U, V, ys, uvs);
    if (rgb) {
        rgb->resize((size_t)F.width * F.height * 3);
        for (int y = 0; y < F.height; ++y)
            for (int x = 0; x < F.width; ++x) vp8_rgb_px(Y, U, V, ys, uvs, F.width, F.height, x, y, rgb->data() + ((size_t)y * F.width + x) * 3);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: vp8_main PACK [RGB_OUT]\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    FILE* out = argc > 2 ? fopen(argv[2], "wb") : nullptr;
    if (argc > 2 && !out) { perror(argv[2]); return 2; }
    uint8_t lb[4];
    while (fread(lb, 1, 4, in) == 4) {
        const size_t n = wp_le32(lb);
        std::vector<uint8_t> file(n);
        if (n && fread(file.data(), 1, n, in) != n) { fprintf(stderr, "short pack\n"); return 2; }
        Vp8Info I;
        std::vector<uint8_t> rgb;
        const int rc = decode(file.data(), n, &I, out ? &rgb : nullptr);
        printf("%d %d %d %d %d %d %d %d\n", rc, I.wp.width, I.wp.height, I.lossy, I.parts, I.wp.vp8x, I.wp.exif, I.wp.xmp);
        if (rc == 0 && I.lossy && out) fwrite(rgb.data(), 1, rgb.size(), out);
    }
    fclose(in);
    if (out) fclose(out);
    return 0;
}
