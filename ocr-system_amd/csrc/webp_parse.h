// WebP container walk (host only, no handle): RIFF / WEBP with one VP8L chunk, bare or inside a VP8X container.  Nothing of the image is
// decoded: the walk reads the chunk headers, the ten VP8X bytes and the five VP8L header bytes.  The rule is the other decoders' (DESIGN.md
// §4): status 0 is a promise of Pillow's bytes, so whatever a lenient and a strict reader could read differently is refused.
//   0  a file the device decodes
//  -2  valid WebP that is not read: lossy (VP8), an ALPH chunk, animation (ANIM / ANMF / the VP8X animation flag), more than
//      WP_MAX_PIXELS pixels, a VP8L chunk of WP_MAX_CHUNK bytes or more
//  -1  corrupt or irregular: no RIFF / WEBP signature, a RIFF size other than the file's (Pillow reads a file with bytes after the RIFF
//      payload; a strict reader need not), an odd RIFF size, a chunk or its padding byte past the file, a first chunk other than VP8X /
//      VP8L / VP8, chunks after the image of a file without VP8X, a VP8X chunk of another size than 10, a second VP8X or VP8L chunk, no
//      image chunk, reserved VP8X flag bits, a VP8L signature byte other than 0x2F, version bits other than 0, a VP8X canvas that differs from the VP8L header
// ICCP, EXIF, XMP and unknown chunks are skipped (convert('RGB') applies no profile); EXIF and XMP are reported.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

constexpr long long WP_MAX_PIXELS = 1ll << 26;   // 8192 x 8192; the longest lines (16384 x 1, 1 x 16384) are far inside
constexpr size_t WP_MAX_CHUNK = (size_t)1 << 28;  // bit positions stay inside 32 bits
constexpr char WP_REASON_LOSSY[] = "lossy WebP (VP8)";

struct WpInfo {
    int width, height, alpha, vp8x, exif, xmp;
    int lossy;              // status -2 for no other reason than the lossy format (a `VP8 ` chunk): vp8_parse.h takes such a file over
    size_t off, len;        // the VP8L payload in the file (status 0 only)
    const char* reason;     // "" for status 0
};

inline uint32_t wp_le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

inline int webp_probe(const uint8_t* f, size_t n, WpInfo* I) {
    memset(I, 0, sizeof(*I));
    I->reason = "";
    auto fail = [&](int rc, const char* why) { I->reason = why; return rc; };
    if (n < 12 || memcmp(f, "RIFF", 4) != 0 || memcmp(f + 8, "WEBP", 4) != 0) return fail(-1, "not a RIFF / WEBP file");
    const uint64_t riff = wp_le32(f + 4);
    if (riff + 8 > n) return fail(-1, "RIFF size past the file");
    if (riff + 8 < n) return fail(-1, "bytes after the RIFF payload");
    if (riff & 1) return fail(-1, "odd RIFF size");
    // pass 1: the chunk structure
    size_t p = 12;
    int nchunks = 0;
    while (p < n) {
        if (p + 8 > n) return fail(-1, "chunk header past the file");
        const uint64_t size = wp_le32(f + p + 4);
        if (size > 0x7FFFFFFFu || p + 8 + size + (size & 1) > n) return fail(-1, "chunk past the file");
        ++nchunks;
        p += 8 + (size_t)size + (size_t)(size & 1);
    }
    if (nchunks == 0) return fail(-1, "no chunk");
    // pass 2: what the chunks are
    const uint8_t* tag0 = f + 12;
    const size_t off0 = 20, size0 = wp_le32(f + 16);
    bool have = false, has_canvas = false;
    int cw = 0, ch = 0;
    const char* refused = nullptr;
    if (memcmp(tag0, "VP8X", 4) == 0) {
        I->vp8x = 1;
        if (size0 != 10) return fail(-1, "VP8X chunk of another size than 10");
        if (f[off0] & 0xC1) return fail(-1, "reserved VP8X flag bits set");   // (libwebp refuses them)
        if (f[off0] & 0x02) refused = "animated WebP";
        has_canvas = true;
        cw = 1 + (f[off0 + 4] | (f[off0 + 5] << 8) | (f[off0 + 6] << 16));
        ch = 1 + (f[off0 + 7] | (f[off0 + 8] << 8) | (f[off0 + 9] << 16));
        p = off0 + 10;
        while (p < n) {
            const uint8_t* tag = f + p;
            const size_t size = wp_le32(f + p + 4);
            if (memcmp(tag, "VP8X", 4) == 0) return fail(-1, "second VP8X chunk");
            if (memcmp(tag, "VP8L", 4) == 0) {
                if (have) return fail(-1, "second VP8L chunk");
                have = true; I->off = p + 8; I->len = size;
            } else if (memcmp(tag, "VP8 ", 4) == 0) { if (!refused) refused = WP_REASON_LOSSY; }
            else if (memcmp(tag, "ALPH", 4) == 0) { if (!refused) refused = "lossy WebP with an ALPH chunk"; }
            else if (memcmp(tag, "ANIM", 4) == 0 || memcmp(tag, "ANMF", 4) == 0) { if (!refused) refused = "animated WebP"; }
            else if (memcmp(tag, "EXIF", 4) == 0) I->exif = 1;
            else if (memcmp(tag, "XMP ", 4) == 0) I->xmp = 1;
            p += 8 + size + (size & 1);
        }
    } else if (memcmp(tag0, "VP8L", 4) == 0) {
        if (nchunks != 1) return fail(-1, "chunks after the image of a file without VP8X");
        have = true; I->off = off0; I->len = size0;
    } else if (memcmp(tag0, "VP8 ", 4) == 0) {
        if (nchunks != 1) return fail(-1, "chunks after the image of a file without VP8X");
        I->lossy = 1;
        return fail(-2, WP_REASON_LOSSY);
    } else {
        return fail(-1, "first chunk is neither VP8X, VP8L nor VP8");
    }
    if (refused) { I->off = I->len = 0; I->lossy = refused == WP_REASON_LOSSY; return fail(-2, refused); }
    if (!have) return fail(-1, "no image chunk");
    const uint8_t* s = f + I->off;
    if (I->len < 5 || s[0] != 0x2F) { I->off = I->len = 0; return fail(-1, "VP8L signature byte is not 0x2F"); }
    const uint32_t v = wp_le32(s + 1);
    if (v >> 29) { I->off = I->len = 0; return fail(-1, "VP8L version is not 0"); }
    I->width = 1 + (int)(v & 0x3FFF); I->height = 1 + (int)((v >> 14) & 0x3FFF); I->alpha = (int)((v >> 28) & 1);
    if (has_canvas && (cw != I->width || ch != I->height)) { I->off = I->len = 0; return fail(-1, "VP8X canvas differs from the VP8L header"); }
    if ((long long)I->width * I->height > WP_MAX_PIXELS) { I->off = I->len = 0; return fail(-2, "more than 2^26 pixels"); }
    if (I->len >= WP_MAX_CHUNK) { I->off = I->len = 0; return fail(-2, "VP8L chunk of 256 MB or more"); }
    return 0;
}
