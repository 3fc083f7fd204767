// Lossy WebP (VP8 key frame) host parser (no handle): the container walk for a file with one `VP8 ` chunk, the 10-byte frame tag and the
// boolean-coded frame header (segments, filter, partitions, quantisers, coefficient probabilities, skip probability).  Its work does not
// grow with the page; everything per macroblock is device work (vp8_dec.h).  The rule is the other decoders' (DESIGN.md §4): status 0 is
// a promise of Pillow's bytes, so whatever a lenient and a strict reader could read differently is refused.
//   0  a file the device decodes (lossless: webp_parse.h decides; lossy: below)
//  -2  valid WebP that is not read: a lossy file with an ALPH chunk, animation, more than WP_MAX_PIXELS pixels, a chunk of
//      WP_MAX_CHUNK bytes or more
//  -1  corrupt or irregular: the container cases of webp_parse.h; both a VP8 and a VP8L chunk, a second VP8 chunk; a chunk shorter than
//      the 10-byte tag; an inter frame; a profile above 3; show_frame 0; a start code other than 9d 01 2a; a zero width or height; a
//      VP8X canvas that differs from the frame header; a first-partition length past the chunk; a partition-size table or a partition
//      past the chunk; an empty last partition (libwebp refuses it); any read of the first partition past its end, a partition that
//      begins with the byte 0xFF (vp8_dec.h says what a read past the end is, and why 0xFF is refused)
// libwebp ignores the two scale bits of each dimension, the colour-space bit and the clamping bit; so does this parser.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "vp8_dec.h"
#include "webp_parse.h"

struct Vp8Info {
    WpInfo wp;        // width, height, vp8x, exif, xmp; off / len: the VP8 (or VP8L) payload; reason
    int lossy, parts;
};

// the frame header of the VP8 payload s[0..len) -> F (everything the device needs but the bytes), 0 or -1 with *why
inline int vp8_parse_frame(const uint8_t* s, size_t len, Vp8Frame* F, const char** why) {
    memset(F, 0, sizeof(*F));
    auto fail = [&](const char* w) { *why = w; return -1; };
    if (len < 10) return fail("VP8 chunk shorter than the frame tag");
    const uint32_t tag = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);
    if (tag & 1) return fail("VP8 inter frame");
    if (((tag >> 1) & 7) > 3) return fail("VP8 profile above 3");
    if (!((tag >> 4) & 1)) return fail("VP8 show_frame is 0");
    const size_t part0 = tag >> 5;
    if (s[3] != 0x9d || s[4] != 0x01 || s[5] != 0x2a) return fail("VP8 start code is not 9d 01 2a");
    F->width = (s[6] | (s[7] << 8)) & 0x3fff;
    F->height = (s[8] | (s[9] << 8)) & 0x3fff;
    if (F->width == 0 || F->height == 0) return fail("VP8 frame of zero width or height");
    if (part0 >= len || part0 > len - 10) return fail("VP8 first partition past the chunk");
    F->mbw = (F->width + 15) >> 4; F->mbh = (F->height + 15) >> 4;
    Vp8Bool b;
    vp8_bool_init(b, s, 10, (uint32_t)(10 + part0));
    if (b.over) return fail("VP8 first partition begins outside the boolean coder's interval");
    vp8_get(b, s, 1);   // colour space
    vp8_get(b, s, 1);   // clamping type
    // segments (the state a key frame starts from: no segments, absolute values, all zero)
    int quant[4] = {0, 0, 0, 0}, fstr[4] = {0, 0, 0, 0}, absolute = 1;
    F->seg_p[0] = F->seg_p[1] = F->seg_p[2] = 255;
    const int use_segment = (int)vp8_get(b, s, 1);
    if (use_segment) {
        F->update_map = (int)vp8_get(b, s, 1);
        if (vp8_get(b, s, 1)) {
            absolute = (int)vp8_get(b, s, 1);
            for (int i = 0; i < 4; ++i) quant[i] = vp8_get(b, s, 1) ? vp8_get_signed(b, s, 7) : 0;
            for (int i = 0; i < 4; ++i) fstr[i] = vp8_get(b, s, 1) ? vp8_get_signed(b, s, 6) : 0;
        }
        if (F->update_map)
            for (int i = 0; i < 3; ++i) F->seg_p[i] = vp8_get(b, s, 1) ? (uint8_t)vp8_get(b, s, 8) : 255;
    }
    // loop filter
    const int simple = (int)vp8_get(b, s, 1);
    const int level = (int)vp8_get(b, s, 6);
    const int sharpness = (int)vp8_get(b, s, 3);
    const int use_lf_delta = (int)vp8_get(b, s, 1);
    int ref_delta[4] = {0, 0, 0, 0}, mode_delta[4] = {0, 0, 0, 0};
    if (use_lf_delta && vp8_get(b, s, 1)) {
        for (int i = 0; i < 4; ++i)
            if (vp8_get(b, s, 1)) ref_delta[i] = vp8_get_signed(b, s, 6);
        for (int i = 0; i < 4; ++i)
            if (vp8_get(b, s, 1)) mode_delta[i] = vp8_get_signed(b, s, 6);
    }
    F->filter_type = level == 0 ? 0 : simple ? 1 : 2;
    // token partitions
    F->parts = 1 << vp8_get(b, s, 2);
    {
        const size_t start = 10 + part0;
        if (len - start < 3 * (size_t)(F->parts - 1)) return fail("VP8 partition-size table past the chunk");
        size_t p = start + 3 * (size_t)(F->parts - 1);
        for (int k = 0; k < F->parts - 1; ++k) {
            const uint8_t* t = s + start + 3 * k;
            const size_t sz = (size_t)t[0] | ((size_t)t[1] << 8) | ((size_t)t[2] << 16);
            if (sz > len - p) return fail("VP8 token partition past the chunk");
            F->part_off[k] = (uint32_t)p; F->part_len[k] = (uint32_t)sz;
            p += sz;
        }
        if (p >= len) return fail("VP8 last token partition is empty");
        F->part_off[F->parts - 1] = (uint32_t)p; F->part_len[F->parts - 1] = (uint32_t)(len - p);
    }
    // quantisers
    const int base_q = (int)vp8_get(b, s, 7);
    int dq[5];   // y1 dc, y2 dc, y2 ac, uv dc, uv ac
    for (int i = 0; i < 5; ++i) dq[i] = vp8_get(b, s, 1) ? vp8_get_signed(b, s, 4) : 0;
    auto clip = [](int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; };
    for (int i = 0; i < 4; ++i) {
        int q = use_segment ? quant[i] + (absolute ? 0 : base_q) : base_q;
        int16_t* m = F->dq[i];
        m[0] = (int16_t)vp8_dc_q(clip(q + dq[0], 127));
        m[1] = (int16_t)vp8_ac_q(clip(q, 127));
        m[2] = (int16_t)(vp8_dc_q(clip(q + dq[1], 127)) * 2);
        m[3] = (int16_t)((vp8_ac_q(clip(q + dq[2], 127)) * 101581) >> 16);
        if (m[3] < 8) m[3] = 8;
        m[4] = (int16_t)vp8_dc_q(clip(q + dq[3], 117));
        m[5] = (int16_t)vp8_ac_q(clip(q + dq[4], 127));
    }
    // filter strengths per segment and macroblock kind (16x16 / 4x4); limit 0: the macroblock is not filtered
    for (int i = 0; i < 4; ++i)
        for (int i4 = 0; i4 < 2; ++i4) {
            Vp8Strength& fs = F->fs[i][i4];
            fs.limit = fs.ilevel = fs.hev = 0;
            if (!F->filter_type) continue;
            int lv = use_segment ? fstr[i] + (absolute ? 0 : level) : level;
            if (use_lf_delta) { lv += ref_delta[0]; if (i4) lv += mode_delta[0]; }
            lv = clip(lv, 63);
            if (lv > 0) {
                int il = lv;
                if (sharpness > 0) {
                    il >>= sharpness > 4 ? 2 : 1;
                    if (il > 9 - sharpness) il = 9 - sharpness;
                }
                if (il < 1) il = 1;
                fs.ilevel = (uint8_t)il; fs.limit = (uint8_t)(2 * lv + il);
                fs.hev = lv >= 40 ? 2 : lv >= 15 ? 1 : 0;
            }
        }
    vp8_get(b, s, 1);   // (the refresh flag of the probabilities: of no effect on a single frame)
    for (int i = 0; i < 1056; ++i) F->coef_p[i] = vp8_bit(b, s, vp8_coef_update(i)) ? (uint8_t)vp8_get(b, s, 8) : vp8_coef_default(i);
    F->use_skip = (int)vp8_get(b, s, 1);
    F->skip_p = F->use_skip ? (uint8_t)vp8_get(b, s, 8) : 0;
    if (b.over) return fail("VP8 frame header past the first partition");
    F->modes = b;
    return 0;
}

// the probe of both kinds: a lossless file as webp_probe reads it, and a still lossy file without ALPH
inline int vp8_probe(const uint8_t* f, size_t n, Vp8Info* I, Vp8Frame* F) {
    memset(I, 0, sizeof(*I));
    int rc = webp_probe(f, n, &I->wp);
    if (rc != -2 || !I->wp.lossy) return rc;
    I->wp.lossy = 0;
    auto fail = [&](int code, const char* why) { I->wp.off = I->wp.len = 0; I->wp.reason = why; return code; };
    // (webp_probe has checked the chunk structure)
    size_t off = 0, len = 0;
    if (I->wp.vp8x) {
        int have = 0, lossless = 0;
        const char* refused = nullptr;
        for (size_t p = 30; p < n;) {
            const uint8_t* tag = f + p;
            const size_t size = wp_le32(f + p + 4);
            if (memcmp(tag, "VP8 ", 4) == 0) { if (have++) return fail(-1, "second VP8 chunk"); off = p + 8; len = size; }
            else if (memcmp(tag, "VP8L", 4) == 0) lossless = 1;
            else if (memcmp(tag, "ALPH", 4) == 0) { if (!refused) refused = "lossy WebP with an ALPH chunk"; }
            else if (memcmp(tag, "ANIM", 4) == 0 || memcmp(tag, "ANMF", 4) == 0) { if (!refused) refused = "animated WebP"; }
            p += 8 + size + (size & 1);
        }
        if (lossless) return fail(-1, "both a VP8 and a VP8L chunk");
        if (refused) return fail(-2, refused);
    } else {
        off = 20; len = wp_le32(f + 16);
    }
    Vp8Frame local;
    if (!F) F = &local;
    const char* why = "";
    if (vp8_parse_frame(f + off, len, F, &why)) return fail(-1, why);
    const int cw = I->wp.vp8x ? 1 + (f[24] | (f[25] << 8) | (f[26] << 16)) : F->width;
    const int ch = I->wp.vp8x ? 1 + (f[27] | (f[28] << 8) | (f[29] << 16)) : F->height;
    I->wp.width = F->width; I->wp.height = F->height; I->wp.alpha = 0;
    if (cw != F->width || ch != F->height) return fail(-1, "VP8X canvas differs from the VP8 frame header");
    if ((long long)F->width * F->height > WP_MAX_PIXELS) return fail(-2, "more than 2^26 pixels");
    if (len >= WP_MAX_CHUNK) return fail(-2, "VP8 chunk of 256 MB or more");
    I->wp.off = off; I->wp.len = len; I->wp.reason = "";
    I->lossy = 1; I->parts = F->parts;
    return 0;
}
