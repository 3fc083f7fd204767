// JBIG2 (ITU-T T.88) host parser for the embedded organisation PDF's /JBIG2Decode uses (no HIP dependency; tests/jbig2_main.cpp
// compiles it alone): one page's stream, behind the segments of an optional /JBIG2Globals stream, with no file header.  It reads the
// generic-region subset: page information, immediate generic regions (arithmetic-coded with the four templates, adaptive pixels and
// typical prediction, or MMR), end of stripe / page / file; profiles and extensions are skipped.  It emits one record per region; no
// pixel is touched.  Status: 0 = the device subset, -2 = valid JBIG2 outside it (symbol dictionaries, text, halftone and refinement
// regions, ...), -1 = corrupt or irregular.  tests/jbig2_reference.py restates every check in the same order.
// The field widths and bit positions below are written from recollection of T.88, not checked against another decoder (README).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

constexpr int JB2_MAX_COLS = 8192;      // = CC_MAX_COLS (ccitt.h): the MMR regions run on the fax decoder's line stages
constexpr int JB2_MAX_REGIONS = 256;    // regions a page

struct Jb2Region {
    uint32_t off, len;        // the coded data inside its buffer (after the region's own header fields)
    int from_globals;         // 1: `off` counts in the globals stream
    uint32_t w, h, x, y;      // the region's bitmap and where its top left corner lies on the page
    int op;                   // 0 OR, 1 AND, 2 XOR, 3 XNOR, 4 REPLACE
    int mmr, tmpl, tpgd;
    int8_t at[8];             // (x, y) of A1..A4; templates 1-3 use the first pair
    int nominal;              // the AT pixels are where the standard puts them by default
};
struct Jb2Page {
    int info[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // width, height, regions, arithmetic regions, MMR regions, highest template, TPGDON anywhere, striped
    int width = 0, height = 0, default_pixel = 0, default_op = 0, override_ok = 0, striped = 0;
    const char* reason = "";
    std::vector<Jb2Region> regions;
};

namespace jb2p {

#define JB2_BAD(msg) do { pg->reason = msg; return -1; } while (0)
#define JB2_OUT(msg) do { pg->reason = msg; return -2; } while (0)

inline uint32_t be(const uint8_t* d, size_t p, int n) {
    uint32_t v = 0;
    for (int i = 0; i < n; ++i) v = (v << 8) | d[p + i];
    return v;
}

// the nominal AT positions of a template (the table in jbig2_dec.h)
inline void nominal_at(int tmpl, int8_t at[8]) {
    static const int8_t N0[8] = {3, -1, -3, -1, 2, -2, -2, -2};
    for (int i = 0; i < 8; ++i) at[i] = 0;
    if (tmpl == 0) { for (int i = 0; i < 8; ++i) at[i] = N0[i]; }
    else { at[0] = tmpl == 1 ? 3 : 2; at[1] = -1; }
}

struct State {
    bool have_page = false, height_known = false, have_stripe = false, stop = false;
    uint64_t page_h = 0, last_stripe = 0;
};

// the segments of one buffer, in order.  Every pass of the loop moves p forward by a whole segment (at least 11 bytes of header).
inline int segments(const uint8_t* d, size_t n, int from_globals, Jb2Page* pg, State& s) {
    size_t p = 0;
    while (p < n && !s.stop) {
        // ---- segment header
        if (n - p < 6) JB2_BAD("segment header past the stream");
        const uint32_t number = be(d, p, 4);
        const unsigned flags = d[p + 4];
        const int type = (int)(flags & 63);
        size_t q = p + 5;
        uint64_t count = d[q] >> 5;
        if (count == 5 || count == 6) JB2_BAD("reserved referred-to segment count");
        if (count == 7) {
            if (n - q < 4) JB2_BAD("segment header past the stream");
            count = be(d, q, 4) & 0x1FFFFFFFu;
            q += 4;
            const uint64_t retain = (count + 8) / 8;   // one bit for the segment itself and one per referred-to segment
            if (n - q < retain) JB2_BAD("segment header past the stream");
            q += (size_t)retain;
        } else {
            q += 1;
        }
        const uint64_t ref_bytes = count * (number <= 256 ? 1u : number <= 65536 ? 2u : 4u);
        if (n - q < ref_bytes) JB2_BAD("segment header past the stream");
        q += (size_t)ref_bytes;
        const int pa_size = (flags & 0x40) ? 4 : 1;
        if (n - q < (size_t)pa_size + 4) JB2_BAD("segment header past the stream");
        const uint32_t assoc = be(d, q, pa_size);
        q += (size_t)pa_size;
        const uint32_t len = be(d, q, 4);
        q += 4;
        // ---- what the segment is
        switch (type) {
            case 0: case 4: case 6: case 7: case 16: case 20: case 22: case 23: case 36: case 38: case 39: case 40: case 42: case 43:
            case 48: case 49: case 50: case 51: case 52: case 53: case 62: break;
            default: JB2_BAD("a segment type that T.88 does not define");
        }
        if (assoc > 1) JB2_OUT("a segment of another page than page 1");
        switch (type) {
            case 0: JB2_OUT("symbol dictionary");
            case 4: case 6: case 7: JB2_OUT("text region");
            case 16: JB2_OUT("pattern dictionary");
            case 20: case 22: case 23: JB2_OUT("halftone region");
            case 36: JB2_OUT("intermediate generic region");
            case 40: case 42: case 43: JB2_OUT("generic refinement region");
            case 53: JB2_OUT("code tables");
            default: break;
        }
        if (len == 0xFFFFFFFFu) JB2_OUT("a segment of unknown length");
        if (n - q < len) JB2_BAD("segment data past the stream");
        const size_t body = q, next = q + len;
        if (type == 48) {
            if (s.have_page) JB2_OUT("a second page information segment");
            if (len != 19) JB2_BAD("page information of the wrong length");
            const uint32_t w = be(d, body, 4), h = be(d, body + 4, 4);
            const unsigned pf = d[body + 16], striping = be(d, body + 17, 2);
            if (pf & 0x80) JB2_BAD("reserved page flag bits");
            if (w == 0 || h == 0) JB2_BAD("an empty page");
            if (w > (uint32_t)JB2_MAX_COLS) JB2_OUT("page wider than 8192");
            if (h != 0xFFFFFFFFu && h > 0x7FFFFFFFu) JB2_OUT("page higher than 2^31 - 1");
            s.have_page = true;
            s.height_known = h != 0xFFFFFFFFu;
            s.page_h = s.height_known ? h : 0;
            pg->width = (int)w; pg->height = (int)s.page_h;
            pg->default_pixel = (int)((pf >> 2) & 1); pg->default_op = (int)((pf >> 3) & 3); pg->override_ok = (int)((pf >> 6) & 1);
            pg->striped = (int)((striping >> 15) & 1);
            pg->info[0] = pg->width; pg->info[1] = pg->height; pg->info[7] = pg->striped;
        } else if (type == 38 || type == 39) {
            if (!s.have_page) JB2_BAD("a region before the page information");
            if (len < 18) JB2_BAD("generic region shorter than its header");
            Jb2Region r{};
            r.w = be(d, body, 4); r.h = be(d, body + 4, 4); r.x = be(d, body + 8, 4); r.y = be(d, body + 12, 4);
            const unsigned rf = d[body + 16], gf = d[body + 17];
            if ((rf & 0xF8) || (rf & 7) > 4) JB2_BAD("reserved region flag bits");
            if (gf & 0xE0) JB2_BAD("reserved generic region flag bits");
            if (gf & 0x10) JB2_OUT("extended template (EXTTEMPLATE)");
            r.op = (int)(rf & 7);
            if (!pg->override_ok && r.op != pg->default_op) JB2_BAD("a region operator other than the page's, which forbids overriding");
            r.mmr = (int)(gf & 1); r.tmpl = (int)((gf >> 1) & 3); r.tpgd = (int)((gf >> 3) & 1);
            size_t at_bytes = 0;
            nominal_at(r.tmpl, r.at);
            r.nominal = 1;
            if (!r.mmr) {
                at_bytes = r.tmpl == 0 ? 8 : 2;
                if (len < 18 + at_bytes) JB2_BAD("generic region shorter than its header");
                for (size_t i = 0; i < at_bytes; i += 2) {
                    const int ax = (int8_t)d[body + 18 + i], ay = (int8_t)d[body + 19 + i];
                    if (ay > 0 || (ay == 0 && ax >= 0)) JB2_BAD("an adaptive template pixel that is not before the current pixel");
                    if (r.at[i] != ax || r.at[i + 1] != ay) r.nominal = 0;
                    r.at[i] = (int8_t)ax; r.at[i + 1] = (int8_t)ay;
                }
            }
            if (r.w == 0 || r.h == 0) JB2_BAD("an empty region");
            if (r.w > (uint32_t)JB2_MAX_COLS) JB2_OUT("region wider than 8192");
            if (pg->regions.size() >= (size_t)JB2_MAX_REGIONS) JB2_OUT("more than 256 regions on the page");
            r.off = (uint32_t)(body + 18 + at_bytes); r.len = (uint32_t)(len - 18 - at_bytes);
            r.from_globals = from_globals;
            pg->regions.push_back(r);
            pg->info[2] += 1; pg->info[3] += !r.mmr; pg->info[4] += r.mmr;
            if (!r.mmr) {
                if (r.tmpl > pg->info[5]) pg->info[5] = r.tmpl;
                if (r.tpgd) pg->info[6] = 1;
            }
        } else if (type == 50) {
            if (len != 4) JB2_BAD("end of stripe of the wrong length");
            s.have_stripe = true;
            s.last_stripe = be(d, body, 4);
        } else if (type == 49 || type == 51) {
            s.stop = true;
        }   // 52 (profiles) and 62 (extension): skipped
        p = next;
    }
    return 0;
}

}  // namespace jb2p

// stream: the page's /JBIG2Decode data; globals: its /JBIG2Globals data or null.  Sizes are limited to 2^28 bytes each (-2 above).
inline int jbig2_parse(const uint8_t* stream, size_t size, const uint8_t* globals, size_t globals_size, Jb2Page* pg) {
    *pg = Jb2Page{};
    if (size >= ((size_t)1 << 28) || globals_size >= ((size_t)1 << 28)) JB2_OUT("a stream of 2^28 bytes or more");
    jb2p::State s;
    if (globals && globals_size) {
        const int rc = jb2p::segments(globals, globals_size, 1, pg, s);
        if (rc) return rc;
    }
    if (!s.stop) {
        const int rc = jb2p::segments(stream, size, 0, pg, s);
        if (rc) return rc;
    }
    if (!s.have_page) JB2_BAD("no page information");
    if (!s.height_known) {
        if (!s.have_stripe) JB2_BAD("unknown page height without an end of stripe");
        if (s.last_stripe + 1 > 0x7FFFFFFFull) JB2_OUT("page higher than 2^31 - 1");
        pg->height = (int)(s.last_stripe + 1);
        pg->info[1] = pg->height;
    }
    for (const Jb2Region& r : pg->regions)
        if (r.x >= (uint32_t)pg->width || r.y >= (uint32_t)pg->height) JB2_BAD("a region that does not meet the page");
    return 0;
}

#undef JB2_BAD
#undef JB2_OUT
