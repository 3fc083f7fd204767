// JPEG 2000 host parser (no HIP dependency; tests/jp2_parse_main.cpp compiles it alone): the boxes of a JP2 / JPX-baseline file, the
// main header and the tile-part headers, then the walk over every packet in progression order (tier 2: inclusion and zero-bit-plane
// tag trees, coding-pass counts, Lblock, segment lengths, the bit stuffing after 0xFF).  It emits one record per code-block; no pixel
// is touched.  Status: 0 = the device subset, -2 = valid outside it, -1 = corrupt or irregular (the parser is strict: where OpenJPEG
// is lenient the file is refused).  tests/jp2_reference.py restates every check in the same order.  With `irreversible`
// the 9/7 transform is taken too (expounded step sizes: Jp2File::irreversible, Jp2Block::hs); tests/jp2_irreversible_reference.py
// restates that form.  With JP2_TAKE_TILES it also reads image and tile origins, a grid of up to 4096 tiles whose tile-parts come in
// any order, and user precinct sizes: the geometry is then in canvas coordinates (Jp2File::tiles, Jp2Block::tile) and each tile has its
// own packet walk, in any of the five progression orders over several precincts; tests/jp2_tiles_reference.py restates that form.
// Without the flag every status and reason is what it was.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

constexpr int JP2_MAX_SIDE = 16384;
constexpr long long JP2_MAX_PIXELS = 1ll << 26;
constexpr int JP2_MAX_LAYERS = 32;
constexpr int JP2_MAX_LEVELS = 6;
constexpr int JP2_MAX_MB = 15;   // magnitude bit-planes of a block: its magnitudes (one fractional bit more) are 16-bit words
constexpr int JP2_MAX_BLOCKS = 1 << 20;
constexpr int JP2_MAX_TILES = 4096;
constexpr uint32_t JP2_MAX_CANVAS = 1u << 30;   // Xsiz, Ysiz: the canvas arithmetic is in int
constexpr unsigned JP2_TAKE_IRREVERSIBLE = 1, JP2_TAKE_TILES = 2;   // what jp2_parse takes beyond the first subset

struct Jp2Seg { size_t off; uint32_t len; int next; };   // one layer's contribution to a block; next: index of the following one, -1 at the end
struct Jp2Block {
    int comp, res, orient;      // orient: 0 LL, 1 HL, 2 LH, 3 HH
    int bx, by;                 // position in the sub-band's code-block grid
    int x, y, w, h;             // rectangle in the component's plane (image coordinates): each tile-component owns its rectangle of the
                                // plane, its sub-bands laid out inside it as the transform reads them (low-pass part top left)
    int tile;                   // index in Jp2File::tiles
    int mb, zbp, passes;        // Mb of the sub-band, zero bit-planes, coding passes in all layers
    int seg_head, seg_tail, nseg;
    int included, lblock;
    float hs;                   // 9/7: half the step size of its sub-band (the magnitudes are in half units); 0 for 5/3
};
struct Jp2Tile { int x0, y0, x1, y1; };   // canvas corners of a tile (no sub-sampling: of each of its tile-components too)
struct Jp2File {
    int info[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // width, height, components, levels, layers, progression order, code-block width, height
    int x0 = 0, y0 = 0;        // the image origin on the canvas (XOsiz, YOsiz); width and height are the image area's
    std::vector<Jp2Tile> tiles;
    int ppx[33] = {}, ppy[33] = {};   // precinct size exponents per resolution (15: none given)
    std::vector<int> part_tile;       // the tile of each entry of parts
    int width = 0, height = 0, comps = 0, levels = 0, layers = 0, order = 0, cbw = 0, cbh = 0, mct = 0;
    int mb[3 * 32 + 1] = {};   // Mb per sub-band, in the QCD's order
    int irreversible = 0;      // 1: the 9/7 transform; step[] then holds the step size per sub-band, in the QCD's order
    float step[3 * 32 + 1] = {};
    const char* reason = "";
    std::vector<Jp2Block> blocks;
    std::vector<Jp2Seg> segs;
    std::vector<std::pair<size_t, size_t>> parts;   // [start, end) of each tile-part's packet data
};

namespace jp2p {

#define JP2_BAD(msg) do { f->reason = msg; return -1; } while (0)
#define JP2_OUT(msg) do { f->reason = msg; return -2; } while (0)

inline uint64_t be(const uint8_t* d, size_t p, int n) {
    uint64_t v = 0;
    for (int i = 0; i < n; ++i) v = (v << 8) | d[p + i];
    return v;
}
inline bool is4(const uint8_t* d, size_t p, const char* t) { return memcmp(d + p, t, 4) == 0; }

// the boxes of jp2h between p and end -> box[4] = {height, width, components, enumerated colour space}
inline int jp2h(const uint8_t* d, size_t p, size_t end, Jp2File* f, uint32_t box[4]) {
    bool have_ihdr = false, have_colr = false, first = true;
    uint32_t hh = 0, ww = 0, nc = 0, bpc = 0, colr = 0;
    while (p < end) {
        if (p + 8 > end) JP2_BAD("box header past the end of jp2h");
        const uint64_t ln = be(d, p, 4);
        if (ln < 8 || ln > end - p) JP2_BAD("box length outside jp2h");
        const size_t b = p + 8, e = p + (size_t)ln;
        const bool ihdr = is4(d, p + 4, "ihdr");
        if (first != ihdr) JP2_BAD("ihdr is not the first box of jp2h");
        first = false;
        if (ihdr) {
            if (e - b != 14) JP2_BAD("ihdr of the wrong length");
            hh = (uint32_t)be(d, b, 4); ww = (uint32_t)be(d, b + 4, 4); nc = (uint32_t)be(d, b + 8, 2); bpc = d[b + 10];
            if (d[b + 11] != 7) JP2_BAD("ihdr compression type is not 7");
            have_ihdr = true;
        } else if (is4(d, p + 4, "colr")) {
            if (have_colr) JP2_OUT("more than one colr box");
            if (e - b < 3) JP2_BAD("colr of the wrong length");
            if (d[b] == 2) JP2_OUT("colr with an ICC profile");
            if (d[b] != 1) JP2_BAD("colr method");
            if (e - b != 7) JP2_BAD("colr of the wrong length");
            colr = (uint32_t)be(d, b + 3, 4);
            if (colr == 18) JP2_OUT("sYCC colour space");
            if (colr != 16 && colr != 17) JP2_OUT("enumerated colour space outside sRGB / grey");
            have_colr = true;
        } else if (is4(d, p + 4, "res ")) {
        } else {
            JP2_OUT("a jp2h box outside the subset (pclr, cmap, cdef, opct, bpcc ...)");
        }
        p = e;
    }
    if (!have_ihdr || !have_colr) JP2_BAD("jp2h without ihdr or colr");
    if (bpc != 7) JP2_OUT("bit depth other than 8 unsigned");
    if (nc != 1 && nc != 3) JP2_OUT("component count other than 1 or 3");
    if ((nc == 3) != (colr == 16)) JP2_OUT("colour space does not match the component count");
    box[0] = hh; box[1] = ww; box[2] = nc; box[3] = colr;
    return 0;
}

// -> [*s, *e) of the codestream; *boxed: box[] is filled from jp2h
inline int find_codestream(const uint8_t* d, size_t n, Jp2File* f, size_t* s, size_t* e, bool* boxed, uint32_t box[4]) {
    static const uint8_t sig[12] = {0, 0, 0, 12, 'j', 'P', ' ', ' ', 13, 10, 0x87, 10};
    *boxed = false;
    if (n >= 4 && d[0] == 0xFF && d[1] == 0x4F && d[2] == 0xFF && d[3] == 0x51) { *s = 0; *e = n; return 0; }
    if (n < 12 || memcmp(d, sig, 12) != 0) JP2_BAD("not a JPEG 2000 file");
    size_t p = 12;
    bool seen_ftyp = false, have_hdr = false;
    for (;;) {
        if (p + 8 > n) JP2_BAD("no codestream box");
        uint64_t ln = be(d, p, 4);
        size_t hl = 8;
        if (ln == 1) {
            if (p + 16 > n) JP2_BAD("box header past the end of the file");
            ln = be(d, p + 8, 8); hl = 16;
        } else if (ln == 0) {
            ln = n - p;
        }
        if (ln < hl || ln > n - p) JP2_BAD("box length outside the file");
        const size_t body = p + hl, end = p + (size_t)ln;
        if (is4(d, p + 4, "ftyp")) {
            if (seen_ftyp || p != 12 || end - body < 8 || (end - body) % 4) JP2_BAD("irregular ftyp box");
            seen_ftyp = true;
            bool ok = is4(d, body, "jp2 ");
            if (!ok && is4(d, body, "jpx "))
                for (size_t q = body + 8; q < end; q += 4) ok |= is4(d, q, "jp2 ") || is4(d, q, "jpxb");
            if (!ok) JP2_OUT("ftyp brand is neither jp2 nor baseline jpx");
        } else if (is4(d, p + 4, "jp2h")) {
            if (!seen_ftyp || have_hdr) JP2_BAD("jp2h out of order");
            const int rc = jp2h(d, body, end, f, box);
            if (rc) return rc;
            have_hdr = true;
        } else if (is4(d, p + 4, "jp2c")) {
            if (!have_hdr) JP2_BAD("jp2c before jp2h");
            *s = body; *e = end; *boxed = true;
            return 0;
        } else {
            if (!seen_ftyp) JP2_BAD("box before ftyp");
            if (!(is4(d, p + 4, "rreq") || is4(d, p + 4, "xml ") || is4(d, p + 4, "uuid") || is4(d, p + 4, "uinf") || is4(d, p + 4, "jp2i")))
                JP2_OUT("a top-level box outside the subset");
        }
        p = end;
    }
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

inline const char* outside_marker(unsigned m) {
    switch (m) {
        case 0xFF5F: return "POC marker";
        case 0xFF5E: return "RGN marker";
        case 0xFF60: return "PPM marker";
        case 0xFF61: return "PPT marker";
        case 0xFF57: return "PLM marker";
        case 0xFF63: return "CRG marker";
        case 0xFF58: return "PLT marker in the main header";
        case 0xFF55: return "TLM marker in a tile-part header";
        case 0xFF52: return "COD marker in a tile-part header";
        case 0xFF5C: return "QCD marker in a tile-part header";
        case 0xFF53: return "COC marker in a tile-part header";
        case 0xFF5D: return "QCC marker in a tile-part header";
    }
    return nullptr;
}

inline int parse_headers(const uint8_t* d, size_t s, size_t e, bool boxed, const uint32_t box[4], Jp2File* f, unsigned take) {
    const bool irreversible = take & JP2_TAKE_IRREVERSIBLE, tiled = take & JP2_TAKE_TILES;
    if (e - s < 4 || !(d[s] == 0xFF && d[s + 1] == 0x4F && d[s + 2] == 0xFF && d[s + 3] == 0x51)) JP2_BAD("no SOC + SIZ");
    size_t p = s + 4;
    if (p + 2 > e) JP2_BAD("SIZ cut short");
    size_t L = (size_t)be(d, p, 2);
    if (L < 41 || p + L > e) JP2_BAD("SIZ of the wrong length");
    const uint32_t rsiz = (uint32_t)be(d, p + 2, 2), X = (uint32_t)be(d, p + 4, 4), Y = (uint32_t)be(d, p + 8, 4), XO = (uint32_t)be(d, p + 12, 4),
                   YO = (uint32_t)be(d, p + 16, 4), XT = (uint32_t)be(d, p + 20, 4), YT = (uint32_t)be(d, p + 24, 4), XTO = (uint32_t)be(d, p + 28, 4),
                   YTO = (uint32_t)be(d, p + 32, 4), C = (uint32_t)be(d, p + 36, 2);
    f->info[0] = X > 0x7FFFFFFFu ? 0x7FFFFFFF : (int)X; f->info[1] = Y > 0x7FFFFFFFu ? 0x7FFFFFFF : (int)Y; f->info[2] = (int)C;
    if (C == 0 || L != 38 + 3 * (size_t)C) JP2_BAD("SIZ of the wrong length");
    if (X == 0 || Y == 0 || XT == 0 || YT == 0) JP2_BAD("SIZ with an empty image or tile");
    if (rsiz != 0) JP2_OUT("capabilities (Rsiz) other than 0");
    if (!tiled) {
        if (XO || YO || XTO || YTO) JP2_OUT("non-zero image or tile origin");
        if (XT < X || YT < Y) JP2_OUT("more than one tile");
    } else {
        if (XO >= X || YO >= Y) JP2_BAD("image origin outside the reference grid");
        if (XTO > XO || YTO > YO || (uint64_t)XTO + XT <= XO || (uint64_t)YTO + YT <= YO) JP2_BAD("origins that leave the first tile empty");
        if (X > JP2_MAX_CANVAS || Y > JP2_MAX_CANVAS) JP2_OUT("reference grid larger than the decoder takes");
        // (XTO <= XO < X: the counts are formed without a sum that could pass 32 bits, XTsiz may be anything up to 2^32 - 1)
        if ((uint64_t)((X - XTO - 1) / XT + 1) * ((Y - YTO - 1) / YT + 1) > (uint64_t)JP2_MAX_TILES) JP2_OUT("more than 4096 tiles");
    }
    if (C != 1 && C != 3) JP2_OUT("component count other than 1 or 3");
    for (uint32_t c = 0; c < C; ++c) {
        const unsigned ssiz = d[p + 38 + 3 * c], xr = d[p + 39 + 3 * c], yr = d[p + 40 + 3 * c];
        if (xr == 0 || yr == 0) JP2_BAD("SIZ with zero sub-sampling");
        if (ssiz != 7) JP2_OUT("bit depth other than 8 unsigned");
        if (xr != 1 || yr != 1) JP2_OUT("sub-sampled components");
    }
    const uint32_t W = X - XO, H = Y - YO;   // the image area (without JP2_TAKE_TILES the origins are 0)
    if (tiled) { f->info[0] = (int)W; f->info[1] = (int)H; }
    if (W > (uint32_t)JP2_MAX_SIDE || H > (uint32_t)JP2_MAX_SIDE || (long long)W * H > JP2_MAX_PIXELS) JP2_OUT("image larger than the decoder takes");
    if (boxed && (box[0] != H || box[1] != W || box[2] != C)) JP2_BAD("ihdr disagrees with SIZ");
    f->width = (int)W; f->height = (int)H; f->comps = (int)C; f->x0 = (int)XO; f->y0 = (int)YO;
    if (!tiled) {
        f->tiles.push_back({0, 0, (int)X, (int)Y});
    } else {
        const uint32_t ntx = (X - XTO - 1) / XT + 1, nty = (Y - YTO - 1) / YT + 1;
        for (uint32_t ty = 0; ty < nty; ++ty)
            for (uint32_t tx = 0; tx < ntx; ++tx) {
                const uint64_t ax = (uint64_t)XTO + (uint64_t)tx * XT, ay = (uint64_t)YTO + (uint64_t)ty * YT;
                f->tiles.push_back({(int)std::max<uint64_t>(ax, XO), (int)std::max<uint64_t>(ay, YO), (int)std::min<uint64_t>(ax + XT, X),
                                    (int)std::min<uint64_t>(ay + YT, Y)});
            }
    }
    p += L;
    size_t cod = 0, codn = 0, qcd = 0, qcdn = 0;
    bool have_cod = false, have_qcd = false;
    std::vector<std::pair<size_t, size_t>> cocs, qccs;
    for (;;) {
        if (p + 4 > e) JP2_BAD("main header cut short");
        const unsigned m = (unsigned)be(d, p, 2);
        L = (size_t)be(d, p + 2, 2);
        if (m == 0xFF90) break;
        if (m < 0xFF00) JP2_BAD("not a marker in the main header");
        if (L < 2 || p + 2 + L > e) JP2_BAD("marker segment of the wrong length");
        const size_t b = p + 4, n = L - 2;
        if (m == 0xFF52) {
            if (have_cod) JP2_BAD("second COD");
            if (L < 12) JP2_BAD("COD of the wrong length");
            have_cod = true; cod = b; codn = n;
        } else if (m == 0xFF5C) {
            if (have_qcd) JP2_BAD("second QCD");
            if (L < 4) JP2_BAD("QCD of the wrong length");
            have_qcd = true; qcd = b; qcdn = n;
        } else if (m == 0xFF53) {
            cocs.push_back({b, n});
        } else if (m == 0xFF5D) {
            qccs.push_back({b, n});
        } else if (m == 0xFF64 || m == 0xFF55) {   // COM, TLM
        } else if (outside_marker(m)) {
            JP2_OUT(outside_marker(m));
        } else {
            JP2_BAD("unknown marker in the main header");
        }
        p = b + n;
    }
    if (!have_cod || !have_qcd) JP2_BAD("main header without COD or QCD");
    const unsigned scod = d[cod], order = d[cod + 1], layers = (unsigned)be(d, cod + 2, 2), mct = d[cod + 4], levels = d[cod + 5], xcb = d[cod + 6],
                   ycb = d[cod + 7], style = d[cod + 8], xform = d[cod + 9];
    if ((scod & ~7u) || order > 4 || mct > 1 || layers == 0 || xcb > 15 || ycb > 15 || xform > 1 || levels > 32 || (style & ~63u))
        JP2_BAD("COD field out of range");
    if (codn != ((scod & 1) ? 10 + (size_t)levels + 1 : 10)) JP2_BAD("COD of the wrong length");
    if (xcb > 8 || ycb > 8 || xcb + ycb > 8) JP2_BAD("code-block size out of range");
    f->order = (int)order; f->layers = (int)layers; f->mct = (int)mct; f->levels = (int)levels; f->cbw = 4 << xcb; f->cbh = 4 << ycb;
    f->info[3] = f->levels; f->info[4] = f->layers; f->info[5] = f->order; f->info[6] = f->cbw; f->info[7] = f->cbh;
    if ((scod & 1) && !tiled) JP2_OUT("user precinct sizes");
    for (unsigned r = 0; r <= levels && r < 33; ++r) {
        f->ppx[r] = (scod & 1) ? d[cod + 10 + r] & 15 : 15;
        f->ppy[r] = (scod & 1) ? d[cod + 10 + r] >> 4 : 15;
        if (r && (f->ppx[r] == 0 || f->ppy[r] == 0)) JP2_BAD("precinct of one sample above resolution 0");
    }
    if (scod & 6) JP2_OUT("SOP or EPH markers");
    if (xform == 0 && !irreversible) JP2_OUT("the 9/7 irreversible transform");
    f->irreversible = xform == 0;
    if (style) JP2_OUT("code-block style bits");
    if (f->cbw > 64 || f->cbh > 64) JP2_OUT("code-block side over 64");
    if (f->layers > JP2_MAX_LAYERS) JP2_OUT("more than 32 layers");
    if (f->levels > JP2_MAX_LEVELS) JP2_OUT("more than 6 decomposition levels");
    if (mct && C != 3) JP2_BAD("component transform on a one-component image");
    // (OpenJPEG leaves a 9/7 line of one sample unscaled and its encoder writes none: such a file cannot be pinned)
    if (f->irreversible)
        for (const Jp2Tile& T : f->tiles)
            for (int r = 1; r <= f->levels; ++r) {
                const int sh = f->levels - r;
                if (cdiv(T.x1, 1 << sh) - cdiv(T.x0, 1 << sh) == 1 || cdiv(T.y1, 1 << sh) - cdiv(T.y0, 1 << sh) == 1)
                    JP2_OUT("the 9/7 transform over a line of one sample");
            }
    const size_t nb = 3 * (size_t)levels + 1;
    const unsigned sq = d[qcd];
    if ((sq & 31) > 2) JP2_BAD("QCD style out of range");
    const int guard = (int)(sq >> 5);
    if (!f->irreversible) {
        if (sq & 31) JP2_OUT("quantised (scalar) step sizes with the reversible transform");
        if (qcdn != 1 + nb) JP2_BAD("QCD of the wrong length");
    } else {
        if ((sq & 31) != 2) JP2_OUT("the 9/7 transform with derived or no quantisation");
        if (qcdn != 1 + 2 * nb) JP2_BAD("QCD of the wrong length");
    }
    for (size_t i = 0; i < nb; ++i) {
        int expn;
        if (!f->irreversible) {
            if (d[qcd + 1 + i] & 7) JP2_BAD("QCD exponent byte with mantissa bits");
            expn = d[qcd + 1 + i] >> 3;
        } else {   // expounded: 5 bits of exponent, 11 of mantissa; the step is formed in double and rounded once, as OpenJPEG does
            const unsigned v = (unsigned)be(d, qcd + 1 + 2 * i, 2);
            expn = (int)(v >> 11);
            f->step[i] = (float)((1.0 + (v & 0x7FF) / 2048.0) * std::ldexp(1.0, 8 - expn));
        }
        const int mb = guard + expn - 1;
        if (mb < 0) JP2_BAD("sub-band without magnitude bits");
        if (mb > JP2_MAX_MB) JP2_OUT("more magnitude bit-planes than the decoder takes");
        f->mb[i] = mb;
    }
    for (const auto& c : cocs) {
        if (c.second < 2 || d[c.first] >= C) JP2_BAD("COC of the wrong length or component");
        const unsigned sc = d[c.first + 1];
        if ((sc & 1) != (scod & 1) || (sc & ~1u) || c.second - 2 != codn - 5 || memcmp(d + c.first + 2, d + cod + 5, codn - 5) != 0)
            JP2_OUT("COC that differs from COD");
    }
    for (const auto& c : qccs) {
        if (c.second < 2 || d[c.first] >= C) JP2_BAD("QCC of the wrong length or component");
        if (c.second - 1 != qcdn || memcmp(d + c.first + 1, d + qcd, qcdn) != 0) JP2_OUT("QCC that differs from QCD");
    }
    // tile-parts: of any tile of the grid, in any order; TPsot counts up within its own tile
    const size_t nt = f->tiles.size();
    std::vector<int> next_tp(nt, 0), total(nt, 0);
    for (;;) {
        if (p + 12 > e) JP2_BAD("SOT cut short");
        if (be(d, p, 2) != 0xFF90 || be(d, p + 2, 2) != 10) JP2_BAD("SOT expected");
        const unsigned isot = (unsigned)be(d, p + 4, 2), tpsot = d[p + 10], tnsot = d[p + 11];
        const uint64_t psot = be(d, p + 6, 4);
        if (isot >= nt) JP2_BAD(tiled ? "tile index outside the grid" : "tile index past the only tile");
        if ((int)tpsot != next_tp[isot] || (tnsot && tpsot >= tnsot)) JP2_BAD("tile-parts out of order");
        if (tiled && tnsot) {
            if (total[isot] && total[isot] != (int)tnsot) JP2_BAD("tile-part count changes within a tile");
            total[isot] = (int)tnsot;
        }
        if ((psot && psot < 14) || (psot && psot > e - 2 - p)) JP2_BAD("tile-part length outside the file");
        const size_t pend = psot ? p + (size_t)psot : e - 2;
        size_t q = p + 12;
        for (;;) {
            if (q + 2 > pend) JP2_BAD("tile-part header cut short");
            const unsigned m = (unsigned)be(d, q, 2);
            if (m == 0xFF93) { q += 2; break; }
            if (q + 4 > pend) JP2_BAD("tile-part header cut short");
            L = (size_t)be(d, q + 2, 2);
            if (m < 0xFF00) JP2_BAD("not a marker in the tile-part header");
            if (L < 2 || q + 2 + L > pend) JP2_BAD("marker segment of the wrong length");
            if (m == 0xFF64 || m == 0xFF58) {   // COM, PLT
            } else if (outside_marker(m)) {
                JP2_OUT(outside_marker(m));
            } else {
                JP2_BAD("unknown marker in a tile-part header");
            }
            q += 2 + L;
        }
        f->parts.push_back({q, pend});
        f->part_tile.push_back((int)isot);
        p = pend;
        if (++next_tp[isot] > 255) JP2_BAD("too many tile-parts");
        if (p + 2 <= e && be(d, p, 2) == 0xFFD9) break;
    }
    if (p + 2 != e) JP2_BAD("data after EOC");
    if (tiled)
        for (size_t t = 0; t < nt; ++t) {
            if (next_tp[t] == 0) JP2_BAD("tile without a tile-part");
            if (total[t] && total[t] != next_tp[t]) JP2_BAD("fewer tile-parts than the tile announces");
        }
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------ tier 2
struct Bits {   // the packet-header bit reader: after a 0xFF byte the next byte carries 7 bits
    const uint8_t* d; size_t p, end; unsigned buf = 0; int ct = 0; bool fail = false;
    void bytein() {
        if (p >= end) { fail = true; ct = 8; buf = 0; return; }
        ct = buf == 0xFF ? 7 : 8;
        buf = d[p++];
    }
    int bit() {
        if (ct == 0) bytein();
        --ct;
        return (int)(buf >> ct) & 1;
    }
    unsigned bits(int n) {
        unsigned v = 0;
        for (int i = 0; i < n; ++i) v = (v << 1) | (unsigned)bit();
        return v;
    }
    size_t align() {
        ct = 0;
        if (buf == 0xFF) { bytein(); ct = 0; }
        return p;
    }
};

struct TagTree {
    struct Level { int off, nx, ny; };
    std::vector<Level> levels;
    std::vector<int> value, low;
    void init(int nx, int ny) {
        int off = 0;
        for (;;) {
            levels.push_back({off, nx, ny});
            off += nx * ny;
            if (nx * ny <= 1) break;
            nx = (nx + 1) / 2; ny = (ny + 1) / 2;
        }
        value.assign((size_t)off, 1 << 30);
        low.assign((size_t)off, 0);
    }
    bool decode(Bits& bio, int x, int y, int threshold) {
        int path[16];
        const int nl = (int)levels.size();
        for (int i = 0; i < nl; ++i) { path[i] = levels[(size_t)i].off + y * levels[(size_t)i].nx + x; x >>= 1; y >>= 1; }
        int lo = 0;
        for (int i = nl - 1; i >= 0 && !bio.fail; --i) {
            const size_t node = (size_t)path[i];
            if (lo > low[node]) low[node] = lo; else lo = low[node];
            while (lo < threshold && lo < value[node] && !bio.fail) {
                if (bio.bit()) value[node] = lo; else ++lo;
            }
            low[node] = lo;
        }
        return value[(size_t)path[0]] < threshold;
    }
};

struct Band { int first, nx, ny; TagTree incl, zbpt; };   // first: index of its first block in Jp2File::blocks

inline int npasses(Bits& bio) {
    if (!bio.bit()) return 1;
    if (!bio.bit()) return 2;
    unsigned v = bio.bits(2);
    if (v != 3) return 3 + (int)v;
    v = bio.bits(5);
    if (v != 31) return 6 + (int)v;
    return 37 + (int)bio.bits(7);
}

inline int ilog2(int v) { int n = 0; while (v > 1) { v >>= 1; ++n; } return n; }

// bands[(c * (levels + 1) + r) * 3 + k]; resolution 0 has one band
inline int geometry(Jp2File* f, std::vector<Band>& bands) {
    const int R = f->levels + 1;
    bands.resize((size_t)f->comps * R * 3);
    for (int c = 0; c < f->comps; ++c)
        for (int r = 0; r < R; ++r) {
            const int rw = cdiv(f->width, 1 << (f->levels - r)), rh = cdiv(f->height, 1 << (f->levels - r));
            const int lw = cdiv(rw, 2), lh = cdiv(rh, 2);
            for (int k = 0; k < (r ? 3 : 1); ++k) {
                const int orient = r ? k + 1 : 0;
                const int x0 = (orient & 1) ? lw : 0, y0 = (orient & 2) ? lh : 0;
                const int w = !r ? rw : (orient & 1) ? rw - lw : lw, h = !r ? rh : (orient & 2) ? rh - lh : lh;
                Band& B = bands[((size_t)c * R + r) * 3 + k];
                B.first = (int)f->blocks.size();
                B.nx = w && h ? cdiv(w, f->cbw) : 0;
                B.ny = w && h ? cdiv(h, f->cbh) : 0;
                if ((long long)B.nx * B.ny + (long long)f->blocks.size() > JP2_MAX_BLOCKS) JP2_OUT("more code-blocks than the decoder takes");
                for (int by = 0; by < B.ny; ++by)
                    for (int bx = 0; bx < B.nx; ++bx) {
                        Jp2Block K;
                        K.comp = c; K.res = r; K.orient = orient; K.bx = bx; K.by = by; K.tile = 0;
                        K.x = x0 + bx * f->cbw; K.y = y0 + by * f->cbh;
                        K.w = w - bx * f->cbw < f->cbw ? w - bx * f->cbw : f->cbw;
                        K.h = h - by * f->cbh < f->cbh ? h - by * f->cbh : f->cbh;
                        K.mb = f->mb[r ? 3 * r - 3 + orient : 0]; K.zbp = 0; K.passes = 0;
                        K.hs = f->irreversible ? 0.5f * f->step[r ? 3 * r - 3 + orient : 0] : 0.0f;
                        K.seg_head = K.seg_tail = -1; K.nseg = 0; K.included = 0; K.lblock = 3;
                        f->blocks.push_back(K);
                    }
                B.incl.init(B.nx, B.ny); B.zbpt.init(B.nx, B.ny);
            }
        }
    return 0;
}

// where the packet walk stands: byte `pos` of tile-part `part` of `parts` (a tile's own tile-parts, in file order), which ends at pend
struct Cursor {
    const std::vector<std::pair<size_t, size_t>>* parts; size_t part, pos, pend;
    void skip_empty() { while (pos == pend && part + 1 < parts->size()) { ++part; pos = (*parts)[part].first; pend = (*parts)[part].second; } }
};

// one packet: the contribution of `layer` to the blocks of the nb bands of one precinct
inline int packet(const uint8_t* d, Jp2File* f, Band* pb, int nb, int layer, Cursor& cur, std::vector<std::pair<int, uint32_t>>& got) {
    cur.skip_empty();
    const size_t pend = cur.pend;
    Bits bio{d, cur.pos, pend};
    got.clear();
    if (bio.bit()) {
        for (int bi = 0; bi < nb; ++bi) {
            Band& B = pb[bi];
            for (int j = 0; j < B.nx * B.ny; ++j) {
                Jp2Block& K = f->blocks[(size_t)(B.first + j)];
                const int inc = !K.included ? (int)B.incl.decode(bio, K.bx, K.by, layer + 1) : bio.bit();
                if (bio.fail) JP2_BAD("packet header runs past its tile-part");
                if (!inc) continue;
                if (!K.included) {
                    int i = 1;
                    while (!B.zbpt.decode(bio, K.bx, K.by, i)) {
                        if (bio.fail) JP2_BAD("packet header runs past its tile-part");
                        if (++i > K.mb + 1) JP2_BAD("zero bit-plane count above Mb");
                    }
                    K.zbp = i - 1;
                    K.included = 1;
                }
                const int n = npasses(bio);
                while (bio.bit()) {
                    if (bio.fail) JP2_BAD("packet header runs past its tile-part");
                    if (++K.lblock > 32) JP2_BAD("Lblock out of range");
                }
                if (bio.fail) JP2_BAD("packet header runs past its tile-part");
                K.passes += n;
                if (K.passes > 3 * (K.mb - K.zbp) - 2) JP2_BAD("more coding passes than the bit-planes hold");
                const int nbits = K.lblock + ilog2(n);
                uint64_t ln = 0;
                for (int i = 0; i < nbits; ++i) ln = (ln << 1) | (uint64_t)bio.bit();
                if (bio.fail) JP2_BAD("packet header runs past its tile-part");
                if (ln > 0xFFFFFFFFull) JP2_BAD("segment length outside the tile-part");
                got.push_back({B.first + j, (uint32_t)ln});
            }
        }
    }
    if (bio.fail) JP2_BAD("packet header runs past its tile-part");
    size_t pos = bio.align();
    if (bio.fail) JP2_BAD("packet header runs past its tile-part");
    for (const auto& g : got) {
        Jp2Block& K = f->blocks[(size_t)g.first];
        if (g.second > pend - pos) JP2_BAD("segment length outside the tile-part");
        if (K.nseg >= JP2_MAX_LAYERS) JP2_BAD("too many segments");
        const int si = (int)f->segs.size();
        f->segs.push_back({pos, g.second, -1});
        if (K.seg_tail >= 0) f->segs[(size_t)K.seg_tail].next = si; else K.seg_head = si;
        K.seg_tail = si; ++K.nseg;
        pos += g.second;
    }
    cur.pos = pos;
    return 0;
}

inline int packets_end(Jp2File* f, Cursor& cur) {
    cur.skip_empty();
    if (cur.pos != cur.pend || cur.part + 1 != cur.parts->size()) JP2_BAD("data left over after the last packet");
    return 0;
}

inline int tier2(const uint8_t* d, Jp2File* f, std::vector<Band>& bands) {
    const int R = f->levels + 1, C = f->comps, Ly = f->layers;
    Cursor cur{&f->parts, 0, f->parts[0].first, f->parts[0].second};
    std::vector<std::pair<int, uint32_t>> got;
    const long long npk = (long long)Ly * R * C;
    for (long long k = 0; k < npk; ++k) {
        int layer, r, c;   // one precinct per resolution, all at position (0, 0): PCRL and CPRL visit the packets in the same order
        if (f->order == 0) { c = (int)(k % C); r = (int)(k / C % R); layer = (int)(k / C / R); }
        else if (f->order == 1) { c = (int)(k % C); layer = (int)(k / C % Ly); r = (int)(k / C / Ly); }
        else if (f->order == 2) { layer = (int)(k % Ly); c = (int)(k / Ly % C); r = (int)(k / Ly / C); }
        else { layer = (int)(k % Ly); r = (int)(k / Ly % R); c = (int)(k / Ly / R); }
        const int rc = packet(d, f, &bands[((size_t)c * R + r) * 3], r ? 3 : 1, layer, cur, got);
        if (rc) return rc;
    }
    return packets_end(f, cur);
}

// ---- JP2_TAKE_TILES: the geometry in canvas coordinates.  A precinct is up to three bands with a code-block grid and two tag trees each.
struct Precinct {
    int comp, res, index;   // index: raster position in the precinct grid of its resolution
    int X, Y;               // the canvas position at which the position-first orders visit it
    int first_band, nb;     // its bands in the tile's band list
};

inline int fdiv(int a, int sh) { return a >> sh; }
inline int cdivp(int a, int sh) { return (int)(((long long)a + (1ll << sh) - 1) >> sh); }

// the precincts and bands of tile t, its blocks appended to f->blocks
inline int geometry_tile(Jp2File* f, int t, std::vector<Precinct>& precs, std::vector<Band>& bands) {
    const Jp2Tile T = f->tiles[(size_t)t];
    const int Lv = f->levels;
    for (int c = 0; c < f->comps; ++c)
        for (int r = 0; r <= Lv; ++r) {
            const int sh = Lv - r;
            const int rx0 = cdivp(T.x0, sh), ry0 = cdivp(T.y0, sh), rx1 = cdivp(T.x1, sh), ry1 = cdivp(T.y1, sh);
            if (rx1 <= rx0 || ry1 <= ry0) continue;
            const int ppx = f->ppx[r], ppy = f->ppy[r];
            const int gx0 = fdiv(rx0, ppx), gy0 = fdiv(ry0, ppy), npx = cdivp(rx1, ppx) - gx0, npy = cdivp(ry1, ppy) - gy0;
            // the low-pass counts of this resolution (the size of the one below) place HL / LH / HH inside the tile's rectangle
            const int lw = cdivp(rx1, 1) - cdivp(rx0, 1), lh = cdivp(ry1, 1) - cdivp(ry0, 1);
            const int xe = std::min(ilog2(f->cbw), r ? ppx - 1 : ppx), ye = std::min(ilog2(f->cbh), r ? ppy - 1 : ppy);
            if ((long long)npx * npy + (long long)f->blocks.size() > JP2_MAX_BLOCKS) JP2_OUT("more code-blocks than the decoder takes");
            for (int py = 0; py < npy; ++py)
                for (int px = 0; px < npx; ++px) {
                    Precinct Q;
                    Q.comp = c; Q.res = r; Q.index = py * npx + px;
                    Q.X = px == 0 && (rx0 & ((1 << ppx) - 1)) ? T.x0 : (int)(((long long)(gx0 + px) << ppx) << sh);
                    Q.Y = py == 0 && (ry0 & ((1 << ppy) - 1)) ? T.y0 : (int)(((long long)(gy0 + py) << ppy) << sh);
                    Q.first_band = (int)bands.size(); Q.nb = r ? 3 : 1;
                    for (int k = 0; k < Q.nb; ++k) {
                        const int orient = r ? k + 1 : 0, xob = orient & 1, yob = orient >> 1;
                        int bx0 = rx0, by0 = ry0, bx1 = rx1, by1 = ry1;                                            // the band, in its own coordinates
                        long long qx0 = (long long)(gx0 + px) << ppx, qy0 = (long long)(gy0 + py) << ppy, qw = 1ll << ppx, qh = 1ll << ppy;   // the precinct, in the band's
                        if (r) {
                            const int nbl = sh + 1;
                            bx0 = cdivp(T.x0 - (xob << (nbl - 1)), nbl); bx1 = cdivp(T.x1 - (xob << (nbl - 1)), nbl);
                            by0 = cdivp(T.y0 - (yob << (nbl - 1)), nbl); by1 = cdivp(T.y1 - (yob << (nbl - 1)), nbl);
                            qx0 >>= 1; qy0 >>= 1; qw >>= 1; qh >>= 1;
                        }
                        const int ax0 = (int)std::max<long long>(qx0, bx0), ay0 = (int)std::max<long long>(qy0, by0);
                        const int ax1 = (int)std::min<long long>(qx0 + qw, bx1), ay1 = (int)std::min<long long>(qy0 + qh, by1);
                        Band B;
                        B.first = (int)f->blocks.size();
                        const bool some = ax1 > ax0 && ay1 > ay0;
                        const int cx0 = some ? fdiv(ax0, xe) : 0, cy0 = some ? fdiv(ay0, ye) : 0;
                        B.nx = some ? cdivp(ax1, xe) - cx0 : 0;
                        B.ny = some ? cdivp(ay1, ye) - cy0 : 0;
                        if ((long long)B.nx * B.ny + (long long)f->blocks.size() > JP2_MAX_BLOCKS) JP2_OUT("more code-blocks than the decoder takes");
                        for (int by = 0; by < B.ny; ++by)
                            for (int bx = 0; bx < B.nx; ++bx) {
                                Jp2Block K;
                                K.comp = c; K.res = r; K.orient = orient; K.bx = bx; K.by = by; K.tile = t;
                                const int kx0 = std::max((cx0 + bx) << xe, ax0), ky0 = std::max((cy0 + by) << ye, ay0);
                                const int kx1 = std::min((cx0 + bx + 1) << xe, ax1), ky1 = std::min((cy0 + by + 1) << ye, ay1);
                                K.x = T.x0 - f->x0 + (r && xob ? lw : 0) + kx0 - bx0;
                                K.y = T.y0 - f->y0 + (r && yob ? lh : 0) + ky0 - by0;
                                K.w = kx1 - kx0; K.h = ky1 - ky0;
                                K.mb = f->mb[r ? 3 * r - 3 + orient : 0]; K.zbp = 0; K.passes = 0;
                                K.hs = f->irreversible ? 0.5f * f->step[r ? 3 * r - 3 + orient : 0] : 0.0f;
                                K.seg_head = K.seg_tail = -1; K.nseg = 0; K.included = 0; K.lblock = 3;
                                f->blocks.push_back(K);
                            }
                        B.incl.init(B.nx, B.ny); B.zbpt.init(B.nx, B.ny);
                        bands.push_back(std::move(B));
                    }
                    precs.push_back(Q);
                }
        }
    return 0;
}

// Every tile in turn: its geometry, then its packets from its own tile-parts.  The position-first orders (RPCL, PCRL, CPRL) visit a
// precinct at the canvas position that is a multiple of its projected size, or at the tile's origin where that origin is no multiple
// (Precinct::X, Y): sorting by that position is the walk over positions.
inline int tier2_tiles(const uint8_t* d, Jp2File* f) {
    std::vector<std::pair<int, uint32_t>> got;
    const int Ly = f->layers, order = f->order;
    std::vector<std::vector<std::pair<size_t, size_t>>> tparts(f->tiles.size());
    for (size_t i = 0; i < f->parts.size(); ++i) tparts[(size_t)f->part_tile[i]].push_back(f->parts[i]);
    for (int t = 0; t < (int)f->tiles.size(); ++t) {
        std::vector<Precinct> precs;
        std::vector<Band> bands;
        int rc = geometry_tile(f, t, precs, bands);
        if (rc) return rc;
        const std::vector<std::pair<size_t, size_t>>& parts = tparts[(size_t)t];
        std::stable_sort(precs.begin(), precs.end(), [order](const Precinct& a, const Precinct& b) {
            if (order <= 1) return a.res != b.res ? a.res < b.res : a.comp != b.comp ? a.comp < b.comp : a.index < b.index;
            if (order == 2 && a.res != b.res) return a.res < b.res;
            if (order == 4 && a.comp != b.comp) return a.comp < b.comp;
            if (a.Y != b.Y) return a.Y < b.Y;
            if (a.X != b.X) return a.X < b.X;
            if (a.comp != b.comp) return a.comp < b.comp;
            return a.res < b.res;
        });
        Cursor cur{&parts, 0, parts[0].first, parts[0].second};
        const size_t np = precs.size();
        if (order == 0) {
            for (int l = 0; l < Ly; ++l)
                for (size_t i = 0; i < np; ++i)
                    if ((rc = packet(d, f, &bands[(size_t)precs[i].first_band], precs[i].nb, l, cur, got))) return rc;
        } else if (order == 1) {
            for (size_t i0 = 0; i0 < np;) {
                size_t i1 = i0;
                while (i1 < np && precs[i1].res == precs[i0].res) ++i1;
                for (int l = 0; l < Ly; ++l)
                    for (size_t i = i0; i < i1; ++i)
                        if ((rc = packet(d, f, &bands[(size_t)precs[i].first_band], precs[i].nb, l, cur, got))) return rc;
                i0 = i1;
            }
        } else {
            for (size_t i = 0; i < np; ++i)
                for (int l = 0; l < Ly; ++l)
                    if ((rc = packet(d, f, &bands[(size_t)precs[i].first_band], precs[i].nb, l, cur, got))) return rc;
        }
        if ((rc = packets_end(f, cur))) return rc;
    }
    return 0;
}

#undef JP2_BAD
#undef JP2_OUT

}  // namespace jp2p

// The whole walk.  There is no headers-only form: a file counts as read only if every one of its packets parses.  `take`: what is
// read beyond the first subset (JP2_TAKE_IRREVERSIBLE: 9/7 files; JP2_TAKE_TILES: tiles, origins, precincts); without a flag such a
// file is -2, as it always was.
inline int jp2_parse(const uint8_t* file, size_t size, Jp2File* f, unsigned take = 0) {
    size_t s = 0, e = 0;
    bool boxed = false;
    uint32_t box[4] = {0, 0, 0, 0};
    if (!file) { f->reason = "no file"; return -1; }
    int rc = jp2p::find_codestream(file, size, f, &s, &e, &boxed, box);
    if (rc) return rc;
    rc = jp2p::parse_headers(file, s, e, boxed, box, f, take);
    if (rc) return rc;
    if (take & JP2_TAKE_TILES) return jp2p::tier2_tiles(file, f);
    std::vector<jp2p::Band> bands;
    rc = jp2p::geometry(f, bands);
    if (rc) return rc;
    return jp2p::tier2(file, f, bands);
}
