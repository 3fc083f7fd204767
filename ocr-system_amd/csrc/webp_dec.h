// Lossless WebP (VP8L) decoding as plain functions.  webpdec.hip runs them on the device, one wave64 per file; tests/webp_main.cpp compiles
// the same text for the host (one "lane"), where the sanitizers can see it.
//
// Everything the walk decides is uniform over the lanes: every lane reads the same bits and takes the same branches.  The lanes differ
// only where work is spread: building a code's tables, filling code-length runs, copying a backward reference and inserting the copied
// pixels into the colour cache.  The four primitives below, the cache stamp's atomicMax and the reduction of the largest group index are
// all that knows about lanes.
//
// Prefix codes are canonical codes of at most 15 bits, first bit read = most significant code bit.  A code is stored as the count of
// codes per length, the symbols sorted by (length, value), and a first-level table over the next WP_FAST bits (length << 12 | symbol;
// WP_SLOW for a longer code).  A lone symbol is a code of 0 bits: its first-level table holds it at every index.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define WP_HD __host__ __device__ inline
#else
#define WP_HD inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define WP_LANES 64
#define WP_LANE() ((int)threadIdx.x)
#define WP_SYNC() __syncthreads()
#define WP_BALLOT(p) ((unsigned long long)__ballot(p))
#else
#define WP_LANES 1
#define WP_LANE() 0
#define WP_SYNC() ((void)0)
#define WP_BALLOT(p) ((p) ? 1ull : 0ull)
#endif

constexpr int WP_FAST = 8;
constexpr unsigned WP_SLOW = 0xFFFFu;
constexpr int WP_MAX_GROUPS = 4096;            // prefix-code groups an entropy image may name (-2 beyond; libwebp's encoder stays below 2600)
constexpr int WP_MAX_CACHE_BITS = 11;
constexpr int WP_GREEN_MAX = 256 + 24 + (1 << WP_MAX_CACHE_BITS);
constexpr int WP_CL_AT = 2336;                 // the 19 lengths of the code-length code sit past the largest alphabet (2328)
constexpr int WP_LENS = WP_CL_AT + 32;
constexpr int WP_TREE_HEAD = 16 + (1 << WP_FAST);   // u16 per code before its sorted symbols: counts, first-level table
constexpr int WP_CL_WORDS = WP_TREE_HEAD + 19;
// u16 of one group of five codes at this colour-cache size
constexpr int wp_group_words(int cache_size) { return 5 * WP_TREE_HEAD + (280 + cache_size) + 256 * 3 + 40; }
constexpr size_t WP_TABLE_WORDS = (size_t)WP_MAX_GROUPS * wp_group_words(1 << WP_MAX_CACHE_BITS);   // u16 per file: never too small
constexpr int wp_subsize(int n, int bits) { return (n + (1 << bits) - 1) >> bits; }
// u32 of the sub-resolution images a file can carry: predictor, cross-colour and entropy image (block bits >= 2), and the palette
constexpr size_t wp_sub_words(int w, int h) { return 3 * (size_t)wp_subsize(w, 2) * wp_subsize(h, 2) + 256; }

enum : int { WP_PREDICTOR = 0, WP_CROSS = 1, WP_GREEN = 2, WP_PALETTE = 3 };

// What stage 1 leaves for stage 2: the transforms in stream order (they are undone last to first).
struct WpTrans { int type, width, bits, count; uint32_t sub; };   // width: of the image the transform gives; count: palette colours; sub: word offset of its data
struct WpHead { int err, ntrans, width; WpTrans t[4]; };           // err: 0 / -1 / -2; width: of the decoded ARGB stream (packed when a palette bundles)

struct WpBits {
    const uint8_t* d;
    uint32_t len, nbits, pos, next;
    uint64_t buf;
    int have;
};

struct WpCtx {
    WpBits b;
    int err;
    uint8_t* lens;       // [WP_LENS]            (device: LDS)
    uint32_t* cache;     // [1 << 11]            (device: LDS)
    uint32_t* stamp;     // [1 << 11]            (device: LDS) position + 1 of the pixel that owns each cache slot
    uint16_t* cl;        // [WP_CL_WORDS]        (device: LDS) the code-length code
    uint16_t* gfast;     // [5 << WP_FAST] or null: the current group's first-level tables (device: LDS)
    uint16_t* tab;       // [WP_TABLE_WORDS]     the groups' codes
    uint32_t* sub;       // [sub_cap]            sub-resolution images and the palette
    uint32_t sub_cap, sub_used;
};

// the 120 short distance codes: (dy << 4) | (8 - dx)
WP_HD int wp_code_to_plane(int i) {
    constexpr uint8_t t[120] = {
        0x18, 0x07, 0x17, 0x19, 0x28, 0x06, 0x27, 0x29, 0x16, 0x1a, 0x26, 0x2a, 0x38, 0x05, 0x37, 0x39, 0x15, 0x1b, 0x36, 0x3a,
        0x25, 0x2b, 0x48, 0x04, 0x47, 0x49, 0x14, 0x1c, 0x35, 0x3b, 0x46, 0x4a, 0x24, 0x2c, 0x58, 0x45, 0x4b, 0x34, 0x3c, 0x03,
        0x57, 0x59, 0x13, 0x1d, 0x56, 0x5a, 0x23, 0x2d, 0x44, 0x4c, 0x55, 0x5b, 0x33, 0x3d, 0x68, 0x02, 0x67, 0x69, 0x12, 0x1e,
        0x66, 0x6a, 0x22, 0x2e, 0x54, 0x5c, 0x43, 0x4d, 0x65, 0x6b, 0x32, 0x3e, 0x78, 0x01, 0x77, 0x79, 0x53, 0x5d, 0x11, 0x1f,
        0x64, 0x6c, 0x42, 0x4e, 0x76, 0x7a, 0x21, 0x2f, 0x75, 0x7b, 0x31, 0x3f, 0x63, 0x6d, 0x52, 0x5e, 0x00, 0x74, 0x7c, 0x41,
        0x4f, 0x10, 0x20, 0x62, 0x6e, 0x30, 0x73, 0x7d, 0x51, 0x5f, 0x40, 0x72, 0x7e, 0x61, 0x6f, 0x50, 0x71, 0x7f, 0x60, 0x70};
    return t[i];
}
WP_HD int wp_cl_order(int i) {
    constexpr uint8_t t[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
    return t[i];
}

// ---- bit reader: least significant bit first; bits past the end read as 0 and make the stream corrupt once consumed (wp_check) ----
WP_HD uint32_t wp_load32(const WpBits& b) {
    if (b.next + 4 <= b.len) {
#if defined(__HIP_DEVICE_COMPILE__)
        return *reinterpret_cast<const uint32_t*>(b.d + b.next);   // (the device copy of a stream starts on a 16-byte boundary)
#else
        uint32_t v;
        memcpy(&v, b.d + b.next, 4);
        return v;
#endif
    }
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4; ++k)
        if (b.next + k < b.len) v |= (uint32_t)b.d[b.next + k] << (8 * k);
    return v;
}
WP_HD void wp_bits_init(WpBits& b, const uint8_t* d, uint32_t len, uint32_t start_byte) {
    b.d = d; b.len = len; b.nbits = len * 8; b.pos = start_byte * 8; b.next = start_byte & ~3u; b.buf = 0; b.have = 0;
    const uint32_t skip = (start_byte & 3u) * 8;
    b.buf = (uint64_t)(wp_load32(b) >> skip); b.have = 32 - (int)skip; b.next += 4;
}
WP_HD uint32_t wp_peek(WpBits& b) {
    if (b.have < 32) {
        b.buf |= (uint64_t)wp_load32(b) << b.have;
        b.have += 32;
        if (b.next < 0xFFFFFFF0u) b.next += 4;
    }
    return (uint32_t)b.buf;
}
WP_HD void wp_skip(WpBits& b, int n) { b.buf >>= n; b.have -= n; if (b.pos < 0xFFFFFF00u) b.pos += (uint32_t)n; }
WP_HD uint32_t wp_read(WpBits& b, int n) {   // n: 0..24
    const uint32_t v = wp_peek(b) & ((1u << n) - 1u);
    wp_skip(b, n);
    return v;
}
WP_HD bool wp_check(WpCtx& c) {
    if (!c.err && c.b.pos > c.b.nbits) c.err = -1;   // read past the chunk
    return c.err == 0;
}

// ---- prefix codes ----
// t: counts [16], first-level table [1 << WP_FAST], then the sorted symbols
WP_HD int wp_walk(const uint16_t* t, uint32_t v, int maxlen, int* len) {
    const uint16_t* sym = t + WP_TREE_HEAD;
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= maxlen; ++l) {
        code |= (int)(v & 1u); v >>= 1;
        const int count = t[l];
        if (code - first < count) { *len = l; return sym[index + code - first]; }
        index += count; first = (first + count) << 1; code <<= 1;
    }
    return -1;
}

WP_HD int wp_sym(WpCtx& c, const uint16_t* t, const uint16_t* fast) {
    const uint32_t v = wp_peek(c.b);
    const unsigned e = fast[v & ((1u << WP_FAST) - 1u)];
    if (e != WP_SLOW) { wp_skip(c.b, (int)(e >> 12)); return (int)(e & 0xFFFu); }
    int len = 0;
    const int s = wp_walk(t, v, 15, &len);
    if (s < 0) { c.err = -1; return 0; }   // (a complete code has no unused pattern)
    wp_skip(c.b, len);
    return s;
}

// lens[0..n) -> the code at t (all lanes).  Legal: a complete code, or a lone symbol of a length below 15 (libwebp's rule).
WP_HD bool wp_build(WpCtx& c, const uint8_t* lens, int n, uint16_t* t) {
    const int lane = WP_LANE();
    WP_SYNC();   // lens is complete; nobody still reads the table that stood at t
    int cnt[16];
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    for (int j = 0; j < n; j += WP_LANES) {
        const int s = j + lane;
        const int l = s < n ? lens[s] : 0;
        for (int q = 1; q < 16; ++q) cnt[q] += __builtin_popcountll(WP_BALLOT(l == q));
    }
    int total = 0, left = 1;
    bool over = false;
    for (int l = 1; l < 16; ++l) {
        total += cnt[l];
        left = 2 * left - cnt[l];
        if (left < 0) { over = true; left = 0; }
    }
    if (total == 0 || (total == 1 && cnt[15]) || (total > 1 && (over || left != 0))) { c.err = -1; return false; }
    uint16_t* sym = t + WP_TREE_HEAD;
    if (lane == 0)
        for (int l = 0; l < 16; ++l) t[l] = (uint16_t)cnt[l];
    int base[16];
    base[1] = 0;
    for (int l = 1; l < 15; ++l) base[l + 1] = base[l] + cnt[l];
    int run[16];
    for (int l = 0; l < 16; ++l) run[l] = 0;
    for (int j = 0; j < n; j += WP_LANES) {
        const int s = j + lane;
        const int l = s < n ? lens[s] : 0;
        for (int q = 1; q < 16; ++q) {
            if (!cnt[q]) continue;
            const unsigned long long m = WP_BALLOT(l == q);
            if (l == q) sym[base[q] + run[q] + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = (uint16_t)s;
            run[q] += __builtin_popcountll(m);
        }
    }
    WP_SYNC();
    for (int e = lane; e < (1 << WP_FAST); e += WP_LANES) {
        unsigned v = WP_SLOW;
        if (total == 1) v = sym[0];
        else {
            int len = 0;
            const int s = wp_walk(t, (uint32_t)e, WP_FAST, &len);
            if (s >= 0) v = ((unsigned)len << 12) | (unsigned)s;
        }
        t[16 + e] = (uint16_t)v;
    }
    WP_SYNC();
    return true;
}

// one prefix code of `size` symbols from the stream -> t
WP_HD bool wp_read_code(WpCtx& c, int size, uint16_t* t) {
    const int lane = WP_LANE();
    WP_SYNC();   // (the previous code's build has read lens)
    for (int s = lane; s < size; s += WP_LANES) c.lens[s] = 0;
    WP_SYNC();
    if (wp_read(c.b, 1)) {
        const int two = (int)wp_read(c.b, 1);
        const int s0 = (int)wp_read(c.b, wp_read(c.b, 1) ? 8 : 1);
        if (s0 >= size) { c.err = -1; return false; }
        int s1 = -1;
        if (two) {
            s1 = (int)wp_read(c.b, 8);
            if (s1 >= size || s1 == s0) { c.err = -1; return false; }
        }
        if (lane == 0) { c.lens[s0] = 1; if (s1 >= 0) c.lens[s1] = 1; }
    } else {
        const int ncl = (int)wp_read(c.b, 4) + 4;
        int clv[19];
        for (int i = 0; i < 19; ++i) clv[i] = 0;
        for (int i = 0; i < ncl; ++i) clv[i] = (int)wp_read(c.b, 3);
        uint8_t* cll = c.lens + WP_CL_AT;
        if (lane == 0)
            for (int i = 0; i < 19; ++i) cll[wp_cl_order(i)] = (uint8_t)clv[i];
        if (!wp_build(c, cll, 19, c.cl)) return false;
        int maxsym = size;
        if (wp_read(c.b, 1)) {
            const int nb = 2 + 2 * (int)wp_read(c.b, 3);
            maxsym = 2 + (int)wp_read(c.b, nb);
            if (maxsym > size) { c.err = -1; return false; }
        }
        int sym = 0, prev = 8;
        while (sym < size && maxsym > 0) {
            --maxsym;
            const int cl = wp_sym(c, c.cl, c.cl + 16);
            if (!wp_check(c)) return false;
            if (cl < 16) {
                if (lane == 0) c.lens[sym] = (uint8_t)cl;
                ++sym;
                if (cl) prev = cl;
            } else {
                const int rep = (int)wp_read(c.b, cl == 16 ? 2 : cl == 17 ? 3 : 7) + (cl == 18 ? 11 : 3);
                if (sym + rep > size) { c.err = -1; return false; }
                if (cl == 16)
                    for (int k = lane; k < rep; k += WP_LANES) c.lens[sym + k] = (uint8_t)prev;
                sym += rep;
            }
        }
    }
    if (!wp_check(c)) return false;
    return wp_build(c, c.lens, size, t);
}

WP_HD int wp_prefix(WpBits& b, int s) {   // the length / distance prefix rule
    if (s < 4) return s + 1;
    const int extra = (s - 2) >> 1;
    return ((2 + (s & 1)) << extra) + (int)wp_read(b, extra) + 1;
}

WP_HD uint32_t wp_hash(uint32_t argb, int bits) { return (0x1E35A7BDu * argb) >> (32 - bits); }

// the five codes of group g: offsets of the codes inside a group
struct WpGroupLayout { int off[5], words; };
WP_HD WpGroupLayout wp_group_layout(int cache_size) {
    WpGroupLayout L;
    const int sizes[5] = {280 + cache_size, 256, 256, 256, 40};
    int o = 0;
    for (int a = 0; a < 5; ++a) { L.off[a] = o; o += WP_TREE_HEAD + sizes[a]; }
    L.words = o;
    return L;
}

// The codes of `ngroups` groups, then the pixel walk: w x h ARGB words into out.  meta: the entropy image (group index in bits 8..23 of
// each word) or null.
WP_HD void wp_image_body(WpCtx& c, int w, int h, uint32_t* out, int cb, const uint32_t* meta, int mbits, int mw, int ngroups) {
    const int lane = WP_LANE();
    const int csize = cb ? 1 << cb : 0;
    const WpGroupLayout L = wp_group_layout(csize);
    const int sizes[5] = {280 + csize, 256, 256, 256, 40};
    for (int g = 0; g < ngroups; ++g)
        for (int a = 0; a < 5; ++a)
            if (!wp_read_code(c, sizes[a], c.tab + (size_t)g * L.words + L.off[a])) return;
    WP_SYNC();
    for (int k = lane; k < csize; k += WP_LANES) { c.cache[k] = 0; c.stamp[k] = 0; }
    WP_SYNC();
    const uint32_t n = (uint32_t)w * (uint32_t)h;
    uint32_t pos = 0;
    int x = 0, y = 0, cur = -1, block = -1;
    const uint16_t* G = c.tab;
    const uint16_t* F[5];
    for (int a = 0; a < 5; ++a) F[a] = nullptr;
    while (pos < n) {
        int g = 0;
        if (meta) {
            const int bl = (y >> mbits) * mw + (x >> mbits);
            if (bl != block) { block = bl; g = (int)((meta[bl] >> 8) & 0xFFFFu); }
            else g = cur;
        }
        if (g != cur) {   // (g < ngroups: ngroups is the largest index + 1)
            cur = g;
            G = c.tab + (size_t)g * L.words;
            if (c.gfast) {   // the group's first-level tables -> LDS
                WP_SYNC();
                for (int a = 0; a < 5; ++a)
                    for (int e = lane; e < (1 << WP_FAST); e += WP_LANES) c.gfast[(a << WP_FAST) + e] = G[L.off[a] + 16 + e];
                WP_SYNC();
                for (int a = 0; a < 5; ++a) F[a] = c.gfast + (a << WP_FAST);
            } else {
                for (int a = 0; a < 5; ++a) F[a] = G + L.off[a] + 16;
            }
        }
        const int s = wp_sym(c, G + L.off[0], F[0]);
        if (s < 256) {
            const uint32_t r = (uint32_t)wp_sym(c, G + L.off[1], F[1]);
            const uint32_t bl = (uint32_t)wp_sym(c, G + L.off[2], F[2]);
            const uint32_t al = (uint32_t)wp_sym(c, G + L.off[3], F[3]);
            const uint32_t p = (al << 24) | (r << 16) | ((uint32_t)s << 8) | bl;
            if (lane == 0) {
                out[pos] = p;
                if (cb) { const uint32_t k = wp_hash(p, cb); c.cache[k] = p; c.stamp[k] = pos + 1; }
            }
            ++pos;
            if (++x == w) { x = 0; ++y; }
        } else if (s < 280) {
            const uint32_t length = (uint32_t)wp_prefix(c.b, s - 256);
            const int ds = wp_sym(c, G + L.off[4], F[4]);
            const int dcode = wp_prefix(c.b, ds);
            uint32_t dist;
            if (dcode > 120) dist = (uint32_t)(dcode - 120);
            else {
                const int pc = wp_code_to_plane(dcode - 1);
                const long long d = (long long)(pc >> 4) * w + 8 - (pc & 15);
                dist = d < 1 ? 1u : (uint32_t)d;
            }
            if (c.err || dist > pos || length > n - pos) { c.err = -1; return; }   // a copy before the first or past the last pixel
            WP_SYNC();   // the pixels written so far are there for every lane
            const uint32_t* src = out + (pos - dist);
            for (uint32_t k0 = 0; k0 < length; k0 += WP_LANES) {
                const uint32_t k = k0 + (uint32_t)lane;
                const bool act = k < length;
                uint32_t p = 0, hk = 0;
                if (act) {
                    p = src[dist >= length ? k : k % dist];   // (always one of the dist pixels before pos: never one this copy writes)
                    out[pos + k] = p;
                }
                if (cb) {   // the copied pixels enter the cache; on equal hash the later pixel wins
                    if (act) {
                        hk = wp_hash(p, cb);
#if defined(__HIP_DEVICE_COMPILE__)
                        atomicMax(&c.stamp[hk], pos + k + 1);
#else
                        c.stamp[hk] = pos + k + 1;
#endif
                    }
                    WP_SYNC();
                    if (act && c.stamp[hk] == pos + k + 1) c.cache[hk] = p;
                    WP_SYNC();
                }
            }
            pos += length;
            const uint32_t nx = (uint32_t)x + length;
            y += (int)(nx / (uint32_t)w); x = (int)(nx % (uint32_t)w);
        } else {
            WP_SYNC();   // (lane 0's cache writes)
            const uint32_t p = c.cache[s - 280];   // s - 280 < csize: the alphabet ends there (no cache: it ends at 280)
            WP_SYNC();
            if (lane == 0) {
                out[pos] = p;
                const uint32_t k = wp_hash(p, cb);
                c.cache[k] = p; c.stamp[k] = pos + 1;
            }
            ++pos;
            if (++x == w) { x = 0; ++y; }
        }
        if (!wp_check(c)) return;
    }
    WP_SYNC();
}

WP_HD int wp_read_cache_bits(WpCtx& c) {
    if (!wp_read(c.b, 1)) return 0;
    const int cb = (int)wp_read(c.b, 4);
    if (cb < 1 || cb > WP_MAX_CACHE_BITS) { c.err = -1; return 0; }
    return cb;
}

// a sub-resolution image (or the palette): its own colour cache, one group, no transforms -> c.sub + its offset; ~0u on error
WP_HD uint32_t wp_subimage(WpCtx& c, int w, int h) {
    const uint32_t words = (uint32_t)w * (uint32_t)h;
    if (c.sub_used + words > c.sub_cap) { c.err = -1; return ~0u; }
    const uint32_t off = c.sub_used;
    c.sub_used += words;
    const int cb = wp_read_cache_bits(c);
    if (!wp_check(c)) return ~0u;
    wp_image_body(c, w, h, c.sub + off, cb, nullptr, 0, 0, 1);
    return c.err ? ~0u : off;
}

WP_HD uint32_t wp_add(uint32_t a, uint32_t b) {
    return (((a & 0xFF00FF00u) + (b & 0xFF00FF00u)) & 0xFF00FF00u) | (((a & 0x00FF00FFu) + (b & 0x00FF00FFu)) & 0x00FF00FFu);
}

// Stage 1 of a file: transform headers and their sub-resolution images, then the ARGB stream -> plane (head->width x h words).
// c.b stands behind the five header bytes.
WP_HD void wp_decode_stream(WpCtx& c, int w, int h, uint32_t* plane, WpHead* head) {
    const int lane = WP_LANE();
    WpHead H;
    H.err = 0; H.ntrans = 0; H.width = w;
    for (int k = 0; k < 4; ++k) { H.t[k].type = H.t[k].width = H.t[k].bits = H.t[k].count = 0; H.t[k].sub = 0; }
    int seen = 0, xs = w;
    c.sub_used = 0;
    while (!c.err && wp_read(c.b, 1)) {
        const int t = (int)wp_read(c.b, 2);
        if (seen & (1 << t)) { c.err = -1; break; }   // a transform repeated
        seen |= 1 << t;
        WpTrans& T = H.t[H.ntrans++];
        T.type = t; T.width = xs;
        if (t == WP_PREDICTOR || t == WP_CROSS) {
            T.bits = (int)wp_read(c.b, 3) + 2;
            T.sub = wp_subimage(c, wp_subsize(xs, T.bits), wp_subsize(h, T.bits));
        } else if (t == WP_PALETTE) {
            T.count = (int)wp_read(c.b, 8) + 1;
            T.bits = T.count > 16 ? 0 : T.count > 4 ? 1 : T.count > 2 ? 2 : 3;
            T.sub = wp_subimage(c, T.count, 1);
            if (!c.err) {   // the palette is delta-coded
                WP_SYNC();
                if (lane == 0)
                    for (int i = 1; i < T.count; ++i) c.sub[T.sub + i] = wp_add(c.sub[T.sub + i], c.sub[T.sub + i - 1]);
                WP_SYNC();
            }
            xs = wp_subsize(xs, T.bits);
        }
        wp_check(c);
    }
    if (!c.err) {
        H.width = xs;
        const int cb = wp_read_cache_bits(c);
        const uint32_t* meta = nullptr;
        int mbits = 0, mw = 0, ngroups = 1;
        if (!c.err && wp_read(c.b, 1)) {
            mbits = (int)wp_read(c.b, 3) + 2;
            mw = wp_subsize(xs, mbits);
            const int mh = wp_subsize(h, mbits);
            const uint32_t off = wp_subimage(c, mw, mh);
            if (!c.err) {
                meta = c.sub + off;
                WP_SYNC();
                int m = 0;
                for (int k = lane; k < mw * mh; k += WP_LANES) { const int g = (int)((meta[k] >> 8) & 0xFFFFu); m = g > m ? g : m; }
#if defined(__HIP_DEVICE_COMPILE__)
                for (int o = 32; o; o >>= 1) { const int q = __shfl_xor(m, o, 64); m = q > m ? q : m; }
#endif
                ngroups = m + 1;
                if (ngroups > WP_MAX_GROUPS) c.err = -2;
            }
        }
        if (wp_check(c)) wp_image_body(c, xs, h, plane, cb, meta, mbits, mw, ngroups);
    }
    H.err = c.err;
    if (lane == 0) *head = H;
}

// ---- stage 2: the inverse transforms, a pixel at a time ----
WP_HD uint32_t wp_avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xFEFEFEFEu) >> 1) + (a & b); }
WP_HD int wp_clip(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
WP_HD int wp_iabs(int v) { return v < 0 ? -v : v; }

// the prediction of modes 0..15 from the left, top, top-left and top-right neighbours
WP_HD uint32_t wp_predict(int mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
    switch (mode) {
        case 1: return L;
        case 2: return T;
        case 3: return TR;
        case 4: return TL;
        case 5: return wp_avg2(wp_avg2(L, TR), T);
        case 6: return wp_avg2(L, TL);
        case 7: return wp_avg2(L, T);
        case 8: return wp_avg2(TL, T);
        case 9: return wp_avg2(T, TR);
        case 10: return wp_avg2(wp_avg2(L, TL), wp_avg2(T, TR));
        case 11: {
            int d = 0;
            for (int sh = 0; sh < 32; sh += 8) {
                const int t = (int)((T >> sh) & 255u), l = (int)((L >> sh) & 255u), q = (int)((TL >> sh) & 255u);
                d += wp_iabs(l - q) - wp_iabs(t - q);
            }
            return d <= 0 ? T : L;
        }
        case 12: {
            uint32_t r = 0;
            for (int sh = 0; sh < 32; sh += 8)
                r |= (uint32_t)wp_clip((int)((L >> sh) & 255u) + (int)((T >> sh) & 255u) - (int)((TL >> sh) & 255u)) << sh;
            return r;
        }
        case 13: {
            const uint32_t A = wp_avg2(L, T);
            uint32_t r = 0;
            for (int sh = 0; sh < 32; sh += 8) {
                const int a = (int)((A >> sh) & 255u), b = (int)((TL >> sh) & 255u);
                r |= (uint32_t)wp_clip(a + (a - b) / 2) << sh;   // (the division truncates towards zero)
            }
            return r;
        }
        default: return 0xFF000000u;   // 0, 14, 15
    }
}

WP_HD int wp_s8(uint32_t v) { return (int)(int8_t)(uint8_t)v; }

// m: the block's element (red_to_blue << 16 | green_to_blue << 8 | green_to_red)
WP_HD uint32_t wp_cross_px(uint32_t m, uint32_t p) {
    const int g = wp_s8(p >> 8);
    const uint32_t r = ((p >> 16) + (uint32_t)((wp_s8(m) * g) >> 5)) & 255u;
    const uint32_t b = (p + (uint32_t)((wp_s8(m >> 8) * g) >> 5) + (uint32_t)((wp_s8(m >> 16) * wp_s8(r)) >> 5)) & 255u;
    return (p & 0xFF00FF00u) | (r << 16) | b;
}

WP_HD uint32_t wp_green_px(uint32_t p) {
    const uint32_t g = (p >> 8) & 255u;
    return (p & 0xFF00FF00u) | ((((p >> 16) + g) & 255u) << 16) | ((p + g) & 255u);
}

// pixel x of a row of packed indices (src: the row's subsize(w, bits) words)
WP_HD uint32_t wp_palette_px(const uint32_t* src, int x, int bits, const uint32_t* pal, int count) {
    const int bpp = 8 >> bits;
    const uint32_t idx = (((src[x >> bits] >> 8) & 255u) >> ((x & ((1 << bits) - 1)) * bpp)) & ((1u << bpp) - 1u);
    return idx < (uint32_t)count ? pal[idx] : 0u;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The whole of stage 2 as plain loops (host): a, b: two planes of w * h words, the decoded stream in a.  Returns the plane that holds
// the w x h ARGB image.
inline uint32_t* wp_untransform_host(const WpHead& H, const uint32_t* sub, int w, int h, uint32_t* a, uint32_t* b) {
    for (int k = H.ntrans - 1; k >= 0; --k) {
        const WpTrans& T = H.t[k];
        const int tw = T.width;
        if (T.type == WP_PREDICTOR) {
            const int sw = wp_subsize(tw, T.bits);
            const uint32_t* m = sub + T.sub;
            a[0] = wp_add(a[0], 0xFF000000u);
            for (int x = 1; x < tw; ++x) a[x] = wp_add(a[x], a[x - 1]);
            for (int y = 1; y < h; ++y) {
                uint32_t* r = a + (size_t)y * tw;
                r[0] = wp_add(r[0], r[-tw]);
                for (int x = 1; x < tw; ++x) {
                    const int mode = (int)((m[(size_t)(y >> T.bits) * sw + (x >> T.bits)] >> 8) & 15u);
                    r[x] = wp_add(r[x], wp_predict(mode, r[x - 1], r[x - tw], r[x - tw - 1], r[x - tw + 1]));
                }
            }
        } else if (T.type == WP_CROSS) {
            const int sw = wp_subsize(tw, T.bits);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < tw; ++x)
                    a[(size_t)y * tw + x] = wp_cross_px(sub[T.sub + (size_t)(y >> T.bits) * sw + (x >> T.bits)], a[(size_t)y * tw + x]);
        } else if (T.type == WP_GREEN) {
            for (size_t i = 0; i < (size_t)tw * h; ++i) a[i] = wp_green_px(a[i]);
        } else {
            const int pw = wp_subsize(tw, T.bits);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < tw; ++x) b[(size_t)y * tw + x] = wp_palette_px(a + (size_t)y * pw, x, T.bits, sub + T.sub, T.count);
            uint32_t* t = a; a = b; b = t;
        }
    }
    return a;
}
#endif
