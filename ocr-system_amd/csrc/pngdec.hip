// Baseline PNG decoder on the device (pngdec.h): what the reference's Image.open(...).convert('RGB') does for .png inputs, byte-identical
// to Pillow.
//
// The chunk walk (a few dozen bytes of headers) is host code; it gathers each file's IDAT payloads into one pinned staging buffer.
// The device then runs, per sub-batch:
//   1. pd_inflate: one wave64 work-group per file inflates its zlib stream.  All decode state is wave-uniform; the input bits sit in a
//      256-byte window held one word per lane (read with readlane), the 32 KB DEFLATE window is a ring in LDS (back-references never
//      read global memory the wave has just written), and the ring is flushed to the filtered-scanline buffer in 16 KB pieces with
//      16-byte stores.  Huffman tables are built per block in LDS (a 10-bit fast table, canonical decode past it); back-reference
//      copies and stored blocks are spread over the 64 lanes (lane k copies src + k mod dist).  Any RFC 1950/1951 violation sets the
//      file's error word;
//   2. pd_adler_part / pd_adler_fin: the Adler-32 of the inflated stream as a parallel reduction (64 KB blocks), compared with the
//      stream's own; every filter byte must be 0..4;
//   3. pd_unfilter: the filters are undone in bands of 64 rows as a skewed wavefront: lane i owns row band*64 + i and runs one byte
//      behind lane i-1, so the up / up-left bytes Up, Avg and Paeth need come from lane i-1 by a cross-lane move and the left byte from
//      the lane's own last steps; row 63 of a band is handed to the next band through LDS.  Palette indices are checked here;
//   4. pd_expand: unfiltered rows -> RGB u8 as Pillow's convert('RGB') maps them; pd_status: error words + host results -> status.
//
// The image streams of PDF's /FlateDecode (flate_image_run: the pages of scanned PDFs) are plain zlib streams of the same rows and take
// the same stages; only the row stage differs with /Predictor: PNG row filters (10..15) are stage 3; TIFF horizontal differencing (2)
// is pd_tiff_predict, a prefix sum mod 256 per row and component across lanes; packed rows (1) have no filter byte and no row stage.
// pd_expand applies /Decode [1 0] and looks /Indexed samples up in the palette the host built.
#include "pngdec.h"

#include <algorithm>
#include <cstring>
#include <vector>

#include "engine.h"

namespace {

constexpr int PD_RING = 32768;          // LDS ring: the largest DEFLATE window
constexpr int PD_FLUSH = 16384;         // ring -> global in pieces of this size (unflushed bytes always lie inside the window)
constexpr int PD_FAST = 10;             // fast Huffman table bits
constexpr int PD_ADLER_BLK = 65536;     // bytes per Adler-32 partial (256 threads x 256 bytes)
constexpr int PD_MAX_ROW = 65536;       // row bytes the unfilter's LDS hand-over row holds
constexpr size_t PD_Z_PAD = 512;        // zero tail per file: the bit reader's word window may look past the stream

enum : int { PD_E_STREAM = 1, PD_E_PALETTE = 2, PD_E_ADLER = 4, PD_E_FILTER = 8 };

__constant__ unsigned short pd_len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ unsigned char pd_len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ unsigned short pd_dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ unsigned char pd_dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ unsigned char pd_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// one canonical Huffman code in LDS: counts per length, symbols sorted by (length, value), and the fast table
// fast[bits] = len << 9 | symbol for codes of <= PD_FAST bits (0: longer code or an unused pattern -> the canonical walk)
struct PdHuff { int cnt[16]; unsigned short sym[288]; unsigned short fast[1 << PD_FAST]; };

struct PdLds {
    uint8_t ring[PD_RING];
    PdHuff lit, dist, cl;
    uint8_t lens[320];
};

// wave-uniform bit reader over the file's stream: lanes hold 64 consecutive words from word `wbase`
struct PdBits {
    const uint32_t* z32;
    unsigned zlen, pos, wbase;
    uint32_t w;
    bool bad;
    __device__ void load(int lane) {
        wbase = pos >> 5;
        if ((size_t)wbase * 4 > (size_t)zlen + 8) { bad = true; wbase = 0; }   // ran past the stream (the tail padding covers one window)
        w = z32[wbase + lane];
    }
    // at least 33 valid bits from `pos`
    __device__ uint64_t peek(int lane) {
        if ((pos >> 5) - wbase >= 32) load(lane);
        const int idx = (int)((pos >> 5) - wbase);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)w, idx), hi = (uint32_t)__builtin_amdgcn_readlane((int)w, idx + 1);
        return ((((uint64_t)hi) << 32) | lo) >> (pos & 31);
    }
    __device__ unsigned bits(int n, int lane) { const unsigned v = (unsigned)peek(lane) & ((1u << n) - 1); pos += n; return v; }
};

// canonical decode past the fast table (puff's walk); -1 = an unused code
__device__ int pd_slow(const PdHuff& h, uint64_t v, int* len) {
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; ++l) {
        code |= (int)(v & 1); v >>= 1;
        const int count = h.cnt[l];
        if (code - first < count) { *len = l; return h.sym[index + code - first]; }
        index += count; first += count; first <<= 1; code <<= 1;
    }
    return -1;
}

__device__ __forceinline__ int pd_decode(const PdHuff& h, PdBits& b, int lane) {
    const uint64_t v = b.peek(lane);
    const unsigned e = h.fast[v & ((1u << PD_FAST) - 1)];
    if (e) { b.pos += e >> 9; return (int)(e & 511); }
    int len = 0;
    const int s = pd_slow(h, v, &len);
    if (s < 0) { b.bad = true; return 0; }
    b.pos += len;
    return s;
}

// builds h from lens[0..n) (wave-cooperative).  zlib's inflate_table rule: never over-subscribed; incomplete only for a single code of
// length 1 (and not at all for the code-length code); no codes at all is allowed for distances only (any use of one is then an error).
__device__ bool pd_build(PdHuff& h, const uint8_t* lens, int n, int kind /*0 code lengths, 1 literal/length, 2 distance*/, int lane) {
    if (lane < 16) h.cnt[lane] = 0;
    __syncthreads();
    int offs_run[16];
    // counts: per length, a ballot over 64 symbols at a time
    for (int l = 1; l <= 15; ++l) {
        int c = 0;
        for (int j = 0; j < n; j += 64) {
            const int s = j + lane;
            c += __popcll(__ballot(s < n && lens[s] == l));
        }
        offs_run[l] = c;
    }
    int left = 1, maxl = 0;
    for (int l = 1; l <= 15; ++l) {
        left = (left << 1) - offs_run[l];
        if (left < 0) return false;   // over-subscribed
        if (offs_run[l]) maxl = l;
    }
    if (maxl == 0 && kind != 2) return false;
    if (left > 0 && maxl != 0 && (kind == 0 || maxl != 1)) return false;   // incomplete
    if (lane == 0)
        for (int l = 1; l <= 15; ++l) h.cnt[l] = offs_run[l];
    // symbols sorted by length, then value: the rank of a symbol among the earlier ones of its length by ballot prefix counts
    int base = 0;
    for (int l = 1; l <= 15; ++l) {
        int run = 0;
        for (int j = 0; j < n; j += 64) {
            const int s = j + lane;
            const bool f = s < n && lens[s] == l;
            const unsigned long long m = __ballot(f);
            if (f) h.sym[base + run + __popcll(m & ((1ull << lane) - 1))] = (unsigned short)s;
            run += __popcll(m);
        }
        base += run;
    }
    __syncthreads();
    if (kind == 0) return true;   // the code-length code is decoded by the canonical walk only
    for (int e = lane; e < (1 << PD_FAST); e += 64) {
        int code = 0, first = 0, index = 0;
        unsigned short v = 0;
        for (int l = 1; l <= PD_FAST; ++l) {
            code |= (e >> (l - 1)) & 1;
            const int count = h.cnt[l];
            if (code - first < count) { v = (unsigned short)((l << 9) | h.sym[index + code - first]); break; }
            index += count; first += count; first <<= 1; code <<= 1;
        }
        h.fast[e] = v;
    }
    __syncthreads();
    return true;
}

__device__ void pd_flush(const PdLds& L, uint8_t* dst, unsigned from, unsigned to, int lane) {
    __syncthreads();
    for (unsigned j = from + lane * 16; j < to; j += 64 * 16)
        *reinterpret_cast<uint4*>(dst + j) = *reinterpret_cast<const uint4*>(L.ring + (j & (PD_RING - 1)));
}

__global__ __launch_bounds__(64) void pd_inflate(const PdFile* __restrict__ F, const uint8_t* __restrict__ z, uint8_t* __restrict__ filt,
                                                 int* __restrict__ err, unsigned* __restrict__ adler_want) {
    __shared__ PdLds L;
    const PdFile& f = F[blockIdx.x];
    if (!f.valid) return;
    const int lane = threadIdx.x;
    const uint8_t* zf = z + f.zoff;
    uint8_t* dst = filt + f.foff;
    PdBits b;
    b.z32 = reinterpret_cast<const uint32_t*>(zf); b.zlen = f.zlen; b.pos = 16; b.bad = false;   // the 2-byte zlib header was checked by the host
    b.load(lane);
    const unsigned total = f.total, wsize = (unsigned)f.wsize;
    unsigned out = 0, flushed = 0;
    int fixed_built = 0;   // 1: lit / dist hold the fixed code
    bool last = false;
    while (!last && !b.bad) {
        const unsigned hdr = b.bits(3, lane);
        last = hdr & 1;
        const unsigned type = hdr >> 1;
        if (type == 0) {   // stored
            b.pos = (b.pos + 7) & ~7u;
            const unsigned v = b.bits(16, lane), nv = b.bits(16, lane);
            if ((v ^ 0xFFFFu) != nv) { b.bad = true; break; }
            const unsigned bp = b.pos >> 3;
            if ((size_t)bp + v > b.zlen || out + v > total) { b.bad = true; break; }
            for (unsigned c = 0; c < v; c += 64) {
                if (c + lane < v) L.ring[(out + c + lane) & (PD_RING - 1)] = zf[bp + c + lane];
                const unsigned o2 = out + min(c + 64, v);
                if (o2 - flushed >= (unsigned)PD_FLUSH) { pd_flush(L, dst, flushed, flushed + PD_FLUSH, lane); flushed += PD_FLUSH; }
            }
            out += v;
            b.pos += v * 8;
            continue;
        }
        if (type == 3) { b.bad = true; break; }
        if (type == 1) {
            if (fixed_built != 1) {
                for (int s = lane; s < 320; s += 64) L.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
                __syncthreads();
                pd_build(L.lit, L.lens, 288, 1, lane);
                pd_build(L.dist, L.lens + 288, 32, 2, lane);
                fixed_built = 1;
            }
        } else {
            fixed_built = 0;
            const unsigned nlen = b.bits(5, lane) + 257, ndist = b.bits(5, lane) + 1, ncl = b.bits(4, lane) + 4;
            if (nlen > 286 || ndist > 30) { b.bad = true; break; }
            if (lane < 19) L.lens[lane] = 0;
            __syncthreads();
            for (unsigned i = 0; i < ncl; ++i) {
                const unsigned v = b.bits(3, lane);
                if (lane == 0) L.lens[pd_cl_order[i]] = (uint8_t)v;
            }
            __syncthreads();
            if (!pd_build(L.cl, L.lens, 19, 0, lane)) { b.bad = true; break; }
            __syncthreads();
            unsigned i = 0;
            const unsigned ntot = nlen + ndist;
            while (i < ntot && !b.bad) {
                int len = 0;
                const int s = pd_slow(L.cl, b.peek(lane), &len);
                if (s < 0) { b.bad = true; break; }
                b.pos += len;
                if (s < 16) { if (lane == 0) L.lens[i] = (uint8_t)s; ++i; continue; }
                unsigned rep, val = 0;
                if (s == 16) {
                    if (i == 0) { b.bad = true; break; }
                    __syncthreads();
                    val = L.lens[i - 1];
                    rep = 3 + b.bits(2, lane);
                } else if (s == 17) rep = 3 + b.bits(3, lane);
                else rep = 11 + b.bits(7, lane);
                if (i + rep > ntot) { b.bad = true; break; }
                if (lane < (int)rep) L.lens[i + lane] = (uint8_t)val;   // rep <= 138: at most three lane sweeps
                if (lane + 64 < (int)rep) L.lens[i + lane + 64] = (uint8_t)val;
                if (lane + 128 < (int)rep) L.lens[i + lane + 128] = (uint8_t)val;
                i += rep;
            }
            if (b.bad) break;
            __syncthreads();
            if (L.lens[256] == 0) { b.bad = true; break; }   // no end-of-block code
            if (!pd_build(L.lit, L.lens, (int)nlen, 1, lane) || !pd_build(L.dist, L.lens + nlen, (int)ndist, 2, lane)) { b.bad = true; break; }
        }
        // ---- compressed data ----
        for (;;) {
            const int sym = pd_decode(L.lit, b, lane);
            if (b.bad) break;
            if (sym < 256) {
                if (out >= total) { b.bad = true; break; }
                if (lane == 0) L.ring[out & (PD_RING - 1)] = (uint8_t)sym;
                ++out;
            } else if (sym == 256) {
                break;
            } else {
                if (sym > 285) { b.bad = true; break; }
                const int li = sym - 257;
                const unsigned len = pd_len_base[li] + b.bits(pd_len_extra[li], lane);
                const int ds = pd_decode(L.dist, b, lane);
                if (b.bad || ds > 29) { b.bad = true; break; }
                const unsigned dist = pd_dist_base[ds] + b.bits(pd_dist_extra[ds], lane);
                if (dist > out || dist > wsize || out + len > total) { b.bad = true; break; }
                __syncthreads();
                for (unsigned c = 0; c < len; c += 64) {
                    const unsigned k = c + lane;
                    uint8_t v = 0;
                    if (k < len) v = L.ring[(out - dist + (dist >= len ? k : k % dist)) & (PD_RING - 1)];
                    if (k < len) L.ring[(out + k) & (PD_RING - 1)] = v;
                }
                out += len;
            }
            if (out - flushed >= (unsigned)PD_FLUSH) { pd_flush(L, dst, flushed, flushed + PD_FLUSH, lane); flushed += PD_FLUSH; }
        }
    }
    unsigned want = 0;
    if (!b.bad) {
        const unsigned bp = (b.pos + 7) >> 3;
        if (out != total || (size_t)bp + 4 != b.zlen) b.bad = true;   // short / long output, a truncated Adler-32 or bytes after it
        else want = ((unsigned)zf[bp] << 24) | ((unsigned)zf[bp + 1] << 16) | ((unsigned)zf[bp + 2] << 8) | zf[bp + 3];
    }
    if (!b.bad && out > flushed) pd_flush(L, dst, flushed, (out + 15) & ~15u, lane);   // (the region has 16 bytes of slack)
    if (lane == 0) {
        if (b.bad) err[blockIdx.x] |= PD_E_STREAM;
        adler_want[blockIdx.x] = want;
    }
}

// Adler-32 partial over one 64 KB block: A-sum and the block's B contribution as if it started from A = 0
__global__ __launch_bounds__(256) void pd_adler_part(const PdFile* __restrict__ F, const uint8_t* __restrict__ filt, const int* __restrict__ err,
                                                     uint2* __restrict__ part) {
    const PdFile& f = F[blockIdx.y];
    const unsigned start = blockIdx.x * (unsigned)PD_ADLER_BLK;
    if (!f.valid || err[blockIdx.y] || start >= f.total) return;
    const int t = threadIdx.x;
    const unsigned blen = min((unsigned)PD_ADLER_BLK, f.total - start);
    const unsigned p0 = start + t * 256u;
    unsigned s = 0, w = 0;
    unsigned plen = 0;
    if (p0 < f.total) {
        plen = min(256u, f.total - p0);
        const uint8_t* src = filt + f.foff + p0;
        for (unsigned q = 0; q < 256; q += 16) {
            const uint4 v = *reinterpret_cast<const uint4*>(src + q);
            const unsigned wd[4] = {v.x, v.y, v.z, v.w};
            for (int k = 0; k < 16; ++k) {
                const unsigned j = q + k;
                const unsigned d = j < plen ? (wd[k >> 2] >> (8 * (k & 3))) & 255u : 0u;
                s += d; w += (plen - j) * d;
            }
        }
    }
    const unsigned after = (p0 + plen <= start + blen && plen) ? start + blen - (p0 + plen) : 0;
    __shared__ unsigned long long rs[256], rb[256];
    rs[t] = s; rb[t] = (unsigned long long)w + (unsigned long long)s * after;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k) { rs[t] += rs[t + k]; rb[t] += rb[t + k]; }
        __syncthreads();
    }
    if (t == 0) part[f.ablk_off + blockIdx.x] = make_uint2((unsigned)(rs[0] % 65521u), (unsigned)(rb[0] % 65521u));
}

// per file: the Adler-32 from the partials vs the stream's own, and every row's filter byte in 0..4
__global__ __launch_bounds__(256) void pd_adler_fin(const PdFile* __restrict__ F, const uint8_t* __restrict__ filt, const uint2* __restrict__ part,
                                                    const unsigned* __restrict__ adler_want, int* __restrict__ err) {
    const PdFile& f = F[blockIdx.x];
    if (!f.valid || err[blockIdx.x]) return;
    const int t = threadIdx.x;
    const unsigned nblk = (f.total + PD_ADLER_BLK - 1) / PD_ADLER_BLK;
    unsigned long long a = 0, bsum = 0;
    for (unsigned c = t; c < nblk; c += 256) {
        const uint2 p = part[f.ablk_off + c];
        const unsigned end = min(f.total, (c + 1) * (unsigned)PD_ADLER_BLK);
        a += p.x;
        bsum += p.y + (unsigned long long)p.x * ((f.total - end) % 65521u);
    }
    bool badf = false;
    if (f.fb)
        for (int r = t; r < f.height; r += 256) badf |= filt[f.foff + (size_t)r * (f.rb + 1)] > 4;
    __shared__ unsigned long long ra[256], rbs[256];
    __shared__ int rf[256];
    ra[t] = a % 65521u; rbs[t] = bsum % 65521u; rf[t] = badf;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k) { ra[t] += ra[t + k]; rbs[t] += rbs[t + k]; rf[t] |= rf[t + k]; }
        __syncthreads();
    }
    if (t == 0) {
        const unsigned A = (unsigned)((1 + ra[0]) % 65521u);
        const unsigned B = (unsigned)((f.total % 65521u + rbs[0]) % 65521u);
        int e = 0;
        if (((B << 16) | A) != adler_want[blockIdx.x]) e |= PD_E_ADLER;
        if (rf[0]) e |= PD_E_FILTER;
        if (e) err[blockIdx.x] |= e;
    }
}

__device__ __forceinline__ int pd_paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

constexpr int PD_U = 8;   // steps per unrolled group: the group's loads are issued before its dependent steps

template <int BPP>
__device__ void pd_unfilter_file(const PdFile& f, uint8_t* __restrict__ fb, uint8_t* prevrow, int lane, bool* pal_bad) {
    const int rb = (int)f.rb, H = f.height;
    const bool pal_check = f.ct == 3 && f.npal < (1 << f.depth);
    const int d = f.depth, ppb = 8 / (d < 8 ? d : 8);
    for (int band = 0; band * 64 < H; ++band) {
        const int r = band * 64 + lane;
        const bool rowok = r < H;
        uint8_t* row = fb + (size_t)(rowok ? r : 0) * (rb + 1);
        const int ft = rowok ? row[0] : 0;
        uint8_t* px = row + 1;
        int last = 0;
        int hc[BPP], hu[BPP];   // own outputs / received up bytes of the last BPP steps ([0]: the most recent)
        for (int k = 0; k < BPP; ++k) hc[k] = hu[k] = 0;
        const int steps = rb + 63;
        for (int t0 = 0; t0 < steps; t0 += PD_U) {
            int raw[PD_U];
#pragma unroll
            for (int u = 0; u < PD_U; ++u) {
                const int x = t0 + u - lane;
                raw[u] = (rowok && x >= 0 && x < rb) ? px[x] : 0;
            }
#pragma unroll
            for (int u = 0; u < PD_U; ++u) {
                const int x = t0 + u - lane;
                const bool act = rowok && x >= 0 && x < rb;
                int up = __shfl_up(last, 1, 64);
                if (lane == 0) up = (band > 0 && x >= 0 && x < rb) ? prevrow[x] : 0;
                const int left = x >= BPP ? hc[BPP - 1] : 0, ul = x >= BPP ? hu[BPP - 1] : 0;
                int o = raw[u];
                switch (ft) {
                    case 1: o += left; break;
                    case 2: o += up; break;
                    case 3: o += (left + up) >> 1; break;
                    case 4: o += pd_paeth(left, up, ul); break;
                    default: break;
                }
                o &= 255;
                if (act) {
                    px[x] = (uint8_t)o;
                    if (lane == 63) prevrow[x] = (uint8_t)o;
#pragma unroll
                    for (int k = BPP - 1; k > 0; --k) { hc[k] = hc[k - 1]; hu[k] = hu[k - 1]; }
                    hc[0] = o; hu[0] = up;
                    last = o;
                    if (pal_check) {
                        const int nf = (x == rb - 1) ? f.width - x * ppb : ppb;
                        for (int q = 0; q < nf; ++q) {
                            const int idx = d == 8 ? o : (o >> (8 - d * (q + 1))) & ((1 << d) - 1);
                            *pal_bad |= idx >= f.npal;
                        }
                    }
                }
            }
        }
        __syncthreads();   // prevrow (row 63 of this band) -> lane 0 of the next band
    }
}

__global__ __launch_bounds__(64) void pd_unfilter(const PdFile* __restrict__ F, uint8_t* __restrict__ filt, int* __restrict__ err) {
    __shared__ uint8_t prevrow[PD_MAX_ROW];
    const PdFile& f = F[blockIdx.x];
    if (!f.valid || err[blockIdx.x] || !f.fb) return;
    const int lane = threadIdx.x;
    bool pal_bad = false;
    uint8_t* fb = filt + f.foff;
    switch (f.bpp) {
        case 1: pd_unfilter_file<1>(f, fb, prevrow, lane, &pal_bad); break;
        case 2: pd_unfilter_file<2>(f, fb, prevrow, lane, &pal_bad); break;
        case 3: pd_unfilter_file<3>(f, fb, prevrow, lane, &pal_bad); break;
        default: pd_unfilter_file<4>(f, fb, prevrow, lane, &pal_bad); break;
    }
    if (__ballot(pal_bad) && lane == 0) err[blockIdx.x] |= PD_E_PALETTE;
}

// /Predictor 2 of a PDF Flate image (TIFF horizontal differencing, 8-bit components): every byte is the difference to the same component
// of the pixel on its left, so a row is an inclusive prefix sum mod 256 per component.  One wave per row: lanes over 64 consecutive
// pixels, a six-step shuffle scan, the chunk's last sums carried into the next chunk.
__global__ __launch_bounds__(64) void pd_tiff_predict(const PdFile* __restrict__ F, uint8_t* __restrict__ filt, const int* __restrict__ err) {
    const PdFile& f = F[blockIdx.y];
    if (!f.valid || err[blockIdx.y] || !f.tiff) return;
    const int lane = threadIdx.x, C = f.bpp;
    for (int r = blockIdx.x; r < f.height; r += gridDim.x) {
        uint8_t* row = filt + f.foff + (size_t)r * f.rb;
        int carry0 = 0, carry1 = 0, carry2 = 0;
        for (int x0 = 0; x0 < f.width; x0 += 64) {
            const int x = x0 + lane;
            const bool act = x < f.width;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c >= C) break;
                int v = act ? row[(size_t)x * C + c] : 0;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int u = __shfl_up(v, d, 64);
                    if (lane >= d) v += u;
                }
                v += c == 0 ? carry0 : c == 1 ? carry1 : carry2;
                if (act) row[(size_t)x * C + c] = (uint8_t)v;
                const int last = __shfl(v, 63, 64) & 255;
                if (c == 0) carry0 = last; else if (c == 1) carry1 = last; else carry2 = last;
            }
        }
    }
}

// unfiltered rows -> RGB u8, as Pillow's convert('RGB') maps them: grey 1 bit -> 0 / 255, 2 bit -> v * 85, 4 bit -> v * 17; palette
// looked up; alpha dropped; grey replicated
__global__ __launch_bounds__(256) void pd_expand(const PdFile* __restrict__ F, const uint8_t* __restrict__ filt, const int* __restrict__ err,
                                                 uint8_t* __restrict__ out) {
    const PdFile& f = F[blockIdx.y];
    if (!f.valid || err[blockIdx.y]) return;
    const size_t npx = (size_t)f.width * f.height;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < npx; p += (size_t)gridDim.x * 256) {
        const int y = (int)(p / f.width), x = (int)(p - (size_t)y * f.width);
        const uint8_t* row = filt + f.foff + (size_t)y * (f.rb + f.fb) + f.fb;
        int r, g, b;
        if (f.depth < 8) {
            const int d = f.depth, bit = x * d;
            const int v = (row[bit >> 3] >> (8 - d - (bit & 7))) & ((1 << d) - 1);
            if (f.ct == 3) { r = f.pal[3 * v]; g = f.pal[3 * v + 1]; b = f.pal[3 * v + 2]; }
            else { r = g = b = d == 1 ? v * 255 : d == 2 ? v * 85 : v * 17; if (f.invert) r = g = b = 255 - r; }
        } else {
            switch (f.ct) {
                case 0: r = g = b = f.invert ? 255 - row[x] : row[x]; break;
                case 2: r = row[3 * x]; g = row[3 * x + 1]; b = row[3 * x + 2]; break;
                case 3: { const int v = row[x]; r = f.pal[3 * v]; g = f.pal[3 * v + 1]; b = f.pal[3 * v + 2]; } break;
                case 4: r = g = b = row[2 * x]; break;
                default: r = row[4 * x]; g = row[4 * x + 1]; b = row[4 * x + 2]; break;
            }
        }
        uint8_t* o = out + (((size_t)f.out_index * f.height + y) * f.width + x) * 3;
        o[0] = (uint8_t)r; o[1] = (uint8_t)g; o[2] = (uint8_t)b;
    }
}

__global__ void pd_status(const PdFile* __restrict__ F, const int* __restrict__ err, int* __restrict__ status, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) status[i] = F[i].valid ? (err[i] ? -1 : 0) : -1;
}

// ---------------- host: chunk walk ----------------
inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

struct CrcTable {
    uint32_t t[256];
    CrcTable() {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[i] = c;
        }
    }
};
uint32_t crc32_of(const uint8_t* p, size_t n) {
    static const CrcTable table;   // (thread-safe initialisation: probes run on provider threads)
    const uint32_t* crc_table = table.t;
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = crc_table[(c ^ p[i]) & 255] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

// EXIF Orientation from an eXIf payload (a TIFF stream); 0 when absent or unreadable
int exif_orientation(const uint8_t* s, size_t n) {
    if (n >= 6 && memcmp(s, "Exif\0\0", 6) == 0) { s += 6; n -= 6; }
    if (n < 8) return 0;
    const bool le = s[0] == 'I' && s[1] == 'I';
    if (!le && !(s[0] == 'M' && s[1] == 'M')) return 0;
    auto u16 = [&](size_t o) -> unsigned { return le ? s[o] | (s[o + 1] << 8) : (s[o] << 8) | s[o + 1]; };
    auto u32 = [&](size_t o) -> uint32_t { return le ? (uint32_t)u16(o) | ((uint32_t)u16(o + 2) << 16) : ((uint32_t)u16(o) << 16) | u16(o + 2); };
    const uint32_t ifd = u32(4);
    if ((size_t)ifd + 2 > n) return 0;
    const unsigned cnt = u16(ifd);
    for (unsigned k = 0; k < cnt; ++k) {
        const size_t e = ifd + 2 + 12 * (size_t)k;
        if (e + 12 > n) return 0;
        if (u16(e) == 0x0112 && u16(e + 2) == 3) return (int)u16(e + 8);
    }
    return 0;
}

struct Walk {
    PdInfo info{};
    uint8_t pal[768];
    std::vector<std::pair<size_t, size_t>> idat;   // (offset, length) of every IDAT payload
    size_t zlen = 0;
    int fb = 1, tiff = 0, invert = 0;   // PdFile's row-stage fields (a PNG file: filter bytes, nothing else)
};

// header = true: stop at the first IDAT (the probe).  Returns 0 / -1 / -2 as pngdec_probe.
int walk(const uint8_t* f, size_t n, Walk* w, bool header) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    PdInfo& I = w->info;
    memset(&I, 0, sizeof(I));
    if (n < 8 || memcmp(f, sig, 8) != 0) return -1;
    size_t p = 8;
    bool ihdr = false, plte = false, unsupported = false;
    for (;;) {
        if (p + 12 > n) return -1;
        const uint32_t len = be32(f + p);
        if (len > 0x7FFFFFFFu || p + 12 + (size_t)len > n) return -1;
        const uint8_t* type = f + p + 4;
        const uint8_t* s = f + p + 8;
        const bool is_idat = memcmp(type, "IDAT", 4) == 0;
        if (!ihdr && memcmp(type, "IHDR", 4) != 0) return -1;
        if (is_idat) break;
        // every chunk before IDAT: Pillow checks its CRC at open
        if (crc32_of(type, 4 + (size_t)len) != be32(s + len)) return -1;
        if (memcmp(type, "IHDR", 4) == 0) {
            if (ihdr || len != 13) return -1;
            ihdr = true;
            I.width = (int)be32(s); I.height = (int)be32(s + 4);
            I.bit_depth = s[8]; I.color_type = s[9]; I.interlace = s[12];
            if (be32(s) == 0 || be32(s + 4) == 0 || be32(s) > 0x7FFFFFFFu || be32(s + 4) > 0x7FFFFFFFu) return -1;
            const int d = s[8], ct = s[9];
            const bool ok = (ct == 0 && (d == 1 || d == 2 || d == 4 || d == 8 || d == 16)) || (ct == 3 && (d == 1 || d == 2 || d == 4 || d == 8)) ||
                            ((ct == 2 || ct == 4 || ct == 6) && (d == 8 || d == 16));
            if (!ok || s[10] != 0 || s[11] != 0 || s[12] > 1) return -1;
            if (d == 16 || s[12] == 1) unsupported = true;
        } else if (memcmp(type, "PLTE", 4) == 0) {
            if (plte || len % 3 != 0 || len < 3 || len > 768 || I.color_type == 0 || I.color_type == 4) return -1;
            plte = true;
            I.palette_size = (int)(len / 3);
            memcpy(w->pal, s, len);
        } else if (memcmp(type, "IEND", 4) == 0) {
            return -1;
        } else if (memcmp(type, "tRNS", 4) == 0) {
            if ((I.color_type == 0 && len < 2) || (I.color_type == 2 && len < 6)) return -1;   // (Pillow reads these many bytes)
        } else if (memcmp(type, "gAMA", 4) == 0) {
            if (len < 4) return -1;
        } else if (memcmp(type, "sRGB", 4) == 0) {
            if (len < 1) return -1;
        } else if (memcmp(type, "pHYs", 4) == 0) {
            if (len < 9) return -1;
        } else if (memcmp(type, "eXIf", 4) == 0) {
            I.orientation = exif_orientation(s, len);
        } else if (memcmp(type, "iCCP", 4) == 0 || memcmp(type, "zTXt", 4) == 0 || memcmp(type, "iTXt", 4) == 0 ||
                   memcmp(type, "acTL", 4) == 0 || memcmp(type, "fcTL", 4) == 0 || memcmp(type, "fdAT", 4) == 0) {
            unsupported = true;   // compressed metadata Pillow inflates at open, or animation: left to Pillow
        } else if (!(type[0] & 0x20)) {
            unsupported = true;   // an unknown critical chunk
        }
        p += 12 + (size_t)len;
    }
    if (I.color_type == 3 && !plte) return -1;
    if (header) return unsupported ? -2 : 0;
    // the IDAT run, then exactly one well-formed IEND
    for (;;) {
        const uint32_t len = be32(f + p);
        w->idat.emplace_back(p + 8, (size_t)len);
        w->zlen += len;
        p += 12 + (size_t)len;
        if (p + 12 > n) return -1;   // (a missing / truncated IEND)
        const uint32_t nl = be32(f + p);
        if (nl > 0x7FFFFFFFu || p + 12 + (size_t)nl > n) return -1;
        if (memcmp(f + p + 4, "IDAT", 4) != 0) break;
    }
    if (memcmp(f + p + 4, "IEND", 4) != 0) return -2;   // chunks after the image data (or between IDATs)
    if (be32(f + p) != 0 || be32(f + p + 8) != 0xAE426082u) return -1;
    if (p + 12 != n) return -2;   // bytes after IEND
    return unsupported ? -2 : 0;
}

struct PdWorkspace { PdFile* F; int* err; unsigned* adler_want; int* status; uint8_t *z, *filt; uint2* part; };
PdWorkspace pd_layout(Arena& a, int n, size_t z_total, size_t filt_total, size_t adler_blocks) {
    PdWorkspace w;
    w.F = a.take<PdFile>(n); w.err = a.take<int>(n); w.adler_want = a.take<unsigned>(n); w.status = a.take<int>(n);
    w.z = a.take<uint8_t>(z_total); w.filt = a.take<uint8_t>(filt_total); w.part = a.take<uint2>(adler_blocks + 1);
    return w;
}


// the device half of both entries: W[i] describes stream i (the pieces of files[i] that make up its zlib stream, its sample layout and
// row stage) where status[i] == 0
int pd_run_walked(lumina_ocr* eng, const std::vector<Walk>& W, const uint8_t* const* files, int n, int height, int width, uint8_t* out_dev,
                  int* status, hipStream_t st, const char* what) {
    std::vector<size_t> fbytes((size_t)n, 0);
    bool any_fb = false, any_tiff = false;
    for (int i = 0; i < n; ++i) {
        const Walk& w = W[(size_t)i];
        int rc = status[i];
        if (rc == 0) {
            const int ch = w.info.color_type == 2 ? 3 : w.info.color_type == 4 ? 2 : w.info.color_type == 6 ? 4 : 1;
            const size_t rb = ((size_t)width * ch * w.info.bit_depth + 7) / 8;
            const size_t total = (size_t)height * (rb + (size_t)w.fb);
            if (rb > (size_t)PD_MAX_ROW || total >= ((size_t)1 << 31) || w.zlen >= ((size_t)1 << 29) - 4096) rc = -2;   // (32-bit byte offsets; bit positions, with the reader's look-ahead)
            fbytes[(size_t)i] = total;
            if (rc == 0) { any_fb |= w.fb != 0; any_tiff |= w.tiff != 0; }
        }
        status[i] = rc;
    }
    lumina_ocr::Staging& stage = eng->pd_stage;
    if (!stage.uploaded) {
        hipEvent_t ev = nullptr;
        LOCR_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        stage.uploaded.reset(ev);
    }
    // sub-batches of at most eng->pd_sub_batch_mb MB of filtered scanlines (at least one file each): the workspace holds one sub-batch
    const size_t sub_filt = (size_t)eng->pd_sub_batch_mb << 20;
    int i0 = 0;
    while (i0 < n) {
        int i1 = i0;
        size_t fsum = 0;
        while (i1 < n && (i1 == i0 || fsum + fbytes[(size_t)i1] <= sub_filt)) { if (status[i1] == 0) fsum += fbytes[(size_t)i1]; ++i1; }
        const int nb = i1 - i0;
        std::vector<PdFile> F((size_t)nb);
        size_t z_total = 0, filt_total = 0, ablk_total = 0, max_ablk = 0;
        int any = 0;
        for (int k = 0; k < nb; ++k) {
            PdFile& f = F[(size_t)k];
            memset(&f, 0, sizeof(f));
            const int i = i0 + k;
            if (status[i] != 0) continue;
            const Walk& w = W[(size_t)i];
            f.valid = 1; ++any;
            f.width = width; f.height = height; f.ct = w.info.color_type; f.depth = w.info.bit_depth; f.out_index = i;
            const int ch = f.ct == 2 ? 3 : f.ct == 4 ? 2 : f.ct == 6 ? 4 : 1;
            f.bpp = f.depth < 8 ? 1 : ch;
            f.rb = (unsigned)(((size_t)width * ch * f.depth + 7) / 8);
            f.total = (unsigned)fbytes[(size_t)i];
            f.npal = w.info.palette_size;
            f.fb = w.fb; f.tiff = w.tiff; f.invert = w.invert;
            if (f.ct == 3) memcpy(f.pal, w.pal, (size_t)f.npal * 3);
            f.zlen = (unsigned)w.zlen;
            f.zoff = z_total; z_total += ((w.zlen + 255) & ~(size_t)255) + PD_Z_PAD;
            f.foff = filt_total; filt_total += ((fbytes[(size_t)i] + 255) & ~(size_t)255) + 256;
            const size_t nab = (fbytes[(size_t)i] + PD_ADLER_BLK - 1) / PD_ADLER_BLK;
            f.ablk_off = (int)ablk_total; ablk_total += nab;
            if (nab > max_ablk) max_ablk = nab;
        }
        if (any) {
            LOCR_CHECK(hipEventSynchronize(stage.uploaded.get()));
            LOCR_CHECK(stage.buf.reserve(z_total, stage.uploaded.get()));
            uint8_t* zs = stage.buf.get();
            for (int k = 0; k < nb; ++k) {
                PdFile& f = F[(size_t)k];
                if (!f.valid) continue;
                const Walk& w = W[(size_t)(i0 + k)];
                uint8_t* d = zs + f.zoff;
                for (const auto& c : w.idat) { memcpy(d, files[i0 + k] + c.first, c.second); d += c.second; }
                memset(d, 0, (zs + f.zoff + ((w.zlen + 255) & ~(size_t)255) + PD_Z_PAD) - d);
                // zlib header: CM 8, CINFO <= 7, FCHECK, no preset dictionary
                const uint8_t* h = zs + f.zoff;
                if (f.zlen < 6 || (h[0] & 15) != 8 || (h[0] >> 4) > 7 || ((h[0] << 8) | h[1]) % 31 != 0 || (h[1] & 0x20)) {
                    status[i0 + k] = -1; f.valid = 0; --any; continue;
                }
                f.wsize = 1 << ((h[0] >> 4) + 8);
            }
        }
        if (any) {
            Arena sizing;
            pd_layout(sizing, nb, z_total, filt_total, ablk_total);
            if (eng_ws_reserve(eng, sizing.off)) return 1;
            Arena a(eng->ws.get(), eng->ws.cap);
            const PdWorkspace w = pd_layout(a, nb, z_total, filt_total, ablk_total);
            if (a.overflow) return locr_fail(eng, what, "workspace layout exceeds the reservation");
            LOCR_CHECK(hipMemcpyAsync(w.F, F.data(), sizeof(PdFile) * nb, hipMemcpyHostToDevice, st));
            LOCR_CHECK(hipMemcpyAsync(w.z, stage.buf.get(), z_total, hipMemcpyHostToDevice, st));
            LOCR_CHECK(hipEventRecord(stage.uploaded.get(), st));
            LOCR_CHECK(hipMemsetAsync(w.err, 0, sizeof(int) * nb, st));
            hipLaunchKernelGGL(pd_inflate, dim3(nb), dim3(64), 0, st, w.F, w.z, w.filt, w.err, w.adler_want);
            hipLaunchKernelGGL(pd_adler_part, dim3((unsigned)max_ablk, nb), dim3(256), 0, st, w.F, w.filt, w.err, w.part);
            hipLaunchKernelGGL(pd_adler_fin, dim3(nb), dim3(256), 0, st, w.F, w.filt, w.part, w.adler_want, w.err);
            if (any_fb) hipLaunchKernelGGL(pd_unfilter, dim3(nb), dim3(64), 0, st, w.F, w.filt, w.err);
            pd_rows_to_rgb(w.F, w.filt, w.err, nb, height, width, any_tiff, out_dev, st);
            hipLaunchKernelGGL(pd_status, dim3((nb + 63) / 64), dim3(64), 0, st, w.F, w.err, w.status, nb);
            std::vector<int> dev_status((size_t)nb);
            LOCR_CHECK(hipMemcpyAsync(dev_status.data(), w.status, sizeof(int) * nb, hipMemcpyDeviceToHost, st));
            LOCR_CHECK(hipStreamSynchronize(st));
            LOCR_CHECK(hipGetLastError());
            for (int k = 0; k < nb; ++k)
                if (F[(size_t)k].valid) status[i0 + k] = dev_status[(size_t)k];
        }
        i0 = i1;
    }
    return 0;
}

}  // namespace

void pd_rows_to_rgb(const PdFile* F, uint8_t* rows, const int* err, int nb, int height, int width, bool any_tiff, uint8_t* out_dev, hipStream_t st) {
    if (any_tiff) hipLaunchKernelGGL(pd_tiff_predict, dim3((unsigned)std::min(height, 1024), nb), dim3(64), 0, st, F, rows, err);
    const size_t npx = (size_t)width * height;
    hipLaunchKernelGGL(pd_expand, dim3((unsigned)std::min<size_t>((npx + 255) / 256, 4096), nb), dim3(256), 0, st, F, rows, err, out_dev);
}

size_t pngdec_workspace_bytes(int n, size_t z_total, size_t filt_total, size_t adler_blocks) {
    Arena a;
    pd_layout(a, n, z_total, filt_total, adler_blocks);
    return a.off;
}

int pngdec_probe(const uint8_t* file, size_t n, PdInfo* info) {
    Walk w;
    const int rc = walk(file, n, &w, true);
    if (info) *info = w.info;
    return rc;
}

int pngdec_run(lumina_ocr* eng, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev, int* status,
               hipStream_t st) {
    std::vector<Walk> W((size_t)n);
    for (int i = 0; i < n; ++i) {
        Walk& w = W[(size_t)i];
        int rc = walk(files[i], sizes[i], &w, false);
        if (rc == 0 && (w.info.width != width || w.info.height != height)) rc = -4;
        status[i] = rc;
    }
    return pd_run_walked(eng, W, files, n, height, width, out_dev, status, st, "png_decode");
}

int flate_image_run(lumina_ocr* eng, const uint8_t* const* streams, const size_t* sizes, int n, int height, int width, const int* params,
                    const uint8_t* const* palettes, uint8_t* out_dev, int* status, hipStream_t st) {
    std::vector<Walk> W((size_t)n);
    for (int i = 0; i < n; ++i) {
        Walk& w = W[(size_t)i];
        const int* q = params + 5 * (size_t)i;
        const int predictor = q[0], comps = q[1], depth = q[2], indexed = q[3], invert = q[4];
        memset(&w.info, 0, sizeof(w.info));
        bool ok = (predictor == 1 || predictor == 2 || (predictor >= 10 && predictor <= 15)) && (comps == 1 || comps == 3) &&
                  (depth == 8 || (comps == 1 && (depth == 1 || depth == 2 || depth == 4)));
        if (predictor == 2 && depth != 8) ok = false;           // (TIFF differencing of packed samples: not taken)
        if (indexed && (comps != 1 || invert || !palettes || !palettes[i])) ok = false;
        if (invert && comps != 1) ok = false;
        if (!ok) { status[i] = -2; continue; }
        if (!streams[i] || sizes[i] == 0) { status[i] = -1; continue; }
        w.info.width = width; w.info.height = height; w.info.bit_depth = depth;
        w.info.color_type = indexed ? 3 : comps == 3 ? 2 : 0;
        if (indexed) { w.info.palette_size = 256; memcpy(w.pal, palettes[i], 768); }
        w.idat.emplace_back((size_t)0, sizes[i]);
        w.zlen = sizes[i];
        w.fb = predictor >= 10; w.tiff = predictor == 2; w.invert = invert != 0;
        status[i] = 0;
    }
    return pd_run_walked(eng, W, streams, n, height, width, out_dev, status, st, "flate_image_decode");
}
