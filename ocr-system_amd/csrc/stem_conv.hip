// Stem convolution fused with input normalisation: u8 HWC page/crop -> 3x3 / stride 2 conv (Cin = 3)
// -> bias + activation -> bf16 NHWC.  Also a standalone normalise kernel (u8 HWC -> bf16 NHWC/NCHW).
//
// The reference has no normalise-to-tensor step (its pre-processing stops at PIL images:
// /root/reference/backend/utils/image_preprocessing.py:191-242); the definition
//   xn = bf16( float(u8) * scale_c + shift_c ),  0 outside the valid page
// is the build's (oracle/nets.py det_normalize / rec_normalize).
//
// One workgroup = 8 x 32 output pixels.  The (17 x 65) x 3 input halo is normalised once into
// LDS as bf16; K = 27 (padded to 32) is two 32x32x16 MFMA steps whose B fragments are gathered
// from LDS (for a fixed kh the 9 (kw, c) values of a pixel are contiguous), weights (A operand,
// 2 KB, pre-packed [kstep][half][cout][8]) come straight from L2.  (stem_conv_kernel: recogniser and classifier stems, and
// the detector's conv1 when it runs un-fused.)
//
// stem12_kernel further down is the detector's conv1 + conv2 in one persistent kernel (its own comment has the structure).  It
// shares no device code with stem_conv_kernel / fill_halo_u8: the two-kernel path is what tests compare it with, bit for bit.
#include "stem_conv.h"

#include <algorithm>
#include <type_traits>

namespace {

constexpr int TH = 8, TW = 32;
constexpr int HH = 2 * (TH - 1) + 3, HW = 2 * (TW - 1) + 3;  // 17 x 65
constexpr int ROW = HW * 3 + 1;                              // bf16 elements per halo row (odd -> fewer conflicts)
constexpr int STAGE_PITCH = 32 * 2 + 16;

// Normalised bf16 halo of one workgroup: rows iy0 .. iy0 + NHH - 1, pixels ix0 .. ix0 + NHW - 1 of image n_img, 3 channels
// interleaved, NROW = NHW * 3 + 1 elements per LDS row (element NHW * 3 of every row is a dump slot nobody reads).
// Aligned 4-byte words of every row segment, all requested before the first is used; addresses are 32-bit offsets from a
// 4-byte-aligned, workgroup-uniform base inside this image; e0 = position of a word's first byte in its row segment.  The
// arithmetic per byte is straight-line (masks and selected indices, no branches: a conditional on the value makes hipcc
// branch around the conversion, ~35 instructions per byte with the old 64-bit offsets against ~9 now).
template <int NHH, int NHW, int NROW>
__device__ __forceinline__ void fill_halo_u8(bf16_t* halo, const StemParams& p, int n_img, int iy0, int ix0, int vh, int vw, int tid) {
    constexpr int SEG = NHW * 3, WPR = (SEG + 3) / 4 + 1, NIT = (NHH * WPR + 255) / 256;
    static_assert(NROW > SEG, "one dump element per row");
    const long long img_off = (long long)n_img * p.H * p.W * 3, all_bytes = (long long)p.N * p.H * p.W * 3;
    const unsigned char* xal = p.x + (img_off & ~3ll);       // p.x is an allocation base (>= 4-byte aligned)
    const int mis = (int)(img_off & 3);
    const long long lo64 = -(img_off & ~3ll), hi64 = all_bytes - (img_off & ~3ll);      // valid byte range relative to xal ...
    const int lo_lim = lo64 < -0x7fffffffll ? -0x7fffffff : (int)lo64, hi_lim = hi64 > 0x7fffffffll ? 0x7fffffff : (int)hi64;   // ... clamped: offsets are 32-bit
    const float sc0 = p.scale[0], sc1 = p.scale[1], sc2 = p.scale[2], sh0 = p.shift[0], sh1 = p.shift[1], sh2 = p.shift[2];
    uint32_t word[NIT];
    int e0s[NIT];
#pragma unroll
    for (int u = 0; u < NIT; ++u) {
        const int i = tid + 256 * u;
        const int hy = i / WPR, wi = i - hy * WPR, iy = iy0 + hy;
        const int q = mis + (iy * p.W + ix0) * 3;            // segment start relative to xal (negative at x = -1, y = 0)
        const int w0 = (q & ~3) + 4 * wi;                    // this thread's aligned word
        e0s[u] = w0 - q;
        // words that start before the tensor hold only pixels left of the page (zeroed below); the one word that may
        // straddle the tensor's end is patched after the loop
        const bool ld = i < NHH * WPR && iy >= 0 && iy < vh && w0 >= lo_lim && w0 + 4 <= hi_lim;
        const uint32_t wv = *reinterpret_cast<const uint32_t*>(xal + (ld ? w0 : 0));   // xal itself is always readable: lo_lim <= 0 < hi_lim
        word[u] = ld ? wv : 0u;
    }
    if (hi_lim & 3) {                                        // tensor size not a multiple of 4: its last, partial word byte by byte
#pragma unroll 1
        for (int u = 0; u < NIT; ++u) {
            const int i = tid + 256 * u;
            const int hy = i / WPR, wi = i - hy * WPR, iy = iy0 + hy;
            const int q = mis + (iy * p.W + ix0) * 3, w0 = (q & ~3) + 4 * wi;
            if (i < NHH * WPR && iy >= 0 && iy < vh && w0 >= lo_lim && w0 < hi_lim && w0 + 4 > hi_lim) {
                uint32_t wv = 0;
                for (int b = 0; b < 4; ++b) if (w0 + b < hi_lim) wv |= (uint32_t)xal[w0 + b] << (8 * b);
#pragma unroll
                for (int uu = 0; uu < NIT; ++uu) if (uu == u) word[uu] = wv;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < NIT; ++u) {
        const int i = tid + 256 * u;
        const int hy = min(i / WPR, NHH - 1), iy = iy0 + hy;
        const bool rowin = iy >= 0 && iy < vh, item = i < NHH * WPR;
        const int e0 = e0s[u];                                // -3 .. SEG + 3
        const int hx0 = (e0 + 3) / 3 - 1, c0 = e0 - hx0 * 3;  // pixel and channel of the word's first byte (e0 >= -3)
        bf16_t* hrow = halo + hy * NROW;
        // the channels of the four bytes are c0, c0+1, c0+2, c0 (mod 3): rotate the constants once per word
        float S[4], T[4];
        S[0] = c0 == 0 ? sc0 : (c0 == 1 ? sc1 : sc2); S[1] = c0 == 0 ? sc1 : (c0 == 1 ? sc2 : sc0); S[2] = c0 == 0 ? sc2 : (c0 == 1 ? sc0 : sc1); S[3] = S[0];
        T[0] = c0 == 0 ? sh0 : (c0 == 1 ? sh1 : sh2); T[1] = c0 == 0 ? sh1 : (c0 == 1 ? sh2 : sh0); T[2] = c0 == 0 ? sh2 : (c0 == 1 ? sh0 : sh1); T[3] = T[0];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int e = e0 + b;
            const int ix = ix0 + hx0 + ((c0 + b >= 3) ? 1 : 0);
            float v = (float)((word[u] >> (8 * b)) & 0xffu) * S[b];
            v = v + T[b];
            const uint32_t keep = (rowin && (unsigned)ix < (unsigned)vw) ? 0xffffu : 0u;   // 0 outside the page
            const int idx = (item && (unsigned)e < (unsigned)SEG) ? e : SEG;
            hrow[idx] = (bf16_t)(f32_to_bf16(v) & keep);
        }
    }
}

// halo offsets of a lane's 16 K-indices (k = ks * 16 + h * 8 + j -> row kh = k / 9, element kr = k % 9), the same for every
// pixel; the five padding indices (k >= 27) re-read element 0: their weights are zero and the data is finite
template <int NROW>
__device__ __forceinline__ void stem_koff(int h, int (&koff)[2][8]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = ks * 16 + h * 8 + j, kh = k / 9;
            koff[ks][j] = k < 27 ? kh * NROW + (k - kh * 9) : 0;
        }
}

__global__ __launch_bounds__(256) void stem_conv_kernel(const StemParams p) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[256 * STAGE_PITCH > HH * ROW * 2 ? 256 * STAGE_PITCH : HH * ROW * 2];
    bf16_t* halo = reinterpret_cast<bf16_t*>(smem);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int tiles_x = (p.Wo + TW - 1) / TW, tiles_y = (p.Ho + TH - 1) / TH;
    const int bid = blockIdx.x;
    const int n_img = bid / (tiles_x * tiles_y);
    const int trem = bid - n_img * tiles_x * tiles_y;
    const int tile_y = trem / tiles_x, tile_x = trem - tile_y * tiles_x;
    const int vw = p.valid_w_per_img ? p.valid_w_per_img[n_img] : p.valid_w;
    const int vh = p.valid_h;

    // ---- stage + normalise the halo ----
    const int iy0 = tile_y * TH * 2 - 1, ix0 = tile_x * TW * 2 - 1;
    fill_halo_u8<HH, HW, ROW>(halo, p, n_img, iy0, ix0, vh, vw, tid);
    __syncthreads();

    // ---- MFMA: D[cout][pixel] ----
    f32x16_t acc[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[mt][j] = 0.f;
    int koff[2][8];
    stem_koff<ROW>(h, koff);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const bf16x8_t afr = *reinterpret_cast<const bf16x8_t*>(p.wpk + ((ks * 2 + h) * 32 + r) * 8);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const bf16_t* hb = halo + (2 * (wave * 2 + mt)) * ROW + 6 * r;
            union { bf16x8_t v; bf16_t s[8]; } b;
#pragma unroll
            for (int j = 0; j < 8; ++j) b.s[j] = hb[koff[ks][j]];
            acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afr, b.v, acc[mt], 0, 0, 0);
        }
    }
    __syncthreads();

    // ---- epilogue ----
    unsigned char* stage = smem;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 b4 = *reinterpret_cast<const float4*>(p.bias + 8 * g + 4 * h);
            acc[mt][4 * g + 0] += b4.x; acc[mt][4 * g + 1] += b4.y; acc[mt][4 * g + 2] += b4.z; acc[mt][4 * g + 3] += b4.w;
        }
    // the activation switch once per kernel, not once per element
#define STEM_ALL(expr) _Pragma("unroll") for (int mt = 0; mt < 2; ++mt) _Pragma("unroll") for (int j = 0; j < 16; ++j) { const float v = acc[mt][j]; acc[mt][j] = (expr); }
    if (p.act == ACT_RELU) { STEM_ALL(fmaxf(v, 0.f)) }
    else if (p.act == ACT_HSWISH) { STEM_ALL(v * fminf(fmaxf(v + 3.f, 0.f), 6.f) * (1.f / 6.f)) }
    else if (p.act != ACT_NONE) { STEM_ALL(apply_act(v, p.act)) }
#undef STEM_ALL
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        const int tp = (wave * 2 + mt) * TW + r;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            uint2 o;
            o.x = pack_bf16x2(acc[mt][4 * g + 0], acc[mt][4 * g + 1]);
            o.y = pack_bf16x2(acc[mt][4 * g + 2], acc[mt][4 * g + 3]);
            *reinterpret_cast<uint2*>(stage + tp * STAGE_PITCH + (8 * g + 4 * h) * 2) = o;
        }
    }
    __syncthreads();
    const int cpp = p.Cout_store / 8;  // 16-byte chunks stored per pixel (1..4)
    for (int i = tid; i < 256 * cpp; i += 256) {
        const int tp = i / cpp, ch = i - tp * cpp;
        const int ty = tp / TW, tx = tp - ty * TW;
        const int oy = tile_y * TH + ty, ox = tile_x * TW + tx;
        if (oy >= p.Ho || ox >= p.Wo) continue;
        const uint4 v = *reinterpret_cast<const uint4*>(stage + tp * STAGE_PITCH + ch * 16);
        *reinterpret_cast<uint4*>(p.y + (((size_t)n_img * p.Ho + oy) * p.Wo + ox) * p.Cout_store + ch * 8) = v;
    }
}

// ---- stem.conv1 + stem.conv2 fused (DBNet): u8 page -> conv 3x3/s2 (3 -> 32) + ReLU -> conv 3x3/s1 (32 -> 32) + ReLU ----
// The 32-channel half-resolution tensor between the two (46 MB per A4 page, written and read back) only exists as an LDS tile.
// A tile is 8 x 32 output pixels of conv2.  STEM12_WGS_PER_CU work-groups per CU stay resident and walk the tiles
// blockIdx.x, + gridDim.x, ... (neighbouring tiles run on neighbouring work-groups at the same time: their halos meet in L2).
// Once per work-group: all 18 weight fragments of conv2 (72 registers), conv1's packed weights and both bias vectors (LDS), and
// the thread's phase-A descriptor (two registers).  Per tile:
//   A  the (21 x 69) x 3 u8 input region is read as aligned 4-byte words, five consecutive words of one row per thread (one
//      16-byte and one 4-byte load), requested one tile ahead, before conv2 of the tile in flight, and normalised into LDS as
//      bf16: float(u8) * scale, + shift, one rounding; 0 outside the page.  Channel rotation, row test, page mask and LDS address
//      are formed once per thread.  Which bytes of which row a thread holds depends on the tile only through the alignment
//      (mod 4) of the tile's first byte, the same for every tile of an image: the descriptor is rebuilt only when it changes;
//   B  conv1 on the matrix cores for the 10 x 34 pixels conv2 needs (11 column tiles of 32 over the four waves).  For a fixed
//      kernel row the 9 (kw, c) values of a pixel are 18 contiguous, 4-byte aligned bytes: 9 aligned dwords per lane and 8
//      v_perm_b32 put the 16 k-values of both MFMA steps in order (the five padding k re-read element 0, as stem_conv_kernel
//      does).  + bias, ReLU, bf16 — pixels outside the half-resolution image become ZERO (conv2 pads its input, not conv1's) —
//      written to a [pixel][32 ch] LDS tile, 80 bytes per pixel (conv2's 16-byte fragment reads at that lane stride are
//      conflict free, and every one of them sits at a compile-time distance from one per-lane address);
//   C  conv2: 2 chunks of 16 channels x 9 taps (the order of the stand-alone kernel: identical sums); the two output rows of a
//      wave share the fragments of the t1 rows they both read (24 fragment reads for 36 MFMAs); bias, ReLU and bf16 packing in
//      registers, v_permlane32_swap makes 16-byte pieces, stored directly (after the next tile's words have been requested).
// Order in the tile loop: barrier (halo complete) - B - barrier (t1 complete) - request words of tile t+1 - C of tile t - A of
// tile t+1 - epilogue and stores of tile t.  Two barriers per tile.
constexpr int F_T1H = TH + 2, F_T1W = TW + 2, F_T1PX = F_T1H * F_T1W;           // 10 x 34 = 340 conv1 pixels
constexpr int F_HH = 2 * (F_T1H - 1) + 3, F_HW = 2 * (F_T1W - 1) + 3;           // 21 x 69 input pixels
constexpr int STEM12_WGS_PER_CU = 3;            // 38 KB of LDS and 164 VGPRs per work-group: three waves per SIMD
constexpr int W_SEG = F_HW * 3;                 // bytes of one halo row segment
constexpr int W_WPR = (W_SEG + 3) / 4 + 1;      // aligned words that cover it at any alignment (53)
constexpr int W_RUN = 5;                        // consecutive words of one row per thread
constexpr int W_RPR = (W_WPR + W_RUN - 1) / W_RUN;   // runs per row (11; the last one reaches two words past the segment)
static_assert(F_HH * W_RPR <= 256, "one run per thread");
constexpr int W_LEAD = 4;                       // slack elements in front of a row: a word's bytes left of the segment land there
constexpr int W_ROW = W_LEAD + 4 * W_RPR * W_RUN;    // 224 bf16 elements per LDS row (even: pixel starts are 4-byte aligned); slack behind too
constexpr int W_ROWB = W_ROW * 2;
constexpr int W_DUMP = F_HH * W_ROWB;           // 48 bytes for the threads without a run
constexpr int W_BIAS = W_DUMP + 48;             // conv1's and conv2's bias, 32 floats each
constexpr int W_A1 = W_BIAS + 256;              // conv1's packed weights [2][2][32][8] bf16
constexpr int W_T1 = W_A1 + 2048;
constexpr int T1_PITCH = 32 * 2 + 16;           // bytes per t1 pixel: 16-byte fragment reads at this lane stride are conflict free
constexpr int W_T1_BYTES = F_T1PX * T1_PITCH;
static_assert(W_ROW % 2 == 0 && W_BIAS % 16 == 0 && W_A1 % 16 == 0 && W_T1 % 16 == 0 && W_DUMP < 0x10000, "LDS layout");

// Phase-A run of one thread (W_RUN aligned words of one halo row): goff = byte offset of its first word from the tile's aligned
// origin; desc = LDS byte address of the first word's first element | channel of its first byte << 16 | (halo pixel of its first
// byte + 1) << 18 | halo row << 25 | has-run << 30
struct Stem12Words { int goff; uint32_t desc; };
// a = (offset of the tile's first byte from the image's aligned base) & 3, pitch = bytes per page row
__device__ __forceinline__ void stem12_describe(Stem12Words& d, int a, int pitch, int wave) {
    // the thread's index from the lane count and the (scalar) wave index: nothing of this is kept ready across the tile loop for the next image
    int lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    const int tid = wave * 64 + lane;
    const bool item = tid < F_HH * W_RPR;
    const int hy = item ? tid / W_RPR : F_HH - 1, wi = item ? (tid - hy * W_RPR) * W_RUN : 0;
    const int rs = a + hy * pitch, s = rs & 3;                // the row segment starts s bytes into its first word
    const int e0 = 4 * wi - s;                                // position of the run's first byte in the segment, >= -3
    const int hx1 = (e0 + 3) / 3, c0 = e0 + 3 - hx1 * 3;
    const int lds = item ? (hy * W_ROW + W_LEAD + e0) * 2 : W_DUMP;
    d.goff = (rs & ~3) + 4 * wi;
    d.desc = (uint32_t)lds | (uint32_t)c0 << 16 | (uint32_t)hx1 << 18 | (uint32_t)hy << 25 | (item ? 1u << 30 : 0u);
}

// What of a tile does not depend on the thread
struct Stem12Tile {
    const unsigned char* xal;   // the image's base rounded down to 4 bytes (p.x is an allocation base, >= 4-byte aligned)
    int n_img, tile_y, tile_x;
    int iy0, ix0;               // page coordinates of the halo's first pixel
    int q0a, a;                 // offset of the halo's first byte from xal, rounded down to 4; its remainder
    int lo_lim, hi_lim;         // valid byte range relative to xal, clamped to 32 bits
    bool xin;                   // every halo column lies inside the page
};
__device__ __forceinline__ Stem12Tile stem12_tile(const StemParams& p, int t, int tiles_x, int tiles_per_img) {
    Stem12Tile c;
    c.n_img = t / tiles_per_img;
    const int trem = t - c.n_img * tiles_per_img;
    c.tile_y = trem / tiles_x; c.tile_x = trem - c.tile_y * tiles_x;
    c.iy0 = 2 * (c.tile_y * TH - 1) - 1; c.ix0 = 2 * (c.tile_x * TW - 1) - 1;
    const long long img_off = (long long)c.n_img * p.H * p.W * 3, all_bytes = (long long)p.N * p.H * p.W * 3;
    const long long base = img_off & ~3ll, lo64 = -base, hi64 = all_bytes - base;
    c.xal = p.x + base;
    c.lo_lim = lo64 < -0x7fffffffll ? -0x7fffffff : (int)lo64; c.hi_lim = hi64 > 0x7fffffffll ? 0x7fffffff : (int)hi64;
    const int q0 = (int)(img_off & 3) + (c.iy0 * p.W + c.ix0) * 3;   // negative at x = -1, y = 0
    c.a = q0 & 3; c.q0a = q0 - c.a;
    c.xin = c.ix0 >= 0 && c.ix0 + F_HW <= p.valid_w;
    return c;
}

// request a tile's words: all loads before the first use.  A run that lies inside the tensor and in a row of the page is five loads
// from one address; else word by word: words that start before the tensor hold only pixels left of the page (zeroed at
// conversion), words of rows outside the page are not read, the one word that may straddle the tensor's end is read byte by byte.
__device__ __forceinline__ void stem12_request(uint32_t (&word)[W_RUN], const Stem12Words& d, const StemParams& p, const Stem12Tile& c) {
    uint32_t desc = d.desc;
    asm volatile("" : "+v"(desc));                            // decoded here, per tile: kept decoded across the tile loop, the fields cost a register each
    const int hy = (int)(desc >> 25) & 31, w0 = c.q0a + d.goff;
    const bool row = (desc >> 30) != 0 && (unsigned)(c.iy0 + hy) < (unsigned)p.valid_h;
    if (row && w0 >= c.lo_lim && w0 + 4 * W_RUN <= c.hi_lim) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(c.xal + w0);
#pragma unroll
        for (int u = 0; u < W_RUN; ++u) word[u] = src[u];
    } else {
#pragma unroll
        for (int u = 0; u < W_RUN; ++u) {
            const int w = w0 + 4 * u;
            uint32_t wv = 0;
            if (row && w >= c.lo_lim && w < c.hi_lim) {
                if (w + 4 <= c.hi_lim) wv = *reinterpret_cast<const uint32_t*>(c.xal + w);
                else for (int b = 0; b < 4; ++b) if (w + b < c.hi_lim) wv |= (uint32_t)c.xal[w + b] << (8 * b);
            }
            word[u] = wv;
        }
    }
}

// words -> normalised bf16 in the halo.  The run's 20 values go to LDS elements W_LEAD + e0 .. + 19 of its row (the slack at both
// ends of a row takes the bytes that belong to the neighbouring pixels): ten 4-byte writes where that is 4-byte aligned, else
// 2 + nine 4-byte writes + 2 bytes.
__device__ __forceinline__ void stem12_convert(unsigned char* smem, const uint32_t (&word)[W_RUN], const Stem12Words& d, const StemParams& p, const Stem12Tile& c) {
    const float sc0 = p.scale[0], sc1 = p.scale[1], sc2 = p.scale[2], sh0 = p.shift[0], sh1 = p.shift[1], sh2 = p.shift[2];
    uint32_t desc = d.desc;
    asm volatile("" : "+v"(desc));                            // (as in stem12_request)
    const int c0 = (int)(desc >> 16) & 3, hy = (int)(desc >> 25) & 31;
    const bool rowin = (unsigned)(c.iy0 + hy) < (unsigned)p.valid_h;
    // byte b of word u has channel (c0 + 4 u + b) mod 3 = (c0 + u + b) mod 3: the constants are rotated once per run
    const bool is0 = c0 == 0, is1 = c0 == 1;
    float X[3], Y[3];
    X[0] = is0 ? sc0 : (is1 ? sc1 : sc2); X[1] = is0 ? sc1 : (is1 ? sc2 : sc0); X[2] = is0 ? sc2 : (is1 ? sc0 : sc1);
    Y[0] = is0 ? sh0 : (is1 ? sh1 : sh2); Y[1] = is0 ? sh1 : (is1 ? sh2 : sh0); Y[2] = is0 ? sh2 : (is1 ? sh0 : sh1);
    uint32_t pk[2 * W_RUN];                                   // element pairs in LDS order
#pragma unroll
    for (int u = 0; u < W_RUN; ++u) {
        const uint32_t w = word[u];
        float f0 = (float)(w & 0xffu) * X[u % 3], f1 = (float)((w >> 8) & 0xffu) * X[(u + 1) % 3];
        float f2 = (float)((w >> 16) & 0xffu) * X[(u + 2) % 3], f3 = (float)(w >> 24) * X[u % 3];
        f0 = f0 + Y[u % 3]; f1 = f1 + Y[(u + 1) % 3]; f2 = f2 + Y[(u + 2) % 3]; f3 = f3 + Y[u % 3];
        uint32_t m01, m23;                                    // 0 outside the page
        if (c.xin) {
            m01 = m23 = rowin ? 0xffffffffu : 0u;
        } else {
            // the word's first byte is byte cw of halo pixel hx; byte b belongs to the next pixel when cw + b >= 3
            const int t = c0 + 4 * u, dp = t / 3, cw = t - 3 * dp;
            const int ix = c.ix0 + ((int)(desc >> 18) & 127) - 1 + dp;
            const bool kA = rowin && (unsigned)ix < (unsigned)p.valid_w, kB = rowin && (unsigned)(ix + 1) < (unsigned)p.valid_w;
            const bool k1 = cw == 2 ? kB : kA, k2 = cw >= 1 ? kB : kA;
            m01 = (kA ? 0xffffu : 0u) | (k1 ? 0xffff0000u : 0u);
            m23 = (k2 ? 0xffffu : 0u) | (kB ? 0xffff0000u : 0u);
        }
        pk[2 * u] = pack_bf16x2(f0, f1) & m01; pk[2 * u + 1] = pack_bf16x2(f2, f3) & m23;
    }
    unsigned char* dst = smem + (desc & 0xffffu);
    if (desc & 2u) {
        *reinterpret_cast<uint16_t*>(dst) = (uint16_t)pk[0];
#pragma unroll
        for (int i = 0; i + 1 < 2 * W_RUN; ++i) *reinterpret_cast<uint32_t*>(dst + 2 + 4 * i) = (pk[i] >> 16) | (pk[i + 1] << 16);
        *reinterpret_cast<uint16_t*>(dst + 8 * W_RUN - 2) = (uint16_t)(pk[2 * W_RUN - 1] >> 16);
    } else {
#pragma unroll
        for (int i = 0; i < 2 * W_RUN; ++i) *reinterpret_cast<uint32_t*>(dst + 4 * i) = pk[i];
    }
}

// v_perm_b32 selectors: a result half from the low / high half of the first (X) or the second (Y) operand
constexpr uint32_t SEL_XL = 0x0504, SEL_XH = 0x0706, SEL_YL = 0x0100, SEL_YH = 0x0302;
constexpr uint32_t stem12_sel(uint32_t lo, uint32_t hi) { return lo | hi << 16; }
// bias + ReLU + one rounding to bf16 of two accumulator values; the two adds as one packed fp32 add (the same IEEE add per element)
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t stem12_bias_relu_pack(float a0, float a1, float b0, float b1) {
    const f32x2_t s = f32x2_t{a0, a1} + f32x2_t{b0, b1};
    return pack_bf16x2(fmaxf(s[0], 0.f), fmaxf(s[1], 0.f));
}
__device__ __forceinline__ uint32_t lds_u32(const unsigned char* smem, int off) { return *reinterpret_cast<const uint32_t*>(smem + off); }

__global__ __launch_bounds__(256, STEM12_WGS_PER_CU) void stem12_kernel(const StemParams p, const bf16_t* w2pk, const float* bias2) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[W_T1 + W_T1_BYTES];
    unsigned char* t1 = smem + W_T1;
    float* sbias = reinterpret_cast<float*>(smem + W_BIAS);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int tiles_x = (p.Wo + TW - 1) / TW, tiles_y = (p.Ho + TH - 1) / TH;
    const int tiles_per_img = tiles_x * tiles_y, tiles = p.N * tiles_per_img;

    // ---- once per work-group ----
    if (tid < 32) { sbias[tid] = p.bias[tid]; sbias[32 + tid] = bias2[tid]; }   // (read after the first barrier)
    if (tid < 128) *reinterpret_cast<uint4*>(smem + W_A1 + tid * 16) = *reinterpret_cast<const uint4*>(p.wpk + tid * 8);
    bf16x8_t w2[2][9];
#pragma unroll
    for (int kc = 0; kc < 2; ++kc)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) w2[kc][tap] = *reinterpret_cast<const bf16x8_t*>(w2pk + ((size_t)(2 * kc + h) * (9 * 32) + tap * 32 + r) * 8);
    // Phase B, k = ks * 16 + h * 8 + j -> kernel row k / 9, element k % 9 of the pixel's 9.  With dword d of row kh = elements 2d, 2d+1:
    //   lower half-wave: A = row0 d0 d1, B = row0 d2 d3, C = row1 d3 d4, E = row2 d0 d1, D = row2 d2
    //   upper half-wave: A = row1 d0 d1, B = row1 d2 d3, C = row2 d3 d4, E = row0 d0 d1, D = row0 d4
    // B and C sit at the same distance from A in both halves; E0's low half is element 0 of row 0, which the padding k re-read.
    Stem12Words d;
    const int wave_s = __builtin_amdgcn_readfirstlane(wave);
    int t = blockIdx.x;
    Stem12Tile c = stem12_tile(p, t, tiles_x, tiles_per_img);
    int a_cur = c.a;
    stem12_describe(d, c.a, 3 * p.W, wave_s);
    uint32_t word[W_RUN];
    stem12_request(word, d, p, c);
    stem12_convert(smem, word, d, p, c);                       // A of the first tile; A of every later one runs behind conv2 of its predecessor

    for (;;) {
        __syncthreads();                                       // the halo is complete (and conv2 of the previous tile has read the t1 tile)

        // ---- B: conv1 (3 -> 32, stride 2) for the 340 pixels of the t1 tile ----
        {
            const int y1_0 = c.tile_y * TH - 1, x1_0 = c.tile_x * TW - 1;   // conv1-output coordinates of the t1 tile's first pixel
            float4 b1[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) b1[g] = *reinterpret_cast<const float4*>(sbias + 8 * g + 4 * h);
            // selectors and addresses are formed here, per tile (a few instructions): held across the tile loop they spill
            int hb = h;
            asm volatile("" : "+v"(hb));
            bf16x8_t a1[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) a1[ks] = *reinterpret_cast<const bf16x8_t*>(smem + W_A1 + ((ks * 2 + hb) * 32 + r) * 16);
            const uint32_t sel_a = hb ? stem12_sel(SEL_YL, SEL_XL) : stem12_sel(SEL_XL, SEL_XH);
            const uint32_t sel_b = hb ? stem12_sel(SEL_XH, SEL_YL) : stem12_sel(SEL_YL, SEL_YH);
            const uint32_t sel_c = hb ? stem12_sel(SEL_XL, SEL_XH) : stem12_sel(SEL_XH, SEL_YL);
            const uint32_t sel_d = hb ? stem12_sel(SEL_XL, SEL_XL) : stem12_sel(SEL_YL, SEL_YH);
            const uint32_t sel_e = hb ? stem12_sel(SEL_YL, SEL_YL) : stem12_sel(SEL_XL, SEL_XH);
            const int offE = hb ? -W_ROWB : 2 * W_ROWB, offD = offE + (hb ? 16 : 8);
            // a t1 tile that lies inside the half-resolution map (all but the tiles on its border) needs no mask on its values
            const bool inside = y1_0 >= 0 && y1_0 + F_T1H <= p.Ho && x1_0 >= 0 && x1_0 + F_T1W <= p.Wo;
            auto column_tiles = [&](auto masked_t) {
            constexpr bool MASKED = decltype(masked_t)::value;
#pragma unroll
            for (int it = 0; it < 3; ++it) {
                if ((wave + 4 * it) * 32 >= F_T1PX) break;
                int rb = r;
                asm volatile("" : "+v"(rb));
                const int pidx = (wave + 4 * it) * 32 + rb;
                const int pcl = min(pidx, F_T1PX - 1), py = pcl / F_T1W, px = pcl - py * F_T1W;
                const int oA = (2 * py + hb) * W_ROWB + W_LEAD * 2 + 12 * px, oE = oA + offE, oD = oA + offD;
                const uint32_t A0 = lds_u32(smem, oA), A1 = lds_u32(smem, oA + 4), B0 = lds_u32(smem, oA + 8), B1 = lds_u32(smem, oA + 12);
                const uint32_t C0 = lds_u32(smem, oA + W_ROWB + 12), C1 = lds_u32(smem, oA + W_ROWB + 16);
                const uint32_t E0 = lds_u32(smem, oE), E1 = lds_u32(smem, oE + 4), D = lds_u32(smem, oD);
                union { bf16x8_t v; uint32_t u[4]; } k0, k1;
                k0.u[0] = __builtin_amdgcn_perm(A0, D, sel_a);
                k0.u[1] = __builtin_amdgcn_perm(A0, A1, sel_b);
                k0.u[2] = __builtin_amdgcn_perm(A1, B0, sel_b);
                k0.u[3] = __builtin_amdgcn_perm(B0, B1, sel_b);
                k1.u[0] = __builtin_amdgcn_perm(C0, C1, sel_c);
                k1.u[1] = __builtin_amdgcn_perm(E0, C1, sel_a);
                k1.u[2] = __builtin_amdgcn_perm(E0, E1, sel_d);
                k1.u[3] = __builtin_amdgcn_perm(D, E0, sel_e);
                f32x16_t acc;
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[j] = 0.f;
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[0], k0.v, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[1], k1.v, acc, 0, 0, 0);
                const int y1 = y1_0 + py, x1 = x1_0 + px;
                const uint32_t keep = (!MASKED || (y1 >= 0 && y1 < p.Ho && x1 >= 0 && x1 < p.Wo)) ? 0xffffffffu : 0u;   // outside: conv2's zero padding
                if (pidx < F_T1PX) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        uint2 o;
                        o.x = stem12_bias_relu_pack(acc[4 * g + 0], acc[4 * g + 1], b1[g].x, b1[g].y) & keep;   // ReLU (checked at launch)
                        o.y = stem12_bias_relu_pack(acc[4 * g + 2], acc[4 * g + 3], b1[g].z, b1[g].w) & keep;
                        *reinterpret_cast<uint2*>(t1 + pidx * T1_PITCH + g * 16 + 8 * h) = o;
                    }
                }
            }
            };
            if (inside) column_tiles(std::false_type{}); else column_tiles(std::true_type{});
        }
        __syncthreads();

        // ---- the next tile's words: in flight under conv2 ----
        const int tn = t + (int)gridDim.x;
        const bool more = tn < tiles;
        Stem12Tile cn = c;
        if (more) {
            cn = stem12_tile(p, tn, tiles_x, tiles_per_img);
            if (cn.a != a_cur) { stem12_describe(d, cn.a, 3 * p.W, wave_s); a_cur = cn.a; }   // another image, its base aligned differently
            stem12_request(word, d, p, cn);
        }

        // ---- C: conv2 (32 -> 32), chunk (16 channels) outer, tap inner: the stand-alone kernel's summation order ----
        f32x16_t acc2[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int j = 0; j < 16; ++j) acc2[mt][j] = 0.f;
        const unsigned char* t1r = t1 + (wave * 2 * F_T1W + r) * T1_PITCH + h * 16;   // every fragment at a constant distance from here
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
#pragma unroll
            for (int row = 0; row < 4; ++row) {                // t1 row wave * 2 + row: tap row `row` of output row 0, `row - 1` of output row 1
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const bf16x8_t bf = *reinterpret_cast<const bf16x8_t*>(t1r + (row * F_T1W + dx) * T1_PITCH + kc * 32);
                    if (row <= 2) acc2[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2[kc][row * 3 + dx], bf, acc2[0], 0, 0, 0);
                    if (row >= 1) acc2[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2[kc][(row - 1) * 3 + dx], bf, acc2[1], 0, 0, 0);
                }
            }
        }

        // ---- A of the next tile: input region -> normalised bf16 halo (its readers passed the barrier above).  Here, before this
        // tile's stores are issued: the wait for the words is then not a wait for those stores (vector-memory operations retire in
        // issue order), and the stores drain under phase B of the next tile ----
        if (more) stem12_convert(smem, word, d, p, cn);

        // ---- epilogue in registers: bias + ReLU -> bf16; v_permlane32_swap trades quad g of the upper half-wave for quad g + 1 of the
        // lower one, so every lane owns 8 consecutive channels of its pixel: direct 16-byte stores ----
        {
            float4 b2[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) b2[g] = *reinterpret_cast<const float4*>(sbias + 32 + 8 * g + 4 * h);
            const int ox = c.tile_x * TW + r;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const int oy = c.tile_y * TH + wave * 2 + mt;
                uint4 pk[2];
#pragma unroll
                for (int gp = 0; gp < 2; ++gp) {
                    uint32_t qx[2], qy[2];
#pragma unroll
                    for (int gq = 0; gq < 2; ++gq) {
                        const int g = 2 * gp + gq;
                        qx[gq] = stem12_bias_relu_pack(acc2[mt][4 * g + 0], acc2[mt][4 * g + 1], b2[g].x, b2[g].y);
                        qy[gq] = stem12_bias_relu_pack(acc2[mt][4 * g + 2], acc2[mt][4 * g + 3], b2[g].z, b2[g].w);
                    }
                    const auto sx2 = __builtin_amdgcn_permlane32_swap(qx[0], qx[1], false, false);
                    const auto sy2 = __builtin_amdgcn_permlane32_swap(qy[0], qy[1], false, false);
                    pk[gp] = make_uint4(sx2[0], sy2[0], sx2[1], sy2[1]);
                }
                if (oy < p.Ho && ox < p.Wo) {
                    bf16_t* ypix = p.y + (((size_t)c.n_img * p.Ho + oy) * p.Wo + ox) * 32 + 8 * h;
                    *reinterpret_cast<uint4*>(ypix) = pk[0];
                    *reinterpret_cast<uint4*>(ypix + 16) = pk[1];
                }
            }
        }
        if (!more) break;
        c = cn; t = tn;
    }
}

// standalone normalise: u8 [N,H,W,3] -> bf16 [N,Hp,Wp,4]-free NHWC(3) or NCHW, zero outside (vh, vw)
__global__ void normalize_kernel(const uint8_t* x, bf16_t* y, int N, int H, int W, int Hp, int Wp, int vh, int vw,
                                 float s0, float s1, float s2, float b0, float b1, float b2, int nchw) {
    const size_t total = (size_t)N * Hp * Wp;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int xx = (int)(i % Wp);
        const size_t t = i / Wp;
        const int yy = (int)(t % Hp), n = (int)(t / Hp);
        float v[3] = {0.f, 0.f, 0.f};
        if (yy < vh && xx < vw) {
            const uint8_t* s = x + (((size_t)n * H + yy) * W + xx) * 3;
            v[0] = (float)s[0] * s0; v[0] = v[0] + b0;
            v[1] = (float)s[1] * s1; v[1] = v[1] + b1;
            v[2] = (float)s[2] * s2; v[2] = v[2] + b2;
        }
        if (nchw) {
            const size_t plane = (size_t)Hp * Wp;
            bf16_t* d = y + (size_t)n * 3 * plane + (size_t)yy * Wp + xx;
            d[0] = f32_to_bf16(v[0]); d[plane] = f32_to_bf16(v[1]); d[2 * plane] = f32_to_bf16(v[2]);
        } else {
            bf16_t* d = y + i * 3;
            d[0] = f32_to_bf16(v[0]); d[1] = f32_to_bf16(v[1]); d[2] = f32_to_bf16(v[2]);
        }
    }
}

}  // namespace

void pack_stem_weights(const bf16_t* ohwi, int cout, bf16_t* out /* [2][2][32][8] */) {
    for (int ks = 0; ks < 2; ++ks)
        for (int h = 0; h < 2; ++h)
            for (int co = 0; co < 32; ++co)
                for (int j = 0; j < 8; ++j) {
                    const int k = ks * 16 + h * 8 + j;  // k = (kh*3 + kw)*3 + c == OHWI inner order
                    out[((ks * 2 + h) * 32 + co) * 8 + j] = (co < cout && k < 27) ? ohwi[co * 27 + k] : (bf16_t)0;
                }
}

hipError_t stem_conv_launch(const StemParams& p, hipStream_t stream) {
    const int tiles_x = (p.Wo + TW - 1) / TW, tiles_y = (p.Ho + TH - 1) / TH;
    hipLaunchKernelGGL(stem_conv_kernel, dim3(p.N * tiles_x * tiles_y), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t stem12_launch(const StemParams& p, const bf16_t* w2pk, const float* bias2, hipStream_t stream) {
    if (p.valid_w_per_img != nullptr || p.Cout_store != 32 || p.act != ACT_RELU) return hipErrorInvalidValue;
    const int tiles_x = (p.Wo + TW - 1) / TW, tiles_y = (p.Ho + TH - 1) / TH, tiles = p.N * tiles_x * tiles_y;
    if (tiles <= 0) return hipErrorInvalidValue;
    // one work-group per slot that is resident at once; each loads the weights once and then walks its tiles
    int dev = 0, cus = 0;
    { hipError_t e = hipGetDevice(&dev); if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev); if (e != hipSuccess) return e; }
    const int grid = std::min(tiles, cus * STEM12_WGS_PER_CU);
    hipLaunchKernelGGL(stem12_kernel, dim3(grid), dim3(256), 0, stream, p, w2pk, bias2);
    return hipGetLastError();
}

hipError_t normalize_launch(const uint8_t* x, bf16_t* y, int N, int H, int W, int Hp, int Wp, int vh, int vw,
                            const float* scale, const float* shift, int nchw, hipStream_t stream) {
    const size_t total = (size_t)N * Hp * Wp;
    int grid = (int)((total + 255) / 256);
    if (grid > 256 * 16) grid = 256 * 16;
    hipLaunchKernelGGL(normalize_kernel, dim3(grid), dim3(256), 0, stream, x, y, N, H, W, Hp, Wp, vh, vw, scale[0], scale[1],
                       scale[2], shift[0], shift[1], shift[2], nchw);
    return hipGetLastError();
}
