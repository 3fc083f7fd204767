// QR codes (Model 2) on the GPU (gfx950): the symbols of a page as (x0, y0, x1, y1, version, level, mask, ndata, errors, rotation, format
// distance, timing mismatches) with their corrected data codewords, in a canonical order.  Everything is integer and every reduction is
// order-free (min / max / add / xor, ballots), so the lists equal the sequential definitions restated in tests/qr_reference.py (versions
// 1-10, lumina_ocr_qrcodes) and tests/qr_versions_reference.py (versions 1-40, lumina_ocr_qrcodes_versions).
//
// All stream-ordered kernels, no host round trip; both calls enqueue 1-5 through one front end:
//   1-3 components_launch (runs.h)      the mask (or the one the caller already has), its run list, the 8-connected components; every run
//                 learns its root, box and area are accumulated at the root
//   4 qr_finders  one wave per row, lanes over the row's roots: a solid square core whose centre row has, before and after the core's run,
//                 two runs of one other component, the ring, concentric and 7/3 of its size -> counted, gathered per page
//   5 qr_decode   stage 1, versions 1-10.  One wave per (page, finder A): lanes over B, a loop over C pick A's partners (64-bit products, no
//                 division, no root), the nearest valid pairs in turn until one decodes.  Per version in reach lane r samples module row r
//                 on the affine grid as one 64-bit word and the timing patterns are counted; the codewords are gathered through the
//                 placement table from the rows in LDS
//  5b qr_decode_versions   stage 2, versions 11 .. max_version (the all-versions call only), for the finders stage 1 gave no symbol.  The
//                 versions in reach are scored on their timing patterns alone (lanes over the pattern's modules), the best one's version
//                 information must agree, then the grid (up to 177 x 177, three words a row) is sampled with lanes over columns and a loop
//                 over rows: the numerators advance by a constant from row to row, so one division at the top and an add-and-carry per
//                 row give the floor division exactly, and a ballot is the row's word.  The function mask is built in LDS from the
//                 alignment centres and the fixed areas (lanes over rows); the codewords are placed without a table: lanes over the
//                 two-column strips count their free modules, a wave prefix sum gives each strip its bit offset, and each lane walks its
//                 strip and ORs whole and partial bytes into the codewords (LDS atomics)
//   6 qr_output   one work-group per page (code_output.h): valid candidates counted, gathered, rank-sorted by (y0, x0, y1, x1, corner root);
//                 int rows of stage 1's codewords, or (the all-versions call) byte rows from the stage that read the symbol
// The stages differ in how a version is scored, how the grid is sampled and how the codewords are placed; the pair search, the quiet
// rings, the format information, the block loop (rs.h: field 0x11D, first root 0) and the result are one piece of code each.  Every
// loop has a constant bound, every table and LDS index is clamped, and no wave waits for another (a work-group is one wave).
#include "qrcodes.h"
#include "code_output.h"
#include "qr_tables.h"
#include "qr_version_tables.h"
#include "rs.h"
#include "runs.h"

namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int QR_SPAN = 8192;          // |B - A|, |C - A| per axis in doubled pixels: keeps every product inside 64 bits
// a candidate's result (code_output.h): y0, x0, y1, x1, root, version, level, mask, ndata, errors, rotation, fdist, timing, state
constexpr int QR_MAX_TOTAL = 346, QR_MAX_NB = 8, QR_RAW = 384;   // stage 1: the codewords and blocks of version 10, its LDS array
constexpr int QRV_ROWS = 177;          // stage 2: modules a side at version 40
constexpr int QRV_RAW = 3712;          // >= QRV_MAX_TOTAL, a multiple of 4
constexpr int QR_RS_LEN = 192, QR_RS_EC = 30;   // both stages: the longest block (153 at version 40, 146 up to version 10) and its EC codewords
constexpr int BIG = 0x7fffffff;
constexpr int QR_PAIR_TRIES = 8;      // of a corner's valid partner pairs, the nearest ones are tried in turn
static_assert(QRV_MAX_BLOCK <= QR_RS_LEN && QRV_MAX_TOTAL <= QRV_RAW && QRV_VERSIONS == 40 && QR_MAX_TOTAL <= QR_RAW, "qr_version_tables.h");

__device__ __forceinline__ i64 labs64(i64 v) { return v < 0 ? -v : v; }
__device__ __forceinline__ i64 floor_div(i64 a, i64 b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }   // b > 0
__device__ __forceinline__ int floor_div32(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }   // b > 0

// 4: finders [B][max_finders] = cx2, cy2, me, root
__global__ __launch_bounds__(256) void qr_finders_kernel(const int* runoff, const unsigned short* rxs, const unsigned short* rxe, const int* parent,
                                                         const int4* box, const int* area, int H, size_t runcap, int min_module, int max_module, int centre_tol,
                                                         int ring_tol, int max_finders, int* nfind, int4* finders, int rows_total) {
    int pg, row, lane;
    if (!row_wave(H, rows_total, pg, row, lane)) return;
    const int* ro = runoff + (size_t)pg * (H + 1);
    const size_t rb = (size_t)pg * runcap;
    const int* P = parent + rb;
    const unsigned short* xs = rxs + rb;
    const unsigned short* xe = rxe + rb;
    for (int id = ro[row] + lane; id < ro[row + 1]; id += 64) {
        if (P[id] != id) continue;
        const int4 bx = box[rb + id];   // x0, x1, y0, y1
        const int w = bx.y - bx.x + 1, h = bx.w - bx.z + 1, mn = w < h ? w : h;
        if (w < 3 * min_module || h < 3 * min_module || w > 3 * max_module || h > 3 * max_module || 4 * iabs(w - h) > mn) continue;
        if (4 * (i64)area[rb + id] < 3 * (i64)w * h) continue;
        const int yc = clampi((bx.z + bx.w) >> 1, 0, H - 1), xc = (bx.x + bx.y) >> 1;
        const int r0 = ro[yc], r1 = ro[yc + 1];
        int lo = r0, hi = r1;   // the first run of the row that ends at or behind xc
        for (int it = 0; it < 17; ++it) {
            if (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((int)xe[mid] < xc) lo = mid + 1; else hi = mid;
            }
        }
        const int j = lo;
        if (j <= r0 || j + 1 >= r1 || (int)xs[j] > xc || P[j] != id) continue;
        const int q = P[j - 1];
        if (q != P[j + 1] || q == id) continue;
        const int4 rx = box[rb + q];
        const int rw = rx.y - rx.x + 1, rh = rx.w - rx.z + 1, me = rw + rh;
        if (112 * (i64)iabs((rx.x + rx.y) - (bx.x + bx.y)) > (i64)centre_tol * me || 112 * (i64)iabs((rx.z + rx.w) - (bx.z + bx.w)) > (i64)centre_tol * me) continue;
        if (224 * (i64)iabs(3 * rw - 7 * w) > 3 * (i64)ring_tol * me || 224 * (i64)iabs(3 * rh - 7 * h) > 3 * (i64)ring_tol * me) continue;
        const int idx = atomicAdd(&nfind[pg], 1);
        if (idx < max_finders) finders[(size_t)pg * max_finders + idx] = make_int4(rx.x + rx.y + 1, rx.z + rx.w + 1, me, id);
    }
}

// ---- what both stages share ------------------------------------------------------------------------------------------------------------------

struct QrGrid { int ax, ay, abx, aby, acx, acy, n; };

// module (col i, row j) of the grid: the ink at pixel (nx / 2n, ny / 2n); off the page reads clear
__device__ __forceinline__ int qr_sample(const u64* mpage, int H, int W, int nw, const QrGrid& g, int i, int j) {
    const int nx = g.ax * g.n + (i - 3) * g.abx + (j - 3) * g.acx, ny = g.ay * g.n + (i - 3) * g.aby + (j - 3) * g.acy;
    if (nx < 0 || ny < 0) return 0;
    const int px = nx / (2 * g.n), py = ny / (2 * g.n);
    if (px >= W || py >= H) return 0;
    return (int)((mpage[(size_t)py * nw + (px >> 6)] >> (px & 63)) & 1ull);
}

__device__ __forceinline__ bool qr_mask_bit(int mask, int y, int x) {
    switch (mask) {
        case 0: return (x + y) % 2 == 0;
        case 1: return y % 2 == 0;
        case 2: return x % 3 == 0;
        case 3: return (x + y) % 3 == 0;
        case 4: return (x / 3 + y / 2) % 2 == 0;
        case 5: return x * y % 2 + x * y % 3 == 0;
        case 6: return (x * y % 2 + x * y % 3) % 2 == 0;
        default: return ((x + y) % 2 + x * y % 3) % 2 == 0;
    }
}

// the partners of corner A = finder a of the nf in lanes (f = cx2, cy2, me, root): lane = B, a loop over C; the valid pairs with a version in
// reach, in the order of (|AB|^2 + |AC|^2, root of B, root of C), are handed to attempt(grid, versions in reach) in turn, the nearest
// QR_PAIR_TRIES of them, until one returns true.  reach(l2, m) -> the versions (bit v) that l2 = |AB|^2 + |AC|^2 (doubled pixels) and
// m = meA + meB + meC allow.  The whole wave calls it (attempt holds barriers).
template <class Reach, class Attempt>
__device__ __forceinline__ void qr_pairs(const int4 f, int nf, int a, int lane, Reach reach, Attempt attempt) {
    const int ax = __shfl(f.x, a), ay = __shfl(f.y, a), ma = __shfl(f.z, a);
    const bool b_ok = lane < nf && lane != a && iabs(f.x - ax) <= QR_SPAN && iabs(f.y - ay) <= QR_SPAN && 4 * iabs(ma - f.z) <= (ma < f.z ? ma : f.z);
    const int abx = b_ok ? f.x - ax : 0, aby = b_ok ? f.y - ay : 0;   // (zero where the products below could leave 64 bits)
    const i64 lab = (i64)abx * abx + (i64)aby * aby;
    int pl = -1, pb = -1, pc = -1;   // the key tried last
#pragma unroll 1
    for (int tries = 0; tries < QR_PAIR_TRIES; ++tries) {
        int best_l = BIG, best_idc = BIG, best_c = 0;
#pragma unroll 1
        for (int c = 0; c < QR_MAX_FINDERS; ++c) {
            if (c >= nf) break;
            const int cx = __shfl(f.x, c), cy = __shfl(f.y, c), mc = __shfl(f.z, c), idc = __shfl(f.w, c);
            bool ok = b_ok && c != a && c != lane && iabs(cx - ax) <= QR_SPAN && iabs(cy - ay) <= QR_SPAN && 4 * iabs(ma - mc) <= (ma < mc ? ma : mc);
            const int acx = ok ? cx - ax : 0, acy = ok ? cy - ay : 0;
            const i64 lac = (i64)acx * acx + (i64)acy * acy, dot = (i64)abx * acx + (i64)aby * acy, cross = (i64)abx * acy - (i64)aby * acx;
            ok = ok && 4 * labs64(lab - lac) <= (lab < lac ? lab : lac) && 64 * dot * dot <= lab * lac && cross > 0;
            const int l = ok ? (int)(lab + lac) : BIG;   // (< 2^29)
            ok = ok && (l > pl || (l == pl && (f.w > pb || (f.w == pb && idc > pc))));   // behind the key tried last
            ok = ok && (l < best_l || (l == best_l && idc < best_idc));
            if (ok && reach(lab + lac, (i64)ma + f.z + mc) != 0ull) { best_l = l; best_idc = idc; best_c = c; }
        }
        const int min_l = wave_min(best_l);
        if (min_l == BIG) return;
        const int min_b = wave_min(best_l == min_l ? f.w : BIG);
        const u64 win = __ballot(best_l == min_l && f.w == min_b);   // roots are distinct: one lane
        if (!win) return;
        const int b = __ffsll((long long)win) - 1, c = __shfl(best_c, b) & 63;
        pl = min_l; pb = min_b; pc = __shfl(best_idc, b);
        QrGrid g;
        g.ax = ax; g.ay = ay; g.n = 1;   // (n: the modules between finder centres, set per version)
        g.abx = __shfl(f.x, b) - ax; g.aby = __shfl(f.y, b) - ay; g.acx = __shfl(f.x, c) - ax; g.acy = __shfl(f.y, c) - ay;
        if (attempt(g, reach((i64)min_l, (i64)ma + __shfl(f.z, b) + __shfl(f.z, c)))) return;
        __syncthreads();
    }
}

// the quiet rings of a D-module symbol, lanes over the SPAN >= D + 2 QR_MAX_QUIET positions of a side -> true when one holds ink
template <int SPAN>
__device__ __forceinline__ bool qr_quiet_dirty(const u64* mpage, int H, int W, int nw, const QrGrid& g, int D, int quiet, int lane) {
    bool dirty = false;
    for (int k = 1; k <= QR_MAX_QUIET; ++k) {
        if (k > quiet) break;
#pragma unroll 1
        for (int t0 = 0; t0 < SPAN; t0 += 64) {
            const int t = t0 + lane - k;
            if (t < D + k)
                dirty = dirty || qr_sample(mpage, H, W, nw, g, t, -k) || qr_sample(mpage, H, W, nw, g, t, D - 1 + k) || qr_sample(mpage, H, W, nw, g, -k, t) ||
                        qr_sample(mpage, H, W, nw, g, D - 1 + k, t);
        }
    }
    return __ballot(dirty) != 0ull;
}

// format information through bit(row, col): lane i < 15 reads bit i of both copies, lanes < 32 measure a word each -> false when neither
// copy is within distance 3 of a word
template <class Bit>
__device__ __forceinline__ bool qr_format(Bit bit, int D, int lane, int& level, int& mpat, int& fdist) {
    int b1 = 0, b2 = 0;
    if (lane < 15) {
        const int r1 = lane < 6 ? lane : (lane == 6 ? 7 : 8), c1 = lane < 8 ? 8 : (lane == 8 ? 7 : 14 - lane);
        const int r2 = lane < 8 ? 8 : D - 15 + lane, c2 = lane < 8 ? D - 1 - lane : 8;
        b1 = bit(r1, c1);
        b2 = bit(r2, c2);
    }
    const int f1 = (int)(__ballot(b1) & 0x7fffull), f2 = (int)(__ballot(b2) & 0x7fffull);
    const int fw = QRV_FORMAT[lane & 31];
    const int k1 = wave_min(lane < 32 ? (__popc(f1 ^ fw) << 5) | lane : BIG), k2 = wave_min(lane < 32 ? (__popc(f2 ^ fw) << 5) | lane : BIG);
    int word;
    if ((k1 >> 5) <= 3) { word = k1 & 31; fdist = k1 >> 5; }
    else if ((k2 >> 5) <= 3) { word = k2 & 31; fdist = (k2 >> 5) + 16; }
    else return false;
    level = (word >> 3) ^ 1; mpat = word & 7;
    return true;
}

// the blocks of a symbol: its `total` codewords in placement order (raw, RAW_CAP of them) de-interleaved block by block into rs.blk,
// corrected there, the data codewords written to od (DATA_CAP of them) -> false when a block has more errors than it can correct.  A
// symbol's total % blocks last blocks hold one data codeword more.  The whole wave calls it (barriers inside).
template <int MAX_NB, int RAW_CAP, int DATA_CAP, int MAX_LEN, int MAX_EC>
__device__ __forceinline__ bool qr_blocks(RsLds<unsigned char, MAX_LEN, MAX_EC, 8>& rs, const unsigned char* raw, int total, int version, int level, int lane,
                                          unsigned char* od, int& ndata, int& errors) {
    const int bi = (version - 1) * 4 + (level & 3);
    const int nb = clampi(QRV_NB[bi], 1, MAX_NB), ec = clampi(QRV_EC[bi], 2, MAX_EC);
    const int nshort = nb - total % nb, dlen = total / nb - ec;
    ndata = total - nb * ec;
    errors = 0;
    if (dlen < 1 || dlen + 1 + ec > MAX_LEN || ndata < 1 || ndata > DATA_CAP || total > RAW_CAP) return false;   // (the tables never say so)
    int dpos = 0;
#pragma unroll 1
    for (int blk = 0; blk < MAX_NB; ++blk) {
        if (blk >= nb) break;
        const int nd = dlen + (blk >= nshort ? 1 : 0), len = nd + ec;
#pragma unroll
        for (int p0 = 0; p0 < MAX_LEN; p0 += 64) {
            const int p = p0 + lane;
            if (p < len) {
                const int src = p < dlen ? p * nb + blk : (p < nd ? dlen * nb + blk - nshort : ndata + (p - nd) * nb + blk);
                rs.blk[p] = raw[clampi(src, 0, RAW_CAP - 1)];
            }
        }
        __syncthreads();
        const int e = rs_correct_block(rs, len, ec, 0, lane);
        if (e < 0) return false;
        errors += e;
#pragma unroll
        for (int p0 = 0; p0 < MAX_LEN; p0 += 64) {
            const int p = p0 + lane;
            if (p < nd && dpos + p < DATA_CAP) od[dpos + p] = rs.blk[p];
        }
        dpos += nd;
        __syncthreads();
    }
    return true;
}

// a decoded symbol's result (one lane): the hull, which is the four outer module corners, (u, v) = 2 (i, j) - 6 in {-7, 2 n + 7}, and the
// 14 ints behind it
__device__ __forceinline__ void qr_write_result(int* o, const QrGrid& g, int H, int W, int ida, int version, int level, int mpat, int ndata, int errors, int fdist,
                                                int timing) {
    const int n = g.n;
    i64 x0 = 0, x1 = 0, y0 = 0, y1 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int u = (k & 1) ? 2 * n + 7 : -7, v = (k & 2) ? 2 * n + 7 : -7;
        const i64 qx = floor_div((i64)g.ax * 2 * n + (i64)u * g.abx + (i64)v * g.acx, 4 * n);
        const i64 qy = floor_div((i64)g.ay * 2 * n + (i64)u * g.aby + (i64)v * g.acy, 4 * n);
        x0 = k == 0 || qx < x0 ? qx : x0; x1 = k == 0 || qx > x1 ? qx : x1;
        y0 = k == 0 || qy < y0 ? qy : y0; y1 = k == 0 || qy > y1 ? qy : y1;
    }
    const auto cl = [](i64 v, int hi) { return (int)(v < 0 ? 0 : (v > hi ? hi : v)); };
    o[0] = cl(y0, H - 1); o[1] = cl(x0, W - 1); o[2] = cl(y1 - 1, H - 1); o[3] = cl(x1 - 1, W - 1); o[4] = ida;
    o[5] = version; o[6] = level; o[7] = mpat; o[8] = ndata; o[9] = errors;
    o[10] = iabs(g.abx) >= iabs(g.aby) ? (g.abx > 0 ? 0 : 2) : (g.aby > 0 ? 1 : 3);
    o[11] = fdist; o[12] = timing; o[CODE_RES_STATE] = CODE_ROW;
}

// ---- stage 1: versions 1-10 ----------------------------------------------------------------------------------------------------------------

// the versions (bit v) whose n = 10 + 4 v modules between finder centres lie within three modules of what l2 and m say
__device__ __forceinline__ u64 reach_mask(i64 l2, i64 m) {
    unsigned out = 0;
    const i64 t = 882 * l2;
#pragma unroll
    for (int v = 1; v <= QR_VERSIONS; ++v) {
        const i64 lo = 2 * (7 + 4 * v) * m, hi = 2 * (13 + 4 * v) * m;
        if (lo * lo <= t && t <= hi * hi) out |= 1u << v;
    }
    return out;
}

struct QrLds {
    u64 rows[64];              // module rows: bit col
    unsigned char raw[QR_RAW];   // the codewords in placement order
    RsLds<unsigned char, QR_RS_LEN, QR_RS_EC, 8> rs;
};

// a candidate (the corner A of g with its partners) through the whole decode -> true with the result in o / od, false when it is none.
// The whole wave calls it (barriers inside) and returns one answer.
__device__ __forceinline__ bool qr_try(QrLds& s, const u64* mpage, int H, int W, int nw, QrGrid g, u64 reach, int quiet, int timing_max, int ida, int lane,
                                       int* o, unsigned char* od) {
    // the version: fewest timing mismatches, the smaller on a tie
    int timing = BIG, version = 0;
    u64 row = 0;
    for (int v = 1; v <= QR_VERSIONS; ++v) {
        if (!((reach >> v) & 1ull)) continue;
        const int D = 17 + 4 * v;
        g.n = D - 7;
        u64 r = 0;
        if (lane < D)
            for (int i = 0; i < 57; ++i)
                if (i < D) r |= (u64)qr_sample(mpage, H, W, nw, g, i, lane) << i;
        __syncthreads();
        s.rows[lane] = r;
        __syncthreads();
        const u64 span = ((1ull << (D - 16)) - 1ull) << 8;   // columns 8 .. D - 9
        const int t = __popcll((s.rows[6] ^ 0x5555555555555555ull) & span) +
                      __popcll(__ballot(lane >= 8 && lane <= D - 9 && (int)((r >> 6) & 1ull) != ((lane & 1) ^ 1)));
        if (t < timing) { timing = t; version = v; row = r; }
    }
    if (version == 0 || timing > timing_max) return false;
    const int D = 17 + 4 * version;
    g.n = D - 7;
    __syncthreads();
    s.rows[lane] = row;
    const bool dirty = qr_quiet_dirty<128>(mpage, H, W, nw, g, D, quiet, lane);
    __syncthreads();
    if (dirty) return false;
    int level, mpat, fdist;
    if (!qr_format([&](int r, int c) { return (int)((s.rows[r & 63] >> (c & 63)) & 1ull); }, D, lane, level, mpat, fdist)) return false;
    // unmask the data modules
    if (lane < D) {
        u64 m = 0;
        for (int x = 0; x < 57; ++x)
            if (x < D && qr_mask_bit(mpat, lane, x)) m |= 1ull << x;
        s.rows[lane] = row ^ (m & ~QR_FUNC[(version - 1) * 64 + lane]);
    }
    __syncthreads();
    // codewords in placement order
    const int total = clampi(QRV_TOTAL[version - 1], 1, QR_MAX_TOTAL), poff = QR_PLACE_OFF[version - 1];
#pragma unroll 1
    for (int k = lane; k < QR_RAW; k += 64) {
        int val = 0;
        if (k < total) {
            for (int bit = 0; bit < 8; ++bit) {
                const int at = poff + 8 * k + bit;
                const unsigned p = QR_PLACE[at < QR_PLACE_N ? at : QR_PLACE_N - 1];
                val = (val << 1) | (int)((s.rows[(p >> 6) & 63] >> (p & 63)) & 1ull);
            }
        }
        s.raw[k] = (unsigned char)val;
    }
    __syncthreads();
    int ndata, errors;
    if (!qr_blocks<QR_MAX_NB, QR_RAW, QR_MAX_DATA>(s.rs, s.raw, total, version, level, lane, od, ndata, errors)) return false;
    if (lane == 0) qr_write_result(o, g, H, W, ida, version, level, mpat, ndata, errors, fdist, timing);
    return true;
}

// 5: one wave per (page, finder): res [B][max_finders][CODE_RES_INTS], resdata [B][max_finders][QR_MAX_DATA]
__global__ __launch_bounds__(64) void qr_decode_kernel(const u64* mask, const int4* finders, const int* nfind, int H, int W, int nw, int max_finders, int quiet,
                                                       int timing_max, int* res, unsigned char* resdata) {
    __shared__ QrLds s;
    const int pg = blockIdx.y, a = blockIdx.x, lane = threadIdx.x;
    const int nf = nfind[pg];
    if (nf > max_finders || a >= nf || nf > QR_MAX_FINDERS) return;
    const u64* mpage = mask + (size_t)pg * H * nw;
    const int4 f = lane < nf ? finders[(size_t)pg * max_finders + lane] : make_int4(0, 0, 0, 0);
    const int ida = __shfl(f.w, a);
    int* o = res + ((size_t)pg * max_finders + a) * CODE_RES_INTS;
    unsigned char* od = resdata + ((size_t)pg * max_finders + a) * QR_MAX_DATA;
    rs_load_tables(s.rs, QR_EXP, QR_LOG, 8, lane);
    qr_pairs(f, nf, a, lane, [](i64 l2, i64 m) { return reach_mask(l2, m); }, [&](const QrGrid& g, u64 reach) { return qr_try(s, mpage, H, W, nw, g, reach, quiet, timing_max, ida, lane, o, od); });
}

// ---- stage 2: versions 11-40 ---------------------------------------------------------------------------------------------------------------

struct QrvLds {
    u64 grid[QRV_ROWS * 3], func[QRV_ROWS * 3];   // module rows and the function mask: bit col % 64 of word col / 64
    unsigned raw[QRV_RAW / 4];                    // the codewords in placement order, as bytes
    RsLds<unsigned char, QR_RS_LEN, QR_RS_EC, 8> rs;
};

// the versions 11 .. max_version (bit v) in reach of l2 = |AB|^2 + |AC|^2 and m = meA + meB + meC: n within 3 + n / 16 modules
__device__ __forceinline__ u64 reach_mask_versions(i64 l2, i64 m, int max_version) {
    u64 out = 0;
    const i64 t = 882 * l2;
#pragma unroll 1
    for (int v = 11; v <= QRV_VERSIONS; ++v) {
        if (v > max_version) break;
        const int n = 10 + 4 * v, w = 3 + n / 16;
        const i64 lo = 2 * (n - w) * m, hi = 2 * (n + w) * m;
        if (lo * lo <= t && t <= hi * hi) out |= 1ull << v;
    }
    return out;
}

// bit (row, col) of a 177 x 3 word array; both clamped
__device__ __forceinline__ int qrv_bit(const u64* rows, int row, int col) {
    const int r = clampi(row, 0, QRV_ROWS - 1), c = clampi(col, 0, QRV_ROWS - 1);
    return (int)((rows[r * 3 + (c >> 6)] >> (c & 63)) & 1ull);
}

// columns lo .. hi (inclusive, clipped) set in a row of three words
__device__ __forceinline__ void qrv_set(u64 (&w)[3], int lo, int hi) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int a = lo - 64 * k < 0 ? 0 : lo - 64 * k, b = hi - 64 * k > 63 ? 63 : hi - 64 * k;
        if (a <= b) w[k] |= (b - a == 63 ? ~0ull : ((1ull << (b - a + 1)) - 1ull)) << a;
    }
}

__device__ __forceinline__ int wave_excl_scan(int v, int lane, int& total) {
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    total = __shfl(inc, 63);
    return inc - v;
}

// strip s of a D-module symbol: its right column, and whether it runs upwards
__device__ __forceinline__ int qrv_strip_right(int s, int D) {
    const int wide = (D - 7) / 2;
    return s < wide ? D - 1 - 2 * s : 5 - 2 * (s - wide);
}

// a lane's strip walked in placement order from bit offset pos: the unmasked bits ORed into s.raw
__device__ __forceinline__ void qrv_walk(QrvLds& s, int strip, int D, int mpat, int total, int pos) {
    const int right = qrv_strip_right(strip, D);
    const bool up = (strip & 1) == 0;
    int cur = -1, acc = 0;
#pragma unroll 1
    for (int k = 0; k < QRV_ROWS; ++k) {
        if (k >= D) break;
        const int row = up ? D - 1 - k : k;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const int col = right - cc;
            if (qrv_bit(s.func, row, col)) continue;
            const int byte = pos >> 3;
            if (byte != cur) {
                if (cur >= 0 && cur < total && acc) atomicOr(&s.raw[cur >> 2], (unsigned)acc << ((cur & 3) * 8));
                cur = byte; acc = 0;
            }
            acc |= (qrv_bit(s.grid, row, col) ^ (qr_mask_bit(mpat, row, col) ? 1 : 0)) << (7 - (pos & 7));
            ++pos;
        }
    }
    if (cur >= 0 && cur < total && acc) atomicOr(&s.raw[cur >> 2], (unsigned)acc << ((cur & 3) * 8));
}

// a candidate through stage 2's decode -> true with the result in o / od.  The whole wave calls it (barriers inside) and returns one answer.
__device__ __forceinline__ bool qr_try_versions(QrvLds& s, const u64* mpage, int H, int W, int nw, QrGrid g, u64 reach, int quiet, int timing_max, int ida,
                                                int lane, int* o, unsigned char* od) {
    // the version: fewest timing mismatches, the smaller on a tie
    int timing = BIG, version = 0;
#pragma unroll 1
    for (int v = 11; v <= QRV_VERSIONS; ++v) {
        if (!((reach >> v) & 1ull)) continue;
        const int Dv = 17 + 4 * v;
        g.n = Dv - 7;
        int t = 0;
#pragma unroll 1
        for (int k0 = 0; k0 < 192; k0 += 64) {
            const int k = k0 + lane, want = (k & 1) ^ 1;
            const bool in = k >= 8 && k <= Dv - 9;
            const bool m1 = in && qr_sample(mpage, H, W, nw, g, k, 6) != want, m2 = in && qr_sample(mpage, H, W, nw, g, 6, k) != want;
            t += __popcll(__ballot(m1)) + __popcll(__ballot(m2));
        }
        if (t < timing) { timing = t; version = v; }
    }
    if (version == 0) return false;
    const int D = 17 + 4 * version;
    g.n = D - 7;
    if (timing > timing_max * D / 57) return false;
    // the version information: the top-right copy, otherwise the bottom-left one, within distance 3
    {
        const int a = lane / 3, b = D - 11 + lane % 3;
        const bool v1 = lane < 18 && qr_sample(mpage, H, W, nw, g, b, a), v2 = lane < 18 && qr_sample(mpage, H, W, nw, g, a, b);
        const unsigned w1 = (unsigned)(__ballot(v1) & 0x3ffffull), w2 = (unsigned)(__ballot(v2) & 0x3ffffull);
        const unsigned want = QRV_VERSION_WORD[clampi(version - 7, 0, QRV_VERSIONS - 7)];
        if (__popc(w1 ^ want) > 3 && __popc(w2 ^ want) > 3) return false;
    }
    __syncthreads();
    // the grid: lane = column (three a lane), a loop over rows; q = floor(numerator / 2n) and the remainder advance by AC's
    {
        const int den = 2 * g.n;
        const int sqx = floor_div32(g.acx, den), srx = g.acx - sqx * den, sqy = floor_div32(g.acy, den), sry = g.acy - sqy * den;
        int qx[3], rx[3], qy[3], ry[3];
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const int i = 64 * w + lane;
            const int nx = g.ax * g.n + (i - 3) * g.abx - 3 * g.acx, ny = g.ay * g.n + (i - 3) * g.aby - 3 * g.acy;
            qx[w] = floor_div32(nx, den); rx[w] = nx - qx[w] * den;
            qy[w] = floor_div32(ny, den); ry[w] = ny - qy[w] * den;
        }
#pragma unroll 1
        for (int j = 0; j < QRV_ROWS; ++j) {
            if (j >= D) break;
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                const int px = qx[w], py = qy[w];
                bool bit = false;
                if (64 * w + lane < D && px >= 0 && py >= 0 && px < W && py < H) bit = (mpage[(size_t)py * nw + (px >> 6)] >> (px & 63)) & 1ull;
                const u64 word = __ballot(bit);
                if (lane == 0) s.grid[j * 3 + w] = word;
                qx[w] += sqx; rx[w] += srx;
                if (rx[w] >= den) { rx[w] -= den; ++qx[w]; }
                qy[w] += sqy; ry[w] += sry;
                if (ry[w] >= den) { ry[w] -= den; ++qy[w]; }
            }
        }
    }
    const bool dirty = qr_quiet_dirty<192>(mpage, H, W, nw, g, D, quiet, lane);
    __syncthreads();
    if (dirty) return false;
    int level, mpat, fdist;
    if (!qr_format([&](int r, int c) { return qrv_bit(s.grid, r, c); }, D, lane, level, mpat, fdist)) return false;
    // the function mask (lanes over rows) and cleared codewords
    {
        const unsigned char* ac = QRV_ALIGN + (version - 1) * QRV_MAX_ALIGN;
        const int cnt = clampi(version / 7 + 2, 2, QRV_MAX_ALIGN), last = ac[cnt - 1];
#pragma unroll 1
        for (int r0 = 0; r0 < 192; r0 += 64) {
            const int r = r0 + lane;
            if (r >= D) continue;
            u64 w[3] = {1ull << 6, 0, 0};                                     // column 6: timing
            if (r == 6) qrv_set(w, 0, D - 1);                                 // row 6: timing
            if (r <= 8) { qrv_set(w, 0, 8); qrv_set(w, D - 8, D - 1); }       // the two upper finders, separators, format
            if (r >= D - 8) qrv_set(w, 0, 8);                                 // the lower finder, format, the dark module
            if (r <= 5) qrv_set(w, D - 11, D - 9);                            // version information
            if (r >= D - 11 && r <= D - 9) qrv_set(w, 0, 5);
            for (int ia = 0; ia < QRV_MAX_ALIGN; ++ia) {
                if (ia >= cnt) break;
                const int ar = ac[ia];
                if (iabs(r - ar) > 2) continue;
                for (int ib = 0; ib < QRV_MAX_ALIGN; ++ib) {
                    if (ib >= cnt) break;
                    const int cc = ac[ib];
                    if ((ar == 6 && (cc == 6 || cc == last)) || (ar == last && cc == 6)) continue;
                    qrv_set(w, cc - 2, cc + 2);
                }
            }
            s.func[r * 3] = w[0]; s.func[r * 3 + 1] = w[1]; s.func[r * 3 + 2] = w[2];
        }
        for (int i = lane; i < QRV_RAW / 4; i += 64) s.raw[i] = 0u;
    }
    __syncthreads();
    // codewords in placement order: strips 64 r + lane
    const int total = clampi(QRV_TOTAL[version - 1], 1, QRV_MAX_TOTAL);
    {
        const int strips = (D - 7) / 2 + 3;   // <= 88
        int cnt[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int sidx = 64 * r + lane;
            cnt[r] = 0;
            if (sidx < strips) {
                const int right = qrv_strip_right(sidx, D);
#pragma unroll 1
                for (int k = 0; k < QRV_ROWS; ++k) {
                    if (k >= D) break;
                    cnt[r] += 2 - qrv_bit(s.func, k, right) - qrv_bit(s.func, k, right - 1);
                }
            }
        }
        int tot0, tot1;
        const int off0 = wave_excl_scan(cnt[0], lane, tot0), off1 = tot0 + wave_excl_scan(cnt[1], lane, tot1);
        if (lane < strips) qrv_walk(s, lane, D, mpat, total, off0);
        if (64 + lane < strips) qrv_walk(s, 64 + lane, D, mpat, total, off1);
    }
    __syncthreads();
    int ndata, errors;
    if (!qr_blocks<QRV_MAX_NB, QRV_RAW, QRV_MAX_DATA>(s.rs, reinterpret_cast<const unsigned char*>(s.raw), total, version, level, lane, od, ndata, errors))
        return false;
    if (lane == 0) qr_write_result(o, g, H, W, ida, version, level, mpat, ndata, errors, fdist, timing);
    return true;
}

// 5b: one wave per (page, finder) that stage 1 left without a symbol; res as stage 1's, resdata [B][max_finders][QRV_MAX_DATA]
__global__ __launch_bounds__(64) void qr_decode_versions_kernel(const u64* mask, const int4* finders, const int* nfind, int H, int W, int nw, int max_finders,
                                                                int quiet, int timing_max, int max_version, int* res, unsigned char* resdata) {
    __shared__ QrvLds s;
    const int pg = blockIdx.y, a = blockIdx.x, lane = threadIdx.x;
    const int nf = nfind[pg];
    if (nf > max_finders || a >= nf || nf > QR_MAX_FINDERS) return;
    int* o = res + ((size_t)pg * max_finders + a) * CODE_RES_INTS;
    if (o[CODE_RES_STATE] == CODE_ROW) return;   // stage 1 has A's symbol
    const u64* mpage = mask + (size_t)pg * H * nw;
    const int4 f = lane < nf ? finders[(size_t)pg * max_finders + lane] : make_int4(0, 0, 0, 0);
    const int ida = __shfl(f.w, a);
    unsigned char* od = resdata + ((size_t)pg * max_finders + a) * QRV_MAX_DATA;
    rs_load_tables(s.rs, QR_EXP, QR_LOG, 8, lane);
    qr_pairs(f, nf, a, lane, [=](i64 l2, i64 m) { return reach_mask_versions(l2, m, max_version); },
             [&](const QrGrid& g, u64 reach) { return qr_try_versions(s, mpage, H, W, nw, g, reach, quiet, timing_max, ida, lane, o, od); });
}

// ---- 6: the output ----------------------------------------------------------------------------------------------------------------------------

// the output kernel of either call (code_output.h): DataOut is int (stage 1's codewords alone, rows of QR_MAX_DATA) or unsigned char (rows
// of QRV_MAX_DATA, a symbol's codewords from the stage that read it)
template <class DataOut, int ROW>
__global__ __launch_bounds__(256) void qr_output_kernel(const int* res_all, const unsigned char* resdata1_all, const unsigned char* resdata2_all, const int* nfind,
                                                        int max_finders, int max_codes, int* tmp_all, int* counts, int* codes, DataOut* data, int* finder_counts) {
    __shared__ CodeOutLds<QR_MAX_CODES> s;
    const int pg = blockIdx.x;
    const int* res = res_all + (size_t)pg * max_finders * CODE_RES_INTS;
    const int n = code_output_rows(s, res, nfind[pg], max_finders, max_codes, tmp_all + (size_t)pg * max_codes * 6, codes + (size_t)pg * max_codes * 12,
                                   counts + pg, finder_counts ? finder_counts + pg : nullptr);
    if (n > max_codes) return;
    const unsigned char* rd1 = resdata1_all + (size_t)pg * max_finders * QR_MAX_DATA;
    const unsigned char* rd2 = resdata2_all ? resdata2_all + (size_t)pg * max_finders * QRV_MAX_DATA : nullptr;
    code_output_data(s, n, max_finders, ROW, data + (size_t)pg * max_codes * ROW, [=](int slot, int j) -> DataOut {
        const int* r = res + slot * CODE_RES_INTS;
        if (j >= r[8]) return 0;
        if (r[5] <= QR_VERSIONS || !rd2) return j < QR_MAX_DATA ? rd1[(size_t)slot * QR_MAX_DATA + j] : 0;
        return rd2[(size_t)slot * QRV_MAX_DATA + j];
    });
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------------

// the workspace's regions: one layout sizes it (the *_workspace_bytes) and carves it (qr_front_end); resdata2 is the all-versions call's
struct QrWorkspace {
    Components c;
    int* nfind; int4* finders; int* res; unsigned char *resdata, *resdata2; int* tmp;
};
QrWorkspace qrcodes_layout(Arena& a, int B, int H, int W, int max_finders, int max_codes, bool versions) {
    QrWorkspace w;
    w.c = components_layout(a, B, H, W, true);
    w.nfind = a.take<int>((size_t)B);
    w.finders = a.take<int4>((size_t)B * max_finders);
    w.res = a.take<int>((size_t)B * max_finders * CODE_RES_INTS);
    w.resdata = a.take<unsigned char>((size_t)B * max_finders * QR_MAX_DATA);
    w.tmp = a.take<int>((size_t)B * max_codes * 6);
    w.resdata2 = versions ? a.take<unsigned char>((size_t)B * max_finders * QRV_MAX_DATA) : nullptr;
    return w;
}

bool qrcodes_args_ok(int B, int H, int W, int max_finders, int max_codes) {
    return page_args_ok(B, H, W) && max_codes >= 1 && max_codes <= QR_MAX_CODES && max_finders >= 1 && max_finders <= QR_MAX_FINDERS;
}

size_t qr_workspace_bytes(int B, int H, int W, int max_finders, int max_codes, bool versions) {
    if (!qrcodes_args_ok(B, H, W, max_finders, max_codes)) return 0;
    Arena a;
    qrcodes_layout(a, B, H, W, max_finders, max_codes, versions);
    return a.off;
}

// what both calls do first: the arguments checked, the workspace carved, everything up to stage 1's decode enqueued
hipError_t qr_front_end(const QrCommon& p, const void* data, bool versions, void* workspace, size_t ws_bytes, hipStream_t st, QrWorkspace& w, const u64*& mask) {
    const int B = p.B, H = p.H, W = p.W;
    if (!qrcodes_args_ok(B, H, W, p.max_finders, p.max_codes) || !qr_params_ok(p)) return hipErrorInvalidValue;
    if (!p.rgb || !p.codes || !data || !p.counts) return hipErrorInvalidValue;
    Arena a(workspace, ws_bytes);
    w = qrcodes_layout(a, B, H, W, p.max_finders, p.max_codes, versions);
    if (a.overflow) return hipErrorOutOfMemory;
    const int nw = (W + 63) / 64;
    const size_t runcap = run_cap(H, W);
    hipError_t e;
    if ((e = hipMemsetAsync(w.nfind, 0, sizeof(int) * (size_t)B, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.res, 0, sizeof(int) * (size_t)B * p.max_finders * CODE_RES_INTS, st)) != hipSuccess) return e;
    if ((e = components_launch(w.c, p.rgb, p.mask_in, p.mask_out, B, H, W, p.threshold, st)) != hipSuccess) return e;
    mask = w.c.mask;
    const int rows = B * H;
    hipLaunchKernelGGL(qr_finders_kernel, row_wave_grid(rows), dim3(256), 0, st, w.c.runoff, w.c.rxs, w.c.rxe, w.c.parent, w.c.box, w.c.area, H, runcap,
                       p.min_module, p.max_module, p.centre_tol, p.ring_tol, p.max_finders, w.nfind, w.finders, rows);
    hipLaunchKernelGGL(qr_decode_kernel, dim3(p.max_finders, B), dim3(64), 0, st, mask, w.finders, w.nfind, H, W, nw, p.max_finders, p.quiet, p.timing_max, w.res,
                       w.resdata);
    return hipSuccess;
}

}  // namespace

bool qr_params_ok(const QrCommon& p) {
    return p.min_module >= 1 && p.max_module >= p.min_module && p.max_module <= QR_MAX_MODULE && p.quiet >= 0 && p.quiet <= QR_MAX_QUIET && p.centre_tol >= 0 &&
           p.centre_tol <= QR_MAX_TOL && p.ring_tol >= 0 && p.ring_tol <= QR_MAX_TOL && p.timing_max >= 0 && p.timing_max <= QR_MAX_TIMING &&
           p.max_finders >= 1 && p.max_finders <= QR_MAX_FINDERS && p.max_codes >= 1 && p.max_codes <= QR_MAX_CODES;
}
bool qr_max_version_ok(int max_version) { return max_version >= QR_VERSIONS && max_version <= QRV_VERSIONS; }

size_t qrcodes_workspace_bytes(int B, int H, int W, int max_finders, int max_codes) { return qr_workspace_bytes(B, H, W, max_finders, max_codes, false); }
size_t qrcodes_versions_workspace_bytes(int B, int H, int W, int max_finders, int max_codes) { return qr_workspace_bytes(B, H, W, max_finders, max_codes, true); }

hipError_t qrcodes_launch(const QrParams& p, void* workspace, size_t ws_bytes, hipStream_t st) {
    QrWorkspace w;
    const u64* mask;
    const hipError_t e = qr_front_end(p, p.data, false, workspace, ws_bytes, st, w, mask);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((qr_output_kernel<int, QR_MAX_DATA>), dim3(p.B), dim3(256), 0, st, w.res, w.resdata, nullptr, w.nfind, p.max_finders, p.max_codes, w.tmp,
                       p.counts, p.codes, p.data, p.finder_counts);
    return hipGetLastError();
}

hipError_t qrcodes_versions_launch(const QrVersionsParams& p, void* workspace, size_t ws_bytes, hipStream_t st) {
    if (!qr_max_version_ok(p.max_version)) return hipErrorInvalidValue;
    QrWorkspace w;
    const u64* mask;
    const hipError_t e = qr_front_end(p, p.data, true, workspace, ws_bytes, st, w, mask);
    if (e != hipSuccess) return e;
    if (p.max_version > QR_VERSIONS)
        hipLaunchKernelGGL(qr_decode_versions_kernel, dim3(p.max_finders, p.B), dim3(64), 0, st, mask, w.finders, w.nfind, p.H, p.W, (p.W + 63) / 64, p.max_finders,
                           p.quiet, p.timing_max, p.max_version, w.res, w.resdata2);
    hipLaunchKernelGGL((qr_output_kernel<unsigned char, QRV_MAX_DATA>), dim3(p.B), dim3(256), 0, st, w.res, w.resdata, w.resdata2, w.nfind, p.max_finders,
                       p.max_codes, w.tmp, p.counts, p.codes, p.data, p.finder_counts);
    return hipGetLastError();
}
