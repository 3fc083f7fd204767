// CCITT fax decoders on the device (ccitt.h): Group 4 (cc_decode, described first) and, on the same tables, bit reader and line stages,
// Group 3 and CCITT RLE (fx_decode, described where it stands).
//
// T.6 has no synchronisation points and codes every line against the one above, so the unit of parallelism is the page: one wave64
// work-group per page.  The changing elements of the reference line and of the line being decoded sit in LDS as u16, next to the lookup
// tables (12 bits for white runs, 13 for black runs, 7 for the modes), which the wave expands from the code lists of ccitt_tables.h when
// it starts.  The walk over the codes is wave-uniform (every lane computes the same state, lane 0 writes it): the stream is read MSB
// first through a 256-byte window held one byte-swapped word per lane (readlane), over a zero-padded tail, as pngdec.hip's reader does.
// After each line the whole wave turns the line's changing elements into pixels: lanes over 32-pixel words (a binary search for the
// colour at the word's start, then the elements inside it), then lanes over the RGB bytes of the output row with coalesced stores.
//
// Hostile streams: every table index is a bit field of the table's width; an unused pattern has entry 0 and ends the page; a0 must
// advance on every code and never passes `columns`; a pass code whose b2 is the line's end is refused (T.6 allows pass mode only when
// b2 lies left of a1, and a1 <= columns; libtiff reads such a code differently, and the host path is libtiff); a line holds at most
// columns + 1 changing elements (the arrays have room for them and three sentinels); the bit position is checked against the stream
// length after every code.  Each of these is status -1.
#include "ccitt.h"

#include <cstring>
#include <vector>

#include "ccitt_tables.h"
#include "engine.h"

namespace {

constexpr int CC_WBITS = 12, CC_BBITS = 13, CC_MBITS = 7;
constexpr size_t CC_Z_PAD = 512;   // zero tail per stream: the bit reader's word window may look past the stream

enum : int { CC_GROUP4 = 1, CC_FAX = 2 };   // CcPage::valid: the kernel that takes the page (0: none)

struct CcPage {
    unsigned long long zoff;   // byte offset of the stream in the batch's buffer
    unsigned zlen;
    int white_value, valid, out_index;   // white_value: the byte a coded-white pixel becomes (0 / 255)
    int k, align;                        // fx_decode: K >= 0 and EncodedByteAlign
};

struct CcLds {
    unsigned short ce[2][CC_MAX_COLS + 8];   // changing elements of two lines, each followed by three sentinels (= columns)
    unsigned short wt[1 << CC_WBITS], bt[1 << CC_BBITS], mt[1 << CC_MBITS];   // code length << 12 | value; 0: no such code
    unsigned bits[CC_MAX_COLS / 32];   // the finished line, 1 = coded black, pixel x at bit x & 31 of word x >> 5
};

// wave-uniform MSB-first bit reader: lanes hold 64 consecutive byte-swapped words from word `wbase`
struct CcBits {
    const uint32_t* z32;
    unsigned zlen, pos, wbase;
    uint32_t w;
    bool bad;
    __device__ void load(int lane) {
        wbase = pos >> 5;
        if ((size_t)wbase * 4 > (size_t)zlen + 8) { bad = true; wbase = 0; }   // ran past the stream (the tail padding covers one window)
        w = __builtin_bswap32(z32[wbase + lane]);
    }
    // the next 32 bits, the first one on top
    __device__ uint32_t peek(int lane) {
        if (bad) return 0;
        if ((pos >> 5) - wbase >= 32) { load(lane); if (bad) return 0; }
        const int idx = (int)((pos >> 5) - wbase);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)w, idx), lo = (uint32_t)__builtin_amdgcn_readlane((int)w, idx + 1);
        return (uint32_t)((((((uint64_t)hi) << 32) | lo) << (pos & 31)) >> 32);
    }
};

__device__ void cc_fill(unsigned short* table, int bits, const unsigned* codes, int ncodes, int lane) {
    for (int i = lane; i < (1 << bits); i += 64) table[i] = 0;
    __syncthreads();
    for (int c = 0; c < ncodes; ++c) {
        const unsigned code = codes[c];
        const int len = (int)((code >> 12) & 15);
        const int base = (int)(code >> 16) << (bits - len), span = 1 << (bits - len);
        for (int i = lane; i < span; i += 64) table[base + i] = (unsigned short)(code & 0xFFFFu);
    }
    __syncthreads();
}

// one run length: make-up codes, then a terminating code.  -1: an unused code, a run longer than `room`, or bits past the stream.
// Ends: every pass returns or adds at least 64 to `total`.
__device__ int cc_run(const CcLds& L, CcBits& b, bool white, int room, unsigned limit, int lane) {
    int total = 0;
    for (;;) {
        const uint32_t top = b.peek(lane);
        const unsigned e = white ? L.wt[top >> (32 - CC_WBITS)] : L.bt[top >> (32 - CC_BBITS)];
        if (e == 0) return -1;
        b.pos += e >> 12;
        total += (int)(e & 4095);
        if (total > room || b.pos > limit) return -1;
        if ((e & 4095) < 64) return total;
    }
}

// one line in the two-dimensional coding against the changing elements `ref` of the line above (T.6; T.4 with K > 0): the line's
// changing elements go to `cur`.  -> their number, -1 corrupt.  Wave-uniform; lane 0 writes.
__device__ __forceinline__ int cc_line_2d(const CcLds& L, CcBits& b, const unsigned short* ref, unsigned short* cur, int W, unsigned limit, int lane) {
    int a0 = -1, n = 0, ri = 0;
    bool white = true;
    while (a0 < W) {
        while ((int)ref[ri] <= a0) ri += 2;   // b1: the first changing element right of a0 that changes to the opposite colour (ends at a sentinel: a0 < W)
        const int b1 = ref[ri], b2 = ref[ri + 1];
        const unsigned e = L.mt[b.peek(lane) >> (32 - CC_MBITS)];
        if (e == 0) return -1;
        b.pos += e >> 12;
        if (b.pos > limit) return -1;
        const int mode = (int)(e & 4095);
        if (mode == CC_M_PASS) {
            if (b2 >= W) return -1;   // T.6, pass mode: "identified when the position of b2 lies to the left of a1", and a1 <= columns
            a0 = b2;   // (b2 > b1 > a0)
            continue;
        }
        if (mode == CC_M_HORIZ) {
            const int start = a0 < 0 ? 0 : a0;
            const int r1 = cc_run(L, b, white, W - start, limit, lane);
            if (r1 < 0) return -1;
            const int r2 = cc_run(L, b, !white, W - start - r1, limit, lane);
            if (r2 < 0) return -1;
            const int t1 = start + r1, t2 = t1 + r2;
            if (t2 <= a0) return -1;
            // (a change at the line's end is the sentinel's and takes no room: a line of `columns` elements may end with such a pair)
            if (n + (t1 < W) + (t2 < W) > W + 1) return -1;
            if (lane == 0) {
                if (t1 < W) cur[n] = (unsigned short)t1;
                if (t2 < W) cur[n + (t1 < W)] = (unsigned short)t2;
            }
            n += (t1 < W) + (t2 < W);
            a0 = t2;
        } else {
            const int d = mode <= CC_M_VR3 ? mode - CC_M_V0 : CC_M_VR3 - mode;
            const int a1 = b1 + d;
            if (a1 <= a0 || a1 > W || (a1 < W && n + 1 > W + 1)) return -1;
            if (a1 < W) {
                if (lane == 0) cur[n] = (unsigned short)a1;
                ++n;
            }
            a0 = a1;
            white = !white;
            ri = ri > 0 ? ri - 1 : ri + 1;
        }
    }
    return n;
}

// the finished line, n <= W + 1 changing elements in `cur` (one of L.ce): its three sentinels, then its pixels as RGB bytes at `row`.
// The whole wave: lanes over 32-pixel words, then over the bytes of the row.
__device__ __forceinline__ void cc_line_out(CcLds& L, unsigned short* cur, int n, int W, uint8_t* row, int wv, int bv, int lane) {
    if (lane < 3) cur[n + lane] = (unsigned short)W;
    __syncthreads();
    // the line's words: pixel x is coded black when an odd number of changing elements lie at or left of it
    for (int j = lane; j * 32 < W; j += 64) {
        const int x0 = j * 32;
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int)cur[mid] <= x0) lo = mid + 1; else hi = mid;
        }
        int k = lo, pos = 0;
        unsigned word = 0;
        for (;;) {
            const int next = k < n ? min((int)cur[k] - x0, 32) : 32;
            if ((k & 1) && next > pos) word |= (next >= 32 ? 0xFFFFFFFFu : ((1u << next) - 1u)) & ~((1u << pos) - 1u);
            pos = next;
            if (pos >= 32) break;
            ++k;
        }
        L.bits[j] = word;
    }
    __syncthreads();
    for (int bx = lane; bx < W * 3; bx += 64) {
        const int px = bx / 3;
        row[bx] = (uint8_t)(((L.bits[px >> 5] >> (px & 31)) & 1u) ? bv : wv);
    }
    __syncthreads();
}

__device__ __forceinline__ void cc_tables(CcLds& L, int W, int lane) {
    cc_fill(L.wt, CC_WBITS, cc_white_codes, CC_N_RUN_CODES, lane);
    cc_fill(L.bt, CC_BBITS, cc_black_codes, CC_N_RUN_CODES, lane);
    cc_fill(L.mt, CC_MBITS, cc_mode_codes, CC_N_MODE_CODES, lane);
    if (lane < 3) L.ce[0][lane] = (unsigned short)W;   // the imaginary white line above the first
    __syncthreads();
}

__global__ __launch_bounds__(64) void cc_decode(const CcPage* __restrict__ P, const uint8_t* __restrict__ z, uint8_t* __restrict__ out,
                                                int* __restrict__ status, int rows, int W) {
    __shared__ CcLds L;
    const CcPage& p = P[blockIdx.x];
    if (p.valid != CC_GROUP4) return;
    const int lane = threadIdx.x;
    cc_tables(L, W, lane);
    CcBits b;
    b.z32 = reinterpret_cast<const uint32_t*>(z + p.zoff); b.zlen = p.zlen; b.pos = 0; b.bad = false;
    b.load(lane);
    const unsigned limit = p.zlen * 8u;
    const int wv = p.white_value, bv = 255 - p.white_value;
    uint8_t* dst = out + (size_t)p.out_index * rows * W * 3;
    int y = 0, sel = 0;
    bool bad = false;
    for (; y < rows; ++y) {
        if ((b.peek(lane) >> 8) == 0x001001u) break;   // EOFB
        unsigned short* cur = L.ce[sel ^ 1];
        const int n = cc_line_2d(L, b, L.ce[sel], cur, W, limit, lane);
        if (n < 0) { bad = true; break; }
        cc_line_out(L, cur, n, W, dst + (size_t)y * W * 3, wv, bv, lane);
        sel ^= 1;
    }
    if (lane == 0) status[blockIdx.x] = (bad || b.bad || y < rows) ? -1 : 0;
}

// one line in the one-dimensional coding (T.4): white and black runs in turn, white first, that add up to W exactly; only the line's
// first run may be 0 long, so the changing elements rise and there are at most W of them.  -> their number, -1 corrupt.
__device__ __forceinline__ int fx_line_1d(const CcLds& L, CcBits& b, unsigned short* cur, int W, unsigned limit, int lane) {
    int a0 = 0, n = 0;
    bool white = true, first = true;
    for (;;) {   // ends: every run after the first adds at least 1 to a0
        const int r = cc_run(L, b, white, W - a0, limit, lane);
        if (r < 0 || (r == 0 && !first)) return -1;
        first = false;
        a0 += r;
        if (a0 >= W) return n;   // (r <= W - a0: the line ends at W exactly)
        if (lane == 0) cur[n] = (unsigned short)a0;
        ++n;
        white = !white;
    }
}

// Group 3 and CCITT RLE (T.4), one wave64 per stream like cc_decode and on its tables, bit reader and line stages.  Every line begins
// with the zero bits in front of it; 11 or more of them and a 1 are an EOL (fill is part of the zeros and may be thousands of bits, so
// they are skipped a word at a time against the stream's length).  The first line decides whether the stream carries EOLs: all lines
// or none.  With k > 0 the bit after an EOL picks the line's coding.  align: without EOLs every line begins on a byte boundary.
__global__ __launch_bounds__(64) void fx_decode(const CcPage* __restrict__ P, const uint8_t* __restrict__ z, uint8_t* __restrict__ out,
                                                int* __restrict__ status, int rows, int W) {
    __shared__ CcLds L;
    const CcPage& p = P[blockIdx.x];
    if (p.valid != CC_FAX) return;
    const int lane = threadIdx.x;
    cc_tables(L, W, lane);
    CcBits b;
    b.z32 = reinterpret_cast<const uint32_t*>(z + p.zoff); b.zlen = p.zlen; b.pos = 0; b.bad = false;
    b.load(lane);
    const unsigned limit = p.zlen * 8u;
    const int wv = p.white_value, bv = 255 - p.white_value;
    const bool two_d = p.k > 0, align = p.align != 0;
    uint8_t* dst = out + (size_t)p.out_index * rows * W * 3;
    int y = 0, sel = 0, st = -1;
    bool eol_mode = false;
    for (; y < rows; ++y) {
        if (align) {
            b.pos = (b.pos + 7u) & ~7u;   // (limit is a multiple of 8)
            // a line that begins in the stream's last byte: libtiff pads its bit window with zeros when a lookup reaches the strip's end
            // and counts the padding when it skips to the byte boundary, so it may read this line from the wrong bit; refused
            if (y > 0 && limit - b.pos <= 8u) break;
        }
        bool eol = false;
        if ((b.peek(lane) >> 21) == 0) {   // 11 zeros or more
            uint32_t top;
            while ((top = b.peek(lane)) == 0 && b.pos <= limit) b.pos += 32;   // ends: the position rises to the limit
            if (top == 0) break;   // zeros to the stream's end
            b.pos += (unsigned)__clz(top) + 1u;
            if (b.pos > limit) break;
            eol = true;
        }
        if (y == 0) {
            eol_mode = eol;
            if ((two_d && !eol) || (align && eol)) { st = -2; break; }   // (nothing to hold either against)
        } else if (eol != eol_mode) break;
        bool one_d = true;
        if (eol && two_d) {
            one_d = (b.peek(lane) >> 31) != 0;
            b.pos += 1;
            if (b.pos > limit) break;
        }
        unsigned short* cur = L.ce[sel ^ 1];
        const int n = one_d ? fx_line_1d(L, b, cur, W, limit, lane) : cc_line_2d(L, b, L.ce[sel], cur, W, limit, lane);
        if (n < 0) break;
        cc_line_out(L, cur, n, W, dst + (size_t)y * W * 3, wv, bv, lane);
        sel ^= 1;
    }
    if (lane == 0) status[blockIdx.x] = (y == rows && !b.bad) ? 0 : st;
}

struct CcWorkspace { CcPage* P; int* status; uint8_t* z; };
CcWorkspace cc_layout(Arena& a, int n, size_t z_total) {
    CcWorkspace w;
    w.P = a.take<CcPage>(n); w.status = a.take<int>(n); w.z = a.take<uint8_t>(z_total);
    return w;
}

}  // namespace

// the batch of either entry: `stride` ints of parameters per stream (4: ccitt_run, Group 4 alone; 5: fax_run, every coding)
static int cc_run_batch(lumina_ocr* eng, const char* what, const uint8_t* const* streams, const size_t* sizes, int n, int rows, int columns,
                        const int* params, int stride, uint8_t* out_dev, int* status, hipStream_t st) {
    std::vector<CcPage> P((size_t)n);
    size_t z_total = 0;
    int any = 0, any_fax = 0;
    for (int i = 0; i < n; ++i) {
        CcPage& p = P[(size_t)i];
        memset(&p, 0, sizeof(p));
        const int* q = params + (size_t)stride * (size_t)i;
        const bool fax = stride == 5 && q[0] >= 0;
        if (columns > CC_MAX_COLS || sizes[i] >= ((size_t)1 << 28)) { status[i] = -2; continue; }   // (32-bit bit positions)
        if (fax ? (q[4] != 0 && q[4] != 1) : (q[0] >= 0 || q[1] != 0 || (stride == 5 && (q[4] < 0 || q[4] > 1)))) { status[i] = -2; continue; }
        if (!streams[i] || sizes[i] == 0) { status[i] = -1; continue; }
        status[i] = 0;
        p.valid = fax ? CC_FAX : CC_GROUP4; ++any; any_fax += fax;
        p.out_index = i;
        p.white_value = ((q[2] != 0) == (q[3] != 0)) ? 255 : 0;   // coded white is sample 1 unless BlackIs1; sample 1 is 255 unless inverted
        p.k = fax ? q[0] : -1;
        p.align = fax ? (q[1] != 0) : 0;
        p.zlen = (unsigned)sizes[i];
        p.zoff = z_total; z_total += ((sizes[i] + 255) & ~(size_t)255) + CC_Z_PAD;
    }
    if (!any) return 0;
    lumina_ocr::Staging& stage = eng->pd_stage;
    if (!stage.uploaded) {
        hipEvent_t ev = nullptr;
        LOCR_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        stage.uploaded.reset(ev);
    }
    LOCR_CHECK(hipEventSynchronize(stage.uploaded.get()));
    LOCR_CHECK(stage.buf.reserve(z_total, stage.uploaded.get()));
    uint8_t* zs = stage.buf.get();
    for (int i = 0; i < n; ++i) {
        const CcPage& p = P[(size_t)i];
        if (!p.valid) continue;
        memcpy(zs + p.zoff, streams[i], sizes[i]);
        memset(zs + p.zoff + sizes[i], 0, ((sizes[i] + 255) & ~(size_t)255) + CC_Z_PAD - sizes[i]);
    }
    Arena sizing;
    cc_layout(sizing, n, z_total);
    if (eng_ws_reserve(eng, sizing.off)) return 1;
    Arena a(eng->ws.get(), eng->ws.cap);
    const CcWorkspace w = cc_layout(a, n, z_total);
    if (a.overflow) return locr_fail(eng, what, "workspace layout exceeds the reservation");
    LOCR_CHECK(hipMemcpyAsync(w.P, P.data(), sizeof(CcPage) * n, hipMemcpyHostToDevice, st));
    LOCR_CHECK(hipMemcpyAsync(w.z, zs, z_total, hipMemcpyHostToDevice, st));
    LOCR_CHECK(hipEventRecord(stage.uploaded.get(), st));
    LOCR_CHECK(hipMemsetAsync(w.status, 0xFF, sizeof(int) * n, st));   // (-1 until the page's wave says otherwise)
    if (any > any_fax) hipLaunchKernelGGL(cc_decode, dim3(n), dim3(64), 0, st, w.P, w.z, out_dev, w.status, rows, columns);
    if (any_fax) hipLaunchKernelGGL(fx_decode, dim3(n), dim3(64), 0, st, w.P, w.z, out_dev, w.status, rows, columns);
    std::vector<int> dev_status((size_t)n);
    LOCR_CHECK(hipMemcpyAsync(dev_status.data(), w.status, sizeof(int) * n, hipMemcpyDeviceToHost, st));
    LOCR_CHECK(hipStreamSynchronize(st));
    LOCR_CHECK(hipGetLastError());
    for (int i = 0; i < n; ++i)
        if (P[(size_t)i].valid) status[i] = dev_status[(size_t)i];
    return 0;
}

int ccitt_run(lumina_ocr* eng, const uint8_t* const* streams, const size_t* sizes, int n, int rows, int columns, const int* params,
              uint8_t* out_dev, int* status, hipStream_t st) {
    return cc_run_batch(eng, "ccitt_decode", streams, sizes, n, rows, columns, params, 4, out_dev, status, st);
}

int fax_run(lumina_ocr* eng, const uint8_t* const* streams, const size_t* sizes, int n, int rows, int columns, const int* params,
            uint8_t* out_dev, int* status, hipStream_t st) {
    return cc_run_batch(eng, "fax_decode", streams, sizes, n, rows, columns, params, 5, out_dev, status, st);
}
