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

#include "ccitt_lines.h"
#include "engine.h"

namespace {

enum : int { CC_GROUP4 = 1, CC_FAX = 2 };   // CcPage::valid: the kernel that takes the page (0: none)

struct CcPage {
    unsigned long long zoff;   // byte offset of the stream in the batch's buffer
    unsigned zlen;
    int white_value, valid, out_index;   // white_value: the byte a coded-white pixel becomes (0 / 255)
    int k, align;                        // fx_decode: K >= 0 and EncodedByteAlign
};

// the finished line (cc_line_words), then its pixels as RGB bytes at `row`: lanes over the bytes of the row
__device__ __forceinline__ void cc_line_out(CcLds& L, unsigned short* cur, int n, int W, uint8_t* row, int wv, int bv, int lane) {
    cc_line_words(L, cur, n, W, lane);
    for (int bx = lane; bx < W * 3; bx += 64) {
        const int px = bx / 3;
        row[bx] = (uint8_t)(((L.bits[px >> 5] >> (px & 31)) & 1u) ? bv : wv);
    }
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
