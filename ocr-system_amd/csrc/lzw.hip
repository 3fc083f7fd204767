// Strip decoders on the device (lzw.h): LZW, PackBits and uncompressed strips -> packed rows -> RGB.
//
// One wave64 work-group per strip; the grid is the strips of the whole sub-batch (an A4 colour page as libtiff writes it is about 180
// strips of 13 rows, so 64 pages are about 11.5 k independent waves).  Each strip decodes straight into the packed-row buffer at
// page_base + first_row * row_bytes; the row stage of the Flate images (pd_rows_to_rgb, pngdec.h: predictor 2, sample unpack, palette,
// invert) then makes RGB.
//
// LZW: all decode state is wave-uniform.  The input bits sit in a 256-byte window held one big-endian word per lane (read with
// readlane).  The string table lives in LDS as 4096 x {offset of the string in this strip's output, length}: every string a code can
// name already stands in the output, so a code is one lane-parallel copy out[pos .. pos+len) = out[off .. off+len) with no chain walk,
// and the new entry is {pos - prev_len, prev_len + 1}.  8 bytes x 4096 = 32 KB of LDS a wave, five waves a CU.  The copy reads bytes that
// other lanes of this wave stored to global memory a step earlier, so an explicit s_waitcnt vmcnt(0) stands before every copy whose
// source reaches past the last wait.  The wait is conservative: the kernel was never run without it, so it is not known to be needed
// (the memory model orders one wave's accesses to an address).  It is written as inline assembly because a fence or __syncthreads()
// is narrowed to wavefront scope with one wave a work-group and then emits no wait at all.
#include "lzw.h"

#include <algorithm>
#include <cstring>
#include <vector>

#include "engine.h"
#include "pngdec.h"

namespace {

constexpr size_t LZ_IN_PAD = 512;   // zero tail per strip: the LZW word window and the PackBits look-ahead read past the strip's end
enum : int { LZ_E_CORRUPT = 1, LZ_E_UNSUPPORTED = 2 };

struct LzStrip {
    unsigned long long in_off, out_off;   // byte offsets of the strip's input in the staged strips / of its first row in the row buffer
    unsigned in_len, total;               // input bytes; bytes the strip must produce = its rows x row bytes
    int page, codec, rle_eod, pad;
};

// LZW, TIFF 6.0 / PDF flavour.  Returns 0 / -1 / -2 (lzw.h); wave-uniform.
__device__ int lz_lzw(const uint8_t* __restrict__ in, unsigned in_len, uint8_t* out, unsigned total, uint2* tab, int lane) {
    const uint32_t* in32 = reinterpret_cast<const uint32_t*>(in);   // (strips start on 256-byte boundaries)
    const unsigned in_bits = in_len * 8;                            // (in_len < 2^28: the host checks)
    unsigned bp = 0, wbase = 0;
    uint32_t w = __builtin_bswap32(in32[lane]);
    auto get = [&](int n) -> unsigned {   // n bits at bp, MSB first; bp + n <= in_bits
        unsigned idx = (bp >> 5) - wbase;
        if (idx >= 63) { wbase = bp >> 5; w = __builtin_bswap32(in32[wbase + lane]); idx = 0; }   // (at most in_len + 256 bytes in: inside the pad)
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)w, (int)idx), lo = (uint32_t)__builtin_amdgcn_readlane((int)w, (int)idx + 1);
        const uint64_t v = ((uint64_t)hi << 32) | lo;
        const unsigned code = (unsigned)(v >> (64 - (bp & 31) - n)) & ((1u << n) - 1);
        bp += n;
        return code;
    };
    if (in_bits < 9) return -1;
    if (get(9) != 256) return -2;
    int nb = 9;
    unsigned next = 258, pos = 0, prev_pos = 0, prev_len = 0 /* 0: the code before was Clear */, fenced = 0;
    // Bound: every iteration consumes nb >= 9 bits of the strip's in_bits, so there are at most in_bits / 9 of them; every read is below
    // pos <= total, every write below total.
    for (;;) {
        if (bp + nb > in_bits) return -1;   // the data ends before the strip is full
        const unsigned code = get(nb);
        if (code == 256) { nb = 9; next = 258; prev_len = 0; continue; }
        if (code == 257) return -1;         // EOI before the strip is full
        if (prev_len == 0) {
            if (code >= 258) return -1;
        } else if (next >= 4096 || code > next) {
            return -1;                      // the table is full and this is no Clear; or a code above the next free entry
        }
        unsigned off = 0, len = 1, srclen = 1;
        if (code >= 256) {
            if (code == next) { off = prev_pos; srclen = prev_len; len = prev_len + 1; }   // KwKwK: the previous string and its first byte again
            else { const uint2 e = tab[code]; off = e.x; len = srclen = e.y; }
        }
        const unsigned wlen = min(len, total - pos);   // clipped at the strip's end
        if (code < 256) {
            if (lane == 0) out[pos] = (uint8_t)code;
        } else {
            if (off + min(srclen, wlen) > fenced) {   // the source holds bytes stored since the last wait
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                fenced = pos;
            }
            for (unsigned i = lane; i < wlen; i += 64) out[pos + i] = out[off + (i < srclen ? i : i - srclen)];
        }
        if (prev_len != 0) {
            tab[next] = make_uint2(prev_pos, prev_len + 1);   // (every lane stores the same wave-uniform entry)
            ++next;
            if (next >= (1u << nb) - 1 && nb < 12) ++nb;   // early change
        }
        prev_pos = pos; prev_len = len;
        pos += wlen;
        if (pos >= total) return 0;
    }
}

// PackBits.  eod: a header byte of 128 ends the data (/RunLengthDecode) instead of being skipped (TIFF).
__device__ int lz_packbits(const uint8_t* __restrict__ in, unsigned in_len, uint8_t* out, unsigned total, int eod, int lane) {
    unsigned ip = 0, op = 0;
    // Bound: every iteration consumes >= 1 byte of in_len; reads reach at most in_len + 128 (inside the pad), writes stay below total.
    while (op < total) {
        if (ip >= in_len) return -1;
        const int h = in[ip];
        const uint8_t b1 = in[ip + 1 + lane], b2 = in[ip + 65 + lane], rep = in[ip + 1];
        if (h == 128) {
            if (eod) return -1;
            ++ip;
            continue;
        }
        unsigned n;
        bool lit = h < 128;
        if (lit) { n = (unsigned)h + 1; if (ip + 1 + n > in_len) return -1; ip += 1 + n; }
        else { n = 257u - (unsigned)h; if (ip + 2 > in_len) return -1; ip += 2; }
        const unsigned wlen = min(n, total - op);
        if ((unsigned)lane < wlen) out[op + lane] = lit ? b1 : rep;
        if ((unsigned)lane + 64 < wlen) out[op + 64 + lane] = lit ? b2 : rep;
        op += wlen;
    }
    return 0;
}

__global__ __launch_bounds__(64) void lz_strips(const LzStrip* __restrict__ S, const uint8_t* __restrict__ in, uint8_t* rows, int* err) {
    __shared__ uint2 tab[4096];
    const LzStrip s = S[blockIdx.x];
    const int lane = threadIdx.x;
    const uint8_t* src = in + s.in_off;
    uint8_t* dst = rows + s.out_off;
    int rc;
    if (s.codec == LZ_CODEC_LZW) rc = lz_lzw(src, s.in_len, dst, s.total, tab, lane);
    else if (s.codec == LZ_CODEC_PACKBITS) rc = lz_packbits(src, s.in_len, dst, s.total, s.rle_eod, lane);
    else if (s.in_len < s.total) rc = -1;
    else {
        for (unsigned i = lane; i < s.total; i += 64) dst[i] = src[i];   // bounded by the strip's byte count (checked above) and its rows
        rc = 0;
    }
    if (rc != 0 && lane == 0) atomicOr(&err[s.page], rc == -2 ? LZ_E_UNSUPPORTED : LZ_E_CORRUPT);
}

__global__ void lz_status(const PdFile* __restrict__ F, const int* __restrict__ err, int* __restrict__ status, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) status[i] = !F[i].valid ? -1 : (err[i] & LZ_E_UNSUPPORTED) ? -2 : err[i] ? -1 : 0;
}

struct LzWorkspace { PdFile* F; LzStrip* S; int *err, *status; uint8_t *in, *rows; };
LzWorkspace lz_layout(Arena& a, int n, int m, size_t in_total, size_t rows_total) {
    LzWorkspace w;
    w.F = a.take<PdFile>(n); w.S = a.take<LzStrip>(m); w.err = a.take<int>(n); w.status = a.take<int>(n);
    w.in = a.take<uint8_t>(in_total); w.rows = a.take<uint8_t>(rows_total);
    return w;
}

}  // namespace

size_t lzw_workspace_bytes(int n, int m, size_t in_total, size_t rows_total) {
    Arena a;
    lz_layout(a, n, m, in_total, rows_total);
    return a.off;
}

int strip_image_run(lumina_ocr* eng, const uint8_t* const* strips, const size_t* sizes, int m, const int* strip_counts, int n, int height,
                    int width, int rows_per_strip, const int* params, const uint8_t* const* palettes, uint8_t* out_dev, int* status,
                    hipStream_t st) {
    const int want = (height + rows_per_strip - 1) / rows_per_strip;
    // first strip of every page; the counts must add up to m whatever they say about each page
    std::vector<size_t> first((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) {
        if (strip_counts[i] < 0) return locr_fail(eng, "strip_image_decode", "negative strip count");
        first[(size_t)i + 1] = first[(size_t)i] + (size_t)strip_counts[i];
    }
    if (first[(size_t)n] != (size_t)m) return locr_fail(eng, "strip_image_decode", "strip counts do not add up to the number of strips");
    std::vector<size_t> rbs((size_t)n, 0);
    bool any_tiff = false;
    for (int i = 0; i < n; ++i) {
        const int* q = params + 7 * (size_t)i;
        const int codec = q[0], predictor = q[1], comps = q[2], depth = q[3], indexed = q[4], invert = q[5], eod = q[6];
        bool ok = (codec == LZ_CODEC_NONE || codec == LZ_CODEC_LZW || codec == LZ_CODEC_PACKBITS) && (predictor == 1 || predictor == 2) &&
                  (comps == 1 || comps == 3) && (depth == 8 || (comps == 1 && (depth == 1 || depth == 2 || depth == 4))) &&
                  (indexed == 0 || indexed == 1) && (invert == 0 || invert == 1) && (eod == 0 || eod == 1);
        if (predictor == 2 && depth != 8) ok = false;
        if (indexed && (comps != 1 || invert || !palettes || !palettes[i])) ok = false;
        if (invert && comps != 1) ok = false;
        if (strip_counts[i] != want) ok = false;
        const size_t rb = ((size_t)width * (size_t)comps * (size_t)depth + 7) / 8;
        if (ok && (rb * (size_t)height >= ((size_t)1 << 31))) ok = false;   // (32-bit byte offsets inside a page)
        int rc = ok ? 0 : -2;
        for (size_t k = first[(size_t)i]; rc == 0 && k < first[(size_t)i + 1]; ++k) {
            if (sizes[k] >= ((size_t)1 << 28)) rc = -2;        // (32-bit bit positions inside a strip)
            else if (sizes[k] && !strips[k]) rc = -1;
        }
        rbs[(size_t)i] = rb;
        status[i] = rc;
        if (rc == 0 && predictor == 2) any_tiff = true;
    }
    lumina_ocr::Staging& stage = eng->pd_stage;
    if (!stage.uploaded) {
        hipEvent_t ev = nullptr;
        LOCR_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        stage.uploaded.reset(ev);
    }
    // sub-batches of at most eng->pd_sub_batch_mb MB of packed rows (at least one page each): the workspace holds one sub-batch
    const size_t sub_rows = (size_t)eng->pd_sub_batch_mb << 20;
    int i0 = 0;
    while (i0 < n) {
        int i1 = i0;
        size_t fsum = 0;
        while (i1 < n && (i1 == i0 || fsum + rbs[(size_t)i1] * height <= sub_rows)) { if (status[i1] == 0) fsum += rbs[(size_t)i1] * height; ++i1; }
        const int nb = i1 - i0;
        std::vector<PdFile> F((size_t)nb);
        std::vector<LzStrip> S;
        size_t in_total = 0, rows_total = 0;
        for (int k = 0; k < nb; ++k) {
            PdFile& f = F[(size_t)k];
            memset(&f, 0, sizeof(f));
            const int i = i0 + k;
            if (status[i] != 0) continue;
            const int* q = params + 7 * (size_t)i;
            f.valid = 1;
            f.width = width; f.height = height; f.depth = q[3]; f.ct = q[4] ? 3 : q[2] == 3 ? 2 : 0; f.out_index = i;
            f.bpp = f.depth < 8 ? 1 : q[2];
            f.rb = (unsigned)rbs[(size_t)i];
            f.total = (unsigned)(rbs[(size_t)i] * height);
            f.fb = 0; f.tiff = q[1] == 2; f.invert = q[5];
            if (q[4]) { f.npal = 256; memcpy(f.pal, palettes[i], 768); }
            f.foff = rows_total; rows_total += (((size_t)f.total + 255) & ~(size_t)255) + 256;
            for (int s = 0; s < want; ++s) {
                const size_t k_in = first[(size_t)i] + (size_t)s;
                const int r0 = s * rows_per_strip, r1 = std::min(height, r0 + rows_per_strip);
                LzStrip z;
                z.in_off = in_total; in_total += ((sizes[k_in] + 255) & ~(size_t)255) + LZ_IN_PAD;
                z.out_off = f.foff + (size_t)r0 * f.rb;
                z.in_len = (unsigned)sizes[k_in]; z.total = (unsigned)((size_t)(r1 - r0) * f.rb);
                z.page = k; z.codec = q[0]; z.rle_eod = q[6]; z.pad = 0;
                S.push_back(z);
            }
        }
        if (!S.empty()) {
            LOCR_CHECK(hipEventSynchronize(stage.uploaded.get()));
            LOCR_CHECK(stage.buf.reserve(in_total, stage.uploaded.get()));
            uint8_t* zs = stage.buf.get();
            // the staging copy: strip j of the sub-batch to zs + S[j].in_off, its slot (size rounded up to 256, + LZ_IN_PAD) zero-filled;
            // the slots were summed into in_total from the same sizes, so every copy lies inside the reservation
            size_t j = 0;
            for (int k = 0; k < nb; ++k) {
                if (!F[(size_t)k].valid) continue;
                for (int s = 0; s < want; ++s, ++j) {
                    const size_t k_in = first[(size_t)(i0 + k)] + (size_t)s;
                    const size_t slot = ((sizes[k_in] + 255) & ~(size_t)255) + LZ_IN_PAD;
                    if (S[j].in_off + slot > in_total) return locr_fail(eng, "strip_image_decode", "staging layout");
                    if (sizes[k_in]) memcpy(zs + S[j].in_off, strips[k_in], sizes[k_in]);
                    memset(zs + S[j].in_off + sizes[k_in], 0, slot - sizes[k_in]);
                }
            }
            const int ms = (int)S.size();
            Arena sizing;
            lz_layout(sizing, nb, ms, in_total, rows_total);
            if (eng_ws_reserve(eng, sizing.off)) return 1;
            Arena a(eng->ws.get(), eng->ws.cap);
            const LzWorkspace w = lz_layout(a, nb, ms, in_total, rows_total);
            if (a.overflow) return locr_fail(eng, "strip_image_decode", "workspace layout exceeds the reservation");
            LOCR_CHECK(hipMemcpyAsync(w.F, F.data(), sizeof(PdFile) * nb, hipMemcpyHostToDevice, st));
            LOCR_CHECK(hipMemcpyAsync(w.S, S.data(), sizeof(LzStrip) * ms, hipMemcpyHostToDevice, st));
            LOCR_CHECK(hipMemcpyAsync(w.in, zs, in_total, hipMemcpyHostToDevice, st));
            LOCR_CHECK(hipEventRecord(stage.uploaded.get(), st));
            LOCR_CHECK(hipMemsetAsync(w.err, 0, sizeof(int) * nb, st));
            hipLaunchKernelGGL(lz_strips, dim3((unsigned)ms), dim3(64), 0, st, w.S, w.in, w.rows, w.err);
            pd_rows_to_rgb(w.F, w.rows, w.err, nb, height, width, any_tiff, out_dev, st);
            hipLaunchKernelGGL(lz_status, dim3((nb + 63) / 64), dim3(64), 0, st, w.F, w.err, w.status, nb);
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
