#pragma once
#include "common.h"

// QR codes (Model 2) of a batch of pages, on the device (qrcodes.hip).  Integer arithmetic throughout: the result does not depend on
// the order anything runs in.  Two calls share one front end (ink mask, run list, finders, the decode of versions 1-10) and one set of
// device steps; QrCommon is what both take.
struct QrCommon {
    const uint8_t* rgb;   // [B][H][W][3]
    int B, H, W;
    int threshold;        // ink = L < threshold, L = Pillow's convert('L')
    int min_module, max_module;   // a finder's core (3 x 3 modules) has sides 3 min_module .. 3 max_module
    int quiet;            // rings of clear modules round the symbol (0 .. QR_MAX_QUIET; pixels off the page are clear)
    int centre_tol;       // core and ring centres agree within centre_tol / 16 of a module
    int ring_tol;         // the ring's sides are 7/3 of the core's within ring_tol / 16 of a module
    int timing_max;       // mismatches allowed in the two timing patterns
    int max_finders;      // capacity of a page's finder list (<= QR_MAX_FINDERS); a page with more finders is not read
    int max_codes;        // capacity of a page's list (<= QR_MAX_CODES)
    int* codes;           // device, [B][max_codes][12] = x0, y0, x1, y1 (the symbol's hull), version, level (0..3 = L, M, Q, H), mask, ndata,
                          // corrected errors, rotation (quarter turns clockwise), format distance (+ 16: second copy), timing mismatches;
                          // sorted by (y0, x0, y1, x1, corner finder's root)
    int* counts;          // device, [B]: true number of symbols (a list is not written when it overflows)
    int* finder_counts;   // optional, device, [B]: true number of finder patterns
    unsigned long long* mask_out;        // optional parity hook: ink mask [B][H][ceil(W / 64)], bit x % 64 of word x / 64
    const unsigned long long* mask_in;   // optional: the ink mask of these pages at this threshold, already computed
};
constexpr int QR_MAX_FINDERS = 64;     // one wave64 lane per finder
constexpr int QR_MAX_CODES = 64;
constexpr int QR_MAX_MODULE = 64;
constexpr int QR_MAX_QUIET = 4;
constexpr int QR_MAX_TOL = 64;
constexpr int QR_MAX_TIMING = 128;
bool qr_params_ok(const QrCommon& p);   // the scalar parameters from min_module to max_codes

// versions 1-10 (definition restated in tests/qr_reference.py)
struct QrParams : QrCommon {
    int* data;            // device, [B][max_codes][QR_MAX_DATA]: the corrected data codewords, zero behind ndata
};
constexpr int QR_MAX_DATA = 288;       // >= 274, the data codewords of 10-L
size_t qrcodes_workspace_bytes(int B, int H, int W, int max_finders, int max_codes);
hipError_t qrcodes_launch(const QrParams& p, void* workspace, size_t ws_bytes, hipStream_t st);

// every version, 1-40 (definition restated in tests/qr_versions_reference.py): stage 1 is the pass above and gives its result bit for
// bit; stage 2 reads versions 11 .. max_version for the corner finders stage 1 gave no symbol
struct QrVersionsParams : QrCommon {
    int max_version;      // 10 .. 40; at 10 stage 2 never runs
    unsigned char* data;  // device, [B][max_codes][QR_VERSIONS_MAX_DATA]: the corrected data codewords as bytes, zero behind ndata
};
constexpr int QR_VERSIONS_MAX_DATA = 2956;   // the data codewords of 40-L
bool qr_max_version_ok(int max_version);
size_t qrcodes_versions_workspace_bytes(int B, int H, int W, int max_finders, int max_codes);
hipError_t qrcodes_versions_launch(const QrVersionsParams& p, void* workspace, size_t ws_bytes, hipStream_t st);
