#pragma once
#include "common.h"

// Aztec codes (compact 1-4 layers, full-range 1-11 layers: the symbols whose module rows fit one 64-bit word) of a batch of pages,
// on the device (aztec.hip; definition restated in tests/aztec_reference.py).  Integer arithmetic throughout: the result does not
// depend on the order anything runs in.
struct AztecParams {
    const uint8_t* rgb;   // [B][H][W][3]
    int B, H, W;
    int threshold;        // ink = L < threshold, L = Pillow's convert('L')
    int min_module, max_module;   // the sides of the core's box (one module)
    int quiet;            // rings of clear modules round the symbol (0 .. AZ_MAX_QUIET; pixels off the page are clear)
    int centre_tol;       // core and 5-module ring concentric within centre_tol / 16 of a module
    int ring_tol;         // the ring's sides are five of the core's within ring_tol / 16 of a module
    int mark_max;         // mismatches allowed in the bullseye's modules and the mode ring's twelve corner modules together
    int max_finders;      // capacity of a page's finder list (<= AZ_MAX_FINDERS); a page with more finders is not read
    int max_codes;        // capacity of a page's list (<= AZ_MAX_CODES)
    int* codes;           // device, [B][max_codes][12] = x0, y0, x1, y1 (the symbol's hull), layers, compact, codeword width, ndata, corrected
                          // errors, rotation (quarter turns clockwise), mode-message errors, bullseye + corner + reference-line mismatches;
                          // sorted by (y0, x0, y1, x1, the core's root)
    int* data;            // device, [B][max_codes][AZ_MAX_DATA]: the corrected data codewords, still bit-stuffed, zero behind ndata
    int* counts;          // device, [B]: true number of symbols (a list is not written when it overflows)
    int* finder_counts;   // optional, device, [B]: true number of finders
    unsigned long long* mask_out;        // optional parity hook: ink mask [B][H][ceil(W / 64)], bit x % 64 of word x / 64
    const unsigned long long* mask_in;   // optional: the ink mask of these pages at this threshold, already computed
};
constexpr int AZ_MAX_DATA = 320;      // >= 316, the codewords of 11 layers
constexpr int AZ_MAX_DATA_ALL = 1664;  // the codewords of 32 layers (lumina_ocr_aztec_layers)
constexpr int AZ_MAX_FINDERS = 64;
constexpr int AZ_MAX_CODES = 64;
constexpr int AZ_MAX_MODULE = 64;
constexpr int AZ_MAX_QUIET = 4;
constexpr int AZ_MAX_TOL = 15;        // of ring_tol; centre_tol <= 64
constexpr int AZ_MAX_MARKS = 64;

bool aztec_params_ok(int min_module, int max_module, int quiet, int centre_tol, int ring_tol, int mark_max, int max_finders, int max_codes);
size_t aztec_workspace_bytes(int B, int H, int W, int max_finders, int max_codes);
hipError_t aztec_launch(const AztecParams& p, void* workspace, size_t ws_bytes, hipStream_t st);

// full-range symbols of every size, 1-32 layers (definition restated in tests/aztec_layers_reference.py): stage 1 is the pass above and
// gives its rows bit for bit; a full-range finder whose mode message says 12 .. max_layers layers and that gave no row is read by a
// second stage with a finer frame and three-word module rows.  p.data is not used: the data rows are data_all.
struct AztecLayersParams : AztecParams {
    int max_layers;             // 11 .. 32; 11 is stage 1 alone
    unsigned short* data_all;   // device, [B][max_codes][AZ_MAX_DATA_ALL]: the corrected data codewords, zero behind ndata
};
bool aztec_max_layers_ok(int max_layers);
size_t aztec_layers_workspace_bytes(int B, int H, int W, int max_finders, int max_codes);
hipError_t aztec_layers_launch(const AztecLayersParams& p, void* workspace, size_t ws_bytes, hipStream_t st);
