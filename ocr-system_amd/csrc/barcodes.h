#pragma once
#include "common.h"

// Code 128, Code 39, EAN-13 / UPC-A, EAN-8, UPC-E and ITF barcodes of a batch of pages, on the device (barcodes.hip; definition restated
// in tests/barcode_reference.py for the first two and tests/linear_reference.py for every kind).
// Integer arithmetic throughout: the result does not depend on the order anything runs in.
struct BarcodeParams {
    const uint8_t* rgb;   // [B][H][W][3]
    int B, H, W;
    int threshold;        // ink = L < threshold, L = Pillow's convert('L')
    int quiet;            // the gap before a start is at least quiet module widths of the start symbol (the page edge is quiet)
    int max_dist;         // a symbol of S pixels and M modules is rejected when its best sum |w_i M - p_i S| exceeds max_dist S M / 256
    int min_rows;         // reads a barcode needs
    int row_gap;          // equal reads join when their rows are at most this far apart (1 .. BARCODE_MAX_ROW_GAP)
    int max_codes;        // capacity of a page's list (<= BARCODE_MAX_CODES)
    int kinds;            // the kinds to read, bit k = kind k (1 .. BARCODE_KINDS_ALL)
    int* codes;           // device, [B][max_codes][8] = x0, y0, x1, y1, kind (0 Code 128, 1 Code 39, 2 EAN-13, 3 EAN-8, 4 UPC-E, 5 ITF), nsym,
                          // rows, flags (bit 0 reversed, bit 1 vertical, bit 2 ITF-14); sorted by (y0, x0, y1, x1, first read)
    int* syms;            // device, [B][max_codes][BARCODE_MAX_SYMS]: the symbol values in reading order, zero behind nsym
    int* counts;          // device, [B]: true number of barcodes (a list is not written when it overflows)
    unsigned long long* mask_out;        // optional parity hook: ink mask [B][H][ceil(W / 64)], bit x % 64 of word x / 64
    const unsigned long long* mask_in;   // optional: the ink mask of these pages at this threshold, already computed
};
constexpr int BARCODE_MAX_SYMS = 64;     // one wave64 lane per symbol
constexpr int BARCODE_ROW_READS = 4;     // reads kept per row, leftmost first
constexpr int BARCODE_MAX_CODES = 256;
constexpr int BARCODE_MAX_ROW_GAP = 16;
constexpr int BARCODE_MAX_DIST = 256;    // keeps max_dist * S * M inside an int (S <= 65535, M <= 15)
constexpr int BARCODE_MAX_QUIET = 64;
constexpr int BARCODE_KINDS_DEFAULT = 3; // Code 128 and Code 39: what lumina_ocr_barcodes reads
constexpr int BARCODE_KINDS_ALL = 63;

bool barcode_params_ok(int quiet, int max_dist, int min_rows, int row_gap, int max_codes);
bool barcode_kinds_ok(int kinds);
size_t barcodes_workspace_bytes(int B, int H, int W, int max_codes);
hipError_t barcodes_launch(const BarcodeParams& p, void* workspace, size_t ws_bytes, hipStream_t st);
