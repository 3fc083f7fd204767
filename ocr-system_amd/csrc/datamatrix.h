#pragma once
#include "common.h"

// Data Matrix (ECC 200, the 21 sizes up to 52 x 52 and 16 x 48) of a batch of pages, on the device (datamatrix.hip; definition
// restated in tests/dm_reference.py).  Integer arithmetic throughout: the result does not depend on the order anything runs in.
struct DmParams {
    const uint8_t* rgb;   // [B][H][W][3]
    int B, H, W;
    int threshold;        // ink = L < threshold, L = Pillow's convert('L')
    int min_module, max_module;   // a candidate's box has sides 8 min_module .. 52 max_module; a size is in reach when both arms give a module in this range
    int quiet;            // rings of clear modules round the symbol (0 .. DM_MAX_QUIET; pixels off the page are clear)
    int timing_max;       // mismatches allowed in the clock tracks and the inner clock bars
    int solid_max;        // clear modules allowed in the L and the inner solid bars
    int max_candidates;   // capacity of a page's candidate list (<= DM_MAX_CANDIDATES); a page with more candidates is not read
    int max_codes;        // capacity of a page's list (<= DM_MAX_CODES)
    int* codes;           // device, [B][max_codes][12] = x0, y0, x1, y1 (the symbol's hull), rows, cols, ndata, corrected errors, rotation
                          // (quarter turns clockwise), timing mismatches, L misses, 0; sorted by (y0, x0, y1, x1, the component's root)
    int* data;            // device, [B][max_codes][DM_MAX_DATA]: the corrected data codewords, zero behind ndata
    int* counts;          // device, [B]: true number of symbols (a list is not written when it overflows)
    int* candidate_counts;   // optional, device, [B]: true number of candidates
    unsigned long long* mask_out;        // optional parity hook: ink mask [B][H][ceil(W / 64)], bit x % 64 of word x / 64
    const unsigned long long* mask_in;   // optional: the ink mask of these pages at this threshold, already computed
};
constexpr int DM_MAX_DATA = 208;         // >= 204, the data codewords of 52 x 52
constexpr int DM_MAX_CANDIDATES = 1024;   // the decode grid is max_candidates waves a page; no lane stands for a candidate
constexpr int DM_MAX_CODES = 64;
constexpr int DM_MAX_MODULE = 64;
constexpr int DM_MAX_QUIET = 4;
constexpr int DM_MAX_TIMING = 128;

// every ECC 200 size (definition restated in tests/dm_sizes_reference.py): stage 1 is the pass above, with the same rows and codewords;
// a root with box sides in 64 min_module .. 144 max_module that gave no such row goes through stage 2, which reads the squares of
// 64 x 64 .. max_size from a candidate list of its own (capacity max_candidates; a page with more is not read by stage 2).  `data` is
// not used: the rows of both stages come as bytes in data_all.
struct DmSizesParams : DmParams {
    int max_size;               // DM_MIN_MAX_SIZE (stage 1 alone) .. DM_MAX_MAX_SIZE
    unsigned char* data_all;    // device, [B][max_codes][DM_MAX_DATA_ALL]: the corrected data codewords, zero behind ndata
};
constexpr int DM_MAX_DATA_ALL = 1560;    // >= 1558, the data codewords of 144 x 144
constexpr int DM_MIN_MAX_SIZE = 52, DM_MAX_MAX_SIZE = 144;

bool dm_max_size_ok(int max_size);
// host only: the placement table of the side x side symbol (64 .. 144) as the second stage uses it, (row << 8 | col) per codeword bit
// -> the number of entries, 0 for another side or when cap is too small
int datamatrix_placement(int side, unsigned short* out, int cap);
size_t datamatrix_sizes_workspace_bytes(int B, int H, int W, int max_candidates, int max_codes);
hipError_t datamatrix_sizes_launch(const DmSizesParams& p, void* workspace, size_t ws_bytes, hipStream_t st);
bool dm_params_ok(int min_module, int max_module, int quiet, int timing_max, int solid_max, int max_candidates, int max_codes);
size_t datamatrix_workspace_bytes(int B, int H, int W, int max_candidates, int max_codes);
hipError_t datamatrix_launch(const DmParams& p, void* workspace, size_t ws_bytes, hipStream_t st);
