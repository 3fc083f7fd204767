#pragma once
#include "common.h"

// Selection marks (checkboxes) of a batch of pages, on the device (marks.hip; definition restated in tests/mark_reference.py).
// Integer arithmetic throughout: the result does not depend on the order anything runs in.
struct MarkParams {
    const uint8_t* rgb;   // [B][H][W][3]
    int B, H, W;
    int threshold;        // ink = L < threshold, L = Pillow's convert('L')
    int min_side;         // a candidate's bounding box has min_side <= w, h <= max_side (and 4 |w - h| <= min(w, h))
    int max_side;         // <= MARK_MAX_SIDE: a candidate's window is one 64-bit word per row, one lane per row
    int max_marks;        // capacity of a page's list (<= MARK_MAX_MARKS)
    int* marks;           // device, [B][max_marks][8] = x0, y0, x1, y1, edge, ink_in, area_in, state; sorted by (y0, x0, y1, x1, root)
    int* counts;          // device, [B]: true number of marks (a list is not written when it overflows)
    unsigned long long* mask_out;        // optional parity hook: ink mask [B][H][ceil(W / 64)], bit x % 64 of word x / 64
    const unsigned long long* mask_in;   // optional: the ink mask of these pages at this threshold, already computed (ink_mask_launch, runs.h)
    // optional, both or neither: the round marks (radio buttons) of the same components, in the same row format and order.  Null: the
    // pass is the one without them (same kernels, same workspace layout)
    int* rounds;          // device, [B][max_marks][8]
    int* round_counts;    // device, [B]
    int out_max;          // ink pixels allowed beyond the outer circle
    int ring_div;         // the ring zone is T = 1 + max(w, h) / ring_div pixels deep
    int band_div;         // the clear band around the box is band_min + min(w, h) / band_div pixels wide (<= 32: one lane per band row)
    int band_min;
};
constexpr int MARK_MAX_SIDE = 64;
constexpr int MARK_MIN_SIDE = 4;
constexpr int MARK_MAX_MARKS = 2048;

constexpr int ROUND_MIN_BAND_DIV = 4;    // band <= ROUND_MAX_BAND_MIN + MARK_MAX_SIDE / ROUND_MIN_BAND_DIV = 32
constexpr int ROUND_MAX_BAND_MIN = 16;

bool round_params_ok(int out_max, int ring_div, int band_div, int band_min);
size_t marks_workspace_bytes(int B, int H, int W, int max_marks, bool rounds = false);
hipError_t marks_launch(const MarkParams& p, void* workspace, size_t ws_bytes, hipStream_t st);
