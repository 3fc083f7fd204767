#pragma once
#include "common.h"

// Rules (long thin ink lines) of ruled tables on a batch of pages, on the device (tables.hip; definition restated in
// tests/table_reference.py).  Integer arithmetic throughout: the result does not depend on the order anything runs in.
struct TableParams {
    const uint8_t* rgb;   // [B][H][W][3]
    int B, H, W;
    int threshold;        // ink = L < threshold, L = Pillow's convert('L')
    int gap;              // runs of one line at most this many non-ink pixels apart merge
    int min_len;          // shortest merged run kept, shortest rule
    int max_thick;        // a component is a rule when area <= max_thick * length
    int max_rules;        // capacity of each list per page (<= TABLE_MAX_RULES)
    int* hrules;          // device, [B][max_rules][5] = x0, y0, x1, y1, area; sorted by (y0, x0, y1, x1)
    int* vrules;          // device, [B][max_rules][5], sorted by (x0, y0, x1, y1)
    int* counts;          // device, [B][2]: true number of horizontal / vertical rules (a list is not written when it overflows)
    unsigned long long* hmask_out;   // optional parity hook: ink mask [B][H][ceil(W / 64)], bit x % 64 of word x / 64
    const unsigned long long* hmask_in;   // optional: the ink mask of these pages at this threshold, already computed (ink_mask_launch, runs.h)
};
constexpr int TABLE_MAX_RULES = 2048;

size_t table_workspace_bytes(int B, int H, int W, int gap, int min_len, int max_rules);
hipError_t table_rules_launch(const TableParams& p, void* workspace, size_t ws_bytes, hipStream_t st);
