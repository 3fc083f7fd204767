#pragma once
#include "common.h"

// Page orientation on the device (orient.hip; definition restated in tests/page_orient_reference.py): whether a page lies sideways
// (ink profiles), pages turned by quarter turns, and the per-page vote of the text-line classifier.  Integer arithmetic throughout:
// the results do not depend on the order anything runs in.
struct QuarterParams {
    const uint8_t* rgb;       // [B][H][W][3]
    int B, H, W;
    int threshold;            // ink = L < threshold, L = Pillow's convert('L') (ink_mask, runs.hip)
    int ratio;                // sideways iff E_c > ratio * E_r
    long long* energies;      // device, [B][2] = E_r, E_c: sums of the squared differences of neighbouring row / column ink counts
    int* sideways;            // device, [B]: 0 / 1
};
constexpr int QUARTER_MAX_RATIO = 1024;   // ratio * E fits 64 bits with room: E <= 65534 * 65535^2 < 2^48

size_t quarter_workspace_bytes(int B, int H, int W);
hipError_t quarter_launch(const QuarterParams& p, void* workspace, size_t ws_bytes, hipStream_t st);

// out [m][H'][W'][3]: page j = np.rot90(pages[idx[j]], t), t in 0..3; (H', W') = (W, H) for odd t.  idx: device, m entries in 0..n-1
// (an entry outside that range leaves its page unwritten).
hipError_t page_turn_launch(const uint8_t* pages, int n, int H, int W, const int* idx, int m, int t, uint8_t* out, hipStream_t st);

// counts [B][2] = number of lines of each page, number of those whose flip flag is set.  page_idx: device, n entries (entries outside
// 0..B-1 are not counted).
hipError_t page_vote_launch(const int* flip, const int* page_idx, int n, int B, int* counts, hipStream_t st);
