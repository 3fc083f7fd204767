#pragma once
#include "runs.h"

// What the matrix-code readers (qrcodes.hip, datamatrix.hip, aztec.hip) agree on between their decode kernels and their output kernel.
//
// A decode kernel leaves one record of CODE_RES_INTS ints per slot of a page (a finder, a candidate), zeroed before it runs:
//   0 .. 4    the sort key y0, x0, y1, x1, root (the hull, then the run id that makes equal hulls distinct)
//   5 .. 12   the last eight ints of the symbol's 12-int row, as they are written out
//   13        the state: 0 nothing, CODE_ROW a symbol, CODE_PENDING left for the reader's next stage
//   14, 15    the reader's own
// The output kernel is one 256-thread work-group per page: code_output_rows, then code_output_data.
constexpr int CODE_RES_INTS = 16, CODE_RES_STATE = 13;
constexpr int CODE_ROW = 1, CODE_PENDING = 2;

template <int CAP>
struct CodeOutLds {
    static_assert((CAP & (CAP - 1)) == 0, "the capacity masks an index");
    int key[CAP * 5], slot[CAP], n;
};

// a page's rows (max_codes <= CAP): the CODE_ROW records of its nslots slots are counted, gathered into tmp [max_codes][6] = y0, x0, y1,
// x1, root, slot, rank-sorted by the key, and written as 12-int rows to out -> the number of rows, also written to *count (and nslots
// to *slot_count when given); s.slot[rank] is the slot of row `rank`.  A page with more slots than max_slots is not read; an
// overflowing list has no rows: its count is all that is reported.
template <int CAP>
__device__ __forceinline__ int code_output_rows(CodeOutLds<CAP>& s, const int* res, int nslots, int max_slots, int max_codes, int* tmp, int* out, int* count,
                                                int* slot_count) {
    if (threadIdx.x == 0) s.n = 0;
    __syncthreads();
    const int lim = nslots > max_slots ? 0 : nslots;
    for (int a = threadIdx.x; a < lim; a += 256) {
        const int* r = res + a * CODE_RES_INTS;
        if (r[CODE_RES_STATE] != CODE_ROW) continue;
        const int idx = atomicAdd(&s.n, 1);
        if (idx >= max_codes) continue;
        int* o = tmp + idx * 6;
        o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3]; o[4] = r[4]; o[5] = a;
    }
    __syncthreads();
    const int n = s.n;
    if (threadIdx.x == 0) {
        *count = n;
        if (slot_count) *slot_count = nslots;
    }
    if (n > max_codes) return n;
    int* slots = s.slot;
    rank_sort<5>(s.key, tmp, 6, n, [=](int i, int rank, const int (&k)[5]) {
        const int slot = clampi(tmp[i * 6 + 5], 0, max_slots - 1);
        const int* r = res + slot * CODE_RES_INTS;
        int* o = out + (size_t)rank * 12;
        o[0] = k[1]; o[1] = k[0]; o[2] = k[3]; o[3] = k[2];
        for (int j = 0; j < 8; ++j) o[4 + j] = r[5 + j];
        slots[rank & (CAP - 1)] = slot;
    });
    __syncthreads();
    return n;
}

// the n data rows of row_len elements behind code_output_rows, by the whole work-group: element j of row `rank` is fetch(slot, j), which
// also gives the zeros behind the symbol's data
template <int CAP, class T, class Fetch>
__device__ __forceinline__ void code_output_data(const CodeOutLds<CAP>& s, int n, int max_slots, int row_len, T* data, Fetch fetch) {
    for (int idx = threadIdx.x; idx < n * row_len; idx += 256) {
        const int rank = idx / row_len, j = idx - rank * row_len;
        data[idx] = fetch(clampi(s.slot[rank & (CAP - 1)], 0, max_slots - 1), j);
    }
}
