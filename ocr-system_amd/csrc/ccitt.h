// CCITT Group 4 (ITU-T T.6) on the device: the pixel work behind PDF's /CCITTFaxDecode with K < 0, the coding of almost every
// black-and-white scan.  A scanned PDF page is one such image; the provider hands its stream here instead of rasterising the page
// (the reference renders PDF pages with pdf2image / poppler, ocr_service.py:508-660).
#pragma once
#include <cstddef>

#include "common.h"

constexpr int CC_MAX_COLS = 8192;   // widest line the decoder takes (its two changing-element arrays are u16 in LDS): A3 at 600 dpi is 7016

struct lumina_ocr;
// streams: HOST pointers to n T.6 streams, all rows x columns.  params: HOST int [n][4] = {K, EncodedByteAlign, BlackIs1, invert}
// (invert: /Decode [1 0]).  out: device RGB u8 [n][rows][columns][3], PDF's convention: a coded-white run is sample 1 unless BlackIs1,
// sample 1 is white (255) unless invert.  status: HOST int [n], 0 ok / -1 corrupt (an unused code, a0 that does not advance, a run past
// the line's end, a pass code whose b2 is the line's end, more than columns + 1 changing elements on a line, bits past the stream's end, fewer than `rows` lines) /
// -2 unsupported (K >= 0, EncodedByteAlign, columns > CC_MAX_COLS).  Decoding stops after `rows` lines or at EOFB; bytes after that are
// ignored.  The pixels of a page with a non-zero status are undefined.  Synchronises the stream.
int ccitt_run(lumina_ocr* eng, const uint8_t* const* streams, const size_t* sizes, int n, int rows, int columns, const int* params,
              uint8_t* out_dev, int* status, hipStream_t st);
