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

// Group 3 and CCITT RLE (ITU-T T.4) beside it: what fax servers write (TIFF-F: Compression 3, and Compression 2) and PDF's
// /CCITTFaxDecode with K >= 0.  params: HOST int [n][5] = {K, EncodedByteAlign, BlackIs1, invert, path}; everything else as ccitt_run.
// K < 0 is Group 4 and takes ccitt_run's kernel unchanged (EncodedByteAlign then -2, as there).  K = 0: every line one-dimensional.
// K > 0: the bit after each EOL says whether the line is one- or two-dimensional (the value of K itself is the encoder's business).
// The decoder finds EOLs by itself: at each line's start it skips zero bits, and 11 or more of them followed by a 1 are an EOL, so fill
// bits (T4Options bit 2, of any length) need no flag; a stream has an EOL in front of every line or of none, which its first line
// decides.  EncodedByteAlign: in a stream without EOLs every line begins on a byte boundary (TIFF Compression 2; PDF /K 0 with
// /EncodedByteAlign true).  Decoding stops after `rows` lines: an RTC, fill or anything else behind them is ignored.
// path: 0 automatic, 1 the serial walk (one wave a stream); 2 is reserved for a line-parallel decode and answers -2.
// status 0: exact pixels.  -1 corrupt, which is everything irregular (libtiff on the host is lenient, the device is not): an unused
// code; a line whose runs do not add up to `columns` exactly; a run of length 0 other than a line's first; what ccitt_run refuses in
// a two-dimensional line; an EOL in front of some lines and not of others; two EOLs in a row before `rows` lines; bits other than 0
// between a line's end and the next EOL; bits past the stream's end.  -2 unsupported: K > 0 in a stream without EOLs (PDF allows it,
// libtiff cannot express it, so nothing can serve as its oracle), EncodedByteAlign in a stream with EOLs (the same), a path other than
// 0 and 1, columns > CC_MAX_COLS.  T.4's uncompressed mode has no code here and ends as an unused code.
int fax_run(lumina_ocr* eng, const uint8_t* const* streams, const size_t* sizes, int n, int rows, int columns, const int* params,
            uint8_t* out_dev, int* status, hipStream_t st);
