// Strip-coded images on the device: the strips of a scanned TIFF page (utils/tiff_pages.py finds them) and PDF's /LZWDecode and
// /RunLengthDecode image streams (utils/pdf_pages.py; one strip a page).  A strip is an independent stream of whole packed rows coded
// with LZW (TIFF 6.0 / PDF flavour: MSB-first codes of 9..12 bits, early change), PackBits, or not at all.  The contract is the other
// decoders': status 0 => byte-identical to Pillow's Image.open(f).convert('RGB'), any other status => the page is left to Pillow.
#pragma once
#include <cstddef>

#include "common.h"

enum : int { LZ_CODEC_NONE = 1, LZ_CODEC_LZW = 5, LZ_CODEC_PACKBITS = 32773 };

// bytes of workspace a sub-batch of n pages in m strips with these totals needs (the layout strip_image_run carves)
size_t lzw_workspace_bytes(int n, int m, size_t in_total, size_t rows_total);

struct lumina_ocr;
// strips / sizes: HOST arrays of m strips, the strips of page 0 first, each page's in row order; strip_counts: HOST int [n], the number
// of strips of each page (their sum is m), -2 for a page whose count is not ceil(height / rows_per_strip).  All n pages are
// height x width with rows_per_strip rows a strip (the last strip of a page holds the rest).  params: HOST int [n][7] = {codec (1 none,
// 5 LZW, 32773 PackBits), predictor (1 | 2: horizontal differencing of 8-bit samples), components (1 | 3), bits per component (8;
// 1 / 2 / 4 with one component), indexed (0 | 1), invert (0 | 1: MinIsWhite, /Decode [1 0]; one non-indexed component), rle_eod (0 | 1:
// a PackBits header byte of 128 ends the data, as in /RunLengthDecode)}.  palettes: HOST, 768 bytes of RGB per indexed page (may be
// null without one).  out: device RGB u8 [n][height][width][3].  status: HOST int [n], the worst (lowest) of the page's strips:
//   0  every strip produced its rows x row bytes (codes or bytes after that are ignored; no EOI needed);
//  -1  corrupt: an LZW code above the next free entry, a code >= 258 right after Clear, a full table and a code other than Clear, EOI or
//      the end of the data before the strip is full, a PackBits literal or repeat that runs past the input, too few raw bytes;
//  -2  unsupported: a combination outside the list above, a wrong strip count, or an LZW strip whose first code is not Clear
//      (old-style LSB-first LZW among them).
// The pixels of a page with a non-zero status are undefined.  Synchronises the stream once per sub-batch.
int strip_image_run(lumina_ocr* eng, const uint8_t* const* strips, const size_t* sizes, int m, const int* strip_counts, int n, int height,
                    int width, int rows_per_strip, const int* params, const uint8_t* const* palettes, uint8_t* out_dev, int* status,
                    hipStream_t st);
