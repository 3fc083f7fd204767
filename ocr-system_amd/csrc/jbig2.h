// JBIG2 (ITU-T T.88) on the device, generic-region subset: the pixel work behind PDF's /JBIG2Decode for bilevel scans whose pages are
// coded as generic regions (jbig2enc without symbol coding, which is OCRmyPDF's lossless default, and striped device output), and for
// the stencils and masks of layered pages.  Symbol dictionaries, text, halftone and refinement regions are told apart and refused.
#pragma once
#include <cstddef>

#include "common.h"

struct lumina_ocr;
struct Jb2Page;
// host only: jbig2_parse (jbig2_parse.h) behind a name that needs no parser header
int jbig2_probe(const uint8_t* stream, size_t size, const uint8_t* globals, size_t globals_size, Jb2Page* page);
// streams / globals: HOST pointers to n page streams and their /JBIG2Globals streams (globals or any entry of it may be null), every
// page height x width.  params: HOST int [n][1] = {invert}.  out: device RGB u8 [n][height][width][3], PDF's convention: bit 1 is black
// (0) and bit 0 white (255) unless invert.  status: HOST int [n], 0 ok / -1 corrupt / -2 valid JBIG2 outside the subset / -4 another
// size than the batch; a page with a non-zero status is not written.  Synchronises the stream.
int jbig2_run(lumina_ocr* eng, const uint8_t* const* streams, const size_t* sizes, const uint8_t* const* globals, const size_t* globals_sizes,
              int n, int height, int width, const int* params, uint8_t* out_dev, int* status, hipStream_t st);
