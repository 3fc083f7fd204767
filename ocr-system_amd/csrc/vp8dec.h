// Lossy WebP (VP8 key frame) decoder on the device: the pixel work behind the reference's
//   Image.open(path) / Image.open(io.BytesIO(bytes)) + convert('RGB')   (ImagePreprocessor.load_image / load_image_bytes,
//   image_preprocessing.py:57-75; .webp inputs)
// byte-identical to Pillow (libwebp), for lossy and lossless files in one batch.  The contract is webpdec.h's: status 0 => the same bytes
// as Pillow's decode, any other status => the file is left to Pillow.  A lossy file with an ALPH chunk and animation are refused with -2.
#pragma once
#include <cstddef>

#include "common.h"

// bytes of workspace a sub-batch of n lossy files of height x width with z_total staged stream bytes needs (the layout vp8dec_run
// carves: macroblock records, coefficient plane, the padded Y, U and V planes)
size_t vp8dec_workspace_bytes(int n, int height, int width, size_t z_total);

// host only: the probe of both kinds (vp8_parse.h); info as lumina_ocr_webp_probe_lossy documents it
int vp8dec_probe(const uint8_t* file, size_t size, int info[8], const char** reason);

struct lumina_ocr;
// files: HOST pointers; all n files must be height x width.  out: device RGB u8 [n][height][width][3].  status: HOST int [n], 0 ok /
// -1 corrupt / -2 unsupported / -4 size mismatch (such a page's pixels are not written).  Lossless files go through webpdec_run.
// Synchronous: synchronises the stream once per sub-batch.
int vp8dec_run(lumina_ocr* eng, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev, int* status,
               hipStream_t st);
