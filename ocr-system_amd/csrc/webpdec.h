// Lossless WebP (VP8L) decoder on the device: the pixel work behind the reference's
//   Image.open(path) / Image.open(io.BytesIO(bytes)) + convert('RGB')   (ImagePreprocessor.load_image / load_image_bytes,
//   image_preprocessing.py:57-75; .webp inputs)
// byte-identical to Pillow (libwebp).  The contract is the PNG decoder's: status 0 => the same bytes as Pillow's decode, any other status
// => the file is left to Pillow.  The lossy format (VP8 key frames, with or without an ALPH chunk) and animation are refused with -2.
#pragma once
#include <cstddef>

#include "common.h"

// bytes of workspace a sub-batch of n files of height x width with z_total staged stream bytes needs (the layout webpdec_run carves)
size_t webpdec_workspace_bytes(int n, int height, int width, size_t z_total);

struct lumina_ocr;
// files: HOST pointers; all n files must be height x width.  out: device RGB u8 [n][height][width][3] (alpha dropped: the stored RGB,
// not pre-multiplied).  status: HOST int [n], 0 ok / -1 corrupt / -2 unsupported / -4 size mismatch (such a page's pixels are not
// written).  Synchronous: synchronises the stream once per sub-batch.
int webpdec_run(lumina_ocr* eng, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev, int* status,
                hipStream_t st);
