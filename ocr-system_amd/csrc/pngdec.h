// Baseline PNG decoder on the device: the pixel work behind the reference's
//   Image.open(path) / Image.open(io.BytesIO(bytes)) + convert('RGB')   (ImagePreprocessor.load_image / load_image_bytes,
//   image_preprocessing.py:57-75; .png inputs, and the PNG pages pdf2image returns for PDFs)
// byte-identical to Pillow.  The contract is the JPEG decoder's: status 0 => the same bytes as Pillow's decode, any other status =>
// the file is left to Pillow.  The device accepts a file only where every conformant decoder agrees.
#pragma once
#include <cstddef>

#include "common.h"

struct PdInfo { int width, height, color_type, bit_depth, interlace, palette_size, orientation; };
// Host only, a walk over the chunks before the first IDAT (no pixel data is read): 0 = a file the device decodes (non-interlaced;
// grey 1/2/4/8 bit, RGB 8, palette 1/2/4/8, grey+alpha 8, RGBA 8), -1 = not a PNG / corrupt header chunks, -2 = valid but outside that
// subset.  orientation: the EXIF Orientation of an eXIf chunk before IDAT (0 without one).
int pngdec_probe(const uint8_t* file, size_t n, PdInfo* info);

// bytes of workspace a batch of n files with these totals needs (the layout pngdec_run carves)
size_t pngdec_workspace_bytes(int n, size_t z_total, size_t filt_total, size_t adler_blocks);

struct lumina_ocr;
// files: HOST pointers; all n files must be height x width.  out: device RGB u8 [n][height][width][3] (grey files: the grey value on
// all three channels).  status: HOST int [n], 0 ok / -1 corrupt / -2 unsupported / -4 size mismatch (such a page's pixels are not
// written).  Synchronous: synchronises the stream once per sub-batch.
int pngdec_run(lumina_ocr* eng, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev, int* status,
               hipStream_t st);

// The image streams of PDF's /FlateDecode: plain zlib streams of height rows (a scanned page is one such image).  The batch contract
// is pngdec_run's and so are the inflate and Adler-32 stages; the row stage depends on /Predictor.  params: HOST int [n][5] =
// {Predictor (1: packed rows; 2: TIFF horizontal differencing, 8-bit samples; 10..15: PNG row filters), components (1 | 3), bits per
// component (8; 1 / 2 / 4 with one component), indexed (0 | 1: the sample is an index into palettes[i]), invert (/Decode [1 0], one
// non-indexed component)}.  palettes: HOST, 768 bytes of RGB per indexed stream (entries past /hival filled by the caller; may be null
// when no stream is indexed).  status: 0 exact pixels / -1 corrupt (zlib header, DEFLATE stream, Adler-32, a PNG filter byte past 4, or
// an inflated length other than rows x row bytes) / -2 a combination outside this list.
int flate_image_run(lumina_ocr* eng, const uint8_t* const* streams, const size_t* sizes, int n, int height, int width, const int* params,
                    const uint8_t* const* palettes, uint8_t* out_dev, int* status, hipStream_t st);

// One image of a sub-batch as the device stages see it.  The row stage below reads width .. out_index, fb .. pal and foff.
struct PdFile {
    unsigned long long zoff, foff;   // byte offsets of the zlib stream / the filtered scanlines in the sub-batch's buffers
    unsigned zlen, rb, total;        // stream bytes; bytes per row (filter byte excluded); inflated bytes = height * (rb + fb)
    int width, height, ct, depth, bpp, npal, wsize, valid, out_index, ablk_off;
    int fb, tiff, invert;            // filter bytes per row (1: PNG rows; 0: packed rows of a PDF Flate image); /Predictor 2 rows; /Decode [1 0]
    uint8_t pal[768];
};

// The row stage both flate_image_run and strip_image_run (lzw.h) end with: rows at rows + F[k].foff (F[k].rb + F[k].fb bytes each) ->
// out_dev[F[k].out_index] as RGB; pd_tiff_predict first where any_tiff (the F[k].tiff images).  F, rows, err: device; images with
// err[k] != 0 or !valid are skipped.  Launches only.
void pd_rows_to_rgb(const PdFile* F, uint8_t* rows, const int* err, int nb, int height, int width, bool any_tiff, uint8_t* out_dev, hipStream_t st);
