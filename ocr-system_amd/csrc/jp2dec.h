// JPEG 2000 decoder on the device: the pixel work behind the reference's Image.open(...).convert('RGB') for .jp2 / .j2k inputs and
// the /JPXDecode pages of scanned PDFs, byte-identical to Pillow (OpenJPEG).  The contract is the JPEG decoder's: status 0 => the
// same bytes as Pillow's decode, any other status => the file is left to Pillow.
//
// Read: a raw codestream or a JP2 / JPX-baseline file; one tile, origin 0, 1 or 3 components of 8 unsigned bits, no sub-sampling;
// the 5/3 reversible transform with 0-6 levels, lossless or cut short by up to 32 quality layers, any progression order, one
// precinct per resolution, code-blocks up to 64 x 64, code-block style 0, with or without the reversible colour transform.
// Everything else (9/7, tiles, precincts ...) is refused with -2; anything irregular with -1.
//
// With `irreversible` the 9/7 irreversible transform is read as well: expounded step sizes (QCD style 2), up to 15 magnitude
// bit-planes a sub-band (OpenJPEG's files of up to 5 levels), no line of one sample above resolution 0.  Its float arithmetic is
// OpenJPEG's operation for operation, so the contract stands: status 0 => Pillow's bytes.  Without it a 9/7 file is -2 as before.
//
// With JP2_TAKE_TILES (flags; JP2_TAKE_IRREVERSIBLE is the option above) tiled files are read too: image and tile origins, up to 4096
// tiles with their tile-parts in any order, user precinct sizes, all five progression orders over several precincts.  height and
// width are those of the image area.  Still -2: SOP / EPH, POC, coding parameters in a tile-part header, PPM / PPT, sub-sampled
// components, more than 4096 tiles.
#pragma once
#include <cstddef>

#include "common.h"

struct Jp2Probe { int info[8]; const char* reason; };
// Host only: boxes, headers and the walk over every packet header (tier 2); no pixel is decoded.  info = {width, height, components,
// levels, layers, progression order, code-block width, code-block height}.  0 / -1 / -2 as above; reason: a static string.
int jp2dec_probe(const uint8_t* file, size_t n, Jp2Probe* out, unsigned flags = 0);

// bytes of workspace a sub-batch needs: nblocks code-blocks with nbytes of coded data, planes component planes of height x width
// cut into tile_components tile-components in all
size_t jp2dec_workspace_bytes(size_t nblocks, size_t nbytes, int pages, size_t planes, int height, int width, size_t tile_components);

struct lumina_ocr;
// files: HOST pointers; all n files must be height x width.  out: device RGB u8 [n][height][width][3] (grey files: the grey value on
// all three channels).  status: HOST int [n], 0 ok / -1 corrupt / -2 unsupported / -4 size mismatch (such a page's pixels are not
// written).  Synchronous: synchronises the stream once per sub-batch.
int jp2dec_run(lumina_ocr* eng, const uint8_t* const* files, const size_t* sizes, int n, int height, int width, uint8_t* out_dev, int* status,
               hipStream_t st, unsigned flags = 0);
