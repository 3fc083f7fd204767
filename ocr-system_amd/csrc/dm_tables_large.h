#pragma once
// Written by lumina_ocr.utils.datamatrix.device_header_large(); tests/test_dm_sizes_tables.py compares.  Data Matrix ECC 200, the
// nine squares of 64 x 64 .. 144 x 144.  DML_SIZES: rows, cols, data codewords, check codewords, region rows, region cols,
// interleaved blocks, 0 of every size (DML_SIZES_HOST: the same for the host).  DML_PLACE: (row << 8 | col) of every codeword bit
// in placement order, the most significant bit of a codeword first, size s at DML_PLACE_OFF[s] .. DML_PLACE_OFF[s + 1]; global
// memory that datamatrix.hip fills once a device from the standard's walk (dml_placement there) and that no kernel writes.
constexpr int DML_NUM_SIZES = 9, DML_PLACE_N = 79264;
#define DML_SIZE_ROWS \
    64, 64, 280, 112, 4, 4, 2, 0, \
    72, 72, 368, 144, 4, 4, 4, 0, \
    80, 80, 456, 192, 4, 4, 4, 0, \
    88, 88, 576, 224, 4, 4, 4, 0, \
    96, 96, 696, 272, 4, 4, 4, 0, \
    104, 104, 816, 336, 4, 4, 6, 0, \
    120, 120, 1050, 408, 6, 6, 6, 0, \
    132, 132, 1304, 496, 6, 6, 8, 0, \
    144, 144, 1558, 620, 6, 6, 10, 0
__device__ const unsigned short DML_SIZES[DML_NUM_SIZES * 8] = {DML_SIZE_ROWS};
static const unsigned short DML_SIZES_HOST[DML_NUM_SIZES * 8] = {DML_SIZE_ROWS};
#define DML_PLACE_OFFSETS 0, 3136, 7232, 12416, 18816, 26560, 35776, 47440, 61840, 79264
__device__ const int DML_PLACE_OFF[DML_NUM_SIZES + 1] = {DML_PLACE_OFFSETS};
static const int DML_PLACE_OFF_HOST[DML_NUM_SIZES + 1] = {DML_PLACE_OFFSETS};
__device__ unsigned short DML_PLACE[DML_PLACE_N];
