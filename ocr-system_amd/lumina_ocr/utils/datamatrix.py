"""Data Matrix, host half (pure Python): the tables of the ECC 200 sizes whose rows fit one 64-bit word (SIZES) and of the nine larger
squares up to 144 x 144 (LARGE_SIZES; ALL_SIZES is both, and every size index below is one of ALL_SIZES), the corrected data codewords
of a device row (lumina_ocr_datamatrix: x0, y0, x1, y1, rows, cols, ndata, errors, rotation, timing mismatches, L misses, 0 + the
codewords) -> text, and the entries the provider reports.

The tables are our reading of the public standard (ISO/IEC 16022), built from its rules: the L finder, the clock tracks and the
alignment bars between data regions make the function masks; the diagonal walk with its four corner cases and the fixed 2 x 2
corner gives the placement; the size table is typed and pinned by modules = 8 (data + check) + remainder (tests/test_dm_tables.py).
csrc/dm_tables.h holds the same tables for the device (device_header() writes it; the test compares), csrc/dm_tables_large.h those
of the larger squares without the placement, which the library builds itself (device_header_large()).

Coordinates: a module is (row, col), row 0 the clock track opposite the L's foot, col 0 the L's upright; a row of modules is one
64-bit word, bit col.  The DATA-REGION MATRIX is the symbol without its function modules, regions pushed together."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

# rows, cols, data codewords, check codewords, region rows, region cols, interleaved blocks
SIZES = ((10, 10, 3, 5, 1, 1, 1), (12, 12, 5, 7, 1, 1, 1), (14, 14, 8, 10, 1, 1, 1), (16, 16, 12, 12, 1, 1, 1), (18, 18, 18, 14, 1, 1, 1),
         (20, 20, 22, 18, 1, 1, 1), (22, 22, 30, 20, 1, 1, 1), (24, 24, 36, 24, 1, 1, 1), (26, 26, 44, 28, 1, 1, 1), (32, 32, 62, 36, 2, 2, 1),
         (36, 36, 86, 42, 2, 2, 1), (40, 40, 114, 48, 2, 2, 1), (44, 44, 144, 56, 2, 2, 1), (48, 48, 174, 68, 2, 2, 1), (52, 52, 204, 84, 2, 2, 2),
         (8, 18, 5, 7, 1, 1, 1), (8, 32, 10, 11, 1, 2, 1), (12, 26, 16, 14, 1, 1, 1), (12, 36, 22, 18, 1, 2, 1), (16, 36, 32, 24, 1, 2, 1),
         (16, 48, 49, 28, 1, 2, 1))
NUM_SIZES = len(SIZES)
MAX_DATA = 208                         # ints a device data row holds (>= 204, the data codewords of 52 x 52)
MAX_CODEWORDS = 288
MAX_BLOCK_LEN, MAX_EC = 242, 68        # 48 x 48: one block of 174 + 68

# The nine larger squares (lumina_ocr_datamatrix_sizes reads them): 4 x 4 or 6 x 6 regions, two to ten interleaved blocks.  The rows are
# written from recollection of the standard; what pins them is structural (data + check = mapping area / 8, tests/test_dm_sizes_tables.py)
# and this project's own encoder.  The codeword at stream position p (data, then check) belongs to block p mod blocks: 144 x 144 has
# 1558 data codewords in ten blocks, eight of 156 + 62 and two of 155 + 62, so its check codewords carry on from block 8.
LARGE_SIZES = ((64, 64, 280, 112, 4, 4, 2), (72, 72, 368, 144, 4, 4, 4), (80, 80, 456, 192, 4, 4, 4), (88, 88, 576, 224, 4, 4, 4),
               (96, 96, 696, 272, 4, 4, 4), (104, 104, 816, 336, 4, 4, 6), (120, 120, 1050, 408, 6, 6, 6), (132, 132, 1304, 496, 6, 6, 8),
               (144, 144, 1558, 620, 6, 6, 10))
ALL_SIZES = SIZES + LARGE_SIZES        # a size index of the functions below is an index into this
NUM_SIZES_ALL = len(ALL_SIZES)
MAX_DATA_ALL = 1560                    # bytes a device data row of lumina_ocr_datamatrix_sizes holds (>= 1558)
MAX_CODEWORDS_ALL = 2178
MAX_BLOCKS_ALL, MAX_BLOCK_LEN_ALL = 10, 243   # 120 x 120: six blocks of 175 + 68
MIN_MAX_SIZE, MAX_MAX_SIZE = 52, 144   # lumina_ocr_datamatrix_sizes' max_size


def size_index(rows: int, cols: int) -> int:
    """-> index into SIZES, or -1."""
    for i, s in enumerate(SIZES):
        if s[0] == rows and s[1] == cols:
            return i
    return -1


def size_index_all(rows: int, cols: int) -> int:
    """-> index into ALL_SIZES, or -1."""
    for i, s in enumerate(ALL_SIZES):
        if s[0] == rows and s[1] == cols:
            return i
    return -1


def mapping_dims(size: int) -> Tuple[int, int]:
    """Rows and columns of the data-region matrix."""
    r, c, _, _, nr, nc, _ = ALL_SIZES[size]
    return r - 2 * nr, c - 2 * nc


def remainder_modules(size: int) -> int:
    nrow, ncol = mapping_dims(size)
    return nrow * ncol - 8 * (ALL_SIZES[size][2] + ALL_SIZES[size][3])


def block_lengths(size: int) -> List[Tuple[int, int]]:
    """-> [(data, check)] of every interleaved block: block b takes the stream positions b, b + nb, ..., its last ne / nb are check."""
    _, _, nd, ne, _, _, nb = ALL_SIZES[size]
    return [(len(range(b, nd + ne, nb)) - ne // nb, ne // nb) for b in range(nb)]


# ---- GF(256), polynomial 0x12D: EXP has 512 entries so that EXP[LOG[a] + LOG[b]] needs no reduction ----
GF_POLY = 0x12D


def _gf_tables() -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    exp, log, x = [0] * 512, [0] * 256, 1
    for i in range(255):
        exp[i], log[x] = x, i
        x <<= 1
        if x & 0x100:
            x ^= GF_POLY
    for i in range(255, 512):
        exp[i] = exp[i - 255]
    return tuple(exp), tuple(log)


GF_EXP, GF_LOG = _gf_tables()


def gf_mul(a: int, b: int) -> int:
    return GF_EXP[GF_LOG[a] + GF_LOG[b]] if a and b else 0


def rs_generator(ec: int) -> List[int]:
    """(x - a^1) ... (x - a^ec), descending powers, the leading 1 first."""
    gen = [1]
    for i in range(1, ec + 1):
        gen = [a ^ gf_mul(b, GF_EXP[i]) for a, b in zip(gen + [0], [0] + gen)]
    return gen


# ---- function modules ----
def function_modules(size: int) -> Dict[Tuple[int, int], bool]:
    """-> {(row, col): dark} of every function module: of each data region the solid left column and bottom row (the L and the inner
    solid bars), the clock row above it (dark on even columns) and the clock column to its right (dark on odd rows)."""
    rows, cols, _, _, nr, nc, _ = ALL_SIZES[size]
    rh, rw = rows // nr, cols // nc
    f: Dict[Tuple[int, int], bool] = {}
    for r in range(rows):
        for c in range(cols):
            lr, lc = r % rh, c % rw
            if lc == 0 or lr == rh - 1:
                f[(r, c)] = True
            elif lr == 0:
                f[(r, c)] = c % 2 == 0
            elif lc == rw - 1:
                f[(r, c)] = r % 2 == 1
    return f


def function_masks(size: int) -> Tuple[List[int], List[int], List[int]]:
    """-> (solid, clock, clock_dark): row words, bit col set where (row, col) is a module of the L or an inner solid bar / of a clock
    track or an inner clock bar / a dark one of those."""
    rows, cols, _, _, nr, nc, _ = ALL_SIZES[size]
    rh, rw = rows // nr, cols // nc
    solid, clock, dark = [0] * rows, [0] * rows, [0] * rows
    for (r, c), d in function_modules(size).items():
        if c % rw == 0 or r % rh == rh - 1:
            solid[r] |= 1 << c
        else:
            clock[r] |= 1 << c
            dark[r] |= int(d) << c
    return solid, clock, dark


# ---- placement ----
def _corner(case: int, nrow: int, ncol: int) -> List[Tuple[int, int]]:
    return {1: [(nrow - 1, 0), (nrow - 1, 1), (nrow - 1, 2), (0, ncol - 2), (0, ncol - 1), (1, ncol - 1), (2, ncol - 1), (3, ncol - 1)],
            2: [(nrow - 3, 0), (nrow - 2, 0), (nrow - 1, 0), (0, ncol - 4), (0, ncol - 3), (0, ncol - 2), (0, ncol - 1), (1, ncol - 1)],
            3: [(nrow - 3, 0), (nrow - 2, 0), (nrow - 1, 0), (0, ncol - 2), (0, ncol - 1), (1, ncol - 1), (2, ncol - 1), (3, ncol - 1)],
            4: [(nrow - 1, 0), (nrow - 1, ncol - 1), (0, ncol - 3), (0, ncol - 2), (0, ncol - 1), (1, ncol - 3), (1, ncol - 2), (1, ncol - 1)]}[case]


_UTAH = ((-2, -2), (-2, -1), (-1, -2), (-1, -1), (-1, 0), (0, -2), (0, -1), (0, 0))


def mapping_placement(nrow: int, ncol: int) -> Tuple[List[List[Tuple[int, int]]], List[int], List[Tuple[Tuple[int, int], bool]]]:
    """The standard's walk over the data-region matrix -> (for every codeword the (row, col) of its bits, the most significant first;
    the corner cases used, in the order met; the fixed modules [((row, col), dark)] of the 2 x 2 corner where the walk leaves it)."""
    seen: Dict[Tuple[int, int], int] = {}
    words: List[List[Tuple[int, int]]] = []
    corners: List[int] = []

    def wrap(r: int, c: int) -> Tuple[int, int]:
        if r < 0:
            r, c = r + nrow, c + 4 - ((nrow + 4) % 8)
        if c < 0:
            r, c = r + 4 - ((ncol + 4) % 8), c + ncol
        return r, c

    def put(cells: List[Tuple[int, int]]) -> None:
        for rc in cells:
            assert 0 <= rc[0] < nrow and 0 <= rc[1] < ncol and rc not in seen, (nrow, ncol, rc)
            seen[rc] = len(words)
        words.append(cells)

    row, col = 4, 0
    while True:
        for case, hit in ((1, row == nrow and col == 0), (2, row == nrow - 2 and col == 0 and ncol % 4 != 0),
                          (3, row == nrow - 2 and col == 0 and ncol % 8 == 4), (4, row == nrow + 4 and col == 2 and ncol % 8 == 0)):
            if hit:
                corners.append(case)
                put(_corner(case, nrow, ncol))
        while True:                                        # up and to the right
            if row < nrow and col >= 0 and (row, col) not in seen:
                put([wrap(row + dr, col + dc) for dr, dc in _UTAH])
            row, col = row - 2, col + 2
            if not (row >= 0 and col < ncol):
                break
        row, col = row + 1, col + 3
        while True:                                        # down and to the left
            if row >= 0 and col < ncol and (row, col) not in seen:
                put([wrap(row + dr, col + dc) for dr, dc in _UTAH])
            row, col = row + 2, col - 2
            if not (row < nrow and col >= 0):
                break
        row, col = row + 3, col + 1
        if not (row < nrow or col < ncol):
            break
    fixed = []
    if (nrow - 1, ncol - 1) not in seen:
        fixed = [((nrow - 1, ncol - 1), True), ((nrow - 2, ncol - 2), True), ((nrow - 1, ncol - 2), False), ((nrow - 2, ncol - 1), False)]
    return words, corners, fixed


def to_symbol(size: int, r: int, c: int) -> Tuple[int, int]:
    """Data-region matrix (r, c) -> symbol (row, col): the function modules of every region are stepped over."""
    rows, cols, _, _, nr, nc, _ = ALL_SIZES[size]
    dh, dw = rows // nr - 2, cols // nc - 2
    return r + 1 + 2 * (r // dh), c + 1 + 2 * (c // dw)


def placement(size: int) -> List[Tuple[int, int]]:
    """-> the symbol (row, col) of every codeword bit in placement order: bit b of codeword k at [8 k + b], the most significant first."""
    words, _, _ = mapping_placement(*mapping_dims(size))
    return [to_symbol(size, r, c) for w in words for r, c in w]


def corner_cases(size: int) -> List[int]:
    return mapping_placement(*mapping_dims(size))[1]


def fixed_modules(size: int) -> List[Tuple[Tuple[int, int], bool]]:
    """The 2 x 2 corner of the 4-module remainder in symbol coordinates, [((row, col), dark)]."""
    return [(to_symbol(size, r, c), d) for (r, c), d in mapping_placement(*mapping_dims(size))[2]]


_PLACEMENT = tuple(tuple(placement(s)) for s in range(NUM_SIZES))


_PLACEMENT_LARGE: Dict[int, Tuple[Tuple[int, int], ...]] = {}


def placement_of(size: int) -> Tuple[Tuple[int, int], ...]:
    if size < NUM_SIZES:
        return _PLACEMENT[size]
    if size not in _PLACEMENT_LARGE:                       # (79 264 bits in all: built when first asked for)
        _PLACEMENT_LARGE[size] = tuple(placement(size))
    return _PLACEMENT_LARGE[size]


def device_header() -> str:
    """The text of csrc/dm_tables.h."""
    rows = lambda v, f, per: ",\n".join("    " + ", ".join(f % x for x in v[i:i + per]) for i in range(0, len(v), per))
    place, off = [], [0]
    for s in range(NUM_SIZES):
        place += [(r << 6) | c for r, c in _PLACEMENT[s]]
        off.append(len(place))
    sizes = [x for s in SIZES for x in s + (0,)]
    return ("#pragma once\n// Written by lumina_ocr.utils.datamatrix.device_header(); tests/test_dm_tables.py compares.  Data Matrix ECC 200, the sizes\n"
            "// whose rows fit a 64-bit word.  DM_SIZES: rows, cols, data codewords, check codewords, region rows, region cols, interleaved\n"
            "// blocks, 0 of every size.  DM_PLACE: (row << 6 | col) of every codeword bit in placement order, the most significant bit of a\n"
            "// codeword first, size s at DM_PLACE_OFF[s] .. DM_PLACE_OFF[s + 1].  DM_EXP / DM_LOG: GF(256), polynomial 0x12D, EXP doubled.\n"
            "constexpr int DM_NUM_SIZES = %d, DM_PLACE_N = %d;\n"
            "__device__ const unsigned char DM_SIZES[DM_NUM_SIZES * 8] = {\n%s};\n"
            "__device__ const unsigned short DM_PLACE[DM_PLACE_N] = {\n%s};\n"
            "__device__ const int DM_PLACE_OFF[DM_NUM_SIZES + 1] = {\n%s};\n"
            "__device__ const unsigned char DM_EXP[512] = {\n%s};\n"
            "__device__ const unsigned char DM_LOG[256] = {\n%s};\n"
            % (NUM_SIZES, len(place), rows(sizes, "%d", 16), rows(place, "0x%03x", 16), rows(off, "%d", 11), rows(list(GF_EXP), "%d", 32),
               rows(list(GF_LOG), "%d", 32)))


def device_header_large() -> str:
    """The text of csrc/dm_tables_large.h.  The placement table itself (79 264 entries) is not written out: datamatrix.hip builds it
    on the host with the walk of mapping_placement and copies it to DML_PLACE once a device; lumina_ocr_datamatrix_placement returns
    what it built and tests/test_dm_sizes_tables.py compares that with placement_of."""
    rows = lambda v, f, per: ",\n".join("    " + ", ".join(f % x for x in v[i:i + per]) for i in range(0, len(v), per))
    off = [0]
    for s in LARGE_SIZES:
        off.append(off[-1] + 8 * (s[2] + s[3]))
    sizes = [x for s in LARGE_SIZES for x in s + (0,)]
    return ("#pragma once\n// Written by lumina_ocr.utils.datamatrix.device_header_large(); tests/test_dm_sizes_tables.py compares.  Data Matrix ECC 200, the\n"
            "// nine squares of 64 x 64 .. 144 x 144.  DML_SIZES: rows, cols, data codewords, check codewords, region rows, region cols,\n"
            "// interleaved blocks, 0 of every size (DML_SIZES_HOST: the same for the host).  DML_PLACE: (row << 8 | col) of every codeword bit\n"
            "// in placement order, the most significant bit of a codeword first, size s at DML_PLACE_OFF[s] .. DML_PLACE_OFF[s + 1]; global\n"
            "// memory that datamatrix.hip fills once a device from the standard's walk (dml_placement there) and that no kernel writes.\n"
            "constexpr int DML_NUM_SIZES = %d, DML_PLACE_N = %d;\n"
            "#define DML_SIZE_ROWS \\\n%s\n"
            "__device__ const unsigned short DML_SIZES[DML_NUM_SIZES * 8] = {DML_SIZE_ROWS};\n"
            "static const unsigned short DML_SIZES_HOST[DML_NUM_SIZES * 8] = {DML_SIZE_ROWS};\n"
            "#define DML_PLACE_OFFSETS %s\n"
            "__device__ const int DML_PLACE_OFF[DML_NUM_SIZES + 1] = {DML_PLACE_OFFSETS};\n"
            "static const int DML_PLACE_OFF_HOST[DML_NUM_SIZES + 1] = {DML_PLACE_OFFSETS};\n"
            "__device__ unsigned short DML_PLACE[DML_PLACE_N];\n"
            % (len(LARGE_SIZES), off[-1], rows(sizes, "%d", 8).replace(",\n", ", \\\n"), ", ".join("%d" % v for v in off)))


# ---- codewords -> text ----
PAD, LATCH_C40, LATCH_BASE256, FNC1, STRUCTURED_APPEND, READER_PROGRAMMING, UPPER_SHIFT = 129, 230, 231, 232, 233, 234, 235
MACRO_05, MACRO_06, LATCH_X12, LATCH_TEXT, LATCH_EDIFACT, ECI, UNLATCH = 236, 237, 238, 239, 240, 241, 254
GS = 0x1D
C40_BASIC = " 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"       # values 3..39 of the basic set (0..2 are the shifts)
TEXT_BASIC = " 0123456789abcdefghijklmnopqrstuvwxyz"
SHIFT2 = "!\"#$%&'()*+,-./:;<=>?@[\\]^_"                  # values 0..26 of shift set 2; 27 = FNC1, 30 = upper shift
TEXT_SHIFT3 = "`ABCDEFGHIJKLMNOPQRSTUVWXYZ{|}~\x7f"
X12_SET = "\r*> 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"


def unrandomise_255(value: int, position: int) -> int:
    """A Base 256 codeword at the 1-based position of the symbol's data -> its value."""
    return (value - ((149 * position) % 255 + 1)) % 256


def randomised_pad(position: int) -> int:
    """The pad codeword at the 1-based position behind the first pad (253-state randomisation of 129)."""
    v = PAD + (149 * position) % 253 + 1
    return v if v <= 254 else v - 254


def _bytes_text(b: bytes) -> str:
    try:
        return b.decode("utf-8")
    except UnicodeDecodeError:
        return b.decode("iso-8859-1")


def _c40_like(data: Sequence[int], at: int, out: List[int], scheme: int) -> Optional[int]:
    """C40 / Text / X12 from data[at] on -> the index behind the segment (after an unlatch, before a lone last codeword, or the end);
    None when a value is not of the set."""
    shift, upper = 0, False
    n = len(data)
    while True:
        if n - at == 0:
            return at
        if n - at == 1:                                    # one codeword left: it is ASCII
            return at
        if data[at] == UNLATCH:
            return at + 1
        v = 256 * data[at] + data[at + 1] - 1
        at += 2
        for u in (v // 1600, v // 40 % 40, v % 40):
            if u > 39:
                return None
            if scheme == LATCH_X12:
                out.append(ord(X12_SET[u]))
                continue
            ch = None
            if shift == 0:
                if u < 3:
                    shift = u + 1
                    continue
                ch = ord((C40_BASIC if scheme == LATCH_C40 else TEXT_BASIC)[u - 3])
            elif shift == 1:
                ch = u
                if u > 31:
                    return None
            elif shift == 2:
                if u < 27:
                    ch = ord(SHIFT2[u])
                elif u == 27:
                    ch = GS
                elif u == 30:
                    upper, shift = True, 0
                    continue
                else:
                    return None
            else:
                if u > 31:
                    return None
                ch = 96 + u if scheme == LATCH_C40 else ord(TEXT_SHIFT3[u])
            shift = 0
            out.append(ch + 128 if upper else ch)
            upper = False


def codewords_text(data: Sequence[int]) -> Tuple[Optional[str], Optional[str]]:
    """The data codewords of a symbol -> (text, None), ("", reason) for what is out of scope (structured append, reader programming,
    ECI), (None, None) when the stream is no valid encodation: that is no symbol.  An FNC1 behind the first position becomes the GS
    character 0x1D (the first position's marks GS1 and yields nothing); the macros are expanded."""
    data = [int(v) & 255 for v in data]
    out: List[int] = []
    tail: List[int] = []
    at, n, upper = 0, len(data), False
    while at < n:
        c = data[at]
        at += 1
        if c == PAD:
            break
        if c <= 128:
            out.append(c - 1 + (128 if upper else 0))
            upper = False
        elif c <= 229:
            out += [ord(ch) for ch in "%02d" % (c - 130)]
        elif c in (LATCH_C40, LATCH_TEXT, LATCH_X12):
            nxt = _c40_like(data, at, out, c)
            if nxt is None:
                return None, None
            at = nxt
        elif c == LATCH_BASE256:
            if at >= n:
                return None, None
            d1 = unrandomise_255(data[at], at + 1)
            at += 1
            if d1 == 0:
                count = n - at
            elif d1 < 250:
                count = d1
            else:
                if at >= n:
                    return None, None
                count = 250 * (d1 - 249) + unrandomise_255(data[at], at + 1)
                at += 1
            if count > n - at:
                return None, None
            out += [unrandomise_255(data[at + i], at + i + 1) for i in range(count)]
            at += count
        elif c == FNC1:
            if at != 1:
                out.append(GS)
        elif c == STRUCTURED_APPEND:
            return "", "structured append"
        elif c == READER_PROGRAMMING:
            return "", "reader programming"
        elif c == UPPER_SHIFT:
            upper = True
        elif c in (MACRO_05, MACRO_06):
            if at != 1:
                return None, None
            out += [ord(ch) for ch in "[)>\x1e%02d\x1d" % (5 if c == MACRO_05 else 6)]
            tail = [0x1E, 0x04]
        elif c == LATCH_EDIFACT:
            while True:
                if n - at <= 2:                            # at most two codewords left: they are ASCII
                    break
                bits = (data[at] << 16) | (data[at + 1] << 8) | data[at + 2]
                at += 3
                done = False
                for k in range(4):
                    v = (bits >> (18 - 6 * k)) & 63
                    if v == 0x1F:
                        at -= (2, 1, 0, 0)[k]              # the unlatch ends at a byte boundary: the bytes behind it are ASCII
                        done = True
                        break
                    out.append(v if v & 0x20 else v | 0x40)
                if done:
                    break
        elif c == ECI:
            return "", "ECI"
        elif c == UNLATCH:
            continue
        else:
            return None, None
    return _bytes_text(bytes(out + tail)), None


def is_gs1(data: Sequence[int]) -> bool:
    """FNC1 in the first position."""
    return len(data) > 0 and int(data[0]) == FNC1


def capacity_errors(size: int) -> int:
    """Errors the symbol's blocks can correct together."""
    return sum(ec // 2 for _, ec in block_lengths(size))


def confidence(size: int, errors: int) -> float:
    """1 - corrected errors / what the blocks can correct: 1.0 for a clean read."""
    return max(0.0, 1.0 - errors / float(capacity_errors(size)))


def read_datamatrix(codes, data) -> List[dict]:
    """Device rows int32 [m,12] + data codewords [m,MAX_DATA] (bytes [m,MAX_DATA_ALL] from lumina_ocr_datamatrix_sizes) -> one dict a symbol, in the rows' order: kind "DataMatrix", content,
    confidence, polygon (the hull's TL, TR, BR, BL as 8 floats), box, rows, cols, rotation, errors, `gs1`: True for a GS1 symbol, and
    `unsupported` with the reason where the content is out of scope (content is then "").  A row whose codewords are no valid
    encodation is left out."""
    out = []
    for c, d in zip(codes, data):
        x0, y0, x1, y1, rows, cols, ndata, errors, rotation = (int(v) for v in c[:9])
        size = size_index_all(rows, cols)
        if size < 0 or ndata != ALL_SIZES[size][2]:
            continue
        cw = [int(v) for v in d[:ndata]]
        text, reason = codewords_text(cw)
        if text is None:
            continue
        e = {"kind": "DataMatrix", "content": text, "confidence": confidence(size, errors),
             "polygon": [float(v) for v in (x0, y0, x1 + 1, y0, x1 + 1, y1 + 1, x0, y1 + 1)], "box": (x0, y0, x1, y1), "rows": rows, "cols": cols,
             "rotation": 90 * rotation, "errors": errors}
        if is_gs1(cw):
            e["gs1"] = True
        if reason is not None:
            e["unsupported"] = reason
        out.append(e)
    return out
