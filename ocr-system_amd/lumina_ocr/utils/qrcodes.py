"""QR codes, host half (pure Python): the tables of QR Code Model 2 versions 1-10, the corrected data codewords of a device row
(lumina_ocr_qrcodes: x0, y0, x1, y1, version, level, mask, ndata, errors, rotation, format distance, timing mismatches + the
codewords) -> text, and the entries the provider reports.

The tables are our reading of the public standard (ISO/IEC 18004), built from its rules: finder, separator, timing and alignment
patterns, the format and version areas and the dark module make the function mask; the two-column zigzag from the bottom right
gives the placement order; the block structure is typed and pinned by the published totals (tests/test_qr_tables.py).
The tables are built for all 40 versions under the *_ALL names (lumina_ocr_qrcodes_versions reads versions 11-40, data codewords as
bytes); the ten-version names are their first ten columns.  csrc/qr_version_tables.h is the device's copy of the *_ALL tables
(device_header_versions()): block counts, totals, alignment centres, version and format words; both decode stages read it.
csrc/qr_tables.h (device_header()) holds what only the ten-version stage reads: function masks, the placement table, GF(256).
The tests compare both files with what these functions write.

Coordinates: a module is (row, col), both 0 .. D - 1, D = 17 + 4 version; a row of modules is one 64-bit word, bit col."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

MIN_VERSION, MAX_VERSION = 1, 10
LEVELS = "LMQH"                        # level index 0..3 as the device reports it
LEVEL_FORMAT_BITS = (1, 0, 3, 2)       # the two level bits of the format information, by level index (index = bits ^ 1)
MAX_DATA = 288                         # ints a device data row holds (>= 274, the data codewords of 10-L)
MAX_CODEWORDS = 346
MAX_BLOCKS, MAX_BLOCK_LEN, MAX_EC = 8, 146, 30
FORMAT_XOR = 0b101010000010010
SECOND_COPY = 16                       # added to the reported format distance when the second copy was the one read


# ---- the tables, all 40 versions: what the functions below read ----
VERSIONS_ALL = 40
MAX_DATA_ALL = 2956                    # bytes a device data row of the all-versions call holds: the data codewords of 40-L
MAX_CODEWORDS_ALL = 3706
MAX_BLOCKS_ALL, MAX_BLOCK_LEN_ALL = 81, 153
MAX_ALIGNMENT = 7
# EC codewords per block and number of blocks, [level][version - 1].  Typed from memory of the standard's table; what pins them is in
# tests/test_qr_version_tables.py (the module count of every version, monotony, the data codewords of nine symbols, the first ten columns)
EC_PER_BLOCK_ALL = (
    (7, 10, 15, 20, 26, 18, 20, 24, 30, 18, 20, 24, 26, 30, 22, 24, 28, 30, 28, 28, 28, 28, 30, 30, 26, 28, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30),
    (10, 16, 26, 18, 24, 16, 18, 22, 22, 26, 30, 22, 22, 24, 24, 28, 28, 26, 26, 26, 26, 28, 28, 28, 28, 28, 28, 28, 28, 28, 28, 28, 28, 28, 28, 28, 28, 28, 28, 28),
    (13, 22, 18, 26, 18, 24, 18, 22, 20, 24, 28, 26, 24, 20, 30, 24, 28, 28, 26, 30, 28, 30, 30, 30, 30, 28, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30),
    (17, 28, 22, 16, 22, 28, 26, 26, 24, 28, 24, 28, 22, 24, 24, 30, 28, 28, 26, 28, 30, 24, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30, 30))
NUM_BLOCKS_ALL = (
    (1, 1, 1, 1, 1, 2, 2, 2, 2, 4, 4, 4, 4, 4, 6, 6, 6, 6, 7, 8, 8, 9, 9, 10, 12, 12, 12, 13, 14, 15, 16, 17, 18, 19, 19, 20, 21, 22, 24, 25),
    (1, 1, 1, 2, 2, 4, 4, 4, 5, 5, 5, 8, 9, 9, 10, 10, 11, 13, 14, 16, 17, 17, 18, 20, 21, 23, 25, 26, 28, 29, 31, 33, 35, 37, 38, 40, 43, 45, 47, 49),
    (1, 1, 2, 2, 4, 4, 6, 6, 8, 8, 8, 10, 12, 16, 12, 17, 16, 18, 21, 20, 23, 23, 25, 27, 29, 34, 34, 35, 38, 40, 43, 45, 48, 51, 53, 56, 59, 62, 65, 68),
    (1, 1, 2, 4, 4, 4, 5, 6, 8, 8, 11, 11, 16, 16, 18, 16, 19, 21, 25, 25, 25, 34, 30, 32, 35, 37, 40, 42, 45, 48, 51, 54, 57, 60, 63, 66, 70, 74, 77, 81))


def alignment_centres(version: int) -> Tuple[int, ...]:
    """The alignment pattern centres of a version by rule: version // 7 + 2 of them, the first 6, the last 4 version + 10, the others
    a constant even step back from the last (version 32 steps by 26, where the rule would say 28)."""
    if version == 1:
        return ()
    c, last = version // 7 + 2, 4 * version + 10
    step = 26 if version == 32 else (4 * version + 2 * c + 1) // (2 * c - 2) * 2
    return (6,) + tuple(last - step * k for k in range(c - 2, -1, -1))


def _data_modules(version: int) -> int:
    """Modules of a version that are no function module, counted from the patterns' sizes."""
    d, c = 17 + 4 * version, (0 if version == 1 else version // 7 + 2)
    n = d * d - 3 * 64 - 2 * (d - 16) - 31            # finders with separators, timing between them, format and the dark module
    if c:
        n -= 25 * (c * c - 3) - 2 * 5 * (c - 2)       # alignment patterns; those on a timing pattern share five modules with it
    return n - (36 if version >= 7 else 0)


ALIGNMENT_CENTRES_ALL = tuple(alignment_centres(v) for v in range(1, VERSIONS_ALL + 1))
TOTAL_CODEWORDS_ALL = tuple(_data_modules(v) // 8 for v in range(1, VERSIONS_ALL + 1))
REMAINDER_BITS_ALL = tuple(_data_modules(v) % 8 for v in range(1, VERSIONS_ALL + 1))

# versions 1-10 under their own names: the first ten columns (tests/test_qr_tables.py pins their values)
TOTAL_CODEWORDS, REMAINDER_BITS = TOTAL_CODEWORDS_ALL[:MAX_VERSION], REMAINDER_BITS_ALL[:MAX_VERSION]
EC_PER_BLOCK = tuple(row[:MAX_VERSION] for row in EC_PER_BLOCK_ALL)
NUM_BLOCKS = tuple(row[:MAX_VERSION] for row in NUM_BLOCKS_ALL)
ALIGNMENT_CENTRES = ALIGNMENT_CENTRES_ALL[:MAX_VERSION]


def dimension(version: int) -> int:
    return 17 + 4 * version


def block_structure(version: int, level: int) -> Tuple[int, int, int, int]:
    """-> (blocks, short blocks, data codewords of a short block, EC codewords of every block); the long blocks, which come last,
    hold one data codeword more."""
    total, nb, ec = TOTAL_CODEWORDS_ALL[version - 1], NUM_BLOCKS_ALL[level][version - 1], EC_PER_BLOCK_ALL[level][version - 1]
    return nb, nb - total % nb, total // nb - ec, ec


def data_codewords(version: int, level: int) -> int:
    return TOTAL_CODEWORDS_ALL[version - 1] - NUM_BLOCKS_ALL[level][version - 1] * EC_PER_BLOCK_ALL[level][version - 1]


# ---- GF(256), polynomial 0x11D: EXP has 512 entries so that EXP[LOG[a] + LOG[b]] needs no reduction ----
def _gf_tables() -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    exp, log, x = [0] * 512, [0] * 256, 1
    for i in range(255):
        exp[i], log[x] = x, i
        x <<= 1
        if x & 0x100:
            x ^= 0x11D
    for i in range(255, 512):
        exp[i] = exp[i - 255]
    return tuple(exp), tuple(log)


GF_EXP, GF_LOG = _gf_tables()


def gf_mul(a: int, b: int) -> int:
    return GF_EXP[GF_LOG[a] + GF_LOG[b]] if a and b else 0


# ---- format and version information ----
def format_word(level: int, mask: int) -> int:
    """The 15 bits drawn for (level index, mask): 5 data bits, 10 BCH(15,5) check bits (generator 0x537), XOR 101010000010010."""
    data = (LEVEL_FORMAT_BITS[level] << 3) | mask
    rem = data
    for _ in range(10):
        rem = (rem << 1) ^ ((rem >> 9) * 0x537)
    return ((data << 10) | rem) ^ FORMAT_XOR


# by the five data bits (level bits << 3 | mask), as the device matches them
FORMAT_WORDS = tuple(format_word(LEVEL_FORMAT_BITS.index(w >> 3), w & 7) for w in range(32))


def version_word(version: int) -> int:
    """The 18 bits of the version information (versions 7 and up): 6 data bits, 12 check bits (generator 0x1F25)."""
    rem = version
    for _ in range(12):
        rem = (rem << 1) ^ ((rem >> 11) * 0x1F25)
    return (version << 12) | rem


def format_positions(version: int) -> Tuple[List[Tuple[int, int]], List[Tuple[int, int]]]:
    """-> the (row, col) of bits 0..14 of the first copy (round the corner finder) and of the second (below the +x finder's
    neighbour row and beside the +y finder)."""
    d = dimension(version)
    first = [(i, 8) for i in range(6)] + [(7, 8), (8, 8), (8, 7)] + [(8, 14 - i) for i in range(9, 15)]
    second = [(8, d - 1 - i) for i in range(8)] + [(d - 15 + i, 8) for i in range(8, 15)]
    return first, second


def version_positions(version: int) -> List[Tuple[Tuple[int, int], Tuple[int, int]]]:
    d = dimension(version)
    return [((i // 3, d - 11 + i % 3), (d - 11 + i % 3, i // 3)) for i in range(18)]


def mask_bit(mask: int, row: int, col: int) -> bool:
    """Is module (row, col) inverted by mask pattern 0..7?"""
    x, y = col, row
    return ((x + y) % 2 == 0, y % 2 == 0, x % 3 == 0, (x + y) % 3 == 0, (x // 3 + y // 2) % 2 == 0, x * y % 2 + x * y % 3 == 0,
            (x * y % 2 + x * y % 3) % 2 == 0, ((x + y) % 2 + x * y % 3) % 2 == 0)[mask]


def function_modules(version: int) -> Dict[Tuple[int, int], bool]:
    """-> {(row, col): dark} of every function module; the format and version areas are present with dark = False (the encoder
    draws them), the dark module is dark."""
    d = dimension(version)
    f: Dict[Tuple[int, int], bool] = {}
    for i in range(d):                                   # timing patterns
        f[(6, i)] = f[(i, 6)] = i % 2 == 0
    for cr, cc in ((3, 3), (3, d - 4), (d - 4, 3)):      # finders with their separators
        for dr in range(-4, 5):
            for dc in range(-4, 5):
                r, c = cr + dr, cc + dc
                if 0 <= r < d and 0 <= c < d:
                    f[(r, c)] = max(abs(dr), abs(dc)) not in (2, 4)
    cs = ALIGNMENT_CENTRES_ALL[version - 1]
    for ar in cs:
        for ac in cs:
            if (ar, ac) in ((6, 6), (6, cs[-1]), (cs[-1], 6)):
                continue
            for dr in range(-2, 3):
                for dc in range(-2, 3):
                    f[(ar + dr, ac + dc)] = max(abs(dr), abs(dc)) != 1
    first, second = format_positions(version)
    for p in first + second:
        f[p] = False
    f[(d - 8, 8)] = True                                  # the dark module
    if version >= 7:
        for a, b in version_positions(version):
            f[a] = f[b] = False
    return f


def function_mask(version: int) -> List[int]:
    """-> D row words, bit col set where (row, col) is a function module."""
    rows = [0] * dimension(version)
    for r, c in function_modules(version):
        rows[r] |= 1 << c
    return rows


def placement(version: int) -> List[Tuple[int, int]]:
    """-> the (row, col) of every data module in placement order: two-column strips from the right edge, alternately upwards and
    downwards, the right column of a strip first, column 6 (the timing pattern) skipped."""
    d, fm = dimension(version), function_mask(version)
    out = []
    right, up = d - 1, True
    while right >= 1:
        if right == 6:
            right = 5
        for k in range(d):
            row = d - 1 - k if up else k
            for col in (right, right - 1):
                if not (fm[row] >> col) & 1:
                    out.append((row, col))
        up = not up
        right -= 2
    return out


_PLACEMENT = {v: tuple(placement(v)) for v in range(MIN_VERSION, MAX_VERSION + 1)}
_FUNCTION = {v: tuple(function_mask(v)) for v in range(MIN_VERSION, MAX_VERSION + 1)}


_PLACEMENT_ALL: Dict[int, Tuple[Tuple[int, int], ...]] = {}     # versions 11-40, built when first asked for
_FUNCTION_ALL: Dict[int, Tuple[int, ...]] = {}


def placement_of(version: int) -> Tuple[Tuple[int, int], ...]:
    if version <= MAX_VERSION:
        return _PLACEMENT[version]
    if version not in _PLACEMENT_ALL:
        _PLACEMENT_ALL[version] = tuple(placement(version))
    return _PLACEMENT_ALL[version]


def function_mask_of(version: int) -> Tuple[int, ...]:
    if version <= MAX_VERSION:
        return _FUNCTION[version]
    if version not in _FUNCTION_ALL:
        _FUNCTION_ALL[version] = tuple(function_mask(version))
    return _FUNCTION_ALL[version]


VERSION_WORDS = tuple(version_word(v) for v in range(7, VERSIONS_ALL + 1))


def device_header_versions() -> str:
    """The text of csrc/qr_version_tables.h: what the all-versions kernel reads.  No placement and no function mask: the kernel
    builds the mask from the alignment centres and walks the strips itself."""
    vs = range(1, VERSIONS_ALL + 1)
    rows = lambda v, f, per: ",\n".join("    " + ", ".join(f % x for x in v[i:i + per]) for i in range(0, len(v), per))
    nb = [NUM_BLOCKS_ALL[lv][v - 1] for v in vs for lv in range(4)]
    ec = [EC_PER_BLOCK_ALL[lv][v - 1] for v in vs for lv in range(4)]
    align = [x for v in vs for x in (list(ALIGNMENT_CENTRES_ALL[v - 1]) + [0] * MAX_ALIGNMENT)[:MAX_ALIGNMENT]]
    return ("#pragma once\n// Written by lumina_ocr.utils.qrcodes.device_header_versions(); tests/test_qr_version_tables.py compares.  QR Code Model 2,\n"
            "// versions 1..40.  QRV_NB / QRV_EC: blocks and EC codewords of a block by (version - 1) * 4 + level (L, M, Q, H); a symbol's\n"
            "// total %% blocks last blocks hold one data codeword more.  QRV_TOTAL: all codewords.  QRV_ALIGN: version / 7 + 2 alignment centres\n"
            "// (none at version 1), zero padded to 7.  QRV_VERSION_WORD: the 18 drawn bits of versions 7..40.  QRV_FORMAT: the 15 drawn bits by\n"
            "// (level bits << 3 | mask).\n"
            "constexpr int QRV_VERSIONS = %d, QRV_MAX_ALIGN = %d, QRV_MAX_TOTAL = %d, QRV_MAX_DATA = %d, QRV_MAX_NB = %d, QRV_MAX_BLOCK = %d;\n"
            "__device__ const unsigned char QRV_NB[QRV_VERSIONS * 4] = {\n%s};\n"
            "__device__ const unsigned char QRV_EC[QRV_VERSIONS * 4] = {\n%s};\n"
            "__device__ const unsigned short QRV_TOTAL[QRV_VERSIONS] = {\n%s};\n"
            "__device__ const unsigned char QRV_ALIGN[QRV_VERSIONS * QRV_MAX_ALIGN] = {\n%s};\n"
            "__device__ const unsigned int QRV_VERSION_WORD[QRV_VERSIONS - 6] = {\n%s};\n"
            "__device__ const unsigned short QRV_FORMAT[32] = {\n%s};\n"
            % (len(vs), MAX_ALIGNMENT, MAX_CODEWORDS_ALL, MAX_DATA_ALL, MAX_BLOCKS_ALL, MAX_BLOCK_LEN_ALL, rows(nb, "%d", 16), rows(ec, "%d", 16),
               rows(list(TOTAL_CODEWORDS_ALL), "%d", 10), rows(align, "%d", 14), rows(list(VERSION_WORDS), "0x%05x", 8),
               rows(list(FORMAT_WORDS), "0x%04x", 8)))


def device_header() -> str:
    """The text of csrc/qr_tables.h."""
    vs = range(MIN_VERSION, MAX_VERSION + 1)
    rows = lambda v, f, per: ",\n".join("    " + ", ".join(f % x for x in v[i:i + per]) for i in range(0, len(v), per))
    func = [w for v in vs for w in list(_FUNCTION[v]) + [0] * (64 - dimension(v))]
    place, off = [], [0]
    for v in vs:
        place += [(r << 6) | c for r, c in _PLACEMENT[v]]
        off.append(len(place))
    return ("#pragma once\n// Written by lumina_ocr.utils.qrcodes.device_header(); tests/test_qr_tables.py compares.  QR Code Model 2, versions 1..10.\n"
            "// QR_FUNC: 64 row words a version, bit col set where (row, col) is a function module.  QR_PLACE: (row << 6 | col) of every data\n"
            "// module in placement order, version v at QR_PLACE_OFF[v - 1] .. QR_PLACE_OFF[v].  QR_EXP / QR_LOG: GF(256), polynomial 0x11D, EXP\n"
            "// doubled.  Totals, block structure and format words: qr_version_tables.h.\n"
            "constexpr int QR_VERSIONS = %d, QR_PLACE_N = %d;\n"
            "__device__ const unsigned long long QR_FUNC[QR_VERSIONS * 64] = {\n%s};\n"
            "__device__ const unsigned short QR_PLACE[QR_PLACE_N] = {\n%s};\n"
            "__device__ const int QR_PLACE_OFF[QR_VERSIONS + 1] = {\n%s};\n"
            "__device__ const unsigned char QR_EXP[512] = {\n%s};\n"
            "__device__ const unsigned char QR_LOG[256] = {\n%s};\n"
            % (len(vs), len(place), rows(func, "0x%016xull", 4), rows(place, "0x%03x", 16), rows(off, "%d", 11), rows(list(GF_EXP), "%d", 32),
               rows(list(GF_LOG), "%d", 32)))


# ---- codewords -> text ----
ALNUM = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ $%*+-./:"
MODE_NUMERIC, MODE_ALNUM, MODE_BYTE, MODE_ECI = 1, 2, 4, 7
ECI_UTF8 = 26


def count_bits(mode: int, version: int) -> int:
    """Width of the character count of a segment: versions 1-9, 10-26 and 27-40 differ."""
    k = 0 if version <= 9 else 1 if version <= 26 else 2
    return {MODE_NUMERIC: (10, 12, 14), MODE_ALNUM: (9, 11, 13), MODE_BYTE: (8, 16, 16)}[mode][k]


class _Bits:
    def __init__(self, data: Sequence[int]):
        self.data, self.pos, self.n = [int(v) & 255 for v in data], 0, 8 * len(data)

    def left(self) -> int:
        return self.n - self.pos

    def take(self, k: int) -> Optional[int]:
        if k > self.left():
            return None
        v = 0
        for _ in range(k):
            v = (v << 1) | ((self.data[self.pos >> 3] >> (7 - (self.pos & 7))) & 1)
            self.pos += 1
        return v


def _bytes_text(b: bytes) -> str:
    try:
        return b.decode("utf-8")
    except UnicodeDecodeError:
        return b.decode("iso-8859-1")


def codewords_text(version: int, data: Sequence[int]) -> Tuple[Optional[str], Optional[str]]:
    """The data codewords of a symbol -> (text, None), ("", reason) for what is out of scope, (None, None) when the bit stream runs
    past the codewords: that is no symbol."""
    bits, out = _Bits(data), []
    while True:
        if bits.left() < 4:                    # a terminator shorter than four bits, at capacity
            break
        mode = bits.take(4)
        if mode == 0:
            break
        if mode == MODE_ECI:
            first = bits.take(8)
            if first is None:
                return None, None
            extra = 0 if first < 0x80 else 1 if first < 0xC0 else 2
            rest = bits.take(8 * extra)
            if rest is None or first >= 0xE0:
                return None, None
            eci = ((first & (0x7F >> extra)) << (8 * extra)) | rest
            if eci != ECI_UTF8:
                return "", "ECI %d" % eci
            continue
        if mode not in (MODE_NUMERIC, MODE_ALNUM, MODE_BYTE):
            return "", {8: "kanji", 3: "structured append", 5: "FNC1", 9: "FNC1"}.get(mode, "mode %d" % mode)
        n = bits.take(count_bits(mode, version))
        if n is None:
            return None, None
        if mode == MODE_NUMERIC:
            for k in range(0, n, 3):
                m = min(3, n - k)
                v = bits.take((0, 4, 7, 10)[m])
                if v is None or v >= 10 ** m:
                    return None, None
                out.append("%0*d" % (m, v))
        elif mode == MODE_ALNUM:
            for k in range(0, n, 2):
                if n - k >= 2:
                    v = bits.take(11)
                    if v is None or v >= 45 * 45:
                        return None, None
                    out.append(ALNUM[v // 45] + ALNUM[v % 45])
                else:
                    v = bits.take(6)
                    if v is None or v >= 45:
                        return None, None
                    out.append(ALNUM[v])
        else:
            raw = []
            for _ in range(n):
                v = bits.take(8)
                if v is None:
                    return None, None
                raw.append(v)
            out.append(_bytes_text(bytes(raw)))
    return "".join(out), None


def capacity_errors(version: int, level: int) -> int:
    """Errors the symbol's blocks can correct together: blocks * floor(ec / 2)."""
    nb, _, _, ec = block_structure(version, level)
    return nb * (ec // 2)


def confidence(version: int, level: int, errors: int) -> float:
    """1 - corrected errors / (blocks * floor(ec / 2)): 1.0 for a clean read, 0.0 when every block used all it can correct."""
    return max(0.0, 1.0 - errors / float(capacity_errors(version, level)))


def read_qrcodes(codes, data) -> List[dict]:
    """Device rows int32 [m,12] + data codewords [m,MAX_DATA] (int32, lumina_ocr_qrcodes) or [m,MAX_DATA_ALL] (uint8,
    lumina_ocr_qrcodes_versions, versions up to 40) -> one dict a symbol, in the rows' order: kind "QRCode", content,
    confidence, polygon (the hull's TL, TR, BR, BL as 8 floats), box, version, level, mask, rotation, errors, and `unsupported` with
    the reason where the content is out of scope (content is then "").  A row whose bit stream runs past its codewords is left out."""
    out = []
    for c, d in zip(codes, data):
        x0, y0, x1, y1, version, level, mask, ndata, errors, rotation = (int(v) for v in c[:10])
        if not (MIN_VERSION <= version <= VERSIONS_ALL and 0 <= level < 4 and 0 < ndata <= len(d)):
            continue
        text, reason = codewords_text(version, list(d[:ndata]))
        if text is None:
            continue
        e = {"kind": "QRCode", "content": text, "confidence": confidence(version, level, errors),
             "polygon": [float(v) for v in (x0, y0, x1 + 1, y0, x1 + 1, y1 + 1, x0, y1 + 1)], "box": (x0, y0, x1, y1), "version": version,
             "level": LEVELS[level], "mask": mask, "rotation": 90 * rotation, "errors": errors}
        if reason is not None:
            e["unsupported"] = reason
        out.append(e)
    return out
