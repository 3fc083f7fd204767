"""Aztec codes, host half (pure Python): the geometry and the fields of the symbols whose module rows fit one 64-bit word (compact 1-4
layers, full-range 1-11 layers), an encoder (tests, the probe), the corrected data codewords of a device row (lumina_ocr_aztec:
x0, y0, x1, y1, layers, compact, codeword width, ndata, errors, rotation, mode-message errors, mismatches + the codewords) -> text,
and the entries the provider reports.

Everything here is written from recollection of the public symbology (ISO/IEC 24778); no standard text and no other implementation
was at hand.  What can be pinned structurally is pinned by tests/test_aztec_tables.py: the field polynomials are primitive, the size
and capacity formulas tabulate, the placement visits every data module exactly once and no function module, the mode bits are
distinct and on their ring.  csrc/aztec_tables.h holds the fields for the device (device_header() writes it; the test compares).

Full-range symbols of 12 .. 32 layers (ALL_SYMBOLS, MAX_DATA_ALL; lumina_ocr_aztec_layers reads them, read_aztec takes their rows with
max_layers above 11) go through the same formulas.  From recollection as well, and pinned only structurally by
tests/test_aztec_layers_tables.py: the polynomial 0x1069 of GF(4096), the 12-bit codewords from 23 layers on, and the reference grid's
lines every 16 modules from the centre.  csrc/aztec_tables12.h holds GF(4096) for the device (device_header12()).

Coordinates: a module is (x, y), x to the right, y down, in the upright symbol; the centre module is (c, c), c = size // 2.  A row of
modules is one 64-bit word, bit x, up to 11 layers and three words above."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

# ---- fields: GF(2^m) by its polynomial; alpha = x ----
FIELD_POLY = {4: 0x13, 6: 0x43, 8: 0x12D, 10: 0x409, 12: 0x1069}


def gf_tables(m: int) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """-> (exp, log): exp has 2 * 2^m entries (exp[i] = alpha^(i mod (2^m - 1))) so that exp[log a + log b] needs no reduction."""
    n, poly = (1 << m) - 1, FIELD_POLY[m]
    exp, log, x = [0] * (2 * (n + 1)), [0] * (n + 1), 1
    for i in range(n):
        exp[i], log[x] = x, i
        x <<= 1
        if x & (n + 1):
            x ^= poly
    for i in range(n, 2 * (n + 1)):
        exp[i] = exp[i - n]
    return tuple(exp), tuple(log)


_TABLES = {m: gf_tables(m) for m in (4, 6, 8, 10, 12)}
_NP_TABLES = {m: (np.array(e, np.int64), np.array(l, np.int64)) for m, (e, l) in _TABLES.items()}


def gf_mul(m: int, a: int, b: int) -> int:
    exp, log = _TABLES[m]
    return exp[log[a] + log[b]] if a and b else 0


def rs_check_words(data: Sequence[int], ec: int, m: int) -> List[int]:
    """The ec check words of data over GF(2^m), generator (x - a^1) ... (x - a^ec), the first word the highest power."""
    exp, log = _NP_TABLES[m]
    gen = np.zeros(ec + 1, np.int64)    # gen[j]: the coefficient j places below the leading one, which is gen[0] = 1
    gen[0] = 1
    for i in range(1, ec + 1):
        low = gen[:i]
        gen[1:i + 1] ^= np.where(low != 0, exp[log[low] + i], 0)
    tail, tail_log = gen[1:], log[gen[1:]]
    rem = np.zeros(ec + 1, np.int64)    # (one spare word behind, always zero)
    for d in data:
        f = int(d) ^ int(rem[0])
        rem[:ec] = rem[1:]
        if f:
            rem[:ec] ^= np.where(tail != 0, exp[tail_log + int(log[f])], 0)
    return [int(v) for v in rem[:ec]]


# ---- sizes ----
MAX_COMPACT_LAYERS, MAX_FULL_LAYERS = 4, 11     # in scope: rows of at most 61 modules
SYMBOLS = tuple((True, L) for L in range(1, 5)) + tuple((False, L) for L in range(1, 12))
MAX_DATA = 320                                  # ints a device data row holds (>= 316, the codewords of 11 layers)
MAX_LAYERS_ALL = 32                             # lumina_ocr_aztec_layers: full-range symbols of every size, rows of up to 151 modules
ALL_SYMBOLS = SYMBOLS + tuple((False, L) for L in range(12, 33))
MAX_DATA_ALL = 1664                             # uint16 words a device data row of lumina_ocr_aztec_layers holds: the codewords of 32 layers


def word_width(layers: int) -> int:
    return 6 if layers <= 2 else 8 if layers <= 8 else 10 if layers <= 22 else 12


def base_size(compact: bool, layers: int) -> int:
    """Side of the matrix without the reference grid's lines."""
    return (11 if compact else 14) + 4 * layers


def modules(compact: bool, layers: int) -> int:
    base = base_size(compact, layers)
    return base if compact else base + 1 + 2 * ((base // 2 - 1) // 15)


def total_bits(compact: bool, layers: int) -> int:
    return ((88 if compact else 112) + 16 * layers) * layers


def total_words(compact: bool, layers: int) -> int:
    return total_bits(compact, layers) // word_width(layers)


def ring_distance(compact: bool) -> int:
    """Chebyshev distance of the mode ring from the centre; the bullseye fills the distances below it, dark at the even ones."""
    return 5 if compact else 7


# ---- function modules ----
def mode_bit_positions(compact: bool) -> List[Tuple[int, int]]:
    """-> (dx, dy) from the centre of mode bit 0, 1, ...: clockwise from the top side's left end."""
    s = ring_distance(compact)
    n = 7 if compact else 10
    off = [(-3 + i) if compact else (-5 + i + i // 5) for i in range(n)]
    out = [(0, 0)] * (4 * n)
    for i, o in enumerate(off):
        out[i] = (o, -s)
        out[n + i] = (s, o)
        out[3 * n - 1 - i] = (o, s)
        out[4 * n - 1 - i] = (-s, o)
    return out


def orientation_marks(compact: bool) -> List[Tuple[int, int, bool]]:
    """-> (dx, dy, dark) of the three modules at every corner of the mode ring: the corner and its two neighbours on the ring."""
    s = ring_distance(compact)
    dark = {(-s, -s), (-s + 1, -s), (-s, -s + 1), (s, -s), (s, -s + 1), (s, s - 1)}
    out = []
    for cx, cy in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
        for dx, dy in ((cx * s, cy * s), (cx * (s - 1), cy * s), (cx * s, cy * (s - 1))):
            out.append((dx, dy, (dx, dy) in dark))
    return out


def grid_coordinate(compact: bool, layers: int, i: int) -> int:
    """Index i of the matrix without the grid lines -> the symbol's coordinate."""
    if compact:
        return i
    half, c = base_size(False, layers) // 2, modules(False, layers) // 2
    if i >= half:
        j = i - half
        return c + j + j // 15 + 1
    j = half - 1 - i
    return c - j - j // 15 - 1


def data_bit_position(compact: bool, layers: int, b: int) -> Tuple[int, int]:
    """Bit b of the symbol's bit stream -> its module (x, y).  Layer 0 is the outermost; a layer's four sides hold 2 rowSize bits each:
    the left side going down, the bottom going right, the right side going up, the top going left; bit 2 j + k of a side is domino j,
    k modules inwards."""
    base = base_size(compact, layers)
    i = 0
    while True:
        row = 4 * (layers - i) + (9 if compact else 12)
        if b < 8 * row:
            break
        b -= 8 * row
        i += 1
    side, r = divmod(b, 2 * row)
    j, k = divmod(r, 2)
    low, high = 2 * i, base - 1 - 2 * i
    x, y = ((low + k, low + j), (low + j, high - k), (high - k, high - j), (high - j, low + k))[side]
    return grid_coordinate(compact, layers, x), grid_coordinate(compact, layers, y)


def function_matrix(compact: bool, layers: int) -> Tuple[np.ndarray, np.ndarray]:
    """-> (is_function bool [n,n], dark bool [n,n]) indexed [y, x]: bullseye, orientation marks, reference grid; the mode ring's bits
    are function modules that are left clear."""
    n, s = modules(compact, layers), ring_distance(compact)
    c = n // 2
    fn, dark = np.zeros((n, n), bool), np.zeros((n, n), bool)
    for y in range(n):
        for x in range(n):
            dx, dy = x - c, y - c
            d = max(abs(dx), abs(dy))
            if d <= s:
                fn[y, x] = True
                dark[y, x] = d < s and d % 2 == 0
            elif not compact and (dx % 16 == 0 or dy % 16 == 0):
                fn[y, x] = True
                dark[y, x] = (dy if dx % 16 == 0 else dx) % 2 == 0
                if dx % 16 == 0 and dy % 16 == 0:
                    dark[y, x] = True
    for dx, dy, d in orientation_marks(compact):
        dark[c + dy, c + dx] = d
    return fn, dark


def mode_words(compact: bool, layers: int, ndata: int) -> List[int]:
    """The mode message's 4-bit words, check words behind."""
    v = ((layers - 1) << 6 | (ndata - 1)) if compact else ((layers - 1) << 11 | (ndata - 1))
    nw = 2 if compact else 4
    data = [(v >> (4 * (nw - 1 - i))) & 15 for i in range(nw)]
    return data + rs_check_words(data, 5 if compact else 6, 4)


def matrix_of_words(compact: bool, layers: int, words: Sequence[int], ndata: int, mode: Optional[Sequence[int]] = None) -> np.ndarray:
    """All codewords of a symbol (data then check) -> bool [n,n] indexed [y, x] (True = dark)."""
    w = word_width(layers)
    assert len(words) == total_words(compact, layers)
    _, m = function_matrix(compact, layers)
    c = m.shape[0] // 2
    mw = mode_words(compact, layers, ndata) if mode is None else list(mode)
    for i, (dx, dy) in enumerate(mode_bit_positions(compact)):
        m[c + dy, c + dx] = bool((mw[i // 4] >> (3 - i % 4)) & 1)
    pad = total_bits(compact, layers) % w
    for j, v in enumerate(words):
        for k in range(w):
            x, y = data_bit_position(compact, layers, pad + j * w + k)
            m[y, x] = bool((v >> (w - 1 - k)) & 1)
    return m


# ---- text <-> bits ----
UPPER, LOWER, MIXED, PUNCT, DIGIT = range(5)
_U = ["PS", " "] + [chr(65 + i) for i in range(26)] + ["LL", "ML", "DL", "BS"]
_L = ["PS", " "] + [chr(97 + i) for i in range(26)] + ["US", "ML", "DL", "BS"]
_M = ["PS", " "] + [chr(i) for i in range(1, 8)] + ["\b", "\t", "\n", "\v", "\f", "\r", "\x1b", "\x1c", "\x1d", "\x1e", "\x1f", "@", "\\", "^", "_", "`", "|",
                                                     "~", "\x7f", "LL", "UL", "PL", "BS"]
_P = ["FLG", "\r", "\r\n", ". ", ", ", ": "] + list("!\"#$%&'()*+,-./:;<=>?[]{}") + ["UL"]
_D = ["PS", " "] + list("0123456789,.") + ["UL", "US"]
TABLES = (_U, _L, _M, _P, _D)
_LATCH = {"LL": LOWER, "ML": MIXED, "DL": DIGIT, "UL": UPPER, "PL": PUNCT}
# the codes that latch from a mode to another, (code, width of the mode it is read in)
_PATH = {(UPPER, LOWER): ["LL"], (UPPER, MIXED): ["ML"], (UPPER, DIGIT): ["DL"], (UPPER, PUNCT): ["ML", "PL"],
         (LOWER, UPPER): ["ML", "UL"], (LOWER, MIXED): ["ML"], (LOWER, DIGIT): ["DL"], (LOWER, PUNCT): ["ML", "PL"],
         (MIXED, UPPER): ["UL"], (MIXED, LOWER): ["LL"], (MIXED, PUNCT): ["PL"], (MIXED, DIGIT): ["UL", "DL"],
         (PUNCT, UPPER): ["UL"], (PUNCT, LOWER): ["UL", "LL"], (PUNCT, MIXED): ["UL", "ML"], (PUNCT, DIGIT): ["UL", "DL"],
         (DIGIT, UPPER): ["UL"], (DIGIT, LOWER): ["UL", "LL"], (DIGIT, MIXED): ["UL", "ML"], (DIGIT, PUNCT): ["UL", "ML", "PL"]}


def _width(mode: int) -> int:
    return 4 if mode == DIGIT else 5


class BitWriter:
    """What the encoder appends to: codes of a mode, raw fields."""

    def __init__(self):
        self.bits: List[int] = []
        self.mode = UPPER

    def put(self, value: int, n: int) -> None:
        self.bits += [(value >> (n - 1 - i)) & 1 for i in range(n)]

    def code(self, name: str, mode: Optional[int] = None) -> None:
        mode = self.mode if mode is None else mode
        self.put(TABLES[mode].index(name), _width(mode))

    def latch(self, to: int) -> None:
        if to != self.mode:
            for name in _PATH[(self.mode, to)]:
                self.code(name)
                self.mode = _LATCH[name]

    def binary(self, data: bytes) -> None:
        if self.mode in (PUNCT, DIGIT):
            self.latch(UPPER)
        at = 0
        while at < len(data):
            n = min(len(data) - at, 2047 + 31)
            self.code("BS")
            if n <= 31:
                self.put(n, 5)
            else:
                self.put(0, 5)
                self.put(n - 31, 11)
            for v in data[at:at + n]:
                self.put(v, 8)
            at += n

    def flg(self, n: int, digits: str = "") -> None:
        """FLG(n) with its ECI digits, shifted into from the current mode (latched from Punct's own)."""
        if self.mode != PUNCT:
            self.code("PS")
        self.put(0, 5)
        self.put(n, 3)
        for d in digits:
            self.put(int(d) + 2, 4)

    def text(self, s: str) -> None:
        """Characters of the five tables in their modes (a latch whenever the mode has not got the character), everything else as
        binary-shifted Latin-1 bytes."""
        i = 0
        while i < len(s):
            ch = s[i]
            if ch in TABLES[self.mode] and len(ch) == 1:
                self.code(ch)
                i += 1
                continue
            to = next((m for m in (UPPER, LOWER, DIGIT, MIXED, PUNCT) if ch in TABLES[m]), None)
            if to is None:
                j = i
                while j < len(s) and not any(s[j] in t for t in TABLES):
                    j += 1
                self.binary(s[i:j].encode("iso-8859-1"))
                i = j
            elif to == PUNCT and self.mode != PUNCT:
                self.code("PS")
                self.code(ch, PUNCT)
                i += 1
            else:
                self.latch(to)


def content_bits(content, eci: Optional[int] = None, gs1: bool = False) -> List[int]:
    """str (Latin-1) or bytes -> the message bits.  eci: an ECI designator in front (26: a str is sent as UTF-8 bytes); gs1: FNC1 first."""
    w = BitWriter()
    if gs1:
        w.flg(0)
    if eci is not None:
        w.flg(len(str(eci)), str(eci))
    if isinstance(content, bytes):
        w.binary(content)
    elif eci == 26:
        w.binary(content.encode("utf-8"))
    else:
        w.text(content)
    return w.bits


def stuff_bits(bits: Sequence[int], w: int) -> List[int]:
    """Message bits -> data codewords of w bits: a word whose first w - 1 bits are all alike gets the other value as its last bit (it
    takes w - 1 bits of the message); the last word is padded with ones."""
    words, i, n = [], 0, len(bits)
    while i < n:
        v = 0
        for k in range(w):
            v = (v << 1) | (bits[i + k] if i + k < n else 1)
        if v >> 1 == (1 << (w - 1)) - 1:
            words.append(v & ~1)
            i += w - 1
        elif v >> 1 == 0:
            words.append(v | 1)
            i += w - 1
        else:
            words.append(v)
            i += w
    return words


def unstuff_words(words: Sequence[int], w: int) -> Optional[List[int]]:
    """Data codewords -> message bits; None when a word is 0 or 2^w - 1."""
    bits: List[int] = []
    for v in words:
        v = int(v)
        if v == 0 or v == (1 << w) - 1 or not 0 <= v < (1 << w):
            return None
        if v == 1:
            bits += [0] * (w - 1)
        elif v == (1 << w) - 2:
            bits += [1] * (w - 1)
        else:
            bits += [(v >> (w - 1 - k)) & 1 for k in range(w)]
    return bits


def symbol_words(content, compact: bool, layers: int, **kw) -> Tuple[List[int], int]:
    """-> (all codewords of the symbol, ndata): the data words are the stuffed message, everything else is check words."""
    w = word_width(layers)
    data = stuff_bits(content_bits(content, **kw), w)
    total = total_words(compact, layers)
    limit = 64 if compact else 2048
    if len(data) > min(total - 3, limit) or not data:
        raise ValueError("the content does not fit %d %s layers" % (layers, "compact" if compact else "full"))
    return data + rs_check_words(data, total - len(data), w), len(data)


def encode(content, compact: bool, layers: int, **kw) -> np.ndarray:
    words, nd = symbol_words(content, compact, layers, **kw)
    return matrix_of_words(compact, layers, words, nd)


def draw(page: np.ndarray, x: int, y: int, matrix: np.ndarray, module: int, rotation: int = 0, ink: int = 0) -> Tuple[int, int, int, int]:
    """Draw a symbol into page (uint8 [H,W,3], in place) with its top-left pixel at (x, y), `module` pixels a module, turned clockwise by
    rotation quarter turns; only dark modules are drawn.  -> the box (x0, y0, x1, y1), inclusive."""
    m = np.rot90(np.asarray(matrix, bool), -int(rotation) % 4)
    side = m.shape[0] * module
    if x < 0 or y < 0 or x + side > page.shape[1] or y + side > page.shape[0]:
        raise ValueError("the symbol does not fit the page")
    page[y:y + side, x:x + side][np.kron(m, np.ones((module, module), bool))] = ink
    return x, y, x + side - 1, y + side - 1


# ---- codewords -> text ----
_ENCODINGS = {3: "iso-8859-1", 26: "utf-8"}


def bits_text(bits: Sequence[int]) -> Tuple[Optional[str], Optional[str], bool]:
    """Message bits -> (text, None, gs1), ("", reason, gs1) for what is out of scope (structured append, FLG(7), an ECI other than 3
    and 26), (None, None, False) when an ECI's digits are none.  FLG(0) in the first position marks GS1 and yields nothing; later
    ones become GS (0x1D).  The stream ends where fewer bits are left than the next field needs."""
    n, at = len(bits), 0
    latch = shift = UPPER
    segs: List[Tuple[str, bytearray]] = [("iso-8859-1", bytearray())]
    gs1, first = False, True

    def take(k: int) -> int:
        nonlocal at
        v = 0
        for b in bits[at:at + k]:
            v = (v << 1) | b
        at += k
        return v

    if n >= 10 and bits[:10] == [1, 1, 1, 0, 1, 1, 1, 1, 0, 1]:           # ML UL in front: a structured-append header
        return "", "structured append", False
    while True:
        mode = shift
        if n - at < _width(mode):
            break
        name = TABLES[mode][take(_width(mode))]
        shift = latch
        if name == "FLG":
            if n - at < 3:
                break
            f = take(3)
            if f == 0:
                if first:
                    gs1 = True
                else:
                    segs[-1][1].append(0x1D)
            elif f == 7:
                return "", "FLG(7)", gs1
            else:
                if n - at < 4 * f:
                    break
                digits = [take(4) - 2 for _ in range(f)]
                if any(not 0 <= d <= 9 for d in digits):
                    return None, None, False
                eci = int("".join(str(d) for d in digits))
                if eci not in _ENCODINGS:
                    return "", "ECI %d" % eci, gs1
                segs.append((_ENCODINGS[eci], bytearray()))
        elif name == "BS":
            if n - at < 5:
                break
            count = take(5)
            if count == 0:
                if n - at < 11:
                    break
                count = take(11) + 31
            for _ in range(count):
                if n - at < 8:
                    break
                segs[-1][1].append(take(8))
        elif name in ("PS", "US"):
            shift = PUNCT if name == "PS" else UPPER
        elif name in _LATCH:
            latch = shift = _LATCH[name]
        else:
            segs[-1][1].extend(name.encode("iso-8859-1"))
        first = first and name == "PS"
    try:
        return "".join(bytes(b).decode(enc) for enc, b in segs), None, gs1
    except UnicodeDecodeError:
        return "".join(bytes(b).decode("iso-8859-1") for _, b in segs), None, gs1


def codewords_text(words: Sequence[int], w: int) -> Tuple[Optional[str], Optional[str], bool]:
    bits = unstuff_words(words, w)
    if bits is None:
        return None, None, False
    return bits_text(bits)


def confidence(ec: int, errors: int) -> float:
    """1 - corrected errors / what the block can correct: 1.0 for a clean read."""
    return max(0.0, 1.0 - errors / float(max(1, ec // 2)))


def read_aztec(codes, data, max_layers: int = MAX_FULL_LAYERS) -> List[dict]:
    """Device rows int32 [m,12] + data codewords [m,MAX_DATA] ([m,MAX_DATA_ALL] from lumina_ocr_aztec_layers, whose max_layers the caller
    passes on: full-range rows above it are left out) -> one dict a symbol, in the rows' order: kind "Aztec", content, confidence,
    polygon (the hull's TL, TR, BR, BL as 8 floats), box, layers, compact, rotation, errors, `gs1`: True for a GS1 symbol, and
    `unsupported` with the reason where the content is out of scope (content is then "").  A row whose codewords are no valid
    message (a stuffed word of 0 or 2^w - 1) is left out."""
    out = []
    for c, d in zip(codes, data):
        x0, y0, x1, y1, layers, compact, w, ndata, errors, rotation = (int(v) for v in c[:10])
        if not (1 <= layers <= (MAX_COMPACT_LAYERS if compact else max(MAX_FULL_LAYERS, min(int(max_layers), MAX_LAYERS_ALL)))) or w != word_width(layers):
            continue
        total = total_words(bool(compact), layers)
        if not 1 <= ndata < total:
            continue
        text, reason, gs1 = codewords_text([int(v) for v in d[:ndata]], w)
        if text is None:
            continue
        e = {"kind": "Aztec", "content": text, "confidence": confidence(total - ndata, errors),
             "polygon": [float(v) for v in (x0, y0, x1 + 1, y0, x1 + 1, y1 + 1, x0, y1 + 1)], "box": (x0, y0, x1, y1), "layers": layers,
             "compact": bool(compact), "rotation": 90 * rotation, "errors": errors}
        if gs1:
            e["gs1"] = True
        if reason is not None:
            e["unsupported"] = reason
        out.append(e)
    return out


def device_header() -> str:
    """The text of csrc/aztec_tables.h."""
    rows = lambda v, per: ",\n".join("    " + ", ".join("%d" % x for x in v[i:i + per]) for i in range(0, len(v), per))
    exp, log, off_e, off_l = [], [], [], []
    for m in (4, 6, 8, 10):
        e, l = _TABLES[m]
        off_e.append(len(exp))
        off_l.append(len(log))
        exp += e
        log += l
    return ("#pragma once\n// Written by lumina_ocr.utils.aztec.device_header(); tests/test_aztec_tables.py compares.  The fields of the Aztec pass:\n"
            "// GF(16) / 0x13, GF(64) / 0x43, GF(256) / 0x12D, GF(1024) / 0x409 as exp (doubled: 2 * 2^m entries) and log tables, field\n"
            "// f = (m - 4) / 2 at AZ_EXP_OFF[f] and AZ_LOG_OFF[f].\n"
            "constexpr int AZ_EXP_N = %d, AZ_LOG_N = %d;\n"
            "__device__ const int AZ_EXP_OFF[4] = {%s};\n"
            "__device__ const int AZ_LOG_OFF[4] = {%s};\n"
            "__device__ const unsigned short AZ_EXP[AZ_EXP_N] = {\n%s};\n"
            "__device__ const unsigned short AZ_LOG[AZ_LOG_N] = {\n%s};\n"
            % (len(exp), len(log), ", ".join(map(str, off_e)), ", ".join(map(str, off_l)), rows(exp, 24), rows(log, 24)))


def device_header12() -> str:
    """The text of csrc/aztec_tables12.h: the field of the 12-bit codewords (23 .. 32 layers)."""
    rows = lambda v, per: ",\n".join("    " + ", ".join("%d" % x for x in v[i:i + per]) for i in range(0, len(v), per))
    exp, log = _TABLES[12]
    return ("#pragma once\n// Written by lumina_ocr.utils.aztec.device_header12(); tests/test_aztec_layers_tables.py compares.  The field of the Aztec\n"
            "// symbols of 23 .. 32 layers: GF(4096) / 0x1069 as exp (doubled: 2 * 2^12 entries) and log tables.\n"
            "constexpr int AZ12_EXP_N = %d, AZ12_LOG_N = %d;\n"
            "__device__ const unsigned short AZ12_EXP[AZ12_EXP_N] = {\n%s};\n"
            "__device__ const unsigned short AZ12_LOG[AZ12_LOG_N] = {\n%s};\n" % (len(exp), len(log), rows(exp, 24), rows(log, 24)))
