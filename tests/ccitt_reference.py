"""Integer restatement of the CCITT Group 4 (ITU-T T.6) decoder behind PDF's CCITTFaxDecode with K < 0, as csrc/ccitt.hip implements it:
the same tables, the same order of checks, the same statuses.  Written as a decoder, from the recommendation's code tables (T.4 tables 2
and 3, T.6 table 1); the tests grade it against source bitmaps encoded by libtiff, and the kernel against it.

    decode(stream, columns, rows, black_is_1=False) -> (status, bits)

bits: uint8 [rows][columns] of 0 / 1 in PDF's convention (a coded-white run gives 1 when BlackIs1 is false, 0 when it is true; in DeviceGray
with the default /Decode 0 is black and 1 is white).  status 0 ok; -1 corrupt: an unused code, a0 that does not advance, a run past the
line's end, a pass code whose b2 is the line's end, more transitions than columns + 1, bits read past the stream's end, or fewer lines
than `rows` before EOFB / the end of the stream.  Decoding stops after `rows` lines or at EOFB, whichever comes first; whatever follows is ignored.
"""
import numpy as np

MAX_COLUMNS = 8192   # the kernel's bound (CC_MAX_COLS): its changing-element arrays are LDS

WHITE_TERM = """00110101 000111 0111 1000 1011 1100 1110 1111 10011 10100 00111 01000 001000 000011 110100 110101 101010 101011 0100111
0001100 0001000 0010111 0000011 0000100 0101000 0101011 0010011 0100100 0011000 00000010 00000011 00011010 00011011 00010010 00010011
00010100 00010101 00010110 00010111 00101000 00101001 00101010 00101011 00101100 00101101 00000100 00000101 00001010 00001011 01010010
01010011 01010100 01010101 00100100 00100101 01011000 01011001 01011010 01011011 01001010 01001011 00110010 00110011 00110100""".split()
WHITE_MAKEUP = """11011 10010 010111 0110111 00110110 00110111 01100100 01100101 01101000 01100111 011001100 011001101 011010010 011010011
011010100 011010101 011010110 011010111 011011000 011011001 011011010 011011011 010011000 010011001 010011010 011000 010011011""".split()
BLACK_TERM = """0000110111 010 11 10 011 0011 0010 00011 000101 000100 0000100 0000101 0000111 00000100 00000111 000011000 0000010111
0000011000 0000001000 00001100111 00001101000 00001101100 00000110111 00000101000 00000010111 00000011000 000011001010 000011001011
000011001100 000011001101 000001101000 000001101001 000001101010 000001101011 000011010010 000011010011 000011010100 000011010101
000011010110 000011010111 000001101100 000001101101 000011011010 000011011011 000001010100 000001010101 000001010110 000001010111
000001100100 000001100101 000001010010 000001010011 000000100100 000000110111 000000111000 000000100111 000000101000 000001011000
000001011001 000000101011 000000101100 000001011010 000001100110 000001100111""".split()
BLACK_MAKEUP = """0000001111 000011001000 000011001001 000001011011 000000110011 000000110100 000000110101 0000001101100 0000001101101
0000001001010 0000001001011 0000001001100 0000001001101 0000001110010 0000001110011 0000001110100 0000001110101 0000001110110
0000001110111 0000001010010 0000001010011 0000001010100 0000001010101 0000001011010 0000001011011 0000001100100 0000001100101""".split()
# 1792 .. 2560, the same for both colours; a run longer than 2560 repeats the 2560 code
EXT_MAKEUP = """00000001000 00000001100 00000001101 000000010010 000000010011 000000010100 000000010101 000000010110 000000010111
000000011100 000000011101 000000011110 000000011111""".split()

assert (len(WHITE_TERM), len(WHITE_MAKEUP), len(BLACK_TERM), len(BLACK_MAKEUP), len(EXT_MAKEUP)) == (64, 27, 64, 27, 13)

WHITE_BITS, BLACK_BITS, MODE_BITS = 12, 13, 7
M_PASS, M_HORIZ, M_V0, M_VR1, M_VR2, M_VR3, M_VL1, M_VL2, M_VL3 = range(1, 10)
MODE_CODES = {"0001": M_PASS, "001": M_HORIZ, "1": M_V0, "011": M_VR1, "000011": M_VR2, "0000011": M_VR3, "010": M_VL1, "000010": M_VL2,
              "0000010": M_VL3}
V_DELTA = {M_V0: 0, M_VR1: 1, M_VR2: 2, M_VR3: 3, M_VL1: -1, M_VL2: -2, M_VL3: -3}
EOFB = 0x001001   # two EOL codes, 24 bits


def run_codes(white: bool):
    """[(code string, run)] of one colour: terminating, make-up and extended make-up codes"""
    term, make = (WHITE_TERM, WHITE_MAKEUP) if white else (BLACK_TERM, BLACK_MAKEUP)
    return ([(c, i) for i, c in enumerate(term)] + [(c, 64 * (i + 1)) for i, c in enumerate(make)]
            + [(c, 1792 + 64 * i) for i, c in enumerate(EXT_MAKEUP)])


def lookup_table(codes, bits: int) -> np.ndarray:
    """entry[next `bits` bits of the stream] = code length << 12 | value; 0 = no code starts with these bits"""
    t = np.zeros(1 << bits, np.uint16)
    for code, value in codes:
        n = len(code)
        assert n <= bits and value < 4096
        base = int(code, 2) << (bits - n)
        assert not t[base:base + (1 << (bits - n))].any(), "codes are not prefix-free"
        t[base:base + (1 << (bits - n))] = (n << 12) | value
    return t


WHITE_TABLE = lookup_table(run_codes(True), WHITE_BITS)
BLACK_TABLE = lookup_table(run_codes(False), BLACK_BITS)
MODE_TABLE = lookup_table(list(MODE_CODES.items()), MODE_BITS)


class _Bits:
    """MSB-first reader over the stream followed by zeros (the kernel's zero-padded tail)"""
    def __init__(self, data: bytes):
        self.v = int.from_bytes(bytes(data) + b"\0" * 8, "big")
        self.total = (len(data) + 8) * 8
        self.limit = len(data) * 8
        self.pos = 0

    def peek(self, n: int) -> int:
        if self.pos + n > self.total:
            return 0
        return (self.v >> (self.total - self.pos - n)) & ((1 << n) - 1)


def _run(b: _Bits, white: bool, room: int) -> int:
    """one run length: make-up codes then a terminating code; -1 = corrupt (an unused code, or a run longer than `room`)"""
    table, bits = (WHITE_TABLE, WHITE_BITS) if white else (BLACK_TABLE, BLACK_BITS)
    total = 0
    while True:
        e = int(table[b.peek(bits)])
        if e == 0:
            return -1
        b.pos += e >> 12
        total += e & 4095
        if total > room or b.pos > b.limit:
            return -1
        if (e & 4095) < 64:
            return total


def decode(stream, columns: int, rows: int, black_is_1: bool = False):
    status, out, _ = decode_ex(stream, columns, rows, black_is_1)
    return status, out


def decode_ex(stream, columns: int, rows: int, black_is_1: bool = False):
    """decode, and the number of bits read when the last line ended (tests cut streams there)"""
    assert 0 < columns <= MAX_COLUMNS and rows > 0
    W = columns
    out = np.zeros((rows, W), np.uint8)
    b = _Bits(stream)
    ref = [W, W, W]   # changing elements of the reference line (the imaginary white line), then three sentinels
    y = 0
    while y < rows:
        if b.peek(24) == EOFB:
            break
        cur = []
        a0, white, ri = -1, True, 0
        while a0 < W:
            while ref[ri] <= a0:   # b1: the first changing element right of a0 that changes to the opposite colour
                ri += 2
            b1, b2 = ref[ri], ref[ri + 1]
            e = int(MODE_TABLE[b.peek(MODE_BITS)])
            if e == 0:
                return -1, out, b.pos
            b.pos += e >> 12
            if b.pos > b.limit:
                return -1, out, b.pos
            mode = e & 4095
            if mode == M_PASS:
                if b2 >= W:   # T.6, pass mode: "identified when the position of b2 lies to the left of a1", and a1 <= columns
                    return -1, out, b.pos
                a0 = b2
                continue
            if mode == M_HORIZ:
                start = max(a0, 0)
                r1 = _run(b, white, W - start)
                if r1 < 0:
                    return -1, out, b.pos
                r2 = _run(b, not white, W - start - r1)
                if r2 < 0:
                    return -1, out, b.pos
                if start + r1 + r2 <= a0:
                    return -1, out, b.pos
                new = [t for t in (start + r1, start + r1 + r2) if t < W]   # (a change at the line's end is the sentinel's)
                if len(cur) + len(new) > W + 1:
                    return -1, out, b.pos
                cur += new
                a0 = start + r1 + r2
                continue
            a1 = b1 + V_DELTA[mode]
            if a1 <= a0 or a1 > W:
                return -1, out, b.pos
            if a1 < W:
                if len(cur) + 1 > W + 1:
                    return -1, out, b.pos
                cur.append(a1)
            a0 = a1
            white = not white
            ri = ri - 1 if ri > 0 else ri + 1
        # the finished line: pixel x is white when an even number of changing elements lie at or left of it
        line = np.zeros(W + 1, np.int64)
        for t in cur:
            line[t] += 1
        coded_white = (np.cumsum(line[:W]) & 1) == 0
        out[y] = coded_white ^ bool(black_is_1)
        ref = cur + [W, W, W]
        y += 1
    return (0 if y == rows else -1), out, b.pos


def to_rgb(bits: np.ndarray, invert: bool = False) -> np.ndarray:
    """bits -> RGB u8 [rows][columns][3] as DeviceGray shows them (/Decode [1 0]: invert)"""
    g = ((bits ^ int(bool(invert))) * 255).astype(np.uint8)
    return np.repeat(g[:, :, None], 3, axis=2)
