"""An integer restatement of the strip decoders of csrc/lzw.hip (LZW in the TIFF 6.0 / PDF flavour, PackBits, raw strips) and of the
row stage behind them (predictor 2, sample unpack, palette, invert), with the device's status rules: 0 exactly when a strip produced
its rows x row bytes, -1 corrupt, -2 an LZW strip that does not start with Clear.  Also the two encoders the cases need and a code
packer for hand-made streams.  Pure Python + numpy; the expected pixels of every test are Pillow's, never this module's."""
import numpy as np

CLEAR, EOI = 256, 257
CODEC_NONE, CODEC_LZW, CODEC_PACKBITS = 1, 5, 32773


# ---- LZW ----
def lzw_decode(data: bytes, total: int):
    """-> (status, bytes produced (clipped at total), counters dict(codes, clears, widest)).  MSB-first codes of 9..12 bits; early
    change: the width grows when the table length reaches 2^bits - 1."""
    data = bytes(data)
    nbits_in = len(data) * 8
    acc = int.from_bytes(data, "big") if data else 0
    counters = dict(codes=0, clears=0, widest=0)
    bp = 0

    def get(n):
        nonlocal bp
        v = (acc >> (nbits_in - bp - n)) & ((1 << n) - 1)
        bp += n
        counters["codes"] += 1
        counters["widest"] = max(counters["widest"], n)
        return v

    out = bytearray()
    if nbits_in < 9:
        return -1, bytes(out), counters
    if get(9) != CLEAR:
        return -2, bytes(out), counters
    counters["clears"] += 1
    nb, nxt = 9, 258
    table = {}          # code -> (offset in out, length)
    prev = None         # (offset, length) of the string written last; None right after Clear
    while True:
        if bp + nb > nbits_in:
            return -1, bytes(out), counters
        code = get(nb)
        if code == CLEAR:
            counters["clears"] += 1
            nb, nxt, prev = 9, 258, None
            continue
        if code == EOI:
            return -1, bytes(out), counters
        if prev is None:
            if code >= 258:
                return -1, bytes(out), counters
        elif nxt >= 4096 or code > nxt:
            return -1, bytes(out), counters
        pos = len(out)
        if code < 256:
            s = bytes([code])
        elif code == nxt:
            s = bytes(out[prev[0]:prev[0] + prev[1]]) + bytes(out[prev[0]:prev[0] + 1])
        else:
            off, ln = table[code]
            s = bytes(out[off:off + ln])
        out += s[:total - pos]
        if prev is not None:
            table[nxt] = (prev[0], prev[1] + 1)
            nxt += 1
            if nxt >= (1 << nb) - 1 and nb < 12:
                nb += 1
        prev = (pos, len(s))
        if len(out) >= total:
            return 0, bytes(out), counters


def pack_codes(codes) -> bytes:
    """[(code, bits), ...] -> bytes, MSB first, the last byte padded with zeros: for hand-made streams"""
    acc = n = 0
    for code, bits in codes:
        assert 0 <= code < (1 << bits)
        acc = (acc << bits) | code
        n += bits
    pad = (-n) % 8
    return (acc << pad).to_bytes((n + pad) // 8, "big")


def lzw_codes(data: bytes, eoi: bool = True):
    """The code list [(code, bits)] of a greedy encoder with the decoder's width rule: Clear first, Clear again when the table is full
    (4096 entries), EOI last."""
    codes = [(CLEAR, 9)]
    nb, nxt = 9, 258
    table = {}
    w = b""
    first = True   # the decoder adds no entry for the first code after Clear

    def emit(code):
        nonlocal nb, nxt, first
        codes.append((code, nb))
        if first:
            first = False
        else:
            nxt += 1
            if nxt >= (1 << nb) - 1 and nb < 12:
                nb += 1

    def code_of(s):
        return s[0] if len(s) == 1 else table[s]

    for b in data:
        wb = w + bytes([b])
        if len(wb) == 1 or wb in table:
            w = wb
            continue
        emit(code_of(w))          # nb and nxt are now the decoder's after it has read this code
        if nxt >= 4096:           # its table is full: the only code it takes now is Clear
            codes.append((CLEAR, nb))
            nb, nxt, table, first = 9, 258, {}, True
        else:
            table[wb] = nxt       # the number the decoder gives w + b when it reads the next code
        w = bytes([b])
    if w:
        emit(code_of(w))
    if eoi:
        codes.append((EOI, nb))
    return codes


def lzw_encode(data: bytes, eoi: bool = True) -> bytes:
    return pack_codes(lzw_codes(data, eoi))


# ---- PackBits ----
def packbits_decode(data: bytes, total: int, eod: bool = False):
    """-> (status, bytes).  A header byte n: 0..127 copies n + 1 bytes, 129..255 repeats the next byte 257 - n times, 128 is skipped (or,
    with eod, ends the data)."""
    data = bytes(data)
    out = bytearray()
    ip = 0
    while len(out) < total:
        if ip >= len(data):
            return -1, bytes(out)
        h = data[ip]
        if h == 128:
            if eod:
                return -1, bytes(out)
            ip += 1
            continue
        if h < 128:
            n = h + 1
            if ip + 1 + n > len(data):
                return -1, bytes(out)
            s = data[ip + 1:ip + 1 + n]
            ip += 1 + n
        else:
            n = 257 - h
            if ip + 2 > len(data):
                return -1, bytes(out)
            s = data[ip + 1:ip + 2] * n
            ip += 2
        out += s[:total - len(out)]
    return 0, bytes(out)


def packbits_encode(data: bytes, eod: bool = False) -> bytes:
    """runs of >= 3 equal bytes become repeats (up to 128), the rest literals (up to 128)"""
    out = bytearray()
    i, n = 0, len(data)
    lit = bytearray()

    def flush():
        nonlocal lit
        for k in range(0, len(lit), 128):
            piece = lit[k:k + 128]
            out.append(len(piece) - 1)
            out.extend(piece)
        lit = bytearray()

    while i < n:
        j = i
        while j < n and data[j] == data[i] and j - i < 128:
            j += 1
        if j - i >= 3:
            flush()
            out.append(257 - (j - i))
            out.append(data[i])
        else:
            lit += data[i:j]
        i = j
    flush()
    if eod:
        out.append(128)
    return bytes(out)


# ---- strips -> pages ----
def row_bytes(width: int, comps: int, bits: int) -> int:
    return (width * comps * bits + 7) // 8


def decode_strip(data: bytes, total: int, codec: int, rle_eod: bool = False):
    """-> (status, bytes, counters or None)"""
    if codec == CODEC_LZW:
        return lzw_decode(data, total)
    if codec == CODEC_PACKBITS:
        st, out = packbits_decode(data, total, rle_eod)
        return st, out, None
    assert codec == CODEC_NONE
    if len(data) < total:
        return -1, b"", None
    return 0, bytes(data[:total]), None


def rows_to_rgb(rows: bytes, height: int, width: int, predictor=1, comps=1, bits=8, indexed=0, invert=0, palette=None) -> np.ndarray:
    """packed rows -> uint8 [H][W][3] as Pillow's convert('RGB') maps them (grey v * 255 / (2^bits - 1))"""
    rb = row_bytes(width, comps, bits)
    a = np.frombuffer(rows, np.uint8).reshape(height, rb)
    if predictor == 2:
        assert bits == 8
        a = (np.cumsum(a.reshape(height, width, comps).astype(np.int64), axis=1) & 255).astype(np.uint8).reshape(height, rb)
    if bits < 8:
        per = 8 // bits
        v = np.stack([(a >> (8 - bits * (k + 1))) & ((1 << bits) - 1) for k in range(per)], axis=2).reshape(height, rb * per)[:, :width]
    else:
        v = a.reshape(height, width, comps)
    if indexed:
        pal = np.frombuffer(bytes(palette), np.uint8).reshape(256, 3)
        return pal[v.reshape(height, width)]
    if comps == 3:
        return np.ascontiguousarray(v)
    g = (v.reshape(height, width).astype(np.int32) * (255 // ((1 << bits) - 1))).astype(np.uint8)
    if invert:
        g = 255 - g
    return np.repeat(g[:, :, None], 3, axis=2)


def decode_page(strips, height: int, width: int, rows_per_strip: int, params, palette=None):
    """params = (codec, predictor, components, bits, indexed, invert, rle_eod).  -> (page status = the lowest of its strips', RGB array or
    None, list of strip statuses, list of strip counters)"""
    codec, predictor, comps, bits, indexed, invert, eod = params
    rb = row_bytes(width, comps, bits)
    want = -(-height // rows_per_strip)
    if len(strips) != want:
        return -2, None, [], []
    rows, sts, ctrs = bytearray(), [], []
    for k, s in enumerate(strips):
        nrows = min(height, (k + 1) * rows_per_strip) - k * rows_per_strip
        st, out, c = decode_strip(bytes(s), nrows * rb, codec, bool(eod))
        sts.append(st)
        ctrs.append(c)
        rows += out.ljust(nrows * rb, b"\0")
    status = min(sts)
    if status != 0:
        return status, None, sts, ctrs
    return 0, rows_to_rgb(bytes(rows), height, width, predictor, comps, bits, indexed, invert, palette), sts, ctrs
