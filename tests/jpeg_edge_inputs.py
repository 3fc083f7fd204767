"""Input builders (test infrastructure, numpy) for the regimes of the JPEG encoder that noise and text pages never enter: flat pages
(Huffman tables of one or two symbols), maximum-swing patterns (DC differences of category 11, AC sizes of 10), grey pages (chroma
AC tables that hold only EOB), a coded stream with 0xFF bytes on both sides of a 4096-byte piece border and a run of them, and a
page whose luma AC histogram drives the optimal-table length limiter well past 16 bits.  Shared by tests/test_jpeg_edge_inputs.py
(CPU: the oracle against Pillow, and each input's property) and tests/test_gpu_jpeg.py (GPU: the device against both).

Every builder returns uint8 [H, W, 3] and is deterministic; INPUTS maps a name to its builder.  The probes at the end read a
property off the oracle's coefficients or file."""
from __future__ import annotations

import heapq
from typing import Callable, Dict, List, Tuple

import numpy as np

from lumina_ocr import synth

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
STD_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                     80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                     95, 98, 112, 100, 103, 99])                   # T.81 Annex K.1, natural order

FLAT_SIZES = [(1, 1), (16, 16), (37, 53), (200, 300)]
FLAT_VALUES = {"white": 255, "black": 0, "grey": 128}
PATTERN_SIZE = (72, 104)           # 9 x 13 blocks: partial MCUs on both sides, dummy luma blocks on the right and at the bottom
QUALITIES = [100, 95, 75, 30, 10, 1]
SETTINGS = [(q, True) for q in QUALITIES] + [(100, False), (30, False)]          # (quality, optimize) pairs the GPU test encodes
PIECE = 4096                       # bytes of coded stream per work-group of the device's 0xFF count and stuffing kernels


def _rgb(grey: np.ndarray) -> np.ndarray:
    return np.repeat(np.asarray(grey, np.uint8)[..., None], 3, axis=-1)


# ---- flat and almost flat pages ---------------------------------------------------------------------------------------------------
def flat(h: int, w: int, value: int) -> np.ndarray:
    return np.full((h, w, 3), value, np.uint8)


def one_ink_pixel(h: int = 37, w: int = 53) -> np.ndarray:
    """white, one black pixel inside the second block row"""
    p = flat(h, w, 255)
    p[11, 20] = 0
    return p


def blank_text_page(h: int = 250, w: int = 333, seed: int = 23) -> np.ndarray:
    """a synthetic text page with every line erased: white, with the shape (and the partial MCUs) of a real page"""
    page, lines = synth.synth_page(h, w, seed, n_lines=max(2, h // 40), noise=0.0)
    page = page.copy()
    for ln in lines:
        x0, y0, x1, y1 = (int(v) for v in ln["box"])
        page[max(0, y0 - 2):y1 + 3, max(0, x0 - 2):x1 + 3] = 255
    return page


# ---- maximum-swing patterns -------------------------------------------------------------------------------------------------------
def _grid(h: int, w: int) -> Tuple[np.ndarray, np.ndarray]:
    return np.mgrid[0:h, 0:w]


def checkerboard(h: int = PATTERN_SIZE[0], w: int = PATTERN_SIZE[1]) -> np.ndarray:
    yy, xx = _grid(h, w)
    return _rgb(np.where((yy + xx) % 2 == 0, 255, 0))


def vertical_stripes(h: int = PATTERN_SIZE[0], w: int = PATTERN_SIZE[1]) -> np.ndarray:
    yy, xx = _grid(h, w)
    return _rgb(np.where(xx % 2 == 0, 255, 0))


def horizontal_stripes(h: int = PATTERN_SIZE[0], w: int = PATTERN_SIZE[1]) -> np.ndarray:
    yy, xx = _grid(h, w)
    return _rgb(np.where(yy % 2 == 0, 255, 0))


def blocks8(h: int = PATTERN_SIZE[0], w: int = PATTERN_SIZE[1]) -> np.ndarray:
    """alternating black and white 8x8 blocks: neighbouring luma DCs are -1024 and 1016 at quality 100"""
    yy, xx = _grid(h, w)
    return _rgb(np.where((yy // 8 + xx // 8) % 2 == 0, 0, 255))


def mcus16(h: int = PATTERN_SIZE[0], w: int = PATTERN_SIZE[1]) -> np.ndarray:
    """alternating black and white 16x16 MCUs: the DC jump sits between the last luma block of an MCU and the first of the next"""
    yy, xx = _grid(h, w)
    return _rgb(np.where((yy // 16 + xx // 16) % 2 == 0, 0, 255))


def saturated_stripes(h: int = PATTERN_SIZE[0], w: int = PATTERN_SIZE[1]) -> np.ndarray:
    """R = 255, G = 0, B in 2-pixel vertical stripes of 0 / 255 that change phase every 2 rows: the 2x2 chroma quads alternate between
    the extremes of Cb, so the chroma blocks carry coefficients as large as the luma blocks of the checkerboard"""
    yy, xx = _grid(h, w)
    p = np.zeros((h, w, 3), np.uint8)
    p[..., 0] = 255
    p[..., 2] = np.where((yy // 2 + xx // 2) % 2 == 0, 255, 0)
    return p


def grey_noise(h: int = 200, w: int = 300, seed: int = 41) -> np.ndarray:
    """luma noise with R = G = B: Cb = Cr = 128 everywhere, every chroma block is EOB only"""
    return _rgb(np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8))


def colour_noise(h: int = 200, w: int = 300, seed: int = 5) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- a coded stream dense in 0xFF -----------------------------------------------------------------------------------------------
FF_SEED, FF_TILE_SEED, FF_SIZE, FF_SETTING = 352, 846, (200, 300), (100, False)


def ff_tile(seed: int) -> np.ndarray:
    """one grey 16x16 MCU whose second luma block codes, under the Annex K.3 tables at quality 100, as 24 one bits in a row: a DC
    difference of 1023 (ten one bits of value) and then the symbol (run 15, size 8), whose code 0xFFFC starts with fourteen.  Block 0
    is flat at 14; block 1 is 141.875 + 50 cos cos of the coefficient at scan position 16 (vertical frequency 1, horizontal 4), plus a
    seeded dither below one grey level: the seed decides whether rounding to pixels leaves scan positions 1-15 exactly zero and the DC
    at 111 (block 0: -912)"""
    rng = np.random.default_rng(seed)
    s = (2 * np.arange(8) + 1) * np.pi / 16
    blk = 141.875 + 50.0 * np.outer(np.cos(s), np.cos(4 * s)) + rng.uniform(-0.5, 0.5, (8, 8))
    tile = np.full((16, 16), 14.0)
    tile[:8, 8:] = blk
    return _rgb(np.rint(tile))


def ff_dense(seed: int = FF_SEED) -> np.ndarray:
    """black / white pixel noise (at quality 100 its coefficients are large, and about 3 % of the coded bytes are 0xFF under the Annex K.3
    tables) with ff_tile(FF_TILE_SEED) in every third MCU: the stream offsets of the tiles cover every bit phase, so some tile's 24 one
    bits are three whole bytes.  Noise alone never gives that run: no code is all ones, so 24 one bits need a ten-bit value of ones
    and a code that starts with fourteen.  FF_SEED was found by searching seeds on the CPU for a stream (before stuffing) with 0xFF at
    4096 k - 1 and 4096 k for some k >= 1; tests/test_jpeg_edge_inputs.py checks that the committed seeds still give both"""
    h, w = FF_SIZE
    page = _rgb(np.where(np.random.default_rng(seed).random((h, w)) < 0.5, 0, 255))
    tile = ff_tile(FF_TILE_SEED)
    for m in range(0, (h // 16) * (w // 16), 3):
        y, x = 16 * (m // (w // 16)), 16 * (m % (w // 16))
        page[y:y + 16, x:x + 16] = tile
    return page


# ---- a luma AC histogram that is Fibonacci-like: the optimal code is a chain, far deeper than 16 bits ----------------------------------
DEEP_SIZE, DEEP_QUALITY = (512, 512), 75


def _deep_symbols() -> List[Tuple[int, int, int]]:
    """(run, value, count), rarest first.  With the reserved pseudo-symbol (count 1) and EOB (one per block: 4096) in its place in the
    order, every count is at least 1 + the sum of all counts two and more places below it, so each Huffman merge joins the growing
    tree with the next symbol: 22 symbols, the rarest 22 deep."""
    rare = [(15, 1), (14, 1), (13, 1), (12, 1), (11, 1), (10, 1), (9, 1), (8, 1), (7, 1), (6, 1), (5, 1), (4, 2), (3, 2), (2, 2), (1, 2), (0, 2)]
    fib = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597]
    out = [(r, v, c) for (r, v), c in zip(rare, fib)]
    below, prev, eob = 1 + sum(fib[:-1]), fib[-1], 4096       # below: the tree's weight when `prev` is about to join it
    assert eob >= below
    below, prev = below + prev, eob
    for run in (4, 3, 2, 1, 0):
        c = max(below, prev) + 1
        out.append((run, 1, c))
        below, prev = below + prev, c
    return out


def deep_huffman() -> np.ndarray:
    """512 x 512 grey page built block by block from designed quantised luma coefficients (values +-1, +-2 at chosen runs; inverse DCT of
    coefficient x quantiser of DEEP_QUALITY, rounded to pixels — the rounding error stays below half a quantiser step)"""
    h, w = DEEP_SIZE
    nb = (h // 8) * (w // 8)
    items: List[List[Tuple[int, int]]] = [[] for _ in range(nb)]      # per block: (run, value) in scan order
    room = np.full(nb, 62)                                            # position 63 stays zero: every block ends in EOB
    rng = np.random.default_rng(7)
    for run, val, count in reversed(_deep_symbols()):                 # most frequent first: spread evenly, the rest where room is left
        per, extra = divmod(count, nb)
        order = np.argsort(-room, kind="stable")
        for j, b in enumerate(order):
            k = per + (1 if j < extra else 0)
            assert room[b] >= k * (run + 1)
            items[b] += [(run, val)] * k
            room[b] -= k * (run + 1)
    scale = 200 - 2 * DEEP_QUALITY
    quant = np.clip((STD_LUMA * scale + 50) // 100, 1, 255)
    coef = np.zeros((nb, 64))
    for b in range(nb):
        k = 0
        for run, val in items[b]:
            k += run + 1
            coef[b, ZIGZAG[k]] = val * quant[ZIGZAG[k]] * (1 if rng.random() < 0.5 else -1)
    u = np.arange(8)
    basis = np.cos((2 * u[None, :] + 1) * u[:, None] * np.pi / 16) * np.where(u[:, None] == 0, np.sqrt(0.125), 0.5)     # [freq, sample]
    px = np.einsum("ur,buv,vc->brc", basis, coef.reshape(nb, 8, 8), basis) + 128.0
    assert px.min() >= 0.0 and px.max() <= 255.0
    img = np.rint(px).reshape(h // 8, w // 8, 8, 8).swapaxes(1, 2).reshape(h, w)
    return _rgb(img)


def _builders() -> Dict[str, Callable[[], np.ndarray]]:
    d: Dict[str, Callable[[], np.ndarray]] = {}
    for name, v in FLAT_VALUES.items():
        for h, w in FLAT_SIZES:
            d["%s_%dx%d" % (name, h, w)] = (lambda h=h, w=w, v=v: flat(h, w, v))
    d.update(one_ink_pixel=one_ink_pixel, blank_text_page=blank_text_page, checkerboard=checkerboard, vertical_stripes=vertical_stripes,
             horizontal_stripes=horizontal_stripes, blocks8=blocks8, mcus16=mcus16, saturated_stripes=saturated_stripes, grey_noise=grey_noise,
             ff_dense=ff_dense, deep_huffman=deep_huffman)
    return d


INPUTS = _builders()
FLAT_INPUTS = ["%s_%dx%d" % (name, h, w) for name in FLAT_VALUES for h, w in FLAT_SIZES] + ["blank_text_page"]


# ---- probes: what a file or a coefficient array holds -------------------------------------------------------------------------------
def segments(data: bytes) -> Tuple[List[Tuple[int, bytes]], int, int]:
    """a baseline file -> ([(marker, payload)] up to and including SOS, offset of the first scan byte, offset of EOI)"""
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    segs, p = [], 2
    while True:
        assert data[p] == 0xFF
        marker, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        segs.append((marker, data[p + 4:p + 2 + n]))
        p += 2 + n
        if marker == 0xDA:
            return segs, p, len(data) - 2


def dht_lengths(data: bytes) -> Dict[int, np.ndarray]:
    """{(class << 4 | id): number of codes of each length 1 .. 16} over the DHT segments (one table per segment, as libjpeg writes them)"""
    out = {}
    for marker, payload in segments(data)[0]:
        if marker == 0xC4:
            assert len(payload) == 17 + sum(payload[1:17])
            out[payload[0]] = np.frombuffer(payload[1:17], np.uint8).astype(np.int64)
    return out


def dht_symbol_counts(data: bytes) -> Dict[int, int]:
    return {k: int(v.sum()) for k, v in dht_lengths(data).items()}


def dqt_tables(data: bytes) -> List[np.ndarray]:
    return [np.frombuffer(payload[1:65], np.uint8) for marker, payload in segments(data)[0] if marker == 0xDB]


def unstuffed_scan(data: bytes) -> bytes:
    """the entropy-coded bytes as they were before byte stuffing"""
    _, p0, p1 = segments(data)
    scan = data[p0:p1]
    assert scan.count(b"\xff") == scan.count(b"\xff\x00")          # baseline, no restart markers: every 0xFF is a stuffed one
    return scan.replace(b"\xff\x00", b"\xff")


def ff_border_hits(stream: bytes) -> List[int]:
    """the k >= 1 with 0xFF at both PIECE * k - 1 and PIECE * k"""
    return [k for k in range(1, (len(stream) - 1) // PIECE + 1) if stream[PIECE * k - 1] == 0xFF and stream[PIECE * k] == 0xFF]


def _nbits(v: np.ndarray) -> np.ndarray:
    a = np.abs(v.astype(np.int64))
    return np.where(a > 0, np.floor(np.log2(np.maximum(a, 1))).astype(np.int64) + 1, 0)


def dc_categories(coefs: np.ndarray, height: int, width: int) -> np.ndarray:
    """categories of the luma DC differences in scan order (coefs: the oracle's [mcus, 6, 64])"""
    dc = coefs[:, :4, 0].astype(np.int64).ravel()
    return _nbits(np.diff(dc, prepend=0))


def max_ac_size(coefs: np.ndarray) -> int:
    return int(_nbits(coefs[:, :, 1:]).max())


def luma_ac_histogram(coefs: np.ndarray) -> np.ndarray:
    """run-length symbol counts [256] of the luma blocks, as the encoder's statistics pass counts them"""
    hist = np.zeros(256, np.int64)
    for blk in coefs[:, :4].reshape(-1, 64)[:, ZIGZAG]:
        nz = np.flatnonzero(blk[1:]) + 1
        prev = 0
        for k in nz:
            run = k - prev - 1
            hist[0xF0] += run // 16
            hist[((run % 16) << 4) + int(_nbits(blk[k:k + 1])[0])] += 1
            prev = k
        if prev != 63:
            hist[0] += 1
    return hist


def huffman_depth(hist: np.ndarray) -> int:
    """longest code of a plain (unlimited) Huffman code over the non-zero counts and the reserved pseudo-symbol of count 1"""
    heap = [(int(c), 0) for c in hist if c] + [(1, 0)]
    heapq.heapify(heap)
    while len(heap) > 1:
        (c1, d1), (c2, d2) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (c1 + c2, max(d1, d2) + 1))
    return heap[0][1]
