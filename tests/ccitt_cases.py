"""Group 4 test material shared by the CPU and GPU tests: source bitmaps, libtiff (through Pillow) as the encoder and as a second
decoder, a second encoder that writes legal codings libtiff's never does, the damage sweep, the committed fixtures."""
import bisect
import functools
import hashlib
import io
import json
import struct
from pathlib import Path

import numpy as np
from PIL import Image, ImageDraw

GOLDEN = Path(__file__).resolve().parent / "golden" / "pdf"


def g4_encode(black: np.ndarray) -> bytes:
    """bool [rows][columns], True = black -> the T.6 strip libtiff writes for it (coded black = True), EOFB included"""
    im = Image.fromarray(np.where(black, 255, 0).astype(np.uint8)).convert("1")
    op = io.BytesIO()
    h, w = black.shape
    im.save(op, "TIFF", compression="group4", strip_size=((w + 7) // 8) * h)
    tif = Image.open(io.BytesIO(op.getvalue()))
    (off,), (cnt,) = tif.tag_v2[273], tif.tag_v2[279]
    assert tif.tag_v2[262] == 1, "expected BlackIsZero: Pillow then packs 255 as bit 1, which libtiff codes as a black run"
    return op.getvalue()[off:off + cnt]


def libtiff_bits(stream: bytes, columns: int, rows: int):
    """the bare T.6 stream as libtiff (through Pillow) decodes it: uint8 [rows][columns], PDF's samples with BlackIs1 false (coded white
    = 1), or None where Pillow refuses the file.  The stream is wrapped in a one-strip classic TIFF with Photometric 0 (WhiteIsZero),
    so a coded-white run comes out of convert('L') as 255."""
    data = bytes(stream) + b"\0" * (len(stream) & 1)
    tags = [(256, 4, columns), (257, 4, rows), (258, 3, 1), (259, 3, 4), (262, 3, 0), (273, 4, 8), (277, 3, 1), (278, 4, rows),
            (279, 4, len(stream))]
    ifd = struct.pack("<H", len(tags)) + b"".join(struct.pack("<HHII", t, ty, 1, v) for t, ty, v in tags) + struct.pack("<I", 0)
    tif = b"II*\0" + struct.pack("<I", 8 + len(data)) + data + ifd
    try:
        im = Image.open(io.BytesIO(tif))
        a = np.asarray(im.convert("L"))
    except (OSError, ValueError, SyntaxError):
        return None
    assert a.shape == (rows, columns)
    return (a > 127).astype(np.uint8)


_POLICY_CODES = None


def _policy_codes():
    """({run: code} for white, for black, {mode: code}) from the restatement's code lists"""
    global _POLICY_CODES
    if _POLICY_CODES is None:
        import ccitt_reference as cr
        _POLICY_CODES = ({r: c for c, r in cr.run_codes(True)}, {r: c for c, r in cr.run_codes(False)}, {m: c for c, m in cr.MODE_CODES.items()},
                         {d: m for m, d in cr.V_DELTA.items()}, cr.M_PASS, cr.M_HORIZ)
    return _POLICY_CODES


def _run_code(codes: dict, n: int) -> str:
    """one run length: 2560 make-ups while 2560 or more remain, one make-up for what is left above 63, a terminating code"""
    out = []
    while n >= 2560:
        out.append(codes[2560])
        n -= 2560
    if n >= 64:
        out.append(codes[n & ~63])
    out.append(codes[n & 63])
    return "".join(out)


def g4_encode_policy_bits(bitmap: np.ndarray, rng, p_horiz: float, stats: dict = None) -> str:
    """the lines of `bitmap` (bool [rows][columns], True = black) by the T.6 coding procedure as a string of '0' / '1', no
    EOFB and no padding.  Pass mode where b2 lies left of a1; else vertical mode where |a1 - b1| <= 3, except that with probability
    `p_horiz` the pair is coded in horizontal mode instead (always legal: the decoder needs no more than the two run lengths); else
    horizontal mode.  stats, if given, counts the codes by mode ('pass', 'vertical', 'horizontal')."""
    white_codes, black_codes, mode_codes, v_mode, m_pass, m_horiz = _policy_codes()
    rows, W = bitmap.shape
    out = []
    count = {"pass": 0, "vertical": 0, "horizontal": 0}
    ref = []   # changing elements of the imaginary white line
    for y in range(rows):
        px = np.concatenate(([False], np.asarray(bitmap[y], bool)))
        cur = [int(x) for x in np.flatnonzero(px[1:] != px[:-1])]   # element k changes to black when k is even
        c, r = cur + [W, W], ref + [W, W, W]
        a0, white, ci = -1, True, 0
        while a0 < W:
            a1, a2 = c[ci], c[ci + 1]
            ri = bisect.bisect_right(ref, a0)      # the first changing element right of a0 ...
            ri += (ri & 1) != (0 if white else 1)  # ... that changes to the colour opposite to a0's
            b1, b2 = r[ri], r[ri + 1]
            if b2 < a1:
                out.append(mode_codes[m_pass])
                count["pass"] += 1
                a0 = b2
            elif abs(a1 - b1) <= 3 and not rng.random() < p_horiz:
                out.append(mode_codes[v_mode[a1 - b1]])
                count["vertical"] += 1
                a0, white, ci = a1, not white, ci + 1
            else:
                start = max(a0, 0)
                first, second = (white_codes, black_codes) if white else (black_codes, white_codes)
                out.append(mode_codes[m_horiz] + _run_code(first, a1 - start) + _run_code(second, a2 - a1))
                count["horizontal"] += 1
                a0, ci = a2, ci + 2
        ref = cur
    if stats is not None:
        stats.update(count)
    return "".join(out)


def bits_to_bytes(bits: str) -> bytes:
    """'0' / '1' -> bytes, MSB first, the last byte padded with zeros"""
    bits += "0" * (-len(bits) % 8)
    return int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""


def g4_encode_policy(bitmap: np.ndarray, rng, p_horiz: float, eofb: bool = True, stats: dict = None) -> bytes:
    """a second Group 4 encoder (see g4_encode_policy_bits), for legal streams that libtiff never writes; EOFB is optional"""
    return bits_to_bytes(g4_encode_policy_bits(bitmap, rng, p_horiz, stats) + ("000000000001" * 2 if eofb else ""))


def policy_bitmaps():
    """name -> bool [rows][columns] (True = black): the shapes at which the decoder's line stage and its bounds can go wrong"""
    rng = np.random.default_rng(4106)
    out = {}
    for w in (1, 2, 31, 32, 33, 63, 64, 65, 2049):   # the finished line is built in 32-pixel words
        for density in (0.05, 0.5):
            out["rand_%dx6_%g" % (w, density)] = rng.random((6, w)) < density
    first = rng.random((2, 65)) < 0.3
    first[:, 0] = True
    out["begins_black_under_begins_black"] = first
    out["black_8192_over_white"] = np.stack([np.ones(8192, bool), np.zeros(8192, bool)])   # three 2560 make-ups, then 512 + 0
    widest = np.repeat(np.random.default_rng(8).random((3, 4096)) < 0.5, 2, axis=1)
    widest[1] = (np.arange(8192) & 1) == 0   # 8192 changing elements on one line (test_widest_line_and_rows)
    out["alternating_8192"] = widest
    return out


def exact_fit_stream(p_horiz: float):
    """(bitmap, stream): a stream whose last line ends on the last bit of its last byte, with no EOFB and no padding bit"""
    rng = np.random.default_rng(515)
    for _ in range(200):
        bm = rng.random((5, 33)) < 0.4
        bits = g4_encode_policy_bits(bm, np.random.default_rng(1), p_horiz)
        if len(bits) % 8 == 0:
            return bm, bits_to_bytes(bits)
    raise AssertionError("no bitmap whose coding fills its last byte")


def flip_bit(stream: bytes, bit: int) -> bytes:
    """bits are counted MSB first"""
    d = bytearray(stream)
    d[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(d)


SWEEP_FILES = ("begins_black_65x12", "rand_65x40", "rand_7x9")


@functools.lru_cache(maxsize=None)
def damage_sweep(name: str):
    """(intact stream, columns, rows, [(label, damaged stream)]): every single-bit flip of begins_black_65x12 and of libtiff's stream
    for rand_7x9, the flips in the first and the last 512 bits of rand_65x40, and each stream cut at every byte length"""
    if name == "rand_7x9":
        bm = bitmaps()[name]
        stream, (rows, columns) = g4_encode(bm), bm.shape
    else:
        stream, columns, rows, _ = fixtures()[name]
    nbits = len(stream) * 8
    flips = range(nbits) if name != "rand_65x40" else sorted(set(range(512)) | set(range(nbits - 512, nbits)))
    damaged = [("bit %d" % b, flip_bit(stream, b)) for b in flips] + [("cut %d" % k, stream[:k]) for k in range(len(stream))]
    return stream, columns, rows, damaged


@functools.lru_cache(maxsize=None)
def sweep_restatement(name: str):
    """[(status, bits)] of the restatement over damage_sweep(name)'s streams: computed once, shared by the CPU and the GPU test"""
    import ccitt_reference as cr
    _, columns, rows, damaged = damage_sweep(name)
    return [cr.decode(d, columns, rows) for _, d in damaged]


def expected_bits(black: np.ndarray, black_is_1: bool) -> np.ndarray:
    """PDF's sample values for the source bitmap: coded white -> 1 unless BlackIs1"""
    return (black == bool(black_is_1)).astype(np.uint8)


def text_bitmap(w=640, h=200) -> np.ndarray:
    im = Image.new("L", (w, h), 255)
    d = ImageDraw.Draw(im)
    for k, line in enumerate(["Invoice 2041-77: 3 x widget @ 19.50", "The quick brown fox jumps over the lazy dog", "TOTAL DUE 58.50 EUR -- net 30 days"]):
        d.text((12 + 7 * k, 20 + 55 * k), line, fill=0, font_size=28)
    return np.asarray(im) < 128


def bitmaps():
    """name -> bool [rows][columns] (True = black)"""
    rng = np.random.default_rng(20260)
    out = {}
    for w, h in ((1, 5), (7, 9), (8, 16), (65, 40), (1000, 12)):
        out["rand_%dx%d" % (w, h)] = rng.random((h, w)) < 0.3
        out["white_%dx%d" % (w, h)] = np.zeros((h, w), bool)
        out["black_%dx%d" % (w, h)] = np.ones((h, w), bool)
    yy, xx = np.mgrid[0:20, 0:65]
    out["checker_65x20"] = ((yy + xx) & 1) == 1
    out["checker4_65x20"] = (((yy // 4) + (xx // 4)) & 1) == 0
    first = rng.random((12, 65)) < 0.2
    first[:, 0] = True                     # every line begins black
    out["begins_black_65x12"] = first
    out["noise_67x40"] = np.random.default_rng(7).random((40, 67)) < 0.5
    out["text_640x200"] = text_bitmap()
    ext = np.zeros((4, 2700), bool)
    ext[0, 2600:2650] = True               # one black run after 2600 white pixels
    ext[1, :] = True                       # a black run over the whole line (2560 + make-up + terminating)
    ext[3, 40:] = True                     # a white-to-edge line above, then 2660 black pixels
    out["extended_2700x4"] = ext
    return out


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, np.uint8).tobytes()).hexdigest()


FIXTURES = ("rand_65x40", "noise_67x40", "text_640x200", "extended_2700x4", "begins_black_65x12")


def write_fixtures():
    """(maintenance, needs libtiff) tests/golden/pdf/<name>.g4 + index.json with columns, rows and the SHA-256 of the expected samples"""
    GOLDEN.mkdir(parents=True, exist_ok=True)
    maps, index = bitmaps(), {}
    for name in FIXTURES:
        bm = maps[name]
        (GOLDEN / (name + ".g4")).write_bytes(g4_encode(bm))
        index[name] = {"columns": int(bm.shape[1]), "rows": int(bm.shape[0]),
                       "sha256_black_is_1_false": sha(expected_bits(bm, False)), "sha256_black_is_1_true": sha(expected_bits(bm, True))}
    (GOLDEN / "index.json").write_text(json.dumps(index, indent=1, sort_keys=True) + "\n")


def fixtures():
    """name -> (stream, columns, rows, {black_is_1: sha256 of the expected samples})"""
    index = json.loads((GOLDEN / "index.json").read_text())
    return {k: ((GOLDEN / (k + ".g4")).read_bytes(), v["columns"], v["rows"], {False: v["sha256_black_is_1_false"], True: v["sha256_black_is_1_true"]})
            for k, v in index.items()}
