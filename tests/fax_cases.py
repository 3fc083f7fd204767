"""Fax (T.4) test material shared by the CPU and GPU tests: libtiff (through Pillow) as the encoder of the five codings it writes and
as a second decoder, a policy encoder for legal codings libtiff never emits, the damage sweep, the committed fixtures.  The source
bitmaps are ccitt_cases.bitmaps()."""
import functools
import io
import json
import struct

import numpy as np
from PIL import Image

import ccitt_cases as cc

GOLDEN = cc.GOLDEN

# coding -> (TIFF Compression, T4Options, K, EncodedByteAlign): the last two are what lumina_ocr_fax_decode is told
MODES = {"1d": (3, 0, 0, 0), "2d": (3, 1, 1, 0), "1d_aligned": (3, 4, 0, 0), "2d_aligned": (3, 5, 1, 0), "rle": (2, None, 0, 1)}
EOL = "000000000001"


def g3_encode(black: np.ndarray, mode: str) -> bytes:
    """bool [rows][columns], True = black -> the one strip libtiff writes for it in that coding (coded black = True)"""
    comp, t4, _, _ = MODES[mode]
    im = Image.fromarray(np.where(black, 255, 0).astype(np.uint8)).convert("1")
    op = io.BytesIO()
    h, w = black.shape
    kw = {"tiffinfo": {292: t4}} if t4 is not None else {}
    im.save(op, "TIFF", compression="group3" if comp == 3 else "tiff_ccitt", strip_size=((w + 7) // 8) * h, **kw)
    tif = Image.open(io.BytesIO(op.getvalue()))
    (off,), (cnt,) = tif.tag_v2[273], tif.tag_v2[279]
    assert tif.tag_v2[262] == 1 and tif.tag_v2[259] == comp and (t4 is None or tif.tag_v2[292] == t4)
    return op.getvalue()[off:off + cnt]


def fax_tiff(stream: bytes, columns: int, rows: int, comp: int, t4opts, fill_order: int = 1, photometric: int = 0, rps=None) -> bytes:
    """the bare stream as the one strip of a classic little-endian TIFF"""
    data = bytes(stream) + b"\0" * (len(stream) & 1)
    tags = [(256, 4, columns), (257, 4, rows), (258, 3, 1), (259, 3, comp), (262, 3, photometric), (266, 3, fill_order), (273, 4, 8),
            (277, 3, 1), (278, 4, rows if rps is None else rps), (279, 4, len(stream))]
    if t4opts is not None:
        tags.append((292, 4, t4opts))
    ifd = struct.pack("<H", len(tags)) + b"".join(struct.pack("<HHII", t, ty, 1, v) for t, ty, v in sorted(tags)) + struct.pack("<I", 0)
    return b"II*\0" + struct.pack("<I", 8 + len(data)) + data + ifd


def libtiff_fax_bits(stream: bytes, columns: int, rows: int, comp: int, t4opts):
    """the bare stream as libtiff (through Pillow) decodes it under Compression `comp` (2 | 3) and T4Options `t4opts`: uint8
    [rows][columns], PDF's samples with BlackIs1 false (coded white = 1), or None where Pillow refuses the file (see
    ccitt_cases.libtiff_bits)"""
    try:
        im = Image.open(io.BytesIO(fax_tiff(stream, columns, rows, comp, t4opts)))
        a = np.asarray(im.convert("L"))
    except (OSError, ValueError, SyntaxError):
        return None
    assert a.shape == (rows, columns)
    return (a > 127).astype(np.uint8)


def intact_bitmaps():
    """name -> bool [rows][columns] (True = black): the shapes of the intact-stream tests"""
    maps = cc.bitmaps()
    out = {k: maps[k] for k in ("rand_65x40", "noise_67x40", "text_640x200", "begins_black_65x12", "extended_2700x4")}
    rng = np.random.default_rng(292)
    for w in (1, 7, 8, 9):
        out["rand_%dx6" % w] = rng.random((6, w)) < 0.4
    out["rand_1728x3"] = rng.random((3, 1728)) < 0.1
    out["white_8192x2"] = np.zeros((2, 8192), bool)
    out["black_8192x2"] = np.ones((2, 8192), bool)
    return out


# ---- the policy encoder: legal codings libtiff never writes ----
def line_1d_bits(line: np.ndarray) -> str:
    """one line as white and black runs in turn, white first; runs from 2560 up as repeated 2560 make-ups"""
    white_codes, black_codes = cc._policy_codes()[:2]
    px = np.concatenate(([False], np.asarray(line, bool), [not line[-1]]))
    edges = [0] + [int(x) for x in np.flatnonzero(px[1:] != px[:-1])]   # (a change at 0: the line begins black after a white run of 0)
    return "".join(cc._run_code(black_codes if k & 1 else white_codes, b - a) for k, (a, b) in enumerate(zip(edges, edges[1:])))


def line_2d_bits(above: np.ndarray, line: np.ndarray, seed: int, p_horiz: float) -> str:
    """one line coded against the one above by ccitt_cases.g4_encode_policy_bits' line coder (the coding of `above` against a white
    line, which it writes first, is cut off: with the same seed it is the same both times)"""
    both = cc.g4_encode_policy_bits(np.stack([above, line]), np.random.default_rng(seed), p_horiz)
    head = cc.g4_encode_policy_bits(np.asarray(above)[None], np.random.default_rng(seed), p_horiz)
    assert both.startswith(head)
    return both[len(head):]


def fax_encode_policy_bits(bitmap: np.ndarray, k: int = 0, eol: bool = True, align: bool = False, fill=(0,), one_d_rows=None,
                           rtc: bool = False, p_horiz: float = 0.3, seed: int = 11) -> str:
    """bool [rows][columns] (True = black) -> a T.4 stream.  eol: an EOL in front of every line, preceded by fill[y % len(fill)] zero
    bits.  k > 0: a tag bit after every EOL; the lines whose index is in one_d_rows (default: every k-th) are one-dimensional, the others
    two-dimensional (line 0 against a white line).  align (without eol): every line begins on a byte boundary.  rtc: six EOLs (each
    with its tag bit 1 when k > 0) after the last line.  As a string of '0' / '1' without padding."""
    rows, W = bitmap.shape
    if one_d_rows is None:
        one_d_rows = range(0, rows, max(k, 1))
    out = []
    for y in range(rows):
        if align and not eol:
            out.append("0" * (-sum(map(len, out)) % 8))
        if eol:
            out.append("0" * fill[y % len(fill)] + EOL)
        one_d = k <= 0 or y in one_d_rows
        if eol and k > 0:
            out.append("1" if one_d else "0")
        above = bitmap[y - 1] if y else np.zeros(W, bool)
        out.append(line_1d_bits(bitmap[y]) if one_d else line_2d_bits(above, bitmap[y], seed + y, p_horiz))
    if rtc:
        out.append((EOL + ("1" if k > 0 else "")) * 6)
    return "".join(out)


def fax_encode_policy(bitmap: np.ndarray, **kw) -> bytes:
    """fax_encode_policy_bits as bytes, the last one padded with zeros"""
    return cc.bits_to_bytes(fax_encode_policy_bits(bitmap, **kw))


def policy_cases():
    """name -> (bitmap, stream, K, align, (Compression, T4Options) libtiff reads it under | None)"""
    maps = cc.bitmaps()
    bm, ext, bb = maps["rand_65x40"], maps["extended_2700x4"], maps["begins_black_65x12"]
    wide = np.stack([np.ones(8192, bool), np.zeros(8192, bool), np.arange(8192) >= 2560 * 2])   # runs of 8192 and 5120: 2560 make-ups repeated
    enc = fax_encode_policy
    return {
        "fill_0_1_7_70_2100": (bm, enc(bm, fill=(0, 1, 7, 70, 2100)), 0, 0, (3, 0)),
        "fill_2d": (bm, enc(bm, k=4, fill=(3, 0, 2100, 9)), 4, 0, (3, 1)),
        "one_d_lines_anywhere": (bm, enc(bm, k=2, one_d_rows=(0, 1, 2, 5, 11, 12, 30, 39), p_horiz=0.5), 2, 0, (3, 1)),
        "first_line_two_d": (bb, enc(bb, k=2, one_d_rows=(3,), p_horiz=0.0), 2, 0, (3, 1)),
        "all_two_d_horizontal": (bm, enc(bm, k=1, one_d_rows=(), p_horiz=1.0), 1, 0, (3, 1)),
        "makeups_2560_1d": (wide, enc(wide), 0, 0, (3, 0)),
        "makeups_2560_2d": (wide, enc(wide, k=2, p_horiz=1.0), 2, 0, (3, 1)),
        "extended_rle": (ext, enc(ext, eol=False, align=True), 0, 1, (2, None)),
        "rtc_1d": (bm, enc(bm, rtc=True), 0, 0, (3, 0)),
        "rtc_2d": (bm, enc(bm, k=4, rtc=True), 4, 0, (3, 1)),
        "rtc_rle": (bm, enc(bm, eol=False, align=True, rtc=True), 0, 1, (2, None)),
        "no_eol_no_alignment": (bm, enc(bm, eol=False), 0, 0, None),   # PDF /K 0 as most writers emit it: libtiff cannot express it
        "no_eol_no_alignment_begins_black": (bb, enc(bb, eol=False), 0, 0, None),
    }


def hostile_cases():
    """name -> (stream, columns, rows, K, align, the status the restatement must give)"""
    maps = cc.bitmaps()
    bm = maps["rand_65x40"]
    enc = fax_encode_policy
    one_d = enc(bm)
    junk = np.random.default_rng(4243).integers(0, 256, 2048, dtype=np.uint8).tobytes()
    short_line = enc(bm[:, :64])          # every line one pixel short of 65 columns
    long_line = enc(np.concatenate([bm, bm[:, :1]], axis=1))
    mixed = cc.bits_to_bytes(fax_encode_policy_bits(bm[:20]) + fax_encode_policy_bits(bm[20:], eol=False))
    return {
        "truncated": (one_d[:len(one_d) // 2], 65, 40, 0, 0, -1),
        "junk": (junk, 65, 40, 0, 0, -1),
        "junk_2d": (junk, 65, 40, 4, 0, -2),                 # (its first bits are no EOL)
        "short_line": (short_line, 65, 40, 0, 0, -1),
        "long_line": (long_line, 65, 40, 0, 0, -1),
        "mixed_eol_and_none": (mixed, 65, 40, 0, 0, -1),
        "two_d_without_eol": (enc(bm, eol=False), 65, 40, 2, 0, -2),
        "aligned_with_eol": (one_d, 65, 40, 0, 1, -2),
        "two_eols_in_a_row": (cc.bits_to_bytes(EOL + "".join("{:08b}".format(x) for x in one_d)), 65, 40, 0, 0, -1),
        "ones_before_an_eol": (cc.flip_bit(enc(bm, fill=(0, 70)), _first_fill_bit(enc(bm, fill=(0, 70)))), 65, 40, 0, 0, -1),
        "zeros_to_the_end": (enc(bm[:3]) + b"\0" * 300, 65, 4, 0, 0, -1),
        "zero_run_inside_a_line": (cc.bits_to_bytes(EOL + "0111" + "0000110111" + "0111" + "0" * 40), 4, 1, 0, 0, -1),   # white 2, black 0, white 2
    }


def _first_fill_bit(stream: bytes) -> int:
    """the position of a fill bit of fax_encode_policy(.., fill=(0, 70)): 30 bits into the first run of 70 zeros or more"""
    bits = "".join("{:08b}".format(x) for x in stream)
    return bits.index("0" * 70) + 30


# ---- the damage sweep ----
SWEEP_FILES = ("rand_65x40", "begins_black_65x12")
SWEEP_MODES = ("1d", "2d", "rle")


@functools.lru_cache(maxsize=None)
def damage_sweep(name: str, mode: str):
    """(intact stream, columns, rows, [(label, damaged stream)]): libtiff's stream of the bitmap in that coding with every single bit
    flipped in turn, and cut at every byte length"""
    bm = cc.bitmaps()[name]
    stream, (rows, columns) = g3_encode(bm, mode), bm.shape
    damaged = [("bit %d" % b, cc.flip_bit(stream, b)) for b in range(len(stream) * 8)] + [("cut %d" % n, stream[:n]) for n in range(len(stream))]
    return stream, columns, rows, damaged


@functools.lru_cache(maxsize=None)
def sweep_restatement(name: str, mode: str):
    """[(status, bits)] of the restatement over damage_sweep(name, mode)'s streams: computed once, shared by the CPU and the GPU test"""
    import fax_reference as fr
    _, columns, rows, damaged = damage_sweep(name, mode)
    _, _, k, align = MODES[mode]
    return [fr.decode(d, columns, rows, k, bool(align)) for _, d in damaged]


# ---- committed streams ----
FIXTURES = (("rand_65x40", "1d"), ("rand_65x40", "2d"), ("rand_65x40", "rle"), ("begins_black_65x12", "2d_aligned"), ("noise_67x40", "1d_aligned"))


def write_fixtures():
    """(maintenance, needs libtiff) tests/golden/pdf/<name>.<coding>.g3 + fax_index.json with columns, rows, K, EncodedByteAlign and
    the SHA-256 of the expected samples"""
    maps, index = cc.bitmaps(), {}
    for name, mode in FIXTURES:
        bm = maps[name]
        key = "%s.%s" % (name, mode)
        (GOLDEN / (key + ".g3")).write_bytes(g3_encode(bm, mode))
        index[key] = {"columns": int(bm.shape[1]), "rows": int(bm.shape[0]), "K": MODES[mode][2], "EncodedByteAlign": MODES[mode][3],
                      "sha256_black_is_1_false": cc.sha(cc.expected_bits(bm, False)), "sha256_black_is_1_true": cc.sha(cc.expected_bits(bm, True))}
    (GOLDEN / "fax_index.json").write_text(json.dumps(index, indent=1, sort_keys=True) + "\n")


def fixtures():
    """name.coding -> (stream, columns, rows, K, EncodedByteAlign, {black_is_1: sha256 of the expected samples})"""
    index = json.loads((GOLDEN / "fax_index.json").read_text())
    return {k: ((GOLDEN / (k + ".g3")).read_bytes(), v["columns"], v["rows"], v["K"], v["EncodedByteAlign"],
                {False: v["sha256_black_is_1_false"], True: v["sha256_black_is_1_true"]}) for k, v in index.items()}


# ---- frames for the reader and the provider ----
def g3_frame(bitmap: np.ndarray, mode: str, photo=0, fill_order=1, rps=None, extra=None):
    """tiff_cases.g4_frame for the fax codings: bitmap bool [H][W], True = black; the strips are libtiff's"""
    import tiff_cases as tc
    comp, t4, _, _ = MODES[mode]
    h, w = bitmap.shape
    im = Image.fromarray(np.where(bitmap, 0, 255).astype(np.uint8)).convert("1")
    info = {278: rps or h, 262: photo}
    if t4 is not None:
        info[292] = t4
    _, strips, got_rps = tc.libtiff_strips(im, "group3" if comp == 3 else "tiff_ccitt", info)
    assert got_rps == (rps or h)
    if fill_order == 2:
        strips = [s.translate(tc.REVERSE) for s in strips]
    tags = tc.base_tags(w, h, comp, photo, 1, 1, rps, extra)
    if t4 is not None:
        tags[292] = (4, [t4])
    if fill_order != 1:
        tags[266] = fill_order
    return dict(strips=strips, tags=tags)
