"""Group 4 test material shared by the CPU and GPU tests: source bitmaps, libtiff (through Pillow) as the encoder, the committed fixtures."""
import hashlib
import io
import json
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
