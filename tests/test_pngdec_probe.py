"""CPU: the host-only PNG probe (lumina_ocr_png_probe) on every seeded case of tests/png_cases.py, and on files it must call corrupt."""
import struct

import pytest

import png_cases as pc
from lumina_ocr.engine import Engine

CASES = pc.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_probe_status_and_info(case):
    name, data, rc = case
    got, info = Engine.png_probe(data)
    assert got == rc, (name, got, info)
    w, h, depth, ct, _, _, interlace = struct.unpack(">IIBBBBB", data[16:29])
    assert (info["width"], info["height"], info["bit_depth"], info["color_type"], info["interlace"]) == (w, h, depth, ct, interlace)
    if name.startswith("exif_o"):
        assert info["orientation"] == int(name[6:])
    else:
        assert info["orientation"] == 0


def test_palette_size():
    data = dict((n, d) for n, d, _ in CASES)["short_plte"]
    assert Engine.png_probe(data)[1]["palette_size"] == 5


@pytest.mark.parametrize("what", ["not_png", "empty", "jpeg", "bad_ihdr_crc", "truncated_header", "truncated_ihdr", "no_plte", "idat_first"])
def test_corrupt_headers(what):
    good = dict((n, d) for n, d, _ in CASES)["np_ct3_d8_29x45_f0"]
    data = {
        "not_png": b"GIF89a" + bytes(40),
        "empty": b"",
        "jpeg": b"\xff\xd8\xff\xe0" + bytes(60),
        "bad_ihdr_crc": good[:29] + bytes([good[29] ^ 0x10]) + good[30:],
        "truncated_header": good[:20],
        "truncated_ihdr": good[:31],
        "no_plte": pc.SIG + good[8:33] + good[good.index(b"IDAT") - 4:],
        "idat_first": pc.SIG + good[good.index(b"IDAT") - 4:],
    }[what]
    assert Engine.png_probe(data)[0] == -1


def test_provider_orientation_sources_without_decoding():
    """The provider's orientation for a lazily opened PNG: eXIf before IDAT is read, a file without one is 1, and a file whose orientation
    Pillow would take from a tEXt chunk ("Raw profile type exif", XMP) is left to the host path (None) — never decoded here."""
    import io

    import numpy as np
    from PIL import Image

    from lumina_ocr.services.ocr_service import OCRService
    by_name = dict((n, d) for n, d, _ in CASES)
    im = Image.open(io.BytesIO(by_name["exif_o6"]))
    assert OCRService._png_orientation(im) == 6 and im._im is None
    im = Image.open(io.BytesIO(by_name["np_ct2_d8_29x45_f4"]))
    assert OCRService._png_orientation(im) == 1 and im._im is None
    for kind, data in pc.text_orientation_files(Image.fromarray(pc.page_samples(np.random.default_rng(2), 20, 30, 3).astype(np.uint8).reshape(20, 30, 3))).items():
        im = Image.open(io.BytesIO(data))
        assert OCRService._png_orientation(im) is None, kind
        assert im._im is None
        assert Image.open(io.BytesIO(data)).getexif().get(0x0112) == 6, kind   # what the host path would apply
