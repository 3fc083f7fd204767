"""CPU: lumina_ocr_webp_probe / lumina_ocr_webp_reason through the C ABI (no handle, no device): statuses and info equal the restatement's
on intact, refused and damaged files, and every refusal names its reason."""
import struct

import pytest

import webp_cases as wc
import webp_reference as wr
import webp_writer as ww
from lumina_ocr.engine import Engine


def _same(data):
    rc, info = Engine.webp_probe(data)
    want_rc, want_info, want_reason = wr.probe(data)
    assert rc == want_rc and {k: info[k] for k in want_info} == want_info, (rc, want_rc, info, want_info)
    assert info["reason"] == want_reason
    return rc, info


def test_intact_and_refused_cases():
    for name, data in wc.writer_cases() + wc.pillow_cases()[::7]:
        rc, info = _same(data)
        assert rc == 0 and info["reason"] == "", name
    reasons = {name: _same(data)[1]["reason"] for name, data in wc.refused_cases()}
    assert reasons == {"lossy": "lossy WebP (VP8)", "lossy-alpha": "lossy WebP with an ALPH chunk", "animated": "animated WebP"}


def test_info_fields():
    by = dict(wc.writer_cases())
    rc, info = _same(by["vp8x-chunks"])
    assert rc == 0 and (info["width"], info["height"], info["alpha"], info["vp8x"], info["exif"], info["xmp"]) == (70, 9, 1, 1, 1, 0)
    rc, info = _same(by["green-alone"])
    assert (info["alpha"], info["vp8x"], info["exif"], info["xmp"]) == (0, 0, 0, 0)
    xmp = ww.write_vp8l(5, 3, [0xFF000000 | k for k in range(15)], vp8x=True, extra_chunks=[(b"XMP ", b"<x:xmpmeta/>", False)])
    assert _same(xmp)[1]["xmp"] == 1
    for w, h in ((16384, 1), (1, 16384)):
        rc, info = _same(by["wide-16384x1" if h == 1 else "tall-1x16384"])
        assert rc == 0 and (info["width"], info["height"]) == (w, h)


def _vp8l(data):
    p = data.index(b"VP8L")
    return p + 8


def _set(data, at, value):
    d = bytearray(data)
    d[at] = value
    return bytes(d)


def _rewrap(chunks):
    body = b"".join(chunks)
    return b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WEBP" + body


@pytest.mark.parametrize("name", ["bare", "vp8x"])
def test_every_refusal_names_its_reason(name):
    by = dict(wc.writer_cases())
    data = by["green-alone"] if name == "bare" else by["vp8x-chunks"]
    p = _vp8l(data)
    vp8l = ww.chunk(b"VP8L", data[p:p + struct.unpack("<I", data[p - 4:p])[0]])
    cases = {
        "not a RIFF / WEBP file": b"RIFX" + data[4:],
        "RIFF size past the file": data[:-2],
        "bytes after the RIFF payload": data + b"\0",
        "VP8L signature byte is not 0x2F": _set(data, p, 0x2E),
        "VP8L version is not 0": _set(data, p + 4, data[p + 4] | 0x20),
        "chunk past the file": _set(data, p - 1, 0x7F),
        "no chunk": _rewrap([]),
        "first chunk is neither VP8X, VP8L nor VP8": _rewrap([ww.chunk(b"EXIF", b"xx"), vp8l]),
        "chunks after the image of a file without VP8X": _rewrap([vp8l, ww.chunk(b"EXIF", b"xx")]),
    }
    if name == "vp8x":
        x = data.index(b"VP8X") + 8
        cases.update({
            "VP8X canvas differs from the VP8L header": _set(data, x + 4, data[x + 4] ^ 1),
            "reserved VP8X flag bits set": _set(data, x, data[x] | 0x80),
            "animated WebP": _set(data, x, data[x] | 0x02),
            "second VP8L chunk": _rewrap([data[12:30], vp8l, vp8l]),
            "second VP8X chunk": _rewrap([data[12:30], data[12:30], vp8l]),
            "no image chunk": _rewrap([data[12:30], ww.chunk(b"EXIF", b"xx")]),
            "VP8X chunk of another size than 10": _rewrap([ww.chunk(b"VP8X", data[20:30] + b"\0\0"), vp8l]),
            "lossy WebP with an ALPH chunk": _rewrap([data[12:30], ww.chunk(b"ALPH", b"\0\0"), vp8l]),
            "lossy WebP (VP8)": _rewrap([data[12:30], ww.chunk(b"VP8 ", b"\0\0"), vp8l]),
        })
    for reason, bad in cases.items():
        rc, info = _same(bad)
        assert rc in (-1, -2) and info["reason"] == reason, (reason, rc, info)
        assert rc == (-2 if reason.startswith(("lossy", "animated")) else -1), reason


def test_size_limit():
    """more than 2^26 pixels: -2; the longest lines are read (test_info_fields)"""
    data = ww.riff(bytes([0x2F]) + struct.pack("<I", (8192 - 1) | ((8193 - 1) << 14)) + b"\0", 8192, 8193)
    rc, info = _same(data)
    assert rc == -2 and info["reason"] == "more than 2^26 pixels"
    assert Engine.webp_probe(ww.riff(bytes([0x2F]) + struct.pack("<I", (8192 - 1) | ((8192 - 1) << 14)) + b"\0", 8192, 8192))[0] == 0


def test_generic_reasons():
    from lumina_ocr.engine import load_library
    lib = load_library()
    Engine.webp_probe(dict(wc.writer_cases())["green-alone"])
    assert lib.lumina_ocr_webp_reason(0) == b"read"
    assert lib.lumina_ocr_webp_reason(-1) == b"corrupt or irregular WebP file"
    assert lib.lumina_ocr_webp_reason(-2) == b"valid WebP that is not read"
    assert lib.lumina_ocr_webp_reason(-4) == b"another size than the batch"


def test_damaged_sample_statuses():
    for name, kind, data in wc.sweep_sample(400, seed=11):
        _same(data)
