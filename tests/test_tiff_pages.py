"""CPU: the TIFF container reader (lumina_ocr/utils/tiff_pages.py) over the files of the tests' own writer (tests/tiff_cases.py): tag
defaults, II and MM, FillOrder 2, several frames; and every refusal, each with its reason, none raising or running long."""
import io
import struct
import time

import numpy as np
import pytest
from PIL import Image, features

import tiff_cases as tc
from lumina_ocr.utils import tiff_pages as tp

needs_libtiff = pytest.mark.skipif(not features.check("libtiff"), reason="libtiff is the Group 4 encoder of these cases")


def one(data):
    pages = tp.read_pages(data)
    assert len(pages) == 1
    return pages[0]


def reason(data):
    p = one(data)
    assert isinstance(p, tp.TiffRefused), p
    return p.reason


def grey(extra=None):
    a = tc.noise(10, 20)
    f = tc.frame(a, 20, tc.LZW, rps=4)
    f["tags"].update(extra or {})
    return f


@pytest.mark.parametrize("name", list(tc.strip_cases()))
def test_reader_gives_the_cases_their_parameters(name):
    c = tc.strip_cases()[name]
    p = one(c["file"])
    assert isinstance(p, tp.PageImage), getattr(p, "reason", None)
    assert (p.width, p.height, p.rows_per_strip) == (c["width"], c["height"], c["rps"])
    assert p.strip_params() == c["params"] and p.palette == c["palette"] and [bytes(s) for s in p.strips] == c["strips"]
    assert p.orientation == 1 and p.fill_order == 1


def test_tag_defaults():
    a = tc.noise(6, 5)
    tags = {256: 5, 257: 6, 258: 8, 262: 1}      # no Compression, SamplesPerPixel, RowsPerStrip, Planar, Predictor, FillOrder, Orientation
    p = one(tc.tiff_file([dict(strips=[a.tobytes()], tags=tags)]))
    assert (p.codec, p.rows_per_strip, p.components, p.bits, p.predictor, p.fill_order, p.orientation, p.invert, p.indexed) == \
        ("none", 6, 1, 8, 1, 1, 1, False, False)
    assert np.array_equal(tc.pillow_rgb(tc.tiff_file([dict(strips=[a.tobytes()], tags=tags)]))[:, :, 0], a)
    del tags[258]                                 # BitsPerSample defaults to 1
    p = one(tc.tiff_file([dict(strips=[bytes(6)], tags=tags)]))
    assert p.bits == 1
    # RowsPerStrip larger than the image (libtiff writes 2^32 - 1 for "one strip")
    tags[258] = 8
    tags[278] = (4, [0xFFFFFFFF])
    assert one(tc.tiff_file([dict(strips=[a.tobytes()], tags=tags)])).rows_per_strip == 6
    # Deflate under both of its numbers
    for comp in (8, 32946):
        t = dict(tags)
        t[259] = comp
        assert one(tc.tiff_file([dict(strips=[a.tobytes()], tags=t)])).codec == "deflate"


def test_byte_orders_agree():
    for big in (False, True):
        f = tc.tiff_file([tc.frame(tc.smooth_rgb(12, 9), 9, tc.LZW, photo=2, spp=3, rps=5, predictor=2, extra={274: 6}),
                          tc.frame(tc.pack_bits(tc.noise(7, 33, top=16), 4), 33, tc.PACKBITS, photo=3, bits=4)], big_endian=big)
        assert f[:4] == (b"MM\x00*" if big else b"II*\x00")
        a, b = tp.read_pages(f)
        assert (a.width, a.height, a.codec, a.rows_per_strip, a.predictor, a.components, a.orientation, len(a.strips)) == (9, 12, "lzw", 5, 2, 3, 6, 3)
        assert (b.width, b.height, b.codec, b.bits, b.indexed, len(b.strips)) == (33, 7, "packbits", 4, True, 1)
        assert b.palette[:48] == bytes(v // 256 for i in range(16) for v in tc.PALETTE16[i]) and b.palette[48:] == bytes(720)
        assert tc.pillow_rgb(f, 0).shape == (9, 12, 3) and tc.pillow_rgb(f, 1).shape == (7, 33, 3)


def test_palette_entry_is_colormap_value_floor_256_as_in_pillow():
    c = tc.strip_cases()["lzw_pal8_331"]
    pal = np.frombuffer(one(c["file"]).palette, np.uint8).reshape(256, 3)
    idx = tc.noise(21, 331, seed=14)
    assert np.array_equal(pal[idx], tc.pillow_rgb(c["file"]))


@needs_libtiff
def test_fill_order_2_and_three_frames():
    bm = np.random.default_rng(3).random((50, 130)) < 0.1
    plain = tc.g4_frame(bm, 0, 1, rps=16)
    f = tc.tiff_file([tc.g4_frame(bm, 0, 2, rps=16), grey(), tc.frame(tc.smooth_rgb(12, 9), 9, tc.NONE, photo=2, spp=3)], big_endian=True)
    a, b, c = tp.read_pages(f)
    assert (a.codec, a.fill_order, a.bits, a.invert, a.rows_per_strip, a.ccitt_params()) == ("group4", 2, 1, True, 16, (-1, 0, 0, 0))
    assert [bytes(s) for s in a.strips] == plain["strips"]          # the bits of each byte reversed back
    assert (b.codec, b.width, b.height, len(b.strips)) == ("lzw", 20, 10, 3) and (c.codec, c.components) == ("none", 3)
    assert one(tc.tiff_file([tc.g4_frame(bm, 1)])).ccitt_params() == (-1, 0, 0, 1)
    for k, shape in enumerate([(50, 130, 3), (10, 20, 3), (12, 9, 3)]):
        assert tc.pillow_rgb(f, k).shape == shape


REFUSALS = [
    ("BigTIFF", lambda: tc.tiff_file([grey()], magic=43)),
    ("tiled", lambda: tc.tiff_file_with_tiles([tc.tiled_frame()[0]])),
    ("PlanarConfiguration 2", lambda: tc.tiff_file([tc.frame(tc.smooth_rgb(4, 4), 4, tc.NONE, photo=2, spp=3, extra={284: 2})])),
    ("ExtraSamples", lambda: tc.tiff_file([dict(strips=[bytes(64)], tags=tc.base_tags(4, 4, 1, 2, 8, 4, extra={338: 2}))])),
    ("4 samples", lambda: tc.tiff_file([dict(strips=[bytes(64)], tags=tc.base_tags(4, 4, 1, 2, 8, 4))])),
    ("16-bit", lambda: tc.tiff_file([dict(strips=[bytes(32)], tags=tc.base_tags(4, 4, 1, 1, 16))])),
    ("SampleFormat", lambda: tc.tiff_file([grey({339: 3})])),
    ("4 samples", lambda: tc.tiff_file([dict(strips=[bytes(64)], tags=tc.base_tags(4, 4, 1, 5, 8, 4))])),      # CMYK as written
    ("CMYK", lambda: tc.tiff_file([grey({262: 5})])),
    ("YCbCr", lambda: tc.tiff_file([grey({262: 6})])),
    ("Lab", lambda: tc.tiff_file([grey({262: 8})])),
    ("JPEG-in-TIFF", lambda: tc.tiff_file([grey({259: 6})])),
    ("JPEG-in-TIFF", lambda: tc.tiff_file([grey({259: 7})])),
    ("Group 3", lambda: tc.tiff_file([grey({259: 3})])),
    ("Group 3", lambda: tc.tiff_file([grey({259: 2})])),
    ("Compression 34712", lambda: tc.tiff_file([grey({259: 34712})])),
    ("uncompressed mode", lambda: tc.tiff_file([dict(strips=[b"\x00\x10\x01"], tags=tc.base_tags(8, 2, 4, 0, 1, extra={293: 2}))])),
    ("Group 4 wider", lambda: tc.tiff_file([dict(strips=[b"\x00\x10\x01"], tags=tc.base_tags(8193, 2, 4, 0, 1))])),
    ("FillOrder 2", lambda: tc.tiff_file([grey({266: 2})])),
    ("Predictor 2", lambda: tc.tiff_file([tc.frame(tc.pack_bits(tc.noise(4, 8, top=16), 4), 8, tc.LZW, bits=4, extra={317: 2})])),
    ("Predictor 2 with compression packbits", lambda: tc.tiff_file([tc.frame(tc.noise(6, 9), 9, tc.PACKBITS, predictor=2)])),
    ("Predictor 2 with compression none", lambda: tc.tiff_file([tc.frame(tc.smooth_rgb(6, 9), 9, tc.NONE, photo=2, spp=3, predictor=2)])),
    ("Predictor 2 with compression group4", lambda: tc.tiff_file([dict(strips=[b"\x00\x10\x01"], tags=tc.base_tags(8, 2, 4, 0, 8, extra={317: 2}))])),
    ("XMP packet without an Orientation", lambda: tc.tiff_file([grey({700: (1, list(XMP6))})])),
    ("tag 256 occurs twice", lambda: _patch_tag(tc.tiff_file([grey({255: 65})]), 255, 256)),
    ("Predictor 3", lambda: tc.tiff_file([grey({317: 3})])),
    ("Orientation 9", lambda: tc.tiff_file([grey({274: 9})])),
    ("strip outside", lambda: tc.tiff_file([grey({273: (4, [8, 20, 1 << 30])})])),
    ("strip outside", lambda: tc.tiff_file([grey({279: (4, [5, 5, 0x7FFFFFFF])})])),
    ("empty strip", lambda: tc.tiff_file([grey({279: (4, [5, 0, 5])})])),
    ("for 2 strips", lambda: tc.tiff_file([grey({278: 5})])),                      # ceil(10 / 5) = 2 strips wanted, 3 stored
    ("RowsPerStrip 0", lambda: tc.tiff_file([grey({278: 0})])),
    ("image size", lambda: tc.tiff_file([grey({256: 0})])),
    ("image size", lambda: tc.tiff_file([grey({257: (4, [70000])})])),
    ("ColorMap", lambda: tc.tiff_file([grey({262: 3})])),
    ("no PhotometricInterpretation", lambda: tc.tiff_file([{"strips": [bytes(4)], "tags": {256: 2, 257: 2, 258: 8}}])),
]


@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_refusals_have_reasons(k):
    word, make = REFUSALS[k]
    t0 = time.time()
    r = reason(make())
    assert word in r, r
    assert time.time() - t0 < 1


XMP6 = (b'<?xpacket begin="" id="W5M0MpCehiHzreSzNTczkc9d"?><x:xmpmeta xmlns:x="adobe:ns:meta/"><rdf:RDF xmlns:rdf="http://www.w3.org/1999/02/'
        b'22-rdf-syntax-ns#"><rdf:Description xmlns:tiff="http://ns.adobe.com/tiff/1.0/" tiff:Orientation="6"/></rdf:RDF></x:xmpmeta><?xpacket end="r"?>')


def _patch_tag(data: bytes, old: int, new: int) -> bytes:
    """the id of entry `old` in the first IFD of a little-endian file becomes `new`"""
    b = bytearray(data)
    n = struct.unpack_from("<H", b, 8)[0]
    for k in range(n):
        if struct.unpack_from("<H", b, 10 + 12 * k)[0] == old:
            struct.pack_into("<H", b, 10 + 12 * k, new)
            return bytes(b)
    raise KeyError(old)


def test_what_pillow_reads_differently_from_the_tags_is_refused():
    """the three refusals above are no whims: Pillow / libtiff ignore Predictor 2 outside LZW and Deflate, take tiff:Orientation from an
    XMP packet when tag 274 is absent, and keep the last of a repeated tag"""
    a = tc.noise(6, 9)
    assert np.array_equal(tc.pillow_rgb(tc.tiff_file([tc.frame(a, 9, tc.PACKBITS, predictor=2)]))[:, :, 0], tc.predict(a, 1))   # left as stored
    assert np.array_equal(tc.pillow_rgb(tc.tiff_file([tc.frame(a, 9, tc.LZW, predictor=2)]))[:, :, 0], a)
    assert tc.pillow_rgb(tc.tiff_file([grey({700: (1, list(XMP6))})])).shape == (20, 10, 3)                                   # turned
    with_tag = tc.tiff_file([grey({700: (1, list(XMP6)), 274: 1})])
    assert tc.pillow_rgb(with_tag).shape == (10, 20, 3) and one(with_tag).orientation == 1                                    # tag 274 wins
    twice = _patch_tag(tc.tiff_file([grey({255: 7})]), 255, 256)               # ImageWidth 7, then 20
    assert Image.open(io.BytesIO(twice)).size == (20, 10)                      # Pillow's header keeps the last, libtiff beneath it does not
    with pytest.raises(OSError):
        tc.pillow_rgb(twice)


def test_max_pages_stops_the_walk():
    f = tc.tiff_file([grey(), grey(), dict(grey(), next=1 << 31)])
    assert one(f).whole_file                                        # the chain is broken behind the third IFD
    first = tp.read_pages(f, max_pages=1)
    assert len(first) == 1 and isinstance(first[0], tp.PageImage)   # which a reader of the first page never looks at
    assert len(tp.read_pages(f, max_pages=2)) == 2


def _patch_count(data: bytes, tag: int, count: int) -> bytes:
    """the count field of `tag` in the first IFD of a little-endian file"""
    b = bytearray(data)
    n = struct.unpack_from("<H", b, 8)[0]
    for k in range(n):
        if struct.unpack_from("<H", b, 10 + 12 * k)[0] == tag:
            struct.pack_into("<I", b, 10 + 12 * k + 4, count)
            return bytes(b)
    raise KeyError(tag)


def test_broken_structure_refuses_without_raising_or_running_long():
    good = tc.tiff_file([grey(), grey(), grey()])
    assert len(tp.read_pages(good)) == 3
    t0 = time.time()
    # an IFD chain looping back to the first IFD / to itself
    loop = tc.tiff_file([grey(), dict(grey(), next=8)])
    assert "revisits" in reason(loop) and one(loop).whole_file
    # a first IFD offset and a next-IFD offset outside the file
    assert "outside the file" in reason(good[:4] + struct.pack("<I", len(good) + 10) + good[8:])
    assert "outside the file" in reason(tc.tiff_file([dict(grey(), next=1 << 31)]))
    # a strip count of 2^31 (and a byte-count count of 2^31)
    for tag in (273, 279):
        r = reason(_patch_count(tc.tiff_file([grey()]), tag, 1 << 31))
        assert "tag %d with %d values" % (tag, 1 << 31) in r
    assert "outside the file" in reason(_patch_count(tc.tiff_file([grey()]), 273, 1 << 19))
    # not a TIFF, too short
    for junk in (b"", b"II", b"II*\x00", b"PK\x03\x04" + bytes(40), b"MM\x00*\x00\x00\x00\x04" + bytes(40)):
        assert one(junk).whole_file
    # more IFDs than the page cap
    old = tp.MAX_PAGES
    tp.MAX_PAGES = 2
    try:
        assert "more than 2 IFDs" in reason(good)
    finally:
        tp.MAX_PAGES = old
    assert time.time() - t0 < 1


def test_truncated_at_every_97th_byte():
    f = tc.tiff_file([grey(), tc.frame(tc.smooth_rgb(12, 9), 9, tc.PACKBITS, photo=2, spp=3, rps=5), grey({274: 3})], big_endian=True)
    t0 = time.time()
    for n in range(0, len(f), 97):
        pages = tp.read_pages(f[:n])
        assert pages and all(isinstance(p, (tp.PageImage, tp.TiffRefused)) for p in pages)
        assert any(isinstance(p, tp.TiffRefused) for p in pages), n     # the last strip ends the file: every cut loses something
        for p in pages:
            if isinstance(p, tp.PageImage):
                assert all(len(s) > 0 for s in p.strips)
    assert time.time() - t0 < 1
    assert all(isinstance(p, tp.PageImage) for p in tp.read_pages(f))
