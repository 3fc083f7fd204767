"""GPU: scanned TIFFs through the provider with LUMINA_OCR_DEVICE_TIFF (OCRService.device_tiff), synthetic weights.  The strips are
decoded on the device, byte-identical to Pillow, so every result must equal the one with the option off; process_tiff_sync reads every
page of a multi-page file, leaves what the reader or a decoder refuses to Pillow, and turns a page nobody decodes into that page's error."""
import asyncio

import numpy as np
import pytest
from PIL import Image, features

import ccitt_cases as cc
import tiff_cases as tc
from lumina_ocr import synth

pytestmark = pytest.mark.gpu
needs_libtiff = pytest.mark.skipif(not features.check("libtiff"), reason="libtiff is the Group 4 encoder of these cases")

W, H = 700, 1000


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    s._allow_synthetic = True
    saved = s.device_tiff
    yield s
    s.device_tiff = saved
    s.cleanup()


@pytest.fixture(scope="module")
def pages():
    return [synth.synth_page(H, W, seed, n_lines=12)[0] for seed in (31, 32)] + [synth.synth_page(800, 600, 33, n_lines=9)[0]]


def _untimed(v):
    if isinstance(v, dict):
        return {k: _untimed(x) for k, x in v.items() if "time" not in k}
    if isinstance(v, list):
        return [_untimed(x) for x in v]
    return v


def _same(a, b):
    return _untimed(a.to_dict()) == _untimed(b.to_dict())


def _black(page):
    return page.mean(axis=2) < 128


def _grey(page):
    return np.asarray(Image.fromarray(page).convert("L"))


def _frames(pages):
    """name -> one frame of tiff_file per codec"""
    h, w = pages[0].shape[:2]
    rgb = pages[0].reshape(h, w * 3)
    return {
        "none": lambda: tc.frame(rgb, w, tc.NONE, photo=2, spp=3, rps=100),
        "lzw": lambda: tc.libtiff_frame(rgb, w, photo=2, spp=3, rps=13, predictor=2),
        "packbits": lambda: tc.frame(_grey(pages[0]), w, tc.PACKBITS, rps=64),
        "deflate": lambda: tc.frame(rgb, w, tc.DEFLATE, photo=2, spp=3, rps=50, predictor=2),            # 20 full strips
        "deflate_last_strip": lambda: tc.frame(_grey(pages[0]), w, tc.DEFLATE, rps=64, extra={259: 32946}),  # 15 full strips and one of 40 rows
        "group4": lambda: tc.g4_frame(_black(pages[0]), 0, 1, rps=64),
        "group4_minisblack_one_strip": lambda: tc.g4_frame(_black(pages[0]), 1, 1),
    }


def _on_and_off(s, source):
    s.device_tiff = False
    off = s.process_image_sync(source)
    s.device_tiff = True
    seen = []
    inner = s._decode_tiff_pages
    s._decode_tiff_pages = lambda entries, reasons: seen.append(inner(entries, reasons)) or seen[-1]
    try:
        on = s.process_image_sync(source)
    finally:
        del s._decode_tiff_pages
    assert seen and list(seen[0]) == [0], "the device did not decode the page"
    assert off.success and off.layout_boxes, off.error
    return on, off


@needs_libtiff
@pytest.mark.parametrize("codec", ["none", "lzw", "packbits", "deflate", "deflate_last_strip", "group4", "group4_minisblack_one_strip"])
def test_one_page_file_equals_option_off(service, pages, codec, tmp_path):
    data = tc.tiff_file([_frames(pages)[codec]()])
    on, off = _on_and_off(service, data)
    assert _same(on, off)
    if codec == "lzw":      # a path, too
        p = tmp_path / "scan.tiff"
        p.write_bytes(data)
        on, off = _on_and_off(service, p)
        assert _same(on, off)
        assert service.get_status()["device_tiff"] is True


@needs_libtiff
@pytest.mark.parametrize("kind", ["orientation6", "mm", "fillorder2"])
def test_orientation_byte_order_and_fill_order(service, pages, kind):
    h, w = pages[0].shape[:2]
    if kind == "orientation6":
        lying = np.ascontiguousarray(np.rot90(pages[0], 1))      # Orientation 6 turns it upright again
        data = tc.tiff_file([tc.libtiff_frame(lying.reshape(w, h * 3), h, photo=2, spp=3, rps=16, extra={274: 6})])
        assert np.array_equal(tc.pillow_rgb(data), pages[0])
    elif kind == "mm":
        data = tc.tiff_file([_frames(pages)["lzw"]()], big_endian=True)
    else:
        data = tc.tiff_file([tc.g4_frame(_black(pages[0]), 0, 2, rps=64)], big_endian=True)
    on, off = _on_and_off(service, data)
    assert _same(on, off)
    assert (on.image_width, on.image_height) == (w, h)


@needs_libtiff
@pytest.mark.parametrize("height", [48, 50])       # RowsPerStrip 16: three full strips, and three with a last strip of two rows
def test_in_place_strip_decode_pixels_equal_pillow(service, height):
    """Group 4 and Deflate pages through the one-image decoders, strip by strip: three same-shape pages a group (the full strips of all
    of them in one call, the last strips in another), every pixel against Pillow's frame"""
    from lumina_ocr.utils import tiff_pages
    s = service
    s._ensure_engine()
    w, rng = 131, np.random.default_rng(height)
    frames = [tc.g4_frame(rng.random((height, w)) < 0.2, k % 2, 1 + k % 2, rps=16) for k in range(3)]
    frames += [tc.frame(tc.smooth_rgb(height, w) + np.uint8(k), w, tc.DEFLATE, photo=2, spp=3, rps=16, predictor=2) for k in range(3)]
    frames += [tc.frame(tc.pack_bits(tc.noise(height, w, seed=9, top=16), 4), w, tc.DEFLATE, photo=3, bits=4, rps=16), tc.g4_frame(rng.random((height, w)) < 0.5, 0, 1)]
    data = tc.tiff_file(frames)
    entries = tiff_pages.read_pages(data)
    assert all(isinstance(e, tiff_pages.PageImage) for e in entries)
    reasons = {}
    got = s._decode_tiff_pages(entries, reasons)
    assert sorted(got) == list(range(len(frames))) and reasons == {}
    for k in range(len(frames)):
        assert np.array_equal(got[k][0].cpu().numpy(), tc.pillow_rgb(data, k)), k
    # a damaged strip in the middle page of a group: that page alone is refused
    bad = list(entries[3:6])
    bad[1] = tiff_pages.PageImage(**{**bad[1].__dict__, "strips": [bad[1].strips[0], b"\x00" * 40] + list(bad[1].strips[2:])})
    out, status = s._decode_tiff_strips_in_place(s._engine, bad, w, height, 16, False)
    assert status == [0, -1, 0]
    assert np.array_equal(out[0].cpu().numpy(), tc.pillow_rgb(data, 3)) and np.array_equal(out[2].cpu().numpy(), tc.pillow_rgb(data, 5))


def test_pass_code_at_the_line_end_goes_to_pillow(service):
    """rand_65x40 with bit 5309 flipped: its last line ends with a pass code whose b2 is the line's end.  T.6 does not allow the
    code there, libtiff reads the line's last two pixels as white, and a decoder that takes the code paints them black.  The device
    refuses the strip (-1), so the page is Pillow's with the option on as with it off; the intact stream is still the device's."""
    s = service
    stream, w, h, _ = cc.fixtures()["rand_65x40"]
    file = lambda strip: tc.tiff_file([dict(strips=[strip], tags=tc.base_tags(w, h, tc.G4, 0, 1, 1, h))])
    def on_and_off(data):
        s.device_tiff = False
        off = s.process_image_sync(data)
        s.device_tiff = True
        seen = []
        inner = s._decode_tiff_pages

        def spy(entries, reasons):
            res = inner(entries, reasons)
            seen.append((sorted(res), dict(reasons)))
            return res
        s._decode_tiff_pages = spy
        try:
            on = s.process_image_sync(data)
        finally:
            del s._decode_tiff_pages
        assert off.success and (off.image_width, off.image_height) == (w, h), off.error
        return on, off, seen

    on, off, seen = on_and_off(file(stream))
    assert seen == [([0], {})] and _same(on, off)
    on, off, seen = on_and_off(file(cc.flip_bit(stream, 5309)))
    assert seen == [([], {0: "group4 strips corrupt (status -1)"})] and _same(on, off)


def _three(pages, second):
    h2, w2 = pages[2].shape[:2]
    return [_frames(pages)["lzw"](), second, tc.frame(_grey(pages[1]), W, tc.PACKBITS, rps=64)], (h2, w2)


@needs_libtiff
def test_three_frames_of_mixed_sizes_and_codecs(service, pages, tmp_path):
    s = service
    frames, _ = _three(pages, tc.g4_frame(_black(pages[2]), 0, 1, rps=48))
    path = tmp_path / "fax.tif"
    path.write_bytes(tc.tiff_file(frames))
    s.device_tiff = True
    doc = s.process_tiff_sync(path)
    assert doc.success and doc.total_pages == 3 and [p.page_number for p in doc.pages] == [1, 2, 3], doc.error
    assert [(p.image_width, p.image_height) for p in doc.pages] == [(W, H), (600, 800), (W, H)]
    via_document = asyncio.run(s.process_document(path, "tif"))
    assert via_document.total_pages == 3 and all(_same(a, b) for a, b in zip(via_document.pages, doc.pages))
    s.device_tiff = False
    for k in range(3):
        im = Image.open(path)
        im.seek(k)
        want = s.process_image_sync(im, page_number=k + 1)
        assert want.success and want.layout_boxes
        assert _same(doc.pages[k], want), k
    # with the option off: one page from "tiff", and "tif" is no supported type
    one = asyncio.run(s.process_document(path, "tiff"))
    assert one.total_pages == 1 and _same(one.pages[0], doc.pages[0])
    assert asyncio.run(s.process_document(path, "tif")).error == "Unsupported file type: tif"
    assert s.get_status()["device_tiff"] is False


def test_tiled_frame_is_pillows_the_others_the_devices(service, pages, tmp_path):
    s = service
    tiled, _ = tc.tiled_frame(800, 608)
    frames, _ = _three(pages, tiled)
    path = tmp_path / "tiled.tiff"
    path.write_bytes(tc.tiff_file_with_tiles(frames))
    s.device_tiff = True
    seen = []
    inner = s._decode_tiff_pages

    def spy(entries, reasons):       # (the caller adds Pillow's pages to the returned dict afterwards: note its keys now)
        res = inner(entries, reasons)
        seen.append((sorted(res), dict(reasons)))
        return res
    s._decode_tiff_pages = spy
    try:
        doc = s.process_tiff_sync(path)
    finally:
        del s._decode_tiff_pages
    assert seen[0] == ([0, 2], {1: "tiled layout"})
    assert doc.total_pages == 3 and all(p.success for p in doc.pages), [p.error for p in doc.pages]
    s.device_tiff = False
    for k in range(3):
        im = Image.open(path)
        im.seek(k)
        assert _same(doc.pages[k], s.process_image_sync(im, page_number=k + 1)), k


def test_undecodable_frame_is_that_pages_error(service, pages, tmp_path):
    s = service
    bad = tc.frame(_grey(pages[2]), 600, tc.NONE, extra={259: 34712})       # JPEG 2000 in TIFF: nobody here decodes it
    frames, _ = _three(pages, bad)
    path = tmp_path / "bad.tiff"
    path.write_bytes(tc.tiff_file(frames))
    s.device_tiff = True
    doc = s.process_tiff_sync(path)
    assert not doc.success and doc.error == "Some pages failed" and doc.total_pages == 3
    assert [p.success for p in doc.pages] == [True, False, True] and [p.page_number for p in doc.pages] == [1, 2, 3]
    err = doc.pages[1].error
    assert "Compression 34712" in err and "Pillow could not decode it: " in err and not err.endswith(": ")
    assert doc.pages[0].layout_boxes and doc.pages[2].layout_boxes
