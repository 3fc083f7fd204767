"""GPU: page orientation through the provider (LUMINA_OCR_PAGE_ORIENTATION=1): a page gives the same boxes, Markdown and processed bytes
whichever of the four ways it lies; sizes and page_rotation; tables and marks on turned pages; a document of mixed orientations; files
decoded on the device; the option off."""
import io

import numpy as np
import pytest
from PIL import Image

from lumina_ocr import arch, synth
from lumina_ocr.utils import layout

import cls_reference as cr
import page_orient_reference as pr

pytestmark = pytest.mark.gpu

H, W = 640, 896


@pytest.fixture(scope="module")
def page():
    return synth.synth_page(H, W, 3, n_lines=10, ruled=True)[0]


@pytest.fixture
def service():
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    saved = (s._allow_synthetic, s._use_page_orient, s._use_tables, s._use_marks, s._use_angle_cls, s.apply_deskew, s.device_png)
    s._allow_synthetic = True
    yield s
    s.cleanup()
    s._allow_synthetic, s._use_page_orient, s._use_tables, s._use_marks, s._use_angle_cls, s.apply_deskew, s.device_png = saved


def _configure(s, orient=True, tables=False, marks=False, deskew=None):
    s.cleanup()
    s._use_page_orient, s._use_tables, s._use_marks = orient, tables, marks
    if deskew is not None:
        s.apply_deskew = deskew


def _lying(page, k):
    return Image.fromarray(np.ascontiguousarray(np.rot90(page, k)))


def _check_rotation(r, page, k, first):
    """result r of np.rot90(page, k) against the result of the upright page"""
    h, w = page.shape[:2]
    assert r.success, r.error
    assert (r.image_width, r.image_height) == ((h, w) if k & 1 else (w, h))                  # the size as stored
    assert (r.page_width_inches, r.page_height_inches) == (float(w), float(h))                # the upright processed page
    assert r.json_output["page_rotation"] == (90 * ((4 - k) % 4)) % 360
    assert Image.open(io.BytesIO(r.processed_image_bytes)).size == (w, h)
    assert r.layout_boxes == first.layout_boxes and r.markdown == first.markdown and r.html == first.html
    assert r.processed_image_bytes == first.processed_image_bytes
    assert {k_: v for k_, v in r.json_output.items() if k_ != "page_rotation"} == {k_: v for k_, v in first.json_output.items() if k_ != "page_rotation"}
    assert layout.validate_layout_boxes(r.layout_boxes) == []


def test_the_four_rotations_of_a_ruled_page_through_the_provider(service, page):
    _configure(service)
    results = [service.process_image_sync(_lying(page, k)) for k in range(4)]
    for k, r in enumerate(results):
        _check_rotation(r, page, k, results[0])
    assert len([b for b in results[0].layout_boxes if b["type"] == "line"]) >= 8
    # to_dict() keys are the ones without the option; the upright page reads as it does without it
    _configure(service, orient=False)
    off = service.process_image_sync(_lying(page, 0))
    assert off.success and "page_rotation" not in off.json_output and sorted(off.to_dict()) == sorted(results[0].to_dict())
    assert off.layout_boxes == results[0].layout_boxes and off.markdown == results[0].markdown
    assert off.processed_image_bytes == results[0].processed_image_bytes
    assert {k: v for k, v in results[0].json_output.items() if k != "page_rotation"} == off.json_output


@pytest.mark.parametrize("kind", ["table", "marks"])
def test_tables_and_marks_on_a_page_lying_on_its_side(service, kind):
    """k = 0 and k = 3 only: one quarter turn, then an upright vote.  The restatement's own vote on these two pages turned by 180 degrees
    is NOT 180 with the provider's seeded networks (the table page: 1 line, under min_lines; the marks page: 5 of 17 lines flipped), so
    k = 1 and k = 2 are left out, as the hand-set orientation path is built for ruled lines; the vote is re-stated below."""
    if kind == "table":
        page = synth.synth_table_page(1, H, W, inset=14, spans=True, rows=4, cols=3, noise=2.0)[0]
    else:
        page = synth.synth_marks_page(1, H, W, n_marks=6, stroke=2, max_side=40)[0]
    charset = arch.ctc_charset()
    nets_ = arch.make_det_weights(), arch.make_rec_weights(num_classes=len(charset), code_path=True), arch.make_cls_weights(orientation_path=True)
    for k, want in ((0, False), (2, False)):      # upright: stays; turned by 180: the vote does not see it (see above)
        res, _ = cr.run_pages(*nets_, np.ascontiguousarray(np.rot90(page, k))[None], charset, post=arch.TEXT_PATH_POST)
        assert pr.vote(res[0]["flips"]) is want and not pr.sideways(np.rot90(page, k)) and pr.sideways(np.rot90(page, k + 1))
    _configure(service, tables=True, marks=True, deskew=False)
    up, side = service.process_image_sync(_lying(page, 0)), service.process_image_sync(_lying(page, 3))
    _check_rotation(up, page, 0, up)
    _check_rotation(side, page, 3, up)
    types = {b["type"] for b in up.layout_boxes}
    assert ("table" in types and up.json_output["tables_count"] == 1) if kind == "table" else ("selection_mark" in types and up.json_output["selection_marks_count"] >= 6)
    _configure(service, orient=False, tables=True, marks=True, deskew=False)
    off = service.process_image_sync(_lying(page, 0))
    assert off.layout_boxes == up.layout_boxes and off.markdown == up.markdown and off.processed_image_bytes == up.processed_image_bytes


def test_a_document_of_mixed_orientations(service, page):
    _configure(service)
    single = service.process_image_sync(_lying(page, 0))
    images = [_lying(page, k) for k in (0, 1, 2, 3, 1, 0)]          # two sizes: process_pages_sync groups them
    out = service.process_pages_sync(images, first_page_number=5)
    assert [r.page_number for r in out] == [5, 6, 7, 8, 9, 10]
    for r, k in zip(out, (0, 1, 2, 3, 1, 0)):
        assert r.success, r.error
        assert r.json_output["page_rotation"] == (90 * ((4 - k) % 4)) % 360
        assert (r.image_width, r.image_height) == ((H, W) if k & 1 else (W, H)) and (r.page_width_inches, r.page_height_inches) == (float(W), float(H))
        assert r.markdown == single.markdown and r.processed_image_bytes == single.processed_image_bytes
        renumber = lambda boxes: [dict(b, page_number=0) for b in boxes]
        assert renumber(r.layout_boxes) == renumber(single.layout_boxes)


def test_files_paths_bytes_and_device_decoders(service, page, tmp_path):
    _configure(service)
    lying = _lying(page, 1)
    want = service.process_image_sync(lying)
    assert want.success and want.json_output["page_rotation"] == 270
    png = tmp_path / "lying.png"
    lying.save(png)
    for device_png in (False, True):
        service.device_png = device_png
        for source in (png, str(png), png.read_bytes()):
            r = service.process_image_sync(source)
            assert r.success and r.json_output["page_rotation"] == 270 and (r.image_width, r.image_height) == (H, W)
            assert r.layout_boxes == want.layout_boxes and r.processed_image_bytes == want.processed_image_bytes
    jpg = tmp_path / "lying.jpg"
    lying.save(jpg, quality=95)
    host = service.process_image_sync(Image.open(jpg))                 # Pillow's decode of the same file
    for source in (jpg, jpg.read_bytes()):                             # baseline JPEG: decoded on the device
        r = service.process_image_sync(source)
        assert r.success and r.json_output["page_rotation"] == 270 and (r.page_width_inches, r.page_height_inches) == (float(W), float(H))
        assert r.layout_boxes == host.layout_boxes and r.processed_image_bytes == host.processed_image_bytes
    assert len([b for b in host.layout_boxes if b["type"] == "line"]) >= 8


def test_the_option_off_is_the_provider_without_it(service, page, monkeypatch):
    """With the variable unset a sideways page is read as it lies: the result is that of the pipeline without the option, json_output has
    no new key, and LUMINA_OCR_PAGE_ORIENTATION=0 is the same provider."""
    import torch
    from lumina_ocr.services import ocr_service as svc
    lying = np.ascontiguousarray(np.rot90(page, 1))
    results = []
    for env in (None, "0"):
        if env is None:
            monkeypatch.delenv("LUMINA_OCR_PAGE_ORIENTATION", raising=False)
        else:
            monkeypatch.setenv("LUMINA_OCR_PAGE_ORIENTATION", env)
        s = object.__new__(svc.OCRService)
        s._initialized = False
        svc.OCRService.__init__(s)
        s._allow_synthetic = True
        r = s.process_image_sync(Image.fromarray(lying))
        assert r.success and s._use_page_orient is False and s._pipeline.page_orient is False and not s._engine.cls_loaded
        dets, processed = s._pipeline.run(torch.from_numpy(lying[None]).cuda(), deskew=s.apply_deskew)
        assert sorted(b["content"] for b in r.layout_boxes if b["type"] == "line") == sorted(dets[0].texts)
        assert (r.page_width_inches, r.page_height_inches) == (float(H), float(W)) == (float(processed.shape[2]), float(processed.shape[1]))
        assert sorted(r.json_output) == ["lines_count", "page_count", "paragraphs_count", "tables_count", "words_count"]
        assert dets[0].turn is None
        s.cleanup()
        d = r.to_dict()
        d.pop("processing_time_ms")
        results.append((d, r.processed_image_bytes))
    assert results[0] == results[1]
