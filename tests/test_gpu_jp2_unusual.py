"""GPU: the device JPEG 2000 decoder (csrc/jp2dec.hip) on valid files that OpenJPEG's encoder never writes (tests/jp2_unusual_cases.py):
rewritten Pillow files (guard bits, tile-parts, extra segments and boxes, empty layers) and synthesised ones (blocks of 13 to 15
bit-planes, the pass-count escape, late inclusion, free byte splits, cut codewords), byte for byte against Pillow; one mixed call per
size with refused files and a sentinel; a sub-batched run; and a scanned PDF whose JPX page is a rewritten file through the provider.
Every file here is valid and has gone through the sanitized host programs first (tests/test_jp2_parser_sanitized.py,
tests/test_jp2_irreversible_sanitized.py); none is built to provoke a fault."""
import numpy as np
import pytest
import torch

import jp2_cases as jc
import jp2_unusual_cases as uc
import jp2_writer as jw
import pdf_cases as pc
from lumina_ocr import synth
from lumina_ocr.engine import Engine

pytestmark = pytest.mark.gpu


def _by_size(cases):
    groups = {}
    for c in cases:
        _, info = Engine.jp2_probe_irreversible(c.data)
        groups.setdefault((info["height"], info["width"]), []).append(c)
    return groups


def _differs(got, want):
    d = np.argwhere(got != want)
    return "%d of %d values differ, first at %s: got %s want %s" % (len(d), got.size, d[0].tolist(), got[tuple(d[0])], want[tuple(d[0])])


def test_every_accepted_case_equals_pillow(engine):
    """one call per size and entry point: 5/3 cases through both entries, 9/7 cases through the irreversible one"""
    groups = _by_size(uc.accepted())
    assert set(groups) == {(31, 33), (40, 64), (63, 65), (65, 63), (100, 130)}
    for (h, w), group in groups.items():
        files = [c.data for c in group]
        out, status = engine.jp2_decode_irreversible(files, h, w)
        assert status == [0] * len(group), (h, w, [(c.name, s) for c, s in zip(group, status) if s])
        got = out.cpu().numpy()
        for k, c in enumerate(group):
            want = jc.expected(c.data)
            assert np.array_equal(got[k], want), (c.name, _differs(got[k], want))
        plain = [k for k, c in enumerate(group) if not c.irreversible]
        out2, status2 = engine.jp2_decode([files[k] for k in plain], h, w)
        assert status2 == [0] * len(plain), (h, w, status2)
        assert np.array_equal(out2.cpu().numpy(), got[plain]), (h, w)


def test_mixed_call_per_size(engine):
    """rewritten, synthesised and plain Pillow files of differing level counts in one batch with the refused variants of that size:
    the accepted slots are Pillow's, the refused ones are -2 and keep the fill"""
    groups = _by_size(uc.accepted())
    refused = _by_size(uc.refused())
    assert set(refused) <= set(groups) and len(refused) >= 2
    for (h, w), group in groups.items():
        plain = [jc.write(jc.content("page" if k % 2 else "noise", h, w, "RGB" if k % 2 else "L", seed=3000 + k), irreversible=bool(k == 2),
                          num_resolutions=1 + k) for k in range(4)]
        entries = [(c.data, 0) for c in group] + [(c.data, -2) for c in refused.get((h, w), [])] + [(d, 0) for d in plain]
        order = np.random.default_rng(h * w).permutation(len(entries))
        entries = [entries[i] for i in order]
        files = [d for d, _ in entries]
        out = torch.full((len(files), h, w, 3), 77, dtype=torch.uint8, device="cuda")
        out, status = engine.jp2_decode_irreversible(files, h, w, out=out)
        assert status == [st for _, st in entries], (h, w, status)
        got = out.cpu().numpy()
        for k, (data, st) in enumerate(entries):
            if st == 0:
                want = jc.expected(data)
                assert np.array_equal(got[k], want), (h, w, k, _differs(got[k], want))
            else:
                assert (got[k] == 77).all(), (h, w, k)


def test_sub_batches(engine):
    """jp2_sub_batch_mb = 1: a 64 x 40 grey page takes 20 KB of coefficient planes and an RGB one 60 KB, so 130 files split into
    several sub-batches; the 15-plane file comes up in each of them, among Pillow files, and the result is the single batch's"""
    h, w = 40, 64
    deep = {c.name: c.data for c in uc.synthesised()}["a_deep_64x40_cb64x32"]
    plain = [jc.write(jc.content("page" if k % 2 else "noise", h, w, "RGB" if k % 3 else "L", seed=3100 + k), irreversible=False, num_resolutions=1 + k % 4)
             for k in range(7)]
    files = [deep if k % 3 == 0 else plain[k % 7] for k in range(130)]
    whole, status = engine.jp2_decode(files, h, w)
    assert status == [0] * len(files)
    engine.set_option("jp2_sub_batch_mb", 1)
    try:
        out = torch.full((len(files), h, w, 3), 77, dtype=torch.uint8, device="cuda")
        out, status = engine.jp2_decode(files, h, w, out=out)
    finally:
        engine.set_option("jp2_sub_batch_mb", 4096)
    assert status == [0] * len(files)
    assert torch.equal(out, whole)
    got = out.cpu().numpy()
    for k in range(8):
        assert np.array_equal(got[k], jc.expected(files[k])), k


def test_rewritten_jpx_page_through_the_provider(monkeypatch, tmp_path):
    """a scanned PDF whose /JPXDecode page is a Pillow file rewritten to three tile-parts, one guard bit, a TLM and the 64-bit box
    length: OCRService decodes it on the device (one jp2_decode call, status 0) and gives what Pillow's pixels give"""
    from PIL import Image
    from lumina_ocr.services import ocr_service as svc
    h, w = 300, 420
    page = synth.synth_page(h, w, 35, n_lines=6)[0]
    base = jc.write(page, irreversible=False)
    data = jw.rewrite(base, **uc.PROVIDER_EDITS)
    assert data != base and np.array_equal(jc.expected(data), page)
    seen = []
    decode = Engine.jp2_decode

    def recording_decode(self, files, *a, **kw):
        out, status = decode(self, files, *a, **kw)
        seen.append(([bytes(f) for f in files], list(status), out.clone()))
        return out, status
    monkeypatch.setattr(Engine, "jp2_decode", recording_decode)
    s = svc.OCRService()
    s.cleanup()
    s._allow_synthetic = True
    saved = s.device_jp2, s.device_pdf, s.jp2_irreversible
    try:
        def pdf_to_images(path, dpi=None, first_page=None, last_page=None):
            raise ImportError("pdf2image not installed")
        monkeypatch.setattr(s._pre, "pdf_to_images", pdf_to_images)
        image = pc.stream_obj("/Type /XObject /Subtype /Image /Width %d /Height %d /ColorSpace /DeviceRGB /BitsPerComponent 8 /Filter /JPXDecode" % (w, h), data)
        pdf = tmp_path / "scan.pdf"
        pdf.write_bytes(pc.document([{"image": image, "box": (504, 360)}]))
        s.device_pdf = s.device_jp2 = True
        s.jp2_irreversible = False
        doc = s.process_pdf_sync(pdf)
        assert doc.success and doc.total_pages == 1, [p.error for p in doc.pages]
        assert len(seen) == 1 and seen[0][0] == [data] and seen[0][1] == [0]
        assert np.array_equal(seen[0][2][0].cpu().numpy(), page)
        want = s.process_pages_sync([Image.fromarray(page)])
        key = lambda r: (r.success, r.error, r.markdown, r.layout_boxes, r.image_width, r.image_height)
        assert want[0].success and want[0].layout_boxes and key(doc.pages[0]) == key(want[0])
    finally:
        s.device_jp2, s.device_pdf, s.jp2_irreversible = saved
        s.cleanup()
