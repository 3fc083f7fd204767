"""CPU: the orientation classifier's block table and weight container, and the crop restatement of tests/cls_reference.py
(held to the oracle's C restatement of the recognition crop bit for bit, turned and unturned)."""
import numpy as np

from lumina_ocr import arch, synth

import cls_reference as cr

QUADS = [
    [0, 0, 320, 0, 320, 32, 0, 32],          # 1:1 sampling at the recogniser's size
    [10, 0, 42, 0, 42, 64, 10, 64],          # tall box: turned by 90 degrees first (h / w = 2 >= 1.5)
    [5, 5, 5, 5, 5, 5, 5, 5],                # degenerate: width 0, all zero
    [17, 20, 400, 31, 398, 60, 15, 49],      # skewed, wider than both caps
    [300, 10, 330, 12, 328, 110, 298, 108],  # tall and skewed
    [40, 40, 90, 40, 90, 60, 40, 60],        # ratio 2.5
    [-8, 90, 60, 90, 60, 130, -8, 130],      # corners off the page: samples clamp to the border
]


def test_cls_block_table():
    t = arch.cls_block_table()
    assert [(b["exp"], b["cout"]) for b in t] == [(8, 8), (24, 8), (32, 8), (32, 16), (88, 16), (88, 16), (40, 16), (48, 16),
                                                  (104, 32), (200, 32), (200, 32)]
    assert [b["stride_h"] for b in t] == [2, 2, 1, 2, 1, 1, 1, 1, 2, 1, 1]
    assert [b["h"] for b in t] == [12, 6, 6, 3, 3, 3, 3, 3, 2, 2, 2]
    assert all(b["se_mid"] == b["exp"] // 4 for b in t) and arch.rec_stem_ch(arch.CLS_SCALE) == 8
    assert [b["res"] for b in t] == [False, False, True, False, True, True, True, True, False, True, True]
    # the recogniser's table is what it was: its own strides, scale 0.5
    assert arch.rec_block_table() == arch.rec_block_table(0.5, [row[5] for row in arch._MV3_SMALL])
    assert [b["stride_h"] for b in arch.rec_block_table()] == [1, 2, 1, 2, 1, 1, 1, 1, 2, 1, 1]


def test_cls_blob_round_trip():
    w = arch.make_cls_weights(7)
    back = arch.read_blob(arch.write_blob(w))
    assert set(back) == set(w) and all(np.array_equal(back[k], w[k]) for k in w)
    assert w["cls.conv1.w"].shape == (8, 3, 3, 3) and w["cls.conv2.w"].shape == (200, 1, 1, 32) and w["cls.fc.w"].shape == (2, 200)
    assert w["cls.b9.se1.w"].shape == (50, 1, 1, 200) and w["cls.b8.dw.w"].shape == (104, 5, 5, 1)


def test_crop_restatement_equals_the_oracle_rec_crop():
    """At 32 x 320 the restatement IS the recognition crop: equal to oracle/csrc's, and its turned form equals the turned crop."""
    from oracle import dbpost
    rng = np.random.default_rng(3)
    page = rng.integers(0, 256, (120, 500, 3), dtype=np.uint8)
    for q in QUADS:
        ref, wref = dbpost.rec_crop(page, q)
        got, wgot = cr.crop(page, q, 32, 320)
        assert wgot == wref and np.array_equal(got, ref), q
        turned, wt = cr.crop(page, q, 32, 320, flip=True)
        assert wt == wref and np.array_equal(turned, cr.turn(ref, wref)), q


def test_cls_crop_width_and_padding():
    assert cr.crop_width([0, 0, 400, 0, 400, 20, 0, 20]) == 192      # ratio 20: the cap
    assert cr.crop_width([0, 0, 60, 0, 60, 30, 0, 30]) == 96         # ratio 2
    assert cr.crop_width([10, 0, 42, 0, 42, 64, 10, 64]) == 96       # vertical box, turned first: ratio 2
    assert cr.crop_width([0, 0, 7, 0, 7, 10, 0, 10]) == 34           # ratio 0.7 (not turned: 10 / 7 < 1.5): ceil(33.6)
    assert cr.crop_width([5, 5, 5, 5, 5, 5, 5, 5]) == 0
    page = np.full((120, 500, 3), 255, np.uint8)
    for q in QUADS:
        c, wc = cr.crop(page, q)
        assert c.shape == (48, 192, 3) and wc == cr.crop_width(q)
        assert c[:, wc:].max(initial=0) == 0 and (wc == 0 or c[:, :wc].min() == 255)


def test_cls_crop_at_48_rows_known_answer():
    """An axis-aligned 192 x 48 box: crop pixel (i, j) samples page point (30 + j + 0.5, 20 + i + 0.5), the mean of a 2 x 2 pixel block
    (exact in float32), rounded half to even — computed here in float64 without the restatement."""
    rng = np.random.default_rng(5)
    page = rng.integers(0, 256, (100, 300, 3), dtype=np.uint8)
    q = page[20:69, 30:223].astype(np.float64)
    want = np.rint((q[:-1, :-1] + q[:-1, 1:] + q[1:, :-1] + q[1:, 1:]) / 4).astype(np.uint8)
    c, wc = cr.crop(page, [30, 20, 222, 20, 222, 68, 30, 68])
    assert wc == 192 and np.array_equal(c, want)
    t, _ = cr.crop(page, [30, 20, 222, 20, 222, 68, 30, 68], flip=True)
    assert np.array_equal(t, want[::-1, ::-1])


def test_orientation_path_decides_ruled_pages():
    """Restatement only: on an upright, enhanced ruled page every detected line is label 0, on the page turned by 180 degrees label 1 and
    flipped, each with |logit1 - logit0| >= CLS_MARGIN."""
    from oracle import dbpost, nets, preprocess
    det_w, cls_w = arch.make_det_weights(1234), arch.make_cls_weights(2718, orientation_path=True)
    page = synth.synth_page(480, 640, 7, n_lines=7, ruled=True)[0]
    page = preprocess.enhance_sharpness(preprocess.enhance_contrast(page, 1.2), 1.1)   # the pipeline's enhance step
    for turned, pg in ((0, page), (1, np.ascontiguousarray(page[::-1, ::-1]))):
        quads, _, _ = dbpost.db_postprocess(arch.f32_to_bf16_bits(nets.det_forward(det_w, pg[None]))[0], 480, 640, **arch.TEXT_PATH_POST)
        crops, widths = zip(*[cr.crop(pg, q) for q in quads])
        label, score, flip, logits = cr.classify(cls_w, np.stack(crops), widths)
        assert len(quads) >= 6 and (label == turned).all() and (flip == turned).all() and (score > 0.99).all()
        assert (np.abs(logits[:, 1] - logits[:, 0]) >= arch.CLS_MARGIN).all()


def test_ruled_page_keeps_the_text_of_the_plain_page():
    a, ga = synth.synth_page(480, 640, 7, n_lines=7)
    b, gb = synth.synth_page(480, 640, 7, n_lines=7, ruled=True)
    assert [g["text"] for g in ga] == [g["text"] for g in gb] and not np.array_equal(a, b)


def test_orientation_path_keeps_dense_rows():
    dense, path = arch.make_cls_weights(2718), arch.make_cls_weights(2718, orientation_path=True)
    assert np.array_equal(dense["cls.b9.dw.w"][2:], path["cls.b9.dw.w"][2:]) and np.array_equal(dense["cls.conv1.w"][1:], path["cls.conv1.w"][1:])
    assert path["cls.fc.w"][0, 1] == arch.CLS_GAIN and path["cls.fc.w"][1, 0] == arch.CLS_GAIN


def test_per_layer_wrappers_chain_to_the_backbone():
    """cls_conv1 -> cls_block x 11 -> cls_conv2 -> cls_pool, each on the previous result, IS backbone(): every tap bit for bit."""
    import torch
    from oracle import nets
    w = arch.make_cls_weights(2718)
    crops, widths = cr.layer_crops(3)
    x = cr.normalize(crops, widths)
    taps = {}
    feat = cr.backbone(w, x, "bf16", taps)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().numpy()           # noqa: E731
    with torch.no_grad():
        y = cr.cls_conv1(w, x)
        assert np.array_equal(nhwc(y), taps["cls.conv1"]) and y.shape == (3, 8, 24, 96)
        for b in arch.cls_block_table():
            y = cr.cls_block(w, nets.nhwc_to_nchw(nhwc(y)), b)              # through the NHWC form the GPU test hands over
            assert np.array_equal(nhwc(y), taps["cls.b%d" % b["idx"]]), b["idx"]
            assert y.shape[1:3] == (b["cout"], b["h"])
        y = cr.cls_conv2(w, y)
        assert np.array_equal(nhwc(y), taps["cls.conv2"]) and y.shape == (3, arch.CLS_FEAT, 2, 96)
        y = cr.cls_pool(y)
        assert np.array_equal(nhwc(y), taps["cls.feat"]) and y.shape == (3, arch.CLS_FEAT, 1, 48)
    assert np.array_equal(y[:, :, 0, :].permute(0, 2, 1).numpy(), feat)


def test_layer_crops_and_width_mask():
    """The per-layer grading's inputs: a noise crop first, text crops after it, the widths cycling through every edge of the mask; the
    normalised input really is zero from each width on and is not before it."""
    crops, widths = cr.layer_crops(33)
    assert crops.shape == (33, 48, 192, 3) and crops.dtype == np.uint8
    assert set(widths.tolist()) == set(cr.LAYER_WIDTHS) and widths[0] == 191 and widths[1] == 192 and widths[2] == 1
    assert len(np.unique(crops[0])) == 256                                   # uniform noise
    for c in crops[1:]:
        assert c.min() < 100 and c.max() > 200 and c[:, :, 0].std() > 10     # ink and paper: a rendered line
    assert len({c.tobytes() for c in crops}) == 33
    a, wa = cr.layer_crops(7)
    assert np.array_equal(a, crops[:7]) and np.array_equal(wa, widths[:7])  # the smaller sets are prefixes
    x = cr.normalize(crops, widths).numpy()
    plain = cr.normalize(crops, np.full(33, 192)).numpy()
    for i, wv in enumerate(widths):
        assert not x[i, :, :, wv:].any() and np.array_equal(x[i, :, :, :wv], plain[i, :, :, :wv])
        assert wv == 192 or plain[i, :, :, wv:].any()                        # the mask removes real pixels
    assert x[2, :, :, 0].any() and not x[2, :, :, 1:].any()                  # width 1: one column survives


def _service(monkeypatch, **attrs):
    from lumina_ocr.services import ocr_service as svc
    s = svc.OCRService()
    s.cleanup()
    for k, v in attrs.items():
        monkeypatch.setattr(s, k, v)
    return s


def test_provider_angle_cls_settings(monkeypatch, tmp_path):
    """Off by default; on without LUMINA_OCR_CLS_WEIGHTS is an error result (checked before any GPU is touched) unless
    LUMINA_OCR_ALLOW_SYNTHETIC=1 allows the seeded classifier."""
    import asyncio
    from PIL import Image
    from lumina_ocr.services import ocr_service as svc
    monkeypatch.delenv("LUMINA_OCR_USE_ANGLE_CLS", raising=False)
    fresh = object.__new__(svc.OCRService)
    fresh._initialized = False
    svc.OCRService.__init__(fresh)
    assert fresh._use_angle_cls is False and fresh._cls_weights == ""
    monkeypatch.setenv("LUMINA_OCR_USE_ANGLE_CLS", "1")
    monkeypatch.setenv("LUMINA_OCR_CLS_WEIGHTS", "/x/cls.locw")
    fresh._initialized = False
    svc.OCRService.__init__(fresh)
    assert fresh._use_angle_cls is True and fresh._cls_weights == "/x/cls.locw"
    p = tmp_path / "page.png"
    Image.fromarray(np.full((48, 64, 3), 255, np.uint8)).save(p)
    s = _service(monkeypatch, _allow_synthetic=False, _use_angle_cls=True, _cls_weights="", _det_weights=str(p), _rec_weights=str(p),
                 _rec_dict=str(p))
    r = asyncio.run(s.process_document(str(p), "png"))
    assert not r.success and "LUMINA_OCR_CLS_WEIGHTS" in r.error and r.combined_markdown == ""
    s.cleanup()
