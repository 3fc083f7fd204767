"""GPU: the orientation classifier (lumina_ocr_load_cls_weights / lumina_ocr_cls_forward) against tests/cls_reference.py — every tap with
dense seeded weights, the head on the engine's own features bit for bit, exact labels on the hand-set orientation path, sub-batches,
and the bench-sized batch."""
import numpy as np
import pytest
import torch

from conftest import close_stats
from lumina_ocr import arch, synth
from oracle import dbpost, nets, preprocess

import cls_reference as cr

pytestmark = pytest.mark.gpu

TAPS = ["cls.conv1"] + ["cls.b%d" % i for i in range(11)] + ["cls.conv2", "cls.feat"]


def _ruled_crops(h=640, w=896, seed=3, n_lines=10, turned=False):
    """Classifier crops of the detector's boxes (text path) on an enhanced ruled synthetic page, upright or turned by 180 degrees."""
    page = synth.synth_page(h, w, seed, n_lines=n_lines, ruled=True)[0]
    if turned:
        page = np.ascontiguousarray(page[::-1, ::-1])
    page = preprocess.enhance_sharpness(preprocess.enhance_contrast(page, 1.2), 1.1)   # as the pipeline sees it
    prob = nets.det_forward(arch.make_det_weights(1234), page[None])
    quads, _, _ = dbpost.db_postprocess(arch.f32_to_bf16_bits(prob)[0], h, w, **arch.TEXT_PATH_POST)
    crops, widths = zip(*[cr.crop(page, q) for q in quads])
    return np.stack(crops), np.array(widths, np.int32)


def _mixed_crops():
    a, wa = _ruled_crops(480, 640, 7, 7)
    b, wb = _ruled_crops(480, 640, 7, 7, turned=True)
    return np.concatenate([a, b]), np.concatenate([wa, wb])


def _run(engine, crops, widths, thresh=arch.CLS_THRESH):
    label, score, flip = engine.cls_forward(torch.from_numpy(crops).cuda(), torch.from_numpy(widths).cuda(), thresh)
    torch.cuda.synchronize()
    return label.cpu().numpy(), score.cpu().numpy(), flip.cpu().numpy()


def test_cls_taps_with_dense_weights(engine):
    w = arch.make_cls_weights(2718)
    crops, widths = _mixed_crops()
    widths[::3] = np.resize(np.array([150, 77, 192, 31, 120], np.int32), len(widths[::3]))   # ragged valid widths: the stem zeroes the rest
    engine.load_cls(w)
    engine.set_option("keep_taps", 1)
    label, score, flip = _run(engine, crops, widths)
    got = {t: engine.read_tap(t) for t in TAPS + ["cls.logits"]}
    engine.set_option("keep_taps", 0)
    taps = {}
    cr.backbone(w, cr.normalize(crops, widths), "bf16", taps)
    for name in TAPS:
        g, r = got[name], taps[name]
        g = g[..., : r.shape[-1]]
        st = close_stats(g, r)
        assert st["within4"] > 0.90 and st["mean_abs"] < 0.01 * max(st["ref_mean_abs"], 1e-3), (name, st)
    # the head on the engine's own features: the same order, every bit
    rl, rs, rf, rlog = cr.head(w, got["cls.feat"][:, 0, :, :arch.CLS_FEAT])
    assert np.array_equal(label, rl) and np.array_equal(flip, rf)
    assert np.array_equal(got["cls.logits"].reshape(-1, 2), arch.bf16_round(rlog))
    assert np.abs(score - rs).max() <= 2e-7 and ((score > 0.5) & (score <= 1.0)).all()


def test_orientation_path_labels_are_exact(engine):
    """Hand-set path: upright lines label 0, turned lines label 1 and flipped, EQUAL to the restatement; the path channels T / B of
    cls.feat are bit-identical."""
    w = arch.make_cls_weights(2718, orientation_path=True)
    engine.load_cls(w)
    for turned in (False, True):
        crops, widths = _ruled_crops(turned=turned)
        engine.set_option("keep_taps", 1)
        label, score, flip = _run(engine, crops, widths)
        feat = engine.read_tap("cls.feat")
        engine.set_option("keep_taps", 0)
        taps = {}
        rl, rs, rf, rlog = cr.classify(w, crops, widths, taps=taps)
        assert np.array_equal(feat[..., :2], taps["cls.feat"][..., :2])
        assert np.array_equal(label, rl) and np.array_equal(flip, rf)
        assert (label == int(turned)).all() and (flip == int(turned)).all() and (score > 0.99).all(), (label, score)
        assert (np.abs(rlog[:, 1] - rlog[:, 0]) >= arch.CLS_MARGIN).all()


def test_sub_batches_equal_one_batch(engine):
    engine.load_cls(arch.make_cls_weights(2718))
    crops, widths = _mixed_crops()
    whole = _run(engine, crops, widths)
    engine.set_option("cls_sub_batch", 3)
    try:
        split = _run(engine, crops, widths)
    finally:
        engine.set_option("cls_sub_batch", 4096)
    for a, b in zip(whole, split):
        assert np.array_equal(a, b)


def test_bench_sized_batch(engine):
    """3279 crops (the bench's 64-page step) in one call: the workspace layout holds, and the first crops equal a small call's."""
    engine.load_cls(arch.make_cls_weights(2718))
    crops, widths = _mixed_crops()
    reps = -(-3279 // len(crops))
    big, bw = np.tile(crops, (reps, 1, 1, 1))[:3279], np.tile(widths, reps)[:3279]
    label, score, flip = _run(engine, big, bw)
    small = _run(engine, crops, widths)
    n = len(crops)
    assert np.array_equal(label[:n], small[0]) and np.array_equal(score[:n], small[1]) and np.array_equal(flip[:n], small[2])
    assert label[3278] == small[0][3278 % n] and score[3278] == small[1][3278 % n]
    assert set(np.unique(label).tolist()) <= {0, 1}
