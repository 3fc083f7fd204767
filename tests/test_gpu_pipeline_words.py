"""GPU: OcrPipeline(word_boxes=True) — everything the option off gives is unchanged bit for bit, and the words equal the restatement
(tests/word_reference.py) applied to the stage outputs (rec_crop -> rec_forward) of the same lines; with angle_cls, under run_oriented,
on a page with a vertical line."""
import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw

from lumina_ocr import arch, synth
from lumina_ocr.pipeline import OcrPipeline

import word_reference as wr

pytestmark = pytest.mark.gpu

H, W = 640, 896


@pytest.fixture(scope="module")
def cls_weights():
    return arch.make_cls_weights(2718, orientation_path=True)


def _pipe(engine, det_weights, code_rec_weights, cls_weights=None, **kw):
    engine.load_det(det_weights)
    engine.load_rec(code_rec_weights)
    if cls_weights is not None:
        engine.load_cls(cls_weights)
    return OcrPipeline(engine, max_dimension=2000, post=arch.TEXT_PATH_POST, **kw)


def _dev(pages):
    return torch.from_numpy(np.ascontiguousarray(pages)).cuda()


def vertical_page():
    """three lines lying, one standing: a strip of text turned clockwise, so that it reads from the top of the page to the bottom"""
    img = Image.new("RGB", (W, H), (255, 255, 255))
    d = ImageDraw.Draw(img)
    font = synth._font(32)
    for k, txt in enumerate(("Invoice No 4471 of March", "total amount due 1 250", "paid by bank transfer")):
        d.text((220, 80 + 70 * k), txt, fill=(10, 10, 10), font=font)
    txt = "Reference AB 77 K9 standing"
    strip = Image.new("RGB", (int(d.textlength(txt, font=font)) + 8, 44), (255, 255, 255))
    ImageDraw.Draw(strip).text((4, 2), txt, fill=(10, 10, 10), font=font)
    img.paste(strip.rotate(-90, expand=True), (60, 40))
    return np.asarray(img, np.uint8).copy()


def _same_but_words(a, b):
    """two PageDetections, field by field, bitwise, the word fields aside"""
    assert a.texts == b.texts and (a.width, a.height) == (b.width, b.height) and a.turn == b.turn
    for f in ("quads", "scores", "det_scores", "text_ids", "lens", "cls_labels", "cls_scores"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None), f
        assert x is None or (x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()), f


def _dist_to_hull(pt, quad):
    """distance of a point from the convex quad (0 inside)"""
    p = np.asarray(quad, np.float64).reshape(4, 2)
    x = np.asarray(pt, np.float64)
    cross = [(p[(k + 1) % 4][0] - p[k][0]) * (x[1] - p[k][1]) - (p[(k + 1) % 4][1] - p[k][1]) * (x[0] - p[k][0]) for k in range(4)]
    if all(c >= 0 for c in cross) or all(c <= 0 for c in cross):
        return 0.0
    best = np.inf
    for k in range(4):
        a, b = p[k], p[(k + 1) % 4]
        ab = b - a
        t = 0.0 if not ab.any() else float(np.clip(np.dot(x - a, ab) / np.dot(ab, ab), 0.0, 1.0))
        best = min(best, float(np.linalg.norm(x - (a + t * ab))))
    return best


def _check_geometry(d, flips):
    """word count = len(text.split()); every word point within 1 px of its line's hull; consecutive words of a line do not overlap along
    the reading edges (the crop's top edge P0 -> P1 and bottom edge P3 -> P2, walked backwards when the crop was turned)"""
    for i, text in enumerate(d.texts):
        n = int(d.word_counts[i])
        assert n == len(text.split()) == len([w for w in text.split(" ") if w]), (i, text)
        assert [text[a:a + c] for a, c in d.word_spans[i, :n]] == text.split()
        P, rot = wr.crop_corners(d.quads[i])
        P = np.asarray(P, np.int64)
        words = [d.word_quads[i, k].reshape(4, 2).astype(np.int64) for k in range(n)]
        for wq in words:
            assert max(_dist_to_hull(pt, d.quads[i]) for pt in wq) <= 1.0, (i, wq.tolist(), d.quads[i].tolist())
        crop_order = [np.stack([wq[(k + rot) % 4] for k in range(4)]) for wq in words]   # the word's points by crop corner
        if flips is not None and flips[i]:
            crop_order = crop_order[::-1]
        for (a, b), (lo, hi) in (((0, 1), (0, 1)), ((3, 2), (3, 2))):
            u = P[b] - P[a]
            for prev, nxt in zip(crop_order, crop_order[1:]):
                assert np.dot(u, prev[hi] - P[a]) <= np.dot(u, nxt[lo] - P[a]), (i, text)
            for wq in crop_order:
                assert np.dot(u, wq[lo] - P[a]) <= np.dot(u, wq[hi] - P[a])


def _check_against_stages(engine, pipe, dets, processed):
    """dets: the detections of the pages of `processed` [m,H,W,3] (device) in order: their words equal the restatement applied to what
    rec_crop -> rec_forward give for the same lines in the same batch"""
    counts = [len(d.texts) for d in dets]
    if sum(counts) == 0:
        return 0
    quads = np.concatenate([d.quads for d in dets]).astype(np.int32)
    page_idx = np.repeat(np.arange(len(dets), dtype=np.int32), counts)
    flips = None
    if dets[0].cls_labels is not None:
        labels, scores = np.concatenate([d.cls_labels for d in dets]), np.concatenate([d.cls_scores for d in dets])
        flips = ((labels == 1) & (scores > np.float32(pipe.cls_thresh))).astype(np.int32)
    crops, widths = engine.rec_crop(processed, _dev(quads), _dev(page_idx), flip=None if flips is None else _dev(flips))
    idx, prob = engine.rec_forward(crops, widths)
    ref = wr.decode_words(idx.cpu().numpy(), prob.cpu().numpy(), quads, widths.cpu().numpy(), flips, pipe.space_id)
    off = 0
    for d, c in zip(dets, counts):
        sl = slice(off, off + c)
        assert np.array_equal(d.text_ids, ref["text"][sl]) and np.array_equal(d.lens, ref["len"][sl])
        assert d.scores.tobytes() == ref["score"][sl].tobytes()
        assert d.word_counts.dtype == np.int32 and np.array_equal(d.word_counts, ref["word_counts"][sl])
        assert np.array_equal(d.word_quads, ref["word_quads"][sl]) and np.array_equal(d.word_spans, ref["word_spans"][sl])
        assert d.word_scores.tobytes() == ref["word_scores"][sl].tobytes()
        _check_geometry(d, None if flips is None else flips[sl])
        off += c
    if flips is not None and flips.any():   # the flags matter: without them the restatement puts a flagged line's words elsewhere
        plain = wr.decode_words(idx.cpu().numpy(), prob.cpu().numpy(), quads, widths.cpu().numpy(), None, pipe.space_id)
        moved = [i for i in np.nonzero(flips)[0] if not np.array_equal(plain["word_quads"][i], ref["word_quads"][i])]
        assert moved, int(flips.sum())   # (a word centred in its line stays where it is)
        assert np.array_equal(plain["word_spans"], ref["word_spans"]) and plain["word_scores"].tobytes() == ref["word_scores"].tobytes()
    return int(ref["word_counts"].sum())


@pytest.fixture(scope="module")
def pages():
    return np.stack([synth.synth_page(H, W, 21, n_lines=9)[0], synth.synth_page(H, W, 22, n_lines=8)[0], vertical_page(),
                     np.full((H, W, 3), 255, np.uint8)])


@pytest.fixture(scope="module")
def form_page():
    return synth.synth_form_page(3)[0]   # 2000 x 1090, the size of the reference's captured sample


def test_words_on_the_form_page(engine, det_weights, code_rec_weights, form_page):
    on_pipe = _pipe(engine, det_weights, code_rec_weights, word_boxes=True)
    on, processed = on_pipe.run(_dev(form_page[None]))
    off, _ = _pipe(engine, det_weights, code_rec_weights).run(_dev(form_page[None]))
    _same_but_words(on[0], off[0])
    assert len(on[0].texts) >= 12 and off[0].word_counts is None
    assert _check_against_stages(engine, on_pipe, on, processed) >= 20


def test_words_on_equals_off_plus_the_restated_words(engine, det_weights, code_rec_weights, pages):
    on_pipe = _pipe(engine, det_weights, code_rec_weights, word_boxes=True)
    assert on_pipe.space_id == len(on_pipe.charset) - 1
    on, processed = on_pipe.run(_dev(pages))
    off, poff = _pipe(engine, det_weights, code_rec_weights).run(_dev(pages))
    assert torch.equal(processed, poff)
    for a, b in zip(on, off):
        _same_but_words(a, b)
        assert b.word_quads is None and b.word_spans is None and b.word_scores is None and b.word_counts is None and b.line_words() is None
        assert a.word_quads.shape == (len(a.texts), 40, 8) and a.word_spans.shape == (len(a.texts), 40, 2)
        assert a.word_scores.shape == (len(a.texts), 40) and a.word_counts.shape == (len(a.texts),)
    assert len(on[0].texts) >= 7 and len(on[1].texts) >= 6 and len(on[3].texts) == 0
    n_words = _check_against_stages(engine, on_pipe, on, processed)
    assert n_words > sum(len(d.texts) for d in on)                      # lines of several words
    # the page with the standing line: a line that takes the crop's rotation branch, with words running down the page
    standing = [i for i, q in enumerate(on[2].quads) if wr.crop_corners(q)[1] == 1 and on[2].word_counts[i] >= 1]
    assert standing, on[2].quads.tolist()
    for i in standing:
        q = on[2].word_quads[i, :on[2].word_counts[i]].reshape(-1, 4, 2)
        assert (np.diff(q[:, 0, 1]) >= 0).all() and (q[:, 3, 1] >= q[:, 0, 1]).all()   # TL of word k+1 below TL of word k; BL below TL
    # line_words: what the layout takes
    lw = on[0].line_words()
    assert [len(x) for x in lw] == on[0].word_counts.tolist()
    assert all(on[0].texts[i][a:a + c] == w for i, x in enumerate(lw) for (a, c, _, _), w in zip(x, on[0].texts[i].split()))


def test_words_with_the_line_classifier(engine, det_weights, code_rec_weights, cls_weights):
    # the hand-set orientation path reads the rule under a line: ruled pages, one upright and two whose lines are read turned
    ruled = [synth.synth_page(H, W, sd, n_lines=9, ruled=True)[0] for sd in (3, 9)]
    both = np.stack([ruled[0], np.rot90(ruled[0], 2), np.rot90(ruled[1], 2)])
    on_pipe = _pipe(engine, det_weights, code_rec_weights, cls_weights, word_boxes=True, angle_cls=True)
    on, processed = on_pipe.run(_dev(both))
    off, _ = _pipe(engine, det_weights, code_rec_weights, cls_weights, angle_cls=True).run(_dev(both))
    for a, b in zip(on, off):
        _same_but_words(a, b)
    assert (on[0].cls_labels == 0).all() and (on[1].cls_labels == 1).sum() >= 5 and (on[2].cls_labels == 1).sum() >= 5
    # (a ruled line reads as one word: the rule fills the gaps between its words)
    assert _check_against_stages(engine, on_pipe, on, processed) >= 20
    flagged = (on[1].cls_labels == 1) & (on[1].cls_scores > np.float32(on_pipe.cls_thresh))
    assert flagged.sum() >= 5 and (on[1].word_counts[flagged] >= 1).all()


@pytest.mark.parametrize("angle_cls", [False, True])
def test_words_under_run_oriented(engine, det_weights, code_rec_weights, cls_weights, angle_cls):
    page = synth.synth_page(H, W, 3, n_lines=10, ruled=True)[0]
    other = synth.synth_page(H, W, 9, n_lines=8, ruled=True)[0]
    batch = np.stack([page, np.rot90(other, 2), np.rot90(page, 2), other])
    kw = dict(page_orient=True, angle_cls=angle_cls)
    on_pipe = _pipe(engine, det_weights, code_rec_weights, cls_weights, word_boxes=True, **kw)
    on, processed = on_pipe.run_oriented(_dev(batch))
    off, poff = _pipe(engine, det_weights, code_rec_weights, cls_weights, **kw).run_oriented(_dev(batch))
    assert [d.turn for d in on] == [0, 2, 2, 0]
    for a, b, pa, pb in zip(on, off, processed, poff):
        _same_but_words(a, b)
        assert torch.equal(pa, pb) and len(a.texts) >= 6 and b.word_counts is None
    total = 0
    for idxs, dets, proc in on_pipe.run_oriented_groups(_dev(batch)):
        total += _check_against_stages(engine, on_pipe, dets, proc)
        for k, d in zip(idxs, dets):
            assert np.array_equal(d.word_quads, on[k].word_quads) and d.word_scores.tobytes() == on[k].word_scores.tobytes()
    assert total == sum(int(d.word_counts.sum()) for d in on) > 20
    # a page turned by 180 degrees gives the words of the upright page
    assert np.array_equal(on[0].word_quads, on[2].word_quads) and np.array_equal(on[3].word_spans, on[1].word_spans)


def test_words_are_not_computed_with_a_gather(engine, det_weights, code_rec_weights):
    class Gather:   # the smallest stand-in: what _submit_lines and finish call
        def begin(self, counts):
            pass

        def submit(self, counts, quads, det_sc, text, length, score):
            return (counts, text.cpu().numpy())

        def finish(self, handle):
            return handle

    pipe = _pipe(engine, det_weights, code_rec_weights, word_boxes=True, gather=Gather())
    (counts, text), _ = pipe.run(_dev(synth.synth_page(H, W, 21, n_lines=9)[0][None]))
    assert counts.sum() == len(text) >= 7
