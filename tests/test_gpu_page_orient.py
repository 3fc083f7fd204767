"""GPU: the page orientation's device half (lumina_ocr_page_quarter / _page_turn / _page_vote) against tests/page_orient_reference.py and
numpy, and OcrPipeline(page_orient=True).run_oriented on ruled synthetic pages with the hand-set text, code and orientation paths: the
result of a page does not depend on which of the four ways it lies."""
import numpy as np
import pytest
import torch

from lumina_ocr import arch, synth
from lumina_ocr.pipeline import OcrPipeline

import page_orient_reference as pr

pytestmark = pytest.mark.gpu

H, W = 640, 896


def _quarter(engine, pages: np.ndarray, **kw):
    e, s = engine.page_quarter(torch.from_numpy(np.ascontiguousarray(pages)).cuda(), **kw)
    torch.cuda.synchronize()
    assert e.dtype == torch.int64 and s.dtype == torch.int32
    return e.cpu().numpy(), s.cpu().numpy()


def _check_quarter(engine, pages: np.ndarray, **kw):
    e, s = _quarter(engine, pages, **kw)
    ref = [pr.energies(p, kw.get("threshold", pr.P["threshold"])) for p in pages]
    assert e.tolist() == [list(r) for r in ref]
    assert s.tolist() == [int(pr.sideways_from(*r, kw.get("ratio", pr.P["ratio"]))) for r in ref]
    return e, s


def test_quarter_equals_the_restatement_on_every_page_kind_and_rotation(engine):
    for kind, page in pr.page_kinds().items():
        for k in range(4):
            _, s = _check_quarter(engine, np.rot90(page, k)[None])
            assert s[0] == (k & 1), (kind, k)


@pytest.mark.parametrize("w", [63, 64, 65, 1414])
def test_quarter_widths_around_a_mask_word(engine, w):
    rng = np.random.default_rng(w)
    pages = rng.integers(0, 256, (3, 97, w, 3), dtype=np.uint8)
    pages[1, :, : w // 2] = 255        # half blank
    pages[2] = np.where(rng.random((97, w, 1)) < 0.1, 0, 255)
    _check_quarter(engine, pages)
    _check_quarter(engine, np.ascontiguousarray(pages.transpose(0, 2, 1, 3)))
    _check_quarter(engine, pages, threshold=77, ratio=5)


def test_quarter_large_page_blank_pages_and_single_lines(engine):
    page = synth.synth_page(3508, 2480, 21)[0]
    _, s = _check_quarter(engine, page[None])
    assert s[0] == 0
    _, s = _check_quarter(engine, np.rot90(page, 1)[None])
    assert s[0] == 1
    for value in (255, 0):
        for shape in ((2, 64, 100, 3), (1, 100, 64, 3), (1, 1, 1, 3), (1, 1, 300, 3), (1, 300, 1, 3)):
            e, s = _check_quarter(engine, np.full(shape, value, np.uint8))
            assert not e.any() and not s.any()
    rng = np.random.default_rng(9)
    _check_quarter(engine, rng.integers(0, 256, (2, 1, 300, 3), dtype=np.uint8))
    _check_quarter(engine, rng.integers(0, 256, (2, 300, 1, 3), dtype=np.uint8))
    # the ratio on the device, on pages small enough to count by hand
    stay = np.full((1, 2, 6, 3), 255, np.uint8)
    stay[0, 0, [0, 2, 4]] = 0        # r = 3 0 -> E_r = 9, c = 1 0 1 0 1 0 -> E_c = 5
    e, s = _quarter(engine, stay)
    assert e.tolist() == [[9, 5]] and s[0] == 0
    tall = np.full((1, 6, 2, 3), 255, np.uint8)
    tall[0, [0, 2, 4, 5], 0] = 0     # E_r = 4, E_c = 16
    e, s = _quarter(engine, tall)
    assert e.tolist() == [[4, 16]] and s[0] == 1
    e, s = _quarter(engine, tall, ratio=4)      # 16 > 4 * 4 is false
    assert e.tolist() == [[4, 16]] and s[0] == 0


def test_quarter_batch_of_64_a4_pages_in_mixed_rotations(engine):
    h, w = synth.A4_200DPI
    portrait = [synth.synth_page(h, w, 30 + i, n_lines=40 + 5 * i, ruled=bool(i & 1))[0] for i in range(4)]
    landscape = [synth.synth_page(w, h, 40 + i, n_lines=30 + 3 * i, ruled=bool(i & 1))[0] for i in range(4)]
    base = []   # all h x w: upright, upside-down, and the landscape renderings lying on either side
    for i in range(4):
        base += [portrait[i], np.rot90(landscape[i], 1), np.rot90(portrait[i], 2), np.rot90(landscape[i], 3)]
    pages = np.stack([base[(5 * i) % 16] for i in range(64)])
    e, s = _check_quarter(engine, pages)
    assert s.tolist() == [((5 * i) % 16) & 1 for i in range(64)]
    assert engine.lib.lumina_ocr_page_quarter_workspace_bytes(64, h, w) > 0 and engine.lib.lumina_ocr_page_quarter_workspace_bytes(1, 70000, w) == 0


@pytest.mark.parametrize("shape", [(1, 1), (63, 65), (1414, 2000)])
def test_page_turn_equals_rot90(engine, shape):
    rng = np.random.default_rng(shape[0])
    pages = rng.integers(0, 256, (4,) + shape + (3,), dtype=np.uint8)
    index = [2, 0, 2, 3, 3]                     # repeats page 2 and 3, skips page 1
    dev = torch.from_numpy(pages).cuda()
    idx = torch.tensor(index, dtype=torch.int32, device="cuda")
    for t in range(4):
        out = engine.page_turn(dev, idx, t)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert got.shape == (5,) + (shape[::-1] if t & 1 else shape) + (3,)
        for j, i in enumerate(index):
            assert np.array_equal(got[j], np.rot90(pages[i], t)), (t, j)
    assert engine.page_turn(dev, idx[:0], 1).shape[0] == 0
    with pytest.raises(ValueError):
        engine.page_turn(dev, idx, 4)


def test_page_vote_equals_a_numpy_count(engine):
    rng = np.random.default_rng(17)
    pages = 9
    idx = np.sort(rng.choice([0, 1, 3, 4, 7], 700)).astype(np.int32)     # pages 2, 5, 6, 8 have no lines
    flip = (rng.random(700) < 0.4).astype(np.int32)
    got = engine.page_vote(torch.from_numpy(flip).cuda(), torch.from_numpy(idx).cuda(), pages)
    torch.cuda.synchronize()
    ref = pr.vote_counts(flip, idx, pages)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), ref)
    assert ref[2].tolist() == [0, 0] and np.array_equal(ref[:, 0], np.bincount(idx, minlength=pages))
    none = engine.page_vote(torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"), 3)
    assert none.cpu().numpy().tolist() == [[0, 0]] * 3


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights():
    return arch.make_det_weights(1234), arch.make_rec_weights(4321, code_path=True), arch.make_cls_weights(2718, orientation_path=True)


@pytest.fixture(scope="module")
def page():
    return synth.synth_page(H, W, 3, n_lines=10, ruled=True)[0]


def _pipe(engine, weights, **kw):
    det_w, rec_w, cls_w = weights
    engine.load_det(det_w)
    engine.load_rec(rec_w)
    engine.load_cls(cls_w)
    return OcrPipeline(engine, max_dimension=2000, post=arch.TEXT_PATH_POST, **kw)


def _dev(pages):
    return torch.from_numpy(np.ascontiguousarray(pages)).cuda()


def _same(a, b, turn=True):
    """two PageDetections, field by field"""
    assert a.texts == b.texts and (a.width, a.height) == (b.width, b.height)
    for f in ("quads", "scores", "det_scores", "text_ids", "lens", "cls_labels", "cls_scores", "hrules", "vrules", "marks"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), f
    assert not turn or a.turn == b.turn


def test_the_four_rotations_of_a_page_give_one_result(engine, weights, page):
    pipe = _pipe(engine, weights, page_orient=True, angle_cls=True, tables=True)
    ref = pr.run_pages(*weights, [np.rot90(page, k) for k in range(4)], pipe.charset, post=arch.TEXT_PATH_POST)
    first = None
    for k in range(4):
        dets, processed = pipe.run_oriented(_dev(np.rot90(page, k)[None]))
        d, p = dets[0], processed[0].cpu().numpy()
        assert d.turn == (4 - k) % 4 == ref[k]["turn"], (k, d.turn)
        assert len(d.texts) >= 8 and (d.cls_labels == 0).all() and d.hrules is not None
        assert p.shape == (H, W, 3) and (d.height, d.width) == (H, W)
        if first is None:
            first = (d, p)
        _same(d, first[0], turn=False)
        assert np.array_equal(p, first[1])
        r = ref[k]
        assert np.array_equal(d.quads, r["quads"]) and d.texts == r["texts"] and np.array_equal(d.cls_labels, r["labels"])
        assert np.array_equal(p, r["processed"])
    # and that result is the one of the upright page without the option
    plain, pp = _pipe(engine, weights, angle_cls=True, tables=True).run(_dev(page[None]))
    _same(first[0], plain[0], turn=False)
    assert plain[0].turn is None and np.array_equal(first[1], pp[0].cpu().numpy())


def test_a_batch_with_all_four_orientations_comes_back_in_input_order(engine, weights, page):
    tall = synth.synth_page(W, H, 8, n_lines=12, ruled=True)[0]        # rendered W x H: its quarter turns share the batch's H x W
    other = synth.synth_page(H, W, 9, n_lines=8, ruled=True)[0]
    batch = [page, np.rot90(tall, 1), np.rot90(page, 2), np.rot90(tall, 3), np.rot90(other, 2), other, np.rot90(tall, 3), np.rot90(page, 2)]
    source = [page, tall, page, tall, other, other, tall, page]
    turns = [0, 3, 2, 1, 2, 0, 1, 2]
    pipe = _pipe(engine, weights, page_orient=True, angle_cls=True)
    dets, processed = pipe.run_oriented(_dev(np.stack(batch)))
    plain = _pipe(engine, weights, angle_cls=True)
    want = {id(p): plain.run(_dev(p[None])) for p in (page, tall, other)}
    assert [d.turn for d in dets] == turns
    for d, p, src in zip(dets, processed, source):
        wd, wp = want[id(src)]
        assert len(d.texts) >= 6
        _same(d, wd[0], turn=False)
        assert np.array_equal(p.cpu().numpy(), wp[0].cpu().numpy())
    groups = pipe.run_oriented_groups(_dev(np.stack(batch)))
    assert sorted(i for idxs, _, _ in groups for i in idxs) == list(range(8))
    assert sorted(tuple(p.shape[1:3]) for _, _, p in groups) == [(H, W), (H, W), (W, H), (W, H)]


def test_an_all_upright_batch_equals_the_option_off(engine, weights, page):
    pages = np.stack([page, synth.synth_page(H, W, 9, n_lines=8, ruled=True)[0], synth.synth_page(H, W, 10, n_lines=12, ruled=True)[0],
                      np.full((H, W, 3), 255, np.uint8)])
    for kw in (dict(), dict(angle_cls=True), dict(tables=True, marks=True)):
        on, pon = _pipe(engine, weights, page_orient=True, **kw).run_oriented(_dev(pages))
        off, poff = _pipe(engine, weights, **kw).run(_dev(pages))
        for a, b, pa, pb in zip(on, off, pon, poff):
            _same(a, b, turn=False)
            assert a.turn == 0 and b.turn is None and torch.equal(pa, pb)
        assert len(on[3].texts) == 0
    blank, _ = _pipe(engine, weights, page_orient=True).run_oriented(_dev(pages[3:]))
    assert blank[0].turn == 0 and blank[0].texts == []


def test_a_page_with_two_lines_is_never_turned_by_180(engine, weights):
    two = synth.synth_page(H, W, 14, n_lines=2, ruled=True)[0]
    pipe = _pipe(engine, weights, page_orient=True, angle_cls=True)
    for k in range(4):
        dets, processed = pipe.run_oriented(_dev(np.rot90(two, k)[None]))
        assert len(dets[0].texts) == 2 and dets[0].turn == (k & 1), (k, dets[0].turn)
        assert tuple(processed[0].shape) == (H, W, 3)
    with pytest.raises(ValueError):
        _pipe(engine, weights).run_oriented(_dev(two[None]))
