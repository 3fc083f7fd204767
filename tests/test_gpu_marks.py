"""GPU: lumina_ocr_selection_marks through the C ABI against the restatement (tests/mark_reference.py): the ink mask (parity hook), the
rows and the counts are EQUAL — the definition is integer arithmetic with a canonical order, so there is no tolerance."""
import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw

from lumina_ocr import arch, synth
from lumina_ocr.engine import EngineError

import mark_reference as mr
import table_reference as tr

pytestmark = pytest.mark.gpu

P = arch.MARK_PARAMS


def check(engine, pages: np.ndarray, **params):
    """pages uint8 [n,H,W,3] -> the per-page rows of the restatement, after asserting the device's output equals them."""
    kw = {k: params.get(k, P[k]) for k in ("threshold", "min_side", "max_side")}
    cap = params.get("max_marks", P["max_marks"])
    rows, cnt, mask = engine.selection_marks(torch.from_numpy(np.ascontiguousarray(pages)).cuda(), max_marks=cap, debug=True, **kw)
    torch.cuda.synchronize()
    rows, cnt, mask = rows.cpu().numpy(), cnt.cpu().numpy(), mask.cpu().numpy().view(np.uint64)
    out = []
    for i, page in enumerate(pages):
        rmask, ref = mr.selection_marks(page, **kw)
        assert np.array_equal(mask[i], rmask), "page %d: ink mask differs" % i
        assert int(cnt[i]) == len(ref), "page %d: count %d, restatement %d" % (i, cnt[i], len(ref))
        n = len(ref) if len(ref) <= cap else 0      # an overflowing list is not written; rows past the count are untouched
        assert np.array_equal(rows[i, :n], ref[:n]), "page %d: rows differ\n%s\n%s" % (i, rows[i, :n], ref[:n])
        assert not rows[i, n:].any(), "page %d: rows past the count were written" % i
        out.append(ref)
    return out


def boxes_page(h: int, w: int, corners, side: int = 20, stroke: int = 2, kinds=None) -> np.ndarray:
    """White page with a box of `side` at every (x0, y0) of corners, its kind cycling through synth.MARK_KINDS."""
    img = Image.new("RGB", (w, h), (255, 255, 255))
    d = ImageDraw.Draw(img)
    for k, (x0, y0) in enumerate(corners):
        synth._draw_mark(d, x0, y0, side, stroke, (kinds or synth.MARK_KINDS)[k % len(kinds or synth.MARK_KINDS)], (10, 10, 10))
    return np.asarray(img, np.uint8).copy()


def noise_page(h: int, w: int, seed: int, density: float) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.repeat(np.where(rng.random((h, w, 1)) < density, 0, 255).astype(np.uint8), 3, axis=2)


@pytest.mark.parametrize("seed,stroke,noise", [(0, 0, 0.0), (1, 1, 3.0), (2, 2, 0.0), (3, 3, 3.0), (4, 4, 3.0)])
def test_marks_pages(engine, seed, stroke, noise):
    pages, gts = zip(*[synth.synth_marks_page(seed + 10 * k, stroke=stroke, noise=noise) for k in (0, 1)])
    for rows, gt in zip(check(engine, np.stack(pages)), gts):
        found = {tuple(r[:4]): int(r[7]) for r in rows.tolist()}
        assert len(gt) == 16 and all(found.get(g["box"]) == int(g["state"] == "selected") for g in gt)


def test_text_form_and_table_pages_have_no_marks(engine):
    plain = np.stack([synth.synth_page(700, 1000, s, n_lines=16)[0] for s in range(3)])
    assert all(len(r) == 0 for r in check(engine, plain))
    assert len(check(engine, synth.synth_form_page(0)[0][None])[0]) == 0
    assert len(check(engine, synth.synth_table_page(3, n_tables=2)[0][None])[0]) == 0


def test_a_box_at_every_bit_offset_of_the_mask_word(engine):
    """x0 % 64 in 0..63: the window of a box is cut from one word or from two"""
    for side in (20, 33, 64):
        corners = [(64 * (k % 8) * 3 + k, 10 + (k // 8) * (side + 12)) for k in range(64)]
        assert sorted(c[0] % 64 for c in corners) == list(range(64))
        rows, = check(engine, boxes_page(8 * (side + 12) + 20, 64 * 3 * 8 + 80, corners, side=side, stroke=1 + side // 20)[None])
        assert len(rows) >= 64 and {tuple(r[:2]) for r in rows.tolist()} >= set(corners)


@pytest.mark.parametrize("h,w", [(200, 300), (63, 200), (200, 64), (65, 65)])
def test_boxes_at_the_corners_and_edges_of_the_page(engine, h, w):
    s = 24
    corners = [(0, 0), (w - s, 0), (0, h - s), (w - s, h - s)]
    if h >= 100 and w >= 100:
        corners += [(w // 2, 0), (w // 2, h - s), (0, h // 2 - s // 2), (w - s, h // 2 - s // 2)]
    rows, = check(engine, boxes_page(h, w, corners, side=s)[None])
    assert {tuple(r[:2]) for r in rows.tolist()} >= set(corners)


@pytest.mark.parametrize("w", [63, 64, 65, 1414])
def test_widths(engine, w):
    pages = []
    for s in range(3):
        pg = boxes_page(200, w, [(max(0, w - 30 - 7 * s), 5 + 3 * s), (3 * s, 60), (min(w - 41, 40 + s), 120)], side=30 + 5 * s)
        dots = np.random.default_rng(s).integers(0, [200, w], (300, 2))
        pg[dots[:, 0], dots[:, 1]] = 0
        pages.append(pg)
    pages = np.stack(pages)
    check(engine, pages)
    check(engine, np.ascontiguousarray(pages.transpose(0, 2, 1, 3)))     # the same as heights


def test_blank_all_ink_and_grey_pages(engine):
    pages = np.stack([np.full((150, 300, 3), 255, np.uint8), np.zeros((150, 300, 3), np.uint8), np.full((150, 300, 3), 128, np.uint8)])
    assert all(len(r) == 0 for r in check(engine, pages))
    rows, = check(engine, np.zeros((1, 40, 40, 3), np.uint8))                 # a page that is one filled square: one selected mark
    assert rows.tolist() == [[0, 0, 39, 39, 160, 400, 400, 1]]


@pytest.mark.parametrize("density", [0.05, 0.3, 0.5])
def test_noise_pages(engine, density):
    """components of every shape, many runs per row, long union chains"""
    check(engine, np.stack([noise_page(160, 200, s, density) for s in range(3)]))
    check(engine, np.stack([np.minimum(noise_page(120, 150, s, density / 4), boxes_page(120, 150, [(5, 5), (70, 40), (100, 80)], side=28)) for s in range(3)]))


def test_overflow_reports_the_true_count(engine):
    page = synth.synth_marks_page(7)[0]
    rows, = check(engine, page[None], max_marks=4)
    assert len(rows) > 4


@pytest.mark.parametrize("params", [dict(threshold=100, min_side=4, max_side=64, max_marks=2048),
                                    dict(threshold=200, min_side=30, max_side=40, max_marks=16),
                                    dict(threshold=128, min_side=12, max_side=12, max_marks=256),
                                    dict(threshold=128, min_side=20, max_side=63, max_marks=1)])
def test_other_parameters(engine, params):
    pages = np.stack([synth.synth_marks_page(2, 500, 700, n_marks=6, table=False)[0], synth.synth_page(500, 700, 2, n_lines=10)[0],
                      boxes_page(500, 700, [(10 + 70 * k, 10 + 60 * k) for k in range(7)], side=12, stroke=2), noise_page(500, 700, 3, 0.02)])
    check(engine, pages, **params)


def test_zero_pages_is_a_no_op(engine):
    rows, cnt = engine.selection_marks(torch.zeros((0, 100, 100, 3), dtype=torch.uint8, device="cuda"))
    assert tuple(cnt.shape) == (0,) and tuple(rows.shape) == (0, P["max_marks"], 8)


def test_a4_batch_of_64_different_pages(engine):
    h, w = synth.A4_200DPI
    base = [synth.synth_marks_page(s, h, w, n_marks=24, noise=3.0 * (s & 1))[0] for s in range(4)]
    base += [synth.synth_page(h, w, 11, n_lines=40)[0], synth.synth_table_page(5, h, w, n_tables=3)[0],
             np.minimum(synth.synth_page(h, w, 12, n_lines=40)[0], synth.synth_marks_page(9, h, w, n_marks=8, table=False)[0]), synth.synth_marks_page(6, h, w, side=40)[0]]
    pages = np.stack([np.roll(base[i % 8], (37 * (i // 8), 53 * (i // 8)), axis=(0, 1)) for i in range(64)])
    assert len({pg.tobytes() for pg in pages}) == 64
    res = check(engine, pages)
    with_marks = [r.tobytes() for r in res if len(r)]
    assert len(with_marks) == 48 and len(set(with_marks)) == 48      # every page with marks has a result of its own; text and table pages have none


@pytest.mark.parametrize("bad", [dict(max_side=65), dict(min_side=3), dict(max_marks=2049), dict(max_marks=0), dict(min_side=40, max_side=30)])
def test_bad_arguments_are_an_error_and_write_nothing(engine, bad):
    pages = torch.from_numpy(synth.synth_marks_page(1, 400, 600, n_marks=4, table=False)[0][None]).cuda()
    kw = dict(threshold=128, min_side=12, max_side=64, max_marks=8)
    kw.update(bad)
    marks = torch.full((1, 8, 8), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    rc = engine.lib.lumina_ocr_selection_marks(engine._h, pages.data_ptr(), 1, 400, 600, kw["threshold"], kw["min_side"], kw["max_side"], kw["max_marks"],
                                               marks.data_ptr(), counts.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and b"selection_marks" in engine.lib.lumina_ocr_last_error(engine._h)
    assert bool((marks == -7).all()) and bool((counts == -7).all())
    with pytest.raises(EngineError):
        engine.selection_marks(pages, **kw)


def test_rules_and_marks_share_the_mask_and_equal_the_solo_calls(engine):
    pages = np.stack([synth.synth_marks_page(3)[0], synth.synth_table_page(4, n_tables=2)[0], synth.synth_page(1100, 1500, 5, n_lines=20, ruled=True)[0]])
    dev = torch.from_numpy(pages).cuda()
    both = engine.rules_and_marks(dev)
    solo = engine.table_rules(dev) + engine.selection_marks(dev)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(both, solo))
    for i, page in enumerate(pages):
        _, rh, rv = tr.table_rules(page)
        ref = mr.selection_marks(page)[1]
        assert both[2][i].tolist() == [len(rh), len(rv)] and int(both[4][i]) == len(ref)
        assert np.array_equal(both[0][i, :len(rh)].cpu().numpy(), rh) and np.array_equal(both[1][i, :len(rv)].cpu().numpy(), rv)
        assert np.array_equal(both[3][i, :len(ref)].cpu().numpy(), ref)
    assert int(both[4][0]) >= 16 and int(both[2][1].sum()) >= 6
