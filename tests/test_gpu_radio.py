"""GPU: lumina_ocr_selection_marks_round / lumina_ocr_rules_and_marks_round through the C ABI against the restatement
(tests/radio_reference.py): the round rows and counts are EQUAL (integer definition, canonical order, no tolerance), the checkbox rows of
the new entries equal those of the unchanged lumina_ocr_selection_marks, and those equal tests/mark_reference.py on every page here."""
import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw

from lumina_ocr import arch, synth
from lumina_ocr.engine import EngineError

import mark_reference as mr
import radio_reference as rr
import table_reference as tr

pytestmark = pytest.mark.gpu

P, R = arch.MARK_PARAMS, arch.ROUND_MARK_PARAMS
SENTINEL = -7


def check(engine, pages: np.ndarray, max_marks: int = P["max_marks"], round_params: dict = None):
    """pages uint8 [n,H,W,3] -> per page (checkbox rows, round rows) of the restatements, after asserting that the device equals them:
    the new entry's two lists, and the old entry's list next to it."""
    pages = np.ascontiguousarray(pages)
    dev = torch.from_numpy(pages).cuda()
    rows, cnt, rrows, rcnt, mask = engine.selection_marks_round(dev, max_marks=max_marks, round_params=round_params, debug=True)
    old_rows, old_cnt = engine.selection_marks(dev, max_marks=max_marks)
    torch.cuda.synchronize()
    assert torch.equal(rows, old_rows) and torch.equal(cnt, old_cnt), "the checkbox rows changed with the round marks on"
    rows, cnt, rrows, rcnt, mask = rows.cpu().numpy(), cnt.cpu().numpy(), rrows.cpu().numpy(), rcnt.cpu().numpy(), mask.cpu().numpy().view(np.uint64)
    out = []
    for i, page in enumerate(pages):
        rmask, sq, rd = rr.selection_marks_round(page, rp=dict(R if round_params is None else round_params))
        assert np.array_equal(mask[i], rmask), "page %d: ink mask differs" % i
        for what, got, n_got, ref in (("checkbox", rows[i], int(cnt[i]), sq), ("round", rrows[i], int(rcnt[i]), rd)):
            assert n_got == len(ref), "page %d: %s count %d, restatement %d" % (i, what, n_got, len(ref))
            n = len(ref) if len(ref) <= max_marks else 0      # an overflowing list is not written
            assert np.array_equal(got[:n], ref[:n]), "page %d: %s rows differ\n%s\n%s" % (i, what, got[:n], ref[:n])
            assert not got[n:].any(), "page %d: %s rows past the count were written" % (i, what)
        out.append((sq, rd))
    return out


def rings_page(h: int, w: int, rings, specks=()) -> np.ndarray:
    """White page with a ring (x0, y0, diameter[, stroke[, dot]]) at every entry of rings and one ink pixel at every (x, y) of specks."""
    img = Image.new("RGB", (w, h), (255, 255, 255))
    d = ImageDraw.Draw(img)
    for x0, y0, diam, *rest in rings:
        synth._draw_radio(d, x0, y0, diam, rest[0] if rest else max(1, diam // 16), bool(rest[1]) if len(rest) > 1 else False, (10, 10, 10))
    page = np.asarray(img, np.uint8).copy()
    for x, y in specks:
        if 0 <= x < w and 0 <= y < h:
            page[y, x] = 0
    return page


# the hard windows on one page of 576 x 420: x0 & 63 in {0, 1, 63 - w / 2, 63} at diameter 30; diameter 64 at x0 & 63 = 0 and 37;
# diameter min_side; and a ring whose band leaves the page at row 0, row H - 1, column 0 and column W - 1
HW_H, HW_W = 420, 576
HARD = [(64, 60, 30), (193, 60, 30, 2, True), (256 + 63 - 15, 60, 30), (447, 60, 30, 1, True),
        (128, 120, 64, 3), (256 + 37, 120, 64, 4, True), (70, 130, 12, 1),
        (200, 0, 30), (200, HW_H - 30, 30, 2, True), (0, 250, 30), (HW_W - 30, 250, 30, 2, True)]


def test_hard_windows_and_the_band_one_pixel_in_and_out(engine):
    assert sorted({x0 & 63 for x0, _, d, *_ in HARD if d == 30} & {0, 1, 48, 63}) == [0, 1, 48, 63]
    band = lambda d: R["band_min"] + d // R["band_div"]
    inside = [[(x0 - band(d), y0 + d // 2), (x0 + d - 1 + band(d), y0 + d // 3), (x0 + d // 2, y0 - band(d)), (x0 + d // 3, y0 + d - 1 + band(d))][k % 4]
              for k, (x0, y0, d, *_) in enumerate(HARD)]
    outside = [[(x0 - band(d) - 1, y0 + d // 2), (x0 + d + band(d), y0 + d // 3), (x0 + d // 2, y0 - band(d) - 1), (x0 + d // 3, y0 + d + band(d))][k % 4]
               for k, (x0, y0, d, *_) in enumerate(HARD)]
    corner = [(x0 - band(d), y0 - band(d)) if k & 1 else (x0 + d - 1 + band(d), y0 + d - 1 + band(d)) for k, (x0, y0, d, *_) in enumerate(HARD)]
    pages = np.stack([rings_page(HW_H, HW_W, HARD), rings_page(HW_H, HW_W, HARD, inside), rings_page(HW_H, HW_W, HARD, outside),
                      rings_page(HW_H, HW_W, HARD, corner)])
    (_, plain), (_, ins), (_, outs), (_, cor) = check(engine, pages)
    boxes = lambda rows: {tuple(r[:2]) for r in rows.tolist()}
    assert boxes(plain) == {(x0, y0) for x0, y0, *_ in HARD} and len(plain) == len(HARD)
    assert [int(r[7]) for r in plain.tolist()] == [int(len(g) > 4 and g[4]) for g in sorted(HARD, key=lambda g: (g[1], g[0]))]
    on_page = lambda pts: {(x0, y0) for (x0, y0, *_), (x, y) in zip(HARD, pts) if 0 <= x < HW_W and 0 <= y < HW_H}
    assert boxes(ins) == boxes(plain) - on_page(inside) and len(on_page(inside)) >= 9        # a pixel in the band's last row / column rejects
    assert boxes(outs) == boxes(plain) and len(on_page(outside)) >= 9                        # one pixel further out does not
    assert boxes(cor) == boxes(plain) - on_page(corner) and len(on_page(corner)) >= 7        # the band's corner pixel counts too
    check(engine, np.ascontiguousarray(pages.transpose(0, 2, 1, 3)))                         # and with x and y exchanged


@pytest.mark.parametrize("w", [63, 64, 65, 130])
def test_widths(engine, w):
    rings = [(w - 24, 4, 24), (0, 50, 20, 1, True), (max(0, w - 64), 100, min(w, 64), 2)]    # at the right edge, at the left one, as wide as the page
    pages = np.stack([rings_page(200, w, rings), rings_page(200, w, rings, [(w - 30, 16), (22, 60), (w // 2, 166)]),
                      rings_page(200, w, rings, [(w - 12, 32), (10, 45)])])
    res = check(engine, pages)
    assert len(res[0][1]) == 3 and len(res[1][1]) == 0 and len(res[2][1]) == 1
    check(engine, np.ascontiguousarray(pages.transpose(0, 2, 1, 3)))


@pytest.mark.parametrize("seed", [0, 3])
def test_radio_and_decoy_pages(engine, seed):
    (page, gt), decoys = synth.synth_radio_page(seed, noise=3.0 * (seed & 1)), synth.synth_round_decoys(seed, noise=3.0 * (seed & 1))[0]
    (sq, rd), (dsq, drd) = check(engine, np.stack([page, decoys]))
    found = {tuple(r[:4]): int(r[7]) for r in rd.tolist()}
    assert found == {g["box"]: int(g["state"] == "selected") for g in gt if g["shape"] == "round"} and len(found) == 13
    assert len(drd) == 0 and len(sq) >= 3


def test_70_roots_in_one_row(engine):
    """more roots in one row of the run list than a wave has lanes: 35 small rings and 35 dots whose first runs share a row"""
    rings = [(10 + 30 * k, 10, 12, 1, bool(k & 1)) for k in range(35)]
    specks = [(10 + 30 * k + 21, 10) for k in range(35)]
    page = rings_page(40, 1100, rings, specks)
    ((sq, rd),) = check(engine, page[None])
    assert len(rd) == 35 and rd[:, 0].tolist() == [10 + 30 * k for k in range(35)] and rd[:, 7].tolist() == [k & 1 for k in range(35)]
    ink = tr.ink_mask(page, 128)
    assert int((ink[10, 1:] & ~ink[10, :-1]).sum()) + int(ink[10, 0]) >= 70


@pytest.mark.parametrize("w", [4160, 8191])
def test_long_sides(engine, w):
    """a side past 4096 pixels (a row of more than 64 mask words): rings of diameter 30 whose window starts at 4096 - k, one page a k,
    the one at k = 15 with a dot, and a ring of min_side whose last column is the page's; then with x and y exchanged"""
    offsets = (0, 1, 15, 31, 63)
    pages = np.stack([rings_page(40, w, [(4096 - k, 5, 30, 2, k == 15), (w - 12, 14, 12, 1)]) for k in offsets])
    assert P["min_side"] == 12 and w > 4096 + 30
    res = check(engine, pages)
    for k, (sq, rd) in zip(offsets, res):
        assert [r[:4] + r[7:] for r in rd.tolist()] == [[4096 - k, 5, 4096 - k + 29, 34, int(k == 15)], [w - 12, 14, w - 1, 25, 0]] and len(sq) == 0
    turned = check(engine, np.ascontiguousarray(pages.transpose(0, 2, 1, 3)))
    for (_, rd), (_, td) in zip(res, turned):
        assert td[:, [1, 0, 3, 2, 7]].tolist() == rd[:, [0, 1, 2, 3, 7]].tolist()


def test_overflow_reports_the_true_count_and_writes_no_row(engine):
    page = synth.synth_radio_page(5)[0]
    ((sq, rd),) = check(engine, page[None], max_marks=4)
    assert len(rd) == 13 > 4
    ((sq, rd),) = check(engine, page[None], max_marks=13)                                     # and a list that is exactly full
    assert len(rd) == 13


def test_other_round_parameters(engine):
    pages = np.stack([synth.synth_radio_page(1, 500, 700, n_marks=6, table=False)[0], synth.synth_round_decoys(1, 500, 700)[0]])
    for rp in (dict(out_max=40, ring_div=1, band_div=4, band_min=0), dict(out_max=0, ring_div=64, band_div=64, band_min=16),
               dict(out_max=3, ring_div=5, band_div=4, band_min=16)):
        check(engine, pages, round_params=rp)


def test_five_pages_in_ragged_groups(engine):
    pages = np.stack([synth.synth_radio_page(s, 400, 600, n_marks=2 + s, table=False, max_side=40, noise=2.0 * (s & 1))[0] for s in range(4)]
                     + [synth.synth_round_decoys(2, 400, 600)[0]])
    whole = check(engine, pages)
    engine.set_option("post_group", 2)
    try:
        split = check(engine, pages)
        both = [t.cpu().numpy() for t in engine.rules_and_marks_round(torch.from_numpy(pages).cuda())]
    finally:
        engine.set_option("post_group", 64)
    assert [len(rd) for _, rd in whole] == [len(rd) for _, rd in split] and sum(len(rd) for _, rd in whole) >= 6
    for i, (sq, rd) in enumerate(whole):
        assert int(both[4][i]) == len(sq) and int(both[6][i]) == len(rd)
        assert np.array_equal(both[3][i, :len(sq)], sq) and np.array_equal(both[5][i, :len(rd)], rd)


def test_rules_and_marks_round_equals_the_separate_calls(engine):
    pages = np.stack([synth.synth_radio_page(3)[0], synth.synth_table_page(4, n_tables=2)[0], synth.synth_marks_page(3)[0]])
    dev = torch.from_numpy(pages).cuda()
    both = engine.rules_and_marks_round(dev)
    solo = engine.table_rules(dev) + engine.selection_marks_round(dev)
    old = engine.rules_and_marks(dev)
    torch.cuda.synchronize()
    assert len(both) == len(solo) == 7 and all(torch.equal(a, b) for a, b in zip(both, solo))
    assert all(torch.equal(a, b) for a, b in zip(both[:5], old))                              # the old entry's five outputs, bit for bit
    for i, page in enumerate(pages):
        _, sq, rd = rr.selection_marks_round(page)
        assert int(both[6][i]) == len(rd) and np.array_equal(both[5][i, :len(rd)].cpu().numpy(), rd)
        assert int(both[4][i]) == len(sq) and np.array_equal(both[3][i, :len(sq)].cpu().numpy(), sq)
    assert int(both[6][0]) == 13 and int(both[6][1]) == 0 and int(both[6][2]) == 0 and int(both[2][1].sum()) >= 6


@pytest.mark.parametrize("bad", [dict(band_div=3), dict(band_min=17), dict(band_min=-1), dict(ring_div=0), dict(out_max=-1)])
def test_bad_round_parameters_are_an_error_and_write_nothing(engine, bad):
    pages = torch.from_numpy(synth.synth_radio_page(1, 400, 600, n_marks=4, table=False)[0][None]).cuda()
    outs = [torch.full(s, SENTINEL, dtype=torch.int32, device="cuda") for s in ((1, 8, 8), (1,), (1, 8, 8), (1,))]
    rp = dict(R, **bad)
    rc = engine.lib.lumina_ocr_selection_marks_round(engine._h, pages.data_ptr(), 1, 400, 600, 128, 12, 64, 8, outs[0].data_ptr(), outs[1].data_ptr(), None,
                                                     rp["out_max"], rp["ring_div"], rp["band_div"], rp["band_min"], outs[2].data_ptr(), outs[3].data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and b"selection_marks_round" in engine.lib.lumina_ocr_last_error(engine._h)
    assert all(bool((t == SENTINEL).all()) for t in outs)
    with pytest.raises(EngineError):
        engine.selection_marks_round(pages, round_params=rp)
    rc = engine.lib.lumina_ocr_selection_marks_round(engine._h, pages.data_ptr(), 1, 400, 600, 128, 12, 64, 8, outs[0].data_ptr(), outs[1].data_ptr(), None,
                                                     R["out_max"], R["ring_div"], R["band_div"], R["band_min"], None, outs[3].data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and all(bool((t == SENTINEL).all()) for t in outs)                        # a round list without its counts' partner
