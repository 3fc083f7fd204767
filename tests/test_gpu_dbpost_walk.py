"""GPU: the DB post-process where its kernels walk or reduce (csrc/dbpost.hip) and both crop kernels, against the oracle per page.

comp_box walks the list of live components with a grid of what is resident, rl_extent lets only the runs without a run below them
report a bottom row, rl_extremes reduces a row's runs per component inside the wave, and crop_kernel stores four columns per thread.
Maps are built like test_db_postprocess_structured_maps: a noise floor below the threshold, ink between 0.5 and 1.0.

Not here, and why:
  * several rows per wave (map heights R*k - 1, R*k, R*k + 1 and a page border inside a wave's rows): the run-list passes still
    take one row per wave, so there is no R;
  * a crop of valid width 1: a quad that is not turned has ch < 1.5 cw, so its width is at least ceil(32 / 1.5) = 22 (32 rows) or
    32 (48 rows), and a turned one is wider still; the 1-pixel-wide quads below are the narrowest input there is (turned, width at
    the cap)."""
import numpy as np
import pytest
import torch

from lumina_ocr import arch
from oracle import dbpost

import cls_reference as cr

pytestmark = pytest.mark.gpu


def _noise(shape, seed):
    return np.random.default_rng(seed).random(shape, dtype=np.float32) * 0.25


def _dots(hp=256, wp=320, seed=1):
    """3 x 3 dots at a 6-pixel pitch, 3 pixels off the borders (a box on the border is clamped and dropped), on a noise floor:
    42 x 52 = 2184 components"""
    p = _noise((hp, wp), seed)
    val = np.random.default_rng(seed + 100).uniform(0.5, 1.0, (hp, wp)).astype(np.float32)
    yy, xx = np.mgrid[0:hp, 0:wp]
    ink = ((yy - 3) % 6 < 3) & ((xx - 3) % 6 < 3) & (yy >= 3) & (xx >= 3) & (yy - (yy - 3) % 6 + 2 < hp - 3) & (xx - (xx - 3) % 6 + 2 < wp - 3)
    p[ink] = val[ink]
    return p


N_DOTS = 42 * 52


def _blobs(n, hp=256, wp=320, seed=2):
    """n rectangles of 8 x 20 pixels on a grid, apart from each other"""
    p = _noise((hp, wp), seed)
    rng = np.random.default_rng(seed + 100)
    for k in range(n):
        y, x = 4 + 12 * (k // 10), 4 + 30 * (k % 10)
        p[y:y + 8, x:x + 20] = rng.uniform(0.5, 1.0)
    return p


def _check(engine, prob, vh, vw, **params):
    """-> (device counts, oracle component counts) per page, after comparing boxes, scores, counts and the zero tail per page"""
    bits = arch.f32_to_bf16_bits(np.ascontiguousarray(prob, np.float32))
    pd = torch.from_numpy(bits.view(np.int16)).cuda().view(torch.bfloat16)
    boxes, scores, counts = engine.det_postprocess(pd, vh, vw, **params)
    torch.cuda.synchronize()
    boxes, scores, counts = boxes.cpu().numpy(), scores.cpu().numpy(), counts.cpu().numpy()
    oparams = {("max_candidates" if k == "max_boxes" else k): v for k, v in params.items()}
    got, comps = [], []
    for i in range(prob.shape[0]):
        rb, rs, ncomp = dbpost.db_postprocess(bits[i], vh, vw, **oparams)
        n = int(counts[i])
        assert n == len(rb), (i, n, len(rb), ncomp, params)
        assert np.array_equal(boxes[i, :n], rb), (i, params)
        assert np.array_equal(scores[i, :n], rs), (i, params)
        assert not boxes[i, n:].any() and not scores[i, n:].any(), (i, params)
        got.append(n)
        comps.append(ncomp)
    return got, comps


@pytest.fixture(scope="module")
def dot_maps():
    return np.stack([_dots(seed=1), _dots(seed=2)])


@pytest.mark.parametrize("min_size", [3, 1])
def test_more_live_components_than_resident_work_groups(engine, dot_maps, min_size):
    """2 x 2184 components under a cap of 4096: every work-group of comp_box takes several.  min_size 1 keeps the dots as boxes
    (their short side is 2), the default drops them all after the walk."""
    got, comps = _check(engine, dot_maps, 256, 320, max_boxes=4096, min_size=min_size)
    assert comps == [N_DOTS, N_DOTS], comps
    assert got == ([N_DOTS, N_DOTS] if min_size == 1 else [0, 0]), got


@pytest.mark.parametrize("cap", [16, 1])
def test_cap_keeps_the_first_components_in_raster_order(engine, dot_maps, cap):
    got, comps = _check(engine, dot_maps, 256, 320, max_boxes=cap, min_size=1)
    assert got == [cap, cap] and min(comps) > cap, (got, comps)


def test_ragged_batches(engine):
    """Pages of 0, 1, 2184, 0 and 37 components in one call, then one empty page alone."""
    empty = _noise((256, 320), 5)
    one = _noise((256, 320), 6); one[100:112, 40:90] = 0.8
    pages = np.stack([empty, one, _dots(seed=3), _noise((256, 320), 7), _blobs(37)])
    got, comps = _check(engine, pages, 256, 320, max_boxes=4096, min_size=1)
    assert comps == [0, 1, N_DOTS, 0, 37] and got[:4] == comps[:4] and 20 < got[4] <= 37, (got, comps)   # (some blobs score below box_thresh)
    got, comps = _check(engine, empty[None], 256, 320, max_boxes=4096, min_size=1)
    assert got == [0] and comps == [0]


def test_no_stale_flags_from_the_call_before(engine):
    """The same workspace twice: a dense page, then an empty one.  Slots of the first call's components must not count in the second."""
    dense, empty = _dots(seed=4)[None], _noise((1, 256, 320), 8)
    got, _ = _check(engine, dense, 256, 320, max_boxes=4096, min_size=1)
    assert N_DOTS - 20 < got[0] <= N_DOTS, got      # (a few dots of this seed average below box_thresh)
    got, comps = _check(engine, empty, 256, 320, max_boxes=4096, min_size=1)
    assert got == [0] and comps == [0]
    few = _blobs(5)[None]                       # and fewer components than before: the rest of the first call's slots stay out
    got, comps = _check(engine, few, 256, 320, max_boxes=4096, min_size=1)
    assert comps == [5] and 1 <= got[0] <= 5, (got, comps)


def _shapes(hp, wp, vh):
    """A U, an inverted U, a staircase joined only through corners, a bar whose lowest run lies in the last valid row and one that ends
    a row above it"""
    p = _noise((hp, wp), 9)
    p[10:60, 10:16] = 0.9; p[10:60, 40:46] = 0.8; p[54:60, 10:46] = 0.7                     # U: two tops, one bottom
    p[10:16, 60:100] = 0.9; p[10:50, 60:66] = 0.8; p[10:70, 94:100] = 0.7                   # inverted U: one top, two bottoms of unequal depth
    for k in range(30):
        p[80 + k, 10 + 4 * k:14 + 4 * k] = 0.6 + 0.01 * k                                    # staircase, 8-connected only
    p[vh - 30:vh, 150:160] = 0.9                                                             # reaches the last valid row (and is cut there)
    p[vh - 30:hp, 170:180] = 0.85                                                            # runs on below the valid height
    p[vh - 31:vh - 1, 200:210] = 0.8                                                         # ends one row above the last valid row
    p[20:40, 230:300] = 0.75; p[26:34, 250:280] = 0.1                                        # a ring: one component around a hole
    return p


@pytest.mark.parametrize("vh", [128, 127, 120])
def test_bottoms_and_tops(engine, vh):
    got, comps = _check(engine, _shapes(128, 320, vh)[None], vh, 320)
    assert comps == [7] and got[0] >= 4, (got, comps)              # (the staircase and the thinner shapes fall to min_size)


@pytest.mark.parametrize("vh", [2304, 2303])
def test_tall_component_to_the_last_row(engine, vh):
    """More than 2048 rows tall (the hull's global scratch), ending in the last row of the map: at the valid height and one above it."""
    p = np.zeros((1, 2304, 64), np.float32)
    p[0, 100:2304, 10:18] = 0.9
    p[0, 5:40, 30:50] = 0.8
    p[0, 2200:2303, 40:50] = 0.7
    got, comps = _check(engine, p, vh, 64)
    assert comps == [3] and got == [3], (got, comps)


def test_rows_with_more_than_64_runs(engine):
    """A 1-pixel comb of 150 teeth under one spine: every tooth row holds 150 runs of one component, over three batches of 64, with a
    bar of its own between two teeth (another component inside a batch) and a second comb upside down (its spine is its bottom)."""
    p = _noise((2, 96, 320), 10)
    p[0, 8:12, 4:304] = 0.9
    p[0, 12:60, 4:304:2] = 0.8
    p[0, 12:60, 5:304:2] = 0.0
    p[0, 20:60, 130:170] = 0.0; p[0, 24:56, 140:160] = 0.7                                  # a window in the comb with a bar inside it
    p[1, 70:74, 10:310] = 0.9
    p[1, 20:70, 10:310:2] = 0.8
    p[1, 20:70, 11:310:2] = 0.0
    p[1, 4:12, 100:200] = 0.75
    got, comps = _check(engine, p, 96, 320, box_thresh=0.3)             # (half of a comb's rectangle is background)
    assert comps == [2, 2] and got == [2, 2], (got, comps)


def test_unaligned_map_width(engine):
    """A map whose rows do not start on 16-byte boundaries: the score sweep's 2-byte path."""
    rng = np.random.default_rng(11)
    hp, wp = 90, 203
    yy, xx = np.mgrid[0:hp, 0:wp]
    p = _noise((2, hp, wp), 12)
    for k in range(16):
        cx, cy, ang = rng.uniform(0, wp), rng.uniform(0, hp), rng.uniform(-1.5, 1.5)
        hl, hw = rng.uniform(8, 30), rng.uniform(2, 6)
        u = (xx - cx) * np.cos(ang) + (yy - cy) * np.sin(ang)
        v = -(xx - cx) * np.sin(ang) + (yy - cy) * np.cos(ang)
        p[k % 2][(np.abs(u) < hl) & (np.abs(v) < hw)] = rng.uniform(0.5, 1.0)
    got, _ = _check(engine, p, 87, 201, box_thresh=0.5)
    assert sum(got) > 4, got


# ---- crops ----
CROP_H, CROP_W = 157, 203          # page sides that are no multiple of 4

QUADS = [
    [20, 30, 150, 30, 150, 60, 20, 60],            # upright, inside the page
    [15, 40, 180, 52, 178, 80, 13, 68],            # skewed
    [-12, -9, 90, -9, 90, 14, -12, 14],            # over the top and left borders
    [120, 140, 230, 140, 230, 170, 120, 170],      # over the bottom and right borders
    [-20, 70, 230, 70, 230, 90, -20, 90],          # over both sides
    [60, -30, 100, -30, 100, 200, 60, 200],        # tall (turned), over top and bottom
    [10, 10, 11, 10, 11, 70, 10, 70],              # 1 pixel wide: turned, width at the cap
    [30, 100, 31, 100, 31, 101, 30, 101],          # 1 x 1
    [0, 50, 203, 50, 203, 56, 0, 56],              # much wider than the cap allows: width clamped
    [40, 40, 100, 40, 100, 79, 40, 79],            # 4 ch^2 < 9 cw^2 by a little: not turned
    [40, 40, 100, 40, 100, 130, 40, 130],          # 4 ch^2 = 9 cw^2: turned
    [50, 20, 110, 20, 110, 109, 50, 109],          # just below: not turned
    [150, 90, 60, 110, 64, 130, 154, 110],         # corners in another order (right to left)
    [5, 5, 5, 5, 5, 5, 5, 5],                      # degenerate: a point
    [0, 0, 10, 0, 10, 0, 0, 0],                    # degenerate: no height
    [7, 3, 7, 3, 7, 30, 7, 30],                    # degenerate: no width (turned, then no height)
    [202, 156, 260, 156, 260, 190, 202, 190],      # only the page's last pixel, the rest clamped
]


@pytest.fixture(scope="module")
def crop_inputs():
    rng = np.random.default_rng(21)
    pages = rng.integers(0, 256, (2, CROP_H, CROP_W, 3), dtype=np.uint8)
    quads = np.array(QUADS + QUADS, np.int32)
    page_idx = np.array([0] * len(QUADS) + [1] * len(QUADS), np.int32)
    return pages, quads, page_idx


def test_rec_crops_32x320(engine, crop_inputs):
    """flip clear against oracle.dbpost.rec_crop; flip set against the restatement of the turned crop (itself pinned to the oracle)."""
    pages, quads, page_idx = crop_inputs
    pg, qd, pi = torch.from_numpy(pages).cuda(), torch.from_numpy(quads).cuda(), torch.from_numpy(page_idx).cuda()
    flip = (np.arange(len(quads)) % 2).astype(np.int32)
    plain, w0 = engine.rec_crop(pg, qd, pi)
    turned, w1 = engine.rec_crop(pg, qd, pi, flip=torch.from_numpy(flip).cuda())
    inverse, w2 = engine.rec_crop(pg, qd, pi, flip=torch.from_numpy(1 - flip).cuda())
    plain, turned, inverse = plain.cpu().numpy(), turned.cpu().numpy(), inverse.cpu().numpy()
    w0, w1, w2 = w0.cpu().numpy(), w1.cpu().numpy(), w2.cpu().numpy()
    assert np.array_equal(w0, w1) and np.array_equal(w0, w2)
    for i, q in enumerate(quads):
        ref, wc = dbpost.rec_crop(pages[page_idx[i]], q)
        assert w0[i] == wc and np.array_equal(plain[i], ref), (i, q.tolist())
        for out, f in ((turned, flip[i]), (inverse, 1 - flip[i])):
            want, _ = cr.crop(pages[page_idx[i]], q, 32, 320, flip=bool(f))
            assert np.array_equal(out[i], want), (i, int(f), q.tolist())
    assert 0 in w0.tolist() and 320 in w0.tolist() and any(0 < w < 320 for w in w0.tolist())


def test_cls_crops_48x192(engine, crop_inputs):
    pages, quads, page_idx = crop_inputs
    crops, widths = engine.cls_crop(torch.from_numpy(pages).cuda(), torch.from_numpy(quads).cuda(), torch.from_numpy(page_idx).cuda())
    crops, widths = crops.cpu().numpy(), widths.cpu().numpy()
    for i, q in enumerate(quads):
        ref, wc = cr.crop(pages[page_idx[i]], q)
        assert widths[i] == wc and np.array_equal(crops[i], ref), (i, q.tolist())
    assert 0 in widths.tolist() and 192 in widths.tolist() and any(0 < w < 192 for w in widths.tolist())


def test_crop_geometry_cases_are_what_they_claim():
    """(no device) the quads above do reach the branches they are named for"""
    cw2 = lambda q: max((q[2] - q[0]) ** 2 + (q[3] - q[1]) ** 2, (q[4] - q[6]) ** 2 + (q[5] - q[7]) ** 2)
    ch2 = lambda q: max((q[6] - q[0]) ** 2 + (q[7] - q[1]) ** 2, (q[4] - q[2]) ** 2 + (q[5] - q[3]) ** 2)
    assert 4 * ch2(QUADS[10]) == 9 * cw2(QUADS[10]) and 4 * ch2(QUADS[9]) < 9 * cw2(QUADS[9]) and 4 * ch2(QUADS[11]) < 9 * cw2(QUADS[11])
    assert [cr.crop_width(q, 32, 320) for q in QUADS[13:16]] == [0, 0, 0]
    assert cr.crop_width(QUADS[6], 32, 320) == 320 and cr.crop_width(QUADS[8], 32, 320) == 320
