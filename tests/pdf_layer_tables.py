"""The layer tables of tests/test_gpu_pdf_layers.py, shared with the sanitized host program's test (tests/test_compose_sanitized.py):
(name, (H, W), pages, layers) with layers as pdf_layers_reference.compose takes them, and the tables compose_params_ok rejects."""
import numpy as np

ALPHAS = (0, 1, 127, 128, 254, 255)
WIDTHS, HEIGHTS = (1, 5, 15, 16, 17, 67), (1, 3, 70)


def _img(rng, h, w, alphas=False):
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if alphas:   # channel 0 is what a mask is read from: the blend's edge values, often
        pick = rng.integers(0, 2, (h, w)).astype(bool)
        a[:, :, 0] = np.where(pick, np.asarray(ALPHAS, np.uint8)[rng.integers(0, len(ALPHAS), (h, w))], a[:, :, 0])
    return a


def random_layers(rng, page, count, H, W):
    """layers of every kind and polarity; rectangles that meet the canvas and stick out of it; sources shown sample for pixel and scaled"""
    out = []
    for k in range(count):
        kind, flip = int(rng.integers(0, 4)) if k >= 8 else k % 4, int(rng.integers(0, 2)) if k >= 8 else (k // 4) % 2
        x0, y0 = int(rng.integers(-6, W)), int(rng.integers(-6, H))
        x1, y1 = int(rng.integers(max(x0, 0) + 1, W + 7)), int(rng.integers(max(y0, 0) + 1, H + 7))
        same = rng.integers(0, 2, 2).astype(bool)
        sw, sh = (x1 - x0 if same[0] else int(rng.integers(1, 40))), (y1 - y0 if same[0] else int(rng.integers(1, 40)))
        mw, mh = (x1 - x0 if same[1] else int(rng.integers(1, 40))), (y1 - y0 if same[1] else int(rng.integers(1, 40)))
        src = _img(rng, sh, sw) if kind != 1 else None
        mask = _img(rng, mh, mw, alphas=True) if kind != 0 else None
        out.append((page, kind, (x0, y0, x1, y1), flip, tuple(int(v) for v in rng.integers(0, 256, 3)), src, mask))
    return out


def small_canvas(W, H):
    rng = np.random.default_rng(1000 * W + H)
    return [l for p in range(2) for l in random_layers(rng, p, 12, H, W)]


def three_pages():
    """67 x 70 = 4690 pixels a page: pages 1 and 2 start 2 and 4 pixels past a 48-byte boundary; 0, 1 and 64 layers"""
    rng = np.random.default_rng(7)
    return random_layers(rng, 1, 1, 70, 67) + random_layers(rng, 2, 64, 70, 67)


def edges():
    """67 x 70: a work-group takes 61 rows, a thread's store covers 5 1/3 pixels.  Rectangle edges at every column of one 16-pixel group
    and at the rows around the band's end."""
    rng = np.random.default_rng(11)
    layers = []
    for k, x in enumerate(range(16, 33)):
        layers.append((0, k % 4, (x, 58 + k % 5, x + 1 + k % 3, 63 + k % 4), k % 2, (k, 2 * k, 3 * k), _img(rng, 4, 3) if k % 4 != 1 else None,
                       _img(rng, 5, 2, True) if k % 4 else None))
    layers.append((0, 0, (0, 60, 67, 61), 0, (0, 0, 0), _img(rng, 1, 67), None))    # the band's last row alone
    layers.append((0, 0, (3, 61, 64, 70), 0, (0, 0, 0), _img(rng, 9, 61), None))    # from the next band's first row on
    return layers


def orders():
    """37 x 67: the identity map and 23 samples over 67 columns on one page; overlapping layers in both orders"""
    rng = np.random.default_rng(13)
    under, src, mask = _img(rng, 37, 67), _img(rng, 9, 23), _img(rng, 31, 40, True)
    a = (0, 0, (0, 0, 67, 37), 0, (0, 0, 0), under, None)                 # sample for pixel
    b = (0, 0, (0, 2, 67, 31), 0, (0, 0, 0), src, None)                   # 23 samples over 67 columns, 9 over 29 rows
    c = (0, 2, (-5, -3, 80, 40), 1, (0, 0, 0), src, mask)
    d = (0, 1, (3, 1, 50, 12), 0, (9, 8, 7), None, mask)
    e = (0, 3, (10, 5, 67, 40), 0, (0, 0, 0), under, mask)
    return [[a, b, c, d, e], [e, d, c, b, a], [b, a], [a, b]]


def alpha(flip):
    H, W = 12, 36
    rng = np.random.default_rng(17)
    mask = np.zeros((H, W, 3), np.uint8)
    mask[:, :, 0] = np.asarray(ALPHAS, np.uint8)[np.arange(W) % 6][None, :]
    return [(0, 0, (0, 0, W, H), 0, (0, 0, 0), _img(rng, H, W), None), (0, 2, (0, 0, W, H), flip, (0, 0, 0), _img(rng, H, W), mask)]


def wide():
    """3 x 4100: a row longer than the 4096-pixel tile: one row a work-group, two tiles, the second short"""
    W = 4100
    rng = np.random.default_rng(19)
    return [(0, 0, (0, 0, W, 2), 0, (0, 0, 0), _img(rng, 2, W), None), (0, 0, (-3, 1, W + 9, 3), 0, (0, 0, 0), _img(rng, 2, 50), None)]


def cases():
    """[(name, (H, W), pages, layers)]: every table the GPU test composes"""
    out = [("canvas_%dx%d" % (W, H), (H, W), 2, small_canvas(W, H)) for W in WIDTHS for H in HEIGHTS]
    out += [("three_pages", (70, 67), 3, three_pages()), ("no_layers", (70, 67), 2, []), ("edges", (70, 67), 1, edges()), ("wide", (3, 4100), 1, wide())]
    out += [("order_%d" % k, (37, 67), 1, o) for k, o in enumerate(orders())]
    out += [("alpha_%d" % f, (12, 36), 1, alpha(f)) for f in (0, 1)]
    return out


def hostile(src, empty):
    """tables compose_params_ok rejects on a 9 x 20 canvas of one page; src: a 4 x 4 image, empty: one of no rows"""
    good = (0, 0, (0, 0, 4, 4), 0, (0, 0, 0), src, None)
    return [
        [(0, 0, (20, 0, 24, 4), 0, (0, 0, 0), src, None)],              # outside the canvas
        [(0, 0, (3, 3, 3, 8), 0, (0, 0, 0), src, None)],                # empty
        [(0, 0, (0, 0, 4, 4), 0, (0, 0, 0), None, None)],               # kind 0 without a source
        [(0, 2, (0, 0, 4, 4), 0, (0, 0, 0), src, None)],                # kind 2 without a mask
        [(0, 1, (0, 0, 4, 4), 0, (0, 0, 0), None, empty)],              # a mask of no rows
        [(0, 4, (0, 0, 4, 4), 0, (0, 0, 0), src, None)],                # kind 4
        [(0, 0, (0, 0, 4, 4), 2, (0, 0, 0), src, None)],                # polarity 2
        [(1, 0, (0, 0, 4, 4), 0, (0, 0, 0), src, None)],                # page 1 of 1
        [good, (0, 0, (-(1 << 25), 0, 4, 4), 0, (0, 0, 0), src, None)],  # a coordinate beyond 2^24
        [good] * 65,                                                    # 65 layers on one page
    ]
