"""The definition of lumina_ocr_page_compose (include/lumina_ocr.h, csrc/compose.h) restated in numpy, and compose_params_ok's twin.

A layer is the tuple Engine.page_compose takes: (page, kind, (x0, y0, x1, y1), flip, (r, g, b), src, mask) with src / mask uint8
[h][w][3] arrays (None where the kind has none).  compose() paints whole rectangles at a time with integer arrays; the per-pixel
formula in plain Python integers is compose_pixel(), which the tests hold against it."""
import numpy as np

MAX_LAYERS = 64
MAX_SIDE = 65535
MAX_COORD = 1 << 24


def sample_map(d, span: int, w: int):
    """the sample that holds the centre of pixel d (an int or an int64 array) of a span of `span` pixels showing w samples"""
    return ((2 * d + 1) * w) // (2 * span)


def div255(t):
    return (t + 128 + ((t + 128) >> 8)) >> 8


def compose_params_ok(layers, n: int, height: int, width: int) -> bool:
    """what csrc/compose.h compose_params_ok accepts (pointers: an array of the right shape stands for a non-null one)"""
    if n < 0 or not (0 < height <= MAX_SIDE and 0 < width <= MAX_SIDE):
        return False
    page, on_page = -1, 0
    for (pg, kind, (x0, y0, x1, y1), flip, fill, src, mask) in layers:
        if not 0 <= pg < n or pg < page:
            return False
        on_page = on_page + 1 if pg == page else 1
        page = pg
        if on_page > MAX_LAYERS or kind not in (0, 1, 2, 3) or flip not in (0, 1) or not all(0 <= int(v) <= 255 for v in fill):
            return False
        if any(abs(int(v)) > MAX_COORD for v in (x0, y0, x1, y1)) or x0 >= x1 or y0 >= y1:
            return False
        if x0 >= width or x1 <= 0 or y0 >= height or y1 <= 0:
            return False
        for need, img in ((kind != 1, src), (kind != 0, mask)):
            if need and (img is None or img.ndim != 3 or img.shape[2] != 3 or not (0 < img.shape[0] <= MAX_SIDE and 0 < img.shape[1] <= MAX_SIDE)):
                return False
    return True


def compose_pixel(c, layer, x: int, y: int):
    """layer painted onto pixel (x, y) whose colour so far is c = (r, g, b): Python integers only"""
    _, kind, (x0, y0, x1, y1), flip, fill, src, mask = layer
    if not (x0 <= x < x1 and y0 <= y < y1):
        return c
    m = 0
    if kind != 0:
        mh, mw = mask.shape[:2]
        m = int(mask[((2 * (y - y0) + 1) * mh) // (2 * (y1 - y0)), ((2 * (x - x0) + 1) * mw) // (2 * (x1 - x0)), 0])
        if flip:
            m = 255 - m
        if kind == 1:
            return tuple(int(v) for v in fill) if m < 128 else c
        if kind == 3 and m >= 128:
            return c
    h, w = src.shape[:2]
    s = [int(v) for v in src[((2 * (y - y0) + 1) * h) // (2 * (y1 - y0)), ((2 * (x - x0) + 1) * w) // (2 * (x1 - x0))]]
    if kind != 2:
        return tuple(s)
    return tuple((s[k] * m + c[k] * (255 - m) + 128 + ((s[k] * m + c[k] * (255 - m) + 128) >> 8)) >> 8 for k in range(3))


def compose(canvas_hw, n: int, layers) -> np.ndarray:
    """-> uint8 [n][H][W][3]: every page white, then its layers in the order given"""
    height, width = canvas_hw
    assert compose_params_ok(layers, n, height, width)
    out = np.full((n, height, width, 3), 255, np.uint8)
    for (pg, kind, (x0, y0, x1, y1), flip, fill, src, mask) in layers:
        cx0, cx1, cy0, cy1 = max(x0, 0), min(x1, width), max(y0, 0), min(y1, height)
        xs, ys = np.arange(cx0, cx1, dtype=np.int64) - x0, np.arange(cy0, cy1, dtype=np.int64) - y0
        dst = out[pg, cy0:cy1, cx0:cx1]
        m = None
        if kind != 0:
            mh, mw = mask.shape[:2]
            m = mask[sample_map(ys, y1 - y0, mh)[:, None], sample_map(xs, x1 - x0, mw)[None, :], 0].astype(np.int64)
            if flip:
                m = 255 - m
        if kind == 1:
            dst[m < 128] = np.asarray(fill, np.uint8)
            continue
        h, w = src.shape[:2]
        s = src[sample_map(ys, y1 - y0, h)[:, None], sample_map(xs, x1 - x0, w)[None, :]]
        if kind == 0:
            dst[...] = s
        elif kind == 3:
            dst[m < 128] = s[m < 128]
        else:
            a = m[:, :, None]
            dst[...] = div255(s.astype(np.int64) * a + dst.astype(np.int64) * (255 - a)).astype(np.uint8)
    return out
