"""Pages for the tests of lumina_ocr_datamatrix_sizes (CPU and GPU): one large symbol a page through lumina_ocr.synth's encoder, the page no
larger than the symbol needs (240 x 256 for 64 x 64 at 3 px a module, 480 x 496 for 144 x 144), and the restatement's answer for a
page, computed once a process and shared."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

from lumina_ocr import synth
from lumina_ocr.utils import datamatrix as dm

import dm_sizes_reference as R2

LARGE = tuple(range(dm.NUM_SIZES, dm.NUM_SIZES_ALL))
SIDES = tuple(dm.ALL_SIZES[s][0] for s in LARGE)
# (side, degrees) at which the restatement read BOTH placements of the sweep recorded in DESIGN.md (3 px a module, placements (32, 24)
# and (37, 29)); the tilt tests assert "reads" at these and equality with the restatement at every angle of the sweep
SWEEP = (0.5, 1.0, 2.0)
PLACEMENTS = ((32, 24), (37, 29))
TILT_READS = ((64, 0.5), (64, 1.0), (104, 0.5), (104, 1.0), (104, 2.0), (144, 0.5), (144, 1.0))


def size_of(side: int) -> int:
    return dm.size_index_all(side, side)


def blank(h: int, w: int) -> np.ndarray:
    return np.full((h, w, 3), 255, np.uint8)


def payload(size: int, tag: str = "") -> str:
    """A text that fills most of the size in ASCII."""
    return (tag + "S%d " % dm.ALL_SIZES[size][0] + "record of a large data matrix / " * 60)[:dm.ALL_SIZES[size][2] - 3]


def page_of(size: int, rotation: int = 0, module: int = 3, text: Optional[str] = None, matrix=None, at: Tuple[int, int] = (32, 24)):
    """-> (page, box, text): the symbol at `at` on a page of (side px + 48) x (side px + 64)."""
    side = dm.ALL_SIZES[size][0] * module
    page = blank(side + 48, side + 64)
    text = payload(size) if text is None else text
    box = synth.draw_dm(page, at[0], at[1], synth.dm_encode(text, size) if matrix is None else matrix, module, rotation)
    return page, box, text


def corrupted(text: str, size: int, block: int, wrong: int) -> np.ndarray:
    """The symbol with `wrong` codewords of one block destroyed: the block's stream positions block + nb (2 i + 1)."""
    cw = synth.dm_interleave(synth.dm_data_codewords(text, size), size)
    nb = dm.ALL_SIZES[size][6]
    for i in range(wrong):
        cw[block + nb * (2 * i + 1)] ^= (0xFF, 0x5A, 0x01, 0x80)[i % 4]
    return synth.dm_matrix(cw, size)


def tilted(page: np.ndarray, degrees: float) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.fromarray(page).rotate(degrees, resample=Image.BICUBIC, fillcolor=(255, 255, 255)))


def tilt_pages(side: int):
    """-> [(degrees, placement, page)] of the sweep, the upright pages (0 degrees) first, and the text."""
    size = size_of(side)
    out = []
    for deg in (0.0,) + SWEEP:
        for at in PLACEMENTS:
            page = page_of(size, rotation=side % 4, at=at)[0]
            out.append((deg, at, tilted(page, deg) if deg else page))
    return out, payload(size)


_SEEN: Dict[tuple, tuple] = {}


def reference(page: np.ndarray, max_size: int = 144, **kw):
    """R2.datamatrix_sizes(page, max_size, **kw), remembered: (mask, codes, data, stage 1's candidates).  Nobody writes to what it returns."""
    key = (page.shape, page.tobytes(), max_size, tuple(sorted(kw.items())))
    if key not in _SEEN:
        _SEEN[key] = R2.datamatrix_sizes(page, max_size, **kw)
    return _SEEN[key]


def found(rc, rd):
    """-> {(x0, y0, x1, y1): text}"""
    return {tuple(int(v) for v in c[:4]): t for c, t in zip(rc, R2.texts(rc, rd))}
