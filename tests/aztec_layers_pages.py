"""Pages for the tests of lumina_ocr_aztec_layers (CPU and GPU): large full-range symbols on pages just large enough for them, and the
restatement's result of a page, computed once."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from lumina_ocr.utils import aztec as az

import aztec_layers_reference as R2
import aztec_pages as AP

# 12: 67 modules, the first row wider than one 64-bit word; 20: 101, the first with reference lines at +-48; 22: 109 modules and 1020
# words, the last on GF(1024); 23: 113, the first on GF(4096); 27: 131, the first with three-word rows and lines at +-64; 32: the largest
SIZES = (12, 20, 22, 23, 27, 32)
# (layers, degrees): the angles the earlier passes promise after the page's de-skew
TILTS = ((12, 0.5), (12, 1.0), (12, 2.0), (22, 0.5), (22, 1.0), (22, 2.0), (32, 0.5), (32, 1.0))


def payload(layers: int, tag: str = "") -> str:
    return AP.payload(False, layers, tag)


def nearly_full(layers: int) -> str:
    """An upper-case text that leaves the symbol about forty check words: its block corrects about twenty wrong codewords."""
    total, w = az.total_words(False, layers), az.word_width(layers)
    text = ("THE QUICK BROWN FOX JUMPS OVER THE LAZY DOG " * 400)[:(total - 40) * w // 5]
    ec = total - az.symbol_words(text, False, layers)[1]
    assert 24 <= ec <= 64, ec
    return text


def page_of(layers: int, module: int = 3, rotation: int = 0, text: str = None, margin: Tuple[int, int] = (13, 9), matrix=None):
    """-> (page, box, text): one symbol with its top-left pixel at `margin` on a page a little larger than it."""
    text = payload(layers) if text is None else text
    s = AP.side_px(False, layers, module)
    page = AP.blank(s + 2 * margin[1] + 5, s + 2 * margin[0] + 3)
    box = az.draw(page, margin[0], margin[1], az.encode(text, False, layers) if matrix is None else matrix, module, rotation)
    return page, box, text


_SEEN: Dict[tuple, tuple] = {}


def reference(page: np.ndarray, max_layers: int = az.MAX_LAYERS_ALL, **kw):
    """R2.aztec_layers of a page, computed once for every (page, parameters)."""
    key = (page.shape, page.tobytes(), max_layers, tuple(sorted(kw.items())))
    if key not in _SEEN:
        _SEEN[key] = R2.aztec_layers(page, max_layers, **kw)
    return _SEEN[key]
