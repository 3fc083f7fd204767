"""Pages for the Aztec tests (CPU and GPU): symbols through lumina_ocr.utils.aztec's encoder, damaged symbols, tilted pages, decoys."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from lumina_ocr import synth
from lumina_ocr.utils import aztec as az

# the smallest and the largest symbol of every codeword width
WIDTH_ENDS = ((True, 1), (False, 2), (True, 3), (False, 8), (False, 9), (False, 11))
# tilt (degrees) each symbol is tested at, at 3 px a module: measured on the restatement, which reads every size at these tilts at
# both of two placements (and most sizes half a degree further)
TILTS = {(True, 4): (0.5, 1.0, 2.0), (False, 4): (0.5, 1.0, 2.0), (False, 8): (2.0,), (False, 11): (1.5,)}


def blank(h: int, w: int) -> np.ndarray:
    return np.full((h, w, 3), 255, np.uint8)


def payload(compact: bool, layers: int, tag: str = "") -> str:
    """A text of mixed modes that fills about three quarters of the symbol's codewords."""
    text = (tag + "Az %d%s " % (layers, "c" if compact else "f") + "Hello, World. 12345 ") * 40
    cap = (az.total_words(compact, layers) * 3 // 4) * az.word_width(layers) // 6
    return text[:max(3, min(cap - 4, 30 * layers))]


def put(page, x, y, text, compact, layers, module=3, rotation=0, matrix=None) -> Tuple[int, int, int, int]:
    return az.draw(page, x, y, az.encode(text, compact, layers) if matrix is None else matrix, module, rotation)


def side_px(compact: bool, layers: int, module: int = 3) -> int:
    return az.modules(compact, layers) * module


def corrupted(text, compact: bool, layers: int, wrong: int, seed: int = 0) -> np.ndarray:
    """The symbol with `wrong` of its codewords destroyed (seeded places and values)."""
    words, nd = az.symbol_words(text, compact, layers)
    rng = np.random.RandomState(1000 * layers + 17 * wrong + seed + (500 if compact else 0))
    w = az.word_width(layers)
    for i in rng.permutation(len(words))[:wrong]:
        words[i] ^= int(rng.randint(1, 1 << w))
    return az.matrix_of_words(compact, layers, words, nd)


def capacity(compact: bool, layers: int, text: str) -> int:
    """Codeword errors the symbol of this text corrects."""
    words, nd = az.symbol_words(text, compact, layers)
    return (len(words) - nd) // 2


def tilted(page: np.ndarray, degrees: float) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.fromarray(page).rotate(degrees, resample=Image.BICUBIC, fillcolor=(255, 255, 255)))


def bullseye(page, x, y, rings: int, module: int) -> None:
    """Concentric squares, dark at the even distances up to `rings`, top-left pixel at (x, y)."""
    n = 2 * rings + 1
    m = np.array([[max(abs(r - rings), abs(c - rings)) % 2 == 0 for c in range(n)] for r in range(n)])
    az.draw(page, x, y, m, module)


def decoys(h: int = 150, w: int = 330) -> Tuple[np.ndarray, List[str]]:
    """What looks like a bullseye and is no symbol: selected radio buttons, QR finders, nested squares of other ratios, a compact and a
    full bullseye alone, a symbol whose quiet ring is dirty."""
    page = blank(h, w)
    kinds = []
    yy, xx = np.mgrid[0:h, 0:w]
    for i, r in enumerate((9, 14)):                                       # selected radio buttons: a disc in a circle
        cx, cy = 20 + 40 * i, 20
        d2 = (xx - cx) ** 2 + (yy - cy) ** 2
        page[(d2 <= (r // 3) ** 2) | ((d2 <= r * r) & (d2 >= (r - 2) ** 2))] = 0
        kinds.append("radio")
    synth.qr_finder(page, 100, 8, 3)
    synth.qr_finder(page, 140, 8, 5)
    kinds += ["qr_finder"] * 2
    for i, (core, gap, ring) in enumerate(((3, 6, 3), (9, 3, 3), (4, 2, 8))):   # nested squares: core, clear gap, ring thickness
        side = core + 2 * (gap + ring)
        x, y = 200 + 40 * i, 8
        page[y:y + side, x:x + side] = 0
        page[y + ring:y + side - ring, x + ring:x + side - ring] = 255
        page[y + ring + gap:y + ring + gap + core, x + ring + gap:x + ring + gap + core] = 0
        kinds.append("nested")
    bullseye(page, 10, 70, 4, 3)
    bullseye(page, 60, 70, 6, 3)
    bullseye(page, 120, 70, 2, 4)
    kinds += ["bullseye"] * 3
    box = put(page, 200, 70, "DIRTY QUIET RING", True, 2)
    page[box[1] + 10:box[1] + 16, box[2] + 2:box[2] + 4] = 0                   # ink one module off the right side
    kinds.append("dirty")
    return page, kinds
