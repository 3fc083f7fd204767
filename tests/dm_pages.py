"""Pages for the Data Matrix tests (CPU and GPU): symbols through lumina_ocr.synth's encoder, damaged symbols.  Pages are 200 x 243
unless a size is given: the smallest that hold a 52 x 52 symbol at 3 px a module with its quiet zone; W is no multiple of 64."""
from __future__ import annotations

import numpy as np

from lumina_ocr import synth
from lumina_ocr.utils import datamatrix as dm

H, W = 200, 243


def blank(h: int = H, w: int = W) -> np.ndarray:
    return np.full((h, w, 3), 255, np.uint8)


def put(page, x, y, text, size, module=3, rotation=0, scheme="ascii", sym=None):
    return synth.draw_dm(page, x, y, synth.dm_encode(text, size, scheme) if sym is None else sym, module, rotation)


def payload(size: int, tag: str = "") -> str:
    """A text that fills most of the size in ASCII (digits pair up, so the tail is letters)."""
    return (tag + "S%d " % size + "data matrix / " * 20)[:max(1, dm.SIZES[size][2] - 1)]


def corrupted(text, size, wrong):
    """The symbol with `wrong` codewords of every block destroyed."""
    cw = synth.dm_interleave(synth.dm_data_codewords(text, size), size)
    nb = dm.SIZES[size][6]
    for b in range(nb):
        for i in range(wrong):
            cw[(2 * i + 1) * nb + b] ^= (0xFF, 0x5A, 0x01, 0x80)[i % 4]
    return synth.dm_matrix(cw, size)
