"""Pages for the all-versions QR pass (lumina_ocr_qrcodes_versions), shared by the CPU tests of the restatement
(tests/test_qr_versions_reference.py) and the GPU tests (tests/test_gpu_qrcodes_versions.py).  A page is 560 x 587: the smallest that
holds a version 40 symbol at 3 px a module with its quiet zone, and its width is no multiple of 64."""
import functools

import numpy as np

from lumina_ocr import synth
from lumina_ocr.utils import qrcodes as qr

H, W = 587, 560
# version, level: the first of the new path (one word); across a word, four centres, 3 remainder bits; the new count widths; the third
# word; the alignment exception; the 153-codeword block; 25 and 81 blocks
EIGHT = ((11, 1), (14, 0), (27, 2), (28, 3), (32, 1), (37, 0), (40, 0), (40, 3))


def blank(h: int = H, w: int = W) -> np.ndarray:
    return np.full((h, w, 3), 255, np.uint8)


def text_for(version: int, level: int, tag: str = "") -> str:
    """Byte-mode text that fills the symbol but for a codeword."""
    head = "%sv%d-%s " % (tag, version, qr.LEVELS[level])
    body = "https://lumina.example/e-invoice?jwt=eyJhbGciOiJSUzI1NiJ9."
    n = qr.data_codewords(version, level) - 4
    return (head + body * (n // len(body) + 1))[:n]


@functools.lru_cache(maxsize=None)
def symbol(version: int, level: int, tag: str = ""):
    text = text_for(version, level, tag)
    sym = synth.qr_encode(text, version, level, (version + level) % 8)
    sym.setflags(write=False)
    return text, sym


def put(page, x, y, version, level, module=3, rotation=0, tag="", sym=None):
    """-> (box, text)"""
    text, drawn = symbol(version, level, tag)
    return synth.draw_qr(page, x, y, drawn if sym is None else sym, module, rotation), text


def corrupted(version: int, level: int, block: int, wrong: int, tag: str = ""):
    """The symbol with `wrong` data codewords of one block changed -> (text, modules)."""
    text = text_for(version, level, tag)
    cw = synth.qr_interleave(synth.qr_data_codewords(text, version, level), version, level)
    nb, short, dlen, _ = qr.block_structure(version, level)
    assert wrong <= dlen + (block >= short)
    for i in range(wrong):                                   # the block's data codeword i in the interleaved sequence
        cw[i * nb + block if i < dlen else dlen * nb + block - short] ^= (0xFF, 0x5A, 0x01, 0x80)[i % 4]
    return text, synth.qr_matrix(cw, version, level, (version + level) % 8)


def version_copy_destroyed(version: int, level: int, copies, tag: str = ""):
    """The symbol with six bits of the named version information copies (0 = top right, 1 = bottom left) inverted."""
    text, sym = symbol(version, level, tag)
    sym = sym.copy()
    for i, pos in enumerate(qr.version_positions(version)):
        if i % 3 == 0:
            for c in copies:
                sym[pos[c]] = not sym[pos[c]]
    return text, sym


def tilted(page: np.ndarray, degrees: float) -> np.ndarray:
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.fromarray(page).rotate(degrees, resample=Image.BICUBIC, fillcolor=(255, 255, 255))))
