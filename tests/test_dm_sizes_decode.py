"""CPU: the host half on what only large Data Matrix symbols produce: Base 256 fields with the two-byte length, the 255- and 253-state
un-randomising at positions past 255, C40 runs over a thousand codewords, and capacity and confidence summed over up to ten blocks."""
import numpy as np

from lumina_ocr import synth
from lumina_ocr.utils import datamatrix as dm


def row(size: int, cw, errors: int = 0):
    rows, cols, nd = dm.ALL_SIZES[size][:3]
    data = np.zeros((1, dm.MAX_DATA_ALL), np.uint8)
    data[0, :nd] = cw
    return np.array([[5, 6, 5 + 3 * cols - 1, 6 + 3 * rows - 1, rows, cols, nd, errors, 0, 0, 0, 0]], np.int32), data


def test_base256_of_1000_bytes_has_the_two_byte_length():
    raw = bytes((37 * i + i // 256) % 256 for i in range(1000))
    size = synth.dm_smallest_size(raw, "base256", large=True)
    assert dm.ALL_SIZES[size][:3] == (120, 120, 1050)
    cw = synth.dm_data_codewords(raw, size, "base256")
    assert cw[0] == dm.LATCH_BASE256 and dm.unrandomise_255(cw[1], 2) == 249 + 4 and dm.unrandomise_255(cw[2], 3) == 0 and 250 * (253 - 249) + 0 == 1000
    assert [dm.unrandomise_255(v, i + 4) for i, v in enumerate(cw[3:1003])] == list(raw)
    assert cw[1003] == dm.PAD and cw[1004:] == [dm.randomised_pad(p + 1) for p in range(1004, 1050)]
    e, = dm.read_datamatrix(*row(size, cw))
    assert e["content"].encode("iso-8859-1") == raw or e["content"].encode("utf-8") == raw
    assert (e["rows"], e["cols"], e["confidence"], e["kind"]) == (120, 120, 1.0, "DataMatrix")
    # the field that fills the symbol: length 0, "to the end"
    full = bytes(65 + i % 26 for i in range(1556))
    cw = synth.dm_data_codewords(full, 29, "base256")
    assert len(cw) == 1558 and dm.unrandomise_255(cw[1], 2) == 0
    assert dm.read_datamatrix(*row(29, cw))[0]["content"] == full.decode()
    # a length of 250 .. 1555 in a 144 x 144 symbol, pads behind it at positions past 255 and 1500
    part = bytes(48 + i % 10 for i in range(1499))
    cw = synth.dm_data_codewords(part, 29, "base256")
    assert cw[1502] == dm.PAD and all(130 <= v <= 254 or 1 <= v <= 128 for v in cw[1503:])
    assert dm.read_datamatrix(*row(29, cw))[0]["content"] == part.decode()


def test_c40_filling_132():
    nd = dm.ALL_SIZES[28][2]
    text = ("INVOICE 2024 LINE %04d " * 200 % tuple(range(200)))[:3 * ((nd - 2) // 2)]
    assert len(text) == 1953 and nd == 1304                                  # the latch, 651 pairs of codewords, the unlatch: no pad
    cw = synth.dm_data_codewords(text, 28, "c40")
    assert len(cw) == nd and cw[0] == dm.LATCH_C40 and cw[-1] == dm.UNLATCH
    assert dm.codewords_text(cw) == (text, None)
    e, = dm.read_datamatrix(*row(28, cw, 31))
    assert e["content"] == text and e["errors"] == 31 and e["confidence"] == 1.0 - 31 / 248.0 and dm.capacity_errors(28) == 8 * 31
    for scheme, sample in (("text", "invoice 2024 line %04d "), ("x12", "SEG*%04d>")):
        t = (sample * 200 % tuple(range(200)))[:1500]
        cw = synth.dm_data_codewords(t, 28, scheme)
        assert dm.codewords_text(cw) == (t, None)


def test_rows_of_both_widths_and_unknown_sizes():
    cw = synth.dm_data_codewords("SMALL", 3)
    codes = np.array([[0, 0, 47, 47, 16, 16, 12, 0, 0, 0, 0, 0]], np.int32)
    wide, narrow = np.zeros((1, dm.MAX_DATA_ALL), np.uint8), np.zeros((1, dm.MAX_DATA), np.int32)
    wide[0, :12], narrow[0, :12] = cw, cw
    assert dm.read_datamatrix(codes, wide) == dm.read_datamatrix(codes, narrow) and dm.read_datamatrix(codes, wide)[0]["content"] == "SMALL"
    bad = codes.copy()
    bad[0, 4:6] = 60
    assert dm.read_datamatrix(bad, wide) == []
    c, d = row(21, synth.dm_data_codewords("x", 21))
    c[0, 6] -= 1
    assert dm.read_datamatrix(c, d) == []
