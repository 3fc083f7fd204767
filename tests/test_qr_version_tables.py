"""The QR tables of all 40 versions (lumina_ocr/utils/qrcodes.py, the *_ALL names): the block table is typed from memory of the
standard, so everything that can pin it without the standard is asserted here; csrc/qr_version_tables.h is the same tables; the
ten-version names still give their old answers."""
from pathlib import Path

from lumina_ocr import synth
from lumina_ocr.utils import qrcodes as qr

import test_qr_tables as old

ALL = range(1, 41)
DATA_CODEWORDS = {(11, 0): 324, (15, 2): 295, (20, 0): 861, (25, 1): 1000, (30, 3): 745, (40, 0): 2956, (40, 1): 2334, (40, 2): 1666, (40, 3): 1276}


def test_the_first_ten_columns_are_the_old_tables_and_the_old_names_are_unchanged():
    assert (qr.MIN_VERSION, qr.MAX_VERSION, qr.MAX_DATA, qr.MAX_CODEWORDS, qr.MAX_BLOCKS, qr.MAX_BLOCK_LEN, qr.MAX_EC) == (1, 10, 288, 346, 8, 146, 30)
    assert qr.TOTAL_CODEWORDS_ALL[:10] == qr.TOTAL_CODEWORDS and qr.REMAINDER_BITS_ALL[:10] == qr.REMAINDER_BITS
    assert qr.ALIGNMENT_CENTRES_ALL[:10] == qr.ALIGNMENT_CENTRES
    assert all(qr.EC_PER_BLOCK_ALL[lv][:10] == qr.EC_PER_BLOCK[lv] and qr.NUM_BLOCKS_ALL[lv][:10] == qr.NUM_BLOCKS[lv] for lv in range(4))
    assert all(len(t) == 40 for t in (qr.TOTAL_CODEWORDS_ALL, qr.REMAINDER_BITS_ALL, qr.ALIGNMENT_CENTRES_ALL) + qr.EC_PER_BLOCK_ALL + qr.NUM_BLOCKS_ALL)
    assert set(qr._PLACEMENT) == set(qr._FUNCTION) == set(range(1, 11))
    for v in old.VERSIONS:
        assert tuple(qr.data_codewords(v, lv) for lv in range(4)) == old.DATA_CODEWORDS[v]
        assert qr.placement_of(v) == tuple(qr.placement(v)) and qr.function_mask_of(v) == tuple(qr.function_mask(v))
        assert [qr.count_bits(m, v) for m in (1, 2, 4)] == ([10, 9, 8] if v <= 9 else [12, 11, 16])


def test_totals_remainders_and_alignment_centres_are_pinned_by_the_module_count():
    assert qr.TOTAL_CODEWORDS_ALL[:1] + qr.TOTAL_CODEWORDS_ALL[10:14] + qr.TOTAL_CODEWORDS_ALL[-2:] == (26, 404, 466, 532, 581, 3532, 3706)
    assert qr.TOTAL_CODEWORDS_ALL[14] == 655
    for v in ALL:
        d, fm, cs = qr.dimension(v), qr.function_mask(v), qr.ALIGNMENT_CENTRES_ALL[v - 1]
        assert d * d - sum(bin(w).count("1") for w in fm) == 8 * qr.TOTAL_CODEWORDS_ALL[v - 1] + qr.REMAINDER_BITS_ALL[v - 1], v
        assert qr.REMAINDER_BITS_ALL[v - 1] in (0, 3, 4, 7)
        if v > 1:
            steps = {b - a for a, b in zip(cs[1:], cs[2:])}
            assert len(cs) == v // 7 + 2 <= qr.MAX_ALIGNMENT and cs[0] == 6 and cs[-1] == 4 * v + 10 and len(steps) <= 1
            assert all(s % 2 == 0 for s in steps)                                           # one even step back from the last
    assert qr.ALIGNMENT_CENTRES_ALL[31] == (6, 34, 60, 86, 112, 138) and qr.ALIGNMENT_CENTRES_ALL[39] == (6, 30, 58, 86, 114, 142, 170)
    assert qr.ALIGNMENT_CENTRES_ALL[13] == (6, 26, 46, 66) and qr.ALIGNMENT_CENTRES_ALL[35] == (6, 24, 50, 76, 102, 128, 154)
    assert max(qr.TOTAL_CODEWORDS_ALL) == qr.MAX_CODEWORDS_ALL == 3706


def test_block_table():
    longest = {}
    for v in ALL:
        for lv in range(4):
            nb, short, dlen, ec = qr.block_structure(v, lv)
            assert 1 <= short <= nb <= qr.MAX_BLOCKS_ALL and 7 <= ec <= qr.MAX_EC and dlen >= 9
            assert short * (dlen + ec) + (nb - short) * (dlen + 1 + ec) == qr.TOTAL_CODEWORDS_ALL[v - 1]
            assert qr.data_codewords(v, lv) == short * dlen + (nb - short) * (dlen + 1)
            longest[(v, lv)] = dlen + (short < nb) + ec
            assert lv == 0 or qr.data_codewords(v, lv) < qr.data_codewords(v, lv - 1)            # falls with the level
            assert v == 1 or qr.data_codewords(v, lv) > qr.data_codewords(v - 1, lv)              # rises with the version
    assert all(qr.data_codewords(v, lv) == n for (v, lv), n in DATA_CODEWORDS.items())
    assert max(longest.values()) == longest[(37, 0)] == qr.MAX_BLOCK_LEN_ALL == 153
    assert qr.block_structure(40, 3)[0] == 81 == qr.MAX_BLOCKS_ALL and qr.block_structure(40, 0)[0] == 25
    assert max(qr.data_codewords(v, lv) for v in ALL for lv in range(4)) == qr.MAX_DATA_ALL == 2956


def test_version_words_count_bits_and_confidence():
    assert format(qr.version_word(7), "018b") == "000111110010010100" and qr.version_word(40) == 0x28C69
    assert qr.VERSION_WORDS == tuple(qr.version_word(v) for v in range(7, 41)) and len(set(qr.VERSION_WORDS)) == 34
    assert min(bin(a ^ b).count("1") for i, a in enumerate(qr.VERSION_WORDS) for b in qr.VERSION_WORDS[:i]) == 8
    assert [[qr.count_bits(m, v) for m in (1, 2, 4)] for v in (11, 26, 27, 40)] == [[12, 11, 16]] * 2 + [[14, 13, 16]] * 2
    assert qr.confidence(40, 3, 0) == 1.0 and qr.confidence(40, 3, 81 * 15) == 0.0 and qr.capacity_errors(25, 1) == 21 * 14
    for v in (14, 32, 40):                                                          # drawn by the encoder, covered by the function mask
        sym, fm, word = synth.qr_encode("7", v, 0, 0), qr.function_mask_of(v), qr.version_word(v)
        for i, (a, b) in enumerate(qr.version_positions(v)):
            assert bool(sym[a]) == bool(sym[b]) == bool((word >> i) & 1) and (fm[a[0]] >> a[1]) & 1 and (fm[b[0]] >> b[1]) & 1


def test_the_device_header_is_the_tables():
    header = Path(__file__).resolve().parent.parent / "ocr-system_amd" / "csrc" / "qr_version_tables.h"
    assert header.read_text() == qr.device_header_versions()
    assert (header.parent / "qr_tables.h").read_text() == qr.device_header()
    assert "QRV_PLACE" not in header.read_text() and header.stat().st_size < 8192      # no placement table


def test_read_qrcodes_takes_large_versions_and_byte_rows():
    import numpy as np
    text = "e-invoice " * 60
    cw = synth.qr_data_codewords(text, 25, 1)
    data = np.zeros((2, qr.MAX_DATA_ALL), np.uint8)
    data[0, :len(cw)] = cw
    small = synth.qr_data_codewords("SMALL", 2, 1)
    data[1, :len(small)] = small
    codes = np.array([[10, 20, 360, 370, 25, 1, 2, len(cw), 3, 0, 0, 0], [400, 20, 474, 94, 2, 1, 0, len(small), 0, 1, 0, 0]], np.int32)
    got = qr.read_qrcodes(codes, data)
    assert [e["content"] for e in got] == [text, "SMALL"] and got[0]["version"] == 25 and got[0]["confidence"] == 1.0 - 3 / (21 * 14.0)
    assert qr.read_qrcodes(np.array([[0, 0, 9, 9, 41, 1, 0, 100, 0, 0, 0, 0]], np.int32), data[:1]) == []
    assert qr.read_qrcodes(np.array([[0, 0, 9, 9, 25, 1, 0, 2957, 0, 0, 0, 0]], np.int32), data[:1]) == []     # more than a row holds
