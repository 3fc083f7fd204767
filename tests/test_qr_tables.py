"""The QR tables (lumina_ocr/utils/qrcodes.py): built from the standard's rules and pinned structurally and by published vectors;
the device's copy (csrc/qr_tables.h) is the same tables."""
from pathlib import Path

from lumina_ocr import synth
from lumina_ocr.utils import qrcodes as qr

VERSIONS = range(1, 11)
DATA_CODEWORDS = {1: (19, 16, 13, 9), 2: (34, 28, 22, 16), 3: (55, 44, 34, 26), 4: (80, 64, 48, 36), 5: (108, 86, 62, 46),
                  6: (136, 108, 76, 60), 7: (156, 124, 88, 66), 8: (194, 154, 110, 86), 9: (232, 182, 132, 100), 10: (274, 216, 154, 122)}


def test_total_codewords_remainder_bits_and_data_modules():
    assert qr.TOTAL_CODEWORDS == (26, 44, 70, 100, 134, 172, 196, 242, 292, 346)
    assert qr.REMAINDER_BITS == (0, 7, 7, 7, 7, 7, 0, 0, 0, 0)
    for v in VERSIONS:
        d = qr.dimension(v)
        fm = qr.function_mask(v)
        assert d == 17 + 4 * v and len(fm) == d and all(w < (1 << d) for w in fm)
        free = d * d - sum(bin(w).count("1") for w in fm)
        assert free == 8 * qr.TOTAL_CODEWORDS[v - 1] + qr.REMAINDER_BITS[v - 1], v
        place = qr.placement(v)
        assert len(place) == free and len(set(place)) == free                      # every data module once
        assert all(not (fm[r] >> c) & 1 for r, c in place)
        assert place[0] == (d - 1, d - 1) and place[1] == (d - 1, d - 2) and place[2] == (d - 2, d - 1)   # up the right edge, right column first


def test_block_structure():
    for v in VERSIONS:
        for lv in range(4):
            nb, short, dlen, ec = qr.block_structure(v, lv)
            assert 1 <= short <= nb <= qr.MAX_BLOCKS and 2 <= ec <= qr.MAX_EC and dlen + 1 + ec <= qr.MAX_BLOCK_LEN + 1
            assert short * (dlen + ec) + (nb - short) * (dlen + 1 + ec) == qr.TOTAL_CODEWORDS[v - 1]
            assert qr.data_codewords(v, lv) == DATA_CODEWORDS[v][lv] == short * dlen + (nb - short) * (dlen + 1)
    assert max(qr.data_codewords(v, lv) for v in VERSIONS for lv in range(4)) == 274 <= qr.MAX_DATA
    assert max(dlen + (short < nb) + ec for v in VERSIONS for lv in range(4) for nb, short, dlen, ec in [qr.block_structure(v, lv)]) == qr.MAX_BLOCK_LEN


def test_alignment_centres():
    want = {2: (6, 18), 3: (6, 22), 4: (6, 26), 5: (6, 30), 6: (6, 34), 7: (6, 22, 38), 8: (6, 24, 42), 9: (6, 26, 46), 10: (6, 28, 50)}
    assert qr.ALIGNMENT_CENTRES[0] == () and all(qr.ALIGNMENT_CENTRES[v - 1] == c for v, c in want.items())
    f = qr.function_modules(7)
    assert f[(22, 22)] and not f[(21, 22)] and f[(20, 20)] and f[(6, 22)]          # a centre, its light ring, its dark ring; on the timing row
    assert f[(22, 38)] and not f[(22, 37)] and (8, 36) not in f                     # (22, 38) is drawn; (6, 38) would overlap the +x finder


def test_format_and_version_words():
    assert format(qr.format_word(1, 0), "015b") == "101010000010010" and format(qr.format_word(0, 0), "015b") == "111011111000100"
    words = [qr.format_word(lv, m) for lv in range(4) for m in range(8)]
    assert sorted(words) == sorted(qr.FORMAT_WORDS) and len(set(words)) == 32
    assert min(bin(a ^ b).count("1") for i, a in enumerate(words) for b in words[:i]) == 7
    assert all(qr.FORMAT_WORDS[(qr.LEVEL_FORMAT_BITS[lv] << 3) | m] == qr.format_word(lv, m) for lv in range(4) for m in range(8))
    assert format(qr.version_word(7), "018b") == "000111110010010100"
    for v in (7, 10):                                                               # drawn by the encoder, covered by the function mask
        sym, fm, word = synth.qr_encode("7", v, 0, 0), qr.function_mask(v), qr.version_word(v)
        for i, (a, b) in enumerate(qr.version_positions(v)):
            assert bool(sym[a]) == bool(sym[b]) == bool((word >> i) & 1) and (fm[a[0]] >> a[1]) & 1 and (fm[b[0]] >> b[1]) & 1
    assert all(p not in qr.function_modules(6) for ab in qr.version_positions(6) for p in ab if p[0] > 8 or p[1] > 8)


def test_galois_field():
    assert qr.GF_EXP[0] == 1 and qr.GF_EXP[1] == 2 and qr.GF_EXP[8] == 0x1D and qr.GF_EXP[255] == 1 and len(qr.GF_EXP) == 512
    assert sorted(qr.GF_EXP[:255]) == list(range(1, 256)) and all(qr.GF_EXP[qr.GF_LOG[a]] == a for a in range(1, 256))
    assert qr.gf_mul(0x53, 0xCA) == qr.gf_mul(0xCA, 0x53) and qr.gf_mul(2, 0x80) == 0x1D and qr.gf_mul(0, 7) == 0


def test_hello_world_1m():
    cw = synth.qr_data_codewords("HELLO WORLD", 1, 1)
    assert cw == [32, 91, 11, 120, 209, 114, 220, 77, 67, 64, 236, 17, 236, 17, 236, 17]
    assert synth.qr_rs_remainder(cw, 10) == [196, 35, 39, 119, 235, 215, 231, 226, 93, 23]
    assert qr.codewords_text(1, cw) == ("HELLO WORLD", None)


def test_the_device_header_is_the_tables():
    header = Path(__file__).resolve().parent.parent / "ocr-system_amd" / "csrc" / "qr_tables.h"
    assert header.read_text() == qr.device_header()
