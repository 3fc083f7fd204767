"""CPU: the geometry, the field and the encoder of lumina_ocr/utils/aztec.py for full-range symbols of 12 .. 32 layers, pinned
structurally as tests/test_aztec_tables.py pins the small sizes, and the generated header of the 12-bit field."""
from pathlib import Path

import numpy as np
import pytest

from lumina_ocr.utils import aztec as az

ROOT = Path(__file__).resolve().parents[1]
LARGE = [L for c, L in az.ALL_SYMBOLS if L > az.MAX_FULL_LAYERS]


def test_the_sizes_in_and_out_of_the_old_scope():
    assert az.SYMBOLS == az.ALL_SYMBOLS[:15] and len(az.SYMBOLS) == 15 and az.MAX_DATA == 320 and az.MAX_FULL_LAYERS == 11
    assert LARGE == list(range(12, 33)) and az.MAX_LAYERS_ALL == 32 and az.MAX_DATA_ALL == 1664 == az.total_words(False, 32)
    assert [az.modules(False, L) for L in (12, 20, 22, 23, 27, 32)] == [67, 101, 109, 113, 131, 151]
    assert [az.word_width(L) for L in (12, 22, 23, 32)] == [10, 10, 12, 12] and az.total_words(False, 22) == 1020


@pytest.mark.parametrize("layers", LARGE)
def test_placement_visits_every_data_module_once_and_no_function_module(layers):
    n = az.modules(False, layers)
    fn, _ = az.function_matrix(False, layers)
    seen = set()
    for b in range(az.total_bits(False, layers)):
        x, y = az.data_bit_position(False, layers, b)
        assert 0 <= x < n and 0 <= y < n and not fn[y, x] and (x, y) not in seen
        seen.add((x, y))
    assert len(seen) + int(fn.sum()) == n * n
    assert az.total_words(False, layers) <= (1 << az.word_width(layers)) - 1


@pytest.mark.parametrize("layers", LARGE)
def test_reference_lines_lie_at_every_multiple_of_16_within_reach(layers):
    n = az.modules(False, layers)
    c = n // 2
    fn, dark = az.function_matrix(False, layers)
    outside = np.maximum(*np.abs(np.mgrid[0:n, 0:n] - c)) > az.ring_distance(False)
    for i in range(n):
        on_line = (i - c) % 16 == 0
        assert bool(fn[i][outside[i]].all()) == on_line and bool(fn[:, i][outside[:, i]].all()) == on_line
        if on_line:
            assert all(bool(dark[i, x]) == ((x - c) % 2 == 0 or (x - c) % 16 == 0) for x in range(n) if outside[i, x])
    assert sorted({abs(i - c) for i in range(n) if (i - c) % 16 == 0}) == list(range(0, c + 1, 16))


def test_the_12_bit_field_and_its_header():
    exp, log = az._TABLES[12]
    assert (exp, log) == az.gf_tables(12) and sorted(exp[:4095]) == list(range(1, 4096)) and len(exp) == 8192 and len(log) == 4096
    assert (ROOT / "ocr-system_amd" / "csrc" / "aztec_tables12.h").read_text() == az.device_header12()
    assert (ROOT / "ocr-system_amd" / "csrc" / "aztec_tables.h").read_text() == az.device_header()


@pytest.mark.parametrize("m,nd,ec", [(12, 50, 30), (12, 1, 2), (10, 40, 21), (4, 4, 6)])
def test_check_words_make_a_codeword(m, nd, ec):
    """every root a^1 .. a^ec of the generator is a root of data + check words"""
    rng = np.random.RandomState(m * 100 + ec)
    data = [int(v) for v in rng.randint(0, 1 << m, nd)]
    block = data + az.rs_check_words(data, ec, m)
    exp, _ = az._TABLES[m]
    assert len(block) == nd + ec and all(0 <= v < (1 << m) for v in block)
    for k in range(1, ec + 1):
        y = 0
        for v in block:
            y = az.gf_mul(m, y, exp[k]) ^ v
        assert y == 0
    block[3 % len(block)] ^= 1
    assert any(__import__("functools").reduce(lambda y, v: az.gf_mul(m, y, exp[k]) ^ v, block, 0) for k in range(1, ec + 1))


def test_stuffing_and_the_character_decoder_work_at_12_bits():
    text = "Wide words, 12 bits: 0123456789 and \xe9\xfc."
    bits = az.content_bits(text)
    words = az.stuff_bits(bits + [0] * 30 + [1] * 30, 12)
    assert all(0 < w < 4095 for w in words) and az.unstuff_words(words, 12)[:len(bits)] == bits
    assert az.codewords_text(az.stuff_bits(bits, 12), 12) == (text, None, False)
