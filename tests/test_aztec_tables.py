"""CPU: what pins lumina_ocr/utils/aztec.py structurally — the fields, the size and capacity formulas, the placement, the mode ring —
and that the device header is the one these tables write."""
import os

import numpy as np
import pytest

from lumina_ocr.utils import aztec as az


@pytest.mark.parametrize("m", [4, 6, 8, 10, 12])
def test_alpha_has_full_order_and_exp_log_are_inverse(m):
    exp, log = az.gf_tables(m)
    n = (1 << m) - 1
    assert len(exp) == 2 * (n + 1) and len(log) == n + 1
    assert sorted(exp[:n]) == list(range(1, n + 1))                     # x generates every non-zero element: its order is 2^m - 1
    assert all(log[exp[i]] == i for i in range(n)) and all(exp[log[a]] == a for a in range(1, n + 1))
    assert all(exp[i] == exp[i - n] for i in range(n, 2 * (n + 1)))
    assert exp[1] == 2 and exp[m] == az.FIELD_POLY[m] ^ (1 << m)


def test_sizes_and_bits_tabulated():
    assert [az.modules(True, L) for L in range(1, 5)] == [15, 19, 23, 27]
    assert [az.modules(False, L) for L in range(1, 12)] == [19, 23, 27, 31, 37, 41, 45, 49, 53, 57, 61]
    assert az.modules(False, 32) == 151 and az.total_bits(False, 32) == 19968
    assert [az.total_bits(True, L) for L in range(1, 5)] == [104, 240, 408, 608]
    assert [az.total_bits(False, L) for L in range(1, 12)] == [128, 288, 480, 704, 960, 1248, 1568, 1920, 2304, 2720, 3168]
    assert [az.word_width(L) for L in (1, 2, 3, 8, 9, 22, 23, 32)] == [6, 6, 8, 8, 10, 10, 12, 12]
    assert max(az.total_words(c, L) for c, L in az.SYMBOLS) == 316 <= az.MAX_DATA
    assert all(az.modules(c, L) <= 61 for c, L in az.SYMBOLS) and len(az.SYMBOLS) == 15
    # a block is no longer than its field's order
    assert all(az.total_words(c, L) <= (1 << az.word_width(L)) - 1 for c, L in az.SYMBOLS)


@pytest.mark.parametrize("compact,layers", az.SYMBOLS)
def test_placement_visits_every_data_module_once_and_no_function_module(compact, layers):
    n = az.modules(compact, layers)
    fn, dark = az.function_matrix(compact, layers)
    seen = set()
    for b in range(az.total_bits(compact, layers)):
        x, y = az.data_bit_position(compact, layers, b)
        assert 0 <= x < n and 0 <= y < n and not fn[y, x] and (x, y) not in seen, (b, x, y)
        seen.add((x, y))
    assert len(seen) + int(fn.sum()) == n * n
    c, s = n // 2, az.ring_distance(compact)
    # the bullseye: dark at the even distances; the reference grid: alternating along the centre lines, dark at the centre's parity
    assert all(dark[c + dy, c + dx] == (max(abs(dx), abs(dy)) % 2 == 0) for dx in range(-s + 1, s) for dy in range(-s + 1, s))
    if not compact:
        assert all(fn[c, x] and fn[x, c] for x in range(n))
        assert all(dark[c, c + d] == dark[c + d, c] == (d % 2 == 0) for d in range(s + 1, c + 1))
        if c >= 16:                                                     # from 5 layers on: the lines at 16 modules either side
            assert layers >= 5 and all(fn[c + 16, x] and fn[c - 16, x] and fn[x, c + 16] and fn[x, c - 16] for x in range(n))
        else:
            assert layers < 5


@pytest.mark.parametrize("compact", [True, False])
def test_mode_bits_are_distinct_and_on_the_ring(compact):
    s = az.ring_distance(compact)
    pos = az.mode_bit_positions(compact)
    assert len(pos) == len(set(pos)) == (28 if compact else 40)
    assert all(max(abs(x), abs(y)) == s and min(abs(x), abs(y)) < s - 1 for x, y in pos)
    marks = az.orientation_marks(compact)
    assert len(marks) == 12 and not set((x, y) for x, y, _ in marks) & set(pos) and sum(d for _, _, d in marks) == 6
    if not compact:
        assert all(x != 0 and y != 0 for x, y in pos)                  # the centre lines belong to the reference grid
    # no rotation of the marks equals the marks: the orientation is unique
    turned = lambda r: {R_turn(x, y, r): d for x, y, d in marks}
    base = turned(0)
    assert all(turned(r) != base for r in (1, 2, 3))
    # the mode message is a codeword of its code
    import aztec_reference as R
    words = az.mode_words(compact, 3, 17)
    assert R.rs_correct(words, 5 if compact else 6, 4) == (words, 0)


def R_turn(x, y, r):
    for _ in range(r):
        x, y = -y, x
    return x, y


def test_the_device_header_is_the_one_the_tables_write():
    path = os.path.join(os.path.dirname(os.path.abspath(az.__file__)), "..", "..", "csrc", "aztec_tables.h")
    with open(path) as f:
        assert f.read() == az.device_header()


def test_check_words_make_a_codeword():
    import aztec_reference as R
    rng = np.random.RandomState(3)
    for m, nd, ec in ((6, 20, 20), (8, 100, 140), (10, 30, 286)):
        data = [int(v) for v in rng.randint(0, 1 << m, nd)]
        block = data + az.rs_check_words(data, ec, m)
        assert R.rs_correct(block, ec, m) == (block, 0)
