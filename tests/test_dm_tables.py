"""The tables of the Data Matrix pass (lumina_ocr/utils/datamatrix.py): the size table pinned by modules = 8 (data + check) +
remainder, the placement (every data module once, no function module, the four corner cases, the 2 x 2 remainder corner), the block
lengths, GF(256) / 0x12D, two published vectors, and csrc/dm_tables.h against device_header()."""
from pathlib import Path

from lumina_ocr import synth
from lumina_ocr.utils import datamatrix as dm

# side or (rows, cols) -> (data, check) as the standard's table gives them
SQUARE = {10: (3, 5), 12: (5, 7), 14: (8, 10), 16: (12, 12), 18: (18, 14), 20: (22, 18), 22: (30, 20), 24: (36, 24), 26: (44, 28), 32: (62, 36),
          36: (86, 42), 40: (114, 48), 44: (144, 56), 48: (174, 68), 52: (204, 84)}
RECT = {(8, 18): (5, 7), (8, 32): (10, 11), (12, 26): (16, 14), (12, 36): (22, 18), (16, 36): (32, 24), (16, 48): (49, 28)}


def test_size_table_modules_are_eight_a_codeword_plus_the_remainder():
    assert dm.NUM_SIZES == 21 == len(SQUARE) + len(RECT)
    for s, (rows, cols, nd, ne, nr, nc, nb) in enumerate(dm.SIZES):
        assert (nd, ne) == (SQUARE[rows] if rows == cols else RECT[(rows, cols)])
        assert cols <= 52 and rows % nr == 0 and cols % nc == 0
        assert (nr, nc) == ((2, 2) if rows == cols and rows >= 32 else (1, 2) if rows != cols and cols >= 32 else (1, 1))
        nrow, ncol = dm.mapping_dims(s)
        remainder = 4 if rows == cols and rows in (12, 16, 20, 24) else 0
        assert nrow * ncol == 8 * (nd + ne) + remainder and dm.remainder_modules(s) == remainder, (rows, cols)
        assert dm.size_index(rows, cols) == s
    assert dm.size_index(64, 64) == -1 and dm.size_index(18, 8) == -1
    assert max(s[2] for s in dm.SIZES) <= dm.MAX_DATA and max(s[2] + s[3] for s in dm.SIZES) == dm.MAX_CODEWORDS


def test_placement_visits_every_data_module_once_and_no_function_module():
    for s, (rows, cols, nd, ne, _, _, _) in enumerate(dm.SIZES):
        place, func = dm.placement_of(s), dm.function_modules(s)
        assert len(place) == 8 * (nd + ne) == len(set(place))
        assert not set(place) & set(func)
        fixed = dm.fixed_modules(s)
        rest = set((r, c) for r in range(rows) for c in range(cols)) - set(func) - set(place)
        assert rest == set(rc for rc, _ in fixed) and len(rest) == dm.remainder_modules(s)
        if fixed:                                    # the 2 x 2 corner at the bottom right of the data: dark on its diagonal
            assert sorted(fixed) == [((rows - 3, cols - 3), True), ((rows - 3, cols - 2), False), ((rows - 2, cols - 3), False), ((rows - 2, cols - 2), True)]


def test_each_corner_case_is_used_by_an_in_scope_size():
    used = {(dm.SIZES[s][0], dm.SIZES[s][1]): dm.corner_cases(s) for s in range(dm.NUM_SIZES)}
    assert used[(14, 14)] == [1] and used[(16, 16)] == [2] and used[(8, 32)] == [3] and used[(8, 18)] == [4]
    assert {k for k, v in used.items() if v == [1]} == {(14, 14), (22, 22), (32, 32), (40, 40), (48, 48)}
    assert {k for k, v in used.items() if v == [2]} == {(16, 16), (24, 24)}
    assert {k for k, v in used.items() if v == [3]} == {(8, 32), (16, 48)}
    assert {k for k, v in used.items() if v == [4]} == {(8, 18), (16, 36)}
    assert all(len(v) <= 1 for v in used.values())
    # corner case 1 of 14 x 14 (a 12 x 12 data matrix): three modules at the bottom left, five down the top right
    words, corners, _ = dm.mapping_placement(12, 12)
    assert corners == [1] and [(11, 0), (11, 1), (11, 2), (0, 10), (0, 11), (1, 11), (2, 11), (3, 11)] in words


def test_first_codeword_sits_in_the_top_left_utah_and_regions_step_over_the_bars():
    # the walk starts at (4, 0): codeword 1's eighth bit is there, its first wraps round to the top right
    assert dm.mapping_placement(8, 8)[0][0][-1] == (4, 0) and dm.placement_of(0)[7] == (5, 1)
    assert dm.to_symbol(9, 13, 13) == (14, 14) and dm.to_symbol(9, 14, 14) == (17, 17)      # 32 x 32: 14 x 14 data regions
    assert dm.to_symbol(16, 0, 13) == (1, 14) and dm.to_symbol(16, 0, 14) == (1, 17)        # 8 x 32: two regions side by side


def test_function_masks():
    for s, (rows, cols, _, _, nr, nc, _) in enumerate(dm.SIZES):
        solid, clock, dark = dm.function_masks(s)
        full = (1 << cols) - 1
        assert solid[rows - 1] == full and all(w & 1 for w in solid)                        # the L
        assert clock[0] == full & ~sum(1 << (j * cols // nc) for j in range(nc))            # the top clock track, without the solid columns' heads
        assert dark[0] == clock[0] & 0x5555555555555555                                     # dark on even columns
        assert not (dark[0] >> (cols - 1)) & 1 and (dark[rows - 2] >> (cols - 1)) & 1 == (rows - 2) % 2   # the right track: light at the top corner
        assert all(not (a & b) and not (d & ~b) for a, b, d in zip(solid, clock, dark))
        assert sum(bin(w).count("1") for w in solid) == nr * cols + nc * rows - nr * nc


def test_block_lengths():
    for s in range(dm.NUM_SIZES):
        assert dm.block_lengths(s) == ([(102, 42), (102, 42)] if dm.SIZES[s][0] == 52 else [(dm.SIZES[s][2], dm.SIZES[s][3])])
        assert max(d + e for d, e in dm.block_lengths(s)) <= dm.MAX_BLOCK_LEN and max(e for _, e in dm.block_lengths(s)) <= dm.MAX_EC
    assert dm.block_lengths(13) == [(174, 68)] and (dm.MAX_BLOCK_LEN, dm.MAX_EC) == (242, 68)
    cw = list(range(1, 205))
    out = synth.dm_interleave(cw, 14)
    assert out[:204] == cw and out[204::2] == synth.dm_rs_remainder(cw[0::2], 42) and out[205::2] == synth.dm_rs_remainder(cw[1::2], 42)


def test_gf256_of_0x12d():
    assert dm.GF_EXP[:9] == (1, 2, 4, 8, 16, 32, 64, 128, 0x2D) and dm.GF_EXP[255] == 1 and len(set(dm.GF_EXP[:255])) == 255
    assert all(dm.GF_EXP[dm.GF_LOG[a]] == a for a in range(1, 256)) and dm.GF_EXP[255:510] == dm.GF_EXP[:255]
    assert dm.gf_mul(0, 7) == 0 and dm.gf_mul(2, 128) == 0x2D and all(dm.gf_mul(a, dm.GF_EXP[255 - dm.GF_LOG[a]]) == 1 for a in range(1, 256))
    gen = dm.rs_generator(5)                                 # roots a^1 .. a^5: the generator vanishes there and not at a^0
    ev = lambda x: [v for v in [0] for c in gen for v in [dm.gf_mul(v, x) ^ c]][-1]
    assert gen == [1, 62, 111, 15, 48, 228] and all(ev(dm.GF_EXP[i]) == 0 for i in range(1, 6)) and ev(1) != 0


def test_published_vectors():
    cw = synth.dm_data_codewords("123456", 0)
    assert cw == [142, 164, 186] and synth.dm_rs_remainder(cw, 5) == [114, 25, 5, 88, 102]
    cw = synth.dm_data_codewords("Wikipedia", dm.size_index(16, 16))
    assert cw == [88, 106, 108, 106, 113, 102, 101, 106, 98, 129, 251, 147]                 # two randomised pads behind the first
    assert synth.dm_rs_remainder(cw, 12) == [104, 216, 88, 39, 233, 202, 71, 217, 26, 92, 25, 232]
    assert dm.codewords_text(cw) == ("Wikipedia", None)


def test_device_header_is_current():
    path = Path(__file__).resolve().parent.parent / "ocr-system_amd" / "csrc" / "dm_tables.h"
    assert path.read_text() == dm.device_header()
