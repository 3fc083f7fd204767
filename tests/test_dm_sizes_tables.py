"""CPU: the tables of the nine large Data Matrix sizes (64 x 64 .. 144 x 144).  The size rows and the interleave of 144 x 144 are written
from recollection of the standard; what pins them here is structural: data + check = mapping area / 8, every mapping module placed
once, the block lengths, the stream-position rule, and the project's own encoder against its own decoder."""
from pathlib import Path

from lumina_ocr import synth
from lumina_ocr.utils import datamatrix as dm

import dm_reference as R1

ROOT = Path(__file__).resolve().parents[1]
LARGE = range(dm.NUM_SIZES, dm.NUM_SIZES_ALL)
# side: (data, check, regions a side, blocks, (data, check) of the first block)
TABLE = {64: (280, 112, 4, 2, (140, 56)), 72: (368, 144, 4, 4, (92, 36)), 80: (456, 192, 4, 4, (114, 48)), 88: (576, 224, 4, 4, (144, 56)),
         96: (696, 272, 4, 4, (174, 68)), 104: (816, 336, 4, 6, (136, 56)), 120: (1050, 408, 6, 6, (175, 68)), 132: (1304, 496, 6, 8, (163, 62)),
         144: (1558, 620, 6, 10, (156, 62))}


def test_the_small_tables_stand_and_the_view_starts_with_them():
    assert dm.ALL_SIZES[:dm.NUM_SIZES] == dm.SIZES and dm.NUM_SIZES == 21 and dm.MAX_DATA == 208
    assert dm.ALL_SIZES[dm.NUM_SIZES:] == dm.LARGE_SIZES and len(dm.LARGE_SIZES) == 9 and dm.NUM_SIZES_ALL == 30
    assert dm.MAX_DATA_ALL == 1560 >= max(s[2] for s in dm.ALL_SIZES) and dm.MAX_CODEWORDS_ALL == max(s[2] + s[3] for s in dm.ALL_SIZES) == 2178
    assert dm.size_index(64, 64) == -1 and dm.size_index_all(64, 64) == 21 and dm.size_index_all(144, 144) == 29 and dm.size_index_all(10, 10) == 0
    assert (ROOT / "ocr-system_amd" / "csrc" / "dm_tables.h").read_text() == dm.device_header()


def test_size_rows():
    assert [s[0] for s in dm.LARGE_SIZES] == sorted(TABLE)
    for s in LARGE:
        rows, cols, nd, ne, nr, nc, nb = dm.ALL_SIZES[s]
        assert rows == cols and (nd, ne, nr, nb) == TABLE[rows][:4] and nr == nc
        assert rows % nr == 0 and cols % nc == 0 and (rows // nr) % 2 == 0
        mr, mc = dm.mapping_dims(s)
        assert (mr, mc) == (rows - 2 * nr, cols - 2 * nc) and mr * mc == 8 * (nd + ne) and dm.remainder_modules(s) == 0
        assert ne % nb == 0 and dm.fixed_modules(s) == []


def test_block_lengths_and_the_rs_instantiation_covers_them():
    for s in LARGE:
        rows, _, nd, ne, _, _, nb = dm.ALL_SIZES[s]
        bl = dm.block_lengths(s)
        assert len(bl) == nb <= dm.MAX_BLOCKS_ALL and bl[0] == TABLE[rows][4] and sum(d for d, _ in bl) == nd and sum(e for _, e in bl) == ne
        assert max(d + e for d, e in bl) <= dm.MAX_BLOCK_LEN_ALL <= 255 and max(e for _, e in bl) <= dm.MAX_EC
        if rows != 144:
            assert len(set(bl)) == 1
    assert dm.block_lengths(27) == [(175, 68)] * 6 and dm.MAX_BLOCK_LEN_ALL == 243
    assert dm.block_lengths(29) == [(156, 62)] * 8 + [(155, 62)] * 2
    assert dm.capacity_errors(29) == 310 and dm.capacity_errors(21) == 56 and dm.confidence(29, 31) == 0.9


def test_every_mapping_module_is_placed_once_and_no_function_module():
    for s in LARGE:
        rows, cols, nd, ne, _, _, _ = dm.ALL_SIZES[s]
        place, function = dm.placement_of(s), dm.function_modules(s)
        assert len(place) == 8 * (nd + ne) == len(set(place)) and len(place) + len(function) == rows * cols
        assert not set(place) & set(function) and all(0 <= r < rows and 0 <= c < cols for r, c in place)
        solid, clock, dark = dm.function_masks(s)
        assert sum(bin(a | b).count("1") for a, b in zip(solid, clock)) == len(function) and not any(a & b for a, b in zip(solid, clock))
        assert all(d & ~c == 0 for d, c in zip(dark, clock))


def test_144_is_dealt_by_stream_position():
    s = 29
    _, _, nd, ne, _, _, nb = dm.ALL_SIZES[s]
    data = [(37 * p + 11) % 256 for p in range(nd)]
    stream = synth.dm_interleave(data, s)
    assert len(stream) == nd + ne and stream[:nd] == data
    blocks = [stream[b::nb] for b in range(nb)]                               # the block of position p is p mod 10
    for b, (d, e) in enumerate(dm.block_lengths(s)):
        assert len(blocks[b]) == d + e and blocks[b][:d] == data[b::nb]
        assert blocks[b][d:] == synth.dm_rs_remainder(data[b::nb], e) and R1.rs_correct(blocks[b], e) == (blocks[b], 0)
    # "check word j of block (j + 8) mod 10": what other readers write
    checks = [synth.dm_rs_remainder(data[b::nb], ne // nb) for b in range(nb)]
    assert all(stream[nd + j] == checks[(j + 8) % nb][j // nb] for j in range(ne))
    # the other sizes: stream position and "ndata + q nb + b" are the same thing
    for t in list(range(dm.NUM_SIZES)) + [21, 26, 28]:
        _, _, d2, e2, _, _, b2 = dm.ALL_SIZES[t]
        cw = [(5 * p + 3) % 256 for p in range(d2)]
        ck = [synth.dm_rs_remainder(cw[b::b2], e2 // b2) for b in range(b2)]
        assert synth.dm_interleave(cw, t) == cw + [ck[b][i] for i in range(e2 // b2) for b in range(b2)]


def test_144_round_trips_with_a_distinct_byte_per_position():
    s = 29
    nd = dm.ALL_SIZES[s][2]
    data = [(p * 7 + p // 256) % 256 for p in range(nd)]
    m = synth.dm_matrix(synth.dm_interleave(data, s), s)
    assert m.shape == (144, 144)
    raw = []
    place = dm.placement_of(s)
    for i in range(len(place) // 8):
        v = 0
        for r, c in place[8 * i:8 * i + 8]:
            v = (v << 1) | int(m[r, c])
        raw.append(v)
    assert raw[:nd] == data
    for (r, c), d in dm.function_modules(s).items():
        assert bool(m[r, c]) == d


def test_device_header_large_is_the_committed_file():
    text = dm.device_header_large()
    assert (ROOT / "ocr-system_amd" / "csrc" / "dm_tables_large.h").read_text() == text
    assert "DML_NUM_SIZES = 9, DML_PLACE_N = 79264;" in text and "0, 3136, 7232, 12416, 18816, 26560, 35776, 47440, 61840, 79264" in text


def test_the_librarys_placement_table_is_the_host_modules():
    """the 79 264 entries are built by the library's own walk, not written out: every one equals placement_of"""
    import ctypes
    from lumina_ocr import engine
    lib = engine.load_library()
    total = 0
    for s in LARGE:
        side = dm.ALL_SIZES[s][0]
        want = [(r << 8) | c for r, c in dm.placement_of(s)]
        buf = (ctypes.c_uint16 * (len(want) + 1))()
        buf[len(want)] = 0xBEEF
        assert lib.lumina_ocr_datamatrix_placement(side, buf, len(want)) == len(want) and list(buf[:len(want)]) == want and buf[len(want)] == 0xBEEF
        assert lib.lumina_ocr_datamatrix_placement(side, buf, len(want) - 1) == 0
        total += len(want)
    assert total == 79264 and lib.lumina_ocr_datamatrix_placement(52, buf, 79264) == 0 and lib.lumina_ocr_datamatrix_placement(100, buf, 79264) == 0
