"""GPU: tiled JPEG 2000 files (tiles, image and tile origins, user precincts: tests/jp2_tiles_cases.py) through
lumina_ocr_jp2_decode_ex vs Pillow's Image.open(f).convert('RGB'), byte for byte; statuses per file in a mixed batch; the refusals;
the files the older entries take, through the new entry, give the older entries' bytes; a tiled batch split into sub-batches.  Every
file here has gone through the sanitized host program (tests/test_jp2_tiles_sanitized.py); none is built to provoke a fault."""
import numpy as np
import pytest
import torch

import jp2_cases as jc
import jp2_irreversible_cases as ic
import jp2_tiles_cases as tc
from lumina_ocr.engine import Engine

pytestmark = pytest.mark.gpu

BOTH = Engine.JP2_F_IRREVERSIBLE | Engine.JP2_F_TILES


def _differs(got, want):
    d = np.argwhere(got != want)
    return "%d of %d values differ, first at %s: got %s want %s" % (len(d), got.size, d[0].tolist(), got[tuple(d[0])], want[tuple(d[0])])


def _by_size(files, flags=BOTH):
    groups = {}
    for name, data in files:
        rc, info = Engine.jp2_probe_ex(data, flags)
        assert rc == 0, (name, rc, info["reason"])
        groups.setdefault((info["height"], info["width"]), []).append((name, data))
    return groups


@pytest.mark.parametrize("group", ["T1", "T2", "T3", "T4", "T5", "T6", "T7", "T8"])
def test_cases_equal_pillow(engine, group):
    """the files of one group, one call per size"""
    cases = [(c.name, c.data) for c in tc.accepted() if c.group == group]
    assert cases
    for (h, w), files in _by_size(cases).items():
        out, status = engine.jp2_decode_ex([d for _, d in files], h, w, BOTH)
        assert status == [0] * len(files), (h, w, status)
        for k, (name, data) in enumerate(files):
            got, want = out[k].cpu().numpy(), jc.expected(data)
            assert got.shape == want.shape and np.array_equal(got, want), (name, _differs(got, want))


def test_tiles_flag_alone_refuses_irreversible(engine):
    c = next(c for c in tc.accepted() if c.name == "T7_64x48")
    rc, info = Engine.jp2_probe_ex(c.data, Engine.JP2_F_TILES)
    assert rc == -2 and "9/7" in info["reason"]
    out = torch.full((1, 128, 192, 3), 77, dtype=torch.uint8, device="cuda")
    out, status = engine.jp2_decode_ex([c.data], 128, 192, Engine.JP2_F_TILES, out=out)
    assert status == [-2] and bool((out == 77).all())


def test_mixed_batch_statuses_per_file(engine):
    """one size, one call: a one-tile 5/3 file, a tiled 5/3 file, a tiled 9/7 file, a corrupt one, another size"""
    h, w = 128, 192
    page = jc.text_page(h, w, seed=11)
    tiled = jc.write(page, irreversible=False, tile_size=(64, 48), precinct_size=(32, 32), progression="PCRL")
    files = [jc.write(page, irreversible=False), tiled, jc.write(page, irreversible=True, tile_size=(64, 48), num_resolutions=4),
             tiled[:len(tiled) // 2], tc.t1_file()]
    out = torch.full((len(files), h, w, 3), 77, dtype=torch.uint8, device="cuda")
    out, status = engine.jp2_decode_ex(files, h, w, BOTH, out=out)
    assert status == [0, 0, 0, -1, -4], status
    got = out.cpu().numpy()
    for k in range(3):
        want = jc.expected(files[k])
        assert np.array_equal(got[k], want), (k, _differs(got[k], want))
    assert (got[3:] == 77).all()
    # the entries without the tiles flag refuse the tiled files, as before, and keep their reasons
    _, status = engine.jp2_decode_irreversible(files, h, w)
    assert status == [0, -2, -2, -1, -2], status   # (the file cut in half is cut inside its codestream box: -1 for every entry)
    rc, info = Engine.jp2_probe_irreversible(tiled)
    assert rc == -2 and info["reason"] == "more than one tile"


def test_refusals(engine):
    for name, data, st, word in tc.refusals():
        rc, info = Engine.jp2_probe_ex(data, BOTH)
        assert rc == st and word in info["reason"], (name, rc, info["reason"])
        h, w = max(1, min(info["height"], 256)), max(1, min(info["width"], 256))
        out = torch.full((1, h, w, 3), 77, dtype=torch.uint8, device="cuda")
        out, status = engine.jp2_decode_ex([data], h, w, BOTH, out=out)
        assert status == [st], (name, status)
        assert bool((out == 77).all()), name


def test_files_of_the_older_entries_give_their_bytes(engine):
    """every accepted file of tests/jp2_cases.py and tests/jp2_irreversible_cases.py through the new entry with both flags: the
    statuses and bytes of lumina_ocr_jp2_decode_irreversible; and with the tiles flag alone the 5/3 ones give lumina_ocr_jp2_decode's"""
    for (h, w), group in _by_size(jc.intact() + ic.intact()).items():
        files = [d for _, d in group]
        a, sa = engine.jp2_decode_ex(files, h, w, BOTH)
        b, sb = engine.jp2_decode_irreversible(files, h, w)
        assert sa == sb == [0] * len(files), (h, w, sa, sb)
        assert torch.equal(a, b), (h, w)
    for (h, w), group in _by_size(jc.intact(), Engine.JP2_F_TILES).items():
        files = [d for _, d in group]
        a, sa = engine.jp2_decode_ex(files, h, w, Engine.JP2_F_TILES)
        b, sb = engine.jp2_decode(files, h, w)
        assert sa == sb == [0] * len(files), (h, w, sa, sb)
        assert torch.equal(a, b), (h, w)


def test_one_tile_with_the_widest_tile_size(engine):
    """XTsiz = YTsiz up to 2^32 - 1 over a one-tile, origin-0 file: Pillow's bytes, and those of the older entry"""
    files = [d for _, d in tc.one_tile_widest()]
    a, sa = engine.jp2_decode_ex(files, 40, 40, BOTH)
    b, sb = engine.jp2_decode(files, 40, 40)
    assert sa == sb == [0, 0] and torch.equal(a, b)
    for k, data in enumerate(files):
        assert np.array_equal(a[k].cpu().numpy(), jc.expected(data)), k


def test_tiled_batch_in_sub_batches(engine):
    """1 MB of coefficient planes per sub-batch: a 150 x 201 RGB page takes 0.7 MB, so each of the five files is a sub-batch"""
    cases = [c for c in tc.accepted() if c.group in ("T1", "T3", "T6") and jc.expected(c.data).shape == (201, 150, 3)][:5]
    assert len(cases) == 5
    engine.set_option("jp2_sub_batch_mb", 1)
    try:
        out, status = engine.jp2_decode_ex([c.data for c in cases], 201, 150, BOTH)
    finally:
        engine.set_option("jp2_sub_batch_mb", 4096)
    assert status == [0] * 5
    for k, c in enumerate(cases):
        got, want = out[k].cpu().numpy(), jc.expected(c.data)
        assert np.array_equal(got, want), (c.name, _differs(got, want))
