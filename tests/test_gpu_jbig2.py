"""GPU: the JBIG2 decoder (jb2_generic, jb2_mmr and jb2_page of csrc/jbig2.hip, through lumina_ocr_jbig2_decode) equal to the
restatement (tests/jbig2_reference.py) byte for byte and status for status: the CPU cases of tests/jbig2_cases.py grouped by size, a
mixed batch with every template, MMR, refused pages and a page of another size in one call, invert, n == 0, a 24-page group with
different region counts, and a 64-stream sample of the damage sweep."""
import numpy as np
import pytest
import torch

import jbig2_cases as jc
import jbig2_reference as jr
import jbig2_writer as jw

pytestmark = pytest.mark.gpu

FILL = 7   # what the output holds before the call: a page with a non-zero status keeps it


def _call(engine, streams, globals_list, h, w, invert=None):
    out = torch.full((len(streams), h, w, 3), FILL, dtype=torch.uint8, device="cuda")
    out, status = engine.jbig2_decode(streams, h, w, globals_list, invert, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy(), status


def _check(engine, pages, h, w, label, invert=None):
    """pages: [(stream, globals)]; one call; every status and every page's bytes equal to the restatement's -> the statuses"""
    got, status = _call(engine, [s for s, _ in pages], [g for _, g in pages], h, w, invert)
    for i, (s, g) in enumerate(pages):
        st, rgb = jr.decode(s, g, h, w, bool(invert[i]) if invert else False)
        assert status[i] == st, (label, i, status[i], st)
        assert np.array_equal(got[i], rgb if st == 0 else np.full((h, w, 3), FILL, np.uint8)), (label, i)
    return status


def test_cpu_cases_by_size(engine):
    groups = {}
    for c in jc.intact():
        groups.setdefault(c.bits.shape, []).append(c)
    for (h, w), cases in groups.items():
        status = _check(engine, [(c.stream, c.globals_data) for c in cases], h, w, (h, w))
        assert status == [0] * len(cases), [(c.name, s) for c, s in zip(cases, status)]
        got, _ = _call(engine, [c.stream for c in cases], [c.globals_data for c in cases], h, w)
        for c, page in zip(cases, got):   # and the source bitmap itself
            assert np.array_equal(page[..., 1], np.where(c.bits, 0, 255)), c.name


def test_mixed_batch(engine):
    """every template with and without typical prediction and moved AT pixels, MMR, overlapping regions, globals, a -1 page, a -2 page
    and a page of another size in one call; the refused pages are not written"""
    cases = [c for c in jc.intact() if c.bits.shape == (37, 70)]
    refused = {c.name: c for c in jc.refused()}
    other = next(c for c in jc.intact() if c.name == "size_33x5_t1")
    pages = [(c.stream, c.globals_data) for c in cases]
    pages.insert(3, (refused["region_before_page"].stream, None))
    pages.insert(9, (refused["type_6"].stream, None))
    pages.insert(12, (other.stream, None))
    pages.append((refused["symbol_dictionary_in_globals"].stream, refused["symbol_dictionary_in_globals"].globals_data))
    status = _check(engine, pages, 37, 70, "mixed")
    assert sorted(set(status)) == [-4, -2, -1, 0] and status.count(0) == len(cases) >= 20


def test_a_damaged_mmr_region_refuses_its_page_only(engine):
    base, _ = jc.sweep_bases()["mmr"]
    sweep, want = jc.damage_sweep(), jc.sweep_restatement()
    hit = next(d for (name, label, d), (st, info, _) in zip(sweep, want) if name == "mmr" and st == -1 and jr.probe(d)[0] == 0)
    status = _check(engine, [(base, None), (hit, None), (base, None)], 8, 16, "mmr")
    assert status == [0, -1, 0]


def test_invert(engine):
    cases = [c for c in jc.intact() if c.bits.shape == (37, 70)][:6]
    inv = [i & 1 for i in range(len(cases))]
    status = _check(engine, [(c.stream, c.globals_data) for c in cases], 37, 70, "invert", inv)
    assert status == [0] * len(cases)


def test_no_pages(engine):
    out, status = engine.jbig2_decode([], 8, 16)
    assert status == [] and tuple(out.shape) == (0, 8, 16, 3)


def test_24_pages_with_different_region_counts(engine):
    h, w = 20, 64
    pages = []
    for k in range(24):
        regions = []
        for j in range(k % 6):   # (page 0, 6, ...: no region at all, the default pixel alone)
            regions.append(dict(bitmap=jc.bitmap(9 + 5 * j + k, 4 + j, 9800 + 10 * k + j), x=(7 * j + k) % 50, y=(3 * j) % 12, op=(j + k) % 5,
                                tmpl=(j + k) % 4, tpgd=bool((j + k) & 4), mmr=(j == 3)))
        pages.append((jw.page(w, h, regions, default_pixel=k & 1), None))
    status = _check(engine, pages, h, w, "24 pages")
    assert status == [0] * 24


def test_damage_sweep_sample(engine):
    """64 streams of the sweep (bit flips and cuts of the two bases) in one call: the statuses of all, the bytes of the accepted"""
    sweep = jc.damage_sweep()
    pages = [(sweep[i][2], None) for i in jc.sweep_sample(64)]
    status = _check(engine, pages, 8, 16, "sweep sample")
    assert status.count(0) >= 10
