"""GPU: lumina_ocr_datamatrix_sizes through the C ABI against the restatement (tests/dm_sizes_reference.py): the ink mask, the rows, the
data bytes, the counts and stage 1's candidate counts are EQUAL (integer arithmetic, a canonical order: no tolerance), rows past the
count are untouched, and the decoded strings are what was rendered.  Pages are as small as their symbols allow."""
import numpy as np
import pytest
import torch

from lumina_ocr import arch, synth
from lumina_ocr.engine import EngineError
from lumina_ocr.utils import datamatrix as dm

import dm_pages as DP
import dm_sizes_pages as LP
import dm_sizes_reference as R2

pytestmark = pytest.mark.gpu

P = arch.DM_PARAMS
KEYS = ("min_module", "max_module", "quiet", "timing_max", "solid_max", "max_candidates")
ORDER = ("threshold",) + KEYS + ("max_codes",)


def check(engine, pages: np.ndarray, max_size: int = 144, **params):
    """pages uint8 [n,H,W,3] -> per page (codes, data, candidates) of the restatement, after asserting the device's output equals them."""
    kw = {k: params.get(k, P[k]) for k in KEYS}
    cap = params.get("max_codes", P["max_codes"])
    n, h, w, _ = pages.shape
    dev = torch.from_numpy(np.ascontiguousarray(pages)).cuda()
    codes = torch.full((n, cap, 12), -7, dtype=torch.int32, device="cuda")
    data = torch.full((n, cap, dm.MAX_DATA_ALL), 0xA5, dtype=torch.uint8, device="cuda")
    cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    nc = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    mask = torch.zeros((n, h, (w + 63) // 64), dtype=torch.int64, device="cuda")
    rc = engine.lib.lumina_ocr_datamatrix_sizes(engine._h, dev.data_ptr(), n, h, w, P["threshold"], *[kw[k] for k in KEYS], cap, max_size, codes.data_ptr(),
                                                data.data_ptr(), cnt.data_ptr(), nc.data_ptr(), None, mask.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, engine.lib.lumina_ocr_last_error(engine._h)
    torch.cuda.synchronize()
    codes, data, cnt, nc, mask = codes.cpu().numpy(), data.cpu().numpy(), cnt.cpu().numpy(), nc.cpu().numpy(), mask.cpu().numpy().view(np.uint64)
    out = []
    for i, page in enumerate(pages):
        rmask, rcodes, rdata, rn = LP.reference(page, max_size, **kw)
        assert np.array_equal(mask[i], rmask), "page %d: ink mask differs" % i
        assert int(nc[i]) == rn, "page %d: %d candidates, restatement %d" % (i, nc[i], rn)
        assert int(cnt[i]) == len(rcodes), "page %d: count %d, restatement %d\n%s" % (i, cnt[i], len(rcodes), rcodes)
        m = len(rcodes) if len(rcodes) <= cap else 0
        assert np.array_equal(codes[i, :m], rcodes[:m]), "page %d: rows differ\n%s\n%s" % (i, codes[i, :m], rcodes[:m])
        assert np.array_equal(data[i, :m], rdata[:m]), "page %d: data bytes differ" % i
        assert (codes[i, m:] == -7).all() and (data[i, m:] == 0xA5).all(), "page %d: rows past the count were written" % i
        out.append((rcodes, rdata, rn))
    return out


def stack(pages):
    """pages of different sizes on white canvases of the largest"""
    h, w = max(p.shape[0] for p in pages), max(p.shape[1] for p in pages)
    out = np.full((len(pages), h, w, 3), 255, np.uint8)
    for o, p in zip(out, pages):
        o[:p.shape[0], :p.shape[1]] = p
    return out


@pytest.mark.parametrize("sides", [LP.SIDES[:5], LP.SIDES[5:]])
def test_the_nine_sizes(engine, sides):
    """fails without the entry: lumina_ocr_datamatrix gives these pages empty lists"""
    made = [LP.page_of(LP.size_of(s), rotation=s % 4) for s in sides]
    pages = stack([m[0] for m in made])
    res = check(engine, pages)
    for (rc, rd, rn), (_, box, text), s in zip(res, made, sides):
        assert LP.found(rc, rd) == {box: text} and tuple(rc[0][4:9]) == (s, s, dm.ALL_SIZES[LP.size_of(s)][2], 0, s % 4)
    old = engine.datamatrix(torch.from_numpy(pages).cuda())
    assert old[2].tolist() == [0] * len(sides)


@pytest.mark.parametrize("side", [64, 144])
def test_every_rotation(engine, side):
    made = [LP.page_of(LP.size_of(side), rotation=k) for k in range(4)]
    res = check(engine, np.stack([m[0] for m in made]))
    for k, ((rc, rd, _), (_, box, text)) in enumerate(zip(res, made)):
        assert LP.found(rc, rd) == {box: text} and int(rc[0][8]) == k


def test_another_pitch_and_a_distinct_byte_per_position(engine):
    page, box, text = LP.page_of(22, rotation=3, module=7)
    (rc, rd, _), = check(engine, page[None])
    assert LP.found(rc, rd) == {box: text}
    nd = dm.ALL_SIZES[29][2]
    data = [(p * 7 + p // 256) % 256 for p in range(nd)]
    page, box, _ = LP.page_of(29, 1, text="", matrix=synth.dm_matrix(synth.dm_interleave(data, 29), 29))
    (rc, rd, _), = check(engine, page[None])
    assert [tuple(r[:4]) for r in rc] == [box] and rd[0, :nd].tolist() == data


@pytest.mark.parametrize("size,block", [(29, 9), (29, 0), (26, 5)])
def test_a_block_corrects_half_its_check_words_and_not_one_more(engine, size, block):
    text = LP.payload(size)
    ec = dm.block_lengths(size)[block][1]
    good, box, _ = LP.page_of(size, text=text, matrix=LP.corrupted(text, size, block, ec // 2))
    bad, _, _ = LP.page_of(size, text=text, matrix=LP.corrupted(text, size, block, ec // 2 + 1))
    res = check(engine, np.stack([good, bad]))
    assert LP.found(*res[0][:2]) == {box: text} and int(res[0][0][0][7]) == ec // 2
    assert text not in R2.texts(*res[1][:2])


def test_both_stages_are_sorted_together_and_stage_one_rows_are_the_old_entrys(engine):
    page = LP.blank(88 * 3 + 48, 88 * 3 + 180)
    b = synth.draw_dm(page, 20, 30, synth.dm_encode(LP.payload(24), 24), 3, 1)
    a = DP.put(page, 88 * 3 + 60, 24, "SMALL 24", dm.size_index(24, 24), 3, 2)
    (rc, rd, _), = check(engine, page[None])
    assert LP.found(rc, rd) == {a: "SMALL 24", b: LP.payload(24)}
    assert [tuple(r[:4]) for r in rc] == [a, b] and a[1] < b[1]
    dev = torch.from_numpy(page[None]).cuda()
    old, new = engine.datamatrix(dev, debug=True), engine.datamatrix_sizes(dev, 144, debug=True)
    torch.cuda.synchronize()
    assert int(old[2][0]) == 1 and int(new[2][0]) == 2 and torch.equal(old[4], new[4])
    assert torch.equal(new[0][0, 0], old[0][0, 0]) and torch.equal(new[1][0, 0, :208].int(), old[1][0, 0]) and not bool(new[1][0, 0, 208:].any())
    check(engine, page[None], 64)
    (rc, rd, _), = check(engine, page[None], 87)
    assert LP.found(rc, rd) == {a: "SMALL 24"}


def test_max_size_52_is_the_old_entry(engine):
    pages = stack([synth.synth_dm_page(5, 300, 500, n_codes=3, text_lines=2)[0], synth.synth_dm_decoys()[0], LP.page_of(21)[0]])
    dev = torch.from_numpy(pages).cuda()
    old = engine.datamatrix(dev, debug=True)
    for cap in (52, 144):
        res = check(engine, pages, cap)
        new = engine.datamatrix_sizes(dev, cap, debug=True)
        torch.cuda.synchronize()
        assert new[1].dtype == torch.uint8 and tuple(new[1].shape[1:]) == (P["max_codes"], dm.MAX_DATA_ALL)
        assert torch.equal(new[3], old[3]) and torch.equal(new[4], old[4])
        if cap == 52:
            assert torch.equal(new[0], old[0]) and torch.equal(new[2], old[2])
            assert torch.equal(new[1][:, :, :208].int(), old[1]) and not bool(new[1][:, :, 208:].any())
        else:
            assert new[2].tolist() == [int(old[2][0]), int(old[2][1]), 1]
            assert torch.equal(new[0][:2], old[0][:2]) and torch.equal(new[1][:2, :, :208].int(), old[1][:2])
        assert len(res[0][0]) == int(old[2][0]) >= 1


def test_what_loses_the_large_symbol_leaves_stage_one_alone(engine):
    page = LP.blank(240, 420)
    a = DP.put(page, 20, 30, "SMALL 24", dm.size_index(24, 24), 3, 1)
    b = synth.draw_dm(page, 200, 24, synth.dm_encode(LP.payload(21), 21), 3, 2)
    touched, ring = page.copy(), page.copy()
    touched[b[1] - 4:b[1] + 2, b[2] - 1:b[2] + 5] = 0
    ring[b[1] - 3:b[1] - 1, b[0] + 30:b[0] + 60] = 0
    res = check(engine, np.stack([page, touched, ring]))
    assert [LP.found(*r[:2]) for r in res] == [{a: "SMALL 24", b: LP.payload(21)}, {a: "SMALL 24"}, {a: "SMALL 24"}]
    (rc, rd, _), = check(engine, ring[None], quiet=0)
    assert LP.found(rc, rd) == {a: "SMALL 24", b: LP.payload(21)}


def test_a_stage_two_list_over_capacity_is_not_read_and_stage_one_is(engine):
    page = LP.blank(240, 620)
    a = DP.put(page, 20, 30, "SMALL 24", dm.size_index(24, 24), 3, 1)
    b = synth.draw_dm(page, 200, 24, synth.dm_encode(LP.payload(21), 21), 3, 2)
    c = synth.draw_dm(page, 410, 30, synth.dm_encode(LP.payload(21, "second "), 21), 3)
    (rc, rd, n1), = check(engine, page[None], min_module=3, max_module=3, max_candidates=2)
    assert LP.found(rc, rd) == {a: "SMALL 24", b: LP.payload(21), c: LP.payload(21, "second ")} and n1 == 1
    (rc, rd, n1), = check(engine, page[None], min_module=3, max_module=3, max_candidates=1)
    assert LP.found(rc, rd) == {a: "SMALL 24"} and n1 == 1
    (rc, rd, _), = check(engine, page[None], min_module=3, max_module=3, max_candidates=2, max_codes=2)   # three symbols, two rows: the count alone
    assert len(rc) == 3


@pytest.mark.parametrize("side", [64, 104, 144])
def test_tilted_pages_equal_the_restatement_and_read_where_the_sweep_read(engine, side):
    made, text = LP.tilt_pages(side)
    res = check(engine, np.stack([m[2] for m in made]))
    for (deg, at, _), (rc, rd, _) in zip(made, res):
        if deg == 0.0 or (side, deg) in LP.TILT_READS:
            assert R2.texts(rc, rd) == [text], (side, deg, at)


def test_ragged_page_groups(engine):
    pages = np.stack([LP.page_of(21, rotation=i, text="PAGE %d of the ragged groups" % i)[0] for i in range(4)])
    engine.set_option("post_group", 3)
    try:
        res = check(engine, pages)
    finally:
        engine.set_option("post_group", 64)
    assert [R2.texts(*r[:2]) for r in res] == [["PAGE %d of the ragged groups" % i] for i in range(4)]


def test_bad_arguments_return_a_status_and_launch_nothing(engine):
    pages = torch.from_numpy(LP.blank(64, 200)[None]).cuda()
    good = dict(P, max_codes=4, max_size=144)
    st = torch.cuda.current_stream().cuda_stream
    for bad in (dict(max_size=51), dict(max_size=145), dict(max_codes=0), dict(max_codes=65), dict(max_candidates=0), dict(max_candidates=1025), dict(quiet=5)):
        kw = dict(good, **bad)
        codes = torch.full((1, max(kw["max_codes"], 1), 12), -7, dtype=torch.int32, device="cuda")
        data = torch.full((1, max(kw["max_codes"], 1), dm.MAX_DATA_ALL), 7, dtype=torch.uint8, device="cuda")
        counts = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        rc = engine.lib.lumina_ocr_datamatrix_sizes(engine._h, pages.data_ptr(), 1, 64, 200, *[kw[k] for k in ORDER], kw["max_size"], codes.data_ptr(),
                                                    data.data_ptr(), counts[:1].data_ptr(), counts[1:].data_ptr(), None, None, st)
        torch.cuda.synchronize()
        err = engine.lib.lumina_ocr_last_error(engine._h)
        assert rc != 0 and b"datamatrix_sizes" in err and b"max_size 52..144" in err, bad
        assert bool((codes == -7).all()) and bool((data == 7).all()) and bool((counts == -7).all())
        with pytest.raises(EngineError, match="datamatrix_sizes"):
            engine.datamatrix_sizes(pages, kw["max_size"], **{k: kw[k] for k in ORDER})
    buf = torch.zeros((1, 4, dm.MAX_DATA_ALL), dtype=torch.int32, device="cuda")
    for args in ((None, buf.data_ptr()), (pages.data_ptr(), None)):
        rc = engine.lib.lumina_ocr_datamatrix_sizes(engine._h, args[0], 1, 64, 200, *[good[k] for k in ORDER], 144, args[1], buf.data_ptr(), buf.data_ptr(), None,
                                                    None, None, st)
        assert rc != 0 and b"datamatrix_sizes: bad arguments" in engine.lib.lumina_ocr_last_error(engine._h)
    rc = engine.lib.lumina_ocr_datamatrix_sizes(engine._h, pages.data_ptr(), 1, 0, 200, *[good[k] for k in ORDER], 144, buf.data_ptr(), buf.data_ptr(),
                                                buf.data_ptr(), None, None, None, st)
    assert rc != 0 and b"dimensions" in engine.lib.lumina_ocr_last_error(engine._h)
    ws = engine.lib.lumina_ocr_datamatrix_sizes_workspace_bytes
    assert ws(2, 64, 200, 256, 16) > ws(1, 64, 200, 256, 16) > 0
    assert ws(1, 0, 200, 256, 16) == 0 and ws(1, 64, 200, 1025, 16) == 0 and ws(0, 64, 200, 256, 16) == 0
    with pytest.raises(TypeError):
        engine.datamatrix_sizes(pages, 144, ring_tol=3)


def test_pipeline_reads_the_large_symbol_with_the_option_and_not_without(engine):
    from lumina_ocr.pipeline import OcrPipeline
    charset = arch.ctc_charset()
    engine.load_det(arch.make_det_weights())
    engine.load_rec(arch.make_rec_weights(num_classes=len(charset), code_path=True))
    form = LP.blank(420, 620)
    form[:120] = synth.synth_page(120, 620, 3, n_lines=3, noise=0.0)[0]
    synth.draw_dm(form, 30, 150, synth.dm_encode(LP.payload(22), 22), 3, 1)
    DP.put(form, 400, 200, "SMALL 24", dm.size_index(24, 24), 4)
    pages = torch.from_numpy(np.stack([form, LP.blank(420, 620)])).cuda()
    kw = dict(charset=charset, post=arch.TEXT_PATH_POST)
    (on, empty), processed = OcrPipeline(engine, datamatrix=True, dm_max_size=144, **kw).run(pages)
    (default, _), _ = OcrPipeline(engine, datamatrix=True, **kw).run(pages)
    _, rc, rd, _ = LP.reference(processed[0].cpu().numpy())
    assert np.array_equal(on.datamatrix, rc) and np.array_equal(on.dm_data, rd) and on.dm_data.dtype == np.uint8 and on.dm_data.shape == (2, dm.MAX_DATA_ALL)
    assert sorted(R2.texts(on.datamatrix, on.dm_data)) == sorted(["SMALL 24", LP.payload(22)])
    assert empty.datamatrix.shape == (0, 12) and empty.dm_data.shape == (0, dm.MAX_DATA_ALL)
    assert [e["content"] for e in dm.read_datamatrix(default.datamatrix, default.dm_data)] == ["SMALL 24"] and default.dm_data.shape == (1, dm.MAX_DATA)
    assert default.texts == on.texts
    for bad in (51, 145):
        with pytest.raises(ValueError, match="dm_max_size"):
            OcrPipeline(engine, datamatrix=True, dm_max_size=bad, **kw)
