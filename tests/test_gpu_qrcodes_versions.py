"""GPU: lumina_ocr_qrcodes_versions through the C ABI against the restatement (tests/qr_versions_reference.py): the ink mask, the finder
counts, the counts, the rows and the data bytes are EQUAL — the definition is integer arithmetic with a canonical order, so there is no
tolerance — and the decoded strings are what was rendered.  Rows past the count are untouched.  Pages are 560 x 587."""
import numpy as np
import pytest
import torch

from lumina_ocr import arch, synth
from lumina_ocr.engine import EngineError
from lumina_ocr.utils import qrcodes as qr

import qr_reference as R1
import qr_version_cases as C
import qr_versions_reference as R

pytestmark = pytest.mark.gpu

P = arch.QR_PARAMS
H, W = C.H, C.W
KEYS = ("min_module", "max_module", "quiet", "centre_tol", "ring_tol", "timing_max", "max_finders")


def check(engine, pages: np.ndarray, max_version: int = 40, **params):
    """pages uint8 [n,H,W,3] -> per page (codes, data, finders) of the restatement, after asserting the device's output equals them."""
    kw = {k: params.get(k, P[k]) for k in KEYS}
    cap = params.get("max_codes", P["max_codes"])
    codes, data, cnt, mask, nf = engine.qrcodes_versions(torch.from_numpy(np.ascontiguousarray(pages)).cuda(), max_version, max_codes=cap, debug=True, **kw)
    torch.cuda.synchronize()
    assert data.dtype == torch.uint8 and tuple(data.shape) == (len(pages), cap, qr.MAX_DATA_ALL)
    codes, data, cnt, mask, nf = codes.cpu().numpy(), data.cpu().numpy(), cnt.cpu().numpy(), mask.cpu().numpy().view(np.uint64), nf.cpu().numpy()
    out = []
    for i, page in enumerate(pages):
        rmask, rc, rd, rf = R.qrcodes(page, max_version, **kw)
        assert np.array_equal(mask[i], rmask), "page %d: ink mask differs" % i
        assert int(nf[i]) == rf, "page %d: %d finders, restatement %d" % (i, nf[i], rf)
        assert int(cnt[i]) == len(rc), "page %d: count %d, restatement %d\n%s" % (i, cnt[i], len(rc), rc)
        n = len(rc) if len(rc) <= cap else 0
        assert np.array_equal(codes[i, :n], rc[:n]), "page %d: rows differ\n%s\n%s" % (i, codes[i, :n], rc[:n])
        assert np.array_equal(data[i, :n], rd[:n]), "page %d: data codewords differ" % i
        assert not codes[i, n:].any() and not data[i, n:].any(), "page %d: rows past the count were written" % i
        out.append((rc, rd, rf))
    return out


def found(rc, rd):
    """-> {(x0, y0, x1, y1): text}"""
    return {tuple(int(v) for v in c[:4]): t for c, t in zip(rc, R.texts(rc, rd))}


@pytest.mark.parametrize("half", [0, 1])
def test_the_eight_versions_read(engine, half):
    """11-M, 14-L, 27-Q, 28-H, 32-M, 37-L, 40-L, 40-H at 3 px: four pages a batch"""
    cases = C.EIGHT[4 * half:4 * half + 4]
    pages = np.stack([C.blank() for _ in cases])
    want = [dict([C.put(pages[i], 14 + i, 15 + 2 * i, v, lv)]) for i, (v, lv) in enumerate(cases)]
    res = check(engine, pages)
    assert [found(*r[:2]) for r in res] == want
    assert [tuple(int(x) for x in r[0][0][4:6]) + (int(r[0][0][7]),) for r in res] == [(v, lv, qr.data_codewords(v, lv)) for v, lv in cases]
    assert all(int(r[0][0][8]) == 0 and int(r[0][0][11]) == 0 for r in res)          # clean: no errors, no timing mismatches


@pytest.mark.parametrize("version", [20, 21, 35])
def test_every_level_where_the_alignment_step_changes(engine, version):
    pages = np.stack([C.blank() for _ in range(4)])
    want = [dict([C.put(pages[lv], 20 + 3 * lv, 17, version, lv, rotation=lv)]) for lv in range(4)]
    res = check(engine, pages)
    assert [found(*r[:2]) for r in res] == want
    assert [tuple(int(x) for x in r[0][0][4:6]) for r in res] == [(version, lv) for lv in range(4)]


@pytest.mark.parametrize("version,level,module", [(28, 3, 3), (11, 1, 7)])
def test_every_rotation(engine, version, level, module):
    pages = np.stack([C.blank() for _ in range(4)])
    want = [dict([C.put(pages[r], 31, 22, version, level, module, r)]) for r in range(4)]
    res = check(engine, pages)
    assert [found(*r[:2]) for r in res] == want and [int(r[0][0][9]) for r in res] == [0, 1, 2, 3]


def test_error_capacity_in_the_last_block(engine):
    """ec // 2 errors in the last block of 40-H and of 37-L are corrected; one more and the symbol is not read as its content"""
    pages = np.stack([C.blank() for _ in range(4)])
    want = []
    for i, (v, lv) in enumerate(((40, 3), (37, 0))):
        nb, _, _, ec = qr.block_structure(v, lv)
        for extra in (0, 1):
            text, sym = C.corrupted(v, lv, nb - 1, ec // 2 + extra)
            box, _ = C.put(pages[2 * i + extra], 12, 13, v, lv, sym=sym)
            want.append({} if extra else {box: text})
    res = check(engine, pages)
    assert [found(*r[:2]) for r in res] == want
    assert int(res[0][0][0][8]) == 15 and int(res[2][0][0][8]) == 15


def test_second_version_copy_mixed_sizes_page_edges_and_a_version_window(engine):
    pages = np.stack([C.blank() for _ in range(4)])
    text, sym = C.version_copy_destroyed(14, 0, (0,))
    a = C.put(pages[0], 20, 20, 14, 0, sym=sym)[0]
    b = C.put(pages[0], 300, 300, 14, 0, sym=C.version_copy_destroyed(14, 0, (0, 1))[1])[0]      # both copies: not read
    c, text12 = C.put(pages[1], 20, 30, 12, 2, 4)
    d = synth.draw_qr(pages[1], 400, 60, synth.qr_encode("SMALL NEIGHBOUR", 3, 1, 2), 4)
    side = qr.dimension(16) * 3
    e, text16 = C.put(pages[2], W - side, H - side, 16, 1, rotation=2)                             # against the right and bottom edges
    f, text14 = C.put(pages[3], 40, 40, 14, 1)
    res = check(engine, pages)
    assert found(*res[0][:2]) == {a: text} and b not in found(*res[0][:2])
    assert found(*res[1][:2]) == {c: text12, d: "SMALL NEIGHBOUR"}
    assert found(*res[2][:2]) == {e: text16} and found(*res[3][:2]) == {f: text14}
    (rc, _, rf), = check(engine, pages[3:], max_version=13)                                        # a version 14 symbol outside the window
    assert len(rc) == 0 and rf == 3


def test_tilted_pages_equal_the_restatement(engine):
    page = C.blank()
    _, text = C.put(page, 90, 100, 25, 1)
    res = check(engine, np.stack([C.tilted(page, 1.0), C.tilted(page, 2.0)]))
    assert R.texts(*res[0][:2]) == [text] and R.texts(*res[1][:2]) == [text]


def test_small_symbols_equal_the_ten_version_call(engine):
    """max_version = 10 on any page, and max_version = 40 on a page of small symbols, give lumina_ocr_qrcodes' rows and codewords"""
    pages = np.stack([synth.synth_qr_page(s, h=H, w=W, n_codes=2, text_lines=3, module_px=3)[0] for s in (3, 4)] + [C.blank()])
    C.put(pages[2], 30, 30, 12, 1)
    dev = torch.from_numpy(pages).cuda()
    old = [t.cpu().numpy() for t in engine.qrcodes(dev, debug=True)]
    assert int(old[2][:2].sum()) >= 3 and int(old[2][2]) == 0
    for max_version, upto in ((10, 3), (40, 2)):
        new = [t.cpu().numpy() for t in engine.qrcodes_versions(dev, max_version, debug=True)]
        assert np.array_equal(new[0][:upto], old[0][:upto]) and np.array_equal(new[2][:upto], old[2][:upto])
        assert np.array_equal(new[1][:upto, :, :qr.MAX_DATA], old[1][:upto]) and not new[1][:upto, :, qr.MAX_DATA:].any()
        assert np.array_equal(new[3], old[3]) and np.array_equal(new[4], old[4])
    assert int(new[2][2]) == 1 and int(new[0][2, 0, 4]) == 12
    again = engine.qrcodes_versions(dev, 40, mask_in=torch.from_numpy(old[3]).cuda(), debug=True)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(again, new))
    for i in range(2):
        rc, rd, _ = R1.codes_of_ink(R1.ink_mask(pages[i], P["threshold"]))
        assert np.array_equal(new[0][i, :len(rc)], rc) and np.array_equal(new[1][i, :len(rc), :qr.MAX_DATA], rd)


def test_ragged_page_groups(engine):
    """Four 250 x 310 pages in groups of 3 + 1: every per-group offset of the entry, the 2956-byte data stride among them.  The split
    call equals the restatement, itself with its own mask handed back in, the call in one group, and every page alone — rows, data,
    counts, mask and finder counts each time."""
    pages = np.stack([C.blank(250, 310) for _ in range(4)])
    want = [dict([C.put(pages[0], 20, 16, 2, 1, tag="P0 ")]), {},
            dict([C.put(pages[2], 14, 12, 11, 1, tag="P2 "), C.put(pages[2], 230, 40, 1, 0, tag="P2b ")]),      # stage 2 beside stage 1
            dict([C.put(pages[3], 18, 14, 12, 2, tag="P3 ")])]
    dev = torch.from_numpy(pages).cuda()
    call = lambda t, **kw: [x.cpu().numpy() for x in engine.qrcodes_versions(t, 40, debug=True, **kw)]
    engine.set_option("post_group", 3)
    try:
        res = check(engine, pages)
        split = call(dev)
        again = call(dev, mask_in=torch.from_numpy(split[3]).cuda())
    finally:
        engine.set_option("post_group", 64)
    assert [found(*r[:2]) for r in res] == want and len({t for f in want for t in f.values()}) == 4
    assert [int(c) for c in split[2]] == [1, 0, 2, 1] and [int(f) for f in split[4]] == [3, 0, 6, 3]
    whole = call(dev)
    for other in (again, whole):
        assert all(np.array_equal(a, b) for a, b in zip(split, other))
    for i in range(4):
        assert all(np.array_equal(a[i:i + 1], b) for a, b in zip(split, call(dev[i:i + 1]))), "page %d alone differs" % i


def test_bad_arguments_return_a_status_and_launch_nothing(engine):
    pages = torch.from_numpy(C.blank(64, 200)[None]).cuda()
    order =("threshold", "min_module", "max_module", "quiet", "centre_tol", "ring_tol", "timing_max", "max_finders", "max_codes", "max_version")
    good = dict(P, max_codes=4, max_version=40)
    st = torch.cuda.current_stream().cuda_stream
    for bad in (dict(max_version=9), dict(max_version=41), dict(max_version=-1), dict(max_codes=0), dict(max_codes=65), dict(max_finders=65), dict(quiet=5),
                dict(min_module=0), dict(timing_max=129)):
        kw = dict(good, **bad)
        codes = torch.full((1, max(kw["max_codes"], 1), 12), -7, dtype=torch.int32, device="cuda")
        data = torch.full((1, max(kw["max_codes"], 1), qr.MAX_DATA_ALL), 249, dtype=torch.uint8, device="cuda")
        counts = torch.full((2,), -7, dtype=torch.int32, device="cuda")
        rc = engine.lib.lumina_ocr_qrcodes_versions(engine._h, pages.data_ptr(), 1, 64, 200, *[kw[k] for k in order], codes.data_ptr(), data.data_ptr(),
                                                    counts[:1].data_ptr(), counts[1:].data_ptr(), None, None, st)
        torch.cuda.synchronize()
        assert rc != 0 and b"qrcodes_versions" in engine.lib.lumina_ocr_last_error(engine._h), bad
        assert bool((codes == -7).all()) and bool((data == 249).all()) and bool((counts == -7).all())
        with pytest.raises(EngineError):
            engine.qrcodes_versions(pages, kw.pop("max_version"), **{k: kw[k] for k in order[:-1]})
    codes = torch.zeros((1, 4, 12), dtype=torch.int32, device="cuda")
    for args in ((None, codes.data_ptr()), (pages.data_ptr(), None)):
        rc = engine.lib.lumina_ocr_qrcodes_versions(engine._h, args[0], 1, 64, 200, *[good[k] for k in order], args[1], codes.data_ptr(), codes.data_ptr(), None,
                                                    None, None, st)
        assert rc != 0 and b"bad arguments" in engine.lib.lumina_ocr_last_error(engine._h)
    rc = engine.lib.lumina_ocr_qrcodes_versions(engine._h, pages.data_ptr(), 1, 0, 200, *[good[k] for k in order], codes.data_ptr(), codes.data_ptr(),
                                                codes.data_ptr(), None, None, None, st)
    assert rc != 0 and b"dimensions" in engine.lib.lumina_ocr_last_error(engine._h)
    with pytest.raises(TypeError):
        engine.qrcodes_versions(pages, 40, max_dist=3)
