"""GPU: the page-analysis entries (table_rules, selection_marks, rules_and_marks, page_quarter, det_postprocess) in the regimes their
own test files never enter, on the pages of tests/page_edge_inputs.py: sides past 4096 pixels (more than 64 mask words per row, so the
run kernels' chunk loop carries a bit across a chunk border; coordinates up to 65534 in the 16-bit run slots), page groups with a
remainder (3 + 3 + 1), components that stress the union-find and the accumulation at the root, and lists exactly at and one past
their capacity of 2048.  Every device result EQUALS the restatement (table_reference, mark_reference, page_orient_reference,
oracle.dbpost): the definitions are integer, there is no tolerance.  tests/test_page_analysis_edge_inputs.py checks the restatements
themselves on the same pages, on the CPU."""
import numpy as np
import pytest
import torch

from lumina_ocr import arch

import mark_reference as mr
import page_edge_inputs as pe
import page_orient_reference as pr
import table_reference as tr
from test_gpu_marks import check as check_marks
from test_gpu_page_orient import _check_quarter
from test_gpu_tables import check as check_rules

pytestmark = pytest.mark.gpu

TP, MP, QP = arch.TABLE_PARAMS, arch.MARK_PARAMS, arch.PAGE_ORIENT_PARAMS
SHORT_RULES = dict(threshold=128, gap=1, min_len=8, max_thick=3, max_rules=2048)    # rules along the short side of a long page too
SENTINEL = -7
LOW_BOX_THRESH = 0.2     # below the 0.25 of prob_of's background: every component of min_size is a box, thin strokes included


def _check_both(engine, pages: np.ndarray):
    """rules_and_marks on pages equals the restatements (and so the solo calls, which the callers check on the same pages)"""
    hr, vr, rc, mk, mc = (t.cpu().numpy() for t in engine.rules_and_marks(torch.from_numpy(pages).cuda()))
    for i, page in enumerate(pages):
        _, rh, rv = tr.table_rules(page)
        ref = mr.selection_marks(page)[1]
        assert rc[i].tolist() == [len(rh), len(rv)] and int(mc[i]) == len(ref), i
        assert np.array_equal(hr[i, :len(rh)], rh) and np.array_equal(vr[i, :len(rv)], rv) and np.array_equal(mk[i, :len(ref)], ref), i
        assert not hr[i, len(rh):].any() and not vr[i, len(rv):].any() and not mk[i, len(ref):].any(), i


def prob_of(ink: np.ndarray) -> np.ndarray:
    """bool -> float32 probability map: 0.9 on the ink, 0.25 (under the threshold of 0.3, exact in bf16) around it"""
    return np.where(ink, np.float32(0.9), np.float32(0.25))


def _post_vs_oracle(engine, prob: np.ndarray, vh: int, vw: int, box_thresh: float = arch.DET_BOX_THRESH) -> int:
    """test_gpu_det's comparison with the C oracle (boxes and scores EQUAL), with the box threshold as a parameter -> boxes in all"""
    from oracle import dbpost
    bits = arch.f32_to_bf16_bits(prob)
    pd = torch.from_numpy(bits.view(np.int16)).cuda().view(torch.bfloat16)
    boxes, scores, counts = engine.det_postprocess(pd, vh, vw, box_thresh=box_thresh)
    torch.cuda.synchronize()
    total = 0
    for i in range(prob.shape[0]):
        rb, rs, ncomp = dbpost.db_postprocess(bits[i], vh, vw, box_thresh=box_thresh)
        n = int(counts[i])
        assert n == len(rb), (i, n, len(rb), ncomp)
        assert np.array_equal(boxes[i, :n].cpu().numpy(), rb), i
        assert np.array_equal(scores[i, :n].cpu().numpy(), rs), i
        assert not boxes[i, n:].any() and not scores[i, n:].any(), i
        total += n
    return total


# ---- long sides --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("turned", [False, True], ids=["long_w", "long_h"])
@pytest.mark.parametrize("shape", pe.LONG_SHAPES, ids=lambda s: "%dx%d" % s)
def test_long_sides(engine, shape, turned):
    """runs that end on, start at and span the 4095 / 4096 border of a row's 64-word chunks (and, on the longest page, the borders
    at 32768 and 61440), frames whose window straddles it, coordinates up to 65534; turned: the long side is H (more than 64 words
    per line of the transposed mask, 65535 rows through row_scan and the per-row waves)"""
    inks, frames = pe.long_inks(*shape)
    pages = pe.page_of(inks)
    whole = [[f for f in frames if f[0] == i] for i in range(len(pages))]
    if turned:
        pages = pe.transposed(pages)
        whole = [[(i, y0, x0, y1, x1) for i, x0, y0, x1, y1 in fs] for fs in whole]
    for rows, fs in zip(check_marks(engine, pages), whole):
        assert {tuple(r[:4]) for r in rows.tolist()} >= {f[1:] for f in fs}
    assert sum(len(fs) for fs in whole) >= 3
    res = check_rules(engine, pages)
    assert sum(len(rv if turned else rh) for rh, rv in res) >= 6 and sum(len(rh if turned else rv) for rh, rv in res) == 0
    res = check_rules(engine, pages, **SHORT_RULES)
    assert sum(len(rh) for rh, rv in res) >= 6 and sum(len(rv) for rh, rv in res) >= 6
    _check_both(engine, pages)
    e, s = _check_quarter(engine, pages)
    assert e.all()


def test_probability_maps_with_blobs_on_the_chunk_border(engine):
    """test_db_postprocess_wide_map's width, with the blobs where its random ones never fall: ending at 4095, starting at 4096,
    spanning the border, specks on either side, touching across it through a corner"""
    maps = pe.long_prob_maps()
    assert maps.shape[1:] == (32, 4160)
    assert _post_vs_oracle(engine, maps, 32, 4160) == 7
    assert _post_vs_oracle(engine, maps[:, :, :4097].copy(), 32, 4097) >= 4      # the border is the map's last column but one
    assert _post_vs_oracle(engine, maps, 31, 4096) >= 4                            # the valid region ends on the border
    low = np.where(maps > 0.5, np.float32(0.9), np.float32(0.25))                  # and with every component of min_size a box
    assert _post_vs_oracle(engine, low, 32, 4160, LOW_BOX_THRESH) > 7


# ---- ragged page groups ------------------------------------------------------------------------------------------------------------
def _filled(shape, dtype=torch.int32):
    return torch.full(shape, SENTINEL, dtype=dtype, device="cuda")


def _raw_entries(engine, pages: np.ndarray, prob_bits: np.ndarray) -> dict:
    """every page-analysis entry through the raw C entry, outputs (and mask hooks) pre-filled with SENTINEL -> name -> numpy array"""
    lib, h, st = engine.lib, engine._h, torch.cuda.current_stream().cuda_stream
    n, H, W, _ = pages.shape
    dev = torch.from_numpy(pages).cuda()
    nw = (W + 63) // 64
    cr, cm, cb = TP["max_rules"], MP["max_marks"], 1000
    out = {}
    hr, vr, rc, hm = _filled((n, cr, 5)), _filled((n, cr, 5)), _filled((n, 2)), _filled((n, H, nw), torch.int64)
    assert lib.lumina_ocr_table_rules(h, dev.data_ptr(), n, H, W, TP["threshold"], TP["gap"], TP["min_len"], TP["max_thick"], cr, hr.data_ptr(),
                                      vr.data_ptr(), rc.data_ptr(), hm.data_ptr(), st) == 0
    out.update(t_hrules=hr, t_vrules=vr, t_counts=rc, t_mask=hm)
    mk, mc, mm = _filled((n, cm, 8)), _filled((n,)), _filled((n, H, nw), torch.int64)
    assert lib.lumina_ocr_selection_marks(h, dev.data_ptr(), n, H, W, MP["threshold"], MP["min_side"], MP["max_side"], cm, mk.data_ptr(), mc.data_ptr(),
                                          mm.data_ptr(), st) == 0
    out.update(m_marks=mk, m_counts=mc, m_mask=mm)
    hr, vr, rc, mk, mc = _filled((n, cr, 5)), _filled((n, cr, 5)), _filled((n, 2)), _filled((n, cm, 8)), _filled((n,))
    assert lib.lumina_ocr_rules_and_marks(h, dev.data_ptr(), n, H, W, TP["threshold"], TP["gap"], TP["min_len"], TP["max_thick"], cr, hr.data_ptr(),
                                          vr.data_ptr(), rc.data_ptr(), MP["min_side"], MP["max_side"], cm, mk.data_ptr(), mc.data_ptr(), st) == 0
    out.update(b_hrules=hr, b_vrules=vr, b_rcounts=rc, b_marks=mk, b_mcounts=mc)
    en, sw = _filled((n, 2), torch.int64), _filled((n,))
    assert lib.lumina_ocr_page_quarter(h, dev.data_ptr(), n, H, W, QP["threshold"], QP["ratio"], en.data_ptr(), sw.data_ptr(), st) == 0
    out.update(q_energies=en, q_sideways=sw)
    prob = torch.from_numpy(prob_bits.view(np.int16)).cuda()
    bx, sc, bc = _filled((n, cb, 8)), torch.full((n, cb), float(SENTINEL), dtype=torch.float32, device="cuda"), _filled((n,))
    assert lib.lumina_ocr_det_postprocess(h, prob.data_ptr(), n, H, W, H, W, arch.DET_THRESH, LOW_BOX_THRESH, arch.DET_UNCLIP_RATIO,
                                          arch.DET_MIN_SIZE, cb, bx.data_ptr(), sc.data_ptr(), bc.data_ptr(), st) == 0
    out.update(d_boxes=bx, d_scores=sc, d_counts=bc)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _rows_equal(got: np.ndarray, ref: np.ndarray, what):
    """the first len(ref) rows are ref, the rows past the count still hold the sentinel"""
    assert np.array_equal(got[:len(ref)], ref), what
    assert (got[len(ref):] == SENTINEL).all(), what


def test_ragged_page_groups(engine):
    """seven pages in groups of 3 + 3 + 1: every pointer an entry offsets per group (pages, lists, counts * 2, mask hooks, the shared
    mask and the rest of the workspace in rules_and_marks) with a group size that does not divide the batch"""
    from oracle import dbpost
    pages = pe.ragged_pages()
    n = len(pages)
    bits = arch.f32_to_bf16_bits(prob_of(np.stack([tr.ink_mask(p) for p in pages])))
    engine.set_option("post_group", 3)
    try:
        split = _raw_entries(engine, pages, bits)
    finally:
        engine.set_option("post_group", 64)
    whole = _raw_entries(engine, pages, bits)
    assert sorted(split) == sorted(whole)
    for k in whole:
        assert np.array_equal(split[k], whole[k]), k
    r = whole
    for i, page in enumerate(pages):
        rmask, rh, rv = tr.table_rules(page)
        ref = mr.selection_marks(page)[1]
        for p in ("t_", "b_"):
            assert r[p + ("counts" if p == "t_" else "rcounts")][i].tolist() == [len(rh), len(rv)], (p, i)
            _rows_equal(r[p + "hrules"][i], rh, (p, i))
            _rows_equal(r[p + "vrules"][i], rv, (p, i))
        for p in ("m_", "b_"):
            assert int(r[p + ("counts" if p == "m_" else "mcounts")][i]) == len(ref), (p, i)
            _rows_equal(r[p + "marks"][i], ref, (p, i))
        assert np.array_equal(r["t_mask"][i].view(np.uint64), rmask) and np.array_equal(r["m_mask"][i].view(np.uint64), rmask), i
        e = pr.energies(page)
        assert r["q_energies"][i].tolist() == list(e) and int(r["q_sideways"][i]) == int(pr.sideways_from(*e)), i
        rb, rs, _ = dbpost.db_postprocess(bits[i], 200, 300, box_thresh=LOW_BOX_THRESH)
        assert int(r["d_counts"][i]) == len(rb) > 0, i
        _rows_equal(r["d_boxes"][i], rb, i)
        _rows_equal(r["d_scores"][i], rs, i)
    assert r["m_counts"].tolist() == list(range(1, n + 1)) and r["t_counts"][:, 0].tolist() == [i % 4 + 1 for i in range(n)]


# ---- hard components ---------------------------------------------------------------------------------------------------------------
def test_hard_components(engine):
    """a spiral and a serpentine (chains of unions as long as the page), spirals whose first run is their last-joined end, nested
    frames, two blobs joined through one corner at the page's right edge, a comb at marks scale joined by its last row only: a wrong
    root gives a wrong box, and the candidate is silently gone"""
    inks = pe.hard_inks()
    names = list(inks)
    stack = np.stack([inks[k] for k in names])
    res = dict(zip(names, check_marks(engine, pe.page_of(stack))))
    (x, y), sides = pe.NESTED_AT, pe.NESTED_SIDES
    assert [r[:4] for r in res["nested"].tolist()] == [[x + 2 * k, y + 2 * k, x + 2 * k + s - 1, y + 2 * k + s - 1] for k, s in enumerate(sides)]
    (x, y), s = pe.COMB_AT, pe.COMB_SIDE
    assert [r[:4] for r in res["combs"].tolist()] == [[x, y, x + s - 1, y + s - 1]]
    assert len(res["small_spirals"]) == 3 and all(len(res[k]) == 0 for k in ("spiral", "serpentine", "diagonal_blobs"))
    check_marks(engine, pe.transposed(pe.page_of(stack)))
    check_marks(engine, pe.page_of(stack[:, ::-1].copy()))        # upside down: the joining row comes FIRST, the teeth hang from the root
    # the thresholded versions through the probability-map path (the same run list and merge, its own root pass)
    for maps in (stack, stack[:, ::-1], np.swapaxes(stack, 1, 2)):
        assert _post_vs_oracle(engine, prob_of(maps), maps.shape[1], maps.shape[2], LOW_BOX_THRESH) == 15


def test_72_roots_in_one_row(engine):
    """more roots in one row of the run list than a wave has lanes: the second pass of the marks kernel's loop over the row"""
    ink = pe.row_of_frames_ink()
    rows, = check_marks(engine, pe.page_of(ink)[None])
    assert len(rows) == pe.ROW_FRAMES == 72 and rows[:, 0].tolist() == [8 + 16 * k for k in range(72)] and set(rows[:, 1].tolist()) == {5}
    rows, = check_marks(engine, pe.transposed(pe.page_of(ink)[None]))
    assert len(rows) == 72
    assert _post_vs_oracle(engine, prob_of(ink)[None], ink.shape[0], ink.shape[1], LOW_BOX_THRESH) == 72


# ---- capacity ----------------------------------------------------------------------------------------------------------------------
def test_marks_at_and_one_past_the_capacity(engine):
    """exactly max_marks = 2048 marks: a full list, sorted, 46 marks sharing every y0; 2049: the count and no rows"""
    pages = pe.page_of(np.stack([pe.marks_grid_ink(2048), pe.marks_grid_ink(2049)]))
    full, over = check_marks(engine, pages, max_marks=2048)      # (check: an overflowing list is not written)
    assert len(full) == 2048 and len(over) == 2049
    full, over = check_marks(engine, pe.transposed(pages), max_marks=2048)
    assert len(full) == 2048 and len(over) == 2049


@pytest.mark.parametrize("turned", [False, True], ids=["horizontal", "vertical"])
def test_rules_at_and_one_past_the_capacity(engine, turned):
    """exactly max_rules = 2048 rules of one direction: 64 share every y0 and 32 every x0; 2049: the count and no rows"""
    for n in (2048, 2049):
        page = pe.page_of(pe.rules_grid_ink(n))[None]
        (rh, rv), = check_rules(engine, pe.transposed(page) if turned else page, **pe.RULE_PARAMS)
        assert (len(rh), len(rv)) == ((0, n) if turned else (n, 0))
