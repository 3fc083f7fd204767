"""CPU: valid JPEG 2000 files that OpenJPEG's encoder never writes (tests/jp2_unusual_cases.py, built by tests/jp2_writer.py).  For
every accepted case Pillow decodes the file, the restatement gives status 0 and Pillow's bytes, the host-only probes give 0 and the
restatement's info, and a pixel-preserving rewrite gives the pixels of the file it was made from.  The refused variants (Mb 16,
33 layers) give -2.  Further assertions keep the cases from being vacuous: the deep files really have 15 coded planes in LL and a
block of 37 passes or more, a fifth of their pixels at least is not clamped, and the three-layer files hold every inclusion class and
an Lblock raised beyond need."""
import numpy as np
import pytest

import jp2_cases as jc
import jp2_irreversible_reference as ir
import jp2_reference as jr
import jp2_unusual_cases as uc
import jp2_writer as jw
from lumina_ocr.engine import Engine

KEYS = ("width", "height", "components", "levels", "layers", "progression", "codeblock_width", "codeblock_height")
ACCEPTED = uc.accepted()
REFUSED = uc.refused()


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("case", ACCEPTED, ids=_ids(ACCEPTED))
def test_accepted_case(case):
    want = jc.expected(case.data)                       # Pillow decodes it
    st, reason, info, rgb = uc.reference(case)
    assert st == 0, reason
    assert np.array_equal(rgb, want), "%d values differ from Pillow's" % int((rgb != want).sum())
    if case.base is not None:
        assert np.array_equal(want, jc.expected(case.base)), "the rewrite changed Pillow's pixels"
    rc, got = Engine.jp2_probe_irreversible(case.data)
    assert (rc, [got[k] for k in KEYS], got["reason"]) == (0, info, "")
    rc, got = Engine.jp2_probe(case.data)
    if case.irreversible:
        assert rc == -2 == jr.probe(case.data)[0] and "9/7" in got["reason"]
    else:
        assert (rc, [got[k] for k in KEYS], got["reason"]) == (0, info, "")
        assert ir.probe(case.data) == (0, "", info)     # the 9/7 restatement reads a 5/3 file as the 5/3 one does


@pytest.mark.parametrize("case", REFUSED, ids=_ids(REFUSED))
def test_refused_case(case):
    st, reason, info = ir.probe(case.data) if case.irreversible else jr.probe(case.data)
    assert st == -2 and ("layers" in reason or "bit-planes" in reason), reason
    for probe in (Engine.jp2_probe, Engine.jp2_probe_irreversible) if not case.irreversible else (Engine.jp2_probe_irreversible,):
        rc, got = probe(case.data)
        assert (rc, [got[k] for k in KEYS]) == (-2, info) and got["reason"], got


def _tier2(data):
    """the restatement's blocks of a file after tier 2"""
    d = bytes(data)
    s, e, box = jr.find_codestream(d)
    P = ir.parse_headers(d, s, e, box, [0] * 8)
    comps = jr.geometry(P)
    jr.tier2(d, P, comps)
    return [K for res in comps for bands in res for B in bands for K in B.blocks]


def test_deep_cases_are_deep():
    """what the restatement reads back, not what the writer meant: 15 coded planes in LL, and a block of 37 passes or more in the
    files that do not stop early (a stopped file has the pass count it was stopped at)"""
    deep = [c for c in uc.synthesised() if c.deep]
    assert len(deep) >= 8
    for c in deep:
        blocks = _tier2(c.data)
        ll = [K for K in blocks if K.r == 0 and K.c == 0]
        assert all(K.mb == 15 and K.zbp == 0 for K in ll), c.name
        assert all(K.mb - K.zbp >= 13 for K in blocks if K.c == 0), c.name
        most = max(K.passes for K in blocks)
        if c.full:
            assert most == 43, c.name
            want = jc.expected(c.data)
            inside = ((want > 0) & (want < 255)).all(axis=2).mean()
            assert inside >= 0.20, (c.name, inside)
    stopped = {c.name: max(K.passes for K in _tier2(c.data)) for c in deep if not c.full}
    assert sorted(stopped.values()) == [20, 36, 37, 38], stopped
    h = [c for c in uc.synthesised() if c.family == "h"]
    assert h and all(K.mb - K.zbp == 15 and K.passes == 43 for K in _tier2(h[0].data))
    g = _tier2([c for c in uc.synthesised() if c.family == "g"][0].data)
    assert max(K.passes for K in g if K.r == 1 and K.orient == 3) >= 37 and max(K.mb - K.zbp for K in g if K.r == 2) <= 12


def test_deep_target_is_hit():
    """the constructor's claim: the even / even samples of a deep file are the chosen target, exactly"""
    plane, target = uc.deep_plane(33, 31, 1501)
    want = jc.expected(uc.synthesised()[0].data)
    assert uc.synthesised()[0].name == "a_deep_33x31" and np.array_equal(want[::2, ::2, 0], target)
    assert int(np.abs(plane[:16, :17]).max()).bit_length() == 15


def test_last_passes_of_deep_blocks_decide():
    """among large random values the last passes take no decision, and a decoder that read a pass count of 37 or more one short
    would give the same pixels: the quiet patch of a deep block is there so that in every block the 37th, the 38th and the last
    pass (where the stopped files and the full file end) each change the coefficients"""
    c = uc.synthesised()[0]
    d = bytes(c.data)
    for K in _tier2(d):
        blob = b"".join(d[o:o + n] for o, n in K.segs)
        nbps = K.mb - K.zbp
        assert K.passes == 3 * nbps - 2 >= 40
        got = {n: jr.tier1_block_walk(blob, K.w, K.h, K.orient, nbps, n) for n in (36, 37, 38, K.passes - 1, K.passes)}
        for n in (37, 38, K.passes):
            assert not np.array_equal(got[n - 1], got[n]), (K.orient, n)


def test_zero_bit_planes_reach_mb15():
    c = [c for c in uc.synthesised() if c.family == "c"][0]
    blocks = _tier2(c.data)
    assert all(K.mb == 15 for K in blocks) and min(K.zbp for K in blocks) >= 7 and max(K.zbp for K in blocks) >= 10


def test_three_layer_cases_hold_every_class():
    for c in (c for c in uc.synthesised() if c.family == "d"):
        firsts = {row["first"] for row in c.report}
        assert firsts == {0, 1, 2, None}, (c.name, firsts)
        assert any(row["lblock"] > row["lblock_needed"] for row in c.report), c.name
        assert any(len(row["sizes"]) == 3 and row["sizes"][1][2] == 0 and row["sizes"][2][2] > 0 for row in c.report), "no empty middle contribution"
        assert any([l for l, _, _ in row["sizes"]] == [0, 2] for row in c.report), "no block that skips the middle layer"
        assert any(len({p for _, p, _ in row["sizes"]}) > 1 for row in c.report), "no uneven pass split"
        # and the restatement reads back what the writer planned
        for K, row in zip(_tier2(c.data), sorted(c.report, key=lambda r: (r["c"], r["r"], r["orient"], r["by"], r["bx"]))):
            assert (K.bx, K.by, K.passes, K.included, K.lblock) == (row["bx"], row["by"], row["passes"], row["first"] is not None, row["lblock"])
            assert [n for _, n in K.segs] == [n for _, _, n in row["sizes"]]
            if row["first"] is not None:
                assert K.zbp == row["zbp"]


def test_cut_codewords_are_cut():
    for c, n in zip((c for c in uc.synthesised() if c.family == "e"), (0, 1, 3)):
        blocks = [K for K in _tier2(c.data) if K.passes]
        assert len(blocks) == 4 and all(sum(ln for _, ln in K.segs) == n and K.passes == 3 * (K.mb - K.zbp) - 2 for K in blocks), c.name


def test_encoder_round_trip():
    """MQEncoder and t1_encode against the restatement's decoder, on their own: every orientation, odd sides, 1 to 15 planes"""
    rng = np.random.default_rng(15)
    for h, w, nbps, orient in ((1, 1, 1, 0), (4, 4, 3, 1), (5, 7, 8, 2), (9, 6, 15, 3), (13, 3, 12, 0)):
        coef = rng.integers(-(1 << nbps) + 1, 1 << nbps, (h, w))
        data = jw.t1_encode(coef, orient, nbps, 3 * nbps - 2)
        assert np.array_equal(jr.tier1_block_walk(data, w, h, orient, nbps, 3 * nbps - 2), coef)


def test_tile_part_cases_have_their_parts():
    """the rewrites that cut tile-parts are read as that many parts, and the empty-layer ones as that many layers"""
    by_name = {c.name: c for c in uc.rewritten()}
    for name, parts in (("grey_parts3_psot0_tn0", 3), ("rpcl_parts7_exact_tn7", 7), ("rpcl_parts24_psot0_tn0", 24), ("rpcl_provider", 3)):
        d = by_name[name].data
        s, e, box = jr.find_codestream(d)
        assert len(jr.parse_headers(d, s, e, box, [0] * 8).parts) == parts, name
    assert jr.probe(by_name["cprl_layers_to32"].data)[2][4] == 32 and jr.probe(by_name["grey_layers_to32"].data)[2][4] == 32
