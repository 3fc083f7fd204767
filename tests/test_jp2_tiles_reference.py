"""CPU: the restatement of the tiled JPEG 2000 path (tests/jp2_tiles_reference.py) against Pillow on every case of
tests/jp2_tiles_cases.py, the shapes the cases are meant to have, the refusals with their reasons, the host probe of the library
(lumina_ocr_jp2_probe_ex, no GPU) against the restatement, the answers of the older entries for the same files, and the damage sweep:
every single-bit flip and every truncation of two small files, where each file the restatement accepts must decode to Pillow's bytes."""
import io

import numpy as np
import pytest
from PIL import Image

import jp2_cases as jc
import jp2_irreversible_reference as ir
import jp2_reference as jr
import jp2_tiles_cases as tc
import jp2_tiles_reference as tr
from jp2_reference import _cdiv

GROUPS = ["T1", "T2", "T3", "T4", "T5", "T6", "T7", "T8"]
OLD_REASONS = ("more than one tile", "user precinct sizes", "non-zero image or tile origin")


def _params(data):
    d = bytes(data)
    s, e, box = jr.find_codestream(d)
    return tr.parse_headers(d, s, e, box, [0] * 8)


@pytest.mark.parametrize("group", GROUPS)
def test_restatement_equals_pillow(group):
    cases = [c for c in tc.accepted() if c.group == group]
    assert cases
    for c in cases:
        st, why, info, rgb = tr.reference(c.data)
        want = jc.expected(c.data)
        assert st == 0, (c.name, st, why)
        assert info[:2] == [want.shape[1], want.shape[0]], c.name
        assert rgb.shape == want.shape and np.array_equal(rgb, want), c.name


def test_the_cases_have_the_shapes_they_are_meant_to():
    by_name = {c.name: c for c in tc.accepted()}
    P = _params(by_name["T1_noise"].data)
    assert len(P.tiles) == 12 and len(P.parts) == 12
    assert {(x1 - x0, y1 - y0) for x0, y0, x1, y1 in P.tiles} == {(64, 64), (22, 64), (64, 9), (22, 9)}
    P = _params(by_name["T2_noise"].data)   # odd corners on the lower resolutions: 100 -> 25 and 70 -> 35 on resolution 0
    assert len(P.parts) == 6 and any(_cdiv(x0, 4) & 1 for x0, _, _, _ in P.tiles) and any(_cdiv(y0, 2) & 1 for _, y0, _, _ in P.tiles)
    P = _params(by_name["T3_offsets"].data)
    assert (P.X0, P.Y0) == (10, 6) and len(P.parts) == 12 and P.tiles[0] == (10, 6, 68, 66)
    P = _params(by_name["T3_odd_origin"].data)
    assert (P.X0, P.Y0) == (3, 5) and len(P.tiles) == 1
    for prog in tc.ORDERS:
        P = _params(by_name["T4_" + prog].data)
        assert P.order == tc.ORDERS.index(prog) and P.pp[-1] == (5, 5) and len(tr.geometry(P)[0][0][P.levels]) == 5 * 7
        assert _params(by_name["T4_%s_layers" % prog].data).layers == 3
    P = _params(by_name["T4_cb64_in_p128"].data)   # 64 x 64 precincts on resolution 4: the code-block side there is 32
    assert (P.cbw, P.cbh) == (64, 64) and P.pp[4] == (6, 6) and P.pp[5] == (7, 7)
    sides = [{(K.w, K.h) for Q in tr.geometry(P)[0][0][r] for B in Q.bands for K in B.blocks} for r in (4, 5)]
    assert (32, 32) in sides[0] and max(max(s) for s in sides[0]) == 32 and (64, 64) in sides[1]
    # T5: tiles of one sample at the odd coordinate 63, in x, in y and in both: a lone high-pass sample on resolution 1
    P = _params(by_name["T5_64x64"].data)
    assert [(x1 - x0, y1 - y0) for x0, y0, x1, y1 in P.tiles] == [(63, 63), (1, 63), (63, 1), (1, 1)] and P.tiles[3][:2] == (63, 63)
    assert _params(by_name["T5_1x64"].data).tiles == [(0, 0, 63, 1), (63, 0, 64, 1)]
    assert _params(by_name["T5_64x1"].data).tiles == [(0, 0, 1, 63), (0, 63, 1, 64)]
    # T7: 9/7, and no tile-component has a line of one sample above its lowest resolution (the parser would refuse it)
    for c in tc.accepted():
        if c.group != "T7":
            continue
        P = _params(c.data)
        assert P.irreversible
        for x0, y0, x1, y1 in P.tiles:
            for r in range(1, P.levels + 1):
                sh = P.levels - r
                assert _cdiv(x1, 1 << sh) - _cdiv(x0, 1 << sh) != 1 and _cdiv(y1, 1 << sh) - _cdiv(y0, 1 << sh) != 1, c.name
    assert sum(len(_params(c.data).tiles) > 1 for c in tc.accepted() if c.group == "T7") >= 5
    # T8: the same pixels as T1 from tile-parts in another order, two a tile, the last with Psot = 0
    P = _params(by_name["T8_reversed"].data)
    assert [t for t, _, _ in P.parts] == list(range(11, -1, -1))
    P = _params(by_name["T8_two_parts"].data)
    assert [t for t, _, _ in P.parts] == list(range(12)) + list(range(11, -1, -1)) and all(b > a for _, a, b in P.parts)
    for name in ("T8_reversed", "T8_two_parts", "T8_two_parts_psot0"):
        assert np.array_equal(tr.reference(by_name[name].data)[3], tr.reference(by_name["T1_noise"].data)[3])
    assert by_name["T8_two_parts_psot0"].data != by_name["T8_two_parts"].data


def test_one_tile_with_the_widest_tile_size():
    """XTsiz up to 2^32 - 1 over a one-tile, origin-0 file: the restatement, the library's probes with and without the tiles flag"""
    from lumina_ocr.engine import Engine
    for name, data in tc.one_tile_widest():
        want = jc.expected(data)
        st, why, info, rgb = tr.reference(data)
        assert st == 0 and np.array_equal(rgb, want), (name, st, why)
        assert np.array_equal(jr.decode(data)[3], want), name
        for flags in (Engine.JP2_F_TILES, Engine.JP2_F_TILES | Engine.JP2_F_IRREVERSIBLE):
            assert Engine.jp2_probe_ex(data, flags) == Engine.jp2_probe(data) and Engine.jp2_probe(data)[0] == 0, (name, flags)


def test_refusals():
    for name, data, st, word in tc.refusals():
        got, why, _ = tr.probe(data)
        assert got == st and word in why, (name, got, why)
    # Pillow reads the valid ones of them; the restatement refuses them as outside the subset, not as corrupt
    assert jc.expected(tc.line_of_one_sample()).shape == (64, 130, 3)


def test_without_the_flags_the_older_restatements_answer():
    c = tc.accepted()[0]
    assert tr.decode(c.data, 0, tier1=False)[:2] == jr.decode(c.data, tier1=False)[:2] == (-2, "more than one tile")
    assert tr.decode(c.data, tr.IRREVERSIBLE, tier1=False)[:2] == (-2, "more than one tile")
    c = next(c for c in tc.accepted() if c.name == "T7_64x48")
    st, why, _ = tr.probe(c.data, tr.TILES)
    assert st == -2 and "9/7" in why


def test_library_probe_equals_restatement():
    """lumina_ocr_jp2_probe_ex (host only) on every case and refusal: status, info and reason are the restatement's"""
    from lumina_ocr.engine import Engine
    both = Engine.JP2_F_IRREVERSIBLE | Engine.JP2_F_TILES
    assert both == tr.IRREVERSIBLE | tr.TILES
    for name, data in [(c.name, c.data) for c in tc.accepted()] + [(n, d) for n, d, _, _ in tc.refusals()]:
        for flags in (both, Engine.JP2_F_TILES):
            rc, info = Engine.jp2_probe_ex(data, flags)
            st, why, inf = tr.probe(data, flags)
            assert rc == st and info["reason"] == why, (name, flags, rc, st, info["reason"], why)
            assert [info[k] for k in ("width", "height", "components", "levels", "layers", "progression", "codeblock_width", "codeblock_height")] == inf, name
    assert Engine.jp2_probe(b"")[0] == -1   # (leaves another reason behind for this thread)
    rc, info = Engine.jp2_probe_ex(tc.t1_file(), 4)   # an unknown flag bit has a reason of its own
    assert rc == -1 and info["reason"] == "unknown flag bits"


def test_older_entries_keep_their_answers():
    """lumina_ocr_jp2_probe and lumina_ocr_jp2_probe_irreversible on T1-T8: -2 with the reasons they always gave, and a one-tile
    file through the new probe answers as through the old ones"""
    from lumina_ocr.engine import Engine
    for c in tc.accepted():
        for probe, ref in ((Engine.jp2_probe, jr.probe), (Engine.jp2_probe_irreversible, ir.probe)):
            rc, info = probe(c.data)
            st, why, _ = ref(c.data)
            assert rc == st == -2 and info["reason"] == why and why in OLD_REASONS, (c.name, rc, info["reason"], why)
    for name, data in jc.intact()[:12]:
        rc, info = Engine.jp2_probe_ex(data, Engine.JP2_F_TILES)
        assert (rc, info) == Engine.jp2_probe(data), name


def _pillow(data):
    try:
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    except Exception:   # noqa: BLE001 (whatever Pillow raises for a damaged file)
        return None


def test_damage_sweep_against_pillow():
    """every single-bit flip and every truncation of the two grey bases, and a thinner sweep of the RGB one (tc.damage_bases): a file
    the restatement accepts decodes to Pillow's bytes, and
    it accepts none where Pillow raises.  OpenJPEG decodes some damaged tiled files in part (a tile-part it cannot place is dropped with
    a warning); the strict parser refuses those.  No case is left out."""
    accepted = {}
    bad = []
    for bname, name, data in tc.full_sweep():
        st, why, info, rgb = tr.reference(data)
        if st != 0:
            continue
        accepted[bname] = accepted.get(bname, 0) + 1
        want = _pillow(data)
        if want is None or want.shape != rgb.shape or not np.array_equal(want, rgb):
            bad.append((bname, name, "Pillow raises" if want is None else "pixels differ"))
    assert not bad, (len(bad), bad[:20])
    print("accepted:", accepted, "of", len(tc.full_sweep()))
    assert all(accepted.get(bname, 0) > 100 for bname, _, _ in tc.damage_bases()), accepted
