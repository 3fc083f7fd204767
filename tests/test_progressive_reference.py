"""CPU: the progressive JPEG restatement (tests/progressive_reference.py) validated against Pillow, with no IDCT of its own: for every
case of tests/progressive_cases.py, Pillow's decode of the restatement's sequential transcode equals Pillow's decode of the
progressive original.  The writer's scan scripts open in Pillow and decode to the pixels of the file they were re-emitted from.  The
host probe of the engine library answers for every case (no device is needed for it)."""
import io

import numpy as np
import pytest
from PIL import Image

import progressive_cases as pc
import progressive_reference as pr
from jpeg_cases import CASES, UNSUPPORTED, make_file, pil_decode

FILES = pc.all_files()


@pytest.fixture(scope="module")
def decoded():
    """name -> (Frame, coefficients, stats): every file goes through the restatement once"""
    out = {}
    for name, w, h, data in FILES:
        st = {}
        fr, coefs = pr.decode(data, st)
        out[name] = (fr, coefs, st)
    return out


@pytest.mark.parametrize("name", [f[0] for f in FILES])
def test_baseline_transcode_decodes_to_the_same_pixels_in_pillow(decoded, name):
    _, w, h, data = next(f for f in FILES if f[0] == name)
    fr, coefs, _ = decoded[name]
    assert (fr.width, fr.height) == (w, h)
    base = pr.write_baseline(fr, coefs)
    im = Image.open(io.BytesIO(base))
    assert im.info.get("progressive", 0) in (0, False) and im.size == (w, h)
    got, want = pil_decode(base), pil_decode(data)
    if not np.array_equal(got, want):
        d = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d values differ, first at %s" % (name, len(d), got.size, d[0].tolist()))


@pytest.mark.parametrize("name", list(pc.SCRIPTS))
def test_writer_scripts_open_in_pillow_and_keep_the_pixels(decoded, name):
    base, script, restarts, tables_first = pc.SCRIPTS[name]
    data = pc.script_file(name)
    im = Image.open(io.BytesIO(data))
    assert im.info.get("progressive") and im.size == (base[2], base[3])
    assert np.array_equal(pil_decode(data), pil_decode(pc.pillow_file(base)))        # the same coefficients under another script
    fr = decoded[name][0]
    assert [(tuple(s["comps"]), s["ss"], s["se"], s["ah"], s["al"]) for s in fr.scans] == [tuple(x) for x in script]
    assert [s["restart"] for s in fr.scans] == (list(restarts) if restarts else [0] * len(script))
    if tables_first:
        assert data.find(b"\xff\xc4") < data.find(b"\xff\xda") and data.find(b"\xff\xc4", data.find(b"\xff\xda")) < 0


def test_generated_tables_pass_libjpegs_check():
    """No code is all ones and none is longer than 16 bits, also for counts that would give a deeper tree (Fibonacci-like)."""
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    for freq in ({s: 1 + s % 7 for s in range(0, 256, 3)}, {s: f for s, f in enumerate(fib)}, {0: 5}, {}):
        bits, vals = pr.gen_table(freq)
        assert pr._counts_ok(bits, vals, False) and sorted(vals) == (sorted(freq) or [0]) and len(bits) == 17


def test_white_page_meets_an_eob_run_of_category_14(decoded):
    fr, coefs, st = decoded[pc.WHITE[0]]
    assert comp_blocks(fr) == 16512 and st["max_eob_category"] == 14


def comp_blocks(fr):
    _, _, bw, bh, _, _ = pr.comp_geometry(fr, 0)
    return bw * bh


def test_vga_noise_scans_span_several_chunks(decoded):
    fr, coefs, st = decoded[pc.NOISE_VGA[0]]
    for sc, nbytes in zip(fr.scans, st["scan_bytes"]):
        chroma_ac = sc["ss"] > 0 and sc["comps"][0] > 0
        if not chroma_ac:
            assert nbytes > 2 * 256, (sc["comps"], sc["ss"], sc["se"], sc["ah"], sc["al"], nbytes)


def test_single_component_scans_walk_the_components_own_raster(decoded):
    fr = decoded[pc.BASE_420[0]][0]                    # 37 x 53, 4:2:0: luma raster 5 x 7, padded grid 6 x 8
    assert pr.comp_geometry(fr, 0) == (2, 2, 5, 7, 6, 8) and pr.comp_geometry(fr, 1) == (1, 1, 3, 4, 3, 4)
    assert len(pr.scan_blocks(fr, [0])[0]) == 35 and len(pr.scan_blocks(fr, [0, 1, 2])[0]) == 12 * 6


def test_the_restatement_refuses_what_the_device_must_refuse():
    data = pc.pillow_file(pc.BASE_420)
    fr = pr.parse(data)
    for drop in (1, 3, 4):                             # the last scans cut off, EOI appended: Pillow decodes it, the device must not claim it
        cut = pc.drop_last_scans(data, drop)
        Image.open(io.BytesIO(cut)).load()
        assert pr.status(cut) == -2, drop
    last = fr.scans[-1]
    assert pr.status(pc.cut_inside_last_scan(data)) == -1                                # cut inside a scan's data
    assert pr.status(pc.swap_ah(data)) == -1                                             # a wrong Ah
    twice, later = pc.repeated_first_scan_file()                                         # a complete coefficient sent again as a first scan:
    assert np.array_equal(pil_decode(twice), pil_decode(later))                          # Pillow lets the later scan win, in silence
    assert not np.array_equal(pil_decode(twice), pil_decode(pc.script_file("spectral_only"))) and pr.status(twice) == -2
    name, kind, w, h, seed, kw, mode = UNSUPPORTED[1]
    assert pr.status(make_file((name, kind, w, h, seed, dict(kw, progressive=True), mode))) == -2 and pr.status(b"nope") == -1   # CMYK, progressive
    with pytest.raises(pr.Refused) as e:
        pr.parse(make_file(CASES[0]))
    assert e.value.code == 1                           # a sequential file: the baseline decoder's


def test_host_probe_answers_for_every_case():
    from lumina_ocr.engine import Engine
    for name, w, h, data in FILES:
        rc, info = Engine.jpeg_probe_progressive(data)
        fr = pr.parse(data)
        assert rc == 0 and (info["width"], info["height"]) == (w, h) and info["progressive"] and info["scans"] == len(fr.scans), name
        assert (info["ncomp"], info["h"], info["v"]) == (fr.ncomp, fr.hs, fr.vs), name
        assert Engine.jpeg_probe(data)[0] == -2, name                                    # the old probe keeps its answer
    for case in CASES[:6]:
        data = make_file(case)
        rc, info = Engine.jpeg_probe_progressive(data)
        rc0, info0 = Engine.jpeg_probe(data)
        assert rc == rc0 == 0 and not info["progressive"] and info["scans"] == 1
        assert all(info[k] == info0[k] for k in info0)
    assert Engine.jpeg_probe_progressive(make_file(UNSUPPORTED[1]))[0] == -2 and Engine.jpeg_probe_progressive(b"nope")[0] == -1


def test_host_probe_agrees_with_the_restatements_parser_on_the_damage_corpus():
    """Header level only (what the probe sees): the same answer for every damaged file, and no crash on any of them."""
    from lumina_ocr.engine import Engine
    differ = []
    for name, data in pc.damage_corpus():
        try:
            pr.parse(data)
            want = 0
        except pr.Refused as e:
            want = e.code if e.code != 1 else Engine.jpeg_probe(data)[0]
        got = Engine.jpeg_probe_progressive(data)[0]
        if got != want:
            differ.append((name, got, want))
    assert not differ, differ[:20]
