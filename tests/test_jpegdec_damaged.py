"""CPU: the JPEG decoders' acceptance rule on damaged and hostile files (tests/jpeg_damage.py) against Pillow.

The contract: status 0 (probe 0 and a successful decode) => byte-identical to Pillow; anything else is left to Pillow.  Pillow's own
answer for some damaged files depends on the host CPU (libjpeg-turbo's C inverse DCT wraps out-of-range samples through a
range-limit table, its SIMD versions saturate), so Pillow is run once per SIMD choice the host offers, each in a child process
with its own environment, and a file may only be accepted if the oracle equals all of them.  The device decoder applies the same
rule (tests/test_gpu_jpegdec_damaged.py grades it file for file against the oracle); its header parser is checked here through
the host-only probe."""
import functools
import hashlib
import os
import pickle
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

import jpeg_damage as jd
from jpeg_cases import CASES, make_file, pil_decode
from oracle import jpeg as oj

HERE = Path(__file__).resolve().parent
SIMD_CHOICES = {"c": {"JSIMD_FORCENONE": "1"}, "sse2": {"JSIMD_FORCESSE2": "1"}, "default": {}}

_CHILD = r"""
import hashlib, pickle, sys
sys.path.insert(0, sys.argv[3])
from jpeg_cases import pil_decode
files = pickle.load(open(sys.argv[1], "rb"))
out = {}
for name, data in files:
    try:
        out[name] = hashlib.sha256(pil_decode(data).tobytes()).hexdigest()
    except Exception as e:              # Pillow refuses the file (or raises while loading it)
        out[name] = None
pickle.dump(out, open(sys.argv[2], "wb"))
"""


@functools.lru_cache(maxsize=1)
def corpus():
    return jd.corpus()


@functools.lru_cache(maxsize=None)
def oracle_digest(name):
    """sha256 of the oracle's pixels, or None if the oracle refuses the file"""
    data = dict(corpus())[name]
    if oj.info(data)[0] != 0:
        return None
    try:
        return hashlib.sha256(oj.decode(data).tobytes()).hexdigest()
    except ValueError:
        return None


@pytest.fixture(scope="module")
def pillow():
    """{simd choice: {name: sha256 of Pillow's pixels, or None}} — one child python per choice, this process's environment untouched"""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "corpus.pkl")
        with open(src, "wb") as f:
            pickle.dump(corpus(), f)
        procs = {}
        for k, extra in SIMD_CHOICES.items():
            env = {e: v for e, v in os.environ.items() if not e.startswith("JSIMD_")}
            env.update(extra)
            procs[k] = subprocess.Popen([sys.executable, "-c", _CHILD, src, os.path.join(d, k + ".pkl"), str(HERE)], env=env)
        out = {}
        for k, p in procs.items():
            assert p.wait(timeout=600) == 0, k
            with open(os.path.join(d, k + ".pkl"), "rb") as f:
                out[k] = pickle.load(f)
    return out


def _accepted(names):
    return [n for n in names if oracle_digest(n) is not None]


def test_corpus_is_stable_and_covers_every_base():
    names = [n for n, _ in corpus()]
    assert names == [n for n, _ in jd.corpus()], "the corpus must be the same on every call (seeded)"
    for b in jd.BASES:
        assert sum(n.startswith(b + "_flip") for n in names) == jd.N_FLIPS
        assert any(n.startswith(b + "_trunc") for n in names) and any(n.startswith(b + "_bare_ff") for n in names), b
    for b in ("rst1_420", "rstrow_420"):
        for kind in ("rst_dup", "rst_drop", "rst_renum", "rst_insert_mid"):
            assert any(n.startswith("%s_%s" % (b, kind)) for n in names), (b, kind)


def test_probe_never_crashes_and_parses_like_the_oracle():
    """The device's host-side header parser (lumina_ocr_jpeg_probe) on every entry: no crash, and the oracle's verdict."""
    from lumina_ocr.engine import Engine
    bad = []
    for name, data in corpus():
        rc, _ = Engine.jpeg_probe(data)
        assert rc in (0, -1, -2), (name, rc)
        if rc != oj.info(data)[0]:
            bad.append((name, rc, oj.info(data)[0]))
    assert not bad, "probe and oracle disagree (name, probe, oracle): %s" % bad[:20]


def test_bad_huffman_tables_are_refused_before_the_scan():
    """Oversubscribed, exactly full (the all-ones code), overlong and out-of-range tables: -1 from the probe AND the oracle, so
    the device never builds a table from them (its look-up table would be written out of bounds)."""
    from lumina_ocr.engine import Engine
    dht = [(n, d) for n, d in corpus() if n.startswith("hdr_dht_") and n != "hdr_dht_roundtrip"]
    assert len(dht) >= 7
    for name, data in dht:
        assert Engine.jpeg_probe(data)[0] == -1, name
        assert oj.info(data)[0] == -1, name
    assert oj.info(dict(corpus())["hdr_dht_roundtrip"])[0] == 0


def test_oracle_accepts_only_what_every_pillow_agrees_on(pillow):
    """Oracle rc 0 => Pillow loads the file under every SIMD choice, and the oracle's pixels equal each of them byte for byte."""
    bad = []
    for name, _ in corpus():
        o = oracle_digest(name)
        if o is None:
            continue
        got = {k: pillow[k][name] for k in pillow}
        if any(v != o for v in got.values()):
            bad.append((name, {k: ("refused" if v is None else "differs" if v != o else "equal") for k, v in got.items()}))
    assert not bad, "%d accepted files differ from Pillow: %s" % (len(bad), bad[:20])


def test_pillow_simd_choices_are_honoured(pillow):
    """(the harness itself) every child decoded the whole corpus and agrees on the clean bases"""
    for k, v in pillow.items():
        assert len(v) == len(corpus()), k
    for name in ("hdr_dht_roundtrip", "craft_clean_control"):
        assert len({pillow[k][name] for k in pillow}) == 1 and pillow["c"][name] is not None, name


def test_damage_that_must_be_refused():
    names = dict(corpus())
    must = [n for n in names if "_rst_" in n or n.startswith(("hdr_dri_", "hdr_sof_", "hdr_sos_", "hdr_dqt_short", "hdr_dqt_16bit_large"))]
    must += [n for n in names if "_trunc" in n or "_bare_ff" in n]
    must += ["craft_dc_accumulates_past_int16", "craft_dc_up_and_down", "craft_idct_out_512", "craft_idct_out_-513", "craft_coef_20000_q1",
             "craft_dequant_overflow_q255", "craft_zrl_past_63", "craft_run_past_63", "tail_missing_eoi", "tail_two_eoi", "tail_ff_before_eoi",
             "hdr_adobe_rgb_t0", "hdr_adobe_rgb_t2"]
    accepted = [n for n in must if oracle_digest(n) is not None]
    assert not accepted, accepted
    assert oj.info(names["hdr_adobe_rgb_t0"])[0] == -2


def test_valid_variants_stay_accepted_and_equal_pillow():
    """Refusal must not become "refuse everything": valid files with unusual headers and edge-of-range coefficients are accepted."""
    must = ["hdr_dht_roundtrip", "hdr_dqt_16bit_same_values", "hdr_adobe_grey_t0", "hdr_adobe_grey_t1", "hdr_adobe_grey_t2",
            "hdr_adobe_grey_after_sof", "hdr_adobe_rgb_t1", "tail_junk_after_eoi", "craft_clean_control",
            "craft_idct_out_300", "craft_idct_out_511", "craft_idct_out_-512", "craft_zrl_to_64"]
    names = dict(corpus())
    for n in must:
        assert oracle_digest(n) is not None, n
        assert np.array_equal(oj.decode(names[n]), pil_decode(names[n])), n
    grey = jd.base_file("grey_text")
    for n in ("hdr_adobe_grey_t0", "hdr_adobe_grey_after_sof"):
        assert np.array_equal(pil_decode(names[n]), pil_decode(grey)), n     # Pillow: an Adobe marker does not change a grey file


def test_each_base_keeps_accepting_undamaging_flips():
    """Bit flips that still decode cleanly (a flipped sign bit, a different coefficient) are accepted on every base."""
    for b in jd.BASES:
        n = len(_accepted([x for x, _ in corpus() if x.startswith(b + "_flip")]))
        assert 5 <= n < jd.N_FLIPS, (b, n)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_clean_cases_stay_accepted(case):
    from lumina_ocr.engine import Engine
    data = make_file(case)
    assert Engine.jpeg_probe(data)[0] == 0 and oj.info(data)[0] == 0
    assert np.array_equal(oj.decode(data), pil_decode(data))
