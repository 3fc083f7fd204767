"""CPU: the host-only JPEG 2000 probe (lumina_ocr_jp2_probe, through ctypes) gives the restatement's status and info on every intact
and refused case of tests/jp2_cases.py and on a seeded sample of 300 files of the damage sweep."""
import pytest

import jp2_cases as jc
import jp2_reference as jr
from lumina_ocr.engine import Engine

KEYS = ("width", "height", "components", "levels", "layers", "progression", "codeblock_width", "codeblock_height")
INTACT = jc.intact()
REFUSED = jc.refused()


def info_list(d):
    return [d[k] for k in KEYS]


@pytest.mark.parametrize("case", INTACT, ids=[c[0] for c in INTACT])
def test_intact(case):
    name, data = case
    rc, info = Engine.jp2_probe(data)
    st, _, inf = jr.probe(data)
    assert st == 0
    assert (rc, info_list(info)) == (st, inf) and info["reason"] == ""


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused(case):
    name, data, word = case
    rc, info = Engine.jp2_probe(data)
    st, _, inf = jr.probe(data)
    assert (rc, info_list(info)) == (st, inf) == (-2, inf)
    assert info["reason"] and info["reason"] != "valid JPEG 2000 outside the device subset", info   # its own reason, not the general one


def test_damage_sample():
    sample = jc.sweep_sample(300, seed=300)
    bad = []
    seen = set()
    for bname, name, data in sample:
        rc, info = Engine.jp2_probe(data)
        st, _, inf = jr.probe(data)
        seen.add(st)
        if (rc, info_list(info)) != (st, inf):
            bad.append((bname, name, rc, st, info_list(info), inf))
    assert not bad, bad[:10]
    assert seen == {0, -1, -2}   # the sample holds all three kinds


def test_not_a_file():
    for data in (b"", b"\x00", b"GIF89a" + bytes(40), b"\xff\xd8\xff\xe0" + bytes(60)):
        assert Engine.jp2_probe(data)[0] == -1 == jr.probe(data)[0]


def test_reason_text():
    from lumina_ocr.engine import load_library
    lib = load_library()
    assert lib.lumina_ocr_jp2_reason(-4) == b"another size than the batch"
    rc, info = Engine.jp2_probe(dict((n, d) for n, d, _ in REFUSED)["irreversible"])
    assert rc == -2 and "9/7" in info["reason"]
