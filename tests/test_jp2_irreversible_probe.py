"""CPU: the host-only probe with the irreversible option (lumina_ocr_jp2_probe_irreversible, through ctypes) gives the restatement's
status and info (tests/jp2_irreversible_reference.py) on the intact and refused 9/7 cases, on the 5/3 cases, and on a seeded sample of
300 files of the 9/7 damage sweep; lumina_ocr_jp2_probe keeps its answer for a 9/7 file."""
import pytest

import jp2_cases as jc
import jp2_irreversible_cases as ic
import jp2_irreversible_reference as ir
from lumina_ocr.engine import Engine

KEYS = ("width", "height", "components", "levels", "layers", "progression", "codeblock_width", "codeblock_height")
INTACT = ic.intact()
REFUSED = ic.refused()


def info_list(d):
    return [d[k] for k in KEYS]


@pytest.mark.parametrize("case", INTACT, ids=[c[0] for c in INTACT])
def test_intact(case):
    name, data = case
    rc, info = Engine.jp2_probe_irreversible(data)
    st, _, inf = ir.probe(data)
    assert st == 0
    assert (rc, info_list(info)) == (st, inf) and info["reason"] == ""
    rc, info = Engine.jp2_probe(data)
    assert rc == -2 and "9/7" in info["reason"]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused(case):
    name, data, word = case
    rc, info = Engine.jp2_probe_irreversible(data)
    st, _, inf = ir.probe(data)
    assert (rc, info_list(info)) == (st, inf) == (-2, inf)
    assert word in info["reason"], info


def test_reversible_cases_keep_their_answers():
    for name, data in jc.intact() + [(n, d) for n, d, _ in jc.refused() if n != "irreversible"]:
        assert Engine.jp2_probe_irreversible(data) == Engine.jp2_probe(data), name


def test_damage_sample():
    sample = ic.sweep_sample(300, seed=9701)
    bad = []
    seen = set()
    for bname, name, data in sample:
        rc, info = Engine.jp2_probe_irreversible(data)
        st, _, inf = ir.probe(data)
        seen.add(st)
        if (rc, info_list(info)) != (st, inf):
            bad.append((bname, name, rc, st, info_list(info), inf))
    assert not bad, bad[:10]
    assert seen == {0, -1, -2}   # the sample holds all three kinds
