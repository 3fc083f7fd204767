"""CPU: the numpy float32 restatement of the 9/7 decoder (tests/jp2_irreversible_reference.py) against Pillow, byte for byte: every
intact case of tests/jp2_irreversible_cases.py, its refusals, and the whole damage sweep of two 9/7 files.  The restatement is what
the host functions and the device decoder are then held to."""
import numpy as np
import pytest

import jp2_cases as jc
import jp2_irreversible_cases as ic
import jp2_irreversible_reference as ir
import jp2_reference as jr

INTACT = ic.intact()
REFUSED = ic.refused()


@pytest.mark.parametrize("case", INTACT, ids=[c[0] for c in INTACT])
def test_restatement_equals_pillow(case):
    name, data = case
    status, reason, info, rgb = ir.reference(data)
    assert status == 0, (name, status, reason)
    exp = jc.expected(data)
    assert rgb.shape == exp.shape and info[0] == exp.shape[1] and info[1] == exp.shape[0]
    assert np.array_equal(rgb, exp), (name, int(np.abs(rgb.astype(int) - exp).max()))


def test_cases_are_irreversible_and_cover_the_list():
    """every case is a 9/7 file the plain restatement refuses for that reason, and the cases hold what they are named for"""
    info = {}
    for name, data in INTACT:
        st, reason, _ = jr.probe(data)
        assert st == -2 and "9/7" in reason, (name, st, reason)
        info[name] = ir.probe(data)[2]
    assert {info[f"prog_{p}"][5] for p in ("LRCP", "RLCP", "RPCL", "PCRL", "CPRL")} == {0, 1, 2, 3, 4}
    assert info["layers_rate_RGB"][4] == 3 and info["layers_db_L"][4] == 2 and info["prog_LRCP"][4] == 2
    assert [info[f"res{nr}_RGB"][3] for nr in (1, 2, 3, 4, 5, 6)] == [0, 1, 2, 3, 4, 5]
    assert info["s5x5_L_r3"][:4] == [5, 5, 1, 2] and info["s17x9_RGB_r4"][:4] == [9, 17, 3, 3]
    assert info["cb8x64_RGB"][6:8] == [8, 64] and info["cb64x8_L"][6:8] == [64, 8] and info["cb4x4_L"][6:8] == [4, 4]
    raw = dict(INTACT)["no_jp2_RGB"]
    assert raw[:4] == b"\xff\x4f\xff\x51" and b"\xff\x58" in dict(INTACT)["plt_RGB"]


def test_reversible_files_take_the_integer_path():
    for name, data in jc.intact()[:12]:
        st, _, info, rgb = ir.decode(data)
        st0, _, info0, rgb0 = jc.reference(data)
        assert (st, info) == (st0, info0) and np.array_equal(rgb, rgb0), name


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_with_reason(case):
    name, data, word = case
    jc.expected(data)   # Pillow reads it: the file is valid
    status, reason, info = ir.probe(data)
    assert status == -2 and word in reason, (name, status, reason)


def test_line_of_one_sample_is_refused():
    """OpenJPEG's encoder writes no 9/7 file with a one-sample line at a resolution above 0, so the header of a 2 x 2 codestream is
    patched to one column: the refusal comes from the headers, before any packet is read"""
    data = bytearray(jc.write(jc.content("noise", 2, 2, "L", 1), irreversible=True, num_resolutions=2, no_jp2=True))
    p = data.index(b"\xff\x51") + 2                 # Lsiz; Xsiz follows Lsiz and Rsiz
    assert int.from_bytes(data[p + 4:p + 8], "big") == 2
    data[p + 4:p + 8] = (1).to_bytes(4, "big")
    st, reason, _ = ir.probe(bytes(data))
    assert st == -2 and "one sample" in reason, (st, reason)


@pytest.mark.parametrize("base", ic.damage_bases(), ids=[b[0] for b in ic.damage_bases()])
def test_damage_sweep_equals_pillow(base):
    """Every damaged variant of the base (each header bit, every 7th data bit, every 16th truncation): a file the restatement accepts
    must decode to Pillow's bytes, with no share left out; Pillow must raise on none of them.
    Counts at the time of writing: rgb97_layers accepted 2175 of 3620, grey97_layers 961 of 2221."""
    bname, data = base
    n_ok = 0
    for name, damaged in jc.damage_sweep(data):
        st, reason, info, rgb = ir.decode(damaged)
        assert st in (0, -1, -2), (bname, name, st)
        if st != 0:
            continue
        exp = jc.expected(damaged)   # (raises if Pillow refuses a file the restatement took)
        assert rgb.shape == exp.shape and np.array_equal(rgb, exp), (bname, name)
        n_ok += 1
    print(bname, "accepted", n_ok, "of", len(jc.damage_sweep(data)))
    assert n_ok >= 100
