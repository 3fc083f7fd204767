"""The EAN / UPC / ITF tables of lumina_ocr/utils/barcodes.py, pinned structurally (they are the maintainer's reading of ISO/IEC 15420
and 16390, as Code 128's are of 15417), and csrc/linear_tables.h against its writer."""
from pathlib import Path

from lumina_ocr.utils import barcodes as bc

ROOT = Path(__file__).resolve().parent.parent


def test_set_l_sums_to_seven_and_r_and_g_are_derived():
    assert len(bc.EAN_L) == 10 and all(len(p) == 4 and sum(map(int, p)) == 7 and all(c in "1234" for c in p) for p in bc.EAN_L)
    assert tuple(bc.EAN_R) == tuple(bc.EAN_L)                                  # the same widths, bar first
    assert tuple(bc.EAN_G) == tuple(p[::-1] for p in bc.EAN_L)                # L's widths reversed, space first
    assert bc.EAN_MATCH == tuple(bc.EAN_L) + tuple(bc.EAN_G) and bc.EAN_MODULES == 7
    # as bars and spaces of single modules, R is L's complement and G is R read backwards: the standard's own derivation
    bits = lambda p, first: "".join(str((i + first) % 2) * int(c) for i, c in enumerate(p))
    for v in range(10):
        l, r, g = bits(bc.EAN_L[v], 0), bits(bc.EAN_R[v], 1), bits(bc.EAN_G[v], 0)
        assert r == "".join("10"[int(c)] for c in l) and g == r[::-1]
        assert l[0] == "0" and l[-1] == "1" and l.count("1") % 2 == 1 and g.count("1") % 2 == 0      # odd and even parity


def test_the_thirty_digit_patterns_are_pairwise_distinct():
    tagged = [("space", p) for p in bc.EAN_L] + [("space", p) for p in bc.EAN_G] + [("bar", p) for p in bc.EAN_R]
    assert len(set(tagged)) == 30
    assert len(set(bc.EAN_MATCH)) == 20                                        # what a left-half digit is matched against


def test_ean13_parity_rows():
    assert len(bc.EAN13_PARITY) == 10 and len(set(bc.EAN13_PARITY)) == 10
    assert all(len(p) == 6 and p[0] == "L" and set(p) <= {"L", "G"} for p in bc.EAN13_PARITY)
    assert bc.EAN13_PARITY[0] == "LLLLLL" and all(p.count("G") == 3 for p in bc.EAN13_PARITY[1:])


def test_upce_parity_rows():
    assert len(bc.UPCE_PARITY) == 20 and len(set(bc.UPCE_PARITY)) == 20
    assert all(len(p) == 6 and set(p) <= {"E", "O"} and p.count("E") == 3 for p in bc.UPCE_PARITY)
    assert all(a != b for p, q in zip(bc.UPCE_PARITY[:10], bc.UPCE_PARITY[10:]) for a, b in zip(p, q))   # number system 1: the complement
    assert all(p[0] == "E" for p in bc.UPCE_PARITY[:10])


def test_itf_rows_are_two_of_five_by_the_weights():
    assert len(bc.ITF_PATTERNS) == 10 and len(set(bc.ITF_PATTERNS)) == 10
    for v, p in enumerate(bc.ITF_PATTERNS):
        assert len(p) == 5 and p.count("w") == 2 and p.count("n") == 3
        s = sum(wt for wt, c in zip((1, 2, 4, 7, 0), p) if c == "w")
        assert (0 if s == 11 else s) == v
    for m, wide in zip(bc.ITF_RATIOS, (4, 5, 6)):
        assert all(sum(bc.itf_widths(v, m)) == m and sorted(set(bc.itf_widths(v, m))) == [2, wide] for v in range(10))


def test_layouts_add_up():
    for kind, modules, elements in ((bc.KIND_EAN13, 95, 59), (bc.KIND_EAN8, 67, 43), (bc.KIND_UPCE, 51, 33)):
        nd, nleft, centre, end, nend, bars = bc.EAN_LAYOUT[kind]
        assert 3 + 4 * nd + (5 if centre is not None else 0) + nend == elements == 2 * bars - 1
        assert 3 + 7 * nd + (5 if centre is not None else 0) + nend == modules
        assert end == elements - nend and (centre is None or centre == 3 + 4 * nleft)


def test_device_header_equals_its_writer_and_the_old_one_is_untouched():
    assert (ROOT / "ocr-system_amd" / "csrc" / "linear_tables.h").read_text() == bc.linear_device_header()
    assert (ROOT / "ocr-system_amd" / "csrc" / "barcode_tables.h").read_text() == bc.device_header()
    assert bc.KINDS[:2] == ("Code128", "Code39") and bc.KINDS[2:] == ("EAN13", "EAN8", "UPCE", "ITF")
