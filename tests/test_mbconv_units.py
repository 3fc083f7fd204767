"""How the fused expand + depthwise kernel splits a strip's expand phase over its four waves (mb_unit_first / mb_unit_next,
csrc/mbconv.h): for every block of the recogniser and of the orientation classifier, every (pixel tile, channel tile) unit is run by
exactly one wave and no wave runs more than ceil(units / 4) of them.  No GPU: the two functions are compiled for the host from the
header the kernel includes and walked exactly as the kernel walks them (a wave starts at mb_unit_first and steps with mb_unit_next
until pt >= ptiles)."""
import os
import subprocess
from pathlib import Path

import pytest

from lumina_ocr import arch

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ocr-system_amd" / "csrc"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PROGRAM = r"""
#include "mbconv.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
    printf("waves %d\n", MB_WAVES);
    for (int a = 1; a + 1 < argc; a += 2) {
        const int ptiles = atoi(argv[a]), mtiles = atoi(argv[a + 1]);
        for (int w = 0; w < MB_WAVES; ++w) {
            int guard = 0;
            for (MbUnit u = mb_unit_first(w, mtiles); u.pt < ptiles && guard < 100000; u = mb_unit_next(u, mtiles), ++guard)
                printf("%d %d %d %d %d\n", ptiles, mtiles, w, u.pt, u.mt);
        }
    }
    return 0;
}
"""


def _cp16(c):
    return (c + 15) // 16 * 16


def _shapes():
    """(ptiles, mtiles) of every block the kernel serves: recogniser (maps 16 rows high at b0) and classifier (24 rows)."""
    out = []
    for table, h in ((arch.rec_block_table(), arch.REC_H // 2), (arch.cls_block_table(), arch.CLS_H // 2)):
        for b in table:
            ew = 32 + 2 * (b["k"] // 2)
            out.append(((h * ew + 31) // 32, (_cp16(b["exp"]) + 31) // 32))
            h = (h + 2 * (b["k"] // 2) - b["k"]) // b["stride_h"] + 1
    return out


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    d = tmp_path_factory.mktemp("mb_units")
    (d / "units.cpp").write_text(PROGRAM)
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O1", "-I", str(CSRC), str(d / "units.cpp"), "-o", str(d / "units")], check=True)

    def run(shapes):
        args = [str(v) for s in shapes for v in s]
        lines = subprocess.run([str(d / "units")] + args, check=True, capture_output=True, text=True).stdout.split("\n")
        assert lines[0] == "waves 4"
        got = {}
        for ln in lines[1:]:
            if ln:
                pt_n, mt_n, w, pt, mt = (int(v) for v in ln.split())
                got.setdefault((pt_n, mt_n), []).append((w, pt, mt))
        return got
    return run


def test_every_unit_once_and_no_wave_above_its_share(walk):
    shapes = sorted(set(_shapes()))
    assert (5, 4) in shapes and (3, 9) in shapes, shapes          # K = 5 on 4 rows x 128 channels, on 2 rows x 288 channels
    got = walk(shapes)
    for ptiles, mtiles in shapes:
        units = got[(ptiles, mtiles)]
        assert sorted((pt, mt) for _, pt, mt in units) == [(pt, mt) for pt in range(ptiles) for mt in range(mtiles)], (ptiles, mtiles)
        assert all(0 <= mt < mtiles for _, _, mt in units)
        share = -(-ptiles * mtiles // 4)
        for w in range(4):
            mine = [pt * mtiles + mt for ww, pt, mt in units if ww == w]
            assert len(mine) <= share, (ptiles, mtiles, w, len(mine))
            assert mine == list(range(w, ptiles * mtiles, 4)), (ptiles, mtiles, w)      # round-robin, ascending (mbconv.h)


def test_edge_tile_counts(walk):
    """Fewer units than waves, one channel tile (the step of four wraps several pixel tiles), more channel tiles than the step."""
    shapes = [(1, 1), (1, 3), (2, 1), (17, 1), (1, 9), (3, 5), (27, 2)]
    got = walk(shapes)
    for ptiles, mtiles in shapes:
        units = got.get((ptiles, mtiles), [])
        assert sorted((pt, mt) for _, pt, mt in units) == [(pt, mt) for pt in range(ptiles) for mt in range(mtiles)], (ptiles, mtiles)
        for w in range(4):
            assert sum(1 for ww, _, _ in units if ww == w) <= -(-ptiles * mtiles // 4)
