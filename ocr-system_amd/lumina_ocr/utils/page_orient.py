"""Host half of the page orientation (the device half: csrc/orient.hip behind lumina_ocr_page_quarter / _page_turn / _page_vote):
which pages of a batch take which pass, and how the passes' results go back into input order.  Pure numpy, no device.

Convention: `turn = t` means the upright page is np.rot90(input_page, t), t quarter turns counter-clockwise."""
from __future__ import annotations

from typing import Iterable, List, Sequence, Tuple

import numpy as np

from .. import arch


def is_sideways(e_r: int, e_c: int, ratio: int = arch.PAGE_ORIENT_PARAMS["ratio"]) -> bool:
    """The rule of lumina_ocr_page_quarter on the two profile energies (Python integers: no overflow)."""
    return int(e_c) > int(ratio) * int(e_r)


def upside_down(votes, min_lines: int = arch.PAGE_ORIENT_PARAMS["min_lines"]) -> np.ndarray:
    """votes int [B,2] = lines, flipped lines per page (lumina_ocr_page_vote) -> bool [B]: at least min_lines lines and more than half
    of them flipped (a tie leaves the page alone)."""
    v = np.asarray(votes, np.int64).reshape(-1, 2)
    return (v[:, 0] >= int(min_lines)) & (2 * v[:, 1] > v[:, 0])


def first_pass_groups(sideways) -> List[Tuple[int, List[int]]]:
    """sideways flags [B] -> [(quarter turn, input indices)]: the pages left as they are (0) and the sideways ones (1, turned by one
    quarter: their batch is W x H), each in input order; empty groups are left out."""
    s = np.asarray(sideways).reshape(-1) != 0
    groups = [(0, np.nonzero(~s)[0].tolist()), (1, np.nonzero(s)[0].tolist())]
    return [g for g in groups if g[1]]


def second_pass(quarter: int, indices: Sequence[int], flipped) -> Tuple[int, List[int], List[int]]:
    """A first-pass group and its pages' upside-down flags -> (total turn of the second pass, input indices that take it, their
    positions in the group).  The second pass turns the RAW page by quarter + 2."""
    f = np.asarray(flipped, bool).reshape(-1)
    assert len(f) == len(indices)
    pos = np.nonzero(f)[0].tolist()
    return (int(quarter) + 2) % 4, [int(indices[k]) for k in pos], pos


def reassemble(n: int, parts: Iterable[Tuple[Sequence[int], Sequence]]) -> list:
    """parts = (input indices, one item per index) of every pass -> the n items in input order; every page exactly once."""
    out = [None] * n
    seen = np.zeros(n, bool)
    for idxs, items in parts:
        assert len(idxs) == len(items)
        for i, it in zip(idxs, items):
            if seen[i]:
                raise ValueError("page %d was produced twice" % i)
            seen[i] = True
            out[i] = it
    if not seen.all():
        raise ValueError("pages %s were not produced" % np.nonzero(~seen)[0].tolist())
    return out


def page_rotation(turn: int) -> int:
    """turn -> the clockwise angle (0 / 90 / 180 / 270) the page was found at: a page found at 90 degrees clockwise is made upright by one
    counter-clockwise quarter turn."""
    return (90 * int(turn)) % 360
