"""CPU: the two exported workspace sizes of the matrix-code readers, lumina_ocr_aztec_workspace_bytes and
lumina_ocr_aztec_layers_workspace_bytes.  They stand for the layout every reader shares (the component regions of runs.h first, the
reader's own behind them): a region moved, resized or realigned shows here.  The literals were read from the library as it was before
the readers shared that layout."""
import pytest

from lumina_ocr import engine

# (pages, height, width, max_finders, max_codes) -> bytes
AZTEC = {(1, 64, 200, 64, 16): 227968, (2, 64, 200, 64, 16): 455424, (3, 2339, 1654, 64, 64): 164115712}
AZTEC_LAYERS = {(1, 64, 200, 64, 16): 400000, (2, 64, 200, 64, 16): 799488, (3, 2339, 1654, 64, 64): 164631808}


@pytest.mark.parametrize("name,want", [("lumina_ocr_aztec_workspace_bytes", AZTEC), ("lumina_ocr_aztec_layers_workspace_bytes", AZTEC_LAYERS)])
def test_workspace_bytes_are_what_they_were(name, want):
    fn = getattr(engine.load_library(), name)
    assert {args: fn(*args) for args in want} == want
    assert fn(1, 0, 200, 64, 16) == 0 and fn(1, 64, 200, 65, 16) == 0      # no rows; more finders than lanes
