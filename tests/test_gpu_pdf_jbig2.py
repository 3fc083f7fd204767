"""GPU: layered PDF pages with JBIG2 layers through the device path: the records of read_pages(layers=True, jbig2=True) decoded by
Engine.jbig2_decode (the JBIG2 stencil, /Mask stream and 1-bit /SMask) and by Pillow / numpy for the other layers, put together by
Engine.page_compose, equal tests/pdf_layers_reference.py fed the restatement's masks, byte for byte; and a one-image JBIG2 page with
/JBIG2Globals through Engine.jbig2_decode alone."""
import numpy as np
import pytest
import torch

import jbig2_reference as jr
import pdf_jbig2_cases as pj
import pdf_layer_cases as lc
import pdf_layers_reference as lr
from lumina_ocr.utils import pdf_pages as pp

pytestmark = pytest.mark.gpu


def _device_record(engine, rec):
    if rec.filter != "JBIG2Decode":
        return torch.from_numpy(np.array(lc.decode_record(rec))).cuda()   # (a writable copy)
    out, status = engine.jbig2_decode([rec.stream], rec.height, rec.width, [rec.params["globals"]], [int(rec.params["invert"])])
    assert status == [0]
    return out[0]


@pytest.mark.parametrize("name", ["stencil_over_dct", "mask_stream", "smask"])
def test_layered_pages_with_jbig2_layers(engine, name):
    data, want, _ = pj.files()[name]
    entry, = pp.read_pages(data, layers=True, jbig2=True)
    assert isinstance(entry, pp.PageLayers)
    table = lc.layer_table(entry, decode=lambda rec: _device_record(engine, rec))
    got = engine.page_compose((entry.height, entry.width), 1, table)
    torch.cuda.synchronize()
    ref = lr.compose((entry.height, entry.width), 1, lc.layer_table(entry, decode=pj.decode_record))   # the restatement's masks
    assert np.array_equal(got.cpu().numpy(), ref) and np.array_equal(ref[0], want)


@pytest.mark.parametrize("name", ["one_image", "one_image_globals", "decode_1_0", "image_mask_alone"])
def test_one_image_pages(engine, name):
    data, want, _ = pj.files()[name]
    rec, = pp.read_pages(data, jbig2=True)
    assert np.array_equal(_device_record(engine, rec).cpu().numpy(), want)
    assert jr.decode(bytes(rec.stream), rec.params["globals"], rec.height, rec.width, rec.params["invert"])[0] == 0
