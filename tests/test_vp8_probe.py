"""CPU: lumina_ocr_webp_probe_lossy / lumina_ocr_webp_reason through the C ABI (no handle, no device): lossy and lossless files are
accepted with their info fields, every refusal carries a reason from the lists of csrc/vp8_parse.h, and lumina_ocr_webp_probe keeps
answering -2 for a lossy file."""
import struct

import vp8_cases as vc
import webp_cases as wc
from lumina_ocr.engine import Engine


def test_intact_cases_and_info_fields():
    for name, data in vc.intact_cases():
        rc, info = Engine.webp_probe_lossy(data)
        h, w = vc.pillow_rgb(data).shape[:2]
        assert rc == 0 and info["reason"] == "" and (info["width"], info["height"], info["lossy"], info["alpha"]) == (w, h, 1, 0), name
        assert info["partitions"] == (int(name.split("-")[1]) if name.startswith("parts-") else 1), name
        rc0, info0 = Engine.webp_probe(data)
        assert rc0 == -2 and info0["reason"] == "lossy WebP (VP8)", name
    by = dict(vc.container_cases())
    assert [Engine.webp_probe_lossy(by[k])[1][f] for k in ("vp8x-plain", "vp8x-chunks", "scale-bits") for f in ("vp8x", "exif", "xmp")] == [1, 0, 0, 1, 1, 0, 0, 0, 0]


def test_lossless_files_answer_as_the_lossless_probe():
    for name, data in wc.writer_cases() + wc.refused_cases()[1:]:
        rc, info = Engine.webp_probe_lossy(data)
        rc0, info0 = Engine.webp_probe(data)
        assert rc == rc0 and {k: info[k] for k in info0} == info0 and info["lossy"] == 0 and info["partitions"] == 0, name


def test_refusals_name_their_reason():
    reasons = {name: (Engine.webp_probe_lossy(data)[0], Engine.webp_probe_lossy(data)[1]["reason"]) for name, data, _ in vc.refused_cases()}
    assert reasons == {"lossy-alpha": (-2, "lossy WebP with an ALPH chunk"), "animated": (-2, "animated WebP"),
                       "inter-frame": (-1, "VP8 inter frame"), "show-frame-0": (-1, "VP8 show_frame is 0"),
                       "vp8-and-vp8l": (-1, "both a VP8 and a VP8L chunk"), "canvas-mismatch": (-1, "VP8X canvas differs from the VP8 frame header")}
    (_, vp8), = vc._chunks(dict(vc.intact_cases())["pillow-48x48-RGB-m4-q80"])
    part0 = (vp8[0] | vp8[1] << 8 | vp8[2] << 16) >> 5

    def tag(s, first):
        t = (s[0] & 31) | first << 5
        return bytes([t & 255, (t >> 8) & 255, (t >> 16) & 255]) + bytes(s[3:])
    damaged = {
        "VP8 profile above 3": bytes([vp8[0] | 0x08]) + vp8[1:],
        "VP8 start code is not 9d 01 2a": vp8[:4] + b"\x02" + vp8[5:],
        "VP8 first partition past the chunk": tag(vp8, len(vp8) - 9),
        "VP8 chunk shorter than the frame tag": vp8[:9],
        "VP8 frame of zero width or height": vp8[:6] + b"\0\0" + vp8[8:],
        "VP8 last token partition is empty": tag(vp8[:10 + part0], part0),
        "VP8 frame header past the first partition": tag(vp8, 3),
    }
    for reason, payload in damaged.items():
        rc, info = Engine.webp_probe_lossy(vc.riff([(b"VP8 ", payload)]))
        assert (rc, info["reason"]) == (-1, reason), (reason, rc, info["reason"])
    # the number of partitions is read; a size table past the chunk is refused
    second = vc.riff([(b"VP8 ", vp8), (b"VP8 ", vp8)])
    assert Engine.webp_probe_lossy(second)[0] == -1
    both = vc.riff([vc.vp8x(0, 48, 48), (b"VP8 ", vp8), (b"VP8 ", vp8)])
    assert Engine.webp_probe_lossy(both) [1]["reason"] == "second VP8 chunk"
    assert struct.unpack("<I", both[4:8])[0] + 8 == len(both)
