"""Scanned TIFFs: the container reader.  Host only, pure Python, modelled on utils/pdf_pages.py.

    read_pages(data) -> [PageImage | TiffRefused, ...]      one entry per IFD, in chain order

A TIFF from a scanner or a fax gateway is a chain of IFDs, each one page stored as strips of whole rows.  This module finds the strips
and says how they are coded; the device decoders make the pixels (lumina_ocr_strip_image_decode for LZW, PackBits and raw strips,
lumina_ocr_fax_decode for Group 4, Group 3 and CCITT RLE, lumina_ocr_flate_image_decode for Deflate), under the contract of the other device decoders:
status 0 => byte-identical to Pillow's Image.open(f) (frame k) .convert('RGB'), anything else => the page is left to Pillow.

The acceptance rule: a combination of tags is accepted only if tests/tiff_cases.py holds a file of that combination and
the device decodes it equal to Pillow.  Accepted: classic TIFF (II and MM), stripped layout (no RowsPerStrip: one strip),
PlanarConfiguration 1, Compression 1 / 2 (CCITT RLE) / 3 (Group 3: T4Options 0, 1, 4, 5) / 4 (Group 4) / 5 (LZW) / 8 and 32946 (Deflate) / 32773 (PackBits); Photometric 0 and 1 with one
sample of 1 / 2 / 4 / 8 bits (Pillow opens 2- and 4-bit MinIsWhite files too), Photometric 2 with three 8-bit samples, Photometric 3
with 1 / 2 / 4 / 8-bit indices (a palette entry is ColorMap value // 256, as in Pillow); Predictor 1, or 2 with 8-bit samples under LZW or Deflate (libtiff ignores the tag elsewhere); FillOrder 2
only with the three fax codings (the bits of each byte are reversed here); Orientation 1..8 from tag 274 (an XMP packet without that tag is refused:
Pillow would read tiff:Orientation from it); no tag twice in an IFD.  Everything else is refused with a reason and nothing is
raised past read_pages: a problem of one IFD's tags refuses that page, a problem of the chain (or any exception of this reader's own)
refuses the whole file, which is then one TiffRefused with .whole_file set."""
import struct
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple, Union

MAX_PAGES = 20000            # IFDs in one chain
MAX_STRIPS = 1 << 20         # strips of one page
MAX_SIDE = 65535
CC_MAX_COLS = 8192           # the fax decoders' widest line (csrc/ccitt.h)
COMPRESSIONS = {1: "none", 2: "rle", 3: "group3", 4: "group4", 5: "lzw", 8: "deflate", 32946: "deflate", 32773: "packbits"}
FAX_CODECS = ("group4", "group3", "rle")
CODEC_ID = {"none": 1, "lzw": 5, "packbits": 32773}   # the codec numbers of lumina_ocr_strip_image_decode

_TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 13: 4}
_REVERSE = bytes(int("{:08b}".format(i)[::-1], 2) for i in range(256))


class TiffRefused(Exception):
    """The file, or one page of it, is outside the scanned-TIFF subset; .reason says why, .whole_file whether it speaks for the file."""
    def __init__(self, reason: str, whole_file: bool = False):
        super().__init__(reason)
        self.reason = reason
        self.whole_file = whole_file


@dataclass
class PageImage:
    width: int
    height: int
    codec: str                      # "none" | "lzw" | "packbits" | "group4" | "group3" | "rle" | "deflate"
    rows_per_strip: int
    strips: List[Any]               # memoryviews into the file (bytes for FillOrder 2: the bits already reversed), in row order
    predictor: int                  # 1 | 2
    components: int                 # 1 | 3
    bits: int                       # per component
    indexed: bool
    palette: Optional[bytes]        # 768 bytes of RGB for indexed pages
    invert: bool                    # MinIsWhite: sample 0 is white
    fill_order: int                 # as stored (1 | 2)
    orientation: int                # 1..8, to be applied after the decode
    two_d: bool = False             # Group 3: T4Options bit 0 (lines may be coded two-dimensionally)

    def strip_rows(self, k: int) -> int:
        return min(self.height, (k + 1) * self.rows_per_strip) - k * self.rows_per_strip

    def strip_params(self) -> Tuple[int, ...]:
        """lumina_ocr_strip_image_decode's params of this page (codec none / lzw / packbits)"""
        return (CODEC_ID[self.codec], self.predictor, self.components, self.bits, int(self.indexed), int(self.invert), 0)

    def flate_params(self) -> Tuple[int, ...]:
        return (self.predictor, self.components, self.bits, int(self.indexed), int(self.invert))

    def ccitt_params(self) -> Tuple[int, ...]:
        """(K, EncodedByteAlign, BlackIs1, invert): a coded-white run is sample 0 in a TIFF, which is white under MinIsWhite.  Group 4:
        K -1; Group 3: K 0, or 1 with two-dimensional lines (fill bits need no flag); CCITT RLE: K 0 with byte-aligned lines."""
        k, align = {"group4": (-1, 0), "group3": (int(self.two_d), 0), "rle": (0, 1)}[self.codec]
        return (k, align, 0, int(not self.invert))


class _Ifd:
    def __init__(self, data: memoryview, le: bool, off: int):
        n = len(data)
        if off < 8 or off + 2 > n:
            raise TiffRefused("IFD offset outside the file", True)
        self.E = "<" if le else ">"
        count = struct.unpack_from(self.E + "H", data, off)[0]
        end = off + 2 + 12 * count
        if count == 0 or end + 4 > n:
            raise TiffRefused("IFD outside the file", True)
        self.data = data
        self.tags: Dict[int, Tuple[int, int, int]] = {}
        self.repeated: Optional[int] = None     # a tag that occurs twice (Pillow keeps the last one, other readers the first)
        for k in range(count):
            tag, typ, cnt = struct.unpack_from(self.E + "HHI", data, off + 2 + 12 * k)
            if tag in self.tags:
                self.repeated = tag
            self.tags.setdefault(tag, (typ, cnt, off + 2 + 12 * k + 8))
        self.next = struct.unpack_from(self.E + "I", data, end)[0]

    def values(self, tag: int, limit: int = MAX_STRIPS) -> Optional[List[int]]:
        """the tag's integer values, None when absent; refuses other types, counts past `limit` and values outside the file"""
        if tag not in self.tags:
            return None
        typ, cnt, at = self.tags[tag]
        if typ not in (1, 3, 4):
            raise TiffRefused("tag %d of type %d" % (tag, typ))
        if cnt == 0 or cnt > limit:
            raise TiffRefused("tag %d with %d values" % (tag, cnt))
        size = _TYPE_SIZE[typ] * cnt
        if size > 4:
            at = struct.unpack_from(self.E + "I", self.data, at)[0]
            if at + size > len(self.data):
                raise TiffRefused("values of tag %d outside the file" % tag)
        return list(struct.unpack_from(self.E + "%d%s" % (cnt, {1: "B", 3: "H", 4: "I"}[typ]), self.data, at))

    def one(self, tag: int, default: Optional[int] = None) -> Optional[int]:
        v = self.values(tag)
        if v is None:
            return default
        if len(v) != 1:
            raise TiffRefused("tag %d with %d values" % (tag, len(v)))
        return v[0]


def _page(ifd: _Ifd) -> PageImage:
    data = ifd.data
    if ifd.repeated is not None:
        raise TiffRefused("tag %d occurs twice" % ifd.repeated)
    for tag in (322, 323, 324, 325):
        if tag in ifd.tags:
            raise TiffRefused("tiled layout")
    width, height = ifd.one(256), ifd.one(257)
    if width is None or height is None:
        raise TiffRefused("no ImageWidth / ImageLength")
    if not (0 < width <= MAX_SIDE and 0 < height <= MAX_SIDE):
        raise TiffRefused("image size %d x %d" % (width, height))
    spp = ifd.one(277, 1)
    if 338 in ifd.tags or spp == 4:
        raise TiffRefused("ExtraSamples / 4 samples per pixel")
    bps = ifd.values(258, 8) or [1]
    fmt = ifd.values(339, 8) or [1]
    if any(f != 1 for f in fmt):
        raise TiffRefused("SampleFormat %r" % (fmt,))
    if any(b > 8 for b in bps):
        raise TiffRefused("%d-bit samples" % max(bps))
    photo = ifd.one(262)
    if photo is None:
        raise TiffRefused("no PhotometricInterpretation")
    if photo in (5, 6, 8, 9, 10):
        raise TiffRefused("colour space %s" % {5: "CMYK", 6: "YCbCr"}.get(photo, "Lab"))
    if photo not in (0, 1, 2, 3):
        raise TiffRefused("PhotometricInterpretation %d" % photo)
    if ifd.one(284, 1) != 1 and spp > 1:
        raise TiffRefused("PlanarConfiguration 2")
    comp = ifd.one(259, 1)
    if comp in (6, 7):
        raise TiffRefused("JPEG-in-TIFF (Compression %d)" % comp)
    if comp not in COMPRESSIONS:
        raise TiffRefused("Compression %d" % comp)
    codec = COMPRESSIONS[comp]
    if photo == 2:
        if spp != 3 or bps != [8, 8, 8]:
            raise TiffRefused("RGB with %d samples of %r bits" % (spp, bps))
        comps, bits = 3, 8
    else:
        if spp != 1 or len(bps) != 1 or bps[0] not in (1, 2, 4, 8):
            raise TiffRefused("%d samples of %r bits" % (spp, bps))
        comps, bits = 1, bps[0]
    palette = None
    if photo == 3:
        cmap = ifd.values(320, 768)
        if cmap is None or len(cmap) != 3 << bits:
            raise TiffRefused("ColorMap missing or not 3 x 2^bits entries")
        k = 1 << bits
        pal = bytearray(768)
        for i in range(k):
            pal[3 * i], pal[3 * i + 1], pal[3 * i + 2] = cmap[i] // 256, cmap[k + i] // 256, cmap[2 * k + i] // 256
        palette = bytes(pal)
    predictor = ifd.one(317, 1)
    if predictor not in (1, 2) or (predictor == 2 and bits != 8):
        raise TiffRefused("Predictor %d with %d-bit samples" % (predictor, bits))
    if predictor == 2 and codec not in ("lzw", "deflate"):
        raise TiffRefused("Predictor 2 with compression %s" % codec)   # (libtiff applies it with LZW and Deflate only; elsewhere the tag is ignored)
    fill = ifd.one(266, 1)
    if fill not in (1, 2) or (fill == 2 and codec not in FAX_CODECS):
        raise TiffRefused("FillOrder %d with compression %s" % (fill, codec))
    if 700 in ifd.tags and 274 not in ifd.tags:
        raise TiffRefused("XMP packet without an Orientation tag")   # (Pillow then takes tiff:Orientation from the XMP)
    orientation = ifd.one(274, 1)
    if orientation not in range(1, 9):
        raise TiffRefused("Orientation %d" % orientation)
    if codec == "group4":
        if bits != 1 or photo not in (0, 1) or predictor != 1:
            raise TiffRefused("Group 4 that is not one bit of grey")
        if ifd.one(293, 0) & 2:
            raise TiffRefused("T6Options: uncompressed mode")
        if width > CC_MAX_COLS:
            raise TiffRefused("Group 4 wider than %d" % CC_MAX_COLS)
    two_d = False
    if codec in ("group3", "rle"):
        if bits != 1 or photo not in (0, 1) or predictor != 1:
            raise TiffRefused("Group 3 / CCITT RLE that is not one bit of grey")
        t4 = ifd.one(292, 0) if codec == "group3" else 0   # (bit 2, fill bits before EOLs, needs nothing: the decoder skips fill anyway)
        if t4 & 2:
            raise TiffRefused("T4Options: uncompressed mode")
        if t4 & ~5:
            raise TiffRefused("T4Options %d" % t4)
        if width > CC_MAX_COLS:
            raise TiffRefused("Group 3 / CCITT RLE wider than %d" % CC_MAX_COLS)
        two_d = bool(t4 & 1)
    rps = ifd.one(278, height)
    if rps == 0:
        raise TiffRefused("RowsPerStrip 0")
    rps = min(rps, height)
    want = -(-height // rps)
    offs, counts = ifd.values(273), ifd.values(279)
    if offs is None or counts is None:
        raise TiffRefused("no StripOffsets / StripByteCounts")
    if len(offs) != want or len(counts) != want:
        raise TiffRefused("%d strip offsets and %d byte counts for %d strips" % (len(offs), len(counts), want))
    strips: List[Any] = []
    for o, c in zip(offs, counts):
        if c == 0:
            raise TiffRefused("empty strip")
        if o < 8 or o + c > len(data):
            raise TiffRefused("strip outside the file")
        strips.append(bytes(data[o:o + c]).translate(_REVERSE) if fill == 2 else data[o:o + c])
    return PageImage(width=width, height=height, codec=codec, rows_per_strip=rps, strips=strips, predictor=predictor, components=comps,
                     bits=bits, indexed=photo == 3, palette=palette, invert=photo == 0, fill_order=fill, orientation=orientation, two_d=two_d)


def is_tiff(head: bytes) -> bool:
    return head[:4] in (b"II*\x00", b"MM\x00*")


def read_pages(data, max_pages: Optional[int] = None) -> List[Union[PageImage, TiffRefused]]:
    """One entry per IFD of the TIFF in `data` (bytes, or anything with the buffer protocol: the records' strips are views into it).  A
    file this reader does not take at all comes back as [TiffRefused(reason, whole_file=True)].  max_pages: stop after that many IFDs
    (the rest of the chain is not looked at).  Never raises."""
    try:
        view = memoryview(data).cast("B")
        head = bytes(view[:4])
        if head in (b"II+\x00", b"MM\x00+"):
            raise TiffRefused("BigTIFF", True)
        if not is_tiff(head) or len(view) < 8:
            raise TiffRefused("no TIFF header", True)
        le = head[:2] == b"II"
        off = struct.unpack_from("<I" if le else ">I", view, 4)[0]
        out: List[Union[PageImage, TiffRefused]] = []
        seen = set()
        while off:
            if off in seen:
                raise TiffRefused("IFD chain revisits offset %d" % off, True)
            if len(out) >= MAX_PAGES:
                raise TiffRefused("more than %d IFDs" % MAX_PAGES, True)
            seen.add(off)
            ifd = _Ifd(view, le, off)
            try:
                out.append(_page(ifd))
            except TiffRefused as e:
                if e.whole_file:
                    raise
                out.append(e)
            off = ifd.next
            if max_pages is not None and len(out) >= max_pages:
                break
        if not out:
            raise TiffRefused("no IFD", True)
        return out
    except TiffRefused as e:
        return [TiffRefused(e.reason, True)]
    except Exception as e:   # hostile values in odd places: the whole file goes to Pillow
        return [TiffRefused("malformed file (%s)" % type(e).__name__, True)]
