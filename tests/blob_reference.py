"""The rule the C loader holds a LOCW weight blob to (csrc/blob_check.h), restated independently in Python.

What a model's blob must contain is taken from the SHAPES OF THE GENERATORS (arch.make_det_weights, make_rec_weights, make_cls_weights,
make_svtr_weights Tiny / Base) and from write_blob's storage rule, not from the C table: the tests that compare the two are therefore
also the pin that the C lists and the generators agree.

    check(kind, buf, n) -> (0, "", "") accepted | (1, reason, tensor) refused

The rule:
  - container: magic LOCW, version 1, `count` tensor records (u16 name_len, name, u8 dtype 0 f32 / 1 bf16, u8 ndim 1 .. 4, u32 dims
    each 1 .. 2^28 with a product of at most 2^34, u64 nbytes = product x element size, zeros to a 16-byte offset, data), nothing
    after the last record, no name twice;
  - every tensor of the model present with the generator's dtype, rank and dims; other tensors are ignored;
  - the CTC head's class count C (dims[0] of ctc.fc.w / svtr.ctc.fc.w and of its bias, which must agree) is free in 2 .. 65536;
  - svtr.config is optional (absent: SVTR-Tiny, bf16); present, it is f32 [12] of whole numbers 0 .. 65536 naming a supported variant;
  - where several tensors are wrong, the one whose name sorts first is reported; container errors are reported in file order.
"""
import functools
import struct

import numpy as np

from lumina_ocr import arch

KINDS = ("det", "rec", "cls", "svtr")
CTC_MIN_CLASSES, CTC_MAX_CLASSES = 2, 65536
CLASSES = -1
CTC_HEADS = {"rec": "ctc.fc", "svtr": "svtr.ctc.fc"}
ELEM = {0: 4, 1: 2}


def storage_dtype(name: str) -> int:
    """write_blob's rule: weights travel as bf16 (1), everything else as f32 (0)"""
    return 1 if name.endswith((".w", ".w_ih", ".w_hh")) else 0


@functools.lru_cache(maxsize=None)
def generator_weights(kind: str, variant: str = "tiny", dtype: str = "bf16", seed: int = 1):
    if kind == "det":
        return arch.make_det_weights(seed)
    if kind == "rec":
        return arch.make_rec_weights(seed)
    if kind == "cls":
        return arch.make_cls_weights(seed)
    return arch.make_svtr_weights(seed, variant=variant, dtype=dtype)


@functools.lru_cache(maxsize=None)
def generator_shapes(kind: str, variant: str = "tiny"):
    """name -> (dtype, dims, required) from the generator's own arrays; the class count of the CTC head is CLASSES"""
    out = {}
    head = CTC_HEADS.get(kind)
    for name, a in generator_weights(kind, variant).items():
        dims = tuple(int(v) for v in a.shape)
        if head and name in (head + ".w", head + ".b"):
            dims = (CLASSES,) + dims[1:]
        out[name] = (storage_dtype(name), dims, name != "svtr.config")
    return out


def parse(buf, n):
    """-> ([(name, dtype, dims, nbytes, data_off)], None) | (None, (reason, tensor)); reads buf[:n] only"""
    if n < 12 or bytes(buf[0:4]) != b"LOCW":
        return None, ("bad magic", "")
    ver, cnt = struct.unpack_from("<II", buf, 4)
    if ver != 1:
        return None, ("unsupported version", "")
    off, out, seen = 12, [], set()
    for _ in range(cnt):
        if n - off < 2:
            return None, ("truncated", "")
        (ln,) = struct.unpack_from("<H", buf, off); off += 2
        if n - off < ln + 2:
            return None, ("truncated", "")
        name = bytes(buf[off:off + ln]).decode("latin-1"); off += ln
        dt, nd = buf[off], buf[off + 1]; off += 2
        if dt > 1:
            return None, ("unknown dtype", name)
        if nd < 1 or nd > 4:
            return None, ("rank out of range", name)
        if n - off < 4 * nd + 8:
            return None, ("truncated", name)
        dims = struct.unpack_from("<%dI" % nd, buf, off); off += 4 * nd
        count = 1
        for v in dims:
            if v == 0 or v > 2 ** 28 or count * v > 2 ** 34:
                return None, ("implausible dimension", name)
            count *= v
        (nb,) = struct.unpack_from("<Q", buf, off); off += 8
        off += (-off) % 16
        if nb != count * ELEM[dt]:
            return None, ("byte count does not match the dimensions", name)
        if off > n or nb > n - off:
            return None, ("truncated data", name)
        if name in seen:
            return None, ("duplicate tensor name", name)
        seen.add(name)
        out.append((name, dt, tuple(dims), nb, off))
        off += nb
    if off != n:
        return None, ("trailing bytes", "")
    return out, None


def svtr_variant(buf, tensors):
    """-> (variant name, None) | (None, reason): the variant a blob's svtr.config names, by the rule of the header"""
    t = {name: (dt, dims, off) for name, dt, dims, _, off in tensors}.get("svtr.config")
    if t is None:
        return "tiny", None
    dt, dims, off = t
    if dt != 0:
        return None, "wrong dtype"
    if len(dims) != 1:
        return None, "wrong rank"
    if dims != (12,):
        return None, "wrong dimension"
    c = np.frombuffer(bytes(buf[off:off + 48]), "<f4")
    if not (np.isfinite(c).all() and (c >= 0).all() and (c <= 65536).all() and (c == np.floor(c)).all()):
        return None, "svtr.config value not a small whole number"
    c = [int(v) for v in c]
    dims_, depths, heads, local, out, dtype = c[0:3], c[3:6], c[6:9], c[9], c[10], c[11]
    for d, dep, h in zip(dims_, depths, heads):
        if d not in (64, 128, 256, 384) or h * 32 != d or not 1 <= dep <= 32:
            return None, "svtr.config out of range (dims 64 / 128 / 256 / 384 with 32-wide heads, depths 1 .. 32)"
    if out != arch.SVTR_OUT or dims_[0] > 128:
        return None, "svtr.config out of range (out_channels 192, dims[0] <= 128)"
    if local > depths[0] + depths[1]:
        return None, "svtr.config out of range (local blocks past stage 1)"
    if dtype > 1:
        return None, "svtr.config out of range (dtype 0 / 1)"
    for name, v in arch.SVTR_VARIANTS.items():
        if (tuple(dims_), tuple(depths), tuple(heads)) == (v["dims"], v["depths"], v["heads"]):
            return name, None
    raise NotImplementedError("a valid svtr.config that no generator produces: the restatement has no shapes for it")


def check(kind, buf, n=None):
    n = len(buf) if n is None else n
    tensors, err = parse(buf, n)
    if err:
        return (1,) + err
    variant = "tiny"
    if kind == "svtr":
        variant, reason = svtr_variant(buf, tensors)
        if reason:
            return 1, reason, "svtr.config"
    have = {name: (dt, dims, nb) for name, dt, dims, nb, _ in tensors}
    spec = generator_shapes(kind, variant)
    head = CTC_HEADS.get(kind)
    bad = {}
    classes = 0
    for name in sorted(spec, key=lambda s: (s != (head or "") + ".w", s)):   # the head's weight states the class count: it goes first
        dt, dims, required = spec[name]
        if name not in have:
            if required:
                bad[name] = "missing tensor"
            continue
        gdt, gdims, gnb = have[name]
        if gdt != dt:
            bad[name] = "wrong dtype"
        elif len(gdims) != len(dims):
            bad[name] = "wrong rank"
        else:
            for g, want in zip(gdims, dims):
                if want == CLASSES:
                    if not CTC_MIN_CLASSES <= g <= CTC_MAX_CLASSES:
                        bad[name] = "class count out of range"
                        break
                    classes = classes or g
                    want = classes
                if g != want:
                    bad[name] = "wrong dimension"
                    break
    if bad:
        first = min(bad)
        return 1, bad[first], first
    return 0, "", ""
