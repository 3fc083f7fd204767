"""Mutants of the generators' LOCW blobs for the tests of the weight loader (csrc/blob_check.h, the eng_load_* of csrc/engine.hip).

A mutant is a recipe over its base blob, never a second copy of it (a detector blob is 25 MB and has some 1500 mutants):
    patches : [(offset, bytes)]      overwritten in place (same length)
    tail    : [(bytes, zero_count)]  appended after the base: the bytes, then zero_count zeros (a tensor's data, which no check reads)
    trunc   : the blob is cut to this length (after the two above), or None
    odd     : the blob is handed over at an odd address
A mutant that changes what ONE tensor says (dtype, rank, a dimension, its layout) stays a well-formed container, so that it reaches
the check behind the parser: the original record is renamed in place (first character -> "~": an unknown tensor, which is ignored)
and the changed record, with a byte count and data that fit its new dims, is appended as one more tensor.  tests/blob_main.cpp and
the restatement (tests/blob_reference.py) both apply the recipe to a working copy and undo it.

full_blob / gpu_mutants build complete blobs with real data, for the loads of tests/test_gpu_blob_refusals.py."""
import struct
from collections import namedtuple

import numpy as np

from lumina_ocr import arch

import blob_reference as br

Mutant = namedtuple("Mutant", "label tensor patches tail trunc odd")
Record = namedtuple("Record", "name dtype dims nbytes hdr_off dims_off nbytes_off data_off")
TORCH = (0, 3, 1, 2)   # OHWI [out][kh][kw][in] -> torch's OIHW [out][in][kh][kw] (depthwise [c][k][k][1] -> [c][1][k][k], SE [mid][1][1][c] -> [mid][c][1][1])


def M(label, tensor="", patches=(), tail=(), trunc=None, odd=False):
    return Mutant(label, tensor, list(patches), list(tail), trunc, odd)


def records(blob):
    """the records of an intact blob, with the offsets of their fields"""
    tensors, err = br.parse(blob, len(blob))
    assert err is None, err
    out, off = [], 12
    for name, dt, dims, nb, data_off in tensors:
        ln = len(name.encode("latin-1"))
        out.append(Record(name, dt, dims, nb, off, off + 2 + ln + 2, off + 2 + ln + 2 + 4 * len(dims), data_off))
        off = data_off + nb
    return out


def header(name, dtype, dims, nbytes, at):
    """a tensor record's header as it stands at file offset `at`, padding included"""
    nb = name.encode("latin-1")
    h = struct.pack("<H", len(nb)) + nb + struct.pack("<BB", dtype, len(dims)) + struct.pack("<%dI" % len(dims), *dims) + struct.pack("<Q", nbytes)
    return h + b"\x00" * ((-(at + len(h))) % 16)


def count_patch(blob, delta):
    (cnt,) = struct.unpack_from("<I", blob, 8)
    return (8, struct.pack("<I", cnt + delta))


def rename_patch(r):
    return (r.hdr_off + 2, b"~")   # (the first character: "x.w" and "x.b" must not become the same name)


def appended(blob, pieces):
    """tail for the tensors `pieces` = [(name, dtype, dims)] appended after the base, with zero data that fits their dims"""
    tail, at = [], len(blob)
    for name, dtype, dims in pieces:
        count = int(np.prod([int(d) for d in dims], dtype=object)) if dims else 1
        nbytes = count * br.ELEM[dtype]
        h = header(name, dtype, dims, nbytes, at)
        tail.append((h, nbytes))
        at += len(h) + nbytes
    return tail


def replaced(blob, r, label, dtype, dims):
    """the tensor of record r says (dtype, dims) instead, in a well-formed container"""
    return M(f"{r.name}:{label}", r.name, [rename_patch(r), count_patch(blob, 1)], appended(blob, [(r.name, dtype, dims)]))


def tensor_mutants(blob, r):
    out = [M(f"{r.name}:missing", r.name, [rename_patch(r)])]
    out.append(replaced(blob, r, "dtype", 1 - r.dtype, r.dims))
    out.append(replaced(blob, r, "rank-1", r.dtype, r.dims[:-1]))          # (rank 0 for a vector: the parser's to refuse)
    out.append(replaced(blob, r, "rank+1", r.dtype, r.dims + (1,)))        # (rank 5 for a conv weight: the parser's to refuse)
    for d, v in enumerate(r.dims):
        for label, nv in ((f"dim{d}-1", v - 1), (f"dim{d}+1", v + 1), (f"dim{d}=0", 0)):
            if label.endswith("-1") and nv == 0:
                continue   # the "=0" mutant
            out.append(replaced(blob, r, label, r.dtype, r.dims[:d] + (nv,) + r.dims[d + 1:]))
    if len(r.dims) == 4:
        torch_dims = tuple(r.dims[i] for i in TORCH)
        if torch_dims != r.dims:
            out.append(replaced(blob, r, "torch-layout", r.dtype, torch_dims))
    e = br.ELEM[r.dtype]
    out.append(M(f"{r.name}:nbytes-short", r.name, [(r.nbytes_off, struct.pack("<Q", r.nbytes - e))]))
    out.append(M(f"{r.name}:nbytes-long", r.name, [(r.nbytes_off, struct.pack("<Q", r.nbytes + e))]))
    out.append(M(f"{r.name}:duplicate", r.name, [count_patch(blob, 1)], appended(blob, [(r.name, r.dtype, r.dims)])))
    return out


def field_boundaries(r):
    ln = len(r.name.encode("latin-1"))
    b = [r.hdr_off, r.hdr_off + 2, r.hdr_off + 2 + ln, r.hdr_off + 2 + ln + 1, r.dims_off]
    b += [r.dims_off + 4 * (d + 1) for d in range(len(r.dims))]
    b += [r.nbytes_off + 8, r.data_off]
    return sorted(set(b))


def blob_mutants(kind, blob, recs):
    first, last = recs[0], recs[-1]
    out = [M("intact"), M("odd-address", odd=True)]
    out.append(M("bad-magic", "", [(0, b"K")]))
    out.append(M("version-2", "", [(4, struct.pack("<I", 2))]))
    out.append(M("count+1", "", [count_patch(blob, 1)]))
    out.append(M("count-ffffffff", "", [(8, b"\xff\xff\xff\xff")]))
    out.append(M("name_len-past-end", "", [(last.hdr_off, b"\xff\xff")]))   # (of the last tensor; no name can be given)
    ndim_off = first.dims_off - 1
    out.append(M("ndim-0", first.name, [(ndim_off, b"\x00")]))
    out.append(M("ndim-5", first.name, [(ndim_off, b"\x05")]))
    out.append(M("dim-2^28+1", first.name, [(first.dims_off, struct.pack("<I", 2 ** 28 + 1))]))
    out.append(M("nbytes-2^64-8", first.name, [(first.nbytes_off, struct.pack("<Q", 2 ** 64 - 8))]))
    cut = [first, last] + recs[10::10]
    for r in cut:
        for b in field_boundaries(r):
            out.append(M(f"trunc@{b}:{r.name}", r.name, trunc=b))
    out.append(M("trunc-mid-last-data", last.name, trunc=last.data_off + last.nbytes // 2))
    out.append(M("extra-tensor", "", [count_patch(blob, 1)], appended(blob, [("unknown.w", 1, (3, 5))])))
    out.append(M("trailing-bytes", "", tail=[(b"\x00" * 16, 0)]))
    head = br.CTC_HEADS.get(kind)
    if head:
        w, b = [r for r in recs if r.name == head + ".w"][0], [r for r in recs if r.name == head + ".b"][0]
        for c in (1, br.CTC_MAX_CLASSES + 1):
            out.append(M(f"classes={c}", head + ".w", [rename_patch(w), rename_patch(b), count_patch(blob, 2)],
                         appended(blob, [(w.name, w.dtype, (c,) + w.dims[1:]), (b.name, b.dtype, (c,))])))
    cfg = [r for r in recs if r.name == "svtr.config"]
    if cfg:
        for slot in range(12):
            for label, v in (("nan", np.nan), ("inf", np.inf), ("-1", -1.0), ("1e30", 1e30), ("64.5", 64.5)):
                out.append(M(f"svtr.config[{slot}]={label}", "svtr.config", [(cfg[0].data_off + 4 * slot, struct.pack("<f", v))]))
    return out


ACCEPTED = ("intact", "odd-address", "extra-tensor")   # + svtr.config missing from a Tiny blob (the variant it stands for by default)


def base_blobs():
    """(name, kind, weights): every generator's intact blob.  per_tensor: the blobs that get the per-tensor mutants (the fp16 SVTR
    blobs differ from the bf16 ones in one svtr.config value only)"""
    return [("det", "det", br.generator_weights("det"), True), ("rec", "rec", br.generator_weights("rec"), True),
            ("cls", "cls", br.generator_weights("cls"), True), ("svtr-tiny-bf16", "svtr", br.generator_weights("svtr", "tiny", "bf16"), True),
            ("svtr-tiny-f16", "svtr", br.generator_weights("svtr", "tiny", "f16"), False),
            ("svtr-base-bf16", "svtr", br.generator_weights("svtr", "base", "bf16"), True),
            ("svtr-base-f16", "svtr", br.generator_weights("svtr", "base", "f16"), False)]


def corpus(kind, blob, per_tensor=True):
    recs = records(blob)
    out = blob_mutants(kind, blob, recs)
    if per_tensor:
        for r in recs:
            out += tensor_mutants(blob, r)
    return out


def serialise(mutants) -> bytes:
    """the recipe file tests/blob_main.cpp reads"""
    out = bytearray(struct.pack("<I", len(mutants)))
    for m in mutants:
        lb = m.label.encode("latin-1")
        out += struct.pack("<H", len(lb)) + lb + struct.pack("<Bq", int(m.odd), -1 if m.trunc is None else m.trunc)
        out += struct.pack("<I", len(m.patches))
        for off, data in m.patches:
            out += struct.pack("<QI", off, len(data)) + data
        out += struct.pack("<I", len(m.tail))
        for data, zeros in m.tail:
            out += struct.pack("<IQ", len(data), zeros) + data
    return bytes(out)


class Workbench:
    """a working copy of the base blob that takes one mutant at a time (the restatement's side of the recipe)"""

    def __init__(self, blob):
        self.work, self.n = bytearray(blob), len(blob)

    def check(self, kind, m):
        undo = [(off, bytes(self.work[off:off + len(data)])) for off, data in m.patches]
        try:
            for off, data in m.patches:
                self.work[off:off + len(data)] = data
            for data, zeros in m.tail:
                self.work += data
                self.work += bytes(zeros)
            n = len(self.work) if m.trunc is None else m.trunc
            return br.check(kind, self.work, n)
        finally:
            del self.work[self.n:]
            for off, data in undo:
                self.work[off:off + len(data)] = data


# ---- complete blobs with real data (GPU loads) ----
def entries_of(weights):
    """[(name, dtype, dims, data bytes)] as write_blob stores them"""
    out = []
    for name, a in weights.items():
        dt = br.storage_dtype(name)
        data = arch.f32_to_bf16_bits(a).tobytes() if dt else np.ascontiguousarray(a, np.float32).tobytes()
        out.append((name, dt, tuple(int(v) for v in a.shape), data))
    return out


def full_blob(entries) -> bytes:
    out = bytearray(b"LOCW" + struct.pack("<II", 1, len(entries)))
    for name, dt, dims, data in entries:
        out += header(name, dt, dims, len(data), len(out))
        out += data
    return bytes(out)


def _with(entries, name, fn):
    assert any(e[0] == name for e in entries), name
    return [fn(e) if e[0] == name else e for e in entries]


def _fit(data, dtype, dims):
    """the tensor's own values, as many as (dtype, dims) take: cut, or repeated"""
    need = int(np.prod(dims)) * br.ELEM[dtype]
    return (data * (need // len(data) + 1))[:need]


def reshaped(entries, name, dims):
    return _with(entries, name, lambda e: (e[0], e[1], tuple(dims), _fit(e[3], e[1], dims)))


def retyped(entries, name):
    def fn(e):
        if e[1] == 1:
            data = arch.bf16_bits_to_f32(np.frombuffer(e[3], np.uint16)).astype(np.float32).tobytes()
        else:
            data = arch.f32_to_bf16_bits(np.frombuffer(e[3], np.float32)).tobytes()
        return (e[0], 1 - e[1], e[2], data)
    return _with(entries, name, fn)


def dims_of(entries, name):
    return [e[2] for e in entries if e[0] == name][0]


def gpu_mutants(kind, weights):
    """[(label, tensor the refusal must name (a tuple: any of them), blob)]: one mutant of each refusal class that `kind` has, with
    model data throughout, so that a loader that had got as far as uploading would change the outputs"""
    E = entries_of(weights)
    conv3 = {"det": "s1.b0.conv1.w", "rec": "rec.conv1.w", "cls": "cls.conv1.w", "svtr": "svtr.pe2.w"}[kind]
    any_w = {"det": "fpn.in3.w", "rec": "rec.b4.project.w", "cls": "cls.b4.project.w", "svtr": "svtr.b3.fc1.w"}[kind]
    any_b = any_w[:-2] + ".b"
    out = [("missing", (any_w,), full_blob([e for e in E if e[0] != any_w])),
           ("dtype", (any_w,), full_blob(retyped(E, any_w))),
           ("rank", (any_w,), full_blob(reshaped(E, any_w, dims_of(E, any_w)[:-1]))),
           ("conv3x3-dims2", (conv3,), full_blob(reshaped(E, conv3, dims_of(E, conv3)[:2] + (1,) + dims_of(E, conv3)[3:]))),
           ("short-bias", (any_b,), full_blob(reshaped(E, any_b, (dims_of(E, any_b)[0] - 1,)))),
           ("duplicate", (any_w,), full_blob(E + [e for e in E if e[0] == any_w])),
           ("truncated", (E[-1][0],), full_blob(E)[:-max(1, len(E[-1][3]) // 2)])]   # (in the middle of the last tensor's data)
    if kind in ("rec", "cls"):
        dw, se = f"{kind}.b3.dw.w", f"{kind}.b3.se1.w"
        out.append(("torch-depthwise", (dw,), full_blob(reshaped(E, dw, tuple(dims_of(E, dw)[i] for i in TORCH)))))
        out.append(("torch-squeeze-excite", (se,), full_blob(reshaped(E, se, tuple(dims_of(E, se)[i] for i in TORCH)))))
    if kind == "rec":
        for label, name in (("short-bw-w_ih", "lstm.l0.bw.w_ih"), ("short-w_hh", "lstm.l1.bw.w_hh"), ("short-fw-w_hh", "lstm.l0.fw.w_hh")):
            d = dims_of(E, name)
            out.append((label, (name,), full_blob(reshaped(E, name, (d[0] - 1, d[1])))))
    if kind in br.CTC_HEADS:
        b = br.CTC_HEADS[kind] + ".b"
        out.append(("bf16-ctc-bias", (b,), full_blob(retyped(E, b))))
    return out
