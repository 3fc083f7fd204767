"""Build check of the pooled stem.conv3 kernel, conv_ring_kernel<0,false,true,4> (ocr-system_amd/csrc/conv_ring.hip): compiles conv_ring.hip
to gfx950 assembly with the Makefile's flags and
  * fails if the pooled instantiation uses scratch, more than 256 VGPRs or more than 81,920 B of LDS (two work-groups per CU rest on all
    three; the LDS size is the launch's dynamic size, read from the source's R_LDS constants, plus the kernel's static group segment);
  * prints the static instruction counts of its tile loop — from the loop's first `s_waitcnt vmcnt(0)` (the kernel's own inline asm,
    marked ;;#ASMSTART) to the end of the kernel, the final store included: vector, scalar, MFMA, LDS, vector-memory, barriers, branches;
  * with --against <other conv_ring.hip> reports whether the bodies of the non-pooled instantiations are identical in both sources.
Run after a compiler update or an edit of the kernel:  python tools/stem_pool_isa_check.py [--against FILE] [SOURCE]  (needs hipcc, no GPU)."""
import argparse
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ocr-system_amd" / "csrc"
SRC = CSRC / "conv_ring.hip"
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC"]
POOLED = "conv_ring_kernel<0,false,true,4>"
MAX_VGPRS, MAX_LDS = 256, 81920
SYM = re.compile(r"^(_ZN\S*conv_ring_kernelILi(\d)ELb(\d)ELb(\d)ELi(\d)EE\S*):")


def compile_asm(src: Path) -> str:
    with tempfile.TemporaryDirectory() as tmp:
        out = Path(tmp) / "conv_ring.s"
        subprocess.check_call(["/opt/rocm/bin/hipcc", *FLAGS, "-I", str(CSRC), "-I", str(ROOT / "include"), "-Wno-unused-command-line-argument",
                               "--cuda-device-only", "-S", str(src), "-o", str(out)])
        return out.read_text()


def kernels(asm: str):
    """-> {instantiation: (symbol, instruction lines of its body)}"""
    out, cur = {}, None
    for line in asm.splitlines():
        m = SYM.match(line)
        if m:
            name = "conv_ring_kernel<%s,%s,%s,%s>" % (m.group(2), "true" if m.group(3) == "1" else "false", "true" if m.group(4) == "1" else "false", m.group(5))
            cur = out.setdefault(name, (m.group(1), []))[1]
            continue
        if cur is not None:
            cur.append(line)
            if "s_endpgm" in line:
                cur = None
    return out


def instructions(body):
    """instruction lines only, comments and labels dropped, local label numbers blanked (they differ with the position in the file)"""
    out = []
    for line in body:
        t = line.split(";")[0].strip() if "#ASM" not in line else line.strip()
        if not t or t.endswith(":") or t.startswith("."):
            continue
        out.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def metadata(asm: str, symbol: str):
    """the kernel's entry of amdhsa.kernels (the entries begin with `- .agpr_count:` or `- .args:`)"""
    for entry in re.split(r"\n\s+- \.", asm[asm.find("amdhsa.kernels:"):]):
        if re.search(r"\.name:\s+%s\n" % re.escape(symbol), entry):
            return "." + entry
    return None


def field(meta: str, key: str) -> int:
    return int(re.search(r"\.%s:\s+(\d+)" % key, meta).group(1))


def dynamic_lds(src: Path) -> int:
    """R_LDS as the source spells it: 2 * (halo rounds of 256 pieces + weight slab) + bias area"""
    text = src.read_text()
    hh, hw, bn = (int(re.search(r"\b%s = (\d+)" % k, text).group(1)) for k in ("R_HH", "R_HW", "R_BN"))
    bias = int(re.search(r"R_BIAS_BYTES = (\d+)", text).group(1))
    a_bytes = (hh * hw * 2 + 255) // 256 * 256 * 16
    return 2 * (a_bytes + 9 * bn * 2 * 16) + bias


def loop_counts(body):
    ins = instructions(body)
    # the tile loop begins with the kernel's own vmcnt(0) (other inline asm of the kernel is empty: register constraints only)
    start = next(i for i, t in enumerate(ins[:-1]) if "#ASMSTART" in t and ins[i + 1].startswith("s_waitcnt"))
    c = dict.fromkeys(["vector", "scalar", "mfma", "lds", "vmem", "barriers", "branches", "waitcnt"], 0)
    for t in ins[start:]:
        op = t.split()[0]
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith("v_"):
            c["vector"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            c["vmem"] += 1
        elif op == "s_barrier":
            c["barriers"] += 1
        elif op.startswith(("s_cbranch", "s_branch")):
            c["branches"] += 1
        elif op == "s_waitcnt":
            c["waitcnt"] += 1
        elif op.startswith("s_") and op not in ("s_nop", "s_endpgm"):
            c["scalar"] += 1
    return c


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("source", nargs="?", default=str(SRC))
    ap.add_argument("--against", help="another conv_ring.hip: are the non-pooled instantiations' bodies identical?")
    args = ap.parse_args()
    src = Path(args.source)
    asm = compile_asm(src)
    found = kernels(asm)
    errors = []
    if POOLED not in found:
        errors.append("no %s among %s" % (POOLED, sorted(found)))
    else:
        symbol, body = found[POOLED]
        meta = metadata(asm, symbol)
        if meta is None:
            errors.append("%s: no metadata" % POOLED)
        else:
            vgprs, scratch = field(meta, "vgpr_count"), field(meta, "private_segment_fixed_size")
            lds = field(meta, "group_segment_fixed_size") + dynamic_lds(src)
            spills = field(meta, "sgpr_spill_count") if ".sgpr_spill_count" in meta else 0
            print("%s: %d VGPRs, %d B scratch, %d B LDS, %d SGPR spills" % (POOLED, vgprs, scratch, lds, spills))
            if scratch:
                errors.append("%s: %d bytes of scratch" % (POOLED, scratch))
            if vgprs > MAX_VGPRS:
                errors.append("%s: %d VGPRs (> %d)" % (POOLED, vgprs, MAX_VGPRS))
            if lds > MAX_LDS:
                errors.append("%s: %d B of LDS (> %d)" % (POOLED, lds, MAX_LDS))
        c = loop_counts(body)
        print("tile loop (static): " + "  ".join("%s %d" % kv for kv in c.items()) + "  | vector per MFMA %.2f" % (c["vector"] / max(1, c["mfma"])))
    if args.against:
        other = kernels(compile_asm(Path(args.against)))
        for name in sorted(set(found) | set(other)):
            if name.split(",")[2] == "true":       # pooled (the profiling build of it included)
                continue
            if name not in found or name not in other:
                print("%s: only in %s" % (name, "this source" if name in found else "the other source"))
                errors.append("%s: missing on one side" % name)
                continue
            a, b = instructions(found[name][1]), instructions(other[name][1])
            same = a == b
            print("%s: %d instructions, %s" % (name, len(a), "identical" if same else "DIFFERENT (%d in the other source)" % len(b)))
            if not same:
                errors.append("%s: body differs from %s" % (name, args.against))
    for e in errors:
        print("FAIL", e)
    return 1 if errors else 0


if __name__ == "__main__":
    sys.exit(main())
