"""Build check of ctc_fc_argmax_kernel (ocr-system_amd/csrc/ops.hip): compiles ops.hip to gfx950 assembly with the Makefile's flags and
checks, for both instantiations, what the kernel's speed rests on and no test can see:
  * no scratch memory, at most 256 VGPRs (two waves per SIMD);
  * in every step, between the LDS-DMA requests of the next weight tile and the kernel's own `s_waitcnt vmcnt(0)` (the inline asm of
    `landed`, marked ;;#ASMSTART) the compiler has put NO vmcnt wait of its own.  hipcc puts one in front of an LDS read that it cannot
    tell from a pending LDS-DMA target (a float4 read of the bias ring gets one, the fragment-typed read does not); such a wait makes
    every tile wait for the weight tile just requested.  The prologue's first request, which is waited for at once, is exempt.
Run after a compiler update or an edit of the kernel:  python tools/ctc_head_isa_check.py  (needs hipcc, no GPU)."""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "ocr-system_amd" / "csrc" / "ops.hip"
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC"]


def kernels(asm: str):
    """-> {instantiation: lines of its body}"""
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_ZN\S*ctc_fc_argmax_kernelILi(\d)E\S*):", line)
        if m:
            cur = out.setdefault("ctc_fc_argmax_kernel<%s>" % m.group(2), [])
            continue
        if cur is not None:
            cur.append(line)
            if "s_endpgm" in line:
                cur = None
    return out


def check(name, body, meta):
    errors = []
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta).group(1))
    if scratch or vgprs > 256:
        errors.append("%s: %d VGPRs, %d bytes of scratch" % (name, vgprs, scratch))
    steps, pending, marked = 0, False, False
    for i, line in enumerate(body):
        if "global_load_lds" in line:
            pending = True
        elif "#ASMSTART" in line:
            marked = True
        elif "s_waitcnt" in line and "vmcnt" in line:
            if marked:                       # the kernel's own wait: the step ends here
                steps += pending
                pending = False
            elif pending and steps:          # (steps == 0: the prologue's first tile, waited for at once)
                errors.append("%s: compiler-inserted '%s' at line %d of the kernel, between a tile request and the end of its step" % (name, line.strip(), i))
            marked = False
    if steps < 4:
        errors.append("%s: only %d steps with a tile request found (expected the prologue, the loop's two and the tail)" % (name, steps))
    print("%s: %d VGPRs, %d B scratch, %d steps checked" % (name, vgprs, scratch, steps))
    return errors


def main():
    with tempfile.TemporaryDirectory() as tmp:
        out = Path(tmp) / "ops.s"
        src = Path(sys.argv[1]) if len(sys.argv) > 1 else SRC    # (another file: a variant of ops.hip in the same directory)
        subprocess.check_call(["/opt/rocm/bin/hipcc", *FLAGS, "-Wno-unused-command-line-argument", "--cuda-device-only", "-S", str(src), "-o", str(out)])
        asm = out.read_text()
    errors = []
    found = kernels(asm)
    if sorted(found) != ["ctc_fc_argmax_kernel<0>", "ctc_fc_argmax_kernel<1>"]:
        errors.append("instantiations found: %s" % sorted(found))
    for name, body in sorted(found.items()):
        sym = re.escape("ILi%sE" % name[-2])
        meta = re.search(r"\.name:\s+_ZN\S*ctc_fc_argmax_kernel%s\S*\n(?:.*\n)*?\s+\.wavefront_size" % sym, asm)
        errors += check(name, body, meta.group(0)) if meta else ["%s: no metadata" % name]
    for e in errors:
        print("FAIL", e)
    return 1 if errors else 0


if __name__ == "__main__":
    sys.exit(main())
