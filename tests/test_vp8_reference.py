"""CPU: the plain-Python restatement of the lossy-WebP decode (tests/vp8_reference.py) against Pillow.  It equals Pillow on every intact
case (none left out, none refused), refuses the refused kinds and the files just beyond the coefficient bound with their reasons, and
decides the damage sweep: every file it accepts is one Pillow reads, with Pillow's bytes; every file it refuses carries a reason from the
-1 / -2 lists; and it accepts exactly vc.SWEEP_ACCEPTED files, so a decoder that refuses too much fails."""
import numpy as np

import vp8_cases as vc
import vp8_reference as R
import webp_reference as wr


def test_equals_pillow_on_every_intact_case():
    cases = vc.intact_cases()
    assert len(cases) == len(vc.pillow_cases()) + len(vc.container_cases()) + len(vc.writer_cases()) >= 380
    for name, data in cases:
        rc, reason, px = R.decode(data)
        assert rc == 0 and reason == "", (name, rc, reason)
        assert np.array_equal(px, vc.pillow_rgb(data)), name


def test_refused_kinds_and_bound():
    got = {name: R.decode(data)[:2] for name, data, _ in vc.refused_cases() + vc.bound_cases()}
    assert got == {"lossy-alpha": (-2, "lossy WebP with an ALPH chunk"), "animated": (-2, "animated WebP"),
                   "inter-frame": (-1, "VP8 inter frame"), "show-frame-0": (-1, "VP8 show_frame is 0"),
                   "vp8-and-vp8l": (-1, "both a VP8 and a VP8L chunk"), "canvas-mismatch": (-1, "VP8X canvas differs from the VP8 frame header"),
                   "bound-block-beyond": (-1, R.R_BOUND), "bound-y2-beyond": (-1, R.R_BOUND)}


def test_decides_the_damage_sweep():
    accepted = {"flip": 0, "cut": 0}
    bad, reasons = [], {}
    container = set()
    for name, kind, data, rc, reason, px in vc.sweep_reference():
        if rc == 0:
            want = vc.pillow_rgb(data)
            if want is None or want.shape != px.shape or not np.array_equal(px, want):
                bad.append((name, "Pillow raises" if want is None else "pixels"))
            accepted[kind] += 1
            continue
        reasons[reason] = reasons.get(reason, 0) + 1
        if rc == -2:
            ok = reason in R.PROBE_REASONS_2
        else:
            ok = reason in R.PROBE_REASONS_1 or reason in R.DECODE_REASONS
            if not ok:   # the container cases of the lossless row: the lossless restatement's own reason for this file
                ok = reason != "" and wr.probe(data)[2] == reason
                container.add(reason)
        if not ok:
            bad.append((name, rc, reason))
    assert not bad, (len(bad), bad[:10])
    print("accepted:", accepted, "refusal reasons:", reasons)
    assert accepted == vc.SWEEP_ACCEPTED, accepted
    # the sweep reaches the decode-level reasons, not only the container's
    assert reasons.get(R.R_PAST_TOKEN, 0) > 0 and reasons.get(R.R_PAST_FIRST, 0) > 0 and reasons.get(R.R_FF, 0) > 0
