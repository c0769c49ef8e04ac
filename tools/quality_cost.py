#!/usr/bin/env python3
"""What the per-picture quality statistic costs a session group (GPU): 256 four-slice 1080p sessions on bench.py's default content,
device-only P steps (WelsHipGroupBench) with the statistic off and with all three planes on, alternating within one process, and the
extra bytes a step copies back.  One JSON line.

    python tools/quality_cost.py [--sessions 256] [--steps 20] [--rounds 3]

The pass's own kernel time comes from a separate profiler run of the same script (no PMC counters):
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/quality_cost.py --rounds 1
k_sse's mean duration there against the bytes printed here (`sse_pass_bytes_per_step`) is its achieved bandwidth."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--qp", type=int, default=24)
    a = ap.parse_args()
    import openh264_amd as oh
    from openh264_amd.utils.synth import synth_sequence
    w, h, ring = 1920, 1080, 2
    fsz = w * h * 3 // 2
    seq = synth_sequence(w, h, 2 * ring)            # bench.py's synthetic content: session s takes frames (3 s) % (n - ring + 1) + slot

    def frame(s, slot):
        k = (s * 3) % (2 * ring - ring + 1) + slot
        return seq[k * fsz:(k + 1) * fsz]

    def group(planes):
        e = oh.Encoder()
        p = e.GetDefaultParams()
        e.close()
        p.iPicWidth, p.iPicHeight, p.iDLayerQp, p.fMaxFrameRate, p.iTargetBitrate = w, h, a.qp, 30.0, 5000000
        p.uiIntraPeriod, p.uiSliceMode, p.uiSliceNum = 0, 1, 4
        p.bPsnrY, p.bPsnrU, p.bPsnrV = planes & 1, (planes >> 1) & 1, (planes >> 2) & 1
        g = oh.EncoderGroup(p, a.sessions, ring_slots=ring)
        for s in range(a.sessions):
            for slot in range(ring):
                g.upload(s, slot, frame(s, slot))
        g.bench(1, 0)                                # the IDR
        g.bench(a.warmup, 0)
        return g

    groups = {0: group(0), 7: group(7)}
    res = {0: [], 7: []}
    for _ in range(a.rounds):
        for planes in (0, 7):
            ev = groups[planes].bench(a.steps, 0)
            res[planes].append(ev["total_ms"] / a.steps)
    for g in groups.values():
        g.close()
    mb_w, mb_h = (w + 15) // 16, (h + 15) // 16
    pass_bytes = a.sessions * (mb_w * mb_h * 384 + (mb_w * 16) * (mb_h * 16) * 3 // 2)     # tiled source + planar reconstruction, read once
    off, on = min(res[0]), min(res[7])
    print(json.dumps(dict(sessions=a.sessions, size="%dx%d" % (w, h), slices=4, steps=a.steps, rounds=a.rounds,
                          step_ms_psnr_off=[round(x, 4) for x in res[0]], step_ms_psnr_on=[round(x, 4) for x in res[7]],
                          ratio_on_off=round(on / off, 4), extra_ms_per_step=round(on - off, 4),
                          extra_d2h_bytes_per_step=24 * a.sessions, sse_pass_bytes_per_step=pass_bytes,
                          sse_pass_gbs_if_extra_is_the_pass=round(pass_bytes / max(on - off, 1e-6) / 1e6, 1))))


if __name__ == "__main__":
    main()
