#!/usr/bin/env python3
"""Generate tests/golden/psnr.json: the per-picture PSNR the *reference* reports (SLayerBSInfo::rPsnr of the picture's VCL layer entry,
codec/encoder/core/src/encoder_ext.cpp:3918-3970) for every case of tests/golden/golden.json, with all three planes requested per picture
(SSourcePicture::bPsnrY / U / V).  Each value is stored as the hexadecimal bit pattern of the float32, so that no JSON rounding can hide
a last-bit difference.  Run where /root/reference and oracle/_ref exist (the build machine; the reference does not travel):

    python tools/make_psnr_golden.py

The program that asks the reference is tests/psnr_api_driver.cpp, linked to oracle/_ref/libref_openh264.so (build_driver below; the
tests link the same program to the ISVCEncoder adapter of integration/welship_isvc.cpp)."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openh264_amd.utils.synth import make_sequence  # noqa: E402

REF = os.environ.get("WELSHIP_REFERENCE", "/root/reference")
REF_LIB_DIR = os.path.join(ROOT, "oracle", "_ref")
DRIVER_SRC = os.path.join(ROOT, "tests", "psnr_api_driver.cpp")


def have_reference():
    return os.path.exists(os.path.join(REF, "codec", "api", "wels", "codec_api.h")) and os.path.exists(os.path.join(REF_LIB_DIR, "libref_openh264.so"))


def build_driver(out, adapter=False):
    """tests/psnr_api_driver.cpp against the reference's API header, linked to the reference encoder or (adapter=True) to the
    ISVCEncoder adapter integration/welship_isvc.cpp, which opens $WELSHIP_LIB at run time."""
    inc = ["-I" + os.path.join(REF, "codec", "api", "wels")]
    if adapter:
        cmd = ["g++", "-O2", "-w"] + inc + [DRIVER_SRC, os.path.join(ROOT, "integration", "welship_isvc.cpp"), "-o", out, "-ldl", "-lpthread"]
    else:
        cmd = ["g++", "-O2", "-w"] + inc + [DRIVER_SRC, "-o", out, "-L" + REF_LIB_DIR, "-lref_openh264", "-lpthread", "-Wl,-rpath," + REF_LIB_DIR]
    subprocess.check_call(cmd)
    return out


def run_driver(exe, case, yuv, workdir, pic="7", param=0, env=None):
    """Encode `yuv` with the golden case's flags; returns (bitstream, [(picture, layer, layer type, (y, u, v) hex)])."""
    fi, fo = os.path.join(workdir, "in.yuv"), os.path.join(workdir, "out.264")
    with open(fi, "wb") as f:
        f.write(yuv)
    out = subprocess.check_output([exe, "-i", fi, "-w", str(case["w"]), "-h", str(case["h"]), "-o", fo] + case["ref_flags"]
                                  + ["-pic", pic, "-param", str(param)], env=env).decode()
    rows = []
    for line in out.splitlines():
        f = line.split()
        rows.append((int(f[0]), int(f[1]), int(f[2]), tuple(f[3:6])))
    with open(fo, "rb") as f:
        return f.read(), rows


def main():
    if not have_reference():
        sys.exit("needs %s and oracle/_ref/libref_openh264.so (make -C oracle)" % REF)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "golden.json")))
    out = {}
    with tempfile.TemporaryDirectory() as td:
        exe = build_driver(os.path.join(td, "psnr_ref"))
        for name in sorted(golden):
            g = golden[name]
            yuv = make_sequence(g.get("content", "synth"), g["w"], g["h"], g["frames"])
            assert hashlib.sha1(yuv).hexdigest() == g["input_sha1"]
            bs, rows = run_driver(exe, g, yuv, td)
            assert hashlib.sha1(bs).hexdigest() == g["sha1"], name + ": the driver's stream differs from the golden one"
            pics = [None] * g["frames"]
            for n, _, layer_type, vals in rows:
                if layer_type == 1:                     # VIDEO_CODING_LAYER
                    assert pics[n] is None
                    pics[n] = list(vals)
                else:
                    assert vals == ("00000000",) * 3, name + ": a non-VCL entry reports a PSNR"
            assert all(p is not None for p in pics)
            out[name] = {"rPsnr": pics}
            print(name, pics[-1])
    with open(os.path.join(ROOT, "tests", "golden", "psnr.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
