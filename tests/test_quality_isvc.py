"""SLayerBSInfo::rPsnr through the ISVCEncoder adapter (integration/welship_isvc.cpp) against the reference encoder: the same small API
program (tests/psnr_api_driver.cpp) linked once to the reference (oracle/_ref/libref_openh264.so) and once to the adapter over the CPU
wave-emulation build of this engine.  Per-picture flag patterns (SSourcePicture::bPsnrY / U / V) and the parameters' flags: every layer
entry's rPsnr must be bitwise equal, and so must the streams."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_psnr_golden as M  # noqa: E402
from openh264_amd.utils.synth import make_sequence  # noqa: E402
from test_quality_stats import GOLDEN  # noqa: E402

CASES = ["p_152x100_qp24_crop", "i_76x80_qp3_checker_overflow", "p_64x64_qp3_checker_idc1_overflow", "p_320x192_qp26_c1_rowslices_idc2",
         "p_320x192_qp20_c2_iper4", "p_176x144_qp28_20f_scene", "i_320x192_qp30_idc1"]
# (per-picture masks, cycled; the parameters' mask): all planes, none, only U, Y and V alternating, the parameters' flags only
PATTERNS = [("7", 0), ("0", 0), ("2", 0), ("1,4", 0), ("0", 7), ("2,0,5", 1)]


@pytest.fixture(scope="module")
def drivers(tmp_path_factory, emu_lib):
    if not M.have_reference():
        pytest.skip("needs the reference: oracle/_ref (make -C oracle) and the reference's API headers")
    d = tmp_path_factory.mktemp("psnr_drivers")
    return M.build_driver(str(d / "ref")), M.build_driver(str(d / "adapter"), adapter=True)


@pytest.mark.parametrize("name", CASES)
def test_adapter_rpsnr_equals_reference(name, drivers, emu_lib, tmp_path):
    ref, adapter = drivers
    g = GOLDEN[name]
    yuv = make_sequence(g.get("content", "synth"), g["w"], g["h"], g["frames"])
    env = dict(os.environ, WELSHIP_LIB=emu_lib)
    for pic, param in PATTERNS:
        bs_r, rows_r = M.run_driver(ref, g, yuv, str(tmp_path), pic=pic, param=param)
        bs_a, rows_a = M.run_driver(adapter, g, yuv, str(tmp_path), pic=pic, param=param, env=env)
        assert bs_a == bs_r, "%s -pic %s -param %d: streams differ" % (name, pic, param)
        assert rows_a == rows_r, "%s -pic %s -param %d: rPsnr differs" % (name, pic, param)
        if pic != "0":      # the pattern really reports something
            assert any(v != "00000000" for row in rows_r for v in row[3])
