"""The per-picture quality statistic on the MI355X (libwelship.so): the checks of tests/test_quality_stats.py for every golden case, a
group of 16 four-slice 1080p sessions (synchronous and pipelined) against the same sessions alone, and the new kernel's resources (read
from the library: that one runs in both tiers).
Reads only tests/golden/*.json and the generated content."""
import os
import re
import shutil
import subprocess

import pytest

from openh264_amd.utils.synth import synth_sequence
from test_quality_stats import GOLDEN, check_case, group_run, session_alone

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_quality_matches_numpy_and_reference_gpu(name, hip_lib):
    check_case(name, hip_lib)


@pytest.mark.gpu
def test_group_1080p_quality_matches_sessions_alone_gpu(hip_lib):
    w, h, n, sessions = 1920, 1080, 3, 16
    params = dict(iDLayerQp=24, uiIntraPeriod=0, uiSliceMode=1, uiSliceNum=4)
    fsz = w * h * 3 // 2
    seq = synth_sequence(w, h, n + 7)
    yuvs = [seq[(s % 8) * fsz:(s % 8 + n) * fsz] for s in range(sessions)]      # every session its own stretch of the motion
    alone = {}
    for s in range(8):
        alone[s] = session_alone(hip_lib, w, h, params, yuvs[s], n)
    off = group_run(hip_lib, w, h, params, yuvs, n, 0, planes=0)
    for ahead in (0, 2):
        steps = group_run(hip_lib, w, h, params, yuvs, n, ahead)
        for i, (q, bs) in enumerate(steps):
            for s in range(sessions):
                assert bs[s] == off[i][1][s] == alone[s % 8][1][i], "ahead %d step %d session %d: stream" % (ahead, i, s)
                assert q[s] == alone[s % 8][0][i], "ahead %d step %d session %d: %r vs %r" % (ahead, i, s, q[s], alone[s % 8][0][i])


def test_quality_kernel_does_not_spill(hip_lib):
    """k_sse keeps its registers: no scratch memory, no spilled VGPR (read from the code object's notes, as tests/test_abi.py does for the
    mode-decision kernels; needs no device)."""
    tool = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(tool) or not shutil.which("bash"):
        pytest.skip("ROCm LLVM tools not available")
    out = subprocess.check_output(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), hip_lib]).decode()
    rows = [l for l in out.splitlines() if re.search(r"\.name:\s+k_sse\b", l)]
    assert rows, "k_sse not found in the library"
    for l in rows:
        m = re.search(r"\.private_segment_fixed_size:\s+(\d+)", l)
        scratch, spills = int(m.group(1)) if m else 0, int(re.search(r"\.vgpr_spill_count:\s+(\d+)", l).group(1))
        assert scratch == 0 and spills == 0, "k_sse: %d bytes of scratch, %d spilled VGPRs" % (scratch, spills)
