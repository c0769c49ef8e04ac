"""Per-picture quality statistic (kernels/quality_pic.h, WelsHipGetFrameQuality / WelsHipGroupGetFrameQuality) on the CPU wave-emulation
build of the same kernel sources.

For every case of golden.json: the stream is unchanged with the statistic on, the sum of squared differences of each plane is what numpy
computes from the reconstruction (a cropped picture: at least that of its visible part -- the reference measures the macroblock-aligned
picture), and the PSNR is the float the reference reports (tests/golden/psnr.json,
tools/make_psnr_golden.py) bit for bit.  Then the plane selection, and session groups -- synchronous and pipelined -- against sessions
alone.  The GPU twin is tests/test_quality_stats_gpu.py (it reuses the helpers here).
"""
import hashlib
import json
import os
import struct

import numpy as np
import pytest

import openh264_amd as oh
from openh264_amd.utils.synth import make_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "golden.json")))
PSNR = json.load(open(os.path.join(ROOT, "tests", "golden", "psnr.json")))


def f32_hex(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", x))[0]


def plane_sse(src, rec, w, h):
    """numpy's sum of squared differences of the three planes of two I420 pictures of w x h (the visible picture)."""
    s = np.frombuffer(src, np.uint8).astype(np.int64)
    r = np.frombuffer(rec, np.uint8).astype(np.int64)
    y, c = w * h, (w // 2) * (h // 2)
    return [int(((s[a:b] - r[a:b]) ** 2).sum()) for a, b in ((0, y), (y, y + c), (y + c, y + 2 * c))]


def make_param(enc, w, h, params, planes=0):
    p = enc.GetDefaultParams()
    p.iPicWidth, p.iPicHeight = w, h
    full = dict(fMaxFrameRate=30.0, iTargetBitrate=5000000)
    full.update(params)
    for k, v in full.items():
        if isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                p.uiSliceMbNum[i] = x
        else:
            setattr(p, k, v)
    p.bPsnrY, p.bPsnrU, p.bPsnrV = planes & 1, (planes >> 1) & 1, (planes >> 2) & 1
    return p


def check_case(name, lib_path):
    """Every picture of a golden case with all planes requested: stream, SSE against numpy, PSNR against the reference's."""
    g = GOLDEN[name]
    w, h, n = g["w"], g["h"], g["frames"]
    yuv = make_sequence(g.get("content", "synth"), w, h, n)
    enc = oh.Encoder(lib_path)
    assert enc.InitializeExt(make_param(enc, w, h, g["params"], planes=7)) == 0, enc.last_error()
    fsz = w * h * 3 // 2
    bs = bytearray()
    for i in range(n):
        src = yuv[i * fsz:(i + 1) * fsz]
        rc, _, b, _ = enc.EncodeFrame(src)
        assert rc == 0, enc.last_error()
        bs += b
        sse, psnr = enc.frame_quality()
        visible = plane_sse(src, enc.GetReconFrame(), w, h)
        if w % 16 == 0 and h % 16 == 0:
            assert sse == visible, "%s picture %d" % (name, i)
        else:       # the reference measures the macroblock-aligned picture: the padding adds to the visible part
            assert all(a >= b for a, b in zip(sse, visible)), "%s picture %d" % (name, i)
        assert [f32_hex(x) for x in psnr] == PSNR[name]["rPsnr"][i], "%s picture %d: %r" % (name, i, psnr)
    assert hashlib.sha1(bytes(bs)).hexdigest() == g["sha1"], "the stream changed with the statistic on"
    if name.endswith("_overflow"):          # the re-encode path: the figures are those of the final reconstruction
        assert enc.overflow_reencodes() > 0
    enc.close()


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_quality_matches_numpy_and_reference(name, emu_lib):
    check_case(name, emu_lib)


def test_psnr_fixture_covers_golden():
    assert sorted(PSNR) == sorted(GOLDEN)
    for name, g in GOLDEN.items():
        assert len(PSNR[name]["rPsnr"]) == g["frames"]


def test_planes_not_requested_report_zero(emu_lib):
    g = GOLDEN["p_152x100_qp24_crop"]
    w, h, n = g["w"], g["h"], g["frames"]
    yuv = make_sequence("synth", w, h, n)
    fsz = w * h * 3 // 2
    # nothing requested: no "quality" key, the getter reports nothing measured
    stats = {}
    bs, _ = oh.encode_sequence(yuv, w, h, lib_path=emu_lib, stats=stats, **dict(g["params"], fMaxFrameRate=30.0, iTargetBitrate=5000000))
    assert "quality" not in stats and hashlib.sha1(bs).hexdigest() == g["sha1"]
    # the option asks for U, from picture 2 on for Y instead; the parameters ask for V throughout
    stats = {}
    bs, _ = oh.encode_sequence(yuv, w, h, lib_path=emu_lib, stats=stats, options_at=[(0, oh.OPTION_PSNR_PLANES, 2), (2, oh.OPTION_PSNR_PLANES, 1)],
                               **dict(g["params"], fMaxFrameRate=30.0, iTargetBitrate=5000000, bPsnrV=1))
    assert hashlib.sha1(bs).hexdigest() == g["sha1"]
    q = stats["quality"]
    assert len(q) == n
    for i, (sse, psnr) in enumerate(q):
        want = [True, False, True] if i >= 2 else [False, True, True]
        for k in range(3):
            hexes = PSNR["p_152x100_qp24_crop"]["rPsnr"][i][k]
            if want[k]:
                assert sse[k] > 0 and f32_hex(psnr[k]) == hexes
            else:
                assert sse[k] == 0 and psnr[k] == 0.0
    # the getter and the option's own value
    enc = oh.Encoder(emu_lib)
    assert enc.InitializeExt(make_param(enc, w, h, g["params"])) == 0
    with pytest.raises(oh.WelsHipError):
        enc.frame_quality()                                     # before the first picture
    assert enc.SetOption(oh.OPTION_PSNR_PLANES, 5) == 0 and enc.GetOption(oh.OPTION_PSNR_PLANES) == (0, 5)
    assert enc.SetOption(oh.OPTION_PSNR_PLANES, 8) == oh.cmInitParaError
    assert enc.EncodeFrame(yuv[:fsz])[0] == 0
    sse, psnr = enc.frame_quality()
    assert sse[1] == 0 and psnr[1] == 0.0 and sse[0] > 0 and sse[2] > 0
    assert enc.SetOption(oh.OPTION_PSNR_PLANES, 0) == 0 and enc.EncodeFrame(yuv[fsz:2 * fsz])[0] == 0
    assert enc.frame_quality() == ([0, 0, 0], [0.0, 0.0, 0.0])
    enc.close()


# ---- session groups -----------------------------------------------------------------------------------------------------------------------
# Low QP on saturated checkerboards: some pictures overflow CAVLC and are coded again (the synchronous group in GroupFinish, the pipelined
# one after later steps have already been submitted) -- the figures must be those of the final reconstructions.
GROUP_CASE = dict(w=64, h=64, frames=5, params=dict(iDLayerQp=3, uiIntraPeriod=0), contents=["checker5", "synth", "checker8", "synth+2"])


def content(name, w, h, n):
    """make_sequence content; "<content>+k": the same sequence from its picture k on."""
    base, _, skip = name.partition("+")
    k = int(skip or 0)
    return make_sequence(base, w, h, n + k)[k * (w * h * 3 // 2):]


def session_alone(lib_path, w, h, params, yuv, frames):
    enc = oh.Encoder(lib_path)
    assert enc.InitializeExt(make_param(enc, w, h, params, planes=7)) == 0
    fsz = w * h * 3 // 2
    q, bs = [], []
    for i in range(frames):
        rc, _, b, _ = enc.EncodeFrame(yuv[i * fsz:(i + 1) * fsz])
        assert rc == 0, enc.last_error()
        q.append(enc.frame_quality())
        bs.append(b)
    reenc = enc.overflow_reencodes()
    enc.close()
    return q, bs, reenc


def group_run(lib_path, w, h, params, yuvs, frames, ahead, planes=7):
    """Per step: the list of (sse, psnr) of every session and the sessions' bitstreams of that step."""
    probe = oh.Encoder(lib_path)
    param = make_param(probe, w, h, params, planes=planes)
    probe.close()
    n = len(yuvs)
    g = oh.EncoderGroup(param, n, ring_slots=2, host_threads=2, lib_path=lib_path)
    fsz = w * h * 3 // 2
    steps = []
    if ahead:
        g.set_pipelined(ahead)
    for i in range(frames):
        pics = g.make_pictures([y[i * fsz:(i + 1) * fsz] for y in yuvs])
        if ahead:
            out = g.encode_frames_pipelined(pics, want_bytes=True)
            if out is not None:
                steps.append((g.frame_quality() if planes else None, out))
        else:
            out = g.encode_frames(pics, want_bytes=True)
            steps.append((g.frame_quality() if planes else None, out))
    while ahead:
        out = g.encode_frames_pipelined(None, want_bytes=True)
        if out is None:
            break
        steps.append((g.frame_quality() if planes else None, out))
    g.close()
    assert len(steps) == frames
    return steps


def check_group(lib_path, case, aheads):
    w, h, n = case["w"], case["h"], case["frames"]
    yuvs = [content(c, w, h, n) for c in case["contents"]]
    alone = [session_alone(lib_path, w, h, case["params"], y, n) for y in yuvs]
    if "overflow" in case:
        assert sum(a[2] for a in alone) > 0, "no session went through the re-encode path"
    for ahead in aheads:
        steps = group_run(lib_path, w, h, case["params"], yuvs, n, ahead)
        for i, (q, bs) in enumerate(steps):
            for s in range(len(yuvs)):
                assert bs[s] == alone[s][1][i], "ahead %d step %d session %d: stream" % (ahead, i, s)
                assert q[s] == alone[s][0][i], "ahead %d step %d session %d: %r vs %r" % (ahead, i, s, q[s], alone[s][0][i])


def test_group_quality_matches_sessions_alone(emu_lib):
    check_group(emu_lib, dict(GROUP_CASE, overflow=True), aheads=(0, 1, 2, 3))


def test_group_without_quality_getter_refuses(emu_lib):
    probe = oh.Encoder(emu_lib)
    param = make_param(probe, 64, 64, GROUP_CASE["params"])
    probe.close()
    g = oh.EncoderGroup(param, 2, lib_path=emu_lib)
    with pytest.raises(oh.WelsHipError):
        g.frame_quality()                                       # before the first step
    g.close()
