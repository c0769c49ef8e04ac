// psnr_api_driver.cpp -- TEST INFRASTRUCTURE: a small program over the reference's public encoder API (codec/api/wels/codec_api.h)
// that asks for the per-picture quality statistic and prints what every SLayerBSInfo entry reports in rPsnr.
//
// Linked either to the reference encoder (oracle/_ref/libref_openh264.so) or to integration/welship_isvc.cpp, the ISVCEncoder adapter
// over this repository's engine ($WELSHIP_LIB); tools/make_psnr_golden.py and tests/test_quality_isvc.py build it both ways.  The
// parameters are set the way oracle/ref_enc_driver.cpp sets them for the same options, so the streams equal the golden ones.
//
//   psnr_api_driver -i in.yuv -w W -h H -o out.264 [-fps F] [-rc M] [-qp Q] [-bitrate BPS] [-iper N] [-complexity C] [-slcmd M]
//                   [-slcnum N] [-slcmbnum N] [-deblock IDC] [-scene 0/1] [-spsid S] [-quiet]
//                   [-param MASK] [-pic MASK,MASK,...]
//
// -param: SEncParamExt::bPsnrY / U / V (bit 0 / 1 / 2); -pic: SSourcePicture::bPsnrY / U / V of picture k = entry k modulo the list.
// Prints one line per layer entry of every picture: "<picture> <layer> <uiLayerType> <rPsnr[0]> <rPsnr[1]> <rPsnr[2]>", the floats as
// the hexadecimal bit patterns of the float32 values.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "codec_api.h"

static unsigned bits_of (float f) { unsigned u; std::memcpy (&u, &f, 4); return u; }

int main (int argc, char** argv) {
  std::string in, out;
  int w = 0, h = 0, rc = -1, qp = 24, bitrate = 5000000, iper = 0, complexity = 0, slcmd = 0, slcnum = 1, slcmbnum = 0, deblock = 0;
  int scene = 0, spsid = 1, param_mask = 0;
  float fps = 30.0f;
  std::vector<int> pic_masks (1, 0);
  for (int i = 1; i < argc; ++i) {
    const char* a = argv[i];
    auto next = [&] () -> const char* { if (i + 1 >= argc) { std::fprintf (stderr, "missing value for %s\n", a); std::exit (2); } return argv[++i]; };
    if (!std::strcmp (a, "-i")) in = next();
    else if (!std::strcmp (a, "-o")) out = next();
    else if (!std::strcmp (a, "-w")) w = std::atoi (next());
    else if (!std::strcmp (a, "-h")) h = std::atoi (next());
    else if (!std::strcmp (a, "-fps")) fps = (float)std::atof (next());
    else if (!std::strcmp (a, "-rc")) rc = std::atoi (next());
    else if (!std::strcmp (a, "-qp")) qp = std::atoi (next());
    else if (!std::strcmp (a, "-bitrate")) bitrate = std::atoi (next());
    else if (!std::strcmp (a, "-iper")) iper = std::atoi (next());
    else if (!std::strcmp (a, "-complexity")) complexity = std::atoi (next());
    else if (!std::strcmp (a, "-slcmd")) slcmd = std::atoi (next());
    else if (!std::strcmp (a, "-slcnum")) slcnum = std::atoi (next());
    else if (!std::strcmp (a, "-slcmbnum")) slcmbnum = std::atoi (next());
    else if (!std::strcmp (a, "-deblock")) deblock = std::atoi (next());
    else if (!std::strcmp (a, "-scene")) scene = std::atoi (next());
    else if (!std::strcmp (a, "-spsid")) spsid = std::atoi (next());
    else if (!std::strcmp (a, "-param")) param_mask = std::atoi (next());
    else if (!std::strcmp (a, "-pic")) {
      pic_masks.clear();
      std::string list = next();
      for (size_t p = 0; p <= list.size();) { size_t e = list.find (',', p); if (e == std::string::npos) e = list.size(); pic_masks.push_back (std::atoi (list.substr (p, e - p).c_str())); p = e + 1; }
    } else if (!std::strcmp (a, "-quiet")) {
    } else { std::fprintf (stderr, "unknown option %s\n", a); return 2; }
  }
  if (in.empty() || out.empty() || w <= 0 || h <= 0 || pic_masks.empty()) { std::fprintf (stderr, "need -i -o -w -h\n"); return 2; }

  ISVCEncoder* enc = NULL;
  if (WelsCreateSVCEncoder (&enc) || !enc) { std::fprintf (stderr, "WelsCreateSVCEncoder failed\n"); return 1; }
  int trace = WELS_LOG_QUIET;
  enc->SetOption (ENCODER_OPTION_TRACE_LEVEL, &trace);
  SEncParamExt p;
  enc->GetDefaultParams (&p);
  p.iUsageType = CAMERA_VIDEO_REAL_TIME;
  p.iPicWidth = w; p.iPicHeight = h;
  p.iTargetBitrate = bitrate; p.iRCMode = (RC_MODES)rc; p.fMaxFrameRate = fps;
  p.iTemporalLayerNum = 1; p.iSpatialLayerNum = 1;
  p.iComplexityMode = (ECOMPLEXITY_MODE)complexity;
  p.uiIntraPeriod = (unsigned)iper;
  p.eSpsPpsIdStrategy = (EParameterSetStrategy)spsid;
  p.iEntropyCodingModeFlag = 0;
  p.bEnableFrameSkip = false;
  p.iMultipleThreadIdc = 1;
  p.iLoopFilterDisableIdc = deblock;
  p.bEnableFrameCroppingFlag = true;
  p.bEnableDenoise = false; p.bEnableBackgroundDetection = false; p.bEnableAdaptiveQuant = false;
  p.bEnableSceneChangeDetect = scene != 0;
  p.bEnableLongTermReference = false;
  p.iMaxQp = 51; p.iMinQp = 0;
  p.bPsnrY = (param_mask & 1) != 0; p.bPsnrU = (param_mask & 2) != 0; p.bPsnrV = (param_mask & 4) != 0;
  SSpatialLayerConfig& l = p.sSpatialLayers[0];
  l.iVideoWidth = w; l.iVideoHeight = h; l.fFrameRate = fps;
  l.iSpatialBitrate = bitrate; l.iDLayerQp = qp;
  l.uiProfileIdc = PRO_BASELINE;
  l.sSliceArgument.uiSliceMode = (SliceModeEnum)slcmd;
  l.sSliceArgument.uiSliceNum = (unsigned)slcnum;
  if (slcmbnum > 0) for (int k = 0; k < MAX_SLICES_NUM_TMP; ++k) l.sSliceArgument.uiSliceMbNum[k] = (unsigned)slcmbnum;
  if (enc->InitializeExt (&p)) { std::fprintf (stderr, "InitializeExt failed\n"); return 1; }

  FILE* fi = std::fopen (in.c_str(), "rb");
  FILE* fo = std::fopen (out.c_str(), "wb");
  if (!fi || !fo) { std::fprintf (stderr, "cannot open the files\n"); return 1; }
  const size_t fsz = (size_t)w * h * 3 / 2;
  std::vector<unsigned char> buf (fsz);
  SSourcePicture pic;
  std::memset (&pic, 0, sizeof (pic));
  pic.iColorFormat = videoFormatI420; pic.iPicWidth = w; pic.iPicHeight = h;
  pic.iStride[0] = w; pic.iStride[1] = pic.iStride[2] = w >> 1;
  pic.pData[0] = buf.data(); pic.pData[1] = buf.data() + (size_t)w * h; pic.pData[2] = pic.pData[1] + (size_t) (w >> 1) * (h >> 1);
  SFrameBSInfo info;
  for (int n = 0; std::fread (buf.data(), 1, fsz, fi) == fsz; ++n) {
    const int m = pic_masks[(size_t)n % pic_masks.size()];
    pic.bPsnrY = (m & 1) != 0; pic.bPsnrU = (m & 2) != 0; pic.bPsnrV = (m & 4) != 0;
    pic.uiTimeStamp = (long long)n * 33;
    std::memset (&info, 0, sizeof (info));
    if (enc->EncodeFrame (&pic, &info)) { std::fprintf (stderr, "EncodeFrame failed at picture %d\n", n); return 1; }
    for (int li = 0; li < info.iLayerNum; ++li) {
      const SLayerBSInfo& L = info.sLayerInfo[li];
      int bytes = 0;
      for (int k = 0; k < L.iNalCount; ++k) bytes += L.pNalLengthInByte[k];
      std::fwrite (L.pBsBuf, 1, (size_t)bytes, fo);
      std::printf ("%d %d %d %08x %08x %08x\n", n, li, (int)L.uiLayerType, bits_of (L.rPsnr[0]), bits_of (L.rPsnr[1]), bits_of (L.rPsnr[2]));
    }
  }
  std::fclose (fi);
  std::fclose (fo);
  enc->Uninitialize();
  WelsDestroySVCEncoder (enc);
  return 0;
}
