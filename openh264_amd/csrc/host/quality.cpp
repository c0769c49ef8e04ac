// quality.cpp -- the host side of the per-picture quality statistic: the default body of Backend::run_sse and the reference's PSNR
// expression over the sums of squared differences the device pass (kernels/quality_pic.h) returns.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "backend.h"
#include "quality.h"
#if defined(WH_EMU)
#include "../kernels/quality_pic.h"
#endif

namespace wh {

// The CPU test build runs the kernel body itself, one emulated wavefront per macroblock row, as EmuBackend::run_scene walks
// wh_scene_mb_body.  Every other backend must launch the kernel: the HIP backend overrides this, and there is no host fall-back.
void Backend::run_sse (const WhSeqParams& P, const WhPicJob* jobs, int n) {
#if defined(WH_EMU)
  for (int j = 0; j < n; ++j) {
    if (!jobs[j].sse_planes || !jobs[j].sse) continue;
    for (int y = 0; y < P.mb_h; ++y) wh_sse_row_body (P, jobs[j], y);
  }
#else
  (void)P; (void)jobs; (void)n;
  fprintf (stderr, "welship: backend %s has no quality-statistic pass\n", name());
  abort();
#endif
}

// CALC_PSNR / WelsCalcPsnr (codec/common/src/utils.cpp:77-80,119-124): the same expression in the same order, evaluated in double
float psnr_of_sse (uint64_t sse, int width, int height) {
  if (sse == 0) return 99.99f;
  return (float) ((10.0 / log (10.0)) * log (65025.0 * width * height / (double) (int64_t)sse));
}

void fill_quality (WelsHipFrameQuality* q, const uint64_t* sse, uint32_t planes, int pic_w, int pic_h) {
  for (int k = 0; k < 3; ++k) {
    const bool on = (planes >> k) & 1;
    q->uiSse[k] = on ? sse[k] : 0;
    q->rPsnr[k] = on ? psnr_of_sse (sse[k], k ? pic_w >> 1 : pic_w, k ? pic_h >> 1 : pic_h) : 0.0f;
  }
  q->uiPlanes = planes & 7u;
}

}  // namespace wh
