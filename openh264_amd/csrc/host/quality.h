// quality.h -- per-picture quality statistic on the host side (quality.cpp).
#pragma once
#include <stdint.h>
#include "../../../include/welship.h"

namespace wh {
// the reference's PSNR of one plane from its integer sum of squared differences (99.99 when the plane is lossless)
float psnr_of_sse (uint64_t sse, int width, int height);
// WelsHipFrameQuality of a picture: the planes not in `planes` report 0 and 0.0, as the reference leaves rPsnr at 0
void fill_quality (WelsHipFrameQuality* q, const uint64_t* sse, uint32_t planes, int pic_w, int pic_h);
}  // namespace wh
