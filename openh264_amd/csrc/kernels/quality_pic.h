// quality_pic.h -- per-picture quality statistic: the sum of squared differences (SSE) between the source picture and its final
// reconstruction, per plane, over the macroblock-aligned picture (mb_w * 16 x mb_h * 16 luma, half of that chroma).
//
// Reference: WelsCalcPsnr (codec/common/src/utils.cpp:101-125) over iCurWidth x iCurHeight = the layer's iVideoWidth x iVideoHeight
// (encoder_ext.cpp:3557,3918-3942), which the reference has rounded UP to whole macroblocks (param_svc.h:486-489): a cropped picture is
// measured with its padding (the source's padding is luma 0 / chroma 128, CWelsPreProcess::Padding -- what src[0] holds as well).  The
// host turns the integer SSE into the reference's float (CALC_PSNR, utils.cpp:77-80).
//
// Inputs: the macroblock-tiled source src[0] (WH_SRC_*) and the planar reconstruction rec[0..2] -- the one copy of the reconstruction
// that is final in every configuration (deblocking idc 1 writes it in mode decision; all-IDR sessions never build the tiled twin).
// Shape: one wavefront walks one macroblock row, four macroblocks per step: lane = (macroblock q of the four, luma row r) reads 16 source
// and 16 reconstructed luma samples, and (q, plane, chroma row) 8 + 8 chroma samples, all loads of a step in flight together.  HBM-bound:
// one read of each input, three 64-bit atomics per row.  Squared differences: bytes unpacked into the 16-bit halves of a register (v_perm_b32), packed 16-bit subtraction,
// v_dot2_i32_i16 of the differences with themselves into the lane's sum.
//
// Overflow bound of the per-lane sums (u32; kept below 2^31 so that the 16-lane row sums of WV_ROWSUM4 fit an int as well): a lane adds
// 16 luma samples per step, mb_w / 4 steps, at most 65025 each: 4 * mb_w * 65025 <= 66.6 M for mb_w <= WH_SSE_MAX_MB_W (4096 samples);
// a row sum of 16 lanes <= 1.07 G < 2^31.  The launcher refuses wider pictures (the session API stops at 4096 anyway).
#pragma once
#include "prims.h"

#define WH_SSE_MAX_MB_W 256
#define WH_SSE_PLANE_Y 1
#define WH_SSE_PLANE_U 2
#define WH_SSE_PLANE_V 4
static_assert (16ull * 4ull * WH_SSE_MAX_MB_W * 65025ull < (1ull << 31), "SSE row sums of one wavefront must fit 31 bits");

#if defined(WH_EMU)
WH_FN void wh_atomic_add_u64 (uint64_t* p, uint64_t v) { *p += v; }
// sum over the four byte lanes of (a - b)^2
WH_FN uint32_t wh_sqdiff4 (uint32_t a, uint32_t b) {
  uint32_t s = 0;
  for (int k = 0; k < 4; ++k) { const int d = (int) ((a >> (8 * k)) & 255) - (int) ((b >> (8 * k)) & 255); s += (uint32_t) (d * d); }
  return s;
}
#else
WH_FN void wh_atomic_add_u64 (WH_G uint64_t* p, uint64_t v) { __hip_atomic_fetch_add (p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
typedef short wh_q16x2 __attribute__ ((ext_vector_type (2)));
WH_FN uint32_t wh_sqdiff4 (uint32_t a, uint32_t b) {
  // bytes 0, 1 and 2, 3 into 16-bit halves (zero-extended), packed subtraction, then d0^2 + d1^2 (+ acc) by one v_dot2_i32_i16 each
  const wh_q16x2 d01 = __builtin_bit_cast (wh_q16x2, __builtin_amdgcn_perm (0u, a, 0x0c010c00u)) - __builtin_bit_cast (wh_q16x2, __builtin_amdgcn_perm (0u, b, 0x0c010c00u));
  const wh_q16x2 d23 = __builtin_bit_cast (wh_q16x2, __builtin_amdgcn_perm (0u, a, 0x0c030c02u)) - __builtin_bit_cast (wh_q16x2, __builtin_amdgcn_perm (0u, b, 0x0c030c02u));
  return (uint32_t)__builtin_amdgcn_sdot2 (d23, d23, __builtin_amdgcn_sdot2 (d01, d01, 0, false), false);
}
#endif

// Macroblock row `mby` of picture J: adds its SSE of the planes in J.sse_planes to J.sse[0..2].
WH_FN void wh_sse_row_body (const WhSeqParams& P, const WhPicJob& J, int mby) {
  WH_G const uint8_t* src = (WH_G const uint8_t*)J.src[0];
  WH_G const uint8_t* ry = (WH_G const uint8_t*)J.rec[0];
  WH_G const uint8_t* ru = (WH_G const uint8_t*)J.rec[1];
  WH_G const uint8_t* rv = (WH_G const uint8_t*)J.rec[2];
  const int planes = (int)J.sse_planes;
  WvLaneArr acc_y, acc_c;              // per-lane sums (lane tables: one register each on the device)
  WV_LANES_BEGIN (lane)
  WV_LOWN (acc_y, lane) = 0; WV_LOWN (acc_c, lane) = 0;
  WV_LANES_END
  for (int mbx0 = 0; mbx0 < P.mb_w; mbx0 += 4) {
    WV_LANES_BEGIN (lane)
    const int q = lane >> 4;
    // lanes past the row's end read its last macroblock (in bounds) and add nothing.  All four loads are issued before any of them is
    // used (a plane that is not requested is read all the same and masked: the pass stays one round trip per step)
    const int mbx = mbx0 + q < P.mb_w ? mbx0 + q : P.mb_w - 1;
    const uint32_t on = mbx0 + q < P.mb_w ? 0xffffffffu : 0u;
    const int r = lane & 15, pl = (lane >> 3) & 1, rc = lane & 7;
    WH_G const uint8_t* s8 = src + WH_SRC_C_OFF (P.mb_w, mbx, mby, pl, rc, 0);
    WH_G const uint8_t* t8 = (pl ? rv : ru) + (size_t) (mby * 8 + rc) * P.rec_stride_c + mbx * 8;
    const WhU4 s = wh_ldg16 (src + WH_SRC_Y_OFF (P.mb_w, mbx, mby, r, 0));
    const WhU4 t = wh_ldg16 (ry + (size_t) (mby * 16 + r) * P.rec_stride_y + mbx * 16);
    const uint32_t s0 = * (WH_G const uint32_t*)s8, s1 = * (WH_G const uint32_t*) (s8 + 4);
    const uint32_t t0 = * (WH_G const uint32_t*)t8, t1 = * (WH_G const uint32_t*) (t8 + 4);
    const uint32_t my = (planes & WH_SSE_PLANE_Y) ? on : 0u, mc = (planes & (pl ? WH_SSE_PLANE_V : WH_SSE_PLANE_U)) ? on : 0u;
    WV_LOWN (acc_y, lane) += my & (wh_sqdiff4 (s.x, t.x) + wh_sqdiff4 (s.y, t.y) + wh_sqdiff4 (s.z, t.z) + wh_sqdiff4 (s.w, t.w));
    WV_LOWN (acc_c, lane) += mc & (wh_sqdiff4 (s0, t0) + wh_sqdiff4 (s1, t1));
    WV_LANES_END
  }
  // row sums of 16 lanes each (< 2^31, see above), added up in 64 bits: luma = all four rows; chroma: lanes with bit 3 clear are Cb, set Cr
  int y0, y1, y2, y3, u0, u1, u2, u3, v0, v1, v2, v3;
  WV_ROWSUM4 (y0, y1, y2, y3, lane, WV_LOWN (acc_y, lane));
  WV_ROWSUM4 (u0, u1, u2, u3, lane, (lane & 8) ? 0 : WV_LOWN (acc_c, lane));
  WV_ROWSUM4 (v0, v1, v2, v3, lane, (lane & 8) ? WV_LOWN (acc_c, lane) : 0);
  const uint64_t ty = (uint64_t) (uint32_t)y0 + (uint32_t)y1 + (uint32_t)y2 + (uint32_t)y3;
  const uint64_t tu = (uint64_t) (uint32_t)u0 + (uint32_t)u1 + (uint32_t)u2 + (uint32_t)u3;
  const uint64_t tv = (uint64_t) (uint32_t)v0 + (uint32_t)v1 + (uint32_t)v2 + (uint32_t)v3;
  WH_G uint64_t* out = (WH_G uint64_t*)J.sse;
  WV_LANES_BEGIN (lane)
  // one vector atomic per requested plane, from the first three lanes (never a scalar memory write)
  if (lane < 3 && (planes & (1 << lane))) wh_atomic_add_u64 (out + lane, lane == 0 ? ty : lane == 1 ? tu : tv);
  WV_LANES_END
}
