// Arithmetic shared by the FilterDetections kernels (filter.hip: greedy NMS, soft_nms.hip: Soft-NMS): box decode +
// clip, IoU, sigmoid and the candidate sort key.  One copy, so that both kernels and the select pass rank the same
// candidate by the same bits.
#pragma once
#include "common.h"

// decode, IoU and sigmoid follow the oracle's operation order with IEEE rounding and no FMA contraction,
// so that NMS decisions on near-ties match the torch oracle (ops/boxes.py)
#pragma clang fp contract(off)

constexpr int FD_BLOCK = 256;
constexpr int FD_MAXDET = 512;

__device__ __forceinline__ float fd_iou(const float4 a, const float4 b) {
  const float aa = fmaxf(a.z - a.x, 0.f) * fmaxf(a.w - a.y, 0.f);
  const float ab = fmaxf(b.z - b.x, 0.f) * fmaxf(b.w - b.y, 0.f);
  const float iw = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f);
  const float ih = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
  const float inter = iw * ih;
  const float u = aa + ab - inter;
  return u > 0.f ? __fdiv_rn(inter, u) : 0.f;
}

__device__ __forceinline__ float fd_sigmoid(float x) { return __fdiv_rn(1.f, 1.f + expf(-x)); }

// scores in (0, 1): the float bits order like the values
__device__ __forceinline__ unsigned long long fd_key(float p, int a) {
  return ((unsigned long long)__float_as_uint(p) << 32) | (unsigned long long)(0xffffffffu - (unsigned)a);
}

__device__ __forceinline__ int fd_key_anchor(unsigned long long key) {
  return (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
}

__device__ __forceinline__ float fd_key_score(unsigned long long key) { return __uint_as_float((unsigned)(key >> 32)); }

// RegressBoxes + ClipBoxes of anchor a in image b (ddtype 1: bf16 deltas, 0: fp32)
__device__ __forceinline__ float4 fd_decode(const float* __restrict__ anchors, const void* __restrict__ deltas,
                                            int ddtype, int b, int a, int A, float box_std, float H, float W) {
  const float4 an = reinterpret_cast<const float4*>(anchors)[a];
  const long long di = ((long long)b * A + a) * 4;
  float d[4];
  if (ddtype == 1) {
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = bf2f(((const bf16_t*)deltas)[di + j]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = ((const float*)deltas)[di + j];
  }
  const float aw = an.z - an.x, ah = an.w - an.y;
  float4 bx;
  bx.x = fminf(fmaxf(an.x + d[0] * box_std * aw, 0.f), W);
  bx.y = fminf(fmaxf(an.y + d[1] * box_std * ah, 0.f), H);
  bx.z = fminf(fmaxf(an.z + d[2] * box_std * aw, 0.f), W);
  bx.w = fminf(fmaxf(an.w + d[3] * box_std * ah, 0.f), H);
  return bx;
}
