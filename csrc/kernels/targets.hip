// Anchor-target assignment on the device (replaces the reference's CPU numpy + Cython path).
//
// Spec: keras-retinanet utils.anchors.anchor_targets_bbox + compute_overlap.pyx (entered at
// /root/reference/train.py:51,429):
//   IoU with the "+1 pixel" convention; argmax over gt (first max wins); positive if
//   IoU >= 0.5, ignore if 0.4 <= IoU < 0.5, negative below; anchors whose centre lies outside
//   the unpadded image (cx >= W or cy >= H) are ignored; regression = corner offsets / anchor
//   w,h / 0.2.  Images without boxes: every anchor negative (except outside ones).
// Output is compact: state int8 (-1/0/1), label int32, regression f32x4, plus the number of
// positives of the whole local batch (the focal / smooth-L1 normaliser) via one integer
// atomic per wave.  One block = 256 anchors of one image; gt boxes are staged through LDS.
#include "common.h"

namespace {
constexpr int kBlock = 256;
constexpr int kTile = 256;  // gt boxes per LDS tile

__global__ __launch_bounds__(kBlock) void anchor_targets_kernel(
    const float* __restrict__ anchors, const float* __restrict__ centers, int A, const float* __restrict__ gt, int G, const int* __restrict__ gt_count,
    const int* __restrict__ image_hw, int8_t* __restrict__ state, int32_t* __restrict__ label,
    float* __restrict__ reg, int* __restrict__ npos, float neg_thr, float pos_thr, float inv_std) {
  __shared__ float sg[kTile * 5];
  const int b = blockIdx.y;
  const int a = blockIdx.x * kBlock + threadIdx.x;
  const int cnt = min(gt_count[b], G);
  float ax1 = 0.f, ay1 = 0.f, ax2 = 0.f, ay2 = 0.f;
  if (a < A) {
    const float4 an = reinterpret_cast<const float4*>(anchors)[a];
    ax1 = an.x; ay1 = an.y; ax2 = an.z; ay2 = an.w;
  }
  const float area_a = (ax2 - ax1 + 1.f) * (ay2 - ay1 + 1.f);
  float best = -1.f;
  int arg = 0;
  const float* gb = gt + (long long)b * G * 5;
  for (int t0 = 0; t0 < cnt; t0 += kTile) {
    const int nt = min(kTile, cnt - t0);
    __syncthreads();
    for (int i = threadIdx.x; i < nt * 5; i += kBlock) sg[i] = gb[t0 * 5 + i];
    __syncthreads();
    for (int j = 0; j < nt; ++j) {
      const float gx1 = sg[j * 5 + 0], gy1 = sg[j * 5 + 1], gx2 = sg[j * 5 + 2], gy2 = sg[j * 5 + 3];
      const float iw = fminf(ax2, gx2) - fmaxf(ax1, gx1) + 1.f;
      const float ih = fminf(ay2, gy2) - fmaxf(ay1, gy1) + 1.f;
      float iou = 0.f;
      if (iw > 0.f && ih > 0.f) {
        const float inter = iw * ih;
        const float ua = area_a + (gx2 - gx1 + 1.f) * (gy2 - gy1 + 1.f) - inter;
        iou = inter / ua;
      }
      if (iou > best) { best = iou; arg = t0 + j; }
    }
  }
  int is_pos = 0;
  if (a < A) {
    const long long o = (long long)b * A + a;
    int st;
    float mx1, my1, mx2, my2;
    int lab = 0;
    if (cnt > 0) {
      st = best < neg_thr ? 0 : (best >= pos_thr ? 1 : -1);
      const float* g = gb + arg * 5;
      mx1 = g[0]; my1 = g[1]; mx2 = g[2]; my2 = g[3];
      lab = (int)g[4];
    } else {
      st = 0;
      mx1 = ax1; my1 = ay1; mx2 = ax2; my2 = ay2;
    }
    // centres pre-rounded DOWN from float64 on the host: same outside test as the fp64 reference
    const float cx = centers[2 * a], cy = centers[2 * a + 1];
    if (cx >= (float)image_hw[2 * b + 1] || cy >= (float)image_hw[2 * b]) st = -1;
    const float aw = ax2 - ax1, ah = ay2 - ay1;
    float4 r;
    r.x = (mx1 - ax1) / aw * inv_std;
    r.y = (my1 - ay1) / ah * inv_std;
    r.z = (mx2 - ax2) / aw * inv_std;
    r.w = (my2 - ay2) / ah * inv_std;
    reinterpret_cast<float4*>(reg)[o] = r;
    state[o] = (int8_t)st;
    label[o] = lab;
    is_pos = st == 1;
  }
  const int w = wave_sum_i(is_pos);
  if ((threadIdx.x & 63) == 0 && w) atomicAdd(npos, w);
}
__global__ void zero_count_kernel(int* c) {
  if (threadIdx.x == 0) c[0] = 0;
}

// ---------------------------------------------------------------------------------------------------------
// ATSS (Zhang et al., CVPR 2020, Algorithm 1; spec: ops.anchors.atss_targets_bbox).  Every box takes, on every
// level, the min(K, h * w) locations whose grid centre is nearest to its own, ordered by (d2, row-major index),
// and all A0 anchors there as candidates; its threshold is mean + unbiased std of their IoUs; a candidate at or
// above it whose grid centre lies inside the box is positive, for the box of largest IoU (first wins a tie).
//
// Pass 1, one wave per (image, box): selection by rank, K wave-wide minima of the 64-bit key (d2 bits, index)
// over a window around the box centre's cell (the whole level when the window cannot be shown to suffice), then
// the candidates' IoUs, their mean and, in a second sweep, the squared deviations.  It leaves the threshold and
// per level the key of the last selected location: a location is selected iff its key <= that one.
// Pass 2, one thread per anchor, boxes staged through LDS: centre inside the box, the anchor's location selected
// on its own level, IoU >= threshold and > the best so far.
// Nothing but the npos count is accumulated across threads, so two calls give the same bits; no launch shape
// depends on the boxes, and boxes at or beyond gt_count[b] are never read.
constexpr int kAtssMaxLev = 5;
constexpr int kAtssMaxK = 16;
constexpr int kAtssWindow = 4;  // ops.anchors.ATSS_WINDOW (atss_window is this rule in Python)
constexpr float kAtssInside = 0.01f;

struct AtssLevels {
  int nlev;
  int first[kAtssMaxLev], h[kAtssMaxLev], w[kAtssMaxLev], stride[kAtssMaxLev];
};

typedef unsigned long long atss_key_t;

// squared distance of a grid centre to the box centre: every operation rounded on its own, so that the fp32
// torch expression gives the same bits.  (__fmul_rn / __fadd_rn are plain operators in the HIP headers, compiled
// there under the default contraction, and came out fused; operators under this pragma do not.)
__device__ __forceinline__ atss_key_t atss_key(int ix, int iy, int w, float stride, float gcx, float gcy) {
#pragma clang fp contract(off)
  const float cx = ((float)ix + 0.5f) * stride, cy = ((float)iy + 0.5f) * stride;
  const float dx = cx - gcx, dy = cy - gcy;
  const float dx2 = dx * dx, dy2 = dy * dy;
  const float d2 = dx2 + dy2;
  return ((atss_key_t)__float_as_uint(d2) << 32) | (unsigned)(iy * w + ix);
}

__device__ __forceinline__ atss_key_t wave_min_key(atss_key_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    const atss_key_t u = ((atss_key_t)hi << 32) | lo;
    v = u < v ? u : v;
  }
  return v;
}

__device__ __forceinline__ float atss_iou(float ax1, float ay1, float ax2, float ay2, float gx1, float gy1, float gx2,
                                          float gy2) {
  const float area_a = (ax2 - ax1 + 1.f) * (ay2 - ay1 + 1.f);
  const float iw = fminf(ax2, gx2) - fmaxf(ax1, gx1) + 1.f;
  const float ih = fminf(ay2, gy2) - fmaxf(ay1, gy1) + 1.f;
  float iou = 0.f;
  if (iw > 0.f && ih > 0.f) {
    const float inter = iw * ih;
    const float ua = area_a + (gx2 - gx1 + 1.f) * (gy2 - gy1 + 1.f) - inter;
    iou = inter / ua;
  }
  return iou;
}

__global__ __launch_bounds__(64) void atss_select_kernel(
    const float* __restrict__ anchors, int A0, const float* __restrict__ gt, int G, const int* __restrict__ gt_count,
    AtssLevels lv, int K, float* __restrict__ thr, atss_key_t* __restrict__ cut, int* __restrict__ sel) {
  __shared__ int s_anchor[kAtssMaxLev * kAtssMaxK];  // first anchor of every selected location, all levels
  const int b = blockIdx.y, g = blockIdx.x, lane = threadIdx.x;
  const long long bg = (long long)b * G + g;
  if (g >= min(gt_count[b], G)) {  // never read; the outputs say so
    if (lane == 0) thr[bg] = __builtin_inff();
    for (int i = lane; i < lv.nlev; i += 64) cut[bg * lv.nlev + i] = 0ull;
    if (sel) for (int i = lane; i < lv.nlev * kAtssMaxK; i += 64) sel[bg * lv.nlev * kAtssMaxK + i] = -1;
    return;
  }
  const float* gp = gt + bg * 5;
  const float gx1 = gp[0], gy1 = gp[1], gx2 = gp[2], gy2 = gp[3];
  const float gcx = __fmul_rn(__fadd_rn(gx1, gx2), 0.5f), gcy = __fmul_rn(__fadd_rn(gy1, gy2), 0.5f);
  int m = 0;  // selected locations so far, over the levels
  for (int l = 0; l < lv.nlev; ++l) {
    const int h = lv.h[l], w = lv.w[l];
    const float stride = (float)lv.stride[l];
    const int k = min(K, h * w);
    const int ix0 = min(max((int)floorf(gcx / stride), 0), w - 1);
    const int iy0 = min(max((int)floorf(gcy / stride), 0), h - 1);
    int x0 = max(ix0 - kAtssWindow, 0), x1 = min(ix0 + kAtssWindow, w - 1);
    int y0 = max(iy0 - kAtssWindow, 0), y1 = min(iy0 + kAtssWindow, h - 1);
    if (x0 != 0 || y0 != 0 || x1 != w - 1 || y1 != h - 1) {
      // a location outside the window is at least kAtssWindow + 0.5 strides away: k locations inside it that are
      // closer than kAtssWindow strides beat all of those; without them the whole level is scanned
      const float r = (float)(kAtssWindow * lv.stride[l]);
      const atss_key_t bound = (atss_key_t)__float_as_uint(__fmul_rn(r, r)) << 32;
      const int rw = x1 - x0 + 1, cells = rw * (y1 - y0 + 1);
      int near = 0;
      for (int t = lane; t < cells; t += 64) near += atss_key(x0 + t % rw, y0 + t / rw, w, stride, gcx, gcy) < bound;
      if (wave_sum_i(near) < k) { x0 = 0; y0 = 0; x1 = w - 1; y1 = h - 1; }
    }
    const int rw = x1 - x0 + 1, cells = rw * (y1 - y0 + 1);
    atss_key_t last = 0ull;
    for (int r = 0; r < k; ++r) {
      // the r-th smallest key: the smallest one above the (r-1)-th (keys are distinct: the index is part)
      atss_key_t mine = ~0ull;
      for (int t = lane; t < cells; t += 64) {
        const atss_key_t key = atss_key(x0 + t % rw, y0 + t / rw, w, stride, gcx, gcy);
        if ((r == 0 || key > last) && key < mine) mine = key;
      }
      last = wave_min_key(mine);
      const int loc = min((int)((unsigned)last & 0x7fffffffu), h * w - 1);  // (a key's index is always below h * w)
      if (lane == 0) {
        s_anchor[m + r] = lv.first[l] + loc * A0;
        if (sel) sel[(bg * lv.nlev + l) * kAtssMaxK + r] = loc;
      }
    }
    if (lane == 0) cut[bg * lv.nlev + l] = last;
    if (sel) for (int r = k + lane; r < kAtssMaxK; r += 64) sel[(bg * lv.nlev + l) * kAtssMaxK + r] = -1;
    m += k;
  }
  __syncthreads();
  const int n = m * A0;
  float s = 0.f;
  for (int c = lane; c < n; c += 64) {
    const float4 an = reinterpret_cast<const float4*>(anchors)[s_anchor[c / A0] + c % A0];
    s += atss_iou(an.x, an.y, an.z, an.w, gx1, gy1, gx2, gy2);
  }
  const float mean = wave_sum(s) / (float)n;
  float q = 0.f;
  for (int c = lane; c < n; c += 64) {
    const float4 an = reinterpret_cast<const float4*>(anchors)[s_anchor[c / A0] + c % A0];
    const float d = atss_iou(an.x, an.y, an.z, an.w, gx1, gy1, gx2, gy2) - mean;
    q += d * d;
  }
  q = wave_sum(q);
  if (lane == 0) thr[bg] = mean + (n > 1 ? sqrtf(q / (float)(n - 1)) : 0.f);
}

constexpr int kAtssBox = 6;  // x1, y1, x2, y2, label, threshold

__global__ __launch_bounds__(kBlock) void atss_assign_kernel(
    const float* __restrict__ anchors, const float* __restrict__ centers, int A, int A0, const float* __restrict__ gt,
    int G, const int* __restrict__ gt_count, const int* __restrict__ image_hw, AtssLevels lv,
    const float* __restrict__ thr, const atss_key_t* __restrict__ cut, int8_t* __restrict__ state,
    int32_t* __restrict__ label, float* __restrict__ reg, int* __restrict__ npos, float inv_std) {
  __shared__ float sg[kTile * kAtssBox];
  const int b = blockIdx.y;
  const int a = blockIdx.x * kBlock + threadIdx.x;
  const int cnt = min(gt_count[b], G);
  float ax1 = 0.f, ay1 = 0.f, ax2 = 0.f, ay2 = 0.f;
  // the anchor's level and location; the grid centre comes from the table (the centers array is rounded down
  // from an inexact sum and serves the outside test alone)
  int lev = 0, ix = 0, iy = 0, w = 1;
  float stride = 1.f, cx = 0.f, cy = 0.f;
  if (a < A) {
    const float4 an = reinterpret_cast<const float4*>(anchors)[a];
    ax1 = an.x; ay1 = an.y; ax2 = an.z; ay2 = an.w;
    for (int l = 1; l < lv.nlev; ++l) lev = a >= lv.first[l] ? l : lev;
    w = lv.w[lev];
    const int loc = (a - lv.first[lev]) / A0;
    ix = loc % w; iy = loc / w;
    stride = (float)lv.stride[lev];
    cx = __fmul_rn((float)ix + 0.5f, stride);
    cy = __fmul_rn((float)iy + 0.5f, stride);
  }
  float best = -1.f;
  int arg = -1;
  const long long bG = (long long)b * G;
  const float* gb = gt + bG * 5;
  for (int t0 = 0; t0 < cnt; t0 += kTile) {
    const int nt = min(kTile, cnt - t0);
    __syncthreads();
    for (int i = threadIdx.x; i < nt * kAtssBox; i += kBlock) {
      const int j = i / kAtssBox, f = i % kAtssBox;
      sg[i] = f < 5 ? gb[(t0 + j) * 5 + f] : thr[bG + t0 + j];
    }
    __syncthreads();
    if (a < A) {
      for (int j = 0; j < nt; ++j) {
        const float gx1 = sg[j * kAtssBox + 0], gy1 = sg[j * kAtssBox + 1], gx2 = sg[j * kAtssBox + 2],
                    gy2 = sg[j * kAtssBox + 3];
        if (!(fminf(fminf(cx - gx1, cy - gy1), fminf(gx2 - cx, gy2 - cy)) > kAtssInside)) continue;
        const float gcx = __fmul_rn(__fadd_rn(gx1, gx2), 0.5f), gcy = __fmul_rn(__fadd_rn(gy1, gy2), 0.5f);
        if (atss_key(ix, iy, w, stride, gcx, gcy) > cut[(bG + t0 + j) * lv.nlev + lev]) continue;
        const float iou = atss_iou(ax1, ay1, ax2, ay2, gx1, gy1, gx2, gy2);
        if (iou >= sg[j * kAtssBox + 5] && iou > best) { best = iou; arg = t0 + j; }
      }
    }
  }
  int is_pos = 0;
  if (a < A) {
    const long long o = (long long)b * A + a;
    int st = 0, lab = 0;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (arg >= 0) {
      const float* g = gb + arg * 5;
      const float aw = ax2 - ax1, ah = ay2 - ay1;
      st = 1;
      lab = (int)g[4];
      r.x = (g[0] - ax1) / aw * inv_std;
      r.y = (g[1] - ay1) / ah * inv_std;
      r.z = (g[2] - ax2) / aw * inv_std;
      r.w = (g[3] - ay2) / ah * inv_std;
    }
    // centres pre-rounded DOWN from float64 on the host: same outside test as the fp64 reference
    if (centers[2 * a] >= (float)image_hw[2 * b + 1] || centers[2 * a + 1] >= (float)image_hw[2 * b]) st = -1;
    reinterpret_cast<float4*>(reg)[o] = r;
    state[o] = (int8_t)st;
    label[o] = lab;
    is_pos = st == 1;
  }
  const int ws = wave_sum_i(is_pos);
  if ((threadIdx.x & 63) == 0 && ws) atomicAdd(npos, ws);
}
}  // namespace

// npos is zeroed here (a one-thread kernel on the same stream: a hipMemsetAsync is a runtime blit that
// measured 170-490 us of idle GPU in front of it at each step start) before the kernel accumulates into it.
MXR_API int mxr_anchor_targets(const float* anchors, const float* centers, int A, const float* gt, int B, int G, const int* gt_count,
                               const int* image_hw, int8_t* state, int32_t* label, float* reg, int* npos,
                               float neg_thr, float pos_thr, float box_std, hipStream_t stream) {
  zero_count_kernel<<<1, 64, 0, stream>>>(npos);
  dim3 grid((A + kBlock - 1) / kBlock, B);
  anchor_targets_kernel<<<grid, kBlock, 0, stream>>>(anchors, centers, A, gt, G, gt_count, image_hw, state, label, reg, npos,
                                                     neg_thr, pos_thr, 1.0f / box_std);
  return (int)hipGetLastError();
}

// ATSS targets.  levels: nlev rows of (first anchor index, h, w, stride), by value into the launches (one graph
// is one padded shape).  thr (B, G) and cut (B, G, nlev) 64-bit are pass 1's results for pass 2; sel
// (B, G, nlev, 16) int32, or null, receives the selected locations in selection order (-1 padded).  Both grids
// depend on B, G and A alone.  Returns hipErrorInvalidValue for a topk outside 1..16 or a table that does not
// tile the A anchors.
MXR_API int mxr_atss_targets(const float* anchors, const float* centers, int A, const int* levels, int nlev, const float* gt,
                             int B, int G, const int* gt_count, const int* image_hw, int topk, float* thr,
                             unsigned long long* cut, int* sel, int8_t* state, int32_t* label, float* reg, int* npos,
                             float box_std, hipStream_t stream) {
  if (topk < 1 || topk > kAtssMaxK || nlev < 1 || nlev > kAtssMaxLev || A < 1) return (int)hipErrorInvalidValue;
  AtssLevels lv;
  lv.nlev = nlev;
  long long locs = 0;
  for (int l = 0; l < kAtssMaxLev; ++l) {
    const bool on = l < nlev;
    lv.first[l] = on ? levels[4 * l] : 0;
    lv.h[l] = on ? levels[4 * l + 1] : 1;
    lv.w[l] = on ? levels[4 * l + 2] : 1;
    lv.stride[l] = on ? levels[4 * l + 3] : 1;
    if (on && (lv.h[l] < 1 || lv.w[l] < 1 || lv.stride[l] < 1)) return (int)hipErrorInvalidValue;
    if (on) locs += (long long)lv.h[l] * lv.w[l];
  }
  if (A % locs) return (int)hipErrorInvalidValue;
  const int A0 = (int)(A / locs);
  long long first = 0;
  for (int l = 0; l < nlev; ++l) {
    if (lv.first[l] != first) return (int)hipErrorInvalidValue;
    first += (long long)lv.h[l] * lv.w[l] * A0;
  }
  zero_count_kernel<<<1, 64, 0, stream>>>(npos);
  if (G > 0) atss_select_kernel<<<dim3(G, B), 64, 0, stream>>>(anchors, A0, gt, G, gt_count, lv, topk, thr, cut, sel);
  dim3 grid((A + kBlock - 1) / kBlock, B);
  atss_assign_kernel<<<grid, kBlock, 0, stream>>>(anchors, centers, A, A0, gt, G, gt_count, image_hw, lv, thr, cut, state,
                                                  label, reg, npos, 1.0f / box_std);
  return (int)hipGetLastError();
}
