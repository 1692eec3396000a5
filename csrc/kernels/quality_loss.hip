// IoU-aware classification losses, --classification-loss qfl / vfl: Quality Focal Loss (Li et al., "Generalized
// Focal Loss", NeurIPS 2020, beta = 2) and Varifocal Loss (Zhang et al., "VarifocalNet", CVPR 2021, alpha = 0.75,
// gamma = 2).  Loss partial sums AND the logit gradients in one pass, under the focal kernel's contract
// (losses.hip): bf16 or fp32 logits with fp32 arithmetic, 16 B per access, one deterministic partial per block, the
// plain [rows, C] or the zero-padded [rows / grp][ld] gradient layout, rows of state -1 dropped, everything divided
// by max(1, #positives) read from device memory.
//
// The label element of a positive row is trained towards q, the IoU of the row's decoded predicted box with its
// decoded target box (a constant in the backward); every other element towards 0 (focal_common.h has the
// per-element forms).  Only the thread whose vector holds that label column needs q -- about one vector in a
// thousand -- so it alone loads the row's prediction (8 B or 16 B), target and anchor (16 B each) and computes the
// IoU there: no per-row q buffer, no second launch.  The branch holds up the wave that meets it for its three loads
// (issued together: one memory round trip) and ~200 instructions (the IoU, a library exp, log1p and division); with
// 1 % positive rows about one wave in sixteen meets it per vector.  Measured at 16 x 200,700 x 80 bf16 logits
// (profiles/quality_loss.txt): 4-5 % of the launch, on top of a launch that without any positive row runs 5 % behind
// focal's on the same body.
#include "common.h"
#include "focal_common.h"

void mxr_loss_finalize_launch(const float* partials, int n, const int* npos, float* out, hipStream_t stream);
MXR_API int mxr_loss_grid();

namespace {

constexpr int kBlock = 256;
constexpr float kBoxStd = 0.2f;
constexpr float kIoUEps = 1e-7f;

template <typename T, int V>
struct Vec;
template <> struct Vec<bf16_t, 8> { typedef uint4 type; };
template <> struct Vec<bf16_t, 4> { typedef uint2 type; };
template <> struct Vec<float, 4> { typedef float4 type; };

// q of one positive row: the IoU of bbox_transform_inv (mean 0, std kBoxStd) of the predicted and of the target
// deltas with anchor a, the predicted corners ordered (the decode is linear, a prediction can flip),
// inter / (area_p + area_g - inter + eps), as ops.losses.iou_loss_rows has it.  The boxes are held relative to the
// anchor's top-left corner, for the reason iou_loss_kernel (losses.hip) gives.  vec: every row of reg starts on a
// 4-element boundary in memory.
template <typename T>
__device__ __forceinline__ float quality_iou(const T* __restrict__ reg, const float* __restrict__ reg_t,
                                             const float* __restrict__ anchors, long long row, int a, bool vec) {
  typedef typename Vec<T, 4>::type VT;
  const float4 an = reinterpret_cast<const float4*>(anchors)[a];
  const float4 t = reinterpret_cast<const float4*>(reg_t)[row];
  T ps[4];
  if (vec) {
    *reinterpret_cast<VT*>(ps) = reinterpret_cast<const VT*>(reg)[row];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) ps[j] = reg[row * 4 + j];
  }
  const float aw = an.z - an.x, ah = an.w - an.y;
  const float sw = kBoxStd * aw, sh = kBoxStd * ah;
  const float gx1 = sw * t.x, gy1 = sh * t.y, gx2 = aw + sw * t.z, gy2 = ah + sh * t.w;
  const float qx1 = sw * Cvt<T>::to_f(ps[0]), qy1 = sh * Cvt<T>::to_f(ps[1]);
  const float qx2 = aw + sw * Cvt<T>::to_f(ps[2]), qy2 = ah + sh * Cvt<T>::to_f(ps[3]);
  const float px1 = fminf(qx1, qx2), px2 = fmaxf(qx1, qx2), py1 = fminf(qy1, qy2), py2 = fmaxf(qy1, qy2);
  const float iw = fmaxf(fminf(px2, gx2) - fmaxf(px1, gx1), 0.f);
  const float ih = fmaxf(fminf(py2, gy2) - fmaxf(py1, gy1), 0.f);
  const float I = iw * ih;
  const float U = (px2 - px1) * (py2 - py1) + (gx2 - gx1) * (gy2 - gy1) - I + kIoUEps;
  return I / U;
}

// what a kernel needs beside the logits
struct QualityArgs {
  const void* reg;          // [rows, 4] predicted deltas, of the logits' type
  const float* reg_t;       // [rows, 4] target deltas
  const float* anchors;     // [A, 4]; row r belongs to anchor r % A
  const int8_t* state;      // [rows]
  const int32_t* label;     // [rows]
  const int* npos;
  int A, kind;
  bool reg_vec;
};

// The label element of a positive row with its soft target: loss and gradient of quality_pos.  The anchor index
// wants a division: 32-bit where the row allows it.
template <typename T>
__device__ __forceinline__ void quality_label_elem(const QualityArgs& a, long long row, float x, float& loss,
                                                   float& grad) {
  const int an = row < 0x7fffffffLL ? (int)row % a.A : (int)(row % a.A);
  const float q = quality_iou<T>((const T*)a.reg, a.reg_t, a.anchors, row, an, a.reg_vec);
  quality_pos(x, q, a.kind, loss, grad);
}

template <typename T>
__device__ __forceinline__ void quality_neg_t(float x, float c_loss, float c_grad, float& loss, float& grad) {
  if constexpr (sizeof(T) == sizeof(float))
    quality_neg_f32(x, c_loss, c_grad, loss, grad);
  else
    focal_neg_g2_inr(x, c_loss, c_grad, loss, grad);
}

// logits / dlogits: [rows, C] row-major, C a multiple of V; 64-bit indices (any size).  fp32, and bf16 from 2^31
// elements on.
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void quality_kernel(const T* __restrict__ logits, QualityArgs a,
                                                         T* __restrict__ dlogits, float* __restrict__ partials,
                                                         long long nvec, int C, int grp, int ld) {
  __shared__ float red[16];
  const float inv = 1.0f / fmaxf(1.0f, (float)(*a.npos));
  const float c = a.kind == kVFL ? kVflAlpha : 1.0f;
  float acc = 0.f;
  typedef typename Vec<T, V>::type VT;
  const VT* in = reinterpret_cast<const VT*>(logits);
  VT* out = reinterpret_cast<VT*>(dlogits);
  for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < nvec; i += (long long)gridDim.x * kBlock) {
    const long long e0 = i * V;
    long long row;
    int c0;
    if (e0 < 0x7fffffffLL) {   // 32-bit division (64-bit integer division is emulated on CDNA)
      const int e = (int)e0, r = e / C;
      row = r;
      c0 = e - r * C;
    } else {
      row = e0 / C;
      c0 = (int)(e0 - row * C);
    }
    const int s = a.state[row];
    VT v = in[i];
    T xs[V];
    *reinterpret_cast<VT*>(xs) = v;
    T gs[V];
    if (s == -1) {
#pragma unroll
      for (int j = 0; j < V; ++j) gs[j] = Cvt<T>::from_f(0.f);
    } else {
      const int lb = (s == 1) ? a.label[row] - c0 : -1;   // the label's index inside this vector, if it is there
      float gv[V];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float l;
        quality_neg_t<T>(Cvt<T>::to_f(xs[j]), c, c, l, gv[j]);
        acc += j == lb ? 0.f : l;
      }
      if (lb >= 0 && lb < V) {                              // rare: the label element of a positive row
        float xl = Cvt<T>::to_f(xs[0]);
#pragma unroll
        for (int j = 1; j < V; ++j) xl = j == lb ? Cvt<T>::to_f(xs[j]) : xl;
        float l, g;
        quality_label_elem<T>(a, row, xl, l, g);
        acc += l;
#pragma unroll
        for (int j = 0; j < V; ++j) gv[j] = j == lb ? g : gv[j];
      }
#pragma unroll
      for (int j = 0; j < V; ++j) gs[j] = Cvt<T>::from_f(gv[j] * inv);
    }
    if (ld > 0)   // padded gradient layout: rows grouped by grp (anchors per pixel), group stride ld
      *reinterpret_cast<VT*>(dlogits + (row / grp) * (long long)ld + (row % grp) * (long long)C + c0) =
          *reinterpret_cast<VT*>(gs);
    else
      out[i] = *reinterpret_cast<VT*>(gs);
  }
  const float bs = block_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = bs;
}

// bf16 fast path (32-bit indexing, < 2^31 elements): U independent 16-B vectors in flight per thread per
// iteration, and CC / GG > 0 the class count and the anchor group size as compile-time constants (80 / 9 for
// COCO), both for the reasons focal_bf16_kernel (losses.hip) states.  Every logit goes through focal_neg_g2_inr
// (the target-0 form of both losses; there is no clip, so no other body); the vector that holds the label of a
// positive row then replaces that one element.
template <int U, int CC = 0, int GG = 0>
__global__ __launch_bounds__(kBlock) void quality_bf16_kernel(const bf16_t* __restrict__ logits, QualityArgs a,
                                                              bf16_t* __restrict__ dlogits,
                                                              float* __restrict__ partials, int nvec, int C_, int grp_,
                                                              int ld) {
  __shared__ float red[16];
  const int C = CC > 0 ? CC : C_;
  const int grp = GG > 0 ? GG : grp_;
  const float inv = 1.0f / fmaxf(1.0f, (float)(*a.npos));
  const float c = a.kind == kVFL ? kVflAlpha : 1.0f;
  const float cg = c * inv;
  float acc = 0.f;
  const uint4* in = reinterpret_cast<const uint4*>(logits);
  const int stride = gridDim.x * kBlock;
  for (int base = blockIdx.x * kBlock + threadIdx.x; base < nvec; base += stride * U) {
    uint4 v[U];
    int row[U], c0[U], st[U], lab[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = base + u * stride;
      st[u] = -2;
      if (i < nvec) {
        const int e = i * 8;
        row[u] = e / C;
        c0[u] = e - row[u] * C;
        st[u] = a.state[row[u]];
        lab[u] = a.label[row[u]];
        v[u] = in[i];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (st[u] == -2) continue;
      const bf16_t* xs = reinterpret_cast<const bf16_t*>(&v[u]);
      bf16_t gs[8];
      if (st[u] == -1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) gs[j] = 0;
      } else {
        const int lb = st[u] == 1 ? lab[u] - c0[u] : -1;   // the label's index inside this vector, if it is there
        float gv[8];
        float accv = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float l;
          focal_neg_g2_inr(bf2f(xs[j]), c, cg, l, gv[j]);
          accv += l;
        }
        if (lb >= 0 && lb < 8) {                           // rare: the label element of a positive row
          float xl = bf2f(xs[0]);
#pragma unroll
          for (int j = 1; j < 8; ++j) xl = j == lb ? bf2f(xs[j]) : xl;
          // its target-0 loss leaves the sum again here (the same bits): a select per logit in the loop above
          // is two instructions in twenty of a kernel that is close to VALU-bound
          float ln, gn, l, g;
          focal_neg_g2_inr(xl, c, cg, ln, gn);
          quality_label_elem<bf16_t>(a, row[u], xl, l, g);
          accv += l - ln;
#pragma unroll
          for (int j = 0; j < 8; ++j) gv[j] = j == lb ? g * inv : gv[j];
        }
        acc += accv;
#pragma unroll
        for (int j = 0; j < 8; ++j) gs[j] = f2bf(gv[j]);
      }
      const int o = ld > 0 ? (row[u] / grp) * ld + (row[u] % grp) * C + c0[u] : (base + u * stride) * 8;
      *reinterpret_cast<uint4*>(dlogits + o) = *reinterpret_cast<const uint4*>(gs);
    }
  }
  const float bs = block_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = bs;
}

// Scalar fallback for C not divisible by the vector width.
template <typename T>
__global__ __launch_bounds__(kBlock) void quality_kernel_scalar(const T* __restrict__ logits, QualityArgs a,
                                                                T* __restrict__ dlogits, float* __restrict__ partials,
                                                                long long n, int C) {
  __shared__ float red[16];
  const float inv = 1.0f / fmaxf(1.0f, (float)(*a.npos));
  const float c = a.kind == kVFL ? kVflAlpha : 1.0f;
  float acc = 0.f;
  for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
    const long long row = i / C;
    const int col = (int)(i - row * C);
    const int s = a.state[row];
    float g = 0.f;
    if (s != -1) {
      const float x = Cvt<T>::to_f(logits[i]);
      float l;
      if (s == 1 && a.label[row] == col)
        quality_label_elem<T>(a, row, x, l, g);
      else
        quality_neg_t<T>(x, c, c, l, g);
      acc += l;
    }
    dlogits[i] = Cvt<T>::from_f(g * inv);
  }
  const float bs = block_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = bs;
}

}  // namespace

// kind: 0 = QFL, 1 = VFL.  dtype: 0 = f32, 1 = bf16, of logits, reg and dlogits; reg_t and anchors f32.  anchors:
// [A, 4], rows a multiple of A.  partials must hold mxr_loss_grid() floats; out one float.  grp / ld: as in
// mxr_focal_fwd_bwd.  Returns -1, before any launch, for what it cannot serve.
MXR_API int mxr_quality_loss_fwd_bwd(const void* logits, const void* reg, const float* reg_t, const float* anchors,
                                     const int8_t* state, const int32_t* label, const int* npos, void* dlogits,
                                     float* partials, float* out, long long rows, int C, int A, int kind, int dtype,
                                     int grp, int ld, hipStream_t stream) {
  if (kind != kQFL && kind != kVFL) return -1;
  if (dtype != 0 && dtype != 1) return -1;
  if (rows < 0 || C <= 0 || A <= 0 || rows % A) return -1;
  // grp / ld: write dlogits into a padded [rows / grp][ld] layout (the packed head's 768-wide pixel rows)
  if (ld > 0 && (dtype != 1 || C % 8 || ld % 8 || grp <= 0 || (long long)grp * C > ld || rows % grp)) return -1;
  const long long n = rows * (long long)C;
  const long long nout = ld > 0 ? rows / grp * ld : n;
  const int grid = mxr_loss_grid();
  const size_t esz = dtype == 1 ? 2 : 4;
  QualityArgs a;
  a.reg = reg;
  a.reg_t = reg_t;
  a.anchors = anchors;
  a.state = state;
  a.label = label;
  a.npos = npos;
  a.A = A;
  a.kind = kind;
  a.reg_vec = (uintptr_t)reg % (4 * esz) == 0;
  if (dtype == 1 && C % 8 == 0 && n < 0x7fffffffLL && nout < 0x7fffffffLL) {
    if (C == 80 && (ld <= 0 || grp == 9))
      quality_bf16_kernel<4, 80, 9><<<grid, kBlock, 0, stream>>>((const bf16_t*)logits, a, (bf16_t*)dlogits, partials,
                                                                 (int)(n / 8), C, grp, ld);
    else
      quality_bf16_kernel<4><<<grid, kBlock, 0, stream>>>((const bf16_t*)logits, a, (bf16_t*)dlogits, partials,
                                                          (int)(n / 8), C, grp, ld);
  } else if (dtype == 1 && C % 8 == 0) {
    quality_kernel<bf16_t, 8><<<grid, kBlock, 0, stream>>>((const bf16_t*)logits, a, (bf16_t*)dlogits, partials, n / 8,
                                                           C, grp, ld);
  } else if (dtype == 0 && C % 4 == 0) {
    quality_kernel<float, 4><<<grid, kBlock, 0, stream>>>((const float*)logits, a, (float*)dlogits, partials, n / 4, C,
                                                          0, 0);
  } else if (dtype == 1) {
    quality_kernel_scalar<bf16_t><<<grid, kBlock, 0, stream>>>((const bf16_t*)logits, a, (bf16_t*)dlogits, partials, n,
                                                               C);
  } else {
    quality_kernel_scalar<float><<<grid, kBlock, 0, stream>>>((const float*)logits, a, (float*)dlogits, partials, n, C);
  }
  mxr_loss_finalize_launch(partials, grid, npos, out, stream);
  return (int)hipGetLastError();
}
