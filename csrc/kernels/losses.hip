// Fused sigmoid-focal and smooth-L1 losses: loss partial sums AND input gradients in one pass.  (And the IoU
// regression losses that --regression-loss puts in smooth-L1's place: iou_loss_kernel below.)
//
// Spec: keras-retinanet losses.focal(alpha=0.25, gamma=2) / smooth_l1(sigma=3) compiled at
// /root/reference/train.py:99-102.  Keras evaluates the focal weight on the
// sigmoid probability and the BCE on the probability clipped to [1e-7, 1-1e-7]; in logit space
// that is BCE(clamp(x, LOGIT_LO, LOGIT_HI)) with zero gradient outside the clamp.  Anchors with
// state -1 are dropped; both losses are divided by max(1, #positives of the local batch), read
// from device memory (written by the anchor-target kernel), so nothing syncs with the host.
//
// The classification tensor is B x 200,700 x 80 (16M logits/image) -> memory-bound: every thread
// moves 16 B per load/store (8 bf16 or 4 f32), one read of the logits and one write of dlogits.
#include "common.h"
#include "focal_common.h"

namespace {

constexpr int kBlock = 256;

template <typename T, int V>
struct Vec;
template <> struct Vec<bf16_t, 8> { typedef uint4 type; };
template <> struct Vec<float, 4> { typedef float4 type; };

// focal_elem for fp32 logits.  focal_elem's fp32 log(1 + e) keeps e only to the rounding of 1 + e, and its
// BCE of the positive class, softplus(xc) - xc, cancels: from |x| = 6 on the gradient is off by 1e-5 .. 1e-3 of
// its value.  Rounding to bf16 hides that; an fp32 gradient shows it.  Here the log is log1p, the BCE of the
// positive class is softplus(-xc) summed directly, and exp / pow / the division are the correctly rounded ones:
// a few ulp per element, like the fp32 autograd of the formula.  The fp32 forms are cold (the training path is
// bf16), so the slower library calls cost nothing that matters.
__device__ __forceinline__ void focal_elem_f32(float x, bool y, float alpha, float gamma, bool g2, float lo, float hi,
                                               float& loss, float& grad) {
  const float e = expf(-fabsf(x));
  const float r = 1.0f / (1.0f + e);
  const float p = x >= 0.f ? r : e * r;        // sigmoid(x)
  const float q = x >= 0.f ? e * r : r;        // 1 - sigmoid(x)
  const float xc = fminf(fmaxf(x, lo), hi);
  const bool inr = (x > lo) && (x < hi);
  const float lg = log1pf(inr ? e : expf(-fabsf(xc)));
  if (y) {
    const float qg = g2 ? q * q : powf(q, gamma);
    const float w = alpha * qg;
    const float bce = fmaxf(-xc, 0.f) + lg;    // softplus(-xc)
    const float dw = -alpha * gamma * p * qg;
    loss = w * bce;
    grad = dw * bce + (inr ? -w * q : 0.f);
  } else {
    const float pg = g2 ? p * p : powf(p, gamma);
    const float w = (1.f - alpha) * pg;
    const float bce = fmaxf(xc, 0.f) + lg;     // softplus(xc)
    const float dw = (1.f - alpha) * gamma * pg * q;
    loss = w * bce;
    grad = dw * bce + (inr ? w * p : 0.f);
  }
}

template <typename T>
__device__ __forceinline__ void focal_elem_t(float x, bool y, float alpha, float gamma, bool g2, float lo, float hi,
                                             float& loss, float& grad) {
  if constexpr (sizeof(T) == sizeof(float))
    focal_elem_f32(x, y, alpha, gamma, g2, lo, hi, loss, grad);
  else
    focal_elem(x, y, alpha, gamma, g2, lo, hi, loss, grad);   // bf16: the bits the fused conv epilogue computes
}

// logits/dlogits: [rows, C] row-major; state/label: [rows].
template <typename T, int V>
__global__ __launch_bounds__(kBlock) void focal_kernel(const T* __restrict__ logits, const int8_t* __restrict__ state,
                                                       const int32_t* __restrict__ label, const int* __restrict__ npos,
                                                       T* __restrict__ dlogits, float* __restrict__ partials,
                                                       long long nvec, int C, float alpha, float gamma, float lo,
                                                       float hi, int grp, int ld) {
  __shared__ float red[16];
  const float inv = 1.0f / fmaxf(1.0f, (float)(*npos));
  const bool g2 = gamma == 2.0f;
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
    const int s = state[row];
    VT v = in[i];
    T xs[V];
    *reinterpret_cast<VT*>(xs) = v;
    T gs[V];
    if (s == -1) {
#pragma unroll
      for (int j = 0; j < V; ++j) gs[j] = Cvt<T>::from_f(0.f);
    } else {
      const int lab = (s == 1) ? label[row] : -1;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float l, g;
        focal_elem_t<T>(Cvt<T>::to_f(xs[j]), (c0 + j) == lab, alpha, gamma, g2, lo, hi, l, g);
        acc += l;
        gs[j] = Cvt<T>::from_f(g * inv);
      }
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

// bf16 fast path (32-bit indexing, < 2^31 elements): U independent 16-B vectors in flight per thread
// per iteration -- the one-vector loop above leaves the kernel latency-bound at ~2.4 TB/s.
// CC / GG > 0: the class count C and the anchor group size compile-time constants (80 / 9 for COCO): the
// per-vector row / column and padded-row divisions become multiply-shifts instead of ~40-instruction
// integer divisions.
// G2: gamma == 2 -- focal_neg_g2_inr per logit (the clip bounds are asymmetric in fp32: -16.118 / 15.942).  (With a runtime gamma
// the compiler if-converts the __powf branch of focal_neg and evaluates it -- log, exp, frexp, ldexp, range
// reduction -- for every element: 4x the instructions.)
template <int U, int CC = 0, int GG = 0, bool G2 = false>
__global__ __launch_bounds__(kBlock) void focal_bf16_kernel(const bf16_t* __restrict__ logits,
                                                            const int8_t* __restrict__ state,
                                                            const int32_t* __restrict__ label,
                                                            const int* __restrict__ npos, bf16_t* __restrict__ dlogits,
                                                            float* __restrict__ partials, int nvec, int C_, float alpha,
                                                            float gamma, float lo, float hi, int grp_, int ld) {
  __shared__ float red[16];
  const int C = CC > 0 ? CC : C_;
  const int grp = GG > 0 ? GG : grp_;
  const float inv = 1.0f / fmaxf(1.0f, (float)(*npos));
  const bool g2 = G2 || gamma == 2.0f;
  const float e_lo = __expf(-fabsf(lo)), e_hi = __expf(-fabsf(hi));
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
        st[u] = state[row[u]];
        lab[u] = label[row[u]];
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
        const int lb = st[u] == 1 ? lab[u] - c0[u] : -1;   // the positive class inside this vector, if any
        float gv[8];
        if constexpr (G2) {
          // every logit as a background class inside the clip range; a logit outside it (a confident
          // negative late in training) sends the vector down the exact path (focal_common.h)
          float x8[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) x8[j] = bf2f(xs[j]);
          acc += focal8_g2(x8, lb, alpha, gamma, lo, hi, e_lo, e_hi, inv, gv);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float l;
            focal_neg(bf2f(xs[j]), alpha, gamma, g2, lo, hi, e_lo, e_hi, l, gv[j]);
            acc += j == lb ? 0.f : l;
          }
          if (lb >= 0 && lb < 8) {                        // rare: one element takes the y = 1 branch
            float l, g;
            focal_elem(bf2f(xs[lb]), true, alpha, gamma, g2, lo, hi, l, g);
            acc += l;
#pragma unroll
            for (int j = 0; j < 8; ++j) gv[j] = j == lb ? g : gv[j];
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) gv[j] *= inv;
        }
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
__global__ __launch_bounds__(kBlock) void focal_kernel_scalar(const T* __restrict__ logits, const int8_t* __restrict__ state,
                                                              const int32_t* __restrict__ label, const int* __restrict__ npos,
                                                              T* __restrict__ dlogits, float* __restrict__ partials,
                                                              long long n, int C, float alpha, float gamma, float lo, float hi) {
  __shared__ float red[16];
  const float inv = 1.0f / fmaxf(1.0f, (float)(*npos));
  const bool g2 = gamma == 2.0f;
  float acc = 0.f;
  for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
    const long long row = i / C;
    const int c = (int)(i - row * C);
    const int s = state[row];
    float g = 0.f;
    if (s != -1) {
      float l;
      focal_elem_t<T>(Cvt<T>::to_f(logits[i]), s == 1 && label[row] == c, alpha, gamma, g2, lo, hi, l, g);
      acc += l;
    }
    dlogits[i] = Cvt<T>::from_f(g * inv);
  }
  const float bs = block_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = bs;
}

// Deterministic final reduction: out[0] = sum(partials) / max(1, npos).
__global__ __launch_bounds__(256) void finalize_kernel(const float* __restrict__ partials, int n, const int* __restrict__ npos,
                                                       float* __restrict__ out) {
  __shared__ float red[16];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) acc += partials[i];
  const float s = block_sum(acc, red);
  if (threadIdx.x == 0) out[0] = s / fmaxf(1.0f, (float)(*npos));
}

// Smooth-L1 over positive anchors. pred/dpred: [rows, 4] (T), target: [rows, 4] f32.
template <typename T>
__global__ __launch_bounds__(kBlock) void smooth_l1_kernel(const T* __restrict__ pred, const float* __restrict__ target,
                                                           const int8_t* __restrict__ state, const int* __restrict__ npos,
                                                           T* __restrict__ dpred, float* __restrict__ partials,
                                                           long long rows, float sigma2, int grp, int ld) {
  __shared__ float red[16];
  const float inv = 1.0f / fmaxf(1.0f, (float)(*npos));
  const float thr = 1.0f / sigma2;
  float acc = 0.f;
  for (long long r = blockIdx.x * (long long)kBlock + threadIdx.x; r < rows; r += (long long)gridDim.x * kBlock) {
    T g[4];
    if (state[r] == 1) {
      const float4 t = reinterpret_cast<const float4*>(target)[r];
      const float tt[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = Cvt<T>::to_f(pred[r * 4 + j]) - tt[j];
        const float ad = fabsf(d);
        float l, gr;
        if (ad < thr) {
          l = 0.5f * sigma2 * ad * ad;
          gr = sigma2 * d;
        } else {
          l = ad - 0.5f / sigma2;
          gr = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        }
        acc += l;
        g[j] = Cvt<T>::from_f(gr * inv);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) g[j] = Cvt<T>::from_f(0.f);
    }
    // grp / ld: the packed regression head's zero-padded [rows / grp][ld] gradient rows
    T* d = dpred + (ld > 0 ? (r / grp) * ld + (r % grp) * 4 : r * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = g[j];
  }
  const float bs = block_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = bs;
}

// IoU regression losses over positive anchors: GIoU (Rezatofighi et al. 2019), DIoU / CIoU (Zheng et al. 2020).
// pred / dpred: [rows, 4] (T) corner deltas, target: [rows, 4] f32 deltas, anchors: [A, 4] f32 (x1, y1, x2, y2);
// row r belongs to anchor r % A.  Both boxes are the project's bbox_transform_inv (mean 0, std kBoxStd) of their
// deltas; the predicted one has its corners ordered (the decode is linear, a prediction can flip) and the
// gradient follows every selection: the ordering, pred corner vs target corner, the max(0, .) of the
// intersection.  It comes out in delta units (through std * anchor side) and already / max(1, npos) * weight.
// A row reads its prediction, target and anchor only when it is positive (~1 % of the rows), so the pass is the
// state read plus the gradient write, as in smooth_l1_kernel.
// The boxes are held relative to the anchor's top-left corner: the loss does not change under a translation, and
// coordinates of the anchor's own size keep the fp32 differences (widths, overlaps) a few ulp from exact where
// image coordinates of ~1000 px would cost them 2-3 digits.
enum { kGIoU = 0, kDIoU = 1, kCIoU = 2 };
constexpr float kBoxStd = 0.2f;
constexpr float kIoUEps = 1e-7f;

template <> struct Vec<bf16_t, 4> { typedef uint2 type; };

template <typename T, int KIND>
__global__ __launch_bounds__(kBlock) void iou_loss_kernel(const T* __restrict__ pred, const float* __restrict__ target,
                                                          const float* __restrict__ anchors,
                                                          const int8_t* __restrict__ state, const int* __restrict__ npos,
                                                          T* __restrict__ dpred, float* __restrict__ partials,
                                                          long long rows, int A, float weight, int grp, int ld,
                                                          bool vec) {
  __shared__ float red[16];
  typedef typename Vec<T, 4>::type VT;
  const float gs = weight / fmaxf(1.0f, (float)(*npos));
  const bool small = rows < 0x7fffffffLL;   // 32-bit division (64-bit integer division is emulated on CDNA)
  float acc = 0.f;
  for (long long r = blockIdx.x * (long long)kBlock + threadIdx.x; r < rows; r += (long long)gridDim.x * kBlock) {
    T g[4];
    if (state[r] == 1) {
      const int a = small ? (int)r % A : (int)(r % A);
      const float4 an = reinterpret_cast<const float4*>(anchors)[a];
      const float4 t = reinterpret_cast<const float4*>(target)[r];
      T ps[4];
      if (vec) {
        *reinterpret_cast<VT*>(ps) = reinterpret_cast<const VT*>(pred)[r];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) ps[j] = pred[r * 4 + j];
      }
      const float aw = an.z - an.x, ah = an.w - an.y;
      const float sw = kBoxStd * aw, sh = kBoxStd * ah;
      const float gx1 = sw * t.x, gy1 = sh * t.y, gx2 = aw + sw * t.z, gy2 = ah + sh * t.w;
      const float qx1 = sw * Cvt<T>::to_f(ps[0]), qy1 = sh * Cvt<T>::to_f(ps[1]);
      const float qx2 = aw + sw * Cvt<T>::to_f(ps[2]), qy2 = ah + sh * Cvt<T>::to_f(ps[3]);
      const bool fx = qx1 > qx2, fy = qy1 > qy2;      // flipped: the gradients of (x1, x2) / (y1, y2) change places
      const float px1 = fx ? qx2 : qx1, px2 = fx ? qx1 : qx2, py1 = fy ? qy2 : qy1, py2 = fy ? qy1 : qy2;
      const float pw = px2 - px1, ph = py2 - py1, gw = gx2 - gx1, gh = gy2 - gy1;
      const float iwr = fminf(px2, gx2) - fmaxf(px1, gx1), ihr = fminf(py2, gy2) - fmaxf(py1, gy1);
      const float iw = fmaxf(iwr, 0.f), ih = fmaxf(ihr, 0.f);
      const float I = iw * ih;
      const float U = pw * ph + gw * gh - I + kIoUEps;
      const float rU = 1.0f / U;
      const float iou = I * rU;
      const float cw = fmaxf(px2, gx2) - fminf(px1, gx1), ch = fmaxf(py2, gy2) - fminf(py1, gy1);
      // which corner each selection took: l* -- the prediction's corner bounds the enclosing box, i* -- the
      // intersection (and the intersection is not clamped away)
      const bool lx1 = px1 < gx1, lx2 = px2 > gx2, ly1 = py1 < gy1, ly2 = py2 > gy2;
      const bool ix1 = iwr > 0.f && px1 > gx1, ix2 = iwr > 0.f && px2 < gx2;
      const bool iy1 = ihr > 0.f && py1 > gy1, iy2 = ihr > 0.f && py2 < gy2;
      // d / d(px1, px2, py1, py2) of I and of U
      const float dI[4] = {ix1 ? -ih : 0.f, ix2 ? ih : 0.f, iy1 ? -iw : 0.f, iy2 ? iw : 0.f};
      const float dU[4] = {-ph - dI[0], ph - dI[1], -pw - dI[2], pw - dI[3]};
      float G[4];     // d L / d(px1, px2, py1, py2)
#pragma unroll
      for (int j = 0; j < 4; ++j) G[j] = (iou * dU[j] - dI[j]) * rU;     // -d IoU
      float L;
      if constexpr (KIND == kGIoU) {
        const float C = cw * ch + kIoUEps;
        const float rC = 1.0f / C;
        const float uc = U * rC;
        L = 1.0f - iou + (C - U) * rC;
        const float dC[4] = {lx1 ? -ch : 0.f, lx2 ? ch : 0.f, ly1 ? -cw : 0.f, ly2 ? cw : 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) G[j] -= (dU[j] - uc * dC[j]) * rC;   // -d (U / C)
      } else {
        const float c2 = cw * cw + ch * ch + kIoUEps;
        const float rc2 = 1.0f / c2;
        const float sx = (px1 + px2) - (gx1 + gx2), sy = (py1 + py2) - (gy1 + gy2);
        const float rr = 0.25f * (sx * sx + sy * sy) * rc2;
        L = 1.0f - iou + rr;
        const float dc2[4] = {lx1 ? -2.f * cw : 0.f, lx2 ? 2.f * cw : 0.f, ly1 ? -2.f * ch : 0.f, ly2 ? 2.f * ch : 0.f};
        const float drho2[4] = {0.5f * sx, 0.5f * sx, 0.5f * sy, 0.5f * sy};
#pragma unroll
        for (int j = 0; j < 4; ++j) G[j] += (drho2[j] - rr * dc2[j]) * rc2;
        if constexpr (KIND == kCIoU) {
          const float php = ph + kIoUEps, ghp = gh + kIoUEps;
          const float at = atanf(gw / ghp) - atanf(pw / php);
          const float v = 0.40528473456935108578f * at * at;             // 4 / pi^2
          const float alpha = v / (1.0f - iou + v + kIoUEps);            // a constant in the backward
          L += alpha * v;
          const float k = alpha * 0.81056946913870217155f * at / (php * php + pw * pw);   // 8 / pi^2
          G[0] += k * php;     // d v / d pw = -k php / alpha, d pw / d px1 = -1
          G[1] -= k * php;
          G[2] -= k * pw;      // d v / d ph = k pw / alpha
          G[3] += k * pw;
        }
      }
      acc += weight * L;
      const float kx = gs * sw, ky = gs * sh;
      g[0] = Cvt<T>::from_f(kx * (fx ? G[1] : G[0]));
      g[1] = Cvt<T>::from_f(ky * (fy ? G[3] : G[2]));
      g[2] = Cvt<T>::from_f(kx * (fx ? G[0] : G[1]));
      g[3] = Cvt<T>::from_f(ky * (fy ? G[2] : G[3]));
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) g[j] = Cvt<T>::from_f(0.f);
    }
    // grp / ld: the packed regression head's zero-padded [rows / grp][ld] gradient rows
    long long o = r * 4;
    if (ld > 0) {
      if (small) {
        const int q = (int)r / grp;
        o = q * (long long)ld + ((int)r - q * grp) * 4;
      } else {
        o = (r / grp) * ld + (r % grp) * 4;
      }
    }
    if (vec) {
      *reinterpret_cast<VT*>(dpred + o) = *reinterpret_cast<const VT*>(g);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) dpred[o + j] = g[j];
    }
  }
  const float bs = block_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = bs;
}

constexpr int kLossGrid = 2048;

template <typename T>
void iou_loss_launch(int kind, const void* pred, const float* target, const float* anchors, const int8_t* state,
                     const int* npos, void* dpred, float* partials, long long rows, int A, float weight, int grp,
                     int ld, hipStream_t stream) {
  // one 8-B (bf16) / 16-B (f32) access per row where every row starts on such a boundary
  const bool vec = ld % 4 == 0 && ((uintptr_t)pred | (uintptr_t)dpred) % (4 * sizeof(T)) == 0;
  const T* p = (const T*)pred;
  T* d = (T*)dpred;
  if (kind == kGIoU)
    iou_loss_kernel<T, kGIoU><<<kLossGrid, kBlock, 0, stream>>>(p, target, anchors, state, npos, d, partials, rows, A,
                                                                weight, grp, ld, vec);
  else if (kind == kDIoU)
    iou_loss_kernel<T, kDIoU><<<kLossGrid, kBlock, 0, stream>>>(p, target, anchors, state, npos, d, partials, rows, A,
                                                                weight, grp, ld, vec);
  else
    iou_loss_kernel<T, kCIoU><<<kLossGrid, kBlock, 0, stream>>>(p, target, anchors, state, npos, d, partials, rows, A,
                                                                weight, grp, ld, vec);
}

}  // namespace

// dtype: 0 = f32, 1 = bf16.  partials must hold kLossGrid floats; out one float.
MXR_API int mxr_focal_fwd_bwd(const void* logits, const int8_t* state, const int32_t* label, const int* npos,
                              void* dlogits, float* partials, float* out, long long rows, int C, float alpha,
                              float gamma, float lo, float hi, int dtype, int grp, int ld, hipStream_t stream) {
  const long long n = rows * (long long)C;
  // grp / ld: write dlogits into a padded [rows / grp][ld] layout (the packed head's 768-wide pixel rows)
  if (ld > 0 && (dtype != 1 || C % 8 || grp <= 0 || (long long)grp * C > ld || rows % grp)) return -1;
  const long long nout = ld > 0 ? rows / (grp > 0 ? grp : 1) * ld : n;
  if (dtype == 1 && C % 8 == 0 && n < 0x7fffffffLL && nout < 0x7fffffffLL) {
    if (C == 80 && (ld <= 0 || grp == 9) && gamma == 2.0f)
      focal_bf16_kernel<4, 80, 9, true><<<kLossGrid, kBlock, 0, stream>>>((const bf16_t*)logits, state, label, npos,
                                                                          (bf16_t*)dlogits, partials, (int)(n / 8), C,
                                                                          alpha, gamma, lo, hi, grp, ld);
    else if (C == 80 && (ld <= 0 || grp == 9))
      focal_bf16_kernel<4, 80, 9><<<kLossGrid, kBlock, 0, stream>>>((const bf16_t*)logits, state, label, npos,
                                                                    (bf16_t*)dlogits, partials, (int)(n / 8), C, alpha,
                                                                    gamma, lo, hi, grp, ld);
    else
      focal_bf16_kernel<4><<<kLossGrid, kBlock, 0, stream>>>((const bf16_t*)logits, state, label, npos,
                                                             (bf16_t*)dlogits, partials, (int)(n / 8), C, alpha, gamma,
                                                             lo, hi, grp, ld);
  } else if (dtype == 1 && C % 8 == 0) {
    const long long nvec = n / 8;
    focal_kernel<bf16_t, 8><<<kLossGrid, kBlock, 0, stream>>>((const bf16_t*)logits, state, label, npos,
                                                              (bf16_t*)dlogits, partials, nvec, C, alpha, gamma, lo, hi,
                                                              grp, ld);
  } else if (dtype == 0 && C % 4 == 0) {
    const long long nvec = n / 4;
    focal_kernel<float, 4><<<kLossGrid, kBlock, 0, stream>>>((const float*)logits, state, label, npos,
                                                             (float*)dlogits, partials, nvec, C, alpha, gamma, lo, hi,
                                                             0, 0);
  } else if (dtype == 1) {
    focal_kernel_scalar<bf16_t><<<kLossGrid, kBlock, 0, stream>>>((const bf16_t*)logits, state, label, npos,
                                                                  (bf16_t*)dlogits, partials, n, C, alpha, gamma, lo, hi);
  } else {
    focal_kernel_scalar<float><<<kLossGrid, kBlock, 0, stream>>>((const float*)logits, state, label, npos,
                                                                 (float*)dlogits, partials, n, C, alpha, gamma, lo, hi);
  }
  finalize_kernel<<<1, 256, 0, stream>>>(partials, kLossGrid, npos, out);
  return (int)hipGetLastError();
}

MXR_API int mxr_smooth_l1_fwd_bwd(const void* pred, const float* target, const int8_t* state, const int* npos,
                                  void* dpred, float* partials, float* out, long long rows, float sigma, int dtype,
                                  int grp, int ld, hipStream_t stream) {
  const float s2 = sigma * sigma;
  if (ld > 0 && (grp <= 0 || 4LL * grp > ld || rows % grp)) return -1;
  if (dtype == 1)
    smooth_l1_kernel<bf16_t><<<kLossGrid, kBlock, 0, stream>>>((const bf16_t*)pred, target, state, npos,
                                                               (bf16_t*)dpred, partials, rows, s2, grp, ld);
  else
    smooth_l1_kernel<float><<<kLossGrid, kBlock, 0, stream>>>((const float*)pred, target, state, npos,
                                                              (float*)dpred, partials, rows, s2, grp, ld);
  finalize_kernel<<<1, 256, 0, stream>>>(partials, kLossGrid, npos, out);
  return (int)hipGetLastError();
}

// kind: 0 = GIoU, 1 = DIoU, 2 = CIoU.  anchors: [A, 4] f32; rows must be a multiple of A.  Everything else as in
// mxr_smooth_l1_fwd_bwd.
MXR_API int mxr_iou_loss_fwd_bwd(const void* pred, const float* target, const float* anchors, const int8_t* state,
                                 const int* npos, void* dpred, float* partials, float* out, long long rows, int A,
                                 int kind, float weight, int dtype, int grp, int ld, hipStream_t stream) {
  if (ld > 0 && (grp <= 0 || 4LL * grp > ld || rows % grp)) return -1;
  if (A <= 0 || rows % A || kind < kGIoU || kind > kCIoU) return -1;
  if (dtype == 1)
    iou_loss_launch<bf16_t>(kind, pred, target, anchors, state, npos, dpred, partials, rows, A, weight, grp, ld, stream);
  else
    iou_loss_launch<float>(kind, pred, target, anchors, state, npos, dpred, partials, rows, A, weight, grp, ld, stream);
  finalize_kernel<<<1, 256, 0, stream>>>(partials, kLossGrid, npos, out);
  return (int)hipGetLastError();
}

MXR_API int mxr_loss_grid() { return kLossGrid; }

// the fixed-order final reduction of n loss partials (the focal epilogue of conv_hx32.hip / conv_hx32_f8.hip)
void mxr_loss_finalize_launch(const float* partials, int n, const int* npos, float* out, hipStream_t stream) {
  finalize_kernel<<<1, 256, 0, stream>>>(partials, n, npos, out);
}
