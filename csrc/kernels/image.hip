// Device-side image preprocessing for real-data training: caffe/tf normalisation, affine warp and
// bilinear resize into the zero-padded NHWC batch.
//
// Spec: keras-retinanet Generator.preprocess_group_entry = preprocess_image (caffe BGR mean
// subtraction) -> random affine (cv2.warpAffine, TransformParameters fill_mode/interpolation/cval)
// -> resize_image (cv2.resize INTER_LINEAR) -> compute_inputs (zero pad, top-left) (SURVEY §2.2
// E-KR-image/E-KR-transform, K22; reached from /root/reference/train.py:179-193).  The sampling
// arithmetic matches csrc/cpu/runtime_cpu.cpp (mxr_cpu_warp_affine / mxr_cpu_resize_bilinear) so the
// host and device paths agree to float rounding; tests/test_kernels_gpu.py pins that.
//
// Layout: images are HWC with 3 channels (BGR); one thread per output pixel writes its 3 channels (the evaluation
// and training batch builders at the end: 4 / 8 consecutive pixels of a row per thread, a whole batch per launch).
// Coordinates are computed in double exactly as the host path does (the warp's inverse matrix is
// formed on the host in double and passed by value).
#include "common.h"

namespace {
constexpr int kBlock = 256;

__device__ __forceinline__ int border_index(int i, int n, int mode, bool& outside) {
  outside = false;
  if (i >= 0 && i < n) return i;
  switch (mode) {
    case 1: return i < 0 ? 0 : n - 1;
    case 2: {
      if (n == 1) return 0;
      const int p = 2 * (n - 1);
      i = ((i % p) + p) % p;
      return i < n ? i : p - i;
    }
    case 3: return ((i % n) + n) % n;
    default: outside = true; return 0;
  }
}

struct Norm { float scale, m0, m1, m2; };

__device__ __forceinline__ float norm_px(const uint8_t* p, int c, const Norm& nm) {
  const float m = c == 0 ? nm.m0 : (c == 1 ? nm.m1 : nm.m2);
  return (float)p[c] * nm.scale - m;
}

// The inverse 2x3 affine of a warp (dst -> src), formed on the host in double.
struct Affine { double a, b, c, d, e, f; };

// Minv of the forward (src -> dst) matrix M, as cv2.warpAffine inverts it; a singular M gives the zero map.
inline Affine invert_affine(const double* M) {
  const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5];
  double det = a * e - b * d;
  det = det != 0 ? 1.0 / det : 0.0;
  Affine r;
  r.a = e * det; r.b = -b * det; r.d = -d * det; r.e = a * det;
  r.c = -(r.a * c + r.b * f); r.f = -(r.d * c + r.e * f);
  return r;
}

// The arithmetic the per-image kernels and the one-launch training kernel share.  Each piece is one inlined
// function, so every caller compiles the same expressions under the same contraction rules: the fused kernel is
// bit-identical to warp_norm_kernel followed by resize_kernel by construction.

// o[0..2] = normalise(src)[Minv * (x, y)]: nearest (llround) or bilinear, border modes as border_index, cval
// (un-normalised) for taps outside under the constant border.
__device__ __forceinline__ void warp_sample(const uint8_t* __restrict__ src, int H, int W, int x, int y,
                                            const Affine& m, int interp, int border, float cval, const Norm& nm,
                                            float* o) {
  const double sxf = m.a * x + m.b * y + m.c;
  const double syf = m.d * x + m.e * y + m.f;
  if (interp == 0) {
    bool o1, o2;
    const int xi = border_index((int)llround(sxf), W, border, o1);
    const int yi = border_index((int)llround(syf), H, border, o2);
    const uint8_t* p = src + ((long long)yi * W + xi) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (o1 || o2) ? cval : norm_px(p, c, nm);
    return;
  }
  const int x0 = (int)floor(sxf), y0 = (int)floor(syf);
  const float tx = (float)(sxf - x0), ty = (float)(syf - y0);
  bool ox0, ox1, oy0, oy1;
  const int xa = border_index(x0, W, border, ox0), xb = border_index(x0 + 1, W, border, ox1);
  const int ya = border_index(y0, H, border, oy0), yb = border_index(y0 + 1, H, border, oy1);
  const uint8_t* p00 = src + ((long long)ya * W + xa) * 3;
  const uint8_t* p01 = src + ((long long)ya * W + xb) * 3;
  const uint8_t* p10 = src + ((long long)yb * W + xa) * 3;
  const uint8_t* p11 = src + ((long long)yb * W + xb) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v00 = (ox0 || oy0) ? cval : norm_px(p00, c, nm);
    const float v01 = (ox1 || oy0) ? cval : norm_px(p01, c, nm);
    const float v10 = (ox0 || oy1) ? cval : norm_px(p10, c, nm);
    const float v11 = (ox1 || oy1) ? cval : norm_px(p11, c, nm);
    const float top = v00 + (v01 - v00) * tx, bot = v10 + (v11 - v10) * tx;
    o[c] = top + (bot - top) * ty;
  }
}

// cv2.resize INTER_LINEAR taps of output index o along an axis of n source / scale s = n / out: half-pixel
// centres, edge clamp.
struct Tap { int i, j; float t; };
__device__ __forceinline__ Tap resize_tap(int o, double s, int n) {
  const double f = (o + 0.5) * s - 0.5;
  int i = (int)floor(f);
  double t = f - i;
  if (i < 0) { i = 0; t = 0; }
  if (i >= n - 1) { i = n - 1; t = 0; }
  Tap r;
  r.i = i; r.j = min(i + 1, n - 1); r.t = (float)t;
  return r;
}

// the two lerps of the resize on its four taps (a b / c e)
__device__ __forceinline__ float resize_lerp(float a, float b, float c, float e, float tx, float ty) {
  const float top = a + (b - a) * tx;
  const float bot = c + (e - c) * tx;
  return top + (bot - top) * ty;
}

// dst[y, x, c] = normalise(src)[Minv * (x, y)] (bilinear or nearest), or plain normalise when warp == 0
__global__ __launch_bounds__(kBlock) void warp_norm_kernel(const uint8_t* __restrict__ src, int H, int W,
                                                           float* __restrict__ dst, int OH, int OW, Affine m, int warp,
                                                           int interp, int border, float cval, Norm nm) {
  const long long total = (long long)OH * OW;
  for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
    const int x = (int)(i % OW), y = (int)(i / OW);
    float* o = dst + i * 3;
    if (!warp) {
      const uint8_t* p = src + i * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = norm_px(p, c, nm);
      continue;
    }
    float v[3];
    warp_sample(src, H, W, x, y, m, interp, border, cval, nm, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = v[c];
  }
}

// cv2.resize INTER_LINEAR (half-pixel centres, edge clamp) of an HWC float image into a batch slot
// with row pitch ld (elements); the padding of the slot is left untouched (pre-zeroed).
template <typename T>
__global__ __launch_bounds__(kBlock) void resize_kernel(const float* __restrict__ src, int H, int W,
                                                        T* __restrict__ dst, int OH, int OW, long long ld) {
  const double sy = (double)H / OH, sx = (double)W / OW;
  const long long total = (long long)OH * OW;
  for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
    const int x = (int)(i % OW), y = (int)(i / OW);
    const Tap tx = resize_tap(x, sx, W), ty = resize_tap(y, sy, H);
    const float* a = src + ((long long)ty.i * W + tx.i) * 3;
    const float* b = src + ((long long)ty.i * W + tx.j) * 3;
    const float* c = src + ((long long)ty.j * W + tx.i) * 3;
    const float* e = src + ((long long)ty.j * W + tx.j) * 3;
    T* o = dst + (long long)y * ld + (long long)x * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) o[ch] = Cvt<T>::from_f(resize_lerp(a[ch], b[ch], c[ch], e[ch], tx.t, ty.t));
  }
}

// ---- evaluation batch builder: normalise + cv2.resize INTER_LINEAR + zero pad, a whole batch per launch ----
constexpr int kMaxBatchImages = 32;
struct ImageDesc { long long off; int H, W, OH, OW; };
struct ImageTable { ImageDesc d[kMaxBatchImages]; };   // passed by value (768 B of kernel arguments)

// PX consecutive pixels (3*PX values) of one row as three 16-byte words
template <typename T> struct Px;
template <> struct Px<float> {
  static constexpr int N = 4;
  __device__ __forceinline__ static void store16(float* o, const float* v) {
#pragma unroll
    for (int q = 0; q < 3; ++q)
      reinterpret_cast<float4*>(o)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
  }
};
template <> struct Px<bf16_t> {
  static constexpr int N = 8;
  __device__ __forceinline__ static uint32_t pk(const bf16_t* v) { return (uint32_t)v[0] | ((uint32_t)v[1] << 16); }
  __device__ __forceinline__ static void store16(bf16_t* o, const bf16_t* v) {
#pragma unroll
    for (int q = 0; q < 3; ++q)
      reinterpret_cast<uint4*>(o)[q] = make_uint4(pk(v + 8 * q), pk(v + 8 * q + 2), pk(v + 8 * q + 4), pk(v + 8 * q + 6));
  }
};

// grid (row chunks, slot).  A work item is Px<T>::N consecutive pixels of one slot row: the row taps and ty are
// computed once per item, every value of the slot -- image, zero padding, empty slot -- is written exactly once
// (the batch needs no zero fill), and the item leaves as three 16-byte stores when VEC (row pitch a multiple of
// 16 bytes: every item is whole and aligned).  Per value the arithmetic is warp_norm_kernel (warp == 0) followed
// by resize_kernel: the same double coordinates and clamps, norm_px on each tap, the same lerp expressions.
template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void batch_resize_norm_kernel(const uint8_t* __restrict__ staging, ImageTable tab,
                                                                   int n_images, T* __restrict__ batch, int Hm, int Wm,
                                                                   Norm nm) {
  constexpr int PX = Px<T>::N;
  const int slot = blockIdx.y;
  int H = 1, W = 1, OH = 0, OW = 0;
  const uint8_t* src = staging;
  if (slot < n_images) {
    const ImageDesc d = tab.d[slot];
    src = staging + d.off; H = d.H; W = d.W; OH = d.OH; OW = d.OW;
  }
  const double sy = OH > 0 ? (double)H / OH : 0.0, sx = OW > 0 ? (double)W / OW : 0.0;
  const long long ld = (long long)Wm * 3;
  T* base = batch + (long long)slot * Hm * ld;
  const int cpr = (Wm + PX - 1) / PX;
  const int items = Hm * cpr;
  const T zero = Cvt<T>::from_f(0.f);
  for (int it = blockIdx.x * kBlock + threadIdx.x; it < items; it += gridDim.x * kBlock) {
    const int y = it / cpr, x0 = (it - y * cpr) * PX;
    T v[PX * 3];
#pragma unroll
    for (int e = 0; e < PX * 3; ++e) v[e] = zero;
    if (y < OH && x0 < OW) {
      const Tap ty = resize_tap(y, sy, H);
      const uint8_t* r0 = src + (long long)ty.i * W * 3;
      const uint8_t* r1 = src + (long long)ty.j * W * 3;
#pragma unroll
      for (int p = 0; p < PX; ++p) {
        const int x = x0 + p;
        if (x < OW) {
          const Tap tx = resize_tap(x, sx, W);
          const uint8_t* a = r0 + tx.i * 3;
          const uint8_t* b = r0 + tx.j * 3;
          const uint8_t* c = r1 + tx.i * 3;
          const uint8_t* e = r1 + tx.j * 3;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch)
            v[p * 3 + ch] = Cvt<T>::from_f(resize_lerp(norm_px(a, ch, nm), norm_px(b, ch, nm), norm_px(c, ch, nm),
                                                       norm_px(e, ch, nm), tx.t, ty.t));
        }
      }
    }
    T* o = base + (long long)y * ld + (long long)x0 * 3;
    if (VEC) {
      Px<T>::store16(o, v);
    } else {
      const int left = (Wm - x0) * 3;
#pragma unroll
      for (int e = 0; e < PX * 3; ++e)
        if (e < left) o[e] = v[e];
    }
  }
}

template <typename T>
int launch_batch_resize_norm(const uint8_t* staging, const ImageTable& tab, int n_images, void* batch, int B, int Hm,
                             int Wm, Norm nm, hipStream_t stream) {
  constexpr int PX = Px<T>::N;
  const long long items = (long long)Hm * ((Wm + PX - 1) / PX);
  if (items > 0x7fffffffLL - 16384LL * kBlock) return -4;
  const dim3 grid(mxr_grid(items, kBlock, 4096), B);
  const bool vec = ((long long)Wm * 3 * sizeof(T)) % 16 == 0 && ((uintptr_t)batch) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL((batch_resize_norm_kernel<T, true>), grid, dim3(kBlock), 0, stream, staging, tab, n_images,
                       (T*)batch, Hm, Wm, nm);
  else
    hipLaunchKernelGGL((batch_resize_norm_kernel<T, false>), grid, dim3(kBlock), 0, stream, staging, tab, n_images,
                       (T*)batch, Hm, Wm, nm);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// ---- training batch builder: normalise + affine warp + cv2.resize INTER_LINEAR + zero pad, a whole batch per launch ----
struct WarpImageDesc { long long off; int H, W, OH, OW; int has_matrix; Affine inv; };   // 80 B
struct WarpImageTable { WarpImageDesc d[kMaxBatchImages]; };   // passed by value: 2560 B of the 4 KiB of kernel arguments

// One resize tap (xx, yy) of the warped, normalised image at source size: what warp_norm_kernel writes at (yy, xx),
// kept in registers.
__device__ __forceinline__ void warp_tap(const uint8_t* __restrict__ src, int H, int W, int xx, int yy, bool warp,
                                         const Affine& m, int interp, int border, float cval, const Norm& nm, float* o) {
  if (!warp) {
    const uint8_t* p = src + ((long long)yy * W + xx) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = norm_px(p, c, nm);
    return;
  }
  warp_sample(src, H, W, xx, yy, m, interp, border, cval, nm, o);
}

// A block works on tiles of kTileRows slot rows x kTileItems work items; the warped source pixels a tile's resize
// taps can name (a rectangle, the taps being monotonic) are staged in LDS when they fit.
constexpr int kTileRows = 8, kTileItems = kBlock / kTileRows;
constexpr int kTileSamples = 2730;   // 32 KiB of 3 x fp32

// The work item of batch_resize_norm_kernel (Px<T>::N consecutive pixels of one slot row, every value of the slot
// written once, three 16-byte stores per item when VEC) on a grid of (tiles, slot); a block takes whole tiles so
// that its threads share source pixels.  Per value the arithmetic is warp_norm_kernel followed by resize_kernel:
// each of the four resize taps is the warp sample of that source pixel (warp_sample, or norm_px alone for a slot
// without a matrix -- uniform over the block) and resize_lerp runs on the four fp32 values.  The fp32 warp value
// never reaches memory: a block evaluates each source pixel of its tile once into LDS, since up-sampling names
// every source pixel from several output pixels (evaluating the four taps per output pixel instead cost 4-9x the
// kernel time at 480x640 -> 800x1067); a tile whose source rectangle does not fit (strong down-sampling) evaluates
// its taps in registers.  interp / border / cval are batch-wide.
template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void batch_warp_resize_norm_kernel(const uint8_t* __restrict__ staging,
                                                                        WarpImageTable tab, int n_images,
                                                                        T* __restrict__ batch, int Hm, int Wm, int interp,
                                                                        int border, float cval, Norm nm) {
  constexpr int PX = Px<T>::N;
  __shared__ float tile[kTileSamples * 3];
  const int slot = blockIdx.y;
  int H = 1, W = 1, OH = 0, OW = 0;
  bool warp = false;
  Affine m = {0, 0, 0, 0, 0, 0};
  const uint8_t* src = staging;
  if (slot < n_images) {
    const WarpImageDesc& d = tab.d[slot];
    src = staging + d.off; H = d.H; W = d.W; OH = d.OH; OW = d.OW;
    warp = d.has_matrix != 0; m = d.inv;
  }
  const double sy = OH > 0 ? (double)H / OH : 0.0, sx = OW > 0 ? (double)W / OW : 0.0;
  const long long ld = (long long)Wm * 3;
  T* base = batch + (long long)slot * Hm * ld;
  const int cpr = (Wm + PX - 1) / PX;
  const int ntx = (cpr + kTileItems - 1) / kTileItems, nty = (Hm + kTileRows - 1) / kTileRows;
  const int ir = threadIdx.x / kTileItems, ic = threadIdx.x % kTileItems;
  const T zero = Cvt<T>::from_f(0.f);
  for (int t = blockIdx.x; t < ntx * nty; t += gridDim.x) {      // uniform over the block (barriers inside)
    const int tr = t / ntx, tc = t - tr * ntx;
    const int ya = tr * kTileRows, xa = tc * kTileItems * PX;    // the tile's first row and pixel
    int r0 = 0, c0 = 0, nr = 0, nc = 0;
    bool staged = false;
    if (warp && ya < OH && xa < OW) {
      const int yb = min(ya + kTileRows, OH) - 1, xb = min(xa + kTileItems * PX, OW) - 1;
      r0 = resize_tap(ya, sy, H).i; nr = resize_tap(yb, sy, H).j - r0 + 1;
      c0 = resize_tap(xa, sx, W).i; nc = resize_tap(xb, sx, W).j - c0 + 1;
      staged = (long long)nr * nc <= kTileSamples;
    }
    if (staged) {
      for (int s = threadIdx.x; s < nr * nc; s += kBlock) {
        const int r = s / nc, c = s - r * nc;
        float v[3];
        warp_sample(src, H, W, c0 + c, r0 + r, m, interp, border, cval, nm, v);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) tile[3 * s + ch] = v[ch];
      }
    }
    __syncthreads();
    const int y = ya + ir, item = tc * kTileItems + ic, x0 = item * PX;
    if (y < Hm && item < cpr) {
      T v[PX * 3];
#pragma unroll
      for (int e = 0; e < PX * 3; ++e) v[e] = zero;
      if (y < OH && x0 < OW) {
        const Tap ty = resize_tap(y, sy, H);
#pragma unroll
        for (int p = 0; p < PX; ++p) {
          const int x = x0 + p;
          if (x < OW) {
            const Tap tx = resize_tap(x, sx, W);
            float a[3], b[3], c[3], e[3];
            if (staged) {
              const int q0 = (ty.i - r0) * nc - c0, q1 = (ty.j - r0) * nc - c0;
#pragma unroll
              for (int ch = 0; ch < 3; ++ch) {
                a[ch] = tile[3 * (q0 + tx.i) + ch]; b[ch] = tile[3 * (q0 + tx.j) + ch];
                c[ch] = tile[3 * (q1 + tx.i) + ch]; e[ch] = tile[3 * (q1 + tx.j) + ch];
              }
            } else {
              warp_tap(src, H, W, tx.i, ty.i, warp, m, interp, border, cval, nm, a);
              warp_tap(src, H, W, tx.j, ty.i, warp, m, interp, border, cval, nm, b);
              warp_tap(src, H, W, tx.i, ty.j, warp, m, interp, border, cval, nm, c);
              warp_tap(src, H, W, tx.j, ty.j, warp, m, interp, border, cval, nm, e);
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
              v[p * 3 + ch] = Cvt<T>::from_f(resize_lerp(a[ch], b[ch], c[ch], e[ch], tx.t, ty.t));
          }
        }
      }
      T* o = base + (long long)y * ld + (long long)x0 * 3;
      if (VEC) {
        Px<T>::store16(o, v);
      } else {
        const int left = (Wm - x0) * 3;
#pragma unroll
        for (int e = 0; e < PX * 3; ++e)
          if (e < left) o[e] = v[e];
      }
    }
    __syncthreads();      // the next tile's staging overwrites what this tile read
  }
}

template <typename T>
int launch_batch_warp_resize_norm(const uint8_t* staging, const WarpImageTable& tab, int n_images, void* batch, int B,
                                  int Hm, int Wm, int interp, int border, float cval, Norm nm, hipStream_t stream) {
  constexpr int PX = Px<T>::N;
  const int cpr = (Wm + PX - 1) / PX;
  const long long tiles = (long long)((cpr + kTileItems - 1) / kTileItems) * ((Hm + kTileRows - 1) / kTileRows);
  if ((long long)Hm * cpr > 0x7fffffffLL - 16384LL * kBlock) return -4;
  const dim3 grid((unsigned)(tiles < 4096 ? tiles : 4096), B);
  const bool vec = ((long long)Wm * 3 * sizeof(T)) % 16 == 0 && ((uintptr_t)batch) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL((batch_warp_resize_norm_kernel<T, true>), grid, dim3(kBlock), 0, stream, staging, tab, n_images,
                       (T*)batch, Hm, Wm, interp, border, cval, nm);
  else
    hipLaunchKernelGGL((batch_warp_resize_norm_kernel<T, false>), grid, dim3(kBlock), 0, stream, staging, tab,
                       n_images, (T*)batch, Hm, Wm, interp, border, cval, nm);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
}  // namespace

// The training batch in one launch: image i (uint8 BGR HWC at staging + off, H x W) is normalised, warped at its own
// size by the forward 2x3 affine matrices[6 * i ..] (cv2.warpAffine; skipped when the row's has_matrix is 0),
// resized to OH x OW and written to the top-left of slot i of the (B, Hm, Wm, 3) batch; the rest of the slot and
// the slots >= n_images are written as zero.  table: n_images rows {byte offset, H, W, OH, OW, has_matrix} and
// matrices: n_images rows of 6 doubles, both in HOST memory (copied into the launch).  dtype: 0 fp32 batch, 1 bf16
// batch.  interp: 0 nearest, 1 linear; border: 0 constant (cval), 1 nearest, 2 reflect, 3 wrap.  At most 32 slots
// per call.
MXR_API int mxr_image_batch_warp_resize_normalize(const uint8_t* staging, long long staging_bytes,
                                                  const long long* table, const double* matrices, int n_images,
                                                  void* batch, int B, int Hm, int Wm, int dtype, int interp, int border,
                                                  float cval, float scale, float m0, float m1, float m2,
                                                  hipStream_t stream) {
  static_assert(sizeof(WarpImageDesc) == 80 && sizeof(WarpImageTable) + 64 <= 4096, "kernel arguments must fit 4 KiB");
  if (B <= 0 || B > kMaxBatchImages || n_images < 0 || n_images > B || Hm <= 0 || Wm <= 0) return -1;
  if (interp < 0 || interp > 1 || border < 0 || border > 3 || (dtype != 0 && dtype != 1)) return -1;
  WarpImageTable tab = {};
  for (int i = 0; i < n_images; ++i) {
    const long long* r = table + 6 * i;
    if (r[1] <= 0 || r[2] <= 0 || r[3] <= 0 || r[4] <= 0 || r[3] > Hm || r[4] > Wm || r[1] > 0x7fffffffLL / 3 / r[2])
      return -2;
    if (r[0] < 0 || r[0] + r[1] * r[2] * 3 > staging_bytes) return -2;
    WarpImageDesc& d = tab.d[i];
    d.off = r[0]; d.H = (int)r[1]; d.W = (int)r[2]; d.OH = (int)r[3]; d.OW = (int)r[4];
    d.has_matrix = r[5] != 0;
    if (d.has_matrix) d.inv = invert_affine(matrices + 6 * i);
  }
  const Norm nm{scale, m0, m1, m2};
  if (dtype == 0)
    return launch_batch_warp_resize_norm<float>(staging, tab, n_images, batch, B, Hm, Wm, interp, border, cval, nm,
                                                stream);
  return launch_batch_warp_resize_norm<bf16_t>(staging, tab, n_images, batch, B, Hm, Wm, interp, border, cval, nm,
                                               stream);
}

// The evaluation batch in one launch: image i (uint8 BGR HWC at staging + off, H x W) is normalised, resized to
// OH x OW and written to the top-left of slot i of the (B, Hm, Wm, 3) batch; the rest of the slot and the slots
// >= n_images are written as zero.  table: n_images rows {byte offset, H, W, OH, OW} in HOST memory (copied into
// the launch).  dtype: 0 fp32 batch, 1 bf16 batch.  At most 32 slots per call.
MXR_API int mxr_image_batch_resize_normalize(const uint8_t* staging, long long staging_bytes, const long long* table,
                                             int n_images, void* batch, int B, int Hm, int Wm, int dtype, float scale,
                                             float m0, float m1, float m2, hipStream_t stream) {
  if (B <= 0 || B > kMaxBatchImages || n_images < 0 || n_images > B || Hm <= 0 || Wm <= 0) return -1;
  ImageTable tab = {};
  for (int i = 0; i < n_images; ++i) {
    const long long* r = table + 5 * i;
    if (r[1] <= 0 || r[2] <= 0 || r[3] <= 0 || r[4] <= 0 || r[3] > Hm || r[4] > Wm || r[1] > 0x7fffffffLL / 3 / r[2])
      return -2;
    if (r[0] < 0 || r[0] + r[1] * r[2] * 3 > staging_bytes) return -2;
    tab.d[i] = ImageDesc{r[0], (int)r[1], (int)r[2], (int)r[3], (int)r[4]};
  }
  const Norm nm{scale, m0, m1, m2};
  if (dtype == 0) return launch_batch_resize_norm<float>(staging, tab, n_images, batch, B, Hm, Wm, nm, stream);
  if (dtype == 1) return launch_batch_resize_norm<bf16_t>(staging, tab, n_images, batch, B, Hm, Wm, nm, stream);
  return -1;
}

// M is the 2x3 src->dst affine (the warp samples src at M^-1 * dst, like cv2.warpAffine without
// WARP_INVERSE_MAP).  warp == 0 skips the warp (normalise only; M ignored, OH/OW must equal H/W).
MXR_API int mxr_image_warp_normalize(const uint8_t* src, int H, int W, float* dst, int OH, int OW, const double* M,
                                     int warp, int interp, int border, float cval, float scale, float m0, float m1,
                                     float m2, hipStream_t stream) {
  if (H <= 0 || W <= 0 || OH <= 0 || OW <= 0) return -1;
  if (!warp && (OH != H || OW != W)) return -2;
  const Affine inv = warp ? invert_affine(M) : Affine{0, 0, 0, 0, 0, 0};
  Norm nm{scale, m0, m1, m2};
  const long long n = (long long)OH * OW;
  hipLaunchKernelGGL(warp_norm_kernel, dim3(mxr_grid(n, kBlock, 16384)), dim3(kBlock), 0, stream, src, H, W, dst, OH,
                     OW, inv, warp, interp, border, cval, nm);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// dtype: 0 fp32 slot, 1 bf16 slot
MXR_API int mxr_image_resize_into(const float* src, int H, int W, void* dst, int OH, int OW, long long ld, int dtype,
                                  hipStream_t stream) {
  if (H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || ld < 3LL * OW) return -1;
  const long long n = (long long)OH * OW;
  if (dtype == 0)
    hipLaunchKernelGGL(resize_kernel<float>, dim3(mxr_grid(n, kBlock, 16384)), dim3(kBlock), 0, stream, src, H, W,
                       (float*)dst, OH, OW, ld);
  else
    hipLaunchKernelGGL(resize_kernel<bf16_t>, dim3(mxr_grid(n, kBlock, 16384)), dim3(kBlock), 0, stream, src, H, W,
                       (bf16_t*)dst, OH, OW, ld);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
