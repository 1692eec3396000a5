// One depthwise-separable block of MobileNet in eval mode, NHWC bf16, as ONE kernel (forward only):
//
//   y = relu6(a2 * (Wpw . bf16(relu6(a1 * dw3x3(x) + b1))) + b2)
//
// x [N, H, W, Ci] bf16; dw3x3 with the tap-major [9][Ci] fp32 table and Keras' padding (taps outside the input read
// zero, no padded copy); a, b the per-channel affine of a batch-norm's running statistics, folded here in fp32 when the
// vectors are loaded (a = gamma * rsqrt(var + eps), b = beta - mean * a: no prepare launch); Wpw [Co, Ci] bf16;
// y [N, Ho, Wo, Co] bf16.  The per-layer chain (dwconv.hip, batch_norm.hip, pwconv.hip, batch_norm.hip) writes and reads
// three activation tensors between x and y that nobody else reads in eval mode; this kernel reads x once (plus the
// halo of its tile, through L1 / L2) and writes y once.
//
// Work split.  A workgroup of 4 waves owns a tile of P output pixels of one image, 8 rows x TW columns (P = 128: 8 x 16,
// P = 64: 8 x 8; grid = (tiles of an image, N), so a tile never spans two images), and produces ALL Co channels of it.
// Pixels past the image and channels past Co are neither read nor written.
//
// Stage 1, depthwise, no matrix instruction (as dwconv.hip: 9 multiply-adds per element).  A work item is (channel
// vector of 8 channels, output column, run of R output rows); items are dealt to the 256 threads with the channel vector
// fastest, so a wave's 16-byte loads are contiguous runs along C.  A thread walks its R rows with a three-row register
// window, so an output costs 3 (stride 1) or 6 (stride 2) loads, not 9; R is the largest of 8, 4, 2, 1 that still gives
// every thread an item (few channels: short runs, more threads).  fp32 accumulation, then the first affine and the
// clamp in fp32, ONE rounding to bf16, into the LDS image Z[P][Ci].  The fp32 depthwise result never exists in memory.
//   The input halo is NOT staged in LDS; the taps are read straight from global memory / L2 by predicate.  Reason: LDS
//   is what limits this kernel (Z alone is 66 to 129 KB), a halo of the whole channel depth cannot stand next to it
//   (P = 128, Ci = 256, stride 2: 17 x 33 pixels x 512 bytes = 287 KB), and a halo staged in channel chunks would put
//   two barriers around every chunk.  What the pointwise stage needs from the layout -- conflict-free 16-byte k-vector
//   reads of 16 adjacent pixel rows -- is given by Z's own row pitch alone: 2 Ci + 16 bytes when Ci % 16 == 0, 2 Ci + 32
//   otherwise, i.e. an odd number of 16-byte units, so the 16 rows of a read fall on distinct bank groups.
//
// Stage 2, pointwise, on __builtin_amdgcn_mfma_f32_16x16x32_bf16.  Z is the B operand (columns = pixels), read from LDS
// in 16-byte k-vectors; the weight is the A operand with pwconv.hip's row permutation (A-row i of the tile pair
// (2 p, 2 p + 1) is output channel 32 p + 8 (i / 4) + 4 h + i % 4), so lane (li, g) ends up with channels 32 p + 8 g ..
// + 7 of ONE pixel: the second affine and clamp run in registers and the result leaves in one 16-byte store.  Co is
// walked in blocks of 128 channels against the resident Z; each block's weight passes through LDS in stages of kc k
// (kc = min(round32(Ci), 128), or 64 where Z leaves no room for 128: Ci > 1000), resident when one stage covers Ci
// and one block covers Co.  The 4 waves tile a block 2 x 2: a wave owns P / 2 pixels x 64 channels (P / 32 x 4
// accumulators; 4 + P / 32 LDS reads per P / 8 MFMAs of a k-step).  Waves and tile pairs whose channels lie past Co
// skip their MFMAs.  Ci % 32 != 0: the vectors past Ci are zero on both operands by predicate; nothing is padded in
// memory.
//
// Deviation from the issue's sketch: the weight stage is 64 k instead of 128 for Ci > 1000, because
// 64 * (2 * 1024 + 16) + 128 * (2 * 128 + 16) bytes = 163 KB does not fit the CU's 160 KB.
//
// The whole rule, a function of the shapes alone (grid and order too: no atomics, no host synchronisation, capturable;
// two calls give the same bits):
//   P = 128 if Ci <= 256 else 64;  TW = P / 8;  grid = (ceil(Ho / 8) * ceil(Wo / TW), N), 256 threads;
//   Z pitch = 2 Ci + (16 if Ci % 16 == 0 else 32);  kc as above;  LDS = P * pitch + 128 * (2 kc + 16):
//     Ci = 32: 20.0 KB   64: 36.0 KB   128: 68.0 KB   256: 100.0 KB   512: 99.0 KB   1024: 147.0 KB
//   (two workgroups per CU up to Ci = 128, one above).
//
// Registers / LDS as compiled (VGPRs + AGPRs, no scratch in any of them; 2 waves per SIMD by registers):
//   sep_block<1,128> 148 + 64   sep_block<2,128> 147 + 64   sep_block<1,64> 148 + 32   sep_block<2,64> 147 + 32
//   LDS: dynamic, as above (nothing static).
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) short sb_bf16x8;
typedef __attribute__((ext_vector_type(4))) float sb_f32x4;

constexpr int kSbThreads = 256;
constexpr int kSbTH = 8;               // rows of a tile
constexpr int kSbBN = 128;             // output channels of one block of the walk over Co
constexpr int kSbMaxC = 1024;          // channels per side the entry point takes
constexpr int kSbLds = 160 * 1024;     // LDS of a CU

struct SbGeom {
  int H, W, Ho, Wo, Ci, Co, V;         // V: channel vectors of the input
  int pt, pl;                          // rows / columns of padding before the first input pixel
  int tiles_x;
  int R, nitems;                       // depthwise stage: rows per item, items per tile
  int zrow;                            // bytes of a row of Z
  int kc, nstages, wrow;               // weight stage: k per stage, stages, bytes of a row
};

struct SbNorm { const float *gamma, *beta, *mean, *var; float eps; };

__device__ __forceinline__ sb_bf16x8 sb_as_frag(const uint4 q) { return __builtin_bit_cast(sb_bf16x8, q); }

__device__ __forceinline__ void sb_unpack(const uint4 q, float* f) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ uint4 sb_pack(const float* f) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = (uint32_t)f2bf(f[2 * i]) | ((uint32_t)f2bf(f[2 * i + 1]) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ void sb_load8(float* f, const float* __restrict__ p) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
  f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

// The affine of a batch-norm in eval mode for channels c .. c + 7.
__device__ __forceinline__ void sb_fold(float (&a)[8], float (&b)[8], const SbNorm& bn, int c) {
  float ga[8], be[8], me[8], va[8];
  sb_load8(ga, bn.gamma + c);
  sb_load8(be, bn.beta + c);
  sb_load8(me, bn.mean + c);
  sb_load8(va, bn.var + c);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a[j] = ga[j] * rsqrtf(va[j] + bn.eps);
    b[j] = be[j] - me[j] * a[j];
  }
}

__device__ __forceinline__ float sb_relu6(float v) { return fminf(fmaxf(v, 0.f), 6.f); }

// One row of a 3 x 3 window: input pixels (iy, ix0 .. ix0 + 2) of channel vector cv; zero outside the image.
__device__ __forceinline__ void sb_row(uint4 (&row)[3], const bf16_t* __restrict__ xn, const SbGeom& g, bool ok, int iy,
                                       int ix0, int cv) {
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) {
    const int ix = ix0 + kx;
    row[kx] = make_uint4(0u, 0u, 0u, 0u);
    if (ok && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W)
      row[kx] = *reinterpret_cast<const uint4*>(xn + ((long long)iy * g.W + ix) * g.Ci + cv * 8);
  }
}

template <int S, int P>
__global__ __launch_bounds__(kSbThreads) void sep_block(const bf16_t* __restrict__ x, const float* __restrict__ w9,
                                                        const SbNorm bn1, const bf16_t* __restrict__ w2,
                                                        const SbNorm bn2, bf16_t* __restrict__ y, const SbGeom g) {
  extern __shared__ uint4 sb_lds[];
  constexpr int TW = P / kSbTH, TP = P / 32;
  char* zl = reinterpret_cast<char*>(sb_lds);
  char* wl = zl + P * g.zrow;
  const int tyi = blockIdx.x / g.tiles_x, txi = blockIdx.x - tyi * g.tiles_x;
  const int oy0 = tyi * kSbTH, ox0 = txi * TW, n = blockIdx.y;

  // ------------------------------------------------------------------ stage 1: Z = bf16(relu6(a1 * dw3x3(x) + b1))
  const bf16_t* xn = x + (long long)n * g.H * g.W * g.Ci;
  for (int it = threadIdx.x; it < g.nitems; it += kSbThreads) {
    const int cv = it % g.V, rest = it / g.V;
    const int tx = rest % TW, r0 = (rest / TW) * g.R;
    float w[9][8], a1[8], b1[8];
#pragma unroll
    for (int t = 0; t < 9; ++t) sb_load8(w[t], w9 + (long long)t * g.Ci + cv * 8);
    sb_fold(a1, b1, bn1, cv * 8);
    const int ox = ox0 + tx, ix0 = ox * S - g.pl;
    const bool cok = ox < g.Wo;
    uint4 win[3][3];
    {
      const int oy = oy0 + r0;
#pragma unroll
      for (int k = 0; k < 3 - S; ++k) sb_row(win[k], xn, g, cok && oy < g.Ho, oy * S - g.pt + k, ix0, cv);
    }
    for (int r = 0; r < g.R; ++r) {
      const int oy = oy0 + r0 + r;
      const bool ok = cok && oy < g.Ho;
#pragma unroll
      for (int k = 3 - S; k < 3; ++k) sb_row(win[k], xn, g, ok, oy * S - g.pt + k, ix0, cv);
      float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          float f[8];
          sb_unpack(win[k][kx], f);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] = fmaf(f[j], w[k * 3 + kx][j], acc[j]);
        }
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = sb_relu6(fmaf(acc[j], a1[j], b1[j]));
      // pixels past the image: zeros (they are columns of the product that nobody stores)
      *reinterpret_cast<uint4*>(zl + ((r0 + r) * TW + tx) * g.zrow + 16 * cv) = ok ? sb_pack(acc) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int k = 0; k + S < 3; ++k)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) win[k][kx] = win[k + S][kx];
    }
  }

  // ------------------------------------------------------------------ stage 2: y = bf16(relu6(a2 * (W . Z) + b2))
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int li = lane & 15, gq = lane >> 4;
  const int wp = wv & 1, wc = wv >> 1;             // the wave's half of the pixels and of the block's channels
  const int vpr = g.kc >> 3;
  const char* zrow0 = zl + (wp * (P / 2) + li) * g.zrow;

  for (int n0 = 0; n0 < g.Co; n0 += kSbBN) {
    // tile pairs (32 channels each) of this wave that hold a channel below Co: 0, 1 or 2
    const int left = g.Co - n0 - 64 * wc;
    const int npairs = left <= 0 ? 0 : left >= 64 ? 2 : (left + 31) >> 5;
    sb_f32x4 acc[TP][4];
#pragma unroll
    for (int t = 0; t < TP; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t][j] = sb_f32x4{0.f, 0.f, 0.f, 0.f};

    for (int s = 0; s < g.nstages; ++s) {
      const int k0 = s * g.kc;
      __syncthreads();                         // Z is written; the previous stage's reads are done
      for (int i = threadIdx.x; i < kSbBN * vpr; i += kSbThreads) {
        const int r = i / vpr, v = i - r * vpr;
        // LDS row r = 16 j + a is row a of MFMA tile j: output channel 32 (j / 2) + 8 (a / 4) + 4 (j % 2) + a % 4
        const int j = r >> 4, a = r & 15;
        const int co = n0 + 32 * (j >> 1) + 8 * (a >> 2) + 4 * (j & 1) + (a & 3);
        const int k = k0 + 8 * v;
        uint4 q = make_uint4(0u, 0u, 0u, 0u);
        if (co < g.Co && k < g.Ci) q = *reinterpret_cast<const uint4*>(w2 + (long long)co * g.Ci + k);
        *reinterpret_cast<uint4*>(wl + r * g.wrow + 16 * v) = q;
      }
      __syncthreads();
      const int ksteps = min(g.kc, (g.Ci - k0 + 31) & ~31) >> 5;
      for (int ks = 0; ks < ksteps; ++ks) {
        const int k = k0 + 32 * ks + 8 * gq;
        uint4 b[TP];
#pragma unroll
        for (int t = 0; t < TP; ++t) {
          b[t] = make_uint4(0u, 0u, 0u, 0u);
          if (k < g.Ci) b[t] = *reinterpret_cast<const uint4*>(zrow0 + 16 * t * g.zrow + 2 * k);
        }
        const char* arow = wl + (64 * wc + li) * g.wrow + (32 * ks + 8 * gq) * 2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if ((j >> 1) < npairs) {
            const sb_bf16x8 a = sb_as_frag(*reinterpret_cast<const uint4*>(arow + 16 * j * g.wrow));
#pragma unroll
            for (int t = 0; t < TP; ++t)
              acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, sb_as_frag(b[t]), acc[t][j], 0, 0, 0);
          }
        }
      }
    }

    // lane (li, gq): pixel wp * P / 2 + 16 t + li of the tile, channels n0 + 64 wc + 32 p + 8 gq .. + 7 from the
    // tile pair (2 p, 2 p + 1)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int co = n0 + 64 * wc + 32 * p + 8 * gq;
      if (p < npairs && co < g.Co) {
        float a2[8], b2[8];
        sb_fold(a2, b2, bn2, co);
#pragma unroll
        for (int t = 0; t < TP; ++t) {
          const int q = wp * (P / 2) + 16 * t + li;
          const int oy = oy0 + q / TW, ox = ox0 + q % TW;
          const sb_f32x4 lo = acc[t][2 * p], hi = acc[t][2 * p + 1];
          float f[8];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            f[e] = sb_relu6(fmaf(lo[e], a2[e], b2[e]));
            f[4 + e] = sb_relu6(fmaf(hi[e], a2[4 + e], b2[4 + e]));
          }
          if (oy < g.Ho && ox < g.Wo)
            *reinterpret_cast<uint4*>(y + (((long long)n * g.Ho + oy) * g.Wo + ox) * g.Co + co) = sb_pack(f);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ host side
inline bool sb_aligned(const void* p) { return p && ((uintptr_t)p & 15) == 0; }

// What the entry point refuses (-1), decided before any launch.
bool sb_served(int N, int H, int W, int Ci, int Co, int stride, int pt, int pl, int Ho, int Wo, int dtype) {
  if (dtype != 1 || (stride != 1 && stride != 2) || N < 1 || N > 65535) return false;
  if (Ci < 8 || Ci > kSbMaxC || Ci % 8 || Co < 8 || Co > kSbMaxC || Co % 8) return false;
  if (H < stride || W < stride || H > (1 << 24) || W > (1 << 24)) return false;
  // Keras' geometry: stride 1 pads one pixel on every side, stride 2 pads bottom and right only, valid window
  if (stride == 1) return pt == 1 && pl == 1 && Ho == H && Wo == W;
  return pt == 0 && pl == 0 && Ho == (H - 2) / 2 + 1 && Wo == (W - 2) / 2 + 1;
}

inline int sb_pixels(int Ci) { return Ci <= 256 ? 128 : 64; }

// Tile, row pitches, weight stage and LDS bytes for Ci input channels.
size_t sb_plan(SbGeom& g, int Ci) {
  const int P = sb_pixels(Ci);
  g.Ci = Ci;
  g.V = Ci / 8;
  g.zrow = 2 * Ci + (Ci % 16 ? 32 : 16);
  const int k32 = (Ci + 31) & ~31;
  g.kc = k32 < 128 ? k32 : 128;
  if ((size_t)P * g.zrow + (size_t)kSbBN * (2 * g.kc + 16) > (size_t)kSbLds) g.kc = 64;
  g.nstages = (Ci + g.kc - 1) / g.kc;
  g.wrow = 2 * g.kc + 16;
  const int tw = P / kSbTH;
  g.R = kSbTH;
  while (g.R > 1 && g.V * tw * (kSbTH / g.R) < kSbThreads) g.R >>= 1;
  g.nitems = g.V * tw * (kSbTH / g.R);
  return (size_t)P * g.zrow + (size_t)kSbBN * g.wrow;
}

template <int S, int P>
int sb_launch(const void* x, const void* w9, const SbNorm& bn1, const void* w2, const SbNorm& bn2, void* y, int N,
              SbGeom& g, size_t lds, hipStream_t stream) {
  g.tiles_x = (g.Wo + P / kSbTH - 1) / (P / kSbTH);
  const long long tiles = (long long)g.tiles_x * ((g.Ho + kSbTH - 1) / kSbTH);
  if (tiles > 0x7fffffffLL) return -1;
  auto kern = sep_block<S, P>;
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kSbLds) != hipSuccess)
      return 2;
    attr_set = true;
  }
  kern<<<dim3((unsigned)tiles, N), kSbThreads, lds, stream>>>((const bf16_t*)x, (const float*)w9, bn1,
                                                             (const bf16_t*)w2, bn2, (bf16_t*)y, g);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace

// out[0 .. 4] = pixels of a workgroup's tile, its columns, k of a weight stage, rows of a depthwise item, LDS bytes,
// for Ci input channels.  -1: not served.
MXR_API int mxr_sepblock_geometry(int Ci, int* out) {
  if (Ci < 8 || Ci > kSbMaxC || Ci % 8 || !out) return -1;
  SbGeom g;
  const size_t lds = sb_plan(g, Ci);
  out[0] = sb_pixels(Ci);
  out[1] = out[0] / kSbTH;
  out[2] = g.kc;
  out[3] = g.R;
  out[4] = (int)lds;
  return 0;
}

// x: bf16 [N, H, W, Ci]; w9: f32 [9][Ci]; bn1: gamma, beta, running mean, running variance, f32 [Ci] each; w2: bf16
// [Co, Ci]; bn2: the same four, f32 [Co]; y: bf16 [N, Ho, Wo, Co], every element written once; dtype 1 = bf16.
// -1: not served.
MXR_API int mxr_sepblock_fwd(const void* x, const void* w9, const void* gamma1, const void* beta1, const void* mean1,
                             const void* var1, float eps1, const void* w2, const void* gamma2, const void* beta2,
                             const void* mean2, const void* var2, float eps2, void* y, int N, int H, int W, int Ci,
                             int Co, int stride, int pad_top, int pad_left, int Ho, int Wo, int dtype,
                             hipStream_t stream) {
  if (!sb_served(N, H, W, Ci, Co, stride, pad_top, pad_left, Ho, Wo, dtype)) return -1;
  const void* ptrs[] = {x, w9, gamma1, beta1, mean1, var1, w2, gamma2, beta2, mean2, var2, y};
  for (const void* p : ptrs)
    if (!sb_aligned(p)) return -1;
  SbGeom g;
  const size_t lds = sb_plan(g, Ci);
  if (lds > (size_t)kSbLds) return -1;
  g.H = H; g.W = W; g.Ho = Ho; g.Wo = Wo; g.Co = Co; g.pt = pad_top; g.pl = pad_left;
  const SbNorm bn1 = {(const float*)gamma1, (const float*)beta1, (const float*)mean1, (const float*)var1, eps1};
  const SbNorm bn2 = {(const float*)gamma2, (const float*)beta2, (const float*)mean2, (const float*)var2, eps2};
  if (sb_pixels(Ci) == 128)
    return stride == 1 ? sb_launch<1, 128>(x, w9, bn1, w2, bn2, y, N, g, lds, stream)
                       : sb_launch<2, 128>(x, w9, bn1, w2, bn2, y, N, g, lds, stream);
  return stride == 1 ? sb_launch<1, 64>(x, w9, bn1, w2, bn2, y, N, g, lds, stream)
                     : sb_launch<2, 64>(x, w9, bn1, w2, bn2, y, N, g, lds, stream);
}
