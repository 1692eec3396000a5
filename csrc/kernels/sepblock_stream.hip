// The K-streamed form of the eval-mode depthwise-separable block of MobileNet, NHWC bf16, ONE kernel (forward only).
// It computes what sepblock.hip computes, from the same operands:
//
//   y = relu6(a2 * (Wpw . bf16(relu6(a1 * dw3x3(x) + b1))) + b2)
//
// x [N, H, W, Ci] bf16; tap-major [9][Ci] fp32 taps; Keras' padding (taps outside the input read zero, no padded copy);
// a = gamma * rsqrt(var + eps), b = beta - mean * a folded here in fp32; Wpw [Co, Ci] bf16; y [N, Ho, Wo, Co] bf16.  Z
// and y are rounded to bf16 once each.  sepblock.hip keeps the whole Z[P][Ci] of a tile in LDS, which at Ci >= 512
// leaves 64 pixels and one workgroup per CU, pulls the whole weight through LDS per 64 pixels and overlaps nothing.
// This kernel never holds Z: it walks Ci in chunks of 32 and keeps two chunks of Z in LDS.
//
// Work split.  A workgroup of 512 threads (8 waves) owns 128 consecutive output pixels of the flattened (n, oy, ox)
// order and a column block of up to 512 output channels: grid = (ceil(N Ho Wo / 128), ceil(Co / 512)).  Tiles are
// linear: nothing is staged per tile shape, a tile may cross row ends and images, and every pixel decodes its own
// (n, oy, ox) once.  For Co > 512 the depthwise stage is computed once per column block.
//
// K loop, one barrier per chunk of 32 input channels.  Z lives in a ring of two slots of 128 pixels x 32 channels with
// a row pitch of 80 bytes (five 16-byte units, odd: the 16 rows of a fragment read fall on distinct bank groups):
// 20 KB.  In iteration c every wave first multiplies chunk c (ring slot c % 2), then produces chunk c + 1 into the other
// slot from taps that were loaded one iteration earlier, then issues the tap loads of chunk c + 2; the barrier follows.
//
// Producer (depthwise).  Per chunk a thread owns one pixel and one 8-channel vector (512 = 128 x 4).  Nine 16-byte tap
// loads straight from global memory / L2; a tap outside the image, and every tap of a pixel past the end, is loaded
// from the pixel's always-valid tap instead (the centre at stride 1, the top left at stride 2) and replaced by zero
// when it is used, so the loads carry no branch and no wait.  72 fp32 multiply-adds against an LDS table [10][Ci]
// filled once per workgroup: the nine taps premultiplied by a1, and b1, which starts the sum (the first norm costs no
// instruction of its own).  Clamp, one rounding, one 16-byte LDS store.
//
// Consumer (pointwise), __builtin_amdgcn_mfma_f32_16x16x32_bf16.  The 8 waves split the column block into 64-channel
// slices and do not split the pixels: a wave holds 128 pixels x 64 channels = 8 x 4 accumulator tiles.  Its A operand
// (the weight, with pwconv.hip's row permutation: A-row i of the tile pair (2 p, 2 p + 1), tile 2 p + h, is channel
// 32 p + 8 (i / 4) + 4 h + i % 4) goes from global memory to registers, four 16-byte loads per lane per chunk, loaded one
// chunk ahead; no weight passes through LDS and each element is read by one wave of the workgroup.  The B operand is
// the Z chunk: 8 fragment reads feed 32 MFMAs.  Waves and tile pairs whose channels lie past Co skip loads and MFMAs;
// rows past Co inside a pair and channel vectors past Ci in the last chunk are zero on both operands by predicate
// (loaded from a clamped address, replaced by zero): nothing is padded in memory.
//
// Epilogue.  Lane (li, g) holds channels 32 p + 8 g .. + 7 of pixel 16 t + li: second affine and clamp in registers, one
// 16-byte store per (t, p).  Pixels past the end and channels past Co are not written.
//
// Deviations from the issue's sketch.  (1) Predicated loads became clamped loads plus a select at the point of use, so
// the K loop has no divergent branch between the loads and the MFMAs.  (2) The loop is peeled, not unrolled: the last
// chunk's MFMAs run after it, and the weight registers are handed over by copies the compiler may rename away.  (3) The
// kernel is instantiated for (stride, FULL), FULL = Co % 512 == 0, where every wave owns two whole tile pairs and the
// channel predicates vanish at compile time.
//
// The whole rule, a function of the shapes alone (no atomics, no workspace, no memset, no host synchronisation;
// capturable; two calls give the same bits):
//   served: bf16, Ci % 8 == 0, 32 <= Ci <= 1024, Co % 8 == 0, 8 <= Co <= 1024, stride 1 or 2 with Keras' geometry
//   (H, W >= stride, <= 2^24), 1 <= N Ho Wo < 2^31 - 128, 16-byte aligned operands;
//   grid = (ceil(N Ho Wo / 128), ceil(Co / 512)), 512 threads; chunks = ceil(Ci / 32);
//   LDS = 40 Ci + 20480 bytes (dynamic): Ci = 32: 21.3 KB   264: 30.3 KB   512: 40.0 KB   1024: 60.0 KB.
//
// Registers / LDS as compiled (VGPRs + AGPRs; scratch 0 bytes in all four; 2 waves per SIMD, i.e. one 8-wave
// workgroup per CU, by registers):
//   sep_block_stream<1,true> 255 + 0   <2,true> 255 + 0   <1,false> 255 + 0   <2,false> 255 + 0
//   LDS: dynamic, as above (nothing static).
// With the eight B fragments of a chunk read at once (32 registers, as sketched) the compiler spilled 44 to 64 bytes
// per lane; they are read in two halves of four, as the issue proposes for that case.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) short ss_bf16x8;
typedef __attribute__((ext_vector_type(4))) float ss_f32x4;

constexpr int kSsThreads = 512;
constexpr int kSsMT = 128;                   // pixels of a workgroup
constexpr int kSsCB = 512;                   // output channels of a column block: 8 waves x 64
constexpr int kSsZRow = 80;                  // bytes of a row of a ring slot: 32 bf16 + 16
constexpr int kSsSlot = kSsMT * kSsZRow;     // bytes of a ring slot
constexpr int kSsMinCi = 32, kSsMaxC = 1024;

struct SsGeom {
  int H, W, Ho, Wo, Ci, Co;
  int pt, pl;                                // rows / columns of padding before the first input pixel
  int M, nch;                                // output pixels N Ho Wo; chunks of 32 input channels
};

struct SsNorm { const float *gamma, *beta, *mean, *var; float eps; };

__device__ __forceinline__ ss_bf16x8 ss_as_frag(const uint4 q) { return __builtin_bit_cast(ss_bf16x8, q); }

__device__ __forceinline__ uint4 ss_zero() { return make_uint4(0u, 0u, 0u, 0u); }

__device__ __forceinline__ uint4 ss_keep(bool keep, const uint4 q) {
  return make_uint4(keep ? q.x : 0u, keep ? q.y : 0u, keep ? q.z : 0u, keep ? q.w : 0u);
}

__device__ __forceinline__ void ss_unpack(const uint4 q, float* f) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ uint4 ss_pack(const float* f) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = (uint32_t)f2bf(f[2 * i]) | ((uint32_t)f2bf(f[2 * i + 1]) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ void ss_load8(float* f, const float* p) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
  f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

__device__ __forceinline__ float ss_relu6(float v) { return fminf(fmaxf(v, 0.f), 6.f); }

// What a thread keeps about its producer item: the pixel's always-valid tap, the taps that lie inside the image.
struct SsItem {
  const bf16_t* xsafe;                       // channel 0 of the always-valid tap of the pixel
  unsigned mask;                             // bit ky * 3 + kx: the tap lies inside the image (0 for a pixel past the end)
  int pp, pv;                                // pixel of the tile, channel vector of the chunk
};

// The nine raw taps of chunk c: branch-free, a tap outside the image reads the always-valid one.
template <int S>
__device__ __forceinline__ void ss_load_taps(uint4 (&xr)[9], const SsItem& it, const SsGeom& g, int c) {
  constexpr int SAFE = S == 1 ? 1 : 0;
  const int kk = min(32 * c + 8 * it.pv, g.Ci - 8);
  const bf16_t* p = it.xsafe + kk;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const long long d = ((long long)(t / 3 - SAFE) * g.W + (t % 3 - SAFE)) * g.Ci;
    xr[t] = *reinterpret_cast<const uint4*>(p + (((it.mask >> t) & 1u) ? d : 0LL));
  }
}

// Chunk c of Z from its raw taps, into a ring slot.
__device__ __forceinline__ void ss_produce(const uint4 (&xr)[9], const SsItem& it, const SsGeom& g, const float* tab,
                                           char* slot, int c) {
  const int k = 32 * c + 8 * it.pv, kk = min(k, g.Ci - 8);
  float acc[8];
  ss_load8(acc, tab + 9 * g.Ci + kk);
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    float f[8], w[8];
    ss_unpack(ss_keep((it.mask >> t) & 1u, xr[t]), f);
    ss_load8(w, tab + t * g.Ci + kk);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = fmaf(f[j], w[j], acc[j]);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = ss_relu6(acc[j]);
  *reinterpret_cast<uint4*>(slot + it.pp * kSsZRow + 16 * it.pv) = ss_keep(k < g.Ci, ss_pack(acc));
}

template <bool FULL>
__device__ __forceinline__ void ss_load_w(uint4 (&wr)[4], const bf16_t* __restrict__ w2, const int (&wrow)[4], int npairs,
                                          const SsGeom& g, int gq, int c) {
  const int kk = min(32 * c + 8 * gq, g.Ci - 8);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    wr[j] = ss_zero();
    if (FULL || (j >> 1) < npairs) wr[j] = *reinterpret_cast<const uint4*>(w2 + wrow[j] + kk);
  }
}

template <bool FULL>
__device__ __forceinline__ void ss_mma(ss_f32x4 (&acc)[8][4], const uint4 (&wr)[4], unsigned wmask, int npairs,
                                       const SsGeom& g, const char* zrow0, int gq, int c) {
  const bool kok = 32 * c + 8 * gq < g.Ci;
  ss_bf16x8 a[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) a[j] = ss_as_frag(ss_keep(kok && (FULL || ((wmask >> j) & 1u)), wr[j]));
  // the B fragments in two halves of four pixel tiles: 16 registers live, not 32
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    uint4 b[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) b[t] = *reinterpret_cast<const uint4*>(zrow0 + 16 * (4 * h + t) * kSsZRow);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (FULL || (j >> 1) < npairs) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
          acc[4 * h + t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[j], ss_as_frag(b[t]), acc[4 * h + t][j], 0, 0, 0);
      }
    }
  }
}

template <int S, bool FULL>
__global__ __launch_bounds__(kSsThreads) void sep_block_stream(const bf16_t* __restrict__ x, const float* __restrict__ w9,
                                                               const SsNorm bn1, const bf16_t* __restrict__ w2,
                                                               const SsNorm bn2, bf16_t* __restrict__ y, const SsGeom g) {
  extern __shared__ uint4 ss_lds[];
  float* tab = reinterpret_cast<float*>(ss_lds);                         // [10][Ci]: taps * a1, b1
  char* ring = reinterpret_cast<char*>(ss_lds) + 40 * g.Ci;              // two slots of Z
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int li = lane & 15, gq = lane >> 4;
  const int m0 = blockIdx.x * kSsMT, cb0 = blockIdx.y * kSsCB;

  // ---------------------------------------------------------------- the thread's producer item
  constexpr int SAFE = S == 1 ? 1 : 0;
  SsItem it;
  it.pp = tid >> 2;
  it.pv = tid & 3;
  {
    const bool pok = m0 + it.pp < g.M;
    const int m = pok ? m0 + it.pp : g.M - 1;
    const int hw = g.Ho * g.Wo;
    const int n = m / hw, r = m - n * hw;
    const int oy = r / g.Wo, ox = r - oy * g.Wo;
    const int iy0 = oy * S - g.pt, ix0 = ox * S - g.pl;
    it.mask = 0u;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int iy = iy0 + t / 3, ix = ix0 + t % 3;
      if (pok && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) it.mask |= 1u << t;
    }
    it.xsafe = x + (((long long)n * g.H + iy0 + SAFE) * g.W + ix0 + SAFE) * g.Ci;
  }

  // ---------------------------------------------------------------- the wave's slice of the column block
  const int cw = cb0 + 64 * wv, left = g.Co - cw;
  const int npairs = FULL ? 2 : left <= 0 ? 0 : left >= 64 ? 2 : (left + 31) >> 5;
  int wrow[4];
  unsigned wmask = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int co = cw + 32 * (j >> 1) + 8 * (li >> 2) + 4 * (j & 1) + (li & 3);
    if (co < g.Co) wmask |= 1u << j;
    wrow[j] = min(co, g.Co - 1) * g.Ci;
  }

  uint4 xr[9], wa[4], wb[4];
  ss_load_taps<S>(xr, it, g, 0);
  ss_load_w<FULL>(wa, w2, wrow, npairs, g, gq, 0);

  for (int i = tid; i < g.Ci; i += kSsThreads) {
    const float a = bn1.gamma[i] * rsqrtf(bn1.var[i] + bn1.eps);
    tab[9 * g.Ci + i] = bn1.beta[i] - bn1.mean[i] * a;
#pragma unroll
    for (int t = 0; t < 9; ++t) tab[t * g.Ci + i] = w9[(long long)t * g.Ci + i] * a;
  }
  __syncthreads();
  ss_produce(xr, it, g, tab, ring, 0);
  if (g.nch > 1) ss_load_taps<S>(xr, it, g, 1);
  __syncthreads();

  ss_f32x4 acc[8][4];
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[t][j] = ss_f32x4{0.f, 0.f, 0.f, 0.f};

  // ---------------------------------------------------------------- K loop
  const int zoff = li * kSsZRow + 16 * gq;
  for (int c = 0; c + 1 < g.nch; ++c) {
    ss_load_w<FULL>(wb, w2, wrow, npairs, g, gq, c + 1);
    ss_mma<FULL>(acc, wa, wmask, npairs, g, ring + (c & 1) * kSsSlot + zoff, gq, c);
    ss_produce(xr, it, g, tab, ring + ((c + 1) & 1) * kSsSlot, c + 1);
    if (c + 2 < g.nch) ss_load_taps<S>(xr, it, g, c + 2);
    __syncthreads();           // chunk c + 1 is written; the reads of chunk c are done
#pragma unroll
    for (int j = 0; j < 4; ++j) wa[j] = wb[j];
  }
  ss_mma<FULL>(acc, wa, wmask, npairs, g, ring + ((g.nch - 1) & 1) * kSsSlot + zoff, gq, g.nch - 1);

  // ---------------------------------------------------------------- epilogue: y = bf16(relu6(a2 * acc + b2))
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int co = cw + 32 * p + 8 * gq;
    if ((FULL || p < npairs) && co < g.Co) {
      float a2[8], b2[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        a2[j] = bn2.gamma[co + j] * rsqrtf(bn2.var[co + j] + bn2.eps);
        b2[j] = bn2.beta[co + j] - bn2.mean[co + j] * a2[j];
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int m = m0 + 16 * t + li;
        const ss_f32x4 lo = acc[t][2 * p], hi = acc[t][2 * p + 1];
        float f[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          f[e] = ss_relu6(fmaf(lo[e], a2[e], b2[e]));
          f[4 + e] = ss_relu6(fmaf(hi[e], a2[4 + e], b2[4 + e]));
        }
        if (m < g.M) *reinterpret_cast<uint4*>(y + (long long)m * g.Co + co) = ss_pack(f);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ host side
inline bool ss_aligned(const void* p) { return p && ((uintptr_t)p & 15) == 0; }

// What the entry point refuses (-1), decided before any launch.
bool ss_served(int N, int H, int W, int Ci, int Co, int stride, int pt, int pl, int Ho, int Wo, int dtype) {
  if (dtype != 1 || (stride != 1 && stride != 2) || N < 1) return false;
  if (Ci < kSsMinCi || Ci > kSsMaxC || Ci % 8 || Co < 8 || Co > kSsMaxC || Co % 8) return false;
  if (H < stride || W < stride || H > (1 << 24) || W > (1 << 24)) return false;
  // Keras' geometry: stride 1 pads one pixel on every side, stride 2 pads bottom and right only, valid window
  if (stride == 1 ? !(pt == 1 && pl == 1 && Ho == H && Wo == W)
                  : !(pt == 0 && pl == 0 && Ho == (H - 2) / 2 + 1 && Wo == (W - 2) / 2 + 1))
    return false;
  const long long M = (long long)N * Ho * Wo;
  return M >= 1 && M < 0x7fffffffLL - kSsMT;
}

template <int S, bool FULL>
int ss_launch(const void* x, const void* w9, const SsNorm& bn1, const void* w2, const SsNorm& bn2, void* y,
              const SsGeom& g, hipStream_t stream) {
  const dim3 grid((unsigned)((g.M + kSsMT - 1) / kSsMT), (unsigned)((g.Co + kSsCB - 1) / kSsCB));
  const size_t lds = (size_t)40 * g.Ci + 2 * kSsSlot;      // at most 60 KB: below the 64 KB that need no attribute
  sep_block_stream<S, FULL><<<grid, kSsThreads, lds, stream>>>((const bf16_t*)x, (const float*)w9, bn1,
                                                               (const bf16_t*)w2, bn2, (bf16_t*)y, g);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace

// The operands and the argument list of mxr_sepblock_fwd (sepblock.hip).  -1: not served, before memory is touched.
MXR_API int mxr_sepblock_stream_fwd(const void* x, const void* w9, const void* gamma1, const void* beta1,
                                    const void* mean1, const void* var1, float eps1, const void* w2, const void* gamma2,
                                    const void* beta2, const void* mean2, const void* var2, float eps2, void* y, int N,
                                    int H, int W, int Ci, int Co, int stride, int pad_top, int pad_left, int Ho, int Wo,
                                    int dtype, hipStream_t stream) {
  if (!ss_served(N, H, W, Ci, Co, stride, pad_top, pad_left, Ho, Wo, dtype)) return -1;
  const void* ptrs[] = {x, w9, gamma1, beta1, mean1, var1, w2, gamma2, beta2, mean2, var2, y};
  for (const void* p : ptrs)
    if (!ss_aligned(p)) return -1;
  SsGeom g;
  g.H = H; g.W = W; g.Ho = Ho; g.Wo = Wo; g.Ci = Ci; g.Co = Co; g.pt = pad_top; g.pl = pad_left;
  g.M = N * Ho * Wo;
  g.nch = (Ci + 31) / 32;
  const SsNorm bn1 = {(const float*)gamma1, (const float*)beta1, (const float*)mean1, (const float*)var1, eps1};
  const SsNorm bn2 = {(const float*)gamma2, (const float*)beta2, (const float*)mean2, (const float*)var2, eps2};
  if (Co % kSsCB == 0)
    return stride == 1 ? ss_launch<1, true>(x, w9, bn1, w2, bn2, y, g, stream)
                       : ss_launch<2, true>(x, w9, bn1, w2, bn2, y, g, stream);
  return stride == 1 ? ss_launch<1, false>(x, w9, bn1, w2, bn2, y, g, stream)
                     : ss_launch<2, false>(x, w9, bn1, w2, bn2, y, g, stream);
}
