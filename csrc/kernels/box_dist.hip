// The distribution box head of Generalized Focal Loss (Li et al., NeurIPS 2020, sections 3.2 / 3.3): per box side a
// softmax over K bins whose expectation is the regressed delta, and Distribution Focal Loss on the two bins that
// bracket the target.  --regression-bins K / --regression-range R; ops.boxes.box_integral and
// ops.losses.distribution_focal_loss are the torch expressions (CPU path, fallback, float64 oracle).
//
//   bins      v_i = -R + i * D, D = 2R / (K - 1), i = 0 .. K-1, in the std-0.2 corner-delta units of the head
//   integral  p = softmax(l) with the maximum subtracted, y = sum_i p_i v_i;  dl_i = g p_i (v_i - y)
//   DFL       u = clamp((t - v_0) / D, 0, K - 1 - 0.01), il = floor(u), wr = u - il, wl = 1 - wr
//             loss = -(wl log p_il + wr log p_il+1) from the log-softmax;  dl_i = p_i - wl [i == il] - wr [i == il + 1]
//             summed over the sides of the rows with state 1, / (4 max(1, npos)) * weight
//
// logits: [rows, 4, K] (bf16 or f32, fp32 arithmetic, one rounding per output), deltas: [rows, 4].  Both entry points
// follow the contract of losses.hip: 64-bit element offsets, grids that depend on the shapes alone, no atomics, one
// loss partial per block plus the shared finalize launch, the same bits on every call, no host synchronisation, -1
// before any launch for what they do not serve.
//
// One thread owns one (row, side): a tile is 64 rows (the padded form: as many whole groups as fit in 64 rows), so
// the 256 threads of a block cover it.  About 1 % of the rows are positive; only those read their logits, with
// per-lane loads (the four lanes of a row read its 4K contiguous values).  The bulk of the backward is the zero
// fill of dlogits (437 MB at 16 x 200,700 x 68 bf16): the tile is built in LDS -- zeros, the positive rows'
// gradients on top -- and leaves in 16-B stores; a tile without a positive row stores zeros without touching LDS.
// The all-rows integral (the prediction model) stages its contiguous tile of logits through LDS with 16-B loads.
#include "common.h"

void mxr_loss_finalize_launch(const float* partials, int n, const int* npos, float* out, hipStream_t stream);
MXR_API int mxr_loss_grid();

namespace {

constexpr int kBlock = 256;
constexpr int kTileRows = kBlock / 4;   // one thread per (row, side)
constexpr int kMaxBins = 32;
constexpr int kRedBytes = 64;           // block_sum's scratch in front of the tile: the tile stays 16-B aligned
constexpr int kMaxLds = 64 * 1024;

template <typename T> struct V16;       // 16 bytes of T
template <> struct V16<bf16_t> { typedef uint4 type; static constexpr int N = 8; };
template <> struct V16<float> { typedef float4 type; static constexpr int N = 4; };

// softmax of one side's K logits at src (global memory or LDS): p[] and the log-softmax terms l[] - lse
template <typename T, int KK>
struct Side {
  static constexpr int KM = KK ? KK : kMaxBins;
  float l[KM];      // l_i - max
  float p[KM];
  float lse;        // log sum exp(l_i - max)
  float y;

  __device__ __forceinline__ void load(const T* src, int K, float R, float D) {
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < KM; ++i) {
      l[i] = (KK || i < K) ? Cvt<T>::to_f(src[KK || i < K ? i : 0]) : -INFINITY;
      m = fmaxf(m, l[i]);
    }
    float S = 0.f;
#pragma unroll
    for (int i = 0; i < KM; ++i) {
      l[i] -= m;
      p[i] = (KK || i < K) ? expf(l[i]) : 0.f;
      S += p[i];
    }
    const float inv = 1.0f / S;
    lse = logf(S);
    y = 0.f;
#pragma unroll
    for (int i = 0; i < KM; ++i) {
      p[i] *= inv;
      if (KK || i < K) y += p[i] * bin(i, R, D);
    }
  }
  __device__ __forceinline__ static float bin(int i, float R, float D) { return (float)i * D - R; }
};

// ---------------------------------------------------------------------------------------------------------------
// integral forward.  state == nullptr: every row; otherwise only rows with state 1 read their logits and the
// others get 0.  STAGED (all rows, 16-B aligned logits): the tile's contiguous logits go through LDS.
// ---------------------------------------------------------------------------------------------------------------
template <typename T, int KK, bool STAGED>
__global__ __launch_bounds__(kBlock) void box_integral_kernel(const T* __restrict__ logits,
                                                              const int8_t* __restrict__ state, T* __restrict__ out,
                                                              long long rows, int Krt, float R, float D, bool vec_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef typename V16<T>::type vec_t;
  constexpr int V = V16<T>::N;
  const int K = KK ? KK : Krt;
  const int K4 = 4 * K;
  T* tile = reinterpret_cast<T*>(smem);
  const int lr = threadIdx.x >> 2, s = threadIdx.x & 3;
  const long long ntiles = (rows + kTileRows - 1) / kTileRows;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long row0 = t * kTileRows;
    const int nrows = (int)((rows - row0) < kTileRows ? (rows - row0) : kTileRows);
    const long long row = row0 + lr;
    const bool live = lr < nrows;
    float y = 0.f;
    if (STAGED) {
      const T* src = logits + row0 * K4;         // 64 rows x 4K elements: a multiple of 16 B from an aligned base
      const int n = nrows * K4;                  // a multiple of 4
      const int nv = n / V;
      for (int i = threadIdx.x; i < nv; i += kBlock)
        reinterpret_cast<vec_t*>(tile)[i] = reinterpret_cast<const vec_t*>(src)[i];
      for (int i = nv * V + threadIdx.x; i < n; i += kBlock) tile[i] = src[i];
      __syncthreads();
      if (live) {
        Side<T, KK> sd;
        sd.load(tile + (lr * 4 + s) * K, K, R, D);
        y = sd.y;
      }
    } else if (live && (state == nullptr || state[row] == 1)) {
      Side<T, KK> sd;
      sd.load(logits + (row * 4 + s) * K, K, R, D);
      y = sd.y;
    }
    // the row's four sides sit in four neighbouring lanes: lane s == 0 stores them as one vector
    const float y1 = __shfl_down(y, 1, 64), y2 = __shfl_down(y, 2, 64), y3 = __shfl_down(y, 3, 64);
    if (live) {
      if (!vec_out) {
        out[row * 4 + s] = Cvt<T>::from_f(y);
      } else if (s == 0) {
        if constexpr (sizeof(T) == 2) {
          uint2 o;
          o.x = (uint32_t)f2bf(y) | ((uint32_t)f2bf(y1) << 16);
          o.y = (uint32_t)f2bf(y2) | ((uint32_t)f2bf(y3) << 16);
          reinterpret_cast<uint2*>(out)[row] = o;
        } else {
          reinterpret_cast<float4*>(out)[row] = make_float4(y, y1, y2, y3);
        }
      }
    }
    if (STAGED) __syncthreads();                 // the next tile's loads overwrite the LDS image
  }
}

// ---------------------------------------------------------------------------------------------------------------
// DFL forward + backward of DFL and integral in one launch.  dlogits: groups of grp rows at a pitch of ld elements
// (ld * sizeof(T) a multiple of 16), gpt groups per tile; the plain [rows, 4K] layout is one group of 64 rows per
// tile at a pitch of 64 * 4K.  A group's columns past its rows' 4K values are never written.
// GG: grp at compile time (0: run time), so that the write-out's index split is a multiplication.
// ---------------------------------------------------------------------------------------------------------------
template <typename T, int KK, int GG>
__global__ __launch_bounds__(kBlock) void box_dist_kernel(const T* __restrict__ logits, const T* __restrict__ dreg,
                                                          const float* __restrict__ target,
                                                          const int8_t* __restrict__ state, const int* __restrict__ npos,
                                                          T* __restrict__ dlogits, float* __restrict__ partials,
                                                          long long rows, int Krt, float R, float D, float weight,
                                                          int grp_rt, long long ld, int gpt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef typename V16<T>::type vec_t;
  constexpr int V = V16<T>::N;
  const int K = KK ? KK : Krt;
  const int K4 = 4 * K;
  const int grp = GG ? GG : grp_rt;
  const int W = grp * K4;                        // a group's valid columns
  const int nvc = (W + V - 1) / V;               // 16-B chunks per group, the last one possibly half (bf16: 4 values)
  const int Wl = nvc * V;                        // LDS pitch of a group
  float* red = reinterpret_cast<float*>(smem);
  T* tile = reinterpret_cast<T*>(smem + kRedBytes);
  const int tr = gpt * grp;                      // rows per tile, <= kTileRows
  const int lr = threadIdx.x >> 2, s = threadIdx.x & 3;
  const int lg = lr / grp;                       // this thread's group inside the tile
  const int loff = lg * Wl + (lr - lg * grp) * K4 + s * K;
  const float sc = weight * 0.25f / fmaxf(1.0f, (float)(*npos));
  const long long ntiles = (rows + tr - 1) / tr;
  vec_t zero;
  __builtin_memset(&zero, 0, sizeof(zero));
  for (int i = threadIdx.x; i < gpt * nvc; i += kBlock) reinterpret_cast<vec_t*>(tile)[i] = zero;
  float acc = 0.f;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const long long row0 = t * tr;
    const int nrows = (int)((rows - row0) < tr ? (rows - row0) : tr);
    const long long row = row0 + lr;
    const bool pos = lr < nrows && state[row] == 1;
    const int any = __syncthreads_or(pos);       // also: the zeros (first tile: the initial fill) are in place
    if (pos) {
      Side<T, KK> sd;
      sd.load(logits + (row * 4 + s) * K, K, R, D);
      const float g = Cvt<T>::to_f(dreg[row * 4 + s]);
      float u = (target[row * 4 + s] + R) / D;
      u = fminf(fmaxf(u, 0.f), (float)(K - 1) - 0.01f);
      const float fl = floorf(u);
      const int il = (int)fl;
      const float wr = u - fl, wl = 1.0f - wr;
      float ll = 0.f, lh = 0.f;
#pragma unroll
      for (int i = 0; i < Side<T, KK>::KM; ++i) {
        if (KK || i < K) {
          ll = i == il ? sd.l[i] : ll;
          lh = i == il + 1 ? sd.l[i] : lh;
          const float d = g * sd.p[i] * (Side<T, KK>::bin(i, R, D) - sd.y) +
                          sc * (sd.p[i] - (i == il ? wl : 0.f) - (i == il + 1 ? wr : 0.f));
          tile[loff + i] = Cvt<T>::from_f(d);
        }
      }
      acc -= wl * (ll - sd.lse) + wr * (lh - sd.lse);
    }
    if (any) __syncthreads();
    // write-out: every group's W columns in 16-B stores (bf16 with W % 8 == 4: one 8-B store at the end); a lane that
    // read LDS puts the zeros back, so the image is clean for the next tile
    const int ngrp = (nrows + grp - 1) / grp;
    T* dst0 = dlogits + (row0 / grp) * ld;
    for (int i = threadIdx.x; i < ngrp * nvc; i += kBlock) {
      const int g = i / nvc, c = i - g * nvc;
      const int left = nrows - g * grp;
      const int wg = (left < grp ? left : grp) * K4;     // the plain layout's last tile: fewer rows
      const int e0 = c * V;
      if (e0 >= wg) continue;
      T* dst = dst0 + g * ld + e0;
      T* src = tile + g * Wl + e0;
      if (e0 + V <= wg) {
        vec_t v = zero;
        if (any) {
          v = *reinterpret_cast<vec_t*>(src);
          *reinterpret_cast<vec_t*>(src) = zero;
        }
        *reinterpret_cast<vec_t*>(dst) = v;
      } else {                                   // 4 values of bf16
        uint2 v = make_uint2(0u, 0u);
        if (any) {
          v = *reinterpret_cast<uint2*>(src);
          *reinterpret_cast<uint2*>(src) = make_uint2(0u, 0u);
        }
        *reinterpret_cast<uint2*>(dst) = v;
      }
    }
    // (the next tile's __syncthreads_or orders these LDS reads and zeros before its positive rows write)
  }
  const float bs = block_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = bs * (weight * 0.25f);
}

template <typename T, int KK>
void integral_launch(const void* logits, const int8_t* state, void* out, long long rows, int K, float R, float D,
                     hipStream_t stream) {
  const long long ntiles = (rows + kTileRows - 1) / kTileRows;
  const int grid = (int)(ntiles < 4096 ? ntiles : 4096);
  const bool vec_out = (uintptr_t)out % (4 * sizeof(T)) == 0;
  if (state == nullptr && (uintptr_t)logits % 16 == 0) {
    const size_t lds = (size_t)kTileRows * 4 * K * sizeof(T);
    box_integral_kernel<T, KK, true><<<grid, kBlock, lds, stream>>>((const T*)logits, state, (T*)out, rows, K, R, D,
                                                                    vec_out);
  } else {
    box_integral_kernel<T, KK, false><<<grid, kBlock, 0, stream>>>((const T*)logits, state, (T*)out, rows, K, R, D,
                                                                   vec_out);
  }
}

template <typename T, int KK, int GG>
void dist_launch(const void* logits, const void* dreg, const float* target, const int8_t* state, const int* npos,
                 void* dlogits, float* partials, long long rows, int K, float R, float D, float weight, int grp,
                 long long ld, int gpt, int grid, size_t lds, hipStream_t stream) {
  box_dist_kernel<T, KK, GG><<<grid, kBlock, lds, stream>>>((const T*)logits, (const T*)dreg, target, state, npos,
                                                            (T*)dlogits, partials, rows, K, R, D, weight, grp, ld, gpt);
}

}  // namespace

// logits [rows, 4, K] -> out [rows, 4], both of dtype (0 = f32, 1 = bf16).  state: nullptr for every row, or [rows]
// int8: rows whose state is not 1 get 0 and their logits are not read.  Returns -1 for what it does not serve.
MXR_API int mxr_box_integral_fwd(const void* logits, const int8_t* state, void* out, long long rows, int K, float R,
                                 int dtype, hipStream_t stream) {
  if (K < 2 || K > kMaxBins || (dtype != 0 && dtype != 1) || !(R > 0.f) || rows < 0) return -1;
  if (rows == 0) return 0;
  const float D = (float)(2.0 * (double)R / (double)(K - 1));
  if (dtype == 1) {
    if (K == 17) integral_launch<bf16_t, 17>(logits, state, out, rows, K, R, D, stream);
    else integral_launch<bf16_t, 0>(logits, state, out, rows, K, R, D, stream);
  } else {
    if (K == 17) integral_launch<float, 17>(logits, state, out, rows, K, R, D, stream);
    else integral_launch<float, 0>(logits, state, out, rows, K, R, D, stream);
  }
  return (int)hipGetLastError();
}

// DFL loss (out[0], * weight / (4 max(1, npos))) and dlogits = integral backward of dreg + DFL gradient.
// logits / dlogits / dreg of dtype; target [rows, 4] f32; partials must hold mxr_loss_grid() floats.
// grp / ld: 0 for the plain [rows, 4K] layout, otherwise dlogits is [rows / grp][ld] with ld >= grp * 4K.
MXR_API int mxr_box_dist_fwd_bwd(const void* logits, const void* dreg, const float* target, const int8_t* state,
                                 const int* npos, void* dlogits, float* partials, float* out, long long rows, int K,
                                 float R, float weight, int dtype, int grp, int ld, hipStream_t stream) {
  if (K < 2 || K > kMaxBins || (dtype != 0 && dtype != 1) || !(R > 0.f) || rows <= 0) return -1;
  const size_t esz = dtype == 1 ? 2 : 4;
  if ((uintptr_t)dlogits % 16) return -1;
  int gpt = 1;
  long long pitch;
  if (ld > 0) {
    if (grp <= 0 || grp > kTileRows || (long long)grp * 4 * K > ld || rows % grp || (ld * esz) % 16) return -1;
    gpt = kTileRows / grp;
    pitch = ld;
  } else {
    grp = kTileRows;
    pitch = (long long)kTileRows * 4 * K;
  }
  const int V = 16 / (int)esz;
  const size_t lds = kRedBytes + (size_t)gpt * (((size_t)grp * 4 * K + V - 1) / V * V) * esz;
  if (lds > (size_t)kMaxLds) return -1;
  const long long tr = (long long)gpt * grp;
  const long long ntiles = (rows + tr - 1) / tr;
  const int maxg = mxr_loss_grid();
  const int grid = (int)(ntiles < maxg ? ntiles : maxg);
  const float D = (float)(2.0 * (double)R / (double)(K - 1));
  const bool g9 = ld > 0 && grp == 9;
#define MXR_DIST(T, KK, GG) \
  dist_launch<T, KK, GG>(logits, dreg, target, state, npos, dlogits, partials, rows, K, R, D, weight, grp, pitch, gpt, \
                         grid, lds, stream)
  if (dtype == 1) {
    if (K == 17 && g9) MXR_DIST(bf16_t, 17, 9);
    else if (K == 17) MXR_DIST(bf16_t, 17, 0);
    else MXR_DIST(bf16_t, 0, 0);
  } else {
    if (K == 17 && g9) MXR_DIST(float, 17, 9);
    else if (K == 17) MXR_DIST(float, 17, 0);
    else MXR_DIST(float, 0, 0);
  }
#undef MXR_DIST
  mxr_loss_finalize_launch(partials, grid, npos, out, stream);
  return (int)hipGetLastError();
}
