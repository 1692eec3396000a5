// BatchNorm + activation (none / ReLU / ReLU6) on NHWC bf16 viewed as [n, C], n = N * H * W: MobileNet's 27 norms.
//
//   pre = gamma * (x - mean) * rstd + beta,   y = bf16(clamp(pre, lo, hi)),   gradient where lo < pre < hi
//   training:  mean / var = the channel's biased batch statistics over the n rows, rstd = 1 / sqrt(var + eps),
//              running = (1 - m) * running + m * batch (running_var takes var * n / (n - 1)), updated in place
//   inference: mean = running_mean, rstd = 1 / sqrt(running_var + eps), nothing updated
//
// Work split.  A lane owns one 16-byte vector column (8 channels).  A workgroup of 256 lanes is 2^vl vector columns
// by 256 >> vl row lanes, vl = min(ceil(log2(C / 8)), 5): all 256 lanes are row lanes at C = 8; at C = 1024 a
// workgroup is 32 columns by 8 row lanes and four workgroups (grid.y) share the channels.  A lane holds kBnK = 8 rows,
// interleaved with the other row lanes (a wave reads whole contiguous row segments), so a chunk is (256 >> vl) * 8
// rows -- 2048 at C = 8, 64 from C = 256 on -- and the grid is (chunks, ceil(C / 8 / 2^vl)), a function of (n, C)
// alone: 2100 workgroups at 4.3 M x 8 down to 263 x 4 at 16,800 x 1024, every form above the 256 CUs.
//
// Statistics without cancellation.  A lane's 8 rows stay in registers (8 uint4 = 32 VGPRs): the lane takes their mean,
// then M2 = sum (x - mean)^2 about that mean from the same registers -- the two-pass form, x read from HBM once, no
// E[x^2] - mean^2 anywhere.  (count, mean, M2) triples are then combined with Chan's formula only: across the row
// lanes of the workgroup by a fixed tree through LDS, across the chunks by the finalize launch.  The finalize gives a
// channel one workgroup: lane t combines a contiguous run of ceil(chunks / 256) chunks in chunk order (the partials
// are channel-major, so a run is contiguous memory), a fixed tree combines the lanes -- 33 steps per lane at the
// largest layer instead of 8400 -- and lane 0 writes mean, rstd and the running statistics.  The finalize carries its
// counts as integers, so n up to 2^31 - 1 is counted exactly.
//
// No atomics; every order is fixed by indices, so two calls give the same bits; no allocation, no synchronisation, no
// memset: the entry points can be captured.  The clamp mask is not stored: forward and backward recompute pre with
// bn_pre(), compiled without FMA contraction, and agree on it bit for bit.
//
// LDS: 17 KB (stats tree and backward sums: 17 floats a lane, odd against bank conflicts), 3 KB (finalize).  VGPRs as compiled for gfx950:
// stats 88, forward apply 84, backward partial 118, backward apply 141 (3 waves a SIMD, 16 loads of 16 bytes in flight
// a lane), finalizes 24 or fewer; no scratch.
// HBM passes: forward reads x twice and writes y once (inference: one read, one write); backward reads dy and x
// twice and writes dx once.  No matrix instruction fits: there is no contraction, only per-channel reductions.
#include "common.h"

namespace {

constexpr int kBnThreads = 256;
constexpr int kBnK = 8;            // rows a lane keeps in registers
constexpr int kBnMaxVl = 5;        // at most 32 vector columns a workgroup
constexpr int kBnTriple = 17;      // count, mean[8], M2[8]
constexpr int kBnSums = 17;        // sum g [8], sum g * xhat [8], one float of padding: 128-bit reads off the same banks

// A lane's place in its workgroup: vector column v (8 channels), row lane rl of rb.
struct BnLane { int v, rl, rb, vpad; bool on; };

__device__ __forceinline__ BnLane bn_lane(int C, int vl) {
  BnLane a;
  a.vpad = 1 << vl;
  a.v = blockIdx.y * a.vpad + (threadIdx.x & (a.vpad - 1));
  a.rl = threadIdx.x >> vl;
  a.rb = kBnThreads >> vl;
  a.on = a.v < (C >> 3);
  return a;
}

// The pre-activation, every operation rounded on its own: forward and backward agree on its bits.
__device__ __forceinline__ float bn_pre(float x, float mean, float rstd, float gamma, float beta, float& xhat) {
#pragma clang fp contract(off)
  const float d = x - mean;
  xhat = d * rstd;
  const float t = xhat * gamma;
  return t + beta;
}

__device__ __forceinline__ void bn_unpack(const uint4 q, float* f) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ uint4 bn_pack(const float* f) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = (uint32_t)f2bf(f[2 * i]) | ((uint32_t)f2bf(f[2 * i + 1]) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// the lane's rows of chunk blockIdx.x: row i is r0 + i * rb + rl; the rows inside n are a prefix, its length returned
__device__ __forceinline__ int bn_load(const bf16_t* __restrict__ p, const BnLane& a, long long n, int C, uint4* q) {
  const long long r0 = (long long)blockIdx.x * (a.rb * kBnK) + a.rl;
  int k = 0;
#pragma unroll
  for (int i = 0; i < kBnK; ++i) {
    const long long r = r0 + (long long)i * a.rb;
    q[i] = make_uint4(0u, 0u, 0u, 0u);
    if (r < n) {
      q[i] = *reinterpret_cast<const uint4*>(p + r * C + a.v * 8);
      ++k;
    }
  }
  return k;
}

__device__ __forceinline__ long long bn_elem(const BnLane& a, int C, int i) {
  return ((long long)blockIdx.x * (a.rb * kBnK) + a.rl + (long long)i * a.rb) * C + a.v * 8;
}

// Chan: (na, ma, Ma) takes in (nb, mb, Mb); an empty side changes nothing
__device__ __forceinline__ void bn_chan(float& na, float& ma, float& Ma, float nb, float mb, float Mb) {
  if (nb == 0.f) return;
  const float tot = na + nb, wb = nb / tot, d = mb - ma;
  ma += d * wb;
  Ma += Mb + d * d * (na * wb);
  na = tot;
}

// the same with exact integer counts (the finalize: n can pass 2^24); below 2^24 the bits are those of the above
__device__ __forceinline__ void bn_chan(int& na, float& ma, float& Ma, int nb, float mb, float Mb) {
  if (nb == 0) return;
  const float wb = (float)nb / (float)(na + nb), d = mb - ma;
  ma += d * wb;
  Ma += Mb + d * d * ((float)na * wb);
  na += nb;
}

struct BnParams { float mu[8], rs[8], ga[8], be[8]; };

__device__ __forceinline__ BnParams bn_params(const float* __restrict__ mean, const float* __restrict__ rstd,
                                              const float* __restrict__ gamma, const float* __restrict__ beta, int v) {
  BnParams p;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    p.mu[j] = mean[v * 8 + j];
    p.rs[j] = rstd[v * 8 + j];
    p.ga[j] = gamma[v * 8 + j];
    p.be[j] = beta[v * 8 + j];
  }
  return p;
}

// ------------------------------------------------------------------------------------------ statistics
// part: [C][chunks][2] = the chunk's mean and M2 of the channel (its count follows from the chunk index)
__global__ __launch_bounds__(kBnThreads) void bn_stats_partial(const bf16_t* __restrict__ x, float* __restrict__ part,
                                                               long long n, int C, int vl, long long chunks) {
  __shared__ float red[kBnThreads * kBnTriple];
  const BnLane a = bn_lane(C, vl);
  float cnt = 0.f, m[8], M2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { m[j] = 0.f; M2[j] = 0.f; }
  if (a.on) {
    uint4 q[kBnK];
    const int k = bn_load(x, a, n, C, q);
    if (k > 0) {
      cnt = (float)k;
#pragma unroll
      for (int i = 0; i < kBnK; ++i) {          // rows past n are zeros
        float f[8];
        bn_unpack(q[i], f);
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] += f[j];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) m[j] /= cnt;
#pragma unroll
      for (int i = 0; i < kBnK; ++i) {
        float f[8];
        bn_unpack(q[i], f);
        if (i < k) {
#pragma unroll
          for (int j = 0; j < 8; ++j) { const float d = f[j] - m[j]; M2[j] += d * d; }
        }
      }
    }
  }
  float* own = red + threadIdx.x * kBnTriple;
  own[0] = cnt;
#pragma unroll
  for (int j = 0; j < 8; ++j) { own[1 + j] = m[j]; own[9 + j] = M2[j]; }
  for (int s = a.rb >> 1; s > 0; s >>= 1) {     // row lane rl takes in rl + s: a fixed tree
    __syncthreads();
    if (a.rl < s) {
      const float* o = red + (threadIdx.x + s * a.vpad) * kBnTriple;
      float tot = cnt;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        tot = cnt;                              // the 8 channels share the counts
        bn_chan(tot, m[j], M2[j], o[0], o[1 + j], o[9 + j]);
      }
      cnt = tot;
      own[0] = cnt;
#pragma unroll
      for (int j = 0; j < 8; ++j) { own[1 + j] = m[j]; own[9 + j] = M2[j]; }
    }
  }
  if (a.rl == 0 && a.on) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float* o = part + ((long long)(a.v * 8 + j) * chunks + blockIdx.x) * 2;
      o[0] = m[j];
      o[1] = M2[j];
    }
  }
}

// one workgroup a channel: lane t combines its run of chunks in chunk order, a fixed tree combines the lanes
__global__ __launch_bounds__(kBnThreads) void bn_stats_finalize(const float* __restrict__ part, float* __restrict__ mean,
                                                                float* __restrict__ rstd, float* __restrict__ rmean,
                                                                float* __restrict__ rvar, long long n, int rows,
                                                                long long chunks, float eps, float momentum) {
  __shared__ float red[kBnThreads * 2];
  __shared__ int cnts[kBnThreads];              // counts are integers: fp32 would lose rows above 2^24
  const int c = blockIdx.x;
  const long long per = (chunks + kBnThreads - 1) / kBnThreads;
  const long long k0 = threadIdx.x * per, k1 = min(k0 + per, chunks);
  const float* q = part + (long long)c * chunks * 2;
  int cnt = 0;
  float m = 0.f, M2 = 0.f;
  for (long long k = k0; k < k1; ++k) {
    const long long left = n - k * rows;
    bn_chan(cnt, m, M2, (int)(left < rows ? left : rows), q[2 * k], q[2 * k + 1]);
  }
  float* own = red + threadIdx.x * 2;
  cnts[threadIdx.x] = cnt; own[0] = m; own[1] = M2;
  for (int s = kBnThreads >> 1; s > 0; s >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < s) {
      bn_chan(cnt, m, M2, cnts[threadIdx.x + s], own[s * 2], own[s * 2 + 1]);
      cnts[threadIdx.x] = cnt; own[0] = m; own[1] = M2;
    }
  }
  if (threadIdx.x == 0) {
    const float var = fmaxf(M2 / (float)cnt, 0.f);
    mean[c] = m;
    rstd[c] = 1.0f / sqrtf(var + eps);
    rmean[c] = (1.0f - momentum) * rmean[c] + momentum * m;
    rvar[c] = (1.0f - momentum) * rvar[c] + momentum * (var * ((float)cnt / (float)(cnt - 1)));
  }
}

// inference: the frozen statistics in the form the apply kernels read
__global__ void bn_stats_frozen(const float* __restrict__ rmean, const float* __restrict__ rvar, float* __restrict__ mean,
                                float* __restrict__ rstd, int C, float eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  mean[c] = rmean[c];
  rstd[c] = 1.0f / sqrtf(rvar[c] + eps);
}

// ------------------------------------------------------------------------------------------ forward apply
__global__ __launch_bounds__(kBnThreads) void bn_act_fwd(const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, bf16_t* __restrict__ y,
                                                         long long n, int C, int vl, float lo, float hi) {
  const BnLane a = bn_lane(C, vl);
  if (!a.on) return;
  const BnParams p = bn_params(mean, rstd, gamma, beta, a.v);
  uint4 q[kBnK];
  const int k = bn_load(x, a, n, C, q);
#pragma unroll
  for (int i = 0; i < kBnK; ++i) {
    if (i >= k) break;
    float f[8], xh;
    bn_unpack(q[i], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float pre = bn_pre(f[j], p.mu[j], p.rs[j], p.ga[j], p.be[j], xh);
      f[j] = pre <= lo ? lo : (pre >= hi ? hi : pre);
    }
    *reinterpret_cast<uint4*>(y + bn_elem(a, C, i)) = bn_pack(f);
  }
}

// ------------------------------------------------------------------------------------------ backward
// part: [C][chunks][2] = the chunk's sum g and sum g * xhat of the channel, g = dy where lo < pre < hi
__global__ __launch_bounds__(kBnThreads) void bn_bwd_partial(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd,
                                                             float* __restrict__ part, long long n, int C, int vl,
                                                             long long chunks, float lo, float hi) {
  __shared__ float red[kBnThreads * kBnSums];
  const BnLane a = bn_lane(C, vl);
  float acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = 0.f;
  if (a.on) {
    const BnParams p = bn_params(mean, rstd, gamma, beta, a.v);
    uint4 qx[kBnK], qd[kBnK];
    const int k = bn_load(x, a, n, C, qx);
    bn_load(dy, a, n, C, qd);
#pragma unroll
    for (int i = 0; i < kBnK; ++i) {
      if (i >= k) break;
      float f[8], d[8], xh;
      bn_unpack(qx[i], f);
      bn_unpack(qd[i], d);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float pre = bn_pre(f[j], p.mu[j], p.rs[j], p.ga[j], p.be[j], xh);
        const float g = (pre > lo && pre < hi) ? d[j] : 0.f;
        acc[j] += g;
        acc[8 + j] += g * xh;
      }
    }
  }
  float* own = red + threadIdx.x * kBnSums;
#pragma unroll
  for (int j = 0; j < 16; ++j) own[j] = acc[j];
  for (int s = a.rb >> 1; s > 0; s >>= 1) {
    __syncthreads();
    if (a.rl < s) {
      const float* o = own + s * a.vpad * kBnSums;
#pragma unroll
      for (int j = 0; j < 16; ++j) { acc[j] += o[j]; own[j] = acc[j]; }
    }
  }
  if (a.rl == 0 && a.on) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float* o = part + ((long long)(a.v * 8 + j) * chunks + blockIdx.x) * 2;
      o[0] = acc[j];
      o[1] = acc[8 + j];
    }
  }
}

__global__ __launch_bounds__(kBnThreads) void bn_bwd_finalize(const float* __restrict__ part, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta, long long chunks) {
  __shared__ float red[kBnThreads * 2];
  const int c = blockIdx.x;
  const long long per = (chunks + kBnThreads - 1) / kBnThreads;
  const long long k0 = threadIdx.x * per, k1 = min(k0 + per, chunks);
  const float* q = part + (long long)c * chunks * 2;
  float u = 0.f, w = 0.f;
  for (long long k = k0; k < k1; ++k) { u += q[2 * k]; w += q[2 * k + 1]; }
  float* own = red + threadIdx.x * 2;
  own[0] = u; own[1] = w;
  for (int s = kBnThreads >> 1; s > 0; s >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < s) {
      u += own[s * 2]; w += own[s * 2 + 1];
      own[0] = u; own[1] = w;
    }
  }
  if (threadIdx.x == 0) { dbeta[c] = u; dgamma[c] = w; }
}

// training: dx = gamma * rstd * (g - dbeta / n - xhat * dgamma / n); frozen statistics: dx = gamma * rstd * g
__global__ __launch_bounds__(kBnThreads) void bn_bwd_apply(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ dgamma, const float* __restrict__ dbeta,
                                                           bf16_t* __restrict__ dx, long long n, int C, int vl, float lo,
                                                           float hi, int training) {
  const BnLane a = bn_lane(C, vl);
  if (!a.on) return;
  const BnParams p = bn_params(mean, rstd, gamma, beta, a.v);
  float m1[8], m2[8];
  const float inv = training ? 1.0f / (float)n : 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) { m1[j] = dbeta[a.v * 8 + j] * inv; m2[j] = dgamma[a.v * 8 + j] * inv; }
  uint4 qx[kBnK], qd[kBnK];
  const int k = bn_load(x, a, n, C, qx);
  bn_load(dy, a, n, C, qd);
#pragma unroll
  for (int i = 0; i < kBnK; ++i) {
    if (i >= k) break;
    float f[8], d[8], xh;
    bn_unpack(qx[i], f);
    bn_unpack(qd[i], d);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float pre = bn_pre(f[j], p.mu[j], p.rs[j], p.ga[j], p.be[j], xh);
      const float g = (pre > lo && pre < hi) ? d[j] : 0.f;
      f[j] = p.ga[j] * p.rs[j] * (g - m1[j] - xh * m2[j]);
    }
    *reinterpret_cast<uint4*>(dx + bn_elem(a, C, i)) = bn_pack(f);
  }
}

// ------------------------------------------------------------------------------------------ host side
struct BnPlan { int vl, ytiles, rows; long long chunks; float lo, hi; };

// false for what the kernels do not serve
bool bn_plan(BnPlan& p, long long n, int C, int dtype, int act) {
  if (dtype != 1 || n < 1 || n > 0x7fffffffLL || C < 8 || C % 8 || act < 0 || act > 2) return false;
  const int V = C / 8;
  p.vl = 0;
  while ((1 << p.vl) < V && p.vl < kBnMaxVl) ++p.vl;
  p.ytiles = (V + (1 << p.vl) - 1) >> p.vl;
  p.rows = (kBnThreads >> p.vl) * kBnK;
  p.chunks = (n + p.rows - 1) / p.rows;
  p.lo = act == 0 ? -INFINITY : 0.f;
  p.hi = act == 2 ? 6.f : INFINITY;
  return p.ytiles <= 65535 && 2 * p.chunks * C <= 0x7fffffffLL;
}

inline bool bn_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// rows of a chunk (one workgroup per chunk and channel tile) at C channels; -1: not served
MXR_API int mxr_bn_chunk_rows(int C) {
  BnPlan p;
  return bn_plan(p, 1, C, 1, 0) ? p.rows : -1;
}

// floats of the work buffer of mxr_bn_stats and mxr_bn_act_bwd; -1: not served
MXR_API int mxr_bn_work(long long n, int C) {
  BnPlan p;
  return bn_plan(p, n, C, 1, 0) ? (int)(2 * p.chunks * C) : -1;
}

// x: bf16 [n, C]; mean, rstd (written), running_mean, running_var: f32 [C].  training: the batch statistics, and the
// running statistics updated in place (n >= 2); else the frozen statistics copied out.  -1: not served; -2: work too
// small.
MXR_API int mxr_bn_stats(const void* x, void* running_mean, void* running_var, void* mean, void* rstd, void* work,
                         long long work_floats, long long n, int C, float eps, float momentum, int training, int dtype,
                         hipStream_t stream) {
  BnPlan p;
  if (!bn_plan(p, n, C, dtype, 0) || !bn_aligned(x) || (training && n < 2)) return -1;
  if (!training) {
    bn_stats_frozen<<<(C + 255) / 256, 256, 0, stream>>>((const float*)running_mean, (const float*)running_var,
                                                         (float*)mean, (float*)rstd, C, eps);
    return hipGetLastError() == hipSuccess ? 0 : 1;
  }
  if (work_floats < 2 * p.chunks * C) return -2;
  bn_stats_partial<<<dim3((unsigned)p.chunks, p.ytiles), kBnThreads, 0, stream>>>((const bf16_t*)x, (float*)work, n, C,
                                                                                 p.vl, p.chunks);
  bn_stats_finalize<<<C, kBnThreads, 0, stream>>>((const float*)work, (float*)mean, (float*)rstd, (float*)running_mean,
                                                  (float*)running_var, n, p.rows, p.chunks, eps, momentum);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

// y = bf16(clamp(gamma * (x - mean) * rstd + beta)); act 0: none, 1: relu, 2: relu6
MXR_API int mxr_bn_act_fwd(const void* x, const void* gamma, const void* beta, const void* mean, const void* rstd, void* y,
                           long long n, int C, int act, int dtype, hipStream_t stream) {
  BnPlan p;
  if (!bn_plan(p, n, C, dtype, act) || !bn_aligned(x) || !bn_aligned(y)) return -1;
  bn_act_fwd<<<dim3((unsigned)p.chunks, p.ytiles), kBnThreads, 0, stream>>>(
      (const bf16_t*)x, (const float*)gamma, (const float*)beta, (const float*)mean, (const float*)rstd, (bf16_t*)y, n, C,
      p.vl, p.lo, p.hi);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

// dx bf16 [n, C], dgamma / dbeta f32 [C]; training selects the batch-statistics form of dx
MXR_API int mxr_bn_act_bwd(const void* dy, const void* x, const void* gamma, const void* beta, const void* mean,
                           const void* rstd, void* dx, void* dgamma, void* dbeta, void* work, long long work_floats,
                           long long n, int C, int act, int training, int dtype, hipStream_t stream) {
  BnPlan p;
  if (!bn_plan(p, n, C, dtype, act) || !bn_aligned(x) || !bn_aligned(dy) || !bn_aligned(dx)) return -1;
  if (work_floats < 2 * p.chunks * C) return -2;
  const dim3 grid((unsigned)p.chunks, p.ytiles);
  bn_bwd_partial<<<grid, kBnThreads, 0, stream>>>((const bf16_t*)dy, (const bf16_t*)x, (const float*)gamma,
                                                  (const float*)beta, (const float*)mean, (const float*)rstd, (float*)work,
                                                  n, C, p.vl, p.chunks, p.lo, p.hi);
  bn_bwd_finalize<<<C, kBnThreads, 0, stream>>>((const float*)work, (float*)dgamma, (float*)dbeta, p.chunks);
  bn_bwd_apply<<<grid, kBnThreads, 0, stream>>>((const bf16_t*)dy, (const bf16_t*)x, (const float*)gamma,
                                                (const float*)beta, (const float*)mean, (const float*)rstd,
                                                (const float*)dgamma, (const float*)dbeta, (bf16_t*)dx, n, C, p.vl, p.lo,
                                                p.hi, training);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
