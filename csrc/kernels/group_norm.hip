// GroupNorm + ReLU on the packed ragged pyramid [B, P, C] (bf16, batch-major): the head towers of --head-norm gn.
//
//   y = relu(gamma * (x - mean) * rstd + beta),   mean / rstd per (image, level, group) over the level's pixels and
//   the group's C / G channels -- F.group_norm on the level's own [B, C, h, w] tensor.
//
// Work split: a level of an image is cut into chunks of kGnRows pixels, one block each; the grid is B * chunks, a
// function of B, the level shapes and C alone (a captured step replays).  In a block a thread owns one 16-byte
// vector column (8 channels, all of one group: channels per group are 8 or 16) and walks the chunk's rows.
//
// No atomics: every reduction is per-block partials (combined across the block's threads through LDS in a fixed
// order) and a finalize launch that walks the partials in a fixed order -- two calls give the same bits.
//
// Statistics: a block takes its chunk's (count, mean, M2) per group in two passes -- the mean first, then the squares
// of the distances from it -- and the finalize combines the chunks with Chan's formula.
//
// The ReLU mask is not stored: the backward recomputes the pre-activation with gn_pre(), the helper the forward
// uses, compiled without FMA contraction so both give the same bits (see atss_key in targets.hip).
#include "common.h"

namespace {

constexpr int kGnMaxLev = 5;
constexpr int kGnRows = 128;      // pixels of one level per block
constexpr int kGnThreads = 256;
constexpr int kGnFinThreads = 1024;
constexpr int kGnFinLanes = kGnFinThreads / 64;   // partial rows summed side by side per channel

struct GnLevels {
  int nlev;
  int off[kGnMaxLev];         // first row of the level inside an image's P rows
  int n[kGnMaxLev];           // pixels of the level
  int cstart[kGnMaxLev + 1];  // first chunk of the level; cstart[nlev] = chunks per image
};

struct GnSeg { int b, l, off, n, cs; };

__device__ __forceinline__ GnSeg gn_level(const GnLevels& lv, int b, int l) {
  GnSeg s = {b, l, lv.off[0], lv.n[0], lv.cstart[0]};
#pragma unroll
  for (int i = 1; i < kGnMaxLev; ++i)
    if (i == l) { s.off = lv.off[i]; s.n = lv.n[i]; s.cs = lv.cstart[i]; }
  return s;
}

// block -> (image, level, rows [r0, r1) of the level)
__device__ __forceinline__ GnSeg gn_locate(const GnLevels& lv, int blk, int& r0, int& r1) {
  const int T = lv.cstart[lv.nlev];
  const int b = blk / T, c = blk - b * T;
  int l = 0;
#pragma unroll
  for (int i = 1; i < kGnMaxLev; ++i)
    if (i < lv.nlev && c >= lv.cstart[i]) l = i;
  const GnSeg s = gn_level(lv, b, l);
  r0 = (c - s.cs) * kGnRows;
  r1 = min(r0 + kGnRows, s.n);
  return s;
}

// The pre-activation, every operation rounded on its own: forward and backward agree on its sign bit for bit.
__device__ __forceinline__ float gn_pre(float x, float mean, float rstd, float gamma, float beta, float& xhat) {
#pragma clang fp contract(off)
  const float d = x - mean;
  xhat = d * rstd;
  const float t = xhat * gamma;
  return t + beta;
}

__device__ __forceinline__ void gn_unpack(const uint4 q, float* f) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ uint4 gn_pack(const float* f) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = (uint32_t)f2bf(f[2 * i]) | ((uint32_t)f2bf(f[2 * i + 1]) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// A thread's place in its block: vector column v (8 channels), row lane rl of rb.
struct GnLane { int v, col, rl, rb, vpad; bool on; };

__device__ __forceinline__ GnLane gn_lane(int C, int vl) {
  GnLane a;
  a.vpad = 1 << vl;
  a.col = threadIdx.x & (a.vpad - 1);
  a.v = blockIdx.y * a.vpad + a.col;
  a.rl = threadIdx.x >> vl;
  a.rb = kGnThreads >> vl;
  a.on = a.v < (C >> 3);
  return a;
}

// ------------------------------------------------------------------------------------------ forward
// per block and group: the chunk's mean and M2 = sum (x - mean)^2, two passes over the chunk (the second one reads
// what the first one left in the caches)
__global__ __launch_bounds__(kGnThreads) void gn_stats_partial(const bf16_t* __restrict__ x, float* __restrict__ part,
                                                               GnLevels lv, int P, int C, int cpg, int vl) {
  __shared__ float red[kGnThreads];
  __shared__ float gmean[kGnThreads];
  int r0, r1;
  const GnSeg s = gn_locate(lv, blockIdx.x, r0, r1);
  const GnLane a = gn_lane(C, vl);
  const int gpv = cpg >> 3, G = C / cpg, ngt = a.vpad / gpv;   // vectors per group, groups of this block's columns
  const int g = blockIdx.y * ngt + threadIdx.x;                // the group thread < ngt finishes
  const long long row0 = (long long)s.b * P + s.off;
  const float nk = (float)((r1 - r0) * cpg);
  float s1 = 0.f;
  if (a.on)
    for (int r = r0 + a.rl; r < r1; r += a.rb) {
      float f[8];
      gn_unpack(*reinterpret_cast<const uint4*>(x + (row0 + r) * C + a.v * 8), f);
      s1 += ((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7]));
    }
  red[threadIdx.x] = s1;
  __syncthreads();
  float mk = 0.f;
  if (threadIdx.x < ngt) {
    float u = 0.f;
    for (int i = 0; i < a.rb; ++i)
      for (int j = 0; j < gpv; ++j) u += red[i * a.vpad + threadIdx.x * gpv + j];
    mk = u / nk;
    gmean[threadIdx.x] = mk;
  }
  __syncthreads();
  float s2 = 0.f;
  if (a.on) {
    const float m = gmean[a.col / gpv];
    for (int r = r0 + a.rl; r < r1; r += a.rb) {
      float f[8];
      gn_unpack(*reinterpret_cast<const uint4*>(x + (row0 + r) * C + a.v * 8), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float d = f[j] - m; f[j] = d * d; }
      s2 += ((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7]));
    }
  }
  red[threadIdx.x] = s2;
  __syncthreads();
  if (threadIdx.x < ngt && g < G) {
    float w = 0.f;
    for (int i = 0; i < a.rb; ++i)
      for (int j = 0; j < gpv; ++j) w += red[i * a.vpad + threadIdx.x * gpv + j];
    float* o = part + ((long long)blockIdx.x * G + g) * 2;
    o[0] = mk;
    o[1] = w;
  }
}

// one thread per (image, level, group): Chan's combination of the chunks' (count, mean, M2), in chunk order
__global__ void gn_stats_finalize(const float* __restrict__ part, float* __restrict__ mean, float* __restrict__ rstd,
                                  GnLevels lv, int B, int C, int cpg, float eps) {
  const int G = C / cpg, idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * lv.nlev * G) return;
  const int g = idx % G, l = (idx / G) % lv.nlev, b = idx / (G * lv.nlev);
  const GnSeg s = gn_level(lv, b, l);
  const int T = lv.cstart[lv.nlev];
  float m = 0.f, M2 = 0.f, cnt = 0.f;
  for (int r = 0, k = s.cs; r < s.n; r += kGnRows, ++k) {
    const float nk = (float)(min(kGnRows, s.n - r) * cpg);
    const float* q = part + ((long long)(b * T + k) * G + g) * 2;   // the chunk's mean and M2
    const float d = q[0] - m, tot = cnt + nk;
    m += d * (nk / tot);
    M2 += q[1] + d * d * (cnt * nk / tot);
    cnt = tot;
  }
  const float var = cnt > 0.f ? fmaxf(M2 / cnt, 0.f) : 0.f;
  mean[idx] = m;
  rstd[idx] = 1.0f / sqrtf(var + eps);
}

__global__ __launch_bounds__(kGnThreads) void gn_relu_apply(const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, bf16_t* __restrict__ y,
                                                            GnLevels lv, int P, int C, int cpg, int vl) {
  int r0, r1;
  const GnSeg s = gn_locate(lv, blockIdx.x, r0, r1);
  const GnLane a = gn_lane(C, vl);
  if (!a.on) return;
  const int G = C / cpg, st = (s.b * lv.nlev + s.l) * G + (a.v * 8) / cpg;
  const float mu = mean[st], rs = rstd[st];
  float ga[8], be[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { ga[j] = gamma[a.v * 8 + j]; be[j] = beta[a.v * 8 + j]; }
  const long long row0 = (long long)s.b * P + s.off;
  for (int r = r0 + a.rl; r < r1; r += a.rb) {
    const long long e = (row0 + r) * C + a.v * 8;
    float f[8], xh;
    gn_unpack(*reinterpret_cast<const uint4*>(x + e), f);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float pre = gn_pre(f[j], mu, rs, ga[j], be[j], xh);
      f[j] = pre > 0.f ? pre : 0.f;
    }
    *reinterpret_cast<uint4*>(y + e) = gn_pack(f);
  }
}

// ------------------------------------------------------------------------------------------ backward
constexpr int kGnAcc = 18;    // per thread: dbeta[8], dgamma[8], s1, s2

// per block: s1 = sum g*gamma, s2 = sum g*gamma*xhat per group; sum g and sum g*xhat per channel
__global__ __launch_bounds__(kGnThreads) void gn_bwd_partial(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd,
                                                             float* __restrict__ ps, float* __restrict__ pc, GnLevels lv,
                                                             int P, int C, int cpg, int vl, long long nblk) {
  __shared__ float red[kGnThreads * kGnAcc];
  int r0, r1;
  const GnSeg s = gn_locate(lv, blockIdx.x, r0, r1);
  const GnLane a = gn_lane(C, vl);
  const int G = C / cpg;
  float acc[kGnAcc];
#pragma unroll
  for (int j = 0; j < kGnAcc; ++j) acc[j] = 0.f;
  if (a.on) {
    const int st = (s.b * lv.nlev + s.l) * G + (a.v * 8) / cpg;
    const float mu = mean[st], rs = rstd[st];
    float ga[8], be[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { ga[j] = gamma[a.v * 8 + j]; be[j] = beta[a.v * 8 + j]; }
    const long long row0 = (long long)s.b * P + s.off;
    for (int r = r0 + a.rl; r < r1; r += a.rb) {
      const long long e = (row0 + r) * C + a.v * 8;
      float f[8], d[8], xh;
      gn_unpack(*reinterpret_cast<const uint4*>(x + e), f);
      gn_unpack(*reinterpret_cast<const uint4*>(dy + e), d);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float pre = gn_pre(f[j], mu, rs, ga[j], be[j], xh);
        const float g = pre > 0.f ? d[j] : 0.f;
        const float gg = g * ga[j];
        acc[j] += g;
        acc[8 + j] += g * xh;
        acc[16] += gg;
        acc[17] += gg * xh;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kGnAcc; ++j) red[threadIdx.x * kGnAcc + j] = acc[j];
  __syncthreads();
  const int gpv = cpg >> 3;
  const int g = blockIdx.y * (a.vpad / gpv) + threadIdx.x;
  if (threadIdx.x < a.vpad / gpv && g < G) {
    float u = 0.f, w = 0.f;
    for (int i = 0; i < a.rb; ++i)
      for (int j = 0; j < gpv; ++j) {
        const int k = i * a.vpad + threadIdx.x * gpv + j;
        u += red[k * kGnAcc + 16];
        w += red[k * kGnAcc + 17];
      }
    float* o = ps + ((long long)blockIdx.x * G + g) * 2;
    o[0] = u;
    o[1] = w;
  }
  for (int ci = threadIdx.x; ci < a.vpad * 8; ci += kGnThreads) {
    const int col = ci >> 3, j = ci & 7, c = (blockIdx.y * a.vpad + col) * 8 + j;
    if (c >= C) continue;
    float u = 0.f, w = 0.f;
    for (int i = 0; i < a.rb; ++i) {
      const int k = (i * a.vpad + col) * kGnAcc + j;
      u += red[k];
      w += red[k + 8];
    }
    pc[(long long)blockIdx.x * C + c] = u;              // dbeta
    pc[(nblk + blockIdx.x) * C + c] = w;                // dgamma
  }
}

// blocks [0, ncb): 64 channels each, dbeta / dgamma over all block partials (kGnFinLanes strided sums, then their
// fixed-order total); blocks from ncb on: one thread per (image, level, group), s1 / s2 over the level's chunks
__global__ __launch_bounds__(kGnFinThreads) void gn_bwd_finalize(const float* __restrict__ ps, const float* __restrict__ pc,
                                                                 float* __restrict__ sg, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta, GnLevels lv, int B, int C, int cpg,
                                                                 int ncb, long long nblk) {
  __shared__ float red[kGnFinThreads * 2];
  if ((int)blockIdx.x < ncb) {
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), lane = threadIdx.x >> 6;
    float u = 0.f, w = 0.f;
    if (c < C)
      for (long long j = lane; j < nblk; j += kGnFinLanes) {
        u += pc[j * C + c];
        w += pc[(nblk + j) * C + c];
      }
    red[threadIdx.x * 2] = u;
    red[threadIdx.x * 2 + 1] = w;
    __syncthreads();
    if (threadIdx.x < 64 && c < C) {
      u = 0.f; w = 0.f;
      for (int i = 0; i < kGnFinLanes; ++i) {
        u += red[(i * 64 + threadIdx.x) * 2];
        w += red[(i * 64 + threadIdx.x) * 2 + 1];
      }
      dbeta[c] = u;
      dgamma[c] = w;
    }
    return;
  }
  const int G = C / cpg, idx = (blockIdx.x - ncb) * kGnFinThreads + threadIdx.x;
  if (idx >= B * lv.nlev * G) return;
  const int g = idx % G, l = (idx / G) % lv.nlev, b = idx / (G * lv.nlev);
  const GnSeg s = gn_level(lv, b, l);
  const int T = lv.cstart[lv.nlev];
  float u = 0.f, w = 0.f;
  for (int r = 0, k = s.cs; r < s.n; r += kGnRows, ++k) {
    const float* q = ps + ((long long)(b * T + k) * G + g) * 2;
    u += q[0];
    w += q[1];
  }
  sg[idx * 2] = u;
  sg[idx * 2 + 1] = w;
}

__global__ __launch_bounds__(kGnThreads) void gn_bwd_apply(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ sg, bf16_t* __restrict__ dx, GnLevels lv,
                                                           int P, int C, int cpg, int vl) {
  int r0, r1;
  const GnSeg s = gn_locate(lv, blockIdx.x, r0, r1);
  const GnLane a = gn_lane(C, vl);
  if (!a.on) return;
  const int G = C / cpg, st = (s.b * lv.nlev + s.l) * G + (a.v * 8) / cpg;
  const float mu = mean[st], rs = rstd[st];
  const float inv = 1.0f / ((float)s.n * (float)cpg);
  const float m1 = sg[st * 2] * inv, m2 = sg[st * 2 + 1] * inv;
  float ga[8], be[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { ga[j] = gamma[a.v * 8 + j]; be[j] = beta[a.v * 8 + j]; }
  const long long row0 = (long long)s.b * P + s.off;
  for (int r = r0 + a.rl; r < r1; r += a.rb) {
    const long long e = (row0 + r) * C + a.v * 8;
    float f[8], d[8], xh;
    gn_unpack(*reinterpret_cast<const uint4*>(x + e), f);
    gn_unpack(*reinterpret_cast<const uint4*>(dy + e), d);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float pre = gn_pre(f[j], mu, rs, ga[j], be[j], xh);
      const float g = pre > 0.f ? d[j] : 0.f;
      f[j] = rs * (g * ga[j] - m1 - xh * m2);
    }
    *reinterpret_cast<uint4*>(dx + e) = gn_pack(f);
  }
}

// ------------------------------------------------------------------------------------------ host side
struct GnPlan { GnLevels lv; int cpg, vl, ytiles; long long nblk; };

// false for what the kernels do not serve
bool gn_plan(GnPlan& p, int B, long long P, int C, int groups, int nlev, const int* lev, int dtype) {
  if (dtype != 1 || nlev < 1 || nlev > kGnMaxLev || B < 1 || C < 8 || C % 8 || groups < 1 || C % groups) return false;
  p.cpg = C / groups;
  if (p.cpg != 8 && p.cpg != 16) return false;
  p.lv.nlev = nlev;
  long long rows = 0, chunks = 0;
  for (int i = 0; i < kGnMaxLev; ++i) {
    const int off = i < nlev ? lev[2 * i] : 0, n = i < nlev ? lev[2 * i + 1] : 0;
    if (off < 0 || n < 0 || (long long)off + n > P) return false;
    p.lv.off[i] = off;
    p.lv.n[i] = n;
    p.lv.cstart[i] = (int)chunks;
    chunks += (n + kGnRows - 1) / kGnRows;
    rows += n;
  }
  p.lv.cstart[kGnMaxLev] = (int)chunks;
  p.lv.cstart[nlev] = (int)chunks;
  p.nblk = chunks * B;
  if (chunks < 1 || rows > P || p.nblk > 0x7fffffffLL || (long long)B * nlev * groups > 0x3fffffffLL) return false;
  const int V = C / 8;
  p.vl = 0;
  while ((1 << p.vl) < V && (1 << p.vl) < kGnThreads) ++p.vl;
  if ((1 << p.vl) < p.cpg / 8) p.vl = 1;
  p.ytiles = (V + (1 << p.vl) - 1) >> p.vl;
  return p.ytiles <= 65535;
}

inline bool gn_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

MXR_API int mxr_gn_chunk_rows() { return kGnRows; }

// x, y: bf16 [B, P, C]; lev: nlev pairs (row offset, pixels) on the host; mean / rstd: f32 [B, nlev, groups];
// part: f32 workspace of part_floats >= 2 * B * chunks * groups.  -1: not served; -2: workspace too small.
MXR_API int mxr_gn_relu_fwd(const void* x, const void* gamma, const void* beta, void* y, void* mean, void* rstd,
                            void* part, long long part_floats, int B, long long P, int C, int groups, float eps, int nlev,
                            const int* lev, int dtype, hipStream_t stream) {
  GnPlan p;
  if (!gn_plan(p, B, P, C, groups, nlev, lev, dtype) || P > 0x7fffffffLL || !gn_aligned(x) || !gn_aligned(y)) return -1;
  if (part_floats < 2 * p.nblk * groups) return -2;
  const dim3 grid((unsigned)p.nblk, p.ytiles);
  const int nst = B * nlev * groups;
  gn_stats_partial<<<grid, kGnThreads, 0, stream>>>((const bf16_t*)x, (float*)part, p.lv, (int)P, C, p.cpg, p.vl);
  gn_stats_finalize<<<(nst + 255) / 256, 256, 0, stream>>>((const float*)part, (float*)mean, (float*)rstd, p.lv, B, C,
                                                           p.cpg, eps);
  gn_relu_apply<<<grid, kGnThreads, 0, stream>>>((const bf16_t*)x, (const float*)gamma, (const float*)beta,
                                                 (const float*)mean, (const float*)rstd, (bf16_t*)y, p.lv, (int)P, C,
                                                 p.cpg, p.vl);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

// work: f32 workspace of work_floats >= 2 * B * chunks * (groups + C) + 2 * B * nlev * groups.
MXR_API int mxr_gn_relu_bwd(const void* dy, const void* x, const void* gamma, const void* beta, const void* mean,
                            const void* rstd, void* dx, void* dgamma, void* dbeta, void* work, long long work_floats, int B,
                            long long P, int C, int groups, int nlev, const int* lev, int dtype, hipStream_t stream) {
  GnPlan p;
  if (!gn_plan(p, B, P, C, groups, nlev, lev, dtype) || P > 0x7fffffffLL || !gn_aligned(x) || !gn_aligned(dy) ||
      !gn_aligned(dx))
    return -1;
  const long long nps = 2 * p.nblk * groups, npc = 2 * p.nblk * C, nsg = 2LL * B * nlev * groups;
  if (work_floats < nps + npc + nsg) return -2;
  float* ps = (float*)work;
  float* pc = ps + nps;
  float* sg = pc + npc;
  const dim3 grid((unsigned)p.nblk, p.ytiles);
  const int nst = B * nlev * groups, ncb = (C + 63) / 64;
  gn_bwd_partial<<<grid, kGnThreads, 0, stream>>>((const bf16_t*)dy, (const bf16_t*)x, (const float*)gamma,
                                                  (const float*)beta, (const float*)mean, (const float*)rstd, ps, pc, p.lv,
                                                  (int)P, C, p.cpg, p.vl, p.nblk);
  gn_bwd_finalize<<<ncb + (nst + kGnFinThreads - 1) / kGnFinThreads, kGnFinThreads, 0, stream>>>(
      ps, pc, sg, (float*)dgamma, (float*)dbeta, p.lv, B, C, p.cpg, ncb, p.nblk);
  gn_bwd_apply<<<grid, kGnThreads, 0, stream>>>((const bf16_t*)dy, (const bf16_t*)x, (const float*)gamma,
                                                (const float*)beta, (const float*)mean, (const float*)rstd, sg,
                                                (bf16_t*)dx, p.lv, (int)P, C, p.cpg, p.vl);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
