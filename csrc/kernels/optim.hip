// Keras-Adam + clipnorm over the flat fp32 parameter/gradient buffers (multi-tensor, fused).
//
// Spec: keras.optimizers.adam(lr=1e-5, clipnorm=0.001) at /root/reference/train.py:104
// (SURVEY §2.8.7): global-norm clip, lr_t = lr*sqrt(1-b2^t)/(1-b1^t), eps OUTSIDE the bias
// correction.  Hyper-parameters and the step counter live in device memory, so the whole
// optimizer is graph-capturable and never syncs with the host:
//   hyper[0] = lr_t (written by the prologue), hyper[1] = lr, iteration counter int64.
// The same pass refreshes the bf16 "compute" weights (W * frozen-BN scale) the forward reads.
//
// Keras-SGD (momentum, nesterov, coupled L2 weight decay) runs over the same tables in one launch:
//   g_eff = g * grad_scale + wd[seg] * p ;  v = momentum * v - lr * g_eff ;
//   p += v   (nesterov: p += momentum * v - lr * g_eff)
// with lr = hyper[1] and momentum = hyper[2] read from device memory (a replayed graph sees a changed value).
//
// Weight EMA (the EMA forms of both kernels, a compile-time parameter): after p_new the same thread loads the
// matching elements of the fp32 average and stores  ema = d * ema + (1 - d) * p_new,  with
//   d = hyper[3] = min(D, (1 + n) / (10 + n)),  n = *iter + 1 - ema_start  (1-based index of this EMA update),
// written by a one-thread prologue that reads the step counter BEFORE this step advances it: a replayed graph gets
// a new d every step.  mxr_swap_refresh exchanges weights and average in place (evaluation on the average).
#include "common.h"

namespace {

struct Chunk {
  long long start;   // flat element offset
  int len;           // elements in this chunk (multiple of 4 except possibly the last of a segment)
  int seg;           // segment index
};
struct Seg {
  long long offset;     // flat offset of the segment
  long long scale_off;  // offset into the scale vector (per output channel) or -1
  int row_len;          // elements per output channel
  int has_copy;         // write the bf16 compute copy
};

constexpr int kBlock = 256;

// d_n of the EMA update that follows the step which takes the counter from `it` to `it + 1` (fp32, as the host
// mirror KerasAdam.ema_decay_at computes it).
__device__ __forceinline__ float ema_decay_of(long long it, float D, long long ema_start) {
  const long long n = it + 1 - ema_start;
  return fminf(D, __fdiv_rn((float)(1 + n), (float)(10 + n)));
}

// SGD's EMA forms: one thread, launched in front of sgd_kernel (whose block 0 advances *iter during the launch).
__global__ void ema_prologue(float* hyper, const long long* iter, float D, long long ema_start) {
  hyper[3] = ema_decay_of(*iter, D, ema_start);
}

template <bool EMA>
__global__ void adam_prologue(float* hyper, long long* iter, float b1, float b2, float D, long long ema_start) {
  if (EMA) hyper[3] = ema_decay_of(*iter, D, ema_start);
  const long long t = *iter + 1;
  const float lr = hyper[1];
  hyper[0] = lr * sqrtf(1.f - powf(b2, (float)t)) / (1.f - powf(b1, (float)t));
  *iter = t;
}

template <bool EMA>
__global__ __launch_bounds__(kBlock) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                      float* __restrict__ m, float* __restrict__ v,
                                                      float* __restrict__ ema, bf16_t* __restrict__ wcopy,
                                                      const float* __restrict__ scales,
                                                      const Chunk* __restrict__ chunks, const Seg* __restrict__ segs,
                                                      const float* __restrict__ grad_scale,
                                                      const float* __restrict__ hyper, float b1, float b2, float eps) {
  const Chunk c = chunks[blockIdx.x];
  const Seg s = segs[c.seg];
  const float gs = *grad_scale;
  const float lr_t = hyper[0];
  const float d = EMA ? hyper[3] : 0.f;
  const long long base = c.start;
  // chunk starts are 4-aligned (segments are 64-aligned, chunk length multiple of 4)
  const int nv = c.len >> 2;
  for (int i = threadIdx.x; i < nv; i += kBlock) {
    const long long e = base + 4LL * i;
    float4 pp = *reinterpret_cast<const float4*>(p + e);
    const float4 gg = *reinterpret_cast<const float4*>(g + e);
    float4 mm = *reinterpret_cast<const float4*>(m + e);
    float4 vv = *reinterpret_cast<const float4*>(v + e);
    float* pa = &pp.x; const float* ga = &gg.x; float* ma = &mm.x; float* va = &vv.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gj = ga[j] * gs;
      ma[j] = b1 * ma[j] + (1.f - b1) * gj;
      va[j] = b2 * va[j] + (1.f - b2) * gj * gj;
      pa[j] -= lr_t * ma[j] / (sqrtf(va[j]) + eps);
    }
    *reinterpret_cast<float4*>(p + e) = pp;
    *reinterpret_cast<float4*>(m + e) = mm;
    *reinterpret_cast<float4*>(v + e) = vv;
    if (EMA) {
      float4 ee = *reinterpret_cast<const float4*>(ema + e);
      float* ea = &ee.x;
#pragma unroll
      for (int j = 0; j < 4; ++j) ea[j] = d * ea[j] + (1.f - d) * pa[j];
      *reinterpret_cast<float4*>(ema + e) = ee;
    }
    if (s.has_copy) {
      const long long le = e - s.offset;
      ushort4 w;
      unsigned short* wa = &w.x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float sc = 1.f;
        if (s.scale_off >= 0) sc = scales[s.scale_off + (le + j) / s.row_len];
        wa[j] = f2bf(pa[j] * sc);
      }
      *reinterpret_cast<ushort4*>(wcopy + e) = w;
    }
  }
  // scalar tail (segment lengths that are not multiples of 4)
  for (int i = (nv << 2) + threadIdx.x; i < c.len; i += kBlock) {
    const long long e = base + i;
    const float gj = g[e] * gs;
    const float mj = b1 * m[e] + (1.f - b1) * gj;
    const float vj = b2 * v[e] + (1.f - b2) * gj * gj;
    const float pj = p[e] - lr_t * mj / (sqrtf(vj) + eps);
    m[e] = mj; v[e] = vj; p[e] = pj;
    if (s.has_copy) {
      float sc = 1.f;
      if (s.scale_off >= 0) sc = scales[s.scale_off + (e - s.offset) / s.row_len];
      wcopy[e] = f2bf(pj * sc);
    }
  }
  // The average's tail is a loop of its own, over the elements this thread has just written: inside the loop above
  // the compiler pairs its multiply-add with the update's (packed fp32 math) and un-fuses the update's fma on the
  // way, and the EMA forms must update p and the slots bit for bit as the plain forms do.
  if (EMA) {
    for (int i = (nv << 2) + threadIdx.x; i < c.len; i += kBlock) {
      const long long e = base + i;
      ema[e] = d * ema[e] + (1.f - d) * p[e];
    }
  }
}

// One element of the SGD update; returns the new parameter, updates the velocity in place.
template <bool NESTEROV, bool DECAY>
__device__ __forceinline__ float sgd_elem(float p, float g, float& v, float gs, float wd, float lr, float mom) {
  float ge = g * gs;
  if (DECAY) ge += wd * p;
  v = mom * v - lr * ge;
  return NESTEROV ? p + mom * v - lr * ge : p + v;
}

template <bool NESTEROV, bool DECAY, bool EMA>
__global__ __launch_bounds__(kBlock) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                     float* __restrict__ v, float* __restrict__ ema,
                                                     bf16_t* __restrict__ wcopy,
                                                     const float* __restrict__ scales, const Chunk* __restrict__ chunks,
                                                     const Seg* __restrict__ segs, const float* __restrict__ seg_wd,
                                                     const float* __restrict__ grad_scale,
                                                     const float* __restrict__ hyper, long long* __restrict__ iter) {
  const Chunk c = chunks[blockIdx.x];
  const Seg s = segs[c.seg];
  const float gs = *grad_scale;
  const float lr = hyper[1];
  const float mom = hyper[2];
  const float wd = DECAY ? seg_wd[c.seg] : 0.f;
  const float d = EMA ? hyper[3] : 0.f;     // ema_prologue wrote it from the counter as it stood before this launch
  // the step counter: nothing in this launch reads it
  if (blockIdx.x == 0 && threadIdx.x == 0) *iter = *iter + 1;
  const long long base = c.start;
  const int nv = c.len >> 2;
  for (int i = threadIdx.x; i < nv; i += kBlock) {
    const long long e = base + 4LL * i;
    float4 pp = *reinterpret_cast<const float4*>(p + e);
    const float4 gg = *reinterpret_cast<const float4*>(g + e);
    float4 vv = *reinterpret_cast<const float4*>(v + e);
    float* pa = &pp.x; const float* ga = &gg.x; float* va = &vv.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) pa[j] = sgd_elem<NESTEROV, DECAY>(pa[j], ga[j], va[j], gs, wd, lr, mom);
    *reinterpret_cast<float4*>(p + e) = pp;
    *reinterpret_cast<float4*>(v + e) = vv;
    if (EMA) {
      float4 ee = *reinterpret_cast<const float4*>(ema + e);
      float* ea = &ee.x;
#pragma unroll
      for (int j = 0; j < 4; ++j) ea[j] = d * ea[j] + (1.f - d) * pa[j];
      *reinterpret_cast<float4*>(ema + e) = ee;
    }
    if (s.has_copy) {
      const long long le = e - s.offset;
      ushort4 w;
      unsigned short* wa = &w.x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float sc = 1.f;
        if (s.scale_off >= 0) sc = scales[s.scale_off + (le + j) / s.row_len];
        wa[j] = f2bf(pa[j] * sc);
      }
      *reinterpret_cast<ushort4*>(wcopy + e) = w;
    }
  }
  // scalar tail (segment lengths that are not multiples of 4)
  for (int i = (nv << 2) + threadIdx.x; i < c.len; i += kBlock) {
    const long long e = base + i;
    float vj = v[e];
    const float pj = sgd_elem<NESTEROV, DECAY>(p[e], g[e], vj, gs, wd, lr, mom);
    v[e] = vj; p[e] = pj;
    if (s.has_copy) {
      float sc = 1.f;
      if (s.scale_off >= 0) sc = scales[s.scale_off + (e - s.offset) / s.row_len];
      wcopy[e] = f2bf(pj * sc);
    }
  }
  // the average's tail: a loop of its own, as in adam_kernel
  if (EMA) {
    for (int i = (nv << 2) + threadIdx.x; i < c.len; i += kBlock) {
      const long long e = base + i;
      ema[e] = d * ema[e] + (1.f - d) * p[e];
    }
  }
}

// Refresh only the bf16 compute copy (after loading weights / broadcast).
__global__ __launch_bounds__(kBlock) void copy_kernel(const float* __restrict__ p, bf16_t* __restrict__ wcopy,
                                                      const float* __restrict__ scales, const Chunk* __restrict__ chunks,
                                                      const Seg* __restrict__ segs) {
  const Chunk c = chunks[blockIdx.x];
  const Seg s = segs[c.seg];
  if (!s.has_copy) return;
  for (int i = threadIdx.x; i < c.len; i += kBlock) {
    const long long e = c.start + i;
    float sc = 1.f;
    if (s.scale_off >= 0) sc = scales[s.scale_off + (e - s.offset) / s.row_len];
    wcopy[e] = f2bf(p[e] * sc);
  }
}

// Exchange the weights and their moving average in place and write the bf16 compute copy of the new weights.
__global__ __launch_bounds__(kBlock) void swap_kernel(float* __restrict__ p, float* __restrict__ ema,
                                                      bf16_t* __restrict__ wcopy, const float* __restrict__ scales,
                                                      const Chunk* __restrict__ chunks, const Seg* __restrict__ segs) {
  const Chunk c = chunks[blockIdx.x];
  const Seg s = segs[c.seg];
  const long long base = c.start;
  const int nv = c.len >> 2;
  for (int i = threadIdx.x; i < nv; i += kBlock) {
    const long long e = base + 4LL * i;
    const float4 pp = *reinterpret_cast<const float4*>(p + e);
    const float4 ee = *reinterpret_cast<const float4*>(ema + e);
    *reinterpret_cast<float4*>(p + e) = ee;
    *reinterpret_cast<float4*>(ema + e) = pp;
    if (s.has_copy) {
      const long long le = e - s.offset;
      const float* na = &ee.x;
      ushort4 w;
      unsigned short* wa = &w.x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float sc = 1.f;
        if (s.scale_off >= 0) sc = scales[s.scale_off + (le + j) / s.row_len];
        wa[j] = f2bf(na[j] * sc);
      }
      *reinterpret_cast<ushort4*>(wcopy + e) = w;
    }
  }
  for (int i = (nv << 2) + threadIdx.x; i < c.len; i += kBlock) {
    const long long e = base + i;
    const float pj = p[e], ej = ema[e];
    p[e] = ej; ema[e] = pj;
    if (s.has_copy) {
      float sc = 1.f;
      if (s.scale_off >= 0) sc = scales[s.scale_off + (e - s.offset) / s.row_len];
      wcopy[e] = f2bf(ej * sc);
    }
  }
}

constexpr int kNormGrid = 1024;

__global__ __launch_bounds__(kBlock) void sumsq_kernel(const float* __restrict__ g, long long n, float* __restrict__ partials) {
  __shared__ float red[16];
  float acc = 0.f;
  const long long nv = n >> 2;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < nv; i += (long long)gridDim.x * kBlock) {
    const float4 x = g4[i];
    acc += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
  }
  for (long long i = (nv << 2) + blockIdx.x * (long long)kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock)
    acc += g[i] * g[i];
  const float s = block_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// out[0] = norm = sqrt(sum) * norm_mul ; out[1] = clip factor * scale_mul (the Adam grad scale)
__global__ __launch_bounds__(256) void norm_finalize(const float* __restrict__ partials, int n, float norm_mul,
                                                     float clipnorm, float scale_mul, float* __restrict__ out) {
  __shared__ float red[16];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) acc += partials[i];
  const float s = block_sum(acc, red);
  if (threadIdx.x == 0) {
    const float norm = sqrtf(s) * norm_mul;
    float f = 1.f;
    if (clipnorm > 0.f && norm >= clipnorm) f = clipnorm / norm;
    out[0] = norm;
    out[1] = f * scale_mul;
  }
}

__global__ __launch_bounds__(kBlock) void scale_kernel(float* __restrict__ g, long long n, const float* __restrict__ s) {
  const float f = *s;
  const long long nv = n >> 2;
  float4* g4 = reinterpret_cast<float4*>(g);
  for (long long i = blockIdx.x * (long long)kBlock + threadIdx.x; i < nv; i += (long long)gridDim.x * kBlock) {
    float4 x = g4[i];
    x.x *= f; x.y *= f; x.z *= f; x.w *= f;
    g4[i] = x;
  }
  for (long long i = (nv << 2) + blockIdx.x * (long long)kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock)
    g[i] *= f;
}

}  // namespace

MXR_API int mxr_chunk_struct_sizes(int* out) {
  out[0] = sizeof(Chunk);
  out[1] = sizeof(Seg);
  return 0;
}

MXR_API int mxr_adam_step(float* p, const float* g, float* m, float* v, void* wcopy, const float* scales,
                          const void* chunks, int nchunks, const void* segs, const float* grad_scale, float* hyper,
                          long long* iter, float b1, float b2, float eps, hipStream_t stream) {
  adam_prologue<false><<<1, 1, 0, stream>>>(hyper, iter, b1, b2, 0.f, 0);
  adam_kernel<false><<<nchunks, kBlock, 0, stream>>>(p, g, m, v, nullptr, (bf16_t*)wcopy, scales,
                                                     (const Chunk*)chunks, (const Seg*)segs, grad_scale, hyper, b1, b2,
                                                     eps);
  return (int)hipGetLastError();
}

// The EMA form: `ema` is the fp32 average (shaped like p), D the decay cap, ema_start the step count at its seeding.
MXR_API int mxr_adam_step_ema(float* p, const float* g, float* m, float* v, float* ema, void* wcopy,
                              const float* scales, const void* chunks, int nchunks, const void* segs,
                              const float* grad_scale, float* hyper, long long* iter, float b1, float b2, float eps,
                              float D, long long ema_start, hipStream_t stream) {
  if (!ema || nchunks <= 0) return (int)hipErrorInvalidValue;
  adam_prologue<true><<<1, 1, 0, stream>>>(hyper, iter, b1, b2, D, ema_start);
  adam_kernel<true><<<nchunks, kBlock, 0, stream>>>(p, g, m, v, ema, (bf16_t*)wcopy, scales, (const Chunk*)chunks,
                                                    (const Seg*)segs, grad_scale, hyper, b1, b2, eps);
  return (int)hipGetLastError();
}

// seg_wd: one weight-decay factor per segment, or null (no decay anywhere: the form without the multiply).
MXR_API int mxr_sgd_step(float* p, const float* g, float* v, void* wcopy, const float* scales, const void* chunks,
                         int nchunks, const void* segs, const float* seg_wd, const float* grad_scale,
                         const float* hyper, long long* iter, int nesterov, hipStream_t stream) {
#define MXR_SGD(N, D, E, EMA)                                                                                 \
  sgd_kernel<N, D, E><<<nchunks, kBlock, 0, stream>>>(p, g, v, EMA, (bf16_t*)wcopy, scales,                   \
                                                      (const Chunk*)chunks, (const Seg*)segs, seg_wd, grad_scale, \
                                                      hyper, iter)
  if (nchunks <= 0) return (int)hipErrorInvalidValue;
  if (nesterov) {
    if (seg_wd) MXR_SGD(true, true, false, nullptr); else MXR_SGD(true, false, false, nullptr);
  } else {
    if (seg_wd) MXR_SGD(false, true, false, nullptr); else MXR_SGD(false, false, false, nullptr);
  }
  return (int)hipGetLastError();
}

// The EMA forms (as mxr_adam_step_ema); the prologue launch belongs to them alone.
MXR_API int mxr_sgd_step_ema(float* p, const float* g, float* v, float* ema, void* wcopy, const float* scales,
                             const void* chunks, int nchunks, const void* segs, const float* seg_wd,
                             const float* grad_scale, float* hyper, long long* iter, int nesterov, float D,
                             long long ema_start, hipStream_t stream) {
  if (!ema || nchunks <= 0) return (int)hipErrorInvalidValue;
  ema_prologue<<<1, 1, 0, stream>>>(hyper, iter, D, ema_start);
  if (nesterov) {
    if (seg_wd) MXR_SGD(true, true, true, ema); else MXR_SGD(true, false, true, ema);
  } else {
    if (seg_wd) MXR_SGD(false, true, true, ema); else MXR_SGD(false, false, true, ema);
  }
#undef MXR_SGD
  return (int)hipGetLastError();
}

// Exchange p and ema element by element and write the bf16 W*s compute copy of the new p: one pass, no temporary.
MXR_API int mxr_swap_refresh(float* p, float* ema, void* wcopy, const float* scales, const void* chunks, int nchunks,
                             const void* segs, hipStream_t stream) {
  if (!p || !ema || nchunks <= 0) return (int)hipErrorInvalidValue;
  swap_kernel<<<nchunks, kBlock, 0, stream>>>(p, ema, (bf16_t*)wcopy, scales, (const Chunk*)chunks, (const Seg*)segs);
  return (int)hipGetLastError();
}

MXR_API int mxr_refresh_copy(const float* p, void* wcopy, const float* scales, const void* chunks, int nchunks,
                             const void* segs, hipStream_t stream) {
  copy_kernel<<<nchunks, kBlock, 0, stream>>>(p, (bf16_t*)wcopy, scales, (const Chunk*)chunks, (const Seg*)segs);
  return (int)hipGetLastError();
}

// out: 2 floats (norm, grad scale). partials: kNormGrid floats.
MXR_API int mxr_grad_norm_clip(const float* g, long long n, float* partials, float norm_mul, float clipnorm,
                               float scale_mul, float* out, hipStream_t stream) {
  sumsq_kernel<<<kNormGrid, kBlock, 0, stream>>>(g, n, partials);
  norm_finalize<<<1, 256, 0, stream>>>(partials, kNormGrid, norm_mul, clipnorm, scale_mul, out);
  return (int)hipGetLastError();
}

MXR_API int mxr_scale_inplace(float* g, long long n, const float* s, hipStream_t stream) {
  scale_kernel<<<mxr_grid(n / 4 + 1, kBlock, 4096), kBlock, 0, stream>>>(g, n, s);
  return (int)hipGetLastError();
}

MXR_API int mxr_norm_grid() { return kNormGrid; }
