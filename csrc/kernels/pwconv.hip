// Pointwise (1x1) convolution on NHWC bf16 activations (fp32 accumulation): forward, data gradient and weight gradient
// of MobileNet's conv_pw_* layers.  With M = N * H * W rows, X [M, Ci], W [Co, Ci], Y [M, Co], all bf16 in memory:
//
//   forward  Y  = bf16(X . W^T)        dgrad  dX = bf16(dY . W)        wgrad  dW = dY^T . X   (fp32 [Co, Ci])
//
// These are the backbone's only contractions, so they run on the matrix unit: __builtin_amdgcn_mfma_f32_16x16x32_bf16,
// whose A operand wants row (lane & 15), 8 adjacent k from 8 * (lane >> 4) in one lane, B the same with a column, and
// whose result gives lane (lane & 15, g = lane >> 4) column lane & 15 of rows 4 g .. 4 g + 3.
//
// pw_gemm<BN> (forward, and the data gradient: the same body on a [Ci, Co] copy of the weight that pw_transpose makes
// in a caller-provided buffer -- dX = dY . (W^T)^T -- so there is no second body).
//   K is contiguous on both operands, and 8 adjacent k of one row are one 16-byte vector: no transposition anywhere.
//   The weight is the A operand (rows = output channels), the activation the B operand (columns = rows of X), so a lane
//   ends up with adjacent output channels of ONE row of Y.  A-row i of the MFMA tile pair (2 p, 2 p + 1) is given output
//   channel 32 p + 8 (i / 4) + 4 h + i % 4 (h = tile parity): lane g then holds channels 32 p + 8 g .. + 7 of its row
//   across the pair, one 16-byte store.  The permutation costs nothing: it is the order in which the weight rows are
//   laid into LDS.
//   Work split: a workgroup (4 waves) owns BN output channels (32, 64, or 128: the smallest that covers Co) and walks
//   256-row tiles of M grid-stride; a wave owns 64 rows (4 MFMA column tiles) x BN channels: 4 x BN / 16 accumulators,
//   32 MFMAs per BN / 16 LDS reads of 16 bytes (at BN = 128 the LDS port and the matrix unit are about level).
//   LDS: the weight tile [BN][kc] (rows padded by 16 bytes: the 16 rows of a read fall on distinct banks),
//   kc = min(round32(K), 128), at most 34 KB.  Registers: the accumulators and two sets of 4 activation vectors, loaded
//   from global memory straight into the B operand one k-step ahead of the MFMAs that use them.
//   Two regimes by K alone:  K <= 128 -- the resident form: the whole [BN][K] weight is laid into LDS once per
//   workgroup and the workgroup streams row tiles past it (conv_pw_1 .. 3: X read once, Y written once, weight read
//   once per workgroup);  K > 128 -- the tiled form: the weight passes through LDS in 128-k stages, two barriers per
//   stage and row tile (conv_pw_4 .. 13; X is re-read by the Co / 128 workgroups of a row tile, through L2).
//   K % 32 != 0 (K % 8 == 0 always): the vectors past K are zero on both operands by predicate; nothing is padded.
//   Rows past M and channels past Co are neither read nor written.
//
// pw_wgrad<TA, TB>: dW[co][ci] = sum_m dY[m][co] X[m][ci].  Both operands are strided along the contraction axis m (a
//   lane would need 8 elements Co or Ci apart).  Chosen: stage 64 rows of dY [64][TA] and X [64][TB] in LDS exactly as
//   they lie in memory (16-byte vectors, coalesced) and read both operands with gfx950's transposing LDS read
//   (ds_read_b64_tr_b16): 16 lanes fetch a 4-row x 16-channel block and each receives one channel's 4 rows.  That costs
//   no shuffle and no second LDS pass, where an explicit transposed store into LDS would write 2-byte elements with
//   heavy bank conflicts.  Which m a k-slot means is free as long as both operands agree: slot 8 g + e is row
//   4 g + e % 4 + 16 (e / 4) of a 32-row step, so the 16 rows of one read are adjacent and, with rows padded by 32
//   bytes, conflict-free.
//   Work split: grid (Ci / TB, Co / TA, splits); TA, TB = 32, 64 or 128, the smallest that covers Co, Ci; the 4 waves
//   tile the TA x TB block 2 x 2 (1 to 16 accumulators each).  M is split so that about 1024 workgroups exist, in
//   multiples of the 64-row stage.  The next stage is loaded into registers while this one is on the MFMA.  Every
//   workgroup writes its fp32 partial into work[split][Co][Ci]; pw_wgrad_final sums the splits per element in index
//   order (8 interleaved sequences, combined in index order).  No atomics: two calls give the same bits.
//
// The whole rule, a function of (M, Ci, Co) alone (no tuner, no table):
//   forward (K = Ci, N = Co) and dgrad (K = Co, N = Ci):  BN = 32 if N <= 32, 64 if N <= 64, else 128;
//     kc = min(round32(K), 128), stages = ceil(K / kc) (1: resident form, > 1: tiled form);
//     grid = (min(ceil(M / 256), max(1, 1024 / ceil(N / BN))), ceil(N / BN)), row tiles walked grid-stride.
//   wgrad:  TA = 32 / 64 / 128 from Co and TB from Ci by the same thresholds; grid = (ceil(Ci / TB), ceil(Co / TA), splits),
//     rows per split = round64(ceil(M / max(1, 1024 / (grid.x * grid.y)))), splits = ceil(M / rows per split).
//
// HBM passes: forward / dgrad read X (or dY) once per Co / 128 (Ci / 128) column block and write the output once;
// wgrad reads dY once per Ci / 128 and X once per Co / 128 block, and writes and reads the partials once.
//
// Registers / LDS as compiled (VGPRs + AGPRs, no scratch in any of them):
//   pw_gemm<32> 82 + 32   pw_gemm<64> 96 + 64   pw_gemm<128> 160 + 128 (one wave per SIMD)
//   LDS: dynamic, BN * (2 kc + 16) bytes, 2.6 to 34.8 KB
//   pw_wgrad<32,32> 42 + 4   pw_wgrad<64,64> 62 + 16   pw_wgrad<128,128> 110 + 64 (8, 6 and 2 waves per SIMD)
//   LDS: 64 * (2 TA + 2 TB + 64) bytes, 12 to 36 KB
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) short pw_bf16x8;
typedef __attribute__((ext_vector_type(4))) short pw_s16x4;
typedef __attribute__((ext_vector_type(4))) float pw_f32x4;

constexpr int kPwThreads = 256;
constexpr int kPwBM = 256;           // rows of a workgroup's tile: 4 waves x 4 MFMA tiles x 16
constexpr int kPwKC = 128;           // k of one LDS stage of the weight
constexpr int kPwBlocks = 1024;      // forward and wgrad aim at about this many workgroups
constexpr int kPwStage = 64;         // wgrad: rows of one LDS stage
constexpr int kPwFinCols = 32;       // pw_wgrad_final: columns per block ...
constexpr int kPwFinLanes = 8;       // ... and interleaved row sequences per column
constexpr int kPwMaxC = 16384;       // channels per side the entry points take

__device__ __forceinline__ pw_bf16x8 pw_as_frag(const uint4 q) { return __builtin_bit_cast(pw_bf16x8, q); }

// ------------------------------------------------------------------------------------------ forward, dgrad
// Y[m][n] = sum_k X[m][k] * W[n][k];  X [M][K], W [N][K], Y [M][N].  kc: k per stage (multiple of 32).
template <int BN>
__global__ __launch_bounds__(kPwThreads) void pw_gemm(const bf16_t* __restrict__ X, const bf16_t* __restrict__ W,
                                                      bf16_t* __restrict__ Y, const long long M, const int K,
                                                      const int N, const int kc, const int nstages, const int mtiles) {
  extern __shared__ uint4 pw_lds[];
  constexpr int NT = BN / 16;
  char* lds = reinterpret_cast<char*>(pw_lds);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.y * BN;
  const int rowb = kc * 2 + 16, vpr = kc >> 3;

  for (int tile = blockIdx.x; tile < mtiles; tile += gridDim.x) {
    const long long mw = (long long)tile * kPwBM + wv * 64;
    pw_f32x4 acc[4][NT];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[t][j] = pw_f32x4{0.f, 0.f, 0.f, 0.f};
    const bf16_t* xrow[4];
    bool mok[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const long long m = mw + 16 * t + li;
      mok[t] = m < M;
      xrow[t] = X + (mok[t] ? m : 0) * K + 8 * g;
    }

    for (int s = 0; s < nstages; ++s) {
      const int k0 = s * kc;
      if (nstages > 1 || tile == (int)blockIdx.x) {
        __syncthreads();                       // the previous stage's reads are done
        for (int i = threadIdx.x; i < BN * vpr; i += kPwThreads) {
          const int r = i / vpr, v = i - r * vpr;
          // LDS row r = 16 j + a is row a of MFMA tile j: output channel 32 (j / 2) + 8 (a / 4) + 4 (j % 2) + a % 4
          const int j = r >> 4, a = r & 15;
          const int n = n0 + 32 * (j >> 1) + 8 * (a >> 2) + 4 * (j & 1) + (a & 3);
          const int k = k0 + 8 * v;
          uint4 q = make_uint4(0u, 0u, 0u, 0u);
          if (n < N && k < K) q = *reinterpret_cast<const uint4*>(W + (long long)n * K + k);
          *reinterpret_cast<uint4*>(lds + r * rowb + 16 * v) = q;
        }
        __syncthreads();
      }
      const int ksteps = min(kc, (K - k0 + 31) & ~31) >> 5;
      uint4 b[4], bn[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        b[t] = make_uint4(0u, 0u, 0u, 0u);
        if (mok[t] && k0 + 8 * g < K) b[t] = *reinterpret_cast<const uint4*>(xrow[t] + k0);
      }
      for (int ks = 0; ks < ksteps; ++ks) {
        const int kn = k0 + 32 * (ks + 1);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          bn[t] = make_uint4(0u, 0u, 0u, 0u);
          if (ks + 1 < ksteps && mok[t] && kn + 8 * g < K) bn[t] = *reinterpret_cast<const uint4*>(xrow[t] + kn);
        }
        const char* arow = lds + li * rowb + (32 * ks + 8 * g) * 2;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const pw_bf16x8 a = pw_as_frag(*reinterpret_cast<const uint4*>(arow + 16 * j * rowb));
#pragma unroll
          for (int t = 0; t < 4; ++t)
            acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, pw_as_frag(b[t]), acc[t][j], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) b[t] = bn[t];
      }
    }

    // lane (li, g): row mw + 16 t + li, channels n0 + 32 p + 8 g .. + 7 from the tile pair (2 p, 2 p + 1)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const long long m = mw + 16 * t + li;
#pragma unroll
      for (int p = 0; p < NT / 2; ++p) {
        const int n = n0 + 32 * p + 8 * g;
        const pw_f32x4 lo = acc[t][2 * p], hi = acc[t][2 * p + 1];
        uint4 q;
        q.x = (uint32_t)f2bf(lo[0]) | ((uint32_t)f2bf(lo[1]) << 16);
        q.y = (uint32_t)f2bf(lo[2]) | ((uint32_t)f2bf(lo[3]) << 16);
        q.z = (uint32_t)f2bf(hi[0]) | ((uint32_t)f2bf(hi[1]) << 16);
        q.w = (uint32_t)f2bf(hi[2]) | ((uint32_t)f2bf(hi[3]) << 16);
        if (m < M && n < N) *reinterpret_cast<uint4*>(Y + m * N + n) = q;
      }
    }
  }
}

// wt[c][r] = w[r][c] for w [R][C]: the [Ci, Co] copy of the weight the data gradient runs on (2 MB at MobileNet's
// largest layer; the entry points take up to 16384 x 16384, 512 MB).  One 2-byte element per lane, reads strided by C:
// fine at a few MB out of L2, not written for more.  It is rebuilt by every dgrad call.
__global__ __launch_bounds__(kPwThreads) void pw_transpose(const bf16_t* __restrict__ w, bf16_t* __restrict__ wt,
                                                           const int R, const int C) {
  const int i = blockIdx.x * kPwThreads + threadIdx.x;
  if (i < R * C) {
    const int c = i / R, r = i - c * R;
    wt[i] = w[r * C + c];
  }
}

// ------------------------------------------------------------------------------------------ wgrad
__device__ __forceinline__ pw_s16x4 pw_tr_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) pw_s16x4*)(p));
}

// Vector i of a [64][T] stage of src [M][C] from row m0, channels c0: zero outside [m0, m1) x [0, C).
template <int T>
__device__ __forceinline__ void pw_stage_load(uint4 (&r)[T / 32], const bf16_t* __restrict__ src, long long m0,
                                              long long m1, int c0, int C) {
#pragma unroll
  for (int v = 0; v < T / 32; ++v) {
    const int i = threadIdx.x + kPwThreads * v;
    const int row = i / (T / 8), cv = i - row * (T / 8);
    const long long m = m0 + row;
    const int c = c0 + 8 * cv;
    r[v] = make_uint4(0u, 0u, 0u, 0u);
    if (m < m1 && c < C) r[v] = *reinterpret_cast<const uint4*>(src + m * C + c);
  }
}

template <int T>
__device__ __forceinline__ void pw_stage_store(char* lds, const uint4 (&r)[T / 32]) {
#pragma unroll
  for (int v = 0; v < T / 32; ++v) {
    const int i = threadIdx.x + kPwThreads * v;
    const int row = i / (T / 8), cv = i - row * (T / 8);
    *reinterpret_cast<uint4*>(lds + row * (2 * T + 32) + 16 * cv) = r[v];
  }
}

// 8 k-slots of 16-channel tile ct for the 32-row step st: slots 8 g + e = rows 4 g + e % 4 + 16 (e / 4).
template <int T>
__device__ __forceinline__ pw_bf16x8 pw_frag_tr(const char* lds, int st, int ct, int g, int q, int pp) {
  const char* p = lds + (32 * st + 4 * g + q) * (2 * T + 32) + 32 * ct + 8 * pp;
  const pw_s16x4 lo = pw_tr_read(p), hi = pw_tr_read(p + 16 * (2 * T + 32));
  return pw_bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// work: f32 [splits][Co][Ci]; block (ci block, co block, split) writes its TA x TB block of row `split`.
template <int TA, int TB>
__global__ __launch_bounds__(kPwThreads) void pw_wgrad(const bf16_t* __restrict__ dY, const bf16_t* __restrict__ X,
                                                       float* __restrict__ work, const long long M, const int Ci,
                                                       const int Co, const long long rows) {
  __shared__ __attribute__((aligned(16))) char sa[kPwStage * (2 * TA + 32)];
  __shared__ __attribute__((aligned(16))) char sb[kPwStage * (2 * TB + 32)];
  constexpr int IA = TA / 32, IB = TB / 32;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
  const int wa = wv >> 1, wb = wv & 1;
  const int ci0 = blockIdx.x * TB, co0 = blockIdx.y * TA;
  const long long m_begin = (long long)blockIdx.z * rows;
  const long long m_end = m_begin + rows < M ? m_begin + rows : M;

  pw_f32x4 acc[IA][IB];
#pragma unroll
  for (int i = 0; i < IA; ++i)
#pragma unroll
    for (int j = 0; j < IB; ++j) acc[i][j] = pw_f32x4{0.f, 0.f, 0.f, 0.f};

  uint4 ra[TA / 32], rb[TB / 32];
  pw_stage_load<TA>(ra, dY, m_begin, m_end, co0, Co);
  pw_stage_load<TB>(rb, X, m_begin, m_end, ci0, Ci);
  for (long long m0 = m_begin; m0 < m_end; m0 += kPwStage) {
    __syncthreads();                           // the previous stage's reads are done
    pw_stage_store<TA>(sa, ra);
    pw_stage_store<TB>(sb, rb);
    __syncthreads();
    if (m0 + kPwStage < m_end) {
      pw_stage_load<TA>(ra, dY, m0 + kPwStage, m_end, co0, Co);
      pw_stage_load<TB>(rb, X, m0 + kPwStage, m_end, ci0, Ci);
    }
#pragma unroll
    for (int st = 0; st < kPwStage / 32; ++st) {
      pw_bf16x8 a[IA], b[IB];
#pragma unroll
      for (int i = 0; i < IA; ++i) a[i] = pw_frag_tr<TA>(sa, st, wa * IA + i, g, q, pp);
#pragma unroll
      for (int j = 0; j < IB; ++j) b[j] = pw_frag_tr<TB>(sb, st, wb * IB + j, g, q, pp);
#pragma unroll
      for (int i = 0; i < IA; ++i)
#pragma unroll
        for (int j = 0; j < IB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }

  // C[row = co][col = ci]: column lane & 15 of ci tile wb * IB + j, rows 4 g + r of co tile wa * IA + i
  float* dst = work + (long long)blockIdx.z * Co * Ci;
#pragma unroll
  for (int i = 0; i < IA; ++i)
#pragma unroll
    for (int j = 0; j < IB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + 16 * (wa * IA + i) + 4 * g + r, ci = ci0 + 16 * (wb * IB + j) + (lane & 15);
        if (co < Co && ci < Ci) dst[(long long)co * Ci + ci] = acc[i][j][r];
      }
}

// dw[col] = sum over the nb rows of work[nb][ncol], fixed order.
__global__ __launch_bounds__(kPwFinCols * kPwFinLanes) void pw_wgrad_final(const float* __restrict__ work,
                                                                           float* __restrict__ dw, const int nb,
                                                                           const int ncol) {
  __shared__ float red[kPwFinLanes][kPwFinCols];
  const int cl = threadIdx.x & (kPwFinCols - 1), lane = threadIdx.x / kPwFinCols;
  const int col = blockIdx.x * kPwFinCols + cl;
  float s = 0.f;
  if (col < ncol)
    for (int b = lane; b < nb; b += kPwFinLanes) s += work[(long long)b * ncol + col];
  red[lane][cl] = s;
  __syncthreads();
  if (lane == 0 && col < ncol) {
    float tot = red[0][cl];
#pragma unroll
    for (int i = 1; i < kPwFinLanes; ++i) tot += red[i][cl];
    dw[col] = tot;
  }
}

// ------------------------------------------------------------------------------------------ host side
inline bool pw_aligned(const void* p) { return p && ((uintptr_t)p & 15) == 0; }

// What every entry point refuses (-1), decided before any launch.
bool pw_served(long long M, int Ci, int Co, int dtype) {
  return dtype == 1 && M >= 1 && M < 0x80000000LL && Ci >= 8 && Co >= 8 && Ci % 8 == 0 && Co % 8 == 0 &&
         Ci <= kPwMaxC && Co <= kPwMaxC;
}

inline int pw_tile(int c) { return c <= 32 ? 32 : c <= 64 ? 64 : 128; }

template <int BN>
void pw_launch_gemm(const void* x, const void* w, void* y, long long M, int K, int N, hipStream_t stream) {
  const int k32 = (K + 31) & ~31;
  const int kc = k32 < kPwKC ? k32 : kPwKC, nstages = (K + kc - 1) / kc;
  const int mtiles = (int)((M + kPwBM - 1) / kPwBM), gy = (N + BN - 1) / BN;
  const int want = kPwBlocks / gy > 0 ? kPwBlocks / gy : 1;
  const dim3 grid(mtiles < want ? mtiles : want, gy);
  pw_gemm<BN><<<grid, kPwThreads, (size_t)BN * (kc * 2 + 16), stream>>>((const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y,
                                                                        M, K, N, kc, nstages, mtiles);
}

// y [M][N] = x [M][K] . w [N][K]^T
int pw_gemm_any(const void* x, const void* w, void* y, long long M, int K, int N, hipStream_t stream) {
  switch (pw_tile(N)) {
    case 32: pw_launch_gemm<32>(x, w, y, M, K, N, stream); break;
    case 64: pw_launch_gemm<64>(x, w, y, M, K, N, stream); break;
    default: pw_launch_gemm<128>(x, w, y, M, K, N, stream); break;
  }
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

struct PwSplit { int gx, gy, splits; long long rows; };

// The weight gradient's grid: blocks over Ci and Co, and M split in multiples of the stage.
bool pw_wgrad_split(PwSplit& s, long long M, int Ci, int Co) {
  const int ta = pw_tile(Co), tb = pw_tile(Ci);
  s.gx = (Ci + tb - 1) / tb;
  s.gy = (Co + ta - 1) / ta;
  const long long want = kPwBlocks / (s.gx * s.gy) > 0 ? kPwBlocks / (s.gx * s.gy) : 1;
  s.rows = ((M + want - 1) / want + kPwStage - 1) / kPwStage * kPwStage;
  s.splits = (int)((M + s.rows - 1) / s.rows);
  return (long long)s.splits * Co * Ci <= 0x7fffffffLL;
}

template <int TA>
void pw_launch_wgrad(int tb, const dim3 grid, const bf16_t* dy, const bf16_t* x, float* work, long long M, int Ci,
                     int Co, long long rows, hipStream_t stream) {
  switch (tb) {
    case 32: pw_wgrad<TA, 32><<<grid, kPwThreads, 0, stream>>>(dy, x, work, M, Ci, Co, rows); break;
    case 64: pw_wgrad<TA, 64><<<grid, kPwThreads, 0, stream>>>(dy, x, work, M, Ci, Co, rows); break;
    default: pw_wgrad<TA, 128><<<grid, kPwThreads, 0, stream>>>(dy, x, work, M, Ci, Co, rows); break;
  }
}

}  // namespace

// x: bf16 [M, Ci]; w: bf16 [Co, Ci]; y: bf16 [M, Co]; dtype 1 = bf16.  -1: not served.
MXR_API int mxr_pwconv_fwd(const void* x, const void* w, void* y, long long M, int Ci, int Co, int dtype,
                           hipStream_t stream) {
  if (!pw_served(M, Ci, Co, dtype) || !pw_aligned(x) || !pw_aligned(w) || !pw_aligned(y)) return -1;
  return pw_gemm_any(x, w, y, M, Ci, Co, stream);
}

// dy: bf16 [M, Co]; w: bf16 [Co, Ci]; wt: bf16, Ci * Co elements of scratch (receives the [Ci, Co] copy of w);
// dx: bf16 [M, Ci], every element written once.
MXR_API int mxr_pwconv_dgrad(const void* dy, const void* w, void* wt, void* dx, long long M, int Ci, int Co, int dtype,
                             hipStream_t stream) {
  if (!pw_served(M, Ci, Co, dtype) || !pw_aligned(dy) || !pw_aligned(w) || !pw_aligned(wt) || !pw_aligned(dx)) return -1;
  pw_transpose<<<(Co * Ci + kPwThreads - 1) / kPwThreads, kPwThreads, 0, stream>>>((const bf16_t*)w, (bf16_t*)wt, Co, Ci);
  return pw_gemm_any(dy, wt, dx, M, Co, Ci, stream);
}

// Floats of workspace mxr_pwconv_wgrad needs (-1: nothing it serves).
MXR_API int mxr_pwconv_wgrad_work(long long M, int Ci, int Co) {
  PwSplit s;
  if (!pw_served(M, Ci, Co, 1) || !pw_wgrad_split(s, M, Ci, Co)) return -1;
  return (int)((long long)s.splits * Co * Ci);
}

// dy: bf16 [M, Co]; x: bf16 [M, Ci]; dw: f32 [Co, Ci]; work: f32, mxr_pwconv_wgrad_work() floats (-2: fewer).
MXR_API int mxr_pwconv_wgrad(const void* dy, const void* x, void* dw, void* work, long long work_floats, long long M,
                             int Ci, int Co, int dtype, hipStream_t stream) {
  PwSplit s;
  if (!pw_served(M, Ci, Co, dtype) || !pw_aligned(dy) || !pw_aligned(x) || !pw_aligned(dw) || !pw_aligned(work) ||
      !pw_wgrad_split(s, M, Ci, Co))
    return -1;
  if (work_floats < (long long)s.splits * Co * Ci) return -2;
  const dim3 grid(s.gx, s.gy, s.splits);
  const bf16_t* d = (const bf16_t*)dy;
  const bf16_t* a = (const bf16_t*)x;
  switch (pw_tile(Co)) {
    case 32: pw_launch_wgrad<32>(pw_tile(Ci), grid, d, a, (float*)work, M, Ci, Co, s.rows, stream); break;
    case 64: pw_launch_wgrad<64>(pw_tile(Ci), grid, d, a, (float*)work, M, Ci, Co, s.rows, stream); break;
    default: pw_launch_wgrad<128>(pw_tile(Ci), grid, d, a, (float*)work, M, Ci, Co, s.rows, stream); break;
  }
  const int ncol = Co * Ci;
  pw_wgrad_final<<<(ncol + kPwFinCols - 1) / kPwFinCols, kPwFinCols * kPwFinLanes, 0, stream>>>(
      (const float*)work, (float*)dw, s.splits, ncol);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
