// Depthwise 3x3 convolution on NHWC bf16 activations (fp32 accumulation): forward, data gradient and weight gradient
// of MobileNet's conv_dw_* layers.
//
//   y[n, oy, ox, c] = sum_{ky, kx} x[n, oy * s + ky - pad_top, ox * s + kx - pad_left, c] * w[ky * 3 + kx][c]
//
// with s = 1 or 2, taps outside the input reading zero (no padded copy exists), and w a tap-major [9][C] fp32 table.
//
// No matrix instruction: a depthwise conv has no reduction over channels -- 9 multiply-adds per output element, about
// 2 flops per byte at bf16.  An MFMA would need the 3x3 taps spread over the diagonal of a 16x16 or 32x32 block, 94 to
// 97 % of it zeros.  The kernels are written for bytes: 16-byte accesses along C, each input element fetched once per
// workgroup.
//
// Work split (all three kernels).  A lane owns one 8-channel vector (one 16-byte load or store).  A workgroup owns a
// chunk of cvw = 1, 2, 4 or 8 channel vectors (the smallest power of two that covers C / 8, at most 8) and a tile of
// TH x TW output pixels, TW = min(32, 128 / cvw); it has 2 * TW * cvw threads (64 to 256).  Lanes run over the chunk's
// channel vectors first, then over neighbouring output columns, so a wave's accesses are contiguous runs along C; the
// last index picks the upper or the lower half of the tile's rows.
//
// Halo: the LDS halo tile form.  The workgroup brings the ((TH - 1) * s + 3) x ((TW - 1) * s + 3) input pixels of its
// tile in once with 16-byte loads (zero where the pixel or the channel vector is outside the tensor) and every tap is
// read back from LDS.  At stride 2 the halo's columns are stored even columns first, then odd ones, so that the lanes of
// neighbouring output columns read neighbouring slots, as at stride 1.  A thread walks R output rows of its column with
// a three-row register window over the LDS tile, so an output costs 3 (stride 1) or 6 (stride 2) LDS reads, not 9.
//   stride 1: TH = 8 (R = 4), halo 10 x (TW + 2);  stride 2: TH = 4 (R = 2), halo 9 x (2 TW + 1).
//   LDS per workgroup: 20.8 to 23.0 KB at stride 1, 37.4 to 38.0 KB at stride 2 (cvw = 4 and 8).
//
// dgrad, stride 1: the forward kernel on dy with the taps flipped and the padding mirrored (2 - pad).
// dgrad, stride 2: a gather in which a lane owns the 2 x 2 quad of dx pixels with padded coordinates (2 qy + {0, 1},
// 2 qx + {0, 1}) for its channel vector: the four parity classes with their 4, 2, 2 and 1 taps are four straight-line
// sums over the same 2 x 2 window of dy, so no wave diverges on parity and every dx element -- those that no window
// reads included -- is written exactly once.  dy outside [0, Ho) x [0, Wo) reads zero from the halo.
//
// wgrad: a workgroup takes a channel chunk and a run of tpb consecutive tiles (over images, then rows, then columns);
// per tile it fills the x halo as the forward does, reads dy from global memory and adds into 9 x 8 fp32 partials per
// lane.  The lanes that share a channel vector are summed through LDS in index order, the workgroup writes one
// [9][C-chunk] partial into the workspace, and dw_wgrad_final sums the workgroups' partials per (tap, channel): eight
// interleaved sequences in index order, combined in index order.  Grid and order depend on the shapes alone: no atomics,
// two calls give the same bits.
//
// Registers / LDS as compiled (VGPRs, no scratch in any of them):
//   dw_fwd<1,4> 160   dw_fwd<2,2> 155   dw_dgrad2<2> 120   dw_wgrad<1,4> 205   dw_wgrad<2,2> 174
// (3, 3, 4, 2 and 2 waves per SIMD; the 72 tap or partial-sum registers are the floor).
#include "common.h"

namespace {

// Scalar fp32 instructions only (no v_pk_add / mul / fma_f32), as in soft_nms.hip.  (The host pass does not know the
// feature.)
#if defined(__HIP_DEVICE_COMPILE__)
#define DW_SCALAR_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define DW_SCALAR_F32
#endif

constexpr int kDwMaxThreads = 256;
constexpr int kDwFinCols = 32;      // dw_wgrad_final: (tap, channel) columns per block ...
constexpr int kDwFinLanes = 8;      // ... and interleaved row sequences per column
constexpr int kDwWgradBlocks = 2048;  // wgrad aims at about this many workgroups

struct DwGeom {
  int Hs, Ws;          // the tensor read through the halo
  int Ho, Wo;          // the tensor the tiles cover
  int C, V;            // channels, channel vectors
  int pt, pl;          // rows / columns of padding before the first source pixel
  int cvl, twl;        // log2 of the chunk's channel vectors and of the tile width
  int tiles_x, tiles_y;
};

__device__ __forceinline__ void dw_unpack(const uint4 q, float* f) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ uint4 dw_pack(const float* f) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = (uint32_t)f2bf(f[2 * i]) | ((uint32_t)f2bf(f[2 * i + 1]) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// The chunk's 9 x 8 taps of channel vector v into registers (flipped for the stride-1 data gradient).
__device__ __forceinline__ void dw_load_taps(float (&w)[9][8], const float* __restrict__ w9, int C, int v, bool vok,
                                             bool flip) {
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int s = flip ? 8 - t : t;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (vok) {
      const float4* p = reinterpret_cast<const float4*>(w9 + (long long)s * C + v * 8);
      a = p[0];
      b = p[1];
    }
    w[t][0] = a.x; w[t][1] = a.y; w[t][2] = a.z; w[t][3] = a.w;
    w[t][4] = b.x; w[t][5] = b.y; w[t][6] = b.z; w[t][7] = b.w;
  }
}

// Slot of halo column c in an LDS row of hw columns: at stride 2 even columns first, then odd ones.
template <int S>
__device__ __forceinline__ int dw_slot(int c, int hw) {
  return S == 2 ? (c >> 1) + (c & 1) * ((hw + 1) >> 1) : c;
}

// hh x hw source pixels from (iy0, ix0) of image n, channel vectors v0 .. v0 + cvw - 1, into LDS; zero outside.
template <int S>
__device__ __forceinline__ void dw_fill(uint4* halo, const bf16_t* __restrict__ src, int n, int iy0, int ix0, int hh,
                                        int hw, const DwGeom& g, int v0) {
  const int cvw = 1 << g.cvl, items = (hh * hw) << g.cvl;
#pragma unroll 4
  for (int i = threadIdx.x; i < items; i += blockDim.x) {
    const int cv = i & (cvw - 1), p = i >> g.cvl;
    const int hr = p / hw, hc = p - hr * hw;
    const int iy = iy0 + hr, ix = ix0 + hc, v = v0 + cv;
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    if (iy >= 0 && iy < g.Hs && ix >= 0 && ix < g.Ws && v < g.V)
      q = *reinterpret_cast<const uint4*>(src + (((long long)n * g.Hs + iy) * g.Ws + ix) * g.C + v * 8);
    halo[((hr * hw + dw_slot<S>(hc, hw)) << g.cvl) + cv] = q;
  }
}

// Rows [k0, 3) of the 3 x 3 window of output (row, tx) of the tile.
template <int S>
__device__ __forceinline__ void dw_window(uint4 (&win)[3][3], const uint4* halo, int k0, int row, int tx, int hw,
                                          int cvl, int cv) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k < k0) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
      win[k][kx] = halo[(((row * S + k) * hw + dw_slot<S>(tx * S + kx, hw)) << cvl) + cv];
  }
}

template <int S>
__device__ __forceinline__ void dw_slide(uint4 (&win)[3][3]) {
#pragma unroll
  for (int k = 0; k + S < 3; ++k)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) win[k][kx] = win[k + S][kx];
}

// ------------------------------------------------------------------------------------------ forward, dgrad stride 1
template <int S, int R>
__global__ __launch_bounds__(kDwMaxThreads) DW_SCALAR_F32
void dw_fwd(const bf16_t* __restrict__ x, const float* __restrict__ w9, bf16_t* __restrict__ y, const DwGeom g,
            const int flip) {
  extern __shared__ uint4 dw_halo[];
  const int tw = 1 << g.twl, cvw = 1 << g.cvl;
  const int cv = threadIdx.x & (cvw - 1), p = threadIdx.x >> g.cvl;
  const int tx = p & (tw - 1), r0 = (p >> g.twl) * R;
  const int tyi = blockIdx.x / g.tiles_x, txi = blockIdx.x - tyi * g.tiles_x;
  const int oy0 = tyi * 2 * R, ox0 = txi * tw, n = blockIdx.z;
  const int v0 = blockIdx.y * cvw, v = v0 + cv;
  const bool vok = v < g.V;
  const int hh = (2 * R - 1) * S + 3, hw = (tw - 1) * S + 3;

  float w[9][8];
  dw_load_taps(w, w9, g.C, v, vok, flip != 0);
  dw_fill<S>(dw_halo, x, n, oy0 * S - g.pt, ox0 * S - g.pl, hh, hw, g, v0);
  __syncthreads();

  uint4 win[3][3];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    dw_window<S>(win, dw_halo, r == 0 ? 0 : 3 - S, r0 + r, tx, hw, g.cvl, cv);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        float f[8];
        dw_unpack(win[k][kx], f);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(f[j], w[k * 3 + kx][j], acc[j]);
      }
    const int oy = oy0 + r0 + r, ox = ox0 + tx;
    if (vok && oy < g.Ho && ox < g.Wo)
      *reinterpret_cast<uint4*>(y + (((long long)n * g.Ho + oy) * g.Wo + ox) * g.C + v * 8) = dw_pack(acc);
    dw_slide<S>(win);
  }
}

// ------------------------------------------------------------------------------------------ dgrad, stride 2
// Tiles of 2R x TW quads over the padded dx plane; g.Hs / g.Ws are dy's Ho / Wo, g.Ho / g.Wo are dx's H / W.
template <int R>
__global__ __launch_bounds__(kDwMaxThreads) DW_SCALAR_F32
void dw_dgrad2(const bf16_t* __restrict__ dy, const float* __restrict__ w9, bf16_t* __restrict__ dx, const DwGeom g) {
  extern __shared__ uint4 dw_halo[];
  const int tw = 1 << g.twl, cvw = 1 << g.cvl;
  const int cv = threadIdx.x & (cvw - 1), p = threadIdx.x >> g.cvl;
  const int tx = p & (tw - 1), r0 = (p >> g.twl) * R;
  const int tyi = blockIdx.x / g.tiles_x, txi = blockIdx.x - tyi * g.tiles_x;
  const int qy0 = tyi * 2 * R, qx0 = txi * tw, n = blockIdx.z;
  const int v0 = blockIdx.y * cvw, v = v0 + cv;
  const bool vok = v < g.V;
  const int hh = 2 * R + 1, hw = tw + 1;   // dy rows qy0 - 1 .. qy0 + 2R - 1, columns qx0 - 1 .. qx0 + TW - 1

  float w[9][8];
  dw_load_taps(w, w9, g.C, v, vok, false);
  dw_fill<1>(dw_halo, dy, n, qy0 - 1, qx0 - 1, hh, hw, g, v0);
  __syncthreads();

  // d[a][b] = dy[qy - 1 + a][qx - 1 + b]: the window of quad (qy, qx); row a = 1 is the next quad's row a = 0
  float d[2][2][8];
#pragma unroll
  for (int b = 0; b < 2; ++b) dw_unpack(dw_halo[((r0 * hw + tx + b) << g.cvl) + cv], d[0][b]);
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int b = 0; b < 2; ++b) dw_unpack(dw_halo[(((r0 + r + 1) * hw + tx + b) << g.cvl) + cv], d[1][b]);
    float o[2][2][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // padded row 2 qy (even): taps ky = 0 from dy row qy, ky = 2 from row qy - 1; odd: ky = 1 from row qy
      o[0][0][j] = fmaf(d[0][0][j], w[8][j], fmaf(d[0][1][j], w[6][j], fmaf(d[1][0][j], w[2][j], d[1][1][j] * w[0][j])));
      o[0][1][j] = fmaf(d[0][1][j], w[7][j], d[1][1][j] * w[1][j]);
      o[1][0][j] = fmaf(d[1][0][j], w[5][j], d[1][1][j] * w[3][j]);
      o[1][1][j] = d[1][1][j] * w[4][j];
    }
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
      for (int px = 0; px < 2; ++px) {
        const int yy = 2 * (qy0 + r0 + r) + py - g.pt, xx = 2 * (qx0 + tx) + px - g.pl;
        if (vok && yy >= 0 && yy < g.Ho && xx >= 0 && xx < g.Wo)
          *reinterpret_cast<uint4*>(dx + (((long long)n * g.Ho + yy) * g.Wo + xx) * g.C + v * 8) = dw_pack(o[py][px]);
      }
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int j = 0; j < 8; ++j) d[0][b][j] = d[1][b][j];
  }
}

// ------------------------------------------------------------------------------------------ wgrad
// work: f32 [gridDim.x][9][C]; block (bx, chunk) writes the chunk's channels of row bx.
template <int S, int R>
__global__ __launch_bounds__(kDwMaxThreads) DW_SCALAR_F32
void dw_wgrad(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, float* __restrict__ work, const DwGeom g,
              const int tpb, const int ntiles) {
  extern __shared__ uint4 dw_halo[];
  const int tw = 1 << g.twl, cvw = 1 << g.cvl;
  const int cv = threadIdx.x & (cvw - 1), p = threadIdx.x >> g.cvl;
  const int tx = p & (tw - 1), r0 = (p >> g.twl) * R;
  const int v0 = blockIdx.y * cvw, v = v0 + cv;
  const bool vok = v < g.V;
  const int hh = (2 * R - 1) * S + 3, hw = (tw - 1) * S + 3;
  const int per_img = g.tiles_x * g.tiles_y;

  float acc[9][8];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[t][j] = 0.f;

  const int t0 = blockIdx.x * tpb, t1 = min(t0 + tpb, ntiles);
  for (int t = t0; t < t1; ++t) {
    const int n = t / per_img, ti = t - n * per_img;
    const int tyi = ti / g.tiles_x, txi = ti - tyi * g.tiles_x;
    const int oy0 = tyi * 2 * R, ox0 = txi * tw;
    __syncthreads();      // the previous tile's reads are done
    dw_fill<S>(dw_halo, x, n, oy0 * S - g.pt, ox0 * S - g.pl, hh, hw, g, v0);
    __syncthreads();
    uint4 win[3][3];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      dw_window<S>(win, dw_halo, r == 0 ? 0 : 3 - S, r0 + r, tx, hw, g.cvl, cv);
      const int oy = oy0 + r0 + r, ox = ox0 + tx;
      uint4 q = make_uint4(0u, 0u, 0u, 0u);
      if (vok && oy < g.Ho && ox < g.Wo)
        q = *reinterpret_cast<const uint4*>(dy + (((long long)n * g.Ho + oy) * g.Wo + ox) * g.C + v * 8);
      float d[8];
      dw_unpack(q, d);
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          float f[8];
          dw_unpack(win[k][kx], f);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[k * 3 + kx][j] = fmaf(d[j], f[j], acc[k * 3 + kx][j]);
        }
      dw_slide<S>(win);
    }
  }

  // the lanes of one channel vector, in index order, tap by tap (the halo tile is free now and large enough:
  // 32 bytes per thread against 16 * hh * hw * cvw)
  float* red = reinterpret_cast<float*>(dw_halo);
  const int npix = 2 * tw, c = threadIdx.x;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    __syncthreads();
    float4* dst = reinterpret_cast<float4*>(red + threadIdx.x * 8);
    dst[0] = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    dst[1] = make_float4(acc[t][4], acc[t][5], acc[t][6], acc[t][7]);
    __syncthreads();
    if (c < cvw * 8) {
      float s = 0.f;
      for (int i = 0; i < npix; ++i) s += red[((i << g.cvl) << 3) + c];
      const int ch = v0 * 8 + c;
      if (ch < g.C) work[((long long)blockIdx.x * 9 + t) * g.C + ch] = s;
    }
  }
}

// dw9[col] = sum over the nb rows of work[nb][ncol], fixed order.
__global__ __launch_bounds__(kDwFinCols * kDwFinLanes) DW_SCALAR_F32
void dw_wgrad_final(const float* __restrict__ work, float* __restrict__ dw9, const int nb, const int ncol) {
  __shared__ float red[kDwFinLanes][kDwFinCols];
  const int cl = threadIdx.x & (kDwFinCols - 1), lane = threadIdx.x / kDwFinCols;
  const int col = blockIdx.x * kDwFinCols + cl;
  float s = 0.f;
  if (col < ncol)
    for (int b = lane; b < nb; b += kDwFinLanes) s += work[(long long)b * ncol + col];
  red[lane][cl] = s;
  __syncthreads();
  if (lane == 0 && col < ncol) {
    float tot = red[0][cl];
#pragma unroll
    for (int i = 1; i < kDwFinLanes; ++i) tot += red[i][cl];
    dw9[col] = tot;
  }
}

// ------------------------------------------------------------------------------------------ host side
struct DwPlan { DwGeom g; int threads, chunks; size_t lds; };

inline bool dw_aligned(const void* p) { return p && ((uintptr_t)p & 15) == 0; }

// What every entry point refuses (-1), decided before any launch.
bool dw_served(int N, int H, int W, int C, int stride, int pt, int pl, int Ho, int Wo, int dtype) {
  return dtype == 1 && (stride == 1 || stride == 2) && N >= 1 && N <= 65535 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1 &&
         C >= 8 && C % 8 == 0 && pt >= 0 && pt <= 2 && pl >= 0 && pl <= 2 && H <= (1 << 24) && W <= (1 << 24) &&
         Ho <= (1 << 24) && Wo <= (1 << 24);
}

// Tiles of th x TW over an oh x ow plane, reading a plane of hs x ws through a halo of hh x hw(TW) pixels.
bool dw_plan(DwPlan& p, int C, int hs, int ws, int oh, int ow, int pt, int pl, int th, int hh, int hw_mul, int hw_add) {
  DwGeom& g = p.g;
  g.Hs = hs; g.Ws = ws; g.Ho = oh; g.Wo = ow; g.C = C; g.V = C / 8; g.pt = pt; g.pl = pl;
  g.cvl = 0;
  while ((1 << g.cvl) < g.V && g.cvl < 3) ++g.cvl;
  g.twl = g.cvl == 3 ? 4 : 5;
  const int tw = 1 << g.twl, cvw = 1 << g.cvl;
  g.tiles_x = (ow + tw - 1) / tw;
  g.tiles_y = (oh + th - 1) / th;
  p.threads = 2 * tw * cvw;
  p.chunks = (g.V + cvw - 1) / cvw;
  p.lds = (size_t)hh * (tw * hw_mul + hw_add) * cvw * sizeof(uint4);
  return (long long)g.tiles_x * g.tiles_y <= 0x3fffffffLL && p.chunks <= 65535;
}

template <int S, int R>
bool dw_plan_conv(DwPlan& p, int C, int hs, int ws, int oh, int ow, int pt, int pl) {
  // halo (2R - 1) S + 3 rows, (TW - 1) S + 3 columns
  return dw_plan(p, C, hs, ws, oh, ow, pt, pl, 2 * R, (2 * R - 1) * S + 3, S, 3 - S);
}

template <int S, int R>
int dw_launch_fwd(const void* x, const void* w9, void* y, int N, int C, int hs, int ws, int oh, int ow, int pt, int pl,
                  int flip, hipStream_t stream) {
  DwPlan p;
  if (!dw_plan_conv<S, R>(p, C, hs, ws, oh, ow, pt, pl)) return -1;
  const dim3 grid((unsigned)(p.g.tiles_x * p.g.tiles_y), p.chunks, N);
  dw_fwd<S, R><<<grid, p.threads, p.lds, stream>>>((const bf16_t*)x, (const float*)w9, (bf16_t*)y, p.g, flip);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

// workgroups along x of the wgrad grid and tiles per workgroup
template <int S, int R>
bool dw_wgrad_split(DwPlan& p, int N, int H, int W, int C, int pt, int pl, int Ho, int Wo, long long& ntiles, int& tpb,
                    long long& nbx) {
  if (!dw_plan_conv<S, R>(p, C, H, W, Ho, Wo, pt, pl)) return false;
  ntiles = (long long)N * p.g.tiles_x * p.g.tiles_y;
  if (ntiles > 0x3fffffffLL) return false;
  const long long want = kDwWgradBlocks / p.chunks > 0 ? kDwWgradBlocks / p.chunks : 1;
  tpb = (int)((ntiles + want - 1) / want);
  nbx = (ntiles + tpb - 1) / tpb;
  return true;
}

template <int S, int R>
int dw_launch_wgrad(const void* dy, const void* x, void* dw9, void* work, long long work_floats, int N, int H, int W,
                    int C, int pt, int pl, int Ho, int Wo, hipStream_t stream) {
  DwPlan p;
  long long ntiles, nbx;
  int tpb;
  if (!dw_wgrad_split<S, R>(p, N, H, W, C, pt, pl, Ho, Wo, ntiles, tpb, nbx)) return -1;
  if (work_floats < nbx * 9 * C) return -1;
  const dim3 grid((unsigned)nbx, p.chunks);
  dw_wgrad<S, R><<<grid, p.threads, p.lds, stream>>>((const bf16_t*)dy, (const bf16_t*)x, (float*)work, p.g, tpb,
                                                     (int)ntiles);
  const int ncol = 9 * C;
  dw_wgrad_final<<<(ncol + kDwFinCols - 1) / kDwFinCols, kDwFinCols * kDwFinLanes, 0, stream>>>(
      (const float*)work, (float*)dw9, (int)nbx, ncol);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace

// x: bf16 [N, H, W, C]; w9: f32 [9][C]; y: bf16 [N, Ho, Wo, C]; dtype 1 = bf16.  -1: not served.
MXR_API int mxr_dwconv3x3_fwd(const void* x, const void* w9, void* y, int N, int H, int W, int C, int stride,
                              int pad_top, int pad_left, int Ho, int Wo, int dtype, hipStream_t stream) {
  if (!dw_served(N, H, W, C, stride, pad_top, pad_left, Ho, Wo, dtype) || !dw_aligned(x) || !dw_aligned(w9) ||
      !dw_aligned(y))
    return -1;
  return stride == 1 ? dw_launch_fwd<1, 4>(x, w9, y, N, C, H, W, Ho, Wo, pad_top, pad_left, 0, stream)
                     : dw_launch_fwd<2, 2>(x, w9, y, N, C, H, W, Ho, Wo, pad_top, pad_left, 0, stream);
}

// dy: bf16 [N, Ho, Wo, C]; dx: bf16 [N, H, W, C], every element written once.
MXR_API int mxr_dwconv3x3_dgrad(const void* dy, const void* w9, void* dx, int N, int H, int W, int C, int stride,
                                int pad_top, int pad_left, int Ho, int Wo, int dtype, hipStream_t stream) {
  if (!dw_served(N, H, W, C, stride, pad_top, pad_left, Ho, Wo, dtype) || !dw_aligned(dy) || !dw_aligned(w9) ||
      !dw_aligned(dx))
    return -1;
  if (stride == 1) return dw_launch_fwd<1, 4>(dy, w9, dx, N, C, Ho, Wo, H, W, 2 - pad_top, 2 - pad_left, 1, stream);
  constexpr int R = 2;
  DwPlan p;
  // quads over padded rows 0 .. H - 1 + pad_top; the dy halo is 2R + 1 rows by TW + 1 columns
  if (!dw_plan(p, C, Ho, Wo, (H + pad_top + 1) / 2, (W + pad_left + 1) / 2, pad_top, pad_left, 2 * R, 2 * R + 1, 1, 1))
    return -1;
  p.g.Ho = H;
  p.g.Wo = W;
  const dim3 grid((unsigned)(p.g.tiles_x * p.g.tiles_y), p.chunks, N);
  dw_dgrad2<R><<<grid, p.threads, p.lds, stream>>>((const bf16_t*)dy, (const float*)w9, (bf16_t*)dx, p.g);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

// Floats of workspace mxr_dwconv3x3_wgrad needs for either stride (0: nothing it serves).
MXR_API int mxr_dwconv_wgrad_work(int N, int Ho, int Wo, int C) {
  if (N < 1 || Ho < 1 || Wo < 1 || C < 8 || C % 8) return 0;
  DwPlan p;
  long long ntiles, nb1 = 0, nb2 = 0;
  int tpb;
  if (!dw_wgrad_split<1, 4>(p, N, Ho, Wo, C, 1, 1, Ho, Wo, ntiles, tpb, nb1)) return 0;
  if (!dw_wgrad_split<2, 2>(p, N, Ho, Wo, C, 0, 0, Ho, Wo, ntiles, tpb, nb2)) return 0;
  const long long nf = (nb1 > nb2 ? nb1 : nb2) * 9 * C;
  return nf <= 0x7fffffffLL ? (int)nf : 0;
}

// dy: bf16 [N, Ho, Wo, C]; x: bf16 [N, H, W, C]; dw9: f32 [9][C]; work: f32, mxr_dwconv_wgrad_work() floats.
MXR_API int mxr_dwconv3x3_wgrad(const void* dy, const void* x, void* dw9, void* work, long long work_floats, int N,
                                int H, int W, int C, int stride, int pad_top, int pad_left, int Ho, int Wo, int dtype,
                                hipStream_t stream) {
  if (!dw_served(N, H, W, C, stride, pad_top, pad_left, Ho, Wo, dtype) || !dw_aligned(dy) || !dw_aligned(x) ||
      !dw_aligned(dw9) || !dw_aligned(work))
    return -1;
  return stride == 1 ? dw_launch_wgrad<1, 4>(dy, x, dw9, work, work_floats, N, H, W, C, pad_top, pad_left, Ho, Wo, stream)
                     : dw_launch_wgrad<2, 2>(dy, x, dw9, work, work_floats, N, H, W, C, pad_top, pad_left, Ho, Wo, stream);
}
