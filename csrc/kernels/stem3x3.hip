// MobileNet's stem: 3x3 / stride 2 convolution of a 3-channel NHWC bf16 image (fp32 accumulation), forward and weight
// gradient.  x [N, H, W, 3], weight (Co, 3, 3, 3) OIHW, y [N, Ho, Wo, Co]; the Keras padding (one zero row below, one
// zero column on the right, valid window) is applied inside the kernels: Ho = (H - 2) / 2 + 1, Wo likewise, so the pad
// row is read only for even H and the pad column only for even W.  There is no data gradient (the image needs none),
// no bias, no activation: batch_norm.hip's statistics kernel follows.
//
// K = 3 * 3 * 3 = 27 pads to 32: one __builtin_amdgcn_mfma_f32_16x16x32_bf16 step (operand layout as in pwconv.hip:
// A row / B column lane & 15, 8 adjacent k from 8 * (lane >> 4) in one lane; the result gives a lane column lane & 15
// of rows 4 g .. 4 g + 3, g = lane >> 4).
//
// Tile: 4 output rows x 64 output columns per workgroup (4 waves, one output row each).  Its 9 input rows of
// (2 * 64 + 1) * 3 = 387 elements go through LDS (7 KB), zero outside the image.
//
// Staging.  An image row is 6 W bytes, so rows are only 2-byte aligned (for odd W every other row is 2 bytes off a
// 4-byte boundary, and a view may start there too).  Rows are therefore fetched as ALIGNED 4-byte words (a word that
// straddles an end of the row is fetched as single elements: nothing outside the row is ever read, so nothing outside
// the tensor), and a row that starts on an odd element is shifted into place by a funnel of two words.  In LDS every
// tile row starts at element 0 whatever its address was.  16-byte loads would need the same funnel over four words
// for three of four alignments; at 387 elements per row the words are already one coalesced 256-byte request per wave.
//
// K order.  For fixed ky the nine values (kx, ci) of a window are nine adjacent elements j = 3 kx + ci of one staged
// row, from element 6 * ox.  The issue proposed k = 9 ky + j; chosen instead:
//     slot 8 ky + j  for j < 8,   slot 24 + ky  for j = 8,   slots 27 .. 31 zero
// because 6 * ox is even: lane group g < 3 then reads its 8 k as FOUR ALIGNED WORDS of row ky = g, and group 3 reads
// the three leftover elements -- 4 word reads against 8 element reads and no unaligned pairs.  The order is private:
// stem3_pack lays the weight out in it and stem3_wgrad_final undoes it.
//
// Forward (stem3_fwd<NT>).  The weight is the A operand (rows = output channels), packed once per call by stem3_pack
// into bf16 [32][32] (2 KB) and resident in registers: one 16-byte vector per lane and MFMA tile.  The patches are the
// B operand (columns = 16 adjacent pixels of the wave's row).  NT = 1 (Co 8, 16): one MFMA per 16 pixels, a lane holds
// channels 4 g .. 4 g + 3 of its pixel, one 8-byte store.  NT = 2 (Co 24, 32): two MFMAs, A row i of tile h is channel
// 8 (i / 4) + 4 h + i % 4 (pwconv.hip's permutation), so a lane holds channels 8 g .. 8 g + 7, one 16-byte store.
// Accumulators are rounded to bf16 once; every element of y is written exactly once, nothing else is.
// The grid is persistent (at most 2048 workgroups walk the tiles grid-stride); the next tile's words are loaded into
// registers before this tile's MFMAs and stored to LDS after them.
//
// Weight gradient (stem3_wgrad<CV>, CV = Co / 8).  dW[co][slot] = sum over pixels of dy[pixel][co] * patch[pixel][slot]:
// the pixels are the contraction.  Same tiles, same staging of x.  The wave's 64 pixels x Co of dy are contiguous in
// memory; they are staged as they lie (16-byte vectors, coalesced) in rows of 32 channels (zero past Co) and read as
// the A operand with the transposing LDS read (ds_read_b64_tr_b16, as pwconv.hip's wgrad: k-slot 8 g + e of a 32-pixel
// step is pixel 4 g + e % 4 + 16 (e / 4)).  The B operand (columns = k slots) is gathered from the staged rows: 8
// element reads per lane and 16-slot tile, 12 bytes apart.  At most 1024 persistent workgroups; each keeps (Co / 16
// rounded up) x 2 accumulators over all its tiles, sums its 4 waves in wave order through LDS and writes one fp32
// [Co][32] partial into the caller's work buffer; stem3_wgrad_final sums the partials per element in index order (8
// interleaved sequences, combined in index order), drops slots 27 .. 31 and writes fp32 (Co, 3, 3, 3).  No atomics,
// no memset: repeat calls are bit-equal and the launches can be captured.
//
// Served (everything else returns -1 before any launch): bf16, no data gradient wanted, Co in {8, 16, 24, 32},
// H, W >= 2, N >= 1, N * H * W * 3 < 2^31 and N * Ho * Wo * 32 < 2^31 (addresses are 64-bit, tile and pixel counts
// are int).  x needs 2-byte alignment only; wpk, y, dy, dw and work 16 bytes.
//
// HBM passes: forward reads x 9 / 8 times (the shared row between row tiles; through L2) and writes y once; wgrad
// reads x 9 / 8 times and dy once, and writes and reads the partials (at most 1024 x 4 KB) once.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) short s3_bf16x8;
typedef __attribute__((ext_vector_type(4))) short s3_s16x4;
typedef __attribute__((ext_vector_type(4))) float s3_f32x4;

constexpr int kS3Threads = 256;
constexpr int kS3TR = 4;                        // output rows of a tile: one per wave
constexpr int kS3TC = 64;                       // output columns of a tile
constexpr int kS3Rows = 2 * kS3TR + 1;          // staged input rows
constexpr int kS3Words = (6 * kS3TC + 4) / 2;   // staged words per row: elements 0 .. 387 (386 is the last one read)
constexpr int kS3RS = kS3Words + 2;             // LDS row stride in words
constexpr int kS3Pre = (kS3Rows * kS3Words + kS3Threads - 1) / kS3Threads;   // words a thread stages per tile
constexpr int kS3FwdBlocks = 2048;              // persistent grids
constexpr int kS3WgBlocks = 1024;
constexpr int kS3DyRow = 96;                    // bytes of a staged dy row: 32 channels + 32 (pwconv.hip's padding)
constexpr int kS3FinOuts = 32, kS3FinLanes = 8;

struct S3Geom {
  int N, H, W, Ho, Wo, Co;
  int tx, ty, ntiles;                           // column tiles, row tiles per image, tiles
};

struct S3Tile { int n, oy0, ox0; };

__device__ __forceinline__ S3Tile s3_tile(const S3Geom& gm, int tile) {
  const int oxt = tile % gm.tx, rest = tile / gm.tx;
  return S3Tile{rest / gm.ty, (rest % gm.ty) * kS3TR, oxt * kS3TC};
}

// (ky, j = 3 kx + ci) of k slot s; false for the zero slots 27 .. 31.
__host__ __device__ __forceinline__ bool s3_slot(int s, int& ky, int& j) {
  ky = s < 24 ? s >> 3 : s - 24;
  j = s < 24 ? s & 7 : 8;
  return s < 27;
}

// The aligned word vw of the element stream that starts `a` elements before x (a = 1 if x is 2 bytes off a 4-byte
// boundary): elements 2 vw - a and 2 vw - a + 1 of x, zero where outside [lo, hi).
__device__ __forceinline__ uint32_t s3_word(const bf16_t* __restrict__ x, long long vw, int a, long long lo,
                                            long long hi) {
  const long long e0 = 2 * vw - a;
  if (e0 >= lo && e0 + 1 < hi) return *reinterpret_cast<const uint32_t*>(x + e0);
  uint32_t r = 0u;
  if (e0 >= lo && e0 < hi) r = x[e0];
  if (e0 + 1 >= lo && e0 + 1 < hi) r |= (uint32_t)x[e0 + 1] << 16;
  return r;
}

// This thread's words of the tile's 9 x 194-word stage, into registers.
__device__ __forceinline__ void s3_stage_load(uint32_t (&pre)[kS3Pre], const bf16_t* __restrict__ x, const int a,
                                              const S3Geom& gm, const S3Tile& t) {
#pragma unroll
  for (int v = 0; v < kS3Pre; ++v) {
    const int i = threadIdx.x + kS3Threads * v;
    const int r = i / kS3Words, j = i - r * kS3Words;
    const int iy = 2 * t.oy0 + r;
    pre[v] = 0u;
    if (r < kS3Rows && iy < gm.H) {
      const long long lo = ((long long)t.n * gm.H + iy) * gm.W * 3, hi = lo + 3LL * gm.W;
      const long long v0 = lo + 6LL * t.ox0 + a;             // the tile row's first element, in the aligned stream
      const long long vw = (v0 >> 1) + j;
      uint32_t w = s3_word(x, vw, a, lo, hi);
      if (v0 & 1) w = (w >> 16) | (s3_word(x, vw + 1, a, lo, hi) << 16);
      pre[v] = w;
    }
  }
}

__device__ __forceinline__ void s3_stage_store(uint32_t* s_in, const uint32_t (&pre)[kS3Pre]) {
#pragma unroll
  for (int v = 0; v < kS3Pre; ++v) {
    const int i = threadIdx.x + kS3Threads * v;
    const int r = i / kS3Words, j = i - r * kS3Words;
    if (r < kS3Rows) s_in[r * kS3RS + j] = pre[v];
  }
}

// ------------------------------------------------------------------------------------------ weight pack
// wpk bf16 [32][32]: row = A row of the forward's MFMA tiles (NT = 1: row = channel; NT = 2: row 16 h + i = channel
// 8 (i / 4) + 4 h + i % 4), column = k slot; zero past Co and past slot 26.  wdtype 0: fp32 weight, 1: bf16.
__global__ __launch_bounds__(1024) void stem3_pack(const void* __restrict__ w, const int wdtype,
                                                   bf16_t* __restrict__ wpk, const int Co) {
  const int row = threadIdx.x >> 5, s = threadIdx.x & 31;
  const int h = row >> 4, i = row & 15;
  const int ch = Co > 16 ? 8 * (i >> 2) + 4 * h + (i & 3) : row;
  int ky, j;
  bf16_t v = 0;
  if (s3_slot(s, ky, j) && ch < Co) {
    const int kx = j / 3, ci = j - 3 * kx;
    const int idx = ((ch * 3 + ci) * 3 + ky) * 3 + kx;
    v = wdtype == 0 ? f2bf(reinterpret_cast<const float*>(w)[idx]) : reinterpret_cast<const bf16_t*>(w)[idx];
  }
  wpk[threadIdx.x] = v;
}

// ------------------------------------------------------------------------------------------ forward
template <int NT>
__global__ __launch_bounds__(kS3Threads) void stem3_fwd(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wpk,
                                                        bf16_t* __restrict__ y, const S3Geom gm) {
  __shared__ uint32_t s_in[kS3Rows * kS3RS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int a = (int)(((uintptr_t)x >> 1) & 1);

  s3_bf16x8 wa[NT];
#pragma unroll
  for (int h = 0; h < NT; ++h)
    wa[h] = __builtin_bit_cast(s3_bf16x8, *reinterpret_cast<const uint4*>(wpk + (16 * h + li) * 32 + 8 * g));

  uint32_t pre[kS3Pre];
  int tile = blockIdx.x;
  if (tile < gm.ntiles) s3_stage_load(pre, x, a, gm, s3_tile(gm, tile));
  for (; tile < gm.ntiles; tile += gridDim.x) {
    const S3Tile t = s3_tile(gm, tile);
    __syncthreads();                             // the previous tile's reads are done
    s3_stage_store(s_in, pre);
    __syncthreads();
    if (tile + (int)gridDim.x < gm.ntiles) s3_stage_load(pre, x, a, gm, s3_tile(gm, tile + gridDim.x));

    const int oy = t.oy0 + wv;
    if (oy >= gm.Ho) continue;                   // wave-uniform; the barriers are above
    const uint16_t* s_el = reinterpret_cast<const uint16_t*>(s_in);
#pragma unroll
    for (int c = 0; c < kS3TC / 16; ++c) {
      const int oxl = 16 * c + li, ox = t.ox0 + oxl;
      uint4 q;
      if (g < 3) {
        const uint32_t* p = s_in + (2 * wv + g) * kS3RS + 3 * oxl;
        q = make_uint4(p[0], p[1], p[2], p[3]);
      } else {
        const uint16_t* p = s_el + (2 * wv) * (2 * kS3RS) + 6 * oxl + 8;
        q = make_uint4((uint32_t)p[0] | ((uint32_t)p[2 * kS3RS] << 16), (uint32_t)p[4 * kS3RS], 0u, 0u);
      }
      const s3_bf16x8 b = __builtin_bit_cast(s3_bf16x8, q);
      s3_f32x4 acc[NT];
#pragma unroll
      for (int h = 0; h < NT; ++h)
        acc[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[h], b, s3_f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      if (ox >= gm.Wo) continue;
      bf16_t* dst = y + (((long long)t.n * gm.Ho + oy) * gm.Wo + ox) * gm.Co;
      if (NT == 1) {
        uint2 o;
        o.x = (uint32_t)f2bf(acc[0][0]) | ((uint32_t)f2bf(acc[0][1]) << 16);
        o.y = (uint32_t)f2bf(acc[0][2]) | ((uint32_t)f2bf(acc[0][3]) << 16);
        if (4 * g < gm.Co) *reinterpret_cast<uint2*>(dst + 4 * g) = o;
      } else {
        const s3_f32x4 lo = acc[0], hi = acc[NT - 1];
        uint4 o;
        o.x = (uint32_t)f2bf(lo[0]) | ((uint32_t)f2bf(lo[1]) << 16);
        o.y = (uint32_t)f2bf(lo[2]) | ((uint32_t)f2bf(lo[3]) << 16);
        o.z = (uint32_t)f2bf(hi[0]) | ((uint32_t)f2bf(hi[1]) << 16);
        o.w = (uint32_t)f2bf(hi[2]) | ((uint32_t)f2bf(hi[3]) << 16);
        if (8 * g < gm.Co) *reinterpret_cast<uint4*>(dst + 8 * g) = o;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ weight gradient
__device__ __forceinline__ s3_s16x4 s3_tr_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s3_s16x4*)(p));
}

// The wave's 64 pixels x Co of dy for this tile: CV vectors per lane, contiguous in memory; zero outside y.
template <int CV>
__device__ __forceinline__ void s3_dy_load(uint4 (&d)[CV], const bf16_t* __restrict__ dy, const S3Geom& gm,
                                           const S3Tile& t, const int wv, const int lane) {
  const int oy = t.oy0 + wv;
#pragma unroll
  for (int v = 0; v < CV; ++v) {
    const int idx = lane + 64 * v;
    const int px = idx / CV, cv = idx - px * CV;
    d[v] = make_uint4(0u, 0u, 0u, 0u);
    if (oy < gm.Ho && t.ox0 + px < gm.Wo)
      d[v] = *reinterpret_cast<const uint4*>(dy + (((long long)t.n * gm.Ho + oy) * gm.Wo + t.ox0 + px) * gm.Co + 8 * cv);
  }
}

template <int CV>
__device__ __forceinline__ void s3_dy_store(char* s_dy_wave, const uint4 (&d)[CV], const int lane) {
#pragma unroll
  for (int v = 0; v < CV; ++v) {
    const int idx = lane + 64 * v;
    const int px = idx / CV, cv = idx - px * CV;
    *reinterpret_cast<uint4*>(s_dy_wave + px * kS3DyRow + 16 * cv) = d[v];
  }
}

// work: f32 [gridDim.x][Co][32]; this workgroup writes row blockIdx.x whole.
template <int CV>
__global__ __launch_bounds__(kS3Threads) void stem3_wgrad(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                          float* __restrict__ work, const S3Geom gm) {
  constexpr int NT = (CV + 1) / 2;               // 16-channel tiles of dy
  __shared__ uint32_t s_in[kS3Rows * kS3RS];
  __shared__ __attribute__((aligned(16))) char s_dy[kS3TR * kS3TC * kS3DyRow];
  static_assert(sizeof(float) * 4 * NT * 2 * kS3Threads <= sizeof(s_dy), "the wave reduce reuses s_dy");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
  const int a = (int)(((uintptr_t)x >> 1) & 1);
  char* s_dy_wave = s_dy + wv * kS3TC * kS3DyRow;

  // channels past Co of the staged dy rows are never written again: zero once (the loop's first barrier orders it)
  for (int i = threadIdx.x; i < (int)sizeof(s_dy) / 16; i += kS3Threads)
    reinterpret_cast<uint4*>(s_dy)[i] = make_uint4(0u, 0u, 0u, 0u);

  // the B operand's gather: column li of slot tile s is k slot 16 s + li -> element j of staged row 2 wv + ky
  int boff[2];
  bool bok[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    int ky, j;
    bok[s] = s3_slot(16 * s + li, ky, j);
    boff[s] = bok[s] ? (2 * wv + ky) * (2 * kS3RS) + j : 0;
  }

  s3_f32x4 acc[NT][2];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int s = 0; s < 2; ++s) acc[i][s] = s3_f32x4{0.f, 0.f, 0.f, 0.f};

  uint32_t pre[kS3Pre];
  uint4 dpre[CV];
  int tile = blockIdx.x;
  if (tile < gm.ntiles) {
    const S3Tile t = s3_tile(gm, tile);
    s3_stage_load(pre, x, a, gm, t);
    s3_dy_load<CV>(dpre, dy, gm, t, wv, lane);
  }
  for (; tile < gm.ntiles; tile += gridDim.x) {
    const S3Tile t = s3_tile(gm, tile);
    __syncthreads();                             // the previous tile's reads are done
    s3_stage_store(s_in, pre);
    s3_dy_store<CV>(s_dy_wave, dpre, lane);
    __syncthreads();
    if (tile + (int)gridDim.x < gm.ntiles) {
      const S3Tile tn = s3_tile(gm, tile + gridDim.x);
      s3_stage_load(pre, x, a, gm, tn);
      s3_dy_load<CV>(dpre, dy, gm, tn, wv, lane);
    }
    if (t.oy0 + wv >= gm.Ho) continue;           // wave-uniform: this wave's dy rows are all zero
    const uint16_t* s_el = reinterpret_cast<const uint16_t*>(s_in);
#pragma unroll
    for (int st = 0; st < kS3TC / 32; ++st) {
      s3_bf16x8 fa[NT], fb[2];
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const char* p = s_dy_wave + (32 * st + 4 * g + q) * kS3DyRow + 32 * i + 8 * pp;
        const s3_s16x4 lo = s3_tr_read(p), hi = s3_tr_read(p + 16 * kS3DyRow);
        fa[i] = s3_bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int px = 32 * st + 4 * g + (e & 3) + 16 * (e >> 2);
          fb[s][e] = bok[s] ? (short)s_el[boff[s] + 6 * px] : (short)0;
        }
      }
#pragma unroll
      for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int s = 0; s < 2; ++s) acc[i][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[s], acc[i][s], 0, 0, 0);
    }
  }

  // the 4 waves' sums in wave order; acc[i][s][r] of lane (li, g) is channel 16 i + 4 g + r, slot 16 s + li
  __syncthreads();
  float* red = reinterpret_cast<float*>(s_dy);
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[((wv * NT * 2 + i * 2 + s) * 4 + r) * 64 + lane] = acc[i][s][r];
  __syncthreads();
  float* dst = work + (long long)blockIdx.x * gm.Co * 32;
  for (int o = threadIdx.x; o < NT * 2 * 4 * 64; o += kS3Threads) {
    float tot = red[o];
#pragma unroll
    for (int w = 1; w < 4; ++w) tot += red[w * NT * 2 * 4 * 64 + o];
    const int ln = o & 63, r = (o >> 6) & 3, s = (o >> 8) & 1, i = o >> 9;
    const int co = 16 * i + 4 * (ln >> 4) + r, slot = 16 * s + (ln & 15);
    if (co < gm.Co) dst[co * 32 + slot] = tot;
  }
}

// dw (Co, 3, 3, 3) OIHW = the nb partials [Co][32] summed per element in index order, slots mapped back.
__global__ __launch_bounds__(kS3FinOuts * kS3FinLanes) void stem3_wgrad_final(const float* __restrict__ work,
                                                                              float* __restrict__ dw, const int nb,
                                                                              const int Co) {
  __shared__ float red[kS3FinLanes][kS3FinOuts];
  const int ol = threadIdx.x & (kS3FinOuts - 1), seq = threadIdx.x / kS3FinOuts;
  const int o = blockIdx.x * kS3FinOuts + ol;
  float sum = 0.f;
  if (o < Co * 27) {
    const int co = o / 27, rem = o - 27 * co;
    const int ci = rem / 9, ky = (rem - 9 * ci) / 3, kx = rem - 9 * ci - 3 * ky;
    const int j = 3 * kx + ci;
    const int slot = j < 8 ? 8 * ky + j : 24 + ky;
    for (int b = seq; b < nb; b += kS3FinLanes) sum += work[((long long)b * Co + co) * 32 + slot];
  }
  red[seq][ol] = sum;
  __syncthreads();
  if (seq == 0 && o < Co * 27) {
    float tot = red[0][ol];
#pragma unroll
    for (int i = 1; i < kS3FinLanes; ++i) tot += red[i][ol];
    dw[o] = tot;
  }
}

// ------------------------------------------------------------------------------------------ host side
inline bool s3_aligned(const void* p, uintptr_t to) { return p && ((uintptr_t)p & (to - 1)) == 0; }

// What every entry point refuses (-1), decided before any launch; fills the geometry.
bool s3_served(S3Geom& gm, long long N, long long H, long long W, int Co, int dtype, int want_dx) {
  if (dtype != 1 || want_dx != 0 || N < 1 || H < 2 || W < 2 || Co < 8 || Co > 32 || Co % 8 != 0) return false;
  if (H >= 0x80000000LL || W >= 0x80000000LL || N >= 0x80000000LL) return false;
  const long long Ho = (H - 2) / 2 + 1, Wo = (W - 2) / 2 + 1;
  if (H * W >= 0x80000000LL || N * H * W * 3 >= 0x80000000LL || N * Ho * Wo * 32 >= 0x80000000LL) return false;
  gm.N = (int)N; gm.H = (int)H; gm.W = (int)W; gm.Ho = (int)Ho; gm.Wo = (int)Wo; gm.Co = Co;
  gm.tx = (gm.Wo + kS3TC - 1) / kS3TC;
  gm.ty = (gm.Ho + kS3TR - 1) / kS3TR;
  gm.ntiles = gm.N * gm.ty * gm.tx;
  return true;
}

inline int s3_blocks(const S3Geom& gm, int cap) { return gm.ntiles < cap ? gm.ntiles : cap; }

}  // namespace

// w: the (Co, 3, 3, 3) OIHW weight, fp32 (wdtype 0) or bf16 (1); wpk: bf16, 1024 elements, all written.
MXR_API int mxr_stem3_pack(const void* w, int wdtype, void* wpk, int Co, hipStream_t stream) {
  if (!w || !s3_aligned(wpk, 16) || (wdtype != 0 && wdtype != 1) || Co < 8 || Co > 32 || Co % 8 != 0) return -1;
  stem3_pack<<<1, 1024, 0, stream>>>(w, wdtype, (bf16_t*)wpk, Co);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

// x: bf16 [N, H, W, 3]; wpk: mxr_stem3_pack's image for this Co; y: bf16 [N, Ho, Wo, Co]; dtype 1 = bf16; want_dx:
// nonzero if the caller needs a gradient of x (never served).  -1: not served.
MXR_API int mxr_stem3_fwd(const void* x, const void* wpk, void* y, long long N, long long H, long long W, int Co,
                          int dtype, int want_dx, hipStream_t stream) {
  S3Geom gm;
  if (!s3_served(gm, N, H, W, Co, dtype, want_dx) || !s3_aligned(x, 2) || !s3_aligned(wpk, 16) || !s3_aligned(y, 16))
    return -1;
  const int grid = s3_blocks(gm, kS3FwdBlocks);
  if (Co <= 16)
    stem3_fwd<1><<<grid, kS3Threads, 0, stream>>>((const bf16_t*)x, (const bf16_t*)wpk, (bf16_t*)y, gm);
  else
    stem3_fwd<2><<<grid, kS3Threads, 0, stream>>>((const bf16_t*)x, (const bf16_t*)wpk, (bf16_t*)y, gm);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

// Floats of workspace mxr_stem3_wgrad needs for an [N, Ho, Wo, Co] dy (-1: nothing it serves).
MXR_API int mxr_stem3_wgrad_work(long long N, long long Ho, long long Wo, int Co) {
  S3Geom gm;
  if (Ho < 1 || Wo < 1 || !s3_served(gm, N, 2 * Ho, 2 * Wo, Co, 1, 0)) return -1;
  return s3_blocks(gm, kS3WgBlocks) * Co * 32;
}

// dy: bf16 [N, Ho, Wo, Co]; x: bf16 [N, H, W, 3]; dw: f32 (Co, 3, 3, 3); work: f32, mxr_stem3_wgrad_work() floats
// (-2: fewer).
MXR_API int mxr_stem3_wgrad(const void* dy, const void* x, void* dw, void* work, long long work_floats, long long N,
                            long long H, long long W, int Co, int dtype, hipStream_t stream) {
  S3Geom gm;
  if (!s3_served(gm, N, H, W, Co, dtype, 0) || !s3_aligned(dy, 16) || !s3_aligned(x, 2) || !s3_aligned(dw, 16) ||
      !s3_aligned(work, 16))
    return -1;
  const int grid = s3_blocks(gm, kS3WgBlocks);
  if (work_floats < (long long)grid * Co * 32) return -2;
  const bf16_t* d = (const bf16_t*)dy;
  const bf16_t* a = (const bf16_t*)x;
  switch (Co / 8) {
    case 1: stem3_wgrad<1><<<grid, kS3Threads, 0, stream>>>(d, a, (float*)work, gm); break;
    case 2: stem3_wgrad<2><<<grid, kS3Threads, 0, stream>>>(d, a, (float*)work, gm); break;
    case 3: stem3_wgrad<3><<<grid, kS3Threads, 0, stream>>>(d, a, (float*)work, gm); break;
    default: stem3_wgrad<4><<<grid, kS3Threads, 0, stream>>>(d, a, (float*)work, gm); break;
  }
  stem3_wgrad_final<<<(Co * 27 + kS3FinOuts - 1) / kS3FinOuts, kS3FinOuts * kS3FinLanes, 0, stream>>>(
      (const float*)work, (float*)dw, grid, Co);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
