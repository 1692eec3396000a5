// Row activity of a sparse gradient over the packed pyramid (the regression tower's backward).
//
// The regression loss has a gradient on positive anchors only, so the gradient entering the regression final is
// zero on all but a fraction of a percent of the packed rows, and every 3x3 data gradient below it widens that
// support by one pixel.  The backward's kernels derive the support FROM THE DATA (no contract with the loss or
// assigner):
//
// * mxr_rows_nonzero: [rows, ld] bf16 -> one bit per row (bit m % 64 of 64-bit word m / 64: word t is exactly the
//   64-row K-tile t of conv_wgrad_p8.hip); a row is set when any element is not +-0;
// * mxr_rows_dilate: the 1 .. nd-fold 3x3 dilations of a row mask per image and level (ConvGeom pyramid tables):
//   conservative supersets of the gradient supports one .. nd layers further down (relu masks ignored);
// * mxr_halo_active_tiles: per mask, the halo tiles (halo_tile.h) whose boxes, extended by one pixel and clipped
//   to the level, hold a set bit -- as a permutation of the tile indices: the active tiles first (ascending), the
//   inactive ones behind them, and the active count in device memory (conv_hx32.hip walks the list; the loop
//   bounds are read on the device: no host synchronisation).  mxr_halo_active_tiles_ext: the same with a mask
//   index and an extension of 0 or 1 pixels per list (0: the tiles whose own OUTPUT pixels meet the mask).
//
// The sparse FORWARD of the regression tower starts from a contract instead: THE LOSS READS THE REGRESSION OUTPUT ON
// state == 1 ROWS ONLY (smooth_l1_kernel / iou_loss_kernel in losses.hip), so the final's output is needed on the
// rows M0 that own a positive anchor and the tower layer k layers below it on the k-fold dilation of M0:
//
// * mxr_rows_positive: the assigner's int8 anchor states -> the row mask M0 (a packed row owns `group` anchors).
//
// Nothing here can check that contract.  The Trainer enforces it: it hands the model the anchor states for a
// forward only when the losses it is about to run read the regression output that way (Trainer.forward_backward's
// request); without the request the forward is dense.
#include "common.h"
#include "conv_common.h"
#include "halo_tile.h"

typedef unsigned long long u64;

namespace {

__global__ __launch_bounds__(256) void rows_nonzero_kernel(const uint4* __restrict__ dy, long long rows, int cpr,
                                                           u64* __restrict__ mask) {
  __shared__ unsigned int bits[2];
  if (threadIdx.x < 2) bits[threadIdx.x] = 0u;
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * 64;
  const int nr = (int)(rows - r0 < 64 ? rows - r0 : 64);
  const int n = nr * cpr;   // 16-B chunks of this word's rows (contiguous: ld = 8 cpr)
  const uint4* src = dy + r0 * cpr;
  for (int c = threadIdx.x; c < n; c += 256) {
    const uint4 v = src[c];
    if (((v.x | v.y | v.z | v.w) & 0x7fff7fffu) != 0u) {
      const int r = c / cpr;
      atomicOr(&bits[r >> 5], 1u << (r & 31));
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) mask[blockIdx.x] = (u64)bits[0] | ((u64)bits[1] << 32);
}

// one thread per packed row: a wave's 64 rows are one word; rows past `rows` vote clear
__global__ __launch_bounds__(256) void rows_positive_kernel(const int8_t* __restrict__ state, long long rows, int group,
                                                            long long nw, u64* __restrict__ mask) {
  const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
  bool pos = false;
  if (m < rows) {
    const int8_t* s = state + m * group;
    for (int a = 0; a < group; ++a) pos |= s[a] == 1;
  }
  const u64 bal = __ballot(pos);
  const long long word = m >> 6;
  if ((threadIdx.x & 63) == 0 && word < nw) mask[word] = bal;
}

// bits [s, s + len) of the mask (len <= 32, s + len <= 64 nw)
__device__ __forceinline__ u64 ra_bits(const u64* __restrict__ mask, long long nw, long long s, int len) {
  const long long w = s >> 6;
  const int o = (int)(s & 63);
  u64 v = mask[w] >> o;
  if (o + len > 64 && w + 1 < nw) v |= mask[w + 1] << (64 - o);
  return v & ((1ull << len) - 1ull);
}

constexpr int RA_MAXD = 8;

__global__ __launch_bounds__(256) void rows_dilate_kernel(const u64* __restrict__ in, u64* __restrict__ out, int nd,
                                                          long long stride, long long nw, ConvGeom g) {
  const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
  int dmin = 2 * RA_MAXD;   // Chebyshev distance to the nearest set pixel of the same image and level
  if (m < g.M) {
    const int b = (int)(m / g.out_img);
    const int q = (int)(m - (long long)b * g.out_img);
    LevelSel s;
    select_level(g, q, s);
    const int loc = q - s.mstart;
    const int y = loc / s.wo, x = loc - y * s.wo;
    const long long base = (long long)b * g.out_img + s.mstart;
    const int xa = max(0, x - nd), xb = min(s.W - 1, x + nd);
    const int cx = x - xa;
    for (int dy = -nd; dy <= nd; ++dy) {
      const int yy = y + dy;
      if ((unsigned)yy >= (unsigned)s.H) continue;
      const u64 w = ra_bits(in, nw, base + (long long)yy * s.W + xa, xb - xa + 1);
      if (w == 0ull) continue;
      int dh = 2 * RA_MAXD;
      const u64 lo = w & ((2ull << cx) - 1ull);   // set pixels at or left of x
      if (lo) dh = cx - (63 - __builtin_clzll(lo));
      const u64 hi = w >> cx;                     // at or right of x
      if (hi) dh = min(dh, (int)__builtin_ctzll(hi));
      dmin = min(dmin, max(dh, dy < 0 ? -dy : dy));
    }
  }
  const long long word = m >> 6;   // a wave's 64 rows are one word
  for (int k = 1; k <= nd; ++k) {
    const u64 bal = __ballot(dmin <= k);
    if ((threadIdx.x & 63) == 0 && word < nw) out[(long long)(k - 1) * stride + word] = bal;
  }
}

// ext: the boxes extended by that many pixels (1: the tile's halo, 0: its output pixels), clipped to the level
__device__ __forceinline__ bool ra_tile_active(const HaloTile& T, const u64* __restrict__ mask, int ext) {
  for (int b = 0; b < T.nbox; ++b) {
    const HaloBox& B = T.b[b];
    const int ya = max(0, B.y0 - ext), yb = min(B.H - 1, B.y0 + B.R - 1 + ext);
    const int xa = max(0, B.x0 - ext), xb = min(B.W - 1, B.x0 + B.C - 1 + ext);
    for (int yy = ya; yy <= yb; ++yy) {
      long long s = (long long)B.out_base + (long long)yy * B.W + xa;
      int len = xb - xa + 1;
      while (len > 0) {
        const int o = (int)(s & 63);
        const int n = min(64 - o, len);
        const u64 v = (mask[s >> 6] >> o) & (n == 64 ? ~0ull : ((1ull << n) - 1ull));
        if (v) return true;
        s += n;
        len -= n;
      }
    }
  }
  return false;
}

constexpr int RA_MAXLIST = 16;
struct ListSel {   // list i: mask which[i], extension ext[i]
  signed char which[RA_MAXLIST], ext[RA_MAXLIST];
};

// one block per list: an ordered compaction of the tile indices
__global__ __launch_bounds__(1024) void halo_active_tiles_kernel(const HaloTile* __restrict__ tiles, int ntiles,
                                                                 const u64* __restrict__ masks, long long stride,
                                                                 int* __restrict__ lists, int* __restrict__ counts,
                                                                 ListSel sel) {
  __shared__ int wcnt[16];
  __shared__ int base_s;
  const u64* mask = masks + (long long)sel.which[blockIdx.x] * stride;
  const int ext = sel.ext[blockIdx.x];
  int* list = lists + (long long)blockIdx.x * ntiles;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) base_s = 0;
  __syncthreads();
  for (int t0 = 0; t0 < ntiles; t0 += 1024) {
    const int t = t0 + threadIdx.x;
    const bool act = t < ntiles && ra_tile_active(tiles[t], mask, ext);
    const u64 bal = __ballot(act);
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int before = base_s;   // active tiles below this wave's first tile
    for (int w = 0; w < wave; ++w) before += wcnt[w];
    const int rank = before + __popcll(bal & ((1ull << lane) - 1ull));   // active tiles below t
    if (t < ntiles) {
      if (act) list[rank] = t;
      else list[ntiles - 1 - (t - rank)] = t;   // the inactive tiles fill the list from its end
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int s = base_s;
      for (int w = 0; w < 16; ++w) s += wcnt[w];
      base_s = s;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = base_s;
}

}  // namespace

// mask: (rows + 63) / 64 words, every one written.  Requires ld % 8 == 0 and 16-B aligned rows.
MXR_API int mxr_rows_nonzero(const void* dy, long long rows, int ld, void* mask, hipStream_t stream) {
  if (rows < 1 || ld < 8 || ld % 8 != 0 || ((uintptr_t)dy & 15)) return -1;
  const long long nw = (rows + 63) / 64;
  if (nw > 0x7fffffffLL) return -4;
  rows_nonzero_kernel<<<(unsigned)nw, 256, 0, stream>>>((const uint4*)dy, rows, ld / 8, (u64*)mask);
  return (int)hipGetLastError();
}

// mask: (rows + 63) / 64 words, every one written (tail bits clear).  state: int8 [rows * group], packed row m owns
// anchors m * group .. m * group + group - 1; a row is set when one of them has state == 1.
MXR_API int mxr_rows_positive(const void* state, long long rows, int group, void* mask, hipStream_t stream) {
  if (rows < 1 || group < 1) return -1;
  const long long nw = (rows + 63) / 64;
  if (nw > 0x7fffffffLL) return -4;
  rows_positive_kernel<<<(unsigned)((nw + 3) / 4), 256, 0, stream>>>((const int8_t*)state, rows, group, nw, (u64*)mask);
  return (int)hipGetLastError();
}

// out + (k - 1) * stride_words: the k-fold 3x3 dilation of `in` per image and level of g (k = 1 .. nd <= 8); masks of
// (g->M + 63) / 64 words over the packed output rows of g.
MXR_API int mxr_rows_dilate(const void* in, void* out, int nd, long long stride_words, const ConvGeom* g,
                            hipStream_t stream) {
  if (nd < 1 || nd > RA_MAXD || g->nlev < 1 || g->nlev > MXR_MAXLEV || g->M < 1) return -1;
  const long long nw = (g->M + 63) / 64;
  if (stride_words < nw || nw > 0x7fffffffLL) return -4;
  for (int l = 0; l < g->nlev; ++l)
    if (g->W[l] != g->Wo[l] || g->H[l] != g->Ho[l]) return -2;
  rows_dilate_kernel<<<(unsigned)((nw + 3) / 4), 256, 0, stream>>>((const u64*)in, (u64*)out, nd, stride_words, nw, *g);
  return (int)hipGetLastError();
}

// For each of the nmask row masks (masks + k * stride_words): lists + k * ntiles = the tile indices, the active
// ones first; counts[k] = how many are active.
// List i (lists + i * ntiles, counts[i]) is built from mask which[i] (0 .. nmask - 1) with the boxes extended by ext[i]
// (0 or 1) pixels; which / ext are HOST arrays of nlist <= 16 entries.
MXR_API int mxr_halo_active_tiles_ext(const void* tiles, int ntiles, const void* masks, long long stride_words,
                                      int nmask, int nlist, const int* which, const int* ext, int* lists, int* counts,
                                      hipStream_t stream) {
  if (ntiles < 1 || nmask < 1 || nlist < 1 || nlist > RA_MAXLIST) return -1;
  ListSel sel = {};
  for (int i = 0; i < nlist; ++i) {
    if (which[i] < 0 || which[i] >= nmask || (ext[i] != 0 && ext[i] != 1)) return -1;
    sel.which[i] = (signed char)which[i];
    sel.ext[i] = (signed char)ext[i];
  }
  halo_active_tiles_kernel<<<(unsigned)nlist, 1024, 0, stream>>>((const HaloTile*)tiles, ntiles, (const u64*)masks,
                                                                 stride_words, lists, counts, sel);
  return (int)hipGetLastError();
}

MXR_API int mxr_halo_active_tiles(const void* tiles, int ntiles, const void* masks, long long stride_words, int nmask,
                                  int* lists, int* counts, hipStream_t stream) {
  if (nmask < 1 || nmask > RA_MAXLIST) return -1;
  int which[RA_MAXLIST], ext[RA_MAXLIST];
  for (int i = 0; i < nmask; ++i) {
    which[i] = i;
    ext[i] = 1;
  }
  return mxr_halo_active_tiles_ext(tiles, ntiles, masks, stride_words, nmask, nmask, which, ext, lists, counts, stream);
}
