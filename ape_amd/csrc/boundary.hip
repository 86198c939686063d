// Boundary bands of instance masks on the device (ape_amd/evaluation.py, boundary_ap): Boundary IoU (Cheng et al., CVPR 2021) compares, for
// two masks, the band of width d along the inside of each contour: band = mask & ~erode(mask), the erosion by the (2d + 1)^2 square
// with everything outside the image counting as background.  The published package erodes every mask on the host (d iterations of a
// 3 x 3 erosion); on words of 64 pixels the same erosion is shifts and ANDs.  All arithmetic is integer: the result is exact.
//
// ROW-PACKED layout: pixel (y, x) is bit x % 64 of word y * wpr + x / 64, wpr = ceil(W / 64); the unused high bits of a row's last word
// are zero.  A row never shares a word with its neighbour, so a horizontal shift is a funnel shift inside one row and a vertical shift
// is a whole number of words; the zero bits behind column W - 1 are the "outside is 0" rule along x.  A row-packed [n, H * wpr] tensor
// is a valid operand of ape_hip_bitmask_pair_counts (maskiou.hip) as it is.
//
//   mask_pack_rows      : n byte masks [H, W] (non-zero = foreground, any base address) -> row-packed bits + area [n].  The lane form of
//                         mask_pack_bits: a lane owns 16 pixels of one row, four neighbouring lanes join into a word, and the pieces of
//                         all rows of all masks form ONE sequence that the waves share out, so a short row does not cost a wave.  A row
//                         starts at any byte address: a lane reads the aligned 16-byte vector its piece begins in, and takes the
//                         vector behind it from the next lane (one shuffle) whenever that lane happens to hold it.
//   bitmask_boundary    : band = m & ~erode(m), barea = popcount(band).  Separable.  Horizontal: the AND of 2d + 1 neighbouring bits,
//                         by doubling (a run of k ANDed with itself shifted by k is a run of 2k) on a 128-bit window of the row, so a
//                         run of up to 64 costs 6 steps; a longer run is the AND of runs of 64 at a stride of one word plus one that
//                         ends with it.  Vertical: a workgroup stages the horizontally eroded words of a tile of rows plus d halo rows
//                         on either side in LDS (rows outside the image are zero) and doubles again, now by whole rows, between two
//                         LDS buffers.  The tile is sized from the LDS the device reports (bd_plan).
//   bitmask_unpack_rows : row-packed bits -> byte masks of 0 / 1, written in aligned 16-byte pieces.
#include "common.h"
#include "../../include/ape_hip.h"

typedef unsigned long long bd_u64;

#define BD_THREADS 256

__device__ __forceinline__ uint32_t bd_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------------------ pack rows
#define PR_UNROLL 4                  // pieces (16 pixels) per lane and step: four independent 16-byte loads in flight

// bit k = (byte k of x != 0), k = 0..3
__device__ __forceinline__ uint32_t pr_nib(uint32_t x) {
  const uint32_t nz = ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u) >> 7;     // bit 8k = byte k non-zero
  return ((nz * 0x00204081u) >> 21) & 0xfu;                                              // bit 8k -> bit 21 + k; no two products meet
}

// the 16 bits of the aligned 16-byte vector number q (byte addresses 16 q .. 16 q + 15); bytes outside [lo, hi) read as 0 and are not loaded
__device__ __forceinline__ uint32_t pr_vector_bits(unsigned long long q, unsigned long long lo, unsigned long long hi) {
  const unsigned long long first = 16ull * q;
  if (first >= hi || first + 16 <= lo) return 0u;
  if (first >= lo && first + 16 <= hi) {
    const uint4 t = *reinterpret_cast<const uint4*>((uintptr_t)first);
    return pr_nib(t.x) | (pr_nib(t.y) << 4) | (pr_nib(t.z) << 8) | (pr_nib(t.w) << 12);
  }
  uint32_t b = 0;
  for (int k = 0; k < 16; ++k) {
    const unsigned long long p = first + k;
    if (p >= lo && p < hi && *reinterpret_cast<const uint8_t*>((uintptr_t)p) != 0) b |= 1u << k;
  }
  return b;
}

// piece g of the sequence = pixels 16 t .. 16 t + 15 of row g / ppr (rows of all masks counted through), t = g % ppr, ppr = 4 wpr.
// Wave v takes the pieces [v * chunk, (v + 1) * chunk), chunk a multiple of 64 * PR_UNROLL: its words are consecutive, and it changes
// from one mask to the next at most a few times.
__global__ __launch_bounds__(BD_THREADS) void mask_pack_rows_kernel(const uint8_t* __restrict__ masks, int H, int W, int wpr, long long pieces,
                                                                    long long chunk, bd_u64* __restrict__ bits, long long ldb,
                                                                    bd_u64* __restrict__ area, long long nbytes) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (BD_THREADS / 64) + (threadIdx.x >> 6);
  const long long g0 = wave * chunk;
  const long long g1 = g0 + chunk < pieces ? g0 + chunk : pieces;
  const int ppr = 4 * wpr;
  const unsigned long long lo = (unsigned long long)(uintptr_t)masks, hi = lo + (unsigned long long)nbytes;
  uint32_t count = 0;                // foreground of mask `cur` met by this lane and not yet added to area
  long long cur = -1;                // the same in every lane of the wave
  // this lane's piece: word-quarter t of row y of mask mi; the one 64-bit division of the kernel, every later step moves on by 64 pieces
  long long mi;
  int y, t;
  {
    const long long g = g0 + lane, rowflat = g / ppr;
    t = (int)(g - rowflat * ppr);
    mi = rowflat / H;
    y = (int)(rowflat - mi * H);
  }
  // the loop bound is the same for every lane of a wave: the shuffles below see whole waves
  for (long long base = g0; base < g1; base += 64 * PR_UNROLL) {
    uint32_t v[PR_UNROLL];
    unsigned long long q[PR_UNROLL];
    int s[PR_UNROLL], valid[PR_UNROLL], py[PR_UNROLL], pt[PR_UNROLL];
    long long pm[PR_UNROLL];
#pragma unroll
    for (int u = 0; u < PR_UNROLL; ++u) {
      const long long g = base + u * 64 + lane;
      pm[u] = mi;
      py[u] = y;
      pt[u] = t;
      const int x0 = 16 * t;
      const int left = g < g1 ? W - x0 : 0;                      // pixels of the piece that lie inside the row
      valid[u] = left < 0 ? 0 : (left > 16 ? 16 : left);
      const unsigned long long a = lo + ((unsigned long long)mi * (unsigned long long)H + (unsigned long long)y) * (unsigned long long)W
                                   + (unsigned long long)x0;
      q[u] = a >> 4;
      s[u] = (int)(a & 15);
      v[u] = valid[u] > 0 ? pr_vector_bits(q[u], lo, hi) : 0u;
      t += 64;                                                   // the piece 64 further on
      const int rows_on = t / ppr;
      t -= rows_on * ppr;
      y += rows_on;
      if (y >= H) {
        const int masks_on = y / H;
        mi += masks_on;
        y -= masks_on * H;
      }
    }
#pragma unroll
    for (int u = 0; u < PR_UNROLL; ++u) {
      // the piece ends in the first s bytes of the vector behind: the next lane's, if the next lane read it
      uint32_t nxt = __shfl_down(v[u], 1, 64);
      const unsigned long long nq = __shfl_down(q[u], 1, 64);
      const int nvalid = __shfl_down(valid[u], 1, 64);
      uint32_t piece = v[u] >> s[u];
      if (valid[u] > 16 - s[u]) {
        if (lane == 63 || nq != q[u] + 1 || nvalid == 0) nxt = pr_vector_bits(q[u] + 1, lo, hi);
        piece |= nxt << (16 - s[u]);
      }
      piece &= (1u << valid[u]) - 1u;
      // four lanes -> one word, held by the lane with lane % 4 == 0
      bd_u64 w = (bd_u64)piece << (16 * (lane & 3));
      w |= __shfl_xor(w, 1, 64);
      w |= __shfl_xor(w, 2, 64);
      const long long g = base + u * 64 + lane;
      const bool writer = (lane & 3) == 0 && g < g1;
      uint32_t pc = 0;
      if (writer) {
        bits[(size_t)pm[u] * ldb + (size_t)py[u] * wpr + (size_t)(pt[u] >> 2)] = w;
        pc = (uint32_t)__popcll(w);
      }
      // area: the wave keeps the count of one mask and adds it when the mask changes; a step that spans two masks adds per lane
      const long long m_first = __shfl(pm[u], 0, 64), m_last = __shfl(pm[u], 63, 64);
      if (m_first == m_last && m_first == cur) {
        count += pc;
      } else {
        const uint32_t total = bd_wave_sum(count);
        if (lane == 0 && total != 0u) atomicAdd(&area[cur], (bd_u64)total);
        count = 0;
        if (m_first == m_last) {
          cur = m_first;
          count = pc;
        } else {
          cur = -1;
          if (pc != 0u) atomicAdd(&area[pm[u]], (bd_u64)pc);
        }
      }
    }
  }
  const uint32_t total = bd_wave_sum(count);
  if (lane == 0 && total != 0u) atomicAdd(&area[cur], (bd_u64)total);
}

static size_t bd_wpr(int W) { return ((size_t)W + 63) / 64; }

extern "C" int ape_hip_mask_pack_rows(const uint8_t* masks, int n, int H, int W, uint64_t* bits, size_t ldb, int64_t* area, void* stream) {
  APE_CHECK_ARG(n >= 0, "ape_hip_mask_pack_rows: n = %d is negative", n);
  APE_CHECK_ARG(H >= 1 && W >= 1, "ape_hip_mask_pack_rows: H = %d, W = %d (both at least 1)", H, W);
  const size_t wpr = bd_wpr(W);
  APE_CHECK_ARG((unsigned long long)H * wpr < (1ull << 31), "ape_hip_mask_pack_rows: a mask of %d x %d is too large (H * ceil(W / 64) below 2^31)", H, W);
  APE_CHECK_ARG(ldb >= (size_t)H * wpr, "ape_hip_mask_pack_rows: ldb = %zu is less than the H * wpr = %zu words of a mask", ldb, (size_t)H * wpr);
  if (n == 0) return 0;
  APE_CHECK_ARG(masks && bits && area, "ape_hip_mask_pack_rows: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(area, 0, (size_t)n * sizeof(int64_t), st) != hipSuccess) {
    ape_set_error("ape_hip_mask_pack_rows: memset failed");
    return -2;
  }
  const long long pieces = (long long)n * H * (long long)(4 * wpr);
  const long long step = 64 * PR_UNROLL;
  // about 8 workgroups per CU; a wave's chunk is a whole number of steps
  const long long waves_want = (long long)8 * ape_cu_count() * (BD_THREADS / 64);
  long long chunk = ((pieces + waves_want - 1) / waves_want + step - 1) / step * step;
  if (chunk < step) chunk = step;
  const long long waves = (pieces + chunk - 1) / chunk;
  const long long blocks = (waves + BD_THREADS / 64 - 1) / (BD_THREADS / 64);
  APE_LAUNCH(mask_pack_rows_kernel, dim3((unsigned)blocks), dim3(BD_THREADS), 0, st, masks, H, W, (int)wpr, pieces, chunk, (bd_u64*)bits,
             (long long)ldb, (bd_u64*)area, (long long)((size_t)n * H * W));
  APE_CHECK_LAUNCH("ape_hip_mask_pack_rows");
  return 0;
}

// ------------------------------------------------------------------------------------------------------------ boundary
#define BD_TILE_WORDS 32                       // widest word tile: 2048 pixels
#define BD_LDS_SOFT ((size_t)48 * 1024)        // preferred LDS per workgroup: three workgroups share a CU's 160 KiB

// 128 bits of a row (wpr words, zero outside) from bit position p (any sign): lo = bits p .. p + 63, hi = bits p + 64 .. p + 127
__device__ __forceinline__ void bd_window(const bd_u64* __restrict__ row, int wpr, long long p, bd_u64& lo, bd_u64& hi) {
  const long long j = p >> 6;                                    // floor
  const int o = (int)(p & 63);
  const bd_u64 w0 = (j >= 0 && j < wpr) ? row[j] : 0ull;
  const bd_u64 w1 = (j + 1 >= 0 && j + 1 < wpr) ? row[j + 1] : 0ull;
  const bd_u64 w2 = (j + 2 >= 0 && j + 2 < wpr) ? row[j + 2] : 0ull;
  lo = o ? (w0 >> o) | (w1 << (64 - o)) : w0;
  hi = o ? (w1 >> o) | (w2 << (64 - o)) : w1;
}

// bit i of the result (i = 0..63) = AND of the row's bits p + i .. p + i + m - 1, 1 <= m <= 64.  Doubling on the 128-bit window: after
// the step with shift k the window holds runs of 2k wherever they end inside it; a run that starts in the low word ends by bit 126.
__device__ __forceinline__ bd_u64 bd_run(const bd_u64* __restrict__ row, int wpr, long long p, int m) {
  bd_u64 lo, hi;
  bd_window(row, wpr, p, lo, hi);
  int k = 1;
  while (2 * k <= m) {                                           // k <= 32
    lo &= (lo >> k) | (hi << (64 - k));
    hi &= hi >> k;
    k *= 2;
  }
  if (k < m) {                                                   // runs of k at i and at i + m - k cover a run of m
    const int s = m - k;
    lo &= (lo >> s) | (hi << (64 - s));
  }
  return lo;
}

// word w of the row eroded along x: bit i = AND of the row's bits 64 w + i - d .. 64 w + i + d
__device__ __forceinline__ bd_u64 bd_erode_row(const bd_u64* __restrict__ row, int wpr, int w, int d) {
  if (row[w] == 0ull) return 0ull;
  const long long p = 64ll * w - d;
  const long long L = 2ll * d + 1;
  if (L <= 64) return bd_run(row, wpr, p, (int)L);
  bd_u64 e = bd_run(row, wpr, p + L - 64, 64);
  for (long long off = 0; off + 64 <= L && e != 0ull; off += 64) e &= bd_run(row, wpr, p + off, 64);
  return e;
}

// workgroup = (mask, row tile, word tile): TR rows x TW words of output from R = TR + 2 d staged rows.  LDS: two buffers of R * TW words.
__global__ __launch_bounds__(BD_THREADS) void bitmask_boundary_kernel(const bd_u64* __restrict__ bits, long long ldb, int H, int wpr, int d, int TR,
                                                                      int TW, int tiles_r, int tiles_w, bd_u64* __restrict__ bbits,
                                                                      long long ldo, bd_u64* __restrict__ barea) {
  extern __shared__ __attribute__((aligned(16))) bd_u64 bd_lds[];
  const int tid = threadIdx.x;
  const int R = TR + 2 * d;
  bd_u64* A = bd_lds;
  bd_u64* B = bd_lds + (size_t)R * TW;
  unsigned blk = blockIdx.x;
  const int c0 = (int)(blk % (unsigned)tiles_w) * TW;
  blk /= (unsigned)tiles_w;
  const int r0 = (int)(blk % (unsigned)tiles_r) * TR;
  const int mi = (int)(blk / (unsigned)tiles_r);
  const bd_u64* __restrict__ m = bits + (size_t)mi * ldb;

  // staged row r is image row r0 - d + r; rows outside the image and words behind the row are zero
  for (int idx = tid; idx < R * TW; idx += BD_THREADS) {
    const int r = idx / TW, c = idx - r * TW;
    const int y = r0 - d + r, w = c0 + c;
    A[idx] = (y >= 0 && y < H && w < wpr) ? bd_erode_row(m + (size_t)y * wpr, wpr, w, d) : 0ull;
  }
  __syncthreads();
  // A[r] = AND of staged rows r .. r + k - 1, for r <= R - k; every loop bound below is the same for the whole workgroup
  const int L = 2 * d + 1;
  int k = 1;
  while (2 * k <= L) {
    const int cnt = (R - 2 * k + 1) * TW;
    for (int idx = tid; idx < cnt; idx += BD_THREADS) B[idx] = A[idx] & A[idx + k * TW];
    __syncthreads();
    bd_u64* t = A;
    A = B;
    B = t;
    k *= 2;
  }
  const int s = L - k;                                           // L is odd, k a power of two below it: 1 <= s < k
  uint32_t count = 0;
  for (int idx = tid; idx < TR * TW; idx += BD_THREADS) {
    const int t = idx / TW, c = idx - t * TW;
    const int y = r0 + t, w = c0 + c;
    if (y < H && w < wpr) {
      const bd_u64 eroded = A[idx] & A[idx + s * TW];            // output row t: staged rows t .. t + 2 d
      const bd_u64 band = m[(size_t)y * wpr + w] & ~eroded;
      bbits[(size_t)mi * ldo + (size_t)y * wpr + w] = band;
      count += (uint32_t)__popcll(band);
    }
  }
  count = bd_wave_sum(count);
  if ((tid & 63) == 0 && count != 0u) atomicAdd(&barea[mi], (bd_u64)count);
}

// the erosion is empty (2 d + 1 exceeds H or W): the band is the mask.  grid = n * per_mask workgroups of BD_THREADS words
__global__ __launch_bounds__(BD_THREADS) void bitmask_copy_count_kernel(const bd_u64* __restrict__ bits, long long ldb, long long words, unsigned per_mask,
                                                                        bd_u64* __restrict__ bbits, long long ldo, bd_u64* __restrict__ barea) {
  const unsigned mi = blockIdx.x / per_mask;
  const long long i = (long long)(blockIdx.x % per_mask) * BD_THREADS + threadIdx.x;
  uint32_t count = 0;
  if (i < words) {
    const bd_u64 v = bits[(size_t)mi * ldb + i];
    bbits[(size_t)mi * ldo + i] = v;
    count = (uint32_t)__popcll(v);
  }
  count = bd_wave_sum(count);
  if ((threadIdx.x & 63) == 0 && count != 0u) atomicAdd(&barea[mi], (bd_u64)count);
}

// bytes of LDS one workgroup may allocate on the current device (0 if there is no device to ask)
static size_t bd_lds_limit() {
  static size_t lim[APE_MAX_DEVICES] = {};
  static bool known[APE_MAX_DEVICES] = {};
  const int d = ape_current_device();
  if (!known[d]) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, d) != hipSuccess || v < 0) return 0;
    lim[d] = (size_t)v;
    known[d] = true;
  }
  return lim[d];
}

// Tile of the boundary kernel for LDS limit `limit`: TR output rows (wanted: max(64, 4 d), so the 2 d halo rows are at most a third of
// the staged ones) by TW words, two buffers of (TR + 2 d) * TW words.  First a tile of at least 2 d + 16 rows inside the preferred
// size, halving the word tile until it fits; then any tile inside it; then any tile inside the whole limit.
static bool bd_plan(int H, size_t wpr, int d, size_t limit, int* TR, int* TW, size_t* bytes) {
  long long want = 4ll * d > 64 ? 4ll * d : 64;
  if (want > H) want = H;
  const size_t soft = limit < BD_LDS_SOFT ? limit : BD_LDS_SOFT;
  for (int pass = 0; pass < 3; ++pass) {
    const size_t budget = pass < 2 ? soft : limit;
    long long least = 1;
    if (pass == 0) least = want < 2ll * d + 16 ? want : 2ll * d + 16;
    for (int tw = wpr < BD_TILE_WORDS ? (int)wpr : BD_TILE_WORDS;; tw = (tw + 1) / 2) {
      long long rows = (long long)(budget / ((size_t)16 * tw)) - 2ll * d;
      if (rows > want) rows = want;
      if (rows >= least) {
        *TR = (int)rows;
        *TW = tw;
        *bytes = (size_t)(rows + 2ll * d) * tw * 16;
        return true;
      }
      if (tw == 1) break;
    }
  }
  return false;
}

extern "C" int ape_hip_bitmask_boundary(const uint64_t* bits, int n, int H, int W, int d, size_t ldb, uint64_t* bbits, size_t ldo,
                                        int64_t* barea, void* stream) {
  APE_CHECK_ARG(n >= 0, "ape_hip_bitmask_boundary: n = %d is negative", n);
  APE_CHECK_ARG(H >= 1 && W >= 1, "ape_hip_bitmask_boundary: H = %d, W = %d (both at least 1)", H, W);
  APE_CHECK_ARG(d >= 1, "ape_hip_bitmask_boundary: d = %d (the band is at least 1 pixel wide)", d);
  const size_t wpr = bd_wpr(W);
  const unsigned long long words = (unsigned long long)H * wpr;
  APE_CHECK_ARG(words < (1ull << 31), "ape_hip_bitmask_boundary: a mask of %d x %d is too large (H * ceil(W / 64) below 2^31)", H, W);
  APE_CHECK_ARG(ldb >= words && ldo >= words, "ape_hip_bitmask_boundary: ldb = %zu / ldo = %zu is less than the H * wpr = %llu words of a mask",
                ldb, ldo, words);
  if (n == 0) return 0;
  APE_CHECK_ARG(bits && bbits && barea, "ape_hip_bitmask_boundary: null pointer");
  APE_CHECK_ARG((const void*)bits != (const void*)bbits, "ape_hip_bitmask_boundary: bits and bbits are the same buffer (not in place)");
  hipStream_t st = (hipStream_t)stream;
  const bool empty = 2ll * d + 1 > H || 2ll * d + 1 > W;         // no pixel has its whole window inside the image
  int TR = 0, TW = 0;
  size_t lds = 0;
  unsigned long long blocks;
  unsigned per_mask = 0;
  int tiles_r = 0, tiles_w = 0;
  if (empty) {
    per_mask = (unsigned)((words + BD_THREADS - 1) / BD_THREADS);
    blocks = (unsigned long long)n * per_mask;
  } else {
    const size_t limit = bd_lds_limit();
    if (limit == 0) {
      ape_set_error("ape_hip_bitmask_boundary: no HIP device to ask for its LDS limit");
      return -2;
    }
    APE_CHECK_ARG(bd_plan(H, wpr, d, limit, &TR, &TW, &lds),
                  "ape_hip_bitmask_boundary: d = %d needs %lld bytes of LDS for one output row, the device allows %zu", d, (2ll * d + 1) * 16, limit);
    tiles_r = (H + TR - 1) / TR;
    tiles_w = (int)((wpr + TW - 1) / TW);
    blocks = (unsigned long long)n * tiles_r * tiles_w;
  }
  APE_CHECK_ARG(blocks <= 0x7fffffffULL, "ape_hip_bitmask_boundary: %d masks of %d x %d are too many for one call", n, H, W);
  if (hipMemsetAsync(barea, 0, (size_t)n * sizeof(int64_t), st) != hipSuccess) {
    ape_set_error("ape_hip_bitmask_boundary: memset failed");
    return -2;
  }
  if (empty) {
    APE_LAUNCH(bitmask_copy_count_kernel, dim3((unsigned)blocks), dim3(BD_THREADS), 0, st, (const bd_u64*)bits, (long long)ldb, (long long)words,
               per_mask, (bd_u64*)bbits, (long long)ldo, (bd_u64*)barea);
  } else {
    if (lds > 64 * 1024) {                       // above 64 KiB the allocation has to be allowed per function (and device)
      static ApeOncePerDevice attr_done;
      if (attr_done.first()) {
        (void)hipFuncSetAttribute((const void*)bitmask_boundary_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bd_lds_limit());
      }
    }
    APE_LAUNCH(bitmask_boundary_kernel, dim3((unsigned)blocks), dim3(BD_THREADS), lds, st, (const bd_u64*)bits, (long long)ldb, H, (int)wpr, d, TR, TW,
               tiles_r, tiles_w, (bd_u64*)bbits, (long long)ldo, (bd_u64*)barea);
  }
  APE_CHECK_LAUNCH("ape_hip_bitmask_boundary");
  return 0;
}

extern "C" int ape_hip_bitmask_boundary_tile(int H, int W, int d, size_t lds_limit, int* tile_rows, int* tile_words) {
  APE_CHECK_ARG(H >= 1 && W >= 1 && d >= 1, "ape_hip_bitmask_boundary_tile: H = %d, W = %d, d = %d (all at least 1)", H, W, d);
  APE_CHECK_ARG(tile_rows && tile_words, "ape_hip_bitmask_boundary_tile: null pointer");
  if (lds_limit == 0) lds_limit = bd_lds_limit();
  if (lds_limit == 0) {
    ape_set_error("ape_hip_bitmask_boundary_tile: no HIP device to ask for its LDS limit");
    return -2;
  }
  size_t bytes = 0;
  if (2ll * d + 1 > H || 2ll * d + 1 > W) {      // the band is the mask: no tile
    *tile_rows = *tile_words = 0;
    return 0;
  }
  if (!bd_plan(H, bd_wpr(W), d, lds_limit, tile_rows, tile_words, &bytes)) return -1;
  return (int)bytes;
}

// ------------------------------------------------------------------------------------------------------------ unpack rows
// one thread = one aligned 16-byte piece of the output: bytes 16 g - s .. 16 g - s + 15 of the n * H * W (s = out's address % 16)
__global__ __launch_bounds__(BD_THREADS) void bitmask_unpack_rows_kernel(const bd_u64* __restrict__ bits, long long ldb, int H, int W, int wpr,
                                                                         size_t total, int s, uint8_t* __restrict__ out) {
  const size_t g = (size_t)blockIdx.x * BD_THREADS + threadIdx.x;
  const long long first = (long long)(16 * g) - s;
  if (first >= (long long)total) return;
  const size_t f0 = first < 0 ? 0 : (size_t)first;
  size_t f1 = (size_t)(first + 16);
  if (f1 > total) f1 = total;
  const size_t rowflat = f0 / (size_t)W;
  int x = (int)(f0 - rowflat * (size_t)W);
  size_t mi = rowflat / (size_t)H;
  int y = (int)(rowflat - mi * (size_t)H);
  uint8_t v[16] = {};
  for (size_t f = f0; f < f1; ++f) {
    v[f - f0] = (uint8_t)((bits[mi * (size_t)ldb + (size_t)y * wpr + (size_t)(x >> 6)] >> (x & 63)) & 1ull);
    if (++x == W) {
      x = 0;
      if (++y == H) {
        y = 0;
        ++mi;
      }
    }
  }
  if (first >= 0 && f1 - f0 == 16) {
    uint4 pk;
    pk.x = v[0] | (v[1] << 8) | (v[2] << 16) | ((uint32_t)v[3] << 24);
    pk.y = v[4] | (v[5] << 8) | (v[6] << 16) | ((uint32_t)v[7] << 24);
    pk.z = v[8] | (v[9] << 8) | (v[10] << 16) | ((uint32_t)v[11] << 24);
    pk.w = v[12] | (v[13] << 8) | (v[14] << 16) | ((uint32_t)v[15] << 24);
    *reinterpret_cast<uint4*>(out + f0) = pk;
  } else {
    for (size_t f = f0; f < f1; ++f) out[f] = v[f - f0];
  }
}

extern "C" int ape_hip_bitmask_unpack_rows(const uint64_t* bits, int n, int H, int W, size_t ldb, uint8_t* masks, void* stream) {
  APE_CHECK_ARG(n >= 0, "ape_hip_bitmask_unpack_rows: n = %d is negative", n);
  APE_CHECK_ARG(H >= 1 && W >= 1, "ape_hip_bitmask_unpack_rows: H = %d, W = %d (both at least 1)", H, W);
  const size_t wpr = bd_wpr(W);
  APE_CHECK_ARG((unsigned long long)H * wpr < (1ull << 31), "ape_hip_bitmask_unpack_rows: a mask of %d x %d is too large (H * ceil(W / 64) below 2^31)", H, W);
  APE_CHECK_ARG(ldb >= (size_t)H * wpr, "ape_hip_bitmask_unpack_rows: ldb = %zu is less than the H * wpr = %zu words of a mask", ldb, (size_t)H * wpr);
  if (n == 0) return 0;
  APE_CHECK_ARG(bits && masks, "ape_hip_bitmask_unpack_rows: null pointer");
  const size_t total = (size_t)n * H * W;
  const int s = (int)((uintptr_t)masks & 15);
  const size_t pieces = (total + s + 15) / 16, blocks = (pieces + BD_THREADS - 1) / BD_THREADS;
  APE_CHECK_ARG(blocks <= 0x7fffffffULL, "ape_hip_bitmask_unpack_rows: %zu output bytes are too many for one call", total);
  APE_LAUNCH(bitmask_unpack_rows_kernel, dim3((unsigned)blocks), dim3(BD_THREADS), 0, (hipStream_t)stream, (const bd_u64*)bits, (long long)ldb, H, W,
             (int)wpr, total, s, masks);
  APE_CHECK_LAUNCH("ape_hip_bitmask_unpack_rows");
  return 0;
}
