// Instance-mask scoring on the device (ape_amd/evaluation.py, mask_ap): the IoU matrix of two sets of [H, W] byte masks, and the way
// back from COCO run lengths to masks.  The host formulation is a.flatten(1).float() @ b.flatten(1).float().T after a device-to-host
// copy of every mask; here the masks are read once, packed to bits, and the n x m contraction runs on words an eighth of the size
// with popcount(a & b).  All arithmetic is integer: the result is exact and does not depend on the order of the adds.
//
//   mask_pack_bits      : n byte masks (non-zero = foreground) -> bits [n, ldb] 64-bit words (pixel p = bit p % 64 of word p / 64, the
//                         unused high bits of the last word zero) + area [n].  One lane takes 16 consecutive bytes with ONE aligned
//                         16-byte load and builds its 16 bits with integer arithmetic; four neighbouring lanes join theirs into a word.
//                         A base pointer that is not a multiple of 16 keeps the aligned loads: the 16 pixels of a lane then lie in two
//                         neighbouring vectors, the second of which is the next lane's (one shuffle); only the vectors that overlap
//                         the mask's first or last bytes are read byte by byte, so nothing outside the mask is touched.
//   mask_paired_counts  : for n (a_i, b_i) pairs of byte masks the three integers |a_i & b_i|, |a_i|, |b_i| -- what the referring-expression
//                         scores need -- in ONE pass over the bytes: the pack's loads and marks for both sides (each with its own
//                         misalignment), popcounts in registers, three atomics per wave; no bits are written.
//   bitmask_pair_counts : inter[i][j] = sum_w popcount(a[i][w] & b[j][w]), a binary GEMM.  A workgroup stages 64 rows of a and 64 rows of
//                         b over 32 words in LDS, a thread owns 4 x 4 pairs; the word axis is split over workgroups until the grid
//                         fills the device, and the partial sums then meet in 64-bit integer atomics on a matrix that the call zeroes
//                         with a memset node of the same stream.
//   rle_decode          : inclusive prefix sums of the runs (clipped to H * W), then for every output byte a binary search for its
//                         column-major position x * H + y: the parity of the run it falls into is its value.  Output is written
//                         row-major in aligned 16-byte pieces.
//   rle_from_string     : HOST, cocoapi maskApi.c rleFrString restated: the inverse of ape_hip_rle_to_string.
#include "common.h"
#include "../../include/ape_hip.h"

typedef unsigned long long mi_u64;

// ------------------------------------------------------------------------------------------------------------ pack
#define MP_THREADS 256
#define MP_UNROLL 4                  // pieces (16 pixels) per lane and step: four independent 16-byte loads in flight

// bit k = (byte k of x != 0), k = 0..3
__device__ __forceinline__ uint32_t mp_nib(uint32_t x) {
  const uint32_t nz = ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u) >> 7;     // bit 8k = byte k non-zero
  return ((nz * 0x00204081u) >> 21) & 0xfu;                                              // bit 8k -> bit 21 + k; no two products meet
}

// the 16 bits of aligned vector v of one mask: the vector holds pixels 16 v - s .. 16 v - s + 15 (s = the mask's byte address % 16);
// pixels outside [0, npix) read as 0 and are not loaded
__device__ __forceinline__ uint32_t mp_vector_bits(const uint8_t* __restrict__ m, long long v, int s, long long npix) {
  const long long first = 16 * v - s;
  if (first >= npix || first + 16 <= 0) return 0u;
  if (first >= 0 && first + 16 <= npix) {
    const uint4 t = *reinterpret_cast<const uint4*>(m + first);
    return mp_nib(t.x) | (mp_nib(t.y) << 4) | (mp_nib(t.z) << 8) | (mp_nib(t.w) << 12);
  }
  uint32_t b = 0;
  for (int k = 0; k < 16; ++k) {
    const long long p = first + k;
    if (p >= 0 && p < npix && m[p] != 0) b |= 1u << k;
  }
  return b;
}

// grid (x, n): the workgroups of row y walk the pieces of mask y, MP_UNROLL * 64 pieces (4096 pixels, 64 words) per wave and step
__global__ __launch_bounds__(MP_THREADS) void mask_pack_bits_kernel(const uint8_t* __restrict__ masks, long long npix, long long stride,
                                                                    mi_u64* __restrict__ bits, long long ldb, mi_u64* __restrict__ area) {
  const int mi = blockIdx.y;
  const uint8_t* __restrict__ m = masks + (size_t)mi * stride;
  mi_u64* __restrict__ out = bits + (size_t)mi * ldb;
  const int s = (int)((uintptr_t)m & 15);
  const long long words = (npix + 63) / 64, pieces = words * 4;
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (MP_THREADS / 64) + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * (MP_THREADS / 64);
  uint32_t count = 0;
  // the loop bound is the same for every lane of a wave: the shuffles below see whole waves
  for (long long base = wave * (64 * MP_UNROLL); base < pieces; base += nwaves * (64 * MP_UNROLL)) {
    uint32_t b[MP_UNROLL];
#pragma unroll
    for (int u = 0; u < MP_UNROLL; ++u) b[u] = mp_vector_bits(m, base + u * 64 + lane, s, npix);
#pragma unroll
    for (int u = 0; u < MP_UNROLL; ++u) {
      const long long t = base + u * 64 + lane;                 // piece = pixels 16 t .. 16 t + 15
      uint32_t piece = b[u];
      if (s != 0) {                                             // uniform: the piece ends in the first s bytes of the next vector
        uint32_t nxt = __shfl_down(b[u], 1, 64);
        // lane 63's neighbour is lane 0 of the next unrolled step, or a vector nobody has loaded yet
        uint32_t wrap = 0;
        if (u + 1 < MP_UNROLL) wrap = __shfl(b[(u + 1) % MP_UNROLL], 0, 64);
        else if (lane == 63) wrap = mp_vector_bits(m, t + 1, s, npix);
        if (lane == 63) nxt = wrap;
        piece = ((piece >> s) | (nxt << (16 - s))) & 0xffffu;
      }
      // four lanes -> one word, held by the lane with lane % 4 == 0
      mi_u64 w = (mi_u64)piece << (16 * (lane & 3));
      w |= __shfl_xor(w, 1, 64);
      w |= __shfl_xor(w, 2, 64);
      const long long wi = t >> 2;
      if ((lane & 3) == 0 && wi < words) {
        out[wi] = w;
        count += (uint32_t)__popcll(w);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
  if (lane == 0 && count != 0u) atomicAdd(&area[mi], (mi_u64)count);
}

extern "C" int ape_hip_mask_pack_bits(const uint8_t* masks, int n, size_t npix, size_t stride, uint64_t* bits, size_t ldb, int64_t* area,
                                      void* stream) {
  APE_CHECK_ARG(n >= 0, "ape_hip_mask_pack_bits: n = %d is negative", n);
  if (n == 0) return 0;
  APE_CHECK_ARG(masks && bits && area, "ape_hip_mask_pack_bits: null pointer");
  APE_CHECK_ARG(n <= 65535, "ape_hip_mask_pack_bits: n = %d masks (at most 65535 per call)", n);
  APE_CHECK_ARG(npix < ((size_t)1 << 32), "ape_hip_mask_pack_bits: a mask of %zu pixels is too large (below 2^32)", npix);
  const size_t words = (npix + 63) / 64;
  APE_CHECK_ARG(ldb >= words, "ape_hip_mask_pack_bits: ldb = %zu is less than the %zu words of a mask", ldb, words);
  APE_CHECK_ARG(stride >= npix || n == 1, "ape_hip_mask_pack_bits: stride %zu is less than the %zu pixels of a mask", stride, npix);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(area, 0, (size_t)n * sizeof(int64_t), st) != hipSuccess) {
    ape_set_error("ape_hip_mask_pack_bits: memset failed");
    return -2;
  }
  if (words == 0) return 0;
  const size_t per_wg = (size_t)(MP_THREADS / 64) * 64 * MP_UNROLL / 4;             // words per workgroup and step
  size_t gx = (words + per_wg - 1) / per_wg;
  const size_t want = ((size_t)8 * ape_cu_count() + n - 1) / n;                      // about 8 workgroups per CU over all masks
  if (gx > want) gx = want;
  if (gx < 1) gx = 1;
  APE_LAUNCH(mask_pack_bits_kernel, dim3((unsigned)gx, (unsigned)n), dim3(MP_THREADS), 0, st, masks, (long long)npix, (long long)stride,
             (mi_u64*)bits, (long long)ldb, (mi_u64*)area);
  APE_CHECK_LAUNCH("ape_hip_mask_pack_bits");
  return 0;
}

// ------------------------------------------------------------------------------------------------------------ paired counts
// the marks of MP_UNROLL * 64 consecutive aligned vectors (b[u] of lane l = vector v0 + 64 u + l) -> pieces in pixel order, for a mask
// whose byte address is s != 0 past a multiple of 16: piece t = the high 16 - s marks of vector t and the low s marks of vector t + 1, the
// next lane's; lane 63 takes lane 0 of the next unrolled step, and behind the last step `own`, which it has loaded itself.  Called by
// whole waves.
__device__ __forceinline__ void mq_pixel_order(uint32_t (&b)[MP_UNROLL], uint32_t own, int s, int lane) {
#pragma unroll
  for (int u = 0; u < MP_UNROLL; ++u) {
    uint32_t nxt = __shfl_down(b[u], 1, 64);
    const uint32_t wrap = u + 1 < MP_UNROLL ? __shfl(b[(u + 1) % MP_UNROLL], 0, 64) : own;     // b[u + 1] is still in vector order
    if (lane == 63) nxt = wrap;
    b[u] = ((b[u] >> s) | (nxt << (16 - s))) & 0xffffu;
  }
}

__device__ __forceinline__ uint32_t mq_marks(const uint4& t) {
  return mp_nib(t.x) | (mp_nib(t.y) << 4) | (mp_nib(t.z) << 8) | (mp_nib(t.w) << 12);
}

// grid (x, n): the waves of row y walk the pieces (16 pixels) of pair y, MP_UNROLL * 64 pieces (4096 pixels) per wave and step, and add
// (|a & b|, |a|, |b|) to out[y][0..2].  a and b are read once, with aligned 16-byte loads whatever their two byte addresses are; nothing
// is stored in between.
__global__ __launch_bounds__(MP_THREADS) void mask_paired_counts_kernel(const uint8_t* __restrict__ a, long long stride_a,
                                                                        const uint8_t* __restrict__ b, long long stride_b, long long npix,
                                                                        mi_u64* __restrict__ out) {
  const int mi = blockIdx.y;
  const uint8_t* __restrict__ ma = a + (size_t)mi * stride_a;
  const uint8_t* __restrict__ mb = b + (size_t)mi * stride_b;
  const int sa = (int)((uintptr_t)ma & 15), sb = (int)((uintptr_t)mb & 15);
  const long long pieces = (npix + 15) / 16;
  const int lane = threadIdx.x & 63;
  // wave w of workgroup x is wave w * gridDim.x + x of the row: with fewer steps than waves, every workgroup's first wave has one
  const long long wave = (long long)(threadIdx.x >> 6) * gridDim.x + blockIdx.x, nwaves = (long long)gridDim.x * (MP_THREADS / 64);
  uint32_t inter = 0, area_a = 0, area_b = 0;                     // a wave counts fewer than 2^32 pixels: npix is below that
  // the loop bound is the same for every lane of a wave: the shuffles of mq_pixel_order see whole waves
  for (long long base = wave * (64 * MP_UNROLL); base < pieces; base += nwaves * (64 * MP_UNROLL)) {
    uint32_t pa[MP_UNROLL], pb[MP_UNROLL];
    uint32_t own_a = 0, own_b = 0;                                // the vector behind the step's last one: nobody else has loaded it
    // wave-uniform: every vector of the step, and the one behind it, lies inside both masks (bytes 16 base - s .. 16 (base + 64 U + 1) - s)
    const bool inner = (base > 0 || (sa | sb) == 0) && 16 * (base + 64 * MP_UNROLL + 1) <= npix;
    if (inner) {                                                  // 2 * MP_UNROLL loads in flight, nothing decided per lane but lane 63's extra
      const uint8_t* __restrict__ qa = ma + 16 * (base + lane) - sa;
      const uint8_t* __restrict__ qb = mb + 16 * (base + lane) - sb;
      uint4 va[MP_UNROLL], vb[MP_UNROLL], wa = make_uint4(0, 0, 0, 0), wb = make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int u = 0; u < MP_UNROLL; ++u) va[u] = *reinterpret_cast<const uint4*>(qa + u * 1024);
#pragma unroll
      for (int u = 0; u < MP_UNROLL; ++u) vb[u] = *reinterpret_cast<const uint4*>(qb + u * 1024);
      if (lane == 63) {
        if (sa != 0) wa = *reinterpret_cast<const uint4*>(qa + (MP_UNROLL - 1) * 1024 + 16);
        if (sb != 0) wb = *reinterpret_cast<const uint4*>(qb + (MP_UNROLL - 1) * 1024 + 16);
      }
#pragma unroll
      for (int u = 0; u < MP_UNROLL; ++u) {
        pa[u] = mq_marks(va[u]);
        pb[u] = mq_marks(vb[u]);
      }
      own_a = mq_marks(wa);
      own_b = mq_marks(wb);
    } else {                                                      // a step at either end of the masks: every vector checks its bytes
#pragma unroll
      for (int u = 0; u < MP_UNROLL; ++u) pa[u] = mp_vector_bits(ma, base + u * 64 + lane, sa, npix);
#pragma unroll
      for (int u = 0; u < MP_UNROLL; ++u) pb[u] = mp_vector_bits(mb, base + u * 64 + lane, sb, npix);
      if (lane == 63) {
        if (sa != 0) own_a = mp_vector_bits(ma, base + 64 * MP_UNROLL, sa, npix);
        if (sb != 0) own_b = mp_vector_bits(mb, base + 64 * MP_UNROLL, sb, npix);
      }
    }
    if (sa != 0) mq_pixel_order(pa, own_a, sa, lane);             // uniform over the workgroup
    if (sb != 0) mq_pixel_order(pb, own_b, sb, lane);
#pragma unroll
    for (int u = 0; u < MP_UNROLL; ++u) {
      inter += (uint32_t)__popc(pa[u] & pb[u]);
      area_a += (uint32_t)__popc(pa[u]);
      area_b += (uint32_t)__popc(pb[u]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    inter += __shfl_xor(inter, o, 64);
    area_a += __shfl_xor(area_a, o, 64);
    area_b += __shfl_xor(area_b, o, 64);
  }
  const uint32_t mine = lane == 0 ? inter : lane == 1 ? area_a : area_b;     // lanes 0..2 carry one sum each
  if (lane < 3 && mine != 0u) atomicAdd(&out[(size_t)mi * 3 + lane], (mi_u64)mine);
}

extern "C" int ape_hip_mask_paired_counts(const uint8_t* a, size_t stride_a, const uint8_t* b, size_t stride_b, int n, size_t npix,
                                          int64_t* out, void* stream) {
  APE_CHECK_ARG(n >= 0, "ape_hip_mask_paired_counts: n = %d is negative", n);
  if (n == 0) return 0;
  APE_CHECK_ARG(out && (npix == 0 || (a && b)), "ape_hip_mask_paired_counts: null pointer");
  APE_CHECK_ARG(n <= 65535, "ape_hip_mask_paired_counts: n = %d pairs (at most 65535 per call)", n);
  APE_CHECK_ARG(npix < ((size_t)1 << 32), "ape_hip_mask_paired_counts: a mask of %zu pixels is too large (below 2^32)", npix);
  APE_CHECK_ARG((stride_a >= npix && stride_b >= npix) || n == 1,
                "ape_hip_mask_paired_counts: stride %zu / %zu is less than the %zu pixels of a mask", stride_a, stride_b, npix);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(out, 0, (size_t)n * 3 * sizeof(int64_t), st) != hipSuccess) {
    ape_set_error("ape_hip_mask_paired_counts: memset failed");
    return -2;
  }
  if (npix == 0) return 0;
  // a workgroup per wave step while that stays below about 8 workgroups per CU over all pairs (one pair of 1024^2 is 256 steps: every CU
  // reads a part; the waves of a workgroup that find no step leave at once), then several steps per wave
  const size_t steps = ((npix + 15) / 16 + 64 * MP_UNROLL - 1) / (64 * MP_UNROLL);
  size_t gx = steps;
  const size_t want = ((size_t)8 * ape_cu_count() + n - 1) / n;
  if (gx > want) gx = want;
  if (gx < 1) gx = 1;
  APE_LAUNCH(mask_paired_counts_kernel, dim3((unsigned)gx, (unsigned)n), dim3(MP_THREADS), 0, st, a, (long long)stride_a, b, (long long)stride_b,
             (long long)npix, (mi_u64*)out);
  APE_CHECK_LAUNCH("ape_hip_mask_paired_counts");
  return 0;
}

// ------------------------------------------------------------------------------------------------------------ pair counts
#define PC_TILE 64                   // rows of a and rows of b per workgroup
#define PC_KW 32                     // words per staging step
#define PC_LD (PC_KW + 2)            // LDS row stride in words: 272 bytes, so the 16 rows one 16-byte read meets lie on 16 x 4 different banks
#define PC_THREADS 256               // 16 x 16 threads, 4 x 4 pairs each
#define PC_MAX_SPAN (1ll << 25)      // words per workgroup: 2^31 bits, a pair's 32-bit partial count cannot overflow

typedef mi_u64 mi_u64x2 __attribute__((ext_vector_type(2)));

// grid (tiles of a * tiles of b, splits): workgroup (t, z) counts words [z * span, min(words, (z + 1) * span)) of its 64 x 64 tile
__global__ __launch_bounds__(PC_THREADS) void bitmask_pair_counts_kernel(const mi_u64* __restrict__ a, int n, long long lda,
                                                                         const mi_u64* __restrict__ b, int m, long long ldb, long long words,
                                                                         long long span, int tiles_j, mi_u64* __restrict__ inter,
                                                                         long long ldi, int atomic) {
  __shared__ __attribute__((aligned(16))) mi_u64 sa[PC_TILE * PC_LD];
  __shared__ __attribute__((aligned(16))) mi_u64 sb[PC_TILE * PC_LD];
  const int tid = threadIdx.x;
  const int i0 = (blockIdx.x / tiles_j) * PC_TILE, j0 = (blockIdx.x % tiles_j) * PC_TILE;
  const long long w0 = (long long)blockIdx.y * span;
  const long long w1 = w0 + span < words ? w0 + span : words;
  const int ti = tid & 15, tj = tid >> 4;                         // a wave: 16 rows of a, 4 rows of b
  const int lr = tid >> 5, lw = tid & 31;                         // staging: thread -> (row lr + 8 r, word lw)
  uint32_t acc[4][4] = {};
  for (long long k0 = w0; k0 < w1; k0 += PC_KW) {
    const bool kin = k0 + lw < w1;
#pragma unroll
    for (int r = 0; r < PC_TILE / 8; ++r) {
      const int row = lr + 8 * r;
      sa[row * PC_LD + lw] = (kin && i0 + row < n) ? a[(size_t)(i0 + row) * lda + k0 + lw] : 0ull;
      sb[row * PC_LD + lw] = (kin && j0 + row < m) ? b[(size_t)(j0 + row) * ldb + k0 + lw] : 0ull;
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < PC_KW; k += 2) {
      mi_u64x2 va[4], vb[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        va[r] = *reinterpret_cast<const mi_u64x2*>(&sa[(ti + 16 * r) * PC_LD + k]);
        vb[r] = *reinterpret_cast<const mi_u64x2*>(&sb[(tj + 16 * r) * PC_LD + k]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] += (uint32_t)__popcll(va[r][0] & vb[c][0]) + (uint32_t)__popcll(va[r][1] & vb[c][1]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + ti + 16 * r;
    if (i >= n) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j0 + tj + 16 * c;
      if (j >= m) continue;
      mi_u64* dst = inter + (size_t)i * ldi + j;
      if (!atomic) *dst = (mi_u64)acc[r][c];
      else if (acc[r][c] != 0u) atomicAdd(dst, (mi_u64)acc[r][c]);
    }
  }
}

extern "C" int ape_hip_bitmask_pair_counts(const uint64_t* a, int n, size_t lda, const uint64_t* b, int m, size_t ldb, size_t words,
                                           int64_t* inter, size_t ldi, void* stream) {
  APE_CHECK_ARG(n >= 0 && m >= 0, "ape_hip_bitmask_pair_counts: n = %d, m = %d (a negative count)", n, m);
  if (n == 0 || m == 0) return 0;
  APE_CHECK_ARG(inter, "ape_hip_bitmask_pair_counts: null pointer (inter)");
  APE_CHECK_ARG(words == 0 || (a && b), "ape_hip_bitmask_pair_counts: null pointer (a or b)");
  APE_CHECK_ARG(lda >= words && ldb >= words, "ape_hip_bitmask_pair_counts: lda = %zu / ldb = %zu is less than words = %zu", lda, ldb, words);
  APE_CHECK_ARG(ldi >= (size_t)m, "ape_hip_bitmask_pair_counts: ldi = %zu is less than m = %d", ldi, m);
  APE_CHECK_ARG(words < ((size_t)1 << 40), "ape_hip_bitmask_pair_counts: words = %zu is too large", words);
  hipStream_t st = (hipStream_t)stream;
  const int tiles_i = ceil_div(n, PC_TILE), tiles_j = ceil_div(m, PC_TILE);
  const long long tiles = (long long)tiles_i * tiles_j;
  APE_CHECK_ARG(tiles <= INT32_MAX, "ape_hip_bitmask_pair_counts: %d x %d pairs are too many for one call", n, m);
  // split the word axis until about 4 workgroups per CU exist; a split is a whole number of staging steps
  const long long steps = ((long long)words + PC_KW - 1) / PC_KW;
  long long splits = ((long long)4 * ape_cu_count() + tiles - 1) / tiles;
  if (splits > steps) splits = steps;
  if (splits < 1) splits = 1;
  long long span = ((steps + splits - 1) / splits) * PC_KW;
  if (span > PC_MAX_SPAN) span = PC_MAX_SPAN;
  splits = words == 0 ? 1 : ((long long)words + span - 1) / span;
  APE_CHECK_ARG(splits <= 65535, "ape_hip_bitmask_pair_counts: words = %zu needs too many splits", words);
  const int atomic = splits > 1 ? 1 : 0;
  if (atomic) {                                                   // partial sums are added: start from zero inside the call
    const hipError_t rc = ldi == (size_t)m ? hipMemsetAsync(inter, 0, (size_t)n * m * sizeof(int64_t), st)
                                           : hipMemset2DAsync(inter, ldi * sizeof(int64_t), 0, (size_t)m * sizeof(int64_t), (size_t)n, st);
    if (rc != hipSuccess) {
      ape_set_error("ape_hip_bitmask_pair_counts: memset failed: %s", hipGetErrorString(rc));
      return -2;
    }
  }
  APE_LAUNCH(bitmask_pair_counts_kernel, dim3((unsigned)tiles, (unsigned)splits), dim3(PC_THREADS), 0, st, (const mi_u64*)a, n, (long long)lda,
             (const mi_u64*)b, m, (long long)ldb, (long long)words, span, tiles_j, (mi_u64*)inter, (long long)ldi, atomic);
  APE_CHECK_LAUNCH("ape_hip_bitmask_pair_counts");
  return 0;
}

// ------------------------------------------------------------------------------------------------------------ RLE decode
// one workgroup per mask: ends[j] = min(counts[0] + .. + counts[j], total) for j < min(nruns, cap)
__global__ __launch_bounds__(1024) void rle_ends_kernel(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ nruns, int cap,
                                                        uint32_t total, uint32_t* __restrict__ ends) {
  __shared__ mi_u64 wsum[16];
  __shared__ mi_u64 carry;
  const uint32_t* c = counts + (size_t)blockIdx.x * cap;
  uint32_t* e = ends + (size_t)blockIdx.x * cap;
  const int R = (int)min(nruns[blockIdx.x], (uint32_t)cap);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < R; base += 1024) {
    const int i = base + threadIdx.x;
    mi_u64 incl = i < R ? (mi_u64)c[i] : 0ull;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const mi_u64 t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    mi_u64 before = carry;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    const mi_u64 sum = before + incl;
    if (i < R) e[i] = sum < (mi_u64)total ? (uint32_t)sum : total;
    __syncthreads();
    if (threadIdx.x == 1023) carry = sum;
    __syncthreads();
  }
}

// value of column-major position pos: the number of runs that end at or before pos is the index of the run it falls into
__device__ __forceinline__ uint32_t rle_value(const uint32_t* __restrict__ e, int R, uint32_t pos) {
  int lo = 0, hi = R;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (e[mid] <= pos) lo = mid + 1;
    else hi = mid;
  }
  return lo < R ? (uint32_t)(lo & 1) : 0u;
}

// one thread = one aligned 16-byte piece of the output: bytes 16 g - s .. 16 g - s + 15 of the n * H * W (s = out's address % 16)
__global__ __launch_bounds__(256) void rle_decode_kernel(const uint32_t* __restrict__ ends, const uint32_t* __restrict__ nruns, int cap, int H, int W,
                                                         size_t total, int s, uint8_t* __restrict__ out) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const long long first = (long long)(16 * g) - s;
  if (first >= (long long)total) return;
  const size_t hw = (size_t)H * W;
  const size_t f0 = first < 0 ? 0 : (size_t)first;
  size_t f1 = (size_t)(first + 16);
  if (f1 > total) f1 = total;
  int mi = (int)(f0 / hw);
  const size_t r = f0 % hw;
  int y = (int)(r / W), x = (int)(r % W);
  const uint32_t* e = ends + (size_t)mi * cap;
  int R = (int)min(nruns[mi], (uint32_t)cap);
  uint8_t v[16];
  for (size_t f = f0; f < f1; ++f) {
    v[f - f0] = (uint8_t)rle_value(e, R, (uint32_t)x * (uint32_t)H + (uint32_t)y);
    if (++x == W) {
      x = 0;
      if (++y == H) {
        y = 0;
        ++mi;
        if (f + 1 < f1) {
          e = ends + (size_t)mi * cap;
          R = (int)min(nruns[mi], (uint32_t)cap);
        }
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

extern "C" int ape_hip_rle_decode_workspace_words(int n, int cap) {
  const long long words = (long long)n * cap;                     // ends [n, cap]
  return (n < 0 || cap < 0 || words > 0x7fffffffLL) ? -1 : (int)words;
}

extern "C" int ape_hip_rle_decode(const uint32_t* counts, const uint32_t* nruns, int n, int cap, int H, int W, uint32_t* workspace,
                                  uint8_t* masks, void* stream) {
  APE_CHECK_ARG(n >= 0, "ape_hip_rle_decode: n = %d is negative", n);
  if (n == 0) return 0;
  APE_CHECK_ARG(counts && nruns && workspace && masks, "ape_hip_rle_decode: null pointer");
  APE_CHECK_ARG(H > 0 && W > 0 && cap >= 1, "ape_hip_rle_decode: H = %d, W = %d, cap = %d (all at least 1)", H, W, cap);
  APE_CHECK_ARG((long long)H * W < 0xffffffffLL, "ape_hip_rle_decode: mask too large (H * W = %lld, below 2^32 - 1)", (long long)H * W);
  APE_CHECK_ARG((long long)n * cap <= 0x7fffffffLL, "ape_hip_rle_decode: n * cap = %lld runs are too many for one call", (long long)n * cap);
  hipStream_t st = (hipStream_t)stream;
  const size_t total = (size_t)n * H * W;
  const int s = (int)((uintptr_t)masks & 15);
  const size_t pieces = (total + s + 15) / 16, blocks = (pieces + 255) / 256;
  APE_CHECK_ARG(blocks <= 0x7fffffffULL, "ape_hip_rle_decode: %zu output bytes are too many for one call", total);
  APE_LAUNCH(rle_ends_kernel, dim3(n), dim3(1024), 0, st, counts, nruns, cap, (uint32_t)((long long)H * W), workspace);
  APE_LAUNCH(rle_decode_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const uint32_t*)workspace, nruns, cap, H, W, total, s, masks);
  APE_CHECK_LAUNCH("ape_hip_rle_decode");
  return 0;
}

// cocoapi maskApi.c rleFrString on the host: 5-bit groups, low first, 0x20 = continuation, 0x10 of the last group = sign; from the
// fourth count on the stored value is the difference to the count two back.  Returns the number of runs, or -(needed) if cap is too small.
extern "C" int ape_hip_rle_from_string(const char* s, int len, uint32_t* counts, int cap) {
  if (len <= 0 || s == nullptr) return 0;
  if (cap > 0 && counts == nullptr) cap = 0;
  long long prev1 = 0, prev2 = 0;                                 // counts[m - 1], counts[m - 2]
  int m = 0, p = 0;
  while (p < len && s[p] != 0) {
    long long x = 0;
    int k = 0;
    bool more = true;
    while (more && p < len && s[p] != 0) {
      const long long c = (long long)s[p] - 48;
      x |= (c & 0x1f) << (5 * k);
      more = (c & 0x20) != 0;
      ++p;
      ++k;
      if (!more && (c & 0x10)) x |= (long long)(~0ull << (5 * k));
      if (k >= 12) more = false;                                  // 60 bits: no count is longer
    }
    if (m > 2) x += prev2;
    if (m < cap) counts[m] = (uint32_t)x;
    prev2 = prev1;
    prev1 = (long long)(uint32_t)x;
    ++m;
  }
  return m <= cap ? m : -m;
}
