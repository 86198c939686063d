// Box-proposal coverage: the greedy one-to-one assignment behind AR@k (detectron2's `_evaluate_box_proposals`, the loop the reference's
// three detection evaluators share), for C (area range, proposal limit) combinations of ONE image in one launch.
//
//   box_cover_overlaps : proposals [n, 4] XYXY in descending score order, gt [m, 4] XYXY, gt_area [m], ranges [C, 2] = (lo, hi),
//                        limits [C] -> overlaps [C, m] float32, match [C, m] int32.  Combination c looks at the first
//                        n_c = min(n, limit_c) proposals and at the GT whose area lies in [lo_c, hi_c], and repeats min(n_c, GT in range)
//                        times: every unused column's best is its maximum IoU over the unused rows (ties: the lowest row), the best
//                        column is the maximum of those (ties: the lowest column); its IoU and row are recorded and both are used up.
//
// One workgroup per combination: the combinations share nothing, so there are no atomics and nobody waits for another workgroup.  The
// n x m IoU matrix is never stored.  What a round needs of it is each unused column's (best IoU, best row), 8 bytes per column in LDS;
// consuming a row invalidates only the columns whose best row it was, and only those are computed again -- by one wave each, its lanes
// striding the rows and meeting in a 64-wide reduction with the key (IoU descending, row ascending).  A round is then one reduction
// over the columns with the key (IoU descending, column ascending), two barriers, and as many column recomputations as the consumed
// row was the best of.  Up to 1024 rows (the reference's largest limit is 1000) are staged in LDS once, so a recomputation's 16 steps per
// lane read at LDS latency; more rows than that are re-read from global memory (n x 16 bytes, resident in L2).
//
// IoU is float32 with exactly the reference's operations in the reference's order and NO multiply-add contraction ((x2 - x1) * (y2 - y1)
// + area_g would fuse otherwise), the division is hipcc's correctly rounded one: the results are the host's, bit for bit.
#include "common.h"
#include "../../include/ape_hip.h"

#pragma clang fp contract(off)

#define BC_THREADS 1024
#define BC_WAVES (BC_THREADS / 64)
#define BC_MAX_M 4096                // columns: 2 x 16 KB of LDS
#define BC_MAX_N 65535               // rows: a bit each, 8 KB of LDS
#define BC_LDS_ROWS 1024             // rows staged in LDS when a combination has no more than these: 16 KB
#define BC_NONE 0x7fffffff

// (value descending, index ascending): is (v, i) ahead of (bv, bi)?
__device__ __forceinline__ bool bc_ahead(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__device__ __forceinline__ float bc_iou(float px1, float py1, float px2, float py2, float gx1, float gy1, float gx2, float gy2, float area_g) {
  const float area_p = (px2 - px1) * (py2 - py1);
  const float w = fmaxf(fminf(px2, gx2) - fmaxf(px1, gx1), 0.f);
  const float h = fmaxf(fminf(py2, gy2) - fmaxf(py1, gy1), 0.f);
  const float inter = w * h;
  return inter > 0.f ? inter / ((area_p + area_g) - inter) : 0.f;
}

// the best unused row of column g among rows [0, nc), by a whole wave: (IoU, row) with the key above in every lane; rows whose bit is
// set in `used` and the row `skip` (consumed in this round, its bit not yet set) do not take part.  (-1, BC_NONE) if there is none.
__device__ __forceinline__ void bc_column_best(const float* prop, int nc, const float* __restrict__ gt, int g,
                                               const uint32_t* used, int skip, int lane, float& best, int& best_row) {
  const float gx1 = gt[4 * g], gy1 = gt[4 * g + 1], gx2 = gt[4 * g + 2], gy2 = gt[4 * g + 3];
  const float area_g = (gx2 - gx1) * (gy2 - gy1);
  float bv = -1.f;
  int br = BC_NONE;
#pragma unroll 4
  for (int r = lane; r < nc; r += 64) {              // ascending rows per lane: `>` keeps the lowest row of a tie
    const float* p = prop + 4 * (size_t)r;
    const float v = bc_iou(p[0], p[1], p[2], p[3], gx1, gy1, gx2, gy2, area_g);
    const bool free_row = ((used[r >> 5] >> (r & 31)) & 1u) == 0u && r != skip;
    if (free_row && v > bv) {
      bv = v;
      br = r;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int orow = __shfl_xor(br, o, 64);
    if (bc_ahead(ov, orow, bv, br)) {
      bv = ov;
      br = orow;
    }
  }
  best = bv;
  best_row = br;
}

// Column state in LDS: val < 0: out of range.  Otherwise row >= 0: unused, (val, row) = its best over the unused rows (row = BC_NONE
// before the first computation); row < 0: used, recorded IoU val with row -1 - row.  A column's state is written only by the wave that
// owns it (columns 64 k .. 64 k + 63 belong to wave k % BC_WAVES) between the two barriers of a round, and read by everybody outside.
__global__ __launch_bounds__(BC_THREADS) void box_cover_kernel(const float* __restrict__ prop, int n, const float* __restrict__ gt,
                                                               const float* __restrict__ gt_area, int m,
                                                               const float* __restrict__ ranges, const int* __restrict__ limits,
                                                               float* __restrict__ overlaps, int* __restrict__ match) {
  __shared__ float s_val[BC_MAX_M];
  __shared__ int s_row[BC_MAX_M];
  __shared__ uint32_t s_used[(BC_MAX_N + 31) / 32];
  __shared__ __attribute__((aligned(16))) float s_prop[4 * BC_LDS_ROWS];
  __shared__ float s_part_val[BC_WAVES];
  __shared__ int s_part_col[BC_WAVES];
  __shared__ int s_part_row[BC_WAVES];
  __shared__ int s_in_range;

  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float lo = ranges[2 * c], hi = ranges[2 * c + 1];
  const int limit = limits[c];
  const int nc = limit > 0 && limit < n ? limit : n;

  const bool staged = nc <= BC_LDS_ROWS;                   // uniform over the workgroup
  if (staged)
    for (int i = tid; i < 4 * nc; i += BC_THREADS) s_prop[i] = prop[i];
  if (tid == 0) s_in_range = 0;
  for (int w = tid; w < (nc + 31) / 32; w += BC_THREADS) s_used[w] = 0u;
  __syncthreads();
  int mine = 0;
  for (int g = tid; g < m; g += BC_THREADS) {
    const float a = gt_area[g];
    const bool in = lo <= a && a <= hi;
    s_val[g] = in ? 0.f : -1.f;
    s_row[g] = BC_NONE;
    mine += in ? 1 : 0;
  }
  if (mine > 0) atomicAdd(&s_in_range, mine);
  __syncthreads();
  const int in_range = s_in_range;
  const int rounds = nc < in_range ? nc : in_range;

  if (rounds > 0) {
    // every column in range: its best over all rows
    for (int base = wave * 64; base < m; base += BC_THREADS) {
      const int g = base + lane;
      unsigned long long todo = __ballot(g < m && s_val[g] >= 0.f);
      while (todo != 0ull) {
        const int gg = base + __builtin_ctzll(todo);
        todo &= todo - 1ull;
        float bv;
        int br;
        if (staged) bc_column_best(s_prop, nc, gt, gg, s_used, -1, lane, bv, br);
        else bc_column_best(prop, nc, gt, gg, s_used, -1, lane, bv, br);
        if (lane == 0) {
          s_val[gg] = bv;
          s_row[gg] = br;
        }
      }
    }
    __syncthreads();

    for (int k = 0; k < rounds; ++k) {
      // the best unused column
      float bv = -1.f;
      int bg = BC_NONE;
      for (int g = tid; g < m; g += BC_THREADS) {    // ascending columns per thread
        const float v = s_val[g];
        if (v >= 0.f && s_row[g] >= 0 && v > bv) {
          bv = v;
          bg = g;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int og = __shfl_xor(bg, o, 64);
        if (bc_ahead(ov, og, bv, bg)) {
          bv = ov;
          bg = og;
        }
      }
      if (lane == 0) {
        s_part_val[wave] = bv;
        s_part_col[wave] = bg;
        s_part_row[wave] = bg != BC_NONE ? s_row[bg] : BC_NONE;
      }
      __syncthreads();
      bv = s_part_val[lane & (BC_WAVES - 1)];
      bg = s_part_col[lane & (BC_WAVES - 1)];
      int brow = s_part_row[lane & (BC_WAVES - 1)];
#pragma unroll
      for (int o = BC_WAVES / 2; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int og = __shfl_xor(bg, o, 64);
        const int orow = __shfl_xor(brow, o, 64);
        if (bc_ahead(ov, og, bv, bg)) {
          bv = ov;
          bg = og;
          brow = orow;
        }
      }
      // rounds <= columns in range, and an unused column always has an unused row left: there is a winner.  The guard keeps a broken
      // invariant from becoming an index.
      if (bg == BC_NONE || brow < 0 || brow >= nc) break;
      const bool last = k + 1 == rounds;
      // the owner of the winning column records it; the columns whose best row is consumed find their next best
      for (int base = wave * 64; base < m; base += BC_THREADS) {
        const int g = base + lane;
        bool need = false;
        if (g < m) {
          if (g == bg) s_row[g] = -1 - brow;
          else need = !last && s_val[g] >= 0.f && s_row[g] == brow;
        }
        unsigned long long todo = __ballot(need);
        while (todo != 0ull) {
          const int gg = base + __builtin_ctzll(todo);
          todo &= todo - 1ull;
          float nv;
          int nr;
          if (staged) bc_column_best(s_prop, nc, gt, gg, s_used, brow, lane, nv, nr);
          else bc_column_best(prop, nc, gt, gg, s_used, brow, lane, nv, nr);
          if (lane == 0) {
            s_val[gg] = nv;
            s_row[gg] = nr;
          }
        }
      }
      __syncthreads();
      if (tid == 0) s_used[brow >> 5] |= 1u << (brow & 31);      // read again only behind the next round's first barrier
    }
  }
  __syncthreads();
  for (int g = tid; g < m; g += BC_THREADS) {
    const float v = s_val[g];
    const int r = s_row[g];
    const bool used = v >= 0.f && r < 0;
    overlaps[(size_t)c * m + g] = v < 0.f ? -1.f : used ? v : 0.f;
    match[(size_t)c * m + g] = used ? -1 - r : -1;
  }
}

extern "C" int ape_hip_box_cover_overlaps(const float* proposals, int n, const float* gt, const float* gt_area, int m, const float* ranges,
                                          const int* limits, int C, float* overlaps, int* match, void* stream) {
  APE_CHECK_ARG(n >= 0 && m >= 0 && C >= 0, "ape_hip_box_cover_overlaps: negative size (n = %d, m = %d, C = %d)", n, m, C);
  if (m == 0 || C == 0) return 0;
  APE_CHECK_ARG(gt && gt_area && ranges && limits && overlaps && match && (n == 0 || proposals), "ape_hip_box_cover_overlaps: null pointer");
  APE_CHECK_ARG(m <= BC_MAX_M, "ape_hip_box_cover_overlaps: m = %d ground-truth boxes (at most %d per call)", m, BC_MAX_M);
  APE_CHECK_ARG(n <= BC_MAX_N, "ape_hip_box_cover_overlaps: n = %d proposals (at most %d per call)", n, BC_MAX_N);
  APE_CHECK_ARG(C <= 65535, "ape_hip_box_cover_overlaps: C = %d combinations (at most 65535 per call)", C);
  APE_LAUNCH(box_cover_kernel, dim3((unsigned)C), dim3(BC_THREADS), 0, (hipStream_t)stream, proposals, n, gt, gt_area, m, ranges, limits,
             overlaps, match);
  APE_CHECK_LAUNCH("ape_hip_box_cover_overlaps");
  return 0;
}
