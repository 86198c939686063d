// Greedy assignment of an image's boxes, two kernels that share nothing but this file (it is the library's last object, build.LINK_LAST,
// and is compiled without multiply-add contraction):
//   box_cover_kernel  : box-proposal coverage, one-to-one and class-agnostic, behind AR@k by area  -- directly below
//   coco_match_kernel : COCOeval's ignore-aware matching of detections to ground truth per class   -- at the end of the file
//
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

// ---------------------------------------------------------------------------------------------------------------------
// COCO matching: the greedy, ignore-aware assignment of pycocotools' COCOeval.evaluateImg for ONE image, all K class groups x A area
// ranges x T IoU thresholds in one launch.
//
//   coco_match : iou [n, m] float64 (row stride ld; a crowd column already holds inter / area_det), det_order [nd] = rows grouped by class,
//                descending score inside a group, det_offsets [K + 1]; gt_order [ng] = columns grouped by class in annotation order,
//                gt_offsets [K + 1]; gt_crowd [m], gt_area [m], det_area [n] by ORIGINAL column / row; thresholds [T]; ranges [A, 2]
//                -> match [A, T, nd] int32 (the original column, or -1), flag [A, T, nd] uint8 (1 true positive, 0 false positive,
//                2 ignored), both by position in det_order.
//   For (group, (lo, hi), t): a ground truth is IGNORED iff crowd or area < lo or area > hi.  The detections go in group order; with
//   lim = min(t, 1 - 1e-10), phase 1 takes, among the not-ignored ground truth not yet taken with iou >= lim, the maximum IoU, the LAST
//   in group order among equals; only if there is none, phase 2 makes the same choice among the ignored ones.  A crowd is never used
//   up, everything else is once taken.  flag = 2 if the matched ground truth is ignored, else 1; without a match flag = 2 if the
//   detection's area lies outside [lo, hi], else 0.
//
// One wave per (group, range, threshold): the problems share nothing, so there is no LDS, no barrier, no atomic and no memset, and a
// wave whose group has no detections leaves at once (with 1203 classes nearly all do).  Lanes stride the group's ground truth -- lane l
// owns positions l, l + 64, ... -- so the taken and the ignored flags of up to 64 x 64 = 4096 ground truths are ONE 64-bit register
// each per lane.  A detection costs one pass over the group's columns of its IoU row and a 64-wide reduction with the key (IoU, position),
// both ascending, for phase 1; phase 2 candidates are collected in the same pass and reduced only when phase 1 found nothing.  The
// first 64 columns of the NEXT detection's row are loaded before the reduction of the current one.  Threshold is the fastest index of
// the grid: the waves of a workgroup read the same rows.  Only float64 comparisons: device and host agree exactly.
#define CM_THREADS 256
#define CM_WAVES (CM_THREADS / 64)
#define CM_MAX_GT 4096               // per group: 64 lanes x the 64 bits of a register
#define CM_MAX_DET 65535             // per group

// (IoU ascending, position ascending): does (v, p) beat (bv, bp)?  No candidate is (-1, -1); a candidate has v >= lim > -1.
__device__ __forceinline__ bool cm_beats(double v, int p, double bv, int bp) { return v > bv || (v == bv && p > bp); }

__device__ __forceinline__ void cm_wave_best(double& bv, int& bp) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const int op = __shfl_xor(bp, o, 64);
    if (cm_beats(ov, op, bv, bp)) {
      bv = ov;
      bp = op;
    }
  }
}

__global__ __launch_bounds__(CM_THREADS) void coco_match_kernel(const double* __restrict__ iou, int n, int m, size_t ld,
                                                                const int* __restrict__ det_order, int nd,
                                                                const int* __restrict__ det_offsets, const int* __restrict__ gt_order, int ng,
                                                                const int* __restrict__ gt_offsets, int K,
                                                                const uint8_t* __restrict__ gt_crowd, const double* __restrict__ gt_area,
                                                                const double* __restrict__ det_area, const double* __restrict__ thresholds,
                                                                int T, const double* __restrict__ ranges, int A,
                                                                int* __restrict__ match, uint8_t* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const long long problem = (long long)blockIdx.x * CM_WAVES + (threadIdx.x >> 6);       // uniform over the wave
  if (problem >= (long long)K * A * T) return;
  const int t = (int)(problem % T), a = (int)((problem / T) % A), k = (int)(problem / ((long long)T * A));

  // offsets from the device are data: nothing they hold becomes an index outside the arrays
  int d0 = det_offsets[k], d1 = det_offsets[k + 1];
  d0 = d0 < 0 ? 0 : d0;
  d1 = d1 > nd ? nd : d1;
  int cnt = d1 - d0;
  if (cnt <= 0) return;
  cnt = cnt > CM_MAX_DET ? CM_MAX_DET : cnt;
  int g0 = gt_offsets[k], g1 = gt_offsets[k + 1];
  g0 = g0 < 0 ? 0 : g0;
  g1 = g1 > ng ? ng : g1;
  int mg = g1 - g0;
  mg = mg < 0 ? 0 : mg > CM_MAX_GT ? CM_MAX_GT : mg;
  const int chunks = (mg + 63) >> 6;

  const double lo = ranges[2 * a], hi = ranges[2 * a + 1];
  const double thr = thresholds[t];
  const double lim = thr < 1.0 - 1e-10 ? thr : 1.0 - 1e-10;

  // bit c of a lane's words speaks of group position lane + 64 c.  `taken` starts set where there is no usable column.
  unsigned long long taken = ~0ull, ign = 0ull, crowd = 0ull;
  int col0 = -1;
  for (int c = 0; c < chunks; ++c) {
    const int j = lane + 64 * c;
    if (j < mg) {
      const int col = gt_order[g0 + j];
      if (col >= 0 && col < m) {
        const double ar = gt_area[col];
        const bool cr = gt_crowd[col] != 0;
        taken &= ~(1ull << c);
        if (cr) crowd |= 1ull << c;
        if (cr || ar < lo || ar > hi) ign |= 1ull << c;
        if (c == 0) col0 = col;
      }
    }
  }

  const size_t out_base = ((size_t)a * T + t) * (size_t)nd;
  int row_next = det_order[d0];
  double v0_next = -1.0;
  if (col0 >= 0 && row_next >= 0 && row_next < n) v0_next = iou[(size_t)row_next * ld + col0];

  for (int i = 0; i < cnt; ++i) {
    const int pos = d0 + i;
    const int row = row_next;
    const double v0 = v0_next;
    const bool row_ok = row >= 0 && row < n;
    if (i + 1 < cnt) {
      row_next = det_order[pos + 1];
      v0_next = -1.0;
      if (col0 >= 0 && row_next >= 0 && row_next < n) v0_next = iou[(size_t)row_next * ld + col0];
    }
    double bv1 = -1.0, bv2 = -1.0;                        // ascending positions per lane: `>=` keeps the last of a tie
    int bp1 = -1, bp2 = -1;
    if (row_ok) {
      if (((taken & 1ull) == 0ull) && v0 >= lim) {
        if (ign & 1ull) {
          bv2 = v0;
          bp2 = lane;
        } else {
          bv1 = v0;
          bp1 = lane;
        }
      }
      for (int c = 1; c < chunks; ++c) {
        const int j = lane + 64 * c;
        if (((taken >> c) & 1ull) == 0ull) {              // implies j < mg and a column inside the matrix
          const double v = iou[(size_t)row * ld + gt_order[g0 + j]];
          if (v >= lim) {
            if ((ign >> c) & 1ull) {
              if (v >= bv2) {
                bv2 = v;
                bp2 = j;
              }
            } else if (v >= bv1) {
              bv1 = v;
              bp1 = j;
            }
          }
        }
      }
    }
    cm_wave_best(bv1, bp1);
    bool ignored_gt = false;
    if (bp1 < 0) {                                        // uniform: every lane holds the wave's result
      cm_wave_best(bv2, bp2);
      bp1 = bp2;
      ignored_gt = true;
    }
    int mcol = -1;
    uint8_t f;
    if (bp1 >= 0) {
      mcol = gt_order[g0 + bp1];
      f = ignored_gt ? 2 : 1;
      const int c = bp1 >> 6;
      if (lane == (bp1 & 63) && ((crowd >> c) & 1ull) == 0ull) taken |= 1ull << c;
    } else {
      f = 0;
      if (row_ok) {
        const double da = det_area[row];
        if (da < lo || da > hi) f = 2;
      }
    }
    if (lane == 0) {
      match[out_base + pos] = mcol;
      flag[out_base + pos] = f;
    }
  }
}

extern "C" int ape_hip_coco_match(const double* iou, int n, int m, size_t ld, const int* det_order, int nd, const int* det_offsets,
                                  const int* gt_order, int ng, const int* gt_offsets, int K, const uint8_t* gt_crowd, const double* gt_area,
                                  const double* det_area, const double* thresholds, int T, const double* ranges, int A, int* match,
                                  uint8_t* flag, void* stream) {
  APE_CHECK_ARG(n >= 0 && m >= 0 && nd >= 0 && ng >= 0 && K >= 0 && T >= 0 && A >= 0,
                "ape_hip_coco_match: negative size (n = %d, m = %d, nd = %d, ng = %d, K = %d, T = %d, A = %d)", n, m, nd, ng, K, T, A);
  if (nd == 0 || T == 0 || A == 0) return 0;
  APE_CHECK_ARG(K > 0, "ape_hip_coco_match: %d detections in no group (K = 0)", nd);
  APE_CHECK_ARG(ng <= CM_MAX_GT, "ape_hip_coco_match: ng = %d grouped ground truths (at most %d per group and call)", ng, CM_MAX_GT);
  APE_CHECK_ARG(nd <= CM_MAX_DET, "ape_hip_coco_match: nd = %d grouped detections (at most %d per group and call)", nd, CM_MAX_DET);
  APE_CHECK_ARG(ld >= (size_t)m, "ape_hip_coco_match: row stride %zu of a matrix with %d columns", ld, m);
  APE_CHECK_ARG(det_order && det_offsets && gt_offsets && det_area && thresholds && ranges && match && flag,
                "ape_hip_coco_match: null pointer");
  APE_CHECK_ARG(ng == 0 || gt_order, "ape_hip_coco_match: null pointer (gt_order)");
  APE_CHECK_ARG(m == 0 || (gt_crowd && gt_area && (n == 0 || iou)), "ape_hip_coco_match: null pointer (ground truth)");
  const long long problems = (long long)K * A * T;
  APE_CHECK_ARG(problems <= 0x7fffffffLL, "ape_hip_coco_match: K x A x T = %lld problems (at most 2^31 - 1 per call)", problems);
  const unsigned grid = (unsigned)((problems + CM_WAVES - 1) / CM_WAVES);
  APE_LAUNCH(coco_match_kernel, dim3(grid), dim3(CM_THREADS), 0, (hipStream_t)stream, iou, n, m, ld, det_order, nd, det_offsets, gt_order,
             ng, gt_offsets, K, gt_crowd, gt_area, det_area, thresholds, T, ranges, A, match, flag);
  APE_CHECK_LAUNCH("ape_hip_coco_match");
  return 0;
}

// ------------------------------------------------------------------------------------------------------------ polygon ground truth
// polygon.hip (COCO polygons -> masks, ape_hip_poly_rasterize) is compiled as part of this object: same flags (no multiply-add
// contraction), and the link line keeps the objects it had (ape_amd/build.py, PART_OF)
#include "polygon.hip"
