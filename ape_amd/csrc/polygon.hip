// COCO polygon ground truth rasterised on the device, pixel for pixel what pycocotools' annToRLE gives (cocoapi maskApi.c rleFrPoly per
// polygon, rleMerge as a union per object).  rleFrPoly walks the polygon's boundary on a 5x grid with its own rounding, records one
// column-major index a = x * h + y per column the walk crosses, sorts the indices, appends h * w, differences them and merges empty runs.
// That sort-difference-merge is a parity: pixel p (column-major) is foreground iff the number of recorded a <= p is odd, and a recorded
// a = h * w changes nothing.  So there is no sort and no sequential merge here:
//   toggle : one wave per polygon edge, its lanes stride over the edge's points.  Point i of the walk is a closed form of its edge and of d,
//            its predecessor is the point before it on the edge or the last point of the previous edge; a crossing (u_i != u_{i-1}) whose
//            column is a pixel column flips ONE bit of the polygon's column-major bitmap with an integer atomic XOR (any order of arrival
//            gives the same bits).  The bitmaps are zeroed by a memset node of the call.  Index h * w is dropped, never written.
//   fill   : one workgroup per OBJECT; per polygon an inclusive prefix parity over the bitmap's 64-bit words -- inside a word the shift-XOR
//            ladder, between words the parity of the popcount of everything before (ballot per wave, 16 wave parities through LDS, a carry from
//            chunk to chunk of PF_THREADS words) -- ORed into the object's column-major bits; then the object's area, a popcount.  A thread
//            owns the same words in every pass, so no atomics and no memset; an object without polygons writes zeros.
//   output : the object's column-major bits -> row-major uint8 0 / 1, in aligned 16-byte pieces; exactly the n * H * W bytes at any address.
// Double arithmetic with one rounding per operation: `ys + s * t + .5` is the C code's.  This file is not compiled on its own: boxcover.hip
// includes it at its end (ape_amd/build.py, PART_OF), which gives it that file's -ffp-contract=off and leaves the link line as it was.
#include "common.h"
#include "../../include/ape_hip.h"

typedef unsigned long long pg_u64;

#define PG_COORD_MAX 65536.0         // |coordinate| bound: 5 * c stays far inside int32 and an edge has at most 655361 points
#define PT_THREADS 256               // toggle: 4 waves = 4 edges per workgroup
#define PF_THREADS 1024              // fill: words per chunk (one per thread) = 65536 pixels
#define PO_THREADS 256               // output: 16 bytes per thread

struct PgEdge {
  int xs, ys, dx, dy, flip;          // after the swap of a flipped edge
  double s;
};

// X[j] = (int)(5 * x + .5); a coordinate outside +-PG_COORD_MAX is clamped (a NaN reads as the lower bound): the walk stays bounded whatever
// the data
__device__ __forceinline__ int pg_grid(double c) {
  c = fmin(fmax(c, -PG_COORD_MAX), PG_COORD_MAX);
  return (int)(5.0 * c + .5);
}

__device__ __forceinline__ PgEdge pg_edge(int xs, int ys, int xe, int ye) {
  PgEdge e;
  e.dx = abs(xe - xs);
  e.dy = abs(ys - ye);
  e.flip = (e.dx >= e.dy && xs > xe) || (e.dx < e.dy && ys > ye);
  if (e.flip) {
    int t = xs; xs = xe; xe = t;
    t = ys; ys = ye; ye = t;
  }
  e.xs = xs;
  e.ys = ys;
  if (e.dx == 0 && e.dy == 0) e.s = 0.0;                          // one point, (xs, ys)
  else e.s = e.dx >= e.dy ? (double)(ye - ys) / (double)e.dx : (double)(xe - xs) / (double)e.dy;
  return e;
}

__device__ __forceinline__ int pg_points(const PgEdge& e) { return (e.dx >= e.dy ? e.dx : e.dy) + 1; }

// point d (0 .. pg_points - 1) of the edge, in walking order
__device__ __forceinline__ void pg_point(const PgEdge& e, int d, int& u, int& v) {
  const int mx = e.dx >= e.dy ? e.dx : e.dy;
  const int t = e.flip ? mx - d : d;
  if (mx == 0) {
    u = e.xs;
    v = e.ys;
  } else if (e.dx >= e.dy) {
    u = t + e.xs;
    v = (int)((double)e.ys + e.s * (double)t + .5);
  } else {
    v = t + e.ys;
    u = (int)((double)e.xs + e.s * (double)t + .5);
  }
}

// ------------------------------------------------------------------------------------------------------------ toggle
// wave g = edge g of all polygons together: the edge that starts at vertex g.  Offsets are data: a range is clamped to [0, V], an edge whose
// polygon cannot be found is skipped.
__global__ __launch_bounds__(PT_THREADS) void poly_toggle_kernel(const double* __restrict__ xy, int V, const int* __restrict__ vert_offsets,
                                                                 int P, int H, int W, long long words, pg_u64* __restrict__ toggles) {
  const int lane = threadIdx.x & 63;
  const long long g64 = (long long)blockIdx.x * (PT_THREADS / 64) + (threadIdx.x >> 6);
  if (g64 >= V) return;
  const int g = (int)g64;
  int lo = 0, hi = P + 1;                                         // the number of offsets <= g, minus one, is the polygon
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (vert_offsets[mid] <= g) lo = mid + 1;
    else hi = mid;
  }
  const int p = lo - 1;
  if (p < 0 || p >= P) return;
  const int v0 = min(max(vert_offsets[p], 0), V), v1 = min(max(vert_offsets[p + 1], v0), V);
  if (g < v0 || g >= v1) return;
  const int k = v1 - v0, j = g - v0, jn = j + 1 < k ? j + 1 : 0;
  const int xs = pg_grid(xy[2 * (size_t)(v0 + j)]), ys = pg_grid(xy[2 * (size_t)(v0 + j) + 1]);
  const int xe = pg_grid(xy[2 * (size_t)(v0 + jn)]), ye = pg_grid(xy[2 * (size_t)(v0 + jn) + 1]);
  const PgEdge cur = pg_edge(xs, ys, xe, ye);
  PgEdge prev = cur;
  if (j > 0) prev = pg_edge(pg_grid(xy[2 * (size_t)(v0 + j - 1)]), pg_grid(xy[2 * (size_t)(v0 + j - 1) + 1]), xs, ys);
  const int npts = pg_points(cur);
  const long long hw = (long long)H * W;
  pg_u64* __restrict__ tog = toggles + (size_t)p * words;
  for (int d = lane; d < npts; d += 64) {
    int u, v, pu, pv;
    if (d > 0) pg_point(cur, d - 1, pu, pv);
    else if (j > 0) pg_point(prev, pg_points(prev) - 1, pu, pv);
    else continue;                                                // the walk's first point has no predecessor
    pg_point(cur, d, u, v);
    if (u == pu) continue;
    double xd = (double)(u < pu ? u : u - 1);
    xd = (xd + .5) / 5.0 - .5;
    if (floor(xd) != xd || xd < 0 || xd > (double)(W - 1)) continue;
    double yd = (double)(v < pv ? v : pv);
    yd = (yd + .5) / 5.0 - .5;
    if (yd < 0) yd = 0;
    else if (yd > (double)H) yd = (double)H;
    yd = ceil(yd);
    const long long a = (long long)(int)xd * H + (long long)(int)yd;
    if (a < 0 || a >= hw) continue;                               // yd == h in the last column: h * w, one past the mask
    atomicXor(&tog[a >> 6], 1ull << (a & 63));
  }
}

// ------------------------------------------------------------------------------------------------------------ fill
__global__ __launch_bounds__(PF_THREADS) void poly_fill_kernel(const pg_u64* __restrict__ toggles, const int* __restrict__ poly_offsets, int P,
                                                               long long hw, long long words, pg_u64* __restrict__ objbits,
                                                               long long* __restrict__ area) {
  __shared__ uint32_t wpar[2][PF_THREADS / 64];
  __shared__ uint32_t wcount[PF_THREADS / 64];
  const int o = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p0 = min(max(poly_offsets[o], 0), P), p1 = min(max(poly_offsets[o + 1], p0), P);
  pg_u64* __restrict__ ob = objbits + (size_t)o * words;
  const pg_u64 tail = (hw & 63) ? (1ull << (hw & 63)) - 1ull : ~0ull;     // the bits of the last word that are pixels
  if (p0 == p1)
    for (long long i = tid; i < words; i += PF_THREADS) ob[i] = 0ull;
  int buf = 0;
  for (int p = p0; p < p1; ++p) {
    const pg_u64* __restrict__ tog = toggles + (size_t)p * words;
    uint32_t carry = 0;                                           // parity of every toggle before this chunk: the same in all threads
    for (long long base = 0; base < words; base += PF_THREADS, buf ^= 1) {
      const long long i = base + tid;
      pg_u64 w = i < words ? tog[i] : 0ull;
      w ^= w << 1;
      w ^= w << 2;
      w ^= w << 4;
      w ^= w << 8;
      w ^= w << 16;
      w ^= w << 32;                                               // bit b = parity of the word's bits 0 .. b
      const pg_u64 odd = __ballot((int)(w >> 63));                // lanes whose whole word has odd parity
      if (lane == 0) wpar[buf][wave] = (uint32_t)__popcll(odd) & 1u;
      __syncthreads();                                            // the only barrier of a chunk: the next chunk writes the other buffer
      const uint32_t waves = (uint32_t)__ballot(lane < PF_THREADS / 64 && wpar[buf][lane & (PF_THREADS / 64 - 1)] != 0u);
      const uint32_t before = carry ^ ((uint32_t)__popc(waves & ((1u << wave) - 1u)) & 1u) ^
                              ((uint32_t)__popcll(odd & ((1ull << lane) - 1ull)) & 1u);
      carry ^= (uint32_t)__popc(waves) & 1u;
      if (i < words) {
        pg_u64 out = before ? ~w : w;
        if (i == words - 1) out &= tail;
        ob[i] = p == p0 ? out : (ob[i] | out);                    // this thread wrote ob[i] itself in the polygon before
      }
    }
  }
  uint32_t count = 0;                                             // fewer than 2^32 pixels in all
  for (long long i = tid; i < words; i += PF_THREADS) count += (uint32_t)__popcll(ob[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off, 64);
  if (lane == 0) wcount[wave] = count;
  __syncthreads();
  if (tid == 0) {
    long long total = 0;
    for (int w = 0; w < PF_THREADS / 64; ++w) total += (long long)wcount[w];
    area[o] = total;
  }
}

// ------------------------------------------------------------------------------------------------------------ output
// one thread = one aligned 16-byte piece of the output: bytes 16 g - s .. 16 g - s + 15 of the n * H * W (s = out's address % 16)
__global__ __launch_bounds__(PO_THREADS) void poly_output_kernel(const pg_u64* __restrict__ objbits, long long words, int H, int W, size_t total,
                                                                 int s, uint8_t* __restrict__ out) {
  const size_t g = (size_t)blockIdx.x * PO_THREADS + threadIdx.x;
  const long long first = (long long)(16 * g) - s;
  if (first >= (long long)total) return;
  const size_t hw = (size_t)H * W;
  const size_t f0 = first < 0 ? 0 : (size_t)first;
  size_t f1 = (size_t)(first + 16);
  if (f1 > total) f1 = total;
  size_t mi = f0 / hw;
  const size_t r = f0 % hw;
  int y = (int)(r / W), x = (int)(r % W);
  const pg_u64* ob = objbits + mi * (size_t)words;
  uint8_t v[16];
  for (size_t f = f0; f < f1; ++f) {
    const size_t pos = (size_t)x * H + y;
    v[f - f0] = (uint8_t)((ob[pos >> 6] >> (pos & 63)) & 1ull);
    if (++x == W) {
      x = 0;
      if (++y == H) {
        y = 0;
        ++mi;
        ob += words;                                              // read only if another byte of the piece follows: f + 1 < f1 <= total
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

// 64-bit words: the polygons' toggle bitmaps [npoly, words] followed by the objects' column-major bits [nobj, words]
extern "C" int ape_hip_poly_workspace_words(int nobj, int npoly, int H, int W) {
  if (nobj < 0 || npoly < 0 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL) return -1;
  const long long words = ((long long)H * W + 63) / 64;
  const long long total = ((long long)nobj + npoly) * words;
  return total > 0x7fffffffLL ? -1 : (int)total;
}

extern "C" int ape_hip_poly_rasterize(const double* xy, int nvert, const int32_t* vert_offsets, int npoly, const int32_t* poly_offsets,
                                      int nobj, int H, int W, uint64_t* workspace, uint8_t* masks, int64_t* area, void* stream) {
  APE_CHECK_ARG(nobj >= 0 && npoly >= 0 && nvert >= 0, "ape_hip_poly_rasterize: nobj = %d, npoly = %d, nvert = %d (a negative count)", nobj,
                npoly, nvert);
  if (nobj == 0) return 0;
  APE_CHECK_ARG(H > 0 && W > 0, "ape_hip_poly_rasterize: H = %d, W = %d (both at least 1)", H, W);
  APE_CHECK_ARG((long long)H * W <= 0x7fffffffLL, "ape_hip_poly_rasterize: mask too large (H * W = %lld, below 2^31)", (long long)H * W);
  APE_CHECK_ARG(ape_hip_poly_workspace_words(nobj, npoly, H, W) >= 0, "ape_hip_poly_rasterize: the workspace of %d objects and %d polygons is too large",
                nobj, npoly);
  APE_CHECK_ARG(poly_offsets && workspace && masks && area, "ape_hip_poly_rasterize: null pointer");
  APE_CHECK_ARG(npoly == 0 || vert_offsets, "ape_hip_poly_rasterize: null pointer (vert_offsets)");
  APE_CHECK_ARG(nvert == 0 || (xy && npoly > 0), "ape_hip_poly_rasterize: %d vertices without coordinates or polygons", nvert);
  APE_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)area & 7) == 0 && ((uintptr_t)xy & 7) == 0,
                "ape_hip_poly_rasterize: xy, workspace and area must be 8-byte aligned");
  const size_t total = (size_t)nobj * H * W;
  const int s = (int)((uintptr_t)masks & 15);
  const size_t pieces = (total + s + 15) / 16, blocks = (pieces + PO_THREADS - 1) / PO_THREADS;
  APE_CHECK_ARG(blocks <= 0x7fffffffULL, "ape_hip_poly_rasterize: %zu output bytes are too many for one call", total);
  hipStream_t st = (hipStream_t)stream;
  const long long hw = (long long)H * W, words = (hw + 63) / 64;
  pg_u64* toggles = (pg_u64*)workspace;
  pg_u64* objbits = toggles + (size_t)npoly * words;
  if (npoly > 0 && nvert > 0) {
    if (hipMemsetAsync(toggles, 0, (size_t)npoly * words * sizeof(pg_u64), st) != hipSuccess) {
      ape_set_error("ape_hip_poly_rasterize: memset failed");
      return -2;
    }
    const unsigned edges = (unsigned)(((long long)nvert + PT_THREADS / 64 - 1) / (PT_THREADS / 64));
    APE_LAUNCH(poly_toggle_kernel, dim3(edges), dim3(PT_THREADS), 0, st, xy, nvert, vert_offsets, npoly, H, W, words, toggles);
  }
  // without a vertex no polygon has a toggle: the fill then sees no polygons at all and never reads the (unset) bitmaps
  APE_LAUNCH(poly_fill_kernel, dim3((unsigned)nobj), dim3(PF_THREADS), 0, st, (const pg_u64*)toggles, poly_offsets, nvert > 0 ? npoly : 0, hw, words,
             objbits, (long long*)area);
  APE_LAUNCH(poly_output_kernel, dim3((unsigned)blocks), dim3(PO_THREADS), 0, st, (const pg_u64*)objbits, words, H, W, total, s, masks);
  APE_CHECK_LAUNCH("ape_hip_poly_rasterize");
  return 0;
}
