// Joint histogram of two label maps: hist[a[i]][b[i]] += 1 -- the primitive both segmentation scores reduce to (ape_amd/evaluation.py):
// the semantic confusion matrix is hist[pred class, gt class] (detectron2's SemSegEvaluator builds it with np.bincount(pred * n + gt)),
// the panoptic segment intersections are hist[gt segment, pred segment] (panopticapi's pq_compute_single_core does np.unique on
// gt * OFFSET + pred).  One pass over the maps, no temporary, no host synchronisation; all arithmetic is integer, so the result does
// not depend on the order in which the adds arrive.
//
// Each lane takes LH_V consecutive pixels per step (one vector load per map).  Label maps are spatially coherent, so equal keys are
// combined before they reach an atomic: a lane whose LH_V keys are equal joins a wave-level run (one ballot: the first lane of every
// run of equal lanes adds the run's length), the other lanes add their own runs.  Two destinations, chosen by the table size:
//   * LDS path    : na * nb 32-bit counters fit the LDS a workgroup may allocate (asked from the device, ape_hip_label_hist_lds_bins):
//                   every workgroup counts into a private table and adds its non-zero bins to hist at the end, one 64-bit atomic each.
//                   The grid shrinks with the table (a workgroup's flush costs up to na * nb atomics): about n / (2 na nb) workgroups.
//   * global path : larger tables (460^2 for PascalContext-459, 101 x 501 panoptic pairs): the combined runs go to hist directly.
#include "common.h"
#include "../../include/ape_hip.h"

#define LH_V 8                       // elements per lane and step
#define LH_LDS_THREADS 1024
#define LH_GLOBAL_THREADS 256
#define LH_CHUNK ((size_t)1 << 30)   // elements per launch: a workgroup's 32-bit LDS counters and a lane's reject count cannot overflow

typedef unsigned long long lh_u64;

template <typename T> struct lh_vec { typedef T type __attribute__((ext_vector_type(LH_V))); };

// (a, b) -> bin index, or -1 for a pair that is counted in `rejected`
__device__ __forceinline__ int lh_key(int av, int bv, int na, int nb, int a_ignore, int b_ignore) {
  if (a_ignore >= 0 && av == a_ignore) av = na - 1;
  if (b_ignore >= 0 && bv == b_ignore) bv = nb - 1;
  return ((unsigned)av < (unsigned)na && (unsigned)bv < (unsigned)nb) ? av * nb + bv : -1;
}

template <bool LDS>
__device__ __forceinline__ void lh_add(unsigned* tab, lh_u64* hist, unsigned& rej, int key, unsigned count) {
  if (key >= 0) {
    if (LDS) atomicAdd(&tab[key], count);
    else atomicAdd(&hist[key], (lh_u64)count);
  } else if (key == -1) {
    rej += count;
  }
}

// n = head + LH_V * nvec + tail; a + head and b + head are aligned to a vector (the launcher sets head = n when they cannot both be)
template <typename TA, typename TB, bool LDS>
__global__ __launch_bounds__(LH_LDS_THREADS) void label_pair_hist_kernel(const TA* __restrict__ a, const TB* __restrict__ b, size_t n, size_t head,
                                                                         size_t nvec, int na, int nb, int a_ignore, int b_ignore,
                                                                         lh_u64* __restrict__ hist, lh_u64* __restrict__ rejected) {
  extern __shared__ __attribute__((aligned(16))) unsigned lh_tab[];
  const int bins = na * nb;
  const unsigned tid = threadIdx.x, nthr = blockDim.x;
  if (LDS) {
    for (int i = tid; i < bins; i += nthr) lh_tab[i] = 0u;
    __syncthreads();
  }
  unsigned rej = 0;
  const size_t gtid = (size_t)blockIdx.x * nthr + tid, gstride = (size_t)gridDim.x * nthr;

  // scalar head and tail
  for (size_t i = gtid; i < head; i += gstride)
    lh_add<LDS>(lh_tab, hist, rej, lh_key((int)a[i], (int)b[i], na, nb, a_ignore, b_ignore), 1u);
  for (size_t i = head + nvec * LH_V + gtid; i < n; i += gstride)
    lh_add<LDS>(lh_tab, hist, rej, lh_key((int)a[i], (int)b[i], na, nb, a_ignore, b_ignore), 1u);

  // vector body: the loop bound is the same for every lane of the workgroup, so the ballot below sees whole waves; the vectors of the
  // next step are requested before the current ones are counted
  typedef typename lh_vec<TA>::type VA;
  typedef typename lh_vec<TB>::type VB;
  const VA* __restrict__ av = reinterpret_cast<const VA*>(a + head);
  const VB* __restrict__ bv = reinterpret_cast<const VB*>(b + head);
  const int lane = tid & 63;
  VA va = {};
  VB vb = {};
  size_t base = (size_t)blockIdx.x * nthr;
  if (base + tid < nvec) { va = av[base + tid]; vb = bv[base + tid]; }
  for (; base < nvec; base += gstride) {
    const bool active = base + tid < nvec;
    const VA ca = va;
    const VB cb = vb;
    const size_t nxt = base + gstride + tid;
    if (nxt < nvec) { va = av[nxt]; vb = bv[nxt]; }
    int k[LH_V];
    bool uniform = true;
#pragma unroll
    for (int j = 0; j < LH_V; ++j) {
      k[j] = lh_key((int)ca[j], (int)cb[j], na, nb, a_ignore, b_ignore);
      uniform = uniform && (k[j] == k[0]);
    }
    if (active && !uniform) {                      // the lane's own runs
      unsigned c = 1;
#pragma unroll
      for (int j = 0; j < LH_V; ++j) {
        if (j + 1 < LH_V && k[j + 1] == k[j]) { ++c; }
        else { lh_add<LDS>(lh_tab, hist, rej, k[j], c); c = 1; }
      }
    }
    // runs of lanes with one key each: -2 (a lane that is idle or has counted its own pixels) adds nothing
    const int key = (active && uniform) ? k[0] : -2;
    const int prev = __shfl_up(key, 1, 64);
    const bool first = (lane == 0) || (key != prev);
    const lh_u64 firsts = __ballot(first);
    if (first) {
      const lh_u64 rest = (firsts >> lane) >> 1;
      const unsigned run = rest ? (unsigned)__ffsll((long long)rest) : (unsigned)(64 - lane);
      lh_add<LDS>(lh_tab, hist, rej, key, run * LH_V);
    }
  }

#pragma unroll
  for (int o = 32; o > 0; o >>= 1) rej += __shfl_xor(rej, o, 64);
  if (lane == 0 && rej != 0u) atomicAdd(rejected, (lh_u64)rej);
  if (LDS) {
    __syncthreads();
    for (int i = tid; i < bins; i += nthr) {
      const unsigned v = lh_tab[i];
      if (v != 0u) atomicAdd(&hist[i], (lh_u64)v);
    }
  }
}

// bytes of LDS one workgroup may allocate on the current device (0 if there is no device to ask)
static size_t lh_lds_limit() {
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

extern "C" int ape_hip_label_hist_lds_bins(void) {
  const size_t lim = lh_lds_limit();
  if (lim == 0) {
    ape_set_error("ape_hip_label_hist_lds_bins: no HIP device to ask for its LDS limit");
    return -2;
  }
  return (int)(lim / sizeof(unsigned));
}

template <typename TA, typename TB>
static int lh_launch(const void* a, const void* b, size_t n, int na, int nb, int a_ignore, int b_ignore, int64_t* hist, int64_t* rejected,
                     hipStream_t stream) {
  const size_t bins = (size_t)na * nb, lds_bytes = bins * sizeof(unsigned);
  const size_t limit = lh_lds_limit();
  const bool lds = limit != 0 && lds_bytes <= limit;
  if (lds && lds_bytes > 64 * 1024) {              // above 64 KiB the allocation has to be allowed per function (and device)
    static ApeOncePerDevice attr_done;
    if (attr_done.first()) {
      (void)hipFuncSetAttribute((const void*)label_pair_hist_kernel<TA, TB, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit);
    }
  }
  const int cus = ape_cu_count();
  for (size_t off = 0; off < n; off += LH_CHUNK) {
    const TA* pa = (const TA*)a + off;
    const TB* pb = (const TB*)b + off;
    const size_t m = n - off < LH_CHUNK ? n - off : LH_CHUNK;
    // elements up to the next vector boundary of either map; the vector body needs one boundary that serves both
    const size_t ha = ((0 - (uintptr_t)pa) % (LH_V * sizeof(TA))) / sizeof(TA), hb = ((0 - (uintptr_t)pb) % (LH_V * sizeof(TB))) / sizeof(TB);
    const bool vec_ok = ha == hb && (uintptr_t)pa % sizeof(TA) == 0 && (uintptr_t)pb % sizeof(TB) == 0 && ha < m;
    const size_t head = vec_ok ? ha : m, nvec = (m - head) / LH_V;
    const size_t steps = nvec > 0 ? nvec : (m + LH_V - 1) / LH_V;     // lane-steps of work
    if (lds) {
      size_t g = m / (2 * bins);
      const size_t by_work = (steps + LH_LDS_THREADS - 1) / LH_LDS_THREADS;
      if (g > by_work) g = by_work;
      if (g > (size_t)2 * cus) g = (size_t)2 * cus;
      if (g < 1) g = 1;
      APE_LAUNCH((label_pair_hist_kernel<TA, TB, true>), dim3((unsigned)g), dim3(LH_LDS_THREADS), lds_bytes, stream, pa, pb, m, head, nvec, na, nb,
                 a_ignore, b_ignore, (lh_u64*)hist, (lh_u64*)rejected);
    } else {
      size_t g = (steps + LH_GLOBAL_THREADS - 1) / LH_GLOBAL_THREADS;
      if (g > (size_t)8 * cus) g = (size_t)8 * cus;
      APE_LAUNCH((label_pair_hist_kernel<TA, TB, false>), dim3((unsigned)g), dim3(LH_GLOBAL_THREADS), 0, stream, pa, pb, m, head, nvec, na, nb,
                 a_ignore, b_ignore, (lh_u64*)hist, (lh_u64*)rejected);
    }
  }
  APE_CHECK_LAUNCH("ape_hip_label_pair_hist");
  return 0;
}

template <typename TA>
static int lh_launch_b(const void* a, const void* b, int b_bytes, size_t n, int na, int nb, int a_ignore, int b_ignore, int64_t* hist,
                       int64_t* rejected, hipStream_t stream) {
  if (b_bytes == 1) return lh_launch<TA, uint8_t>(a, b, n, na, nb, a_ignore, b_ignore, hist, rejected, stream);
  if (b_bytes == 2) return lh_launch<TA, int16_t>(a, b, n, na, nb, a_ignore, b_ignore, hist, rejected, stream);
  return lh_launch<TA, int32_t>(a, b, n, na, nb, a_ignore, b_ignore, hist, rejected, stream);
}

extern "C" int ape_hip_label_pair_hist(const void* a, int a_bytes, const void* b, int b_bytes, size_t n, int na, int nb, int a_ignore,
                                       int b_ignore, int64_t* hist, int64_t* rejected, void* stream) {
  APE_CHECK_ARG((a_bytes == 1 || a_bytes == 2 || a_bytes == 4) && (b_bytes == 1 || b_bytes == 2 || b_bytes == 4),
                "ape_hip_label_pair_hist: element width %d / %d (1 = uint8, 2 = int16, 4 = int32)", a_bytes, b_bytes);
  APE_CHECK_ARG(na >= 1 && nb >= 1 && (int64_t)na * nb <= INT32_MAX, "ape_hip_label_pair_hist: table %d x %d (both >= 1, na * nb < 2^31)", na, nb);
  if (n == 0) return 0;
  APE_CHECK_ARG(a && b && hist && rejected, "ape_hip_label_pair_hist: null pointer");
  if (a_bytes == 1) return lh_launch_b<uint8_t>(a, b, b_bytes, n, na, nb, a_ignore, b_ignore, hist, rejected, (hipStream_t)stream);
  if (a_bytes == 2) return lh_launch_b<int16_t>(a, b, b_bytes, n, na, nb, a_ignore, b_ignore, hist, rejected, (hipStream_t)stream);
  return lh_launch_b<int32_t>(a, b, b_bytes, n, na, nb, a_ignore, b_ignore, hist, rejected, (hipStream_t)stream);
}
