// libpdd: friends-of-friends grouping of single-pulse candidates across DM
// row, time and width -- connected components of the link graph of
// pypulsar_amd/spgroup.py (restated by brute force in
// tests/spgroup_oracle.py).  gfx950.
//
// Candidates are the int32 records {row, start, width, snr bits} of
// pdd_sp_search in canonical order, i.e. sorted by the 64-bit cell key
// (start >> 10) * nrows + row first.  Two candidates are linked when their
// rows differ by at most row_tol and the gap between their extents
// [start, start + width) is at most time_tol samples.
//
// Kernels:
//   k_spg_init     parent[i] = i (the label array is the union-find forest).
//   k_spg_link     one lane per candidate i.  A partner lies at most two
//                  windows away (width <= 1025, time_tol <= 1023); every pair
//                  is tested once, from its higher index: the partners of i
//                  with a lower index are in windows K - 2, K - 1 (rows r -
//                  row_tol .. r + row_tol: one contiguous key range each) and
//                  in the part of its own window below i.  The ranges are
//                  found by binary search over the records' keys -- no grid
//                  of the plane -- and scanned.  Linked pairs are united by
//                  hooking the larger root under the smaller with a
//                  compare-and-swap, so a component's final root is its
//                  smallest index whatever the order of events.  The only
//                  loops are lock-free retries: a failed hook means another
//                  lane's hook succeeded.
//   k_spg_flatten  label[i] = find(i), in a launch of its own.
//   k_spg_sum_init / k_spg_sum / k_spg_sum_final
//                  the group records: integer atomics at the root's record
//                  (order independent), after a segmented scan over each run
//                  of neighbouring lanes that share a root -- after the
//                  canonical sort a bow tie's members are close in index, so
//                  a run costs one set of atomics, not one per lane.
#include "pdd_internal.h"

namespace pdd {

namespace {

constexpr int kSpgThreads = 256;
constexpr int kSpgMaxRowTol = 16;
constexpr int kSpgMaxTimeTol = 1023;
constexpr int kSpgWinShift = 10;  // windows of 1024 starts (kSpWin of pdd_search.hip)
constexpr int kSpgReach = 2;      // (1025 + 1023) / 1024 windows back

// The forest is read and written by many waves at once: relaxed agent-scope
// atomics, never plain accesses the compiler may keep in a register.
__device__ __forceinline__ int32_t spg_ld(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void spg_st(int32_t* p, int32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Root of x.  parent[y] <= y always.  kHalve: with path halving, which writes
// only a non-root -- a non-root never becomes a root again, so it cannot
// collide with a hook (a compare-and-swap on a root) -- and writes an
// ancestor.  k_spg_flatten finds without it: a halving store of an ancestor
// that lands after the owner's store of the root would leave a label that is
// not the root.
template <bool kHalve>
__device__ __forceinline__ int32_t spg_find(int32_t* parent, int32_t x) {
  int32_t p = spg_ld(parent + x);
  while (p != x) {
    const int32_t g = spg_ld(parent + p);
    if (kHalve && g != p) spg_st(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

__device__ __forceinline__ void spg_unite(int32_t* parent, int32_t a, int32_t b) {
  for (;;) {
    a = spg_find<true>(parent, a);
    b = spg_find<true>(parent, b);
    if (a == b) return;
    const int32_t hi = max(a, b), lo = min(a, b);
    if (atomicCAS(parent + hi, hi, lo) == hi) return;
    // (hi was hooked by another lane meanwhile: find again)
  }
}

__device__ __forceinline__ int64_t spg_key(const int4 c, int64_t nrows) {
  return (int64_t)(c.y >> kSpgWinShift) * nrows + c.x;
}

// First index in [lo, hi) whose key is >= key (hi: none).
__device__ __forceinline__ int64_t spg_lower(const int4* __restrict__ cands, int64_t lo, int64_t hi,
                                             int64_t nrows, int64_t key) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (spg_key(cands[mid], nrows) < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kSpgThreads) void k_spg_init(int64_t k, int32_t* __restrict__ parent) {
  const int64_t i = (int64_t)blockIdx.x * kSpgThreads + threadIdx.x;
  if (i < k) parent[i] = (int32_t)i;
}

__global__ __launch_bounds__(kSpgThreads) void k_spg_link(const int4* __restrict__ cands, int64_t k,
                                                          int64_t nrows, int row_tol, int time_tol,
                                                          int32_t* parent) {
  const int64_t i = (int64_t)blockIdx.x * kSpgThreads + threadIdx.x;
  if (i >= k) return;
  const int4 a = cands[i];
  const int64_t K = a.y >> kSpgWinShift;
  const int64_t rlo = max((int64_t)a.x - row_tol, (int64_t)0);
  const int64_t rhi = min((int64_t)a.x + row_tol, nrows - 1);
  const int ea = a.y + a.z;
  int64_t from = 0;
  for (int back = kSpgReach; back >= 0; --back) {
    const int64_t W = K - back;
    if (W < 0) continue;
    // every index found is in [0, i): nothing outside the list is read,
    // whatever the records hold.  The range bounds ascend, so each search
    // starts where the last one ended: only the first spans the whole list.
    const int64_t j0 = spg_lower(cands, from, i, nrows, W * nrows + rlo);
    const int64_t j1 = back ? spg_lower(cands, j0, i, nrows, W * nrows + rhi + 1) : i;
    from = j1;
    for (int64_t j = j0; j < j1; ++j) {
      const int4 b = cands[j];
      const int gap = max(a.y, b.y) - min(ea, b.y + b.z);
      if (abs(a.x - b.x) <= row_tol && gap <= time_tol) spg_unite(parent, (int32_t)i, (int32_t)j);
    }
  }
}

__global__ __launch_bounds__(kSpgThreads) void k_spg_flatten(int64_t k, int32_t* parent) {
  const int64_t i = (int64_t)blockIdx.x * kSpgThreads + threadIdx.x;
  if (i >= k) return;
  // (no hook runs in this launch: the roots are final, and every value a
  // lane reads -- a parent of the link launch or a root stored here -- is an
  // ancestor)
  spg_st(parent + i, spg_find<false>(parent, (int32_t)i));
}

// float32 bits -> unsigned key with the order of the values, as zap_key of
// pdd_zap.hip; -0 counts as +0 (they compare equal as floats).
__device__ __forceinline__ uint32_t spg_snr_key(int32_t bits) {
  uint32_t b = (uint32_t)bits;
  if (b == 0x80000000u) b = 0;
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

// The record of a root starts as the identity of its atomics; every other
// record is zeros and stays so.  Slots 6, 7 of a root hold the 64-bit
// (snr key << 32 | ~index) maximum until k_spg_sum_final unpacks it.
__global__ __launch_bounds__(kSpgThreads) void k_spg_sum_init(const int32_t* __restrict__ label,
                                                              int64_t k, int4* __restrict__ groups) {
  const int64_t i = (int64_t)blockIdx.x * kSpgThreads + threadIdx.x;
  if (i >= k) return;
  const bool root = label[i] == (int32_t)i;
  const int32_t big = 0x7fffffff;
  groups[2 * i] = root ? make_int4(0, 0, big, 0) : make_int4(0, 0, 0, 0);
  groups[2 * i + 1] = root ? make_int4(big, 0, 0, 0) : make_int4(0, 0, 0, 0);
}

__global__ __launch_bounds__(kSpgThreads) void k_spg_sum(const int4* __restrict__ cands,
                                                         const int32_t* __restrict__ label,
                                                         int64_t k, int32_t* groups) {
  const int64_t i = (int64_t)blockIdx.x * kSpgThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  // (no early return: every lane of the wave takes part in the shuffles; a
  // lane past the end, or one with a label outside the list, has root -1 and
  // adds nothing)
  int32_t g = -1;
  int4 c = make_int4(0, 0, 0, 0);
  if (i < k) {
    g = label[i];
    c = cands[i];
    if (g < 0 || (int64_t)g >= k) g = -1;
  }
  const int32_t gprev = __shfl_up(g, 1);
  const bool head = lane == 0 || gprev != g;
  const unsigned long long heads = __ballot(head);
  // first lane of this lane's run: the highest head at or below it
  const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
  int32_t cnt = 1, rlo = c.x, rhi = c.x, slo = c.y, ehi = c.y + c.z;
  uint32_t bkey = spg_snr_key(c.w), bidx = ~(uint32_t)i;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int32_t ocnt = __shfl_up(cnt, d), orlo = __shfl_up(rlo, d), orhi = __shfl_up(rhi, d);
    const int32_t oslo = __shfl_up(slo, d), oehi = __shfl_up(ehi, d);
    const uint32_t okey = __shfl_up(bkey, d), oidx = __shfl_up(bidx, d);
    if (lane - d >= start) {
      cnt += ocnt;
      rlo = min(rlo, orlo);
      rhi = max(rhi, orhi);
      slo = min(slo, oslo);
      ehi = max(ehi, oehi);
      if (okey > bkey || (okey == bkey && oidx > bidx)) {
        bkey = okey;
        bidx = oidx;
      }
    }
  }
  const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
  if (!tail || g < 0) return;
  int32_t* rec = groups + (int64_t)g * 8;
  atomicAdd(rec + 0, cnt);
  atomicMin(rec + 2, rlo);
  atomicMax(rec + 3, rhi);
  atomicMin(rec + 4, slo);
  atomicMax(rec + 5, ehi);
  atomicMax(reinterpret_cast<unsigned long long*>(rec + 6),
            ((unsigned long long)bkey << 32) | (unsigned long long)bidx);
}

__global__ __launch_bounds__(kSpgThreads) void k_spg_sum_final(const int4* __restrict__ cands,
                                                               int64_t k, int32_t* __restrict__ groups) {
  const int64_t i = (int64_t)blockIdx.x * kSpgThreads + threadIdx.x;
  if (i >= k) return;
  int32_t* rec = groups + i * 8;
  if (rec[0] <= 0) return;
  const int32_t best = (int32_t)~(uint32_t)rec[6];
  rec[1] = best;
  rec[6] = (best >= 0 && (int64_t)best < k) ? cands[best].w : 0;
  rec[7] = 0;
}

}  // namespace

}  // namespace pdd

using namespace pdd;

extern "C" {

int pdd_spg_label(const int32_t* cands, int64_t k, int64_t nrows, int row_tol, int time_tol,
                  int32_t* label, void* stream) {
  PDD_REQUIRE(k >= 0 && k < (1ll << 31), "pdd_spg_label: k out of range 0..2^31-1");
  PDD_REQUIRE(row_tol >= 0 && row_tol <= kSpgMaxRowTol, "pdd_spg_label: row_tol out of range 0..%d",
              kSpgMaxRowTol);
  PDD_REQUIRE(time_tol >= 0 && time_tol <= kSpgMaxTimeTol,
              "pdd_spg_label: time_tol out of range 0..%d", kSpgMaxTimeTol);
  PDD_REQUIRE(nrows >= 1 && nrows <= (1ll << 31), "pdd_spg_label: nrows out of range 1..2^31");
  if (k == 0) return 0;
  PDD_REQUIRE(cands && label, "pdd_spg_label: null pointer");
  PDD_REQUIRE(((uintptr_t)cands & 15) == 0, "pdd_spg_label: cands must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const unsigned nb = (unsigned)cdiv(k, kSpgThreads);
  const int4* c4 = reinterpret_cast<const int4*>(cands);
  k_spg_init<<<nb, kSpgThreads, 0, st>>>(k, label);
  PDD_LAUNCHED();
  k_spg_link<<<nb, kSpgThreads, 0, st>>>(c4, k, nrows, row_tol, time_tol, label);
  PDD_LAUNCHED();
  k_spg_flatten<<<nb, kSpgThreads, 0, st>>>(k, label);
  PDD_LAUNCHED();
  return 0;
}

int pdd_spg_summarise(const int32_t* cands, const int32_t* label, int64_t k, int32_t* groups,
                      void* stream) {
  PDD_REQUIRE(k >= 0 && k < (1ll << 31), "pdd_spg_summarise: k out of range 0..2^31-1");
  if (k == 0) return 0;
  PDD_REQUIRE(cands && label && groups, "pdd_spg_summarise: null pointer");
  PDD_REQUIRE(((uintptr_t)cands & 15) == 0 && ((uintptr_t)groups & 15) == 0,
              "pdd_spg_summarise: cands and groups must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const unsigned nb = (unsigned)cdiv(k, kSpgThreads);
  const int4* c4 = reinterpret_cast<const int4*>(cands);
  k_spg_sum_init<<<nb, kSpgThreads, 0, st>>>(label, k, reinterpret_cast<int4*>(groups));
  PDD_LAUNCHED();
  k_spg_sum<<<nb, kSpgThreads, 0, st>>>(c4, label, k, groups);
  PDD_LAUNCHED();
  k_spg_sum_final<<<nb, kSpgThreads, 0, st>>>(c4, k, groups);
  PDD_LAUNCHED();
  return 0;
}

}  // extern "C"
