// libpdd: the jerk search -- harmonic stages and candidates of the (r, z, w)
// volume of every DM row.  gfx950.
//
// Definitions (restated in tests/jerk_oracle.py): the volume
// P[l][d][j][i], float32 [nw][D][nz][ni], holds for every jerk w_l = (l - L0)
// dw the plane pdd_acc_correlate writes with that slab's taps
// (pypulsar_amd/jerk.py:template_bank).  Stage H sums harmonics on the TOP
// harmonic's grid, §6f's rule in both template axes (lc = l - L0, jc = j - J0):
//   S_H[l][j][i] = sum_{h=1..H} P[L0 + floor((lc h + H/2) / H)][d]
//                                [J0 + floor((jc h + H/2) / H)][(i h + H/2) / H]
// float32, ascending h from the h = 1 term.  A cell with i >= 2 H rlo is a
// candidate when S >= thr, S > the 13 of its 26 neighbours that precede it in
// (l, j, i) order and S >= the 13 that follow; outside the volume or the
// searched range counts as -inf.
//
// Kernel: k_jerk_step<H>, compiled per H (1..16); a stage is nw + 1 launches
// in stream order over a ring of three S_H slabs [D][nz][ni] in the caller's
// scratch.  Launch s = -1 .. nw - 1 computes slab s + 1 of S_H (every sum
// once; written to ring slot (s + 1) % 3 and kept in registers) and judges
// slab s from it and the slabs s and s - 1 read back from the ring.  (H = 1,
// where S_1 is the volume itself: nothing is written, the slabs s and s - 1
// are read from the volume.)  As in
// k_acc_search<H> (pdd_accel.hip): one thread per half-bin position i, plus a
// halo position on each side of a workgroup; columns exact in 32 bits, once;
// the harmonic z rows walked incrementally with workgroup-uniform remainders
// (the w slab of a harmonic is fixed for a launch: one uniform floor each at
// its start); the H loads of a sum independent, added in ascending h.  A row of
// the three slabs is exchanged through LDS once (one barrier): of the slabs s
// - 1 and s + 1 the three-cell maxima of the rows j - 1, j, j + 1 are kept in
// registers, of slab s what k_acc_search keeps.  The only atomic is the
// candidate counter.
#include <cmath>

#include "pdd_internal.h"

namespace pdd {

namespace {

constexpr int kJrkThreads = 256;
constexpr int kJrkTile = kJrkThreads - 2;  // positions per workgroup
constexpr int kJrkMaxNw = 63;              // w trials (odd)
constexpr int kJrkMaxNz = 255;             // z trials (odd; kAccMaxNz)
constexpr int kJrkMaxStages = 8;
constexpr int kJrkMaxHarm = 16;

// Thread t of workgroup blk holds position i = 2 H rlo + blk * 254 - 1 + t:
// threads 1..254 own it (they store its S and report it), threads 0 and 255
// are the neighbours of the first and the last.  s: the judged slab (-1: none
// yet); slab s + 1 is computed while s + 1 < nw.  ring_prev / ring_cur /
// ring_next: the ring slots of the slabs s - 1, s and s + 1 ([D][nz][ni]
// each); a slot is read only where an earlier launch of this stage wrote it
// (positions in [2 H rlo, ni) of a slab inside the volume).  H = 1: S_1 is
// the volume itself -- nothing is stored, ring_prev and ring_cur are the
// slabs s - 1 and s of the volume.
//
// sh[j & 1][0..2]: row j + 1 of the slabs s - 1, s, s + 1.  The buffer a
// thread writes in iteration j + 2 was read in iteration j, before the
// barrier of iteration j + 1.
template <int H>
__global__ __launch_bounds__(kJrkThreads) void k_jerk_step(
    const float* __restrict__ vol, int64_t D, int nw, int nz, int64_t ni, int s, float thr,
    int64_t rlo, int64_t nblk, const float* __restrict__ ring_prev,
    const float* __restrict__ ring_cur, float* __restrict__ ring_next,
    int32_t* __restrict__ cands, int64_t max_cands, unsigned long long* __restrict__ count) {
  __shared__ float sh[2][3][kJrkThreads];
  const int tid = threadIdx.x;
  const int64_t d = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int64_t ilo = 2 * (int64_t)H * rlo;  // stage H searches [ilo, ni)
  const int64_t i = ilo + blk * kJrkTile - 1 + tid;
  const bool owner = tid >= 1 && tid <= kJrkTile;
  const bool in = i >= ilo && i < ni;
  const int J0 = (nz - 1) / 2, L0 = (nw - 1) / 2;
  const bool have_prev = s >= 1, have_cur = s >= 0, have_next = s + 1 < nw;
  const int64_t slab = (int64_t)nz * ni;  // floats of one row's plane
  const uint32_t iu = in ? (uint32_t)i : 0u;
  const uint32_t cq = iu / (uint32_t)H, cr = iu % (uint32_t)H;
  int32_t col[H];
  int rem[H];
  const float* hp[H];  // harmonic q + 1: its z row of its slab of this DM row (uniform)
  const int lc = s + 1 - L0;
#pragma unroll
  for (int q = 0; q < H; ++q) {
    const uint32_t h = q + 1;
    col[q] = (int32_t)(cq * h + (cr * h + (uint32_t)(H / 2)) / (uint32_t)H);
    const int num = -J0 * (q + 1) + H / 2;  // z row 0: jc = -J0
    const int f0 = num >= 0 ? num / H : -((-num + H - 1) / H);  // floor division
    rem[q] = num - f0 * H;
    const int lnum = lc * (q + 1) + H / 2;
    const int lf = lnum >= 0 ? lnum / H : -((-lnum + H - 1) / H);
    // (no slab to compute: the pointer is not used)
    hp[q] = vol + (have_next ? ((int64_t)(L0 + lf) * D + d) * slab + (int64_t)(J0 + f0) * ni : 0);
  }
  auto stage_sum = [&]() {
    float v[H];
#pragma unroll
    for (int q = 0; q < H; ++q) v[q] = hp[q][col[q]];
    float a = v[0];
#pragma unroll
    for (int q = 1; q < H; ++q) a += v[q];
    return a;
  };
  const float* rp = ring_prev + d * slab + (in ? i : 0);
  const float* rc = ring_cur + d * slab + (in ? i : 0);
  float* rn = ring_next + d * slab + (in ? i : 0);
  const int tl = max(tid - 1, 0), tr = min(tid + 1, kJrkThreads - 1);  // (halo threads: unused)
  // z row 0 of the three slabs
  float p_c = (in && have_prev) ? rp[0] : -INFINITY;
  float c_c = (in && have_cur) ? rc[0] : -INFINITY;
  float n_c = -INFINITY;
  if (in && have_next) {
    n_c = stage_sum();
    if (H > 1 && owner) rn[0] = n_c;
  }
  sh[1][0][tid] = p_c;
  sh[1][1][tid] = c_c;
  sh[1][2][tid] = n_c;
  __syncthreads();
  // Rolling registers.  Slab s: the cell and its two neighbours of row j, the
  // three-cell maximum of row j - 1.  Slabs s - 1 and s + 1: the three-cell
  // maxima of rows j - 1 and j.
  float c_l = sh[1][1][tl], c_r = sh[1][1][tr];
  float pm_cur = fmaxf(fmaxf(sh[1][0][tl], p_c), sh[1][0][tr]);
  float nm_cur = fmaxf(fmaxf(sh[1][2][tl], n_c), sh[1][2][tr]);
  float cm_prev = -INFINITY, pm_prev = -INFINITY, nm_prev = -INFINITY;
#pragma unroll 1
  for (int j = 0; j < nz; ++j) {
#pragma unroll
    for (int q = 0; q < H; ++q) {  // the rows of z row j + 1
      rem[q] += q + 1;
      if (rem[q] >= H) {
        rem[q] -= H;
        hp[q] += ni;
      }
    }
    // (past the last z row nothing is read)
    const bool more = in && j + 1 < nz;
    const int64_t o = (int64_t)(j + 1) * ni;
    const float p_n = (more && have_prev) ? rp[o] : -INFINITY;
    const float c_n = (more && have_cur) ? rc[o] : -INFINITY;
    float n_n = -INFINITY;
    if (more && have_next) {
      n_n = stage_sum();
      if (H > 1 && owner) rn[o] = n_n;
    }
    float(*buf)[kJrkThreads] = sh[j & 1];  // (row j's buffers sh[(j + 1) & 1] are still being read)
    buf[0][tid] = p_n;
    buf[1][tid] = c_n;
    buf[2][tid] = n_n;
    __syncthreads();
    const float cn_l = buf[1][tl], cn_r = buf[1][tr];
    const float pm_next = fmaxf(fmaxf(buf[0][tl], p_n), buf[0][tr]);
    const float cm_next = fmaxf(fmaxf(cn_l, c_n), cn_r);
    const float nm_next = fmaxf(fmaxf(buf[2][tl], n_n), buf[2][tr]);
    const float before = fmaxf(fmaxf(fmaxf(pm_prev, pm_cur), pm_next), fmaxf(cm_prev, c_l));
    const float after = fmaxf(fmaxf(fmaxf(nm_prev, nm_cur), nm_next), fmaxf(cm_next, c_r));
    const bool hit = (c_c >= thr) & (c_c > before) & (c_c >= after);
    if (in && owner && have_cur && hit) {
      const unsigned long long slot = atomicAdd(count, 1ull);
      if ((int64_t)slot < max_cands) {
        int32_t* c = cands + slot * 8;
        c[0] = (int32_t)d;
        c[1] = (int32_t)i;
        c[2] = j - J0;
        c[3] = s - L0;
        c[4] = H;
        c[5] = __float_as_int(c_c);
        c[6] = 0;
        c[7] = 0;
      }
    }
    cm_prev = fmaxf(fmaxf(c_l, c_c), c_r);
    c_c = c_n;
    c_l = cn_l;
    c_r = cn_r;
    pm_prev = pm_cur;
    pm_cur = pm_next;
    nm_prev = nm_cur;
    nm_cur = nm_next;
  }
}

typedef void (*JerkStepKernel)(const float*, int64_t, int, int, int64_t, int, float, int64_t,
                               int64_t, const float*, const float*, float*, int32_t*, int64_t,
                               unsigned long long*);
#define PDD_JRK_K(h) k_jerk_step<h>
const JerkStepKernel kJerkStep[kJrkMaxHarm] = {
    PDD_JRK_K(1),  PDD_JRK_K(2),  PDD_JRK_K(3),  PDD_JRK_K(4),  PDD_JRK_K(5),  PDD_JRK_K(6),
    PDD_JRK_K(7),  PDD_JRK_K(8),  PDD_JRK_K(9),  PDD_JRK_K(10), PDD_JRK_K(11), PDD_JRK_K(12),
    PDD_JRK_K(13), PDD_JRK_K(14), PDD_JRK_K(15), PDD_JRK_K(16)};
#undef PDD_JRK_K

}  // namespace

}  // namespace pdd

using namespace pdd;

extern "C" {

int pdd_jerk_search(const float* vol, int64_t D, int nw, int nz, int64_t ni, const int32_t* harms,
                    int n_harms, const float* thr, int64_t rlo, float* scratch,
                    int64_t scratch_floats, int32_t* cands, int64_t max_cands,
                    unsigned long long* count, void* stream) {
  PDD_REQUIRE(vol && harms && thr && count && scratch && (cands || max_cands == 0),
              "pdd_jerk_search: null pointer");
  PDD_REQUIRE(D >= 0 && ni > 0 && ni < (1ll << 31) && max_cands >= 0,
              "pdd_jerk_search: bad shape");
  PDD_REQUIRE(nw >= 1 && nw <= kJrkMaxNw && (nw & 1), "pdd_jerk_search: nw must be odd, 1..%d",
              kJrkMaxNw);
  PDD_REQUIRE(nz >= 1 && nz <= kJrkMaxNz && (nz & 1), "pdd_jerk_search: nz must be odd, 1..%d",
              kJrkMaxNz);
  PDD_REQUIRE(rlo >= 1, "pdd_jerk_search: rlo must be >= 1");
  PDD_REQUIRE(n_harms >= 1 && n_harms <= kJrkMaxStages, "pdd_jerk_search: 1..%d stages",
              kJrkMaxStages);
  for (int i = 0; i < n_harms; ++i) {
    PDD_REQUIRE(harms[i] >= 1 && harms[i] <= kJrkMaxHarm,
                "pdd_jerk_search: harmonic count %d out of range 1..%d", harms[i], kJrkMaxHarm);
    PDD_REQUIRE(i == 0 || harms[i] > harms[i - 1], "pdd_jerk_search: harms must ascend");
  }
  PDD_REQUIRE(D * cdiv(ni, kJrkTile) < (1ll << 31) && D < (1ll << 31),
              "pdd_jerk_search: too large");
  const int64_t slab = D * (int64_t)nz * ni;  // floats of one S_H slab (D ni < 2^39: < 2^47)
  PDD_REQUIRE(scratch_floats >= 3 * slab,
              "pdd_jerk_search: scratch of %lld floats, 3 D nz ni = %lld needed",
              (long long)scratch_floats, (long long)(3 * slab));
  if (D == 0) return 0;
  for (int i = 0; i < n_harms; ++i) {
    const int64_t ilo = 2 * (int64_t)harms[i] * rlo;  // stage H searches [ilo, ni)
    if (ilo >= ni) break;  // (and for every later stage)
    const int64_t nblk = cdiv(ni - ilo, kJrkTile);
    for (int s = -1; s < nw; ++s) {
      // ring slots of the slabs s - 1, s, s + 1 (slot = slab % 3); H = 1: the
      // slabs of the volume themselves (next is not written)
      const bool ring = harms[i] > 1;
      const float* prev = ring ? scratch + ((s + 2) % 3) * slab : vol + max(s - 1, 0) * slab;
      const float* cur = ring ? scratch + ((s + 3) % 3) * slab : vol + max(s, 0) * slab;
      float* next = scratch + ((s + 1) % 3) * slab;
      kJerkStep[harms[i] - 1]<<<(unsigned)(D * nblk), kJrkThreads, 0, as_stream(stream)>>>(
          vol, D, nw, nz, ni, s, thr[i], rlo, nblk, prev, cur, next, cands, max_cands, count);
      PDD_LAUNCHED();
    }
  }
  return 0;
}

}  // extern "C"
