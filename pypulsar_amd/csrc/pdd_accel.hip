// libpdd: acceleration search of a DM-time plane in the Fourier domain -- the
// (r, z) plane of every DM row by direct correlation of the whitened complex
// spectrum with the responses of drifting signals, and its harmonic-stage
// candidate search.  gfx950.
//
// Definitions (restated in tests/accel_oracle.py): the
// whitened spectrum F[d][k], k < nn (0 outside), is correlated with taps
// t[j][phi][e], |e| <= hw_j <= M, built on the host
// (pypulsar_amd/accel.py:template_bank) from the response of a signal that
// drifts z_j bins of 1/T over the observation:
//   A[d][j][i] = sum_e F[d][k0 + e] t[j][phi][e],  k0 = i >> 1, phi = i & 1,
//   P[d][j][i] = |A|^2,  i < ni = 2 nn (half-bin positions r = i / 2).
// z = 0, phi = 0 without zero padding is a delta: P is the whitened power.
// The generalisation to z != 0 of PrestoFFT.interpolate
// (formats/prestofft.py:76-96), whose sinc term is corrected here (§6f).
//
// Kernels:
//   k_acc_correlate  VALU form.  A workgroup takes 512 consecutive k0 of one
//                    row; the window [k0 - M, k0 + 512 + M) is staged in LDS
//                    once and reused by every z and both phi.  Lanes sit on
//                    consecutive k0 (LDS reads of consecutive 8-byte words),
//                    two k0 a thread, 256 apart; the taps are wave-uniform
//                    (scalar loads), each feeding both k0.  Each LDS read of
//                    F feeds a register block of 4 z x 2 phi accumulators: 16
//                    packed (re, im) fused multiply-adds per read, each lane
//                    an explicit fma.  The loop of a z group runs
//                    to the group's own half-width, so zero taps beyond it
//                    are not multiplied.  Fixed order: deterministic.
//   k_acc_search<H>  one launch per stage, compiled per H (1..16).  One
//                    thread per half-bin position i (+ one halo position on
//                    each side of a workgroup) walks the z rows of the plane:
//                    each row of stage sums S_H is exchanged through LDS
//                    once (left and right neighbour), the rows above and
//                    below a cell are kept as three-cell maxima in registers,
//                    candidates leave through one atomic counter.  The
//                    H loads of a sum are independent and added in ascending
//                    h; the plane rows of the harmonics are walked
//                    incrementally (no division per load).
#include <cmath>

#include "pdd_internal.h"

namespace pdd {

namespace {

constexpr int kAccThreads = 256;
constexpr int kAccKB = 2;                  // k0 per thread (kAccThreads apart)
constexpr int kAccTile = kAccKB * kAccThreads;  // k0 per k_acc_correlate workgroup
constexpr int kAccMaxM = 512;              // largest common half-width of the taps
constexpr int kAccZB = 4;                  // z values per register block
constexpr int kAccMaxNz = 255;             // z trials (odd)
constexpr int kAccMaxGroups = (kAccMaxNz + kAccZB - 1) / kAccZB;
constexpr int kAccMaxStages = 8;
constexpr int kAccMaxHarm = 16;
constexpr int kAccSearchTile = kAccThreads - 2;  // positions per k_acc_search workgroup

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct Groups {
  int hw[kAccMaxGroups];  // the largest half-width of each group of kAccZB z values
};

__global__ __launch_bounds__(kAccThreads) void k_acc_correlate(
    const float* __restrict__ spec, int64_t nn, int64_t ld, const float* __restrict__ taps,
    Groups G, int nz, int M, int64_t nblk, float* __restrict__ powers) {
  __shared__ f32x2 sF[kAccTile + 2 * kAccMaxM];
  const int tid = threadIdx.x;
  const int64_t d = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int64_t kfirst = blk * kAccTile;
  const f32x2* row = reinterpret_cast<const f32x2*>(spec) + d * ld;
  // the window [kfirst - M, kfirst + tile + M): bins outside [0, nn) are 0
  for (int t = tid; t < kAccTile + 2 * M; t += kAccThreads) {
    const int64_t k = kfirst - M + t;
    f32x2 v = {0.f, 0.f};
    if (k >= 0 && k < nn) v = row[k];
    sF[t] = v;
  }
  __syncthreads();
  const int64_t ni = 2 * nn;
  const int W = 2 * M + 1;  // taps per (z, phi)
  float* prow = powers + d * (int64_t)nz * ni;
  for (int j0 = 0, g = 0; j0 < nz; j0 += kAccZB, ++g) {
    const int hw = G.hw[g];  // (<= M, checked by the host)
    // the taps of z value u, phase phi: [(j 2 + phi) W + M + e][2]; a z past
    // the last is computed as the last and not stored
    const float* tp[kAccZB];
#pragma unroll
    for (int u = 0; u < kAccZB; ++u)
      tp[u] = taps + ((int64_t)min(j0 + u, nz - 1) * 2 * W + (M - hw)) * 2;
    f32x2 acc[kAccKB][kAccZB][2];  // (re, im) of A at k0 = kfirst + tid + 256 b
#pragma unroll
    for (int b = 0; b < kAccKB; ++b)
#pragma unroll
      for (int u = 0; u < kAccZB; ++u) acc[b][u][0] = acc[b][u][1] = f32x2{0.f, 0.f};
    const f32x2* f = sF + tid + (M - hw);
#pragma unroll 2
    for (int t = 0; t <= 2 * hw; ++t) {
      f32x2 vx[kAccKB], vy[kAccKB];
#pragma unroll
      for (int b = 0; b < kAccKB; ++b) {
        const f32x2 v = f[t + b * kAccThreads];
        vx[b] = f32x2{v.x, v.x};
        vy[b] = f32x2{v.y, v.y};
      }
#pragma unroll
      for (int u = 0; u < kAccZB; ++u) {
#pragma unroll
        for (int phi = 0; phi < 2; ++phi) {
          const float tr = tp[u][(phi * W + t) * 2], ti = tp[u][(phi * W + t) * 2 + 1];
          // (re, im) += v.x (tr, ti), then += v.y (-ti, tr): two packed fused
          // multiply-adds (v_pk_fma_f32 with the taps as a scalar register
          // pair; broadcast and negation are operand modifiers), each lane
          // an explicit fma -- the library is built with -ffp-contract=off
#pragma unroll
          for (int b = 0; b < kAccKB; ++b) {
            acc[b][u][phi] = __builtin_elementwise_fma(vx[b], f32x2{tr, ti}, acc[b][u][phi]);
            acc[b][u][phi] = __builtin_elementwise_fma(vy[b], f32x2{-ti, tr}, acc[b][u][phi]);
          }
        }
      }
    }
#pragma unroll
    for (int b = 0; b < kAccKB; ++b) {
      const int64_t k0 = kfirst + tid + b * kAccThreads;
      if (k0 < nn) {
#pragma unroll
        for (int u = 0; u < kAccZB; ++u) {
          if (j0 + u < nz) {
            f32x2 p;
            p.x = acc[b][u][0].x * acc[b][u][0].x + acc[b][u][0].y * acc[b][u][0].y;
            p.y = acc[b][u][1].x * acc[b][u][1].x + acc[b][u][1].y * acc[b][u][1].y;
            *reinterpret_cast<f32x2*>(prow + (int64_t)(j0 + u) * ni + 2 * k0) = p;
          }
        }
      }
    }
  }
}

// One stage of the search, H a compile-time constant (its divisions are
// multiplications and its loops straight-line code); one launch per stage.
// Thread t of workgroup blk holds position i = 2 H rlo + blk * 254 - 1 + t:
// threads 1..254 own a position, threads 0 and 255 are the neighbours of the
// first and the last.
//
// Columns: col[h - 1] = (i h + H / 2) / H does not depend on the z row; exact
// in 32 bits through i = H q + r:  q h + (r h + H / 2) / H  (<= i < 2^31; the
// product i h needs 64 bits).
// Rows: fl[h - 1] = floor(((j - J0) h + H / 2) / H) with its remainder, walked
// from j = 0 by adding h (h <= H: at most one carry a row); uniform over the
// workgroup (scalar registers).
// S_H = the sum over h = 1..H, float32 in ascending h from the h = 1 term, of
// P[J0 + fl[h - 1]][col[h - 1]]; the H loads are independent.
//
// Row j + 1 of S is exchanged through sh[j & 1] (one write, one barrier, two
// reads: the neighbours); the rows j - 1 and j are kept in registers.  The
// buffer a thread writes in iteration j + 2 was read in iteration j, before
// the barrier of iteration j + 1.
template <int H>
__global__ __launch_bounds__(kAccThreads) void k_acc_search(
    const float* __restrict__ powers, int nz, int64_t ni, float thr, int64_t rlo, int64_t nblk,
    int32_t* __restrict__ cands, int64_t max_cands, unsigned long long* __restrict__ count) {
  __shared__ float sh[2][kAccThreads];
  const int tid = threadIdx.x;
  const int64_t d = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int64_t ilo = 2 * (int64_t)H * rlo;  // stage H searches [ilo, ni)
  const int64_t i = ilo + blk * kAccSearchTile - 1 + tid;
  const float* P = powers + d * (int64_t)nz * ni;
  const bool owner = tid >= 1 && tid <= kAccSearchTile;
  const bool in = i >= ilo && i < ni;
  const int J0 = (nz - 1) / 2;
  const uint32_t iu = in ? (uint32_t)i : 0u;
  const uint32_t cq = iu / (uint32_t)H, cr = iu % (uint32_t)H;
  int32_t col[H];
  int fl[H], rem[H];
#pragma unroll
  for (int q = 0; q < H; ++q) {
    const uint32_t h = q + 1;
    col[q] = (int32_t)(cq * h + (cr * h + (uint32_t)(H / 2)) / (uint32_t)H);
    const int num = -J0 * (q + 1) + H / 2;  // z row 0: jc = -J0
    const int f0 = num >= 0 ? num / H : -((-num + H - 1) / H);  // floor division
    fl[q] = f0;
    rem[q] = num - f0 * H;
  }
  auto stage_sum = [&]() {
    float v[H];
#pragma unroll
    for (int q = 0; q < H; ++q) v[q] = P[(int64_t)(J0 + fl[q]) * ni + col[q]];
    float s = v[0];
#pragma unroll
    for (int q = 1; q < H; ++q) s += v[q];
    return s;
  };
  // Rolling registers: of z row j - 1 the largest of the three neighbours
  // above (m_prev), of row j the cell and its two neighbours, of row j + 1
  // (just exchanged through LDS) the largest of the three below.
  const int tl = max(tid - 1, 0), tr = min(tid + 1, kAccThreads - 1);  // (halo threads: unused)
  float s = in ? stage_sum() : -INFINITY;
  sh[1][tid] = s;
  __syncthreads();
  float s_l = sh[1][tl], s_r = sh[1][tr];
  float m_prev = -INFINITY;
#pragma unroll 1
  for (int j = 0; j < nz; ++j) {
#pragma unroll
    for (int q = 0; q < H; ++q) {  // the rows of z row j + 1
      rem[q] += q + 1;
      if (rem[q] >= H) {
        rem[q] -= H;
        fl[q] += 1;
      }
    }
    // (past the last z row nothing is read)
    const float n_c = (in && j + 1 < nz) ? stage_sum() : -INFINITY;
    float* buf = sh[j & 1];  // (row j + 1; row j's buffer sh[(j + 1) & 1] is still being read)
    buf[tid] = n_c;
    __syncthreads();
    const float n_l = buf[tl], n_r = buf[tr];
    const float m_next = fmaxf(fmaxf(n_l, n_c), n_r);
    const bool hit = (s >= thr) & (s > s_l) & (s > m_prev) & (s >= s_r) & (s >= m_next);
    if (in && owner && hit) {
      const unsigned long long slot = atomicAdd(count, 1ull);
      if ((int64_t)slot < max_cands) {
        int32_t* c = cands + slot * 6;
        c[0] = (int32_t)d;
        c[1] = (int32_t)i;
        c[2] = j - J0;
        c[3] = H;
        c[4] = __float_as_int(s);
        c[5] = 0;
      }
    }
    m_prev = fmaxf(fmaxf(s_l, s), s_r);
    s = n_c;
    s_l = n_l;
    s_r = n_r;
  }
}

typedef void (*AccSearchKernel)(const float*, int, int64_t, float, int64_t, int64_t, int32_t*,
                                int64_t, unsigned long long*);
#define PDD_ACC_K(h) k_acc_search<h>
const AccSearchKernel kAccSearch[kAccMaxHarm] = {
    PDD_ACC_K(1),  PDD_ACC_K(2),  PDD_ACC_K(3),  PDD_ACC_K(4),  PDD_ACC_K(5),  PDD_ACC_K(6),
    PDD_ACC_K(7),  PDD_ACC_K(8),  PDD_ACC_K(9),  PDD_ACC_K(10), PDD_ACC_K(11), PDD_ACC_K(12),
    PDD_ACC_K(13), PDD_ACC_K(14), PDD_ACC_K(15), PDD_ACC_K(16)};
#undef PDD_ACC_K

}  // namespace

}  // namespace pdd

using namespace pdd;

extern "C" {

int pdd_acc_correlate(const float* spec, int64_t D, int64_t nn, int64_t ld, const float* taps,
                      const int32_t* hw, int nz, int M, float* powers, void* stream) {
  PDD_REQUIRE(spec && taps && hw && powers, "pdd_acc_correlate: null pointer");
  PDD_REQUIRE(D >= 0 && nn > 0 && ld >= nn && nn < (1ll << 30), "pdd_acc_correlate: bad shape");
  PDD_REQUIRE(nz >= 1 && nz <= kAccMaxNz && (nz & 1), "pdd_acc_correlate: nz must be odd, 1..%d",
              kAccMaxNz);
  PDD_REQUIRE(M >= 0 && M <= kAccMaxM, "pdd_acc_correlate: M out of range 0..%d", kAccMaxM);
  PDD_REQUIRE(((uintptr_t)spec & 7) == 0 && ((uintptr_t)powers & 7) == 0,
              "pdd_acc_correlate: spec and powers must be 8-byte aligned");
  Groups G;
  for (int g = 0; g < kAccMaxGroups; ++g) G.hw[g] = 0;
  for (int j = 0; j < nz; ++j) {
    PDD_REQUIRE(hw[j] >= 0 && hw[j] <= M, "pdd_acc_correlate: half-width %d outside 0..M=%d",
                hw[j], M);
    if (hw[j] > G.hw[j / kAccZB]) G.hw[j / kAccZB] = hw[j];
  }
  const int64_t nblk = cdiv(nn, kAccTile);
  PDD_REQUIRE(D * nblk < (1ll << 31), "pdd_acc_correlate: too large");
  if (D == 0) return 0;
  k_acc_correlate<<<(unsigned)(D * nblk), kAccThreads, 0, as_stream(stream)>>>(
      spec, nn, ld, taps, G, nz, M, nblk, powers);
  PDD_LAUNCHED();
  return 0;
}

int pdd_acc_search(const float* powers, int64_t D, int nz, int64_t ni, const int32_t* harms,
                   int n_harms, const float* thr, int64_t rlo, int32_t* cands, int64_t max_cands,
                   unsigned long long* count, void* stream) {
  PDD_REQUIRE(powers && harms && thr && count && (cands || max_cands == 0),
              "pdd_acc_search: null pointer");
  PDD_REQUIRE(D >= 0 && ni > 0 && ni < (1ll << 31) && max_cands >= 0,
              "pdd_acc_search: bad shape");
  PDD_REQUIRE(nz >= 1 && nz <= kAccMaxNz && (nz & 1), "pdd_acc_search: nz must be odd, 1..%d",
              kAccMaxNz);
  PDD_REQUIRE(rlo >= 1, "pdd_acc_search: rlo must be >= 1");
  PDD_REQUIRE(n_harms >= 1 && n_harms <= kAccMaxStages, "pdd_acc_search: 1..%d stages",
              kAccMaxStages);
  for (int i = 0; i < n_harms; ++i) {
    PDD_REQUIRE(harms[i] >= 1 && harms[i] <= kAccMaxHarm,
                "pdd_acc_search: harmonic count %d out of range 1..%d", harms[i], kAccMaxHarm);
    PDD_REQUIRE(i == 0 || harms[i] > harms[i - 1], "pdd_acc_search: harms must ascend");
  }
  PDD_REQUIRE(D * cdiv(ni, kAccSearchTile) < (1ll << 31), "pdd_acc_search: too large");
  if (D == 0) return 0;
  for (int i = 0; i < n_harms; ++i) {
    const int64_t ilo = 2 * (int64_t)harms[i] * rlo;  // stage H searches [ilo, ni)
    if (ilo >= ni) break;  // (and for every later stage)
    const int64_t nblk = cdiv(ni - ilo, kAccSearchTile);
    kAccSearch[harms[i] - 1]<<<(unsigned)(D * nblk), kAccThreads, 0, as_stream(stream)>>>(
        powers, nz, ni, thr[i], rlo, nblk, cands, max_cands, count);
    PDD_LAUNCHED();
  }
  return 0;
}

}  // extern "C"
