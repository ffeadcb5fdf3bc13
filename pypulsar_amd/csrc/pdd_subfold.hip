// libpdd: folding of periodicity candidates from the raw file-order block into
// (sub-integration, subband, phase) cubes, and the DM refinement on such a
// cube.  gfx950.
//
// New (the reference has no subband fold; PRESTO's prepfold draws this panel).
// The arithmetic is stated in include/pdd.h and restated by brute force in
// tests/subfold_oracle.py.  The phase model is pdd_fold_rows' (pdd_fold.hip):
// dedispersed sample i has P_i = P0 + i step + (i (i - 1) / 2) accel (mod 2^64)
// and falls into bin ((P_i >> 32) * nbins) >> 32, whatever its channel.
//
// Kernels:
//   k_subfold     one workgroup per (job, part, slice of <= 4096 dedispersed
//                 samples, tile of 64 lanes' channels).  A lane owns one
//                 channel, or four adjacent ones of the same subband, and
//                 walks CONSECUTIVE dedispersed samples i, reading row
//                 i + b[c] of its channels: the lanes of a wave sit on
//                 adjacent channels, so a wave's loads cover adjacent bytes of
//                 a few neighbouring rows.  The four quarters of the slice
//                 are walked by the workgroup's four waves.  Every lane of a wave
//                 is at the same sample, so the bin is wave-uniform; a lane
//                 keeps the running sum of the current bin in a register and
//                 adds it to the workgroup's LDS histogram [bin][lane] only
//                 when the bin changes (lane-consecutive addresses: no bank
//                 conflict, no contention inside a wave).  At the end the
//                 lanes of each subband are summed and every non-empty
//                 (subband, bin) cell goes to the cube with one global
//                 atomic; channel sums and squares cost one atomic a lane.
//                 8-bit input accumulates in integers up to that atomic (the
//                 float64 adds of integers below 2^53 are exact in any order).
//                 Loads: 8-bit blocks whose rows are 4-byte aligned (x, ld and
//                 C multiples of 4) take one channel a lane and stage chunks
//                 of 256 dedispersed samples: the raw rows [i + bmin, i + 256
//                 + bmax) of the tile's 64 channels go to LDS with coalesced
//                 4-byte loads and a lane reads its channel back at row
//                 k + b[c] - bmin.  A tile whose delays span more rows than
//                 the staging holds (960 less the chunk), unaligned blocks
//                 and float32 input read per lane, 8 rows in flight.
//   k_subfold_dm  one workgroup per job: parts collapsed by the trial's
//                 shifts into LDS, subband statistics from the channel
//                 statistics, ladder entries spread over the waves with lanes
//                 across bins, every sum in the order the header states.
#include <algorithm>

#include "pdd_internal.h"

namespace pdd {

namespace {

constexpr int kSfThreads = 256;
constexpr int kSfWaves = kSfThreads / 64;
constexpr int kSfSlice = 4096;     // dedispersed samples per workgroup
constexpr int kSfUnroll = 8;       // rows a lane has in flight per channel
constexpr int kSfChunk = 256;      // dedispersed samples staged at once
constexpr int kSfStageRows = 960;  // most raw rows of a staged chunk (64 bytes each)
constexpr int kSfMaxBins = 256;
constexpr int kSfMaxPart = 128;
constexpr int kSfMaxCells = 8192;
constexpr int kSfMaxDm = 1024;
constexpr int kSfJob = 8;          // int64 words of a job

template <typename T>
struct SfTypes;
template <>
struct SfTypes<uint8_t> {
  using val_t = uint32_t;   // a sample
  using run_t = uint32_t;   // a lane's sums over <= kSfSlice / kSfWaves samples of 4 channels
  using sq_t = uint64_t;
  using hist_t = uint32_t;  // a workgroup's cell: <= kSfSlice * 4 * 255
  using cell_t = uint64_t;  // 64 lanes of them
};
template <>
struct SfTypes<float> {
  using val_t = double;
  using run_t = double;
  using sq_t = double;
  using hist_t = double;
  using cell_t = double;
};

template <typename T, int CPL, bool STAGE>
__global__ __launch_bounds__(kSfThreads) void k_subfold(
    const T* __restrict__ x, int64_t n, int64_t C, int64_t ld, int64_t t_first,
    const int64_t* __restrict__ jobs, const int32_t* __restrict__ table, int npart, int nsub,
    int nbins, int nslice, int ntile, int stage_rows, double* __restrict__ cube, int32_t* __restrict__ cnt,
    double* __restrict__ chansum, double* __restrict__ chansq) {
  using TY = SfTypes<T>;
  using val_t = typename TY::val_t;
  using run_t = typename TY::run_t;
  using sq_t = typename TY::sq_t;
  using hist_t = typename TY::hist_t;
  using cell_t = typename TY::cell_t;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  hist_t* hist = reinterpret_cast<hist_t*>(smem);                      // [nbins][64]
  int* hc = reinterpret_cast<int*>(hist + (size_t)nbins * 64);         // [nbins]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  int64_t blk = blockIdx.x;
  const int tile = (int)(blk % ntile);
  blk /= ntile;
  const int slice = (int)(blk % nslice);
  blk /= nslice;
  const int part = (int)(blk % npart);
  const int64_t j = blk / npart;
  const int64_t* jb = jobs + kSfJob * j;
  const uint64_t P0 = (uint64_t)jb[0], step = (uint64_t)jb[1], accel = (uint64_t)jb[2];
  const int64_t L = jb[3], i0 = jb[4], i1 = jb[5], trow = jb[6];
  // the workgroup's dedispersed samples [a, e): its slice of the part, cut to the call's range
  const int64_t pbeg = (int64_t)part * L;
  const int64_t a = max(i0, pbeg + (int64_t)slice * kSfSlice);
  const int64_t e = min(i1, pbeg + min(L, (int64_t)(slice + 1) * kSfSlice));
  if (a >= e) return;  // (uniform over the workgroup)
  for (int t = tid; t < nbins * 64; t += kSfThreads) hist[t] = hist_t(0);
  for (int t = tid; t < nbins; t += kSfThreads) hc[t] = 0;
  __syncthreads();

  const int64_t per = (e - a + kSfWaves - 1) / kSfWaves;
  const int64_t wa = a + (int64_t)wv * per;
  const int len = (int)max((int64_t)0, min(e, wa + per) - wa);  // <= kSfSlice / kSfWaves
  const int64_t c0 = ((int64_t)tile * 64 + lane) * CPL;
  // Per channel the element offset of its row of sample wa and the steps
  // [klo, khi) whose row lies inside the block: every load is guarded.
  int64_t off[CPL];
  int klo[CPL], khi[CPL];
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int64_t c = c0 + q;
    off[q] = 0;
    klo[q] = 1;
    khi[q] = 0;
    if (c < C) {
      const int64_t r0 = wa + (int64_t)table[trow * C + c] - t_first;  // row of sample wa
      off[q] = r0 * ld + c;
      klo[q] = (int)min((int64_t)len, max((int64_t)0, -r0));
      khi[q] = (int)max((int64_t)0, min((int64_t)len, n - r0));
    }
  }
  run_t run = run_t(0), cs[CPL];
  sq_t cq[CPL];
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    cs[q] = run_t(0);
    cq[q] = sq_t(0);
  }
  int runc = 0, runbin = -1;
  const uint64_t nb = (uint64_t)nbins;
  // one dedispersed sample of the lane's channels; the bin is wave-uniform
  auto consume = [&](const val_t* v, uint64_t& P, uint64_t& d) {
    const int bin = (int)(((P >> 32) * nb) >> 32);
    if (bin != runbin) {
      if (runc) {
        atomicAdd(&hist[runbin * 64 + lane], run);
        if (tile == 0 && lane == 0) atomicAdd(&hc[runbin], runc);
      }
      runbin = bin;
      run = run_t(0);
      runc = 0;
    }
#pragma unroll
    for (int q = 0; q < CPL; ++q) {
      run += v[q];
      cs[q] += v[q];
      cq[q] += (sq_t)v[q] * (sq_t)v[q];
    }
    runc += 1;
    P += d;
    d += accel;
  };
  bool staged = false;
  if constexpr (STAGE) {
    // 8-bit input, one channel a lane, x, ld and C multiples of 4: where the
    // delays of the tile's 64 channels span few enough rows, chunks of the raw
    // rows are staged in LDS with coalesced 4-byte loads (16 lanes a row
    // segment) and each lane reads its channel back at row k + b[c] - bmin.
    uint32_t* stage32 = reinterpret_cast<uint32_t*>(hc + nbins);  // [stage_rows][16]
    const unsigned char* stage8 = reinterpret_cast<const unsigned char*>(stage32);
    const bool have = c0 < C;
    const int bc = have ? table[trow * C + c0] : 0;
    int lo = have ? bc : 0x7fffffff, hi = have ? bc : -0x7fffffff - 1;
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, __shfl_xor(lo, o));
      hi = max(hi, __shfl_xor(hi, o));
    }
    const int64_t span = (int64_t)hi - lo;  // (the same in every wave of the workgroup)
    if (span >= 0 && kSfChunk + span <= stage_rows) {
      staged = true;
      const int rel = have ? bc - lo : 0;
      const int64_t tc = (int64_t)tile * 64;
      for (int64_t ca = a; ca < e; ca += kSfChunk) {  // (uniform trip count)
        const int m = (int)min((int64_t)kSfChunk, e - ca);
        const int64_t r0 = ca + lo - t_first;          // block row of the first staged row
        const int nd = (m + (int)span) * 16;           // <= stage_rows * 16
#pragma unroll 4
        for (int idx = tid; idx < nd; idx += kSfThreads) {
          const int64_t row = r0 + (idx >> 4);
          const int64_t c = tc + ((idx & 15) << 2);
          uint32_t w = 0;
          if (row >= 0 && row < n && c < C)            // (C % 4 == 0: c + 3 < C)
            w = *reinterpret_cast<const uint32_t*>(x + row * ld + c);
          stage32[idx] = w;
        }
        __syncthreads();
        const int k0 = wv * (kSfChunk / kSfWaves), k1 = min(m, k0 + kSfChunk / kSfWaves);
        if (k0 < k1) {
          const uint64_t i = (uint64_t)(ca + k0);
          const uint64_t tri = i == 0 ? 0 : (i * (i - 1)) >> 1;
          uint64_t P = P0 + i * step + tri * accel;
          uint64_t d = step + i * accel;
          for (int k = k0; k < k1; k += kSfUnroll) {
            val_t v[kSfUnroll];
#pragma unroll
            for (int u = 0; u < kSfUnroll; ++u)
              v[u] = k + u < k1 ? (val_t)stage8[(k + u + rel) * 64 + lane] : val_t(0);
#pragma unroll
            for (int u = 0; u < kSfUnroll; ++u)
              if (k + u < k1) consume(&v[u], P, d);
          }
        }
        __syncthreads();
      }
    }
  }
  if (!staged && len > 0) {  // (uniform over the wave)
    const uint64_t i = (uint64_t)wa;  // < 2^31
    const uint64_t tri = i == 0 ? 0 : (i * (i - 1)) >> 1;
    uint64_t P = P0 + i * step + tri * accel;
    uint64_t d = step + i * accel;  // P_{i+1} - P_i
    for (int k = 0; k < len; k += kSfUnroll) {
      val_t v[kSfUnroll][CPL];
#pragma unroll
      for (int u = 0; u < kSfUnroll; ++u) {
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
          const int kk = k + u;
          v[u][q] = (kk >= klo[q] && kk < khi[q]) ? (val_t)x[off[q] + (int64_t)kk * ld] : val_t(0);
        }
      }
#pragma unroll
      for (int u = 0; u < kSfUnroll; ++u)
        if (k + u < len) consume(v[u], P, d);
    }
  }
  if (runc) {
    atomicAdd(&hist[runbin * 64 + lane], run);
    if (tile == 0 && lane == 0) atomicAdd(&hc[runbin], runc);
  }
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    if (c0 + q < C) {
      atomicAdd(&chansum[j * C + c0 + q], (double)cs[q]);
      atomicAdd(&chansq[j * C + c0 + q], (double)cq[q]);
    }
  }
  __syncthreads();
  // the lanes of each subband of the tile, summed; one atomic per non-empty cell
  const int64_t cps = C / nsub;
  const int64_t tc0 = (int64_t)tile * 64 * CPL, tc1 = min(C, tc0 + 64 * CPL);
  const int64_t s_lo = tc0 / cps, s_hi = (tc1 - 1) / cps;
  const int ncell = (int)(s_hi - s_lo + 1) * nbins;
  for (int t = tid; t < ncell; t += kSfThreads) {
    const int64_t s = s_lo + t / nbins;
    const int b = t % nbins;
    const int l0 = (int)((max(tc0, s * cps) - tc0) / CPL);
    const int l1 = (int)((min(tc1, (s + 1) * cps) - tc0 + CPL - 1) / CPL);
    cell_t sum = cell_t(0);
    for (int l = l0; l < l1; ++l) sum += (cell_t)hist[b * 64 + l];
    if (sum != cell_t(0))
      atomicAdd(&cube[((j * npart + part) * nsub + s) * nbins + b], (double)sum);
  }
  if (tile == 0) {
    for (int b = tid; b < nbins; b += kSfThreads)
      if (hc[b]) atomicAdd(&cnt[(j * npart + part) * nbins + b], hc[b]);
  }
}

// The outputs of k_subfold start from zero (one launch for the four).
__global__ __launch_bounds__(kSfThreads) void k_subfold_zero(double* __restrict__ cube,
                                                             int32_t* __restrict__ cnt,
                                                             double* __restrict__ chansum,
                                                             double* __restrict__ chansq,
                                                             int64_t ncube, int64_t ncnt,
                                                             int64_t nchan) {
  const int64_t stride = (int64_t)gridDim.x * kSfThreads;
  const int64_t most = max(ncube, max(ncnt, nchan));
  for (int64_t i = (int64_t)blockIdx.x * kSfThreads + threadIdx.x; i < most; i += stride) {
    if (i < ncube) cube[i] = 0.0;
    if (i < ncnt) cnt[i] = 0;
    if (i < nchan) {
      chansum[i] = 0.0;
      chansq[i] = 0.0;
    }
  }
}

// floor(a / b) for b > 0
__device__ __forceinline__ int64_t sf_floordiv(int64_t a, int64_t b) {
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// fold.trial_shift reduced to [0, nbins): 64-bit, so any int32 trial is safe
__device__ __forceinline__ int sf_shift(int ia, int ib, int p, int N, int nbins) {
  const int64_t m = 2 * p + 1 - N;
  int s = (int)(sf_floordiv((int64_t)ia * m * N + 2 * (int64_t)ib * m * m + (int64_t)N * N,
                            2 * (int64_t)N * N) % nbins);
  return s < 0 ? s + nbins : s;
}

__device__ __forceinline__ int sf_wrap(int r, int nbins) {
  r %= nbins;
  return r < 0 ? r + nbins : r;
}

// a before b in the order (chi2 descending, |k - mid| ascending, k ascending)
__device__ __forceinline__ bool sf_better(double ca, int ka, double cb, int kb, int mid) {
  if (ca > cb) return true;
  if (!(ca == cb)) return false;
  const int da = abs(ka - mid), db = abs(kb - mid);
  if (da != db) return da < db;
  return ka < kb;
}

size_t subfold_dm_lds(int nsub, int nbins, int npart, int ndm) {
  return sizeof(double) * ((size_t)nsub * nbins + 2 * (size_t)nsub + kSfWaves * kSfMaxBins + ndm +
                           kSfThreads) +
         sizeof(int) * ((size_t)nbins + npart + kSfThreads);
}

__global__ __launch_bounds__(kSfThreads) void k_subfold_dm(
    const double* __restrict__ cube, const int32_t* __restrict__ cnt,
    const double* __restrict__ chansum, const double* __restrict__ chansq,
    const int64_t* __restrict__ ntot, const int32_t* __restrict__ trials,
    const int32_t* __restrict__ rtab, int64_t C, int npart, int nsub, int nbins, int ndm,
    double* __restrict__ chi2, int32_t* __restrict__ best, double* __restrict__ best_chi2,
    double* __restrict__ best_prof, int64_t* __restrict__ best_cnt, double* __restrict__ sub,
    double* __restrict__ subints) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int cells = nsub * nbins;
  double* ssub = reinterpret_cast<double*>(smem);  // [nsub][nbins]
  double* smu = ssub + cells;                      // [nsub]
  double* svar = smu + nsub;                       // [nsub]
  double* term = svar + nsub;                      // [waves][kSfMaxBins]
  double* schi = term + kSfWaves * kSfMaxBins;     // [ndm]
  double* rc = schi + ndm;                         // [threads]
  int* scb = reinterpret_cast<int*>(rc + kSfThreads);  // [nbins]
  int* sshift = scb + nbins;                       // [npart]
  int* rk = sshift + npart;                        // [threads]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t j = blockIdx.x;
  const double* jc = cube + j * (int64_t)npart * cells;
  const int32_t* jn = cnt + j * (int64_t)npart * nbins;
  const int ia = trials[2 * j], ib = trials[2 * j + 1];
  for (int p = tid; p < npart; p += kSfThreads) sshift[p] = sf_shift(ia, ib, p, npart, nbins);
  __syncthreads();
  for (int t = tid; t < cells; t += kSfThreads) {
    const int b = t % nbins;
    const int64_t s = t / nbins;
    double acc = 0.0;
    for (int p = 0; p < npart; ++p) {
      int idx = b + sshift[p];
      idx = idx >= nbins ? idx - nbins : idx;
      acc += jc[((int64_t)p * nsub + s) * nbins + idx];
    }
    ssub[t] = acc;
    sub[j * cells + t] = acc;
  }
  for (int b = tid; b < nbins; b += kSfThreads) {
    int acc = 0;
    for (int p = 0; p < npart; ++p) {
      int idx = b + sshift[p];
      idx = idx >= nbins ? idx - nbins : idx;
      acc += jn[p * nbins + idx];
    }
    scb[b] = acc;
  }
  for (int t = tid; t < npart * nbins; t += kSfThreads) {
    const int b = t % nbins;
    const int64_t p = t / nbins;
    double acc = 0.0;
    for (int s = 0; s < nsub; ++s) acc += jc[(p * nsub + s) * nbins + b];
    subints[j * (int64_t)npart * nbins + t] = acc;
  }
  const int64_t cps = C / nsub;
  const double nt = (double)ntot[j];
  for (int s = tid; s < nsub; s += kSfThreads) {
    double mu = 0.0, var = 0.0;
    if (nt > 0.0) {
      for (int64_t c = s * cps; c < (s + 1) * cps; ++c) {
        const double m = chansum[j * C + c] / nt;
        const double v = chansq[j * C + c] / nt - m * m;
        mu += m;
        var += v;
      }
    }
    smu[s] = mu;
    svar[s] = var;
  }
  __syncthreads();
  const int32_t* jr = rtab + j * (int64_t)ndm * nsub;
  const double dof = (double)(nbins - 1);
  for (int kb = 0; kb < ndm; kb += kSfWaves) {  // (uniform over the workgroup)
    const int k = kb + wv;                      // (uniform over the wave)
    if (k < ndm) {
      for (int b = lane; b < nbins; b += 64) {
        double S = 0.0, E = 0.0, V = 0.0;
        for (int s = 0; s < nsub; ++s) {
          int idx = b + sf_wrap(jr[(int64_t)k * nsub + s], nbins);
          idx = idx >= nbins ? idx - nbins : idx;
          const double c = (double)scb[idx];
          S += ssub[s * nbins + idx];
          E += smu[s] * c;
          V += svar[s] * c;
        }
        double val = 0.0;
        if (V > 0.0) {
          const double dlt = S - E;
          val = (dlt * dlt) / V;
        }
        term[wv * kSfMaxBins + b] = val;
      }
    }
    __syncthreads();
    if (k < ndm && lane == 0) {
      double acc = 0.0;
      for (int b = 0; b < nbins; ++b) acc += term[wv * kSfMaxBins + b];
      acc = acc / dof;
      schi[k] = acc;
      chi2[j * ndm + k] = acc;
    }
    __syncthreads();
  }
  // the best entry by the total order
  const int mid = ndm / 2;
  double mc = 0.0;
  int mk = -1;
  for (int k = tid; k < ndm; k += kSfThreads) {
    if (mk < 0 || sf_better(schi[k], k, mc, mk, mid)) {
      mc = schi[k];
      mk = k;
    }
  }
  rc[tid] = mc;
  rk[tid] = mk;
  __syncthreads();
  for (int o = kSfThreads / 2; o > 0; o >>= 1) {
    if (tid < o && rk[tid + o] >= 0) {
      if (rk[tid] < 0 || sf_better(rc[tid + o], rk[tid + o], rc[tid], rk[tid], mid)) {
        rc[tid] = rc[tid + o];
        rk[tid] = rk[tid + o];
      }
    }
    __syncthreads();
  }
  const int kbest = rk[0];
  if (tid == 0) {
    best[j] = kbest;
    best_chi2[j] = rc[0];
  }
  for (int b = tid; b < nbins; b += kSfThreads) {
    double S = 0.0;
    int64_t cc = 0;
    for (int s = 0; s < nsub; ++s) {
      int idx = b + sf_wrap(jr[(int64_t)kbest * nsub + s], nbins);
      idx = idx >= nbins ? idx - nbins : idx;
      S += ssub[s * nbins + idx];
      cc += scb[idx];
    }
    best_prof[j * nbins + b] = S;
    best_cnt[j * nbins + b] = cc;
  }
}

int subfold_limits(const char* who, int64_t J, int64_t C, int npart, int nsub, int nbins) {
  PDD_REQUIRE(J >= 0 && J < (1ll << 20), "%s: bad job count", who);
  PDD_REQUIRE(nbins >= 2 && nbins <= kSfMaxBins, "%s: nbins out of range 2..%d", who, kSfMaxBins);
  PDD_REQUIRE(npart >= 1 && npart <= kSfMaxPart, "%s: npart out of range 1..%d", who, kSfMaxPart);
  PDD_REQUIRE(npart * nbins <= kSfMaxCells, "%s: npart * nbins exceeds %d", who, kSfMaxCells);
  PDD_REQUIRE(C >= 1 && C <= (1ll << 20), "%s: bad channel count", who);
  PDD_REQUIRE(nsub >= 1 && C % nsub == 0, "%s: nsub must divide the %lld channels", who,
              (long long)C);
  PDD_REQUIRE((int64_t)nsub * nbins <= kSfMaxCells, "%s: nsub * nbins exceeds %d", who,
              kSfMaxCells);
  return 0;
}

template <typename T, int CPL, bool STAGE>
int launch_subfold(const void* x, int64_t n, int64_t C, int64_t ld, int64_t t_first,
                   const int64_t* jobs_dev, int64_t J, const int32_t* table, int npart, int nsub,
                   int nbins, int64_t lmax, int64_t span, double* cube, int32_t* cnt,
                   double* chansum, double* chansq, hipStream_t st) {
  const int64_t nslice = cdiv(lmax, kSfSlice), ntile = cdiv(C, 64 * CPL);
  const int64_t blocks = J * npart * nslice * ntile;
  PDD_REQUIRE(blocks < (1ll << 31), "pdd_subfold: too large");
  const int stage_rows = STAGE ? (int)std::min<int64_t>(kSfStageRows, kSfChunk + span) : 0;
  const size_t lds = (size_t)nbins * 64 * sizeof(typename SfTypes<T>::hist_t) +
                     (size_t)nbins * sizeof(int) + (size_t)stage_rows * 64;
  if (lds > 64 * 1024) {
    // (more than the default 64 KiB of dynamic LDS: the largest case once per instance)
    static bool raised = false;
    if (!raised) {
      PDD_HIP(hipFuncSetAttribute(
          reinterpret_cast<const void*>(&k_subfold<T, CPL, STAGE>),
          hipFuncAttributeMaxDynamicSharedMemorySize,
          (int)(kSfMaxBins * 64 * sizeof(typename SfTypes<T>::hist_t) + kSfMaxBins * sizeof(int) +
                kSfStageRows * 64)));
      raised = true;
    }
  }
  k_subfold<T, CPL, STAGE><<<(unsigned)blocks, kSfThreads, lds, st>>>(
      static_cast<const T*>(x), n, C, ld, t_first, jobs_dev, table, npart, nsub, nbins, (int)nslice,
      (int)ntile, stage_rows, cube, cnt, chansum, chansq);
  PDD_LAUNCHED();
  return 0;
}

}  // namespace

}  // namespace pdd

using namespace pdd;

extern "C" {

int pdd_subfold_zero(double* cube, int32_t* cnt, double* chansum, double* chansq, int64_t J,
                     int64_t C, int npart, int nsub, int nbins, void* stream) {
  if (subfold_limits("pdd_subfold_zero", J, C, npart, nsub, nbins)) return -1;
  if (J == 0) return 0;
  PDD_REQUIRE(cube && cnt && chansum && chansq, "pdd_subfold_zero: null pointer");
  const int64_t ncnt = J * npart * nbins, ncube = ncnt * nsub, nchan = J * C;
  const int64_t most = std::max(ncube, std::max(ncnt, nchan));
  const int64_t blocks = std::min<int64_t>(cdiv(most, kSfThreads), 1 << 16);
  // (the loop runs to the largest of the three lengths; each store is guarded)
  k_subfold_zero<<<(unsigned)blocks, kSfThreads, 0, as_stream(stream)>>>(
      cube, cnt, chansum, chansq, ncube, ncnt, nchan);
  PDD_LAUNCHED();
  return 0;
}

int pdd_subfold(const void* x, int dtype, int64_t n, int64_t C, int64_t ld, int64_t t_first,
                const int64_t* jobs, const int64_t* jobs_dev, int64_t J, const int32_t* table,
                int64_t rows, int npart, int nsub, int nbins, double* cube, int32_t* cnt,
                double* chansum, double* chansq, int64_t tile_span, void* stream) {
  if (subfold_limits("pdd_subfold", J, C, npart, nsub, nbins)) return -1;
  PDD_REQUIRE(dtype == PDD_U8 || dtype == PDD_F32, "pdd_subfold: 8-bit or float32 input only");
  PDD_REQUIRE(n > 0 && n < (1ll << 31) && ld >= C && t_first >= 0 && t_first < (1ll << 40),
              "pdd_subfold: bad shape");
  PDD_REQUIRE(rows >= 0 && rows < (1ll << 31), "pdd_subfold: bad table");
  if (J == 0) return 0;
  PDD_REQUIRE(x && jobs && jobs_dev && table && cube && cnt && chansum && chansq,
              "pdd_subfold: null pointer");
  int64_t lmax = 0, bmax = 0;
  for (int64_t j = 0; j < J; ++j) {
    const int64_t* jb = jobs + kSfJob * j;
    const int64_t L = jb[3], i0 = jb[4], i1 = jb[5], row = jb[6], jbmax = jb[7];
    PDD_REQUIRE(L >= 1 && L * npart < (1ll << 31), "pdd_subfold: job %lld: bad part length %lld",
                (long long)j, (long long)L);
    PDD_REQUIRE(row >= 0 && row < rows && jbmax >= 0 && jbmax < (1ll << 31),
                "pdd_subfold: job %lld: bad table row or largest delay", (long long)j);
    PDD_REQUIRE(i0 >= 0 && i0 <= i1 && i1 <= L * npart,
                "pdd_subfold: job %lld folds [%lld, %lld), outside [0, %lld)", (long long)j,
                (long long)i0, (long long)i1, (long long)(L * npart));
    PDD_REQUIRE(i0 == i1 || (t_first <= i0 && i1 - 1 + jbmax < t_first + n),
                "pdd_subfold: job %lld: the block [%lld, %lld) does not cover samples [%lld, %lld) "
                "with delays up to %lld",
                (long long)j, (long long)t_first, (long long)(t_first + n), (long long)i0,
                (long long)i1, (long long)jbmax);
    lmax = std::max(lmax, L);
    bmax = std::max(bmax, jb[7]);
  }
  hipStream_t st = as_stream(stream);
  // 8-bit blocks whose rows are 4-byte aligned go through the LDS-staged
  // loads (one channel a lane); otherwise four adjacent channels a lane where
  // they share a subband and the band is wide enough to fill the lanes
  const bool four = (C / nsub) % 4 == 0 && C >= 256;
  const int64_t span = tile_span >= 0 ? std::min(tile_span, bmax) : bmax;  // sizes the staging only
  const bool aligned = reinterpret_cast<uintptr_t>(x) % 4 == 0 && ld % 4 == 0 && C % 4 == 0;
#define PDD_SUBFOLD_ARGS \
  x, n, C, ld, t_first, jobs_dev, J, table, npart, nsub, nbins, lmax, span, cube, cnt, chansum, \
      chansq, st
  if (dtype == PDD_U8) {
    if (aligned) return launch_subfold<uint8_t, 1, true>(PDD_SUBFOLD_ARGS);
    return four ? launch_subfold<uint8_t, 4, false>(PDD_SUBFOLD_ARGS)
                : launch_subfold<uint8_t, 1, false>(PDD_SUBFOLD_ARGS);
  }
  return four ? launch_subfold<float, 4, false>(PDD_SUBFOLD_ARGS)
              : launch_subfold<float, 1, false>(PDD_SUBFOLD_ARGS);
#undef PDD_SUBFOLD_ARGS
}

int pdd_subfold_dm(const double* cube, const int32_t* cnt, const double* chansum,
                   const double* chansq, const int64_t* ntot, const int32_t* trials,
                   const int32_t* rtab, int64_t J, int64_t C, int npart, int nsub, int nbins,
                   int ndm, double* chi2, int32_t* best, double* best_chi2, double* best_prof,
                   int64_t* best_cnt, double* sub, double* subints, void* stream) {
  if (subfold_limits("pdd_subfold_dm", J, C, npart, nsub, nbins)) return -1;
  PDD_REQUIRE(ndm >= 1 && ndm <= kSfMaxDm, "pdd_subfold_dm: ndm out of range 1..%d", kSfMaxDm);
  if (J == 0) return 0;
  PDD_REQUIRE(cube && cnt && chansum && chansq && ntot && trials && rtab && chi2 && best &&
                  best_chi2 && best_prof && best_cnt && sub && subints,
              "pdd_subfold_dm: null pointer");
  const size_t lds = subfold_dm_lds(nsub, nbins, npart, ndm);
  if (lds > 64 * 1024) {
    static bool raised = false;
    if (!raised) {
      PDD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_subfold_dm),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      raised = true;
    }
  }
  k_subfold_dm<<<(unsigned)J, kSfThreads, lds, as_stream(stream)>>>(
      cube, cnt, chansum, chansq, ntot, trials, rtab, C, npart, nsub, nbins, ndm, chi2, best,
      best_chi2, best_prof, best_cnt, sub, subints);
  PDD_LAUNCHED();
  return 0;
}

}  // extern "C"
