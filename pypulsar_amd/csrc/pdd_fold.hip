// libpdd: folding of DM-time plane rows at candidate periods and the search
// of the folds over period / period-derivative offsets.  gfx950.
//
// New (the reference folds on the host: Datfile.pulses, formats/datfile.py:
// 231-275, cuts single turns, Pulse.downsample_Nbins and SummedPulse.__iadd__,
// formats/pulse.py:197-215 and :425-482, bin and sum them).  The arithmetic is
// stated in include/pdd.h and restated in tests/fold_oracle.py.
//
// Phase is a 64-bit unsigned fraction of a turn (wrap-around arithmetic):
// sample i of a row has P_i = P0 + i step + (i (i - 1) / 2) accel (mod 2^64)
// and falls into bin ((P_i >> 32) * nbins) >> 32.
//
// Kernels:
//   k_fold_rows    one workgroup per (job, part, slice of <= 16384 samples).
//                  A wave stages 1024 consecutive samples in LDS with
//                  lane-strided (coalesced) loads; every lane then walks 16
//                  CONSECUTIVE samples of them (LDS stride 17: no bank
//                  conflict).  Consecutive samples fall into the same or a
//                  nearby bin, so the lane keeps the running float64 sum of
//                  its current bin in registers and touches the workgroup's
//                  LDS histogram (float64 / int32 atomics) only when the bin
//                  changes.  The phase of a lane's first sample comes from the
//                  closed form, the later ones from P += d, d += accel.  The
//                  histogram is added to the (zeroed) output with global
//                  atomics, once per workgroup.
//   k_fold_search  one workgroup per (job, tile of trials).  The job's
//                  sub-integrations and counts are staged once in LDS; the
//                  job's mean and variance are taken in a fixed order.  A
//                  wave takes one trial at a time: lane p computes the
//                  integer shift of part p, lane b sums bin b over the parts
//                  in ascending p (the shift is read from lane p's register),
//                  the chi-square terms of a batch of trials go to a wave-
//                  private LDS buffer and one lane per trial sums them in
//                  ascending b -- the oracle's order, operation by operation.
//   k_fold_best    one workgroup per job: the best trial by the total order
//                  (chi2 descending, |ib|, |ia|, ib, ia ascending) and its
//                  summed profile.
#include <algorithm>

#include "pdd_internal.h"

namespace pdd {

namespace {

constexpr int kFoldThreads = 256;
constexpr int kFoldWaves = kFoldThreads / 64;
constexpr int kFoldPer = 16;                        // consecutive samples per lane
constexpr int kFoldWaveTile = 64 * kFoldPer;        // samples a wave stages at once
constexpr int kFoldTile = kFoldWaves * kFoldWaveTile;  // samples per workgroup iteration
constexpr int kFoldSlice = 4 * kFoldTile;           // samples per workgroup
constexpr int kFoldMaxBins = 256;
constexpr int kFoldMaxPart = 128;
constexpr int kFoldMaxCells = 8192;
constexpr int kFoldMaxTrial = 256;
constexpr int kFoldTermBuf = 1024;                  // float64 chi-square terms per wave

__global__ __launch_bounds__(kFoldThreads) void k_fold_rows(
    const float* __restrict__ plane, int64_t D, int64_t ld, int64_t L,
    const int64_t* __restrict__ jobs, int npart, int nbins, int nslice,
    double* __restrict__ prof, int32_t* __restrict__ cnt, double* __restrict__ sumsq) {
  __shared__ float buf[kFoldWaves][64 * (kFoldPer + 1)];
  __shared__ double hp[kFoldMaxBins];
  __shared__ int hc[kFoldMaxBins];
  __shared__ double red[kFoldWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int slice = blockIdx.x % nslice;
  const int part = (blockIdx.x / nslice) % npart;
  const int64_t j = blockIdx.x / ((int64_t)nslice * npart);
  const int64_t row = jobs[4 * j];
  if (row < 0 || row >= D) return;  // (refused on the host already; uniform)
  const uint64_t P0 = (uint64_t)jobs[4 * j + 1], step = (uint64_t)jobs[4 * j + 2],
                 accel = (uint64_t)jobs[4 * j + 3];
  const int64_t part0 = (int64_t)part * L;
  const int64_t s_begin = (int64_t)slice * kFoldSlice;
  const int64_t s_end = min(L, s_begin + (int64_t)kFoldSlice);
  const float* src = plane + row * ld + part0;
  for (int b = tid; b < nbins; b += kFoldThreads) {
    hp[b] = 0.0;
    hc[b] = 0;
  }
  __syncthreads();
  double run = 0.0, sq = 0.0;
  int runc = 0, runbin = -1;
  const uint64_t nb = (uint64_t)nbins;
  for (int64_t t0 = s_begin; t0 < s_end; t0 += kFoldTile) {  // (uniform trip count)
    const int64_t base = t0 + (int64_t)wv * kFoldWaveTile;
    float v[kFoldPer];
#pragma unroll
    for (int u = 0; u < kFoldPer; ++u) {
      const int64_t idx = base + u * 64 + lane;
      v[u] = idx < s_end ? src[idx] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kFoldPer; ++u) {
      const int k = u * 64 + lane;  // sample k of the wave's tile: lane k / 16, element k % 16
      buf[wv][k + (k >> 4)] = v[u];
    }
    __syncthreads();
    const int64_t first = base + (int64_t)lane * kFoldPer;
    if (first < s_end) {
      const uint64_t i = (uint64_t)(part0 + first);  // index in the row, < 2^31
      const uint64_t tri = i == 0 ? 0 : (i * (i - 1)) >> 1;
      uint64_t P = P0 + i * step + tri * accel;
      uint64_t d = step + i * accel;  // P_{i+1} - P_i
      const int m = (int)min((int64_t)kFoldPer, s_end - first);
#pragma unroll
      for (int e = 0; e < kFoldPer; ++e) {
        if (e < m) {
          const double x = (double)buf[wv][lane * (kFoldPer + 1) + e];
          const int bin = (int)(((P >> 32) * nb) >> 32);
          if (bin != runbin) {
            if (runc) {
              atomicAdd(&hp[runbin], run);
              atomicAdd(&hc[runbin], runc);
            }
            runbin = bin;
            run = 0.0;
            runc = 0;
          }
          run += x;
          runc += 1;
          sq += x * x;
          P += d;
          d += accel;
        }
      }
    }
    __syncthreads();
  }
  if (runc) {
    atomicAdd(&hp[runbin], run);
    atomicAdd(&hc[runbin], runc);
  }
  for (int o = 32; o > 0; o >>= 1) sq += __shfl_down(sq, o);
  if (lane == 0) red[wv] = sq;
  __syncthreads();
  const int64_t cell = (j * npart + part) * (int64_t)nbins;
  for (int b = tid; b < nbins; b += kFoldThreads) {
    if (hc[b]) {
      atomicAdd(&prof[cell + b], hp[b]);
      atomicAdd(&cnt[cell + b], hc[b]);
    }
  }
  if (tid == 0) atomicAdd(&sumsq[j * npart + part], (red[0] + red[1]) + (red[2] + red[3]));
}

// The outputs of k_fold_rows start from zero (one launch for the three).
__global__ __launch_bounds__(kFoldThreads) void k_fold_zero(double* __restrict__ prof,
                                                            int32_t* __restrict__ cnt,
                                                            double* __restrict__ sumsq,
                                                            int64_t cells, int64_t parts) {
  const int64_t i = (int64_t)blockIdx.x * kFoldThreads + threadIdx.x;
  if (i < cells) {
    prof[i] = 0.0;
    cnt[i] = 0;
  }
  if (i < parts) sumsq[i] = 0.0;
}

// floor(a / b) for b > 0
__device__ __forceinline__ int floordiv(int a, int b) {
  const int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// The shift of part p of N for trial (ia, ib), reduced to [0, nbins):
// floor((ia m N + 2 ib m m + N N) / (2 N N)), m = 2 p + 1 - N.
// (|ia|, |ib| <= 256, N <= 128: every product is below 2^25.)
__device__ __forceinline__ int fold_shift(int ia, int ib, int p, int N, int nbins) {
  const int m = 2 * p + 1 - N;
  int s = floordiv(ia * m * N + 2 * ib * m * m + N * N, 2 * N * N) % nbins;
  return s < 0 ? s + nbins : s;
}

// Mean and population variance of a job from its staged parts, in a fixed
// order: part sums in ascending bin, then the parts' sums, counts and sums of
// squares in ascending part.  stat[0] = mu, stat[1] = var (0 without samples).
__device__ __forceinline__ void fold_stats(const double* sp, const int* sc,
                                           const double* __restrict__ sumsq_j, int npart, int nbins,
                                           double* psum, long long* pcnt, double* stat) {
  const int tid = threadIdx.x;
  if (tid < npart) {
    double s = 0.0;
    long long c = 0;
    for (int b = 0; b < nbins; ++b) {
      s += sp[tid * nbins + b];
      c += sc[tid * nbins + b];
    }
    psum[tid] = s;
    pcnt[tid] = c;
  }
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0, q = 0.0;
    long long c = 0;
    for (int p = 0; p < npart; ++p) {
      tot += psum[p];
      q += sumsq_j[p];
      c += pcnt[p];
    }
    double mu = 0.0, var = 0.0;
    if (c > 0) {
      mu = tot / (double)c;
      var = q / (double)c - mu * mu;
    }
    stat[0] = mu;
    stat[1] = var;
  }
  __syncthreads();
}

// NB = ceil(nbins / 64): the bins lane + 64 k of a trial are one lane's.
template <int NB>
__global__ __launch_bounds__(kFoldThreads) void k_fold_search(
    const double* __restrict__ prof, const int32_t* __restrict__ cnt,
    const double* __restrict__ sumsq, int npart, int nbins, int A, int B, int tiles,
    double* __restrict__ chi2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int cells = npart * nbins;
  double* sp = reinterpret_cast<double*>(smem);                       // [cells]
  double* term = sp + cells;                                          // [waves][kFoldTermBuf]
  double* psum = term + kFoldWaves * kFoldTermBuf;                    // [kFoldMaxPart]
  long long* pcnt = reinterpret_cast<long long*>(psum + kFoldMaxPart);  // [kFoldMaxPart]
  double* stat = reinterpret_cast<double*>(pcnt + kFoldMaxPart);      // [2]
  int* sc = reinterpret_cast<int*>(stat + 2);                         // [cells]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t job = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles;
  const double* gp = prof + job * cells;
  const int32_t* gc = cnt + job * cells;
  for (int i = tid; i < cells; i += kFoldThreads) {
    sp[i] = gp[i];
    sc[i] = gc[i];
  }
  __syncthreads();
  fold_stats(sp, sc, sumsq + job * npart, npart, nbins, psum, pcnt, stat);
  const double mu = stat[0], var = stat[1];
  const bool good = var > 0.0;

  const int nb_ = 2 * B + 1;
  const int ntrial = (2 * A + 1) * nb_;
  const int per = (ntrial + tiles - 1) / tiles;     // trials of a tile
  const int t0 = tile * per, t1 = min(ntrial, t0 + per);
  const int per_wave = (per + kFoldWaves - 1) / kFoldWaves;
  const int stride = nbins + 1;                     // (odd stride in float64: no bank conflict)
  const int batch = min(64, kFoldTermBuf / stride);
  const int nbatch = (per_wave + batch - 1) / batch;
  double* tb = term + wv * kFoldTermBuf;
  double* out = chi2 + job * ntrial;
  const double dof = (double)(nbins - 1);

  int bk[NB];
  bool act[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    bk[k] = lane + 64 * k;
    act[k] = bk[k] < nbins;
  }
  for (int bt = 0; bt < nbatch; ++bt) {  // (uniform over the workgroup)
    for (int q = 0; q < batch; ++q) {
      const int t = t0 + wv + kFoldWaves * (bt * batch + q);  // (uniform over the wave)
      if (t >= t1) break;
      const int ia = t / nb_ - A, ib = t % nb_ - B;
      // lane p holds the shifts of parts p and p + 64 (all lanes compute)
      const int s_lo = fold_shift(ia, ib, min(lane, npart - 1), npart, nbins);
      const int s_hi = fold_shift(ia, ib, min(lane + 64, npart - 1), npart, nbins);
      double S[NB];
      int C[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        S[k] = 0.0;
        C[k] = 0;
      }
      // Parts in ascending p, four at a time: the 8 NB LDS reads of a group are
      // independent of each other and of the adds of the group before.  Lanes
      // without a bin read cell 0 of the part (their sums are never stored).
      int p = 0;
      for (; p + 4 <= npart; p += 4) {
        double v[4][NB];
        int c[4][NB];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int s = __builtin_amdgcn_readlane(p + u < 64 ? s_lo : s_hi, (p + u) & 63);
          const int base = (p + u) * nbins;
#pragma unroll
          for (int k = 0; k < NB; ++k) {
            int idx = bk[k] + s;
            idx = idx >= nbins ? idx - nbins : idx;
            idx = act[k] ? base + idx : base;
            v[u][k] = sp[idx];
            c[u][k] = sc[idx];
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int k = 0; k < NB; ++k) {
            S[k] += v[u][k];
            C[k] += c[u][k];
          }
        }
      }
      for (; p < npart; ++p) {
        const int s = __builtin_amdgcn_readlane(p < 64 ? s_lo : s_hi, p & 63);
        const int base = p * nbins;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          int idx = bk[k] + s;
          idx = idx >= nbins ? idx - nbins : idx;
          idx = act[k] ? base + idx : base;
          S[k] += sp[idx];
          C[k] += sc[idx];
        }
      }
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        if (act[k]) {
          double val = 0.0;
          if (good && C[k] > 0) {
            const double c = (double)C[k];
            const double dlt = S[k] - c * mu;
            val = (dlt * dlt) / (c * var);
          }
          tb[q * stride + bk[k]] = val;
        }
      }
    }
    __syncthreads();
    if (lane < batch) {
      const int t = t0 + wv + kFoldWaves * (bt * batch + lane);
      if (t < t1) {
        double acc = 0.0;
#pragma unroll 8
        for (int b = 0; b < nbins; ++b) acc += tb[lane * stride + b];  // (+ 0.0 where C == 0)
        out[t] = good ? acc / dof : 0.0;
      }
    }
    __syncthreads();
  }
}

struct Best {
  double c;
  int ia, ib;
};

// a before b in the order (chi2 descending, |ib|, |ia|, ib, ia ascending)
__device__ __forceinline__ bool fold_better(const Best& a, const Best& b) {
  if (a.c > b.c) return true;
  if (!(a.c == b.c)) return false;
  const int aib = abs(a.ib), bib = abs(b.ib), aia = abs(a.ia), bia = abs(b.ia);
  if (aib != bib) return aib < bib;
  if (aia != bia) return aia < bia;
  if (a.ib != b.ib) return a.ib < b.ib;
  return a.ia < b.ia;
}

__global__ __launch_bounds__(kFoldThreads) void k_fold_best(
    const double* __restrict__ prof, const int32_t* __restrict__ cnt,
    const double* __restrict__ chi2, int npart, int nbins, int A, int B,
    int32_t* __restrict__ best, double* __restrict__ best_chi2, double* __restrict__ best_prof,
    int32_t* __restrict__ best_cnt) {
  __shared__ double bc[kFoldThreads];
  __shared__ int bia[kFoldThreads], bib[kFoldThreads], bok[kFoldThreads];
  const int tid = threadIdx.x;
  const int64_t job = blockIdx.x;
  const int nb_ = 2 * B + 1, ntrial = (2 * A + 1) * nb_;
  const double* in = chi2 + job * ntrial;
  Best me = {0.0, 0, 0};
  bool have = false;
  for (int t = tid; t < ntrial; t += kFoldThreads) {
    const Best o = {in[t], t / nb_ - A, t % nb_ - B};
    if (!have || fold_better(o, me)) me = o;
    have = true;
  }
  bc[tid] = me.c;
  bia[tid] = me.ia;
  bib[tid] = me.ib;
  bok[tid] = have ? 1 : 0;
  __syncthreads();
  for (int o = kFoldThreads / 2; o > 0; o >>= 1) {
    if (tid < o && bok[tid + o]) {
      const Best x = {bc[tid], bia[tid], bib[tid]}, y = {bc[tid + o], bia[tid + o], bib[tid + o]};
      if (!bok[tid] || fold_better(y, x)) {
        bc[tid] = y.c;
        bia[tid] = y.ia;
        bib[tid] = y.ib;
        bok[tid] = 1;
      }
    }
    __syncthreads();
  }
  const int ia = bia[0], ib = bib[0];
  if (tid == 0) {
    best[2 * job] = ia;
    best[2 * job + 1] = ib;
    best_chi2[job] = bc[0];
  }
  const int cells = npart * nbins;
  for (int b = tid; b < nbins; b += kFoldThreads) {
    double S = 0.0;
    int C = 0;
    for (int p = 0; p < npart; ++p) {
      int idx = b + fold_shift(ia, ib, p, npart, nbins);
      idx = idx >= nbins ? idx - nbins : idx;
      S += prof[job * cells + p * nbins + idx];
      C += cnt[job * cells + p * nbins + idx];
    }
    best_prof[job * nbins + b] = S;
    best_cnt[job * nbins + b] = C;
  }
}

size_t fold_search_lds(int cells) {
  return (size_t)cells * (sizeof(double) + sizeof(int)) +
         sizeof(double) * (kFoldWaves * kFoldTermBuf + 2 * kFoldMaxPart + 2);
}

template <int NB>
int launch_fold_search(const double* prof, const int32_t* cnt, const double* sumsq, int64_t J,
                       int npart, int nbins, int A, int B, int tiles, double* chi2,
                       hipStream_t st) {
  const size_t lds = fold_search_lds(npart * nbins);
  if (lds > 64 * 1024) {
    // (more than the default 64 KiB of dynamic LDS: the largest case once per instance)
    static bool raised = false;
    if (!raised) {
      PDD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fold_search<NB>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)fold_search_lds(kFoldMaxCells)));
      raised = true;
    }
  }
  k_fold_search<NB><<<(unsigned)(J * tiles), kFoldThreads, lds, st>>>(prof, cnt, sumsq, npart,
                                                                     nbins, A, B, tiles, chi2);
  PDD_LAUNCHED();
  return 0;
}

}  // namespace

}  // namespace pdd

using namespace pdd;

extern "C" {

int pdd_fold_rows(const float* plane, int64_t D, int64_t n, int64_t ld, const int64_t* jobs,
                  const int64_t* jobs_dev, int64_t J, int npart, int nbins, double* prof,
                  int32_t* cnt, double* sumsq, void* stream) {
  PDD_REQUIRE(J >= 0 && J < (1ll << 20), "pdd_fold_rows: bad job count");
  PDD_REQUIRE(nbins >= 2 && nbins <= kFoldMaxBins, "pdd_fold_rows: nbins out of range 2..%d",
              kFoldMaxBins);
  PDD_REQUIRE(npart >= 1 && npart <= kFoldMaxPart, "pdd_fold_rows: npart out of range 1..%d",
              kFoldMaxPart);
  PDD_REQUIRE(npart * nbins <= kFoldMaxCells, "pdd_fold_rows: npart * nbins exceeds %d",
              kFoldMaxCells);
  PDD_REQUIRE(D >= 0 && n > 0 && ld >= n && n < (1ll << 31), "pdd_fold_rows: bad shape");
  if (J == 0) return 0;
  PDD_REQUIRE(plane && jobs && jobs_dev && prof && cnt && sumsq, "pdd_fold_rows: null pointer");
  for (int64_t j = 0; j < J; ++j)
    PDD_REQUIRE(jobs[4 * j] >= 0 && jobs[4 * j] < D,
                "pdd_fold_rows: job %lld folds row %lld, outside [0, %lld)", (long long)j,
                (long long)jobs[4 * j], (long long)D);
  const int64_t L = n / npart;
  PDD_REQUIRE(L >= 1, "pdd_fold_rows: fewer samples than parts");
  const int64_t nslice = cdiv(L, kFoldSlice);
  const int64_t blocks = J * npart * nslice;
  PDD_REQUIRE(blocks < (1ll << 31), "pdd_fold_rows: too large");
  hipStream_t st = as_stream(stream);
  const int64_t cells = J * npart * nbins;
  k_fold_zero<<<(unsigned)cdiv(cells, kFoldThreads), kFoldThreads, 0, st>>>(prof, cnt, sumsq, cells,
                                                                           J * npart);
  PDD_LAUNCHED();
  k_fold_rows<<<(unsigned)blocks, kFoldThreads, 0, st>>>(plane, D, ld, L, jobs_dev, npart, nbins,
                                                        (int)nslice, prof, cnt, sumsq);
  PDD_LAUNCHED();
  return 0;
}

int pdd_fold_search(const double* prof, const int32_t* cnt, const double* sumsq, int64_t J,
                    int npart, int nbins, int A, int B, double* chi2, int32_t* best,
                    double* best_chi2, double* best_prof, int32_t* best_cnt, void* stream) {
  PDD_REQUIRE(J >= 0 && J < (1ll << 20), "pdd_fold_search: bad job count");
  PDD_REQUIRE(nbins >= 2 && nbins <= kFoldMaxBins, "pdd_fold_search: nbins out of range 2..%d",
              kFoldMaxBins);
  PDD_REQUIRE(npart >= 1 && npart <= kFoldMaxPart, "pdd_fold_search: npart out of range 1..%d",
              kFoldMaxPart);
  PDD_REQUIRE(npart * nbins <= kFoldMaxCells, "pdd_fold_search: npart * nbins exceeds %d",
              kFoldMaxCells);
  PDD_REQUIRE(A >= 0 && A <= kFoldMaxTrial && B >= 0 && B <= kFoldMaxTrial,
              "pdd_fold_search: trial half-widths out of range 0..%d", kFoldMaxTrial);
  if (J == 0) return 0;
  PDD_REQUIRE(prof && cnt && sumsq && chi2 && best && best_chi2 && best_prof && best_cnt,
              "pdd_fold_search: null pointer");
  const int ntrial = (2 * A + 1) * (2 * B + 1);
  const int tiles = (int)std::min<int64_t>(64, cdiv(ntrial, 1024));
  PDD_REQUIRE(J * tiles < (1ll << 31), "pdd_fold_search: too large");
  hipStream_t st = as_stream(stream);
  int rc;
  switch ((nbins + 63) / 64) {
    case 1: rc = launch_fold_search<1>(prof, cnt, sumsq, J, npart, nbins, A, B, tiles, chi2, st); break;
    case 2: rc = launch_fold_search<2>(prof, cnt, sumsq, J, npart, nbins, A, B, tiles, chi2, st); break;
    case 3: rc = launch_fold_search<3>(prof, cnt, sumsq, J, npart, nbins, A, B, tiles, chi2, st); break;
    default: rc = launch_fold_search<4>(prof, cnt, sumsq, J, npart, nbins, A, B, tiles, chi2, st); break;
  }
  if (rc) return rc;
  k_fold_best<<<(unsigned)J, kFoldThreads, 0, st>>>(prof, cnt, chi2, npart, nbins, A, B, best,
                                                   best_chi2, best_prof, best_cnt);
  PDD_LAUNCHED();
  return 0;
}

}  // extern "C"
