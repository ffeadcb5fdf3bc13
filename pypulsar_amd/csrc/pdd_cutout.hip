// libpdd: cut-outs of single-pulse candidates -- the dedispersed
// frequency-time image and the DM-time image ("bow tie") of many candidates
// from one time-major block of the file (pypulsar_amd/cutout.py; DESIGN.md
// §6k; restated by brute force in tests/cutout_oracle.py).  gfx950.
//
// A job is five int64 {t0, f, row0, bmin, bmax}: the first raw row of the
// image relative to the block's first row (may be negative), the samples
// summed per image bin, the job's first row of the int32 delay table
// [rows][C], and (DM-time only) bounds of the entries of its ndm table rows.
//
//   FT[s][b]  = sum_{c in subband s} sum_{k<f} X(c, t0 + b f + k + table[row0][c])
//   DMT[d][b] = sum_{all c}          sum_{k<f} X(c, t0 + b f + k + table[row0 + d][c])
//   X(c, t)   = x[t][c] for 0 <= t < n, else padvals[c] (NULL: 0)
//
// 8-bit input: the in-range part is an exact int32 sum (C f 255 < 2^31);
// the result is float32(that sum) + the float32 pad term.  float32 input:
// float32 sums in a fixed order.  No atomics: the same bits for any batching.
// A job that breaks its contract (f outside 1..fmax, a table row outside the
// table, an entry outside [bmin, bmax], a span above the stated one) reads
// and writes nothing out of bounds: its image comes back as NaN.
//
// Kernels:
//   k_cut_ft   one wave per (job, bin, 64 / G neighbouring subbands): the G
//              lanes of a subband stride over its channels -- lanes run
//              along the channel axis, whose delays are nearly equal, so a
//              wave reads few rows -- each lane sums its f samples, and a
//              butterfly over the G lanes adds them.
//   k_cut_box  DM-time, step 1: per job the box sums
//                P[c][r][m] = sum_{k<f} x[t0 + bmin + m f + r + k][c]
//              of every position u = m f + r a trial can ask for, once.  A
//              block takes 16 channels x one tile of ML f <= 1024 positions:
//              each thread slides one box along a sixteenth of the tile
//              (8-bit: exact; float32: restarted every 16 steps), into LDS,
//              and the tile is written out residue-major -- position m f + r
//              at [r][m] -- so that the nbin boxes of one (trial, channel),
//              f samples apart, are neighbours in memory.
//   k_cut_dmt  DM-time, step 2: a block owns 64 bins x 2 trials; lanes run
//              along the bins, the four waves split the channels.  Per
//              (trial, channel) the delay is wave-uniform: one scalar table
//              read, one contiguous 64-element read of P, 16 of them in
//              flight.  ndm nbin C reads whatever f is.  The waves' partial
//              sums are added through LDS in wave order.
#include <algorithm>

#include "pdd_internal.h"

namespace pdd {

namespace {

constexpr int kCutThreads = 256;
constexpr int kCutJob = 5;            // int64 fields of a job
constexpr int kCutMaxF = 1024;
constexpr int kCutMaxImg = 1024;      // nbin, ndm
constexpr int64_t kCutMaxSpan = 1ll << 22;
constexpr int64_t kCutMaxT0 = 1ll << 40;
constexpr int kCutMaxGridZ = 65535;
constexpr int kBoxChans = 16;         // channels of a k_cut_box tile
constexpr int kBoxSegs = kCutThreads / kBoxChans;
constexpr int kBoxTile = 1024;        // positions of a k_cut_box tile, at most (>= kCutMaxF)
constexpr int kDmtTrials = 2;         // trials a k_cut_dmt block holds in registers
constexpr int kDmtChans = 8;          // channels whose reads a k_cut_dmt wave has in flight

template <typename T> struct CutAcc { typedef int32_t type; };
template <> struct CutAcc<float> { typedef float type; };

struct CutJob {
  int64_t t0, f, row0, bmin, bmax;
};

__device__ __forceinline__ CutJob cut_job(const int64_t* __restrict__ jobs, int64_t j) {
  const int64_t* p = jobs + j * kCutJob;
  return {p[0], p[1], p[2], p[3], p[4]};
}

__device__ __forceinline__ bool cut_job_ok(const CutJob& jb, int fmax) {
  return jb.f >= 1 && jb.f <= fmax && jb.t0 >= -kCutMaxT0 && jb.t0 <= kCutMaxT0;
}

// Box positions of a DM-time job: u in [0, U), in M rows of f.
__device__ __forceinline__ bool cut_dmt_ok(const CutJob& jb, int fmax, int nbin, int ndm,
                                           int64_t rows, int64_t span, int64_t* M) {
  if (!cut_job_ok(jb, fmax) || jb.row0 < 0 || jb.row0 + ndm > rows || jb.bmax < jb.bmin ||
      jb.bmin < -kCutMaxT0 || jb.bmax > kCutMaxT0 || jb.bmax - jb.bmin >= kCutMaxSpan)
    return false;
  const int64_t U = (int64_t)(nbin - 1) * jb.f + (jb.bmax - jb.bmin) + 1;
  *M = (U + jb.f - 1) / jb.f;
  return *M * jb.f <= span;
}

template <typename T>
__global__ __launch_bounds__(kCutThreads) void k_cut_ft(
    const T* __restrict__ x, int64_t n, int C, int64_t ld, const int64_t* __restrict__ jobs,
    const int32_t* __restrict__ table, int64_t rows, const float* __restrict__ pad, int nbin,
    int nsub, int cps, int G, int fmax, float* __restrict__ out) {
  typedef typename CutAcc<T>::type Acc;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t j = blockIdx.z;
  const int b = blockIdx.y;
  const int s = (blockIdx.x * (kCutThreads / 64) + wave) * (64 / G) + lane / G;
  const int i = lane % G;
  const CutJob jb = cut_job(jobs, j);
  const bool ok = cut_job_ok(jb, fmax) && jb.row0 >= 0 && jb.row0 < rows;
  const bool live = s < nsub;
  Acc acc = 0;
  float psum = 0.f;
  if (ok && live) {
    const int32_t* __restrict__ tab = table + jb.row0 * C;
    for (int c = s * cps + i; c < (s + 1) * cps; c += G) {
      const int64_t r0 = jb.t0 + (int64_t)b * jb.f + tab[c];
      const int64_t klo = max((int64_t)0, -r0), khi = min(jb.f, n - r0);
      const T* __restrict__ xc = x + (r0 + klo) * ld + c;
      const int nk = (int)max(khi - klo, (int64_t)0);
#pragma unroll 8
      for (int k = 0; k < nk; ++k) acc += (Acc)xc[k * ld];
      if (pad) psum += (float)(jb.f - max(khi - klo, (int64_t)0)) * pad[c];
    }
  }
  // (every lane takes part; the butterfly leaves the same sum in all G lanes)
  for (int d = G >> 1; d >= 1; d >>= 1) {
    acc += __shfl_xor(acc, d);
    psum += __shfl_xor(psum, d);
  }
  if (live && i == 0)
    out[(j * nsub + s) * nbin + b] = ok ? (float)acc + psum : __builtin_nanf("");
}

// x[t][c], 0 outside rows 0..n-1; n >= 1.  The load is unconditional, at a
// clamped row, so that a run of them can be in flight together.
template <typename T>
__device__ __forceinline__ typename CutAcc<T>::type cut_val(const T* __restrict__ x, int64_t n,
                                                            int64_t ld, int c, int64_t t) {
  typedef typename CutAcc<T>::type Acc;
  const int64_t tc = min(max(t, (int64_t)0), n - 1);
  const Acc v = (Acc)x[tc * ld + c];
  return tc == t ? v : (Acc)0;
}

template <typename T, typename B>
__global__ __launch_bounds__(kCutThreads) void k_cut_box(
    const T* __restrict__ x, int64_t n, int C, int64_t ld, const int64_t* __restrict__ jobs,
    int64_t rows, int nbin, int ndm, int fmax, int64_t span, B* __restrict__ P) {
  typedef typename CutAcc<T>::type Acc;
  constexpr int kLtMax = kBoxTile;
  // a box slides along its whole segment (8-bit: exact) or 16 steps (float32)
  constexpr int kRestart = sizeof(T) == 1 ? kLtMax : 16;
  __shared__ B tile[kBoxChans * kLtMax];
  const int64_t j = blockIdx.z;
  const CutJob jb = cut_job(jobs, j);
  int64_t M = 0;
  if (!cut_dmt_ok(jb, fmax, nbin, ndm, rows, span, &M)) return;
  const int f = (int)jb.f;
  const int ML = kLtMax / f, LT = ML * f;  // f <= 1024 <= kLtMax
  const int64_t m_first = (int64_t)blockIdx.x * ML;
  if (m_first >= M) return;
  const int cl = threadIdx.x % kBoxChans, seg = threadIdx.x / kBoxChans;
  const int c = blockIdx.y * kBoxChans + cl;
  const int SL = (LT + kBoxSegs - 1) / kBoxSegs;
  const int ua = seg * SL, ub = min(ua + SL, LT);
  if (c < C && n <= 0) {
    for (int u = ua; u < ub; ++u) tile[cl * LT + u] = (B)0;
  } else if (c < C && ua < ub) {
    // raw row of the first sample of box ua of this tile
    const int64_t ta = jb.t0 + jb.bmin + m_first * f + ua;
    for (int u0 = ua; u0 < ub; u0 += kRestart) {
      const int64_t t = ta + (u0 - ua);
      Acc s = 0;
#pragma unroll 8
      for (int k = 0; k < f; ++k) s += cut_val(x, n, ld, c, t + k);
      tile[cl * LT + u0] = (B)s;
      const int steps = min(kRestart, ub - u0);
#pragma unroll 8
      for (int i = 1; i < steps; ++i) {
        s += cut_val(x, n, ld, c, t + i + f - 1) - cut_val(x, n, ld, c, t + i - 1);
        tile[cl * LT + u0 + i] = (B)s;
      }
    }
  }
  __syncthreads();
  B* __restrict__ Pj = P + j * span * C;
  const int64_t Mf = M * f;
  for (int e = threadIdx.x; e < kBoxChans * LT; e += kCutThreads) {
    const int ml = e % ML, r = (e / ML) % f, ecl = e / LT;
    const int ec = blockIdx.y * kBoxChans + ecl;
    const int64_t m = m_first + ml;
    if (ec < C && m < M) Pj[ec * Mf + r * M + m] = tile[ecl * LT + ml * f + r];
  }
}

template <typename B>
__global__ __launch_bounds__(kCutThreads) void k_cut_dmt(
    const B* __restrict__ P, int64_t n, int C, const int64_t* __restrict__ jobs,
    const int32_t* __restrict__ table, int64_t rows, const float* __restrict__ pad, int nbin,
    int ndm, int fmax, int64_t span, float* __restrict__ out) {
  typedef typename CutAcc<B>::type Acc;  // (uint16, uint32: int32; float: float)
  __shared__ Acc racc[kCutThreads / 64][kDmtTrials][64];
  __shared__ float rpad[kCutThreads / 64][kDmtTrials][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t j = blockIdx.z;
  const int bfirst = blockIdx.x * 64, b = bfirst + lane;
  const int d0 = blockIdx.y * kDmtTrials;
  const CutJob jb = cut_job(jobs, j);
  int64_t M = 0;
  bool ok = cut_dmt_ok(jb, fmax, nbin, ndm, rows, span, &M);
  Acc acc[kDmtTrials];
  float psum[kDmtTrials];
#pragma unroll
  for (int q = 0; q < kDmtTrials; ++q) {
    acc[q] = 0;
    psum[q] = 0.f;
  }
  bool bad = false;
  if (ok) {
    const uint32_t f = (uint32_t)jb.f;
    // u / f for u < 2^22, f <= 2^10: (u * ceil(2^32 / f)) >> 32
    const uint64_t magic = ((1ull << 32) + f - 1) / f;
    const B* __restrict__ Pj = P + j * span * C;
    const int64_t Mf = M * f;
    const int Cq = (C + 3) / 4;
    const int c_end = min(C, (wave + 1) * Cq);
    const int bb = min(b, nbin - 1);  // (a lane past the last bin repeats it; not stored)
    const int32_t* tab[kDmtTrials];
#pragma unroll
    for (int q = 0; q < kDmtTrials; ++q)  // (a trial past the last repeats it; not stored)
      tab[q] = table + (jb.row0 + min(d0 + q, ndm - 1)) * C;
    // position of box 0 of (trial q, channel c) in P; an entry outside the
    // stated bounds poisons the image and stands in as position 0
    auto first_box = [&](int q, int c) -> int64_t {
      const int64_t bins = tab[q][c];
      const bool out_of_bounds = bins < jb.bmin || bins > jb.bmax;
      bad |= out_of_bounds;
      const uint32_t u0 = out_of_bounds ? 0u : (uint32_t)(bins - jb.bmin);
      const uint32_t m0 = (uint32_t)(((uint64_t)u0 * magic) >> 32);
      return c * Mf + (int64_t)(u0 - m0 * f) * M + m0;
    };
    int c = wave * Cq;
    for (; c + kDmtChans <= c_end; c += kDmtChans) {
      B v[kDmtChans][kDmtTrials];
#pragma unroll
      for (int i = 0; i < kDmtChans; ++i)
#pragma unroll
        for (int q = 0; q < kDmtTrials; ++q) v[i][q] = Pj[first_box(q, c + i) + bb];
#pragma unroll
      for (int i = 0; i < kDmtChans; ++i)
#pragma unroll
        for (int q = 0; q < kDmtTrials; ++q) acc[q] += (Acc)v[i][q];
    }
    for (; c < c_end; ++c)
#pragma unroll
      for (int q = 0; q < kDmtTrials; ++q) acc[q] += (Acc)Pj[first_box(q, c) + bb];
    if (pad) {
      // the samples of this wave's boxes outside the block: none for most (trial, channel)
      for (c = wave * Cq; c < c_end; ++c)
#pragma unroll
        for (int q = 0; q < kDmtTrials; ++q) {
          const int64_t bins = tab[q][c];
          const int64_t w0 = jb.t0 + bins + (int64_t)bfirst * f;
          if (w0 < 0 || w0 + (int64_t)64 * f > n) {
            const int64_t r0 = jb.t0 + bins + (int64_t)bb * f;
            const int64_t in = min(r0 + (int64_t)f, n) - max(r0, (int64_t)0);
            psum[q] += (float)((int64_t)f - max(in, (int64_t)0)) * pad[c];
          }
        }
    }
  }
#pragma unroll
  for (int q = 0; q < kDmtTrials; ++q) {
    racc[wave][q][lane] = acc[q];
    rpad[wave][q][lane] = psum[q];
  }
  // (bad is wave-uniform; any wave's counts)
  const int anybad = __syncthreads_or(bad ? 1 : 0);
  if (wave != 0 || b >= nbin) return;
#pragma unroll
  for (int q = 0; q < kDmtTrials; ++q) {
    const int d = d0 + q;
    if (d >= ndm) continue;
    Acc a = racc[0][q][lane];
    float p = rpad[0][q][lane];
    for (int w = 1; w < kCutThreads / 64; ++w) {
      a += racc[w][q][lane];
      p += rpad[w][q][lane];
    }
    out[(j * ndm + d) * nbin + b] = (ok && !anybad) ? (float)a + p : __builtin_nanf("");
  }
}

// The limits both entry points share (checked before any pointer is looked at).
int cut_check_common(const char* who, int dtype, int64_t n, int64_t C, int64_t ld, int64_t J,
                     int64_t rows, int nbin, int fmax) {
  PDD_REQUIRE(dtype == PDD_U8 || dtype == PDD_F32, "%s: dtype must be PDD_U8 or PDD_F32", who);
  PDD_REQUIRE(J >= 0 && J < (1ll << 31), "%s: J out of range 0..2^31-1", who);
  PDD_REQUIRE(nbin >= 1 && nbin <= kCutMaxImg, "%s: nbin out of range 1..%d", who, kCutMaxImg);
  PDD_REQUIRE(fmax >= 1 && fmax <= kCutMaxF, "%s: fmax out of range 1..%d", who, kCutMaxF);
  PDD_REQUIRE(C >= 1 && C < (1ll << 31) && C * fmax * 255 < (1ll << 31),
              "%s: C * fmax * 255 must be below 2^31", who);
  PDD_REQUIRE(n >= 0 && n < (1ll << 40) && ld >= C && ld < (1ll << 22) && rows >= 1 &&
                  rows * C < (1ll << 40),
              "%s: n, ld or rows out of range", who);
  return 0;
}

}  // namespace

}  // namespace pdd

using namespace pdd;

extern "C" {

int pdd_cutout_ft(const void* x, int dtype, int64_t n, int64_t C, int64_t ld, const int64_t* jobs,
                  int64_t J, const int32_t* table, int64_t rows, const float* padvals, int nbin,
                  int nsub, int fmax, float* out, void* stream) {
  if (cut_check_common("pdd_cutout_ft", dtype, n, C, ld, J, rows, nbin, fmax)) return -1;
  PDD_REQUIRE(nsub >= 1 && nsub <= C && C % nsub == 0, "pdd_cutout_ft: nsub must divide C");
  if (J == 0) return 0;
  PDD_REQUIRE((x || n == 0) && jobs && table && out, "pdd_cutout_ft: null pointer");
  const int cps = (int)(C / nsub);
  int G = 1;
  while (G < 64 && G < cps) G <<= 1;
  hipStream_t st = as_stream(stream);
  const unsigned gx = (unsigned)cdiv(cdiv(nsub, 64 / G), kCutThreads / 64);
  for (int64_t j0 = 0; j0 < J; j0 += kCutMaxGridZ) {
    const dim3 grid(gx, (unsigned)nbin, (unsigned)std::min<int64_t>(J - j0, kCutMaxGridZ));
    float* o = out + j0 * nsub * nbin;
    const int64_t* jb = jobs + j0 * kCutJob;
    if (dtype == PDD_U8)
      k_cut_ft<uint8_t><<<grid, kCutThreads, 0, st>>>((const uint8_t*)x, n, (int)C, ld, jb, table,
                                                      rows, padvals, nbin, nsub, cps, G, fmax, o);
    else
      k_cut_ft<float><<<grid, kCutThreads, 0, st>>>((const float*)x, n, (int)C, ld, jb, table,
                                                    rows, padvals, nbin, nsub, cps, G, fmax, o);
    PDD_LAUNCHED();
  }
  return 0;
}

int pdd_cutout_dmt(const void* x, int dtype, int64_t n, int64_t C, int64_t ld, const int64_t* jobs,
                   int64_t J, const int32_t* table, int64_t rows, const float* padvals, int nbin,
                   int ndm, int fmax, int64_t span, void* work, int64_t work_bytes, float* out,
                   void* stream) {
  if (cut_check_common("pdd_cutout_dmt", dtype, n, C, ld, J, rows, nbin, fmax)) return -1;
  PDD_REQUIRE(ndm >= 1 && ndm <= kCutMaxImg, "pdd_cutout_dmt: ndm out of range 1..%d", kCutMaxImg);
  PDD_REQUIRE(span >= 1 && span <= kCutMaxSpan, "pdd_cutout_dmt: span out of range 1..2^22");
  if (J == 0) return 0;
  PDD_REQUIRE((x || n == 0) && jobs && table && out, "pdd_cutout_dmt: null pointer");
  // box sums: 16 bits hold fmax * 255 up to fmax = 257
  const int64_t per_job = span * C * ((dtype == PDD_U8 && fmax * 255 <= 65535) ? 2 : 4);
  PDD_REQUIRE(work && work_bytes >= per_job && ((uintptr_t)work & 3) == 0,
              "pdd_cutout_dmt: work must hold %lld bytes (one job), 4-byte aligned",
              (long long)per_job);
  const bool wide = per_job == span * C * 4;
  hipStream_t st = as_stream(stream);
  const int64_t pass = std::min<int64_t>(std::min<int64_t>(J, work_bytes / per_job), kCutMaxGridZ);
  // tiles of a job: at most span / (a tile's positions), a tile holds more
  // than half of kBoxTile positions whatever f is
  const int64_t lt_min = kBoxTile / 2;
  const unsigned tiles = (unsigned)(span / lt_min + 1);
  for (int64_t j0 = 0; j0 < J; j0 += pass) {
    const unsigned jn = (unsigned)std::min<int64_t>(J - j0, pass);
    const int64_t* jb = jobs + j0 * kCutJob;
    float* o = out + j0 * ndm * nbin;
    const dim3 gbox(tiles, (unsigned)cdiv(C, kBoxChans), jn);
    const dim3 gdmt((unsigned)cdiv(nbin, 64), (unsigned)cdiv(ndm, kDmtTrials), jn);
    if (dtype == PDD_F32) {
      k_cut_box<float, float><<<gbox, kCutThreads, 0, st>>>((const float*)x, n, (int)C, ld, jb,
                                                            rows, nbin, ndm, fmax, span,
                                                            (float*)work);
      PDD_LAUNCHED();
      k_cut_dmt<float><<<gdmt, kCutThreads, 0, st>>>((const float*)work, n, (int)C, jb, table,
                                                     rows, padvals, nbin, ndm, fmax, span, o);
    } else if (wide) {
      k_cut_box<uint8_t, uint32_t><<<gbox, kCutThreads, 0, st>>>((const uint8_t*)x, n, (int)C, ld,
                                                                 jb, rows, nbin, ndm, fmax, span,
                                                                 (uint32_t*)work);
      PDD_LAUNCHED();
      k_cut_dmt<uint32_t><<<gdmt, kCutThreads, 0, st>>>((const uint32_t*)work, n, (int)C, jb,
                                                        table, rows, padvals, nbin, ndm, fmax,
                                                        span, o);
    } else {
      k_cut_box<uint8_t, uint16_t><<<gbox, kCutThreads, 0, st>>>((const uint8_t*)x, n, (int)C, ld,
                                                                 jb, rows, nbin, ndm, fmax, span,
                                                                 (uint16_t*)work);
      PDD_LAUNCHED();
      k_cut_dmt<uint16_t><<<gdmt, kCutThreads, 0, st>>>((const uint16_t*)work, n, (int)C, jb,
                                                        table, rows, padvals, nbin, ndm, fmax,
                                                        span, o);
    }
    PDD_LAUNCHED();
  }
  return 0;
}

}  // extern "C"
