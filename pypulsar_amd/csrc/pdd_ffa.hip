// libpdd: fast-folding (FFA) search of a DM-time plane for long periods --
// downsampling + detrending, the radix-2 fast-folding butterfly with a matched
// boxcar score, and the candidate search of the periodogram.  gfx950.
//
// The arithmetic is stated in include/pdd.h and restated in
// tests/ffa_oracle.py.
//
// Kernels:
//   k_ffa_down     one workgroup per (row, chunk): y[i] = the float32 sum of f
//                  consecutive samples (ascending), the chunk's float64 mean by
//                  a fixed tree
//   k_ffa_detrend  one workgroup per (row, chunk): y' = float32(double(y) -
//                  base(i)), base the line between the means of consecutive
//                  chunks at their centres; the chunk's float64 sums of y' and
//                  y'^2 by a fixed tree
//   k_ffa_sigma    one wave per row: the chunks' sums in a fixed order -> sigma
//   k_ffa_pass     one pass of the butterfly.  The transform of Mp = 2^K rows
//                  is cut into npass passes of <= kpass stages.  A pass that
//                  starts at level a (blocks of 2^a rows are transformed) and
//                  runs k stages handles, per workgroup, trial s0 of 2^k
//                  consecutive level-a blocks: it gathers those 2^k rows of p0
//                  bins (pass 0: 2^k consecutive rows of the series itself, no
//                  reshape), runs the k stages between two LDS buffers (the
//                  circular shift is an LDS address) and writes trials
//                  s0 2^k .. s0 2^k + 2^k - 1 of its level-(a + k) block: 2^k
//                  consecutive rows of the workspace.  The last pass scores
//                  its 2^k finished profiles in LDS (prefix sums into the free
//                  buffer, the widths in a loop) and writes only the S/N and
//                  the width index.
//                  Lanes run along the bin axis in every phase (consecutive
//                  lanes, consecutive LDS words), so no access has a stride of
//                  p0 floats and rows need no padding.
//   k_ffa_search   one thread per trial (+ one halo trial on each side of a
//                  workgroup), candidates through one atomic counter
#include <cmath>

#include "pdd_internal.h"

namespace pdd {

namespace {

constexpr int kFfaPrepThreads = 256;
constexpr int kFfaThreads = 512;                // k_ffa_pass workgroup
constexpr int kFfaWaves = kFfaThreads / 64;
constexpr int kFfaLoads = 8;                    // independent global loads of a thread
constexpr int kFfaLds = 160 * 1024;             // LDS a workgroup may declare
constexpr int kFfaMaxK = 8;                     // stages of one pass (256 rows in LDS)
constexpr int kFfaTabBytes = kFfaMaxK * (1 << kFfaMaxK) * 4;  // the passes' shift tables
constexpr int kFfaMinBins = 2, kFfaMaxBins = 1024;
constexpr int kFfaMaxWidths = 16;
constexpr int kFfaScoreBytes = 2 * kFfaMaxWidths * 8;  // the widths' float64 terms
constexpr int kFfaTile = 256 - 2;               // trials per k_ffa_search workgroup

struct FfaInfo {
  int64_t M;   // real rows n_ds / p0
  int K;       // Mp = 2^K = max(2, next power of two >= M)
  int kpass;   // stages per pass (the last pass: the rest)
  int npass;
};

// The split of the K stages into passes, the same on the host and the device:
// kfit stages fit (two buffers of 2^kfit rows of p0 floats beside the shift
// tables); npass = ceil(K / kfit) passes of kpass = ceil(K / npass) stages, so
// equal passes that leave LDS for a second workgroup where K allows.
__host__ __device__ inline FfaInfo ffa_info(int64_t n_ds, int p0) {
  FfaInfo I;
  I.M = n_ds / p0;
  int K = 1;
  while ((1ll << K) < I.M) ++K;
  I.K = K;
  int kfit = 1;
  while (kfit < kFfaMaxK && (int64_t)8 * p0 * (2ll << kfit) <= kFfaLds - kFfaTabBytes - kFfaScoreBytes)
    ++kfit;
  I.npass = (K + kfit - 1) / kfit;
  I.kpass = (K + I.npass - 1) / I.npass;
  return I;
}

__host__ __device__ inline int64_t ffa_pass_lds(int p0, int k) {
  return kFfaScoreBytes + (int64_t)8 * p0 * (1ll << k) + (int64_t)4 * k * (1ll << k);
}

// Fixed binary tree over the workgroup's 256 partial sums (deterministic).
__device__ __forceinline__ double ffa_block_sum(double v, double* part) {
  const int tid = threadIdx.x;
  __syncthreads();  // (part may still be read from a previous call)
  part[tid] = v;
  __syncthreads();
  for (int o = kFfaPrepThreads / 2; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  return part[0];
}

__global__ __launch_bounds__(kFfaPrepThreads) void k_ffa_down(const float* __restrict__ x,
                                                              int64_t ld, int64_t f, int64_t n_ds,
                                                              int64_t L, int64_t nchunk,
                                                              float* __restrict__ y,
                                                              double* __restrict__ mean) {
  __shared__ double part[kFfaPrepThreads];
  const int64_t c = blockIdx.x, d = blockIdx.y;
  const int64_t i0 = c * L, i1 = c == nchunk - 1 ? n_ds : i0 + L;
  const float* row = x + d * ld;
  double s = 0.0;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += kFfaPrepThreads) {
    const float* p = row + i * f;
    float acc = p[0];
    for (int64_t q = 1; q < f; ++q) acc += p[q];
    y[d * n_ds + i] = acc;
    s += (double)acc;
  }
  const double tot = ffa_block_sum(s, part);
  if (threadIdx.x == 0) mean[d * nchunk + c] = tot / (double)(i1 - i0);
}

// Centre of chunk c: the mean index of its samples.
__device__ __forceinline__ double ffa_centre(int64_t c, int64_t L, int64_t nchunk, int64_t n_ds) {
  const int64_t len = c == nchunk - 1 ? n_ds - c * L : L;
  return (double)(c * L) + 0.5 * (double)(len - 1);
}

__global__ __launch_bounds__(kFfaPrepThreads) void k_ffa_detrend(float* __restrict__ y,
                                                                 int64_t n_ds, int64_t L,
                                                                 int64_t nchunk,
                                                                 const double* __restrict__ mean,
                                                                 double* __restrict__ part_out) {
  __shared__ double part[kFfaPrepThreads];
  const int64_t c = blockIdx.x, d = blockIdx.y;
  const int64_t i0 = c * L, i1 = c == nchunk - 1 ? n_ds : i0 + L;
  const double* m = mean + d * nchunk;
  const double ctr = ffa_centre(c, L, nchunk, n_ds);
  double s1 = 0.0, s2 = 0.0;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += kFfaPrepThreads) {
    // the pair of chunks whose centres enclose sample i
    const int64_t lo = (double)i < ctr ? c - 1 : c;
    double base;
    if (lo < 0) {
      base = m[0];
    } else if (lo >= nchunk - 1) {
      base = m[nchunk - 1];
    } else {
      const double c0 = ffa_centre(lo, L, nchunk, n_ds), c1 = ffa_centre(lo + 1, L, nchunk, n_ds);
      base = m[lo] + (m[lo + 1] - m[lo]) * (((double)i - c0) / (c1 - c0));
    }
    const float v = (float)((double)y[d * n_ds + i] - base);
    y[d * n_ds + i] = v;
    s1 += (double)v;
    s2 += (double)v * (double)v;
  }
  const double t1 = ffa_block_sum(s1, part);
  const double t2 = ffa_block_sum(s2, part);
  if (threadIdx.x == 0) {
    part_out[(d * nchunk + c) * 2] = t1;
    part_out[(d * nchunk + c) * 2 + 1] = t2;
  }
}

__global__ __launch_bounds__(64) void k_ffa_sigma(const double* __restrict__ part, int64_t nchunk,
                                                  int64_t n_ds, double* __restrict__ sigma) {
  const int64_t d = blockIdx.x;
  const int lane = threadIdx.x;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t c = lane; c < nchunk; c += 64) {
    s1 += part[(d * nchunk + c) * 2];
    s2 += part[(d * nchunk + c) * 2 + 1];
  }
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  if (lane == 0) {
    const double mu = s1 / (double)n_ds;
    const double var = s2 / (double)n_ds - mu * mu;
    sigma[d] = var > 0.0 ? sqrt(var) : 0.0;
  }
}

// The largest v of the wave's 64 lanes, in every lane: an inclusive scan of
// each row of 16 lanes by DPP row shifts, the rows combined by the two row
// broadcasts (the result stands in lane 63), one readlane.  The whole wave
// must call it.
__device__ __forceinline__ float ffa_wave_max(float v) {
  constexpr int kNegInf = (int)0xff800000u;
#define PDD_FFA_DPP_MAX(ctrl, rows)                                                            \
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(kNegInf, __float_as_int(v), ctrl, \
                                                          rows, 0xf, false)))
  PDD_FFA_DPP_MAX(0x111, 0xf);  // row_shr:1
  PDD_FFA_DPP_MAX(0x112, 0xf);  // row_shr:2
  PDD_FFA_DPP_MAX(0x114, 0xf);  // row_shr:4
  PDD_FFA_DPP_MAX(0x118, 0xf);  // row_shr:8
  PDD_FFA_DPP_MAX(0x142, 0xa);  // row_bcast:15 into rows 1 and 3
  PDD_FFA_DPP_MAX(0x143, 0xc);  // row_bcast:31 into rows 2 and 3
#undef PDD_FFA_DPP_MAX
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// Inclusive sums over the wave's lanes (any association), the same way.
__device__ __forceinline__ float ffa_wave_scan(float v) {
#define PDD_FFA_DPP_ADD(ctrl, rows)                                                          \
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, rows, 0xf, false))
  PDD_FFA_DPP_ADD(0x111, 0xf);
  PDD_FFA_DPP_ADD(0x112, 0xf);
  PDD_FFA_DPP_ADD(0x114, 0xf);
  PDD_FFA_DPP_ADD(0x118, 0xf);
  PDD_FFA_DPP_ADD(0x142, 0xa);
  PDD_FFA_DPP_ADD(0x143, 0xc);
#undef PDD_FFA_DPP_ADD
  return v;
}

// Lane i takes (v, idx) of lane i - n of its row of 16 where that is the
// better pair: the larger v, on equal v the smaller idx.
template <int kCtrl>
__device__ __forceinline__ void ffa_row_best(double& v, int& idx) {
  const long long bits = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)bits, kCtrl, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp((int)0xfff00000u, (int)(bits >> 32), kCtrl, 0xf, 0xf,
                                             false);                  // (no source lane: -inf)
  const int oi = __builtin_amdgcn_update_dpp(0x7fffffff, idx, kCtrl, 0xf, 0xf, false);
  const double ov = __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
  if (ov > v || (ov == v && oi < idx)) {
    v = ov;
    idx = oi;
  }
}

struct FfaPass {
  const float* y;        // [D][n_ds] detrended series, row stride ld
  int64_t n_ds, ld;
  int p_lo, np, pass;
  const float* ws_in;    // [D np][slot] level-a rows (pass > 0)
  float* ws_out;         // [D np][slot] (passes before the last)
  int64_t slot;
  const double* sigma;   // [D]
  const int64_t* toff;   // [np] first trial of base period p_lo + i on the row's axis
  float* snr;            // [D][ntrial] (null: no score)
  uint8_t* widx;
  int64_t ntrial;
  float* prof;           // [D np][prof_slot] finished profiles (test hook; null: none)
  int64_t prof_slot;
  int nw;
  int widths[kFfaMaxWidths];
  double ducy;
};

// (4 waves per SIMD: two workgroups share a CU where their LDS allows)
__global__ __launch_bounds__(kFfaThreads, 4) void k_ffa_pass(FfaPass A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ffa_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned probu = blockIdx.y, du = probu / (unsigned)A.np;
  const int64_t prob = probu, d = du;
  const int p0 = A.p_lo + (int)(probu - du * (unsigned)A.np);
  const FfaInfo I = ffa_info(A.n_ds, p0);
  const int a = A.pass * I.kpass;          // the level this pass starts from
  if (a >= I.K) return;                    // (uniform: this base period is finished)
  const int k = min(I.kpass, I.K - a);
  const int64_t Mp = 1ll << I.K;
  if ((int64_t)blockIdx.x >= (Mp >> k)) return;
  if (Mp * p0 > A.slot && (A.pass > 0 || a + k < I.K)) return;  // (refused by the host already)
  const bool last = a + k == I.K;
  const int rows = 1 << k;
  const int nel = rows * p0;
  double* sc = reinterpret_cast<double*>(ffa_smem);  // the score's terms per width
  float* src = reinterpret_cast<float*>(ffa_smem + kFfaScoreBytes);
  float* dst = src + nel;
  int* tab = reinterpret_cast<int*>(dst + nel);
  const int64_t s0 = (int64_t)blockIdx.x & ((1ll << a) - 1);  // trial of the level-a blocks
  const int64_t g = (int64_t)blockIdx.x >> a;                 // group of 2^k level-a blocks

  // shift of output row R in stage t: trial s_t = s0 2^t + (R mod 2^t) of its
  // block takes the tail at ((s_t + 1) >> 1) mod p0
  for (int idx = tid; idx < k * rows; idx += kFfaThreads) {
    const int t = (idx >> k) + 1, R = idx & (rows - 1);
    const unsigned st = ((unsigned)s0 << t) + (unsigned)(R & ((1 << t) - 1));  // (< Mp <= 2^30)
    tab[idx] = (int)(((st + 1) >> 1) % (unsigned)p0);
  }
  // element e = R p0 + b of the workgroup: thread tid holds e = tid + 512 i
  const int R0 = tid / p0, b0 = tid - R0 * p0;
  const int dr = kFfaThreads / p0, db = kFfaThreads - dr * p0;
  // The gather, kFfaLoads independent loads at a time.  Pass 0: the 2^k rows
  // are consecutive in the series (real below row M, zero from there on);
  // later passes: row R of the workgroup is row ((g 2^k + R) << a) + s0 of the
  // workspace, p0 << a floats after row R - 1.
  {
    const float* in;
    int64_t skip;      // floats between the ends and starts of consecutive rows
    int nreal;         // elements that exist in memory
    if (a == 0) {
      in = A.y + d * A.ld + g * rows * p0;
      skip = 0;
      const int64_t left = (I.M - g * rows) * p0;
      nreal = (int)(left < 0 ? 0 : (left < nel ? left : nel));
    } else {
      in = A.ws_in + prob * A.slot + (((g * rows) << a) + s0) * p0;
      skip = ((int64_t)p0 << a) - p0;
      nreal = nel;
    }
    int R = R0, b = b0;
    for (int e0 = tid; e0 < nel; e0 += kFfaLoads * kFfaThreads) {
      float v[kFfaLoads];
#pragma unroll
      for (int u = 0; u < kFfaLoads; ++u) {
        const int e = e0 + u * kFfaThreads;
        v[u] = e < nreal ? in[e + R * skip] : 0.f;
        b += db;
        R += dr;
        if (b >= p0) {
          b -= p0;
          ++R;
        }
      }
#pragma unroll
      for (int u = 0; u < kFfaLoads; ++u) {
        const int e = e0 + u * kFfaThreads;
        if (e < nel) src[e] = v[u];
      }
    }
  }
  __syncthreads();
  // A stage: wave wv takes output rows wv, wv + 8, ..; the row's head and
  // tail rows and its shift are scalars, the lanes run along the bins.
  const int wvs = __builtin_amdgcn_readfirstlane(wv);
  for (int t = 1; t <= k; ++t) {
    const int half_el = (1 << (t - 1)) * p0;
    const int jm = (1 << t) - 1;
    const int* sh = tab + (t - 1) * rows;
    for (int R = wvs; R < rows; R += kFfaWaves) {
      const int j = R & jm;
      const float* h = src + (R - ((j + 1) >> 1)) * p0;   // head[j >> 1]
      const float* tl = h + half_el;                      // tail[j >> 1]
      float* o = dst + R * p0;
      const unsigned shift = (unsigned)__builtin_amdgcn_readfirstlane(sh[R]);
#pragma unroll 4
      for (int b = lane; b < p0; b += 64) {
        unsigned bb = (unsigned)b + shift;                // (b + shift) mod p0
        bb = min(bb, bb - (unsigned)p0);
        o[b] = h[b] + tl[bb];
      }
    }
    __syncthreads();
    float* tmp = src;
    src = dst;
    dst = tmp;
  }
  // src: trials s0 2^k + R of the level-(a + k) block g
  if (!last) {
    float* out = A.ws_out + prob * A.slot + ((g << (a + k)) + (s0 << k)) * p0;
#pragma unroll 4
    for (int e = tid; e < nel; e += kFfaThreads) out[e] = src[e];
    return;
  }
  if (A.prof && Mp * p0 <= A.prof_slot) {
    float* out = A.prof + prob * A.prof_slot + (s0 << k) * p0;
    for (int e = tid; e < nel; e += kFfaThreads) out[e] = src[e];
  }
  if (!A.snr) return;
  // The admitted widths (ascending) and their float64 terms, once per
  // workgroup: sc[wi] = 1 / (sigma sqrt(M w (1 - w / p0))), sc[16 + wi] = w / p0.
  const double sg = A.sigma[d];
  const int wmax = max(1, (int)floor(A.ducy * (double)p0));
  int nwv = 0;
  while (nwv < A.nw && A.widths[nwv] <= wmax && A.widths[nwv] < p0) ++nwv;
  if (tid < kFfaMaxWidths) {
    const double dw = tid < nwv ? (double)A.widths[tid] : 1.0;
    sc[tid] = 1.0 / (sg * sqrt((double)I.M * dw * (1.0 - dw / (double)p0)));
    sc[kFfaMaxWidths + tid] = dw / (double)p0;
  }
  __syncthreads();
  // One wave per profile.  Prefix sums: lane l sums its q consecutive bins,
  // the lanes' totals are scanned across the wave, and the lane writes its
  // bins' prefixes; q is odd, so the lanes' stride of q words touches every
  // bank once.  Boxcars: lanes along the bins, every width in registers.
  const int q = ((p0 + 63) >> 6) | 1;
  const int wlast = nwv ? A.widths[nwv - 1] : 0;
  for (int it = 0; it < (rows + kFfaWaves - 1) / kFfaWaves; ++it) {
    const int R = it * kFfaWaves + wv;
    const bool active = R < rows;           // (uniform over the wave)
    const float* x = src + (active ? R : 0) * p0;
    float* P = dst + (active ? R : 0) * p0; // inclusive prefix sums of the profile
    if (active) {
      const int i0 = min(p0, lane * q), i1 = min(p0, i0 + q);
      float run = 0.f;
      for (int i = i0; i < i1; ++i) run += x[i];
      const float incl = ffa_wave_scan(run);
      // (wave_shr:1: the sum of the lanes before this one, 0 in lane 0)
      const float excl = __int_as_float(
          __builtin_amdgcn_update_dpp(0, __float_as_int(incl), 0x138, 0xf, 0xf, false));
      run = 0.f;
      for (int i = i0; i < i1; ++i) {
        run += x[i];
        P[i] = excl + run;
      }
    }
    __syncthreads();
    if (!active) continue;
    const float T = P[p0 - 1];
    float m[kFfaMaxWidths];
#pragma unroll
    for (int wi = 0; wi < kFfaMaxWidths; ++wi) m[wi] = -INFINITY;
    // groups of 64 bins whose widest boxcar ends inside the profile ...
    int base = 0;
    for (; base + 63 + wlast <= p0; base += 64) {
      const int b = base + lane;
      const float cb = b ? P[b - 1] : 0.f;
#pragma unroll
      for (int wi = 0; wi < kFfaMaxWidths; ++wi)
        if (wi < nwv) m[wi] = fmaxf(m[wi], P[b + A.widths[wi] - 1] - cb);  // (uniform branch)
    }
    // ... and the rest, where it may wrap around
    for (; base < p0; base += 64) {
      const int b = base + lane;
      if (b < p0) {
        const float cb = b ? P[b - 1] : 0.f;
        const float tcb = T - cb;
#pragma unroll
        for (int wi = 0; wi < kFfaMaxWidths; ++wi) {
          if (wi < nwv) {
            const int e = b + A.widths[wi];
            const float pe = P[e <= p0 ? e - 1 : e - p0 - 1];
            m[wi] = fmaxf(m[wi], e <= p0 ? pe - cb : tcb + pe);
          }
        }
      }
    }
    // lane wi < nwv: snr of width wi; the best of lanes 0..15, the narrower on ties
    float mv = -INFINITY;
#pragma unroll
    for (int wi = 0; wi < kFfaMaxWidths; ++wi) {
      if (wi < nwv) {
        const float mw = ffa_wave_max(m[wi]);
        if (lane == wi) mv = mw;
      }
    }
    double v = -INFINITY;
    if (lane < nwv) v = ((double)mv - sc[kFfaMaxWidths + lane] * (double)T) * sc[lane];
    int bi = lane;
    ffa_row_best<0x111>(v, bi);   // lane 15: the best of lanes 0..15
    ffa_row_best<0x112>(v, bi);
    ffa_row_best<0x114>(v, bi);
    ffa_row_best<0x118>(v, bi);
    const int64_t s = (s0 << k) + R;
    if (lane == 15 && s < Mp - 1) {
      const int64_t tr = A.toff[p0 - A.p_lo] + s;
      if (tr >= 0 && tr < A.ntrial) {
        const bool ok = nwv > 0 && sg > 0.0;
        A.snr[d * A.ntrial + tr] = ok ? (float)v : 0.f;
        A.widx[d * A.ntrial + tr] = ok ? (uint8_t)bi : (uint8_t)0;
      }
    }
  }
}

// Thread t of workgroup blk holds trial k = blk * 254 - 1 + t: threads 1..254
// own a trial, threads 0 and 255 are the neighbours of the first and last.
__global__ __launch_bounds__(256) void k_ffa_search(const float* __restrict__ snr,
                                                    const uint8_t* __restrict__ widx, int64_t nt,
                                                    int64_t ld, float thr, int64_t nblk,
                                                    int32_t* __restrict__ cands, int64_t max_cands,
                                                    unsigned long long* __restrict__ count) {
  __shared__ float sh[256];
  const int tid = threadIdx.x;
  const int64_t d = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int64_t k = blk * kFfaTile - 1 + tid;
  const bool in = k >= 0 && k < nt;
  const float v = in ? snr[d * ld + k] : -INFINITY;
  sh[tid] = v;
  __syncthreads();
  if (in && tid >= 1 && tid <= kFfaTile && v >= thr && v > sh[tid - 1] && v >= sh[tid + 1]) {
    const unsigned long long slot = atomicAdd(count, 1ull);
    if ((int64_t)slot < max_cands) {
      int32_t* c = cands + slot * 4;
      c[0] = (int32_t)d;
      c[1] = (int32_t)k;
      c[2] = (int32_t)widx[d * ld + k];
      c[3] = __float_as_int(v);
    }
  }
}

}  // namespace

}  // namespace pdd

using namespace pdd;

extern "C" {

int pdd_ffa_plan_info(int64_t n_ds, int p0, int64_t* info) {
  PDD_REQUIRE(info, "pdd_ffa_plan_info: null pointer");
  PDD_REQUIRE(p0 >= kFfaMinBins && p0 <= kFfaMaxBins, "pdd_ffa_plan_info: p0 out of range %d..%d",
              kFfaMinBins, kFfaMaxBins);
  PDD_REQUIRE(n_ds >= 2 * (int64_t)p0 && n_ds < (1ll << 31),
              "pdd_ffa_plan_info: n_ds must be in [2 p0, 2^31)");
  const FfaInfo I = ffa_info(n_ds, p0);
  info[0] = I.M;
  info[1] = I.K;
  info[2] = I.kpass;
  info[3] = I.npass;
  return 0;
}

int pdd_ffa_downsample(const float* x, int64_t D, int64_t n, int64_t ld, int64_t f, int64_t L,
                       float* y, double* mean, void* stream) {
  PDD_REQUIRE(x && y && mean, "pdd_ffa_downsample: null pointer");
  PDD_REQUIRE(D >= 0 && n > 0 && ld >= n && n < (1ll << 31) && f >= 1 && f <= n && L >= 1,
              "pdd_ffa_downsample: bad shape");
  const int64_t n_ds = n / f;
  const int64_t nchunk = n_ds / L > 1 ? n_ds / L : 1;
  PDD_REQUIRE(D < 65536 && nchunk < (1ll << 31), "pdd_ffa_downsample: too large");
  if (D == 0) return 0;
  k_ffa_down<<<dim3((unsigned)nchunk, (unsigned)D), kFfaPrepThreads, 0, as_stream(stream)>>>(
      x, ld, f, n_ds, L, nchunk, y, mean);
  PDD_LAUNCHED();
  return 0;
}

int pdd_ffa_detrend(float* y, int64_t D, int64_t n_ds, int64_t L, const double* mean, double* part,
                    double* sigma, void* stream) {
  PDD_REQUIRE(y && mean && part && sigma, "pdd_ffa_detrend: null pointer");
  PDD_REQUIRE(D >= 0 && n_ds > 0 && n_ds < (1ll << 31) && L >= 1, "pdd_ffa_detrend: bad shape");
  const int64_t nchunk = n_ds / L > 1 ? n_ds / L : 1;
  PDD_REQUIRE(D < 65536 && nchunk < (1ll << 31), "pdd_ffa_detrend: too large");
  if (D == 0) return 0;
  k_ffa_detrend<<<dim3((unsigned)nchunk, (unsigned)D), kFfaPrepThreads, 0, as_stream(stream)>>>(
      y, n_ds, L, nchunk, mean, part);
  PDD_LAUNCHED();
  k_ffa_sigma<<<(unsigned)D, 64, 0, as_stream(stream)>>>(part, nchunk, n_ds, sigma);
  PDD_LAUNCHED();
  return 0;
}

int pdd_ffa_pass(const float* y, int64_t D, int64_t n_ds, int64_t ld, int p_lo, int np, int pass,
                 const float* ws_in, float* ws_out, int64_t slot, const double* sigma,
                 const int64_t* toff, const int32_t* widths, int n_widths, double ducy_max,
                 float* snr, uint8_t* widx, int64_t ntrial, float* prof, void* stream) {
  PDD_REQUIRE(y, "pdd_ffa_pass: null pointer");
  PDD_REQUIRE((snr == nullptr) == (widx == nullptr), "pdd_ffa_pass: null pointer (snr / widx)");
  PDD_REQUIRE(!snr || (sigma && toff && widths), "pdd_ffa_pass: null pointer (score arguments)");
  PDD_REQUIRE(D >= 0 && np >= 1 && pass >= 0 && pass < 32 && slot >= 0 && ntrial >= 0 && ld >= n_ds,
              "pdd_ffa_pass: bad shape");
  PDD_REQUIRE(p_lo >= kFfaMinBins && p_lo + np - 1 <= kFfaMaxBins,
              "pdd_ffa_pass: base periods out of range %d..%d", kFfaMinBins, kFfaMaxBins);
  PDD_REQUIRE(n_ds >= 2 * (int64_t)(p_lo + np - 1) && n_ds < (1ll << 31),
              "pdd_ffa_pass: n_ds must be in [2 p0, 2^31)");
  PDD_REQUIRE(D * np < 65536, "pdd_ffa_pass: more than 65535 problems in one launch");
  PDD_REQUIRE(!prof || np == 1, "pdd_ffa_pass: the profile hook takes one base period");
  PDD_REQUIRE(!snr || (n_widths >= 1 && n_widths <= kFfaMaxWidths && ducy_max > 0.0),
              "pdd_ffa_pass: 1..%d widths and ducy_max > 0", kFfaMaxWidths);
  FfaPass A;
  A.nw = 0;
  for (int i = 0; snr && i < n_widths; ++i) {
    PDD_REQUIRE(widths[i] >= 1 && widths[i] <= kFfaMaxBins && (i == 0 || widths[i] > widths[i - 1]),
                "pdd_ffa_pass: widths must ascend within 1..%d", kFfaMaxBins);
    A.widths[A.nw++] = widths[i];
  }
  int64_t gx = 0, lds = 0, prof_slot = 0;
  for (int p0 = p_lo; p0 < p_lo + np; ++p0) {
    const FfaInfo I = ffa_info(n_ds, p0);
    const int a = pass * I.kpass;
    if (a >= I.K) continue;
    const int k = I.kpass < I.K - a ? I.kpass : I.K - a;
    const bool last = a + k == I.K;
    const int64_t need = (1ll << I.K) * p0;
    PDD_REQUIRE(pass == 0 || (ws_in && slot >= need), "pdd_ffa_pass: workspace (in) missing or short");
    PDD_REQUIRE(last || (ws_out && slot >= need), "pdd_ffa_pass: workspace (out) missing or short");
    PDD_REQUIRE(ffa_pass_lds(p0, k) <= kFfaLds, "pdd_ffa_pass: pass does not fit in LDS");
    if (ffa_pass_lds(p0, k) > lds) lds = ffa_pass_lds(p0, k);
    if (((1ll << I.K) >> k) > gx) gx = (1ll << I.K) >> k;
    if (last) prof_slot = need;
  }
  if (D == 0 || gx == 0) return 0;
  PDD_REQUIRE(gx < (1ll << 31), "pdd_ffa_pass: too large");
  A.y = y;
  A.n_ds = n_ds;
  A.ld = ld;
  A.p_lo = p_lo;
  A.np = np;
  A.pass = pass;
  A.ws_in = ws_in;
  A.ws_out = ws_out;
  A.slot = slot;
  A.sigma = sigma;
  A.toff = toff;
  A.snr = snr;
  A.widx = widx;
  A.ntrial = ntrial;
  A.prof = prof;
  A.prof_slot = prof_slot;
  A.ducy = ducy_max;
  if (lds > 64 * 1024) {
    // (more than the default 64 KiB of dynamic LDS: raised once to the most a pass takes)
    static bool raised = false;
    if (!raised) {
      PDD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ffa_pass),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kFfaLds));
      raised = true;
    }
  }
  k_ffa_pass<<<dim3((unsigned)gx, (unsigned)(D * np)), kFfaThreads, (size_t)lds,
               as_stream(stream)>>>(A);
  PDD_LAUNCHED();
  return 0;
}

int pdd_ffa_search(const float* snr, const uint8_t* widx, int64_t D, int64_t ntrial, int64_t ld,
                   float threshold, int32_t* cands, int64_t max_cands, unsigned long long* count,
                   void* stream) {
  PDD_REQUIRE(snr && widx && count && (cands || max_cands == 0), "pdd_ffa_search: null pointer");
  PDD_REQUIRE(D >= 0 && ntrial >= 0 && ld >= ntrial && ntrial < (1ll << 31) && max_cands >= 0,
              "pdd_ffa_search: bad shape");
  if (D == 0 || ntrial == 0) return 0;
  const int64_t nblk = cdiv(ntrial, kFfaTile);
  PDD_REQUIRE(D * nblk < (1ll << 31), "pdd_ffa_search: too large");
  k_ffa_search<<<(unsigned)(D * nblk), 256, 0, as_stream(stream)>>>(snr, widx, ntrial, ld,
                                                                   threshold, nblk, cands,
                                                                   max_cands, count);
  PDD_LAUNCHED();
  return 0;
}

}  // extern "C"
