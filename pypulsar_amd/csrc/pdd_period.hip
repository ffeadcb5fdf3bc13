// libpdd: periodicity search of a DM-time plane -- mean removal + zero
// padding, running-median whitening of the power spectrum and fused
// harmonic-sum candidate search.  gfx950.
//
// The arithmetic is the reference's: PrestoFFT.deredden
// (formats/prestofft.py:151-195, PRESTO's running-median whitening with block
// lengths int(initialbuflen * ln(offset))) and PrestoFFT.harmonic_sum
// (:98-113, S_H[k] = sum_{h=1..H} P[h k] for k < nn / H), restated in
// tests/period_oracle.py.  The FFT between k_ps_prep and the rest is rocFFT
// through torch.fft.rfft (pypulsar_amd/periodicity.py); spectra are
// interleaved (re, im) float32 pairs, row stride ld in COMPLEX elements, of
// which the first nn = nfft / 2 bins are used (PRESTO's packed layout drops
// the Nyquist bin).
//
// Departures from the reference:
//   * rows are zero padded AFTER their mean is removed (PRESTO pads with the
//     mean before the FFT);
//   * where the whitening level of a bin is <= 0 or NaN (a dead row) the
//     normalised power and spectrum are 0, not inf/NaN.
//
// Kernels:
//   k_ps_prep      one block per row: float64 mean in a fixed order (thread-
//                  strided partial sums, LDS tree), then
//                  float32(double(x) - mean) and the zero padding
//   k_ps_medians   one wave per (row, block of <= 256 bins): powers into LDS,
//                  exact selection by counting the smaller and the
//                  smaller-or-equal elements, np.median's rule
//   k_ps_normalise 1024 bins per workgroup: the blocks of its first and last
//                  bin by a 64-way search of the offset table, the lines of
//                  the blocks between them staged in LDS, each bin's block
//                  by a search there; the reference's line between
//                  consecutive block levels
//   k_ps_harmsum   one thread per output bin, harmonics gathered at stride h
//   k_ps_search    one thread per bin (+ one halo bin on each side of a
//                  workgroup): the harmonic sums of all stages cumulatively in
//                  ascending h (the bits of k_ps_harmsum), neighbours through
//                  LDS, candidates through one atomic counter
#include <cmath>

#include "pdd_internal.h"

namespace pdd {

namespace {

constexpr int kPsThreads = 256;
constexpr int kPsMaxBlock = 256;   // longest whitening block (maxbuflen)
constexpr int kPsMaxStages = 8;
constexpr int kPsMaxHarm = 32;
constexpr int kPsTile = kPsThreads - 2;  // bins per k_ps_search workgroup (2 halo threads)
constexpr int kPsNormTile = 4 * kPsThreads;  // bins per k_ps_normalise workgroup

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Stages {
  int n;
  int h[kPsMaxStages];
  float thr[kPsMaxStages];
};

__global__ __launch_bounds__(kPsThreads) void k_ps_prep(const float* __restrict__ x, int64_t n,
                                                        int64_t ld, int64_t nfft,
                                                        float* __restrict__ out) {
  __shared__ double part[kPsThreads];
  const int tid = threadIdx.x;
  const float* row = x + (int64_t)blockIdx.x * ld;
  float* orow = out + (int64_t)blockIdx.x * nfft;
  // thread t sums samples t + 256 i, those with i % 4 == u into partial sum u
  // in ascending i; the partial sums are combined in a fixed order and the
  // threads' by a fixed binary tree: one association, whatever the schedule
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  int64_t t = tid;
  for (; t + 3 * kPsThreads < n; t += 4 * kPsThreads) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = row[t + u * kPsThreads];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] += (double)v[u];
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (t + u * kPsThreads < n) a[u] += (double)row[t + u * kPsThreads];
  const double s = (a[0] + a[1]) + (a[2] + a[3]);
  part[tid] = s;
  __syncthreads();
  for (int o = kPsThreads / 2; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  const double mean = part[0] / (double)n;
  for (t = tid; t < nfft; t += kPsThreads)
    orow[t] = t < n ? (float)((double)row[t] - mean) : 0.f;
}

// med[d][j] = np.median(P[offs[j] : offs[j] + lens[j]]) / ln 2.  With
// less = #{q : P[q] < v} and leq = #{q : P[q] <= v}, the value v is the order
// statistic r exactly when less <= r < leq (ties share their ranks): the
// statistics (len - 1) / 2 and len / 2 are the middle ones (the same for an
// odd length).  A block holding a NaN, or a table entry outside [0, nn) or
// longer than 256, gives NaN (normalised to 0 later).
__global__ __launch_bounds__(kPsThreads) void k_ps_medians(const float* __restrict__ spec,
                                                           int64_t D, int64_t nn, int64_t ld,
                                                           const int32_t* __restrict__ offs,
                                                           const int32_t* __restrict__ lens,
                                                           int64_t B, float* __restrict__ med) {
  __shared__ __attribute__((aligned(16))) float P[kPsThreads / 64][kPsMaxBlock];
  __shared__ float mid[kPsThreads / 64][2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t item = (int64_t)blockIdx.x * (kPsThreads / 64) + wv;
  const bool live = item < D * B;
  const int64_t d = live ? item / B : 0, j = live ? item % B : 0;
  int64_t off = offs[j];
  int len = lens[j];
  const bool ok = live && len >= 1 && len <= kPsMaxBlock && off >= 0 && off + len <= nn;
  if (!ok) len = 0;
  const f32x2* row = reinterpret_cast<const f32x2*>(spec) + d * ld;
  for (int i = lane; i < len; i += 64) {
    const f32x2 z = row[off + i];
    P[wv][i] = z.x * z.x + z.y * z.y;
  }
  if (lane < 2) mid[wv][lane] = NAN;
  __syncthreads();
  const int lo = (len - 1) / 2, hi = len / 2;
  const int len4 = len & ~3;
  bool bad = false;
  for (int i = lane; i < len; i += 64) {
    const float v = P[wv][i];
    int less = 0, leq = 0;
    for (int q = 0; q < len4; q += 4) {  // (the same address in every lane: a broadcast)
      const f32x4 u = *reinterpret_cast<const f32x4*>(&P[wv][q]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        less += u[e] < v ? 1 : 0;
        leq += u[e] <= v ? 1 : 0;
      }
    }
    for (int q = len4; q < len; ++q) {
      const float u = P[wv][q];
      less += u < v ? 1 : 0;
      leq += u <= v ? 1 : 0;
    }
    // (a NaN compares false with everything, so the counts are no ranks any
    // more: the block's level is NaN)
    bad |= !(v == v);
    if (less <= lo && lo < leq) mid[wv][0] = v;  // (lanes of equal v store the same bits)
    if (less <= hi && hi < leq) mid[wv][1] = v;
  }
  const bool nan = __any(bad);
  __syncthreads();
  if (live && lane == 0) {
    const float m = (mid[wv][0] + mid[wv][1]) * 0.5f;
    med[item] = (nan || !ok) ? NAN : m / 0.69314718055994530942f;
  }
}

// The last block j of [0, B) with offs[j] <= q (0 when q < offs[0]; offs
// ascends), by a 64-way search: every lane of the wave probes one entry per
// step, so a table of 4096 blocks takes 2 dependent loads, not 12.  The
// whole wave must call it (with a wave-uniform q).
__device__ __forceinline__ int ps_find_block(const int32_t* __restrict__ offs, int B, int64_t q) {
  const int lane = threadIdx.x & 63;
  int lo = 0, n = B;
  while (n > 1) {
    const int stride = (n + 63) >> 6;
    const int idx = lo + lane * stride;
    const bool le = idx < lo + n && offs[idx] <= q;
    const int c = __popcll(__ballot(le));  // (the lanes with offs <= q are a prefix)
    if (c == 0) return lo;
    const int end = lo + n;
    lo += (c - 1) * stride;
    n = min(stride, end - lo);
  }
  return lo;
}

// The reference's correction of block j < B - 1 at offset i within it:
//   lineval = med[j] + slope * (0.5 (lens[j] + lens[j+1]) - i),
//   slope = (med[j+1] - med[j]) / (lens[j] + lens[j+1]);
// bins from offs[B-1] on use the last lineval of block B - 2; bin 0 is 1.
// A workgroup takes 1024 consecutive bins (thread t: bins t + 256 u); the
// blocks of its first and last bin bound each bin's own search.
__global__ __launch_bounds__(kPsThreads) void k_ps_normalise(
    const float* __restrict__ spec, int64_t nn, int64_t ld, const int32_t* __restrict__ offs,
    const int32_t* __restrict__ lens, int B, const float* __restrict__ med, int64_t nblk,
    float* __restrict__ powers, float* __restrict__ spec_out) {
  // the tile's blocks staged in LDS (at most one per bin, + 1): start, level,
  // slope and half span of the line each applies
  __shared__ int s_off[kPsNormTile + 1];
  __shared__ float s_m0[kPsNormTile + 1], s_slope[kPsNormTile + 1], s_half[kPsNormTile + 1];
  const int64_t d = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int64_t k0 = blk * kPsNormTile;
  const int jlo = ps_find_block(offs, B, k0);
  const int jhi = ps_find_block(offs, B, k0 + kPsNormTile - 1);
  const int nb = max(1, min(jhi - jlo + 1, kPsNormTile + 1));
  const int ilast = lens[B - 2] - 1;  // the offset bins from offs[B-1] on use, in block B - 2
  for (int t = threadIdx.x; t < nb; t += kPsThreads) {
    const int j = jlo + t;             // (<= jhi <= B - 1)
    const int jj = min(j, B - 2);      // the block whose line the bins of block j use
    const float m0 = med[d * B + jj], m1 = med[d * B + jj + 1];
    const float tot = (float)(lens[jj] + lens[jj + 1]);
    s_off[t] = offs[j];
    s_m0[t] = m0;
    s_slope[t] = (m1 - m0) / tot;
    s_half[t] = 0.5f * tot;
  }
  __syncthreads();
  const f32x2* row = reinterpret_cast<const f32x2*>(spec) + d * ld;
  f32x2* orow = spec_out ? reinterpret_cast<f32x2*>(spec_out) + d * nn : nullptr;
#pragma unroll
  for (int u = 0; u < kPsNormTile / kPsThreads; ++u) {
    const int64_t k = k0 + threadIdx.x + u * kPsThreads;
    if (k >= nn) break;
    float p = 1.f;
    f32x2 z = {1.f, 0.f};
    if (k > 0) {
      z = row[k];
      int lo = 0, hi = nb - 1;  // the last staged block with s_off <= k
      while (lo < hi) {
        const int m = (lo + hi + 1) >> 1;
        if (s_off[m] <= k) lo = m; else hi = m - 1;
      }
      // (bins before offs[0] other than 0: none for offs[0] == 1)
      const int i = jlo + lo >= B - 1 ? ilast : max((int)(k - s_off[lo]), 0);
      const float lineval = s_m0[lo] + s_slope[lo] * (s_half[lo] - (float)i);
      if (lineval > 0.f) {
        p = (z.x * z.x + z.y * z.y) / lineval;
        const float s = 1.f / sqrtf(lineval);
        z.x *= s;
        z.y *= s;
      } else {
        p = z.x = z.y = 0.f;
      }
    }
    powers[d * nn + k] = p;
    if (orow) orow[k] = z;
  }
}

__global__ __launch_bounds__(kPsThreads) void k_ps_harmsum(const float* __restrict__ powers,
                                                           int64_t ld, int nharm, int64_t nout,
                                                           int64_t nblk, float* __restrict__ out) {
  const int64_t d = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int64_t k = blk * kPsThreads + threadIdx.x;
  if (k >= nout) return;
  const float* row = powers + d * ld;
  float s = row[k];
  for (int h = 2; h <= nharm; ++h) s += row[h * k];  // (h k <= nharm (nout - 1) < nn)
  out[d * nout + k] = s;
}

// Thread t of workgroup blk holds bin k = blk * 254 - 1 + t: threads 1..254
// own a bin, threads 0 and 255 are the neighbours of the first and last.
// The loads of a stage's harmonics are independent (lanes hold consecutive k,
// harmonic h at stride h); the sum is taken in ascending h.
__global__ __launch_bounds__(kPsThreads) void k_ps_search(
    const float* __restrict__ powers, int64_t nn, int64_t ld, Stages S, int64_t rlo, int64_t nblk,
    int32_t* __restrict__ cands, int64_t max_cands, unsigned long long* __restrict__ count) {
  __shared__ float sh[kPsThreads];
  const int tid = threadIdx.x;
  const int64_t d = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int64_t kfirst = rlo + blk * kPsTile;  // the workgroup's first owned bin
  const int64_t k = kfirst - 1 + tid;
  const float* row = powers + d * ld;
  float s = 0.f;
  int hdone = 0;
  for (int si = 0; si < S.n; ++si) {
    const int H = S.h[si];
    const int64_t kend = nn / H;   // stage H searches [rlo, kend)
    if (kfirst >= kend) break;     // uniform over the workgroup (and for every later stage)
    const bool in = k >= rlo && k < kend;
    if (in) {
      for (int h0 = hdone + 1; h0 <= H; h0 += 8) {  // (h, H uniform: scalar branches)
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = h0 + q <= H ? row[(h0 + q) * k] : 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q)
          if (h0 + q <= H) s += v[q];  // (h k <= H (kend - 1) < nn)
      }
    }
    hdone = H;
    sh[tid] = in ? s : -INFINITY;
    __syncthreads();
    if (in && tid >= 1 && tid <= kPsTile && s >= S.thr[si] && s > sh[tid - 1] &&
        s >= sh[tid + 1]) {
      const unsigned long long slot = atomicAdd(count, 1ull);
      if ((int64_t)slot < max_cands) {
        int32_t* c = cands + slot * 4;
        c[0] = (int32_t)d;
        c[1] = (int32_t)k;
        c[2] = H;
        c[3] = __float_as_int(s);
      }
    }
    __syncthreads();
  }
}

}  // namespace

}  // namespace pdd

using namespace pdd;

extern "C" {

int pdd_ps_prep(const float* x, int64_t D, int64_t n, int64_t ld, int64_t nfft, float* out,
                void* stream) {
  PDD_REQUIRE(x && out, "pdd_ps_prep: null pointer");
  PDD_REQUIRE(D >= 0 && n > 0 && ld >= n && nfft >= n, "pdd_ps_prep: bad shape");
  PDD_REQUIRE(D < (1ll << 31), "pdd_ps_prep: too large");
  if (D == 0) return 0;
  k_ps_prep<<<(unsigned)D, kPsThreads, 0, as_stream(stream)>>>(x, n, ld, nfft, out);
  PDD_LAUNCHED();
  return 0;
}

int pdd_ps_block_medians(const float* spec, int64_t D, int64_t nn, int64_t ld, const int32_t* offs,
                         const int32_t* lens, int64_t B, float* med, void* stream) {
  PDD_REQUIRE(spec && offs && lens && med, "pdd_ps_block_medians: null pointer");
  PDD_REQUIRE(D >= 0 && nn > 0 && ld >= nn && B >= 1 && nn < (1ll << 31),
              "pdd_ps_block_medians: bad shape");
  PDD_REQUIRE(((uintptr_t)spec & 7) == 0, "pdd_ps_block_medians: spec must be 8-byte aligned");
  const int64_t blocks = cdiv(D * B, kPsThreads / 64);
  PDD_REQUIRE(blocks < (1ll << 31), "pdd_ps_block_medians: too large");
  if (D == 0) return 0;
  k_ps_medians<<<(unsigned)blocks, kPsThreads, 0, as_stream(stream)>>>(spec, D, nn, ld, offs, lens,
                                                                      B, med);
  PDD_LAUNCHED();
  return 0;
}

int pdd_ps_normalise(const float* spec, int64_t D, int64_t nn, int64_t ld, const int32_t* offs,
                     const int32_t* lens, int64_t B, const float* med, float* powers_out,
                     float* spec_out, void* stream) {
  PDD_REQUIRE(spec && offs && lens && med && powers_out, "pdd_ps_normalise: null pointer");
  PDD_REQUIRE(D >= 0 && nn > 0 && ld >= nn && nn < (1ll << 31), "pdd_ps_normalise: bad shape");
  PDD_REQUIRE(B >= 2 && B < (1ll << 31), "pdd_ps_normalise: needs at least 2 blocks");
  PDD_REQUIRE(((uintptr_t)spec & 7) == 0 && ((uintptr_t)spec_out & 7) == 0,
              "pdd_ps_normalise: spectra must be 8-byte aligned");
  const int64_t nblk = cdiv(nn, kPsNormTile);
  PDD_REQUIRE(D * nblk < (1ll << 31), "pdd_ps_normalise: too large");
  if (D == 0) return 0;
  k_ps_normalise<<<(unsigned)(D * nblk), kPsThreads, 0, as_stream(stream)>>>(
      spec, nn, ld, offs, lens, (int)B, med, nblk, powers_out, spec_out);
  PDD_LAUNCHED();
  return 0;
}

int pdd_ps_harmsum(const float* powers, int64_t D, int64_t nn, int64_t ld, int nharm, float* out,
                   void* stream) {
  PDD_REQUIRE(powers && out, "pdd_ps_harmsum: null pointer");
  PDD_REQUIRE(D >= 0 && nn > 0 && ld >= nn && nn < (1ll << 31), "pdd_ps_harmsum: bad shape");
  PDD_REQUIRE(nharm >= 1 && nharm <= kPsMaxHarm, "pdd_ps_harmsum: nharm out of range 1..%d",
              kPsMaxHarm);
  const int64_t nout = nn / nharm;
  const int64_t nblk = cdiv(nout, kPsThreads);
  PDD_REQUIRE(D * nblk < (1ll << 31), "pdd_ps_harmsum: too large");
  if (D == 0 || nout == 0) return 0;
  k_ps_harmsum<<<(unsigned)(D * nblk), kPsThreads, 0, as_stream(stream)>>>(powers, ld, nharm, nout,
                                                                          nblk, out);
  PDD_LAUNCHED();
  return 0;
}

int pdd_ps_search(const float* powers, int64_t D, int64_t nn, int64_t ld, const int32_t* harms,
                  int n_harms, const float* thr, int64_t rlo, int32_t* cands, int64_t max_cands,
                  unsigned long long* count, void* stream) {
  PDD_REQUIRE(powers && harms && thr && count && (cands || max_cands == 0),
              "pdd_ps_search: null pointer");
  PDD_REQUIRE(D >= 0 && nn > 0 && ld >= nn && nn < (1ll << 31) && max_cands >= 0,
              "pdd_ps_search: bad shape");
  PDD_REQUIRE(rlo >= 1, "pdd_ps_search: rlo must be >= 1");
  PDD_REQUIRE(n_harms >= 1 && n_harms <= kPsMaxStages, "pdd_ps_search: 1..%d stages",
              kPsMaxStages);
  Stages S;
  S.n = n_harms;
  for (int i = 0; i < n_harms; ++i) {
    PDD_REQUIRE(harms[i] >= 1 && harms[i] <= kPsMaxHarm,
                "pdd_ps_search: harmonic count %d out of range 1..%d", harms[i], kPsMaxHarm);
    PDD_REQUIRE(i == 0 || harms[i] > harms[i - 1], "pdd_ps_search: harms must ascend");
    S.h[i] = harms[i];
    S.thr[i] = thr[i];
  }
  const int64_t kend = nn / harms[0];  // the widest stage's range
  if (D == 0 || rlo >= kend) return 0;
  const int64_t nblk = cdiv(kend - rlo, kPsTile);
  PDD_REQUIRE(D * nblk < (1ll << 31), "pdd_ps_search: too large");
  k_ps_search<<<(unsigned)(D * nblk), kPsThreads, 0, as_stream(stream)>>>(
      powers, nn, ld, S, rlo, nblk, cands, max_cands, count);
  PDD_LAUNCHED();
  return 0;
}

}  // extern "C"
