// libpdd: sideband search for pulsars in binaries shorter than the
// observation (Ransom, Cordes & Eikenberry 2003; PRESTO's search_bin) --
// short real FFTs of overlapping stretches of the whitened power spectrum,
// their normalised half-bin power spectra ("mini spectra"), harmonic stages
// and candidates, fused in one kernel per mini-FFT length.  gfx950, wave64.
//
// Definition (restated in tests/sideband_oracle.py).  For a
// row of whitened powers P[0..nn), L = 2^log2L and stride = L >> shift,
// segment j < nseg = (nn - rlo - L) / stride + 1 starts at lo_j = rlo + j
// stride.  With x_i = min(P[lo + i], clip) (clip > 0) and A_k = sum_i x_i
// exp(-2 pi i i k / L), k = 0..L/2:
//   M[2k]     = L |A_k|^2 / A_0^2
//   M[2k + 1] = (pi^2 / 16) L |A_k - A_{k+1}|^2 / A_0^2      (interbinning)
// (all 0 where A_0 <= 0: a dead row).  S_H[q] = sum_{h=1..H} M[h q] for q <
// L / H in float32, ascending h; q of [qlo, L / H) is a candidate of stage H
// when S_H[q] >= thr, > S_H[q-1] and >= S_H[q+1], neighbours outside the
// range counting as -inf (pdd_ps_search's rule).
//
// k_sb_search<LOG2L>, one instance per length 32..16384:
//   * TS = min(L / 8, 1024) threads work on a segment (one radix-4 butterfly
//     of the L/2-point complex FFT each, two at L = 16384); a workgroup of
//     max(256, TS) threads takes G = 2048 / L (>= 1) consecutive segments of
//     one row, so every lane has a butterfly in every pass;
//   * G > 1: the segments' common window of (G - 1) stride + L powers is
//     loaded once (coalesced, clipped) into LDS and the first pass of each
//     segment reads it there; G == 1: the segment goes straight into the
//     first FFT buffer.  No lane reads a column >= nn;
//   * the real FFT is the complex FFT of z_j = x_2j + i x_2j+1 (the window
//     itself, read as float pairs): Stockham autosort, radix-4 passes between
//     two LDS buffers (a pass reads element b + k L/8, k < 4, of butterfly b:
//     consecutive lanes, consecutive addresses) and one radix-2 pass where
//     log2(L/2) is odd; twiddles from the caller's float32 table of (cos,
//     sin)(2 pi j / L), j < L/2, the other half by negation;
//   * complex element i of a buffer lives at i + (i >> 4): the writes of the
//     first two passes (strides 4 and 16 elements) would otherwise fall 4-way
//     on the 32 store banks; float i of M and S_H lives at i + (i >> 5), which
//     spreads the stride-H gathers of the stages;
//   * the split pass A_k = E_k - i w^k O_k and the two powers per k go
//     straight into the idle buffer as M; S_H goes into the other one; the
//     local maxima are read from there and appended with one atomic per wave.
// LDS per workgroup: 8.5 L bytes a segment + the window (DESIGN §6q has the
// table; 136 KiB at L = 16384, set through the dynamic-LDS attribute).
// Everything runs in a fixed order: the dump is the same bits every launch.
#include <cmath>

#include "pdd_internal.h"

namespace pdd {

namespace {

constexpr int kSbMinLog2 = 5, kSbMaxLog2 = 14;
constexpr int kSbMaxStages = 4;
constexpr int kSbMaxHarm = 8;
constexpr float kSbInterbin = 0.61685027506808491368f;  // pi^2 / 16

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct SbStages {
  int n;
  int h[kSbMaxStages];
  float thr[kSbMaxStages];
};

template <int LOG2L>
struct SbCfg {
  static constexpr int L = 1 << LOG2L;
  static constexpr int N = L / 2;                    // complex points
  static constexpr int LOG2N = LOG2L - 1;
  static constexpr int NB = N / 4;                   // radix-4 butterflies a pass
  static constexpr int TS = NB < 1024 ? NB : 1024;   // threads a segment
  static constexpr int BLOCK = TS < 256 ? 256 : TS;  // threads a workgroup
  static constexpr int G = BLOCK / TS;               // segments a workgroup
  static constexpr int CBUF = N + (N >> 4);          // padded complex elements a buffer
};

__host__ __device__ constexpr int sb_round4(int v) { return (v + 3) & ~3; }

// floats of the window region of a workgroup (none where it holds one segment)
template <int LOG2L>
__host__ __device__ constexpr int sb_window_floats(int shift) {
  using C = SbCfg<LOG2L>;
  return C::G > 1 ? sb_round4((C::G - 1) * (C::L >> shift) + C::L) : 0;
}

template <int LOG2L>
constexpr size_t sb_lds_bytes(int shift) {
  using C = SbCfg<LOG2L>;
  return sizeof(float) * ((size_t)sb_window_floats<LOG2L>(shift) + 2u * C::G * 2u * C::CBUF);
}

__device__ __forceinline__ int sb_padc(int i) { return i + (i >> 4); }  // complex elements
__device__ __forceinline__ int sb_padf(int i) { return i + (i >> 5); }  // floats

__device__ __forceinline__ f32x2 sb_cmul(f32x2 a, f32x2 w) {
  f32x2 r;
  r.x = a.x * w.x - a.y * w.y;
  r.y = a.x * w.y + a.y * w.x;
  return r;
}

// exp(-2 pi i j / L) for j < L from the table of (cos, sin)(2 pi j / L), j < L / 2
template <int L>
__device__ __forceinline__ f32x2 sb_twiddle(const f32x2* __restrict__ tw, int j) {
  const bool up = j >= L / 2;
  const f32x2 c = tw[up ? j - L / 2 : j];
  f32x2 w;
  w.x = up ? -c.x : c.x;
  w.y = up ? c.y : -c.y;
  return w;
}

// A_k, 0 <= k <= N, of the real sequence whose packed complex FFT is Z (padded)
template <int LOG2L>
__device__ __forceinline__ f32x2 sb_real_bin(const f32x2* Z, const f32x2* __restrict__ tw, int k) {
  using C = SbCfg<LOG2L>;
  const f32x2 a = Z[sb_padc(k & (C::N - 1))];
  f32x2 b = Z[sb_padc((C::N - k) & (C::N - 1))];
  b.y = -b.y;
  f32x2 c;  // (cos, sin)(2 pi k / L); k == N: (-1, 0)
  if (k < C::N) {
    c = tw[k];
  } else {
    c.x = -1.f;
    c.y = 0.f;
  }
  const f32x2 e = (a + b) * 0.5f, o = (a - b) * 0.5f;
  // -i w^k = -sin - i cos
  f32x2 r;
  r.x = e.x + (o.y * c.x - o.x * c.y);
  r.y = e.y - (o.y * c.y + o.x * c.x);
  return r;
}

template <int LOG2L>
__global__ __launch_bounds__(SbCfg<LOG2L>::BLOCK) void k_sb_search(
    const float* __restrict__ powers, int64_t nn, int64_t ld, int64_t rlo, int shift, float clip,
    SbStages S, int qlo, const f32x2* __restrict__ tw, int64_t nseg, int64_t nblk,
    float* __restrict__ mini, int32_t* __restrict__ cands, int64_t max_cands,
    unsigned long long* __restrict__ count) {
  using C = SbCfg<LOG2L>;
  constexpr int L = C::L, N = C::N, NB = C::NB, TS = C::TS;
  extern __shared__ __attribute__((aligned(16))) float sb_smem[];
  const int tid = threadIdx.x;
  const int g = tid / TS, t = tid % TS;
  const int64_t d = blockIdx.x / nblk, blk = blockIdx.x % nblk;
  const int stride = L >> shift;
  const int64_t seg0 = blk * C::G;
  const int gv = (int)(nseg - seg0 < C::G ? nseg - seg0 : C::G);  // live segments (>= 1)
  const int64_t lo0 = rlo + seg0 * stride;
  const float* row = powers + d * ld + lo0;
  const int winf = sb_window_floats<LOG2L>(shift);
  f32x2* const base = reinterpret_cast<f32x2*>(sb_smem + winf);
  f32x2* const b0 = base + (size_t)g * C::CBUF;
  f32x2* const b1 = base + (size_t)(C::G + g) * C::CBUF;

  // ---- the window: columns lo0 .. lo0 + wlen - 1 <= nn - 1 (the last live
  // segment ends at or before nn) ----
  const int wlen = (gv - 1) * stride + L;
  if (C::G > 1) {
    for (int i = tid; i < winf; i += C::BLOCK) {
      float v = 0.f;
      if (i < wlen) {
        v = row[i];
        if (clip > 0.f) v = fminf(v, clip);
      }
      sb_smem[i] = v;
    }
  } else {
    float* f0 = reinterpret_cast<float*>(b0);
    for (int i = tid; i < L; i += C::BLOCK) {
      float v = row[i];
      if (clip > 0.f) v = fminf(v, clip);
      f0[i + 2 * (i >> 5)] = v;  // float c of complex j = i / 2 at 2 padc(j) + c
    }
  }
  __syncthreads();

  // ---- Stockham passes: n = N >> ls points a sub-transform, s = 1 << ls of
  // them interleaved; butterfly b = p s + q reads b + k NB and writes q + s (4
  // p + k) ----
  const f32x2* win = reinterpret_cast<const f32x2*>(sb_smem + g * stride);
  f32x2* src = b0;
  f32x2* dst = C::G > 1 ? b0 : b1;
#pragma unroll
  for (int ls = 0; ls + 2 <= C::LOG2N; ls += 2) {
    const int s = 1 << ls;
    for (int b = t; b < NB; b += TS) {
      f32x2 x0, x1, x2, x3;
      if (ls == 0 && C::G > 1) {
        x0 = win[b];
        x1 = win[b + NB];
        x2 = win[b + 2 * NB];
        x3 = win[b + 3 * NB];
      } else {
        x0 = src[sb_padc(b)];
        x1 = src[sb_padc(b + NB)];
        x2 = src[sb_padc(b + 2 * NB)];
        x3 = src[sb_padc(b + 3 * NB)];
      }
      const int p = b >> ls, q = b & (s - 1);
      const f32x2 apc = x0 + x2, amc = x0 - x2, bpd = x1 + x3, bmd = x1 - x3;
      f32x2 jb;  // i (x1 - x3)
      jb.x = -bmd.y;
      jb.y = bmd.x;
      const int o = q + ((p << 2) << ls);
      f32x2 y1 = amc - jb, y2 = apc - bpd, y3 = amc + jb;
      if (p) {  // (the last pass has p == 0 everywhere: no table read)
        const int j1 = p << (ls + 1);  // p L / n
        y1 = sb_cmul(y1, sb_twiddle<L>(tw, j1));
        y2 = sb_cmul(y2, sb_twiddle<L>(tw, 2 * j1));
        y3 = sb_cmul(y3, sb_twiddle<L>(tw, 3 * j1));
      }
      dst[sb_padc(o)] = apc + bpd;
      dst[sb_padc(o + s)] = y1;
      dst[sb_padc(o + 2 * s)] = y2;
      dst[sb_padc(o + 3 * s)] = y3;
    }
    __syncthreads();
    src = dst;
    dst = dst == b0 ? b1 : b0;
  }
  if (C::LOG2N & 1) {  // the last, radix-2 pass: n = 2, s = N / 2, no twiddle
    for (int b = t; b < N / 2; b += TS) {
      const f32x2 x0 = src[sb_padc(b)], x1 = src[sb_padc(b + N / 2)];
      dst[sb_padc(b)] = x0 + x1;
      dst[sb_padc(b + N / 2)] = x0 - x1;
    }
    __syncthreads();
    src = dst;
    dst = dst == b0 ? b1 : b0;
  }

  // ---- split pass and powers: Z in src, M into dst ----
  float* const M = reinterpret_cast<float*>(dst);
  {
    const f32x2 z0 = src[0];
    const float a0 = z0.x + z0.y;
    const bool live = a0 > 0.f;
    const float scale = live ? (float)L / (a0 * a0) : 0.f;
    for (int k = t; k < N; k += TS) {
      const f32x2 ak = sb_real_bin<LOG2L>(src, tw, k), an = sb_real_bin<LOG2L>(src, tw, k + 1);
      const f32x2 df = ak - an;
      const float m0 = (ak.x * ak.x + ak.y * ak.y) * scale;
      const float m1 = kSbInterbin * ((df.x * df.x + df.y * df.y) * scale);
      M[sb_padf(2 * k)] = live ? m0 : 0.f;
      M[sb_padf(2 * k + 1)] = live ? m1 : 0.f;
    }
  }
  __syncthreads();
  const bool mine = g < gv;
  if (mini && mine) {
    float* out = mini + ((d * nseg + seg0 + g) * (int64_t)L);
    for (int i = t; i < L; i += TS) out[i] = M[sb_padf(i)];
  }

  // ---- stages: S_H into the buffer Z has left, then its local maxima ----
  float* const SH = reinterpret_cast<float*>(const_cast<f32x2*>(src));
  const int lane = tid & 63;
  const int lo = (int)(lo0 + (int64_t)g * stride);
  for (int si = 0; si < S.n; ++si) {
    const int H = S.h[si];
    const int qend = L / H;  // stage H searches [qlo, qend)
    for (int q = t; q <= qend; q += TS) {
      if (q < qlo - 1) continue;
      float v = -INFINITY;
      if (q >= qlo && q < qend) {
        v = M[sb_padf(q)];
        for (int h = 2; h <= H; ++h) v += M[sb_padf(h * q)];  // (h q <= H (qend - 1) < L)
      }
      SH[sb_padf(q)] = v;
    }
    __syncthreads();
    const float thr = S.thr[si];
    for (int q0 = 0; q0 < qend; q0 += TS) {  // (uniform bounds: whole waves reach the ballot)
      const int q = q0 + t;
      bool hit = false;
      float v = 0.f;
      if (mine && q >= qlo && q < qend) {
        v = SH[sb_padf(q)];
        hit = v >= thr && v > SH[sb_padf(q - 1)] && v >= SH[sb_padf(q + 1)];
      }
      const unsigned long long mask = __ballot(hit);
      if (mask) {
        const int leader = __ffsll((long long)mask) - 1;
        unsigned long long slot0 = 0;
        if (lane == leader) slot0 = atomicAdd(count, (unsigned long long)__popcll(mask));
        slot0 = __shfl(slot0, leader);
        if (hit) {
          const unsigned long long slot = slot0 + __popcll(mask & ((1ull << lane) - 1ull));
          if ((int64_t)slot < max_cands) {
            int32_t* c = cands + slot * 6;
            c[0] = (int32_t)d;
            c[1] = LOG2L;
            c[2] = lo;
            c[3] = q;
            c[4] = H;
            c[5] = __float_as_int(v);
          }
        }
      }
    }
    __syncthreads();
  }
}

template <int LOG2L>
int sb_launch(const float* powers, int64_t D, int64_t nn, int64_t ld, int64_t rlo, int shift,
              float clip, const SbStages& S, int qlo, const float* twiddle, int64_t nseg,
              float* mini, int32_t* cands, int64_t max_cands, unsigned long long* count,
              hipStream_t st) {
  using C = SbCfg<LOG2L>;
  const int64_t nblk = cdiv(nseg, C::G);
  PDD_REQUIRE(D * nblk < (1ll << 31), "pdd_sb_search: too large");
  const size_t lds = sb_lds_bytes<LOG2L>(shift);
  if (lds > 64 * 1024)
    PDD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sb_search<LOG2L>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  k_sb_search<LOG2L><<<(unsigned)(D * nblk), C::BLOCK, lds, st>>>(
      powers, nn, ld, rlo, shift, clip, S, qlo, reinterpret_cast<const f32x2*>(twiddle), nseg,
      nblk, mini, cands, max_cands, count);
  PDD_LAUNCHED();
  return 0;
}

}  // namespace

}  // namespace pdd

using namespace pdd;

extern "C" {

int pdd_sb_search(const float* powers, int64_t D, int64_t nn, int64_t ld, int64_t rlo, int log2L,
                  int shift, float clip, const int32_t* harms, int nharm, const float* thr,
                  int qlo, const float* twiddle, float* mini, int32_t* cands, int64_t max_cands,
                  int64_t* count, void* stream) {
  PDD_REQUIRE(powers && harms && thr && twiddle && count && (cands || max_cands == 0),
              "pdd_sb_search: null pointer");
  PDD_REQUIRE(D >= 0 && nn > 0 && nn < (1ll << 31) && max_cands >= 0, "pdd_sb_search: bad shape");
  PDD_REQUIRE(ld >= nn, "pdd_sb_search: ld must be >= nn");
  PDD_REQUIRE(rlo >= 1, "pdd_sb_search: rlo must be >= 1");
  PDD_REQUIRE(log2L >= kSbMinLog2 && log2L <= kSbMaxLog2, "pdd_sb_search: log2L out of range %d..%d",
              kSbMinLog2, kSbMaxLog2);
  PDD_REQUIRE(shift >= 0 && shift <= 3, "pdd_sb_search: shift out of range 0..3");
  PDD_REQUIRE(nharm >= 1 && nharm <= kSbMaxStages, "pdd_sb_search: 1..%d stages", kSbMaxStages);
  PDD_REQUIRE(clip >= 0.f, "pdd_sb_search: clip must be >= 0 (0: none)");
  SbStages S;
  S.n = nharm;
  for (int i = 0; i < kSbMaxStages; ++i) {
    S.h[i] = 1;
    S.thr[i] = 0.f;
  }
  for (int i = 0; i < nharm; ++i) {
    PDD_REQUIRE(harms[i] >= 1 && harms[i] <= kSbMaxHarm,
                "pdd_sb_search: harmonic count %d out of range 1..%d", harms[i], kSbMaxHarm);
    PDD_REQUIRE(i == 0 || harms[i] > harms[i - 1], "pdd_sb_search: harms must ascend");
    S.h[i] = harms[i];
    S.thr[i] = thr[i];
  }
  const int64_t L = 1ll << log2L;
  // (qlo == L / 8, the default 4 at L = 32, leaves a stage of 8 harmonics an empty range)
  PDD_REQUIRE(qlo >= 1 && qlo <= L / 8, "pdd_sb_search: qlo out of range 1..L/8");
  PDD_REQUIRE(((uintptr_t)twiddle & 7) == 0, "pdd_sb_search: twiddle must be 8-byte aligned");
  if (D == 0 || nn - rlo < L) return 0;
  const int64_t stride = L >> shift;
  const int64_t nseg = (nn - rlo - L) / stride + 1;
  hipStream_t st = as_stream(stream);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(count);
#define PDD_SB_CASE(E)                                                                          \
  case E:                                                                                       \
    return sb_launch<E>(powers, D, nn, ld, rlo, shift, clip, S, qlo, twiddle, nseg, mini, cands, \
                        max_cands, cnt, st);
  switch (log2L) {
    PDD_SB_CASE(5)
    PDD_SB_CASE(6)
    PDD_SB_CASE(7)
    PDD_SB_CASE(8)
    PDD_SB_CASE(9)
    PDD_SB_CASE(10)
    PDD_SB_CASE(11)
    PDD_SB_CASE(12)
    PDD_SB_CASE(13)
    PDD_SB_CASE(14)
  }
#undef PDD_SB_CASE
  return -1;
}

}  // extern "C"
