// libpdd: RFI excision on the raw time-major block -- the per (interval,
// channel) statistics an rfifind-style mask is decided from, and the in-place
// replacement of masked cells in the streaming path.  gfx950.
//
// Definitions (restated in tests/rfi_oracle.py): the block
// x[t][c] is cut into intervals of P = ptsperint samples; for interval i and
// channel c over its N = P samples
//   avg = sum x / N,  var = population variance,  std = sqrt(var),
//   pow = max_{k=1..P/2} |rfft(x - avg)[k]|^2 / (P var)   (0 where var == 0).
// 8-bit input: S1 = sum x and S2 = sum x^2 are exact integers,
//   avg = double(S1) / double(N),  var = double(N S2 - S1 S1) / double(N N).
// float32 input: the sums of d = x - pivot and of d d are taken in double,
//   avg = pivot + sum d / N,  var = max(sum d d / N - (sum d / N)^2, 0).
//
// Kernels:
//   k_rfi_prep<T>   pass (a).  One workgroup owns (interval, tile of 8 V
//                   channels, one of S spans of the interval's samples), V =
//                   16 / sizeof(T) the channels of one 16-byte load: 128 B of
//                   every raw row, the whole tile read once.  S is chosen so
//                   that a batch of few channels still fills the device; the
//                   spans' sums are added in span order by k_rfi_finish<T>.
//                   Lane (r, l) of the 32 x 8 thread grid loads the 16 bytes
//                   l of row r (8 lanes = 128 contiguous bytes a row, 8 rows a
//                   wave instruction), adds them to its V pairs of sums, and
//                   puts x - pivot as float into the LDS tile [channel][64
//                   times]; the tile then leaves as float4 along time, 16
//                   lanes = 256 contiguous bytes of one output row.  LDS: time
//                   index rotated by 4 l per lane column, so the 32 lanes of a
//                   ds_write_b32 half (4 rows x 8 lanes) fall on banks
//                   (r + 4 l) mod 32, all distinct, and a ds_read_b128 row
//                   (16 lanes, 256 B) covers the 64 banks once.
//                   pivot: the (rounded, for 8 bits) mean of the row's first
//                   <= 64 samples.  Bins k >= 1 of the transform do not depend
//                   on the constant removed; the pivot keeps the float32
//                   rounding at the scale of the fluctuations without a second
//                   read of the interval (the exact mean is known only after
//                   the last sample).
//   k_rfi_power     pass (b).  One wave per spectrum row: the largest
//                   re^2 + im^2 of bins 1..P/2 read as 16-byte pairs of bins,
//                   reduced over the wave, divided by P var.  No power array.
//   k_rfi_apply<T>  one thread per (32-channel bitmap word, 8 rows): words
//                   that are zero -- the common case -- touch no data; others
//                   read-modify-write 16-byte pieces (scalar stores where a
//                   piece is unaligned or crosses the last channel).
#include <cmath>

#include "pdd_internal.h"

namespace pdd {

namespace {

constexpr int kRfiThreads = 256;
constexpr int kRfiLanes = 8;                       // 16-byte loads per raw row of a tile
constexpr int kRfiRows = kRfiThreads / kRfiLanes;  // raw rows per pass of the workgroup
constexpr int kRfiTT = 64;                         // times per LDS tile (two passes)
constexpr int kRfiApplyRows = 8;                   // rows per k_rfi_apply thread
constexpr int kRfiTargetBlocks = 2048;             // k_rfi_prep workgroups aimed at (8 a CU)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <typename T>
struct RfiTraits;
template <>
struct RfiTraits<uint8_t> {
  static constexpr int V = 16;
  typedef uint32_t Sum1;            // per thread: <= 255 P / 32
  typedef unsigned long long Sum2;  // sums of squares
};
template <>
struct RfiTraits<float> {
  static constexpr int V = 4;
  typedef double Sum1;
  typedef double Sum2;
};

// The V elements of a 16-byte piece starting at channel c (nv of them valid)
// as floats; `vec`: the piece is 16-byte aligned.
__device__ __forceinline__ void rfi_load(const uint8_t* p, int nv, bool vec, float (&v)[16]) {
  if (vec && nv == 16) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = (float)((w[j >> 2] >> (8 * (j & 3))) & 0xffu);
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = j < nv ? (float)p[j] : 0.f;
  }
}
__device__ __forceinline__ void rfi_load(const float* p, int nv, bool vec, float (&v)[4]) {
  if (vec && nv == 4) {
    const f32x4 w = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = w[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[j] : 0.f;
  }
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
  const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t rfi_shfl(uint32_t v, int m) { return __shfl_xor(v, m); }
__device__ __forceinline__ unsigned long long rfi_shfl(unsigned long long v, int m) {
  return shfl_xor_u64(v, m);
}
__device__ __forceinline__ double rfi_shfl(double v, int m) {
  return __longlong_as_double((long long)shfl_xor_u64((unsigned long long)__double_as_longlong(v), m));
}

__device__ __forceinline__ void rfi_finish(uint32_t s1, unsigned long long s2, float /*pivot*/,
                                           int64_t P, double* avg, double* var) {
  const unsigned long long N = (unsigned long long)P, S1 = s1;
  *avg = (double)S1 / (double)N;
  *var = (double)(N * s2 - S1 * S1) / (double)(N * N);
}
__device__ __forceinline__ void rfi_finish(double s1, double s2, float pivot, int64_t P,
                                           double* avg, double* var) {
  const double m = s1 / (double)P;
  *avg = (double)pivot + m;
  *var = fmax(s2 / (double)P - m * m, 0.0);
}

// raw: [nint P][C] (row stride ld elements).  Workgroup ((i ntile + tile) S +
// s): interval i, channels cfirst + tile 8 V ..., samples [s span, (s + 1)
// span) of the interval (span a multiple of 64).  rows: [(c - cfirst) nint +
// i][P] float.  part: [workgroup][2][8 V] sums of the span (8 bits: of x and
// x x; float32: of d = x - pivot and d d); pivots: [i ntile + tile][8 V].
template <typename T>
__global__ __launch_bounds__(kRfiThreads) void k_rfi_prep(
    const T* __restrict__ raw, int64_t nint, int64_t ld, int64_t P, int64_t cfirst,
    int64_t clast, int64_t ntile, int64_t S, int64_t span, bool vec_in, bool vec_out,
    float* __restrict__ rows, typename RfiTraits<T>::Sum2* __restrict__ part,
    float* __restrict__ pivots) {
  constexpr int V = RfiTraits<T>::V;
  constexpr int TC = kRfiLanes * V;
  typedef typename RfiTraits<T>::Sum1 Sum1;
  typedef typename RfiTraits<T>::Sum2 Sum2;
  __shared__ float tile[TC * kRfiTT];
  __shared__ float piv[TC];
  __shared__ Sum1 w1[kRfiThreads / 64][TC];
  __shared__ Sum2 w2[kRfiThreads / 64][TC];
  const int tid = threadIdx.x;
  const int64_t cell = blockIdx.x / S, sp = blockIdx.x % S;
  const int64_t i = cell / ntile;
  const int64_t c0 = cfirst + (cell % ntile) * TC;  // first channel of the tile
  const int64_t tend = (sp + 1) * span < P ? (sp + 1) * span : P;
  const T* base = raw + i * P * ld;
  // pivot of channel c0 + tid: mean of the first <= 64 samples
  if (tid < TC) {
    const int64_t c = c0 + tid;
    float p = 0.f;
    if (c < clast) {
      const int n0 = (int)(P < kRfiTT ? P : kRfiTT);
      float s = 0.f;
      for (int t = 0; t < n0; ++t) s += (float)base[t * ld + c];
      p = s / (float)n0;
      if (sizeof(T) == 1) p = rintf(p);
    }
    piv[tid] = p;
    if (sp == 0) pivots[cell * TC + tid] = p;
  }
  __syncthreads();
  const int l = tid % kRfiLanes, r = tid / kRfiLanes;
  const int64_t cl = c0 + l * V;  // the lane's first channel
  const int nv = (int)(clast - cl < V ? (clast - cl < 0 ? 0 : clast - cl) : V);
  float pv[V];
  Sum1 s1[V];
  Sum2 s2[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    pv[j] = piv[l * V + j];
    s1[j] = 0;
    s2[j] = 0;
  }
  // the read side: channel ch = tid / 16, four times t4 = 4 (tid % 16) a pass
  const int t4 = 4 * (tid % 16), chr = tid / 16;
  for (int64_t tb = sp * span; tb < tend; tb += kRfiTT) {
#pragma unroll
    for (int h = 0; h < kRfiTT / kRfiRows; ++h) {
      const int rr = r + h * kRfiRows;
      const int64_t t = tb + rr;
      float v[V];
      if (t < tend && nv > 0) {
        rfi_load(base + t * ld + cl, nv, vec_in, v);
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = pv[j];
      }
      const bool live = t < tend;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if (sizeof(T) == 1) {
          const uint32_t u = live ? (uint32_t)v[j] : 0u;
          s1[j] += u;
          s2[j] += u * u;
        } else {
          const double d = live ? (double)v[j] - (double)pv[j] : 0.0;
          s1[j] += d;
          s2[j] += d * d;
        }
        tile[(l * V + j) * kRfiTT + ((rr + 4 * l) & (kRfiTT - 1))] = v[j] - pv[j];
      }
    }
    __syncthreads();
    for (int ch = chr; ch < TC; ch += kRfiThreads / 16) {
      const int64_t c = c0 + ch;
      const int64_t t = tb + t4;
      if (c < clast && t < tend) {
        const float* src = tile + ch * kRfiTT + ((t4 + 4 * (ch / V)) & (kRfiTT - 1));
        const f32x4 q = *reinterpret_cast<const f32x4*>(src);
        float* dst = rows + ((c - cfirst) * nint + i) * P + t;
        if (vec_out) {
          *reinterpret_cast<f32x4*>(dst) = q;  // (P, span % 4 == 0: t + 3 < tend)
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (t + j < tend) dst[j] = q[j];
        }
      }
    }
    __syncthreads();
  }
  // sums over the 8 rows of a wave (lane bits 3..5), then over the waves
#pragma unroll
  for (int j = 0; j < V; ++j) {
#pragma unroll
    for (int m = kRfiLanes; m < 64; m <<= 1) {
      s1[j] += rfi_shfl(s1[j], m);
      s2[j] += rfi_shfl(s2[j], m);
    }
  }
  if ((tid & 63) < kRfiLanes) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      w1[tid / 64][l * V + j] = s1[j];
      w2[tid / 64][l * V + j] = s2[j];
    }
  }
  __syncthreads();
  if (tid < TC) {
    Sum1 a = w1[0][tid];
    Sum2 b = w2[0][tid];
#pragma unroll
    for (int w = 1; w < kRfiThreads / 64; ++w) {
      a += w1[w][tid];
      b += w2[w][tid];
    }
    part[((int64_t)blockIdx.x * 2 + 0) * TC + tid] = (Sum2)a;
    part[((int64_t)blockIdx.x * 2 + 1) * TC + tid] = b;
  }
}

// One thread per (cell = i ntile + tile, channel of the tile): the spans'
// sums added in span order, then avg, std and P var.
template <typename T>
__global__ __launch_bounds__(kRfiThreads) void k_rfi_finish(
    const typename RfiTraits<T>::Sum2* __restrict__ part, const float* __restrict__ pivots,
    int64_t nint, int64_t C, int64_t P, int64_t cfirst, int64_t clast, int64_t ntile, int64_t S,
    double* __restrict__ avg, double* __restrict__ sd, double* __restrict__ nvar) {
  constexpr int TC = kRfiLanes * RfiTraits<T>::V;
  typedef typename RfiTraits<T>::Sum1 Sum1;
  typedef typename RfiTraits<T>::Sum2 Sum2;
  const int64_t g = (int64_t)blockIdx.x * kRfiThreads + threadIdx.x;
  const int64_t cell = g / TC, ch = g % TC;
  if (cell >= nint * ntile) return;
  const int64_t i = cell / ntile, c = cfirst + (cell % ntile) * TC + ch;
  if (c >= clast) return;
  Sum2 a = 0, b = 0;
  for (int64_t sp = 0; sp < S; ++sp) {
    a += part[((cell * S + sp) * 2 + 0) * TC + ch];
    b += part[((cell * S + sp) * 2 + 1) * TC + ch];
  }
  double m, var;
  rfi_finish((Sum1)a, b, pivots[cell * TC + ch], P, &m, &var);
  avg[i * C + c] = m;
  sd[i * C + c] = sqrt(var);
  nvar[(c - cfirst) * nint + i] = (double)P * var;
}

// spec: [nrows][L] complex float32, L = P / 2 + 1; row = cl nint + i.
__global__ __launch_bounds__(kRfiThreads) void k_rfi_power(
    const float* __restrict__ spec, int64_t nrows, int64_t L, const double* __restrict__ nvar,
    int64_t nint, int64_t C, int64_t cfirst, double* __restrict__ pw) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (kRfiThreads / 64) + (threadIdx.x >> 6);
  if (row >= nrows) return;  // (whole waves: no barrier below)
  // bins 1 .. L-1 of the row are the complex elements [s, e) of the array;
  // pairs (2 q, 2 q + 1) are 16-byte aligned
  const int64_t s = row * L + 1, e = row * L + L;
  float best = 0.f;
  for (int64_t q = s / 2 + lane; 2 * q < e; q += 64) {
    const int64_t k = 2 * q;
    if (k >= s && k + 1 < e) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(spec + 2 * k);
      best = fmaxf(best, fmaxf(v.x * v.x + v.y * v.y, v.z * v.z + v.w * v.w));
    } else {
      if (k >= s) best = fmaxf(best, spec[2 * k] * spec[2 * k] + spec[2 * k + 1] * spec[2 * k + 1]);
      if (k + 1 >= s && k + 1 < e)
        best = fmaxf(best, spec[2 * k + 2] * spec[2 * k + 2] + spec[2 * k + 3] * spec[2 * k + 3]);
    }
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) best = fmaxf(best, __shfl_xor(best, m));
  if (lane == 0) {
    const double nv = nvar[row];
    const int64_t cl = row / nint, i = row % nint;
    pw[i * C + cfirst + cl] = nv > 0.0 ? (double)best / nv : 0.0;
  }
}

template <typename T>
__global__ __launch_bounds__(kRfiThreads) void k_rfi_apply(
    T* __restrict__ data, int64_t n, int64_t C, int64_t ld, int64_t t0, int64_t P,
    const uint32_t* __restrict__ bitmap, int64_t nint, int64_t W, const T* __restrict__ fill,
    bool vec) {
  constexpr int V = 16 / (int)sizeof(T);  // elements of a 16-byte piece
  const int64_t g = (int64_t)blockIdx.x * kRfiThreads + threadIdx.x;
  const int64_t w = g % W, tb = (g / W) * kRfiApplyRows;
  if (tb >= n) return;
  int64_t iv = (t0 + tb) / P, rem = (t0 + tb) % P;
  const int64_t c0 = w * 32;
  for (int k = 0; k < kRfiApplyRows && tb + k < n; ++k) {
    if (iv >= nint) return;  // past the bitmap: left alone
    const uint32_t bits = bitmap[iv * W + w];
    if (bits) {
      T* row = data + (tb + k) * ld + c0;
#pragma unroll
      for (int p = 0; p < 32 / V; ++p) {
        const uint32_t b = (bits >> (p * V)) & (uint32_t)((1ull << V) - 1);
        if (!b) continue;
        const int64_t c = c0 + p * V;
        if (vec && c + V <= C) {
          if (sizeof(T) == 1) {
            u32x4 x = *reinterpret_cast<const u32x4*>(row + p * V);
            const u32x4 f = *reinterpret_cast<const u32x4*>(fill + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const uint32_t nib = (b >> (4 * j)) & 0xfu;
              // byte mask of the 4 channels of word j
              const uint32_t m = ((nib & 1u) * 0xffu) | ((nib & 2u) * (0xff00u >> 1)) |
                                 ((nib & 4u) * (0xff0000u >> 2)) | ((nib & 8u) * (0xff000000u >> 3));
              x[j] = (x[j] & ~m) | (f[j] & m);
            }
            *reinterpret_cast<u32x4*>(row + p * V) = x;
          } else {
            f32x4 x = *reinterpret_cast<const f32x4*>(row + p * V);
            const f32x4 f = *reinterpret_cast<const f32x4*>(fill + c);
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if ((b >> j) & 1u) x[j] = f[j];
            *reinterpret_cast<f32x4*>(row + p * V) = x;
          }
        } else {
          for (int j = 0; j < V; ++j)
            if (((b >> j) & 1u) && c + j < C) row[p * V + j] = fill[c + j];
        }
      }
    }
    if (++rem == P) {
      rem = 0;
      ++iv;
    }
  }
}

template <typename T>
int rfi_prep(const T* raw, int64_t nint, int64_t C, int64_t ld, int64_t P, int64_t c0, int64_t nc,
             float* rows, double* avg, double* sd, double* nvar, hipStream_t st) {
  constexpr int TC = kRfiLanes * RfiTraits<T>::V;
  typedef typename RfiTraits<T>::Sum2 Sum2;
  const int64_t ntile = cdiv(nc, TC), ncell = nint * ntile;
  // spans of whole 64-sample tiles: about kRfiTargetBlocks workgroups in all
  const int64_t tiles = cdiv(P, kRfiTT);
  int64_t S = cdiv(kRfiTargetBlocks, ncell);
  S = S < 1 ? 1 : (S > tiles ? tiles : S);
  const int64_t span = cdiv(tiles, S) * kRfiTT;
  S = cdiv(P, span);
  PDD_REQUIRE(ncell * S < (1ll << 31), "pdd_rfi_stats_prep: too large");
  Sum2* part = static_cast<Sum2*>(scratch(st, kScratchPartial, (size_t)(ncell * S) * 2 * TC * sizeof(Sum2)));
  float* pivots = static_cast<float*>(scratch(st, kScratchSmall, (size_t)ncell * TC * sizeof(float)));
  if (!part || !pivots) return -2;
  const bool vec_in = ((uintptr_t)raw & 15) == 0 && (ld * sizeof(T)) % 16 == 0 &&
                      (c0 * sizeof(T)) % 16 == 0;
  const bool vec_out = ((uintptr_t)rows & 15) == 0 && P % 4 == 0;
  k_rfi_prep<T><<<(unsigned)(ncell * S), kRfiThreads, 0, st>>>(
      raw, nint, ld, P, c0, c0 + nc, ntile, S, span, vec_in, vec_out, rows, part, pivots);
  PDD_LAUNCHED();
  k_rfi_finish<T><<<(unsigned)cdiv(ncell * TC, kRfiThreads), kRfiThreads, 0, st>>>(
      part, pivots, nint, C, P, c0, c0 + nc, ntile, S, avg, sd, nvar);
  PDD_LAUNCHED();
  return 0;
}

template <typename T>
int rfi_apply(T* data, int64_t n, int64_t C, int64_t ld, int64_t t0, int64_t P,
              const uint32_t* bitmap, int64_t nint, const T* fill, hipStream_t st) {
  const int64_t W = cdiv(C, 32);
  const int64_t threads = cdiv(n, kRfiApplyRows) * W;
  PDD_REQUIRE(cdiv(threads, kRfiThreads) < (1ll << 31), "pdd_rfi_apply: too large");
  const bool vec = ((uintptr_t)data & 15) == 0 && (ld * sizeof(T)) % 16 == 0 &&
                   ((uintptr_t)fill & 15) == 0;
  k_rfi_apply<T><<<(unsigned)cdiv(threads, kRfiThreads), kRfiThreads, 0, st>>>(
      data, n, C, ld, t0, P, bitmap, nint, W, fill, vec);
  PDD_LAUNCHED();
  return 0;
}

}  // namespace

}  // namespace pdd

using namespace pdd;

extern "C" {

int pdd_rfi_stats_prep(const void* raw, int dtype, int64_t nint, int64_t C, int64_t ld,
                       int64_t ptsperint, int64_t c0, int64_t nc, float* rows, double* avg,
                       double* std, double* nvar, void* stream) {
  PDD_REQUIRE(raw && rows && avg && std && nvar, "pdd_rfi_stats_prep: null pointer");
  PDD_REQUIRE(dtype == PDD_U8 || dtype == PDD_F32, "pdd_rfi_stats_prep: dtype must be u8 or f32");
  PDD_REQUIRE(nint >= 0 && C > 0 && ld >= C && c0 >= 0 && nc >= 0 && c0 + nc <= C,
              "pdd_rfi_stats_prep: bad shape");
  // (8 bits: N^2 65025 and the per-thread 32-bit sums stay in range)
  PDD_REQUIRE(ptsperint >= 16 && ptsperint <= (1ll << 23),
              "pdd_rfi_stats_prep: ptsperint out of range 16..2^23");
  if (nint == 0 || nc == 0) return 0;
  hipStream_t st = as_stream(stream);
  if (dtype == PDD_U8)
    return rfi_prep(static_cast<const uint8_t*>(raw), nint, C, ld, ptsperint, c0, nc, rows, avg,
                    std, nvar, st);
  return rfi_prep(static_cast<const float*>(raw), nint, C, ld, ptsperint, c0, nc, rows, avg, std,
                  nvar, st);
}

int pdd_rfi_stats_power(const float* spec, int64_t nrows, int64_t ptsperint, const double* nvar,
                        int64_t nint, int64_t C, int64_t c0, double* pow, void* stream) {
  PDD_REQUIRE(spec && nvar && pow, "pdd_rfi_stats_power: null pointer");
  PDD_REQUIRE(nrows >= 0 && nint > 0 && nrows % nint == 0 && C > 0 && c0 >= 0 &&
                  c0 + nrows / nint <= C && ptsperint >= 16,
              "pdd_rfi_stats_power: bad shape");
  PDD_REQUIRE(((uintptr_t)spec & 15) == 0, "pdd_rfi_stats_power: spec must be 16-byte aligned");
  if (nrows == 0) return 0;
  const int64_t nblk = cdiv(nrows, kRfiThreads / 64);
  PDD_REQUIRE(nblk < (1ll << 31), "pdd_rfi_stats_power: too large");
  k_rfi_power<<<(unsigned)nblk, kRfiThreads, 0, as_stream(stream)>>>(
      spec, nrows, ptsperint / 2 + 1, nvar, nint, C, c0, pow);
  PDD_LAUNCHED();
  return 0;
}

int pdd_rfi_apply(void* data, int dtype, int64_t n, int64_t C, int64_t ld, int64_t t0,
                  int64_t ptsperint, const uint32_t* bitmap, int64_t nint, const void* fill,
                  void* stream) {
  PDD_REQUIRE(data && bitmap && fill, "pdd_rfi_apply: null pointer");
  PDD_REQUIRE(dtype == PDD_U8 || dtype == PDD_F32, "pdd_rfi_apply: dtype must be u8 or f32");
  PDD_REQUIRE(n >= 0 && C > 0 && ld >= C && t0 >= 0 && ptsperint >= 1 && nint >= 0,
              "pdd_rfi_apply: bad shape");
  if (n == 0 || nint == 0) return 0;
  hipStream_t st = as_stream(stream);
  if (dtype == PDD_U8)
    return rfi_apply(static_cast<uint8_t*>(data), n, C, ld, t0, ptsperint, bitmap, nint,
                     static_cast<const uint8_t*>(fill), st);
  return rfi_apply(static_cast<float*>(data), n, C, ld, t0, ptsperint, bitmap, nint,
                   static_cast<const float*>(fill), st);
}

}  // extern "C"
