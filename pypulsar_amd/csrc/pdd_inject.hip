// Injection of synthetic pulsars and bursts into a raw time-major block
// (pdd_inject; definition in include/pdd.h and pypulsar_amd/inject.py,
// DESIGN.md §6p; restated in tests/inject_oracle.py).
//
//   k_inject<T, V>  one workgroup per (group of 256 channels, 64 rows).  A
//                   thread keeps V adjacent channels (V = 4: a dword of 8-bit
//                   or 16 bytes of float32 data; a wave takes 64 channels as
//                   16 quads x 4 adjacent rows, a thread rows r, r + 4, ...;
//                   V = 1: one channel per thread, every row of the tile) and
//                   walks its
//                   rows job by job: the per-channel job constants are loaded
//                   once per job, the sums of its 64 cells stay in registers,
//                   and the block is read and written once at the end, only
//                   where a job covered a cell.  A job whose envelope over
//                   the group's channels misses the tile's rows costs two
//                   scalar loads.
//   k_inject<T, V, true>  the same with Keplerian orbits (pdd_inject_orbit):
//                   a job with an orbit carries its orbital phase psi per
//                   channel as a second wrapping 64-bit integer (ophase +
//                   i ostep), looks the orbital term q up in its float64
//                   table (two adjacent knots, plain vector loads) and takes
//                   U(q) off the phase.  The job's m, ostep and table offset
//                   are kernel arguments (scalar, uniform over the
//                   workgroup); a job with m = -1 runs the plain path.  The
//                   tile has kInjOrbRows rows, so the sums of a thread take
//                   half the registers and nothing spills.  Launched only
//                   when some job has an orbit.
//
// The value of a cell depends on (absolute sample, channel) alone: the linear
// part of the phase is advanced by exact wrapping adds from P0 + i step, the
// float64 drift is evaluated directly per cell, the dither is a hash of the
// cell.  Built with -ffp-contract=off: every float operation below is one
// IEEE operation.
#include "pdd_internal.h"

namespace pdd {

namespace {

constexpr int kInjThreads = 256;
constexpr int kInjGroup = 256;  // channels per workgroup = PDD_INJECT_GROUP
constexpr int kInjRows = 64;    // rows per workgroup
constexpr int kInjCells = 64;   // cells per thread (kInjGroup kInjRows / kInjThreads)
constexpr int kInjOrbRows = 32; // rows per workgroup of the orbit instantiations
static_assert(kInjGroup == PDD_INJECT_GROUP, "the envelope entries of `range` follow the tile");

typedef float f32x4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) TabPair {
  float a, b;
};

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// U(d) = (uint64)((d - floor(d)) 2^64); a difference that rounds to 1 is 0.
__device__ __forceinline__ uint64_t frac_to_u64(double d) {
  double fr = d - floor(d);
  if (fr >= 1.0) fr = 0.0;
  return (uint64_t)(fr * 18446744073709551616.0);
}

__device__ __forceinline__ float quantise(float x, float acc, uint32_t hrow, int64_t c, float vmax) {
  const uint32_t h = fmix32(hrow ^ ((uint32_t)c * 0x27d4eb2fu));
  const float u = (float)(h >> 8) * 5.9604644775390625e-8f;
  float y = x + acc;
  y = y + u;
  y = floorf(y);
  return fminf(vmax, fmaxf(0.0f, y));
}

// The orbits of a launch: per job m (-1: none; else the table has 2^m + 1
// knots), the orbital phase step per sample and the table's first element in
// qtab, all checked by the entry point.  Empty for the plain instantiations.
template <bool ORB>
struct OrbArgs {};
template <>
struct OrbArgs<true> {
  const uint64_t* ophase;  // [J][C]
  const double* qtab;
  uint64_t ostep[PDD_INJECT_MAX_JOBS];
  int64_t off[PDD_INJECT_MAX_JOBS];
  int8_t m[PDD_INJECT_MAX_JOBS];
};

template <typename T, int V, bool ORB = false>
__global__ __launch_bounds__(kInjThreads) void k_inject(
    T* __restrict__ data, int64_t n, int64_t C, int64_t ld, int64_t t0, int64_t G,
    const uint64_t* __restrict__ phase, const double* __restrict__ drift,
    const int64_t* __restrict__ range, const float* __restrict__ tables, int J, int lb,
    uint32_t seed, float vmax, const OrbArgs<ORB> oa) {
  constexpr int ROWS = ORB ? kInjOrbRows : kInjRows;  // rows of this tile
  constexpr int R = kInjGroup * ROWS / kInjThreads / V;  // rows per thread (kInjCells / V)
  constexpr int RS = V == 4 ? 4 : 1;           // row stride of a thread
  const int64_t g = (int64_t)blockIdx.x % G, rt = (int64_t)blockIdx.x / G;
  const int t = threadIdx.x;
  // V = 4: a wave takes 64 channels; its lanes are 16 channel quads x 4
  // adjacent rows, so the 4 rows of a channel read neighbouring table entries
  // (a load instruction touches about 16 table lines, not 64)
  const int64_t c0 = g * kInjGroup + (V == 4 ? (t >> 6) * 64 + (t & 15) * 4 : t);
  const int64_t r0 = rt * ROWS + (V == 4 ? ((t >> 4) & 3) : 0);  // this thread's first row
  const int64_t a0 = t0 + rt * ROWS;                       // the tile's absolute rows
  const int64_t a1 = a0 + (n - rt * ROWS < ROWS ? n - rt * ROWS : ROWS);
  const int64_t B1 = ((int64_t)1 << lb) + 1;                   // table row length

  float acc[R][V];
  uint64_t cov = 0;  // bit k V + v: cell (row k, channel v) is covered
#pragma unroll
  for (int k = 0; k < R; ++k)
#pragma unroll
    for (int v = 0; v < V; ++v) acc[k][v] = 0.0f;

  for (int j = 0; j < J; ++j) {
    const int64_t* rj = range + (int64_t)j * (C + G) * 2;
    const int64_t elo = rj[(C + g) * 2], ehi = rj[(C + g) * 2 + 1];
    if (ehi <= a0 || elo >= a1) continue;  // (uniform over the workgroup)
    uint64_t ph[V], inc[V];
    double k2[V], k3 = 0.0;
    int64_t lo[V], hi[V];
    const float* tab[V];
    bool curved = false;
    // the job's orbit (uniform over the workgroup)
    int om = -1;
    uint64_t ostep = 0;
    const double* qt = nullptr;
    uint64_t op[ORB ? V : 1];
    if constexpr (ORB) {
      om = oa.m[j];
      ostep = oa.ostep[j];
      qt = oa.qtab + oa.off[j];
#pragma unroll
      for (int v = 0; v < V; ++v) op[v] = 0;
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int64_t c = c0 + v;
      lo[v] = hi[v] = 0;
      ph[v] = inc[v] = 0;
      k2[v] = 0.0;
      tab[v] = tables;
      if (c < C) {
        const int64_t jc = (int64_t)j * C + c;
        lo[v] = rj[c * 2];
        hi[v] = rj[c * 2 + 1];
        const uint64_t step = phase[jc * 2 + 1];
        ph[v] = phase[jc * 2] + (uint64_t)(t0 + r0) * step;
        inc[v] = step * (uint64_t)RS;
        k2[v] = drift[jc * 2];
        k3 = drift[jc * 2 + 1];
        tab[v] = tables + jc * B1;
        curved = curved || k2[v] != 0.0;
        if constexpr (ORB)
          if (om >= 0) op[v] = oa.ophase[jc] + (uint64_t)(t0 + r0) * ostep;
      }
    }
    curved = curved || k3 != 0.0;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const int64_t i = t0 + r0 + (int64_t)k * RS;
      const bool live = i < a1;
      const double x = (double)i;
      const double xx = x * x;
      const double xk3 = x * k3;
#pragma unroll
      for (int v = 0; v < V; ++v) {
        if (live && i >= lo[v] && i < hi[v]) {
          uint64_t p = ph[v];
          if (curved) {
            const double s = k2[v] + xk3;
            p += frac_to_u64(xx * s);
          }
          if constexpr (ORB) {
            if (om >= 0) {
              // k + 1 <= 2^m: k is the top m bits of psi
              const uint64_t psi = op[v];
              const double* kn = qt + (psi >> (64 - om));
              const double w = (double)((uint32_t)(psi >> (32 - om))) * 2.3283064365386963e-10;
              const double qa = kn[0], qb = kn[1];
              const double dq = qb - qa;
              const double mq = dq * w;
              p -= frac_to_u64(qa + mq);
            }
          }
          const uint32_t b = (uint32_t)(p >> (64 - lb));
          const float wgt = (float)((uint32_t)(p >> (40 - lb)) & 0xffffffu) * 5.9604644775390625e-8f;
          // (the pair as one 8-byte load; entries are 4-byte aligned)
          const TabPair tp = *reinterpret_cast<const TabPair*>(tab[v] + b);
          const float ta = tp.a, tb = tp.b;
          const float d = tb - ta;
          const float m = d * wgt;
          acc[k][v] = acc[k][v] + (ta + m);
          cov |= 1ull << (k * V + v);
        }
        ph[v] += inc[v];
        if constexpr (ORB) op[v] += ostep * (uint64_t)RS;
      }
    }
  }
  if (!cov) return;

#pragma unroll
  for (int k = 0; k < R; ++k) {
    const uint32_t bits = (uint32_t)(cov >> (k * V)) & ((1u << V) - 1u);
    if (!bits) continue;
    const int64_t r = r0 + (int64_t)k * RS;
    const uint64_t i = (uint64_t)(t0 + r);
    T* row = data + r * ld + c0;
    uint32_t hrow = 0;
    if (sizeof(T) == 1)
      hrow = fmix32(fmix32((uint32_t)i ^ seed) ^ (uint32_t)(i >> 32) ^ 0x9e3779b9u);
    if (V == 4) {
      if (sizeof(T) == 1) {
        uint32_t w = *reinterpret_cast<const uint32_t*>(row);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          if (!((bits >> v) & 1u)) continue;
          const float x = (float)((w >> (8 * v)) & 0xffu);
          const uint32_t q = (uint32_t)quantise(x, acc[k][v], hrow, c0 + v, vmax);
          w = (w & ~(0xffu << (8 * v))) | (q << (8 * v));
        }
        *reinterpret_cast<uint32_t*>(row) = w;
      } else {
        f32x4 w = *reinterpret_cast<const f32x4*>(row);
#pragma unroll
        for (int v = 0; v < 4; ++v)
          if ((bits >> v) & 1u) w[v] = w[v] + acc[k][v];
        *reinterpret_cast<f32x4*>(row) = w;
      }
    } else {
      if (sizeof(T) == 1)
        row[0] = (T)quantise((float)row[0], acc[k][0], hrow, c0, vmax);
      else
        row[0] = (T)((float)row[0] + acc[k][0]);
    }
  }
}

template <typename T>
int inject(T* data, int64_t n, int64_t C, int64_t ld, int64_t t0, const uint64_t* phase,
           const double* drift, const int64_t* range, const float* tables, int J, int lb,
           uint32_t seed, int vmax, const OrbArgs<true>* orb, hipStream_t st) {
  const int64_t G = cdiv(C, kInjGroup);
  const int64_t blocks = G * cdiv(n, orb ? kInjOrbRows : kInjRows);
  PDD_REQUIRE(blocks < (1ll << 31), "%s: too large", orb ? "pdd_inject_orbit" : "pdd_inject");
  // four adjacent channels as one aligned access where the shape allows
  const bool vec = C % 4 == 0 && ld % 4 == 0 && ((uintptr_t)data & (4 * sizeof(T) - 1)) == 0;
  if (orb) {
    if (vec)
      k_inject<T, 4, true><<<(unsigned)blocks, kInjThreads, 0, st>>>(
          data, n, C, ld, t0, G, phase, drift, range, tables, J, lb, seed, (float)vmax, *orb);
    else
      k_inject<T, 1, true><<<(unsigned)blocks, kInjThreads, 0, st>>>(
          data, n, C, ld, t0, G, phase, drift, range, tables, J, lb, seed, (float)vmax, *orb);
  } else if (vec) {
    k_inject<T, 4><<<(unsigned)blocks, kInjThreads, 0, st>>>(
        data, n, C, ld, t0, G, phase, drift, range, tables, J, lb, seed, (float)vmax,
        OrbArgs<false>());
  } else {
    k_inject<T, 1><<<(unsigned)blocks, kInjThreads, 0, st>>>(
        data, n, C, ld, t0, G, phase, drift, range, tables, J, lb, seed, (float)vmax,
        OrbArgs<false>());
  }
  PDD_LAUNCHED();
  return 0;
}

// The checks and the launch of both entry points; `who` names the entry in
// the messages.  ometa == nullptr: no job has an orbit.
int inject_entry(const char* who, void* data, int dtype, int64_t n, int64_t C, int64_t ld,
                 int64_t t0, const uint64_t* phase, const double* drift, const int64_t* range,
                 const float* tables, int J, int B, int64_t seed, int vmax,
                 const uint64_t* ophase, const int64_t* ometa, const double* qtab, int64_t qlen,
                 void* stream) {
  PDD_REQUIRE(data, "%s: null pointer", who);
  PDD_REQUIRE(dtype == PDD_U8 || dtype == PDD_F32, "%s: dtype must be u8 or f32", who);
  PDD_REQUIRE(n >= 0 && C > 0 && ld >= C && t0 >= 0 && n <= (1ll << 52) && t0 <= (1ll << 52) - n,
              "%s: bad shape", who);
  PDD_REQUIRE(J >= 0 && J <= PDD_INJECT_MAX_JOBS, "%s: J out of range 0..64", who);
  PDD_REQUIRE(B >= 64 && B <= 4096 && (B & (B - 1)) == 0,
              "%s: B must be a power of two in 64..4096", who);
  PDD_REQUIRE(seed >= 0 && seed < (1ll << 32), "%s: seed must fit 32 bits", who);
  PDD_REQUIRE(vmax >= 1 && vmax <= 255, "%s: vmax out of range 1..255", who);
  PDD_REQUIRE(J == 0 || (phase && drift && range && tables), "%s: null job table", who);
  OrbArgs<true> orb;
  bool any = false;
  if (ometa) {
    orb.ophase = ophase;
    orb.qtab = qtab;
    for (int j = 0; j < PDD_INJECT_MAX_JOBS; ++j) {
      orb.m[j] = -1;
      orb.ostep[j] = 0;
      orb.off[j] = 0;
    }
    PDD_REQUIRE(qlen >= 0, "%s: qlen < 0", who);
    for (int j = 0; j < J; ++j) {
      const int64_t m = ometa[3 * j], off = ometa[3 * j + 2];
      if (m == -1) continue;
      PDD_REQUIRE(m >= PDD_INJECT_ORBIT_MIN_M && m <= PDD_INJECT_ORBIT_MAX_M,
                  "%s: job %d: m = %lld outside 6..22 (or -1: no orbit)", who, j, (long long)m);
      PDD_REQUIRE(ophase && qtab, "%s: null orbit table (job %d has an orbit)", who, j);
      PDD_REQUIRE(((uintptr_t)qtab & 7) == 0, "%s: qtab is not 8-byte aligned", who);
      PDD_REQUIRE(off >= 0 && off % 8 == 0,
                  "%s: job %d: table offset %lld is negative or no multiple of 8 bytes", who, j,
                  (long long)off);
      PDD_REQUIRE(off / 8 + ((int64_t)1 << m) + 1 <= qlen,
                  "%s: job %d: its table of 2^%lld + 1 knots at byte %lld runs past qlen = %lld",
                  who, j, (long long)m, (long long)off, (long long)qlen);
      orb.m[j] = (int8_t)m;
      orb.ostep[j] = (uint64_t)ometa[3 * j + 1];
      orb.off[j] = off / 8;
      any = true;
    }
  }
  if (n == 0 || J == 0) return 0;
  int lb = 0;
  while ((1 << lb) < B) ++lb;
  hipStream_t st = as_stream(stream);
  const OrbArgs<true>* po = any ? &orb : nullptr;
  if (dtype == PDD_U8)
    return inject(static_cast<uint8_t*>(data), n, C, ld, t0, phase, drift, range, tables, J, lb,
                  (uint32_t)seed, vmax, po, st);
  return inject(static_cast<float*>(data), n, C, ld, t0, phase, drift, range, tables, J, lb,
                (uint32_t)seed, vmax, po, st);
}

}  // namespace

}  // namespace pdd

using namespace pdd;

extern "C" {

int pdd_inject(void* data, int dtype, int64_t n, int64_t C, int64_t ld, int64_t t0,
               const uint64_t* phase, const double* drift, const int64_t* range,
               const float* tables, int J, int B, int64_t seed, int vmax, void* stream) {
  return inject_entry("pdd_inject", data, dtype, n, C, ld, t0, phase, drift, range, tables, J, B,
                      seed, vmax, nullptr, nullptr, nullptr, 0, stream);
}

int pdd_inject_orbit(void* data, int dtype, int64_t n, int64_t C, int64_t ld, int64_t t0,
                     const uint64_t* phase, const double* drift, const int64_t* range,
                     const float* tables, int J, int B, int64_t seed, int vmax,
                     const uint64_t* ophase, const int64_t* ometa, const double* qtab,
                     int64_t qlen, void* stream) {
  PDD_REQUIRE(J <= 0 || J > PDD_INJECT_MAX_JOBS || ometa, "pdd_inject_orbit: null ometa");
  return inject_entry("pdd_inject_orbit", data, dtype, n, C, ld, t0, phase, drift, range, tables,
                      J, B, seed, vmax, ophase, ometa, qtab, qlen, stream);
}

}  // extern "C"
