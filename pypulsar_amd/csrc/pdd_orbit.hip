// libpdd: coherent orbit demodulation -- one time series resampled into the
// pulsar's frame by a bank of Keplerian templates (the operation of the
// reference's bin/demodulate.py, for many trial orbits at once).  The [T, n]
// result is searched and folded like a DM-time plane.  gfx950, wave64.
//
// Definition (include/pdd.h, DESIGN.md §6r, restated in tests/orbit_oracle.py).
// Template (pb, x, e, omega, t0) has the Roemer delay
//   D(t) = x [(cos E - e) sin omega + sin E sqrt(1 - e^2) cos omega],
//   E - e sin E = 2 pi (t - t0) / pb,
// and output sample j is taken at input position p_j (in samples) with
//   p_j - (D(p_j dt) - D(0)) / dt = j.
// p is solved in float64 at the knots j = k K only; between two knots it is
// p_k + (p_{k+1} - p_k) (i / K), one IEEE operation each, in this order.
//
// k_orbit_resample<VEC, MODE>: workgroup b serves output tile b / T of template
// b % T, so the workgroups in flight share one input window of about 1.1 tile +
// 2 samples through L2.  A tile spans nkn - 1 knot intervals, nkn = min(2045,
// 16384 / K): 16384 - K samples for K >= 16, 2044 K below (a multiple of 4
// either way), so that the position solves, which idle most lanes when there
// are few of them, are paid once per 16 Ki outputs where K allows it, and so
// that nkn knots fill whole rounds of the 256 lanes but for 3 lanes of the last.
//   * The tile's nkn knots (those at or below knot nk - 1) are solved a round
//     of 256 at a time -- Newton on Kepler's equation inside Newton on the
//     position, both with fixed starting values and exit rules, so the bits do
//     not depend on the launch -- kept in LDS and, when asked for, written to
//     the dump.  The tile's last knot belongs to the next tile's dump except
//     at the end of the row.
//   * Every lane then interpolates VEC consecutive positions a pass (one knot
//     interval for all of them when K >= VEC) and gathers them; a position
//     outside [0, n - 1] (or a NaN) gives `fill`, so no element outside the
//     row is read.
//   * VEC = 4, 2 or 1 floats a store: the widest that the alignment of `out`
//     and ld_out allows.
#include <cmath>

#include "pdd_internal.h"

namespace pdd {

namespace {

constexpr int kOrbBlock = 256;      // threads a workgroup
constexpr int kOrbMaxK = 256;
constexpr int kOrbMaxKnots = 2045;  // knots a tile at most: 8 rounds of the lanes less 3
constexpr int kOrbSpan = 16384;     // samples a tile may span
constexpr double kOrbPi = 3.14159265358979323846;
constexpr double kOrbTwoPi = 6.28318530717958647692;
constexpr double kOrbInvTwoPi = 0.15915494309189533577;

// knots of a tile, both ends included
__host__ __device__ constexpr int orb_tile_knots(int K) {
  return kOrbSpan / K < kOrbMaxKnots ? kOrbSpan / K : kOrbMaxKnots;
}

struct OrbTemplate {
  double n;      // 2 pi / pb
  double x, e, t0;
  double so, co;  // sin omega, sqrt(1 - e^2) cos omega
};

// sin E and cos E of the eccentric anomaly at mean anomaly M
__device__ __forceinline__ void orb_anomaly(double M, double e, double& sE, double& cE) {
  M = M - kOrbTwoPi * rint(M * kOrbInvTwoPi);
  const double a = fabs(M);
  double s, c;
  if (e == 0.0) {  // (uniform in a workgroup) circular: E = M
    sincos(a, &s, &c);
  } else {
    // from pi Newton descends monotonically (E - e sin E is convex on [0, pi])
    double E = e < 0.8 ? a + e * sin(a) : kOrbPi;
    for (int it = 0; it < 40; ++it) {
      sincos(E, &s, &c);
      const double d = (E - e * s - a) / (1.0 - e * c);
      E = E - d;
      if (!(fabs(d) > 1e-8)) {
        // the last step to first order: what is left is d^2 / 2 <= 5e-17
        const double s1 = s - c * d;
        c = c + s * d;
        s = s1;
        break;
      }
    }
  }
  sE = M < 0.0 ? -s : s;
  cE = c;
}

// D(t) and dD/dt
__device__ __forceinline__ void orb_delay(const OrbTemplate& o, double t, double& D, double& dD) {
  double s, c;
  orb_anomaly(o.n * (t - o.t0), o.e, s, c);
  D = o.x * ((c - o.e) * o.so + s * o.co);
  dD = o.x * (c * o.co - s * o.so) * (o.n / (1.0 - o.e * c));
}

// the position, in samples, of output sample j
__device__ __forceinline__ double orb_position(const OrbTemplate& o, double dt, double D0, double j) {
  double p = j;
  for (int it = 0; it < 16; ++it) {
    double D, dD;
    orb_delay(o, p * dt, D, dD);
    const double d = ((p - j) - (D - D0) / dt) / (1.0 - dD);
    p = p - d;
    // quadratic: what is left is (A / 2) d^2, A = |d2p/dj2| (far below 1 for beta <= 0.1):
    // under 5e-10 A samples
    if (!(fabs(d) > 3e-5)) break;
  }
  return p;
}

template <int VEC>
struct OrbVec;
template <>
struct OrbVec<4> {
  typedef float type __attribute__((ext_vector_type(4)));
};
template <>
struct OrbVec<2> {
  typedef float type __attribute__((ext_vector_type(2)));
};
template <>
struct OrbVec<1> {
  typedef float type;
};

template <int VEC, int MODE>
__global__ __launch_bounds__(kOrbBlock) void k_orbit_resample(
    const float* __restrict__ row, int64_t n, double dt, const double* __restrict__ orbits,
    int64_t T, int log2K, float fill, float* __restrict__ out, int64_t ld_out,
    double* __restrict__ knots, int64_t nk) {
  __shared__ double P[kOrbMaxKnots];
  const int K = 1 << log2K;
  const int nknot = orb_tile_knots(K);
  const int tile_len = (nknot - 1) << log2K;
  const int64_t tile = blockIdx.x / T;
  const int64_t tmpl = blockIdx.x - tile * T;
  const int64_t j0 = tile * tile_len;
  const int64_t k0 = tile * (nknot - 1);

  if ((int)threadIdx.x < nknot) {
    const double* __restrict__ ob = orbits + tmpl * 5;
    OrbTemplate o;
    o.n = kOrbTwoPi / ob[0];
    o.x = ob[1];
    o.e = ob[2];
    o.t0 = ob[4];
    {
      double s, c;
      sincos(ob[3], &s, &c);
      o.so = s;
      o.co = sqrt(1.0 - o.e * o.e) * c;
    }
    double D0, dD0;
    orb_delay(o, 0.0, D0, dD0);
    for (int q = threadIdx.x; q < nknot; q += kOrbBlock) {
      const int64_t k = k0 + q;
      if (k >= nk) break;
      const double p = orb_position(o, dt, D0, (double)(k << log2K));
      P[q] = p;
      if (knots && (q < nknot - 1 || k == nk - 1)) knots[tmpl * nk + k] = p;
    }
  }
  __syncthreads();

  float* __restrict__ orow = out + tmpl * ld_out;
  const double last = (double)(n - 1);
  const int ilast = (int)(n - 1);
  const double invK = 1.0 / (double)K;  // a power of two: i * invK == i / K exactly
  const bool shared = K >= VEC;         // the VEC samples of a lane lie in one knot interval
  for (int base = threadIdx.x * VEC; base < tile_len; base += kOrbBlock * VEC) {
    const int64_t j = j0 + base;
    if (j >= n) break;
    int q = base >> log2K;
    double pk = P[q];
    double dk = P[q + 1] - pk;
    float v[VEC];
#pragma unroll
    for (int u = 0; u < VEC; ++u) {
      const int i = base + u;
      v[u] = fill;
      if (j + u < n) {
        if (!shared && u > 0) {
          q = i >> log2K;
          pk = P[q];
          dk = P[q + 1] - pk;
        }
        const double w = (double)(i & (K - 1)) * invK;
        const double p = pk + dk * w;
        if (p >= 0.0 && p <= last) {
          if (MODE == PDD_ORBIT_NEAREST) {
            v[u] = row[(int)floor(p + 0.5)];
          } else {
            const double fl = floor(p);
            const int i0 = (int)fl;
            const float a = row[i0];
            if (i0 < ilast) {
              const float f = (float)(p - fl);
              v[u] = a + (row[i0 + 1] - a) * f;
            } else {
              v[u] = a;
            }
          }
        }
      }
    }
    if (VEC > 1 && j + VEC <= n) {
      typename OrbVec<VEC>::type pack;
#pragma unroll
      for (int u = 0; u < VEC; ++u) reinterpret_cast<float*>(&pack)[u] = v[u];
      *reinterpret_cast<typename OrbVec<VEC>::type*>(orow + j) = pack;
    } else {
#pragma unroll
      for (int u = 0; u < VEC; ++u)
        if (j + u < n) orow[j + u] = v[u];
    }
  }
}

template <int VEC>
int orbit_launch(const float* row, int64_t n, double dt, const double* orbits, int64_t T, int log2K,
                 int mode, float fill, float* out, int64_t ld_out, double* knots, int64_t nk,
                 int64_t ntile, hipStream_t st) {
  const unsigned grid = (unsigned)(ntile * T);
  if (mode == PDD_ORBIT_NEAREST)
    k_orbit_resample<VEC, PDD_ORBIT_NEAREST><<<grid, kOrbBlock, 0, st>>>(
        row, n, dt, orbits, T, log2K, fill, out, ld_out, knots, nk);
  else
    k_orbit_resample<VEC, PDD_ORBIT_LINEAR><<<grid, kOrbBlock, 0, st>>>(
        row, n, dt, orbits, T, log2K, fill, out, ld_out, knots, nk);
  PDD_LAUNCHED();
  return 0;
}

}  // namespace

}  // namespace pdd

using namespace pdd;

extern "C" {

int pdd_orbit_resample(const float* row, int64_t n, double dt, const double* orbits, int64_t T,
                       int K, int mode, float fill, float* out, int64_t ld_out, double* knots,
                       void* stream) {
  PDD_REQUIRE(row && orbits && out, "pdd_orbit_resample: null pointer");
  PDD_REQUIRE(n >= 2 && n < (1ll << 31), "pdd_orbit_resample: n must be in 2..2^31 - 1");
  PDD_REQUIRE(T >= 0, "pdd_orbit_resample: bad shape");
  PDD_REQUIRE(ld_out >= n, "pdd_orbit_resample: ld_out must be >= n");
  PDD_REQUIRE(dt > 0.0, "pdd_orbit_resample: dt must be > 0");
  PDD_REQUIRE(K >= 1 && K <= kOrbMaxK && (K & (K - 1)) == 0,
              "pdd_orbit_resample: K must be a power of two in 1..%d", kOrbMaxK);
  PDD_REQUIRE(mode == PDD_ORBIT_NEAREST || mode == PDD_ORBIT_LINEAR,
              "pdd_orbit_resample: unknown mode %d", mode);
  if (T == 0) return 0;
  const int64_t ntile = cdiv(n, (int64_t)(orb_tile_knots(K) - 1) * K);
  PDD_REQUIRE(T <= ((1ll << 31) - 1) / ntile,
              "pdd_orbit_resample: too many templates for one launch (at most %lld at this n)",
              (long long)(((1ll << 31) - 1) / ntile));
  int log2K = 0;
  while ((1 << log2K) < K) ++log2K;
  const int64_t nk = (n - 1) / K + 2;
  hipStream_t st = as_stream(stream);
  const uintptr_t a = reinterpret_cast<uintptr_t>(out);
  if ((a & 15) == 0 && (ld_out & 3) == 0)
    return orbit_launch<4>(row, n, dt, orbits, T, log2K, mode, fill, out, ld_out, knots, nk, ntile,
                           st);
  if ((a & 7) == 0 && (ld_out & 1) == 0)
    return orbit_launch<2>(row, n, dt, orbits, T, log2K, mode, fill, out, ld_out, knots, nk, ntile,
                           st);
  return orbit_launch<1>(row, n, dt, orbits, T, log2K, mode, fill, out, ld_out, knots, nk, ntile,
                         st);
}

}  // extern "C"
