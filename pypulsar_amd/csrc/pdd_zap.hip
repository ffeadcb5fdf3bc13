// libpdd: Fourier-domain interference ("birdie") zapping -- an order-
// statistic spectrum across the rows of a plane of whitened power spectra,
// and the fill of listed bin intervals with the whitened mean level.  gfx950.
//
// A periodic terrestrial signal is in (nearly) every DM row of the plane, a
// celestial one in a few neighbouring rows: the median across rows keeps the
// first and discards the second (pypulsar_amd/zap.py, DESIGN.md §6i;
// restated in tests/zap_oracle.py).
//
// Kernels:
//   k_zap_percentile<RC>  one lane per bin, consecutive lanes consecutive
//                  bins: every row's load is one coalesced line per wave and
//                  the R loads of a lane are independent.  The R values of
//                  the bin's column live in RC registers (RC: R rounded up
//                  to a multiple of 8, the rest padded with the largest key)
//                  as order-preserving unsigned keys, and are sorted by
//                  Batcher's merge-exchange network, fully unrolled: every
//                  index is a compile-time constant (no private array in
//                  memory, no scratch).  The network only moves values, so
//                  the result is a value present in the column, whatever the
//                  ties; the rank-th is picked by a uniform select chain.
//   k_zap_apply    one wave per (interval, row): the wave walks the interval
//                  64 bins at a time, so a long interval costs no more per
//                  bin than as many short ones.
#include "pdd_internal.h"

namespace pdd {

namespace {

constexpr int kZapThreads = 256;
constexpr int kZapMaxRows = 64;
constexpr int kZapApplyThreads = 64;

typedef float f32x2 __attribute__((ext_vector_type(2)));

// float32 bits -> unsigned key with the order of the values (negative
// values: all bits flipped; others: the sign bit set), and back.  -0 sorts
// just below +0; a NaN is outside the contract.
__device__ __forceinline__ uint32_t zap_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float zap_unkey(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

// Merge exchange (Knuth 5.2.2 M; Batcher's odd-even merge sort for a power
// of two) on RC keys: the network of the next power of two without the
// comparators that reach past RC -- those would hold the largest key on
// their upper side and exchange nothing.
template <int RC>
__device__ __forceinline__ void zap_sort(uint32_t (&a)[RC]) {
#pragma unroll
  for (int p = 1; p < RC; p <<= 1) {
#pragma unroll
    for (int k = p; k >= 1; k >>= 1) {
#pragma unroll
      for (int j = k % p; j + k < RC; j += 2 * k) {
#pragma unroll
        for (int i = 0; i < k; ++i) {
          const int lo = i + j, hi = i + j + k;
          if (hi < RC && lo / (2 * p) == hi / (2 * p)) {
            const uint32_t x = a[lo], y = a[hi];
            a[lo] = min(x, y);
            a[hi] = max(x, y);
          }
        }
      }
    }
  }
}

template <int RC>
__global__ __launch_bounds__(kZapThreads) void k_zap_percentile(const float* __restrict__ powers,
                                                                int R, int64_t nn, int64_t ld,
                                                                int rank, float* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * kZapThreads + threadIdx.x;
  if (k >= nn) return;
  uint32_t a[RC];
#pragma unroll
  for (int r = 0; r < RC; ++r)  // (R uniform: scalar branches; the loads are independent)
    a[r] = r < R ? zap_key(powers[(int64_t)r * ld + k]) : 0xffffffffu;
  zap_sort<RC>(a);
  uint32_t res = a[0];
#pragma unroll
  for (int r = 1; r < RC; ++r) res = r == rank - 1 ? a[r] : res;
  out[k] = zap_unkey(res);
}

// bins: [nz][2] inclusive intervals; block (iv, d) fills interval iv of row d.
__global__ __launch_bounds__(kZapApplyThreads) void k_zap_apply(float* __restrict__ powers,
                                                                int64_t ldp, f32x2* __restrict__ spec,
                                                                int64_t lds, int64_t nn,
                                                                const int32_t* __restrict__ bins,
                                                                int64_t nz) {
  const int64_t d = blockIdx.x / nz, iv = blockIdx.x % nz;
  // (the contract is 1 <= lo <= hi < nn: a list that breaks it writes nothing
  // outside the row)
  const int64_t lo = max((int64_t)bins[2 * iv], (int64_t)1);
  const int64_t hi = min((int64_t)bins[2 * iv + 1], nn - 1);
  float* prow = powers + d * ldp;
  const f32x2 fill = {0.70710677f, 0.70710677f};
  for (int64_t k = lo + threadIdx.x; k <= hi; k += kZapApplyThreads) {
    prow[k] = 1.0f;
    if (spec) spec[d * lds + k] = fill;
  }
}

template <int RC>
void zap_launch(const float* powers, int R, int64_t nn, int64_t ld, int rank, float* out,
                hipStream_t st) {
  k_zap_percentile<RC><<<(unsigned)cdiv(nn, kZapThreads), kZapThreads, 0, st>>>(powers, R, nn, ld,
                                                                              rank, out);
}

}  // namespace

}  // namespace pdd

using namespace pdd;

extern "C" {

int pdd_zap_percentile(const float* powers, int64_t R, int64_t nn, int64_t ld, int rank,
                       float* out, void* stream) {
  PDD_REQUIRE(powers && out, "pdd_zap_percentile: null pointer");
  PDD_REQUIRE(R >= 1 && R <= kZapMaxRows, "pdd_zap_percentile: R out of range 1..%d",
              kZapMaxRows);
  PDD_REQUIRE(rank >= 1 && rank <= R, "pdd_zap_percentile: rank out of range 1..R");
  PDD_REQUIRE(nn > 0 && ld >= nn && nn < (1ll << 31), "pdd_zap_percentile: bad shape");
  hipStream_t st = as_stream(stream);
  switch ((R + 7) / 8) {
    case 1: zap_launch<8>(powers, (int)R, nn, ld, rank, out, st); break;
    case 2: zap_launch<16>(powers, (int)R, nn, ld, rank, out, st); break;
    case 3: zap_launch<24>(powers, (int)R, nn, ld, rank, out, st); break;
    case 4: zap_launch<32>(powers, (int)R, nn, ld, rank, out, st); break;
    case 5: zap_launch<40>(powers, (int)R, nn, ld, rank, out, st); break;
    case 6: zap_launch<48>(powers, (int)R, nn, ld, rank, out, st); break;
    case 7: zap_launch<56>(powers, (int)R, nn, ld, rank, out, st); break;
    default: zap_launch<64>(powers, (int)R, nn, ld, rank, out, st); break;
  }
  PDD_LAUNCHED();
  return 0;
}

int pdd_zap_apply(float* powers, int64_t ldp, float* spec, int64_t lds, int64_t D, int64_t nn,
                  const int32_t* bins, int64_t nz, void* stream) {
  PDD_REQUIRE(D >= 0 && nz >= 0, "pdd_zap_apply: bad shape");
  if (D == 0 || nz == 0) return 0;
  PDD_REQUIRE(powers && bins, "pdd_zap_apply: null pointer");
  PDD_REQUIRE(nn >= 2 && ldp >= nn && (!spec || lds >= nn) && nn < (1ll << 31),
              "pdd_zap_apply: bad shape");
  PDD_REQUIRE(((uintptr_t)spec & 7) == 0, "pdd_zap_apply: spec must be 8-byte aligned");
  PDD_REQUIRE(D * nz < (1ll << 31), "pdd_zap_apply: too large");
  k_zap_apply<<<(unsigned)(D * nz), kZapApplyThreads, 0, as_stream(stream)>>>(
      powers, ldp, reinterpret_cast<f32x2*>(spec), lds, nn, bins, nz);
  PDD_LAUNCHED();
  return 0;
}

}  // extern "C"
