// libpdd: SIGPROC filterbanks packed below a byte (1, 2 and 4 bits per
// sample), gfx950.  Order within a byte is SIGPROC's: the first channel sits
// in the least significant bits (4 bits: low nibble first, as
// formats/psrfits.py unpack_4bit; 2 bits: shifts 0, 2, 4, 6; 1 bit: bit 0
// first), so channel i of a little-endian word w is (w >> i*nbits) & mask.
//
//   pdd_unpack_bits                the general path: packed rows -> uint8 rows,
//                                  for everything that takes an 8-bit block
//   pdd_zdm_packed_int_downsample  the hot path: pdd_zdm_int_downsample
//                                  (pdd_ops.hip) reading packed rows, no 8-bit
//                                  intermediate in HBM
#include "pdd_internal.h"

namespace pdd {

namespace {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------- unpack
// 16 channels per thread: one 2 NB-byte load, one 16-byte store.  Host side
// guarantees nchan % 16 == 0, `in` and ld_in multiples of 2 NB, `out` and
// ld_out multiples of 16.
template <int NB>
__global__ __launch_bounds__(256) void k_unpack_vec(const uint8_t* __restrict__ in, int64_t nspec,
                                                    int64_t per_row, int64_t ld_in,
                                                    uint8_t* __restrict__ out, int64_t ld_out) {
  constexpr uint32_t MASK = (1u << NB) - 1u;
  const int64_t total = nspec * per_row;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * 256) {
    const int64_t s = i / per_row, g = i - s * per_row;
    const uint8_t* p = in + s * ld_in + g * (2 * NB);
    uint64_t w;
    if constexpr (NB == 4) {
      const uint2 q = *reinterpret_cast<const uint2*>(p);
      w = ((uint64_t)q.y << 32) | q.x;
    } else if constexpr (NB == 2) {
      w = *reinterpret_cast<const uint32_t*>(p);
    } else {
      w = *reinterpret_cast<const uint16_t*>(p);
    }
    uint32_t o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t v = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        v |= ((uint32_t)(w >> ((4 * q + e) * NB)) & MASK) << (8 * e);
      o[q] = v;
    }
    *reinterpret_cast<uint4*>(out + s * ld_out + g * 16) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// Narrow fallback (any row length, any stride): one packed byte per thread,
// 8 / NB single-byte stores.
template <int NB>
__global__ __launch_bounds__(256) void k_unpack_bytes(const uint8_t* __restrict__ in,
                                                      int64_t nspec, int64_t row_bytes,
                                                      int64_t ld_in, uint8_t* __restrict__ out,
                                                      int64_t ld_out) {
  constexpr int PER = 8 / NB;
  constexpr uint32_t MASK = (1u << NB) - 1u;
  const int64_t total = nspec * row_bytes;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * 256) {
    const int64_t s = i / row_bytes, b = i - s * row_bytes;
    const uint32_t w = in[s * ld_in + b];
    uint8_t* o = out + s * ld_out + b * PER;
#pragma unroll
    for (int e = 0; e < PER; ++e) o[e] = (uint8_t)((w >> (e * NB)) & MASK);
  }
}

// ---------------------------------------------------------------- fused prologue
// Sum of the 32 / NB bit fields of one word (exact, <= 120).
template <int NB>
__device__ __forceinline__ uint32_t field_sum(uint32_t w) {
  if constexpr (NB == 1) {
    return (uint32_t)__popc(w);
  } else if constexpr (NB == 2) {
    w = (w & 0x33333333u) + ((w >> 2) & 0x33333333u);  // nibbles <= 6
    w = (w & 0x0f0f0f0fu) + ((w >> 4) & 0x0f0f0f0fu);  // bytes <= 12
    return (w * 0x01010101u) >> 24;
  } else {
    w = (w & 0x0f0f0f0fu) + ((w >> 4) & 0x0f0f0f0fu);  // bytes <= 30
    return (w * 0x01010101u) >> 24;
  }
}

// Per-spectrum channel mean of packed rows, rounded half to even:
// m[s] = rint(double(sum) / double(nchan)), the value k_zdm_int_ds_vec takes
// from k_spectrum_mean_vec (pdd_ops.hip).  One wave per spectrum, 16-byte
// loads, exact integer sum of the bit fields.
template <int NB>
__global__ __launch_bounds__(256) void k_packed_mean(const uint8_t* __restrict__ in, int64_t nspec,
                                                     int64_t nchan, int64_t row_bytes, int64_t ld,
                                                     int* __restrict__ m) {
  const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (s >= nspec) return;
  const uint4* row = reinterpret_cast<const uint4*>(in + s * ld);
  const int64_t nv = row_bytes / 16;
  unsigned long long acc = 0;
  for (int64_t v = lane; v < nv; v += 64) {
    const uint4 q = row[v];
    acc += field_sum<NB>(q.x) + field_sum<NB>(q.y) + field_sum<NB>(q.z) + field_sum<NB>(q.w);
  }
  const double total = wave_sum_d((double)acc);  // integers < 2^53: exact
  if (lane == 0) m[s] = (int)rint(total / (double)nchan);
}

// pdd_zdm_int_downsample's kernel (k_zdm_int_ds_vec, pdd_ops.hip) on packed
// rows: out[c][j] = offset + sum_{k < f} z(x[j f + k][c], m[j f + k]), the
// same MODEs.  One block = 64 outputs (64 f spectra) x 256 channels.  A
// thread decodes 32 channels of a row from one 4 NB-byte load (16 / 8 / 4
// bytes), so a wave reads 8 rows x 8 contiguous loads; the 256 x 66 uint16
// tile (33 KiB for every NB) is written transposed and every wave then stores
// whole 64-output rows of the image.  Tile row e*8 + seg holds channel
// seg*32 + e: the 8 segments of a wave land in neighbouring rows, not 32 rows
// (a multiple of 32 LDS words) apart.
template <int NB, int MODE>
__global__ __launch_bounds__(256) void k_packed_zdm_ds(const uint8_t* __restrict__ in,
                                                       int64_t nchan, int64_t ld,
                                                       const int* __restrict__ mean, int f,
                                                       uint16_t* __restrict__ out, int64_t ld_out,
                                                       int64_t nout, int64_t tiles_c, int offset) {
  constexpr int CPT = 32;       // channels per thread
  constexpr int TC = 8 * CPT;   // channels per block
  constexpr int PW = 32 / NB;   // channels per 32-bit word
  constexpr uint32_t MASK = (1u << NB) - 1u;
  __shared__ uint16_t tile[TC][66];
  const int64_t tj = blockIdx.x / tiles_c, tc = blockIdx.x % tiles_c;
  const int64_t j0 = tj * 64, c0 = tc * TC;
  const int seg = threadIdx.x & 7, r0 = threadIdx.x >> 3;
  const int64_t c = c0 + seg * CPT;
  const uint8_t* col = in + c * NB / 8;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int jl = r0 + 32 * pass;
    const int64_t j = j0 + jl;
    int acc[CPT];
#pragma unroll
    for (int e = 0; e < CPT; ++e) acc[e] = offset;
    if (j < nout && c < nchan) {
      for (int k = 0; k < f; ++k) {
        const int64_t t = j * f + k;
        uint32_t w[NB];
        if constexpr (NB == 4) {
          const uint4 q = *reinterpret_cast<const uint4*>(col + t * ld);
          w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        } else if constexpr (NB == 2) {
          const uint2 q = *reinterpret_cast<const uint2*>(col + t * ld);
          w[0] = q.x; w[1] = q.y;
        } else {
          w[0] = *reinterpret_cast<const uint32_t*>(col + t * ld);
        }
        const int m = MODE ? mean[t] : 0;
#pragma unroll
        for (int e = 0; e < CPT; ++e) {
          const int z = (int)((w[e / PW] >> ((e % PW) * NB)) & MASK) - m;
          acc[e] += MODE == 2 ? (z & 255) : z;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < CPT; ++e) tile[e * 8 + seg][jl] = (uint16_t)acc[e];
  }
  __syncthreads();
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t j = j0 + tx;
#pragma unroll 4
  for (int p = ty; p < TC; p += 4) {
    const int64_t cc = c0 + (p & 7) * CPT + (p >> 3);
    if (j < nout && cc < nchan) out[cc * ld_out + j] = tile[p][tx];
  }
}

int grid_for(int64_t items) {
  int64_t g = cdiv(items, 256);
  if (g > 2048 * 8) g = 2048 * 8;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace

}  // namespace pdd

using namespace pdd;

extern "C" {

int pdd_unpack_bits(const void* in, int nbits, int64_t nspec, int64_t nchan, int64_t ld_in_bytes,
                    uint8_t* out, int64_t ld_out, void* stream) {
  PDD_REQUIRE(in && out, "pdd_unpack_bits: null pointer");
  PDD_REQUIRE(nbits == 1 || nbits == 2 || nbits == 4,
              "pdd_unpack_bits: nbits %d not supported (1, 2, 4)", nbits);
  PDD_REQUIRE(nspec >= 0 && nchan > 0 && (nchan * nbits) % 8 == 0,
              "pdd_unpack_bits: bad shape (nchan * nbits must be a multiple of 8)");
  const int64_t row_bytes = nchan * nbits / 8;
  PDD_REQUIRE(ld_in_bytes >= row_bytes && ld_out >= nchan, "pdd_unpack_bits: stride too small");
  if (nspec == 0) return 0;
  hipStream_t s = as_stream(stream);
  const uint8_t* x = static_cast<const uint8_t*>(in);
  const int64_t lw = 2 * nbits;  // bytes of the vector path's load
  const bool vec = nchan % 16 == 0 && (uintptr_t)out % 16 == 0 && ld_out % 16 == 0 &&
                   (uintptr_t)in % lw == 0 && ld_in_bytes % lw == 0;
#define UP(B)                                                                                    \
  do {                                                                                           \
    if (vec)                                                                                     \
      k_unpack_vec<B><<<grid_for(nspec * (nchan / 16)), 256, 0, s>>>(x, nspec, nchan / 16,       \
                                                                     ld_in_bytes, out, ld_out);  \
    else                                                                                         \
      k_unpack_bytes<B><<<grid_for(nspec * row_bytes), 256, 0, s>>>(x, nspec, row_bytes,         \
                                                                    ld_in_bytes, out, ld_out);   \
  } while (0)
  if (nbits == 1) UP(1);
  else if (nbits == 2) UP(2);
  else UP(4);
#undef UP
  PDD_LAUNCHED();
  return 0;
}

int pdd_zdm_packed_int_downsample(const void* in, int nbits, int64_t nspec, int64_t nchan,
                                  int64_t ld_in_bytes, int64_t factor, int mode, int offset,
                                  uint16_t* out, int64_t ld_out, void* stream) {
  PDD_REQUIRE(in && out, "pdd_zdm_packed_int_downsample: null pointer");
  PDD_REQUIRE(nbits == 1 || nbits == 2 || nbits == 4,
              "pdd_zdm_packed_int_downsample: nbits %d not supported (1, 2, 4)", nbits);
  PDD_REQUIRE(mode >= PDD_ZDM_NONE && mode <= PDD_ZDM_WRAP,
              "pdd_zdm_packed_int_downsample: bad mode %d", mode);
  PDD_REQUIRE(nspec >= 0 && nchan > 0, "pdd_zdm_packed_int_downsample: bad shape");
  PDD_REQUIRE(factor >= 1 && factor <= 64 && 64 % factor == 0,
              "pdd_zdm_packed_int_downsample: factor must divide 64");
  const int64_t row_bytes = nchan * nbits / 8;
  PDD_REQUIRE((nchan * nbits) % 8 == 0 && row_bytes % 16 == 0 && ld_in_bytes % 16 == 0 &&
                  (uintptr_t)in % 16 == 0 && ld_in_bytes >= row_bytes,
              "pdd_zdm_packed_int_downsample: packed rows must be 16-byte aligned "
              "(nchan * nbits / 8 %% 16 == 0, ld_in_bytes %% 16 == 0)");
  PDD_REQUIRE(ld_out >= nspec / factor, "pdd_zdm_packed_int_downsample: ld_out too small");
  const int vmax = (1 << nbits) - 1;
  const int lo = mode == PDD_ZDM_INT ? -vmax * (int)factor : 0;
  const int hi = (mode == PDD_ZDM_WRAP ? 255 : vmax) * (int)factor;
  PDD_REQUIRE(offset + lo >= 0 && offset + hi <= 65535,
              "pdd_zdm_packed_int_downsample: offset %d cannot hold [%d, %d] in uint16", offset,
              lo, hi);
  if (nspec < factor) return 0;
  const int64_t nout = nspec / factor;
  const int64_t tiles_c = cdiv(nchan, 256);
  const int64_t blocks = cdiv(nout, 64) * tiles_c;
  PDD_REQUIRE(blocks < (1ll << 31), "pdd_zdm_packed_int_downsample: too large");
  hipStream_t s = as_stream(stream);
  const uint8_t* x = static_cast<const uint8_t*>(in);
  int* mean = nullptr;
  if (mode != PDD_ZDM_NONE) {
    mean = static_cast<int*>(scratch(s, kScratchSmall, (size_t)nspec * sizeof(int)));
    if (!mean) return -2;
  }
#define PZ(B, M)                                                                         \
  k_packed_zdm_ds<B, M><<<(unsigned)blocks, 256, 0, s>>>(x, nchan, ld_in_bytes, mean,    \
                                                         (int)factor, out, ld_out, nout, \
                                                         tiles_c, offset)
#define PB(B)                                                                            \
  do {                                                                                   \
    if (mean)                                                                            \
      k_packed_mean<B><<<(unsigned)cdiv(nspec, 4), 256, 0, s>>>(x, nspec, nchan,         \
                                                                row_bytes, ld_in_bytes,  \
                                                                mean);                   \
    if (mode == PDD_ZDM_NONE) PZ(B, 0);                                                  \
    else if (mode == PDD_ZDM_INT) PZ(B, 1);                                              \
    else PZ(B, 2);                                                                       \
  } while (0)
  if (nbits == 1) PB(1);
  else if (nbits == 2) PB(2);
  else PB(4);
#undef PB
#undef PZ
  PDD_LAUNCHED();
  return 0;
}

}  // extern "C"
