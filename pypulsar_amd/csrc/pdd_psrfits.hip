// libpdd: PSRFITS search-mode subint decode on the device (SURVEY.md §8(f)
// rank 3), gfx950.  One HBM-bound pass replaces the reference's host chain
// (formats/psrfits.py):
//   unpack_4bit            psrfits.py:37-50   (low nibble first)
//   read_subint            psrfits.py:67-107  ((data*scales)+offsets)*weights,
//                                             float32, in that order
//   get_spectra            psrfits.py:140-183 (concatenate subints, transpose
//                                             to [chan, time], skip/trunc,
//                                             band flip when the band ascends)
// Input: nsub consecutive BINTABLE rows copied verbatim (row_bytes each; the
// DATA column starts data_off bytes into a row), big-endian as on disk:
// nbits 4 (two samples per byte), 8 (uint8), 16 (int16, FITS 'I'), 32
// (float32, FITS 'E').  wso: [nsub][3][nchan] float32 scale, offset, weight.
// Output: out[c'][j] for j < N, the sample g = s0 + j of the concatenated
// subints (subint g / nsblk, spectrum g % nsblk), c' = flip ? nchan-1-c : c.
// 64 x 64 (spectrum x channel) tiles through LDS: the decode reads rows
// channel-fastest (coalesced), the store writes channel rows time-fastest.
#include "pdd_internal.h"

namespace pdd {

namespace {

template <int NBITS>
__device__ __forceinline__ float decode(const uint8_t* __restrict__ data, int64_t idx) {
  if constexpr (NBITS == 8) {
    return (float)data[idx];
  } else if constexpr (NBITS == 4) {
    const uint8_t b = data[idx >> 1];
    return (float)((idx & 1) ? (b >> 4) : (b & 15));
  } else if constexpr (NBITS == 16) {
    const uint8_t* p = data + 2 * idx;
    return (float)(int16_t)(((uint16_t)p[0] << 8) | p[1]);
  } else {
    const uint8_t* p = data + 4 * idx;
    const uint32_t u = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    return __uint_as_float(u);
  }
}

template <int NBITS>
__global__ __launch_bounds__(256) void k_psrfits_subints(
    const uint8_t* __restrict__ raw, int64_t row_bytes, int64_t data_off, int64_t nsblk,
    int64_t nchan, const float* __restrict__ wso, int64_t s0, int64_t N, int flip,
    float* __restrict__ out, int64_t ld_out, int64_t tiles_c) {
  __shared__ float tile[64][65];
  const int64_t tt = blockIdx.x / tiles_c, tc = blockIdx.x % tiles_c;
  const int64_t j0 = tt * 64, c0 = tc * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t c = c0 + tx;
#pragma unroll 4
  for (int i = ty; i < 64; i += 4) {
    const int64_t j = j0 + i;
    if (j < N && c < nchan) {
      const int64_t g = s0 + j, sub = g / nsblk, s = g - sub * nsblk;
      const uint8_t* data = raw + sub * row_bytes + data_off;
      const float* p = wso + sub * 3 * nchan;
      const float v = decode<NBITS>(data, s * nchan + c);
      tile[i][tx] = ((v * p[c]) + p[nchan + c]) * p[2 * nchan + c];
    }
  }
  __syncthreads();
#pragma unroll 4
  for (int i = ty; i < 64; i += 4) {
    const int64_t cc = c0 + i, j = j0 + tx;
    if (j < N && cc < nchan) out[(flip ? nchan - 1 - cc : cc) * ld_out + j] = tile[tx][i];
  }
}

// ---- pdd_psrfits_block: SUBINT rows -> the stream's time-major raw block ----
// A streaming pass, no transpose: DATA and the block are both channel-fastest.
// A lane owns a chunk of VEC consecutive channels (one LB-byte load) and keeps
// it over the spectra of one subint, so its scale, offset and weight (read
// big-endian from the row itself) are loaded once per chunk and block, not
// once per sample.  DATA is only byte-aligned in general: where every
// (spectrum, polarisation) run of a subint shares one residue mod LB
// (nchan nbits / 8 a multiple of LB) the chunks are shifted by the `shc`
// channels that bring the loads onto LB-byte addresses -- lane 0 takes the
// peeled head [0, shc), the last lane the short tail, both element by element
// -- and every other shape falls to the element path spectrum by spectrum
// (a chunk is loaded wide whenever its absolute address allows).  Stores take
// the widest form the absolute output address allows (16, 8, 4 bytes, else
// elements).
// Channels per lane: 16 for uint8 output (one 16-byte store; an 8- or 16-byte
// load), 4 for float32 output (8 from 4-bit samples): one 16-byte store a lane,
// so a wave's store covers whole consecutive lines.  (16 channels a lane with
// four float4 stores 64 bytes apart measured 0.36 of the HBM rate from 8-bit
// rows where this form's 32-bit case, one store a lane, measured 0.59.)
template <int NBITS, bool F32OUT>
struct BlockCfg {
  static constexpr int VEC = !F32OUT ? 16 : NBITS == 4 ? 8 : 4;
  static constexpr int LB = VEC * NBITS / 8;  // bytes per wide load: 4, 8 or 16
  static constexpr int W = LB / 4;
};

constexpr int kBlockSPT = 32;  // spectra per lane and block

__device__ __forceinline__ int64_t cdiv_dev(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct BlockArgs {
  const uint8_t* rows;
  int64_t row_bytes, data_off, scl_off, offs_off, wts_off;
  int64_t nsblk, nchan, s0, n, ld_out, sub_first, chunks_per_sub, ts;
  int npol, pol0, lc_log2, peel;
  void* out;
};

// big-endian float32 at any byte address
__device__ __forceinline__ float be_f32(const uint8_t* p) {
  uint32_t u;
  if (((uintptr_t)p & 3) == 0) {
    u = __builtin_bswap32(*reinterpret_cast<const uint32_t*>(p));
  } else {
    u = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
  }
  return __uint_as_float(u);
}

// elements e0 .. e0+cnt-1 of a subint's DATA as float
template <int NBITS, int VEC>
__device__ __forceinline__ void load_chunk(const uint8_t* __restrict__ data, int64_t e0, int cnt,
                                           float (&v)[VEC]) {
  constexpr int LB = VEC * NBITS / 8, W = LB / 4;
  const uint8_t* p = data + (NBITS == 4 ? (e0 >> 1) : e0 * (NBITS / 8));
  const bool wide = cnt == VEC && ((uintptr_t)p & (LB - 1)) == 0 && (NBITS != 4 || !(e0 & 1));
  if (wide) {
    uint32_t w[W];
    if constexpr (W == 4) {
      const uint4 q = *reinterpret_cast<const uint4*>(p);
      w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else if constexpr (W == 2) {
      const uint2 q = *reinterpret_cast<const uint2*>(p);
      w[0] = q.x; w[1] = q.y;
    } else {
      w[0] = *reinterpret_cast<const uint32_t*>(p);
    }
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      if constexpr (NBITS == 4) {
        v[i] = (float)((w[i >> 3] >> (4 * (i & 7))) & 15u);
      } else if constexpr (NBITS == 8) {
        v[i] = (float)((w[i >> 2] >> (8 * (i & 3))) & 255u);
      } else if constexpr (NBITS == 16) {
        const uint32_t b = __builtin_bswap32(w[i >> 1]);
        v[i] = (float)(int16_t)((i & 1) ? (b & 0xffffu) : (b >> 16));
      } else {
        v[i] = __uint_as_float(__builtin_bswap32(w[i]));
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = i < cnt ? decode<NBITS>(data, e0 + i) : 0.0f;
  }
}

template <int VEC>
__device__ __forceinline__ void store_chunk(float* __restrict__ p, const float (&f)[VEC], int cnt) {
  if (cnt == VEC && ((uintptr_t)p & 15) == 0) {
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q)
      reinterpret_cast<float4*>(p)[q] = make_float4(f[4 * q], f[4 * q + 1], f[4 * q + 2], f[4 * q + 3]);
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i)
      if (i < cnt) p[i] = f[i];
  }
}

// VEC == 16 only (4- and 8-bit input)
__device__ __forceinline__ void store_chunk(uint8_t* __restrict__ p, const uint32_t (&b)[16], int cnt) {
  const uintptr_t a = (uintptr_t)p;
  if (cnt == 16 && (a & 3) == 0) {
    uint32_t w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      w[q] = b[4 * q] | (b[4 * q + 1] << 8) | (b[4 * q + 2] << 16) | (b[4 * q + 3] << 24);
    if ((a & 15) == 0) {
      *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    } else if ((a & 7) == 0) {
      reinterpret_cast<uint2*>(p)[0] = make_uint2(w[0], w[1]);
      reinterpret_cast<uint2*>(p)[1] = make_uint2(w[2], w[3]);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) reinterpret_cast<uint32_t*>(p)[q] = w[q];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i < cnt) p[i] = (uint8_t)b[i];
  }
}

template <int NBITS, bool F32OUT, bool SUM>
__global__ __launch_bounds__(256) void k_psrfits_block(const BlockArgs a) {
  constexpr int VEC = BlockCfg<NBITS, F32OUT>::VEC, LB = BlockCfg<NBITS, F32OUT>::LB;
  const int64_t subt = blockIdx.x / a.chunks_per_sub, tchunk = blockIdx.x - subt * a.chunks_per_sub;
  const int64_t sub = a.sub_first + subt, base = sub * a.nsblk;
  // spectra [lo, hi) of this subint are wanted; the block takes [sb, se) of them
  const int64_t lo = a.s0 > base ? a.s0 - base : 0;
  const int64_t hi = a.s0 + a.n - base < a.nsblk ? a.s0 + a.n - base : a.nsblk;
  const int64_t sb = tchunk * a.ts, se = sb + a.ts < hi ? sb + a.ts : hi;
  if (se <= lo || sb >= se) return;
  const int LC = 1 << a.lc_log2, TY = 256 >> a.lc_log2;
  const int tx = threadIdx.x & (LC - 1), ty = threadIdx.x >> a.lc_log2;
  const uint8_t* __restrict__ row = a.rows + sub * a.row_bytes;
  const uint8_t* __restrict__ data = row + a.data_off;
  const int64_t nchan = a.nchan;
  int shc = 0;  // channels ahead of the first LB-aligned address
  if (a.peel) {
    const int shbits = (int)((LB - ((uintptr_t)data & (LB - 1))) & (LB - 1)) * 8;
    if (shbits % NBITS == 0) shc = shbits / NBITS;
  }
  const int first = shc > 0 ? 0 : 1;
  const int64_t nck = cdiv_dev(nchan - shc, VEC) + 1 - first;
  for (int64_t k = tx; k < nck; k += LC) {
    const int64_t c_lo = shc + (k + first - 1) * VEC;
    const int64_t cb = c_lo > 0 ? c_lo : 0;
    const int64_t ce = c_lo + VEC < nchan ? c_lo + VEC : nchan;
    const int cnt = (int)(ce - cb);
    float scl0[VEC], of0[VEC], scl1[VEC], of1[VEC], wt[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const bool ok = i < cnt;
      const int64_t c = cb + i;
      wt[i] = (a.wts_off >= 0 && ok) ? be_f32(row + a.wts_off + 4 * c) : 1.0f;
      if constexpr (F32OUT) {
        const int64_t pc = (int64_t)a.pol0 * nchan + c;
        scl0[i] = (a.scl_off >= 0 && ok) ? be_f32(row + a.scl_off + 4 * pc) : 1.0f;
        of0[i] = (a.offs_off >= 0 && ok) ? be_f32(row + a.offs_off + 4 * pc) : 0.0f;
        if constexpr (SUM) {
          scl1[i] = (a.scl_off >= 0 && ok) ? be_f32(row + a.scl_off + 4 * (pc + nchan)) : 1.0f;
          of1[i] = (a.offs_off >= 0 && ok) ? be_f32(row + a.offs_off + 4 * (pc + nchan)) : 0.0f;
        }
      }
    }
    int64_t s = sb + ty;
    if (s < lo) s += (lo - s + TY - 1) / TY * TY;
#pragma unroll 2
    for (; s < se; s += TY) {
      const int64_t e0 = (s * a.npol + a.pol0) * nchan + cb;
      const int64_t j = base + s - a.s0;
      float v[VEC];
      load_chunk<NBITS, VEC>(data, e0, cnt, v);
      if constexpr (F32OUT) {
        float f[VEC];
        if constexpr (SUM) {
          float v1[VEC];
          load_chunk<NBITS, VEC>(data, e0 + nchan, cnt, v1);
#pragma unroll
          for (int i = 0; i < VEC; ++i)
            f[i] = (((v[i] * scl0[i]) + of0[i]) + ((v1[i] * scl1[i]) + of1[i])) * wt[i];
        } else {
#pragma unroll
          for (int i = 0; i < VEC; ++i) f[i] = ((v[i] * scl0[i]) + of0[i]) * wt[i];
        }
        store_chunk<VEC>(reinterpret_cast<float*>(a.out) + j * a.ld_out + cb, f, cnt);
      } else {
        uint32_t b[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) b[i] = wt[i] != 0.0f ? (uint32_t)v[i] : 0u;
        store_chunk(reinterpret_cast<uint8_t*>(a.out) + j * a.ld_out + cb, b, cnt);
      }
    }
  }
}

}  // namespace

}  // namespace pdd

using namespace pdd;

extern "C" {

int pdd_psrfits_block(const uint8_t* rows, int64_t nsub, int64_t row_bytes, int64_t data_off,
                      int64_t scl_off, int64_t offs_off, int64_t wts_off, int nbits, int64_t nsblk,
                      int64_t nchan, int npol, int pol0, int npol_sum, int64_t s0, int64_t n,
                      int out_code, void* out, int64_t ld_out, void* stream) {
  PDD_REQUIRE(rows && out, "pdd_psrfits_block: null pointer");
  PDD_REQUIRE(nbits == 4 || nbits == 8 || nbits == 16 || nbits == 32,
              "pdd_psrfits_block: nbits %d not supported (4, 8, 16, 32)", nbits);
  PDD_REQUIRE(nsub >= 1 && nsblk >= 1 && nchan >= 1 && npol >= 1 && n >= 0 && s0 >= 0 &&
                  row_bytes >= 1 && data_off >= 0,
              "pdd_psrfits_block: bad shape");
  PDD_REQUIRE(nsblk < (1ll << 31) && nchan < (1ll << 31) && nsub < (1ll << 31) && npol <= 4,
              "pdd_psrfits_block: too large");
  PDD_REQUIRE(nbits != 4 || ((int64_t)npol * nchan) % 2 == 0,
              "pdd_psrfits_block: 4-bit spectra of %lld samples do not fill whole bytes",
              (long long)((int64_t)npol * nchan));
  PDD_REQUIRE(s0 + n <= nsub * nsblk, "pdd_psrfits_block: samples [%lld, %lld) beyond %lld",
              (long long)s0, (long long)(s0 + n), (long long)(nsub * nsblk));
  PDD_REQUIRE(data_off + (nsblk * npol * nchan * nbits + 7) / 8 <= row_bytes,
              "pdd_psrfits_block: DATA column exceeds the row");
  PDD_REQUIRE(scl_off >= -1 && offs_off >= -1 && wts_off >= -1,
              "pdd_psrfits_block: a column offset is -1 (not applied) or >= 0");
  PDD_REQUIRE(scl_off < 0 || scl_off + 4 * (int64_t)npol * nchan <= row_bytes,
              "pdd_psrfits_block: DAT_SCL column exceeds the row");
  PDD_REQUIRE(offs_off < 0 || offs_off + 4 * (int64_t)npol * nchan <= row_bytes,
              "pdd_psrfits_block: DAT_OFFS column exceeds the row");
  PDD_REQUIRE(wts_off < 0 || wts_off + 4 * nchan <= row_bytes,
              "pdd_psrfits_block: DAT_WTS column exceeds the row");
  PDD_REQUIRE(pol0 >= 0 && (npol_sum == 1 || npol_sum == 2) && pol0 + npol_sum <= npol,
              "pdd_psrfits_block: polarisations %d .. %d of %d", pol0, pol0 + npol_sum - 1, npol);
  PDD_REQUIRE(ld_out >= nchan, "pdd_psrfits_block: ld_out %lld < nchan %lld", (long long)ld_out,
              (long long)nchan);
  PDD_REQUIRE(out_code == PDD_U8 || out_code == PDD_F32,
              "pdd_psrfits_block: output is PDD_U8 or PDD_F32");
  PDD_REQUIRE(out_code != PDD_U8 || (nbits <= 8 && npol_sum == 1 && scl_off == -1 && offs_off == -1),
              "pdd_psrfits_block: PDD_U8 output needs nbits <= 8, one polarisation and no "
              "scales or offsets");
  if (n == 0) return 0;
  // (BlockCfg: channels a lane and bytes a wide load)
  const int vec = out_code == PDD_U8 ? 16 : nbits == 4 ? 8 : 4, lb = vec * nbits / 8;
  BlockArgs a;
  a.rows = rows;
  a.row_bytes = row_bytes; a.data_off = data_off;
  a.scl_off = scl_off; a.offs_off = offs_off; a.wts_off = wts_off;
  a.nsblk = nsblk; a.nchan = nchan; a.s0 = s0; a.n = n; a.ld_out = ld_out;
  a.npol = npol; a.pol0 = pol0;
  a.out = out;
  // every (spectrum, polarisation) run of a subint at one residue mod lb
  a.peel = (nchan * nbits) % 8 == 0 && (nchan * nbits / 8) % lb == 0;
  // channel lanes: the chunks of one spectrum plus the peeled head, a power of two <= 256
  a.lc_log2 = 0;
  while (a.lc_log2 < 8 && (1ll << a.lc_log2) < cdiv(nchan, vec) + 1) ++a.lc_log2;
  a.ts = (int64_t)kBlockSPT * (256 >> a.lc_log2);
  a.chunks_per_sub = cdiv(nsblk, a.ts);
  a.sub_first = s0 / nsblk;
  const int64_t nsubt = (s0 + n - 1) / nsblk - a.sub_first + 1;
  const int64_t blocks = nsubt * a.chunks_per_sub;
  PDD_REQUIRE(blocks < (1ll << 31), "pdd_psrfits_block: too large");
  hipStream_t s = as_stream(stream);
#define PB(B, F, S) k_psrfits_block<B, F, S><<<(unsigned)blocks, 256, 0, s>>>(a)
  const bool sum = npol_sum == 2;
  if (out_code == PDD_U8) {
    if (nbits == 4) PB(4, false, false);
    else PB(8, false, false);
  } else if (nbits == 4) {
    if (sum) PB(4, true, true); else PB(4, true, false);
  } else if (nbits == 8) {
    if (sum) PB(8, true, true); else PB(8, true, false);
  } else if (nbits == 16) {
    if (sum) PB(16, true, true); else PB(16, true, false);
  } else {
    if (sum) PB(32, true, true); else PB(32, true, false);
  }
#undef PB
  PDD_LAUNCHED();
  return 0;
}

int pdd_psrfits_subints(const uint8_t* raw, int64_t nsub, int64_t row_bytes, int64_t data_off,
                        int nbits, int64_t nsblk, int64_t nchan, const float* wso, int64_t s0,
                        int64_t N, int flip, float* out, int64_t ld_out, void* stream) {
  PDD_REQUIRE(raw && wso && out, "pdd_psrfits_subints: null pointer");
  PDD_REQUIRE(nbits == 4 || nbits == 8 || nbits == 16 || nbits == 32,
              "pdd_psrfits_subints: nbits %d not supported (4, 8, 16, 32)", nbits);
  PDD_REQUIRE(nsub >= 1 && nsblk >= 1 && nchan >= 1 && N >= 0 && s0 >= 0 && ld_out >= N,
              "pdd_psrfits_subints: bad shape");
  PDD_REQUIRE(s0 + N <= nsub * nsblk, "pdd_psrfits_subints: samples [%lld, %lld) beyond %lld",
              (long long)s0, (long long)(s0 + N), (long long)(nsub * nsblk));
  PDD_REQUIRE(data_off + (nsblk * nchan * nbits + 7) / 8 <= row_bytes,
              "pdd_psrfits_subints: DATA column exceeds the row");
  if (N == 0) return 0;
  const int64_t tiles_c = cdiv(nchan, 64);
  const int64_t blocks = cdiv(N, 64) * tiles_c;
  PDD_REQUIRE(blocks < (1ll << 31), "pdd_psrfits_subints: too large");
  hipStream_t s = as_stream(stream);
#define PF(B)                                                                                      \
  k_psrfits_subints<B><<<(unsigned)blocks, 256, 0, s>>>(raw, row_bytes, data_off, nsblk, nchan, \
                                                        wso, s0, N, flip, out, ld_out, tiles_c)
  if (nbits == 4) PF(4);
  else if (nbits == 8) PF(8);
  else if (nbits == 16) PF(16);
  else PF(32);
#undef PF
  PDD_LAUNCHED();
  return 0;
}

}  // extern "C"
