// libpdd: batched brute-force DM sweep, gfx950.
//
//   plane[d][t] = sum_c X(c, t + table[d][c]),  t < n_out
//
// which is, per DM trial, Spectra.dedisperse(dm, padval, trim) followed by the
// channel sum of bin/waterfaller.py:140 (formats/spectra.py:229-260).
//
// Design:
//  * a workgroup owns a tile of DB = NW*DPW DM trials x TB = S*64*G samples;
//    each wave owns DPW trials, each lane G*S output samples per trial;
//  * channels are processed in chunks of `cc`; for every channel of a chunk
//    the workgroup stages X(c, t0 + bmin_c + e), e < 64*G + span_c, into LDS
//    ONCE (bmin_c / span_c = min / extent of the tile's shifts at channel c)
//    and all DB trials read it from there: one coalesced HBM/L2 read feeds
//    DB trials;
//  * the LDS image is STRIPED: element e packs the S samples
//    e, e+Q, e+2Q, ... (Q = 64*G) of the tile, so one aligned 8- or 16-byte
//    ds_read per lane returns S samples that share the SAME shift -- the
//    shift is wave-uniform per (trial, channel), read from the channel-major
//    table through the scalar cache;
//  * float32 input accumulates in float32 registers (exact for integer data);
//  * 8-bit input is staged as packed u16 pairs and accumulated with plain
//    32-bit integer adds (two u16 lanes per add, no carry while <= 257
//    channels are summed), flushed to float32 every 256 channels -- exact;
//  * blockIdx is remapped so the n_dblk DM blocks of one time tile run
//    back to back on ONE XCD and re-read the tile's input from that XCD's L2.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "fx_walk.h"
#include "pdd_internal.h"
#include "sweep_plan.h"

namespace pdd {

template <bool U8, int S>
struct ElemOf {
  static constexpr int bytes = U8 ? 2 * S : 4 * S;
  static_assert(bytes == 8 || bytes == 16, "LDS element must be 8 or 16 bytes");
  using type = typename std::conditional<bytes == 8, uint2, uint4>::type;
};

__device__ __forceinline__ uint32_t get_w(const uint2& v, int i) { return i == 0 ? v.x : v.y; }
__device__ __forceinline__ uint32_t get_w(const uint4& v, int i) {
  return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w));
}
__device__ __forceinline__ void set_w(uint2& v, int i, uint32_t x) {
  if (i == 0) v.x = x; else v.y = x;
}
__device__ __forceinline__ void set_w(uint4& v, int i, uint32_t x) {
  if (i == 0) v.x = x; else if (i == 1) v.y = x; else if (i == 2) v.z = x; else v.w = x;
}

__device__ __forceinline__ int64_t wrap_mod(int64_t s, int64_t N) {
  int64_t r = s % N;
  return r < 0 ? r + N : r;
}

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;

// Stage one channel of the striped image with the reference pad semantics
// (register path: used for 8-bit data and for float32 channels whose window
// leaves [0, N), i.e. edge tiles, pads and rotation).
template <bool U8, int S, int Q, int NT>
__device__ __forceinline__ void stage_channel_regs(typename ElemOf<U8, S>::type* dst,
                                                   const void* xv, int64_t ld, int c, int64_t N,
                                                   int64_t sb, int ne, bool inside, int pad_mode,
                                                   const float* __restrict__ padvals) {
  using E = typename ElemOf<U8, S>::type;
  constexpr int WORDS = U8 ? S / 2 : S;
  if constexpr (U8) {
    const uint8_t* row = reinterpret_cast<const uint8_t*>(xv) + (int64_t)c * ld;
    if (inside) {
      const uint8_t* rb = row + sb;
      for (int e = threadIdx.x; e < ne; e += NT) {
        E v;
#pragma unroll
        for (int h = 0; h < WORDS; ++h)
          set_w(v, h, (uint32_t)rb[e + (2 * h) * Q] | ((uint32_t)rb[e + (2 * h + 1) * Q] << 16));
        dst[e] = v;
      }
    } else {
      const uint32_t pv = (pad_mode == PDD_PAD_VALUE) ? (uint32_t)padvals[c] : 0u;
      for (int e = threadIdx.x; e < ne; e += NT) {
        E v;
#pragma unroll
        for (int h = 0; h < WORDS; ++h) {
          uint32_t lo, hi;
          const int64_t s0 = sb + e + (2 * h) * Q, s1 = s0 + Q;
          if (pad_mode == PDD_PAD_ROTATE) {
            lo = row[wrap_mod(s0, N)];
            hi = row[wrap_mod(s1, N)];
          } else {
            lo = (s0 >= 0 && s0 < N) ? (uint32_t)row[s0] : pv;
            hi = (s1 >= 0 && s1 < N) ? (uint32_t)row[s1] : pv;
          }
          set_w(v, h, lo | (hi << 16));
        }
        dst[e] = v;
      }
    }
  } else {
    const float* row = reinterpret_cast<const float*>(xv) + (int64_t)c * ld;
    const float pv = (pad_mode == PDD_PAD_VALUE) ? padvals[c] : 0.f;
    for (int e = threadIdx.x; e < ne; e += NT) {
      E v;
#pragma unroll
      for (int k = 0; k < S; ++k) {
        const int64_t s = sb + e + k * Q;
        float f;
        if (inside) f = row[s];
        else if (pad_mode == PDD_PAD_ROTATE) f = row[wrap_mod(s, N)];
        else f = (s >= 0 && s < N) ? row[s] : pv;
        set_w(v, k, __float_as_uint(f));
      }
      dst[e] = v;
    }
  }
}

// float32 channel fully inside [0, N): asynchronous LDS-DMA
// (global_load_lds_dword) straight into the striped image.  One
// wave-instruction writes 256 contiguous LDS bytes = 16 elements x 4 stripes;
// lane l loads sample (e0 + l/4) of stripe l%4.  Elements past ne are filled
// from a clamped (valid) address and never read.
template <int Q, int NW>
__device__ __forceinline__ int stage_channel_dma(uint4* dst, const float* rb, int ne, int w,
                                                 int lane) {
  // Issued through inline asm: hipcc would otherwise treat the DMA as a
  // pending LDS write and put vmcnt(0) in front of every ds_read of the OTHER
  // buffer.  The kernel waits for it explicitly (vmcnt(0) before the barrier
  // that publishes the chunk).
  const int nq = (ne + 15) >> 4;
  const int k = lane & 3;
  for (int q = w; q < nq; q += NW) {
    const int e = min(q * 16 + (lane >> 2), ne - 1);
    const float* src = rb + e + k * Q;
    const uint32_t lds_addr = (uint32_t)(uintptr_t)(lds_void_t*)(dst + q * 16);
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dword %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(src), "s"(__builtin_amdgcn_readfirstlane(lds_addr))
        : "memory");
  }
  return w < nq ? (nq - 1 - w) / NW + 1 : 0;  // DMAs this wave issued
}

// s_waitcnt vmcnt(n) for a run-time n (the counter field is an immediate):
// "all but the youngest n vector-memory operations of this wave are done".
__device__ __forceinline__ void wait_vmcnt(int n) {
  n = __builtin_amdgcn_readfirstlane(n);
  switch (n < 63 ? n : 63) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
    case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
    case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
    case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    case 13: asm volatile("s_waitcnt vmcnt(13)" ::: "memory"); break;
    case 14: asm volatile("s_waitcnt vmcnt(14)" ::: "memory"); break;
    case 15: asm volatile("s_waitcnt vmcnt(15)" ::: "memory"); break;
    case 16: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
    case 17: asm volatile("s_waitcnt vmcnt(17)" ::: "memory"); break;
    case 18: asm volatile("s_waitcnt vmcnt(18)" ::: "memory"); break;
    case 19: asm volatile("s_waitcnt vmcnt(19)" ::: "memory"); break;
    case 20: asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); break;
    case 21: asm volatile("s_waitcnt vmcnt(21)" ::: "memory"); break;
    case 22: asm volatile("s_waitcnt vmcnt(22)" ::: "memory"); break;
    case 23: asm volatile("s_waitcnt vmcnt(23)" ::: "memory"); break;
    case 24: asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); break;
    case 25: asm volatile("s_waitcnt vmcnt(25)" ::: "memory"); break;
    case 26: asm volatile("s_waitcnt vmcnt(26)" ::: "memory"); break;
    case 27: asm volatile("s_waitcnt vmcnt(27)" ::: "memory"); break;
    case 28: asm volatile("s_waitcnt vmcnt(28)" ::: "memory"); break;
    case 29: asm volatile("s_waitcnt vmcnt(29)" ::: "memory"); break;
    case 30: asm volatile("s_waitcnt vmcnt(30)" ::: "memory"); break;
    case 31: asm volatile("s_waitcnt vmcnt(31)" ::: "memory"); break;
    case 32: asm volatile("s_waitcnt vmcnt(32)" ::: "memory"); break;
    case 33: asm volatile("s_waitcnt vmcnt(33)" ::: "memory"); break;
    case 34: asm volatile("s_waitcnt vmcnt(34)" ::: "memory"); break;
    case 35: asm volatile("s_waitcnt vmcnt(35)" ::: "memory"); break;
    case 36: asm volatile("s_waitcnt vmcnt(36)" ::: "memory"); break;
    case 37: asm volatile("s_waitcnt vmcnt(37)" ::: "memory"); break;
    case 38: asm volatile("s_waitcnt vmcnt(38)" ::: "memory"); break;
    case 39: asm volatile("s_waitcnt vmcnt(39)" ::: "memory"); break;
    case 40: asm volatile("s_waitcnt vmcnt(40)" ::: "memory"); break;
    case 41: asm volatile("s_waitcnt vmcnt(41)" ::: "memory"); break;
    case 42: asm volatile("s_waitcnt vmcnt(42)" ::: "memory"); break;
    case 43: asm volatile("s_waitcnt vmcnt(43)" ::: "memory"); break;
    case 44: asm volatile("s_waitcnt vmcnt(44)" ::: "memory"); break;
    case 45: asm volatile("s_waitcnt vmcnt(45)" ::: "memory"); break;
    case 46: asm volatile("s_waitcnt vmcnt(46)" ::: "memory"); break;
    case 47: asm volatile("s_waitcnt vmcnt(47)" ::: "memory"); break;
    case 48: asm volatile("s_waitcnt vmcnt(48)" ::: "memory"); break;
    case 49: asm volatile("s_waitcnt vmcnt(49)" ::: "memory"); break;
    case 50: asm volatile("s_waitcnt vmcnt(50)" ::: "memory"); break;
    case 51: asm volatile("s_waitcnt vmcnt(51)" ::: "memory"); break;
    case 52: asm volatile("s_waitcnt vmcnt(52)" ::: "memory"); break;
    case 53: asm volatile("s_waitcnt vmcnt(53)" ::: "memory"); break;
    case 54: asm volatile("s_waitcnt vmcnt(54)" ::: "memory"); break;
    case 55: asm volatile("s_waitcnt vmcnt(55)" ::: "memory"); break;
    case 56: asm volatile("s_waitcnt vmcnt(56)" ::: "memory"); break;
    case 57: asm volatile("s_waitcnt vmcnt(57)" ::: "memory"); break;
    case 58: asm volatile("s_waitcnt vmcnt(58)" ::: "memory"); break;
    case 59: asm volatile("s_waitcnt vmcnt(59)" ::: "memory"); break;
    case 60: asm volatile("s_waitcnt vmcnt(60)" ::: "memory"); break;
    case 61: asm volatile("s_waitcnt vmcnt(61)" ::: "memory"); break;
    case 62: asm volatile("s_waitcnt vmcnt(62)" ::: "memory"); break;
    case 63: asm volatile("s_waitcnt vmcnt(63)" ::: "memory"); break;
  }
}

template <bool U8, int S, int G, int DPW, int NW, int CC, int NBUF>
__global__ __launch_bounds__(NW * 64) void k_sweep(
    const void* __restrict__ xv, int64_t ld, int C, int64_t N, const int* __restrict__ rel,
    int Dpad, int D, const int* __restrict__ bmin, const int* __restrict__ bspan, int pad_mode,
    const float* __restrict__ padvals, float* __restrict__ out, int64_t ld_out, int64_t n_out,
    int dbg, int stride, int n_tblk, int n_dblk) {
  constexpr int cc = CC;
  constexpr int Q = 64 * G;
  constexpr int TB = S * Q;
  constexpr int DB = NW * DPW;
  constexpr int NT = NW * 64;
  constexpr int WORDS = U8 ? S / 2 : S;  // 32-bit words per LDS element
  constexpr bool DMA = !U8 && S == 4;
  using E = typename ElemOf<U8, S>::type;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  E* lds = reinterpret_cast<E*>(smem);
  const int64_t buf_elems = (int64_t)cc * stride;  // one of the two chunk buffers

  // XCD-aware tile order: blocks b and b+8 share an XCD; give each XCD a
  // contiguous run of L so the DM blocks of one time tile share its L2.
  const int total = n_tblk * n_dblk;
  const int full = (total / 8) * 8;
  const int bid = blockIdx.x;
  const int L = (bid < full) ? (bid % 8) * (total / 8) + bid / 8 : bid;
  const int dblk = L % n_dblk, tblk = L / n_dblk;
  const int64_t t0 = (int64_t)tblk * TB;
  // wave index as a scalar so the per-(channel, trial) offsets are fetched by
  // scalar loads (one s_load per channel for the wave's DPW trials)
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int d0 = dblk * DB + w * DPW;
  const int* bmin_b = bmin + (int64_t)dblk * C;
  const int* bspan_b = bspan + (int64_t)dblk * C;

  // stage chunk [c0, c0 + ncc) into buffer `b`; returns the number of
  // LDS-DMA instructions this wave left in flight
  auto stage = [&](int c0, int b) -> int {
    const int ncc = min(cc, C - c0);
    int ndma = 0;
    E* base = lds + b * buf_elems;
    for (int i = 0; i < ncc; ++i) {
      const int c = c0 + i;
      const int bm = bmin_b[c];
      const int ne = Q + bspan_b[c];
      const int64_t sb = t0 + bm;
      const bool inside = (sb >= 0) && (sb + (int64_t)(S - 1) * Q + ne <= N);
      E* dst = base + (int64_t)i * stride;
      if constexpr (DMA) {
        if (inside) {
          ndma += stage_channel_dma<Q, NW>(reinterpret_cast<uint4*>(dst),
                                           reinterpret_cast<const float*>(xv) + (int64_t)c * ld + sb,
                                           ne, w, lane);
          continue;
        }
      }
      stage_channel_regs<U8, S, Q, NT>(dst, xv, ld, c, N, sb, ne, inside, pad_mode, padvals);
    }
    return ndma;
  };

  float accf[DPW][G][S];
#pragma unroll
  for (int j = 0; j < DPW; ++j)
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int k = 0; k < S; ++k) accf[j][g][k] = 0.f;
  uint32_t acc16[U8 ? DPW : 1][U8 ? G : 1][U8 ? WORDS : 1];
  if constexpr (U8) {
#pragma unroll
    for (int j = 0; j < DPW; ++j)
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int h = 0; h < WORDS; ++h) acc16[j][g][h] = 0u;
  }
  int since_flush = 0;

  // Ring of NBUF channel-chunk buffers: chunks k+1 .. k+NBUF-1 are staged
  // (LDS-DMA in flight for float32) while chunk k is accumulated.  One
  // barrier per chunk; before it every wave waits with a COUNTED vmcnt that
  // retires only chunk k's DMAs and keeps the younger chunks in flight.
  int pend[NBUF];  // pend[s] = DMAs this wave has in flight for chunk k+s
#pragma unroll
  for (int s2 = 0; s2 < NBUF; ++s2) pend[s2] = 0;
#pragma unroll
  for (int s2 = 0; s2 < NBUF - 1; ++s2)
    if (s2 * cc < C) pend[s2] = stage(s2 * cc, s2);
  int cur = 0;
  for (int c0 = 0; c0 < C; c0 += cc) {
    const int ncc = min(cc, C - c0);
    if constexpr (DMA) {
      int younger = 0;
#pragma unroll
      for (int s2 = 1; s2 < NBUF - 1; ++s2) younger += pend[s2];
      wait_vmcnt(younger);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // offsets of this chunk's channels for the wave's trials, into SGPRs
    // before any LDS read is issued (scalar loads share lgkmcnt with LDS):
    // rel[c][d] = table[d][c] - bmin(block, c) >= 0
    int off[CC][DPW];
#pragma unroll
    for (int i = 0; i < CC; ++i) {
      const int* rp = rel + (int64_t)(c0 + (i < ncc ? i : 0)) * Dpad + d0;
#pragma unroll
      for (int j = 0; j < DPW; ++j) off[i][j] = rp[j];
    }
    {
      // refill the buffer chunk k-1 used (every wave is past it: barrier)
      const int cn = c0 + (NBUF - 1) * cc;
      int b = cur + NBUF - 1;
      b = b >= NBUF ? b - NBUF : b;
      const int n = cn < C ? stage(cn, b) : 0;
#pragma unroll
      for (int s2 = 0; s2 < NBUF - 2; ++s2) pend[s2] = pend[s2 + 1];
      pend[NBUF - 2] = n;
    }
    // ---- accumulate: every wave reads the image at its trials' shifts
    const E* img = lds + cur * buf_elems;
#pragma unroll
    for (int i = 0; i < CC; ++i) {
      if (i >= ncc) break;
      const E* base = img + (int64_t)i * stride + lane;
#pragma unroll
      for (int j = 0; j < DPW; ++j) {
        const E* p = base + off[i][j];
        E v[G];
#pragma unroll
        for (int g = 0; g < G; ++g) v[g] = p[g * 64];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if constexpr (U8) {
#pragma unroll
            for (int h = 0; h < WORDS; ++h) acc16[j][g][h] += get_w(v[g], h);
          } else {
#pragma unroll
            for (int k = 0; k < S; ++k) accf[j][g][k] += __uint_as_float(get_w(v[g], k));
          }
        }
      }
      if constexpr (U8) {
        if (++since_flush == 256) {
          since_flush = 0;
#pragma unroll
          for (int j = 0; j < DPW; ++j)
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
              for (int h = 0; h < WORDS; ++h) {
                accf[j][g][2 * h] += (float)(acc16[j][g][h] & 0xffffu);
                accf[j][g][2 * h + 1] += (float)(acc16[j][g][h] >> 16);
                acc16[j][g][h] = 0u;
              }
        }
      }
    }
    cur = cur + 1 == NBUF ? 0 : cur + 1;
  }
  if constexpr (U8) {
#pragma unroll
    for (int j = 0; j < DPW; ++j)
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int h = 0; h < WORDS; ++h) {
          accf[j][g][2 * h] += (float)(acc16[j][g][h] & 0xffffu);
          accf[j][g][2 * h + 1] += (float)(acc16[j][g][h] >> 16);
        }
  }
  // ---- write the tile (lane-consecutive samples: coalesced rows)
#pragma unroll
  for (int j = 0; j < DPW; ++j) {
    const int d = d0 + j;
    if (d >= D) continue;
    float* orow = out + (int64_t)d * ld_out;
#pragma unroll
    for (int k = 0; k < S; ++k)
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int64_t t = t0 + k * Q + g * 64 + lane;
        if (t < n_out) orow[t] = accf[j][g][k];
      }
  }
}

// ------------------------------------------------------------------ LDS helpers
typedef __attribute__((address_space(3))) float lds_float_t;
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) f32x2_t lds_f32x2_t;
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) f32x4_t lds_f32x4_t;

__device__ __forceinline__ uint32_t lds_addr_of(const void* p) {
  return (uint32_t)(uintptr_t)(const lds_float_t*)p;
}

// 256 consecutive ints (1 KiB) -> LDS by one dwordx4 LDS-DMA
// wave-instruction (lane l: ints 4l .. 4l + 3); lanes past n (a multiple of
// 4) stay idle, so nothing lands past the n ints; src and lds_dst 16-B
// aligned.  Used for the per-chunk metadata rows, so they travel on the same
// counted vmcnt as the sample DMAs and never touch a VGPR early.  (Measured
// and dropped, round 5: the rows one chunk further ahead, kept in flight
// through the next barrier by the compiler's LDS-DMA builtin -- the
// staging-free skeleton 48 -> 32 ms per configs[3] launch, but production
// 102.2 -> 107.1 ms.)
__device__ __forceinline__ void dma_ints4(int* lds_dst, const int* src, int n, int lane) {
  const uint32_t la = __builtin_amdgcn_readfirstlane(lds_addr_of(lds_dst));
  if (lane * 4 < n) {
    const int* p = src + lane * 4;
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(p), "s"(la)
        : "memory");
  }
}


// ------------------------------------------------------------------ interleaved
// The production sweep.  A pre-pass (k_interleave) rewrites each channel of
// the input segment as 16-byte ELEMENTS that hold 4 samples a quarter of the
// segment apart:
//     R[c][j] = ( X(c, b+j), X(c, b+j+Qs), X(c, b+j+2Qs), X(c, b+j+3Qs) ),
//     b = t_base + lo,  j < nR = Qs + hi - lo + 64
// with the reference pad semantics (value / rotate) baked in, so the sweep
// never sees an edge.  It is a pure re-layout (each sample is read once and
// written once, ~1x the input bytes; u8/f32 input both become float32).
// A sweep tile (DB trials x Tq elements) then stages each channel's window
// R[c][t0 + bmin_c - lo + e], e < Tq + span_c, with 1 KiB LDS-DMA
// instructions (global_load_lds_dwordx4, one element per lane) issued by
// dedicated loader waves, and every compute-wave ds_read_b128 at a trial's
// (wave-uniform) shift returns 4 samples -- one per quarter -- that share it.
// Output (trial d, element e, quarter k) is plane[d][t_base + e + k*Qs].
// Each thread writes kIlPer elements 256 apart, issuing all their loads
// before any store (memory-level parallelism for the strided quarter reads).
constexpr int kIlPer = 4;
// Input layouts of the pre-pass: channel-major rows (x[c * ld + s]) or the
// "pieces" layout an all-gather of channel-major time slices produces,
// x[(s / P) * C * P + c * P + s % P] (P = piece, a power of two; C = all
// channels of the plan) ...
// ... or time-major spectra (file order), x[s * ld_t + c].
struct InLayout {
  int64_t ld;      // channel-major row stride (piece == 0, ld_t == 0)
  int64_t piece;   // P, 0 = channel-major
  int psh;         // log2(P)
  int64_t pstride; // C * P
  int64_t ld_t;    // time-major spectrum stride, 0 = not time-major
  __device__ __forceinline__ int64_t at(int c, int64_t s) const {
    if (ld_t) return s * ld_t + c;
    return piece ? (s >> psh) * pstride + (int64_t)c * piece + (s & (piece - 1))
                 : (int64_t)c * ld + s;
  }
};

// Sample sources of the pre-pass and of stage 1: at(c, s) = sample s of
// channel c.  Rows of uint8_t / uint16_t / float in an InLayout ...
template <typename InT>
struct SrcRows {
  const InT* x;
  InLayout lay;
  __device__ __forceinline__ SrcRows(const void* xv, const InLayout& l)
      : x(static_cast<const InT*>(xv)), lay(l) {}
  __device__ __forceinline__ InT at(int c, int64_t s) const { return x[lay.at(c, s)]; }
};
// ... or an 8-bit block DOWNSAMPLED by F <= 4 on the fly
// (formats/spectra.py:329-351: sample s = the co-add of raw samples
// s*F .. s*F + F - 1, <= 1020, exact), so a downsampled DDplan step never
// writes and re-reads its downsampled copy; pads and rotation act on the
// downsampled series (N = raw length / F).  VEC: the F raw bytes of a sample
// are one aligned 2- or 4-byte load (summed by v_sad_u8 against zero).
template <int F, bool VEC>
struct SrcCoadd {
  const uint8_t* x;
  int64_t ld;
  __device__ __forceinline__ SrcCoadd(const void* xv, const InLayout& l)
      : x(static_cast<const uint8_t*>(xv)), ld(l.ld) {}
  __device__ __forceinline__ uint32_t at(int c, int64_t s) const {
    const uint8_t* q = x + (int64_t)c * ld + s * F;
    if constexpr (VEC && F == 4) {
      return __builtin_amdgcn_sad_u8(*reinterpret_cast<const uint32_t*>(q), 0u, 0u);
    } else if constexpr (VEC && F == 2) {
      return __builtin_amdgcn_sad_u8((uint32_t)*reinterpret_cast<const uint16_t*>(q), 0u, 0u);
    } else {
      uint32_t a = 0;
#pragma unroll
      for (int k = 0; k < F; ++k) a += q[k];
      return a;
    }
  }
};

// The two element kinds: float32 QUARTERS (4 samples Qs apart) and, for 8-bit
// data (and 16-bit data <= 1023), u16 EIGHTHS: 8 samples as packed u16 pairs
// (word h = sample 2h | sample 2h+1 << 16; pads are integers, checked by the
// caller).  add: one pattern term of stage 1, component by component.
struct ElemF32 {
  using value_t = float;
  using elem_t = float4;
  static constexpr int S = 4;
  static __device__ __forceinline__ float4 pack(const float (&v)[4]) {
    return make_float4(v[0], v[1], v[2], v[3]);
  }
  static __device__ __forceinline__ float4 add(float4 a, const float4& b) {
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    return a;
  }
};
struct ElemU16 {
  using value_t = uint32_t;
  using elem_t = uint4;
  static constexpr int S = 8;
  static __device__ __forceinline__ uint4 pack(const uint32_t (&v)[8]) {
    return make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16),
                      v[6] | (v[7] << 16));
  }
  static __device__ __forceinline__ uint4 add(const uint4& a, const uint4& b) {
    return make_uint4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
  }
};

// The reference pad semantics, once: inside [0, N) the data, else the
// rotated sample or the channel's pad value.
template <typename V>
__device__ __forceinline__ V pad_value(int pad_mode, const float* __restrict__ padvals, int c) {
  return (pad_mode == PDD_PAD_VALUE) ? (V)padvals[c] : (V)0;
}
template <typename V, typename Src>
__device__ __forceinline__ V padded_sample(const Src& src, int c, int64_t s, int64_t N,
                                           int pad_mode, V pv) {
  if (s >= 0 && s < N) return (V)src.at(c, s);
  if (pad_mode == PDD_PAD_ROTATE) return (V)src.at(c, wrap_mod(s, N));
  return pv;
}

// Arguments of every pre-pass instance (x: the input of the instance's
// source; R: float4 or uint4 elements, the same 16 bytes), so one table
// (kIlInstances) selects and launches them.
struct IlArgs {
  const void* x;
  InLayout lay;
  int64_t N, base, Qs, nR;
  int pad_mode;
  const float* padvals;
  void* R;
};

template <typename Src, typename El>
__global__ __launch_bounds__(256) void k_interleave(const IlArgs a) {
  using V = typename El::value_t;
  const Src src(a.x, a.lay);
  const int c = blockIdx.y;
  const int64_t j0 = (int64_t)blockIdx.x * (256 * kIlPer) + threadIdx.x;
  const V pv = pad_value<V>(a.pad_mode, a.padvals, c);
  V v[kIlPer][El::S];
#pragma unroll
  for (int i = 0; i < kIlPer; ++i)
#pragma unroll
    for (int k = 0; k < El::S; ++k)
      v[i][k] = padded_sample<V>(src, c, a.base + j0 + i * 256 + k * a.Qs, a.N, a.pad_mode, pv);
  typename El::elem_t* R = static_cast<typename El::elem_t*>(a.R);
#pragma unroll
  for (int i = 0; i < kIlPer; ++i) {
    const int64_t j = j0 + i * 256;
    if (j < a.nR) R[(int64_t)c * a.nR + j] = El::pack(v[i]);
  }
}

// Vector form for 16-B aligned rows (F = 2 or 4): a thread builds J = 16 / F
// CONSECUTIVE elements from one 16-byte load per eighth (J co-adds), and
// stores them as J contiguous 16-byte elements (a wave writes 4-8 KiB in one
// piece); the element run's base must be a multiple of J (base % J == 0,
// Qs % J == 0).  Runs that touch a pad or the wrap take the per-sample path.
template <int F>
__global__ __launch_bounds__(256) void k_interleave_u16_ds_v(const IlArgs a) {
  static_assert(F == 2 || F == 4, "16-byte loads of 4 or 8 co-adds");
  constexpr int J = 16 / F;
  const SrcCoadd<F, false> src(a.x, a.lay);
  const int c = blockIdx.y;
  const int64_t j0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * J;
  if (j0 >= a.nR) return;
  const uint32_t pv = pad_value<uint32_t>(a.pad_mode, a.padvals, c);
  const uint8_t* row = src.x + (int64_t)c * src.ld;
  uint32_t v[J][8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int64_t s0 = a.base + j0 + k * a.Qs;
    if (s0 >= 0 && s0 + J <= a.N) {
      const uint4 q = *reinterpret_cast<const uint4*>(row + s0 * F);
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        if constexpr (F == 4) {
          v[h][k] = __builtin_amdgcn_sad_u8(w[h], 0u, 0u);
        } else {
          v[2 * h][k] = __builtin_amdgcn_sad_u8(w[h] & 0xffffu, 0u, 0u);
          v[2 * h + 1][k] = __builtin_amdgcn_sad_u8(w[h] >> 16, 0u, 0u);
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < J; ++e) v[e][k] = padded_sample<uint32_t>(src, c, s0 + e, a.N, a.pad_mode, pv);
    }
  }
  uint4* dst = static_cast<uint4*>(a.R) + (int64_t)c * a.nR + j0;
#pragma unroll
  for (int e = 0; e < J; ++e)
    if (j0 + e < a.nR) dst[e] = ElemU16::pack(v[e]);
}

// Every pre-pass instance: (downsampling factor, vector form, plan dtype,
// element kind) -> kernel and the elements one of its blocks builds.  vec:
// 16 = the J-consecutive form, 1 = aligned F-byte co-add loads, 0 = bytes.
typedef void (*il_fn)(IlArgs);
struct IlInstance {
  int ds, vec, dtype;
  bool u16;
  il_fn fn;
  int per_block;
};
static const IlInstance kIlInstances[] = {
    {1, 0, PDD_U8, true, k_interleave<SrcRows<uint8_t>, ElemU16>, 256 * kIlPer},
    {1, 0, PDD_U16, true, k_interleave<SrcRows<uint16_t>, ElemU16>, 256 * kIlPer},
    {1, 0, PDD_U8, false, k_interleave<SrcRows<uint8_t>, ElemF32>, 256 * kIlPer},
    {1, 0, PDD_U16, false, k_interleave<SrcRows<uint16_t>, ElemF32>, 256 * kIlPer},
    {1, 0, PDD_F32, false, k_interleave<SrcRows<float>, ElemF32>, 256 * kIlPer},
    {2, 16, PDD_U16, true, k_interleave_u16_ds_v<2>, 256 * 8},
    {4, 16, PDD_U16, true, k_interleave_u16_ds_v<4>, 256 * 4},
    {2, 1, PDD_U16, true, k_interleave<SrcCoadd<2, true>, ElemU16>, 256 * kIlPer},
    {2, 0, PDD_U16, true, k_interleave<SrcCoadd<2, false>, ElemU16>, 256 * kIlPer},
    {3, 0, PDD_U16, true, k_interleave<SrcCoadd<3, false>, ElemU16>, 256 * kIlPer},
    {4, 1, PDD_U16, true, k_interleave<SrcCoadd<4, true>, ElemU16>, 256 * kIlPer},
    {4, 0, PDD_U16, true, k_interleave<SrcCoadd<4, false>, ElemU16>, 256 * kIlPer},
};

// ------------------------------------------------------------------ factorised sweep
// Exact factorisation of the 8-bit sweep over groups of fx = 4 (or 2)
// adjacent channels.  Within a group (channels c0..c0+3) trial d's shifts are its base
// shift b = table[d][c0] plus a RELATIVE pattern r = (0, r1, r2, r3); the
// group's contribution to plane[d][t] is
//     sum_k X(c0 + k, t + b + r_k) = S_r(t + b),  S_r(u) = sum_k X(c0 + k, u + r_k),
// the same samples summed in integers, so the plane is bit-identical to the
// channel-by-channel sum.  Across a DM grid a group takes few distinct
// patterns (configs[3]: 27 769 over 1024 groups, 6.8 per group): stage 1
// (k_fx_patterns) writes every pattern series S_r once as a u16-eighths image
// row (sums of four samples <= 1020 stay exact in the packed u16 lanes), and
// stage 2 is k_sweep_il over the GROUPS, each trial reading its pattern's
// window at its base shift: a quarter of the LDS reads and adds of the
// channel sweep, the same window staging (a tile stages every pattern its
// trials use: 3.8 of a group's patterns per 48-trial block, 0.88 x the
// channel windows' elements).
__global__ __launch_bounds__(256) void k_fx_patterns(const uint4* __restrict__ R, int64_t nR,
                                                     const int4* __restrict__ pat, int fx,
                                                     uint4* __restrict__ P) {
  const int64_t p = blockIdx.x;
  const int4 q = pat[p];  // {c0, r1, r2, r3}
  const uint4* r0 = R + (int64_t)q.x * nR;
  const int64_t j0 = (int64_t)blockIdx.y * (256 * kIlPer) + threadIdx.x;
  auto at = [&](int k, int r, int64_t j) -> uint4 {
    const int64_t e = j + r;  // elements no trial reads may fall outside the row
    return (e >= 0 && e < nR) ? r0[(int64_t)k * nR + e] : make_uint4(0u, 0u, 0u, 0u);
  };
  uint4 v[kIlPer];
#pragma unroll
  for (int i = 0; i < kIlPer; ++i) {
    const int64_t j = j0 + i * 256;
    if (j >= nR) continue;
    const uint4 a = at(0, 0, j), b = at(1, q.y, j);
    const uint4 c = fx > 2 ? at(2, q.z, j) : make_uint4(0u, 0u, 0u, 0u);
    const uint4 d = fx > 3 ? at(3, q.w, j) : make_uint4(0u, 0u, 0u, 0u);
    v[i] = make_uint4(a.x + b.x + c.x + d.x, a.y + b.y + c.y + d.y, a.z + b.z + c.z + d.z,
                      a.w + b.w + c.w + d.w);
  }
#pragma unroll
  for (int i = 0; i < kIlPer; ++i) {
    const int64_t j = j0 + i * 256;
    if (j < nR) P[p * nR + j] = v[i];
  }
}

// Stage 1 through LDS: one workgroup per (group, kFxE-element block) loads
// the group's four rows over the block (+ the group's relative-shift range)
// ONCE and writes every pattern of the group from them (the plain kernel
// above reads four rows per pattern element from L2: 4 x 16 B per 16 B
// written).  gtab: [NG + 1] first pattern of each group, then [NG] x {lo,
// hi} = the group's min(0, r) / max(0, r) over its patterns (hi - lo <=
// kFxRspan, checked by the plan), then [n_pat] x {first, last - nR}: the
// pattern row's elements stage 2 reads (fx_build): kFxE-element blocks
// outside that range are not written.  (kFxE, kFxRspan, kFxEf: sweep_plan.h.)
// The group's pattern descriptors 64 at a time, one wave-wide load: lane i
// holds pattern pb + i's relative shifts and row range (fx_build), which the
// pattern loops take by v_readlane -- no dependent scalar loads per pattern.
struct FxBatch {
  int y, z, w, lo, hi;
};
__device__ __forceinline__ FxBatch fx_batch(const int4* __restrict__ pat, const int* __restrict__ rng,
                                            int pb, int p1) {
  const int pl = min(pb + (int)(threadIdx.x & 63), p1 - 1);
  const int4 q = pat[pl];
  return {q.y, q.z, q.w, rng[2 * pl], rng[2 * pl + 1]};
}

// Arguments of every LDS stage-1 instance: the pre-pass's (x: the
// u16-eighths image or the sweep's input; lay .. padvals only for the input
// sources; R: the pattern image, uint4 or float4 elements) and the plan's
// tables, so one table (kFxS1Instances) sets their LDS limits and launches them.
struct FxS1Args : IlArgs {
  const int4* pat;
  const int* gtab;
  int NG;
  // the persistent form (k_fx_stage1_p): NG x element blocks items, the item
  // counters of its queues (zeroed before the launch), and whether 8-bit
  // input may be loaded in aligned words (fx_s1_words)
  int64_t n_items;
  unsigned int* queue;
  int words;
  int slot;  // byte offset of the item slot in the dynamic LDS (behind the rows)
};

// Stage-1 sources.  load_row fills one LDS row with the elements [i0, i0 + W)
// of channel c's image row (zeros outside [0, nR): elements no trial reads).
// The image rows a pre-pass wrote (R in HBM: downsampled input) ...
struct FxFromImage {
  using El = ElemU16;
  static constexpr int kBlock = kFxE;
  static constexpr bool kNontemporal = false;
  const uint4* R;
  int64_t nR;
  __device__ __forceinline__ explicit FxFromImage(const FxS1Args& a)
      : R(static_cast<const uint4*>(a.x)), nR(a.nR) {}
  __device__ __forceinline__ void load_row(uint4* L, int c, int64_t i0, int W) const {
    for (int e = threadIdx.x; e < W; e += 256) {
      const int64_t i = i0 + e;
      L[e] = (i >= 0 && i < nR) ? R[(int64_t)c * nR + i] : make_uint4(0u, 0u, 0u, 0u);
    }
  }
  // the same element by element (the persistent kernel's prefetch)
  __device__ __forceinline__ bool inner(int64_t i0, int W, int = 0) const {
    return i0 >= 0 && i0 + W <= nR;
  }
  __device__ __forceinline__ uint4 elem(int c, int64_t i, bool in) const {
    return (in || (i >= 0 && i < nR)) ? R[(int64_t)c * nR + i] : make_uint4(0u, 0u, 0u, 0u);
  }
};
// ... or straight from the input (no image R in HBM): each row element is
// built the way k_interleave would -- S samples X(c, base + i + m*Qs) with the
// reference pads (value / rotate).  Saves the image's write and read, and the
// interleave launch, per segment (the per-rank work of a DM-sharded step that
// does not shrink with the world size).  Integer input gives u16 eighths;
// float32 input the float32 QUARTERS, each pattern element the float sum of
// its group's fx elements in channel order (x_c0 + x_c0+1 [+ x_c0+2 +
// x_c0+3]); the sweep then adds pattern series instead of channels -- the
// reference's float64 channel sum regrouped, within the float32 parity bar
// (and exact for integer-valued data).
template <typename InT>
struct FxFromInput {
  static constexpr bool kF32 = std::is_same<InT, float>::value;
  using El = typename std::conditional<kF32, ElemF32, ElemU16>::type;
  using V = typename El::value_t;
  static constexpr int kBlock = kF32 ? kFxEf : kFxE;
  // non-temporal: the pattern image is read back only after the whole
  // stage (12.6 against 13.0 ms per configs[3] launch, same box; the
  // float32 stage 1 measured 8.6 ms with it against 7.5 without, on
  // another box, so it keeps plain stores)
  static constexpr bool kNontemporal = !kF32;
  const SrcRows<InT> src;
  const FxS1Args& a;
  __device__ __forceinline__ explicit FxFromInput(const FxS1Args& a_) : src(a_.x, a_.lay), a(a_) {}
  __device__ __forceinline__ void load_row(typename El::elem_t* L, int c, int64_t i0, int W) const {
    const V pv = pad_value<V>(a.pad_mode, a.padvals, c);
    // a block whose rows lie inside [0, nR) and whose samples inside [0, N)
    // (every block but the segment's edges) loads without per-sample tests
    const int64_t s_lo = a.base + i0, s_hi = s_lo + W - 1 + (El::S - 1) * a.Qs;
    const bool inner = i0 >= 0 && i0 + W <= a.nR && s_lo >= 0 && s_hi < a.N;
    if (inner) {
      for (int e = threadIdx.x; e < W; e += 256) {
        V v[El::S];
#pragma unroll
        for (int m = 0; m < El::S; ++m) v[m] = (V)src.at(c, s_lo + e + m * a.Qs);
        L[e] = El::pack(v);
      }
      return;
    }
    for (int e = threadIdx.x; e < W; e += 256) {
      const int64_t i = i0 + e;
      V v[El::S];
#pragma unroll
      for (int m = 0; m < El::S; ++m) {
        const int64_t sm = a.base + i + m * a.Qs;
        v[m] = (i < 0 || i >= a.nR) ? (V)0 : padded_sample<V>(src, c, sm, a.N, a.pad_mode, pv);
      }
      L[e] = El::pack(v);
    }
  }
  // the same element by element (the persistent kernel's prefetch).  inner:
  // rows [i0, i0 + W) and their samples, widened by `slack` samples, need no test
  __device__ __forceinline__ bool inner(int64_t i0, int W, int slack = 0) const {
    const int64_t s_lo = a.base + i0, s_hi = s_lo + W - 1 + (El::S - 1) * a.Qs;
    return i0 >= 0 && i0 + W <= a.nR && s_lo - slack >= 0 && s_hi + slack < a.N;
  }
  __device__ __forceinline__ typename El::elem_t elem(int c, int64_t i, bool in) const {
    V v[El::S];
    if (in) {
#pragma unroll
      for (int m = 0; m < El::S; ++m) v[m] = (V)src.at(c, a.base + i + m * a.Qs);
    } else {
      const V pv = pad_value<V>(a.pad_mode, a.padvals, c);
#pragma unroll
      for (int m = 0; m < El::S; ++m)
        v[m] = (i < 0 || i >= a.nR) ? (V)0
                                     : padded_sample<V>(src, c, a.base + i + m * a.Qs, a.N, a.pad_mode, pv);
    }
    return El::pack(v);
  }
};

// Stage 1 through LDS: load the group's FXG rows (Src), then write every
// pattern of the group from them: pattern element j = the sum of the rows'
// elements at j + r_k, in channel order ((a + b) + c) + d.
// The pattern loop: L holds the group's FXG rows, W = kBlock + hi - lo
// elements each from element j0 + lo on; B0 = the group's first descriptor
// batch (fx_batch at p0), loaded by the caller.
template <typename Src, int FXG>
__device__ __forceinline__ void fx_write_patterns(const FxS1Args& a, const typename Src::El::elem_t* L,
                                                  int64_t j0, int p0, int p1, int lo, int W,
                                                  const FxBatch& B0) {
  using El = typename Src::El;
  using E = typename El::elem_t;
  constexpr int kE = Src::kBlock;
  const int4* __restrict__ pat = a.pat;
  E* __restrict__ P = static_cast<E*>(a.R);
  const int64_t nR = a.nR;
  const int* rng = a.gtab + 3 * a.NG + 1;
  for (int pb = p0; pb < p1; pb += 64) {
    const FxBatch B = pb == p0 ? B0 : fx_batch(pat, rng, pb, p1);
    for (int i = 0; i < min(64, p1 - pb); ++i) {
      const int p = pb + i;
      const int4 q = make_int4(0, __builtin_amdgcn_readlane(B.y, i), __builtin_amdgcn_readlane(B.z, i),
                               __builtin_amdgcn_readlane(B.w, i));
      const int64_t jlo = __builtin_amdgcn_readlane(B.lo, i), jhi = nR + __builtin_amdgcn_readlane(B.hi, i);
      if (j0 >= jhi || j0 + kE <= jlo) continue;  // no trial of p reads this block
#pragma unroll
      for (int e = threadIdx.x; e < kE; e += 256) {
        const int64_t j = j0 + e;
        if (j >= nR) break;  // (a block's elements outside [jlo, jhi): written, unread)
        E s = El::add(L[e - lo], L[W + e - lo + q.y]);
        if constexpr (FXG > 2) {
          s = El::add(s, L[2 * W + e - lo + q.z]);
          s = El::add(s, L[3 * W + e - lo + q.w]);
        }
        E* dst = P + (int64_t)p * nR + j;
        if constexpr (Src::kNontemporal) {
          typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));
          const u32x4v sv = {s.x, s.y, s.z, s.w};
          __builtin_nontemporal_store(sv, reinterpret_cast<u32x4v*>(dst));
        } else {
          *dst = s;
        }
      }
    }
  }
}

// One workgroup per (group, element block): the rows, a barrier, the
// patterns.  The form for grids of less than one wave of persistent
// workgroups (and the persistent kernel's A/B partner, -DPDD_FX_S1_ONESHOT).
template <typename Src, int FXG>
__global__ __launch_bounds__(256) void k_fx_stage1(const FxS1Args a) {
  using E = typename Src::El::elem_t;
  constexpr int kE = Src::kBlock;
  extern __shared__ __attribute__((aligned(16))) unsigned char fx_smem[];
  E* L = reinterpret_cast<E*>(fx_smem);
  const int* __restrict__ gtab = a.gtab;
  const int NG = a.NG;
  const int g = blockIdx.x;
  const int64_t j0 = (int64_t)blockIdx.y * kE;
  const int p0 = gtab[g], p1 = gtab[g + 1];
  const int lo = gtab[NG + 1 + 2 * g], hi = gtab[NG + 2 + 2 * g];
  const int W = kE + hi - lo;
  const Src src(a);
  for (int k = 0; k < FXG; ++k) src.load_row(L + k * W, g * FXG + k, j0 + lo, W);
  __syncthreads();
  if (p1 > p0)
    fx_write_patterns<Src, FXG>(a, L, j0, p0, p1, lo, W,
                                fx_batch(a.pat, gtab + 3 * NG + 1, p0, p1));
}

// The persistent form: a grid of (resident workgroups per CU) x (CUs)
// workgroups takes (group, element block) ITEMS in the order of fx_walk.h
// (group fastest) from one queue per XCD -- queue x holds items x, x + 8, ...;
// a workgroup drains the queue of its own XCD first, then the others' -- and
// holds item i + 1's rows in registers (issued before item i's pattern loop,
// written to LDS after the barrier that ends it), so the input loads run
// under the pattern stores.  What a thread holds for the next item:
// FxPreElems, packed elements (FXG x ceil(W / 256) <= 3 or 5; float32 and image
// elements are the loaded words themselves) ...
template <typename Src, int FXG>
struct FxPreElems {
  using E = typename Src::El::elem_t;
  // (rows wider than kWmax elements -- relative shifts spanning more than 256
  // -- are not prefetched: they load at commit, the way the one-item kernel does)
  static constexpr int kWmax = Src::kBlock + 256;
  static constexpr int kPer = (kWmax + 255) / 256;
  E r[FXG][kPer];
  __device__ __forceinline__ void fetch(const Src& src, int c0, int64_t i0, int W) {
    if (W > kWmax) return;
    const bool in = src.inner(i0, W);
#pragma unroll
    for (int k = 0; k < FXG; ++k)
#pragma unroll
      for (int n = 0; n < kPer; ++n) {
        const int e = threadIdx.x + n * 256;
        if (e < W) r[k][n] = src.elem(c0 + k, i0 + e, in);
      }
  }
  __device__ __forceinline__ void commit(const Src& src, E* L, int c0, int64_t i0, int W) const {
    if (W > kWmax) {
      for (int k = 0; k < FXG; ++k) src.load_row(L + k * W, c0 + k, i0, W);
      return;
    }
#pragma unroll
    for (int k = 0; k < FXG; ++k)
#pragma unroll
      for (int n = 0; n < kPer; ++n) {
        const int e = threadIdx.x + n * 256;
        if (e < W) L[k * W + e] = r[k][n];
      }
  }
};
// ... or, for 8-bit input on interior blocks of aligned input (FxS1Args.words),
// raw words, unpacked into the u16 eighths only on the way to LDS: mode 1 (rows:
// channel-major or pieces) = the 4 consecutive samples of one row, one dword
// per eighth, so a thread's unit is 4 consecutive elements of a row (the
// window is widened to dword boundaries: up to 3 samples read on either
// side, hence the slack of `inner`, are dropped); mode 2 (time-major) = the
// group's FXG channels of one spectrum, one FXG-byte word per eighth, so a
// unit is one element of all FXG rows.  Mode 0: edge blocks and unaligned
// input load their rows at commit the way the one-item kernel does.
template <int FXG>
struct FxPreWords {
  using Src = FxFromInput<uint8_t>;
  // (rows wider than kWmax elements -- relative shifts spanning more than 256
  // -- are not prefetched: 4 units per thread cover FXG x (kWmax / 4 + 1))
  static constexpr int kWmax = kFxE + 256;
  static constexpr int kUnits = FXG * ((kWmax + 3) / 4 + 1) > kWmax ? FXG * ((kWmax + 3) / 4 + 1) : kWmax;
  static constexpr int kU = (kUnits + 255) / 256;
  uint32_t d[kU][8];
  int mode, sh, nq;
  __device__ __forceinline__ void fetch(const Src& src, int c0, int64_t i0, int W) {
    const FxS1Args& a = src.a;
    const uint8_t* __restrict__ x = src.src.x;
    const int64_t s0 = a.base + i0;
    mode = 0;
    if (!a.words || W > kWmax) return;
    if (a.lay.ld_t) {
      if (!src.inner(i0, W)) return;
      mode = 2;
#pragma unroll
      for (int n = 0; n < kU; ++n) {
        const int e = threadIdx.x + n * 256;
        if (e < W) {
#pragma unroll
          for (int m = 0; m < 8; ++m) {
            const uint8_t* q = x + (s0 + e + m * a.Qs) * a.lay.ld_t + c0;
            if constexpr (FXG == 4) d[n][m] = *reinterpret_cast<const uint32_t*>(q);
            else d[n][m] = *reinterpret_cast<const uint16_t*>(q);
          }
        }
        // (one unit's 8 addresses at a time: scheduling all units' loads
        // together spills registers at 4 waves per SIMD)
        __builtin_amdgcn_sched_barrier(0);
      }
      return;
    }
    if (!src.inner(i0, W, 3)) return;
    mode = 1;
    sh = (int)(s0 & 3);
    nq = (W + sh + 3) >> 2;
    if (a.lay.piece) fetch_rows<true>(a, x, c0, s0 - sh);
    else fetch_rows<false>(a, x, c0, s0 - sh);
  }
  template <bool PIECES>
  __device__ __forceinline__ void fetch_rows(const FxS1Args& a, const uint8_t* __restrict__ x, int c0,
                                             int64_t sa) {
#pragma unroll
    for (int n = 0; n < kU; ++n) {
      const int f = threadIdx.x + n * 256;
      if (f < FXG * nq) {
        const int k = f / nq, q = f - k * nq;
        const int64_t s = sa + 4 * q;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          const int64_t sm = s + m * a.Qs;
          const int64_t o = PIECES ? (sm >> a.lay.psh) * a.lay.pstride + (int64_t)(c0 + k) * a.lay.piece +
                                         (sm & (a.lay.piece - 1))
                                   : (int64_t)(c0 + k) * a.lay.ld + sm;
          d[n][m] = *reinterpret_cast<const uint32_t*>(x + o);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  __device__ __forceinline__ void commit(const Src& src, uint4* L, int c0, int64_t i0, int W) const {
    if (mode == 0) {
      for (int k = 0; k < FXG; ++k) src.load_row(L + k * W, c0 + k, i0, W);
      return;
    }
    if (mode == 2) {
#pragma unroll
      for (int n = 0; n < kU; ++n) {
        const int e = threadIdx.x + n * 256;
        if (e < W) {
#pragma unroll
          for (int k = 0; k < FXG; ++k) {
            uint32_t v[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) v[m] = (d[n][m] >> (8 * k)) & 0xffu;
            L[k * W + e] = ElemU16::pack(v);
          }
        }
      }
      return;
    }
#pragma unroll
    for (int n = 0; n < kU; ++n) {
      const int f = threadIdx.x + n * 256;
      if (f < FXG * nq) {
        const int k = f / nq, q = f - k * nq;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int e = 4 * q - sh + j;
          uint32_t v[8];
#pragma unroll
          for (int m = 0; m < 8; ++m) v[m] = (d[n][m] >> (8 * j)) & 0xffu;
          if (e >= 0 && e < W) L[k * W + e] = ElemU16::pack(v);
        }
      }
    }
  }
};

// An item's geometry from the group table.
struct FxItem {
  int g, p0, p1, lo, W;
  int64_t j0;
};
template <int kE>
__device__ __forceinline__ FxItem fx_item(const FxS1Args& a, int i) {
  const FxWalkItem w = fx_walk_item(i, a.NG);
  const int* __restrict__ gtab = a.gtab;
  const int g = w.group;
  const int lo = gtab[a.NG + 1 + 2 * g], hi = gtab[a.NG + 2 + 2 * g];
  return {g, gtab[g], gtab[g + 1], lo, kE + hi - lo, w.block * kE};
}
// The next item of queue `xcd` from its ticket (the queue counter's value
// before this workgroup's increment), or of the next queue that has one; -1:
// none left.  (Counters stay far below 2^32: n_items < 2^31 - 16 x grid.)
__device__ __forceinline__ int fx_take(unsigned int* queue, int xcd, unsigned int ticket, int n_items) {
  for (int t = 0;; ++t) {
    const int64_t i = (int64_t)ticket * kFxXcds + xcd;
    if (i < n_items) return (int)i;
    if (t == kFxXcds - 1) return -1;
    xcd = (xcd + 1) % kFxXcds;
    ticket = atomicAdd(queue + xcd, 1u);
  }
}

// (The u16-eighths instances keep the register budget of 4 waves per SIMD --
// 4 workgroups per CU, what their LDS allows at rspan <= 128; the float32
// rows of 1024 elements leave room for 2.)
template <typename Src, int FXG>
__global__ __launch_bounds__(256, Src::kBlock == kFxE ? 4 : 2) void k_fx_stage1_p(const FxS1Args a) {
  using E = typename Src::El::elem_t;
  using Pre = typename std::conditional<std::is_same<Src, FxFromInput<uint8_t>>::value, FxPreWords<FXG>,
                                        FxPreElems<Src, FXG>>::type;
  constexpr int kE = Src::kBlock;
  extern __shared__ __attribute__((aligned(16))) unsigned char fx_smem[];
  E* L = reinterpret_cast<E*>(fx_smem);
  // (item numbers pass from thread 0 to the workgroup through two words
  // behind the rows)
  int* slot = reinterpret_cast<int*>(fx_smem + a.slot);
  const int n_items = (int)a.n_items;
  const int xcd = fx_walk_xcd(blockIdx.x);
  if (threadIdx.x == 0) {
    slot[0] = fx_take(a.queue, xcd, atomicAdd(a.queue + xcd, 1u), n_items);
    slot[1] = fx_take(a.queue, xcd, atomicAdd(a.queue + xcd, 1u), n_items);
  }
  __syncthreads();
  const int first = __builtin_amdgcn_readfirstlane(slot[0]);
  int nx = __builtin_amdgcn_readfirstlane(slot[1]);
  if (first < 0) return;
  const Src src(a);
  Pre pre;
  // (the descriptor loads of an item's first 64 patterns travel with its
  // rows: a load issued inside the pattern loop would wait for the prefetch)
  const int* rng = a.gtab + 3 * a.NG + 1;
  FxItem cur = fx_item<kE>(a, first);
  FxBatch Bc = {0, 0, 0, 0, 0};
  if (cur.p1 > cur.p0) Bc = fx_batch(a.pat, rng, cur.p0, cur.p1);
  pre.fetch(src, cur.g * FXG, cur.j0 + cur.lo, cur.W);
  pre.commit(src, L, cur.g * FXG, cur.j0 + cur.lo, cur.W);
  for (;;) {
    __syncthreads();  // item cur's rows are in LDS; every thread has read the slot
    FxItem nxt = cur;
    FxBatch Bn = Bc;
    if (nx >= 0) {
      nxt = fx_item<kE>(a, nx);
      if (nxt.p1 > nxt.p0) Bn = fx_batch(a.pat, rng, nxt.p0, nxt.p1);
      pre.fetch(src, nxt.g * FXG, nxt.j0 + nxt.lo, nxt.W);
    }
    fx_write_patterns<Src, FXG>(a, L, cur.j0, cur.p0, cur.p1, cur.lo, cur.W, Bc);
    if (nx < 0) break;
    // the item after next.  (Taken here, not before the pattern loop: the
    // compiler waits for an atomic's result where it is issued, and with it
    // for the prefetch loads in flight.)
    if (threadIdx.x == 0) slot[0] = fx_take(a.queue, xcd, atomicAdd(a.queue + xcd, 1u), n_items);
    __syncthreads();  // every thread has read item cur's rows
    const int nn = __builtin_amdgcn_readfirstlane(slot[0]);
    pre.commit(src, L, nxt.g * FXG, nxt.j0 + nxt.lo, nxt.W);
    cur = nxt;
    Bc = Bn;
    nx = nn;
  }
}

// Every LDS stage-1 instance (groups of 2 or 4: fx_build makes no others):
// (source, group size) -> kernels.  src: the plan's dtype when stage 1 reads
// the input, kFxImage when it reads a pre-pass image.
typedef void (*fx_s1_fn)(FxS1Args);
constexpr int kFxImage = -1;
struct FxS1Instance {
  int src, fx;
  fx_s1_fn fn, fn_p;  // one item per workgroup / persistent
  int block;          // elements per item (the source's kBlock)
};
#define PDD_FX_S1(SRC_, ...)                                                              \
  {SRC_, 2, k_fx_stage1<__VA_ARGS__, 2>, k_fx_stage1_p<__VA_ARGS__, 2>, __VA_ARGS__::kBlock}, \
  {SRC_, 4, k_fx_stage1<__VA_ARGS__, 4>, k_fx_stage1_p<__VA_ARGS__, 4>, __VA_ARGS__::kBlock}
static const FxS1Instance kFxS1Instances[] = {
    PDD_FX_S1(kFxImage, FxFromImage), PDD_FX_S1(PDD_U8, FxFromInput<uint8_t>),
    PDD_FX_S1(PDD_U16, FxFromInput<uint16_t>), PDD_FX_S1(PDD_F32, FxFromInput<float>)};
#undef PDD_FX_S1

// A whole window from ONE wave: runs of up to four consecutive 1 KiB DMAs
// share one M0 value, the instruction offset (0 / 1024 / 2048 / 3072 bytes)
// moving both the global source and the LDS destination
// (scripts/probes/dma_offset.hip checks the LDS side on the device).
__device__ __forceinline__ int stage_il_dma_win(uint32_t lds_dst, const float4* src, int ne,
                                                int lane) {
  const int nq = (ne + 63) >> 6;
  uint32_t keep;
#define PDD_DMA_RUN(TEXT)                                                                      \
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t" TEXT "s_mov_b32 m0, %0" \
               : "=&s"(keep) : "v"(s), "s"(m) : "memory")
  for (int q = 0; q < nq; q += 4) {
    const float4* s = src + q * 64 + lane;
    const uint32_t m = __builtin_amdgcn_readfirstlane(lds_dst + q * 1024);
    switch (min(4, nq - q)) {
      case 1: PDD_DMA_RUN("global_load_lds_dwordx4 %1, off\n\t"); break;
      case 2: PDD_DMA_RUN("global_load_lds_dwordx4 %1, off\n\t"
                          "global_load_lds_dwordx4 %1, off offset:1024\n\t"); break;
      case 3: PDD_DMA_RUN("global_load_lds_dwordx4 %1, off\n\t"
                          "global_load_lds_dwordx4 %1, off offset:1024\n\t"
                          "global_load_lds_dwordx4 %1, off offset:2048\n\t"); break;
      default: PDD_DMA_RUN("global_load_lds_dwordx4 %1, off\n\t"
                           "global_load_lds_dwordx4 %1, off offset:1024\n\t"
                           "global_load_lds_dwordx4 %1, off offset:2048\n\t"
                           "global_load_lds_dwordx4 %1, off offset:3072\n\t"); break;
#undef PDD_DMA_RUN
    }
  }
  return nq;
}

// A factorised window of nq pieces from a wave-uniform source address in an
// SGPR pair (the saddr form; the lanes' VGPR offset is lane * 16 for every
// DMA: no VALU address arithmetic), as ONE asm block per run of up to four:
// M0 set once, then the pieces with instruction offsets, each after the
// first behind an s_cmp / s_cbranch on the remaining count (a compiler switch
// over min(4, nq - q) became a tree of ~20 scalar instructions and four
// branches per run).  Returns the DMAs issued.
__device__ __forceinline__ int stage_il_dma_s2(uint32_t lds_dst, const float4* src, int nq,
                                               uint32_t voff) {
  for (int q = 0; q < nq; q += 4) {
    const float4* s = src + q * 64;
    const uint32_t m = __builtin_amdgcn_readfirstlane(lds_dst + q * 1024);
    const int left = __builtin_amdgcn_readfirstlane(nq - q);
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2\n\t"
        "s_cmp_lt_i32 %4, 2\n\t"
        "s_cbranch_scc1 1f\n\t"
        "global_load_lds_dwordx4 %1, %2 offset:1024\n\t"
        "s_cmp_lt_i32 %4, 3\n\t"
        "s_cbranch_scc1 1f\n\t"
        "global_load_lds_dwordx4 %1, %2 offset:2048\n\t"
        "s_cmp_lt_i32 %4, 4\n\t"
        "s_cbranch_scc1 1f\n\t"
        "global_load_lds_dwordx4 %1, %2 offset:3072\n"
        "1:\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(s), "s"(m), "s"(left)
        : "memory", "scc");
  }
  return nq;
}

// The last rem (< 64) elements of a window: one DMA piece from a
// wave-uniform source with lanes >= rem masked off, so nothing lands past
// the window's end in LDS.  Returns the DMAs issued (1).
__device__ __forceinline__ int stage_il_dma_tail(uint32_t lds_dst, const float4* src, int rem,
                                                 uint32_t voff, int lane) {
  if (lane < rem) {
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(src), "s"(lds_dst)
        : "memory");
  }
  return 1;
}


// Synchronisation of k_sweep_il: one s_barrier per chunk.  Before barrier k
// the loader waves retire chunk k's DMAs with a counted vmcnt (chunks k+1 ..
// k+NBUF-2 stay in flight); after it they refill the buffer chunk k-1 used.
// (Measured and dropped, DESIGN.md §3: an LDS-counter hand-off without
// barriers; the compute waves reading their shifts by scalar loads.)
// Metadata: mt[dblk][c][ROW], ROW = DB + 4: the tile's DB shifts at channel c
// relative to their minimum bmin, as byte offsets into the channel's LDS
// image (16 x elements), then {bmin, span, 0, 0} (in elements).  Loader 0 DMAs
// the rows of chunk j into ONE shared ring (slot j % MR) MA = 2(NBUF-1)
// chunks ahead, before the samples of chunk j - MA + NBUF - 1; its counted
// vmcnt before barrier k therefore also retires the rows of chunk
// k + NBUF - 1, which every loader reads after barrier k to issue that
// chunk's samples, and the compute waves read the shifts of chunk k after
// the same barrier.  (il_ma, il_mr, il_slot, il_meta_bytes: sweep_plan.h, shared
// with the planner.)

// Tile order of k_sweep_il.  Blocks b and b+8 share an XCD (and its L2).
// XCD x walks its time tiles in bands of GT time tiles, each band in 2-D
// groups of GT time tiles x GJ trial blocks: at one channel the concurrent
// windows of such a group overlap along both axes (a trial block's window
// extends its neighbour's by the span, a time tile's by Tq), so the group
// re-reads each staged element ~GT*GJ*(Tq+S)/(GT*Tq + GJ*S) times from L2.
// Channel sweeps: XCD x owns the time tiles [x*TX, (x+1)*TX), TX = n_tblk / 8
// (8 x 4 groups).  Factorised sweeps (XI): band b of XCD x is global band
// 8b + x, so the eight XCDs sweep eight ADJACENT bands with the same
// trial-block groups at the same time and the windows two neighbouring bands
// share are fetched from HBM once, into the Infinity Cache (8 x 2 groups
// since the chunk packing orders each trial block's groups by its own
// windows, so that neighbouring trial blocks no longer stage the same
// group at the same time: configs[3] 94.23 -> 93.03 ms per launch, north
// star 61.34 -> 59.20 ms, L2-side fetch 478 -> 412 GB).  Leftover time tiles (n_tblk % 8) follow in natural order.
#ifndef PDD_IL_GT
#define PDD_IL_GT 8
#endif
#ifndef PDD_IL_GJ
#define PDD_IL_GJ 4
#endif
#ifndef PDD_FX_GT
#define PDD_FX_GT 8
#endif
// (PDD_FX_GJ = 2: sweep_plan.h, the planner pairs the trial blocks by it)
// float32 factorised tiles: 8 x 1 groups (their plans do not pair trial
// blocks: configs[1] f32 stage 2 23.45-23.53 -> 22.95-23.01 ms against 8 x 2)
#ifndef PDD_FX_GJF
#define PDD_FX_GJF 1
#endif
template <int GT = PDD_IL_GT, int GJ = PDD_IL_GJ, bool XI = false>
__device__ __forceinline__ void il_tile_of(int bid, int n_tblk, int n_dblk, int& dblk, int& tblk) {
  const int TX = n_tblk / 8;
  const int owned = 8 * TX * n_dblk;
  if (bid >= owned) {
    const int L = bid - owned;
    dblk = L % n_dblk;
    tblk = 8 * TX + L / n_dblk;
    return;
  }
  const int x = bid % 8, k = bid / 8;  // k-th tile of XCD x
  const int band = k / (GT * n_dblk);
  const int gtb = min(GT, TX - band * GT);  // time tiles in this band
  int r = k - band * GT * n_dblk;
  const int nj = (n_dblk + GJ - 1) / GJ;
  const int jg = min(r / (gtb * GJ), nj - 1);
  const int gj = min(GJ, n_dblk - jg * GJ);  // trial blocks in this group
  r -= jg * gtb * GJ;
  dblk = jg * GJ + r % gj;
  if constexpr (XI) {
    const int nb = (TX + GT - 1) / GT;
    tblk = (band < nb - 1 ? (band * 8 + x) * GT : 8 * (nb - 1) * GT + x * gtb) + r / gj;
  } else {
    tblk = x * TX + band * GT + r / gj;
  }
}

// Eight consecutive metadata rows' window fields {bmin, span, offset,
// source row} (row stride ROW ints) by eight scalar loads and one wait
// (the sweep's loader waves; they read no LDS).  The plan pads the table so
// eight rows from any chunk start are inside the allocation.
typedef int i32x4s_t __attribute__((ext_vector_type(4)));
struct il_rows8 {
  i32x4s_t r0, r1, r2, r3, r4, r5, r6, r7;
};
template <int ROW>
__device__ __forceinline__ il_rows8 il_load_rows8(const int* p) {
  il_rows8 o;
  asm volatile(
      "s_load_dwordx4 %0, %8, %9\n\ts_load_dwordx4 %1, %8, %10\n\t"
      "s_load_dwordx4 %2, %8, %11\n\ts_load_dwordx4 %3, %8, %12\n\t"
      "s_load_dwordx4 %4, %8, %13\n\ts_load_dwordx4 %5, %8, %14\n\t"
      "s_load_dwordx4 %6, %8, %15\n\ts_load_dwordx4 %7, %8, %16\n\t"
      "s_waitcnt lgkmcnt(0)"
      // early-clobber outputs: a row's registers must not overlap the base
      // address the later loads of the block still read (a load returning
      // before the next one issues would change its address)
      : "=&s"(o.r0), "=&s"(o.r1), "=&s"(o.r2), "=&s"(o.r3), "=&s"(o.r4), "=&s"(o.r5),
        "=&s"(o.r6), "=&s"(o.r7)
      : "s"(p), "i"(0), "i"(ROW * 4), "i"(2 * ROW * 4), "i"(3 * ROW * 4), "i"(4 * ROW * 4),
        "i"(5 * ROW * 4), "i"(6 * ROW * 4), "i"(7 * ROW * 4));
  return o;
}

// a + b + c: one v_add3_u32 (two packed-u16 sample adds per lane)
__device__ __forceinline__ uint32_t add3_u32(uint32_t a, uint32_t b, uint32_t c) {
  return a + b + c;
}

// Factorised sweeps (FX): the kernel's "channels" are the channel groups;
// a chunk's windows (one per pattern its trials use) come from the plan's
// window records wt[dblk][chunk][kFxWin] = {bmin, length, buffer offset,
// pattern row | window count << 20}, one vector load per loader lane, two
// chunks ahead.
template <int G, int DPW, int NCW, int NLW, int CC, int NBUF, bool U16 = false, bool FX = false>
__global__ __launch_bounds__((NCW + NLW) * 64) void k_sweep_il(
    const float4* __restrict__ R0, int64_t nR, int C, int lo, const int* __restrict__ mt,
    const int* __restrict__ cht, int maxch, float* __restrict__ out, int64_t ld_out, int D,
    int64_t Qs, int64_t t_base, int64_t n_out, int buf_e, int n_tblk, int n_dblk, int dbg,
    int64_t row_g, int64_t row_d, int flush_n, float out_bias, const float* __restrict__ r2_pad,
    int64_t r2_nR, int64_t r2_ov, const int4* __restrict__ wt, const int* __restrict__ sig) {
  // Grouped sweeps: C is the channel count of ONE group; blockIdx.x / (tiles
  // per group) is the group, whose channels are R rows [grp*C, grp*C + C),
  // whose tables are mt[grp][...], and whose trial d lands in plane row
  // grp*row_g + d*row_d (ungrouped: 0, 0, 1).
  constexpr int Tq = 64 * G;
  constexpr int DB = NCW * DPW;
  constexpr int ROW = DB + 4;
  constexpr int SLOT = il_slot(CC, DB);
  constexpr int MA = il_ma(NBUF), MR = il_mr(NBUF);
  static_assert(ROW % 4 == 0, "metadata rows land as 16-byte quads");
  constexpr int S = U16 ? 8 : 4;  // samples per 16-byte element (quarters / eighths)
  static_assert((U16 ? (DPW >= 4 && DPW <= 8) : DPW == 4) && G == (U16 ? 2 : 4) &&
                    DPW * CC <= 64 && CC % 2 == 0,
                "4 (f32) or 4..8 (u16) trials per wave, 4 (f32) or 2 (u16) groups; one lane "
                "per (channel, trial)");
  static_assert(NBUF >= 2 && MA >= 2 * NBUF - 2 && MR > MA, "ring geometry");
  extern __shared__ __attribute__((aligned(16))) float smf[];
  uint4* img = reinterpret_cast<uint4*>(smf);
  int* metar = reinterpret_cast<int*>(img + NBUF * buf_e);  // [MR][SLOT]

  const int per_grp = n_tblk * n_dblk;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  // developer builds only (PDD_SWEEP_DEBUG bit 2): per-wave cycle stamps
  // written into `out` instead of the plane
  const bool stamps = (dbg & 4) != 0;

  // One tile per workgroup.  (A persistent grid -- 256 workgroups walking
  // their XCD's tiles -- measured no faster for the channel sweep: the L2 hit
  // rate of the staging fell from 77% to 48% at unchanged kernel time.)
  int dblk, tblk;
  const int grp = blockIdx.x / per_grp;
  il_tile_of<FX ? PDD_FX_GT : PDD_IL_GT, FX ? (U16 ? PDD_FX_GJ : PDD_FX_GJF) : PDD_IL_GJ, FX>(
      blockIdx.x - grp * per_grp, n_tblk, n_dblk, dblk, tblk);
  const float4* R = R0 + (int64_t)grp * C * nR;
  const int64_t t0 = (int64_t)tblk * Tq;
  const int* mt_b = mt + ((int64_t)grp * n_dblk + dblk) * (C + 1) * ROW;
  const int* cht_t = cht + ((int64_t)grp * n_dblk + dblk) * (maxch + 1);
  const int nchunk = cht_t[0];
  const uint32_t img_lds = lds_addr_of(img);
  const uint32_t voff16 = (uint32_t)lane * 16u;
  // FX tiles: the chunk's window records (lane i = window i, one vector load)
  const int4* wt_b = FX ? wt + ((int64_t)grp * n_dblk + dblk) * maxch * kFxWin : nullptr;
  auto fx_rec = [&](int k) -> int4 {
    if constexpr (FX) return wt_b[(int64_t)min(k, nchunk - 1) * kFxWin + lane];
    else return make_int4(0, 0, 0, 0);
  };
  // one loader's share of chunk k's window DMAs (windows first, first +
  // step, ...): lane i computes window i's source, LDS address and piece
  // count once, then the loader issues its own windows from SGPRs.
  // (Measured and dropped: every wave of the workgroup issuing a share of
  // the DMAs -- configs[3] 101.6 -> 116.4 ms per launch.)
  auto fx_issue = [&](int k, const int4& rec, int first, int step) -> int {
    // the compiler's wait for the record (vmcnt(0): it cannot see the DMAs)
    // lands here, before any DMA of this chunk
    asm volatile("" ::"v"(rec.x), "v"(rec.y), "v"(rec.z), "v"(rec.w));
    const int b = k % NBUF;
    const int nw = __builtin_amdgcn_readlane(rec.w, 0) >> 20;
    const uint64_t sv = (uint64_t)(R + (int64_t)(rec.w & 0xfffff) * nR + (t0 + rec.x - lo));
    const uint32_t dv = img_lds + (uint32_t)((b * buf_e + rec.z) * 16);
    // whole 64-element pieces, then the window's last rv < 64 elements as
    // one piece under an EXEC mask: windows sit back to back in the buffer.
    // (Every window in whole pieces, round 4's layout: configs[3] stage 2
    // 99.25 against 95.36 ms per launch, north star 69.17 against 64.94.)
    const int qv = rec.y >> 6;
    const int rv = rec.y & 63;
    int n = 0;
    for (int i = first; i < nw; i += step) {
      const uint32_t lo32 = __builtin_amdgcn_readlane((uint32_t)sv, i);
      const uint32_t hi32 = __builtin_amdgcn_readlane((uint32_t)(sv >> 32), i);
      const float4* src = (const float4*)(((uint64_t)hi32 << 32) | lo32);
      const uint32_t dst = __builtin_amdgcn_readlane(dv, i);
      const int nq = __builtin_amdgcn_readlane(qv, i);
      n += stage_il_dma_s2(dst, src, nq, voff16);
      const int rem = __builtin_amdgcn_readlane(rv, i);
      if (rem) n += stage_il_dma_tail(dst + (uint32_t)nq * 1024u, src + nq * 64, rem, voff16, lane);
    }
    return n;
  };
  if (w >= NCW) {
    // ---------------- loader waves: metadata rows + sample windows
    // Top issue priority: a loader shares its SIMD with compute waves that
    // have an LDS read or add ready every cycle.
    __builtin_amdgcn_s_setprio(3);
    const int lw = w - NCW;
    int* ring = metar;  // the shared ring (loader 0 fills it)
    // (Measured and dropped, round 5: windows to the loaders in reverse
    // order, so that loader 0, which also issues the metadata rows, takes the
    // fewest -- configs[3] 97.2 / north star 81.7 ms per launch either way.)
    // chunk k = channels c0 .. c0 + ncc - 1 (cht: c0 | ncc << 20), packed
    // into its buffer at the per-channel offsets of the metadata rows
    // (loader 0 reads chunk k + MA's table entry one iteration ahead: a
    // scalar load's latency is not on the loaders' per-chunk path)
    int e_next = (lw == 0 && MA < nchunk) ? cht_t[1 + MA] : 0;
    auto issue_meta = [&](int k) -> int {
      if (k >= nchunk || lw != 0) return 0;
      const int e = k < MA ? cht_t[1 + k] : e_next;
      if (k >= MA && k + 1 < nchunk) e_next = cht_t[2 + k];
      const int n_int = (e >> 20) * ROW;
      int n = 0;
      // 1 KiB per DMA: a chunk's rows in ceil(n_int / 256) instructions (the
      // metadata DMAs of a 96-trial chunk: 4 instead of 13 dword DMAs;
      // configs[3] stage 2 103.1 -> 102.2 ms per launch)
#pragma unroll
      for (int m = 0; m < (SLOT + 255) / 256; ++m) {
        if (m * 256 >= n_int) break;
        dma_ints4(ring + (k % MR) * SLOT + m * 256, mt_b + (int64_t)(e & 0xfffff) * ROW + m * 256,
                  n_int - m * 256, lane);
        ++n;
      }
      return n;
    };
    // FX: the records are loaded two chunks ahead; the load issued after a
    // chunk's DMAs (and the metadata DMAs) is the wave's youngest vector-memory
    // operation, so the counted wait before the next barrier leaves it in
    // flight and its latency is off the per-chunk path
    int4 rec_next = fx_rec(0);
    int4 rec_next2 = fx_rec(1);
    int rec_tail = 0;  // a record load issued after the last chunk's DMAs
    auto issue_samples = [&](int k) -> int {
      if constexpr (FX) {
        const int4 rec = rec_next;
        rec_next = rec_next2;  // (chunk k + 2's record: rec_ahead)
        return fx_issue(k, rec, lw, NLW);
      }
      const int b = k % NBUF;
      // the chunk's window rows {bmin, span, offset, source row} by scalar
      // loads from the global table, all eight issued before one wait: the
      // loaders read no LDS.  (They used to read these fields from the
      // metadata ring, 4 LDS reads per channel queued behind the compute
      // waves' read stream: configs[3] u8 260.1 -> 239.0 ms per launch.)
      static_assert(CC <= 8, "at most eight rows per chunk");
      const int e = cht_t[1 + k];
      const int ncc = e >> 20;
      const il_rows8 r8 = il_load_rows8<ROW>(mt_b + (int64_t)(e & 0xfffff) * ROW + DB);
      const i32x4s_t rr[8] = {r8.r0, r8.r1, r8.r2, r8.r3, r8.r4, r8.r5, r8.r6, r8.r7};
      int n = 0;
#pragma unroll
      for (int i = 0; i < CC; ++i) {
        if (i >= ncc) break;
        // window i from loader i mod NLW, its DMAs in runs sharing M0
        if (i % NLW == lw)
          n += stage_il_dma_win(img_lds + (uint32_t)((b * buf_e + rr[i].z) * 16),
                                R + (int64_t)(rr[i].w & 0xfffff) * nR + (t0 + rr[i].x - lo),
                                Tq + rr[i].y, lane);
      }
      return n;
    };
    auto rec_ahead = [&](int c) -> int {
      rec_tail = 0;
      if constexpr (FX) {
        if (c + 2 < nchunk) {
          rec_next2 = fx_rec(c + 2);
          rec_tail = 1;
          return 1;
        }
      }
      return 0;
    };
    for (int k = 0; k < MA; ++k) issue_meta(k);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // prologue: every ring's first MA slots landed
    asm volatile("" ::: "memory");
    int hist[NBUF];  // hist[i]: DMAs this wave issued i+1 iterations ago
#pragma unroll
    for (int i = 0; i < NBUF; ++i) hist[i] = 0;
#pragma unroll
    for (int s2 = 0; s2 < NBUF - 1; ++s2) {
#pragma unroll
      for (int i = NBUF - 1; i > 0; --i) hist[i] = hist[i - 1];
      hist[0] = s2 < nchunk ? issue_samples(s2) + rec_ahead(s2) : 0;
    }
    uint64_t ts_poll = 0, ts_issue = 0, ts_wait = 0, tA = 0, tB = 0;
    for (int k = 0; k < nchunk; ++k) {
      // retire chunk k (and everything older); the NBUF-2 younger chunks stay in flight
      if (stamps) tA = __builtin_amdgcn_s_memtime();
      int younger = FX ? rec_tail : 0;
#pragma unroll
      for (int i = 0; i < NBUF - 2; ++i) younger += hist[i];
      wait_vmcnt(younger);
      if (stamps) { tB = __builtin_amdgcn_s_memtime(); ts_wait += tB - tA; tA = tB; }
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (stamps) { tB = __builtin_amdgcn_s_memtime(); ts_poll += tB - tA; tA = tB; }
      // metadata rows first (loader 0), then the chunk's windows: the rows'
      // latency overlaps the window DMAs instead of trailing them (configs[3]
      // stage 2 101.4 -> 96.3 ms per launch, north star 83.9 -> 82.2).  The
      // compiler's wait for the window records (vmcnt(0): it cannot see the
      // DMAs) is forced here, before any DMA of this iteration, on records
      // loaded one and two chunks ago
      if constexpr (FX)
        asm volatile("" ::"v"(rec_next.x), "v"(rec_next.y), "v"(rec_next.z), "v"(rec_next.w),
                     "v"(rec_next2.x), "v"(rec_next2.y), "v"(rec_next2.z), "v"(rec_next2.w));
      int n = issue_meta(k + MA);
      n += k + NBUF - 1 < nchunk ? issue_samples(k + NBUF - 1) : 0;
      if (k + NBUF - 1 < nchunk) n += rec_ahead(k + NBUF - 1);
      else rec_tail = 0;
#pragma unroll
      for (int i = NBUF - 1; i > 0; --i) hist[i] = hist[i - 1];
      hist[0] = n;
      if (stamps) ts_issue += __builtin_amdgcn_s_memtime() - tA;
    }
    if (stamps && lane == 0) {
      float* o = out + ((int64_t)blockIdx.x * (NCW + NLW) + w) * 4;
      o[0] = (float)ts_wait; o[1] = (float)ts_poll; o[2] = (float)ts_issue; o[3] = 0.f;
    }
    return;
  }

  // ---------------- compute waves: ds_read_b128 at the trial's shift + adds
  // float32 elements: 4 quarter samples per read, float accumulators as float
  // pairs (the adds issue as v_pk_add_f32: two samples per VALU instruction).
  // u16 elements (8/16-bit data): 8 eighth samples per read as packed u16
  // pairs, accumulated with plain 32-bit adds into `lo` (two u16 lanes per
  // add, one v_add3_u32 per channel pair) and normalised every flush_n
  // channels: each lane's bit 15 moves into `hi` (a count of 2^15 per lane,
  // also packed) and `lo` keeps the low 15 bits, so a lane never carries
  // into its neighbour while flush_n * (input bound) <= 32767 (the plan's
  // flush_n).  The total hi * 2^15 + lo is exact (float32-exact below 2^24,
  // the same bound as float accumulators).  16 registers per trial instead
  // of 24 (u16 partial sums + float totals): the tile holds DPW = 6 trials
  // per wave (DB 72) in the registers DPW = 4 took.
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  constexpr int AJ = U16 ? 1 : DPW, AG = U16 ? 1 : G, AH = U16 ? 1 : S / 2;
  f32x2_t acc[AJ][AG][AH];
#pragma unroll
  for (int j = 0; j < AJ; ++j)
#pragma unroll
    for (int g = 0; g < AG; ++g)
#pragma unroll
      for (int h = 0; h < AH; ++h) acc[j][g][h] = (f32x2_t){0.f, 0.f};
  // carries: HI8 (DPW > 6) -- one byte per sample, four samples per
  // register (totals < 255 * 2^15 + 2^16, checked by the plan: 12 registers
  // per trial, DPW = 8 fits); else one u16 per sample, two per register
  // (totals < 2^24: 16 registers per trial)
  constexpr bool HI8 = U16 && DPW > 6;
  constexpr int NHI = U16 ? (HI8 ? 2 : 4) : 1;
  uint32_t lo16[U16 ? DPW : 1][U16 ? G : 1][4], hic[U16 ? DPW : 1][U16 ? G : 1][NHI];
  if constexpr (U16) {
#pragma unroll
    for (int j = 0; j < DPW; ++j)
#pragma unroll
      for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int h = 0; h < 4; ++h) lo16[j][g][h] = 0u;
#pragma unroll
        for (int h = 0; h < NHI; ++h) hic[j][g][h] = 0u;
      }
  }
  auto normalise16 = [&]() {
    if constexpr (U16) {
#pragma unroll
      for (int j = 0; j < DPW; ++j)
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if constexpr (HI8) {
            // lo words 2q and 2q + 1 -> carry bytes 0 / 2 and 1 / 3 of hic[q]
#pragma unroll
            for (int q = 0; q < 2; ++q) {
              const uint32_t ca = (lo16[j][g][2 * q] >> 15) & 0x00010001u;
              const uint32_t cb = (lo16[j][g][2 * q + 1] >> 15) & 0x00010001u;
              hic[j][g][q] += ca + (cb << 8);
            }
          } else {
#pragma unroll
            for (int h = 0; h < 4; ++h) hic[j][g][h] += (lo16[j][g][h] >> 15) & 0x00010001u;
          }
#pragma unroll
          for (int h = 0; h < 4; ++h) lo16[j][g][h] &= 0x7fff7fffu;
        }
    }
  };
  // plane value of trial j, group g, eighth / quarter k2 (before out_bias)
  auto value = [&](int j, int g, int k2) -> float {
    if constexpr (U16) {
      const int h = k2 >> 1, half = k2 & 1;
      const uint32_t l = half ? (lo16[j][g][h] >> 16) : (lo16[j][g][h] & 0xffffu);
      uint32_t c;
      if constexpr (HI8)
        c = (hic[j][g][h >> 1] >> (8 * ((h & 1) + 2 * half))) & 0xffu;
      else
        c = half ? (hic[j][g][h] >> 16) : (hic[j][g][h] & 0xffffu);
      return (float)(c * 32768u + l);
    } else {
      return acc[j][g][k2 >> 1][k2 & 1];
    }
  };
  int since_flush = 0;
  const uint32_t lane_byte = lds_addr_of(img) + lane * 16;
  const uint32_t meta_base = lds_addr_of(metar) + w * DPW * 4;  // loader 0's ring
  typedef int i32x4_t __attribute__((ext_vector_type(4)));
  typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
  static_assert(!U16 || DPW * CC <= 64, "one lane per (channel, trial) shift");
  typedef __attribute__((address_space(3))) u32x4_t lds_u32x4_t;
  uint64_t ts_poll = 0, ts_comp = 0, tA = 0, tB = 0;
  int vmeta_n = 0, ncc_n = 0;  // FX: the next chunk's shifts and count
  // (Measured and dropped, round 6: compute-wave issue priorities by age,
  // raised for the youngest third, or rotating by chunk -- the older waves
  // finish a chunk ~20% earlier and wait at its barrier, but the LDS stays
  // saturated to the end of the chunk: configs[3] 89.5 ms per launch either
  // way, DESIGN.md appendix.)
  __builtin_amdgcn_s_barrier();  // prologue barrier (metadata landed)
  asm volatile("" ::: "memory");
  if (stamps) tB = __builtin_amdgcn_s_memtime();
  for (int k = 0; k < nchunk; ++k) {
    const int b = k % NBUF;
    if (stamps) {
      tA = __builtin_amdgcn_s_memtime();
      ts_comp += tA - tB;
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (stamps) { tB = __builtin_amdgcn_s_memtime(); ts_poll += tB - tA; }
    const int slot = k % MR;
    // ONE ds_read_b32 brings the wave's DPW shifts of all CC channels of the
    // chunk (lane DPW*i + j = trial j at channel i, as LDS byte offsets: the
    // plan stores them pre-scaled by 16), each broadcast by v_readlane when
    // its reads issue.  (A ds_read_b128 of 4 shifts per channel costs 4 LDS
    // cycles per channel; this costs 2 per chunk plus one VALU per shift:
    // configs[3] u8 288 -> 280 ms, configs[1] u8 32.7 -> 27.3 ms.)
    // (the shifts include the channel's offset in the packed buffer; row 0's
    // last field is the chunk's channel count)
    typedef __attribute__((address_space(3))) int lds_int_t;
    const int ml = min(lane / DPW, CC - 1) * ROW + lane % DPW;
    auto read_shifts = [&](int sl) -> int {
      return *(const lds_int_t*)(uintptr_t)(meta_base + (uint32_t)((sl * SLOT + ml) * 4));
    };
    auto read_count = [&](int sl) -> int {
      return *(const lds_int_t*)(uintptr_t)(lds_addr_of(metar) + (uint32_t)((sl * SLOT + DB + 3) * 4));
    };
    int vmeta, ncc;
    if constexpr (FX) {
      // chunk k + 1's shifts and count are read during chunk k (its ring
      // slot landed before barrier k), so no dependent LDS round trip stands
      // between a barrier and the first sample read
      vmeta = k == 0 ? read_shifts(slot) : vmeta_n;
      ncc = __builtin_amdgcn_readfirstlane(k == 0 ? read_count(slot) : ncc_n) >> 20;
      if (k + 1 < nchunk) {
        vmeta_n = read_shifts((k + 1) % MR);
        ncc_n = read_count((k + 1) % MR);
      }
    } else {
      vmeta = read_shifts(slot);
      // (the channel count rides in a separate read: folding it into the shift
      // read -- lanes >= DPW * CC -- measured 1.6% slower for u16, neutral for f32)
      ncc = __builtin_amdgcn_readfirstlane(read_count(slot)) >> 20;
    }
    const uint32_t cb = lane_byte + (uint32_t)(b * buf_e * 16);
    if constexpr (U16) {
      // normalise before a chunk could carry a u16 lane past 65535
      if (since_flush + ncc > flush_n) {
        since_flush = 0;
        normalise16();
      }
      since_flush += ncc;
      // channel pairs (acc + x_c + x_c+1: one v_add3_u32 per two samples);
      // u16 chunks always hold an even count (an odd channel count ends in
      // a pad channel whose window is a row of zeros)
      u32x4_t v0[G], v1[G];
      auto pair = [&](int i) {
#pragma unroll
        for (int j = 0; j < DPW; ++j) {
          const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane(vmeta, DPW * i + j);
          const uint32_t s1 = (uint32_t)__builtin_amdgcn_readlane(vmeta, DPW * (i + 1) + j);
#pragma unroll
          for (int g2 = 0; g2 < G; ++g2) {
            v0[g2] = *(const lds_u32x4_t*)(uintptr_t)(cb + s0 + g2 * 1024);
            v1[g2] = *(const lds_u32x4_t*)(uintptr_t)(cb + s1 + g2 * 1024);
          }
#pragma unroll
          for (int g2 = 0; g2 < G; ++g2) {
            lo16[j][g2][0] = add3_u32(lo16[j][g2][0], v0[g2].x, v1[g2].x);
            lo16[j][g2][1] = add3_u32(lo16[j][g2][1], v0[g2].y, v1[g2].y);
            lo16[j][g2][2] = add3_u32(lo16[j][g2][2], v0[g2].z, v1[g2].z);
            lo16[j][g2][3] = add3_u32(lo16[j][g2][3], v0[g2].w, v1[g2].w);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      };
#pragma unroll
      for (int i = 0; i < CC; i += 2)
        if (i < ncc) pair(i);
    } else {
#pragma unroll
      for (int i = 0; i < CC; ++i) {
        if (i >= ncc) break;
        // the channel's DPW read addresses first (readlane + add each), then
        // two trials of reads in flight: trial j's adds overlap trial j+1's
        // reads (the accumulators take 64 of the 128 VGPRs, the reads 2 x 4G)
        uint32_t a[DPW];
#pragma unroll
        for (int j = 0; j < DPW; ++j)
          a[j] = cb + (uint32_t)__builtin_amdgcn_readlane(vmeta, DPW * i + j);
        f32x4_t v[DPW][G];
#pragma unroll
        for (int j = 0; j < DPW; ++j)
#pragma unroll
          for (int g2 = 0; g2 < G; ++g2)
            v[j][g2] = *(const lds_f32x4_t*)(uintptr_t)(a[j] + g2 * 1024);
#pragma unroll
        for (int j = 0; j < DPW; ++j)
#pragma unroll
          for (int g2 = 0; g2 < G; ++g2) {
            acc[j][g2][0] += v[j][g2].xy;
            acc[j][g2][1] += v[j][g2].zw;
          }
        __builtin_amdgcn_sched_group_barrier(0x002, 2 * DPW, 0);  // addresses
        __builtin_amdgcn_sched_group_barrier(0x100, G, 0);        // reads, trial 0
        __builtin_amdgcn_sched_group_barrier(0x100, G, 0);        // reads, trial 1
#pragma unroll
        for (int j = 0; j < DPW; ++j) {
          __builtin_amdgcn_sched_group_barrier(0x002, 2 * G, 0);  // adds, trial j
          if (j + 2 < DPW) __builtin_amdgcn_sched_group_barrier(0x100, G, 0);  // reads, j+2
        }
      }
    }
  }
  if (stamps) ts_comp += __builtin_amdgcn_s_memtime() - tB;
  if (stamps) {
    if (lane == 0) {
      float* o = out + ((int64_t)blockIdx.x * (NCW + NLW) + w) * 4;
      o[0] = 0.f; o[1] = (float)ts_poll; o[2] = (float)ts_comp; o[3] = 1.f;
    }
    return;
  }
  const int d0 = dblk * DB + w * DPW;
  if constexpr (S == 8) {
    if (r2_pad) {
      // Output as the NEXT sweep's float32 quarters image (subband chain,
      // pdd_subband_chain): row r = grp*row_g + d*row_d of R2 ([rows][r2_nR]
      // float4, quarter length Q2 = 2 Qs, single segment, t_base 0) holds
      //   R2[r][j] = (X(j), X(j + Q2), X(j + 2 Q2), X(j + 3 Q2)),  j < r2_nR,
      // X(t) = this sweep's sample t (t < n_out) or the next sweep's pad
      // r2_pad[r].  A lane's eighths (e + k Qs, k < 8) are elements e (even k)
      // and e + Qs (odd k), and its even eighths 2, 4, 6 + the pad are element
      // Q2 + e of the overlap tail (e < r2_ov = r2_nR - Q2 <= Qs).
      float4* R2 = reinterpret_cast<float4*>(out);
#pragma unroll
      for (int j = 0; j < DPW; ++j) {
        const int d = d0 + j;
        if (d >= D) continue;
        const int64_t r = (int64_t)grp * row_g + (int64_t)d * row_d;
        const float pv = r2_pad[r];
        float4* rrow = R2 + r * r2_nR;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const int64_t e = t0 + g * 64 + lane;
          if (e >= Qs) continue;
          float x8[8];
#pragma unroll
          for (int k2 = 0; k2 < 8; ++k2)
            x8[k2] = (e + k2 * Qs < n_out) ? value(j, g, k2) + out_bias : pv;
          rrow[e] = make_float4(x8[0], x8[2], x8[4], x8[6]);
          rrow[e + Qs] = make_float4(x8[1], x8[3], x8[5], x8[7]);
          if (e < r2_ov) rrow[2 * Qs + e] = make_float4(x8[2], x8[4], x8[6], pv);
        }
      }
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < DPW; ++j) {
    const int d = d0 + j;
    if (d >= D) continue;
    float* orow = out + ((int64_t)grp * row_g + (int64_t)d * row_d) * ld_out + t_base;
    // delay-aligned factorised tiles (fx_skew): trial d's tile covers the
    // elements [t0 - sig[d], t0 - sig[d] + Tq); each element of [0, Qs) is
    // stored by exactly one tile of the trial
    const int64_t ts = t0 - ((FX && sig) ? (int64_t)sig[d] : 0);
#pragma unroll
    for (int k2 = 0; k2 < S; ++k2)
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const int64_t t = ts + g * 64 + lane;
        if (t >= 0 && t < Qs && t_base + t + k2 * Qs < n_out)
          orow[t + k2 * Qs] = value(j, g, k2) + out_bias;
      }
  }
}

// ------------------------------------------------------------------ kernel selection
// The instanced shapes are the lists of sweep_plan.h (expanded here: this is
// what instantiates the kernels); nullptr: no instance for the tiling.
typedef void (*sweep_il_fn)(const float4*, int64_t, int, int, const int*, const int*, int, float*,
                            int64_t, int, int64_t, int64_t, int64_t, int, int, int, int, int64_t,
                            int64_t, int, float, const float*, int64_t, int64_t, const int4*,
                            const int*);
static sweep_il_fn il_kernel_for(const Variant& v, bool fx = false) {
#define X(...) \
  if (il_shape_is(v, fx, __VA_ARGS__)) return k_sweep_il<__VA_ARGS__>;
  PDD_SWEEP_IL_SHAPES(X)
#undef X
  return nullptr;
}

typedef void (*sweep_fn)(const void*, int64_t, int, int64_t, const int*, int, int, const int*,
                         const int*, int, const float*, float*, int64_t, int64_t, int, int, int,
                         int);

static sweep_fn kernel_for(const Variant& v) {
#define X(...) \
  if (generic_shape_is(v, __VA_ARGS__)) return k_sweep<__VA_ARGS__>;
  PDD_SWEEP_GENERIC_SHAPES(X)
#undef X
  return nullptr;
}

// Developer knobs (kernel stamps, timing-only decompositions, forced
// tilings) live in scripts/probes/dev_knobs.patch, applied to a copy of the
// sources by scripts/build_dev.sh; the production library reads no
// environment variable: no debug bits (here), no forced tiling
// (pdd_sweep_plan.hip).
static int debug_flags() { return 0; }

}  // namespace pdd

// The planner's scalars (pdd::PlanDims, sweep_plan.h) + the device copies of
// its tables + the execute-time switches.
struct pdd_sweep_plan : pdd::PlanDims {
  int* d_tab = nullptr;    // generic: [C][Dpad] relative shifts; interleaved: metadata rows
  int* d_bmin = nullptr;   // generic: [n_dblk][C]; interleaved: chunk tables
  int* d_bspan = nullptr;  // [n_dblk][C]
  int* d_pat = nullptr;    // factorised: [n_pat][4] {c0, r1, r2, r3}
  int* d_wt = nullptr;     // factorised: [n_dblk][maxch][kFxWin][4] window records
  int* d_gtab = nullptr;   // factorised: per group first pattern + relative-shift range (LDS stage 1)
  int* d_sig = nullptr;    // factorised, delay-aligned tiles: [Dpad] per-trial skew (fx_skew)
  int input_max = 0;       // largest input value (integer input; 0 = the dtype's bound)
  int poison = 0;          // pdd_sweep_plan_set_poison: 0xFF-fill the pattern image (tests)
  // factorised, LDS stage 1: workgroups of the persistent grid (resident per
  // CU x CUs of the plan's device) with the pre-pass image / the input as source
  int fx_s1_wgs[2] = {0, 0};
  int64_t seg_bytes = 0;   // pdd_sweep_plan_set_segment_bytes: segment budget cap (0 = default)
  // timing of the sweep kernel (pdd_sweep_set_timing): one event pair per
  // bracketed launch, recorded on the execute stream without host syncs
  static constexpr int kEvPairs = 1024;
  hipEvent_t* ev = nullptr;  // [2 * kEvPairs]
  int timing = 0;
  int timed = 0;             // launches bracketed since the last query
  int dropped = 0;           // launches past the pool (not bracketed)
};

using namespace pdd;

// Interleaved path: the output is produced in time segments whose
// interleaved copy R fits a scratch budget (the library's per-stream
// scratch, pdd::scratch, reused across calls); each segment is one k_interleave + one k_sweep_il.
// IlExtra.ds > 1: x is the 8-bit block at the raw rate (channel-major rows
// of N * ds samples, lay.ld apart), co-added by ds in the interleave
// pre-pass.  IlExtra.r2_pad: the output is the next sweep's quarters image
// (k_sweep_il's R2 epilogue; one segment).  IlExtra.R_pre: the image of this
// sweep was built by the previous one (quarter length Qs_pre, nR_pre
// elements per row): no interleave pre-pass, one segment.
// Output samples one segment of the interleaved path can hold (<= 0: the
// delay span alone exceeds the scratch budget of R).  The budget is capped
// by the device memory free now (plus what this stream's image / pattern
// slots already hold): a smaller GPU or a busier one gets more, shorter
// segments instead of a scratch allocation failure.
// Sample range [lo, hi] of an image row around the segment's columns:
// channel plans min(0, min bin) .. max(0, max bin); factorised plans the
// skewed shifts' range plus the extra time tiles of delay-aligned tiles.
static void il_lohi(const pdd_sweep_plan* p, int64_t& lo, int64_t& hi) {
  if (p->fx) {
    lo = p->fx_lo;
    hi = (int64_t)p->fx_hi + p->fx_tpad;
  } else {
    lo = std::min(0, p->min_bin);
    hi = std::max(0, p->max_bin);
  }
}

// Geometry of a segment of cnt output columns: eighth / quarter length Qs
// (whole tiles of Tq elements), nR = Qs + margin elements per image row
// (margin: the delay span and one wave of slack), n_tblk time tiles.  The
// one place it is derived: a caller's pattern buffer is sized
// (pdd_sweep_pattern_bytes) by what execute_il checks it against.  Qs_pre:
// the image was built by the previous sweep with that geometry (IlExtra).
struct IlSeg {
  int64_t lo, hi, margin, Qs, nR, n_tblk;
};
static IlSeg il_seg(const pdd_sweep_plan* p, int64_t cnt, int64_t Qs_pre = 0, int64_t nR_pre = 0) {
  const int Tq = 64 * p->v.G;
  IlSeg g;
  il_lohi(p, g.lo, g.hi);
  g.margin = (g.hi - g.lo) + 64;
  g.Qs = Qs_pre ? Qs_pre : cdiv(cdiv(cnt, p->v.S), Tq) * Tq;
  g.nR = Qs_pre ? nR_pre : g.Qs + g.margin;
  // (delay-aligned factorised tiles: fx_tpad / Tq more time tiles, whose
  // trials cover the columns their skew moved past the last tile)
  g.n_tblk = g.Qs / Tq + (p->fx ? p->fx_tpad / Tq : 0);
  return g;
}

static int64_t il_seg_samples(const pdd_sweep_plan* p, hipStream_t st) {
  const int Tq = 64 * p->v.G;
  const int64_t C = p->C * p->n_grp;
  // bytes of R per segment: 16 GiB = one segment per quarter of a 4096 x
  // 2^22 block (configs[3] at 4 time batches), few launches per step
  int64_t budget = (int64_t)16 << 30;
  // factorised plans also hold the stage-1 pattern image (n_pat + 1 rows)
  const int64_t rows = C + (p->fx ? p->n_pat + 2 : 0);
  // (80 GiB: configs[3] in 4 launches of 1.04 M columns -- 572.9 against 578.3
  // ms per step with 8 launches of 40 GiB; the free-memory cap below keeps
  // smaller or busier GPUs on more, shorter segments)
  if (p->fx) budget = (int64_t)80 << 30;
  if (p->seg_bytes > 0) {
    // a caller's cap (pdd_sweep_plan_set_segment_bytes: tests of the
    // multi-segment path on small blocks)
    budget = std::max<int64_t>(p->seg_bytes, 1 << 16);
  } else {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
      const int64_t avail = (int64_t)fr + (int64_t)scratch_held(st, kScratchImage) +
                            (p->fx ? (int64_t)scratch_held(st, kScratchPattern) : 0);
      // keep 1/8 of it and 512 MiB for the caller
      budget = std::min(budget, std::max<int64_t>(avail - avail / 8 - ((int64_t)512 << 20),
                                                  (int64_t)64 << 20));
    }
  }
  const int64_t nr_max = budget / (rows * 16);
  return (nr_max - il_seg(p, 0).margin) / Tq * Tq * p->v.S;
}

struct IlExtra {
  int ds = 1;
  bool one_seg = false;  // the caller checked that one segment fits (pdd_subband_chain)
  const float* r2_pad = nullptr;
  int64_t r2_nR = 0, r2_ov = 0;
  const float4* R_pre = nullptr;
  int64_t Qs_pre = 0, nR_pre = 0;
  // factorised plans, staged execution (pdd_sweep_execute_stage): bit 0 =
  // stage 1 (pattern image), bit 1 = stage 2 (the sweep), into the caller's
  // pattern buffer P_ext of P_bytes (one segment)
  int stages = 3;
  uint4* P_ext = nullptr;
  int64_t P_bytes = 0;
};

// One execute of the interleaved path: what the three parts of a segment
// (image, patterns, sweep) share.
struct IlRun {
  const pdd_sweep_plan* p;
  const void* x;
  int64_t N;
  InLayout lay;
  int64_t x_off;
  int pad_mode;
  const float* padvals;
  const IlExtra& ex;
  hipStream_t st;
  // factorised plans with the LDS stage 1 build their pattern image straight
  // from x (FxFromInput): no u16-eighths image R
  bool fx_direct;
  float4* R;  // C rows of the image + one row of zeros (the u16 kernel's pad channel)
  uint4* P;   // factorised plans: the pattern image (stage 1), n_pat rows + a row of zeros
};

static int il_launch_failed() {
  set_error("pdd_sweep_execute: kernel launch failed");
  return -3;
}

// Part 1: the segment's image by the pre-pass (r.R == nullptr: built by the
// previous sweep / none, factorised stage 1 reads x).
static int il_build_image(const IlRun& r, const IlSeg& g, int64_t t_base) {
  const pdd_sweep_plan* p = r.p;
  if (!r.R) return 0;
  const int64_t C = p->C * p->n_grp;
  if (hipMemsetAsync(r.R + C * g.nR, 0, (size_t)g.nR * sizeof(float4), r.st) != hipSuccess)
    return il_launch_failed();
  const int ds = r.ex.ds;
  const int64_t b0 = t_base + g.lo + r.x_off;
  int vec = 0;
  if (ds == 2 || ds == 4) {
    const int J = 16 / ds;
    if ((uintptr_t)r.x % 16 == 0 && r.lay.ld % 16 == 0 && b0 % J == 0 && g.Qs % J == 0) vec = 16;
    else if ((uintptr_t)r.x % ds == 0 && r.lay.ld % ds == 0) vec = 1;
  }
  for (const IlInstance& k : kIlInstances) {
    if (k.ds != ds || k.vec != vec || k.dtype != p->dtype || k.u16 != (p->v.S == 8)) continue;
    const IlArgs a{r.x, r.lay, r.N, b0, g.Qs, g.nR, r.pad_mode, r.padvals, r.R};
    hipLaunchKernelGGL(k.fn, dim3((unsigned)cdiv(g.nR, k.per_block), (unsigned)C), dim3(256), 0,
                       r.st, a);
    return hipGetLastError() == hipSuccess ? 0 : il_launch_failed();
  }
  set_error("pdd_sweep_execute: no pre-pass kernel (downsample %d, dtype %d)", ds, p->dtype);
  return -3;
}

// Dynamic LDS of an LDS stage-1 instance: the group's rows (the persistent
// kernel adds kFxSlotBytes for its item slot).
constexpr size_t kFxSlotBytes = 16;
static size_t fx_s1_lds(const pdd_sweep_plan* p, const FxS1Instance& k) {
  return (size_t)(p->fx * (k.block + p->fx_rspan)) * sizeof(uint4);
}
// 8-bit input the persistent stage 1 may load in aligned words (FxPreWords):
// time-major, the fx channels of a group as one fx-byte word per spectrum;
// rows and pieces, 4 consecutive samples of a row as one dword.
static bool fx_s1_words(const void* x, const InLayout& lay, int fx, int64_t Qs) {
  const uintptr_t xa = (uintptr_t)x;
  if (lay.ld_t) return xa % fx == 0 && lay.ld_t % fx == 0;
  return xa % 4 == 0 && Qs % 4 == 0 && (lay.piece ? lay.piece % 4 == 0 : lay.ld % 4 == 0);
}

// Part 2 (factorised plans): the segment's pattern image by stage 1.
static int il_build_patterns(const IlRun& r, const IlSeg& g, int64_t t_base) {
  const pdd_sweep_plan* p = r.p;
  // pdd_sweep_plan_set_poison (a parity-test switch): the pattern rows
  // are filled with 0xFF bytes first, so a sum that read an element stage
  // 1 did not write (the per-pattern ranges of fx_build) shows as a NaN /
  // an overflowed lane instead of a stale-but-plausible value
  if (p->poison &&
      hipMemsetAsync(r.P, 0xFF, (size_t)(p->n_pat * g.nR) * sizeof(uint4), r.st) != hipSuccess)
    return il_launch_failed();
  if (hipMemsetAsync(r.P + p->n_pat * g.nR, 0, (size_t)g.nR * sizeof(uint4), r.st) != hipSuccess)
    return il_launch_failed();
  if (!p->d_gtab) {
    // (a group's relative shifts span more than kFxRspan: the plain stage 1)
    hipLaunchKernelGGL(k_fx_patterns, dim3((unsigned)p->n_pat, (unsigned)cdiv(g.nR, 256 * kIlPer)),
                       dim3(256), 0, r.st, (const uint4*)r.R, g.nR, (const int4*)p->d_pat, p->fx, r.P);
    return hipGetLastError() == hipSuccess ? 0 : il_launch_failed();
  }
  for (const FxS1Instance& k : kFxS1Instances) {
    if (k.src != (r.fx_direct ? p->dtype : kFxImage) || k.fx != p->fx) continue;
    const int NG = (int)(p->C / p->fx);
    FxS1Args a{{r.fx_direct ? r.x : r.R, r.lay, r.N, t_base + g.lo + r.x_off, g.Qs, g.nR,
                r.pad_mode, r.padvals, r.P},
               (const int4*)p->d_pat, p->d_gtab, NG, 0, nullptr, 0, 0};
    const int64_t nblk = cdiv(g.nR, k.block);
    const size_t lds = fx_s1_lds(p, k);
    const int wgs = p->fx_s1_wgs[r.fx_direct];
    a.n_items = NG * nblk;
#ifndef PDD_FX_S1_ONESHOT
    // more than one wave of persistent workgroups: the persistent kernel
    if (wgs > 0 && a.n_items > wgs && a.n_items < (1ll << 31) - 16ll * wgs) {
      a.queue = static_cast<unsigned int*>(scratch(r.st, kScratchSmall, kFxXcds * sizeof(unsigned int)));
      if (!a.queue) return -2;
      if (hipMemsetAsync(a.queue, 0, kFxXcds * sizeof(unsigned int), r.st) != hipSuccess)
        return il_launch_failed();
      a.words = r.fx_direct && p->dtype == PDD_U8 && fx_s1_words(r.x, r.lay, p->fx, g.Qs);
      a.slot = (int)lds;
      hipLaunchKernelGGL(k.fn_p, dim3((unsigned)wgs), dim3(256), lds + kFxSlotBytes, r.st, a);
      return hipGetLastError() == hipSuccess ? 0 : il_launch_failed();
    }
#endif
    hipLaunchKernelGGL(k.fn, dim3((unsigned)NG, (unsigned)nblk), dim3(256), lds, r.st, a);
    return hipGetLastError() == hipSuccess ? 0 : il_launch_failed();
  }
  set_error("pdd_sweep_execute: no stage-1 kernel (groups of %d, dtype %d)", p->fx, p->dtype);
  return -3;
}

// Part 3: the sweep of the segment's cnt columns from t_base on, between
// the plan's timing events.
static int il_launch_sweep(const IlRun& r, const IlSeg& g, int64_t t_base, int64_t cnt, float* out,
                           int64_t ld_out, int64_t row_g, int64_t row_d, float out_bias, int flush_n) {
  const pdd_sweep_plan* p = r.p;
  const IlExtra& ex = r.ex;
  const int64_t blocks = g.n_tblk * p->n_dblk * p->n_grp;
  if (blocks >= (1ll << 31)) {
    set_error("pdd_sweep_execute: grid too large");
    return -1;
  }
  pdd_sweep_plan* pm = const_cast<pdd_sweep_plan*>(p);
  const bool bracket = p->timing && p->timed < pdd_sweep_plan::kEvPairs;
  if (p->timing && !bracket) pm->dropped++;
  if (bracket) (void)hipEventRecord(p->ev[2 * p->timed], r.st);
  hipLaunchKernelGGL(il_kernel_for(p->v, p->fx != 0), dim3((unsigned)blocks), dim3(p->v.threads()),
                     p->lds_bytes, r.st, ex.R_pre ? ex.R_pre : (p->fx ? (const float4*)r.P : r.R),
                     g.nR, (int)(p->fx ? p->fx_rows - 1 : p->C), (int)g.lo, p->d_tab, p->d_bmin,
                     p->maxch, out, ld_out, (int)p->D, g.Qs, t_base, t_base + cnt, p->stride,
                     (int)g.n_tblk, (int)p->n_dblk, debug_flags(), row_g, row_d, flush_n, out_bias,
                     ex.r2_pad, ex.r2_nR, ex.r2_ov, (const int4*)p->d_wt, p->d_sig);
  const int rc = hipGetLastError() == hipSuccess ? 0 : il_launch_failed();
  if (bracket) {
    (void)hipEventRecord(p->ev[2 * p->timed + 1], r.st);
    pm->timed++;
  }
  return rc;
}

static int execute_il(const pdd_sweep_plan* p, const void* x, int64_t N, InLayout lay,
                      int64_t x_off, int pad_mode, const float* padvals, float* out,
                      int64_t ld_out, int64_t n_out, int64_t row_g, int64_t row_d, float out_bias,
                      void* stream, const IlExtra& ex = IlExtra()) {
  const int Tq = 64 * p->v.G;
  const int SP = p->v.S;  // samples per element: 4 (float32 quarters) or 8 (u16 eighths)
  const bool u16 = (SP == 8);
  PDD_REQUIRE(!u16 || p->dtype != PDD_F32, "pdd_sweep_execute: u16 path needs integer input");
  // packed u16 lanes are normalised to 15 bits every floor(32767 / max value)
  // channels (k_sweep_il): 128 channels of 8-bit values, 32 of 16-bit values
  // <= 1023, 64 of the wrap-mode zero-DM image downsampled by 2 (<= 510;
  // pdd_sweep_plan_set_input_max); factorised plans sum patterns of fx samples
  const int vmax = p->input_max > 0 ? p->input_max : (p->dtype == PDD_U8 ? 255 : 1023);
  const int flush_n = std::min(256, 32767 / (vmax * std::max(1, p->fx)));
  PDD_REQUIRE(!u16 || flush_n >= p->v.CC, "pdd_sweep_execute: input bound %d too large for the "
              "packed 16-bit sums", vmax);
  const int64_t C = p->C * p->n_grp;  // all channels (groups are contiguous channel ranges)
  hipStream_t st = as_stream(stream);
  // output samples per segment
  int64_t seg = (ex.one_seg || ex.P_ext) ? std::max<int64_t>(n_out, 1) : il_seg_samples(p, st);
  IlSeg ga = il_seg(p, 0);
  PDD_REQUIRE(seg > 0, "pdd_sweep_execute: delay span %lld too wide for the segment budget",
              (long long)(ga.hi - ga.lo));
  // equal segments (whole tiles): every launch does the same work
  const int64_t nseg = cdiv(n_out, seg);
  seg = cdiv(cdiv(n_out, nseg), (int64_t)SP * Tq) * SP * Tq;
  ga = il_seg(p, seg);  // the longest segment: scratch is sized by it
  PDD_REQUIRE(!(ex.r2_pad || ex.R_pre) || nseg == 1,
              "pdd_subband_chain: the stages need one segment each (%lld)", (long long)nseg);
  if (ex.R_pre)
    PDD_REQUIRE(ga.lo == 0 && n_out <= SP * ex.Qs_pre && ex.Qs_pre % Tq == 0 &&
                    ex.nR_pre >= ex.Qs_pre + ga.hi + 64 && !u16,
                "pdd_subband_chain: stage-2 image does not cover this plan");
  IlRun r{p, x, N, lay, x_off, pad_mode, padvals, ex, st,
          p->fx && p->d_gtab && !ex.R_pre && ex.ds == 1, nullptr, ex.P_ext};
  if (!ex.R_pre && !r.fx_direct) {
    r.R = static_cast<float4*>(scratch(st, kScratchImage, (size_t)((C + 1) * ga.nR) * sizeof(float4)));
    if (!r.R) return -2;
  }
  if (ex.P_ext)
    PDD_REQUIRE(p->fx && (int64_t)(p->n_pat + 1) * ga.nR * 16 <= ex.P_bytes,
                "pdd_sweep_execute_stage: pattern buffer of %lld bytes < %lld",
                (long long)ex.P_bytes, (long long)((p->n_pat + 1) * ga.nR * 16));
  if (p->fx) {
    // (ds > 1: the interleave pre-pass co-adds the raw rows into R and stage
    // 1 builds the patterns from R: sums of fx co-adds <= 4 * 1020 stay exact)
    PDD_REQUIRE(u16 == (p->dtype != PDD_F32) && !ex.r2_pad && !ex.R_pre && p->n_grp == 1 &&
                    (u16 || r.fx_direct),
                "pdd_sweep_execute: factorised plans take single-group input (float32: raw rate)");
    if (!r.P)
      r.P = static_cast<uint4*>(scratch(st, kScratchPattern, (size_t)((p->n_pat + 1) * ga.nR) * sizeof(uint4)));
    if (!r.P) return -2;
  }
  int rc = 0;
  for (int64_t t_base = 0; t_base < n_out && rc == 0; t_base += seg) {
    const int64_t cnt = std::min(seg, n_out - t_base);
    const IlSeg g = il_seg(p, cnt, ex.R_pre ? ex.Qs_pre : 0, ex.nR_pre);
    if (ex.r2_pad && ex.r2_nR != 2 * g.Qs + ex.r2_ov) {
      set_error("pdd_subband_chain: stage-2 image geometry mismatch");
      return -4;
    }
    rc = il_build_image(r, g, t_base);
    if (rc == 0 && p->fx && (ex.stages & 1)) rc = il_build_patterns(r, g, t_base);
    if (rc == 0 && (ex.stages & 2))  // (staged: stage 1 only)
      rc = il_launch_sweep(r, g, t_base, cnt, out, ld_out, row_g, row_d, out_bias, flush_n);
  }
  return rc;
}

static hipError_t upload(int** dst, const std::vector<int>& v) {
  hipError_t e = hipMalloc(dst, v.size() * sizeof(int));
  if (e == hipSuccess) e = hipMemcpy(*dst, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice);
  return e;
}

// Plan (pdd_sweep_plan.hip: no HIP in it), upload its tables, raise the
// kernels' dynamic LDS limits.
static int plan_create(const int32_t* host_table, int64_t n_grp, int64_t D, int64_t C, int dtype,
                       int flags, pdd_sweep_plan** plan_out) {
  PDD_REQUIRE(host_table && plan_out, "pdd_sweep_plan_create: null pointer");
  SweepPlan sp;
  std::string err;
  const int status = plan_sweep(host_table, n_grp, D, C, dtype, flags, sp, err);
  if (status != 0) {
    set_error("%s", err.c_str());
    return status;
  }
  pdd_sweep_plan* p = new pdd_sweep_plan();
  static_cast<PlanDims&>(*p) = sp;
  const bool il = p->v.kind == 0;
  hipError_t e = upload(&p->d_tab, il ? sp.meta : sp.rel);
  if (e == hipSuccess) e = upload(&p->d_bmin, il ? sp.chunks : sp.bmin);
  if (e == hipSuccess) e = upload(&p->d_bspan, sp.bspan);
  if (e == hipSuccess && p->fx) e = upload(&p->d_pat, sp.fxt.pat);
  if (e == hipSuccess && p->fx) e = upload(&p->d_wt, sp.fxt.wt);
  if (e == hipSuccess && p->fx_sig_max > 0) e = upload(&p->d_sig, sp.fxt.sig);
  if (e == hipSuccess && !sp.fxt.gtab.empty()) {
    e = upload(&p->d_gtab, sp.fxt.gtab);
    // the LDS stage 1 (gtab: every group's shift range fits kFxRspan)
    int dev = 0, cus = 0;
    if (e == hipSuccess) e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    for (const FxS1Instance& k : kFxS1Instances) {
      const int lds_max = (int)(4 * (kFxEf + kFxRspan) * sizeof(uint4));
      if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
      if (e == hipSuccess)
        e = hipFuncSetAttribute((const void*)k.fn_p, hipFuncAttributeMaxDynamicSharedMemorySize,
                                lds_max + (int)kFxSlotBytes);
      // the persistent grid of this plan's instances: what the device holds at once
      if (e == hipSuccess && k.fx == p->fx && (k.src == kFxImage || k.src == p->dtype)) {
        int per_cu = 0;
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k.fn_p, 256,
                                                         fx_s1_lds(p, k) + kFxSlotBytes);
        p->fx_s1_wgs[k.src != kFxImage] = per_cu * cus;
      }
    }
  }
  if (e != hipSuccess) {
    set_error("pdd_sweep_plan_create: %s", hipGetErrorString(e));
    pdd_sweep_plan_destroy(p);
    return -2;
  }
  if (p->lds_bytes > 64 * 1024) {
    const void* kf = il ? (const void*)il_kernel_for(p->v, p->fx != 0) : (const void*)kernel_for(p->v);
    e = hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, p->lds_bytes);
    if (e != hipSuccess) {
      set_error("pdd_sweep_plan_create: hipFuncSetAttribute: %s", hipGetErrorString(e));
      pdd_sweep_plan_destroy(p);
      return -2;
    }
  }
  *plan_out = p;
  return 0;
}

// The shape, stride, piece and pad checks of the execute entry points (fn:
// the entry point's name in the message).  N >= N_min samples per row, ld_min
// apart at least (channel-major input); 0 <= n_out <= n_out_max columns.
struct ExecShape {
  const char* fn;
  int64_t N, N_min, ld, ld_min, piece, x_off, n_out, n_out_max, ld_out, row_g, row_d;
  int pad_mode;
  const float* padvals;
};
static int check_execute(const ExecShape& a) {
  PDD_REQUIRE(a.N >= a.N_min && a.n_out >= 0 && a.n_out <= a.n_out_max && a.ld_out >= a.n_out &&
                  a.x_off >= 0 && a.row_g >= 0 && a.row_d >= 0,
              "%s: bad shape", a.fn);
  PDD_REQUIRE(a.piece > 0 || a.ld >= a.ld_min, "%s: row stride %lld < %lld", a.fn, (long long)a.ld,
              (long long)a.ld_min);
  PDD_REQUIRE(a.piece == 0 || (a.piece & (a.piece - 1)) == 0, "%s: piece must be 2^k", a.fn);
  PDD_REQUIRE(a.pad_mode == PDD_PAD_ROTATE || (a.pad_mode == PDD_PAD_VALUE && a.padvals),
              "%s: bad pad mode %d", a.fn, a.pad_mode);
  return 0;
}
// Channel-major rows ld apart, or pieces of `piece` samples of C channels.
static InLayout in_layout(int64_t ld, int64_t piece = 0, int64_t C = 0) {
  InLayout lay{ld, piece, 0, C * piece, 0};
  while ((1ll << lay.psh) < piece) ++lay.psh;
  return lay;
}
constexpr int64_t kAnyColumns = INT64_MAX;

extern "C" {

int pdd_sweep_plan_create(const int32_t* host_table, int64_t D, int64_t C, int dtype,
                          pdd_sweep_plan** plan_out) {
  return plan_create(host_table, 1, D, C, dtype, PDD_SWEEP_FACTOR, plan_out);
}

int pdd_sweep_plan_create_ex(const int32_t* host_table, int64_t D, int64_t C, int dtype, int flags,
                             pdd_sweep_plan** plan_out) {
  return plan_create(host_table, 1, D, C, dtype, flags, plan_out);
}

int pdd_sweep_plan_create_grouped(const int32_t* host_table, int64_t n_grp, int64_t D, int64_t C,
                                  int dtype, pdd_sweep_plan** plan_out) {
  return plan_create(host_table, n_grp, D, C, dtype, 0, plan_out);
}

int pdd_sweep_plan_factor(const pdd_sweep_plan* p, int64_t* n_patterns) {
  PDD_REQUIRE(p, "pdd_sweep_plan_factor: null pointer");
  if (n_patterns) *n_patterns = p->n_pat;
  return p->fx;
}

int pdd_sweep_plan_skew(const pdd_sweep_plan* p, int64_t* extra_tiles) {
  PDD_REQUIRE(p, "pdd_sweep_plan_skew: null pointer");
  if (extra_tiles) *extra_tiles = p->fx ? p->fx_tpad / (64 * p->v.G) : 0;
  return p->fx ? p->fx_sig_max : 0;
}

int pdd_sweep_plan_info(const pdd_sweep_plan* p, int64_t* info) {
  PDD_REQUIRE(p && info, "pdd_sweep_plan_info: null pointer");
  info[0] = p->D;
  info[1] = p->C;
  info[2] = p->v.DB();
  info[3] = p->v.TB();
  info[4] = p->lds_bytes;
  info[5] = p->max_bin;
  info[6] = p->min_bin;
  info[7] = p->vi;
  return 0;
}

int pdd_sweep_execute(const pdd_sweep_plan* p, const void* x, int64_t N, int64_t ld, int pad_mode,
                      const float* padvals, float* out, int64_t ld_out, int64_t n_out,
                      void* stream) {
  return pdd_sweep_execute_ex(p, x, N, ld, 0, 0, pad_mode, padvals, out, ld_out, n_out, 0.f,
                              stream);
}

int pdd_sweep_execute_ex(const pdd_sweep_plan* p, const void* x, int64_t N, int64_t ld,
                         int64_t piece, int64_t x_off, int pad_mode, const float* padvals,
                         float* out, int64_t ld_out, int64_t n_out, float out_bias, void* stream) {
  PDD_REQUIRE(p && x && out, "pdd_sweep_execute: null pointer");
  if (int rc = check_execute({"pdd_sweep_execute", N, 1, ld, N, piece, x_off, n_out, kAnyColumns,
                              ld_out, 0, 0, pad_mode, padvals}))
    return rc;
  if (n_out == 0) return 0;
  if (p->v.kind == 0)
    return execute_il(p, x, N, in_layout(ld, piece, p->C * p->n_grp), x_off, pad_mode, padvals, out,
                      ld_out, n_out, 0, 1, out_bias, stream);
  PDD_REQUIRE(piece == 0 && x_off == 0 && out_bias == 0.f,
              "pdd_sweep_execute: the generic (sparse-grid) kernel reads channel-major input "
              "at offset 0 without an output bias");
  // every staged index must stay inside int64 / the LDS image: the shifts are
  // bounded by the plan, the samples by N + n_out.
  const int64_t n_tblk = cdiv(n_out, p->v.TB());
  const int64_t blocks = n_tblk * p->n_dblk;
  PDD_REQUIRE(blocks < (1ll << 31), "pdd_sweep_execute: grid too large");
  sweep_fn fn = kernel_for(p->v);
  PDD_REQUIRE(fn != nullptr, "pdd_sweep_execute: no kernel");
  hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(p->v.threads()), p->lds_bytes,
                     as_stream(stream), x, ld, (int)p->C, N, p->d_tab, (int)p->Dpad, (int)p->D,
                     p->d_bmin, p->d_bspan, pad_mode, padvals, out, ld_out, n_out, debug_flags(),
                     p->stride, (int)n_tblk, (int)p->n_dblk);
  PDD_LAUNCHED();
  return 0;
}

int pdd_sweep_execute_tm(const pdd_sweep_plan* p, const void* x, int64_t N, int64_t ld_t,
                         int64_t x_off, int pad_mode, const float* padvals, float* out,
                         int64_t ld_out, int64_t n_out, float out_bias, void* stream) {
  PDD_REQUIRE(p && x && out, "pdd_sweep_execute_tm: null pointer");
  // (the spectrum stride takes the row stride's place in the checks: >= all channels)
  if (int rc = check_execute({"pdd_sweep_execute_tm", N, 1, ld_t, p->C * p->n_grp, 0, x_off, n_out,
                              kAnyColumns, ld_out, 0, 0, pad_mode, padvals}))
    return rc;
  if (n_out == 0) return 0;
  PDD_REQUIRE(p->v.kind == 0, "pdd_sweep_execute_tm: the generic (sparse-grid) kernel reads "
              "channel-major input");
  InLayout lay = in_layout(0);
  lay.ld_t = ld_t;
  return execute_il(p, x, N, lay, x_off, pad_mode, padvals, out, ld_out, n_out, 0, 1, out_bias,
                    stream);
}

int64_t pdd_sweep_pattern_bytes(const pdd_sweep_plan* p, int64_t n_out) {
  PDD_REQUIRE(p && n_out >= 0, "pdd_sweep_pattern_bytes: bad arguments");
  if (!p->fx || !p->d_gtab || p->v.kind != 0) return 0;
  return (int64_t)(p->n_pat + 1) * il_seg(p, std::max<int64_t>(n_out, 1)).nR * 16;
}

int pdd_sweep_execute_stage(const pdd_sweep_plan* p, const void* x, int64_t N, int64_t ld,
                            int64_t piece, int64_t x_off, int pad_mode, const float* padvals,
                            float* out, int64_t ld_out, int64_t n_out, float out_bias,
                            void* patterns, int64_t pattern_bytes, int stage, void* stream) {
  PDD_REQUIRE(p && x && patterns && (out || stage == 1), "pdd_sweep_execute_stage: null pointer");
  PDD_REQUIRE(p->fx && p->d_gtab && p->v.kind == 0 && p->n_grp == 1,
              "pdd_sweep_execute_stage: needs a factorised single-group plan");
  PDD_REQUIRE(stage >= 1 && stage <= 3, "pdd_sweep_execute_stage: stage %d not 1, 2 or 3", stage);
  // (stage 1 alone writes no plane: no ld_out to check)
  if (int rc = check_execute({"pdd_sweep_execute_stage", N, 1, ld, N, piece, x_off, n_out,
                              kAnyColumns, stage == 1 ? n_out : ld_out, 0, 0, pad_mode, padvals}))
    return rc;
  if (n_out == 0) return 0;
  IlExtra ex;
  ex.stages = stage;
  ex.P_ext = static_cast<uint4*>(patterns);
  ex.P_bytes = pattern_bytes;
  return execute_il(p, x, N, in_layout(ld, piece, p->C), x_off, pad_mode, padvals, out, ld_out,
                    n_out, 0, 1, out_bias, stream, ex);
}

int pdd_stream_create_cu_mask(const uint32_t* mask, int n_words, void** stream) {
  PDD_REQUIRE(mask && stream && n_words > 0, "pdd_stream_create_cu_mask: bad arguments");
  hipStream_t st = nullptr;
  PDD_HIP(hipExtStreamCreateWithCUMask(&st, (uint32_t)n_words, mask));
  *stream = st;
  return 0;
}

int pdd_stream_destroy(void* stream) {
  PDD_REQUIRE(stream, "pdd_stream_destroy: null stream");
  PDD_HIP(hipStreamDestroy(as_stream(stream)));
  return 0;
}

int pdd_sweep_execute_grouped(const pdd_sweep_plan* p, const void* x, int64_t N, int64_t ld,
                              int pad_mode, const float* padvals, float* out, int64_t ld_out,
                              int64_t n_out, int64_t row_g, int64_t row_d, void* stream) {
  PDD_REQUIRE(p && x && out, "pdd_sweep_execute_grouped: null pointer");
  PDD_REQUIRE(p->v.kind == 0, "pdd_sweep_execute_grouped: plan has no grouped kernel");
  if (int rc = check_execute({"pdd_sweep_execute_grouped", N, 1, ld, N, 0, 0, n_out, kAnyColumns,
                              ld_out, row_g, row_d, pad_mode, padvals}))
    return rc;
  if (n_out == 0) return 0;
  return execute_il(p, x, N, in_layout(ld), 0, pad_mode, padvals, out, ld_out, n_out, row_g, row_d,
                    0.f, stream);
}

int pdd_sweep_execute_ds(const pdd_sweep_plan* p, const uint8_t* x8, int64_t n_raw, int64_t ld,
                         int64_t ds, int pad_mode, const float* padvals, float* out,
                         int64_t ld_out, int64_t n_out, int64_t row_g, int64_t row_d,
                         void* stream) {
  PDD_REQUIRE(p && x8 && out, "pdd_sweep_execute_ds: null pointer");
  PDD_REQUIRE(p->v.kind == 0 && p->v.S == 8 && p->dtype == PDD_U16,
              "pdd_sweep_execute_ds: needs a PDD_U16 plan on the 16-bit interleaved tiling");
  PDD_REQUIRE(ds >= 2 && ds <= 4, "pdd_sweep_execute_ds: downsample factor %lld not in 2..4",
              (long long)ds);
  const int64_t N = n_raw / ds;
  if (int rc = check_execute({"pdd_sweep_execute_ds", N, 0, ld, n_raw, 0, 0, n_out, N, ld_out, row_g,
                              row_d, pad_mode, padvals}))
    return rc;
  if (n_out == 0) return 0;
  IlExtra ex;
  ex.ds = (int)ds;
  return execute_il(p, x8, N, in_layout(ld), 0, pad_mode, padvals, out, ld_out, n_out,
                    p->n_grp > 1 ? row_g : 0, row_d, 0.f, stream, ex);
}

int pdd_subband_chain(const pdd_sweep_plan* p1, const void* x, int64_t n_raw, int64_t ld, int64_t ds,
                      int pad1_mode, const float* pad1vals, const pdd_sweep_plan* p2,
                      const float* pad2vals, float* out, int64_t ld_out, int64_t n_out,
                      int64_t row_g, int64_t row_d, void* stream) {
  PDD_REQUIRE(p1 && p2 && x && out && pad2vals, "pdd_subband_chain: null pointer");
  PDD_REQUIRE(p1->v.kind == 0 && p1->v.S == 8 &&
                  ((p1->dtype == PDD_U8 && ds == 1) || (p1->dtype == PDD_U16 && ds >= 2 && ds <= 4)),
              "pdd_subband_chain: stage 1 needs an 8-bit (ds 1) or 16-bit (ds 2..4) plan on the "
              "16-bit interleaved tiling");
  PDD_REQUIRE(p2->v.kind == 0 && p2->v.S == 4 && p2->dtype == PDD_F32 && p2->min_bin >= 0,
              "pdd_subband_chain: stage 2 needs a float32 interleaved plan with delays >= 0");
  PDD_REQUIRE(p2->C * p2->n_grp == p1->D * p1->n_grp,
              "pdd_subband_chain: stage-2 channels (%lld) != stage-1 rows (%lld)",
              (long long)(p2->C * p2->n_grp), (long long)(p1->D * p1->n_grp));
  const int64_t N1 = n_raw / ds;
  if (int rc = check_execute({"pdd_subband_chain", N1, 1, ld, n_raw, 0, 0, n_out, N1, ld_out, row_g,
                              row_d, pad1_mode, pad1vals}))
    return rc;
  if (n_out == 0) return 0;
  // factorised plans sweep single-group input through their pattern image:
  // they do not chain (pdd.h)
  if (p1->fx || p2->fx) {
    set_error("pdd_subband_chain: factorised plans do not chain");
    return PDD_ENOCHAIN;
  }
  // stage 1 covers N1 samples in one segment of eighth length Qs1; stage 2
  // reads quarters of length 2 Qs1 (a multiple of its 256-element tile)
  // (ov: stage 2's row margin, its delay span + 64 -- its delays are >= 0)
  const int64_t Qs1 = il_seg(p1, N1).Qs;
  const int64_t ov = il_seg(p2, n_out).margin;
  if (!(ov <= Qs1 && (2 * Qs1) % (64 * p2->v.G) == 0)) {
    set_error("pdd_subband_chain: block of %lld samples does not chain (stage-2 span %d)",
              (long long)N1, p2->max_bin);
    return PDD_ENOCHAIN;  // nothing launched: run the stages apart
  }
  const int64_t C2 = p2->C * p2->n_grp;
  const int64_t nR2 = 2 * Qs1 + ov;
  hipStream_t st = as_stream(stream);
  // stage 2's image first, THEN the one-segment check of both stages (their
  // budgets are capped by the device memory free after it): the decision is
  // made once, here, and the stages run with it (IlExtra.one_seg) instead of
  // re-deriving it from a free-memory figure that their own scratch changes
  float4* R2 = static_cast<float4*>(scratch(st, kScratchChain, (size_t)(C2 * nR2) * sizeof(float4)));
  if (!R2) return -2;
  if (!(il_seg_samples(p1, st) >= N1 && il_seg_samples(p2, st) >= n_out)) {
    set_error("pdd_subband_chain: block of %lld samples does not chain (one segment per stage "
              "needed)", (long long)N1);
    return PDD_ENOCHAIN;  // nothing launched: run the stages apart
  }
  IlExtra e1;
  e1.ds = (int)ds;
  e1.one_seg = true;
  e1.r2_pad = pad2vals;
  e1.r2_nR = nR2;
  e1.r2_ov = ov;
  // stage-1 rows (= stage-2 channels): trial d of group g -> row d * n_grp1 + g
  int rc = execute_il(p1, x, N1, in_layout(ld), 0, pad1_mode, pad1vals, (float*)R2, 0, N1,
                      1, p1->n_grp, 0.f, stream, e1);
  if (rc == 0) {
    IlExtra e2;
    e2.one_seg = true;
    e2.R_pre = R2;
    e2.Qs_pre = 2 * Qs1;
    e2.nR_pre = nR2;
    rc = execute_il(p2, nullptr, N1, in_layout(0), 0, PDD_PAD_VALUE, pad2vals, out, ld_out,
                    n_out, row_g, row_d, 0.f, stream, e2);
  }
  return rc;
}

int pdd_sweep_plan_set_input_max(pdd_sweep_plan* p, int max_value) {
  PDD_REQUIRE(p, "pdd_sweep_plan_set_input_max: null pointer");
  PDD_REQUIRE(p->dtype != PDD_F32, "pdd_sweep_plan_set_input_max: integer-input plans only");
  const int bound = p->dtype == PDD_U8 ? 255 : 1023;
  PDD_REQUIRE(max_value >= 1 && max_value <= bound,
              "pdd_sweep_plan_set_input_max: %d outside [1, %d]", max_value, bound);
  p->input_max = max_value;
  return 0;
}

int pdd_sweep_plan_set_poison(pdd_sweep_plan* p, int on) {
  PDD_REQUIRE(p, "pdd_sweep_plan_set_poison: null pointer");
  p->poison = on ? 1 : 0;
  return 0;
}

int pdd_sweep_plan_set_segment_bytes(pdd_sweep_plan* p, int64_t bytes) {
  PDD_REQUIRE(p, "pdd_sweep_plan_set_segment_bytes: null pointer");
  PDD_REQUIRE(bytes >= 0, "pdd_sweep_plan_set_segment_bytes: negative budget");
  p->seg_bytes = bytes;
  return 0;
}

int pdd_sweep_set_timing(pdd_sweep_plan* p, int on) {
  PDD_REQUIRE(p, "pdd_sweep_set_timing: null pointer");
  if (on && !p->ev) {
    p->ev = new hipEvent_t[2 * pdd_sweep_plan::kEvPairs]();
    for (int i = 0; i < 2 * pdd_sweep_plan::kEvPairs; ++i) PDD_HIP(hipEventCreate(&p->ev[i]));
  }
  p->timing = on ? 1 : 0;
  p->timed = 0;
  p->dropped = 0;
  return 0;
}

int pdd_sweep_timing_read(pdd_sweep_plan* p, float* total_ms, int64_t* launches) {
  PDD_REQUIRE(p && total_ms && launches, "pdd_sweep_timing_read: null pointer");
  PDD_REQUIRE(p->timing && p->timed, "pdd_sweep_timing_read: no timed launch (pdd_sweep_set_timing)");
  PDD_REQUIRE(!p->dropped, "pdd_sweep_timing_read: %d launches past the %d-pair event pool",
              p->dropped, pdd_sweep_plan::kEvPairs);
  PDD_HIP(hipEventSynchronize(p->ev[2 * p->timed - 1]));
  double sum = 0.0;
  for (int i = 0; i < p->timed; ++i) {
    float ms = 0.f;
    PDD_HIP(hipEventElapsedTime(&ms, p->ev[2 * i], p->ev[2 * i + 1]));
    sum += ms;
  }
  *total_ms = (float)sum;
  *launches = p->timed;
  p->timed = 0;
  return 0;
}

int pdd_sweep_kernel_ms(pdd_sweep_plan* p, float* ms) {
  int64_t n = 0;
  return pdd_sweep_timing_read(p, ms, &n);
}

int pdd_sweep_plan_destroy(pdd_sweep_plan* p) {
  if (!p) return 0;
  if (p->ev) {
    for (int i = 0; i < 2 * pdd_sweep_plan::kEvPairs; ++i)
      if (p->ev[i]) (void)hipEventDestroy(p->ev[i]);
    delete[] p->ev;
  }
  if (p->d_tab) (void)hipFree(p->d_tab);
  if (p->d_bmin) (void)hipFree(p->d_bmin);
  if (p->d_bspan) (void)hipFree(p->d_bspan);
  if (p->d_pat) (void)hipFree(p->d_pat);
  if (p->d_wt) (void)hipFree(p->d_wt);
  if (p->d_gtab) (void)hipFree(p->d_gtab);
  if (p->d_sig) (void)hipFree(p->d_sig);
  delete p;
  return 0;
}

}  // extern "C"
