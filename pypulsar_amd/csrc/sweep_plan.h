// The sweep planner's interface: plain C++17, no HIP.  plan_sweep
// (pdd_sweep_plan.hip) turns a [n_grp][D][C] delay table into the tiling, the
// chunk packing, the factorisation and every host table the kernels of
// pdd_sweep.hip read; pdd_sweep.hip uploads them.  The constants both sides
// use are defined here, once.  tests/native/plan_dump.cpp runs the planner
// on the CPU (tests/test_sweep_plan.py).
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/pdd.h"

namespace pdd {

// ------------------------------------------------------------------ shared with the kernels
// Metadata ring of k_sweep_il (synchronisation comment in pdd_sweep.hip):
// loader 0 DMAs the rows of chunk j MA = 2(NBUF-1) chunks ahead.
constexpr int il_ma(int nbuf) { return 2 * nbuf - 2; }
// (ring slots: chunk j's rows are written after barrier j - MA and read by
// the end of chunk j's compute -- factorised tiles read them a chunk early
// -- and every wave has finished its reads of chunk j before barrier j + 1,
// after which chunk j + MA + 1 may overwrite the slot: MA + 1 slots suffice.
// Two buffers: 3 slots; the fourth slot's 3.2 KiB went to the chunk buffers,
// configs[3] stage 2 90.76 -> 90.08 ms, north star 59.42 -> 58.57 ms per
// launch.)
constexpr int il_mr(int nbuf) { return nbuf <= 2 ? 3 : (nbuf <= 4 ? 8 : (nbuf <= 8 ? 16 : 32)); }
constexpr int il_slot(int cc, int db) { return (cc * (db + 4) + 63) / 64 * 64; }
constexpr int il_meta_bytes(int nbuf, int cc, int db) { return il_mr(nbuf) * il_slot(cc, db) * 4; }

// Factorised sweeps: trial blocks per XCD tile group of the u16 kernel (tile
// order of k_sweep_il; fx_build pairs the blocks' group orders when it is 2)
#ifndef PDD_FX_GJ
#define PDD_FX_GJ 2
#endif
// window records per chunk: wt[dblk][chunk][kFxWin] (k_sweep_il FX)
constexpr int kFxWin = 64;
// Stage 1 through LDS (k_fx_stage1): kFxE-element blocks, groups whose
// relative-shift range is <= kFxRspan (checked by the plan: gtab)
constexpr int kFxE = 512, kFxRspan = 512;
// float32 stage 1 (k_fx_stage1<FxFromInput<float>, g>) builds 1024-element blocks: configs[1]
// f32 7.31 -> 7.10 ms per launch against 512 (8-bit stage 1: 512 best, 12.5
// against 14.2 ms at 1024)
constexpr int kFxEf = 1024;
// Largest mean chunk ratio (re-chunked pair order / own packing) at which a
// factorised plan keeps the pair order of its trial blocks (fx_build).
#ifndef PDD_FX_PAIR_MAX
#define PDD_FX_PAIR_MAX 1.06
#endif

// ------------------------------------------------------------------ variants
// kind 0: interleaved image + k_sweep_il (dedicated loader waves, NLW);
// kind 1: generic striped k_sweep (register staging; sparse-grid fallback).
struct Variant {
  int kind;
  bool u8;     // kind 1: 8-bit input staged as u16 pairs
  int S, G, DPW, NW, CC, NBUF;
  int NLW;     // kind 0: loader waves (NW = compute waves)
  int threads() const { return (NW + (kind == 0 ? NLW : 0)) * 64; }
  int elem_bytes() const { return kind == 0 ? 16 : (u8 ? 2 * S : 4 * S); }
  int Q() const { return 64 * G; }
  int TB() const { return S * 64 * G; }
  int DB() const { return NW * DPW; }
  // LDS "stride" (elements per channel per buffer) for a max span
  int64_t stride_for(int max_span) const {
    if (kind == 0) return (64 * G + max_span + 63) / 64 * 64;  // whole 64-element DMA granules
    return (Q() + max_span + 15) / 16 * 16;
  }
  int64_t chan_bytes(int64_t stride) const { return stride * elem_bytes(); }
};

// Candidate tilings, best first; the plan takes the first whose LDS fits (a
// sparser grid -- wider shift span per trial block -- moves down the list;
// grouped sweeps skip the kinds that cannot sweep groups).
// Every entry is reached by a named test (tests/test_gpu_parity.py
// test_sweep_variant_ladder, tests/test_sweep_plan.py).
static const Variant kF32Variants[] = {
    {0, false, 4, 4, 4, 14, 8, 2, 2},  // DB 56, 2 packed buffers of <= 8 channels (configs[1]:
                                       //   37.9 ms against 39.4 with 3 buffers)
    {0, false, 4, 4, 4, 8, 8, 2, 2},   // DB 32
    {1, false, 4, 4, 1, 8, 1, 2, 0},   // generic, DB 8
    {1, false, 4, 1, 1, 1, 1, 2, 0}    // generic, DB 1 (any span that fits 160 KB)
};
// 8-bit input: u16 eighths (12 compute + 4 loader waves: with half the
// compute per staged byte the extra loaders pay off), then the float32-image
// tilings, then the generic u16 kernel.
// Factorised 8/16-bit plans try these first (before their channel tiling):
// u16 eighths, DB 96 -- 8 trials per compute wave with byte-wide carry
// counts (plane sums < 255 * 2^15: C * input bound checked by the plan).
// configs[3] g 4 101.8 -> 97.2 ms per launch, north star g 2 83.3 -> 81.6
// against DB 72; the channel kernel is 2% slower at DB 96 (configs[1] u8
// 21.0 -> 21.5 ms), so channel plans keep DB 72.
#ifndef PDD_FX_DPW
#define PDD_FX_DPW 8
#endif
static const Variant kU8FxVariants[] = {{0, false, 8, 2, PDD_FX_DPW, 12, 8, 2, 4}};
// 8-bit input, short grids (plan_sweep): u16 eighths, DB 40 in 8-wave
// tiles (5 compute waves of 8 trials + 3 loaders, <= 78 KB of LDS, 120
// VGPRs): two tiles per CU, so one tile's first window DMAs and plane stores
// run under the other's reads.  Reported as variant kShortVi.  (configs[2]
// stage-1 sweep 1.34 -> 1.12 ms against 10 + 4 waves, one tile per CU;
// float32 short grids in 7 + 1-wave DB-28 tiles, two per CU: 1.60 -> 1.57
// ms, not kept: each of the two trial blocks stages every window again.)
static const Variant kU8Short = {0, false, 8, 2, 8, 5, 8, 2, 3};
// float32 input, grouped short grids: quarters, DB 52 (13 compute + 3 loader
// waves; configs[2] stage 2: 50 trials per pass in 52 slots instead of 56)
static const Variant kF32Short = {0, false, 4, 4, 4, 13, 8, 2, 3};
static constexpr int kShortVi = 100;
static const Variant kU8Variants[] = {
    {0, false, 8, 2, 6, 12, 8, 2, 4},   // u16 eighths, DB 72: 6 trials per compute wave in the
                                        //   registers 4 took with float totals (k_sweep_il's
                                        //   15-bit normalised sums), 2 packed buffers
    {0, false, 8, 2, 4, 12, 8, 2, 4},   // u16 eighths, DB 48 (configs[3]: 236.7 ms against 239.0
                                        //   with 3 buffers, once the loaders read no LDS)
    {0, false, 4, 4, 4, 8, 8, 2, 2},    // f32 image of u8 data, DB 32
    {1, true, 8, 2, 1, 8, 1, 2, 0},     // generic u16, DB 8
    {1, true, 8, 1, 1, 1, 1, 2, 0}      // generic u16, DB 1
};

// LDS per workgroup: 16-wave (il) tiles run one per CU, <= 8-wave tiles two
inline int64_t lds_budget(const Variant& v) {
  if (v.kind == 0) return (v.NW + v.NLW) * 2 <= 16 ? 78 * 1024 : 158 * 1024;
  return v.NW >= 16 ? 150 * 1024 : 76 * 1024;
}
static constexpr int kLdsMax = 160 * 1024;

// The instanced kernel shapes, listed once: pdd_sweep.hip expands each list
// into the function-pointer selection (which instantiates the kernels), the
// planner into "is there an instance for this tiling".
// k_sweep_il<G, DPW, NCW, NLW, CC, NBUF, U16, FX>: u16 eighths (S = 8) or
// float32 quarters (S = 4); FX = factorised stage 2.
#define PDD_SWEEP_IL_SHAPES(X)          \
  X(2, 8, 12, 4, 8, 2, true, true)      \
  X(2, 6, 12, 4, 8, 2, true, true)      \
  X(2, 4, 12, 4, 8, 2, true, true)      \
  X(4, 4, 14, 2, 8, 2, false, true)     \
  X(2, 8, 5, 3, 8, 2, true, false)      \
  X(2, 6, 12, 4, 8, 2, true, false)     \
  X(2, 4, 12, 4, 8, 2, true, false)     \
  X(4, 4, 13, 3, 8, 2, false, false)    \
  X(4, 4, 14, 2, 8, 2, false, false)    \
  X(4, 4, 8, 2, 8, 2, false, false)
// k_sweep<U8, S, G, DPW, NW, CC, NBUF>
#define PDD_SWEEP_GENERIC_SHAPES(X) \
  X(false, 4, 4, 1, 8, 1, 2)        \
  X(false, 4, 1, 1, 1, 1, 2)        \
  X(true, 8, 2, 1, 8, 1, 2)         \
  X(true, 8, 1, 1, 1, 1, 2)
inline bool il_shape_is(const Variant& v, bool fx, int G, int DPW, int NCW, int NLW, int CC, int NBUF,
                        bool U16, bool FX) {
  return fx == FX && v.S == (U16 ? 8 : 4) && v.G == G && v.DPW == DPW && v.NW == NCW &&
         v.NLW == NLW && v.CC == CC && v.NBUF == NBUF;
}
inline bool generic_shape_is(const Variant& v, bool U8, int S, int G, int DPW, int NW, int CC,
                             int NBUF) {
  return v.u8 == U8 && v.S == S && v.G == G && v.DPW == DPW && v.NW == NW && v.CC == CC &&
         v.NBUF == NBUF;
}
inline bool il_instanced(const Variant& v, bool fx) {
#define X(...) if (il_shape_is(v, fx, __VA_ARGS__)) return true;
  PDD_SWEEP_IL_SHAPES(X)
#undef X
  return false;
}

// ------------------------------------------------------------------ the plan
// Tables of a factorised plan (module comment at k_fx_patterns): the
// pattern pool, the per-(trial block, group) metadata rows in the layout of
// the channel sweep (DB LDS byte offsets -- the trial's pattern window +
// base shift -- then {0, 0, 0, group | groups in the chunk << 20}), the chunk
// tables, and the window records of every chunk.
struct FxTables {
  std::vector<int> pat;            // [n_pat][4] {c0, r1, r2, r3}
  std::vector<int> wt;             // [n_dblk][maxch][kFxWin][4] window records
  std::vector<int> mt, cht, gtab;  // gtab empty: a group's shift range exceeds kFxRspan
  int64_t n_pat = 0, rows_pb = 0;  // metadata rows per trial block
  int rspan = 0;                   // widest relative-shift range of a group
  int maxch = 0;
  double cost_b = 0, cost_f = 0;   // modelled cycles per time tile: channel sweep / factorised
  double el_f = 0, el_b = 0;       // staged elements per time tile (the model's inputs)
  double pair_ratio = 1.0;         // mean chunks of the re-chunked pair order / own packing
  // delay-aligned tiles: trial d's tile covers output elements [t0 - sig[d],
  // t0 - sig[d] + Tq) (sig per padded trial, >= 0); the pattern rows cover
  // samples lo_f .. hi_f (+ tpad) around the segment (fx_skew)
  std::vector<int> sig;
  int sig_max = 0, lo_f = 0, hi_f = 0;
};

// The scalars of a finished plan (pdd_sweep_plan embeds them).
struct PlanDims {
  Variant v = {};
  int vi = 0;              // reported index of the tiling in its candidate list (kShortVi)
  int dtype = PDD_F32;     // input element type
  int64_t n_grp = 1;       // independent channel groups (grouped sweep)
  int64_t D = 0, C = 0, Dpad = 0, n_dblk = 0;
  int max_span = 0, stride = 0, lds_bytes = 0;
  int max_bin = 0, min_bin = 0;
  int maxch = 0;           // interleaved kernel: most chunks of a trial block
  int fx = 0;              // factorised sweep: channels per group (0 = channel by channel)
  int64_t n_pat = 0;       // factorised: pattern series (stage-1 rows, + 1 zero row)
  int64_t fx_rows = 0;     // factorised: metadata rows per trial block (groups + pad groups)
  int fx_rspan = 0;        // factorised: widest relative-shift range of a group (stage-1 LDS)
  int fx_lo = 0, fx_hi = 0;  // factorised: pattern-row sample range (skewed shifts; fx_build)
  int fx_tpad = 0;         // factorised: extra time-tile elements per segment (max skew, whole tiles)
  int fx_sig_max = 0;      // factorised: largest per-trial skew
};

// A finished plan: the scalars and the host tables the kernels read.
struct SweepPlan : PlanDims {
  // generic kernel (kind 1)
  std::vector<int> rel;     // [C][Dpad] shifts relative to the block minimum
  std::vector<int> bmin;    // [n_dblk][C] block minimum per channel
  // interleaved kernel (kind 0); factorised plans: the rows / chunks of the groups
  std::vector<int> meta;    // metadata rows [n_grp][n_dblk][C + 1][DB + 4] (+ 8 rows of zeros)
  std::vector<int> chunks;  // chunk tables [n_grp * n_dblk][1 + maxch]: count, then c0 | ncc << 20
  std::vector<int> bspan;   // [n_dblk][C] shift span per (block, channel), last group's
  // factorised plans: pat, wt, gtab, sig and the cost model (mt and cht moved
  // into meta and chunks; pair_ratio: the pair-order build's)
  FxTables fxt;
};

// Plans the sweep of host_table[n_grp][D][C] (flags: PDD_SWEEP_*).  Returns 0,
// or a libpdd status with the message for set_error in `err`.
int plan_sweep(const int32_t* host_table, int64_t n_grp, int64_t D, int64_t C, int dtype, int flags,
               SweepPlan& plan, std::string& err);

}  // namespace pdd
