// libpdd: the sweep planner.  Host-only std::vector arithmetic over the
// [n_grp][D][C] delay table: the trial tiling (the ladder of candidate
// Variants), the chunk packing, the factorisation (groups of 4, 2 or none, by
// the cost model) and the delay-aligned skew.  Everything the kernels of
// pdd_sweep.hip do follows from the tables built here (sweep_plan.h).
// No HIP: the file also compiles as plain C++ (c++ -x c++ -std=c++17), which
// is how tests/native/plan_dump.cpp runs it on the CPU.
#include <algorithm>
#include <array>
#include <map>
#include <unordered_map>
#include <utility>

#include "sweep_plan.h"

namespace pdd {

static int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The production library reads no environment variable: no forced tiling
// (developer builds: scripts/probes/dev_knobs.patch, scripts/build_dev.sh).
static int forced_variant() { return -1; }

// Delay-aligned tiles (factorised plans).  A trial block's tile reads, at
// group g, the windows [t0 + b[d][g], t0 + b[d][g] + Tq) of its trials: the
// window of a pattern spans the drift of b[d][g] over the block's trials (up
// to ~680 samples at the bottom of the north star's band against Tq = 128
// elements).  Trial d's tile may as well cover the output elements [t0 -
// sig[d], t0 - sig[d] + Tq) for any per-trial skew sig[d]: it then reads
// group g at b[d][g] - sig[d].  With sig[d] = b[d][gr] - min over the block
// (gr: a reference group near the middle of the band, the one minimising the
// summed drift of b - sig over the groups) the drift of group g becomes
// |drift(g) - drift(gr)|: the north star stages 24% fewer window elements,
// configs[3] 19% (tests/native/plan_dump.cpp).  The plane is the same
// sum at the same (trial, column): only which tile produces a column changes
// (each segment gets ceil(max sig / Tq) more time tiles; the kernel stores
// elements inside [0, Qs) only).
static void fx_skew(const int32_t* tab, int64_t D, int64_t C, int64_t DB, int fx,
                    std::vector<int>& sig) {
  const int64_t NG = C / fx, n_dblk = cdiv(D, DB);
  sig.assign((size_t)(n_dblk * DB), 0);
  std::vector<int> lo((size_t)NG), hi((size_t)NG);
  for (int64_t b = 0; b < n_dblk; ++b) {
    auto base = [&](int64_t j, int64_t g) -> int {
      return tab[std::min(b * DB + j, D - 1) * C + g * fx];
    };
    // candidate reference groups: 17 evenly spaced, then the neighbourhood
    // of the best at the finest step
    auto drift = [&](int64_t gr) -> int64_t {
      std::fill(lo.begin(), lo.end(), INT32_MAX);
      std::fill(hi.begin(), hi.end(), INT32_MIN);
      for (int64_t j = 0; j < DB; ++j) {
        const int s = base(j, gr);
        for (int64_t g = 0; g < NG; ++g) {
          const int x = base(j, g) - s;
          lo[(size_t)g] = std::min(lo[(size_t)g], x);
          hi[(size_t)g] = std::max(hi[(size_t)g], x);
        }
      }
      int64_t t = 0;
      for (int64_t g = 0; g < NG; ++g) t += (int64_t)hi[(size_t)g] - lo[(size_t)g];
      return t;
    };
    int64_t best = -1, best_t = INT64_MAX;
    const int64_t step = std::max<int64_t>(1, NG / 16);
    for (int64_t gr = 0; gr < NG; gr += step) {
      const int64_t t = drift(gr);
      if (t < best_t) { best_t = t; best = gr; }
    }
    for (int64_t gr = std::max<int64_t>(0, best - step + 1); gr < std::min(NG, best + step); gr += std::max<int64_t>(1, step / 8)) {
      const int64_t t = drift(gr);
      if (t < best_t) { best_t = t; best = gr; }
    }
    int mn = INT32_MAX;
    for (int64_t j = 0; j < DB; ++j) mn = std::min(mn, base(j, best));
    for (int64_t j = 0; j < DB; ++j) sig[(size_t)(b * DB + j)] = base(j, best) - mn;
  }
}

static bool fx_build(const int32_t* tab, int64_t D, int64_t C, const Variant& v, int64_t buf_e,
                     int fx, bool force, FxTables& T, bool pairs = true, bool skew = true) {
  if (C % fx != 0 || C < 2 * fx) return false;
  T.el_f = T.el_b = 0;
  const int64_t NG = C / fx, DB = v.DB(), ROW = DB + 4, Tq = 64 * v.G;
  const int64_t n_dblk = cdiv(D, DB);
  // per-trial skew (fx_skew; all zero: tiles aligned on the plane's columns)
  if (skew) fx_skew(tab, D, C, DB, fx, T.sig);
  else T.sig.assign((size_t)(n_dblk * DB), 0);
  const std::vector<int>& sig = T.sig;
  T.sig_max = 0;
  for (int s : sig) T.sig_max = std::max(T.sig_max, s);
  // the group base shift of (padded trial dp, group g) as the tile reads it
  auto bsk = [&](int64_t dp, int64_t g) -> int {
    return tab[std::min(dp, D - 1) * C + g * fx] - sig[(size_t)dp];
  };
  // the pattern rows' sample range relative to the segment: every channel's
  // shift less its trial's skew (a pattern sums its channels at r_k more)
  int32_t lo_all = 0, hi_all = 0;
  for (int64_t d = 0; d < D; ++d)
    for (int64_t c = 0; c < C; ++c) {
      lo_all = std::min(lo_all, tab[d * C + c] - sig[(size_t)d]);
      hi_all = std::max(hi_all, tab[d * C + c] - sig[(size_t)d]);
    }
  // (rounded down to 16 samples: the downsampling pre-pass of the stream
  // takes its 16-byte vector form only on aligned segment starts)
  lo_all = -((-lo_all + 15) / 16 * 16);
  T.lo_f = lo_all;
  T.hi_f = hi_all;
  // pattern of (trial, group): relative shifts r1..r3 (packed key) -> pool row
  std::vector<int> pid((size_t)(D * NG));
  std::unordered_map<uint64_t, int> idx;
  T.pat.clear();
  for (int64_t g = 0; g < NG; ++g) {
    idx.clear();
    for (int64_t d = 0; d < D; ++d) {
      const int32_t* r = tab + d * C + g * fx;
      uint64_t key = 0;
      for (int k = 1; k < fx; ++k) {
        const int64_t rel = (int64_t)r[k] - r[0];
        if (rel < -(1 << 20) || rel >= (1 << 20)) return false;
        key = (key << 21) | (uint64_t)(rel + (1 << 20));
      }
      auto it = idx.find(key);
      int id;
      if (it == idx.end()) {
        id = (int)(T.pat.size() / 4);
        idx.emplace(key, id);
        T.pat.push_back((int)(g * fx));
        for (int k = 1; k < 4; ++k) T.pat.push_back(k < fx ? r[k] - r[0] : 0);
      } else {
        id = it->second;
      }
      pid[(size_t)(d * NG + g)] = id;
    }
  }
  T.n_pat = (int64_t)T.pat.size() / 4;
  {
    // per group: first pattern, then the relative-shift range (stage 1 via LDS)
    T.gtab.assign((size_t)(NG + 1 + 2 * NG), 0);
    bool fits = true;
    int64_t g = -1;
    for (int64_t p = 0; p < T.n_pat; ++p) {
      const int64_t pg = T.pat[(size_t)(4 * p)] / fx;
      while (g < pg) T.gtab[(size_t)(++g)] = (int)p;
      int& lo = T.gtab[(size_t)(NG + 1 + 2 * pg)];
      int& hi = T.gtab[(size_t)(NG + 2 + 2 * pg)];
      for (int k = 1; k < fx; ++k) {
        lo = std::min(lo, T.pat[(size_t)(4 * p + k)]);
        hi = std::max(hi, T.pat[(size_t)(4 * p + k)]);
      }
      if (hi - lo > kFxRspan) fits = false;
      T.rspan = std::max(T.rspan, hi - lo);
    }
    while (g < NG) T.gtab[(size_t)(++g)] = (int)T.n_pat;
    if (!fits) T.gtab.clear();
  }
  if (!T.gtab.empty()) {
    // then [n_pat] x {first, last - nR} = the pattern row's elements stage 2
    // reads: trials of pattern p have base shifts b in [bmin_p, bmax_p], so
    // its windows cover elements [bmin_p - lo, Qs + bmax_p - lo) of a
    // segment's row (nR = Qs + hi - lo + 64; lo = min(0, min bin), hi =
    // max(0, max bin)); stage 1 skips its kFxE-element blocks outside them
    // (5-10% of the image's bytes are delay overhang no trial of the pattern
    // reads)
    // (skewed: b = the base shift less the trial's skew; rows cover [lo_f,
    // Qs + tpad + hi_f), tpad = the skew rounded up to whole time tiles)
    const size_t o = (size_t)(3 * NG + 1);
    T.gtab.resize(o + 2 * (size_t)T.n_pat);
    for (int64_t p = 0; p < T.n_pat; ++p) {
      T.gtab[o + 2 * p] = INT32_MAX;
      T.gtab[o + 2 * p + 1] = INT32_MIN;
    }
    for (int64_t d = 0; d < D; ++d)
      for (int64_t g = 0; g < NG; ++g) {
        const size_t q = o + 2 * (size_t)pid[(size_t)(d * NG + g)];
        const int32_t b = bsk(d, g);
        T.gtab[q] = std::min(T.gtab[q], b - lo_all);
        T.gtab[q + 1] = std::max(T.gtab[q + 1], b - hi_all - 64);
      }
  }
  // float32 patterns are built only by the LDS stage 1 from the input rows
  // (k_fx_stage1<FxFromInput<float>, g>: float adds)
  if (v.S == 4 && T.gtab.empty()) return false;
  // (a quick screen: stage 1 + stage 2 adds against the channel sweep's)
  if (!force && (double)T.n_pat * fx + (double)D * NG > 0.75 * (double)D * C) return false;
  if (T.n_pat + 1 >= (1 << 20)) return false;
  const int zero_row = (int)T.n_pat;  // pad groups read a window of this row of zeros
  // Rows (metadata) are laid out per trial block in chunk order: the groups,
  // in pairs (the u16 loop adds two per v_add3_u32), and a pad group wherever
  // a group goes alone -- the last of an odd count, or one whose pair's
  // windows do not fit a chunk buffer together.
  std::vector<std::vector<int>> rows_of((size_t)n_dblk);  // per block: mt rows [row][ROW]
  std::vector<std::vector<int>> chunks((size_t)n_dblk);
  std::vector<std::vector<std::vector<std::array<int, 4>>>> cw((size_t)n_dblk);
  auto gran = [&](int span) -> int64_t { return (Tq + span + 63) / 64 * 64; };
  // a pattern window takes exactly its Tq + span elements of the chunk
  // buffer: its last DMA piece lands under an EXEC mask (k_sweep_il fx_issue)
  auto gran_fx = [&](int span) -> int64_t { return Tq + span; };
  int64_t rows_pb = 0;
  double cost_b = 0, cost_f = 0;
  std::vector<int64_t> prev_seq;  // the even trial block's group order
  double ratio_sum = 0;            // (pair order) replayed / own chunks, summed over odd blocks
  int64_t ratio_n = 0;
  for (int64_t b = 0; b < n_dblk; ++b) {
    std::vector<int>& M = rows_of[(size_t)b];
    int64_t r0 = 0, nrow = 0, used = 0;
    std::vector<std::array<int, 4>> rec;  // the open chunk's window records
    auto close = [&]() {
      if (nrow == 0) return;
      for (int64_t r = r0; r < r0 + nrow; ++r) M[(size_t)(r * ROW + DB + 3)] = (int)(r | (nrow << 20));
      chunks[(size_t)b].push_back((int)(r0 | (nrow << 20)));
      for (auto& x : rec) x[3] |= (int)rec.size() << 20;
      cw[(size_t)b].push_back(rec);
      rec.clear();
      r0 += nrow;
      nrow = 0;
      used = 0;
    };
    // windows of group g in this block: {pattern row, bmin, span}, first-use order
    auto windows = [&](int64_t g, std::vector<std::array<int, 3>>& w) {
      w.clear();
      if (g < 0 || g >= NG) {
        w.push_back({zero_row, 0, 0});
        return;
      }
      for (int64_t j = 0; j < DB; ++j) {
        const int64_t d = std::min(b * DB + j, D - 1);
        const int id = pid[(size_t)(d * NG + g)];
        const int base = bsk(b * DB + j, g);
        size_t i = 0;
        while (i < w.size() && w[i][0] != id) ++i;
        if (i == w.size()) w.push_back({id, base, base});
        else {
          w[i][1] = std::min(w[i][1], base);
          w[i][2] = std::max(w[i][2], base);
        }
      }
      for (auto& x : w) x[2] -= x[1];  // span
    };
    auto need_of = [&](const std::vector<std::array<int, 3>>& w) {
      int64_t n = 0;
      for (auto& x : w) n += gran_fx(x[2]);
      return n;
    };
    // one row (group g, or a pad group for g < 0) with its windows
    auto place = [&](int64_t g, const std::vector<std::array<int, 3>>& w) {
      const size_t base_row = M.size();
      M.resize(base_row + (size_t)ROW, 0);
      std::vector<int64_t> off(w.size());
      for (size_t i = 0; i < w.size(); ++i) {
        off[i] = used;
        rec.push_back({w[i][1], (int)(Tq + w[i][2]), (int)used, w[i][0]});
        used += gran_fx(w[i][2]);
      }
      for (int64_t j = 0; j < DB; ++j) {
        int o = (int)(16 * off[0]);
        if (g >= 0 && g < NG) {
          const int64_t d = std::min(b * DB + j, D - 1);
          const int id = pid[(size_t)(d * NG + g)];
          const int base = bsk(b * DB + j, g);
          size_t i = 0;
          while (w[i][0] != id) ++i;
          o = (int)(16 * (off[i] + base - w[i][1]));
        }
        M[base_row + (size_t)j] = o;
      }
      ++nrow;
    };
    // Packing: a plane row sums over all groups and the sums are exact in
    // any order (float32 plans: regrouped within tolerance), so the groups
    // go into the chunks in any order, in pairs.  Two packings are built
    // per trial block and the one with the lower modelled time is placed:
    //  - best fit: the largest remaining group that fits, then the largest
    //    partner that fits beside it (fewest chunks);
    //  - balanced: the largest remaining group, then the SMALLEST partner
    //    that fits, so every chunk mixes large and small window sets and its
    //    compute (groups) tracks its staging (elements).
    // A chunk's compute overlaps the next chunk's staging, so the model sums
    // max(compute of chunk k, staging of chunk k + 1) plus a fixed cost per
    // chunk.  A group with no partner closes the chunk (or, alone in a fresh
    // chunk, takes a pad group).  (Measured, round 5, stage 2 per launch:
    // best fit / balanced / the model's choice, configs[3] 93.55 / 92.53 /
    // 92.42 ms, north star 62.02 / 66.95 / 61.77 ms.  Best fit over in-order
    // pairs, configs[3] 305 -> 256 chunks per trial block, stage 2 95.1 ms
    // either way; north star 461 -> 361, 65.2 -> 63.1 ms; configs[1] f32 23.9
    // -> 23.7 ms.  Best fit among the 16 lowest unplaced groups only, to keep
    // neighbouring trial blocks in step: configs[3] 97.0 ms.)
    std::vector<std::array<int, 3>> wz;
    windows(-1, wz);
    {
      std::vector<std::vector<std::array<int, 3>>> wg((size_t)NG);
      std::vector<int64_t> need_g((size_t)NG);
      for (int64_t g = 0; g < NG; ++g) {
        windows(g, wg[(size_t)g]);
        need_g[(size_t)g] = need_of(wg[(size_t)g]);
      }
      const int64_t need_z = need_of(wz);
      auto nw = [&](int64_t g) -> int64_t { return g < 0 ? 1 : (int64_t)wg[(size_t)g].size(); };
      auto nd = [&](int64_t g) -> int64_t { return g < 0 ? need_z : need_g[(size_t)g]; };
      // chunks as group lists (-1: a pad group); false when a group cannot fit
      auto pack = [&](bool balanced, std::vector<std::vector<int64_t>>& out) -> bool {
        out.clear();
        std::multimap<int64_t, int64_t> pool;  // need -> group
        for (int64_t g = 0; g < NG; ++g) pool.emplace(need_g[(size_t)g], g);
        auto largest = [&](int64_t room, int64_t wroom) -> int64_t {
          auto it = pool.upper_bound(room);
          while (it != pool.begin()) {
            --it;
            if (nw(it->second) <= wroom) {
              const int64_t g = it->second;
              pool.erase(it);
              return g;
            }
          }
          return -1;
        };
        auto smallest = [&](int64_t room, int64_t wroom) -> int64_t {
          for (auto it = pool.begin(); it != pool.end() && it->first <= room; ++it)
            if (nw(it->second) <= wroom) {
              const int64_t g = it->second;
              pool.erase(it);
              return g;
            }
          return -1;
        };
        std::vector<int64_t> cur;
        int64_t used_c = 0, win_c = 0;
        auto flush = [&]() {
          out.push_back(cur);
          cur.clear();
          used_c = win_c = 0;
        };
        while (!pool.empty()) {
          const bool fresh = cur.empty();
          const int64_t room = buf_e - used_c, wroom = kFxWin - win_c;
          const int64_t a = (int64_t)cur.size() + 2 <= v.CC ? largest(room, wroom) : -1;
          if (a < 0) {
            if (fresh) return false;
            flush();
            continue;
          }
          const int64_t bg = balanced ? smallest(room - nd(a), wroom - nw(a))
                                      : largest(room - nd(a), wroom - nw(a));
          if (bg >= 0 || (fresh && nd(a) + need_z <= room && nw(a) + 1 <= wroom)) {
            cur.push_back(a);
            cur.push_back(bg);
            used_c += nd(a) + nd(bg);
            win_c += nw(a) + nw(bg);
          } else if (fresh) {
            return false;
          } else {
            pool.emplace(nd(a), a);
            flush();
          }
        }
        if (!cur.empty()) flush();
        return true;
      };
      const double kc_g = v.S == 8 ? 440.0 * (double)DB / 48.0 : 1156.0 * (double)DB / 56.0;
      const double st_e = v.S == 8 ? 1.0 : 1.28;
      auto model = [&](const std::vector<std::vector<int64_t>>& ch) -> double {
        auto bytes = [&](const std::vector<int64_t>& c) {
          int64_t n = 0;
          for (int64_t g : c) n += nd(g);
          return (double)n;
        };
        double t = ch.empty() ? 0.0 : st_e * bytes(ch[0]);
        for (size_t k = 0; k < ch.size(); ++k)
          t += std::max(kc_g * (double)ch[k].size(), k + 1 < ch.size() ? st_e * bytes(ch[k + 1]) : 0.0) +
               1200.0;
        return t;
      };
      // (float32 tiles keep best fit: balanced chunks measured 23.24 -> 24.08
      // ms per configs[1] launch although the model preferred them)
      std::vector<std::vector<int64_t>> ch_f, ch_b, ch_r;
      const bool ok_f = pack(false, ch_f);
      const bool ok_b = v.S == 8 && pack(true, ch_b);
      if (!ok_f && !ok_b) return false;
      const auto* ch = !ok_b ? &ch_f : (!ok_f ? &ch_b : (model(ch_b) < model(ch_f) ? &ch_b : &ch_f));
      // The second trial block of an XCD tile group (PDD_FX_GJ = 2) stages
      // its groups in the first block's order, re-chunked to its own window
      // sizes, so the two blocks' concurrent tiles stage the same group's
      // pattern rows at about the same time (L2 hits).  The plan uses it
      // only where the re-chunked orders cost at most 5% more chunks than
      // the blocks' own packings on average (fx_build runs again without it
      // otherwise).  (Measured, round 5: configs[3], +2% chunks, stage 2
      // 90.84 -> 88.69 ms per launch, L2-side fetch 418 -> 329 GB; the north
      // star, +11% chunks, 59.01 -> 59.99 ms with it; a 2.5% per-block gate
      // instead: configs[3] 90.48 -> 91.08, north star 60.76 -> 59.44.)
      if (pairs && v.S == 8 && PDD_FX_GJ == 2 && (b & 1) && !prev_seq.empty()) {
        bool ok = true;
        std::vector<int64_t> cur;
        int64_t used_c = 0, win_c = 0;
        for (size_t i = 0; i + 1 < prev_seq.size() && ok; i += 2) {
          const int64_t ga = prev_seq[i], gb = prev_seq[i + 1];
          const int64_t need = nd(ga) + nd(gb), w = nw(ga) + nw(gb);
          if (need > buf_e || w > kFxWin) { ok = false; break; }
          if ((int64_t)cur.size() + 2 > v.CC || used_c + need > buf_e || win_c + w > kFxWin) {
            ch_r.push_back(cur);
            cur.clear();
            used_c = win_c = 0;
          }
          cur.push_back(ga);
          cur.push_back(gb);
          used_c += need;
          win_c += w;
        }
        if (ok && !cur.empty()) ch_r.push_back(cur);
        if (ok) {
          ratio_sum += (double)ch_r.size() / (double)std::max<size_t>(1, ch->size());
          ++ratio_n;
          ch = &ch_r;
        }
      }
      prev_seq.clear();
      if (!(b & 1))
        for (const auto& c : *ch) prev_seq.insert(prev_seq.end(), c.begin(), c.end());
      for (const auto& c : *ch) {
        for (int64_t g : c) place(g, g < 0 ? wz : wg[(size_t)g]);
        close();
      }
    }
    close();
    rows_pb = std::max(rows_pb, r0);
    // cost model of one tile of this trial block (CU cycles; calibrated on
    // MI355X, round 5): the compute waves take ~440 cycles per channel of a
    // 48-trial u16 tile (~110 per group of 4 once factorised: the adds and
    // LDS reads scale with C / g and with the tile's trials), the loaders
    // ~1.0 per staged element (LDS-DMA issue and landing); the tile pays
    // 1.016 x the larger plus 0.203 x the smaller (the DMAs' LDS writes take
    // LDS cycles from the compute waves' reads).  Fitted on the DB 96 tiles
    // of configs[3] g 4 (1.37 M cycles per tile, staging-bound), the north
    // star g 4 (1.89 M) and g 2 (2.22 M, both terms ~1.8 M).
    int64_t el_b = 0, el_f = 0;  // staged elements: channel sweep / factorised
    for (int64_t c = 0; c < C; ++c) {
      int lo_ = INT32_MAX, hi_ = INT32_MIN;
      for (int64_t j = 0; j < DB; ++j) {
        const int x = tab[std::min(b * DB + j, D - 1) * C + c];
        lo_ = std::min(lo_, x);
        hi_ = std::max(hi_, x);
      }
      el_b += gran(hi_ - lo_);
    }
    for (const auto& ch : cw[(size_t)b])
      for (const auto& r : ch) el_f += (r[1] + 63) / 64 * 64;
    T.el_f += (double)el_f;
    T.el_b += (double)el_b;
    if (v.S == 8) {
      const double kc = 440.0 * (double)DB / 48.0;  // compute cycles per channel of the tile
      auto tile = [](double comp, double st) {
        return 1.016 * std::max(comp, st) + 0.203 * std::min(comp, st);
      };
      cost_b += tile(kc * (double)C, (double)el_b);
      cost_f += tile(kc * (double)C / fx, (double)el_f);
    } else {
      // float32 quarters (configs[1] f32: 1.18 M cycles per 56-trial tile,
      // compute-bound at ~1156 cycles per channel; staging ~1.28 per element)
      const double kc = 1156.0 * (double)DB / 56.0;
      cost_b += std::max(kc * (double)C, 1.28 * (double)el_b);
      cost_f += std::max(kc * (double)C / fx, 1.28 * (double)el_f);
    }
  }
  // stage 1 per time tile: every pattern's Tq elements (2 KiB of eighths, 4 KiB
  // of quarters), written once for all trial blocks, ~251 CU cycles per 2 KiB
  // pattern row plus ~655 per channel group (its input rows and shift range
  // staged once): fitted on k_fx_stage1 (8-bit input), configs[3] g 4 (12.6 ms per
  // 1.04 M-column launch) and the north star g 4 / g 2 (12.65 / 6.48 ms)
  cost_f += ((double)T.n_pat * 251.0 + (double)NG * 655.0) * (double)Tq / 128.0;
  // the channel sweep's interleave pre-pass: every channel's Tq elements per
  // time tile, written and read once (factorised plans build their pattern
  // rows from the input directly)
  cost_b += (double)C * (double)(Tq * 16) * 2.0 / 6.7;
  T.cost_b = cost_b;
  T.cost_f = cost_f;
  T.pair_ratio = ratio_n ? ratio_sum / (double)ratio_n : 1.0;
  // (the plan takes the factorised tables below 0.95 of the channel sweep's
  // modelled cost: configs[1] u8 g 2 models at 0.927 and measures 18.6
  // against 21.6 ms per step; the margin was 0.9.  Developer builds print the
  // model's numbers with PDD_SWEEP_DEBUG bit 3.)
  if (!force && cost_f > 0.95 * cost_b) return false;
  T.rows_pb = rows_pb;
  T.mt.assign((size_t)(n_dblk * rows_pb * ROW), 0);
  for (int64_t b = 0; b < n_dblk; ++b)
    std::copy(rows_of[(size_t)b].begin(), rows_of[(size_t)b].end(),
              T.mt.begin() + (size_t)(b * rows_pb * ROW));
  size_t maxch = 0;
  for (const auto& l : chunks) maxch = std::max(maxch, l.size());
  T.maxch = (int)maxch;
  T.cht.assign((size_t)(n_dblk * (maxch + 1)), 0);
  T.wt.assign((size_t)(n_dblk * maxch * kFxWin * 4), 0);
  for (int64_t b = 0; b < n_dblk; ++b) {
    const auto& l = chunks[(size_t)b];
    T.cht[(size_t)(b * (maxch + 1))] = (int)l.size();
    for (size_t k = 0; k < l.size(); ++k) {
      T.cht[(size_t)(b * (maxch + 1) + 1 + k)] = l[k];
      const auto& r = cw[(size_t)b][k];
      int* o = &T.wt[((size_t)b * maxch + k) * kFxWin * 4];
      for (size_t i = 0; i < r.size(); ++i)
        for (int f = 0; f < 4; ++f) o[i * 4 + f] = r[i][f];
    }
  }
  return true;
}

static int fail(std::string& err, const std::string& msg) {
  err = "pdd_sweep_plan_create: " + msg;
  return -1;
}

int plan_sweep(const int32_t* host_table, int64_t n_grp, int64_t D, int64_t C, int dtype, int flags,
               SweepPlan& plan, std::string& err) {
  if (!(n_grp >= 1 && n_grp * C < (1 << 20))) return fail(err, "bad group count");
  if (!(D > 0 && C > 0 && D < (1 << 24) && C < (1 << 20)))
    return fail(err, "bad extents D=" + std::to_string(D) + " C=" + std::to_string(C));
  if (!(dtype == PDD_F32 || dtype == PDD_U8 || dtype == PDD_U16)) return fail(err, "dtype must be F32, U8 or U16");
  // 16-bit input (<= 1023) shares the 8-bit tilings minus the generic kernel
  const bool int_in = dtype != PDD_F32;
  const Variant* cands = int_in ? kU8Variants : kF32Variants;
  const int ncand = int_in ? (int)(sizeof(kU8Variants) / sizeof(Variant))
                           : (int)(sizeof(kF32Variants) / sizeof(Variant));

  const int fv = forced_variant();
  // Short grids (the grouped sweeps of a DDplan step: 40-50 trials per
  // group) waste most of a 72-trial tile: 8/16-bit plans start at the
  // 48-trial tiling when it pads the grid to >= 3% fewer trial slots
  // (configs[2] stage 1: 40 trials in 48 slots instead of 72)
  int v0 = 0;
  auto slots = [&](const Variant& x) { return cdiv(D, (int64_t)x.DB()) * x.DB(); };
  if (int_in && slots(kU8Variants[1]) * 103 < slots(kU8Variants[0]) * 100) v0 = 1;
  // ... and grouped plans at the 40-trial tiling (kU8Short, reported as
  // variant kShortVi) when that pads to >= 3% fewer slots again (configs[2]
  // stage 1: 40 trials in 40 slots)
  // (grouped plans only: single-group plans keep the tilings their
  // factorised sweeps are instanced for; kU8Short's 8 trials per wave keep
  // byte-wide carry counts: plane sums <= 255 * 2^15)
  const bool short_first =
      fv < 0 && n_grp > 1 &&
      (int_in ? slots(kU8Short) * 103 < std::min(slots(kU8Variants[0]), slots(kU8Variants[1])) * 100 &&
                    C * (dtype == PDD_U8 ? 255 : 1023) <= 255 * 32768
              : slots(kF32Short) * 103 < slots(kF32Variants[0]) * 100);
  std::vector<std::pair<Variant, int>> cl;  // (tiling, its reported index)
  if (short_first) cl.push_back({int_in ? kU8Short : kF32Short, kShortVi});
  for (int vi = (fv >= 0 && fv < ncand) ? fv : v0; vi < ncand; ++vi) cl.push_back({cands[vi], vi});
  for (const auto& cv : cl) {
    const Variant v = cv.first;
    const int vi = cv.second;
    const bool il = v.kind == 0;
    if (n_grp > 1 && !il) continue;  // only the interleaved kernel sweeps groups
    if (dtype == PDD_U16 && !il)       // the generic kernel reads 8-bit or float32 rows
      return fail(err, "DM grid too sparse for a 16-bit-input tile");
    const int64_t DB = v.DB();
    const int64_t n_dblk = cdiv(D, DB);
    const int64_t Dpad = n_dblk * DB;
    std::vector<int> meta;  // interleaved path: metadata rows of every group, concatenated
    std::vector<std::vector<int>> chunks;  // interleaved path: per (group, block) chunk list
    int max_span = 0, mx = INT32_MIN, mn = INT32_MAX;
    std::vector<int> rel, bmin, bspan;
    const bool last = (vi == ncand - 1);
    // interleaved kernel: NBUF chunk buffers of buf_e 16-B elements each
    // (what the LDS holds beside the metadata ring); a chunk packs up to CC
    // channel windows of 64-element DMA granules, Tq + span each
    int64_t buf_e = 0;
    bool fits = true;
    if (il) {
      const int64_t room = (last ? kLdsMax : lds_budget(v)) - il_meta_bytes(v.NBUF, v.CC, v.DB());
      buf_e = std::max<int64_t>(0, room / (v.NBUF * 16) / 64 * 64);
    }
    for (int64_t grp = 0; grp < n_grp; ++grp) {
      const int32_t* htab = host_table + grp * D * C;
      rel.assign((size_t)(C * Dpad), 0);
      bmin.assign((size_t)(n_dblk * C), 0);
      bspan.assign((size_t)(n_dblk * C), 0);
      for (int64_t d = 0; d < Dpad; ++d) {
        const int32_t* row = htab + std::min(d, D - 1) * C;
        for (int64_t c = 0; c < C; ++c) rel[(size_t)(c * Dpad + d)] = row[c];
      }
      for (int64_t b = 0; b < n_dblk; ++b) {
        for (int64_t c = 0; c < C; ++c) {
          int lo = INT32_MAX, hi = INT32_MIN;
          for (int64_t d = b * DB; d < (b + 1) * DB; ++d) {
            const int x = rel[(size_t)(c * Dpad + d)];
            lo = std::min(lo, x);
            hi = std::max(hi, x);
          }
          bmin[(size_t)(b * C + c)] = lo;
          bspan[(size_t)(b * C + c)] = hi - lo;
          max_span = std::max(max_span, hi - lo);
          mx = std::max(mx, hi);
          mn = std::min(mn, lo);
        }
      }
      // offsets relative to the block's minimum shift at each channel (what the
      // kernel adds to its LDS base): rel[c][d] = table[d][c] - bmin[d / DB][c]
      for (int64_t c = 0; c < C; ++c)
        for (int64_t d = 0; d < Dpad; ++d) rel[(size_t)(c * Dpad + d)] -= bmin[(size_t)((d / DB) * C + c)];
      if (il) {
        // meta[grp][dblk][c][DB + 4] = the DB shifts as LDS byte offsets in the
        // chunk buffer (16 x (shift - bmin + channel offset)), then {bmin, span,
        // channel offset (elements), c | channels in the chunk << 20}; chunks filled
        // greedily, channel order, up to CC channels or buf_e elements
        const int64_t ROWN = DB + 4;
        const int64_t Tq = 64 * v.G;
        const size_t moff = meta.size();
        meta.resize(moff + (size_t)(n_dblk * (C + 1) * ROWN), 0);
        const bool pairs = v.S == 8;  // the u16 kernel sums channel pairs
        for (int64_t b = 0; b < n_dblk && fits; ++b) {
          std::vector<int> list;
          int64_t c0 = 0, used = 0, ncc = 0;
          auto close = [&]() {
            for (int64_t c = c0; c < c0 + ncc; ++c)
              meta[moff + (size_t)((b * (C + 1) + c) * ROWN + DB + 3)] =
                  (int)((c < C ? c : (n_grp - grp) * C) | (ncc << 20));
            list.push_back((int)(c0 | (ncc << 20)));
          };
          // window of channel c (c == C: the pad channel, Tq elements of zeros)
          auto win_of = [&](int64_t c) -> int64_t {
            return (Tq + (c < C ? bspan[(size_t)(b * C + c)] : 0) + 63) / 64 * 64;
          };
          auto place = [&](int64_t c) {
            const size_t base = moff + (size_t)((b * (C + 1) + c) * ROWN);
            for (int64_t d = 0; d < DB; ++d)
              meta[base + d] = (int)(16 * ((c < C ? rel[(size_t)(c * Dpad + b * DB + d)] : 0) + used));
            meta[base + DB] = c < C ? bmin[(size_t)(b * C + c)] : 0;
            meta[base + DB + 1] = c < C ? bspan[(size_t)(b * C + c)] : 0;
            meta[base + DB + 2] = (int)used;
            used += win_of(c);
            ++ncc;
          };
          const int64_t step = pairs ? 2 : 1;
          for (int64_t c = 0; c < C; c += step) {
            const int64_t w = win_of(c) + (pairs ? win_of(c + 1) : 0);
            if (w > buf_e) { fits = false; break; }
            if (ncc + step > v.CC || used + w > buf_e) {
              close();
              c0 = c;
              used = 0;
              ncc = 0;
            }
            place(c);
            if (pairs) place(c + 1);  // c + 1 == C: the pad channel
          }
          if (fits) close();
          chunks.push_back(std::move(list));
        }
      }
    }  // groups
    // generic kernel: stride rounded to 16 elements, NBUF chunk buffers of
    // CC channels; interleaved kernel: NBUF packed buffers + the metadata ring
    const int64_t stride = il ? buf_e : v.stride_for(max_span);
    const int64_t need = il ? v.NBUF * buf_e * 16 + il_meta_bytes(v.NBUF, v.CC, v.DB())
                            : v.NBUF * v.chan_bytes(stride) * v.CC;
    if (il && (int64_t)max_span + 64 * v.G > (int64_t)1 << 20) continue;  // windows too wide
    if (il ? !fits : need > lds_budget(v) && !(last && need <= kLdsMax)) {
      if (last) return fail(err, "DM grid too sparse for one LDS tile (span " + std::to_string(max_span) + " bins)");
      continue;
    }
    plan = SweepPlan();
    static_cast<PlanDims&>(plan) = PlanDims{v, vi, dtype, n_grp, D, C, Dpad, n_dblk, max_span, (int)stride,
                                            (int)need, mx, mn};
    plan.bspan.swap(bspan);
    if (!il) {
      plan.rel.swap(rel);
      plan.bmin.swap(bmin);
      return 0;
    }
    // (+ 8 rows of zeros: the loaders' scalar loads of a chunk's window
    // rows read 8 rows from its first channel)
    meta.resize(meta.size() + (size_t)(8 * (DB + 4)), 0);
    plan.meta.swap(meta);
    size_t maxch = 0;
    for (const auto& l : chunks) maxch = std::max(maxch, l.size());
    plan.chunks.assign(chunks.size() * (maxch + 1), 0);
    for (size_t i = 0; i < chunks.size(); ++i) {
      plan.chunks[i * (maxch + 1)] = (int)chunks[i].size();
      for (size_t k = 0; k < chunks[i].size(); ++k) plan.chunks[i * (maxch + 1) + 1 + k] = chunks[i][k];
    }
    plan.maxch = (int)maxch;
    // 8/16-bit single-group sweeps: the factorised tables when they pay
    // groups of 4 channels, or of 2 where 4 do not fit or pay (the
    // cheaper by the cost model; PDD_SWEEP_FACTOR_G2 / _G4: that size only)
    // Factorised u16 plans first try their own 96-trial tiling
    // (kU8FxVariants: measured faster for factorised stage 2, slower for
    // the channel kernel), then the channel plan's tiling.
    if (!((flags & PDD_SWEEP_FACTOR) && n_grp == 1 && v.S == (dtype == PDD_F32 ? 4 : 8) &&
          il_instanced(v, true)))
      return 0;
    FxTables T, T2;
    const bool force = (flags & PDD_SWEEP_FACTOR_FORCE) != 0;
    const bool skew = (flags & PDD_SWEEP_NO_SKEW) == 0;
    int fxg = 0;
    std::vector<Variant> fc;
    if (v.S == 8)
      for (const Variant& x : kU8FxVariants)
        if (C * (dtype == PDD_U8 ? 255 : 1023) <= 255 * 32768 && il_instanced(x, true)) fc.push_back(x);
    fc.push_back(v);
    for (const Variant& f : fc) {
      const int64_t room_f = lds_budget(f) - il_meta_bytes(f.NBUF, f.CC, f.DB());
      const int64_t buf_f = std::max<int64_t>(0, room_f / (f.NBUF * 16) / 64 * 64);
      // (the pair order of the trial blocks is kept where it costs at most
      // PDD_FX_PAIR_MAX times the chunks on average, fx_build; the cost
      // screen may turn the plan down without the pair order: keep it then)
      auto build = [&](int g, FxTables& X) {
        if (!fx_build(host_table, D, C, f, buf_f, g, force, X, true, skew)) return false;
        const double ratio = X.pair_ratio;
        bool ok = true;
        if (ratio > PDD_FX_PAIR_MAX && !fx_build(host_table, D, C, f, buf_f, g, force, X, false, skew))
          ok = fx_build(host_table, D, C, f, buf_f, g, force, X, true, skew);
        X.pair_ratio = ratio;  // reported: what the pair order cost
        return ok;
      };
      if (!(flags & PDD_SWEEP_FACTOR_G2) && build(4, T)) fxg = 4;
      if (!(flags & PDD_SWEEP_FACTOR_G4) && build(2, T2) && (fxg == 0 || T2.cost_f < T.cost_f)) {
        fxg = 2;
        std::swap(T, T2);
      }
      if (!fxg) continue;
      // the plan runs the factorised tiling: its trial blocks, LDS
      plan.v = f;
      plan.n_dblk = cdiv(D, f.DB());
      plan.Dpad = plan.n_dblk * f.DB();
      plan.stride = (int)buf_f;
      plan.lds_bytes = (int)(f.NBUF * buf_f * 16 + il_meta_bytes(f.NBUF, f.CC, f.DB()));
      plan.fx = fxg;
      plan.n_pat = T.n_pat;
      plan.fx_rows = T.rows_pb;
      plan.fx_rspan = T.rspan;  // stage 1 sizes its LDS to it: more workgroups per CU
      plan.fx_lo = T.lo_f;
      plan.fx_hi = T.hi_f;
      plan.fx_tpad = (int)(cdiv(T.sig_max, 64 * f.G) * 64 * f.G);
      plan.fx_sig_max = T.sig_max;
      plan.maxch = T.maxch;
      plan.meta.swap(T.mt);
      plan.chunks.swap(T.cht);
      plan.fxt = std::move(T);
      break;
    }
    return 0;
  }
  return fail(err, "no variant");
}

}  // namespace pdd
