// The sweep planner on the CPU: reads a raw int32 [n_grp][D][C] delay table
// and prints the finished plan as one JSON object -- status and message, every
// scalar, the factorised cost model's figures and an FNV-1a digest of each
// table the library would upload (tests/test_sweep_plan.py compares them with
// tests/golden/golden_sweep_plans.json).  Plain C++, no HIP, no GPU:
//   c++ -x c++ -std=c++17 -O3 -ffp-contract=off -Ipypulsar_amd/csrc -o build/plan_dump \
//       tests/native/plan_dump.cpp pypulsar_amd/csrc/pdd_sweep_plan.hip
//   build/plan_dump table.bin n_grp D C dtype flags
// (dtype: PDD_F32 / PDD_U8 / PDD_U16 = 0 / 1 / 2; flags: PDD_SWEEP_*, e.g. 3 =
// forced factorisation, 19 = the same with plane-aligned tiles)
#include <cstdio>
#include <cstdlib>

#include "sweep_plan.h"

static void vec(const char* name, const std::vector<int>& v, const char* sep = ", ") {
  uint64_t h = 1469598103934665603ull;  // FNV-1a, 64 bits, over the bytes
  const unsigned char* b = reinterpret_cast<const unsigned char*>(v.data());
  for (size_t i = 0; i < v.size() * sizeof(int); ++i) h = (h ^ b[i]) * 1099511628211ull;
  printf("\"%s\": {\"n\": %zu, \"fnv\": \"%016llx\"}%s", name, v.size(), (unsigned long long)h, sep);
}

int main(int argc, char** argv) {
  if (argc < 7) {
    fprintf(stderr, "usage: plan_dump table.bin n_grp D C dtype flags\n");
    return 2;
  }
  const int64_t n_grp = atoll(argv[2]), D = atoll(argv[3]), C = atoll(argv[4]);
  const int dtype = atoi(argv[5]), flags = atoi(argv[6]);
  if (n_grp < 1 || D < 1 || C < 1) return 2;
  std::vector<int32_t> tab((size_t)(n_grp * D * C));
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(tab.data(), 4, tab.size(), f) != tab.size()) {
    fprintf(stderr, "plan_dump: cannot read %zu shifts from %s\n", tab.size(), argv[1]);
    return 2;
  }
  fclose(f);
  pdd::SweepPlan p;
  std::string err, msg;
  const int st = pdd::plan_sweep(tab.data(), n_grp, D, C, dtype, flags, p, err);
  for (char c : err) {
    if (c == '"' || c == '\\') msg += '\\';
    msg += c;
  }
  printf("{\"status\": %d, \"message\": \"%s\"", st, msg.c_str());
  if (st == 0) {
    printf(", \"variant\": %d, \"DB\": %d, \"TB\": %d, \"Dpad\": %lld, \"n_dblk\": %lld, \"max_span\": %d, "
           "\"stride\": %d, \"lds_bytes\": %d, \"min_bin\": %d, \"max_bin\": %d, \"maxch\": %d, \"fx\": %d, "
           "\"n_pat\": %lld, \"fx_rows\": %lld, \"fx_rspan\": %d, \"fx_lo\": %d, \"fx_hi\": %d, "
           "\"fx_tpad\": %d, \"sig_max\": %d, \"gtab_empty\": %s, ",
           p.vi, p.v.DB(), p.v.TB(), (long long)p.Dpad, (long long)p.n_dblk, p.max_span, p.stride,
           p.lds_bytes, p.min_bin, p.max_bin, p.maxch, p.fx, (long long)p.n_pat, (long long)p.fx_rows,
           p.fx_rspan, p.fx_lo, p.fx_hi, p.fx_tpad, p.fx_sig_max, p.fxt.gtab.empty() ? "true" : "false");
    printf("\"cost_f\": %.17g, \"cost_b\": %.17g, \"el_f\": %.17g, \"el_b\": %.17g, \"pair_ratio\": %.17g, "
           "\"tables\": {", p.fxt.cost_f, p.fxt.cost_b, p.fxt.el_f, p.fxt.el_b, p.fxt.pair_ratio);
    vec("rel", p.rel);
    vec("bmin", p.bmin);
    vec("meta", p.meta);
    vec("chunks", p.chunks);
    vec("bspan", p.bspan);
    vec("pat", p.fxt.pat);
    vec("wt", p.fxt.wt);
    vec("gtab", p.fxt.gtab);
    vec("sig", p.fxt.sig, "}");
  }
  printf("}\n");
  return 0;
}
