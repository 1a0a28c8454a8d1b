// Prints the fit schedule that sched_plan (corenav_gp_amd/csrc/cgp_sched_plan.hpp) decides for each line of its standard input.
// A line is a list of name=value words that set members of a default SchedIn (names below); the answer is one line per input.
// Built and driven by tests/test_sched_plan_cpu.py: includes the plan header and nothing else of the library.
#include "cgp_sched_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

using namespace cgp;

static bool set(SchedIn &in, const std::string &k, long long v) {
  if (k == "esz") in.esz = (int)v;
  else if (k == "batch") in.batch = (int)v;
  else if (k == "NT") in.NT = (int)v;
  else if (k == "ET") in.ET = (int)v;
  else if (k == "M") in.M = (int)v;
  else if (k == "xid") in.xid = v != 0;
  else if (k == "matern") in.matern = v != 0;
  else if (k == "in_rows") in.in_rows = v != 0;
  else if (k == "want_alpha") in.want_alpha = v != 0;
  else if (k == "prof") in.prof = v != 0;
  else if (k == "nstreams") in.nstreams = (int)v;
  else if (k == "lat_cap") in.lat_cap = (int)v;
  else if (k == "mid_cap") in.mid_cap = (int)v;
  else if (k == "lat_units") in.lat_units = (size_t)v;
  else if (k == "lat_img_fits") in.lat_img_fits = (int)v;
  else if (k == "lat_images_fit") in.lat_images_fit = v != 0;
  else if (k == "refine") in.refine = (int)v;
  else if (k == "refined") in.refined = v != 0;
  else if (k == "refine_bufs") in.refine_bufs = v != 0;
  else if (k == "refine_max_nt") in.refine_max_nt = (int)v;
  else if (k == "no_latency") in.sw.no_latency = v != 0;
  else if (k == "sw_split_diag") in.sw.split_diag = v != 0;
  else if (k == "fused_diag") in.sw.fused_diag = v != 0;
  else if (k == "overlap") in.sw.overlap = v != 0;
  else if (k == "fat_diag") in.sw.fat_diag = v != 0;
  else if (k == "acc_off") in.sw.acc_off = v != 0;
  else if (k == "sk_fused_trmm") in.sw.sk_fused_trmm = v != 0;
  else if (k == "one_launch") in.sw.one_launch = v != 0;
  else if (k == "lat_fits_env") in.lat_fits_env = (int)v;
  else if (k == "mid_fits_env") in.mid_fits_env = (int)v;
  else if (k == "xsplit32_env") in.xsplit32_env = (int)v;
  else if (k == "group0_env") in.group0_env = (int)v;
  else if (k == "sched_lag_env") in.sched_lag_env = (int)v;
  else if (k == "tuned_groups") in.tuned_groups = (int)v;
  else return false;
  return true;
}

int main() {
  static const char *names[] = {"Latency", "OneLaunch", "LookAhead", "Launches"};
  std::string line;
  while (std::getline(std::cin, line)) {
    SchedIn in;
    std::istringstream ws(line);
    std::string w;
    while (ws >> w) {
      const size_t eq = w.find('=');
      if (eq == std::string::npos || !set(in, w.substr(0, eq), atoll(w.c_str() + eq + 1))) {
        fprintf(stderr, "bad word: %s\n", w.c_str());
        return 2;
      }
    }
    const SchedPlan p = sched_plan(in);
    printf("%s mid=%d split_diag=%d xsplit=%d acc=%d trmm=%d tune=%d G=%d gb=", names[(int)p.sched], p.mid, p.split_diag, p.xsplit, p.use_acc,
           p.split_trmm, p.tune_eligible, p.G);
    for (int g = 0; g < p.G; ++g) printf("%s%d", g ? "," : "", p.gb[g]);
    printf(" alpha=%d refine=%d,%d,%d\n", p.want_alpha, p.rsteps, p.rsolve, p.ralpha_all);
  }
  return 0;
}
