// Stand-alone host program over csrc/spx_plan.h alone (no HIP, no library): reads one case per line from stdin and prints
// the plan as one JSON line (tests/test_plan.py, tests/test_gpu_r_plan_runs.py).
//   factor N= D= H= [time=1] [lean=1] [defer=1] [dest=1] [demoted=1] [rhs_rows=1] [Np=] [OPTION=value ...]
//   ei     N= M= D= H= [S=] [nmodels=] [flags=] [pending=1] [fant_budget=] [ring_budget=] [Np=] [OPTION=value ...]
// OPTION is a name spx_set_option takes, the value what it stores (tri-states -1 / 0 / 1).  Np defaults to the handle's
// (N padded to 128), the K(X*,X) budget to option kstar_budget_bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "../../spearmint_amd/csrc/spx_plan.h"

static bool set_option(Options& o, const std::string& k, int64_t v)
{
    static const std::map<std::string, int Options::*> ints = {
        {"gemm_waves", &Options::gemm_variant}, {"covar", &Options::cov_kind}, {"streams", &Options::nstreams},
        {"kstar_ring", &Options::ring_opt}, {"kstar_corun", &Options::corun_opt},
        {"flow_rearm_after", &Options::flow_rearm_after}, {"flow_spin_limit", &Options::flow_spin_limit},
        {"lean_lazy", &Options::lean_lazy}, {"step_overlap", &Options::step_overlap}, {"ei_fused", &Options::ei_fused},
        {"ei_flow", &Options::ei_flow}, {"lean_flow_cov", &Options::lean_flow_cov},
        {"lean_flow_yield", &Options::lean_flow_yield}, {"lean_flow_cu", &Options::lean_flow_cu},
        {"lean_flow", &Options::lean_flow}, {"lean_ps", &Options::lean_ps}, {"lean_merge", &Options::lean_merge},
        {"lean_one", &Options::lean_one}, {"lean_poll", &Options::lean_poll}, {"lean_zc", &Options::lean_zc},
        {"stage_copies", &Options::stage_copies}, {"cov_flat", &Options::cov_flat}, {"gemm_partial", &Options::gemm_partial}};
    if (k == "kstar_budget_bytes") { o.kst_budget = v; return true; }
    if (k == "timing") { o.timing = v != 0; return true; }
    auto it = ints.find(k);
    if (it == ints.end()) return false;
    o.*(it->second) = (int)v;
    return true;
}

#define J(f) printf("\"" #f "\": %lld, ", (long long)p.f)

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind, tok;
        if (!(in >> kind)) continue;
        std::map<std::string, int64_t> kv;
        Options o;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "plan_client: bad token '%s'\n", tok.c_str()); return 2; }
            const std::string k = tok.substr(0, eq);
            const int64_t v = strtoll(tok.c_str() + eq + 1, nullptr, 0);
            if (!set_option(o, k, v)) kv[k] = v;
        }
        auto get = [&](const char* k, int64_t dflt) { auto it = kv.find(k); if (it == kv.end()) return dflt; int64_t v = it->second; kv.erase(it); return v; };
        if (kind == "factor") {
            FactorShape s;
            s.N = get("N", 1); s.D = (int)get("D", 1); s.H = (int)get("H", 1);
            s.Np = (int)get("Np", round_up(s.N, SPX_PADN));
            s.have_time = get("time", 0); s.lean = get("lean", 0); s.defer_sync = get("defer", 0); s.have_dest = get("dest", 0);
            s.flow_demoted = get("demoted", 0); s.rhs_rows_on = get("rhs_rows", 0);
            const FactorPlan p = plan_factor(o, s);
            printf("{");
            J(lean); J(nm); J(nh); J(Np); J(nblk); J(Dp); J(hs); J(rl); J(flow); J(tiled); J(flow_alone); J(yield);
            J(cov_in_flow); J(lazy); J(ps); J(merged_prologue); J(fused); J(zero_copy); J(poll); J(zero_in_kernel); J(bracket); J(step);
            J(fused_items); J(vstride); J(nfl); J(hyp_doubles); J(xs_bytes); J(vec_bytes); J(nn_bytes); J(dinv_bytes);
            J(info_bytes); J(ps_bytes); J(rhs_bytes); J(diagL_bytes);
            printf("\"kind\": \"factor\"}\n");
        } else if (kind == "ei") {
            EiShape s;
            s.N = get("N", 1); s.M = get("M", 1); s.D = (int)get("D", 1); s.H = (int)get("H", 1); s.S = (int)get("S", 0);
            s.Np = (int)get("Np", round_up(s.N, SPX_PADN));
            s.nmodels = (int)get("nmodels", 1); s.flags = (int32_t)get("flags", 0); s.factor_pending = get("pending", 0);
            s.kst_budget = o.kst_budget; s.fant_budget = get("fant_budget", 0); s.ring_budget = get("ring_budget", 0);
            const EiPlan p = plan_ei(o, s);
            printf("{");
            J(per_sec); J(keep_mom); J(time_only); J(constrained); J(Mp); J(Mc); J(Hb); J(nrb); J(Dp); J(fused); J(gemm_path);
            J(timing_on); J(ns); J(kst_bufs); J(slots); J(ringed); J(slot_bytes); J(R); J(ring_items); J(trim_ring); J(overlap);
            J(cov_flat); J(corun); J(gemm_nlive); J(cov_live_rows); J(n_info); J(cs_bytes); J(s2_bytes); J(kst_bytes);
            J(bgS_bytes); J(part_bytes); J(scratch_bytes); J(draw_bytes); J(mean_bytes);
            printf("\"kind\": \"ei\"}\n");
        } else {
            fprintf(stderr, "plan_client: unknown case kind '%s'\n", kind.c_str());
            return 2;
        }
        if (!kv.empty()) { fprintf(stderr, "plan_client: unknown key '%s'\n", kv.begin()->first.c_str()); return 2; }
    }
    return 0;
}
