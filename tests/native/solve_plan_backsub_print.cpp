// solve_plan_backsub_print.cpp -- where the landmark back-substitution runs (UploadPlan::bsub_in_solve, is-vins_amd/csrc/isv_solve_plan.h)
// without a GPU: reads cases from stdin, one per line as key=value words in solve_plan_print.cpp's vocabulary (the keys this rule does
// not look at are accepted and ignored), and prints one line per case with the field and the five conditions it is made of.
// tests/test_solve_plan_backsub.py builds it under AddressSanitizer + UBSan and compares.
//
// keys (integers; missing = 0, ISV_SOLVE_ST defaults to -1 = unset):
//   case=<name>
//   N Nr est_ex n_prior_slots prior_H_sz max_lm max_batch        the handle's shape (N: device frames = Nr + est_ex)
//   n_cus dogleg_per_cu_regs                                    the device
//   sb st dense front st_ws cs                                  SolveSizes
//   ISV_BSUB_IN_DOGLEG=1, ISV_LEGACY_VISUAL=1, ISV_NO_SPLIT=1, ISV_GENERIC_N=1, ISV_SOLVE_ST = 0 | 1
//   B Ftot Fmax Lmax n_tiles resident                           the upload
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include "../../is-vins_amd/csrc/isv_solve_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::map<std::string, long long> kv;
        std::string name = "?", word;
        std::istringstream words(line);
        while (words >> word) {
            const size_t eq = word.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "not key=value: %s\n", word.c_str()); return 2; }
            if (word.substr(0, eq) == "case") name = word.substr(eq + 1);
            else kv[word.substr(0, eq)] = atoll(word.c_str() + eq + 1);
        }
        if (kv.empty()) continue;
        auto get = [&](const char *k) { auto it = kv.find(k); return it == kv.end() ? 0ll : it->second; };
        auto on = [&](const char *k) { return kv.count(k) != 0; };
        SolveShape s;
        s.N = (int)get("N"); s.Nr = (int)get("Nr"); s.est_ex = (int)get("est_ex"); s.n_prior_slots = (int)get("n_prior_slots");
        s.prior_H_sz = (int)get("prior_H_sz"); s.max_lm = (int)get("max_lm"); s.max_batch = (size_t)get("max_batch");
        SolveDevice dev;
        dev.n_cus = (int)get("n_cus"); dev.dogleg_per_cu_regs = (int)get("dogleg_per_cu_regs");
        SolveSizes z;
        z.build_solve_sb_bytes = (size_t)get("sb"); z.build_solve_st_bytes = (size_t)get("st"); z.build_solve_lds_bytes = (size_t)get("dense");
        z.front_lds_bytes = (size_t)get("front"); z.build_solve_st_ws_doubles = (size_t)get("st_ws"); z.build_solve_cs_doubles = (size_t)get("cs");
        SolveEnv e;
        e.bsub_in_dogleg = on("ISV_BSUB_IN_DOGLEG"); e.legacy_visual = on("ISV_LEGACY_VISUAL"); e.no_split = on("ISV_NO_SPLIT"); e.generic_n = on("ISV_GENERIC_N");
        e.solve_st = kv.count("ISV_SOLVE_ST") ? (kv["ISV_SOLVE_ST"] != 0 ? 1 : 0) : -1;
        UploadShape u;
        u.B = (int)get("B"); u.Ftot = (size_t)get("Ftot"); u.Fmax = (size_t)get("Fmax"); u.Lmax = (size_t)get("Lmax"); u.n_tiles = (int)get("n_tiles");
        u.est_ex = s.est_ex; u.resident = (int)get("resident");

        const HandlePlan h = plan_handle(s, e, dev, z);
        const UploadPlan p = plan_upload(h, dev, e, u);
        printf("case %s bsub_in_solve=%d solve_st=%d fused=%d threads=%u est_ex=%d bsub_split=%d hook=%d solve=%d\n", name.c_str(), (int)p.bsub_in_solve,
               (int)h.solve_st, (int)p.fused, h.roles[KR_SOLVE].threads, s.est_ex, (int)p.bsub_split, (int)e.bsub_in_dogleg, (int)h.roles[KR_SOLVE].inst);
    }
    return 0;
}
