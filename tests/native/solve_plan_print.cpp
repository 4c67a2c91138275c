// solve_plan_print.cpp -- the solver's launch rules (is-vins_amd/csrc/isv_solve_plan.h) without a GPU: reads cases from stdin, one
// per line as key=value words, and prints for each the four ISV_DEBUG_PATH lines the library would print, then one line per plan
// with the fields those lines do not carry.  tests/test_solve_plan.py builds it under AddressSanitizer + UBSan and compares.
//
// keys (all integers; missing = 0, the tri-states default to -1 = unset):
//   case=<name>
//   N Nr est_ex n_prior_slots prior_H_sz max_lm max_batch                      the handle's shape (N: device frames = Nr + est_ex)
//   n_cus dogleg_per_cu_regs                                                  the device
//   sb st dense front st_ws cs                                                SolveSizes: build_solve_sb_bytes, build_solve_st_bytes,
//                                                                             build_solve_lds_bytes, front_lds_bytes, ..._st_ws_doubles, ..._cs_doubles
//   ISV_<HOOK>=1, ISV_SOLVE_ST / ISV_CHAIN_SPLIT = 0 | 1                       the environment
//   B Ftot Fmax Lmax n_tiles init_mode resident                               the upload
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include "../../is-vins_amd/csrc/isv_solve_plan.h"

static const char *role_name[KR_COUNT] = {"SOLVE", "CHAIN", "POSE", "LIN_GRAM_CHAIN", "LIN_GRAM_CHAIN_R1", "POSE_DOGLEG", "RANK1", "RANK1_SPLIT", "SCHUR_SPLIT",
                                          "LIN_GRAM", "LIN_GRAM_SMALL", "DOGLEG", "DOGLEG_CONTROL", "STEP_CONTROL", "SWEEP", "FRONT"};
static const char *inst_name[] = {"NONE", "PLAIN", "DENSE", "SB_N11", "SB_RT", "SB_BIG", "ST_N11", "ST_RT", "ST_N18", "ST_BIG", "LGC_N11", "LGC_RT", "LGC_BIG", "LGC_R1", "PD_N11", "PD_RT"};
static const char *role_or_none(SolverRole r) { return r == KR_COUNT ? "NONE" : role_name[r]; }

int main() {
    std::string line;
    char out[512];
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
        auto tri = [&](const char *k) { return kv.count(k) ? (kv[k] != 0 ? 1 : 0) : -1; };
        SolveShape s;
        s.N = (int)get("N"); s.Nr = (int)get("Nr"); s.est_ex = (int)get("est_ex"); s.n_prior_slots = (int)get("n_prior_slots");
        s.prior_H_sz = (int)get("prior_H_sz"); s.max_lm = (int)get("max_lm"); s.max_batch = (size_t)get("max_batch");
        SolveDevice dev;
        dev.n_cus = (int)get("n_cus"); dev.dogleg_per_cu_regs = (int)get("dogleg_per_cu_regs");
        SolveSizes z;
        z.build_solve_sb_bytes = (size_t)get("sb"); z.build_solve_st_bytes = (size_t)get("st"); z.build_solve_lds_bytes = (size_t)get("dense");
        z.front_lds_bytes = (size_t)get("front"); z.build_solve_st_ws_doubles = (size_t)get("st_ws"); z.build_solve_cs_doubles = (size_t)get("cs");
        SolveEnv e;
        e.one_stream = on("ISV_ONE_STREAM"); e.split_control = on("ISV_SPLIT_CONTROL"); e.generic_n = on("ISV_GENERIC_N");
        e.lg_batch_waves = on("ISV_LG_BATCH_WAVES"); e.debug_sw_global = on("ISV_DEBUG_SW_GLOBAL"); e.legacy_visual = on("ISV_LEGACY_VISUAL");
        e.no_split = on("ISV_NO_SPLIT"); e.no_update = on("ISV_DEBUG_NO_UPDATE"); e.no_pose_dogleg = on("ISV_NO_POSE_DOGLEG");
        e.marg_one_kernel = on("ISV_MARG_ONE_KERNEL"); e.marg_split = on("ISV_MARG_SPLIT"); e.tail_one_wave = on("ISV_TAIL_ONE_WAVE");
        e.r1_dense = on("ISV_R1_DENSE"); e.debug_path = true;
        e.solve_st = tri("ISV_SOLVE_ST"); e.chain_split = tri("ISV_CHAIN_SPLIT");
        UploadShape u;
        u.B = (int)get("B"); u.Ftot = (size_t)get("Ftot"); u.Fmax = (size_t)get("Fmax"); u.Lmax = (size_t)get("Lmax"); u.n_tiles = (int)get("n_tiles");
        u.est_ex = s.est_ex; u.init_mode = (int)get("init_mode"); u.resident = (int)get("resident");

        const HandlePlan h = plan_handle(s, e, dev, z);
        const UploadPlan p = plan_upload(h, dev, e, u);
        printf("case %s\n", name.c_str());
        plan_format_lds(out, sizeof(out), h); fputs(out, stdout);
        plan_format_solve_st(out, sizeof(out), h); fputs(out, stdout);
        plan_format_handle(out, sizeof(out), h, e); fputs(out, stdout);
        plan_format_enqueue(out, sizeof(out), p); fputs(out, stdout);
        printf("plan: handle wd_ld=%d tvis_sz=%d nt=%d lds_r1=%zu r1_dense=%d can_split=%d sw_global_ok=%d has_sw_part=%d chain_split=%d solve_st=%d split_cap=%d r1_groups=%zu marg_one=%d",
               h.wd_ld, h.tvis_sz, h.nt, h.lds_r1, (int)h.r1_dense, (int)h.can_split, (int)h.sw_global_ok, (int)h.has_sw_part, (int)h.chain_split, (int)h.solve_st, h.split_cap, h.r1_groups, (int)h.marg_one);
        for (int r = 0; r < KR_COUNT; r++)
            if (h.roles[r].inst != KI_NONE) printf(" %s=%s/%u/%zu", role_name[r], inst_name[h.roles[r].inst], h.roles[r].threads, h.roles[r].lds);
        printf("\n");
        printf("plan: upload fused_visual=%d fused_refusal=%d ctl_stage_lm=%d dg_stage_ph=%d sw_global=%d control_in_wg=%d GrMax=%d Gs=%d visual=%s/%zu sweep=%zu solve=%s/%zu "
               "backsub=%u/%zu dogleg=%s/%zu step_control=%zu prior=%zu/%zu proj=%zu/%zu grids=%u/%u/%u/%u/%u/%u/%u/%u finalize_wide=%d do_update=%d clear_marg=%d marg_bwd=%d marg_fwd_wide=%d\n",
               (int)p.fused_visual, (int)p.fused_refusal, (int)p.ctl_stage_lm, (int)p.dg_stage_ph, (int)p.sw_global, (int)p.control_in_wg, p.GrMax, p.Gs,
               role_or_none(p.visual_role), p.lds_visual, p.lds_sweep, role_or_none(p.solve_role), p.lds_solve, p.grid_backsub_y, p.lds_backsub,
               role_or_none(p.dogleg_role), p.lds_dogleg, p.lds_step_control, p.lds_prior, p.lds_prior_c, p.lds_proj, p.lds_proj_c,
               p.grid_init_state, p.grid_imu_raw, p.grid_imu_weight, p.grid_imu_c, p.grid_model, p.grid_tiles, p.grid_split_y, p.grid_fold_y,
               (int)p.finalize_wide, p.do_update, p.clear_marg, (int)p.marg_bwd, (int)p.marg_fwd_wide);
    }
    return 0;
}
