// The launch planners of whisperkit_amd/csrc/launch_plan.h (the SAME header the launchers include) behind a line protocol, built with g++ and
// driven by tests/test_kernel_harness.py and tests/test_launch_plan.py.  One request per stdin line, one answer per stdout line:
//   gemm M N K lda a_batch_stride ldc d_model epi split out_bases epi_mode no256 persist persist_wgs cus  ->  <kernel label> grid <x> <y>
//   ln d f32_bases y16 y16_lo has_lo v4                                                                ->  <kernel label>
//   dec32 mode N K n_bt [WH_D32_<NAME>=<value> ...]                                                    ->  ks tw rt tc ntw grid
//   xatt n_head forced_passes                                                                          ->  passes splits
//   self self_rows                                                                                     ->  passes
//   xabs d n_head max_batch batch spw n_split n_bt              ->  supported auto_width auto_splits attn_grid vup_ks vup_grid
//   knob NAME [value]                     (sets / unsets the variable in this process, then parses it)    ->  knobs.h value_of
// Knob values a line does not name are the defaults of csrc/knobs.h (the table, never the environment).
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "knobs.h"
#include "launch_plan.h"

using namespace wh;

static int dflt(knob::Id k) { return knob::kTable[k].dflt; }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "gemm") {
            long long M, N, K, lda, stride, ldc, d_model, epi, split, bases;
            plan::GemmKnobs k{};
            in >> M >> N >> K >> lda >> stride >> ldc >> d_model >> epi >> split >> bases >> k.epi_mode >> k.no256 >> k.persist >> k.persist_wgs >> k.cus;
            if (!in) { std::printf("ERROR %s\n", line.c_str()); return 1; }
            const plan::GemmPlan p = plan::gemm_plan((int)M, (int)N, (int)K, (int)lda, stride, (int)ldc, (int)d_model, (int)epi, split != 0, (uintptr_t)bases, k);
            const char* sp = split ? "_split" : "";
            if (p.family == plan::GEMM_256) std::printf("gemm256%s_kernel<mode %d>", sp, p.mode);
            else if (p.family == plan::GEMM_256P) std::printf("gemm256p_kernel<mode %d>", p.mode);
            else std::printf("gemm%s_kernel<%s>", sp, p.family == plan::GEMM_128 ? "128,128" : "64,64");
            std::printf(" grid %u %u\n", p.grid_x, p.grid_y);
        } else if (what == "ln") {
            long long d, f32_bases, y16, y16_lo, has_lo, v4;
            in >> d >> f32_bases >> y16 >> y16_lo >> has_lo >> v4;
            if (!in) { std::printf("ERROR %s\n", line.c_str()); return 1; }
            const plan::LnKernel w = plan::layernorm_plan((int)d, (uintptr_t)f32_bases, (uintptr_t)y16, (uintptr_t)y16_lo, has_lo != 0, (int)v4);
            std::printf("%s\n", w == plan::LN_V4_NT ? "layernorm_v4_kernel<NT>" : w == plan::LN_V4 ? "layernorm_v4_kernel" : "layernorm_kernel");
        } else if (what == "dec32") {
            int mode, N, K, n_bt;
            in >> mode >> N >> K >> n_bt;
            if (!in) { std::printf("ERROR %s\n", line.c_str()); return 1; }
            using namespace knob;
            plan::Dec32Knobs k{dflt(WH_D32_KS_RESID), dflt(WH_D32_KS_FC2), dflt(WH_D32_KS_Q), dflt(WH_D32_KS_WIDE), dflt(WH_D32_TILE_KB), dflt(WH_D32_TC),
                               dflt(WH_D32_TC_BT), dflt(WH_D32_RT2_TC), dflt(WH_D32_NTW), dflt(WH_D32_RT_BT), dflt(WH_D32_RT4_BT), dflt(WH_D32_RT4_MODES)};
            const struct { const char* name; int* v; } named[] = {
                {"WH_D32_KS_RESID", &k.ks_resid}, {"WH_D32_KS_FC2", &k.ks_fc2}, {"WH_D32_KS_Q", &k.ks_q}, {"WH_D32_KS_WIDE", &k.ks_wide}, {"WH_D32_TILE_KB", &k.tile_kb},
                {"WH_D32_TC", &k.tc}, {"WH_D32_TC_BT", &k.tc_bt}, {"WH_D32_RT2_TC", &k.rt2_tc}, {"WH_D32_NTW", &k.ntw}, {"WH_D32_RT_BT", &k.rt_bt},
                {"WH_D32_RT4_BT", &k.rt4_bt}, {"WH_D32_RT4_MODES", &k.rt4_modes}};
            std::string kv;
            while (in >> kv) {
                const size_t eq = kv.find('=');
                bool found = false;
                for (const auto& n : named)
                    if (eq != std::string::npos && kv.compare(0, eq, n.name) == 0) { *n.v = std::atoi(kv.c_str() + eq + 1); found = true; }
                if (!found) { std::printf("ERROR unknown knob %s\n", kv.c_str()); return 1; }
            }
            const plan::Dec32Plan p = plan::dec32_plan(mode, N, K, n_bt, k);
            std::printf("%d %d %d %d %d %u\n", p.ks, p.tw, p.rt, p.tc, p.ntw ? 1 : 0, p.grid);
        } else if (what == "xatt") {
            int n_head, forced;
            in >> n_head >> forced;
            const plan::CrossAttnPlan p = plan::cross_attn_plan(n_head, forced, 1500);
            std::printf("%d %d\n", p.passes, p.splits);
        } else if (what == "self") {
            int rows;
            in >> rows;
            std::printf("%d\n", plan::self_attn_passes(rows));
        } else if (what == "xabs") {
            int d, n_head, max_batch, batch, spw, n_split, n_bt;
            in >> d >> n_head >> max_batch >> batch >> spw >> n_split >> n_bt;
            const plan::XabsVupPlan v = plan::xabs_vup_plan(d, n_head, n_bt);
            std::printf("%d %d %d %u %d %u\n", plan::xabs_supported(d, n_head) ? 1 : 0, plan::xabs_auto_width(d, n_head) ? 1 : 0, plan::xabs_auto_splits(max_batch),
                        plan::xabs_attn_grid(batch, spw, n_split), v.ks, v.grid);
        } else if (what == "knob") {
            std::string name, value;
            in >> name;
            int id = -1;
            for (int i = 0; i < knob::kCount; ++i) if (name == knob::kTable[i].name) id = i;
            if (id < 0 || knob::kTable[id].parse == knob::STR) { std::printf("ERROR %s\n", line.c_str()); return 1; }
            if (in >> value) setenv(name.c_str(), value.c_str(), 1); else unsetenv(name.c_str());
            std::printf("%d\n", knob::value_of((knob::Id)id));
        } else {
            std::printf("ERROR %s\n", line.c_str());
            return 1;
        }
    }
    return 0;
}
