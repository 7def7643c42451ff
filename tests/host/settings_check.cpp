// settings_check.cpp — host-only check of csrc/settings.cpp (tests/test_settings_host.py compiles and runs it; no HIP, no GPU).
//
// For every MLP_* knob of the engine the variable is set to each of: unset, "", "0", "1", "2", "-1", "abc" (and to values beyond each
// clamp, and in the coupled combinations), Settings::from_env() is called, and EVERY field is compared with the table below: the
// knob's own field (and the fields coupled to it) with the listed value, every other field with its default.
//
// The table was transcribed BY HAND from the commit before settings.cpp existed (1c178a7), where each knob was parsed at its point of
// use; the comment of each row cites that place (file:line of that commit) and the rule found there.  It is not derived from
// settings.cpp: a parse rule that changed on the way shows up here.  atoi("") = atoi("abc") = 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "settings.h"

using mlp::Settings;

static const double U64_MINUS_1 = 18446744073709551615.0;  // (uint64_t)atoll("-1")

struct Row {
    const char* env;    // the variable
    const char* field;  // the field of Settings it decides (a variable with coupled fields has one row per field)
    double (*get)(const Settings&);
    double want[7];  // unset, "", "0", "1", "2", "-1", "abc"
};
static const char* const VALUES[7] = {nullptr, "", "0", "1", "2", "-1", "abc"};

#define F(name) #name, [](const Settings& s) { return (double)s.name; }
// the recurring rules
#define PRESENCE {0, 1, 1, 1, 1, 1, 1}  // != nullptr
#define NOT_ZERO {1, 1, 0, 1, 1, 1, 1}  // !(e && e[0] == '0')
static const Row ROWS[] = {
    {"MLP_NO_GRAPH", F(use_graph), {1, 1, 1, 0, 1, 1, 1}},                  // engine.hip:74-75   use_graph = !(ng && ng[0] == '1')
    {"MLP_BATCH", F(batch), {32, 1, 1, 1, 2, 1, 1}},                        // engine.hip:119-120 max(1, min(RING = 64, atoi)); engine.h:588 default 32
    {"MLP_GRAPH_ITERS", F(graph_iters), {10, 1, 1, 1, 2, 1, 1}},            // engine.hip:121-122 max(1, min(32, atoi)); engine.h:595 default 10
    {"MLP_DEBUG_SYNC", F(debug_sync), PRESENCE},                            // engine.hip:1638    getenv != nullptr (static)
    {"MLP_KPROF", F(kprof), {0, 0, 0, 1, 2, -1, 0}},                        // engine.hip:1391    set ? atoi : 0
    {"MLP_HYPER_PROF", F(hyper_prof), PRESENCE},                            // kernels.hip:5177   getenv != nullptr
    {"MLP_PUMP_DEBUG", F(pump_debug), PRESENCE},                            // engine.hip:1034    getenv != nullptr (static)
    {"MLP_BANDED", F(banded_mode), {-1, 0, 0, 1, 1, 1, 0}},                 // engine.hip:86-87   if set: atoi != 0 ? 1 : 0; engine.h:494 default -1
    {"MLP_DETERMINISTIC", F(det_mode), {-1, 0, 0, 1, 1, 1, 0}},             // engine.hip:84-85   the same; engine.h:493 default -1
    {"MLP_LAZY_DSE", F(lazy_dse), NOT_ZERO},                                // engine.hip:93-94   !(lz && lz[0] == '0')
    {"MLP_LOWRANK", F(lr_force), {-1, 0, 0, 1, 2, 0, 0}},                   // engine.hip:78-79   max(0, min(LR_MAX = 32, atoi)); engine.h:521 default -1
    {"MLP_BIGTILE", F(force_big_tiles), {0, 0, 0, 1, 1, 1, 0}},             // engine.hip:82-83   bt && atoi != 0
    {"MLP_LDPAD", F(ld_pad), {16, 0, 0, 0, 2, 0, 0}},                       // engine.hip:80-81   max(0, min(4096, atoi)) & ~1; engine.h:518 default 16
    {"MLP_STREAM_BALANCED", F(sw_balanced), {1, 0, 0, 1, 2, -1, 0}},        // engine.hip:102     atoi; engine.h:525 default 1
    {"MLP_FPULL", F(fpull), NOT_ZERO},                                      // engine.hip:116     if set: fp[0] != '0'; engine.h:507 default true
    {"MLP_PB_DET", F(pb_det), {-1, 0, 0, 1, 2, -1, 0}},                     // engine.hip:483     set ? atoi : -1 (static)
    {"MLP_TK_RIDE", F(tk_ride), NOT_ZERO},                                  // kernels.hip:5257-5258 off iff e && e[0] == '0'
    {"MLP_RK_RIDE", F(rk_ride), NOT_ZERO},                                  // kernels.hip:5576-5577
    {"MLP_RATIO_LIST", F(ratio_list), NOT_ZERO},                            // kernels.hip:5307-5308
    {"MLP_RATIO_LIST_CAP", F(ratio_list_cap), {8, 0, 0, 1, 2, 0, 0}},       // kernels.hip:5309-5310 cp ? max(0, min(RL_CAP = 8, atoi)) : RL_CAP
    {"MLP_BTRAN_RIDE", F(btran_ride), NOT_ZERO},                            // kernels.hip:5316-5317
    {"MLP_V_RIDE", F(v_ride), NOT_ZERO},                                    // kernels.hip:5323-5324
    {"MLP_RATIO_ONE", F(ratio_one), NOT_ZERO},                              // kernels.hip:5252-5253
    {"MLP_RATIO_TWO_KERNELS", F(ratio_two), PRESENCE},                      // engine.hip:95      getenv != nullptr
    {"MLP_RATIO_SPIN_LIMIT", F(ratio_spin_limit), {20000000, 0, 0, 1, 2, -1, 0}},  // engine.hip:101 atoll; engine.h:366 default 20000000
    {"MLP_STR_K", F(str_kmax), {230, 0, 0, 1, 2, -1, 0}},                   // engine.hip:99      atoi; engine.h:369 default 230
    {"MLP_SMALL_BASIS", F(small_basis), NOT_ZERO},                          // kernels.hip:5439-5440
    {"MLP_SMALL_BASIS_K", F(sb_kmax), {160, 0, 0, 1, 2, 0, 0}},             // engine.hip:98      max(0, min(256, atoi)); engine.h:370 default 160
    {"MLP_PRIMAL_HEAD", F(primal_head), NOT_ZERO},                          // kernels.hip:5454-5455
    {"MLP_PRIMAL_HEAD_K", F(ph_kmax), {-1, 0, 0, 1, 2, 0, 0}},              // engine.hip:97      max(0, atoi); engine.h:375 default -1
    {"MLP_PULL_INSIDE", F(pull_inside), NOT_ZERO},                          // kernels.hip:5625-5626
    {"MLP_HEAD_APPLY", F(head_apply), NOT_ZERO},                            // kernels.hip:5631-5632
    {"MLP_HYPER", F(hyper_mode), {-1, 0, 0, 1, 1, 0, 0}},                   // engine.hip:96      atoi > 0 ? 1 : 0; engine.h:381 default -1
    {"MLP_HYPER_HEAVY", F(hyper_heavy), {0, 0, 0, 1, 2, -1, 0}},            // engine.hip:100     atol; engine.h:382 default 0
    {"MLP_ORDER_FROM", F(order_from), {4096, 0, 0, 1, 2, U64_MINUS_1, 0}},  // engine.hip:91      (uint64_t)atoll; engine.h:490 default 4096
    {"MLP_ORDER_EVERY", F(order_every), {2048, 0, 0, 1, 2, U64_MINUS_1, 0}},  // engine.hip:92    (uint64_t)atoll; engine.h:488 default 2048
    {"MLP_SWEEP_PACKED", F(use_pack), NOT_ZERO},                            // engine.hip:90      if set: sp[0] != '0'; engine.h:482 default true
    {"MLP_REFRESH_TOL", F(refresh_tol), {1e-7, 0, 0, 1, 2, -1, 0}},         // engine.hip:76-77   atof; engine.h:569 default 1e-7
    {"MLP_FINAL_REFRESH", F(final_refresh_pivots), {50000, 0, 0, 1, 2, -1, 0}},  // engine.hip:88-89 atol; engine.h:589 default 50000
    {"MLP_REINVERT_GJ", F(reinvert_gj), PRESENCE},                          // engine.hip:3253    getenv != nullptr (static)
    {"MLP_FACTOR", F(fac_mode), {-1, 0, 0, 1, 1, 0, 0}},                    // engine.hip:103     atoi > 0 ? 1 : 0; engine.h:392 default -1
    {"MLP_FACTOR_FROM", F(fac_auto_cap), {8192, 256, 256, 256, 256, 256, 256}},  // engine.hip:108 max(256, atoi); engine.h:399 default 8192
    {"MLP_FACTOR_BUMP", F(fac_bump_max), {1024, 0, 0, 1, 2, 0, 0}},         // engine.hip:109-111 max(0, min(FAC_BMAX = 1024, want)); engine.h:419
    {"MLP_FACTOR_BUMP", F(fac_sb_max), {4096, 0, 0, 1, 2, 0, 0}},           // engine.hip:112     want < FAC_BMAX: min(fac_sb_max, fac_bump_max)
    {"MLP_FACTOR_SB", F(fac_sb_max), {4096, 0, 0, 1, 2, 0, 0}},             // engine.hip:114     max(0, min(FAC_SB_MAX = 4096, atoi)); engine.h:422
    {"MLP_FACTOR_SB_FROM", F(fac_sb_from), {48, 1, 1, 1, 2, 1, 1}},         // engine.hip:115     max(1, atoi); engine.h:423 default 48
    {"MLP_FACTOR_J", F(fac_J), {64, 1, 1, 1, 2, 1, 1}},                     // engine.hip:104-105 fac_J_ = fac_period_ = max(1, min(64, atoi)); engine.h:395
    {"MLP_FACTOR_J", F(fac_period), {48, 1, 1, 1, 2, 1, 1}},                // ... engine.h:396 default 48
    {"MLP_FACTOR_J", F(fac_period_auto), {1, 0, 0, 0, 0, 0, 0}},            // engine.hip:106     fac_period_auto_ = false; engine.h:397 default true
    {"MLP_FACTOR_FUSE", F(fac_fuse), NOT_ZERO},                             // engine.hip:1452    !(e && e[0] == '0') (static)
    {"MLP_FACTOR_RHO_PART", F(fac_rho_part), NOT_ZERO},                     // engine.hip:1453    the same (static)
    {"MLP_TRANSPORT", "transport.size", [](const Settings& s) { return (double)s.transport.size(); }, {0, 0, 1, 1, 1, 2, 3}},  // engine.hip:1089 the string itself
    {"MLP_SHARD_DEFER", F(shard_defer), NOT_ZERO},                          // engine.hip:1240-1241 !(sd && sd[0] == '0')
    {"MLP_NO_WSHARD", F(no_wshard), {0, 0, 0, 1, 1, 1, 0}},                 // engine.hip:117-118 nws && atoi != 0
    {"MLP_FACTOR_SHARED_DEVICE", F(fac_shared_device), {0, 0, 0, 1, 0, 0, 0}},  // engine.hip:2493 e && e[0] == '1' (static)
    {"MLP_TEST_GOLIVE_SKEW", F(golive_skew), {-1, 0, 0, 1, 2, -1, 0}},      // engine.hip:962-963 sk && atoi(sk) == shard_rank (ranks are >= 0: -1 matches none)
};
static const size_t NROWS = sizeof(ROWS) / sizeof(ROWS[0]);

// values beyond each clamp, and the coupled knobs in combination: {variable = value [, variable2 = value2]} -> field == want
struct Extra {
    const char *env, *val, *env2, *val2, *field;
    double want;
};
static const Extra EXTRAS[] = {
    {"MLP_BATCH", "1000", nullptr, nullptr, "batch", 64},
    {"MLP_GRAPH_ITERS", "1000", nullptr, nullptr, "graph_iters", 32},
    {"MLP_LOWRANK", "1000", nullptr, nullptr, "lr_force", 32},
    {"MLP_LDPAD", "100000", nullptr, nullptr, "ld_pad", 4096},
    {"MLP_LDPAD", "7", nullptr, nullptr, "ld_pad", 6},  // & ~1
    {"MLP_LDPAD", "-7", nullptr, nullptr, "ld_pad", 0},
    {"MLP_RATIO_LIST_CAP", "1000", nullptr, nullptr, "ratio_list_cap", 8},
    {"MLP_SMALL_BASIS_K", "1000", nullptr, nullptr, "sb_kmax", 256},
    {"MLP_PRIMAL_HEAD_K", "-1000", nullptr, nullptr, "ph_kmax", 0},
    {"MLP_PRIMAL_HEAD_K", "100000", nullptr, nullptr, "ph_kmax", 100000},  // (no upper clamp at the parse: run_loop takes the min with the kernel's bound)
    {"MLP_FACTOR_FROM", "100000", nullptr, nullptr, "fac_auto_cap", 100000},
    {"MLP_FACTOR_SB_FROM", "-1000", nullptr, nullptr, "fac_sb_from", 1},
    {"MLP_FACTOR_SB", "100000", nullptr, nullptr, "fac_sb_max", 4096},
    {"MLP_FACTOR_J", "1000", nullptr, nullptr, "fac_J", 64},
    {"MLP_FACTOR_J", "1000", nullptr, nullptr, "fac_period", 64},
    {"MLP_FACTOR_J", "1000", nullptr, nullptr, "fac_period_auto", 0},
    {"MLP_FACTOR_J", "8", nullptr, nullptr, "fac_period", 8},
    // MLP_FACTOR_BUMP at or above the dense carrier's capacity leaves the sparse carrier's limit alone (engine.hip:112)
    {"MLP_FACTOR_BUMP", "5000", nullptr, nullptr, "fac_bump_max", 1024},
    {"MLP_FACTOR_BUMP", "5000", nullptr, nullptr, "fac_sb_max", 4096},
    {"MLP_FACTOR_BUMP", "1024", nullptr, nullptr, "fac_sb_max", 4096},
    {"MLP_FACTOR_BUMP", "1023", nullptr, nullptr, "fac_bump_max", 1023},
    {"MLP_FACTOR_BUMP", "1023", nullptr, nullptr, "fac_sb_max", 1023},
    {"MLP_FACTOR_BUMP", "8", nullptr, nullptr, "fac_sb_max", 8},
    // MLP_FACTOR_SB is read after MLP_FACTOR_BUMP and overrides what that one left (engine.hip:114)
    {"MLP_FACTOR_BUMP", "8", "MLP_FACTOR_SB", "100", "fac_sb_max", 100},
    {"MLP_FACTOR_BUMP", "8", "MLP_FACTOR_SB", "100", "fac_bump_max", 8},
    {"MLP_FACTOR_BUMP", "64", "MLP_FACTOR_SB", "0", "fac_sb_max", 0},
};

static int failures = 0;
static void clear_env() {
    for (size_t r = 0; r < NROWS; ++r) unsetenv(ROWS[r].env);
    unsetenv("MLP_POOL_POISON");
}
static void expect(double got, double want, const std::string& what) {
    if (got == want) return;
    std::fprintf(stderr, "FAIL %s: got %.17g, want %.17g\n", what.c_str(), got, want);
    failures += 1;
}
static const Row* row_of_field(const char* field) {
    for (size_t r = 0; r < NROWS; ++r)
        if (!std::strcmp(ROWS[r].field, field)) return &ROWS[r];
    std::fprintf(stderr, "no row for field %s\n", field);
    std::exit(2);
}

int main() {
    clear_env();
    {   // a default-constructed Settings is from_env() of an environment without MLP_* variables: every field, the string too
        const Settings d, e = Settings::from_env();
        for (size_t r = 0; r < NROWS; ++r) {
            expect(ROWS[r].get(d), ROWS[r].want[0], std::string("default-constructed ") + ROWS[r].field);
            expect(ROWS[r].get(e), ROWS[r].get(d), std::string("from_env() without variables, ") + ROWS[r].field);
        }
        if (d.transport != e.transport || !d.transport.empty()) expect(1, 0, "transport of an empty environment");
    }
    size_t checks = 0;
    for (size_t k = 0; k < NROWS; ++k) {
        if (k > 0 && !std::strcmp(ROWS[k].env, ROWS[k - 1].env)) continue;  // (coupled rows: the variable was done with its first row)
        for (int v = 0; v < 7; ++v) {
            clear_env();
            if (VALUES[v]) setenv(ROWS[k].env, VALUES[v], 1);
            const Settings s = Settings::from_env();
            for (size_t r = 0; r < NROWS; ++r) {
                // the field's value under this variable: the row of (variable, field) if there is one, else the field's default
                double want = ROWS[r].want[0];
                bool own = !std::strcmp(ROWS[r].env, ROWS[k].env);
                if (!own) {
                    bool coupled = false;
                    for (size_t q = 0; q < NROWS; ++q)
                        if (!std::strcmp(ROWS[q].env, ROWS[k].env) && !std::strcmp(ROWS[q].field, ROWS[r].field)) coupled = true;
                    if (coupled) continue;  // (checked through the row of this variable)
                } else {
                    want = ROWS[r].want[v];
                }
                expect(ROWS[r].get(s), want,
                       std::string(ROWS[k].env) + (VALUES[v] ? std::string("=\"") + VALUES[v] + "\"" : std::string(" unset")) + " -> " + ROWS[r].field);
                checks += 1;
            }
            if (!std::strcmp(ROWS[k].env, "MLP_TRANSPORT") && s.transport != (VALUES[v] ? VALUES[v] : ""))
                expect(1, 0, std::string("MLP_TRANSPORT is kept verbatim: ") + s.transport);
        }
    }
    for (const Extra& x : EXTRAS) {
        clear_env();
        setenv(x.env, x.val, 1);
        if (x.env2) setenv(x.env2, x.val2, 1);
        const Settings s = Settings::from_env();
        expect(row_of_field(x.field)->get(s), x.want,
               std::string(x.env) + "=" + x.val + (x.env2 ? std::string(" ") + x.env2 + "=" + x.val2 : std::string()) + " -> " + x.field);
        checks += 1;
    }
    {   // MLP_POOL_POISON is the pool's, process-wide: no field of a Solution's settings follows it
        clear_env();
        setenv("MLP_POOL_POISON", "1", 1);
        const Settings s = Settings::from_env();
        for (size_t r = 0; r < NROWS; ++r) expect(ROWS[r].get(s), ROWS[r].want[0], std::string("MLP_POOL_POISON=1 -> ") + ROWS[r].field);
    }
    std::printf("settings_check: %zu rows, %zu comparisons, %d failures\n", NROWS, checks, failures);
    return failures ? 1 : 0;
}
