// settings.h — every MLP_* environment knob of the engine as one plain value.  Host-only: nothing of HIP.
// A Solution reads the environment ONCE, when it is created (Settings::from_env), and keeps the result for life; a clone gets its
// parent's.  The one exception is MLP_POOL_POISON: it belongs to the device block pool, which is process-wide (engine.hip).
#pragma once
#include <cstdint>
#include <string>

namespace mlp {

struct Settings {
    // bounds of the clamps: the kernel-side constants of the same meaning (kernels.h; engine.hip asserts that they agree)
    static constexpr int kRing = 64, kLrMax = 32, kFacBmax = 1024, kFacSbMax = 4096, kRlCap = 8;

    // --- graphs and batches
    bool use_graph = true;                    // MLP_NO_GRAPH=1: eager launches
    int batch = 32;                           // MLP_BATCH: iterations per host round trip (1 .. RING)
    int graph_iters = 10;                     // MLP_GRAPH_ITERS: iterations per graph once a geometry has run for a while (1 = off; .. 32)
    // --- diagnostics
    bool debug_sync = false;                  // MLP_DEBUG_SYNC (with MLP_NO_GRAPH=1): synchronise after every stage and name it
    int kprof = 0;                            // MLP_KPROF: 1 kernel timeline marks; 2..5 per-rank quantity in the records
    bool hyper_prof = false;                  // MLP_HYPER_PROF: per-stage wall-clock marks of the hypersparse kernel
    bool pump_debug = false;                  // MLP_PUMP_DEBUG: progress reports of the pump transports
    // --- representation and passes
    int banded_mode = -1;                     // MLP_BANDED: 1 force on, 0 off, -1 auto
    int det_mode = -1;                        // MLP_DETERMINISTIC: 1 force the pulled F products, 0 never, -1 auto
    bool lazy_dse = true;                     // MLP_LAZY_DSE=0: maintain beta in every pivot like the reference
    int lr_force = -1;                        // MLP_LOWRANK: force the delayed-update period (0 = off; .. LR_MAX); -1: 32 from cap 8192
    bool force_big_tiles = false;             // MLP_BIGTILE: the large-nucleus tiling of the fused W pass at any size (tests)
    int ld_pad = 16;                          // MLP_LDPAD: extra doubles per row of a large W (0 .. 4096, even)
    int sw_balanced = 1;                      // MLP_STREAM_BALANCED=0: fixed 128-row strips; N > 1: that many blocks
    bool fpull = true;                        // MLP_FPULL=0: the blocked push + k_ratio_primal_fused (A/B, tests)
    int pb_det = -1;                          // MLP_PB_DET: 1 / 0 force the deterministic blocked push on / off for unsharded solves
    // --- forms of an iteration (Geom.forms, Geom.rl_cap)
    bool tk_ride = true;                      // MLP_TK_RIDE=0: t_K in a BTRAN launch of its own
    bool rk_ride = true;                      // MLP_RK_RIDE=0: rho_K likewise
    bool ratio_list = true;                   // MLP_RATIO_LIST=0: the grid form of the primal Harris test as two passes with the in-kernel wait
    int ratio_list_cap = kRlCap;              // MLP_RATIO_LIST_CAP: entries a block may list (0: every decision re-scans; .. RL_CAP)
    bool btran_ride = true;                   // MLP_BTRAN_RIDE=0: rho_K and t_K of a medium-nucleus pivot in a k_btran launch
    bool v_ride = true;                       // MLP_V_RIDE=0: the v partials in the pass over W, the v tail in k_post_fused
    bool ratio_one = true;                    // MLP_RATIO_ONE=0: the grid forms of the Harris tests at any size
    bool ratio_two = false;                   // MLP_RATIO_TWO_KERNELS: two launches for the two Harris passes (Engine::ratio_two latches too)
    long long ratio_spin_limit = 20000000LL;  // MLP_RATIO_SPIN_LIMIT: polls before a fused ratio test gives up (0: the first launch stalls)
    int str_kmax = 230;                       // MLP_STR_K: largest nucleus the sparse tableau row (k_row_touch / k_row_pull) is used for (0: never)
    bool small_basis = true;                  // MLP_SMALL_BASIS=0: never k_small_basis
    int sb_kmax = 160;                        // MLP_SMALL_BASIS_K: largest nucleus, at the end of a full record ring, k_small_basis is used for (0 .. 256);
                                              // measured crossover with the three launches at k ~ 110-120 (tools/small_basis_curve.py)
    bool primal_head = true;                  // MLP_PRIMAL_HEAD=0: never k_primal_head
    int ph_kmax = -1;                         // MLP_PRIMAL_HEAD_K: its bound on the nucleus (0: off); -1: primal_head_kmax(longest column)
    bool pull_inside = true;                  // MLP_PULL_INSIDE=0: the touched columns pulled by a launch of their own
    bool head_apply = true;                   // MLP_HEAD_APPLY=0: the update kernel applies the basic side
    int hyper_mode = -1;                      // MLP_HYPER: 1 on wherever the kernel applies, 0 off, -1 auto (<= 16 non-zeros per row on average)
    long hyper_heavy = 0;                     // MLP_HYPER_HEAVY: eta-update entries one workgroup takes on (0: the kernel's default)
    // --- banded sweep
    uint64_t order_from = 4096;               // MLP_ORDER_FROM: pivots after which the locality order is switched on
    uint64_t order_every = 2048;              // MLP_ORDER_EVERY: pivots between its rebuilds
    bool use_pack = true;                     // MLP_SWEEP_PACKED=0: always the indirect path through the full copy (Engine::use_pack latches off too)
    // --- accuracy
    double refresh_tol = 1e-7;                // MLP_REFRESH_TOL: re-invert when the two-way pivot check disagrees by more than this
    long final_refresh_pivots = 50000;        // MLP_FINAL_REFRESH: pivots before the final refresh / polish (0 = never)
    bool reinvert_gj = false;                 // MLP_REINVERT_GJ: the unblocked Gauss-Jordan at any size (A/B of the blocked inversion)
    // --- compact factor
    int fac_mode = -1;                        // MLP_FACTOR: 1 from the start (back to the explicit inverse when the peel leaves a bump), 0 never, -1 auto
    int fac_auto_cap = 8192;                  // MLP_FACTOR_FROM: auto tries it when the nucleus would need more slots than this (>= 256)
    int fac_bump_max = kFacBmax;              // MLP_FACTOR_BUMP: largest bump carried through its dense inverse (below FAC_BMAX: caps fac_sb_max too)
    int fac_sb_max = kFacSbMax;               // MLP_FACTOR_SB: largest bump eliminated sparsely, LU with fill (0 = never); one whose rows outgrow
                                              // their slots falls back to the dense inverse (b <= fac_bump_max)
    int fac_sb_from = 48;                     // MLP_FACTOR_SB_FROM: smaller bumps keep the dense inverse, one wave-sized product per solve (>= 1)
    int fac_J = 64;                           // MLP_FACTOR_J: rank-1 terms the factor has room for (1 .. 64) ...
    int fac_period = 48;                      // ... = the pivots between refactorisations when set ...
    bool fac_period_auto = true;              // ... which fac_refactor otherwise retunes (Engine::fac_J_, fac_period_ are the live values)
    bool fac_fuse = true;                     // MLP_FACTOR_FUSE=0: the single-purpose launches around the solves of a dual iteration
    bool fac_rho_part = true;                 // MLP_FACTOR_RHO_PART=0
    // --- sharding
    std::string transport;                    // MLP_TRANSPORT: peer (default) / host / rccl / pump, unless enable_sharding names one
    bool shard_defer = true;                  // MLP_SHARD_DEFER=0: sharded from the first pivot
    bool no_wshard = false;                   // MLP_NO_WSHARD: keep the streaming pass replicated on every rank
    bool fac_shared_device = false;           // MLP_FACTOR_SHARED_DEVICE=1 (test hook): keep the factor although ranks share a device
    int golive_skew = -1;                     // MLP_TEST_GOLIVE_SKEW=<rank> (test hook): that rank publishes a perturbed fingerprint

    static Settings from_env();
};

}  // namespace mlp
