// settings.cpp — the only place of the engine that reads MLP_* variables (the pool's MLP_POOL_POISON aside).  The parse rules differ per
// knob on purpose (first character '1', first character not '0', atoi > 0, atoi != 0, mere presence): each is what the suite and the
// tools have always set.
#include "settings.h"

#include <algorithm>
#include <cstdlib>

namespace mlp {

static const char* env(const char* name) { return std::getenv(name); }
static bool not_zero(const char* name) {  // on unless the value starts with '0'
    const char* e = env(name);
    return !(e && e[0] == '0');
}
static int clamped(const char* e, int lo, int hi) { return std::max(lo, std::min(hi, std::atoi(e))); }

Settings Settings::from_env() {
    Settings s;
    const char* ng = env("MLP_NO_GRAPH");
    s.use_graph = !(ng && ng[0] == '1');
    if (const char* bs = env("MLP_BATCH")) s.batch = clamped(bs, 1, kRing);
    if (const char* gi = env("MLP_GRAPH_ITERS")) s.graph_iters = clamped(gi, 1, 32);

    s.debug_sync = env("MLP_DEBUG_SYNC") != nullptr;
    if (const char* kp = env("MLP_KPROF")) s.kprof = std::atoi(kp);
    s.hyper_prof = env("MLP_HYPER_PROF") != nullptr;
    s.pump_debug = env("MLP_PUMP_DEBUG") != nullptr;

    if (const char* bd = env("MLP_BANDED")) s.banded_mode = std::atoi(bd) != 0 ? 1 : 0;
    if (const char* dm = env("MLP_DETERMINISTIC")) s.det_mode = std::atoi(dm) != 0 ? 1 : 0;
    s.lazy_dse = not_zero("MLP_LAZY_DSE");
    if (const char* lr = env("MLP_LOWRANK")) s.lr_force = clamped(lr, 0, kLrMax);
    const char* bt = env("MLP_BIGTILE");
    s.force_big_tiles = bt && std::atoi(bt) != 0;
    if (const char* lp = env("MLP_LDPAD")) s.ld_pad = clamped(lp, 0, 4096) & ~1;
    if (const char* sb = env("MLP_STREAM_BALANCED")) s.sw_balanced = std::atoi(sb);
    if (const char* fp = env("MLP_FPULL")) s.fpull = fp[0] != '0';
    if (const char* pd = env("MLP_PB_DET")) s.pb_det = std::atoi(pd);

    s.tk_ride = not_zero("MLP_TK_RIDE");
    s.rk_ride = not_zero("MLP_RK_RIDE");
    s.ratio_list = not_zero("MLP_RATIO_LIST");
    if (const char* cp = env("MLP_RATIO_LIST_CAP")) s.ratio_list_cap = clamped(cp, 0, kRlCap);
    s.btran_ride = not_zero("MLP_BTRAN_RIDE");
    s.v_ride = not_zero("MLP_V_RIDE");
    s.ratio_one = not_zero("MLP_RATIO_ONE");
    s.ratio_two = env("MLP_RATIO_TWO_KERNELS") != nullptr;
    if (const char* rs = env("MLP_RATIO_SPIN_LIMIT")) s.ratio_spin_limit = std::atoll(rs);
    if (const char* sk = env("MLP_STR_K")) s.str_kmax = std::atoi(sk);
    s.small_basis = not_zero("MLP_SMALL_BASIS");
    if (const char* sbk = env("MLP_SMALL_BASIS_K")) s.sb_kmax = clamped(sbk, 0, 256);
    s.primal_head = not_zero("MLP_PRIMAL_HEAD");
    if (const char* phk = env("MLP_PRIMAL_HEAD_K")) s.ph_kmax = std::max(0, std::atoi(phk));
    s.pull_inside = not_zero("MLP_PULL_INSIDE");
    s.head_apply = not_zero("MLP_HEAD_APPLY");
    if (const char* hy = env("MLP_HYPER")) s.hyper_mode = std::atoi(hy) > 0 ? 1 : 0;
    if (const char* hh = env("MLP_HYPER_HEAVY")) s.hyper_heavy = std::atol(hh);

    if (const char* of = env("MLP_ORDER_FROM")) s.order_from = (uint64_t)std::atoll(of);
    if (const char* oe = env("MLP_ORDER_EVERY")) s.order_every = (uint64_t)std::atoll(oe);
    if (const char* sp = env("MLP_SWEEP_PACKED")) s.use_pack = sp[0] != '0';

    if (const char* rt = env("MLP_REFRESH_TOL")) s.refresh_tol = std::atof(rt);
    if (const char* fr = env("MLP_FINAL_REFRESH")) s.final_refresh_pivots = std::atol(fr);
    s.reinvert_gj = env("MLP_REINVERT_GJ") != nullptr;

    if (const char* fm = env("MLP_FACTOR")) s.fac_mode = std::atoi(fm) > 0 ? 1 : 0;
    if (const char* ff = env("MLP_FACTOR_FROM")) s.fac_auto_cap = std::max(256, std::atoi(ff));
    if (const char* fb = env("MLP_FACTOR_BUMP")) {  // (lowering the bump limit lowers it for both carriers of the bump)
        const int want = std::atoi(fb);
        s.fac_bump_max = std::max(0, std::min(kFacBmax, want));
        if (want < kFacBmax) s.fac_sb_max = std::min(s.fac_sb_max, s.fac_bump_max);  // (a value at or above the dense carrier's capacity leaves the sparse carrier's limit alone)
    }
    if (const char* fs = env("MLP_FACTOR_SB")) s.fac_sb_max = clamped(fs, 0, kFacSbMax);
    if (const char* fs = env("MLP_FACTOR_SB_FROM")) s.fac_sb_from = std::max(1, std::atoi(fs));
    if (const char* fj = env("MLP_FACTOR_J")) {  // a fixed period; default: 48, and 64 while a refactorisation is expensive (fac_refactor)
        s.fac_J = s.fac_period = clamped(fj, 1, 64);
        s.fac_period_auto = false;
    }
    s.fac_fuse = not_zero("MLP_FACTOR_FUSE");
    s.fac_rho_part = not_zero("MLP_FACTOR_RHO_PART");

    if (const char* tr = env("MLP_TRANSPORT")) s.transport = tr;
    s.shard_defer = not_zero("MLP_SHARD_DEFER");
    const char* nws = env("MLP_NO_WSHARD");
    s.no_wshard = nws && std::atoi(nws) != 0;
    const char* fsd = env("MLP_FACTOR_SHARED_DEVICE");
    s.fac_shared_device = fsd && fsd[0] == '1';
    if (const char* sk = env("MLP_TEST_GOLIVE_SKEW")) s.golive_skew = std::atoi(sk);
    return s;
}

}  // namespace mlp
