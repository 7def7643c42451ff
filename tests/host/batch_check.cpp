// batch_check.cpp — host-only check of csrc/batch.h (tests/test_batch_host.py compiles and runs it; no HIP, no GPU).
//
// Every decision of batch.h is compared with the expression Engine::run_loop held before batch.h existed, over the full cross product
// of small value sets of that decision's inputs (the sets are listed at each walk).  The decisions that feed each other — graph choice
// and batch size, head room, factor room, graph split — are walked as a chain: every (graph, multi, B) the first produces goes through
// the cross product of the next one's inputs, and so on, so every reachable combination is compared without walking unreachable ones.
//
// The ref_* functions were transcribed BY HAND from engine.hip of the commit before batch.h (8434fb7), statement for statement; each
// cites its lines there.  They are not derived from batch.h: an expression that changed on the way shows up here.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <tuple>

#include "batch.h"

using namespace mlp;

static const int RING = 64;  // kernels.h (= Settings::kRing)
static long cases = 0, failures = 0;

#define CHECK(what, got, want)                                                                      \
    do {                                                                                            \
        cases += 1;                                                                                 \
        if (!((got) == (want))) {                                                                   \
            if (failures++ < 20) std::printf("FAIL %s: %lld, expected %lld (line %d)\n", what, (long long)(got), (long long)(want), __LINE__); \
        }                                                                                           \
    } while (0)

// ---- engine.hip:1800-1801
static bool ref_long_run(bool use_graph, int graph_iters, uint64_t graph_batches_in_geom) { return use_graph && graph_iters > 1 && graph_batches_in_geom >= 8; }
static bool ref_sample(bool profile, int sample_every, uint64_t batches_run, bool long_run) {
    return profile && (sample_every == 1 || batches_run % (long_run ? 4 : 8) == 0);
}
// ---- engine.hip:1820-1822
static int ref_hyper_gap(bool capable, uint64_t hyper_off_until, uint64_t lifetime_pivots) {
    int hyper_gap = 0;
    if (hyper_off_until > lifetime_pivots && capable) hyper_gap = (int)std::min<uint64_t>(hyper_off_until - lifetime_pivots, (uint64_t)1 << 20);
    return hyper_gap;
}
// ---- engine.hip:1840-1858 (hyper_backoff_max = 8: engine.h:385); taken = stats.iterations - before
static void ref_backoff(bool hyper_bail, uint64_t taken, uint64_t lifetime_pivots, int& hyper_bail_streak, uint64_t& hyper_off_until) {
    const int hyper_backoff_max = 8;
    if (hyper_bail) {
        if (taken >= 16) {
            hyper_bail_streak = 0;
            hyper_off_until = lifetime_pivots + 1;
        } else {
            hyper_bail_streak = std::min(hyper_bail_streak + 1, hyper_backoff_max);
            hyper_off_until = lifetime_pivots + ((uint64_t)2 << hyper_bail_streak);
        }
    } else if (taken >= 16) {
        hyper_bail_streak = 0;
    }
}
// ---- engine.hip:1868, 1876
static void ref_row(int str_kmax, int sb_kmax, bool stepping, bool fac_on_, int k_, int max_row_nnz_, bool& want, bool& sb_now) {
    want = str_kmax > 0 && !stepping && !fac_on_ && k_ + RING + 1 <= str_kmax && max_row_nnz_ <= 4096;
    sb_now = want && k_ + RING + 1 <= sb_kmax;
}
// ---- engine.hip:1901-1917
struct RefGraphs {
    bool brief, graph_now, counts, multi;
    int B;
};
static RefGraphs ref_graphs(bool use_graph, bool pump_backend_, bool sample, int hyper_gap, bool have_graph, int eager_iters_in_geom, bool long_run,
                            bool cold_start_, int graph_iters, int batch, int64_t pivot_budget) {
    RefGraphs r;
    r.brief = hyper_gap > 0 && hyper_gap <= 4;
    r.graph_now = use_graph && !pump_backend_ && !sample && !r.brief && (have_graph || eager_iters_in_geom >= 4);
    r.counts = !have_graph && !r.brief;  // if (!have_graph && !brief) eager_iters_in_geom += 1;
    r.multi = r.graph_now && (long_run || cold_start_) && graph_iters > 1;
    int B = r.graph_now ? (r.multi ? RING : batch) : 1;
    if (pivot_budget > 0 && (int64_t)B > pivot_budget) B = (int)pivot_budget;
    if (hyper_gap > 0 && B > hyper_gap) B = hyper_gap;
    r.B = B;
    return r;
}
// ---- engine.hip:1826-1827 (the hypersparse branch's own batch)
static int ref_hyper_batch(int64_t pivot_budget) {
    int B = RING;
    if (pivot_budget > 0 && (int64_t)B > pivot_budget) B = (int)pivot_budget;
    return B;
}
// ---- engine.hip:1922-1927 (inside `if (ph)`)
static void ref_head(int kmax, int k_, int& B, bool& ph) {
    const int room = kmax - k_;
    const int Bp = std::min(B, room);
    if (Bp >= std::min(B, 4)) B = Bp;
    else ph = false;
}
// ---- engine.hip:1938-1946; refactor_ok: what fac_refactor() returns.  false: the loop `continue`s (B is not used)
static bool ref_factor(int fac_period_, int nlow, bool refactor_ok, int& B, bool& refactored) {
    refactored = false;
    int room = fac_period_ - nlow;
    if (room < std::min(fac_period_, std::max(1, std::min(B, 8)))) {
        refactored = true;
        if (!refactor_ok) return false;
        room = fac_period_;
    }
    if (B > room) B = room;
    return true;
}
// ---- engine.hip:1955-1959: gm / g1 are requested (get_graph never returns null), nfull launches of gm, B - nfull * graph_iters of g1
static void ref_split(bool multi, bool cold_start_, int B, int graph_iters, int& nfull, bool& gm, bool& g1) {
    nfull = multi ? B / graph_iters : 0;
    gm = multi && (nfull > 0 || cold_start_);
    g1 = B - nfull * graph_iters > 0 || !gm;
}

int main() {
    const int graph_iters_set[] = {1, 3, 10, 32};
    const uint64_t gbig_set[] = {0, 7, 8, 9};
    // sampling: booleans x sample_every {0, 1} x batches_run 0..17 x graph_iters x graph_batches_in_geom
    for (int profile = 0; profile < 2; ++profile)
        for (int every = 0; every < 2; ++every)
            for (uint64_t run = 0; run <= 17; ++run)
                for (int ug = 0; ug < 2; ++ug)
                    for (int gi : graph_iters_set)
                        for (uint64_t gb : gbig_set) {
                            const bool lr = batch_long_run(ug, gi, gb);
                            CHECK("long_run", lr, ref_long_run(ug, gi, gb));
                            CHECK("sample", batch_sampled(profile, every, run, lr), ref_sample(profile, every, run, ref_long_run(ug, gi, gb)));
                        }
    // hypersparse gap: capable x lifetime pivots x (off_until - lifetime) below, at and above every value of the gap's set and its cap
    const uint64_t life_set[] = {0, 5, 1000, (uint64_t)1 << 33};
    const int64_t delta_set[] = {-5, -1, 0, 1, 4, 5, 64, ((int64_t)1 << 20) - 1, (int64_t)1 << 20, ((int64_t)1 << 20) + 1, (int64_t)1 << 40};
    for (int cap = 0; cap < 2; ++cap)
        for (uint64_t life : life_set)
            for (int64_t d : delta_set) {
                if (d < 0 && (uint64_t)(-d) > life) continue;
                CHECK("hyper_gap", hyper_gap_of(cap, life + (uint64_t)d, life), ref_hyper_gap(cap, life + (uint64_t)d, life));
            }
    // back-off: bailed x pivots of the launch {0, 15, 16, 64} x streak 0..8 x lifetime pivots after x off_until before
    const uint64_t taken_set[] = {0, 15, 16, 64};
    const uint64_t off_set[] = {0, 50, ((uint64_t)1 << 33) + 5};
    for (int bailed = 0; bailed < 2; ++bailed)
        for (uint64_t taken : taken_set)
            for (int streak = 0; streak <= 8; ++streak)
                for (uint64_t life : life_set)
                    for (uint64_t off : off_set) {
                        int rs = streak;
                        uint64_t ro = off;
                        ref_backoff(bailed, taken, life, rs, ro);
                        const HyperBackoff b = hyper_backoff({streak, off}, bailed, taken, life, 8);
                        CHECK("backoff streak", b.streak, rs);
                        CHECK("backoff off_until", b.off_until, ro);
                    }
    // row form: str_kmax x sb_kmax x booleans x k around str_kmax - 65 and sb_kmax - 65 x longest row around 4096
    const int strk_set[] = {0, 100, 230}, sbk_set[] = {0, 160, 256}, rownnz_set[] = {1, 4096, 4097};
    for (int strk : strk_set)
        for (int sbk : sbk_set)
            for (int stepping = 0; stepping < 2; ++stepping)
                for (int fac = 0; fac < 2; ++fac)
                    for (int rn : rownnz_set) {
                        std::set<int> ks = {0};
                        for (int d = -2; d <= 2; ++d) {
                            ks.insert(std::max(0, strk - 65 + d));
                            ks.insert(std::max(0, sbk - 65 + d));
                        }
                        for (int k : ks) {
                            bool want, sb;
                            ref_row(strk, sbk, stepping, fac, k, rn, want, sb);
                            const RowChoice r = row_choice(strk, sbk, stepping, fac, k, RING, rn);
                            CHECK("row want", r.want, want);
                            CHECK("row sb", r.sb, sb);
                        }
                    }
    // graph choice and batch size: booleans x eager_iters_in_geom 0..5 x hyper_gap x budget x batch x graph_iters x graph_batches_in_geom
    const int gap_set[] = {0, 1, 4, 5, 64, 1 << 20};
    const int64_t budget_set[] = {-1, 1, 7, 64, 1000};
    const int batch_set[] = {1, 5, 32, 64};
    std::set<std::tuple<bool, bool, int, int>> planned;  // (graph, multi, B, graph_iters) reached
    for (int64_t budget : budget_set) CHECK("hyper batch", clip_batch(RING, budget, 0), ref_hyper_batch(budget));
    for (int bits = 0; bits < 32; ++bits)
        for (int eager = 0; eager <= 5; ++eager)
            for (int gap : gap_set)
                for (int64_t budget : budget_set)
                    for (int batch : batch_set)
                        for (int gi : graph_iters_set)
                            for (uint64_t gb : gbig_set) {
                                const bool ug = bits & 1, pump = bits & 2, sample = bits & 4, have = bits & 8, cold = bits & 16;
                                const bool lr = ref_long_run(ug, gi, gb);
                                const RefGraphs r = ref_graphs(ug, pump, sample, gap, have, eager, lr, cold, gi, batch, budget);
                                BatchPlan p;
                                p.sample = sample;
                                p.hyper_gap = gap;
                                const bool counts = plan_graphs(p, ug, pump, have, eager, lr, cold, gi, batch, RING, budget);
                                CHECK("brief", p.brief, r.brief);
                                CHECK("graph", p.graph, r.graph_now);
                                CHECK("counts as eager", counts, r.counts);
                                CHECK("multi", p.multi, r.multi);
                                CHECK("B", p.B, r.B);
                                CHECK("sample kept", p.sample, sample);
                                CHECK("gap kept", p.hyper_gap, gap);
                                planned.insert({r.graph_now, r.multi, r.B, gi});
                            }
    // head room: every planned batch x (kmax - k) in -1..6 and 70, at two values of k
    std::set<std::tuple<bool, bool, int, int>> headed = planned;  // (a batch without the head keeps its B)
    const int room_set[] = {-1, 0, 1, 2, 3, 4, 5, 6, 70};
    for (const auto& t : planned)
        for (int room : room_set)
            for (int k : {0, 57}) {
                int B = std::get<2>(t);
                bool ph = true;
                ref_head(k + room, k, B, ph);
                const HeadRoom h = head_room(std::get<2>(t), k + room, k);
                CHECK("head kept", h.head, ph);
                CHECK("head B", h.B, B);
                headed.insert({std::get<0>(t), std::get<1>(t), B, std::get<3>(t)});
            }
    // factor room: every batch so far x period {1, 48, 64} x nlow 0..period x the refactorisation's outcome
    std::set<std::tuple<bool, bool, int, int>> roomed = headed;  // (without the factor a batch keeps its B)
    for (const auto& t : headed)
        for (int period : {1, 48, 64})
            for (int nlow = 0; nlow <= period; ++nlow)
                for (int ok = 0; ok < 2; ++ok) {
                    int B = std::get<2>(t);
                    bool refactored;
                    const bool goes_on = ref_factor(period, nlow, ok, B, refactored);
                    int room = factor_room(period, nlow), Bn = std::get<2>(t);
                    const bool due = factor_refactor_due(room, period, Bn);
                    CHECK("refactor due", due, refactored);
                    if (due && !ok) {
                        CHECK("factor left", false, goes_on);
                        continue;
                    }
                    if (due) room = period;
                    if (Bn > room) Bn = room;  // (Engine::fit_factor_room)
                    CHECK("factor B", Bn, B);
                    roomed.insert({std::get<0>(t), std::get<1>(t), B, std::get<3>(t)});
                }
    // graph split: every batch that replays graphs x cold start
    for (const auto& t : roomed)
        for (int cold = 0; cold < 2; ++cold) {
            if (!std::get<0>(t)) continue;
            int nfull;
            bool gm, g1;
            ref_split(std::get<1>(t), cold, std::get<2>(t), std::get<3>(t), nfull, gm, g1);
            BatchPlan p;
            p.graph = true;
            p.multi = std::get<1>(t);
            p.B = std::get<2>(t);
            split_graphs(p, cold, std::get<3>(t));
            CHECK("nfull", p.nfull, nfull);
            CHECK("multi graph", p.multi_graph, gm);
            CHECK("single graph", p.single_graph, g1);
        }
    std::printf("%ld cases, %ld failures\n", cases, failures);
    return failures ? 1 : 0;
}
