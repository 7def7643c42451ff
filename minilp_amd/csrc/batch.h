// batch.h — what Engine::run_loop decides once per batch, as pure functions of plain values ("Where the batch is
// decided").  Host-only, like settings.h: nothing of HIP and nothing of the engine, so tests/host/batch_check.cpp walks the policy on
// the CPU.  The engine gathers the results in one BatchPlan per batch; like an IterPlan it is never compared and never a cache key.
#pragma once
#include <algorithm>
#include <cstdint>

namespace mlp {

struct BatchPlan {
    bool sample = false;      // ONE eager iteration bracketed by HIP events (profile mode)
    int hyper_gap = 0;        // pivots the multi-kernel path still has to take before the hypersparse kernel is tried again (0: none owed)
    bool brief = false;       // the few iterations handed over by the hypersparse kernel: eager, no graph is captured for them
    bool graph = false;       // the batch replays graphs
    bool multi = false;       // ... of several iterations first
    int B = 1;                // iterations the batch may take
    int nfull = 0;            // launches of the graph of several iterations; the remainder of B as one-iteration graphs
    bool multi_graph = false, single_graph = false;  // which of the two graphs the batch needs (captured if missing)
};

// ---- sampling (profile mode): every 8th batch is a sampled iteration, every 4th once the geometry runs on graphs of several iterations
inline bool batch_long_run(bool use_graph, int graph_iters, uint64_t graph_batches_in_geom) {
    return use_graph && graph_iters > 1 && graph_batches_in_geom >= 8;
}
inline bool batch_sampled(bool profile, int sample_every, uint64_t batches_run, bool long_run) {
    return profile && (sample_every == 1 || batches_run % (long_run ? 4 : 8) == 0);
}

// ---- hypersparse kernel
inline int hyper_gap_of(bool capable, uint64_t off_until, uint64_t lifetime_pivots) {
    if (!(off_until > lifetime_pivots && capable)) return 0;
    return (int)std::min<uint64_t>(off_until - lifetime_pivots, (uint64_t)1 << 20);
}
struct HyperBackoff {
    int streak;          // bail-outs in a row after short runs
    uint64_t off_until;  // lifetime pivot count until which the multi-kernel path runs
};
// Dense iterations come in clusters (measured on config 3: handing over one pivot at a time costs 173 bail-outs
// and 185 ms against 28 and 172 ms with a back-off): after a run of >= 16 hypersparse iterations the multi-kernel
// path takes that one pivot only; after a short run it keeps going for 4, 8, ... 512 pivots before the next attempt
inline HyperBackoff hyper_backoff(HyperBackoff now, bool bailed, uint64_t pivots_taken, uint64_t lifetime_pivots, int streak_max) {
    if (bailed) {
        if (pivots_taken >= 16) return {0, lifetime_pivots + 1};
        const int streak = std::min(now.streak + 1, streak_max);
        return {streak, lifetime_pivots + ((uint64_t)2 << streak)};
    }
    if (pivots_taken >= 16) now.streak = 0;
    return now;
}

// ---- forms of the small-nucleus iteration: decided by the size the nucleus can reach within a full record ring
struct RowChoice {
    bool want;  // sparse tableau row
    bool sb;    // ... and k_small_basis allowed
};
inline RowChoice row_choice(int str_kmax, int sb_kmax, bool stepping, bool fac_on, int k, int ring, int max_row_nnz) {
    const bool want = str_kmax > 0 && !stepping && !fac_on && k + ring + 1 <= str_kmax && max_row_nnz <= 4096;
    return {want, want && k + ring + 1 <= sb_kmax};
}

// ---- graphs or eager launches, and how many iterations
inline int clip_batch(int B, int64_t budget, int gap) {
    if (budget > 0 && (int64_t)B > budget) B = (int)budget;
    if (gap > 0 && B > gap) B = gap;
    return B;
}
// Fills brief, graph, multi and B from sample and hyper_gap; returns whether the batch counts towards the eager iterations a geometry
// runs before its graph is captured.
inline bool plan_graphs(BatchPlan& p, bool use_graph, bool pump, bool have_graph, int eager_iters_in_geom, bool long_run, bool cold_start,
                        int graph_iters, int batch, int ring, int64_t budget) {
    p.brief = p.hyper_gap > 0 && p.hyper_gap <= 4;
    p.graph = use_graph && !pump && !p.sample && !p.brief && (have_graph || eager_iters_in_geom >= 4);
    p.multi = p.graph && (long_run || cold_start) && graph_iters > 1;
    p.B = clip_batch(p.graph ? (p.multi ? ring : batch) : 1, budget, p.hyper_gap);
    return !have_graph && !p.brief;
}

// ---- small-nucleus primal head: the batch must end before the nucleus can outgrow the kernel's slots (every pivot may add one); a
// batch that would be cut below 4 iterations (or below itself) drops the head instead
struct HeadRoom {
    bool head;
    int B;
};
inline HeadRoom head_room(int B, int kmax, int k) {
    const int Bp = std::min(B, kmax - k);
    if (Bp >= std::min(B, 4)) return {true, Bp};
    return {false, B};
}

// ---- compact factor: every basis change of the batch appends a rank-1 term; refactor when fewer than a batch of them fit
inline int factor_room(int period, int nlow) { return period - nlow; }
inline bool factor_refactor_due(int room, int period, int B) { return room < std::min(period, std::max(1, std::min(B, 8))); }

// ---- whole multi-iteration graphs first, the remainder of the batch as one-iteration graphs (a cold solve captures the graph of
// several iterations ahead of its first use)
inline void split_graphs(BatchPlan& p, bool cold_start, int graph_iters) {
    p.nfull = p.multi ? p.B / graph_iters : 0;
    p.multi_graph = p.multi && (p.nfull > 0 || cold_start);
    p.single_graph = p.B - p.nfull * graph_iters > 0 || !p.multi_graph;
}

}  // namespace mlp
