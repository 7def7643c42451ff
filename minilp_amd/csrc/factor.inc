// factor.inc — the COMPACT FACTOR of the basis (SURVEY §8 row f3; HISTORY.md §2.6).  Included by kernels.hip.
//
// The default representation of B^-1 (singleton split + explicit dense nucleus inverse, DESIGN.md §2) costs 8 k^2 bytes and
// O(k^2) traffic per pivot whatever the sparsity of the nucleus.  For models whose bases are permutable to (near-)triangular
// form — networks with gains, transport / assignment structure, staircase models: their LU has no fill — this file holds the
// second representation, selected by the MEASURED shape of the basis (Engine::fac_try_enable):
//
//   refactorisation = an iterated column-singleton PEEL of the basis matrix B0 (lu.rs:118-304 is the reference's left-looking
//     LU; its column order `order_simple`, ordering.rs:4-21, is by column count — the peel is the same idea carried to its
//     fixed point): level 1 holds the basic columns with a single entry, they claim their rows; a column all of whose other
//     rows have been claimed joins the next level, and so on.  In (row, position) peel order B0 is upper triangular, so when
//     the peel consumes every column the "factors" are A itself plus the order: nothing is stored, nothing fills.
//   FTRAN x = B0^-1 b (lu.rs:79-106 with the reach restriction of 432-463 replaced by level scheduling): levels in DESCENDING
//     order, every position PULLS along the CSR row of its pivot row: x[p] = (b[i] - sum A[i, c] x[pos(c)]) / A[i, var(p)].
//   BTRAN y = B0^-T c: levels ASCENDING, every position pulls along its CSC column: y[i] = (c[p] - sum A[i', var(p)] y[i']) / pivot.
//     Both are fixed-order pulls: no atomics, bit-reproducible.
//   eta file (solver.rs:1274-1284, 1305-1338): the transformations since the refactorisation are kept in ADDITIVE form,
//     B^-1 = B0^-1 + sum_j U_j V_j^T with U_j = -(alpha_q - e_r) / alpha_q[r] (by position), V_j = rho_r (by row) of pivot j —
//     a solve is the B0 solve plus nlow dot products and one axpy pass, with no dependent chain through the terms.
//   refactor trigger (solver.rs:1096-1103: eta nnz >= LU nnz): after fac_J pivots.
//
// One persistent kernel per solve (k_fac_solve): one workgroup per CU, the levels separated by a grid barrier (write-through
// stores + one agent-scope counter; all workgroups are co-resident by construction).  Memory: two ints + one double per
// position, (2 fac_J + 2) m doubles of work vectors — against 8 k^2 for the explicit inverse.

static_assert(FAC_TAIL == BLK, "the tail walks one item per lane");
constexpr int FAC_SEG_LEVELS = 512;  // levels of a run of small levels whose table fits LDS at a time

// Grid barrier of the persistent solve kernel: `bar` starts at zero at every launch (the kernel's last workgroup resets it)
// and counts arrivals; `target` = arrivals after which this barrier opens.  Stores that other workgroups will read are made
// with st_agent (write-through), so draining the store queue before the arrival is all the release that is needed; readers use
// ld_agent.  Bounded: a grid that is not co-resident (another process holding the CUs) ends the batch with ITER_STALL.
__device__ __forceinline__ bool fac_grid_barrier(Ctl* c, unsigned* bar, unsigned target) {
    __shared__ int s_ok;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every lane's write-through stores have left before the arrival is announced
    __syncthreads();
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // The arrivals count on bar[0]; the waiters poll a RELEASE word on a line of its own (bar[FAC_BAR_FLAG]) that the last arrival
        // sets: polling loads on the counter's line queued with the arrivals behind them (a level of the transport family's walk
        // 5.0 -> 2.9 us).  (Counting the arrivals in two steps — eight counters 4 KB apart, then bar[0] — changed nothing at 256 workgroups.)
        unsigned* flag = bar + FAC_BAR_FLAG;
        const bool last = __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == target;
        int ok = 1;
        if (last) {
            __hip_atomic_store(flag, target, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            for (long spins = 0; __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target; ++spins) {
                if (spins > 40000000L) {
                    ok = 0;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
        }
        s_ok = ok;
    }
    __syncthreads();
    return s_ok != 0;
}
// (the words of fac_bar back to zero: the last workgroup of a kernel that used the barrier)
__device__ __forceinline__ void fac_bar_reset(unsigned* bar) {
    bar[0] = 0u;
    bar[1] = 0u;
    bar[FAC_BAR_FLAG] = 0u;
}

// Workgroup barrier for data exchanged through LDS only: waits for this wave's LDS traffic, NOT for its global loads and stores.
// __syncthreads() is a workgroup fence — s_waitcnt vmcnt(0) before the s_barrier — so a level loop that copies results out to memory
// (or keeps record loads of later levels in flight) paid one memory round trip per level (~1-1.7 us) for nothing.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// One or TWO solves with the compact factor in one walk over the levels (the second right-hand side shares every barrier and every
// edge load with the first: the dual iteration's alpha_q = B^-1 a_q and tau = B^-1 rho, the primal iteration's rho = B^-T e_r and
// v = B^-T alpha_q — a solve is a chain of dependent steps, not bandwidth, so the second one is almost free).
//   dir 0: FTRAN  x = B^-1 b.   src 0: b = the entering column (scattered into fac_rhs by the stage head; cleared here),
//                               src 1: b = rho (rv[i].x), src 2: b = sp (dense, by row).       dst 0: alpha_q, dst 1: tau.
//   dir 1: BTRAN  y = B^-T c.   src 0: c = e_r, src 1: c = alpha_q, src 2: c = sp (by position).  dst 0: rho (rv[i].x; also
//                               ||rho||^2 -> it.rho_sq), dst 1: v (rv[i].y).
//   srcB < 0: a single solve.   always: run whatever the iteration status (solves outside an iteration: recalc_obj_coeffs, ...).
__global__ void __launch_bounds__(BLK) k_fac_solve(DevView v, int dir, int srcA, int dstA, int srcB, int dstB, const double* sp, int always, int fuse) {
    Ctl* c = v.ctl;
    if (!always && (c->halt || c->it.status != ITER_PIVOT)) return;
    // fuse & 1 (BTRAN of a dual iteration): the leaving row's scalars — k_btran_prep's work, one launch fewer; nothing in this kernel reads them
    if ((fuse & 1) && blockIdx.x == 0 && threadIdx.x < 64) btran_prep_wave(v, c, (int)threadIdx.x, c->it.r, 1, 0, 1);
    const int tid = threadIdx.x, nb = (int)gridDim.x, m = v.m;
    const int nlev = v.fac_meta[0];
    const int nlow = c->nlow;
    const int nl = srcB >= 0 ? 2 : 1;  // right-hand sides ("lanes")
    unsigned* bar = v.fac_bar;
    // (selects, not tables: a table indexed by the lane of the solve lives in scratch memory)
    double* const x0a = v.fac_x0;
    double* const x0b = v.fac_x0 + m;
    auto X0 = [&](int l) -> double* { return l == 0 ? x0a : x0b; };
    auto SRC = [&](int l) -> int { return l == 0 ? srcA : srcB; };
    auto DST = [&](int l) -> int { return l == 0 ? dstA : dstB; };
    const int r_leave = c->it.r;
    KMARK0(c, dir * 10);
    auto rhs_of = [&](int l, int i_row, int p_pos) -> double {  // entry of lane l's right-hand side (FTRAN: by row, BTRAN: by position)
        const int sc = SRC(l);
        if (dir == 0) return sc == 0 ? v.fac_rhs[i_row] : (sc == 1 ? v.rv[i_row].x : sp[i_row]);
        return sc == 0 ? (p_pos == r_leave ? 1.0 : 0.0) : (sc == 1 ? v.alpha_q[p_pos] : sp[p_pos]);
    };
    __shared__ double s_coef[2][64];
    // ---- coefficients of the pending rank-1 terms, coef_j = V_j . b (FTRAN) / U_j . c (BTRAN), in a fixed order.
    // A sparse right-hand side (the entering column, e_r): workgroup j forms its coefficient directly.  A DENSE one (rho, alpha_q,
    // sp): one workgroup streams only ~50 GB/s, so a 200 000-row dot product per workgroup would cost more than the whole solve;
    // instead every workgroup forms the partial sums of its slice for all terms (wave sums, combined in wave order), and after
    // the first grid barrier workgroup j adds the partials of term j in workgroup order.
    __shared__ double s_w[BLK / 64][64];
    __shared__ double s_inv[64];
    if (tid < 64) s_inv[tid] = tid < nlow ? c->fac_inv[tid] : 0.0;
    __syncthreads();
    bool any_dense = false;
    for (int l = 0; l < nl; ++l) {
        if (SRC(l) == 0) {
            if ((int)blockIdx.x < nlow) {
                const int j = (int)blockIdx.x;
                double acc = 0.0;
                if (dir == 0) {
                    const double* Vj = v.fac_V + (size_t)j * m;
                    const int var = c->it.entering_var;
                    const int end = v.csc_ptr[var + 1];
                    for (int e = v.csc_ptr[var] + tid; e < end; e += BLK) acc += v.csc_val[e] * Vj[v.csc_row[e]];
                } else if (tid == 0) {
                    acc = -v.fac_U[(size_t)j * m + r_leave] * c->fac_inv[j];
                }
                acc = block_sum(acc);
                if (tid == 0) st_agent(&v.fac_coef[l * 64 + j], acc);
            }
        } else if (nlow > 0 && dir == 0 && SRC(l) == 1 && c->fac_rho_part_ok && c->fac_rho_part_n == nlow) {
            // tau = B^-1 rho: the BTRAN that produced rho left the partial sums of V_j . rho behind (region 2 of fac_part; its epilogue
            // holds rho in registers and rho is sparse — the dense pass here cost 14-25 us of a 50-60 us solve at 200 000 rows with 32
            // terms pending).  Same lanes, same trees, same order as the pass below: the same bits.
            if ((int)blockIdx.x < nlow) {
                double a_ = 0.0;
                for (int i_ = tid; i_ < nb; i_ += BLK) a_ += ld_agent(&v.fac_part[((size_t)2 * 64 + blockIdx.x) * nb + i_]);
                a_ = block_sum(a_);
                if (tid == 0) st_agent(&v.fac_coef[l * 64 + blockIdx.x], a_);
            }
        } else if (nlow > 0) {
            any_dense = true;
            const double* T0 = dir == 0 ? v.fac_V : v.fac_U;
            const int wv = tid >> 6, ln = tid & 63;
            __syncthreads();  // (s_w of the other lane has been consumed)
            // (eight terms at a time: their loads are in flight together and the eight wave reductions interleave — one term per trip
            // was a chain of nlow memory round trips, 50-66 us with 64 terms pending; per term the same sums in the same order)
            for (int j0 = 0; j0 < nlow; j0 += 8) {
                double acc[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] = 0.0;
                for (int idx = (int)blockIdx.x * BLK + tid; idx < m; idx += nb * BLK) {
                    const double rr = rhs_of(l, idx, idx);
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (j0 + u < nlow) {
                            double tv = T0[(size_t)(j0 + u) * m + idx];
                            if (dir == 1) tv = -tv * s_inv[j0 + u];  // (U_j is stored unscaled: see k_fac_append)
                            acc[u] += tv * rr;
                        }
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] = wave_sum(acc[u]);
                if (ln == 0) {
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (j0 + u < nlow) s_w[wv][j0 + u] = acc[u];
                }
            }
            __syncthreads();
            if (tid < nlow) {
                double a = s_w[0][tid];
                for (int w2 = 1; w2 < BLK / 64; ++w2) a += s_w[w2][tid];
                st_agent(&v.fac_part[((size_t)l * 64 + tid) * nb + blockIdx.x], a);
            }
        }
    }
    // ---- the B0 solve: (FTRAN: the bump first,) level by level (, BTRAN: the bump last)
    unsigned target = 0;
    bool ok = true;
    bool coef_pending = any_dense;  // the partial sums still have to be added up (after the first barrier)
    int barriers = 0;
    const int nbump = v.fac_meta[2];
#define FAC_BARRIER()                                                                             \
    do {                                                                                          \
        target += (unsigned)nb;                                                                   \
        ok = fac_grid_barrier(c, bar, target) && ok;                                              \
        barriers += 1;                                                                            \
        if (coef_pending) {                                                                       \
            coef_pending = false;                                                                 \
            if ((int)blockIdx.x < nlow)                                                           \
                for (int l_ = 0; l_ < nl; ++l_) {                                                 \
                    if (SRC(l_) == 0) continue;                                                   \
                    double a_ = 0.0;                                                              \
                    for (int i_ = tid; i_ < nb; i_ += BLK) a_ += ld_agent(&v.fac_part[((size_t)l_ * 64 + blockIdx.x) * nb + i_]); \
                    a_ = block_sum(a_);                                                           \
                    if (tid == 0) st_agent(&v.fac_coef[l_ * 64 + blockIdx.x], a_);                \
                }                                                                                 \
        }                                                                                         \
    } while (0)
    // (A data-flow walk of the grid's segments — sentinel values + bounded waits instead of a barrier per level — was built and measured in
    // round 5: a hop from one workgroup's store to another's polling load costs ~5 us on this device, the sentinel pass 13 us; the late solve
    // of the config-3 family 424 us against 414, the transport family 15.6 s against 14.3 s.  Removed in round 6.)
    auto ldx = [&](const double* p) -> double { return ld_agent(p); };
    extern __shared__ double s_dyn[];
    double (*const s_bt)[FAC_BMAX] = reinterpret_cast<double (*)[FAC_BMAX]>(s_dyn);  // dense carrier of the bump: its two right-hand sides (the segments
                                                                                     // that use s_dyn never overlap in time)
    // The levels this solve has to walk (lu.rs:432-463: the reference restricts a sparse solve to the REACH of its right-hand side; here
    // the restriction is by level).  x0 is zero outside a solve (the epilogue clears what it read), so a level that is not walked reads
    // as zero.  FTRAN (levels descending): nothing above the highest level of the right-hand side's rows can become non-zero.  BTRAN
    // (ascending): nothing below the lowest level of supp(c), nothing above the highest level a dependent of supp(c) reaches
    // (fac_reach_of_pos, propagated along the edges at the refactorisation).  Measured on the oracle's bases of the transport family:
    // 88 % of the unit-vector BTRANs and 89 % of the column FTRANs end at level <= 4 of 18.  A bump couples everything: full range.
    int lev_lo = 0, lev_hi = nlev - 1;
    if (v.fac_skip) {
        int lo2 = INT_MAX, hi2 = -1;
        for (int l = 0; l < nl; ++l) {
            int a = 0, b = INT_MAX;
            if (dir == 0) {
                b = SRC(l) == 0 ? c->fac_aq_hi : (SRC(l) == 1 ? c->fac_rho_hi : INT_MAX);
            } else if (SRC(l) == 0) {
                a = v.fac_lev_of_pos[r_leave];
                b = v.fac_reach_of_pos[r_leave];
            } else if (SRC(l) == 1) {
                a = c->fac_aq_lo;
                b = c->fac_aq_reach;
            }
            lo2 = min(lo2, a);
            hi2 = max(hi2, b);
        }
        lev_lo = max(0, min(lo2, nlev));
        lev_hi = min(hi2, nlev - 1);
    }
    // Levels [tail, nlev) are all small (<= FAC_TAIL positions: the level sizes of these bases decay geometrically): ONE workgroup
    // walks them with workgroup barriers (~0.3 us) instead of grid barriers.
    const int nsplit = v.fac_meta[4];  // levels [0, nsplit) come from the column steps of the peel, level nsplit is the bump, (nsplit, nlev) the row steps
    auto do_item = [&](int idx) {  // one position of the peel, through its resolved edge list (built at the refactorisation)
        const int p = v.fac_items[idx];
        const int i = v.fac_irow[idx];
        const double piv = v.fac_ipiv[idx];
        const int* eidx = dir == 0 ? v.fac_fidx : v.fac_bidx;   // FTRAN: the other basic columns of the pivot row; BTRAN: the other rows of the column
        const double* eval = dir == 0 ? v.fac_fval : v.fac_bval;
        const int beg = dir == 0 ? v.fac_fptr[idx] : v.fac_bptr[idx], end = dir == 0 ? v.fac_fptr[idx + 1] : v.fac_bptr[idx + 1];
        const int out = dir == 0 ? p : i;
        double accA = 0.0, accB = 0.0;
        for (int e = beg; e < end; ++e) {
            const int t = eidx[e];
            const double a = eval[e];
            accA += a * ldx(&x0a[t]);
            if (nl == 2) accB += a * ldx(&x0b[t]);
        }
        st_agent(&x0a[out], (rhs_of(0, i, p) - accA) / piv);
        if (nl == 2) st_agent(&x0b[out], (rhs_of(1, i, p) - accB) / piv);
    };
    // The walk is a sequence of segments — levels one workgroup walks alone (the small ones), levels the whole grid walks (a grid
    // barrier after each), the bump (one workgroup) — in the order of the triangular form: FTRAN  row-step levels (descending), bump,
    // column-step levels (descending);  BTRAN the reverse.  Work of workgroup 0 alone is followed by a grid barrier only where the grid
    // takes over (`solo`: every workgroup evaluates the same conditions, so all of them pass the same barriers).
    bool solo = false;
    auto join = [&]() {
        if (solo) {
            FAC_BARRIER();
            solo = false;
        }
    };
    // The small levels (at most BLK positions each: the upper column steps and most row steps of the peel) are a chain of 50-150
    // dependent steps on the config-3 family.  Walked through memory a step costs three to four round trips (item -> edge list ->
    // vector -> store acknowledged): 3 us, 400-500 us per solve.  Here workgroup 0 walks a run of small levels in PIECES of at most
    // FAC_TAIL_CAP positions, each in two passes: a PARALLEL pass over the piece's items (FacTailRec records, built at the
    // refactorisation, one coalesced load each) folds the right-hand-side entry and every edge whose target lies outside the piece
    // (final by then) into the item's LDS slot and leaves the item's edges INSIDE the piece in LDS as well; the level-by-level pass
    // then touches LDS only — x = (slot - sum over the edges inside) / pivot — and copies the results out to memory without waiting.
    double* const s_tail_x = s_dyn;                                            // [2][FAC_TAIL_CAP]: the piece's part of the solve vectors
    double* const s_tpiv = s_dyn + 2 * FAC_TAIL_CAP;                           // [FAC_TAIL_CAP] pivots
    double* const s_teval = s_dyn + 3 * FAC_TAIL_CAP;                          // [FAC_TAIL_CAP][FAC_TAIL_K] coefficients of the edges inside the piece
    int* const s_teslot = reinterpret_cast<int*>(s_dyn + (3 + FAC_TAIL_K) * FAC_TAIL_CAP);  // [FAC_TAIL_CAP][FAC_TAIL_K] their (piece-local) slots
    int* const s_tout = s_teslot + FAC_TAIL_K * FAC_TAIL_CAP;                  // [FAC_TAIL_CAP] where the result goes in memory
    int* const s_tnin = s_tout + FAC_TAIL_CAP;                                 // [FAC_TAIL_CAP] edges inside the piece (-1: more than FAC_TAIL_K, walked from the record)
    __shared__ int s_lslot[FAC_SEG_LEVELS], s_lsize[FAC_SEG_LEVELS];
    __shared__ int s_sblptr[FAC_SB_ROUNDS + 2];
    __shared__ int s_trow[FAC_SB_DT], s_tcol[FAC_SB_DT];  // dense tail of the sparse bump factor: its row / column slots
    __shared__ double s_ttmp[2][FAC_SB_DT];
    __shared__ int s_cut;
    auto seg_small = [&](int a, int b) {  // levels [a, b] (a run of small levels) by workgroup 0
        a = max(a, lev_lo);
        b = min(b, lev_hi);
        if (a > b) return;
        solo = true;
        if (blockIdx.x != 0) return;
        const FacTailRec* prog = dir == 0 ? v.fac_tprog_f : v.fac_tprog_b;
        const int* eidx = dir == 0 ? v.fac_fidx : v.fac_bidx;
        const int* eslot = dir == 0 ? v.fac_fslot : v.fac_bslot;
        const double* eval = dir == 0 ? v.fac_fval : v.fac_bval;
        int done = 0;  // levels of the run walked so far (from the end the solve starts at)
        while (done < b - a + 1) {
            // the next piece: up to FAC_SEG_LEVELS levels from the walking end, cut where FAC_TAIL_CAP positions are full
            const int nwin = min(FAC_SEG_LEVELS, b - a + 1 - done);
            const int w0 = dir == 0 ? b - done - nwin + 1 : a + done;  // lowest level of the window
            if (tid == 0) s_cut = 1;  // (a level holds at most FAC_TAIL <= FAC_TAIL_CAP positions: the first always fits)
            for (int t = tid; t < nwin; t += BLK) {
                s_lslot[t] = v.fac_ltslot[w0 + t];
                s_lsize[t] = v.fac_lptr[w0 + t + 1] - v.fac_lptr[w0 + t];
            }
            __syncthreads();
            for (int t = tid; t < nwin; t += BLK) {  // (slots ascend with the level: the positions from the walking end to level t)
                const int span = dir == 0 ? s_lslot[nwin - 1] + s_lsize[nwin - 1] - s_lslot[nwin - 1 - t] : s_lslot[t] + s_lsize[t] - s_lslot[0];
                if (span <= FAC_TAIL_CAP) atomicMax(&s_cut, t + 1);
            }
            __syncthreads();
            const int nsteps = s_cut;
            const int o = dir == 0 ? nwin - nsteps : 0;  // the piece = window levels [o, o + nsteps)
            const int slot_lo = s_lslot[o], slot_hi = s_lslot[o + nsteps - 1] + s_lsize[o + nsteps - 1];
            // pass 1 (parallel over the piece): right-hand side, the edges that leave the piece, the edges inside into LDS
            for (int k = slot_lo + tid; k < slot_hi; k += BLK) {
                const FacTailRec r = prog[k];
                const int q = k - slot_lo;
                const int nall = (int)((unsigned)r.out_n >> 24), n = min(nall, FAC_TAIL_INLINE);
                double accA = 0.0, accB = 0.0;
                int nin = 0;
#pragma unroll
                for (int e = 0; e < FAC_TAIL_INLINE; ++e) {
                    if (e < n) {
                        if (r.slot[e] < slot_lo || r.slot[e] >= slot_hi) {
                            accA += r.val[e] * ldx(&x0a[r.tgt[e]]);
                            if (nl == 2) accB += r.val[e] * ldx(&x0b[r.tgt[e]]);
                        } else {
                            if (nin < FAC_TAIL_K) {
                                s_teslot[q * FAC_TAIL_K + nin] = r.slot[e] - slot_lo;
                                s_teval[q * FAC_TAIL_K + nin] = r.val[e];
                            }
                            nin += 1;
                        }
                    }
                }
                if (r.ovf >= 0) {  // (a long edge list: the edges beyond the inline ones, from the lists in memory)
                    for (int e = r.ovf; e < r.ovf + nall - FAC_TAIL_INLINE; ++e) {
                        const int sl = eslot[e];
                        if (sl < slot_lo || sl >= slot_hi) {
                            accA += eval[e] * ldx(&x0a[eidx[e]]);
                            if (nl == 2) accB += eval[e] * ldx(&x0b[eidx[e]]);
                        } else {
                            if (nin < FAC_TAIL_K) {
                                s_teslot[q * FAC_TAIL_K + nin] = sl - slot_lo;
                                s_teval[q * FAC_TAIL_K + nin] = eval[e];
                            }
                            nin += 1;
                        }
                    }
                }
                s_tail_x[q] = rhs_of(0, r.rhs, r.rhs) - accA;
                if (nl == 2) s_tail_x[FAC_TAIL_CAP + q] = rhs_of(1, r.rhs, r.rhs) - accB;
                s_tpiv[q] = r.piv;
                s_tout[q] = r.out_n & 0xFFFFFF;
                s_tnin[q] = nin <= FAC_TAIL_K ? nin : -1;
            }
            __syncthreads();
            // pass 2: level by level inside LDS
            for (int step = 0; step < nsteps; ++step) {
                const int li = o + (dir == 0 ? nsteps - 1 - step : step);
                if (tid < s_lsize[li]) {
                    const int q = s_lslot[li] + tid - slot_lo;
                    const int nin = s_tnin[q];
                    double accA = 0.0, accB = 0.0;
                    if (nin >= 0) {
#pragma unroll
                        for (int e = 0; e < FAC_TAIL_K; ++e)
                            if (e < nin) {
                                const int sl = s_teslot[q * FAC_TAIL_K + e];
                                const double a = s_teval[q * FAC_TAIL_K + e];
                                accA += a * s_tail_x[sl];
                                if (nl == 2) accB += a * s_tail_x[FAC_TAIL_CAP + sl];
                            }
                    } else {  // (rare: more edges inside the piece than the LDS copy holds — from the record and the lists)
                        const FacTailRec r = prog[slot_lo + q];
                        const int nall = (int)((unsigned)r.out_n >> 24), n = min(nall, FAC_TAIL_INLINE);
                        for (int e = 0; e < n; ++e)
                            if (r.slot[e] >= slot_lo && r.slot[e] < slot_hi) {
                                accA += r.val[e] * s_tail_x[r.slot[e] - slot_lo];
                                if (nl == 2) accB += r.val[e] * s_tail_x[FAC_TAIL_CAP + r.slot[e] - slot_lo];
                            }
                        if (r.ovf >= 0)
                            for (int e = r.ovf; e < r.ovf + nall - FAC_TAIL_INLINE; ++e) {
                                const int sl = eslot[e];
                                if (sl >= slot_lo && sl < slot_hi) {
                                    accA += eval[e] * s_tail_x[sl - slot_lo];
                                    if (nl == 2) accB += eval[e] * s_tail_x[FAC_TAIL_CAP + sl - slot_lo];
                                }
                            }
                    }
                    const double piv = s_tpiv[q];
                    const int out = s_tout[q];
                    const double ra = (s_tail_x[q] - accA) / piv;
                    s_tail_x[q] = ra;
                    st_agent(&x0a[out], ra);
                    if (nl == 2) {
                        const double rb = (s_tail_x[FAC_TAIL_CAP + q] - accB) / piv;
                        s_tail_x[FAC_TAIL_CAP + q] = rb;
                        st_agent(&x0b[out], rb);
                    }
                }
                lds_barrier();  // (the copies to memory stay in flight: they are waited for once, below)
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the copies in memory have landed before the next piece / the bump / the grid reads them
            __syncthreads();
            done += nsteps;
        }
    };
    auto seg_grid = [&](int a, int b) {  // levels [a, b] by the whole grid
        a = max(a, lev_lo);
        b = min(b, lev_hi);
        if (a > b) return;
        join();
        // Everything of an item except the entries of the solve vector it pulls is known before the solve reaches its level: its place,
        // pivot, right-hand-side entries and (up to four) edges.  A lane loads that for its first item of the NEXT level before it
        // arrives at the barrier, so the chain after the barrier is vector gather -> store instead of item -> edge list -> vector ->
        // store (a level of the grid cost 7 us: barrier 2.5 + four dependent round trips).
        constexpr int GE = 4;
        struct GItem { int out, n, beg; double piv, rA, rB; int t[GE]; double a[GE]; };
        const int* eidx = dir == 0 ? v.fac_fidx : v.fac_bidx;
        const double* eval = dir == 0 ? v.fac_fval : v.fac_bval;
        const int* eptr = dir == 0 ? v.fac_fptr : v.fac_bptr;
        auto pre = [&](int lev, GItem& g) -> bool {
            const int idx = v.fac_lptr[lev] + (int)blockIdx.x * BLK + tid;
            const bool ok = idx < v.fac_lptr[lev + 1];
            const int ix = ok ? idx : v.fac_lptr[lev];  // (branch-free loads; a level of the list is never empty)
            const int p = v.fac_items[ix], i = v.fac_irow[ix];
            g.piv = v.fac_ipiv[ix];
            g.beg = eptr[ix];
            g.n = eptr[ix + 1] - g.beg;
            g.out = dir == 0 ? p : i;
            g.rA = rhs_of(0, i, p);
            g.rB = nl == 2 ? rhs_of(1, i, p) : 0.0;
#pragma unroll
            for (int e = 0; e < GE; ++e) {
                const int ee = g.beg + min(e, max(g.n - 1, 0));
                g.t[e] = g.n > 0 ? eidx[ee] : 0;
                g.a[e] = g.n > 0 ? eval[ee] : 0.0;
            }
            return ok;
        };
        auto fin = [&](const GItem& g) {
            double accA = 0.0, accB = 0.0;
#pragma unroll
            for (int e = 0; e < GE; ++e)
                if (e < g.n) {
                    accA += g.a[e] * ldx(&x0a[g.t[e]]);
                    if (nl == 2) accB += g.a[e] * ldx(&x0b[g.t[e]]);
                }
            for (int e = g.beg + GE; e < g.beg + g.n; ++e) {
                const int t = eidx[e];
                const double a2 = eval[e];
                accA += a2 * ldx(&x0a[t]);
                if (nl == 2) accB += a2 * ldx(&x0b[t]);
            }
            st_agent(&x0a[g.out], (g.rA - accA) / g.piv);
            if (nl == 2) st_agent(&x0b[g.out], (g.rB - accB) / g.piv);
        };
        // (two items in alternating roles, the loop unrolled by two: the next level's static loads are issued BEFORE this level's gathers, so
        // the two chains run side by side; no copies of an item, which would make the compiler wait for every load in flight)
        auto level_of = [&](int step) { return dir == 0 ? b - step : a + step; };
        auto extras = [&](int lev) {  // (a level beyond one item per lane)
            const int lo = v.fac_lptr[lev], hi = v.fac_lptr[lev + 1];
            for (int idx = lo + (int)blockIdx.x * BLK + tid + nb * BLK; idx < hi; idx += nb * BLK) do_item(idx);
        };
        const int last = b - a;
        GItem g0, g1;
        bool h0 = pre(level_of(0), g0), h1 = false;
        for (int step = 0; step <= last; step += 2) {
            if (step + 1 <= last) h1 = pre(level_of(step + 1), g1);
            if (h0) fin(g0);
            extras(level_of(step));
            FAC_BARRIER();
            if (step + 1 > last) break;
            if (step + 2 <= last) h0 = pre(level_of(step + 2), g0);
            if (h1) fin(g1);
            extras(level_of(step + 1));
            FAC_BARRIER();
        }
    };
    auto seg_bump = [&]() {
        if (nbump <= 0 || nsplit < lev_lo || nsplit > lev_hi) return;
        solo = true;
        if (blockIdx.x != 0) return;
        if (v.fac_meta[8]) {
            // SPARSE FACTOR of the bump (factor_sb.inc): the same two right-hand sides, then the rounds of the elimination as levels —
            // FTRAN: L ascending, U descending; BTRAN: U^T ascending, L^T descending — on vectors in LDS.
            // vectors in LDS, addressed by OFFSET into s_dyn (pointer tables would live in scratch and turn every access into a flat load):
            // P = by ROW slot: t -> y (FTRAN), w -> y (BTRAN) at 0, Q = by COLUMN slot: x (FTRAN), c (BTRAN) at nbump; second right-hand
            // side 2 nbump further
            const int oP = 0, oQ = nbump, oL = 2 * nbump;
            // one item in pull form: out = (rhs - sum over its edges) / piv
            auto sb_apply = [&](const FacSbRec& rc, int od, int orh, bool same) {
                if (same && rc.n == 0) return;  // (L / L^T item without edges: the value stays)
                double accA = 0.0, accB = 0.0;
#pragma unroll
                for (int e = 0; e < FAC_SB_INL; ++e)
                    if (e < rc.n) {
                        accA += rc.val[e] * s_dyn[od + rc.idx[e]];
                        if (nl == 2) accB += rc.val[e] * s_dyn[od + oL + rc.idx[e]];
                    }
                // (the edges beyond the inline ones, eight loads in flight at a time: one at a time was a memory round trip per edge, and
                // the long lists — rows and multiplier lists of the last rounds — sit one per level on the critical path)
                for (int e0 = FAC_SB_INL; e0 < rc.n; e0 += 8) {
                    int ti[8];
                    double ta[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int ee = min(e0 + u, rc.n - 1) - FAC_SB_INL;
                        ti[u] = v.fac_sb_oidx[rc.ovf + ee];
                        ta[u] = v.fac_sb_oval[rc.ovf + ee];
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (e0 + u < rc.n) {
                            accA += ta[u] * s_dyn[od + ti[u]];
                            if (nl == 2) accB += ta[u] * s_dyn[od + oL + ti[u]];
                        }
                }
                const double ra = (s_dyn[orh + rc.rhs] - accA) / rc.piv;
                double rb = 0.0;
                if (nl == 2) rb = (s_dyn[orh + oL + rc.rhs] - accB) / rc.piv;
                s_dyn[od + rc.out] = ra;
                if (nl == 2) s_dyn[od + oL + rc.out] = rb;
            };
            {   // the right-hand side of the bump from its resolved record (factor_sb.inc, kinds 4 / 5): FTRAN t[u] = b[row] - the row-step
                // columns on the row, BTRAN c[s] = c[position] - the column's entries on pivot rows of the peel
                const FacSbRec* rr = v.fac_sb_rec + (size_t)(dir == 0 ? 4 : 5) * FAC_SB_MAX;
                const int o2 = dir == 0 ? oP : oQ;
                const bool edges = dir == 1 || nsplit + 1 < nlev;
                for (int t = tid; t < nbump; t += BLK) {
                    const FacSbRec rc = rr[t];
                    double accA = 0.0, accB = 0.0;
                    if (edges) {
#pragma unroll
                        for (int e = 0; e < FAC_SB_INL; ++e)
                            if (e < rc.n) {
                                accA += rc.val[e] * ldx(&x0a[rc.idx[e]]);
                                if (nl == 2) accB += rc.val[e] * ldx(&x0b[rc.idx[e]]);
                            }
                        for (int e = FAC_SB_INL; e < rc.n; ++e) {
                            const int t2 = v.fac_sb_oidx[rc.ovf + e - FAC_SB_INL];
                            const double a = v.fac_sb_oval[rc.ovf + e - FAC_SB_INL];
                            accA += a * ldx(&x0a[t2]);
                            if (nl == 2) accB += a * ldx(&x0b[t2]);
                        }
                    }
                    s_dyn[o2 + t] = rhs_of(0, rc.rhs, rc.rhs) - accA;
                    if (nl == 2) s_dyn[o2 + oL + t] = rhs_of(1, rc.rhs, rc.rhs) - accB;
                }
            }
            const int nr = v.fac_meta[9];                 // rounds of the sparse elimination
            const int ntl = v.fac_meta[10];               // rows x columns of the dense tail: one more level behind the rounds
            const int nlv = nr + (ntl > 0 ? 1 : 0);
            for (int t = tid; t <= nlv; t += BLK) s_sblptr[t] = v.fac_sb_lptr[t];  // (the level table: read per level below)
            if (tid < ntl) {
                s_trow[tid] = v.fac_sb_trow[tid];
                s_tcol[tid] = v.fac_sb_tcol[tid];
            }
            __syncthreads();
            KMARK0(c, 20);
            // `count` levels from `first` in direction `dirn`, items of kind `kind`: results to (and edges from) the vector at od, the
            // right-hand-side entry from the vector at orh.  The records do not depend on the solve: a lane's first item of the next TWO
            // levels is in flight during a level's arithmetic (three records in rotating ROLES, the loop unrolled by three: copying a record
            // to rotate it made the compiler drain every load in flight at the loop head)
            auto walk = [&](int kind, int od, int orh, int first, int count, int dirn) {
                const FacSbRec* rec = v.fac_sb_rec + (size_t)kind * FAC_SB_MAX;
                const bool same = od == orh;
                auto lvl = [&](int step) { return first + dirn * step; };
                auto fetch = [&](int step, FacSbRec& rc) -> bool {  // (branch-free: the load is always issued, so it can stay in flight)
                    const int sc = min(step, count - 1);
                    const int q = s_sblptr[lvl(sc)] + tid;
                    const bool okf = step < count && q < s_sblptr[lvl(sc) + 1];
                    rc = rec[okf ? q : 0];
                    return okf;
                };
                auto stage = [&](int step, const FacSbRec& rc, bool have) {
                    const int lo = s_sblptr[lvl(step)], hi = s_sblptr[lvl(step) + 1];
                    if (have) sb_apply(rc, od, orh, same);
                    for (int q = lo + tid + BLK; q < hi; q += BLK) {
                        const FacSbRec rx = rec[q];
                        sb_apply(rx, od, orh, same);
                    }
                    lds_barrier();
                };
                if (count <= 0) return;
                FacSbRec r0, r1, r2;
                bool h0 = fetch(0, r0), h1 = fetch(1, r1), h2 = false;
                for (int step = 0; step < count; step += 3) {
                    h2 = fetch(step + 2, r2);
                    stage(step, r0, h0);
                    if (step + 1 >= count) break;
                    h0 = fetch(step + 3, r0);
                    stage(step + 1, r1, h1);
                    if (step + 2 >= count) break;
                    h1 = fetch(step + 4, r1);
                    stage(step + 2, r2, h2);
                }
            };
            if (dir == 0) {
                walk(0, oP, oP, 0, nlv, 1);  // L: the rounds ascending, then the tail's rows take their multipliers
                KMARK0(c, 21);
                if (ntl > 0) {  // x[tail columns] = K_t^-1 y[tail rows] (the transposed copy: consecutive lanes read consecutive words)
                    if (tid < ntl) {
                        double a0 = 0.0, a1 = 0.0;
                        for (int a = 0; a < ntl; a += 8) {
                            double wv[8];
#pragma unroll
                            for (int u = 0; u < 8; ++u) wv[u] = v.fac_sb_tinvT[(size_t)min(a + u, ntl - 1) * FAC_SB_DT + tid];
#pragma unroll
                            for (int u = 0; u < 8; ++u)
                                if (a + u < ntl) {
                                    a0 += wv[u] * s_dyn[oP + s_trow[a + u]];
                                    if (nl == 2) a1 += wv[u] * s_dyn[oP + oL + s_trow[a + u]];
                                }
                        }
                        s_dyn[oQ + s_tcol[tid]] = a0;
                        if (nl == 2) s_dyn[oQ + oL + s_tcol[tid]] = a1;
                    }
                    lds_barrier();
                }
                walk(1, oQ, oP, nr - 1, nr, -1);  // U: the rounds descending
            } else {
                walk(2, oP, oQ, 0, nlv, 1);  // U^T: the rounds ascending, then the tail's columns take their entries on frozen rows
                KMARK0(c, 21);
                if (ntl > 0) {  // y[tail rows] = K_t^-T t[tail columns] (t sits at the row slot its column is paired with)
                    if (tid < ntl) {
                        s_ttmp[0][tid] = s_dyn[oP + s_trow[tid]];
                        if (nl == 2) s_ttmp[1][tid] = s_dyn[oP + oL + s_trow[tid]];
                    }
                    lds_barrier();
                    if (tid < ntl) {
                        double a0 = 0.0, a1 = 0.0;
                        for (int b2 = 0; b2 < ntl; b2 += 8) {
                            double wv[8];
#pragma unroll
                            for (int u = 0; u < 8; ++u) wv[u] = v.fac_sb_tinv[(size_t)min(b2 + u, ntl - 1) * FAC_SB_DT + tid];
#pragma unroll
                            for (int u = 0; u < 8; ++u)
                                if (b2 + u < ntl) {
                                    a0 += wv[u] * s_ttmp[0][b2 + u];
                                    if (nl == 2) a1 += wv[u] * s_ttmp[1][b2 + u];
                                }
                        }
                        s_dyn[oP + s_trow[tid]] = a0;
                        if (nl == 2) s_dyn[oP + oL + s_trow[tid]] = a1;
                    }
                    lds_barrier();
                }
                walk(3, oP, oP, nr - 1, nr, -1);  // L^T: the rounds descending
            }
            KMARK0(c, 22);
            if (dir == 0) {
                for (int s2 = tid; s2 < nbump; s2 += BLK) {
                    st_agent(&x0a[v.fac_bpos[s2]], s_dyn[oQ + s2]);
                    if (nl == 2) st_agent(&x0b[v.fac_bpos[s2]], s_dyn[oQ + oL + s2]);
                }
            } else {
                for (int u = tid; u < nbump; u += BLK) {
                    st_agent(&x0a[v.fac_brow[u]], s_dyn[oP + u]);
                    if (nl == 2) st_agent(&x0b[v.fac_brow[u]], s_dyn[oP + oL + u]);
                }
            }
        } else if (dir == 0) {
            // x_b = K^-1 (b[bump rows] - entries of the row-step columns on those rows): one workgroup, a wave per bump slot, fixed order
            // (a bump row holds bump columns and columns removed by row steps — a column-step column has no entry on a row that
            // stayed active — and the row-step levels have just been walked)
            for (int t = tid; t < nbump; t += BLK) {
                const int i = v.fac_brow[t];
                double accA = 0.0, accB = 0.0;
                if (nsplit + 1 < nlev)
                    for (int e = v.csr_ptr[i]; e < v.csr_ptr[i + 1]; ++e) {
                        const int p2 = v.fac_pos_of_var[v.csr_col[e]];
                        if (p2 >= 0 && v.fac_lev_of_pos[p2] != nsplit) {
                            accA += v.csr_val[e] * ldx(&x0a[p2]);
                            if (nl == 2) accB += v.csr_val[e] * ldx(&x0b[p2]);
                        }
                    }
                s_bt[0][t] = rhs_of(0, i, 0) - accA;
                if (nl == 2) s_bt[1][t] = rhs_of(1, i, 0) - accB;
            }
            __syncthreads();
            // (through the TRANSPOSE of the inverse: a lane per bump slot walks a column, coalesced across the lanes and with independent
            // loads — the wave-per-slot form over the rows cost 140 us at b = 205: one dependent load -> reduce -> store chain per slot)
            for (int s2 = tid; s2 < nbump; s2 += BLK) {
                double a0 = 0.0, a1 = 0.0;
                int t = 0;
                for (; t + 8 <= nbump; t += 8) {  // eight independent loads in flight, both right-hand sides share them
                    double w[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) w[u] = v.fac_WbT[(size_t)(t + u) * FAC_BMAX + s2];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        a0 += w[u] * s_bt[0][t + u];
                        if (nl == 2) a1 += w[u] * s_bt[1][t + u];
                    }
                }
                for (; t < nbump; ++t) {
                    const double w = v.fac_WbT[(size_t)t * FAC_BMAX + s2];
                    a0 += w * s_bt[0][t];
                    if (nl == 2) a1 += w * s_bt[1][t];
                }
                st_agent(&x0a[v.fac_bpos[s2]], a0);
                if (nl == 2) st_agent(&x0b[v.fac_bpos[s2]], a1);
            }
        } else {
            // t_b = c_b - F^T y (pull along the bump columns over their entries on the pivot rows of the column steps; they have none on
            // the rows of the row steps), then y[bump rows] = K^-T t_b
            for (int s2 = tid; s2 < nbump; s2 += BLK) {
                const int p = v.fac_bpos[s2];
                const int var = v.fac_var_of_pos[p];
                double accA = 0.0, accB = 0.0;
                for (int e = v.csc_ptr[var]; e < v.csc_ptr[var + 1]; ++e) {
                    const int row = v.csc_row[e];
                    if (v.fac_bslot_of_row[row] < 0) {
                        accA += v.csc_val[e] * ldx(&x0a[row]);
                        if (nl == 2) accB += v.csc_val[e] * ldx(&x0b[row]);
                    }
                }
                s_bt[0][s2] = rhs_of(0, 0, p) - accA;
                if (nl == 2) s_bt[1][s2] = rhs_of(1, 0, p) - accB;
            }
            __syncthreads();
            for (int u = tid; u < nbump; u += BLK) {
                double a0 = 0.0, a1 = 0.0;
                int s2 = 0;
                for (; s2 + 8 <= nbump; s2 += 8) {
                    double w[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) w[j] = v.fac_Wb[(size_t)(s2 + j) * FAC_BMAX + u];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        a0 += w[j] * s_bt[0][s2 + j];
                        if (nl == 2) a1 += w[j] * s_bt[1][s2 + j];
                    }
                }
                for (; s2 < nbump; ++s2) {
                    const double w = v.fac_Wb[(size_t)s2 * FAC_BMAX + u];
                    a0 += w * s_bt[0][s2];
                    if (nl == 2) a1 += w * s_bt[1][s2];
                }
                st_agent(&x0a[v.fac_brow[u]], a0);
                if (nl == 2) st_agent(&x0b[v.fac_brow[u]], a1);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    };
    // the host's segment list (ascending levels): runs of small levels (workgroup 0, LDS), runs of other levels (the grid), the bump
    const int nseg = v.fac_meta[7];
    const int km = dir * 10;
    KMARK0(c, km + 1);
    for (int sg = 0; sg < nseg; ++sg) {
        const int q = dir == 0 ? nseg - 1 - sg : sg;
        const int kind = v.fac_segs[3 * q], a = v.fac_segs[3 * q + 1], b = v.fac_segs[3 * q + 2];
        if (kind == 2) seg_bump();
        else if (kind == 1) seg_small(a, b);
        else seg_grid(a, b);
        if (sg < 5) KMARK0(c, km + 2 + sg);
    }
    join();
    KMARK0(c, km + 7);
    // (the coefficients are read below: at least one barrier after the direct form, two after the partial sums)
    while (barriers < (any_dense ? 2 : 1)) FAC_BARRIER();
#undef FAC_BARRIER
    // ---- result = B0 solve + sum_j (U_j | V_j) coef_j, in term order; ||rho||^2 on the way
    // (a term whose coefficient is an exact zero — the usual case with a sparse right-hand side: its V_j / U_j does not meet the
    // support — adds exact zeros: it is skipped, same bits, a fraction of the reads)
    __shared__ int s_cj[2][64];
    __shared__ int s_ncj[2];
    if (tid < 64)
        for (int l = 0; l < nl; ++l) s_coef[l][tid] = tid < nlow ? ld_agent(&v.fac_coef[l * 64 + tid]) : 0.0;
    __syncthreads();
    if (tid < nl) {
        int n2 = 0;
        for (int j = 0; j < nlow; ++j)
            if (s_coef[tid][j] != 0.0) s_cj[tid][n2++] = j;
        s_ncj[tid] = n2;
    }
    __syncthreads();
    const double* T = dir == 0 ? v.fac_U : v.fac_V;
    double sq = 0.0;
    int st_hi = -1, st_lo = INT_MAX, st_reach = -1;  // level statistics of lane A's result (the right-hand side of a later solve)
    // rho = B^-T e_r of a dual iteration: its entries stay in registers for the partial sums of V_j . rho (see the coefficient stage)
    constexpr int RT = 8;  // trips of the loop below a lane may make (m <= RT x grid x BLK, else the FTRAN forms the sums itself)
    const bool rho_part = dir == 1 && dstA == 0 && srcA == 0 && !always && !(fuse & 8) && nlow > 0 && (long)m <= (long)RT * nb * BLK;
    double rk[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) rk[t] = 0.0;
    int trip = 0;
    // (the B0 solve's entries of FOUR trips are loaded before the first trip's stores: the stores may alias as far as the compiler knows,
    // so the loop was one memory round trip after the other, three or four of them at 200 000 rows)
    constexpr int CH = 4;
    const int stride = nb * BLK;
    for (int base = (int)blockIdx.x * BLK + tid; base < m; base += CH * stride) {
      double xa[CH][2];
#pragma unroll
      for (int u = 0; u < CH; ++u) {
          const int i2 = base + u * stride;
          xa[u][0] = i2 < m ? ld_agent(&x0a[i2]) : 0.0;
          xa[u][1] = (nl == 2 && i2 < m) ? ld_agent(&x0b[i2]) : 0.0;
      }
      // (term by term for the four rows at once — four independent loads per term; per row the same sums in the same order)
#pragma unroll
      for (int l = 0; l < 2; ++l) {
          if (l >= nl) break;
          const int ncj = s_ncj[l];
          for (int jj = 0; jj < ncj; ++jj) {
              const int j = s_cj[l][jj];
              const double cf = s_coef[l][j], iv = s_inv[j];
              double tv[CH];
#pragma unroll
              for (int u = 0; u < CH; ++u) tv[u] = base + u * stride < m ? T[(size_t)j * m + base + u * stride] : 0.0;
#pragma unroll
              for (int u = 0; u < CH; ++u) {
                  double t2 = tv[u];
                  if (dir == 0) t2 = -t2 * iv;
                  xa[u][l] += t2 * cf;
              }
          }
      }
#pragma unroll
      for (int u = 0; u < CH; ++u) {
        const int idx = base + u * stride;
        if (idx >= m) break;
        for (int l = 0; l < nl; ++l) {
            const double xv = l == 0 ? xa[u][0] : xa[u][1];
            X0(l)[idx] = 0.0;  // (zero outside a solve: the levels a later solve skips read as zero)
            if (dir == 0) {
                if (DST(l) == 0) {
                    v.alpha_q[idx] = xv;
                    if ((fuse & 4) && nlow < v.fac_J) {  // the pivot's eta transformation as the next rank-1 term (k_fac_append's work)
                        v.fac_U[(size_t)nlow * m + idx] = xv - (idx == r_leave ? 1.0 : 0.0);
                        v.fac_V[(size_t)nlow * m + idx] = v.rv[idx].x;
                    }
                    if (idx == r_leave) {
                        if (fuse & 2) {  // plan_update of the compact factor (k_post_ftran's work)
                            c->it.inv_alpha = 1.0 / xv;
                            c->it.alpha_sq = 1.0;
                            c->fold = 0;
                            c->up.kase = -1;
                            c->up.r = r_leave;
                        }
                        if ((fuse & 4) && nlow < v.fac_J) c->fac_inv[nlow] = 1.0 / xv;
                    }
                } else {
                    v.tau[idx] = xv;
                }
            } else {
                if (DST(l) == 0) {
                    v.rv[idx].x = xv;
                    if (rho_part) {
#pragma unroll
                        for (int t = 0; t < RT; ++t)
                            if (t == trip) rk[t] = xv;
                    }
                } else {
                    v.rv[idx].y = xv;
                }
            }
            if (l == 0) {
                sq += xv * xv;
                if (xv != 0.0 && dstA == 0) {
                    if (dir == 1) {
                        const int lv = v.fac_lev_of_row[idx];
                        st_hi = max(st_hi, lv < 0 ? INT_MAX : lv);
                    } else {
                        const int lv = v.fac_lev_of_pos[idx];
                        st_lo = min(st_lo, lv < 0 ? 0 : lv);
                        st_reach = max(st_reach, lv < 0 ? INT_MAX : v.fac_reach_of_pos[idx]);
                    }
                }
            }
        }
        ++trip;
      }
    }
    if (rho_part) {
        bool mine = false;
#pragma unroll
        for (int t = 0; t < RT; ++t) mine = mine || rk[t] != 0.0;
        const bool any_here = __syncthreads_or(mine ? 1 : 0) != 0;  // (rho is sparse: most workgroups hold none of it and leave zeros)
        if (any_here) {
            const int wv = tid >> 6, ln = tid & 63;
            for (int j0 = 0; j0 < nlow; j0 += 8) {
                double acc[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] = 0.0;
#pragma unroll
                for (int t = 0; t < RT; ++t) {
                    const int idx = (int)blockIdx.x * BLK + tid + t * nb * BLK;
                    if (rk[t] != 0.0) {  // (a zero entry adds an exact zero in the dense pass)
#pragma unroll
                        for (int u = 0; u < 8; ++u)
                            if (j0 + u < nlow) acc[u] += v.fac_V[(size_t)(j0 + u) * m + idx] * rk[t];
                    }
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[u] = wave_sum(acc[u]);
                if (ln == 0) {
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (j0 + u < nlow) s_w[wv][j0 + u] = acc[u];
                }
            }
            __syncthreads();
            if (tid < nlow) {
                double a = s_w[0][tid];
                for (int w2 = 1; w2 < BLK / 64; ++w2) a += s_w[w2][tid];
                st_agent(&v.fac_part[((size_t)2 * 64 + tid) * nb + blockIdx.x], a);
            }
        } else if (tid < nlow) {
            st_agent(&v.fac_part[((size_t)2 * 64 + tid) * nb + blockIdx.x], 0.0);
        }
    }
    if (dstA == 0) {  // order-independent integer reductions: wave shuffles, one atomic per wave
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            st_hi = max(st_hi, __shfl_down(st_hi, o, 64));
            st_lo = min(st_lo, __shfl_down(st_lo, o, 64));
            st_reach = max(st_reach, __shfl_down(st_reach, o, 64));
        }
        if ((tid & 63) == 0) {
            if (dir == 1) {
                if (st_hi >= 0) atomicMax(&c->fac_rho_hi, st_hi);
            } else {
                if (st_lo != INT_MAX) atomicMin(&c->fac_aq_lo, st_lo);
                if (st_reach >= 0) atomicMax(&c->fac_aq_reach, st_reach);
            }
        }
    }
    if (dir == 0 && (srcA == 0 || srcB == 0) && blockIdx.x == 0) {  // the head scattered the entering column into fac_rhs: clear it again
        const int var = c->it.entering_var;
        const int end = v.csc_ptr[var + 1];
        for (int e = v.csc_ptr[var] + tid; e < end; e += BLK) v.fac_rhs[v.csc_row[e]] = 0.0;
    }
    sq = block_sum(sq);
    if (tid == 0) st_agent(&v.red_key[blockIdx.x], sq);
    KMARK0(c, dir * 10 + 8);
    // ---- the last workgroup to finish closes the solve: fixed-order sum of the partials, barrier counter back to zero
    if (!last_block_arrives(&v.fac_bar[1], (unsigned)nb)) return;
    double s = 0.0;
    for (int i = tid; i < nb; i += BLK) s += ld_agent(&v.red_key[i]);
    s = block_sum(s);
    if (tid == 0) {
        if (dir == 1 && dstA == 0) c->it.rho_sq = s;
        if (dir == 1 && dstA == 0) {  // (the partial sums describe THIS rho with THIS many terms)
            c->fac_rho_part_n = nlow;
            c->fac_rho_part_ok = rho_part ? 1 : 0;
        }
        if (dir == 0 && (srcA == 1 || srcB == 1)) c->fac_rho_part_ok = 0;
        if ((fuse & 4) && (ok || always)) {
            if (nlow < v.fac_J) {
                c->nlow = nlow + 1;
            } else {  // the host failed to refactor in time (as in k_fac_append)
                c->it.status = ITER_SINGULAR;
                c->halt = 1;
                push_rec(c, 0);
            }
        }
        fac_bar_reset(v.fac_bar);
        // the statistics this solve consumed start afresh (every workgroup read them before its first barrier)
        if (dir == 0 && (srcA == 1 || srcB == 1)) c->fac_rho_hi = -1;
        if (dir == 1 && (srcA == 1 || srcB == 1)) {
            c->fac_aq_lo = INT_MAX;
            c->fac_aq_reach = -1;
        }
        if (!ok && !always) {  // a barrier gave up: the grid was not co-resident.  Nothing of this iteration is applied.
            c->it.status = ITER_STALL;
            c->halt = 1;
            push_rec(c, 0);
        }
    }
}
// Processes that run this persistent grid on the SAME device (a sharded solve whose ranks share a GPU and keep the factor:
// MLP_FACTOR_SHARED_DEVICE).  A workgroup takes a whole CU's LDS, so two full grids of two processes cannot be resident together: each
// gets a part of the CUs, every grid barrier waits for workgroups that cannot start until the other grid leaves, and the waiters give up
// at the spin bound with a half-done solve (both ranks of the 20-pivot test then found "no entering column" on a feasible model).  The
// grids are therefore sized to fit side by side: CUs / sharers workgroups each (never fewer than the 64 pending terms need).
static int g_fac_sharers = 1;
void fac_solve_set_sharers(int n) { g_fac_sharers = n < 1 ? 1 : n; }
static int fac_grid_blocks_full();
static int fac_grid_blocks() {
    const int full = fac_grid_blocks_full();
    if (g_fac_sharers <= 1) return full;
    const int part = full / g_fac_sharers;
    return part >= 64 ? part : (full < 64 ? full : 64);
}
static int fac_grid_blocks_full() {
    static int n = 0;
    if (n == 0) {
        int dev = 0, cus = 0;
        // workgroups per CU: measured at 200 000 rows — one per CU: 394 ... 905 us per pivot over the solve, four per CU:
        // 429 ... 1 701 (the grid barrier's cost grows with the number of arriving workgroups faster than the extra waves hide latency)
        // (at 128 KB of dynamic LDS per workgroup only ONE is co-resident per CU: more would not fit the persistent grid its barriers need)
        static const int per_cu = 1;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) n = cus * per_cu;
        else n = 64;
        if (n > 1024) n = 1024;  // (the partial sums travel through red_key: >= 1024 entries)
    }
    return n;
}
int fac_solve_grid_blocks() { return fac_grid_blocks(); }
constexpr size_t FAC_TAIL_LDS = sizeof(double) * (3 + FAC_TAIL_K) * FAC_TAIL_CAP + sizeof(int) * (FAC_TAIL_K + 2) * FAC_TAIL_CAP;  // the piece of a run of small levels
constexpr size_t FAC_SB_LDS = sizeof(double) * 4 * FAC_SB_MAX;  // sparse bump factor: two vectors per right-hand side
constexpr size_t FAC_SOLVE_LDS = FAC_TAIL_LDS > FAC_SB_LDS ? FAC_TAIL_LDS : FAC_SB_LDS;
// gfx950 has 160 KB of LDS per workgroup; the solve asks for FAC_SOLVE_LDS = 128 KB dynamic + ~10 KB static.  A device that cannot grant it
// cannot run the compact factor at all: say so once, loudly, instead of leaving every solve to fail at launch (the engine then sees
// hipErrorLaunchFailure from pull_ctl without a cause).
static void fac_solve_lds_attr() {
    static bool done = false;
    if (!done) {
        int dev = 0, lds = 0;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
        const hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void*>(k_fac_solve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)FAC_SOLVE_LDS);
        const hipError_t e2 = hipSuccess;
        if (e1 != hipSuccess || e2 != hipSuccess || (lds > 0 && (size_t)lds < FAC_SOLVE_LDS + 12 * 1024)) {
            (void)hipGetLastError();
            std::fprintf(stderr, "[mlp] compact factor: k_fac_solve needs %zu bytes of dynamic LDS (+ ~10 KB static), the device grants %d per workgroup "
                                 "(%s): the solves will fail to launch — run with MLP_FACTOR=0\n", FAC_SOLVE_LDS, lds, hipGetErrorString(e1 != hipSuccess ? e1 : e2));
        }
        done = true;
    }
}
void launch_fac_solve(const DevView& dv, const Geom& g, int dir, int src, int dst, const double* src_ptr, int always, hipStream_t st, int fuse) {
    (void)g;
    fac_solve_lds_attr();
    hipLaunchKernelGGL(k_fac_solve, dim3(fac_grid_blocks()), dim3(BLK), FAC_SOLVE_LDS, st, dv, dir, src, dst, -1, -1, src_ptr, always, fuse);
}
void launch_fac_solve2(const DevView& dv, const Geom& g, int dir, int srcA, int dstA, int srcB, int dstB, hipStream_t st, int fuse) {
    (void)g;
    fac_solve_lds_attr();
    hipLaunchKernelGGL(k_fac_solve, dim3(fac_grid_blocks()), dim3(BLK), FAC_SOLVE_LDS, st, dv, dir, srcA, dstA, srcB, dstB, (const double*)nullptr, 0, fuse);
}

// The eta transformation of this pivot as a new rank-1 term (solver.rs:1274-1284): U = -(alpha_q - e_r) / alpha_q[r] by
// position, V = rho_r by row.  Runs before the update kernel (which zeroes alpha_q and rho behind itself).
__global__ void __launch_bounds__(BLK) k_fac_append(DevView v) {
    Ctl* c = v.ctl;
    if (c->halt || c->it.status != ITER_PIVOT) return;  // (a bound flip changes no basis)
    const int j = c->nlow, m = v.m, r = c->it.r;
    if (j >= v.fac_J) {  // the host failed to refactor in time
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            c->it.status = ITER_SINGULAR;
            c->halt = 1;
            push_rec(c, 0);
        }
        return;
    }
    // (U is kept UNSCALED with its factor beside it — readers form -(alpha_q - e_r) * inv, the same two roundings as before — so that the
    // FTRAN of a dual iteration can write the term in its own epilogue, before 1 / alpha_q[r] is known to every workgroup: fuse & 4)
    double* U = v.fac_U + (size_t)j * m;
    double* V = v.fac_V + (size_t)j * m;
    for (int p = blockIdx.x * BLK + threadIdx.x; p < m; p += gridDim.x * BLK) {
        U[p] = v.alpha_q[p] - (p == r ? 1.0 : 0.0);
        V[p] = v.rv[p].x;
    }
    if (!last_block_arrives(&v.fac_bar[2], gridDim.x)) return;
    if (threadIdx.x == 0) {
        v.fac_bar[2] = 0u;
        c->fac_inv[j] = c->it.inv_alpha;
        c->nlow = j + 1;
    }
}
void launch_fac_append(const DevView& dv, hipStream_t st) {
    hipLaunchKernelGGL(k_fac_append, dim3(grid_for(dv.m, 4, 256)), dim3(BLK), 0, st, dv);
}

// c_B by position into alpha_q (recalc_obj_coeffs, solver.rs:1199-1231)
__global__ void __launch_bounds__(BLK) k_fac_gather_cb(DevView v) {
    const int p = blockIdx.x * BLK + threadIdx.x;
    if (p < v.m) v.alpha_q[p] = v.obj_c[v.basic_vars[p]];
    if (p == 0) {
        v.ctl->it.status = ITER_PIVOT;
        v.ctl->halt = 0;
        v.ctl->up.kase = -1;
    }
}
void launch_fac_gather_cb(const DevView& dv, hipStream_t st) {
    hipLaunchKernelGGL(k_fac_gather_cb, dim3(blocks_for(dv.m)), dim3(BLK), 0, st, dv);
}

// ------------------------------------------------------------------ refactorisation: the peel, one level per pair of launches
__global__ void __launch_bounds__(BLK) k_fac_peel_init(DevView v, int* cnt, int* level, int* row_lev, int* claim, int* rcnt, int* claim_r) {
    const int t = blockIdx.x * BLK + threadIdx.x;
    const int N = v.m + v.n;
    if (t < v.m) {
        const int var = v.basic_vars[t];
        v.fac_var_of_pos[t] = var;
        cnt[t] = v.csc_ptr[var + 1] - v.csc_ptr[var];
        level[t] = 0;
        row_lev[t] = 0;
        claim[t] = INT_MAX;
        claim_r[t] = INT_MAX;
        int nbasic = 0;  // basic columns that meet row t (the row steps of the peel count them down)
        for (int e = v.csr_ptr[t]; e < v.csr_ptr[t + 1]; ++e) nbasic += v.var_loc[v.csr_col[e]] >= 0 ? 1 : 0;
        rcnt[t] = nbasic;
    }
    if (t < N) {
        const int loc = v.var_loc[t];
        v.fac_pos_of_var[t] = loc >= 0 ? loc : -1;
    }
}
// candidates of this level: unpeeled columns with exactly one unclaimed row bid for it (lowest position wins)
__global__ void __launch_bounds__(BLK) k_fac_peel_claim(DevView v, const int* cnt, const int* level, const int* row_lev, int* claim, int* cand_row,
                                                         int* counters) {
    const int p = blockIdx.x * BLK + threadIdx.x;
    if (p >= v.m) return;
    int cr = -1;
    if (level[p] == 0) {
        const int n1 = cnt[p];
        if (n1 == 1) {
            const int var = v.fac_var_of_pos[p];
            for (int e = v.csc_ptr[var]; e < v.csc_ptr[var + 1]; ++e) {
                const int row = v.csc_row[e];
                if (row_lev[row] == 0) {
                    cr = row;
                    v.fac_pval[p] = v.csc_val[e];
                    break;
                }
            }
            if (cr >= 0) atomicMin(&claim[cr], p);
        } else if (n1 <= 0) {
            counters[2] = 1;  // a basic column without an unclaimed row: the basis is singular
        }
    }
    cand_row[p] = cr;
}
__global__ void __launch_bounds__(BLK) k_fac_peel_commit(DevView v, int lev, int* cnt, int* level, int* row_lev, const int* claim, const int* cand_row,
                                                          int* counters) {
    const int p = blockIdx.x * BLK + threadIdx.x;
    if (p >= v.m) return;
    const int i = cand_row[p];
    if (i < 0 || level[p] != 0 || claim[i] != p) return;
    level[p] = lev;
    v.fac_prow[p] = i;
    row_lev[i] = lev;
    for (int e = v.csr_ptr[i]; e < v.csr_ptr[i + 1]; ++e) {  // row i leaves: the other basic columns it meets lose an unclaimed row
        const int p2 = v.fac_pos_of_var[v.csr_col[e]];
        if (p2 >= 0 && p2 != p) atomicSub(&cnt[p2], 1);
    }
    atomicAdd(&counters[0], 1);
}
// place of a peel step in the one list of levels: the column steps ascending, the bump (a level of its own, fac_meta[4], empty in
// fac_lptr: its positions are walked through the dense inverse), then the row steps descending (fac_meta[4] column steps, fac_meta[5]
// row steps); 1-based here (0 = bump), as the fill below counts
__device__ __forceinline__ int fac_unified_level(const DevView& v, int mark) {
    return mark > 0 ? mark : (mark < 0 ? v.fac_meta[4] + v.fac_meta[5] + mark + 2 : 0);
}
__global__ void __launch_bounds__(BLK) k_fac_peel_fill(DevView v, const int* level, int* cursor) {
    const int p = blockIdx.x * BLK + threadIdx.x;
    const int lev = p < v.m ? fac_unified_level(v, level[p]) : 0;
    // (the order inside a level does not matter: its positions are independent.)  Wave-aggregated: the lanes of a wave that share a
    // level take their places with ONE atomic — a level of 10^5 positions was 10^5 serialised atomics on one address, 2 ms per
    // refactorisation (rocprofv3, profiles/r04_factor_transport_kernel_stats.csv: the first cut spent 16 % of the solve here).
    unsigned long long todo = __ballot(lev > 0);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lv = __shfl(lev, leader, 64);
        const unsigned long long same = __ballot(lev == lv) & todo;
        int base = 0;
        if (lane == leader) base = atomicAdd(&cursor[lv - 1], __popcll(same));
        base = __shfl(base, leader, 64);
        if (lev == lv && ((same >> lane) & 1ull)) v.fac_items[v.fac_lptr[lv - 1] + base + __popcll(same & ((1ull << lane) - 1ull))] = p;
        todo &= ~same;
    }
}
// K = B0[bump rows, bump columns] as a dense b x b matrix (row = bump row slot, column = bump position slot), pitch FAC_BMAX
__global__ void __launch_bounds__(BLK) k_fac_bump_build(DevView v, double* Kd, int b) {
    const int s2 = blockIdx.x * BLK + threadIdx.x;
    if (s2 >= b) return;
    const int var = v.fac_var_of_pos[v.fac_bpos[s2]];
    for (int e = v.csc_ptr[var]; e < v.csc_ptr[var + 1]; ++e) {
        const int u = v.fac_bslot_of_row[v.csc_row[e]];
        if (u >= 0) Kd[(size_t)u * FAC_BMAX + s2] = v.csc_val[e];
    }
}
void launch_fac_bump_build(const DevView& dv, double* Kd, int b, hipStream_t st) {
    (void)hipMemsetAsync(Kd, 0, sizeof(double) * (size_t)b * FAC_BMAX, st);
    hipLaunchKernelGGL(k_fac_bump_build, dim3(blocks_for(b)), dim3(BLK), 0, st, dv, Kd, b);
}
// The whole peel in ONE launch (round 4, after the profile showed the host-paced form — two launches and one 4-byte read-back per
// level — at ~30 us per level, 10 % of a late pivot): the claim and commit phases of every level separated by grid barriers.
// Every value another workgroup wrote is read with an agent-scope load.
//
// Two kinds of step (the classical triangularisation with a bump): a COLUMN step removes the columns with a single entry on the
// rows still active (they claim that row), a ROW step removes the rows with a single entry on the columns still active (they claim
// that column).  Column steps run until they stall, then row steps until they stall, and so on until neither removes anything; what
// is left is the bump.  In the order [column steps ascending, bump, row steps DESCENDING] the basis is upper triangular around the
// bump: a column-step pivot row holds, besides its pivot, only columns removed later (or the bump); a row-step pivot row only
// columns removed by EARLIER row steps — so the two solves of k_fac_solve walk one list of levels with the bump in the middle.
// On the config-3 family at 60 000 rows the column peel alone leaves a bump of 3 004 at the end of the solve, both peels 306.
// level[p] / row_lev[i]: +s for column step s (1-based), -s for row step s, 0 = bump.  lsteps[0] = number of steps that removed
// something, lsteps[t] = +/- the running total after step t (sign = kind).
__global__ void __launch_bounds__(BLK) k_fac_peel_all(DevView v, int* cnt, int* level, int* row_lev, int* claim, int* cand_row, int* counters, int* lsteps,
                                                      int max_levels, int* rcnt, int* claim_r, int* cand_col) {
    const int tid = threadIdx.x, nb = (int)gridDim.x, m = v.m;
    unsigned* bar = v.fac_bar;
    unsigned target = 0;
    int prev = 0, nsteps = 0, nc = 0, nr = 0;
    bool ok = true;
    int kind = 0;       // 0: column steps, 1: row steps
    int stalled = 0;    // consecutive kinds that removed nothing
    while (nsteps < max_levels && stalled < 2) {
        if (kind == 0) {
            for (int p = (int)blockIdx.x * BLK + tid; p < m; p += nb * BLK) {  // claim: unpeeled columns with one active row bid for it
                int cr = -1;
                if (ld_agent(&level[p]) == 0) {
                    const int n1 = ld_agent(&cnt[p]);
                    if (n1 == 1) {
                        const int var = v.fac_var_of_pos[p];
                        for (int e = v.csc_ptr[var]; e < v.csc_ptr[var + 1]; ++e) {
                            const int row = v.csc_row[e];
                            if (ld_agent(&row_lev[row]) == 0) {
                                cr = row;
                                break;
                            }
                        }
                        if (cr >= 0) atomicMin(&claim[cr], p);
                    } else if (n1 <= 0) {
                        counters[2] = 1;  // a basic column without an active row: the basis is singular
                    }
                }
                cand_row[p] = cr;
            }
        } else {
            for (int i = (int)blockIdx.x * BLK + tid; i < m; i += nb * BLK) {  // claim: active rows with one active column bid for it
                int cp = -1;
                if (ld_agent(&row_lev[i]) == 0) {
                    const int n1 = ld_agent(&rcnt[i]);
                    if (n1 == 1) {
                        for (int e = v.csr_ptr[i]; e < v.csr_ptr[i + 1]; ++e) {
                            const int p2 = v.fac_pos_of_var[v.csr_col[e]];
                            if (p2 >= 0 && ld_agent(&level[p2]) == 0) {
                                cp = p2;
                                break;
                            }
                        }
                        if (cp >= 0) atomicMin(&claim_r[cp], i);
                    } else if (n1 <= 0) {
                        counters[2] = 1;  // an active row without an active column: singular
                    }
                }
                cand_col[i] = cp;
            }
        }
        target += (unsigned)nb;
        ok = fac_grid_barrier(v.ctl, bar, target) && ok;
        const int mark = kind == 0 ? nc + 1 : -(nr + 1);
        for (int t = (int)blockIdx.x * BLK + tid; t < m; t += nb * BLK) {  // commit: the lowest bidder takes the pivot
            int p, i;
            if (kind == 0) {
                p = t;
                i = cand_row[p];
                if (i < 0 || ld_agent(&level[p]) != 0 || ld_agent(&claim[i]) != p) continue;
            } else {
                i = t;
                p = cand_col[i];
                if (p < 0 || ld_agent(&row_lev[i]) != 0 || ld_agent(&claim_r[p]) != i) continue;
            }
            st_agent(&level[p], mark);
            v.fac_prow[p] = i;
            st_agent(&row_lev[i], mark);
            const int var = v.fac_var_of_pos[p];
            for (int e = v.csr_ptr[i]; e < v.csr_ptr[i + 1]; ++e) {  // row i leaves: the other basic columns it meets lose an active row
                const int col = v.csr_col[e];
                if (col == var) v.fac_pval[p] = v.csr_val[e];
                const int p2 = v.fac_pos_of_var[col];
                if (p2 >= 0 && p2 != p) atomicSub(&cnt[p2], 1);
            }
            for (int e = v.csc_ptr[var]; e < v.csc_ptr[var + 1]; ++e) {  // column p leaves: the other rows it meets lose an active column
                const int i2 = v.csc_row[e];
                if (i2 != i) atomicSub(&rcnt[i2], 1);
            }
            atomicAdd(&counters[0], 1);
        }
        target += (unsigned)nb;
        ok = fac_grid_barrier(v.ctl, bar, target) && ok;
        const int total = ld_agent(&counters[0]);  // (every workgroup reads the same value: they take the same branch)
        if (total == prev) {
            stalled += 1;
            kind ^= 1;
            continue;
        }
        stalled = 0;
        nsteps += 1;
        if (kind == 0) nc += 1;
        else nr += 1;
        if (blockIdx.x == 0 && tid == 0) lsteps[nsteps] = kind == 0 ? total : -total;
        prev = total;
        if (total == m) break;
    }
    if (!last_block_arrives(&v.fac_bar[1], (unsigned)nb)) return;
    if (tid == 0) {
        lsteps[0] = nsteps;
        counters[1] = ok ? 0 : 1;  // a barrier gave up (grid not co-resident): the host falls back to the paced form
        fac_bar_reset(v.fac_bar);
    }
}
void launch_fac_peel_all(const DevView& dv, int* cnt, int* level, int* row_lev, int* claim, int* cand_row, int* counters, int* lsteps, int max_levels,
                         int* rcnt, int* claim_r, int* cand_col, hipStream_t st) {
    hipLaunchKernelGGL(k_fac_peel_all, dim3(fac_grid_blocks()), dim3(BLK), 0, st, dv, cnt, level, row_lev, claim, cand_row, counters, lsteps, max_levels,
                       rcnt, claim_r, cand_col);
}
void launch_fac_peel_init(const DevView& dv, int* cnt, int* level, int* row_lev, int* claim, int* rcnt, int* claim_r, hipStream_t st) {
    hipLaunchKernelGGL(k_fac_peel_init, dim3(blocks_for((long)dv.m + dv.n)), dim3(BLK), 0, st, dv, cnt, level, row_lev, claim, rcnt, claim_r);
}
void launch_fac_peel_level(const DevView& dv, int lev, int* cnt, int* level, int* row_lev, int* claim, int* cand_row, int* counters, hipStream_t st) {
    hipLaunchKernelGGL(k_fac_peel_claim, dim3(blocks_for(dv.m)), dim3(BLK), 0, st, dv, cnt, level, row_lev, claim, cand_row, counters);
    hipLaunchKernelGGL(k_fac_peel_commit, dim3(blocks_for(dv.m)), dim3(BLK), 0, st, dv, lev, cnt, level, row_lev, claim, cand_row, counters);
}
void launch_fac_peel_fill(const DevView& dv, const int* level, int* cursor, hipStream_t st) {
    hipLaunchKernelGGL(k_fac_peel_fill, dim3(blocks_for(dv.m)), dim3(BLK), 0, st, dv, level, cursor);
}
// Resolved edge lists of the solves, in level order (index = place in fac_items): for the FTRAN the other basic columns of the
// pivot row as (position, value) pairs, for the BTRAN the other rows of the column as (row, value) pairs — a solve then walks
// item -> edges -> vector (three dependent loads) instead of item -> row -> CSR -> variable -> position -> vector.
// pass 0: counts (then an exclusive scan), pass 1: fill.
__global__ void __launch_bounds__(BLK) k_fac_edges(DevView v, int pass, int* fcnt, int* bcnt, const int* level) {
    const int idx = blockIdx.x * BLK + threadIdx.x;
    const int npeeled = v.fac_meta[1];
    if (idx >= npeeled) {
        if (pass == 0 && idx == npeeled) {
            fcnt[idx] = 0;
            bcnt[idx] = 0;
        }
        return;
    }
    const int p = v.fac_items[idx];
    const int i = v.fac_prow[p];
    const int var = v.fac_var_of_pos[p];
    if (pass == 1) {
        v.fac_irow[idx] = i;
        v.fac_ipiv[idx] = v.fac_pval[p];
        v.fac_idx_of_pos[p] = idx;
        v.fac_idx_of_row[i] = idx;
        v.fac_lev_of_pos[p] = fac_unified_level(v, level[p]) - 1;  // (level indices from zero, as in fac_lptr)
        v.fac_lev_of_row[i] = fac_unified_level(v, level[p]) - 1;
    }
    int nf = 0, nbk = 0;
    int fo = pass ? v.fac_fptr[idx] : 0, bo = pass ? v.fac_bptr[idx] : 0;
    for (int e = v.csr_ptr[i]; e < v.csr_ptr[i + 1]; ++e) {
        const int p2 = v.fac_pos_of_var[v.csr_col[e]];
        if (p2 >= 0 && p2 != p) {
            if (pass) {
                v.fac_fidx[fo + nf] = p2;
                v.fac_fval[fo + nf] = v.csr_val[e];
            }
            nf += 1;
        }
    }
    for (int e = v.csc_ptr[var]; e < v.csc_ptr[var + 1]; ++e) {
        const int row = v.csc_row[e];
        if (row != i) {
            if (pass) {
                v.fac_bidx[bo + nbk] = row;
                v.fac_bval[bo + nbk] = v.csc_val[e];
            }
            nbk += 1;
        }
    }
    if (pass == 0) {
        fcnt[idx] = nf;
        bcnt[idx] = nbk;
    }
}
void launch_fac_edges(const DevView& dv, int pass, int* fcnt, int* bcnt, const int* level, hipStream_t st) {
    hipLaunchKernelGGL(k_fac_edges, dim3(blocks_for((long)dv.m + 1)), dim3(BLK), 0, st, dv, pass, fcnt, bcnt, level);
}
// Highest level any BTRAN dependent of a position reaches: y[row of p2] depends on y[row of p] when column p2 has an entry on the
// pivot row of p — the FTRAN edge list of p — so reach(p) = max(level(p), reach of its FTRAN edges), one level at a time, descending.
// The bump is one level (the dense inverse couples its positions): they share reach = max(bump level, reach of the row-step columns
// on the bump rows).  One launch, one workgroup (round 4: one launch per level was ~5 us x 100 levels per refactorisation on the
// config-3 family): the levels are small except the first few, and a level costs its edges / 1024.
__global__ void __launch_bounds__(1024) k_fac_reach_all(DevView v, int lev_hi, int lev_lo) {
    const int nbump = v.fac_meta[2], nsplit = v.fac_meta[4];
    const int tid = threadIdx.x;
    __shared__ int s_red[16];
    for (int lev = lev_hi; lev >= lev_lo; --lev) {
        if (lev == nsplit) {
            int rch = nsplit;
            for (int t = tid; t < nbump; t += 1024) {
                const int i = v.fac_brow[t];
                for (int e = v.csr_ptr[i]; e < v.csr_ptr[i + 1]; ++e) {
                    const int p2 = v.fac_pos_of_var[v.csr_col[e]];
                    if (p2 >= 0 && v.fac_lev_of_pos[p2] > nsplit) rch = max(rch, v.fac_reach_of_pos[p2]);
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) rch = max(rch, __shfl_down(rch, o, 64));
            if ((tid & 63) == 0) s_red[tid >> 6] = rch;
            __syncthreads();
            rch = s_red[0];
            for (int w = 1; w < 16; ++w) rch = max(rch, s_red[w]);
            for (int t = tid; t < nbump; t += 1024) {
                v.fac_reach_of_pos[v.fac_bpos[t]] = rch;
                v.fac_lev_of_pos[v.fac_bpos[t]] = nsplit;
                v.fac_lev_of_row[v.fac_brow[t]] = nsplit;
            }
        } else {
            const int lo = v.fac_lptr[lev], hi = v.fac_lptr[lev + 1];
            for (int idx = lo + tid; idx < hi; idx += 1024) {
                int rch = lev;
                for (int e = v.fac_fptr[idx]; e < v.fac_fptr[idx + 1]; ++e) rch = max(rch, v.fac_reach_of_pos[v.fac_fidx[e]]);
                v.fac_reach_of_pos[v.fac_items[idx]] = rch;
            }
        }
        __syncthreads();  // (one workgroup: its own earlier stores are visible after the barrier)
    }
}
// one LARGE level by the whole grid (the first column steps of a big model hold 10^4-10^5 positions each: 66 trips of a dependent chain
// for the one workgroup above — 238 us per refactorisation at 200 000 rows, most of it in three levels)
__global__ void __launch_bounds__(BLK) k_fac_reach_level(DevView v, int lev) {
    const int lo = v.fac_lptr[lev], hi = v.fac_lptr[lev + 1];
    for (int idx = lo + (int)blockIdx.x * BLK + (int)threadIdx.x; idx < hi; idx += (int)gridDim.x * BLK) {
        int rch = lev;
        for (int e = v.fac_fptr[idx]; e < v.fac_fptr[idx + 1]; ++e) rch = max(rch, v.fac_reach_of_pos[v.fac_fidx[e]]);
        v.fac_reach_of_pos[v.fac_items[idx]] = rch;
    }
}
// levels [lev_lo, lev_hi] descending by one workgroup / one level of `size` positions by the grid
void launch_fac_reach_all(const DevView& dv, int lev_hi, int lev_lo, hipStream_t st) {
    if (lev_hi >= lev_lo) hipLaunchKernelGGL(k_fac_reach_all, dim3(1), dim3(1024), 0, st, dv, lev_hi, lev_lo);
}
void launch_fac_reach_level(const DevView& dv, int lev, int size, hipStream_t st) {
    hipLaunchKernelGGL(k_fac_reach_level, dim3(std::max(1, std::min(1024, (size + BLK - 1) / BLK))), dim3(BLK), 0, st, dv, lev);
}

// Explicit inverse of the bump (K = B0[bump rows, bump columns], b <= FAC_BMAX) in ONE launch: Gauss-Jordan on [K | I] with partial
// pivoting by row choice (no physical swaps: row piv_j serves column j, the result is gathered at the end), the rows dealt out to
// the workgroups, ONE grid barrier per column — the search for the next pivot rides in the elimination (the lane that owns column
// j + 1 sees every updated entry of it).  Round 4: the per-column launches of launch_gauss_jordan (four per column) cost 1.5 ms per
// refactorisation at b = 76 on the config-3 family, 50 us per pivot.  Fixed order everywhere: bit-reproducible.
//   K, W: b x FAC_BMAX work arrays (W starts as I), out: fac_Wb (out[j][c] = (K^-1)[j][c]);  part_*: 2 x gridDim.x partial maxima.
constexpr int FAC_GJ_BLOCKS = 64;
__global__ void __launch_bounds__(BLK) k_fac_bump_invert(DevView v, double* K, double* W, double* out, double* outT, int b, int* flag, double* part_val, int* part_row) {
    const int tid = threadIdx.x, nb = (int)gridDim.x, wg = (int)blockIdx.x;
    constexpr int P = FAC_BMAX;
    unsigned* bar = v.fac_bar;
    unsigned target = 0;
    bool ok = true;
    __shared__ int s_piv[FAC_BMAX];
    __shared__ double s_pv[FAC_BMAX];
    __shared__ double s_rv[BLK];
    __shared__ int s_rr[BLK];
    for (int i = wg; i < b; i += nb)
        for (int c = tid; c < b; c += BLK) st_agent(&W[(size_t)i * P + c], c == i ? 1.0 : 0.0);
    unsigned used = 0u;  // bit t: own row wg + t * nb has served as a pivot row (b <= 1024, nb = 64: at most 16 own rows)
    if (tid == 0) {      // candidates for column 0
        double bv = -1.0;
        int br = -1;
        for (int i = wg; i < b; i += nb) {
            const double a = fabs(K[(size_t)i * P]);
            if (a > bv) { bv = a; br = i; }
        }
        st_agent(&part_val[wg], bv);
        st_agent(&part_row[wg], br);
    }
    bool singular = false;
    for (int j = 0; j < b; ++j) {
        target += (unsigned)nb;
        ok = fac_grid_barrier(v.ctl, bar, target) && ok;
        // every workgroup reduces the partial maxima itself (ties: the lowest row)
        double bv = -1.0;
        int br = INT_MAX;
        if (tid < nb) {
            bv = ld_agent(&part_val[(j & 1) * nb + tid]);
            br = ld_agent(&part_row[(j & 1) * nb + tid]);
            if (br < 0) { bv = -1.0; br = INT_MAX; }
        }
        s_rv[tid] = bv;
        s_rr[tid] = br;
        __syncthreads();
        for (int o = BLK / 2; o > 0; o >>= 1) {
            if (tid < o) {
                const double v2 = s_rv[tid + o];
                const int r2 = s_rr[tid + o];
                if (v2 > s_rv[tid] || (v2 == s_rv[tid] && r2 < s_rr[tid])) { s_rv[tid] = v2; s_rr[tid] = r2; }
            }
            __syncthreads();
        }
        const int piv = s_rr[0];
        const double pmax = s_rv[0];
        __syncthreads();
        if (!(pmax > 0.0) || piv == INT_MAX) {  // (every workgroup takes the same branch)
            singular = true;
            break;
        }
        const double pv = ld_agent(&K[(size_t)piv * P + j]);
        if (tid == 0) {
            s_piv[j] = piv;
            s_pv[j] = pv;
        }
        if (piv % nb == wg) used |= 1u << (piv / nb);
        const double inv = 1.0 / pv;
        double cv = -1.0;  // the lane that owns column j + 1: best unused own row for the next column
        int cr = -1;
        // the multipliers of the own rows, all read before any lane stores (the lane of column j zeroes K[i][j] below)
        double fr[FAC_BMAX / FAC_GJ_BLOCKS];
#pragma unroll
        for (int t = 0; t < FAC_BMAX / FAC_GJ_BLOCKS; ++t) {
            const int i = wg + t * nb;
            fr[t] = i < b ? ld_agent(&K[(size_t)i * P + j]) * inv : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < FAC_BMAX / FAC_GJ_BLOCKS; ++t) {
            const int i = wg + t * nb;
            if (i >= b || i == piv) continue;
            const double f = fr[t];
            const bool free_row = !((used >> t) & 1u);
            if (f != 0.0) {
                for (int c = tid; c < b; c += BLK) {
                    const double kn = ld_agent(&K[(size_t)i * P + c]) - f * ld_agent(&K[(size_t)piv * P + c]);
                    st_agent(&K[(size_t)i * P + c], c == j ? 0.0 : kn);
                    st_agent(&W[(size_t)i * P + c], ld_agent(&W[(size_t)i * P + c]) - f * ld_agent(&W[(size_t)piv * P + c]));
                    if (c == j + 1 && free_row && fabs(kn) > cv) { cv = fabs(kn); cr = i; }
                }
            } else if (free_row && j + 1 < b && tid == (j + 1) % BLK) {
                const double a = fabs(ld_agent(&K[(size_t)i * P + j + 1]));
                if (a > cv) { cv = a; cr = i; }
            }
        }
        if (j + 1 < b && tid == (j + 1) % BLK) {
            st_agent(&part_val[((j + 1) & 1) * nb + wg], cv);
            st_agent(&part_row[((j + 1) & 1) * nb + wg], cr);
        }
    }
    target += (unsigned)nb;
    ok = fac_grid_barrier(v.ctl, bar, target) && ok;
    if (!singular)
        for (int j = wg; j < b; j += nb) {
            const int piv = s_piv[j];
            const double inv = 1.0 / s_pv[j];
            for (int c = tid; c < b; c += BLK) {
                const double x = ld_agent(&W[(size_t)piv * P + c]) * inv;
                out[(size_t)j * P + c] = x;
                outT[(size_t)c * P + j] = x;
            }
        }
    if (!last_block_arrives(&v.fac_bar[1], (unsigned)nb)) return;
    if (tid == 0) {
        if (singular) flag[0] = 1;
        if (!ok) flag[1] = 1;  // a barrier gave up: the caller falls back to the launch-per-column form
        fac_bar_reset(v.fac_bar);
    }
}
void launch_fac_bump_invert(const DevView& dv, double* K, double* W, double* out, double* outT, int b, int* flag, double* part_val, int* part_row, hipStream_t st) {
    hipLaunchKernelGGL(k_fac_bump_invert, dim3(FAC_GJ_BLOCKS), dim3(BLK), 0, st, dv, K, W, out, outT, b, flag, part_val, part_row);
}

// Plan of the solves' walk, on the device (no read-back): which levels workgroup 0 walks alone — at most FAC_TAIL positions: the
// upper column steps and most row steps of the peel — their
// slots (places of their items among all such items, ascending with the level), and the segments: runs of such levels (kind 1),
// runs of the others (0, walked by the grid), the bump (2).
constexpr int FAC_PLAN_LEVELS = 4096 + 2;  // (FAC_MAX_LEVELS + 2 of engine.hip)
__global__ void __launch_bounds__(BLK) k_fac_plan(DevView v, int* ltslot, int* segs) {
    const int nlev = min(v.fac_meta[0], FAC_PLAN_LEVELS), nsplit = v.fac_meta[4];
    __shared__ int s_sz[FAC_PLAN_LEVELS];
    __shared__ short s_ok[FAC_PLAN_LEVELS];
    __shared__ int s_sl[FAC_PLAN_LEVELS];
    for (int lev = threadIdx.x; lev < nlev; lev += BLK) {  // (the level table into LDS in parallel: the plan itself is one lane's sequential walk)
        const int sz = v.fac_lptr[lev + 1] - v.fac_lptr[lev];
        s_sz[lev] = sz;
        s_ok[lev] = (sz > 0 && sz <= FAC_TAIL && lev != nsplit) ? 1 : 0;
        s_sl[lev] = -1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int used = 0;
        for (int lev = 0; lev < nlev; ++lev)
            if (s_ok[lev]) {
                s_sl[lev] = 0;  // chosen
                used += s_sz[lev];
            }
        int slot = 0, nseg = 0, first_small = nlev;
        for (int lev = 0; lev < nlev; ++lev)
            if (s_sl[lev] >= 0) {
                s_sl[lev] = slot;
                slot += s_sz[lev];
            }
        for (int lev = 0; lev < nlev;) {
            if (lev == nsplit) {
                segs[3 * nseg] = 2; segs[3 * nseg + 1] = lev; segs[3 * nseg + 2] = lev;
                nseg += 1;
                lev += 1;
                continue;
            }
            const int kind = s_sl[lev] >= 0 ? 1 : 0;
            int e = lev;
            while (e + 1 < nlev && e + 1 != nsplit && (s_sl[e + 1] >= 0 ? 1 : 0) == kind) e += 1;
            segs[3 * nseg] = kind; segs[3 * nseg + 1] = lev; segs[3 * nseg + 2] = e;
            nseg += 1;
            if (kind == 1 && first_small == nlev) first_small = lev;
            lev = e + 1;
        }
        v.fac_meta[7] = nseg;
        v.fac_meta[3] = first_small;
        v.fac_meta[6] = used;
    }
    __syncthreads();
    for (int lev = threadIdx.x; lev < nlev; lev += BLK) ltslot[lev] = s_sl[lev];
}
void launch_fac_plan(const DevView& dv, int* ltslot, int* segs, hipStream_t st) {
    hipLaunchKernelGGL(k_fac_plan, dim3(1), dim3(BLK), 0, st, dv, ltslot, segs);
}
// The items of the small levels as records (FacTailRec), by LDS slot: a target that is itself such an item becomes its slot.
__global__ void __launch_bounds__(BLK) k_fac_tail_prog(DevView v, FacTailRec* pf, FacTailRec* pb, int nlev) {
    const int lev = blockIdx.x;
    const int slot0 = v.fac_ltslot[lev];
    if (lev >= nlev || slot0 < 0) return;
    const int idx = v.fac_lptr[lev] + (int)threadIdx.x;
    if (idx >= v.fac_lptr[lev + 1]) return;
    const int k = slot0 + (int)threadIdx.x;
    const int p = v.fac_items[idx], i = v.fac_irow[idx];
    const double piv = v.fac_ipiv[idx];
    for (int dir = 0; dir < 2; ++dir) {
        const int* eidx = dir == 0 ? v.fac_fidx : v.fac_bidx;
        const double* eval = dir == 0 ? v.fac_fval : v.fac_bval;
        const int beg = dir == 0 ? v.fac_fptr[idx] : v.fac_bptr[idx], end = dir == 0 ? v.fac_fptr[idx + 1] : v.fac_bptr[idx + 1];
        const int n = min(end - beg, 255);  // (a longer list cannot be a record: FAC_TAIL_MAXEDGES in the plan... the host keeps such levels with the grid)
        FacTailRec r;
        r.out_n = (n << 24) | (dir == 0 ? p : i);
        r.rhs = dir == 0 ? i : p;
        r.piv = piv;
        r.ovf = n > FAC_TAIL_INLINE ? beg + FAC_TAIL_INLINE : -1;
        r.pad[0] = r.pad[1] = r.pad[2] = 0;
        int* eslot = dir == 0 ? v.fac_fslot : v.fac_bslot;
        for (int e = beg + FAC_TAIL_INLINE; e < beg + n; ++e) {  // slots of the edges beyond the inline ones
            const int t = eidx[e];
            int sl = -1;
            const int j = dir == 0 ? v.fac_idx_of_pos[t] : v.fac_idx_of_row[t];
            if (j >= 0) {
                const int lj = dir == 0 ? v.fac_lev_of_pos[t] : v.fac_lev_of_row[t];
                const int sj = v.fac_ltslot[lj];
                if (sj >= 0) sl = sj + j - v.fac_lptr[lj];
            }
            eslot[e] = sl;
        }
        for (int e = 0; e < FAC_TAIL_INLINE; ++e) {
            int t = 0, sl = -1;
            double a = 0.0;
            if (e < end - beg) {
                t = eidx[beg + e];
                a = eval[beg + e];
                const int j = dir == 0 ? v.fac_idx_of_pos[t] : v.fac_idx_of_row[t];
                if (j >= 0) {  // (a peeled position: is its level one of the small ones?)
                    const int lj = dir == 0 ? v.fac_lev_of_pos[t] : v.fac_lev_of_row[t];
                    const int sj = v.fac_ltslot[lj];
                    if (sj >= 0) sl = sj + j - v.fac_lptr[lj];
                }
            }
            r.tgt[e] = t;
            r.slot[e] = sl;
            r.val[e] = a;
        }
        (dir == 0 ? pf : pb)[k] = r;
    }
}
void launch_fac_tail_prog(const DevView& dv, FacTailRec* pf, FacTailRec* pb, int nlev, hipStream_t st) {
    if (nlev > 0) hipLaunchKernelGGL(k_fac_tail_prog, dim3(nlev), dim3(BLK), 0, st, dv, pf, pb, nlev);
}

__global__ void __launch_bounds__(BLK) k_fac_bump_transpose(const double* in, double* outT, int b) {
    const int j = blockIdx.x;
    for (int c = threadIdx.x; c < b; c += BLK) outT[(size_t)c * FAC_BMAX + j] = in[(size_t)j * FAC_BMAX + c];
}
void launch_fac_bump_transpose(const double* in, double* outT, int b, hipStream_t st) {
    if (b > 0) hipLaunchKernelGGL(k_fac_bump_transpose, dim3(b), dim3(BLK), 0, st, in, outT, b);
}
