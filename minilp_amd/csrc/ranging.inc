// ranging.inc — cost and rhs ranging of the current basis (include/minilp_hip.h: mlp_solution_cost_ranging, mlp_solution_rhs_ranging;
// DESIGN.md "Ranging").  How far may a cost coefficient / a right-hand side move before the basis stops being optimal / feasible?
//
// Requests are served in batches of R = RG_BATCH:
//   cost ranging of R basic positions:  the R rows of B^-1 as ONE block rho[m][R] (interleaved by row: a gather of row i returns R
//       contiguous doubles), then ONE pass over A's CSC for the whole batch that forms alpha_i = rho . a_i for every non-basic column
//       and runs the two ratio tests of every request on (r_i, status_i, alpha_i);
//   rhs ranging of R rows whose slack is non-basic:  the R columns of B^-1 restricted to the nucleus as H[k][R], then ONE pass by
//       position that pulls the singleton part h_p = (e - F h_K)_p / D_p per CSR row and runs the ratio tests on (xB, loB, hiB).
// Side-effect free in the sense of duals.inc: only the private buffers of RangingBufs are written; the pending rank-1 terms of the
// delayed-update mode are applied, not folded; the compact factor is not re-peeled (launch_fac_block: one level-scheduled solve per
// request on a copy of the view with private result vectors, scattered into the same block); Ctl, d, rv and the work vectors are
// untouched.  The two accumulators of the sweeps — csc_block_dot over a column of A, csr_nucleus_pull over a singleton row — and
// launch_fac_block are shared with cuts.inc, gmi.inc and tableau.inc.  No float atomics; every sum has a fixed order that depends on
// the request alone (never on what else is in the batch, or where), and the reductions across columns / positions are exact minima
// and maxima: the two numbers of a request are bit-identical whatever the call.

constexpr double RG_INF = __builtin_huge_val();

// ---- the accumulators every batched pass shares (ranging.inc, cuts.inc, gmi.inc, tableau.inc).  Both leave in acc[r], on every lane of
// the group, a sum whose order depends on the column / row and on G alone: lane gl takes the entries gl, gl + G, ... in storage order
// into R accumulators (the [..][R] block is read as double2), then the xor tree of the lane group.  They shuffle: every thread of the
// workgroup calls them, a thread without work with live = false / sg < 0.  Their callers form the thread's column / position in long
// (the grid may hold more than 2^31 threads) and narrow the quotient, which never passes N, m or k by more than a workgroup: a 64-bit
// index kept live through the entry loop costs two VGPRs, and k_gmi_sweep / k_tab_b_rhs sit at the 80-register step of the occupancy.
// the CSC block dot: acc[r] = sum over the entries e of column var of A of a_e * blk[row_e][r]
template <int R, int G>
__device__ __forceinline__ void csc_block_dot(const DevView& v, const double* blk, bool live, int var, int gl, double (&acc)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
    if (live) {
        const int end = v.csc_ptr[var + 1];
        for (int e = v.csc_ptr[var] + gl; e < end; e += G) {
            const double a = v.csc_val[e];
            const double2* rr = reinterpret_cast<const double2*>(blk + (size_t)v.csc_row[e] * R);
#pragma unroll
            for (int r = 0; r < R; r += 2) {
                const double2 t = rr[r >> 1];
                acc[r] += a * t.x;
                acc[r + 1] += a * t.y;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = group_sum<G>(acc[r]);
}
// the CSR nucleus pull of singleton row sg: acc[r] = sum over the entries e of CSR row sg whose column is a nucleus basic of
// a_e * blk[slot_e][r] (blk by nucleus slot)
template <int R, int G>
__device__ __forceinline__ void csr_nucleus_pull(const DevView& v, const double* blk, int sg, int gl, double (&acc)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
    if (sg >= 0) {
        const int end = v.csr_ptr[sg + 1];
        for (int e = v.csr_ptr[sg] + gl; e < end; e += G) {
            const int l2 = v.var_loc[v.csr_col[e]];
            if (l2 < 0) continue;
            const int s = v.kslot_of_pos[l2];
            if (s < 0) continue;
            const double a = v.csr_val[e];
            const double2* hh = reinterpret_cast<const double2*>(blk + (size_t)s * R);
#pragma unroll
            for (int r = 0; r < R; r += 2) {
                const double2 t = hh[r >> 1];
                acc[r] += a * t.x;
                acc[r + 1] += a * t.y;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = group_sum<G>(acc[r]);
}
// R values as one row of a [..][R] block (double2 stores: one 128-byte line at R = 16)
template <int R>
__device__ __forceinline__ void store_block_row(double* row, const double (&x)[R]) {
    double2* out = reinterpret_cast<double2*>(row);
#pragma unroll
    for (int r = 0; r < R; r += 2) {
        double2 t;
        t.x = x[r];
        t.y = x[r + 1];
        out[r >> 1] = t;
    }
}
// entry (s, c) of the nucleus inverse with the pending terms applied (term order)
__device__ __forceinline__ double rg_w(const DevView& v, int nlow, int s, int c) {
    double w = v.W[(size_t)s * v.ld + c];
    double l = 0.0;
    for (int j = 0; j < nlow; ++j) l += v.U[(size_t)j * v.ld + s] * v.V[(size_t)j * v.ld + c];
    return nlow ? w + l : w;
}

// Rows of B^-1: workgroup (x, r) fills columns [x * BLK, +BLK) of the nucleus part of request r's row.
//   nucleus position (slot s):            W[s, :] on the nucleus rows, zero on singleton rows
//   singleton position (row sg, diag D):  1 / D on sg and -(1 / D) sum_e A[sg, e] W[slot(e), :] over the nucleus columns of CSR row sg
//                                         (CSR order) — a sparse combination of stored rows, no pass over W
template <int R>
__global__ void __launch_bounds__(BLK) k_rg_rows(DevView v, RangingBufs b) {
    const int r = blockIdx.y;
    const int p = b.req[r];
    if (p < 0) return;
    const int k = v.ctl->k, nlow = v.lrJ ? v.ctl->nlow : 0;
    const int c = blockIdx.x * BLK + threadIdx.x;
    const int ks = v.kslot_of_pos[p];
    if (ks >= 0) {
        if (c < k) b.blk[(size_t)v.row_of_kslot[c] * R + r] = rg_w(v, nlow, ks, c);
        return;
    }
    const int sg = v.srow_of_pos[p];
    const double inv = 1.0 / v.sdiag_of_pos[p];
    if (c == 0) b.blk[(size_t)sg * R + r] = inv;
    if (c >= k) return;
    double acc = 0.0;
    const int end = v.csr_ptr[sg + 1];
    for (int e = v.csr_ptr[sg]; e < end; ++e) {
        const int loc = v.var_loc[v.csr_col[e]];
        if (loc < 0) continue;
        const int s = v.kslot_of_pos[loc];
        if (s >= 0) acc += v.csr_val[e] * rg_w(v, nlow, s, c);
    }
    b.blk[(size_t)v.row_of_kslot[c] * R + r] = -(inv * acc);
}
// Columns of B^-1 restricted to the nucleus: H[s][r] = W[s, slot(row_r)]; a request whose row a singleton covers has h_K = 0 (its only
// entry, 1 / D at the covering position, is formed by the pull).  One thread per row slot serves the whole batch: the host sorts a
// call's requests by column slot, so neighbouring requests share the 64-byte sectors of the row-major W.
template <int R>
__global__ void __launch_bounds__(BLK) k_rg_cols(DevView v, RangingBufs b) {
    const int s = blockIdx.x * BLK + threadIdx.x;
    if (s >= v.ctl->k) return;
    const int nlow = v.lrJ ? v.ctl->nlow : 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = b.req[r];
        const int c = row >= 0 ? v.kslot_of_row[row] : -1;
        if (c >= 0) b.blk[(size_t)s * R + r] = rg_w(v, nlow, s, c);
    }
}
// compact factor: right-hand side of one solve (the unit vector of idx, or column r of a block X[m][R]), and its result (dir 0: the
// FTRAN's tau, 1: the BTRAN's v) into column r of the block
__global__ void __launch_bounds__(BLK) k_rg_unit(double* u, int m, int idx) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i < m) u[i] = i == idx ? 1.0 : 0.0;
}
template <int R>
__global__ void __launch_bounds__(BLK) k_rg_col(const double* __restrict__ X, double* __restrict__ u, int m, int r) {
    const long step = (long)gridDim.x * BLK;
    for (long i = (long)blockIdx.x * BLK + threadIdx.x; i < m; i += step) u[i] = X[(size_t)i * R + r];
}
template <int R>
__global__ void __launch_bounds__(BLK) k_rg_take(SolveBufs s, double* __restrict__ blk, int m, int r, int dir) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i < m) blk[(size_t)i * R + r] = dir ? s.rv[i].y : s.tau[i];
}

__device__ __forceinline__ double rg_wave_min(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmin(x, __shfl_down(x, o, 64));
    return x;
}
__device__ __forceinline__ double rg_wave_max(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_down(x, o, 64));
    return x;
}
// (max of lo[r], min of hi[r]) over the workgroup -> out[2 r], out[2 r + 1]; exact, so the order does not matter
template <int R>
__device__ void rg_block_write(const double (&lo)[R], const double (&hi)[R], double* out) {
    __shared__ double s[BLK / 64][2 * R];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double a = rg_wave_max(lo[r]), c = rg_wave_min(hi[r]);
        if (l == 0) {
            s[w][2 * r] = a;
            s[w][2 * r + 1] = c;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * R) {
        double a = s[0][threadIdx.x];
        for (int q = 1; q < BLK / 64; ++q) a = (threadIdx.x & 1) ? fmin(a, s[q][threadIdx.x]) : fmax(a, s[q][threadIdx.x]);
        out[threadIdx.x] = a;
    }
}

// Cost ranging: one pass over A's CSC for the whole batch (G lanes per column as k_du_reduced).  Basic columns are skipped; for a
// non-basic column i, alpha_i[r] = rho_r . a_i (csc_block_dot) and
//   at lower: alpha > 0 bounds delta+ by r_i / alpha, alpha < 0 bounds delta- ;   at upper: the mirror image;
//   non-basic at neither bound: alpha != 0 pins both at 0;   fixed: imposes nothing.
// |alpha| <= EPS counts as zero; a reduced cost of the wrong sign is clamped to 0.
template <int R, int G>
__global__ void __launch_bounds__(BLK) k_rg_cost_sweep(DevView v, RangingBufs b) {
    const int var = (int)(((long)blockIdx.x * BLK + threadIdx.x) / G);
    const int gl = threadIdx.x & (G - 1);
    double acc[R], lo[R], hi[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { lo[r] = -RG_INF; hi[r] = RG_INF; }
    int loc = 0;
    if (var < b.N) loc = v.var_loc[var];
    const bool live = var < b.N && loc < 0;
    csc_block_dot<R, G>(v, b.blk, live, var, gl, acc);
    if (live && gl == 0) {
        const int stt = nb_status_of(v.nbflags[-1 - loc]);
        if (stt != 4) {
            const double ri = b.r[var];
            const double num = stt == 1 ? fmax(ri, 0.0) : fmin(ri, 0.0);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double a = acc[r];
                if (!(fabs(a) > EPS)) continue;
                if (stt == 3) {
                    lo[r] = 0.0;
                    hi[r] = 0.0;
                } else {
                    const double q = num / a;
                    if ((stt == 1) == (a > 0.0)) hi[r] = q;
                    else lo[r] = q;
                }
            }
        }
    }
    rg_block_write<R>(lo, hi, b.part + (size_t)blockIdx.x * 2 * R);
}
// Rhs ranging: one pass by basic position (G lanes per position).  A nucleus position reads h = H[slot]; a singleton position pulls
// h_p = ((row_r == its row) - sum_e A[sg_p, e] H[slot(e)]) / D_p over the nucleus columns of its CSR row (csr_nucleus_pull) — a
// pull per row, no push, no atomics.  Then x_B + delta h must stay in [loB, hiB]; |h| <= EPS counts as zero; x_B a hair outside a bound
// is clamped onto it.
template <int R, int G>
__global__ void __launch_bounds__(BLK) k_rg_rhs_pull(DevView v, RangingBufs b) {
    const int p = (int)(((long)blockIdx.x * BLK + threadIdx.x) / G);
    const int gl = threadIdx.x & (G - 1);
    double acc[R], lo[R], hi[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { lo[r] = -RG_INF; hi[r] = RG_INF; }
    int ks = 0, sg = -1;
    if (p < v.m && !b.fac) {
        ks = v.kslot_of_pos[p];
        if (ks < 0) sg = v.srow_of_pos[p];
    }
    csr_nucleus_pull<R, G>(v, b.blk, sg, gl, acc);
    if (p < v.m && gl == 0) {
        const double x = v.xB[p];
        const double up = fmax(v.hiB[p] - x, 0.0), dn = fmin(v.loB[p] - x, 0.0);
        const double inv = sg >= 0 ? 1.0 / v.sdiag_of_pos[p] : 0.0;
        const double* hrow = b.blk + (size_t)(b.fac ? p : (ks >= 0 ? ks : 0)) * R;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double h;
            if (sg >= 0) h = ((b.req[r] == sg ? 1.0 : 0.0) - acc[r]) * inv;
            else h = hrow[r];
            if (!(fabs(h) > EPS)) continue;
            if (h > 0.0) {
                hi[r] = up / h;
                lo[r] = dn / h;
            } else {
                hi[r] = dn / h;
                lo[r] = up / h;
            }
        }
    }
    rg_block_write<R>(lo, hi, b.part + (size_t)blockIdx.x * 2 * R);
}
// one workgroup: the per-block partials -> out[2 R]
template <int R>
__global__ void __launch_bounds__(BLK) k_rg_final(RangingBufs b, int nb) {
    double lo[R], hi[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { lo[r] = -RG_INF; hi[r] = RG_INF; }
    for (int t = threadIdx.x; t < nb; t += BLK) {
        const double* p = b.part + (size_t)t * 2 * R;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            lo[r] = fmax(lo[r], p[2 * r]);
            hi[r] = fmin(hi[r], p[2 * r + 1]);
        }
    }
    rg_block_write<R>(lo, hi, b.out);
}

static inline int rg_lanes(const Geom& g) { return g.lanes <= 4 ? 4 : g.lanes <= 16 ? 16 : 64; }
int ranging_blocks(const Geom& g, int kind, int N) { return blocks_for((long)(kind == 0 ? N : g.m) * rg_lanes(g)); }

static inline int tab_grid(long n) { return (int)std::min<long>(blocks_for(n), 8192); }  // (the kernels behind it stride)
// Compact factor: "solve these requests into the columns of a block".  One level-scheduled solve per request (pending terms included) on a
// copy of the view with private result vectors; dir 0: blk[:, r] = B^-1 x_r (by position), 1: B^-T x_r (by row); x_r = column r of
// X[m][R], or, without X, the unit vector of h_req[r].  k_fac_solve with src 2 / dst 1 reads its right-hand side from `unit` alone, walks
// every level, and its epilogue stores all m entries of tau / rv.y: nothing of one solve is left for the next, so rv and tau need no clear
// between the solves (rv.x is neither written nor read here).
static void launch_fac_block(const DevView& dv, const Geom& g, const SolveBufs& s, int dir, int nreq, const int* h_req, const double* X,
                             double* blk, hipStream_t st) {
    constexpr int R = RG_BATCH;
    const int m = g.m;
    DevView pv = dv;
    pv.rv = s.rv;
    pv.tau = s.tau;
    for (int r = 0; r < nreq; ++r) {
        if (X) hipLaunchKernelGGL(k_rg_col<R>, dim3(tab_grid(m)), dim3(BLK), 0, st, X, s.unit, m, r);
        else hipLaunchKernelGGL(k_rg_unit, dim3(blocks_for(m)), dim3(BLK), 0, st, s.unit, m, h_req[r]);
        launch_fac_solve(pv, g, dir, 2, 1, s.unit, 1, st);
        hipLaunchKernelGGL(k_rg_take<R>, dim3(blocks_for(m)), dim3(BLK), 0, st, s, blk, m, r, dir);
    }
}
// the block of one batch: rows (kind 0) / nucleus columns (kind 1) of B^-1 of its requests (the sparse rows take their rows here too)
void launch_ranging_block(const DevView& dv, const Geom& g, const RangingBufs& b, int kind, int nreq, const int* h_req, hipStream_t st) {
    constexpr int R = RG_BATCH;
    const int m = g.m;
    const size_t rows = (kind == 0 || b.fac) ? (size_t)m : (size_t)b.k;
    if (rows) (void)hipMemsetAsync(b.blk, 0, sizeof(double) * rows * R, st);
    if (b.fac) {
        launch_fac_block(dv, g, b, kind == 0 ? 1 : 0, nreq, h_req, nullptr, b.blk, st);
    } else if (kind == 0) {
        hipLaunchKernelGGL(k_rg_rows<R>, dim3(blocks_for(b.k), nreq), dim3(BLK), 0, st, dv, b);
    } else if (b.k > 0) {
        hipLaunchKernelGGL(k_rg_cols<R>, dim3(blocks_for(b.k)), dim3(BLK), 0, st, dv, b);
    }
}
void launch_ranging_batch(const DevView& dv, const Geom& g, const RangingBufs& b, int kind, int nreq, const int* h_req, hipStream_t st) {
    constexpr int R = RG_BATCH;
    launch_ranging_block(dv, g, b, kind, nreq, h_req, st);
    const int nb = ranging_blocks(g, kind, b.N);
    if (kind == 0)
        LANES_SWITCH(g.lanes,
                     hipLaunchKernelGGL((k_rg_cost_sweep<R, 4>), dim3(nb), dim3(BLK), 0, st, dv, b),
                     hipLaunchKernelGGL((k_rg_cost_sweep<R, 16>), dim3(nb), dim3(BLK), 0, st, dv, b),
                     hipLaunchKernelGGL((k_rg_cost_sweep<R, 64>), dim3(nb), dim3(BLK), 0, st, dv, b));
    else
        LANES_SWITCH(g.lanes,
                     hipLaunchKernelGGL((k_rg_rhs_pull<R, 4>), dim3(nb), dim3(BLK), 0, st, dv, b),
                     hipLaunchKernelGGL((k_rg_rhs_pull<R, 16>), dim3(nb), dim3(BLK), 0, st, dv, b),
                     hipLaunchKernelGGL((k_rg_rhs_pull<R, 64>), dim3(nb), dim3(BLK), 0, st, dv, b));
    hipLaunchKernelGGL(k_rg_final<R>, dim3(1), dim3(BLK), 0, st, b, nb);
}
