// duals.inc — dual values, reduced costs and a KKT certificate of the current basis (include/minilp_hip.h: mlp_solution_dual_values,
// mlp_solution_reduced_costs, mlp_solution_certificate; DESIGN.md "Duals and the certificate").
//
// Side-effect free: every kernel here reads the solver state and writes ONLY the private buffers of DualsBufs.  In particular
//   - the transposed solve y = B^-T c_B of the explicit representation applies the pending rank-1 terms of the delayed-update mode
//     itself (y_K = W0^T t + V (U^T t)) instead of folding them into W0 (flush_lowrank changes W0's bits);
//   - d, rv, alpha_q, the work vectors and Ctl are not touched (the compact factor's solve runs on a copy of the view whose rv is
//     private; its scratch — fac_x0, the barrier words — is scratch of every solve).
// Costs are the model's internal ones (obj_c: minimisation sense, never the artificial costs of the feasibility phase, which live
// in d only); the host turns signs for a Maximize problem.  No float atomics: every reduction has a fixed order (per-block partials,
// then one block), so two reads of the same state are bit-identical.

constexpr int DU_WT_ROWS = 128;   // rows of W0 per workgroup of the transposed pass (partials: ceil(k / 128) x ld doubles)

// c_B by position; y on singleton rows = c_p / diag (a singleton column's only entry), zero on nucleus rows
__global__ void __launch_bounds__(BLK) k_du_gather(DevView v, DualsBufs b) {
    const int p = blockIdx.x * BLK + threadIdx.x;
    if (p >= v.m) return;
    const double cb = v.obj_c[v.basic_vars[p]];
    b.cb[p] = cb;
    if (b.fac) return;
    const int ks = v.kslot_of_pos[p];
    if (ks < 0) b.y[v.srow_of_pos[p]] = cb / v.sdiag_of_pos[p];
    else b.y[v.row_of_kslot[ks]] = 0.0;
}
// t_K = c_K - F^T y_S (G lanes per nucleus column)
template <int G>
__global__ void __launch_bounds__(BLK) k_du_rhs(DevView v, DualsBufs b) {
    const int slot = (blockIdx.x * BLK + threadIdx.x) / G;
    const int gl = threadIdx.x & (G - 1);
    if (slot >= v.ctl->k) return;
    const int p = v.pos_of_kslot[slot];
    const int var = v.basic_vars[p];
    const int end = v.csc_ptr[var + 1];
    double acc = 0.0;
    for (int e = v.csc_ptr[var] + gl; e < end; e += G) acc += v.csc_val[e] * b.y[v.csc_row[e]];
    acc = group_sum<G>(acc);
    if (gl == 0) b.tK[slot] = b.cb[p] - acc;
}
// W0^T t_K: workgroup (x, s) sums rows [s * DU_WT_ROWS, +DU_WT_ROWS) of columns [x * BLK, +BLK) into part[s][col]
__global__ void __launch_bounds__(BLK) k_du_wt(DevView v, DualsBufs b) {
    const int k = v.ctl->k;
    const int j = blockIdx.x * BLK + threadIdx.x;
    const int i0 = blockIdx.y * DU_WT_ROWS;
    if (i0 >= k || j >= k) return;
    const int i1 = min(k, i0 + DU_WT_ROWS);
    const double* w = v.W + (size_t)i0 * v.ld + j;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int i = i0;
    for (; i + 4 <= i1; i += 4, w += 4 * (size_t)v.ld) {  // four rows in flight per lane
        a0 += __builtin_nontemporal_load(w) * b.tK[i];
        a1 += __builtin_nontemporal_load(w + v.ld) * b.tK[i + 1];
        a2 += __builtin_nontemporal_load(w + 2 * (size_t)v.ld) * b.tK[i + 2];
        a3 += __builtin_nontemporal_load(w + 3 * (size_t)v.ld) * b.tK[i + 3];
    }
    for (; i < i1; ++i, w += v.ld) a0 += __builtin_nontemporal_load(w) * b.tK[i];
    b.part[(size_t)blockIdx.y * v.ld + j] = (a0 + a1) + (a2 + a3);
}
// delayed-update mode: h_j = U_j . t_K, one workgroup per pending term
__global__ void __launch_bounds__(BLK) k_du_lr(DevView v, DualsBufs b) {
    const int j = blockIdx.x, k = v.ctl->k;
    if (j >= v.ctl->nlow) return;
    const double* Uj = v.U + (size_t)j * v.ld;
    double h = 0.0;
    for (int s = threadIdx.x; s < k; s += BLK) h += Uj[s] * b.tK[s];
    h = block_sum(h);
    if (threadIdx.x == 0) b.lrh[j] = h;
}
// y_K = sum of the partials (stripe order) + sum_j V_j h_j (term order), scattered to the nucleus rows
__global__ void __launch_bounds__(BLK) k_du_wt_reduce(DevView v, DualsBufs b) {
    const int k = v.ctl->k;
    const int j = blockIdx.x * BLK + threadIdx.x;
    if (j >= k) return;
    const int ns = (k + DU_WT_ROWS - 1) / DU_WT_ROWS;
    double s = 0.0;
    for (int t = 0; t < ns; ++t) s += b.part[(size_t)t * v.ld + j];
    if (v.lrJ) {
        const int nlow = v.ctl->nlow;
        double l = 0.0;
        for (int q = 0; q < nlow; ++q) l += v.V[(size_t)q * v.ld + j] * b.lrh[q];
        s += l;
    }
    b.y[v.row_of_kslot[j]] = s;
}
// (compact factor: the solve's private rv.y -> y)
__global__ void __launch_bounds__(BLK) k_du_take_rv(DevView v, DualsBufs b) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i < v.m) b.y[i] = b.rv[i].y;
}

// Per-block partial of the certificate: two sums and three (max, index) pairs.  Index ties go to the smaller index.
struct DuAcc {
    double s0, s1;
    double mx[3];
    double ix[3];
};
__device__ __forceinline__ void du_acc_init(DuAcc& a) {
    a.s0 = a.s1 = 0.0;
    for (int q = 0; q < 3; ++q) { a.mx[q] = 0.0; a.ix[q] = -1.0; }
}
__device__ __forceinline__ void du_max(DuAcc& a, int q, double val, double idx) {
    if (val > a.mx[q] || (val == a.mx[q] && val > 0.0 && (a.ix[q] < 0.0 || idx < a.ix[q]))) { a.mx[q] = val; a.ix[q] = idx; }
}
__device__ __forceinline__ void du_merge(DuAcc& a, const DuAcc& o) {
    a.s0 += o.s0;
    a.s1 += o.s1;
    for (int q = 0; q < 3; ++q) du_max(a, q, o.mx[q], o.ix[q]);
}
// fixed-order tree over the workgroup; thread 0 writes the block's record (8 doubles)
__device__ void du_block_write(DuAcc a, double* out) {
    __shared__ DuAcc s[BLK];
    __syncthreads();  // (a second call in the same kernel: the first one's thread 0 has read s[0])
    s[threadIdx.x] = a;
    __syncthreads();
    for (int w = BLK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) du_merge(s[threadIdx.x], s[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const DuAcc& r = s[0];
        out[0] = r.s0; out[1] = r.s1;
        out[2] = r.mx[0]; out[3] = r.ix[0]; out[4] = r.mx[1]; out[5] = r.ix[1]; out[6] = r.mx[2]; out[7] = r.ix[2];
    }
}
__device__ __forceinline__ double du_x(const DevView& v, int var) {
    const int loc = v.var_loc[var];
    return loc >= 0 ? v.xB[loc] : v.xN[-1 - loc];
}

// Reduced costs by variable over A's CSC (G lanes per column, like k_recalc_d): r_j = c_j - a_j . y, basic entries zeroed exactly;
// the dual value of a row is y on its row, zeroed exactly when its slack is basic.  Certificate terms of the same pass, per block:
//   s0 = c . x over the structural variables, s1 = sum_j r_j l_j (l_j: the bound minimising r_j x_j; x_j when that bound is infinite,
//   or the variable is fixed by fix_var), mx0 = max bound violation (structural), mx1 = max dual infeasibility |r_j| at an infinite
//   bound, mx2 = max |c_j - a_j . y| over basic j (the accuracy of y).
template <int G>
__global__ void __launch_bounds__(BLK) k_du_reduced(DevView v, DualsBufs b) {
    const int var = (blockIdx.x * BLK + threadIdx.x) / G;
    const int gl = threadIdx.x & (G - 1);
    DuAcc a;
    du_acc_init(a);
    double acc = 0.0;
    if (var < b.N) {
        const int end = v.csc_ptr[var + 1];
        for (int e = v.csc_ptr[var] + gl; e < end; e += G) acc += v.csc_val[e] * b.y[v.csc_row[e]];
    }
    acc = group_sum<G>(acc);
    if (var < b.N && gl == 0) {
        const int loc = v.var_loc[var];
        const double x = loc >= 0 ? v.xB[loc] : v.xN[-1 - loc];
        const double lo = v.var_lo[var], hi = v.var_hi[var];
        double r = v.obj_c[var] - acc;
        if (loc >= 0) {
            a.mx[2] = fabs(r);
            a.ix[2] = (double)var;
            r = 0.0;
        } else {
            double l;
            if (r == 0.0 || (v.nbflags[-1 - loc] & NB_FIXED)) l = x;
            else l = r > 0.0 ? lo : hi;
            if (r != 0.0 && isinf(l)) {
                l = x;
                a.mx[1] = fabs(r);
                a.ix[1] = (double)var;
            }
            a.s1 = r * l;
        }
        b.r[var] = r;
        if (var >= b.nv) b.pi[var - b.nv] = loc >= 0 ? 0.0 : b.y[var - b.nv];
        else {
            a.s0 = v.obj_c[var] * x;
            const double bv = fmax(fmax(lo - x, x - hi), 0.0);
            if (bv > 0.0) { a.mx[0] = bv; a.ix[0] = (double)var; }
        }
    }
    du_block_write(a, b.bpart + (size_t)blockIdx.x * 8);
}
// Row activities over the CSR (every entry but the row's own slack: a cut row taken from the tableau has terms on the slacks of other
// rows): s0 = b . y, mx0 = max violation of the row against its slack's bounds (slack = rhs - activity must lie in [lo_s, hi_s]).
template <int G>
__global__ void __launch_bounds__(BLK) k_du_rows(DevView v, DualsBufs b) {
    const int i = (blockIdx.x * BLK + threadIdx.x) / G;
    const int gl = threadIdx.x & (G - 1);
    DuAcc a;
    du_acc_init(a);
    double acc = 0.0;
    if (i < v.m) {
        const int end = v.csr_ptr[i + 1];
        for (int e = v.csr_ptr[i] + gl; e < end; e += G) {
            const int col = v.csr_col[e];
            if (col != b.nv + i) acc += v.csr_val[e] * du_x(v, col);
        }
    }
    acc = group_sum<G>(acc);
    if (i < v.m && gl == 0) {
        const int sv = b.nv + i;
        const double s = b.rhs[i] - acc;
        const double viol = fmax(fmax(v.var_lo[sv] - s, s - v.var_hi[sv]), 0.0);
        if (viol > 0.0) { a.mx[0] = viol; a.ix[0] = (double)i; }
        a.s0 = b.rhs[i] * b.y[i];
    }
    du_block_write(a, b.rpart + (size_t)blockIdx.x * 8);
}
// one workgroup: the partials of both passes in block order -> cert[0..11]
__global__ void __launch_bounds__(BLK) k_du_final(DualsBufs b, int nb_var, int nb_row) {
    DuAcc a, r;
    du_acc_init(a);
    du_acc_init(r);
    for (int t = threadIdx.x; t < nb_var; t += BLK) {  // (each thread: a strided, fixed subset; then the fixed tree)
        const double* p = b.bpart + (size_t)t * 8;
        DuAcc o{p[0], p[1], {p[2], p[4], p[6]}, {p[3], p[5], p[7]}};
        du_merge(a, o);
    }
    for (int t = threadIdx.x; t < nb_row; t += BLK) {
        const double* p = b.rpart + (size_t)t * 8;
        DuAcc o{p[0], p[1], {p[2], p[4], p[6]}, {p[3], p[5], p[7]}};
        du_merge(r, o);
    }
    du_block_write(a, b.cert);
    du_block_write(r, b.cert + 8);
}

void launch_duals(const DevView& dv, const Geom& g, const DualsBufs& b, hipStream_t st) {
    const int m = g.m;
    hipLaunchKernelGGL(k_du_gather, dim3(blocks_for(m)), dim3(BLK), 0, st, dv, b);
    if (b.fac) {  // compact factor: the level-scheduled BTRAN of c_B (pending terms included) into a private rv
        DevView pv = dv;
        pv.rv = b.rv;
        launch_fac_solve(pv, g, 1, 2, 1, b.cb, 1, st);
        hipLaunchKernelGGL(k_du_take_rv, dim3(blocks_for(m)), dim3(BLK), 0, st, dv, b);
    } else if (b.k > 0) {
        LANES_SWITCH(g.lanes,
                     hipLaunchKernelGGL(k_du_rhs<4>, dim3(blocks_for((long)b.k * 4)), dim3(BLK), 0, st, dv, b),
                     hipLaunchKernelGGL(k_du_rhs<16>, dim3(blocks_for((long)b.k * 16)), dim3(BLK), 0, st, dv, b),
                     hipLaunchKernelGGL(k_du_rhs<64>, dim3(blocks_for((long)b.k * 64)), dim3(BLK), 0, st, dv, b));
        hipLaunchKernelGGL(k_du_wt, dim3(blocks_for(b.k), (b.k + DU_WT_ROWS - 1) / DU_WT_ROWS), dim3(BLK), 0, st, dv, b);
        if (dv.lrJ) hipLaunchKernelGGL(k_du_lr, dim3(LR_MAX), dim3(BLK), 0, st, dv, b);
        hipLaunchKernelGGL(k_du_wt_reduce, dim3(blocks_for(b.k)), dim3(BLK), 0, st, dv, b);
    }
    const int nbv = duals_var_blocks(g, b.N), nbr = duals_row_blocks(g);
    LANES_SWITCH(g.lanes,
                 hipLaunchKernelGGL(k_du_reduced<4>, dim3(nbv), dim3(BLK), 0, st, dv, b),
                 hipLaunchKernelGGL(k_du_reduced<16>, dim3(nbv), dim3(BLK), 0, st, dv, b),
                 hipLaunchKernelGGL(k_du_reduced<64>, dim3(nbv), dim3(BLK), 0, st, dv, b));
    LANES_SWITCH(g.lanes,
                 hipLaunchKernelGGL(k_du_rows<4>, dim3(nbr), dim3(BLK), 0, st, dv, b),
                 hipLaunchKernelGGL(k_du_rows<16>, dim3(nbr), dim3(BLK), 0, st, dv, b),
                 hipLaunchKernelGGL(k_du_rows<64>, dim3(nbr), dim3(BLK), 0, st, dv, b));
    hipLaunchKernelGGL(k_du_final, dim3(1), dim3(BLK), 0, st, b, nbv, nbr);
}
static inline int du_lanes(const Geom& g) { return g.lanes <= 4 ? 4 : g.lanes <= 16 ? 16 : 64; }
int duals_var_blocks(const Geom& g, int N) { return blocks_for((long)N * du_lanes(g)); }
int duals_row_blocks(const Geom& g) { return blocks_for((long)g.m * du_lanes(g)); }
int duals_wt_stripes(int k) { return (k + DU_WT_ROWS - 1) / DU_WT_ROWS; }
