// tableau.inc — reading the simplex tableau of the current basis (include/minilp_hip.h: mlp_solution_binv_rows, mlp_solution_binv_cols,
// mlp_solution_tableau_rows, mlp_solution_tableau_cols, mlp_solution_basis_solve; DESIGN.md §7.4).
//
// Requests are served in batches of R = RG_BATCH that share one pass over the large operand:
//   rows of B^-1:      the block rho[m][R] of launch_ranging_block (ranging.inc), read back as it is;
//   tableau rows:      the same block, then k_tab_sweep — one pass over A's CSC, alpha = csc_block_dot (ranging.inc) kept as it is in a
//                      dense block [N][R] by variable (basic variables: 0, the requested variable itself: exactly 1) — and the count /
//                      scan / fill of cuts.inc, which turn the block into sparse rows sorted by variable (launch_rows_generate, the
//                      phase 1 that the Gomory and the GMI round share, then launch_cut_fill);
//   solves with dense right-hand sides X[m][R] (interleaved like the block: entry i of all R right-hand sides is one 128-byte line):
//       FTRAN  Y_K = W X_K (one wave per row of W, lanes stride its columns, R accumulators per lane, xor tree of the wave), then the pull
//              Y_S = D^-1 (X_S - F Y_K) per singleton row over its CSR entries;
//       BTRAN  Y_S = D^-1 X_S, T_K = X_K - F^T Y_S as a pull per nucleus column over its CSC entries, Y_K = W^T T_K (one thread per column
//              of W, R accumulators, the right-hand sides wave-uniform; partial sums per row stripe, reduced in stripe order);
//       W = W0 + the pending rank-1 terms of the delayed-update mode, applied in term order, never folded;
//       compact factor: one level-scheduled solve per right-hand side on a copy of the view with private result vectors
//              (launch_fac_block, ranging.inc);
//       the two pulls are the accumulators of ranging.inc: csr_nucleus_pull (k_tab_f_pull), csc_block_dot (k_tab_b_rhs).
// Side-effect free in the sense of duals.inc: only the private buffers of TabBufs / RangingBufs are written.  No float atomics; every sum
// has a fixed order that depends on its own right-hand side alone (never on what else is in the batch, or in which place), so the numbers
// of a request are bit-identical whatever the call.  Every kernel walks its index space with a stride loop or a grid computed to cover
// it (long arithmetic): no size of m, k or N is left out.

constexpr int TB_STRIPES = 16;  // the transposed pass splits the rows of W0 into at most this many stripes (its partials: stripes x k x R)

template <int R, int G>
__global__ void __launch_bounds__(BLK) k_tab_sweep(DevView v, RangingBufs b, double* __restrict__ ad) {
    const int var = (int)(((long)blockIdx.x * BLK + threadIdx.x) / G);
    const int gl = threadIdx.x & (G - 1);
    double acc[R];
    int loc = 0;
    if (var < b.N) loc = v.var_loc[var];
    const bool live = var < b.N && loc < 0;
    csc_block_dot<R, G>(v, b.blk, live, var, gl, acc);
    if (var < b.N && gl == 0) {  // a basic variable: 0, and exactly 1 in the rows that were asked for it (req: -1 at an empty place)
        if (!live) {
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = b.req[r] == loc ? 1.0 : 0.0;
        }
        store_block_row<R>(ad + (size_t)var * R, acc);
    }
}

// right-hand sides formed on the device (X cleared beforehand), workgroup r = request r: mode 1 the unit vector of row req[r],
// mode 2 column req[r] of [A | I] (its CSC entries, by row)
template <int R>
__global__ void __launch_bounds__(BLK) k_tab_rhs(DevView v, TabBufs b, const int* __restrict__ req, int mode) {
    const int r = blockIdx.x;
    const int id = req[r];
    if (id < 0) return;
    if (mode == 1) {
        if (threadIdx.x == 0) b.X[(size_t)id * R + r] = 1.0;
        return;
    }
    const int end = v.csc_ptr[id + 1];
    for (int e = v.csc_ptr[id] + threadIdx.x; e < end; e += BLK) b.X[(size_t)v.csc_row[e] * R + r] = v.csc_val[e];
}

// ------------------------------------------------------------------- FTRAN, explicit inverse
// X_K by column slot
template <int R>
__global__ void __launch_bounds__(BLK) k_tab_f_gather(DevView v, TabBufs b) {
    const long n = (long)b.k * R, step = (long)gridDim.x * BLK;
    for (long i = (long)blockIdx.x * BLK + threadIdx.x; i < n; i += step)
        b.XK[i] = b.X[(size_t)v.row_of_kslot[i / R] * R + (i % R)];
}
// pending terms: lrh[j][r] = Z_j . XK[:, r] with Z = V (FTRAN, by column slot) or U (BTRAN, by row slot); workgroup j, thread (g, r) sums
// the slots g, g + 16, ... of right-hand side r, then the 16 partial sums in the order of g
template <int R>
__global__ void __launch_bounds__(BLK) k_tab_lr(DevView v, TabBufs b, int use_u) {
    __shared__ double sh[BLK];
    const int j = blockIdx.x;
    const int nlow = min(v.ctl->nlow, LR_MAX);
    if (j >= nlow) return;
    const double* z = (use_u ? v.U : v.V) + (size_t)j * v.ld;
    const int r = threadIdx.x % R, g = threadIdx.x / R;
    double h = 0.0;
    for (int s = g; s < b.k; s += BLK / R) h += z[s] * b.XK[(size_t)s * R + r];
    sh[threadIdx.x] = h;
    __syncthreads();
    if ((int)threadIdx.x < R) {
        double t = 0.0;
        for (int q = 0; q < BLK / R; ++q) t += sh[q * R + threadIdx.x];
        b.lrh[j * R + threadIdx.x] = t;
    }
}
// Y_K = W X_K: one wave per row slot (stride loop over the rows), lanes stride the columns in storage order, then the xor tree of the wave;
// lane r < R finishes right-hand side r: the pending terms in term order, then the stores (one 128-byte line each)
template <int R>
__global__ void __launch_bounds__(BLK) k_tab_wx(DevView v, TabBufs b) {
    const int k = b.k, nlow = v.lrJ ? min(v.ctl->nlow, LR_MAX) : 0;
    const int lane = threadIdx.x & 63;
    const long nw = (long)gridDim.x * (BLK / 64);
    for (long s = (long)blockIdx.x * (BLK / 64) + (threadIdx.x >> 6); s < k; s += nw) {
        const double* w = v.W + (size_t)s * v.ld;
        double acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.0;
        for (int c = lane; c < k; c += 64) {
            const double a = __builtin_nontemporal_load(w + c);
            const double2* xx = reinterpret_cast<const double2*>(b.XK + (size_t)c * R);
#pragma unroll
            for (int r = 0; r < R; r += 2) {
                const double2 t = xx[r >> 1];
                acc[r] += a * t.x;
                acc[r + 1] += a * t.y;
            }
        }
        double mine = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const double t = group_sum<64>(acc[r]);
            if (lane == r) mine = t;
        }
        if (lane < R) {
            if (nlow) {
                double l = 0.0;
                for (int j = 0; j < nlow; ++j) l += v.U[(size_t)j * v.ld + s] * b.lrh[j * R + lane];
                mine += l;
            }
            b.YK[(size_t)s * R + lane] = mine;
            b.Y[(size_t)v.pos_of_kslot[s] * R + lane] = mine;
        }
    }
}
// singleton positions: Y_p = (X[row_p] - sum_e A[row_p, e] Y_K[slot(e)]) / D_p over the nucleus columns of the CSR row (G lanes, storage
// order, xor tree of the lane group) — a pull per row, no push, no atomics
template <int R, int G>
__global__ void __launch_bounds__(BLK) k_tab_f_pull(DevView v, TabBufs b) {
    const int p = (int)(((long)blockIdx.x * BLK + threadIdx.x) / G);
    const int gl = threadIdx.x & (G - 1);
    double acc[R];
    int sg = -1;
    if (p < v.m && v.kslot_of_pos[p] < 0) sg = v.srow_of_pos[p];
    csr_nucleus_pull<R, G>(v, b.YK, sg, gl, acc);
    if (sg >= 0 && gl == 0) {
        const double d = v.sdiag_of_pos[p];
        const double2* xx = reinterpret_cast<const double2*>(b.X + (size_t)sg * R);
        double2* out = reinterpret_cast<double2*>(b.Y + (size_t)p * R);
#pragma unroll
        for (int r = 0; r < R; r += 2) {  // (pair by pair: load, finish, store)
            const double2 x = xx[r >> 1];
            double2 t;
            t.x = (x.x - acc[r]) / d;
            t.y = (x.y - acc[r + 1]) / d;
            out[r >> 1] = t;
        }
    }
}

// ------------------------------------------------------------------- BTRAN, explicit inverse
// Y on singleton rows = X_p / D_p (Y cleared beforehand: zero on nucleus rows until the reduce writes them)
template <int R>
__global__ void __launch_bounds__(BLK) k_tab_b_gather(DevView v, TabBufs b) {
    const long n = (long)v.m * R, step = (long)gridDim.x * BLK;
    for (long i = (long)blockIdx.x * BLK + threadIdx.x; i < n; i += step) {
        const long p = i / R;
        if (v.kslot_of_pos[p] < 0) b.Y[(size_t)v.srow_of_pos[p] * R + (i % R)] = b.X[i] / v.sdiag_of_pos[p];
    }
}
// T_K = X_K - F^T Y_S by row slot: a pull over the CSC entries of the nucleus column (G lanes; its nucleus rows read exact zeros)
template <int R, int G>
__global__ void __launch_bounds__(BLK) k_tab_b_rhs(DevView v, TabBufs b) {
    const int slot = (int)(((long)blockIdx.x * BLK + threadIdx.x) / G);
    const int gl = threadIdx.x & (G - 1);
    double acc[R];
    int p = -1, var = 0;
    if (slot < b.k) {
        p = v.pos_of_kslot[slot];
        var = v.basic_vars[p];
    }
    csc_block_dot<R, G>(v, b.Y, p >= 0, var, gl, acc);
    if (p >= 0 && gl == 0) {
        const double2* xx = reinterpret_cast<const double2*>(b.X + (size_t)p * R);
        double2* out = reinterpret_cast<double2*>(b.XK + (size_t)slot * R);
#pragma unroll
        for (int r = 0; r < R; r += 2) {  // (pair by pair: load, subtract, store)
            const double2 x = xx[r >> 1];
            double2 t;
            t.x = x.x - acc[r];
            t.y = x.y - acc[r + 1];
            out[r >> 1] = t;
        }
    }
}
// W0^T T_K: workgroup (x, s) sums rows [s * rows, + rows) of columns [x * BLK, + BLK) into part[s][column][R]; the R right-hand-side
// entries of a row are wave-uniform
template <int R>
__global__ void __launch_bounds__(BLK) k_tab_wt(DevView v, TabBufs b, int rows) {
    const int k = b.k;
    const long c = (long)blockIdx.x * BLK + threadIdx.x;
    const long i0 = (long)blockIdx.y * rows;
    if (i0 >= k || c >= k) return;
    const long i1 = min((long)k, i0 + rows);
    const double* w = v.W + (size_t)i0 * v.ld + c;
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
#pragma unroll 4
    for (long i = i0; i < i1; ++i, w += v.ld) {
        const double a = __builtin_nontemporal_load(w);
        const double* t = b.XK + (size_t)i * R;
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] += a * t[r];
    }
    store_block_row<R>(b.part + ((size_t)blockIdx.y * k + c) * R, acc);
}
// Y_K = the partials in stripe order + sum_j V_j (U_j . T_K) in term order, scattered to the nucleus rows
template <int R>
__global__ void __launch_bounds__(BLK) k_tab_wt_reduce(DevView v, TabBufs b, int ns) {
    const int k = b.k, nlow = v.lrJ ? min(v.ctl->nlow, LR_MAX) : 0;
    const long n = (long)k * R, step = (long)gridDim.x * BLK;
    for (long i = (long)blockIdx.x * BLK + threadIdx.x; i < n; i += step) {
        const long c = i / R;
        const int r = (int)(i % R);
        double s = 0.0;
        for (int t = 0; t < ns; ++t) s += b.part[(size_t)t * n + i];
        if (nlow) {
            double l = 0.0;
            for (int j = 0; j < nlow; ++j) l += v.V[(size_t)j * v.ld + c] * b.lrh[j * R + r];
            s += l;
        }
        b.Y[(size_t)v.row_of_kslot[c] * R + r] = s;
    }
}
int tab_wt_stripes(int k) { return std::max(1, std::min(TB_STRIPES, (k + DU_WT_ROWS - 1) / DU_WT_ROWS)); }
static inline int tab_wt_rows(int k) { const int ns = tab_wt_stripes(k); return (k + ns - 1) / ns; }

// Phase 1 of a batch of sparse rows, whatever their kind (kernels.h: RowKind): the block of rows of B^-1, the kind's sweep over A into the
// dense block, (GMI: the clear of the requests that met a free column,) count, scan, heads.  Phase 2 is launch_cut_fill on the block.
void launch_rows_generate(const DevView& dv, const Geom& g, const RangingBufs& b, RowKind kind, const GmiBufs* gb, int nreq, const int* h_req,
                          double* dense, int* cnt, int* off, int* sums, int* len, double* rhs, hipStream_t st) {
    constexpr int R = RG_BATCH;
    launch_ranging_block(dv, g, b, 0, nreq, h_req, st);
    if (kind == ROWS_GMI) hipLaunchKernelGGL(k_gmi_head<R>, dim3(1), dim3(64), 0, st, dv, b.req, *gb);
    const int nb = ranging_blocks(g, 0, b.N);
#define ROW_SWEEP(G)                                                                                                              \
    do {                                                                                                                          \
        if (kind == ROWS_TABLEAU) hipLaunchKernelGGL((k_tab_sweep<R, G>), dim3(nb), dim3(BLK), 0, st, dv, b, dense);              \
        else if (kind == ROWS_GOMORY) hipLaunchKernelGGL((k_cut_sweep<R, G>), dim3(nb), dim3(BLK), 0, st, dv, b, dense);          \
        else hipLaunchKernelGGL((k_gmi_sweep<R, G>), dim3(nb), dim3(BLK), 0, st, dv, b, *gb, dense);                              \
    } while (0)
    LANES_SWITCH(g.lanes, ROW_SWEEP(4), ROW_SWEEP(16), ROW_SWEEP(64));
#undef ROW_SWEEP
    const int nseg = cut_segments(b.N);
    const long n = (long)R * nseg;
    const int* total = sums + (n + SCAN_TILE - 1) / SCAN_TILE;
    if (kind == ROWS_GMI) {
        hipLaunchKernelGGL(k_gmi_clear<R>, dim3(blocks_for((long)b.N * R)), dim3(BLK), 0, st, *gb, b.N, dense);
        hipLaunchKernelGGL((k_cut_compact<R, 2>), dim3(blocks_for(n)), dim3(BLK), 0, st, dense, b.N, nseg, cnt, nullptr, nullptr, nullptr,
                           dv.var_loc, dv.xN, gb->part);
    } else {
        hipLaunchKernelGGL((k_cut_compact<R, 0>), dim3(blocks_for(n)), dim3(BLK), 0, st, dense, b.N, nseg, cnt, nullptr, nullptr, nullptr,
                           nullptr, nullptr, nullptr);
    }
    launch_exclusive_scan(cnt, off, n, sums, st);
    if (kind == ROWS_GMI) hipLaunchKernelGGL(k_gmi_heads<R>, dim3(R), dim3(BLK), 0, st, *gb, off, total, nseg, len, rhs);
    else hipLaunchKernelGGL(k_cut_heads<R>, dim3(1), dim3(64), 0, st, dv, b.req, off, total, nseg, len, rhs);
}
// right-hand sides of a batch formed on the device: mode 1 unit vectors of the rows req[], mode 2 the columns req[] of [A | I]
void launch_tab_rhs(const DevView& dv, const TabBufs& b, const int* req, int nreq, int mode, hipStream_t st) {
    constexpr int R = RG_BATCH;
    (void)hipMemsetAsync(b.X, 0, sizeof(double) * (size_t)dv.m * R, st);
    if (nreq > 0) hipLaunchKernelGGL(k_tab_rhs<R>, dim3(nreq), dim3(BLK), 0, st, dv, b, req, mode);
}
// one batch of solves: Y = B^-1 X (X by row, Y by position) or, transposed, Y = B^-T X (X by position, Y by row)
void launch_tab_solve(const DevView& dv, const Geom& g, const TabBufs& b, int transpose, int nreq, hipStream_t st) {
    constexpr int R = RG_BATCH;
    const int m = g.m, k = b.k;
    if (m <= 0) return;
    (void)hipMemsetAsync(b.Y, 0, sizeof(double) * (size_t)m * R, st);
    if (b.fac) {
        launch_fac_block(dv, g, b, transpose ? 1 : 0, nreq, nullptr, b.X, b.Y, st);
        return;
    }
    const int G = rg_lanes(g);
    if (!transpose) {
        if (k > 0) {
            hipLaunchKernelGGL(k_tab_f_gather<R>, dim3(tab_grid((long)k * R)), dim3(BLK), 0, st, dv, b);
            if (dv.lrJ) hipLaunchKernelGGL(k_tab_lr<R>, dim3(LR_MAX), dim3(BLK), 0, st, dv, b, 0);
            hipLaunchKernelGGL(k_tab_wx<R>, dim3(tab_grid((long)k * 64)), dim3(BLK), 0, st, dv, b);
        }
        const int nb = blocks_for((long)m * G);
        LANES_SWITCH(g.lanes,
                     hipLaunchKernelGGL((k_tab_f_pull<R, 4>), dim3(nb), dim3(BLK), 0, st, dv, b),
                     hipLaunchKernelGGL((k_tab_f_pull<R, 16>), dim3(nb), dim3(BLK), 0, st, dv, b),
                     hipLaunchKernelGGL((k_tab_f_pull<R, 64>), dim3(nb), dim3(BLK), 0, st, dv, b));
    } else {
        hipLaunchKernelGGL(k_tab_b_gather<R>, dim3(tab_grid((long)m * R)), dim3(BLK), 0, st, dv, b);
        if (k > 0) {
            const int nb = blocks_for((long)k * G);
            LANES_SWITCH(g.lanes,
                         hipLaunchKernelGGL((k_tab_b_rhs<R, 4>), dim3(nb), dim3(BLK), 0, st, dv, b),
                         hipLaunchKernelGGL((k_tab_b_rhs<R, 16>), dim3(nb), dim3(BLK), 0, st, dv, b),
                         hipLaunchKernelGGL((k_tab_b_rhs<R, 64>), dim3(nb), dim3(BLK), 0, st, dv, b));
            const int ns = tab_wt_stripes(k), rows = tab_wt_rows(k);
            hipLaunchKernelGGL(k_tab_wt<R>, dim3(blocks_for(k), ns), dim3(BLK), 0, st, dv, b, rows);
            if (dv.lrJ) hipLaunchKernelGGL(k_tab_lr<R>, dim3(LR_MAX), dim3(BLK), 0, st, dv, b, 1);
            hipLaunchKernelGGL(k_tab_wt_reduce<R>, dim3(tab_grid((long)k * R)), dim3(BLK), 0, st, dv, b, ns);
        }
    }
}
