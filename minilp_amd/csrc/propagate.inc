// propagate.inc — bound propagation from row activities (include/minilp_hip.h: mlp_solution_propagate_bounds,
// mlp_solution_tighten_by_propagation; DESIGN.md §7.9).  A read like fixing.inc's: the matrix, the bounds and the fixed flags are read,
// only the private buffers of PropBufs are written.  The model is the internal one: every CSR row r is sum_j a_rj x_j = rhs_r over all
// its entries (its own slack, and in a cut row the slacks of other rows), every column j of [A | I] has the working bounds [lo_j, hi_j].
//   k_pp_setup   the working bounds [N] from var_lo / var_hi; a non-basic column flagged NB_FIXED is [xN, xN];
//   k_pp_rows    one pass over the CSR, G lanes per row (the lanes stride over the row, the partial sums meet in group_sum's xor tree,
//                as in k_du_rows): minfin / maxfin, the sums of the finite minimal / maximal contributions, and mininf / maxinf, the
//                integer counts of the infinite ones;
//   k_pp_cols    one pass over the CSC of [A | I], G lanes per column (as in k_du_reduced): per entry the candidates from the rest of
//                its row, reduced by min and max (exact: the order is immaterial), then per column the rounding of a marked variable,
//                the acceptance test, the clamp and the infeasibility test.  Both bounds are written into the OTHER buffer pair, so a
//                round reads only the bounds of its start (Jacobi).  Two integer words: bounds accepted, columns found infeasible;
//   k_pp_list    the structural variables whose working bounds differ from var_lo / var_hi (NB_FIXED columns left out), compacted per
//                tile exactly as k_cb_classify does; launch_exclusive_scan and k_cb_gather finish the list: ascending, no atomics.
// No float atomics (the two words are integer counts: their order is immaterial).  Every kernel strides: rows, columns and tiles beyond
// what one grid covers are served by the same workgroups, with long indices.

template <int G>
__device__ __forceinline__ int group_sum_int(int x) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
template <int G>
__device__ __forceinline__ double group_min(double x) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) x = fmin(x, __shfl_xor(x, o, 64));
    return x;
}
template <int G>
__device__ __forceinline__ double group_max(double x) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
    return x;
}

__global__ void __launch_bounds__(BLK) k_pp_setup(DevView v, PropBufs b) {
    const long step = (long)gridDim.x * BLK;
    for (long j = (long)blockIdx.x * BLK + threadIdx.x; j < b.N; j += step) {
        double lo = v.var_lo[j], hi = v.var_hi[j];
        const int loc = v.var_loc[j];
        if (loc < 0 && (v.nbflags[-1 - loc] & NB_FIXED)) lo = hi = v.xN[-1 - loc];
        b.lo[0][j] = lo;
        b.hi[0][j] = hi;
    }
}

template <int G>
__global__ void __launch_bounds__(BLK) k_pp_rows(DevView v, PropBufs b, int cur) {
    const double* __restrict__ lo = b.lo[cur];
    const double* __restrict__ hi = b.hi[cur];
    const int gl = threadIdx.x & (G - 1);
    const long step = (long)gridDim.x * (BLK / G);
    if (blockIdx.x == 0 && threadIdx.x == 0) b.word[0] = b.word[1] = 0;  // (k_pp_cols of this round runs behind this kernel)
    for (long i0 = (long)blockIdx.x * (BLK / G); i0 < b.m; i0 += step) {  // (i0 is the workgroup's: every lane makes the same trips)
        const long i = i0 + threadIdx.x / G;
        double mn = 0.0, mx = 0.0;
        int mni = 0, mxi = 0;
        if (i < b.m) {
            const int end = v.csr_ptr[i + 1];
            for (int e = v.csr_ptr[i] + gl; e < end; e += G) {
                const double a = v.csr_val[e];
                if (a == 0.0) continue;
                const int col = v.csr_col[e];
                const double l = lo[col], u = hi[col];
                const double cmin = a > 0.0 ? a * l : a * u, cmax = a > 0.0 ? a * u : a * l;
                if (isinf(cmin)) mni += 1;
                else mn += cmin;
                if (isinf(cmax)) mxi += 1;
                else mx += cmax;
            }
        }
        mn = group_sum<G>(mn);
        mx = group_sum<G>(mx);
        mni = group_sum_int<G>(mni);
        mxi = group_sum_int<G>(mxi);
        if (i < b.m && gl == 0) {
            b.rowfin[i] = make_double2(mn, mx);
            b.rowinf[i] = make_int2(mni, mxi);
        }
    }
}

template <int G>
__global__ void __launch_bounds__(BLK) k_pp_cols(DevView v, PropBufs b, int cur) {
    __shared__ int s_cnt[2];
    const double* __restrict__ lo = b.lo[cur];
    const double* __restrict__ hi = b.hi[cur];
    double* __restrict__ nlo = b.lo[cur ^ 1];
    double* __restrict__ nhi = b.hi[cur ^ 1];
    const double inf = __builtin_huge_val();
    const int gl = threadIdx.x & (G - 1);
    const long step = (long)gridDim.x * (BLK / G);
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    int acc = 0, bad = 0;
    for (long j0 = (long)blockIdx.x * (BLK / G); j0 < b.N; j0 += step) {
        const long j = j0 + threadIdx.x / G;
        double up = inf, dn = -inf, l = 0.0, u = 0.0;
        if (j < b.N) {
            l = lo[j];
            u = hi[j];
            const int end = v.csc_ptr[j + 1];
            for (int e = v.csc_ptr[j] + gl; e < end; e += G) {
                const double a = v.csc_val[e];
                if (a == 0.0) continue;
                const int r = v.csc_row[e];
                const double2 fin = b.rowfin[r];
                const int2 ni = b.rowinf[r];
                const double cmin = a > 0.0 ? a * l : a * u, cmax = a > 0.0 ? a * u : a * l;
                const bool imin = isinf(cmin), imax = isinf(cmax);
                const double rest_min = (!imin && ni.x == 0) ? fin.x - cmin : ((imin && ni.x == 1) ? fin.x : -inf);
                const double rest_max = (!imax && ni.y == 0) ? fin.y - cmax : ((imax && ni.y == 1) ? fin.y : inf);
                const double rhs = b.rhs[r];
                const double t_min = (rhs - rest_min) / a, t_max = (rhs - rest_max) / a;
                up = fmin(up, a > 0.0 ? t_min : t_max);
                dn = fmax(dn, a > 0.0 ? t_max : t_min);
            }
        }
        up = group_min<G>(up);
        dn = group_max<G>(dn);
        if (j < b.N && gl == 0) {
            if (b.mask && j < b.nv && b.mask[j]) {
                up = floor(up + 1e-9);
                dn = ceil(dn - 1e-9);
            }
            const bool acc_u = (isinf(u) && isfinite(up)) || up < u - 1e-7 * fmax(1.0, fabs(u));
            const bool acc_l = (isinf(l) && isfinite(dn)) || dn > l + 1e-7 * fmax(1.0, fabs(l));
            double out_l = l, out_u = u;
            if (acc_l) {
                const double over = dn - u;  // against the bounds of the round's start
                if (over > 1e-9 * fmax(1.0, fabs(u))) bad += 1;
                out_l = over > 0.0 ? u : dn;
                acc += 1;
            }
            if (acc_u) {
                const double over = l - up;
                if (over > 1e-9 * fmax(1.0, fabs(l))) bad += 1;
                out_u = over > 0.0 ? l : up;
                acc += 1;
            }
            nlo[j] = out_l;
            nhi[j] = out_u;
        }
    }
    if (acc) atomicAdd(&s_cnt[0], acc);
    if (bad) atomicAdd(&s_cnt[1], bad);
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(b.word + threadIdx.x, s_cnt[threadIdx.x]);
}

// the list: k_cb_classify's compaction on another predicate (c.nv, c.tcnt, c.svar / slo / shi are the staging of CutoffBufs)
__global__ void __launch_bounds__(BLK) k_pp_list(DevView v, PropBufs b, CutoffBufs c, int cur) {
    __shared__ int s_w[BLK / 64];
    const double* __restrict__ lo = b.lo[cur];
    const double* __restrict__ hi = b.hi[cur];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long ntiles = ((long)c.nv + BLK - 1) / BLK;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long j = tile * BLK + threadIdx.x;
        bool listed = false;
        double nlo = 0.0, nhi = 0.0;
        if (j < c.nv) {
            const int loc = v.var_loc[j];
            if (!(loc < 0 && (v.nbflags[-1 - loc] & NB_FIXED))) {
                nlo = lo[j];
                nhi = hi[j];
                listed = nlo != v.var_lo[j] || nhi != v.var_hi[j];
            }
        }
        const unsigned long long bal = __ballot(listed);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_w[w] = __popcll(bal);
        __syncthreads();
        int base = 0, total = 0;
#pragma unroll
        for (int q = 0; q < BLK / 64; ++q) {
            const int n = s_w[q];
            if (q < w) base += n;
            total += n;
        }
        if (listed) {
            const size_t at = (size_t)tile * BLK + base + before;
            c.svar[at] = (uint32_t)j;
            c.slo[at] = nlo;
            c.shi[at] = nhi;
        }
        if (threadIdx.x == 0) c.tcnt[tile] = total;
        __syncthreads();  // (s_w is written again by the next tile)
    }
}

static inline int prop_lanes(const Geom& g) { return g.lanes <= 4 ? 4 : g.lanes <= 16 ? 16 : 64; }
void launch_prop_setup(const DevView& dv, const PropBufs& b, hipStream_t st) {
    hipLaunchKernelGGL(k_pp_setup, dim3(tab_grid(b.N)), dim3(BLK), 0, st, dv, b);
}
void launch_prop_round(const DevView& dv, const Geom& g, const PropBufs& b, int cur, hipStream_t st) {
    const int G = prop_lanes(g);
    const int nbr = tab_grid((long)b.m * G), nbc = tab_grid((long)b.N * G);
    LANES_SWITCH(g.lanes,
                 hipLaunchKernelGGL(k_pp_rows<4>, dim3(nbr), dim3(BLK), 0, st, dv, b, cur),
                 hipLaunchKernelGGL(k_pp_rows<16>, dim3(nbr), dim3(BLK), 0, st, dv, b, cur),
                 hipLaunchKernelGGL(k_pp_rows<64>, dim3(nbr), dim3(BLK), 0, st, dv, b, cur));
    LANES_SWITCH(g.lanes,
                 hipLaunchKernelGGL(k_pp_cols<4>, dim3(nbc), dim3(BLK), 0, st, dv, b, cur),
                 hipLaunchKernelGGL(k_pp_cols<16>, dim3(nbc), dim3(BLK), 0, st, dv, b, cur),
                 hipLaunchKernelGGL(k_pp_cols<64>, dim3(nbc), dim3(BLK), 0, st, dv, b, cur));
}
void launch_prop_list(const DevView& dv, const PropBufs& b, const CutoffBufs& c, int cur, int* sums, hipStream_t st) {
    const long ntiles = cutoff_tiles(c.nv);
    if (ntiles <= 0) return;
    const int nb = (int)std::min<long>(ntiles, CB_MAX_BLOCKS);
    hipLaunchKernelGGL(k_pp_list, dim3(nb), dim3(BLK), 0, st, dv, b, c, cur);
    launch_exclusive_scan(c.tcnt, c.toff, ntiles, sums, st);
    hipLaunchKernelGGL(k_cb_gather, dim3(nb), dim3(BLK), 0, st, c);
}
