// fixing.inc — reduced-cost bounds from a cutoff, the batched fixing of variables and new bounds for them (include/minilp_hip.h:
// mlp_solution_cutoff_bounds, mlp_solution_fix_vars, mlp_solution_unfix_vars, mlp_solution_set_var_bounds; DESIGN.md §7.7, §7.8).
//
// The read (side-effect free like ranging.inc: only the private buffers of CutoffBufs are written):
//   k_cb_classify is ONE pass over the structural variables in tiles of BLK: location, flags, reduced cost, bounds (and, for a marked
//       column, its value) are loaded once, the bound g / |d_j| is formed, and the listed variables of the tile are compacted in place —
//       ballot and prefix count inside each wave, the wave counts summed in wave order — into the tile's own stretch of the staging
//       arrays, with the tile's count beside them;
//   launch_exclusive_scan turns the tile counts into offsets (its last sum is the length of the list);
//   k_cb_gather moves each tile's stretch to its offset.
// Tiles ascend, places inside a tile ascend: the list is in ascending variable number whatever the grid, and bit-identical from run to
// run.  No atomics.  Both kernels stride over the tiles with a tile index in long arithmetic: no number of variables is left out.
//
// The mutators (the non-basic requests of fix_vars and every request of set_var_bounds, DESIGN.md §7.8, all served together; the host
// sorts them by variable):
//   k_mv_classify ONE grid-stride pass over the requests.  It writes private buffers only.  New bounds (fix = 0): a BASIC column gets no
//                 target; a NON-BASIC column keeps its side — at lower: lo', at upper: hi', both flags (lo == hi, not fixed): lower if
//                 d_j >= 0, else upper, no flag: clamp(xN, lo', hi') — and the new flags come from the target against lo' / hi'; a column
//                 fixed by fix_var(s) keeps value and flags.  A fixing (fix = 1, lo == hi == the value asked for): the target is that
//                 value whatever the flags, the flags NB_AT_MIN | NB_AT_MAX | NB_FIXED.  Either way diff = target - xN.  Three integer
//                 counts (their order is immaterial): requests that shift, basic requests, and requests whose side has an infinite new
//                 bound (set_var_bounds then refuses);
//   k_fx_scatter  delta[var_i] = diff_i into a dense, zeroed delta[N] (the variables of a call are distinct: no two writes meet);
//   k_fx_rhs      r = A delta as a pull per CSR row in storage order — the sum of a row does not depend on the order of the list —
//                 into column 0 of the interleaved right-hand-side block of tableau.inc; launch_tab_solve then runs ONE FTRAN through
//                 the dense right-hand-side path of every representation of B^-1;
//   k_fx_apply    x_B -= B^-1 r;
//   k_mv_commit   one workgroup: obj += sum diff_i d_i over the requests in ascending variable number (thread t sums the requests t,
//                 t + BLK, ... and the partial sums meet in a fixed tree), then xN where it moved and the flags of the non-basic
//                 requests; new bounds are written for every request, by variable (var_lo / var_hi) and, for a basic one, by position
//                 (loB / hiB: the copies the pivots carry along); a fixing writes no bound;
//   k_fx_release  unfix_vars: the flags of a released column rebuilt from its value against the bounds.
// No float atomics; a request index is a long; no LDS beyond the reduction tree.

constexpr int CB_MAX_BLOCKS = 1024;  // workgroups of the two passes of the read (they stride over the tiles beyond that)

__global__ void __launch_bounds__(BLK) k_cb_classify(DevView v, CutoffBufs b) {
    __shared__ int s_w[BLK / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long ntiles = ((long)b.nv + BLK - 1) / BLK;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long j = tile * BLK + threadIdx.x;
        bool listed = false;
        double nlo = 0.0, nhi = 0.0;
        if (j < b.nv) {
            const int loc = v.var_loc[j];
            if (loc < 0) {
                const int col = -1 - loc;
                const int stt = nb_status_of(v.nbflags[col]);
                if (stt == 1 || stt == 2) {  // basic, free and fixed columns impose nothing
                    const double dj = v.d[col];
                    const double num = (stt == 1 ? fmax(dj, 0.0) : fmax(-dj, 0.0)) + 0.0;  // (the wrong sign clamped to 0: no entry)
                    if (num > 0.0) {
                        const double lo = v.var_lo[j], hi = v.var_hi[j];
                        double t = b.g / num;
                        if (b.mask && b.mask[j]) {
                            const double x = v.xN[col];
                            if (x == floor(x)) t = floor(t + 1e-9);
                        }
                        if (stt == 1) {
                            const double nh = fmax(lo + t, lo);
                            if (nh < hi) { listed = true; nlo = lo; nhi = nh; }
                        } else {
                            const double nl = fmin(hi - t, hi);
                            if (nl > lo) { listed = true; nlo = nl; nhi = hi; }
                        }
                    }
                }
            }
        }
        const unsigned long long bal = __ballot(listed);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_w[w] = __popcll(bal);
        __syncthreads();
        int base = 0, total = 0;
#pragma unroll
        for (int q = 0; q < BLK / 64; ++q) {
            const int c = s_w[q];
            if (q < w) base += c;
            total += c;
        }
        if (listed) {
            const size_t at = (size_t)tile * BLK + base + before;
            b.svar[at] = (uint32_t)j;
            b.slo[at] = nlo;
            b.shi[at] = nhi;
        }
        if (threadIdx.x == 0) b.tcnt[tile] = total;
        __syncthreads();  // (s_w is written again by the next tile)
    }
}
__global__ void __launch_bounds__(BLK) k_cb_gather(CutoffBufs b) {
    const long ntiles = ((long)b.nv + BLK - 1) / BLK;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if ((int)threadIdx.x < b.tcnt[tile]) {
            const size_t from = (size_t)tile * BLK + threadIdx.x, to = (size_t)b.toff[tile] + threadIdx.x;
            b.ovar[to] = b.svar[from];
            b.olo[to] = b.slo[from];
            b.ohi[to] = b.shi[from];
        }
    }
}
long cutoff_tiles(int nv) { return ((long)nv + BLK - 1) / BLK; }
void launch_cutoff_bounds(const DevView& dv, const CutoffBufs& b, int* sums, hipStream_t st) {
    const long ntiles = cutoff_tiles(b.nv);
    if (ntiles <= 0) return;
    const int nb = (int)std::min<long>(ntiles, CB_MAX_BLOCKS);
    hipLaunchKernelGGL(k_cb_classify, dim3(nb), dim3(BLK), 0, st, dv, b);
    launch_exclusive_scan(b.tcnt, b.toff, ntiles, sums, st);
    hipLaunchKernelGGL(k_cb_gather, dim3(nb), dim3(BLK), 0, st, b);
}

// ------------------------------------------------------------------- fix_vars / set_var_bounds / unfix_vars
__global__ void __launch_bounds__(BLK) k_mv_classify(DevView v, BoundBufs b, int fix) {
    const long step = (long)gridDim.x * BLK;
    for (long i = (long)blockIdx.x * BLK + threadIdx.x; i < b.n; i += step) {
        const int loc = v.var_loc[b.var[i]];
        double diff = 0.0, target = 0.0;
        uint8_t f = 0;
        if (loc >= 0) {
            atomicAdd(b.cnt + 1, 1);
        } else {
            const int col = -1 - loc;
            const double x = v.xN[col], lo = b.lo[i], hi = b.hi[i];
            f = v.nbflags[col];
            target = x;
            if (fix || !(f & NB_FIXED)) {
                if (fix) {
                    target = lo;  // (lo == hi: the value asked for; an already fixed column is moved)
                } else {
                    const bool at_min = (f & NB_AT_MIN) != 0, at_max = (f & NB_AT_MAX) != 0;
                    const int side = at_min && at_max ? (v.d[col] >= 0.0 ? 1 : 2) : (at_min ? 1 : (at_max ? 2 : 0));
                    if (side == 1) target = lo;
                    else if (side == 2) target = hi;
                    else target = fmin(fmax(x, lo), hi);
                    if (isinf(target)) {  // the bound on the column's side is infinite: the dual path cannot serve the request
                        atomicAdd(b.cnt + 2, 1);
                        target = x;
                    }
                }
                diff = target - x;
                f = fix ? (uint8_t)(NB_AT_MIN | NB_AT_MAX | NB_FIXED) : (uint8_t)((target == lo ? NB_AT_MIN : 0) | (target == hi ? NB_AT_MAX : 0));
                if (diff != 0.0) atomicAdd(b.cnt, 1);
            }
        }
        b.target[i] = target;
        b.diff[i] = diff;
        b.flags[i] = f;
    }
}
__global__ void __launch_bounds__(BLK) k_fx_scatter(BoundBufs b) {
    const long step = (long)gridDim.x * BLK;
    for (long i = (long)blockIdx.x * BLK + threadIdx.x; i < b.n; i += step) {
        const double diff = b.diff[i];
        if (diff != 0.0) b.delta[b.var[i]] = diff;
    }
}
template <int R>
__global__ void __launch_bounds__(BLK) k_fx_rhs(DevView v, BoundBufs b) {
    const long step = (long)gridDim.x * BLK;
    for (long row = (long)blockIdx.x * BLK + threadIdx.x; row < v.m; row += step) {
        const int end = v.csr_ptr[row + 1];
        double acc = 0.0;
        for (int e = v.csr_ptr[row]; e < end; ++e) acc += v.csr_val[e] * b.delta[v.csr_col[e]];
        b.X[(size_t)row * R] = acc;
    }
}
template <int R>
__global__ void __launch_bounds__(BLK) k_fx_apply(DevView v, BoundBufs b) {
    const long step = (long)gridDim.x * BLK;
    for (long p = (long)blockIdx.x * BLK + threadIdx.x; p < v.m; p += step) {
        const double y = b.Y[(size_t)p * R];
        if (y != 0.0) v.xB[p] -= y;
    }
}
__global__ void __launch_bounds__(BLK) k_mv_commit(DevView v, BoundBufs b, int fix, int shifted) {
    __shared__ double sh[BLK];
    if (shifted) {
        double s = 0.0;
        for (long i = threadIdx.x; i < b.n; i += BLK) {
            const double diff = b.diff[i];
            if (diff != 0.0) s += diff * v.d[-1 - v.var_loc[b.var[i]]];
        }
        sh[threadIdx.x] = s;
        __syncthreads();
        for (int o = BLK / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) v.ctl->it.obj += sh[0];
    }
    for (long i = threadIdx.x; i < b.n; i += BLK) {
        const int var = b.var[i], loc = v.var_loc[var];
        if (!fix) {
            const double lo = b.lo[i], hi = b.hi[i];
            b.var_lo[var] = lo;
            b.var_hi[var] = hi;
            if (loc >= 0) {
                v.loB[loc] = lo;
                v.hiB[loc] = hi;
            }
        }
        if (loc < 0) {
            const int col = -1 - loc;
            if (b.diff[i] != 0.0) v.xN[col] = b.target[i];
            v.nbflags[col] = b.flags[i];
        }
    }
}
__global__ void __launch_bounds__(BLK) k_fx_release(DevView v, BoundBufs b) {
    const long step = (long)gridDim.x * BLK;
    for (long i = (long)blockIdx.x * BLK + threadIdx.x; i < b.n; i += step) {
        const int var = b.var[i], col = -1 - v.var_loc[var];  // (the host lists non-basic columns only)
        const double cur = v.xN[col];
        v.nbflags[col] = (uint8_t)((cur == v.var_lo[var] ? NB_AT_MIN : 0) | (cur == v.var_hi[var] ? NB_AT_MAX : 0));
    }
}

void launch_move_classify(const DevView& dv, const BoundBufs& b, int fix, hipStream_t st) {
    (void)hipMemsetAsync(b.cnt, 0, 3 * sizeof(int), st);
    hipLaunchKernelGGL(k_mv_classify, dim3(tab_grid(b.n)), dim3(BLK), 0, st, dv, b, fix);
}
void launch_move_commit(const DevView& dv, const BoundBufs& b, int fix, int shifted, hipStream_t st) {
    hipLaunchKernelGGL(k_mv_commit, dim3(1), dim3(BLK), 0, st, dv, b, fix, shifted);
}
void launch_fix_rhs(const DevView& dv, const BoundBufs& b, int N, hipStream_t st) {
    constexpr int R = RG_BATCH;
    (void)hipMemsetAsync(b.delta, 0, sizeof(double) * (size_t)N, st);
    (void)hipMemsetAsync(b.X, 0, sizeof(double) * (size_t)dv.m * R, st);
    hipLaunchKernelGGL(k_fx_scatter, dim3(tab_grid(b.n)), dim3(BLK), 0, st, b);
    hipLaunchKernelGGL(k_fx_rhs<R>, dim3(tab_grid(dv.m)), dim3(BLK), 0, st, dv, b);
}
void launch_fix_apply(const DevView& dv, const BoundBufs& b, hipStream_t st) {
    hipLaunchKernelGGL(k_fx_apply<RG_BATCH>, dim3(tab_grid(dv.m)), dim3(BLK), 0, st, dv, b);
}
void launch_fix_release(const DevView& dv, const BoundBufs& b, hipStream_t st) {
    hipLaunchKernelGGL(k_fx_release, dim3(tab_grid(b.n)), dim3(BLK), 0, st, dv, b);
}
