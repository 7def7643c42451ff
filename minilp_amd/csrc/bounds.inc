// bounds.inc — new bounds for structural variables of a solved model (include/minilp_hip.h: mlp_solution_set_var_bounds,
// mlp_solution_tighten_by_reduced_cost; DESIGN.md §7.8).  The generalisation of the non-basic path of fix_vars (fixing.inc): the shift
// r = A delta, the FTRAN and x_B -= B^-1 r are the kernels of fixing.inc as they are (k_fx_scatter, k_fx_rhs, k_fx_apply); what is new is
//   k_sb_classify    ONE grid-stride pass over the requests (ascending variable number, the host sorts them).  It writes private buffers
//                    only: a BASIC column gets no target; a NON-BASIC column keeps its side — at lower: lo', at upper: hi', both flags
//                    (lo == hi, not fixed): lower if d_j >= 0, else upper, no flag: clamp(xN, lo', hi') — and diff = target - xN, the new
//                    flags from the target against lo' / hi'.  A column fixed by fix_var(s) keeps value and flags.  Three integer counts:
//                    requests that shift, basic requests, and requests whose side has an infinite new bound (the call then refuses);
//   k_sb_commit      one workgroup: obj += sum diff_i d_i over the requests in ascending variable number with the fixed tree of
//                    k_fx_commit, then xN and the flags of the non-basic requests and the bounds of all, by variable (var_lo / var_hi) and,
//                    for a basic request, by position (loB / hiB: the copies the pivots carry along);
//   k_sb_apply_list  the device-to-device variant: the list k_cb_gather left in CutoffBufs (its length is read on the device) is written to
//                    the bounds.  A listed column is non-basic at the bound that does not move: no value, no flag changes.
// No float atomics (the counts are integers: their order is immaterial); a request index is a long; no LDS beyond the reduction tree.

__global__ void __launch_bounds__(BLK) k_sb_classify(DevView v, BoundBufs b) {
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
            if (!(f & NB_FIXED)) {
                const bool at_min = (f & NB_AT_MIN) != 0, at_max = (f & NB_AT_MAX) != 0;
                const int side = at_min && at_max ? (v.d[col] >= 0.0 ? 1 : 2) : (at_min ? 1 : (at_max ? 2 : 0));
                if (side == 1) target = lo;
                else if (side == 2) target = hi;
                else target = fmin(fmax(x, lo), hi);
                if (isinf(target)) {  // the bound on the column's side is infinite: the dual path cannot serve the request
                    atomicAdd(b.cnt + 2, 1);
                    target = x;
                }
                diff = target - x;
                f = (uint8_t)((target == lo ? NB_AT_MIN : 0) | (target == hi ? NB_AT_MAX : 0));
                if (diff != 0.0) atomicAdd(b.cnt, 1);
            }
        }
        b.target[i] = target;
        b.diff[i] = diff;
        b.flags[i] = f;
    }
}
__global__ void __launch_bounds__(BLK) k_sb_commit(DevView v, BoundBufs b, int shifted) {
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
        const double lo = b.lo[i], hi = b.hi[i];
        b.var_lo[var] = lo;
        b.var_hi[var] = hi;
        if (loc >= 0) {
            v.loB[loc] = lo;
            v.hiB[loc] = hi;
        } else {
            const int col = -1 - loc;
            if (b.diff[i] != 0.0) v.xN[col] = b.target[i];
            v.nbflags[col] = b.flags[i];
        }
    }
}
__global__ void __launch_bounds__(BLK) k_sb_apply_list(DevView v, CutoffBufs c, const int* __restrict__ count, double* __restrict__ var_lo,
                                                       double* __restrict__ var_hi) {
    const long n = *count, step = (long)gridDim.x * BLK;
    for (long i = (long)blockIdx.x * BLK + threadIdx.x; i < n; i += step) {
        const uint32_t var = c.ovar[i];
        const double lo = c.olo[i], hi = c.ohi[i];
        var_lo[var] = lo;
        var_hi[var] = hi;
        const int loc = v.var_loc[var];
        if (loc >= 0) {  // (k_cb_classify lists non-basic columns only; the copy by position is kept true whatever the list)
            v.loB[loc] = lo;
            v.hiB[loc] = hi;
        }
    }
}

void launch_bounds_classify(const DevView& dv, const BoundBufs& b, hipStream_t st) {
    (void)hipMemsetAsync(b.cnt, 0, 3 * sizeof(int), st);
    hipLaunchKernelGGL(k_sb_classify, dim3(tab_grid(b.n)), dim3(BLK), 0, st, dv, b);
}
void launch_bounds_commit(const DevView& dv, const BoundBufs& b, int shifted, hipStream_t st) {
    hipLaunchKernelGGL(k_sb_commit, dim3(1), dim3(BLK), 0, st, dv, b, shifted);
}
void launch_bounds_apply_list(const DevView& dv, const CutoffBufs& c, const int* count, double* var_lo, double* var_hi, hipStream_t st) {
    const int nb = (int)std::min<long>(std::max<long>(cutoff_tiles(c.nv), 1), CB_MAX_BLOCKS);
    hipLaunchKernelGGL(k_sb_apply_list, dim3(nb), dim3(BLK), 0, st, dv, c, count, var_lo, var_hi);
}
