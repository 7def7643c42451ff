// bounds.inc — the device-to-device variant of new bounds (include/minilp_hip.h: mlp_solution_tighten_by_reduced_cost; DESIGN.md §7.8).
// set_var_bounds itself runs on the kernels of fixing.inc.
//   k_sb_apply_list  the list k_cb_gather left in CutoffBufs (its length is read on the device) is written to the bounds.  A listed
//                    column is non-basic at the bound that does not move: no value, no flag changes.  A request index is a long; no LDS.

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

void launch_bounds_apply_list(const DevView& dv, const CutoffBufs& c, const int* count, double* var_lo, double* var_hi, hipStream_t st) {
    const int nb = (int)std::min<long>(std::max<long>(cutoff_tiles(c.nv), 1), CB_MAX_BLOCKS);
    hipLaunchKernelGGL(k_sb_apply_list, dim3(nb), dim3(BLK), 0, st, dv, c, count, var_lo, var_hi);
}
