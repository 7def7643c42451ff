// rhs.inc — new right-hand sides for a solved model and the batched what-if read (include/minilp_hip.h: mlp_solution_set_rhs,
// mlp_solution_rhs_scenarios; DESIGN.md §7.10).
//
// Both calls are x_B + B^-1 (b' - b): the changes of up to R = RG_BATCH right-hand sides go into the zeroed interleaved block X[m][R]
// of tableau.inc, launch_tab_solve runs ONE batch of FTRANs through the dense right-hand-side path of whichever representation of B^-1
// is live, and one scan over the positions reads the result.
//   k_rh_scatter  column r of X gets val[(s0 + r) * n + i] - cur[i] at row[i], straight from the list as the caller gave it (set_rhs:
//                 one column, val holds the changes, cur is absent).  The rows of a call are distinct: no two writes meet, and the block
//                 does not depend on the order of the list;
//   k_rh_scan     thread (g, r) of a workgroup walks the positions g, g + BLK / R, ... of the workgroup's stride for right-hand side r:
//                 sum += c_B[p] y[p], and the largest violation of x_B[p] + y[p] against [loB - EPS, hiB + EPS] — the predicate of
//                 price_dual_one — with its position, the lowest on a tie.  The BLK / R threads of a right-hand side meet in a fixed tree.
//                 apply (set_rhs): x_B[p] = x_B[p] + y[p] as well;
//   k_rh_finish   one workgroup: thread (g, r) takes the partials of the workgroups g, g + BLK / R, ... of right-hand side r, then the same
//                 tree; apply: the sum of column 0 is added to the device-held objective.
// The grid of the scan depends on m alone, a right-hand side's walk and tree are the same in every column: its numbers are bit-identical
// from run to run and whatever its column, its neighbours or the length of the call.  The maximum is exact, so its order is immaterial.
// set_rhs is this scan with nreq = 1: the threads with r > 0, 15 of every 16, idle and the line of Y is still fetched 16 wide; only
// r == 0 stores x_B, so nothing races.  That is the price of one scan for both calls (about 0.17 ms per call at m = 6000, DESIGN.md §7.10).
// No float atomics; a position is a long; every kernel strides, so no m is left out.

constexpr int RH_MAX_BLOCKS = 1024;  // workgroups of the scan (they stride over the positions beyond that)
constexpr int RH_NONE = 0x7fffffff;  // position of "no violation"

int rhs_blocks(int m) { return std::min(tab_grid((long)m * RG_BATCH), RH_MAX_BLOCKS); }

template <int R>
__global__ void __launch_bounds__(BLK) k_rh_scatter(RhsBufs b, long s0, int nreq) {
    const long total = (long)nreq * b.n, step = (long)gridDim.x * BLK;
    for (long i = (long)blockIdx.x * BLK + threadIdx.x; i < total; i += step) {
        const long r = i / b.n, c = i - r * b.n;
        double d = b.val[(s0 + r) * b.n + c];
        if (b.cur) d -= b.cur[c];
        b.X[(size_t)b.row[c] * R + r] = d;
    }
}
// (violation, position): the larger violation, the lower position on a tie
__device__ __forceinline__ void rh_worse(double& viol, int& pos, double oviol, int opos) {
    if (oviol > viol || (oviol == viol && opos < pos)) {
        viol = oviol;
        pos = opos;
    }
}
// the BLK / R threads of a right-hand side meet in the fixed tree both kernels share
template <int R>
__device__ __forceinline__ void rh_tree(double* s_sum, double* s_viol, int* s_pos, double sum, double viol, int pos) {
    s_sum[threadIdx.x] = sum;
    s_viol[threadIdx.x] = viol;
    s_pos[threadIdx.x] = pos;
    __syncthreads();
    for (int o = BLK / 2; o >= R; o >>= 1) {  // (o is a multiple of R: a right-hand side meets itself only)
        if ((int)threadIdx.x < o) {
            s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
            rh_worse(s_viol[threadIdx.x], s_pos[threadIdx.x], s_viol[threadIdx.x + o], s_pos[threadIdx.x + o]);
        }
        __syncthreads();
    }
}
template <int R>
__global__ void __launch_bounds__(BLK) k_rh_scan(DevView v, RhsBufs b, int nreq, int apply) {
    __shared__ double s_sum[BLK];
    __shared__ double s_viol[BLK];
    __shared__ int s_pos[BLK];
    constexpr int PG = BLK / R;  // positions a workgroup visits per step
    const int r = threadIdx.x % R, g = threadIdx.x / R;
    const long step = (long)gridDim.x * PG;
    double sum = 0.0, viol = 0.0;
    int pos = RH_NONE;
    if (r < nreq) {
        for (long p = (long)blockIdx.x * PG + g; p < v.m; p += step) {
            const double y = b.Y[(size_t)p * R + r];
            sum += v.obj_c[v.basic_vars[p]] * y;
            const double val = v.xB[p] + y, lo = v.loB[p], hi = v.hiB[p];
            double infeas = 0.0;
            if (val < lo - EPS) infeas = lo - val;
            else if (val > hi + EPS) infeas = val - hi;
            if (infeas > 0.0) rh_worse(viol, pos, infeas, (int)p);
            if (apply) v.xB[p] = val;
        }
    }
    rh_tree<R>(s_sum, s_viol, s_pos, sum, viol, pos);
    if ((int)threadIdx.x < R) {
        const size_t at = (size_t)blockIdx.x * R + threadIdx.x;
        b.psum[at] = s_sum[threadIdx.x];
        b.pviol[at] = s_viol[threadIdx.x];
        b.ppos[at] = s_pos[threadIdx.x];
    }
}
template <int R>
__global__ void __launch_bounds__(BLK) k_rh_finish(DevView v, RhsBufs b, int nblk, int apply) {
    __shared__ double s_sum[BLK];
    __shared__ double s_viol[BLK];
    __shared__ int s_pos[BLK];
    const int r = threadIdx.x % R, g = threadIdx.x / R;
    double sum = 0.0, viol = 0.0;
    int pos = RH_NONE;
    for (long q = g; q < nblk; q += BLK / R) {  // thread (g, r): the workgroups g, g + BLK / R, ... of right-hand side r
        const size_t at = (size_t)q * R + r;
        sum += b.psum[at];
        rh_worse(viol, pos, b.pviol[at], b.ppos[at]);
    }
    rh_tree<R>(s_sum, s_viol, s_pos, sum, viol, pos);
    if ((int)threadIdx.x < R) {
        b.osum[r] = s_sum[r];
        b.oviol[r] = s_viol[r];
        b.opos[r] = s_pos[r] == RH_NONE ? -1 : s_pos[r];
        if (apply && r == 0) v.ctl->it.obj += s_sum[0];
    }
}

void launch_rhs_scatter(const DevView& dv, const RhsBufs& b, long s0, int nreq, hipStream_t st) {
    constexpr int R = RG_BATCH;
    (void)hipMemsetAsync(b.X, 0, sizeof(double) * (size_t)dv.m * R, st);
    if (nreq > 0 && b.n > 0) hipLaunchKernelGGL(k_rh_scatter<R>, dim3(tab_grid((long)nreq * b.n)), dim3(BLK), 0, st, b, s0, nreq);
}
void launch_rhs_scan(const DevView& dv, const RhsBufs& b, int nreq, int apply, hipStream_t st) {
    constexpr int R = RG_BATCH;
    const int nblk = rhs_blocks(dv.m);
    hipLaunchKernelGGL(k_rh_scan<R>, dim3(nblk), dim3(BLK), 0, st, dv, b, nreq, apply);
    hipLaunchKernelGGL(k_rh_finish<R>, dim3(1), dim3(BLK), 0, st, dv, b, nblk, apply);
}
