// branch.inc — branching penalties of the current basis (include/minilp_hip.h: mlp_solution_branch_penalties; DESIGN.md §7.6): the
// objective change of the first dual-simplex pivot in the down branch and in the up branch of a basic fractional variable
// (Driebeek–Tomlin), the column that would enter, +inf when no column can.
//
// A dual ratio test on the tableau row of the candidate, RG_BATCH = 16 requests per pass over A, beside ranging.inc:
//   the 16 rows of B^-1 come from launch_ranging_block (every representation of B^-1 it serves) as ONE block rho[m][16];
//   k_bp_head forms f_dn = xB_p - floor(xB_p) and f_up = ceil(xB_p) - xB_p per request (one wave per batch, ONE launch for all the
//       batches of a call: nothing a batch writes is read by it);
//   k_bp_sweep is one pass over A's CSC: alpha = csc_block_dot (ranging.inc), then the classification of the column — status (nbflags),
//       reduced cost, value (xN) and integrality mark are loaded ONCE per column and shared by the 16 requests — and per request the
//       column's candidate (value, column) for the branch it is eligible in, reduced at once over the workgroup to the per-block
//       partials (a thread owns one column: no running minima are kept per lane);
//   k_bp_final reduces the partials the same way and writes the 4 x 16 numbers of the batch.
// The reduction is the exact lexicographic minimum of (value, column): the lowest column wins among exactly equal values, whatever the
// order of the tree.  No float atomics; alpha's sum has the fixed order of csc_block_dot.  So the numbers of a request are bit-identical
// alone, anywhere in any batch, and from run to run.  Side-effect free like ranging: only the private buffers of BranchBufs are written.

constexpr int BP_NOCOL = 0x7fffffff;  // column of an empty candidate set (reported as -1)

// (value, column) <- the lexicographic minimum with (v2, c2)
__device__ __forceinline__ void bp_take(double& v, int& c, double v2, int c2) {
    if (v2 < v || (v2 == v && c2 < c)) {
        v = v2;
        c = c2;
    }
}
// over the lanes 0, STEP, 2 STEP, ... of a wave (the others carry nothing); the result is on lane 0
template <int STEP>
__device__ __forceinline__ void bp_wave_min(double& v, int& c) {
#pragma unroll
    for (int o = 32; o >= STEP; o >>= 1) {
        const double v2 = __shfl_down(v, o, 64);
        const int c2 = __shfl_down(c, o, 64);
        bp_take(v, c, v2, c2);
    }
}

// workgroup q = batch q (one wave): req and f hold RG_BATCH requests / 2 RG_BATCH fractions per batch
template <int R>
__global__ void k_bp_head(DevView v, const int* __restrict__ req, double* __restrict__ f) {
    const int r = threadIdx.x;
    if (r >= R) return;
    const size_t at = (size_t)blockIdx.x * R + r;
    const int p = req[at];
    const double x = p >= 0 ? v.xB[p] : 0.0;
    f[2 * at] = x - floor(x);
    f[2 * at + 1] = ceil(x) - x;
}

// One pass over A's CSC for the whole batch (G lanes per column as k_rg_cost_sweep).  For a non-basic column i, with rho = |d_i| / |alpha_i|
// (d_i of the wrong sign clamped to 0, |alpha_i| <= EPS counts as zero):
//   at lower: alpha > 0 is eligible in the down branch, alpha < 0 in the up branch;   at upper: the mirror image;
//   non-basic at neither bound: eligible in both with ratio 0;   fixed: never eligible.
// Candidate f * rho, or max(f * rho, |d_i|) for a column marked integer that sits on a bound at an integral value (Tomlin).
// Partials: slot 2 r = down, 2 r + 1 = up of request r.
template <int R, int G>
__global__ void __launch_bounds__(BLK) k_bp_sweep(DevView v, RangingBufs b, BranchBufs bb) {
    __shared__ double sv[BLK / 64][2 * R];
    __shared__ int sc[BLK / 64][2 * R];
    const int var = (int)(((long)blockIdx.x * BLK + threadIdx.x) / G);
    const int gl = threadIdx.x & (G - 1);
    double acc[R];
    int loc = 0;
    if (var < b.N) loc = v.var_loc[var];
    const bool live = var < b.N && loc < 0;
    csc_block_dot<R, G>(v, b.blk, live, var, gl, acc);
    // the classification of the column, once for the 16 requests: 4 = takes no part (basic, fixed, a lane without a column)
    int stt = 4;
    double num = 0.0;
    bool strong = false;
    if (live && gl == 0) {
        stt = nb_status_of(v.nbflags[-1 - loc]);
        if (stt == 1 || stt == 2) {
            const double ri = b.r[var];
            num = (stt == 1 ? fmax(ri, 0.0) : fmax(-ri, 0.0)) + 0.0;
            if (bb.mask && bb.mask[var]) {
                const double xn = v.xN[-1 - loc];
                strong = xn == floor(xn);
            }
        }
    }
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        double vd = RG_INF, vu = RG_INF;
        int cd = BP_NOCOL, cu = BP_NOCOL;
        const double a = acc[r];
        if (stt != 4 && fabs(a) > EPS) {
            if (stt == 3) {
                vd = 0.0; cd = var;
                vu = 0.0; cu = var;
            } else {
                const double rho = num / fabs(a);
                const bool down = (stt == 1) == (a > 0.0);
                double t = bb.f[2 * r + (down ? 0 : 1)] * rho;
                if (strong) t = fmax(t, num);
                if (down) { vd = t; cd = var; }
                else { vu = t; cu = var; }
            }
        }
        bp_wave_min<G>(vd, cd);
        bp_wave_min<G>(vu, cu);
        if (l == 0) {
            sv[w][2 * r] = vd; sc[w][2 * r] = cd;
            sv[w][2 * r + 1] = vu; sc[w][2 * r + 1] = cu;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * R) {
        double x = sv[0][threadIdx.x];
        int c = sc[0][threadIdx.x];
        for (int q = 1; q < BLK / 64; ++q) bp_take(x, c, sv[q][threadIdx.x], sc[q][threadIdx.x]);
        bb.pval[(size_t)blockIdx.x * 2 * R + threadIdx.x] = x;
        bb.pcol[(size_t)blockIdx.x * 2 * R + threadIdx.x] = c;
    }
}
// one workgroup of BP_FINAL threads: the per-block partials -> oval[2 R], ocol[2 R].  Thread t takes slot t % 2R of the blocks t / 2R,
// + BP_FINAL / 2R, ... (a row of partials is read by 2R neighbouring threads; the loads of four rows are in flight together: the loop is
// a chain of load latencies otherwise), then the stripes meet in LDS.
constexpr int BP_FINAL = 1024;
template <int R>
__global__ void __launch_bounds__(BP_FINAL) k_bp_final(BranchBufs bb, int nb) {
    constexpr int S = BP_FINAL / (2 * R);
    __shared__ double sv[S][2 * R];
    __shared__ int sc[S][2 * R];
    const int slot = threadIdx.x % (2 * R), stripe = threadIdx.x / (2 * R);
    double x = RG_INF;
    int c = BP_NOCOL;
#pragma unroll 4
    for (int t = stripe; t < nb; t += S) bp_take(x, c, bb.pval[(size_t)t * 2 * R + slot], bb.pcol[(size_t)t * 2 * R + slot]);
    sv[stripe][slot] = x;
    sc[stripe][slot] = c;
    __syncthreads();
    if (stripe == 0) {
        for (int q = 1; q < S; ++q) bp_take(x, c, sv[q][slot], sc[q][slot]);
        bb.oval[slot] = x;
        bb.ocol[slot] = x == RG_INF ? -1 : c;
    }
}

// the fractions of all nbat batches of a call (req: their requests, -1 at the empty places)
void launch_branch_heads(const DevView& dv, const int* req, double* f, int nbat, hipStream_t st) {
    hipLaunchKernelGGL(k_bp_head<RG_BATCH>, dim3(nbat), dim3(64), 0, st, dv, req, f);
}
// one batch of at most RG_BATCH basic fractional requests (b.req, bb.f, bb.oval / bb.ocol already point at the batch)
void launch_branch_batch(const DevView& dv, const Geom& g, const RangingBufs& b, const BranchBufs& bb, int nreq, const int* h_req,
                         hipStream_t st) {
    constexpr int R = RG_BATCH;
    launch_ranging_block(dv, g, b, 0, nreq, h_req, st);
    const int nb = ranging_blocks(g, 0, b.N);
    LANES_SWITCH(g.lanes,
                 hipLaunchKernelGGL((k_bp_sweep<R, 4>), dim3(nb), dim3(BLK), 0, st, dv, b, bb),
                 hipLaunchKernelGGL((k_bp_sweep<R, 16>), dim3(nb), dim3(BLK), 0, st, dv, b, bb),
                 hipLaunchKernelGGL((k_bp_sweep<R, 64>), dim3(nb), dim3(BLK), 0, st, dv, b, bb));
    hipLaunchKernelGGL(k_bp_final<R>, dim3(1), dim3(BP_FINAL), 0, st, bb, nb);
}
