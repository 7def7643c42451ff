// gmi.inc — a round of Gomory mixed-integer cuts in one call (include/minilp_hip.h: mlp_solution_add_gmi_cuts; DESIGN.md §7.5).
//
// Generation beside cuts.inc, RG_BATCH = 16 requests per pass over A:
//   the 16 rows of B^-1 come from launch_ranging_block (every representation of B^-1 it serves) as ONE block rho[m][16];
//   k_gmi_head forms f0 = xB_p - floor(xB_p) per request and the fraction test min(f0, 1 - f0) < away;
//   k_gmi_sweep is one pass over A's CSC: alpha = csc_block_dot (ranging.inc), then the classification of the column: status (nbflags),
//       value (xN) and integrality mark are loaded ONCE per column and shared by the 16 requests; it writes the stored coefficients
//       c[N][16] BY VARIABLE (basic, fixed, skipped: 0) and, for a free column with |alpha| > EPS, the request's free flag (a plain
//       store of the constant 1: every writer stores the same value);
//   k_gmi_clear zeroes the block column of a request that met a free column (a skipped request contributes no term and nothing to the
//       edge norms); the count pass is k_cut_compact in its MODE 2, which also leaves the partial right-hand sides sum c_j xN_j per
//       (segment, request), in variable order; the scan and the ordered fill are those of cuts.inc; k_gmi_heads sums the partials of a
//       request in a fixed order (thread t takes segments t, t + BLK, ... in order, then a fixed tree in LDS) and writes row length,
//       rhs and status.
// No float atomics, no ballots; every sum has an order that depends on the request alone, so a row, its rhs and its status are
// bit-identical from run to run and whatever else the call holds.  Side-effect free like ranging: only the private buffers are written
// (the edge norms are fed by launch_cut_fill, as for the Gomory round).

template <int R>
__global__ void k_gmi_head(DevView v, const int* __restrict__ req, GmiBufs gb) {
    const int r = threadIdx.x;
    if (r >= R) return;
    const int p = req[r];
    const double x = p >= 0 ? v.xB[p] : 0.0;
    const double f0 = x - floor(x);
    gb.f0[r] = f0;
    gb.skip[r] = (p < 0 || fmin(f0, 1.0 - f0) < gb.away) ? 1 : 0;
    gb.freef[r] = 0;
}

template <int R, int G>
__global__ void __launch_bounds__(BLK) k_gmi_sweep(DevView v, RangingBufs b, GmiBufs gb, double* __restrict__ cd) {
    const int var = (int)(((long)blockIdx.x * BLK + threadIdx.x) / G);
    const int gl = threadIdx.x & (G - 1);
    double acc[R];
    int loc = 0;
    if (var < b.N) loc = v.var_loc[var];
    const bool live = var < b.N && loc < 0;
    csc_block_dot<R, G>(v, b.blk, live, var, gl, acc);
    if (var < b.N && gl == 0) {
        // the classification of the column, once for the 16 requests: 4 fixed (no term), 1 at lower, 2 at upper, 3 free
        int stt = 4;
        bool isint = false;
        if (live) {
            stt = nb_status_of(v.nbflags[-1 - loc]);
            const double xn = v.xN[-1 - loc];
            isint = gb.mask[var] != 0 && xn == floor(xn);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double c = 0.0;
            if (stt != 4 && !gb.skip[r]) {
                const double a = acc[r];
                if (stt == 3) {
                    if (fabs(a) > EPS) gb.freef[r] = 1;
                } else {
                    const double f0 = gb.f0[r];
                    const double ab = stt == 1 ? a : -a;
                    double g;
                    if (isint) {
                        const double f = ab - floor(ab);
                        g = f <= f0 ? f / f0 : (1.0 - f) / (1.0 - f0);
                    } else {
                        g = ab >= 0.0 ? ab / f0 : -ab / (1.0 - f0);
                    }
                    c = stt == 1 ? -g : g;
                }
            }
            acc[r] = c;
        }
        store_block_row<R>(cd + (size_t)var * R, acc);
    }
}
// a request that met a free column has no cut: its block column is cleared before the count and the edge norms
template <int R>
__global__ void __launch_bounds__(BLK) k_gmi_clear(GmiBufs gb, int N, double* __restrict__ cd) {
    const long i = (long)blockIdx.x * BLK + threadIdx.x;
    if (i >= (long)N * R) return;
    if (gb.freef[i % R]) cd[i] = 0.0;
}
// workgroup r = request r: rhs = -1 + sum c_j xN_j (partials in a fixed order), row length from the scanned offsets, status
template <int R>
__global__ void __launch_bounds__(BLK) k_gmi_heads(GmiBufs gb, const int* __restrict__ off, const int* __restrict__ total, int nseg,
                                                   int* __restrict__ len, double* __restrict__ rhs) {
    __shared__ double sh[BLK];
    const int r = blockIdx.x;
    double s = 0.0;
    for (int t = threadIdx.x; t < nseg; t += BLK) s += gb.part[(size_t)r * nseg + t];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = BLK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int b = off[(size_t)r * nseg];
        const int e = r + 1 < R ? off[(size_t)(r + 1) * nseg] : *total;
        len[r] = e - b;
        rhs[r] = -1.0 + sh[0];
        gb.status[r] = gb.skip[r] ? 1 : gb.freef[r] ? 2 : 0;
    }
}
// (phase 1 of a batch is launch_rows_generate with ROWS_GMI, tableau.inc; phase 2 is launch_cut_fill on cd)
