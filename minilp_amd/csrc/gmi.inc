// gmi.inc — a round of Gomory mixed-integer cuts in one call (include/minilp_hip.h: mlp_solution_add_gmi_cuts; DESIGN.md §7.5).
//
// Generation beside cuts.inc, RG_BATCH = 16 requests per pass over A:
//   the 16 rows of B^-1 come from launch_ranging_block (every representation of B^-1 it serves) as ONE block rho[m][16];
//   k_gmi_head forms f0 = xB_p - floor(xB_p) per request and the fraction test min(f0, 1 - f0) < away;
//   k_gmi_sweep is the pass of k_cut_sweep over A's CSC with the classification of the column applied at its end: status (nbflags),
//       value (xN) and integrality mark are loaded ONCE per column and shared by the 16 requests; it writes the stored coefficients
//       c[N][16] BY VARIABLE (basic, fixed, skipped: 0) and, for a free column with |alpha| > EPS, the request's free flag (a plain
//       store of the constant 1: every writer stores the same value);
//   k_gmi_clear zeroes the block column of a request that met a free column (a skipped request contributes no term and nothing to the
//       edge norms); k_gmi_count is the count pass of cuts.inc with the partial right-hand sides sum c_j xN_j per (segment, request),
//       in variable order; the scan and the ordered fill are those of cuts.inc; k_gmi_heads sums the partials of a request in a fixed
//       order (thread t takes segments t, t + BLK, ... in order, then a fixed tree in LDS) and writes row length, rhs and status.
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
    const int var = (blockIdx.x * BLK + threadIdx.x) / G;
    const int gl = threadIdx.x & (G - 1);
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
    int loc = 0;
    if (var < b.N) loc = v.var_loc[var];
    const bool live = var < b.N && loc < 0;
    if (live) {
        const int end = v.csc_ptr[var + 1];
        for (int e = v.csc_ptr[var] + gl; e < end; e += G) {
            const double a = v.csc_val[e];
            const double2* rr = reinterpret_cast<const double2*>(b.blk + (size_t)v.csc_row[e] * R);
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
    if (var < b.N && gl == 0) {
        // the classification of the column, once for the 16 requests: 4 fixed (no term), 1 at lower, 2 at upper, 3 free
        int stt = 4;
        bool isint = false;
        if (live) {
            stt = rg_nb_status(v.nbflags[-1 - loc]);
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
        double2* out = reinterpret_cast<double2*>(cd + (size_t)var * R);
#pragma unroll
        for (int r = 0; r < R; r += 2) {
            double2 t;
            t.x = acc[r];
            t.y = acc[r + 1];
            out[r >> 1] = t;
        }
    }
}
// a request that met a free column has no cut: its block column is cleared before the count and the edge norms
template <int R>
__global__ void __launch_bounds__(BLK) k_gmi_clear(GmiBufs gb, int N, double* __restrict__ cd) {
    const long i = (long)blockIdx.x * BLK + threadIdx.x;
    if (i >= (long)N * R) return;
    if (gb.freef[i % R]) cd[i] = 0.0;
}
// the count pass of k_cut_compact (thread = (segment, request), variable order) with the segment's share of sum c_j xN_j
template <int R>
__global__ void __launch_bounds__(BLK) k_gmi_count(DevView v, GmiBufs gb, const double* __restrict__ cd, int N, int nseg,
                                                   int* __restrict__ cnt) {
    const long gid = (long)blockIdx.x * BLK + threadIdx.x;
    const int r = (int)(gid % R);
    const long seg = gid / R;
    if (seg >= nseg) return;
    const int v0 = (int)seg * CUT_SEG, v1 = min(N, v0 + CUT_SEG);
    int pos = 0;
    double s = 0.0;
    for (int j = v0; j < v1; ++j) {
        const double c = cd[(size_t)j * R + r];
        if (c != 0.0) {  // (only a non-basic column holds a non-zero)
            s += c * v.xN[-1 - v.var_loc[j]];
            ++pos;
        }
    }
    cnt[(size_t)r * nseg + seg] = pos;
    gb.part[(size_t)r * nseg + seg] = s;
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

// phase 1 of a batch (the buffers of launch_cut_generate, cd: [N][RG_BATCH]); phase 2 is launch_cut_fill on cd
void launch_gmi_generate(const DevView& dv, const Geom& g, const RangingBufs& b, const GmiBufs& gb, int nreq, const int* h_req,
                         double* cd, int* cnt, int* off, int* sums, int* len, double* rhs, hipStream_t st) {
    constexpr int R = RG_BATCH;
    launch_ranging_block(dv, g, b, 0, nreq, h_req, st);
    hipLaunchKernelGGL(k_gmi_head<R>, dim3(1), dim3(64), 0, st, dv, b.req, gb);
    const int nb = ranging_blocks(g, 0, b.N);
    LANES_SWITCH(g.lanes,
                 hipLaunchKernelGGL((k_gmi_sweep<R, 4>), dim3(nb), dim3(BLK), 0, st, dv, b, gb, cd),
                 hipLaunchKernelGGL((k_gmi_sweep<R, 16>), dim3(nb), dim3(BLK), 0, st, dv, b, gb, cd),
                 hipLaunchKernelGGL((k_gmi_sweep<R, 64>), dim3(nb), dim3(BLK), 0, st, dv, b, gb, cd));
    hipLaunchKernelGGL(k_gmi_clear<R>, dim3(blocks_for((long)b.N * R)), dim3(BLK), 0, st, gb, b.N, cd);
    const int nseg = cut_segments(b.N);
    const long n = (long)R * nseg;
    hipLaunchKernelGGL(k_gmi_count<R>, dim3(blocks_for(n)), dim3(BLK), 0, st, dv, gb, cd, b.N, nseg, cnt);
    launch_exclusive_scan(cnt, off, n, sums, st);
    hipLaunchKernelGGL(k_gmi_heads<R>, dim3(R), dim3(BLK), 0, st, gb, off, sums + (n + SCAN_TILE - 1) / SCAN_TILE, nseg, len, rhs);
}
