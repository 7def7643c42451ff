// cuts.inc — a round of cuts in one call (include/minilp_hip.h: mlp_solution_add_gomory_cuts, mlp_solution_add_constraints_csr;
// DESIGN.md §7.3).
//
// Cut generation, RG_BATCH = 16 Gomory cuts per pass over A:
//   the 16 rows of B^-1 come from launch_ranging_block (ranging.inc: explicit inverse with its pending terms applied, singleton
//   positions, compact factor) as ONE block rho[m][16]; k_cut_sweep is the pass of k_rg_cost_sweep over A's CSC with
//   f = floor(alpha) - alpha at its end instead of a ratio test, written as a dense block f[N][16] BY VARIABLE (basic variables: 0);
//   then the non-zero f become sparse rows on the device: a count pass (per segment of CUT_SEG variables and request), an exclusive
//   scan in request-major order, and an ordered fill.  A thread owns one (segment, request) pair in both passes and walks its
//   segment in variable order, so every cut comes out sorted by variable with no atomics, no ballots and no LDS, bit-identically
//   from run to run and whatever else the batch holds (alpha_j[r] is summed in storage order, then by the xor tree of the lane
//   group: its value depends on request r alone).  Side-effect free like ranging: only the private buffers are written.
// Row append (R = 1 is Solution::add_constraint): one re-layout of the CSC for R new rows (they are the last R rows, so every column
//   gains its new entries at its end, in row order): per-column counts from the R sorted rows, a scan, one copy kernel.

constexpr int CUT_SEG = 16;  // variables per (segment, request) thread of the count / fill passes

template <int R, int G>
__global__ void __launch_bounds__(BLK) k_cut_sweep(DevView v, RangingBufs b, double* __restrict__ fd) {
    const int var = (blockIdx.x * BLK + threadIdx.x) / G;
    const int gl = threadIdx.x & (G - 1);
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
    const bool live = var < b.N && v.var_loc[var] < 0;
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
        double2* out = reinterpret_cast<double2*>(fd + (size_t)var * R);
#pragma unroll
        for (int r = 0; r < R; r += 2) {
            double2 t;
            t.x = live ? floor(acc[r]) - acc[r] : 0.0;
            t.y = live ? floor(acc[r + 1]) - acc[r + 1] : 0.0;
            out[r >> 1] = t;
        }
    }
}
// count / fill: thread (segment, request); MODE 0 counts the non-zero f of its segment, MODE 1 writes them behind off[r * nseg + seg]
template <int R, int MODE>
__global__ void __launch_bounds__(BLK) k_cut_compact(const double* __restrict__ fd, int N, int nseg, int* __restrict__ cnt,
                                                     const int* __restrict__ off, int* __restrict__ ocol, double* __restrict__ oval) {
    const long gid = (long)blockIdx.x * BLK + threadIdx.x;
    const int r = (int)(gid % R);
    const long seg = gid / R;
    if (seg >= nseg) return;
    const int v0 = (int)seg * CUT_SEG, v1 = min(N, v0 + CUT_SEG);
    int pos = MODE ? off[(size_t)r * nseg + seg] : 0;
    for (int j = v0; j < v1; ++j) {
        const double f = fd[(size_t)j * R + r];
        if (f != 0.0) {  // exact zeros carry no information
            if (MODE) {
                ocol[pos] = j;
                oval[pos] = f;
            }
            ++pos;
        }
    }
    if (!MODE) cnt[(size_t)r * nseg + seg] = pos;
}
// row lengths and right-hand sides of the batch: len[r] from the scanned offsets, rhs[r] = floor(xB_p) - xB_p
template <int R>
__global__ void k_cut_heads(DevView v, const int* __restrict__ req, const int* __restrict__ off, const int* __restrict__ total,
                            int nseg, int* __restrict__ len, double* __restrict__ rhs) {
    const int r = threadIdx.x;
    if (r >= R) return;
    const int b = off[(size_t)r * nseg];
    const int e = r + 1 < R ? off[(size_t)(r + 1) * nseg] : *total;
    len[r] = e - b;
    const int p = req[r];
    const double x = p >= 0 ? v.xB[p] : 0.0;
    rhs[r] = floor(x) - x;
}
// steepest-edge norms: the tableau row of a Gomory cut in the extended basis IS its coefficient row, so gamma_j += f_j[r]^2 for
// the requests of the batch in their order (what k_gamma_add_row adds cut by cut)
template <int R>
__global__ void __launch_bounds__(BLK) k_cut_gamma(DevView v, const double* __restrict__ fd, int N) {
    const int var = blockIdx.x * BLK + threadIdx.x;
    if (var >= N) return;
    const int loc = v.var_loc[var];
    if (loc >= 0) return;
    double g = v.gamma[-1 - loc];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double f = fd[(size_t)var * R + r];
        g += f * f;
    }
    v.gamma[-1 - loc] = g;
}

int cut_segments(int N) { return (N + CUT_SEG - 1) / CUT_SEG; }

// phase 1 of a batch: block of rows, sweep, count, scan, heads.  cnt / off: RG_BATCH * cut_segments(N) ints each, sums: the scan's
// scratch (its last element is the total), len / rhs: RG_BATCH each.
void launch_cut_generate(const DevView& dv, const Geom& g, const RangingBufs& b, int nreq, const int* h_req, double* fd, int* cnt,
                         int* off, int* sums, int* len, double* rhs, hipStream_t st) {
    constexpr int R = RG_BATCH;
    launch_ranging_block(dv, g, b, 0, nreq, h_req, st);
    const int nb = ranging_blocks(g, 0, b.N);
    LANES_SWITCH(g.lanes,
                 hipLaunchKernelGGL((k_cut_sweep<R, 4>), dim3(nb), dim3(BLK), 0, st, dv, b, fd),
                 hipLaunchKernelGGL((k_cut_sweep<R, 16>), dim3(nb), dim3(BLK), 0, st, dv, b, fd),
                 hipLaunchKernelGGL((k_cut_sweep<R, 64>), dim3(nb), dim3(BLK), 0, st, dv, b, fd));
    const int nseg = cut_segments(b.N);
    const long n = (long)R * nseg;
    hipLaunchKernelGGL((k_cut_compact<R, 0>), dim3(blocks_for(n)), dim3(BLK), 0, st, fd, b.N, nseg, cnt, nullptr, nullptr, nullptr);
    launch_exclusive_scan(cnt, off, n, sums, st);
    hipLaunchKernelGGL(k_cut_heads<R>, dim3(1), dim3(64), 0, st, dv, b.req, off, sums + (n + SCAN_TILE - 1) / SCAN_TILE, nseg, len, rhs);
}
// phase 2: the ordered fill (ocol / oval hold the batch's total), and the edge norms when the primal norms are kept
void launch_cut_fill(const DevView& dv, const double* fd, int N, const int* off, int* ocol, double* oval, bool gamma, hipStream_t st) {
    constexpr int R = RG_BATCH;
    const int nseg = cut_segments(N);
    hipLaunchKernelGGL((k_cut_compact<R, 1>), dim3(blocks_for((long)R * nseg)), dim3(BLK), 0, st, fd, N, nseg, nullptr, off, ocol, oval);
    if (gamma) hipLaunchKernelGGL(k_cut_gamma<R>, dim3(blocks_for(N)), dim3(BLK), 0, st, dv, fd, N);
}

// ------------------------------------------------------------------- row append (R >= 1 rows)
// The R new rows are the tail of the CSR (rptr[0..R] are the row pointers of the new rows, each row = its sorted terms on old
// columns followed by its slack).  cnt[j] = number of new rows that hold old column j (binary search per row); cnt[n_old] = 0.
__device__ __forceinline__ int csc_find(const int* __restrict__ rcol, int b, int e, int j) {  // index of j in the sorted [b, e), or -1
    int lo = b, hi = e;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rcol[mid] < j) lo = mid + 1;
        else hi = mid;
    }
    return lo < e && rcol[lo] == j ? lo : -1;
}
__global__ void __launch_bounds__(BLK) k_csc_rows_count(const int* __restrict__ rptr, const int* __restrict__ rcol, int R, int n_old,
                                                        int* __restrict__ cnt) {
    const int j = blockIdx.x * BLK + threadIdx.x;
    if (j > n_old) return;
    int c = 0;
    if (j < n_old)
        for (int i = 0; i < R; ++i) c += csc_find(rcol, rptr[i], rptr[i + 1] - 1, j) >= 0;
    cnt[j] = c;
}
// shift: exclusive scan of cnt (shift[n_old] = all new entries on old columns).  Old column j moves by shift[j] and gains its new
// entries at its end in row order; the R slack columns follow, one entry (+1) each (solver.rs:250).
template <int G>
__global__ void __launch_bounds__(BLK) k_csc_append_rows(const int* __restrict__ optr, const int* __restrict__ orow,
                                                         const double* __restrict__ oval, int n_old, int row0, int R,
                                                         const int* __restrict__ rptr, const int* __restrict__ rcol,
                                                         const double* __restrict__ rval, const int* __restrict__ shift,
                                                         int* __restrict__ nptr, int* __restrict__ nrow, double* __restrict__ nval) {
    const int j = (blockIdx.x * BLK + threadIdx.x) / G;
    const int gl = threadIdx.x & (G - 1);
    if (j >= n_old + R) return;
    if (j >= n_old) {
        if (gl == 0) {
            const int i = j - n_old;
            const int b = optr[n_old] + shift[n_old] + i;
            nptr[j] = b;
            if (i == R - 1) nptr[j + 1] = b + 1;
            nrow[b] = row0 + i;
            nval[b] = 1.0;
        }
        return;
    }
    const int ob = optr[j], oe = optr[j + 1];
    const int nb = ob + shift[j];
    for (int e = ob + gl; e < oe; e += G) {
        nrow[nb + (e - ob)] = orow[e];
        nval[nb + (e - ob)] = oval[e];
    }
    if (gl == 0) {
        nptr[j] = nb;
        int w = nb + (oe - ob);
        for (int i = 0; i < R; ++i) {
            const int at = csc_find(rcol, rptr[i], rptr[i + 1] - 1, j);
            if (at >= 0) {
                nrow[w] = row0 + i;
                nval[w] = rval[at];
                ++w;
            }
        }
    }
}
void launch_csc_append_rows(const int* optr, const int* orow, const double* oval, int n_old, int row0, int R, const int* rptr,
                            const int* rcol, const double* rval, int* cnt, int* sums, int* nptr, int* nrow, double* nval,
                            hipStream_t st) {
    hipLaunchKernelGGL(k_csc_rows_count, dim3(blocks_for(n_old + 1)), dim3(BLK), 0, st, rptr, rcol, R, n_old, cnt);
    launch_exclusive_scan(cnt, cnt, (long)n_old + 1, sums, st);
    hipLaunchKernelGGL(k_csc_append_rows<16>, dim3(blocks_for((long)(n_old + R) * 16)), dim3(BLK), 0, st, optr, orow, oval, n_old, row0,
                       R, rptr, rcol, rval, cnt, nptr, nrow, nval);
}
