// cuts.inc — a round of cuts in one call (include/minilp_hip.h: mlp_solution_add_gomory_cuts, mlp_solution_add_constraints_csr;
// DESIGN.md §7.3).
//
// Cut generation, RG_BATCH = 16 Gomory cuts per pass over A:
//   the 16 rows of B^-1 come from launch_ranging_block (ranging.inc: explicit inverse with its pending terms applied, singleton
//   positions, compact factor) as ONE block rho[m][16]; k_cut_sweep is one pass over A's CSC: alpha = csc_block_dot (ranging.inc, the
//   accumulator of every batched pass), then f = floor(alpha) - alpha written as a dense block f[N][16] BY VARIABLE (basic variables: 0);
//   then the non-zero f become sparse rows on the device: a count pass (per segment of CUT_SEG variables and request), an exclusive
//   scan in request-major order, and an ordered fill.  A thread owns one (segment, request) pair in both passes and walks its
//   segment in variable order, so every cut comes out sorted by variable with no atomics, no ballots and no LDS, bit-identically
//   from run to run and whatever else the batch holds (alpha_j[r] is summed in storage order, then by the xor tree of the lane
//   group: its value depends on request r alone).  The launches of phase 1 are launch_rows_generate (tableau.inc), shared with the
//   tableau rows and the GMI round.  Side-effect free like ranging: only the private buffers are written.
// Row append (R = 1 is Solution::add_constraint): one re-layout of the CSC for R new rows (they are the last R rows, so every column
//   gains its new entries at its end, in row order): per-column counts from the R sorted rows, a scan, one copy kernel.

constexpr int CUT_SEG = 16;  // variables per (segment, request) thread of the count / fill passes

template <int R, int G>
__global__ void __launch_bounds__(BLK) k_cut_sweep(DevView v, RangingBufs b, double* __restrict__ fd) {
    const int var = (int)(((long)blockIdx.x * BLK + threadIdx.x) / G);
    const int gl = threadIdx.x & (G - 1);
    double acc[R];
    const bool live = var < b.N && v.var_loc[var] < 0;
    csc_block_dot<R, G>(v, b.blk, live, var, gl, acc);
    if (var < b.N && gl == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = live ? floor(acc[r]) - acc[r] : 0.0;
        store_block_row<R>(fd + (size_t)var * R, acc);
    }
}
// count / fill: thread (segment, request); MODE 0 counts the non-zero f of its segment, MODE 1 writes them behind off[r * nseg + seg],
// MODE 2 (GMI) counts and leaves the segment's share of the right-hand side, sum f_j xN_j in variable order, in part
template <int R, int MODE>
__global__ void __launch_bounds__(BLK) k_cut_compact(const double* __restrict__ fd, int N, int nseg, int* __restrict__ cnt,
                                                     const int* __restrict__ off, int* __restrict__ ocol, double* __restrict__ oval,
                                                     const int* __restrict__ var_loc, const double* __restrict__ xN,
                                                     double* __restrict__ part) {
    const long gid = (long)blockIdx.x * BLK + threadIdx.x;
    const int r = (int)(gid % R);
    const long seg = gid / R;
    if (seg >= nseg) return;
    const int v0 = (int)seg * CUT_SEG, v1 = min(N, v0 + CUT_SEG);
    int pos = MODE == 1 ? off[(size_t)r * nseg + seg] : 0;
    double s = 0.0;
    for (int j = v0; j < v1; ++j) {
        const double f = fd[(size_t)j * R + r];
        if (f != 0.0) {  // exact zeros carry no information (only a non-basic column holds a non-zero)
            if (MODE == 1) {
                ocol[pos] = j;
                oval[pos] = f;
            }
            if (MODE == 2) s += f * xN[-1 - var_loc[j]];
            ++pos;
        }
    }
    if (MODE != 1) cnt[(size_t)r * nseg + seg] = pos;
    if (MODE == 2) part[(size_t)r * nseg + seg] = s;
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

// (phase 1 of a batch — block of rows, sweep, count, scan, heads — is launch_rows_generate, tableau.inc)
// phase 2: the ordered fill (ocol / oval hold the batch's total), and the edge norms when the primal norms are kept
void launch_cut_fill(const DevView& dv, const double* fd, int N, const int* off, int* ocol, double* oval, bool gamma, hipStream_t st) {
    constexpr int R = RG_BATCH;
    const int nseg = cut_segments(N);
    hipLaunchKernelGGL((k_cut_compact<R, 1>), dim3(blocks_for((long)R * nseg)), dim3(BLK), 0, st, fd, N, nseg, nullptr, off, ocol, oval,
                       nullptr, nullptr, nullptr);
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
