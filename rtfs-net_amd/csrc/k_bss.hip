// BSS-eval SDR (mir_eval.separation.bss_eval_sources' SDR column, fast_bss_eval's permutation rule): the ratio after the estimate has
// been projected onto the 512 delayed copies of the true source (definition: rtfs_amd.h, "BSS-eval SDR").  All float64.
//   bss_corr_kernel    one workgroup per (chunk of BSS_CHUNK samples, reference j, tile of 256 lags), a flat work list.  It stages the
//                      chunk of s_j in LDS and then, one right-hand signal x at a time (s_j itself, the n estimates, the mixture), the
//                      chunk of x with its 511-sample halo, and accumulates sum_t s[t] x[t + k].  Wave w takes samples [1024 w, 1024 w
//                      + 1024) of the chunk, lane l the four lags 4 l .. 4 l + 3 of the tile (4 samples x 4 lags per step: three 16-byte
//                      LDS reads feed 16 FMAs); the four waves fold through LDS in wave order.  One partial per (chunk, j, x, lag), one
//                      writer, plain stores.  The workgroup of (j = 0, tile 0) also writes the chunk's sum of x^2 per signal.
//   bss_solve_kernel   one workgroup per (recording, reference j): folds that reference's partials chunk by chunk in chunk order, then
//                      Levinson-Durbin on Toeplitz(r_j) for all right-hand sides at once.  NT threads own 512 / NT taps each (tap i
//                      belongs to thread i % NT); the predictor lives in two LDS buffers, the solutions in registers; per order one
//                      reduction (wave butterfly, then the waves' sums in wave order) and one exchange of the predictor.  NT = 512:
//                      two barriers per order; NT = 64: a single wave, no cross-wave step -- the production form, the faster of the two
//                      on the MI355X.  Writes num = c'd and den = max(ee - num, 0).
//   bss_final_kernel   one thread per recording: the n x n matrix 10 log10(num / den), the permutation with the largest mean in
//                      itertools order (first maximum), sdr, sdr_i and perm.
// A recording's chunks count from its own start and every fold has a fixed order, so its bits depend on neither batch, pool nor
// scheduling.  The block entry and the pooled entry run the SAME kernels; they differ in how a workgroup finds its recording (batch
// index | bisection of column 10 of score_many_plan's table) and its rows (base + offset | device arrays of pointers, dword loads).
#include "common.h"
#include "kernels.h"

namespace {

constexpr int F = BSS_TAPS, CH = BSS_CHUNK, TILE = 256, NTILE = F / TILE;
constexpr int XS = CH + F;  // staged samples of a right-hand signal: the chunk and its halo (the last one is never multiplied)
static_assert(CH % 1024 == 0 && F == 512 && CH == SCORE_MOM_CHUNK, "four waves of 1024 samples; the pooled work list is column 10");

struct BssRows {  // where the signals are: block entry (table == nullptr) or pooled
    const float *clean, *est, *mix;                 // (B,n,L), (B,n,L), (B,L) | nullptr
    const float *const *cleans, *const *ests, *const *mixes;  // R device pointers each
    const int* table;                               // device copy of score_many_plan's table
    int R, L, nc;                                   // pooled: R recordings; block: L and chunks per row
};

// recording and chunk of global chunk g, the recording's length and first global chunk
__device__ __forceinline__ void bss_locate(const BssRows& a, int g, int& row, int& c, int& L) {
    if (a.table) {
        const int R1 = a.R + 1;
        const int* first = a.table + SC_MC0 * R1;
        int r = 0, hi = a.R;  // the last r with first[r] <= g
        while (hi - r > 1) {
            const int mid = (r + hi) >> 1;
            if (first[mid] <= g) r = mid; else hi = mid;
        }
        row = r;
        c = g - first[r];
        L = a.table[SC_L * R1 + r];
    } else {
        row = g / a.nc;
        c = g - row * a.nc;
        L = a.L;
    }
}

__global__ __launch_bounds__(256) void bss_corr_kernel(BssRows a, int n, int with_mix, double* __restrict__ corr, double* __restrict__ eep) {
    __shared__ __attribute__((aligned(16))) float S[CH];
    __shared__ __attribute__((aligned(16))) float X[XS];
    __shared__ double red[4][TILE];
    __shared__ double red2[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int NR = n + with_mix, NQ = 1 + NR;
    const int g = (int)blockIdx.x / (n * NTILE), rem = (int)blockIdx.x % (n * NTILE), j = rem / NTILE, tile = rem % NTILE;
    int row, c, L;
    bss_locate(a, g, row, c, L);
    const float *pc, *pe, *pm;
    if (a.table) {
        pc = a.cleans[row];
        pe = a.ests[row];
        pm = with_mix ? a.mixes[row] : nullptr;
    } else {
        pc = a.clean + (size_t)row * n * L;
        pe = a.est + (size_t)row * n * L;
        pm = with_mix ? a.mix + (size_t)row * L : nullptr;
    }
    const int t0 = c * CH;
    const float* s = pc + (size_t)j * L;
    for (int i = tid; i < CH; i += 256) S[i] = t0 + i < L ? s[t0 + i] : 0.f;
    const bool want_ee = j == 0 && tile == 0;
    const int k0 = tile * TILE + 4 * lane;  // this lane's first lag
    for (int q = 0; q < NQ; ++q) {
        const float* x = q == 0 ? s : (q <= n ? pe + (size_t)(q - 1) * L : pm);
        double sq = 0;
        for (int i = tid; i < XS; i += 256) {
            const float v = t0 + i < L ? x[t0 + i] : 0.f;
            X[i] = v;
            if (i < CH) sq += (double)v * (double)v;
        }
        __syncthreads();  // S (first round) and X are staged; red / red2 of the previous round have been read
        double acc[4] = {0, 0, 0, 0};
        for (int t = w * 1024; t < (w + 1) * 1024; t += 4) {
            const f32x4 sv = *(const f32x4*)&S[t];
            const f32x4 xa = *(const f32x4*)&X[t + k0], xb = *(const f32x4*)&X[t + k0 + 4];  // t + k0 + 7 <= XS - 1
            const double sd[4] = {(double)sv[0], (double)sv[1], (double)sv[2], (double)sv[3]};
            const double xd[7] = {(double)xa[0], (double)xa[1], (double)xa[2], (double)xa[3], (double)xb[0], (double)xb[1], (double)xb[2]};
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) acc[kk] = fma(sd[u], xd[u + kk], acc[kk]);
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) red[w][4 * lane + kk] = acc[kk];
        if (want_ee && q > 0) {
            sq = wave_sum_d(sq);
            if (lane == 0) red2[w] = sq;
        }
        __syncthreads();
        corr[(((size_t)g * n + j) * NQ + q) * F + tile * TILE + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        if (want_ee && q > 0 && tid == 0) eep[(size_t)g * NR + (q - 1)] = (red2[0] + red2[1]) + (red2[2] + red2[3]);
        // the next round's staging writes X only; its barrier orders these reads of red / red2 before the next writes to them
    }
}

// Levinson-Durbin for NR right-hand sides.  Stop rule: the recursion ends at order m when the prediction error E_m <= r[0] 2^-46 (or at
// order 0 when r[0] is not positive); taps m .. 511 stay 0 and `order` = m taps were solved (512: the guard never fired).
template <int NT, int NR>
__global__ __launch_bounds__(NT) void bss_solve_kernel(const int* __restrict__ table, int R, int nc_block, int n, const double* __restrict__ corr,
                                                       const double* __restrict__ eep, double* __restrict__ nd, double* __restrict__ dbg_r,
                                                       double* __restrict__ dbg_d, double* __restrict__ dbg_ee, int* __restrict__ dbg_order) {
    constexpr int TPL = F / NT, NW = NT / 64, NQ = NR + 1;
    __shared__ double r[F], A[2][F], D[NR][F], EE[NR];
    __shared__ double red[2][NW][NQ];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row = (int)blockIdx.x / n, j = (int)blockIdx.x % n;
    int g0, nc;
    if (table) {
        g0 = table[SC_MC0 * (R + 1) + row];
        nc = table[SC_MC0 * (R + 1) + row + 1] - g0;
    } else {
        g0 = row * nc_block;
        nc = nc_block;
    }
    // fold the partials chunk by chunk, in chunk order
    const size_t cstride = (size_t)n * NQ * F;
    const double* base = corr + ((size_t)g0 * n + j) * NQ * F;
#pragma unroll
    for (int u = 0; u < TPL; ++u) {
        const int i = tid + NT * u;
        double s[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) s[q] = 0;
        for (int c = 0; c < nc; ++c)
#pragma unroll
            for (int q = 0; q < NQ; ++q) s[q] += base[c * cstride + (size_t)q * F + i];
        r[i] = s[0];
#pragma unroll
        for (int q = 0; q < NR; ++q) D[q][i] = s[1 + q];
        A[0][i] = A[1][i] = i == 0 ? 1.0 : 0.0;
    }
    if (tid < NR) {
        double s = 0;
        for (int c = 0; c < nc; ++c) s += eep[(size_t)(g0 + c) * NR + tid];
        EE[tid] = s;
    }
    __syncthreads();
    const double r0 = r[0], floor_e = r0 * 0x1p-46;
    double a[TPL], x[TPL][NR];
#pragma unroll
    for (int u = 0; u < TPL; ++u) {
        a[u] = tid + NT * u == 0 ? 1.0 : 0.0;  // a[0] = 1: the predictor polynomial's leading coefficient
#pragma unroll
        for (int q = 0; q < NR; ++q) x[u][q] = 0;
    }
    int order = 0;
    double E = r0;
    if (r0 > 0) {
        order = 1;
        if (tid == 0)
#pragma unroll
            for (int q = 0; q < NR; ++q) x[0][q] = D[q][0] / r0;
        for (int m = 1; m < F; ++m) {
            // a, x are of order m - 1: p[0] = sum_{i < m} a[i] r[m - i] (a[0] = 1), p[1 + q] = sum_{i < m} x_q[i] r[m - i]
            double p[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) p[q] = 0;
#pragma unroll
            for (int u = 0; u < TPL; ++u) {
                const int i = tid + NT * u;
                if (i < m) {
                    const double rv = r[m - i];
                    p[0] = fma(a[u], rv, p[0]);
#pragma unroll
                    for (int q = 0; q < NR; ++q) p[1 + q] = fma(x[u][q], rv, p[1 + q]);
                }
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) p[q] = wave_sum_d(p[q]);
            if (NW > 1) {
                if (lane == 0)
#pragma unroll
                    for (int q = 0; q < NQ; ++q) red[m & 1][w][q] = p[q];
                __syncthreads();
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    double s = red[m & 1][0][q];
#pragma unroll
                    for (int v = 1; v < NW; ++v) s += red[m & 1][v][q];
                    p[q] = s;
                }
            }
            const double k = -p[0] / E, En = E * (1.0 - k * k);
            if (!(En > floor_e)) break;  // every thread holds the same values: the whole workgroup leaves together
            const double* Aold = A[(m - 1) & 1];
            double* Anew = A[m & 1];
            double mu[NR];
#pragma unroll
            for (int q = 0; q < NR; ++q) mu[q] = (D[q][m] - p[1 + q]) / En;
#pragma unroll
            for (int u = 0; u < TPL; ++u) {
                const int i = tid + NT * u;
                if (i <= m) {
                    const double am = Aold[m - i];
                    const double an = fma(k, am, a[u]);    // a_new[i]
                    const double anr = fma(k, a[u], am);   // a_new[m - i], the backward vector's entry i
#pragma unroll
                    for (int q = 0; q < NR; ++q) x[u][q] = fma(mu[q], anr, x[u][q]);
                    a[u] = an;
                    Anew[i] = an;
                }
            }
            __syncthreads();
            E = En;
            order = m + 1;
        }
    }
    // num = c'd
    double p[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) p[q] = 0;
#pragma unroll
    for (int u = 0; u < TPL; ++u)
#pragma unroll
        for (int q = 0; q < NR; ++q) p[q] = fma(x[u][q], D[q][tid + NT * u], p[q]);
#pragma unroll
    for (int q = 0; q < NR; ++q) p[q] = wave_sum_d(p[q]);
    __syncthreads();  // a break leaves straight after the reduction's reads of red
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < NR; ++q) red[0][w][q] = p[q];
    __syncthreads();
    if (tid < NR) {
        double num = red[0][0][tid];
        for (int v = 1; v < NW; ++v) num += red[0][v][tid];
        const double den = EE[tid] - num;
        double* o = nd + ((size_t)blockIdx.x * NR + tid) * 2;
        o[0] = num;
        o[1] = den > 0 ? den : (den != den ? den : 0.0);
        if (dbg_ee) dbg_ee[(size_t)blockIdx.x * NR + tid] = EE[tid];
    }
    if (dbg_r) {
#pragma unroll
        for (int u = 0; u < TPL; ++u) {
            const int i = tid + NT * u;
            dbg_r[(size_t)blockIdx.x * F + i] = r[i];
#pragma unroll
            for (int q = 0; q < NR; ++q) dbg_d[((size_t)blockIdx.x * NR + q) * F + i] = D[q][i];
        }
        if (tid == 0) dbg_order[blockIdx.x] = order;
    }
}

// the permutation of range(n) with the largest mean of M[p[j]][j] over the sources: lexicographic (itertools) order, first maximum
__device__ __forceinline__ void bss_best_perm(const double (*M)[4], int n, int* best) {
    int p[4];
    for (int i = 0; i < n; ++i) p[i] = best[i] = i;
    double bm = 0;
    bool first = true;
    while (true) {
        double s = 0;
        for (int j = 0; j < n; ++j) s += M[p[j]][j];
        s /= (double)n;
        if (first || s > bm) {
            bm = s;
            first = false;
            for (int i = 0; i < n; ++i) best[i] = p[i];
        }
        int k = n - 2;
        while (k >= 0 && p[k] > p[k + 1]) --k;
        if (k < 0) break;
        int q = n - 1;
        while (p[q] < p[k]) --q;
        int tmp = p[k]; p[k] = p[q]; p[q] = tmp;
        for (int lo = k + 1, hi = n - 1; lo < hi; ++lo, --hi) { tmp = p[lo]; p[lo] = p[hi]; p[hi] = tmp; }
    }
}

// nd (rows, n[j], NR[q], 2): q < n the estimates, q = n the mixture.  perm[j] = the estimate assigned to clean source j.
__global__ __launch_bounds__(64) void bss_final_kernel(int rows, int n, int with_mix, const double* __restrict__ nd, float* __restrict__ sdr,
                                                       float* __restrict__ sdr_i, int* __restrict__ perm_out) {
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= rows) return;
    constexpr int MAXN = 4;
    const int NR = n + with_mix;
    double db[MAXN + 1][MAXN];  // [q][j]
    for (int j = 0; j < n; ++j)
        for (int q = 0; q < NR; ++q) {
            const double* v = nd + (((size_t)row * n + j) * NR + q) * 2;
            db[q][j] = 10.0 * log10(v[0] / v[1]);
        }
    int best[MAXN];
    bss_best_perm(db, n, best);
    for (int j = 0; j < n; ++j) {
        const double v = db[best[j]][j];
        sdr[(size_t)row * n + j] = (float)v;
        if (with_mix) sdr_i[(size_t)row * n + j] = (float)(v - db[n][j]);
        perm_out[(size_t)row * n + j] = best[j];
    }
}

struct BssWs {
    double *corr, *eep, *nd;
};
// three regions, each rounded up to 256 bytes: correlation partials (G, n, 1 + NR, 512), sum-of-squares partials (G, NR), num / den
// (rows, n, NR, 2); G = chunks over all recordings
size_t bss_carve(long long G, long long rows, int n, int with_mix, char* base, BssWs* w) {
    const size_t NR = (size_t)(n + with_mix);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        off = align_up(off, 256);
        char* r = base ? base + off : nullptr;
        off += bytes;
        return r;
    };
    w->corr = (double*)take((size_t)G * n * (1 + NR) * F * sizeof(double));
    w->eep = (double*)take((size_t)G * NR * sizeof(double));
    w->nd = (double*)take((size_t)rows * n * NR * 2 * sizeof(double));
    return off;
}

template <int NT>
void solve_launch(int NR, int blocks, hipStream_t st, const int* table, int R, int nc, int n, const BssWs& w, const BssDebug& d) {
#define BSS_SOLVE(K) \
    hipLaunchKernelGGL((bss_solve_kernel<NT, K>), dim3(blocks), dim3(NT), 0, st, table, R, nc, n, w.corr, w.eep, w.nd, d.r, d.d, d.ee, d.order)
    switch (NR) {
        case 1: BSS_SOLVE(1); break;
        case 2: BSS_SOLVE(2); break;
        case 3: BSS_SOLVE(3); break;
        case 4: BSS_SOLVE(4); break;
        default: BSS_SOLVE(5); break;
    }
#undef BSS_SOLVE
}

int bss_launch(const BssRows& a, long long G, int rows, int n, int with_mix, const BssWs& w, float* sdr, float* sdr_i, int* perm,
               const BssDebug& dbg, hipStream_t st) {
    int r;
    hipLaunchKernelGGL(bss_corr_kernel, dim3((unsigned)(G * n * NTILE)), dim3(256), 0, st, a, n, with_mix, w.corr, w.eep);
    if ((r = rtfs_launch_status()) != RTFS_OK) return r;
    if (dbg.form == 512)
        solve_launch<512>(n + with_mix, rows * n, st, a.table, a.R, a.nc, n, w, dbg);
    else  // production: the single wave measured faster at 32 x 2 s and at 256 x 2 s ("BSS-eval SDR")
        solve_launch<64>(n + with_mix, rows * n, st, a.table, a.R, a.nc, n, w, dbg);
    if ((r = rtfs_launch_status()) != RTFS_OK) return r;
    hipLaunchKernelGGL(bss_final_kernel, dim3(cdiv(rows, 64)), dim3(64), 0, st, rows, n, with_mix, w.nd, sdr, sdr_i, perm);
    return rtfs_launch_status();
}

}  // namespace

size_t bss_sdr_workspace_bytes(int B, int n_src, int L, int with_mix) {
    if (B < 1 || L < 1 || n_src < 1 || n_src > 4) return 0;
    BssWs w;
    return bss_carve((long long)B * cdiv(L, CH), B, n_src, with_mix != 0, nullptr, &w);
}

int launch_bss_sdr(const float* clean, const float* est, const float* mix, int B, int n_src, int L, void* ws, size_t ws_bytes, float* sdr,
                   float* sdr_i, int* perm, const BssDebug& dbg, hipStream_t st) {
    const int with_mix = mix != nullptr;
    if (!clean || !est || !ws || !sdr || !perm || (with_mix && !sdr_i) || B < 1 || L < 1 || n_src < 1 || n_src > 4) return RTFS_ERR_ARG;
    if (dbg.form != 0 && dbg.form != 64 && dbg.form != 512) return RTFS_ERR_ARG;
    const int nc = cdiv(L, CH);
    const long long G = (long long)B * nc;
    if (G * n_src * NTILE > 0x7fffffffLL || (long long)B * n_src > 0x7fffffffLL) return RTFS_ERR_SHAPE;
    BssWs w;
    if (bss_carve(G, B, n_src, with_mix, nullptr, &w) > ws_bytes) return RTFS_ERR_WORKSPACE;
    bss_carve(G, B, n_src, with_mix, (char*)ws, &w);
    BssRows a = {clean, est, mix, nullptr, nullptr, nullptr, nullptr, 0, L, nc};
    return bss_launch(a, G, B, n_src, with_mix, w, sdr, sdr_i, perm, dbg, st);
}

// 0 for a plan that is not one of R recordings
size_t bss_sdr_many_workspace_bytes(const int* plan, int R, int with_mix) {
    if (!plan || R < 1) return 0;
    const int R1 = R + 1, n_src = plan[SC_L * R1 + R];
    if (plan[SC_K0 * R1 + R] != R || n_src < 1 || n_src > 4) return 0;
    BssWs w;
    return bss_carve(plan[SC_MC0 * R1 + R], R, n_src, with_mix != 0, nullptr, &w);
}

int launch_bss_sdr_many(const float* const* mixes, const float* const* cleans, const float* const* ests, const int* table, const int* plan,
                        int R, int n_src, int fs, void* ws, size_t ws_bytes, float* sdr, float* sdr_i, int* perm, const BssDebug& dbg,
                        hipStream_t st) {
    const int with_mix = mixes != nullptr;
    if (!cleans || !ests || !table || !plan || !ws || !sdr || !perm || (with_mix && !sdr_i)) return RTFS_ERR_ARG;
    if (R < 1 || n_src < 1 || n_src > 4 || (fs != 16000 && fs != 10000)) return RTFS_ERR_ARG;
    if (dbg.form != 0 && dbg.form != 64 && dbg.form != 512) return RTFS_ERR_ARG;
    const int R1 = R + 1;
    if (plan[SC_L * R1 + R] != n_src || plan[SC_L10 * R1 + R] != fs || plan[SC_K0 * R1 + R] != R) return RTFS_ERR_ARG;
    const long long G = plan[SC_MC0 * R1 + R];
    if (G * n_src * NTILE > 0x7fffffffLL) return RTFS_ERR_SHAPE;
    BssWs w;
    if (bss_carve(G, R, n_src, with_mix, nullptr, &w) > ws_bytes) return RTFS_ERR_WORKSPACE;
    bss_carve(G, R, n_src, with_mix, (char*)ws, &w);
    BssRows a = {nullptr, nullptr, nullptr, cleans, ests, mixes, table, R, 0, 0};
    return bss_launch(a, G, R, n_src, with_mix, w, sdr, sdr_i, perm, dbg, st);
}

// ================================================================ BSS-eval SIR and SAR: the joint projection onto all sources
// (definition: rtfs_amd.h, "BSS-eval SIR and SAR").  J = n + m true sources: the n scored ones, then m others.  Four launches:
//   bss_xcorr_kernel       bss_corr_kernel's scheme with every one of the J sources staged; its right-hand signals are the J sources and
//                          the n estimates (partials xc (G, J, J + n, 512): r_ij[k >= 0] from the pair (stage s_i, read s_j), the negative
//                          lags from the pair (stage s_j, read s_i)) and, for a scored source, the mixture.  What bss_solve_kernel reads --
//                          r_jj, the d rows of the estimates and the mixture, the sums of squares -- is stored a second time in that
//                          kernel's own layout; the arithmetic per (staged, read) pair is bss_corr_kernel's, so those bits are its bits.
//   bss_solve_kernel       unchanged: p_j and max(ee - p_j, 0) per (estimate | mixture, scored source).
//   bss_joint_kernel       one workgroup of 512 threads per recording, thread t owns tap t.  Folds the partials chunk by chunk in chunk
//                          order, then a block Levinson recursion with J x J blocks over the 512 orders for all n estimates at once.  The
//                          forward predictor, the solutions and the right-hand sides live in registers; the backward predictor lives in
//                          LDS and is updated in place (at size m its block t sits in slot (t - m) mod 512, so the shift by one tap that
//                          every order asks for costs nothing); r_ij in LDS, component-major (conflict-free 8-byte reads).  Per order one
//                          reduction of J^2 + J n values (wave butterfly, then the eight waves' sums in wave order) and two barriers.
//   bss_eval_final_kernel  one thread per recording: the SDR and SIR matrices, the permutation by the chosen rule, the outputs.
// Every fold has a fixed order and nothing is atomic: a recording's bits depend on neither batch, pool nor scheduling.
namespace {

struct BssJointRows {
    BssRows a;
    const float* other;          // block entry: (B, m, L) | nullptr
    const float* const* others;  // pooled entry: R m device pointers, row r's at [r m, r m + m)
    int m;
};

__global__ __launch_bounds__(256) void bss_xcorr_kernel(BssJointRows jr, int n, int with_mix, double* __restrict__ corr, double* __restrict__ eep,
                                                        double* __restrict__ xc) {
    __shared__ __attribute__((aligned(16))) float S[CH];
    __shared__ __attribute__((aligned(16))) float X[XS];
    __shared__ double red[4][TILE];
    __shared__ double red2[4];
    const BssRows& a = jr.a;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m = jr.m, J = n + m, NR = n + with_mix, NQ = 1 + NR, NX = J + n;
    const int g = (int)blockIdx.x / (J * NTILE), rem = (int)blockIdx.x % (J * NTILE), i = rem / NTILE, tile = rem % NTILE;
    int row, c, L;
    bss_locate(a, g, row, c, L);
    const float *pc, *pe, *pm;
    if (a.table) {
        pc = a.cleans[row];
        pe = a.ests[row];
        pm = with_mix ? a.mixes[row] : nullptr;
    } else {
        pc = a.clean + (size_t)row * n * L;
        pe = a.est + (size_t)row * n * L;
        pm = with_mix ? a.mix + (size_t)row * L : nullptr;
    }
    auto source = [&](int k) -> const float* {
        if (k < n) return pc + (size_t)k * L;
        return a.table ? jr.others[(size_t)row * m + (k - n)] : jr.other + ((size_t)row * m + (k - n)) * L;
    };
    const int t0 = c * CH;
    const float* s = source(i);
    for (int u = tid; u < CH; u += 256) S[u] = t0 + u < L ? s[t0 + u] : 0.f;
    const bool want_ee = i == 0 && tile == 0;
    const int k0 = tile * TILE + 4 * lane;  // this lane's first lag
    const int nq = NX + (i < n ? with_mix : 0);
    for (int q = 0; q < nq; ++q) {
        const float* x = q < J ? source(q) : (q < NX ? pe + (size_t)(q - J) * L : pm);
        double sq = 0;
        for (int u = tid; u < XS; u += 256) {
            const float v = t0 + u < L ? x[t0 + u] : 0.f;
            X[u] = v;
            if (u < CH) sq += (double)v * (double)v;
        }
        __syncthreads();  // S (first round) and X are staged; red / red2 of the previous round have been read
        double acc[4] = {0, 0, 0, 0};
        for (int t = w * 1024; t < (w + 1) * 1024; t += 4) {
            const f32x4 sv = *(const f32x4*)&S[t];
            const f32x4 xa = *(const f32x4*)&X[t + k0], xb = *(const f32x4*)&X[t + k0 + 4];  // t + k0 + 7 <= XS - 1
            const double sd[4] = {(double)sv[0], (double)sv[1], (double)sv[2], (double)sv[3]};
            const double xd[7] = {(double)xa[0], (double)xa[1], (double)xa[2], (double)xa[3], (double)xb[0], (double)xb[1], (double)xb[2]};
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) acc[kk] = fma(sd[u], xd[u + kk], acc[kk]);
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) red[w][4 * lane + kk] = acc[kk];
        const bool ee_round = want_ee && q >= J;
        if (ee_round) {
            sq = wave_sum_d(sq);
            if (lane == 0) red2[w] = sq;
        }
        __syncthreads();
        const double v = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        if (q < NX) xc[(((size_t)g * J + i) * NX + q) * F + tile * TILE + tid] = v;
        if (i < n) {  // bss_solve_kernel's layout: q = 0 the source itself, then the estimates, then the mixture
            const int oq = q == i ? 0 : (q >= J ? 1 + (q - J) : -1);
            if (oq >= 0) corr[(((size_t)g * n + i) * NQ + oq) * F + tile * TILE + tid] = v;
        }
        if (ee_round && tid == 0) eep[(size_t)g * NR + (q - J)] = (red2[0] + red2[1]) + (red2[2] + red2[3]);
        // the next round's staging writes X only; its barrier orders these reads of red / red2 before the next writes to them
    }
}

// Gauss-Jordan without pivoting on a J x J error block (symmetric positive definite when all is well).  false when a pivot is not above
// its floor: the stop rule.  The inverse is then not to be used.
template <int J>
__device__ __forceinline__ bool bss_invert(const double (&E)[J][J], const double (&floor_)[J], double (&inv)[J][J]) {
    double A[J][J];
#pragma unroll
    for (int i = 0; i < J; ++i)
#pragma unroll
        for (int j = 0; j < J; ++j) {
            A[i][j] = E[i][j];
            inv[i][j] = i == j ? 1.0 : 0.0;
        }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < J; ++i) {
        const double p = A[i][i];
        ok = ok && p > floor_[i];
        const double ip = 1.0 / p;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            A[i][j] *= ip;
            inv[i][j] *= ip;
        }
#pragma unroll
        for (int k = 0; k < J; ++k)
            if (k != i) {
                const double f = A[k][i];
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    A[k][j] = fma(-f, A[i][j], A[k][j]);
                    inv[k][j] = fma(-f, inv[i][j], inv[k][j]);
                }
            }
    }
    return ok;
}

constexpr int JT = 512, JW = JT / 64;  // threads and waves of the joint solve
template <int J, int N>
constexpr size_t bss_joint_lds() {
    return (size_t)(2 * F * J * J + JW * (J * J + J * N) + (J * J + J * N) + 2 * J * N + 2 * 4 * J * J) * sizeof(double);
}

// Block Levinson on the block-Toeplitz matrix with blocks M[a - b], M[k][i][j] = r_ij[k], M[-k] = M[k]'.  At size m (m taps solved):
//   forward predictor  Fw[0 .. m-1] (Fw[0] = I):  sum_b M[a - b] Fw[b] = E_f at a = 0, 0 at a = 1 .. m-1
//   backward predictor Bw[0 .. m-1] (Bw[m-1] = I): the same with E_b at a = m-1 and 0 above
//   step:  delta = sum_{t < m} M[m - t] Fw[t],  eta = sum_{t < m} M[m - t] X[t]
//          K_f = E_b^-1 delta,  K_b = E_f^-1 delta',  E_f <- E_f - delta' K_f,  E_b <- E_b - delta K_b
//          Fw[t] <- Fw[t] - Bw[t-1] K_f,  Bw[t] <- Bw[t-1] - Fw[t] K_b  (t = 0 .. m; Bw[-1] = Fw[m] = 0),  X[t] <- X[t] + Bw[t] E_b^-1 (Y[m] - eta)
// Stop rule: the recursion ends at order m (taps m .. 511 stay 0) when a pivot of the new E_f or E_b, eliminated without pivoting, is not
// above 2^-46 r_ii[0] of its source i; at order 0 the block is M[0].  A silent source (r_ii[0] = 0) is decoupled: its diagonal entry of
// M[0] is taken as 1, all its other correlations are 0, so its taps come out 0 and the others do not see it.  When at most one source
// is active and it is a scored one, the joint projection IS the scalar one: p_all is taken from bss_solve_kernel's result (bit-equal,
// so SIR = +inf and SAR = SDR exactly); with no active source p_all = 0.
// Outputs pall (rows, N, 2): p_all = C'D_all and ee per estimate.
template <int J, int N>
__global__ __launch_bounds__(JT) void bss_joint_kernel(const int* __restrict__ table, int R, int nc_block, int with_mix,
                                                       const double* __restrict__ xc, const double* __restrict__ eep,
                                                       const double* __restrict__ nd, double* __restrict__ pall, double* __restrict__ dbg_r,
                                                       double* __restrict__ dbg_d, int* __restrict__ dbg_order) {
    constexpr int JJ = J * J, NV = JJ + J * N, NX = J + N;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* Rl = lds;                 // [JJ][512]: component (i, j), lag k
    double* Bl = Rl + F * JJ;         // [JJ][512]: component, slot
    double* red = Bl + F * JJ;        // [JW][NV]
    double* fin = red + JW * NV;      // [NV]
    double* yb = fin + NV;            // [2][J N]: Y[m], double-buffered by the order's parity
    double* Es = yb + 2 * J * N;      // [2][4][JJ]: E_f, E_b and their inverses, double-buffered
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int row = blockIdx.x, NR = N + with_mix;
    int g0, nc;
    if (table) {
        g0 = table[SC_MC0 * (R + 1) + row];
        nc = table[SC_MC0 * (R + 1) + row + 1] - g0;
    } else {
        g0 = row * nc_block;
        nc = nc_block;
    }
    // fold the partials chunk by chunk, in chunk order: tap t's J x J block of M and its J x N block of the right-hand sides
    double Y[J][N];
    {
        double s[J][NX];
#pragma unroll
        for (int i = 0; i < J; ++i)
#pragma unroll
            for (int q = 0; q < NX; ++q) s[i][q] = 0;
        const double* base = xc + (size_t)g0 * J * NX * F + t;
        for (int c = 0; c < nc; ++c)
#pragma unroll
            for (int i = 0; i < J; ++i)
#pragma unroll
                for (int q = 0; q < NX; ++q) s[i][q] += base[((size_t)(c * J + i) * NX + q) * F];
#pragma unroll
        for (int i = 0; i < J; ++i) {
#pragma unroll
            for (int j = 0; j < J; ++j) Rl[(i * J + j) * F + t] = s[i][j];
#pragma unroll
            for (int q = 0; q < N; ++q) Y[i][q] = s[i][J + q];
        }
    }
    if (t < N) {
        double s = 0;
        for (int c = 0; c < nc; ++c) s += eep[(size_t)(g0 + c) * NR + t];
        pall[((size_t)row * N + t) * 2 + 1] = s;
    }
    __syncthreads();
    if (dbg_r) {  // all lags: r_ij[k] at 511 + k, r_ij[-k] = r_ji[k]
#pragma unroll
        for (int i = 0; i < J; ++i) {
#pragma unroll
            for (int j = 0; j < J; ++j) {
                double* o = dbg_r + ((size_t)row * JJ + i * J + j) * (2 * F - 1) + (F - 1);
                o[t] = Rl[(i * J + j) * F + t];
                if (t) o[-t] = Rl[(j * J + i) * F + t];
            }
#pragma unroll
            for (int q = 0; q < N; ++q) dbg_d[(((size_t)row * N + q) * J + i) * F + t] = Y[i][q];
        }
    }
    double floor_[J], E0[J][J];
    int nact = 0, solo = 0;
#pragma unroll
    for (int i = 0; i < J; ++i) {
#pragma unroll
        for (int j = 0; j < J; ++j) E0[i][j] = Rl[(i * J + j) * F];
        floor_[i] = E0[i][i] * 0x1p-46;
        if (E0[i][i] == 0) {
            E0[i][i] = 1.0;
        } else {
            ++nact;
            solo = i;
        }
    }
    if (nact == 0 || (nact == 1 && solo < N)) {  // the joint set is empty or one scored source: the scalar solve has the answer
        if (t < N) pall[((size_t)row * N + t) * 2] = nact == 0 ? 0.0 : nd[(((size_t)row * N + solo) * NR + t) * 2];
        if (dbg_order && t == 0) dbg_order[row] = nact == 0 ? 0 : F;
        return;
    }
    double Fw[J][J], X[J][N], Ef[J][J], Eb[J][J], Eif[J][J], Eib[J][J];
#pragma unroll
    for (int i = 0; i < J; ++i) {
#pragma unroll
        for (int j = 0; j < J; ++j) Fw[i][j] = t == 0 && i == j ? 1.0 : 0.0;
#pragma unroll
        for (int q = 0; q < N; ++q) X[i][q] = 0;
    }
    int order = 0;
    if (bss_invert<J>(E0, floor_, Eif)) {
        order = 1;
        if (t == 0) {
#pragma unroll
            for (int i = 0; i < J; ++i) {
#pragma unroll
                for (int q = 0; q < N; ++q) {
                    double v = 0;
#pragma unroll
                    for (int k = 0; k < J; ++k) v = fma(Eif[i][k], Y[k][q], v);
                    X[i][q] = v;
                }
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    Bl[(i * J + j) * F + (F - 1)] = i == j ? 1.0 : 0.0;  // Bw[0] = I of size 1 sits in slot (0 - 1) mod 512
                    Es[0 * JJ + i * J + j] = Es[1 * JJ + i * J + j] = E0[i][j];
                    Es[2 * JJ + i * J + j] = Es[3 * JJ + i * J + j] = Eif[i][j];
                }
            }
        }
        for (int m = 1; m < F; ++m) {
            double acc[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) acc[v] = 0;
            if (t < m) {
                const double* Rm = Rl + (m - t);
#pragma unroll
                for (int i = 0; i < J; ++i)
#pragma unroll
                    for (int k = 0; k < J; ++k) {
                        const double rv = Rm[(i * J + k) * F];
#pragma unroll
                        for (int j = 0; j < J; ++j) acc[i * J + j] = fma(rv, Fw[k][j], acc[i * J + j]);
#pragma unroll
                        for (int q = 0; q < N; ++q) acc[JJ + i * N + q] = fma(rv, X[k][q], acc[JJ + i * N + q]);
                    }
            }
            if (t == m)
#pragma unroll
                for (int i = 0; i < J; ++i)
#pragma unroll
                    for (int q = 0; q < N; ++q) yb[(m & 1) * J * N + i * N + q] = Y[i][q];
#pragma unroll
            for (int v = 0; v < NV; ++v) acc[v] = wave_sum_d(acc[v]);
            if (lane == 0)
#pragma unroll
                for (int v = 0; v < NV; ++v) red[w * NV + v] = acc[v];
            __syncthreads();  // also: the previous order's E blocks (thread 0) and Bl slots are written
            if (t < NV) {
                double s = red[t];
#pragma unroll
                for (int u = 1; u < JW; ++u) s += red[u * NV + t];
                fin[t] = s;
            }
            __syncthreads();
            const double* Eo = Es + ((m - 1) & 1) * 4 * JJ;
            double dl[J][J], Kf[J][J], Kb[J][J], G[J][N];
#pragma unroll
            for (int i = 0; i < J; ++i)
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    dl[i][j] = fin[i * J + j];
                    Ef[i][j] = Eo[0 * JJ + i * J + j];
                    Eb[i][j] = Eo[1 * JJ + i * J + j];
                    Eif[i][j] = Eo[2 * JJ + i * J + j];
                    Eib[i][j] = Eo[3 * JJ + i * J + j];
                }
#pragma unroll
            for (int i = 0; i < J; ++i)
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    double a = 0, b = 0;
#pragma unroll
                    for (int k = 0; k < J; ++k) {
                        a = fma(Eib[i][k], dl[k][j], a);
                        b = fma(Eif[i][k], dl[j][k], b);
                    }
                    Kf[i][j] = a;
                    Kb[i][j] = b;
                }
#pragma unroll
            for (int i = 0; i < J; ++i)
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    double a = Ef[i][j], b = Eb[i][j];
#pragma unroll
                    for (int k = 0; k < J; ++k) {
                        a = fma(-dl[k][i], Kf[k][j], a);
                        b = fma(-dl[i][k], Kb[k][j], b);
                    }
                    Ef[i][j] = a;
                    Eb[i][j] = b;
                }
            const bool okf = bss_invert<J>(Ef, floor_, Eif), okb = bss_invert<J>(Eb, floor_, Eib);
            if (!(okf && okb)) break;  // every thread holds the same values: the whole workgroup leaves together
            if (t == 0) {
                double* En = Es + (m & 1) * 4 * JJ;
#pragma unroll
                for (int i = 0; i < J; ++i)
#pragma unroll
                    for (int j = 0; j < J; ++j) {
                        En[0 * JJ + i * J + j] = Ef[i][j];
                        En[1 * JJ + i * J + j] = Eb[i][j];
                        En[2 * JJ + i * J + j] = Eif[i][j];
                        En[3 * JJ + i * J + j] = Eib[i][j];
                    }
            }
#pragma unroll
            for (int i = 0; i < J; ++i)
#pragma unroll
                for (int q = 0; q < N; ++q) {
                    double v = 0;
#pragma unroll
                    for (int k = 0; k < J; ++k) v = fma(Eib[i][k], yb[(m & 1) * J * N + k * N + q] - fin[JJ + k * N + q], v);
                    G[i][q] = v;
                }
            if (t <= m) {
                double* slot = Bl + ((t - m - 1) & (F - 1));
                double Bo[J][J], Bn[J][J];
#pragma unroll
                for (int i = 0; i < J; ++i)
#pragma unroll
                    for (int j = 0; j < J; ++j) Bo[i][j] = t >= 1 ? slot[(i * J + j) * F] : 0.0;
#pragma unroll
                for (int i = 0; i < J; ++i)
#pragma unroll
                    for (int j = 0; j < J; ++j) {
                        double a = Fw[i][j], b = Bo[i][j];
#pragma unroll
                        for (int k = 0; k < J; ++k) {
                            a = fma(-Bo[i][k], Kf[k][j], a);
                            b = fma(-Fw[i][k], Kb[k][j], b);
                        }
                        dl[i][j] = a;  // the new Fw, kept apart until Bn is formed from the old one
                        Bn[i][j] = b;
                    }
#pragma unroll
                for (int i = 0; i < J; ++i) {
#pragma unroll
                    for (int j = 0; j < J; ++j) {
                        Fw[i][j] = dl[i][j];
                        slot[(i * J + j) * F] = Bn[i][j];
                    }
#pragma unroll
                    for (int q = 0; q < N; ++q) {
                        double v = X[i][q];
#pragma unroll
                        for (int k = 0; k < J; ++k) v = fma(Bn[i][k], G[k][q], v);
                        X[i][q] = v;
                    }
                }
            }
            order = m + 1;
            // the next order's first barrier orders this order's reads of fin, yb and Es before their next writes (yb and Es alternate)
        }
    }
    // p_all = C'D_all per estimate
    double p[N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
        double v = 0;
#pragma unroll
        for (int i = 0; i < J; ++i) v = fma(X[i][q], Y[i][q], v);
        p[q] = wave_sum_d(v);
    }
    __syncthreads();  // a break leaves straight after the reads of fin; red was last read before that barrier
    if (lane == 0)
#pragma unroll
        for (int q = 0; q < N; ++q) red[w * NV + q] = p[q];
    __syncthreads();
    if (t < N) {
        double s = red[t];
        for (int u = 1; u < JW; ++u) s += red[u * NV + t];
        pall[((size_t)row * N + t) * 2] = s;
    }
    if (dbg_order && t == 0) dbg_order[row] = order;
}

// nd as bss_final_kernel's; pall (rows, n, 2) = p_all and ee per estimate.  sar[j] is the SAR of the estimate assigned to source j.
__global__ __launch_bounds__(64) void bss_eval_final_kernel(int rows, int n, int with_mix, int by_sir, const double* __restrict__ nd,
                                                            const double* __restrict__ pall, float* __restrict__ sdr, float* __restrict__ sir,
                                                            float* __restrict__ sar, float* __restrict__ sdr_i, int* __restrict__ perm_out,
                                                            double* __restrict__ dbg_pall, double* __restrict__ dbg_pj) {
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= rows) return;
    constexpr int MAXN = 4;
    const int NR = n + with_mix;
    double db[MAXN + 1][MAXN], si[MAXN][MAXN], sa[MAXN];  // [q][j]
    for (int j = 0; j < n; ++j)
        for (int q = 0; q < NR; ++q) {
            const double* v = nd + (((size_t)row * n + j) * NR + q) * 2;
            db[q][j] = 10.0 * log10(v[0] / v[1]);
            if (q < n) {
                const double pa = pall[((size_t)row * n + q) * 2], d = pa - v[0];
                si[q][j] = 10.0 * log10(v[0] / (d > 0 ? d : (d != d ? d : 0.0)));
                if (dbg_pj) dbg_pj[((size_t)row * n + q) * n + j] = v[0];
            }
        }
    for (int q = 0; q < n; ++q) {
        const double pa = pall[((size_t)row * n + q) * 2], d = pall[((size_t)row * n + q) * 2 + 1] - pa;
        sa[q] = 10.0 * log10(pa / (d > 0 ? d : (d != d ? d : 0.0)));
        if (dbg_pall) dbg_pall[(size_t)row * n + q] = pa;
    }
    int best[MAXN];
    bss_best_perm(by_sir ? si : db, n, best);
    for (int j = 0; j < n; ++j) {
        const double v = db[best[j]][j];
        sdr[(size_t)row * n + j] = (float)v;
        sir[(size_t)row * n + j] = (float)si[best[j]][j];
        sar[(size_t)row * n + j] = (float)sa[best[j]];
        if (with_mix) sdr_i[(size_t)row * n + j] = (float)(v - db[n][j]);
        perm_out[(size_t)row * n + j] = best[j];
    }
}

struct BssEvalWs {
    BssWs s;
    double *xc, *pall;
};
// bss_carve's three regions for the n scored sources, then the joint partials (G, J, J + n, 512) and p_all / ee (rows, n, 2)
size_t bss_eval_carve(long long G, long long rows, int n, int m, int with_mix, char* base, BssEvalWs* w) {
    size_t off = align_up(bss_carve(G, rows, n, with_mix, base, &w->s), 256);
    const int J = n + m;
    w->xc = (double*)(base ? base + off : nullptr);
    off = align_up(off + (size_t)G * J * (J + n) * F * sizeof(double), 256);
    w->pall = (double*)(base ? base + off : nullptr);
    return off + (size_t)rows * n * 2 * sizeof(double);
}

template <int J, int N>
int joint_launch_one(int rows, hipStream_t st, const int* table, int R, int nc, int with_mix, const BssEvalWs& w, const BssEvalDebug& d) {
    constexpr size_t lds = bss_joint_lds<J, N>();
    static_assert(lds <= 160 * 1024, "the joint solve's LDS");
    if (lds > 48 * 1024 && rtfs_set_max_lds((const void*)bss_joint_kernel<J, N>, lds) != RTFS_OK) return RTFS_ERR_LAUNCH;
    hipLaunchKernelGGL((bss_joint_kernel<J, N>), dim3(rows), dim3(JT), lds, st, table, R, nc, with_mix, w.xc, w.s.eep, w.s.nd, w.pall, d.r, d.d,
                       d.order);
    return rtfs_launch_status();
}

int joint_launch(int J, int n, int rows, hipStream_t st, const int* table, int R, int nc, int with_mix, const BssEvalWs& w,
                 const BssEvalDebug& d) {
#define BSS_JOINT(JJ_, NN_) \
    if (J == JJ_ && n == NN_) return joint_launch_one<JJ_, NN_>(rows, st, table, R, nc, with_mix, w, d)
    BSS_JOINT(1, 1);
    BSS_JOINT(2, 1);
    BSS_JOINT(2, 2);
    BSS_JOINT(3, 1);
    BSS_JOINT(3, 2);
    BSS_JOINT(3, 3);
    BSS_JOINT(4, 1);
    BSS_JOINT(4, 2);
    BSS_JOINT(4, 3);
    BSS_JOINT(4, 4);
#undef BSS_JOINT
    return RTFS_ERR_ARG;
}

int bss_eval_launch(const BssJointRows& jr, long long G, int rows, int n, int with_mix, int perm_by, const BssEvalWs& w, float* sdr, float* sir,
                    float* sar, float* sdr_i, int* perm, const BssEvalDebug& dbg, hipStream_t st) {
    int r;
    const int J = n + jr.m;
    hipLaunchKernelGGL(bss_xcorr_kernel, dim3((unsigned)(G * J * NTILE)), dim3(256), 0, st, jr, n, with_mix, w.s.corr, w.s.eep, w.xc);
    if ((r = rtfs_launch_status()) != RTFS_OK) return r;
    solve_launch<64>(n + with_mix, rows * n, st, jr.a.table, jr.a.R, jr.a.nc, n, w.s, BssDebug{nullptr, nullptr, nullptr, nullptr, 0});
    if ((r = rtfs_launch_status()) != RTFS_OK) return r;
    if ((r = joint_launch(J, n, rows, st, jr.a.table, jr.a.R, jr.a.nc, with_mix, w, dbg)) != RTFS_OK) return r;
    hipLaunchKernelGGL(bss_eval_final_kernel, dim3(cdiv(rows, 64)), dim3(64), 0, st, rows, n, with_mix, perm_by == BSS_PERM_BY_SIR, w.s.nd, w.pall,
                       sdr, sir, sar, sdr_i, perm, dbg.pall, dbg.pj);
    return rtfs_launch_status();
}

bool bss_eval_counts_ok(int n_src, int n_other) { return n_src >= 1 && n_other >= 0 && n_src + n_other <= 4; }

}  // namespace

size_t bss_eval_workspace_bytes(int B, int n_src, int n_other, int L, int with_mix) {
    if (B < 1 || L < 1 || !bss_eval_counts_ok(n_src, n_other)) return 0;
    BssEvalWs w;
    return bss_eval_carve((long long)B * cdiv(L, CH), B, n_src, n_other, with_mix != 0, nullptr, &w);
}

int launch_bss_eval(const float* clean, const float* est, const float* mix, const float* other, int B, int n_src, int n_other, int L, void* ws,
                    size_t ws_bytes, float* sdr, float* sir, float* sar, float* sdr_i, int* perm, int perm_by, const BssEvalDebug& dbg,
                    hipStream_t st) {
    const int with_mix = mix != nullptr;
    if (!clean || !est || !ws || !sdr || !sir || !sar || !perm || (with_mix && !sdr_i) || B < 1 || L < 1) return RTFS_ERR_ARG;
    if (!bss_eval_counts_ok(n_src, n_other) || (n_other > 0 && !other)) return RTFS_ERR_ARG;
    if (perm_by != BSS_PERM_BY_SDR && perm_by != BSS_PERM_BY_SIR) return RTFS_ERR_ARG;
    const int nc = cdiv(L, CH);
    const long long G = (long long)B * nc;
    if (G * (n_src + n_other) * NTILE > 0x7fffffffLL || (long long)B * n_src > 0x7fffffffLL) return RTFS_ERR_SHAPE;
    BssEvalWs w;
    if (bss_eval_carve(G, B, n_src, n_other, with_mix, nullptr, &w) > ws_bytes) return RTFS_ERR_WORKSPACE;
    bss_eval_carve(G, B, n_src, n_other, with_mix, (char*)ws, &w);
    BssJointRows jr = {{clean, est, mix, nullptr, nullptr, nullptr, nullptr, 0, L, nc}, other, nullptr, n_other};
    return bss_eval_launch(jr, G, B, n_src, with_mix, perm_by, w, sdr, sir, sar, sdr_i, perm, dbg, st);
}

// 0 for a plan that is not one of R recordings
size_t bss_eval_many_workspace_bytes(const int* plan, int R, int n_other, int with_mix) {
    if (!plan || R < 1) return 0;
    const int R1 = R + 1, n_src = plan[SC_L * R1 + R];
    if (plan[SC_K0 * R1 + R] != R || !bss_eval_counts_ok(n_src, n_other)) return 0;
    BssEvalWs w;
    return bss_eval_carve(plan[SC_MC0 * R1 + R], R, n_src, n_other, with_mix != 0, nullptr, &w);
}

int launch_bss_eval_many(const float* const* mixes, const float* const* cleans, const float* const* ests, const float* const* others,
                         const int* table, const int* plan, int R, int n_src, int n_other, int fs, void* ws, size_t ws_bytes, float* sdr,
                         float* sir, float* sar, float* sdr_i, int* perm, int perm_by, hipStream_t st) {
    const int with_mix = mixes != nullptr;
    if (!cleans || !ests || !table || !plan || !ws || !sdr || !sir || !sar || !perm || (with_mix && !sdr_i)) return RTFS_ERR_ARG;
    if (R < 1 || !bss_eval_counts_ok(n_src, n_other) || (n_other > 0 && !others) || (fs != 16000 && fs != 10000)) return RTFS_ERR_ARG;
    if (perm_by != BSS_PERM_BY_SDR && perm_by != BSS_PERM_BY_SIR) return RTFS_ERR_ARG;
    const int R1 = R + 1;
    if (plan[SC_L * R1 + R] != n_src || plan[SC_L10 * R1 + R] != fs || plan[SC_K0 * R1 + R] != R) return RTFS_ERR_ARG;
    const long long G = plan[SC_MC0 * R1 + R];
    if (G * (n_src + n_other) * NTILE > 0x7fffffffLL) return RTFS_ERR_SHAPE;
    BssEvalWs w;
    if (bss_eval_carve(G, R, n_src, n_other, with_mix, nullptr, &w) > ws_bytes) return RTFS_ERR_WORKSPACE;
    bss_eval_carve(G, R, n_src, n_other, with_mix, (char*)ws, &w);
    BssJointRows jr = {{nullptr, nullptr, nullptr, cleans, ests, mixes, table, R, 0, 0}, nullptr, others, n_other};
    return bss_eval_launch(jr, G, R, n_src, with_mix, perm_by, w, sdr, sir, sar, sdr_i, perm,
                           BssEvalDebug{nullptr, nullptr, nullptr, nullptr, nullptr}, st);
}
