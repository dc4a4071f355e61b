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
    int p[MAXN], best[MAXN];
    for (int i = 0; i < n; ++i) p[i] = best[i] = i;
    double bm = 0;
    bool first = true;
    while (true) {  // permutations of range(n) in lexicographic (itertools) order; first maximum of the mean wins
        double s = 0;
        for (int j = 0; j < n; ++j) s += db[p[j]][j];
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
