// The metrics tracker's four PIT figures (SDR, SDRi, SI-SNR, SI-SNRi; reference src/metrics/allwrapper.py:35-56) for R mixtures of
// different lengths in one pass over the samples.  Per mixture the tracker asks for four pairwise matrices -- (estimate, clean) and
// (stacked mixture, clean), each as snr and as sisdr -- and all four follow from ONE set of float64 moments of the 2 n + 1 signals
// (pit_pairwise_kernel's algebra, k_loss.hip), so every sample is read once where the four single-length launches read it four times:
//   score_moments_kernel   one workgroup per (chunk of SCORE_MOM_CHUNK samples, recording), a flat work list (score_many_plan, k_stoi.hip):
//                          sums, sums of squares, <est_i, clean_j> and <mix, clean_j>; one partial per workgroup, one writer, no atomics.
//                          A recording's chunks count from its own start, so its partials do not depend on the pool.
//   score_sdr_fold_kernel  one workgroup per recording: folds its partials in a fixed order (lane c % 256 takes chunk c, then the block
//                          sum), derives the matrices (zero-mean, EPS 1e-8, noise^2 clamped at 0, 10 log10(. + eps)) and scans the n!
//                          permutations in itertools order, first minimum wins.
// Recordings are separate allocations at any 4-byte alignment: dword loads only.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int MAXN = 4;

// moment m of a partial: [s1 (2n+1) | s2 (2n+1) | <est_i, clean_j> (n n) | <mix, clean_j> (n)], signals ordered mix, clean 0.., est 0..
template <int N>
__global__ __launch_bounds__(256) void score_moments_kernel(const float* const* __restrict__ mixes, const float* const* __restrict__ cleans,
                                                            const float* const* __restrict__ ests, const int* __restrict__ table, int R,
                                                            double* __restrict__ mom) {
    constexpr int NS = 2 * N + 1, NM = score_moments(N);
    __shared__ double red[4][NM];
    const int tid = threadIdx.x, R1 = R + 1;
    const int* first = table + SC_MC0 * R1;
    int r = 0, hi = R;  // the last r with first[r] <= blockIdx.x
    while (hi - r > 1) {
        const int mid = (r + hi) >> 1;
        if (first[mid] <= (int)blockIdx.x) r = mid; else hi = mid;
    }
    const int L = table[SC_L * R1 + r];
    const int l0 = ((int)blockIdx.x - first[r]) * SCORE_MOM_CHUNK, l1 = min(L, l0 + SCORE_MOM_CHUNK);
    const float *m = mixes[r], *c = cleans[r], *e = ests[r];
    double acc[NM];
#pragma unroll
    for (int k = 0; k < NM; ++k) acc[k] = 0;
    for (int l = l0 + tid; l < l1; l += 256) {
        double v[NS];
        v[0] = (double)m[l];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            v[1 + j] = (double)c[(size_t)j * L + l];
            v[1 + N + j] = (double)e[(size_t)j * L + l];
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            acc[s] += v[s];
            acc[NS + s] += v[s] * v[s];
        }
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = 0; j < N; ++j) acc[2 * NS + i * N + j] += v[1 + N + i] * v[1 + j];
#pragma unroll
        for (int j = 0; j < N; ++j) acc[2 * NS + N * N + j] += v[0] * v[1 + j];
    }
#pragma unroll
    for (int k = 0; k < NM; ++k) {
        const double s = wave_sum_d(acc[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = s;
    }
    __syncthreads();
    if (tid < NM) mom[(size_t)blockIdx.x * NM + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// -loss of one (estimate, target) pair from its moments: PairwiseNegSDR.forward with zero_mean and take_log, as pit_pairwise_kernel
__device__ __forceinline__ float pair_loss(double se, double st, double ee, double tt, double et, double Ld, bool sisdr) {
    const double eps = 1e-8;
    const double me = se / Ld, mt = st / Ld;
    ee -= Ld * me * me;
    tt -= Ld * mt * mt;
    et -= Ld * me * mt;
    double proj2, noise2;
    if (!sisdr) {  // snr: proj = t, noise = e - t
        proj2 = tt;
        noise2 = ee - 2 * et + tt;
    } else {
        const double alpha = et / (tt + eps);
        proj2 = alpha * alpha * tt;
        noise2 = ee - 2 * alpha * et + alpha * alpha * tt;
    }
    noise2 = noise2 < 0 ? 0 : noise2;
    return (float)(-10.0 * log10(proj2 / (noise2 + eps) + eps));
}

__global__ __launch_bounds__(256) void score_sdr_fold_kernel(const int* __restrict__ table, int R, int n, const double* __restrict__ mom,
                                                             float* __restrict__ out, int* __restrict__ perm_out) {
    __shared__ double red[4];
    __shared__ double M[score_moments(MAXN)];
    __shared__ float pws[2][MAXN * MAXN];  // [snr | sisdr][estimate][target]
    __shared__ float base[2][MAXN];        // (mixture, clean j)
    const int tid = threadIdx.x, r = blockIdx.x, R1 = R + 1;
    const int NS = 2 * n + 1, NM = score_moments(n);
    const int c0 = table[SC_MC0 * R1 + r], nc = table[SC_MC0 * R1 + r + 1] - c0;
    for (int k = 0; k < NM; ++k) {
        double s = 0;
        for (int c = tid; c < nc; c += 256) s += mom[(size_t)(c0 + c) * NM + k];
        s = wave_sum_d(s);
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) M[k] = red[0] + red[1] + red[2] + red[3];
    }
    __syncthreads();
    const double Ld = (double)table[SC_L * R1 + r];
    if (tid < 2 * n * n) {
        const int kind = tid / (n * n), i = (tid % (n * n)) / n, j = tid % n;  // estimate i, target j
        pws[kind][i * MAXN + j] = pair_loss(M[1 + n + i], M[1 + j], M[NS + 1 + n + i], M[NS + 1 + j], M[2 * NS + i * n + j], Ld, kind == 1);
    } else if (tid >= 64 && tid < 64 + 2 * n) {
        const int kind = (tid - 64) / n, j = (tid - 64) % n;
        base[kind][j] = pair_loss(M[0], M[1 + j], M[NS], M[NS + 1 + j], M[2 * NS + n * n + j], Ld, kind == 1);
    }
    __syncthreads();
    if (tid < 2) {  // lane 0: snr, lane 1: sisdr
        // permutations of range(n) in lexicographic (itertools) order; loss = mean_i pw[perm[i]][i]; first minimum wins
        const float* pw = pws[tid];
        int p[MAXN], best[MAXN];
        for (int i = 0; i < n; ++i) p[i] = best[i] = i;
        float bl = 0.f;
        bool first = true;
        while (true) {
            float s = 0.f;
            for (int i = 0; i < n; ++i) s += pw[p[i] * MAXN + i];
            s /= (float)n;
            if (first || s < bl) {
                bl = s;
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
        // the stacked mixture's matrix has equal rows, so every permutation gives mean_j base[j], summed in target order
        float b = 0.f;
        for (int j = 0; j < n; ++j) b += base[tid][j];
        b /= (float)n;
        out[(size_t)r * 4 + 2 * tid] = bl;
        out[(size_t)r * 4 + 2 * tid + 1] = bl - b;
        if (tid == 1)
            for (int i = 0; i < n; ++i) perm_out[(size_t)r * n + i] = best[i];
    }
}

}  // namespace

int launch_sdr_many(const float* const* mixes, const float* const* cleans, const float* const* ests, const int* table, const int* plan, int R,
                    int n_src, int fs, void* ws, size_t ws_bytes, float* out, int* perm, hipStream_t st) {
    ScoreManyWs w;
    int r = score_many_carve(plan, R, n_src, fs, ws, ws_bytes, &w);
    if (r != RTFS_OK) return r;
    const dim3 grid(plan[SC_MC0 * (R + 1) + R]), block(256);
    switch (n_src) {
        case 1: hipLaunchKernelGGL(score_moments_kernel<1>, grid, block, 0, st, mixes, cleans, ests, table, R, w.mom); break;
        case 2: hipLaunchKernelGGL(score_moments_kernel<2>, grid, block, 0, st, mixes, cleans, ests, table, R, w.mom); break;
        case 3: hipLaunchKernelGGL(score_moments_kernel<3>, grid, block, 0, st, mixes, cleans, ests, table, R, w.mom); break;
        default: hipLaunchKernelGGL(score_moments_kernel<4>, grid, block, 0, st, mixes, cleans, ests, table, R, w.mom); break;
    }
    if ((r = rtfs_launch_status()) != RTFS_OK) return r;
    hipLaunchKernelGGL(score_sdr_fold_kernel, dim3(R), block, 0, st, table, R, n_src, w.mom, out, perm);
    return rtfs_launch_status();
}
