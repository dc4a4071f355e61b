// Training mixtures on the device (rtfs-net_amd/datas.py mix_batch; DESIGN.md "Training mixtures"): what the reference's
// System.online_mixing_collate (src/system/core.py:183-202) does with torch ops, and the target-speaker form this project trains
// (a target plus interferers at a drawn SNR, at a drawn crop of each utterance), as one planned call of two launches.
//   rtfs_mix_plan         host only: validates the recipe and builds the int64 table the launches read from device memory
//   mix_moments_kernel    pass 1, one workgroup per (row, chunk): float64 partial moments of the row's segments into the workspace
//   mix_apply_kernel      pass 2, one workgroup per (row, chunk): re-reduces the row's partials in a fixed order, forms the gains and
//                         the mixture's mean / deviation FROM THE MOMENTS, then writes mixture and sources (no third pass over samples)
// tests/mix_oracle.py restates the definition in float64 numpy.  All arithmetic on samples is IEEE float64 multiply, add, subtract in a
// fixed order; that is only reproducible bit for bit without fused multiply-add, so contraction is off for the file (as k_mouth.hip).
// Caller's stream, no allocation, nothing read back, no atomics: one writer per cell and fixed reduction orders.
#pragma clang fp contract(off)
#include <math.h>
#include <string.h>

#include "../../include/rtfs_amd.h"
#include "common.h"

namespace {

constexpr int MJ = RTFS_MIX_MAX_SOURCES;
constexpr int MCHUNK = RTFS_MIX_CHUNK;
constexpr int MW = RTFS_MIX_TABLE_WORDS;
constexpr int MM = RTFS_MIX_MOMENTS;  // [sum x_j (J) | E(ref_j) (J) | sum x_i x_j, i <= j, row-major (J (J + 1) / 2; the diagonal is E(x_j))]
constexpr int MG = 2 * MJ;            // first cross product
static_assert(MJ == 4 && MM == 2 * MJ + MJ * (MJ + 1) / 2, "the moment layout is written out for four slots");

// one slot of a row as the kernels hold it: segment and reference already point at their first sample
struct MixSlot {
    const char* x;
    const char* r;
    double a;
    int xi16, ri16;
};

__device__ __forceinline__ MixSlot mix_slot(const long long* __restrict__ table, int b, int j) {
    const long long* w = table + ((size_t)b * MJ + j) * MW;
    MixSlot s;
    s.x = (const char*)(uintptr_t)w[0];
    s.r = (const char*)(uintptr_t)w[1];
    s.a = __longlong_as_double(w[2]);
    s.xi16 = (int)(w[3] & 1);
    s.ri16 = (int)((w[3] >> 1) & 1);
    return s;
}

// sample i of a segment: float32 as it lies, int16 PCM as (float)s / 32768 (exact)
__device__ __forceinline__ double mix_ld(const char* p, int i16, int i) {
    return i16 ? (double)((float)((const short*)p)[i] * (1.0f / 32768.0f)) : (double)((const float*)p)[i];
}

// ---------------------------------------------------------------- pass 1
__global__ __launch_bounds__(256) void mix_moments_kernel(const long long* __restrict__ table, double* __restrict__ part, int L, int NC) {
    __shared__ double red[4][MM];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / NC, c = blockIdx.x - b * NC;
    const int lo = c * MCHUNK, n = min(MCHUNK, L - lo);
    MixSlot s[MJ];
#pragma unroll
    for (int j = 0; j < MJ; ++j) s[j] = mix_slot(table, b, j);
    double acc[MM];
#pragma unroll
    for (int k = 0; k < MM; ++k) acc[k] = 0.0;
    for (int i = lo + tid; i < lo + n; i += 256) {
        double x[MJ];
#pragma unroll
        for (int j = 0; j < MJ; ++j) {
            x[j] = s[j].x ? mix_ld(s[j].x, s[j].xi16, i) : 0.0;
            acc[j] += x[j];
            if (s[j].r) {
                const double r = mix_ld(s[j].r, s[j].ri16, i);
                acc[MJ + j] += r * r;  // the square of a float32 value is exact in double
            }
        }
        int k = MG;
#pragma unroll
        for (int p = 0; p < MJ; ++p)
#pragma unroll
            for (int q = p; q < MJ; ++q) acc[k++] += x[p] * x[q];
    }
#pragma unroll
    for (int k = 0; k < MM; ++k) {
        const double v = wave_sum_d(acc[k]);
        if ((tid & 63) == 0) red[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid < MM) part[((size_t)b * NC + c) * MM + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// ---------------------------------------------------------------- pass 2
// y[0 .. n) = val(i): a scalar head up to the row's own 16-byte grid, 16-byte stores (a wave: 1024 contiguous bytes, whole 128-byte
// lines), a scalar tail
template <class F>
__device__ __forceinline__ void mix_write_row(float* __restrict__ y, int n, int tid, F val) {
    int head = (int)((4 - ((((uintptr_t)y) >> 2) & 3)) & 3);
    head = head < n ? head : n;
    if (tid < head) y[tid] = val(tid);
    const int nq = (n - head) >> 2;
    for (int q = tid; q < nq; q += 256) {
        const int i = head + 4 * q;
        *(f32x4*)(y + i) = f32x4{val(i), val(i + 1), val(i + 2), val(i + 3)};
    }
    for (int i = head + 4 * nq + tid; i < n; i += 256) y[i] = val(i);
}

template <bool NORM>
__global__ __launch_bounds__(256) void mix_apply_kernel(const long long* __restrict__ table, const double* __restrict__ part,
                                                         float* __restrict__ mixture, float* __restrict__ sources, double* __restrict__ stats,
                                                         int L, int NC, int n_out, double eps) {
    __shared__ double red[4][MM];
    __shared__ double sh[2 * MJ + 2];  // [g_j | mean(g_j x_j) | mean(m) | inv]
    const int tid = threadIdx.x;
    const int b = blockIdx.x / NC, c = blockIdx.x - b * NC;
    MixSlot s[MJ];
#pragma unroll
    for (int j = 0; j < MJ; ++j) s[j] = mix_slot(table, b, j);
    // every workgroup of a row sums the same partials in the same order (NC <= 256: thread tid holds chunk tid; lanes, then waves), so
    // all of them apply the same constants
    const double* pr = part + (size_t)b * NC * MM;
#pragma unroll
    for (int k = 0; k < MM; ++k) {
        const double v = wave_sum_d(tid < NC ? pr[(size_t)tid * MM + k] : 0.0);
        if ((tid & 63) == 0) red[tid >> 6][k] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double M[MM], g[MJ];
        for (int k = 0; k < MM; ++k) M[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
        const int diag[MJ] = {MG, MG + 4, MG + 7, MG + 9};
        double sm = 0.0;
        for (int j = 0; j < MJ; ++j) {
            g[j] = !s[j].x ? 0.0 : (s[j].r ? s[j].a * sqrt(M[MJ + j] / M[diag[j]]) : s[j].a);  // no eps: silence gives inf / NaN
            sh[j] = g[j];
            sh[MJ + j] = g[j] * (M[j] / (double)L);
            if (s[j].x) sm += g[j] * M[j];
        }
        double smm = 0.0;  // g^T G g
        int k = MG;
        for (int p = 0; p < MJ; ++p)
            for (int q = p; q < MJ; ++q, ++k)
                if (s[p].x && s[q].x) smm += (p == q ? 1.0 : 2.0) * (g[p] * g[q]) * M[k];
        // L = 1: NaN, as torch.std (said outright: the two roundings of the one square need not cancel to the 0 / 0 that gives it)
        double var = L > 1 ? (smm - sm * sm / (double)L) / (double)(L - 1) : __builtin_nan("");
        var = var < 0.0 ? 0.0 : var;  // rounding of a constant mixture; NaN stays NaN
        sh[2 * MJ] = sm / (double)L;
        sh[2 * MJ + 1] = 1.0 / (sqrt(var) + eps);
        if (c == 0) {
            double* st = stats + (size_t)b * (MJ + 2);
            for (int j = 0; j < MJ; ++j) st[j] = g[j];
            st[MJ] = sh[2 * MJ];
            st[MJ + 1] = sh[2 * MJ + 1];
        }
    }
    __syncthreads();
    double g[MJ];
#pragma unroll
    for (int j = 0; j < MJ; ++j) g[j] = sh[j];
    const double mean = sh[2 * MJ], inv = sh[2 * MJ + 1];
    const int lo = c * MCHUNK, n = min(MCHUNK, L - lo);
    // the mixture: the non-empty slots in the order j = 0, 1, ..., multiply then add
    mix_write_row(mixture + (size_t)b * L + lo, n, tid, [&](int i) {
        double m = 0.0;
        bool first = true;
#pragma unroll
        for (int j = 0; j < MJ; ++j) {
            if (!s[j].x) continue;
            const double t = g[j] * mix_ld(s[j].x, s[j].xi16, lo + i);
            m = first ? t : m + t;
            first = false;
        }
        return NORM ? (float)((m - mean) * inv) : (float)m;
    });
    for (int j = 0; j < n_out; ++j) {
        const MixSlot sj = mix_slot(table, b, j);
        const double gj = sh[j], mj = sh[MJ + j];
        mix_write_row(sources + ((size_t)b * n_out + j) * L + lo, n, tid, [&](int i) {
            const double t = sj.x ? gj * mix_ld(sj.x, sj.xi16, lo + i) : 0.0;
            return NORM ? (float)((t - mj) * inv) : (float)t;
        });
    }
}

int mix_refuse(int* refused, long long where, int reason) {
    if (refused) {
        refused[0] = (int)where;
        refused[1] = reason;
    }
    return RTFS_ERR_ARG;
}

bool mix_sizes_ok(int B, int L) { return B >= 1 && L >= 1 && L <= RTFS_MIX_MAX_LENGTH && (long long)B * cdiv(L, MCHUNK) <= 0x7fffffffLL; }

}  // namespace

extern "C" {

size_t rtfs_mix_workspace_bytes(int B, int L) {
    if (!mix_sizes_ok(B, L)) return 0;
    return (size_t)B * cdiv(L, MCHUNK) * MM * sizeof(double);
}

int rtfs_mix_plan(const long long* slots, const double* a, int B, int L, int n_out, long long* table, size_t* ws_bytes, int* refused) {
    if (!slots || !a || B < 1) return mix_refuse(refused, -1, RTFS_MIX_BAD_ARGUMENT);
    if (L < 1 || L > RTFS_MIX_MAX_LENGTH) return mix_refuse(refused, -1, RTFS_MIX_BAD_LENGTH);
    if (!mix_sizes_ok(B, L) || (long long)B * MJ > 0x7fffffffLL) return mix_refuse(refused, -1, RTFS_MIX_BAD_ARGUMENT);
    if (n_out < 0 || n_out > MJ) return mix_refuse(refused, -1, RTFS_MIX_BAD_N_OUT);
    for (int b = 0; b < B; ++b) {
        int used = 0;
        for (int j = 0; j < MJ; ++j) {
            const long long idx = (long long)b * MJ + j;
            const long long* w = slots + idx * RTFS_MIX_RECIPE_WORDS;
            if (!w[0]) continue;
            ++used;
            for (int h = 0; h < 2; ++h) {  // the segment, then its reference
                const long long addr = w[4 * h], len = w[4 * h + 1], dt = w[4 * h + 2], start = w[4 * h + 3];
                if (h && !addr) continue;
                if (dt != RTFS_MIX_F32 && dt != RTFS_MIX_I16) return mix_refuse(refused, idx, RTFS_MIX_BAD_DTYPE);
                if (addr & (dt == RTFS_MIX_F32 ? 3 : 1)) return mix_refuse(refused, idx, RTFS_MIX_MISALIGNED);
                if (start < 0 || len < 0 || start > len || len - start < L)
                    return mix_refuse(refused, idx, h ? RTFS_MIX_REFERENCE_RANGE : RTFS_MIX_SEGMENT_RANGE);
            }
        }
        if (!used) return mix_refuse(refused, (long long)b * MJ, RTFS_MIX_EMPTY_ROW);
    }
    if (ws_bytes) *ws_bytes = rtfs_mix_workspace_bytes(B, L);
    if (table) {
        for (long long idx = 0; idx < (long long)B * MJ; ++idx) {
            const long long* w = slots + idx * RTFS_MIX_RECIPE_WORDS;
            long long* t = table + idx * MW;
            t[0] = t[1] = t[2] = t[3] = 0;
            if (!w[0]) continue;
            t[0] = w[0] + w[3] * (w[2] == RTFS_MIX_F32 ? 4 : 2);
            if (w[4]) t[1] = w[4] + w[7] * (w[6] == RTFS_MIX_F32 ? 4 : 2);
            memcpy(&t[2], &a[idx], sizeof(double));
            t[3] = (w[2] == RTFS_MIX_I16 ? 1 : 0) | (w[4] && w[6] == RTFS_MIX_I16 ? 2 : 0);
        }
    }
    return RTFS_OK;
}

int rtfs_mix_f32(const long long* table, float* mixture, float* sources, double* stats, int B, int L, int n_out, int normalize, double eps,
                 void* ws, size_t ws_bytes, void* stream) {
    if (!table || !mixture || !stats || !ws) return RTFS_ERR_ARG;
    if (!mix_sizes_ok(B, L) || n_out < 0 || n_out > MJ) return RTFS_ERR_SHAPE;
    if (n_out > 0 && !sources) return RTFS_ERR_ARG;
    if (ws_bytes < rtfs_mix_workspace_bytes(B, L)) return RTFS_ERR_WORKSPACE;
    if (((((uintptr_t)table) | ((uintptr_t)stats) | ((uintptr_t)ws)) & 7) || ((((uintptr_t)mixture) | ((uintptr_t)sources)) & 3)) return RTFS_ERR_ARG;
    const int NC = cdiv(L, MCHUNK);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mix_moments_kernel, dim3((unsigned)(B * NC)), dim3(256), 0, st, table, (double*)ws, L, NC);
    const int e = rtfs_launch_status();
    if (e != RTFS_OK) return e;
    if (normalize)
        hipLaunchKernelGGL(mix_apply_kernel<true>, dim3((unsigned)(B * NC)), dim3(256), 0, st, table, (const double*)ws, mixture, sources, stats, L,
                           NC, n_out, eps);
    else
        hipLaunchKernelGGL(mix_apply_kernel<false>, dim3((unsigned)(B * NC)), dim3(256), 0, st, table, (const double*)ws, mixture, sources, stats,
                           L, NC, n_out, eps);
    return rtfs_launch_status();
}

}  // extern "C"
