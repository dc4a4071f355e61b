// Reverberant training mixtures (rtfs-net_amd/datas.py reverberate / mix_batch(rirs=...); DESIGN.md "Reverberant mixtures"; definition:
// rtfs_amd.h "Reverberant mixtures"): every source convolved with its own room impulse response before the mix, history read from the
// utterance itself.
//   rtfs_reverb_plan       host only: validates S jobs and builds the int64 job table the launch reads from device memory
//   reverb_kernel          one workgroup per (image s, tile of RV_TILE output samples), a flat work list.  It walks the N taps of its tile
//                          in chunks of RV_CHUNK: per chunk it stages the taps (as doubles) and the RV_TILE + RV_CHUNK - 1 samples they
//                          touch (int16 converted, zeros outside the utterance) in LDS.  Thread i owns the 8 outputs 8 i .. 8 i + 7 in
//                          float64 registers behind a sliding window of 11 samples: per 4 taps one 16-byte LDS read of samples and two
//                          of taps feed 32 FMAs (bss_corr_kernel's scheme, 4 x 8 instead of 4 x 4).  The window rotates through three
//                          register groups, so the loop is written three steps (12 taps) at a time and the taps of a chunk that are
//                          left over (fewer than 12) take a plain loop.  No tap and no sample is padded into the sum: exactly the N
//                          products of the definition enter, in the order k = 0 .. N - 1.  One rounding to float32, then 16-byte stores
//                          on the image row's own 16-byte grid through LDS, scalar head and tail.
//   rtfs_mix_reverb_plan   host only: rtfs_mix_plan's recipe with an RIR per slot and per reference -> one table [reverb jobs | mix table]
//   rtfs_mix_reverb_f32    the reverb launch (skipped without images), then the two launches of rtfs_mix_f32, which read an image as one
//                          more float32 allocation
// The product of two float32 values is exact in float64, so fma(h, x, acc) is the rounded sum acc + h x and the order alone fixes the
// bits: the same job gives the same image whatever the batch.  Caller's stream, no allocation on the device, nothing read back, no
// atomics, one writer per cell.
#include <string.h>

#include <array>
#include <map>
#include <vector>

#include "../../include/rtfs_amd.h"
#include "common.h"

namespace {

constexpr int RT = RTFS_REVERB_TILE, RC = RTFS_REVERB_TAP_CHUNK, RW = RTFS_REVERB_JOB_WORDS, RR = RTFS_REVERB_RECIPE_WORDS;
constexpr int RNT = RT / 8;    // threads: 8 outputs each
constexpr int RXS = RT + RC;   // staged samples of a chunk (the last one is never multiplied)
constexpr int MJ = RTFS_MIX_MAX_SOURCES;
static_assert(RT % 512 == 0 && RC % 12 == 0 && RNT % 64 == 0 && RNT <= 256, "8 outputs per thread, whole waves; 12 taps per unrolled round");
static_assert(RW == 6 && RR == 7 && RTFS_MIX_RIR_WORDS == 6, "the records are written out below");

typedef double f64x2 __attribute__((ext_vector_type(2)));

// 4 taps x 8 outputs: output u takes tap v against window sample 3 + u - v (w = [lo | mid | hi], 12 samples of which 11 are used)
__device__ __forceinline__ void reverb_step(double (&acc)[8], const f32x4 lo, const f32x4 mid, const f32x4 hi, const double* __restrict__ h4) {
    const f64x2 ha = *(const f64x2*)h4, hb = *(const f64x2*)(h4 + 2);
    const double h[4] = {ha[0], ha[1], hb[0], hb[1]};
    const double w[11] = {(double)lo[0], (double)lo[1], (double)lo[2], (double)lo[3], (double)mid[0], (double)mid[1],
                          (double)mid[2], (double)mid[3], (double)hi[0], (double)hi[1], (double)hi[2]};
#pragma unroll
    for (int v = 0; v < 4; ++v)  // taps in ascending order: the order of the sum
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = fma(h[v], w[3 + u - v], acc[u]);
}

__global__ __launch_bounds__(RNT) void reverb_kernel(const long long* __restrict__ jobs, float* __restrict__ images, int L, int NT) {
    __shared__ __attribute__((aligned(16))) float X[RXS];
    __shared__ __attribute__((aligned(16))) double H[RC];
    const int tid = threadIdx.x;
    const int s = (int)blockIdx.x / NT, tile = (int)blockIdx.x - s * NT;
    const long long* w = jobs + (size_t)s * RW;
    const char* src = (const char*)(uintptr_t)w[0];
    const long long n_x = w[1], q = w[2];  // q = start + offset
    const float* rir = (const float*)(uintptr_t)w[3];
    const int N = (int)w[4], i16 = (int)w[5];
    const int t0 = tile * RT;
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k0 = 0; k0 < N; k0 += RC) {
        const int nk = min(RC, N - k0);
        __syncthreads();  // the previous chunk's reads of X and H are done
        // X[i] = x~[q + t0 - (k0 + RC - 1) + i]: output t, tap k0 + kk reads X[t + RC - 1 - kk]
        const long long base = q + t0 - (long long)(k0 + RC - 1);
        for (int i = tid; i < RXS; i += RNT) {
            const long long gi = base + i;
            float v = 0.f;
            if (gi >= 0 && gi < n_x) v = i16 ? (float)((const short*)src)[gi] * (1.0f / 32768.0f) : ((const float*)src)[gi];
            X[i] = v;
        }
        for (int i = tid; i < nk; i += RNT) H[i] = (double)rir[k0 + i];
        __syncthreads();
        const int b0 = 8 * tid + RC - 4;  // window base of step m: b0 - 4 m, a multiple of 4; the window is X[b .. b + 10]
        const int rounds = nk / 12;
        f32x4 mid = *(const f32x4*)&X[b0 + 4], hi = *(const f32x4*)&X[b0 + 8];  // b0 + 11 <= RXS - 1
        for (int r = 0; r < rounds; ++r) {
            const int b = b0 - 12 * r;  // b - 8 >= 8 tid + RC - 4 - 12 (RC / 12 - 1) - 8 = 8 tid >= 0
            const f32x4 a = *(const f32x4*)&X[b];
            reverb_step(acc, a, mid, hi, &H[12 * r]);
            hi = *(const f32x4*)&X[b - 4];
            reverb_step(acc, hi, a, mid, &H[12 * r + 4]);
            mid = *(const f32x4*)&X[b - 8];
            reverb_step(acc, mid, hi, a, &H[12 * r + 8]);  // the next round's window is [X[b - 12] | mid = X[b - 8] | hi = X[b - 4]]
        }
        for (int kk = 12 * rounds; kk < nk; ++kk) {  // fewer than 12 taps
            const double h = H[kk];
            const float* x = &X[8 * tid + RC - 1 - kk];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] = fma(h, (double)x[u], acc[u]);
        }
    }
    __syncthreads();  // X is free: the tile's float32 results go through it to reach the row's 16-byte grid
#pragma unroll
    for (int u = 0; u < 8; ++u) X[8 * tid + u] = (float)acc[u];
    __syncthreads();
    const int n = min(RT, L - t0);
    float* y = images + (size_t)s * L + t0;
    int head = (int)((4 - ((((uintptr_t)y) >> 2) & 3)) & 3);
    head = head < n ? head : n;
    if (tid < head) y[tid] = X[tid];
    const int nq = (n - head) >> 2;
    for (int c = tid; c < nq; c += RNT) {
        const int i = head + 4 * c;
        *(f32x4*)(y + i) = f32x4{X[i], X[i + 1], X[i + 2], X[i + 3]};
    }
    for (int i = head + 4 * nq + tid; i < n; i += RNT) y[i] = X[i];
}

int reverb_refuse(int* refused, long long where, int reason) {
    if (refused) {
        refused[0] = (int)where;
        refused[1] = reason;
    }
    return RTFS_ERR_ARG;
}

bool reverb_sizes_ok(long long S, int L) { return S >= 1 && L >= 1 && L <= RTFS_MIX_MAX_LENGTH && S * cdiv(L, RT) <= 0x7fffffffLL; }

// the checks of one job -> 0 or the reason; rec = [source address | length | dtype | start | RIR address | taps | offset]
int reverb_job_reason(const long long* rec, int L) {
    const long long addr = rec[0], len = rec[1], dt = rec[2], start = rec[3], rir = rec[4], taps = rec[5], off = rec[6];
    if (!addr || !rir) return RTFS_MIX_BAD_ARGUMENT;
    if (dt != RTFS_MIX_F32 && dt != RTFS_MIX_I16) return RTFS_MIX_BAD_DTYPE;
    if ((addr & (dt == RTFS_MIX_F32 ? 3 : 1)) || (rir & 3)) return RTFS_MIX_MISALIGNED;
    if (start < 0 || len < 0 || start > len || len - start < L) return RTFS_MIX_SEGMENT_RANGE;
    if (taps < 1 || taps > RTFS_REVERB_MAX_TAPS) return RTFS_REVERB_BAD_TAPS;
    if (off < 0 || off >= taps) return RTFS_REVERB_BAD_OFFSET;
    return 0;
}

void reverb_job_write(const long long* rec, long long* t) {
    t[0] = rec[0];
    t[1] = rec[1];
    t[2] = rec[3] + rec[6];
    t[3] = rec[4];
    t[4] = rec[5];
    t[5] = rec[2] == RTFS_MIX_I16 ? 1 : 0;
}

}  // namespace

extern "C" {

int rtfs_reverb_plan(const long long* jobs, int S, int L, long long* table, int* refused) {
    if (!jobs || S < 1) return reverb_refuse(refused, -1, RTFS_MIX_BAD_ARGUMENT);
    if (L < 1 || L > RTFS_MIX_MAX_LENGTH) return reverb_refuse(refused, -1, RTFS_MIX_BAD_LENGTH);
    if (!reverb_sizes_ok(S, L)) return reverb_refuse(refused, -1, RTFS_MIX_BAD_ARGUMENT);
    for (int s = 0; s < S; ++s) {
        const int reason = reverb_job_reason(jobs + (size_t)s * RR, L);
        if (reason) return reverb_refuse(refused, s, reason);
    }
    if (table)
        for (int s = 0; s < S; ++s) reverb_job_write(jobs + (size_t)s * RR, table + (size_t)s * RW);
    return RTFS_OK;
}

int rtfs_reverb_f32(const long long* table, float* images, int S, int L, void* stream) {
    if (!table || !images) return RTFS_ERR_ARG;
    if (!reverb_sizes_ok(S, L)) return RTFS_ERR_SHAPE;
    if ((((uintptr_t)table) & 7) || (((uintptr_t)images) & 3)) return RTFS_ERR_ARG;
    const int NT = cdiv(L, RT);
    hipLaunchKernelGGL(reverb_kernel, dim3((unsigned)(S * NT)), dim3(RNT), 0, (hipStream_t)stream, table, images, L, NT);
    return rtfs_launch_status();
}

int rtfs_mix_reverb_plan(const long long* slots, const double* a, const long long* rirs, int B, int L, int n_out, long long images,
                         long long* table, int* n_images, size_t* ws_bytes, int* refused) {
    if (!rirs) return reverb_refuse(refused, -1, RTFS_MIX_BAD_ARGUMENT);
    size_t ws = 0;
    int code = rtfs_mix_plan(slots, a, B, L, n_out, nullptr, &ws, refused);  // every refusal of the dry recipe, in its order
    if (code != RTFS_OK) return code;
    if (images & 3) return reverb_refuse(refused, -1, RTFS_MIX_MISALIGNED);
    // one image per distinct (source, dtype, start, RIR, taps, offset), numbered in the order slots name them: segment, then reference
    std::map<std::array<long long, 6>, int> seen;
    std::vector<long long> jobs, patched(slots, slots + (size_t)B * MJ * RTFS_MIX_RECIPE_WORDS);
    for (long long idx = 0; idx < (long long)B * MJ; ++idx) {
        const long long* w = slots + idx * RTFS_MIX_RECIPE_WORDS;
        const long long* r = rirs + idx * RTFS_MIX_RIR_WORDS;
        if (!w[0]) continue;
        for (int h = 0; h < 2; ++h) {
            if (!w[4 * h] || !r[3 * h]) continue;  // no reference | dry
            const long long rec[RR] = {w[4 * h], w[4 * h + 1], w[4 * h + 2], w[4 * h + 3], r[3 * h], r[3 * h + 1], r[3 * h + 2]};
            const int reason = reverb_job_reason(rec, L);
            if (reason) return reverb_refuse(refused, idx, reason);
            const std::array<long long, 6> key = {rec[0], rec[2], rec[3], rec[4], rec[5], rec[6]};
            auto it = seen.find(key);
            if (it == seen.end()) {
                it = seen.emplace(key, (int)seen.size()).first;
                jobs.insert(jobs.end(), rec, rec + RR);
            }
            long long* p = patched.data() + idx * RTFS_MIX_RECIPE_WORDS + 4 * h;  // the image row as a float32 source of L samples
            p[0] = images + (long long)it->second * L * 4;
            p[1] = L;
            p[2] = RTFS_MIX_F32;
            p[3] = 0;
        }
    }
    const long long S = (long long)seen.size();
    if (S && !reverb_sizes_ok(S, L)) return reverb_refuse(refused, -1, RTFS_MIX_BAD_ARGUMENT);
    if (table && S && !images) return reverb_refuse(refused, -1, RTFS_MIX_BAD_ARGUMENT);
    if (table) {
        for (long long s = 0; s < S; ++s) reverb_job_write(jobs.data() + s * RR, table + s * RW);
        code = rtfs_mix_plan(patched.data(), a, B, L, n_out, table + S * RW, nullptr, refused);
        if (code != RTFS_OK) return code;
    }
    if (n_images) *n_images = (int)S;
    if (ws_bytes) *ws_bytes = ws;
    return RTFS_OK;
}

int rtfs_mix_reverb_f32(const long long* table, int n_images, float* images, float* mixture, float* sources, double* stats, int B, int L,
                        int n_out, int normalize, double eps, void* ws, size_t ws_bytes, void* stream) {
    if (!table || !mixture || !stats || !ws || n_images < 0 || (n_images && !images)) return RTFS_ERR_ARG;
    if (L < 1 || L > RTFS_MIX_MAX_LENGTH || (n_images && !reverb_sizes_ok(n_images, L)) || n_out < 0 || n_out > MJ) return RTFS_ERR_SHAPE;
    if (n_out > 0 && !sources) return RTFS_ERR_ARG;
    const size_t need = rtfs_mix_workspace_bytes(B, L);
    if (!need) return RTFS_ERR_SHAPE;
    if (ws_bytes < need) return RTFS_ERR_WORKSPACE;
    if (((((uintptr_t)table) | ((uintptr_t)stats) | ((uintptr_t)ws)) & 7) ||
        ((((uintptr_t)mixture) | ((uintptr_t)sources) | ((uintptr_t)images)) & 3))
        return RTFS_ERR_ARG;
    if (n_images) {
        const int e = rtfs_reverb_f32(table, images, n_images, L, stream);
        if (e != RTFS_OK) return e;
    }
    return rtfs_mix_f32(table + (size_t)n_images * RW, mixture, sources, stats, B, L, n_out, normalize, eps, ws, ws_bytes, stream);
}

}  // extern "C"
