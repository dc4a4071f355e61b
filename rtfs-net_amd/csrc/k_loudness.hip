// ITU-R BS.1770 integrated loudness on the device (rtfs-net_amd/datas.py loudness / loudness_many / loudness_normalize; DESIGN.md
// "Loudness"; the definition stands in include/rtfs_amd.h): K-weighting, 400 ms blocks, two gates, for a pool of R mono recordings of
// different lengths, float32 or int16 PCM read where they lie, as one planned call of four launches.
//   rtfs_loudness_plan    host only: validates the pool, designs the filter for fs (loudness.h) and writes the ONE table
//   loud_ends_kernel      one wave per (recording, hop of H = fs / 10 samples): every lane runs its piece of the hop through the
//                         cascade from ZERO state; the piece end states are combined across the lanes with A^p into the hop's end state
//   loud_scan_kernel      one thread per recording: the hop end states combined along the recording with A^H -> every hop's start state
//   loud_energy_kernel    one wave per (recording, hop): the lanes' true start states from the hop's, then the second sweep over the
//                         samples (they sit in the memory-side cache) with the true states: E_h = sum y^2
//   loud_gate_kernel      one workgroup per recording: block energies z, both gates in the z domain, lufs and kept
//   loud_gain_kernel      (rtfs_loudness_gain_f32) out = (float)(x g), g = 10^((target - lufs) / 20) formed on the device
// The recurrence is linear: s' = A s + B x, y = C s + D x over the state s = (z1, z2, w1, w2) of two transposed direct form II biquads.
// A piece of n samples run from zero state ends in e; from state s it ends in A^n s + e.  That is all the stitching uses, and the
// energies are NOT expanded around it: the second sweep runs the plain recurrence from the true state, so a large DC offset that the
// high-pass cancels costs no digits.  tests/loudness_oracle.py restates every step in float64 numpy and measures it against an
// 80-bit run of the plain recurrence.  All arithmetic is IEEE float64 multiply, add, subtract, divide in a fixed order without fused
// multiply-add (contraction is off for the file, as k_mix.hip); no atomics, one writer per cell, nothing read back: the same inputs give
// the same bits, and a recording's result does not depend on what else is in the pool.
#pragma clang fp contract(off)
#include <math.h>
#include <string.h>

#include "../../include/rtfs_amd.h"
#include "common.h"
#include "loudness.h"

namespace {

constexpr int LN = RTFS_LOUD_LANES;
constexpr int HW = RTFS_LOUD_HEADER_WORDS;
constexpr int TW = RTFS_LOUD_TABLE_WORDS;
constexpr int GCHUNK = RTFS_LOUD_CHUNK;
static_assert(LN == 64, "one wave per hop");
// header words: [fs | H | p | R | hops | blocks | samples | chunks | b0 b1 b2 a1 a2 c1 c2 (8..14) | absolute gate (15) | A^p (16..31) |
//                A^q (32..47), q the length of the one ragged piece | A^H (48..63)]
// record words: [address | L | is int16 | hops | first hop | first sample | first chunk | first block]
enum { H_FS, H_H, H_P, H_R, H_HOPS, H_BLOCKS, H_SAMPLES, H_CHUNKS, H_COEF, H_GATE = 15, H_AP = 16, H_AQ = 32, H_AH = 48 };
enum { T_ADDR, T_LEN, T_I16, T_HOPS, T_HOP0, T_SMP0, T_CHUNK0, T_BLK0 };

__device__ __forceinline__ double loud_hd(const long long* __restrict__ table, int w) { return __longlong_as_double(table[w]); }

// the recording whose [first, next first) range of the given prefix word holds g: every recording has at least one hop, block and chunk
__device__ __forceinline__ int loud_find(const long long* __restrict__ table, int R, int word, long long g) {
    int lo = 0, hi = R - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[HW + (size_t)mid * TW + word] <= g)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// sample i of a recording: float32 as it lies, int16 PCM as (float)s / 32768 (exact)
__device__ __forceinline__ double loud_ld(const char* p, int i16, long long i) {
    return i16 ? (double)((float)((const short*)p)[i] * (1.0f / 32768.0f)) : (double)((const float*)p)[i];
}

struct LoudCoef {
    double b0, b1, b2, a1, a2, c1, c2;
};
__device__ __forceinline__ LoudCoef loud_coef(const long long* __restrict__ table) {
    LoudCoef c;
    c.b0 = loud_hd(table, H_COEF), c.b1 = loud_hd(table, H_COEF + 1), c.b2 = loud_hd(table, H_COEF + 2);
    c.a1 = loud_hd(table, H_COEF + 3), c.a2 = loud_hd(table, H_COEF + 4), c.c1 = loud_hd(table, H_COEF + 5), c.c2 = loud_hd(table, H_COEF + 6);
    return c;
}

// one sample through the cascade; returns y
__device__ __forceinline__ double loud_step(const LoudCoef& c, double x, double (&s)[4]) {
    const double v = c.b0 * x + s[0];
    s[0] = (c.b1 * x - c.a1 * v) + s[1];
    s[1] = c.b2 * x - c.a2 * v;
    const double y = v + s[2];
    s[2] = (-2.0 * v - c.c1 * y) + s[3];
    s[3] = v - c.c2 * y;
    return y;
}

// samples [lo, hi) of a hop that starts at sample `at` through the cascade, in order; use(y) sees every output.  The loads do not depend
// on the state, so they go out eight at a time in front of the eight dependent steps (one load per step leaves a wave waiting on
// memory 25 to 300 times a piece); the arithmetic and its order are those of the plain loop.
template <class F>
__device__ __forceinline__ void loud_sweep(const LoudCoef& c, const char* x, int i16, long long at, int lo, int hi, double (&s)[4], F use) {
    int i = lo;
    for (; i + 8 <= hi; i += 8) {
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = loud_ld(x, i16, at + i + k);
#pragma unroll
        for (int k = 0; k < 8; ++k) use(loud_step(c, v[k], s));
    }
    for (; i < hi; ++i) use(loud_step(c, loud_ld(x, i16, at + i), s));
}

// s <- M s + e, rows left to right
__device__ __forceinline__ void loud_advance(const double (&M)[16], const double (&e)[4], double (&s)[4]) {
    double r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (((M[4 * i] * s[0] + M[4 * i + 1] * s[1]) + M[4 * i + 2] * s[2]) + M[4 * i + 3] * s[3]) + e[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = r[i];
}

// the lanes' pieces of a hop: lane l takes [min(l p, H), min((l + 1) p, H)), p = ceil(H / 64); the lanes behind the ragged one are empty.
// Walks the pieces in order from state s (uniform in the wave) with the lanes' zero-state ends e; lane `lane` keeps the state at the
// start of its own piece in `mine`; s ends as the state behind the hop.
__device__ __forceinline__ void loud_lane_scan(const long long* __restrict__ table, int H, int p, const double (&e)[4], int lane, double (&s)[4],
                                               double (&mine)[4]) {
    double Ap[16], Aq[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) Ap[i] = loud_hd(table, H_AP + i), Aq[i] = loud_hd(table, H_AQ + i);
    for (int l = 0; l < LN; ++l) {
        const int n = min(p, H - l * p);  // uniform
        if (n <= 0) break;
        if (l == lane) {
#pragma unroll
            for (int i = 0; i < 4; ++i) mine[i] = s[i];
        }
        double el[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) el[i] = __shfl(e[i], l, 64);
        if (n == p)
            loud_advance(Ap, el, s);
        else
            loud_advance(Aq, el, s);
    }
}

// ---------------------------------------------------------------- launch 1
// ws: lane ends (hops, 4, 64) | hop ends (hops, 4) | hop starts (hops, 4) | hop energies (hops)
__global__ __launch_bounds__(64) void loud_ends_kernel(const long long* __restrict__ table, double* __restrict__ lane_e, double* __restrict__ hop_e) {
    const int lane = threadIdx.x;
    const int R = (int)table[H_R], H = (int)table[H_H], p = (int)table[H_P];
    const long long g = blockIdx.x;
    const long long* rec = table + HW + (size_t)loud_find(table, R, T_HOP0, g) * TW;
    const char* x = (const char*)(uintptr_t)rec[T_ADDR];
    const int i16 = (int)rec[T_I16];
    const long long at = (g - rec[T_HOP0]) * H;
    const LoudCoef c = loud_coef(table);
    const int lo = min(lane * p, H), hi = min(lo + p, H);
    double e[4] = {0.0, 0.0, 0.0, 0.0};
    loud_sweep(c, x, i16, at, lo, hi, e, [](double) {});
#pragma unroll
    for (int i = 0; i < 4; ++i) lane_e[((size_t)g * 4 + i) * LN + lane] = e[i];
    double s[4] = {0.0, 0.0, 0.0, 0.0}, mine[4] = {0.0, 0.0, 0.0, 0.0};
    loud_lane_scan(table, H, p, e, lane, s, mine);
    if (lane < 4) hop_e[(size_t)g * 4 + lane] = lane == 0 ? s[0] : (lane == 1 ? s[1] : (lane == 2 ? s[2] : s[3]));
}

// ---------------------------------------------------------------- launch 2
__global__ __launch_bounds__(64) void loud_scan_kernel(const long long* __restrict__ table, const double* __restrict__ hop_e, double* __restrict__ hop_s) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= (int)table[H_R]) return;
    const long long* rec = table + HW + (size_t)r * TW;
    double AH[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) AH[i] = loud_hd(table, H_AH + i);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const long long h0 = rec[T_HOP0], nh = rec[T_HOPS];
    for (long long h = h0; h < h0 + nh; h += 8) {  // the ends of eight hops are loaded in front of the eight dependent steps
        const int n = (int)min(8LL, h0 + nh - h);
        double e[8][4];
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int i = 0; i < 4; ++i) e[k][i] = k < n ? hop_e[(size_t)(h + k) * 4 + i] : 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k >= n) break;
#pragma unroll
            for (int i = 0; i < 4; ++i) hop_s[(size_t)(h + k) * 4 + i] = s[i];
            loud_advance(AH, e[k], s);
        }
    }
}

// ---------------------------------------------------------------- launch 3
__global__ __launch_bounds__(64) void loud_energy_kernel(const long long* __restrict__ table, const double* __restrict__ lane_e,
                                                          const double* __restrict__ hop_s, double* __restrict__ hop_E) {
    const int lane = threadIdx.x;
    const int R = (int)table[H_R], H = (int)table[H_H], p = (int)table[H_P];
    const long long g = blockIdx.x;
    const long long* rec = table + HW + (size_t)loud_find(table, R, T_HOP0, g) * TW;
    const char* x = (const char*)(uintptr_t)rec[T_ADDR];
    const int i16 = (int)rec[T_I16];
    const long long at = (g - rec[T_HOP0]) * H;
    const LoudCoef c = loud_coef(table);
    double e[4], s[4], mine[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        e[i] = lane_e[((size_t)g * 4 + i) * LN + lane];
        s[i] = hop_s[(size_t)g * 4 + i];
    }
    loud_lane_scan(table, H, p, e, lane, s, mine);
    const int lo = min(lane * p, H), hi = min(lo + p, H);
    double acc = 0.0;
    loud_sweep(c, x, i16, at, lo, hi, mine, [&](double y) { acc += y * y; });
    acc = wave_sum_d(acc);
    if (lane == 0) hop_E[g] = acc;
}

// ---------------------------------------------------------------- launch 4
// block j of a recording: z = (((E_j + E_{j+1}) + E_{j+2}) + E_{j+3}) / (4 H)
__device__ __forceinline__ double loud_block(const double* __restrict__ E, long long j, double n) { return (((E[j] + E[j + 1]) + E[j + 2]) + E[j + 3]) / n; }

// (a, b) summed over the workgroup in a fixed order: lanes by butterfly, then the four waves
__device__ __forceinline__ void loud_block_sum(double& a, double& b, double (*red)[2]) {
    a = wave_sum_d(a), b = wave_sum_d(b);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = a, red[threadIdx.x >> 6][1] = b;
    __syncthreads();
    a = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    b = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
}

__global__ __launch_bounds__(256) void loud_gate_kernel(const long long* __restrict__ table, const double* __restrict__ hop_E, double* __restrict__ out,
                                                         double* __restrict__ z_out) {
    __shared__ double red[4][2];
    const int tid = threadIdx.x, r = blockIdx.x;
    const long long* rec = table + HW + (size_t)r * TW;
    const double* E = hop_E + rec[T_HOP0];
    const long long nb = rec[T_HOPS] - 3;
    const double n = (double)(4 * table[H_H]), gate = loud_hd(table, H_GATE);
    double sum = 0.0, cnt = 0.0;
    int bad = 0;
    for (long long j = tid; j < nb; j += 256) {
        const double z = loud_block(E, j, n);
        if (z_out) z_out[rec[T_BLK0] + j] = z;
        bad |= !(fabs(z) <= 1.7976931348623157e308);  // inf or NaN
        if (z > gate) sum += z, cnt += 1.0;
    }
    double nbad = (double)bad;
    loud_block_sum(sum, cnt, red);
    const double rel = 0.1 * (sum / cnt);  // cnt = 0: NaN, and no block passes below
    double sum2 = 0.0, cnt2 = 0.0;
    for (long long j = tid; j < nb; j += 256) {
        const double z = loud_block(E, j, n);
        if (z > gate && z > rel) sum2 += z, cnt2 += 1.0;
    }
    loud_block_sum(sum2, cnt2, red);
    double dummy = 0.0;
    loud_block_sum(nbad, dummy, red);
    if (tid == 0) {
        double lufs = cnt2 > 0.0 ? -0.691 + 10.0 * log10(sum2 / cnt2) : -(double)INFINITY;
        if (nbad > 0.0) lufs = __builtin_nan("");
        out[2 * (size_t)r] = lufs;
        out[2 * (size_t)r + 1] = nbad > 0.0 ? 0.0 : cnt2;
    }
}

// ---------------------------------------------------------------- the gain launch
__global__ __launch_bounds__(256) void loud_gain_kernel(const long long* __restrict__ table, const double* __restrict__ loud, double target,
                                                         float* __restrict__ out, double* __restrict__ stats) {
    const int tid = threadIdx.x;
    const int R = (int)table[H_R];
    const long long g = blockIdx.x;
    const int r = loud_find(table, R, T_CHUNK0, g);
    const long long* rec = table + HW + (size_t)r * TW;
    const char* x = (const char*)(uintptr_t)rec[T_ADDR];
    const int i16 = (int)rec[T_I16];
    const long long c = g - rec[T_CHUNK0], lo = c * GCHUNK, L = rec[T_LEN];
    const int n = (int)min((long long)GCHUNK, L - lo);
    const double lufs = loud[2 * (size_t)r];
    const double gain = fabs(lufs) <= 1.7976931348623157e308 ? exp10((target - lufs) / 20.0) : 1.0;
    if (c == 0 && tid == 0) stats[r] = gain;
    float* y = out + rec[T_SMP0] + lo;
    for (int i = tid; i < n; i += 256) y[i] = (float)(loud_ld(x, i16, lo + i) * gain);
}

int loud_refuse(int* refused, long long where, int reason) {
    if (refused) {
        refused[0] = (int)where;
        refused[1] = reason;
    }
    return RTFS_ERR_ARG;
}

bool loud_rate_ok(int fs) { return fs >= RTFS_LOUD_MIN_RATE && fs <= RTFS_LOUD_MAX_RATE && fs % 10 == 0; }

// what the launches take from the HOST copy of the table: sizes only, checked against what a plan can have written
bool loud_header_ok(const long long* t) {
    return t[H_R] >= 1 && t[H_R] <= 0x7fffffffLL && loud_rate_ok((int)t[H_FS]) && t[H_H] * 10 == t[H_FS] && t[H_HOPS] >= 4 * t[H_R] &&
           t[H_HOPS] <= 0x7fffffffLL && t[H_CHUNKS] >= t[H_R] && t[H_CHUNKS] <= 0x7fffffffLL && t[H_BLOCKS] == t[H_HOPS] - 3 * t[H_R];
}

size_t loud_ws_bytes(long long hops) { return (size_t)hops * (4 * LN + 4 + 4 + 1) * sizeof(double); }

}  // namespace

extern "C" {

int rtfs_loudness_design(int fs, double* coef) {
    if (!loud_rate_ok(fs) || !coef) return RTFS_ERR_ARG;
    const LoudFilter f = loud_design(fs);
    const double v[8] = {f.b0, f.b1, f.b2, f.a1, f.a2, f.c1, f.c2, loud_abs_gate()};
    memcpy(coef, v, sizeof(v));
    return RTFS_OK;
}

int rtfs_loudness_plan(const long long* recs, int R, int fs, long long* table, size_t* ws_bytes, long long* totals, int* refused) {
    if (!recs || R < 1) return loud_refuse(refused, -1, RTFS_LOUD_BAD_ARGUMENT);
    if (!loud_rate_ok(fs)) return loud_refuse(refused, -1, RTFS_LOUD_BAD_RATE);
    const long long H = fs / 10;
    long long hops = 0, samples = 0, chunks = 0;
    for (int r = 0; r < R; ++r) {
        const long long* w = recs + (size_t)r * RTFS_LOUD_RECORD_WORDS;
        const long long addr = w[0], len = w[1], dt = w[2];
        if (!addr) return loud_refuse(refused, r, RTFS_LOUD_BAD_ARGUMENT);
        if (dt != RTFS_MIX_F32 && dt != RTFS_MIX_I16) return loud_refuse(refused, r, RTFS_LOUD_BAD_DTYPE);
        if (addr & (dt == RTFS_MIX_F32 ? 3 : 1)) return loud_refuse(refused, r, RTFS_LOUD_MISALIGNED);
        if (len < 4 * H) return loud_refuse(refused, r, RTFS_LOUD_TOO_SHORT);
        if (len > RTFS_LOUD_MAX_LENGTH) return loud_refuse(refused, r, RTFS_LOUD_TOO_LONG);
        hops += len / H;
        samples += len;
        chunks += (len + GCHUNK - 1) / GCHUNK;
    }
    if (hops > 0x7fffffffLL || chunks > 0x7fffffffLL) return loud_refuse(refused, -1, RTFS_LOUD_BAD_ARGUMENT);
    if (ws_bytes) *ws_bytes = loud_ws_bytes(hops);
    if (totals) totals[0] = hops, totals[1] = hops - 3LL * R, totals[2] = samples, totals[3] = chunks;
    if (table) {
        const long long p = (H + LN - 1) / LN, q = H % p;  // q = 0: no ragged piece, A^q is never used
        const LoudFilter f = loud_design(fs);
        table[H_FS] = fs, table[H_H] = H, table[H_P] = p, table[H_R] = R;
        table[H_HOPS] = hops, table[H_BLOCKS] = hops - 3LL * R, table[H_SAMPLES] = samples, table[H_CHUNKS] = chunks;
        const double coef[8] = {f.b0, f.b1, f.b2, f.a1, f.a2, f.c1, f.c2, loud_abs_gate()};
        memcpy(table + H_COEF, coef, sizeof(coef));
        double M[16];
        loud_power(f, p, M);
        memcpy(table + H_AP, M, sizeof(M));
        loud_power(f, q, M);
        memcpy(table + H_AQ, M, sizeof(M));
        loud_power(f, H, M);
        memcpy(table + H_AH, M, sizeof(M));
        long long hop = 0, smp = 0, chunk = 0, blk = 0;
        for (int r = 0; r < R; ++r) {
            const long long* w = recs + (size_t)r * RTFS_LOUD_RECORD_WORDS;
            long long* t = table + HW + (size_t)r * TW;
            const long long nh = w[1] / H;
            t[T_ADDR] = w[0], t[T_LEN] = w[1], t[T_I16] = w[2] == RTFS_MIX_I16 ? 1 : 0, t[T_HOPS] = nh;
            t[T_HOP0] = hop, t[T_SMP0] = smp, t[T_CHUNK0] = chunk, t[T_BLK0] = blk;
            hop += nh, smp += w[1], chunk += (w[1] + GCHUNK - 1) / GCHUNK, blk += nh - 3;
        }
    }
    return RTFS_OK;
}

int rtfs_loudness_f32(const long long* table, const long long* host_table, double* out, double* z, void* ws, size_t ws_bytes, void* stream) {
    if (!table || !host_table || !out || !ws) return RTFS_ERR_ARG;
    if (!loud_header_ok(host_table)) return RTFS_ERR_SHAPE;
    const long long hops = host_table[H_HOPS];
    const int R = (int)host_table[H_R];
    if (ws_bytes < loud_ws_bytes(hops)) return RTFS_ERR_WORKSPACE;
    if ((((uintptr_t)table) | ((uintptr_t)out) | ((uintptr_t)z) | ((uintptr_t)ws)) & 7) return RTFS_ERR_ARG;
    double* lane_e = (double*)ws;
    double* hop_e = lane_e + (size_t)hops * 4 * LN;
    double* hop_s = hop_e + (size_t)hops * 4;
    double* hop_E = hop_s + (size_t)hops * 4;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(loud_ends_kernel, dim3((unsigned)hops), dim3(64), 0, st, table, lane_e, hop_e);
    int e = rtfs_launch_status();
    if (e != RTFS_OK) return e;
    hipLaunchKernelGGL(loud_scan_kernel, dim3((unsigned)cdiv(R, 64)), dim3(64), 0, st, table, (const double*)hop_e, hop_s);
    if ((e = rtfs_launch_status()) != RTFS_OK) return e;
    hipLaunchKernelGGL(loud_energy_kernel, dim3((unsigned)hops), dim3(64), 0, st, table, (const double*)lane_e, (const double*)hop_s, hop_E);
    if ((e = rtfs_launch_status()) != RTFS_OK) return e;
    hipLaunchKernelGGL(loud_gate_kernel, dim3((unsigned)R), dim3(256), 0, st, table, (const double*)hop_E, out, z);
    return rtfs_launch_status();
}

int rtfs_loudness_gain_f32(const long long* table, const long long* host_table, const double* loud, double target, float* out, double* stats,
                           void* stream) {
    if (!table || !host_table || !loud || !out || !stats) return RTFS_ERR_ARG;
    if (!loud_header_ok(host_table)) return RTFS_ERR_SHAPE;
    if (((((uintptr_t)table) | ((uintptr_t)loud) | ((uintptr_t)stats)) & 7) || (((uintptr_t)out) & 3)) return RTFS_ERR_ARG;
    hipLaunchKernelGGL(loud_gain_kernel, dim3((unsigned)host_table[H_CHUNKS]), dim3(256), 0, (hipStream_t)stream, table, loud, target, out, stats);
    return rtfs_launch_status();
}

}  // extern "C"
