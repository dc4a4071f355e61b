// Preparing raw recordings on the device (rtfs-net_amd/datas.py; DESIGN.md "Preparing recordings"): what the reference does on the host in
// front of the model inputs (src/datas/transform.py:151-167, avspeech_dataset.py:18-22, infer_any_video.py:63-80).
//   lips_prepare_kernel     uint8 mouth ROIs (N,Tv,H,W) -> float32 lips (N,1,Tv,88,88): scale, crop, flip, normalise, one launch; its RATE
//                           form also selects the frames of a track at another frame rate (frame_rate.h): output frame p reads c(p)
//   wavnorm_stats_kernel    per-chunk (sum, sum of squares) of every mixture / source row in float64, shifted by the row's first sample
//   wavnorm_apply_kernel    every workgroup re-reduces its row's partials in a fixed order, then (x - mean) / (std_mix + eps)
//   resample_kernel         polyphase FIR with torchaudio's Hann-windowed sinc bank; bank rows and the input segment resident in LDS
// tests/prep_oracle.py restates the three in float64 numpy.  All run on the caller's stream, allocate nothing, read nothing back and use no
// atomics: one writer per output element and fixed reduction orders, so results are deterministic and a call is graph-capturable.
#include <math.h>

#include "../../include/rtfs_amd.h"
#include "common.h"
#include "frame_rate.h"
#include "kernels.h"

namespace {

// ================================================================ lips
constexpr int CROP = 88;                        // the reference's crop_size (transform.py:155)
constexpr int IMG_QUADS = CROP * CROP / 4;      // 1936 output quads per frame; 88 % 4 == 0, so a quad never crosses a row
constexpr int LIPS_TRACKS = RTFS_LIPS_MAX_TRACKS_PER_LAUNCH;

// (dy, dx, flip) of every track of the launch BY VALUE, packed dy | dx << 15 | flip << 30 (checked on the host: 0 <= dy, dx < 2^15)
struct LipsTable {
    unsigned v[LIPS_TRACKS];
};

// One workgroup per frame.  The 256 possible values go through the reference's float64 arithmetic once per workgroup into an LDS table.
// A lane produces 4 adjacent output pixels: it reads the (at most two) ALIGNED dwords that hold its 4 source bytes and funnel-shifts
// them together (dx is arbitrary, so row starts are not aligned); a dword that holds a byte of the ROI tensor lies in the same page as
// that byte.  Stores: 16 bytes per lane, 1024 contiguous bytes per wave; a frame is 30976 bytes = 242 whole 128-byte lines.
// RATE: the track holds Tv_in camera frames at a / b fps and output frame t of its Tv reads camera frame c(t) < Tv_in (block-uniform).
template <bool RATE>
__global__ __launch_bounds__(256) void lips_prepare_kernel(const unsigned char* __restrict__ roi, LipsTable tab, float* __restrict__ out,
                                                            int track0, int Tv, int H, int W, double mean, double stdv, int Tv_in,
                                                            long long a, long long b) {
    __shared__ float lut[256];
    const int tid = threadIdx.x;
    lut[tid] = (float)((((double)tid - 0.0) / 255.0 - mean) / stdv);
    __syncthreads();
    const int nl = blockIdx.x / Tv, t = blockIdx.x - nl * Tv;
    const unsigned e = tab.v[nl];
    const int dy = e & 0x7fff, dx = (e >> 15) & 0x7fff;
    const bool flip = (e >> 30) & 1;
    const size_t img = (size_t)(track0 + nl) * Tv + t;
    const size_t img_in = RATE ? (size_t)(track0 + nl) * Tv_in + (size_t)fr_source(a, b, t) : img;
    const unsigned char* src = roi + img_in * H * W + (size_t)dy * W + dx;
    float* dst = out + img * (CROP * CROP);
    for (int q = tid; q < IMG_QUADS; q += 256) {
        const int y = q / (CROP / 4), x0 = 4 * (q - y * (CROP / 4));
        const unsigned char* p = src + (size_t)y * W + (flip ? CROP - 4 - x0 : x0);  // first of the 4 source bytes
        const uintptr_t a = (uintptr_t)p;
        const unsigned sh = (unsigned)(a & 3);
        const unsigned* ap = (const unsigned*)(a - sh);
        unsigned w = ap[0];
        if (sh) w = (unsigned)((((unsigned long long)ap[1] << 32) | w) >> (8 * sh));
        if (flip) w = __builtin_bswap32(w);
        *(f32x4*)(dst + 4 * q) = f32x4{lut[w & 255], lut[(w >> 8) & 255], lut[(w >> 16) & 255], lut[w >> 24]};
    }
}

// ================================================================ waveform normalisation
constexpr int WN_CHUNK = 16384;  // floats per workgroup: 64 KB in, 64 KB out

__device__ __forceinline__ void block_sum2_d(double& a, double& b, double* red, int tid) {
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    __syncthreads();
    if ((tid & 63) == 0) {
        red[2 * (tid >> 6)] = a;
        red[2 * (tid >> 6) + 1] = b;
    }
    __syncthreads();
    a = (red[0] + red[2]) + (red[4] + red[6]);
    b = (red[1] + red[3]) + (red[5] + red[7]);
}

// row r < B: mixture row r; row r >= B: source row r - B of (B*K, L)
__device__ __forceinline__ const float* wn_row(const float* mix, const float* src, int B, int L, int r) {
    return r < B ? mix + (size_t)r * L : src + (size_t)(r - B) * L;
}

__global__ __launch_bounds__(256) void wavnorm_stats_kernel(const float* __restrict__ mix, const float* __restrict__ src, double* __restrict__ part,
                                                             int B, int L, int NC) {
    __shared__ double red[8];
    const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const float* x = wn_row(mix, src, B, L, r);
    const double x0 = (double)x[0];  // the shift: sums of deviations from the first sample keep a large DC offset out of the squares
    const int lo = c * WN_CHUNK, n = min(WN_CHUNK, L - lo);
    x += lo;
    double s = 0.0, ss = 0.0;
    const int n4 = (((uintptr_t)x) & 15) == 0 ? n >> 2 : 0;
    for (int i = tid; i < n4; i += 256) {
        const f32x4 v = *(const f32x4*)(x + 4 * i);
        const double d0 = (double)v.x - x0, d1 = (double)v.y - x0, d2 = (double)v.z - x0, d3 = (double)v.w - x0;
        s += (d0 + d1) + (d2 + d3);
        ss += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
    for (int i = 4 * n4 + tid; i < n; i += 256) {
        const double d = (double)x[i] - x0;
        s += d;
        ss += d * d;
    }
    block_sum2_d(s, ss, red, tid);
    if (tid == 0) {
        part[2 * ((size_t)r * NC + c)] = s;
        part[2 * ((size_t)r * NC + c) + 1] = ss;
    }
}

__global__ __launch_bounds__(256) void wavnorm_apply_kernel(const float* __restrict__ mix, const float* __restrict__ src,
                                                             const float* __restrict__ std_in, const double* __restrict__ part,
                                                             float* __restrict__ mix_out, float* __restrict__ src_out, int B, int K, int L, int NC,
                                                             double eps) {
    __shared__ double red[8];
    const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const int b = r < B ? r : (r - B) / K;  // the mixture whose deviation scales this row
    // own row: sum -> mean; mixture row b: sum and sum of squares -> unbiased std.  Every workgroup of a row sums the same partials in
    // the same order (thread tid: tid, tid + 256, ...; then lanes, then waves), so all of them apply the same two constants.
    double s = 0.0, sm = 0.0, ssm = 0.0;
    for (int i = tid; i < NC; i += 256) {
        s += part[2 * ((size_t)r * NC + i)];
        sm += part[2 * ((size_t)b * NC + i)];
        ssm += part[2 * ((size_t)b * NC + i) + 1];
    }
    double dummy = 0.0;
    block_sum2_d(s, dummy, red, tid);
    block_sum2_d(sm, ssm, red, tid);
    const float* x = wn_row(mix, src, B, L, r);
    const double mean = (double)x[0] + s / (double)L;
    double sd;
    if (std_in) {
        sd = (double)std_in[b];
    } else {
        sd = sqrt((ssm - sm * sm / (double)L) / (double)(L - 1));  // L = 1: 0 / 0 = NaN, as torch.std
    }
    const double inv = 1.0 / (sd + eps);
    float* y = r < B ? mix_out + (size_t)r * L : src_out + (size_t)(r - B) * L;
    const int lo = c * WN_CHUNK, n = min(WN_CHUNK, L - lo);
    x += lo;
    y += lo;
    const int n4 = ((((uintptr_t)x) | ((uintptr_t)y)) & 15) == 0 ? n >> 2 : 0;
    for (int i = tid; i < n4; i += 256) {
        const f32x4 v = *(const f32x4*)(x + 4 * i);
        *(f32x4*)(y + 4 * i) = f32x4{(float)(((double)v.x - mean) * inv), (float)(((double)v.y - mean) * inv),
                                     (float)(((double)v.z - mean) * inv), (float)(((double)v.w - mean) * inv)};
    }
    for (int i = 4 * n4 + tid; i < n; i += 256) y[i] = (float)(((double)x[i] - mean) * inv);
}

// ================================================================ resampling
constexpr int RS_MAX = RTFS_RESAMPLE_MAX_RATIO;  // reduced orig, new <= 640
constexpr int RS_XSEG = 16384;                   // floats of input one tile may stage (a tile of one frame at 640:1 needs 8398)
constexpr int RS_TILE_OUT = 2048;                // outputs per tile when the input segment allows

struct RsPlan {
    int o, n, width, taps, span;  // span = 2 width + 1: the taps of a phase that can be non-zero, from tap floor(o p / n) on
    int jf;                       // frames per tile
    size_t lds;
};

int rs_gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

int rs_plan(int orig, int neu, RsPlan& P) {
    if (orig < 1 || neu < 1) return RTFS_ERR_ARG;
    const int g = rs_gcd(orig, neu);
    P.o = orig / g;
    P.n = neu / g;
    if (P.o > RS_MAX || P.n > RS_MAX) return RTFS_ERR_ARG;
    const double base = (double)(P.o < P.n ? P.o : P.n) * 0.99;
    P.width = (int)ceil(6.0 * (double)P.o / base);
    P.taps = 2 * P.width + P.o;
    P.span = 2 * P.width + 1;
    int jf = (RS_XSEG - 2 * P.width) / P.o;
    const int cap = RS_TILE_OUT / P.n;
    if (jf > cap) jf = cap;
    P.jf = jf < 1 ? 1 : jf;
    P.lds = ((size_t)P.n * P.span + (size_t)P.n + (size_t)P.jf * P.o + 2 * (size_t)P.width) * sizeof(float);
    return RTFS_OK;
}

// bank[p, k] in float64, torchaudio's order of operations (functional._get_sinc_resample_kernel, "sinc_interp_hann", width 6, rolloff 0.99)
float rs_tap(const RsPlan& P, int p, int k) {
    const double base = (double)(P.o < P.n ? P.o : P.n) * 0.99;
    double t = (-(double)p / (double)P.n + (double)(k - P.width) / (double)P.o) * base;
    t = t < -6.0 ? -6.0 : (t > 6.0 ? 6.0 : t);
    const double c = cos(t * M_PI / 6.0 / 2.0);
    const double win = c * c;
    const double tp = t * M_PI;
    const double scale = base / (double)P.o;
    const double sinc = tp == 0.0 ? 1.0 : sin(tp) / tp;
    return (float)(sinc * (win * scale));
}

// y[j n + p] = sum_s bank[p, c(p) + s] * x[j o + c(p) + s - width], c(p) = floor(o p / n), s in [0, span): the other taps of row p are
// exact float32 zeros (the clip of t to +-6 puts them on the window's zero; rtfs_resample_plan verifies it when it builds a bank).
// A workgroup copies the n x span non-zero bank (<= 41 KB) and c(p) into LDS once, then walks tiles of `jf` frames: it stages the tile's
// input segment [j0 o - width, (j0 + jf) o + width) in LDS with the recording's zero padding as predicates, and every thread forms
// outputs j0 n + tid, + 256, ...: adjacent lanes read adjacent bank rows (odd pitch `span`: no bank conflicts) and write adjacent floats.
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ x, const float* __restrict__ bank, float* __restrict__ y, int L,
                                                        int Lout, int o, int n, int width, int taps, int span, int jf, int tiles) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    float* bk = rs_lds;                 // n * span
    int* cp = (int*)(bk + n * span);    // n
    float* xs = (float*)(cp + n);       // jf * o + 2 * width
    const int tid = threadIdx.x;
    for (int p = tid; p < n; p += 256) cp[p] = (o * p) / n;
    for (int i = tid; i < n * span; i += 256) {
        const int p = i / span, s = i - p * span;
        bk[i] = bank[(size_t)p * taps + (o * p) / n + s];
    }
    const float* xr = x + (size_t)blockIdx.y * L;
    float* yr = y + (size_t)blockIdx.y * Lout;
    const int seg = jf * o + 2 * width, outs = jf * n;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long x0 = (long long)tile * jf * o - width;
        __syncthreads();  // the bank is in place / the previous tile's segment is no longer read
        for (int i = tid; i < seg; i += 256) {
            const long long xi = x0 + i;
            xs[i] = xi >= 0 && xi < L ? xr[xi] : 0.f;
        }
        __syncthreads();
        const long long g0 = (long long)tile * outs;
        for (int gl = tid; gl < outs && g0 + gl < Lout; gl += 256) {
            const int jl = gl / n, p = gl - jl * n;
            const float* b = bk + p * span;
            const float* xv = xs + jl * o + cp[p];
            float acc = 0.f;
#pragma unroll 4
            for (int s = 0; s < span; ++s) acc = fmaf(b[s], xv[s], acc);
            yr[g0 + gl] = acc;
        }
    }
}

}  // namespace

// ================================================================ launchers
// a == 0: no selection, Tv frames in and out; otherwise Tv = P(Tv_in) at a / b fps (reduced)
static int launch_lips_prepare_any(const unsigned char* roi, const int* table, float* out, int N, int Tv, int Tv_in, long long a, long long b,
                                   int H, int W, double mean, double stdv, hipStream_t st) {
    if (!roi || !table || !out) return RTFS_ERR_ARG;
    if (N < 1 || Tv < 1 || Tv_in < 1 || (long long)N * Tv_in > 0x7fffffffLL || H < CROP || W < CROP || H > 0x7fff || W > 0x7fff || (long long)N * Tv > 0x7fffffffLL) return RTFS_ERR_SHAPE;
    if (((uintptr_t)out) & 15) return RTFS_ERR_ARG;
    if (!(stdv != 0.0)) return RTFS_ERR_ARG;
    for (int i = 0; i < N; ++i) {  // an offset that leaves the ROI is refused before anything is launched
        const int dy = table[3 * i], dx = table[3 * i + 1], fl = table[3 * i + 2];
        if (dy < 0 || dx < 0 || dy + CROP > H || dx + CROP > W || (fl != 0 && fl != 1)) return RTFS_ERR_ARG;
    }
    for (int t0 = 0; t0 < N; t0 += LIPS_TRACKS) {
        const int nt = N - t0 < LIPS_TRACKS ? N - t0 : LIPS_TRACKS;
        if ((long long)nt * Tv > 0x7fffffffLL) return RTFS_ERR_SHAPE;
        LipsTable tab;
        for (int i = 0; i < LIPS_TRACKS; ++i)
            tab.v[i] = i < nt ? (unsigned)table[3 * (t0 + i)] | ((unsigned)table[3 * (t0 + i) + 1] << 15) | ((unsigned)table[3 * (t0 + i) + 2] << 30)
                              : 0u;
        if (a)
            hipLaunchKernelGGL(lips_prepare_kernel<true>, dim3(nt * Tv), dim3(256), 0, st, roi, tab, out, t0, Tv, H, W, mean, stdv, Tv_in, a, b);
        else
            hipLaunchKernelGGL(lips_prepare_kernel<false>, dim3(nt * Tv), dim3(256), 0, st, roi, tab, out, t0, Tv, H, W, mean, stdv, Tv, 0LL, 0LL);
        const int e = rtfs_launch_status();
        if (e != RTFS_OK) return e;
    }
    return RTFS_OK;
}

int launch_lips_prepare(const unsigned char* roi, const int* table, float* out, int N, int Tv, int H, int W, double mean, double stdv,
                        hipStream_t st) {
    return launch_lips_prepare_any(roi, table, out, N, Tv, Tv, 0, 0, H, W, mean, stdv, st);
}

int launch_lips_prepare_rate(const unsigned char* roi, const int* table, float* out, int N, int Tv_in, int H, int W, double mean, double stdv,
                             int rate_num, int rate_den, hipStream_t st) {
    long long a, b;
    if (!fr_reduce(rate_num, rate_den, &a, &b) || Tv_in < 1) return RTFS_ERR_ARG;
    const long long Tv = fr_count(a, b, Tv_in);
    if (Tv < 1 || Tv > 0x7fffffffLL) return RTFS_ERR_SHAPE;  // a single frame at more than 50 fps shows in no model frame
    return launch_lips_prepare_any(roi, table, out, N, (int)Tv, Tv_in, a, b, H, W, mean, stdv, st);
}

size_t wav_normalize_workspace_bytes(int B, int K, int L) {
    if (B < 1 || K < 0 || L < 1) return 0;
    return (size_t)B * (1 + K) * cdiv(L, WN_CHUNK) * 2 * sizeof(double);
}

int launch_wav_normalize(const float* mix, const float* src, const float* std_in, float* mix_out, float* src_out, int B, int K, int L,
                         double eps, void* ws, size_t ws_bytes, hipStream_t st) {
    if (!mix || !mix_out || !ws) return RTFS_ERR_ARG;
    if (B < 1 || K < 0 || L < 1 || (long long)B * (1 + K) > 65535) return RTFS_ERR_SHAPE;
    if (K > 0 && (!src || !src_out)) return RTFS_ERR_ARG;
    if (ws_bytes < wav_normalize_workspace_bytes(B, K, L)) return RTFS_ERR_WORKSPACE;
    if ((((uintptr_t)ws) & 7) || ((((uintptr_t)mix) | ((uintptr_t)src) | ((uintptr_t)mix_out) | ((uintptr_t)src_out) | ((uintptr_t)std_in)) & 3))
        return RTFS_ERR_ARG;
    const int NC = cdiv(L, WN_CHUNK), R = B * (1 + K);
    hipLaunchKernelGGL(wavnorm_stats_kernel, dim3(NC, R), dim3(256), 0, st, mix, src, (double*)ws, B, L, NC);
    int e = rtfs_launch_status();
    if (e != RTFS_OK) return e;
    hipLaunchKernelGGL(wavnorm_apply_kernel, dim3(NC, R), dim3(256), 0, st, mix, src, std_in, (const double*)ws, mix_out, src_out, B, K, L, NC,
                       eps);
    return rtfs_launch_status();
}

int resample_plan(int orig, int neu, int* o, int* n, int* width, int* taps, float* bank) {
    RsPlan P;
    const int e = rs_plan(orig, neu, P);
    if (e != RTFS_OK) return e;
    if (o) *o = P.o;
    if (n) *n = P.n;
    if (width) *width = P.width;
    if (taps) *taps = P.taps;
    if (bank) {
        for (int p = 0; p < P.n; ++p) {
            const int c = (P.o * p) / P.n;
            for (int k = 0; k < P.taps; ++k) {
                const float v = rs_tap(P, p, k);
                bank[(size_t)p * P.taps + k] = v;
                if ((k < c || k >= c + P.span) && v != 0.f) return RTFS_ERR_SHAPE;  // the kernel's support assumption does not hold
            }
        }
    }
    return RTFS_OK;
}

long long resample_out_len(int orig, int neu, long long L) {
    RsPlan P;
    if (rs_plan(orig, neu, P) != RTFS_OK || L < 0) return -1;
    return ((long long)P.n * L + P.o - 1) / P.o;
}

int launch_resample(const float* x, const float* bank, float* y, int B, int L, int orig, int neu, hipStream_t st) {
    if (!x || !bank || !y) return RTFS_ERR_ARG;
    RsPlan P;
    const int e = rs_plan(orig, neu, P);
    if (e != RTFS_OK) return e;
    if (B < 1 || B > 65535 || L < 1) return RTFS_ERR_SHAPE;
    const long long Lout = resample_out_len(orig, neu, L);
    if (Lout < 1 || Lout > 0x7fffffffLL) return RTFS_ERR_SHAPE;
    if ((((uintptr_t)x) | ((uintptr_t)bank) | ((uintptr_t)y)) & 3) return RTFS_ERR_ARG;
    const long long frames = (Lout + P.n - 1) / P.n, tiles = (frames + P.jf - 1) / P.jf;
    if (tiles > 0x7fffffffLL) return RTFS_ERR_SHAPE;
    if (P.lds > 48 * 1024 && rtfs_set_max_lds((const void*)resample_kernel, P.lds) != RTFS_OK) return RTFS_ERR_LAUNCH;
    long long gx = 2048 / B;  // enough workgroups to fill the chip; the rest of a row is walked tile by tile with the bank resident
    gx = gx < 1 ? 1 : gx;
    gx = tiles < gx ? tiles : gx;
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)gx, B), dim3(256), P.lds, st, x, bank, y, L, (int)Lout, P.o, P.n, P.width, P.taps, P.span,
                       P.jf, (int)tiles);
    return rtfs_launch_status();
}

extern "C" {

int rtfs_lips_prepare_u8(const unsigned char* roi, const int* table, float* out, int N, int Tv, int H, int W, double mean, double std,
                         void* stream) {
    return launch_lips_prepare(roi, table, out, N, Tv, H, W, mean, std, (hipStream_t)stream);
}

int rtfs_lips_prepare_rate_u8(const unsigned char* roi, const int* table, float* out, int N, int Tv_in, int H, int W, double mean, double std,
                              int rate_num, int rate_den, void* stream) {
    return launch_lips_prepare_rate(roi, table, out, N, Tv_in, H, W, mean, std, rate_num, rate_den, (hipStream_t)stream);
}

size_t rtfs_wav_normalize_workspace_bytes(int B, int K, int L) { return wav_normalize_workspace_bytes(B, K, L); }

int rtfs_wav_normalize_f32(const float* mix, const float* src, const float* std_in, float* mix_out, float* src_out, int B, int K, int L,
                           double eps, void* ws, size_t ws_bytes, void* stream) {
    return launch_wav_normalize(mix, src, std_in, mix_out, src_out, B, K, L, eps, ws, ws_bytes, (hipStream_t)stream);
}

int rtfs_resample_plan(int orig_freq, int new_freq, int* o, int* n, int* width, int* taps, float* bank) {
    return resample_plan(orig_freq, new_freq, o, n, width, taps, bank);
}

long long rtfs_resample_out_len(int orig_freq, int new_freq, long long L) { return resample_out_len(orig_freq, new_freq, L); }

int rtfs_resample_f32(const float* x, const float* bank, float* y, int B, int L, int orig_freq, int new_freq, void* stream) {
    return launch_resample(x, bank, y, B, L, orig_freq, new_freq, (hipStream_t)stream);
}

}  // extern "C"
