// Long recordings in overlapping windows (AVNet.separate_long; DESIGN.md "Long recordings"): the two streaming passes around the fused
// separator.  A recording of L samples is cut into N windows of `window` samples every `hop` samples (both multiples of SPF = 640, one
// video frame at 25 fps and 16 kHz), the B * N windows go through the ordinary fused forward as a batch, and the results are cross-faded
// back into (B, n_src, L).  tests/longform_oracle.py restates plan, framing, weights and overlap-add in float64.
//   longform_plan          host only: argument checks and N = 1 (L <= window), else 1 + ceil((L - window) / hop)
//   longform_frame_speakers_kernel  ONE launch for both gathers, K >= 1 lip tracks per recording: window n of recording b = samples
//                          [n hop, n hop + window) with zeros past L, written once, and per track the video frames [n hop / SPF,
//                          (n hop + window) / SPF) with an index past Tv - 1 reading frame Tv - 1.  (B,512,Tv) is K = 1 of (B,K,512,Tv)
//   longform_ola_kernel    gather form: an output sample sums its <= ceil(window / hop) windows in ascending n, each times
//                          w[i] = min(1, (i + 0.5) / V, (window - i - 0.5) / V), V = window - hop (w = 1 when V = 0), and divides by the sum
//                          of those weights, all recomputed in registers from the index: no atomics, no accumulator to clear, no weight
//                          buffer; every output element has exactly one writer, so the result is deterministic
// Stores follow the rules measured in round 3: a lane writes 16 bytes, a wave 1024 contiguous bytes = whole 128-byte lines.
// A window row is window * 4 bytes and a video row group 512 * (window / SPF) * 4 bytes, both multiples of 128; the (B * N, 512, window / SPF)
// gather and the (B, n_src, L) output are addressed as flat arrays, so the 200-byte video rows and an L that is not a multiple of 4
// never start a store inside a line: the last quad of the whole output is the only partial one.  Loads are 16 bytes where the source is
// aligned (always when L % 4 == 0 or B * n_src == 1) and coalesced dwords otherwise.
#include "common.h"
#include "kernels.h"
#include "longform_common.h"  // SPF, VCH, ola_weight, many_find
#include "../../include/rtfs_amd.h"  // RTFS_MAX_SPEAKERS

namespace {

// K lip tracks per recording (AVNet.separate_long: K = 1, separate_long_speakers): the audio window is written ONCE per (b, n), the K
// video windows of the row behind each other, target row (b N + n) K + k - the (rows, K, 512, Wv) layout separate_speakers takes
// without a copy.  The video share of a row is the flat (K, 512, Wv) array, K * 512 * Wv * 4 bytes = a multiple of 128, and 512 * Wv is
// a multiple of 4, so a quad never serves two tracks.
__global__ __launch_bounds__(256) void longform_frame_speakers_kernel(const float* __restrict__ wav, const float* __restrict__ video,
                                                                      float* __restrict__ wav_win, float* __restrict__ video_win, int N, int K,
                                                                      int L, int Tv, int window, int hop, int qa_pad) {
    const int row = blockIdx.x, b = row / N, n = row - b * N;
    const int Wv = window / SPF;
    int q = blockIdx.y * 256 + threadIdx.x;
    if (q < qa_pad) {  // audio quads; the segment is padded to whole waves so no wave serves both gathers
        if (q >= window / 4) return;
        const int i = 4 * q;
        const long long p = (long long)n * hop + i;  // position in the recording
        const float* src = wav + (size_t)b * L;
        f32x4 v;
        if (p + 3 < L && (((uintptr_t)(src + p)) & 15) == 0) {
            v = *(const f32x4*)(src + p);
        } else {
            v.x = p < L ? src[p] : 0.f;
            v.y = p + 1 < L ? src[p + 1] : 0.f;
            v.z = p + 2 < L ? src[p + 2] : 0.f;
            v.w = p + 3 < L ? src[p + 3] : 0.f;
        }
        *(f32x4*)(wav_win + (size_t)row * window + i) = v;
        return;
    }
    q -= qa_pad;
    const int per = VCH * Wv / 4;  // quads of one track's window
    if (q >= K * per) return;
    const int k = q / per, qk = q - k * per;
    const float* src = video + ((size_t)b * K + k) * VCH * Tv;
    const int f0 = (int)((long long)n * hop / SPF);
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int j = 4 * qk + u, c = j / Wv, f = j - c * Wv;
        const long long fr = (long long)f0 + f;
        v[u] = src[(size_t)c * Tv + (fr < Tv ? (int)fr : Tv - 1)];
    }
    *(f32x4*)(video_win + (size_t)row * K * VCH * Wv + 4 * (size_t)q) = f32x4{v[0], v[1], v[2], v[3]};
}

// one output element: windows n_lo .. n_hi contain sample t
__device__ __forceinline__ void ola_range(int t, int N, int window, int hop, int* n_lo, int* n_hi) {
    const int hi = t / hop;
    *n_hi = hi < N - 1 ? hi : N - 1;
    const int d = t - window + 1;  // n * hop >= d
    *n_lo = d <= 0 ? 0 : (d + hop - 1) / hop;
}

__global__ __launch_bounds__(256) void longform_ola_kernel(const float* __restrict__ y, float* __restrict__ out, size_t total, int n_src, int N,
                                                           int L, int window, int hop) {
    const size_t g = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;  // flat index into (B, n_src, L)
    if (g >= total) return;
    const int V = window - hop;
    const float Vf = (float)V;
    const size_t r0 = g / (size_t)L;
    const int t0 = (int)(g - r0 * (size_t)L);
    float res[4];
    if (t0 + 3 < L && (t0 & 3) == 0) {
        // the quad lies in one row at a multiple of 4: its four samples share their windows (hop and window are multiples of 4) and
        // sit at a multiple of 4 inside each, so every window contributes one aligned 16-byte load
        const int b = (int)(r0 / n_src), s = (int)(r0 - (size_t)b * n_src);
        int n_lo, n_hi;
        ola_range(t0, N, window, hop, &n_lo, &n_hi);
        float acc[4] = {0.f, 0.f, 0.f, 0.f}, ws[4] = {0.f, 0.f, 0.f, 0.f};
        for (int n = n_lo; n <= n_hi; ++n) {
            const int i = t0 - n * hop;
            const f32x4 v = *(const f32x4*)(y + (((size_t)b * N + n) * n_src + s) * window + i);
            const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float w = V == 0 ? 1.f : ola_weight(i + k, window, Vf);
                acc[k] += w * vv[k];
                ws[k] += w;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) res[k] = acc[k] / ws[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            res[k] = 0.f;
            if (g + k >= total) continue;
            size_t r = r0;
            int t = t0 + k;
            if (t >= L) {  // L >= 1 and k <= 3: the quad may run over several rows when L < 4
                r += (size_t)(t / L);
                t = t % L;
            }
            const int b = (int)(r / n_src), s = (int)(r - (size_t)b * n_src);
            int n_lo, n_hi;
            ola_range(t, N, window, hop, &n_lo, &n_hi);
            float acc = 0.f, ws = 0.f;
            for (int n = n_lo; n <= n_hi; ++n) {
                const int i = t - n * hop;
                const float w = V == 0 ? 1.f : ola_weight(i, window, Vf);
                acc += w * y[(((size_t)b * N + n) * n_src + s) * window + i];
                ws += w;
            }
            res[k] = acc / ws;
        }
    }
    if (g + 3 < total) {
        *(f32x4*)(out + g) = f32x4{res[0], res[1], res[2], res[3]};
    } else {  // the tail of the whole output: the only partial line
        for (int k = 0; k < 4 && g + k < total; ++k) out[g + k] = res[k];
    }
}

}  // namespace

int longform_plan(int L, int Tv, int window, int hop, int* N) {
    if (L < 1 || Tv < 1 || window < SPF || hop < SPF || hop > window || window % SPF || hop % SPF) return RTFS_ERR_ARG;
    const long long n = L <= window ? 1 : 1 + ((long long)L - window + hop - 1) / hop;
    if (n > 0x7fffffffLL) return RTFS_ERR_ARG;
    if (N) *N = (int)n;
    return RTFS_OK;
}

int launch_longform_frame_speakers(const float* wav, const float* video, float* wav_win, float* video_win, int B, int K, int L, int Tv,
                                   int window, int hop, hipStream_t st) {
    int N = 0;
    const int e = longform_plan(L, Tv, window, hop, &N);
    if (e != RTFS_OK) return e;
    if (K < 1 || K > RTFS_MAX_SPEAKERS) return RTFS_ERR_ARG;
    if (B < 1 || (long long)B * N * K > 0x7fffffffLL) return RTFS_ERR_SHAPE;
    if ((((uintptr_t)wav_win) | ((uintptr_t)video_win)) & 15) return RTFS_ERR_ARG;
    const int qa_pad = cdiv(window / 4, 64) * 64;
    const long long quads = qa_pad + (long long)K * VCH * (window / SPF) / 4;
    if ((quads + 255) / 256 > 65535) return RTFS_ERR_SHAPE;
    hipLaunchKernelGGL(longform_frame_speakers_kernel, dim3(B * N, (unsigned)((quads + 255) / 256)), dim3(256), 0, st, wav, video, wav_win,
                       video_win, N, K, L, Tv, window, hop, qa_pad);
    return rtfs_launch_status();
}

int launch_longform_overlap_add(const float* y, float* out, int B, int n_src, int L, int window, int hop, hipStream_t st) {
    int N = 0;
    const int e = longform_plan(L, 1, window, hop, &N);
    if (e != RTFS_OK) return e;
    if (B < 1 || n_src < 1 || (long long)B * N > 0x7fffffffLL || (long long)B * n_src > 0x7fffffffLL) return RTFS_ERR_SHAPE;
    if ((((uintptr_t)y) | ((uintptr_t)out)) & 15) return RTFS_ERR_ARG;
    const size_t total = (size_t)B * n_src * L, blocks = (total + 1023) / 1024;
    if (blocks > 0x7fffffffULL) return RTFS_ERR_SHAPE;
    hipLaunchKernelGGL(longform_ola_kernel, dim3((unsigned)blocks), dim3(256), 0, st, y, out, total, n_src, N, L, window, hop);
    return rtfs_launch_status();
}

// ----------------------------------------------------------------------------- many recordings of different lengths in one pooled pass
// AVNet.separate_many (DESIGN.md "Many recordings"): R recordings, each planned on its own with longform_plan, their sum(N_r) windows
// laid out in recording order, then window order, so the fused forward runs on full chunks that straddle recordings.  The recordings
// stay where they are (R separate allocations): the kernels read them through a device table of per-recording pointers and the plan
// table of longform_many_plan, 5 * R int64 words [row0 | N | L | Tv | out_off].  Recording r's (n_src, L_r) result starts out_off[r]
// floats into ONE flat output; out_off is a multiple of MANY_ALIGN = 32 floats (a 128-byte line), so no 16-byte store and no line is
// shared by two recordings, and the floats between two blocks are never written.  Per recording the arithmetic is that of the two
// kernels above, term by term and in the same order.
namespace {

constexpr int MANY_ALIGN = 32;  // floats: every recording's block of the flat output starts on a 128-byte line

// TK (AVNet.separate_many_speakers): K_r lip tracks per recording.  The table of longform_many_speakers_plan carries two more columns,
// [.. | K | trow0]: recording r's video is (K_r, 512, Tv_r), window n's K_r target rows are trow0[r] + n K_r + k - per recording the
// (rows, K, 512, Wv) layout of longform_frame_speakers_kernel - and its result block is (K_r, L_r).  The audio window is written once.
template <bool TK>
__global__ __launch_bounds__(256) void longform_frame_many_kernel(const float* const* __restrict__ wavs, const float* const* __restrict__ videos,
                                                                  const long long* __restrict__ table, float* __restrict__ wav_win,
                                                                  float* __restrict__ video_win, int R, int window, int hop, int qa_pad) {
    const int row = blockIdx.x;
    const int r = many_find(table, R, row);  // block-uniform: scalar loads
    const int n = row - (int)table[r];
    if (n >= (int)table[R + r]) return;  // a table that does not cover this row: write nothing
    const int L = (int)table[2 * R + r], Tv = (int)table[3 * R + r];
    const int Wv = window / SPF;
    int q = blockIdx.y * 256 + threadIdx.x;
    if (q < qa_pad) {  // audio quads; the segment is padded to whole waves so no wave serves both gathers
        if (q >= window / 4) return;
        const int i = 4 * q;
        const long long p = (long long)n * hop + i;  // position in the recording
        const float* src = wavs[r];
        f32x4 v;
        if (p + 3 < L && (((uintptr_t)(src + p)) & 15) == 0) {
            v = *(const f32x4*)(src + p);
        } else {
            v.x = p < L ? src[p] : 0.f;
            v.y = p + 1 < L ? src[p + 1] : 0.f;
            v.z = p + 2 < L ? src[p + 2] : 0.f;
            v.w = p + 3 < L ? src[p + 3] : 0.f;
        }
        *(f32x4*)(wav_win + (size_t)row * window + i) = v;
        return;
    }
    q -= qa_pad;
    const int per = VCH * Wv / 4;  // quads of one track's window
    const int K = TK ? (int)table[5 * (size_t)R + r] : 1;
    if (q >= K * per) return;
    const int kt = TK ? q / per : 0, qk = q - kt * per;
    const float* src = videos[r] + (size_t)kt * VCH * Tv;
    const size_t trow = TK ? (size_t)(table[6 * (size_t)R + r] + (long long)n * K) : (size_t)row;  // the window's first target row
    const int f0 = (int)((long long)n * hop / SPF);
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = 4 * qk + k, c = j / Wv, f = j - c * Wv;
        const long long fr = (long long)f0 + f;
        v[k] = src[(size_t)c * Tv + (fr < Tv ? (int)fr : Tv - 1)];
    }
    *(f32x4*)(video_win + trow * VCH * Wv + 4 * (size_t)q) = f32x4{v[0], v[1], v[2], v[3]};
}

template <bool TK>
__global__ __launch_bounds__(256) void longform_ola_many_kernel(const float* __restrict__ y, float* __restrict__ out,
                                                                const long long* __restrict__ table, long long out_floats, int R, int n_src_,
                                                                int window, int hop) {
    const long long g = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;  // flat index into the padded output
    if (g >= out_floats) return;
    const int r = many_find(table + 4 * (size_t)R, R, g);
    // y rows of window n: (row0 + n) n_src + s; with K_r tracks trow0 + n K_r + s (n_src := K_r, row0 n_src := trow0)
    const int n_src = TK ? (int)table[5 * (size_t)R + r] : n_src_;
    const size_t yrow0 = TK ? (size_t)table[6 * (size_t)R + r] : (size_t)table[r] * n_src;
    const int N = (int)table[R + r], L = (int)table[2 * R + r];
    const long long total = (long long)n_src * L, e = g - table[4 * (size_t)R + r];  // this recording's (n_src, L) block, and the index into it
    if (e >= total) return;  // padding up to the next recording's line: never written
    const int V = window - hop;
    const float Vf = (float)V;
    const int s0 = (int)(e / L), t0 = (int)(e - (long long)s0 * L);
    float res[4];
    if (t0 + 3 < L && (t0 & 3) == 0) {
        // the quad lies in one row at a multiple of 4: one aligned 16-byte load per window, as in longform_ola_kernel
        int n_lo, n_hi;
        ola_range(t0, N, window, hop, &n_lo, &n_hi);
        float acc[4] = {0.f, 0.f, 0.f, 0.f}, ws[4] = {0.f, 0.f, 0.f, 0.f};
        for (int n = n_lo; n <= n_hi; ++n) {
            const int i = t0 - n * hop;
            const f32x4 v = *(const f32x4*)(y + (yrow0 + (size_t)n * n_src + s0) * window + i);
            const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float w = V == 0 ? 1.f : ola_weight(i + k, window, Vf);
                acc[k] += w * vv[k];
                ws[k] += w;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) res[k] = acc[k] / ws[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            res[k] = 0.f;
            if (e + k >= total) continue;
            int s = s0, t = t0 + k;
            if (t >= L) {  // L >= 1 and k <= 3: the quad may run over several sources when L < 4
                s += t / L;
                t = t % L;
            }
            int n_lo, n_hi;
            ola_range(t, N, window, hop, &n_lo, &n_hi);
            float acc = 0.f, ws = 0.f;
            for (int n = n_lo; n <= n_hi; ++n) {
                const int i = t - n * hop;
                const float w = V == 0 ? 1.f : ola_weight(i, window, Vf);
                acc += w * y[(yrow0 + (size_t)n * n_src + s) * window + i];
                ws += w;
            }
            res[k] = acc / ws;
        }
    }
    if (e + 3 < total) {
        *(f32x4*)(out + g) = f32x4{res[0], res[1], res[2], res[3]};
    } else {  // the tail of a recording: the only partial quad of its block
        for (int k = 0; k < 4 && e + k < total; ++k) out[g + k] = res[k];
    }
}

}  // namespace

// K null: n_src result rows per recording, 5 R table words.  K (longform_many_speakers_plan): K[r] lip tracks and result rows of
// recording r, 7 R words [.. | K | trow0], trow0 the recording's first target row (targets of window n: trow0 + n K .. + K - 1).
static int many_plan(const long long* L, const long long* Tv, const long long* K, int R, int window, int hop, int n_src_, long long* table,
                     long long* total_windows, long long* total_targets, long long* out_floats) {
    if (!L || !Tv || R < 1 || n_src_ < 1) return RTFS_ERR_ARG;
    long long rows = 0, trows = 0, off = 0;
    for (int r = 0; r < R; ++r) {
        if (L[r] < 1 || Tv[r] < 1 || L[r] > 0x7fffffffLL || Tv[r] > 0x7fffffffLL) return RTFS_ERR_ARG;
        if (K && (K[r] < 1 || K[r] > RTFS_MAX_SPEAKERS)) return RTFS_ERR_ARG;
        const int n_src = K ? (int)K[r] : n_src_;
        int N = 0;
        const int e = longform_plan((int)L[r], (int)Tv[r], window, hop, &N);
        if (e != RTFS_OK) return e;
        if (table) {
            table[r] = rows;
            table[(size_t)R + r] = N;
            table[2 * (size_t)R + r] = L[r];
            table[3 * (size_t)R + r] = Tv[r];
            table[4 * (size_t)R + r] = off;
            if (K) {
                table[5 * (size_t)R + r] = K[r];
                table[6 * (size_t)R + r] = trows;
            }
        }
        rows += N;
        trows += (long long)N * n_src;
        if (rows > 0x7fffffffLL || (K && trows > 0x7fffffffLL)) return RTFS_ERR_SHAPE;
        const long long block = ((long long)n_src * L[r] + MANY_ALIGN - 1) / MANY_ALIGN * MANY_ALIGN;  // n_src, L < 2^31: below 2^62
        if (off > (1LL << 62) - block) return RTFS_ERR_SHAPE;
        off += block;
    }
    if (total_windows) *total_windows = rows;
    if (total_targets) *total_targets = trows;
    if (out_floats) *out_floats = off;
    return RTFS_OK;
}

int longform_many_plan(const long long* L, const long long* Tv, int R, int window, int hop, int n_src, long long* table, long long* total_windows,
                       long long* out_floats) {
    return many_plan(L, Tv, nullptr, R, window, hop, n_src, table, total_windows, nullptr, out_floats);
}

int longform_many_speakers_plan(const long long* L, const long long* Tv, const long long* K, int R, int window, int hop, long long* table,
                                long long* total_windows, long long* total_targets, long long* out_floats) {
    if (!K) return RTFS_ERR_ARG;
    return many_plan(L, Tv, K, R, window, hop, 1, table, total_windows, total_targets, out_floats);
}

int launch_longform_frame_many(const float* const* wavs, const float* const* videos, const long long* table, float* wav_win, float* video_win,
                               int R, int total_windows, int window, int hop, hipStream_t st) {
    const int e = longform_plan(1, 1, window, hop, nullptr);
    if (e != RTFS_OK) return e;
    if (R < 1 || total_windows < R) return RTFS_ERR_SHAPE;
    if ((((uintptr_t)wav_win) | ((uintptr_t)video_win)) & 15) return RTFS_ERR_ARG;
    if ((((uintptr_t)wavs) | ((uintptr_t)videos) | ((uintptr_t)table)) & 7) return RTFS_ERR_ARG;
    const int qa_pad = cdiv(window / 4, 64) * 64, qv = VCH * (window / SPF) / 4;
    hipLaunchKernelGGL(longform_frame_many_kernel<false>, dim3(total_windows, cdiv(qa_pad + qv, 256)), dim3(256), 0, st, wavs, videos, table, wav_win,
                       video_win, R, window, hop, qa_pad);
    return rtfs_launch_status();
}

// max_K: the largest K_r of the table (sizes the grid; a recording with fewer tracks leaves its surplus blocks idle)
int launch_longform_frame_many_speakers(const float* const* wavs, const float* const* videos, const long long* table, float* wav_win,
                                        float* video_win, int R, int total_windows, int max_K, int window, int hop, hipStream_t st) {
    const int e = longform_plan(1, 1, window, hop, nullptr);
    if (e != RTFS_OK) return e;
    if (max_K < 1 || max_K > RTFS_MAX_SPEAKERS) return RTFS_ERR_ARG;
    if (R < 1 || total_windows < R) return RTFS_ERR_SHAPE;
    if ((((uintptr_t)wav_win) | ((uintptr_t)video_win)) & 15) return RTFS_ERR_ARG;
    if ((((uintptr_t)wavs) | ((uintptr_t)videos) | ((uintptr_t)table)) & 7) return RTFS_ERR_ARG;
    const int qa_pad = cdiv(window / 4, 64) * 64;
    const long long quads = qa_pad + (long long)max_K * VCH * (window / SPF) / 4;
    if ((quads + 255) / 256 > 65535) return RTFS_ERR_SHAPE;
    hipLaunchKernelGGL(longform_frame_many_kernel<true>, dim3(total_windows, (unsigned)((quads + 255) / 256)), dim3(256), 0, st, wavs, videos, table,
                       wav_win, video_win, R, window, hop, qa_pad);
    return rtfs_launch_status();
}

int launch_longform_overlap_add_many(const float* y, float* out, const long long* table, int R, int total_windows, long long out_floats,
                                     int n_src, int window, int hop, hipStream_t st) {
    const int e = longform_plan(1, 1, window, hop, nullptr);
    if (e != RTFS_OK) return e;
    if (R < 1 || total_windows < R || n_src < 1 || out_floats < MANY_ALIGN || out_floats % MANY_ALIGN) return RTFS_ERR_SHAPE;
    if ((((uintptr_t)y) | ((uintptr_t)out)) & 15) return RTFS_ERR_ARG;
    if (((uintptr_t)table) & 7) return RTFS_ERR_ARG;
    const long long blocks = (out_floats + 1023) / 1024;
    if (blocks > 0x7fffffffLL) return RTFS_ERR_SHAPE;
    hipLaunchKernelGGL(longform_ola_many_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, y, out, table, out_floats, R, n_src, window, hop);
    return rtfs_launch_status();
}

int launch_longform_overlap_add_many_speakers(const float* y, float* out, const long long* table, int R, int total_windows, long long out_floats,
                                              int window, int hop, hipStream_t st) {
    const int e = longform_plan(1, 1, window, hop, nullptr);
    if (e != RTFS_OK) return e;
    if (R < 1 || total_windows < R || out_floats < MANY_ALIGN || out_floats % MANY_ALIGN) return RTFS_ERR_SHAPE;
    if ((((uintptr_t)y) | ((uintptr_t)out)) & 15) return RTFS_ERR_ARG;
    if (((uintptr_t)table) & 7) return RTFS_ERR_ARG;
    const long long blocks = (out_floats + 1023) / 1024;
    if (blocks > 0x7fffffffLL) return RTFS_ERR_SHAPE;
    hipLaunchKernelGGL(longform_ola_many_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, y, out, table, out_floats, R, 1, window, hop);
    return rtfs_launch_status();
}
