// Live streams at the microphone's own rate (datas.open_resample_streams / ResampleStreamPool; DESIGN.md "Live streams at the
// microphone's rate"): rtfs_resample_f32 chunk by chunk.  tests/live_resample_oracle.py restates counters, emitted ranges and the history
// in numpy.
//
// Notation of rtfs_resample_plan: o, n the reduced rates, width, span = 2 width + 1, c(p) = floor(o p / n).  Output q = j n + p of a
// recording is sum_{s < span} bank[p, c(p) + s] x[j o + c(p) - width + s]: it reads the inputs first(q) = j o + c(p) - width through
// last(q) = first(q) + 2 width.  last(q) never decreases with q, and #{q : j o + c(p) < B} = ceil(n B / o), so
//   G(A) = #{q : last(q) < A} = ceil(n max(0, A - width) / o).
//
// Host counters per slot (kept by the caller, nothing is read back): a input samples received, g output samples emitted, side.
//   push of m samples:  a' = a + m, g' = G(a'), emits g .. g' - 1;  side' = 1 - side when m > 0
//   flush:              emits g .. ceil(n a / o) - 1 with exact zeros for input indices >= a;  counters return to zero
// Input indices < 0 are exact zeros too (the recording's own padding in rtfs_resample_f32).  g = G(a) between calls, so last(g) >= a and
// the next output needs no input older than a - 2 width.
//
// State per slot, device resident: hist (slots, 2, 2 width), two history buffers.  Buffer `side` holds the inputs a - 2 width .. a - 1,
// input x in cell x - (a - 2 width); cells of indices < 0 hold zeros that nothing reads.
//
//   live_resample_plan     host only, the single place with the arithmetic: counters + chunk sizes -> new counters and the tick table,
//                          7 int64 words per named slot, column-major [slot | a | m | g | k | out_off | side]; the caller appends one
//                          column of chunk pointers and uploads the 8 R words with one copy
//   live_resample_kernel   ONE launch, grid (tiles + history blocks, R): a tile block forms up to `tile` outputs of its slot with the
//                          fmaf chain of resample_kernel (k_prep.hip), a history block writes 256 cells of buffer 1 - side
//   live_resample_reset_kernel  gives a slot's history defined contents (zeros)
//
// WHY NO BLOCK READS A CELL THAT ANOTHER BLOCK OF THE SAME LAUNCH WRITES.  Every read of state - a staged input x < a, or an input x < a
// that stays in the history because m < 2 width - goes to buffer `side` of its slot; every write goes to buffer 1 - side, one thread per
// cell.  Two named slots never share state and the planner refuses a slot named twice.  A push with m = 0 and a flush write no history
// (the side stays).  Outputs have one writer each: tile t of table row r owns out[out_off + t tile .. ).
#include "../../include/rtfs_amd.h"  // RTFS_LIVE_*
#include "common.h"
#include "kernels.h"

namespace {

constexpr int LR_ALIGN = RTFS_LIVE_ALIGN;
constexpr int LR_XSEG = 16384;     // floats of input one tile may stage, as resample_kernel
constexpr int LR_TILE_OUT = 2048;  // outputs per tile when the input segment allows
constexpr long long LR_LIMIT = 1LL << 50;  // a and m stay below it, so n (a + m) fits 64 bits at n <= 640
// columns of the tick table
enum { C_SLOT, C_A, C_M, C_G, C_K, C_OFF, C_SIDE, C_PTR };

struct LrPlan {
    int o, n, width, taps, span;
    int jf;    // a tile is jf * n outputs; unaligned to frames, so it touches at most jf + 1 frames of o inputs
    int segf;  // floats of the staged segment: (jf + 1) o + 2 width
    size_t lds;
};

int lr_plan(int orig, int neu, LrPlan& P) {
    if (resample_plan(orig, neu, &P.o, &P.n, &P.width, &P.taps, nullptr) != RTFS_OK) return RTFS_ERR_ARG;
    P.span = 2 * P.width + 1;
    int jf = (LR_XSEG - 2 * P.width) / P.o - 1;
    const int cap = LR_TILE_OUT / P.n;
    if (jf > cap) jf = cap;
    P.jf = jf < 1 ? 1 : jf;
    P.segf = (P.jf + 1) * P.o + 2 * P.width;
    P.lds = ((size_t)P.n * P.span + (size_t)P.n + (size_t)P.segf) * sizeof(float);
    return RTFS_OK;
}

long long lr_G(const LrPlan& P, long long A) {
    const long long B = A - P.width;
    return B <= 0 ? 0 : (P.n * B + P.o - 1) / P.o;
}

// input x of the stream of table row r: an exact zero outside [0, a + m) (m = 0 at a flush), buffer `side` below a, the chunk from a on.
// An x < a - 2 width is never asked for by an output (last(g) >= a); a staged segment starts at its first frame's start and may reach
// below it, where the answer is unused and must only not be read from memory.
template <bool I16>
__device__ __forceinline__ float lr_sample(long long x, long long a, long long lim, int H, const float* __restrict__ hs, const void* chunk) {
    if (x < 0 || x >= lim || x < a - H) return 0.f;
    if (x < a) return hs[x - (a - H)];
    if (I16) return (float)((const short*)chunk)[x - a] * (1.0f / 32768.0f);  // exact: a power of two
    return ((const float*)chunk)[x - a];
}

template <bool I16>
__global__ __launch_bounds__(256) void live_resample_kernel(const long long* __restrict__ table, const float* __restrict__ bank, float* hist,
                                                             float* __restrict__ out, int R, int tiles, int o, int n, int width, int taps,
                                                             int span, int tile) {
    extern __shared__ __attribute__((aligned(16))) float lr_lds[];
    const int tid = threadIdx.x, r = blockIdx.y, H = 2 * width;
    const long long a = table[(size_t)C_A * R + r], m = table[(size_t)C_M * R + r];
    const size_t slot = (size_t)table[(size_t)C_SLOT * R + r], side = (size_t)table[(size_t)C_SIDE * R + r];
    const float* hs = hist + (slot * 2 + side) * H;
    const void* chunk = (const void*)(uintptr_t)table[(size_t)C_PTR * R + r];
    if ((int)blockIdx.x >= tiles) {
        // ---- history: cell i of buffer 1 - side holds input a' - 2 width + i
        if (m <= 0) return;  // nothing arrived: the side stays
        const int i = ((int)blockIdx.x - tiles) * 256 + tid;
        if (i < H) hist[(slot * 2 + (1 - side)) * H + i] = lr_sample<I16>(a + m - H + i, a, a + m, H, hs, chunk);
        return;
    }
    const long long k = table[(size_t)C_K * R + r], t0 = (long long)blockIdx.x * tile;
    if (t0 >= k) return;  // a tile past this slot's outputs
    float* bk = lr_lds;               // n * span
    int* cp = (int*)(bk + n * span);  // n
    float* xs = (float*)(cp + n);     // (jf + 1) o + 2 width
    for (int p = tid; p < n; p += 256) cp[p] = (o * p) / n;
    for (int i = tid; i < n * span; i += 256) {
        const int p = i / span, s = i - p * span;
        bk[i] = bank[(size_t)p * taps + (o * p) / n + s];
    }
    const int outs = (int)(k - t0 < tile ? k - t0 : tile);
    const long long q0 = table[(size_t)C_G * R + r] + t0, j0 = q0 / n;
    const int p0 = (int)(q0 - j0 * n);
    const int frames = (p0 + outs - 1) / n + 1;  // <= jf + 1
    const int seg = frames * o + H;
    const long long x0 = j0 * o - width;
    for (int i = tid; i < seg; i += 256) xs[i] = lr_sample<I16>(x0 + i, a, a + m, H, hs, chunk);
    __syncthreads();
    float* y = out + table[(size_t)C_OFF * R + r] + t0;
    for (int gl = tid; gl < outs; gl += 256) {
        const int e = p0 + gl, jl = e / n, p = e - jl * n;
        const float* b = bk + p * span;
        const float* xv = xs + jl * o + cp[p];
        float acc = 0.f;
#pragma unroll 4
        for (int s = 0; s < span; ++s) acc = fmaf(b[s], xv[s], acc);
        y[gl] = acc;
    }
}

__global__ __launch_bounds__(256) void live_resample_reset_kernel(const long long* __restrict__ ids, float* __restrict__ hist, int cells) {
    const size_t slot = ids ? (size_t)ids[blockIdx.x] : blockIdx.x;
    const int i = blockIdx.y * 256 + threadIdx.x;
    if (i < cells) hist[slot * cells + i] = 0.f;
}

}  // namespace

int live_resample_plan(const long long* slot_ids, const long long* counters, const long long* n_samples, int R, int slots, int flush,
                       int orig, int neu, long long max_chunk_in, long long* new_counters, long long* table, long long* sizes, int* refused) {
    auto refuse = [&](int r, int reason) {
        if (refused) {
            refused[0] = r;
            refused[1] = reason;
        }
        return RTFS_ERR_ARG;
    };
    LrPlan P;
    if (!slot_ids || !counters || R < 1 || slots < 1 || max_chunk_in < 1 || max_chunk_in > LR_LIMIT || (!flush && !n_samples) ||
        lr_plan(orig, neu, P) != RTFS_OK)
        return refuse(-1, RTFS_LIVE_BAD_ARGUMENT);
    for (int r = 0; r < R; ++r) {
        if (slot_ids[r] < 0 || slot_ids[r] >= slots) return refuse(r, RTFS_LIVE_UNKNOWN_SLOT);
        for (int q = 0; q < r; ++q)
            if (slot_ids[q] == slot_ids[r]) return refuse(r, RTFS_LIVE_REPEATED_SLOT);
    }
    long long off = 0, max_m = 0, max_k = 0;
    // two passes, so that a refusal at any slot leaves every output unwritten: pass 0 only checks, pass 1 only writes
    for (int pass = 0; pass < 2; ++pass) {
        off = max_m = max_k = 0;
        for (int r = 0; r < R; ++r) {
            const long long a = counters[3 * r], g = counters[3 * r + 1], side = counters[3 * r + 2];
            if (a < 0 || a > LR_LIMIT || g != lr_G(P, a) || (side != 0 && side != 1)) return refuse(r, RTFS_LIVE_BAD_COUNTERS);
            long long m = 0, g1;
            if (!flush) {
                m = n_samples[r];
                if (m < 0 || m > max_chunk_in) return refuse(r, RTFS_LIVE_CHUNK_SIZE);
                if (a + m > LR_LIMIT) return refuse(r, RTFS_LIVE_BAD_ARGUMENT);
                g1 = lr_G(P, a + m);
            } else {
                g1 = (P.n * a + P.o - 1) / P.o;  // rtfs_resample_out_len of the samples received
            }
            const long long k = g1 - g;
            if (pass && table) {
                const long long col[RTFS_LIVE_RESAMPLE_PLAN_WORDS] = {slot_ids[r], a, m, g, k, off, side};
                for (int w = 0; w < RTFS_LIVE_RESAMPLE_PLAN_WORDS; ++w) table[(size_t)w * R + r] = col[w];
            }
            if (pass && new_counters) {
                new_counters[3 * r] = flush ? 0 : a + m;
                new_counters[3 * r + 1] = flush ? 0 : g1;
                new_counters[3 * r + 2] = flush ? 0 : (m > 0 ? 1 - side : side);
            }
            off += (k + LR_ALIGN - 1) / LR_ALIGN * LR_ALIGN;
            max_m = m > max_m ? m : max_m;
            max_k = k > max_k ? k : max_k;
        }
    }
    if (sizes) {
        sizes[0] = off;
        sizes[1] = max_m;
        sizes[2] = max_k;
    }
    if (refused) refused[0] = -1, refused[1] = 0;
    return RTFS_OK;
}

int launch_live_resample(const long long* table, const float* bank, float* hist, float* out, int R, long long max_m, long long max_k,
                         int flush, bool i16, int orig, int neu, hipStream_t st) {
    LrPlan P;
    if (lr_plan(orig, neu, P) != RTFS_OK) return RTFS_ERR_ARG;
    if (R < 1 || R > 65535 || max_m < 0 || max_k < 0 || (flush && max_m != 0)) return RTFS_ERR_SHAPE;
    if (((((uintptr_t)hist) | ((uintptr_t)out)) & 15) || (((uintptr_t)table) & 7) || (((uintptr_t)bank) & 3)) return RTFS_ERR_ARG;
    if (max_k == 0 && max_m == 0) return RTFS_OK;  // nothing arrived, nothing is ready
    const int tile = P.jf * P.n;
    const long long tiles = (max_k + tile - 1) / tile, blocks = tiles + (max_m > 0 ? cdiv(2 * P.width, 256) : 0);
    if (blocks > 0x7fffffffLL) return RTFS_ERR_SHAPE;
    const void* kern = i16 ? (const void*)live_resample_kernel<true> : (const void*)live_resample_kernel<false>;
    if (P.lds > 48 * 1024 && rtfs_set_max_lds(kern, P.lds) != RTFS_OK) return RTFS_ERR_LAUNCH;
    if (i16)
        hipLaunchKernelGGL(live_resample_kernel<true>, dim3((unsigned)blocks, R), dim3(256), P.lds, st, table, bank, hist, out, R, (int)tiles,
                           P.o, P.n, P.width, P.taps, P.span, tile);
    else
        hipLaunchKernelGGL(live_resample_kernel<false>, dim3((unsigned)blocks, R), dim3(256), P.lds, st, table, bank, hist, out, R, (int)tiles,
                           P.o, P.n, P.width, P.taps, P.span, tile);
    return rtfs_launch_status();
}

int launch_live_resample_reset(const long long* ids, float* hist, int R, int orig, int neu, hipStream_t st) {
    LrPlan P;
    if (lr_plan(orig, neu, P) != RTFS_OK) return RTFS_ERR_ARG;
    if (R < 1) return RTFS_ERR_SHAPE;
    if ((((uintptr_t)hist) & 15) || (((uintptr_t)ids) & 7)) return RTFS_ERR_ARG;
    hipLaunchKernelGGL(live_resample_reset_kernel, dim3(R, cdiv(4 * P.width, 256)), dim3(256), 0, st, ids, hist, 4 * P.width);
    return rtfs_launch_status();
}

extern "C" {

int rtfs_live_resample_plan(const long long* slot_ids, const long long* counters, const long long* n_samples, int R, int slots, int flush,
                            int orig_freq, int new_freq, long long max_chunk_in, long long* new_counters, long long* table, long long* sizes,
                            int* refused) {
    return live_resample_plan(slot_ids, counters, n_samples, R, slots, flush, orig_freq, new_freq, max_chunk_in, new_counters, table, sizes,
                              refused);
}

int rtfs_live_resample_f32(const long long* table, const float* bank, float* hist, float* out, int R, long long max_m, long long max_k,
                           int flush, int orig_freq, int new_freq, void* stream) {
    if (!table || !bank || !hist || (!out && max_k > 0)) return RTFS_ERR_ARG;
    return launch_live_resample(table, bank, hist, out, R, max_m, max_k, flush, false, orig_freq, new_freq, (hipStream_t)stream);
}

int rtfs_live_resample_i16(const long long* table, const float* bank, float* hist, float* out, int R, long long max_m, long long max_k,
                           int flush, int orig_freq, int new_freq, void* stream) {
    if (!table || !bank || !hist || (!out && max_k > 0)) return RTFS_ERR_ARG;
    return launch_live_resample(table, bank, hist, out, R, max_m, max_k, flush, true, orig_freq, new_freq, (hipStream_t)stream);
}

int rtfs_live_resample_reset(const long long* ids, float* hist, int R, int orig_freq, int new_freq, void* stream) {
    if (!hist) return RTFS_ERR_ARG;
    return launch_live_resample_reset(ids, hist, R, orig_freq, new_freq, (hipStream_t)stream);
}

}  // extern "C"
