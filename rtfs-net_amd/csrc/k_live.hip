// Live streams chunk by chunk (AVNet.open_streams / StreamPool; DESIGN.md "Live streams", "Every face of a stream"): the stateful form
// of the long-form plan of k_longform.hip.  A stream delivers audio and lip frames a chunk at a time; window n = samples [n hop, n hop +
// window) is run as soon as its samples AND its frames have arrived, and after window n the samples [n hop, (n + 1) hop) can be touched by
// no later window, so they leave at once.  The concatenated outputs are separate_long's of the whole recording.  tests/live_oracle.py
// and tests/live_speakers_oracle.py restate counters, readiness, ring positions and the streaming overlap-add in float64.
//
// A slot has ONE microphone track and K lip tracks, 1 <= K <= RTFS_MAX_SPEAKERS; the single-track pool is K = 1.  State per slot, device
// resident, allocated once (C = window + max_chunk samples, C / SPF frames):
//   audio ring  (slots, C)                sample p of the stream lives in cell p % C: stored once, framed once, whatever K
//   video ring  (slots, K, 512, C / SPF)  frame q of track k lives in column q % (C / SPF) of plane (slot, k); channel-major like the lip
//                                         embedding, so the framing gather reads runs of a window's frames as k_longform.hip does
//   accumulator (slots, n_acc, C)         the weighted sum so far of a sample that later windows still reach, in cell t % C; n_acc = the
//                                         rows of y per window: n_src of `forward` at K = 1, K of separate_speakers otherwise
// Host counters per slot (kept by the caller, nothing is read back): a samples received, f frames received, e windows emitted,
// o samples output.  The K tracks of a slot are pushed together with ONE m, so they share f (and a, e, o).
//
//   live_plan                          host only, the single place with the arithmetic: counters + the sizes of this push / flush -> new
//                                      counters and the tick table, 13 int64 words per named slot, column-major
//                                      [slot | a | na | f | nf | e | cnt | row0 | o | end | out_off | apos | fpos]; the caller appends the
//                                      1 + K columns of chunk pointers [aptr | vptr_0 | .. | vptr_{K-1}] - the K chunks of a slot are K
//                                      separate allocations - and uploads the (14 + K) R words with one copy
//   live_ingest_frame_speakers_kernel  ONE launch: blocks x >= rows append the audio chunk and the K lip chunks of their slot to the
//                                      rings; blocks x < rows write the audio window once and the K video windows of the row behind
//                                      each other: video_win (rows * K, 512, Wv), target row r K + k
//   live_ola_kernel                    gather form, one thread per 4 samples of one of the n_acc rows: final samples are divided and
//                                      written to the flat output, samples a later window still reaches go back to the accumulator
//   live_reset_kernel                  gives a slot's state defined contents (zeros)
//   live_faces_plan, live_ingest_frame_faces_kernel, live_ola_faces_kernel: the same three steps for slots whose faces come and go (a
//                                      birth window per face, ragged target rows); their table and their disjointness argument stand
//                                      at the head of their section at the end of this file
//
// WHY THE INGEST BLOCKS AND THE FRAMING BLOCKS OF ONE LAUNCH NEVER TOUCH THE SAME RING CELL.  A framing block reads sample p of window
// n >= e from the audio ring only if p < a (it arrived in an earlier push), so it reads stream positions in [e hop, a); an ingest block
// writes the stream positions [a, a + na).  live_plan refuses a push unless a + na - e hop <= C, so all positions of [e hop, a + na) have
// different residues mod C: the cells read and the cells written are disjoint, whatever order the blocks run in.  Per lip track the same
// holds in its plane (slot, k): frame q of window n >= e is read only if q < f, positions [e hop / SPF, f); an ingest block writes
// [f, f + nf) of that plane; all tracks of a slot share f and e, and live_plan refuses a push unless f + nf - e hop / SPF <= C / SPF.
// Two planes (another track, another slot) share no cell at all, and live_plan refuses a slot named twice.  The cells read are intact
// for the same reason: every accepted push kept a - e hop <= C and f - e hop / SPF <= C / SPF, for all K tracks at once, and e only
// grows.  A flush writes no ring cell.
//
// WHY THE ACCUMULATOR IS C FLOATS LONG.  A tick reads the sums of [e hop, (e - 1) hop + window) and writes those of [e' hop, (e' - 1) hop +
// window) with e' = e + cnt.  A ready window has a' >= (e' - 1) hop + window, so both ranges lie in [e hop, e hop + C): distinct residues
// mod C, every cell has at most one thread, which reads before it writes.  (A ring of `window` floats would alias t and t + window as
// soon as one tick emits window / hop + 1 windows.)  Which cells hold a sum is known from the counters (t < (e - 1) hop + window), so
// no kernel depends on the value of a cell that holds none.
//
// LAUNCH SIZES.  window / hop as longform_plan takes them, max_chunk a positive multiple of SPF, and K (window + max_chunk) <=
// RTFS_LIVE_MAX_CAPACITY (live_speakers_sizes_ok): the video share of the grids grows K-fold, so the framing / ingest grid has
// < 0.45 K C / 256 and the reset grid of a K-track pool < 0.7 K C / 256 blocks in y, the overlap-add grid C / 1024, all below 65535.
// open_streams refuses a larger pool, so a pool it accepted cannot fail at a launch (the launchers check their grids all the same).
//
// Stores follow k_longform.hip: a lane writes 16 bytes, a wave 1024 contiguous bytes, wherever the layout is aligned - the framed
// windows always, the rings when the write position is a multiple of 4 (always when chunks are multiples of 4 samples), the output when
// its block length is a multiple of 4 (always but at a flush).  Chunks may start at any 4-byte boundary: an unaligned chunk is read
// with dword loads.
#include "common.h"
#include "kernels.h"
#include "longform_common.h"  // SPF, VCH, ola_weight, many_find
#include "../../include/rtfs_amd.h"  // RTFS_LIVE_*

namespace {

constexpr int LIVE_ALIGN = RTFS_LIVE_ALIGN;  // floats: every slot's block of the flat output starts on a 128-byte line
// columns of the tick table
enum { T_SLOT, T_A, T_NA, T_F, T_NF, T_E, T_CNT, T_ROW0, T_O, T_END, T_OFF, T_APOS, T_FPOS, T_APTR, T_VPTR };

__device__ __forceinline__ f32x4 load4(const float* p) {  // 16 bytes when aligned, else four dwords
    if ((((uintptr_t)p) & 15) == 0) return *(const f32x4*)p;
    return f32x4{p[0], p[1], p[2], p[3]};
}

// table columns T_VPTR + k hold the chunk address of lip track k
__global__ __launch_bounds__(256) void live_ingest_frame_speakers_kernel(const long long* __restrict__ table, float* aring, float* vring,
                                                                         float* __restrict__ wav_win, float* __restrict__ video_win, int R,
                                                                         int rows, int K, int window, int hop, int C, int qa_pad, int qin_pad) {
    const int Cv = C / SPF, Wv = window / SPF;
    int q = blockIdx.y * 256 + threadIdx.x;
    if ((int)blockIdx.x >= rows) {
        // ---- ingest: the audio chunk and the K lip chunks of table row r -> rings of its slot
        const int r = blockIdx.x - rows;
        const long long slot = table[(size_t)T_SLOT * R + r];
        const int na = (int)table[(size_t)T_NA * R + r], nf = (int)table[(size_t)T_NF * R + r];
        if (q < qin_pad) {  // audio quads; padded to whole waves so no wave serves both copies
            const int j = 4 * q;
            if (j >= na) return;
            const float* src = (const float*)(uintptr_t)table[(size_t)T_APTR * R + r] + j;
            float* dst = aring + (size_t)slot * C;
            int cell = (int)table[(size_t)T_APOS * R + r] + j;  // apos < C, j < max_chunk < C: one wrap at most
            if (cell >= C) cell -= C;
            if (j + 3 < na && cell + 3 < C && (cell & 3) == 0) {
                *(f32x4*)(dst + cell) = load4(src);
            } else {
                for (int u = 0; u < 4 && j + u < na; ++u) dst[cell + u < C ? cell + u : cell + u - C] = src[u];
            }
            return;
        }
        q -= qin_pad;
        const int per = VCH * nf / 4;  // quads of one track's (512, nf) chunk: VCH % 4 == 0, a quad never serves two tracks
        if (nf == 0 || q >= K * per) return;
        const int k = q / per, qk = q - k * per;
        const float* src = (const float*)(uintptr_t)table[(size_t)(T_VPTR + k) * R + r];  // (512, nf)
        float* dst = vring + ((size_t)slot * K + k) * VCH * Cv;
        const int fpos = (int)table[(size_t)T_FPOS * R + r];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = 4 * qk + u;
            const int c = idx / nf, j = idx - c * nf;
            int cell = fpos + j;
            if (cell >= Cv) cell -= Cv;
            dst[(size_t)c * Cv + cell] = src[idx];
        }
        return;
    }
    // ---- framing: row -> (slot, window n)
    const int row = blockIdx.x;
    const int r = many_find(table + (size_t)T_ROW0 * R, R, row);  // block-uniform: scalar loads
    const int nl = row - (int)table[(size_t)T_ROW0 * R + r];
    if (nl >= (int)table[(size_t)T_CNT * R + r]) return;  // a table that does not cover this row: write nothing
    const long long slot = table[(size_t)T_SLOT * R + r], n = table[(size_t)T_E * R + r] + nl;
    const long long a0 = table[(size_t)T_A * R + r], lim_a = a0 + table[(size_t)T_NA * R + r];  // at a flush na = 0: lim_a = L
    if (q < qa_pad) {  // audio quads: the window of the row is written once, whatever K
        if (q >= window / 4) return;
        const int i = 4 * q;
        const long long p = n * hop + i;  // position in the stream: a multiple of 4
        int cell = (int)((n * hop) % C) + i;  // i < window <= C; C % 4 == 0, so a quad never wraps
        if (cell >= C) cell -= C;
        const float* ring = aring + (size_t)slot * C;
        const float* chunk = (const float*)(uintptr_t)table[(size_t)T_APTR * R + r];
        f32x4 v;
        if (p + 3 < a0) {
            v = *(const f32x4*)(ring + cell);
        } else if (p >= a0 && p + 3 < lim_a) {
            v = load4(chunk + (p - a0));
        } else {  // the quad straddles ring | chunk | zeros past L
            float e[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) e[u] = p + u >= lim_a ? 0.f : p + u >= a0 ? chunk[p + u - a0] : ring[cell + u];
            v = f32x4{e[0], e[1], e[2], e[3]};
        }
        *(f32x4*)(wav_win + (size_t)row * window + i) = v;
        return;
    }
    q -= qa_pad;
    const int per = VCH * Wv / 4;  // quads of one track's window
    if (q >= K * per) return;
    const int k = q / per, qk = q - k * per;
    const long long f0 = table[(size_t)T_F * R + r];
    const int nf = (int)table[(size_t)T_NF * R + r];
    const long long last = f0 + nf - 1, fbase = n * (hop / SPF);  // at a flush nf = 0: last = Tv - 1
    const int cell0 = (int)(fbase % Cv), cell_last = (int)(last % Cv);
    const float* ring = vring + ((size_t)slot * K + k) * VCH * Cv;
    const float* chunk = (const float*)(uintptr_t)table[(size_t)(T_VPTR + k) * R + r];
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int j = 4 * qk + u, c = j / Wv, f = j - c * Wv;
        long long fr = fbase + f;
        int cell = cell0 + f;  // f < Wv <= Cv
        if (cell >= Cv) cell -= Cv;
        if (fr > last) {
            fr = last;
            cell = cell_last;
        }
        v[u] = fr >= f0 ? chunk[(size_t)c * nf + (fr - f0)] : ring[(size_t)c * Cv + cell];
    }
    *(f32x4*)(video_win + (size_t)row * K * VCH * Wv + 4 * (size_t)q) = f32x4{v[0], v[1], v[2], v[3]};
}

__global__ __launch_bounds__(256) void live_ola_kernel(const long long* __restrict__ table, const float* __restrict__ y, float* __restrict__ out,
                                                       float* acc, int R, int n_src, int window, int hop, int C, int flush) {
    const int r = blockIdx.x, s = blockIdx.z;
    const long long e0 = table[(size_t)T_E * R + r], e1 = e0 + table[(size_t)T_CNT * R + r];
    const long long o = table[(size_t)T_O * R + r], end = table[(size_t)T_END * R + r];
    const long long hi = flush ? end : (e1 > e0 ? (e1 - 1) * hop + window : o);  // samples [o, hi) change in this tick
    const long long t = o + 4 * ((long long)blockIdx.y * 256 + threadIdx.x);      // o is a multiple of hop: the quad sits at a multiple of 4
    if (t >= hi) return;
    // the quad's four samples share their windows (hop and window are multiples of 4): n_lo .. n_hi of the windows emitted so far
    const long long th = t / hop, d = t - window + 1;
    const long long n_hi = th < e1 - 1 ? th : e1 - 1, n_lo = d <= 0 ? 0 : (d + hop - 1) / hop;
    const int V = window - hop;
    const float Vf = (float)V;
    float* cell = acc + ((size_t)table[(size_t)T_SLOT * R + r] * n_src + s) * C + (size_t)(t % C);
    float a[4] = {0.f, 0.f, 0.f, 0.f}, ws[4] = {0.f, 0.f, 0.f, 0.f};
    if (e0 >= 1 && t < (e0 - 1) * hop + window) {  // an earlier tick's windows reached these samples
        const f32x4 v = *(const f32x4*)cell;
        a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
    }
    const size_t row0 = (size_t)table[(size_t)T_ROW0 * R + r];
    for (long long n = n_lo; n <= n_hi; ++n) {  // ascending n: the order of longform_ola_kernel
        const int i = (int)(t - n * hop);
        float w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            w[k] = V == 0 ? 1.f : ola_weight(i + k, window, Vf);
            ws[k] += w[k];
        }
        if (n < e0) continue;  // already in the accumulator
        const f32x4 v = *(const f32x4*)(y + ((row0 + (size_t)(n - e0)) * n_src + s) * window + i);
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] += w[k] * vv[k];
    }
    if (t >= end) {  // a later window still reaches these samples (never at a flush)
        *(f32x4*)cell = f32x4{a[0], a[1], a[2], a[3]};
        return;
    }
    const long long idx = table[(size_t)T_OFF * R + r] + (long long)s * (end - o) + (t - o);  // block (n_src, end - o) of the flat output
    if (t + 3 < end && (idx & 3) == 0) {
        *(f32x4*)(out + idx) = f32x4{a[0] / ws[0], a[1] / ws[1], a[2] / ws[2], a[3] / ws[3]};
    } else {  // a flush whose length is not a multiple of 4: its tail, and the rows of further sources
        for (int k = 0; k < 4 && t + k < end; ++k) out[idx + k] = a[k] / ws[k];
    }
}

// K scales the video ring, n_acc the accumulator: a single-track pool has (1, n_src), a K-track pool (K, K)
__global__ __launch_bounds__(256) void live_reset_kernel(const long long* __restrict__ ids, float* __restrict__ aring, float* __restrict__ vring,
                                                         float* __restrict__ acc, int K, int n_acc, int C) {
    const size_t slot = ids ? (size_t)ids[blockIdx.x] : blockIdx.x;
    const int qa = C / 4, qv = K * (VCH * (C / SPF) / 4), qc = n_acc * (C / 4);  // the launcher bounds their sum: all below 2^31
    int q = blockIdx.y * 256 + threadIdx.x;
    const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
    if (q < qa) {
        *(f32x4*)(aring + slot * C + 4 * (size_t)q) = z;
        return;
    }
    q -= qa;
    if (q < qv) {
        *(f32x4*)(vring + slot * K * VCH * (C / SPF) + 4 * (size_t)q) = z;
        return;
    }
    q -= qv;
    if (q < qc) *(f32x4*)(acc + slot * n_acc * C + 4 * (size_t)q) = z;
}

// what live_plan and the overlap-add need of the sizes, whatever K (LAUNCH SIZES at the top)
int live_sizes_ok(int window, int hop, int max_chunk) {
    if (longform_plan(1, 1, window, hop, nullptr) != RTFS_OK) return 0;
    return max_chunk >= SPF && max_chunk % SPF == 0 && (long long)window + max_chunk <= RTFS_LIVE_MAX_CAPACITY;
}

}  // namespace

int live_speakers_sizes_ok(int window, int hop, int max_chunk, int K) {
    if (K < 1 || K > RTFS_MAX_SPEAKERS || !live_sizes_ok(window, hop, max_chunk)) return 0;
    return (long long)K * ((long long)window + max_chunk) <= RTFS_LIVE_MAX_CAPACITY;
}

int live_plan(const long long* slot_ids, const long long* counters, const long long* n_audio, const long long* n_video, int R, int slots,
              int flush, int window, int hop, int max_chunk, int n_src, long long* new_counters, long long* table, long long* sizes,
              int* refused) {
    auto refuse = [&](int r, int reason) {
        if (refused) {
            refused[0] = r;
            refused[1] = reason;
        }
        return RTFS_ERR_ARG;
    };
    if (!live_sizes_ok(window, hop, max_chunk) || !slot_ids || !counters || R < 1 || slots < 1 || n_src < 1 || (!flush && (!n_audio || !n_video)))
        return refuse(-1, RTFS_LIVE_BAD_ARGUMENT);
    const long long W = window, H = hop, Hv = hop / SPF, Wv = window / SPF, C = W + max_chunk, Cv = C / SPF, LIMIT = 1LL << 60;
    for (int r = 0; r < R; ++r) {
        if (slot_ids[r] < 0 || slot_ids[r] >= slots) return refuse(r, RTFS_LIVE_UNKNOWN_SLOT);
        for (int q = 0; q < r; ++q)
            if (slot_ids[q] == slot_ids[r]) return refuse(r, RTFS_LIVE_REPEATED_SLOT);
    }
    long long rows = 0, off = 0, max_span = 0, max_na = 0, max_nf = 0;
    // two passes, so that a refusal at any slot leaves every output unwritten: pass 0 only checks, pass 1 only writes
    for (int pass = 0; pass < 2; ++pass) {
        rows = off = max_span = max_na = max_nf = 0;
        for (int r = 0; r < R; ++r) {
            const long long a = counters[4 * r], f = counters[4 * r + 1], e = counters[4 * r + 2], o = counters[4 * r + 3];
            // what this planner itself maintains: o = e hop, windows 0 .. e - 1 were ready, the rings still hold what window e needs
            if (a < 0 || f < 0 || e < 0 || a > LIMIT || f > LIMIT || o != e * H || (e > 0 && (a < (e - 1) * H + W || f < (e - 1) * Hv + Wv)) ||
                a - e * H > C || f - e * Hv > Cv)
                return refuse(r, RTFS_LIVE_BAD_COUNTERS);
            long long na = 0, nf = 0, e1, end, span;
            if (!flush) {
                na = n_audio[r];
                nf = n_video[r];
                if (na < 0 || na > max_chunk || nf < 0 || nf > max_chunk / SPF) return refuse(r, RTFS_LIVE_CHUNK_SIZE);
                if (a + na - e * H > C) return refuse(r, RTFS_LIVE_AUDIO_CAPACITY);
                if (f + nf - e * Hv > Cv) return refuse(r, RTFS_LIVE_VIDEO_CAPACITY);
                const long long ka = a + na >= W ? (a + na - W) / H + 1 : 0, kf = f + nf >= Wv ? (f + nf - Wv) / Hv + 1 : 0;  // windows that fit
                const long long k = ka < kf ? ka : kf;
                e1 = k > e ? k : e;
                end = e1 * H;
                span = e1 > e ? (e1 - 1) * H + W - o : 0;
            } else {
                if (a > 0 && f < 1) return refuse(r, RTFS_LIVE_NO_FRAMES);
                e1 = a == 0 ? 0 : a <= W ? 1 : 1 + (a - W + H - 1) / H;  // longform_plan's N for L = a
                end = a;
                span = a - o;
            }
            if (pass && table) {
                const long long col[13] = {slot_ids[r], a, na, f, nf, e, e1 - e, rows, o, end, off, a % C, f % Cv};
                for (int k = 0; k < 13; ++k) table[(size_t)k * R + r] = col[k];
            }
            if (pass && new_counters) {
                new_counters[4 * r] = flush ? 0 : a + na;
                new_counters[4 * r + 1] = flush ? 0 : f + nf;
                new_counters[4 * r + 2] = flush ? 0 : e1;
                new_counters[4 * r + 3] = flush ? 0 : end;
            }
            rows += e1 - e;
            off += ((long long)n_src * (end - o) + LIVE_ALIGN - 1) / LIVE_ALIGN * LIVE_ALIGN;
            if (rows > 0x7fffffffLL || off > LIMIT) return refuse(r, RTFS_LIVE_BAD_ARGUMENT);
            max_span = span > max_span ? span : max_span;
            max_na = na > max_na ? na : max_na;
            max_nf = nf > max_nf ? nf : max_nf;
        }
    }
    if (sizes) {
        sizes[0] = rows;
        sizes[1] = off;
        sizes[2] = max_span;
        sizes[3] = max_na;
        sizes[4] = max_nf;
    }
    if (refused) refused[0] = -1, refused[1] = 0;
    return RTFS_OK;
}

int launch_live_overlap_add(const long long* table, const float* y, float* out, float* acc, int R, long long max_span, int n_src, int window,
                            int hop, int max_chunk, int flush, hipStream_t st) {
    if (!live_sizes_ok(window, hop, max_chunk)) return RTFS_ERR_ARG;
    const long long C = (long long)window + max_chunk;
    if (R < 1 || n_src < 1 || n_src > 65535 || max_span < 0 || max_span > C) return RTFS_ERR_SHAPE;
    if ((((uintptr_t)y) | ((uintptr_t)out) | ((uintptr_t)acc)) & 15) return RTFS_ERR_ARG;
    if (((uintptr_t)table) & 7) return RTFS_ERR_ARG;
    if (max_span == 0) return RTFS_OK;
    if ((max_span + 1023) / 1024 > 65535) return RTFS_ERR_SHAPE;
    hipLaunchKernelGGL(live_ola_kernel, dim3(R, (unsigned)((max_span + 1023) / 1024), n_src), dim3(256), 0, st, table, y, out, acc, R, n_src,
                       window, hop, (int)C, flush ? 1 : 0);
    return rtfs_launch_status();
}

int launch_live_ingest_frame_speakers(const long long* table, float* aring, float* vring, float* wav_win, float* video_win, int R, int rows,
                                      int K, int max_na, int max_nf, int window, int hop, int max_chunk, hipStream_t st) {
    if (!live_speakers_sizes_ok(window, hop, max_chunk, K)) return RTFS_ERR_ARG;
    if (R < 1 || rows < 0 || max_na < 0 || max_na > max_chunk || max_nf < 0 || max_nf > max_chunk / SPF) return RTFS_ERR_SHAPE;
    if ((((uintptr_t)aring) | ((uintptr_t)vring) | ((uintptr_t)wav_win) | ((uintptr_t)video_win)) & 15) return RTFS_ERR_ARG;
    if (((uintptr_t)table) & 7) return RTFS_ERR_ARG;
    if (rows == 0 && max_na == 0 && max_nf == 0) return RTFS_OK;  // nothing arrived, nothing is ready
    const int qa_pad = cdiv(window / 4, 64) * 64, qin_pad = cdiv(cdiv(max_na, 4), 64) * 64;
    const long long qv = (long long)K * VCH * (window / SPF) / 4, qiv = (long long)K * VCH * max_nf / 4;
    const long long frame_q = rows > 0 ? qa_pad + qv : 0, ingest_q = qin_pad + qiv;
    const bool ingest = max_na > 0 || max_nf > 0;
    const long long gy = ((frame_q > ingest_q ? frame_q : ingest_q) + 255) / 256;
    if (gy > 65535) return RTFS_ERR_SHAPE;
    hipLaunchKernelGGL(live_ingest_frame_speakers_kernel, dim3(rows + (ingest ? R : 0), (unsigned)gy), dim3(256), 0, st, table, aring, vring,
                       wav_win, video_win, R, rows, K, window, hop, window + max_chunk, qa_pad, qin_pad);
    return rtfs_launch_status();
}

int launch_live_reset(const long long* ids, float* aring, float* vring, float* acc, int R, int K, int n_acc, int window, int max_chunk,
                      hipStream_t st) {
    if (!live_speakers_sizes_ok(window, window, max_chunk, K)) return RTFS_ERR_ARG;
    if (R < 1 || n_acc < 1) return RTFS_ERR_SHAPE;
    if ((((uintptr_t)aring) | ((uintptr_t)vring) | ((uintptr_t)acc)) & 15) return RTFS_ERR_ARG;
    if (((uintptr_t)ids) & 7) return RTFS_ERR_ARG;
    const int C = window + max_chunk;
    const long long quads = (long long)C / 4 * (1 + n_acc) + (long long)K * VCH * (C / SPF) / 4;
    if ((quads + 255) / 256 > 65535) return RTFS_ERR_SHAPE;
    hipLaunchKernelGGL(live_reset_kernel, dim3(R, (unsigned)((quads + 255) / 256)), dim3(256), 0, st, ids, aring, vring, acc, K, n_acc, C);
    return rtfs_launch_status();
}

// ================================================================ faces that come and go (FaceStreamPool; DESIGN.md "Faces that come and go")
// A slot of a pool opened with max_speakers = Kmax has Kmax PLANES, laid out exactly as the K = Kmax pool above lays out its tracks (video
// ring (slots, Kmax, 512, C / SPF), accumulator (slots, Kmax, C)), and any number of them hold a face.  A face is its plane index j and
// a birth window b_j (host state, -1 = the plane is free): it takes part in window n iff n >= b_j, it is framed, separated and summed
// for those windows only, and its output is the stream [b_j hop, ..).  The slot's counters (a, f, e, o) and its readiness are shared.
//
// TICK TABLE, int64, column-major over the R named slots, RTFS_LIVE_FACES_PLAN_WORDS(Kmax) = 15 + 2 Kmax columns from live_faces_plan:
//   0 .. 12             live_plan's 13 words; row0 counts WINDOW rows (the audio windows), out_off steps by the slot's (P, end - o) block
//   13                  P: the faces present in this tick = the active faces of a push / the faces that take part in a flush
//   14                  trow0: the slot's first TARGET row (the ragged rows of video_win and y)
//   15 .. 14 + Kmax     plane of present face i, ascending (-1 behind the P-th)
//   15 + Kmax .. 14 + 2 Kmax   birth of present face i (0 behind the P-th)
// and the caller appends 1 + Kmax columns of chunk addresses [aptr | vptr of present face 0 | .. ] (0 behind the P-th) for ONE upload.
// Targets are window-major: window n of a slot holds the present faces with b <= n in ascending plane, so the target row of
// (window n, present face i) is trow0 + sum_u max(0, n - max(e, b_u)) + #{u < i : b_u <= n}: at most 16 block-uniform scalar steps.
//
// DISJOINTNESS, PER PLANE.  The audio argument is the one at the top of the file.  In plane (slot, j) a framing block reads frame q of a
// window n >= max(e, b_j) only if q < f: stream positions [max(e, b_j) hop / SPF, f); an ingest block writes [f, f + nf) of the planes
// that hold a face.  All present faces share f and e, and live_faces_plan keeps live_plan's rule f + nf - e hop / SPF <= C / SPF, so the
// cells read and written have different residues mod C / SPF in every plane.  A plane that is free, or was given to a new face, still
// holds its previous occupant's frames and sums: they are never read, because a face's first frame went in at f_add <= b_j hop / SPF and
// no window below b_j reads the plane, and an accumulator cell of plane j is read only when e > b_j and t >= b_j hop, which a tick of
// THIS face (the one that brought e above b_j) wrote.  The flush clamp reads frame f - 1 >= b_j hop / SPF, inside the face's own frames:
// a face takes part in a flush only if f > b_j hop / SPF.
namespace {

// columns of the faces table behind live_plan's 13: F_PLANE + i and F_BIRTH(Kmax) + i for present face i, then the pointer columns
enum { F_P = T_FPOS + 1, F_TROW0, F_PLANE };
__host__ __device__ constexpr int F_BIRTH(int Kmax) { return F_PLANE + Kmax; }
__host__ __device__ constexpr int F_APTR(int Kmax) { return F_PLANE + 2 * Kmax; }
__host__ __device__ constexpr int F_VPTR(int Kmax) { return F_PLANE + 2 * Kmax + 1; }

// target row of (window n, present face i); every operand is block-uniform
__device__ __forceinline__ long long faces_target_row(const long long* __restrict__ table, int R, int r, int Kmax, int P, long long e, long long n,
                                                      int i) {
    long long t = table[(size_t)F_TROW0 * R + r];
    for (int u = 0; u < P; ++u) {
        const long long b = table[(size_t)(F_BIRTH(Kmax) + u) * R + r], lo = b > e ? b : e;
        if (n > lo) t += n - lo;  // the windows [lo, n) of face u lie in front
        if (u < i && b <= n) ++t;  // and the lower faces of window n
    }
    return t;
}

__global__ __launch_bounds__(256) void live_ingest_frame_faces_kernel(const long long* __restrict__ table, float* aring, float* vring,
                                                                      float* __restrict__ wav_win, float* __restrict__ video_win, int R, int rows,
                                                                      int Kmax, int window, int hop, int C, int qa_pad, int qin_pad) {
    const int Cv = C / SPF, Wv = window / SPF;
    int q = blockIdx.y * 256 + threadIdx.x;
    if ((int)blockIdx.x >= rows) {
        // ---- ingest: the audio chunk once, the lip chunk of every present face -> its plane
        const int r = blockIdx.x - rows;
        const long long slot = table[(size_t)T_SLOT * R + r];
        const int na = (int)table[(size_t)T_NA * R + r], nf = (int)table[(size_t)T_NF * R + r];
        if (q < qin_pad) {
            const int j = 4 * q;
            if (j >= na) return;
            const float* src = (const float*)(uintptr_t)table[(size_t)F_APTR(Kmax) * R + r] + j;
            float* dst = aring + (size_t)slot * C;
            int cell = (int)table[(size_t)T_APOS * R + r] + j;
            if (cell >= C) cell -= C;
            if (j + 3 < na && cell + 3 < C && (cell & 3) == 0) {
                *(f32x4*)(dst + cell) = load4(src);
            } else {
                for (int u = 0; u < 4 && j + u < na; ++u) dst[cell + u < C ? cell + u : cell + u - C] = src[u];
            }
            return;
        }
        q -= qin_pad;
        const int per = VCH * nf / 4;  // quads of one face's (512, nf) chunk
        const int P = (int)table[(size_t)F_P * R + r];
        if (nf == 0 || q >= P * per) return;
        const int i = q / per, qk = q - i * per;
        const long long plane = table[(size_t)(F_PLANE + i) * R + r];
        const float* src = (const float*)(uintptr_t)table[(size_t)(F_VPTR(Kmax) + i) * R + r];  // (512, nf)
        float* dst = vring + ((size_t)slot * Kmax + plane) * VCH * Cv;
        const int fpos = (int)table[(size_t)T_FPOS * R + r];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = 4 * qk + u;
            const int c = idx / nf, j = idx - c * nf;
            int cell = fpos + j;
            if (cell >= Cv) cell -= Cv;
            dst[(size_t)c * Cv + cell] = src[idx];
        }
        return;
    }
    // ---- framing: window row -> (slot, window n)
    const int row = blockIdx.x;
    const int r = many_find(table + (size_t)T_ROW0 * R, R, row);
    const int nl = row - (int)table[(size_t)T_ROW0 * R + r];
    if (nl >= (int)table[(size_t)T_CNT * R + r]) return;
    const long long slot = table[(size_t)T_SLOT * R + r], e = table[(size_t)T_E * R + r], n = e + nl;
    const long long a0 = table[(size_t)T_A * R + r], lim_a = a0 + table[(size_t)T_NA * R + r];
    if (q < qa_pad) {  // the audio window, once
        if (q >= window / 4) return;
        const int i = 4 * q;
        const long long p = n * hop + i;
        int cell = (int)((n * hop) % C) + i;
        if (cell >= C) cell -= C;
        const float* ring = aring + (size_t)slot * C;
        const float* chunk = (const float*)(uintptr_t)table[(size_t)F_APTR(Kmax) * R + r];
        f32x4 v;
        if (p + 3 < a0) {
            v = *(const f32x4*)(ring + cell);
        } else if (p >= a0 && p + 3 < lim_a) {
            v = load4(chunk + (p - a0));
        } else {
            float x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = p + u >= lim_a ? 0.f : p + u >= a0 ? chunk[p + u - a0] : ring[cell + u];
            v = f32x4{x[0], x[1], x[2], x[3]};
        }
        *(f32x4*)(wav_win + (size_t)row * window + i) = v;
        return;
    }
    q -= qa_pad;
    const int per = VCH * Wv / 4;  // a multiple of 64: the face of a quad is wave-uniform
    const int P = (int)table[(size_t)F_P * R + r];
    const int want = q / per, qk = q - want * per;  // the want-th face of window n
    if (want >= P) return;
    int i = -1, seen = 0;
    for (int u = 0; u < P; ++u) {
        if (table[(size_t)(F_BIRTH(Kmax) + u) * R + r] > n) continue;
        if (seen == want) i = u;
        ++seen;
    }
    if (i < 0) return;  // window n has fewer faces
    const long long trow = faces_target_row(table, R, r, Kmax, P, e, n, i);
    const long long plane = table[(size_t)(F_PLANE + i) * R + r];
    const long long f0 = table[(size_t)T_F * R + r];
    const int nf = (int)table[(size_t)T_NF * R + r];
    const long long last = f0 + nf - 1, fbase = n * (hop / SPF);  // at a flush nf = 0: last = f - 1 >= b hop / SPF
    const int cell0 = (int)(fbase % Cv), cell_last = (int)(last % Cv);
    const float* ring = vring + ((size_t)slot * Kmax + plane) * VCH * Cv;
    const float* chunk = (const float*)(uintptr_t)table[(size_t)(F_VPTR(Kmax) + i) * R + r];
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int j = 4 * qk + u, c = j / Wv, f = j - c * Wv;
        long long fr = fbase + f;
        int cell = cell0 + f;
        if (cell >= Cv) cell -= Cv;
        if (fr > last) {
            fr = last;
            cell = cell_last;
        }
        v[u] = fr >= f0 ? chunk[(size_t)c * nf + (fr - f0)] : ring[(size_t)c * Cv + cell];
    }
    *(f32x4*)(video_win + (size_t)trow * VCH * Wv + 4 * (size_t)qk) = f32x4{v[0], v[1], v[2], v[3]};
}

// live_ola_kernel with a birth per (slot, present face): blockIdx.z = present face i
__global__ __launch_bounds__(256) void live_ola_faces_kernel(const long long* __restrict__ table, const float* __restrict__ y,
                                                             float* __restrict__ out, float* acc, int R, int Kmax, int window, int hop, int C,
                                                             int flush) {
    const int r = blockIdx.x, s = blockIdx.z;
    const int P = (int)table[(size_t)F_P * R + r];
    if (s >= P) return;
    const long long b = table[(size_t)(F_BIRTH(Kmax) + s) * R + r];
    const long long e0 = table[(size_t)T_E * R + r], e1 = e0 + table[(size_t)T_CNT * R + r];
    if (e1 <= b) return;  // no window of this face yet
    const long long o = table[(size_t)T_O * R + r], end = table[(size_t)T_END * R + r];
    const long long hi = flush ? end : (e1 > e0 ? (e1 - 1) * hop + window : o);
    const long long t = o + 4 * ((long long)blockIdx.y * 256 + threadIdx.x);
    if (t >= hi || t < b * hop) return;  // b hop is a multiple of 4: a quad lies on one side
    const long long th = t / hop, d = t - window + 1;
    const long long n_hi = th < e1 - 1 ? th : e1 - 1;
    long long n_lo = d <= 0 ? 0 : (d + hop - 1) / hop;
    if (n_lo < b) n_lo = b;
    const int V = window - hop;
    const float Vf = (float)V;
    const long long plane = table[(size_t)(F_PLANE + s) * R + r];
    float* cell = acc + ((size_t)table[(size_t)T_SLOT * R + r] * Kmax + plane) * C + (size_t)(t % C);
    float a[4] = {0.f, 0.f, 0.f, 0.f}, ws[4] = {0.f, 0.f, 0.f, 0.f};
    if (e0 > b && t < (e0 - 1) * hop + window) {  // an earlier tick's windows OF THIS FACE reached these samples
        const f32x4 v = *(const f32x4*)cell;
        a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
    }
    for (long long n = n_lo; n <= n_hi; ++n) {  // ascending n
        const int i = (int)(t - n * hop);
        float w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            w[k] = V == 0 ? 1.f : ola_weight(i + k, window, Vf);
            ws[k] += w[k];
        }
        if (n < e0) continue;  // already in the accumulator
        const f32x4 v = *(const f32x4*)(y + (size_t)faces_target_row(table, R, r, Kmax, P, e0, n, s) * window + i);
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] += w[k] * vv[k];
    }
    if (t >= end) {
        *(f32x4*)cell = f32x4{a[0], a[1], a[2], a[3]};
        return;
    }
    const long long idx = table[(size_t)T_OFF * R + r] + (long long)s * (end - o) + (t - o);  // block (P, end - o) of the flat output
    if (t + 3 < end && (idx & 3) == 0) {
        *(f32x4*)(out + idx) = f32x4{a[0] / ws[0], a[1] / ws[1], a[2] / ws[2], a[3] / ws[3]};
    } else {
        for (int k = 0; k < 4 && t + k < end; ++k) out[idx + k] = a[k] / ws[k];
    }
}

}  // namespace

int live_faces_plan(const long long* slot_ids, const long long* counters, const long long* n_audio, const long long* n_video, int R, int slots,
                    int flush, int window, int hop, int max_chunk, int Kmax, const long long* births, int row_cap, long long* new_counters,
                    long long* table, long long* row_counts, long long* sizes, int* refused) {
    auto refuse = [&](int r, int reason) {
        if (refused) {
            refused[0] = r;
            refused[1] = reason;
        }
        return RTFS_ERR_ARG;
    };
    if (!live_speakers_sizes_ok(window, hop, max_chunk, Kmax) || !slot_ids || !counters || !births || R < 1 || slots < 1 || row_cap < 0 ||
        (!flush && (!n_audio || !n_video)))
        return refuse(-1, RTFS_LIVE_BAD_ARGUMENT);
    const long long W = window, H = hop, Hv = hop / SPF, Wv = window / SPF, C = W + max_chunk, Cv = C / SPF, LIMIT = 1LL << 60;
    for (int r = 0; r < R; ++r) {
        if (slot_ids[r] < 0 || slot_ids[r] >= slots) return refuse(r, RTFS_LIVE_UNKNOWN_SLOT);
        for (int q = 0; q < r; ++q)
            if (slot_ids[q] == slot_ids[r]) return refuse(r, RTFS_LIVE_REPEATED_SLOT);
    }
    long long rows = 0, targets = 0, off = 0, max_span = 0, max_na = 0, max_nf = 0;
    // two passes as in live_plan: pass 0 only checks, pass 1 only writes
    for (int pass = 0; pass < 2; ++pass) {
        rows = targets = off = max_span = max_na = max_nf = 0;
        for (int r = 0; r < R; ++r) {
            const long long a = counters[4 * r], f = counters[4 * r + 1], e = counters[4 * r + 2], o = counters[4 * r + 3];
            const long long* bs = births + (size_t)r * Kmax;
            if (a < 0 || f < 0 || e < 0 || a > LIMIT || f > LIMIT || o != e * H || (e > 0 && (a < (e - 1) * H + W || f < (e - 1) * Hv + Wv)) ||
                a - e * H > C || f - e * Hv > Cv)
                return refuse(r, RTFS_LIVE_BAD_COUNTERS);
            for (int j = 0; j < Kmax; ++j)  // a birth is ceil(f_add / Hv) of an f_add <= f
                if (bs[j] < -1 || (bs[j] >= 0 && bs[j] > (f + Hv - 1) / Hv)) return refuse(r, RTFS_LIVE_BAD_COUNTERS);
            long long na = 0, nf = 0, e1, end, span;
            if (!flush) {
                na = n_audio[r];
                nf = n_video[r];
                if (na < 0 || na > max_chunk || nf < 0 || nf > max_chunk / SPF) return refuse(r, RTFS_LIVE_CHUNK_SIZE);
                if (a + na - e * H > C) return refuse(r, RTFS_LIVE_AUDIO_CAPACITY);
                if (f + nf - e * Hv > Cv) return refuse(r, RTFS_LIVE_VIDEO_CAPACITY);
                const long long ka = a + na >= W ? (a + na - W) / H + 1 : 0, kf = f + nf >= Wv ? (f + nf - Wv) / Hv + 1 : 0;
                const long long k = ka < kf ? ka : kf;
                e1 = k > e ? k : e;
                end = e1 * H;
                span = e1 > e ? (e1 - 1) * H + W - o : 0;
            } else {
                e1 = a == 0 ? 0 : a <= W ? 1 : 1 + (a - W + H - 1) / H;  // longform_plan's N for L = a
                end = a;
                span = a - o;
            }
            // the faces present: every active face of a push; of a flush those with a window and a frame of their own
            long long plane[RTFS_MAX_SPEAKERS], birth[RTFS_MAX_SPEAKERS];
            int P = 0;
            for (int j = 0; j < Kmax; ++j)
                if (bs[j] >= 0 && (!flush || (e1 > bs[j] && f > bs[j] * Hv))) plane[P] = j, birth[P] = bs[j], ++P;
            if (!flush && P == 0) return refuse(r, RTFS_LIVE_NO_FACES);
            if (flush && a > 0 && P == 0) return refuse(r, RTFS_LIVE_NO_FRAMES);
            if (rows + (e1 - e) > row_cap) return refuse(r, RTFS_LIVE_BAD_ARGUMENT);
            if (pass && table) {
                const long long col[15] = {slot_ids[r], a, na, f, nf, e, e1 - e, rows, o, end, off, a % C, f % Cv, P, targets};
                for (int k = 0; k < 15; ++k) table[(size_t)k * R + r] = col[k];
                for (int i = 0; i < Kmax; ++i) {
                    table[(size_t)(F_PLANE + i) * R + r] = i < P ? plane[i] : -1;
                    table[(size_t)(F_BIRTH(Kmax) + i) * R + r] = i < P ? birth[i] : 0;
                }
            }
            if (pass && new_counters) {
                new_counters[4 * r] = flush ? 0 : a + na;
                new_counters[4 * r + 1] = flush ? 0 : f + nf;
                new_counters[4 * r + 2] = flush ? 0 : e1;
                new_counters[4 * r + 3] = flush ? 0 : end;
            }
            for (long long n = e; n < e1; ++n) {
                long long c = 0;
                for (int i = 0; i < P; ++i) c += birth[i] <= n;
                if (pass && row_counts) row_counts[rows + (n - e)] = c;
                targets += c;
            }
            rows += e1 - e;
            off += ((long long)P * (end - o) + LIVE_ALIGN - 1) / LIVE_ALIGN * LIVE_ALIGN;
            if (targets > 0x7fffffffLL || off > LIMIT) return refuse(r, RTFS_LIVE_BAD_ARGUMENT);
            max_span = span > max_span ? span : max_span;
            max_na = na > max_na ? na : max_na;
            max_nf = nf > max_nf ? nf : max_nf;
        }
    }
    if (sizes) {
        sizes[0] = rows;
        sizes[1] = targets;
        sizes[2] = off;
        sizes[3] = max_span;
        sizes[4] = max_na;
        sizes[5] = max_nf;
    }
    if (refused) refused[0] = -1, refused[1] = 0;
    return RTFS_OK;
}

int launch_live_ingest_frame_faces(const long long* table, float* aring, float* vring, float* wav_win, float* video_win, int R, int rows,
                                   int Kmax, int max_na, int max_nf, int window, int hop, int max_chunk, hipStream_t st) {
    if (!live_speakers_sizes_ok(window, hop, max_chunk, Kmax)) return RTFS_ERR_ARG;
    if (R < 1 || rows < 0 || max_na < 0 || max_na > max_chunk || max_nf < 0 || max_nf > max_chunk / SPF) return RTFS_ERR_SHAPE;
    if ((((uintptr_t)aring) | ((uintptr_t)vring) | ((uintptr_t)wav_win) | ((uintptr_t)video_win)) & 15) return RTFS_ERR_ARG;
    if (((uintptr_t)table) & 7) return RTFS_ERR_ARG;
    if (rows == 0 && max_na == 0 && max_nf == 0) return RTFS_OK;  // nothing arrived, nothing is ready
    const int qa_pad = cdiv(window / 4, 64) * 64, qin_pad = cdiv(cdiv(max_na, 4), 64) * 64;
    const long long qv = (long long)Kmax * VCH * (window / SPF) / 4, qiv = (long long)Kmax * VCH * max_nf / 4;
    const long long frame_q = rows > 0 ? qa_pad + qv : 0, ingest_q = qin_pad + qiv;
    const bool ingest = max_na > 0 || max_nf > 0;
    const long long gy = ((frame_q > ingest_q ? frame_q : ingest_q) + 255) / 256;
    if (gy > 65535) return RTFS_ERR_SHAPE;
    hipLaunchKernelGGL(live_ingest_frame_faces_kernel, dim3(rows + (ingest ? R : 0), (unsigned)gy), dim3(256), 0, st, table, aring, vring, wav_win,
                       video_win, R, rows, Kmax, window, hop, window + max_chunk, qa_pad, qin_pad);
    return rtfs_launch_status();
}

int launch_live_overlap_add_faces(const long long* table, const float* y, float* out, float* acc, int R, long long max_span, int Kmax,
                                  int window, int hop, int max_chunk, int flush, hipStream_t st) {
    if (!live_speakers_sizes_ok(window, hop, max_chunk, Kmax)) return RTFS_ERR_ARG;
    const long long C = (long long)window + max_chunk;
    if (R < 1 || max_span < 0 || max_span > C) return RTFS_ERR_SHAPE;
    if ((((uintptr_t)y) | ((uintptr_t)out) | ((uintptr_t)acc)) & 15) return RTFS_ERR_ARG;
    if (((uintptr_t)table) & 7) return RTFS_ERR_ARG;
    if (max_span == 0) return RTFS_OK;
    if ((max_span + 1023) / 1024 > 65535) return RTFS_ERR_SHAPE;
    hipLaunchKernelGGL(live_ola_faces_kernel, dim3(R, (unsigned)((max_span + 1023) / 1024), Kmax), dim3(256), 0, st, table, y, out, acc, R, Kmax,
                       window, hop, (int)C, flush ? 1 : 0);
    return rtfs_launch_status();
}
