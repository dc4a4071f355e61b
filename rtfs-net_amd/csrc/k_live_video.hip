// Live streams from camera frames (FRCNNVideoModel.open_streams / LipStreamPool; DESIGN.md "Live streams from camera frames"): the lip
// embedding chunk by chunk.  Only the stem of the front-end is temporal (Conv3d kernel 5, padding 2; k_video.hip), so embedding q needs
// the prepared lips frames q - 2 .. q + 2 and nothing else: the state of a stream is its last four prepared frames, the look-ahead two
// frames.  tests/live_video_oracle.py restates counters, emitted ranges and the windows in numpy.
//
// Host counters per slot (kept by the caller, nothing is read back): g frames received, v embeddings emitted, side.
//   push of m frames:  g' = g + m, v' = max(v, g' - 2), emits v .. v' - 1;  side' = 1 - side when m > 0
//   flush:             emits v .. g - 1 with zero planes for frame indices >= g;  counters return to zero
// Frames with index < 0 are zero planes too.  Zero means 0.0f in the PREPARED domain, what vid_pad_kernel writes, not f(0).
//
// State per slot, device resident: hist (slots, 2, 4, 88, 88), two history buffers.  Buffer `side` holds the frames max(0, g - 4) .. g - 1,
// frame p in plane p % 4.
//
//   live_video_plan            host only, the single place with the arithmetic: counters + chunk sizes -> new counters and the tick
//                              table, 8 int64 words per named slot, column-major [slot | g | m | v | k | row0 | out_off | side]; the
//                              caller appends one column of chunk pointers and uploads the 9 R words with one copy
//   live_video_ingest_kernel   ONE launch: block x < 5 rows writes plane j = x % 5 of output frame x / 5's zero-bordered window
//                              (rows, 5, 94, 94), the stem's layout at T = 1; blocks x >= 5 rows write the new history planes
//   live_video_scatter_kernel  (n, 512) embeddings of the tick's rows -> column row - row0 of each slot's (512, k) block
//   live_video_reset_kernel    gives a slot's history (and, with timestamps, its held planes) defined contents (zeros)
//
// WHY NO BLOCK READS A HISTORY CELL THAT ANOTHER BLOCK OF THE SAME LAUNCH WRITES.  Every read of the launch - a window plane of a frame
// p < g, or a frame p < g that stays in the history because m < 4 - goes to buffer `side` of its slot; every write goes to buffer
// 1 - side of its slot, plane p % 4 for the frames p in [max(0, g' - 4), g'), which are four different residues: one writer per cell.
// Two named slots never share state, and live_video_plan refuses a slot named twice.  A push with m = 0 and a flush write no history
// (the side stays).  (One ring indexed p % 4 would have the block that writes frame g + 1 race the block that still reads frame g - 3
// when m < 4, and a ring of 8 does the same with m > 4: the read and written index ranges are m - 3 .. m + 3 apart.)
// A plane of buffer `side` is read only for a frame index in [max(0, g - 4), g): it was written by the push that made it current or
// carried over by it, so no kernel depends on what reset wrote.
//
// AT THE CAMERA'S OWN FRAME RATE (frame_rate.h; DESIGN.md "Live streams at the camera's frame rate") a slot has one more counter, n camera
// frames received, and g = P(n): everything above stays in MODEL frames.  live_video_rate_plan is live_video_plan with chunk sizes in
// camera frames; its table has one more column, n0 = the camera frames received before the push, in front of the chunk pointers.  The
// ingest kernel's RATE instantiation differs in one line: a frame p >= g comes from chunk index c(p) - n0, which is >= 0 because
// p >= g = P(n0) means c(p) >= n0, and < the chunk's camera frames because p < g + m = P(n0 + chunk).  Camera frames that no model frame
// shows are never read.  A push whose frames give no model frame (m = 0) advances n only: no history block runs for it.
//
// WITH PER-FRAME TIMESTAMPS (frame_rate.h; DESIGN.md "Live streams with per-frame timestamps") the camera frame a model frame shows is
// decided on the host from the stamps: live_video_stamp_plan is live_video_rate_plan with three more counters (the last stamp, the
// watermark W, the side of the held plane; g = G(W) once a frame has arrived), three more table columns (hside | offset into the source
// list | camera frames of the chunk) and, behind the chunk pointers, the source list: one word per newly final model frame p in
// [g, g + m), the chunk-local index of c(p) or -1 for camera frame n0 - 1, the last frame of an earlier push.  No older frame can be
// asked for (frame_rate.h: p >= G(W) admits every frame stamped <= W), but n0 - 1 need not be in the history: when its own tick was
// not final yet, no model frame has shown it.  So a slot has one more plane of state, held (slots, 2, 88, 88): buffer `hside` holds the
// prepared last camera frame received.  The ingest kernel's STAMP instantiation reads a frame p >= g from the chunk at its source index
// or, for -1, from held[slot, hside]; one more block per named slot with camera frames writes the chunk's LAST frame, prepared, into
// held[slot, 1 - hside].  A flush may finalise frames too (all of them show the held frame); it writes neither history nor held.
//
// THE HELD PLANE HAS ONE WRITER PER CELL AND NO READER IN THE SAME LAUNCH.  Every read of held - a window plane or a history plane whose
// source is -1 - goes to buffer hside of its slot; the one write goes to buffer 1 - hside of its slot, by the one held block of that
// table row, and named slots are distinct.  hside flips iff the push brought a camera frame (m_cam > 0), independently of the history
// side, which flips iff a model frame became final (m > 0): frames without a final model frame move held only, an `until` without
// frames moves the history only.  The history argument above is unchanged: a frame p >= g is read from the chunk or from held[hside],
// neither of which the launch writes.  held[hside] is read only when n0 >= 1, so a push wrote it: nothing depends on what reset wrote.
#include "common.h"
#include "frame_rate.h"
#include "kernels.h"
#include "longform_common.h"  // VCH, many_find
#include "../../include/rtfs_amd.h"  // RTFS_LIVE_*

namespace {

constexpr int LV_CROP = 88, LV_PAD = 94, LV_PLANE = LV_PAD * LV_PAD, LV_IMG = LV_CROP * LV_CROP, LV_HIST = 4, LV_WIN = 5;
constexpr int LV_ALIGN = RTFS_LIVE_ALIGN;
// columns of the tick table
enum { V_SLOT, V_G, V_M, V_V, V_K, V_ROW0, V_OFF, V_SIDE, V_PTR, V_N0 = V_PTR, V_RATE_PTR, V_HSIDE = V_RATE_PTR, V_SOFF, V_MCAM, V_STAMP_PTR,
       V_SOURCES };
// where a frame p >= g lies in the chunk: at p - g, at c(p) - n0 by the rate rule, or at the index the host's source list names
enum { LV_PLAIN, LV_RATE, LV_STAMP };

// a / b fps, reduced; 25 / 1 where the chunk already is at the model's rate
struct FrameRate {
    long long a, b;
};

// where frame p of the slot of table row r comes from in this launch: nowhere (a zero plane), buffer `side`, or the chunk
template <bool U8>
struct FrameSrc {
    const float* f;          // prepared plane (88, 88), or null
    const unsigned char* b;  // uint8 plane (H, W) at the crop offset, or null
};

template <bool U8, int MODE>
__device__ __forceinline__ FrameSrc<U8> frame_src(const long long* __restrict__ table, const float* hist, const float* held, int R, int r,
                                                  long long p, int H, int W, int dy, int dx, FrameRate fr) {
    constexpr bool RATE = MODE == LV_RATE;
    const long long g = table[(size_t)V_G * R + r], lim = g + table[(size_t)V_M * R + r];  // at a flush m = 0: frames >= g are zeros
    FrameSrc<U8> s{nullptr, nullptr};
    if (p < 0 || p >= lim) return s;
    if (p < g) {
        const size_t slot = (size_t)table[(size_t)V_SLOT * R + r], side = (size_t)table[(size_t)V_SIDE * R + r];
        s.f = hist + ((slot * 2 + side) * LV_HIST + (size_t)(p & 3)) * LV_IMG;
        return s;
    }
    if (MODE == LV_STAMP) {
        const long long i = table[(size_t)V_SOURCES * R + table[(size_t)V_SOFF * R + r] + (p - g)];
        if (i < 0) {  // camera frame n0 - 1
            const size_t slot = (size_t)table[(size_t)V_SLOT * R + r], hside = (size_t)table[(size_t)V_HSIDE * R + r];
            s.f = held + (slot * 2 + hside) * LV_IMG;
            return s;
        }
        const uintptr_t chunk = (uintptr_t)table[(size_t)V_STAMP_PTR * R + r];
        if (U8) {
            s.b = (const unsigned char*)chunk + ((size_t)i * H + dy) * W + dx;
        } else {
            s.f = (const float*)chunk + (size_t)i * LV_IMG;
        }
        return s;
    }
    // the frame's index in the chunk and the chunk's address (block-uniform)
    const size_t i = RATE ? (size_t)(fr_source(fr.a, fr.b, p) - table[(size_t)V_N0 * R + r]) : (size_t)(p - g);
    const uintptr_t chunk = (uintptr_t)table[(size_t)(RATE ? V_RATE_PTR : V_PTR) * R + r];
    if (U8) {
        s.b = (const unsigned char*)chunk + (i * H + dy) * W + dx;
    } else {
        s.f = (const float*)chunk + i * LV_IMG;
    }
    return s;
}

template <bool U8, int MODE>
__global__ __launch_bounds__(256) void live_video_ingest_kernel(const long long* __restrict__ table, float* hist, float* held,
                                                                float* __restrict__ win, int R, int rows, int hist_blocks, int H, int W, int dy,
                                                                int dx, double mean, double stdv, FrameRate fr) {
    __shared__ float lut[256];
    const int tid = threadIdx.x;
    if (U8) {  // the 256 possible values through the reference's float64 arithmetic, as lips_prepare_kernel (k_prep.hip)
        lut[tid] = (float)((((double)tid - 0.0) / 255.0 - mean) / stdv);
        __syncthreads();
    }
    if ((int)blockIdx.x < rows * LV_WIN) {
        // ---- stem input: plane j of output frame `row`
        const int row = blockIdx.x / LV_WIN, j = blockIdx.x - row * LV_WIN;
        const int r = many_find(table + (size_t)V_ROW0 * R, R, row);  // block-uniform
        const int nl = row - (int)table[(size_t)V_ROW0 * R + r];
        if (nl >= (int)table[(size_t)V_K * R + r]) return;  // a table that does not cover this row: write nothing
        const long long p = table[(size_t)V_V * R + r] + nl - 2 + j;
        const FrameSrc<U8> s = frame_src<U8, MODE>(table, hist, held, R, r, p, H, W, dy, dx, fr);
        float* dst = win + (size_t)blockIdx.x * LV_PLANE;
        for (int i = tid; i < LV_PLANE; i += 256) {
            const int yy = i / LV_PAD, y = yy - 3, x = i - yy * LV_PAD - 3;
            float v = 0.f;
            if (y >= 0 && y < LV_CROP && x >= 0 && x < LV_CROP) {
                if (s.f) v = s.f[y * LV_CROP + x];
                else if (U8 && s.b) v = lut[s.b[(size_t)y * W + x]];
            }
            dst[i] = v;
        }
        return;
    }
    if (MODE == LV_STAMP && (int)blockIdx.x >= rows * LV_WIN + hist_blocks) {
        // ---- held: the chunk's last camera frame, prepared, into buffer 1 - hside of the slot of table row r
        const int r = blockIdx.x - rows * LV_WIN - hist_blocks;
        const long long mc = table[(size_t)V_MCAM * R + r];
        if (mc <= 0) return;  // no camera frame arrived: the side stays
        const size_t slot = (size_t)table[(size_t)V_SLOT * R + r], other = 1 - (size_t)table[(size_t)V_HSIDE * R + r];
        const uintptr_t chunk = (uintptr_t)table[(size_t)V_STAMP_PTR * R + r];
        const float* sf = U8 ? nullptr : (const float*)chunk + (size_t)(mc - 1) * LV_IMG;
        const unsigned char* sb = U8 ? (const unsigned char*)chunk + ((size_t)(mc - 1) * H + dy) * W + dx : nullptr;
        float* dst = held + (slot * 2 + other) * LV_IMG;
        for (int i = tid; i < LV_IMG; i += 256) {
            const int y = i / LV_CROP, x = i - y * LV_CROP;
            dst[i] = U8 ? lut[sb[(size_t)y * W + x]] : sf[i];
        }
        return;
    }
    // ---- history: plane c of buffer 1 - side of the slot of table row r
    const int hb = blockIdx.x - rows * LV_WIN, r = hb / LV_HIST, c = hb - r * LV_HIST;
    const long long m = table[(size_t)V_M * R + r];
    if (m <= 0) return;  // nothing arrived: the side stays
    const long long g1 = table[(size_t)V_G * R + r] + m;
    const long long p = g1 - LV_HIST + ((c - (g1 - LV_HIST)) & 3);  // the frame of [g' - 4, g') that lives in plane c
    if (p < 0) return;
    const FrameSrc<U8> s = frame_src<U8, MODE>(table, hist, held, R, r, p, H, W, dy, dx, fr);
    const size_t slot = (size_t)table[(size_t)V_SLOT * R + r], other = 1 - (size_t)table[(size_t)V_SIDE * R + r];
    float* dst = hist + ((slot * 2 + other) * LV_HIST + c) * LV_IMG;
    for (int i = tid; i < LV_IMG; i += 256) {
        const int y = i / LV_CROP, x = i - y * LV_CROP;
        float v = 0.f;
        if (s.f) v = s.f[i];
        else if (U8 && s.b) v = lut[s.b[(size_t)y * W + x]];
        dst[i] = v;
    }
}

// emb (n, 512): frame i = row row_begin + i of the tick -> out[out_off + c k + (row - row0)]
__global__ __launch_bounds__(256) void live_video_scatter_kernel(const float* __restrict__ emb, const long long* __restrict__ table,
                                                                 float* __restrict__ out, int R, int row_begin) {
    const int row = row_begin + blockIdx.x;
    const int r = many_find(table + (size_t)V_ROW0 * R, R, row);
    const long long col = row - table[(size_t)V_ROW0 * R + r], k = table[(size_t)V_K * R + r];
    if (col >= k) return;
    float* dst = out + table[(size_t)V_OFF * R + r] + col;
    for (int c = threadIdx.x; c < VCH; c += 256) dst[(size_t)c * k] = emb[(size_t)blockIdx.x * VCH + c];
}

// per_slot floats of state per slot (a multiple of 4): the history, or the held planes
__global__ __launch_bounds__(256) void live_video_reset_kernel(const long long* __restrict__ ids, float* __restrict__ hist, int per_slot) {
    const size_t slot = ids ? (size_t)ids[blockIdx.x] : blockIdx.x;
    const int q = blockIdx.y * 256 + threadIdx.x;
    if (q < per_slot / 4) *(f32x4*)(hist + slot * per_slot + 4 * (size_t)q) = f32x4{0.f, 0.f, 0.f, 0.f};
}

}  // namespace

// What the planner takes and gives with per-frame timestamps: the timebase, the stamps of all chunks one behind the other in the order
// the slots are named, one `until` per named slot (null: none) and the source list it writes.
struct StampPlan {
    long long tb;
    const long long* stamps;
    const long long* until;
    long long* sources;
};

// The one planner.  rate == nullptr: the chunk sizes are model frames, 3 counters per slot (g, v, side), 8 table columns, 3 sizes.
// Otherwise n_frames and max_frames count camera frames at rate->a / rate->b fps, a slot has a fourth counter n (camera frames
// received; g == P(n)), the table a ninth column n0 = n and sizes a fourth word, the largest m in model frames.
// sp != nullptr (rate is ignored): camera frames with stamps; 7 counters per slot (g, v, side, n, last stamp, watermark W, hside), g == G(W)
// once n > 0; 12 table columns (the nine | hside | offset into the source list | camera frames of the chunk), 5 sizes (... | words of
// the source list) and one source per newly final model frame.  A flush may finalise frames as well: m = g_end - g, all from held.
static int live_video_plan_any(const long long* slot_ids, const long long* counters, const long long* n_frames, int R, int slots, int flush,
                               int max_frames, const FrameRate* rate, const StampPlan* sp, long long* new_counters, long long* table,
                               long long* sizes, int* refused) {
    const int CW = sp ? 7 : rate ? 4 : 3;
    const int TW = sp ? RTFS_LIVE_VIDEO_STAMP_PLAN_WORDS : rate ? RTFS_LIVE_VIDEO_RATE_PLAN_WORDS : RTFS_LIVE_VIDEO_PLAN_WORDS;
    auto refuse = [&](int r, int reason) {
        if (refused) {
            refused[0] = r;
            refused[1] = reason;
        }
        return RTFS_ERR_ARG;
    };
    if (!slot_ids || !counters || R < 1 || slots < 1 || max_frames < 1 || (!flush && !n_frames)) return refuse(-1, RTFS_LIVE_BAD_ARGUMENT);
    if (sp && (sp->tb < 1 || sp->tb > FR_MAX_TIMEBASE)) return refuse(-1, RTFS_LIVE_BAD_TIMEBASE);
    const long long LIMIT = 1LL << 60;
    for (int r = 0; r < R; ++r) {
        if (slot_ids[r] < 0 || slot_ids[r] >= slots) return refuse(r, RTFS_LIVE_UNKNOWN_SLOT);
        for (int q = 0; q < r; ++q)
            if (slot_ids[q] == slot_ids[r]) return refuse(r, RTFS_LIVE_REPEATED_SLOT);
    }
    long long rows = 0, off = 0, max_m = 0, max_in = 0, at = 0, soff = 0;
    // two passes, so that a refusal at any slot leaves every output unwritten: pass 0 only checks, pass 1 only writes
    for (int pass = 0; pass < 2; ++pass) {
        rows = off = max_m = max_in = at = soff = 0;
        for (int r = 0; r < R; ++r) {
            const long long g = counters[CW * r], v = counters[CW * r + 1], side = counters[CW * r + 2];
            const long long n0 = rate || sp ? counters[CW * r + 3] : g;
            if (g < 0 || v < 0 || g > LIMIT || v > g || v < (g > 2 ? g - 2 : 0) || (side != 0 && side != 1))
                return refuse(r, RTFS_LIVE_BAD_COUNTERS);
            if (!sp && rate && (n0 < 0 || n0 > FR_MAX_FRAMES || g != fr_count(rate->a, rate->b, n0))) return refuse(r, RTFS_LIVE_BAD_COUNTERS);
            long long m = 0, m_in = 0, v1;
            if (sp) {
                const long long tl = counters[CW * r + 4], Wm = counters[CW * r + 5], hs = counters[CW * r + 6], tb = sp->tb;
                if (n0 < 0 || n0 > FR_MAX_FRAMES || tl < 0 || tl >= FR_MAX_STAMP || Wm < 0 || Wm > FR_MAX_STAMP || (hs != 0 && hs != 1) ||
                    (n0 == 0 ? (g != 0 || tl != 0) : (tl > Wm || g != fr_stamp_count(tb, Wm))))
                    return refuse(r, RTFS_LIVE_BAD_COUNTERS);
                const long long u = sp->until ? sp->until[r] : 0;
                if (u < 0 || u > FR_MAX_STAMP) return refuse(r, RTFS_LIVE_BAD_STAMP);
                long long W1 = u > Wm ? u : Wm, g1, tl1 = tl;
                const long long* ts = sp->stamps ? sp->stamps + at : nullptr;
                if (!flush) {
                    m_in = n_frames[r];
                    if (m_in < 0 || m_in > max_frames) return refuse(r, RTFS_LIVE_CHUNK_SIZE);
                    if (m_in > 0 && !ts) return refuse(r, RTFS_LIVE_BAD_ARGUMENT);
                    if (n0 + m_in > FR_MAX_FRAMES) return refuse(r, RTFS_LIVE_BAD_COUNTERS);
                    long long prev = n0 > 0 ? tl : -1;
                    for (long long i = 0; i < m_in; ++i) {
                        if (ts[i] < 0 || ts[i] >= FR_MAX_STAMP) return refuse(r, RTFS_LIVE_BAD_STAMP);
                        if (ts[i] < Wm || ts[i] <= prev) return refuse(r, RTFS_LIVE_STAMP_ORDER);  // promised not to come / not increasing
                        prev = ts[i];
                    }
                    if (m_in > 0) tl1 = ts[m_in - 1], W1 = tl1 > W1 ? tl1 : W1;
                    const long long G1 = fr_stamp_count(tb, W1);
                    g1 = n0 + m_in == 0 ? 0 : (G1 > g ? G1 : g);  // nothing to show before the first camera frame
                    v1 = g1 - 2 > v ? g1 - 2 : v;
                } else {
                    const long long G1 = fr_stamp_count(tb, W1), last = fr_stamp_count(tb, tl) + 1;  // the last frame's own tick is shown
                    g1 = n0 == 0 ? 0 : (G1 > last ? (G1 > g ? G1 : g) : (last > g ? last : g));
                    v1 = g1;
                }
                m = g1 - g;
                if (m > max_frames) return refuse(r, RTFS_LIVE_TOO_MANY_FINAL);
                if (pass && sp->sources) {
                    long long j = -1;  // the last frame of the chunk whose tick is at or before p
                    for (long long p = g; p < g1; ++p) {
                        while (j + 1 < m_in && fr_stamp_shows(tb, ts[j + 1], p)) ++j;
                        sp->sources[soff + (p - g)] = j >= 0 ? j : (n0 > 0 ? -1 : 0);  // frame n0 - 1; the stream's first frame
                    }
                }
                if (pass && new_counters) {
                    const long long nc[3] = {tl1, W1, m_in > 0 ? 1 - hs : hs};
                    for (int w = 0; w < 3; ++w) new_counters[CW * r + 4 + w] = flush ? 0 : nc[w];
                }
                if (pass && table) {
                    const long long col[3] = {hs, soff, m_in};
                    for (int w = 0; w < 3; ++w) table[(size_t)(RTFS_LIVE_VIDEO_RATE_PLAN_WORDS + w) * R + r] = col[w];
                }
            } else if (!flush) {
                m = m_in = n_frames[r];
                if (m_in < 0 || m_in > max_frames) return refuse(r, RTFS_LIVE_CHUNK_SIZE);
                if (rate) {
                    if (n0 + m_in > FR_MAX_FRAMES) return refuse(r, RTFS_LIVE_BAD_COUNTERS);
                    m = fr_count(rate->a, rate->b, n0 + m_in) - g;  // the model frames these camera frames complete; may be 0
                }
                v1 = g + m - 2 > v ? g + m - 2 : v;
            } else {
                v1 = g;
            }
            const long long k = v1 - v;
            if (pass && table) {
                const long long col[RTFS_LIVE_VIDEO_RATE_PLAN_WORDS] = {slot_ids[r], g, m, v, k, rows, off, side, n0};
                for (int w = 0; w < TW && w < RTFS_LIVE_VIDEO_RATE_PLAN_WORDS; ++w) table[(size_t)w * R + r] = col[w];
            }
            if (pass && new_counters) {
                new_counters[CW * r] = flush ? 0 : g + m;
                new_counters[CW * r + 1] = flush ? 0 : v1;
                new_counters[CW * r + 2] = flush ? 0 : (m > 0 ? 1 - side : side);
                if (rate || sp) new_counters[CW * r + 3] = flush ? 0 : n0 + m_in;
            }
            rows += k;
            off += ((long long)VCH * k + LV_ALIGN - 1) / LV_ALIGN * LV_ALIGN;
            if (rows > 0x7fffffffLL / LV_WIN || off > LIMIT) return refuse(r, RTFS_LIVE_BAD_ARGUMENT);
            max_m = m > max_m ? m : max_m;
            max_in = m_in > max_in ? m_in : max_in;
            at += m_in;
            soff += sp ? m : 0;
        }
    }
    if (sizes) {
        sizes[0] = rows;
        sizes[1] = off;
        sizes[2] = max_in;
        if (rate || sp) sizes[3] = max_m;
        if (sp) sizes[4] = soff;
    }
    if (refused) refused[0] = -1, refused[1] = 0;
    return RTFS_OK;
}

int live_video_plan(const long long* slot_ids, const long long* counters, const long long* n_frames, int R, int slots, int flush,
                    int max_frames, long long* new_counters, long long* table, long long* sizes, int* refused) {
    return live_video_plan_any(slot_ids, counters, n_frames, R, slots, flush, max_frames, nullptr, nullptr, new_counters, table, sizes, refused);
}

int live_video_rate_plan(const long long* slot_ids, const long long* counters, const long long* n_frames, int R, int slots, int flush,
                         int max_frames, int rate_num, int rate_den, long long* new_counters, long long* table, long long* sizes,
                         int* refused) {
    FrameRate fr;
    if (!fr_reduce(rate_num, rate_den, &fr.a, &fr.b)) {
        if (refused) refused[0] = -1, refused[1] = RTFS_LIVE_BAD_RATE;
        return RTFS_ERR_ARG;
    }
    return live_video_plan_any(slot_ids, counters, n_frames, R, slots, flush, max_frames, &fr, nullptr, new_counters, table, sizes, refused);
}

int frame_rate_map(int rate_num, int rate_den, long long n_in, long long* n_out, long long* src) {
    long long a, b;
    if (!fr_reduce(rate_num, rate_den, &a, &b) || n_in < 0 || n_in > FR_MAX_FRAMES || !n_out) return RTFS_ERR_ARG;
    *n_out = fr_count(a, b, n_in);
    if (src)
        for (long long p = 0; p < *n_out; ++p) src[p] = fr_source(a, b, p);
    return RTFS_OK;
}

int live_video_stamp_plan(const long long* slot_ids, const long long* counters, const long long* n_frames, const long long* stamps,
                          const long long* until, int R, int slots, int flush, int max_frames, long long timebase, long long* new_counters,
                          long long* table, long long* sources, long long* sizes, int* refused) {
    const StampPlan sp{timebase, stamps, until, sources};
    return live_video_plan_any(slot_ids, counters, n_frames, R, slots, flush, max_frames, nullptr, &sp, new_counters, table, sizes, refused);
}

int timestamp_map(const long long* stamps, long long n, long long timebase, long long until, long long* n_out, long long* src) {
    if (timebase < 1 || timebase > FR_MAX_TIMEBASE || n < 0 || n > FR_MAX_FRAMES || (n > 0 && !stamps) || until < 0 || until > FR_MAX_STAMP || !n_out)
        return RTFS_ERR_ARG;
    for (long long i = 0; i < n; ++i)
        if (stamps[i] < 0 || stamps[i] >= FR_MAX_STAMP || (i > 0 && stamps[i] <= stamps[i - 1])) return RTFS_ERR_ARG;
    long long g_end = 0;
    if (n > 0) {  // the flush rule on a stream whose pushes brought every frame and whose largest `until` is this one
        const long long last = stamps[n - 1], G1 = fr_stamp_count(timebase, until > last ? until : last);
        g_end = fr_stamp_count(timebase, last) + 1;
        g_end = G1 > g_end ? G1 : g_end;
    }
    if (g_end > FR_MAX_FRAMES) return RTFS_ERR_ARG;
    *n_out = g_end;
    if (src) {
        long long j = 0;
        for (long long p = 0; p < g_end; ++p) {
            while (j + 1 < n && fr_stamp_shows(timebase, stamps[j + 1], p)) ++j;
            src[p] = j;
        }
    }
    return RTFS_OK;
}

// mode LV_STAMP: the table of live_video_stamp_plan, its chunk pointers and its source list; held is the third piece of state; a flush
// may bring model frames (max_m > 0, read from held) and writes no state
static int launch_ingest_any(const long long* table, float* hist, float* held, float* windows, int R, int rows, int max_m, int max_cam,
                             int flush, bool u8, int H, int W, int dy, int dx, double mean, double stdv, int mode, FrameRate fr, hipStream_t st) {
    const bool stamp = mode == LV_STAMP;
    if (R < 1 || rows < 0 || max_m < 0 || max_cam < 0 || (flush && !stamp && max_m != 0) || (flush && max_cam != 0)) return RTFS_ERR_SHAPE;
    if (u8) {
        if (H < LV_CROP || W < LV_CROP || H > 0x7fff || W > 0x7fff) return RTFS_ERR_SHAPE;
        if (dy < 0 || dx < 0 || dy + LV_CROP > H || dx + LV_CROP > W || !(stdv != 0.0)) return RTFS_ERR_ARG;
    }
    if (((((uintptr_t)hist) | ((uintptr_t)held) | ((uintptr_t)windows)) & 15) || (((uintptr_t)table) & 7)) return RTFS_ERR_ARG;
    if (rows == 0 && max_m == 0 && max_cam == 0) return RTFS_OK;  // nothing arrived, nothing is ready
    const long long hist_blocks = max_m > 0 && !flush ? (long long)R * LV_HIST : 0;
    const long long blocks = (long long)rows * LV_WIN + hist_blocks + (max_cam > 0 ? R : 0);
    if (blocks > 0x7fffffffLL) return RTFS_ERR_SHAPE;
    if (blocks == 0) return RTFS_OK;
    auto go = [&](auto kernel) {
        if (u8)
            hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, st, table, hist, held, windows, R, rows, (int)hist_blocks, H, W, dy,
                               dx, mean, stdv, fr);
        else
            hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, st, table, hist, held, windows, R, rows, (int)hist_blocks, LV_CROP,
                               LV_CROP, 0, 0, 0.0, 1.0, fr);
    };
    if (u8 && stamp) go(live_video_ingest_kernel<true, LV_STAMP>);
    else if (stamp) go(live_video_ingest_kernel<false, LV_STAMP>);
    else if (u8 && mode == LV_RATE) go(live_video_ingest_kernel<true, LV_RATE>);
    else if (u8) go(live_video_ingest_kernel<true, LV_PLAIN>);
    else if (mode == LV_RATE) go(live_video_ingest_kernel<false, LV_RATE>);
    else go(live_video_ingest_kernel<false, LV_PLAIN>);
    return rtfs_launch_status();
}

int launch_live_video_ingest(const long long* table, float* hist, float* windows, int R, int rows, int max_m, int flush, bool u8, int H, int W,
                             int dy, int dx, double mean, double stdv, int rate_num, int rate_den, hipStream_t st) {
    FrameRate fr{25, 1};
    const bool rate = rate_num != 0 || rate_den != 0;  // 0 / 0: the chunks hold model frames (table of 8 columns + the pointers)
    if (rate && !fr_reduce(rate_num, rate_den, &fr.a, &fr.b)) return RTFS_ERR_ARG;
    return launch_ingest_any(table, hist, nullptr, windows, R, rows, max_m, 0, flush, u8, H, W, dy, dx, mean, stdv, rate ? LV_RATE : LV_PLAIN, fr,
                             st);
}

int launch_live_video_ingest_stamp(const long long* table, float* hist, float* held, float* windows, int R, int rows, int max_m, int max_cam,
                                   int flush, bool u8, int H, int W, int dy, int dx, double mean, double stdv, hipStream_t st) {
    return launch_ingest_any(table, hist, held, windows, R, rows, max_m, max_cam, flush, u8, H, W, dy, dx, mean, stdv, LV_STAMP, FrameRate{25, 1},
                             st);
}

int launch_live_video_scatter(const float* emb, const long long* table, float* out, int R, int row_begin, int n, hipStream_t st) {
    if (R < 1 || row_begin < 0 || n < 1 || (long long)row_begin + n > 0x7fffffffLL) return RTFS_ERR_SHAPE;
    if (((((uintptr_t)emb) | ((uintptr_t)out)) & 15) || (((uintptr_t)table) & 7)) return RTFS_ERR_ARG;
    hipLaunchKernelGGL(live_video_scatter_kernel, dim3(n), dim3(256), 0, st, emb, table, out, R, row_begin);
    return rtfs_launch_status();
}

int launch_live_video_reset(const long long* ids, float* hist, int R, hipStream_t st) {
    if (R < 1) return RTFS_ERR_SHAPE;
    if ((((uintptr_t)hist) & 15) || (((uintptr_t)ids) & 7)) return RTFS_ERR_ARG;
    hipLaunchKernelGGL(live_video_reset_kernel, dim3(R, cdiv(2 * LV_HIST * LV_IMG / 4, 256)), dim3(256), 0, st, ids, hist, 2 * LV_HIST * LV_IMG);
    return rtfs_launch_status();
}

int launch_live_video_stamp_reset(const long long* ids, float* hist, float* held, int R, hipStream_t st) {
    if (R < 1) return RTFS_ERR_SHAPE;
    if (((((uintptr_t)hist) | ((uintptr_t)held)) & 15) || (((uintptr_t)ids) & 7)) return RTFS_ERR_ARG;
    if (int rc = launch_live_video_reset(ids, hist, R, st)) return rc;
    hipLaunchKernelGGL(live_video_reset_kernel, dim3(R, cdiv(2 * LV_IMG / 4, 256)), dim3(256), 0, st, ids, held, 2 * LV_IMG);
    return rtfs_launch_status();
}

extern "C" {

int rtfs_live_video_plan(const long long* slot_ids, const long long* counters, const long long* n_frames, int R, int slots, int flush,
                         int max_frames, long long* new_counters, long long* table, long long* sizes, int* refused) {
    return live_video_plan(slot_ids, counters, n_frames, R, slots, flush, max_frames, new_counters, table, sizes, refused);
}

int rtfs_live_video_ingest_u8(const long long* table, float* hist, float* windows, int R, int rows, int max_m, int flush, int H, int W,
                              int dy, int dx, double mean, double std, void* stream) {
    if (!table || !hist || (!windows && rows > 0)) return RTFS_ERR_ARG;
    return launch_live_video_ingest(table, hist, windows, R, rows, max_m, flush, true, H, W, dy, dx, mean, std, 0, 0, (hipStream_t)stream);
}

int rtfs_live_video_ingest_f32(const long long* table, float* hist, float* windows, int R, int rows, int max_m, int flush, void* stream) {
    if (!table || !hist || (!windows && rows > 0)) return RTFS_ERR_ARG;
    return launch_live_video_ingest(table, hist, windows, R, rows, max_m, flush, false, 0, 0, 0, 0, 0.0, 1.0, 0, 0, (hipStream_t)stream);
}

int rtfs_frame_rate_map(int rate_num, int rate_den, long long n_in, long long* n_out, long long* src) {
    return frame_rate_map(rate_num, rate_den, n_in, n_out, src);
}

int rtfs_live_video_rate_plan(const long long* slot_ids, const long long* counters, const long long* n_frames, int R, int slots, int flush,
                              int max_frames, int rate_num, int rate_den, long long* new_counters, long long* table, long long* sizes,
                              int* refused) {
    return live_video_rate_plan(slot_ids, counters, n_frames, R, slots, flush, max_frames, rate_num, rate_den, new_counters, table, sizes,
                                refused);
}

int rtfs_live_video_ingest_rate_u8(const long long* table, float* hist, float* windows, int R, int rows, int max_m, int flush, int H, int W,
                                   int dy, int dx, double mean, double std, int rate_num, int rate_den, void* stream) {
    if (!table || !hist || (!windows && rows > 0) || rate_num < 1 || rate_den < 1) return RTFS_ERR_ARG;
    return launch_live_video_ingest(table, hist, windows, R, rows, max_m, flush, true, H, W, dy, dx, mean, std, rate_num, rate_den,
                                    (hipStream_t)stream);
}

int rtfs_live_video_ingest_rate_f32(const long long* table, float* hist, float* windows, int R, int rows, int max_m, int flush, int rate_num,
                                    int rate_den, void* stream) {
    if (!table || !hist || (!windows && rows > 0) || rate_num < 1 || rate_den < 1) return RTFS_ERR_ARG;
    return launch_live_video_ingest(table, hist, windows, R, rows, max_m, flush, false, 0, 0, 0, 0, 0.0, 1.0, rate_num, rate_den,
                                    (hipStream_t)stream);
}

size_t rtfs_video_windows_workspace_bytes(int rows) { return video_windows_workspace_bytes(rows); }

int rtfs_video_frontend_windows_f32(const float* windows, const float* pack, const long long* table, float* out, int R, int row_begin,
                                    int n, void* ws, size_t ws_bytes, void* stream) {
    if (!windows || !pack || !table || !out || !ws) return RTFS_ERR_ARG;
    if (R < 1 || row_begin < 0 || n < 1 || (long long)row_begin + n > 0x7fffffffLL / LV_WIN) return RTFS_ERR_SHAPE;
    if (ws_bytes < video_windows_workspace_bytes(n)) return RTFS_ERR_WORKSPACE;
    if (((((uintptr_t)windows) | ((uintptr_t)out) | ((uintptr_t)ws)) & 15) || (((uintptr_t)table) & 7)) return RTFS_ERR_ARG;
    float* emb = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + video_windows_workspace_bytes(n)) - (size_t)n * VCH;
    if (int rc = video_frontend_windows(windows + (size_t)row_begin * LV_WIN * LV_PLANE, pack, emb, n, ws, ws_bytes, (hipStream_t)stream)) return rc;
    return launch_live_video_scatter(emb, table, out, R, row_begin, n, (hipStream_t)stream);
}

int rtfs_live_video_reset(const long long* ids, float* hist, int R, void* stream) {
    if (!hist) return RTFS_ERR_ARG;
    return launch_live_video_reset(ids, hist, R, (hipStream_t)stream);
}

int rtfs_timestamp_map(const long long* stamps, long long n, long long timebase, long long until, long long* n_out, long long* src) {
    return timestamp_map(stamps, n, timebase, until, n_out, src);
}

int rtfs_live_video_stamp_plan(const long long* slot_ids, const long long* counters, const long long* n_frames, const long long* stamps,
                               const long long* until, int R, int slots, int flush, int max_frames, long long timebase,
                               long long* new_counters, long long* table, long long* sources, long long* sizes, int* refused) {
    return live_video_stamp_plan(slot_ids, counters, n_frames, stamps, until, R, slots, flush, max_frames, timebase, new_counters, table,
                                 sources, sizes, refused);
}

int rtfs_live_video_ingest_stamp_u8(const long long* table, float* hist, float* held, float* windows, int R, int rows, int max_m, int max_cam,
                                    int flush, int H, int W, int dy, int dx, double mean, double std, long long timebase, void* stream) {
    if (!table || !hist || !held || (!windows && rows > 0) || timebase < 1 || timebase > FR_MAX_TIMEBASE) return RTFS_ERR_ARG;
    return launch_live_video_ingest_stamp(table, hist, held, windows, R, rows, max_m, max_cam, flush, true, H, W, dy, dx, mean, std,
                                          (hipStream_t)stream);
}

int rtfs_live_video_ingest_stamp_f32(const long long* table, float* hist, float* held, float* windows, int R, int rows, int max_m, int max_cam,
                                     int flush, long long timebase, void* stream) {
    if (!table || !hist || !held || (!windows && rows > 0) || timebase < 1 || timebase > FR_MAX_TIMEBASE) return RTFS_ERR_ARG;
    return launch_live_video_ingest_stamp(table, hist, held, windows, R, rows, max_m, max_cam, flush, false, 0, 0, 0, 0, 0.0, 1.0,
                                          (hipStream_t)stream);
}

int rtfs_live_video_stamp_reset(const long long* ids, float* hist, float* held, int R, void* stream) {
    if (!hist || !held) return RTFS_ERR_ARG;
    return launch_live_video_stamp_reset(ids, hist, held, R, (hipStream_t)stream);
}

}  // extern "C"
