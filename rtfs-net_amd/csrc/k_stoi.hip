// Evaluation metric on the device: classic STOI (Taal et al. 2011) as pystoi 0.4.1 computes it -- the metric the reference's
// src/metrics/allwrapper.py:57-62 calls as stoi(clean, estimate, 16000, extended=False).  tests/metrics_oracle.py restates pystoi in
// float64 and names the conventions followed (frame ranges, eps, the 1e-5 short path).  Per (clean x, estimate y) row:
//   stoi_resample_kernel  pystoi utils.resample_oct = scipy.signal.resample_poly(x, 5, 8, window = h / sum(h)) at 16 kHz: the 581 taps
//                         (ideal sinc times Kaiser(beta = 0.1102 (60 - 8.7)), half length 290) are computed in double in each
//                         workgroup's prologue (no host->device copy: the call stays capturable); output n = sum_j 5 h[290 + 8n - 5j] x[j],
//                         which is resample_poly's pre-pad / pre-remove alignment written out, zero outside [0, L).  (row chunk, row, x|y)
//   stoi_mask_kernel      remove_silent_frames: windowed (hanning(258)[1:-1]) 256-sample frames at hop 128, starts range(0, L - 256, 128)
//                         (the last full frame excluded, as pystoi), clean energies 20 log10(|frame| + eps) in double, keep where
//                         max - 40 - e < 0, and a ballot prefix scan that lists the kept frame indices.  One workgroup per row.
//   stoi_bands_kernel     the STFT of the overlap-added kept frames (same window, frames, hop; rfft n = 512) restricted to bins
//                         7 .. 218, the only bins the 15 one-third-octave bands cover, and the band values sqrt(sum |X|^2).  Reduced frame
//                         j is built from the at most three kept frames it overlaps.  (frame group, row)
//   stoi_corr_kernel      intermediate intelligibility per (30-frame segment, band) in double, folded to one partial sum per workgroup.
//   stoi_final_kernel     folds a row's partials in a fixed order: d = sum / (segments * 15), or 1e-5 when fewer than 30 frames remain.
//   estoi_corr_kernel     extended STOI (Jensen & Taal 2016) on the same band values and the same work list: per 30-frame segment the
//   estoi_final_kernel    15 x 30 matrices of x and y normalised per band, then per frame, and correlated (further down; DESIGN.md,
//                         "Extended STOI"); the final stage folds its partials and, when asked, the classic ones in one launch.
// The DFT runs on the VALU in double, one bin per lane with the twiddle advanced by a complex rotation (no table, no LDS bank conflicts,
// error ~256 ulp): 212 bins x 256 samples is too small and too oddly shaped (15 unequal bands) for a matrix-core tile to pay, and double
// keeps weak bands exact next to strong ones.  No atomics: every partial has one writer and is folded in a fixed order.
// Each stage is a __forceinline__ device body working on ONE row, wrapped twice: by the stoi_*_kernel above for a (B, L) block and by a
// stoi_many_*_kernel for R recordings of different lengths, whose grid is a flat work list and whose row pointers, L10, K0 and offsets come
// from score_many_plan's table (rtfs_amd.h).  Same body, same cut of the work, same fold: a recording's result is bit-equal either way.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int SF = 256, SHOP = 128;       // frame length, hop
constexpr int NBAND = 15, SEG = 30;       // bands, frames per segment
constexpr int BIN0 = 7, NBIN = 212;       // bins 7 .. 218 (thirdoct(10000, 512, 15, 150): band 0 starts at 7, band 14 ends before 219)
constexpr int RS_UP = 5, RS_DOWN = 8, RS_HALF = 290;  // 16 kHz -> 10 kHz; ceil((60 - 8) / (28.714 / 160)) = 290
constexpr int RS_OUT = 4;                 // resampled outputs per lane
constexpr int BAND_FPW = 4;               // reduced frames per bands workgroup
// band edges [lo, hi) as bin numbers relative to BIN0 (pystoi thirdoct's argmin rule; tests/metrics_oracle.py:band_edges)
__constant__ int kBandEdge[NBAND + 1] = {7 - BIN0, 9 - BIN0, 11 - BIN0, 14 - BIN0, 17 - BIN0, 22 - BIN0, 27 - BIN0, 34 - BIN0,
                                         43 - BIN0, 55 - BIN0, 69 - BIN0, 87 - BIN0, 109 - BIN0, 138 - BIN0, 174 - BIN0, 219 - BIN0};

__device__ __forceinline__ double block_sum_256(double v, double* red, int tid) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// np.hanning(258)[1:-1][i] = 0.5 - 0.5 cos(2 pi (i + 1) / 257)
__device__ __forceinline__ double hann258(int i) { return 0.5 - 0.5 * cospi(2.0 * (i + 1) / 257.0); }

// modified Bessel function I0 by its power series (x <= 6 here: 40 terms reach double precision)
__device__ double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, s = 1.0;
    for (int k = 1; k < 40; ++k) {
        term *= q / ((double)k * k);
        s += term;
    }
    return s;
}

// Prologue of the resample kernels: the 581 taps, scaled, into LDS (ends with a barrier).
__device__ __forceinline__ void resample_taps(double* taps, double* red, int tid) {
    // pystoi _resample_window_oct: kaiser(581, beta) * sinc(t / 8) (its constant factor 2 p fc cancels in h / sum(h))
    const double beta = 0.1102 * (60.0 - 8.7), i0b = bessel_i0(beta);
    double part = 0;
    for (int i = tid; i < 2 * RS_HALF + 1; i += 256) {
        const double r = (double)(i - RS_HALF) / RS_HALF;
        const double t = (double)(i - RS_HALF) / RS_DOWN;  // sinc(2 fc t), fc = 1 / (2 max(p, q)) = 1 / 16
        const double sinc = i == RS_HALF ? 1.0 : sinpi(t) / (M_PI * t);
        const double h = bessel_i0(beta * sqrt(1.0 - r * r)) / i0b * sinc;
        taps[i] = h;
        part += h;
    }
    const double scale = RS_UP / block_sum_256(part, red, tid);  // window = h / sum(h); resample_poly multiplies it by up
    for (int i = tid; i < 2 * RS_HALF + 1; i += 256) taps[i] *= scale;
    __syncthreads();
}

// Outputs [1024 chunk, 1024 chunk + 1024) of one row: src (L) -> dst (L10).
__device__ __forceinline__ void resample_chunk(const float* __restrict__ src, float* __restrict__ dst, int L, int L10, int chunk,
                                               const double* taps, int tid) {
    const long long n0 = (long long)chunk * (256 * RS_OUT);
#pragma unroll
    for (int r = 0; r < RS_OUT; ++r) {
        const long long n = n0 + r * 256 + tid;
        if (n >= L10) break;
        const long long c = n * RS_DOWN;  // output n sits at upsampled position 8n; input j at 5j
        const long long num = c - RS_HALF;
        long long jlo = num <= 0 ? 0 : (num + RS_UP - 1) / RS_UP;
        long long jhi = (c + RS_HALF) / RS_UP;
        if (jhi > L - 1) jhi = L - 1;
        double acc = 0;
        for (long long j = jlo; j <= jhi; ++j) acc += taps[RS_HALF + (int)(c - RS_UP * j)] * (double)src[j];
        dst[n] = (float)acc;
    }
}

__global__ __launch_bounds__(256) void stoi_resample_kernel(const float* __restrict__ clean, const float* __restrict__ est, int L, int L10,
                                                            float* __restrict__ xr, float* __restrict__ yr) {
    __shared__ double taps[2 * RS_HALF + 1];
    __shared__ double red[4];
    const int tid = threadIdx.x, b = blockIdx.y;
    resample_taps(taps, red, tid);
    resample_chunk((blockIdx.z ? est : clean) + (size_t)b * L, (blockIdx.z ? yr : xr) + (size_t)b * L10, L, L10, blockIdx.x, taps, tid);
}

// One workgroup per row: clean frame energies, maximum, mask, kept index list (ascending) and its length.
__device__ __forceinline__ void mask_row(const float* __restrict__ x, int K0, double* __restrict__ e, int* __restrict__ ki,
                                         int* __restrict__ kcount, double* red, int* wcount, int tid) {
    const int lane = tid & 63, wv = tid >> 6;
    double w[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) w[r] = hann258(lane + 64 * r);
    double mx = -1e300;
    for (int f = wv; f < K0; f += 4) {  // one wave per frame
        const float* fr = x + (size_t)f * SHOP;
        double s = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double v = w[r] * (double)fr[lane + 64 * r];
            s += v * v;
        }
        s = wave_sum_d(s);
        const double en = 20.0 * log10(sqrt(s) + 2.220446049250313e-16);  // eps = float64 eps: an all-zero frame stays finite
        if (lane == 0) e[f] = en;
        mx = fmax(mx, en);
    }
    mx = wave_max_d(mx);
    if (lane == 0) red[wv] = mx;
    __syncthreads();  // also orders the energy writes above before the reads below (same workgroup)
    mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    int base = 0;
    for (int f0 = 0; f0 < K0; f0 += 256) {
        const int f = f0 + tid;
        const bool keep = f < K0 && (mx - 40.0 - e[f]) < 0;
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wcount[wv] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int q = 0; q < wv; ++q) off += wcount[q];
        if (keep) ki[off + __popcll(m & ((1ull << lane) - 1ull))] = f;
        base += wcount[0] + wcount[1] + wcount[2] + wcount[3];
        __syncthreads();
    }
    if (tid == 0) *kcount = base;
}

__global__ __launch_bounds__(256) void stoi_mask_kernel(const float* __restrict__ xr, int L10, int K0, double* __restrict__ energy,
                                                        int* __restrict__ kidx, int* __restrict__ kcount) {
    __shared__ double red[4];
    __shared__ int wcount[4];
    const int b = blockIdx.x;
    mask_row(xr + (size_t)b * L10, K0, energy + (size_t)b * K0, kidx + (size_t)b * K0, kcount + b, red, wcount, threadIdx.x);
}

// LDS of a bands workgroup
struct BandsLds {
    double sx[SF], sy[SF];
    double px[NBIN], py[NBIN];
};

// Band values of reduced frames j = BAND_FPW * group + 0 .. BAND_FPW - 1 of one row (frames j < F = K - 1 exist): x, y the row's 10 kHz
// signals, ki its kept-frame list, xb / yb its (Fmax, 15) band values.
__device__ __forceinline__ void bands_group(const float* __restrict__ x, const float* __restrict__ y, const int* __restrict__ ki, int F,
                                            int group, double* __restrict__ xb, double* __restrict__ yb, BandsLds& lds, int tid) {
    double *sx = lds.sx, *sy = lds.sy, *px = lds.px, *py = lds.py;
    const double wn = hann258(tid);
    const double wo = hann258(tid < SHOP ? tid + SHOP : tid - SHOP);  // window at the position the neighbouring frame contributes
    double cr = 1, ci = 0, sr = 1, si = 0;
    if (tid < NBIN) sincospi(2.0 * (BIN0 + tid) / 512.0, &si, &sr);  // rotation by -2 pi k / 512 (sign of |X| is irrelevant)
    for (int q = 0; q < BAND_FPW; ++q) {
        const int j = group * BAND_FPW + q;
        if (j >= F) break;  // uniform over the workgroup
        // overlap-added reduced signal over [128 j, 128 j + 256): kept frames j - 1 (first half), j, j + 1 (second half)
        const size_t self = (size_t)ki[j] * SHOP + tid;
        double vx = wn * (double)x[self], vy = wn * (double)y[self];
        if (tid < SHOP) {
            if (j >= 1) {
                const size_t o = (size_t)ki[j - 1] * SHOP + tid + SHOP;
                vx += wo * (double)x[o];
                vy += wo * (double)y[o];
            }
        } else {
            const size_t o = (size_t)ki[j + 1] * SHOP + tid - SHOP;
            vx += wo * (double)x[o];
            vy += wo * (double)y[o];
        }
        __syncthreads();  // the previous frame's readers of sx / sy / px / py are done
        sx[tid] = wn * vx;  // the STFT's own window
        sy[tid] = wn * vy;
        __syncthreads();
        if (tid < NBIN) {
            double xre = 0, xim = 0, yre = 0, yim = 0;
            cr = 1;
            ci = 0;
            for (int n = 0; n < SF; ++n) {
                const double a = sx[n], c = sy[n];
                xre = fma(a, cr, xre);
                xim = fma(a, ci, xim);
                yre = fma(c, cr, yre);
                yim = fma(c, ci, yim);
                const double t = cr * sr - ci * si;
                ci = fma(cr, si, ci * sr);
                cr = t;
            }
            px[tid] = xre * xre + xim * xim;
            py[tid] = yre * yre + yim * yim;
        }
        __syncthreads();
        if (tid < 2 * NBAND) {
            const int band = tid % NBAND;
            const double* p = tid < NBAND ? px : py;
            double s = 0;
            for (int k = kBandEdge[band]; k < kBandEdge[band + 1]; ++k) s += p[k];
            (tid < NBAND ? xb : yb)[(size_t)j * NBAND + band] = sqrt(s);
        }
    }
}

__global__ __launch_bounds__(256) void stoi_bands_kernel(const float* __restrict__ xr, const float* __restrict__ yr, int L10, int K0, int Fmax,
                                                         const int* __restrict__ kidx, const int* __restrict__ kcount,
                                                         double* __restrict__ xb, double* __restrict__ yb) {
    __shared__ BandsLds lds;
    const int b = blockIdx.y;
    bands_group(xr + (size_t)b * L10, yr + (size_t)b * L10, kidx + (size_t)b * K0, kcount[b] - 1, blockIdx.x,
                xb + (size_t)b * Fmax * NBAND, yb + (size_t)b * Fmax * NBAND, lds, threadIdx.x);
}

// One lane per (segment s, band): frames s .. s + 29 of the row's (Fmax, 15) band values, K kept frames; the sum over the 256 lanes of
// work-list chunk `chunk` (exact zero past the row's own segments).
__device__ __forceinline__ double corr_chunk(const double* __restrict__ xb, const double* __restrict__ yb, int K, int chunk, double* red,
                                             int tid) {
    const int J = K - 1 - (SEG - 1);  // segments m = 30 .. F'
    const int p = chunk * 256 + tid;
    double corr = 0;
    if (J > 0 && p < J * NBAND) {
        const int s = p / NBAND, band = p % NBAND;
        const double* xs = xb + (size_t)s * NBAND + band;
        const double* ys = yb + (size_t)s * NBAND + band;
        double xv[SEG], yv[SEG];
        double nx = 0, ny = 0;
#pragma unroll
        for (int t = 0; t < SEG; ++t) {
            xv[t] = xs[(size_t)t * NBAND];
            yv[t] = ys[(size_t)t * NBAND];
            nx += xv[t] * xv[t];
            ny += yv[t] * yv[t];
        }
        const double eps = 2.220446049250313e-16;
        const double a = sqrt(nx) / (sqrt(ny) + eps);
        const double clip = 1.0 + 5.623413251903491;  // 1 + 10^(15 / 20)
        double mx = 0, my = 0;
#pragma unroll
        for (int t = 0; t < SEG; ++t) {
            yv[t] = fmin(yv[t] * a, xv[t] * clip);
            mx += xv[t];
            my += yv[t];
        }
        mx /= SEG;
        my /= SEG;
        double sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int t = 0; t < SEG; ++t) {
            const double u = xv[t] - mx, v = yv[t] - my;
            sxx += u * u;
            syy += v * v;
            sxy += u * v;
        }
        corr = sxy / ((sqrt(sxx) + eps) * (sqrt(syy) + eps));
    }
    return block_sum_256(corr, red, tid);
}

__global__ __launch_bounds__(256) void stoi_corr_kernel(const double* __restrict__ xb, const double* __restrict__ yb, int Fmax,
                                                        const int* __restrict__ kcount, int nchunk, double* __restrict__ partial) {
    __shared__ double red[4];
    const int tid = threadIdx.x, b = blockIdx.y;
    const double corr = corr_chunk(xb + (size_t)b * Fmax * NBAND, yb + (size_t)b * Fmax * NBAND, kcount[b], blockIdx.x, red, tid);
    if (tid == 0) partial[(size_t)b * nchunk + blockIdx.x] = corr;
}

// Folds a row's nchunk partials (lane c % 256 takes partial c, then the block sum): read only when the row has a segment.  `per` = terms
// per segment the mean runs over: NBAND for classic STOI, SEG for extended STOI.
__device__ __forceinline__ void final_row(const double* __restrict__ partial, int nchunk, int K, int per, float* __restrict__ d,
                                          int* __restrict__ kept, double* red, int tid) {
    const int J = K - 1 - (SEG - 1);
    double s = 0;
    if (J > 0)
        for (int c = tid; c < nchunk; c += 256) s += partial[c];
    s = block_sum_256(s, red, tid);
    if (tid == 0) {
        *d = J > 0 ? (float)(s / ((double)J * per)) : 1e-5f;  // pystoi returns 1e-5 below 30 frames
        *kept = K;
    }
}

__global__ __launch_bounds__(256) void stoi_final_kernel(const double* __restrict__ partial, int nchunk, const int* __restrict__ kcount,
                                                         float* __restrict__ d, int* __restrict__ kept) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    final_row(partial + (size_t)b * nchunk, nchunk, kcount[b], NBAND, d + b, kept + b, red, threadIdx.x);
}

// ---------------------------------------------------------------- extended STOI (Jensen & Taal 2016; pystoi 0.4.1 extended=True)
// Same stages up to the band values; then each 30-frame segment's 15 x 30 matrix of x and of y is normalised per band (minus the mean
// over the 30 frames, divided by the Euclidean norm) and then per frame (minus the mean over the 15 bands, divided by the norm), and
// d = sum(x_n * y_n) / 30 / J.  Two deliberate differences from pystoi (tests/estoi_oracle.py): its eps * standard_normal
// noise terms are left out (they move d by ~1e-16), and a norm of exactly zero gives the inverse 0, so silent rows score exactly 0.0 and
// nothing is ever NaN.  The stage runs on the classic correlation work list: chunk c owns the segments s with floor(15 s / 256) == c,
// at most 18 of them and possibly none (its partial is then an exact 0.0, written all the same).

// v + (v of the lane a DPP row pattern pairs this lane with); every lane of the wave must be active
template <int CTRL>
__device__ __forceinline__ double dpp_pair_sum(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return v + __hiloint2double(hi, lo);
}

// Sum over the 16 lanes of a segment's group = one DPP row: the xor butterfly 1, 2, 4, 8 written as quad_perm [1,0,3,2], quad_perm
// [2,3,0,1], row_half_mirror (lane i <-> 7 - i: the other quad, whose four lanes agree by then) and row_mirror (i <-> 15 - i: the
// other half).  Register moves, no LDS round trip as with ds_bpermute; each step pairs two lanes that hold a + b and b + a, so every
// lane ends with the same bits.
__device__ __forceinline__ double group16_sum(double v) {
    v = dpp_pair_sum<0xB1>(v);
    v = dpp_pair_sum<0x4E>(v);
    v = dpp_pair_sum<0x141>(v);
    return dpp_pair_sum<0x140>(v);
}

__device__ __forceinline__ double inv_or_zero(double sumsq) {
    const double n = sqrt(sumsq);
    return n > 0 ? 1.0 / n : 0.0;
}

// One segment per 16-lane group, lane = band (lane 15 and the lanes of a group without a segment carry zeros and load nothing): frames
// s .. s + 29 of the row's (Fmax, 15) band values -> this lane's share of sum(x_n * y_n).  Executed by whole waves (shuffles).
__device__ __forceinline__ double estoi_segment(const double* __restrict__ xb, const double* __restrict__ yb, int s, int band, bool live) {
    double xv[SEG], yv[SEG];
    double mx = 0, my = 0;
#pragma unroll
    for (int t = 0; t < SEG; ++t) {
        xv[t] = live ? xb[(size_t)(s + t) * NBAND + band] : 0.0;
        yv[t] = live ? yb[(size_t)(s + t) * NBAND + band] : 0.0;
        mx += xv[t];
        my += yv[t];
    }
    mx /= SEG;
    my /= SEG;
    double nx = 0, ny = 0;
#pragma unroll
    for (int t = 0; t < SEG; ++t) {  // per band: centre over the 30 frames
        xv[t] -= mx;
        yv[t] -= my;
        nx += xv[t] * xv[t];
        ny += yv[t] * yv[t];
    }
    const double ix = inv_or_zero(nx), iy = inv_or_zero(ny);
    const bool isband = band < NBAND;
    double acc = 0;
#pragma unroll
    for (int t = 0; t < SEG; ++t) {  // per frame: centre over the 15 bands (mean first, then the squares of the centred values)
        const double u = xv[t] * ix, v = yv[t] * iy;
        const double mu = group16_sum(u) / NBAND, mv = group16_sum(v) / NBAND;  // by all 16 lanes: no shuffle under a lane condition
        const double cu = isband ? u - mu : 0.0;
        const double cv = isband ? v - mv : 0.0;
        const double iu = inv_or_zero(group16_sum(cu * cu)), iv = inv_or_zero(group16_sum(cv * cv));
        acc += (cu * iu) * (cv * iv);
    }
    return acc;
}

// Sum over the segments work-list chunk `chunk` owns (K kept frames): groups 0 .. 15 take its slots 0 .. 15, groups 0 and 1 of wave 0
// its slots 16 and 17 in a second trip.
__device__ __forceinline__ double estoi_corr_chunk(const double* __restrict__ xb, const double* __restrict__ yb, int K, int chunk,
                                                   double* red, int tid) {
    const int J = K - 1 - (SEG - 1);
    const int s_lo = cdiv(chunk * 256, NBAND);
    int s_hi = cdiv((chunk + 1) * 256, NBAND);  // s_hi - s_lo <= 18
    s_hi = s_hi < J ? s_hi : J;
    const int g = tid >> 4, band = tid & 15;
    double acc = estoi_segment(xb, yb, s_lo + g, band, band < NBAND && s_lo + g < s_hi);
    if (tid < 64 && s_lo + 16 < s_hi)  // uniform over wave 0
        acc += estoi_segment(xb, yb, s_lo + 16 + g, band, band < NBAND && g < 2 && s_lo + 16 + g < s_hi);
    return block_sum_256(acc, red, tid);
}

__global__ __launch_bounds__(256) void estoi_corr_kernel(const double* __restrict__ xb, const double* __restrict__ yb, int Fmax,
                                                         const int* __restrict__ kcount, int nchunk, double* __restrict__ partial) {
    __shared__ double red[4];
    const int tid = threadIdx.x, b = blockIdx.y;
    const double corr = estoi_corr_chunk(xb + (size_t)b * Fmax * NBAND, yb + (size_t)b * Fmax * NBAND, kcount[b], blockIdx.x, red, tid);
    if (tid == 0) partial[(size_t)b * nchunk + blockIdx.x] = corr;
}

// Extended STOI of one row from its partials pe and, with dc, classic STOI from its partials pc (final_row twice, uniform branch).
__device__ __forceinline__ void estoi_final_row(const double* __restrict__ pe, const double* __restrict__ pc, int nchunk, int K,
                                                float* __restrict__ de, float* __restrict__ dc, int* __restrict__ kept, double* red, int tid) {
    final_row(pe, nchunk, K, SEG, de, kept, red, tid);
    if (dc) final_row(pc, nchunk, K, NBAND, dc, kept, red, tid);  // block_sum_256 opens with a barrier: the reads of red above are done
}

__global__ __launch_bounds__(256) void estoi_final_kernel(const double* __restrict__ pe, const double* __restrict__ pc, int nchunk,
                                                          const int* __restrict__ kcount, float* __restrict__ de, float* __restrict__ dc,
                                                          int* __restrict__ kept) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    estoi_final_row(pe + (size_t)b * nchunk, dc ? pc + (size_t)b * nchunk : nullptr, nchunk, kcount[b], de + b, dc ? dc + b : nullptr,
                    kept + b, red, threadIdx.x);
}

// ---------------------------------------------------------------- many recordings of different lengths (score_many_plan's table)
// Column c of the table is table[c * (R + 1) + r]; row R holds the totals of the offset and work-list columns (rtfs_amd.h).

struct ScoreRec {
    int r, item;  // recording and the work item's index inside it
};

// Recording of entry w of a flat work list: the last r with first[r] <= w (first = a work-list column, ascending, first[R] = the total).
__device__ __forceinline__ ScoreRec score_find(const int* __restrict__ first, int R, int w) {
    int lo = 0, hi = R;  // invariant: first[lo] <= w < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= w) lo = mid; else hi = mid;
    }
    return {lo, w - first[lo]};
}

__global__ __launch_bounds__(256) void stoi_many_resample_kernel(const float* const* __restrict__ cleans, const float* const* __restrict__ ests,
                                                                 const int* __restrict__ table, int R, float* __restrict__ xr,
                                                                 float* __restrict__ yr) {
    __shared__ double taps[2 * RS_HALF + 1];
    __shared__ double red[4];
    const int tid = threadIdx.x, R1 = R + 1;
    resample_taps(taps, red, tid);
    const ScoreRec w = score_find(table + SC_RS0 * R1, R, blockIdx.x);
    const size_t off = (size_t)table[SC_RS_OFF * R1 + w.r];
    resample_chunk((blockIdx.y ? ests : cleans)[w.r], (blockIdx.y ? yr : xr) + off, table[SC_L * R1 + w.r], table[SC_L10 * R1 + w.r], w.item,
                   taps, tid);
}

// x / y of recording r at 10 kHz: the resampled copy, or the recording itself at fs = 10000
__device__ __forceinline__ const float* score_row10(const float* const* __restrict__ rows, const float* __restrict__ res, const int* table,
                                                    int R1, int r) {
    return res ? res + (size_t)table[SC_RS_OFF * R1 + r] : rows[r];
}

__global__ __launch_bounds__(256) void stoi_many_mask_kernel(const float* const* __restrict__ cleans, const float* __restrict__ xr,
                                                             const int* __restrict__ table, int R, double* __restrict__ energy,
                                                             int* __restrict__ kidx, int* __restrict__ kcount) {
    __shared__ double red[4];
    __shared__ int wcount[4];
    const int r = blockIdx.x, R1 = R + 1;
    const size_t fo = (size_t)table[SC_FR_OFF * R1 + r];
    mask_row(score_row10(cleans, xr, table, R1, r), table[SC_K0 * R1 + r], energy + fo, kidx + fo, kcount + r, red, wcount, threadIdx.x);
}

__global__ __launch_bounds__(256) void stoi_many_bands_kernel(const float* const* __restrict__ cleans, const float* const* __restrict__ ests,
                                                              const float* __restrict__ xr, const float* __restrict__ yr,
                                                              const int* __restrict__ table, int R, const int* __restrict__ kidx,
                                                              const int* __restrict__ kcount, double* __restrict__ xb, double* __restrict__ yb) {
    __shared__ BandsLds lds;
    const int R1 = R + 1;
    const ScoreRec w = score_find(table + SC_BG0 * R1, R, blockIdx.x);
    const size_t bo = (size_t)table[SC_BD_OFF * R1 + w.r] * NBAND;
    bands_group(score_row10(cleans, xr, table, R1, w.r), score_row10(ests, yr, table, R1, w.r), kidx + table[SC_FR_OFF * R1 + w.r],
                kcount[w.r] - 1, w.item, xb + bo, yb + bo, lds, threadIdx.x);
}

__global__ __launch_bounds__(256) void stoi_many_corr_kernel(const double* __restrict__ xb, const double* __restrict__ yb,
                                                             const int* __restrict__ table, int R, const int* __restrict__ kcount,
                                                             double* __restrict__ partial) {
    __shared__ double red[4];
    const int tid = threadIdx.x, R1 = R + 1;
    const ScoreRec w = score_find(table + SC_CC0 * R1, R, blockIdx.x);
    const size_t bo = (size_t)table[SC_BD_OFF * R1 + w.r] * NBAND;
    const double corr = corr_chunk(xb + bo, yb + bo, kcount[w.r], w.item, red, tid);
    if (tid == 0) partial[blockIdx.x] = corr;
}

__global__ __launch_bounds__(256) void stoi_many_final_kernel(const double* __restrict__ partial, const int* __restrict__ table, int R,
                                                              const int* __restrict__ kcount, float* __restrict__ d, int* __restrict__ kept) {
    __shared__ double red[4];
    const int r = blockIdx.x, R1 = R + 1;
    const int c0 = table[SC_CC0 * R1 + r];
    final_row(partial + c0, table[SC_CC0 * R1 + r + 1] - c0, kcount[r], NBAND, d + r, kept + r, red, threadIdx.x);
}

__global__ __launch_bounds__(256) void estoi_many_corr_kernel(const double* __restrict__ xb, const double* __restrict__ yb,
                                                              const int* __restrict__ table, int R, const int* __restrict__ kcount,
                                                              double* __restrict__ partial) {
    __shared__ double red[4];
    const int tid = threadIdx.x, R1 = R + 1;
    const ScoreRec w = score_find(table + SC_CC0 * R1, R, blockIdx.x);
    const size_t bo = (size_t)table[SC_BD_OFF * R1 + w.r] * NBAND;
    const double corr = estoi_corr_chunk(xb + bo, yb + bo, kcount[w.r], w.item, red, tid);
    if (tid == 0) partial[blockIdx.x] = corr;
}

__global__ __launch_bounds__(256) void estoi_many_final_kernel(const double* __restrict__ pe, const double* __restrict__ pc,
                                                               const int* __restrict__ table, int R, const int* __restrict__ kcount,
                                                               float* __restrict__ de, float* __restrict__ dc, int* __restrict__ kept) {
    __shared__ double red[4];
    const int r = blockIdx.x, R1 = R + 1;
    const int c0 = table[SC_CC0 * R1 + r];
    estoi_final_row(pe + c0, dc ? pc + c0 : nullptr, table[SC_CC0 * R1 + r + 1] - c0, kcount[r], de + r, dc ? dc + r : nullptr, kept + r, red,
                    threadIdx.x);
}

struct StoiDims {
    int L10, K0, Fmax, nchunk;
    bool resample;
};

StoiDims stoi_dims(int L, int fs) {
    StoiDims s;
    s.resample = fs != 10000;
    s.L10 = s.resample ? (int)(((long long)L * RS_UP + RS_DOWN - 1) / RS_DOWN) : L;  // resample_poly: ceil(L up / down)
    s.K0 = s.L10 > SF ? cdiv(s.L10 - SF, SHOP) : 0;
    s.Fmax = s.K0 > 0 ? s.K0 - 1 : 0;
    const int segs = s.Fmax >= SEG ? s.Fmax - (SEG - 1) : 0;
    s.nchunk = segs > 0 ? cdiv(segs * NBAND, 256) : 1;
    return s;
}

struct StoiWs {
    float *xr, *yr;
    double *energy, *xb, *yb, *partial, *partial2;
    int *kidx, *kcount;
};

// `extra`: one more region of B * nchunk partials after the classic layout (extended STOI together with classic STOI)
size_t stoi_carve(const StoiDims& s, int B, char* base, StoiWs* w, bool extra = false) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        off = align_up(off, 256);
        char* r = base ? base + off : nullptr;
        off += bytes;
        return r;
    };
    const size_t rows = s.resample ? (size_t)B * s.L10 : 0;
    w->xr = (float*)take(rows * sizeof(float));
    w->yr = (float*)take(rows * sizeof(float));
    w->energy = (double*)take((size_t)B * s.K0 * sizeof(double));
    w->kidx = (int*)take((size_t)B * s.K0 * sizeof(int));
    w->kcount = (int*)take((size_t)B * sizeof(int));
    w->xb = (double*)take((size_t)B * s.Fmax * NBAND * sizeof(double));
    w->yb = (double*)take((size_t)B * s.Fmax * NBAND * sizeof(double));
    w->partial = (double*)take((size_t)B * s.nchunk * sizeof(double));
    w->partial2 = extra ? (double*)take((size_t)B * s.nchunk * sizeof(double)) : nullptr;
    return off;
}

}  // namespace

int stoi_check_args(int B, int L, int fs) {
    if (fs != 16000 && fs != 10000) return RTFS_ERR_ARG;
    if (B < 1 || L < 1 || L > (1 << 26)) return RTFS_ERR_SHAPE;
    if (stoi_dims(L, fs).K0 < 1) return RTFS_ERR_SHAPE;  // pystoi needs one frame (np.max of no energies raises)
    return RTFS_OK;
}

size_t stoi_workspace_bytes(int B, int L, int fs) {
    if (stoi_check_args(B, L, fs) != RTFS_OK) return 0;
    StoiWs w;
    return stoi_carve(stoi_dims(L, fs), B, nullptr, &w);
}

// Stages 1 .. 3 of a (B, L) block, shared by classic and extended STOI: resample, mask, band values.
static int launch_stoi_bands(const float* clean, const float* est, int B, int L, const StoiDims& s, const StoiWs& w, hipStream_t st) {
    const float *xr = clean, *yr = est;
    if (s.resample) {
        hipLaunchKernelGGL(stoi_resample_kernel, dim3(cdiv(s.L10, 256 * RS_OUT), B, 2), dim3(256), 0, st, clean, est, L, s.L10, w.xr, w.yr);
        const int r = rtfs_launch_status();
        if (r != RTFS_OK) return r;
        xr = w.xr;
        yr = w.yr;
    }
    hipLaunchKernelGGL(stoi_mask_kernel, dim3(B), dim3(256), 0, st, xr, s.L10, s.K0, w.energy, w.kidx, w.kcount);
    int r = rtfs_launch_status();
    if (r != RTFS_OK) return r;
    if (s.Fmax > 0) {
        hipLaunchKernelGGL(stoi_bands_kernel, dim3(cdiv(s.Fmax, BAND_FPW), B), dim3(256), 0, st, xr, yr, s.L10, s.K0, s.Fmax, w.kidx, w.kcount,
                           w.xb, w.yb);
        if ((r = rtfs_launch_status()) != RTFS_OK) return r;
    }
    return RTFS_OK;
}

int launch_stoi(const float* clean, const float* est, int B, int L, int fs, void* ws, size_t ws_bytes, float* d, int* kept, hipStream_t st) {
    const int e = stoi_check_args(B, L, fs);
    if (e != RTFS_OK) return e;
    const StoiDims s = stoi_dims(L, fs);
    StoiWs w;
    if (stoi_carve(s, B, nullptr, &w) > ws_bytes) return RTFS_ERR_WORKSPACE;
    stoi_carve(s, B, (char*)ws, &w);
    int r = launch_stoi_bands(clean, est, B, L, s, w, st);
    if (r != RTFS_OK) return r;
    if (s.Fmax >= SEG) {  // otherwise every row takes the 1e-5 path and the partials are never read
        hipLaunchKernelGGL(stoi_corr_kernel, dim3(s.nchunk, B), dim3(256), 0, st, w.xb, w.yb, s.Fmax, w.kcount, s.nchunk, w.partial);
        if ((r = rtfs_launch_status()) != RTFS_OK) return r;
    }
    hipLaunchKernelGGL(stoi_final_kernel, dim3(B), dim3(256), 0, st, w.partial, s.nchunk, w.kcount, d, kept);
    return rtfs_launch_status();
}

size_t estoi_workspace_bytes(int B, int L, int fs, int with_classic) {
    if (stoi_check_args(B, L, fs) != RTFS_OK) return 0;
    StoiWs w;
    return stoi_carve(stoi_dims(L, fs), B, nullptr, &w, with_classic != 0);
}

int launch_estoi(const float* clean, const float* est, int B, int L, int fs, void* ws, size_t ws_bytes, float* d_ext, float* d_classic,
                 int* kept, hipStream_t st) {
    const int e = stoi_check_args(B, L, fs);
    if (e != RTFS_OK) return e;
    const StoiDims s = stoi_dims(L, fs);
    const bool both = d_classic != nullptr;
    StoiWs w;
    if (stoi_carve(s, B, nullptr, &w, both) > ws_bytes) return RTFS_ERR_WORKSPACE;
    stoi_carve(s, B, (char*)ws, &w, both);
    int r = launch_stoi_bands(clean, est, B, L, s, w, st);
    if (r != RTFS_OK) return r;
    double* pe = both ? w.partial2 : w.partial;  // the classic partials stay where launch_stoi keeps them
    if (s.Fmax >= SEG) {
        if (both) {
            hipLaunchKernelGGL(stoi_corr_kernel, dim3(s.nchunk, B), dim3(256), 0, st, w.xb, w.yb, s.Fmax, w.kcount, s.nchunk, w.partial);
            if ((r = rtfs_launch_status()) != RTFS_OK) return r;
        }
        hipLaunchKernelGGL(estoi_corr_kernel, dim3(s.nchunk, B), dim3(256), 0, st, w.xb, w.yb, s.Fmax, w.kcount, s.nchunk, pe);
        if ((r = rtfs_launch_status()) != RTFS_OK) return r;
    }
    hipLaunchKernelGGL(estoi_final_kernel, dim3(B), dim3(256), 0, st, pe, w.partial, s.nchunk, w.kcount, d_ext, d_classic, kept);
    return rtfs_launch_status();
}

// ---------------------------------------------------------------- many recordings: planner, ragged workspace, launches
namespace {

// The nine regions of the pooled workspace, sized by the totals in row R of the plan: each region is ONE array over all recordings
// (recording r's slice starts at its *_OFF / first-entry column), so the size grows with the sums, not with R times the longest.
size_t score_carve(const int* plan, int R, int n_src, char* base, ScoreManyWs* w) {
    const int R1 = R + 1;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        off = align_up(off, 256);
        char* r = base ? base + off : nullptr;
        off += bytes;
        return r;
    };
    const size_t rs = (size_t)plan[SC_RS_OFF * R1 + R], fr = (size_t)plan[SC_FR_OFF * R1 + R], bd = (size_t)plan[SC_BD_OFF * R1 + R];
    w->xr = (float*)take(rs * sizeof(float));
    w->yr = (float*)take(rs * sizeof(float));
    w->energy = (double*)take(fr * sizeof(double));
    w->kidx = (int*)take(fr * sizeof(int));
    w->kcount = (int*)take((size_t)R * sizeof(int));
    w->xb = (double*)take(bd * NBAND * sizeof(double));
    w->yb = (double*)take(bd * NBAND * sizeof(double));
    w->partial = (double*)take((size_t)plan[SC_CC0 * R1 + R] * sizeof(double));
    w->mom = (double*)take((size_t)plan[SC_MC0 * R1 + R] * score_moments(n_src) * sizeof(double));
    return off;
}

}  // namespace

int score_many_plan(const long long* L, int R, int n_src, int fs, int* table, size_t* ws_bytes) {
    if (!L || !table || R < 1 || n_src < 1 || n_src > 4 || (fs != 16000 && fs != 10000)) return RTFS_ERR_ARG;
    for (int r = 0; r < R; ++r)
        if (L[r] < 1 || L[r] > (1 << 26) || stoi_check_args(1, (int)L[r], fs) != RTFS_OK) return RTFS_ERR_SHAPE;
    const int R1 = R + 1;
    long long rs_off = 0, fr_off = 0, bd_off = 0, rs0 = 0, bg0 = 0, cc0 = 0, mc0 = 0;
    for (int r = 0; r <= R; ++r) {
        const long long tot[7] = {rs_off, fr_off, bd_off, rs0, bg0, cc0, mc0};
        for (int c = 0; c < 7; ++c) {
            if (tot[c] > 0x7fffffffLL) return RTFS_ERR_SHAPE;
            table[(SC_RS_OFF + c) * R1 + r] = (int)tot[c];
        }
        if (r == R) break;
        const StoiDims s = stoi_dims((int)L[r], fs);
        table[SC_L * R1 + r] = (int)L[r];
        table[SC_L10 * R1 + r] = s.L10;
        table[SC_K0 * R1 + r] = s.K0;
        table[SC_FMAX * R1 + r] = s.Fmax;
        rs_off += s.resample ? s.L10 : 0;
        fr_off += s.K0;
        bd_off += s.Fmax;
        rs0 += s.resample ? cdiv(s.L10, 256 * RS_OUT) : 0;
        bg0 += cdiv(s.Fmax, BAND_FPW);
        cc0 += s.Fmax >= SEG ? s.nchunk : 0;  // below 30 frames the row takes the 1e-5 path and has no correlation chunk
        mc0 += cdiv((int)L[r], SCORE_MOM_CHUNK);
    }
    if (mc0 * score_moments(n_src) > 0x7fffffffLL || bd_off * NBAND > 0x7fffffffLL) return RTFS_ERR_SHAPE;
    table[SC_L * R1 + R] = n_src;  // row R of the four per-recording columns records what the plan was made for
    table[SC_L10 * R1 + R] = fs;
    table[SC_K0 * R1 + R] = R;
    table[SC_FMAX * R1 + R] = 0;
    if (ws_bytes) {
        ScoreManyWs w;
        *ws_bytes = score_carve(table, R, n_src, nullptr, &w);
    }
    return RTFS_OK;
}

int score_many_carve(const int* plan, int R, int n_src, int fs, void* ws, size_t ws_bytes, ScoreManyWs* w) {
    if (!plan || !ws || R < 1 || n_src < 1 || n_src > 4 || (fs != 16000 && fs != 10000)) return RTFS_ERR_ARG;
    const int R1 = R + 1;
    if (plan[SC_L * R1 + R] != n_src || plan[SC_L10 * R1 + R] != fs || plan[SC_K0 * R1 + R] != R) return RTFS_ERR_ARG;
    if (score_carve(plan, R, n_src, nullptr, w) > ws_bytes) return RTFS_ERR_WORKSPACE;
    score_carve(plan, R, n_src, (char*)ws, w);
    return RTFS_OK;
}

// Stages 1 .. 3 of the pooled pass, shared by classic and extended STOI: resample, mask, band values.
static int launch_stoi_many_bands(const float* const* cleans, const float* const* ests, const int* table, const int* plan, int R,
                                  const ScoreManyWs& w, hipStream_t st) {
    const int R1 = R + 1;
    const int n_rs = plan[SC_RS0 * R1 + R], n_bg = plan[SC_BG0 * R1 + R];
    int r;
    const float *xr = nullptr, *yr = nullptr;  // fs = 10000: the stages read the recordings themselves
    if (n_rs > 0) {
        hipLaunchKernelGGL(stoi_many_resample_kernel, dim3(n_rs, 2), dim3(256), 0, st, cleans, ests, table, R, w.xr, w.yr);
        if ((r = rtfs_launch_status()) != RTFS_OK) return r;
        xr = w.xr;
        yr = w.yr;
    }
    hipLaunchKernelGGL(stoi_many_mask_kernel, dim3(R), dim3(256), 0, st, cleans, xr, table, R, w.energy, w.kidx, w.kcount);
    if ((r = rtfs_launch_status()) != RTFS_OK) return r;
    if (n_bg > 0) {
        hipLaunchKernelGGL(stoi_many_bands_kernel, dim3(n_bg), dim3(256), 0, st, cleans, ests, xr, yr, table, R, w.kidx, w.kcount, w.xb, w.yb);
        if ((r = rtfs_launch_status()) != RTFS_OK) return r;
    }
    return RTFS_OK;
}

int launch_stoi_many(const float* const* cleans, const float* const* ests, const int* table, const int* plan, int R, int n_src, int fs, void* ws,
                     size_t ws_bytes, float* d, int* kept, hipStream_t st) {
    ScoreManyWs w;
    int r = score_many_carve(plan, R, n_src, fs, ws, ws_bytes, &w);
    if (r != RTFS_OK) return r;
    const int n_cc = plan[SC_CC0 * (R + 1) + R];
    if ((r = launch_stoi_many_bands(cleans, ests, table, plan, R, w, st)) != RTFS_OK) return r;
    if (n_cc > 0) {
        hipLaunchKernelGGL(stoi_many_corr_kernel, dim3(n_cc), dim3(256), 0, st, w.xb, w.yb, table, R, w.kcount, w.partial);
        if ((r = rtfs_launch_status()) != RTFS_OK) return r;
    }
    hipLaunchKernelGGL(stoi_many_final_kernel, dim3(R), dim3(256), 0, st, w.partial, table, R, w.kcount, d, kept);
    return rtfs_launch_status();
}

// The pooled workspace for extended STOI: the plan's nine regions and, with classic STOI as well, a tenth of (total of column 9) partials
// appended at the next multiple of 256 (no existing offset moves).  0 for a plan that is not one of R recordings.
size_t estoi_many_workspace_bytes(const int* plan, int R, int with_classic) {
    if (!plan || R < 1) return 0;
    const int R1 = R + 1, n_src = plan[SC_L * R1 + R];
    if (plan[SC_K0 * R1 + R] != R || n_src < 1 || n_src > 4) return 0;
    ScoreManyWs w;
    const size_t nine = score_carve(plan, R, n_src, nullptr, &w);
    return with_classic ? align_up(nine, 256) + (size_t)plan[SC_CC0 * R1 + R] * sizeof(double) : nine;
}

int launch_estoi_many(const float* const* cleans, const float* const* ests, const int* table, const int* plan, int R, int n_src, int fs,
                      void* ws, size_t ws_bytes, float* d_ext, float* d_classic, int* kept, hipStream_t st) {
    const bool both = d_classic != nullptr;
    ScoreManyWs w;
    int r = score_many_carve(plan, R, n_src, fs, ws, ws_bytes, &w);  // the plan / argument checks of launch_stoi_many
    if (r != RTFS_OK) return r;
    if (both && estoi_many_workspace_bytes(plan, R, 1) > ws_bytes) return RTFS_ERR_WORKSPACE;
    const int n_cc = plan[SC_CC0 * (R + 1) + R];
    // the classic partials stay where launch_stoi_many keeps them; with both, the extended ones take the tenth region
    double* pe = both ? (double*)((char*)ws + align_up(score_carve(plan, R, n_src, nullptr, &w), 256)) : nullptr;
    score_carve(plan, R, n_src, (char*)ws, &w);
    if (!both) pe = w.partial;
    if ((r = launch_stoi_many_bands(cleans, ests, table, plan, R, w, st)) != RTFS_OK) return r;
    if (n_cc > 0) {
        if (both) {
            hipLaunchKernelGGL(stoi_many_corr_kernel, dim3(n_cc), dim3(256), 0, st, w.xb, w.yb, table, R, w.kcount, w.partial);
            if ((r = rtfs_launch_status()) != RTFS_OK) return r;
        }
        hipLaunchKernelGGL(estoi_many_corr_kernel, dim3(n_cc), dim3(256), 0, st, w.xb, w.yb, table, R, w.kcount, pe);
        if ((r = rtfs_launch_status()) != RTFS_OK) return r;
    }
    hipLaunchKernelGGL(estoi_many_final_kernel, dim3(R), dim3(256), 0, st, pe, w.partial, table, R, w.kcount, d_ext, d_classic, kept);
    return rtfs_launch_status();
}
