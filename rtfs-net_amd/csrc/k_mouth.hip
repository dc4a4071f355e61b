// Mouth ROIs from whole camera frames (rtfs-net_amd/datas.py mouth_affine / mouth_rois; DESIGN.md "Mouth ROIs from camera frames"): what
// the reference does on the host between a face tracker's landmarks and the uint8 mouth ROIs (RTFSNet_file.py:20-73, 111-118: align_face,
// the lip bounding box, cv2.resize, grey), composed into ONE affine map per (frame, face) and ONE bilinear sampling of the source frame.
//   mouth_affine        host only: eye corners + four lip points -> the 2 x 3 map from ROI pixel (j, i) to source point (sx, sy)
//   mouth_rois_kernel   one launch for J jobs (source plane, geometry, map, destination), a grid over (job, band of output bytes)
// tests/mouth_oracle.py restates both in float64 numpy and the results are compared BIT for bit, so every operation below is an IEEE
// float64 + - * / sqrt floor rint in a fixed order.  That only holds without fused multiply-add: hipcc contracts a * b + c into one
// v_fma_f64 on the device by default (one rounding instead of two), and numpy never does.  Hence the pragma, for the whole file - the
// kernel and the host planner alike.
#pragma clang fp contract(off)
#include <math.h>

#include "../../include/rtfs_amd.h"
#include "common.h"
#include "kernels.h"

namespace {

constexpr int MJ_WORDS = RTFS_MOUTH_JOB_WORDS;
constexpr int MJ_MAX_DIM = 0x7fff;   // source frames and ROIs up to 32767 pixels a side
constexpr int MJ_MAX_OUT = 4096;     // ROI side: Ho * Wo < 2^24

// one job, 12 int64 words as the host writes them
struct MouthJob {
    const unsigned char* src;
    unsigned char* dst;
    long long H, W, pitch, fmt;  // fmt = pixel stride in bytes | order << 16 (0 grey, 1 BGR, 2 RGB)
    double A[6];
};
static_assert(sizeof(MouthJob) == MJ_WORDS * 8, "job layout");

// A tap outside the frame is 0 (warpAffine's constant border).  A colour tap becomes grey first, in OpenCV's 8-bit BGR2GRAY fixed point.
__device__ __forceinline__ double mouth_tap(const unsigned char* __restrict__ src, int H, int W, long long pitch, int pix, int order, int y,
                                            int x) {
    if ((unsigned)y >= (unsigned)H || (unsigned)x >= (unsigned)W) return 0.0;
    const unsigned char* p = src + (size_t)y * (size_t)pitch + (size_t)x * (size_t)pix;
    if (order == 0) return (double)p[0];
    const int c0 = p[0], c1 = p[1], c2 = p[2];
    const int B = order == 1 ? c0 : c2, R = order == 1 ? c2 : c0;
    return (double)((1868 * B + 9617 * c1 + 4899 * R + 8192) >> 14);
}

// A source coordinate far outside the frame is clamped IN DOUBLE to where all of its taps are still outside (so the result, 0, is
// unchanged) before it is converted to an integer.  Written so that a NaN lands on the lower bound.
__device__ __forceinline__ double mouth_clamp(double s, int n) {
    const double hi = (double)n + 1.0;
    return !(s >= -2.0) ? -2.0 : (s > hi ? hi : s);
}

__device__ __forceinline__ unsigned mouth_pixel(const unsigned char* __restrict__ src, int H, int W, long long pitch, int pix, int order,
                                                double a00, double a01, double a02, double a10, double a11, double a12, int i, int j) {
    const double dj = (double)j, di = (double)i;
    const double sx = mouth_clamp((a00 * dj + a01 * di) + a02, W);
    const double sy = mouth_clamp((a10 * dj + a11 * di) + a12, H);
    const double x0 = floor(sx), y0 = floor(sy);
    const double fx = sx - x0, fy = sy - y0;
    const int ix = (int)x0, iy = (int)y0;
    const double p00 = mouth_tap(src, H, W, pitch, pix, order, iy, ix), p01 = mouth_tap(src, H, W, pitch, pix, order, iy, ix + 1);
    const double p10 = mouth_tap(src, H, W, pitch, pix, order, iy + 1, ix), p11 = mouth_tap(src, H, W, pitch, pix, order, iy + 1, ix + 1);
    const double gx = 1.0 - fx, gy = 1.0 - fy;
    const double v = gy * (gx * p00 + fx * p01) + fy * (gx * p10 + fx * p11);
    double r = rint(v);  // ties to even
    r = r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r);
    return (unsigned)(int)r;
}

// Workgroup = (job, band).  The ROI plane of a job is Ho * Wo contiguous bytes from dst; it is cut into UNITS, the aligned dwords of
// memory that hold at least one of its bytes (unit u = the dword at (dst - (dst & 3)) + 4 u), and a band is `upb` consecutive units.  A
// lane forms the up to four pixels of a unit - consecutive j, wrapping into the next row where Wo is no multiple of 4 - and stores one
// dword; only the first and last unit of a plane that starts or ends off the dword grid fall back to byte stores of their own bytes.
// Adjacent lanes hold adjacent j, so for an upright face their taps are neighbours in the source.  The job's geometry and its six
// matrix entries are block-uniform: the compiler fetches them once with scalar loads and keeps them in SGPRs.  No LDS, no atomics, one
// writer per byte, nothing read back: deterministic and graph-capturable.
__global__ __launch_bounds__(256) void mouth_rois_kernel(const MouthJob* __restrict__ jobs, int Ho, int Wo, int bpj, int upb) {
    const int job = blockIdx.x / bpj, band = blockIdx.x - job * bpj;
    const MouthJob* __restrict__ jb = jobs + job;
    const unsigned char* __restrict__ src = jb->src;
    unsigned char* __restrict__ dst = jb->dst;
    const int H = (int)jb->H, W = (int)jb->W, pix = (int)(jb->fmt & 0xffff), order = (int)(jb->fmt >> 16);
    const long long pitch = jb->pitch;
    const double a00 = jb->A[0], a01 = jb->A[1], a02 = jb->A[2], a10 = jb->A[3], a11 = jb->A[4], a12 = jb->A[5];
    const int N = Ho * Wo, s = (int)((uintptr_t)dst & 3);
    const int units = (N + s + 3) >> 2;
    const int u_hi = min(units, (band + 1) * upb);
    for (int u = band * upb + (int)threadIdx.x; u < u_hi; u += 256) {
        const int f0 = 4 * u - s;
        int i = f0 >= 0 ? f0 / Wo : 0, j = f0 >= 0 ? f0 - i * Wo : 0;  // of the unit's first byte inside the plane
        unsigned word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int f = f0 + k;
            if (f >= 0 && f < N) {
                word |= mouth_pixel(src, H, W, pitch, pix, order, a00, a01, a02, a10, a11, a12, i, j) << (8 * k);
                if (++j == Wo) {
                    j = 0;
                    ++i;
                }
            }
        }
        if (f0 >= 0 && f0 + 4 <= N) {
            *(unsigned*)(dst + f0) = word;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (f0 + k >= 0 && f0 + k < N) dst[f0 + k] = (unsigned char)(word >> (8 * k));
        }
    }
}

bool mouth_finite(const double* v, int n) {
    for (int i = 0; i < n; ++i)
        if (!isfinite(v[i])) return false;
    return true;
}

}  // namespace

// ================================================================ the planner (host only)
int mouth_affine(const double* eyes, const double* lips, long long n, int out_h, int out_w, int crop_h, int crop_w, double* A,
                 long long* refused) {
    if (refused) *refused = -1;
    if (!eyes || !lips || !A || n < 0) return RTFS_ERR_ARG;
    if (crop_h < 1 || crop_w < 1 || crop_h > out_h || crop_w > out_w || out_h > MJ_MAX_OUT || out_w > MJ_MAX_OUT) return RTFS_ERR_ARG;
    const double tx = 0.5 * 256.0, ty = 0.35 * 256.0;  // the reference's eye position in its 256 x 256 aligned face: (128, 89.6)
    const double span = 0.3 * 256.0;                   // ... and its distance between the eye corners: (1 - 2 * 0.35) * 256
    const double offx = 0.5 - (double)(out_w - crop_w) / 2.0, offy = 0.5 - (double)(out_h - crop_h) / 2.0;
    for (long long f = 0; f < n; ++f) {
        const double* e = eyes + 4 * f;
        const double* l = lips + 8 * f;
        double* M = A + 6 * f;
        if (refused) *refused = f;
        if (!mouth_finite(e, 4) || !mouth_finite(l, 8)) return RTFS_ERR_ARG;
        const double xl = e[0], yl = e[1], xr = e[2], yr = e[3];
        const double dx = xr - xl, dy = yr - yl;
        const double dist = sqrt(dx * dx + dy * dy);
        if (!(dist > 0.0)) return RTFS_ERR_ARG;
        const double s = span / dist;
        const double a = s * (dx / dist), b = s * (dy / dist);
        const double cx = (xl + xr) / 2.0, cy = (yl + yr) / 2.0;
        double qx0 = 0, qx1 = 0, qy0 = 0, qy1 = 0;
        for (int k = 0; k < 4; ++k) {  // the lip points in the aligned face: q = R (p - c) + t, R = [[a, b], [-b, a]]
            const double ux = l[2 * k] - cx, uy = l[2 * k + 1] - cy;
            const double qx = (a * ux + b * uy) + tx, qy = (a * uy - b * ux) + ty;
            qx0 = k == 0 || qx < qx0 ? qx : qx0;
            qx1 = k == 0 || qx > qx1 ? qx : qx1;
            qy0 = k == 0 || qy < qy0 ? qy : qy0;
            qy1 = k == 0 || qy > qy1 ? qy : qy1;
        }
        const double w = (qx1 - qx0) + 1.0, h = (qy1 - qy0) + 1.0;  // boundingRect
        const double kx = w / (double)crop_w, ky = h / (double)crop_h;
        const double n2 = a * a + b * b;
        // ROI pixel (j, i) shows the aligned point q = (qx0 + (j + offx) kx - 0.5, qy0 + (i + offy) ky - 0.5): cv2.resize's pixel-centre
        // rule with the box in the central crop; its source point is p = c + R^T (q - t) / |R|.  The matrix is read off that map at three
        // ROI pixels, the origin and one step along each axis (for an upright face at scale 1 its entries are then exact integers).
        double P[3][2];
        for (int k = 0; k < 3; ++k) {
            const double j = k == 1 ? 1.0 : 0.0, i = k == 2 ? 1.0 : 0.0;
            const double gx = ((qx0 + (j + offx) * kx) - 0.5) - tx, gy = ((qy0 + (i + offy) * ky) - 0.5) - ty;
            P[k][0] = cx + (a * gx - b * gy) / n2;
            P[k][1] = cy + (b * gx + a * gy) / n2;
        }
        M[0] = P[1][0] - P[0][0];
        M[1] = P[2][0] - P[0][0];
        M[2] = P[0][0];
        M[3] = P[1][1] - P[0][1];
        M[4] = P[2][1] - P[0][1];
        M[5] = P[0][1];
        if (!mouth_finite(M, 6)) return RTFS_ERR_ARG;
    }
    if (refused) *refused = -1;
    return RTFS_OK;
}

// ================================================================ the launcher
// jobs: the DEVICE table; host_jobs: the same words on the host, or NULL.  With host_jobs every job is checked here, before the launch.
int launch_mouth_rois(const long long* jobs, const long long* host_jobs, int J, int out_h, int out_w, hipStream_t st) {
    if (!jobs || (((uintptr_t)jobs) & 7)) return RTFS_ERR_ARG;
    if (J < 1 || out_h < 1 || out_w < 1 || out_h > MJ_MAX_OUT || out_w > MJ_MAX_OUT) return RTFS_ERR_SHAPE;
    if (host_jobs) {
        for (int r = 0; r < J; ++r) {
            const long long* w = host_jobs + (size_t)MJ_WORDS * r;
            const long long H = w[2], W = w[3], pitch = w[4], pix = w[5] & 0xffff, order = w[5] >> 16;
            if (!w[0] || !w[1] || H < 1 || W < 1 || H > MJ_MAX_DIM || W > MJ_MAX_DIM || pitch < 0 || pitch > 0x7fffffffLL) return RTFS_ERR_ARG;
            if (order < 0 || order > 2 || pix < (order ? 3 : 1)) return RTFS_ERR_ARG;
            if (!mouth_finite((const double*)(w + 6), 6)) return RTFS_ERR_ARG;
        }
    }
    const int units = (out_h * out_w + 3) / 4 + 1;  // the most a plane can have (it starts 3 bytes past a dword)
    int bpj = cdiv(2048, J);                        // enough workgroups for the chip when there are few jobs ...
    const int most = cdiv(units, 256);              // ... and never a workgroup with an idle pass
    bpj = bpj > most ? most : bpj;
    const int upb = cdiv(cdiv(units, bpj), 256) * 256;
    bpj = cdiv(units, upb);
    if ((long long)J * bpj > 0x7fffffffLL) return RTFS_ERR_SHAPE;
    hipLaunchKernelGGL(mouth_rois_kernel, dim3((unsigned)(J * bpj)), dim3(256), 0, st, (const MouthJob*)jobs, out_h, out_w, bpj, upb);
    return rtfs_launch_status();
}

extern "C" {

int rtfs_mouth_affine(const double* eyes, const double* lips, long long n, int out_h, int out_w, int crop_h, int crop_w, double* A,
                      long long* refused) {
    return mouth_affine(eyes, lips, n, out_h, out_w, crop_h, crop_w, A, refused);
}

int rtfs_mouth_rois_u8(const long long* jobs, const long long* host_jobs, int J, int out_h, int out_w, void* stream) {
    return launch_mouth_rois(jobs, host_jobs, J, out_h, out_w, (hipStream_t)stream);
}

}  // extern "C"
