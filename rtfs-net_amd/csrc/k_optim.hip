// Optimizer step on the device (rtfs-net_amd/optimizers.py: AdamW): gradient gather, global-norm clip and the AdamW update in
// two launches (three with a collective in between), whatever the number of parameter tensors.
//   optim_gather_kernel   per-tensor gradients -> one contiguous flat_g (+ per-chunk sums of squares)
//   optim_sumsq_kernel    per-chunk sums of squares of flat_g alone (after an all-reduce)
//   optim_adamw_kernel    finishes the norm, forms the clip coefficient, decays, updates p / exp_avg / exp_avg_sq
// Every tensor is cut into chunks of OPTIM_CHUNK floats; one workgroup per chunk finds (tensor, offset) in a device-resident table that
// depends on the tensor sizes only (rtfs_optim_plan builds it once).  What changes every step - the gradient pointers autograd hands
// over, the parameter pointers, the hyper-parameter sets - travels BY VALUE in the kernel arguments, so a host that runs steps ahead
// of the device cannot overwrite what a queued launch will read.
// Deterministic: no atomics; one float64 partial per chunk, written by that chunk's workgroup; every workgroup of the update kernel
// re-reduces the partials itself in the same fixed order (thread tid sums partials tid, tid + 256, ...; then waves, then lanes).
// Arithmetic is torch's single-tensor AdamW after clip_grad_norm_ (float32, float64 only inside the norm).
#include "../../include/rtfs_amd.h"
#include "common.h"
#include "kernels.h"

#define OPTIM_CHUNK RTFS_OPTIM_CHUNK
#define OPTIM_MAXT RTFS_OPTIM_MAX_TENSORS
#define OPTIM_MAXH RTFS_OPTIM_MAX_HYPER
#define OPTIM_SKIP 255

namespace {

struct GradPtrs {
    const float* g[OPTIM_MAXT];
};
struct ParamPtrs {
    float* p[OPTIM_MAXT];
};
struct Hyper {  // one parameter group at one step count (host doubles rounded to float, as torch rounds its Python scalars)
    float decay, omb1, b2, omb2, step_size, bc2_sqrt, eps, pad;
};
struct UpdateArgs {
    Hyper h[OPTIM_MAXH];
    unsigned char idx[OPTIM_MAXT];  // hyper set of each tensor; OPTIM_SKIP = no gradient: untouched
};

// table (int64, device): flat_off[T] | numel[T] | chunk_tensor[NC] | chunk_off[NC]
struct Chunk {
    int t;        // tensor
    long long o;  // first element of the chunk inside the tensor
    long long f;  // the same element's index in the flat buffers (a multiple of 4: slices start on 16 bytes, chunks are 16 KB)
    int n;        // elements in the chunk
    int pad;      // zero floats after the chunk up to the next slice (last chunk of a tensor: 0..3)
};
__device__ __forceinline__ bool chunk_of(const long long* __restrict__ table, int T, int NC, int c, Chunk& k) {
    k.t = (int)table[2 * (size_t)T + c];
    if (k.t < 0 || k.t >= T) return false;
    k.o = table[2 * (size_t)T + NC + c];
    const long long numel = table[T + k.t];
    k.f = table[k.t] + k.o;
    const long long left = numel - k.o;
    k.n = left < OPTIM_CHUNK ? (int)left : OPTIM_CHUNK;
    k.pad = left <= OPTIM_CHUNK ? (int)((4 - (numel & 3)) & 3) : 0;
    return k.n > 0;
}

__device__ __forceinline__ double block_sum_d(double v, double* red, int tid) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ double sq4(f32x4 v) {
    return ((double)v.x * (double)v.x + (double)v.y * (double)v.y) + ((double)v.z * (double)v.z + (double)v.w * (double)v.w);
}

__global__ __launch_bounds__(256) void optim_gather_kernel(GradPtrs gp, const long long* __restrict__ table, int T, int NC,
                                                           float* __restrict__ flat_g, double* __restrict__ partials, int zero_missing) {
    __shared__ double red[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    Chunk k;
    if (!chunk_of(table, T, NC, c, k)) {
        if (partials && tid == 0) partials[c] = 0.0;
        return;
    }
    const float* g = gp.g[k.t];
    float* dst = flat_g + k.f;
    double ss = 0.0;
    if (g == nullptr) {  // no gradient: skipped (single rank) or zeros (the collective reads the whole buffer)
        if (zero_missing)
            for (int i = tid; i < k.n + k.pad; i += 256) dst[i] = 0.f;
    } else {
        g += k.o;
        const int n4 = (((uintptr_t)g) & 15) == 0 ? k.n >> 2 : 0;  // 16-byte loads when autograd's buffer allows; dst always does
        for (int i = tid; i < n4; i += 256) {
            const f32x4 v = *(const f32x4*)(g + 4 * i);
            *(f32x4*)(dst + 4 * i) = v;
            ss += sq4(v);
        }
        for (int i = 4 * n4 + tid; i < k.n; i += 256) {
            const float v = g[i];
            dst[i] = v;
            ss += (double)v * (double)v;
        }
        if (tid < k.pad) dst[k.n + tid] = 0.f;
    }
    if (partials) {
        ss = block_sum_d(ss, red, tid);
        if (tid == 0) partials[c] = ss;
    }
}

__global__ __launch_bounds__(256) void optim_sumsq_kernel(const long long* __restrict__ table, int T, int NC, const float* __restrict__ flat_g,
                                                          double* __restrict__ partials) {
    __shared__ double red[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    Chunk k;
    double ss = 0.0;
    if (chunk_of(table, T, NC, c, k)) {
        const float* g = flat_g + k.f;
        const int n4 = k.n >> 2;
        for (int i = tid; i < n4; i += 256) ss += sq4(*(const f32x4*)(g + 4 * i));
        for (int i = 4 * n4 + tid; i < k.n; i += 256) ss += (double)g[i] * (double)g[i];
    }
    ss = block_sum_d(ss, red, tid);
    if (tid == 0) partials[c] = ss;
}

__device__ __forceinline__ void ld4(float* a, const float* src) {
    const f32x4 v = *(const f32x4*)src;
    a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
}
__device__ __forceinline__ void st4(float* dst, const float* a) { *(f32x4*)dst = f32x4{a[0], a[1], a[2], a[3]}; }

__device__ __forceinline__ void adamw_one(float& p, float& m, float& v, float g, float gmul, const Hyper& h) {
    g = gmul * g;                             // clip_grad_norm_: g.mul_(clip_coef_clamped) (with the 1 / world of the average folded in)
    p = p * h.decay;                          // param.mul_(1 - lr * weight_decay)
    m = m + h.omb1 * (g - m);                 // exp_avg.lerp_(grad, 1 - beta1)
    v = v * h.b2 + (h.omb2 * g) * g;          // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
    p = p - h.step_size * (m / denom);        // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__global__ __launch_bounds__(256) void optim_adamw_kernel(ParamPtrs pp, UpdateArgs ua, const long long* __restrict__ table, int T, int NC,
                                                          const float* __restrict__ flat_g, float* __restrict__ exp_avg,
                                                          float* __restrict__ exp_avg_sq, const double* __restrict__ partials,
                                                          float max_norm, float grad_scale, float* __restrict__ total_norm) {
    __shared__ double red[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    // ||grad_scale * g||: every workgroup sums the NC partials in the same order, so all of them form the same coefficient
    double ss = 0.0;
    for (int i = tid; i < NC; i += 256) ss += partials[i];
    ss = block_sum_d(ss, red, tid);
    const float norm = (float)(sqrt(ss) * (double)grad_scale);
    if (c == 0 && tid == 0 && total_norm) *total_norm = norm;
    float coef = 1.f;
    if (max_norm > 0.f) {
        coef = max_norm / (norm + 1e-6f);
        coef = coef > 1.f ? 1.f : coef;  // torch.clamp(max=1.0): a NaN coefficient stays NaN (error_if_nonfinite=False)
    }
    const float gmul = grad_scale * coef;
    Chunk k;
    if (!chunk_of(table, T, NC, c, k)) return;
    const int hi = ua.idx[k.t];
    if (hi >= OPTIM_MAXH) return;  // OPTIM_SKIP: torch skips a parameter without a gradient entirely
    const Hyper h = ua.h[hi];
    float* p = pp.p[k.t] + k.o;
    const float* g = flat_g + k.f;
    float* m = exp_avg + k.f;
    float* v = exp_avg_sq + k.f;
    const int n4 = k.n >> 2;
    if ((((uintptr_t)p) & 15) == 0) {
        for (int i = tid; i < n4; i += 256) {
            float pa[4], ma[4], va[4], ga[4];
            ld4(pa, p + 4 * i); ld4(ma, m + 4 * i); ld4(va, v + 4 * i); ld4(ga, g + 4 * i);
#pragma unroll
            for (int j = 0; j < 4; ++j) adamw_one(pa[j], ma[j], va[j], ga[j], gmul, h);
            st4(p + 4 * i, pa); st4(m + 4 * i, ma); st4(v + 4 * i, va);
        }
    } else {  // a parameter that is a misaligned view: the flat side still moves in 16-byte pieces
        for (int i = tid; i < n4; i += 256) {
            float pa[4], ma[4], va[4], ga[4];
            float* q = p + 4 * i;
#pragma unroll
            for (int j = 0; j < 4; ++j) pa[j] = q[j];
            ld4(ma, m + 4 * i); ld4(va, v + 4 * i); ld4(ga, g + 4 * i);
#pragma unroll
            for (int j = 0; j < 4; ++j) adamw_one(pa[j], ma[j], va[j], ga[j], gmul, h);
#pragma unroll
            for (int j = 0; j < 4; ++j) q[j] = pa[j];
            st4(m + 4 * i, ma); st4(v + 4 * i, va);
        }
    }
    for (int i = 4 * n4 + tid; i < k.n; i += 256) {  // the tail of a tensor (43 of RTFS-Net's tensors are one float)
        float pv = p[i], mv = m[i], vv = v[i];
        adamw_one(pv, mv, vv, g[i], gmul, h);
        p[i] = pv;
        m[i] = mv;
        v[i] = vv;
    }
}

bool plan_ok(const void* table, int T, int NC) { return table && T >= 1 && T <= OPTIM_MAXT && NC >= T; }

}  // namespace

extern "C" {

int rtfs_optim_plan(const long long* numel, int n_tensors, long long* table, long long* flat_floats, int* n_chunks) {
    if (!numel || n_tensors < 1 || n_tensors > OPTIM_MAXT) return RTFS_ERR_ARG;
    long long off = 0, nc = 0;
    for (int t = 0; t < n_tensors; ++t) {
        if (numel[t] < 1) return RTFS_ERR_SHAPE;
        off += (numel[t] + 3) / 4 * 4;
        nc += (numel[t] + OPTIM_CHUNK - 1) / OPTIM_CHUNK;
        if (off > 0x7fffffffLL || nc > 0x7fffffffLL) return RTFS_ERR_SHAPE;
    }
    if (flat_floats) *flat_floats = off;
    if (n_chunks) *n_chunks = (int)nc;
    if (table) {
        const size_t T = (size_t)n_tensors;
        long long o = 0, c = 0;
        for (int t = 0; t < n_tensors; ++t) {
            table[t] = o;
            table[T + t] = numel[t];
            for (long long e = 0; e < numel[t]; e += OPTIM_CHUNK, ++c) {
                table[2 * T + c] = t;
                table[2 * T + nc + c] = e;
            }
            o += (numel[t] + 3) / 4 * 4;
        }
    }
    return RTFS_OK;
}

int rtfs_optim_gather_f32(const float* const* grads, const long long* table, int n_tensors, int n_chunks, float* flat_g, double* partials,
                          int zero_missing, void* stream) {
    if (!grads || !flat_g || !plan_ok(table, n_tensors, n_chunks)) return RTFS_ERR_ARG;
    if ((((uintptr_t)flat_g) & 15) || (((uintptr_t)partials) & 7) || (((uintptr_t)table) & 7)) return RTFS_ERR_ARG;
    GradPtrs gp;
    for (int t = 0; t < OPTIM_MAXT; ++t) {
        gp.g[t] = t < n_tensors ? grads[t] : nullptr;
        if (((uintptr_t)gp.g[t]) & 3) return RTFS_ERR_ARG;
    }
    hipLaunchKernelGGL(optim_gather_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, gp, table, n_tensors, n_chunks, flat_g,
                       partials, zero_missing);
    return rtfs_launch_status();
}

int rtfs_optim_sumsq_f32(const long long* table, int n_tensors, int n_chunks, const float* flat_g, double* partials, void* stream) {
    if (!flat_g || !partials || !plan_ok(table, n_tensors, n_chunks)) return RTFS_ERR_ARG;
    if ((((uintptr_t)flat_g) & 15) || (((uintptr_t)partials) & 7) || (((uintptr_t)table) & 7)) return RTFS_ERR_ARG;
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, table, n_tensors, n_chunks, flat_g, partials);
    return rtfs_launch_status();
}

int rtfs_optim_adamw_f32(float* const* params, const unsigned char* hyper_index, const float* hyper, int n_hyper, const long long* table,
                         int n_tensors, int n_chunks, const float* flat_g, float* exp_avg, float* exp_avg_sq, const double* partials,
                         float max_norm, float grad_scale, float* total_norm, void* stream) {
    if (!params || !hyper_index || !hyper || !flat_g || !exp_avg || !exp_avg_sq || !partials || !plan_ok(table, n_tensors, n_chunks))
        return RTFS_ERR_ARG;
    if (n_hyper < 1 || n_hyper > OPTIM_MAXH) return RTFS_ERR_ARG;
    if ((((uintptr_t)flat_g) | ((uintptr_t)exp_avg) | ((uintptr_t)exp_avg_sq)) & 15) return RTFS_ERR_ARG;
    if ((((uintptr_t)partials) & 7) || (((uintptr_t)table) & 7) || (((uintptr_t)total_norm) & 3)) return RTFS_ERR_ARG;
    static_assert(sizeof(Hyper) == 8 * sizeof(float), "hyper set = 8 floats");
    ParamPtrs pp;
    UpdateArgs ua;
    for (int i = 0; i < OPTIM_MAXH; ++i)
        for (int j = 0; j < 8; ++j) ((float*)&ua.h[i])[j] = i < n_hyper ? hyper[8 * i + j] : 0.f;
    for (int t = 0; t < OPTIM_MAXT; ++t) {
        pp.p[t] = t < n_tensors ? params[t] : nullptr;
        ua.idx[t] = t < n_tensors ? hyper_index[t] : OPTIM_SKIP;
        if (t >= n_tensors || ua.idx[t] == OPTIM_SKIP) continue;
        if (ua.idx[t] >= n_hyper || !pp.p[t] || (((uintptr_t)pp.p[t]) & 3)) return RTFS_ERR_ARG;
    }
    hipLaunchKernelGGL(optim_adamw_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, pp, ua, table, n_tensors, n_chunks, flat_g,
                       exp_avg, exp_avg_sq, partials, max_norm, grad_scale, total_norm);
    return rtfs_launch_status();
}

}  // extern "C"
