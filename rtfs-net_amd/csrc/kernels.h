// Internal (C++) launch interface between the C-ABI layer (api.hip) and the kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "common.h"

struct PwArgs {
    const float* x = nullptr;     // (B, CIN, P)
    const float* x2 = nullptr;    // optional second addend (gateway: the bottleneck residual a1)
    float* res_out = nullptr;     // gateway: PReLU(dw1x1(x [+x2])) written through, (B, CIN, P)
    const float* wt = nullptr;    // (CIN, COUT) transposed 1x1 weight (exact-f32 kernels)
    const void* w16 = nullptr;    // [CIN/32][hi|lo][COUT][32] f16 split image of 256*W (f16x3 kernels)
    const void* w16b = nullptr;   // S3 + decoder taps: K-permuted taps image (packing.taps_perm_image)
    const float* bias = nullptr;  // (COUT)
    const float* aux = nullptr;   // EPI_BIAS_RES: residual (B,COUT,P); EPI_S3: encoder output a0 (B,COUT,P)
    float* out = nullptr;         // (B, COUT, P)
    const double* stats = nullptr;  // PRO_GLN_RELU: (B,2) sum / sumsq of x
    double inv_count = 0;
    const float* gamma = nullptr;
    const float* beta = nullptr;
    const float* gw = nullptr;  // gateway depthwise scale (CIN)
    const float* gb = nullptr;  // gateway depthwise bias (CIN)
    const float* slope = nullptr;  // PReLU slope (1)
    int P = 0;
    int cs = 0;         // channel stride (floats) of every (B, C, P) tensor of the call; 0 = P (contiguous).  The fused separator pads it
                        // to a multiple of 32 floats so that every 64-pixel wave segment is whole 128-byte lines ("pitch")
    int cout_live = 0;  // EPI_TAPS: number of real output channels
    unsigned* tile_ctr = nullptr;  // persistent kernels: zeroed counter word that hands out tiles (null: static stride)
    // optional CAF prologue of the gateway kernel (fused separator path): x <- CAF(x, video) before the residual add
    const float* caf_r = nullptr;    // (B,256,Tv) resize(video)
    const float* caf_att = nullptr;  // (B,256,Tv) softmax attention
    const float *caf_w_key = nullptr, *caf_bn_key = nullptr, *caf_w_val = nullptr, *caf_bn_val = nullptr;
    int caf_T = 0, caf_F = 0, caf_Tv = 0;
};

// What the pointwise launchers (k_pw.hip, k_pw16.hip, k_pwr.hip, k_pws.hip, k_b2b.hip, k_bnh.hip, k_s3f.hip) chose on their last call from
// this thread (host side only; rtfs_debug_pw_f32 hands it to tests/test_hip_pw_edges.py, which asserts the route every case is meant to take).
// Every launcher clears the record on entry and appends one job per kernel it launches, so a refusal leaves n == 0.
enum PwFamily { PW_FAM_F32 = 1, PW_FAM_PW16 = 2, PW_FAM_PWS = 3, PW_FAM_RES2 = 4, PW_FAM_B2B = 5, PW_FAM_B2B4 = 6, PW_FAM_HEAD4 = 7,
                PW_FAM_PWR = 8, PW_FAM_BN_HEAD = 9, PW_FAM_TAIL = 10 };
// cin / cout / pro / epi: the template form (0 where the kernel has none); caf: CAF prologue; am: a1_mode (B2B: 1); mode: PWR MODE, PWS HAS_X2,
// BN_HEAD WRES, TAIL K; tps: tiles per sample; ntiles = tps * B; grid: workgroups launched; counter: 1 = tiles from the counter word, 0 = static stride
struct PwRouteJob { int family, cin, cout, pro, epi, caf, am, mode, tps, ntiles, grid, counter; };
struct PwRoute { int n; PwRouteJob job[2]; };
const PwRoute& pw_route_last();
void pw_route_clear();
void pw_route_add(const PwRouteJob& j);

int launch_stft(const float* wav, float* spec, int B, int L, int T, hipStream_t st);
int launch_enc_conv(const float* spec, const float* w, float* a0, double* stats, int B, int C, int T, int F, size_t cs,
                    size_t bs, hipStream_t st);
// gLN statistics of the encoder output computed from the spectrogram (a0 is not formed) + the encoder's f16x3 fragment image (32 KB at img)
// + (one extra row of workgroups) up to two 256 -> 256 f16x3 weight images [8 chunks][hi|lo][256 rows][64 B] copied with their rows padded to
// 72 bytes (294912 B each): the LDS image of the head / tail kernels, which they fetch by LDS-DMA - a DMA writes LDS linearly, so the
// conflict-free row padding has to exist in memory
struct EncPadJobs {
    const void* src[2] = {nullptr, nullptr};
    void* dst[2] = {nullptr, nullptr};
};
int launch_enc_stats(const float* spec, const float* w, double* stats, void* img, const EncPadJobs& pad, int B, int T, int F, hipStream_t st);
int launch_dec_istft(const float* z, float* wav, int B, int T, int F, int L, size_t zcs, size_t zbs, hipStream_t st);

int launch_pw_audio_bn(const PwArgs& a, int B, hipStream_t st);
int launch_pw_gateway_proj(const PwArgs& a, int B, hipStream_t st);
int launch_pw_residual(const PwArgs& a, int B, hipStream_t st);
int launch_pw_s3(const PwArgs& a, int B, hipStream_t st);
int launch_pw_dec_taps(const PwArgs& a, int B, hipStream_t st);
int launch_pw16_audio_bn(const PwArgs& a, int B, hipStream_t st);
int launch_pw16_gateway_proj(const PwArgs& a, int B, hipStream_t st);
int launch_pw16_residual(const PwArgs& a, int B, hipStream_t st);
int launch_pw16_s3(const PwArgs& a, int B, hipStream_t st);
int launch_pw16_dec_taps(const PwArgs& a, int B, hipStream_t st);
// 256 -> 256 with register-resident pixels (k_pwr.hip)
int launch_pwr_audio_bn(const PwArgs& a, int B, hipStream_t st);
int launch_pwr_s3(const PwArgs& a, int B, hipStream_t st);
int launch_pwr_s3_taps(const PwArgs& a, int B, hipStream_t st);  // S3 + decoder taps: writes z (B,18,P), not the separated spectrum
// block boundary: residual_conv(i) + gateway/projection(i+1) back to back (k_pws.hip)
struct B2bArgs {
    const float* x = nullptr;     // expanded_i (B,64,P)
    float* res = nullptr;         // in: residual_i, out: residual_{i+1} (B,256,P), rewritten in place
    const float* a1 = nullptr;    // bottleneck output (B,256,P), RefinementModule's residual
    float* xenc = nullptr;        // x_enc_{i+1} (B,64,P)
    const void* w1_16 = nullptr;  // residual_conv f16x3 image [2][hi|lo][256][32]
    const float* b1 = nullptr;    // (256)
    const void* w2_16 = nullptr;  // projection f16x3 image [8][hi|lo][64][32] with the K axis in accumulator order
    const float* bp = nullptr;    // (64)
    const float *gw = nullptr, *gb = nullptr, *slope = nullptr;
    int P = 0;
    int cs = 0;  // channel stride of x / res / a1 / xenc (floats); 0 = P
    const float *caf_r = nullptr, *caf_att = nullptr, *caf_w_key = nullptr, *caf_bn_key = nullptr, *caf_w_val = nullptr, *caf_bn_val = nullptr;
    const float *caf_rt = nullptr, *caf_attt = nullptr;  // (B, Tv, 256) transposed copies of caf_r / caf_att (k_b2b.hip)
    int caf_T = 0, caf_F = 0, caf_Tv = 0;
    // k_b2b.hip only: bit 0 = `res` does not contain a1 yet (read a1, add it to the block input); bit 1 = write the new residual WITH a1 added, so
    // that the next boundary runs with bit 0 clear and never reads a1.  1 = the reference sequence as written (launch_pws_b2b knows no other).
    // bit 2 (with a CAF, i.e. the first boundary): `res` is not read - residual_0 = PReLU(gw a1 + gb) is formed from the a1 rows (the head kernel
    // then need not write it).
    int a1_mode = 1;
    // k_b2b.hip only, separation of K targets per mixture (rtfs_separator_speakers_f32): the launch runs over targets t, and reads `x` of
    // sample t / xk and `a1` of sample t / a1k (1 = the sample itself).  `res` and `xenc` are always the target's own.
    // A different number of targets per mixture (rtfs_separator_targets_f32): a divisor of 0 reads the sample from the table instead,
    // mix_of[t] - mix_base (mix_of: DEVICE, one int per target of this launch; mix_base: the first mixture of the launch's batch part).
    int xk = 1, a1k = 1;
    const int* mix_of = nullptr;
    int mix_base = 0;
};
int launch_pws_b2b(const B2bArgs& a, int B, hipStream_t st);
bool launch_pws_b2b4_qualifies(const B2bArgs& a);
// second generation (k_b2b.hip): padded channel rows (cs % 64 == 0), no CAF; ctr = zeroed tile counter of this launch or null.
// RTFS_ERR_ARG = call does not qualify, use launch_pws_b2b
int launch_pws_b2b4(const B2bArgs& a, int B, unsigned* ctr, hipStream_t st);
// audio bottleneck (gLN -> ReLU -> 1x1 256->256) + first block head (gateway + projection) in one kernel (k_bnh.hip): padded rows only,
// RTFS_ERR_ARG = call does not qualify, use launch_pwr_audio_bn + launch_pws_head4
struct BnHeadArgs {
    const float* spec = nullptr;    // spectrogram (B,2,T,F): the encoder output a0 is rebuilt on the fly, not read
    const void* enc_img = nullptr;  // encoder f16x3 fragment image (enc_stats_kernel)
    int T = 0, F = 0;
    float* a1 = nullptr;            // bottleneck output (B,256,cs)
    float* res = nullptr;           // gateway output (B,256,cs); null = not written (the first boundary forms it from a1: B2bArgs::a1_mode bit 2)
    float* xenc = nullptr;          // projection output (B,64,cs)
    const double* stats = nullptr;  // (B,2) sum / sumsq of a0
    double inv_count = 0;
    const float *gamma = nullptr, *beta = nullptr;  // gLN (256)
    const void* w16 = nullptr;      // bottleneck f16x3 image [8][hi|lo][256][32]
    const float* bias = nullptr;    // (256)
    const float *gw = nullptr, *gb = nullptr, *slope = nullptr;  // gateway dw 1x1 (256), PReLU (1)
    const void* w2_16 = nullptr;    // projection f16x3 image [8][hi|lo][64][32], K in accumulator order
    const float* bp = nullptr;      // (64)
    int P = 0, cs = 0;
    int stagger = 2;                // start offset between the four workgroup groups, in units of 8128 cycles (s_sleep 127); 0 = none
    unsigned* tile_ctr = nullptr;
};
bool launch_bn_head_qualifies(const BnHeadArgs& a);  // same conditions as launch_tail_s3t (same P, same pitch)
int launch_bn_head(const BnHeadArgs& a, int B, hipStream_t st);
// residual conv of the last block application + S3 mask + complex product + decoder taps in one kernel (k_s3f.hip): padded rows only,
// RTFS_ERR_ARG = call does not qualify, use launch_pws_residual + launch_pwr_s3_taps
struct TailS3Args {
    const float* x = nullptr;     // expanded (B,64,cs)
    const float* res = nullptr;   // residual (B,256,cs)
    const float* spec = nullptr;  // spectrogram (B,2,T,F): the encoder output a0 is rebuilt on the fly, not read
    const void* enc_img = nullptr;  // encoder f16x3 fragment image (enc_stats_kernel)
    int T = 0, F = 0;
    float* z = nullptr;           // decoder taps (B,cout_live,cs)
    const void* w1_16 = nullptr;  // residual_conv f16x3 image [2][hi|lo][256][32]
    const float* b1 = nullptr;    // (256)
    const void* w16 = nullptr;    // mask conv f16x3 image [8][hi|lo][256 rows of 72 bytes: 32 halfs + 8 bytes of padding] (EncPadJobs)
    const float* bias = nullptr;  // (256)
    const float* slope = nullptr; // mask head PReLU (1)
    const void* w16b = nullptr;   // K-permuted taps image (packing.taps_perm_image)
    const double* stats = nullptr;  // (B,2) sum / sumsq of a0 (range normalisation of the taps operand), may be null
    double inv_count = 0;
    int P = 0, cs = 0, cout_live = 0;
    unsigned* tile_ctr = nullptr;
    int K = 1;  // targets per mixture: target t reads `spec` and `stats` of mixture t / K (the a0 it rebuilds is the mixture's)
    // K = 0 (rtfs_separator_targets_f32): the mixture is mix_of[t] - mix_base, as in B2bArgs
    const int* mix_of = nullptr;
    int mix_base = 0;
};
int launch_tail_s3t(const TailS3Args& a, int B, hipStream_t st);
int launch_pws_head4(const PwArgs& a, int B, hipStream_t st);  // block head on padded rows (k_b2b.hip); RTFS_ERR_ARG = use launch_pws_gateway_proj
int launch_pws_gateway_proj(const PwArgs& a, int B, hipStream_t st);
int launch_pws_residual(const PwArgs& a, int B, hipStream_t st);
int launch_mfma_f16_selftest(const float* A, const float* B, float* D, hipStream_t st);
int launch_nearest_index_selftest(const int* pairs, int n_pairs, const int* offsets, int* out_src, int* out_first_dst, hipStream_t st);  // k_caf.hip

// Depthwise 4x4 family.  Tensors are (B, C, H, W) contiguous.
struct DwArgs {
    const float* x = nullptr;
    // input fold (IN_AFFINE): x is a pre-norm conv output, its gLN is applied at load time
    const double* in_stats = nullptr;
    double in_inv_count = 0;
    const float* in_gamma = nullptr;
    const float* in_beta = nullptr;
    const float* w[4] = {nullptr, nullptr, nullptr, nullptr};     // (C,16) each
    const float* bias[4] = {nullptr, nullptr, nullptr, nullptr};  // (C) or null
    float* out[4] = {nullptr, nullptr, nullptr, nullptr};
    double* stats_out[4] = {nullptr, nullptr, nullptr, nullptr};  // (B,2) each
    int C = 0, H = 0, W = 0, TH = 8;
    int cs = 0;  // channel stride (floats) of the (B, C, H, W) tensors x / out[] / addend; 0 = H * W.  gate / emb (Hg x Wg) stay contiguous
    int in_combine = 0;  // lane-exchange kernels, MODE 0: the input is the same-size TFAR combination gLN(x) * sigmoid(gLN(gate)) + gLN(emb) of three
                         // pre-norm tensors (folds: loc_* / gate_* / emb_*, all with g_inv_count), formed at load time (fusion.py:62-67)
    int rev = 0;  // lane-exchange kernels: walk the tensor back to front (a consumer that starts where its producer stopped finds that end in the
                  // memory-side cache: tools/bench_mall.hip)
    int job_stride = 0, job_off = 0;  // two jobs interleaved per sample in one launch (launch_dw_s2_stats): logical block id -> sample id / job_stride,
                                      // this job's block (id % job_stride) - job_off if that lies in [0, gx * gy); 0 = one job (id -> x, y, z)
    int gx = 0, gy = 0, nblk = 0, blk0 = 0;  // set by the launchers of the lane-exchange kernels: logical grid (gx, gy, B) behind a 1-D launch
                                              // (XCD order); blk0 = first block of this job when several jobs share one launch
    // MODE 2 (TFAR apply) / stride-2 kernel: the low-resolution side
    int Hg = 0, Wg = 0;
    const double* loc_stats = nullptr;
    double loc_inv_count = 0;
    const float* loc_gamma = nullptr;
    const float* loc_beta = nullptr;
    const float* gate = nullptr;
    const double* gate_stats = nullptr;
    const float* gate_gamma = nullptr;
    const float* gate_beta = nullptr;
    const float* emb = nullptr;
    const double* emb_stats = nullptr;
    const float* emb_gamma = nullptr;
    const float* emb_beta = nullptr;
    double g_inv_count = 0;
    const float* addend = nullptr;  // optional "+ d0" (pre-norm c0 with its fold)
    const double* add_stats = nullptr;
    double add_inv_count = 0;
    const float* add_gamma = nullptr;
    const float* add_beta = nullptr;
};

struct GCombineArgs {
    const float *l, *gate, *emb;
    const double *l_stats, *gate_stats, *emb_stats;
    const float *l_gamma, *l_beta, *gate_gamma, *gate_beta, *emb_gamma, *emb_beta;
    double inv_count;
    float* out;
    int C, HW;
};

// What the launchers below chose on their last call from this thread (host side only; rtfs_debug_dw_f32 hands it to the tests, which assert
// the route every case is meant to take: a shape that silently falls to the one-column kernel must not pass for coverage of the packed one).
// Every launcher clears the record on entry and appends one job per kernel job it launches, so a refusal leaves n == 0.
enum DwFamily { DW_FAM_S1 = 1, DW_FAM_1P = 2, DW_FAM_G3 = 3, DW_FAM_S2X = 4, DW_FAM_S2_POOL = 5, DW_FAM_S2_STATS = 6, DW_FAM_G_FORM = 7,
                DW_FAM_G_COMBINE = 8, DW_FAM_2P = 9 };
struct DwRouteJob { int family, nconv, in_affine, mode, var, TH, gx, gy; };  // TH, gx, gy: the effective band height and logical grid
struct DwRoute { int n; DwRouteJob job[4]; };
const DwRoute& dw_route_last();

int launch_dw_s1(const DwArgs& a, int nconv, bool in_affine, int mode, int B, hipStream_t st);
// One launch for the block's three independent low-resolution conv jobs (steps 10 and 11: four plain convs on one input as two 2-conv
// jobs + one conv on a gLN-folded input): each alone is 576 workgroups, too few to fill the chip
int launch_dw_g3(const DwArgs& conv4, const DwArgs& aff1, int B, hipStream_t st);
int launch_dw_s2_pool(const DwArgs& a, int B, hipStream_t st);
// the stride-2 + pool pass and a statistics-only pass (MODE 1, input fold) over the SAME input in one launch; RTFS_ERR_ARG = not eligible
int launch_dw_s2_stats(const DwArgs& s2, const DwArgs& stats, int B, hipStream_t st);
// two TFAR layers in a row without the tensor between them (k_dw.hip, dw2p_body): pass 0 = statistics of the second layer's conv, pass 1 = the
// second layer's apply.  RTFS_ERR_ARG before any launch = the shape is not this launcher's
int launch_dw_two_pass(const DwArgs& first, const DwArgs& second, int pass, int B, hipStream_t st);
int launch_g_form(const float* p0, const float* c1, const double* st1, double inv_count, const float* gamma,
                  const float* beta, float* g, int B, int C, int HW, hipStream_t st);
int launch_g_combine(const GCombineArgs& a, int B, hipStream_t st);
int launch_transpose(const float* x, float* y, int N, int H, int W, hipStream_t st);
int launch_stats(const float* x, double* stats, int B, size_t N, hipStream_t st);
int launch_stats2(const float* x, double* stats, int B, size_t N, double* part, hipStream_t st);  // part: 512 * B doubles

// Fused dual-path SRU sweep.  Sequence n = (b, row): element (c, s) at
//   x[(n / R) * bstride + (n % R) * rstride + c * cstride + s],  s = 0..Ls-1 contiguous.
struct DpArgs {
    const float* x = nullptr;
    float* out = nullptr;
    int R = 0, Ls = 0;
    size_t bstride = 0, rstride = 0, cstride = 0;
    const float* ln_gamma = nullptr;  // (64)
    const float* ln_beta = nullptr;   // (64)
    const float* W0 = nullptr;        // (512, 256)  layer-0 projection, column (dir*32+j)*4+m
    const float* Wl = nullptr;        // 3 x (64, 256) layers 1-3, k=3 columns padded to 4 (m=3 zero)
    const float* wc = nullptr;        // 4 x (128)   [v_f(dir,j) | v_r(dir,j)]
    const float* bias = nullptr;      // 4 x (128)   [b_f | b_r]
    const float* Wt = nullptr;        // (512 = kk*64+ci, 64 co)  ConvTranspose1d weight, re-ordered
    const float* bt = nullptr;        // (64)
    const float* whh = nullptr;       // LSTM cell: 4 x 2 x (32 k, 128 = gate*32 + j) recurrent weights; then W0/Wl columns are
                                      // dir*128 + gate*32 + j (gates i,f,g,o) and bias is 4 x (256) = b_ih + b_hh
};
size_t dualpath_lds_bytes(int Ls);
int launch_dualpath(const DpArgs& a, int nseq, hipStream_t st);
int launch_sru_standalone(const float* x, float* h, int L, int N, const float* W0, const float* Wl, const float* wc,
                          const float* bias, hipStream_t st);

// TF attention
struct RowCanArgs {
    const float* x = nullptr;      // (B,64,T,64); cl: (B,T,64,64) channel-last (NOUT == 96)
    int cl = 0;                    // channel-last X (NOUT == 96) / residual (NOUT == 64): the RTFS block's route from the time sweep
    const float* wt = nullptr;     // (64, NOUT) transposed 1x1 weights of every ConvActNorm in the call
    const float* bias = nullptr;   // (NOUT)
    const float* slope = nullptr;  // (ngroups) PReLU slope of each ConvActNorm
    const float* gamma = nullptr;  // (NOUT, 64)
    const float* beta = nullptr;   // (NOUT, 64)
    int ngroups = 0;
    int group_start[13] = {0};     // channel range of each LayerNorm group
    unsigned char group_of[96] = {0};
    int T = 0;
    int rpw = 0;  // frames per workgroup (set by the launcher: 8, fewer for small batches)
    float vscale = 1.f;  // NOUT == 96: V is stored times this power of two, folded into the V modules' LayerNorm affine (exact); see ATT_VSC
    float *q = nullptr, *k = nullptr, *v = nullptr;  // NOUT == 96
    const float* res = nullptr;                       // NOUT == 64: residual
    float* out = nullptr;
};
struct AttnArgs {
    const float *q = nullptr, *k = nullptr, *v = nullptr;
    float* out = nullptr;  // (B,64,T,64), channel = head*16 + c
    int T = 0;
    float scale = 0.f;
    float vscale = 1.f;  // v holds vscale * V (a power of two); the output is divided by it
    int npairs = 0;  // B * heads, set by the launcher
};
int launch_row_can_qkv(const RowCanArgs& a, int B, hipStream_t st);
int launch_row_can_proj(const RowCanArgs& a, int B, hipStream_t st);
int launch_attn_core(const AttnArgs& a, int B, hipStream_t st);
size_t attn_core_lds_bytes(int T);
// The power of two attention() stores V times.  The core splits V into f16 hi + lo unscaled otherwise, and the low part of an element
// below 2^-3 is an f16 subnormal (quantum 2^-24): an absolute floor of 2^-25 that a single-key row (T = 1: the output is V[0]) carries
// whole - 1.5e-5 of an element of 2e-3 (tests/test_hip_attn_edges.py).  Times 64 the floor is 2^-31; f16 overflows from |V| = 1023 on
// (a LayerNorm output over 1024 elements is at most 32 |gamma| + |beta|).  P is scaled by 2^12 in the kernel for the same reason.
constexpr float ATT_VSC = 64.f;
// What the three attention launchers chose on their last call from this thread (host side only; rtfs_debug_attn_f32 hands it to
// tests/test_hip_attn_edges.py, which asserts the route every case is meant to take).  Every launcher clears the record on entry and
// appends one job per kernel it launches, so a refusal leaves n == 0.
enum AttnFamily { ATT_FAM_QKV = 1, ATT_FAM_CORE = 2, ATT_FAM_PROJ = 3 };
// cl: channel-last form (rows); rpw: frames per workgroup (rows; core 0); gx, gy: grid; lds: dynamic LDS bytes (core; rows 0); npairs: B * heads (core)
struct AttnRouteJob { int family, cl, rpw, gx, gy, lds, npairs; };
struct AttnRoute { int n; AttnRouteJob job[1]; };
const AttnRoute& attn_route_last();

// CAF
struct CafArgs {
    const float* audio = nullptr;  // (B,256,T,F)
    const float* video = nullptr;  // (B,512,Tv)
    float* out = nullptr;          // (B,256,T,F)
    float* r_out = nullptr;        // (B,256,Tv) workspace: resize(video)
    float* att_out = nullptr;      // (B,256,Tv) workspace: softmax attention
    float *r_t = nullptr, *att_t = nullptr;  // optional (B,Tv,256) transposed copies of the two (fused separator)
    int T = 0, F = 0, Tv = 0;
    const float *w_key = nullptr, *bn_key = nullptr;  // (256), (4,256) = [weight | bias | running_mean | running_var]
    const float *w_val = nullptr, *bn_val = nullptr;
    const float *w_att = nullptr, *b_att = nullptr, *g_att = nullptr, *be_att = nullptr;          // (1024,2),(1024)x3
    const float *w_resize = nullptr, *b_resize = nullptr, *g_resize = nullptr, *be_resize = nullptr;  // (256,2),(256)x3
};
int launch_caf_video(const CafArgs& a, int B, hipStream_t st);
int launch_caf_apply(const CafArgs& a, int B, hipStream_t st);
int dualpath_timing_enable(int on);
int dualpath_timing_collect(float* ms, int* ls, int* nseq, int cap);

// Fused dual-path SRU sweep, f16x3 generation (k_dualpath16.hip).  Same sequence addressing as DpArgs.
struct Dp16Args {
    const float* x = nullptr;
    float* out = nullptr;
    int nseq = 0, R = 0, Ls = 0;
    size_t bstride = 0, rstride = 0, cstride = 0;  // x: sequence n at (n / R) bstride + (n % R) rstride; channel stride (channel-major)
    // Channel-last sides (generation 3 only, k_dualpath16s.hip): a position's 64 channels are contiguous, positions `pstride` floats apart.
    // layout bit 0: x channel-last (cstride unused); bit 1: out channel-last.  Layouts 0 and 3: out shares x's strides; layout 2 (x channel-major,
    // out channel-last - the F sweep feeding the T sweep) addresses out with its own ob / or / op strides.
    int layout = 0;
    size_t pstride = 0;
    size_t obstride = 0, orstride = 0, opstride = 0;
    const float* ln_gamma = nullptr;
    const float* ln_beta = nullptr;
    const half8* w16_l0 = nullptr;  // [16 chunks][hi|lo][256 cols = dir*128 + gate*32 + j][32 k'], k' = kk*64 + c
    const half8* w16_l = nullptr;   // 3 x [2 chunks][hi|lo][256][32]; gate 3 = identity block (highway input)
    const half8* w16_ct = nullptr;  // [8 chunks][hi|lo][64 co][64 k'], k' = kk*64 + ci
    // the same three images in MFMA fragment order (generation 3, k_dualpath16s.hip): [K step 16][dir][gate tile m][hi|lo][lane] x half8 with
    // lane (h, r) = W[k = 16 step + 8 h + j][col = dir*128 + m*32 + r]; conv-transpose: [tap][co tile][ks][hi|lo][lane], W[co = 32 tile + r][k = 16 ks + 8 h + j]
    const half8 *wf_l0 = nullptr, *wf_l = nullptr, *wf_ct = nullptr;
    const float* wc16 = nullptr;    // 4 x (128): v_f, v_r scaled by -log2(e)
    const float* bias16 = nullptr;  // 4 x (128): b_f, b_r scaled by -log2(e)
    const float* bt = nullptr;      // (64)
    unsigned long long* stamps = nullptr;  // diagnostic build only: [workgroups][16] s_memtime stamps
};
size_t dp16_lds_bytes(int Ls, int nseq_per_wg);
int launch_dualpath16(const Dp16Args& a, hipStream_t st);
// generation 3 (k_dualpath16s.hip): 256-thread workgroups, two per CU, L <= 128; launch_dualpath16 routes to it
size_t dp16s_lds_bytes(int Ls, int nseq_per_wg);
int launch_dualpath16s(const Dp16Args& a, hipStream_t st);
bool dualpath_gen2();  // RTFS_SWEEP_GEN2=1: the sweeps up to Ls = 256 run on generation 2 (channel-major only)
void* dualpath_timing_begin(int Ls, int nseq, hipStream_t st);
void dualpath_timing_end(void* slot, hipStream_t st);

// VP block (video 1-D TDANetBlock)
size_t vp_lds_bytes(int Tv);
int launch_vp_block(const float* video, const float* pack, float* out, int B, int Tv, hipStream_t st);

// evaluation-side loss path (k_loss.hip): pairwise negative SNR / SI-SDR / SD-SDR + best permutation, n_src <= 4
int launch_pit_pairwise(const float* est, const float* tgt, int B, int n, int L, int kind, int zero_mean, int take_log, float* pw,
                        float* min_loss, int* perm, hipStream_t st);

// evaluation metric (k_stoi.hip): classic STOI as pystoi 0.4.1 computes it, fs 16000 (resampled to 10 kHz on the device) or 10000
size_t stoi_workspace_bytes(int B, int L, int fs);
int launch_stoi(const float* clean, const float* est, int B, int L, int fs, void* ws, size_t ws_bytes, float* d, int* kept, hipStream_t st);

// scoring many recordings of different lengths in one pooled pass (k_stoi.hip: planner, workspace, STOI; k_score.hip: the four PIT
// figures from float64 moments).  `plan` is the HOST table score_many_plan wrote, `table` its device copy (layout: rtfs_amd.h).
// column c of the table is table[c * (R + 1) + r]; row R holds the totals of the offset and work-list columns
enum { SC_L, SC_L10, SC_K0, SC_FMAX, SC_RS_OFF, SC_FR_OFF, SC_BD_OFF, SC_RS0, SC_BG0, SC_CC0, SC_MC0, SC_COLS };
constexpr int SCORE_MOM_CHUNK = 4096;  // samples per moment workgroup, counted from the recording's own start
// moments of the 2 n + 1 signals (mix, n clean, n estimates): sums, sums of squares, <est_i, clean_j>, <mix, clean_j>
constexpr int score_moments(int n) { return 2 * (2 * n + 1) + n * n + n; }
struct ScoreManyWs {
    float *xr, *yr;
    double *energy, *xb, *yb, *partial, *mom;
    int *kidx, *kcount;
};
int score_many_plan(const long long* L, int R, int n_src, int fs, int* table, size_t* ws_bytes);
// checks the plan's own record of (R, n_src, fs) against the call's and the workspace size, then carves: RTFS_ERR_ARG / RTFS_ERR_WORKSPACE
int score_many_carve(const int* plan, int R, int n_src, int fs, void* ws, size_t ws_bytes, ScoreManyWs* w);
int launch_stoi_many(const float* const* cleans, const float* const* ests, const int* table, const int* plan, int R, int n_src, int fs, void* ws,
                     size_t ws_bytes, float* d, int* kept, hipStream_t st);
int launch_sdr_many(const float* const* mixes, const float* const* cleans, const float* const* ests, const int* table, const int* plan, int R,
                    int n_src, int fs, void* ws, size_t ws_bytes, float* out, int* perm, hipStream_t st);

// extended STOI (k_stoi.hip; Jensen & Taal 2016 as pystoi 0.4.1's extended=True branch without its noise terms): stages 1-3 of classic
// STOI, then per 30-frame segment the 15 x 30 band matrix normalised along both axes and correlated.  d_classic non-NULL: classic STOI
// on the same band values as well (bit-equal to launch_stoi / launch_stoi_many), one more partial region (with_classic).
size_t estoi_workspace_bytes(int B, int L, int fs, int with_classic);
int launch_estoi(const float* clean, const float* est, int B, int L, int fs, void* ws, size_t ws_bytes, float* d_ext, float* d_classic,
                 int* kept, hipStream_t st);
size_t estoi_many_workspace_bytes(const int* plan, int R, int with_classic);
int launch_estoi_many(const float* const* cleans, const float* const* ests, const int* table, const int* plan, int R, int n_src, int fs,
                      void* ws, size_t ws_bytes, float* d_ext, float* d_classic, int* kept, hipStream_t st);

// BSS-eval SDR (k_bss.hip): 512-tap projection of every estimate (and the mixture) onto every clean source from float64 correlations,
// Levinson-Durbin per clean source, permutation by the largest mean.  The pooled entry works on score_many_plan's table (columns 0 and
// 10) with a workspace of its own.  BssDebug: optional copies of the folded r (rows n, 512), d (rows n, NR, 512), ee (rows n, NR) and the
// order reached (rows n); form 0 = the production solver, 64 | 512 = that many threads per (recording, clean source).
constexpr int BSS_TAPS = 512, BSS_CHUNK = 4096;
struct BssDebug {
    double *r, *d, *ee;
    int* order;
    int form;
};
size_t bss_sdr_workspace_bytes(int B, int n_src, int L, int with_mix);
int launch_bss_sdr(const float* clean, const float* est, const float* mix, int B, int n_src, int L, void* ws, size_t ws_bytes, float* sdr,
                   float* sdr_i, int* perm, const BssDebug& dbg, hipStream_t st);
size_t bss_sdr_many_workspace_bytes(const int* plan, int R, int with_mix);
int launch_bss_sdr_many(const float* const* mixes, const float* const* cleans, const float* const* ests, const int* table, const int* plan,
                        int R, int n_src, int fs, void* ws, size_t ws_bytes, float* sdr, float* sdr_i, int* perm, const BssDebug& dbg,
                        hipStream_t st);
// BSS-eval SIR and SAR (k_bss.hip): the joint projection onto all J = n_src + n_other true sources (block Levinson, J x J blocks) next
// to the scalar ones; four launches.  BssEvalDebug: optional copies of the folded r_ij (rows, J, J, 1023: lag k at 511 + k), D_all (rows,
// n_src, J, 512), p_all (rows, n_src), p_j (rows, n_src[estimate], n_src[source]) and the joint order reached (rows).
constexpr int BSS_PERM_BY_SDR = 0, BSS_PERM_BY_SIR = 1;
struct BssEvalDebug {
    double *r, *d, *pall, *pj;
    int* order;
};
size_t bss_eval_workspace_bytes(int B, int n_src, int n_other, int L, int with_mix);
int launch_bss_eval(const float* clean, const float* est, const float* mix, const float* other, int B, int n_src, int n_other, int L, void* ws,
                    size_t ws_bytes, float* sdr, float* sir, float* sar, float* sdr_i, int* perm, int perm_by, const BssEvalDebug& dbg,
                    hipStream_t st);
size_t bss_eval_many_workspace_bytes(const int* plan, int R, int n_other, int with_mix);
int launch_bss_eval_many(const float* const* mixes, const float* const* cleans, const float* const* ests, const float* const* others,
                         const int* table, const int* plan, int R, int n_src, int n_other, int fs, void* ws, size_t ws_bytes, float* sdr,
                         float* sir, float* sar, float* sdr_i, int* perm, int perm_by, hipStream_t st);

// long recordings in overlapping windows (k_longform.hip): window plan (host), framing of audio + video in one launch, cross-faded overlap-add
int longform_plan(int L, int Tv, int window, int hop, int* N);
// K lip tracks per recording (one track: K = 1): the audio window once, video_win (B*N*K, 512, window / SPF), target row (b*N + n)*K + k
int launch_longform_frame_speakers(const float* wav, const float* video, float* wav_win, float* video_win, int B, int K, int L, int Tv,
                                   int window, int hop, hipStream_t st);
int launch_longform_overlap_add(const float* y, float* out, int B, int n_src, int L, int window, int hop, hipStream_t st);
// many recordings of different lengths, their windows pooled (k_longform.hip): per-recording table (host), then the same two passes reading
// the recordings through device tables of pointers
int longform_many_plan(const long long* L, const long long* Tv, int R, int window, int hop, int n_src, long long* table, long long* total_windows,
                       long long* out_floats);
int launch_longform_frame_many(const float* const* wavs, const float* const* videos, const long long* table, float* wav_win, float* video_win,
                               int R, int total_windows, int window, int hop, hipStream_t st);
int launch_longform_overlap_add_many(const float* y, float* out, const long long* table, int R, int total_windows, long long out_floats,
                                     int n_src, int window, int hop, hipStream_t st);
// the same with K_r lip tracks per recording (AVNet.separate_many_speakers): 7 R table words [.. | K | trow0], target row trow0 + n K + k
int longform_many_speakers_plan(const long long* L, const long long* Tv, const long long* K, int R, int window, int hop, long long* table,
                                long long* total_windows, long long* total_targets, long long* out_floats);
int launch_longform_frame_many_speakers(const float* const* wavs, const float* const* videos, const long long* table, float* wav_win,
                                        float* video_win, int R, int total_windows, int max_K, int window, int hop, hipStream_t st);
int launch_longform_overlap_add_many_speakers(const float* y, float* out, const long long* table, int R, int total_windows, long long out_floats,
                                              int window, int hop, hipStream_t st);

// live streams chunk by chunk (k_live.hip): tick plan (host), chunk ingest + framing in one launch, overlap-add with a carried accumulator
int live_plan(const long long* slot_ids, const long long* counters, const long long* n_audio, const long long* n_video, int R, int slots,
              int flush, int window, int hop, int max_chunk, int n_src, long long* new_counters, long long* table, long long* sizes,
              int* refused);
int live_speakers_sizes_ok(int window, int hop, int max_chunk, int K);
// K lip tracks per slot (one track: K = 1); the table carries 1 + K columns of chunk pointers behind the plan's 13
int launch_live_ingest_frame_speakers(const long long* table, float* aring, float* vring, float* wav_win, float* video_win, int R, int rows,
                                      int K, int max_na, int max_nf, int window, int hop, int max_chunk, hipStream_t st);
int launch_live_overlap_add(const long long* table, const float* y, float* out, float* acc, int R, long long max_span, int n_src, int window,
                            int hop, int max_chunk, int flush, hipStream_t st);
// K scales the video ring, n_acc the accumulator rows
int launch_live_reset(const long long* ids, float* aring, float* vring, float* acc, int R, int K, int n_acc, int window, int max_chunk,
                      hipStream_t st);

// faces that come and go: Kmax planes per slot, a birth window per face; the table is documented at the faces section of k_live.hip
int live_faces_plan(const long long* slot_ids, const long long* counters, const long long* n_audio, const long long* n_video, int R, int slots,
                    int flush, int window, int hop, int max_chunk, int Kmax, const long long* births, int row_cap, long long* new_counters,
                    long long* table, long long* row_counts, long long* sizes, int* refused);
int launch_live_ingest_frame_faces(const long long* table, float* aring, float* vring, float* wav_win, float* video_win, int R, int rows,
                                   int Kmax, int max_na, int max_nf, int window, int hop, int max_chunk, hipStream_t st);
int launch_live_overlap_add_faces(const long long* table, const float* y, float* out, float* acc, int R, long long max_span, int Kmax,
                                  int window, int hop, int max_chunk, int flush, hipStream_t st);

// preparing raw recordings (k_prep.hip): uint8 mouth ROIs -> normalised lips, waveform normalisation, polyphase resampling
int launch_lips_prepare(const unsigned char* roi, const int* table, float* out, int N, int Tv, int H, int W, double mean, double stdv,
                        hipStream_t st);
// the same with frame selection: roi (N,Tv_in,H,W) at rate_num / rate_den fps -> out (N,1,P(Tv_in),88,88)
int launch_lips_prepare_rate(const unsigned char* roi, const int* table, float* out, int N, int Tv_in, int H, int W, double mean, double stdv,
                             int rate_num, int rate_den, hipStream_t st);
size_t wav_normalize_workspace_bytes(int B, int K, int L);
int launch_wav_normalize(const float* mix, const float* src, const float* std_in, float* mix_out, float* src_out, int B, int K, int L,
                         double eps, void* ws, size_t ws_bytes, hipStream_t st);
int resample_plan(int orig, int neu, int* o, int* n, int* width, int* taps, float* bank);
long long resample_out_len(int orig, int neu, long long L);
int launch_resample(const float* x, const float* bank, float* y, int B, int L, int orig, int neu, hipStream_t st);

// mouth ROIs from whole camera frames (k_mouth.hip): landmarks -> one affine map per (frame, face) (host), one sampling launch for J jobs
int mouth_affine(const double* eyes, const double* lips, long long n, int out_h, int out_w, int crop_h, int crop_w, double* A,
                 long long* refused);
int launch_mouth_rois(const long long* jobs, const long long* host_jobs, int J, int out_h, int out_w, hipStream_t st);

// video front-end (k_video.hip): FRCNNVideoModel, ResNet-18 trunk, PReLU, eval
size_t video_pack_floats();
size_t video_workspace_bytes(int B, int T);
int video_frontend(const float* lips, const float* pack, float* out, int B, int T, void* ws, size_t ws_bytes, hipStream_t st);
// the same from a caller's padded window volume (rows, 5, 94, 94), T = 1 per row: -> emb (n, 512) at the end of the workspace
size_t video_windows_workspace_bytes(int rows);
int video_frontend_windows(const float* windows, const float* pack, float* emb, int n, void* ws, size_t ws_bytes, hipStream_t st);

// live streams from camera frames (k_live_video.hip): tick plan (host), chunk ingest + stem windows in one launch, embedding scatter
int live_video_plan(const long long* slot_ids, const long long* counters, const long long* n_frames, int R, int slots, int flush,
                    int max_frames, long long* new_counters, long long* table, long long* sizes, int* refused);
// ... and at the camera's own frame rate (frame_rate.h): chunk sizes in camera frames, a fourth counter and a ninth table column
int live_video_rate_plan(const long long* slot_ids, const long long* counters, const long long* n_frames, int R, int slots, int flush,
                         int max_frames, int rate_num, int rate_den, long long* new_counters, long long* table, long long* sizes,
                         int* refused);
int frame_rate_map(int rate_num, int rate_den, long long n_in, long long* n_out, long long* src);
// rate_num = rate_den = 0: the chunks hold model frames (the table of live_video_plan)
int launch_live_video_ingest(const long long* table, float* hist, float* windows, int R, int rows, int max_m, int flush, bool u8, int H, int W,
                             int dy, int dx, double mean, double stdv, int rate_num, int rate_den, hipStream_t st);
// ... and with per-frame timestamps (frame_rate.h): seven counters, twelve table columns, the source list and the held plane
int live_video_stamp_plan(const long long* slot_ids, const long long* counters, const long long* n_frames, const long long* stamps,
                          const long long* until, int R, int slots, int flush, int max_frames, long long timebase, long long* new_counters,
                          long long* table, long long* sources, long long* sizes, int* refused);
int timestamp_map(const long long* stamps, long long n, long long timebase, long long until, long long* n_out, long long* src);
int launch_live_video_ingest_stamp(const long long* table, float* hist, float* held, float* windows, int R, int rows, int max_m, int max_cam,
                                   int flush, bool u8, int H, int W, int dy, int dx, double mean, double stdv, hipStream_t st);
int launch_live_video_stamp_reset(const long long* ids, float* hist, float* held, int R, hipStream_t st);
int launch_live_video_scatter(const float* emb, const long long* table, float* out, int R, int row_begin, int n, hipStream_t st);
int launch_live_video_reset(const long long* ids, float* hist, int R, hipStream_t st);

// live streams at the microphone's rate (k_live_resample.hip): tick plan (host), the polyphase resampler chunk by chunk in one launch
int live_resample_plan(const long long* slot_ids, const long long* counters, const long long* n_samples, int R, int slots, int flush,
                       int orig, int neu, long long max_chunk_in, long long* new_counters, long long* table, long long* sizes, int* refused);
int launch_live_resample(const long long* table, const float* bank, float* hist, float* out, int R, long long max_m, long long max_k,
                         int flush, bool i16, int orig, int neu, hipStream_t st);
int launch_live_resample_reset(const long long* ids, float* hist, int R, int orig, int neu, hipStream_t st);

// training-side GEMMs and SRU scans (k_train_gemm.hip, k_train_rnn.hip)
struct GemmArgs {
    const float *A = nullptr, *B = nullptr;
    float* C = nullptr;
    int lda = 0, ldb = 0, ldc = 0, M = 0, N = 0, K = 0;
    int ncb = 0, nrb = 0;  // NT: column / row blocks
    int kchunk = 0;        // TN: k range of one wave
    const float* bias = nullptr;  // NT modes 0/1: added per column
    size_t sA = 0, sB = 0, sC = 0;  // batch strides (blockIdx.y)
};
// C (M,N) [+]= A (M,K) . Bt (N,K)^T  (both K-contiguous; N % 64 == 0, K % 16 == 0)
// mode 0: C = ; 1: C += ; 2: C (rows x 64) [(row + colblk) * ldc + col % 64] += (atomics; the fold of unfold windows)
int launch_gemm_nt(const float* A, int lda, const float* Bt, int ldb, float* C, int ldc, int M, int N, int K, int mode,
                   hipStream_t st, const float* bias = nullptr, int batch = 1, size_t sA = 0, size_t sB = 0, size_t sC = 0);
// C (M,N) += A (K,M)^T . B (K,N)  (split-K with f32 atomics; M, N % 64 == 0)
int launch_gemm_tn(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, long K, hipStream_t st, int batch = 1,
                   size_t sA = 0, size_t sB = 0, size_t sC = 0);
struct SruScanArgs {
    const float* U = nullptr;    // (L, N, KC), column m*64 + dir*32 + j
    const float* xin = nullptr;  // (L, N, 64) highway input of layers 1-3; nullptr: U's m = 3 block (layer 0)
    const float* wc = nullptr;   // (128) v_f | v_r
    const float* bias = nullptr; // (128) b_f | b_r
    float* h = nullptr;          // forward: (L, N, 64)
    float* c = nullptr;          // forward: written; backward: read
    const float* g = nullptr;    // backward: dL/dh (L, N, 64)
    float* dU = nullptr;         // backward: (L, N, KC)
    float* dxp = nullptr;        // backward, layers 1-3: highway gradient (L, N, 64)
    float* dwc = nullptr;        // backward: (128) running sums
    float* dbias = nullptr;      // backward: (128)
    int L = 0, N = 0, KC = 0;
    long ts = 0, ns = 0;  // row of (step t, sequence n) = t*ts + n*ns
    int pad = 0;          // sequence-major dual-path layout: zero the 7 non-step rows of each slot
};
int launch_sru_scan_fwd(const SruScanArgs& a, hipStream_t st);
int launch_sru_scan_bwd(const SruScanArgs& a, hipStream_t st);
// dual-path training layout kernels: x (B, 64, R, Ls) <-> rows [n*Ls + s][64]
int launch_dp_ln_fwd(const float* x, const float* gamma, const float* beta, float* xn, int nseq, int R, int Ls, hipStream_t st);
int launch_dp_out(const float* y, const float* bias, const float* x, float* out, int nseq, int R, int Ls, hipStream_t st);
int launch_dp_dy(const float* dout, float* dy, float* dbias, int nseq, int R, int Ls, hipStream_t st);
int launch_dp_ln_bwd(const float* x, const float* dxn, const float* dout, const float* gamma, float* dx, float* dgamma, float* dbeta,
                     int nseq, int R, int Ls, hipStream_t st);
// channel-last ConvNormAct training kernels (k_train_conv.hip)
struct ClStageArgs {  // y = act(gLN(x)) over rows x C, per-sample statistics
    const float* x = nullptr;
    float* y = nullptr;
    const double* stats = nullptr;  // (B, 2) sum, sum of squares of x per sample (norm only)
    const float *gamma = nullptr, *beta = nullptr, *slope = nullptr;
    const float *rmean = nullptr, *rvar = nullptr;  // norm 2: BatchNorm running statistics (per channel)
    const double* cstats = nullptr;                 // norm 3: per-channel (sum, sum of squares) of this batch
    double inv_rows = 0;                            // norm 3: 1 / (rows over the whole batch)
    const float* dy = nullptr;  // backward
    float* dx = nullptr;
    double* S = nullptr;        // backward scratch (B, 2)
    float* partial = nullptr;   // backward: cl_stage_partial_floats(B, C) floats of per-workgroup sums (two-stage reduction)
    float *dgamma = nullptr, *dbeta = nullptr, *dslope = nullptr;
    size_t n = 0;               // elements per sample = rows per sample * C
    int C = 0, norm = 0, act = 0;
};
#define CL_DW_WGRAD_MAX_WG 2048
struct ClDwArgs {
    const float *x = nullptr, *w = nullptr, *bias = nullptr, *dy = nullptr;
    float *y = nullptr, *dx = nullptr, *dw = nullptr;
    float* scratch = nullptr;  // wgrad: CL_DW_WGRAD_MAX_WG x kh*kw x C per-workgroup partial sums
    int B = 0, H = 0, W = 0, C = 0, Ho = 0, Wo = 0, kh = 0, kw = 0, s = 1, pt = 0, pl = 0;
    int Cp = 0;  // row pitch in channels (set by the launcher; C is the slice a launch covers)
};
struct GatewayArgs {  // y = PReLU(w_c * (x + xr) + b_c) over n4 float4 of rows x C (C fastest)
    const float *x = nullptr, *xr = nullptr, *w = nullptr, *b = nullptr, *slope = nullptr, *dy = nullptr;
    float *y = nullptr, *dx = nullptr, *partial = nullptr;
    size_t n4 = 0;
    int C = 0;
};
int launch_gateway(const GatewayArgs& a, bool bwd, float* dw, float* db, float* dslope, hipStream_t st);
size_t cl_stage_partial_floats(int B, int C);
int launch_cl_norm_act_fwd(const ClStageArgs& a, int B, hipStream_t st);
int launch_cl_norm_act_bwd(const ClStageArgs& a, int B, hipStream_t st, int part = 0);
int launch_cl_colsum(const float* d, float* out, size_t n, int C, hipStream_t st, float* partial = nullptr);
int launch_cl_chan_stats(const float* x, double* stats, size_t n, int C, hipStream_t st);
int launch_bn_update(const double* stats, float* rmean, float* rvar, int C, double rows, float momentum, hipStream_t st);
int launch_cl_dw(const ClDwArgs& a, int what /* 0 fwd, 1 bwd data, 2 wgrad */, hipStream_t st);
// TF attention training kernels (k_train_attn.hip)
struct LngArgs {  // PReLU + LayerNormalization4D((C_group, 64)) over rows (b,t,f) x CZ
    const float* Z = nullptr;      // pre-activation rows
    float* Y = nullptr;            // forward output rows
    const float* res = nullptr;    // forward: optional residual rows added to Y (same shape)
    float* stats = nullptr;        // (B*T, 16, 2) mean, rstd per group (written forward, read backward)
    const float *slope = nullptr, *gamma = nullptr, *beta = nullptr;  // (CZ), (CZ,64), (CZ,64)
    const float* dY = nullptr;     // backward
    float* dZ = nullptr;
    float *dgamma = nullptr, *dbeta = nullptr, *dslope = nullptr;      // (CZ,64), (CZ,64), (ngroups)
    float* scratch = nullptr;      // backward: (workgroups, 2, CZ*64) partial sums of dgamma | dbeta
    int CZ = 0, ngroups = 0, nbt = 0;
    int gstart[17] = {0};
    unsigned char gof[128] = {0};  // channel -> group, 255 = padding channel
};
int launch_att_lng(const LngArgs& a, int nbt, bool bwd, hipStream_t st);
int launch_att_pack_qkv(float* rows, float* Qp, float* Kp, float* Vp, int B, int T, int Tp, int dir, hipStream_t st);
int launch_att_pack_o(float* rows, float* Op, int B, int T, int Tp, int dir, hipStream_t st);
int launch_att_softmax(float* S, const float* P, int nbatch, int T, int Tp, float scale, bool bwd, hipStream_t st);
int launch_pool2d(const float* x, float* y, size_t N, int H, int W, int Ho, int Wo, bool bwd, hipStream_t st, int C = 1);
int launch_tfar_combine(const float* le, const float* gate, const float* ge, float* out, size_t N, int H, int W, int Hg, int Wg, hipStream_t st,
                        int C = 1);
int launch_tfar_combine_bwd(const float* dout, const float* le, const float* gate, float* dle, float* dgate, float* dge, size_t N, int H, int W,
                            int Hg, int Wg, hipStream_t st, int C = 1);
int launch_patch3x3_rows(const float* z, float* rows, int B, int T, int F, hipStream_t st);
int launch_istft_adjoint(const float* dwav, float* dspec, int B, int T, int L, hipStream_t st);
int launch_cmul(const float* a, const float* b, float* out, int B, size_t half, int conj_a, hipStream_t st);
int launch_caf_att(const float* in, float* out, const float* dout, float* din, int nbc, int Tv, bool bwd, hipStream_t st);
int launch_caf_combine(const float* key, const float* value, const float* r, const float* att, float* out, size_t N, int T, int F, int Tv,
                       hipStream_t st);
int launch_caf_combine_rows(const float* key, const float* value, const float* r, const float* att, float* out, int B, int T, int F, int C, int Tv,
                            hipStream_t st);
int launch_caf_combine_rows_bwd(const float* dout, const float* key, const float* value, const float* r, const float* att, float* dkey,
                                float* dvalue, float* dr, float* datt, int B, int T, int F, int C, int Tv, hipStream_t st);
int launch_caf_combine_bwd(const float* dout, const float* key, const float* value, const float* r, const float* att, float* dkey,
                           float* dvalue, float* dr, float* datt, size_t N, int T, int F, int Tv, hipStream_t st);
int launch_pit_sdr_bwd(const float* est, const float* tgt, const int* perm, const float* dmin, float* dest, int B, int n, int L, int kind,
                       int zero_mean, int take_log, hipStream_t st);
int launch_ln_rows(const float* x, const float* gamma, const float* beta, float* y, const float* dy, float* dx, float* dgamma, float* dbeta,
                   size_t N, int C, bool bwd, hipStream_t st, const float* res = nullptr);
int launch_mha_core(const float* qkv, const float* pmask, float* o, const float* dout, float* dqkv, int B, int T, int nh, int hd, bool bwd,
                    hipStream_t st);
struct LstmScanArgs {
    const float* U = nullptr;     // forward: (rows, 256) pre-activations incl. both biases, column dir*128 + gate*32 + j
    const float* whh = nullptr;   // (2, 128, 32)
    float *G = nullptr, *c = nullptr, *h = nullptr, *hprev = nullptr;  // forward: written; backward: G, c read
    const float* g = nullptr;     // backward: dL/dh (rows, 64)
    float* dU = nullptr;          // backward: (rows, 256)
    int L = 0, N = 0, pad = 0;
    long ts = 0, ns = 0;
};
int launch_lstm_scan(const LstmScanArgs& a, bool bwd, hipStream_t st);
int launch_rows_bias_res(const float* y, const float* bias, const float* x, float* out, size_t n, int C, hipStream_t st);
int launch_rows_permute(const float* x, float* y, int B, int H, int W, int C, hipStream_t st);
size_t att_lng_scratch_floats(int nbt);
struct GruScanArgs {
    const float* U = nullptr;     // forward: (rows, 192) = W_ih x + b_ih, column dir*96 + gate*32 + j (gates r, z, n)
    const float* whh = nullptr;   // (2, 96, 32)
    const float* bhh = nullptr;   // (2, 96)
    float *S = nullptr, *h = nullptr, *hprev = nullptr;  // forward: written; backward: S, hprev read
    const float* g = nullptr;     // backward: dL/dh (rows, 64)
    float *dU = nullptr, *dHR = nullptr;  // backward: (rows, 192) each
    int L = 0, N = 0, pad = 0;
    long ts = 0, ns = 0;
};
int launch_gru_scan(const GruScanArgs& a, bool bwd, hipStream_t st);
