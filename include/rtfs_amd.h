/* rtfs_amd.h -- C ABI of the MI355X-native RTFS-Net separator forward pass (librtfs_amd.so).
 *
 * The reference (SutirthaChakraborty/RTFS-Net) has no FFI of its own: its hot path is the Python
 * nn.Module tree under AVNet.forward (src/models/tdavnet.py:86-97) plus ONE third-party native
 * operator, sru.SRU (src/models/layers/rnn_layers.py:99-105,150).  Each entry point below is what a
 * binding for one of those modules / that operator calls; the comment on each names the reference
 * interface it replaces.  INTEGRATION.md shows the ctypes stubs a maintainer would add.
 *
 * Conventions (all entry points):
 *   - raw DEVICE pointers, float32, contiguous row-major, reference layouts:
 *       spectrogram-shaped tensors (B, C, T, F) with F fastest; waveforms (B, L); lip embedding (B, 512, Tv)
 *   - `pack` = that module's parameters as ONE contiguous device buffer laid out as documented in
 *     rtfs-net_amd/packing.py (every tensor padded to a multiple of 64 floats, 1x1 weights stored
 *     transposed [cin][cout]); rtfs_pack_floats(kind) returns the expected length
 *   - caller allocates outputs and the workspace (size from the matching *_workspace_bytes query);
 *     kernels are enqueued on `stream` (a hipStream_t passed as void*), never synchronise, never
 *     allocate, never call back; workspace contents are scratch
 *   - return 0 on success; <0 on error: -1 bad shape, -2 workspace too small, -3 launch failure, -4 bad argument
 *   - eval-mode semantics (BatchNorm running statistics, no dropout); re-entrant: the only host-side state is a mutex-guarded cache
 *     of per-(device, kernel) launch attributes, the per-(device, caller stream) internal side streams of
 *     rtfs_separator_forward_f32 (forked from `stream` by an event and joined back into it inside the call: from outside all work of a call
 *     is ordered on `stream`), the process-wide DEFAULT of the batch split (rtfs_set_batch_split; the _ex entry points take it per call) and
 *     the diagnostic sweep-timing log (off by default), so the
 *     library may be driven from several host threads / devices in one process (one thread per stream).
 *   - length limits of the FUSED entry points (they keep a whole sweep / score row / video pyramid on chip and return -1 beyond):
 *       time sweep (dim 3) of rtfs_dualpath_sru_f32                                   <= 512 positions (8.2 s of audio)
 *       rtfs_block_f32, rtfs_separator_forward_f32 with the SRU cell (rnn_kind 0)      T/2 <= 512 (T <= 1025 frames: 8.2 s of audio)
 *       frequency sweep, rtfs_dualpath_lstm_f32, rtfs_block_f32 / rtfs_separator_forward_f32 with the LSTM cell (rnn_kind 1)
 *                                                                                     <= 250 positions (T/2 <= 250: 4 s of audio)
 *       keys of rtfs_tf_attention_f32                                                 <= 512
 *       video frames of rtfs_vp_block_f32                                             <= 256 (10.2 s at 25 fps)
 *     The reference has no length limit (rnn_layers.py:136-162, attention.py:149-189; infer_any_video.py:86 feeds whole files): longer
 *     inputs go through the UNFUSED entry points below (rtfs_*_forward_train_f32 and friends: GEMM + scan + GEMM sweeps, batched-GEMM
 *     attention, per-layer video block), which take any length; rtfs-net_amd/{models,layers}.py route by length (FUSED_MAX_*).
 *     Recordings past the fused limit are also served ON the fused path by the long-form entry points (rtfs_longform_*: overlapping
 *     windows of a length the fused separator takes, run as a batch and cross-faded back together; AVNet.separate_long).
 * F must satisfy F/2 == 64 wherever a block / attention is involved (the reference's n_freqs: 64 ties
 * LayerNormalization4D's parameters to 64 compressed frequency bins, config/lrs2_RTFSNet_4_layer.yaml:68).
 */
#ifndef RTFS_AMD_H
#define RTFS_AMD_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

enum rtfs_pack_kind {
    RTFS_PACK_ENCODER = 0,
    RTFS_PACK_AUDIO_BN = 1,
    RTFS_PACK_BLOCK = 2,
    RTFS_PACK_DUALPATH = 3,
    RTFS_PACK_ATTENTION = 4,
    RTFS_PACK_TFAR = 5,
    RTFS_PACK_CAF = 6,
    RTFS_PACK_S3 = 7,
    RTFS_PACK_DECODER = 8,
    RTFS_PACK_BLOCK_LSTM = 9,    /* RTFS block whose two DualPathRNN layers use rnn_type LSTM */
    RTFS_PACK_DUALPATH_LSTM = 10
};

/* library / build identification: returns "rtfs_amd <version> gfx950" */
const char* rtfs_version(void);
/* number of floats in a parameter pack of the given kind */
size_t rtfs_pack_floats(int kind);
/* frames of the STFT for a waveform of L samples: 1 + L/128 */
int rtfs_num_frames(int L);

/* STFTEncoder.forward (src/models/TDAVNet/encoder.py:161-175): wav (B,L) -> a0 (B,256,T,129).
 * workspace holds the (B,2,T,129) spectrogram.  If stats != NULL it receives (B,2) doubles
 * = (sum, sum of squares) of a0 per sample (consumed by the audio bottleneck's gLN). */
size_t rtfs_stft_encoder_workspace_bytes(int B, int L);
int rtfs_stft_encoder_f32(const float* wav, const float* pack, float* a0, double* stats, int B, int L, void* ws,
                          size_t ws_bytes, void* stream);

/* audio_bottleneck = ConvNormAct(gLN -> ReLU -> Conv2d 1x1 256->256) (tdavnet.py:59,89;
 * layers/conv_layers.py:65-129).  stats: (B,2) doubles of x as produced by the encoder, or NULL to
 * have them computed here (needs the workspace). */
size_t rtfs_audio_bottleneck_workspace_bytes(int B);
int rtfs_audio_bottleneck_f32(const float* x, const double* stats, const float* pack, float* out, int B, int T, int F,
                              void* ws, size_t ws_bytes, void* stream);

/* RTFS block = TDANetBlock.forward, is2d, upsampling_depth 2, globalatt = [DualPathRNN(F), DualPathRNN(T),
 * MultiHeadSelfAttention2D] (src/models/separators/tdanet.py:104-131).  x_res may be NULL; otherwise the block
 * input is x + x_res (RefinementModule's residual, refinement_module.py:51,60). */
size_t rtfs_block_workspace_bytes(int B, int T, int F);
int rtfs_block_f32(const float* x, const float* x_res, const float* pack, float* out, int B, int T, int F, void* ws,
                   size_t ws_bytes, void* stream, int rnn_kind /* 0 = SRU pack, 1 = LSTM pack */);

/* DualPathRNN.forward with rnn_type SRU, kernel 8, stride 1, 4 layers, bidirectional, hidden 32
 * (src/models/layers/rnn_layers.py:136-162).  x, out (B,64,T,F); dim = 4 sweeps along F (F <= 250), 3 along T (T <= 512).  Past
 * T = 256 the batch runs in consecutive sub-batches of < 4 GB each (the sweep kernel's 32-bit offsets), any B; past T = 250 the sweep is
 * the f16x3 kernel whatever RTFS_GEMM_F32 says (the exact-f32 A/B kernels stop at 250). */
size_t rtfs_dualpath_workspace_bytes(int B, int T, int F);
int rtfs_dualpath_sru_f32(const float* x, const float* pack, float* out, int B, int T, int F, int dim, void* ws,
                          size_t ws_bytes, void* stream);

/* The same module with rnn_type LSTM = nn.LSTM(512, 32, num_layers 4, bidirectional) (rnn_layers.py:116-122), the
 * reference's stock-torch alternative cell; exact-f32 MFMA GEMMs + per-step recurrent term.  pack kind DUALPATH_LSTM. */
int rtfs_dualpath_lstm_f32(const float* x, const float* pack, float* out, int B, int T, int F, int dim, void* ws,
                           size_t ws_bytes, void* stream);

/* MultiHeadSelfAttention2D.forward, 4 heads, hid_chan 4, dim 3 (src/models/layers/attention.py:149-189). x (B,64,T,64). */
size_t rtfs_tf_attention_workspace_bytes(int B, int T);
int rtfs_tf_attention_f32(const float* x, const float* pack, float* out, int B, int T, void* ws, size_t ws_bytes,
                          void* stream);

/* InjectionMultiSum.forward (TFAR, src/models/layers/fusion.py:54-69): local (B,64,H,W), global (B,64,Hg,Wg). */
size_t rtfs_tfar_workspace_bytes(int B, int H, int W, int Hg, int Wg);
int rtfs_tfar_f32(const float* local, const float* global, const float* pack, float* out, int B, int H, int W, int Hg,
                  int Wg, void* ws, size_t ws_bytes, void* stream);

/* CAF = ATTNFusion.forward with video_fusion False -> ATTNFusionCell (src/models/TDAVNet/fusion.py:204-212,
 * src/models/layers/fusion.py:252-274): audio (B,256,T,F), video (B,512,Tv) -> fused audio. */
size_t rtfs_caf_workspace_bytes(int B, int Tv);
int rtfs_caf_f32(const float* audio, const float* video, const float* pack, float* out, int B, int T, int F, int Tv,
                 void* ws, size_t ws_bytes, void* stream);

/* VP block = the video-side 1-D TDANetBlock.forward (upsampling_depth 4, kernel 3, BatchNorm1d, GlobalAttention;
 * src/models/separators/tdanet.py:104-131 with yaml video_params): video (B,512,Tv) -> (B,512,Tv), Tv <= 256 (see the conventions).
 * One launch, one workgroup per sample: Tv <= 120 runs entirely in LDS; 121 <= Tv <= 256 stages its three full-rate 64 x Tv tensors in
 * out's own slice for the sample (so `out` must not alias `video`) and keeps the rest in LDS.
 * pack = rtfs-net_amd/packing.py:pack_vp (eval BatchNorm folded); rtfs_vp_pack_floats() returns its length. */
size_t rtfs_vp_pack_floats(void);
int rtfs_vp_block_f32(const float* video, const float* pack, float* out, int B, int Tv, void* stream);

/* S^3 = MaskGenerator.forward with RI_split, n_src 1 (src/models/TDAVNet/mask_generator.py:67-99):
 * refined, a0 (B,256,T,F) -> separated embedding (B,1,256,T,F). */
int rtfs_s3_mask_f32(const float* refined, const float* a0, const float* pack, float* out, int B, int T, int F,
                     void* stream);

/* STFTDecoder.forward (src/models/TDAVNet/decoder.py:110-132): x (B,1,256,T,129) -> wav (B,1,L). */
size_t rtfs_istft_decoder_workspace_bytes(int B, int T);
int rtfs_istft_decoder_f32(const float* x, const float* pack, float* wav, int B, int T, int L, void* ws, size_t ws_bytes,
                           void* stream);

/* The whole separator, AVNet.forward minus the (tiny, 0.004 GMAC) video-side VP block whose output the caller
 * passes in (src/models/tdavnet.py:86-97, refinement_module.py:45-62):
 *   encoder -> audio bottleneck -> block -> CAF(video_vp) -> (repeats-1) x block(+a1) -> S^3 -> decoder.
 * packs: encoder, audio_bn, block, caf, s3, decoder.  wav (B,L), video_vp (B,512,Tv) -> out (B,1,L).
 * video_ready: optional hipEvent_t (as void*, may be NULL) recorded by the caller after video_vp was produced on
 * ANOTHER stream; the library makes `stream` wait for it right before the CAF block, so the VP block overlaps the
 * encoder and the first RTFS block. */
size_t rtfs_separator_workspace_bytes(int B, int L, int Tv);
/* Throughput option of rtfs_separator_forward_f32 (process-wide, default 1 = off; 0 restores the default / RTFS_SPLIT): the batch is cut
 * into n parts (each >= 8 mixtures) that run as independent chains on internal side streams forked from and joined back into `stream`, so the
 * HBM-bound kernels of one part run beside the latency-bound sweeps of another (batch 32: 14.2 -> 13.0 ms with n = 2).  Results per mixture
 * do not depend on it.  Call it before rtfs_separator_workspace_bytes: the workspace layout follows the setting. */
int rtfs_set_batch_split(int n);
/* Route of the RTFS block's steps 15-17 (process-wide).  0 (default): by size - where a 64-channel full-resolution tensor of the call exceeds
 * the 256 MB memory-side cache (256e6 bytes; batch 31 at 2 s), fusion 0's output xf0 is not written: two launches rebuild it from c0 ("15 + 16": statistics of the concat
 * layer's local conv, "15 + 17": the apply) in place of the three that write it, read it for the statistic and read it again; 1: always the
 * three launches; 2: the two passes wherever their launcher takes the shape (tests and A/B runs).  RTFS_ERR_ARG outside 0..2. */
int rtfs_set_dw_two_pass(int mode);
/* The same option PER CALL (re-entrant: two host threads can pick different schedules): split = 1 .. 8 parts for this call, 0 = the process
 * default above.  The workspace query and the forward call must be given the same value. */
size_t rtfs_separator_workspace_bytes_ex(int B, int L, int Tv, int split);
int rtfs_separator_forward_ex_f32(const float* wav, const float* video_vp, const float* pack_enc, const float* pack_bn,
                                  const float* pack_block, const float* pack_caf, const float* pack_s3,
                                  const float* pack_dec, float* out, int B, int L, int Tv, int repeats, void* ws,
                                  size_t ws_bytes, void* stream, void* video_ready, int rnn_kind, int split);
int rtfs_separator_forward_f32(const float* wav, const float* video_vp, const float* pack_enc, const float* pack_bn,
                               const float* pack_block, const float* pack_caf, const float* pack_s3,
                               const float* pack_dec, float* out, int B, int L, int Tv, int repeats, void* ws,
                               size_t ws_bytes, void* stream, void* video_ready, int rnn_kind /* 0 SRU, 1 LSTM block pack */);

/* K target speakers of each mixture in one call: the reference separates a mixture once per visible speaker (its evaluation lists every
 * mixture once per speaker, side by side in one unshuffled batch: test.py:128-140, avspeech_dataset.py:81-84; inference on a video calls
 * the model once per face).  Only the part of the separator before the CAF depends on the audio alone (refinement_module.py:45-62: block 0
 * runs on the bottleneck output, the video enters after it): STFT, encoder statistics, bottleneck + block head and block 0's body run once
 * per mixture; the CAF boundary fans out to the B * K targets, and the other blocks, the mask, the decoder and the iSTFT run per target.
 * wav (B,L); video_vp (B*K,512,Tv) and out (B*K,1,L) per target, mixture-major: target t = b*K + k, so out reads as (B,K,L).  Target t's
 * result is what rtfs_separator_forward_ex_f32 returns for mixture b and lips t.  Same cells, length limits and -1 rules as the fused
 * separator; -4 for K < 1, K > 16, repeats < 2 (no CAF boundary to fan out at) or RTFS_GEMM_F32=1 (the unfused A/B sequence), all before
 * the first launch.  split cuts the MIXTURES (each part >= 8 of them) and a part carries its mixtures' targets; the workspace query takes
 * the same split, returns 0 for out-of-range arguments and for K = 1 asks no more than rtfs_separator_workspace_bytes_ex. */
size_t rtfs_separator_speakers_workspace_bytes(int B, int K, int L, int Tv, int split);
int rtfs_separator_speakers_f32(const float* wav, const float* video_vp, const float* pack_enc, const float* pack_bn,
                                const float* pack_block, const float* pack_caf, const float* pack_s3, const float* pack_dec,
                                float* out, int B, int K, int L, int Tv, int repeats, void* ws, size_t ws_bytes, void* stream,
                                void* video_ready, int rnn_kind, int split);

/* A different number of targets per mixture (AVNet.separate_speakers(counts=...)): mixture b has counts[b] targets, 1 <= counts[b] <=
 * RTFS_MAX_SPEAKERS; the targets are mixture-major, N = sum(counts).  wav (B,L); video_vp (N,512,Tv) and out (N,1,L) per target.  Target t's
 * result is what rtfs_separator_forward_ex_f32 returns for mixture mix_of[t] with lips t; with all counts equal to K it is bit for bit the
 * result of rtfs_separator_speakers_f32.  counts is a HOST array of B ints (it sizes the workspace and places the batch parts); mix_of is the
 * caller's DEVICE array of N ints, non-decreasing, mix_of[t] = the mixture of target t.  The call uploads nothing, allocates nothing and reads
 * nothing back, so with the table in place it can be captured in a HIP graph like the fixed-K entry.  The library TRUSTS that mix_of matches
 * counts (a table entry outside [0, B) reads outside the workspace): build it from counts.
 * The prefix runs on the B mixtures; the CAF boundary and the tail kernel read mix_of[t] where the fixed-K entry divides t by K; the
 * workspace is sized by B where it depends on the mixture and by N where it depends on the target.  split cuts the MIXTURES (each part >= 8
 * of them); a part carries its mixtures' targets, starts at the target sum(counts before its first mixture) and hands its kernels that
 * first mixture as the base the table entries are taken relative to.
 * Same cells, length limits and -1 / -4 rules as rtfs_separator_speakers_f32, and -4 for a NULL counts or mix_of, a count outside 1 .. 16 or
 * N != sum(counts), all before the first launch and before any device call.  The workspace query returns 0 for such arguments and, with all
 * counts equal to K, what rtfs_separator_speakers_workspace_bytes(B, K, ...) returns. */
size_t rtfs_separator_targets_workspace_bytes(const int* counts, int B, int L, int Tv, int split);
int rtfs_separator_targets_f32(const float* wav, const float* video_vp, const int* counts, const int* mix_of, const float* pack_enc,
                               const float* pack_bn, const float* pack_block, const float* pack_caf, const float* pack_s3,
                               const float* pack_dec, float* out, int B, int N, int L, int Tv, int repeats, void* ws, size_t ws_bytes,
                               void* stream, void* video_ready, int rnn_kind, int split);

/* Operator-level seam: sru.SRU(input_size=512, hidden_size=32, num_layers=4, bidirectional=True).forward
 * (call site src/models/layers/rnn_layers.py:150; third-party asappresearch `sru`, v2 recurrence).
 * x (L,N,512) -> h (L,N,64).  pack = the DUALPATH pack (only its SRU part is read). */
size_t rtfs_sru_workspace_bytes(int L, int N);
int rtfs_sru_f32(const float* x, const float* pack, float* h, int L, int N, void* ws, size_t ws_bytes, void* stream);

/* Training side of the same operator (upstream sru's forward/backward pair behind
 * rnn_layers.py:150 when the module is used from train.py).  The forward keeps U = x.W, the cell states and the
 * inter-layer activations of all four layers in `saved` (rtfs_sru_saved_floats(L,N) floats, caller-owned) for the backward.
 * tpack (rtfs_sru_train_pack_floats() floats, rtfs-net_amd/packing.py:pack_sru_train):
 *   Wt0 (256,512) | Wt1..3 (192,64) | Wp0 (512,256) | Wp1..3 (64,192) | weight_c (4,128) | bias (4,128)
 *   with Wt = Wp^T and projection columns re-ordered to m*64 + dir*32 + j.
 * backward: dh (L,N,64) -> dx (L,N,512) and dparams (rtfs_sru_grad_floats() floats, overwritten):
 *   dWp0 (512,256) | dWp1..3 (64,192) | d weight_c (4,128) | d bias (4,128). */
size_t rtfs_sru_train_pack_floats(void);
size_t rtfs_sru_grad_floats(void);
size_t rtfs_sru_saved_floats(int L, int N);
size_t rtfs_sru_backward_workspace_bytes(int L, int N);
int rtfs_sru_forward_train_f32(const float* x, const float* tpack, float* h, float* saved, int L, int N, void* stream);
int rtfs_sru_backward_f32(const float* x, const float* tpack, const float* saved, const float* dh, float* dx, float* dparams,
                          int L, int N, void* ws, size_t ws_bytes, void* stream);
/* DualPathRNN.forward / backward for training (src/models/layers/rnn_layers.py:136-162), one set of six symbols per
 * cell: rtfs_dualpath_* (rnn_type SRU), rtfs_dualpath_lstm_* (LSTM), rtfs_dualpath_gru_* (GRU).  Common to the three:
 * x, out, dout, dx (B,64,T,F); dim as in the reference (4: sweep along F, 3: along T).  `saved` (*_saved_floats) is written by the forward
 * and read by the backward; the same workspace size (*_train_workspace_bytes) serves both; dparams (*_grad_floats()) is overwritten.
 * Refused: RTFS_ERR_ARG (null pointer, B < 1, dim), then RTFS_ERR_SHAPE (sweep axis < 8; backward: > 256), then RTFS_ERR_WORKSPACE.
 * Every tpack starts with LN gamma (64) | LN beta (64) and ends with the ConvTranspose1d weight as (co, (7-k)*64 + ci) | as
 * (ci, k*64 + co) | bias (64); every dparams starts with dgamma | dbeta and ends with d ConvTranspose1d weight as ((7-k)*64 + ci, co) | d bias.
 *
 * SRU cell.  dim 14 / 13 (this cell only; the others answer RTFS_ERR_ARG): the same sweeps with x, out, dout, dx as rows (B,T,F,64) (the
 * layout the training kernels of a block hand each other; size queries take the plain 4 / 3).
 * tpack (rtfs_dualpath_train_pack_floats(), packing.py:pack_dualpath_train), between the common parts: SRU training pack with layer-0
 *   rows in k*64 + c order.
 * dparams (rtfs_dualpath_grad_floats()): SRU gradients (rtfs_sru_backward_f32 layout, layer-0 rows k*64 + c). */
size_t rtfs_dualpath_train_pack_floats(void);
size_t rtfs_dualpath_grad_floats(void);
size_t rtfs_dualpath_saved_floats(int B, int T, int F, int dim);
size_t rtfs_dualpath_train_workspace_bytes(int B, int T, int F, int dim);
int rtfs_dualpath_forward_train_f32(const float* x, const float* tpack, float* out, float* saved, int B, int T, int F, int dim,
                                    void* ws, size_t ws_bytes, void* stream);
int rtfs_dualpath_backward_f32(const float* x, const float* tpack, const float* saved, const float* dout, float* dx,
                               float* dparams, int B, int T, int F, int dim, void* ws, size_t ws_bytes, void* stream);
/* LSTM cell (rnn_layers.py:116-122: nn.LSTM(512, 32, 4 layers, bidirectional)).
 * tpack (rtfs_dualpath_lstm_train_pack_floats(), packing.py:pack_dualpath_lstm_train), between the common parts: per layer [W_ih both
 *   directions (256, Din), rows dir*128 + gate*32 + j, layer-0 columns in k*64 + c order | its transpose | b_ih + b_hh (256) | W_hh (2,128,32)].
 * dparams (rtfs_dualpath_lstm_grad_floats()): per layer [dW_ih (256, Din) | d bias (256; the gradient of b_ih and of b_hh alike) |
 *   dW_hh (2,128,32)]. */
size_t rtfs_dualpath_lstm_train_pack_floats(void);
size_t rtfs_dualpath_lstm_grad_floats(void);
size_t rtfs_dualpath_lstm_saved_floats(int B, int T, int F, int dim);
size_t rtfs_dualpath_lstm_train_workspace_bytes(int B, int T, int F, int dim);
int rtfs_dualpath_lstm_forward_train_f32(const float* x, const float* tpack, float* out, float* saved, int B, int T, int F, int dim,
                                         void* ws, size_t ws_bytes, void* stream);
int rtfs_dualpath_lstm_backward_f32(const float* x, const float* tpack, const float* saved, const float* dout, float* dx,
                                    float* dparams, int B, int T, int F, int dim, void* ws, size_t ws_bytes, void* stream);
/* GRU cell (rnn_layers.py:116-122: nn.GRU(512, 32, 4 layers, bidirectional); gates r, z, n).  There is no fused inference kernel for
 * this cell (no reference yaml uses it in a DualPathRNN): the forward below also serves inference.
 * tpack (rtfs_dualpath_gru_train_pack_floats(), packing.py:pack_dualpath_gru_train), between the common parts: per layer [W_ih both
 *   directions (192, Din), rows dir*96 + gate*32 + j, layer-0 columns in k*64 + c order | its transpose | b_ih (192) | W_hh (2,96,32) |
 *   b_hh (192)].
 * dparams (rtfs_dualpath_gru_grad_floats()): per layer [dW_ih | db_ih | dW_hh | db_hh]. */
size_t rtfs_dualpath_gru_train_pack_floats(void);
size_t rtfs_dualpath_gru_grad_floats(void);
size_t rtfs_dualpath_gru_saved_floats(int B, int T, int F, int dim);
size_t rtfs_dualpath_gru_train_workspace_bytes(int B, int T, int F, int dim);
int rtfs_dualpath_gru_forward_train_f32(const float* x, const float* tpack, float* out, float* saved, int B, int T, int F, int dim,
                                        void* ws, size_t ws_bytes, void* stream);
int rtfs_dualpath_gru_backward_f32(const float* x, const float* tpack, const float* saved, const float* dout, float* dx, float* dparams,
                                   int B, int T, int F, int dim, void* ws, size_t ws_bytes, void* stream);
/* ConvNormAct.forward / backward for training (src/models/layers/conv_layers.py:65-129: pre_norm -> pre_act -> conv -> norm -> act),
 * 1x1 dense (channels up to 1024) or depthwise k x k (taps up to 4 x 5, stride 1 "same" or stride 2 symmetric; stride 2 on a map whose
 * padded height or width is below k is RTFS_ERR_SHAPE, as in nn.Conv), norms: none | gLN |
 * BatchNorm (post-norm only; frozen running statistics, or train mode = statistics of the batch), acts: none | ReLU | PReLU | Sigmoid.
 * cfg (HOST int[15]): Cin, Cout, k, stride, depthwise, pre_norm (0/1), pre_act (0 none, 1 ReLU, 2 PReLU, 3 Sigmoid), norm (0 none, 1 gLN,
 *   2 frozen BatchNorm, 3 train-mode BatchNorm), act, has_bias, is2d, phase, world, in_rows, out_rows.
 *   in_rows / out_rows: the input / output (and their gradients) are (B, H, W, C) rows instead of (B, C, H, W): modules chained inside a
 *   training step hand rows to each other and skip the layout changes; a rows input is not copied into `saved`, the backward takes it
 *   again as `x` (NULL otherwise).
 *   phase / world serve SyncBatchNorm (norm 3 only): phase 1 runs the forward up to the batch statistics (rtfs_cna_saved_stats_offset:
 *   2*Cout doubles inside `saved`, which the caller all-reduces), phase 2 resumes with the normalisation over rows * world samples; the
 *   backward likewise stops after the dgamma / dbeta sums (rtfs_cna_grad_norm_offsets) and resumes with the input gradient; phase 0 =
 *   everything in one call, world = 1.  x (B,Cin,H,W) -> out (B,Cout,Ho,Wo) (rtfs_cna_out_shape).
 * params (rtfs_cna_param_floats, packing.py:pack_cna_train; every slot padded to 64 floats, unused slots ignored):
 *   pre gamma | pre beta | pre slope | W (Cout,Cin) or (C,kh*kw) | W^T (dense only) | bias | gamma | beta | slope | running mean | running var.
 * dparams (rtfs_cna_grad_floats, overwritten): the slots pre gamma ... slope without W^T. */
size_t rtfs_cna_param_floats(const int* cfg);
size_t rtfs_cna_grad_floats(const int* cfg);
size_t rtfs_cna_saved_floats(const int* cfg, int B, int H, int W);
size_t rtfs_cna_workspace_bytes(const int* cfg, int B, int H, int W);
void rtfs_cna_out_shape(const int* cfg, int H, int W, int* Ho, int* Wo);
size_t rtfs_cna_saved_stats_offset(const int* cfg, int B, int H, int W);
void rtfs_cna_grad_norm_offsets(const int* cfg, size_t* dgamma, size_t* dbeta);
int rtfs_cna_forward_train_f32(const float* x, const float* params, float* out, float* saved, const int* cfg, int B, int H, int W,
                               void* ws, size_t ws_bytes, void* stream);
int rtfs_cna_backward_f32(const float* x, const float* params, const float* saved, const float* dout, float* dx, float* dparams,
                          const int* cfg, int B, int H, int W, void* ws, size_t ws_bytes, void* stream);
/* after a forward with norm = 3: nn.BatchNorm's running_mean / running_var update (momentum, unbiased variance) from the batch
 * statistics kept in `saved`; the two pointers are the module's buffers on the device. */
int rtfs_cna_bn_update_f32(const float* saved, const int* cfg, int B, int H, int W, float* running_mean, float* running_var,
                           float momentum, void* stream);
/* MultiHeadSelfAttention2D.forward / backward for training (src/models/layers/attention.py:149-189; 4 heads, hid_chan 4, n_freqs 64).
 * x, out, dout, dx (B,64,T,64).  tpack (rtfs_tf_attention_train_pack_floats(), packing.py:pack_attention_train):
 *   W_qkv (128,64) rows [Q h0..3 (4 each) | K h0..3 | V h0..3 (16 each) | 32 zero rows] | its transpose | bias (128) | PReLU slope per
 *   row (128) | LN gamma (128,64) | LN beta (128,64) | W_proj (64,64) | its transpose | bias (64) | slope per row (64) | gamma (64,64) | beta.
 * dparams (rtfs_tf_attention_grad_floats(), overwritten): dW_qkv | dbias (128) | dslope per module (64 slots, 12 used: Q h0..3, K h0..3,
 *   V h0..3) | dgamma (128,64) | dbeta | dW_proj | dbias (64) | dslope (64 slots, 1 used) | dgamma (64,64) | dbeta. */
size_t rtfs_tf_attention_train_pack_floats(void);
size_t rtfs_tf_attention_grad_floats(void);
size_t rtfs_tf_attention_saved_floats(int B, int T);
size_t rtfs_tf_attention_train_workspace_bytes(int B, int T);
/* rows != 0: x, out, dout, dx are rows (B, T, 64 f, 64 c) instead of (B, 64, T, 64); a rows input is read in place and handed to the
 * backward again as `x` (NULL otherwise). */
int rtfs_tf_attention_forward_train_f32(const float* x, const float* tpack, float* out, float* saved, int B, int T, int rows, void* ws,
                                        size_t ws_bytes, void* stream);
int rtfs_tf_attention_backward_f32(const float* x, const float* tpack, const float* saved, const float* dout, float* dx, float* dparams,
                                   int B, int T, int rows, void* ws, size_t ws_bytes, void* stream);
/* Layout change between the reference's (B, C, P) and the rows (B, P, C) the training kernels hand each other (to_rows != 0: the
 * former to the latter); each direction is the other's adjoint. */
int rtfs_layout_f32(const float* x, float* y, int B, int C, int P, int to_rows, void* stream);

/* Glue of the RTFS block with its adjoints (training side).  inner = 1: channel-first planes (N = B*C, H, W); inner = C > 1: rows
 * (N = B, H, W, C), channels fastest (what the training kernels hand each other inside a block).
 * F.adaptive_avg_pool2d as called at separators/tdanet.py:116 and its adjoint;
 * the last line of InjectionMultiSum.forward (layers/fusion.py:54-69): out = local * up(gate) + up(glob), up = nearest
 * interpolation (Hg, Wg) -> (H, W) (identity when equal), and its adjoint (dlocal like local; dgate, dglob like gate). */
int rtfs_adaptive_avg_pool2d_f32(const float* x, float* y, int N, int H, int W, int Ho, int Wo, int inner, void* stream);
int rtfs_adaptive_avg_pool2d_backward_f32(const float* dy, float* dx, int N, int H, int W, int Ho, int Wo, int inner, void* stream);
int rtfs_tfar_combine_f32(const float* local, const float* gate, const float* glob, float* out, int N, int H, int W, int Hg, int Wg,
                          int inner, void* stream);
int rtfs_tfar_combine_backward_f32(const float* dout, const float* local, const float* gate, float* dlocal, float* dgate, float* dglob,
                                   int N, int H, int W, int Hg, int Wg, int inner, void* stream);
/* Training side of STFTEncoder / STFTDecoder / the S^3 multiply.
 * Encoder (encoder.py:161-175): the waveform is data, so only the Conv2d(2->256, 3x3) weight has a gradient: dw (256,2,3,3) from
 *   wav (B,L) and da0 (B,256,T,129).
 * Decoder (decoder.py:110-132): dwav (B,L) -> dx (B,256,T,129) and dw (256,2,3,3) (ConvTranspose2d weight as stored): the adjoint of
 *   torch.istft (window, overlap-add envelope, crop) followed by the adjoint of the transposed convolution.
 * S^3 (mask_generator.py:71-82): complex multiply of [re 128 | im 128]-split maps (B,256,P); conj_first selects conj(a) (x) b, which is
 *   the adjoint with respect to either factor. */
size_t rtfs_stft_encoder_backward_workspace_bytes(int B, int L);
int rtfs_stft_encoder_backward_f32(const float* wav, const float* da0, float* dw, int B, int L, void* ws, size_t ws_bytes, void* stream);
size_t rtfs_istft_decoder_backward_workspace_bytes(int B, int T);
int rtfs_istft_decoder_backward_f32(const float* x, const float* w, const float* dwav, float* dx, float* dw, int B, int T, int L, void* ws,
                                    size_t ws_bytes, void* stream);
int rtfs_s3_cmul_f32(const float* a, const float* b, float* out, int B, int P, int conj_first, void* stream);

/* Glue of ATTNFusionCell.forward (layers/fusion.py:252-274) with its adjoints (training side).
 * attention: att_embed (B, 4C, Tv) -> reshape (B, C, 4, Tv) -> mean over the 4 -> softmax over Tv -> att (B, C, Tv).
 * combine: fused = key * up(resized) + up(att) * value with key/value/fused (N = B*C, T, F), resized/att (N, Tv), up = nearest
 * interpolation over time broadcast over F; the backward returns all four gradients. */
int rtfs_caf_attention_f32(const float* att_embed, float* att, int B, int C, int Tv, void* stream);
int rtfs_caf_attention_backward_f32(const float* att, const float* datt, float* datt_embed, int B, int C, int Tv, void* stream);
int rtfs_caf_combine_f32(const float* key, const float* value, const float* resized, const float* att, float* out, int N, int T, int F,
                         int Tv, void* stream);
int rtfs_caf_combine_backward_f32(const float* dout, const float* key, const float* value, const float* resized, const float* att,
                                  float* dkey, float* dvalue, float* dresized, float* datt, int N, int T, int F, int Tv, void* stream);
/* rtfs_caf_combine[_backward]_f32 on rows: key, value, out and their gradients (B, T, F, C) with C fastest; resized, att and their
 * gradients stay (B, C, Tv). */
int rtfs_caf_combine_rows_f32(const float* key, const float* value, const float* resized, const float* att, float* out, int B, int T, int F,
                              int C, int Tv, void* stream);
int rtfs_caf_combine_rows_backward_f32(const float* dout, const float* key, const float* value, const float* resized, const float* att,
                                       float* dkey, float* dvalue, float* dresized, float* datt, int B, int T, int F, int C, int Tv,
                                       void* stream);
/* The RTFS block's gateway on rows (B, T, F, C), C fastest (reference separators/tdanet.py:30-38 `gateway = ConvNormAct(in_chan, in_chan, 1,
 * groups=in_chan, act_type)` applied at :106-108 to `x + x_res`): out = PReLU(w_c * (x + x_res) + b_c) in one pass (x_res may be NULL);
 * backward in one pass: dx (the gradient of x and of x_res alike) and dparams = [dw C | db C | dslope 1] (each slot rounded up to 64
 * floats; rtfs_gateway_grad_floats).  w, b: the depthwise Conv2d's weight (C,1,1,1) and bias; slope: nn.PReLU's single weight. */
size_t rtfs_gateway_grad_floats(int C);
size_t rtfs_gateway_workspace_bytes(int C);
int rtfs_gateway_forward_train_f32(const float* x, const float* x_res, const float* w, const float* b, const float* slope, float* out,
                                   size_t rows, int C, void* stream);
int rtfs_gateway_backward_f32(const float* x, const float* x_res, const float* w, const float* b, const float* slope, const float* dout,
                              float* dx, float* dparams, size_t rows, int C, void* ws, size_t ws_bytes, void* stream);
/* Gradient of PITLossWrapper(PairwiseNegSDR) (src/losses/pit_wrapper.py:84-110 around matrix.py:22-53) with respect to the estimates,
 * for the permutation the forward chose: dmin_loss (B) = upstream gradient of min_loss, perm (B, n_src) as returned by
 * rtfs_pit_pairwise_sdr_f32 -> dests (B, n_src, L).  (The targets are data.) */
int rtfs_pit_sdr_backward_f32(const float* ests, const float* targets, const int* perm, const float* dmin_loss, float* dests, int B,
                              int n_src, int L, int sdr_type, int zero_mean, int take_log, void* stream);
/* Pieces of the video-side MultiHeadSelfAttention (src/models/layers/attention.py:28-73) with their adjoints, on rows (b, t) x C:
 * nn.LayerNorm over C; nn.Linear (in_proj / out_proj of nn.MultiheadAttention; N, K multiples of 64); the attention core
 * softmax(q k^T / sqrt(head_dim)) v on the packed projections [q | k | v] (T <= 256, head_dim <= 16), with an optional keep-mask
 * (B*n_head, T, T), already scaled by 1/(1-p), for the dropout nn.MultiheadAttention applies to the attention weights in train mode. */
int rtfs_layernorm_rows_f32(const float* x, const float* gamma, const float* beta, float* y, int N, int C, void* stream);
int rtfs_layernorm_rows_backward_f32(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, float* dbeta, int N,
                                     int C, void* stream);
int rtfs_linear_rows_f32(const float* x, const float* W, const float* bias, float* y, int M, int N, int K, void* stream);
int rtfs_linear_rows_backward_f32(const float* x, const float* W, const float* dy, float* dx, float* dW, float* dbias, int M, int N, int K,
                                  void* ws, size_t ws_bytes, void* stream);
int rtfs_mha_core_f32(const float* qkv, const float* pmask, float* o, int B, int T, int n_head, int head_dim, void* stream);
int rtfs_mha_core_backward_f32(const float* qkv, const float* pmask, const float* dout, float* dqkv, int B, int T, int n_head, int head_dim,
                               void* stream);
/* The two GEMM forms of the training path (bf16x3 split on the matrix cores), exposed for tests:
 * kind 0: C (M,N) = A (M,K) . B (N,K)^T (accumulate != 0: C += ...), N % 64 == 0, K % 16 == 0;
 * kind 1: C (M,N) += A (K,M)^T . B (K,N), M % 64 == 0, N % 64 == 0. */
int rtfs_debug_gemm_f32(int kind, const float* A, const float* B, float* C, int M, int N, int K, int accumulate, void* stream);

/* The inference depthwise family's launchers one at a time, exposed for tests (tests/test_hip_dw_edges.py).  It fills the launcher's
 * argument struct from the flat description, calls the production launcher, and returns the launcher's status unchanged (so the
 * RTFS_ERR_ARG "not eligible, fall back" answers of the fused launchers stay visible).  It zeroes no statistics: the caller does.
 *   op 0 stride-1 conv (nconv / in_affine / mode), 1 the three-job low-resolution launch (two descriptions: the 4-conv job, the folded
 *   1-conv job), 2 stride-2 + pool beside a MODE 1 statistics pass (two descriptions), 3 stride-2 + pool, 4 g = p0 + gLN(c1),
 *   5 the same-size combine gLN(l) * sigmoid(gLN(gate)) + gLN(emb), 6 / 7 two TFAR layers without the tensor between them (two descriptions:
 *   the first layer as op 0 takes it with in_affine, mode 2 and no addend - out[] unused; the second as op 0 takes its statistics pass (6:
 *   w[0], stats_out[0]) or its apply with addend == the first's x (7: w[0], out[0], the folds) - x unused; TH and rev are the second's).
 * One conv description is 35 device pointers, 14 ints and 4 doubles (a second one follows the first in each array):
 *   ptrs  0 x | 1 in_stats 2 in_gamma 3 in_beta | 4-7 w[k] | 8-11 bias[k] | 12-15 out[k] | 16-19 stats_out[k] | 20 loc_stats 21 loc_gamma
 *         22 loc_beta | 23 gate 24 gate_stats 25 gate_gamma 26 gate_beta | 27 emb 28 emb_stats 29 emb_gamma 30 emb_beta | 31 addend
 *         32 add_stats 33 add_gamma 34 add_beta
 *   ints  0 B 1 C 2 H 3 W 4 Hg 5 Wg 6 TH (requested band height) 7 cs (channel stride in floats, 0 = H * W) 8 rev 9 nconv 10 in_affine
 *         11 mode 12 in_combine 13 present (bits 0-3: bias[k], bit 4: addend; a pointer whose bit is clear is ignored)
 *   dbls  0 in_inv_count 1 loc_inv_count 2 g_inv_count 3 add_inv_count
 * op 4: ptrs p0, c1, c1_stats, gamma, beta, g; ints B, C, HW; dbls inv_count.
 * op 5: ptrs l, gate, emb, l_stats, gate_stats, emb_stats, l_gamma, l_beta, gate_gamma, gate_beta, emb_gamma, emb_beta, out; ints B, C, HW;
 *       dbls inv_count.
 * route (host ints, route_cap >= 33): route[0] = jobs launched (0 after a refusal), then per job family (1 one-column stride-1, 2 packed
 * stride-1, 3 three-job launch, 4 packed stride-2, 5 one-column stride-2, 6 stride-2 + statistics launch, 7 g_form, 8 g_combine, 9 two
 * TFAR layers in one launch: nconv 2, mode 1 = statistics pass / 2 = apply pass), nconv,
 * in_affine, mode, var (bit 0 addend, 1 shared gathers, 2 combined input, 3 row mapping, 4 whole-row mapping), effective TH, gx, gy.
 * Refused: RTFS_ERR_ARG (null array, short array, unknown op, B / C / H / W < 1) before any launcher runs. */
int rtfs_debug_dw_f32(int op, void* const* ptrs, int n_ptrs, const int* ints, int n_ints, const double* dbls, int n_dbls, int* route,
                      int route_cap, void* stream);

/* The inference pointwise (1x1 conv) family's launchers one at a time, exposed for tests (tests/test_hip_pw_edges.py).  It fills PwArgs,
 * B2bArgs, BnHeadArgs or TailS3Args (k_bnh.hip, k_s3f.hip: ops 8 and 9) from the flat description, calls ONE production launcher and returns the launcher's status unchanged (RTFS_ERR_ARG "does not
 * qualify, fall back" and RTFS_ERR_SHAPE stay visible).
 *   op 0 the exact-f32 launchers, 1 the first f16x3 generation (both: ints[11] = kind 0 audio bottleneck, 1 gateway + projection, 2 residual
 *   conv, 3 S3 mask, 4 decoder taps; contiguous rows only, cs must be 0), 2 streaming gateway + projection (x2 / CAF by the pointers given),
 *   3 block head on padded rows, 4 streaming residual conv, 5 first-generation block boundary, 6 block boundary on padded rows,
 *   7 register-resident 256 -> 256 (kind 0 audio bottleneck, 1 S3 mask, 2 S3 mask + decoder taps),
 *   8 fused bottleneck + first block head (launch_bn_head), 9 fused residual conv + S3 mask + decoder taps (launch_tail_s3t).  Ops 8 and 9
 *   first run the production launch_enc_stats on ints[14] mixtures, as the separator does: it adds the a0 statistics into `stats` (zeroed by
 *   the caller), writes the encoder fragment image (enc_img, 8192 floats) and the padded copy (wpad, 73728 floats) of the 256 -> 256 weight
 *   image w16 that the kernel reads.  Op 8: a1 = ptr 24 (written), res_out may be null.  Op 9: x, res_out (read only), out = z, w2_16 / bp =
 *   the residual conv's image and bias, w16 / bias = the mask conv's, xk = K (0: mix_of / mix_base), kind bit 0 = launch with stats null.
 *   ptrs (32)  0 x | 1 x2 | 2 res_out (ops 5, 6: res, in and out) | 3 wt | 4 w16 (ops 5, 6: w1_16) | 5 w16b | 6 bias (ops 5, 6: b1) | 7 aux
 *              8 out (ops 5, 6: xenc) | 9 stats 10 gamma 11 beta | 12 gw 13 gb 14 slope | 15 tile_ctr (null or one zeroed word)
 *              16 caf_r 17 caf_att 18 caf_w_key 19 caf_bn_key 20 caf_w_val 21 caf_bn_val 22 caf_rt 23 caf_attt | 24 a1 25 w2_16 26 bp 27 mix_of
 *              28 spec (mixtures, 2, T, F) 29 enc_w (256, 18) 30 enc_img 31 wpad
 *   ints (15)  0 B (ops 5, 6: targets of the launch) 1 P 2 cs (floats, 0 = P) 3 cout_live 4 caf_T 5 caf_F 6 caf_Tv 7 a1_mode 8 xk 9 a1k
 *              10 mix_base 11 kind 12 T 13 F 14 mixtures (ops 8, 9)
 *   dbls (1)   0 inv_count
 * route (host ints, route_cap >= 25): route[0] = kernels launched (0 after a refusal), then per kernel family (1 exact f32, 2 first f16x3
 * generation, 3 streaming gateway + projection, 4 streaming residual conv, 5 first-generation boundary, 6 boundary on padded rows, 7 head on
 * padded rows, 8 register-resident 256 -> 256), CIN, COUT, PRO, EPI, CAF, a1_mode, mode (family 8: MODE; family 3: HAS_X2), tiles per
 * sample, tiles, workgroups, 1 = tiles from the counter word / 0 = static stride.  Families 9 (fused head; mode = res written) and 10
 * (fused tail; mode = K) likewise; launch_enc_stats is not part of the record.
 * Refused: RTFS_ERR_ARG (null or short array, unknown op or kind, B / P < 1, cs != 0 for ops 0 and 1) before any launcher runs. */
int rtfs_debug_pw_f32(int op, void* const* ptrs, int n_ptrs, const int* ints, int n_ints, const double* dbls, int n_dbls, int* route,
                      int route_cap, void* stream);

/* The inference attention family's three launchers (k_attn.hip) one at a time, exposed for tests (tests/test_hip_attn_edges.py).  It fills
 * RowCanArgs / AttnArgs from the flat description (the Q/K/V group table by the helper attention() itself uses), calls ONE production
 * launcher and returns the launcher's status unchanged (launch_attn_core's RTFS_ERR_SHAPE past 512 keys stays visible).
 *   op 0 launch_row_can_qkv:  x, wt (64, 96), bias (96), slope (12), gamma / beta (96, 64) -> q, k (B,4,T,256), v (B,4,T,1024)
 *   op 1 launch_attn_core:    q, k, v -> out (B,64,T,64); dbls[0] = score scale, 0 = the 1/16 of the model
 *   As between the production launches, v holds 64 V (rtfs_debug_attn_vscale(); an exact power of two): op 0 writes it so, op 1 reads it so.
 *   op 2 launch_row_can_proj: x (the core's output, always channel-major), res, wt (64, 64), bias (64), slope (1), gamma / beta (64, 64) -> out
 *   ptrs (11)  0 x | 1 res | 2 wt 3 bias 4 slope 5 gamma 6 beta | 7 q 8 k 9 v | 10 out       (a pointer its op does not use is ignored)
 *   ints (3)   0 B 1 T 2 cl (op 0: x is channel-last (B,T,64 f,64 c); op 2: res is)
 *   dbls (1)   0 scale (op 1)
 * route (host ints, route_cap >= 8): route[0] = kernels launched (0 after a refusal), then family (1 Q/K/V rows, 2 core, 3 projection rows),
 * cl, frames per workgroup (core: 0), grid x, grid y, dynamic LDS bytes (rows: 0), (b, head) pairs (rows: 0).
 * Refused: RTFS_ERR_ARG (null or short array, a null pointer the op uses, unknown op, B < 1, T < 1) before any launcher runs. */
int rtfs_debug_attn_f32(int op, void* const* ptrs, int n_ptrs, const int* ints, int n_ints, const double* dbls, int n_dbls, int* route,
                        int route_cap, void* stream);
double rtfs_debug_attn_vscale(void);

/* Diagnostic build of the dual-path sweep with s_memtime stamps at phase boundaries (profiling aid only).
 * x, out: (B, 64, R, Ls) with sequences along the last axis; stamps: DEVICE u64 [ceil(B*R/seqs_per_wg)][16]. */
int rtfs_debug_sweep_stamps(const float* x, const float* pack, float* out, int B, int R, int Ls, unsigned long long* stamps,
                            void* stream);

/* Self test of the f16 MFMA fragment layout the split-precision GEMM kernels assume: D (32x32) = A (32x16) . B (16x32),
 * all DEVICE pointers, row-major; exact for small integer data. */
int rtfs_selftest_mfma_f16(const float* A, const float* B, float* D, void* stream);

/* Self test of the nearest up-sampling index rule every kernel shares (torch's float32 rule).  All DEVICE pointers,
 * int32.  pairs[2p], pairs[2p+1] = (n_in, n_out) with 1 <= n_in <= n_out; offsets[2p], offsets[2p+1] = where pair p's tables start in
 * out_src / out_first_dst.  One launch writes out_src[offsets[2p] + d] = source index read by destination d (d < n_out) and
 * out_first_dst[offsets[2p+1] + j] = first destination whose source is >= j (j <= n_in; n_out at j = n_in). */
int rtfs_selftest_nearest_index(const int* pairs, int n_pairs, const int* offsets, int* out_src, int* out_first_dst, void* stream);

/* Measurement hook (bench.py roofline leg; no reference counterpart).  While enabled (on = n > 0), every n-th launch of the fused
 * dual-path sweep kernel is bracketed by HIP events recorded on the stream it is launched on (on = 0: off).  collect() waits for
 * the recorded launches (host-side, call it outside any timed region / graph capture), writes per-launch
 * milliseconds + sequence length + sequence count (HOST pointers, up to cap entries), clears the log and returns the
 * number of entries (or <0 on error). */
int rtfs_sweep_timing_enable(int on);
/* Diagnostics: kernel launches issued by this library in this process so far (every launcher counts; memsets and event records do not).
 * tests/test_hip_parity.py pins the launches of one small-batch forward with it. */
unsigned long long rtfs_debug_launch_count(void);
int rtfs_sweep_timing_collect(float* ms, int* seq_len, int* n_seq, int cap);

/* Evaluation-side loss (the step after the path): PairwiseNegSDR.forward
 * (src/losses/matrix.py:22-53; sdr_type 0 = "snr", 1 = "sisdr", 2 = "sdsdr") followed by PITLossWrapper's factorial search
 * over source permutations (src/losses/pit_wrapper.py:84-110, pit_from = "pw_mtx", perm_reduce = None), n_src <= 4.
 * ests, targets (B, n_src, L) -> pw_loss (B, n_src[est], n_src[target]); min_loss (B) = loss of the best permutation;
 * perm (B, n_src) int32 with perm[b][i] = estimate assigned to target i (the reference's batch_indices, so
 * reordered[b][i] = ests[b][perm[b][i]]).  All device pointers; the batch mean of min_loss is the wrapper's return value. */
int rtfs_pit_pairwise_sdr_f32(const float* ests, const float* targets, int B, int n_src, int L, int sdr_type, int zero_mean,
                              int take_log, float* pw_loss, float* min_loss, int* perm, void* stream);

/* Evaluation metric (the reference's test-time scoring, src/metrics/allwrapper.py:57-62): classic STOI (Taal et al. 2011) as
 * pystoi 0.4.1 computes stoi(clean, estimate, fs, extended=False): resample to 10 kHz (pystoi utils.resample_oct), remove the frames
 * more than 40 dB below the clean signal's loudest, one-third-octave band envelopes of the 512-point STFT, mean correlation of
 * clipped, normalised 30-frame segments.  clean, est (B, L) -> d (B) float32 and kept_frames (B) int32 = frames silence removal kept
 * (a speech-activity count); d = 1e-5 when fewer than 30 STFT frames remain, as pystoi returns.  fs = 16000 or 10000 (no resampling),
 * any other rate returns -4 before any launch; L needs at least one 256-sample frame at 10 kHz (L >= 410 at 16 kHz, 257 at 10 kHz).
 * Rows are scored independently (a row's result does not depend on the batch); no atomics, capturable in a graph. */
size_t rtfs_stoi_workspace_bytes(int B, int L, int fs);
int rtfs_stoi_f32(const float* clean, const float* est, int B, int L, int fs, void* ws, size_t ws_bytes, float* d, int* kept_frames,
                  void* stream);

/* Scoring R recordings of different lengths in one pooled pass (metrics.stoi_many / sdr_many, ALLMetricsTracker.update_many): the
 * scoring half of AVNet.separate_many.  Recording r is L_r samples: mix (L_r), clean and est contiguous (n_src, L_r), each a separate
 * allocation at any 4-byte alignment, reached through DEVICE arrays of R device pointers (dword loads only, no packing copy).
 * rtfs_score_many_plan (host only, no device touched; the single place with the arithmetic): L (R lengths, host), n_src 1 .. 4, fs
 *   16000 | 10000 -> ws_bytes (may be NULL) and the RTFS_SCORE_COLS * (R + 1) int32 words of `table`, column-major: word
 *   table[c * (R + 1) + r] is column c of recording r, and row R closes the prefix sums.  Columns:
 *     0 L        the recording's length              row R: n_src   (rows R of columns 0 .. 3 record what the plan was made for;
 *     1 L10      its length at 10 kHz, ceil(5 L / 8) row R: fs       the launches compare them with their own arguments)
 *     2 K0       its frames before silence removal   row R: R
 *     3 Fmax     K0 - 1, the most STFT frames        row R: 0
 *     4 rs_off   where its 10 kHz copies start in the two resample regions, floats (all 0 at fs = 10000: nothing is resampled)
 *     5 fr_off   where its K0 frame energies / kept-frame indices start, elements
 *     6 bd_off   where its (Fmax, 15) band values start, frames
 *     7 rs0      its first resample chunk  (ceil(L10 / 1024) chunks; 0 at fs = 10000)
 *     8 bg0      its first band frame group (ceil(Fmax / 4) groups)
 *     9 cc0      its first correlation chunk = its first STOI partial (ceil(15 (Fmax - 29) / 256) chunks; 0 when Fmax < 30)
 *    10 mc0      its first moment chunk = its first moment partial (ceil(L / 4096) chunks of 4096 samples from ITS OWN start)
 *   Columns 4 .. 10 are exclusive prefix sums over the recordings, row R their totals.  The four flat work lists (7 .. 10) are the launch
 *   grids: workgroup w finds its recording by bisection (the last r with first[r] <= w), so no workgroup exists for padding up to the
 *   longest recording.  The workspace is RAGGED: nine regions (two resample copies, energies, kept indices, R kept counts, two band
 *   arrays, STOI partials, moment partials of 2 (2 n_src + 1) + n_src^2 + n_src doubles), each ONE array over all recordings sized by a
 *   total of row R and rounded up to 256 bytes, so ws_bytes grows with sum(L_r), not R * max(L_r), and stays within the sum of
 *   rtfs_stoi_workspace_bytes(1, L_r, fs) plus the moment partials (the only padding is 9 * 255 bytes per CALL, none per recording).
 *   Refused: -4 for a NULL L or table, R < 1, n_src outside 1 .. 4, fs not 16000 / 10000; -1 for a length rtfs_stoi_f32 refuses
 *   (L < 410 at 16 kHz, < 257 at 10 kHz, > 2^26) or a total past 2^31 - 1.
 * Both launches below take `table` = the DEVICE copy of those words (4-byte aligned; upload it together with the pointer arrays in ONE
 *   host-to-device copy) and `plan` = the HOST words the planner wrote, from which they size their grids and verify ws_bytes (-2) and
 *   that R, n_src and fs are the plan's (-4); NULL pointers are -4.  All refusals come before any launch.  Neither synchronises,
 *   allocates or calls back; both share one workspace (disjoint regions).  Because of the table upload a call is NOT capturable.
 * rtfs_stoi_many_f32: classic STOI of the R pairs (cleans[r][0 .. L_r), ests[r][0 .. L_r)): the five stages of rtfs_stoi_f32 with the
 *   recording's own L, L10, K0 and Fmax -> d (R) float32, kept_frames (R) int32.  A recording's arithmetic, lane assignment and fold
 *   order are those of rtfs_stoi_f32 with B = 1 (shared device code), so d[r] and kept_frames[r] are BIT-EQUAL to that call.
 * rtfs_sdr_many_f32: the metrics tracker's four PIT figures.  One pass accumulates in float64 the first and second moments of the
 *   2 n_src + 1 signals and the cross moments <est_i, clean_j>, <mix, clean_j>, one partial per moment chunk; a second launch folds each
 *   recording's partials in a fixed order and derives the snr and sisdr pairwise matrices of (est, clean) and (mix stacked n_src times,
 *   clean) as rtfs_pit_pairwise_sdr_f32 does (zero_mean, take_log, EPS 1e-8), best permutation in itertools order, first minimum.
 *   -> out (R, 4) float32 in the loss sign [sdr, sdr - baseline, sisnr, sisnr - baseline] and perm (R, n_src) int32 of the (est, clean)
 *   sisdr search.  The dB figures agree with four rtfs_pit_pairwise_sdr_f32 calls to float64 rounding of the moments, not bit for bit:
 *   the sums are chunked differently. */
#define RTFS_SCORE_COLS 11
int rtfs_score_many_plan(const long long* L, int R, int n_src, int fs, int* table, size_t* ws_bytes);
int rtfs_stoi_many_f32(const float* const* cleans, const float* const* ests, const int* table, const int* plan, int R, int n_src, int fs,
                       void* ws, size_t ws_bytes, float* d, int* kept_frames, void* stream);
int rtfs_sdr_many_f32(const float* const* mixes, const float* const* cleans, const float* const* ests, const int* table, const int* plan,
                      int R, int n_src, int fs, void* ws, size_t ws_bytes, float* out, int* perm, void* stream);

/* Extended STOI (ESTOI, Jensen & Taal 2016) as pystoi 0.4.1 computes stoi(clean, estimate, fs, extended=True), with two deliberate
 * differences (below).  Stages 1 .. 3 are those of rtfs_stoi_f32 (resampling to 10 kHz, silence removal, band values x, y of shape
 * (15, F)).  With F < 30 d_ext = 1e-5.  Otherwise each of the J = F - 29 segments (15 bands x 30 frames, one per m = 30 .. F) of x and of
 * y is normalised twice -- per band: minus its mean over the 30 frames, divided by its Euclidean norm; then per frame: minus its mean
 * over the 15 bands, divided by its norm -- and d_ext = sum(x_n * y_n) / 30 / J, in double, stored as float32.
 *   Noise: pystoi adds eps * standard_normal before each of the two normalisations; this library does not (on the test signals the
 *     terms move d by about 1e-16), so the result is deterministic.
 *   Zero norms: a norm of exactly zero gives the inverse 0 (inv = n > 0 ? 1 / n : 0), so a silent estimate and an all-zero clean signal
 *     score exactly 0.0 and nothing is ever NaN (pystoi's answer there is whatever its noise happens to be).
 *   pystoi is not installed where this project is developed: agreement with the package itself is not measured; the definition is
 *   tests/estoi_oracle.py.
 * Work cut: the correlation stage runs on the classic stage's work list, ceil(15 J / 256) chunks per row (column 9 of the pooled table);
 *   chunk c owns the segments s with floor(15 s / 256) == c (at most 18; a planned chunk may own none and then writes the partial 0.0).
 *   One writer per partial, fixed fold order, no atomics: a row's result does not depend on the batch or the pool.
 * rtfs_estoi_f32: clean, est (B, L) -> d_ext (B) float32, kept_frames (B) int32 and, when d_classic is not NULL, d_classic (B) = classic
 *   STOI from the same band values, BIT-EQUAL to rtfs_stoi_f32.  The workspace is that of rtfs_stoi_f32, plus one more region of B *
 *   nchunk partials when with_classic != 0 (pass with_classic = 1 to the size query exactly when d_classic is not NULL; a workspace sized
 *   with it also serves a call without).  Refusals as rtfs_stoi_f32, all before any launch: -4 for fs other than 16000 / 10000 or a NULL
 *   pointer (d_classic excepted), -1 for rows too short for one frame, -2 for a small workspace.  Capturable in a graph.
 * rtfs_estoi_many_f32: the same for R recordings of different lengths on rtfs_score_many_plan's table (arguments, checks and codes as
 *   rtfs_stoi_many_f32).  ESTOI alone fits the plan's own workspace (its partials take the STOI partial region).  With d_classic the
 *   ESTOI partials take a TENTH region of 8 * (total of column 9) bytes appended after the nine, starting at the next multiple of 256:
 *   rtfs_estoi_many_workspace_bytes(plan, R, 1) (0 for a NULL plan or one not made for R recordings); the nine existing offsets,
 *   those rtfs_sdr_many_f32 uses included, do not move.  d_ext[r] and d_classic[r] are BIT-EQUAL to rtfs_estoi_f32 on recording r alone
 *   (shared device code).  Not capturable (table upload). */
size_t rtfs_estoi_workspace_bytes(int B, int L, int fs, int with_classic);
int rtfs_estoi_f32(const float* clean, const float* est, int B, int L, int fs, void* ws, size_t ws_bytes, float* d_ext,
                   float* d_classic /* NULL: not wanted */, int* kept_frames, void* stream);
size_t rtfs_estoi_many_workspace_bytes(const int* plan, int R, int with_classic);
int rtfs_estoi_many_f32(const float* const* cleans, const float* const* ests, const int* table, const int* plan, int R, int n_src, int fs,
                        void* ws, size_t ws_bytes, float* d_ext, float* d_classic /* NULL: not wanted */, int* kept_frames, void* stream);

/* BSS-eval SDR: the SDR column of mir_eval.separation.bss_eval_sources / fast_bss_eval, the ratio after the estimate has been projected
 * onto the F = 512 delayed copies of the true source, so that a fixed delay or a short linear distortion is allowed (the "sdr" figure
 * of rtfs_sdr_many_f32 and of the reference's tracker is plain SNR: one sample of delay ruins it).  Definition, for a reference s and
 * an estimate e of L >= 1 float32 samples, ALL arithmetic in float64, F = 512 fixed (mir_eval's default), no mean removal:
 *     r[k] = sum_t s[t] s[t+k],  d[k] = sum_t s[t] e[t+k],  k = 0 .. 511 (terms past the end are absent; the products are exact)
 *     G = Toeplitz(r),  G c = d,  num = c'd,  ee = sum e^2,  den = max(ee - num, 0),  SDR = 10 log10(num / den)
 *   IEEE as it comes: +inf for den = 0 < num, -inf for num = 0 < den, NaN for 0 / 0.  This equals mir_eval's
 *   |s_target|^2 / |e_pad - s_target|^2 with s_target = s * c, the full convolution of length L + 511, and e zero-padded to that length.
 *   Solver: Levinson-Durbin.  Stop rule: when the prediction error at order k is <= r[0] 2^-46, or r[0] = 0, the recursion stops and taps
 *   k .. 511 are 0 (a silent reference gives c = 0: -inf, or NaN for a silent estimate as well).  It is a guard, not a measurement.
 *   Sources: with n_src = n <= 4 all n^2 values SDR(e_i, s_j) are formed (the estimates scored against s_j share G_j); the permutation
 *   maximises the mean SDR over the sources, scanned in itertools order, first maximum (fast_bss_eval's rule; mir_eval chooses by SIR,
 *   which needs the joint projection: see "BSS-eval SIR and SAR" below).  perm[b][j] = the estimate assigned to clean source j, the convention of
 *   rtfs_pit_pairwise_sdr_f32; sdr[b][j] = SDR(e_perm[b][j], s_j) in positive dB.  With a mixture the baseline of source j is
 *   SDR(mix, s_j) and sdr_i[b][j] = sdr[b][j] - baseline[j] (subtracted in float64, stored as float32).
 *   Agreement with the mir_eval package itself is not measured (it is not installed where this project is developed); the definition
 *   is tests/bss_oracle.py.
 * Work cut (three launches): correlation partials per (chunk of 4096 samples from the recording's own start, clean source, 256 lags),
 *   one writer each; per (recording, clean source) a fold of the partials in chunk order and the recursion for all right-hand sides at
 *   once; per recording the matrix, the search and the outputs.  No atomics: a row's bits depend on neither batch, pool nor scheduling.
 * rtfs_bss_sdr_f32: clean, est (B, n_src, L), mix (B, L) or NULL -> sdr (B, n_src) float32, sdr_i (B, n_src) float32 (required with mix,
 *   untouched without), perm (B, n_src) int32.  It allocates, uploads and reads back nothing: capturable in a graph.  Refused before any
 *   launch: -4 for a NULL pointer (mix excepted; sdr_i only with mix), B < 1, L < 1 or n_src outside 1 .. 4; -1 when B * ceil(L / 4096) *
 *   n_src * 2 workgroups exceed 2^31 - 1; -2 for a workspace below rtfs_bss_sdr_workspace_bytes(B, n_src, L, mix != NULL) (0 for
 *   arguments the call refuses; a workspace sized with_mix = 1 also serves a call without).
 * rtfs_bss_sdr_many_f32: the same for R recordings of different lengths on rtfs_score_many_plan's table, of which it uses columns 0 and
 *   10 only; arguments, checks and codes as rtfs_stoi_many_f32 (mixes may be NULL, then sdr_i is untouched).  The workspace is its own,
 *   rtfs_bss_sdr_many_workspace_bytes(plan, R, with_mix) (0 for a NULL plan or one not made for R recordings): RTFS_SCORE_COLS and the
 *   regions of the plan's workspace do not move.  The kernels are those of rtfs_bss_sdr_f32, so row r is BIT-EQUAL to that call on
 *   recording r alone.  Not capturable (table upload).
 * rtfs_debug_bss_f64: rtfs_bss_sdr_f32 that also copies out, per (row b, clean source j) at index b n_src + j, the folded r_j (512
 *   doubles), the d rows (NR = n_src + (mix != NULL) rows of 512: the estimates, then the mixture), the ee values (NR) and the order
 *   the recursion reached (int32; 512 = the guard did not fire).  form: 0 = the production solver, 512 = one thread per tap (two
 *   barriers per order), 64 = a single wave with 8 taps per lane; -4 for another value or a NULL debug pointer. */
size_t rtfs_bss_sdr_workspace_bytes(int B, int n_src, int L, int with_mix);
int rtfs_bss_sdr_f32(const float* clean, const float* est, const float* mix /* NULL: no baseline */, int B, int n_src, int L, void* ws,
                     size_t ws_bytes, float* sdr, float* sdr_i, int* perm, void* stream);
size_t rtfs_bss_sdr_many_workspace_bytes(const int* plan, int R, int with_mix);
int rtfs_bss_sdr_many_f32(const float* const* mixes /* NULL: no baseline */, const float* const* cleans, const float* const* ests,
                          const int* table, const int* plan, int R, int n_src, int fs, void* ws, size_t ws_bytes, float* sdr, float* sdr_i,
                          int* perm, void* stream);
int rtfs_debug_bss_f64(const float* clean, const float* est, const float* mix, int B, int n_src, int L, void* ws, size_t ws_bytes, float* sdr,
                       float* sdr_i, int* perm, int form, double* r_out, double* d_out, double* ee_out, int* order_out, void* stream);

/* BSS-eval SIR and SAR: the other two time-domain ratios of mir_eval.separation.bss_eval_sources, which need the projection of the
 * estimate onto the delayed copies of ALL true sources at once.  True sources s_0 .. s_{J-1}: the n = n_src clean sources that the
 * estimates are scored against, then m = n_other "other" sources (an interfering talker, noise) that belong to the span but are not
 * scored; J = n + m, 1 <= n, J <= 4.  Estimate e, L float32 samples, ALL arithmetic in float64, F = 512, no mean removal:
 *     r_ij[k] = sum_t s_i[t] s_j[t+k],  k = -511 .. 511   (r_ij[-k] = r_ji[k]; terms past the end are absent)
 *     d_i[k]  = sum_t s_i[t] e[t+k],    k = 0 .. 511,     ee = sum e^2
 *     G_all   = the (J 512)^2 matrix with G[(i,a),(j,b)] = r_ij[a-b],  G_all C = D_all,  p_all = C'D_all   (|P_all e|^2)
 *     p_j     = c_j'd_j with Toeplitz(r_jj) c_j = d_j                 (|s_target|^2, the num of "BSS-eval SDR")
 *     SDR_j = 10 log10(p_j / max(ee - p_j, 0))       (the value of rtfs_bss_sdr_f32, bit for bit)
 *     SIR_j = 10 log10(p_j / max(p_all - p_j, 0))
 *     SAR   = 10 log10(p_all / max(ee - p_all, 0))
 *   These are mir_eval's |s_target|^2 / |e_interf|^2 and |s_target + e_interf|^2 / |e_artif|^2 with s_target = s_j * c_j, e_interf =
 *   P_all e - s_target and e_artif = e_pad - P_all e on the zero-padded length L + 511 (e_interf is orthogonal to s_target, so the closed
 *   forms hold).  IEEE as it comes (+-inf, NaN for 0/0), as for the SDR.
 *   Solver: block Levinson with J x J blocks over the 512 orders (tap-major ordering: G_all is block-Toeplitz with blocks M[k][i][j] =
 *   r_ij[k], M[-k] = M[k]'), forward and backward block predictors, the error blocks E_f and E_b of every order inverted by Gauss-Jordan
 *   without pivoting.  Stop rule, the scalar one generalised: the recursion ends at order m, taps m .. 511 stay 0, when a pivot of the
 *   order's E_f or E_b is <= 2^-46 r_ii[0] of its source i (order 0: the block M[0]; two identical sources stop there, p_all = 0).  It is
 *   a guard, not a measurement.  A source with r_jj[0] = 0 (silent) is left out of the joint set and its taps are 0.  When the joint set
 *   is one scored source, P_all is that source's scalar projection and p_all is taken from the scalar solve: SIR = +inf and SAR = SDR
 *   bit for bit, for J = 1 and for n = 1 with silent others alike (a single-talker segment does not turn into NaN).  An empty joint set
 *   has p_all = 0.  G_all is the Gram matrix of 512 J vectors in R^(L + 511): rows shorter than 512 J + 512 samples are rank-deficient or
 *   close to it and belong with the degenerate rows (the call finishes; the figures are whatever the stop rule leaves).
 *   Permutation, perm_by: RTFS_BSS_PERM_BY_SDR (0) the rule of rtfs_bss_sdr_f32 -- then sdr, sdr_i and perm ARE that call's, bit for bit
 *   -- or RTFS_BSS_PERM_BY_SIR (1) mir_eval's rule: the largest mean over the sources of SIR(e_perm[j], s_j), itertools order, first
 *   maximum.  sir[b][j] = SIR(e_perm[b][j], s_j); sar[b][j] = SAR(e_perm[b][j]).
 *   Agreement with the mir_eval package itself is not measured (it is not installed where this project is developed); the definition
 *   is tests/bss_eval_oracle.py.
 * Work cut (four launches): the correlation partials of "BSS-eval SDR" with every one of the J sources staged and the J sources and n
 *   estimates (for a scored source also the mixture) as right-hand signals; the scalar solves, unchanged; one workgroup per recording
 *   for the fold in chunk order and the block recursion for all n estimates at once; one thread per recording for the matrices, the
 *   search and the outputs.  No atomics: a row's bits depend on neither batch, pool nor scheduling.
 * rtfs_bss_eval_f32: clean, est (B, n_src, L), mix (B, L) or NULL, other (B, n_other, L) or NULL -> sdr, sir, sar (B, n_src) float32,
 *   sdr_i (B, n_src) (required with mix, untouched without), perm (B, n_src) int32.  It allocates, uploads and reads back nothing:
 *   capturable in a graph.  Refused before any launch: -4 for a NULL pointer (mix excepted; sdr_i only with mix; other only with n_other
 *   > 0), B < 1, L < 1, n_src < 1, n_other < 0, n_src + n_other > 4 or an unknown perm_by; -1 when B * ceil(L / 4096) * J * 2 workgroups
 *   exceed 2^31 - 1; -2 for a workspace below rtfs_bss_eval_workspace_bytes (0 for arguments the call refuses).
 * rtfs_bss_eval_many_f32: the same for R recordings of different lengths on rtfs_score_many_plan's table, of which it uses columns 0
 *   and 10 only (RTFS_SCORE_COLS does not move); arguments, checks and codes as rtfs_bss_sdr_many_f32.  others: R * n_other device
 *   pointers, recording r's rows at [r n_other, (r + 1) n_other), each L_r samples; NULL with n_other = 0.  The workspace is its own,
 *   rtfs_bss_eval_many_workspace_bytes(plan, R, n_other, with_mix).  The kernels are those of rtfs_bss_eval_f32: row r is BIT-EQUAL to
 *   that call on recording r alone.  Not capturable (table upload).
 * rtfs_debug_bss_eval_f64: rtfs_bss_eval_f32 that also copies out, per row b, the folded r_ij at all lags (J, J, 1023 doubles: lag k at
 *   index 511 + k), D_all (n_src, J, 512: d_i of estimate q at [q][i]), p_all (n_src), p_j (n_src estimates x n_src sources) and the
 *   order the joint recursion reached (int32; 512 = the guard did not fire, also reported when the scalar solve stood in; 0 for an
 *   empty joint set); -4 for a NULL debug pointer. */
#define RTFS_BSS_PERM_BY_SDR 0
#define RTFS_BSS_PERM_BY_SIR 1
size_t rtfs_bss_eval_workspace_bytes(int B, int n_src, int n_other, int L, int with_mix);
int rtfs_bss_eval_f32(const float* clean, const float* est, const float* mix /* NULL: no baseline */, const float* other /* NULL: none */,
                      int B, int n_src, int n_other, int L, void* ws, size_t ws_bytes, float* sdr, float* sir, float* sar, float* sdr_i,
                      int* perm, int perm_by, void* stream);
size_t rtfs_bss_eval_many_workspace_bytes(const int* plan, int R, int n_other, int with_mix);
int rtfs_bss_eval_many_f32(const float* const* mixes /* NULL: no baseline */, const float* const* cleans, const float* const* ests,
                           const float* const* others /* NULL: none */, const int* table, const int* plan, int R, int n_src, int n_other,
                           int fs, void* ws, size_t ws_bytes, float* sdr, float* sir, float* sar, float* sdr_i, int* perm, int perm_by,
                           void* stream);
int rtfs_debug_bss_eval_f64(const float* clean, const float* est, const float* mix, const float* other, int B, int n_src, int n_other, int L,
                            void* ws, size_t ws_bytes, float* sdr, float* sir, float* sar, float* sdr_i, int* perm, int perm_by, double* r_out,
                            double* d_out, double* pall_out, double* pj_out, int* order_out, void* stream);

/* Long recordings in overlapping windows on the fused separator (AVNet.separate_long; no reference counterpart: infer_any_video.py:63-86
 * hands a whole track to one forward).  SPF = 640 samples per video frame (16 kHz, 25 fps).  A recording of L samples is cut into N
 * windows of `window` samples every `hop` samples; window n covers samples [n hop, n hop + window) (zeros past L) and video frames
 * [n hop / SPF, (n hop + window) / SPF) (an index past Tv - 1 reads frame Tv - 1).
 * rtfs_longform_plan (host only, no device call): checks L >= 1, Tv >= 1, window % SPF == 0, hop % SPF == 0, 0 < hop <= window (-4
 *   otherwise) and writes N = 1 if L <= window, else 1 + ceil((L - window) / hop).  N may be NULL.
 * rtfs_longform_frame_f32: rtfs_longform_frame_speakers_f32 (below) with K = 1: video (B,512,Tv) -> video_win (B*N, 512, window / SPF), row b*N + n.
 * rtfs_longform_overlap_add_f32 (one launch): y (B*N, n_src, window) -> out (B, n_src, L),
 *   out[b,s,t] = sum_n w[t - n hop] y[b*N + n, s, t - n hop] / sum_n w[t - n hop] over the windows that contain t, in ascending n, with
 *   w[i] = 1 if window == hop, else min(1, (i + 0.5) / V, (window - i - 0.5) / V), V = window - hop.  Gather form: every output element is
 *   written exactly once, no atomics, no scratch; deterministic.
 * Both take the caller's stream, allocate nothing and read nothing back; wav_win, video_win, y and out must be 16-byte aligned (-4). */
int rtfs_longform_plan(int L, int Tv, int window, int hop, int* N);
int rtfs_longform_frame_f32(const float* wav, const float* video, float* wav_win, float* video_win, int B, int L, int Tv, int window, int hop,
                            void* stream);
int rtfs_longform_overlap_add_f32(const float* y, float* out, int B, int n_src, int L, int window, int hop, void* stream);

/* Every face of a recording (AVNet.separate_long_speakers): K lip tracks per recording, 1 <= K <= RTFS_MAX_SPEAKERS (the limit of
 * rtfs_separator_speakers_f32), one audio track.  Plan, zeros past L and edge-frame replication are those described above.
 * rtfs_longform_frame_speakers_f32 (one launch): wav (B,L), video (B,K,512,Tv) -> wav_win (B*N, window), written ONCE per window, and
 *   video_win (B*N*K, 512, window / SPF), target row (b*N + n)*K + k: the (rows, K, 512, window / SPF) layout rtfs_separator_speakers_f32
 *   takes without a copy.  Its result y (B*N, K, window) is the (B*N, n_src, window) layout of rtfs_longform_overlap_add_f32 with
 *   n_src = K, which serves as it stands.  K outside [1, RTFS_MAX_SPEAKERS]: -4; B*N*K > 2^31 - 1 or a grid that does not fit: -1.
 * Takes the caller's stream, allocates nothing, reads nothing back; wav_win and video_win must be 16-byte aligned (-4). */
#define RTFS_MAX_SPEAKERS 16
int rtfs_longform_frame_speakers_f32(const float* wav, const float* video, float* wav_win, float* video_win, int B, int K, int L, int Tv,
                                     int window, int hop, void* stream);

/* Many recordings of different lengths in one pooled pass (AVNet.separate_many): R recordings, each planned on its own with
 * rtfs_longform_plan (N_r windows); the sum(N_r) windows are laid out in recording order, then window order, so `forward` runs on
 * chunks that straddle recordings.  Per recording, framing, weights and the division are exactly those of the three entries above.
 * rtfs_longform_many_plan (host only, the single place with the arithmetic): L, Tv (R each, host) -> total_windows = sum(N_r), out_floats =
 *   the size of ONE flat output and, when `table` is not NULL, the 5 * R int64 words [row0 | N | L | Tv | out_off] the kernels read FROM
 *   DEVICE MEMORY (the caller uploads them): row0[r] = sum of N before r, out_off[r] = where recording r's (n_src, L_r) block starts in the
 *   flat output, in floats.  Padding rule: every block is rounded up to a multiple of RTFS_LONGFORM_MANY_ALIGN = 32 floats, so out_off[r]
 *   = sum over q < r of 32 * ceil(n_src * L_q / 32), every block starts on a 128-byte line of a 128-byte aligned buffer, and out_floats
 *   (the sum over all r) is a whole number of lines; the floats between the end of a block and the next line are never written.
 *   Call it first with table NULL for the sizes.  R < 1, n_src < 1, an L_r or Tv_r outside [1, 2^31 - 1], a window / hop that
 *   rtfs_longform_plan refuses: -4; sum(N_r) > 2^31 - 1: -1.  total_windows and out_floats may be NULL.
 * rtfs_longform_frame_many_f32 (one launch for both gathers): wavs, videos = DEVICE arrays of R device pointers, recording r's (L_r) samples
 *   and its contiguous (512, Tv_r) video - separate allocations, no packing copy - -> wav_win (total_windows, window), video_win
 *   (total_windows, 512, window / SPF), row row0[r] + n.  A recording whose pointer is not 16-byte aligned is read with dword loads.
 * rtfs_longform_overlap_add_many_f32 (one launch): y (total_windows, n_src, window) -> out (out_floats), recording r at out + out_off[r]
 *   as (n_src, L_r).  Gather form: every element of every block is written exactly once, weights recomputed in registers, no atomics, no
 *   accumulator, no scratch; deterministic.
 * Both take the caller's stream, allocate nothing and read nothing back; wav_win, video_win, y and out must be 16-byte aligned and the
 * tables 8-byte aligned (-4).  The kernels trust the device tables: pass what rtfs_longform_many_plan wrote. */
#define RTFS_LONGFORM_MANY_ALIGN 32
int rtfs_longform_many_plan(const long long* L, const long long* Tv, int R, int window, int hop, int n_src, long long* table,
                            long long* total_windows, long long* out_floats);
int rtfs_longform_frame_many_f32(const float* const* wavs, const float* const* videos, const long long* table, float* wav_win, float* video_win,
                                 int R, int total_windows, int window, int hop, void* stream);
int rtfs_longform_overlap_add_many_f32(const float* y, float* out, const long long* table, int R, int total_windows, long long out_floats,
                                       int n_src, int window, int hop, void* stream);

/* The pooled pass with K_r lip tracks per recording (AVNet.separate_many_speakers), 1 <= K_r <= RTFS_MAX_SPEAKERS, n_src 1.
 * rtfs_longform_many_speakers_plan (host only): L, Tv, K (R each, host) -> total_windows = sum(N_r), total_targets = sum(N_r K_r),
 *   out_floats, and the 7 * R int64 words [row0 | N | L | Tv | out_off | K | trow0]: the five columns of rtfs_longform_many_plan with
 *   K_r in place of n_src (recording r's block is (K_r, L_r), same padding rule), then K_r and trow0[r] = sum of N_q K_q before r.  The K_r
 *   targets of window n of recording r are rows trow0[r] + n K_r + k: per recording the (windows, n_src := K_r, ..) layout of the
 *   overlap-add.  Refusals as rtfs_longform_many_plan, and -4 for a NULL K or a K_r outside 1 .. 16, -1 for total_targets > 2^31 - 1.
 * rtfs_longform_frame_many_speakers_f32 (one launch): videos[r] = recording r's contiguous (K_r, 512, Tv_r) -> wav_win (total_windows,
 *   window), each audio window written ONCE, and video_win (total_targets, 512, window / SPF).  max_K = the largest K_r (sizes the grid; -4
 *   outside 1 .. 16).
 * rtfs_longform_overlap_add_many_speakers_f32 (one launch): y (total_targets, window) -> out (out_floats), recording r at out + out_off[r]
 *   as (K_r, L_r).  Alignment rules and trust in the device table as above. */
int rtfs_longform_many_speakers_plan(const long long* L, const long long* Tv, const long long* K, int R, int window, int hop, long long* table,
                                     long long* total_windows, long long* total_targets, long long* out_floats);
int rtfs_longform_frame_many_speakers_f32(const float* const* wavs, const float* const* videos, const long long* table, float* wav_win,
                                          float* video_win, int R, int total_windows, int max_K, int window, int hop, void* stream);
int rtfs_longform_overlap_add_many_speakers_f32(const float* y, float* out, const long long* table, int R, int total_windows,
                                                long long out_floats, int window, int hop, void* stream);

/* Live streams chunk by chunk (AVNet.open_streams / StreamPool; DESIGN.md "Live streams"): the stateful form of the long-form plan.  Window
 * n of a stream is run as soon as a >= n hop + window samples AND f >= n hop / SPF + window / SPF frames have arrived; after window n the
 * samples [n hop, (n + 1) hop) are final.  The concatenated outputs of any chunking equal rtfs_longform_* on the whole recording.
 * A slot has one audio track and K lip tracks, 1 <= K <= RTFS_MAX_SPEAKERS, pushed together with one n_video; the entry points without
 * "speakers" in their name are K = 1 of those with it (below).
 * State (caller-allocated, 16-byte aligned, C = window + max_chunk): aring (slots, C), vring (slots, K, 512, C / SPF), acc (slots, n_src, C);
 * sample p lives in cell p % C, frame q of track k in column q % (C / SPF) of plane (slot, k).  n_src counts the rows of a window's
 * result y: the model's sources at K = 1, the K targets of rtfs_separator_speakers_f32 otherwise.  The caller keeps four counters per
 * slot [a samples received | f frames received | e windows emitted | o samples output], shared by the K tracks; nothing is ever read
 * back from the device.
 * rtfs_live_plan (host only, no device call, the single place with the arithmetic): for the R slots named in slot_ids, counters (R x 4,
 *   row-major) and the chunk sizes n_audio, n_video of this push (ignored when flush != 0) -> new_counters (R x 4), sizes[5] = [rows =
 *   ready windows of the tick | out_floats of ONE flat output | max_span = most samples one slot changes | largest n_audio | largest
 *   n_video] and the tick table, RTFS_LIVE_PLAN_WORDS = 13 int64 words per named slot, column-major:
 *   [slot | a | na | f | nf | e | cnt | row0 | o | end | out_off | apos | fpos]: cnt ready windows e .. e + cnt - 1 in rows row0 ..; the
 *   slot's (n_src, end - o) result starts out_off floats into the flat output, out_off a multiple of RTFS_LIVE_ALIGN = 32 floats (a
 *   128-byte line); apos = a % C and fpos = f % (C / SPF) are the ring positions the chunks are written at.  A push emits every ready
 *   window and makes [o, (e + cnt) hop) final.  A flush (L = a, Tv = f) emits the windows rtfs_longform_plan(L) still owes - zeros past
 *   L, a frame index past Tv - 1 reads frame Tv - 1 -, makes [o, L) final and returns zero counters.
 *   Refusals return -4, write nothing else, and name themselves in refused[2] = [index into slot_ids or -1 | RTFS_LIVE_* reason]:
 *   a window / hop rtfs_longform_plan refuses, max_chunk not a positive multiple of SPF, C > RTFS_LIVE_MAX_CAPACITY, R < 1,
 *   n_src < 1; a slot id outside [0, slots) or named twice; a chunk outside [0, max_chunk] samples / [0, max_chunk / SPF] frames; a push after which a + na - e hop > C or
 *   f + nf - e hop / SPF > C / SPF (it would overwrite a cell that window e still needs: one side ran too far ahead of the other); a
 *   flush of a slot with samples and no frame; counters this planner cannot have produced.  new_counters, table, sizes, refused may
 *   be NULL.
 * rtfs_live_ingest_frame_speakers_f32 (one launch): table = the plan's 13 R words followed by 1 + K columns [aptr | vptr_0 | .. |
 *   vptr_{K-1}], the DEVICE addresses of each slot's audio chunk (na floats, any 4-byte alignment) and of its K contiguous (512, nf)
 *   video chunks - separate allocations, read where they lie, nothing packed first -, uploaded by the caller.  Appends the chunks to the
 *   rings and writes the ready windows wav_win (rows, window), once per window, and video_win (rows * K, 512, window / SPF), target row
 *   r*K + k; a framed sample comes from the ring if it arrived in an earlier push and from the chunk otherwise.  No block reads a ring
 *   cell another block writes: the capacity rule makes the two sets disjoint in every plane (k_live.hip).  Sizes
 *   rtfs_live_speakers_sizes_ok refuses: -4.
 * rtfs_live_ingest_frame_f32: the same with K = 1, table columns [aptr | vptr].
 * rtfs_live_overlap_add_f32 (one launch): y (rows, n_src, window) -> final samples (acc + this tick's weighted windows in ascending n) /
 *   weight sum into out (out_floats), weights and order those of rtfs_longform_overlap_add_f32; samples a later window still reaches go
 *   back to acc.  Gather form: one thread per four samples of a source, every cell has one thread, no atomics; deterministic.
 * rtfs_live_reset_f32 (one launch): zeroes the state of the R slots in ids (DEVICE array; NULL = slots 0 .. R - 1): one lip track and
 *   n_src accumulator rows.  rtfs_live_reset_speakers_f32: K lip tracks and K accumulator rows.
 * rtfs_live_speakers_sizes_ok (host only): 1 when window / hop / max_chunk are what rtfs_live_plan takes, 1 <= K <= RTFS_MAX_SPEAKERS and
 *   K * (window + max_chunk) <= RTFS_LIVE_MAX_CAPACITY - the video share of the launch grids grows K-fold -, else 0.  A pool of sizes this
 *   accepts cannot fail at a launch.
 * The launches take the caller's stream, allocate nothing and read nothing back, and trust the device table: pass what rtfs_live_plan
 * wrote.  State, wav_win, video_win, y, out must be 16-byte aligned and the tables 8-byte aligned (-4).  RTFS_LIVE_MAX_CAPACITY bounds C
 * (2^24 samples, 17 minutes of history per slot) so that every launch grid of an accepted size fits; a grid that would not is -1. */
#define RTFS_LIVE_ALIGN 32
#define RTFS_LIVE_MAX_CAPACITY (1 << 24)
#define RTFS_LIVE_PLAN_WORDS 13
#define RTFS_LIVE_BAD_ARGUMENT 1
#define RTFS_LIVE_UNKNOWN_SLOT 2
#define RTFS_LIVE_REPEATED_SLOT 3
#define RTFS_LIVE_CHUNK_SIZE 4
#define RTFS_LIVE_AUDIO_CAPACITY 5
#define RTFS_LIVE_VIDEO_CAPACITY 6
#define RTFS_LIVE_NO_FRAMES 7
#define RTFS_LIVE_BAD_COUNTERS 8
int rtfs_live_plan(const long long* slot_ids, const long long* counters, const long long* n_audio, const long long* n_video, int R, int slots,
                   int flush, int window, int hop, int max_chunk, int n_src, long long* new_counters, long long* table, long long* sizes,
                   int* refused);
int rtfs_live_ingest_frame_f32(const long long* table, float* aring, float* vring, float* wav_win, float* video_win, int R, int rows,
                               int max_na, int max_nf, int window, int hop, int max_chunk, void* stream);
int rtfs_live_overlap_add_f32(const long long* table, const float* y, float* out, float* acc, int R, long long max_span, int n_src,
                              int window, int hop, int max_chunk, int flush, void* stream);
int rtfs_live_reset_f32(const long long* ids, float* aring, float* vring, float* acc, int R, int n_src, int window, int max_chunk,
                        void* stream);

/* K lip tracks per slot (AVNet.open_streams(speakers = K) / SpeakerStreamPool): described above */
int rtfs_live_speakers_sizes_ok(int window, int hop, int max_chunk, int K);
int rtfs_live_ingest_frame_speakers_f32(const long long* table, float* aring, float* vring, float* wav_win, float* video_win, int R, int rows,
                                        int K, int max_na, int max_nf, int window, int hop, int max_chunk, void* stream);
int rtfs_live_reset_speakers_f32(const long long* ids, float* aring, float* vring, float* acc, int R, int K, int window, int max_chunk,
                                 void* stream);

/* Faces that come and go (AVNet.open_streams(max_speakers = Kmax) / FaceStreamPool; DESIGN.md "Faces that come and go").  State is laid
 * out as for K = Kmax above (rtfs_live_speakers_sizes_ok(window, hop, max_chunk, Kmax) is the size rule, rtfs_live_reset_speakers_f32 with
 * K = Kmax the reset); a FACE is a plane 0 .. Kmax - 1 of its slot with a birth window b (host state, -1 = the plane is free): it takes
 * part in window n iff n >= b, and its output is the stream from sample b hop on.  The counters (a, f, e, o) stay the slot's.
 * rtfs_live_faces_plan (host only, the single place with the arithmetic): rtfs_live_plan plus births (R x Kmax, row-major, plane j of
 *   named slot r) -> new_counters (R x 4), row_counts[rows] = the targets of every ready window in row order (row_cap = its capacity),
 *   sizes[6] = [rows | targets | out_floats | max_span | largest n_audio | largest n_video] and the tick table,
 *   RTFS_LIVE_FACES_PLAN_WORDS(Kmax) = 15 + 2 Kmax int64 words per named slot, column-major: the 13 words of rtfs_live_plan (row0 counts
 *   window rows; out_off steps by the slot's (P, end - o) block) | P = faces present | trow0 = the slot's first target row | Kmax columns
 *   plane of present face i, ascending, -1 behind the P-th | Kmax columns birth of present face i.  Present are the active faces of a
 *   push; of a flush the faces with N > b and f > b hop / SPF (a window and a frame of their own).  Targets are window-major, within a
 *   window the present faces with b <= n in ascending plane; face i of the block owns samples [max(o, b hop), end), the cells before are
 *   never written.  Refusals as rtfs_live_plan's, and: Kmax outside [1, RTFS_MAX_SPEAKERS] or more ready windows than row_cap
 *   (RTFS_LIVE_BAD_ARGUMENT), a birth below -1 or above ceil(f SPF / hop) (RTFS_LIVE_BAD_COUNTERS), a push to a slot without a face
 *   (RTFS_LIVE_NO_FACES), a flush of a slot with samples in which no face takes part (RTFS_LIVE_NO_FRAMES).
 * rtfs_live_ingest_frame_faces_f32 (one launch): table = the plan's words followed by 1 + Kmax columns [aptr | vptr of present face 0 |
 *   ..], DEVICE addresses as for rtfs_live_ingest_frame_speakers_f32 (0 behind the P-th).  Appends the audio chunk once and each present
 *   face's chunk to its plane; writes wav_win (rows, window) and video_win (targets, 512, window / SPF) at the ragged target rows.
 * rtfs_live_overlap_add_faces_f32 (one launch): y (targets, window) -> the flat output; rtfs_live_overlap_add_f32 with the sums of face i
 *   running over windows n >= b only; with every plane present and all births 0 it is that kernel operation for operation.
 * Kmax outside [1, RTFS_MAX_SPEAKERS] or sizes rtfs_live_speakers_sizes_ok refuses: -4; an empty tick: RTFS_OK without a launch. */
#define RTFS_LIVE_FACES_PLAN_WORDS(Kmax) (15 + 2 * (Kmax))
#define RTFS_LIVE_NO_FACES 9
int rtfs_live_faces_plan(const long long* slot_ids, const long long* counters, const long long* n_audio, const long long* n_video, int R,
                         int slots, int flush, int window, int hop, int max_chunk, int Kmax, const long long* births, int row_cap,
                         long long* new_counters, long long* table, long long* row_counts, long long* sizes, int* refused);
int rtfs_live_ingest_frame_faces_f32(const long long* table, float* aring, float* vring, float* wav_win, float* video_win, int R, int rows,
                                     int Kmax, int max_na, int max_nf, int window, int hop, int max_chunk, void* stream);
int rtfs_live_overlap_add_faces_f32(const long long* table, const float* y, float* out, float* acc, int R, long long max_span, int Kmax,
                                    int window, int hop, int max_chunk, int flush, void* stream);

/* Video front-end (the step before the path): FRCNNVideoModel.forward with backbone_type "resnet",
 * relu_type "prelu", eval mode (src/models/videomodels/frcnn_videomodel.py:61-72, resnet.py:23-118).
 * lips (B, 1, T, 88, 88) grey-scale mouth crops -> out (B, 512, T), the lip embedding AVNet.forward takes.
 * pack: rtfs-net_amd/packing.py:pack_video (eval BatchNorm folded into f16x3 weight images + bias, PReLU slopes). */
size_t rtfs_video_pack_floats(void);
size_t rtfs_video_workspace_bytes(int B, int T);
int rtfs_video_frontend_f32(const float* lips, const float* pack, float* out, int B, int T, void* ws, size_t ws_bytes, void* stream);

/* Live streams from camera frames (FRCNNVideoModel.open_streams / LipStreamPool; DESIGN.md "Live streams from camera frames"): the lip
 * embedding chunk by chunk.  Only the stem is temporal (kernel 5, padding 2), so embedding q needs prepared lips frames q - 2 .. q + 2 and
 * nothing else.  The caller keeps three integers per slot [g frames received | v embeddings emitted | side]; a push of m frames gives
 * g' = g + m, v' = max(v, g' - 2) and emits v .. v' - 1; a flush emits v .. g - 1 with zero planes for indices >= g and returns zero
 * counters.  Frames with index < 0 are zero planes as well: the stem's own padding, 0.0f in the PREPARED domain.  The concatenated
 * outputs of any chunking equal rtfs_video_frontend_f32 on the whole track.
 * State (caller-allocated, 16-byte aligned): hist (slots, 2, 4, 88, 88), two history buffers per slot; buffer `side` holds the prepared
 *   frames max(0, g - 4) .. g - 1, frame p in plane p % 4.  A launch reads buffer `side` and writes buffer 1 - side; a push with m > 0
 *   flips the side, so no block reads a cell another block of the same launch writes.  Which planes hold a frame follows from g.
 * rtfs_live_video_plan (host only, no device call, the single place with the arithmetic): for the R slots named in slot_ids, counters
 *   (R x 3, row-major) and n_frames (R; ignored when flush != 0) -> new_counters (R x 3), sizes[3] = [rows = sum of k | out_floats of ONE
 *   flat output | largest m] and the tick table, RTFS_LIVE_VIDEO_PLAN_WORDS = 8 int64 words per named slot, column-major:
 *   [slot | g | m | v | k | row0 | out_off | side]: the slot emits k embeddings v .. v + k - 1 in rows row0 .. of the tick's output frames
 *   (rows lie in the order the slots are named, then by frame index); its contiguous (512, k) block starts out_off floats into the flat
 *   output, out_off a multiple of RTFS_LIVE_ALIGN floats; side is the buffer that is read.
 *   Refusals return -4, write nothing else, and name themselves in refused[2] = [index into slot_ids or -1 | RTFS_LIVE_* reason]:
 *   R < 1, slots < 1, max_frames < 1 or a missing array (BAD_ARGUMENT); a slot id outside [0, slots) or named twice; m outside
 *   [0, max_frames] (CHUNK_SIZE); counters this planner cannot have produced (negative, v > g, v < max(0, g - 2), side not 0 / 1:
 *   BAD_COUNTERS).  new_counters, table, sizes, refused may be NULL.
 * rtfs_live_video_ingest_u8 / _f32 (one launch each): table = the plan's 8 R words followed by one more column, the DEVICE address of each
 *   slot's chunk - separate allocations, read where they lie: uint8 (m, H, W) at any byte alignment, or float32 prepared lips
 *   (m, 88, 88) at 4-byte alignment.  Writes the tick's stem input windows (rows, 5, 94, 94): for output frame n its own zero-bordered
 *   5-frame window, the stem's layout at T = 1, and leaves buffer 1 - side of every slot with m > 0 holding frames g' - 4 .. g' - 1.
 *   uint8 pixels go through f(v) = (float)(((double(v) - 0.0) / 255.0 - mean) / std) at crop offset (dy, dx), exactly as
 *   rtfs_lips_prepare_u8 without flip.  flush != 0: frames >= g are zero planes and no history is written.
 * rtfs_video_frontend_windows_f32: stem, max-pool, trunk and average pool of rtfs_video_frontend_f32 on rows [row_begin, row_begin + n)
 *   of a window volume (windows points at row 0), then frame row's 512 values go to column row - row0 of its slot's (512, k) block of out
 *   through the table.  ws: rtfs_video_windows_workspace_bytes(n).
 * rtfs_live_video_reset (one launch): zeroes both history buffers of the R slots in ids (DEVICE array; NULL = slots 0 .. R - 1).  No
 *   kernel depends on those contents.
 * The launches take the caller's stream, allocate nothing, read nothing back, use no atomics and trust the device table: pass what
 * rtfs_live_video_plan wrote.  hist, windows, out 16-byte aligned, tables 8-byte aligned (-4); a grid that would not fit: -1. */
#define RTFS_LIVE_VIDEO_PLAN_WORDS 8
int rtfs_live_video_plan(const long long* slot_ids, const long long* counters, const long long* n_frames, int R, int slots, int flush,
                         int max_frames, long long* new_counters, long long* table, long long* sizes, int* refused);
int rtfs_live_video_ingest_u8(const long long* table, float* hist, float* windows, int R, int rows, int max_m, int flush, int H, int W,
                              int dy, int dx, double mean, double std, void* stream);
int rtfs_live_video_ingest_f32(const long long* table, float* hist, float* windows, int R, int rows, int max_m, int flush, void* stream);
size_t rtfs_video_windows_workspace_bytes(int rows);
int rtfs_video_frontend_windows_f32(const float* windows, const float* pack, const long long* table, float* out, int R, int row_begin,
                                    int n, void* ws, size_t ws_bytes, void* stream);
int rtfs_live_video_reset(const long long* ids, float* hist, int R, void* stream);

/* Live streams and recordings at the camera's own frame rate (DESIGN.md "Live streams at the camera's frame rate"; csrc/frame_rate.h).
 * The rule: camera frame i of a stream at a / b fps (reduced) has the 25 fps tick r(i) = floor(i 25 b / a + 1/2); model frame p shows
 * c(p) = max{i : r(i) <= p} = ceil(a (2p + 1) / (50 b)) - 1, and n camera frames give the model frames p with c(p) < n,
 * P(n) = floor((50 b n + a) / (2 a)) of them.  No frame is blended; at 25 / 1, c(p) = p and P(n) = n.
 * rtfs_frame_rate_map (host only): *n_out = P(n_in) and, when src is not NULL, src[p] = c(p) for p < P(n_in).  -4 for a rate outside
 *   [1, 240] fps, a reduced numerator or denominator above 2^20, n_in outside [0, 2^36] or n_out NULL; nothing is written then.
 * rtfs_live_video_rate_plan (host only): rtfs_live_video_plan with n_frames and max_frames in CAMERA frames.  counters (R x 4):
 *   [g | v | side | n camera frames received], g == P(n); new_counters likewise.  g, m, v, k, row0, out_off, side keep their meaning in
 *   model frames, m = P(n + n_frames) - g (it may be 0: then g, v and side stay and only n advances).  The table has
 *   RTFS_LIVE_VIDEO_RATE_PLAN_WORDS = 9 columns, the eight of rtfs_live_video_plan and n0 = n; sizes[4] = [rows | out_floats | largest
 *   chunk in camera frames | largest m in model frames], the last one sizes the window volume (it exceeds the chunk below 25 fps).  A
 *   flush emits v .. P(n) - 1.  Refusals as rtfs_live_video_plan, and RTFS_LIVE_BAD_RATE (refused[0] = -1) for a rate
 *   rtfs_frame_rate_map refuses; g != P(n) or n + n_frames > 2^36: BAD_COUNTERS.  At 25 / 1 the first eight columns, the first three
 *   counters and sizes[0..2] are those of rtfs_live_video_plan.
 * rtfs_live_video_ingest_rate_u8 / _f32 (one launch each): rtfs_live_video_ingest_* on the 9 R words of the rate plan followed by the
 *   column of chunk addresses; chunks hold CAMERA frames and model frame p >= g is read from chunk index c(p) - n0.  Camera frames that
 *   no model frame shows are not read, nor anything behind the chunk; max_m is sizes[3]; a slot with m == 0 keeps its history untouched.
 * rtfs_lips_prepare_rate_u8: rtfs_lips_prepare_u8 on roi (N,Tv_in,H,W) at rate_num / rate_den fps -> out (N,1,P(Tv_in),88,88),
 *   out[n,0,p] = the prepared roi[n,c(p)].  P(Tv_in) == 0 (a single frame above 50 fps): -1. */
#define RTFS_LIVE_VIDEO_RATE_PLAN_WORDS 9
#define RTFS_LIVE_BAD_RATE 10
int rtfs_frame_rate_map(int rate_num, int rate_den, long long n_in, long long* n_out, long long* src);
int rtfs_live_video_rate_plan(const long long* slot_ids, const long long* counters, const long long* n_frames, int R, int slots, int flush,
                              int max_frames, int rate_num, int rate_den, long long* new_counters, long long* table, long long* sizes,
                              int* refused);
int rtfs_live_video_ingest_rate_u8(const long long* table, float* hist, float* windows, int R, int rows, int max_m, int flush, int H, int W,
                                   int dy, int dx, double mean, double std, int rate_num, int rate_den, void* stream);
int rtfs_live_video_ingest_rate_f32(const long long* table, float* hist, float* windows, int R, int rows, int max_m, int flush, int rate_num,
                                    int rate_den, void* stream);
int rtfs_lips_prepare_rate_u8(const unsigned char* roi, const int* table, float* out, int N, int Tv_in, int H, int W, double mean,
                              double std, int rate_num, int rate_den, void* stream);

/* Live streams with per-frame timestamps (DESIGN.md "Live streams with per-frame timestamps"; csrc/frame_rate.h): cameras that drop
 * frames or change rate.  Camera frame i carries an integer stamp tau_i in a timebase of tb ticks per second, 1 <= tb <= 2^30,
 * 0 <= tau < 2^40, strictly increasing within a stream.  Its 25 fps tick is r(i) = G(tau_i), G(W) = floor((50 W + tb) / (2 tb)); model
 * frame p shows c(p) = max(0, max{i : 50 tau_i < tb (2p + 1)}), the last camera frame whose tick is at or before p and the first camera
 * frame before that.  Once every frame stamped below a watermark W is in, exactly the model frames p < G(W) are final.  With
 * tau_i = i tb b / a this is the rule of rtfs_frame_rate_map.
 * rtfs_timestamp_map (host only): the whole-track rule.  n stamps and the largest `until` of the stream (0: none) -> *n_out =
 *   g_end = max(G(max(tau_{n-1}, until)), r(n - 1) + 1) (0 for n == 0) and, when src is not NULL, src[p] = c(p) for p < g_end.  -4 for a
 *   timebase, a stamp or an until outside the bounds, stamps that do not increase, n or g_end above 2^36, or n_out NULL.
 * rtfs_live_video_stamp_plan (host only): rtfs_live_video_rate_plan with stamps.  counters (R x 7): [g | v | side | n | last stamp |
 *   watermark W | hside], g == G(W) once n > 0 (g == 0 before).  n_frames (R): camera frames per chunk, at most max_frames; stamps: the
 *   stamps of all chunks one behind the other in the order the slots are named; until (R, or NULL for none): the caller's promise that
 *   every later frame of the slot is stamped >= until[r] (0: no promise).  A push gives W' = max(W, the chunk's last stamp, until),
 *   g' = max(g, G(W')) - but g' = 0 while no camera frame has ever arrived - v' = max(v, g' - 2), side flips iff m = g' - g > 0, hside
 *   flips iff n_frames > 0.  A flush (n_frames and stamps ignored) ends the stream at g_end = max(g, G(max(W, until)), r(n - 1) + 1), so
 *   the last camera frame is shown at least by its own tick: it finalises m = g_end - g frames, emits v .. g_end - 1 and returns zero
 *   counters.  The table has RTFS_LIVE_VIDEO_STAMP_PLAN_WORDS = 12 columns, the nine of the rate plan | hside | soff | m_cam = n_frames;
 *   sources (at most R max_frames words) holds at soff + (p - g), for each newly final model frame p of the slot, the chunk-local index
 *   of c(p) or -1 for camera frame n - 1, the held frame; sizes[5] = [rows | out_floats | largest chunk | largest m | words of sources].
 *   Refusals as rtfs_live_video_rate_plan, and: a timebase outside [1, 2^30] (RTFS_LIVE_BAD_TIMEBASE, refused[0] = -1); a stamp outside
 *   [0, 2^40) or an until outside [0, 2^40] (RTFS_LIVE_BAD_STAMP); a stamp below W, or not above its predecessor
 *   (RTFS_LIVE_STAMP_ORDER); m > max_frames (RTFS_LIVE_TOO_MANY_FINAL: advance until in smaller steps); counters this planner cannot have
 *   produced (BAD_COUNTERS).
 * rtfs_live_video_ingest_stamp_u8 / _f32 (one launch each): table = the plan's 12 R words, the column of chunk addresses and the
 *   sizes[4] source words, 13 R + sizes[4] words in all.  State: hist as above and held (slots, 2, 88, 88), 16-byte aligned: buffer hside
 *   holds the prepared last camera frame received.  A model frame p >= g is read from the chunk at its source index or, for -1, from
 *   held[slot, hside]; one more block per slot with m_cam > 0 writes the chunk's last frame, prepared, into held[slot, 1 - hside].  All
 *   reads of held go to hside and the one write to 1 - hside, so no block reads a cell another block of the launch writes.  Camera
 *   frames that no model frame shows are not read, except the chunk's last.  max_m = sizes[3], max_cam = sizes[2]; flush != 0: max_cam
 *   must be 0, frames in [g, g + m) come from held, frames behind are zero planes, and neither history nor held is written.  A
 *   timebase outside [1, 2^30], a NULL or misaligned pointer: -4 before any launch.
 * rtfs_live_video_stamp_reset (two launches): rtfs_live_video_reset, and zeroes both held planes of the same slots.  No kernel depends
 *   on those contents: held[hside] is read only after a push wrote it. */
#define RTFS_LIVE_VIDEO_STAMP_PLAN_WORDS 12
#define RTFS_LIVE_BAD_TIMEBASE 11
#define RTFS_LIVE_BAD_STAMP 12
#define RTFS_LIVE_STAMP_ORDER 13
#define RTFS_LIVE_TOO_MANY_FINAL 14
int rtfs_timestamp_map(const long long* stamps, long long n, long long timebase, long long until, long long* n_out, long long* src);
int rtfs_live_video_stamp_plan(const long long* slot_ids, const long long* counters, const long long* n_frames, const long long* stamps,
                               const long long* until, int R, int slots, int flush, int max_frames, long long timebase,
                               long long* new_counters, long long* table, long long* sources, long long* sizes, int* refused);
int rtfs_live_video_ingest_stamp_u8(const long long* table, float* hist, float* held, float* windows, int R, int rows, int max_m, int max_cam,
                                    int flush, int H, int W, int dy, int dx, double mean, double std, long long timebase, void* stream);
int rtfs_live_video_ingest_stamp_f32(const long long* table, float* hist, float* held, float* windows, int R, int rows, int max_m, int max_cam,
                                     int flush, long long timebase, void* stream);
int rtfs_live_video_stamp_reset(const long long* ids, float* hist, float* held, int R, void* stream);

/* Optimizer step on the device (rtfs-net_amd/optimizers.py AdamW; the reference builds torch.optim.AdamW through
 * src/system/optimizers.py:58-108 and Lightning clips at gradient_clip_val 5.0, train.py:142): gather of the per-tensor gradients into
 * one flat buffer, global-norm clip and AdamW in a number of launches that does not depend on the number of tensors.
 * Layout: tensor t owns floats [flat_off[t], flat_off[t] + numel[t]) of every flat buffer (flat_g, exp_avg, exp_avg_sq), flat_off
 * rounded up to 4 floats, and is cut into chunks of RTFS_OPTIM_CHUNK floats, one workgroup and one float64 partial each.
 * rtfs_optim_plan (host only): numel (n_tensors, host) -> flat_floats, n_chunks and, when `table` is not NULL, the
 *   2 * n_tensors + 2 * n_chunks int64 words [flat_off | numel | chunk_tensor | chunk_off] the kernels read FROM DEVICE MEMORY (the caller
 *   uploads them once).  n_tensors > RTFS_OPTIM_MAX_TENSORS -> -4 (pointer tables travel in the kernel arguments).
 * rtfs_optim_gather_f32 (one launch): grads = HOST array of n_tensors device pointers, copied into the launch (they change every
 *   step).  A NULL gradient is skipped (its slice of flat_g is left as it is and its partials are 0) or, with zero_missing, written as
 *   zeros.  partials (n_chunks float64, may be NULL) = sum of squares per chunk.
 * rtfs_optim_sumsq_f32 (one launch): the partials of flat_g alone, over every tensor (after a collective on flat_g).
 * rtfs_optim_adamw_f32 (one launch): total = sqrt(sum partials) * grad_scale -> *total_norm (may be NULL);
 *   coef = max_norm > 0 ? min(1, max_norm / (total + 1e-6)) : 1; per element of every tensor whose hyper_index is not 255:
 *   g = (grad_scale * coef) * flat_g; p *= decay; m += omb1 * (g - m); v = b2 * v + omb2 * g * g;
 *   p -= step_size * m / (sqrt(v) / bc2_sqrt + eps).  params / hyper_index (n_tensors) and hyper (n_hyper <= RTFS_OPTIM_MAX_HYPER sets of
 *   8 floats: decay = 1 - lr * wd, omb1 = 1 - beta1, b2, omb2 = 1 - beta2, step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t),
 *   eps, 0) are HOST arrays copied into the launch.  Parameters are written where they live; 16-byte accesses where a pointer allows.
 * No atomics: the same inputs give the same bits.  Caller's stream, no allocation, no synchronisation; flat buffers 16-byte aligned,
 * partials and table 8-byte aligned (-4 otherwise, before any launch).  The bias corrections are host values, so a captured graph would
 * replay one step count: not graph-replayable. */
#define RTFS_OPTIM_CHUNK 4096
#define RTFS_OPTIM_MAX_TENSORS 320
#define RTFS_OPTIM_MAX_HYPER 16
int rtfs_optim_plan(const long long* numel, int n_tensors, long long* table, long long* flat_floats, int* n_chunks);
int rtfs_optim_gather_f32(const float* const* grads, const long long* table, int n_tensors, int n_chunks, float* flat_g, double* partials,
                          int zero_missing, void* stream);
int rtfs_optim_sumsq_f32(const long long* table, int n_tensors, int n_chunks, const float* flat_g, double* partials, void* stream);
int rtfs_optim_adamw_f32(float* const* params, const unsigned char* hyper_index, const float* hyper, int n_hyper, const long long* table,
                         int n_tensors, int n_chunks, const float* flat_g, float* exp_avg, float* exp_avg_sq, const double* partials,
                         float max_norm, float grad_scale, float* total_norm, void* stream);

/* Preparing raw recordings (rtfs-net_amd/datas.py; csrc/k_prep.hip): what the reference does on the host in front of the model inputs.
 * All entries take the caller's stream, allocate nothing, read nothing back and use no atomics (deterministic; graph-capturable at fixed
 * shapes); bad arguments return the error codes above before anything is launched.
 * rtfs_lips_prepare_u8 (src/datas/transform.py:151-167 collapsed): roi uint8 (N,Tv,H,W) on the device, H, W >= 88 -> out float32
 *   (N,1,Tv,88,88), 16-byte aligned: out[n,0,t,y,x] = f(roi[n,t,dy+y, dx + (flip ? 87-x : x)]),
 *   f(v) = (float)(((double(v) - 0.0) / 255.0 - mean) / std).  table = HOST array (N,3) of dy, dx, flip per track, checked here (an
 *   offset that leaves the ROI, a flip other than 0 / 1: -4) and copied into the launch: one launch per
 *   RTFS_LIPS_MAX_TRACKS_PER_LAUNCH tracks.
 * rtfs_wav_normalize_f32 (avspeech_dataset.py:18-22, 145-148): mix (B,L), src (B,K,L) or NULL with K = 0 -> the same shapes;
 *   mix_out = (mix - mean(mix)) / (s + eps), src_out[b,k] = (src[b,k] - mean(src[b,k])) / (s[b] + eps) with s[b] the unbiased standard
 *   deviation of mixture row b, or std_in[b] (B floats on the device) when std_in is not NULL.  Means and deviations are accumulated in
 *   float64; L = 1 gives NaN as torch.std does.  Two launches; ws >= rtfs_wav_normalize_workspace_bytes, 8-byte aligned.
 * rtfs_resample_plan (host only): o, n = orig / gcd, new / gcd (either > RTFS_RESAMPLE_MAX_RATIO: -4), base = min(o, n) * 0.99,
 *   width = ceil(6 o / base), taps = 2 width + o and, when bank is not NULL, the n * taps float32 kernel bank of torchaudio's Resample
 *   defaults computed in float64: t = clip((-p / n + (k - width) / o) * base, -6, 6), bank[p,k] = sinc(pi t) cos^2(pi t / 12) base / o.
 * rtfs_resample_out_len (host only): ceil(n L / o), or -1 for a ratio the plan refuses.
 * rtfs_resample_f32 (one launch): x (B,L), bank (n,taps) on the device -> y (B, ceil(n L / o)),
 *   y[j n + p] = sum_k bank[p,k] xpad[j o + k], xpad = x with width zeros in front and width + o behind (predicates, no padded copy).
 *   Taps outside [floor(o p / n), floor(o p / n) + 2 width] are exact zeros of the bank (the plan verifies it) and are skipped. */
#define RTFS_LIPS_MAX_TRACKS_PER_LAUNCH 512
#define RTFS_RESAMPLE_MAX_RATIO 640
int rtfs_lips_prepare_u8(const unsigned char* roi, const int* table, float* out, int N, int Tv, int H, int W, double mean, double std,
                         void* stream);
size_t rtfs_wav_normalize_workspace_bytes(int B, int K, int L);
int rtfs_wav_normalize_f32(const float* mix, const float* src, const float* std_in, float* mix_out, float* src_out, int B, int K, int L,
                           double eps, void* ws, size_t ws_bytes, void* stream);
int rtfs_resample_plan(int orig_freq, int new_freq, int* o, int* n, int* width, int* taps, float* bank);
long long rtfs_resample_out_len(int orig_freq, int new_freq, long long L);
int rtfs_resample_f32(const float* x, const float* bank, float* y, int B, int L, int orig_freq, int new_freq, void* stream);

/* Live streams at the microphone's own rate (datas.open_resample_streams / ResampleStreamPool; DESIGN.md "Live streams at the
 * microphone's rate"; csrc/k_live_resample.hip): rtfs_resample_f32 chunk by chunk.  In the notation of rtfs_resample_plan (o, n, width,
 * span = 2 width + 1, c(p) = floor(o p / n)) output q = j n + p reads the inputs j o + c(p) - width .. last(q) = j o + c(p) + width, and
 * G(A) = #{q : last(q) < A} = ceil(n max(0, A - width) / o).  The caller keeps three integers per slot [a input samples received |
 * g output samples emitted | side]; a push of m samples gives a' = a + m, g' = G(a') and emits g .. g' - 1; a flush emits
 * g .. ceil(n a / o) - 1 (rtfs_resample_out_len of the samples received) with exact zeros for inputs >= a and returns zero counters.
 * Inputs with index < 0 are exact zeros as well.  Every output is formed by the fmaf chain of rtfs_resample_f32 in the same order on the
 * same values, so the concatenated outputs of any chunking are BIT-equal to rtfs_resample_f32 on the whole recording; an output leaves
 * width / orig_freq seconds after the last input it reads arrived.
 * State (caller-allocated, 16-byte aligned): hist (slots, 2, 2 width), two history buffers per slot; buffer `side` holds the inputs
 *   a - 2 width .. a - 1, input x in cell x - (a - 2 width).  A launch reads buffer `side` and writes buffer 1 - side; a push with m > 0
 *   flips the side, so no block reads a cell another block of the same launch writes.  Which cells hold a sample follows from a.
 * rtfs_live_resample_plan (host only, no device call, the single place with the arithmetic): for the R slots named in slot_ids, counters
 *   (R x 3, row-major) and n_samples (R; ignored when flush != 0) -> new_counters (R x 3), sizes[3] = [out_floats of ONE flat output |
 *   largest m | largest k] and the tick table, RTFS_LIVE_RESAMPLE_PLAN_WORDS = 7 int64 words per named slot, column-major:
 *   [slot | a | m | g | k | out_off | side]: the slot emits the k outputs g .. g + k - 1; its block starts out_off floats into the flat
 *   output, out_off a multiple of RTFS_LIVE_ALIGN floats; side is the buffer that is read.
 *   Refusals return -4, write nothing else, and name themselves in refused[2] = [index into slot_ids or -1 | RTFS_LIVE_* reason]:
 *   R < 1, slots < 1, max_chunk_in < 1, a missing array or a ratio rtfs_resample_plan refuses (BAD_ARGUMENT); a slot id outside
 *   [0, slots) or named twice; m outside [0, max_chunk_in] (CHUNK_SIZE); counters this planner cannot have produced (negative,
 *   g != G(a), side not 0 / 1: BAD_COUNTERS).  new_counters, table, sizes, refused may be NULL.
 * rtfs_live_resample_f32 / _i16 (one launch each): table = the plan's 7 R words followed by one more column, the DEVICE address of each
 *   slot's chunk - separate allocations, read where they lie: float32 at any 4-byte alignment, or int16 PCM at any 2-byte alignment,
 *   which enters as (float)s / 32768 (exact).  bank = the (n, taps) bank of rtfs_resample_plan on the device.  Writes each slot's k
 *   outputs and leaves buffer 1 - side of every slot with m > 0 holding the inputs a' - 2 width .. a' - 1.  max_m, max_k = sizes[1],
 *   sizes[2]; flush != 0 requires max_m == 0 and writes no history.
 * rtfs_live_resample_reset (one launch): zeroes both history buffers of the R slots in ids (DEVICE array; NULL = slots 0 .. R - 1).  No
 *   kernel depends on those contents.
 * The launches take the caller's stream, allocate nothing, read nothing back, use no atomics and trust the device table: pass what
 * rtfs_live_resample_plan wrote.  hist, out 16-byte aligned, tables 8-byte aligned (-4); a grid that would not fit: -1. */
#define RTFS_LIVE_RESAMPLE_PLAN_WORDS 7
int rtfs_live_resample_plan(const long long* slot_ids, const long long* counters, const long long* n_samples, int R, int slots, int flush,
                            int orig_freq, int new_freq, long long max_chunk_in, long long* new_counters, long long* table, long long* sizes,
                            int* refused);
int rtfs_live_resample_f32(const long long* table, const float* bank, float* hist, float* out, int R, long long max_m, long long max_k,
                           int flush, int orig_freq, int new_freq, void* stream);
int rtfs_live_resample_i16(const long long* table, const float* bank, float* hist, float* out, int R, long long max_m, long long max_k,
                           int flush, int orig_freq, int new_freq, void* stream);
int rtfs_live_resample_reset(const long long* ids, float* hist, int R, int orig_freq, int new_freq, void* stream);

/* Mouth ROIs from whole camera frames (datas.mouth_affine / mouth_rois; DESIGN.md "Mouth ROIs from camera frames"; csrc/k_mouth.hip):
 * the reference's step between a face tracker's landmarks and the uint8 mouth ROIs (RTFSNet_file.py:20-73, 111-118) as ONE affine map
 * per (frame, face) and ONE bilinear sampling of the source frame.  All arithmetic is IEEE float64 in a fixed order without fused
 * multiply-add; tests/mouth_oracle.py restates it and both entries are bit-equal to it.
 * rtfs_mouth_affine (host only, no device call): eyes (n,2,2) = the eye corner on the left in the image, then the right one, lips
 *   (n,4,2) = the four points whose bounding box is the mouth, float64 (x, y) in source pixels -> A (n,2,3), the map from ROI pixel
 *   (j, i) to the source point sx = A00 j + A01 i + A02, sy = A10 j + A11 i + A12.  With d = right - left, dist = |d|, s = 76.8 / dist,
 *   a = s dx / dist, b = s dy / dist, c the eyes' midpoint and t = (128, 89.6), a point p lies at q = [[a, b], [-b, a]] (p - c) + t in the
 *   reference's 256 x 256 aligned face; the lip box there is x0 = min qx, w = max qx - x0 + 1 (likewise y0, h); ROI pixel (j, i) shows
 *   the aligned point x0 + (j - (out_w - crop_w) / 2 + 0.5) w / crop_w - 0.5 (likewise y): the box fills the central crop_h x crop_w of
 *   the ROI; and p = c + R^T (q - t) / (a a + b b).  -4 for a missing array, crop outside [1, out], out > 4096 (refused[0] = -1) and for
 *   a set with a non-finite landmark, dist == 0 or a non-finite matrix entry (refused[0] = its index).  refused may be NULL.
 * rtfs_mouth_rois_u8 (one launch): J jobs of RTFS_MOUTH_JOB_WORDS = 12 int64 words, row-major: [source plane address | destination
 *   address | H | W | row pitch in bytes | pixel stride in bytes + 65536 * order (0 grey, 1 BGR, 2 RGB) | the six doubles of A].  jobs is
 *   the table on the DEVICE, host_jobs the same words on the host or NULL; with host_jobs every job is checked before the launch (-4: a
 *   null address, H or W outside [1, 32767], pitch outside [0, 2^31), an unknown order, a colour pixel stride below 3, a non-finite
 *   matrix entry).  Jobs may differ in everything and may share a source.  Every job writes out_h * out_w contiguous bytes at any
 *   alignment: per pixel x0 = floor(sx), fx = sx - x0 (likewise y; sx, sy clamped to [-2, W + 1], [-2, H + 1] in double first), taps
 *   (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1), a tap outside the frame 0, a colour tap (1868 B + 9617 G + 4899 R + 8192) >> 14 first,
 *   v = (1-fy) ((1-fx) p00 + fx p01) + fy ((1-fx) p10 + fx p11), out = rint(v) clamped to 0 .. 255.  Takes the caller's stream,
 *   allocates nothing, reads nothing back, no atomics.  out_h, out_w outside [1, 4096] or a grid that would not fit: -1. */
#define RTFS_MOUTH_JOB_WORDS 12
int rtfs_mouth_affine(const double* eyes, const double* lips, long long n, int out_h, int out_w, int crop_h, int crop_w, double* A,
                      long long* refused);
int rtfs_mouth_rois_u8(const long long* jobs, const long long* host_jobs, int J, int out_h, int out_w, void* stream);

/* Training mixtures on the device (datas.mix_batch, System.online_mixing_collate / System.mix_batch; DESIGN.md "Training mixtures";
 * csrc/k_mix.hip): the reference's online mixing (src/system/core.py:183-202) and the target-speaker form (a target plus interferers at
 * a drawn SNR, each at a drawn crop of its utterance) as a host recipe, one table upload and TWO launches.
 * A recipe has B rows of J = RTFS_MIX_MAX_SOURCES slots.  Slot (b, j) names a segment of L samples of a source allocation, a factor a
 * (float64) and optionally a reference segment; a slot may be empty.  Sources are separate device allocations read where they lie:
 * float32 at any 4-byte alignment or int16 PCM at any 2-byte alignment, which enters as (float)s / 32768; both may appear in one call
 * and an allocation or segment may appear in any number of slots and rows.  With x_j the slot's segment and E(x) = sum x^2 (raw, no
 * mean removal, as the reference), everything in float64:
 *   g_j = a_j without a reference, a_j sqrt(E(ref_j) / E(x_j)) with one (no eps: a silent segment gives inf / NaN as core.py:197),
 *   0 for an empty slot, which reads nothing;  m[t] = sum_j g_j x_j[t] over the non-empty slots in the order j = 0, 1, ..., multiply
 *   then add, never fused;  without normalisation mixture[b,t] = (float)m[t], sources[b,j,t] = (float)(g_j x_j[t]) for j < n_out;
 *   with it (avspeech_dataset.py:145-148, the rule of rtfs_wav_normalize_f32) s = the unbiased standard deviation of m,
 *   inv = 1 / (s + eps), mixture = (float)((m - mean(m)) inv), sources[j] = (float)((g_j x_j - g_j (sum x_j / L)) inv); L = 1 gives NaN.
 *   A source row of an empty slot is (float)0, or (float)((0 - 0) inv).
 *   stats (B, J + 2) float64 on the device = [g_0 .. g_{J-1} | mean(m) | inv]; always written, never read back by the library.
 * rtfs_mix_plan (host only, no device call, the single place with the arithmetic): slots = B * J records of RTFS_MIX_RECIPE_WORDS = 8
 *   int64 words, row-major [source address (0: an empty slot) | source length in samples | dtype RTFS_MIX_F32 / RTFS_MIX_I16 | start
 *   sample | reference source address (0: none) | its length | its dtype | its start sample], a = B * J factors -> *ws_bytes and, when
 *   table is not NULL, the B * J * RTFS_MIX_TABLE_WORDS = 4 int64 words rtfs_mix_f32 reads FROM DEVICE MEMORY (the caller uploads them
 *   once), per slot [address of the segment's first sample (0: empty) | address of the reference's first sample (0: none) | the bits
 *   of a | (segment is int16) + 2 (reference is int16)].  Refusals return -4, write nothing else and name themselves in
 *   refused[2] = [row * J + slot or -1 | RTFS_MIX_* reason]: B < 1, a missing array, a grid that would not fit (BAD_ARGUMENT); L outside
 *   [1, RTFS_MIX_MAX_LENGTH] (BAD_LENGTH); n_out outside [0, J] (BAD_N_OUT); a segment or reference that leaves its source
 *   (SEGMENT_RANGE / REFERENCE_RANGE); a row whose slots are all empty (EMPTY_ROW, slot 0 of the row); an address that is misaligned
 *   for its dtype (MISALIGNED); an unknown dtype (BAD_DTYPE).  table, ws_bytes, refused may be NULL.
 * rtfs_mix_workspace_bytes: B * ceil(L / RTFS_MIX_CHUNK) * RTFS_MIX_MOMENTS doubles; 0 for sizes the plan refuses.
 * rtfs_mix_f32 (two launches): pass 1, one workgroup per (row, chunk of RTFS_MIX_CHUNK samples), writes the chunk's RTFS_MIX_MOMENTS
 *   float64 partial moments into ws: [sum x_j (J) | E(ref_j) (J) | sum x_i x_j, i <= j, row-major (the diagonal is E(x_j))]; the square
 *   or product of two float32 values is exact in double.  Pass 2 re-reduces its row's partials in a fixed order (L is bounded so that
 *   a row has at most 256 chunks, one per thread), forms the gains and sum m = sum_j g_j sum x_j, sum m^2 = g^T G g, hence mean and
 *   deviation without a pass over m, and writes the outputs: 16-byte stores on each output row's own 16-byte grid, scalar head and
 *   tail.  mixture (B,L), sources (B,n_out,L) (may be NULL with n_out = 0) 4-byte aligned; stats, ws, table 8-byte aligned (-4);
 *   ws_bytes below the query: -2; sizes the plan refuses: -1; all before any launch.  Caller's stream, no allocation, nothing read
 *   back, no atomics: the same inputs give the same bits.  The launches trust the device table: pass what rtfs_mix_plan wrote. */
#define RTFS_MIX_MAX_SOURCES 4
#define RTFS_MIX_CHUNK 4096
#define RTFS_MIX_MAX_LENGTH (1 << 20)
#define RTFS_MIX_RECIPE_WORDS 8
#define RTFS_MIX_TABLE_WORDS 4
#define RTFS_MIX_MOMENTS 18
#define RTFS_MIX_F32 0
#define RTFS_MIX_I16 1
#define RTFS_MIX_BAD_ARGUMENT 1
#define RTFS_MIX_BAD_LENGTH 2
#define RTFS_MIX_BAD_N_OUT 3
#define RTFS_MIX_SEGMENT_RANGE 4
#define RTFS_MIX_REFERENCE_RANGE 5
#define RTFS_MIX_EMPTY_ROW 6
#define RTFS_MIX_MISALIGNED 7
#define RTFS_MIX_BAD_DTYPE 8
size_t rtfs_mix_workspace_bytes(int B, int L);
int rtfs_mix_plan(const long long* slots, const double* a, int B, int L, int n_out, long long* table, size_t* ws_bytes, int* refused);
int rtfs_mix_f32(const long long* table, float* mixture, float* sources, double* stats, int B, int L, int n_out, int normalize, double eps,
                 void* ws, size_t ws_bytes, void* stream);

/* Reverberant mixtures (datas.reverberate, datas.mix_batch(rirs=...), System.mix_batch(rirs=...); DESIGN.md "Reverberant mixtures";
 * csrc/k_reverb.hip): every source convolved with its own room impulse response (RIR) before the mix, the WHAMR! / SMS-WSJ recipe.
 * A job names a source x of n_x samples (float32 at any 4-byte alignment, or int16 PCM at any 2-byte alignment entering as
 * (float)s / 32768, read where it lies), a segment start p with 0 <= p, p + L <= n_x, an RIR h of N float32 taps on the device at any
 * 4-byte alignment, 1 <= N <= RTFS_REVERB_MAX_TAPS, and an offset o, 0 <= o < N.  With x~[i] = x[i] for 0 <= i < n_x and 0 elsewhere,
 * the image is
 *   r[t] = (float) sum_{k=0}^{N-1} h[k] x~[p + t + o - k],  t = 0 .. L-1.
 * The sum is in float64, where the product of two float32 values is exact; its terms are added one by one in the order k = 0, 1, ...
 * (fused multiply-add on the converted operands, which rounds once per term as add after an exact multiply does), so the same inputs
 * give the same bits whatever the batch or the scheduling.  Exactly the N terms of the sum enter: no tap and no sample is padded in,
 * and a sample outside [max(0, p + o - N + 1), min(n_x, p + o + L)) never reaches an output.  History before the segment is read from
 * the utterance itself (a crop of a reverberant utterance, not a reverberated crop); before sample 0 and past the last sample the
 * room is silent.  o lets a caller cancel the direct-path delay (o = argmax |h|): the image then stays sample-aligned with the dry
 * segment.
 * A reverberant mixture is the mixture definition above applied to images: a slot with an RIR contributes its image r_j wherever the
 * definition says x_j, a reference with an RIR contributes E(r_ref); the energy rule, the SNRs (now between images), the order of the
 * sum, the normalisation and stats are unchanged, and a slot without an RIR is read dry from its source as before.
 * rtfs_reverb_plan (host only, no device call): jobs = S records of RTFS_REVERB_RECIPE_WORDS = 7 int64 words [source address | source
 *   length in samples | dtype RTFS_MIX_F32 / RTFS_MIX_I16 | start p | RIR address | taps N | offset o] -> when table is not NULL, the
 *   S * RTFS_REVERB_JOB_WORDS = 6 int64 words rtfs_reverb_f32 reads FROM DEVICE MEMORY, per job [source address | n_x | p + o | RIR
 *   address | N | source is int16].  Refusals return -4, write nothing else and name themselves in refused[2] = [job or -1 | reason],
 *   with the RTFS_MIX_* reasons and two more: S < 1, a missing array, a work list of S * ceil(L / RTFS_REVERB_TILE) past 2^31 - 1
 *   (BAD_ARGUMENT, -1); L outside [1, RTFS_MIX_MAX_LENGTH] (BAD_LENGTH, -1); per job, in this order: a null source or RIR address
 *   (BAD_ARGUMENT); an unknown dtype (BAD_DTYPE); a source address misaligned for its dtype or an RIR address off the 4-byte grid
 *   (MISALIGNED); a segment that leaves its source (SEGMENT_RANGE); taps outside [1, RTFS_REVERB_MAX_TAPS] (RTFS_REVERB_BAD_TAPS); an
 *   offset outside [0, taps) (RTFS_REVERB_BAD_OFFSET).  table and refused may be NULL.
 * rtfs_reverb_f32 (one launch): images (S, L) float32, 4-byte aligned, row s = the image of job s; table 8-byte aligned (-4); sizes
 *   the plan refuses: -1.  One workgroup per (image, tile of RTFS_REVERB_TILE outputs) walks the taps in chunks of
 *   RTFS_REVERB_TAP_CHUNK, staging the chunk's taps and the TILE + CHUNK - 1 samples they touch in LDS (int16 converted, zeros outside
 *   the utterance); each thread keeps 8 consecutive outputs in float64 registers.  16-byte stores on the row's own 16-byte grid,
 *   scalar head and tail.  Caller's stream, no allocation, no workspace, nothing read back, no atomics, one writer per cell.  The
 *   launch trusts the device table: pass what rtfs_reverb_plan wrote.
 * rtfs_mix_reverb_plan (host only): rtfs_mix_plan's slots and a, plus rirs = B * J records of RTFS_MIX_RIR_WORDS = 6 int64 words [RIR
 *   address of the slot's segment (0: dry) | its taps | its offset | RIR address of the slot's reference (0: dry) | its taps | its
 *   offset].  Every distinct (source address, dtype, start, RIR address, taps, offset) gets ONE image row, numbered in the order the
 *   slots name them (row-major; a slot's segment before its reference): a target's image that is also its interferers' reference is
 *   computed once.  -> *n_images = S, *ws_bytes = rtfs_mix_workspace_bytes(B, L) and, when table is not NULL, ONE table of
 *   S * RTFS_REVERB_JOB_WORDS + B * J * RTFS_MIX_TABLE_WORDS words: the reverb jobs, then rtfs_mix_plan's table of the recipe in which
 *   every reverberant segment or reference is the float32 row `images + 4 L row` (images: the device address of the (S, L) buffer the
 *   caller allocates after a first call with table = NULL; it may be 0 while table is NULL or S is 0).  Refusals (-4, refused as
 *   above with row * J + slot, nothing else written): a missing array and everything rtfs_mix_plan refuses, first; then images off
 *   the 4-byte grid (MISALIGNED, -1); then per slot in row-major order what rtfs_reverb_plan refuses of a job; then S * tiles past
 *   2^31 - 1 or a table asked for with S > 0 and images = 0 (BAD_ARGUMENT, -1).  With no RIR anywhere S = 0 and the table is
 *   rtfs_mix_plan's.
 * rtfs_mix_reverb_f32 (THREE launches; two with n_images = 0, then it is rtfs_mix_f32 on the same table): the reverb launch on the
 *   first n_images jobs of the table, then rtfs_mix_f32 on the words behind them.  Arguments and error codes as rtfs_mix_f32; images
 *   4-byte aligned and not NULL when n_images > 0.  All checks before any launch. */
#define RTFS_REVERB_TILE 1024
#define RTFS_REVERB_TAP_CHUNK 768
#define RTFS_REVERB_MAX_TAPS 16384
#define RTFS_REVERB_RECIPE_WORDS 7
#define RTFS_REVERB_JOB_WORDS 6
#define RTFS_MIX_RIR_WORDS 6
#define RTFS_REVERB_BAD_TAPS 9
#define RTFS_REVERB_BAD_OFFSET 10
int rtfs_reverb_plan(const long long* jobs, int S, int L, long long* table, int* refused);
int rtfs_reverb_f32(const long long* table, float* images, int S, int L, void* stream);
int rtfs_mix_reverb_plan(const long long* slots, const double* a, const long long* rirs, int B, int L, int n_out, long long images,
                         long long* table, int* n_images, size_t* ws_bytes, int* refused);
int rtfs_mix_reverb_f32(const long long* table, int n_images, float* images, float* mixture, float* sources, double* stats, int B, int L,
                        int n_out, int normalize, double eps, void* ws, size_t ws_bytes, void* stream);

/* Loudness (datas.loudness / loudness_many / loudness_normalize, MixRecipe.lufs, System.mix_batch(loudness=...); DESIGN.md "Loudness";
 * csrc/k_loudness.hip, csrc/loudness.h): ITU-R BS.1770 integrated loudness of mono recordings, float64 throughout.
 * Sample rate: fs an integer, RTFS_LOUD_MIN_RATE = 8000 <= fs <= RTFS_LOUD_MAX_RATE = 192000, fs % 10 == 0.  H = fs / 10 is one hop
 *   of 100 ms, a block is 4 H samples.
 * Input: float32 at any 4-byte alignment, or int16 PCM at any 2-byte alignment entering as (float)s / 32768; read where it lies.
 * K-weighting: two biquads in series with zero initial state; coefficients from the design formulas in float64 on the host
 *   (csrc/loudness.h, the single place):
 *   shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196;  K = tan(pi f0 / fs), Vh = 10^(G/20),
 *              Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2;  b = [Vh + Vb K/Q + K^2, 2 (K^2 - Vh), Vh - Vb K/Q + K^2] / a0,
 *              a = [1, 2 (K^2 - 1) / a0, (1 - K/Q + K^2) / a0]
 *   high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773;  b = [1, -2, 1], a formed as above from its own K.
 *   At 48 kHz these are the standard's table (shelf b 1.53512485958697, -2.69169618940638, 1.19839281085285, a -1.69065929318241,
 *   0.73248077421585; high-pass a -1.99004745483398, 0.99007225036621).
 * Hop and block energies: with y the filtered signal of a recording of L samples, E_h = sum of y[n]^2 over n in [h H, (h + 1) H) for
 *   h < floor(L / H); the L mod H samples behind the last whole hop are never read.  Block j has
 *   z_j = (E_j + E_{j+1} + E_{j+2} + E_{j+3}) / (4 H) for j < nb = floor(L / H) - 3: complete blocks only, as the standard says
 *   (pyloudnorm rounds the block count instead; agreement with that package is not measured).
 * Gates, applied to z (no logarithm decides a gate): absolute z_j > 10^((-70 + 0.691) / 10); relative z_j > 0.1 x the mean of z over
 *   the absolutely gated blocks.  lufs = -0.691 + 10 log10(mean of z over the blocks passing both), kept = the number of such blocks.
 *   No surviving block: lufs = -inf, kept = 0.  Any non-finite z_j: lufs = NaN (kept = 0).
 * The cascade is the linear system s' = A s + B x, y = C s + D x over the four states of two transposed direct form II biquads.  A
 *   wave takes a hop and gives lane l the piece [min(l p, H), min((l + 1) p, H)), p = ceil(H / RTFS_LOUD_LANES); every lane runs its
 *   piece from zero state, the piece end states are combined across the lanes with A^p (A^(H mod p) behind the one ragged piece), the
 *   hop end states along the recording with A^H in a per-recording scan, and a second sweep over the samples accumulates the
 *   energies from the true start states.  The powers are multiplied out on the host in long double and rounded once.
 * rtfs_loudness_design (host only): the eight doubles [shelf b0 b1 b2 a1 a2 | high-pass a1 a2 | the absolute gate] for fs; -4 for a
 *   rate the definition does not cover.
 * rtfs_loudness_plan (host only, no device call): recs = R records of RTFS_LOUD_RECORD_WORDS = 3 int64 words [address | length in
 *   samples | dtype RTFS_MIX_F32 / RTFS_MIX_I16] -> *ws_bytes, totals[4] = [hops | blocks | samples | gain chunks] of the pool and,
 *   when table is not NULL, the RTFS_LOUD_HEADER_WORDS + R * RTFS_LOUD_TABLE_WORDS int64 words the launches read FROM DEVICE MEMORY
 *   (one upload): the header [fs | H | p | R | hops | blocks | samples | chunks | the eight doubles of rtfs_loudness_design | A^p |
 *   A^(H mod p) | A^H, row-major], then per recording [address | L | is int16 | hops | first hop | first sample | first gain chunk |
 *   first block], the last four being the recording's offsets in the flat work lists and buffers.  Refusals return -4, write nothing
 *   else and name themselves in refused[2] = [recording or -1 | RTFS_LOUD_* reason]: R < 1, a missing array, a work list past
 *   2^31 - 1 (BAD_ARGUMENT, -1); a rate outside the definition (BAD_RATE, -1); per recording in this order a null address
 *   (BAD_ARGUMENT), an unknown dtype (BAD_DTYPE), an address misaligned for its dtype (MISALIGNED), L < 4 H (TOO_SHORT),
 *   L > RTFS_LOUD_MAX_LENGTH = 2^26 (TOO_LONG).  table, ws_bytes, totals, refused may be NULL.
 * rtfs_loudness_f32 (FOUR launches): out (R, 2) float64 = [lufs | kept]; z, if not NULL, the flat float64 buffer of totals[1] block
 *   energies, recording r at its first-block offset.  Flat work lists over (recording, hop), one wave each, for the two sweeps; one
 *   thread per recording for the scan; one workgroup per recording for the gates.  host_table: the host copy of the table, of which
 *   only the header's sizes are read.  table, out, z, ws 8-byte aligned (-4); ws_bytes below the plan's: -2; a header no plan
 *   writes: -1; all before any launch.  Caller's stream, no allocation, nothing read back, no atomics, fixed reduction orders: the
 *   same inputs give the same bits, and entry r of a pool is bit-equal to recording r measured alone.
 * rtfs_loudness_gain_f32 (one launch): out, flat float32 of totals[2] samples, recording r at its first-sample offset:
 *   out = (float)(x g) with g = 10^((target - lufs) / 20) formed on the device in float64 from loud (R, 2) as rtfs_loudness_f32 wrote
 *   it, g = 1 where lufs is not finite; stats (R) float64 = g.  One workgroup per (recording, chunk of RTFS_LOUD_CHUNK samples). */
#define RTFS_LOUD_LANES 64
#define RTFS_LOUD_CHUNK 4096
#define RTFS_LOUD_MAX_LENGTH (1 << 26)
#define RTFS_LOUD_MIN_RATE 8000
#define RTFS_LOUD_MAX_RATE 192000
#define RTFS_LOUD_RECORD_WORDS 3
#define RTFS_LOUD_HEADER_WORDS 64
#define RTFS_LOUD_TABLE_WORDS 8
#define RTFS_LOUD_BAD_ARGUMENT 1
#define RTFS_LOUD_BAD_RATE 2
#define RTFS_LOUD_TOO_SHORT 3
#define RTFS_LOUD_TOO_LONG 4
#define RTFS_LOUD_MISALIGNED 5
#define RTFS_LOUD_BAD_DTYPE 6
int rtfs_loudness_design(int fs, double* coef);
int rtfs_loudness_plan(const long long* recs, int R, int fs, long long* table, size_t* ws_bytes, long long* totals, int* refused);
int rtfs_loudness_f32(const long long* table, const long long* host_table, double* out, double* z, void* ws, size_t ws_bytes, void* stream);
int rtfs_loudness_gain_f32(const long long* table, const long long* host_table, const double* loud, double target, float* out, double* stats,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
