/*
 * libmms2ut_hip — C-ABI of the MI355X-native mm_s2ut_transformer training path.
 *
 * Every entry point takes raw device pointers, int64 sizes/strides, scalars and the HIP stream to
 * enqueue on (PyTorch's current stream).  All buffers, including workspaces, belong to the caller
 * (PyTorch's caching allocator).  The library keeps one piece of state: a per-device pool of
 * zeroed ticket arrays for the short-M GEMM's in-kernel split-K (4 MiB, allocated on the device's
 * first such launch; one 8 KiB slice per (device, stream), handed out under a mutex; every completed
 * launch leaves its slice zero).  Apart from that pool, the GEMM route switches below and the bound
 * step seed, entry points keep no state and may be called from several host threads; kernels are
 * only ever enqueued on the passed stream.  Functions return 0 on success and non-zero on error;
 * mms2ut_last_error() returns the message (thread-local).
 *
 * Each entry cites the reference interface (or the fairseq/PyTorch op it executes for the
 * reference) that it replaces — see SURVEY.md §8(a)/(b) and INTEGRATION.md.
 */
#ifndef MMS2UT_H
#define MMS2UT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef _Float16 mms2ut_half;

/* ---------------------------------------------------------------- errors / introspection */
const char* mms2ut_last_error(void);
/* A non-blocking HIP stream (hipStreamNonBlocking) at a priority clamped to the device's range
 * (lower = more urgent): the trainer's critical-path and weight-gradient side streams, so that no
 * work a caller leaves on the legacy NULL stream implicitly orders itself behind them.           */
int mms2ut_stream_create(int priority, hipStream_t* out);
/* Destroys a stream from mms2ut_stream_create (after the work enqueued on it has completed).     */
int mms2ut_stream_destroy(hipStream_t stream);
int mms2ut_version(void);

/* ---------------------------------------------------------------- GEMM (MFMA fp16, fp32 acc)
 * Replaces every nn.Linear / bmm / conv-as-GEMM the reference executes through cuBLAS:
 * fairseq MultiheadAttention q/k/v/out_proj, TransformerEncoderLayer/DecoderLayer fc1/fc2,
 * Conv1dSubsampler convs (im2col), fusion projections (fuse.py:76-78,116; nn.MultiheadAttention
 * in_proj/out_proj for fuse.py:161), the gate dense (mm_s2s_transformer.py:613-614) and the tied
 * output projection — forward, dgrad and wgrad.
 *   C[m][n] = epi(alpha * sum_k A(m,k) B(n,k))
 *   A(m,k) = a_kcontig ? A[m*lda+k] : A[k*lda+m];  B(n,k) = b_kcontig ? B[n*ldb+k] : B[k*ldb+n]
 *   batch z in [0,batch): z1 = z / bdiv, z2 = z % bdiv; X += z1*sX1 + z2*sX2 (elements)
 *   split-K (epi = MMS_EPI_F32 only): slab s written at C + s*sCsplit (fp32)            */
enum {
  MMS_EPI_F16 = 0,          /* C = alpha*acc (+bias)                                      */
  MMS_EPI_RELU_DROP = 1,    /* C = dropout(relu(alpha*acc + bias))        (fc1)           */
  MMS_EPI_DROP_RESID = 2,   /* C = aux + dropout(alpha*acc + bias)        (out_proj, fc2) */
  MMS_EPI_F32 = 3,          /* C(fp32) = alpha*acc                        (split-K slabs) */
  MMS_EPI_GATE = 4,         /* g = sigmoid(acc+bias); C = t + g*(o-t); out2 = g; o = aux[:, :N], t = aux[:, N:2N] */
  MMS_EPI_RELU_DROP_BWD = 5,/* C = aux>0 ? alpha*acc/(1-p) : 0            (fc2 dgrad -> fc1 pre-act) */
  MMS_EPI_F16_ACC = 6,      /* C += alpha*acc                                               */
  MMS_EPI_GELU_DROP = 7,    /* z = alpha*acc + bias; out2 = z; C = dropout(gelu(z))  (torch F.gelu, erf form) */
  MMS_EPI_GELU_DROP_BWD = 8 /* z = aux: C = keep ? alpha*acc/(1-p) * gelu'(z) : 0 (mask regenerated from seed/offset) */
};

typedef struct mms2ut_gemm_args {
  const mms2ut_half* A;
  const mms2ut_half* B;
  void* C;
  int M, N, K;
  int a_kcontig, b_kcontig;
  int64_t lda, ldb, ldc;
  int batch, bdiv;
  int64_t sA1, sA2, sB1, sB2, sC1, sC2;
  int splitk;
  int64_t sCsplit;
  int epi;
  float alpha;
  const mms2ut_half* bias;
  const mms2ut_half* aux;
  int64_t ldaux, sX1, sX2;
  mms2ut_half* out2;
  int64_t ldo2;
  float dropout_p;
  uint64_t seed, offset;
  int64_t ld_rng;
  /* optional (epi = MMS_EPI_F32, a_kcontig = 0): fp32 A-row sums alpha*sum_k A(m,k) of split s
   * -> rowsum[s*ld_rowsum + m].  The weight-gradient GEMM's A is dy^T, so these are the split-K
   * partials of the bias gradient (replaces a separate column-sum pass over dy).             */
  float* rowsum;
  int64_t ld_rowsum;
  /* split-K with a fused-epilogue fixup (any epi but MMS_EPI_F32, batch 1, splitk > 1, N % 4 == 0):
   * the splits write alpha-scaled fp32 partials to splitk_ws[s][M][N] (>= splitk*M*N floats),
   * then one pass sums them in split order and applies the epilogue exactly as the unsplit GEMM
   * (same bias / residual / dropout counters).  For the short-M shapes (decoder tokens) whose
   * unsplit grid covers a tenth of the CUs.                                                       */
  float* splitk_ws;
  int64_t splitk_ws_floats;
} mms2ut_gemm_args;

int mms2ut_gemm_f16(const mms2ut_gemm_args* args, hipStream_t stream);
/* NT shapes (both operands K-contiguous, batch 1, no split) may run on 96 / 160 / 192 x 128 tiles
 * instead of 128 x 128 ones when that takes fewer rounds of the 512 block slots, or (96 rows) fills
 * a short single round better, weighted by each height's measured per-round cost (e.g. M = 11-16 k
 * rows x N = 768: one round instead of two); bit-identical results.  mode 1: by that rule (default;
 * env MMS2UT_GEMM_TALL overrides it at first use), 0: never, 2 / 3 / 5: 160 / 192 / 96-row tiles
 * for every qualifying NT shape (tests).                                                          */
int mms2ut_gemm_set_tall(int mode);

/* Short-M NT GEMMs (a 128x128 grid of fewer than 128 tiles: the decoder's ~470-row projections).
 * mode 1 (default; env MMS2UT_GEMM_SKINNY overrides it at first use): a measured route table —
 * N <= 1024 on the short-M kernel (one-shot operand loads per small tile, K split across blocks
 * with an in-kernel last-arrival reduction into the caller's splitk_ws, epilogue fused, no second
 * launch), N > 1024 with K <= 1024 unsplit on the 128-row tiles, the rest on the split-K + fixup
 * route the caller asked for; 0: always the caller's route (A/B runs, tests); 2: the short-M kernel
 * for every short-M shape (tests).                                                              */
int mms2ut_gemm_set_skinny(int mode);
/* Test hook of the short-M kernel's split-K hand-off (placement-independent: write-through partials,
 * a relaxed agent-scope ticket, write-through reads).  scatter != 0 deals the splits of every tile
 * over different XCD groups (bid % 8) instead of keeping them together; xcc_out (device, >= grid
 * ints, or NULL) receives each block's hardware XCD id (HW_REG_XCC_ID).  Bits are identical either
 * way.                                                                                         */
int mms2ut_gemm_skinny_debug(int scatter, int* xcc_out);
/* Test hook of the fused epilogues: staged != 0 routes every fp16 epilogue through the fp32 LDS
 * staging (the round-5 form) instead of the register epilogue (plain / ReLU-dropout: element math
 * in the MFMA layout, fp16 through LDS).  Bits are identical either way.                        */
int mms2ut_gemm_set_epilogue(int staged);

/* Grouped weight gradients of one transformer layer (torch.nn.Linear weight / bias grads of the
 * reference layer's projections): for each of the n <= 8 problems, dW[N, K] = dy[rows, N]^T @
 * x[rows, K] (fp16, row stride K, overwritten) and, when db != NULL, db[N] = column sums of dy —
 * all in ONE launch over the union of the problems' 128x128 tiles, unsplit (fp32 accumulation over
 * all rows, no split-K slabs).  lddy, ldx multiples of 8; N, K multiples of 8; dy, x, dW 16-B
 * aligned.  Deterministic (fixed reduction order per tile).  max_blocks > 0 caps the grid
 * (rounded down to a multiple of 8): blocks then walk the tiles persistently, so a launch on a
 * side stream never holds more than that many block slots (0: one block per tile).            */
typedef struct mms2ut_wgrad {
  const mms2ut_half* dy;
  int64_t lddy;
  const mms2ut_half* x;
  int64_t ldx;
  mms2ut_half* dW;
  mms2ut_half* db;
  int N, K;
} mms2ut_wgrad;
int mms2ut_wgrad_group(const mms2ut_wgrad* w, int n, int64_t rows, int max_blocks, hipStream_t stream);

/* live GEMM timing for the benchmark roofline: between begin/end every mms2ut_gemm_f16 launch
 * is bracketed by HIP events on its own stream (or, in stamp mode below, timed by its own
 * workgroups); end() synchronises and returns the summed event time (0 in stamp mode), the launch
 * count and the launched (padded) FLOPs.  Bench-only instrumentation, not thread-safe.      */
int mms2ut_profile_begin(int max_launches);
int mms2ut_profile_end(float* total_ms, int* launches, double* flops);
/* algorithmic HBM bytes of the GEMM launches of the last begin/end window (A and B read once, C
 * written once; fp32 split-K slabs, residual / accumulate / gate operands included)            */
int mms2ut_profile_bytes(double* bytes);
/* per-launch record of the last finished window (first n launches): kernel ms, launched FLOPs and
 * a class word: bit0 A K-contiguous, bit1 B K-contiguous, bits 2-7 epilogue, bit8 batched,
 * bit9 split-K.  Lets the bench split forward / dgrad (NT) from weight-gradient (TN) launches.   */
int mms2ut_profile_launches(float* ms, double* flops, int* cls, int n);
/* the same window's shapes: mnk[4i..4i+3] = M, N, K, batch * splitk of launch i                  */
int mms2ut_profile_shapes(int* mnk, int n);
/* stamp mode for the open window (call right after profile_begin): instead of events, every GEMM
 * kernel's blocks store {start, end} s_memrealtime ticks (2 x u64 per block) into `stamps`
 * (device, 16-B aligned, room for cap_blocks blocks).  profile_blocks then gives, per launch,
 * the first block slot and one past the last (a split-K fixup's blocks follow its GEMM's; a
 * value > cap_blocks means the buffer overflowed and the launch was not recorded).  A launch's
 * duration = max(end) - min(start) over its slots, in ticks of mms2ut_wallclock_khz.  Bench-only
 * instrumentation (no reference counterpart).                                                    */
int mms2ut_profile_stamps(unsigned long long* stamps, long cap_blocks);
int mms2ut_profile_blocks(long* first_last, int n);
int mms2ut_wallclock_khz(int* khz);

/* sum `nsplit` fp32 slabs [rows, cols] (slab stride `slab`) * alpha -> out, row stride ldo.
 * mode bit0: fp16 output (else fp32); bit1: accumulate into out (else overwrite)            */
int mms2ut_splitk_reduce(const float* slabs, int nsplit, int64_t slab, int rows, int cols,
                         void* out, int64_t ldo, int mode, float alpha, hipStream_t stream);
/* the weight-gradient epilogue in one launch: fp16 dW = sum of `nsplit` fp32 slabs [rows, cols]
 * (row stride ldo) and fp16 db[rows] = sum of the GEMM's rowsum partials rs_slabs[nsplit][rows].
 * rows, cols, ldo multiples of 4.  Replaces the bias column-sum of dy (fairseq Linear.bias.grad). */
int mms2ut_splitk_reduce_bias(const float* slabs, int nsplit, int64_t slab, int rows, int cols,
                              mms2ut_half* out, int64_t ldo, const float* rs_slabs,
                              mms2ut_half* rs_out, hipStream_t stream);

/* batched transpose of row-major fp16 matrices: dst[d.dst + c*rows + r] = src[d.src + r*cols + c]
 * (element offsets).  descs (DEVICE memory) sorted by tile0, the first 64x64 tile of each matrix;
 * rows, cols multiples of 8.  Keeps the W^T images that make every dgrad GEMM NT (K-contiguous
 * operands) — the reference's cuBLAS dgrad reads W in place.                                    */
typedef struct mms2ut_transpose_desc {
  int64_t src, dst;
  int32_t rows, cols, tile0, pad;
} mms2ut_transpose_desc;
int mms2ut_transpose_batch(const mms2ut_half* src, mms2ut_half* dst, const mms2ut_transpose_desc* descs,
                           int n, int total_tiles, hipStream_t stream);

/* `waiter` waits for all work enqueued on `signaler` so far (event record + stream wait).
 * Forks/joins the weight-gradient side stream (the reference's DDP/autograd stream overlap). */
int mms2ut_stream_wait(hipStream_t waiter, hipStream_t signaler);
/* Device-scope events (no timing, no system-scope fence): ordering between this process's streams
 * on one GPU — the deferred optimizer chunks before the next forward reads them, the weight
 * transpose before the dgrad GEMMs, per-group gradient hand-offs (torch's CUDA events in the
 * reference's DDP / autograd stream syncs).  Not for host synchronisation.                       */
int mms2ut_event_create(hipEvent_t* out);
int mms2ut_event_record(hipEvent_t event, hipStream_t stream);
int mms2ut_event_wait(hipStream_t stream, hipEvent_t event);
int mms2ut_event_destroy(hipEvent_t event);
/* HIP-graph replay of the training step: every dropout kernel adds *delta (a device uint64) to
 * the seed it was launched or captured with; delta == NULL (the default) leaves seeds unchanged.
 * mms2ut_step_seed_advance(delta, inc) is the first node of a captured step (delta += inc), so
 * each replay draws fresh masks (fairseq reseeds torch's generator per update in
 * Trainer.train_step; here the per-update seed lives on the device).                           */
int mms2ut_bind_step_seed(const uint64_t* delta);
int mms2ut_step_seed_advance(uint64_t* delta, uint64_t inc, hipStream_t stream);

/* ---------------------------------------------------------------- LayerNorm (eps, affine)
 * Replaces fairseq LayerNorm (self_attn_layer_norm / final_layer_norm / encoder_attn_layer_norm /
 * encoder.layer_norm / decoder.layer_norm) and nn.LayerNorm image_pre_norm_module
 * (mm_s2s_transformer.py:188-190,595).  Rows of D fp16, statistics fp32.                  */
int mms2ut_layernorm_fwd(const mms2ut_half* x, const mms2ut_half* gamma, const mms2ut_half* beta,
                         mms2ut_half* y, float* mean, float* rstd, int64_t rows, int D, float eps,
                         hipStream_t stream);
/* dx = LN'(dy) (+ dres if non-null); partial dgamma/dbeta sums -> part[nblk][2][D] (fp32).
 * dx may be null (parameter grads only).  If dxd is non-null it also receives dropout(dx) with
 * counters offset + row*D + col: the residual-branch dropout of the sublayer below, whose
 * output-projection gradient consumes it (saves a separate dropout pass).                  */
int mms2ut_layernorm_bwd(const mms2ut_half* dy, const mms2ut_half* x, const mms2ut_half* gamma,
                         const float* mean, const float* rstd, const mms2ut_half* dres,
                         mms2ut_half* dx, float* part, int64_t rows, int D, mms2ut_half* dxd,
                         float p, uint64_t seed, uint64_t offset, hipStream_t stream);
int mms2ut_layernorm_bwd_parts(int64_t rows);
/* number of [2*D] fp32 partial rows mms2ut_layernorm_bwd{,_ex} write for (rows, D) */
int mms2ut_layernorm_bwd_nparts(int64_t rows, int D);
/* layernorm_fwd with an output layout and dropout folded in (the fusion image path,
 * mm_s2s_transformer.py:188-190 image_pre_norm -> SA_image_dropout -> [B, Ti(+1), Di] keys):
 * input row r is written to output row (r / grp) * grp_out + r % grp (grp = 0: identity), and
 * y = dropout_p(LN(x)) with counters offset + r*D + col (the unpadded element index).         */
int mms2ut_layernorm_fwd_ex(const mms2ut_half* x, const mms2ut_half* gamma, const mms2ut_half* beta,
                            mms2ut_half* y, float* mean, float* rstd, int64_t rows, int D, float eps,
                            int64_t grp, int64_t grp_out, float p, uint64_t seed, uint64_t offset,
                            hipStream_t stream);
/* layernorm_bwd whose dy is read through the same layout (row r from (r / dy_grp) * dy_grp_out +
 * r % dy_grp) and dropout (dy_p, dy_seed, dy_offset; unpadded counters): the backward of
 * layernorm_fwd_ex without materialising the unpadded, dropped-out gradient.  D % 256 == 0.    */
int mms2ut_layernorm_bwd_ex(const mms2ut_half* dy, const mms2ut_half* x, const mms2ut_half* gamma,
                            const float* mean, const float* rstd, const mms2ut_half* dres,
                            mms2ut_half* dx, float* part, int64_t rows, int D, mms2ut_half* dxd,
                            float p, uint64_t seed, uint64_t offset, int64_t dy_grp, int64_t dy_grp_out,
                            float dy_p, uint64_t dy_seed, uint64_t dy_offset, hipStream_t stream);
/* column sums of fp32 partials [nparts][ncol] -> out (fp16), out += if accumulate */
int mms2ut_colsum_parts(const float* part, int nparts, int ncol, mms2ut_half* out, int accumulate,
                        hipStream_t stream);
/* column sums of an fp16 matrix [rows][cols] (row stride ld) -> part[nparts][cols] fp32 (bias grads) */
int mms2ut_colsum_f16(const mms2ut_half* x, int64_t rows, int cols, int64_t ld, float* part,
                      int nparts, hipStream_t stream);
int mms2ut_colsum_nparts(int64_t rows);

/* ---------------------------------------------------------------- attention softmax
 * Masked softmax over attention scores S[z][Tq][ldS] (fp16) with per-batch key lengths
 * (key padding mask, fairseq/torch MHA key_padding_mask), optional causal mask
 * (buffered_future_mask), optional "always-valid" trailing key (add_bias_kv column of
 * nn.MultiheadAttention, fuse.py:161), and attention-prob dropout (p, counter RNG).
 * Keys may instead be masked by key_mask[b*ld_mask + j] != 0 (bool key_padding_mask).
 * Writes P (undropped) and Pd (dropped, may alias P when p == 0).  z = b*H + h.            */
int mms2ut_attn_softmax_fwd(const mms2ut_half* S, mms2ut_half* P, mms2ut_half* Pd, int Z, int H,
                            int Tq, int Tk, int64_t ldS, const int32_t* key_len,
                            const uint8_t* key_mask, int64_t ld_mask, int causal,
                            int extra_key, float p, uint64_t seed, uint64_t offset,
                            hipStream_t stream);
/* dS = P * (dPd*mask/(1-p) - sum_j Pd_j dPd_j) ; dP may alias dS                            */
int mms2ut_attn_softmax_bwd(const mms2ut_half* P, const mms2ut_half* dPd, mms2ut_half* dS, int Z,
                            int H, int Tq, int Tk, int64_t ldS, const int32_t* key_len, int causal,
                            int extra_key, float p, uint64_t seed, uint64_t offset,
                            hipStream_t stream);
/* The same two kernels (H = 1) for the query-side fusion attention (gated fusion below), whose
 * key / value biases travel as `npad` tail columns of the query-side matrices.  Forward: row r
 * adds scale * q_aug[r*ld_q + 0] to the scores of keys j < n_img and scale * q_aug[r*ld_q + 1] to
 * the keys j >= n_img before the maximum, and writes u_aug[r*ld_u + 0..npad) = {sum of Pd over
 * j < n_img, sum over j >= n_img, 0, ...}.  Backward: du_aug[r*ld_du + 0 / 1] is added to dPd on
 * the keys j < n_img / j >= n_img, and dq_aug[r*ld_dq + 0..npad) = {scale * sum of dS over
 * j < n_img, scale * sum over j >= n_img, 0, ...}.  2 <= npad <= 64.                          */
int mms2ut_attn_softmax_fwd_aug(const mms2ut_half* S, mms2ut_half* P, mms2ut_half* Pd, int Z, int Tq, int Tk,
                                int64_t ldS, const uint8_t* key_mask, int64_t ld_mask, int extra_key, float p,
                                uint64_t seed, uint64_t offset, const mms2ut_half* q_aug, int64_t ld_q,
                                float scale, int n_img, mms2ut_half* u_aug, int64_t ld_u, int npad,
                                hipStream_t stream);
int mms2ut_attn_softmax_bwd_aug(const mms2ut_half* P, const mms2ut_half* dPd, mms2ut_half* dS, int Z, int Tq,
                                int Tk, int64_t ldS, float p, uint64_t seed, uint64_t offset,
                                const mms2ut_half* du_aug, int64_t ld_du, float scale, int n_img,
                                mms2ut_half* dq_aug, int64_t ld_dq, int npad, hipStream_t stream);
/* out[rows][Dia] = [wkv[rows][Di] | bkv | bias_kv (or 0) | 0...], and its inverse for the gradient
 * (g_bias_kv may be NULL); rows = 2d (the K then the V half).                                  */
int mms2ut_fusion_pack_kv(const mms2ut_half* wkv, const mms2ut_half* bkv, const mms2ut_half* bias_kv,
                          mms2ut_half* out, int rows, int Di, int Dia, hipStream_t stream);
int mms2ut_fusion_unpack_kv(const mms2ut_half* dw, mms2ut_half* g_wkv, mms2ut_half* g_bkv,
                            mms2ut_half* g_bias_kv, int rows, int Di, int Dia, hipStream_t stream);

/* ---------------------------------------------------------------- fused multi-head attention
 * Flash-style fwd/bwd (scores stay on chip) for fairseq MultiheadAttention in the encoder
 * (self, key padding), decoder (causal self + target padding) and decoder cross attention
 * (encoder padding): softmax(scale * q k^T + masks) -> dropout(p) -> @ v, per (b, h).
 * Element (b, h, t, d) of X lives at X[b*sXb + t*ldX + h*hd + d] (sXb = 0 -> T*ldX).
 * Padding: keys j >= key_len[b] masked (key_len may be null).  head_dim in {64, 96, 128}.
 * lse[z*Tq + t] (z = b*H + h) receives the row log-sum-exp for the backward pass.          */
typedef struct mms2ut_attn_args {
  const mms2ut_half* q;
  const mms2ut_half* k;
  const mms2ut_half* v;
  mms2ut_half* o;
  int64_t ldq, ldk, ldv, ldo;
  int64_t sqb, skb, svb, sob;
  int B, H, Tq, Tk, hd;
  const int32_t* key_len;
  int causal;
  float scale;
  float p;
  uint64_t seed, offset;
  float* lse;
} mms2ut_attn_args;

int mms2ut_mha_varlen_fwd(const mms2ut_attn_args* args, hipStream_t stream);
/* dq/dk/dv written (not accumulated); Dd: fp32 workspace [B*H*Tq]                          */
int mms2ut_mha_varlen_bwd(const mms2ut_attn_args* args, const mms2ut_half* dout, int64_t lddo,
                          int64_t sdob, float* Dd, mms2ut_half* dq, int64_t lddq, int64_t sdqb,
                          mms2ut_half* dk, int64_t lddk, int64_t sdkb, mms2ut_half* dv,
                          int64_t lddv, int64_t sdvb, hipStream_t stream);

/* Launch plans: the decisions the two launchers above take for these arguments (the launchers call
 * the same code), without launching anything.  Same argument checks and errors as the launchers.
 *   forward:  nw = waves per block (8 or 16; a block owns 16*nw query rows), short_k = 1 when the
 *             head's whole K / V is staged in LDS up front (Tk <= 128), grid_x * grid_y blocks.
 *   backward: fused = 1 for the one-launch persistent kernel (nkc = key chunks of 128, 1 or 2;
 *             kv16 = 16-byte dK / dV stores; grid = blocks, rounds = ceil(B*H / grid) heads per
 *             block at most), else the three-kernel route (rows_prep = 1: the D = rowsum(dO*O)
 *             kernel that reads whole token rows, 0: the one-wave-per-(head, row) kernel).
 *             Fields of the route not taken are 0.                                            */
typedef struct mms2ut_attn_fwd_plan {
  int nw, short_k, grid_x, grid_y;
} mms2ut_attn_fwd_plan;
typedef struct mms2ut_attn_bwd_plan {
  int fused, nkc, kv16, rows_prep, grid, rounds;
} mms2ut_attn_bwd_plan;
int mms2ut_mha_varlen_fwd_plan(const mms2ut_attn_args* args, mms2ut_attn_fwd_plan* plan);
int mms2ut_mha_varlen_bwd_plan(const mms2ut_attn_args* args, const mms2ut_half* dout, int64_t lddo,
                               int64_t sdob, float* Dd, mms2ut_half* dq, int64_t lddq, int64_t sdqb,
                               mms2ut_half* dk, int64_t lddk, int64_t sdkb, mms2ut_half* dv,
                               int64_t lddv, int64_t sdvb, mms2ut_attn_bwd_plan* plan);

/* ---------------------------------------------------------------- elementwise / embedding */
/* y = dropout(x) elementwise (n elements, counter offset) ; y may alias x                   */
int mms2ut_dropout_fwd(const mms2ut_half* x, mms2ut_half* y, int64_t n, float p, uint64_t seed,
                       uint64_t offset, hipStream_t stream);
/* materialise the keep-mask (uint8) the kernels use — for parity tests / debugging          */
int mms2ut_dropout_mask(uint8_t* keep, int64_t n, float p, uint64_t seed, uint64_t offset,
                        hipStream_t stream);
/* encoder input: x[b,t,:] = dropout(scale*h[b,t,:] + pos[t+2 if t<len[b] else 1, :])
 * (fairseq S2TTransformerEncoder._forward: embed_scale, SinusoidalPositionalEmbedding(pad mask)) */
int mms2ut_encoder_embed_fwd(const mms2ut_half* h, const mms2ut_half* pos_table, const int32_t* len,
                             mms2ut_half* x, int B, int T, int D, float scale, float p,
                             uint64_t seed, uint64_t offset, hipStream_t stream);
/* backward of the above w.r.t. h: dh = scale * dropout_mask * dx                             */
int mms2ut_scale_dropout_bwd(const mms2ut_half* dx, mms2ut_half* dh, int64_t n, float scale,
                             float p, uint64_t seed, uint64_t offset, hipStream_t stream);
/* decoder input (fairseq TransformerDecoder.extract_features, StackedEmbedding n=1):
 * x = dropout(scale*E[tok] + pos[make_positions(tok)])                                      */
int mms2ut_token_embed_fwd(const int64_t* tok, const mms2ut_half* E, const mms2ut_half* pos_table,
                           mms2ut_half* x, int B, int T, int D, int pad_idx, float scale, float p,
                           uint64_t seed, uint64_t offset, hipStream_t stream);
/* dE[tok] += scale*mask*dx (fp32 accumulation buffer dE32 [V][D], D <= 1024; pad rows skipped).
 * Deterministic: one block per vocabulary row sums its positions in ascending order (no float
 * atomics), so the tied-embedding gradient is bit-reproducible.  Every block scans all B*T token
 * ids (O(V * B*T) id reads, ~0.05 ms at the unit vocabulary V = 1004): sized for unit / character
 * vocabularies, not for 10^4+ word vocabularies.                                              */
int mms2ut_token_embed_bwd(const int64_t* tok, const mms2ut_half* dx, float* dE32, int B, int T,
                           int D, int V, int pad_idx, float scale, float p, uint64_t seed,
                           uint64_t offset, hipStream_t stream);
/* out(fp16) = a(fp16) + b32(fp32) elementwise                                                */
int mms2ut_add_f32_to_f16(const mms2ut_half* a, const float* b, mms2ut_half* out, int64_t n,
                          hipStream_t stream);
/* GLU over the channel (last) dim: y[r, c] = x[r, c] * sigmoid(x[r, c + C]), x row stride 2C */
int mms2ut_glu_fwd(const mms2ut_half* x, mms2ut_half* y, int64_t rows, int C, hipStream_t stream);
int mms2ut_glu_bwd(const mms2ut_half* x, const mms2ut_half* dy, mms2ut_half* dx, int64_t rows,
                   int C, hipStream_t stream);
/* Conv1d (stride 2, pad k/2) as implicit GEMM: im2col of x[B][Tin][C] -> col[B*Tout][C*k]
 * ordered (c, k) to match the PyTorch weight [out][C][k] (fairseq Conv1dSubsampler)          */
int mms2ut_im2col(const mms2ut_half* x, mms2ut_half* col, int B, int Tin, int Tout, int C, int k,
                  int stride, int pad, hipStream_t stream);
/* im2col with a row stride ldcol >= C*k; columns [C*k, ldcol) are zero (K padded to whole GEMM
 * k-tiles: the first conv's C*k = 80*5 = 400 -> 448)                                          */
int mms2ut_im2col_ld(const mms2ut_half* x, mms2ut_half* col, int B, int Tin, int Tout, int C, int k,
                     int stride, int pad, int ldcol, hipStream_t stream);
int mms2ut_col2im(const mms2ut_half* dcol, mms2ut_half* dx, int B, int Tin, int Tout, int C, int k,
                  int stride, int pad, hipStream_t stream);
/* fusion gate backward (mm_s2s_transformer.py:613-618):
 * dpre = dres*(o-t)*g*(1-g); dmerge_direct = [dres*g, dres*(1-g)]                            */
int mms2ut_gate_bwd(const mms2ut_half* dres, const mms2ut_half* merge, const mms2ut_half* g,
                    mms2ut_half* dpre, mms2ut_half* dmerge, int64_t rows, int D,
                    hipStream_t stream);
/* copy rows with strides (cols fp16 elements)                                               */
int mms2ut_copy2d(const mms2ut_half* src, int64_t lds, mms2ut_half* dst, int64_t ldd, int64_t rows,
                  int cols, hipStream_t stream);
/* copy2d, and columns [cols, cols + zcols) of every dst row set to zero in the same launch
 * (src may be NULL with cols = 0: a strided zero fill) — the zero-padded weight / key layouts of
 * the subsampler and the fusion without a separate memset                                     */
int mms2ut_copy2d_pad(const mms2ut_half* src, int64_t lds, mms2ut_half* dst, int64_t ldd, int64_t rows,
                      int cols, int zcols, hipStream_t stream);
/* out = a + b (fp16) */
int mms2ut_add_f16(const mms2ut_half* a, const mms2ut_half* b, mms2ut_half* out, int64_t n,
                   hipStream_t stream);

/* ---------------------------------------------------------------- label-smoothed CE
 * fairseq speech_to_unit -> LabelSmoothedCrossEntropyCriterion.compute_loss (reference copy
 * criterions/speech_to_speech_criterion.py:58-102): fp32 log_softmax over V, eps-smoothing,
 * pad targets ignored, reduce=sum.  loss_out[2] += {loss, nll} (fp32; per-block partials in
 * part[2 * MMS_LS_XENT_PARTS] summed in a fixed order: bit-reproducible).  lse[rows] saved for
 * the backward.                                                                              */
#define MMS_LS_XENT_PARTS 512
int mms2ut_ls_xent_fwd(const mms2ut_half* logits, int64_t ld, const int64_t* target, int64_t rows,
                       int V, float eps, int pad_idx, float* lse, float* part, float* loss_out,
                       hipStream_t stream);
/* the same, for a trainer's step log: acc[0..1] += {loss, nll} (may be NULL) and call_out[0..1] =
 * this call's {loss, nll} (written, may be NULL) — no zeroed accumulator and no copies        */
int mms2ut_ls_xent_fwd_log(const mms2ut_half* logits, int64_t ld, const int64_t* target, int64_t rows,
                           int V, float eps, int pad_idx, float* lse, float* part, float* acc, float* call_out,
                           hipStream_t stream);
/* validation scoring, forward only (no lse, no gradient): for every row whose target is not
 * pad_idx, mms2ut_ls_xent_fwd's fp32 loss / nll and the argmax over columns [0, V) (ties to the
 * lowest column).  stats[4] (fp64, device) += {loss, nll, ntokens, n_correct}: it accumulates
 * over calls, the caller zeroes it once per split.  Sums are formed in fp64 from the per-row fp32
 * values, counts are exact integers; block partials in part[4 * MMS_LS_XENT_PARTS] (fp64) are
 * summed in a fixed order (bit-reproducible).  logits 8-byte aligned, ld % 4 == 0, ld >= V.      */
int mms2ut_ls_xent_eval(const mms2ut_half* logits, int64_t ld, const int64_t* target, int64_t rows,
                        int V, float eps, int pad_idx, double* part, double* stats, hipStream_t stream);
/* dlogits = grad * ((1-eps-eps_i)(p - onehot) + eps_i(V p - 1)), 0 on pad rows; in place OK */
int mms2ut_ls_xent_bwd(const mms2ut_half* logits, int64_t ld, const int64_t* target, int64_t rows,
                       int V, float eps, int pad_idx, const float* lse, const float* grad,
                       mms2ut_half* dlogits, hipStream_t stream);
/* R-Drop (fairseq RdropLabelSmoothedCrossEntropyCriterion, --rdrop-alpha; the reference's
 * criterions/speech_to_speech_criterion.py:46-56, :70-76): logits [rows = 2R, ld] hold two dropout
 * passes over the same R targets (row r and row r + R), target[R] are the first half's.  One wave
 * per pair.  kl = 1/2 sum over non-pad pairs of sum_v (p_v - q_v)(log p_v - log q_v)
 * (compute_kl_loss), loss = the label-smoothed CE over all 2R rows + alpha * kl.  lse[rows] as
 * mms2ut_ls_xent_fwd writes it for non-pad rows (bit-identical), 0 for pad pairs (their logits are
 * not read).  Block partials of {loss, nll, kl} in part[3 * MMS_LS_XENT_PARTS], summed in a fixed
 * order: acc[0..1] += {loss, nll}, acc_kl[0] += kl, call_out[0..2] = {loss, nll, kl} (each may be
 * NULL, not all).  rows even, ld % 4 == 0, ld >= V, 2 <= V <= 4096, logits 8-byte aligned.      */
int mms2ut_ls_xent_rdrop_fwd(const mms2ut_half* logits, int64_t ld, const int64_t* target, int64_t rows,
                             int V, float eps, int pad_idx, float alpha, float* lse, float* part,
                             float* acc, float* acc_kl, float* call_out, hipStream_t stream);
/* dlogits = grad * [(p - y_smooth) + alpha * dkl/dz] for both rows of every pair, 0 on pad pairs
 * and on the pad columns [V, ld); in place OK.  The KL sums are recomputed from lse.            */
int mms2ut_ls_xent_rdrop_bwd(const mms2ut_half* logits, int64_t ld, const int64_t* target, int64_t rows,
                             int V, float eps, int pad_idx, float alpha, const float* lse,
                             const float* grad, mms2ut_half* dlogits, hipStream_t stream);

/* ---------------------------------------------------------------- FP16Optimizer + Adam
 * fairseq FP16Optimizer (fp32 master, dynamic loss scale) + clip_grad_norm_ + Adam (fairseq
 * optim/adam.py) + DynamicLossScaler, entirely device-side (no host sync per step).
 * `ost` is a device fp32 state vector (indices MMS_OST_*), initialised by the host once
 * (loss_scale = --fp16-init-scale, iter = 0, last_overflow = -1, step = 0).
 *   grad_sqnorm -> grad_norm_finalize (mult = 1/(loss_scale*sample_size), norm, overflow)
 *   -> optim_prepare (Adam step/step size, clip coef, scaler update) -> adam (skips on overflow) */
enum {
  MMS_OST_MULT = 0, MMS_OST_GNORM = 1, MMS_OST_OVERFLOW = 2, MMS_OST_STEP = 3,
  MMS_OST_STEP_SIZE = 4, MMS_OST_LOSS_SCALE = 5, MMS_OST_ITER = 6, MMS_OST_LAST_OVERFLOW = 7,
  MMS_OST_LAST_RESCALE = 8, MMS_OST_CLIP_COEF = 9, MMS_OST_FATAL = 10, MMS_OST_LR = 11,
  MMS_OST_INCONSISTENT = 12, MMS_OST_SIZE = 16
};
int mms2ut_grad_sqnorm(const mms2ut_half* grad, int64_t n, float* part, int nparts,
                       hipStream_t stream);
int mms2ut_grad_norm_finalize(const float* part, int nparts, float* ost, const float* sample_size,
                              hipStream_t stream);
/* lr = fairseq inverse_sqrt(lr, warmup_init_lr, warmup_updates) evaluated on device at the count of
 * completed (non-overflow) updates, stored in ost[MMS_OST_LR] for adam. */
int mms2ut_optim_prepare(float* ost, float lr, float warmup_init_lr, float warmup_updates, float beta1,
                         float beta2, float clip_norm, float scale_window, float min_loss_scale,
                         hipStream_t stream);
/* CTC loss of a multitask CTC head (fairseq CtcCriterion: F.ctc_loss on log_softmax(logits.float()),
 * reduction "sum").  logits: fp16 batch-major rows b*T + t, leading dim ld >= V; targets int64
 * [B, tgt_ld] (first tgt_len[b] used, max_tgt_len = max tgt_len); in_len / tgt_len int32 [B];
 * work: fp32 scratch of mms2ut_ctc_workspace_floats(B, T, max_tgt_len) elements, kept from fwd to
 * bwd.  fwd ADDS the summed loss to *loss_sum (zero_infinity: infinite per-utterance losses count
 * 0).  bwd writes dlogits (ldd >= V, padded rows/columns 0) = grad_scale[0] * d loss / d logits;
 * impossible alignments get a zero gradient.                                                     */
int mms2ut_ctc_workspace_floats(int B, int T, int max_tgt_len, int64_t* n);
int mms2ut_ctc_loss_fwd(const mms2ut_half* logits, int64_t ld, int B, int T, int V, const int64_t* targets,
                        int64_t tgt_ld, int max_tgt_len, const int* in_len, const int* tgt_len, int blank,
                        int zero_infinity, float* work, float* loss_sum, hipStream_t stream);
int mms2ut_ctc_loss_bwd(const mms2ut_half* logits, int64_t ld, int B, int T, int V, const int64_t* targets,
                        int64_t tgt_ld, int max_tgt_len, const int* in_len, const int* tgt_len, int blank,
                        const float* work, const float* grad_scale, mms2ut_half* dlogits, int64_t ldd,
                        hipStream_t stream);
/* fairseq Trainer._check_grad_norms on device.  stage 0: buf[0..world) = 0 except
 * buf[rank] = ost[MMS_OST_GNORM]; the caller SUM-all-reduces buf; stage 1: ost[MMS_OST_INCONSISTENT]
 * = 1 when the norms are finite and max|n_r - n_0| / (n_0 + 1e-6) >= 1e-6 (sticky: never cleared)
 * — optim_prepare then sets MMS_OST_FATAL, which is sticky as well: from that step on no rank
 * updates anything (the host raises FloatingPointError on every rank at its next check).        */
int mms2ut_grad_norm_check(float* buf, int world, int rank, float* ost, int stage, hipStream_t stream);
/* x *= alpha in place (fp16, n % 8 == 0): the data-parallel gradient pre-division by world size
 * (torch DDP's allreduce hook divides each bucket before its SUM all-reduce)                    */
int mms2ut_scale_f16(mms2ut_half* x, int64_t n, float alpha, hipStream_t stream);
/* dst[0..n) = vals[0..n) (fp32, n <= 8; vals is a host array read at the call, passed to the
 * kernel as arguments): the trainer's per-step log vector (loss / nll / ntokens / nsentences /
 * sample size) initialised in one launch instead of a fill per slot                          */
int mms2ut_set_f32(float* dst, int n, const float* vals, hipStream_t stream);
/* acc (fp32) += x (fp16), n % 8 == 0: gradient accumulation over --update-freq micro-batches    */
int mms2ut_accum_f16_f32(float* acc, const mms2ut_half* x, int64_t n, hipStream_t stream);
int mms2ut_adam_fp16_master(mms2ut_half* param, const mms2ut_half* grad, float* master,
                            float* exp_avg, float* exp_avg_sq, int64_t n, const float* ost,
                            float beta1, float beta2, float eps, float weight_decay, hipStream_t stream);

/* ---------------------------------------------------------------- beam-search decoding
 * fairseq SequenceGenerator._generate (fairseq-generate --beam 10 --max-len-a 1, SURVEY §8f row 2;
 * scripts/textless/2_inference.sh:34-44).  log_softmax_step: log_softmax(logits.float()) of each
 * hypothesis row (get_normalized_probs) fused with the step's masking: NaN -> -inf, pad -> -inf,
 * mode 1 (step >= max_len): every token but eos -> -inf, mode 2 (step < min_len): eos -> -inf.
 * lprobs [rows][V] fp32.                                                                    */
int mms2ut_log_softmax_step(const mms2ut_half* logits, int64_t ld, int64_t rows, int V, int pad_idx,
                            int eos_idx, int mode, float* lprobs, hipStream_t stream);
/* The same step with fairseq-generate's --temperature and --unkpen: the logit is
 * fp16(float(logits) / temperature) (fairseq divides the decoder output in its own dtype before the
 * float cast), and unk_penalty is subtracted from lprobs[:, unk_idx] after the pad mask and before
 * the eos masks.  temperature > 0.  temperature == 1 and unk_penalty == 0 run
 * mms2ut_log_softmax_step's kernel: nothing is rounded twice.                                  */
int mms2ut_log_softmax_step_ext(const mms2ut_half* logits, int64_t ld, int64_t rows, int V, int pad_idx,
                                int eos_idx, int unk_idx, int mode, float temperature, float unk_penalty,
                                float* lprobs, hipStream_t stream);
/* --no-repeat-ngram-size n (fairseq NGramRepeatBlock), one launch per step: for every row r of
 * tokens [rows][ldt] int64 (history h[0..step], position 0 is </s>) and every start i in
 * [0, step+1-n] with h[i .. i+n-2] == h[step+2-n .. step], lprobs[r][h[i+n-1]] = -inf; nothing
 * else is written, and nothing at all while step + 1 < n.  lprobs [rows][V] fp32.  It runs after
 * the eos masks, so it may ban </s> at a forced-eos step, and n = 1 bans every token of the
 * history including position 0's </s>.  1 <= n <= 64, step < ldt.                              */
int mms2ut_ngram_block(const int64_t* tokens, int64_t ldt, int64_t rows, int step, int n, float* lprobs, int V,
                       hipStream_t stream);
/* fairseq Sampling.step: draw o = b*beam + slot (b < bsz, slot < beam) samples one token from row
 * o of lprobs [bsz*beam][V] (from row b*beam when first_step).  Kept set: the whole row in
 * vocabulary order; with topk > 0 the topk best; with topp > 0 the prefix of the descending order
 * up to and including the first running sum of expf(lprob) that reaches topp (sorted orders break
 * ties to the lower index).  With C_j the fp32 running sum over the kept set, the draw is the
 * smallest j with C_j > u * C_last, u = (h >> 8) * 2^-24, h the 32-bit hash of csrc/common.h
 * (mms_hash's h) for the counter pair c = ids[b] * 2^32 + step * 2^8 + slot under `seed`.
 * Outputs [bsz*beam]: out_lprob the row's lprob of the token, out_score = that + prev_scores
 * [o * ld_prev] (no addend when first_step), out_tok, out_beam = slot, out_kept the kept count.
 * V <= 4096, beam <= 256; topk and topp exclude each other.                                   */
int mms2ut_sample_step(const float* lprobs, const float* prev_scores, int64_t ld_prev, const int64_t* ids,
                       int bsz, int beam, int V, int step, int first_step, uint64_t seed, int topk, float topp,
                       float* out_score, float* out_lprob, int64_t* out_tok, int64_t* out_beam,
                       int32_t* out_kept, hipStream_t stream);
/* One step of decoder self-attention against the K|V cache of one layer,
 * cache [slots][maxT][width = 2*H*hd] (K in columns [0, H*hd), V in [H*hd, 2*H*hd)), addressed
 * through slot [N][maxT] int32: key/value row t (t < T) of hypothesis n is row t of cache slot
 * slot[n][t] (beam reorders permute the table, not the cache).  T = *step + 1 is read on the
 * device (the step replays as a graph); row T-1 is this step's K|V, read from kv_new [N][ld_new]
 * and stored into row T-1 of slot n (slot[n][T-1] = n).  q [N][ldq] (head h at column h*hd),
 * out [N][ldo] fp16; softmax(scale q k^T) v per head in fp32.                                 */
int mms2ut_decode_self_attn(const mms2ut_half* q, int64_t ldq, mms2ut_half* cache, int32_t* slot, int N, int H,
                            int hd, int maxT, const int32_t* step, const mms2ut_half* kv_new, int64_t ld_new,
                            int64_t width, mms2ut_half* out, int64_t ldo, float scale, hipStream_t stream);
/* fairseq TransformerDecoder incremental embedding: x[n] = scale*E[tok[n]] + pos[pad+1+*step]
 * (E [V][D], pos sinusoid table [>= pad+2+step][D], fp16; step on the device).             */
int mms2ut_decode_embed(const int64_t* tok, const mms2ut_half* E, const mms2ut_half* pos, const int32_t* step,
                        int pad_idx, mms2ut_half* x, int N, int D, float scale, hipStream_t stream);
/* Decoder-step split-K epilogue: out[rows][cols] (fp16, row stride ldo) = act(sum of nsplit fp32
 * slabs [rows][cols] (slab elements apart) + bias) (+ aux, row stride ldaux); act = ReLU if relu.
 * bias / aux may be null.                                                                      */
int mms2ut_splitk_epilogue_f16(const float* slabs, int nsplit, int64_t slab, int rows, int cols,
                               const mms2ut_half* bias, const mms2ut_half* aux, int64_t ldaux, int relu,
                               mms2ut_half* out, int64_t ldo, hipStream_t stream);
/* The same reduction with the residual (aux required) followed by the next LayerNorm:
 * xout = fp16(fp16(sum of slabs + bias) + aux), y = LN(xout; gamma, beta, eps) — one launch,
 * bit-identical to mms2ut_splitk_epilogue_f16 + mms2ut_layernorm_fwd.  cols <= 1024.          */
int mms2ut_splitk_epilogue_ln_f16(const float* slabs, int nsplit, int64_t slab, int rows, int cols,
                                  const mms2ut_half* bias, const mms2ut_half* aux, int64_t ldaux,
                                  mms2ut_half* xout, int64_t ldx, const mms2ut_half* gamma,
                                  const mms2ut_half* beta, float eps, mms2ut_half* y, int64_t ldy,
                                  hipStream_t stream);
/* BeamSearch.step candidate selection: per sentence b, the top k (<= 32) of
 * lprobs[b*beam + j][v] + prev_scores[(b*beam + j) * ld_prev] over j < beam (j = 0 only when
 * first_step, prev_scores unused), v < V; descending, ties to the lower flat index j*V + v.
 * Outputs [bsz][k]: score (fp32), token v, beam j (int64).  work: bsz*32*k uint64 scratch
 * (two passes: 32 waves per sentence, then a merge).                                          */
int mms2ut_beam_topk(const float* lprobs, const float* prev_scores, int64_t ld_prev, int bsz, int beam, int V,
                     int first_step, int k, float* out_score, int64_t* out_tok, int64_t* out_beam,
                     uint64_t* work, hipStream_t stream);
/* The search bookkeeping around BeamSearch.step (SequenceGenerator._generate); bool tensors are
 * bytes 0/1.  beam_eos_scan: eos_mask [bsz][k] = (cand_tok == eos_idx && cand_score != -inf),
 * cleared where j < beam and ignore [bsz][beam] is set; *count (device int32) = the true entries
 * in columns [0, beam): the hypotheses that finish at this step.  Needs 1 <= beam <= k.        */
int mms2ut_beam_eos_scan(const float* cand_score, const int64_t* cand_tok, const uint8_t* ignore, int bsz,
                         int beam, int k, int eos_idx, uint8_t* eos_mask, int32_t* count, hipStream_t stream);
/* beam_advance: per sentence b, candidate j is masked when eos_mask[b][j] or (j < beam and
 * ignore[b][j]); the beam smallest of masked*2*beam + j, ascending (torch.topk largest=False),
 * become hypotheses r = 0 .. beam-1: active [bsz*beam] = b*beam + cand_beam[b][j] (the parent
 * row, fairseq's reorder_state), new_ignore [bsz][beam] = masked,
 * tok_out[b*beam+r][0..step] = tok_in[parent][0..step], tok_out[..][step+1] = cand_tok[b][j],
 * score_out[b*beam+r][0..step-1] = score_in[parent][0..step-1], score_out[..][step] = cand_score[b][j].
 * Histories are [bsz*beam][ldt] int64 / [bsz*beam][lds] fp32 with step + 2 <= ldt, step + 1 <= lds;
 * the update is out of place (children may share a parent): *_out must differ from *_in, and
 * columns past the ones named are left as they are.  1 <= beam <= k <= 32, cand_beam in [0, beam). */
int mms2ut_beam_advance(const uint8_t* eos_mask, const uint8_t* ignore, const float* cand_score,
                        const int64_t* cand_tok, const int64_t* cand_beam, int bsz, int beam, int k, int step,
                        const int64_t* tok_in, int64_t* tok_out, int64_t ldt, const float* score_in,
                        float* score_out, int64_t lds, uint8_t* new_ignore, int64_t* active, hipStream_t stream);
/* reorder_incremental_state: src [L][Nsrc][maxT][width], dst [L][N][maxT][width] (each decoder
 * layer's self-attention K|V rows); dst[l][n][0:rows] = src[l][idx[n]][0:rows], idx[n] < Nsrc.
 * width % 8 == 0, 16-B aligned.                                                              */
int mms2ut_kv_cache_gather(const mms2ut_half* src, mms2ut_half* dst, const int64_t* idx, int L, int Nsrc,
                           int N, int maxT, int rows, int width, hipStream_t stream);

/* ---------------------------------------------------------------- fbank front end
 * fairseq get_fbank -> torchaudio.compliance.kaldi.fbank (audio_utils.py:326-349), 80 bins,
 * 25 ms / 10 ms, snip_edges, DC removal, pre-emphasis 0.97, povey window, 512-pt FFT, power,
 * mel (mel_banks: [nbins][257] fp32 dense table), log(max(x, FLT_EPS)); then utterance CMVN
 * (data-config feature transform) and zero-padded fp16 collation [B][Tmax][nbins]
 * (_collate_frames).  wave: concatenated fp32 samples (x 2^15), wave_off[B+1].              */
int mms2ut_fbank_frames(const int64_t* wave_off, int B, int32_t* n_frames_out, hipStream_t stream);
/* mel_range[2*m], mel_range[2*m+1]: first / one-past-last nonzero FFT bin of filter m; at most
 * 1024 nonzero weights over all filters (80 Kaldi bins: ~510)                                  */
int mms2ut_fbank_f32(const float* wave, const int64_t* wave_off, const int32_t* frame_off, int B,
                     int total_frames, const float* mel_banks, const int32_t* mel_range, int nbins,
                     float* feats, hipStream_t stream);
/* stats: caller-owned workspace of MMS_CMVN_WS_FLOATS(B, nbins) floats: [B][2][nbins] fp32
 * (per-utterance mean, std), then 8-B aligned fp64 slice partials [B][MMS_CMVN_SPLIT][2][nbins]   */
#define MMS_CMVN_SPLIT 8
#define MMS_CMVN_WS_FLOATS(B, nbins) ((((int64_t)2 * (B) * (nbins) + 1) & ~(int64_t)1) + \
                                      (int64_t)2 * (B) * MMS_CMVN_SPLIT * 2 * (nbins))
int mms2ut_fbank_cmvn_collate(const float* feats, const int32_t* frame_off, int B, int Tmax,
                              int nbins, int cmvn, float* stats, mms2ut_half* out, hipStream_t stream);
/* fairseq SpecAugmentTransform (feature_transforms/specaugment.py, the `specaugment` entry of
 * the data config's `_train` transforms, applied after utterance_cmvn by
 * speech_to_speech_dataset.py:271-272), in place on the collated features x [B][Tmax][nbins].
 * masks[b]: n_freq (f0, width) pairs then n_time (t0, width) pairs, drawn on the host; width 0 =
 * no mask.  use_const = 0: mask value = the utterance's mean over its valid [T][nbins] region
 * (the transform's mask_value=None default); otherwise mask_value.  Time warp is not built.   */
int mms2ut_specaugment_f16(mms2ut_half* x, const int32_t* frame_off, int B, int Tmax, int nbins,
                           const int32_t* masks, int n_freq, int n_time, int use_const,
                           float mask_value, hipStream_t stream);
/* Noise augmentation (--noise-config-yaml): the reference's select_noise + add_noise_v2
 * (audio_utils.py:27-42, :161-233 with noise_waveform_start=-1, add_white_noise=False,
 * normalize=True; called per utterance on the CPU by speech_to_speech_dataset.py:217-240), in
 * place on the wave batch in front of mms2ut_fbank_f32.  bank: the noise clips' int16 samples back
 * to back, bank_off[n_clips + 1].  params: [B][3 + n_mix] int32 rows {apply, start, f, clip ids}:
 * apply 0 leaves the utterance's samples bit-untouched; start is the crop start into the tiled
 * noise (the noise sample of utterance sample t is n[(start + t) mod L], L = the shortest chosen
 * clip); f is the bit pattern of the fp32 factor 1 / (10^(SNR/20) + 1), computed on the host (no
 * pow on the device).  n_mix > 1: the noise is floor(mean of the clips), i.e. -1 where the integer
 * sum of the int16 samples is negative and 0 elsewhere.  With x = wave * 2^-15, every
 * operation rounded to fp32 on its own (no FMA), sums exact in fp64:
 *   clean_amp = sum|x| / T; noise_amp = sum|seg| / T; g = f * clean_amp / (noise_amp + 1e-14);
 *   y = x * (1 - f) + seg * g; wave = y / max(max|y|, 1) * 2^15.
 * Three launches over grid (B, MMS_NOISE_SPLIT), deterministic (no atomics); an utterance's
 * result does not depend on its offset in the batch.  The kernels never read outside a clip for
 * any params row (rows with a clip id out of range or an empty clip are skipped); the caller
 * validates ids, 0 <= start and start + T <= ceil(T / L) * L.
 * ws: caller-owned workspace of MMS_NOISE_WS_DOUBLES(B) doubles.                                */
#define MMS_NOISE_SPLIT    8
#define MMS_NOISE_MAX_MIX  4
#define MMS_NOISE_WS_DOUBLES(B) ((int64_t)3 * (B) * MMS_NOISE_SPLIT)
int mms2ut_noise_mix_f32(float* wave, const int64_t* wave_off, int B,
                         const int16_t* bank, const int64_t* bank_off, int n_clips,
                         const int32_t* params, int n_mix, double* ws, hipStream_t stream);

/* ---------------------------------------------------------------- sample-rate conversion
 * Data preparation (the reference's scripts/preprocess/1_preprocess.ipynb, `ffmpeg -ar 16000`):
 * bandlimited sinc interpolation in the polyphase form of torchaudio.functional.resample.  With
 * o = orig / gcd(orig, new), n = new / gcd, K = 2 width + o taps per phase,
 *   y[j n + i] = sum_{c < K} h[i][c] xp[j o + c],  xp[t] = x[t - width] inside the clip, 0 outside.
 * x: B mono fp32 clips back to back, in_off[B + 1]; clip b of L samples writes ceil(n L / o)
 * outputs at y + out_off[b] (and never more than out_off[b + 1] - out_off[b]); max_out: the
 * longest clip's output count (sizes the grid).  taps: the table tap-major, [K][n] fp32
 * (taps[c n + i] = h[i][c], built on the host in fp64: prepare.resample_taps), K n at most
 * MMS_RESAMPLE_MAX_TAPS (4 MiB, an XCD's L2).  y16 (may be null): the same launch also writes
 * int16 = clip(rint(y), -32768, 32767), manifest.write_wav's rounding, at the same offsets.
 * Taps outside a clip contribute exactly 0 and a neighbouring clip is never read; an output is
 * one chain of K fp32 FMAs in tap order, so a clip's result is bit-identical alone, anywhere in
 * a batch and from run to run.  mms2ut_resample_plan: the output frames (n outputs each) one
 * block owns for this filter, about MMS_RESAMPLE_TILE outputs, fewer where the input window
 * ((frames - 1) o + K floats) would exceed MMS_RESAMPLE_LDS_FLOATS; an error where the table is
 * over the cap or not even MMS_RESAMPLE_R frames fit.                                          */
#define MMS_RESAMPLE_THREADS    256
#define MMS_RESAMPLE_R          4
#define MMS_RESAMPLE_TILE       2048
#define MMS_RESAMPLE_LDS_FLOATS 16384
#define MMS_RESAMPLE_MAX_TAPS   (1 << 20)
int mms2ut_resample_plan(int o, int n, int K, int* tile_frames);
int mms2ut_resample_f32(const float* x, const int64_t* in_off, const int64_t* out_off, int B,
                        int64_t max_out, const float* taps, int o, int n, int width, int K, float* y,
                        int16_t* y16, hipStream_t stream);

/* ---------------------------------------------------------------- unit vocoder (CodeHiFiGAN)
 * Forward-only kernels of fairseq's CodeHiFiGAN generator (csrc/vocoder.hip, vocoder.py).
 * Activations are time-major fp16 rows [T, C]; C is a multiple of 8 and >= 8 everywhere (16-byte
 * rows), anything else is refused.  All accumulation is fp32.
 *
 * mms2ut_conv1d_tm: implicit-GEMM dilated Conv1d (no im2col image; the tile of csrc/conv1d_tm.h,
 * which mms2ut_asr_conv runs too), one launch:
 *   v[q, co]  = bias[co] + sum_{j < taps, ci} in(x[q + j*dil - pad, ci]) * W[co, ci, j]
 *               (rows outside [0, T_in) read as zeros; in = leaky-ReLU(in_slope) if in_act)
 *   v        += res[q, co]                       if res
 *   v         = leaky-ReLU(v, out_slope)         if out_act
 *   y[q, co]  = v | scale * v | y[q, co] + scale * v      (acc = NONE | SET | ADD)
 * w is the weight repacked once at load (vocoder.pack_conv_weight): Cin is cut into slices of
 * MMS_VOC_CIN_CHUNK; a slice of width cw contributes ceil(taps * cw / 32) K-steps, reduction index
 * kk = j * cw + ci zero-padded to the step; the image is [K-step][Cout rounded up to 16][32] fp16,
 * mms2ut_conv1d_tm_packed_halves() elements in all.  (taps - 1) * dil <= MMS_VOC_MAX_SPAN.
 * The polyphase fields (phases, ostride, ooff, nq, w_phase) are for mms2ut_conv_transpose1d_tm;
 * a plain convolution passes phases = ostride = 1, ooff = 0, nq = T_out, w_phase = 0.          */
#define MMS_VOC_CIN_CHUNK 64
#define MMS_VOC_MAX_SPAN  64
enum { MMS_VOC_ACC_NONE = 0, MMS_VOC_ACC_SET = 1, MMS_VOC_ACC_ADD = 2 };
typedef struct {
  const void* x;        /* fp16 [T_in, Cin], row stride ldx */
  int64_t ldx;
  int T_in, Cin;
  const void* w;        /* packed fp16 weight image(s) */
  int64_t w_phase;      /* elements between the images of consecutive phases */
  const float* bias;    /* fp32 [Cout] or NULL */
  void* y;              /* fp16 [T_out, Cout], row stride ldy */
  int64_t ldy;
  int T_out, Cout;
  int taps, dil, pad;
  int nq;               /* output indices q in [0, nq) per phase */
  int phases, ostride, ooff;   /* output row of (q, phase r) = q * ostride + r + ooff */
  int in_act;
  float in_slope;
  const void* res;      /* fp16 [T_out, Cout] or NULL, row stride ldres */
  int64_t ldres;
  int acc;              /* MMS_VOC_ACC_* */
  float scale;
  int out_act;
  float out_slope;
} mms2ut_conv1d_tm_args;
int mms2ut_conv1d_tm_packed_halves(int Cin, int Cout, int taps, int64_t* out);
int mms2ut_conv1d_tm(const mms2ut_conv1d_tm_args* a, hipStream_t stream);
/* ConvTranspose1d(k, stride u, padding p), y[t*u - p + j, co] += in(x[t, ci]) * W[ci, co, j], output
 * length (T - 1) * u - 2p + k, as u polyphase convolutions in one launch of the kernel above: output
 * phase r = (t' + p) mod u is a convolution over ceil(k/u) taps.  w_packed holds u images of
 * mms2ut_conv1d_tm_packed_halves(Cin, Cout, ceil(k/u)) elements each; image r is the packing of
 * Wr[co, ci, m'] = W[ci, co, r + (ceil(k/u) - 1 - m') * u] (0 where that tap is >= k).           */
int mms2ut_conv_transpose1d_tm(const void* x, int64_t ldx, int T, int Cin, const void* w_packed,
                               const float* bias, void* y, int64_t ldy, int Cout, int k, int stride,
                               int padding, int in_act, float in_slope, hipStream_t stream);
/* conv_post + tanh (Cout = 1): y[t] = tanh(bias + sum_{j, ci} lrelu(x[t + j - pad, ci]) * w[j, ci]),
 * w fp32 [taps, Cin], y fp32 [T].                                                               */
int mms2ut_conv_post_tanh(const void* x, int64_t ldx, int T, int Cin, const float* w, float bias,
                          int taps, int pad, float in_slope, float* y, hipStream_t stream);
/* Embedding gather + duration repeat: out[t', :] = dict[codes[src(t')], :] (fp16 [n_embed, D]),
 * src(t') = the first i with cum[i] > t' (cum: inclusive prefix sum of the durations, int64 [T],
 * T_out = cum[T - 1]); cum NULL: src(t') = t' and T_out = T.  A code outside [0, n_embed) yields a
 * zero row.                                                                                     */
int mms2ut_embed_repeat(const void* dict, int n_embed, int D, const int64_t* codes, int T,
                        const int64_t* cum, int64_t T_out, void* out, hipStream_t stream);
/* One layer of fairseq's VariancePredictor in eval mode, fp32 end to end (the rounded durations
 * must match the fp32 reference): h = LayerNorm(ReLU(Conv1d(x; taps, pad))) over [T, Cout],
 * taps = 2 * pad + 1.  x fp32 [n_rows, Cin]; idx (int64 [T]) non-NULL: row t of the input is
 * x[idx[t]] (the embedding lookup), else x has T rows.  w fp32 [taps, Cin, Cout].  proj_w NULL:
 * h is written to out (fp32 [T, Cout]).  proj_w (fp32 [Cout]) non-NULL: the last layer,
 * logd[t] = h[t] . proj_w + proj_b and dur[t] = max(round_half_even(exp(logd[t]) - 1), 1).     */
int mms2ut_var_pred_layer_f32(const float* x, const int64_t* idx, int n_rows, int T, int Cin,
                              const float* w, const float* b, int taps, int pad, int Cout,
                              const float* ln_g, const float* ln_b, float eps, float* out,
                              const float* proj_w, float proj_b, float* logd, int32_t* dur,
                              hipStream_t stream);
/* The whole generator for one utterance in one call (fairseq CodeGenerator.forward without speaker
 * or f0 inputs): embedding gather + duration repeat, conv_pre, per stage the transposed conv and
 * its nk ResBlocks (x = sum_j ResBlock_j(x) / nk), conv_post + tanh -- the launches a caller would
 * issue through the entry points above, in the same order with the same arguments (the result is
 * bit-identical), without a host round trip per launch.  A conv of a ResBlock: kernel k (odd),
 * dilation dil, padding dil (k - 1) / 2.  ups[i]: ConvTranspose1d(k, stride u, padding (k - u) / 2),
 * weights packed as mms2ut_conv_transpose1d_tm wants them; every other weight as mms2ut_conv1d_tm.
 * T_frames: the rows after the duration repeat (cum[T - 1], or T with cum NULL).
 * mms2ut_hifigan_sizes: ws_halves = fp16 elements of the caller-owned workspace, T_wave = the
 * samples written to wave (fp32).  launches (may be NULL) receives the number of kernel launches. */
#define MMS_VOC_MAX_STAGES    8
#define MMS_VOC_MAX_RESBLOCKS 4
#define MMS_VOC_MAX_DILS      4
typedef struct {
  const void* w;        /* packed fp16 */
  const float* b;       /* fp32 [Cout] */
  int k, dil;
} mms2ut_voc_conv;
typedef struct {
  const void* w;
  const float* b;
  int k, u, cout;
} mms2ut_voc_up;
typedef struct {
  const void* dict;     /* fp16 [n_embed, D] */
  int n_embed, D;
  int C0;               /* conv_pre's output channels (upsample_initial_channel) */
  int n_stages, nk;
  int nd[MMS_VOC_MAX_RESBLOCKS];                 /* dilations of ResBlock j */
  mms2ut_voc_conv pre;
  mms2ut_voc_up ups[MMS_VOC_MAX_STAGES];
  mms2ut_voc_conv c1[MMS_VOC_MAX_STAGES][MMS_VOC_MAX_RESBLOCKS][MMS_VOC_MAX_DILS];
  mms2ut_voc_conv c2[MMS_VOC_MAX_STAGES][MMS_VOC_MAX_RESBLOCKS][MMS_VOC_MAX_DILS];
  const float* post_w;  /* fp32 [post_k, C_last] */
  float post_b;
  int post_k;
  float slope, post_slope;                       /* 0.1 and 0.01 in fairseq */
} mms2ut_hifigan;
int mms2ut_hifigan_sizes(const mms2ut_hifigan* m, int64_t T_frames, int64_t* ws_halves, int64_t* T_wave);
int mms2ut_hifigan_fwd(const mms2ut_hifigan* m, const int64_t* codes, int T, const int64_t* cum,
                       int64_t T_frames, void* ws, float* wave, int* launches, hipStream_t stream);

/* ---------------------------------------------------------------- wav2vec2 CTC transcription
 * Forward-only kernels in front of and behind the transformer body of HF Wav2Vec2ForCTC
 * (feat_extract_norm "layer", do_stable_layer_norm) -- csrc/asr.hip, asr.py.  Activations are
 * time-major fp16 rows [T, C] as in the vocoder; all accumulation is fp32.
 *
 * mms2ut_wave_stats: stats[0] = mean, stats[1] = 1 / sqrt(var + eps) of x[0, n) (population variance,
 * the mean squared deviation from the mean), reduced through per-block partial sums in double that
 * every reader folds in the same order (no atomics).  ws: MMS_ASR_STAT_WS_DOUBLES doubles.       */
#define MMS_ASR_STAT_PARTS      64
#define MMS_ASR_STAT_WS_DOUBLES (2 * MMS_ASR_STAT_PARTS)
int mms2ut_wave_stats(const float* x, int64_t n, float eps, double* ws, float* stats, hipStream_t stream);
/* Feature-extractor layer 0 in one launch, T0 = (n - k) / stride + 1 frames:
 *   y[t, c] = GELU(LayerNorm_c(bias[c] + sum_j ((x[t * stride + j] - stats[0]) * stats[1]) * w[j, c]))
 * x fp32 [n]; w fp32 [k, C] (the Conv1d weight [C, 1, k] transposed); bias, ln_g, ln_b fp32 [C];
 * y fp16 [T0, C], row stride ldy; GELU in the erf form.                                           */
#define MMS_ASR_CONV0_MAX_C 512
#define MMS_ASR_CONV0_MAX_K 16
#define MMS_ASR_CONV0_MAX_S 16
int mms2ut_asr_conv0(const float* x, int64_t n, const float* stats, const float* w, const float* bias,
                     const float* ln_g, const float* ln_b, float eps, int k, int stride, int C, void* y,
                     int64_t ldy, hipStream_t stream);
/* Implicit-GEMM Conv1d with a stride and groups (no im2col image; the tile of csrc/conv1d_tm.h,
 * which mms2ut_conv1d_tm runs too), one launch; group g reads the
 * columns [g Cin, (g + 1) Cin) of x and writes the columns [g Cout, (g + 1) Cout) of y:
 *   v[q, co] = bias[co] + sum_{j < taps, ci} x[q * stride + j - pad, ci] * W[co, ci, j]
 *              (rows outside [0, T_in) read as zeros)
 *   y[q, co] = v                          res NULL  (feature-extractor layers 1..)
 *            = GELU(v)                    res NULL and gelu set (HuBERT's extractor layers 1..: no norm)
 *            = res[q, co] + GELU(v)       res given (the positional convolution)
 * w: one image per group in the layout of mms2ut_conv1d_tm (vocoder.pack_conv_weight of the group's
 * [Cout, Cin, taps] weight), w_group elements apart.  127 * stride + taps <= MMS_ASR_CONV_MAX_ROWS;
 * (T_out - 1) * stride + taps <= T_in + 2 pad.                                                    */
#define MMS_ASR_CONV_MAX_ROWS 264
typedef struct {
  const void* x;        /* fp16 [T_in, groups * Cin], row stride ldx */
  int64_t ldx;
  int T_in, Cin;        /* Cin, Cout: per group */
  const void* w;        /* packed fp16 weight images */
  int64_t w_group;      /* elements between the images of consecutive groups */
  const float* bias;    /* fp32 [groups * Cout] or NULL */
  void* y;              /* fp16 [T_out, groups * Cout], row stride ldy */
  int64_t ldy;
  int T_out, Cout;
  int taps, stride, pad, groups;
  const void* res;      /* fp16 [T_out, groups * Cout] or NULL, row stride ldres */
  int64_t ldres;
  int gelu;             /* with res NULL: y = GELU(v), rounded to fp16 once, after the GELU */
} mms2ut_asr_conv_args;
int mms2ut_asr_conv(const mms2ut_asr_conv_args* a, hipStream_t stream);
/* In place over fp16 rows [T, C] (row stride ld): x = GELU(LayerNorm(x; g, b fp32 [C], eps)).     */
#define MMS_ASR_LN_MAX_C 1024
int mms2ut_asr_ln_gelu(void* x, int64_t ld, int T, int C, const float* g, const float* b, float eps,
                       hipStream_t stream);
/* Greedy CTC decoding of B utterances, one block each.  logits fp32 [B, Tmax, ld >= V]; bias (fp32 [V]
 * or NULL) is added in place first (the head's bias).  For utterance b with T = lens[b] frames (Tmax
 * with lens NULL): ids[b, t] = argmax_v logits[b, t, v] (the lowest index on ties); out[b, 0..count[b])
 * = the ids that differ from their predecessor and from `blank`, in order; bad[b] = 1 if any of its
 * T x V logits is not finite, else 0.  ids, out int32 [B, Tmax]; count, bad int32 [B].             */
int mms2ut_ctc_greedy(float* logits, int64_t ld, int V, int B, int Tmax, const int32_t* lens,
                      const float* bias, int blank, int32_t* ids, int32_t* out, int32_t* count,
                      int32_t* bad, hipStream_t stream);

/* ---------------------------------------------------------------- speech-to-unit quantisation
 * HF HubertModel (feat_extract_norm "group", post-LN encoder) features and their nearest k-means
 * centroid -- csrc/units.hip, units.py.  Extractor layers 1.. and the positional convolution are
 * mms2ut_asr_conv (gelu / res), the layers run on the GEMM, LayerNorm and attention kernels.
 *
 * Layer 0, T0 = (n - k) / stride + 1 frames:
 *   v[t, c] = bias[c] + sum_j xn[t * stride + j] * w[j, c],  xn = (x - stats[0]) * stats[1] or x (stats NULL)
 *   y[t, c] = GELU((v[t, c] - mean_c) * rstd_c * gn_g[c] + gn_b[c])
 * mean_c and rstd_c = 1 / sqrt(var_c + eps): the mean and biased variance of v[:, c] over all T0 frames
 * (GroupNorm with one group per channel), from per-slice sums of v and v^2 in double that are added in
 * slice order (no atomics).  bias may be NULL.  ws: MMS_HUBERT_GN_PARTS * C * 2 doubles.  mr fp32
 * [C, 2] receives (mean_c, rstd_c).  w fp32 [k, C]; y fp16 [T0, C], row stride ldy.  Limits as
 * mms2ut_asr_conv0.                                                                                 */
#define MMS_HUBERT_GN_PARTS 256
int mms2ut_hubert_conv0(const float* x, int64_t n, const float* stats, const float* w, const float* bias,
                        const float* gn_g, const float* gn_b, float eps, int k, int stride, int C, double* ws,
                        float* mr, void* y, int64_t ldy, hipStream_t stream);
/* Nearest centroid of fp16 rows X [R, d] (row stride ldx): argmin_c cnorm[c] - 2 x . C_c over c < Kc,
 * the lowest index on ties.  Each centroid is given as two fp16 images of round_up(Kc, 16) rows of d
 * (rows past Kc: anything finite, they take no part): c_hi = fp16(C), c_lo = fp16((C - c_hi) *
 * MMS_KMEANS_LO_SCALE); x . C = x . c_hi + (x . c_lo) / MMS_KMEANS_LO_SCALE, both sums in fp32.
 * d: a multiple of 8.  The centroid axis is cut into chunks of `chunk` (a multiple of 64); chunk ch
 * writes its best (score, index) of row r to pscore / pidx [ch * R + r].  mms2ut_kmeans_chunks gives
 * the chunk the library would choose (chunk 0) or checks a given one, and the number of chunks.
 * mms2ut_kmeans_fold, one block per utterance of a packed batch (R = B * Tmax, T = lens[b] or Tmax
 * frames): code[b, t] = the best index over the chunks in chunk order; merged[b, 0..count[b]) = the
 * codes that differ from their predecessor; bad[b] = 1 if the best score of any of its frames is not
 * finite.  code, merged int32 [B, Tmax]; count, bad int32 [B].                                     */
#define MMS_KMEANS_LO_SCALE 2048
#define MMS_KMEANS_SMALL_BLOCKS 512
int mms2ut_kmeans_chunks(int R, int Kc, int chunk, int* chunk_out, int* nchunks);
int mms2ut_kmeans_assign(const void* X, int64_t ldx, int R, int d, const void* c_hi, const void* c_lo,
                         const float* cnorm, int Kc, int chunk, float* pscore, int32_t* pidx, hipStream_t stream);
int mms2ut_kmeans_fold(const float* pscore, const int32_t* pidx, int nchunks, int B, int Tmax, const int32_t* lens,
                       int32_t* code, int32_t* merged, int32_t* count, int32_t* bad, hipStream_t stream);
/* The top_k nearest centroids (1 <= top_k <= min(MMS_KMEANS_TOPK_MAX, Kc)): mms2ut_kmeans_assign's inputs,
 * chunks and score, with the top_k smallest (score, index) pairs per row ordered by (score, index), so the
 * first is mms2ut_kmeans_assign's choice.  Chunk ch writes its list of row r to pscore / pidx
 * [(ch * R + r) * top_k ...].  mms2ut_kmeans_topk_fold merges the chunks' lists of the frames t < lens[b]
 * (or Tmax) of a packed batch: idx[b, t, 0..top_k) and dist[b, t, j] = sqrt(max(xnorm + score, 0)), the
 * correctly rounded Euclidean distance, xnorm fp32 [B * Tmax] = mms2ut_kmeans_row_norms of X.  Other rows
 * are not written.  bad int32 [B], ZEROED by the caller: set to 1 where a frame has a score, norm or
 * distance that is not finite, or top_k distances that are all 0.                                    */
#define MMS_KMEANS_TOPK_MAX 32
int mms2ut_kmeans_topk(const void* X, int64_t ldx, int R, int d, const void* c_hi, const void* c_lo,
                       const float* cnorm, int Kc, int chunk, int top_k, float* pscore, int32_t* pidx,
                       hipStream_t stream);
int mms2ut_kmeans_topk_fold(const float* pscore, const int32_t* pidx, int nchunks, int B, int Tmax,
                            const int32_t* lens, const float* xnorm, int top_k, int32_t* idx, float* dist,
                            int32_t* bad, hipStream_t stream);
/* Length-penalised beam search over the frames' top_k candidates -- csrc/units_beam.hip, the float32
 * evaluation of the reference's mhubert.py HubertCode.decode(beamsearch=True).  idx int32, dist fp32
 * [B, Tmax, top_k] (mms2ut_kmeans_topk_fold's), T = lens[b] (or Tmax) frames per utterance, one block each.
 * A kept sequence carries (score, runs, last token), at first one empty sequence of score 1.  Frame t's
 * candidate seq * top_k + j appends idx[t, j]; its score is
 *   f32(score + f32(f32(m / T) * f32(dist[t, j] / s)))
 * with m the candidate's run count, m / T formed in double, s the sum of the frame's top_k distances in
 * numpy's pairwise order; every operation rounds on its own.  The beamsize candidates of lowest (score,
 * candidate index) are kept in that order.  beam_code[b, 0..T) = the first kept sequence after the last
 * frame, merged[b, 0..count[b]) = its runs collapsed; bad[b] = 1 where a frame's s is 0 or not finite
 * (the other outputs of b then mean nothing).  ws: mms2ut_units_beam_ws bytes, holding the (parent,
 * token) back-pointers [B, Tmax, beamsize].  Integer and fp32 work only, no atomics: every run gives the
 * same bits.  Limits: 1 <= top_k <= MMS_KMEANS_TOPK_MAX, beamsize >= 1, beamsize * top_k <=
 * MMS_UNITS_BEAM_MAX_CAND.                                                                            */
#define MMS_UNITS_BEAM_MAX_CAND 2048
int mms2ut_units_beam_ws(int B, int Tmax, int beamsize, int64_t* bytes);
int mms2ut_units_beam(const int32_t* idx, const float* dist, int B, int Tmax, const int32_t* lens, int top_k,
                      int beamsize, void* ws, int32_t* beam_code, int32_t* merged, int32_t* count, int32_t* bad,
                      hipStream_t stream);

/* ---------------------------------------------------------------- unit codebook training (k-means)
 * scikit-learn's MiniBatchKMeans.fit on fp16 rows X [N, d] (d a multiple of 8, 16-byte aligned rows) --
 * csrc/kmeans.hip, kmeans.py.  The assignment is mms2ut_kmeans_assign.  No float atomics: every sum has a
 * fixed order and every run gives the same bits.
 *
 * `state` (where an entry takes one; may be NULL outside a fit): MMS_KMEANS_STATE doubles, zeroed before a
 * fit: [0] steps run, [1] the EWA inertia, [2] its minimum, [3] steps without improvement, [4] done.  Once
 * done is set, every kernel that was given the state returns without writing.
 *
 * row_norms: norms[r] = |X_r|^2 (fp32 per lane, the lanes added in double).
 * gather: out[r] = X[idx[r]] (fp16, or fp32 with wide != 0; contiguous rows of d), norms_out[r] =
 *   norms[idx[r]] (both NULL: no norms).  Indices may repeat; one outside [0, N) is clamped.
 * train_fold: code[r] / best[r] = the best (index, score) over the chunks in chunk order of
 *   mms2ut_kmeans_assign's partials (the lowest index wins a tie); partials[b] = the sum over block b's 256
 *   rows of max(xnorm[r] + best[r], 0) in double ((R + 255) / 256 doubles); *inertia (may be NULL with a
 *   state) = their sum in block order; *bad is set to 1 (never cleared) if a best score is not finite.
 *   With a state: MiniBatchKMeans._mini_batch_convergence with tol 0 on inertia / R, smoothing alpha;
 *   max_no_improvement < 0 disables stopping.
 * accumulate: sums[c] = the fp32 sum of the rows of Xb [R, d] whose code is c, added in row order;
 *   cnt[c] = how many.  Nothing of size R x K is formed.
 * update, one launch: where cnt[c] > 0, C[c] = (C[c] * counts[c] + sums[c]) / (counts[c] + cnt[c]) in
 *   double and counts[c] += cnt[c]; then the images of C that mms2ut_kmeans_assign reads (c_hi, c_lo:
 *   round_up(K, 16) rows, rows past K untouched; cnorm summed in double).  sums, cnt, counts NULL: the
 *   images only.  *bad is set to 1 if a centre is not finite or exceeds fp16's range.
 * pp: k-means++ over Xs [n, d] as sklearn's _kmeans_plusplus runs it.  Centre 0 is row `first`; for centre
 *   c >= 1 the T candidates are the searchsorted (clipped to n - 1) of u[(c - 1) * T + t] * potential in the
 *   double inclusive cumulative sum of the closest squared distances; the candidate with the lowest
 *   potential is taken, the lowest t on a tie.  Distances are sum (x - y)^2 in fp32.  chosen int32 [K]: the
 *   rows taken.  u: (K - 1) * T doubles on the device.  Workspaces: closest n floats, dist T * n floats,
 *   partials ((n + MMS_KMEANS_PP_ROWS - 1) / MMS_KMEANS_PP_ROWS) * T doubles, cand T int32.  No host read.
 * step: one mini-batch step over the rows idx int32 [R] of X: gather, assign, train_fold's fold, accumulate,
 *   update, then the stopping rule.  The step that meets the rule keeps its update.                  */
#define MMS_KMEANS_STATE 8
#define MMS_KMEANS_PP_MAX_TRIALS 16
#define MMS_KMEANS_PP_ROWS 16
typedef struct {
  const void* X;          /* fp16 [N, d], row stride ldx */
  int64_t ldx, N;
  const float* norms;     /* [N]: mms2ut_kmeans_row_norms */
  int R, d, K, chunk;     /* batch rows, width, centroids, mms2ut_kmeans_chunks' chunk */
  float* C;               /* fp32 [K, d] centres */
  int64_t* counts;        /* [K] rows each centre has received */
  void *c_hi, *c_lo;      /* fp16 [round_up(K, 16), d] */
  float* cnorm;           /* [K] */
  void* Xb;               /* workspaces: fp16 [R, d] */
  float *xnorm_b, *pscore;/* [R]; [nchunks, R] */
  int32_t *pidx, *code;   /* [nchunks, R]; [R] */
  float* best;            /* [R] */
  double* partials;       /* [(R + 255) / 256] */
  float* sums;            /* [K, d] */
  int32_t *cnt, *bad;     /* [K]; [1] */
  double* state;          /* [MMS_KMEANS_STATE] */
  double alpha;
  int max_no_improvement; /* < 0: never stop early */
} mms2ut_kmeans_step_args;
int mms2ut_kmeans_row_norms(const void* X, int64_t ldx, int64_t R, int d, float* norms, hipStream_t stream);
int mms2ut_kmeans_gather(const void* X, int64_t ldx, int64_t N, const float* norms, const int32_t* idx, int R, int d,
                         void* out, int wide, float* norms_out, const double* state, hipStream_t stream);
int mms2ut_kmeans_train_fold(const float* pscore, const int32_t* pidx, int nchunks, int R, const float* xnorm,
                             int32_t* code, float* best, double* partials, double* inertia, int32_t* bad,
                             double* state, double alpha, int max_no_improvement, hipStream_t stream);
int mms2ut_kmeans_accumulate(const void* Xb, int64_t ldx, const int32_t* code, int R, int d, int K, float* sums,
                             int32_t* cnt, const double* state, hipStream_t stream);
int mms2ut_kmeans_update(float* C, int64_t* counts, const float* sums, const int32_t* cnt, int K, int d, void* c_hi,
                         void* c_lo, float* cnorm, int32_t* bad, const double* state, hipStream_t stream);
int mms2ut_kmeans_pp(const void* Xs, int n, int d, int K, int T, int first, const double* u, float* closest, float* dist,
                     double* partials, int32_t* cand, int32_t* chosen, hipStream_t stream);
int mms2ut_kmeans_step(const mms2ut_kmeans_step_args* args, const int32_t* idx, hipStream_t stream);

/* ---------------------------------------------------------------- image front end (ViT features)
 * timm's eval transform of the vit_*_patch16_384 models on the device: torchvision Resize(S, bicubic) on
 * a PIL image, CenterCrop(S), ToTensor, Normalize, then the patch rows of the patch-embedding GEMM; one
 * launch for the batch.  The resample is Pillow's 8-bit Image.resize(BICUBIC) bit for bit: a horizontal
 * then a vertical pass with int32 coefficients of 22 fractional bits, each pixel
 * clamp((2^21 + sum pix * k) >> 22, 0, 255), the intermediate kept as uint8 (in LDS).
 *   img: the decoded images, packed uint8 HWC (row stride 3 w), image b at byte offset desc[b].src.
 *   tab: int32 tables the host computed in double (vision.py resample_rows), for the cropped S x S
 *     window only.  Per axis of image b: S pairs (first source index, taps) at tab + hb / vb, and S rows
 *     of hn / vn coefficients (taps <= hn used) at tab + hk / vk.  An axis that is not resampled is the
 *     table (i, 1), coefficient 2^22.
 *   norm: fp16 [3][256], the normalised value of every uint8 per channel ((u8 / 255 - mean) / std in
 *     fp32, rounded once).
 *   out: fp16 [B, (S/P)^2, 3 P P], a patch's columns in (c, py, px) order.
 *   max_rows: the most source rows any patch row of the batch reads; max_rows * P * 3 bytes of LDS,
 *     at most MMS_VISION_TILE_BYTES.
 * A descriptor or table offset that does not fit img_bytes / tab_len (int32s) leaves that image's
 * patches unwritten; nothing is read or written out of bounds.                                      */
#define MMS_VISION_TILE_BYTES 49152
#define MMS_VISION_MAX_SIDE   65535
typedef struct mms2ut_image_desc {
  int64_t src;            /* byte offset of pixel (0, 0) in img                                    */
  int32_t w, h;           /* source width and height                                               */
  int32_t hb, hk, hn;     /* horizontal: bounds offset, coefficient offset, coefficients per row   */
  int32_t vb, vk, vn;     /* vertical: the same                                                    */
} mms2ut_image_desc;
int mms2ut_vision_patches(const uint8_t* img, int64_t img_bytes, const mms2ut_image_desc* desc, int B,
                          const int32_t* tab, int64_t tab_len, const mms2ut_half* norm, mms2ut_half* out,
                          int S, int P, int max_rows, hipStream_t stream);
/* bad[b] = 1 where x[b * ld .. b * ld + n) holds an fp16 inf or NaN; other entries are left as they
 * are (the caller zeroes bad).  x 16-byte aligned, ld and n multiples of 8.                          */
int mms2ut_nonfinite_rows_f16(const mms2ut_half* x, int64_t ld, int B, int64_t n, int32_t* bad,
                              hipStream_t stream);

/* ---------------------------------------------------------------- transformer layers
 * One whole pre-LN transformer layer per call — SURVEY §8b "encoder / decoder layer fwd/bwd":
 *   MMS_LAYER_ENC: fairseq TransformerEncoderLayer (encoder_normalize_before; A5, reached from
 *     S2TTransformerEncoder._forward at mm_s2s_transformer.py:464):
 *     x += drop(out_proj(MHA(LN1(x), key_len))); x += drop(fc2(drop(relu(fc1(LN3(x))))))
 *   MMS_LAYER_DEC: fairseq TransformerDecoderLayer (decoder_normalize_before; A10, reached at
 *     mm_s2s_transformer.py:693-696): causal self-attention block (LN1), cross-attention block
 *     (LN2, q_proj, K|V of the encoder output precomputed for all layers, out_proj), FFN (LN3).
 * The kernels are the ones the per-launch entries above run (GEMM epilogues, flash attention,
 * LayerNorm), enqueued in one call: forward on `s`; backward's dgrad chain on `main` and its
 * weight / bias / LayerNorm-parameter gradients on `side` (forked per job; side == main or NULL
 * runs them in order on main).  Dropout: rate and counter offset per site, one seed.
 * Buffers (the library never allocates): the forward writes what the backward needs and the
 * layer output into `saved` (mms2ut_layer_arena: byte offsets per MMS_SLOT_*); the backward writes
 * dx (and dropout(dx) when emit_p > 0) and every temporary into `scratch` (mms2ut_layer_scratch),
 * which the side stream reads — keep it (and `saved`) alive until the side stream is joined.
 * Split-K partials go to the per-stream workspaces sized by mms2ut_layer_ws.               */
enum { MMS_LAYER_ENC = 0, MMS_LAYER_DEC = 1 };
enum {
  MMS_SLOT_M1 = 0, MMS_SLOT_R1, MMS_SLOT_H1, MMS_SLOT_QKV, MMS_SLOT_LSE_SA, MMS_SLOT_O, MMS_SLOT_XA,
  MMS_SLOT_M2, MMS_SLOT_R2, MMS_SLOT_H2, MMS_SLOT_Q, MMS_SLOT_LSE_CA, MMS_SLOT_CO, MMS_SLOT_XB,
  MMS_SLOT_M3, MMS_SLOT_R3, MMS_SLOT_H3, MMS_SLOT_F1, MMS_SLOT_OUT, MMS_LAYER_NSLOT
};

typedef struct mms2ut_layer {
  int kind;                       /* MMS_LAYER_ENC / MMS_LAYER_DEC                               */
  int B, T, Tk, d, H, F;          /* T: the layer's length; Tk: cross-attention keys (decoder)   */
  float eps;
  const int32_t* self_len;        /* [B] self-attention key lengths                              */
  const int32_t* cross_len;       /* [B] decoder: encoder output lengths                         */
  /* parameters ([out, in] row-major fp16) */
  const mms2ut_half *ln1_g, *ln1_b, *w_qkv, *b_qkv, *w_o, *b_o;     /* self-attention block    */
  const mms2ut_half *ln2_g, *ln2_b, *w_cq, *b_cq, *w_co, *b_co;     /* cross-attention block   */
  const mms2ut_half* kv;          /* decoder: K | V of the encoder output [B*Tk] rows, ld_kv     */
  int64_t ld_kv;
  const mms2ut_half *ln3_g, *ln3_b, *w_fc1, *b_fc1, *w_fc2, *b_fc2; /* FFN block               */
  /* W^T images [in, out] of the dgrad weights, or NULL (transposed reads of W) */
  const mms2ut_half *wt_qkv, *wt_o, *wt_cq, *wt_co, *wt_fc1, *wt_fc2;
  /* gradients (views of the flat gradient buffer); g_ln*: [gamma | beta] */
  mms2ut_half *g_ln1, *g_w_qkv, *g_b_qkv, *g_w_o, *g_b_o;
  mms2ut_half *g_ln2, *g_w_cq, *g_b_cq, *g_w_co, *g_b_co;
  mms2ut_half *g_ln3, *g_w_fc1, *g_b_fc1, *g_w_fc2, *g_b_fc2;
  /* dropout: residual / attention-probability / activation rates, counter offsets per site */
  float p_drop, p_attn, p_act;
  uint64_t seed;
  uint64_t off_sa_attn, off_sa_res, off_ca_attn, off_ca_res, off_act, off_ffn_res;
  const mms2ut_half* x;           /* layer input [B*T, d]                                        */
  void* saved;                    /* forward arena; holds the output (MMS_SLOT_OUT)              */
} mms2ut_layer;

typedef struct mms2ut_layer_grad {
  const mms2ut_half* dy;          /* gradient of the layer output [B*T, d]                       */
  const mms2ut_half* dy_drop;     /* dropout(dy) with the FFN residual mask, or NULL             */
  float emit_p;                   /* > 0: also write dropout(dx) (the layer below's residual mask) */
  uint64_t emit_seed, emit_offset;
  mms2ut_half* dkv;               /* decoder: gradient of this layer's K | V columns, ld_dkv     */
  int64_t ld_dkv;
  void* scratch;
  float* main_ws;
  int64_t main_ws_floats;
  float* side_ws;
  int64_t side_ws_floats;
  int side_blocks;                /* grid cap of the grouped weight-gradient launch on the side   */
                                  /* stream (mms2ut_wgrad_group max_blocks; 0 = one per tile)      */
} mms2ut_layer_grad;

/* arena size (and the byte offset of every MMS_SLOT_*, -1 for slots the kind does not use)     */
int mms2ut_layer_arena(const mms2ut_layer* layer, int64_t* offsets, int64_t* bytes);
/* backward scratch size; dx_offsets[0] = dx, [1] = dropout(dx) (-1 unless emit_p > 0)          */
int mms2ut_layer_scratch(const mms2ut_layer* layer, float emit_p, int64_t* dx_offsets, int64_t* bytes);
/* floats of the main-stream (split-K fixup) and side-stream (weight-gradient slabs) workspaces   */
int mms2ut_layer_ws(const mms2ut_layer* layer, int64_t* main_floats, int64_t* side_floats);
int mms2ut_layer_fwd(const mms2ut_layer* layer, float* main_ws, int64_t main_ws_floats, hipStream_t stream);
int mms2ut_layer_bwd(const mms2ut_layer* layer, const mms2ut_layer_grad* grad, hipStream_t main,
                     hipStream_t side);
/* Launches the grouped weight gradients a layer backward held back (mms2ut_layer_bwd launches a
 * layer's group from inside the next layer's backward, behind its self-attention backward; env
 * MMS2UT_WGRAD_DEFER selects the point, 0 = no deferral), on the side stream behind `main`'s work
 * so far.  No-op when nothing is pending.  Call before joining the side stream or reporting a
 * gradient ready point (the host package does both).                                         */
int mms2ut_wgrad_flush(hipStream_t main);

/* ---------------------------------------------------------------- Conv1d subsampler
 * fairseq Conv1dSubsampler — SURVEY §8b mms2ut_conv1d_glu_{fwd,bwd} (A3; S2TTransformerEncoder's
 * front, reached at mm_s2s_transformer.py:464): nlayers x [Conv1d(C_l -> cout_l, k_l, stride 2,
 * padding k_l / 2) -> GLU over channels], input x [B][T][C] fp16 (row b*T + t), output
 * [B][T_out][cout_last / 2] at the arena offset conv1d_glu_arena returns.  One call enqueues the
 * layer sequence (im2col, projection GEMM with bias, GLU); the backward the GLU backward, the
 * weight / bias gradients on `side` (g_w[l] viewed [cout][C k], NULL = skip) and the input
 * gradients of layers > 0 (dgrad through wt[l] = W^T image [C k][cout] when non-NULL, col2im).
 * The first layer's input gradient is not formed (fbank features are not trained).  Buffers as for
 * the layers: arena (forward -> backward), scratch (keep until the side stream is joined),
 * per-stream workspaces from conv1d_glu_ws.                                                     */
#define MMS_CONV_MAX 4
typedef struct mms2ut_conv1d_glu {
  int B, T, C, nlayers;
  int k[MMS_CONV_MAX];            /* kernel sizes                                                */
  int cout[MMS_CONV_MAX];         /* conv output channels (2 x GLU channels), multiples of 16    */
  const mms2ut_half* w[MMS_CONV_MAX];    /* [cout][C_l][k] (nn.Conv1d weight)                   */
  const mms2ut_half* b[MMS_CONV_MAX];
  const mms2ut_half* wt[MMS_CONV_MAX];   /* W^T images [C_l k][cout] for the dgrads, or NULL     */
  mms2ut_half* g_w[MMS_CONV_MAX];
  mms2ut_half* g_b[MMS_CONV_MAX];
  const mms2ut_half* x;
  void* saved;
} mms2ut_conv1d_glu;
int mms2ut_conv1d_glu_arena(const mms2ut_conv1d_glu* c, int64_t* out_offset, int64_t* bytes);
/* dx_offset: the gradient of layer 1's input (= layer 0's GLU output) in the scratch, -1 for one layer */
int mms2ut_conv1d_glu_scratch(const mms2ut_conv1d_glu* c, int64_t* dx_offset, int64_t* bytes);
int mms2ut_conv1d_glu_ws(const mms2ut_conv1d_glu* c, int64_t* main_floats, int64_t* side_floats);
int mms2ut_conv1d_glu_fwd(const mms2ut_conv1d_glu* c, float* main_ws, int64_t main_ws_floats, hipStream_t stream);
int mms2ut_conv1d_glu_bwd(const mms2ut_conv1d_glu* c, const mms2ut_half* dy, void* scratch, float* main_ws,
                          int64_t main_ws_floats, float* side_ws, int64_t side_ws_floats, int side_blocks,
                          hipStream_t main, hipStream_t side);

/* ---------------------------------------------------------------- gated fusion
 * The fusion tail — SURVEY §8b mms2ut_gated_fusion_{fwd,bwd} (A6-A9: fuse_img_feat,
 * mm_s2s_transformer.py:594-622; SelectiveAttention fuse.py:65-117, MultimodalAttention =
 * nn.MultiheadAttention(add_bias_kv) fuse.py:145-167): image LayerNorm (image_pre_norm) +
 * SA_image dropout into a [B][Ti + extra][Di] key layout, SA_text dropout, q = text Wq^T + bq,
 * k|v = img Wkv^T + bkv (extra: + the bias_k|bias_v row per batch), one-head softmax attention
 * (key padding mask [B][>= Tk] uint8, 1 = padded; SA_attention dropout), out-projection, and either
 * the sigmoid gate (gate: merge = [attn_out | text], g = sigmoid(merge Wg^T + bg),
 * out = text + g (attn_out - text)) or the residual out = text + attn_out.  The output lives in
 * the arena (gated_fusion_arena's offset).  The backward writes d(text) (and with want_dimg the
 * image-feature gradient) into the scratch (offsets from gated_fusion_scratch) and the parameter
 * gradients (weight / bias gradients on `side`; g_ln / g_bias_kv are [gamma|beta], [k|v] spans).
 *
 * Two forms of the one-head attention compute the same function (hd = d, nothing non-linear
 * between the k / v projections and the attention products).  The key-side form projects every
 * image row to k|v.  The query-side form moves the projections to the B*Te query rows:
 * S = scale (q W_k) X^T, O = (Pd X) W_v^T, with b_k, b_v and bias_kv as tail columns of
 * [W | b | bias_kv] padded to a multiple of 64.  mms2ut_gated_fusion_route() returns the form a
 * descriptor takes (0 key-side, 1 query-side): the one with fewer GEMM FLOPs, or the one forced by
 * mms2ut_gated_fusion_set_route (-1 by cost, 0, 1; for tests and A/B runs; not to be changed
 * between a forward and its backward).  Arena, scratch and workspace sizes follow the route.     */
int mms2ut_gated_fusion_set_route(int mode);
typedef struct mms2ut_gated_fusion {
  int B, Te, Ti, Di, d;
  int extra;                      /* multimodal_attention (add_bias_kv); 0: selective_attention  */
  int gate;                       /* use_selective_gate                                          */
  int image_pre_norm;
  float eps;
  float p_img, p_txt, p_attn;     /* SA_image / SA_text / SA_attention dropout                  */
  uint64_t seed, off_img, off_txt, off_attn;
  const uint8_t* key_mask;        /* [B][ld_mask], 1 = padded image key, or NULL                 */
  int64_t ld_mask;
  const mms2ut_half *ln_g, *ln_b, *wq, *bq, *wkv, *bkv, *bias_kv, *wo, *bo, *wg, *bg;
  mms2ut_half *g_ln, *g_wq, *g_bq, *g_wkv, *g_bkv, *g_bias_kv, *g_wo, *g_bo, *g_wg, *g_bg;
  const mms2ut_half *wt_q, *wt_kv, *wt_o, *wt_g;   /* W^T images for the dgrads, or NULL        */
  const mms2ut_half* text;        /* [B*Te, d] encoder output                                    */
  const mms2ut_half* img;         /* [B*Ti, Di] image features                                   */
  void* saved;
} mms2ut_gated_fusion;
int mms2ut_gated_fusion_route(const mms2ut_gated_fusion* f);
int mms2ut_gated_fusion_arena(const mms2ut_gated_fusion* f, int64_t* out_offset, int64_t* bytes);
/* offsets[0] = d(text), offsets[1] = d(img) (-1 without want_dimg)                             */
int mms2ut_gated_fusion_scratch(const mms2ut_gated_fusion* f, int want_dimg, int64_t* offsets, int64_t* bytes);
int mms2ut_gated_fusion_ws(const mms2ut_gated_fusion* f, int64_t* main_floats, int64_t* side_floats);
int mms2ut_gated_fusion_fwd(const mms2ut_gated_fusion* f, float* main_ws, int64_t main_ws_floats, hipStream_t stream);
int mms2ut_gated_fusion_bwd(const mms2ut_gated_fusion* f, const mms2ut_half* dres, int want_dimg, void* scratch,
                            float* main_ws, int64_t main_ws_floats, float* side_ws, int64_t side_ws_floats,
                            int side_blocks, hipStream_t main, hipStream_t side);

/* Buffer sizes of a coarse entry in one query: op MMS_OP_LAYER
 * (desc = mms2ut_layer*), MMS_OP_CONV1D_GLU (mms2ut_conv1d_glu*) or MMS_OP_GATED_FUSION
 * (mms2ut_gated_fusion*) -> sizes[0] forward arena bytes, [1] backward scratch bytes (layer: no
 * emitted dropout; fusion: without the image gradient), [2] main-stream and [3] side-stream
 * workspace floats.                                                                             */
enum { MMS_OP_LAYER = 0, MMS_OP_CONV1D_GLU = 1, MMS_OP_GATED_FUSION = 2 };
int mms2ut_workspace_size(int op, const void* desc, int64_t* sizes);

/* ---------------------------------------------------------------- ViT attention rollout
 * What the reference's scripts/extract_feature/vit_rollout.py computes from a hook on timm's
 * attn_drop, without the [H][T][T] probabilities (csrc/rollout.hip).  Everything is fp32 and every
 * run gives the same bits.
 *
 * rollout_probs_f16: out[b][i][j] (row stride T, batch stride out_batch floats) = the mean, max or
 * min over heads h of softmax_j(scale * q[b T + i][h hd ..] . k[b T + j][h hd ..]) -- the packed q|k|v
 * rows mha_varlen_fwd reads (row strides ldq, ldk in elements, multiples of 8), all T keys, no
 * padding.  The mean adds heads 0 .. H - 1 in order and multiplies by 1 / H.  hd: 64, 96 or 128;
 * T <= MMS_ROLLOUT_MAX_T.
 *
 * rollout_discard_f32: in each of nmat contiguous matrices of n non-negative floats, the k smallest
 * become 0, except flat index 0, which is counted among the k but kept.  Among entries equal to the
 * k-th smallest, lower flat indices go first (the order of a stable sort).  Membership is decided on
 * the bit patterns alone.  n <= MMS_ROLLOUT_MAX_T^2, 0 <= k <= n.
 *
 * rollout_chain_f32: a [B][L][T][T], the processed matrices of layers 1 .. L.  Per image: a_l =
 * (F_l + I) / 2, s_i = sum_j a_l[i][j], a_l[i][j] /= s_j (MMS_ROLLOUT_NORM_REFERENCE: the reference's
 * a / a.sum(-1)) or /= s_i (MMS_ROLLOUT_NORM_ROW); R = a_L ... a_1; mask[b][j] = R[0][1 + j] /
 * max_j R[0][1 + j], [B][T - 1]; the sums between the fp32 input and the fp32 mask are carried in
 * double (sums: a workspace of B L T doubles, the s_i of every matrix).  bad[b] = 1 and a zero mask
 * where the maximum is not positive or an entry is not finite.                                  */
#define MMS_ROLLOUT_MAX_T 640
enum { MMS_ROLLOUT_MEAN = 0, MMS_ROLLOUT_MAX = 1, MMS_ROLLOUT_MIN = 2 };
enum { MMS_ROLLOUT_NORM_REFERENCE = 0, MMS_ROLLOUT_NORM_ROW = 1 };
int mms2ut_rollout_probs_f16(const mms2ut_half* q, const mms2ut_half* k, int64_t ldq, int64_t ldk, int B, int H,
                             int T, int hd, float scale, int fusion, float* out, int64_t out_batch,
                             hipStream_t stream);
int mms2ut_rollout_discard_f32(float* x, int nmat, int64_t n, int64_t k, hipStream_t stream);
int mms2ut_rollout_chain_f32(const float* a, int B, int L, int T, int normalization, double* sums, float* mask,
                             int32_t* bad, hipStream_t stream);

/* ---------------------------------------------------------------- scoring of generated sequences
 * The integer kernels behind fairseq-generate's closing BLEU4 / WER line and the reference's
 * scripts/wer.py (csrc/score.hip).  A batch is n_pairs right-padded int32 rows ref [n_pairs][ld_ref] and
 * pred [n_pairs][ld_pred] (row strides in elements, also the longest length a row can hold) with int32
 * lengths per row (clamped to [0, ld]); tokens are arbitrary int32.  One block per pair.  ld_ref, ld_pred
 * <= MMS_SCORE_MAX_LEN: beyond it the call fails and nothing is launched.  n_pairs = 0 is a no-op.
 * Integer arithmetic and integer atomic adds only: every run gives the same bits.
 *
 * ngram_stats: fairseq libbleu's bleu_add for every pair, added into the persistent device
 * stats[10] = {reflen, predlen, match1, count1, match2, count2, match3, count3, match4, count4}.
 * Reference tokens equal to unk (unk < 0: none) become -999; then both sequences are trimmed as libbleu
 * does: right (end = len - 1; while end > 0 and s[end] is eos or pad: end--; len = end + 1), then left
 * (leading pad tokens dropped).  reflen += len(ref), predlen += len(pred); for n = 1 .. 4, where
 * len(pred) >= n: count_n += len(pred) - n + 1, and where also len(ref) >= n: match_n += the sum over
 * distinct n-grams g of min(occurrences in pred, occurrences in ref), n-grams compared by exact token
 * equality (libbleu compares 64-bit FNV hashes of them).
 *
 * edit_distance: the unit-cost Levenshtein distance of every pair over exactly the given lengths (no
 * trimming; the reference's unk becomes -999 as above), written to dist[n_pairs] (NULL: not written)
 * and added into the persistent device totals[2] = {sum of distances, sum of ref lengths}.        */
#define MMS_SCORE_MAX_LEN 4096
int mms2ut_ngram_stats(const int32_t* ref, int64_t ld_ref, const int32_t* ref_len, const int32_t* pred,
                       int64_t ld_pred, const int32_t* pred_len, int n_pairs, int pad, int eos, int unk,
                       int64_t* stats, hipStream_t stream);
int mms2ut_edit_distance(const int32_t* ref, int64_t ld_ref, const int32_t* ref_len, const int32_t* pred,
                         int64_t ld_pred, const int32_t* pred_len, int n_pairs, int unk, int32_t* dist,
                         int64_t* totals, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMS2UT_H */
