/* ctcn.h -- C ABI of libctcn.so: the MI355X (gfx950) CTC acoustic-model hot path.
 *
 * The reference (Diamondfan/CTC_pytorch) has no FFI of its own: its seam is the Python class surface
 * (timit/models/model_ctc.py, timit/utils/ctcDecoder.py, nn.CTCLoss at timit/steps/train_ctc.py:144).
 * Every entry point below replaces one torch op that surface dispatches; the reference call site it
 * replaces is cited per function.  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - plain C: raw device pointers, sizes, a HIP stream passed as void* (hipStream_t); no torch types.
 *   - every function returns int: 0 = OK, <0 = error (CTCN_E*); text via ctcn_last_error() (thread-local).
 *   - the caller owns every buffer (inputs, outputs, reserve, workspace); the library allocates nothing on
 *     the device and keeps no pointer past the call; all work is enqueued on `stream` and the call returns
 *     without synchronising (except where stated).
 *   - all tensors are dense row-major float32 unless stated; "T,B,C" means time-major (t, b, c).
 */
#ifndef CTCN_H
#define CTCN_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CTCN_OK 0
#define CTCN_EINVAL (-1)      /* bad dims / null pointer / misaligned */
#define CTCN_EHIP (-2)        /* HIP runtime error (message carries hipGetErrorString) */
#define CTCN_EUNSUPPORTED (-3)
#define CTCN_EWORKSPACE (-4)  /* workspace too small */

/* reduction of the CTC loss (the values of torch's at::Reduction) */
#define CTCN_REDUCTION_NONE 0
#define CTCN_REDUCTION_MEAN 1
#define CTCN_REDUCTION_SUM 2

#define CTCN_CELL_LSTM 0 /* gate rows i,f,g,o */
#define CTCN_CELL_GRU 1  /* gate rows r,z,n */
#define CTCN_CELL_TANH 2 /* Elman RNN, tanh */

int ctcn_version(void);
const char *ctcn_last_error(void);
/* number of CUs of the current device (host query, used to size grids / workspaces) */
int ctcn_device_cus(void);
/* XCDs of the current device when consecutive workgroup ids are dealt round-robin over them (probed once), else 1 */
int ctcn_device_xcds(void);
/* options: "rnn_persistent" = 1 (default): the recurrence of ctcn_rnn_fwd/bwd runs as ONE persistent launch per layer
 * (W_hh slice resident in VGPRs, h_t handed between workgroups in-launch); 0: one launch per timestep.
 * "handoff" = 1 (default): persistent launches place each (direction, batch-tile) group on one XCD and hand h_t over
 * through that XCD's L2 when the device allows it (falls back to 0 otherwise); 0: device-scope write-through hand-off.
 * "poll_depth" = 2 (default): flag polls kept in flight per polling wave in the XCD-local hand-off (1..4).
 * "bwd_scatter" = 1 (default): the persistent backward recurrence exchanges partial dh tiles (scatter formulation); 0: every
 * workgroup gathers the whole d(pre-activation) tile (rnn_bwd_persist).
 * "handoff_tags" = 1 (default): the scatter formulation hands its partial tiles over WITHOUT flags: every float carries a
 * step tag in its mantissa LSB (cleared again by the consumer: partial sums lose 1 ulp) and the consumer polls the block itself,
 * which removes the producer's store drain and the consumer's flag round trip from the per-step chain; 0: drain + one flag per block.
 * "side_split_wgs" = 8 (default): workgroups per CU launched by the XCD-filtered operand-split kernels of the weight-gradient
 * side stream (1..16; measured at cfg2: 1 -> 20.2, 2 -> 18.0, 4 -> 17.0, 8..16 -> 16.8 ms per step: the side work is nearly critical).
 * "beam_fast" = 1 (default): ctcn_beam_decode uses the restructured search (wave-local top-W extraction, LM in LDS, ln p precomputed
 * by a parallel pre-pass) whenever W <= 60, W*V <= 3328 and V <= 256 (beams wider than 52 prune nothing: slower); 0: always the generic kernel (same results; ~5x slower at W = 20).
 * Wider beams -- the reference's class default is beam_width = 200 (ctcDecoder.py:170) -- always run the generic kernel beam_kernel<NT>, 1 024 threads per
 * utterance beyond W = 64.  Round 5: its selection is a pruning bound (every wave's k-th largest thread maximum by a ballot search on order-preserving
 * keys) + a rank count of the ~W survivors instead of W block-wide arg-max rounds per frame: the cfg5 batch (128 x 800 x 62) at W = 200 takes
 * 11.8 ms (peaky) / 28.1 ms (flat) instead of 657 / 1 556 ms, W = 256 14.2 / 34.8 instead of 1 066 / 2 514 (profiles/r05_wide_beam.txt).
 * "gemm_tile256" = 1 (default): the bf16x3 GEMM multiplies activation-sized products (M >= 1024 rows, enough tiles to fill the
 * device) with 256 x 256 / 256 x 128 workgroup tiles staged by global_load_lds; 0: always the 128 x 128 tile (same results).
 * "gemm_a_inline" = 1 (default): those tiles take a row-major float32 A operand as it is and split it into bf16 planes while staging
 * it (no separate plane pass over A; same planes, same results); 0: A is pre-split like B.
 * "conv_mfma" = 1 (default): ctcn_conv2d_fwd / _bwd run as implicit GEMMs on v_mfma_f32_16x16x4_f32 (im2col tile of 64 positions and
 * the filter matrix staged in LDS; exact float32 in both matmul precisions); 0: the direct (lane-per-position) kernels.
 * "gemm_tn" = 1 (default): bf16x3 products C = A^T B with BOTH operands contraction-major (transA = 1, transB = 0: the weight
 * gradients dW = da^T x; M >= 128, N >= 32, K >= 1024, 16-B aligned rows) run on the TN tile -- float32 rows split into hi / lo while
 * they are staged, ds_read_b64_tr_b16 fragments, split-K queue -- instead of a transposing plane pass + the NT plane tiles; the same
 * bf16x3 operands and products, the k-sums grouped differently (results agree to float32 rounding of the sums).
 * "rnn_fwd_tagged" = 1 (default): forward persistent recurrence as a tagged gather (rnn_fwd_tagged: no flags, no store drain; the
 * h_t dwords carry the step tag and the gathering waves poll the data itself) where it applies -- precision 1, LSTM / GRU, H % 32 == 0,
 * XCD-local placement; 0: the flag + data kernel (rnn_fwd_persist) everywhere.  "tag_poll_delay" = 8: 64-cycle sleeps between the
 * step barrier and a gathering wave's first poll.
 * "edit_wave" = 1 (default): ctcn_edit_distance runs one wavefront per utterance along anti-diagonals (labels up to 512 symbols);
 * 0: one lane per utterance with its DP row in LDS (also the path for longer labels).
 * "gemm_big_tiles" = 0 (default): 1 lets the bf16x3 GEMM use 256x128 / 128x256 workgroup tiles (same results, measured slower).
 * "tn_splits_xcd" = 1 (default, round 5): the TN tile sizes its split-K count for the CUs of the XCDs it may run on (xcd_allow of
 * ctcn_rnn_bwd_weights: one round of items on the idle XCDs next to a recurrence) instead of for the whole device (two rounds of items half
 * as long, each paying a prologue, a 128-KB partial store and its share of the reduce pass): cfg2 13.22 -> 13.15 ms per step; 0: as before.
 * The k-sums are grouped differently (float32 rounding of the sums), deterministically either way.
 * "xcd_interleave" = 1 (default; round 5): which physical XCD hosts group g -- (direction, 16-row batch tile) -- of a persistent recurrence that
 * leaves XCDs idle on a device of eight, and therefore which XCDs its side-stream GEMMs (pipelined projection chunks, weight gradients) get:
 * 0: XCD g; 1: the even XCDs first {0 2 4 6 | 1 3 5 7}; 2: {0 1 4 5 | ..}; 3: {0 3 4 7 | ..}; 4: {0 2 5 7 | ..}; 5: {0 4 1 5 | ..}.  The host
 * derives its xcd_allow masks from the same order (ops._idle_xcd_mask).  Same results whatever the order.  Measured at cfg2 (two runs each):
 * order 0 13.19 / 13.20 ms per step; orders 1, 3, 4 -- ONE recurrence XCD and one GEMM XCD in every pair (2k, 2k + 1) -- 13.04-13.08; orders 2,
 * 5 -- both XCDs of a pair on the same side -- 13.26-13.31; cfg1 / cfg3 / shipped YAML unchanged.  A recurrence that takes EVERY XCD (cfg4:
 * groups = XCDs) keeps group g on XCD g whatever the option says: there is nothing to place.  (The cfg4 trajectory divergence first seen while the
 * order applied to that launch too had nothing to do with placement: round 6 traced it to the parked tiles of rnn_fwd_tagged)
 * "rnn_slow_items" = 0 (parity harness): N > 0 runs the SLOW instantiation of rnn_fwd_tagged, whose item waves sleep N x 64 cycles before they read
 * the parked partial tiles, at every step.  Results must not change (test_rnn_fwd_tagged_with_slow_item_waves): the hand-off inside a workgroup may
 * rest on barriers and buffer parity only, never on which wave is faster.  "rnn_slow_exchange" = N: the same for the exchange waves; both options also select
 * the SLOW instantiations of rnn_bwd_scatter / rnn_bwd_scatter2 (item waves sleep before they read the parked tiles / start their gather, exchange waves
 * behind the barrier before they read the staged operand): test_rnn_bwd_with_slow_waves.
 * "ctc_lattice_skew" = 1 (default): the CTC lattice passes of ctcn_ctc_fwd / ctcn_ctc_fwd_both / ctcn_ctc_fwd_ex run wave-skewed where the lattice
 * has at most 256 states (label rows of up to 127 symbols): one state per lane, neighbour states by DPP wave shifts, the waves a pipeline three
 * four-frame chunks apart that hands its edge states on through a small LDS ring (ctc.hip: ctc_lattices_skew_kernel: one barrier per chunk); 0: the classic kernels
 * (lattice row in LDS, an LDS round trip and a barrier on every frame's chain).  Every stored value is bit-identical either way (test_ctc_lattice_skew.py);
 * longer label rows and ctcn_ctc_bwd's in-place beta pass take the classic kernels whatever the option says.  ctcn_diag_ctc_lattice_plan shows
 * the choice.  "ctc_slow_wave" = 0 (parity harness): a bit per wave (0..15; other values clamp) selects the SLOW instantiation of the skewed
 * kernel, whose named waves sleep 32 x 64 cycles before their ring read and after their ring write in every chunk.  Results must not change:
 * the hand-off rests on the barrier and the ring's depth, never on which wave is faster.
 * "bn_rows4" = 1 (default, round 5): BatchNorm over (rows, C) with C % 4 == 0 forms its column sums with 16-B loads, sixteen row phases per
 * workgroup (colreduce_rows4_kernel, behind the dense and the length-aware entry points alike); 0: the dword kernel (colreduce_rows_kernel).  Same chunks, same element values, float64 partials grouped differently: the float32
 * results agreed bit for bit wherever compared (tools/bn_rows_probe.py).  cfg2 13.33 -> 13.25 ms per step, cfg4 53.2 -> 52.8.
 * "tn_splits_force" = 0 (default; development): n > 0 forces the split-K count of the TN tile (tools/gemm_tn_splits_probe.py: the rule's own
 * choice -- one round of (tile, split) items on the CUs the launch may use -- is where the time is shortest on the cfg2 / cfg4 products).
 * "gemm_bf16_single" = 0 (default): 1 = the opt-in bf16 mode (round 5).  With precision 1 the 256-row GEMM tiles -- every product over the T*B
 * rows of a layer: input projections, dx, weight gradients (plane, float32-A and TN tile) -- multiply the bf16 ROUNDINGS of their operands once
 * (ah*bh, f32 accumulate) instead of the three bf16x3 products (al*bh + ah*bl + ah*bh); the recurrent matmul and the small tiles keep bf16x3.
 * Result = the product of the rounded operands to f32 summation order (tools/gemm_single_probe.py: 2-5e-6 of mean |C|); against the exact product
 * an element moves by up to 1.5e-2 of mean |C|.  BASELINE.json's north_star tolerance ("loss and activations within 1e-3 bf16 tolerance"):
 * full-size cfg2 / cfg3 / cfg4 loss within 1e-5 .. 3e-5 of the REFERENCE's, gradient norms within 6e-4 .. 4e-3, log-probs 2-3e-3 mean (1.8e-2 max)
 * next to the default mode's (test_bf16_single_mode_against_reference_checksums).  Tile time 1.27-1.84x shorter; cfg2 13.21 -> 12.69 ms per
 * step, cfg3 7.71 -> 7.42, cfg4 52.6 -> 45.5.  The default (0) keeps every parity statement of this header (1e-5 against the reference).
 * "gemm_dx_wide" = 1 (default): ctcn_gemm_dx takes its 256 x 320 float32-A tile (gemm_af32_n320pp_kernel) where the tile counts say it wins
 * (the rule at ctcn_gemm_dx below); 0: never (ctcn_gemm_dx is ctcn_gemm(0, 0, ...)); 2: wherever the tile is eligible (tests).  0 and 1 give the same bits.
 * "beam_occ2" = 0 (default, round 5): 1 / 2 launch the fast beam search compiled for eight waves per SIMD (<= 64 VGPRs, 43 spilled dwords)
 * with <= 68 KB of dynamic LDS (4 096-slot trie; 2: LM in global memory, 8 192 slots) so that two utterances share a CU.  Same results;
 * measured SLOWER (cfg5, three searches in flight: 279 k -> 248 k utt/s peaky, 128 k -> 97 k flat; profiles/r05_beam_occ2_ab.txt) and kept
 * as an experiment switch.
 * "beam_generic_threads" = 0 (default): the generic beam kernel runs 256 threads per utterance, 1 024 beyond W = 64 or 3 500 candidates per frame;
 * 256 / 512 / 1024 force one (measurements); a forced count below W is raised to the smallest of the three >= W (one thread per beam slot), so
 * the option never changes a result.
 * "beam_bitonic" = 1 (default): the generic beam kernel ranks up to 256 survivors of its pruning bound (the reference's W = 200 leaves ~1.1 W) by a
 * bitonic sort on waves 0-3 (DPP / v_permlane swaps); 0 = by counting pairs, as it does for more survivors.  Same labellings and scores.
 * "beam_cand_global" = 0 (default): 1 keeps the generic kernel's candidate table in global memory (L2) even where the LDS would hold it; the LM
 * table takes the room.  With "beam_generic_threads" = 512 two searches of the reference-default width then share a CU (116 VGPRs, 77 KB of
 * LDS each).  Same results bit for bit (test_beam_generic_kernel_occupancy_options).  Measured on the kernel as it stood at the start of the
 * round's last session (cfg5, W = 200, profiles/r06_wide_beam_probe.txt): +13 % / +22 % utterances/s (peaky / flat) with twelve searches in
 * flight, -13 % with three, one batch 14 % slower -- an opt-in for offline decoding with many batches in flight, not the default.
 * "conv_dbg" = 0 (default): development only (tools/conv_phase_probe.py) -- conv_mfma_kernel skips its window load (1), MFMA loop (2) and /
 * or output phase (4); results are invalid.
 * "fwd_pipe_any_chunking" = 0 (default): the input projection is pipelined with the forward recurrence (ctcn_rnn_call.side_stream) only
 * when a time-chunk count exists whose chunk pair the side stream digests in one round of 256-row tiles on the idle XCDs (cfg2: 10 chunks
 * of 2 560 rows), with at least 72 steps per chunk, at a flop rate the idle XCDs sustain within the recurrence's time for the chunk, and with
 * eight CUs of every recurrence XCD left free; 1: with the default 8 chunks otherwise too (slower where measured: cfg3 8.51 vs 7.87 ms per
 * step; the parity tests of the pipeline use it).  "fwd_pipe_min_input" = 0: smallest layer input width that is pipelined (experiments).
 * Environment CTCN_LOG_PIPE=1 prints the decision of every ctcn_rnn_fwd_ex call to stderr.
 * "fwd_rsv_lds" = 2 (default): rnn_fwd_tagged moves its reserve traffic through LDS (the items park their values, exchange waves store
 * them with 16-B stores in the pause before their first poll, pre-activations arrive by LDS DMA two steps ahead) for H > 384; 1: wherever the
 * reserves are 16-B aligned; 0: never (scattered dword stores / loads from the item waves).  Same values either way.
 * "bwd_item_gather" = 1 (default): the scatter formulation of the backward recurrence runs as rnn_bwd_scatter2 (item waves gather their own
 * 256-B quarters of the partial tiles, one barrier per step, all reserve traffic on the exchange waves through LDS DMA, 64-bit reserve
 * addresses, up to 40 slices = H <= 640) where it measured faster: more than 20 slices (H > 320); 0: never; 2: wherever it applies.
 * "bwd_poll_delay" = -1 (auto): 64-cycle sleeps before an item wave's first poll of a step in rnn_bwd_scatter2.
 * "rnn_recurrence_only" = 0 (default); 1 is a MEASUREMENT aid: ctcn_rnn_fwd / ctcn_rnn_bwd skip their input-projection
 * and deferred gradient GEMMs so that bench.py can time the recurrent kernel alone -- outputs are not valid. */
int ctcn_set_option(const char *name, int value);
int ctcn_get_option(const char *name);
/* The names ctcn_set_option knows, index 0 .. n-1; NULL past the end.  (Round 6: what a harness needs to snapshot the whole table -- the
 * reference has no counterpart; tests/conftest.py asserts that every GPU test leaves the table as it found it.)
 * "xcd_interleave_force" = 0 (default; development): 1 applies "xcd_interleave" to a recurrence that takes EVERY XCD too (cfg4) -- a
 * relabelling of XCDs with bit-identical results, held to that by test_rnn_results_do_not_depend_on_the_xcd_order. */
const char *ctcn_option_name(int index);
/* optional device int that persistent kernels set to a non-zero code if an in-launch hand-off times out (sticky);
 * the caller zeroes it and reads it at its own synchronisation points.  PROCESS-WIDE default (one word for every call that does not
 * bring its own in ctcn_rnn_call.status): a caller with several models / devices passes per-call words instead. */
int ctcn_set_status_buffer(int *dev_word);

/* ---------------------------------------------------------------------------------------------------
 * GEMM (MFMA, f32 in / f32 accumulate: v_mfma_f32_32x32x2_f32, or bf16x3 split operands: v_mfma_f32_32x32x16_bf16)
 * replaces: nn.Linear (model_ctc.py:137,166) and the input-projection part of nn.LSTM/GRU/RNN
 * (model_ctc.py:33).  C[M,N] = op(A)[M,K] * op(B)[K,N] + beta*C, row-major:
 *   transA==0: A[m*lda+k]   transA!=0: A[k*lda+m]     transB==0: B[k*ldb+n]   transB!=0: B[n*ldb+k]
 * ws/ws_bytes: optional split-K workspace (deterministic two-pass reduce); may be NULL/0.
 * precision: 0 = exact f32 MFMA; 1 = each f32 operand split into bf16 hi + lo planes, three bf16 MFMAs per product
 * (hi*hi + hi*lo + lo*hi), f32 accumulate: ~2^-16 relative operand error instead of bf16's 2^-8. */
int ctcn_gemm(int transA, int transB, int M, int N, int K, const float *A, int lda, const float *B, int ldb,
              float *C, int ldc, float beta, int precision, void *ws, size_t ws_bytes, void *stream);

/* ctcn_gemm_dx: C[M,N] = A[M,K] * B[K,N] + beta*C for a row-major float32 A (k contiguous) and a row-major K x N B: ctcn_gemm(0, 0, ...)
 * with one more tile, 256 x 320, for the dx product of a recurrent layer (dx = da W_ih: N = the layer's input width).  The tile is eligible
 * with precision 1, option "gemm_bf16_single" off, N % 320 == 0, K >= 64, K % 4 == 0, lda % 4 == 0, A 16-byte aligned and a workspace that
 * holds B's bf16 planes; it is taken when ceil(tiles_wide / CUs) * r < ceil(tiles_128 / CUs), tiles_wide = ceil(M / 256) * N / 320,
 * tiles_128 = ceil(M / 256) * ceil(N / 128), r = the measured cost of a wide tile in 256 x 128 tiles (1 < r < 2): fewer rounds of one tile
 * per CU.  Every other call is ctcn_gemm(0, 0, ...) itself.  Where the rule takes the tile ctcn_gemm runs a 256-row tile (more than one
 * tile per CU), which adds the same products in the same k order: bit-identical results.  (Forced by option "gemm_dx_wide" = 2 onto a
 * product small enough for ctcn_gemm to split over K, the tile differs from it by the order of the partial sums.) */
int ctcn_gemm_dx(int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *C, int ldc, float beta, int precision, void *ws,
                 size_t ws_bytes, void *stream);

/* out[b,a,c] = in[a,b,c]  (x.transpose(0,1), model_ctc.py:175) */
int ctcn_transpose01(const float *in, float *out, int A, int B, int C, void *stream);
/* materialise any <=4-D strided view: out contiguous [d0][d1][d2][d3] = in[i0*s0+i1*s1+i2*s2+i3*s3] (element strides);
 * the .contiguous() calls of CTC_Model.forward (model_ctc.py:153,158) */
int ctcn_copy_strided4(const float *in, float *out, int d0, int d1, int d2, int d3, size_t s0, size_t s1, size_t s2,
                       size_t s3, void *stream);
/* nn.ReLU when it is not fused into the BatchNorm apply pass (LayerCNN with batch_norm=False, model_ctc.py:64) */
int ctcn_relu_fwd(const float *x, float *y, size_t n, void *stream);
int ctcn_relu_bwd(const float *y, const float *dy, float *dx, size_t n, void *stream);
/* nn.MaxPool2d(pooling_size) of LayerCNN (model_ctc.py:52-53,64-65): kernel = stride = (kh, kw), no padding, floor; x / dx are
 * `planes` (= B*C) images of Hi x Wi, y / dy / arg of (Hi/kh) x (Wi/kw).  `arg` (one byte per output) keeps the winner's offset
 * ki*kw + kj inside its window for the backward pass (first maximum wins, NaN replaces anything: torch's scan rule). kh*kw <= 256. */
int ctcn_maxpool2d_fwd(const float *x, float *y, unsigned char *arg, size_t planes, int Hi, int Wi, int kh, int kw, void *stream);
int ctcn_maxpool2d_bwd(const float *dy, const unsigned char *arg, float *dx, size_t planes, int Hi, int Wi, int kh, int kw, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Recurrent layer, bias-free, 1 layer, 1 or 2 directions, zero initial state, no packing/masking.
 * replaces: rnn_type(input_size, hidden_size, bidirectional, bias=False)(x)  (model_ctc.py:24-25,33)
 *   x (T,B,I); w_ih[d] (G*H,I); w_hh[d] (G*H,H); y (T,B,dirs*H) = [fwd | rev]
 *   gates  (T,B,dirs,G*H): reserve; fwd leaves the saved activations, bwd overwrites it with d(pre-act)
 *   aux    (T,B,dirs,H)  : reserve; LSTM cell state c / GRU W_hn*h ; unused (may be NULL) for TANH
 * G = 4 (LSTM) / 3 (GRU) / 1 (TANH).  H must be a multiple of 4. */
size_t ctcn_rnn_scratch_bytes(int cell, int B, int H, int dirs);
int ctcn_rnn_fwd(int cell, int T, int B, int I, int H, int dirs, const float *x, const float *w_ih0,
                 const float *w_hh0, const float *w_ih1, const float *w_hh1, float *y, float *gates, float *aux,
                 int precision, void *ws, size_t ws_bytes, void *stream);
/* ctcn_rnn_fwd followed by the layer's inverted dropout (BatchRNN: rnn -> nn.Dropout, timit/models/model_ctc.py:33-34): y as above (the
 * backward pass needs it) and y_drop = ctcn_dropout(y, p, seed, offset), bit for bit.  Where the tagged-gather recurrence applies the
 * dropped values are stored by the recurrence itself (option "rnn_fused_dropout" = 1, the default: Philox in the item waves' idle time,
 * no pass over y afterwards); everywhere else the dropout kernel runs behind the recurrence. */
int ctcn_rnn_fwd_dropout(int cell, int T, int B, int I, int H, int dirs, const float *x, const float *w_ih0, const float *w_hh0,
                         const float *w_ih1, const float *w_hh1, float *y, float *gates, float *aux, float *y_drop, float p, uint64_t seed,
                         uint64_t offset, int precision, void *ws, size_t ws_bytes, void *stream);
/* dy (T,B,dirs*H); dx (T,B,I) or NULL; dw_* same shapes as w_*; beta_w: 0 overwrite / 1 accumulate into dw.
 * scratch: ctcn_rnn_scratch_bytes() bytes (transposed W_hh + carried dh/dc state). */
int ctcn_rnn_bwd(int cell, int T, int B, int I, int H, int dirs, const float *x, const float *w_ih0,
                 const float *w_hh0, const float *w_ih1, const float *w_hh1, const float *y, float *gates,
                 float *aux, const float *dy, float *dx, float *dw_ih0, float *dw_hh0, float *dw_ih1,
                 float *dw_hh1, float beta_w, int precision, void *scratch, void *ws, size_t ws_bytes,
                 void *stream);
/* ctcn_rnn_bwd for a layer whose output went through ctcn_rnn_fwd_dropout: dy is the gradient of the DROPPED output, and the layer sees
 * ctcn_dropout(dy, p, seed, offset) -- bit for bit.  The scatter recurrence applies the keep mask as it consumes dy (option
 * "rnn_fused_dropout"); every other path first runs the dropout kernel into dy_tmp (T*B*dirs*H floats) and reads that. */
int ctcn_rnn_bwd_dropout(int cell, int T, int B, int I, int H, int dirs, const float *x, const float *w_ih0, const float *w_hh0,
                         const float *w_ih1, const float *w_hh1, const float *y, float *gates, float *aux, const float *dy, float *dx,
                         float *dw_ih0, float *dw_hh0, float *dw_ih1, float *dw_hh1, float beta_w, int precision, void *scratch, void *ws,
                         size_t ws_bytes, void *stream, float p, uint64_t seed, uint64_t offset, float *dy_tmp);
/* Per-call extras of the recurrent layer (ctcn_rnn_fwd_ex / ctcn_rnn_bwd_ex).  The library keeps NO state between calls (round 3: the
 * one-shot setters ctcn_set_prelaunch_event / ctcn_set_fwd_overlap and the thread-local hand-over of the _dropout entry points are gone):
 * everything a call needs beyond its tensors is in this struct, owned by the caller, read during the call only.  Zero-initialise it;
 * a NULL pointer = all zero = the plain ctcn_rnn_fwd / ctcn_rnn_bwd.  Two models on two streams (or two host threads) share nothing but
 * the option table (ctcn_set_option: process-wide tuning switches, read-only during calls) and, unless `status` is given, the process
 * default status word. */
typedef struct ctcn_rnn_call {
  /* dropout of the layer output (BatchRNN: rnn -> nn.Dropout, model_ctc.py:33-34).  fwd: y_drop != NULL asks for y_drop =
   * ctcn_dropout(y, drop_p, drop_seed, drop_offset) beside y.  bwd: dy_tmp != NULL says dy is the gradient of the DROPPED output (same
   * p / seed / offset); dy_tmp (T*B*dirs*H floats) is scratch for the paths that run the dropout kernel first. */
  float drop_p;
  uint64_t drop_seed, drop_offset;
  float *y_drop;
  float *dy_tmp;
  /* fwd: pipeline the input projection with the persistent recurrence.  The library projects the first pair of time chunks on the call's
   * stream, records side_event (hipEvent_t) right before the recurrence launch and issues the remaining chunk GEMMs on side_stream behind
   * that event, restricted to the XCDs of xcd_allow (bit x = XCD x: the ones the recurrence leaves idle), each pair followed by a counter
   * update the recurrence checks when it enters a new chunk.  side_ws / side_ws_bytes: workspace of the side-stream GEMMs.  Ignored (whole
   * projection first) where the tagged-gather recurrence does not apply.  The caller joins side_stream before it reuses x or side_ws. */
  void *side_stream, *side_event, *side_ws;
  size_t side_ws_bytes;
  unsigned xcd_allow;
  /* bwd: hipEvent_t recorded on the call's stream immediately before the recurrence is launched, behind the call's own preparatory
   * memsets / transposes; work meant to run next to that recurrence on another stream (ctcn_rnn_bwd_weights of the layer above) waits
   * for it. */
  void *prelaunch_event;
  /* device int32 the persistent kernels of THIS call set on a hand-off timeout (sticky); NULL: the process default of
   * ctcn_set_status_buffer (which may be NULL too: timeouts then only poison the output). */
  int *status;
  /* out (the one field the library writes): where the name of the recurrent kernel THIS call launched is stored (a string literal:
   * "rnn_fwd_tagged", "rnn_fwd_persist", "rnn_fwd_step", "rnn_bwd_scatter2", "rnn_bwd_scatter", "rnn_bwd_persist", "rnn_bwd_step"); NULL: not
   * wanted.  Per call, unlike the process-wide ctcn_rnn_last_kernel (last writer of any thread wins): what the host's batch-chunk decision
   * reads. */
  const char **launched;
} ctcn_rnn_call;
int ctcn_rnn_fwd_ex(int cell, int T, int B, int I, int H, int dirs, const float *x, const float *w_ih0, const float *w_hh0,
                    const float *w_ih1, const float *w_hh1, float *y, float *gates, float *aux, int precision, void *ws, size_t ws_bytes,
                    void *stream, const ctcn_rnn_call *call);
int ctcn_rnn_bwd_ex(int cell, int T, int B, int I, int H, int dirs, const float *x, const float *w_ih0, const float *w_hh0,
                    const float *w_ih1, const float *w_hh1, const float *y, float *gates, float *aux, const float *dy, float *dx,
                    float *dw_ih0, float *dw_hh0, float *dw_ih1, float *dw_hh1, float beta_w, int precision, void *scratch, void *ws,
                    size_t ws_bytes, void *stream, const ctcn_rnn_call *call);
/* ctcn_rnn_bwd with dw_ih0 == dw_hh0 == NULL runs the recurrence and dx only and leaves d(pre-activation) in gates
 * (and aux for the GRU n-gate); this call then produces the weight gradients from it: dW_ih = da^T x, dW_hh = da^T h_prev.
 * It has no consumer inside the backward pass, so the host side issues it on a second stream next to the NEXT layer's
 * persistent recurrence; xcd_allow != 0 (bit x = XCD x) keeps the bf16x3 GEMM workgroups of precision 1 on those XCDs,
 * i.e. off the ones the recurrence occupies.  ws must not be shared with calls running concurrently on another stream. */
int ctcn_rnn_bwd_weights(int cell, int T, int B, int I, int H, int dirs, const float *x, const float *y,
                         const float *gates, const float *aux, float *dw_ih0, float *dw_hh0, float *dw_ih1,
                         float *dw_hh1, float beta_w, int precision, unsigned xcd_allow, void *ws, size_t ws_bytes,
                         void *stream);

/* ---------------------------------------------------------------------------------------------------
 * BatchNorm, statistics per channel over (outer x inner) elements; x viewed as (outer, C, inner).
 *   inner==1 : BatchNorm1d over (T*B) rows   (model_ctc.py:29-32, :136,165-166)
 *   inner>1  : BatchNorm2d on NCHW            (model_ctc.py:47,63)
 * train fwd: y = gamma*(x-mean)*rstd+beta; saves mean,rstd (C each); updates running stats in place
 * (momentum 0.1 semantics: rm = (1-mom)*rm + mom*mean; rv uses the unbiased variance).
 * relu!=0 fuses nn.ReLU (model_ctc.py:64) into the apply pass and its mask into the backward pass.
 * Accuracy: the per-channel sums (x, x^2; dy', dy' xhat) are float64; mean = s / n and var = max(ss / n - mean^2, 0) are formed in float64 and
 * save_mean, save_rstd stored as float32; y = fma((x - save_mean) * save_rstd, gamma, beta) in float32.  Therefore y is off by about
 * |gamma| * rstd * ulp(mean) / 2 on a channel whose mean is large against its spread (the float32 save_mean), and var by about
 * 3 n 2^-53 mean^2 (the cancellation in ss / n - mean^2: negligible until it nears var + eps).  A constant channel is exact: save_mean is the
 * value, var 0, y = beta.  tests/bn_ref.py derives the per-element bounds the tests hold every entry point to.
 * ws: >= ctcn_bn_ws_bytes(outer, C, inner) (0 for dims that are not positive). */
size_t ctcn_bn_ws_bytes(int outer, int C, int inner);
int ctcn_bn_fwd_train(const float *x, float *y, const float *gamma, const float *beta, float *running_mean,
                      float *running_var, float *save_mean, float *save_rstd, int outer, int C, int inner,
                      float eps, float momentum, int relu, void *ws, size_t ws_bytes, void *stream,
                      long long *num_batches_tracked /* device int64 or NULL: += 1 by the statistics kernel (nn.BatchNorm's counter, no launch of its own) */);
/* Synchronised BatchNorm for data-parallel training (statistics over the global batch): every rank calls
 * _sums (per-channel fp64 [C][2]: sum x, sum x^2 / sum dy', sum dy'*xhat), the host all-reduces the 2*C doubles, and
 * _finish normalises with count_total = global number of elements per channel.  In the backward finish local_sums feed
 * dgamma / dbeta (the gradient all-reduce adds the ranks up), global_sums feed dx. */
int ctcn_bn_fwd_sums(const float *x, double *sums, int outer, int C, int inner, void *ws, size_t ws_bytes, void *stream);
int ctcn_bn_fwd_finish(const float *x, float *y, const float *gamma, const float *beta, float *running_mean,
                       float *running_var, float *save_mean, float *save_rstd, const double *sums, double count_total,
                       int outer, int C, int inner, float eps, float momentum, int relu, void *stream,
                       long long *num_batches_tracked /* as in ctcn_bn_fwd_train */);
int ctcn_bn_bwd_sums(const float *x, const float *y, const float *dy, const float *save_mean, const float *save_rstd,
                     double *sums, int outer, int C, int inner, int relu, void *ws, size_t ws_bytes, void *stream);
int ctcn_bn_bwd_finish(const float *x, const float *y, const float *dy, const float *gamma, const float *save_mean,
                       const float *save_rstd, float *dx, float *dgamma, float *dbeta, const double *local_sums,
                       const double *global_sums, double count_total, int outer, int C, int inner, int relu,
                       float beta_acc, void *ws, size_t ws_bytes, void *stream);
int ctcn_bn_fwd_eval(const float *x, float *y, const float *gamma, const float *beta, const float *running_mean,
                     const float *running_var, int outer, int C, int inner, float eps, int relu, void *stream);
/* y is only read when relu!=0 (mask = y>0). dx may alias dy. */
int ctcn_bn_bwd(const float *x, const float *y, const float *dy, const float *gamma, const float *save_mean,
                const float *save_rstd, float *dx, float *dgamma, float *dbeta, int outer, int C, int inner,
                int relu, float beta_acc, void *ws, size_t ws_bytes, void *stream);
/* BatchNorm (training statistics) + ReLU + inverted dropout in ONE apply pass, and its backward (round 5).
 * replaces: LayerCNN.forward's `x = self.batch_norm(x); x = self.activation(x); ...; x = self.dropout(x)` (model_ctc.py:62-67, no pooling between
 * them) and its autograd.  y_drop = ctcn_dropout(relu(bn(x)), p, seed, offset) bit for bit (same expression per element, same Philox words: word
 * i & 3 of group offset + (i >> 2)); the un-dropped activation is not stored.  ctcn_bn_bwd_dropout takes dy_drop = the gradient of the DROPPED
 * output, regenerates the keep mask from the counters and recomputes the ReLU mask from x (it needs beta for that): dx, dgamma, dbeta as
 * ctcn_dropout backward followed by ctcn_bn_bwd would give them, without the two passes over the dropped / un-dropped tensors.  0 < p < 1. */
int ctcn_bn_fwd_train_dropout(const float *x, float *y_drop, const float *gamma, const float *beta, float *running_mean, float *running_var,
                              float *save_mean, float *save_rstd, int outer, int C, int inner, float eps, float momentum, int relu, void *ws,
                              size_t ws_bytes, void *stream, long long *num_batches_tracked, float p, uint64_t seed, uint64_t offset);
int ctcn_bn_bwd_dropout(const float *x, const float *dy_drop, const float *gamma, const float *beta, const float *save_mean, const float *save_rstd,
                        float *dx, float *dgamma, float *dbeta, int outer, int C, int inner, int relu, float beta_acc, void *ws, size_t ws_bytes,
                        void *stream, float p, uint64_t seed, uint64_t offset);

/* Length-aware BatchNorm and frame mask: padding never reaches the statistics, the outputs or the gradients.
 * lens[b] (device int32) = real frames of utterance b; the geometry names the two layouts of the model:
 *   inner == 1 (rows = T * batch, time-major; frame must be 1): row r is valid iff r / batch < lens[r % batch]
 *   inner  > 1 (NCHW; batch must equal outer, inner = T' * frame): element i of plane (o, c) is valid iff i / frame < lens[o]
 * (lens are clamped to [0, T] on the device.)  The statistics, dgamma / dbeta and the dx reduction terms run over the valid elements with
 * n = sum(lens) * frame taken on the device (no host sync); running statistics use that n (unbiased variance: n - 1).  n = 1: var = 0 and
 * running_var is updated with that biased value (no n / (n - 1)); n = 0 (every length 0): mean = 0, var = 0, y = dx = 0, dgamma / dbeta = 0 (or
 * their beta_acc base), and the running statistics move towards 0 by the momentum.  y and dx are 0 at
 * invalid elements by select, and no pass reads x / y / dy there.  Otherwise the contract of ctcn_bn_fwd_train / _eval / ctcn_bn_bwd
 * (relu, num_batches_tracked, beta_acc, deterministic float64 partials).  ws: >= ctcn_bn_masked_ws_bytes(outer, C, inner).
 * ctcn_mask_frames: y = valid ? x : 0 (its own backward); y may alias x. */
size_t ctcn_bn_masked_ws_bytes(int outer, int C, int inner);
int ctcn_mask_frames(const float *x, float *y, const int *lens, int batch, int frame, int outer, int C, int inner, void *stream);
int ctcn_bn_fwd_train_masked(const float *x, float *y, const float *gamma, const float *beta, float *running_mean, float *running_var,
                             float *save_mean, float *save_rstd, const int *lens, int batch, int frame, int outer, int C, int inner,
                             float eps, float momentum, int relu, void *ws, size_t ws_bytes, void *stream, long long *num_batches_tracked);
int ctcn_bn_fwd_eval_masked(const float *x, float *y, const float *gamma, const float *beta, const float *running_mean,
                            const float *running_var, const int *lens, int batch, int frame, int outer, int C, int inner, float eps,
                            int relu, void *stream);
int ctcn_bn_bwd_masked(const float *x, const float *y, const float *dy, const float *gamma, const float *save_mean, const float *save_rstd,
                       float *dx, float *dgamma, float *dbeta, const int *lens, int batch, int frame, int outer, int C, int inner, int relu,
                       float beta_acc, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Dropout (inverted, Philox4x32-10 counter RNG keyed by (seed, offset + element index)).
 * replaces: nn.Dropout (model_ctc.py:26,34,58,67).  bwd regenerates the mask from (seed, offset). */
int ctcn_dropout(const float *x, float *y, size_t n, float p, uint64_t seed, uint64_t offset, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Conv2d (bias) NCHW, direct; replaces nn.Conv2d in LayerCNN (model_ctc.py:46,61).
 * x (B,Ci,Hi,Wi) w (Co,Ci,kh,kw) y (B,Co,Ho,Wo), Ho=(Hi+2ph-kh)/sh+1.
 * Default: MFMA implicit GEMMs (option "conv_mfma") for Co <= 64, kh*kw <= 25 and LDS images within 158 KB; everything else on the direct
 * kernels, which (round 6) run a filter bank beyond their 60-KB LDS budget as (output-channel range, input-channel range) slices -- the
 * reference's own example front-end, model_ctc.py:232-233: (1,32,(3,41)) = 123 taps and (32,32,(3,21)) = 258 KB of filters -- slowly, not
 * with an error.  CTCN_EUNSUPPORTED only beyond ~900 taps per (output, input) channel pair. */
size_t ctcn_conv2d_ws_bytes(int B, int Ci, int Hi, int Wi, int Co, int kh, int kw, int sh, int sw, int ph, int pw);
int ctcn_conv2d_fwd(const float *x, const float *w, const float *bias, float *y, int B, int Ci, int Hi, int Wi,
                    int Co, int kh, int kw, int sh, int sw, int ph, int pw, void *stream);
int ctcn_conv2d_bwd(const float *x, const float *w, const float *dy, float *dx /*or NULL*/, float *dw,
                    float *dbias, int B, int Ci, int Hi, int Wi, int Co, int kh, int kw, int sh, int sw, int ph,
                    int pw, float beta_acc, void *ws, size_t ws_bytes, void *stream);
/* (B,C,T,F) <-> (T,B,C*F), feature index c*F+f   (model_ctc.py:153-158) */
int ctcn_bctf_to_tbcf(const float *in, float *out, int B, int C, int T, int F, void *stream);
int ctcn_tbcf_to_bctf(const float *in, float *out, int B, int C, int T, int F, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * log_softmax over the last dim (+ arg-max, lowest index on ties) and its backward.
 * replaces: nn.LogSoftmax (model_ctc.py:140,168,181); torch.max(out,-1) (train_ctc.py:51, ctcDecoder.py:163)
 * argmax (rows) int32 may be NULL. */
int ctcn_log_softmax_fwd(const float *logits, float *lp, int32_t *argmax, int rows, int V, void *stream);
int ctcn_log_softmax_bwd(const float *lp, const float *dlp, float *dlogits, int rows, int V, void *stream);
int ctcn_argmax(const float *lp, int32_t *argmax, int rows, int V, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * CTC loss (blank = 0, zero_infinity = False); replaces nn.CTCLoss(reduction='sum') forward/backward
 * (train_ctc.py:144,47-48,63).  lp (T,B,V) log-probs; targets (B,Lmax) int64 zero-padded;
 * in_len/tgt_len (B) int64.  alpha: (T,B,2*Lmax+1) reserve.  nll (B): per-utterance negative
 * log-likelihood (+inf when no alignment exists).  Lmax <= 2047 (sixteen lattice states per thread), else CTCN_EUNSUPPORTED.
 * bwd: grad_lp[t,b,c] = gscale[0] * (exp(lp) - exp(logsum_{s:ext(s)=c}(alpha+beta) + nll - lp)) for
 * t < in_len[b], 0 beyond; gscale is a 1-element DEVICE float (the upstream gradient of the summed loss).
 * alpha is overwritten with alpha+beta. */
int ctcn_ctc_fwd(const float *lp, const int64_t *targets, const int64_t *in_len, const int64_t *tgt_len,
                 float *alpha, float *nll, int T, int B, int V, int Lmax, void *stream);
int ctcn_ctc_bwd(const float *lp, const int64_t *targets, const int64_t *in_len, const int64_t *tgt_len,
                 float *alpha, const float *nll, const float *gscale, float *grad_lp, int T, int B, int V,
                 int Lmax, void *stream);
/* The same loss when a gradient will be wanted (training, train_ctc.py:47 followed by :63): alpha AND beta, each into its
 * own (T,B,2*Lmax+1) lattice, in ONE launch -- the two passes are independent chains of T dependent steps, so side by
 * side they cost one chain -- then ctcn_ctc_grad adds them on the fly (the same single f32 add as ctcn_ctc_bwd's
 * in-place pass: bit-identical gradients) and leaves both lattices untouched. */
int ctcn_ctc_fwd_both(const float *lp, const int64_t *targets, const int64_t *in_len, const int64_t *tgt_len,
                      float *alpha, float *beta, float *nll, int T, int B, int V, int Lmax, void *stream);
int ctcn_ctc_grad(const float *lp, const int64_t *targets, const int64_t *in_len, const int64_t *tgt_len,
                  const float *alpha, const float *beta, const float *nll, const float *gscale, float *grad_lp,
                  int T, int B, int V, int Lmax, void *stream);
/* out[0] = sum_b nll[b]  (deterministic order) */
int ctcn_sum_f32(const float *x, float *out, int n, void *stream);
/* The whole nn.CTCLoss(blank, reduction, zero_infinity) contract; the four entry points above are these with blank = 0,
 * reduction 'sum', zero_infinity = 0 (bit for bit).
 * fwd_ex: ctcn_ctc_fwd_both with beta != NULL, ctcn_ctc_fwd with beta == NULL (alpha only: no gradient wanted).  The extended
 *   label string is blank, target[0], blank, ..., blank; blank must lie in [0, V) and labels should differ from it (as in torch).
 * grad_ex: ctcn_ctc_grad with beta != NULL; beta == NULL means alpha already holds alpha + beta.  The gradient of utterance b is
 *   scaled by gscale[b * gscale_stride] (stride 0: the DEVICE scalar upstream gradient of 'sum' / 'mean'; 1: the (B) upstream
 *   gradient of 'none'), divided by B * max(tgt_len[b], 1) when reduction == CTCN_REDUCTION_MEAN.  zero_infinity != 0: the rows
 *   of an utterance with nll = +inf are 0 instead of NaN.  Rows of utterances with lengths outside the tensors stay NaN.
 *   A -inf log-prob gives NaN at that cell of a feasible utterance's gradient, as torch does, and finite values elsewhere.
 * reduce: nll' = nll with +inf replaced by 0 if zero_infinity; NONE: out (B) = nll'; SUM: out[0] = sum_b nll'_b; MEAN:
 *   out[0] = (1/B) sum_b nll'_b / max(tgt_len[b], 1) (tgt_len may be NULL unless MEAN).  One workgroup, fixed order, double
 *   partials; NaN (every output) while the status word of ctcn_set_status_buffer is set, as ctcn_sum_f32.
 * pack_targets: concatenated targets flat (n_flat) int64 + tgt_len (B) -> padded (B, Lmax) int64, row b = flat[o_b .. o_b +
 *   tgt_len[b]) (o_b = sum of the lengths before b, negative ones counted as 0) truncated to Lmax, zeros after; nothing past
 *   flat[n_flat) is read.  Lmax > 0. */
int ctcn_ctc_fwd_ex(const float *lp, const int64_t *targets, const int64_t *in_len, const int64_t *tgt_len, float *alpha,
                    float *beta, float *nll, int T, int B, int V, int Lmax, int blank, void *stream);
int ctcn_ctc_grad_ex(const float *lp, const int64_t *targets, const int64_t *in_len, const int64_t *tgt_len, const float *alpha,
                     const float *beta, const float *nll, const float *gscale, int gscale_stride, int reduction, int zero_infinity,
                     int blank, float *grad_lp, int T, int B, int V, int Lmax, void *stream);
int ctcn_ctc_reduce(const float *nll, const int64_t *tgt_len, float *out, int B, int reduction, int zero_infinity, void *stream);
int ctcn_ctc_pack_targets(const int64_t *flat, int64_t n_flat, const int64_t *tgt_len, int64_t *padded, int B, int Lmax, void *stream);
/* CTC forced alignment: the best path of the KNOWN transcript through the lattice of ctcn_ctc_fwd_ex, its per-frame scores and the
 * frames of every target token (the capability of torchaudio's forced_align + merge_tokens; the reference has no counterpart).
 * For utterance b: Tb = in_len[b], L = tgt_len[b], S = 2L + 1, ext(s) = blank for even s, targets[b, s >> 1] for odd s (targets is
 * the padded (B, Lmax) layout; ctcn_ctc_pack_targets converts concatenated ones), any blank in [0, V).
 *   v[0][s] = lp[0, b, ext(s)] for s <= 1, -inf otherwise;
 *   v[t][s] = max(v[t-1][s], v[t-1][s-1], v[t-1][s-2] if allowed) + lp[t, b, ext(s)] -- ONE float32 add, never fused or reordered;
 *   s-2 is allowed under the loss's rule (s odd, s >= 2, ext(s) != ext(s-2)).
 *   Ties: the predecessor with the smallest move wins (s, then s-1, then s-2: a candidate replaces the best so far only if
 *   strictly greater).  End state: S-1, or S-2 only if v[Tb-1][S-2] > v[Tb-1][S-1] (and S > 1).  The result is a function of the
 *   input alone: a float32 restatement with the same tie rule gives the same bits.
 * Outputs (every element is written, the caller need not clear them):
 *   score (B) float32 = the end value; ok (B) int32 = (score != -inf);
 *   paths (B, T) int32 = ext(s_t) for t < Tb, -1 beyond; frame_scores (B, T) float32 = lp[t, b, paths[b, t]], 0 beyond;
 *   starts, ends (B, Lmax) int32, each may be NULL = first and one-past-last frame spent in state 2j + 1, -1 for j >= L.
 *   No alignment (score == -inf): ok = 0, paths -1, frame_scores 0, spans -1.  Tb == 0: ok = (L == 0), score 0 / -inf.  Lengths
 *   outside the tensors (Tb < 0, Tb > T, L < 0, L > Lmax): ok = 0, score NaN, fills as for no alignment.
 * One workgroup per utterance; a 2-bit move per (t, s), packed 16 to a word, kept in LDS when T * ceil((2 Lmax + 1) / 16) words fit
 * beside the value rows in 64 KB, otherwise in ws (the _ws_bytes query answers 0 in the first case, where ws may be NULL): arithmetic on
 * (T, Lmax) alone, no learnt state.  Lmax == 0 is legal (all-blank paths); Lmax <= 2047 as for the loss, else CTCN_EUNSUPPORTED. */
size_t ctcn_ctc_align_ws_bytes(int T, int B, int Lmax);
int ctcn_ctc_align(const float *lp, const int64_t *targets, const int64_t *in_len, const int64_t *tgt_len, int32_t *paths,
                   float *frame_scores, float *score, int32_t *ok, int32_t *starts, int32_t *ends, int T, int B, int V, int Lmax,
                   int blank, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Adam with L2-coupled weight decay over one flat buffer; replaces torch.optim.Adam.step
 * (train_ctc.py:145,65).  step is the 1-based step count. */
int ctcn_adam_step(float *p, const float *g, float *m, float *v, size_t n, float lr, float beta1, float beta2,
                   float eps, float weight_decay, int step, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Global gradient-norm clipping and a non-finite-step guard over the flat gradient; replaces
 * torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) (the reference carries it commented out at train_ctc.py:64) in front
 * of Adam, and the drop-the-step rule of torch.amp.GradScaler.step.  Everything is enqueued on `stream`; nothing synchronises, nothing
 * is allocated, no state is kept: the decision lives in a caller-owned DEVICE control block. */
#define CTCN_NORM_L2 2
#define CTCN_NORM_INF 0
typedef struct ctcn_clip_ctl {
  float total_norm;   /* written by ctcn_grad_norm (pass &ctl->total_norm, &ctl->nonfinite) */
  int32_t nonfinite;  /* 1: total_norm is NaN or Inf (an element of g is, or the float32 norm overflowed) */
  float clip_coef;    /* min(1, max_norm / (total_norm + 1e-6)) in float32: torch's expression and epsilon; NaN stays NaN */
  int32_t apply;      /* 0: ctcn_adam_step_ex writes nothing (the step was dropped) */
  int32_t step;       /* applied steps so far = the bias-correction count; the caller initialises (0) and may rewrite it (checkpoints) */
  int32_t skipped;    /* dropped steps so far; the caller initialises (0) */
  float step_size;    /* (float)((double)lr / (1 - beta1^step)) */
  float sqrt_bc2;     /* (float)sqrt(1 - beta2^step): the expressions ctcn_adam_step evaluates on the host, in double */
} ctcn_clip_ctl;
/* grad_norm: *total_norm = the norm of g[0..n) (norm_type CTCN_NORM_L2 or CTCN_NORM_INF), *nonfinite (may be NULL) as above.
 *   L2: every float32 square is widened to double; chunk c = elements [16384 c, 16384 (c+1)) is summed in a fixed order whichever workgroup
 *   takes it, the chunk partials are added in index order by one thread, and (float)sqrt(sum) is stored: the result is a function of the
 *   bits of g alone (not of the grid, the device, the stream or the alignment of g), so every data-parallel rank derives the same
 *   coefficient from its all-reduced buffer.  No atomics.  INF: max |g[i]|, exact.  NaN / Inf in g reach total_norm as they do in torch
 *   (NaN wins over Inf).  n = 0 gives 0.
 *   seg_offsets (nseg + 1 DEVICE int64, segment s = [seg_offsets[s], seg_offsets[s+1]) clipped to [0, n)) / seg_norms (nseg DEVICE float32):
 *   the same norm per segment (one segment per parameter tensor: per-layer telemetry), 16 fixed slices per segment; nseg = 0: both NULL.
 *   grid_blocks = 0 sizes the grid from ctcn_device_cus(); any other value forces that many workgroups (tests: the result must not move).
 *   ws: ctcn_grad_norm_ws_bytes(n, nseg) bytes, 8-byte aligned, the caller's.
 * clip_control (one thread, behind grad_norm): clip_coef from ctl->total_norm and max_norm (> 0; +inf: no clipping); then, if
 *   skip_nonfinite and ctl->nonfinite: skipped += 1, step unchanged, apply = 0; otherwise step += 1, apply = 1; then step_size and
 *   sqrt_bc2 from the (new) step.  lr and the betas are per-call host arguments (param_groups[0]['lr'] changes between epochs).
 * adam_step_ex: ctcn_adam_step with gv = g * clip_coef + weight_decay * p (clip first, then the L2 decay, as clip_grad_norm_ followed by
 *   Adam.step) and step_size / sqrt_bc2 / apply read from ctl.  g is NOT written back: the fused path saves that pass, so after the step
 *   the gradient buffer still holds the unclipped gradient.  With clip_coef = 1 and apply = 1, p, m and v are ctcn_adam_step's bit for bit
 *   for equal step_size / sqrt_bc2 -- those are rounded to float32 from doubles whose pow() is the device library's here and the host
 *   libm's there: the two agree unless the last ulp of a double pow decides a float32 rounding.
 * scale_by_device_scalar: x[i] *= *scalar in place (the stand-alone clip_grad_norm_, which leaves clipped gradients behind as torch
 *   does; a NaN coefficient poisons them, as in torch with error_if_nonfinite = False). */
size_t ctcn_grad_norm_ws_bytes(size_t n, int nseg);
int ctcn_grad_norm(const float *g, size_t n, int norm_type, const int64_t *seg_offsets, int nseg, float *seg_norms, float *total_norm,
                   int32_t *nonfinite, int grid_blocks, void *ws, size_t ws_bytes, void *stream);
int ctcn_clip_control(ctcn_clip_ctl *ctl, float max_norm, float lr, float beta1, float beta2, int skip_nonfinite, void *stream);
int ctcn_adam_step_ex(float *p, const float *g, float *m, float *v, size_t n, float beta1, float beta2, float eps, float weight_decay,
                      const ctcn_clip_ctl *ctl, void *stream);
int ctcn_scale_by_device_scalar(float *x, size_t n, const float *scalar, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Data-parallel exchange step: SUM all-reduce of the flat float32 gradient buffer (or a slice of it) over RCCL / xGMI,
 * one communicator per rank.  The reference is single-device (train_ctc.py:63-65 loss.backward(); optimizer.step()); utterance-
 * sharded data parallelism inserts this one collective between the two calls.  librccl.so is opened at run time.
 *   rank 0 calls ctcn_comm_unique_id (128 bytes) and hands the blob to the other ranks by any host channel; every rank then
 *   calls ctcn_comm_init (collective: blocks until all `world` ranks arrived).  The communicator is the only object the library
 *   owns; ctcn_comm_allreduce_sum_f32 is enqueued on `stream` (in place) and returns without synchronising.  A handle that ctcn_comm_init
 *   did not hand out, or that ctcn_comm_destroy has taken back, is answered with CTCN_EINVAL (the library keeps the list of live handles)
 *   instead of reaching RCCL, which would dereference it. */
int ctcn_comm_unique_id(void *id128);
int ctcn_comm_init(const void *id128, int rank, int world, void **comm);
int ctcn_comm_allreduce_sum_f32(void *comm, float *buf, size_t n, void *stream);
int ctcn_comm_destroy(void *comm);

/* ---------------------------------------------------------------------------------------------------
 * Greedy decode: collapse of arg-max paths (drop blank, drop frame-to-frame repeats, first lens[b]
 * frames); replaces GreedyDecoder.decode / CTC_Model.compute_wer inner loops
 * (ctcDecoder.py:152-166,80-92; model_ctc.py:190-199).  idx int32, element (t,b) at idx[t*stride_t+b*stride_b]
 * (time-major (T,B): stride_t=B, stride_b=1; batch-major (B,T): stride_t=1, stride_b=T);
 * out_ids (B,T) int32; out_len (B) int32. */
int ctcn_greedy_collapse(const int32_t *idx, size_t stride_t, size_t stride_b, const int32_t *lens, int32_t *out_ids,
                         int32_t *out_len, int T, int B, int blank, void *stream);

/* Tokens of a per-frame class path with their frames and scores: what ctcn_greedy_collapse throws away.  The path is the arg-max
 * path (ctcn_argmax) or the `paths` of ctcn_ctc_align; the reference has no counterpart (its decoders return strings).
 * path int32, element (t,b) at path[t*stride_t+b*stride_b] as for ctcn_greedy_collapse; lp (T,B,V) float32 contiguous; lens (B) int32;
 * any blank in [0, V).  For utterance b, n = clamp(lens[b], 0, T), k_t = path[t, b]:
 *   a class id outside [0, V) counts as blank; its frame never indexes lp and adds 0 to every sum (ctcn_ctc_align writes -1 for
 *   utterances without an alignment);
 *   frame t < n starts token j when k_t is not blank and (t == 0 or k_t != k_{t-1}) -- ctcn_greedy_collapse's rule, the same integers for
 *   a path of valid ids; start_j = t; end_j = the first t' > t with t' == n or k_t' != k_t;
 *   over the frames t of [start_j, end_j), k the token's class:
 *     tok_mean_j = mean of lp[t, b, k]; tok_min_j = their minimum (exact);
 *     tok_margin_j = mean of lp[t, b, k] - max_{c != k} lp[t, b, c] (the max exact, the difference taken in double);
 *   path_score[b] = sum over all t < n of lp[t, b, k_t], blank frames included.
 *   Sums accumulate in double and are rounded once to float32.
 * Outputs (every element is written, the caller need not clear them): out_ids, starts, ends (B,T) int32, -1 from out_len[b] on;
 *   out_len (B) int32; tok_mean, tok_min, tok_margin (B,T) float32, 0 from out_len[b] on; path_score (B) float32, 0 for n == 0.
 * One workgroup per utterance; the row of a frame inside a token is read once (for the best competitor), a blank frame's one element,
 * nothing at or past n.  No workspace, no learnt state, no option. */
int ctcn_path_tokens(const int32_t *path, size_t stride_t, size_t stride_b, const float *lp, const int32_t *lens, int32_t *out_ids,
                     int32_t *out_len, int32_t *starts, int32_t *ends, float *tok_mean, float *tok_min, float *tok_margin,
                     float *path_score, int T, int B, int V, int blank, void *stream);

/* Levenshtein distance per utterance between collapsed predictions a (B,lda) int32 / a_len (B) int32 and labels
 * b (B,ldb) int64 / b_len (B) int64 -> out (B) int32; replaces editdistance.eval in CTC_Model.compute_wer
 * (model_ctc.py:200).  max_b_len >= max(b_len). */
int ctcn_edit_distance(const int32_t *a, const int32_t *a_len, const int64_t *b, const int64_t *b_len, int32_t *out, int B,
                       int lda, int ldb, int max_b_len, void *stream);
/* ---------------------------------------------------------------------------------------------------
 * Error breakdown (editops.hip): what lies behind that distance -- substitutions, deletions, insertions, the alignment, the confusion table.
 * Definition.  h[0..nh) is the hypothesis and r[0..nr) the reference, both AFTER the class map:
 *   D[i][0] = i, D[0][j] = j, D[i][j] = min(D[i-1][j-1] + (h[i-1] != r[j-1]), D[i][j-1] + 1, D[i-1][j] + 1)
 * The move of cell (i, j) is the first candidate, in this order, that attains the minimum: diagonal (a correct pair or a substitution),
 * deletion (from (i, j-1): reference symbol j-1 has no partner), insertion (from (i-1, j): hypothesis symbol i-1 has none).  Row 0 has only
 * deletions, column 0 only insertions.  The alignment is the chain of moves from (nh, nr) back to (0, 0), emitted in forward order: a
 * function of the two sequences alone (h = [1], r = [1, 1]: del r0, cor;  h = [a, b], r = [b, a]: sub, sub).
 * Class map: map (V int32, or NULL) is applied to both sequences before the recursion -- a value in [0, V) replaces the id, -1 removes the
 * symbol (the sequence gets shorter), an id outside [0, V) passes through unchanged and never indexes anything.
 *   a (B,lda) int32 / a_len (B) int32, b (B,ldb) int64 / b_len (B) int64: the operands and the length clamps of ctcn_edit_distance
 *   (a_len to [0, lda], b_len to [0, min(max_b_len, ldb)]); nothing is read past the clamped lengths
 *   counts (B,6) int32: sub, del, ins, cor, nh, nr (lengths after the map); sub + del + cor == nr, sub + ins + cor == nh, sub + del + ins ==
 *   the Levenshtein distance of the mapped sequences
 *   ali (B, lda + ldb, 2) int32 or NULL: the (reference id, hypothesis id) pairs, -1 = none, and (-1, -1) past the last pair;
 *   ali_len (B) int32 or NULL: the number of pairs
 *   conf ((V+1)*(V+1)) int64 or NULL, zeroed by the caller, ACCUMULATED into across calls (integer atomic adds: exact, independent of
 *   order): [r][h] counts an aligned pair (correct pairs on the diagonal), row V the insertions by hypothesis class, column V the deletions
 *   by reference class, [V][V] stays 0; pairs with a member outside [0, V) are counted in `counts` but not entered
 * One wavefront per utterance; the 2-bit moves live in LDS where hypothesis, reference and moves fit in 64 KB (32 x (800 x <= 64): 17 KB),
 * else in ws (ctcn_edit_ops_ws_bytes, 0 in the LDS case; 4-byte aligned).  max_b_len > 512: CTCN_EUNSUPPORTED (the range of the
 * wavefront distance kernel).  map or conf given: V > 0. */
size_t ctcn_edit_ops_ws_bytes(int B, int lda, int max_b_len);
int ctcn_edit_ops(const int32_t *a, const int32_t *a_len, const int64_t *b, const int64_t *b_len, const int32_t *map, int V,
                  int32_t *counts, int32_t *ali, int32_t *ali_len, long long *conf, int B, int lda, int ldb, int max_b_len, void *ws,
                  size_t ws_bytes, void *stream);
/* (loss, sum of dist[0..B), sum of tgt_len[0..B), *status or 0) as four doubles in out4 (device memory): the per-step statistics of the
 * reference's run_epoch (loss.item(), total_wer's numerator and denominator, timit/steps/train_ctc.py:55-60) plus the sticky hand-off
 * status, gathered in one launch so that the host can fetch them with one small copy a step later. */
int ctcn_step_stats(const float *loss, const int32_t *dist, const int64_t *tgt_len, int B, const int32_t *status, double *out4, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Filterbank front-end (fbank.hip; the statistics of the normalisation: cmvn.hip): waveform -> log-mel features with one global mean / variance normalisation; replaces the three Kaldi
 * binaries of timit/steps/make_feat.sh (compute-fbank-feats --config=conf/fbank.conf, compute-cmvn-stats, apply-cmvn --norm-vars=true).
 * The computation is Kaldi's, as its feature-window, feature-fbank and mel-computations sources document it; option names and defaults are
 * Kaldi's.  window_type: 0 hamming, 1 hanning, 2 povey (Kaldi's default), 3 rectangular, 4 blackman.  high_freq <= 0 is an offset from Nyquist.
 * Not here: VTLN (pitch: ctcn_pitch below; per-speaker, per-utterance and sliding-window normalisation: ctcn_cmvn_accumulate_groups, ctcn_cmvn_apply, ctcn_cmvn_sliding below; deltas, splicing and frame skipping: ctcn_frame_context below; MFCC: ctcn_mfcc below; the spectrogram types: ctcn_spectrogram, ctcn_logspec below; resampling in front of them: ctcn_resample below).  Zero-initialise the struct and fill every field (ctc_pytorch_amd/utils/features.py holds the
 * defaults). */
typedef struct ctcn_fbank_opts {
  float samp_freq, frame_shift_ms, frame_length_ms, preemph_coeff, blackman_coeff, low_freq, high_freq, energy_floor;
  int32_t window_type, num_mel_bins, remove_dc_offset, round_to_power_of_two, snip_edges, use_energy, raw_energy, htk_compat, use_log_fbank,
      use_power;
} ctcn_fbank_opts;
/* Frames of a signal of num_samples samples: snip_edges != 0: 0 if num_samples < frame_length, else 1 + (num_samples - frame_length) /
 * frame_shift; snip_edges == 0: (num_samples + frame_shift / 2) / frame_shift.  Lengths in samples.  CTCN_EINVAL for a negative sample
 * count, a frame length or shift that is not positive, or a count beyond int. */
int ctcn_fbank_frames(long long num_samples, int frame_length, int frame_shift, int snip_edges);
/* The plan of a configuration, built on the HOST into the caller's buffer (no HIP call) and uploaded by the caller once: 4-byte words,
 * Npad = the frame length rounded up to a power of two,
 *   [0, Npad)            float  the window (feature-window's formulas in double, rounded once), 0 from the frame length on
 *   [Npad, 5 Npad)       float64 (cos, -sin)(2 pi k / Npad), k < Npad: the transform runs in float64 (a float32 one leaves ~1e-7 of the
 *                               frame's RMS in every bin, 1e-4 .. 1e-3 of the log of the weakest filters)
 *   [5 Npad, +128)       int32  first FFT bin of every mel filter; [+128, +256) its number of bins; [+256, +384) the offset of its weights
 *   [5 Npad + 384, +Npad) float the triangular weights of mel-computations, filter after filter (every bin feeds at most two filters, so
 *                               Npad words hold them); computed in double and rounded once -- Kaldi forms the same expressions in float32,
 *                               whose mel scale carries ~1e-7 relative noise that the 34-mel filter spacing turns into ~1e-5 of a weight
 * plan_bytes: the size of that block, 0 for options the kernel does not take.  Supported: round_to_power_of_two, Npad in {256, 512, 1024},
 * 3 <= num_mel_bins <= 128; anything else CTCN_EUNSUPPORTED.  CTCN_EINVAL: NULL, frequencies outside (0, Nyquist], an empty filter (Kaldi's
 * "num-mel-bins too large"), a buffer smaller than plan_bytes. */
size_t ctcn_fbank_plan_bytes(const ctcn_fbank_opts *opts);
int ctcn_fbank_plan(const ctcn_fbank_opts *opts, void *plan, size_t plan_bytes);
/* wave (B, Nmax): float32 on Kaldi's scale (the int16 range, not +-1) or, with wave_is_int16, int16 converted on load (the same values give
 * the same bits); lens (B) int32 samples, clamped to [0, Nmax]; opts on the host, plan = the block above in DEVICE memory; mean / scale: F
 * device floats each or both NULL, F = num_mel_bins + (use_energy ? 1 : 0).
 * feats (B, Tmax, F): rows below frames[b] hold the features -- per frame, in Kaldi's order: window extraction (snip_edges == 0 reflects the
 * signal at both ends), dither, DC removal, raw log-energy, pre-emphasis, window, zero padding, real FFT, power (or magnitude) spectrum over
 * bins 0 .. Npad/2 - 1, mel bank, log(max(e, FLT_EPSILON)), energy in column 0 (last column under htk_compat), then (x - mean) * scale as a
 * float32 subtraction followed by a float32 multiplication; rows from frames[b] on are written as zeros.  frames (B) int32 = the frame
 * count of the utterance, at most Tmax.  The rows of an utterance depend on its own samples alone, not on B, Nmax, Tmax or its neighbours.
 * dither > 0 adds dither * N(0, 1) to every sample of every extracted window: Philox4x32-10 keyed by seed, counter (utterance index b +
 * utt_offset, frame, sample pair), Box-Muller -- a function of those alone (not Kaldi's generator); b + utt_offset < 2^26, frames < 2^28.
 * One wave per frame (Npad / 64 points per lane), four waves per workgroup sharing the staged samples of up to eight neighbouring frames;
 * a half-length complex FFT in float64 (radix 8, 8, Npad / 128 through LDS) and a split step; everything else is float32. */
int ctcn_fbank(const void *wave, int wave_is_int16, const int32_t *lens, const ctcn_fbank_opts *opts, const void *plan, const float *mean,
               const float *scale, float *feats, int32_t *frames, int B, int Nmax, int Tmax, float dither, uint64_t seed, uint64_t utt_offset,
               void *stream);
/* stats (2, F + 1) DEVICE doubles, Kaldi's CMVN statistics matrix: row 0 the per-column sums with the frame count in the last column, row 1
 * the sums of squares with 0 there.  ADDS the rows t < frames[b] (clamped to [0, Tmax]) of feats (B, Tmax, F) to it; nothing at or beyond
 * frames[b] is read.  Every workgroup leaves float64 partial sums of its 64 rows in ws, one launch adds them up in index order: a function
 * of the input bits, not of scheduling.  ws: ctcn_cmvn_accumulate_ws_bytes(B, Tmax, F) bytes, 8-byte aligned. */
size_t ctcn_cmvn_accumulate_ws_bytes(int B, int Tmax, int F);
int ctcn_cmvn_accumulate(const float *feats, const int32_t *frames, double *stats, int B, int Tmax, int F, void *ws, size_t ws_bytes,
                         void *stream);
/* MFCC, the recipe's second feature type (feat_type=mfcc: compute-mfcc-feats --config=conf/mfcc.conf), by the same kernel: Kaldi's
 * feature-mfcc.  The options are Kaldi's MfccOptions under the filterbank's field names plus num_ceps and cepstral_lifter; Kaldi's MFCC
 * defaults differ from the filterbank's in use_energy = true (and num_mel_bins = 23, num_ceps = 13, cepstral_lifter = 22).  There is no
 * use_log_fbank / use_power: an MFCC is always taken from the log of the mel-filtered power spectrum.  Zero-initialise and fill every field
 * (utils/features.MfccConfig holds the defaults).  Per frame, N = num_mel_bins, C = num_ceps, Q = cepstral_lifter:
 *   1. log-mel energies m[0..N) and the log energy e exactly as ctcn_fbank computes them with use_power, use_log_fbank (the same code);
 *   2. c[k] = sum_n D[k][n] m[n], k < C, summed in ascending n with one fused multiply-add per term: D[0][n] = sqrt(1 / N),
 *      D[k][n] = sqrt(2 / N) cos(pi / N (n + 0.5) k) -- the first C rows of Kaldi's ComputeDctMatrix;
 *   3. c[k] *= 1 + Q / 2 sin(pi k / Q), a float32 multiplication of its own (Q = 0: no lifter);
 *   4. use_energy: e is raised to log(energy_floor) where energy_floor > 0, and c[0] = e;
 *   5. htk_compat: c[0] goes to column C - 1 and the others move down by one; without use_energy it is multiplied by sqrt(2) first (in
 *      double, rounded once, as Kaldi's `*= M_SQRT2` does);
 *   6. (x - mean[col]) * scale[col] on the final columns, as ctcn_fbank.
 * The plan: the filterbank plan of the same frame and mel options, bit for bit, in words [0, 6 Npad + 384); then
 *   [6 Npad + 384, + N C)  float  the DCT table, bin-major: D[k][n] at word n C + k (lanes owning consecutive cepstra read consecutive words)
 *   [.. + N C, + C)        float  the lifter (ones for Q = 0)
 * both computed in double and rounded once.  Limits beyond the filterbank's (which all carry over): 1 <= num_ceps <= num_mel_bins and
 * cepstral_lifter >= 0, else CTCN_EINVAL; num_ceps <= 64, else CTCN_EUNSUPPORTED (one lane per coefficient; the table stays within 32 KB
 * of LDS).  ctcn_mfcc takes ctcn_fbank's arguments with feats (B, Tmax, C) and mean / scale of C floats; frame counts: ctcn_fbank_frames. */
typedef struct ctcn_mfcc_opts {
  float samp_freq, frame_shift_ms, frame_length_ms, preemph_coeff, blackman_coeff, low_freq, high_freq, energy_floor, cepstral_lifter;
  int32_t window_type, num_mel_bins, num_ceps, remove_dc_offset, round_to_power_of_two, snip_edges, use_energy, raw_energy, htk_compat;
} ctcn_mfcc_opts;
size_t ctcn_mfcc_plan_bytes(const ctcn_mfcc_opts *opts);
int ctcn_mfcc_plan(const ctcn_mfcc_opts *opts, void *plan, size_t plan_bytes);
int ctcn_mfcc(const void *wave, int wave_is_int16, const int32_t *lens, const ctcn_mfcc_opts *opts, const void *plan, const float *mean,
              const float *scale, float *feats, int32_t *frames, int B, int Nmax, int Tmax, float dither, uint64_t seed, uint64_t utt_offset,
              void *stream);
/* Spectrogram, the recipe's third feature type (feat_type=spectrogram: compute-spectrogram-feats --config=conf/spectrogram.conf), by the
 * same kernel: Kaldi's feature-spectrogram.  The options are Kaldi's SpectrogramOptions under the filterbank's field names: the frame
 * options, energy_floor (0), raw_energy (true) and return_raw_fft (false; true is Kaldi's complex output and not built).  Zero-initialise
 * and fill every field (utils/features.SpectrogramConfig holds the defaults).  Per frame, F = Npad / 2 + 1:
 *   1. extraction (both snip_edges rules), dither, DC removal, raw log-energy, pre-emphasis, window, zero padding and the float64 real
 *      transform exactly as ctcn_fbank runs them (the same code);
 *   2. the power of bins 0 .. Npad / 2 INCLUSIVE, rounded once to float32; the Nyquist bin, which the filterbank never reads, comes from
 *      the split step's first element: (Re Z[0] - Im Z[0])^2;
 *   3. log(max(p, FLT_EPSILON));
 *   4. column 0 (the DC bin) is replaced by the log energy e -- log(max(sum x^2, FLT_EPSILON)) before pre-emphasis and window (raw_energy)
 *      or behind the window -- raised to log(energy_floor) where energy_floor > 0;
 *   5. (x - mean[col]) * scale[col], as ctcn_fbank.
 * The plan: words [0, 5 Npad) of the filterbank plan of the same frame options, bit for bit (window, float64 twiddles); nothing behind them.
 * Limits: the filterbank's frame limits (round_to_power_of_two, Npad in {256, 512, 1024}; else CTCN_EUNSUPPORTED) and return_raw_fft = false
 * (true: CTCN_EUNSUPPORTED); every refusal comes from ctcn_spectrogram_plan (and again from ctcn_spectrogram before any launch).
 * ctcn_spectrogram takes ctcn_fbank's arguments with feats (B, Tmax, F) and mean / scale of F floats; lanes store columns lane, lane + 64,
 * ... of a row; frame counts: ctcn_fbank_frames.  ctcn_cmvn_accumulate takes F = 257 or 513 as it is. */
typedef struct ctcn_spectrogram_opts {
  float samp_freq, frame_shift_ms, frame_length_ms, preemph_coeff, blackman_coeff, energy_floor;
  int32_t window_type, remove_dc_offset, round_to_power_of_two, snip_edges, raw_energy, return_raw_fft;
} ctcn_spectrogram_opts;
size_t ctcn_spectrogram_plan_bytes(const ctcn_spectrogram_opts *opts);
int ctcn_spectrogram_plan(const ctcn_spectrogram_opts *opts, void *plan, size_t plan_bytes);
int ctcn_spectrogram(const void *wave, int wave_is_int16, const int32_t *lens, const ctcn_spectrogram_opts *opts, const void *plan,
                     const float *mean, const float *scale, float *feats, int32_t *frames, int B, int Nmax, int Tmax, float dither, uint64_t seed,
                     uint64_t utt_offset, void *stream);
/* The recipe's own spectrogram (timit/local/make_spectrum.py: librosa.stft, magphase, log1p, one mean and one standard deviation per
 * utterance), as numpy states it.  Options after its audio_conf: sample_rate (16000), window_size (0.025 s), window_stride (0.01 s) --
 * doubles, because n_fft = int(sample_rate * window_size) and hop = int(sample_rate * window_stride) are Python's double products (a
 * float32 0.01 gives a hop of 159) --, window: 0 hamming, 1 hann, 2 blackman, 3 bartlett (scipy.signal.windows' SYMMETRIC forms of length
 * n_fft, which is what librosa gets from the callable), normalize (true), input_scale (1.0): multiplied onto every sample in float32
 * first (log1p is not scale-free; the reference's loader may hand floats in +-1).  Per utterance of n samples, F = n_fft / 2 + 1:
 *   1. T = 0 for n = 0, else 1 + n / hop (ctcn_logspec_frames);
 *   2. frame t = samples t hop - n_fft / 2 .. + n_fft of the signal extended as numpy.pad(mode="reflect") extends it: the edge sample
 *      is not repeated, the period is 2 (n - 1), folded as often as needed, n = 1 is constant;
 *   3. the window, kept in float64 and multiplied in float64, an n_fft-point real transform in float64 (half-length complex passes of the radices fbank_core.h lists: 8, 5, 5
 *      for 400), the magnitude of bins 0 .. n_fft / 2 rounded once to float32, log1pf;
 *   4. m = the mean and s = the standard deviation (ddof = 0) of all T F values of the utterance, from float64 sums and sums of squares,
 *      each rounded once to float32; with normalize the output is (x - m) / s, a float32 subtraction and a correctly rounded float32
 *      division (numpy's np.add(x, -m), np.divide(., s)).  s == 0 (silence, or one value) gives ZEROS: the reference divides 0 by 0 there
 *      and stores NaN.
 * feats (B, Tmax, F): rows from frames[b] on are zero; frames (B) int32, at most Tmax; stats (B, 2) float32 = the (m, s) that were applied
 * or, without normalize, would have been ((0, 0) for an utterance without frames).  An utterance's rows and stats depend on its own samples
 * alone.  No atomics: the feature kernel leaves one float64 (sum, sum of squares) per workgroup in ws, a second kernel adds an utterance's
 * partials in index order in every one of its workgroups (the same bits in each), writes stats and normalises in place.
 * The plan (host, 4-byte words, W = n_fft rounded up to a multiple of 64): [0, 2 W) float64 the window, zeros from n_fft on (so lane-strided
 * loads of W / 64 registers stay in bounds) -- float64 because a float32 window or product leaves ~1e-3 of absolute noise in every bin, which
 * log1p shows as 1e-5 in a valley 500 times below the spectrum's level; [2 W, 2 W + 4 n_fft) float64 (cos, -sin)(2 pi k / n_fft), k < n_fft.
 * Limits: n_fft in {256, 400, 512, 1024}, else CTCN_EUNSUPPORTED; CTCN_EINVAL: NULL, a rate, size, stride or scale that is not positive,
 * an unknown window, a hop below 1, a buffer smaller than plan_bytes; all from ctcn_logspec_plan, before any launch.  A stride too long
 * for the LDS staging of one frame is CTCN_EUNSUPPORTED from ctcn_logspec.  wave, wave_is_int16, lens, B, Nmax, Tmax as ctcn_fbank takes
 * them; there is no dither.
 * ws: ctcn_logspec_ws_bytes(opts, B, Tmax) bytes, 8-byte aligned. */
typedef struct ctcn_logspec_opts {
  double sample_rate, window_size, window_stride;
  float input_scale;
  int32_t window, normalize;
} ctcn_logspec_opts;
int ctcn_logspec_frames(long long num_samples, int hop);
size_t ctcn_logspec_plan_bytes(const ctcn_logspec_opts *opts);
int ctcn_logspec_plan(const ctcn_logspec_opts *opts, void *plan, size_t plan_bytes);
size_t ctcn_logspec_ws_bytes(const ctcn_logspec_opts *opts, int B, int Tmax);
int ctcn_logspec(const void *wave, int wave_is_int16, const int32_t *lens, const ctcn_logspec_opts *opts, const void *plan, float *feats,
                 int32_t *frames, float *stats, int B, int Nmax, int Tmax, void *ws, size_t ws_bytes, void *stream);
/* The transform of both front-ends on the HOST (no HIP call; works without a GPU): power[0 .. n / 2] = |X[k]|^2 of the n real values of
 * `frame`, n in {256, 400, 512, 1024}, by the kernels' own passes and split step (fbank_core.h) with a loop over the 64 lanes standing in
 * for the wave.  CTCN_EINVAL for NULL, CTCN_EUNSUPPORTED for another n. */
int ctcn_fbank_power_host(const double *frame, int n, double *power);
/* Waveform resampling in front of the feature kernels (resample.hip): Kaldi's LinearResample as its ResampleWaveform configures it -- what
 * the Kaldi binaries run under --allow-downsample / --allow-upsample -- and, read at the original rate, the recipe's speed perturbation:
 * perturbing by factor f at rate sr is orig_freq = round(sr f), new_freq = sr (ceil(n / f) samples; sox `speed f` with this filter).
 * Options: integer rates fin = orig_freq and fout = new_freq in Hz, cutoff in Hz (ResampleWaveform: 0.99 * 0.5 * min(fin, fout)), num_zeros
 * (ResampleWaveform: 6); utils/features.Resampler holds those defaults.  With g = gcd(fin, fout), iu = fin / g input and ou = fout / g output
 * samples per unit (ou = the number of filter phases) and ww = num_zeros / (2 cutoff):
 *   1. the plan, on the host in double, for every phase i < ou: t = i / fout; lo = ceil((t - ww) fin), hi = floor((t + ww) fin);
 *      first[i] = lo (may be negative), ntaps[i] = hi - lo + 1; for j < ntaps[i]: dt = (lo + j) / fin - t,
 *      w[i][j] = filt(dt) win(dt) / fin rounded once to float32 (Kaldi's storage type), with
 *      win(dt) = 0.5 (1 + cos(2 pi cutoff / num_zeros dt)) for |dt| < ww, else 0, and filt(dt) = sin(2 pi cutoff dt) / (pi dt), 2 cutoff at 0;
 *   2. the output length (Kaldi's flush = true): ceil(n fout / fin) in integer arithmetic, 0 for n = 0 (ctcn_resample_samples;
 *      CTCN_EINVAL for a negative count or a rate that is not positive, CTCN_EUNSUPPORTED for a length beyond int);
 *   3. output sample k, u = k / ou, p = k % ou: y[k] = sum_j w[p][j] x[first[p] + u iu + j], j ascending, samples outside [0, n) counting
 *      as zero and never read; accumulated in float64 from the float32 weights and float32 samples (int16 converted exactly) and rounded
 *      once to float32.  A float32 product is exact in double, so the sum is one number with or without fused multiply-adds: numpy's
 *      ascending double sum over the plan's weights gives the same bits.  Output stays on the input's scale; nothing is rounded to int16.
 * The plan block (host, 4-byte words): [0, 8) int32 ou, iu, the weight row stride S (the longest tap count made odd: lanes on neighbouring
 * phases meet different LDS banks), the longest tap count, outputs per workgroup tile (a multiple of ou, at most 2048 unless ou is larger),
 * the smallest first[], staged input samples per tile, 0; [8, 8 + ou) int32 first; [8 + ou, 8 + 2 ou) int32 ntaps; [8 + 2 ou, + ou S) float
 * the weights, row p at p S, zeros behind ntaps[p].
 * ctcn_resample: wave (B, Nmax) float32 or, with wave_is_int16, int16; lens (B) int32 samples clamped to [0, Nmax]; opts on the host, plan
 * the block in DEVICE memory; out (B, Mmax) float32: the first min(ceil(lens[b] fout / fin), Mmax) values of row b are the samples, the
 * rest of the row zeros.  One launch, grid (tiles of Mmax, B): the workgroup stages the table and the tile's input span in LDS, every lane
 * computes whole outputs.  A row depends on its own samples alone, not on B, Nmax, Mmax or its neighbours.
 * Limits, all CTCN_EUNSUPPORTED from ctcn_resample_plan (plan_bytes: 0) and again from ctcn_resample before any launch: rates that are not
 * positive or beyond 2^24, num_zeros <= 0, a cutoff that is not positive or with 2 cutoff > min(fin, fout), a table of ou S floats beyond
 * 24 576 (96 KB of LDS) or one unit's reach of input samples beyond 8192.  CTCN_EINVAL: NULL, B outside [1, 65 535], a small buffer.
 * ctcn_resample_host: the same sum for ONE utterance on the HOST (no HIP call; works without a GPU), `plan` the host block of the same
 * options; returns the number of samples written (out_cap must hold them) or an error code. */
typedef struct ctcn_resample_opts {
  double cutoff;
  int32_t orig_freq, new_freq, num_zeros;
} ctcn_resample_opts;
int ctcn_resample_samples(long long num_samples, int orig_freq, int new_freq);
size_t ctcn_resample_plan_bytes(const ctcn_resample_opts *opts);
int ctcn_resample_plan(const ctcn_resample_opts *opts, void *plan, size_t plan_bytes);
int ctcn_resample(const void *wave, int wave_is_int16, const int32_t *lens, const ctcn_resample_opts *opts, const void *plan, float *out, int B,
                  int Nmax, int Mmax, void *stream);
int ctcn_resample_host(const void *wave, int wave_is_int16, int num_samples, const ctcn_resample_opts *opts, const void *plan, float *out,
                       int out_cap);
/* Deltas, frame splicing, frame skipping and the downsample pad behind the feature kernels (context.hip): the stage between a zero-padded
 * base batch and the (B, T, F') batch the model consumes -- Kaldi's add-deltas (feature-functions' DeltaFeatures) followed by what the
 * reference's loader does per utterance on the host (timit/utils/tools.py make_context :66-75 and skip_feat :77-86, the zero rows of
 * SpeechDataset.__getitem__, data_loader.py:100-104, and the length fractions of create_input :119-140).  Options: left, right (context
 * frames), skip (0 and 1 both keep every frame), n_downsample, delta_order (0: no deltas), delta_window.  For an utterance of T frames of F
 * columns:
 *   1. the delta scales, on the host in float32 as Kaldi builds them: s_0 = [1]; for i = 1 .. delta_order, s_i has 2 i window + 1 entries,
 *      s_i[j + k + i window] += (float) j * s_{i-1}[k + (i - 1) window] for j = -window .. window (outer loop), k = -(i - 1) window ..
 *      (i - 1) window (a float32 multiplication, then a float32 addition), then every entry times the float32 of 1.0 / sum j^2
 *      (ctcn_delta_scales; window 2: s_1 = [-0.2, -0.1, 0, 0.1, 0.2]);
 *   2. delta'd frame u, F1 = F (delta_order + 1) columns [static F | order 1 F | order 2 F]: column f of order i is
 *      sum_j s_i[j + i window] x[clamp(u + j, 0, T - 1)][f], j = -i window .. i window ascending, entries that are zero skipped (as Kaldi
 *      skips them), clamped against the utterance's OWN length; accumulated in float64 -- the product of two float32 values is exact
 *      there, so the sum is one number with or without fused multiply-adds -- and rounded once to float32 (Kaldi adds the terms in
 *      float32, one AddVec per offset; the difference is the rounding of that sum);
 *   3. spliced row t, F2 = (left + 1 + right) F1 columns: the delta'd frames clamp(t - left, 0, T - 1) .. clamp(t + right, 0, T - 1) back
 *      to back, the oldest first;
 *   4. kept rows: t = 0, skip, 2 skip, ...: n_kept = ceil(T / skip);
 *   5. n_out = n_kept rounded up to a multiple of n_downsample (ctcn_context_frames; 0 for T = 0); rows n_kept .. n_out - 1 are zeros and
 *      count as frames.
 * ctcn_frame_context: feats (B, Tin_max, F) float32, frames (B) int32 in DEVICE memory, clamped to [0, Tin_max]; base rows at or beyond
 * frames[b] are never read.  out (B, Tout_max, F2) float32, Tout_max = ctcn_context_frames(Tin_max, skip, n_downsample) (the count is
 * monotone in T, so this is the largest n_out of any batch padded to Tin_max, a data-parallel shard of one included; another value:
 * CTCN_EINVAL): EVERY element is written -- frames, pad rows, zeros from n_out on -- the caller need not clear it.  out_frames (B) int32 =
 * n_out; fractions (B) float32 = (float)((double) n_out / (double) Tout_max), what create_input stores (0 where Tout_max is 0).
 * One launch on the caller's stream, grid (tiles of output rows, B): the workgroup stages the tile's run of base frames -- (rows - 1) skip +
 * left + 1 + right + 2 delta_order delta_window of them -- in LDS, forms every delta'd frame of it once, and writes the output rows from
 * LDS with consecutive lanes on consecutive floats.  No atomics, no workspace, no host synchronisation.  A row depends on its own
 * utterance alone, not on B, Tin_max or its neighbours.
 * ctcn_frame_context_tile: the output rows of one workgroup (at most 16; fewer where that span exceeds 64 KB of LDS), or an error code.
 * Limits, from every entry point that takes the options, before any launch: CTCN_EINVAL for NULL, a negative left / right / skip /
 * delta_order, n_downsample, delta_window or F below 1, B outside [1, 65 535], Tin_max beyond 2^30; CTCN_EUNSUPPORTED for left or right
 * beyond 64, skip or n_downsample beyond 1024, delta_order beyond 2, delta_window beyond 5, F beyond 65 536, or a single output row whose
 * span of frames exceeds 144 KB of LDS (F = 257 with two delta orders of window 5 fits with up to 14 context frames a side).
 * ctcn_frame_context_host: the same computation for ONE utterance on the HOST (no HIP call; works without a GPU): feats (num_frames, F),
 * out (out_rows, F2) written in full as the kernel writes a row of the batch with Tout_max = out_rows, *fraction (or NULL) = n_out /
 * out_rows; returns n_out (out_rows must hold it) or an error code. */
typedef struct ctcn_context_opts {
  int32_t left, right, skip, n_downsample, delta_order, delta_window;
} ctcn_context_opts;
int ctcn_context_frames(int num_frames, int skip, int n_downsample);
/* scales: room for 2 order window + 1 floats; returns that count. */
int ctcn_delta_scales(int order, int window, float *scales);
int ctcn_frame_context_tile(const ctcn_context_opts *opts, int F);
int ctcn_frame_context(const float *feats, const int32_t *frames, const ctcn_context_opts *opts, float *out, int32_t *out_frames,
                       float *fractions, int B, int Tin_max, int F, int Tout_max, void *stream);
int ctcn_frame_context_host(const float *feats, int num_frames, int F, const ctcn_context_opts *opts, float *out, int out_rows,
                            float *fraction);
/* SpecAugment on the base features, in front of ctcn_frame_context (specaug.hip): time warp, frequency masks and time masks (Park et al.,
 * Interspeech 2019), drawn per utterance from a counter-based generator so that host, device and a numpy restatement agree bit for bit.
 * Options: warp_window (W; 0: no warp), num_freq_masks, freq_width, num_time_masks, time_width, time_ratio, fill.  For utterance b of a
 * padded base batch feats (B, Tmax, F) float32:
 *   T = clamp(frames[b], 0, Tmax); the utterance's 64-bit index is u = utt_offset + b;
 *   draw(d) = the four words r0 .. r3 of philox4(seed, (u << 8) | d) of common.h: counter (low 32 bits, high 32 bits, 0, 0), key = seed --
 *   the dropout kernels' convention;
 *   rnd(word, n) = ((uint64)(word >> 8) * n) >> 24, an integer in [0, n): integer arithmetic only.
 *   1. time warp, d = 0, active when W > 0 and T > 2 W: c = W + rnd(r0, T - 2 W), w = c + rnd(r1, 2 W - 1) - (W - 1), so c in [W, T - W) and
 *      w in [1, T - 1].  Output row t < T reads a source position in integers: for t < w, num = t c, den = w, base = 0; otherwise
 *      num = (t - w) (T - c), den = T - w, base = c.  In int64: i0 = base + num / den, rem = num % den, i1 = min(i0 + 1, T - 1).  With
 *      rem = 0 the element is x[i0] itself; otherwise a = (double) rem / (double) den and the element is
 *      (float)((1.0 - a) * x[i0] + a * x[i1]), every float64 operation rounded on its own (no fused multiply-add);
 *   2. frequency masks, d = 1 .. num_freq_masks: len = rnd(r0, min(freq_width, F) + 1), f0 = rnd(r1, F - len + 1); columns [f0, f0 + len)
 *      of every row < T become fill;
 *   3. time masks, d = 9 + k, k < num_time_masks: cap = min(time_width, T, (int) floor((double) time_ratio * (double) T)),
 *      len = rnd(r0, cap + 1), t0 = rnd(r1, T - len + 1); rows [t0, t0 + len) become fill.
 * Warp first, then masks: the masks are positions in the WARPED output, so the whole is one gather, out[t][f] = masked ? fill :
 * warped(t, f).  Rows t >= T of the output are zeros; input rows at or beyond frames[b] are never read; every output element is written.
 * With all three parts off the output equals the input on rows < T, bit for bit.  An utterance's result depends on (seed, u, T, F, the
 * options, its own frames) alone, not on B, Tmax or its neighbours.
 * ctcn_spec_augment: feats, frames (B) int32 and out (B, Tmax, F) in DEVICE memory; out must not alias feats (the warp gathers).  One
 * launch on the caller's stream, grid (tiles of 32 rows, B): one wave computes the utterance's draws, one Philox call per lane, and parks
 * the intervals in LDS; every row of the tile is classified once (zero, fill, copy, interpolate) with its source rows and weight; then
 * consecutive lanes write consecutive floats, and a row inside a time mask is written without reading its source.  No atomics, no
 * workspace, no host synchronisation.
 * ctcn_spec_augment_plan: the intervals the kernel uses for ONE utterance of T frames, on the HOST (no HIP call): warp[2] = (c, w) or
 * (0, 0) without a warp, freq[2 num_freq_masks] = (f0, len) pairs, time[2 num_time_masks] = (t0, len) pairs (a pointer may be NULL where
 * its count is 0).
 * ctcn_spec_augment_host: the same computation for ONE utterance on the HOST (no HIP call; works without a GPU), through the interval and
 * interpolation functions the kernel is compiled from: feats, out (T, F).
 * Limits, from every entry point before any launch: CTCN_EINVAL for NULL, a negative count, width or window, a time_ratio outside [0, 1]
 * or NaN, a fill that is not finite, F below 1, B outside [1, 65 535], Tmax (T) negative or beyond 2^30; CTCN_EUNSUPPORTED for
 * num_freq_masks beyond 8, num_time_masks beyond 32, F beyond 65 536. */
typedef struct ctcn_specaug_opts {
  int32_t warp_window, num_freq_masks, freq_width, num_time_masks, time_width;
  float time_ratio, fill;
} ctcn_specaug_opts;
int ctcn_spec_augment(const float *feats, const int32_t *frames, const ctcn_specaug_opts *opts, uint64_t seed, uint64_t utt_offset, float *out,
                      int B, int Tmax, int F, void *stream);
int ctcn_spec_augment_plan(const ctcn_specaug_opts *opts, uint64_t seed, uint64_t utt_index, int T, int F, int32_t *warp, int32_t *freq,
                           int32_t *time);
int ctcn_spec_augment_host(const float *feats, int T, int F, const ctcn_specaug_opts *opts, uint64_t seed, uint64_t utt_index, float *out);
/* Reverberation and additive noise on the waveform (reverb.hip): multi-condition data, the one augmentation that touches the samples
 * themselves -- a room impulse response (RIR) convolved into the utterance and background noise added at a drawn signal-to-noise ratio
 * (SNR).  The project's own definition, modelled on Kaldi's wav-reverberate with --shift-output=false --normalize-output=true (one RIR, one
 * background noise repeated over the whole utterance, the SNR taken against the early part of the reverberated signal); host, device and a
 * numpy restatement agree bit for bit.
 * Inputs: utterance b of a padded batch wave (B, Nmax), float32 or int16 (converted to float32 exactly, as ctcn_resample does), has
 * n = clamp(lens[b], 0, Nmax) samples x[0 .. n) and the 64-bit running index u = utt_offset + b; a bank of R impulse responses h_r[0 .. K_r)
 * and N noises q_m[0 .. L_m), float32, and of J <= 16 SNRs in dB.  Either bank may be empty (not both); a row with K_r < 1 or L_m < 1, or
 * with a value that is not finite, is refused.
 *   Power sum S(v) of a float32 vector of len elements, in float64 ((double) v[i] squared is exact there): the elements are cut into chunks of
 *   1024 consecutive ones, the last chunk filled with zeros; a chunk is reduced by the halving tree t[j] += t[j + 512] for j < 512, then
 *   t[j] += t[j + 256] for j < 256, ... down to t[0] += t[1]; the chunk sums t[0] are added in ascending order, starting from 0.  The value
 *   depends on the vector alone -- not on the grid, the batch or a tile -- and no floating-point atomic is involved.
 *   Draws, integer arithmetic only, philox4 and rnd(word, n) as for ctcn_spec_augment: draw 0 = philox4(seed, (u << 8) | 0): reverberation
 *   is on if R > 0 and rnd(w0, 1 << 24) < floor((double) rir_prob * 2^24), and then r = rnd(w1, R); draw 1 = philox4(seed, (u << 8) | 1): noise
 *   is on if N > 0 and rnd(w0, 1 << 24) < floor((double) noise_prob * 2^24), and then m = rnd(w1, N), the SNR index j = rnd(w2, J) and the
 *   offset off = rnd(w3, L_m).
 *   Fixed once per bank, on the host (ctcn_reverb_bank): per noise row P_m = S(q_m) / L_m; per RIR the peak p = the first index of the
 *   largest value of h_r and the early window [lo, hi) with lo = max(0, p - floor(0.001 fs)), hi = min(K, p + floor(0.05 fs)) (fs =
 *   sample_frequency, the products in double; an empty window -- fs below 20 Hz -- is refused); per SNR G_j = pow(10, -snr_j / 10) in double
 *   from the host's pow: no pow runs on the device.
 * Per utterance:
 *   1. P_in = S(x) / n.
 *   2. With an RIR: y[i] = fl32(sum_{k = 0 .. min(i, K - 1)} (double) h[k] * (double) x[i - k]) for i in [0, n), k ascending, the sum
 *      starting from +0.0 (a float32 x float32 product is exact in float64, so the sum is one number with or without fused multiply-adds;
 *      a result of zero is +0.0); the early signal e = x * h[lo .. hi) over its FULL length n + (hi - lo) - 1, by the same sum (only taps
 *      that meet a sample take part) and the same rounding; P_sig = S(e) / len(e).  Without an RIR: y = x and P_sig = P_in.
 *   3. With a noise row whose P_m > 0: g = sqrt((G_j * P_sig) / P_m) and z[i] = fl32((double) y[i] + g * (double) q[(off + i) mod L_m]) --
 *      the multiplication, the division, the square root, the product and the sum are float64 operations rounded one by one (no fused
 *      multiply-add on the device or the host).  Otherwise (noise off, or an all-zero row) z = y.
 *   4. With normalize: if P_out = S(z) / n > 0, s = sqrt(P_in / P_out) and out[i] = fl32(s * (double) z[i]); otherwise out = z.
 *   5. out[n .. Nmax) are zeros; nothing behind an utterance in its padded row, or behind a bank row's length, is ever read; n = 0 gives
 *      a row of zeros.
 * With both probabilities 0 the output has the input's bits (s = sqrt(P / P) = 1).  An utterance's result
 * depends on (seed, u, the options, the bank, its own samples) alone, not on B, Nmax or its neighbours.
 * The bank block (host, 4-byte words, 8-byte aligned): [0, 16) int32 a tag, R, N, J, the RIR row stride, the noise row stride, the longest
 * early window, 0, then the word offsets of the four tables and the block's size; R x (K, p, lo, hi) int32; N x L_m int32; (8-byte
 * aligned) N float64 P_m and 16 float64 G_j; R x stride float32 the impulse responses, zeros behind K; N x stride float32 the noises.
 * ctcn_reverb_bank_bytes: the block's size, 0 for shapes ctcn_reverb_bank refuses.  ctcn_reverb_bank: rirs (R, rir_stride) and noises
 * (N, noise_stride) padded rows on the HOST with their lengths; builds the block (no HIP call).
 * ctcn_reverb_plan: the draws of ONE utterance on the host from the host block: draws[4] = r or -1, m or -1, j, off (0, 0 without noise).
 * ctcn_reverb: wave, lens (B) int32, out (B, Nmax) float32 and ws in DEVICE memory, bank_host the block on the host (its header is read
 * there), bank_dev its copy in device memory; out must not alias wave.  Launches on the caller's stream, a launch boundary in front of each
 * phase that needs a sum over a whole utterance, no grid-wide barrier, no flag, no host synchronisation: the convolution (grid: tiles of
 * 2048 outputs and of the early signal x B; taps staged in LDS 1024 at a time, ascending, every lane owning eight consecutive outputs
 * with the input window sliding through its registers; the early signal is reduced to its power sums and never stored), the per-utterance
 * sums (P_in, P_sig, g), the noise addition with the sums of z^2, the sum to s, the scaling -- the last three only where the options need
 * them.  ws: ctcn_reverb_ws_bytes(bank_host, B, Nmax) bytes, 8-byte aligned (0 for bad arguments); too small: CTCN_EWORKSPACE.
 * ctcn_reverb_host: the same computation for ONE utterance on the HOST (no HIP call; works without a GPU), through the draw, gain, mix and
 * scale functions the kernels are compiled from: out (num_samples).
 * ctcn_reverb_limits: out[6] = outputs per tile (2048), taps per staged chunk (1024), elements per power-sum chunk (1024), the longest
 * impulse response (16 384), the most SNRs (16), outputs per lane (8).
 * Limits, from the bank builder before any launch: CTCN_EUNSUPPORTED for an RIR row stride beyond 16 384 taps, more than 16 SNRs, a noise
 * row beyond 2^30 samples, more than 2^20 rows; CTCN_EINVAL for NULL, both banks empty, a row length outside [1, stride], a value or an SNR
 * that is not finite, a noise bank without an SNR, a sample_frequency outside (0, 2^24].  From every entry point that takes the options:
 * CTCN_EINVAL for NULL or a probability outside [0, 1] (NaN included); from ctcn_reverb and ctcn_reverb_host: CTCN_EINVAL for a block
 * ctcn_reverb_bank did not build, B outside [1, 65 535], Nmax (num_samples) negative or beyond 2^30. */
typedef struct ctcn_reverb_opts {
  float rir_prob, noise_prob;
  int32_t normalize;
} ctcn_reverb_opts;
int ctcn_reverb_limits(int32_t *out);
size_t ctcn_reverb_bank_bytes(int R, int rir_stride, int N, int noise_stride, int num_snrs);
int ctcn_reverb_bank(const float *rirs, const int32_t *rir_len, int R, int rir_stride, const float *noises, const int32_t *noise_len, int N,
                     int noise_stride, const double *snrs, int num_snrs, double sample_frequency, void *bank, size_t bank_bytes);
int ctcn_reverb_plan(const void *bank, const ctcn_reverb_opts *opts, uint64_t seed, uint64_t utt_index, int32_t *draws);
size_t ctcn_reverb_ws_bytes(const void *bank_host, int B, int Nmax);
int ctcn_reverb(const void *wave, int wave_is_int16, const int32_t *lens, const void *bank_host, const void *bank_dev,
                const ctcn_reverb_opts *opts, uint64_t seed, uint64_t utt_offset, float *out, int B, int Nmax, void *ws, size_t ws_bytes,
                void *stream);
int ctcn_reverb_host(const void *wave, int wave_is_int16, int num_samples, const void *bank, const ctcn_reverb_opts *opts, uint64_t seed,
                     uint64_t utt_index, float *out);
/* Mean / variance normalisation per group of utterances and over a sliding window (cmvn.hip): the three Kaldi calls of a standard
 * recipe that ctcn_cmvn_accumulate and the mean / scale arguments of the feature kernels do not cover -- compute-cmvn-stats --spk2utt
 * (statistics per speaker), apply-cmvn --utt2spk (applied per utterance) and apply-cmvn-sliding.  A group is a speaker, or, with one id
 * per utterance, the utterance itself.  Kaldi's binaries do not run here; the definitions below restate its sources (transform/cmvn,
 * feat/feature-functions' SlidingWindowCmn) and fix the arithmetic, so that host, device and a numpy restatement agree bit for bit.
 * ctcn_cmvn_accumulate_groups: stats (G, 2, F + 1) DEVICE doubles, one statistics matrix of ctcn_cmvn_accumulate's layout per group; group
 * (B) int32 in DEVICE memory.  ADDS the rows t < frames[b] (clamped to [0, Tmax]) of utterance b to stats[group[b]]; an utterance whose id
 * is outside [0, G) contributes nothing, and nothing at or beyond frames[b] is read.  The 64-row float64 partial sums are those of
 * ctcn_cmvn_accumulate (the same kernel, the same workspace: ctcn_cmvn_accumulate_ws_bytes); a second launch with one thread per (group,
 * statistic) adds the partials of the group's utterances in ascending (utterance, block) order, starting from 0, and then that sum to
 * stats; the frame counts likewise in ascending utterance order.  A function of the input bits; with G = 1 and every id 0 it writes what
 * ctcn_cmvn_accumulate writes, bit for bit.  G at most 65 535.
 * ctcn_cmvn_apply: out (B, Tmax, F) = the rows of feats normalised with the statistics of the utterance's group, formed on the device (no
 * host round trip between accumulation and use).  Per group, with n = stats[g][0][F], in double, every operation rounded on its own (no
 * fused multiply-add) -- the formulas of utils/features.GlobalCMVN.mean_scale:
 *   m = sum / n, mean = fl32(m); v = max(sumsq / n - m * m, 1e-20), scale = fl32(1 / sqrt(v)), or 1.0f with norm_vars = 0;
 *   out = (x - mean) * scale, a float32 subtraction followed by a float32 multiplication: the feature kernels' expression.
 * Rows at or beyond frames[b] are written as zeros and never read, as in the padded batch the feature kernels return.  out may be feats
 * itself (in place), not a shifted overlap of it.  group == NULL: group 0 for every utterance.  An utterance whose id is outside [0, G), or
 * whose group has no frames (n <= 0), is copied through unnormalised.
 * ctcn_cmvn_sliding: Kaldi's SlidingWindowCmnOptions under their names with their defaults: cmn_window (600), min_cmn_window (100),
 * normalize_variance (false), center (false).  The window [s, e) of frame t in an utterance of n frames (SlidingWindowCmn's rule;
 * ctcn_cmvn_sliding_window states it on the host):
 *   1. center: s = t - cmn_window / 2, e = s + cmn_window; otherwise s = t - cmn_window, e = t + 1;
 *   2. s < 0: e -= s, s = 0;
 *   3. not center and e > t: e = max(t + 1, min_cmn_window);
 *   4. e > n: s -= e - n, e = n, s = max(s, 0).
 * So 0 <= s <= t < e <= n without center (a frame in the middle of a long utterance sees the cmn_window frames before it and itself:
 * cmn_window + 1 frames, as in Kaldi), and from one frame to the next either bound stays or advances by one.  Per (utterance, column), in
 * double: S and Q, the sums of x and of x * x ((double) x squared is exact) over the window.  At t = 0 they are summed over [s_0, e_0) in
 * ascending order from 0.  At t > 0, first frame s_{t-1} is subtracted if the start advanced, then frame e_{t-1} is added if the end
 * advanced.  With w = e - s and m = S / w:
 *   means only: out = fl32((double) x_t - m);
 *   normalize_variance and w > 1: v = max(Q / w - m * m, 1e-10), out = fl32(((double) x_t - m) * (1.0 / sqrt(v)));
 *   normalize_variance and w = 1: variance 1, out = fl32((double) x_t - m).
 * Every operation is rounded on its own; nothing is fused.  (Kaldi keeps the output in float32 and updates it as x + (-1 / w) S, and forms
 * the variance as Q / w - S^2 / w^2 followed by pow(-0.5): the same quantities, rounded at other points.)  Rows at or beyond frames[b] are
 * written as zeros and never read.  out must not overlap feats: the window reads frames behind the one it writes (CTCN_EINVAL).
 * cmn_window >= 1 and 1 <= min_cmn_window <= cmn_window are required in both modes (CTCN_EINVAL) -- stricter than Kaldi, which checks only
 * when centred.  One wave per (64 columns, utterance), lanes on the contiguous columns of a row; the chain in time is two float64
 * additions per frame, and the row loads are kept off it: the frames of ctcn_cmvn_sliding_run consecutive steps -- the frame itself, the one
 * leaving and the one entering the window -- are loaded into registers one run ahead of their use.
 * ctcn_cmvn_sliding_run: the frames of one such run under these options (16), or an error code.
 * ctcn_cmvn_sliding_window: the window of frame t < n on the HOST.  ctcn_cmvn_sliding_host: the computation for ONE utterance, feats and out
 * (num_frames, F), and ctcn_cmvn_norm_host: mean[F] and scale[F] of ONE statistics matrix (2, F + 1) with a positive count -- both on the
 * HOST (no HIP call; work without a GPU), through the functions the kernels are compiled from (cmvn_core.h).
 * Limits: CTCN_EINVAL for NULL, B outside [1, 65 535], Tmax outside [1, 2^30] (the host twin takes 0 frames), F or G below 1. */
typedef struct ctcn_sliding_cmn_opts {
  int32_t cmn_window, min_cmn_window, normalize_variance, center;
} ctcn_sliding_cmn_opts;
int ctcn_cmvn_accumulate_groups(const float *feats, const int32_t *frames, const int32_t *group, double *stats, int B, int Tmax, int F, int G,
                                void *ws, size_t ws_bytes, void *stream);
int ctcn_cmvn_apply(const float *feats, const int32_t *frames, const int32_t *group, const double *stats, float *out, int B, int Tmax, int F,
                    int G, int norm_vars, void *stream);
int ctcn_cmvn_sliding(const float *feats, const int32_t *frames, float *out, int B, int Tmax, int F, const ctcn_sliding_cmn_opts *opts,
                      void *stream);
int ctcn_cmvn_sliding_run(const ctcn_sliding_cmn_opts *opts);
int ctcn_cmvn_sliding_window(int t, int n, const ctcn_sliding_cmn_opts *opts, int32_t *start, int32_t *end);
int ctcn_cmvn_sliding_host(const float *feats, int num_frames, int F, const ctcn_sliding_cmn_opts *opts, float *out);
int ctcn_cmvn_norm_host(const double *stats, int F, int norm_vars, float *mean, float *scale);
/* Pitch features (pitch.hip, pitch_core.h): Kaldi's compute-kaldi-pitch-feats followed by process-kaldi-pitch-feats (Ghahremani et al.,
 * ICASSP 2014), the offline computation under Kaldi's option names and defaults (frames_per_chunk = 0, max_frames_latency = 0,
 * simulate_first_pass_online = false, nccf_ballast_online = false).  utils/features.PitchConfig / ProcessPitchConfig hold the defaults.
 * Refused by the plan builder with CTCN_EUNSUPPORTED (plan_bytes: 0) and again by every entry before any launch: snip_edges = false, a
 * preemphasis_coefficient other than 0, rates that are not whole numbers of Hz, min_f0 >= max_f0, more than 1024 lags, a lowpass_cutoff above
 * the Nyquist frequency of the lower rate, W + last lag beyond 8192 samples, more than 16 upsampling taps.  With fs = sample_frequency,
 * rf = resample_frequency:
 *   1. downsample: the waveform goes through ctcn_resample with orig_freq = fs, new_freq = rf, num_zeros = lowpass_filter_width, cutoff =
 *      lowpass_cutoff (LinearResample, flushed): M = ceil(N rf / fs) float32 samples.  ctcn_pitch takes THAT batch; ops.pitch does both.
 *   2. lags, in float32 as Kaldi's BaseFloat loop: lag = float(1 / max_f0); while lag <= float(1 / min_f0): keep it, lag = float(double(lag)
 *      (1 + double(delta_pitch))).  S lags (417 under the defaults).  Integer lags measured: first = ceil(rf (1 / max_f0 - ufw / (2 rf))) ..
 *      last = floor(rf (1 / min_f0 + ufw / (2 rf))), ufw = upsample_filter_width (8 .. 82).  W = int(rf frame_length / 1000), shift =
 *      int(rf frame_shift / 1000) (100, 40).
 *   3. frames: T = 0 for M < W, else (M - W) / shift + 1 (ctcn_pitch_frames takes N, the count at fs).  Frame t reads W + last samples from
 *      t shift; samples behind the utterance are zeros.  T may exceed the filterbank's count by one.
 *   4. correlation, in float64, sample order, every operation rounded on its own: mean = (sum of the first W samples) / W; v[i] = x[i] - mean
 *      over the whole window; e1 = sum v[i]^2, i < W; per integer lag l: e2 = sum v[l + i]^2, inner = sum v[i] v[l + i]; prod = e1 e2;
 *      nccf_pitch[l] = inner / sqrt(prod + ballast), nccf_pov[l] = inner / sqrt(prod), 0 where the square root is 0.  ballast =
 *      (var W)^2 nccf_ballast with var = Q / M - (S / M)^2 over the utterance's M downsampled samples, S and Q (sum, sum of squares) formed
 *      as 256 partial sums -- partial i takes samples i, i + 256, ... in order -- added in ascending order: one shape, no atomics.
 *   5. upsampling (Kaldi's ArbitraryResample: input rate rf, cutoff rf / 2, num_zeros = ufw): for lag i, t = double(lags[i]) - first / rf,
 *      fw = ufw / rf; taps j = max(ceil(rf (t - fw)), 0) .. min(floor(rf (t + fw)), last - first); d = t - j / rf; weight = filt(d) win(d)
 *      / rf rounded once to float32, win(d) = 0.5 (1 + cos(2 pi (rf / 2) / ufw d)) for |d| < fw, else 0, filt(d) = sin(2 pi (rf / 2) d) /
 *      (pi d), rf at 0.  Both rows: sum over the taps in order of double(weight) * nccf[j] (float64 product, then float64 sum), rounded to
 *      float32 ONCE -- the rows of step 4 stay float64 until here.
 *   6. Viterbi over the frames, float64: local[i] = (1 - n) + (soft_min_f0 lags[i]) n with n = double(nccf_pitch[i]); forward[i] =
 *      local[i] + min_j (prev[j] + pen[|i - j|]), pen[d] = d^2 c, c = log(1 + delta_pitch)^2 penalty_factor; prev = 0 before the first
 *      frame; the frame's minimum is subtracted from forward after every frame; backpointer = the LOWEST j that attains the minimum (the
 *      minimum and that j do not depend on the order of evaluation; Kaldi's bound-tightening search reaches the same minimum, its choice
 *      among exact float ties is not reproduced).  After the last frame the lowest-index arg-min of forward starts the walk back.
 *   7. raw output, one row per frame: [nccf_pov at the chosen lag, float32(1) / lags[chosen]].
 *   8. post-processing (ctcn_pitch_process) in float64, rounded once; columns in this order, each if asked for:
 *      POV feature: pov_scale (pow(1.0001 - n, 0.15) - 1) + pov_offset, n clipped to [-1, 1];
 *      normalised log pitch: pitch_scale (log p_t - sum_w(pov log p) / sum_w(pov)) over the frames [t - left, t + right] inside the
 *        utterance in ascending order, pov = 1 / (1 + exp(-r)), r = -5.2 + 5.4 exp(7.5 (a - 1)) + 4.8 a - 2 exp(-10 a) + 4.2 exp(20 (a - 1)),
 *        a = min(|n|, 1);
 *      delta log pitch: delta_pitch_scale (sum_k s[k] log p[clamp(t + k)] + delta_pitch_noise_stddev g), s = ctcn_delta_scales of order 1 and
 *        delta_window, g a unit Gaussian from Philox keyed by (seed, utterance index, frame) as the filterbank's dither (sample 0);
 *      raw log pitch.
 *      Refused: delay other than 0, a context beyond 1500 frames, delta_window outside [1, 5] (CTCN_EUNSUPPORTED); no column (CTCN_EINVAL).
 *   9. pasting to base features (paste-feats --length-tolerance) is host glue: utils/features.paste_features.
 * Steps 4 to 7 agree bit for bit between the kernels, ctcn_pitch_host and the restatement tests/pitch_ref.py; step 8 goes through pow, exp
 * and log and is held to a tolerance.
 * The plan block (host, 4-byte words, 8-byte aligned): [0, 16) int32 S, first, last, W, shift, the tap row stride, the frames of
 * backpointers the walk back stages at a time, last - first + 1, zeros; then S float lags; S float 1 / lag; S int32 first tap (relative to
 * `first`); S int32 tap counts; S x stride float weights; a pad word if needed for alignment; S double soft_min_f0 lags[i]; S double pen[d].
 * ctcn_pitch: wave (B, Mmax) float32 at rf, lens (B) int32 clamped to [0, Mmax]; plan in DEVICE memory; out (B, Tmax, 2) float32, rows at
 * or beyond frames[b] zero; lag_index (B, Tmax) int32 or NULL: the chosen state per frame; frames (B) int32; ws of
 * ctcn_pitch_workspace_bytes (256-byte aligned: the ballast, the two float32 correlation planes, 16-bit backpointers).  Tmax at most the
 * frames Mmax samples hold.  Three launches: the sums, the correlation and upsampling, the search with its walk back (one workgroup per utterance).
 * ctcn_pitch_host: ONE utterance on the host (no HIP call), plan the host block; returns the frame count.  ctcn_pitch_process: raw
 * (B, Tmax, 2) -> out (B, Tmax, C), C the number of columns asked for, rows at or beyond frames[b] zero; utterance b draws its noise from
 * (seed, b + utt_offset).  ctcn_pitch_process_host: one utterance of num_frames frames; returns C. */
typedef struct ctcn_pitch_opts {
  float sample_frequency, frame_length, frame_shift, preemphasis_coefficient, min_f0, max_f0, soft_min_f0, penalty_factor, lowpass_cutoff,
      resample_frequency, delta_pitch, nccf_ballast;
  int32_t lowpass_filter_width, upsample_filter_width, snip_edges;
} ctcn_pitch_opts;
typedef struct ctcn_pitch_process_opts {
  float pitch_scale, pov_scale, pov_offset, delta_pitch_scale, delta_pitch_noise_stddev;
  int32_t normalization_left_context, normalization_right_context, delta_window, delay, add_pov_feature, add_normalized_log_pitch,
      add_delta_pitch, add_raw_log_pitch;
} ctcn_pitch_process_opts;
int ctcn_pitch_frames(long long num_samples, const ctcn_pitch_opts *opts);
size_t ctcn_pitch_plan_bytes(const ctcn_pitch_opts *opts);
int ctcn_pitch_plan(const ctcn_pitch_opts *opts, void *plan, size_t plan_bytes);
size_t ctcn_pitch_workspace_bytes(const ctcn_pitch_opts *opts, int B, int Tmax);
int ctcn_pitch(const float *wave, const int32_t *lens, const ctcn_pitch_opts *opts, const void *plan, float *out, int32_t *lag_index,
               int32_t *frames, int B, int Mmax, int Tmax, void *ws, size_t ws_bytes, void *stream);
int ctcn_pitch_host(const float *wave, int num_samples, const ctcn_pitch_opts *opts, const void *plan, float *out, int32_t *lag_index,
                    int out_cap);
int ctcn_pitch_process(const float *raw, const int32_t *frames, const ctcn_pitch_process_opts *opts, float *out, int B, int Tmax,
                       uint64_t seed, uint64_t utt_offset, void *stream);
int ctcn_pitch_process_host(const float *raw, int num_frames, const ctcn_pitch_process_opts *opts, uint64_t seed, uint64_t utt_index,
                            float *out);

/* ---------------------------------------------------------------------------------------------------
 * CTC prefix beam search with bigram LM; replaces BeamDecoder.decode -> ctcBeamSearch.decode
 * (ctcDecoder.py:181-192; BeamSearch.py:73-153).  One workgroup per utterance.
 *   x (T,B,V) float32: log-probs (input_is_prob==0, exp taken on device) or probabilities exp(lp)
 *   lens (B) int32; lm ((V+1)*(V+1)) float64 ln-probs, row V = '<s>', column V = '</s>'
 *   out_ids (B,T) int32, out_len (B) int32, out_score (B) float64 (length-normalised prTotal)
 *   status (B) int32: 0 ok, 1 best labelling empty (reference raises IndexError), 2 log(0) (ValueError), 3 node table of the workspace
 *   exhausted, 4 internal hand-over between the waves of the search timed out (a bug, never seen; outputs zeroed for 2..4)
 *   ws: >= ctcn_beam_ws_bytes(T,B,V,W)
 *   1 <= W <= 1 024 (round 6; was 256): the reference takes any beam_width (ctcDecoder.py:170, default 200).  W <= 60 with W*V <= 3 328 runs
 *   the restructured search, everything else the generic kernel, whose beam state sits in dynamic LDS sized for W (146 KB at W = 1 024);
 *   wider beams: CTCN_EUNSUPPORTED. */
size_t ctcn_beam_ws_bytes(int T, int B, int V, int W);
int ctcn_beam_decode(const float *x, int input_is_prob, const int32_t *lens, const double *lm, double alpha,
                     int W, int blank, int32_t *out_ids, int32_t *out_len, double *out_score, int32_t *status,
                     int T, int B, int V, void *ws, size_t ws_bytes, void *stream);
/* The same search returning the `nbest` (1 <= nbest <= W) best labellings of every utterance: the first nbest entries of the final
 * `last.sort()` of BeamSearch.py:150, of which the reference keeps element [0] ("optional n-best output") -- a stable
 * descending sort by the length-normalised score, entry 0 = what ctcn_beam_decode returns.
 *   out_ids (B,nbest,T) int32, out_len (B,nbest) int32, out_score (B,nbest) float64; out_count (B) int32 or NULL: labellings actually
 *   returned for the utterance (the final beam can hold fewer than nbest; the remaining entries have length 0 and score 0) */
int ctcn_beam_decode_nbest(const float *x, int input_is_prob, const int32_t *lens, const double *lm, double alpha,
                           int W, int blank, int nbest, int32_t *out_ids, int32_t *out_len, double *out_score,
                           int32_t *out_count, int32_t *status, int T, int B, int V, void *ws, size_t ws_bytes, void *stream);
/* The same search with a language model of order `lm_order`:
 *   2: lm is the (V+1)^2 table above -- the launches and the bits of ctcn_beam_decode_nbest (which is this call with lm_order = 2);
 *   3: lm is ((V+1)^3) float64 ln-probs tri[c0][c1][k] = ln P(k | c0, c1); index V = '<s>' for c0 and c1, '</s>' for k.  The LM term of an
 *      extension of labelling y by class k (and of the final step, k = V) is tri[V][V][k] for len(y) == 0, tri[V][y[0]][k] for len(y) == 1,
 *      tri[y[-2]][y[-1]][k] beyond; everything else is the search above, on the same paths (the fast kernel and its occ2 builds where
 *      order 2 takes them, the generic kernel elsewhere: every width 1..1 024; the order is a template parameter of both).  The table
 *      stays in global memory (63^3 doubles = 2.0 MB sit in an XCD's L2); every beam slot carries one class more (154 KB of LDS at
 *      W = 1 024).  All paths return the same bits, and a context-free table (tri[c0] = lm for every c0) the bits of order 2.  A table
 *      beyond 64 MiB (V > 202) and any other order: CTCN_EUNSUPPORTED before any launch.  Cost: DESIGN section 7s.
 *   ws: >= ctcn_beam_ws_bytes(T,B,V,W) for either order; out_count may be NULL; nbest = 1 gives ctcn_beam_decode's outputs. */
int ctcn_beam_decode_lm(const float *x, int input_is_prob, const int32_t *lens, const double *lm, int lm_order, double alpha,
                        int W, int blank, int nbest, int32_t *out_ids, int32_t *out_len, double *out_score,
                        int32_t *out_count, int32_t *status, int T, int B, int V, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * RNN language model and n-best rescoring (lm.hip; the reference's to-do list names both, it has neither).  The model's recurrent layers,
 * BatchNorm, output product and log-softmax are the entry points above; these are the kernels in front of and behind them.  Integer inputs
 * are int32; float operands need 4-byte alignment only (16-byte paths are taken where pointers and row lengths allow), float64 ones 8.
 * `status` is ONE device int32 the kernels OR bits into (1: an embedding id outside [0, V); 2: a target outside [0, V)); the caller clears
 * it and reads it where it synchronises anyway.  Every product, sum and quotient named below is rounded on its own (no fused multiply-add),
 * and no float is ever added atomically: each result is a function of the inputs' bits.
 *
 * Embedding, forward: y (N,E) = table (V,E) rows by ids (N).  A row whose id is padding_idx (-1: none) is zeros; an id outside [0, V)
 * never indexes the table: its row is zeros and status bit 1 is raised. */
int ctcn_embedding_fwd(const int32_t *ids, const float *table, float *y, int N, int V, int E, int padding_idx, int32_t *status, void *stream);
/* Embedding, backward: dtable[v,:] = beta * dtable[v,:] + s_v, where s_v = ((dy[n0,:] + dy[n1,:]) + dy[n2,:]) + ... over the rows
 * n0 < n1 < ... with ids[n] == v, float32 additions in that order (the order is the definition: the result equals a host loop bit for bit).
 * beta is 0 (dtable is not read: s_v, or zeros for an empty list) or 1 (accumulate, as the weight gradients of ctcn_gemm do).  The
 * padding_idx row and rows no id names get beta * dtable[v,:]; ids outside [0, V) contribute nothing.  ws: the workspace bytes query
 * below (a stable counting sort of the rows by id: 8 N + 4 (V + 1) + 4 ceil(N / 256) V bytes plus padding; 0 for bad arguments or beyond
 * 2^30 counters), 4-byte aligned; too small: CTCN_EWORKSPACE. */
size_t ctcn_embedding_bwd_ws_bytes(int N, int V);
int ctcn_embedding_bwd(const int32_t *ids, const float *dy, float *dtable, int N, int V, int E, int padding_idx, float beta, void *ws,
                       size_t ws_bytes, void *stream);
/* Negative log-likelihood over log-probs: lp (T*B, V) time-major, the output of the log-softmax entry point; tgt (T*B) int32.
 *   tok (T*B) float32 = -lp[n, tgt[n]]; 0 for tgt[n] == ignore_index; +inf for a log-prob of -inf (as torch)
 *   seq_sum (B) float64 = sum over t ascending of (double)tok[t,b]; total (1) float64 = sum over b ascending of seq_sum[b]
 *   count (1) int32 = rows whose target is not ignore_index
 * A target outside [0, V) that is not ignore_index contributes 0 and raises status bit 2. */
int ctcn_nll_fwd(const float *lp, const int32_t *tgt, int T, int B, int V, int ignore_index, float *tok, double *seq_sum, double *total,
                 int32_t *count, int32_t *status, void *stream);
/* Gradient of that loss with respect to the logits the log-probs came from: dz[n,v] = g_n * (exp(lp[n,v]) - [v == tgt[n]]), float32 expf,
 * one subtraction, one product; rows that are ignored or whose target is outside [0, V) are zeros; exp(-inf) = 0, never NaN.
 * g_n = g[n * g_stride]: stride 0 = the scalar upstream gradient of 'sum' / 'mean' (read on the device), stride 1 = reduction 'none'.
 * count != NULL: g_n is divided by max(*count, 1) first ('mean'; the count stays on the device).  One read of lp, one write of dz; a wave
 * per row for V <= 512, a workgroup per row above. */
int ctcn_xent_bwd(const float *lp, const int32_t *tgt, float *dz, int N, int V, int ignore_index, const float *g, int g_stride,
                  const int32_t *count, void *stream);
/* From the n-best search's out_ids (B,N,T), out_len (B,N), count (B) to the LM's time-major batch of S = B*N sequences of L + 1 steps
 * (L <= T: the longest labelling, which the caller has read): sequence s = (b,k) of length l has in_ids[:, s] = [boundary, y_1 .. y_l,
 * 0 ...], tgt[:, s] = [y_1 .. y_l, boundary, ignore_index ...] and lens[s] = l + 1.  A slot k >= count[b] is the empty sequence
 * (lens = 1): no sequence has zero steps.  Lengths are clamped to [0, min(L, T)]. */
int ctcn_lm_pack_nbest(const int32_t *out_ids, const int32_t *out_len, const int32_t *count, int B, int N, int T, int L, int boundary,
                       int ignore_index, int32_t *in_ids, int32_t *tgt, int32_t *lens, void *stream);
/* The rescored winner per utterance: over k < count[b], in float64, t_k = (score[b,k] + weight * lm[b,k]) + len_bonus * out_len[b,k];
 * the largest t_k wins, the lowest k on ties.  best_ids (B,T) = its ids with zeros behind its length, best_len (B), best_score (B) = t_k,
 * best_k (B).  count[b] == 0: length 0, score 0, best_k = -1.  score, lm (B,N) float64. */
int ctcn_rescore_select(const double *score, const double *lm, const int32_t *out_len, const int32_t *count, const int32_t *out_ids,
                        double weight, double len_bonus, int B, int N, int T, int32_t *best_ids, int32_t *best_len, double *best_score,
                        int32_t *best_k, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Diagnostics (not on the compute path).
 * ctcn_diag_squat: `wgs_per_xcd` workgroups of `threads` threads (+ `lds_bytes` of LDS each) on every XCD that only hold their CU
 * slots for `usec` microseconds (clock-bounded, <= 5 s) -- what an RCCL kernel waiting for a slow peer looks like to the rest of the
 * chip.  The data-parallel co-residency contract of the persistent recurrences is tested against it.
 * ctcn_rnn_last_kernel: name of the recurrent kernel the most recent ctcn_rnn_fwd (which = 0) / ctcn_rnn_bwd (which = 1) of this
 * PROCESS launched ("rnn_fwd_tagged", "rnn_fwd_persist", "rnn_fwd_step", "rnn_bwd_scatter", "rnn_bwd_scatter2", "rnn_bwd_persist",
 * "rnn_bwd_step"; "" before the first call).  The one piece of state the library keeps between compute calls: two atomic pointers to
 * string literals (relaxed; with several calling threads the last writer wins -- the backward pass of autograd runs on another thread
 * than the reader, which is why it is not thread-local), read by nothing on the compute path. */
int ctcn_diag_squat(int wgs_per_xcd, int threads, int lds_bytes, unsigned usec, void *stream);
/* ctcn_diag_pipeline_chunks: the plan of the projection pipeline (ctcn_rnn_call.side_stream of ctcn_rnn_fwd_ex) for a layer shape on a device
 * of `xcds` XCDs and `cus` CUs with the idle XCDs `xcd_allow`: the number of time chunks (even, 8..24) it would be pipelined with, 0 = not
 * pipelined (the one-round / 72-steps / throughput / free-CU rules of rnn.hip), -1 = bad arguments.  Pure arithmetic, no device needed. */
int ctcn_diag_pipeline_chunks(int cell, int T, int B, int I, int H, int dirs, int xcds, int cus, unsigned xcd_allow);
/* ctcn_diag_gemm_plan: what ctcn_gemm (and the internal side-stream / shifted forms: xcd_allow, b_shift, same_a / same_b = the operand's bf16
 * planes of the previous call are still in the workspace) would do with a product on a device of `xcds` XCDs and `cus` CUs, given A and B
 * modulo 16 bytes and the workspace's size -- the plan of gemm.hip's plan_gemm under the current options.  out[CTCN_GEMM_PLAN_INTS] =
 * path (0 f32, 1 f32 queued, 2 bf16x3 direct, 3 planes 128-row tile, 4 the same queued, 5 planes 256-row tile, 6 256-row tile with float32 A,
 * 7 256-row tile queued, 8 TN tile), workgroup tile rows / 64, columns / 64, wnt, split-K count, k-chunk, split pass of A, of B (0 none,
 * 1 rows, 2 transposing, 3 transposing queued), grid x, grid y, 16-B loads of A, of B (direct kernels).  CTCN_EINVAL on the arguments
 * ctcn_gemm refuses.  Pure arithmetic, no device needed.
 * ctcn_diag_gemm_on_xcds: ctcn_gemm with its workgroups confined to the XCDs of `xcd_allow` (0: ctcn_gemm itself) -- the side-stream forms
 * the recurrent layer uses, for tests.
 * ctcn_diag_gemm_shift_b_pair: the weight-gradient pair of a recurrent layer, for tests: C1 (M x N1) = A^T B1, then C2 (M x N2) =
 * A2^T shift_k(B2) with B2's rows delayed (shift > 0) or advanced (shift < 0) by |shift| < K contraction steps, zeros shifted in; A, A2
 * (K x M, lda), B1, B2 (K x N). Both run in one sequence; reuse != 0 asks the second product to take A's bf16 planes from the first;
 * reuse == 2 also overwrites A's K x M window with NaN between the two products (the second then must not read A: pass A2 == A). */
#define CTCN_GEMM_PLAN_INTS 12
int ctcn_diag_gemm_plan(int transA, int transB, int M, int N, int K, int lda, int ldb, int ldc, int precision, int b_shift, int a_mod16,
                        int b_mod16, int has_ws, size_t ws_bytes, unsigned xcd_allow, int same_a, int same_b, int cus, int xcds, int *out);
int ctcn_diag_gemm_on_xcds(int transA, int transB, int M, int N, int K, const float *A, int lda, const float *B, int ldb, float *C, int ldc,
                           float beta, int precision, void *ws, size_t ws_bytes, void *stream, unsigned xcd_allow);
int ctcn_diag_gemm_shift_b_pair(int M, int N1, int N2, int K, const float *A, int lda, const float *B1, int ldb1, float *C1, int ldc1,
                                const float *A2, const float *B2, int ldb2, float *C2, int ldc2, float beta, int precision, void *ws,
                                size_t ws_bytes, void *stream, unsigned xcd_allow, int shift, int reuse);
/* ctcn_diag_dx_plan: what ctcn_gemm_dx would do on a device of `cus` CUs under the current options, given A modulo 16 bytes and the
 * workspace's size: out[CTCN_DX_PLAN_INTS] = eligible for the 256 x 320 tile, takes it, tiles_wide (0 when not eligible), tiles_128.
 * Pure arithmetic, no device needed. */
#define CTCN_DX_PLAN_INTS 4
int ctcn_diag_dx_plan(int M, int N, int K, int lda, int precision, int a_mod16, int has_ws, size_t ws_bytes, int cus, int *out);
/* ctcn_diag_beam_plan: what ctcn_beam_decode would do with a (T,B,V) batch at beam width W under the current options (beam_fast, beam_occ2,
 * beam_generic_threads, beam_cand_global) on a device that gives one workgroup `lds_max` bytes of LDS, the generic kernel taking
 * `generic_static_lds` of them as static LDS (the decode call asks the runtime for both) -- the plan of decode.hip's plan_beam.
 * out[CTCN_BEAM_PLAN_INTS] = path (0 fast kernel, 1 its occ2 build, 2 generic kernel); the fast kernel's fit whichever path is taken: fits,
 * candidate slots per thread (0: too many), LM table in LDS, LDS trie slots, dynamic LDS bytes; the generic kernel: threads, beam-state
 * capacity, survivor-list capacity, candidate table in LDS, LM table in LDS, dynamic LDS bytes, static + dynamic LDS within lds_max; trie
 * nodes per utterance, slots of the global hash table; the workspace of the fast and of the generic path, each as (bytes & 0x7fffffff,
 * bytes >> 31) -- ctcn_beam_ws_bytes is the larger.  CTCN_EINVAL on bad arguments, CTCN_EUNSUPPORTED (out filled) where the decode call
 * answers it: the generic kernel is taken and its LDS does not fit.  Pure arithmetic, no device needed. */
#define CTCN_BEAM_PLAN_INTS 19
int ctcn_diag_beam_plan(int T, int B, int V, int W, int lds_max, int generic_static_lds, int *out);
/* ... of ctcn_beam_decode_lm at LM order `lm_order`; 2 gives ctcn_diag_beam_plan's answer.  CTCN_EUNSUPPORTED (out untouched) for an order
 * other than 2 or 3 and for an order-3 table beyond the cap. */
int ctcn_diag_beam_plan_lm(int T, int B, int V, int W, int lm_order, int lds_max, int generic_static_lds, int *out);
/* ctcn_diag_ctc_lattice_plan: the launch of a CTC lattice pass over label rows of Lmax symbols (S = 2 Lmax + 1 states) under the current
 * "ctc_lattice_skew" -- the plan of ctc.hip's plan_ctc_lattice.  out[CTCN_CTC_LATTICE_PLAN_INTS] = skewed (1) or classic (0) kernel, waves of
 * 64 states that cover the lattice (ceil(S / 64)), states per thread, threads per workgroup, dynamic LDS bytes, and the skew of the skewed
 * kernel in frames per wave (a constant of the build).  CTCN_EINVAL on bad arguments.  Pure arithmetic, no device needed. */
#define CTCN_CTC_LATTICE_PLAN_INTS 6
int ctcn_diag_ctc_lattice_plan(int Lmax, int *out);
const char *ctcn_rnn_last_kernel(int which);

/* ---- host end of the decoders (hostjoin.hip; no kernel, no HIP call: works without a GPU) -------------------------------------------------
 * replaces: `' '.join(self.classes[k] for k in labelling)` (BeamSearch.py:152-153; ctcDecoder.py:60-118 for the greedy decoder), once per
 * utterance of a decoded batch.  ids: B rows of `row_stride` int32 label ids (the pinned copy of ctcn_beam_decode's out_ids), lens[b] valid
 * per row; words / word_off[V] / word_len[V]: the vocabulary's UTF-8 bytes back to back, followed by 16 readable bytes, the byte offset and
 * the byte length of every word (word_len[k] < 0: id k has no word); sep: the byte between two words (0: none).  Writes row b's string to
 * out[out_off[b] .. out_off[b + 1]) and returns out_off[B]; CTCN_EINVAL on bad arguments, CTCN_EWORKSPACE when out_cap is too small (result + 17 bytes), -(16 + k) for an id k outside the vocabulary (the KeyError /
 * IndexError of the Python expression). */
long long ctcn_join_tokens(const int32_t *ids, long long row_stride, const int32_t *lens, int B, const char *words, const int32_t *word_off,
                           const int32_t *word_len, int V, int sep, char *out, long long out_cap, long long *out_off);
/* ctcn_levenshtein: unit-cost edit distance of two int32 sequences (the code points of two strings, or word ids), host code.
 * replaces: Decoder._edit_distance (ctcDecoder.py:131-150; cer :127-129 and wer :118-125 call it once per decoded utterance).  -1 on bad
 * arguments. */
long long ctcn_levenshtein(const int32_t *a, long long na, const int32_t *b, long long nb);
/* ctcn_levenshtein_ops: the alignment behind ctcn_levenshtein, by the move rule of ctcn_edit_ops (diagonal, then deletion, then insertion), host
 * code: word- and string-level scoring, and the decode driver, whose hypotheses are on the host already.  counts4 = (sub, del, ins, cor);
 * ali (nh + nr, 2) int32 or NULL: the (reference, hypothesis) pairs in forward order, -1 = none, (-1, -1) past the last pair.  Returns the
 * number of pairs; CTCN_EINVAL on bad arguments (a NULL counts4 is one). */
long long ctcn_levenshtein_ops(const int32_t *hyp, long long nh, const int32_t *ref, long long nr, long long *counts4, int32_t *ali);

#ifdef __cplusplus
}
#endif
#endif
