/*
 * s2vt.h -- C ABI of libs2vt_hip.so: the MI355X-native S2VT REINFORCE hot path.
 *
 * The reference (adwardlee/multitask-end-to-end-video-captioning) has no FFI layer: its boundary
 * is the Python class Video_Caption_Generator whose build_* methods emit TensorFlow-1.1 graph ops
 * (tf_s2vt.py:53-266, reinforcement_multisampling_tf_s2vt.py:63-466).  Each entry point below
 * replaces the TF ops of one stretch of those graphs; the reference lines are cited per function.
 * INTEGRATION.md shows the ctypes binding and how Video_Caption_Generator.build_* map onto it.
 *
 * Conventions
 *   - Plain C: pointers, sizes, POD structs.  No torch / TF types.  All tensors are row-major
 *     fp32 (token ids int32), DEVICE pointers owned by the caller; the library allocates nothing
 *     on the device -- scratch comes from a caller-provided workspace (query *_workspace_bytes).
 *   - Every call takes a hipStream_t (as void*) and is asynchronous w.r.t. the host; no hidden
 *     synchronisation.  The core API is handle-free (all state is in the arguments); the session
 *     API at the end wraps the samplers around a handle that owns its workspace.
 *   - Return value: 0 = S2VT_OK, < 0 = S2VT_E_*.  Never throws, never exits.  After
 *     S2VT_E_HIP, s2vt_last_hip_error() holds the hipError_t.
 *   - Numeric contract: forward contractions are ascending-k fp32 fmaf chains on
 *     v_mfma_f32_16x16x4_f32, transcendental functions are fixed instruction sequences, sampling
 *     is Gumbel-max over Philox4x32-10 -- forward activations, logits and token ids are
 *     bit-identical to oracle/s2vt_oracle.c.  Gradients / reductions are order-free fp32.
 *   - Fast path: pointers 16-byte aligned, leading dimensions and K / N multiples of 4.  Matrices may be any size
 *     (operands are addressed per tile); a gather table passed as rowidx / token ids, a broadcast block (rowmod)
 *     and the weight matrix must each fit a 2 GiB window.  Anything else takes a scalar path with identical results.
 */
#ifndef S2VT_H
#define S2VT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S2VT_OK 0
#define S2VT_E_BADARG (-1)   /* null pointer, non-positive size, inconsistent dims */
#define S2VT_E_ALIGN (-2)    /* workspace not 256-byte aligned */
#define S2VT_E_WORKSPACE (-3)/* workspace too small */
#define S2VT_E_HIP (-4)      /* a HIP call failed: see s2vt_last_hip_error() */
#define S2VT_E_CHAIN_TIMEOUT (-5) /* a persistent recurrence timed out earlier (starved of CUs): activations since are suspect, variable
                                     updates queued behind it were SKIPPED on the device; see s2vt_chain_fault / s2vt_chain_ack */

typedef void* s2vt_stream;   /* hipStream_t */

/* Model dimensions: the constructor arguments of Video_Caption_Generator (tf_s2vt.py:54-66). */
typedef struct s2vt_dims {
    int32_t dim_image;            /* d   = 1536 */
    int32_t n_words;              /* |V|        */
    int32_t word_dim;             /* E   = 500  */
    int32_t lstm_dim;             /* H   = 1000 */
    int32_t n_video_lstm_step;    /* Tv  = 5    */
    int32_t n_caption_lstm_step;  /* Tc  = 20 (35 in the reference files) */
    int32_t label_dim;            /* A   = 400 attributes (multitask head), 0 if absent */
    int32_t reserved;             /* model bits: 0 = tf_s2vt.py, or S2VT_MODEL_RESIDUAL (the field keeps its name: the struct is unchanged) */
} s2vt_dims;

/* Model bit in s2vt_dims.reserved: the residual captioner of residual_tf_s2vt.py.  At every decode step (build_model :149-151,
 * build_generator :206-208, build_sampler :263-265) output2 = output1 + output2 before logit_words = xw_plus_b(output2, embed_word_W,
 * embed_word_b); nothing else differs from tf_s2vt.py -- same variables, same checkpoint layout.  Contract:
 * s = fl32(o1 + o2), one fp32 addition per element; o1 = LSTM1's DropoutWrapper output of that decode step (dropped, code 256 + step, in the
 * training unroll; undropped in samplers, generator and beam search), o2 = LSTM2's; LSTM2's recurrent state stays the un-summed h'; the
 * logits are the same ascending-k chain on s.  Backward: dWout = s^T dlogits, and ds = dlogits Wout^T reaches LSTM2 as before AND is added to
 * the gradient w.r.t. LSTM1's dropped output of the decode steps.
 *   Honoured by: s2vt_sample / _ex, s2vt_beam_encode / _step, s2vt_teacher_forced_fwd (+ _reuse / _steps / _live), s2vt_bptt_bwd (+ _phase /
 *     _steps / _live / _bf16 / _split) and their workspace-size functions.  The sampler workspace grows by one [R, H] float block, the beam
 *     workspace by [B beam, H] floats + [B beam] int32, each rounded up to 256 bytes, behind the plain regions; the training workspace and the
 *     bf16 / split scratch do not change.  A residual model's sampler always takes per-step launches (no persistent decode loop).
 *   Accepted, same behaviour (no logits there, or they only read what the calls above leave): s2vt_frame_embed_fwd / _bwd, s2vt_bptt_dvideo,
 *     s2vt_split_grad_dlogits_planes, s2vt_softmax_nll_fwd_bwd_split, s2vt_bf16_grad_workspace_bytes, s2vt_split_grad_workspace_bytes.
 *   Every other entry point that takes s2vt_dims (s2vt_sample_mix, s2vt_scheduled_fwd, s2vt_averaged_fwd / _bptt_bwd, s2vt_topk_feed_fwd / _bptt_bwd / _decode, s2vt_create and the handle calls, every s2vt_attn_*)
 *     returns S2VT_E_BADARG (size functions: 0) when the bit is set.  Any other bit: S2VT_E_BADARG / 0 everywhere. */
#define S2VT_MODEL_RESIDUAL 1

/* Trainable variables (tf_s2vt.py:68-88; LSTM kernels are created lazily by BasicLSTMCell under
 * s2vt/LSTM{1,2}/basic_lstm_cell/{weights,biases}).  The same struct carries gradients. */
typedef struct s2vt_params {
    float* Wemb;            /* [V, E]                                                    */
    float* encode_image_W;  /* [d, E]                                                    */
    float* encode_image_b;  /* [E]                                                       */
    float* lstm1_W;         /* [E + H, 4H]   rows [x ; h], columns [i | j | f | o]       */
    float* lstm1_b;         /* [4H]                                                      */
    float* lstm2_W;         /* [H + E + H, 4H] rows [out1 ; embed ; h2]                  */
    float* lstm2_b;         /* [4H]                                                      */
    float* embed_word_W;    /* [H, V]                                                    */
    float* embed_word_b;    /* [V]                                                       */
    float* attr_W;          /* [d, A] or NULL (reinforce_multitask_e2e_attribute_loss.py:112-114) */
    float* attr_b;          /* [A]    or NULL                                            */
} s2vt_params;

/* ---- library info / errors --------------------------------------------------------------- */
int s2vt_version(void);
/* bit 0: built with EXPERIMENTAL=1 (the opt-in decode-loop experiments decode4.hip / decode_loop.hip are linked in). */
int s2vt_build_flags(void);
int s2vt_last_hip_error(void);
/* Up to 8 device buffers set to zero by ONE launch (4-byte aligned, byte counts multiples of 4): the gradient bucket and the
 * other buffers a step must find zeroed -- each hipMemsetAsync / tensor-library fill is a ~5-20 us launch of its own. */
int s2vt_zero_regions(void* const* ptrs, const size_t* bytes, int32_t count, s2vt_stream stream);
const char* s2vt_error_string(int code);

/* ---- launch profiler (measurement only; bench.py's roofline leg) ---------------------------------
 * While enabled, every contraction launch is bracketed by two hipEvents recorded on the stream the
 * kernel is launched on and tallied per (kernel class, tile configuration) with its flops
 * (2*M*K*N of that launch, structural-zero segments excluded).  Call s2vt_prof_collect only after
 * synchronising the stream(s); it returns the number of rows written and resets the tally.
 * kernel_class: 0 = STORE contraction, 1 = fused LSTM cell, 2 = vocab logits + pick, 3 = TN weight grad. */
typedef struct s2vt_prof_row {
    int32_t kernel_class;
    int32_t tile_cfg;
    int64_t launches;
    double total_ms;
    double total_flops;
    char name[32];
} s2vt_prof_row;
int s2vt_prof_enable(int on);
/* Restrict the event brackets to one (kernel_class, tile_cfg); -1 = any.  Two events per launch cost ~1.5 us of
 * stream time each, ~10 % of a 600-launch step: bench.py profiles every launch during warm-up to find the dominant
 * kernel and only that kernel inside the timed region. */
int s2vt_prof_filter(int kernel_class, int tile_cfg);
int s2vt_prof_collect(s2vt_prof_row* rows, int max_rows);

/* ---- test hook: evaluate the contract's scalar functions on the device --------------------
 * fn: 0 exp, 1 log, 2 tanh, 3 sigmoid.  y[i] = fn(x[i]).  (Bitwise comparison with the oracle.) */
int s2vt_math_eval(int fn, const float* x, float* y, int64_t n, s2vt_stream stream);
/* Gumbel noise words of the sampler stream for (video, sample, step), columns [0, V). */
int s2vt_gumbel_eval(uint64_t seed, int32_t video, int32_t sample, int32_t step, float* out, int32_t V,
                     s2vt_stream stream);
/* Both Gumbel forms of the sampler on given Philox words: exact[i] = the fixed-sequence value that decides a token
 * (-log(-log(u)), u = ((words[i] >> 9) + 0.5) 2^-23), fast[i] = the two-hardware-log value the pick screens compare
 * under kGumbelScreenMargin (csrc/detmath.h).  Only the top 23 bits of a word count: 2^23 words cover the domain.
 * NULL or n < 0: S2VT_E_BADARG; n == 0: nothing is launched. */
int s2vt_gumbel_words_eval(const uint32_t* words, float* exact, float* fast, int64_t n, s2vt_stream stream);

/* ---- tf.nn.xw_plus_b / tf.matmul over a concatenated operand -------------------------------
 * C[m, :] = act( chain over [A0[r0(m)] ; A1[r1(m)] ; A2[r2(m)]] @ W  (+ bias) ), the chain
 * optionally continuing from Cinit.  Replaces tf.nn.xw_plus_b (tf_s2vt.py:98,153) and the
 * tf.concat + matmul inside BasicLSTMCell.  A segment with ptr == NULL is an all-zero input
 * (the reference's `padding`) and is skipped; rowidx gathers rows (tf.nn.embedding_lookup). */
typedef struct s2vt_operand {
    const float* ptr;       /* [rows, ld] */
    const int32_t* rowidx;  /* optional [M] */
    int32_t ld;
    int32_t k;              /* columns of this segment = rows of W it multiplies */
    int32_t rowmod;         /* > 0: row(m) = m % rowmod before rowidx */
    int32_t reserved;
} s2vt_operand;

int s2vt_gemm(const s2vt_operand* segs, int32_t nseg, const float* W, int32_t ldw, const float* bias,
              const float* Cinit, int32_t ldcinit, float* C, int32_t ldc, int32_t M, int32_t N, int32_t act_tanh,
              int32_t tile_cfg, s2vt_stream stream);

/* The same contraction with the weight matrix given TRANSPOSED, Wt[N, K] (row n = output column n, K contiguous, row
 * stride ldw): C = act([seg0;seg1;seg2] @ Wt^T + bias).  This is how the backward data-gradient products read the
 * forward weights as they lie (dX = dZ @ W^T) -- no transposed copies.  Same ascending-k chain, bit-identical to
 * s2vt_gemm on the transposed matrix. */
int s2vt_gemm_nt(const s2vt_operand* segs, int32_t nseg, const float* Wt, int32_t ldw, const float* bias,
                 const float* Cinit, int32_t ldcinit, float* C, int32_t ldc, int32_t M, int32_t N, int32_t act_tanh,
                 int32_t tile_cfg, s2vt_stream stream);

/* The order-free form of the same product for GRADIENTS (dX = dZ @ W^T, compared within tolerance, never part of the
 * bit-exact forward): C[M, N] = A[M, K] @ Wt[N, K]^T with the reduction cut into `splits` K slabs that run as
 * independent tiles -- a product with a long K and few output tiles (dO2 at B = 64: 1280 x 1000 outputs, K = 12000)
 * otherwise leaves most CUs idle -- written to `slabs` [splits][M][N] (slab_floats floats) and summed into C (ldc == N).
 * splits = 0: the library's choice for the shape (1 = no slabs; then `slabs` may be NULL); tile_cfg < 0: its tile. */
int s2vt_gemm_nt_splitk(const float* A, int32_t lda, const float* Wt, int32_t ldw, float* C, int32_t ldc, int32_t M,
                        int32_t N, int32_t K, int32_t splits, int32_t tile_cfg, float* slabs, size_t slab_floats,
                        s2vt_stream stream);

/* ---- BasicLSTMCell + DropoutWrapper, one call (tf_s2vt.py:74-77,119-143) --------------------
 * z = [x0 ; x1 ; h_prev] @ W + b ; i,j,f,o = split(z) ; c' = c*sig(f+1) + sig(i)*tanh(j) ;
 * h' = tanh(c')*sig(o) ; out = keep<1 ? (h'/keep)*mask : h'  (mask from the dropout Philox
 * stream, keyed by video_id/sample_id/drop_code).  W rows are consumed in the order x0, x1, h.
 * x0/x1 may be NULL (zero input) -- their rows of W are skipped, h_prev multiplies the LAST H rows.
 * gates (optional, [M,4H]) receives sig(i) | tanh(j) | sig(f+1) | sig(o) for the backward pass. */
int s2vt_lstm_cell_fwd(const s2vt_operand* x0, const s2vt_operand* x1, const float* h_prev, const float* c_prev,
                       int32_t state_rowmod, const float* W, const float* b, float* c_new, float* h_new, float* out,
                       float* gates, int32_t M, int32_t H, float keep, uint64_t seed, const int32_t* video_id,
                       const int32_t* sample_id, uint32_t drop_code, int32_t tile_cfg, s2vt_stream stream);
/* The same with a residual operand, the decode step of residual_tf_s2vt.py:149-151,206-208,263-265: out[m] = dropout(h'[m]) + res[row(m)],
 * one fp32 addition in the cell kernel's epilogue (no launch of its own).  res: k == H, ld >= H, rowmod / rowidx honoured as in s2vt_gemm
 * (row(m) = m % rowmod, then rowidx[.]); res->ptr and `out` are required.  c_new, h_new (the un-summed h') and gates are exactly those of
 * s2vt_lstm_cell_fwd. */
int s2vt_lstm_cell_fwd_res(const s2vt_operand* x0, const s2vt_operand* x1, const float* h_prev, const float* c_prev,
                           int32_t state_rowmod, const float* W, const float* b, const s2vt_operand* res, float* c_new, float* h_new,
                           float* out, float* gates, int32_t M, int32_t H, float keep, uint64_t seed, const int32_t* video_id,
                           const int32_t* sample_id, uint32_t drop_code, int32_t tile_cfg, s2vt_stream stream);

/* The gathered-state form of the cell, one decode step of a beam search: every launch row reads its state and its carried partial
 * through index arrays (device, int32 [M]), with no gathered copy of either.
 *   z[m] = Cinit[cinit_rowidx[m]] + [x0 ; x1 ; h_prev[state_rowidx[m]]] @ W, the chain continued from the partial in ascending k, then the
 *   bias and the pointwise cell on c_prev[state_rowidx[m]]; there is no dropout (a decode step never drops), `out` does not exist.
 * state_rowidx NULL: row m of h_prev / c_prev.  Cinit NULL: the chain starts from +0 (cinit_rowidx is ignored); cinit_rowidx NULL: row m
 * of Cinit (rows ldcinit >= 4H floats apart).  Indices are NOT checked: every one must name a row of its array.  With identity maps and no
 * Cinit the results are s2vt_lstm_cell_fwd's, bit for bit.
 * With state_rowidx another workgroup may own the source row of a launch row, so the state cannot be advanced in place: c_new / h_new
 * [M, H] must not overlap ANY part of c_prev / h_prev (equal pointers are S2VT_E_BADARG; partial overlap is the caller's to avoid).
 * S2VT_E_BADARG also for NULL h_prev / c_prev / W / b / c_new / h_new, M < 0, H <= 0, ldcinit < 4H with Cinit.  M == 0: S2VT_OK.
 * tile_cfg as in s2vt_lstm_cell_fwd (kind 1 of s2vt_tile_count).  Every cell tile has this form on the 16-byte path.  Off it (H % 4 != 0
 * or unaligned operands) one tile has none: a launch forced onto gw16x16u(1x4)k64 runs gw16x16u(1x4), the 32-deep tile of the same 16 rows,
 * as the tiles with has_scalar == 0 hand theirs to `fallback`; s2vt_tile_info does not report it, and the results are the same bits. */
int s2vt_lstm_cell_fwd_gather(const s2vt_operand* x0, const s2vt_operand* x1, const float* h_prev, const float* c_prev,
                              const int32_t* state_rowidx, const float* Cinit, int32_t ldcinit, const int32_t* cinit_rowidx, const float* W,
                              const float* b, float* c_new, float* h_new, float* gates, int32_t M, int32_t H, int32_t tile_cfg,
                              s2vt_stream stream);

/* ---- vocab logits + token pick, one decode step ---------------------------------------------
 * logits = out2 @ embed_word_W + embed_word_b (tf_s2vt.py:153); token = tf.argmax(logits,1) for
 * rows with sample_id < 0 (tf_s2vt.py:262) or one draw of tf.multinomial(log_softmax(logits),1)
 * (reinforcement_multisampling_tf_s2vt.py:333-336) as Gumbel-max otherwise.  The logits stay
 * on chip unless logits_out != NULL.  packed[m] must be zero on entry; on exit it holds
 * (orderable(key) << 32) | ~token.  tokens_out (optional) receives the int32 ids.
 * The pick is exact for |logit + bias + noise| < 16384: its screen compares fast keys under the fixed kGumbelScreenMargin
 * (csrc/detmath.h), which must cover the rounding of logit + noise, so one ulp of a key must not exceed it (2^-10 below 16384). */
int s2vt_vocab_pick(const float* out2, int32_t ld, const float* W, const float* b, int32_t M, int32_t H, int32_t V,
                    const int32_t* video_id, const int32_t* sample_id, int32_t step, uint64_t seed,
                    unsigned long long* packed, int32_t* tokens_out, float* logits_out, int32_t tile_cfg,
                    s2vt_stream stream);

/* ---- the tile tables behind every tile_cfg argument, and the live-row forms of the three calls above -----------------
 * A seam for tests and tuning: no kernels of its own.  kind is the profiler's kernel_class: 0 = STORE contraction (s2vt_gemm), 1 = fused
 * LSTM cell, 2 = vocab logits + pick, 4 = STORE with the weights transposed (s2vt_gemm_nt).  s2vt_tile_count: the entries of that table
 * (tile_cfg in [0, count) forces one, anything else is the library's choice), or S2VT_E_BADARG for another kind.  s2vt_tile_info: entry
 * tile_cfg of the table -- rows x cols of the workgroup's tile (cols per gate for the cell tiles), its name as s2vt_prof_collect reports it,
 * and which forms it has.  An entry without the form a launch needs hands the launch to entry `fallback` of the same table (-1: it has every
 * form it can be asked for): has_scalar == 0 and operands off the fast path, or has_live == 0 and a live-row launch.  Kind 4 has no live-row
 * form at all. */
typedef struct s2vt_tile_desc {
    int32_t rows;
    int32_t cols;
    int32_t fallback;
    int32_t has_scalar;
    int32_t has_live;
    int32_t reserved;
    char name[32];
} s2vt_tile_desc;
int s2vt_tile_count(int kind);
int s2vt_tile_info(int kind, int tile_cfg, s2vt_tile_desc* out);

/* Live-row launches: what the early-exit samplers (S2VT_SAMPLE_STOP_AT_EOS) issue per decode step, one launch at a time.  The arguments
 * of s2vt_gemm / s2vt_lstm_cell_fwd_res / s2vt_vocab_pick keep their meaning, with M the CAPACITY -- the caller's row count, the rows of
 * every per-row array -- and two more:
 *   live    device, int32: distinct row indices in [0, M) in ascending order (what the samplers' row lists hold); only the first
 *           min(*n_live, M) entries are read.  NULL: the rows are 0 .. min(*n_live, M) - 1.
 *   n_live  device, int32: the number of live rows, read by the kernel (no host round trip).  NULL: all M entries of `live`.
 * Both NULL: S2VT_E_BADARG.  Row r = live[i] is computed exactly as row r of the dense call: every per-row access -- the segments (before
 * their own rowmod / rowidx), Cinit, c_prev / h_prev (before state_rowmod), the residual operand, video_id / sample_id, and every output --
 * uses row r of the caller's arrays.  Rows that are not listed are neither read nor written.  Bit-identical to the dense call on the
 * listed rows.  The other argument checks are those of the dense entries (M == 0: S2VT_OK, nothing is launched).  Fast path: as for
 * the dense calls, except that with a list a plain segment is addressed from its base by the caller's row, so all M of its rows must fit
 * a 2 GiB window (a dense call's operand is addressed per tile); a larger one takes the scalar path with identical results.
 *   s2vt_lstm_cell_fwd_live: res may be NULL (the plain cell); otherwise as in s2vt_lstm_cell_fwd_res.
 *   s2vt_vocab_pick_live: packed[r * pick_stride] is row r's word (pick_stride >= 1 64-bit words apart; the samplers keep one word per
 *     128-byte line, pick_stride = 16), zero on entry for the listed rows; there is no tokens_out -- the word's low half is ~token. */
int s2vt_gemm_live(const s2vt_operand* segs, int32_t nseg, const float* W, int32_t ldw, const float* bias, const float* Cinit,
                   int32_t ldcinit, float* C, int32_t ldc, int32_t M, int32_t N, int32_t act_tanh, const int32_t* live,
                   const int32_t* n_live, int32_t tile_cfg, s2vt_stream stream);
int s2vt_lstm_cell_fwd_live(const s2vt_operand* x0, const s2vt_operand* x1, const float* h_prev, const float* c_prev,
                            int32_t state_rowmod, const float* W, const float* b, const s2vt_operand* res, float* c_new, float* h_new,
                            float* out, float* gates, int32_t M, int32_t H, float keep, uint64_t seed, const int32_t* video_id,
                            const int32_t* sample_id, uint32_t drop_code, const int32_t* live, const int32_t* n_live, int32_t tile_cfg,
                            s2vt_stream stream);
int s2vt_vocab_pick_live(const float* out2, int32_t ld, const float* W, const float* b, int32_t M, int32_t H, int32_t V,
                         const int32_t* video_id, const int32_t* sample_id, int32_t step, uint64_t seed, unsigned long long* packed,
                         int32_t pick_stride, float* logits_out, const int32_t* live, const int32_t* n_live, int32_t tile_cfg,
                         s2vt_stream stream);

/* ---- frame embedding (tf_s2vt.py:97-101): emb[B*Tv, E] = video[B*Tv, d] @ encode_image_W + b */
int s2vt_frame_embed_fwd(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, float* emb,
                         s2vt_stream stream);

/* ---- samplers: build_multinomial_sampler x K + build_sampler, one call ------------------------
 * (reinforcement_multisampling_tf_s2vt.py:294-391, driven at :743-753).  Frame embed + encode once,
 * then Tc decode steps for K sampled rows-blocks (+ one greedy block when with_greedy) entirely
 * on the device: no host round trip per step.  Rows are sample-major (row k*B + j = sample k of
 * video j, :764-782), the greedy block last.  ids_out: int32 [(K + with_greedy) * B, Tc].
 * Noise: Philox stream (seed; video = video_base + j; sample = k; step). */
size_t s2vt_sample_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t K, int32_t with_greedy);
int s2vt_sample(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t K,
                int32_t with_greedy, uint64_t seed, int32_t video_base, int32_t* ids_out, void* workspace,
                size_t workspace_bytes, s2vt_stream stream);
/* s2vt_sample with flags.  S2VT_SAMPLE_STOP_AT_EOS (opt-in; NOT what the reference does, whose samplers run all Tc steps for every row,
 * reinforcement_multisampling_tf_s2vt.py:318-337): a row leaves the decode loop once it has picked <eos> = 0 -- every later step's cell
 * and vocabulary launches cover the rows still sampling only (compact row lists kept on the device, no host round trip) -- and its ids
 * behind the first <eos> are 0.  Ids up to and including the first <eos> are bit-identical to s2vt_sample's, and those are the only
 * positions the objective looks at (the mask of cider_evaluation.py:145-172 ends there). */
#define S2VT_SAMPLE_STOP_AT_EOS 1
int s2vt_sample_ex(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t K, int32_t with_greedy,
                   uint64_t seed, int32_t video_base, int32_t flags, int32_t* ids_out, void* workspace, size_t workspace_bytes,
                   s2vt_stream stream);

/* s2vt_sample with the vocabulary pick screened: per decode step the bf16 product bf16(h) . bf16(embed_word_W) of
 * the step's rows gives approximate logits, a proven margin (|h - bf16(h)| max|W[:, v]| + 1.004 |h| max|W[:, v] - bf16(W[:, v])|, what the
 * two casts miss, + 2^-11 |h| max|W[:, v]| per 1024 reduction steps for the accumulation, plus the Gumbel screen's) keeps the columns of a row that can still win it, and only those get the exact ascending-k fp32 chain and the exact Gumbel
 * expression.  ids_out is bit-identical to s2vt_sample's.  S2VT_PICK_PRODUCTS=3 in the environment (read once), or an explicit
 * S2VT_PICK_TILE, screens on the three-product split-bf16 product instead (margin 2^-10 |h| max|W[:, v]| per 1024 steps; the lo planes
 * of the scratch are written only then): the same ids, a slower product, fewer survivors.  workspace / workspace_bytes: s2vt_sample's, carved and left as s2vt_sample
 * leaves it.  screen_ws (256-byte aligned): a scratch of its own of s2vt_sample_screen_workspace_bytes bytes -- a 256-byte head block,
 * the hi / lo planes of embed_word_W^T [V][pad(H)] (bf16, pad = up to a multiple of 64), embed_word_W^T in fp32 [V][H up to a
 * multiple of 4] (a surviving column is read as one row), the hi / lo planes of the step's rows [R][pad(H)] and the approximate logits
 * [R][V up to a multiple of 4] fp32, each region rounded up to 256 bytes: about 118 MB at V = 12000, H = 1000, R = 384.  The head block holds, per call: uint64 survivors summed over rows and steps (byte 0), uint32 the most survivors of one row
 * (byte 8), uint32 rows that took every column because a key, norm or margin was not finite (byte 12); then the two column-norm maxima the
 * margin uses (floats, bytes 16 and 20).
 * ..._workspace_bytes returns 0 where the path does not serve the call -- (K + with_greedy) * B <= 64 rows (the persistent decode
 * loop's shapes), lstm_dim > 2048, a residual model, bad arguments, 257 - 384 rows while S2VT_DECLOOP=2 or S2VT_DEC4=1 asks for the
 * opt-in fragment-order forms there, or S2VT_PICK_SCREEN=0 in the environment (read once) -- and
 * s2vt_sample_screened then returns S2VT_E_BADARG.  Other errors as s2vt_sample; S2VT_E_WORKSPACE for either block too small. */
size_t s2vt_sample_screen_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t K, int32_t with_greedy);
int s2vt_sample_screened(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t K, int32_t with_greedy,
                         uint64_t seed, int32_t video_base, int32_t* ids_out, void* workspace, size_t workspace_bytes, void* screen_ws,
                         size_t screen_bytes, s2vt_stream stream);

/* ---- mixed sampler: build_mix_sample of reinforce_multitask_e2e_attribute_by_groudtruth_greedy_s2vt.py:512-599 (built at :828, run
 * beside build_sampler on the same batch at :957-960), whose reward is that script's baseline.  A greedy decode in which the word fed
 * back at step t >= 1 is the ground-truth word caption[b][t - 1] with probability p_gt and the row's own argmax of step t - 1 otherwise
 * (:576-587: tf.multinomial over log([p, 1.00001 - p]), so p_gt = p / 1.00001); step 0 feeds <bos> = 1; the emitted id is always the
 * argmax (:595), whatever was fed.  ids_out: int32 [(1 + with_greedy) * B, Tc] -- block 0 the B mixed rows, block 1 (with_greedy) the
 * plain greedy rows of build_sampler, bit-identical to s2vt_sample's greedy block; both decode from ONE encode.
 * The coin is a pure function of (seed, global video id, step): u = u01(philox4x32_10(counter (0, video_base + b, 0, t), key (seed_lo,
 * seed_hi ^ 0x4D495853)).x) with u01(x) = ((x >> 9) + 0.5) * 2^-23, ground truth iff u < p_gt -- p_gt = 1 always feeds it, p_gt = 0
 * never; a batch split over ranks draws the same coins (as the Gumbel stream of s2vt_sample).
 * caption: DEVICE int32 [B][n_caption_lstm_step] row-major; an id outside [0, n_words) is clamped into that range where it is read, so
 * no caption can make the embedding gather leave Wemb.  Errors: S2VT_E_BADARG (a NULL pointer, B <= 0, p_gt outside [0, 1] or NaN),
 * S2VT_E_ALIGN, S2VT_E_WORKSPACE, S2VT_E_CHAIN_TIMEOUT as s2vt_sample_ex.  The workspace is s2vt_sample's for the same row count
 * followed by the fed words; ..._workspace_bytes: 0 on bad arguments. */
size_t s2vt_sample_mix_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t with_greedy);
int s2vt_sample_mix(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, const int32_t* caption, float p_gt,
                    int32_t with_greedy, uint64_t seed, int32_t video_base, int32_t* ids_out, void* workspace, size_t workspace_bytes,
                    s2vt_stream stream);

/* ---- batched beam search: build_generator(beam_size, length_normalization_factor) of final_beam_search.py:201-294 for B videos
 * at once.  The reference runs one B = 1 graph per live beam per step (beam_probability, :203-224) and keeps the captions in TopN
 * heaps (beam_search.py:44-80); here one call per decode step advances every live hypothesis of every video, and only the
 * heap bookkeeping stays on the host.
 *
 * s2vt_vocab_topk: for each row r of logits [R, V] (row stride ld), ids[r, j] / logp[r, j] (j < k, 1 <= k <= 16) = the k largest
 * logits ordered by value descending, then index ascending on exact ties (tf.nn.top_k's order, :217), and l[id] - lse with
 * lse = max + log(sum exp(l - max)) evaluated exactly as s2vt_softmax_nll_fwd_bwd evaluates it: logp is bit-identical to that
 * call's lp_target for target = id (same ld, same pointer alignment).  Finite logits only: NaN is out of scope. */
int s2vt_vocab_topk(const float* logits, int32_t ld, int32_t R, int32_t V, int32_t k, int32_t* ids, float* logp, s2vt_stream stream);
/* Workspace of a beam decoder for B videos and up to beam hypotheses per video (1 <= beam <= 16): the sampler's encode half for
 * B rows plus LSTM2 state, gathered cell inputs and logits for B * beam rows.  0 on bad arguments. */
size_t s2vt_beam_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t beam);
/* Frame embedding + encoding stage for the B videos (final_beam_search.py:226-253), as the samplers run it (persistent
 * recurrences, no per-step cell launches), and the word-independent half of every decode step: the LSTM1 trajectory -- shared
 * by all beams of a video, it never sees a word -- and its products h1 @ W2[0:H]. */
int s2vt_beam_encode(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t beam, void* workspace,
                     size_t workspace_bytes, s2vt_stream stream);
/* Decode step t (0 <= t < Tc) for R <= B * beam live hypotheses (beam_probability, :203-224, with the expansion of :255-290 left
 * to the caller), no host synchronisation.  Hypothesis m continues video video_of_row[m] from row parent[m] of step t - 1 (at
 * t = 0: from the video's encoder state; parent is ignored) with word[m] (<bos> = 1 at t = 0).  The three int32 [R] arrays are
 * device pointers (one host-to-device copy of a [3][R] block suits them); indices out of range are clamped, not reported.
 * Writes top_ids / top_logp [R, k] (s2vt_vocab_topk of the step's logits) and, when logits_out is given, the logits [R, V]. */
int s2vt_beam_step(const s2vt_dims* d, const s2vt_params* p, int32_t B, int32_t beam, int32_t t, int32_t R, const int32_t* video_of_row,
                   const int32_t* parent, const int32_t* word, int32_t k, int32_t* top_ids, float* top_logp, float* logits_out,
                   void* workspace, size_t workspace_bytes, s2vt_stream stream);

/* ---- teacher-forced unroll: build_model (tf_s2vt.py:90-153) / build_loss
 * (reinforcement_multisampling_tf_s2vt.py:227-292) forward --------------------------------------
 * video [B,Tv,d]; the N = rep*B rows are sample-major copies of the B videos (row n uses video
 * n % B -- the reference tiles the feature block 8x on the host, :779-782; here it is never
 * materialised).  caption int32 [N,Tc]; previous word = <bos> at t=0 else caption[:,t-1].
 * Dropout-wrapped cells: keep < 1 draws the masks from the dropout Philox stream (seed; video_id,
 * sample_id per row; code = layer*256 + step); keep >= 1 disables dropout.  logits_out
 * [Tc*N, V] is TIME-MAJOR (row t*N + n).  Activations needed by s2vt_bptt_bwd stay in the workspace. */
size_t s2vt_train_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t N);
int s2vt_teacher_forced_fwd(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t N,
                            const int32_t* caption, float keep, uint64_t seed, const int32_t* video_id,
                            const int32_t* sample_id, float* logits_out, void* workspace, size_t workspace_bytes,
                            s2vt_stream stream);

/* ---- scheduled-sampling unroll: build_model of generate_words_tf_s2vt.py:101-211 (forward) -------------------------------------------
 * The training unroll decodes: at step t >= 1 row n of LSTM2 is fed the ground-truth word caption[n][t - 1] when its coin says so and
 * its own argmax of step t - 1 otherwise (:159-168); step 0 feeds <bos> = 1 (:161-163).  The argmax is behind tf.stop_gradient (:166),
 * so the gradient of the step is that of a teacher-forced step on the words that were fed: after the call the training workspace
 * (s2vt_train_workspace_bytes, unchanged) is what s2vt_teacher_forced_fwd leaves for a caption whose previous words are `fed` -- prev
 * holds the fed words, tgt the ground truth, G1 .. O2 the activations -- and s2vt_bptt_bwd* / s2vt_bptt_dvideo run on it as they are.
 * Coin (:136-139,159: tf.multinomial over log([p, 1.00001 - p]), so p_gt = p / 1.00001; p = 0.5 is written into the reference's graph):
 * s2vt_sample_mix's, extended by the sample id -- u = u01(philox4x32_10(counter (0, video_id[n], sample_id[n], t), key (coin_seed_lo,
 * coin_seed_hi ^ 0x4D495853)).x), ground truth iff u < p_gt.  With sample_id = 0 these are s2vt_sample_mix's coins for video_base + b =
 * video_id.  video_id / sample_id are required whatever keep says; they also key the dropout streams (keep, seed: as s2vt_teacher_forced_fwd).
 * Per step: the dropout-wrapped cells (:151-154,181-184), logits = xw_plus_b(dropped out2) (:189), generated = argmax (lowest index on ties,
 * :193).  Quirk SQ1 (:194-199): the running mask one_mask[n] *= (generated[n] != 0) is updated BEFORE it weighs the step's cross entropy,
 * so it follows the model's own picks, not the caption, and the position at which the model emits <eos> is already masked (s2vt_caption_mask
 * keeps that position).  All outputs are device memory:
 *   logits_out [Tc*N, V] time-major, bit-identical to s2vt_teacher_forced_fwd's for the same fed words (:200 `probs`);
 *   generated, fed [N, Tc] int32 (fed[:, 0] = 1);  mask [N, Tc] (:201 `caption_mask`, transposed);
 *   coef_tm [Tc*N] = loss_weight * mask and target_tm [Tc*N] = caption, both time-major: what s2vt_softmax_nll_fwd_bwd takes (smoothing 0;
 *   the loss of :198-210 is sum(coef * nll) / sum(mask) + the weight decay term);
 *   *mask_sum, *mask_sum_copy = sum(mask), each may be NULL (the copy: the gradient bucket's tail slot), summed in a fixed order.
 * sum(mask) = 0 -- every row emits <eos> at step 0 -- is the reference's 0/0 and is not repaired here.
 * caption: device int32 [N, Tc]; an id outside [0, n_words) is clamped into that range where it is read.  One fused cell launch, one pick
 * launch and one small launch per step, no host round trip.  scratch: s2vt_scheduled_scratch_bytes(d, N) bytes (0 on bad arguments), 256-byte
 * aligned like the workspace.  Errors: S2VT_E_BADARG (a NULL pointer other than the two sums, N % B != 0, keep <= 0, p_gt outside [0, 1] or
 * NaN), S2VT_E_ALIGN, S2VT_E_WORKSPACE, S2VT_E_CHAIN_TIMEOUT. */
size_t s2vt_scheduled_scratch_bytes(const s2vt_dims* d, int32_t N);
int s2vt_scheduled_fwd(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t N, const int32_t* caption, float p_gt,
                       uint64_t coin_seed, float loss_weight, float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id,
                       float* logits_out, int32_t* generated, int32_t* fed, float* mask, float* coef_tm, int32_t* target_tm, float* mask_sum,
                       float* mask_sum_copy, void* workspace, size_t workspace_bytes, void* scratch, size_t scratch_bytes, s2vt_stream stream);

/* ---- averaged-embedding unroll: build_model of average_generate_words_tf_s2vt.py:88-165 (forward and backward) ------------------------
 * s2vt_scheduled_fwd without the coin.  Step 0 feeds <bos> = 1 alone (:124-127); at step t >= 1 row n of LSTM2 is fed
 *   x[n] = (Wemb[caption[n][t - 1]] + Wemb[g[n][t - 1]]) / 2   (:131-133),  g[.][t - 1] = argmax of step t - 1's logits, lowest index on ties (:156)
 * -- in fp32 one rounded addition and an exact halving, so with both ids equal x is that row of Wemb bit for bit.  Both cells are
 * dropout-wrapped (:138-142; keep, seed, video_id, sample_id as s2vt_teacher_forced_fwd, the ids required whatever keep says),
 * logits = xw_plus_b(dropped out2) (:152).  The mask is the FED placeholder (:92,154), not a running mask: quirk SQ1 does not exist here.
 * Loss (:153-164): loss_weight * sum_t sum_n xent * mask[n][t] / sum(mask) + the weight decay term; no label smoothing, no batch mean.
 * Outputs, device memory: logits_out [Tc*N, V] time-major (:155 `probs`); generated [N, Tc] int32; coef_tm [Tc*N] = loss_weight * mask and
 * target_tm [Tc*N] = caption, both time-major (what s2vt_softmax_nll_fwd_bwd takes, smoothing 0); *mask_sum, *mask_sum_copy = sum(mask),
 * each may be NULL, summed in s2vt_scheduled_fwd's fixed order.  caption: device int32 [N, Tc], an id outside [0, n_words) is clamped
 * where it is read; mask: device float [N, Tc].  One fused cell launch (the step's mean block a dense operand at kw = H), one pick launch
 * and one small launch per step, no host round trip.
 * workspace: the training workspace (s2vt_train_workspace_bytes, unchanged): G1 .. O2 hold the activations; prev holds the ground-truth
 * previous words, which is NOT what LSTM2 was fed -- s2vt_bptt_bwd* on it would compute another graph's gradient.
 * scratch: s2vt_averaged_scratch_bytes(d, N) bytes (0 on bad arguments), 256-byte aligned: the packed picks, then what the backward reads
 * again -- Xbar [Tc*N, E] (block 0: Wemb[1] for every row) and the id pair (truth, picked) of every (step, row), (1, 1) at step 0.
 * Errors: S2VT_E_BADARG (a NULL pointer other than the two sums, N % B != 0, keep <= 0, a model bit), S2VT_E_ALIGN, S2VT_E_WORKSPACE (a short
 * workspace or scratch), S2VT_E_CHAIN_TIMEOUT.
 *
 * s2vt_averaged_bptt_bwd: s2vt_bptt_bwd on that workspace and scratch.  The argmax is not differentiable, everything else is -- no
 * stop_gradient stands in front of the second lookup (:132): dWemb[caption[n][t-1]] += dx[n][t] / 2 and dWemb[g[n][t-1]] += dx[n][t] / 2
 * (s2vt_embed_scatter_add2), and LSTM2's weight gradient for the word rows is Xbar^T dZ2, the mean as the operand.
 * precision: 0 = fp32 MFMA products (s2vt_bptt_bwd's; grad_ws NULL); 1 = bf16 operands (s2vt_bptt_bwd_bf16's, grad_ws of
 * s2vt_bf16_grad_workspace_bytes); 2 = s2vt_bptt_bwd_split's rule (split-bf16 above 256 rows, grad_ws of s2vt_split_grad_workspace_bytes;
 * dlogits NULL = the planes s2vt_softmax_nll_fwd_bwd_split left there).  Whole pass only (no phases, steps or live rows).
 * Errors: s2vt_bptt_bwd's, and S2VT_E_BADARG for a precision outside 0..2 or a grad_ws that does not go with it. */
size_t s2vt_averaged_scratch_bytes(const s2vt_dims* d, int32_t N);
int s2vt_averaged_fwd(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t N, const int32_t* caption, const float* mask,
                      float loss_weight, float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id, float* logits_out,
                      int32_t* generated, float* coef_tm, int32_t* target_tm, float* mask_sum, float* mask_sum_copy, void* workspace,
                      size_t workspace_bytes, void* scratch, size_t scratch_bytes, s2vt_stream stream);
int s2vt_averaged_bptt_bwd(const s2vt_dims* d, const s2vt_params* p, const s2vt_params* grads, const float* video, int32_t B, int32_t N,
                           const float* dlogits, float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id, void* workspace,
                           size_t workspace_bytes, const void* scratch, size_t scratch_bytes, int32_t precision, void* grad_ws, size_t grad_ws_bytes,
                           s2vt_stream stream);

/* ---- top-k score-weighted embedding unroll: build_model / build_generator of sum_generate_words_tf_s2vt.py:101-275 ----------------------
 * s2vt_averaged_fwd with another operand.  Step 0 feeds <bos> = 1 (:158-161); at step t >= 1 row n of LSTM2 is fed (:163-174,208-210)
 *   scores, ids = top_k(logits[t - 1][n], k),   w = scores / reduce_sum(scores)   (raw logits, no softmax),   x[n] = sum_j w[j] Wemb[ids[j]]
 * with top_k's order (value descending, index ascending on exact ties: s2vt_vocab_topk's), the sum of the scores added in ascending j, w
 * an IEEE division, and x the chain ((((0 + w0 e0) + w1 e1) + ...) in ascending j, each product and each addition rounded on its own (no
 * FMA).  A sum of 0 is the script's own 0/0 and is not repaired.  Quirk TK1: the coin of :156 is compared with a Python int (:165), which is
 * always False, so the ground-truth branch is never built -- there is no coin and no p_gt here, and the caption enters as labels only.
 * Both cells are dropout-wrapped (keep, seed, video_id, sample_id as s2vt_teacher_forced_fwd, the ids required whatever keep says).  The
 * mask is the FED placeholder (:106,204), not a running mask.  Loss (:212-218): loss_weight * sum xent * mask / sum(mask) + weight decay.
 * 1 <= k <= 8, k <= n_words (the script's k is 5).
 * Outputs as s2vt_averaged_fwd: logits_out [Tc*N, V] time-major; generated [N, Tc] int32 = ids[.][0]; coef_tm [Tc*N] = loss_weight * mask
 * and target_tm [Tc*N]; *mask_sum, *mask_sum_copy (each may be NULL).  One fused cell launch, one pick launch and one mix launch per step,
 * no host round trip.
 * workspace: the training workspace (s2vt_train_workspace_bytes, unchanged).
 * scratch: s2vt_topk_feed_scratch_bytes(d, N, k) bytes (0 on bad arguments), 256-byte aligned: the packed picks, then what the backward
 * reads again, time-major, block t holding what step t was fed -- X [Tc*N, E] (block 0: Wemb[1] for every row), ids / w [Tc*N, k] and the
 * raw sums S [Tc*N] (block 0: ids 1, w (1, 0, ...), S 1).
 * Errors: S2VT_E_BADARG (a NULL pointer other than the two sums, N % B != 0, keep <= 0, k outside 1..8 or above n_words, a model bit),
 * S2VT_E_ALIGN, S2VT_E_WORKSPACE (a short workspace or scratch), S2VT_E_CHAIN_TIMEOUT.
 *
 * s2vt_topk_feed_bptt_bwd: the backward of that unroll.  The ids are constants, everything else is differentiable -- no stop_gradient
 * anywhere in :163-174 -- so the loss of step t reaches logits[t - 1] through the weights: with ds_j = dx . Wemb[ids_j] and
 * g = sum_j w_j ds_j, dlogits[t - 1][n][ids_j] += (ds_j - g) / S, and from there embed_word_W, embed_word_b and LSTM2's earlier state.
 * dlogits [Tc*N, V] is READ AND WRITTEN: on entry the softmax part (what s2vt_softmax_nll_fwd_bwd leaves), on return the completed
 * gradient with respect to the logits.  dWemb[ids_j] += w_j dx (s2vt_embed_scatter_addk).  LSTM2's recurrence runs step by step (the
 * new edge crosses its steps); fp32 products only -- the bf16 and split-bf16 product sets are not implemented for this backward -- and
 * the whole pass only (no phases, live rows or step cuts).  Errors: as above. */
size_t s2vt_topk_feed_scratch_bytes(const s2vt_dims* d, int32_t N, int32_t k);
int s2vt_topk_feed_fwd(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t N, const int32_t* caption, const float* mask,
                       float loss_weight, float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id, int32_t k,
                       float* logits_out, int32_t* generated, float* coef_tm, int32_t* target_tm, float* mask_sum, float* mask_sum_copy,
                       void* workspace, size_t workspace_bytes, void* scratch, size_t scratch_bytes, s2vt_stream stream);
int s2vt_topk_feed_bptt_bwd(const s2vt_dims* d, const s2vt_params* p, const s2vt_params* grads, const float* video, int32_t B, int32_t N,
                            float* dlogits, float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id, int32_t k,
                            void* workspace, size_t workspace_bytes, const void* scratch, size_t scratch_bytes, s2vt_stream stream);
/* build_generator of the same script (:221-275) for B videos: no dropout; per step the cell launch on the step's mix, the logits, then
 * unshifted_softmax = 1: probs = exp(l) / sum exp(l) as s2vt_softmax_unshifted_argmax writes them (:255) and the emitted word
 *   argmax(probs) (:257); 0: the emitted word is the first of the top-k ids;
 * weights_mode = 1: top_k, weights and mix from the probabilities (:259-268; needs unshifted_softmax = 1) -- the script's generator;
 *   0: from the raw logits, the training rule.
 * The `break` of :273 tests a tensor and never fires: Tc words per video.  ids_out [B, Tc] int32; logits_out [Tc*B, V] time-major or NULL.
 * workspace: s2vt_topk_feed_decode_workspace_bytes(d, B, k) bytes (0 on bad arguments), 256-byte aligned.  Errors: S2VT_E_BADARG,
 * S2VT_E_ALIGN, S2VT_E_WORKSPACE, S2VT_E_CHAIN_TIMEOUT. */
size_t s2vt_topk_feed_decode_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t k);
int s2vt_topk_feed_decode(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t k, int32_t weights_mode,
                          int32_t unshifted_softmax, int32_t* ids_out, float* logits_out, void* workspace, size_t workspace_bytes,
                          s2vt_stream stream);
/* The mix alone (sum_generate_words_tf_s2vt.py:166-173), on R rows.  weights_mode 0: scores = logits [R, ld >= V] (plane NULL);
 * 1: scores = plane [R, ldp >= V] (logits unread).  Writes ids [R, k], w [R, k], score_sum [R] and x [R, ldx >= E] as described above;
 * Wemb [V, E] contiguous.  R = 0: nothing is launched. */
int s2vt_topk_mix_fwd(const float* logits, int32_t ld, const float* plane, int32_t ldp, int32_t weights_mode, int32_t R, int32_t V, int32_t k,
                      const float* Wemb, int32_t E, int32_t* ids, float* w, float* score_sum, float* x, int32_t ldx, s2vt_stream stream);
/* Its backward, the ids constants: dscores[r][ids[r][j]] += (ds_j - g) / score_sum[r] (ds_j = dx[r] . Wemb[ids[r][j]], g = sum_j w_j ds_j;
 * no other column of dscores [R, lds >= V] is written) and, dO non-NULL, dO[r][0:H] += sum_j that * Wout[:, ids[r][j]] (Wout [H, V],
 * dO [R, ldo >= H]).  dx [R, lddx >= E]; the ids must lie inside Wemb. */
int s2vt_topk_mix_bwd(const float* dx, int32_t lddx, const int32_t* ids, const float* w, const float* score_sum, const float* Wemb, int32_t E,
                      const float* Wout, int32_t V, int32_t H, int32_t k, int32_t R, float* dscores, int32_t lds, float* dO, int32_t ldo,
                      s2vt_stream stream);

/* Same, inside a REINFORCE step: LSTM1's state trajectory depends only on the frames and the weights, and the
 * sampler pass of the step (s2vt_sample / s2vt_encode_fwd on the SAME video block, SAME weights) has just
 * computed it.  Pass that call's workspace (and its row count R = (K + with_greedy) * B) and the trajectory and
 * gates are copied from it instead of being recomputed.  sampler_workspace == NULL: identical to the above. */
int s2vt_teacher_forced_fwd_reuse(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t N,
                                  const int32_t* caption, float keep, uint64_t seed, const int32_t* video_id,
                                  const int32_t* sample_id, float* logits_out, void* workspace, size_t workspace_bytes,
                                  const void* sampler_workspace, size_t sampler_workspace_bytes, int32_t sampler_rows,
                                  s2vt_stream stream);

/* Same, unrolling only the first `caption_steps` (1 .. Tc) decode steps: when no row of the batch has an unmasked
 * position at t >= caption_steps -- the padding behind the longest caption of the batch (tf_s2vt.py:371-401 pads every
 * caption to Tc; cider_evaluation.py:145-172 masks a sample behind its first <eos>) -- those steps add exact zeros to the
 * loss and to every gradient, so a caller that knows the masks on the host skips them.  `caption` keeps its [N, Tc] row
 * stride; logits_out is [caption_steps * N, V]; the workspace is the one s2vt_train_workspace_bytes sizes (its layout does
 * not depend on caption_steps).  Pair it with s2vt_bptt_bwd_steps at the SAME caption_steps. */
int s2vt_teacher_forced_fwd_steps(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t N,
                                  const int32_t* caption, int32_t caption_steps, float keep, uint64_t seed,
                                  const int32_t* video_id, const int32_t* sample_id, float* logits_out, void* workspace,
                                  size_t workspace_bytes, const void* sampler_workspace, size_t sampler_workspace_bytes,
                                  int32_t sampler_rows, s2vt_stream stream);

/* Same, and the vocabulary projection only for the LIVE (step, row) pairs: live_rows[r] (ascending, < caption_steps * N,
 * time-major index t * N + n) names the unrolled row whose logits land in row r of logits_out [n_live, V].  A position behind a
 * sample's first <eos> is masked (cider_evaluation.py:145-172): its logits feed nothing, its loss term and every gradient
 * contribution are exact zeros -- on a trained model's samples (8 of 20 positions live) the four vocabulary-sized kernels of a
 * step (logits, softmax, dWout, dO2: a third of it) shrink with the live fraction.  At 257-384 rows LSTM2's recurrence also stops
 * a row behind its last live step (rows sorted by length on the device; the history slots of a stopped row are not written and
 * nothing reads them); the other recurrence forms step every row.
 * live_rows == NULL (n_live == 0): every row, as s2vt_teacher_forced_fwd_steps.  Pair it with s2vt_bptt_bwd_live on the same list.
 * The list must be closed towards earlier steps (t * N + n live => (t - 1) * N + n live), as masks up to a first <eos> are: the
 * backward also leaves the dead rows out of LSTM2's weight- and input-gradient products, whose dZ2 rows are zeros only BEHIND
 * a row's last live step. */
int s2vt_teacher_forced_fwd_live(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t N,
                                 const int32_t* caption, int32_t caption_steps, const int32_t* live_rows, int32_t n_live, float keep,
                                 uint64_t seed, const int32_t* video_id, const int32_t* sample_id, float* logits_out,
                                 void* workspace, size_t workspace_bytes, const void* sampler_workspace,
                                 size_t sampler_workspace_bytes, int32_t sampler_rows, s2vt_stream stream);

/* ---- softmax / NLL rows, forward + backward ----------------------------------------------------
 * nll[r] = -sum_v q[v] * log_softmax(logits[r])[v],  q = onehot(target[r])*(1-s) + s/V
 * (tf.losses.softmax_cross_entropy(label_smoothing=s), tf_s2vt.py:155; s = 0 gives the
 * log-prob of the sampled word, reinforcement_multisampling_tf_s2vt.py:286-288), and
 * logits[r,:] <- coef[r] * (softmax(logits[r]) - q)   (the gradient of sum_r coef[r]*nll[r]).
 * XE: coef = the Q1 batch-mean weights; REINFORCE: coef[r] = (reward - baseline)[n] * mask[n,t]
 * (:643-646) -- in both cases WITHOUT the 1/sum(mask) factor, which is applied after the
 * data-parallel all-reduce by s2vt_grad_finalize.  lp_target (optional) = log-prob of target. */
int s2vt_softmax_nll_fwd_bwd(float* logits, int32_t ld, int32_t R, int32_t V, const int32_t* target, const float* coef,
                             float smoothing, float* nll, float* lp_target, s2vt_stream stream);
/* The same with one label-smoothing value PER ROW (smoothing_rows [R]): rows of two objectives -- the reward-scaled NLL of
 * sampled captions (s = 0) and the smoothed XE of ground-truth captions (s = 0.05), reinforce_multitask_e2e_attribute_s2vt.py:850
 * -- share one teacher-forced pass. */
int s2vt_softmax_nll_fwd_bwd_rows(float* logits, int32_t ld, int32_t R, int32_t V, const int32_t* target, const float* coef,
                                  const float* smoothing_rows, float* nll, float* lp_target, s2vt_stream stream);

/* ---- back-propagation through the unroll (what tf.gradients builds, :650) ---------------------
 * dlogits [Tc*N, V] time-major (output of s2vt_softmax_nll_fwd_bwd); the workspace must still hold
 * the activations of the matching s2vt_teacher_forced_fwd call (same d, B, N, keep, seed, ids).
 * Gradients are ACCUMULATED into `grads` (same layout as the parameters; zero it first). */
int s2vt_bptt_bwd(const s2vt_dims* d, const s2vt_params* p, const s2vt_params* grads, const float* video, int32_t B,
                  int32_t N, const float* dlogits, float keep, uint64_t seed, const int32_t* video_id,
                  const int32_t* sample_id, void* workspace, size_t workspace_bytes, s2vt_stream stream);

/* The same in parts, for data-parallel callers that start the all-reduce of a gradient slice as soon as it is final and
 * let it run under the rest of the backward:  phase 1 = the vocab projection (embed_word_W / _b final; also the
 * gradient w.r.t. LSTM2's outputs);  3 = LSTM2's recurrence and weight gradients (lstm2_W / _b final);  4 = everything
 * after (input gradients, LSTM1, Wemb, frame embedding);  2 = 3 + 4;  0 = s2vt_bptt_bwd.  Call them in the order
 * 1, 3, 4 (or 1, 2) on the same workspace. */
int s2vt_bptt_bwd_phase(const s2vt_dims* d, const s2vt_params* p, const s2vt_params* grads, const float* video, int32_t B,
                        int32_t N, const float* dlogits, float keep, uint64_t seed, const int32_t* video_id,
                        const int32_t* sample_id, void* workspace, size_t workspace_bytes, int32_t phase, s2vt_stream stream);

/* The backward of s2vt_teacher_forced_fwd_steps: dlogits is [caption_steps * N, V]; steps behind caption_steps carry no
 * gradient (the recurrences start from zero at the last unrolled step).  phase as above. */
int s2vt_bptt_bwd_steps(const s2vt_dims* d, const s2vt_params* p, const s2vt_params* grads, const float* video, int32_t B,
                        int32_t N, const float* dlogits, int32_t caption_steps, float keep, uint64_t seed,
                        const int32_t* video_id, const int32_t* sample_id, void* workspace, size_t workspace_bytes, int32_t phase,
                        s2vt_stream stream);

/* The backward of s2vt_teacher_forced_fwd_live: dlogits is [n_live, V] (row r = unrolled row live_rows[r]); the vocabulary
 * gradients are reduced over the live rows, the gradient w.r.t. LSTM2's outputs is computed for them and is zero elsewhere;
 * LSTM2's weight gradients and d[out1 ; embed] likewise take the Tv encode steps plus the live decode rows. */
int s2vt_bptt_bwd_live(const s2vt_dims* d, const s2vt_params* p, const s2vt_params* grads, const float* video, int32_t B,
                       int32_t N, const float* dlogits, int32_t caption_steps, const int32_t* live_rows, int32_t n_live, float keep,
                       uint64_t seed, const int32_t* video_id, const int32_t* sample_id, void* workspace, size_t workspace_bytes,
                       int32_t phase, s2vt_stream stream);

/* ---- opt-in bf16 mode of the backward's gradient contractions (NON-PARITY) ------------------------------
 * s2vt_bptt_bwd_bf16 is s2vt_bptt_bwd_live with every weight-gradient and data-gradient contraction on bf16 operands (round to
 * nearest even) with fp32 accumulation; the recurrences, dropout, the embedding scatter, the bias gradients (fp32 column sums of
 * the fp32 operands) and the gradient buffers stay fp32, and nothing before the backward changes: ids, logits, NLL and loss are
 * those of the fp32 mode, only the gradients differ.  Everything runs on `stream`, deterministically.  bf16_ws: a scratch of its
 * own (256-byte aligned) of s2vt_bf16_grad_workspace_bytes(d, B, N) bytes, returned 0 on bad arguments; at BASELINE configs[2]
 * (H 1000, E 500, |V| 12000, B 64, N 320) it is 348 MB, the bf16 copies of dlogits (2 x 154 MB) the most of it. */
size_t s2vt_bf16_grad_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t N);
int s2vt_bptt_bwd_bf16(const s2vt_dims* d, const s2vt_params* p, const s2vt_params* grads, const float* video, int32_t B,
                       int32_t N, const float* dlogits, int32_t caption_steps, const int32_t* live_rows, int32_t n_live, float keep,
                       uint64_t seed, const int32_t* video_id, const int32_t* sample_id, void* workspace, size_t workspace_bytes,
                       int32_t phase, void* bf16_ws, size_t bf16_ws_bytes, s2vt_stream stream);

/* fp32 -> bf16 (RNE, NaN kept), rows optionally gathered: row r of the input is src[rowidx ? rowidx[r] : r].
 * transpose = 0: dst[r][c] for c < Kp = C rounded up to 64 (zeros past C); ldd >= Kp, ldd % 8 == 0, dst 16-byte aligned.
 * transpose = 1: dst[c][r] for r < Rp (zeros for R <= r < Rp; Rp a multiple of 64, ldd >= Rp, ldd % 8 == 0); optionally also
 *   the row form into row_dst (row_ldd >= Kp, row_ldd % 4 == 0) and colsum[c] += sum_r src[row r][c] in fp32 (fixed order, no
 *   atomics) through `scratch` (4 * ceil(Rp / 256) * C bytes). */
int s2vt_cast_bf16(const float* src, int32_t ld, const int32_t* rowidx, int32_t R, int32_t C, int32_t transpose, uint16_t* dst, int32_t ldd,
                   int32_t Rp, float* colsum, uint16_t* row_dst, int32_t row_ldd, void* scratch, size_t scratch_bytes, s2vt_stream stream);
/* C[M,N] (+)= A[M,Kp] B[N,Kp]^T: bf16 operands (Kp % 64 == 0, lda / ldb >= Kp and % 8 == 0, 16-byte aligned), fp32 accumulation,
 * no atomics.  accumulate 1: C += the product.  mfma: 16 / 32 = v_mfma_f32_16x16x32_bf16 / _32x32x16_bf16, 0 = the library's choice. */
int s2vt_gemm_bf16_nt(const uint16_t* A, int32_t lda, const uint16_t* B, int32_t ldb, float* C, int32_t ldc, int32_t M, int32_t N,
                      int32_t Kp, int32_t accumulate, int32_t mfma, s2vt_stream stream);

/* ---- split-bf16 products of the backward's gradient contractions (the default fp32 mode's arithmetic) ----------
 * s2vt_bptt_bwd_split is s2vt_bptt_bwd_live with each gradient contraction A.B^T computed from split operands -- hi = bf16(x),
 * lo = bf16(x - hi), both round to nearest even -- as Ahi.Bhi^T + Ahi.Blo^T + Alo.Bhi^T on bf16 MFMA with fp32 accumulation (about
 * 3 x 2^-18 of |x.y| per product); the recurrences, dropout, the embedding scatter, the other bias gradients (fp32 column sums), clip
 * and Adam stay fp32, and ids, logits, NLL and loss are those of s2vt_bptt_bwd_live.  At N <= 256 rows it runs s2vt_bptt_bwd_live's
 * fp32 body (the gated side-stream overlap); so does every shape when the environment sets S2VT_SPLIT_GRADS=0 (read once) -- then
 * bit-identical to s2vt_bptt_bwd_live.  Deterministic, no atomics.  split_ws: a scratch of its own (256-byte aligned) of
 * s2vt_split_grad_workspace_bytes(d, B, N) bytes (0 on bad arguments): about twice the bf16 mode's -- 0.7 GB at BASELINE
 * configs[2], several GB at the reference defaults (B 256, K 8, 35 caption steps).  It is held to that size in every mode: the
 * fp32 body never touches it, but a smaller one is S2VT_E_WORKSPACE there as well. */
size_t s2vt_split_grad_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t N);
int s2vt_bptt_bwd_split(const s2vt_dims* d, const s2vt_params* p, const s2vt_params* grads, const float* video, int32_t B,
                        int32_t N, const float* dlogits, int32_t caption_steps, const int32_t* live_rows, int32_t n_live, float keep,
                        uint64_t seed, const int32_t* video_id, const int32_t* sample_id, void* workspace, size_t workspace_bytes,
                        int32_t phase, void* split_ws, size_t split_ws_bytes, s2vt_stream stream);
/* s2vt_cast_bf16 in split form: dst (row_dst) take hi = bf16(x), dst_lo (row_dst_lo) lo = bf16(x - hi), same layouts and rules
 * (dst_lo 16-byte aligned, row_dst_lo 8-byte aligned, given together with row_dst).  NaN -> NaN / NaN; +-Inf -> +-Inf / NaN; a
 * finite x that rounds to +-Inf in bf16 -> +-Inf / -+Inf. */
int s2vt_cast_bf16_split(const float* src, int32_t ld, const int32_t* rowidx, int32_t R, int32_t C, int32_t transpose, uint16_t* dst,
                         uint16_t* dst_lo, int32_t ldd, int32_t Rp, float* colsum, uint16_t* row_dst, uint16_t* row_dst_lo, int32_t row_ldd,
                         void* scratch, size_t scratch_bytes, s2vt_stream stream);
/* C[M,N] (+)= Ah.Bh^T + Ah.Bl^T + Al.Bh^T over Kp (the layout rules of s2vt_gemm_bf16_nt for all four planes), fp32 accumulation,
 * no atomics.  scratch (optional): where the tiles do not fill the chip the reduction is split into up to 8 slabs, summed in slab
 * order, when scratch holds them (4 x slabs x M x N bytes; 32 x M x N always suffices); with less it is not split. */
int s2vt_gemm_bf16x3_nt(const uint16_t* Ah, const uint16_t* Al, int32_t lda, const uint16_t* Bh, const uint16_t* Bl, int32_t ldb, float* C,
                        int32_t ldc, int32_t M, int32_t N, int32_t Kp, int32_t accumulate, void* scratch, size_t scratch_bytes, s2vt_stream stream);
/* s2vt_gemm_bf16x3_nt without a scratch (never split), on the workgroup tile the caller names: tile 0 = 128 x 128 (what
 * s2vt_gemm_bf16x3_nt launches), 1 = 192 x 96; anything else is S2VT_E_BADARG and nothing is written.  Every output element keeps
 * one accumulator, the same K steps and the same order of the three products: the two tiles give the same bits.  A seam for
 * tests and tuning.  s2vt_gemm_bf16x3_nt_tile_choice (host only, no device needed): the tile the library's rule takes for an
 * M x N product on `cus` compute units, one workgroup per unit -- 1 where ceil(tiles192 / cus) x 192.96 is smaller than
 * ceil(tiles128 / cus) x 128.128, else 0; S2VT_E_BADARG unless all three are positive.  The sampler's pick screen
 * (s2vt_sample_screened) asks this rule with the device's unit count; the env S2VT_PICK_TILE (read once) = 0 or 1 forces its
 * tile instead.  Every other NT product of the library keeps 128 x 128. */
int s2vt_gemm_bf16x3_nt_tile(const uint16_t* Ah, const uint16_t* Al, int32_t lda, const uint16_t* Bh, const uint16_t* Bl, int32_t ldb, float* C,
                             int32_t ldc, int32_t M, int32_t N, int32_t Kp, int32_t accumulate, s2vt_stream stream, int32_t tile);
int s2vt_gemm_bf16x3_nt_tile_choice(int32_t M, int32_t N, int32_t cus);
/* C[M,N] (+)= Ah.Bh^T over Kp: the one-product form on the hi planes alone (bf16(x), what s2vt_cast_bf16_split writes to dst; the layout
 * rules of s2vt_gemm_bf16_nt), fp32 accumulation, 192 x 96 workgroup tiles, never split, no atomics.  |C - A.B^T| <= (2^-7 + 2^-11)
 * ceil(Kp / 1024) |a_m| |b_n|: the product of the sampler's default pick screen, whose margin covers exactly that -- not a gradient's. */
int s2vt_gemm_bf16x1_nt(const uint16_t* Ah, int32_t lda, const uint16_t* Bh, int32_t ldb, float* C, int32_t ldc, int32_t M, int32_t N, int32_t Kp,
                        int32_t accumulate, s2vt_stream stream);

/* The K-major form of s2vt_gemm_bf16x3_nt, for products that sum over the ROW index of both operands (weight gradients) without
 * transposed copies: C[M,N] (+)= sum over k < K of A[k][m].B[k][n] with the same three products, planes stored by rows -- A as
 * [K][lda], B as [K][ldb] (lda >= M, ldb >= N, both % 8 == 0, 16-byte aligned; K is any count: rows >= K are never read; the
 * columns of a row up to the next multiple of 128 may be read, which stays inside the planes or reads zeros; (K + 65).ld.2 bytes
 * must stay below 2 GiB).  The same K steps and accumulation order as the NT form: on planes that are each other's transposes the two
 * return the same bits.  bias (optional, [N]): the caller has put ones into column M of A's hi plane and zeros into that of its lo
 * plane (lda > M); the product's row M -- the column sums of B -- is ADDED to bias, whatever `accumulate` says.  scratch as for the
 * NT form, counting M + 1 rows with a bias. */
int s2vt_gemm_bf16x3_tn(const uint16_t* Ah, const uint16_t* Al, int32_t lda, const uint16_t* Bh, const uint16_t* Bl, int32_t ldb, float* C,
                        int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t accumulate, float* bias, void* scratch, size_t scratch_bytes,
                        s2vt_stream stream);
/* The fused form of the split mode (the default; S2VT_SPLIT_FUSED=0, read once, restores transposed casts + NT products everywhere):
 * every weight gradient runs K-major on operands cast by rows, the bias gradients embed_word_b and lstm2_b ride in their weight's
 * product as a row of ones (sums of hi + lo, 2^-17 relative per term, fixed order), and dlogits can reach the backward as planes:
 *  - s2vt_split_grad_active(N): 1 when s2vt_bptt_bwd_split at N unrolled rows runs this form (N > 256, both knobs on), else 0.
 *  - s2vt_softmax_nll_fwd_bwd_split: s2vt_softmax_nll_fwd_bwd (smoothing_rows == NULL) or _rows (smoothing_rows given, `smoothing`
 *    ignored) with the same nll / lp_target bits, but dlogits -- the same fp32 values -- is written as hi / lo planes
 *    [R][bf16_pad(V)] (pad columns zero) into split_ws, where s2vt_bptt_bwd_split(d, ..., B, N, ...) of the same d, B, N reads it,
 *    and `logits` is left unchanged.  Returns 0 then.  Returns 1 where the shape is not the in-register softmax kernel's (V % 4,
 *    V > 12288, ld % 4, alignment): dlogits is then written in place as fp32, exactly as the unfused entries do, and must be passed
 *    to the backward.  Requires s2vt_split_grad_active(N), V == d->n_words and R <= n_caption_lstm_step x N.
 *  - s2vt_bptt_bwd_split with dlogits == NULL: "the planes are in split_ws".  They are read by phase 0 and phase 1 only, with the R
 *    rows (all unrolled rows, or n_live) the softmax call wrote; phases 3 and 4 reuse that region of split_ws, so the vocabulary
 *    phase runs first -- and nothing else may use split_ws between the softmax call and it.  (Phases 2, 3 and 4 do not read dlogits
 *    and accept the same NULL.)  NULL where this form is not active (s2vt_split_grad_active(N) == 0) is a bad argument.
 *  - s2vt_split_grad_dlogits_planes: where in split_ws those planes lie (byte offsets of the hi and lo plane, elements per row). */
int s2vt_split_grad_active(int32_t N);
int s2vt_split_grad_dlogits_planes(const s2vt_dims* d, int32_t B, int32_t N, size_t* hi_offset, size_t* lo_offset, int32_t* ld);
int s2vt_softmax_nll_fwd_bwd_split(float* logits, int32_t ld, int32_t R, int32_t V, const int32_t* target, const float* coef, float smoothing,
                                   const float* smoothing_rows, float* nll, float* lp_target, const s2vt_dims* d, int32_t B, int32_t N,
                                   void* split_ws, size_t split_ws_bytes, s2vt_stream stream);

/* The forward form of the split-bf16 product: C[M,N] (+)= sum over k < K of A[m][k].B[k][n] with the same three products -- A by
 * rows as in the NT form ([M][lda], lda >= bf16_pad(K), % 8 == 0), B K-major as in the TN form ([K][ldb], ldb >= N, % 8 == 0: a
 * weight as it lies in memory, cast by rows -- no transposed copy), all planes 16-byte aligned.  A's columns in [K, bf16_pad(K)) ARE
 * read and must be finite (s2vt_cast_bf16_split leaves zeros there); B's rows >= K are never read, its columns up to the next
 * multiple of 128 may be; (bf16_pad(K) + 1).ldb.2 bytes must stay below 2 GiB, else S2VT_E_BADARG.  The same K steps and accumulation
 * order as the other two forms: the same bits as either on explicitly transposed planes.  bias (optional, fp32 [N], accumulate == 0
 * only): C = product + bias[col].  scratch as for the NT form. */
int s2vt_gemm_bf16x3_nn(const uint16_t* Ah, const uint16_t* Al, int32_t lda, const uint16_t* Bh, const uint16_t* Bl, int32_t ldb, float* C,
                        int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t accumulate, const float* bias, void* scratch, size_t scratch_bytes,
                        s2vt_stream stream);

/* The teacher-forced forward of an UPDATE whose backward is the fused split form: s2vt_teacher_forced_fwd_live with the split
 * workspace of (d, B, N) (s2vt_split_grad_workspace_bytes; validated like the backward's: S2VT_E_ALIGN when not 256-byte aligned,
 * S2VT_E_WORKSPACE when short, before anything is launched).  Both recurrences, dropout, the sampler-state reuse, live rows and
 * caption_steps are those of the live entry, bit for bit; what changes is the arithmetic of the hoisted products, by stage
 * (s2vt_split_fwd_stage(): the env S2VT_SPLIT_FWD, read once -- 0, 1 or 2; anything else or unset = the default, 1):
 *   1  the vocabulary logits O2.embed_word_W + b run as s2vt_gemm_bf16x3_nn on split-bf16 planes (within ~1e-6 of the product's
 *      maximum of the fp32 chain's value, the arithmetic the backward's gradient products already use);
 *   2  LSTM2's hoisted input partials ([O1 ; embed(prev)].lstm2_W[0:H+E], encode and decode rows) too -- LSTM2's states then differ
 *      from the live entry's by rounding-level amounts.
 * Where the shape does not fit (the split mode is not active for N: N <= 256 or S2VT_SPLIT_GRADS=0; lstm_dim % 8; planes beyond the
 * K-major loader's reach) or at stage 0 the fp32 products run and the call IS s2vt_teacher_forced_fwd_live.  S2VT_SPLIT_FUSED, which
 * picks the operand layout of the BACKWARD's products, does not change the forward.  The forward uses AT, W (and at stage 2 BT) of
 * the split workspace and never the dlogits planes' region.  The token-deciding paths never come here.
 * s2vt_split_fwd_active(N): the stage that applies at N unrolled rows (0: the fp32 products). */
int s2vt_split_fwd_stage(void);
int s2vt_split_fwd_active(int32_t N);
int s2vt_teacher_forced_fwd_split(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t N,
                                  const int32_t* caption, int32_t caption_steps, const int32_t* live_rows, int32_t n_live, float keep,
                                  uint64_t seed, const int32_t* video_id, const int32_t* sample_id, float* logits_out,
                                  void* workspace, size_t workspace_bytes, const void* sampler_workspace,
                                  size_t sampler_workspace_bytes, int32_t sampler_rows, void* split_ws, size_t split_ws_bytes,
                                  s2vt_stream stream);

/* Gradient w.r.t. the frame features, for the end-to-end scripts where they are the CNN's output
 * (e2e_tf_s2vt.py:106-121,163-166: the optimizer differentiates through `video` into Inception-ResNet-v2):
 * d_video[B, Tv, dim_image] = d_emb @ encode_image_W^T, from the d_emb the preceding s2vt_bptt_bwd (phase 0 or 2)
 * left in `workspace`.  Unnormalised like the weight gradients (scale by 1/sum(mask) as s2vt_grad_finalize does). */
int s2vt_bptt_dvideo(const s2vt_dims* d, const s2vt_params* p, int32_t B, int32_t N, float* d_video, void* workspace,
                      size_t workspace_bytes, s2vt_stream stream);

/* dWemb[idx[r], :] += dE[r, :]  -- gradient of tf.nn.embedding_lookup (tf_s2vt.py:128-134). */
int s2vt_embed_scatter_add(const float* dE, int32_t ld, const int32_t* idx, int32_t R, int32_t E, float* dWemb,
                           s2vt_stream stream);
/* dWemb[idx_a[r], :] += scale * dE[r, :] and dWemb[idx_b[r], :] += scale * dE[r, :] -- the gradient of a scaled sum of two lookups
 * (average_generate_words_tf_s2vt.py:131-133, scale = 1/2); a row whose two ids are equal receives both additions.  dE [R, ld >= E];
 * the ids must lie inside dWemb.  R = 0: nothing is launched. */
int s2vt_embed_scatter_add2(const float* dE, int32_t ld, const int32_t* idx_a, const int32_t* idx_b, float scale, int32_t R, int32_t E,
                            float* dWemb, s2vt_stream stream);
/* dWemb[ids[r][j], :] += w[r][j] * dE[r, :] for j < k -- the gradient of a weighted sum of k lookups with the weights held fixed
 * (sum_generate_words_tf_s2vt.py:171-173); ids, w [R, k], 1 <= k <= 8; equal ids in a row each receive their addition.  dE [R, ld >= E];
 * the ids must lie inside dWemb.  R = 0: nothing is launched. */
int s2vt_embed_scatter_addk(const float* dE, int32_t ld, const int32_t* ids, const float* w, int32_t k, int32_t R, int32_t E, float* dWemb,
                            s2vt_stream stream);

/* ---- host glue of the REINFORCE step, on the device (decode_captions_masks, cider_evaluation.py:145-172; the objective's
 * coefficients, reinforcement_multisampling_tf_s2vt.py:641-646).
 * s2vt_caption_mask: ids [N, Tc] -> mask [N, Tc] (1 up to and including the first <eos> = 0; may be NULL), target_tm [Tc*N]
 *   (the ids time-major, what s2vt_softmax_nll_fwd_bwd takes; may be NULL), *mask_sum = *mask_sum_copy = sum(mask) (each may be NULL).
 * s2vt_pg_coef: coef_tm[t*N + n] = mask[n][t] * (rewards[n] - baseline[n]) * scale  (rewards NULL = 1, baseline NULL = 0).
 * s2vt_step_scalars: *loss = sum(coef * nll) / *mask_sum_local, *gscale = 1 / *mask_sum_global (the bucket's tail slot after the
 *   all-reduce), *sumsq = 0 -- every output optional; one launch. */
int s2vt_caption_mask(const int32_t* ids, int32_t N, int32_t Tc, float* mask, int32_t* target_tm, float* mask_sum, float* mask_sum_copy, s2vt_stream stream);
int s2vt_pg_coef(const float* mask, const float* rewards, const float* baseline, float scale, int32_t N, int32_t Tc, float* coef_tm,
                 s2vt_stream stream);
int s2vt_step_scalars(const float* coef, const float* nll, int64_t R, const float* mask_sum_local, const float* mask_sum_global, float* loss,
                      float* gscale, float* sumsq, s2vt_stream stream);

/* ---- the same for the XE update (tf_s2vt.py:150-166) and the mixed multitask objective (reinforce_multitask_e2e_attribute_s2vt.py:850):
 * one launch each instead of the tensor-library expressions (single process; a data-parallel caller needs the GLOBAL column
 * sums and keeps its own expressions).  Tc <= 128.
 * s2vt_xe_prep: coef_tm[t*N + n] = q1 ? (sum_n' mask[n'][t] / n_global) * loss_weight : mask[n][t] * loss_weight;
 *   target_tm[t*N + n] = caption[n][t] (may be NULL); *mask_sum = sum(mask) (may be NULL).
 * s2vt_mixed_prep: rows 0..Ns-1 = the sampled captions, Ns..Ns+B-1 = the ground truth (N = Ns + B):
 *   coef_tm[t*N + n] = n < Ns ? mask[n][t] * ((rewards[n] - baseline[n]) * (1 - lambda)) / sum(mask)
 *                             : (q1 ? (sum_b gt_mask[b][t] / n_global_b) * loss_weight : gt_mask[n-Ns][t] * loss_weight) * (lambda / sum(gt_mask));
 *   smooth_tm[t*N + n] = n < Ns ? 0 : smoothing;  caption_all [N, Tc] = [sampled ; gt_caption], target_tm [Tc*N] the same ids time-major;
 *   sums = {sum(mask), sum(gt_mask)}.  lambda_loss is a DOUBLE: (1 - lambda) is formed in double and rounded to fp32 once, lambda itself
 *   rounded to fp32 -- what the tensor expressions of a data-parallel caller (model.mixed_update) do with a Python float, so the two
 *   paths give the same bits for a non-dyadic lambda (0.9: 0.1 -> 0x3dcccccd, not the 0x3dccccd0 of 1 - fl32(0.9)).
 * s2vt_mixed_loss: out3 = {sum over sampled rows, sum over ground-truth rows, both} of coef[r] * nll[r], r < R; the row of entry r is
 *   (live_rows ? live_rows[r] : r) % N. */
int s2vt_xe_prep(const float* mask, const int32_t* caption, int32_t N, int32_t Tc, float loss_weight, float n_global, int32_t q1, float* coef_tm,
                 int32_t* target_tm, float* mask_sum, s2vt_stream stream);
int s2vt_mixed_prep(const float* mask, const float* gt_mask, const float* rewards, const float* baseline, const int32_t* sampled,
                    const int32_t* gt_caption, int32_t Ns, int32_t B, int32_t Tc, double lambda_loss, float loss_weight, int32_t q1,
                    float smoothing, float n_global_b, float* coef_tm, float* smooth_tm, int32_t* caption_all, int32_t* target_tm, float* sums, s2vt_stream stream);
int s2vt_mixed_loss(const float* coef, const float* nll, const int32_t* live_rows, int64_t R, int32_t N, int32_t Ns, float* out3, s2vt_stream stream);

/* ---- gradient finalisation + tf.clip_by_global_norm + tf.train.AdamOptimizer ------------------
 * (reinforcement_multisampling_tf_s2vt.py:638-652; tf_s2vt.py:163-166,445-448).
 * s2vt_grad_finalize: g <- g * (*gscale) + weight_decay * theta over one flat range, and
 *   *sumsq += sum g^2.  gscale (device scalar, may be NULL = 1) carries 1/sum(mask) computed after
 *   the all-reduce; weight_decay implements decay_value * l2_loss for the decayed variables (Q3).
 * s2vt_adam_tf: g' = g * clip_norm / max(sqrt(*sumsq), clip_norm) (clip_norm <= 0 or sumsq NULL:
 *   no clipping), then TF-form Adam with step count `step` >= 1 (epsilon outside the bias
 *   correction). */
int s2vt_grad_finalize(float* g, const float* theta, int64_t n, const float* gscale, float weight_decay, float* sumsq,
                       s2vt_stream stream);
int s2vt_adam_tf(float* theta, const float* g, float* m, float* v, int64_t n, const float* sumsq, float clip_norm,
                 float lr, int64_t step, float beta1, float beta2, float eps, s2vt_stream stream);
/* The same update with a receipt: when the launch applies the update it writes `step` to *applied_step (device int32).
 * Every s2vt_adam_tf* launch is a no-op ON THE DEVICE while a persistent-recurrence fault is pending (s2vt_chain_fault):
 * gradients computed from a starved recurrence never reach the variables, and after a device synchronise
 * *applied_step tells the host which update was the last one applied. */
int s2vt_adam_tf_guarded(float* theta, const float* g, float* m, float* v, int64_t n, const float* sumsq, float clip_norm,
                         float lr, int64_t step, float beta1, float beta2, float eps, int32_t* applied_step, s2vt_stream stream);

/* tf.train.GradientDescentOptimizer behind tf.clip_by_global_norm (generate_words_tf_s2vt.py:412-418): theta -= lr * g * clip_norm /
 * max(sqrt(*sumsq), clip_norm) over one flat range (clip_norm <= 0 or sumsq NULL: no clipping, as s2vt_adam_tf), step >= 1.  The same
 * receipt (*applied_step = step, may be NULL) and the same on-device no-op while a persistent-recurrence fault is pending as
 * s2vt_adam_tf_guarded. */
int s2vt_sgd_guarded(float* theta, const float* g, int64_t n, const float* sumsq, float clip_norm, float lr, int64_t step, int32_t* applied_step,
                     s2vt_stream stream);

/* ---- temporal attention, one decode step (original_attention.py:106-128) ----------------------
 * Inputs: hWa [B,H] = h_prev @ embed_att_Wa (s2vt_gemm); P [Tv,B,H] = Vt @ embed_att_Ua + ba (hoisted,
 * :107); Vt [Tv,B,H] frame embeddings; w [H] = embed_att_w.
 *   scores[t,b] = sum_h tanh(hWa[b,h] + P[t,b,h]) * w[h]            (:113-115)
 *   alpha[t,b]  = exp(scores) / (sum_t exp(scores) (+1 if that sum is 0))   (:116-121, no max shift)
 *   ctx[b,h]    = sum_t alpha[t,b] * Vt[t,b,h]                       (:127-128)
 * Backward: given dctx [B,H] returns dhWa [B,H], dP [Tv,B,H], dVt [Tv,B,H] (the context path only;
 * add dP @ Ua^T upstream) and ACCUMULATES dw [H].  de_scratch: [Tv*B] floats. */
int s2vt_attention_fwd(const float* hWa, const float* P, const float* Vt, const float* w, float* scores, float* alpha,
                       float* ctx, int32_t Tv, int32_t B, int32_t H, s2vt_stream stream);
int s2vt_attention_bwd(const float* hWa, const float* P, const float* Vt, const float* w, const float* alpha,
                       const float* dctx, float* de_scratch, float* dhWa, float* dP, float* dVt, float* dw, int32_t Tv,
                       int32_t B, int32_t H, s2vt_stream stream);

/* The row -> video forms of the two calls above, for rows that share image blocks (the K samples of a video in self-critical
 * REINFORCE): N = n_video * samples rows, sample-major -- row s * n_video + j is sample s of video j -- over P / Vt [Tv, n_video, H],
 * ONE block per video.  hWa, dctx, dhWa, ctx [N, H] and scores, alpha [Tv, N] stay per row.  Forward: the same chains as
 * s2vt_attention_fwd, so bit-identical to it on P / Vt tiled `samples` times; row_video_scratch: [N] int32.  Backward: dP / dVt
 * [Tv, n_video, H] take the SUM over the video's rows (acc != 0: added to what is there), with no atomics -- every element has one
 * owning thread that adds the rows in ascending s, so two runs give equal bits; dw [H] is accumulated with atomicAdd as above.
 * de_scratch: [N * Tv] floats. */
int s2vt_attention_fwd_rows(const float* hWa, const float* P, const float* Vt, const float* w, float* scores, float* alpha, float* ctx,
                            int32_t* row_video_scratch, int32_t Tv, int32_t n_video, int32_t samples, int32_t H, s2vt_stream stream);
int s2vt_attention_bwd_rows(const float* hWa, const float* P, const float* Vt, const float* w, const float* alpha, const float* dctx,
                            float* de_scratch, float* dhWa, float* dP, float* dVt, float* dw, int32_t Tv, int32_t n_video,
                            int32_t samples, int32_t H, int32_t acc, s2vt_stream stream);

/* ---- the temporal-attention captioner as a whole model (original_attention.py:53-251) -----------
 * Variables of original_attention.py:55-86 in the reference's own layouts (names = the TF variable names; LSTM3 lives under
 * s2vt/LSTM3/basic_lstm_cell).  The word embedding has dim_hidden columns (:65); s2vt_dims.word_dim is ignored here.
 * Numeric contract: every pre-activation is one ascending-k fmaf chain over the rows of its matrix, the
 * row blocks in order of availability -- LSTM3: current_embed [H:2H], h [2H:3H], atten [0:H]; output layer: current_embed
 * [2H:3H], atten [H:2H], output1 [0:H]; forward activations, alphas, logits and greedy ids are bit-identical to
 * oracle/s2vt_oracle.py::attention_forward.  n_video_lstm_step <= 64. */
typedef struct s2vt_attn_params {
    float* Wemb;            /* [V, H] */
    float* encode_image_W;  /* [D, H] */
    float* encode_image_b;  /* [H] */
    float* embed_att_w;     /* [H] (TF shape [H, 1]) */
    float* embed_att_Wa;    /* [H, H] */
    float* embed_att_Ua;    /* [H, H] */
    float* embed_att_ba;    /* [H] */
    float* embed_word_W;    /* [H, V] */
    float* embed_word_b;    /* [V] */
    float* embed_nn_Wp;     /* [3H, H]  rows [output1 ; atten ; current_embed]  (:134) */
    float* embed_nn_bp;     /* [H] */
    float* lstm3_W;         /* [3H, 4H] rows [atten ; current_embed ; h], columns [i | j | f | o]  (:131) */
    float* lstm3_b;         /* [4H] */
} s2vt_attn_params;

size_t s2vt_attn_workspace_bytes(const s2vt_dims* d, int32_t B);
/* build_model's unroll (:88-143) on B rows with the DropoutWrapper on LSTM3's output (keep, Philox stream as the S2VT cells:
 * code 768 + step): logits [caption_steps*B, V] time-major (row t*B + b); caption [B, Tc] int32 (the word fed at step t is
 * caption[:, t-1], zeros at t = 0, :105,141-142).  caption_steps (1..Tc): unroll only the leading steps (every later position of
 * the batch is masked).  alphas_out: optional [caption_steps][Tv][B].  Activations stay in the workspace for s2vt_attn_bptt_bwd. */
int s2vt_attn_teacher_forced_fwd(const s2vt_dims* d, const s2vt_attn_params* p, const float* video, int32_t B, const int32_t* caption,
                                 int32_t caption_steps, float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id,
                                 float* logits, float* alphas_out, void* workspace, size_t workspace_bytes, s2vt_stream stream);
/* The loss kernels' inputs from what build_model is fed: caption [B, Tc] int32 and caption_mask [B, Tc] (row-major) -> time-major
 * target_tm[t*B + b], coef_tm[t*B + b] = mask[b, t] (cross_entropy * caption_mask[:, i], :145), reg_tm = beta * mask (NULL: not wanted),
 * *mask_sum = sum(mask) (:149).  One launch. */
int s2vt_attn_loss_inputs(const int32_t* caption, const float* mask, int32_t B, int32_t Tc, float beta, int32_t* target_tm, float* coef_tm,
                          float* reg_tm, float* mask_sum, s2vt_stream stream);
/* loss = (sum_r coef[r] * nll[r] + sum_r reg_coef[r] * max(0, reg_m - sum(alpha[0:8])[r])) / *mask_sum_local  (:144-149; reg_coef =
 * beta * mask time-major or NULL, reg_m = m; the first-8-frames sums are the ones the forward left in the workspace);
 * *gscale = 1 / *mask_sum_global; *sumsq = 0.  One launch, after s2vt_attn_teacher_forced_fwd on the same workspace. */
int s2vt_attn_step_scalars(const float* coef, const float* nll, int64_t R, const float* reg_coef, float reg_m, const float* mask_sum_local,
                           const float* mask_sum_global, float* loss, float* gscale, float* sumsq, const s2vt_dims* d, int32_t B,
                           void* workspace, size_t workspace_bytes, s2vt_stream stream);
/* tf.gradients of (sum coef * nll + sum regulariser) through the unroll the forward call left in the workspace: dlogits
 * [caption_steps*B, V] = d/dlogits (s2vt_softmax_nll_fwd_bwd), reg_coef [caption_steps*B] = beta * mask[b, t] time-major or NULL.
 * ACCUMULATES into `grads` (same layout as the variables; un-normalised: scale by 1 / sum(mask) afterwards).  lstm_dim % 4 == 0. */
int s2vt_attn_bptt_bwd(const s2vt_dims* d, const s2vt_attn_params* p, const s2vt_attn_params* grads, const float* video, int32_t B,
                       const float* dlogits, int32_t caption_steps, const float* reg_coef, float reg_m, float keep, uint64_t seed,
                       const int32_t* video_id, const int32_t* sample_id, void* workspace, size_t workspace_bytes, s2vt_stream stream);
/* build_generator / build_sampler (:155-251): greedy decode of B videos, the whole loop on the device (the picked word of step
 * t-1 is the gather index of step t's embedding operand); ids_out [B, Tc] int32, alphas_out optional [Tc][Tv][B] (saved_alphas). */
int s2vt_attn_decode_greedy(const s2vt_dims* d, const s2vt_attn_params* p, const float* video, int32_t B, int32_t video_base, int32_t* ids_out,
                            float* alphas_out, void* workspace, size_t workspace_bytes, s2vt_stream stream);

/* ---- self-critical REINFORCE on the attention captioner: rows that share image blocks ---------------------------------------
 * Rows are sample-major everywhere: row s * B + j is sample s of video j (as on the S2VT path); a greedy block comes last with
 * sample id -1.  These forms run the per-step launches: the persistent recurrences (attn_chain*.hip) hold one image block per row and
 * at most 64 rows, and are not used here.
 *
 * s2vt_attn_sample: K multinomial captions per video (+ the greedy one) -- ONE prologue (frame embedding, V @ Ua + ba) for the B
 * videos, then the decode loop of s2vt_attn_decode_greedy on (K + with_greedy) * B rows with the attention step in its row -> video
 * form.  Gumbel-max over Philox with counters (video_base + j, s, step) and `seed`; the greedy block takes the argmax.  No dropout, no
 * <bos>, no host round trip per step.  ids_out [K*B, Tc] (NULL when K = 0), greedy_out [B, Tc] (NULL without with_greedy), int32.
 * K = 0 with with_greedy gives the ids of s2vt_attn_decode_greedy.  ..._workspace_bytes: 0 on bad arguments. */
size_t s2vt_attn_sample_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t K, int32_t with_greedy);
int s2vt_attn_sample(const s2vt_dims* d, const s2vt_attn_params* p, const float* video, int32_t B, int32_t K, int32_t with_greedy, uint64_t seed,
                     int32_t video_base, int32_t* ids_out, int32_t* greedy_out, void* workspace, size_t workspace_bytes, s2vt_stream stream);
/* s2vt_attn_sample with flags (bit 0 = S2VT_SAMPLE_STOP_AT_EOS; any other bit: S2VT_E_BADARG; flags == 0 is s2vt_attn_sample).  Same
 * argument checks, same workspace (s2vt_attn_sample_workspace_bytes serves both), K = 0 with with_greedy allowed.
 * S2VT_SAMPLE_STOP_AT_EOS (opt-in; NOT what the reference's samplers do, which run all Tc steps for every row): a row leaves the decode
 * loop once it has picked <eos> = 0 -- every later step's launches (query projection, attention step, LSTM3, output layer, vocabulary
 * pick) cover the rows still sampling only, through a compact row list and its length kept on the device; no host round trip.
 * Contract: for every row of ids_out / greedy_out, the ids up to and including the row's first <eos> are bit-identical to
 * s2vt_attn_sample's, and the ids behind it are 0.  Every element of both arrays is written.  Those leading ids are the only positions
 * the objective's mask keeps, so the REINFORCE update is the same update. */
int s2vt_attn_sample_ex(const s2vt_dims* d, const s2vt_attn_params* p, const float* video, int32_t B, int32_t K, int32_t with_greedy, uint64_t seed,
                        int32_t video_base, int32_t flags, int32_t* ids_out, int32_t* greedy_out, void* workspace, size_t workspace_bytes,
                        s2vt_stream stream);
/* Workspace of the three calls below for N = n_video * samples rows over n_video image blocks (0 on bad arguments). */
size_t s2vt_attn_rows_workspace_bytes(const s2vt_dims* d, int32_t n_video, int32_t samples);
/* s2vt_attn_teacher_forced_fwd on N rows that share n_video image blocks: caption [N, Tc], video [n_video, Tv, D], video_id / sample_id
 * [N] for LSTM3's dropout stream (code 768 + step); logits [caption_steps*N, V], alphas_out [caption_steps][Tv][N], the first-8-frames
 * sums per row.  The chains of the numeric contract in the same block order: logits and alphas are bit-identical to
 * s2vt_attn_teacher_forced_fwd on the feature block tiled `samples` times. */
int s2vt_attn_teacher_forced_fwd_rows(const s2vt_dims* d, const s2vt_attn_params* p, const float* video, int32_t n_video, int32_t samples,
                                      const int32_t* caption, int32_t caption_steps, float keep, uint64_t seed, const int32_t* video_id,
                                      const int32_t* sample_id, float* logits, float* alphas_out, void* workspace, size_t workspace_bytes,
                                      s2vt_stream stream);
/* s2vt_attn_step_scalars after s2vt_attn_teacher_forced_fwd_rows on the same workspace (R <= Tc * N). */
int s2vt_attn_step_scalars_rows(const float* coef, const float* nll, int64_t R, const float* reg_coef, float reg_m, const float* mask_sum_local,
                                const float* mask_sum_global, float* loss, float* gscale, float* sumsq, const s2vt_dims* d, int32_t n_video,
                                int32_t samples, void* workspace, size_t workspace_bytes, s2vt_stream stream);
/* s2vt_attn_bptt_bwd through that unroll: dlogits [caption_steps*N, V], reg_coef [caption_steps*N] or NULL; ACCUMULATES into `grads`.
 * The gradients of the image blocks are [Tv, n_video, H], summed over the video's rows and the steps without atomics
 * (s2vt_attention_bwd_rows); the Ua / ba / encode_image products run on Tv * n_video rows. */
int s2vt_attn_bptt_bwd_rows(const s2vt_dims* d, const s2vt_attn_params* p, const s2vt_attn_params* grads, const float* video, int32_t n_video,
                            int32_t samples, const float* dlogits, int32_t caption_steps, const float* reg_coef, float reg_m, float keep,
                            uint64_t seed, const int32_t* video_id, const int32_t* sample_id, void* workspace, size_t workspace_bytes,
                            s2vt_stream stream);

/* ---- batched beam search for the attention captioner: the decode step of build_generator / build_sampler
 * (original_attention.py:155-251) under the beam bookkeeping of final_beam_search.py:201-294, for B videos at once.  Same division of
 * work as s2vt_beam_*: one call per decode step advances every live hypothesis of every video, the heaps stay on the host.
 *
 * Workspace of a decoder for B videos and up to beam hypotheses per video (1 <= beam <= 16): the frame embeddings and the hoisted
 * image part for B videos -- ONE [Tv, H] block each per video, shared by its hypotheses, never copied per hypothesis -- plus two
 * LSTM3 state buffers, the step's activations and logits for B * beam rows.  0 on bad arguments (n_video_lstm_step <= 64). */
size_t s2vt_attn_beam_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t beam);
/* Frame embedding V = video @ encode_image_W + b (time-major, :159-162) and the hoisted image part V @ Ua + ba (:171) of the B videos:
 * everything of a decode step that does not depend on a word. */
int s2vt_attn_beam_encode(const s2vt_dims* d, const s2vt_attn_params* p, const float* video, int32_t B, int32_t beam, void* workspace,
                          size_t workspace_bytes, s2vt_stream stream);
/* Decode step t (0 <= t < Tc) for R <= B * beam live hypotheses, no host synchronisation; steps are issued in order t = 0, 1, ...
 * Hypothesis m continues video video_of_row[m] from row parent[m] of step t - 1 with word[m]; at t = 0 it starts from the zero state
 * with no word (state1 = h_prev = current_embed = 0, :164-169: parent and word are ignored -- this model feeds no <bos>).  The step is query h @ Wa ->
 * score / softmax / context over the video's block (row -> video: the image blocks are indexed through video_of_row) -> LSTM3 ->
 * tanh([embed ; atten ; output1] @ Wp + bp) -> vocabulary logits, no dropout (:188), each chain in the block order of the numeric
 * contract above: the logits of a hypothesis are bit-identical to what s2vt_attn_teacher_forced_fwd (keep = 1) gives at step t for
 * that hypothesis' word prefix.  The three int32 [R] arrays are device pointers; indices out of range are clamped, not reported.
 * Writes top_ids / top_logp [R, k] (s2vt_vocab_topk of the step's logits) and, when given, logits_out [R, V] and alphas_out [Tv][R]. */
int s2vt_attn_beam_step(const s2vt_dims* d, const s2vt_attn_params* p, int32_t B, int32_t beam, int32_t t, int32_t R,
                        const int32_t* video_of_row, const int32_t* parent, const int32_t* word, int32_t k, int32_t* top_ids, float* top_logp,
                        float* logits_out, float* alphas_out, void* workspace, size_t workspace_bytes, s2vt_stream stream);

/* ---- multitask attribute head (reinforce_multitask_e2e_attribute_loss.py:375-380, 606-626) -----
 * mean_feat[b,:] = mean_t video[b,t,:]; z = mean_feat @ attr_W + attr_b;
 * bce = max(z,0) - z*y + log(1+exp(-|z|))  (tf.nn.sigmoid_cross_entropy_with_logits); labels/bce optional.
 * Backward: dz = scale * (sigmoid(z) - y); d_attr_W += mean_feat^T dz; d_attr_b += colsum(dz)
 * (scale = alpha / (A * B_global) for the normalised multilabel loss at :379,957). */
int s2vt_attr_head_fwd(const float* video, int32_t B, int32_t Tv, int32_t D, const float* attr_W, const float* attr_b,
                       int32_t A, const float* labels, float* mean_feat, float* z, float* bce, s2vt_stream stream);
int s2vt_attr_head_bwd(const float* mean_feat, const float* z, const float* labels, int32_t B, int32_t D, int32_t A,
                       float scale, float* dz_scratch, float* d_attr_W, float* d_attr_b, s2vt_stream stream);
/* evaluate_multilabel (reinforce_multitask_e2e_attribute_loss.py:606-626): the head's forward followed by
 * scores[B, A] = sigmoid(z) (:624).  mean_feat [B, D] and z [B, A] are written as by s2vt_attr_head_fwd. */
int s2vt_attr_head_scores(const float* video, int32_t B, int32_t Tv, int32_t D, const float* attr_W, const float* attr_b,
                          int32_t A, float* mean_feat, float* z, float* scores, s2vt_stream stream);

/* ==== session API + the single-op entry points of the boundary ============= */

/* ---- session handle: owns ONE device workspace sized for (max_B, max_K); nothing else is allocated.
 * s2vt_encode_fwd = encoding stage (tf_s2vt.py:97-122) + the decode-stage work that does not depend on a
 * sampled word (the LSTM1 trajectory and its W2 partials); s2vt_decode_greedy = build_sampler
 * (tf_s2vt.py:217-266; B = 1 is build_generator :169-214); s2vt_decode_multinomial = K runs of
 * build_multinomial_sampler (reinforcement_multisampling_tf_s2vt.py:294-339, driven at :743-753) on the
 * SAME encode -- any number of decode calls may follow one encode call.  ids_out: int32 [B, Tc] resp.
 * [K*B, Tc] (sample-major).  One handle per (device, stream); a handle is not thread-safe. */
typedef struct s2vt_handle s2vt_handle;
int s2vt_create(const s2vt_dims* d, int32_t max_B, int32_t max_K, s2vt_handle** out);
int s2vt_destroy(s2vt_handle* h);
int s2vt_encode_fwd(s2vt_handle* h, const s2vt_params* p, const float* video, int32_t B, s2vt_stream stream);
int s2vt_decode_greedy(s2vt_handle* h, const s2vt_params* p, int32_t* ids_out, s2vt_stream stream);
int s2vt_decode_multinomial(s2vt_handle* h, const s2vt_params* p, int32_t K, uint64_t seed, int32_t video_base,
                            int32_t* ids_out, s2vt_stream stream);

/* ---- BasicLSTMCell weight layouts.  The kernels consume the TF layout directly (W[in+H, 4H], columns
 * [i | j | f | o], rows [x ; h]); these convert to / from a split, gate-interleaved form
 * (Wx[in, H, 4], Wh[H, H, 4]: the four gates of a unit adjacent) for hosts that keep i2h / h2h apart. */
int s2vt_pack_weights(const float* W_tf, int32_t in_dim, int32_t H, float* Wx_packed, float* Wh_packed, s2vt_stream stream);
int s2vt_unpack_weights(const float* Wx_packed, const float* Wh_packed, int32_t in_dim, int32_t H, float* W_tf,
                        s2vt_stream stream);

/* ---- frame embedding backward (gradient of tf.nn.xw_plus_b, tf_s2vt.py:98): ACCUMULATES
 * d_encode_image_W[d, E] += video[B*Tv, d]^T @ d_emb[B*Tv, E] and d_encode_image_b[E] += colsum(d_emb). */
int s2vt_frame_embed_bwd(const s2vt_dims* d, const float* video, const float* d_emb, int32_t B, float* d_encode_image_W,
                         float* d_encode_image_b, s2vt_stream stream);

/* ---- BasicLSTMCell backward, one step (inverse of s2vt_lstm_cell_fwd's pointwise part): gates [M,4H] as
 * saved by the forward, dh [M,H] = total gradient w.r.t. h' (recurrent + output), dc_in [M,H] or NULL,
 * c_prev NULL = zero state.  Writes dz [M,4H] (pre-activation gate gradients, columns i|j|f|o) and
 * dc_prev [M,H]; the weight / input gradients are contractions with dz (s2vt_gemm / s2vt_bptt_bwd). */
int s2vt_lstm_cell_bwd(const float* gates, const float* c_new, const float* c_prev, const float* dh, const float* dc_in,
                       float* dz, float* dc_prev, int32_t M, int32_t H, s2vt_stream stream);

/* ---- build_generator's word choice exactly as the reference writes it (tf_s2vt.py:208-209): p = exp(l) / sum(exp(l))
 * WITHOUT a max shift, in fp32, then argmax (first maximum wins; NaN never wins; all-NaN -> 0).  A logit >= 88.72
 * overflows to inf / inf = NaN and the choice becomes <eos> = 0 instead of argmax(l).  ids [R]; probs [R, V] or NULL. */
int s2vt_softmax_unshifted_argmax(const float* logits, int32_t ld, int32_t R, int32_t V, int32_t* ids, float* probs,
                                  s2vt_stream stream);

/* ---- the two objectives by name.  s2vt_xent_smooth_fwd_bwd: tf.losses.softmax_cross_entropy with
 * label_smoothing (tf_s2vt.py:155).  s2vt_pg_nll_fwd_bwd: the reward-scaled NLL of
 * reinforcement_multisampling_tf_s2vt.py:286-291,643-646 -- coef[t*N+n] = adv[n] * mask[n,t] is formed on
 * the device (coef_scratch: N*Tc floats), logits/target time-major; both overwrite logits with d/dlogits. */
int s2vt_xent_smooth_fwd_bwd(float* logits, int32_t ld, int32_t R, int32_t V, const int32_t* target, const float* coef,
                             float label_smoothing, float* nll, s2vt_stream stream);
int s2vt_pg_nll_fwd_bwd(float* logits, int32_t ld, int32_t N, int32_t Tc, int32_t V, const int32_t* target_tm,
                        const float* adv, const float* mask, float* coef_scratch, float* nll, float* lp_target,
                        s2vt_stream stream);

/* out[r, :] = Wemb[idx[r], :]  -- tf.nn.embedding_lookup (tf_s2vt.py:128-134). */
int s2vt_embed_gather(const float* Wemb, int32_t ldw, const int32_t* idx, int32_t R, int32_t E, float* out, int32_t ldo,
                      s2vt_stream stream);

/* tf.clip_by_global_norm over one flat range (reinforcement_multisampling_tf_s2vt.py:650):
 * g *= clip_norm / max(||g||, clip_norm); *sumsq_scratch receives ||g||^2 (before clipping). */
int s2vt_global_norm_clip(float* g, int64_t n, float clip_norm, float* sumsq_scratch, s2vt_stream stream);

/* ---- generic order-free pieces for backward graphs composed on the host (used by the attention captioner's
 * training step, attention.py; the S2VT path has them fused inside s2vt_bptt_bwd) ---------------------------
 * s2vt_gemm_tn : C[Kout,N] (+)= A[row(m), :Kout]^T @ B[m, :N] over m < Mred  (weight gradients; rowidx gathers rows)
 * s2vt_transpose: out[c, r] = in[r, c]                       s2vt_colsum: out[n] += sum_m X[m, n]  (bias gradients)
 * s2vt_tanh_bwd : dx = dy * (1 - y^2)                        s2vt_dropout_bwd: dh = (dout / keep) * mask, the adjoint
 *                 of the DropoutWrapper output of s2vt_lstm_cell_fwd (same seed / ids / drop_code). */
int s2vt_gemm_tn(const float* A, int32_t lda, const int32_t* rowidx, const float* B, int32_t ldb, float* C, int32_t ldc,
                 int32_t Mred, int32_t Kout, int32_t N, int32_t accumulate, s2vt_stream stream);
int s2vt_transpose(const float* in, int32_t ldi, float* out, int32_t ldo, int32_t R, int32_t Cc, s2vt_stream stream);
int s2vt_colsum(const float* X, int32_t ld, int32_t M, int32_t N, float* out, s2vt_stream stream);
int s2vt_tanh_bwd(const float* y, const float* dy, float* dx, int64_t n, s2vt_stream stream);
int s2vt_dropout_bwd(const float* dout, int32_t ld, float* dh, int32_t M, int32_t H, float keep, uint64_t seed,
                     uint32_t drop_code, const int32_t* video_id, const int32_t* sample_id, s2vt_stream stream);

/* ---- a whole BasicLSTMCell recurrence in one call: the unroll of tf_s2vt.py:113-153 for a cell whose step input is
 * known before the loop.  Step t = 0 .. T-1:  z = cinit_t (+) H_hist[t] @ W[kw0 : kw0 + H, :]  (cinit_t = cinit +
 * t * cinit_tstride, rows ldcinit apart, for t < cinit_steps; absent otherwise), BasicLSTMCell pointwise with C_hist[t],
 * results to C_hist[t+1], H_hist[t+1] ([T+1, M, H], slot 0 = the initial state), the activated gates to gates[t]
 * ([T, M, 4H] or NULL; may alias cinit) and the DropoutWrapper output to out[t] ([T, M, H] or NULL; Philox code
 * drop_code0 + t).  persistent = 1: ONE persistent launch with the recurrent weights resident in LDS and the state
 * exchanged through L2 (needs M <= 384, H % 4 == 0, H <= 1024, H / 4 <= the CU count; S2VT_E_BADARG otherwise); 0: T launches of
 * the fused cell kernel; -1: persistent when the shape fits.  Both forms give the same bits.  scratch:
 * s2vt_lstm_recurrence_scratch_bytes(H) bytes, 256-byte aligned (persistent form only). */
size_t s2vt_lstm_recurrence_scratch_bytes(int32_t H);
int s2vt_lstm_recurrence_fwd(const float* W, int32_t kw0, const float* b, const float* cinit, int64_t cinit_tstride, int32_t ldcinit,
                             int32_t cinit_steps, float* C_hist, float* H_hist, float* gates, float* out, int32_t M, int32_t H,
                             int32_t T, float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id,
                             uint32_t drop_code0, int32_t persistent, void* scratch, size_t scratch_bytes, s2vt_stream stream);
/* ---- two such recurrences on the same rows behind one call: LSTM1 of the bidirectional captioner (bidirection_tf_s2vt.py:113-121,
 * static_bidirectional_rnn over the frames and the zero padding; the cell has no DropoutWrapper).  Each direction is described in
 * CHAIN-STEP order: step t = 0 .. T-1 reads slot t of its C_hist / H_hist ([T+1, M, H], slot 0 = the initial state), writes slot
 * t + 1 and gates[t] ([T, M, 4H] activated, or NULL; gates == cinit is refused: the window moves, the gates must not overwrite it).  Its carried partial covers the window of steps
 * [cinit_t0, cinit_t0 + cinit_steps): step t continues from cinit + (t - cinit_t0) * cinit_tstride (rows ldcinit apart); cinit_tstride
 * may be negative.  The forward direction takes the hoisted frame products as a prefix (t0 = 0, steps = Tv); the backward direction
 * consumes time T-1 .. 0, so its slot k + 1 is the state after time T-1-k and the frame products are a suffix read backwards
 * (t0 = Tc, steps = Tv, cinit = the product of frame Tv-1, cinit_tstride = -(one frame's stride)).
 * persistent = 1: ONE persistent launch advances both directions behind one grid hand-off per step -- a workgroup keeps the
 * [H x 16] slices of both cells in LDS and a wave interleaves the two MFMA chains (M <= 64, H % 4 == 0, H <= 1024, H / 4 <= the
 * CU count; S2VT_E_BADARG otherwise, S2VT_E_ALIGN when a W is not 16-byte aligned); 0: per-step launches of the fused cell kernel;
 * -1: the one-launch form when the shape fits, else one s2vt_lstm_recurrence_fwd per direction (cut in two at cinit_t0, the first
 * part's last slot being the second part's slot 0: nothing is copied); 2: that pair of persistent recurrences, asked for by name
 * (S2VT_E_BADARG where s2vt_lstm_recurrence_fwd's persistent form does not serve the shape).  Every form gives the bits of two
 * s2vt_lstm_recurrence_fwd calls.  scratch: s2vt_lstm_birecurrence_scratch_bytes(H) bytes, 256-byte aligned. */
typedef struct s2vt_lstm_dir {
    const float* W; int32_t kw0; const float* b;      /* the cell's matrix [kw0 + H, 4H] (its recurrent rows start at kw0) and bias [4H] */
    const float* cinit; int64_t cinit_tstride; int32_t ldcinit; int32_t cinit_t0; int32_t cinit_steps;   /* carried partial; cinit NULL = none */
    float* C_hist; float* H_hist; float* gates;
} s2vt_lstm_dir;
size_t s2vt_lstm_birecurrence_scratch_bytes(int32_t H);
int s2vt_lstm_birecurrence_fwd(const s2vt_lstm_dir* fw, const s2vt_lstm_dir* bw, int32_t M, int32_t H, int32_t T, int32_t persistent,
                               void* scratch, size_t scratch_bytes, s2vt_stream stream);
/* ---- the bidirectional captioner (bidirection_tf_s2vt.py:48-216) as library calls on one caller-owned workspace.  LSTM1 is the pair of
 * recurrences above over T = Tv + Tc steps (frames, then zero padding; no DropoutWrapper, no word ever enters it); LSTM2 reads
 * [fw ; bw ; embed ; h2].  d: the usual dims (reserved = 0; label_dim unused).  Rows are time-major (row t * B + b).  lstm1_form: the
 * `persistent` argument of s2vt_lstm_birecurrence_fwd (-1: the library's choice).  Argument errors return S2VT_E_BADARG, the size functions 0;
 * both answer without a GPU.
 * s2vt_bidir_teacher_forced_fwd: build_model's logits (:113-156) for caption [B, Tc] -> logits_out [Tc * B, V]; keep = LSTM2's DropoutWrapper
 *   (Philox codes 512 + step, video_id / sample_id [B] needed when keep < 1); leaves in the workspace what the backward needs.
 * s2vt_bidir_bptt_bwd: given dlogits [Tc * B, V] (s2vt_softmax_nll_fwd_bwd's output) ADDS the fp32 gradient products of all eleven
 *   variables into `grads` (the caller zeroes them; Wemb's gradient is dense); same keep / seed / ids as the forward call on the same workspace.
 * s2vt_bidir_decode_greedy: build_generator's arithmetic (:187-215) for B videos -> ids_out [B, Tc] (and, optionally, logits_out
 *   [B, Tc, V]): LSTM1 and [fw ; bw] @ W2[:2H] once per video, LSTM2's Tv encode steps as one recurrence, then per decode step ONE fused cell
 *   launch that continues from the hoisted partial with the fed word's Wemb rows gathered as an operand, and the pick launch.
 *   unshifted_softmax != 0: the pick is argmax(exp(l) / sum exp(l)) as :211-212 write it (s2vt_softmax_unshifted_argmax), else argmax(l). */
typedef struct s2vt_bidir_params {
    float* Wemb;            /* [V, E] */
    float* encode_image_W;  /* [D, E] */
    float* encode_image_b;  /* [E] */
    float* lstm1_fw_W;      /* [E + H, 4H]  s2vt/LSTM1/bidirectional_rnn/fw/basic_lstm_cell/weights (name recalled from TF 1.1) */
    float* lstm1_fw_b;      /* [4H] */
    float* lstm1_bw_W;      /* [E + H, 4H]  .../bw/... */
    float* lstm1_bw_b;      /* [4H] */
    float* lstm2_W;         /* [2H + E + H, 4H] rows [fw ; bw ; embed ; h2] */
    float* lstm2_b;         /* [4H] */
    float* embed_word_W;    /* [H, V] */
    float* embed_word_b;    /* [V] */
} s2vt_bidir_params;
size_t s2vt_bidir_workspace_bytes(const s2vt_dims* d, int32_t B);
int s2vt_bidir_teacher_forced_fwd(const s2vt_dims* d, const s2vt_bidir_params* p, const float* video, int32_t B, const int32_t* caption, float keep,
                                  uint64_t seed, const int32_t* video_id, const int32_t* sample_id, int32_t lstm1_form, float* logits_out, void* workspace,
                                  size_t workspace_bytes, s2vt_stream stream);
int s2vt_bidir_bptt_bwd(const s2vt_dims* d, const s2vt_bidir_params* p, const s2vt_bidir_params* grads, const float* video, int32_t B,
                        const float* dlogits, float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id, void* workspace,
                        size_t workspace_bytes, s2vt_stream stream);
size_t s2vt_bidir_decode_workspace_bytes(const s2vt_dims* d, int32_t B);
int s2vt_bidir_decode_greedy(const s2vt_dims* d, const s2vt_bidir_params* p, const float* video, int32_t B, int32_t unshifted_softmax, int32_t video_base,
                             int32_t lstm1_form, int32_t* ids_out, float* logits_out, void* workspace, size_t workspace_bytes, s2vt_stream stream);
/* ---- the self-critical REINFORCE stage on that model (reinforcement_multisampling_tf_s2vt.py:227-339 applied to it).  No word enters LSTM1,
 * so both LSTM1 directions and [fw ; bw] @ W2[:2H] depend on the video only: the samples of a video share them.  Rows are SAMPLE-MAJOR (row
 * s * B + j is sample s of video j; the video of row n is n % B) and `video` is always the B distinct blocks [B, Tv, D], never tiled.  Same
 * conventions as above: caller-owned 256-byte-aligned workspace, S2VT_E_BADARG / S2VT_E_ALIGN / S2VT_E_WORKSPACE before any launch, size
 * functions 0 on bad shapes (S >= 1, K >= 0, K + with_greedy >= 1, S * B * T within int).
 * s2vt_bidir_sample: K multinomial captions per video -> sampled_out [K * B, Tc] and (with_greedy) the greedy one -> greedy_out [B, Tc], int32.
 *   LSTM1, the hoisted partial and LSTM2's Tv encode steps run on B rows; the Tc decode steps on R = (K + with_greedy) * B rows, each the fused
 *   cell launch of s2vt_bidir_decode_greedy continuing from the video's slice of the partial (row % B), then s2vt_vocab_pick: Gumbel-max over
 *   Philox counters (video_base + j, s, step), the greedy block last with sample id -1 (s2vt_sample's convention).  No dropout, <bos> = 1 fed at
 *   step 0, no host round trip.  K = 0 with greedy equals s2vt_bidir_decode_greedy(unshifted_softmax = 0).  A NULL output is legal where its
 *   block does not exist (sampled_out at K = 0, greedy_out without with_greedy).
 * s2vt_bidir_teacher_forced_fwd_rows: caption [S * B, Tc], video_id / sample_id [S * B] -> logits_out [Tc * S * B, V] (row t * N + n),
 *   bit-identical to s2vt_bidir_teacher_forced_fwd on the S-times tiled block: LSTM1 and its input products on B rows, the 2H-row part of
 *   LSTM2's partial on T * B rows and continued per row with the fed word's Wemb rows, LSTM2 / DropoutWrapper / vocabulary projection on S * B rows.
 * s2vt_bidir_bptt_bwd_rows: the backward of that call on the same workspace, ADDING into `grads` as s2vt_bidir_bptt_bwd does.  LSTM2's
 *   pre-activation gradients are summed over the samples of a video (ascending s, one owning thread per element, no atomics); lstm2_W's
 *   two H-row blocks, lstm2_b, the gradient into [fw ; bw] and all of LSTM1 / encode_image_* run on T * B (B) rows from that sum. */
size_t s2vt_bidir_sample_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t K, int32_t with_greedy);
int s2vt_bidir_sample(const s2vt_dims* d, const s2vt_bidir_params* p, const float* video, int32_t B, int32_t K, int32_t with_greedy, uint64_t seed,
                      int32_t video_base, int32_t lstm1_form, int32_t* sampled_out, int32_t* greedy_out, void* workspace, size_t workspace_bytes,
                      s2vt_stream stream);
/* ---- batched beam search on that model: the s2vt_beam_* family (above) for the bidirectional captioner, same conventions as the other
 * s2vt_bidir_* drivers (size function 0 on bad shapes; 1 <= beam <= 16).  No word enters LSTM1, so every hypothesis of a video shares both
 * LSTM1 directions and [fw ; bw] @ W2[:2H]; only the fused LSTM2 cell launch and the vocabulary product run on the R <= B * beam rows.
 * s2vt_bidir_beam_encode: exactly the once-per-video prefix of s2vt_bidir_sample -- LSTM1, the 2H-row partial of all T steps, LSTM2's Tv
 *   encode steps as one recurrence.  S2VT_E_CHAIN_TIMEOUT while a chain fault is pending.
 * s2vt_bidir_beam_step: s2vt_beam_step's semantics -- decode step t (0 <= t < Tc) for R live hypotheses; hypothesis m continues video
 *   video_of_row[m] from row parent[m] of step t - 1 (t = 0: the video's encoder state, parent ignored) with word[m] (<bos> = 1 at t = 0).
 *   The three int32 [R] arrays are device pointers; indices out of range are clamped, not reported.  A parent is clamped into
 *   [0, B * beam), the parity buffer's rows, not into step t - 1's R (which the call does not know): one at or past that R cannot fault,
 *   but it reads a row that an earlier step or nothing wrote, and the row's results mean nothing.  R == 0: S2VT_OK.  Steps are issued in
 *   order.  Writes top_ids / top_logp [R, k] (s2vt_vocab_topk of the step's logits; 1 <= k <= 16, k <= n_words) and, when logits_out is
 *   given, the logits [R, V].  Launches: one index kernel (the clamped [3][R] block into the workspace), ONE gathered-state cell launch (Wemb
 *   rows by word, h / c by parent, the partial of step Tv + t by video -- no gathered copy of state or partial), the vocabulary product
 *   on h', the top-k.  LSTM2's state lives in two parity buffers [B * beam, H] (c | h): step t writes parity t & 1 and reads the other, so
 *   issuing step t twice gives the same bits.
 * Workspace: s2vt_bidir_decode_workspace_bytes' encode part, then 4 * B * beam * H floats of state, B * beam * V of logits and 3 * B * beam
 * int32, each rounded up to 256 bytes. */
size_t s2vt_bidir_beam_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t beam);
int s2vt_bidir_beam_encode(const s2vt_dims* d, const s2vt_bidir_params* p, const float* video, int32_t B, int32_t beam, int32_t lstm1_form,
                           void* workspace, size_t workspace_bytes, s2vt_stream stream);
int s2vt_bidir_beam_step(const s2vt_dims* d, const s2vt_bidir_params* p, int32_t B, int32_t beam, int32_t t, int32_t R, const int32_t* video_of_row,
                         const int32_t* parent, const int32_t* word, int32_t k, int32_t* top_ids, float* top_logp, float* logits_out,
                         void* workspace, size_t workspace_bytes, s2vt_stream stream);
/* The sample sum on its own: out[(t * B + b) * C + c] = sum_s dz[((t * S + s) * B + b) * C + c], s ascending, no atomics (two runs give equal
 * bits).  C % 4 == 0 and 16-byte aligned pointers (S2VT_E_ALIGN): the kernel moves 16 bytes per lane. */
int s2vt_bidir_sample_sum(const float* dz, float* out, int32_t T, int32_t B, int32_t S, int32_t C, s2vt_stream stream);
size_t s2vt_bidir_rows_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t S);
int s2vt_bidir_teacher_forced_fwd_rows(const s2vt_dims* d, const s2vt_bidir_params* p, const float* video, int32_t B, int32_t S, const int32_t* caption,
                                       float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id, int32_t lstm1_form, float* logits_out,
                                       void* workspace, size_t workspace_bytes, s2vt_stream stream);
int s2vt_bidir_bptt_bwd_rows(const s2vt_dims* d, const s2vt_bidir_params* p, const s2vt_bidir_params* grads, const float* video, int32_t B, int32_t S,
                             const float* dlogits, float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id, void* workspace,
                             size_t workspace_bytes, s2vt_stream stream);
/* ---- back-propagation through that recurrence (tf.gradients through the unroll, reinforcement_multisampling_tf_s2vt.py:650):
 * for t = T-1 .. 0:  dh = dext_t (through the DropoutWrapper mask, Philox code drop_code0 + t; dext_t = dext + (t - dext_t0) *
 * dext_tstride, rows ld_ext apart, for t >= dext_t0; dext NULL = none) + dZ[t+1] @ W[kw0 : kw0 + H, :]^T;  dZ[t] ([T, M, 4H],
 * pre-activation gradients in the i | j | f | o column order) from dh, the carried cell gradient, gates[t] ([T, M, 4H]
 * activated, as s2vt_lstm_recurrence_fwd saved them) and C_hist ([T+1, M, H]).  persistent = 1: ONE launch -- workgroup
 * (unit group, gate) keeps its [H x 16] slice of the recurrent rows in LDS, dz crosses the chip as per-gate images in MFMA
 * operand order, the four gate partials of a unit group meet through a 4-workgroup exchange, the cell gradient stays in
 * registers (M <= 384, H % 4 == 0, H <= 1024, 4 * ceil(H / 16) <= the CU count; S2VT_E_BADARG otherwise; above 256 rows a
 * workgroup owns 32 units and half the row tiles); 0: per step one pointwise launch + split-K slabs of the product; -1:
 * persistent when the shape fits (M <= 384).  Results agree to
 * reduction order (gradients are order-free).  scratch: s2vt_lstm_recurrence_bwd_scratch_bytes(M, H)
 * bytes, 256-byte aligned. */
size_t s2vt_lstm_recurrence_bwd_scratch_bytes(int32_t M, int32_t H);
int s2vt_lstm_recurrence_bwd(const float* W, int32_t kw0, const float* gates, const float* C_hist, const float* dext, int64_t dext_tstride,
                             int32_t ld_ext, int32_t dext_t0, float* dZ, int32_t M, int32_t H, int32_t T, float keep, uint64_t seed,
                             const int32_t* video_id, const int32_t* sample_id, uint32_t drop_code0, int32_t persistent, void* scratch,
                             size_t scratch_bytes, s2vt_stream stream);
/* Where in the training workspace of (d, B, N) LSTM2's pre-activation gradients lie after LSTM2's phase of the backward (phase 0, 2
 * or 3): byte offset and length in floats of dZ2 [T][N][4H], T = n_video_lstm_step + n_caption_lstm_step, of which the steps the
 * forward call unrolled are written.  They come out of the backward recurrence alone (no atomics behind them): what a test of its
 * dispatch compares bit for bit. */
int s2vt_train_workspace_dz2(const s2vt_dims* d, int32_t B, int32_t N, size_t* offset, size_t* floats);
/* The same with dZ[t+1] @ W[kw0 : kw0 + H, :]^T on split-bf16 operands (x = hi + lo, hi = bf16(x), lo = bf16(x - hi); three bf16 MFMA
 * products per fp32 one, fp32 accumulators: 16 significant bits per operand) -- the recurrence s2vt_bptt_bwd_split runs for LSTM2
 * where its gradient products run split.  Same arguments and scratch.  Served by the register-weights form of the one-launch
 * recurrence only: persistent = 1, 256 < M <= 384, more than 8 column tiles of 16 units, W 16-byte aligned; S2VT_E_BADARG elsewhere.
 * The pointwise part, the dropout stream and the dZ history are fp32 as above. */
int s2vt_lstm_recurrence_bwd_split(const float* W, int32_t kw0, const float* gates, const float* C_hist, const float* dext, int64_t dext_tstride,
                                   int32_t ld_ext, int32_t dext_t0, float* dZ, int32_t M, int32_t H, int32_t T, float keep, uint64_t seed,
                                   const int32_t* video_id, const int32_t* sample_id, uint32_t drop_code0, int32_t persistent, void* scratch,
                                   size_t scratch_bytes, s2vt_stream stream);
/* Grid-wide waits of the persistent recurrence that gave up (bounded spins), over all launches of this process; 0 =
 * healthy.  Read after synchronising the stream. */
int s2vt_chain_timeouts(void);
/* The persistent recurrence needs all its workgroups resident at once.  The launcher checks the occupancy and never
 * overlaps two persistent grids of one process, but it cannot see another process on the same GPU: if a grid-wide wait
 * gives up, a fault is raised (host-visible counter + device-resident word) and stays raised until acknowledged:
 *   - s2vt_chain_fault(): 1 while a fault is pending (a host-memory read: no synchronisation, callable every step);
 *   - every entry point that launches a recurrence or updates variables returns S2VT_E_CHAIN_TIMEOUT while it is pending,
 *     and s2vt_adam_tf* launches already queued behind the faulting kernel skip their update on the device;
 *   - s2vt_chain_ack(disable): synchronises the device, clears the fault; disable != 0 turns the persistent form off for
 *     the rest of the process (the per-step launches give the same bits).  The caller then repeats the work since the
 *     last applied update. */
int s2vt_chain_fault(void);
int s2vt_chain_ack(int disable_persistent);
/* s2vt_chain_hold(1) ... s2vt_chain_hold(0) (nestable): while held, every recurrence whose form the library chooses takes its
 * per-step launches (same bits, ~5 % slower) instead of the persistent grid.  For callers that have OTHER kernels in flight on
 * the same GPU beside the library's stream -- an asynchronous RCCL all-reduce of a gradient slice (model.backward(overlap=True)):
 * a persistent grid needs every workgroup co-resident and must not be started while part of the chip is taken. */
int s2vt_chain_hold(int on);

/* In-place SUM all-reduce of the flat gradient bucket over an existing RCCL communicator (ncclComm_t as
 * void*), on `stream` -- the exchange step of SURVEY.md section 8(e) for C/C++ hosts (Python hosts use
 * torch.distributed).  The library never loads RCCL itself (a communicator belongs to the instance that made it):
 * it calls, in this order, the entry point registered with s2vt_set_rccl_allreduce, a `ncclAllReduce` visible in the
 * global symbol scope, or one from an already loaded librccl; S2VT_E_BADARG if there is none. */
int s2vt_allreduce_grads(float* bucket, int64_t n, void* rccl_comm, s2vt_stream stream);
/* Register the `ncclAllReduce` of the host's own RCCL (needed when it was loaded RTLD_LOCAL); NULL unregisters. */
int s2vt_set_rccl_allreduce(void* nccl_allreduce_fn_ptr);

/* ---- ROUGE-L reward on the device (csrc/rouge.hip; the arithmetic contract: DESIGN.md section 3) ----
 * The reward of the reference's rouge_* scripts (`from rouge_evaluation import *`: evaluate_captions_cider returns pycocoevalcap's
 * Rouge, beta = 1.2, one candidate against ALL references of its video) scored where the sampler's ids are born.
 * The reference corpus, uploaded once: every reference's token ids in one stream, the references sorted by video. */
typedef struct s2vt_rouge_refs {       /* all device pointers */
    const int32_t* tokens;             /* [ref_offsets[n_refs]] */
    const int32_t* ref_offsets;        /* [n_refs + 1] ascending */
    const int32_t* video_refs;         /* [n_videos + 1] ascending: video v owns references [video_refs[v], video_refs[v+1]), >= 1 each */
    int32_t n_videos, n_refs;
} s2vt_rouge_refs;
/* out[n] = float32(ROUGE-L F-measure) of row n = ids[n * ld .. n * ld + Tc) cut BEFORE its first eos_id (m ids; m = 0 scores 0)
 * against the references of video video_of_row[n]:
 *     l_j = LCS(candidate, r_j);  p = max_j double(l_j) / double(m);  r = max_j double(l_j) / double(len r_j)
 *     score = p == 0 || r == 0 ? 0 : ((1 + beta2) * p * r) / (r + beta2 * p)
 * every operation one IEEE double operation in this order, none fused: bit-equal to s2vt_rouge_score (s2vt_host.h).  pr_out
 * (may be NULL): [N][2] = p, r.  One launch, no workspace, no atomics; two runs give equal bits.  ld >= Tc (rows of a wider buffer
 * work), 1 <= Tc <= 128, any number of references per video, any reference length.  N == 0: S2VT_OK, nothing launched.
 * S2VT_E_BADARG (answered without a GPU): NULL pointers, ld < Tc, Tc outside [1, 128], N < 0, n_videos < 1, beta2 negative or not
 * finite.  A video_of_row[n] outside [0, n_videos) is device data the host cannot see: that row's out (and pr_out) is NaN, nothing
 * else is touched. */
int s2vt_rouge_l_score(const s2vt_rouge_refs* refs, const int32_t* ids, int32_t ld, int32_t N, int32_t Tc, int32_t eos_id,
                       const int32_t* video_of_row, double beta2, float* out, double* pr_out, s2vt_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* S2VT_H */
