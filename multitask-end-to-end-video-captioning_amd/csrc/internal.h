// internal.h -- launcher interfaces shared by the translation units of libs2vt_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_mfma.h"

namespace s2vt {

// forward contraction (exact ascending-k chain); epi in {EPI_STORE, EPI_LSTM, EPI_PICK}.
// cfg < 0: pick a tile configuration from the shape; >= 0 forces table entry `cfg` (tests, tuning).
hipError_t launch_gemm(const GemmArgs& a, int epi, int cfg, hipStream_t st);

// ---- in-library launch profiler (bench.py's roofline leg): when enabled, every contraction launch
// is bracketed by two hipEvents ON ITS OWN STREAM and tallied per (class, tile cfg) with its flops.
// class: 0 STORE, 1 LSTM, 2 PICK, 3 TN.  Collect only after the stream has been synchronised.
struct ProfRow { int cls, cfg; long launches; double ms, flops; const char* name; };
void prof_enable(bool on);
bool prof_on();
bool prof_wants(int cls, int cfg);          // profiler on and (cls, cfg) passes the filter
void prof_filter(int cls, int cfg);         // -1 = any
void prof_record(int cls, int cfg, const char* name, double flops, hipEvent_t e0, hipEvent_t e1);
hipError_t prof_events(hipEvent_t* e0, hipEvent_t* e1);
int prof_collect(ProfRow* rows, int max_rows);
int gemm_num_cfgs(int epi);
const char* gemm_cfg_name(int epi, int cfg);
// one entry of a tile table as launch_gemm sees it: rows x columns (per group) of the workgroup's tile, the entry that takes the launch when
// this one lacks the form asked for (-1: none), whether it has a scalar form and a live-row form (GemmArgs::omap / m_dev) of its own
struct GemmCfgInfo { const char* name; int BM, CG, fallback; bool has_scalar, has_live; };
bool gemm_cfg_info(int epi, int cfg, GemmCfgInfo* out);

// C[Kout, N] (+)= sum_m A[row(m), k] * B[m, n]   (weight gradients; order-free, fp32 MFMA)
struct TnArgs {
    const float* A; const int* rowidx; int lda;       // [Mred, Kout] (rows optionally gathered)
    const float* B; int ldb;                           // [Mred, N]
    float* C; int ldc;                                 // [Kout, N]
    int Mred, Kout, N;
    int accumulate;                                    // 1: C += result (fp32 atomics when split)
    float* colsum;                                     // optional [N]: += column sums of B (bias gradient), see launch_gemm_tn
    int gather_rows;                                   // rows of the table `rowidx` indexes (0 = not stated by the caller): the vector paths form
                                                       // rowidx * lda * 4 in 32 bits, so a table known to reach 2 GiB takes the scalar (64-bit) path
};
// colsum: when given, the column sums of B are ADDED to it -- inside the contraction on the vector path, by a colsum launch
// otherwise (so callers never launch one themselves).
hipError_t launch_gemm_tn(const TnArgs& a, hipStream_t st);

hipError_t launch_prep_caption(const int32_t* cap, int32_t* prev, int32_t* tgt, int N, int Tc, hipStream_t st);
hipError_t launch_caption_mask(const int32_t* ids, int N, int Tc, float* mask, int32_t* target_tm, float* mask_sum, float* mask_sum_copy, hipStream_t st);
hipError_t launch_xe_prep(const float* mask, const int32_t* cap, int N, int Tc, float loss_weight, float n_glob, int q1, float* coef_tm,
                          int32_t* target_tm, float* msum, hipStream_t st);
hipError_t launch_mixed_prep(const float* mask, const float* gmask, const float* rewards, const float* baseline, const int32_t* cap,
                             const int32_t* gcap, int Ns, int B, int Tc, float one_minus_lam, float lam, float loss_weight, int q1,
                             float smoothing, float n_glob_b, float* coef_tm, float* smooth_tm, int32_t* cap_all, int32_t* target_tm, float* sums, hipStream_t st);
hipError_t launch_mixed_loss(const float* coef, const float* nll, const int32_t* live_rows, int R, int N, int Ns, float* out3, hipStream_t st);
hipError_t launch_pg_coef(const float* mask, const float* rewards, const float* baseline, float scale, int N, int Tc, float* coef_tm,
                          hipStream_t st);
hipError_t launch_step_scalars(const float* coef, const float* nll, int64_t R, const float* msum_local, const float* gsum_global, float* loss,
                               float* gscale, float* sumsq, hipStream_t st);
hipError_t launch_softmax_nll(float* logits, int ld, int R, int V, const int32_t* target, const float* coef,
                              float smoothing, float* nll, float* lp_t, hipStream_t st, const float* smooth_rows = nullptr);
hipError_t launch_softmax_unshifted_argmax(const float* logits, int ld, int R, int V, int32_t* ids, float* probs, hipStream_t st);
hipError_t launch_lstm_bwd_pointwise(const float* gates, const float* c_new, const float* c_prev, const float* dh_rec,
                                     int nslab, size_t slab_stride, const float* dout_ext, int ld_ext, const float* dc_in,
                                     float* dc_out, float* dz, int M, int H, float keep, uint64_t seed, uint32_t drop_code,
                                     const int32_t* video_id, const int32_t* sample_id, hipStream_t st);
// out[t][n][u] = keep < 1 ? (h[t][n % B][u] / keep) * mask(n, t, u) : h[...]   (DropoutWrapper output of a cell whose
// state trajectory is shared by the rep = N / B sample rows of a video); code = code_base + t
hipError_t launch_expand_dropout(const float* h, float* out, int T, int B, int N, int H, float keep, uint64_t seed,
                                 uint32_t code_base, const int32_t* video_id, const int32_t* sample_id, hipStream_t st);
// dh[t][j][u] = sum_k (dout[t][k*B + j][u] / keep) * mask(k*B + j, t, u)   (adjoint of the above; dout rows ld_out apart)
// add != NULL: dout[t] + add[t - add_t0] for t >= add_t0 (add: [T - add_t0][N][H], rows H apart), same pass, same order
hipError_t launch_reduce_dropout(const float* dout, int ld_out, float* dh, int T, int B, int N, int H, float keep,
                                 uint64_t seed, uint32_t code_base, const int32_t* video_id, const int32_t* sample_id,
                                 hipStream_t st, const float* add = nullptr, int add_t0 = 0);
hipError_t launch_add_inplace(float* a, const float* b, size_t n, hipStream_t st);      // a[i] = b[i] + a[i]
hipError_t launch_colsum(const float* X, int ld, int M, int N, float* out, hipStream_t st);
hipError_t launch_sum_slabs(float* dst, const float* slabs, int nslab, size_t stride, size_t n, hipStream_t st);
// up to 8 buffers zeroed by one launch (sizes in 4-byte words)
struct ZeroList {
    uint32_t* p[8]; size_t n[8]; int count;
    ZeroList() : count(0) {}
    void add(void* ptr, size_t bytes) { if (ptr && bytes) { p[count] = static_cast<uint32_t*>(ptr); n[count] = bytes / 4; ++count; } }
};
hipError_t launch_zero_regions(const ZeroList& z, hipStream_t st);
// up to 4 device-to-device copies by one launch (16-byte aligned pointers, byte counts multiples of 16; anything else: false)
struct CopyList {
    uint4* dst[4]; const uint4* src[4]; size_t n16[4]; int count;
    CopyList() : count(0) {}
    bool add(void* d, const void* s, size_t bytes)
    {
        if (!bytes) return true;
        if (count >= 4 || ((reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(s) | bytes) & 15u)) return false;
        dst[count] = static_cast<uint4*>(d); src[count] = static_cast<const uint4*>(s); n16[count] = bytes / 16; ++count;
        return true;
    }
};
hipError_t launch_copy_regions(const CopyList& c, hipStream_t st);
hipError_t launch_gather_rows(const float* src, int ld, const int32_t* idx, int R, int C, float* dst, int ldd, hipStream_t st);   // dst[r,:] = src[idx[r],:]
hipError_t launch_scatter_rows(const float* src, int ld, const int32_t* idx, int R, int C, float* dst, int ldd, hipStream_t st);  // dst[idx[r],:] = src[r,:]
hipError_t launch_gather_i32(const int32_t* src, const int32_t* idx, int R, int32_t* dst, hipStream_t st);
hipError_t launch_scatter_add_rows(const float* dE, int ld, const int32_t* idx, int R, int E, float* dW, int ldw,
                                   hipStream_t st);
hipError_t launch_transpose(const float* in, int ldi, float* out, int ldo, int R, int Cc, hipStream_t st);
// ---- top-k score-weighted embedding feedback (topk_feed.hip; sum_generate_words_tf_s2vt.py:163-174)
constexpr int kTopkFeedMax = 8;                        // the largest k (the script's is 5)
// what the row's first thread writes beside the mix inside an unroll: generated[n][t] (emit[n] when given -- the generator's argmax of the
// probabilities -- else the first id), and, with a caption, loss_weight * mask[n][t] and the clamped target
struct TopkStep {
    const int32_t* caption; const float* mask; int N, Tc, t; float loss_weight;
    int32_t* generated; float* coef_tm; int32_t* target_tm; const int32_t* emit;
};
// ids / wts / S / x may be NULL together (the step's bookkeeping only); step may be NULL
hipError_t launch_topk_mix_fwd(const float* scores, int ld, int R, int V, int k, const float* Wemb, int E, int32_t* ids, float* wts, float* S,
                               float* x, int ldx, const TopkStep* step, hipStream_t st);
hipError_t launch_topk_mix_bwd(const float* dx, int lddx, const int32_t* ids, const float* wts, const float* S, const float* Wemb, int E,
                               const float* Wout, int V, int H, int k, int R, float* dscores, int lds, float* dO, int ldo, hipStream_t st);
hipError_t launch_scatter_add_rowsk(const float* dE, int ld, const int32_t* ids, const float* wts, int k, int R, int E, float* dW, int ldw,
                                    hipStream_t st);
hipError_t launch_grad_finalize(float* g, const float* theta, int64_t n, const float* gscale, float wd, float* sumsq,
                                hipStream_t st);
// fault: optional device word -- nonzero makes the launch a no-op (a persistent recurrence timed out upstream: the
// gradients are garbage); applied_step: optional device word that receives `step` when the update IS applied
hipError_t launch_adam_tf(float* theta, const float* g, float* m, float* v, int64_t n, const float* sumsq, float clip,
                          float lr_t, float b1, float b2, float eps, hipStream_t st, const unsigned* fault = nullptr,
                          int32_t* applied_step = nullptr, int32_t step = 0);
// theta -= lr * g * clip / max(sqrt(*sumsq), clip) (plain gradient descent behind the global-norm clip); fault / applied_step as above
hipError_t launch_sgd(float* theta, const float* g, int64_t n, const float* sumsq, float clip, float lr, hipStream_t st,
                      const unsigned* fault = nullptr, int32_t* applied_step = nullptr, int32_t step = 0);

// ---- a whole LSTM recurrence (T steps, M <= 64 rows) in one persistent launch (chain.hip)
struct ChainArgs {
    const float* W; int ldw; int kw0;                 // full cell matrix [*, 4H] (ldw floats per row); the recurrent rows start at kw0
    const float* bias;                                 // [4H]
    const float* cinit; long long cinit_tstride; int ldcinit; int cinit_steps;   // carried partial of step t < cinit_steps: cinit + t*tstride (signed: a caller may walk its partials backwards), rows ldcinit apart; NULL = none
    const float* h0; const float* c0;                  // initial state [M, H] or NULL = zeros
    float* C; float* Hh; size_t state_tstride;         // state histories: step t writes slot t + 1 (C + (t+1)*state_tstride)
    float* gates; size_t gates_tstride;                // optional activated gates [T][M][4H] (si | tj | sf | so)
    float* out; size_t out_tstride;                    // optional DropoutWrapper output [T][M][H]
    int M, H, T;
    float keep; uint32_t seed_lo, seed_hi, drop_code0; // dropout of `out`: code = drop_code0 + t
    const int32_t* video_id; const int32_t* sample_id;
    float* abuf;                                       // chain_scratch_floats(H) floats, 16-byte aligned
    unsigned* sync;                                    // kChainSyncBytes bytes: arrival counters + timeout word
    unsigned* status;                                  // (set by the launcher) host-mapped count of timed-out waits
    unsigned* fault;                                   // (set by the launcher) device-resident fault word: 1 after a timeout until chain_ack()
    unsigned spin_limit;                               // (set by the launcher) polls before a grid-wide wait gives up
    int ncg, tpp, img_tiles;                           // (set by the launcher) column groups, row tiles per row part, row tiles of one state image
    // optional (the register-weights form, 257-384 rows; ignored -- a dense launch, same results -- elsewhere): rows sorted by length.
    // perm[v] = row of every per-row array that virtual row v stands for (a permutation of 0 .. M-1), nlive[t] = virtual rows
    // 0 .. nlive[t]-1 are computed at step t (non-increasing in t); the other rows' histories are NOT written at that step
    const int32_t* perm; const int32_t* nlive;
};
bool chain_live_capable(int M, int H);                 // the forward AND backward recurrences of this shape take perm / nlive
hipError_t launch_row_order(const int32_t* live_rows, int n_live, int N, int Tv, int Tc, int32_t* perm, int32_t* nlive, hipStream_t st);
constexpr size_t kChainSyncBytes = 9 * 128;            // 8 counter shards + the status line, a block of its own (multiple of 16)
bool chain_eligible(int M, int H);                     // shape fits the persistent form on this device (and S2VT_CHAIN != 0)
size_t chain_scratch_floats(int H);
hipError_t launch_lstm_chain(const ChainArgs& a, hipStream_t st);
unsigned chain_timeouts();                             // grid-wide waits that gave up, all launches of this process (0 = healthy)
bool chain_operands_ok(const float* W, int ldw, const float* abuf);   // alignment the persistent form needs (else: per-step launches)
bool chain_fault();                                    // a timeout has happened and has not been acknowledged: results since are suspect
const unsigned* chain_fault_word();                    // device word of the current device (1 = fault), NULL when the persistent form is unavailable
hipError_t chain_ack(bool disable);                    // acknowledge (device idle!); disable: per-step launches for the rest of the process

// ---- gated overlap (train.hip, S2VT_OVERLAP=2): a side stream that is released once a persistent grid is RESIDENT.  A persistent recurrence at
// <= 256 rows holds one wave per SIMD at <= 380 VGPRs and spends half its time in hand-offs: an independent weight-gradient contraction can
// share the CUs with it -- provided the recurrence's workgroups got their slots first (a contraction that fills the chip first leaves no
// room for them: the grid would be partly resident and spin until the contraction drains).  The next persistent launch of the arming thread
// records g->ev behind its counter-zeroing kernel and, behind the grid's launch, queues on g->side {wait for g->ev; a one-wave kernel that
// polls the grid's first arrival until every workgroup has arrived, bounded}.  What the caller then launches on g->side starts beside the grid.
struct ChainGate { hipStream_t side; hipEvent_t ev; bool fired; };
void chain_gate_arm(ChainGate* g);                   // nullptr disarms; consumed (fired = true) by the next persistent launch of this thread
hipError_t chain_gate_zeroed(hipStream_t st);        // (launchers) behind the zeroing kernel
hipError_t chain_gate_launched(const unsigned* sync, unsigned arrivals);   // (launchers) behind the grid's launch; arrivals = workgroups arriving at the first hand-off

// ---- the backward recurrence of one cell in one persistent launch (chain.hip): dZ[t] for t = T-1 .. 0
struct BwdChainLaunch {
    const float* W; int ldw; int kw0;                  // cell matrix [*, 4H]; the recurrent rows start at kw0
    const float* gates; size_t gates_tstride;          // activated gates [T][M][4H]
    const float* C; size_t state_tstride;              // cell states [T+1][M][H]
    const float* dext; size_t dext_tstride; int ld_ext; int dext_t0;   // upstream gradient w.r.t. the (dropped) output of step t >= dext_t0; NULL = none
    float* dZ; size_t dz_tstride;                      // [T][M][4H]
    int M, H, T;
    float keep; uint32_t seed_lo, seed_hi, drop_code0;
    const int32_t* video_id; const int32_t* sample_id;
    float* img; float* ex; unsigned* sync;             // scratch, sizes from bwd_chain_scratch (16-byte aligned)
    const int32_t* perm; const int32_t* nlive;         // optional, as ChainArgs: step t runs virtual rows 0 .. nlive[t]-1 only (their dZ rows are the only ones written)
    bool split;                                        // dz @ Whh^T as three bf16 products on split operands (only where bwd_chain_split_serves)
};
bool bwd_chain_eligible(int M, int H);               // the shape fits the persistent form on this device
bool bwd_chain_split_serves(int M, int H);           // ... in its register-weights form (above 256 rows), which has split-bf16 kernels
bool bwd_chain_auto(int M, int H);                   // ... and it is the faster form there (chosen when the caller does not say)
void bwd_chain_scratch(int H, int M, size_t* img_floats, size_t* ex_floats, size_t* sync_bytes);
hipError_t launch_lstm_bwd_chain(const BwdChainLaunch& a, hipStream_t st);

// ---- the sampler's LSTM2 step at 257-384 rows on fragment-order operands (decode4.hip)
struct Dec4Geom { int eg, hg, ech, hch, erow, hgp, ngt, ncg, tpp, img_tiles; };
struct Dec4Launch {
    const float* wemb_p; const float* w2_p; const float* bias;
    const float* cinit; int ldcinit; int cinit_rowmod;
    const unsigned long long* tok; int tok_stride; int tok_const;
    const float* himg_in; float* himg_out;
    const float* c_prev; int cprev_rowmod;
    float* c_new; float* h_new;
    int R, H, E, V;
};
bool decode4_eligible(int R, int H, int E);
void decode4_geometry(int R, int H, int E, Dec4Geom* out);
hipError_t decode4_pack(const float* Wemb, const float* W2, int V, int H, int E, const Dec4Geom& q, float* wemb_p, float* w2_p, hipStream_t st);
hipError_t decode4_state_to_image(const float* h, int B, int R, int H, const Dec4Geom& q, float* img, hipStream_t st);
hipError_t launch_decode_lstm4(const Dec4Launch& a, const Dec4Geom& q, hipStream_t st);

// ---- the sampler's whole decode loop in one persistent launch (decode_loop.hip), on decode4's packed operands
struct DecLoopLaunch {
    const float* wemb_p; const float* w2_p; const float* bias2;
    const float* P2; size_t p2_tstride; int ldp2; int B;      // carried partial of decode step t (row % B)
    const float* c0;                                          // [B, H] cell state at the start of the decoding stage
    float* himg0; float* himg1;                               // state images (himg0 = h at the start, himg1 zeroed)
    unsigned long long* packed; int pick_stride;              // [Tc][R][pick_stride], zeroed
    const float* Wout; int ldwo; const float* bout;
    uint64_t seed; int video_base;                            // noise ids as sampler_rows_kernel: video = video_base + row % B, sample = row / B
    int noise_rows;                                           // rows [0, noise_rows) are sampled (sample id >= 0), the rest argmax
    int R, H, E, V, Tc;
    unsigned* sync;                                           // kChainSyncBytes
};
bool decode_loop_eligible(int R, int H, int E, int V);
hipError_t launch_decode_loop(const DecLoopLaunch& a, const Dec4Geom& q, hipStream_t st);

// ---- temporal attention step (attn.hip): score -> softmax -> context, one workgroup per batch row
struct AttnFwdArgs {
    const float* hWa;            // [B, H] query projection h_prev @ Wa, or NULL = zeros (the first decode step)
    const float* P;              // [Tv, B, H] hoisted image part V @ Ua + ba (original_attention.py:107)
    const float* Vt;             // [Tv, B, H] frame embeddings, time-major (:98)
    const float* w;              // [H]
    float* scores;               // optional [Tv, B]
    float* alpha;                // [Tv, B]
    float* asum;                 // optional [B]: alpha[0] + ... + alpha[min(8, Tv) - 1] (the regulariser's first-8-frames sum, :118,123)
    float* ctx;                  // [B, H]
    int Tv, B, H;
    int RC, ldT, vec;            // (set by the launcher) frames per LDS chunk, LDS row stride, 16-byte path
    // the row -> video form (beam search: the B rows are hypotheses that share their video's image block).  row_video == NULL:
    // row b reads block b of P / Vt, which hold B blocks per frame -- the form above, and the same kernel as before.  Else row b
    // reads block clamp(row_video[b], 0, n_video - 1) of P / Vt [Tv, n_video, H]; hWa, alpha, asum, ctx stay per row (stride B).
    const int32_t* row_video;    // [B] device, or NULL
    int n_video;
    // live rows (the early-exit sampler; needs row_video): workgroup i < *n_live is row live[i], the others return at once.  Both
    // device-resident, both NULL = every row.  Everything else is indexed by the row as above.
    const int32_t* live;         // [<= B] rows, each in [0, B)
    const int32_t* n_live;       // [1]
};
hipError_t launch_attn_fwd(const AttnFwdArgs& a, hipStream_t st);
struct AttnBwdArgs {
    const float* hWa; const float* P; const float* Vt; const float* w; const float* alpha;    // as the forward (hWa may be NULL = zeros)
    const float* dctx; int ld_dctx;                    // dense part of d(ctx) [B, ld] or NULL
    const float* slabs; int nslab; size_t slab_stride; int ld_slab;   // + sum_s slabs[s][b * ld_slab + col0 + h] (split-K slabs of a [B, ld_slab] product)
    int ctx_col0, emb_col0;                            // column of the ctx / embedding block inside a slab row
    const float* demb_dense; int ld_demb; float* demb_out;   // optional: demb_out[b, h] = demb_dense[b, h] + sum_s slabs[..emb_col0 + h]
    const float* reg_coef;                             // optional [B]: beta * mask[b, t] of the alpha regulariser (:123), with ...
    const float* asum; float reg_m;                    // ... the forward's first-8-frames sums [B] and the margin m
    float* dhWa;                                       // [B, H] (optional)
    float* dP; float* dVt; int acc;                    // [Tv, B, H]; acc != 0: += (accumulated over the decode steps)
    float* dw;                                         // [H], atomicAdd
    int Tv, B, H;
    int vec;                                           // (set by the launcher) 16-byte path
};
hipError_t launch_attn_bwd(const AttnBwdArgs& a, hipStream_t st);
// The shared-block backward (self-critical REINFORCE on the attention captioner): the a.B = n_video * samples rows are sample-major
// (row s * n_video + j is sample s of video j) and the samples of a video share its one block of P / Vt, so dP / dVt are
// [Tv, n_video, H] and take the SUM over the video's rows.  Two launches, no atomics on dP / dVt:
//   1. one workgroup per row: dctx (dense part + slabs), dalpha, the open-hinge term, de[Tv] -> de_rows / dctx_rows (and demb_out)
//   2. one workgroup per (video, 256-column slice): the video's rows in ascending s -- T = tanh(hWa[row] + P[t][video]) once, dhWa[row]
//      written, dP[t] / dVt[t] / dw summed in registers -- then ONE add into the video's block (every element has one owner; two runs
//      give equal bits there).  dw keeps its atomicAdd.
struct AttnBwdRowsArgs {
    AttnBwdArgs a;               // as above with B = rows; P / Vt / dP / dVt hold n_video blocks per frame
    int n_video, samples;
    float* de_rows;              // [rows][Tv] scratch
    float* dctx_rows;            // [rows][H] scratch: the assembled d(ctx); NULL = a.dctx is complete (no slabs) and is read in place
};
hipError_t launch_attn_bwd_rows(const AttnBwdRowsArgs& r, hipStream_t st);
hipError_t launch_attn_row_video(int32_t* row_video, int rows, int n_video, hipStream_t st);   // row_video[i] = i % n_video (sample-major rows)

// ---- vocabulary top-k with log-probabilities (beam.hip): ids / logp [R, k] of logits [R, V] (row stride ld), 1 <= k <= 16
hipError_t launch_vocab_topk(const float* logits, int ld, int R, int V, int k, int32_t* ids, float* logp, hipStream_t st);

// ---- the attention captioner's whole forward recurrence in one persistent launch (attn_chain.hip)
struct AttnChainLaunch {
    const float* W3; int ldw; const float* b3;          // LSTM3 [3H, 4H] (rows [0,H) context, [H,2H) embedding -- hoisted by the caller --, [2H,3H) h)
    const float* cinit; size_t cinit_tstride; int ldcinit;   // the hoisted embedding partial of step t (NULL = none)
    float* C; float* Hh; float* Out; size_t state_tstride;   // histories [T+1][B][H]: step t writes slot t + 1 (slot 0 = the zero state, not touched)
    float* gates; size_t gates_tstride;                 // [T][B][4H] (may alias cinit)
    const float* Wa; int ldwa; const float* P; const float* Vt; const float* w;
    float* hWa; size_t hwa_tstride;                     // [T][B][H], slots 1 .. T-1 written
    float* alpha; float* asum; float* ctx;              // [T][Tv][B], [T][B], [T][B][H]
    int B, H, T, Tv;
    float keep; uint32_t seed_lo, seed_hi, drop_code0; const int32_t* video_id; const int32_t* sample_id;
    float* img;                                         // attn_chain_scratch_floats(H) floats, 16-byte aligned
    unsigned* sync;                                     // kAttnChainSyncBytes
};
constexpr size_t kAttnChainSyncBytes = 3 * kChainSyncBytes;
bool attn_chain_eligible(int B, int H, int Tv);       // the persistent form serves this shape on this device (S2VT_ACHAIN != 0, no hold / fault)
size_t attn_chain_scratch_floats(int H);
hipError_t launch_attn_chain(const AttnChainLaunch& a, hipStream_t st);

// ---- ... and its backward recurrence (attn_chain_bwd.hip)
struct AttnBwdChainLaunch {
    const float* W3; int ldw; const float* Wa; int ldwa;
    const float* gates; size_t gates_tstride; const float* C; size_t state_tstride;      // forward histories
    float* dcat; size_t dcat_tstride; int ld_cat;           // d[out | ctx | emb] of the output layer, [T][B][3H]; Tv > 5: the ctx block comes back as the TOTAL d(ctx_t)
    float* deh;                                             // Tv > 5: [T][Tv][B] floats of scratch (d(score) per step, for the dP / dV accumulation behind the launch)
    float* dZ; size_t dz_tstride;                           // [T][B][4H]
    const float* hWa; size_t hwa_tstride; const float* P; const float* Vt; const float* w; const float* alpha;
    const float* reg_coef; const float* asum; float reg_m;  // alpha regulariser (reg_coef NULL = none)
    float* dhWa; size_t dhwa_tstride;                       // [T][B][H], slots >= 1 written
    float* dP; float* dVt; float* dw;                       // accumulated (zeroed / owned by the caller)
    int B, H, T, Tv;
    float keep; uint32_t seed_lo, seed_hi, drop_code0; const int32_t* video_id; const int32_t* sample_id;
    float* img; float* ex; float* dctxs; unsigned* sync;    // scratch, sizes from attn_bwd_chain_scratch (16-byte aligned)
};
bool attn_bwd_chain_eligible(int B, int H, int Tv);
void attn_bwd_chain_scratch(int H, size_t* img_floats, size_t* ex_floats, size_t* row_floats, size_t* sync_bytes);
hipError_t launch_attn_bwd_chain(const AttnBwdChainLaunch& a, hipStream_t st);

// ---- the opt-in bf16 mode of the S2VT backward's gradient contractions (bwd_bf16.hip): operands cast to bf16, fp32 accumulation
constexpr int kBf16K = 64;                            // K step of gemm_bf16_nt: a bf16 operand row holds bf16_pad(K) elements, zeros past K
__host__ __device__ inline int bf16_pad(int k) { return (k + kBf16K - 1) / kBf16K * kBf16K; }
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
// RNE, NaN kept (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t pack2(float a, float b)
{
    const f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

// split of two values: hi = bf16(x), lo = bf16(x - float(hi)), both RNE.  x - float(hi) is exact for finite x whose hi is
// finite, so hi + lo carries 16 significant bits.  NaN: hi and lo NaN.  +-Inf, and finite x beyond the largest bf16 (x rounds to
// +-Inf in hi): hi = +-Inf and lo = x - hi = NaN (Inf) / -+Inf (finite x) -- a product that takes such an element is NaN, where
// fp32 arithmetic would give +-Inf or NaN (Inf) or a finite value (finite x).
__device__ __forceinline__ void split2(float a, float b, uint32_t& hi, uint32_t& lo)
{
    hi = pack2(a, b);
    lo = pack2(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
}
// dst[r][k] = bf16(src[row(r)][k]) (row(r) = rowidx ? rowidx[r] : r) for k < K, zeros up to bf16_pad(K); dst 16-byte aligned, ldd % 8 == 0
// dst_lo (optional): the split form -- dst = bf16(x) (hi), dst_lo = bf16(x - hi) (lo), same ldd
// ones: rows bf16_pad(K + 1) wide with column K = 1 -- the operand A of launch_gemm_bf16x3_tn with a bias row
// width (0 = bf16_pad(K + ones); a multiple of 8, >= K + ones): the columns written per row, zeros past K -- a row placed inside a wider one
hipError_t launch_cast_rows_bf16(const float* src, int ld, const int32_t* rowidx, int R, int K, uint16_t* dst, int ldd, hipStream_t st,
                                 uint16_t* dst_lo = nullptr, int ones = 0, int width = 0);
// dst[c][r] = bf16(src[row(r)][c]) for r < R, zeros for R <= r < Rp (Rp a multiple of 64; dst 16-byte aligned, ldd % 8 == 0).
// rdst (optional): the row form as well, rdst[r][c] for c < bf16_pad(C) (8-byte aligned, rldd % 4 == 0).
// colsum (optional): += the column sums of the fp32 input rows (fixed order, no atomics), through part[cast_tr_part_floats(Rp, C)].
struct CastTrArgs {
    const float* src; int ld; const int32_t* rowidx; int R, C;
    uint16_t* dst; int ldd; int Rp;
    float* colsum; float* part;
    uint16_t* rdst; int rldd;
    uint16_t* dst_lo; uint16_t* rdst_lo;             // (optional) the split form: dst / rdst take hi = bf16(x), these lo = bf16(x - hi)
};
hipError_t launch_cast_tr_bf16(const CastTrArgs& a, hipStream_t st);
size_t cast_tr_part_floats(int Rp, int C);
// C[M,N] (+)= A[M,Kp] B[N,Kp]^T, bf16 operands (rows 16-byte aligned, lda / ldb % 8 == 0, Kp % 64 == 0), fp32 accumulation, no atomics.
// mfma: 16 (v_mfma_f32_16x16x32_bf16), 32 (v_mfma_f32_32x32x16_bf16), 0 = the library's choice
hipError_t launch_gemm_bf16_nt(const uint16_t* A, int lda, const uint16_t* B, int ldb, float* C, int ldc, int M, int N, int Kp, int accumulate,
                               int mfma, hipStream_t st);
// C[M,N] (+)= Ah Bh^T + Ah Bl^T + Al Bh^T: split-bf16 operands (hi / lo planes with the layout rules of launch_gemm_bf16_nt), fp32
// accumulation, no atomics.  part: optional split-K scratch of part_floats floats (gemm_bf16x3_part_floats(M, N, Kp) for the full
// split; fewer -> no split); cls: the launch profiler's class (2 the sampler's pick screen, 3 weight gradients, 4 data gradients).
// tile: 0 = 128 x 128 workgroup tiles, 1 = 192 x 96 (launches without a scratch only: with one, 128 x 128 whatever tile says) -- the same
// bits either way.  gemm_bf16x3_nt_tile_choice: 1 where ceil(tiles / cus) x the tile's area is smaller with 192 x 96 (host only);
// gemm_bf16x3_pick_tile: what the pick screen's product takes -- that rule on this device's CUs, or the env S2VT_PICK_TILE (read once: 0 or 1)
hipError_t launch_gemm_bf16x3_nt(const uint16_t* Ah, const uint16_t* Al, int lda, const uint16_t* Bh, const uint16_t* Bl, int ldb, float* C, int ldc,
                                 int M, int N, int Kp, int accumulate, float* part, size_t part_floats, int cls, hipStream_t st, int tile = 0);
int gemm_bf16x3_nt_tile_choice(int M, int N, int cus);
// C[M,N] (+)= Ah Bh^T: the one-product form on the hi planes alone (same layout rules), 192 x 96 workgroup tiles, never split.  bf16 x bf16
// in fp32 -- |C - A B^T| up to 2^-7 of sum |a_k b_k|: the pick screen's product (its margin covers that), not a gradient's
hipError_t launch_gemm_bf16x1_nt(const uint16_t* Ah, int lda, const uint16_t* Bh, int ldb, float* C, int ldc, int M, int N, int Kp, int accumulate, int cls,
                                 hipStream_t st);
int gemm_bf16x3_pick_tile(int M, int N);
size_t gemm_bf16x3_part_floats(int M, int N, int Kp);
// The K-major form: C[M,N] (+)= sum_k A[k][m] B[k][n] over K rows of planes stored by rows ([K][lda], [K][ldb]; lda, ldb % 8 == 0, 16-byte
// aligned; rows >= K are never read, columns up to the next multiple of 128 may be -- they lie inside the planes or read zeros).  The
// same K steps and MFMA order as the NT form: equal bits on transposed planes.  bias (optional): A's column M holds ones (lda > M),
// and bias[n] += the product's row M, the column sums of B; the split-K scratch then counts M + 1 rows.
bool gemm_bf16x3_tn_ok(int lda, int ldb, int K);     // the planes' byte offsets fit the loader's 32 bits
hipError_t launch_gemm_bf16x3_tn(const uint16_t* Ah, const uint16_t* Al, int lda, const uint16_t* Bh, const uint16_t* Bl, int ldb, float* C, int ldc,
                                 int M, int N, int K, int accumulate, float* bias, float* part, size_t part_floats, int cls, hipStream_t st);
// The forward form: C[M,N] (+)= sum_k A[m][k] B[k][n] -- A by rows as in the NT form ([M][lda], lda >= bf16_pad(K); its columns in
// [K, bf16_pad(K)) ARE read and must be finite: cast_rows_bf16 leaves zeros, or the ones column, there), B K-major as in the TN form
// ([K][ldb], a weight as it lies in memory cast by rows; k rows >= K are never read; gemm_bf16x3_tn_ok(ldb, ldb, K) must hold).  The same
// K steps and MFMA order again: equal bits with NT / TN on explicitly transposed planes.  cbias (optional, accumulate == 0 only): fp32 [N],
// C = product + cbias[col].  cls 0: the forward's class of the launch profiler.
hipError_t launch_gemm_bf16x3_nn(const uint16_t* Ah, const uint16_t* Al, int lda, const uint16_t* Bh, const uint16_t* Bl, int ldb, float* C, int ldc,
                                 int M, int N, int K, int accumulate, const float* cbias, float* part, size_t part_floats, int cls, hipStream_t st);
// the split softmax (aux.hip): as launch_softmax_nll, but dlogits leaves as hi / lo planes [R][ldp] (ldp >= bf16_pad(V), pad columns zero)
// and the logits stay; false: the shape is not the register kernel's (V % 4, V > 12288, alignment) -- nothing launched
bool softmax_nll_split_ok(const float* logits, int ld, int V, const uint16_t* hi, const uint16_t* lo, int ldp);
hipError_t launch_softmax_nll_split(const float* logits, int ld, int R, int V, const int32_t* target, const float* coef, float smoothing, float* nll,
                                    float* lp_t, uint16_t* hi, uint16_t* lo, int ldp, hipStream_t st, const float* smooth_rows = nullptr);

// ---- the sampler's screened vocabulary pick (pick_screen.hip): bf16 approximate logits screen the columns of a row, the survivors
// get the exact fp32 chain and Gumbel expression -- the packed picks are those of launch_gemm(EPI_PICK), bit for bit.  The screen's product
// is bf16(h) bf16(W) (one product; the margin takes what the two casts miss, measured) unless the env asks for the three-product split form
// (margin constant C = 2^-10): S2VT_PICK_PRODUCTS=3, or any explicit S2VT_PICK_TILE (a tile of the three-product kernel) -- read once
int pick_screen_products();                           // 1 or 3
constexpr int kPickScreenMaxH = 2048;                 // the resolve kernel stages h and a column of W in LDS
constexpr size_t kPickScreenHeadBytes = 256;          // counters + nwmax: the scratch's first block, zeroed by ..._prepare
struct PickScreenWs {
    unsigned long long* counters;                     // [0] survivors summed over rows and steps; then uint32 most survivors of a row, uint32 rows that took every column
    float* nwmax;                                     // [0] max_v |W[:, v]|_2, [1] max_v |W[:, v] - bf16(W[:, v])|_2, rounded up (bytes 16, 20 of the head block)
    uint16_t *Wh, *Wl;                                // hi / lo planes of embed_word_W^T [V][Hp] (one product: Wl stays unwritten)
    float* Wt;                                        // embed_word_W^T in fp32 [V][ldt], zeros past H: a survivor's column as one row
    uint16_t *hh, *hl;                                // hi / lo planes of the step's rows [R][Hp] (one product: hl stays unwritten)
    float* L;                                         // approximate logits [R][ldl]; above 12288 columns the resolve kernel leaves its fast keys there
    int Hp, ldl, ldt;                                 // bf16_pad(H); V rounded up to 4; H rounded up to 4
};
// once per sampler call: zero the head block, cast W^T, transpose W, take the column norms' maximum
hipError_t launch_pick_screen_prepare(const float* W, int H, int V, const PickScreenWs& s, hipStream_t st);
// one decode step's pick on R rows h[R][H]: cast, product (profiler class 2), resolve; pick zeroed beforehand, as for EPI_PICK
hipError_t launch_pick_screen_step(const float* h, int ldh, const float* W, const float* bias, int R, int H, int V, const int32_t* vid,
                                   const int32_t* sid, uint64_t seed, int step, unsigned long long* pick, int pick_stride, const PickScreenWs& s,
                                   hipStream_t st);

// order-free NN contraction for the backward data path with optional split-K slabs:
// slab s (blockIdx.y) holds the partial over its K range at C + s * slab_stride.
struct NnBwdArgs {
    const float* A; int lda;        // [M, K]
    const float* W; int ldw;        // [K, N]
    float* C; int ldc;              // [M, N] (x splits)
    int M, N, K;
    int splits; size_t slab_stride;
};
hipError_t launch_gemm_nn_bwd(const NnBwdArgs& a, hipStream_t st);

}  // namespace s2vt
