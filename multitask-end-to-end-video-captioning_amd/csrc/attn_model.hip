// attn_model.hip -- the temporal-attention captioner of original_attention.py as whole-model entry points:
// build_model's unroll with saved activations (:88-150), back-propagation through it (the train_op of train(), :436-441),
// and the greedy sampler of build_generator / build_sampler (:155-251).  All loops run inside the library; the caller
// passes device pointers and one workspace.
//
// Per decode step the recurrence is  query -> score/softmax/context -> LSTM3:
//     hWa_t  = out_{t-1} @ Wa                              (out = the DropoutWrapper output: `h_prev = output1`, :135)
//     a_t, ctx_t = attention(hWa_t, P, V)                  (attn.hip: one launch)
//     z_t    = emb_t @ W3[H:2H]  ->  h_{t-1} @ W3[2H:3H]  ->  ctx_t @ W3[0:H]   (+ b3;  ONE ascending-k chain, blocks in
//              order of availability -- the numeric contract)
// and everything that does not feed the recurrence is batched over all steps: the embedding rows of W3 (hoisted, one
// product for all steps: the chain's first block), the output layer tanh([emb ; ctx ; out] @ Wp + bp) and the vocabulary
// logits after the loop, every weight gradient and the [out | ctx | emb] data gradient of the output layer in the
// backward.  Forward activations are bit-identical to oracle/s2vt_oracle.py::attention_forward; gradients are order-free.
//
// Self-critical REINFORCE (s2vt_attn_sample, s2vt_attn_teacher_forced_fwd_rows, s2vt_attn_bptt_bwd_rows): N = samples * B sample-major rows
// (row s * B + j = sample s of video j) share the B image blocks -- one prologue, the attention step in its row -> video form, the
// shared-block attention backward of attn.hip, the image-side gradient products on Tv * B rows.  Scope: these forms run the PER-STEP
// launches; the persistent recurrences (attn_chain*.hip: one image block per row, B <= 64) are not used by them and are unchanged -- at
// the working shape N = 320 they would not be eligible anyway.
//
// In this file: the decode step of the three samplers (greedy, multinomial, beam) is ONE function, decode_step on a DecodeStep (its
// attention half, attn_attend, also serves the teacher-forced unroll), so the ascending-k chains of LSTM3 and of the output layer are
// stated once.  The backward is a driver (attn_bptt_bwd_impl: validate and carve, decide `persistent` and `gated`) over the stages of
// the per-call context AttnBwd, in this order: vocab, output_layer_grads (at once, or beside the persistent recurrence), dcat,
// recurrence_persistent | recurrence_steps, lstm3_and_query_grads, image_side -- with one exit: once the gate has been armed or the
// side stream forked, every path passes the join, a failed launch's included.  The image blocks (encidx, Vt, P) are an AttnImg in
// each of the three workspaces.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include <mutex>

#include "api_util.h"
#include "detmath.h"

using namespace s2vt_api;

namespace {

constexpr int kXSlabs = 8;        // most split-K slabs of the per-step product dz @ W3^T  ([B, 3H], K = 4H)
constexpr int kQSlabs = 4;        // ... of dhWa @ Wa^T ([B, H], K = H)
constexpr uint32_t kDropCode3 = 768u;   // dropout stream of LSTM3: code = 768 + decode step (layer 3 * 256)

__global__ void attn_enc_index_kernel(int32_t* idx, int B, int Tv)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * Tv) return;
    const int t = i / B, j = i % B;
    idx[i] = j * Tv + t;     // row of video[B*Tv, d] feeding time-major row (frame t, video j)   (the transpose of :98)
}

__global__ void attn_rows_kernel(int32_t* vid, int32_t* sid, int B, int video_base)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    vid[i] = video_base + i;
    sid[i] = -1;             // greedy: argmax of the logits, no noise
}

__global__ void attn_unpack_ids_kernel(const unsigned long long* packed, int32_t* ids, int R, int T, int stride)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R * T) return;
    const int m = i / T, t = i % T;
    ids[i] = (int32_t)(~(uint32_t)packed[((size_t)t * R + m) * stride]);
}

__global__ __launch_bounds__(256) void attn_tanh_bwd_kernel(float* dy, const float* y, size_t n4)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 d = reinterpret_cast<float4*>(dy)[i];
    const float4 v = reinterpret_cast<const float4*>(y)[i];
    d.x *= 1.f - v.x * v.x; d.y *= 1.f - v.y * v.y; d.z *= 1.f - v.z * v.z; d.w *= 1.f - v.w * v.w;
    reinterpret_cast<float4*>(dy)[i] = d;
}

// BasicLSTMCell backward of one decode step of LSTM3.  The gradient w.r.t. the step's DROPPED output has two sources -- the
// output layer (dcat's first H columns) and the next step's attention query (split-K slabs of dhWa @ Wa^T) -- and goes back
// through the DropoutWrapper mask; the gradient w.r.t. the clean h comes from the next step's recurrent rows (the last H
// columns of the slabs of dz @ W3^T).
struct AttnCellBwdArgs {
    const float* gates; const float* c_new; const float* c_prev;
    const float* dcat; int ld_cat;                         // [B, 3H]: columns [0, H) = d(out)
    const float* dqs; int nq; size_t q_stride;             // slabs [nq][B][H] or NULL
    const float* dxs; int nx; size_t x_stride; int ld_x; int x_col0;   // slabs [nx][B][3H], recurrent block at x_col0, or NULL
    const float* dc_in; float* dc_out; float* dz;
    int M, H;
    float keep; uint32_t seed_lo, seed_hi, drop_code;
    const int32_t* video_id; const int32_t* sample_id;
};

__global__ __launch_bounds__(256) void attn_cell_bwd_kernel(const AttnCellBwdArgs a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.M * a.H) return;
    const int H = a.H, m = i / H, u = i % H;
    float dout = a.dcat[(size_t)m * a.ld_cat + u];
    if (a.dqs)
        for (int s = 0; s < a.nq; ++s) dout += a.dqs[(size_t)s * a.q_stride + i];
    if (a.keep < 1.0f)
        dout = (dout / a.keep) * dropout_keep01(a.seed_lo, a.seed_hi, (uint32_t)a.video_id[m], (uint32_t)a.sample_id[m], a.drop_code,
                                               (uint32_t)u, a.keep);
    float dh = dout;
    if (a.dxs)
        for (int s = 0; s < a.nx; ++s) dh += a.dxs[(size_t)s * a.x_stride + (size_t)m * a.ld_x + a.x_col0 + u];
    const float* g = a.gates + (size_t)m * 4 * H + u;
    const float si = g[0], tj = g[H], sf = g[2 * H], so = g[3 * H];
    const float tc = dm_tanhf(a.c_new[i]);
    const float cp = a.c_prev[i];
    float dc = dh * so * (1.f - tc * tc);
    if (a.dc_in) dc += a.dc_in[i];
    float* z = a.dz + (size_t)m * 4 * H + u;
    z[0] = dc * tj * si * (1.f - si);
    z[H] = dc * si * (1.f - tj * tj);
    z[2 * H] = dc * cp * sf * (1.f - sf);
    z[3 * H] = dh * tc * so * (1.f - so);
    a.dc_out[i] = dc * sf;
}

// loss = (sum coef * nll + sum reg_coef * max(0, m - asum)) / sum(mask)  (original_attention.py:144-149), 1 / the global sum(mask)
// for the gradient bucket, a zeroed ||g||^2 accumulator: one workgroup, deterministic.
__global__ __launch_bounds__(256) void attn_step_scalars_kernel(const float* coef, const float* nll, const float* reg_coef, const float* asum,
                                                                float reg_m, int R, const float* msum_local, const float* gsum_global,
                                                                float* loss, float* gscale, float* sumsq)
{
    __shared__ double sh[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < R; i += 256) {
        s += (double)coef[i] * (double)nll[i];
        if (reg_coef) {
            const float hinge = reg_m - asum[i];
            if (hinge > 0.f) s += (double)(reg_coef[i] * hinge);
        }
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (loss) *loss = (float)(sh[0] / (double)*msum_local);
        if (gscale) *gscale = 1.0f / *gsum_global;
        if (sumsq) *sumsq = 0.f;
    }
}

// caption [B, Tc] / mask [B, Tc] (row-major, as fed) -> what the loss kernels take, time-major: target_tm[t*B + b], coef_tm[t*B + b] =
// mask[b, t], reg_tm = beta * mask (optional), *mask_sum = sum(mask): ONE launch of one workgroup (deterministic sum) instead of
// four tensor-library kernels per step.
__global__ __launch_bounds__(256) void attn_loss_inputs_kernel(const int32_t* cap, const float* mask, int B, int Tc, float beta, int32_t* target_tm,
                                                               float* coef_tm, float* reg_tm, float* mask_sum)
{
    __shared__ double sh[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < B * Tc; i += 256) {
        const int t = i / B, b = i % B;
        const float m = mask[b * Tc + t];
        target_tm[i] = cap[b * Tc + t];
        coef_tm[i] = m;
        if (reg_tm) reg_tm[i] = beta * m;
        s += (double)m;
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *mask_sum = (float)sh[0];
}

// The image blocks of a call's videos: what attn_prologue makes and every attention launch reads.  Each workspace carves the three
// regions where it always did (they are not adjacent).
struct AttnImg {
    int32_t* encidx;               // [Tv*B] the row of video[B*Tv, d] feeding time-major row (frame t, video b)
    float *Vt, *P;                 // [Tv*B, H] frame embeddings (time-major) and the hoisted image part
};

// Saved activations + backward scratch, carved from the caller's buffer.  Everything is time-major ([step][row]), so a
// truncated unroll (caption_steps < Tc) is the leading part of the full one's layout.
struct AttnWs {
    AttnImg img;
    int32_t *prev, *tgt, *vid, *sid;
    float *hWa, *alpha, *asum, *ctx;   // [Tc][B][H], [Tc][Tv][B], [Tc][B], [Tc][B][H]
    float *G3, *C3, *H3, *O3;      // gates [Tc][B][4H] (first the hoisted partial); states / dropped outputs [(Tc+1)][B][H], slot t+1 = step t
    float* Y;                      // [Tc*B, H] output layer
    float *dY, *dcat, *dZ3, *dxs, *dqs, *dc, *dhWa, *dEmb, *dPt, *dVtt, *dEv;
    float* bslab; size_t bslab_floats;    // split-K slabs of the batched data-gradient products
    unsigned long long* packed;    // greedy picks [Tc][B][kPickStride]
    float* aimg; unsigned* async_; // persistent forward recurrence (attn_chain.hip): fragment images, hand-off counters
    float *bimg, *bex, *brow_; unsigned* bsync;   // persistent backward recurrence (attn_chain_bwd.hip)
    float* deh;                                   // ... its d(score) history [Tc][Tv][B] (more than 5 frames: dP / dV are accumulated behind the launch)
    int32_t* rowvid; float* dctxr;                // the shared-block form only: row -> video [rows], the assembled d(ctx) of one step [rows][H]
};

// n_video > 0: the shared-block form -- B rows (sample-major) over n_video image blocks: the image arrays (encidx, Vt, P and their gradients)
// count n_video blocks per frame, everything else B rows, and rowvid / dctxr follow at the end.  n_video = 0: one block per row, the
// layout as it always was.
size_t carve_attn(Carver& c, const s2vt_dims* d, int B, AttnWs* out, int n_video = 0)
{
    const size_t H = d->lstm_dim, V = d->n_words, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step, b = B, nv = n_video > 0 ? n_video : B;
    AttnWs w;
    w.img.encidx = c.take<int32_t>(Tv * nv); w.prev = c.take<int32_t>(Tc * b); w.tgt = c.take<int32_t>(Tc * b);
    w.vid = c.take<int32_t>(b); w.sid = c.take<int32_t>(b);
    w.img.Vt = c.take<float>(Tv * nv * H); w.img.P = c.take<float>(Tv * nv * H);
    w.hWa = c.take<float>(Tc * b * H); w.alpha = c.take<float>(Tc * Tv * b); w.asum = c.take<float>(Tc * b); w.ctx = c.take<float>(Tc * b * H);
    w.G3 = c.take<float>(Tc * b * 4 * H); w.C3 = c.take<float>((Tc + 1) * b * H); w.H3 = c.take<float>((Tc + 1) * b * H);
    w.O3 = c.take<float>((Tc + 1) * b * H);
    w.Y = c.take<float>(Tc * b * H);
    w.dY = c.take<float>(Tc * b * H); w.dcat = c.take<float>(Tc * b * 3 * H); w.dZ3 = c.take<float>(Tc * b * 4 * H);
    w.dxs = c.take<float>((size_t)kXSlabs * b * 3 * H); w.dqs = c.take<float>((size_t)kQSlabs * b * H); w.dc = c.take<float>(b * H);
    w.dhWa = c.take<float>(Tc * b * H); w.dEmb = c.take<float>(Tc * b * H);
    w.dPt = c.take<float>(Tv * nv * H); w.dVtt = c.take<float>(Tv * nv * H); w.dEv = c.take<float>(Tv * nv * H);
    w.deh = c.take<float>(Tc * Tv * b);
    {
        // dY = dlogits @ Wout^T ([Tc B, H], K = |V|) and dcat = dpre @ Wp^T ([Tc B, 3H], K = H) when they are short of tiles
        size_t need = 0;
        for (size_t tc = 1; tc <= Tc; ++tc) {
            const int s1 = dx_splits((int)(tc * b), (int)H, (int)V), s2 = dx_splits((int)(tc * b), (int)(3 * H), (int)H);
            const size_t n1 = s1 > 1 ? (size_t)s1 * tc * b * H : 0, n2 = s2 > 1 ? (size_t)s2 * tc * b * 3 * H : 0;
            if (n1 > need) need = n1;
            if (n2 > need) need = n2;
        }
        w.bslab = need ? c.take<float>(need) : nullptr;
        w.bslab_floats = need;
    }
    w.packed = c.take<unsigned long long>(Tc * b * kPickStride);
    w.aimg = c.take<float>(attn_chain_scratch_floats((int)H)); w.async_ = c.take<unsigned>(kAttnChainSyncBytes / 4);
    {
        size_t imgf, exf, rowf, syncb;
        attn_bwd_chain_scratch((int)H, &imgf, &exf, &rowf, &syncb);
        w.bimg = c.take<float>(imgf); w.bex = c.take<float>(exf); w.brow_ = c.take<float>(rowf); w.bsync = c.take<unsigned>(syncb / 4);
    }
    w.rowvid = nullptr; w.dctxr = nullptr;
    if (n_video > 0) { w.rowvid = c.take<int32_t>(b); w.dctxr = c.take<float>(b * H); }
    if (out) *out = w;
    return c.off;
}

bool attn_dims_ok(const s2vt_dims* d)
{
    return d && d->dim_image > 0 && d->n_words > 0 && d->lstm_dim > 0 && d->n_video_lstm_step > 0 && d->n_video_lstm_step <= 64 &&
           d->n_caption_lstm_step > 0 && d->reserved == 0;      // (no model bit is implemented here: refused, never ignored)
}

bool attn_params_ok(const s2vt_attn_params* p)
{
    return p && p->Wemb && p->encode_image_W && p->encode_image_b && p->embed_att_w && p->embed_att_Wa && p->embed_att_Ua &&
           p->embed_att_ba && p->embed_word_W && p->embed_word_b && p->embed_nn_Wp && p->embed_nn_bp && p->lstm3_W && p->lstm3_b;
}

// frame embedding to H dims in time-major rows (frame t, video b) (:95-98) and the hoisted image part V @ Ua + ba (:107)
int attn_prologue(const s2vt_dims* d, const s2vt_attn_params* p, const float* video, int B, const AttnImg& w, hipStream_t st)
{
    const int H = d->lstm_dim, D = d->dim_image, Tv = d->n_video_lstm_step;
    hipLaunchKernelGGL(attn_enc_index_kernel, dim3((B * Tv + 255) / 256), dim3(256), 0, st, w.encidx, B, Tv);
    HIP_TRY(hipGetLastError());
    ASeg sv = make_seg(video, D, D, 0, 0, w.encidx);
    HIP_TRY(store_call(&sv, 1, p->encode_image_W, H, p->encode_image_b, w.Vt, H, Tv * B, H, 0, -1, st));
    ASeg sp = make_seg(w.Vt, H, H, 0);
    HIP_TRY(store_call(&sp, 1, p->embed_att_Ua, H, p->embed_att_ba, w.P, H, Tv * B, H, 0, -1, st));
    return S2VT_OK;
}

// (inside a step or a stage: hand a failed launch's error to the driver, whose HIP_TRY records it)
#define HIP_CHECK(expr) do { const hipError_t _e = (expr); if (_e != hipSuccess) return _e; } while (0)

// One decode step on M rows: what the greedy loop, the multinomial sampler and the beam step differ in is data, not code -- where a
// row's state lives, how its word and its parent's h are gathered, which image block it reads, and the early-exit mode's row list and
// tiles.  The teacher-forced unroll uses the first half (attn_attend) with its own query.
struct DecodeStep {
    const s2vt_attn_params* p; AttnImg img;
    int t, M, H, Tv;
    const float *c_prev, *h_prev; float *c_new, *h_new;     // LSTM3 state [M][H]: slots t / t + 1 of a history, or ping-pong
    const int32_t* h_rows;                                  // h_prev is gathered through it (beam: the clamped parent), or NULL = row m
    const unsigned long long* word_key; const int32_t* word_idx;   // the word fed at t > 0: the packed picks of step t-1 (stride kPickStride), or clamped words (beam)
    float *hWa, *alpha, *asum, *ctx, *Y;                    // the step's [M][H], [Tv][M], [M] (or NULL), [M][H], [M][H]
    const int32_t* row_video; int n_video;                  // the row -> video form: the M rows share n_video image blocks (NULL, 0: one per row)
    const int32_t *live, *n_live; int store_cfg, lstm_cfg;  // early-exit mode: every launch covers rows live[0 .. *n_live) only (device-resident); its tile knobs (-1: the cost model's)
};

// query -> score / softmax / context (:113-128): hWa = query @ Wa, then ONE attention launch
hipError_t attn_attend(const DecodeStep& s, const float* query, hipStream_t st)
{
    const int H = s.H;
    if (s.t > 0) {     // (step 0: the query is the zero state, h_prev @ Wa = 0, :102)
        ASeg sq = make_seg(query, H, H, 0, 0, s.h_rows);
        HIP_CHECK(store_call(&sq, 1, s.p->embed_att_Wa, H, nullptr, s.hWa, H, s.M, H, 0, s.store_cfg, st, nullptr, 0, false, s.live, s.n_live));
    }
    AttnFwdArgs a;
    std::memset(&a, 0, sizeof(a));
    a.hWa = s.t > 0 ? s.hWa : nullptr; a.P = s.img.P; a.Vt = s.img.Vt; a.w = s.p->embed_att_w;
    a.alpha = s.alpha; a.asum = s.asum; a.ctx = s.ctx;
    a.Tv = s.Tv; a.B = s.M; a.H = H;
    a.row_video = s.row_video; a.n_video = s.n_video;
    a.live = s.live; a.n_live = s.n_live;
    return launch_attn_fwd(a, st);
}

// The decode step of the samplers (build_generator / build_sampler, :155-251; no dropout -- self.lstm3, not lstm3_dropout, :188,:235 --
// so the query is the clean h): attention, then LSTM3 as ONE ascending-k chain over the word's embedding rows, h_prev, the context
// (blocks in order of availability), then the output layer tanh([embed ; atten ; h_new] @ Wp + bp) in the order
// [2H:3H], [H:2H], [0:H].  Step 0 has no word (current_embed = 0, :169) and starts from the zero state, so both chains are shorter.
hipError_t decode_step(const DecodeStep& s, hipStream_t st)
{
    const s2vt_attn_params* p = s.p;
    const int H = s.H, ks = s.word_key ? kPickStride : 1;
    const NoiseIds none{nullptr, nullptr, 0};
    const int z = s.t == 0;      // step 0: LSTM3's chain is the context block alone, the output layer's has no word block
    HIP_CHECK(attn_attend(s, s.h_prev, st));
    ASeg s3[3] = {make_seg(p->Wemb, H, H, H, 0, s.word_idx, s.word_key, ks), make_seg(s.h_prev, H, H, 2 * H, 0, s.h_rows), make_seg(s.ctx, H, H, 0)};
    HIP_CHECK(lstm_call(s3 + 2 * z, 3 - 2 * z, p->lstm3_W, p->lstm3_b, s.c_prev, 0, s.c_new, s.h_new, nullptr, nullptr, s.M, H, 1.0f, none, 0, s.lstm_cfg, st,
                        nullptr, 0, 0, s.live, s.n_live));
    ASeg sy[3] = {make_seg(p->Wemb, H, H, 2 * H, 0, s.word_idx, s.word_key, ks), make_seg(s.ctx, H, H, H), make_seg(s.h_new, H, H, 0)};
    return store_call(sy + z, 3 - z, p->embed_nn_Wp, H, p->embed_nn_bp, s.Y, H, s.M, H, 1, s.store_cfg, st, nullptr, 0, false, s.live, s.n_live);
}

// alphas [steps][Tv][rows] out of the workspace
hipError_t copy_alphas_out(float* dst, const float* src, size_t bytes, hipStream_t st)
{
    CopyList cl;
    if (cl.add(dst, src, bytes)) return launch_copy_regions(cl, st);
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st);
}


// ---- batched beam search (final_beam_search.py:201-294 over the decode step of original_attention.py:155-251) ----------------
// Beam step, stage 1: what the R live hypotheses continue from.  The parent's LSTM3 cell state is copied into dense rows (the cell
// kernel reads c_prev by row number); its h is NOT copied -- the query projection and the cell's recurrent segment gather it through
// the clamped parent index (ASeg::rowidx), as the word's embedding rows are gathered through the clamped word.  Step 0 starts from
// the zero state (:164-165).  Indices are device data the host does not see here: out-of-range values are clamped into range
// (nothing is read outside the workspace or the embedding table), as beam_gather_kernel (beam.hip) clamps.
__global__ __launch_bounds__(256) void attn_beam_gather_kernel(const int32_t* parent, const int32_t* word, int t, int Rmax, int H, int V,
                                                               const float* c_prev, float* c_out, int32_t* par_out, int32_t* word_out)
{
    const int m = blockIdx.x;
    int par = 0;
    if (t > 0) {
        par = parent[m];
        par = par < 0 ? 0 : (par >= Rmax ? Rmax - 1 : par);
    }
    const float* cs = c_prev + (size_t)par * H;
    for (int i = threadIdx.x; i < H; i += 256) c_out[(size_t)m * H + i] = t > 0 ? cs[i] : 0.f;
    if (threadIdx.x == 0) {
        const int wd = word[m];
        par_out[m] = par;
        word_out[m] = wd < 0 ? 0 : (wd >= V ? V - 1 : wd);
    }
}

constexpr int kBeamTopkMax = 16;

struct AttnBeamWs {
    AttnImg img;                       // of the B videos (s2vt_attn_beam_encode)
    float *c[2], *h[2];                // LSTM3 state [Rmax][H]: step t writes slot t & 1 and reads the other (rows are permuted between steps)
    float* cg;                         // the parents' cell state, gathered [Rmax][H]
    int32_t *par, *word;               // clamped parent rows / words [Rmax]
    float *hWa, *alpha, *ctx, *Y;      // [Rmax][H], [Tv][Rmax], [Rmax][H], [Rmax][H]
    float* logits;                     // [Rmax][V] (when the caller does not ask for them)
};

size_t carve_attn_beam(Carver& c, const s2vt_dims* d, int B, int beam, AttnBeamWs* out)
{
    const size_t H = d->lstm_dim, V = d->n_words, Tv = d->n_video_lstm_step, b = B, Rmax = (size_t)B * beam;
    AttnBeamWs w;
    w.img.encidx = c.take<int32_t>(Tv * b);
    w.img.Vt = c.take<float>(Tv * b * H); w.img.P = c.take<float>(Tv * b * H);
    for (int i = 0; i < 2; ++i) { w.c[i] = c.take<float>(Rmax * H); w.h[i] = c.take<float>(Rmax * H); }
    w.cg = c.take<float>(Rmax * H);
    w.par = c.take<int32_t>(Rmax); w.word = c.take<int32_t>(Rmax);
    w.hWa = c.take<float>(Rmax * H); w.alpha = c.take<float>(Tv * Rmax); w.ctx = c.take<float>(Rmax * H); w.Y = c.take<float>(Rmax * H);
    w.logits = c.take<float>(Rmax * V);
    if (out) *out = w;
    return c.off;
}

// The multinomial sampler's workspace: the image blocks of the B videos and one step's worth of per-row state for R = (K + greedy) B rows.
struct AttnSampleWs {
    AttnImg img;                       // of the B videos
    int32_t *vid, *sid, *rowvid;
    float *c[2], *h[2];                // LSTM3 state [R][H]: step t reads slot t & 1 and writes the other
    float *hWa, *alpha, *ctx, *Y;      // [R][H], [Tv][R], [R][H], [R][H]
    unsigned long long* packed;        // picks [Tc][R][kPickStride]
    int32_t* live[2];                  // stop-at-<eos> mode: the rows still sampling at the current / previous step (ascending) [R] ...
    int32_t* nlive;                    // ... and their count per step [Tc], device-resident
};

size_t carve_attn_sample(Carver& c, const s2vt_dims* d, int B, int R, AttnSampleWs* out)
{
    const size_t H = d->lstm_dim, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step, b = B, r = R;
    AttnSampleWs w;
    w.img.encidx = c.take<int32_t>(Tv * b); w.vid = c.take<int32_t>(r); w.sid = c.take<int32_t>(r); w.rowvid = c.take<int32_t>(r);
    w.img.Vt = c.take<float>(Tv * b * H); w.img.P = c.take<float>(Tv * b * H);
    for (int i = 0; i < 2; ++i) { w.c[i] = c.take<float>(r * H); w.h[i] = c.take<float>(r * H); }
    w.hWa = c.take<float>(r * H); w.alpha = c.take<float>(Tv * r); w.ctx = c.take<float>(r * H); w.Y = c.take<float>(r * H);
    w.packed = c.take<unsigned long long>(Tc * r * kPickStride);
    for (int i = 0; i < 2; ++i) w.live[i] = c.take<int32_t>(r);        // (at the end: the regions above lie where they always did)
    w.nlive = c.take<int32_t>(Tc);
    if (out) *out = w;
    return c.off;
}

// rows = n_video * samples of the shared-block forms (the sampler, the _rows unroll and its backward)
bool attn_rows_shape_ok(const s2vt_dims* d, int n_video, int samples)
{
    return attn_dims_ok(d) && n_video > 0 && samples > 0 && (int64_t)n_video * samples <= INT_MAX / 64 / d->n_caption_lstm_step;
}

// noise ids of the sampler's rows (sample-major): video = video_base + row % B, sample = row / B for the K multinomial blocks, -1
// (argmax, no noise) for the greedy block behind them; and the row -> video map of the attention step
__global__ void attn_sample_rows_kernel(int32_t* vid, int32_t* sid, int32_t* rowvid, int R, int B, int K, int video_base)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R) return;
    vid[i] = video_base + i % B;
    sid[i] = i / B < K ? i / B : -1;
    rowvid[i] = i % B;
}

// ids[m][t] for rows m0 .. m0 + n - 1 of the R packed rows.  A word that was never written (stop-at-<eos> mode: the row had left the
// loop; a pick always leaves a non-zero word) reads as <eos> = 0.
__global__ void attn_unpack_rows_kernel(const unsigned long long* packed, int32_t* ids, int R, int m0, int n, int T, int stride)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * T) return;
    const int m = i / T, t = i % T;
    const unsigned long long w = packed[((size_t)t * R + m0 + m) * stride];
    ids[i] = w ? (int32_t)(~(uint32_t)w) : 0;
}

bool attn_beam_shape_ok(const s2vt_dims* d, int B, int beam)
{
    return attn_dims_ok(d) && B > 0 && beam >= 1 && beam <= kBeamTopkMax && (int64_t)B * beam <= INT_MAX / 4;
}

// ---- the teacher-forced unroll and its backward: what both check alike, in the ABI's order (bad argument, alignment, workspace), and
// the carve.  ptrs_ok: the call's own pointers; own_rc: the one check each makes of its own, which comes before the workspace's size
int attn_unroll_open(const s2vt_dims* d, bool ptrs_ok, int B, int caption_steps, float keep, const int32_t* video_id, const int32_t* sample_id,
                     void* workspace, size_t workspace_bytes, int n_video, int own_rc, AttnWs* w)
{
    if (!attn_dims_ok(d) || !ptrs_ok || !workspace || B <= 0) return S2VT_E_BADARG;
    if (!(keep > 0.0f) || (keep < 1.0f && (!video_id || !sample_id))) return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    if (caption_steps < 1 || caption_steps > d->n_caption_lstm_step) return S2VT_E_BADARG;
    if (own_rc != S2VT_OK) return own_rc;
    Carver c(workspace, workspace_bytes);
    carve_attn(c, d, B, w, n_video);
    return c.ok() ? S2VT_OK : S2VT_E_WORKSPACE;
}

// the persistent recurrences (attn_chain*.hip) load W3 and Wa 16 bytes at a time
bool attn_chain_weights_ok(const s2vt_attn_params* p)
{
    return !chain_fault() && !(reinterpret_cast<uintptr_t>(p->lstm3_W) & 15) && !(reinterpret_cast<uintptr_t>(p->embed_att_Wa) & 15);
}

// the whole forward recurrence -- query projection, score / softmax / context, LSTM3, all Tc steps -- as ONE persistent launch
AttnChainLaunch attn_fwd_chain_args(const s2vt_attn_params* p, const AttnWs& w, int B, int H, int Tc, int Tv, float keep, const NoiseIds& ids)
{
    const size_t BH = (size_t)B * H;
    AttnChainLaunch a;
    std::memset(&a, 0, sizeof(a));
    a.W3 = p->lstm3_W; a.ldw = 4 * H; a.b3 = p->lstm3_b;
    a.cinit = w.G3; a.cinit_tstride = (size_t)4 * BH; a.ldcinit = 4 * H;
    a.C = w.C3; a.Hh = w.H3; a.Out = w.O3; a.state_tstride = BH; a.gates = w.G3; a.gates_tstride = (size_t)4 * BH;
    a.Wa = p->embed_att_Wa; a.ldwa = H; a.P = w.img.P; a.Vt = w.img.Vt; a.w = p->embed_att_w;
    a.hWa = w.hWa; a.hwa_tstride = BH; a.alpha = w.alpha; a.asum = w.asum; a.ctx = w.ctx;
    a.B = B; a.H = H; a.T = Tc; a.Tv = Tv;
    a.keep = keep; a.seed_lo = (uint32_t)ids.seed; a.seed_hi = (uint32_t)(ids.seed >> 32); a.drop_code0 = kDropCode3;
    a.video_id = ids.video_id; a.sample_id = ids.sample_id;
    a.img = w.aimg; a.sync = w.async_;
    return a;
}

// A weight gradient C[M, N] += A[rows, M]^T B[rows, N] (+ colsum += B's column sums); idx: A's rows gathered out of a table of gather_rows
// rows (0 = not stated)
TnArgs tn(const float* A, const int32_t* idx, int gather_rows, int lda, const float* B, int ldb, float* C, int ldc, int rows, int M, int N, float* colsum = nullptr)
{
    return TnArgs{A, idx, lda, B, ldb, C, ldc, rows, M, N, 1, colsum, gather_rows};
}

// One backward call of the attention captioner: what every stage reads (filled once by attn_bptt_bwd_impl, which is the driver) and the
// stages themselves, each straight-line, in the driver's order.  n_video > 0 is the shared-block form: B sample-major rows over n_video
// image blocks, per-step launches, the attention backward of launch_attn_bwd_rows (dP / dVt one block per video, summed over its rows),
// the image-side products on Tv * n_video rows.
struct AttnBwd {
    SideStream& ss;
    int H, V, D, Tv, Tc, B, n_video;     // (Tc: the steps the forward call unrolled)
    int NV, R, R1; size_t BH;            // image blocks per frame; rows of the all-step products: every step | the steps that have a word
    AttnWs w;
    const s2vt_attn_params *p, *grads; const float *video, *dlogits, *reg_coef; float reg_m, keep; uint64_t seed; const int32_t *video_id, *sample_id;
    hipStream_t st; bool persistent, gated;   // the recurrence as one launch; the weight gradients that feed nothing in it beside it (side stream)
    bool side_used = false;              // the gate has been armed or the side stream forked: the driver owes the join

    TnArgs dwout() const { return tn(w.Y, nullptr, 0, H, dlogits, V, grads->embed_word_W, V, R, H, V, grads->embed_word_b); }

    // ---- vocabulary projection: dWout, dbout (at once, or deferred: on the side stream behind the gate) and d(output layer), back
    // through its tanh
    hipError_t vocab() const
    {
        if (!gated) HIP_CHECK(launch_gemm_tn(dwout(), st));
        HIP_CHECK(nn_bwd_slabs(dlogits, V, p->embed_word_W, V, w.dY, H, R, H, V, w.bslab, st, w.bslab_floats));
        hipLaunchKernelGGL(attn_tanh_bwd_kernel, dim3((unsigned)(((size_t)R * H / 4 + 255) / 256)), dim3(256), 0, st, w.dY, w.Y, (size_t)R * H / 4);
        return hipGetLastError();
    }
    // ---- output layer: Wp rows [output1 ; atten ; current_embed] and its bias (either stream, as dWout) ...
    hipError_t output_layer_grads(hipStream_t s) const
    {
        HIP_CHECK(launch_gemm_tn(tn(w.O3 + BH, nullptr, 0, H, w.dY, H, grads->embed_nn_Wp, H, R, H, H, grads->embed_nn_bp), s));
        HIP_CHECK(launch_gemm_tn(tn(w.ctx, nullptr, 0, H, w.dY, H, grads->embed_nn_Wp + (size_t)H * H, H, R, H, H), s));
        return Tc > 1 ? launch_gemm_tn(tn(p->Wemb, w.prev + B, V, H, w.dY + BH, H, grads->embed_nn_Wp + (size_t)2 * H * H, H, R1, H, H), s) : hipSuccess;
    }
    // ... and d[out | ctx | emb] for every step at once; the image-side accumulators of the recurrence start from zero
    hipError_t dcat() const
    {
        HIP_CHECK(nn_bwd_slabs(w.dY, H, p->embed_nn_Wp, H, w.dcat, 3 * H, R, 3 * H, H, w.bslab, st, w.bslab_floats));
        ZeroList z;
        z.add(w.dPt, (size_t)Tv * NV * H * 4); z.add(w.dVtt, (size_t)Tv * NV * H * 4);
        return launch_zero_regions(z, st);
    }

    // ---- the recurrence, back through time, as ONE persistent launch: cell backward, dz @ [W3 h rows ; W3 context rows]^T, attention
    // backward, dhWa @ Wa^T, all Tc steps
    hipError_t recurrence_persistent()
    {
        AttnBwdChainLaunch a;
        std::memset(&a, 0, sizeof(a));
        a.W3 = p->lstm3_W; a.ldw = 4 * H; a.Wa = p->embed_att_Wa; a.ldwa = H;
        a.gates = w.G3; a.gates_tstride = (size_t)4 * BH; a.C = w.C3; a.state_tstride = BH;
        a.dcat = w.dcat; a.dcat_tstride = (size_t)3 * BH; a.ld_cat = 3 * H; a.dZ = w.dZ3; a.dz_tstride = (size_t)4 * BH;
        a.hWa = w.hWa; a.hwa_tstride = BH; a.P = w.img.P; a.Vt = w.img.Vt; a.w = p->embed_att_w; a.alpha = w.alpha;
        a.reg_coef = reg_coef; a.asum = w.asum; a.reg_m = reg_m;
        a.dhWa = w.dhWa; a.dhwa_tstride = BH; a.dP = w.dPt; a.dVt = w.dVtt; a.dw = grads->embed_att_w;
        a.deh = w.deh;
        a.B = B; a.H = H; a.T = Tc; a.Tv = Tv;
        a.keep = keep; a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.drop_code0 = kDropCode3;
        a.video_id = video_id; a.sample_id = sample_id;
        a.img = w.bimg; a.ex = w.bex; a.dctxs = w.brow_; a.sync = w.bsync;
        ChainGate gate{ss.s, ss.ev[3], false};
        if (gated) { chain_gate_arm(&gate); side_used = true; }
        const hipError_t re = launch_attn_bwd_chain(a, st);
        chain_gate_arm(nullptr);
        HIP_CHECK(re);
        if (gated) {
            // (reads: dlogits, Y, dY, O3, ctx, Wemb -- final since before the launch; writes: the gradients of embed_word_W/b and embed_nn_Wp/bp,
            //  which nothing else in this call touches.  A gate that did not fire -- a zero-step launch -- puts the side stream behind the caller's)
            if (!gate.fired) HIP_CHECK(fork_to(st, ss.s, ss.ev[3]));
            HIP_CHECK(launch_gemm_tn(dwout(), ss.s));
            HIP_CHECK(output_layer_grads(ss.s));
        }
        // the embedding block of dz @ W3^T does not feed the recurrence: all steps >= 1 at once, on top of the output layer's block
        if (Tc > 1) {
            ASeg sz = make_seg(w.dZ3 + 4 * BH, 4 * H, 4 * H, 0);
            HIP_CHECK(store_call(&sz, 1, p->lstm3_W + (size_t)H * 4 * H, 4 * H, nullptr, w.dEmb + BH, H, R1, H, 0, -1, st, w.dcat + 3 * BH + 2 * H, 3 * H, true));
        }
        return hipSuccess;
    }

    // ---- the recurrence in per-step launches.  Split-K plan of a per-step data-gradient product (order-free): what nn_bwd makes of
    // the slabs asked of it over a reduction of K
    static int slabs_made(int asked, int K)
    {
        const int kper = ((K + asked - 1) / asked + BK - 1) / BK * BK;
        return (K + kper - 1) / kper;
    }
    hipError_t recurrence_steps() const
    {
        // enough slabs for >= ~512 workgroups
        int sx = (512 + ((3 * H + 63) / 64) - 1) / ((3 * H + 63) / 64) / ((B + 63) / 64);
        sx = sx < 1 ? 1 : (sx > kXSlabs ? kXSlabs : sx);
        int sq = kQSlabs;
        while (sq > 1 && H / sq < 128) --sq;
        const int nx = slabs_made(sx, 4 * H), nq = slabs_made(sq, H);
        for (int t = Tc - 1; t >= 0; --t) {
            const bool last = t == Tc - 1;
            AttnCellBwdArgs a;      // BasicLSTMCell backward of step t -> dz
            std::memset(&a, 0, sizeof(a));
            a.gates = w.G3 + (size_t)t * 4 * BH; a.c_new = w.C3 + (t + 1) * BH; a.c_prev = w.C3 + t * BH;
            a.dcat = w.dcat + (size_t)t * 3 * BH; a.ld_cat = 3 * H;
            a.dqs = last ? nullptr : w.dqs; a.nq = nq; a.q_stride = BH;
            a.dxs = last ? nullptr : w.dxs; a.nx = nx; a.x_stride = 3 * BH; a.ld_x = 3 * H; a.x_col0 = 2 * H;
            a.dc_in = last ? nullptr : w.dc; a.dc_out = w.dc; a.dz = w.dZ3 + (size_t)t * 4 * BH;
            a.M = B; a.H = H; a.keep = keep; a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.drop_code = kDropCode3 + (uint32_t)t;
            a.video_id = video_id; a.sample_id = sample_id;
            hipLaunchKernelGGL(attn_cell_bwd_kernel, dim3((B * H + 255) / 256), dim3(256), 0, st, a);
            HIP_CHECK(hipGetLastError());
            // d[ctx | emb | h_prev] = dz @ W3^T as split-K slabs: the attention backward sums the ctx and emb blocks, the next
            // (earlier) step's cell backward the h block
            HIP_CHECK(nn_bwd(w.dZ3 + (size_t)t * 4 * BH, 4 * H, p->lstm3_W, 4 * H, w.dxs, 3 * H, B, 3 * H, 4 * H, sx, 3 * BH, st, sx > 1 ? kSlabTileCfg : -1));
            AttnBwdArgs g;
            std::memset(&g, 0, sizeof(g));
            g.hWa = t > 0 ? w.hWa + t * BH : nullptr; g.P = w.img.P; g.Vt = w.img.Vt; g.w = p->embed_att_w; g.alpha = w.alpha + (size_t)t * Tv * B;
            g.dctx = w.dcat + (size_t)t * 3 * BH + H; g.ld_dctx = 3 * H;
            g.slabs = w.dxs; g.nslab = nx; g.slab_stride = 3 * BH; g.ld_slab = 3 * H; g.ctx_col0 = 0; g.emb_col0 = H;
            if (t > 0) { g.demb_dense = w.dcat + (size_t)t * 3 * BH + 2 * H; g.ld_demb = 3 * H; g.demb_out = w.dEmb + t * BH; }
            if (reg_coef) { g.reg_coef = reg_coef + (size_t)t * B; g.asum = w.asum + (size_t)t * B; g.reg_m = reg_m; }
            g.dhWa = t > 0 ? w.dhWa + t * BH : nullptr; g.dP = w.dPt; g.dVt = w.dVtt; g.acc = 1; g.dw = grads->embed_att_w;
            g.Tv = Tv; g.B = B; g.H = H;
            AttnBwdRowsArgs r;      // (the shared-block form: the rows of a video are summed into its one block)
            std::memset(&r, 0, sizeof(r));
            r.a = g; r.n_video = n_video; r.samples = n_video > 0 ? B / n_video : 0; r.de_rows = w.deh; r.dctx_rows = w.dctxr;
            HIP_CHECK(n_video > 0 ? launch_attn_bwd_rows(r, st) : launch_attn_bwd(g, st));
            // gradient w.r.t. the previous step's dropped output through this step's query: dhWa @ Wa^T (slabs, summed by the cell backward)
            if (t > 0) HIP_CHECK(nn_bwd(w.dhWa + t * BH, H, p->embed_att_Wa, H, w.dqs, H, B, H, H, sq, BH, st, sq > 1 ? kSlabTileCfg : -1));
        }
        return hipSuccess;
    }

    // ---- weight gradients of the recurrence, one contraction over all unrolled steps per block: W3 rows [0, H) atten (+ b3), [2H, 3H)
    // h_prev, [H, 2H) current_embed; Wa (the query of step t = the out of step t-1); the embedding rows (tf.nn.embedding_lookup, :141-142)
    hipError_t lstm3_and_query_grads() const
    {
        HIP_CHECK(launch_gemm_tn(tn(w.ctx, nullptr, 0, H, w.dZ3, 4 * H, grads->lstm3_W, 4 * H, R, H, 4 * H, grads->lstm3_b), st));
        HIP_CHECK(launch_gemm_tn(tn(w.H3, nullptr, 0, H, w.dZ3, 4 * H, grads->lstm3_W + (size_t)2 * H * 4 * H, 4 * H, R, H, 4 * H), st));
        if (Tc > 1) {
            HIP_CHECK(launch_gemm_tn(tn(p->Wemb, w.prev + B, V, H, w.dZ3 + 4 * BH, 4 * H, grads->lstm3_W + (size_t)H * 4 * H, 4 * H, R1, H, 4 * H), st));
            HIP_CHECK(launch_gemm_tn(tn(w.O3 + BH, nullptr, 0, H, w.dhWa + BH, H, grads->embed_att_Wa, H, R1, H, H), st));
            HIP_CHECK(launch_scatter_add_rows(w.dEmb + BH, H, w.prev + B, R1, H, grads->Wemb, H, st));
        }
        return hipSuccess;
    }
    // ---- image part P = V @ Ua + ba and the frame embedding V = video @ encode_image_W + b
    hipError_t image_side() const
    {
        HIP_CHECK(launch_gemm_tn(tn(w.img.Vt, nullptr, 0, H, w.dPt, H, grads->embed_att_Ua, H, Tv * NV, H, H, grads->embed_att_ba), st));
        ASeg sp = make_seg(w.dPt, H, H, 0);
        HIP_CHECK(store_call(&sp, 1, p->embed_att_Ua, H, nullptr, w.dEv, H, Tv * NV, H, 0, -1, st, w.dVtt, H, true));     // dV = dV(ctx path) + dP @ Ua^T
        return launch_gemm_tn(tn(video, w.img.encidx, Tv * NV, D, w.dEv, H, grads->encode_image_W, H, Tv * NV, D, H, grads->encode_image_b), st);
    }

    // every stage, in order, up to the first that fails
    hipError_t stages()
    {
        HIP_CHECK(vocab());
        if (!gated) HIP_CHECK(output_layer_grads(st));
        HIP_CHECK(dcat());
        HIP_CHECK(persistent ? recurrence_persistent() : recurrence_steps());
        HIP_CHECK(lstm3_and_query_grads());
        return image_side();
    }
};

}  // namespace

extern "C" {

size_t s2vt_attn_workspace_bytes(const s2vt_dims* d, int32_t B)
{
    if (!attn_dims_ok(d) || B <= 0) return 0;
    Carver c(nullptr, 0);
    return carve_attn(c, d, B, nullptr);
}

// n_video = 0: the unroll on B videos.  n_video > 0 (s2vt_attn_teacher_forced_fwd_rows): B = n_video * samples sample-major rows over
// n_video image blocks -- one prologue for the n_video videos, the attention step in its row -> video form, per-step launches.
static int attn_tf_fwd_impl(const s2vt_dims* d, const s2vt_attn_params* p, const float* video, int32_t B, const int32_t* caption,
                            int32_t caption_steps, float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id,
                            float* logits, float* alphas_out, void* workspace, size_t workspace_bytes, s2vt_stream stream, int n_video)
{
    AttnWs w;
    int rc = attn_unroll_open(d, attn_params_ok(p) && video && caption && logits, B, caption_steps, keep, video_id, sample_id, workspace, workspace_bytes,
                              n_video, chain_fault() ? S2VT_E_CHAIN_TIMEOUT : S2VT_OK, &w);
    if (rc != S2VT_OK) return rc;
    const int H = d->lstm_dim, V = d->n_words, Tv = d->n_video_lstm_step, Tc = caption_steps;
    hipStream_t st = S(stream);
    const size_t BH = (size_t)B * H;
    const NoiseIds ids{video_id, sample_id, seed};

    if (n_video > 0) HIP_TRY(launch_attn_row_video(w.rowvid, B, n_video, st));
    HIP_TRY(launch_prep_caption(caption, w.prev, w.tgt, B, d->n_caption_lstm_step, st));      // prev[t*B + b] = caption[b][t-1] for t >= 1
    {
        ZeroList z;     // zero initial state (:100-101), the zero partial of step 0 (current_embed = 0, :105)
        z.add(w.C3, BH * 4); z.add(w.H3, BH * 4); z.add(w.O3, BH * 4); z.add(w.G3, BH * 4 * 4);
        HIP_TRY(launch_zero_regions(z, st));
    }
    rc = attn_prologue(d, p, video, n_video > 0 ? n_video : B, w.img, st);
    if (rc != S2VT_OK) return rc;
    // the embedding rows of W3 for every step >= 1 in one product, written where the step's gates will go: the first block of
    // each pre-activation chain (the word fed at step t is caption[:, t-1], :141-142)
    if (Tc > 1) {
        ASeg se = make_seg(p->Wemb, H, H, H, 0, w.prev + B);
        HIP_TRY(store_call(&se, 1, p->lstm3_W, 4 * H, nullptr, w.G3 + 4 * BH, 4 * H, (Tc - 1) * B, 4 * H, 0, -1, st));
    }
    if (n_video == 0 && attn_chain_eligible(B, H, Tv) && attn_chain_weights_ok(p)) {
        HIP_TRY(launch_attn_chain(attn_fwd_chain_args(p, w, B, H, Tc, Tv, keep, ids), st));
    } else {
        DecodeStep s{};     // (its attention half: the query is the DROPPED output, `h_prev = output1`, :135)
        s.p = p; s.img = w.img; s.M = B; s.H = H; s.Tv = Tv; s.store_cfg = -1;
        s.row_video = w.rowvid; s.n_video = n_video;       // (n_video > 0: the B rows share n_video image blocks; else NULL, 0)
        for (int t = 0; t < Tc; ++t) {
            s.t = t; s.hWa = w.hWa + t * BH; s.alpha = w.alpha + (size_t)t * Tv * B; s.asum = w.asum + (size_t)t * B; s.ctx = w.ctx + t * BH;
            HIP_TRY(attn_attend(s, w.O3 + t * BH, st));                                                     // (:113-128)
            // LSTM3 (:131): the chain continues from the hoisted partial with the recurrent rows, then the context rows
            ASeg s3[2] = {make_seg(w.H3 + t * BH, H, H, 2 * H), make_seg(w.ctx + t * BH, H, H, 0)};
            HIP_TRY(lstm_call(s3, 2, p->lstm3_W, p->lstm3_b, w.C3 + t * BH, 0, w.C3 + (t + 1) * BH, w.H3 + (t + 1) * BH, w.O3 + (t + 1) * BH,
                              w.G3 + (size_t)t * 4 * BH, B, H, keep, ids, kDropCode3 + (uint32_t)t, -1, st, w.G3 + (size_t)t * 4 * BH, 4 * H, 0));
        }
    }
    // output layer for all steps at once (:134): chain blocks [embed ; atten ; output1]; step 0 has no word
    {
        ASeg s0[2] = {make_seg(w.ctx, H, H, H), make_seg(w.O3 + BH, H, H, 0)};
        HIP_TRY(store_call(s0, 2, p->embed_nn_Wp, H, p->embed_nn_bp, w.Y, H, B, H, 1, -1, st));
        if (Tc > 1) {
            ASeg s1[3] = {make_seg(p->Wemb, H, H, 2 * H, 0, w.prev + B), make_seg(w.ctx + BH, H, H, H), make_seg(w.O3 + 2 * BH, H, H, 0)};
            HIP_TRY(store_call(s1, 3, p->embed_nn_Wp, H, p->embed_nn_bp, w.Y + BH, H, (Tc - 1) * B, H, 1, -1, st));
        }
    }
    // vocabulary logits (:143), rows t*B + b
    ASeg so = make_seg(w.Y, H, H, 0);
    HIP_TRY(store_call(&so, 1, p->embed_word_W, V, p->embed_word_b, logits, V, Tc * B, V, 0, -1, st));
    if (alphas_out) HIP_TRY(copy_alphas_out(alphas_out, w.alpha, (size_t)Tc * Tv * B * 4, st));
    return S2VT_OK;
}

int s2vt_attn_teacher_forced_fwd(const s2vt_dims* d, const s2vt_attn_params* p, const float* video, int32_t B, const int32_t* caption,
                                 int32_t caption_steps, float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id,
                                 float* logits, float* alphas_out, void* workspace, size_t workspace_bytes, s2vt_stream stream)
{
    return attn_tf_fwd_impl(d, p, video, B, caption, caption_steps, keep, seed, video_id, sample_id, logits, alphas_out, workspace, workspace_bytes,
                            stream, 0);
}

int s2vt_attn_teacher_forced_fwd_rows(const s2vt_dims* d, const s2vt_attn_params* p, const float* video, int32_t n_video, int32_t samples,
                                      const int32_t* caption, int32_t caption_steps, float keep, uint64_t seed, const int32_t* video_id,
                                      const int32_t* sample_id, float* logits, float* alphas_out, void* workspace, size_t workspace_bytes,
                                      s2vt_stream stream)
{
    if (!attn_rows_shape_ok(d, n_video, samples)) return S2VT_E_BADARG;
    return attn_tf_fwd_impl(d, p, video, n_video * samples, caption, caption_steps, keep, seed, video_id, sample_id, logits, alphas_out, workspace,
                            workspace_bytes, stream, n_video);
}

int s2vt_attn_loss_inputs(const int32_t* caption, const float* mask, int32_t B, int32_t Tc, float beta, int32_t* target_tm, float* coef_tm,
                          float* reg_tm, float* mask_sum, s2vt_stream stream)
{
    if (!caption || !mask || !target_tm || !coef_tm || !mask_sum || B <= 0 || Tc <= 0) return S2VT_E_BADARG;
    hipLaunchKernelGGL(attn_loss_inputs_kernel, dim3(1), dim3(256), 0, S(stream), caption, mask, B, Tc, beta, target_tm, coef_tm, reg_tm, mask_sum);
    HIP_TRY(hipGetLastError());
    return S2VT_OK;
}

// rows: the unroll's B, or n_video * samples of the shared-block form (n_video > 0); shape_ok: what the entry point checks of them
static int attn_step_scalars_impl(const float* coef, const float* nll, int64_t R, const float* reg_coef, float reg_m, const float* mask_sum_local,
                                  const float* mask_sum_global, float* loss, float* gscale, float* sumsq, const s2vt_dims* d, bool shape_ok,
                                  int rows, int n_video, void* workspace, size_t workspace_bytes, s2vt_stream stream)
{
    if (!coef || !nll || R < 0 || !mask_sum_local || !mask_sum_global || !shape_ok || !workspace) return S2VT_E_BADARG;
    if (R > (int64_t)d->n_caption_lstm_step * rows) return S2VT_E_BADARG;
    Carver c(workspace, workspace_bytes);
    AttnWs w;
    carve_attn(c, d, rows, &w, n_video);
    if (!c.ok()) return S2VT_E_WORKSPACE;
    hipLaunchKernelGGL(attn_step_scalars_kernel, dim3(1), dim3(256), 0, S(stream), coef, nll, reg_coef, w.asum, reg_m, (int)R, mask_sum_local,
                       mask_sum_global, loss, gscale, sumsq);
    HIP_TRY(hipGetLastError());
    return S2VT_OK;
}

int s2vt_attn_step_scalars(const float* coef, const float* nll, int64_t R, const float* reg_coef, float reg_m, const float* mask_sum_local,
                           const float* mask_sum_global, float* loss, float* gscale, float* sumsq, const s2vt_dims* d, int32_t B,
                           void* workspace, size_t workspace_bytes, s2vt_stream stream)
{
    return attn_step_scalars_impl(coef, nll, R, reg_coef, reg_m, mask_sum_local, mask_sum_global, loss, gscale, sumsq, d, attn_dims_ok(d) && B > 0, B, 0,
                                  workspace, workspace_bytes, stream);
}

// The driver only: validate and carve, decide `persistent` and `gated`, then the stages of AttnBwd in order -- vocab, output_layer_grads
// (now, or beside the persistent recurrence), dcat, recurrence_persistent | recurrence_steps, lstm3_and_query_grads, image_side -- and ONE
// exit: once the gate has been armed or the side stream forked, a call that fails passes the join like one that succeeds.
static int attn_bptt_bwd_impl(const s2vt_dims* d, const s2vt_attn_params* p, const s2vt_attn_params* grads, const float* video, int32_t B,
                              const float* dlogits, int32_t caption_steps, const float* reg_coef, float reg_m, float keep, uint64_t seed,
                              const int32_t* video_id, const int32_t* sample_id, void* workspace, size_t workspace_bytes, s2vt_stream stream,
                              int n_video)
{
    AttnWs w;
    const int rc = attn_unroll_open(d, attn_params_ok(p) && attn_params_ok(grads) && video && dlogits, B, caption_steps, keep, video_id, sample_id, workspace,
                                    workspace_bytes, n_video, d && (d->lstm_dim & 3) ? S2VT_E_BADARG : S2VT_OK, &w);
    if (rc != S2VT_OK) return rc;
    AttnBwd x{side_stream()};
    const SideStream& ss = x.ss;
    const int H = d->lstm_dim, Tv = d->n_video_lstm_step, Tc = caption_steps;
    x.H = H; x.V = d->n_words; x.D = d->dim_image; x.Tv = Tv; x.Tc = Tc; x.B = B; x.n_video = n_video;
    x.NV = n_video > 0 ? n_video : B; x.R = Tc * B; x.R1 = (Tc - 1) * B; x.BH = (size_t)B * H;
    x.p = p; x.grads = grads; x.video = video; x.dlogits = dlogits; x.reg_coef = reg_coef; x.reg_m = reg_m;
    x.keep = keep; x.seed = seed; x.video_id = video_id; x.sample_id = sample_id; x.st = S(stream); x.w = w;
    x.persistent = n_video == 0 && attn_bwd_chain_eligible(B, H, Tv) && attn_chain_weights_ok(p);
    // Gated overlap (S2VT_OVERLAP=0 switches it off): the weight gradients of the vocabulary projection and of the output layer feed
    // nothing in the recurrence -- with the persistent backward recurrence they are launched on the side stream once its grid is resident and
    // run BESIDE it (a one-wave-per-SIMD grid that waits in hand-offs more than half of its time), joined at the end of the call.
    // Measured (bench.py --workload attention / attention32, S2VT_OVERLAP=0 against 2, twice each): Tv = 5: 2.63 -> 2.57 ms per step; Tv = 32: 3.25 -> 3.27.
    // This recurrence holds 150 KB of LDS per CU, so the LDS-staged contractions cannot share a CU with it (as they do with the LSTM recurrences'
    // 64 KB): they fill the CUs its workgroups leave at the end and run beside the launches that follow it.  On for the register-frames form only.
    x.gated = ss.ok && ss.mode == 2 && x.persistent && Tv <= 5;
    std::unique_lock<std::mutex> side_lk(side_stream_mutex(), std::defer_lock);
    if (x.gated) side_lk.lock();

    const hipError_t e = x.stages();
    // join: the caller's stream waits for the side stream's gradients (after a failed launch too: nothing stays behind on the side stream
    // that the caller's stream does not wait for)
    const hipError_t j = x.side_used ? fork_to(ss.s, x.st, ss.ev[2]) : hipSuccess;
    HIP_TRY(e);
    HIP_TRY(j);
    return S2VT_OK;
}

int s2vt_attn_bptt_bwd(const s2vt_dims* d, const s2vt_attn_params* p, const s2vt_attn_params* grads, const float* video, int32_t B,
                       const float* dlogits, int32_t caption_steps, const float* reg_coef, float reg_m, float keep, uint64_t seed,
                       const int32_t* video_id, const int32_t* sample_id, void* workspace, size_t workspace_bytes, s2vt_stream stream)
{
    return attn_bptt_bwd_impl(d, p, grads, video, B, dlogits, caption_steps, reg_coef, reg_m, keep, seed, video_id, sample_id, workspace,
                              workspace_bytes, stream, 0);
}

int s2vt_attn_step_scalars_rows(const float* coef, const float* nll, int64_t R, const float* reg_coef, float reg_m, const float* mask_sum_local,
                                const float* mask_sum_global, float* loss, float* gscale, float* sumsq, const s2vt_dims* d, int32_t n_video,
                                int32_t samples, void* workspace, size_t workspace_bytes, s2vt_stream stream)
{
    const bool ok = attn_rows_shape_ok(d, n_video, samples);
    return attn_step_scalars_impl(coef, nll, R, reg_coef, reg_m, mask_sum_local, mask_sum_global, loss, gscale, sumsq, d, ok, ok ? n_video * samples : 0,
                                  n_video, workspace, workspace_bytes, stream);
}

int s2vt_attn_bptt_bwd_rows(const s2vt_dims* d, const s2vt_attn_params* p, const s2vt_attn_params* grads, const float* video, int32_t n_video,
                            int32_t samples, const float* dlogits, int32_t caption_steps, const float* reg_coef, float reg_m, float keep,
                            uint64_t seed, const int32_t* video_id, const int32_t* sample_id, void* workspace, size_t workspace_bytes,
                            s2vt_stream stream)
{
    if (!attn_rows_shape_ok(d, n_video, samples)) return S2VT_E_BADARG;
    return attn_bptt_bwd_impl(d, p, grads, video, n_video * samples, dlogits, caption_steps, reg_coef, reg_m, keep, seed, video_id, sample_id,
                              workspace, workspace_bytes, stream, n_video);
}

int s2vt_attn_decode_greedy(const s2vt_dims* d, const s2vt_attn_params* p, const float* video, int32_t B, int32_t video_base, int32_t* ids_out,
                            float* alphas_out, void* workspace, size_t workspace_bytes, s2vt_stream stream)
{
    if (!attn_dims_ok(d) || !attn_params_ok(p) || !video || !ids_out || !workspace || B <= 0) return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    const int H = d->lstm_dim, V = d->n_words, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step;
    Carver c(workspace, workspace_bytes);
    AttnWs w;
    carve_attn(c, d, B, &w);
    if (!c.ok()) return S2VT_E_WORKSPACE;
    hipStream_t st = S(stream);
    const size_t BH = (size_t)B * H;
    {
        ZeroList z;
        z.add(w.C3, BH * 4); z.add(w.H3, BH * 4); z.add(w.packed, (size_t)Tc * B * kPickStride * 8);
        HIP_TRY(launch_zero_regions(z, st));
    }
    hipLaunchKernelGGL(attn_rows_kernel, dim3((B + 255) / 256), dim3(256), 0, st, w.vid, w.sid, B, video_base);
    HIP_TRY(hipGetLastError());
    const int rc = attn_prologue(d, p, video, B, w.img, st);
    if (rc != S2VT_OK) return rc;
    const NoiseIds ids{w.vid, w.sid, 0};
    DecodeStep s{};     // state in the history slots t / t + 1, one image block per row, the regulariser's sum kept
    s.p = p; s.img = w.img; s.M = B; s.H = H; s.Tv = Tv; s.store_cfg = s.lstm_cfg = -1;
    for (int t = 0; t < Tc; ++t) {
        s.t = t;
        s.c_prev = w.C3 + t * BH; s.h_prev = w.H3 + t * BH; s.c_new = w.C3 + (t + 1) * BH; s.h_new = w.H3 + (t + 1) * BH;
        s.word_key = t > 0 ? w.packed + (size_t)(t - 1) * B * kPickStride : nullptr;                      // the word picked at step t-1 (:196-197)
        s.hWa = w.hWa + t * BH; s.alpha = w.alpha + (size_t)t * Tv * B; s.asum = w.asum + (size_t)t * B; s.ctx = w.ctx + t * BH; s.Y = w.Y + t * BH;
        HIP_TRY(decode_step(s, st));
        HIP_TRY(pick_call(s.Y, H, p->embed_word_W, p->embed_word_b, B, H, V, ids, t, w.packed + (size_t)t * B * kPickStride, nullptr, -1, st, kPickStride));
    }
    hipLaunchKernelGGL(attn_unpack_ids_kernel, dim3((B * Tc + 255) / 256), dim3(256), 0, st, w.packed, ids_out, B, Tc, kPickStride);
    HIP_TRY(hipGetLastError());
    if (alphas_out) HIP_TRY(copy_alphas_out(alphas_out, w.alpha, (size_t)Tc * Tv * B * 4, st));
    return S2VT_OK;
}

size_t s2vt_attn_rows_workspace_bytes(const s2vt_dims* d, int32_t n_video, int32_t samples)
{
    if (!attn_rows_shape_ok(d, n_video, samples)) return 0;
    Carver c(nullptr, 0);
    return carve_attn(c, d, n_video * samples, nullptr, n_video);
}

size_t s2vt_attn_sample_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t K, int32_t with_greedy)
{
    if (K < 0 || (K == 0 && !with_greedy) || !attn_rows_shape_ok(d, B, K + (with_greedy ? 1 : 0))) return 0;
    Carver c(nullptr, 0);
    return carve_attn_sample(c, d, B, (K + (with_greedy ? 1 : 0)) * B, nullptr);
}

// K multinomial captions per video and (with_greedy) the greedy one: the decode loop of s2vt_attn_decode_greedy on R = (K + greedy) B
// sample-major rows that share the B image blocks (one prologue; the attention step in its row -> video form).  The PICK epilogue
// draws Gumbel-max noise from the Philox counters (video_base + j, s, step) for sample s >= 0 and takes the argmax for the greedy
// block (sample id -1); the packed pick of step t-1 is the embedding gather index of step t.  No dropout, no <bos>, no host round
// trip.  Per-step launches: the persistent recurrences (attn_chain*.hip) hold one image block per row and at most 64 rows.
// stop_at_eos (s2vt_attn_sample_ex): every step's five launches cover the rows still sampling only -- a compact list of rows and its
// length, both on the device (live_rows_kernel on the picks of step t - 1); state stays where it is, indexed by the original row, so a
// row's chains are those of the full launch (the tile does not enter a chain) and its ids up to its first <eos> the same bits.
static int attn_sample_impl(const s2vt_dims* d, const s2vt_attn_params* p, const float* video, int32_t B, int32_t K, int32_t with_greedy,
                            uint64_t seed, int32_t video_base, int stop_at_eos, int32_t* ids_out, int32_t* greedy_out, void* workspace,
                            size_t workspace_bytes, s2vt_stream stream)
{
    const int g = with_greedy ? 1 : 0;
    if (K < 0 || (K == 0 && !g) || !attn_rows_shape_ok(d, B, K + g) || !attn_params_ok(p) || !video || !workspace) return S2VT_E_BADARG;
    if ((K > 0 && !ids_out) || (g && !greedy_out)) return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    const int H = d->lstm_dim, V = d->n_words, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step, R = (K + g) * B;
    Carver c(workspace, workspace_bytes);
    AttnSampleWs w;
    carve_attn_sample(c, d, B, R, &w);
    if (!c.ok()) return S2VT_E_WORKSPACE;
    hipStream_t st = S(stream);
    {
        ZeroList z;     // the zero state (:164-165); the pick words are combined with atomicMax from zero
        z.add(w.c[0], (size_t)R * H * 4); z.add(w.h[0], (size_t)R * H * 4); z.add(w.packed, (size_t)Tc * R * kPickStride * 8);
        HIP_TRY(launch_zero_regions(z, st));
    }
    hipLaunchKernelGGL(attn_sample_rows_kernel, dim3((R + 255) / 256), dim3(256), 0, st, w.vid, w.sid, w.rowvid, R, (int)B, (int)K, (int)video_base);
    HIP_TRY(hipGetLastError());
    const int rc = attn_prologue(d, p, video, B, w.img, st);
    if (rc != S2VT_OK) return rc;
    const NoiseIds ids{w.vid, w.sid, seed};
    // stop-at-<eos> mode: tiles for launches whose row count only the device knows -- row tiles small enough that the launch shrinks
    // with the count (the reasoning of the S2VT sampler, api.hip sample_decode).  Dev knobs: S2VT_ATTN_EOS_STORE_CFG (the query and
    // output-layer products; -1 = the cost model's tile, 64 rows at these widths), S2VT_ATTN_EOS_LSTM_CFG, S2VT_ATTN_EOS_PICK_CFG.
    // Measured at R = 384, Tv = 5, mean length 6.8 (tools/bench_attn_rl.py --stop-at-eos, table in profiles/NOTES.md), ms per sampler
    // call, 5.30 for the loop that never stops: these defaults 4.06 (the cost model's store tile is 64x32 there); cell step on the
    // tile the full row count would get (96 rows) 4.69, on 16 / 48 / 64 rows 6.36 / 4.83 / 4.68; store 64x64 / 64x96 / 64x128
    // 4.78 / 5.45 / 6.23; pick 32x96 / 64x64 / 64x128 instead of choose_pick's 64x96 4.25 / 4.18 / 4.33.
    int scfg = -1, lcfg = -1, pcfg = -1;
    if (stop_at_eos) {
        static const int sk = [] { const char* e = getenv("S2VT_ATTN_EOS_STORE_CFG"); return e ? atoi(e) : -1; }();
        static const int lk = [] { const char* e = getenv("S2VT_ATTN_EOS_LSTM_CFG"); return e ? atoi(e) : 4; }();     // kLstm[4] = gw32x16u
        static const int pk = [] { const char* e = getenv("S2VT_ATTN_EOS_PICK_CFG"); return e ? atoi(e) : -1; }();
        scfg = sk; lcfg = R > 64 ? lk : -1; pcfg = pk;
    }
    DecodeStep s{};     // state ping-pong (step t reads slot t & 1), the R rows over the B image blocks, one step's worth of everything else
    s.p = p; s.img = w.img; s.M = R; s.H = H; s.Tv = Tv; s.store_cfg = scfg; s.lstm_cfg = lcfg;
    s.hWa = w.hWa; s.alpha = w.alpha; s.ctx = w.ctx; s.Y = w.Y; s.row_video = w.rowvid; s.n_video = B;
    for (int t = 0; t < Tc; ++t) {
        s.t = t;
        s.c_prev = w.c[t & 1]; s.h_prev = w.h[t & 1]; s.c_new = w.c[(t & 1) ^ 1]; s.h_new = w.h[(t & 1) ^ 1];
        s.word_key = t > 0 ? w.packed + (size_t)(t - 1) * R * kPickStride : nullptr;                      // the word picked at step t-1 (:196-197)
        if (stop_at_eos) {
            // a finished row's state stays in whichever slot it was last written to and is never read again; its later pick words stay zero
            HIP_TRY(launch_live_rows(s.word_key, kPickStride, w.live[(t + 1) & 1], w.nlive + (t > 0 ? t - 1 : 0), w.live[t & 1], w.nlive + t, R, st));
            s.live = w.live[t & 1]; s.n_live = w.nlive + t;
        }
        HIP_TRY(decode_step(s, st));
        HIP_TRY(pick_call(w.Y, H, p->embed_word_W, p->embed_word_b, R, H, V, ids, t, w.packed + (size_t)t * R * kPickStride, nullptr, pcfg, st, kPickStride,
                          s.live, s.n_live));
    }
    if (K > 0) {
        hipLaunchKernelGGL(attn_unpack_rows_kernel, dim3((K * B * Tc + 255) / 256), dim3(256), 0, st, w.packed, ids_out, R, 0, (int)(K * B), Tc, kPickStride);
        HIP_TRY(hipGetLastError());
    }
    if (g) {
        hipLaunchKernelGGL(attn_unpack_rows_kernel, dim3((B * Tc + 255) / 256), dim3(256), 0, st, w.packed, greedy_out, R, (int)(K * B), (int)B, Tc, kPickStride);
        HIP_TRY(hipGetLastError());
    }
    return S2VT_OK;
}

int s2vt_attn_sample(const s2vt_dims* d, const s2vt_attn_params* p, const float* video, int32_t B, int32_t K, int32_t with_greedy, uint64_t seed,
                     int32_t video_base, int32_t* ids_out, int32_t* greedy_out, void* workspace, size_t workspace_bytes, s2vt_stream stream)
{
    return attn_sample_impl(d, p, video, B, K, with_greedy, seed, video_base, 0, ids_out, greedy_out, workspace, workspace_bytes, stream);
}

int s2vt_attn_sample_ex(const s2vt_dims* d, const s2vt_attn_params* p, const float* video, int32_t B, int32_t K, int32_t with_greedy, uint64_t seed,
                        int32_t video_base, int32_t flags, int32_t* ids_out, int32_t* greedy_out, void* workspace, size_t workspace_bytes,
                        s2vt_stream stream)
{
    if (flags & ~S2VT_SAMPLE_STOP_AT_EOS) return S2VT_E_BADARG;
    return attn_sample_impl(d, p, video, B, K, with_greedy, seed, video_base, flags & S2VT_SAMPLE_STOP_AT_EOS, ids_out, greedy_out, workspace,
                            workspace_bytes, stream);
}

size_t s2vt_attn_beam_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t beam)
{
    if (!attn_beam_shape_ok(d, B, beam)) return 0;
    Carver c(nullptr, 0);
    return carve_attn_beam(c, d, B, beam, nullptr);
}

int s2vt_attn_beam_encode(const s2vt_dims* d, const s2vt_attn_params* p, const float* video, int32_t B, int32_t beam, void* workspace,
                          size_t workspace_bytes, s2vt_stream stream)
{
    if (!attn_beam_shape_ok(d, B, beam) || !attn_params_ok(p) || !video || !workspace) return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    Carver c(workspace, workspace_bytes);
    AttnBeamWs w;
    carve_attn_beam(c, d, B, beam, &w);
    if (!c.ok()) return S2VT_E_WORKSPACE;
    return attn_prologue(d, p, video, B, w.img, S(stream));
}

int s2vt_attn_beam_step(const s2vt_dims* d, const s2vt_attn_params* p, int32_t B, int32_t beam, int32_t t, int32_t R, const int32_t* video_of_row,
                        const int32_t* parent, const int32_t* word, int32_t k, int32_t* top_ids, float* top_logp, float* logits_out,
                        float* alphas_out, void* workspace, size_t workspace_bytes, s2vt_stream stream)
{
    if (!attn_beam_shape_ok(d, B, beam) || !attn_params_ok(p) || !video_of_row || !parent || !word || !top_ids || !top_logp || !workspace)
        return S2VT_E_BADARG;
    if (t < 0 || t >= d->n_caption_lstm_step || R < 0 || R > B * beam || k < 1 || k > kBeamTopkMax || k > d->n_words) return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    Carver c(workspace, workspace_bytes);
    AttnBeamWs w;
    carve_attn_beam(c, d, B, beam, &w);
    if (!c.ok()) return S2VT_E_WORKSPACE;
    if (R == 0) return S2VT_OK;
    const int H = d->lstm_dim, V = d->n_words, Tv = d->n_video_lstm_step;
    hipStream_t st = S(stream);
    // 1. gather: the parents' cell state (zeros at step 0), the clamped parent rows and words
    hipLaunchKernelGGL(attn_beam_gather_kernel, dim3(R), dim3(256), 0, st, parent, word, (int)t, (int)(B * beam), H, V, w.c[(t & 1) ^ 1], w.cg, w.par, w.word);
    HIP_TRY(hipGetLastError());
    // 2. - 5. the decode step on the R hypotheses: state ping-pong (step t writes slot t & 1; rows are permuted between steps), the
    // parent's clean h gathered through the parent index and its cell state from the dense copy, the word's embedding rows through
    // the clamped word, row -> video: hypothesis m reads its video's one [Tv, H] block of P and Vt
    DecodeStep s{};
    s.p = p; s.img = w.img; s.t = t; s.M = R; s.H = H; s.Tv = Tv; s.store_cfg = s.lstm_cfg = -1;
    s.c_prev = w.cg; s.h_prev = w.h[(t & 1) ^ 1]; s.h_rows = w.par; s.c_new = w.c[t & 1]; s.h_new = w.h[t & 1]; s.word_idx = w.word;
    s.hWa = w.hWa; s.alpha = alphas_out ? alphas_out : w.alpha; s.ctx = w.ctx; s.Y = w.Y; s.row_video = video_of_row; s.n_video = B;
    HIP_TRY(decode_step(s, st));
    // 6. vocabulary logits on the store tile, 7. top-k words and their log-probabilities
    float* logits = logits_out ? logits_out : w.logits;
    ASeg so = make_seg(w.Y, H, H, 0);
    HIP_TRY(store_call(&so, 1, p->embed_word_W, V, p->embed_word_b, logits, V, R, V, 0, -1, st));
    HIP_TRY(launch_vocab_topk(logits, V, R, V, k, top_ids, top_logp, st));
    return S2VT_OK;
}

}  // extern "C"
