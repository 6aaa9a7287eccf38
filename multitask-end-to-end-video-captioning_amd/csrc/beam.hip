// beam.hip -- batched beam-search decoding (final_beam_search.py:201-294 for B videos at once): the vocabulary top-k with its
// log-normaliser, and the library's beam step (parent-state gather, LSTM2 cell, vocabulary logits, top-k) with no host sync.
// The caption bookkeeping (the reference's TopN heaps, beam_search.py:44-80) stays on the host: its tie order follows heap
// history, which only a host heap reproduces.
#include <hip/hip_runtime.h>

#include <climits>

#include "api_util.h"
#include "detmath.h"
#include "rowreduce.h"
#include "topk_select.h"

using namespace s2vt_api;

namespace s2vt {

// ---------------------------------------------------------------------------------------------
// Vocabulary top-k with log-probabilities.  One workgroup (4 x wave64) per row of logits [R, V] (row stride ld):
//   ids [R, k]:  the k largest logits, by value descending, then index ascending on exact ties (a total order: deterministic,
//                and the order tf.nn.top_k returns);
//   logp[R, k]:  l[id] - lse, lse = max + log(sum exp(l - max)) evaluated in EXACTLY the order of softmax_nll_kernel (aux.hip):
//                same 256-thread stride, same float4 / tail split, dm_expf / dm_logf, the same block_reduce -- so logp is
//                bit-identical to the lp_t that s2vt_softmax_nll_fwd_bwd returns for that target.
// Selection: every thread keeps a sorted list of its KMAX best (value, index) pairs in registers while it streams its strided
// float4s (the row is read from HBM once; the normaliser's second pass hits L2), then k rounds of block arg-max over the list
// heads: xor-butterfly inside each wave, the four wave winners through LDS, the owning thread pops its head.  No atomics.
// Inputs are finite logits: NaN is out of scope (a NaN never enters a list and poisons lse).
// ---------------------------------------------------------------------------------------------
template <int KMAX>
__global__ __launch_bounds__(256) void vocab_topk_kernel(const float* logits, int ld, int V, int k, int32_t* ids, float* logp)
{
    __shared__ float sh[8];
    __shared__ float swv[2][4];
    __shared__ int swi[2][4];
    const int row = blockIdx.x;
    const float* l = logits + (size_t)row * ld;
    const int tid = threadIdx.x;
    const bool vec = ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(logits) & 15) == 0);
    const int V4 = vec ? (V >> 2) : 0;

    float tv[KMAX];
    int ti[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) { tv[j] = -INFINITY; ti[j] = INT_MAX; }

    // pass 1: row max (softmax_nll_kernel's order) + the per-thread candidate lists
    float mx = -INFINITY;
    for (int i = tid; i < V4; i += 256) {
        const float4 v = reinterpret_cast<const float4*>(l)[i];
        mx = fmaxf(fmaxf(mx, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
        tk_insert<KMAX>(tv, ti, v.x, 4 * i);
        tk_insert<KMAX>(tv, ti, v.y, 4 * i + 1);
        tk_insert<KMAX>(tv, ti, v.z, 4 * i + 2);
        tk_insert<KMAX>(tv, ti, v.w, 4 * i + 3);
    }
    for (int i = V4 * 4 + tid; i < V; i += 256) {
        const float v = l[i];
        mx = fmaxf(mx, v);
        tk_insert<KMAX>(tv, ti, v, i);
    }
    mx = block_reduce<true>(mx, sh);

    // pass 2: sum exp(l - max), term for term as softmax_nll_kernel adds it
    float se = 0.f;
    for (int i = tid; i < V4; i += 256) {
        const float4 v = reinterpret_cast<const float4*>(l)[i];
        se += dm_expf(v.x - mx) + dm_expf(v.y - mx) + dm_expf(v.z - mx) + dm_expf(v.w - mx);
    }
    for (int i = V4 * 4 + tid; i < V; i += 256) se += dm_expf(l[i] - mx);
    se = block_reduce<false>(se, sh);
    const float lse = mx + dm_logf(se);

    // k rounds of block arg-max over the list heads (LDS double-buffered by round parity: one barrier per round)
    const int lane = tid & 63, w = tid >> 6;
    for (int r = 0; r < k; ++r) {
        float bv = tv[0];
        int bi = ti[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (tk_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        const int p = r & 1;
        if (lane == 0) { swv[p][w] = bv; swi[p][w] = bi; }
        __syncthreads();
        bv = swv[p][0]; bi = swi[p][0];
#pragma unroll
        for (int q = 1; q < 4; ++q)
            if (tk_better(swv[p][q], swi[p][q], bv, bi)) { bv = swv[p][q]; bi = swi[p][q]; }
        if (ti[0] == bi) {                                   // indices are unique: exactly one thread owns the winner
#pragma unroll
            for (int j = 0; j < KMAX - 1; ++j) { tv[j] = tv[j + 1]; ti[j] = ti[j + 1]; }
            tv[KMAX - 1] = -INFINITY; ti[KMAX - 1] = INT_MAX;
        }
        if (tid == 0) {
            ids[(size_t)row * k + r] = bi;
            logp[(size_t)row * k + r] = bv - lse;
        }
    }
}

hipError_t launch_vocab_topk(const float* logits, int ld, int R, int V, int k, int32_t* ids, float* logp, hipStream_t st)
{
    if (R <= 0) return hipSuccess;
    if (k <= 1)
        hipLaunchKernelGGL(vocab_topk_kernel<1>, dim3(R), dim3(256), 0, st, logits, ld, V, k, ids, logp);
    else if (k <= 2)
        hipLaunchKernelGGL(vocab_topk_kernel<2>, dim3(R), dim3(256), 0, st, logits, ld, V, k, ids, logp);
    else if (k <= 4)
        hipLaunchKernelGGL(vocab_topk_kernel<4>, dim3(R), dim3(256), 0, st, logits, ld, V, k, ids, logp);
    else if (k <= 8)
        hipLaunchKernelGGL(vocab_topk_kernel<8>, dim3(R), dim3(256), 0, st, logits, ld, V, k, ids, logp);
    else
        hipLaunchKernelGGL(vocab_topk_kernel<16>, dim3(R), dim3(256), 0, st, logits, ld, V, k, ids, logp);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Beam step, stage 1: the inputs of the LSTM2 cell for the R live hypotheses, gathered into dense scratch rows:
//   c / h  <- the parent's LSTM2 state (step 0: the video's encoder state, slot Tv of c2e / h2e);
//   p2     <- row (Tv + t) * B + video of the shared LSTM1 products h1 @ W2[0:H] (every beam of a video shares LSTM1);
//   word   <- the word the hypothesis continues from.
// Indices are device data the host does not see here: out-of-range values are clamped into range (nothing is read outside
// the workspace or the embedding table); the host driver (beam_generator.BatchedBeamSearch) only passes valid ones.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void beam_gather_kernel(const int32_t* video_of_row, const int32_t* parent, const int32_t* word, int t,
                                                          int B, int Rmax, int H, int V, const float* c_enc, const float* h_enc,
                                                          const float* c_prev, const float* h_prev, const float* P2t, float* c_out,
                                                          float* h_out, float* p2_out, int32_t* word_out, int32_t* vid_out)
{
    const int m = blockIdx.x;
    int vid = video_of_row[m];
    vid = vid < 0 ? 0 : (vid >= B ? B - 1 : vid);
    const float *cs, *hs;
    if (t == 0) {
        cs = c_enc + (size_t)vid * H; hs = h_enc + (size_t)vid * H;
    } else {
        int par = parent[m];
        par = par < 0 ? 0 : (par >= Rmax ? Rmax - 1 : par);
        cs = c_prev + (size_t)par * H; hs = h_prev + (size_t)par * H;
    }
    const float* ps = P2t + (size_t)vid * 4 * H;
    for (int i = threadIdx.x; i < H; i += 256) {
        c_out[(size_t)m * H + i] = cs[i];
        h_out[(size_t)m * H + i] = hs[i];
    }
    for (int i = threadIdx.x; i < 4 * H; i += 256) p2_out[(size_t)m * 4 * H + i] = ps[i];
    if (threadIdx.x == 0) {
        if (vid_out) vid_out[m] = vid;                       // residual model: the clamped row -> video map of the cell launch's out1 operand
        const int wd = word[m];
        word_out[m] = wd < 0 ? 0 : (wd >= V ? V - 1 : wd);
    }
}

}  // namespace s2vt

namespace {

constexpr int kTopkMax = 16;

struct BeamWs {
    SampleEnc enc;                      // the sampler's encode half for B rows (sample_encode)
    float *c2, *h2;                     // LSTM2 state after the last step [Rmax][H] (row = hypothesis of that step)
    float *c2g, *h2g, *p2g;             // the cell's gathered inputs [Rmax][H], [Rmax][H], [Rmax][4H]
    int32_t* word;                      // clamped words [Rmax]
    float* logits;                      // [Rmax][V] (when the caller does not ask for them)
    float* out2; int32_t* vid;          // residual model only (else NULL), carved last: out1 + out2 of the step [Rmax][H], the clamped videos [Rmax]
};

size_t carve_beam(Carver& c, const s2vt_dims* d, int B, int beam, BeamWs* w)
{
    const size_t H = d->lstm_dim, V = d->n_words;
    const size_t Rmax = (size_t)B * beam;
    BeamWs t;
    carve_sample_enc(c, d, B, t.enc);
    t.enc.chain_sync = c.take<unsigned>(kChainSyncBytes / 4);
    t.enc.chain_abuf = c.take<float>(chain_scratch_floats((int)H));
    t.c2 = c.take<float>(Rmax * H); t.h2 = c.take<float>(Rmax * H);
    t.c2g = c.take<float>(Rmax * H); t.h2g = c.take<float>(Rmax * H);
    t.p2g = c.take<float>(Rmax * 4 * H);
    t.word = c.take<int32_t>(Rmax);
    t.logits = c.take<float>(Rmax * V);
    t.out2 = nullptr; t.vid = nullptr;
    if (is_residual(d)) { t.out2 = c.take<float>(Rmax * H); t.vid = c.take<int32_t>(Rmax); }
    if (w) *w = t;
    return c.off;
}

bool beam_shape_ok(const s2vt_dims* d, int B, int beam)
{
    return dims_ok_res(d) && B > 0 && beam >= 1 && beam <= kTopkMax && (int64_t)B * beam <= INT_MAX / 4;
}

}  // namespace

extern "C" {

int s2vt_vocab_topk(const float* logits, int32_t ld, int32_t R, int32_t V, int32_t k, int32_t* ids, float* logp, s2vt_stream stream)
{
    if (!logits || !ids || !logp || R < 0 || V <= 0 || ld < V || k < 1 || k > kTopkMax || k > V) return S2VT_E_BADARG;
    if (R == 0) return S2VT_OK;
    HIP_TRY(launch_vocab_topk(logits, ld, R, V, k, ids, logp, S(stream)));
    return S2VT_OK;
}

size_t s2vt_beam_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t beam)
{
    if (!beam_shape_ok(d, B, beam)) return 0;
    Carver c(nullptr, 0);
    return carve_beam(c, d, B, beam, nullptr);
}

int s2vt_beam_encode(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t beam, void* workspace,
                     size_t workspace_bytes, s2vt_stream stream)
{
    if (!beam_shape_ok(d, B, beam) || !sampler_params_ok(p) || !video || !workspace) return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    Carver c(workspace, workspace_bytes);
    BeamWs w;
    carve_beam(c, d, B, beam, &w);
    if (!c.ok()) return S2VT_E_WORKSPACE;
    if (chain_fault()) return S2VT_E_CHAIN_TIMEOUT;
    return sample_encode(d, p, video, B, w.enc, stream);
}

int s2vt_beam_step(const s2vt_dims* d, const s2vt_params* p, int32_t B, int32_t beam, int32_t t, int32_t R, const int32_t* video_of_row,
                   const int32_t* parent, const int32_t* word, int32_t k, int32_t* top_ids, float* top_logp, float* logits_out,
                   void* workspace, size_t workspace_bytes, s2vt_stream stream)
{
    if (!beam_shape_ok(d, B, beam) || !sampler_params_ok(p) || !video_of_row || !parent || !word || !top_ids || !top_logp || !workspace)
        return S2VT_E_BADARG;
    if (t < 0 || t >= d->n_caption_lstm_step || R < 0 || R > B * beam || k < 1 || k > kTopkMax || k > d->n_words) return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    Carver c(workspace, workspace_bytes);
    BeamWs w;
    carve_beam(c, d, B, beam, &w);
    if (!c.ok()) return S2VT_E_WORKSPACE;
    if (R == 0) return S2VT_OK;
    const int H = d->lstm_dim, E = d->word_dim, V = d->n_words, Tv = d->n_video_lstm_step;
    hipStream_t st = S(stream);
    const size_t BH = (size_t)B * H;
    // 1. gather: parents' LSTM2 state, the video's LSTM1 partial of this step, the words
    hipLaunchKernelGGL(beam_gather_kernel, dim3(R), dim3(256), 0, st, video_of_row, parent, word, (int)t, (int)B, (int)(B * beam), H, V,
                       w.enc.c2e + (size_t)Tv * BH, w.enc.h2e + (size_t)Tv * BH, w.c2, w.h2, w.enc.P2 + (size_t)(Tv + t) * 4 * BH, w.c2g,
                       w.h2g, w.p2g, w.word, w.vid);
    HIP_TRY(hipGetLastError());
    // 2. LSTM2 at R rows on the gathered partial, words and parent state
    Lstm2Step s2{};
    s2.p = p; s2.M = R; s2.H = H; s2.E = E;
    s2.partial = w.p2g; s2.word_idx = w.word; s2.c_prev = w.c2g; s2.h_prev = w.h2g;
    s2.c_new = w.c2; s2.h_new = w.h2; s2.lstm_cfg = -1;
    // residual model (residual_tf_s2vt.py:206-208): the cell launch also writes out1 + h', out1 = slot Tv + t + 1 of the video's LSTM1 history
    if (w.out2) { s2.out = w.out2; s2.out1 = w.enc.h1 + (size_t)(Tv + t + 1) * BH; s2.out1_rowidx = w.vid; }
    HIP_TRY(lstm2_step(s2, st));
    // 3. vocabulary logits on the store tile
    float* logits = logits_out ? logits_out : w.logits;
    ASeg so = make_seg(w.out2 ? w.out2 : w.h2, H, H, 0);
    HIP_TRY(store_call(&so, 1, p->embed_word_W, V, p->embed_word_b, logits, V, R, V, 0, -1, st));
    // 4. top-k words and their log-probabilities
    HIP_TRY(launch_vocab_topk(logits, V, R, V, k, top_ids, top_logp, st));
    return S2VT_OK;
}

}  // extern "C"
