// topk_feed.hip -- the decode feedback of sum_generate_words_tf_s2vt.py:163-174,208-210 (training) and :255-268 (build_generator): LSTM2
// is fed a weighted sum of the embeddings of the model's own top-k words, the weights being those k scores divided by their sum.  The
// ids are the only part that is not differentiable, so the mix has a backward of its own, and the embedding scatter takes k weighted ids.
#include <hip/hip_runtime.h>

#include <climits>

#include "api_util.h"
#include "topk_select.h"

using namespace s2vt_api;

namespace s2vt {

// ---------------------------------------------------------------------------------------------
// Top-k mix, forward.  One workgroup (4 x wave64) per row of the score plane [R, V] (row stride ld):
//   ids [R, k]: the k largest scores in vocab_topk_kernel's total order (beam.hip) -- value descending, index ascending on exact ties,
//               which is the order tf.nn.top_k returns (topk_select.h); selected the same way (per-thread sorted lists, k rounds of block arg-max);
//   S   [R]   : ((s_0 + s_1) + s_2) + ... , the scores added in ascending k (:170 tf.reduce_sum over k entries);
//   w   [R, k]: s_j / S, an IEEE division.  S = 0 is the script's own 0/0 and is left as it is;
//   x   [R, E]: ((((0 + w_0 e_0) + w_1 e_1) + ...), e_j = Wemb[ids_j] -- the chain of :171-173 from a zero vector, every product and every
//               addition rounded on its own (no FMA).
// The scores are finite: a NaN never enters a list, and an id that was never set is written as 0 so that nothing is read outside Wemb.
// step != NULL (an unroll): the row's first thread also writes generated = ids_0 (or the word the caller chose) and, in training, the loss
// coefficient loss_weight * mask and the clamped target of the step, as avg_step_kernel does (train.hip).  ids == NULL: only those (the
// last step forms no mix).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void topk_mix_fwd_kernel(const float* scores, int ld, int V, int k, const float* Wemb, int E, int32_t* ids,
                                                           float* wts, float* S, float* x, int ldx, const TopkStep step, bool has_step)
{
    __shared__ float swv[2][4];
    __shared__ int swi[2][4];
    __shared__ float sel_v[kTopkFeedMax];
    __shared__ int sel_i[kTopkFeedMax];
    __shared__ float sel_w[kTopkFeedMax];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* l = scores + (size_t)row * ld;

    float tv[kTopkFeedMax];
    int ti[kTopkFeedMax];
#pragma unroll
    for (int j = 0; j < kTopkFeedMax; ++j) { tv[j] = -INFINITY; ti[j] = INT_MAX; }
    // (eight independent loads in flight per thread, then their insertions: the lists' data-dependent branches would otherwise put one
    //  memory round trip in front of every element; the order of insertion does not change a sorted list under a total order)
    constexpr int U = 8;
    int i0 = tid;
    for (; i0 + (U - 1) * 256 < V; i0 += U * 256) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = l[i0 + u * 256];
#pragma unroll
        for (int u = 0; u < U; ++u) tk_insert<kTopkFeedMax>(tv, ti, v[u], i0 + u * 256);
    }
    for (; i0 < V; i0 += 256) tk_insert<kTopkFeedMax>(tv, ti, l[i0], i0);

    // k rounds of block arg-max over the list heads (LDS double-buffered by round parity: one barrier per round)
    const int lane = tid & 63, wv = tid >> 6;
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
        if (lane == 0) { swv[p][wv] = bv; swi[p][wv] = bi; }
        __syncthreads();
        bv = swv[p][0]; bi = swi[p][0];
#pragma unroll
        for (int q = 1; q < 4; ++q)
            if (tk_better(swv[p][q], swi[p][q], bv, bi)) { bv = swv[p][q]; bi = swi[p][q]; }
        if (ti[0] == bi && bi != INT_MAX) {                  // indices are unique: exactly one thread owns the winner
#pragma unroll
            for (int j = 0; j < kTopkFeedMax - 1; ++j) { tv[j] = tv[j + 1]; ti[j] = ti[j + 1]; }
            tv[kTopkFeedMax - 1] = -INFINITY; ti[kTopkFeedMax - 1] = INT_MAX;
        }
        if (tid == 0) { sel_v[r] = bv; sel_i[r] = (unsigned)bi < (unsigned)V ? bi : 0; }
    }
    if (tid == 0) {
        float sum = sel_v[0];
        for (int j = 1; j < k; ++j) sum = __fadd_rn(sum, sel_v[j]);
        for (int j = 0; j < k; ++j) sel_w[j] = __fdiv_rn(sel_v[j], sum);
        if (ids) {
            for (int j = 0; j < k; ++j) { ids[(size_t)row * k + j] = sel_i[j]; wts[(size_t)row * k + j] = sel_w[j]; }
            S[row] = sum;
        }
        if (has_step) {
            const size_t nt = (size_t)row * step.Tc + step.t, tn = (size_t)step.t * step.N + row;
            step.generated[nt] = step.emit ? step.emit[row] : sel_i[0];
            if (step.caption) {
                const int32_t c = step.caption[nt];
                step.coef_tm[tn] = step.loss_weight * step.mask[nt];
                step.target_tm[tn] = c < 0 ? 0 : c >= V ? V - 1 : c;
            }
        }
    }
    if (!x) return;
    __syncthreads();
    for (int e = tid; e < E; e += 256) {
        float acc = 0.f;
        for (int j = 0; j < k; ++j) acc = __fadd_rn(acc, __fmul_rn(sel_w[j], Wemb[(size_t)sel_i[j] * E + e]));
        x[(size_t)row * ldx + e] = acc;
    }
}

hipError_t launch_topk_mix_fwd(const float* scores, int ld, int R, int V, int k, const float* Wemb, int E, int32_t* ids, float* wts, float* S,
                               float* x, int ldx, const TopkStep* step, hipStream_t st)
{
    if (R <= 0) return hipSuccess;
    TopkStep none{};
    hipLaunchKernelGGL(topk_mix_fwd_kernel, dim3(R), dim3(256), 0, st, scores, ld, V, k, Wemb, E, ids, wts, S, x, ldx, step ? *step : none,
                       step != nullptr);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Top-k mix, backward.  One workgroup per row.  With x = sum_j w_j e_j, w_j = s_j / S, S = sum_j s_j and the ids constants:
//   ds_j = dx . e_j,  g = sum_j w_j ds_j,  dl_j = (ds_j - g) / S                        (d x / d s_j = (e_j - x) / S)
//   dscores[row][ids_j] += dl_j            -- the columns of a row are distinct: no conflicts, every other column keeps its bits
//   dO[row][:]          += sum_j dl_j Wout[:, ids_j]   (Wout [H, V]: the gradient w.r.t. the dropped LSTM2 output that made the scores)
// dO == NULL: the first addition only.  The k columns of Wout are H strided reads each: 256 threads per row keep them in flight.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void topk_mix_bwd_kernel(const float* dx, int lddx, const int32_t* ids, const float* wts, const float* S,
                                                           const float* Wemb, int E, const float* Wout, int V, int H, int k, int R,
                                                           float* dscores, int lds, float* dO, int ldo)
{
    __shared__ float part[4][kTopkFeedMax];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int id[kTopkFeedMax];
    float dl[kTopkFeedMax];
#pragma unroll
    for (int j = 0; j < kTopkFeedMax; ++j) { id[j] = j < k ? ids[(size_t)r * k + j] : 0; dl[j] = 0.f; }
    for (int e = tid; e < E; e += 256) {
        const float d = dx[(size_t)r * lddx + e];
#pragma unroll
        for (int j = 0; j < kTopkFeedMax; ++j)
            if (j < k) dl[j] += d * Wemb[(size_t)id[j] * E + e];
    }
#pragma unroll
    for (int j = 0; j < kTopkFeedMax; ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dl[j] += __shfl_xor(dl[j], o, 64);
        if (lane == 0) part[wv][j] = dl[j];
    }
    __syncthreads();
    float g = 0.f;
#pragma unroll
    for (int j = 0; j < kTopkFeedMax; ++j) {
        dl[j] = (part[0][j] + part[1][j]) + (part[2][j] + part[3][j]);
        if (j < k) g += wts[(size_t)r * k + j] * dl[j];
    }
    const float sum = S[r];
#pragma unroll
    for (int j = 0; j < kTopkFeedMax; ++j) dl[j] = (dl[j] - g) / sum;
    if (tid < k) {
        float mine = 0.f; int col = 0;
#pragma unroll
        for (int j = 0; j < kTopkFeedMax; ++j)
            if (j == tid) { mine = dl[j]; col = id[j]; }
        dscores[(size_t)r * lds + col] += mine;
    }
    if (!dO) return;
    for (int h = tid; h < H; h += 256) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < kTopkFeedMax; ++j)
            if (j < k) acc += dl[j] * Wout[(size_t)h * V + id[j]];
        dO[(size_t)r * ldo + h] += acc;
    }
}

hipError_t launch_topk_mix_bwd(const float* dx, int lddx, const int32_t* ids, const float* wts, const float* S, const float* Wemb, int E,
                               const float* Wout, int V, int H, int k, int R, float* dscores, int lds, float* dO, int ldo, hipStream_t st)
{
    if (R <= 0) return hipSuccess;
    hipLaunchKernelGGL(topk_mix_bwd_kernel, dim3(R), dim3(256), 0, st, dx, lddx, ids, wts, S, Wemb, E, Wout, V, H, k, R, dscores, lds, dO, ldo);
    return hipGetLastError();
}

// dW[ids[r][j]] += w[r][j] * dE[r] for j < k: scatter_add_rows2_kernel (train.hip) with k ids and a weight per id; one wave per row
__global__ __launch_bounds__(256) void scatter_add_rowsk_kernel(const float* dE, int ld, const int32_t* ids, const float* wts, int k, int R, int E,
                                                                float* dW, int ldw)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    for (int e = threadIdx.x & 63; e < E; e += 64) {
        const float v = dE[(size_t)r * ld + e];
        for (int j = 0; j < k; ++j) atomicAdd(dW + (size_t)ids[(size_t)r * k + j] * ldw + e, wts[(size_t)r * k + j] * v);
    }
}

hipError_t launch_scatter_add_rowsk(const float* dE, int ld, const int32_t* ids, const float* wts, int k, int R, int E, float* dW, int ldw,
                                    hipStream_t st)
{
    if (R <= 0) return hipSuccess;
    hipLaunchKernelGGL(scatter_add_rowsk_kernel, dim3((R + 3) / 4), dim3(256), 0, st, dE, ld, ids, wts, k, R, E, dW, ldw);
    return hipGetLastError();
}

}  // namespace s2vt

using namespace s2vt;

namespace {

// before the generator's step 0: the rows' video ids, sample id -1 (the pick launches draw no noise) and Wemb[1] as every row's operand
__global__ __launch_bounds__(256) void topk_decode_open_kernel(const float* Wemb, int B, int V, int E, int32_t* vid, int32_t* sid, float* X)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int bos = V > 1 ? 1 : 0;
    if (i < (size_t)B) { vid[i] = (int32_t)i; sid[i] = -1; }
    if (i < (size_t)B * E) X[i] = Wemb[(size_t)bos * E + i % E];
}

// The generator's workspace: the sampler's for B rows (encode half, LSTM2 state ping-pong, packed picks), then the step's operand, mix,
// logits (when the caller keeps none) and probabilities, and the emitted words of the step
struct TopkDecodeWs { SampleWs w; float* X; int32_t* ids; float *wts, *sums, *logits, *probs; int32_t* emit; };
size_t carve_topk_decode(Carver& c, const s2vt_dims* d, int B, int k, TopkDecodeWs* out)
{
    TopkDecodeWs t;
    carve_sample(c, d, B, B, &t.w);
    t.X = c.take<float>((size_t)B * d->word_dim);
    t.ids = c.take<int32_t>((size_t)B * k);
    t.wts = c.take<float>((size_t)B * k);
    t.sums = c.take<float>(B);
    t.logits = c.take<float>((size_t)B * d->n_words);
    t.probs = c.take<float>((size_t)B * d->n_words);
    t.emit = c.take<int32_t>(B);
    if (out) *out = t;
    return c.off;
}
bool decode_k_ok(const s2vt_dims* d, int k) { return k >= 1 && k <= kTopkFeedMax && k <= d->n_words; }

}  // namespace

extern "C" {

int s2vt_topk_mix_fwd(const float* logits, int32_t ld, const float* plane, int32_t ldp, int32_t weights_mode, int32_t R, int32_t V, int32_t k,
                      const float* Wemb, int32_t E, int32_t* ids, float* w, float* score_sum, float* x, int32_t ldx, s2vt_stream stream)
{
    if (!Wemb || !ids || !w || !score_sum || !x || R < 0 || V <= 0 || E <= 0 || ldx < E || k < 1 || k > kTopkFeedMax || k > V)
        return S2VT_E_BADARG;
    if (weights_mode == 0 ? (!logits || plane || ld < V) : (weights_mode != 1 || !plane || ldp < V)) return S2VT_E_BADARG;
    HIP_TRY(launch_topk_mix_fwd(weights_mode ? plane : logits, weights_mode ? ldp : ld, R, V, k, Wemb, E, ids, w, score_sum, x, ldx, nullptr,
                                S(stream)));
    return S2VT_OK;
}

int s2vt_topk_mix_bwd(const float* dx, int32_t lddx, const int32_t* ids, const float* w, const float* score_sum, const float* Wemb, int32_t E,
                      const float* Wout, int32_t V, int32_t H, int32_t k, int32_t R, float* dscores, int32_t lds, float* dO, int32_t ldo,
                      s2vt_stream stream)
{
    if (!dx || !ids || !w || !score_sum || !Wemb || !dscores || R < 0 || V <= 0 || E <= 0 || lddx < E || lds < V || k < 1 || k > kTopkFeedMax || k > V)
        return S2VT_E_BADARG;
    if (dO && (!Wout || H <= 0 || ldo < H)) return S2VT_E_BADARG;
    HIP_TRY(launch_topk_mix_bwd(dx, lddx, ids, w, score_sum, Wemb, E, Wout, V, H, k, R, dscores, lds, dO, ldo, S(stream)));
    return S2VT_OK;
}

int s2vt_embed_scatter_addk(const float* dE, int32_t ld, const int32_t* ids, const float* w, int32_t k, int32_t R, int32_t E, float* dWemb,
                            s2vt_stream stream)
{
    if (!dE || !ids || !w || !dWemb || R < 0 || E <= 0 || ld < E || k < 1 || k > kTopkFeedMax) return S2VT_E_BADARG;
    HIP_TRY(launch_scatter_add_rowsk(dE, ld, ids, w, k, R, E, dWemb, E, S(stream)));
    return S2VT_OK;
}

size_t s2vt_topk_feed_decode_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t k)
{
    if (!dims_ok(d) || B <= 0 || !decode_k_ok(d, k)) return 0;
    Carver c(nullptr, 0);
    return carve_topk_decode(c, d, B, k, nullptr);
}

int s2vt_topk_feed_decode(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t k, int32_t weights_mode,
                          int32_t unshifted_softmax, int32_t* ids_out, float* logits_out, void* workspace, size_t workspace_bytes,
                          s2vt_stream stream)
{
    if (!dims_ok(d) || !sampler_params_ok(p) || !video || !ids_out || !workspace || B <= 0 || !decode_k_ok(d, k)) return S2VT_E_BADARG;
    if (weights_mode < 0 || weights_mode > 1 || unshifted_softmax < 0 || unshifted_softmax > 1 || (weights_mode == 1 && !unshifted_softmax))
        return S2VT_E_BADARG;                                                                  // (the probability plane is the unshifted softmax's)
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    if (chain_fault()) return S2VT_E_CHAIN_TIMEOUT;
    Carver c(workspace, workspace_bytes);
    TopkDecodeWs x;
    carve_topk_decode(c, d, B, k, &x);
    if (!c.ok()) return S2VT_E_WORKSPACE;
    const SampleWs& w = x.w;
    const int H = d->lstm_dim, E = d->word_dim, V = d->n_words, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step;
    const size_t BH = (size_t)B * H, enc = (size_t)Tv * BH;
    hipStream_t st = S(stream);
    {
        const int rc = sample_encode(d, p, video, B, w, stream);
        if (rc != S2VT_OK) return rc;
    }
    {
        ZeroList z;
        z.add(w.packed, (size_t)Tc * B * kPickStride * 8);
        HIP_TRY(launch_zero_regions(z, st));
        const size_t n = (size_t)B * (E > 1 ? E : 1);
        hipLaunchKernelGGL(topk_decode_open_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p->Wemb, B, V, E, w.vid, w.sid, x.X);
        HIP_TRY(hipGetLastError());
    }
    const NoiseIds none{nullptr, nullptr, 0}, argmax{w.vid, w.sid, 0};
    for (int t = 0; t < Tc; ++t) {
        // the cell on [out1 ; x ; h2]: the hoisted out1 partial, the step's mix as a dense operand at kw = H, then h2 at kw = H + E
        const int nxt = (t + 1) & 1;
        const float* const c_prev = t == 0 ? w.c2e + enc : w.c2[t & 1];
        const float* const h_prev = t == 0 ? w.h2e + enc : w.h2[t & 1];
        ASeg s2[2] = {make_seg(x.X, E, E, H), make_seg(h_prev, H, H, H + E)};
        HIP_TRY(lstm_call(s2, 2, p->lstm2_W, p->lstm2_b, c_prev, 0, w.c2[nxt], w.h2[nxt], nullptr, nullptr, B, H, 1.0f, none, 0, -1, st,
                          w.P2 + (size_t)(Tv + t) * 4 * BH, 4 * H, 0));
        float* const lt = logits_out ? logits_out + (size_t)t * B * V : x.logits;
        HIP_TRY(pick_call(w.h2[nxt], H, p->embed_word_W, p->embed_word_b, B, H, V, argmax, t, w.packed + (size_t)t * B * kPickStride, lt, -1, st,
                          kPickStride));
        if (unshifted_softmax) HIP_TRY(launch_softmax_unshifted_argmax(lt, V, B, V, x.emit, x.probs, st));
        const TopkStep ts{nullptr, nullptr, B, Tc, t, 0.0f, ids_out, nullptr, nullptr, unshifted_softmax ? x.emit : nullptr};
        const bool more = t + 1 < Tc;
        HIP_TRY(launch_topk_mix_fwd(weights_mode ? x.probs : lt, V, B, V, k, p->Wemb, E, more ? x.ids : nullptr, more ? x.wts : nullptr,
                                    more ? x.sums : nullptr, more ? x.X : nullptr, E, &ts, st));
    }
    return S2VT_OK;
}

}  // extern "C"
