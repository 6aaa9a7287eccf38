// api.hip -- extern "C" boundary of libs2vt_hip.so (declared in include/s2vt.h) and the on-device
// drivers of the S2VT sampler: the workspace carve (carve_sample_enc, carve_sample), the encode half (sample_encode), the
// LSTM2 decode step shared with the beam search (lstm2_step) and the decode driver over the stages of SampleDecode
// (sample_decode).  Everything here is host code + a few trivial helper kernels; the contraction kernels live in
// gemm_mfma.h / fwd.hip.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "api_util.h"

namespace s2vt_api {
std::atomic<int> g_last_hip{0};
}
using namespace s2vt_api;

namespace {

__global__ void math_eval_kernel(int fn, const float* x, float* y, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    y[i] = fn == 0 ? dm_expf(v) : fn == 1 ? dm_logf(v) : fn == 2 ? dm_tanhf(v) : dm_sigmoidf(v);
}

__global__ void gumbel_eval_kernel(uint32_t lo, uint32_t hi, uint32_t video, uint32_t sample, uint32_t step, float* out,
                                   int V)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < V) out[n] = gumbel_at(lo, hi, video, sample, step, (uint32_t)n);
}

__global__ void gumbel_words_eval_kernel(const uint32_t* words, float* exact, float* fast, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t w = words[i];
    exact[i] = gumbel_from_word(w);
    fast[i] = gumbel_fast_from_word(w);
}

__global__ void fill_i32_kernel(int32_t* p, int32_t v, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// row ids of the sampler: row r = k*B + j -> video video_base + j, sample k (greedy block: -1)
__global__ void sampler_rows_kernel(int32_t* vid, int32_t* sid, int B, int K, int R, int video_base)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R) return;
    vid[i] = video_base + i % B;
    sid[i] = (i / B) < K ? i / B : -1;
}

// packed [T][R] (entries `stride` words apart) -> ids [R][T].  A word that was never written (stop-at-<eos> mode: the row had
// left the loop) reads as <eos> = 0.
__global__ void unpack_ids_kernel(const unsigned long long* packed, int32_t* ids, int R, int T, int stride)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R * T) return;
    const int m = i / T, t = i % T;
    const unsigned long long w = packed[((size_t)t * R + m) * stride];
    ids[i] = w ? (int32_t)(~(uint32_t)w) : 0;
}

// mixed mode: the word every row is fed at step t >= 1 -- its own pick of step t - 1 (decoded as unpack_ids_kernel does), or, for the
// rows [mix_lo, mix_lo + B) whose coin says so, the ground-truth word caption[b][t - 1] clamped into [0, V)
__global__ __launch_bounds__(256) void mix_words_kernel(const unsigned long long* picked, int stride, const int32_t* caption, int Tc, int t,
                                                        int mix_lo, int B, int R, int V, int video_base, uint32_t seed_lo, uint32_t seed_hi,
                                                        float p_gt, int32_t* word)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const unsigned long long w = picked[(size_t)r * stride];
    int32_t id = w ? (int32_t)(~(uint32_t)w) : 0;
    const int b = r - mix_lo;
    if (b >= 0 && b < B && mix_feeds_truth(seed_lo, seed_hi, (uint32_t)(video_base + b), 0u, (uint32_t)t, p_gt)) {
        const int32_t c = caption[(size_t)b * Tc + t - 1];
        id = c < 0 ? 0 : c >= V ? V - 1 : c;
    }
    word[r] = id;
}

// stop-at-<eos> mode: the rows still sampling at step t from those of step t - 1 and the words they just picked (a row leaves
// once it has picked <eos> = 0; order preserved).  One workgroup; step 0: every row.
__global__ __launch_bounds__(256) void live_rows_kernel(const unsigned long long* picked, int stride, const int32_t* prev, const int32_t* nprev,
                                                        int32_t* next, int32_t* nnext, int R)
{
    __shared__ int cnt[256];
    __shared__ int base;
    const int tid = threadIdx.x;
    if (!picked) {                                              // step 0
        for (int i = tid; i < R; i += 256) next[i] = i;
        if (tid == 0) *nnext = R;
        return;
    }
    const int n = *nprev;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int i = c0 + tid;
        int row = -1, alive = 0;
        if (i < n) {
            row = prev[i];
            alive = (uint32_t)(~(uint32_t)picked[(size_t)row * stride]) != 0u;
        }
        cnt[tid] = alive;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {                     // inclusive scan
            const int v = tid >= o ? cnt[tid - o] : 0;
            __syncthreads();
            cnt[tid] += v;
            __syncthreads();
        }
        if (alive) next[base + cnt[tid] - 1] = row;
        __syncthreads();
        if (tid == 255) base += cnt[255];
        __syncthreads();
    }
    if (tid == 0) *nnext = base;
}

}  // namespace

extern "C" {

int s2vt_version(void) { return 100; }

int s2vt_zero_regions(void* const* ptrs, const size_t* bytes, int32_t count, s2vt_stream stream)
{
    if (count < 0 || count > 8 || (count && (!ptrs || !bytes))) return S2VT_E_BADARG;
    ZeroList z;
    for (int i = 0; i < count; ++i) {
        if (bytes[i] & 3u) return S2VT_E_BADARG;
        if (ptrs[i] && (reinterpret_cast<uintptr_t>(ptrs[i]) & 3u)) return S2VT_E_ALIGN;
        z.add(ptrs[i], bytes[i]);
    }
    HIP_TRY(launch_zero_regions(z, S(stream)));
    return S2VT_OK;
}
int s2vt_last_hip_error(void) { return g_last_hip.load(); }

const char* s2vt_error_string(int code)
{
    switch (code) {
        case S2VT_OK: return "ok";
        case S2VT_E_BADARG: return "bad argument";
        case S2VT_E_ALIGN: return "workspace not 256-byte aligned";
        case S2VT_E_WORKSPACE: return "workspace too small";
        case S2VT_E_HIP: return "HIP error (see s2vt_last_hip_error)";
        case S2VT_E_CHAIN_TIMEOUT: return "a persistent recurrence timed out (GPU shared with another persistent kernel?): results since are suspect, updates were skipped; s2vt_chain_ack() and repeat";
        default: return "unknown error";
    }
}

int s2vt_prof_enable(int on)
{
    prof_enable(on != 0);
    return S2VT_OK;
}

int s2vt_prof_filter(int kernel_class, int tile_cfg)
{
    prof_filter(kernel_class, tile_cfg);
    return S2VT_OK;
}

int s2vt_prof_collect(s2vt_prof_row* rows, int max_rows)
{
    if (!rows || max_rows <= 0) return S2VT_E_BADARG;
    ProfRow tmp[64];
    const int n = prof_collect(tmp, max_rows < 64 ? max_rows : 64);
    for (int i = 0; i < n; ++i) {
        rows[i].kernel_class = tmp[i].cls; rows[i].tile_cfg = tmp[i].cfg; rows[i].launches = tmp[i].launches;
        rows[i].total_ms = tmp[i].ms; rows[i].total_flops = tmp[i].flops;
        std::strncpy(rows[i].name, tmp[i].name, sizeof(rows[i].name) - 1);
        rows[i].name[sizeof(rows[i].name) - 1] = 0;
    }
    return n;
}

int s2vt_math_eval(int fn, const float* x, float* y, int64_t n, s2vt_stream stream)
{
    if (!x || !y || n < 0 || fn < 0 || fn > 3) return S2VT_E_BADARG;
    if (n == 0) return S2VT_OK;
    hipLaunchKernelGGL(math_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), fn, x, y, n);
    HIP_TRY(hipGetLastError());
    return S2VT_OK;
}

// C = act([segs] @ W + bias) continuing Cinit; W as [k][n] rows (ldw >= N) or, w_transposed, as [n][k] rows (ldw >= the segments' K)
static int gemm_impl(const s2vt_operand* segs, int32_t nseg, const float* W, int32_t ldw, const float* bias, const float* Cinit,
                     int32_t ldcinit, float* C, int32_t ldc, int32_t M, int32_t N, int32_t act_tanh, int32_t tile_cfg,
                     s2vt_stream stream, bool w_transposed, const int32_t* live = nullptr, const int32_t* n_live = nullptr)
{
    if (!segs || nseg < 1 || nseg > 3 || !W || !C || M < 0 || N <= 0 || ldc < N || (!w_transposed && ldw < N)) return S2VT_E_BADARG;
    if (Cinit && ldcinit < N) return S2VT_E_BADARG;
    ASeg a[3];
    int kw = 0;
    for (int i = 0; i < nseg; ++i) {
        if (segs[i].k < 0 || (segs[i].ptr && segs[i].ld < segs[i].k)) return S2VT_E_BADARG;
        seg_from_operand(a[i], &segs[i], kw);
        kw += segs[i].k;
    }
    if (w_transposed && ldw < kw) return S2VT_E_BADARG;
    if (M == 0) return S2VT_OK;
    HIP_TRY(store_call(a, nseg, W, ldw, bias, C, ldc, M, N, act_tanh ? 1 : 0, tile_cfg, S(stream), Cinit, ldcinit, w_transposed, live, n_live));
    return S2VT_OK;
}

int s2vt_gemm_nt(const s2vt_operand* segs, int32_t nseg, const float* Wt, int32_t ldw, const float* bias, const float* Cinit,
                 int32_t ldcinit, float* C, int32_t ldc, int32_t M, int32_t N, int32_t act_tanh, int32_t tile_cfg,
                 s2vt_stream stream)
{
    return gemm_impl(segs, nseg, Wt, ldw, bias, Cinit, ldcinit, C, ldc, M, N, act_tanh, tile_cfg, stream, true);
}

int s2vt_gumbel_eval(uint64_t seed, int32_t video, int32_t sample, int32_t step, float* out, int32_t V, s2vt_stream stream)
{
    if (!out || V <= 0) return S2VT_E_BADARG;
    hipLaunchKernelGGL(gumbel_eval_kernel, dim3((V + 255) / 256), dim3(256), 0, S(stream), (uint32_t)seed,
                       (uint32_t)(seed >> 32), (uint32_t)video, (uint32_t)sample, (uint32_t)step, out, V);
    HIP_TRY(hipGetLastError());
    return S2VT_OK;
}

int s2vt_gumbel_words_eval(const uint32_t* words, float* exact, float* fast, int64_t n, s2vt_stream stream)
{
    if (!words || !exact || !fast || n < 0 || n > (int64_t)0x7fffffff * 256) return S2VT_E_BADARG;
    if (n == 0) return S2VT_OK;
    hipLaunchKernelGGL(gumbel_words_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), words, exact, fast, n);
    HIP_TRY(hipGetLastError());
    return S2VT_OK;
}

int s2vt_gemm(const s2vt_operand* segs, int32_t nseg, const float* W, int32_t ldw, const float* bias, const float* Cinit,
              int32_t ldcinit, float* C, int32_t ldc, int32_t M, int32_t N, int32_t act_tanh, int32_t tile_cfg,
              s2vt_stream stream)
{
    return gemm_impl(segs, nseg, W, ldw, bias, Cinit, ldcinit, C, ldc, M, N, act_tanh, tile_cfg, stream, false);
}

// ---- the live-row forms of the single-op calls (GemmArgs::omap / m_dev): what the early-exit samplers launch, one launch at a time
int s2vt_gemm_live(const s2vt_operand* segs, int32_t nseg, const float* W, int32_t ldw, const float* bias, const float* Cinit,
                   int32_t ldcinit, float* C, int32_t ldc, int32_t M, int32_t N, int32_t act_tanh, const int32_t* live,
                   const int32_t* n_live, int32_t tile_cfg, s2vt_stream stream)
{
    if (!live && !n_live) return S2VT_E_BADARG;
    return gemm_impl(segs, nseg, W, ldw, bias, Cinit, ldcinit, C, ldc, M, N, act_tanh, tile_cfg, stream, false, live, n_live);
}

// res != NULL: the residual form, out[m] = dropout(h'[m]) + res[row(m)]
static int lstm_cell_impl(const s2vt_operand* x0, const s2vt_operand* x1, const float* h_prev, const float* c_prev,
                          int32_t state_rowmod, const float* W, const float* b, float* c_new, float* h_new, float* out,
                          float* gates, int32_t M, int32_t H, float keep, uint64_t seed, const int32_t* video_id,
                          const int32_t* sample_id, uint32_t drop_code, int32_t tile_cfg, s2vt_stream stream, const s2vt_operand* res,
                          const int32_t* live = nullptr, const int32_t* n_live = nullptr)
{
    if (!h_prev || !c_prev || !W || !b || !c_new || !h_new || M < 0 || H <= 0) return S2VT_E_BADARG;
    if (keep < 1.0f && (!video_id || !sample_id || !out || !(keep > 0.0f))) return S2VT_E_BADARG;
    ASeg a[3];
    int kw = 0, n = 0;
    const s2vt_operand* xs[2] = {x0, x1};
    for (int i = 0; i < 2; ++i) {
        if (!xs[i]) continue;
        if (xs[i]->k < 0 || (xs[i]->ptr && xs[i]->ld < xs[i]->k)) return S2VT_E_BADARG;
        seg_from_operand(a[n++], xs[i], kw);
        kw += xs[i]->k;
    }
    a[n++] = make_seg(h_prev, H, H, kw, state_rowmod);
    if (M == 0) return S2VT_OK;
    NoiseIds ids{video_id, sample_id, seed};
    ASeg r;
    if (res) seg_from_operand(r, res, 0);
    HIP_TRY(lstm_call(a, n, W, b, c_prev, state_rowmod, c_new, h_new, out, gates, M, H, keep, ids, drop_code, tile_cfg,
                      S(stream), nullptr, 0, 0, live, n_live, res ? &r : nullptr));
    return S2VT_OK;
}

int s2vt_lstm_cell_fwd(const s2vt_operand* x0, const s2vt_operand* x1, const float* h_prev, const float* c_prev,
                       int32_t state_rowmod, const float* W, const float* b, float* c_new, float* h_new, float* out,
                       float* gates, int32_t M, int32_t H, float keep, uint64_t seed, const int32_t* video_id,
                       const int32_t* sample_id, uint32_t drop_code, int32_t tile_cfg, s2vt_stream stream)
{
    return lstm_cell_impl(x0, x1, h_prev, c_prev, state_rowmod, W, b, c_new, h_new, out, gates, M, H, keep, seed, video_id, sample_id, drop_code,
                          tile_cfg, stream, nullptr);
}

int s2vt_lstm_cell_fwd_res(const s2vt_operand* x0, const s2vt_operand* x1, const float* h_prev, const float* c_prev,
                           int32_t state_rowmod, const float* W, const float* b, const s2vt_operand* res, float* c_new, float* h_new,
                           float* out, float* gates, int32_t M, int32_t H, float keep, uint64_t seed, const int32_t* video_id,
                           const int32_t* sample_id, uint32_t drop_code, int32_t tile_cfg, s2vt_stream stream)
{
    if (!res || !res->ptr || !out || res->k != H || res->ld < H || res->rowmod < 0) return S2VT_E_BADARG;
    return lstm_cell_impl(x0, x1, h_prev, c_prev, state_rowmod, W, b, c_new, h_new, out, gates, M, H, keep, seed, video_id, sample_id, drop_code,
                          tile_cfg, stream, res);
}

int s2vt_lstm_cell_fwd_live(const s2vt_operand* x0, const s2vt_operand* x1, const float* h_prev, const float* c_prev,
                            int32_t state_rowmod, const float* W, const float* b, const s2vt_operand* res, float* c_new, float* h_new,
                            float* out, float* gates, int32_t M, int32_t H, float keep, uint64_t seed, const int32_t* video_id,
                            const int32_t* sample_id, uint32_t drop_code, const int32_t* live, const int32_t* n_live, int32_t tile_cfg,
                            s2vt_stream stream)
{
    if (!live && !n_live) return S2VT_E_BADARG;
    if (res && (!res->ptr || !out || res->k != H || res->ld < H || res->rowmod < 0)) return S2VT_E_BADARG;
    return lstm_cell_impl(x0, x1, h_prev, c_prev, state_rowmod, W, b, c_new, h_new, out, gates, M, H, keep, seed, video_id, sample_id, drop_code,
                          tile_cfg, stream, res, live, n_live);
}

// ---- the gathered-state form of the cell (GemmArgs::cinit_rowidx / cprev_rowidx): what the bidirectional beam step launches
int s2vt_lstm_cell_fwd_gather(const s2vt_operand* x0, const s2vt_operand* x1, const float* h_prev, const float* c_prev,
                              const int32_t* state_rowidx, const float* Cinit, int32_t ldcinit, const int32_t* cinit_rowidx, const float* W,
                              const float* b, float* c_new, float* h_new, float* gates, int32_t M, int32_t H, int32_t tile_cfg,
                              s2vt_stream stream)
{
    if (!h_prev || !c_prev || !W || !b || !c_new || !h_new || M < 0 || H <= 0) return S2VT_E_BADARG;
    if (Cinit && ldcinit < 4 * H) return S2VT_E_BADARG;
    if (state_rowidx && (c_new == c_prev || h_new == h_prev)) return S2VT_E_BADARG;   // another workgroup owns the source row: in place is a race
    ASeg a[3];
    int kw = 0, n = 0;
    const s2vt_operand* xs[2] = {x0, x1};
    for (int i = 0; i < 2; ++i) {
        if (!xs[i]) continue;
        if (xs[i]->k < 0 || (xs[i]->ptr && xs[i]->ld < xs[i]->k)) return S2VT_E_BADARG;
        seg_from_operand(a[n++], xs[i], kw);
        kw += xs[i]->k;
    }
    a[n++] = make_seg(h_prev, H, H, kw, 0, state_rowidx);
    if (M == 0) return S2VT_OK;
    // no index at all: the plain twin (same bits); an index on either operand: the GS twin, whose other index may be NULL
    HIP_TRY(lstm_call(a, n, W, b, c_prev, 0, c_new, h_new, nullptr, gates, M, H, 1.0f, NoiseIds{nullptr, nullptr, 0}, 0u, tile_cfg, S(stream), Cinit,
                      Cinit ? ldcinit : 0, 0, nullptr, nullptr, nullptr, Cinit ? cinit_rowidx : nullptr, state_rowidx));
    return S2VT_OK;
}

int s2vt_vocab_pick(const float* out2, int32_t ld, const float* W, const float* b, int32_t M, int32_t H, int32_t V,
                    const int32_t* video_id, const int32_t* sample_id, int32_t step, uint64_t seed,
                    unsigned long long* packed, int32_t* tokens_out, float* logits_out, int32_t tile_cfg,
                    s2vt_stream stream)
{
    if (!out2 || !W || !b || !video_id || !sample_id || !packed || M < 0 || H <= 0 || V <= 0 || ld < H)
        return S2VT_E_BADARG;
    if (M == 0) return S2VT_OK;
    NoiseIds ids{video_id, sample_id, seed};
    HIP_TRY(pick_call(out2, ld, W, b, M, H, V, ids, step, packed, logits_out, tile_cfg, S(stream)));
    if (tokens_out) {
        hipLaunchKernelGGL(unpack_ids_kernel, dim3((M + 255) / 256), dim3(256), 0, S(stream), packed, tokens_out, M, 1, 1);
        HIP_TRY(hipGetLastError());
    }
    return S2VT_OK;
}

int s2vt_vocab_pick_live(const float* out2, int32_t ld, const float* W, const float* b, int32_t M, int32_t H, int32_t V,
                         const int32_t* video_id, const int32_t* sample_id, int32_t step, uint64_t seed, unsigned long long* packed,
                         int32_t pick_stride, float* logits_out, const int32_t* live, const int32_t* n_live, int32_t tile_cfg,
                         s2vt_stream stream)
{
    if (!out2 || !W || !b || !video_id || !sample_id || !packed || M < 0 || H <= 0 || V <= 0 || ld < H || pick_stride < 1 || (!live && !n_live))
        return S2VT_E_BADARG;
    if (M == 0) return S2VT_OK;
    NoiseIds ids{video_id, sample_id, seed};
    HIP_TRY(pick_call(out2, ld, W, b, M, H, V, ids, step, packed, logits_out, tile_cfg, S(stream), pick_stride, live, n_live));
    return S2VT_OK;
}

// the tile tables of fwd.hip as a caller of the tile_cfg arguments sees them
static bool tile_kind_ok(int kind) { return kind == EPI_STORE || kind == EPI_LSTM || kind == EPI_PICK || kind == EPI_STORE_NT; }

int s2vt_tile_count(int kind) { return tile_kind_ok(kind) ? gemm_num_cfgs(kind) : S2VT_E_BADARG; }

int s2vt_tile_info(int kind, int tile_cfg, s2vt_tile_desc* out)
{
    GemmCfgInfo g;
    if (!out || !tile_kind_ok(kind) || !gemm_cfg_info(kind, tile_cfg, &g)) return S2VT_E_BADARG;
    std::memset(out, 0, sizeof(*out));
    out->rows = g.BM; out->cols = g.CG; out->fallback = g.fallback; out->has_scalar = g.has_scalar; out->has_live = g.has_live;
    std::strncpy(out->name, g.name, sizeof(out->name) - 1);
    return S2VT_OK;
}

int s2vt_frame_embed_fwd(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, float* emb,
                         s2vt_stream stream)
{
    if (!dims_ok_res(d) || !p || !p->encode_image_W || !p->encode_image_b || !video || !emb || B < 0) return S2VT_E_BADARG;   // (no logits here: the variants agree)
    if (B == 0) return S2VT_OK;
    ASeg a = make_seg(video, d->dim_image, d->dim_image, 0);
    HIP_TRY(store_call(&a, 1, p->encode_image_W, d->word_dim, p->encode_image_b, emb, d->word_dim,
                       B * d->n_video_lstm_step, d->word_dim, 0, -1, S(stream)));
    return S2VT_OK;
}

// ---------------------------------------------------------------------------------------------
// samplers
// ---------------------------------------------------------------------------------------------
}  // extern "C"

namespace s2vt_api {

hipError_t launch_live_rows(const unsigned long long* picked, int stride, const int32_t* prev, const int32_t* nprev, int32_t* next,
                            int32_t* nnext, int R, hipStream_t st)
{
    hipLaunchKernelGGL(live_rows_kernel, dim3(1), dim3(256), 0, st, picked, stride, prev, nprev, next, nnext, R);
    return hipGetLastError();
}

// The sampler's environment switches, read once per process.  (decode_loop.hip and decode4.hip read the two forms' own switches.)
struct SamplerKnobs {
    bool frag_small;              // S2VT_DECLOOP unset or >= 1: the fragment-order operands are carved at <= 64 rows
    bool frag_big;                // S2VT_DECLOOP >= 2 or S2VT_DEC4=1: also at 257-384 rows
    int eos_lstm_cfg, eos_pick_cfg;   // dev knobs: tiles of the early-exit mode's launches (S2VT_EOS_LSTM_CFG, default kLstm[4] = gw32x16u; S2VT_EOS_PICK_CFG)
};
const SamplerKnobs& sampler_knobs()
{
    static const SamplerKnobs k = [] {
        const char* loop = getenv("S2VT_DECLOOP"); const char* dec4 = getenv("S2VT_DEC4");
        const char* lc = getenv("S2VT_EOS_LSTM_CFG"); const char* pc = getenv("S2VT_EOS_PICK_CFG");
        return SamplerKnobs{!loop || atoi(loop) >= 1, (loop && atoi(loop) >= 2) || (dec4 && dec4[0] == '1'), lc ? atoi(lc) : 4, pc ? atoi(pc) : -1};
    }();
    return k;
}

// The eight regions of the encode half: they depend on B only and lead the sampler's and the beam search's workspaces.
void carve_sample_enc(Carver& c, const s2vt_dims* d, int B, SampleEnc& e)
{
    const size_t H = d->lstm_dim, E = d->word_dim, Tv = d->n_video_lstm_step, T = Tv + d->n_caption_lstm_step;
    e.emb = c.take<float>((size_t)B * Tv * E);
    e.Xp1 = c.take<float>((size_t)B * Tv * 4 * H);
    e.c1 = c.take<float>((T + 1) * B * H); e.h1 = c.take<float>((T + 1) * B * H);     // LSTM1 state history, slot 0 = zeros
    e.G1 = c.take<float>(T * B * 4 * H);                                                // LSTM1 activated gates (reused by the update pass)
    e.P2 = c.take<float>(T * B * 4 * H);                                                // h1[t+1] @ W2[0:H] for every step
    e.c2e = c.take<float>((Tv + 1) * (size_t)B * H); e.h2e = c.take<float>((Tv + 1) * (size_t)B * H);
}

// Workspace of one sampler pass: the encode half, then what depends on the number of decode rows R.
size_t carve_sample(Carver& c, const s2vt_dims* d, int B, int R, SampleWs* w)
{
    const size_t H = d->lstm_dim, E = d->word_dim, Tc = d->n_caption_lstm_step;
    SampleWs t;
    carve_sample_enc(c, d, B, t);
    for (int i = 0; i < 2; ++i) { t.c2[i] = c.take<float>((size_t)R * H); t.h2[i] = c.take<float>((size_t)R * H); }
    t.packed = c.take<unsigned long long>((size_t)Tc * R * kPickStride);
    t.vid = c.take<int32_t>(R); t.sid = c.take<int32_t>(R); t.bos = c.take<int32_t>(R);
    t.chain_sync = c.take<unsigned>(kChainSyncBytes / 4);
    t.chain_abuf = c.take<float>(chain_scratch_floats((int)H));
    t.wemb_p = t.w2_p = t.himg[0] = t.himg[1] = nullptr;
    // fragment-order operands of the persistent decode loop (decode_loop.hip: default at <= 64 rows; S2VT_DECLOOP=2 / S2VT_DEC4=1 also at
    // 257-384 rows, where both forms measured no gain) -- sized by the shape and the two opt-in switches, never by the device: every caller of the
    // size query sees the same carve.  (24.6 + 40 MB of packed operands at the bench dimensions: not taken at 384 rows unless asked for.)
    const SamplerKnobs& k = sampler_knobs();
    if (((R <= 64 && k.frag_small) || (R > 256 && R <= 384 && k.frag_big)) && (H & 3) == 0 && H >= 132 &&
        (size_t)d->n_words * ((E + 15) / 16 * 16) * 4 < (1ull << 31)) {
        Dec4Geom q;
        decode4_geometry(R, (int)H, (int)E, &q);
        t.wemb_p = c.take<float>((size_t)d->n_words * q.erow);
        t.w2_p = c.take<float>((size_t)q.ncg * 4 * q.ngt * 256);
        for (int i = 0; i < 2; ++i) t.himg[i] = c.take<float>((size_t)q.img_tiles * q.hgp * 256);
    }
    t.live[0] = c.take<int32_t>(R); t.live[1] = c.take<int32_t>(R); t.nlive = c.take<int32_t>(Tc + 1);
    // residual model: the one block it adds, behind every region of the plain carve (callers that re-carve to find LSTM1's history see
    // the same offsets either way)
    t.out2 = is_residual(d) ? c.take<float>((size_t)R * H) : nullptr;
    if (w) *w = t;
    return c.off;
}

hipError_t lstm_recurrence(const float* W, int kw0, const float* bias, const float* cinit, long long cinit_tstride, int ldcinit,
                           int cinit_steps, float* C, float* Hh, size_t state_tstride, float* gates, size_t gates_tstride,
                           float* out, size_t out_tstride, int M, int H, int T, float keep, const NoiseIds& ids,
                           uint32_t drop_code0, float* chain_abuf, unsigned* chain_sync, hipStream_t st, const int32_t* perm, const int32_t* nlive)
{
    if (chain_abuf && chain_sync && chain_eligible(M, H) && chain_operands_ok(W, 4 * H, chain_abuf)) {    // (unaligned W: per-step launches)
        ChainArgs a;
        std::memset(&a, 0, sizeof(a));
        a.W = W; a.ldw = 4 * H; a.kw0 = kw0; a.bias = bias;
        a.cinit = cinit; a.cinit_tstride = cinit_tstride; a.ldcinit = ldcinit; a.cinit_steps = cinit_steps;
        a.h0 = Hh; a.c0 = C; a.C = C; a.Hh = Hh; a.state_tstride = state_tstride;
        a.gates = gates; a.gates_tstride = gates_tstride; a.out = out; a.out_tstride = out_tstride;
        a.M = M; a.H = H; a.T = T; a.keep = keep;
        a.seed_lo = (uint32_t)ids.seed; a.seed_hi = (uint32_t)(ids.seed >> 32); a.drop_code0 = drop_code0;
        a.video_id = ids.video_id; a.sample_id = ids.sample_id;
        a.abuf = chain_abuf; a.sync = chain_sync;
        a.perm = perm; a.nlive = nlive;                        // (forms that cannot skip rows run dense: the same results)
        return launch_lstm_chain(a, st);
    }
    for (int t = 0; t < T; ++t) {
        ASeg s1 = make_seg(Hh + (size_t)t * state_tstride, H, H, kw0);
        hipError_t e = lstm_call(&s1, 1, W, bias, C + (size_t)t * state_tstride, 0, C + (size_t)(t + 1) * state_tstride,
                                 Hh + (size_t)(t + 1) * state_tstride, out ? out + (size_t)t * out_tstride : nullptr,
                                 gates ? gates + (size_t)t * gates_tstride : nullptr, M, H, keep, ids, drop_code0 + (uint32_t)t, -1, st,
                                 (cinit && t < cinit_steps) ? cinit + (long long)t * cinit_tstride : nullptr, ldcinit, 0);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// Encoding stage (tf_s2vt.py:97-122) plus everything of the decoding stage that does not depend on a
// sampled word: frame embedding, the whole LSTM1 trajectory, its products with the out1 rows of W2, LSTM2 over
// the Tv frames.  Leaves the encoder state in slot Tv of w.c2e / w.h2e.
int sample_encode(const s2vt_dims* d, const s2vt_params* p, const float* video, int B, const SampleEnc& w, s2vt_stream stream)
{
    const int H = d->lstm_dim, E = d->word_dim, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step;
    hipStream_t st = S(stream);
    const int T = Tv + Tc;
    const size_t BH = (size_t)B * H;
    // zero initial states (tf_s2vt.py:105-107)
    {
        ZeroList z;
        z.add(w.c1, BH * 4); z.add(w.h1, BH * 4); z.add(w.c2e, BH * 4); z.add(w.h2e, BH * 4);
        HIP_TRY(launch_zero_regions(z, st));
    }
    int rc = s2vt_frame_embed_fwd(d, p, video, B, w.emb, stream);
    if (rc != S2VT_OK) return rc;

    NoiseIds none{nullptr, nullptr, 0};
    // Each cell product is the ascending-k chain of concat([x, h]) @ W (tf_s2vt.py:119-143).  The rows of W
    // that multiply inputs known before the step are consumed first, batched over time; the per-step
    // launch continues the chain from that partial with the rows whose inputs the step produces.
    // ---- LSTM1: sees the frames, then only the zero padding and its own state -- never a sampled word,
    // so its whole trajectory (Tv + Tc steps) is per VIDEO and runs first, on B rows.
    {
        ASeg sx = make_seg(w.emb, E, E, 0);
        HIP_TRY(store_call(&sx, 1, p->lstm1_W, 4 * H, nullptr, w.Xp1, 4 * H, B * Tv, 4 * H, 0, -1, st));
    }
    // (one persistent launch for the whole trajectory when B <= 64: chain.hip)
    HIP_TRY(lstm_recurrence(p->lstm1_W, E, p->lstm1_b, w.Xp1, (size_t)4 * H, Tv * 4 * H, Tv, w.c1, w.h1, BH, w.G1, (size_t)4 * BH,
                            nullptr, 0, B, H, T, 1.0f, none, 0, w.chain_abuf, w.chain_sync, st));
    // ---- the out1 rows of W2 for every step at once (M = T*B)
    {
        ASeg so = make_seg(w.h1 + BH, H, H, 0);
        HIP_TRY(store_call(&so, 1, p->lstm2_W, 4 * H, nullptr, w.P2, 4 * H, T * B, 4 * H, 0, -1, st));
    }
    // ---- LSTM2 encoding stage (tf_s2vt.py:122: word slot = zero padding), M = B: the chain continues from the out1 partial
    HIP_TRY(lstm_recurrence(p->lstm2_W, H + E, p->lstm2_b, w.P2, (size_t)4 * BH, 4 * H, Tv, w.c2e, w.h2e, BH, nullptr, 0, nullptr, 0, B, H, Tv,
                            1.0f, none, 0, w.chain_abuf, w.chain_sync, st));
    return S2VT_OK;
}

// The chain of the cell on [out1 ; word ; h2] continues the hoisted out1 partial (W2 rows 0:H) with the word's rows
// of Wemb at kw = H, then h2 at kw = H + E.
hipError_t lstm2_step(const Lstm2Step& s, hipStream_t st)
{
    const NoiseIds none{nullptr, nullptr, 0};
    ASeg s2[2] = {make_seg(s.p->Wemb, s.E, s.E, s.H, 0, s.word_idx, s.word_key, s.word_key ? kPickStride : 1),
                  make_seg(s.h_prev, s.H, s.H, s.H + s.E, s.state_rowmod)};
    const ASeg res = make_seg(s.out1, s.H, s.H, 0, s.out1_rowmod, s.out1_rowidx);
    return lstm_call(s2, 2, s.p->lstm2_W, s.p->lstm2_b, s.c_prev, s.state_rowmod, s.c_new, s.h_new, s.out, nullptr, s.M, s.H, 1.0f, none, 0,
                     s.lstm_cfg, st, s.partial, 4 * s.H, s.partial_rowmod, s.live, s.n_live, s.out ? &res : nullptr);
}

// (inside a stage: hand a failed launch's error to the driver, whose HIP_TRY records it)
#define HIP_CHECK(expr) do { const hipError_t _e = (expr); if (_e != hipSuccess) return _e; } while (0)

// One decode call of the sampler: R rows = K multinomial row blocks, then (mixed mode) one argmax block fed ground-truth words by coin, then
// (with_greedy) one argmax block, row r of video r % B.  The
// workspace may be carved for more rows than the call decodes (session API): whether the fragment-order operands exist follows the
// carve, every stride, grid and eligibility test the R of the call.  The stages are straight-line.
struct SampleDecode {
    const s2vt_params* p; const SampleWs& w;
    int B, K, R; uint64_t seed; int video_base; bool stop_at_eos; hipStream_t st;
    int H, E, V, Tv, Tc;
    size_t BH, enc;          // enc: where sample_encode left the encoder state, slot Tv of the c2e / h2e history
    Dec4Geom q4;
    const SampleMix* mix = nullptr;   // mixed mode: the argmax block at rows [K B, K B + B) is fed ground-truth words by coin
    const PickScreenWs* screen = nullptr;   // s2vt_sample_screened: the pick of step_launches is the screened one (pick_screen.hip), same packed picks

    unsigned long long* picks(int t) const { return w.packed + (size_t)t * R * kPickStride; }     // the packed picks of step t [R]
    const float* partial(int t) const { return w.P2 + (size_t)(Tv + t) * 4 * BH; }                // the out1 partial of step t [B][4H]
    NoiseIds ids() const { return NoiseIds{w.vid, w.sid, seed}; }

    hipError_t open()
    {
        ZeroList z;
        z.add(w.packed, (size_t)Tc * R * kPickStride * 8);
        HIP_CHECK(launch_zero_regions(z, st));
        hipLaunchKernelGGL(sampler_rows_kernel, dim3((R + 255) / 256), dim3(256), 0, st, w.vid, w.sid, B, K, R, video_base);
        hipLaunchKernelGGL(fill_i32_kernel, dim3((R + 255) / 256), dim3(256), 0, st, w.bos, 1, R);   // <bos> = 1
        return hipGetLastError();
    }
    // the fragment-order operands (decode4.hip), packed once per call: same chain, same bits
    hipError_t pack_fragments()
    {
        decode4_geometry(R, H, E, &q4);
        HIP_CHECK(decode4_pack(p->Wemb, p->lstm2_W, V, H, E, q4, w.wemb_p, w.w2_p, st));
        HIP_CHECK(decode4_state_to_image(w.h2e + enc, B, R, H, q4, w.himg[0], st));
        return hipMemsetAsync(w.himg[1], 0, (size_t)q4.img_tiles * q4.hgp * 1024, st);
    }
    // all Tc steps -- LSTM2, vocabulary logits, pick -- in one persistent launch (decode_loop.hip)
    hipError_t persistent_loop()
    {
        DecLoopLaunch a;
        std::memset(&a, 0, sizeof(a));
        a.wemb_p = w.wemb_p; a.w2_p = w.w2_p; a.bias2 = p->lstm2_b;
        a.P2 = partial(0); a.p2_tstride = (size_t)4 * BH; a.ldp2 = 4 * H; a.B = B;
        a.c0 = w.c2e + enc;
        a.himg0 = w.himg[0]; a.himg1 = w.himg[1];
        a.packed = w.packed; a.pick_stride = kPickStride;
        a.Wout = p->embed_word_W; a.ldwo = V; a.bout = p->embed_word_b;
        a.seed = seed; a.video_base = video_base; a.noise_rows = K * B;
        a.R = R; a.H = H; a.E = E; a.V = V; a.Tc = Tc;
        a.sync = w.chain_sync;
        return launch_decode_loop(a, q4, st);
    }
    // step t with the LSTM2 cell on the fragment-order operands (decode4.hip), then the pick
    hipError_t step_fragment(int t)
    {
        const int nxt = (t + 1) & 1;
        Dec4Launch a;
        std::memset(&a, 0, sizeof(a));
        a.wemb_p = w.wemb_p; a.w2_p = w.w2_p; a.bias = p->lstm2_b;
        a.cinit = partial(t); a.ldcinit = 4 * H; a.cinit_rowmod = B;
        a.tok = t == 0 ? nullptr : picks(t - 1); a.tok_stride = kPickStride; a.tok_const = 1;     // <bos> = 1
        a.himg_in = w.himg[t & 1]; a.himg_out = w.himg[nxt];
        a.c_prev = t == 0 ? w.c2e + enc : w.c2[t & 1]; a.cprev_rowmod = t == 0 ? B : 0;
        a.c_new = w.c2[nxt]; a.h_new = w.h2[nxt];
        a.R = R; a.H = H; a.E = E; a.V = V;
        HIP_CHECK(launch_decode_lstm4(a, q4, st));
        return pick_call(w.h2[nxt], H, p->embed_word_W, p->embed_word_b, R, H, V, ids(), t, picks(t), nullptr, -1, st, kPickStride);
    }
    // mixed mode, t >= 1: the words step t is fed, chosen per row between its pick of step t - 1 and the ground-truth caption
    hipError_t mix_words(int t)
    {
        hipLaunchKernelGGL(mix_words_kernel, dim3((R + 255) / 256), dim3(256), 0, st, picks(t - 1), kPickStride, mix->caption, Tc, t, K * B, B, R, V,
                           video_base, (uint32_t)seed, (uint32_t)(seed >> 32), mix->p_gt, mix->word);
        return hipGetLastError();
    }
    // step t as two launches of the contraction kernel: the LSTM2 cell, then the pick.  Stop-at-<eos> mode: both cover the rows still
    // sampling (compact index -> row through the live list, their number on the device); a finished row's state stays where it is,
    // nothing reads it again, its later words are never written (= <eos>)
    hipError_t step_launches(int t)
    {
        const int nxt = (t + 1) & 1;
        Lstm2Step s{};
        s.p = p; s.M = R; s.H = H; s.E = E;
        s.partial = partial(t); s.partial_rowmod = B;
        if (t == 0) { s.word_idx = w.bos; s.c_prev = w.c2e + enc; s.h_prev = w.h2e + enc; s.state_rowmod = B; }
        else {
            if (mix) { HIP_CHECK(mix_words(t)); s.word_idx = mix->word; }
            else s.word_key = picks(t - 1);
            s.c_prev = w.c2[t & 1]; s.h_prev = w.h2[t & 1];
        }
        s.c_new = w.c2[nxt]; s.h_new = w.h2[nxt];
        s.lstm_cfg = -1;
        int pick_cfg = -1;
        if (stop_at_eos) {
            // tiles for a launch whose live-row count only the device knows: small row tiles cost a few % while every row is live
            // and follow the count down afterwards
            // -- measured at R = 384, mean length 7 (tools/eos_sweep.sh): cell step on 32-row tiles 2.40 ms per sampler call against 2.79
            // with the tile the full row count would get (96 rows) and 3.32 for the loop that never stops; the pick's 64 x 96 tile stays
            if (R > 64) s.lstm_cfg = sampler_knobs().eos_lstm_cfg;
            pick_cfg = sampler_knobs().eos_pick_cfg;
            HIP_CHECK(launch_live_rows(t == 0 ? nullptr : picks(t - 1), kPickStride, w.live[nxt], w.nlive + (t > 0 ? t - 1 : 0), w.live[t & 1], w.nlive + t, R, st));
            s.live = w.live[t & 1]; s.n_live = w.nlive + t;
        }
        // residual model: the cell launch also writes out1 + h' (out1 = slot Tv + t + 1 of LSTM1's history, row % B), and the pick reads that
        if (w.out2) { s.out = w.out2; s.out1 = w.h1 + (size_t)(Tv + t + 1) * BH; s.out1_rowmod = B; }
        HIP_CHECK(lstm2_step(s, st));
        if (screen) return launch_pick_screen_step(w.h2[nxt], H, p->embed_word_W, p->embed_word_b, R, H, V, w.vid, w.sid, seed, t, picks(t), kPickStride, *screen, st);
        return pick_call(w.out2 ? w.out2 : w.h2[nxt], H, p->embed_word_W, p->embed_word_b, R, H, V, ids(), t, picks(t), nullptr, pick_cfg, st, kPickStride, s.live, s.n_live);
    }
};

// Decoding stage (tf_s2vt.py:126-153 as specialised by the samplers): LSTM2 + vocab at M = R rows; the R rows of a video share its
// out1 partial (row % B).  Needs sample_encode's results in the same workspace.  The driver picks one of three forms -- the persistent
// launch (<= 64 rows), per-step launches on the fragment-order operands (257-384 rows, opt-in), per-step launches of the contraction
// kernel -- and leaves through the one unpack.  The early-exit mode takes the last form only: the other two cannot skip rows.  So does the
// mixed mode (one more argmax block in front of the greedy one): the other two read the fed word from the packed picks.  The residual
// model (w.out2) takes the last form too: the other two project h2, not out1 + h2 (extending them is open).
int sample_decode(const s2vt_dims* d, const s2vt_params* p, int B, int K, int with_greedy, uint64_t seed, int video_base,
                  int32_t* ids_out, const SampleWs& w, s2vt_stream stream, int stop_at_eos, const SampleMix* mix, const PickScreenWs* screen)
{
    const int H = d->lstm_dim, E = d->word_dim, V = d->n_words, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step;
    const int R = (K + (mix ? 1 : 0) + (with_greedy ? 1 : 0)) * B;
    hipStream_t st = S(stream);
    SampleDecode s{p, w, B, K, R, seed, video_base, stop_at_eos != 0, st, H, E, V, Tv, Tc, (size_t)B * H, (size_t)Tv * B * H, {}, mix, screen};
    HIP_TRY(s.open());
    if (screen) HIP_TRY(launch_pick_screen_prepare(p->embed_word_W, H, V, *screen, st));      // embed_word_W is constant over the Tc steps
    const bool loop1 = !screen && !stop_at_eos && !mix && !w.out2 && w.wemb_p && (B & 15) == 0 && decode_loop_eligible(R, H, E, V) && chain_operands_ok(p->embed_word_W, V, w.himg[0]);
    const bool dec4 = !screen && !stop_at_eos && !mix && !w.out2 && (loop1 || (w.wemb_p && decode4_eligible(R, H, E)));
    if (dec4) HIP_TRY(s.pack_fragments());
    if (loop1) {
        HIP_TRY(s.persistent_loop());
    } else {
        for (int t = 0; t < Tc; ++t) HIP_TRY(dec4 ? s.step_fragment(t) : s.step_launches(t));
    }
    hipLaunchKernelGGL(unpack_ids_kernel, dim3((R * Tc + 255) / 256), dim3(256), 0, st, w.packed, ids_out, R, Tc, kPickStride);
    HIP_TRY(hipGetLastError());
    return S2VT_OK;
}

bool sampler_params_ok(const s2vt_params* p)
{
    return p && p->Wemb && p->encode_image_W && p->encode_image_b && p->lstm1_W && p->lstm1_b && p->lstm2_W && p->lstm2_b &&
           p->embed_word_W && p->embed_word_b;
}

}  // namespace s2vt_api

extern "C" {

int s2vt_build_flags(void)
{
    return 1;       // bit 0: the fragment-order decode kernels (decode4.hip, decode_loop.hip) are in this library (always, since round 6)
}

size_t s2vt_sample_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t K, int32_t with_greedy)
{
    if (!dims_ok_res(d) || B <= 0 || K < 0) return 0;
    Carver c(nullptr, 0);
    return carve_sample(c, d, B, (K + (with_greedy ? 1 : 0)) * B, nullptr);
}

int s2vt_sample_ex(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t K, int32_t with_greedy,
                   uint64_t seed, int32_t video_base, int32_t flags, int32_t* ids_out, void* workspace, size_t workspace_bytes,
                   s2vt_stream stream)
{
    if (!dims_ok_res(d) || !sampler_params_ok(p) || !video || !ids_out || !workspace || B <= 0 || K < 0 || (K == 0 && !with_greedy) || (flags & ~1))
        return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    if (chain_fault()) return S2VT_E_CHAIN_TIMEOUT;
    const int R = (K + (with_greedy ? 1 : 0)) * B;
    Carver c(workspace, workspace_bytes);
    SampleWs w;
    carve_sample(c, d, B, R, &w);
    if (!c.ok()) return S2VT_E_WORKSPACE;
    int rc = sample_encode(d, p, video, B, w, stream);
    if (rc != S2VT_OK) return rc;
    return sample_decode(d, p, B, K, with_greedy, seed, video_base, ids_out, w, stream, flags & S2VT_SAMPLE_STOP_AT_EOS);
}

int s2vt_sample(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t K, int32_t with_greedy,
                uint64_t seed, int32_t video_base, int32_t* ids_out, void* workspace, size_t workspace_bytes,
                s2vt_stream stream)
{
    return s2vt_sample_ex(d, p, video, B, K, with_greedy, seed, video_base, 0, ids_out, workspace, workspace_bytes, stream);
}

// ---- the screened form of s2vt_sample (pick_screen.hip).  Its scratch is a block of its own: the sampler workspace and its carve stay as
// they are (train.hip and session.hip carve it again).
static bool pick_screen_enabled()
{
    static const bool on = [] { const char* e = getenv("S2VT_PICK_SCREEN"); return !(e && e[0] == '0'); }();
    return on;
}

// head block (counters, nwmax), W^T planes, W^T in fp32, row planes, approximate logits; 0: the path does not serve the shape
static size_t carve_pick_screen(Carver& c, const s2vt_dims* d, int R, PickScreenWs* s)
{
    const size_t H = d->lstm_dim, V = d->n_words, Hp = bf16_pad((int)H), ldl = (V + 3) & ~(size_t)3, ldt = (H + 3) & ~(size_t)3;
    if (R <= 64 || H > (size_t)kPickScreenMaxH) return 0;                 // <= 64 rows: the persistent decode loop's shapes
    PickScreenWs t;
    char* head = c.take<char>(kPickScreenHeadBytes);
    t.counters = reinterpret_cast<unsigned long long*>(head);
    t.nwmax = reinterpret_cast<float*>(head ? head + 16 : nullptr);
    t.Wh = c.take<uint16_t>(V * Hp); t.Wl = c.take<uint16_t>(V * Hp);
    t.Wt = c.take<float>(V * ldt);
    t.hh = c.take<uint16_t>((size_t)R * Hp); t.hl = c.take<uint16_t>((size_t)R * Hp);
    t.L = c.take<float>((size_t)R * ldl);
    t.Hp = (int)Hp; t.ldl = (int)ldl; t.ldt = (int)ldt;
    if (s) *s = t;
    return c.off;
}

size_t s2vt_sample_screen_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t K, int32_t with_greedy)
{
    if (!dims_ok(d) || B <= 0 || K < 0 || !pick_screen_enabled()) return 0;
    if ((long long)(K + (with_greedy ? 1 : 0)) * B > 0x7fffffffll) return 0;
    const int R = (K + (with_greedy ? 1 : 0)) * B;
    if (sampler_knobs().frag_big && R > 256 && R <= 384) return 0;       // the opt-in fragment-order forms were asked for: they keep the call
    Carver c(nullptr, 0);
    return carve_pick_screen(c, d, R, nullptr);
}

int s2vt_sample_screened(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t K, int32_t with_greedy,
                         uint64_t seed, int32_t video_base, int32_t* ids_out, void* workspace, size_t workspace_bytes, void* screen_ws,
                         size_t screen_bytes, s2vt_stream stream)
{
    if (!dims_ok(d) || !sampler_params_ok(p) || !video || !ids_out || !workspace || !screen_ws || B <= 0 || K < 0 || (K == 0 && !with_greedy))
        return S2VT_E_BADARG;
    if (s2vt_sample_screen_workspace_bytes(d, B, K, with_greedy) == 0) return S2VT_E_BADARG;      // not a call this path serves
    if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(screen_ws)) & 255u) return S2VT_E_ALIGN;
    if (chain_fault()) return S2VT_E_CHAIN_TIMEOUT;
    const int R = (K + (with_greedy ? 1 : 0)) * B;
    Carver c(workspace, workspace_bytes), cs(screen_ws, screen_bytes);
    SampleWs w;
    PickScreenWs sw;
    carve_sample(c, d, B, R, &w);
    carve_pick_screen(cs, d, R, &sw);
    if (!c.ok() || !cs.ok()) return S2VT_E_WORKSPACE;
    int rc = sample_encode(d, p, video, B, w, stream);
    if (rc != S2VT_OK) return rc;
    return sample_decode(d, p, B, K, with_greedy, seed, video_base, ids_out, w, stream, 0, nullptr, &sw);
}

// mixed sampler: carve_sample for R = (1 + with_greedy) * B rows, then the fed words [R]
static size_t carve_sample_mix(Carver& c, const s2vt_dims* d, int B, int R, SampleWs* w, SampleMix* m)
{
    carve_sample(c, d, B, R, w);
    int32_t* word = c.take<int32_t>(R);
    if (m) m->word = word;
    return c.off;
}

size_t s2vt_sample_mix_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t with_greedy)
{
    if (!dims_ok(d) || B <= 0) return 0;
    Carver c(nullptr, 0);
    return carve_sample_mix(c, d, B, (1 + (with_greedy ? 1 : 0)) * B, nullptr, nullptr);
}

int s2vt_sample_mix(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, const int32_t* caption, float p_gt,
                    int32_t with_greedy, uint64_t seed, int32_t video_base, int32_t* ids_out, void* workspace, size_t workspace_bytes,
                    s2vt_stream stream)
{
    if (!dims_ok(d) || !sampler_params_ok(p) || !video || !caption || !ids_out || !workspace || B <= 0 || !(p_gt >= 0.0f && p_gt <= 1.0f))
        return S2VT_E_BADARG;                                                     // (a NaN p_gt fails both comparisons)
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    if (chain_fault()) return S2VT_E_CHAIN_TIMEOUT;
    Carver c(workspace, workspace_bytes);
    SampleWs w;
    SampleMix m{caption, p_gt, nullptr};
    carve_sample_mix(c, d, B, (1 + (with_greedy ? 1 : 0)) * B, &w, &m);
    if (!c.ok()) return S2VT_E_WORKSPACE;
    int rc = sample_encode(d, p, video, B, w, stream);
    if (rc != S2VT_OK) return rc;
    return sample_decode(d, p, B, 0, with_greedy, seed, video_base, ids_out, w, stream, 0, &m);
}

}  // extern "C"
