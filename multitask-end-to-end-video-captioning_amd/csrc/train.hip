// train.hip -- extern "C" entry points of the update half of the step: teacher-forced unroll with
// saved activations (build_model / build_loss), softmax-NLL forward+backward (XE and the
// reward-scaled policy-gradient NLL), back-propagation through time, gradient finalisation,
// global-norm clip + TF-form Adam.
#include <hip/hip_runtime.h>

#include <functional>
#include <mutex>

#include <cstdlib>

#include "api_util.h"

using namespace s2vt_api;

namespace s2vt_api {
// An optional second stream for the backward pass: the recurrences (25 dependent steps of small kernels, ~half the
// matrix pipes idle) run on the caller's stream while weight-gradient contractions that do not depend on them
// run here, forked / joined with events so the call keeps its stream semantics.  Created once per process.
// (mode 1: S2VT_OVERLAP=1, ungated, below; 2: gated overlap with the persistent backward recurrences, round 5)
// One per DEVICE (the first version was a process-wide static created on whichever device was current at first use -- a second model
// on another GPU then recorded / waited on device 0's events): indexed by hipGetDevice like chain.hip's per-device state, each entry created on
// first use with its device current.  A device index beyond the table, or a creation failure, yields the one-stream entry (ok = false).
SideStream& side_stream()
{
    constexpr int kMaxDev = 32;
    static SideStream table[kMaxDev];
    static bool made[kMaxDev] = {};
    static SideStream none;                              // ok = false, mode 0
    static const int mode = [] {
        // Mode 1 (S2VT_OVERLAP=1, ungated).  Measured on MI355X: the two streams do run concurrently, but the kernels
        // only slow each other down (TN 724 -> 1462 us, slab GEMM 28 -> 46 us per launch) for a net 0.1 ms of
        // 15.6, and per-launch durations stop meaning anything for the roofline.
        // Mode 2 (round 5, the default; S2VT_OVERLAP=0 switches it off): the weight-gradient contractions that do not feed a recurrence run
        // on the side stream BESIDE the persistent backward recurrence they are independent of -- dWout beside LSTM2's, LSTM2's three beside
        // LSTM1's -- released by a gate once the recurrence's grid is resident (internal.h ChainGate).  A persistent recurrence at <= 256 rows
        // is one wave per SIMD at <= 380 VGPRs that waits in hand-offs half the time; the contraction fills the other half of the pipe.
        const char* on = getenv("S2VT_OVERLAP");
        const int m = on ? atoi(on) : 2;
        return (m < 1 || m > 2) ? 0 : m;
    }();
    int dev = -1;
    if (mode == 0 || hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return none;
    std::lock_guard<std::mutex> lk(side_stream_mutex());
    if (!made[dev]) {
        made[dev] = true;
        SideStream& t = table[dev];
        t.mode = mode;
        bool good = hipStreamCreateWithFlags(&t.s, hipStreamNonBlocking) == hipSuccess;
        for (auto& e : t.ev)
            good = good && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        t.ok = good;
    }
    return table[dev];
}
// side waits for everything issued so far on `from`
hipError_t fork_to(hipStream_t from, hipStream_t to, hipEvent_t ev)
{
    hipError_t e = hipEventRecord(ev, from);
    return e != hipSuccess ? e : hipStreamWaitEvent(to, ev, 0);
}
std::mutex& side_stream_mutex()
{
    static std::mutex mu;
    return mu;
}
}  // namespace s2vt_api

namespace {

__global__ void enc_index_kernel(int32_t* idx, int B, int Tv)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * Tv) return;
    const int t = i / B, j = i % B;
    idx[i] = j * Tv + t;     // row of video[B*Tv, d] / emb[B*Tv, E] feeding (step t, video j)
}

// Saved activations + backward scratch of one teacher-forced unroll, carved from the caller's buffer.
// LSTM1 never sees the caption (its input is the frame embedding, then the zero padding), so its clean
// state trajectory is per VIDEO: it is computed and back-propagated on B rows, and only its
// dropout-wrapped output O1 is expanded to the N = rep*B sample rows.
struct TrainWs {
    float *emb, *Xp1;
    int32_t *prev, *tgt, *encidx;
    float *G1, *C1, *H1, *O1, *G2, *C2, *H2, *O2;
    float *dO2, *dZ1, *dZ2, *dX2, *dX1, *dH1, *slab, *dc;
    int32_t* decidx;     // inverse of encidx: row of dX1 (time-major) for row j*Tv + t of d_video
    float* chain_abuf;   // persistent-recurrence scratch (chain.hip)
    unsigned* chain_sync;
    float *bimg, *bex;   // persistent BACKWARD recurrence scratch (chain.hip): dz images, partial-tile exchange
    unsigned* bsync;
    float* dO2s;         // split-K slabs of dO2 = dlogits @ Wout^T when it has few rows (NULL otherwise)
    size_t dO2s_rows;    // ... rows x slabs it holds
    float* dO2p;         // dO2 of the LIVE rows only (the *_live entry points), scattered into dO2
    float *dZ2p, *dX2p;  // the live decode rows of dZ2 (packed copy) and of dX2 (computed packed, scattered into dX2)
    int32_t* prevp;      // previous word of the live decode rows
    int32_t *perm, *nlive;   // live rows in the recurrences (chain_live_capable shapes): LSTM2's rows by length, live rows per step
    size_t dXs_floats;   // capacity of dXs
    float* dXs;          // split-K slabs of dX2 / dX1 when they are short of tiles (NULL otherwise)
};

// Split-K plan of the recurrent data-gradient product dz[M,4H] @ Whh^T[4H,H] (order-free): enough K slabs
// that the launch has >= ~512 workgroups of the 64x32 tile; the slabs are summed by the next step's
// pointwise kernel.
constexpr int kMaxSlabs = 16;
// dO2 = dlogits[Tc N, V] @ Wout^T -> [Tc N, H] has K = |V| = 12000 but, at N = 64, only 1280 x 1000 outputs: as 64x32 tiles with
// the whole K each it ran 80 TFLOP/s (12 % of the XE step).  Order-free, so up to this many rows it is cut into K slabs
// and the slabs are summed.
constexpr int kDo2SplitRows = 2048, kDo2Slabs = 12;
int do2_splits(int rows, int H, int V)
{
    static const int cap = [] { const char* e = getenv("S2VT_DO2_SPLITS"); const int v = e ? atoi(e) : kDo2Slabs; return v < 1 ? 1 : (v > kDo2Slabs ? kDo2Slabs : v); }();   // dev knob
    if (rows > kDo2SplitRows || (H & 3)) return 1;
    return slab_splits(rows, H, V, cap);
}
struct SlabPlan { int splits, kper, nslab; };
SlabPlan slab_plan(int M, int H)
{
    const int K = 4 * H;
    static const int want = [] { const char* e = getenv("S2VT_SLAB_WGS"); return e ? atoi(e) : 512; }();     // dev knob
    static const int tn_ = [] { const char* e = getenv("S2VT_SLAB_TILE_N"); return e ? atoi(e) : 32; }();   // dev knob (columns of the tile nn_bwd will get)
    const long tiles = (long)((M + 63) / 64) * ((H + tn_ - 1) / tn_);
    int splits = (int)((want + tiles - 1) / tiles);
    if (splits < 1) splits = 1;
    if (splits > kMaxSlabs) splits = kMaxSlabs;
    SlabPlan p;
    p.kper = ((K + splits - 1) / splits + BK - 1) / BK * BK;      // what nn_bwd computes from `splits`
    p.nslab = (K + p.kper - 1) / p.kper;
    p.splits = splits;
    return p;
}

// scratch of the persistent backward recurrence for any row count up to Mmax (the one- and two-part forms lay it out differently)
void bwd_scratch_max(int H, int Mmax, size_t* imgf, size_t* exf, size_t* syncb)
{
    *imgf = *exf = *syncb = 0;
    for (int m : {64, 128, 256, 384}) {
        size_t a, b, s;
        bwd_chain_scratch(H, Mmax < m ? Mmax : m, &a, &b, &s);
        if (a > *imgf) *imgf = a;
        if (b > *exf) *exf = b;
        if (s > *syncb) *syncb = s;
    }
}

size_t carve_train(Carver& c, const s2vt_dims* d, int B, int N, TrainWs* out)
{
    const size_t H = d->lstm_dim, E = d->word_dim, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step;
    const size_t T = Tv + Tc, n = N, b = B;
    TrainWs w;
    w.emb = c.take<float>(b * Tv * E);
    w.Xp1 = c.take<float>(b * Tv * 4 * H);
    w.prev = c.take<int32_t>(Tc * n); w.tgt = c.take<int32_t>(Tc * n); w.encidx = c.take<int32_t>(Tv * b);
    w.G1 = c.take<float>(T * b * 4 * H); w.C1 = c.take<float>((T + 1) * b * H); w.H1 = c.take<float>((T + 1) * b * H);
    w.O1 = c.take<float>(T * n * H);
    w.G2 = c.take<float>(T * n * 4 * H); w.C2 = c.take<float>((T + 1) * n * H); w.H2 = c.take<float>((T + 1) * n * H);
    w.O2 = c.take<float>(T * n * H);
    w.dO2 = c.take<float>(Tc * n * H);
    w.dO2p = c.take<float>(Tc * n * H);
    w.dZ2p = c.take<float>(Tc * n * 4 * H); w.dX2p = c.take<float>(Tc * n * (H + E)); w.prevp = c.take<int32_t>(Tc * n);
    w.dZ1 = c.take<float>(T * b * 4 * H); w.dZ2 = c.take<float>(T * n * 4 * H);
    w.dX2 = c.take<float>(T * n * (H + E)); w.dX1 = c.take<float>(Tv * b * E); w.dH1 = c.take<float>(T * b * H);
    w.slab = c.take<float>((size_t)kMaxSlabs * n * H); w.dc = c.take<float>(n * H);
    w.decidx = c.take<int32_t>(Tv * b);
    w.perm = c.take<int32_t>(n); w.nlive = c.take<int32_t>(T);
    w.chain_sync = c.take<unsigned>(kChainSyncBytes / 4);
    w.chain_abuf = c.take<float>(chain_scratch_floats((int)H));
    {
        size_t imgf, exf, syncb;
        bwd_scratch_max((int)H, N, &imgf, &exf, &syncb);       // (sized for the larger of the two recurrences: N >= B rows)
        w.bimg = c.take<float>(imgf); w.bex = c.take<float>(exf); w.bsync = c.take<unsigned>(syncb / 4);
    }
    // (a truncated unroll -- caption_steps < Tc, the *_steps entry points -- has fewer rows and may split where the full one
    //  does not: both scratch blocks are sized for the worst of all step counts)
    {
        size_t need = 0;
        for (size_t tc = 1; tc <= Tc; ++tc) {
            const int s2 = do2_splits((int)(tc * n), (int)H, d->n_words);
            if (s2 > 1 && (size_t)s2 * tc * n > need) need = (size_t)s2 * tc * n;
        }
        w.dO2s = need ? c.take<float>(need * H) : nullptr;
        w.dO2s_rows = need;
    }
    {
        size_t need = 0;
        for (size_t tc = 1; tc <= Tc; ++tc) {
            const int s2 = dx_splits((int)((Tv + tc) * n), (int)(H + E), (int)(4 * H));
            const size_t need2 = s2 > 1 ? (size_t)s2 * (Tv + tc) * n * (H + E) : 0;
            if (need2 > need) need = need2;
        }
        const int s1 = dx_splits((int)(Tv * b), (int)E, (int)(4 * H));
        const size_t need1 = s1 > 1 ? (size_t)s1 * Tv * b * E : 0;
        if (need1 > need) need = need1;
        w.dXs = need ? c.take<float>(need) : nullptr;
        w.dXs_floats = need;
    }
    if (out) *out = w;
    return c.off;
}

// Scratch of the bf16 mode of the backward (s2vt_bptt_bwd_bf16): bf16 copies of the operands of every gradient contraction, reused
// in stream order -- L: the left operand of a data-gradient product in row form (dlogits, dZ2, dZ1 rows); W: the weight it multiplies;
// BT / AT: both operands of a weight gradient transposed ([column][reduction row], the rows of two segments -- encode steps, decode
// steps -- each padded to the K step, so that a product over the decode steps only starts at a padded column); part: column-sum partials.
// Split mode (s2vt_bptt_bwd_split): the same four buffers hold the hi planes, followed by a copy of their whole region for the lo
// planes (lo of a hi pointer = that pointer + lo_delta elements), and kpart: gemm_bf16x3_nt's split-K slabs.  The fused form of the
// split mode (split_fused(), the default) keeps no transposed operand: BT stays unused and AT holds the A operand of a weight gradient by
// rows ([reduction row][bf16_pad(width + 1)], the encode rows followed by the decode rows) for gemm_bf16x3_tn, whose B operand is L.
// S2VT_SPLIT_FUSED=0 (read once): the transposed casts and gemm_bf16x3_nt for every product, dlogits always as fp32.
static bool split_fused()
{
    static const int on = [] { const char* e = getenv("S2VT_SPLIT_FUSED"); return e ? atoi(e) : 1; }();
    return on != 0;
}

struct Bf16Ws { uint16_t *L, *W, *AT, *BT; float* part; size_t lo_delta; float* kpart; size_t kpart_floats; };

size_t carve_bf16(Carver& c, const s2vt_dims* d, int B, int N, Bf16Ws* out, bool split = false)
{
    const size_t H = d->lstm_dim, E = d->word_dim, V = d->n_words, D = d->dim_image, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step;
    const size_t T = Tv + Tc;
    const size_t Kv = bf16_pad((int)V), K4 = bf16_pad((int)(4 * H)), Kr = bf16_pad((int)(Tc * N));
    const size_t ke = bf16_pad((int)(Tv * N)), Kt = ke + Kr;                                       // LSTM2: encode | decode
    const size_t ke1 = bf16_pad((int)(Tv * B)), K1 = ke1 + bf16_pad((int)(Tc * B));                // LSTM1: encode | decode
    auto mx = [](std::initializer_list<size_t> l) { size_t m = 0; for (size_t v : l) m = v > m ? v : m; return m; };
    Bf16Ws w;
    const size_t off0 = c.off;
    w.L = c.take<uint16_t>(mx({Tc * N * Kv, T * N * K4, Tv * B * K4}));
    w.W = c.take<uint16_t>(mx({H * Kv, (H + E) * K4, E * K4}));
    const bool fused = split && split_fused();
    const size_t Hp1 = bf16_pad((int)H + 1), Ep = bf16_pad((int)E);
    // (BT is carved in the fused form too, though nothing is written there: the scratch size is part of the interface -- callers and
    //  tests size buffers by "two planes of everything the bf16 mode holds" -- and S2VT_SPLIT_FUSED must not change it)
    w.BT = c.take<uint16_t>(mx({V * Kr, 4 * H * Kt, 4 * H * K1, E * ke1}));
    w.AT = c.take<uint16_t>(mx({H * Kr, H * Kt, E * Kr, E * ke1, H * K1, D * ke1, fused ? T * N * Hp1 : 0, fused ? Tc * N * Ep : 0}));
    w.lo_delta = 0; w.kpart = nullptr; w.kpart_floats = 0;
    if (split) {
        const size_t hi_bytes = c.off - off0;                    // (a multiple of 256: the lo region starts right behind)
        c.take<char>(hi_bytes);
        w.lo_delta = hi_bytes / sizeof(uint16_t);
        const int Re = (int)(Tv * N), Rr = (int)(Tc * N), Re1 = (int)(Tv * B);
        if (fused)                                               // (weight gradients: K-major, a bias row where one rides)
            w.kpart_floats = mx({gemm_bf16x3_part_floats((int)H + 1, (int)V, (int)Kr), gemm_bf16x3_part_floats(Rr, (int)H, (int)Kv),
                                 gemm_bf16x3_part_floats((int)H + 1, (int)(4 * H), bf16_pad((int)(T * N))),
                                 gemm_bf16x3_part_floats((int)E, (int)(4 * H), (int)Kr),
                                 gemm_bf16x3_part_floats((int)(T * N), (int)(H + E), (int)K4), gemm_bf16x3_part_floats(Re, (int)(H + E), (int)K4),
                                 gemm_bf16x3_part_floats(Rr, (int)(H + E), (int)K4)});
        else
        w.kpart_floats = mx({gemm_bf16x3_part_floats((int)H, (int)V, (int)Kr), gemm_bf16x3_part_floats(Rr, (int)H, (int)Kv),
                             gemm_bf16x3_part_floats((int)H, (int)(4 * H), (int)Kt), gemm_bf16x3_part_floats((int)E, (int)(4 * H), (int)Kr),
                             gemm_bf16x3_part_floats((int)(T * N), (int)(H + E), (int)K4), gemm_bf16x3_part_floats(Re, (int)(H + E), (int)K4),
                             gemm_bf16x3_part_floats(Rr, (int)(H + E), (int)K4), gemm_bf16x3_part_floats(Re1, (int)E, (int)K4),
                             gemm_bf16x3_part_floats((int)E, (int)(4 * H), (int)ke1), gemm_bf16x3_part_floats((int)H, (int)(4 * H), (int)K1),
                             gemm_bf16x3_part_floats((int)D, (int)E, (int)ke1)});
        w.kpart = c.take<float>(w.kpart_floats);
    }
    w.part = c.take<float>(mx({cast_tr_part_floats((int)Kr, (int)V), cast_tr_part_floats((int)(ke > Kr ? ke : Kr), (int)(4 * H)),
                               cast_tr_part_floats((int)(K1 - ke1 > ke1 ? K1 - ke1 : ke1), (int)(4 * H)), cast_tr_part_floats((int)ke1, (int)E)}));
    if (out) *out = w;
    return c.off;
}

bool params_ok(const s2vt_params* p)
{
    return p && p->Wemb && p->encode_image_W && p->encode_image_b && p->lstm1_W && p->lstm1_b && p->lstm2_W && p->lstm2_b &&
           p->embed_word_W && p->embed_word_b;
}

// Back-propagation through one cell's unroll: dZ[t] for t = T-1 .. 0.  ONE persistent launch when the shape fits
// (bwd_chain_eligible: M <= 128 rows by default), else per step {pointwise, split-K slabs of dz @ Whh^T summed by the next
// pointwise launch}.  dext: upstream gradient w.r.t. the (dropped) output of step t >= dext_t0.
struct BwdScratch { float* slab; float* dc; float* bimg; float* bex; unsigned* bsync; };
hipError_t lstm_recurrence_bwd(const float* W, int kw0, const float* gates, const float* C, const float* dext, size_t dext_tstride,
                               int ld_ext, int dext_t0, float* dZ, int M, int H, int T, float keep, uint64_t seed, uint32_t drop_code0,
                               const int32_t* video_id, const int32_t* sample_id, const BwdScratch& sc, int persistent, hipStream_t st,
                               const int32_t* perm = nullptr, const int32_t* nlive = nullptr, bool split = false,
                               const std::function<hipError_t(int)>* between = nullptr)
{
    // between: a graph with an edge from step t's dZ to step t - 1's upstream gradient (the top-k feed: dZ2[t] -> dx[t] -> dext[t - 1]).
    // The persistent chain cannot take such an edge, so the per-step form runs, and (*between)(t) is called behind step t's launches.
    const size_t MH = (size_t)M * H;
    const bool can = !between && sc.bimg && sc.bex && sc.bsync && bwd_chain_eligible(M, H) && !(reinterpret_cast<uintptr_t>(W) & 15);
    if (persistent == 1 && !can) return hipErrorInvalidValue;
    if (persistent == 1 || (persistent == -1 && can && bwd_chain_auto(M, H))) {
        BwdChainLaunch a;
        std::memset(&a, 0, sizeof(a));
        a.W = W; a.ldw = 4 * H; a.kw0 = kw0; a.gates = gates; a.gates_tstride = 4 * MH; a.C = C; a.state_tstride = MH;
        a.dext = dext; a.dext_tstride = dext_tstride; a.ld_ext = ld_ext; a.dext_t0 = dext_t0;
        a.dZ = dZ; a.dz_tstride = 4 * MH; a.M = M; a.H = H; a.T = T;
        a.keep = keep; a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.drop_code0 = drop_code0;
        a.video_id = video_id; a.sample_id = sample_id;
        a.img = sc.bimg; a.ex = sc.bex; a.sync = sc.bsync;
        a.perm = perm; a.nlive = nlive;
        a.split = split && bwd_chain_split_serves(M, H);      // (the other persistent forms have no split kernels: fp32 there)
        return launch_lstm_bwd_chain(a, st);
    }
    const SlabPlan sp = slab_plan(M, H);
    for (int t = T - 1; t >= 0; --t) {
        hipError_t e = launch_lstm_bwd_pointwise(gates + (size_t)t * 4 * MH, C + (t + 1) * MH, C + t * MH, t == T - 1 ? nullptr : sc.slab, sp.nslab, MH,
                                                 (dext && t >= dext_t0) ? dext + (size_t)(t - dext_t0) * dext_tstride : nullptr, ld_ext,
                                                 t == T - 1 ? nullptr : sc.dc, sc.dc, dZ + (size_t)t * 4 * MH, M, H, keep, seed, drop_code0 + (uint32_t)t,
                                                 video_id, sample_id, st);
        if (e != hipSuccess) return e;
        if (t > 0) {
            e = nn_bwd(dZ + (size_t)t * 4 * MH, 4 * H, W + (size_t)kw0 * 4 * H, 4 * H, sc.slab, H, M, H, 4 * H, sp.splits, MH, st);
            if (e != hipSuccess) return e;
            if (between && (e = (*between)(t)) != hipSuccess) return e;
        }
    }
    return hipSuccess;
}


// The stages of a training unroll that do not depend on a word, shared by the teacher-forced and the scheduled-sampling forward: the
// frame-gather index, zero initial states, frame embedding, LSTM1's whole trajectory of T steps on B rows (or its copy out of the sampler
// pass's workspace), its dropped output O1 for the N sample rows, and the out1 partials of LSTM2's Tv encode steps in G2.
int unroll_front(const s2vt_dims* d, const s2vt_params* p, const float* video, int B, int N, int T, float keep, uint64_t seed,
                 const int32_t* video_id, const int32_t* sample_id, const TrainWs& w, const void* sampler_workspace,
                 size_t sampler_workspace_bytes, int sampler_rows, s2vt_stream stream, bool encode_partials = true)
{
    const int H = d->lstm_dim, E = d->word_dim, Tv = d->n_video_lstm_step;
    const size_t NH = (size_t)N * H, BH = (size_t)B * H;
    hipStream_t st = S(stream);
    hipLaunchKernelGGL(enc_index_kernel, dim3((B * Tv + 255) / 256), dim3(256), 0, st, w.encidx, B, Tv);
    HIP_TRY(hipGetLastError());
    // zero initial states (tf_s2vt.py:105-107): slot 0 of the state histories
    {
        ZeroList z;
        if (!sampler_workspace) { z.add(w.C1, BH * 4); z.add(w.H1, BH * 4); }      // (taken whole from the sampler pass otherwise)
        z.add(w.C2, NH * 4); z.add(w.H2, NH * 4);
        HIP_TRY(launch_zero_regions(z, st));
    }
    if (!sampler_workspace) {                     // (with the sampler's workspace the frame embedding is taken from there too, below)
        int rc = s2vt_frame_embed_fwd(d, p, video, B, w.emb, stream);
        if (rc != S2VT_OK) return rc;
    }

    NoiseIds none{nullptr, nullptr, 0};
    // Every contraction below is the SAME ascending-k chain as concat([x, h]) @ W (tf_s2vt.py:119-143):
    // the rows of W that multiply non-recurrent inputs are consumed first, for all time steps in one
    // batched launch; the per-step launch then continues each chain from that partial with the
    // recurrent rows.
    // ---- LSTM1: input rows of W1 for the Tv frames (row j*Tv + t of emb), then the recurrence on B rows
    if (sampler_workspace) {
        // The sampler pass of this step already ran LSTM1 on these videos with these weights (its state never
        // sees a word or a dropout mask): take its state history and activated gates instead of recomputing.
        Carver sc(const_cast<void*>(sampler_workspace), sampler_workspace_bytes);
        SampleWs sw;
        carve_sample(sc, d, B, sampler_rows, &sw);
        if (!sc.ok() || sampler_rows <= 0) return S2VT_E_WORKSPACE;
        CopyList cl;
        // (the frame embedding the backward's dW1 product reads: the same product of the same operands in the sampler pass)
        if (cl.add(w.C1, sw.c1, (size_t)(T + 1) * BH * 4) && cl.add(w.H1, sw.h1, (size_t)(T + 1) * BH * 4) && cl.add(w.G1, sw.G1, (size_t)T * 4 * BH * 4) &&
            cl.add(w.emb, sw.emb, (size_t)B * Tv * E * 4)) {
            HIP_TRY(launch_copy_regions(cl, st));                                  // one library launch
        } else {                                                                   // (B * H not a multiple of 4: the runtime's copies)
            HIP_TRY(hipMemcpyAsync(w.emb, sw.emb, (size_t)B * Tv * E * 4, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipMemcpyAsync(w.C1, sw.c1, (size_t)(T + 1) * BH * 4, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipMemcpyAsync(w.H1, sw.h1, (size_t)(T + 1) * BH * 4, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipMemcpyAsync(w.G1, sw.G1, (size_t)T * 4 * BH * 4, hipMemcpyDeviceToDevice, st));
        }
    } else {
        {
            ASeg sx = make_seg(w.emb, E, E, 0);
            HIP_TRY(store_call(&sx, 1, p->lstm1_W, 4 * H, nullptr, w.Xp1, 4 * H, B * Tv, 4 * H, 0, -1, st));
        }
        // tf_s2vt.py:119 (encode) / :140 (decode, zero padding input: only the recurrent rows remain)
        HIP_TRY(lstm_recurrence(p->lstm1_W, E, p->lstm1_b, w.Xp1, (size_t)4 * H, Tv * 4 * H, Tv, w.C1, w.H1, BH, w.G1, (size_t)4 * BH,
                                nullptr, 0, B, H, T, 1.0f, none, 0, w.chain_abuf, w.chain_sync, st));
    }
    // DropoutWrapper(LSTM1) output for the N sample rows (tf_s2vt.py:75; code = 256 + t)
    HIP_TRY(launch_expand_dropout(w.H1 + BH, w.O1, T, B, N, H, keep, seed, 256u, video_id, sample_id, st));
    // ---- LSTM2, encode steps: the out1 rows of W2, written where the step's activated gates will go (the step kernel reads its
    // partial, then overwrites it).  encode_partials = false: the caller makes them (the split forward's stage B)
    if (encode_partials) {
        ASeg se = make_seg(w.O1, H, H, 0);                                       // encode: the word slot is the zero padding (:122)
        HIP_TRY(store_call(&se, 1, p->lstm2_W, 4 * H, nullptr, w.G2, 4 * H, Tv * N, 4 * H, 0, -1, st));
    }
    return S2VT_OK;
}

// ---- scheduled sampling (generate_words_tf_s2vt.py:101-211): the kernels around the per-step decode launches
__device__ __forceinline__ int32_t clamp_word(int32_t c, int V) { return c < 0 ? 0 : c >= V ? V - 1 : c; }

// before step 0: <bos> = 1 as every row's first fed word (:161-163), the ground truth as the workspace's time-major targets, and the
// all-argmax sample ids of the pick launches
__global__ __launch_bounds__(256) void sched_open_kernel(const int32_t* caption, int N, int Tc, int V, int32_t* prev, int32_t* tgt, int32_t* fed,
                                                         int32_t* argmax_sid)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N * Tc) return;
    const int t = i / N, n = i - t * N;
    tgt[i] = clamp_word(caption[(size_t)n * Tc + t], V);
    if (t == 0) { prev[n] = 1; fed[(size_t)n * Tc] = 1; argmax_sid[n] = -1; }
}

// behind the pick of step t, one thread per row: the row's argmax out of its packed pick (decoded as unpack_ids_kernel does), the running
// mask one_mask *= (generated != 0) updated BEFORE it weighs the step (:194-199), the step's loss coefficient and target, and the word
// step t + 1 is fed -- caption[n][t] when the coin of step t + 1 says so, the pick otherwise (:159-168)
__global__ __launch_bounds__(256) void sched_step_kernel(const unsigned long long* picked, int stride, const int32_t* caption, int N, int Tc, int t,
                                                         int V, const int32_t* video_id, const int32_t* sample_id, uint32_t seed_lo,
                                                         uint32_t seed_hi, float p_gt, float loss_weight, float* running, int32_t* generated,
                                                         int32_t* fed, float* mask, float* coef_tm, int32_t* target_tm, int32_t* prev)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const unsigned long long w = picked[(size_t)n * stride];
    const int32_t g = w ? (int32_t)(~(uint32_t)w) : 0;
    const float m = (t == 0 ? 1.0f : running[n]) * (g != 0 ? 1.0f : 0.0f);
    running[n] = m;
    const int32_t truth = clamp_word(caption[(size_t)n * Tc + t], V);
    generated[(size_t)n * Tc + t] = g;
    mask[(size_t)n * Tc + t] = m;
    coef_tm[(size_t)t * N + n] = loss_weight * m;
    target_tm[(size_t)t * N + n] = truth;
    if (t + 1 < Tc) {
        const int32_t word = mix_feeds_truth(seed_lo, seed_hi, (uint32_t)video_id[n], (uint32_t)sample_id[n], (uint32_t)(t + 1), p_gt) ? truth : g;
        fed[(size_t)n * Tc + t + 1] = word;
        prev[(size_t)(t + 1) * N + n] = word;
    }
}

// sum(mask) in a fixed order: one workgroup, thread i adds entries i, i + 256, ..., then the tree of caption_mask_kernel
__global__ __launch_bounds__(256) void sched_mask_sum_kernel(const float* mask, int n, float* mask_sum, float* mask_sum_copy)
{
    __shared__ float sh[4];
    float local = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) local += mask[i];
    for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float total = (sh[0] + sh[1]) + (sh[2] + sh[3]);
        if (mask_sum) *mask_sum = total;
        if (mask_sum_copy) *mask_sum_copy = total;
    }
}

// The scratch of the scheduled unroll beside the training workspace: every step's packed picks (zeroed up front: the pick packs by atomic
// maximum), the running mask, the pick launches' sample ids
struct SchedScratch { unsigned long long* packed; float* running; int32_t* argmax_sid; };
size_t carve_sched(Carver& c, const s2vt_dims* d, int N, SchedScratch* out)
{
    SchedScratch s;
    s.packed = c.take<unsigned long long>((size_t)d->n_caption_lstm_step * N * kPickStride);
    s.running = c.take<float>(N);
    s.argmax_sid = c.take<int32_t>(N);
    if (out) *out = s;
    return c.off;
}

// (inside a stage: hand a failed launch's error to the driver, whose HIP_TRY records it)
#define HIP_CHECK(expr) do { const hipError_t _e = (expr); if (_e != hipSuccess) return _e; } while (0)

// The decoding stage of the scheduled unroll, in straight-line stages.  Step t continues DESIGN section 3's chain of the cell on
// [out1 ; word ; h2] from the out1 partial in G2[Tv + t] with the fed word's rows of Wemb at kw = H, then H2[Tv + t] at kw = H + E -- the
// blocks the teacher-forced pass multiplies in the same order, so the activations are the ones it leaves for the same fed words.
struct SchedDecode {
    const s2vt_params* p; const TrainWs& w; const SchedScratch& x;
    int N, H, E, V, Tv, Tc; float keep; NoiseIds ids; hipStream_t st;
    const int32_t* caption; float p_gt, loss_weight; uint64_t coin_seed;
    float* logits; int32_t *generated, *fed; float *mask, *coef_tm; int32_t* target_tm;
    size_t NH;

    unsigned long long* picks(int t) const { return x.packed + (size_t)t * N * kPickStride; }

    hipError_t open()
    {
        ZeroList z;
        z.add(x.packed, (size_t)Tc * N * kPickStride * 8);
        HIP_CHECK(launch_zero_regions(z, st));
        hipLaunchKernelGGL(sched_open_kernel, dim3((N * Tc + 255) / 256), dim3(256), 0, st, caption, N, Tc, V, w.prev, w.tgt, fed, x.argmax_sid);
        return hipGetLastError();
    }
    // out1 @ W2[0:H] of the Tc decode steps, where the steps' activated gates will go
    hipError_t decode_partials()
    {
        ASeg so = make_seg(w.O1 + (size_t)Tv * NH, H, H, 0);
        return store_call(&so, 1, p->lstm2_W, 4 * H, nullptr, w.G2 + (size_t)Tv * 4 * NH, 4 * H, Tc * N, 4 * H, 0, -1, st);
    }
    // LSTM2 over the Tv frames (:151-154; the word slot is the zero padding): leaves the encoder state in slot Tv of C2 / H2
    hipError_t encode()
    {
        return lstm_recurrence(p->lstm2_W, H + E, p->lstm2_b, w.G2, (size_t)4 * NH, 4 * H, Tv, w.C2, w.H2, NH, w.G2, (size_t)4 * NH, w.O2, NH, N, H,
                               Tv, keep, ids, 512u, w.chain_abuf, w.chain_sync, st);
    }
    hipError_t step(int t)
    {
        const int u = Tv + t;
        float* const g2 = w.G2 + (size_t)u * 4 * NH;
        ASeg s2[2] = {make_seg(p->Wemb, E, E, H, 0, w.prev + (size_t)t * N), make_seg(w.H2 + (size_t)u * NH, H, H, H + E)};
        HIP_CHECK(lstm_call(s2, 2, p->lstm2_W, p->lstm2_b, w.C2 + (size_t)u * NH, 0, w.C2 + (size_t)(u + 1) * NH, w.H2 + (size_t)(u + 1) * NH,
                            w.O2 + (size_t)u * NH, g2, N, H, keep, ids, 512u + (uint32_t)u, -1, st, g2, 4 * H, 0));
        const NoiseIds argmax{ids.video_id, x.argmax_sid, 0};                 // (sample id -1: no noise is drawn, the seed is not read)
        HIP_CHECK(pick_call(w.O2 + (size_t)u * NH, H, p->embed_word_W, p->embed_word_b, N, H, V, argmax, t, picks(t), logits + (size_t)t * N * V, -1,
                            st, kPickStride));
        hipLaunchKernelGGL(sched_step_kernel, dim3((N + 255) / 256), dim3(256), 0, st, picks(t), kPickStride, caption, N, Tc, t, V, ids.video_id,
                           ids.sample_id, (uint32_t)coin_seed, (uint32_t)(coin_seed >> 32), p_gt, loss_weight, x.running, generated, fed, mask,
                           coef_tm, target_tm, w.prev);
        return hipGetLastError();
    }
    hipError_t close(float* mask_sum, float* mask_sum_copy)
    {
        hipLaunchKernelGGL(sched_mask_sum_kernel, dim3(1), dim3(256), 0, st, mask, N * Tc, mask_sum, mask_sum_copy);
        return hipGetLastError();
    }
};

// ---- averaged embeddings (average_generate_words_tf_s2vt.py:88-165): the scheduled unroll without the coin.  Step t >= 1 feeds LSTM2
// the mean of two rows of Wemb, (Wemb[caption[n][t - 1]] + Wemb[argmax of step t - 1]) / 2 (:131-133) -- no row of Wemb, so every step's
// operand is written out as a dense block Xbar[t] [N, E], which the cell launch reads at kw = H and the backward reads again.

// before step 0, one thread per element of the larger of [N, Tc] and [N, E]: the ground truth as the workspace's time-major targets and
// teacher-forced previous words, the all-argmax sample ids of the pick launches, <bos> = 1 as both ids of step 0 and Wemb[1] as every
// row of block 0 (:124-127)
__global__ __launch_bounds__(256) void avg_open_kernel(const int32_t* caption, const float* Wemb, int N, int Tc, int V, int E, int32_t* prev,
                                                       int32_t* tgt, int32_t* argmax_sid, int32_t* ida, int32_t* idb, float* xbar)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int32_t bos = clamp_word(1, V);
    if (i < (size_t)N * Tc) {
        const int t = (int)(i / N), n = (int)(i - (size_t)t * N);
        tgt[i] = clamp_word(caption[(size_t)n * Tc + t], V);
        prev[i] = t == 0 ? bos : clamp_word(caption[(size_t)n * Tc + t - 1], V);
        if (t == 0) { argmax_sid[n] = -1; ida[n] = bos; idb[n] = bos; }
    }
    if (i < (size_t)N * E) xbar[i] = Wemb[(size_t)bos * E + i % E];
}

// behind the pick of step t, one thread per element of [N, E]: the row's argmax out of its packed pick (decoded as unpack_ids_kernel
// does); the row's first thread writes generated, the step's loss coefficient loss_weight * mask (:154: the fed mask) and target, and the
// id pair of step t + 1; every thread its element of step t + 1's mean, one rounded addition and an exact halving
__global__ __launch_bounds__(256) void avg_step_kernel(const unsigned long long* picked, int stride, const int32_t* caption, const float* mask,
                                                       const float* Wemb, int N, int Tc, int t, int V, int E, float loss_weight, int32_t* generated,
                                                       float* coef_tm, int32_t* target_tm, int32_t* ida, int32_t* idb, float* xbar)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N * E) return;
    const int n = (int)(i / E), e = (int)(i - (size_t)n * E);
    const unsigned long long w = picked[(size_t)n * stride];
    const int32_t g = w ? (int32_t)(~(uint32_t)w) : 0;
    const int32_t truth = clamp_word(caption[(size_t)n * Tc + t], V);
    const int32_t pick = clamp_word(g, V);                  // (a pick is a column of the logits: in range already)
    if (e == 0) {
        generated[(size_t)n * Tc + t] = g;
        coef_tm[(size_t)t * N + n] = loss_weight * mask[(size_t)n * Tc + t];
        target_tm[(size_t)t * N + n] = truth;
        if (t + 1 < Tc) { ida[(size_t)(t + 1) * N + n] = truth; idb[(size_t)(t + 1) * N + n] = pick; }
    }
    if (t + 1 < Tc) xbar[(size_t)(t + 1) * N * E + i] = (Wemb[(size_t)truth * E + e] + Wemb[(size_t)pick * E + e]) * 0.5f;
}

// dW[ia[r]] += scale * dE[r] and dW[ib[r]] += scale * dE[r] (twice into the same row when the two ids are equal): one wave per row
__global__ __launch_bounds__(256) void scatter_add_rows2_kernel(const float* dE, int ld, const int32_t* ia, const int32_t* ib, float scale, int R,
                                                                int E, float* dW, int ldw)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int a = ia[r], b = ib[r];
    for (int e = threadIdx.x & 63; e < E; e += 64) {
        const float v = scale * dE[(size_t)r * ld + e];
        atomicAdd(dW + (size_t)a * ldw + e, v);
        atomicAdd(dW + (size_t)b * ldw + e, v);
    }
}
hipError_t launch_scatter_add_rows2(const float* dE, int ld, const int32_t* ia, const int32_t* ib, float scale, int R, int E, float* dW, int ldw,
                                    hipStream_t st)
{
    if (R <= 0) return hipSuccess;
    hipLaunchKernelGGL(scatter_add_rows2_kernel, dim3((R + 3) / 4), dim3(256), 0, st, dE, ld, ia, ib, scale, R, E, dW, ldw);
    return hipGetLastError();
}

// The scratch of the averaged unroll beside the training workspace: every step's packed picks (zeroed up front), the pick launches' sample
// ids, and what the backward reads again -- Xbar [Tc N, E] and the id pair (truth, picked) [Tc N] each, time-major
struct AvgScratch { unsigned long long* packed; int32_t* argmax_sid; float* xbar; int32_t *ida, *idb; };
size_t carve_avg(Carver& c, const s2vt_dims* d, int N, AvgScratch* out)
{
    const size_t R = (size_t)d->n_caption_lstm_step * N;
    AvgScratch s;
    s.packed = c.take<unsigned long long>(R * kPickStride);
    s.argmax_sid = c.take<int32_t>(N);
    s.xbar = c.take<float>(R * d->word_dim);
    s.ida = c.take<int32_t>(R);
    s.idb = c.take<int32_t>(R);
    if (out) *out = s;
    return c.off;
}

// The decoding stage of the averaged unroll: SchedDecode's stages with the step's mean block as a dense operand at kw = H
struct AvgDecode {
    const s2vt_params* p; const TrainWs& w; const AvgScratch& x;
    int N, H, E, V, Tv, Tc; float keep; NoiseIds ids; hipStream_t st;
    const int32_t* caption; const float* mask; float loss_weight;
    float* logits; int32_t* generated; float* coef_tm; int32_t* target_tm;
    size_t NH;

    unsigned long long* picks(int t) const { return x.packed + (size_t)t * N * kPickStride; }
    unsigned elem_blocks() const { return (unsigned)(((size_t)N * E + 255) / 256); }

    hipError_t open()
    {
        ZeroList z;
        z.add(x.packed, (size_t)Tc * N * kPickStride * 8);
        HIP_CHECK(launch_zero_regions(z, st));
        const size_t n = (size_t)N * (Tc > E ? Tc : E);
        hipLaunchKernelGGL(avg_open_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, caption, p->Wemb, N, Tc, V, E, w.prev, w.tgt,
                           x.argmax_sid, x.ida, x.idb, x.xbar);
        return hipGetLastError();
    }
    hipError_t decode_partials()
    {
        ASeg so = make_seg(w.O1 + (size_t)Tv * NH, H, H, 0);
        return store_call(&so, 1, p->lstm2_W, 4 * H, nullptr, w.G2 + (size_t)Tv * 4 * NH, 4 * H, Tc * N, 4 * H, 0, -1, st);
    }
    hipError_t encode()
    {
        return lstm_recurrence(p->lstm2_W, H + E, p->lstm2_b, w.G2, (size_t)4 * NH, 4 * H, Tv, w.C2, w.H2, NH, w.G2, (size_t)4 * NH, w.O2, NH, N, H,
                               Tv, keep, ids, 512u, w.chain_abuf, w.chain_sync, st);
    }
    hipError_t step(int t)
    {
        const int u = Tv + t;
        float* const g2 = w.G2 + (size_t)u * 4 * NH;
        ASeg s2[2] = {make_seg(x.xbar + (size_t)t * N * E, E, E, H), make_seg(w.H2 + (size_t)u * NH, H, H, H + E)};
        HIP_CHECK(lstm_call(s2, 2, p->lstm2_W, p->lstm2_b, w.C2 + (size_t)u * NH, 0, w.C2 + (size_t)(u + 1) * NH, w.H2 + (size_t)(u + 1) * NH,
                            w.O2 + (size_t)u * NH, g2, N, H, keep, ids, 512u + (uint32_t)u, -1, st, g2, 4 * H, 0));
        const NoiseIds argmax{ids.video_id, x.argmax_sid, 0};
        HIP_CHECK(pick_call(w.O2 + (size_t)u * NH, H, p->embed_word_W, p->embed_word_b, N, H, V, argmax, t, picks(t), logits + (size_t)t * N * V, -1,
                            st, kPickStride));
        hipLaunchKernelGGL(avg_step_kernel, dim3(elem_blocks()), dim3(256), 0, st, picks(t), kPickStride, caption, mask, p->Wemb, N, Tc, t, V, E,
                           loss_weight, generated, coef_tm, target_tm, x.ida, x.idb, x.xbar);
        return hipGetLastError();
    }
    hipError_t close(float* mask_sum, float* mask_sum_copy)
    {
        hipLaunchKernelGGL(sched_mask_sum_kernel, dim3(1), dim3(256), 0, st, mask, N * Tc, mask_sum, mask_sum_copy);
        return hipGetLastError();
    }
};

// ---- top-k score-weighted embeddings (sum_generate_words_tf_s2vt.py:101-219): the averaged unroll with another operand.  Step t >= 1
// feeds LSTM2 x = sum_j w_j Wemb[id_j] over the top-k logits of step t - 1, w = those logits over their sum (:163-174,208-210); the coin
// of :156,165 never selects the ground truth (quirk TK1), so the caption enters as labels only.  Every step's operand is a dense block
// X[t] [N, E]; ids, weights and the raw sums are kept for the backward, which differentiates the weights.

// before step 0, one thread per element of the largest of [N, Tc], [N, E] and [N, k]: the ground truth as the workspace's time-major
// targets and teacher-forced previous words, the all-argmax sample ids of the pick launches, and block 0 of the scratch -- Wemb[1] for
// every row (:158-161), written as the mix (<bos>, weight 1) + (<bos>, weight 0) ... with sum 1, which is what its gradient is
__global__ __launch_bounds__(256) void topk_open_kernel(const int32_t* caption, const float* Wemb, int N, int Tc, int V, int E, int k, int32_t* prev,
                                                        int32_t* tgt, int32_t* argmax_sid, int32_t* ids, float* wts, float* sums, float* X)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int32_t bos = clamp_word(1, V);
    if (i < (size_t)N * Tc) {
        const int t = (int)(i / N), n = (int)(i - (size_t)t * N);
        tgt[i] = clamp_word(caption[(size_t)n * Tc + t], V);
        prev[i] = t == 0 ? bos : clamp_word(caption[(size_t)n * Tc + t - 1], V);
        if (t == 0) { argmax_sid[n] = -1; sums[n] = 1.0f; }
    }
    if (i < (size_t)N * k) { ids[i] = bos; wts[i] = i % k == 0 ? 1.0f : 0.0f; }
    if (i < (size_t)N * E) X[i] = Wemb[(size_t)bos * E + i % E];
}

// The scratch of the top-k unroll beside the training workspace: every step's packed picks (zeroed up front), the pick launches' sample
// ids, and what the backward reads again -- X [Tc N, E], ids / w [Tc N, k] and S [Tc N], time-major, block t the mix step t was fed
struct TopkScratch { unsigned long long* packed; int32_t* argmax_sid; float* X; int32_t* ids; float *wts, *sums; };
size_t carve_topk(Carver& c, const s2vt_dims* d, int N, int k, TopkScratch* out)
{
    const size_t R = (size_t)d->n_caption_lstm_step * N;
    TopkScratch s;
    s.packed = c.take<unsigned long long>(R * kPickStride);
    s.argmax_sid = c.take<int32_t>(N);
    s.X = c.take<float>(R * d->word_dim);
    s.ids = c.take<int32_t>(R * k);
    s.wts = c.take<float>(R * k);
    s.sums = c.take<float>(R);
    if (out) *out = s;
    return c.off;
}
bool topk_k_ok(const s2vt_dims* d, int k) { return k >= 1 && k <= kTopkFeedMax && k <= d->n_words; }

// The decoding stage of the top-k unroll: AvgDecode's stages, the step kernel replaced by the top-k mix of the step's logits
struct TopkDecode {
    const s2vt_params* p; const TrainWs& w; const TopkScratch& x;
    int N, H, E, V, Tv, Tc, k; float keep; NoiseIds ids; hipStream_t st;
    const int32_t* caption; const float* mask; float loss_weight;
    float* logits; int32_t* generated; float* coef_tm; int32_t* target_tm;
    size_t NH;

    unsigned long long* picks(int t) const { return x.packed + (size_t)t * N * kPickStride; }

    hipError_t open()
    {
        ZeroList z;
        z.add(x.packed, (size_t)Tc * N * kPickStride * 8);
        HIP_CHECK(launch_zero_regions(z, st));
        const int widest = Tc > E ? (Tc > k ? Tc : k) : (E > k ? E : k);
        const size_t n = (size_t)N * widest;
        hipLaunchKernelGGL(topk_open_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, caption, p->Wemb, N, Tc, V, E, k, w.prev, w.tgt,
                           x.argmax_sid, x.ids, x.wts, x.sums, x.X);
        return hipGetLastError();
    }
    hipError_t decode_partials()
    {
        ASeg so = make_seg(w.O1 + (size_t)Tv * NH, H, H, 0);
        return store_call(&so, 1, p->lstm2_W, 4 * H, nullptr, w.G2 + (size_t)Tv * 4 * NH, 4 * H, Tc * N, 4 * H, 0, -1, st);
    }
    hipError_t encode()
    {
        return lstm_recurrence(p->lstm2_W, H + E, p->lstm2_b, w.G2, (size_t)4 * NH, 4 * H, Tv, w.C2, w.H2, NH, w.G2, (size_t)4 * NH, w.O2, NH, N, H,
                               Tv, keep, ids, 512u, w.chain_abuf, w.chain_sync, st);
    }
    hipError_t step(int t)
    {
        const int u = Tv + t;
        float* const g2 = w.G2 + (size_t)u * 4 * NH;
        ASeg s2[2] = {make_seg(x.X + (size_t)t * N * E, E, E, H), make_seg(w.H2 + (size_t)u * NH, H, H, H + E)};
        HIP_CHECK(lstm_call(s2, 2, p->lstm2_W, p->lstm2_b, w.C2 + (size_t)u * NH, 0, w.C2 + (size_t)(u + 1) * NH, w.H2 + (size_t)(u + 1) * NH,
                            w.O2 + (size_t)u * NH, g2, N, H, keep, ids, 512u + (uint32_t)u, -1, st, g2, 4 * H, 0));
        const NoiseIds argmax{ids.video_id, x.argmax_sid, 0};
        float* const lt = logits + (size_t)t * N * V;
        HIP_CHECK(pick_call(w.O2 + (size_t)u * NH, H, p->embed_word_W, p->embed_word_b, N, H, V, argmax, t, picks(t), lt, -1, st, kPickStride));
        const TopkStep ts{caption, mask, N, Tc, t, loss_weight, generated, coef_tm, target_tm, nullptr};
        const size_t nx = (size_t)(t + 1) * N;                 // (the last step forms no mix: its bookkeeping only)
        const bool more = t + 1 < Tc;
        return launch_topk_mix_fwd(lt, V, N, V, k, p->Wemb, E, more ? x.ids + nx * k : nullptr, more ? x.wts + nx * k : nullptr,
                                   more ? x.sums + nx : nullptr, more ? x.X + nx * E : nullptr, E, &ts, st);
    }
    hipError_t close(float* mask_sum, float* mask_sum_copy)
    {
        hipLaunchKernelGGL(sched_mask_sum_kernel, dim3(1), dim3(256), 0, st, mask, N * Tc, mask_sum, mask_sum_copy);
        return hipGetLastError();
    }
};
}  // namespace

extern "C" {

size_t s2vt_lstm_recurrence_bwd_scratch_bytes(int32_t M, int32_t H)
{
    if (M <= 0 || H <= 0) return 0;
    Carver c(nullptr, 0);
    size_t imgf, exf, syncb;
    bwd_scratch_max(H, M, &imgf, &exf, &syncb);
    c.take<float>((size_t)kMaxSlabs * M * H); c.take<float>((size_t)M * H);
    c.take<float>(imgf); c.take<float>(exf); c.take<unsigned>(syncb / 4);
    return c.off;
}

static int recurrence_bwd_entry(const float* W, int32_t kw0, const float* gates, const float* C_hist, const float* dext, int64_t dext_tstride,
                               int32_t ld_ext, int32_t dext_t0, float* dZ, int32_t M, int32_t H, int32_t T, float keep, uint64_t seed,
                               const int32_t* video_id, const int32_t* sample_id, uint32_t drop_code0, int32_t persistent, void* scratch,
                               size_t scratch_bytes, s2vt_stream stream, bool split)
{
    if (!W || !gates || !C_hist || !dZ || M <= 0 || H <= 0 || T < 0 || kw0 < 0 || persistent < -1 || persistent > 1 || !scratch) return S2VT_E_BADARG;
    if (dext && (ld_ext < H || dext_t0 < 0)) return S2VT_E_BADARG;
    if (!(keep > 0.0f) || (keep < 1.0f && (!video_id || !sample_id))) return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(scratch) & 255u) return S2VT_E_ALIGN;
    if (chain_fault()) return S2VT_E_CHAIN_TIMEOUT;
    Carver c(scratch, scratch_bytes);
    size_t imgf, exf, syncb;
    bwd_scratch_max(H, M, &imgf, &exf, &syncb);
    BwdScratch sc;
    sc.slab = c.take<float>((size_t)kMaxSlabs * M * H); sc.dc = c.take<float>((size_t)M * H);
    sc.bimg = c.take<float>(imgf); sc.bex = c.take<float>(exf); sc.bsync = c.take<unsigned>(syncb / 4);
    if (!c.ok()) return S2VT_E_WORKSPACE;
    if (persistent == 1 && !bwd_chain_eligible(M, H)) return S2VT_E_BADARG;
    if (split && (persistent != 1 || !bwd_chain_split_serves(M, H) || (reinterpret_cast<uintptr_t>(W) & 15))) return S2VT_E_BADARG;
    HIP_TRY(lstm_recurrence_bwd(W, kw0, gates, C_hist, dext, (size_t)dext_tstride, ld_ext, dext_t0, dZ, M, H, T, keep, seed, drop_code0, video_id,
                                sample_id, sc, persistent, S(stream), nullptr, nullptr, split));
    return S2VT_OK;
}

int s2vt_lstm_recurrence_bwd(const float* W, int32_t kw0, const float* gates, const float* C_hist, const float* dext, int64_t dext_tstride,
                             int32_t ld_ext, int32_t dext_t0, float* dZ, int32_t M, int32_t H, int32_t T, float keep, uint64_t seed,
                             const int32_t* video_id, const int32_t* sample_id, uint32_t drop_code0, int32_t persistent, void* scratch,
                             size_t scratch_bytes, s2vt_stream stream)
{
    return recurrence_bwd_entry(W, kw0, gates, C_hist, dext, dext_tstride, ld_ext, dext_t0, dZ, M, H, T, keep, seed, video_id, sample_id, drop_code0,
                                persistent, scratch, scratch_bytes, stream, false);
}

int s2vt_lstm_recurrence_bwd_split(const float* W, int32_t kw0, const float* gates, const float* C_hist, const float* dext, int64_t dext_tstride,
                                   int32_t ld_ext, int32_t dext_t0, float* dZ, int32_t M, int32_t H, int32_t T, float keep, uint64_t seed,
                                   const int32_t* video_id, const int32_t* sample_id, uint32_t drop_code0, int32_t persistent, void* scratch,
                                   size_t scratch_bytes, s2vt_stream stream)
{
    return recurrence_bwd_entry(W, kw0, gates, C_hist, dext, dext_tstride, ld_ext, dext_t0, dZ, M, H, T, keep, seed, video_id, sample_id, drop_code0,
                                persistent, scratch, scratch_bytes, stream, true);
}

size_t s2vt_train_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t N)
{
    if (!dims_ok_res(d) || B <= 0 || N <= 0 || N % B) return 0;      // (the residual model's unroll needs no region of its own)
    Carver c(nullptr, 0);
    return carve_train(c, d, B, N, nullptr);
}

int s2vt_train_workspace_dz2(const s2vt_dims* d, int32_t B, int32_t N, size_t* offset, size_t* floats)
{
    if (!dims_ok_res(d) || B <= 0 || N <= 0 || N % B || !offset || !floats) return S2VT_E_BADARG;
    alignas(256) static char origin[256];                             // (a base to measure from: nothing is read or written through it)
    Carver c(origin, 0);
    TrainWs w;
    carve_train(c, d, B, N, &w);
    *offset = (size_t)(reinterpret_cast<const char*>(w.dZ2) - origin);
    *floats = (size_t)(d->n_video_lstm_step + d->n_caption_lstm_step) * N * 4 * d->lstm_dim;
    return S2VT_OK;
}

int s2vt_teacher_forced_fwd(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t N,
                            const int32_t* caption, float keep, uint64_t seed, const int32_t* video_id,
                            const int32_t* sample_id, float* logits, void* workspace, size_t workspace_bytes,
                            s2vt_stream stream)
{
    return s2vt_teacher_forced_fwd_reuse(d, p, video, B, N, caption, keep, seed, video_id, sample_id, logits, workspace,
                                         workspace_bytes, nullptr, 0, 0, stream);
}

int s2vt_teacher_forced_fwd_reuse(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t N,
                                  const int32_t* caption, float keep, uint64_t seed, const int32_t* video_id,
                                  const int32_t* sample_id, float* logits, void* workspace, size_t workspace_bytes,
                                  const void* sampler_workspace, size_t sampler_workspace_bytes, int32_t sampler_rows,
                                  s2vt_stream stream)
{
    return s2vt_teacher_forced_fwd_steps(d, p, video, B, N, caption, d ? d->n_caption_lstm_step : 0, keep, seed, video_id, sample_id,
                                         logits, workspace, workspace_bytes, sampler_workspace, sampler_workspace_bytes, sampler_rows,
                                         stream);
}

int s2vt_teacher_forced_fwd_steps(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t N,
                                  const int32_t* caption, int32_t caption_steps, float keep, uint64_t seed,
                                  const int32_t* video_id, const int32_t* sample_id, float* logits, void* workspace,
                                  size_t workspace_bytes, const void* sampler_workspace, size_t sampler_workspace_bytes,
                                  int32_t sampler_rows, s2vt_stream stream)
{
    return s2vt_teacher_forced_fwd_live(d, p, video, B, N, caption, caption_steps, nullptr, 0, keep, seed, video_id, sample_id, logits,
                                        workspace, workspace_bytes, sampler_workspace, sampler_workspace_bytes, sampler_rows, stream);
}

// The teacher-forced forward.  split_entry false: s2vt_teacher_forced_fwd_live, every product an fp32 chain.  true:
// s2vt_teacher_forced_fwd_split -- the split workspace is validated with the other arguments (before anything is launched), and at
// stage >= 1 the vocabulary logits, at stage 2 LSTM2's hoisted input partials too, run as split-bf16 NN products where the shape fits.
constexpr int kSplitFwdDefault = 1;      // the highest stage that is kept as the default (profiles/NOTES.md)
static bool split_mode_on(int N);        // (below, with the backward: S2VT_SPLIT_GRADS and the 256-row threshold)

static int teacher_forced_fwd_body(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t N,
                                   const int32_t* caption, int32_t caption_steps, const int32_t* live_rows, int32_t n_live, float keep,
                                   uint64_t seed, const int32_t* video_id, const int32_t* sample_id, float* logits, void* workspace,
                                   size_t workspace_bytes, const void* sampler_workspace, size_t sampler_workspace_bytes,
                                   int32_t sampler_rows, s2vt_stream stream, void* split_ws, size_t split_ws_bytes, bool split_entry, int stage)
{
    if ((live_rows == nullptr) != (n_live == 0) || n_live < 0) return S2VT_E_BADARG;
    if (!dims_ok_res(d) || !params_ok(p) || !video || !caption || !logits || !workspace || B <= 0 || N <= 0 || N % B)
        return S2VT_E_BADARG;
    if (!(keep > 0.0f) || (keep < 1.0f && (!video_id || !sample_id))) return S2VT_E_BADARG;
    if (split_entry && !split_ws) return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    if (split_entry && (reinterpret_cast<uintptr_t>(split_ws) & 255u)) return S2VT_E_ALIGN;
    if (chain_fault()) return S2VT_E_CHAIN_TIMEOUT;
    if (caption_steps < 1 || caption_steps > d->n_caption_lstm_step) return S2VT_E_BADARG;
    if (live_rows && (n_live > caption_steps * N || ((d->lstm_dim | d->word_dim) & 3))) return S2VT_E_BADARG;     // (packed rows move as 16-byte pieces)
    // Tc / T below are the steps this call UNROLLS; every buffer is time-major, so a truncated unroll is the leading part
    // of the full one's layout (the workspace is carved by the model's dimensions whatever caption_steps says)
    const int H = d->lstm_dim, E = d->word_dim, V = d->n_words, Tv = d->n_video_lstm_step, Tc = caption_steps;
    const int T = Tv + Tc;
    Carver c(workspace, workspace_bytes);
    TrainWs w;
    carve_train(c, d, B, N, &w);
    if (!c.ok()) return S2VT_E_WORKSPACE;
    Bf16Ws bw{};
    if (split_entry) {
        // (held to its declared size whatever the stage or the shape makes of it, as the backward holds it)
        Carver cb(split_ws, split_ws_bytes);
        carve_bf16(cb, d, B, N, &bw, true);
        if (!cb.ok()) return S2VT_E_WORKSPACE;
    }
    hipStream_t st = S(stream);
    const size_t NH = (size_t)N * H;
    const int Rd = live_rows ? n_live : Tc * N;               // decode rows of the hoisted products
    // What runs on split-bf16: where the backward's products do (the split mode is active for N -- whichever operand layout
    // S2VT_SPLIT_FUSED gives the backward: the forward's arithmetic does not depend on that knob), operands the casts can place (H % 8: the
    // embedding columns start at a 16-byte boundary behind O1's), planes within the K-major loader's reach and row planes that fit their region.
    const int K4 = bf16_pad(4 * H), Kv = bf16_pad(V), Hp1 = bf16_pad(H + 1), HEp = bf16_pad(H + E);
    const bool split_on = split_entry && stage >= 1 && split_mode_on(N) && !(H & 7);
    // stage A's A planes [Rd][bf16_pad(H + 1)]: AT (the fused carve counts them: always; the unfused one may be shorter), else BT
    const size_t bt_cap = split_entry ? (size_t)(bw.AT - bw.BT) : 0, at_cap = split_entry ? (size_t)(bw.L + bw.lo_delta - bw.AT) : 0;
    uint16_t* const o2p = (size_t)Rd * Hp1 <= at_cap ? bw.AT : (size_t)Rd * Hp1 <= bt_cap ? bw.BT : nullptr;
    const bool split_logits = split_on && o2p && gemm_bf16x3_tn_ok(Kv, Kv, H);
    // (stage B's A planes live in BT, unused by the fused backward and free until the backward otherwise: [rows][bf16_pad(H + E)])
    const bool split_g2 = split_on && stage >= 2 && gemm_bf16x3_tn_ok(K4, K4, H + E) && (size_t)(Tv * N > Rd ? Tv * N : Rd) * HEp <= bt_cap;
    auto lo = [&](uint16_t* hi) { return hi + bw.lo_delta; };
    auto nn = [&](uint16_t* A, int lda, uint16_t* Bm, int ldb, float* Cm, int ldc, int M, int Nn, int K, const float* cbias) {
        return launch_gemm_bf16x3_nn(A, lo(A), lda, Bm, lo(Bm), ldb, Cm, ldc, M, Nn, K, 0, cbias, bw.kpart, bw.kpart_floats, 0, st);
    };

    HIP_TRY(launch_prep_caption(caption, w.prev, w.tgt, N, d->n_caption_lstm_step, st));
    {
        const int rc = unroll_front(d, p, video, B, N, T, keep, seed, video_id, sample_id, w, sampler_workspace, sampler_workspace_bytes,
                                    sampler_rows, stream, !split_g2);
        if (rc != S2VT_OK) return rc;
    }
    NoiseIds ids{video_id, sample_id, seed};
    if (split_g2) {
        // ---- stage B: lstm2_W's input rows [H + E][4H] as K-major planes in W (the Wout cast of stage A follows in stream order), then
        // the encode partials O1[:Tv] . lstm2_W[0:H] from row planes in BT
        HIP_TRY(launch_cast_rows_bf16(p->lstm2_W, 4 * H, nullptr, H + E, 4 * H, bw.W, K4, st, lo(bw.W)));
        HIP_TRY(launch_cast_rows_bf16(w.O1, H, nullptr, Tv * N, H, bw.BT, bf16_pad(H), st, lo(bw.BT)));
        HIP_TRY(nn(bw.BT, bf16_pad(H), bw.W, K4, w.G2, 4 * H, Tv * N, 4 * H, H, nullptr));
        // decode rows: one row-plane set [Rd][bf16_pad(H + E)] -- O1 in columns 0 .. H - 1, the previous words' embedding rows behind them
        // (zeros up to the padded width)
        if (live_rows) HIP_TRY(launch_gather_i32(w.prev, live_rows, n_live, w.prevp, st));
        HIP_TRY(launch_cast_rows_bf16(w.O1 + (size_t)Tv * NH, H, live_rows, Rd, H, bw.BT, HEp, st, lo(bw.BT), 0, H));
        HIP_TRY(launch_cast_rows_bf16(p->Wemb, E, live_rows ? w.prevp : w.prev, Rd, E, bw.BT + H, HEp, st, lo(bw.BT) + H, 0, HEp - H));
    }
    // ---- LSTM2, decode steps: rows of W2 for [out1 ; embed(prev word)] for all steps at once
    {
        if (!live_rows) {
            if (split_g2) {
                HIP_TRY(nn(bw.BT, HEp, bw.W, K4, w.G2 + (size_t)Tv * 4 * NH, 4 * H, Tc * N, 4 * H, H + E, nullptr));
            } else {
                ASeg sd[2] = {make_seg(w.O1 + (size_t)Tv * NH, H, H, 0), make_seg(p->Wemb, E, E, H, 0, w.prev)};   // decode (:143)
                HIP_TRY(store_call(sd, 2, p->lstm2_W, 4 * H, nullptr, w.G2 + (size_t)Tv * 4 * NH, 4 * H, Tc * N, 4 * H, 0, -1, st));
            }
        } else {
            // live rows: the partials of the unmasked positions only (both operands gathered through the list), packed, then
            // scattered into the zeroed decode part -- a masked position's cell then steps from a zero partial: finite values
            // that feed nothing (its logits are not computed, its gradients are zeros)
            if (split_g2) {
                HIP_TRY(nn(bw.BT, HEp, bw.W, K4, w.dZ2p, 4 * H, n_live, 4 * H, H + E, nullptr));
            } else {
                HIP_TRY(launch_gather_i32(w.prev, live_rows, n_live, w.prevp, st));
                ASeg sd[2] = {make_seg(w.O1 + (size_t)Tv * NH, H, H, 0, 0, live_rows), make_seg(p->Wemb, E, E, H, 0, w.prevp)};
                HIP_TRY(store_call(sd, 2, p->lstm2_W, 4 * H, nullptr, w.dZ2p, 4 * H, n_live, 4 * H, 0, -1, st));   // (dZ2p: free until the backward)
            }
            float* const dec = w.G2 + (size_t)Tv * 4 * NH;
            ZeroList z;
            z.add(dec, (size_t)Tc * N * 4 * H * 4);
            // (recurrences that stop the rows behind their <eos> leave those rows' histories unwritten: G2 keeps the zeros of this
            //  fill there, and the cell states get zeros too, so that a DENSE backward recurrence over this workspace -- the per-step
            //  form under s2vt_chain_hold -- multiplies its zero gradients with finite values)
            if (live_rows && Tc <= 128 && chain_live_capable(N, H)) z.add(w.C2 + (size_t)(Tv + 1) * NH, (size_t)Tc * NH * 4);
            HIP_TRY(launch_zero_regions(z, st));
            HIP_TRY(launch_scatter_rows(w.dZ2p, 4 * H, live_rows, n_live, 4 * H, dec, 4 * H, st));
        }
    }
    // the recurrence continues each chain from its partial in G2[t] and overwrites it with the activated gates.  Live rows at
    // 257-384 rows: a row behind its <eos> stops stepping (rows by length, live rows per step -- its histories there are not
    // written and not read: every consumer below and in the backward pass gathers the live pairs)
    const bool rec_live = live_rows && Tc <= 128 && chain_live_capable(N, H);
    // (the kernel also VALIDATES the list -- per-row prefix, strictly ascending -- and raises the sticky fault otherwise, so it runs for
    //  every live pass it can take, whether or not the recurrences of this shape use the order)
    if (live_rows && Tc <= 128 && N <= 1024) HIP_TRY(launch_row_order(live_rows, n_live, N, Tv, Tc, w.perm, w.nlive, st));
    HIP_TRY(lstm_recurrence(p->lstm2_W, H + E, p->lstm2_b, w.G2, (size_t)4 * NH, 4 * H, T, w.C2, w.H2, NH, w.G2, (size_t)4 * NH,
                            w.O2, NH, N, H, T, keep, ids, 512u, w.chain_abuf, w.chain_sync, st, rec_live ? w.perm : nullptr,
                            rec_live ? w.nlive : nullptr));
    // Residual model (residual_tf_s2vt.py:149-151): output2 = output1 + output2 ahead of the vocabulary projection -- O2[Tv:] becomes
    // s = O1[Tv:] + O2[Tv:] in place, whichever form the recurrence took (a row the live recurrence did not write holds nothing anyone
    // reads, before or after).  Every later reader of the decode part of w.O2 wants s: the logits product below, dWout = s^T dlogits in all
    // three precision modes (vocab_fp32's tn, vocab_tr's tr, vocab_fused's rows1).  The dropout backward of LSTM2 regenerates its mask
    // from Philox and never reads O2; LSTM2's own weight gradients read O1 and H2 (the un-summed h'), the encode part of O2 is untouched.
    // (The scheduled forward writes and reads O2 per step; it refuses the residual bit.)
    if (is_residual(d)) HIP_TRY(launch_add_inplace(w.O2 + (size_t)Tv * NH, w.O1 + (size_t)Tv * NH, (size_t)Tc * NH, st));
    // vocab logits for all Tc steps at once (tf_s2vt.py:153): rows t*N + n -- or only the LIVE ones (row r of the output is
    // row live_rows[r] of the unroll: a masked position's logits feed nothing, its loss term and gradient are exact zeros)
    if (split_logits) {
        // stage A: the decode rows of O2 (gathered) as row planes [Rd][bf16_pad(H + 1)] in AT -- the layout and the ones column of
        // vocab_fused's rows1 cast; the product's K = H never multiplies that column with anything but a zero -- Wout as K-major planes
        // [H][bf16_pad(V)] in W, and the NN product with the fp32 bias.  L is not touched: the split softmax writes the dlogits planes there next.
        HIP_TRY(launch_cast_rows_bf16(w.O2 + (size_t)Tv * NH, H, live_rows, Rd, H, o2p, Hp1, st, lo(o2p), 1));
        HIP_TRY(launch_cast_rows_bf16(p->embed_word_W, V, nullptr, H, V, bw.W, Kv, st, lo(bw.W)));
        HIP_TRY(nn(o2p, Hp1, bw.W, Kv, logits, V, Rd, V, H, p->embed_word_b));
        return S2VT_OK;
    }
    ASeg so = make_seg(w.O2 + (size_t)Tv * NH, H, H, 0, 0, live_rows);
    HIP_TRY(store_call(&so, 1, p->embed_word_W, V, p->embed_word_b, logits, V, Rd, V, 0, -1, st));
    return S2VT_OK;
}

int s2vt_teacher_forced_fwd_live(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t N,
                                 const int32_t* caption, int32_t caption_steps, const int32_t* live_rows, int32_t n_live, float keep,
                                 uint64_t seed, const int32_t* video_id, const int32_t* sample_id, float* logits, void* workspace,
                                 size_t workspace_bytes, const void* sampler_workspace, size_t sampler_workspace_bytes,
                                 int32_t sampler_rows, s2vt_stream stream)
{
    return teacher_forced_fwd_body(d, p, video, B, N, caption, caption_steps, live_rows, n_live, keep, seed, video_id, sample_id, logits,
                                   workspace, workspace_bytes, sampler_workspace, sampler_workspace_bytes, sampler_rows, stream, nullptr, 0,
                                   false, 0);
}

// S2VT_SPLIT_FWD (read once): 0 = the fp32 forward, 1 = stage A (the vocabulary logits on split-bf16), 2 = stages A and B (LSTM2's hoisted
// input partials too).  Anything else, or unset: the default.
int s2vt_split_fwd_stage(void)
{
    static const int stage = [] {
        const char* e = getenv("S2VT_SPLIT_FWD");
        if (e && (e[0] == '0' || e[0] == '1' || e[0] == '2') && !e[1]) return e[0] - '0';
        return kSplitFwdDefault;
    }();
    return stage;
}

int s2vt_split_fwd_active(int32_t N)
{
    return split_mode_on(N) ? s2vt_split_fwd_stage() : 0;
}

int s2vt_teacher_forced_fwd_split(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t N,
                                  const int32_t* caption, int32_t caption_steps, const int32_t* live_rows, int32_t n_live, float keep,
                                  uint64_t seed, const int32_t* video_id, const int32_t* sample_id, float* logits, void* workspace,
                                  size_t workspace_bytes, const void* sampler_workspace, size_t sampler_workspace_bytes,
                                  int32_t sampler_rows, void* split_ws, size_t split_ws_bytes, s2vt_stream stream)
{
    return teacher_forced_fwd_body(d, p, video, B, N, caption, caption_steps, live_rows, n_live, keep, seed, video_id, sample_id, logits,
                                   workspace, workspace_bytes, sampler_workspace, sampler_workspace_bytes, sampler_rows, stream, split_ws,
                                   split_ws_bytes, true, s2vt_split_fwd_stage());
}

size_t s2vt_scheduled_scratch_bytes(const s2vt_dims* d, int32_t N)
{
    if (!dims_ok(d) || N <= 0) return 0;
    Carver c(nullptr, 0);
    return carve_sched(c, d, N, nullptr);
}

int s2vt_scheduled_fwd(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t N, const int32_t* caption, float p_gt,
                       uint64_t coin_seed, float loss_weight, float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id,
                       float* logits_out, int32_t* generated, int32_t* fed, float* mask, float* coef_tm, int32_t* target_tm, float* mask_sum,
                       float* mask_sum_copy, void* workspace, size_t workspace_bytes, void* scratch, size_t scratch_bytes, s2vt_stream stream)
{
    if (!dims_ok(d) || !params_ok(p) || !video || !caption || !video_id || !sample_id || !logits_out || !generated || !fed || !mask || !coef_tm ||
        !target_tm || !workspace || !scratch || B <= 0 || N <= 0 || N % B)
        return S2VT_E_BADARG;
    if (!(p_gt >= 0.0f && p_gt <= 1.0f) || !(keep > 0.0f)) return S2VT_E_BADARG;              // (a NaN fails the comparisons)
    if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(scratch)) & 255u) return S2VT_E_ALIGN;
    if (chain_fault()) return S2VT_E_CHAIN_TIMEOUT;
    const int H = d->lstm_dim, E = d->word_dim, V = d->n_words, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step;
    Carver c(workspace, workspace_bytes);
    TrainWs w;
    carve_train(c, d, B, N, &w);
    Carver cs(scratch, scratch_bytes);
    SchedScratch x;
    carve_sched(cs, d, N, &x);
    if (!c.ok() || !cs.ok()) return S2VT_E_WORKSPACE;
    hipStream_t st = S(stream);
    SchedDecode s{p, w, x, N, H, E, V, Tv, Tc, keep, NoiseIds{video_id, sample_id, seed}, st, caption, p_gt, loss_weight, coin_seed,
                  logits_out, generated, fed, mask, coef_tm, target_tm, (size_t)N * H};
    HIP_TRY(s.open());
    {
        const int rc = unroll_front(d, p, video, B, N, Tv + Tc, keep, seed, video_id, sample_id, w, nullptr, 0, 0, stream);
        if (rc != S2VT_OK) return rc;
    }
    HIP_TRY(s.decode_partials());
    HIP_TRY(s.encode());
    for (int t = 0; t < Tc; ++t) HIP_TRY(s.step(t));
    HIP_TRY(s.close(mask_sum, mask_sum_copy));
    return S2VT_OK;
}

size_t s2vt_averaged_scratch_bytes(const s2vt_dims* d, int32_t N)
{
    if (!dims_ok(d) || N <= 0) return 0;
    Carver c(nullptr, 0);
    return carve_avg(c, d, N, nullptr);
}

int s2vt_averaged_fwd(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t N, const int32_t* caption, const float* mask,
                      float loss_weight, float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id, float* logits_out,
                      int32_t* generated, float* coef_tm, int32_t* target_tm, float* mask_sum, float* mask_sum_copy, void* workspace,
                      size_t workspace_bytes, void* scratch, size_t scratch_bytes, s2vt_stream stream)
{
    if (!dims_ok(d) || !params_ok(p) || !video || !caption || !mask || !video_id || !sample_id || !logits_out || !generated || !coef_tm ||
        !target_tm || !workspace || !scratch || B <= 0 || N <= 0 || N % B)
        return S2VT_E_BADARG;
    if (!(keep > 0.0f)) return S2VT_E_BADARG;                                                  // (a NaN fails the comparison)
    if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(scratch)) & 255u) return S2VT_E_ALIGN;
    if (chain_fault()) return S2VT_E_CHAIN_TIMEOUT;
    const int H = d->lstm_dim, E = d->word_dim, V = d->n_words, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step;
    Carver c(workspace, workspace_bytes);
    TrainWs w;
    carve_train(c, d, B, N, &w);
    Carver cs(scratch, scratch_bytes);
    AvgScratch x;
    carve_avg(cs, d, N, &x);
    if (!c.ok() || !cs.ok()) return S2VT_E_WORKSPACE;
    hipStream_t st = S(stream);
    AvgDecode s{p, w, x, N, H, E, V, Tv, Tc, keep, NoiseIds{video_id, sample_id, seed}, st, caption, mask, loss_weight,
                logits_out, generated, coef_tm, target_tm, (size_t)N * H};
    HIP_TRY(s.open());
    {
        const int rc = unroll_front(d, p, video, B, N, Tv + Tc, keep, seed, video_id, sample_id, w, nullptr, 0, 0, stream);
        if (rc != S2VT_OK) return rc;
    }
    HIP_TRY(s.decode_partials());
    HIP_TRY(s.encode());
    for (int t = 0; t < Tc; ++t) HIP_TRY(s.step(t));
    HIP_TRY(s.close(mask_sum, mask_sum_copy));
    return S2VT_OK;
}

size_t s2vt_topk_feed_scratch_bytes(const s2vt_dims* d, int32_t N, int32_t k)
{
    if (!dims_ok(d) || N <= 0 || !topk_k_ok(d, k)) return 0;
    Carver c(nullptr, 0);
    return carve_topk(c, d, N, k, nullptr);
}

int s2vt_topk_feed_fwd(const s2vt_dims* d, const s2vt_params* p, const float* video, int32_t B, int32_t N, const int32_t* caption, const float* mask,
                       float loss_weight, float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id, int32_t k,
                       float* logits_out, int32_t* generated, float* coef_tm, int32_t* target_tm, float* mask_sum, float* mask_sum_copy,
                       void* workspace, size_t workspace_bytes, void* scratch, size_t scratch_bytes, s2vt_stream stream)
{
    if (!dims_ok(d) || !params_ok(p) || !video || !caption || !mask || !video_id || !sample_id || !logits_out || !generated || !coef_tm ||
        !target_tm || !workspace || !scratch || B <= 0 || N <= 0 || N % B || !topk_k_ok(d, k))
        return S2VT_E_BADARG;
    if (!(keep > 0.0f)) return S2VT_E_BADARG;                                                  // (a NaN fails the comparison)
    if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(scratch)) & 255u) return S2VT_E_ALIGN;
    if (chain_fault()) return S2VT_E_CHAIN_TIMEOUT;
    const int H = d->lstm_dim, E = d->word_dim, V = d->n_words, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step;
    Carver c(workspace, workspace_bytes);
    TrainWs w;
    carve_train(c, d, B, N, &w);
    Carver cs(scratch, scratch_bytes);
    TopkScratch x;
    carve_topk(cs, d, N, k, &x);
    if (!c.ok() || !cs.ok()) return S2VT_E_WORKSPACE;
    hipStream_t st = S(stream);
    TopkDecode s{p, w, x, N, H, E, V, Tv, Tc, k, keep, NoiseIds{video_id, sample_id, seed}, st, caption, mask, loss_weight,
                 logits_out, generated, coef_tm, target_tm, (size_t)N * H};
    HIP_TRY(s.open());
    {
        const int rc = unroll_front(d, p, video, B, N, Tv + Tc, keep, seed, video_id, sample_id, w, nullptr, 0, 0, stream);
        if (rc != S2VT_OK) return rc;
    }
    HIP_TRY(s.decode_partials());
    HIP_TRY(s.encode());
    for (int t = 0; t < Tc; ++t) HIP_TRY(s.step(t));
    HIP_TRY(s.close(mask_sum, mask_sum_copy));
    return S2VT_OK;
}

int s2vt_caption_mask(const int32_t* ids, int32_t N, int32_t Tc, float* mask, int32_t* target_tm, float* mask_sum, float* mask_sum_copy, s2vt_stream stream)
{
    if (!ids || N <= 0 || Tc <= 0) return S2VT_E_BADARG;
    HIP_TRY(launch_caption_mask(ids, N, Tc, mask, target_tm, mask_sum, mask_sum_copy, S(stream)));
    return S2VT_OK;
}

int s2vt_pg_coef(const float* mask, const float* rewards, const float* baseline, float scale, int32_t N, int32_t Tc, float* coef_tm,
                 s2vt_stream stream)
{
    if (!mask || !coef_tm || N <= 0 || Tc <= 0) return S2VT_E_BADARG;
    HIP_TRY(launch_pg_coef(mask, rewards, baseline, scale, N, Tc, coef_tm, S(stream)));
    return S2VT_OK;
}

int s2vt_xe_prep(const float* mask, const int32_t* caption, int32_t N, int32_t Tc, float loss_weight, float n_global, int32_t q1, float* coef_tm,
                 int32_t* target_tm, float* mask_sum, s2vt_stream stream)
{
    if (!mask || !coef_tm || (target_tm && !caption) || N <= 0 || Tc <= 0 || Tc > 128 || !(n_global > 0.0f)) return S2VT_E_BADARG;
    HIP_TRY(launch_xe_prep(mask, caption, N, Tc, loss_weight, n_global, q1, coef_tm, target_tm, mask_sum, S(stream)));
    return S2VT_OK;
}

int s2vt_mixed_prep(const float* mask, const float* gt_mask, const float* rewards, const float* baseline, const int32_t* sampled,
                    const int32_t* gt_caption, int32_t Ns, int32_t B, int32_t Tc, double lambda_loss, float loss_weight, int32_t q1,
                    float smoothing, float n_global_b, float* coef_tm, float* smooth_tm, int32_t* caption_all, int32_t* target_tm, float* sums, s2vt_stream stream)
{
    if (!mask || !gt_mask || !rewards || !baseline || !sampled || !gt_caption || !coef_tm || !smooth_tm || !caption_all || !target_tm || !sums) return S2VT_E_BADARG;
    if (Ns <= 0 || B <= 0 || Tc <= 0 || Tc > 128 || !(n_global_b > 0.0f)) return S2VT_E_BADARG;
    HIP_TRY(launch_mixed_prep(mask, gt_mask, rewards, baseline, sampled, gt_caption, Ns, B, Tc, (float)(1.0 - lambda_loss), (float)lambda_loss,
                              loss_weight, q1, smoothing, n_global_b, coef_tm, smooth_tm, caption_all, target_tm, sums, S(stream)));
    return S2VT_OK;
}

int s2vt_mixed_loss(const float* coef, const float* nll, const int32_t* live_rows, int64_t R, int32_t N, int32_t Ns, float* out3, s2vt_stream stream)
{
    if (!coef || !nll || !out3 || R < 0 || R > 0x7fffffff || N <= 0 || Ns < 0 || Ns > N) return S2VT_E_BADARG;
    HIP_TRY(launch_mixed_loss(coef, nll, live_rows, (int)R, N, Ns, out3, S(stream)));
    return S2VT_OK;
}

int s2vt_gemm_nt_splitk(const float* A, int32_t lda, const float* Wt, int32_t ldw, float* C, int32_t ldc, int32_t M, int32_t N,
                        int32_t K, int32_t splits, int32_t tile_cfg, float* slabs, size_t slab_floats, s2vt_stream stream)
{
    if (!A || !Wt || !C || M < 0 || N <= 0 || K <= 0 || lda < K || ldw < K || ldc < N || splits < 0 || splits > 64) return S2VT_E_BADARG;
    if (M == 0) return S2VT_OK;
    hipStream_t st = S(stream);
    int s = splits == 0 ? dx_splits(M, N, K) : splits;
    if (s > 1 && (ldc != N || !slabs)) { if (splits) return S2VT_E_BADARG; s = 1; }
    if (s <= 1) { HIP_TRY(nn_bwd(A, lda, Wt, ldw, C, ldc, M, N, K, 1, 0, st, tile_cfg)); return S2VT_OK; }
    const size_t stride = (size_t)M * N;
    const int kper = ((K + s - 1) / s + BK - 1) / BK * BK, nslab = (K + kper - 1) / kper;     // what nn_bwd makes of `s`
    if ((size_t)nslab * stride > slab_floats) return S2VT_E_WORKSPACE;
    HIP_TRY(nn_bwd(A, lda, Wt, ldw, slabs, N, M, N, K, s, stride, st, tile_cfg >= 0 ? tile_cfg : kSlabTileCfg));
    HIP_TRY(launch_sum_slabs(C, slabs, nslab, stride, stride, st));
    return S2VT_OK;
}

int s2vt_step_scalars(const float* coef, const float* nll, int64_t R, const float* mask_sum_local, const float* mask_sum_global, float* loss,
                      float* gscale, float* sumsq, s2vt_stream stream)
{
    if (R < 0 || ((coef == nullptr) != (nll == nullptr))) return S2VT_E_BADARG;
    HIP_TRY(launch_step_scalars(coef, nll, R, mask_sum_local, mask_sum_global, loss, gscale, sumsq, S(stream)));
    return S2VT_OK;
}

int s2vt_softmax_nll_fwd_bwd(float* logits, int32_t ld, int32_t R, int32_t V, const int32_t* target, const float* coef,
                             float smoothing, float* nll, float* lp_target, s2vt_stream stream)
{
    if (!logits || !target || !coef || R < 0 || V <= 0 || ld < V) return S2VT_E_BADARG;
    HIP_TRY(launch_softmax_nll(logits, ld, R, V, target, coef, smoothing, nll, lp_target, S(stream)));
    return S2VT_OK;
}

int s2vt_softmax_unshifted_argmax(const float* logits, int32_t ld, int32_t R, int32_t V, int32_t* ids, float* probs,
                                  s2vt_stream stream)
{
    if (!logits || !ids || R < 0 || V <= 0 || ld < V) return S2VT_E_BADARG;
    HIP_TRY(launch_softmax_unshifted_argmax(logits, ld, R, V, ids, probs, S(stream)));
    return S2VT_OK;
}

int s2vt_softmax_nll_fwd_bwd_rows(float* logits, int32_t ld, int32_t R, int32_t V, const int32_t* target, const float* coef,
                                  const float* smoothing_rows, float* nll, float* lp_target, s2vt_stream stream)
{
    if (!logits || !target || !coef || !smoothing_rows || R < 0 || V <= 0 || ld < V) return S2VT_E_BADARG;
    HIP_TRY(launch_softmax_nll(logits, ld, R, V, target, coef, 0.0f, nll, lp_target, S(stream), smoothing_rows));
    return S2VT_OK;
}

int s2vt_bptt_bwd(const s2vt_dims* d, const s2vt_params* p, const s2vt_params* grads, const float* video, int32_t B,
                  int32_t N, const float* dlogits, float keep, uint64_t seed, const int32_t* video_id,
                  const int32_t* sample_id, void* workspace, size_t workspace_bytes, s2vt_stream stream)
{
    return s2vt_bptt_bwd_phase(d, p, grads, video, B, N, dlogits, keep, seed, video_id, sample_id, workspace, workspace_bytes, 0,
                               stream);
}

int s2vt_bptt_bwd_phase(const s2vt_dims* d, const s2vt_params* p, const s2vt_params* grads, const float* video, int32_t B,
                        int32_t N, const float* dlogits, float keep, uint64_t seed, const int32_t* video_id,
                        const int32_t* sample_id, void* workspace, size_t workspace_bytes, int32_t phase, s2vt_stream stream)
{
    return s2vt_bptt_bwd_steps(d, p, grads, video, B, N, dlogits, d ? d->n_caption_lstm_step : 0, keep, seed, video_id, sample_id,
                               workspace, workspace_bytes, phase, stream);
}

int s2vt_bptt_bwd_steps(const s2vt_dims* d, const s2vt_params* p, const s2vt_params* grads, const float* video, int32_t B,
                        int32_t N, const float* dlogits, int32_t caption_steps, float keep, uint64_t seed,
                        const int32_t* video_id, const int32_t* sample_id, void* workspace, size_t workspace_bytes, int32_t phase,
                        s2vt_stream stream)
{
    return s2vt_bptt_bwd_live(d, p, grads, video, B, N, dlogits, caption_steps, nullptr, 0, keep, seed, video_id, sample_id, workspace,
                              workspace_bytes, phase, stream);
}

// Precision of the backward's gradient contractions: fp32 MFMA (s2vt_bptt_bwd_live), bf16 operands (s2vt_bptt_bwd_bf16), or
// split-bf16 operands, three bf16 products per product (s2vt_bptt_bwd_split)
enum GradMode { kGradFp32 = 0, kGradBf16 = 1, kGradSplit = 2 };

// s2vt_bptt_bwd_split's dispatch: the split products where the unrolled rows exceed the gated side stream's 256 (all of that
// step's contractions -- the REINFORCE shapes); at <= 256 rows the fp32 body with its side-stream overlap.  S2VT_SPLIT_GRADS=0: the
// fp32 body at every shape (read once).
static int split_grad_mode(int N)
{
    static const int on = [] { const char* e = getenv("S2VT_SPLIT_GRADS"); return e ? atoi(e) : 1; }();
    return on && N > 256 ? kGradSplit : kGradFp32;
}
static bool split_mode_on(int N) { return split_grad_mode(N) == kGradSplit; }
// ... and LSTM2's backward recurrence with them, where its register-weights form serves the shape (bwd_chain_split_serves: above 256 rows).
// S2VT_BCHAIN_SPLIT=0 (dev knob, read once): the fp32 recurrence beside the split products.
static bool split_recurrence()
{
    static const bool on = [] { const char* e = getenv("S2VT_BCHAIN_SPLIT"); return !(e && e[0] == '0'); }();
    return on;
}

// Phases of the backward (the ABI's `phase`, 0 to 4), for data-parallel callers that start a slice's all-reduce as soon as its gradients
// are final:  kVocab = the vocab projection (embed_word_W / _b final);  kLstm2 = LSTM2's recurrence + its weight gradients (lstm2_W / _b
// final);  kRest = everything after (dX2, LSTM1, Wemb, frame embedding);  kLstm2AndRest = kLstm2 + kRest;  kAll = all.
enum BwdPhase { kAll = 0, kVocab = 1, kLstm2AndRest = 2, kLstm2 = 3, kRest = 4 };

// A weight gradient C[M, N] += A[rows, M]^T B[rows, N] (+ colsum += B's column sums); idx: A's rows gathered out of a table of gather_rows
// rows (0 = not stated)
static TnArgs tn(const float* A, const int32_t* idx, int gather_rows, int lda, const float* B, int ldb, float* C, int ldc, int rows, int M, int N,
                 float* colsum = nullptr)
{
    return TnArgs{A, idx, lda, B, ldb, C, ldc, rows, M, N, 1, colsum, gather_rows};
}

// One backward call: what every stage reads (filled once by bptt_bwd_body, which is the driver) and the stages themselves.  Each of the
// four product stages -- vocab projection, LSTM2's weight gradients, dX2, LSTM1's tail -- has one straight-line function per
// implementation: *_fp32 (fp32 MFMA; the live-row list, when given, cuts the decode steps down to a second, packed contraction),
// *_tr (bf16 / split-bf16 on transposed operands: tr + mm) and *_fused (split-bf16 on operands by rows: rows / rows1 + mmt).  The bf16
// scratch is reused in stream order, so the order of casts and products inside a stage is part of it.
struct BpttBwd {
    SideStream& ss;
    int H, E, V, D, Tv, Tc, T, B, N;     // (Tc, T: the steps the forward call unrolled)
    int K4, Re, Rd;                      // bf16_pad(4 H); rows of the N-row products: encode steps | decode steps (the live rows when listed)
    size_t NH; TrainWs w; Bf16Ws bw;
    const s2vt_params *p, *grads; const float *video, *dlogits; const int32_t* live_rows; int n_live;
    float keep; uint64_t seed; const int32_t *video_id, *sample_id;
    // The embedding operand of LSTM2's decode steps as (table, row index, table rows): row r of the operand is row emb_idx[r] of emb_tab
    // (emb_idx NULL: row r itself).  (Wemb, prev, V) in every teacher-forced backward; (Xbar, none, Tc N) in the averaged one, whose
    // operand is no row of Wemb -- there emb_ida / emb_idb are the two rows of Wemb each operand row is the mean of (NULL otherwise).
    const float* emb_tab; const int32_t* emb_idx; int emb_rows; const int32_t *emb_ida, *emb_idb;
    // (the top-k unroll: each operand row is sum_j emb_wk[r][j] Wemb[emb_idk[r][j]] over emb_k ids -- NULL / 0 otherwise)
    const int32_t* emb_idk; const float* emb_wk; int emb_k;
    bool bf16, split, fused;             // bf16: either bf16 mode; fused: the split mode without transposed operands (carve_bf16)
    hipStream_t st, sd, sv;              // the caller's; LSTM2's weight gradients' and the deferred dWout's; the vocab stage's dWout's
    bool gate1, gate2;                   // gated overlap beside LSTM1's / LSTM2's recurrence

    // the decode rows of dZ2 (live: the packed copy the LSTM2 phase left in the workspace)
    const float* dzd() const { return live_rows ? w.dZ2p : w.dZ2 + (size_t)Tv * 4 * NH; }

    // ---- bf16 / split mode: each operand of a gradient contraction is cast once (a shared one serves every product that reads it; split:
    // its hi and lo planes from one read), then gemm_bf16_nt / gemm_bf16x3_nt; the recurrences, dropout reductions and the embedding
    // scatter stay as they are.  Everything on the caller's stream.
    uint16_t* lo(uint16_t* hi) const { return split && hi ? hi + bw.lo_delta : nullptr; }
    hipError_t tr(const float* src, int ld, const int32_t* idx, int R, int C, uint16_t* dst, int ldd, float* colsum = nullptr,
                  uint16_t* rdst = nullptr, int rldd = 0) const
    {
        CastTrArgs a{src, ld, idx, R, C, dst, ldd, bf16_pad(R), colsum, bw.part, rdst, rldd, lo(dst), lo(rdst)};
        return launch_cast_tr_bf16(a, st);
    }
    hipError_t rows(const float* src, int ld, const int32_t* idx, int R, int K, uint16_t* dst, int ldd) const
    {
        return launch_cast_rows_bf16(src, ld, idx, R, K, dst, ldd, st, lo(dst));
    }
    // (acc = 1: a weight gradient, accumulated into its buffer; 0: a data gradient)
    hipError_t mm(uint16_t* A, int lda, uint16_t* Bm, int ldb, float* Cm, int ldc, int M, int Nn, int Kp, int acc) const
    {
        if (split)
            return launch_gemm_bf16x3_nt(A, lo(A), lda, Bm, lo(Bm), ldb, Cm, ldc, M, Nn, Kp, acc, bw.kpart, bw.kpart_floats, acc ? 3 : 4, st);
        return launch_gemm_bf16_nt(A, lda, Bm, ldb, Cm, ldc, M, Nn, Kp, acc, 0, st);
    }
    // fused split mode: a weight gradient from operands by rows, C[M, Nn] += A[K rows][M]^T B[K rows][Nn] (+ bias += B's column sums through
    // the ones column that rows1 puts behind A's M columns)
    hipError_t rows1(const float* src, int ld, const int32_t* idx, int R, int K, uint16_t* dst, int ldd) const
    {
        return launch_cast_rows_bf16(src, ld, idx, R, K, dst, ldd, st, lo(dst), 1);
    }
    hipError_t mmt(uint16_t* A, int lda, uint16_t* Bm, int ldb, float* Cm, int ldc, int M, int Nn, int K, float* bias) const
    {
        return launch_gemm_bf16x3_tn(A, lo(A), lda, Bm, lo(Bm), ldb, Cm, ldc, M, Nn, K, 1, bias, bw.kpart, bw.kpart_floats, 3, st);
    }

    // ---- steps shared between stages
    // n packed rows (row r belonging to row live_rows[r] of dst) into dst, every other row of it zero
    hipError_t scatter_into_zeroed(const float* packed, int ld, int n, float* dst, size_t bytes) const
    {
        ZeroList z;
        z.add(dst, bytes);
        const hipError_t e = launch_zero_regions(z, st);
        return e != hipSuccess ? e : launch_scatter_rows(packed, ld, live_rows, n, ld, dst, ld, st);
    }
    // embedding rows (gradient of tf.nn.embedding_lookup): scatter-add of the embed slice of dX2
    // (averaged: half of each row's gradient into either row of its id pair, average_generate_words_tf_s2vt.py:131-133)
    // (top-k: each row's gradient, weighed, into its k rows, sum_generate_words_tf_s2vt.py:171-173)
    hipError_t wemb_scatter_add() const
    {
        if (emb_idk)
            return launch_scatter_add_rowsk(w.dX2 + (size_t)Tv * N * (H + E) + H, H + E, emb_idk, emb_wk, emb_k, Tc * N, E, grads->Wemb, E, st);
        if (emb_ida)
            return launch_scatter_add_rows2(w.dX2 + (size_t)Tv * N * (H + E) + H, H + E, emb_ida, emb_idb, 0.5f, Tc * N, E, grads->Wemb, E, st);
        if (live_rows) return launch_scatter_add_rows(w.dX2p + H, H + E, w.prevp, n_live, E, grads->Wemb, E, st);
        return launch_scatter_add_rows(w.dX2 + (size_t)Tv * N * (H + E) + H, H + E, emb_idx, Tc * N, E, grads->Wemb, E, st);
    }
    // dZ2 by rows into L, [encode steps | decode steps]: the B operand of the fused LSTM2 products and dX2's A
    hipError_t cast_dz2_rows() const
    {
        HIP_CHECK(rows(w.dZ2, 4 * H, nullptr, Re, 4 * H, bw.L, K4));
        return rows(dzd(), 4 * H, nullptr, Rd, 4 * H, bw.L + (size_t)Re * K4, K4);
    }

    // ---- vocab projection: dWout (+ the bias gradient) = O2^T dlogits and dO2 = dlogits Wout^T -> dO2t.  R rows: every unrolled
    // (step, row) pair, or the LIVE ones only (dlogits is then [n_live, V], row r belonging to row live_rows[r] of the unroll; the masked
    // rows' dlogits are exact zeros in the full form, so leaving them out of the reductions changes nothing and their dO2 rows are the
    // zeros the driver writes)
    hipError_t vocab_fused(int R, float* dO2t) const
    {
        // dlogits by rows, once (or there already): dWout's B (K-major; + the bias gradient) and dO2's A
        const int Kv = bf16_pad(V), Hp1 = bf16_pad(H + 1);
        if (dlogits) HIP_CHECK(rows(dlogits, V, nullptr, R, V, bw.L, Kv));
        HIP_CHECK(rows1(w.O2 + (size_t)Tv * NH, H, live_rows, R, H, bw.AT, Hp1));
        HIP_CHECK(mmt(bw.AT, Hp1, bw.L, Kv, grads->embed_word_W, V, H, V, R, grads->embed_word_b));
        HIP_CHECK(rows(p->embed_word_W, V, nullptr, H, V, bw.W, Kv));
        return mm(bw.L, Kv, bw.W, Kv, dO2t, H, R, H, Kv, 0);
    }
    hipError_t vocab_tr(int R, float* dO2t) const
    {
        // dlogits once, in both forms: transposed (dWout's B, + the bias gradient) and by rows (dO2's A)
        const int Kr = bf16_pad(R), Kv = bf16_pad(V);
        HIP_CHECK(tr(dlogits, V, nullptr, R, V, bw.BT, Kr, grads->embed_word_b, bw.L, Kv));
        HIP_CHECK(tr(w.O2 + (size_t)Tv * NH, H, live_rows, R, H, bw.AT, Kr));
        HIP_CHECK(mm(bw.AT, Kr, bw.BT, Kr, grads->embed_word_W, V, H, V, Kr, 1));
        HIP_CHECK(rows(p->embed_word_W, V, nullptr, H, V, bw.W, Kv));
        return mm(bw.L, Kv, bw.W, Kv, dO2t, H, R, H, Kv, 0);
    }
    // (deferred != NULL: dWout is handed back for the driver to launch behind LSTM2's recurrence instead)
    hipError_t vocab_fp32(int R, float* dO2t, TnArgs* deferred) const
    {
        // the bias gradient rides in the same pass over dlogits
        const TnArgs a = tn(w.O2 + (size_t)Tv * NH, live_rows, live_rows ? Tc * N : 0, H, dlogits, V, grads->embed_word_W, V, R, H, V, grads->embed_word_b);
        if (deferred) *deferred = a;
        else HIP_CHECK(launch_gemm_tn(a, sv));
        int s2 = w.dO2s ? do2_splits(R, H, V) : 1;
        if ((size_t)s2 * R > w.dO2s_rows) s2 = 1;            // (a live-row count between two step counts the carve did not see)
        if (s2 > 1) {
            const size_t stride = (size_t)R * H;
            HIP_CHECK(nn_bwd(dlogits, V, p->embed_word_W, V, w.dO2s, H, R, H, V, s2, stride, st, kSlabTileCfg));
            const int kper = ((V + s2 - 1) / s2 + BK - 1) / BK * BK;       // what nn_bwd made of `splits`
            return launch_sum_slabs(dO2t, w.dO2s, (V + kper - 1) / kper, stride, stride, st);
        }
        return nn_bwd(dlogits, V, p->embed_word_W, V, dO2t, H, R, H, V, 1, 0, st);
    }

    // ---- LSTM2's weight gradients over [encode steps | decode steps (live: the packed live rows)]: out1, the embedding rows of the previous
    // words (decode segment only) and h2 against dZ2, lstm2_b with the last.  On sd: beside dX2 and LSTM1's recurrence, or (gated) launched
    // by the driver behind LSTM1's recurrence.
    hipError_t l2_grads_fused() const
    {
        // dZ2 once, by rows: the B operand of all three products (+ lstm2_b with the last) and dX2's A (phase 4); out1 / h2 by rows over
        // the same two segments, the embedding rows over the decode one
        const int Hp = bf16_pad(H), Hp1 = bf16_pad(H + 1), Ep = bf16_pad(E);
        HIP_CHECK(cast_dz2_rows());
        HIP_CHECK(rows(w.O1, H, nullptr, Re, H, bw.AT, Hp));
        HIP_CHECK(rows(w.O1 + (size_t)Tv * NH, H, live_rows, Rd, H, bw.AT + (size_t)Re * Hp, Hp));
        HIP_CHECK(mmt(bw.AT, Hp, bw.L, K4, grads->lstm2_W, 4 * H, H, 4 * H, Re + Rd, nullptr));
        HIP_CHECK(rows(emb_tab, E, live_rows ? w.prevp : emb_idx, Rd, E, bw.AT, Ep));                 // Wemb [V, E] rows of the previous words
        HIP_CHECK(mmt(bw.AT, Ep, bw.L + (size_t)Re * K4, K4, grads->lstm2_W + (size_t)H * 4 * H, 4 * H, E, 4 * H, Rd, nullptr));
        HIP_CHECK(rows1(w.H2, H, nullptr, Re, H, bw.AT, Hp1));
        HIP_CHECK(rows1(w.H2 + (size_t)Tv * NH, H, live_rows, Rd, H, bw.AT + (size_t)Re * Hp1, Hp1));
        return mmt(bw.AT, Hp1, bw.L, K4, grads->lstm2_W + (size_t)(H + E) * 4 * H, 4 * H, H, 4 * H, Re + Rd, grads->lstm2_b);
    }
    hipError_t l2_grads_tr() const
    {
        // dZ2 once: transposed -- the B operand of all three products, + lstm2_b -- and by rows (dX2's A, phase 4)
        const int ke = bf16_pad(Re), Kd = bf16_pad(Rd), Kt = ke + Kd;
        HIP_CHECK(tr(w.dZ2, 4 * H, nullptr, Re, 4 * H, bw.BT, Kt, grads->lstm2_b, bw.L, K4));
        HIP_CHECK(tr(dzd(), 4 * H, nullptr, Rd, 4 * H, bw.BT + ke, Kt, grads->lstm2_b, bw.L + (size_t)Re * K4, K4));
        HIP_CHECK(tr(w.O1, H, nullptr, Re, H, bw.AT, Kt));
        HIP_CHECK(tr(w.O1 + (size_t)Tv * NH, H, live_rows, Rd, H, bw.AT + ke, Kt));
        HIP_CHECK(mm(bw.AT, Kt, bw.BT, Kt, grads->lstm2_W, 4 * H, H, 4 * H, Kt, 1));
        HIP_CHECK(tr(emb_tab, E, live_rows ? w.prevp : emb_idx, Rd, E, bw.AT, Kd));                   // Wemb [V, E] rows of the previous words
        HIP_CHECK(mm(bw.AT, Kd, bw.BT + ke, Kt, grads->lstm2_W + (size_t)H * 4 * H, 4 * H, E, 4 * H, Kd, 1));
        HIP_CHECK(tr(w.H2, H, nullptr, Re, H, bw.AT, Kt));
        HIP_CHECK(tr(w.H2 + (size_t)Tv * NH, H, live_rows, Rd, H, bw.AT + ke, Kt));
        return mm(bw.AT, Kt, bw.BT, Kt, grads->lstm2_W + (size_t)(H + E) * 4 * H, 4 * H, H, 4 * H, Kt, 1);
    }
    hipError_t l2_grads_fp32() const
    {
        float* const gO1 = grads->lstm2_W, *const gEmb = gO1 + (size_t)H * 4 * H, *const gH2 = gO1 + (size_t)(H + E) * 4 * H;
        if (!live_rows) {
            HIP_CHECK(launch_gemm_tn(tn(w.O1, nullptr, 0, H, w.dZ2, 4 * H, gO1, 4 * H, T * N, H, 4 * H), sd));
            HIP_CHECK(launch_gemm_tn(tn(emb_tab, emb_idx, emb_idx ? emb_rows : 0, E, dzd(), 4 * H, gEmb, 4 * H, Tc * N, E, 4 * H), sd));
            return launch_gemm_tn(tn(w.H2, nullptr, 0, H, w.dZ2, 4 * H, gH2, 4 * H, T * N, H, 4 * H, grads->lstm2_b), sd);
        }
        // Live rows: behind its first <eos> a row's dZ2 is an exact zero at every later step (zero upstream gradient, zero carried
        // dh / dc), so the weight gradients are reduced over the Tv encode steps (every row) plus the LIVE decode rows -- their
        // dZ2 rows as a packed copy, the matching activation rows gathered through the same list.
        HIP_CHECK(launch_gemm_tn(tn(w.O1, nullptr, 0, H, w.dZ2, 4 * H, gO1, 4 * H, Re, H, 4 * H), sd));
        HIP_CHECK(launch_gemm_tn(tn(w.O1 + (size_t)Tv * NH, live_rows, Tc * N, H, w.dZ2p, 4 * H, gO1, 4 * H, Rd, H, 4 * H), sd));
        HIP_CHECK(launch_gemm_tn(tn(emb_tab, w.prevp, emb_rows, E, w.dZ2p, 4 * H, gEmb, 4 * H, Rd, E, 4 * H), sd));
        HIP_CHECK(launch_gemm_tn(tn(w.H2, nullptr, 0, H, w.dZ2, 4 * H, gH2, 4 * H, Re, H, 4 * H, grads->lstm2_b), sd));
        return launch_gemm_tn(tn(w.H2 + (size_t)Tv * NH, live_rows, Tc * N, H, w.dZ2p, 4 * H, gH2, 4 * H, Rd, H, 4 * H, grads->lstm2_b), sd);
    }
    // (one name for the driver's two call sites: at once, or deferred behind LSTM1's recurrence)
    hipError_t l2_grads() const
    {
        // (planes too large for the K-major loader's 32-bit offsets: the transposed form)
        if (fused && gemm_bf16x3_tn_ok(bf16_pad(H + 1) > bf16_pad(E) ? bf16_pad(H + 1) : bf16_pad(E), K4, Re + Rd)) return l2_grads_fused();
        return bf16 ? l2_grads_tr() : l2_grads_fp32();
    }

    // ---- d[out1 ; embed] for every step at once -- with live rows: the encode steps, then the live decode rows (from the packed dZ2
    // of the LSTM2 phase), scattered into the zeroed decode part
    // (one function for the three bf16 forms: mm picks the product.  recast: phase 4 alone -- the row form phase 3 made, again)
    hipError_t dx2_bf16(bool recast) const
    {
        if (recast) HIP_CHECK(cast_dz2_rows());
        HIP_CHECK(rows(p->lstm2_W, 4 * H, nullptr, H + E, 4 * H, bw.W, K4));
        if (!live_rows) return mm(bw.L, K4, bw.W, K4, w.dX2, H + E, T * N, H + E, K4, 0);
        HIP_CHECK(mm(bw.L, K4, bw.W, K4, w.dX2, H + E, Re, H + E, K4, 0));
        HIP_CHECK(mm(bw.L + (size_t)Re * K4, K4, bw.W, K4, w.dX2p, H + E, Rd, H + E, K4, 0));
        return scatter_into_zeroed(w.dX2p, H + E, n_live, w.dX2 + (size_t)Tv * N * (H + E), (size_t)Tc * N * (H + E) * 4);
    }
    hipError_t dx2_fp32() const
    {
        if (!live_rows) return nn_bwd_slabs(w.dZ2, 4 * H, p->lstm2_W, 4 * H, w.dX2, H + E, T * N, H + E, 4 * H, w.dXs, st, w.dXs_floats);
        HIP_CHECK(nn_bwd_slabs(w.dZ2, 4 * H, p->lstm2_W, 4 * H, w.dX2, H + E, Tv * N, H + E, 4 * H, w.dXs, st, w.dXs_floats));
        HIP_CHECK(nn_bwd_slabs(w.dZ2p, 4 * H, p->lstm2_W, 4 * H, w.dX2p, H + E, n_live, H + E, 4 * H, w.dXs, st, w.dXs_floats));
        return scatter_into_zeroed(w.dX2p, H + E, n_live, w.dX2 + (size_t)Tv * N * (H + E), (size_t)Tc * N * (H + E) * 4);
    }

    // ---- LSTM1's tail: dX1, LSTM1's weight gradients over all unrolled steps, the embedding scatter-add, the frame embedding
    hipError_t lstm1_tail_bf16() const
    {
        // dZ1 once: transposed over [encode steps | decode steps] (+ lstm1_b), and the encode rows by rows (dX1's A)
        const int Re1 = Tv * B, Rd1 = Tc * B, ke = bf16_pad(Re1), K1 = ke + bf16_pad(Rd1);
        HIP_CHECK(tr(w.dZ1, 4 * H, nullptr, Re1, 4 * H, bw.BT, K1, grads->lstm1_b, bw.L, K4));
        HIP_CHECK(tr(w.dZ1 + (size_t)Re1 * 4 * H, 4 * H, nullptr, Rd1, 4 * H, bw.BT + ke, K1, grads->lstm1_b));
        HIP_CHECK(rows(p->lstm1_W, 4 * H, nullptr, E, 4 * H, bw.W, K4));
        HIP_CHECK(mm(bw.L, K4, bw.W, K4, w.dX1, E, Re1, E, K4, 0));
        HIP_CHECK(tr(w.emb, E, w.encidx, Re1, E, bw.AT, ke));                                         // the frame embedding, time-major
        HIP_CHECK(mm(bw.AT, ke, bw.BT, K1, grads->lstm1_W, 4 * H, E, 4 * H, ke, 1));
        HIP_CHECK(tr(w.H1, H, nullptr, Re1, H, bw.AT, K1));
        HIP_CHECK(tr(w.H1 + (size_t)Re1 * H, H, nullptr, Rd1, H, bw.AT + ke, K1));
        HIP_CHECK(mm(bw.AT, K1, bw.BT, K1, grads->lstm1_W + (size_t)E * 4 * H, 4 * H, H, 4 * H, K1, 1));
        HIP_CHECK(wemb_scatter_add());
        HIP_CHECK(tr(video, D, w.encidx, Re1, D, bw.AT, ke));
        HIP_CHECK(tr(w.dX1, E, nullptr, Re1, E, bw.BT, ke, grads->encode_image_b));
        return mm(bw.AT, ke, bw.BT, ke, grads->encode_image_W, E, D, E, ke, 1);
    }
    // (the split mode's too: LSTM1's contractions -- B rows, not N: dX1 [Tv B, E], the weight gradients over (Tv + Tc) B rows -- stay on
    // fp32 MFMA)
    hipError_t lstm1_tail_fp32() const
    {
        HIP_CHECK(nn_bwd_slabs(w.dZ1, 4 * H, p->lstm1_W, 4 * H, w.dX1, E, Tv * B, E, 4 * H, w.dXs, st, w.dXs_floats));
        HIP_CHECK(launch_gemm_tn(tn(w.emb, w.encidx, Tv * B, E, w.dZ1, 4 * H, grads->lstm1_W, 4 * H, Tv * B, E, 4 * H), st));
        HIP_CHECK(launch_gemm_tn(tn(w.H1, nullptr, 0, H, w.dZ1, 4 * H, grads->lstm1_W + (size_t)E * 4 * H, 4 * H, T * B, H, 4 * H, grads->lstm1_b), st));
        HIP_CHECK(wemb_scatter_add());
        return launch_gemm_tn(tn(video, w.encidx, Tv * B, D, w.dX1, E, grads->encode_image_W, E, Tv * B, D, E, grads->encode_image_b), st);
    }
};

// The backward of s2vt_bptt_bwd_live; mode != kGradFp32: its gradient contractions on bf16 / split-bf16 operands, bf16_ws their scratch.
// The driver only: validate and carve; streams, gates and the side-stream lock; then the stages of BpttBwd in the order of the phases --
// vocab projection | LSTM2's recurrence (the deferred dWout beside it), live-row gathers, LSTM2's weight gradients (now, or deferred
// beside LSTM1's recurrence) | dX2, dropout reduction + LSTM1's recurrence, LSTM1's tail -- and ONE successful exit, through the join.
// The bf16 and split modes never fork (their SideStream is a local one with ok = false, so sd == sv == st): for them, and for the
// single-phase calls, `sd != st` makes the join nothing.
static int bptt_bwd_body(const s2vt_dims* d, const s2vt_params* p, const s2vt_params* grads, const float* video, int32_t B,
                         int32_t N, const float* dlogits, int32_t caption_steps, const int32_t* live_rows, int32_t n_live, float keep,
                         uint64_t seed, const int32_t* video_id, const int32_t* sample_id, void* workspace, size_t workspace_bytes,
                         int32_t phase, int mode, void* bf16_ws, size_t bf16_ws_bytes, s2vt_stream stream, const AvgScratch* avg = nullptr)
{
    const int bf16 = mode != kGradFp32;
    const bool split = mode == kGradSplit;
    if ((live_rows == nullptr) != (n_live == 0) || n_live < 0) return S2VT_E_BADARG;
    if (bf16 && !bf16_ws) return S2VT_E_BADARG;
    if (phase < kAll || phase > kRest) return S2VT_E_BADARG;
    const bool fused = split && split_fused();               // no transposed operands: K-major weight gradients (carve_bf16)
    // (fused split mode: dlogits == NULL = its planes are in bf16_ws already, s2vt_softmax_nll_fwd_bwd_split -- read by the vocabulary
    //  phase only; phases 2 to 4 never look at dlogits and take the same NULL from a caller that runs the phases one by one)
    if (!dlogits && !fused) return S2VT_E_BADARG;
    if (!dims_ok_res(d) || !params_ok(p) || !params_ok(grads) || !video || !workspace || B <= 0 || N <= 0 || N % B)
        return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    if (bf16_ws && (reinterpret_cast<uintptr_t>(bf16_ws) & 255u)) return S2VT_E_ALIGN;
    if (chain_fault()) return S2VT_E_CHAIN_TIMEOUT;
    if (caption_steps < 1 || caption_steps > d->n_caption_lstm_step) return S2VT_E_BADARG;
    if (live_rows && (n_live > caption_steps * N || ((d->lstm_dim | d->word_dim) & 3))) return S2VT_E_BADARG;
    if (avg && (live_rows || caption_steps != d->n_caption_lstm_step || is_residual(d))) return S2VT_E_BADARG;   // (the averaged unroll is whole and plain)
    // the steps the forward call unrolled (s2vt_teacher_forced_fwd_steps): later steps carry no gradient, so the
    // recurrences start from zero at step T - 1 and every contraction covers the leading T (Tc) steps only
    const int H = d->lstm_dim, E = d->word_dim, V = d->n_words, Tv = d->n_video_lstm_step, Tc = caption_steps, T = Tv + Tc;
    Carver c(workspace, workspace_bytes);
    TrainWs w;
    carve_train(c, d, B, N, &w);
    if (!c.ok()) return S2VT_E_WORKSPACE;
    Bf16Ws bw{};
    // (a scratch that came with the call is held to its declared size in every mode: s2vt_bptt_bwd_split's fp32 body -- N <= 256 rows,
    //  or S2VT_SPLIT_GRADS=0 -- never touches split_ws, but a caller whose scratch is too small learns it at the first shape, not the first large one)
    if (bf16_ws) {
        Carver cb(bf16_ws, bf16_ws_bytes);
        carve_bf16(cb, d, B, N, &bw, split || !bf16);
        if (!cb.ok()) return S2VT_E_WORKSPACE;
    }
    hipStream_t st = S(stream);
    const size_t NH = (size_t)N * H;
    const bool do_vocab = phase == kAll || phase == kVocab, do_l2 = phase == kAll || phase == kLstm2AndRest || phase == kLstm2,
               do_rest = phase == kAll || phase == kLstm2AndRest || phase == kRest;

    // ---- streams, gates, the side-stream lock
    SideStream one_stream;                                   // (ok = false: the bf16 mode keeps to the caller's stream)
    SideStream& ss = bf16 ? one_stream : side_stream();
    BpttBwd x{ss};
    // gated overlap (mode 2): only beside recurrences that run as ONE-part persistent grids (<= 256 rows: room for a second wave per SIMD)
    x.gate2 = ss.ok && ss.mode == 2 && phase == kAll && N <= 256 && bwd_chain_auto(N, H) && !(reinterpret_cast<uintptr_t>(p->lstm2_W) & 15);
    // (LSTM1's recurrence is gated only where LSTM2's is: at N > 256 rows -- the REINFORCE step's 320 -- LSTM2's three contractions are 0.6 ms
    //  each and lose more beside the 64-row recurrence than it gains: 12.26 -> 12.28 ms measured, profiles/r05_overlap_ab.jsonl)
    x.gate1 = ss.ok && ss.mode == 2 && phase == kAll && N <= 256 && B <= 256 && bwd_chain_auto(B, H) && !(reinterpret_cast<uintptr_t>(p->lstm1_W) & 15);
    const bool side_on = ss.ok && phase == kAll && (ss.mode == 1 || x.gate1 || x.gate2);
    hipStream_t sd = side_on ? ss.s : st;                    // weight-gradient work that may run beside a recurrence (whole-pass calls only)
    x.H = H; x.E = E; x.V = V; x.D = d->dim_image; x.Tv = Tv; x.Tc = Tc; x.T = T; x.B = B; x.N = N;
    x.K4 = bf16_pad(4 * H); x.Re = Tv * N; x.Rd = live_rows ? n_live : Tc * N; x.NH = NH;
    x.w = w; x.bw = bw; x.p = p; x.grads = grads; x.video = video; x.dlogits = dlogits; x.live_rows = live_rows; x.n_live = n_live;
    x.emb_tab = avg ? avg->xbar : p->Wemb; x.emb_idx = avg ? nullptr : w.prev; x.emb_rows = avg ? Tc * N : V;
    x.emb_ida = avg ? avg->ida : nullptr; x.emb_idb = avg ? avg->idb : nullptr;
    x.emb_idk = nullptr; x.emb_wk = nullptr; x.emb_k = 0;
    x.keep = keep; x.seed = seed; x.video_id = video_id; x.sample_id = sample_id; x.bf16 = bf16; x.split = split; x.fused = fused;
    x.st = st; x.sd = sd; x.sv = (phase == kAll && ss.ok && ss.mode == 1) ? sd : st;   // (phase 1: its gradients must be final on the caller's stream)
    // The side stream and its events are ONE per process: two host threads driving distinct workspaces must not interleave their
    // record / wait pairs (a wait enqueued after the OTHER thread's record of the same event would order this call's side work behind
    // the wrong point).  The lock covers this call's enqueueing only -- the launches themselves are asynchronous as ever.
    std::unique_lock<std::mutex> side_lk(side_stream_mutex(), std::defer_lock);
    if (side_on) side_lk.lock();
    ChainGate gate{ss.s, ss.ev[3], false};
    const BwdScratch sc{w.slab, w.dc, w.bimg, w.bex, w.bsync};

    // ---- vocab projection
    TnArgs dwout;                                            // (mode 2: the vocabulary projection's weight gradient is launched behind LSTM2's recurrence)
    const bool dwout_deferred = x.gate2 && do_l2;            // (a gate means a whole pass on fp32 products: the vocab stage runs, and takes its fp32 form)
    if (do_vocab) {
        if (x.sv != st) HIP_TRY(fork_to(st, x.sv, ss.ev[0]));
        float* const dO2t = live_rows ? w.dO2p : w.dO2;     // where dO2 lands: packed rows are scattered afterwards
        // (planes too large for the K-major loader's 32-bit offsets: the transposed form, which needs dlogits as fp32 -- the split
        //  softmax entry applies the same rule and leaves them so)
        const bool fused_v = fused && gemm_bf16x3_tn_ok(bf16_pad(H + 1), bf16_pad(V), x.Rd);
        if (!fused_v && !dlogits) return S2VT_E_BADARG;
        if (fused_v) HIP_TRY(x.vocab_fused(x.Rd, dO2t));
        else if (bf16) HIP_TRY(x.vocab_tr(x.Rd, dO2t));
        else HIP_TRY(x.vocab_fp32(x.Rd, dO2t, dwout_deferred ? &dwout : nullptr));
        if (live_rows) HIP_TRY(x.scatter_into_zeroed(w.dO2p, H, x.Rd, w.dO2, (size_t)Tc * N * H * 4));
    }
    const bool l2_deferred = x.gate1 && do_rest && sd != st;
    if (do_l2) {
        // ---- LSTM2 back through time (one persistent launch up to 128 rows: chain.hip)
        // (live rows: the forward pass of this workspace stopped the rows behind their <eos>, see there -- the same order here)
        const bool rec_live = live_rows && Tc <= 128 && chain_live_capable(N, H);
        if (live_rows && Tc <= 128 && N <= 1024) HIP_TRY(launch_row_order(live_rows, n_live, N, Tv, Tc, w.perm, w.nlive, st));
        if (dwout_deferred) chain_gate_arm(&gate);
        const hipError_t re = lstm_recurrence_bwd(p->lstm2_W, H + E, w.G2, w.C2, w.dO2, NH, H, Tv, w.dZ2, N, H, T, keep, seed, 512u, video_id, sample_id, sc, -1, st,
                                                  rec_live ? w.perm : nullptr, rec_live ? w.nlive : nullptr, split && split_recurrence());
        chain_gate_arm(nullptr);
        HIP_TRY(re);
        if (dwout_deferred) {
            // dWout = O2^T dlogits beside the recurrence (reads dlogits and O2, writes embed_word_W's gradient: nothing the recurrence touches);
            // the gate has put the side stream behind "every workgroup of the grid resident" -- or, when the recurrence took its per-step
            // form after all (a hold, a fault), the side stream simply follows the caller's
            if (!gate.fired) HIP_TRY(fork_to(st, sd, ss.ev[3]));
            HIP_TRY(launch_gemm_tn(dwout, sd));
        }
        // Live rows: the packed copies of the live dZ2 rows / previous words are read on BOTH streams (weight gradients on the side
        // stream, dX2 and the embedding scatter on the caller's), so they are made on the caller's stream, ahead of the fork
        if (live_rows) {
            HIP_TRY(launch_gather_rows(w.dZ2 + (size_t)Tv * 4 * NH, 4 * H, live_rows, n_live, 4 * H, w.dZ2p, 4 * H, st));
            HIP_TRY(launch_gather_i32(x.emb_idx, live_rows, n_live, w.prevp, st));
        }
        // dZ2 is complete: LSTM2's weight gradients go to the side stream, beside dX2 and LSTM1's recurrence (mode 2: beside LSTM1's
        // recurrence only -- launched below once that grid is resident; dX2 keeps the chip to itself)
        if (sd != st) HIP_TRY(fork_to(st, sd, ss.ev[1]));
        if (!l2_deferred) HIP_TRY(x.l2_grads());
    }
    if (do_rest) {
        HIP_TRY(bf16 ? x.dx2_bf16(!do_l2) : x.dx2_fp32());
        // ---- LSTM1 back through time, on the B per-video rows: the gradient w.r.t. its dropped output is
        // first reduced over the rep sample rows of each video (with their dropout masks)
        // (residual model: ds = dlogits Wout^T -- w.dO2, which the vocab stage wrote and nothing since has touched, zeros at the rows a
        //  live-row call does not unroll -- is also the gradient w.r.t. LSTM1's dropped output of the decode steps: d o1 = dX2[:, 0:H] + ds)
        HIP_TRY(launch_reduce_dropout(w.dX2, H + E, w.dH1, T, B, N, H, keep, seed, 256u, video_id, sample_id, st, is_residual(d) ? w.dO2 : nullptr, Tv));
        if (l2_deferred) chain_gate_arm(&gate);
        const hipError_t re = lstm_recurrence_bwd(p->lstm1_W, E, w.G1, w.C1, w.dH1, (size_t)B * H, H, 0, w.dZ1, B, H, T, 1.0f, seed, 0u, nullptr, nullptr, sc, -1, st);
        chain_gate_arm(nullptr);
        HIP_TRY(re);
        if (l2_deferred) HIP_TRY(x.l2_grads());            // beside LSTM1's recurrence (they read dZ2: final since ev[1])
        HIP_TRY(bf16 && !split ? x.lstm1_tail_bf16() : x.lstm1_tail_fp32());
    }
    if (sd != st) HIP_TRY(fork_to(sd, st, ss.ev[2]));        // join: the caller's stream waits for the side stream's gradients
    return S2VT_OK;
}

int s2vt_bptt_bwd_live(const s2vt_dims* d, const s2vt_params* p, const s2vt_params* grads, const float* video, int32_t B,
                       int32_t N, const float* dlogits, int32_t caption_steps, const int32_t* live_rows, int32_t n_live, float keep,
                       uint64_t seed, const int32_t* video_id, const int32_t* sample_id, void* workspace, size_t workspace_bytes,
                       int32_t phase, s2vt_stream stream)
{
    return bptt_bwd_body(d, p, grads, video, B, N, dlogits, caption_steps, live_rows, n_live, keep, seed, video_id, sample_id, workspace,
                         workspace_bytes, phase, 0, nullptr, 0, stream);
}

size_t s2vt_bf16_grad_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t N)
{
    if (!dims_ok_res(d) || B <= 0 || N <= 0 || N % B) return 0;
    Carver c(nullptr, 0);
    return carve_bf16(c, d, B, N, nullptr);
}

int s2vt_bptt_bwd_bf16(const s2vt_dims* d, const s2vt_params* p, const s2vt_params* grads, const float* video, int32_t B,
                       int32_t N, const float* dlogits, int32_t caption_steps, const int32_t* live_rows, int32_t n_live, float keep,
                       uint64_t seed, const int32_t* video_id, const int32_t* sample_id, void* workspace, size_t workspace_bytes,
                       int32_t phase, void* bf16_ws, size_t bf16_ws_bytes, s2vt_stream stream)
{
    return bptt_bwd_body(d, p, grads, video, B, N, dlogits, caption_steps, live_rows, n_live, keep, seed, video_id, sample_id, workspace,
                         workspace_bytes, phase, 1, bf16_ws, bf16_ws_bytes, stream);
}

size_t s2vt_split_grad_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t N)
{
    if (!dims_ok_res(d) || B <= 0 || N <= 0 || N % B) return 0;
    Carver c(nullptr, 0);
    return carve_bf16(c, d, B, N, nullptr, true);
}

int s2vt_bptt_bwd_split(const s2vt_dims* d, const s2vt_params* p, const s2vt_params* grads, const float* video, int32_t B,
                        int32_t N, const float* dlogits, int32_t caption_steps, const int32_t* live_rows, int32_t n_live, float keep,
                        uint64_t seed, const int32_t* video_id, const int32_t* sample_id, void* workspace, size_t workspace_bytes,
                        int32_t phase, void* split_ws, size_t split_ws_bytes, s2vt_stream stream)
{
    if (!split_ws) return S2VT_E_BADARG;
    return bptt_bwd_body(d, p, grads, video, B, N, dlogits, caption_steps, live_rows, n_live, keep, seed, video_id, sample_id, workspace,
                         workspace_bytes, phase, split_grad_mode(N), split_ws, split_ws_bytes, stream);
}

int s2vt_averaged_bptt_bwd(const s2vt_dims* d, const s2vt_params* p, const s2vt_params* grads, const float* video, int32_t B, int32_t N,
                           const float* dlogits, float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id, void* workspace,
                           size_t workspace_bytes, const void* scratch, size_t scratch_bytes, int32_t precision, void* grad_ws, size_t grad_ws_bytes,
                           s2vt_stream stream)
{
    if (!dims_ok(d) || N <= 0 || !scratch || precision < 0 || precision > 2 || (precision != 0) != (grad_ws != nullptr)) return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(scratch) & 255u) return S2VT_E_ALIGN;
    Carver cs(const_cast<void*>(scratch), scratch_bytes);
    AvgScratch x;
    carve_avg(cs, d, N, &x);
    if (!cs.ok()) return S2VT_E_WORKSPACE;
    const int mode = precision == 2 ? split_grad_mode(N) : precision == 1 ? kGradBf16 : kGradFp32;
    return bptt_bwd_body(d, p, grads, video, B, N, dlogits, d->n_caption_lstm_step, nullptr, 0, keep, seed, video_id, sample_id, workspace,
                         workspace_bytes, kAll, mode, grad_ws, grad_ws_bytes, stream, &x);
}

// The backward of the top-k unroll.  Its graph has a second recurrent edge, dZ2[t] -> dx[t] -> dlogits[t - 1] -> dO2[t - 1]: the vocabulary
// data gradient runs once up front on the softmax part of dlogits (the map is linear, the mix's part is added to dO2 step by step), LSTM2's
// recurrence is unrolled in its per-step form with the mix backward between steps, and dWout / the bias gradient run once behind the
// loop on the completed dlogits.  From there on, the stages of BpttBwd with the operand (X, none, Tc N).  One stream, fp32 products.
int s2vt_topk_feed_bptt_bwd(const s2vt_dims* d, const s2vt_params* p, const s2vt_params* grads, const float* video, int32_t B, int32_t N,
                            float* dlogits, float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id, int32_t k,
                            void* workspace, size_t workspace_bytes, const void* scratch, size_t scratch_bytes, s2vt_stream stream)
{
    if (!dims_ok(d) || !params_ok(p) || !params_ok(grads) || !video || !dlogits || !video_id || !sample_id || !workspace || !scratch || B <= 0 ||
        N <= 0 || N % B || !topk_k_ok(d, k))
        return S2VT_E_BADARG;
    if (!(keep > 0.0f)) return S2VT_E_BADARG;                                                  // (a NaN fails the comparison)
    if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(scratch)) & 255u) return S2VT_E_ALIGN;
    if (chain_fault()) return S2VT_E_CHAIN_TIMEOUT;
    const int H = d->lstm_dim, E = d->word_dim, V = d->n_words, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step, T = Tv + Tc;
    Carver c(workspace, workspace_bytes);
    TrainWs w;
    carve_train(c, d, B, N, &w);
    Carver cs(const_cast<void*>(scratch), scratch_bytes);
    TopkScratch ts;
    carve_topk(cs, d, N, k, &ts);
    if (!c.ok() || !cs.ok()) return S2VT_E_WORKSPACE;
    hipStream_t st = S(stream);
    const size_t NH = (size_t)N * H;
    SideStream one_stream;                                   // (ok = false: everything on the caller's stream)
    BpttBwd x{one_stream};
    x.gate1 = x.gate2 = false;
    x.H = H; x.E = E; x.V = V; x.D = d->dim_image; x.Tv = Tv; x.Tc = Tc; x.T = T; x.B = B; x.N = N;
    x.K4 = bf16_pad(4 * H); x.Re = Tv * N; x.Rd = Tc * N; x.NH = NH;
    x.w = w; x.bw = Bf16Ws{}; x.p = p; x.grads = grads; x.video = video; x.dlogits = dlogits; x.live_rows = nullptr; x.n_live = 0;
    x.emb_tab = ts.X; x.emb_idx = nullptr; x.emb_rows = Tc * N; x.emb_ida = x.emb_idb = nullptr;
    x.emb_idk = ts.ids; x.emb_wk = ts.wts; x.emb_k = k;
    x.keep = keep; x.seed = seed; x.video_id = video_id; x.sample_id = sample_id; x.bf16 = x.split = x.fused = false;
    x.st = x.sd = x.sv = st;
    const BwdScratch sc{w.slab, w.dc, w.bimg, w.bex, w.bsync};

    // ---- dO2 = dlogits Wout^T of the softmax part; dWout waits for the completed dlogits
    TnArgs dwout;
    HIP_TRY(x.vocab_fp32(x.Rd, w.dO2, &dwout));
    // ---- LSTM2 back through time, step by step; behind decode step td >= 1: dx[td] = dZ2 W2[H : H + E]^T (the packed-row block of the
    // workspace, unused in a whole pass, holds it), then the mix backward into dlogits[td - 1] and dO2[td - 1], which step td - 1 reads
    const std::function<hipError_t(int)> between = [&](int t) -> hipError_t {
        const int td = t - Tv;
        if (td < 1) return hipSuccess;
        HIP_CHECK(nn_bwd(w.dZ2 + (size_t)t * 4 * NH, 4 * H, p->lstm2_W + (size_t)H * 4 * H, 4 * H, w.dX2p, E, N, E, 4 * H, 1, 0, st));
        const size_t r = (size_t)td * N;
        return launch_topk_mix_bwd(w.dX2p, E, ts.ids + r * k, ts.wts + r * k, ts.sums + r, p->Wemb, E, p->embed_word_W, V, H, k, N,
                                   dlogits + (size_t)(td - 1) * N * V, V, w.dO2 + (size_t)(td - 1) * NH, H, st);
    };
    HIP_TRY(lstm_recurrence_bwd(p->lstm2_W, H + E, w.G2, w.C2, w.dO2, NH, H, Tv, w.dZ2, N, H, T, keep, seed, 512u, video_id, sample_id, sc, 0, st,
                                nullptr, nullptr, false, &between));
    HIP_TRY(launch_gemm_tn(dwout, st));
    HIP_TRY(x.l2_grads_fp32());
    // ---- dX2, LSTM1 back through time on the B per-video rows, its tail (the embedding scatter takes the k weighted ids)
    HIP_TRY(x.dx2_fp32());
    HIP_TRY(launch_reduce_dropout(w.dX2, H + E, w.dH1, T, B, N, H, keep, seed, 256u, video_id, sample_id, st, nullptr, Tv));
    HIP_TRY(lstm_recurrence_bwd(p->lstm1_W, E, w.G1, w.C1, w.dH1, (size_t)B * H, H, 0, w.dZ1, B, H, T, 1.0f, seed, 0u, nullptr, nullptr, sc, -1, st));
    HIP_TRY(x.lstm1_tail_fp32());
    return S2VT_OK;
}

int s2vt_split_grad_active(int32_t N)
{
    return split_grad_mode(N) == kGradSplit && split_fused();
}

int s2vt_softmax_nll_fwd_bwd_split(float* logits, int32_t ld, int32_t R, int32_t V, const int32_t* target, const float* coef, float smoothing,
                                   const float* smoothing_rows, float* nll, float* lp_target, const s2vt_dims* d, int32_t B, int32_t N,
                                   void* split_ws, size_t split_ws_bytes, s2vt_stream stream)
{
    if (!logits || !target || !coef || R < 0 || V <= 0 || ld < V || !dims_ok_res(d) || B <= 0 || N <= 0 || N % B || !split_ws) return S2VT_E_BADARG;
    if (V != d->n_words || (size_t)R > (size_t)d->n_caption_lstm_step * N || !s2vt_split_grad_active(N)) return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(split_ws) & 255u) return S2VT_E_ALIGN;
    Carver cb(split_ws, split_ws_bytes);
    Bf16Ws bw{};
    carve_bf16(cb, d, B, N, &bw, true);
    if (!cb.ok()) return S2VT_E_WORKSPACE;
    const int Kv = bf16_pad(V);
    if (!softmax_nll_split_ok(logits, ld, V, bw.L, bw.L + bw.lo_delta, Kv) || !gemm_bf16x3_tn_ok(bf16_pad(d->lstm_dim + 1), Kv, R)) {
        // not the register kernel's shape (or planes beyond the K-major product's reach): fp32 dlogits in place, for the backward to cast
        HIP_TRY(launch_softmax_nll(logits, ld, R, V, target, coef, smoothing_rows ? 0.0f : smoothing, nll, lp_target, S(stream), smoothing_rows));
        return 1;
    }
    HIP_TRY(launch_softmax_nll_split(logits, ld, R, V, target, coef, smoothing_rows ? 0.0f : smoothing, nll, lp_target, bw.L, bw.L + bw.lo_delta, Kv,
                                     S(stream), smoothing_rows));
    return S2VT_OK;
}

int s2vt_split_grad_dlogits_planes(const s2vt_dims* d, int32_t B, int32_t N, size_t* hi_offset, size_t* lo_offset, int32_t* ld)
{
    if (!dims_ok_res(d) || B <= 0 || N <= 0 || N % B || !hi_offset || !lo_offset || !ld) return S2VT_E_BADARG;
    Carver cb(nullptr, 0);
    Bf16Ws bw{};
    carve_bf16(cb, d, B, N, &bw, true);
    *hi_offset = 0;                                            // (L is the first region of the carve)
    *lo_offset = bw.lo_delta * sizeof(uint16_t);
    *ld = bf16_pad(d->n_words);
    return S2VT_OK;
}

int s2vt_gemm_bf16x3_tn(const uint16_t* Ah, const uint16_t* Al, int32_t lda, const uint16_t* Bh, const uint16_t* Bl, int32_t ldb, float* C,
                        int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t accumulate, float* bias, void* scratch, size_t scratch_bytes,
                        s2vt_stream stream)
{
    if (!Ah || !Al || !Bh || !Bl || !C || M < 0 || N < 0 || K < 0 || lda < M + (bias ? 1 : 0) || ldb < N || ldc < N || (lda & 7) || (ldb & 7))
        return S2VT_E_BADARG;
    if (accumulate < 0 || accumulate > 1 || (scratch_bytes && !scratch) || !gemm_bf16x3_tn_ok(lda, ldb, K)) return S2VT_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(Ah) | reinterpret_cast<uintptr_t>(Al) | reinterpret_cast<uintptr_t>(Bh) | reinterpret_cast<uintptr_t>(Bl)) & 15)
        return S2VT_E_ALIGN;
    HIP_TRY(launch_gemm_bf16x3_tn(Ah, Al, lda, Bh, Bl, ldb, C, ldc, M, N, K, accumulate, bias, static_cast<float*>(scratch), scratch_bytes / 4, 3, S(stream)));
    return S2VT_OK;
}

int s2vt_cast_bf16_split(const float* src, int32_t ld, const int32_t* rowidx, int32_t R, int32_t C, int32_t transpose, uint16_t* dst,
                         uint16_t* dst_lo, int32_t ldd, int32_t Rp, float* colsum, uint16_t* row_dst, uint16_t* row_dst_lo, int32_t row_ldd,
                         void* scratch, size_t scratch_bytes, s2vt_stream stream)
{
    if (!src || !dst || !dst_lo || R < 0 || C <= 0 || ld < C || transpose < 0 || transpose > 1) return S2VT_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(dst_lo)) & 15) return S2VT_E_ALIGN;
    if (!transpose) {
        if (colsum || row_dst || row_dst_lo || ldd < bf16_pad(C) || (ldd & 7)) return S2VT_E_BADARG;
        HIP_TRY(launch_cast_rows_bf16(src, ld, rowidx, R, C, dst, ldd, S(stream), dst_lo));
        return S2VT_OK;
    }
    if (Rp < R || Rp % kBf16K || ldd < Rp || (ldd & 7)) return S2VT_E_BADARG;
    if (!row_dst != !row_dst_lo) return S2VT_E_BADARG;
    if (row_dst && (row_ldd < bf16_pad(C) || (row_ldd & 3))) return S2VT_E_BADARG;
    if (row_dst && ((reinterpret_cast<uintptr_t>(row_dst) | reinterpret_cast<uintptr_t>(row_dst_lo)) & 7)) return S2VT_E_ALIGN;
    if (colsum && (!scratch || scratch_bytes < cast_tr_part_floats(Rp, C) * 4)) return S2VT_E_WORKSPACE;
    CastTrArgs a{src, ld, rowidx, R, C, dst, ldd, Rp, colsum, static_cast<float*>(scratch), row_dst, row_ldd, dst_lo, row_dst_lo};
    HIP_TRY(launch_cast_tr_bf16(a, S(stream)));
    return S2VT_OK;
}

int s2vt_gemm_bf16x3_nt(const uint16_t* Ah, const uint16_t* Al, int32_t lda, const uint16_t* Bh, const uint16_t* Bl, int32_t ldb, float* C,
                        int32_t ldc, int32_t M, int32_t N, int32_t Kp, int32_t accumulate, void* scratch, size_t scratch_bytes, s2vt_stream stream)
{
    if (!Ah || !Al || !Bh || !Bl || !C || M < 0 || N < 0 || Kp < 0 || Kp % kBf16K || lda < Kp || ldb < Kp || ldc < N || (lda & 7) || (ldb & 7))
        return S2VT_E_BADARG;
    if (accumulate < 0 || accumulate > 1 || (scratch_bytes && !scratch)) return S2VT_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(Ah) | reinterpret_cast<uintptr_t>(Al) | reinterpret_cast<uintptr_t>(Bh) | reinterpret_cast<uintptr_t>(Bl)) & 15)
        return S2VT_E_ALIGN;
    HIP_TRY(launch_gemm_bf16x3_nt(Ah, Al, lda, Bh, Bl, ldb, C, ldc, M, N, Kp, accumulate, static_cast<float*>(scratch), scratch_bytes / 4, 3, S(stream)));
    return S2VT_OK;
}

int s2vt_gemm_bf16x3_nt_tile(const uint16_t* Ah, const uint16_t* Al, int32_t lda, const uint16_t* Bh, const uint16_t* Bl, int32_t ldb, float* C,
                             int32_t ldc, int32_t M, int32_t N, int32_t Kp, int32_t accumulate, s2vt_stream stream, int32_t tile)
{
    if (tile < 0 || tile > 1) return S2VT_E_BADARG;
    if (!Ah || !Al || !Bh || !Bl || !C || M < 0 || N < 0 || Kp < 0 || Kp % kBf16K || lda < Kp || ldb < Kp || ldc < N || (lda & 7) || (ldb & 7))
        return S2VT_E_BADARG;
    if (accumulate < 0 || accumulate > 1) return S2VT_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(Ah) | reinterpret_cast<uintptr_t>(Al) | reinterpret_cast<uintptr_t>(Bh) | reinterpret_cast<uintptr_t>(Bl)) & 15)
        return S2VT_E_ALIGN;
    HIP_TRY(launch_gemm_bf16x3_nt(Ah, Al, lda, Bh, Bl, ldb, C, ldc, M, N, Kp, accumulate, nullptr, 0, 3, S(stream), tile));
    return S2VT_OK;
}

int s2vt_gemm_bf16x1_nt(const uint16_t* Ah, int32_t lda, const uint16_t* Bh, int32_t ldb, float* C, int32_t ldc, int32_t M, int32_t N, int32_t Kp,
                        int32_t accumulate, s2vt_stream stream)
{
    if (!Ah || !Bh || !C || M < 0 || N < 0 || Kp < 0 || Kp % kBf16K || lda < Kp || ldb < Kp || ldc < N || (lda & 7) || (ldb & 7)) return S2VT_E_BADARG;
    if (accumulate < 0 || accumulate > 1) return S2VT_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(Ah) | reinterpret_cast<uintptr_t>(Bh)) & 15) return S2VT_E_ALIGN;
    HIP_TRY(launch_gemm_bf16x1_nt(Ah, lda, Bh, ldb, C, ldc, M, N, Kp, accumulate, 3, S(stream)));
    return S2VT_OK;
}

int s2vt_gemm_bf16x3_nt_tile_choice(int32_t M, int32_t N, int32_t cus)
{
    if (M <= 0 || N <= 0 || cus <= 0) return S2VT_E_BADARG;
    return gemm_bf16x3_nt_tile_choice(M, N, cus);
}

int s2vt_gemm_bf16x3_nn(const uint16_t* Ah, const uint16_t* Al, int32_t lda, const uint16_t* Bh, const uint16_t* Bl, int32_t ldb, float* C,
                        int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t accumulate, const float* bias, void* scratch, size_t scratch_bytes,
                        s2vt_stream stream)
{
    if (!Ah || !Al || !Bh || !Bl || !C || M < 0 || N < 0 || K < 0 || lda < bf16_pad(K) || ldb < N || ldc < N || (lda & 7) || (ldb & 7))
        return S2VT_E_BADARG;
    if (accumulate < 0 || accumulate > 1 || (bias && accumulate) || (scratch_bytes && !scratch) || !gemm_bf16x3_tn_ok(ldb, ldb, K)) return S2VT_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(Ah) | reinterpret_cast<uintptr_t>(Al) | reinterpret_cast<uintptr_t>(Bh) | reinterpret_cast<uintptr_t>(Bl)) & 15)
        return S2VT_E_ALIGN;
    HIP_TRY(launch_gemm_bf16x3_nn(Ah, Al, lda, Bh, Bl, ldb, C, ldc, M, N, K, accumulate, bias, static_cast<float*>(scratch), scratch_bytes / 4, 0, S(stream)));
    return S2VT_OK;
}

int s2vt_cast_bf16(const float* src, int32_t ld, const int32_t* rowidx, int32_t R, int32_t C, int32_t transpose, uint16_t* dst, int32_t ldd,
                   int32_t Rp, float* colsum, uint16_t* row_dst, int32_t row_ldd, void* scratch, size_t scratch_bytes, s2vt_stream stream)
{
    if (!src || !dst || R < 0 || C <= 0 || ld < C || transpose < 0 || transpose > 1) return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(dst) & 15) return S2VT_E_ALIGN;
    if (!transpose) {
        if (colsum || row_dst || ldd < bf16_pad(C) || (ldd & 7)) return S2VT_E_BADARG;
        HIP_TRY(launch_cast_rows_bf16(src, ld, rowidx, R, C, dst, ldd, S(stream)));
        return S2VT_OK;
    }
    if (Rp < R || Rp % kBf16K || ldd < Rp || (ldd & 7)) return S2VT_E_BADARG;
    if (row_dst && (row_ldd < bf16_pad(C) || (row_ldd & 3))) return S2VT_E_BADARG;
    if (row_dst && (reinterpret_cast<uintptr_t>(row_dst) & 7)) return S2VT_E_ALIGN;
    if (colsum && (!scratch || scratch_bytes < cast_tr_part_floats(Rp, C) * 4)) return S2VT_E_WORKSPACE;
    CastTrArgs a{src, ld, rowidx, R, C, dst, ldd, Rp, colsum, static_cast<float*>(scratch), row_dst, row_ldd};
    HIP_TRY(launch_cast_tr_bf16(a, S(stream)));
    return S2VT_OK;
}

int s2vt_gemm_bf16_nt(const uint16_t* A, int32_t lda, const uint16_t* Bm, int32_t ldb, float* C, int32_t ldc, int32_t M, int32_t N, int32_t Kp,
                      int32_t accumulate, int32_t mfma, s2vt_stream stream)
{
    if (!A || !Bm || !C || M < 0 || N < 0 || Kp < 0 || Kp % kBf16K || lda < Kp || ldb < Kp || ldc < N || (lda & 7) || (ldb & 7)) return S2VT_E_BADARG;
    if (accumulate < 0 || accumulate > 1 || (mfma != 0 && mfma != 16 && mfma != 32)) return S2VT_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(Bm)) & 15) return S2VT_E_ALIGN;
    HIP_TRY(launch_gemm_bf16_nt(A, lda, Bm, ldb, C, ldc, M, N, Kp, accumulate, mfma, S(stream)));
    return S2VT_OK;
}

int s2vt_bptt_dvideo(const s2vt_dims* d, const s2vt_params* p, int32_t B, int32_t N, float* d_video, void* workspace,
                      size_t workspace_bytes, s2vt_stream stream)
{
    if (!dims_ok_res(d) || !p || !p->encode_image_W || !d_video || !workspace || B <= 0 || N <= 0 || N % B) return S2VT_E_BADARG;
    Carver c(workspace, workspace_bytes);
    TrainWs w;
    carve_train(c, d, B, N, &w);
    if (!c.ok()) return S2VT_E_WORKSPACE;
    hipStream_t st = S(stream);
    const int E = d->word_dim, D = d->dim_image, Tv = d->n_video_lstm_step;
    // d_video[j*Tv + t, :] = dX1[t*B + j, :] @ encode_image_W^T   (dX1 is what s2vt_bptt_bwd left, time-major)
    hipLaunchKernelGGL(enc_index_kernel, dim3((B * Tv + 255) / 256), dim3(256), 0, st, w.decidx, Tv, B);
    HIP_TRY(hipGetLastError());
    GemmArgs a;
    std::memset(&a, 0, sizeof(a));
    a.seg[0] = make_seg(w.dX1, E, E, 0, 0, w.decidx);
    a.nseg = 1;
    a.W = p->encode_image_W; a.ldw = E; a.M = B * Tv; a.N = D; a.C = d_video; a.ldc = D;       // encode_image_W [D][E] is W^T as it lies
    HIP_TRY(launch_gemm(a, EPI_STORE_NT, -1, st));
    return S2VT_OK;
}

int s2vt_embed_scatter_add(const float* dE, int32_t ld, const int32_t* idx, int32_t R, int32_t E, float* dWemb,
                           s2vt_stream stream)
{
    if (!dE || !idx || !dWemb || R < 0 || E <= 0 || ld < E) return S2VT_E_BADARG;
    HIP_TRY(launch_scatter_add_rows(dE, ld, idx, R, E, dWemb, E, S(stream)));
    return S2VT_OK;
}

int s2vt_embed_scatter_add2(const float* dE, int32_t ld, const int32_t* idx_a, const int32_t* idx_b, float scale, int32_t R, int32_t E,
                            float* dWemb, s2vt_stream stream)
{
    if (!dE || !idx_a || !idx_b || !dWemb || R < 0 || E <= 0 || ld < E) return S2VT_E_BADARG;
    HIP_TRY(launch_scatter_add_rows2(dE, ld, idx_a, idx_b, scale, R, E, dWemb, E, S(stream)));
    return S2VT_OK;
}

int s2vt_grad_finalize(float* g, const float* theta, int64_t n, const float* gscale, float weight_decay, float* sumsq,
                       s2vt_stream stream)
{
    if (!g || !sumsq || n < 0 || (weight_decay != 0.0f && !theta)) return S2VT_E_BADARG;
    HIP_TRY(launch_grad_finalize(g, theta, n, gscale, weight_decay, sumsq, S(stream)));
    return S2VT_OK;
}

int s2vt_adam_tf(float* theta, const float* g, float* m, float* v, int64_t n, const float* sumsq, float clip_norm,
                 float lr, int64_t step, float beta1, float beta2, float eps, s2vt_stream stream)
{
    return s2vt_adam_tf_guarded(theta, g, m, v, n, sumsq, clip_norm, lr, step, beta1, beta2, eps, nullptr, stream);
}

int s2vt_adam_tf_guarded(float* theta, const float* g, float* m, float* v, int64_t n, const float* sumsq, float clip_norm,
                         float lr, int64_t step, float beta1, float beta2, float eps, int32_t* applied_step, s2vt_stream stream)
{
    if (!theta || !g || !m || !v || n < 0 || step < 1) return S2VT_E_BADARG;
    if (chain_fault()) return S2VT_E_CHAIN_TIMEOUT;        // (a fault raised after this check is caught by the kernel itself)
    // lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t), epsilon outside the bias correction
    const double lr_t = (double)lr * sqrt(1.0 - pow((double)beta2, (double)step)) / (1.0 - pow((double)beta1, (double)step));
    HIP_TRY(launch_adam_tf(theta, g, m, v, n, sumsq, clip_norm, (float)lr_t, beta1, beta2, eps, S(stream), chain_fault_word(), applied_step,
                           (int32_t)step));
    return S2VT_OK;
}

int s2vt_sgd_guarded(float* theta, const float* g, int64_t n, const float* sumsq, float clip_norm, float lr, int64_t step, int32_t* applied_step,
                     s2vt_stream stream)
{
    if (!theta || !g || n < 0 || step < 1) return S2VT_E_BADARG;
    if (chain_fault()) return S2VT_E_CHAIN_TIMEOUT;        // (a fault raised after this check is caught by the kernel itself)
    HIP_TRY(launch_sgd(theta, g, n, sumsq, clip_norm, lr, S(stream), chain_fault_word(), applied_step, (int32_t)step));
    return S2VT_OK;
}

}  // extern "C"
