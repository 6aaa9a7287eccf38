// bidir.hip -- the two LSTM1 recurrences of the bidirectional captioner (bidirection_tf_s2vt.py:113-121, a
// static_bidirectional_rnn over the frames and the zero padding) advanced by ONE persistent launch.
//
// The two directions are independent chains of the same length on the same rows.  Two persistent grids cannot run side
// by side (profiles/NOTES.md, "Two persistent grids side by side"), and at M <= 64 a step of lstm_chain_kernel<*, 1, 1> is
// half one dependent MFMA chain per wave and half the grid hand-off.  Here workgroup j owns hidden units 4j .. 4j+3 of
// BOTH cells:
//   * both [H x 16] weight slices are resident in LDS (2 x 64 KB at H = 1000, chain.hip's B-fragment order);
//   * a wave carries two accumulators, one per direction, and interleaves their MFMAs k-step by k-step: neither chain's
//     order changes, each instruction's predecessor is now two issue slots away;
//   * each direction has its own ping-pong state image in L2 (A-fragment order, sc1 stores and loads as in chain.hip);
//     the h_t stores of both directions go out behind ONE drain and ONE arrival, and one poll releases both loads.
// Everything else is chain.hip's: the image layout, GridSync (bounded spins, the sticky fault word), the co-residency check,
// the one-persistent-grid-at-a-time ordering (chain_common.h).  Arithmetic contract unchanged: every
// pre-activation is cinit (+) the ascending-k fp32 chain over the recurrent rows and the pointwise part is the EPI_LSTM
// expression sequence, so the states and gates of each direction are bit-identical to s2vt_lstm_recurrence_fwd's
// (tests/test_gpu_bidirection_chain.py).  LSTM1 of this model has no DropoutWrapper (bidirection_tf_s2vt.py:67-72): there is
// no dropped output here.
//
// The carried partial of a direction covers a WINDOW of chain steps [t0, t0 + steps): the forward direction sees the frames
// first (a prefix), the backward direction runs through the padding first and meets the frames last (a suffix, consumed in
// descending time: a negative step stride).  lstm_recurrence() takes a prefix only; the fallback (shapes the one-launch form
// does not serve, per-step launches) cuts a direction at t0 into two calls, the first one's last history slot being the
// second one's slot 0 -- no kernel change and no copy.
#include <hip/hip_runtime.h>

#include "api_util.h"
#include "chain_common.h"

using namespace s2vt_api;

namespace s2vt {

namespace {

struct BiDir {
    const float* W; int kw0; const float* bias;        // full cell matrix [*, 4H]; the recurrent rows start at kw0
    const float* cinit; long long cinit_tstride; int ldcinit; int t0; int steps;   // carried partial of chain step t in [t0, t0 + steps): cinit + (t - t0) * tstride
    float* C; float* Hh; float* gates;                 // histories in chain-step order: step t reads slot t, writes slot t + 1; gates[t] optional
};
struct BiChainArgs {
    BiDir d[2];
    int ldw, M, H, T;
    size_t state_tstride, gates_tstride;
    float* abuf;                                       // 2 directions x 2 parities x 4 row tiles x NG KB, zero-filled by the launcher
    unsigned* sync; unsigned* status; unsigned* fault; unsigned spin_limit;
};

// M <= 64: wave w owns row tile (w + blockIdx) % 4 of both directions (chain.hip's NC = 1, TMW = 1 form, twice).
template <int NG>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void lstm_bichain_kernel(const BiChainArgs g)
{
    constexpr int ZS = 20;                                     // z tile row stride (floats)
    constexpr int IMG = 4 * NG * 256;                          // floats of one state image (4 row tiles)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Wl = smem;                                          // [2 directions][NG][64 lanes][4]: B fragments of this workgroup's 16 gate columns
    const int tid = threadIdx.x, lane = tid & 63;
    const int pwave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* zb = smem + 2 * NG * 256 + pwave * (2 * 16 * ZS);   // one z tile per direction
    const int wave = (pwave + (int)blockIdx.x) & 3;            // (speed only: neighbouring CUs walk different lines of the images)
    const int l15 = lane & 15, lq = lane >> 4;
    const int H = g.H, M = g.M, T = g.T;
    const int u0 = (int)blockIdx.x * 4;
    const int tb = wave;                                       // this wave's row tile
    const bool tok = tb * 16 < M;

    // ---- both slices of recurrent rows -> LDS, once (chain.hip's order: element (k, cc = uu * 4 + gate) goes to group k / 16,
    // lane (k % 4) * 16 + cc, component (k % 16) / 4)
#pragma unroll
    for (int d = 0; d < 2; ++d)
        for (int idx = tid; idx < NG * 16 * 4; idx += 256) {
            const int k = idx >> 2, gt = idx & 3;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (k < H) v = *reinterpret_cast<const f32x4*>(g.d[d].W + (size_t)(g.d[d].kw0 + k) * g.ldw + (size_t)gt * H + u0);
            const int j = k >> 4, e = (k & 15) >> 2, kq = k & 3;
#pragma unroll
            for (int uu = 0; uu < 4; ++uu) Wl[(((d * NG + j) * 64 + kq * 16 + uu * 4 + gt) << 2) + e] = v[uu];
        }

    // ---- the (row, unit) pair this lane finishes at every step, in both directions
    const int rt = lane >> 2, uu = lane & 3;
    const int row = tb * 16 + rt;
    const bool rok = tok && row < M;
    const int u = u0 + uu;
    float bi[2], bj[2], bf[2], bo[2], c_reg[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        bi[d] = g.d[d].bias[u]; bj[d] = g.d[d].bias[H + u]; bf[d] = g.d[d].bias[2 * H + u]; bo[d] = g.d[d].bias[3 * H + u];
        c_reg[d] = rok ? g.d[d].C[(size_t)row * H + u] : 0.0f;      // slot 0 = the initial state
    }
    // where this lane's h value sits in an A-fragment image: k = u -> group u / 16, lane (u % 4) * 16 + rt, component (u % 16) / 4
    const size_t a_own = ((size_t)(tb * NG + (u >> 4)) * 64 + (size_t)((u & 3) * 16 + rt)) * 4 + ((u & 15) >> 2);
    float* const img0 = g.abuf;                                // direction d, parity p: img0 + (2 d + p) * IMG

    GridSync gs{(gu32*)g.sync, g.status, g.fault, g.spin_limit, (int)gridDim.x, false};

    // ---- arrival 0: h_0 of both directions in fragment order (rows >= M and k >= H stay zero)
    if (rok) {
#pragma unroll
        for (int d = 0; d < 2; ++d)
            __hip_atomic_store((gu32*)(img0 + (size_t)(2 * d) * IMG + a_own), __float_as_uint(g.d[d].Hh[(size_t)row * H + u]), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    // the carried partials of a step (accumulator layout: lane (column l15, row group lq) holds rows lq*4 + r of the tile)
    const int ccol = (l15 & 3) * H + u0 + (l15 >> 2);          // W / cinit column of tile column l15
    float ci[2][4];
    auto load_cinit = [&](int t) __attribute__((always_inline)) {
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const BiDir& q = g.d[d];
            const bool has = q.cinit && t >= q.t0 && t < q.t0 + q.steps;       // (uniform)
            const float* base = q.cinit + (long long)(t - q.t0) * q.cinit_tstride;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = tb * 16 + lq * 4 + r;
                ci[d][r] = (has && tok && m < M) ? base[(size_t)m * q.ldcinit + ccol] : 0.0f;
            }
        }
    };
    load_cinit(0);
    gs.arrive(tid);
    const int voff = tok ? lane * 16 : (int)0x80000000u;       // a tile that is not this wave's reads nothing (out of range: zeros)

    for (int t = 0; t < T; ++t) {
        f32x4 acc[2];
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            acc[d] = f32x4{ci[d][0], ci[d][1], ci[d][2], ci[d][3]};
            asm volatile("" : "+v"(acc[d]));                   // the partials are in registers before the rings below are issued
        }
        gs.wait_all((unsigned)t, pwave, lane);
        // ---- A fragments of both directions straight into registers: two rings of RING groups, refilled in place
        const int par = t & 1;
        const __amdgpu_buffer_rsrc_t rsA0 = __builtin_amdgcn_make_buffer_rsrc(img0 + (size_t)(0 + par) * IMG + (size_t)tb * NG * 256, 0, NG * 1024, 0x00020000);
        const __amdgpu_buffer_rsrc_t rsA1 = __builtin_amdgcn_make_buffer_rsrc(img0 + (size_t)(2 + par) * IMG + (size_t)tb * NG * 256, 0, NG * 1024, 0x00020000);
        constexpr int RING = NG < 16 ? NG : 16;                // 2 x 16 KB per wave in flight (chain.hip: one ring of 32)
        f32x4 a[2][RING];
        static_for<0, RING>([&](auto j_) {
            constexpr int j = decltype(j_)::value;
            a[0][j] = bload16_sc1(rsA0, voff, j * 1024);
            a[1][j] = bload16_sc1(rsA1, voff, j * 1024);
        });
        __builtin_amdgcn_sched_barrier(0);
        const f32x4* bl = reinterpret_cast<const f32x4*>(Wl) + lane;
        constexpr int PB = NG < 4 ? NG : 4;                    // B fragments read PB groups ahead
        f32x4 b[PB][2];
        static_for<0, PB>([&](auto j_) {
            constexpr int j = decltype(j_)::value;
            b[j][0] = bl[j * 64]; b[j][1] = bl[(NG + j) * 64];
        });
        static_for<0, NG>([&](auto j_) {
            constexpr int j = decltype(j_)::value;
            const f32x4 b0 = b[j % PB][0], b1 = b[j % PB][1];
            if constexpr (j + PB < NG) { b[j % PB][0] = bl[(j + PB) * 64]; b[j % PB][1] = bl[(NG + j + PB) * 64]; }
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, 4>([&](auto e_) {
                constexpr int e = decltype(e_)::value;
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0][j % RING][e], b0[e], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1][j % RING][e], b1[e], acc[1], 0, 0, 0);
            });
            if constexpr (j + RING < NG) {
                __builtin_amdgcn_sched_barrier(0);             // the refills stay behind the MFMAs that read these registers, and in place
                a[0][j % RING] = bload16_sc1(rsA0, voff, (j + RING) * 1024);
                a[1][j % RING] = bload16_sc1(rsA1, voff, (j + RING) * 1024);
                __builtin_amdgcn_sched_barrier(0);
            }
        });
        // ---- per direction: the gates of a unit meet through the wave's LDS tile z[row][uu*4 + gate]; BasicLSTMCell pointwise
        // (gate order i, j, f, o; forget_bias 1.0 added at run time) -- the EPI_LSTM expressions
        float hv[2], siv[2], tjv[2], sfv[2], sov[2];
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            float* zd = zb + d * (16 * ZS);
#pragma unroll
            for (int r = 0; r < 4; ++r) zd[(lq * 4 + r) * ZS + l15] = acc[d][r];
            __builtin_amdgcn_wave_barrier();
            const f32x4 z = *reinterpret_cast<const f32x4*>(zd + rt * ZS + uu * 4);
            __builtin_amdgcn_wave_barrier();
            const float zi = z[0] + bi[d], zj = z[1] + bj[d], zf = z[2] + bf[d], zo = z[3] + bo[d];
            const float si = dm_sigmoidf(zi);
            const float tj = dm_tanhf(zj);
            const float sf = dm_sigmoidf(zf + 1.0f);
            const float so = dm_sigmoidf(zo);
            const float t1 = c_reg[d] * sf;
            const float t2 = si * tj;
            const float cc = t1 + t2;
            hv[d] = dm_tanhf(cc) * so;
            c_reg[d] = cc;
            siv[d] = si; tjv[d] = tj; sfv[d] = sf; sov[d] = so;
        }
        // The hand-off first: both h_t write-through, drained and signalled ONCE, before the history stores
        if (t + 1 < T) {
            if (rok) {
#pragma unroll
                for (int d = 0; d < 2; ++d)
                    __hip_atomic_store((gu32*)(img0 + (size_t)(2 * d + (par ^ 1)) * IMG + a_own), __float_as_uint(hv[d]), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            }
            gs.arrive(tid);
        }
        if (rok) {
            const size_t o = (size_t)row * H + u;
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                g.d[d].C[(size_t)(t + 1) * g.state_tstride + o] = c_reg[d];
                g.d[d].Hh[(size_t)(t + 1) * g.state_tstride + o] = hv[d];
                if (g.d[d].gates) {
                    float* gp = g.d[d].gates + (size_t)t * g.gates_tstride + (size_t)row * 4 * H + u;
                    gp[0] = siv[d]; gp[H] = tjv[d]; gp[2 * H] = sfv[d]; gp[3 * H] = sov[d];
                }
            }
        }
        if (t + 1 < T) load_cinit(t + 1);
    }
}

typedef void (*BiFn)(const BiChainArgs);
struct BiCfg { int ng; BiFn fn; };
const BiCfg kBi[] = {{8, lstm_bichain_kernel<8>}, {64, lstm_bichain_kernel<64>}};
constexpr int kNumBi = 2;
constexpr int kBiMaxRows = 64;                                 // the 8-unit form's 128 KB slice cannot be doubled
constexpr int kMaxDev = 32;
int bi_lds_bytes(int ng) { return (2 * ng * 256 + 4 * 2 * 16 * 20) * 4; }     // 141,312 bytes at ng = 64
int bi_cfg(int H) { return (H + 15) / 16 <= 8 ? 0 : 1; }
struct BiDev { std::once_flag once; bool ok = false; int per_cu[kNumBi] = {}; };
BiDev g_bidev[kMaxDev];
BiDev* bi_dev_state()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return nullptr;
    BiDev& d = g_bidev[dev];
    std::call_once(d.once, [&d] {
        bool ok = true;
        for (int i = 0; ok && i < kNumBi; ++i) {
            const void* fn = reinterpret_cast<const void*>(kBi[i].fn);
            ok = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bi_lds_bytes(kBi[i].ng)) == hipSuccess;
            int n = 0;
            // co-residency is CHECKED, not assumed
            if (ok && hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, 256, bi_lds_bytes(kBi[i].ng)) == hipSuccess) d.per_cu[i] = n;
        }
        d.ok = ok;
    });
    return &d;
}

// the one-launch form serves this shape on this device
bool bichain_eligible(int M, int H)
{
    if (!(M >= 1 && M <= kBiMaxRows) || !chain_eligible(M, H)) return false;      // (S2VT_CHAIN=0, a hold, chain_ack(disable), H % 4, H <= 1024, H / 4 <= CUs)
    ChainHost hst;
    BiDev* b = bi_dev_state();
    if (!chain_host(&hst) || !b || !b->ok) return false;
    return (long)b->per_cu[bi_cfg(H)] * hst.num_cus >= H / 4;   // every workgroup of the grid fits on the chip at once
}

size_t bichain_scratch_floats(int H)
{
    const size_t two = (size_t)2 * 2 * 4 * ((H + 15) / 16 <= 8 ? 8 : 64) * 256;          // 2 directions x 2 parities x 4 row tiles
    const size_t one = chain_scratch_floats(H);                                           // (the fallback's recurrences, one after the other)
    return two > one ? two : one;
}

hipError_t launch_lstm_bichain(const BiChainArgs& a, hipStream_t st)
{
    if (!bichain_eligible(a.M, a.H)) return hipErrorInvalidValue;
    if (a.T <= 0) return hipSuccess;
    ChainHost hst;
    if (!chain_host(&hst)) return hipErrorInvalidValue;
    const BiCfg& c = kBi[bi_cfg(a.H)];
    BiChainArgs k = a;
    k.status = hst.status_dev; k.fault = hst.fault; k.spin_limit = hst.spin_limit;
    ChainLaunchOrder order;                                    // one persistent grid at a time per process
    hipError_t e = order.before(st, hst.device);
    if (e != hipSuccess) return e;
    // every polled word and the fragment images start from zero on EVERY call
    ZeroList z;
    z.add(a.sync, kChainSyncBytes); z.add(a.abuf, (size_t)2 * 2 * 4 * c.ng * 256 * 4);
    e = launch_zero_regions(z, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(c.fn, dim3((unsigned)(a.H / 4)), dim3(256), bi_lds_bytes(c.ng), st, k);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return order.after(st, hst.device);
}

bool dir_ok(const s2vt_lstm_dir* d, int H)
{
    if (!d || !d->W || !d->b || !d->C_hist || !d->H_hist || d->kw0 < 0) return false;
    if (d->cinit && (d->cinit_t0 < 0 || d->cinit_steps < 0 || d->ldcinit < 4 * H)) return false;
    if (d->cinit && d->gates == d->cinit) return false;       // (the plain recurrence lets the gates overwrite the partial; here the window moves)
    return true;
}

// one direction through lstm_recurrence(), which takes its carried partial as a prefix: cut at the window's first step.
// (lstm_recurrence's step stride is signed: the backward direction walks its frame products last frame first.)
hipError_t dir_recurrence(const s2vt_lstm_dir* d, int M, int H, int T, float* abuf, unsigned* sync, hipStream_t st)
{
    const size_t MH = (size_t)M * H;
    const NoiseIds none{nullptr, nullptr, 0};
    int t0 = 0, steps = 0;
    if (d->cinit && d->cinit_steps > 0 && d->cinit_t0 < T) { t0 = d->cinit_t0; steps = d->cinit_steps < T - t0 ? d->cinit_steps : T - t0; }
    if (t0 > 0) {
        hipError_t e = lstm_recurrence(d->W, d->kw0, d->b, nullptr, 0, 0, 0, d->C_hist, d->H_hist, MH, d->gates, 4 * MH, nullptr, 0, M, H, t0, 1.0f,
                                       none, 0, abuf, sync, st);
        if (e != hipSuccess) return e;
    }
    return lstm_recurrence(d->W, d->kw0, d->b, steps ? d->cinit : nullptr, (long long)d->cinit_tstride, d->ldcinit, steps, d->C_hist + (size_t)t0 * MH,
                           d->H_hist + (size_t)t0 * MH, MH, d->gates ? d->gates + (size_t)t0 * 4 * MH : nullptr, 4 * MH, nullptr, 0, M, H, T - t0, 1.0f,
                           none, 0, abuf, sync, st);
}

}  // namespace

}  // namespace s2vt

extern "C" {

size_t s2vt_lstm_birecurrence_scratch_bytes(int32_t H)
{
    if (H <= 0) return 0;
    return ((bichain_scratch_floats(H) * 4 + 255) & ~size_t(255)) + ((kChainSyncBytes + 255) & ~size_t(255));
}

int s2vt_lstm_birecurrence_fwd(const s2vt_lstm_dir* fw, const s2vt_lstm_dir* bw, int32_t M, int32_t H, int32_t T, int32_t persistent,
                               void* scratch, size_t scratch_bytes, s2vt_stream stream)
{
    if (M <= 0 || H <= 0 || T < 0 || persistent < -1 || persistent > 2 || !dir_ok(fw, H) || !dir_ok(bw, H)) return S2VT_E_BADARG;
    if (chain_fault()) return S2VT_E_CHAIN_TIMEOUT;
    float* abuf = nullptr;
    unsigned* sync = nullptr;
    bool one = false;
    if (persistent != 0) {
        const bool fits = bichain_eligible(M, H);
        const bool aligned = chain_operands_ok(fw->W, 4 * H, fw->W) && chain_operands_ok(bw->W, 4 * H, bw->W);
        if (persistent == 1 && !fits) return S2VT_E_BADARG;
        if (persistent == 1 && !aligned) return S2VT_E_ALIGN;
        if (persistent == 2 && !chain_eligible(M, H)) return S2VT_E_BADARG;
        if (persistent == 2 && !aligned) return S2VT_E_ALIGN;
        one = persistent != 2 && fits && aligned;
        if (one || chain_eligible(M, H)) {                     // (-1 where neither fits: per-step launches, no scratch)
            if (!scratch) return S2VT_E_BADARG;
            if (reinterpret_cast<uintptr_t>(scratch) & 255u) return S2VT_E_ALIGN;
            Carver c(scratch, scratch_bytes);
            sync = c.take<unsigned>(kChainSyncBytes / 4);
            abuf = c.take<float>(bichain_scratch_floats(H));
            if (!c.ok()) return S2VT_E_WORKSPACE;
        }
    }
    if (one) {
        BiChainArgs a;
        std::memset(&a, 0, sizeof(a));
        const s2vt_lstm_dir* dirs[2] = {fw, bw};
        for (int i = 0; i < 2; ++i) {
            const s2vt_lstm_dir* d = dirs[i];
            BiDir& q = a.d[i];
            q.W = d->W; q.kw0 = d->kw0; q.bias = d->b;
            q.cinit = d->cinit; q.cinit_tstride = d->cinit_tstride; q.ldcinit = d->ldcinit; q.t0 = d->cinit_t0; q.steps = d->cinit ? d->cinit_steps : 0;
            q.C = d->C_hist; q.Hh = d->H_hist; q.gates = d->gates;
        }
        a.ldw = 4 * H; a.M = M; a.H = H; a.T = T;
        a.state_tstride = (size_t)M * H; a.gates_tstride = (size_t)4 * M * H;
        a.abuf = abuf; a.sync = sync;
        HIP_TRY(launch_lstm_bichain(a, S(stream)));
        return S2VT_OK;
    }
    HIP_TRY(dir_recurrence(fw, M, H, T, abuf, sync, S(stream)));
    HIP_TRY(dir_recurrence(bw, M, H, T, abuf, sync, S(stream)));
    return S2VT_OK;
}


// ---------------------------------------------------------------------------------------------------------------------
// The bidirectional captioner's drivers (bidirection_tf_s2vt.py:85-216): the model composed from the library's own entry
// points on one caller-owned workspace, as the attention captioner's are.  Rows are time-major (row t * B + b) except the frame
// embedding (row b * Tv + t, the reference's reshape); the backward direction's history is in chain-step order and every
// consumer reads it through the index map rev[t * B + b] = (T-1-t) * B + b, which is its own inverse.
}  // extern "C"

namespace {

__global__ void bidir_index_kernel(int B, int Tv, int Tc, int V, const int32_t* caption, int32_t* tm, int32_t* rev, int32_t* fed, int32_t* srcf,
                                   int32_t* srcb, int32_t* framesb)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, T = Tv + Tc;
    if (i < Tv * B) {
        const int t = i / B, b = i % B;
        tm[i] = b * Tv + t;                                    // embedding row of time-major row t * B + b
        framesb[i] = b * Tv + (Tv - 1 - t);                    // ... of the backward direction's chain row (Tc + t) * B + b
        const int bb = i / Tv, tt = i % Tv;
        srcf[i] = tt * B + bb;                                 // time-major row behind embedding row b * Tv + t
        srcb[i] = (Tv - 1 - tt) * B + bb;
    }
    if (i < T * B) rev[i] = (T - 1 - i / B) * B + i % B;
    if (fed && i < Tc * B) {
        const int t = i / B, b = i % B;
        int w = t == 0 ? 1 : caption[(size_t)b * Tc + t - 1];  // <bos>, then the previous word (:131-136)
        fed[i] = w < 0 ? 0 : (w >= V ? V - 1 : w);
    }
}
__global__ void bidir_ids_kernel(int B, int Tc, int t, int32_t video_base, const int32_t* tok, int32_t* ids, int32_t* vid, int32_t* sid)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (t < 0) { vid[b] = video_base + b; sid[b] = -1; ids[b] = 1; return; }      // (set-up: the greedy block's noise ids; ids = the fed word, <bos>)
    ids[(size_t)b * Tc + t] = tok[b];
}

struct BiWs {
    int32_t *tm, *rev, *fed, *srcf, *srcb, *framesb;
    float *emb, *xp[2], *C1[2], *H1[2], *G1[2], *P2, *G2, *C2, *H2, *O2;
    float *dO2, *dZ2, *dd[2], *dE, *dZ1, *demb[2];
    void *chain, *bchain;
    size_t chain_bytes, bchain_bytes;
};
bool bidir_dims_ok(const s2vt_dims* d, int B)
{
    return d && B > 0 && d->reserved == 0 && d->dim_image > 0 && d->n_words > 1 && d->word_dim > 0 && d->lstm_dim > 0 && d->n_video_lstm_step > 0 &&
           d->n_caption_lstm_step > 0 && d->n_caption_lstm_step <= 128;
}
size_t bidir_carve(const s2vt_dims* d, int B, void* base, size_t cap, BiWs* w, bool train)
{
    const size_t H = d->lstm_dim, E = d->word_dim, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step, T = Tv + Tc, BH = (size_t)B * H;
    Carver c(base, cap);
    BiWs t;
    std::memset(&t, 0, sizeof(t));
    t.tm = c.take<int32_t>(Tv * B); t.rev = c.take<int32_t>(T * B); t.fed = c.take<int32_t>(Tc * B);
    t.srcf = c.take<int32_t>(Tv * B); t.srcb = c.take<int32_t>(Tv * B); t.framesb = c.take<int32_t>(Tv * B);
    t.emb = c.take<float>(Tv * B * E);
    for (int k = 0; k < 2; ++k) {
        t.xp[k] = c.take<float>(Tv * B * 4 * H); t.C1[k] = c.take<float>((T + 1) * BH); t.H1[k] = c.take<float>((T + 1) * BH);
        t.G1[k] = train ? c.take<float>(T * 4 * BH) : nullptr;
    }
    t.P2 = c.take<float>(T * 4 * BH);
    t.C2 = c.take<float>((T + 1) * BH); t.H2 = c.take<float>((T + 1) * BH); t.O2 = c.take<float>(T * BH);
    t.chain_bytes = s2vt_lstm_birecurrence_scratch_bytes((int32_t)H);
    t.chain = c.take<char>(t.chain_bytes);
    if (train) {
        t.G2 = c.take<float>(T * 4 * BH);
        t.dO2 = c.take<float>(Tc * BH); t.dZ2 = c.take<float>(T * 4 * BH); t.dd[0] = c.take<float>(T * BH); t.dd[1] = c.take<float>(T * BH);
        t.dE = c.take<float>(Tc * B * E); t.dZ1 = c.take<float>(T * 4 * BH); t.demb[0] = c.take<float>(Tv * B * E); t.demb[1] = c.take<float>(Tv * B * E);
        t.bchain_bytes = s2vt_lstm_recurrence_bwd_scratch_bytes(B, (int32_t)H);
        t.bchain = c.take<char>(t.bchain_bytes);
    }
    if (w) *w = t;
    return c.off;
}
#define RC_TRY(expr) do { const int rc_ = (expr); if (rc_ != S2VT_OK) return rc_; } while (0)

// frame embedding, both LSTM1 recurrences (histories left in w.C1 / w.H1 / w.G1)
int bidir_lstm1(const s2vt_dims* d, const s2vt_bidir_params* p, const float* video, int B, const int32_t* caption, const BiWs& w, int form, s2vt_stream stream)
{
    const int H = d->lstm_dim, E = d->word_dim, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step, T = Tv + Tc, D = d->dim_image;
    const size_t BH = (size_t)B * H;
    const int n = (T * B > Tc * B ? T * B : Tc * B);
    hipLaunchKernelGGL(bidir_index_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), B, Tv, Tc, d->n_words, caption, w.tm, w.rev,
                       caption ? w.fed : nullptr, w.srcf, w.srcb, w.framesb);
    HIP_TRY(hipGetLastError());
    s2vt_operand o{video, nullptr, D, D, 0, 0};
    RC_TRY(s2vt_gemm(&o, 1, p->encode_image_W, E, p->encode_image_b, nullptr, 0, w.emb, E, B * Tv, E, 0, -1, stream));
    const float* W1[2] = {p->lstm1_fw_W, p->lstm1_bw_W};
    const float* b1[2] = {p->lstm1_fw_b, p->lstm1_bw_b};
    s2vt_lstm_dir dir[2];
    for (int k = 0; k < 2; ++k) {
        s2vt_operand e{w.emb, w.tm, E, E, 0, 0};
        RC_TRY(s2vt_gemm(&e, 1, W1[k], 4 * H, nullptr, nullptr, 0, w.xp[k], 4 * H, Tv * B, 4 * H, 0, -1, stream));
        HIP_TRY(hipMemsetAsync(w.C1[k], 0, BH * 4, S(stream)));                // zero initial states
        HIP_TRY(hipMemsetAsync(w.H1[k], 0, BH * 4, S(stream)));
        std::memset(&dir[k], 0, sizeof(dir[k]));
        dir[k].W = W1[k]; dir[k].kw0 = E; dir[k].b = b1[k];
        dir[k].cinit = k ? w.xp[k] + (size_t)(Tv - 1) * B * 4 * H : w.xp[k];    // the backward cell meets the frames last, last frame first
        dir[k].cinit_tstride = k ? -(int64_t)B * 4 * H : (int64_t)B * 4 * H;
        dir[k].ldcinit = 4 * H; dir[k].cinit_t0 = k ? Tc : 0; dir[k].cinit_steps = Tv;
        dir[k].C_hist = w.C1[k]; dir[k].H_hist = w.H1[k]; dir[k].gates = w.G1[k];
    }
    return s2vt_lstm_birecurrence_fwd(&dir[0], &dir[1], B, H, T, form, w.chain, w.chain_bytes, stream);
}

bool bidir_params_ok(const s2vt_bidir_params* p)
{
    return p && p->Wemb && p->encode_image_W && p->encode_image_b && p->lstm1_fw_W && p->lstm1_fw_b && p->lstm1_bw_W && p->lstm1_bw_b && p->lstm2_W &&
           p->lstm2_b && p->embed_word_W && p->embed_word_b;
}

}  // namespace

extern "C" {

size_t s2vt_bidir_workspace_bytes(const s2vt_dims* d, int32_t B)
{
    return bidir_dims_ok(d, B) ? bidir_carve(d, B, nullptr, 0, nullptr, true) : 0;
}

size_t s2vt_bidir_decode_workspace_bytes(const s2vt_dims* d, int32_t B)
{
    if (!bidir_dims_ok(d, B)) return 0;
    Carver c(nullptr, 0);
    c.off = bidir_carve(d, B, nullptr, 0, nullptr, false);
    const size_t BH = (size_t)B * d->lstm_dim;
    c.take<float>(4 * BH); c.take<float>(BH); c.take<float>((size_t)B * d->n_words); c.take<unsigned long long>(B); c.take<int32_t>(3 * (size_t)B);
    return c.off;
}

int s2vt_bidir_teacher_forced_fwd(const s2vt_dims* d, const s2vt_bidir_params* p, const float* video, int32_t B, const int32_t* caption, float keep,
                                  uint64_t seed, const int32_t* video_id, const int32_t* sample_id, int32_t lstm1_form, float* logits_out, void* workspace,
                                  size_t workspace_bytes, s2vt_stream stream)
{
    if (!bidir_dims_ok(d, B) || !bidir_params_ok(p) || !video || !caption || !logits_out || !workspace || !(keep > 0.0f) || keep > 1.0f ||
        (keep < 1.0f && (!video_id || !sample_id)) || lstm1_form < -1 || lstm1_form > 2)
        return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    BiWs w;
    if (bidir_carve(d, B, workspace, workspace_bytes, &w, true) > workspace_bytes) return S2VT_E_WORKSPACE;
    const int H = d->lstm_dim, E = d->word_dim, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step, T = Tv + Tc, V = d->n_words;
    const size_t BH = (size_t)B * H;
    RC_TRY(bidir_lstm1(d, p, video, B, caption, w, lstm1_form, stream));
    // [fw ; bw (; embed)] @ W2[:2H (+ E)] hoisted for all T steps; the encode steps feed no word (zero rows contribute nothing)
    s2vt_operand enc[2] = {{w.H1[0] + BH, nullptr, H, H, 0, 0}, {w.H1[1] + BH, w.rev, H, H, 0, 0}};
    RC_TRY(s2vt_gemm(enc, 2, p->lstm2_W, 4 * H, nullptr, nullptr, 0, w.P2, 4 * H, Tv * B, 4 * H, 0, -1, stream));
    s2vt_operand dec[3] = {{w.H1[0] + BH + (size_t)Tv * BH, nullptr, H, H, 0, 0}, {w.H1[1] + BH, w.rev + (size_t)Tv * B, H, H, 0, 0}, {p->Wemb, w.fed, E, E, 0, 0}};
    RC_TRY(s2vt_gemm(dec, 3, p->lstm2_W, 4 * H, nullptr, nullptr, 0, w.P2 + (size_t)Tv * B * 4 * H, 4 * H, Tc * B, 4 * H, 0, -1, stream));
    HIP_TRY(hipMemsetAsync(w.C2, 0, BH * 4, S(stream)));
    HIP_TRY(hipMemsetAsync(w.H2, 0, BH * 4, S(stream)));
    // LSTM2 over all T steps; the only dropout of build_model is its wrapper, on its own Philox codes (layer 2: 512 + step)
    RC_TRY(s2vt_lstm_recurrence_fwd(p->lstm2_W, 2 * H + E, p->lstm2_b, w.P2, (int64_t)B * 4 * H, 4 * H, T, w.C2, w.H2, w.G2, w.O2, B, H, T, keep, seed,
                                    video_id, sample_id, 512u, -1, w.chain, w.chain_bytes, stream));
    s2vt_operand o{w.O2 + (size_t)Tv * BH, nullptr, H, H, 0, 0};
    return s2vt_gemm(&o, 1, p->embed_word_W, V, p->embed_word_b, nullptr, 0, logits_out, V, Tc * B, V, 0, -1, stream);
}

int s2vt_bidir_bptt_bwd(const s2vt_dims* d, const s2vt_bidir_params* p, const s2vt_bidir_params* grads, const float* video, int32_t B,
                        const float* dlogits, float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id, void* workspace,
                        size_t workspace_bytes, s2vt_stream stream)
{
    if (!bidir_dims_ok(d, B) || !bidir_params_ok(p) || !bidir_params_ok(grads) || !video || !dlogits || !workspace || !(keep > 0.0f) || keep > 1.0f ||
        (keep < 1.0f && (!video_id || !sample_id)))
        return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    BiWs w;
    if (bidir_carve(d, B, workspace, workspace_bytes, &w, true) > workspace_bytes) return S2VT_E_WORKSPACE;
    const int H = d->lstm_dim, E = d->word_dim, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step, T = Tv + Tc, V = d->n_words, D = d->dim_image;
    const size_t BH = (size_t)B * H;
    const s2vt_bidir_params* g = grads;
    // vocabulary projection
    RC_TRY(s2vt_gemm_tn(w.O2 + (size_t)Tv * BH, H, nullptr, dlogits, V, g->embed_word_W, V, Tc * B, H, V, 1, stream));
    RC_TRY(s2vt_colsum(dlogits, V, Tc * B, V, g->embed_word_b, stream));
    s2vt_operand dl{dlogits, nullptr, V, V, 0, 0};
    RC_TRY(s2vt_gemm_nt(&dl, 1, p->embed_word_W, V, nullptr, nullptr, 0, w.dO2, H, Tc * B, H, 0, -1, stream));
    // LSTM2 over all T steps; its outputs feed the logits from step Tv on
    RC_TRY(s2vt_lstm_recurrence_bwd(p->lstm2_W, 2 * H + E, w.G2, w.C2, w.dO2, (int64_t)BH, H, Tv, w.dZ2, B, H, T, keep, seed, video_id, sample_id, 512u, -1,
                                    w.bchain, w.bchain_bytes, stream));
    float* gW2 = g->lstm2_W;
    const float* dZ2d = w.dZ2 + (size_t)Tv * B * 4 * H;
    RC_TRY(s2vt_gemm_tn(w.H1[0] + BH, H, nullptr, w.dZ2, 4 * H, gW2, 4 * H, T * B, H, 4 * H, 1, stream));
    RC_TRY(s2vt_gemm_tn(w.H1[1] + BH, H, w.rev, w.dZ2, 4 * H, gW2 + (size_t)H * 4 * H, 4 * H, T * B, H, 4 * H, 1, stream));
    RC_TRY(s2vt_gemm_tn(p->Wemb, E, w.fed, dZ2d, 4 * H, gW2 + (size_t)2 * H * 4 * H, 4 * H, Tc * B, E, 4 * H, 1, stream));
    RC_TRY(s2vt_gemm_tn(w.H2, H, nullptr, w.dZ2, 4 * H, gW2 + (size_t)(2 * H + E) * 4 * H, 4 * H, T * B, H, 4 * H, 1, stream));
    RC_TRY(s2vt_colsum(w.dZ2, 4 * H, T * B, 4 * H, g->lstm2_b, stream));
    // into LSTM2's inputs: d fw in time order, d bw already in chain-step order (rev is its own inverse), d embed -> Wemb's rows
    s2vt_operand z{w.dZ2, nullptr, 4 * H, 4 * H, 0, 0}, zr{w.dZ2, w.rev, 4 * H, 4 * H, 0, 0}, zd{dZ2d, nullptr, 4 * H, 4 * H, 0, 0};
    RC_TRY(s2vt_gemm_nt(&z, 1, p->lstm2_W, 4 * H, nullptr, nullptr, 0, w.dd[0], H, T * B, H, 0, -1, stream));
    RC_TRY(s2vt_gemm_nt(&zr, 1, p->lstm2_W + (size_t)H * 4 * H, 4 * H, nullptr, nullptr, 0, w.dd[1], H, T * B, H, 0, -1, stream));
    RC_TRY(s2vt_gemm_nt(&zd, 1, p->lstm2_W + (size_t)2 * H * 4 * H, 4 * H, nullptr, nullptr, 0, w.dE, E, Tc * B, E, 0, -1, stream));
    RC_TRY(s2vt_embed_scatter_add(w.dE, E, w.fed, Tc * B, E, g->Wemb, stream));
    // LSTM1: one backward recurrence per direction, every step carries a gradient from LSTM2
    const float* W1[2] = {p->lstm1_fw_W, p->lstm1_bw_W};
    float* gW1[2] = {g->lstm1_fw_W, g->lstm1_bw_W};
    float* gb1[2] = {g->lstm1_fw_b, g->lstm1_bw_b};
    for (int k = 0; k < 2; ++k) {
        RC_TRY(s2vt_lstm_recurrence_bwd(W1[k], E, w.G1[k], w.C1[k], w.dd[k], (int64_t)BH, H, 0, w.dZ1, B, H, T, 1.0f, 0, nullptr, nullptr, 0u, -1, w.bchain,
                                        w.bchain_bytes, stream));
        const float* dZf = w.dZ1 + (size_t)(k ? Tc : 0) * B * 4 * H;            // the steps that saw a frame
        RC_TRY(s2vt_gemm_tn(w.emb, E, k ? w.framesb : w.tm, dZf, 4 * H, gW1[k], 4 * H, Tv * B, E, 4 * H, 1, stream));
        RC_TRY(s2vt_gemm_tn(w.H1[k], H, nullptr, w.dZ1, 4 * H, gW1[k] + (size_t)E * 4 * H, 4 * H, T * B, H, 4 * H, 1, stream));
        RC_TRY(s2vt_colsum(w.dZ1, 4 * H, T * B, 4 * H, gb1[k], stream));
        s2vt_operand f{dZf, k ? w.srcb : w.srcf, 4 * H, 4 * H, 0, 0};
        RC_TRY(s2vt_gemm_nt(&f, 1, W1[k], 4 * H, nullptr, k ? w.demb[0] : nullptr, k ? E : 0, w.demb[k], E, B * Tv, E, 0, -1, stream));
    }
    RC_TRY(s2vt_gemm_tn(video, D, nullptr, w.demb[1], E, g->encode_image_W, E, B * Tv, D, E, 1, stream));
    return s2vt_colsum(w.demb[1], E, B * Tv, E, g->encode_image_b, stream);
}

int s2vt_bidir_decode_greedy(const s2vt_dims* d, const s2vt_bidir_params* p, const float* video, int32_t B, int32_t unshifted_softmax, int32_t video_base,
                             int32_t lstm1_form, int32_t* ids_out, float* logits_out, void* workspace, size_t workspace_bytes, s2vt_stream stream)
{
    if (!bidir_dims_ok(d, B) || !bidir_params_ok(p) || !video || !ids_out || !workspace || lstm1_form < -1 || lstm1_form > 2) return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    BiWs w;
    const int H = d->lstm_dim, E = d->word_dim, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step, T = Tv + Tc, V = d->n_words;
    const size_t BH = (size_t)B * H;
    Carver c(workspace, workspace_bytes);
    c.off = bidir_carve(d, B, workspace, workspace_bytes, &w, false);
    float* st = c.take<float>(4 * BH);                         // c | h, two parities
    float* out2 = c.take<float>(BH);
    float* logits = c.take<float>((size_t)B * V);
    unsigned long long* packed = c.take<unsigned long long>(B);
    int32_t* iw = c.take<int32_t>(3 * (size_t)B);
    if (!c.ok()) return S2VT_E_WORKSPACE;
    int32_t *tok = iw, *vid = iw + B, *sid = iw + 2 * B;
    hipStream_t hs = S(stream);
    const unsigned nb = (unsigned)((B + 255) / 256);
    hipLaunchKernelGGL(bidir_ids_kernel, dim3(nb), dim3(256), 0, hs, B, Tc, -1, video_base, nullptr, tok, vid, sid);
    HIP_TRY(hipGetLastError());
    // LSTM1 and [fw ; bw] @ W2[:2H] once per video, LSTM2's Tv encode steps as a recurrence
    RC_TRY(bidir_lstm1(d, p, video, B, nullptr, w, lstm1_form, stream));
    s2vt_operand o1[2] = {{w.H1[0] + BH, nullptr, H, H, 0, 0}, {w.H1[1] + BH, w.rev, H, H, 0, 0}};
    RC_TRY(s2vt_gemm(o1, 2, p->lstm2_W, 4 * H, nullptr, nullptr, 0, w.P2, 4 * H, T * B, 4 * H, 0, -1, stream));
    HIP_TRY(hipMemsetAsync(w.C2, 0, BH * 4, hs));
    HIP_TRY(hipMemsetAsync(w.H2, 0, BH * 4, hs));
    RC_TRY(s2vt_lstm_recurrence_fwd(p->lstm2_W, 2 * H + E, p->lstm2_b, w.P2, (int64_t)B * 4 * H, 4 * H, Tv, w.C2, w.H2, nullptr, nullptr, B, H, Tv, 1.0f, 0,
                                    nullptr, nullptr, 0u, -1, w.chain, w.chain_bytes, stream));
    const float* cprev = w.C2 + (size_t)Tv * BH;
    const float* hprev = w.H2 + (size_t)Tv * BH;
    const NoiseIds none{nullptr, nullptr, 0};
    for (int t = 0; t < Tc; ++t) {
        // the fused cell launch: the chain goes on from its slice of the hoisted partial with the fed word's rows of Wemb (gathered as an
        // operand) and the state's rows; then the pick launch
        float* cn = st + (size_t)(t & 1) * 2 * BH;
        float* hn = cn + BH;
        ASeg segs[2] = {make_seg(p->Wemb, E, E, 2 * H, 0, tok), make_seg(hprev, H, H, 2 * H + E)};
        HIP_TRY(lstm_call(segs, 2, p->lstm2_W, p->lstm2_b, cprev, 0, cn, hn, out2, nullptr, B, H, 1.0f, none, 0u, -1, hs, w.P2 + (size_t)(Tv + t) * B * 4 * H,
                          4 * H));
        if (unshifted_softmax || logits_out) {
            s2vt_operand o{out2, nullptr, H, H, 0, 0};
            RC_TRY(s2vt_gemm(&o, 1, p->embed_word_W, V, p->embed_word_b, nullptr, 0, logits, V, B, V, 0, -1, stream));
            if (logits_out)
                HIP_TRY(hipMemcpy2DAsync(logits_out + (size_t)t * V, (size_t)Tc * V * 4, logits, (size_t)V * 4, (size_t)V * 4, B, hipMemcpyDeviceToDevice, hs));
        }
        if (unshifted_softmax) RC_TRY(s2vt_softmax_unshifted_argmax(logits, V, B, V, tok, nullptr, stream));
        else {
            HIP_TRY(hipMemsetAsync(packed, 0, (size_t)B * 8, hs));                  // the pick is an atomicMax on a zeroed word per row
            RC_TRY(s2vt_vocab_pick(out2, H, p->embed_word_W, p->embed_word_b, B, H, V, vid, sid, t, 0, packed, tok, nullptr, -1, stream));
        }
        hipLaunchKernelGGL(bidir_ids_kernel, dim3(nb), dim3(256), 0, hs, B, Tc, t, 0, tok, ids_out, vid, sid);
        HIP_TRY(hipGetLastError());
        cprev = cn; hprev = hn;
    }
    return S2VT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// The self-critical REINFORCE stage (reinforcement_multisampling_tf_s2vt.py:227-339 on this model).  No word ever enters LSTM1, so
// both LSTM1 directions, their histories and [fw ; bw] @ W2[:2H] depend on the video only: the S sample rows of a video share them,
// forward and backward.  Rows are sample-major (row s * B + j is sample s of video j, the video of row n is n % B) and the feature
// block is never tiled.  What sees a per-sample operand (the fed word, LSTM2's state, its dropout noise, the logits) runs on
// N = S * B rows; what only sees the video runs on B rows, and its gradient is the sum over the video's S rows (the sample sum).
namespace {

// sampler set-up (t < 0): noise ids and <bos> of the R = (K + greedy) * B decode rows, the greedy block last with sample id -1
// (s2vt_sample's convention); step t: the picks into sampled [K * B, Tc] / greedy [B, Tc]
__global__ void bidir_sample_ids_kernel(int B, int K, int R, int Tc, int t, int32_t video_base, int32_t* tok, int32_t* sampled, int32_t* greedy,
                                        int32_t* vid, int32_t* sid)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int s = r / B;
    if (t < 0) { vid[r] = video_base + r % B; sid[r] = s < K ? s : -1; tok[r] = 1; return; }
    if (s < K) sampled[(size_t)r * Tc + t] = tok[r];
    else greedy[(size_t)(r - K * B) * Tc + t] = tok[r];
}
// fed[t * N + n] = the word row n is fed at decode step t: <bos>, then the previous word (clamped as bidir_index_kernel does)
__global__ void bidir_rows_fed_kernel(int N, int Tc, int V, const int32_t* caption, int32_t* fed)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)Tc * N) return;
    const int t = (int)(i / N), n = (int)(i % N);
    const int w = t == 0 ? 1 : caption[(size_t)n * Tc + t - 1];
    fed[i] = w < 0 ? 0 : (w >= V ? V - 1 : w);
}
// out[t][n][:] = in[t][n % B][:] for t < T: the encode steps' partial of the N rows (no word is fed there: the shared chain is the whole one)
__global__ __launch_bounds__(256) void bidir_tile_rows_kernel(const f32x4* __restrict__ in, f32x4* __restrict__ out, int T, int B, int N, int C4)
{
    const size_t total = (size_t)T * N * C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t row = i / C4;
        const int c = (int)(i % C4), t = (int)(row / N), n = (int)(row % N);
        out[i] = in[((size_t)t * B + n % B) * C4 + c];
    }
}
// The sample sum: out[t * B + b][:] = sum_s in[t * N + s * B + b][:], ascending s, one owning thread per output element, no atomics (two
// runs give equal bits).  HBM-bound: 16-byte loads, consecutive lanes on consecutive 16 bytes of a row, four samples in flight.
__global__ __launch_bounds__(256) void bidir_sample_sum_kernel(const f32x4* __restrict__ in, f32x4* __restrict__ out, int TB, int B, int S, int C4)
{
    const size_t total = (size_t)TB * C4, BC = (size_t)B * C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t row = i / C4;
        const int c = (int)(i % C4);
        const f32x4* src = in + ((row / B) * S * B + row % B) * C4 + c;      // row t * N + b; sample s lies s * B rows on
        f32x4 acc = src[0];
        int s = 1;
        for (; s + 4 <= S; s += 4) {
            const f32x4 v0 = src[(size_t)s * BC], v1 = src[(size_t)(s + 1) * BC], v2 = src[(size_t)(s + 2) * BC], v3 = src[(size_t)(s + 3) * BC];
            acc += v0; acc += v1; acc += v2; acc += v3;
        }
        for (; s < S; ++s) acc += src[(size_t)s * BC];
        out[i] = acc;
    }
}
unsigned grid_for(size_t total) { const size_t nb = (total + 255) / 256; return (unsigned)(nb < 1 ? 1 : (nb > (1u << 20) ? (1u << 20) : nb)); }

// the rows drivers' workspace: the B-row workspace of the plain drivers (LSTM1's side, the shared partial in b.P2, the sample sum in
// b.dZ2, dd / dZ1 / demb) and LSTM2's side at N rows behind it
struct BiRowsWs {
    BiWs b;
    int32_t* fed;
    float *P2, *G2, *C2, *H2, *O2, *dO2, *dZ2, *dE;
    void* bchain;
    size_t bchain_bytes;
};
bool bidir_rows_ok(const s2vt_dims* d, int B, int S)
{
    if (!bidir_dims_ok(d, B) || S < 1) return false;
    const long long T = (long long)d->n_video_lstm_step + d->n_caption_lstm_step;
    return (long long)S * B <= 0x7fffffffLL / T;                 // S * B, and every row count T * S * B of a product, within int
}
size_t bidir_rows_carve(const s2vt_dims* d, int B, int S, void* base, size_t cap, BiRowsWs* w)
{
    const size_t H = d->lstm_dim, E = d->word_dim, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step, T = Tv + Tc, N = (size_t)S * B, NH = N * H;
    BiRowsWs t;
    std::memset(&t, 0, sizeof(t));
    Carver c(base, cap);
    c.off = bidir_carve(d, B, base, cap, &t.b, true);
    t.fed = c.take<int32_t>(Tc * N);
    t.P2 = c.take<float>(T * 4 * NH); t.G2 = c.take<float>(T * 4 * NH);
    t.C2 = c.take<float>((T + 1) * NH); t.H2 = c.take<float>((T + 1) * NH); t.O2 = c.take<float>(T * NH);
    t.dO2 = c.take<float>(Tc * NH); t.dZ2 = c.take<float>(T * 4 * NH); t.dE = c.take<float>(Tc * N * E);
    t.bchain_bytes = s2vt_lstm_recurrence_bwd_scratch_bytes((int32_t)N, (int32_t)H);
    t.bchain = c.take<char>(t.bchain_bytes);
    if (w) *w = t;
    return c.off;
}
size_t bidir_sample_carve(const s2vt_dims* d, int B, int R, void* base, size_t cap, BiWs* w, float** st, float** out2, unsigned long long** packed,
                          int32_t** iw)
{
    const size_t RH = (size_t)R * d->lstm_dim;
    Carver c(base, cap);
    c.off = bidir_carve(d, B, base, cap, w, false);
    float* a = c.take<float>(4 * RH);                          // c | h, two parities
    float* o = c.take<float>(RH);
    unsigned long long* k = c.take<unsigned long long>(R);
    int32_t* i = c.take<int32_t>(3 * (size_t)R);
    if (st) { *st = a; *out2 = o; *packed = k; *iw = i; }
    return c.off;
}

}  // namespace

extern "C" {

size_t s2vt_bidir_sample_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t K, int32_t with_greedy)
{
    if (!bidir_dims_ok(d, B) || K < 0 || (K == 0 && !with_greedy) || ((long long)K + 1) * B > 0x7fffffffLL) return 0;
    return bidir_sample_carve(d, B, (K + (with_greedy ? 1 : 0)) * B, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int s2vt_bidir_sample(const s2vt_dims* d, const s2vt_bidir_params* p, const float* video, int32_t B, int32_t K, int32_t with_greedy, uint64_t seed,
                      int32_t video_base, int32_t lstm1_form, int32_t* sampled_out, int32_t* greedy_out, void* workspace, size_t workspace_bytes,
                      s2vt_stream stream)
{
    if (!bidir_dims_ok(d, B) || !bidir_params_ok(p) || !video || !workspace || K < 0 || (K == 0 && !with_greedy) || (K > 0 && !sampled_out) ||
        (with_greedy && !greedy_out) || ((long long)K + 1) * B > 0x7fffffffLL || lstm1_form < -1 || lstm1_form > 2)
        return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    const int H = d->lstm_dim, E = d->word_dim, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step, T = Tv + Tc, V = d->n_words;
    const int R = (K + (with_greedy ? 1 : 0)) * B;
    const size_t BH = (size_t)B * H, RH = (size_t)R * H;
    BiWs w;
    float *st, *out2;
    unsigned long long* packed;
    int32_t* iw;
    if (bidir_sample_carve(d, B, R, workspace, workspace_bytes, &w, &st, &out2, &packed, &iw) > workspace_bytes) return S2VT_E_WORKSPACE;
    int32_t *tok = iw, *vid = iw + R, *sid = iw + 2 * (size_t)R;
    hipStream_t hs = S(stream);
    const unsigned nb = (unsigned)((R + 255) / 256);
    hipLaunchKernelGGL(bidir_sample_ids_kernel, dim3(nb), dim3(256), 0, hs, B, K, R, Tc, -1, video_base, tok, sampled_out, greedy_out, vid, sid);
    HIP_TRY(hipGetLastError());
    // once per VIDEO: LSTM1, [fw ; bw] @ W2[:2H] for all T steps, LSTM2's Tv encode steps
    RC_TRY(bidir_lstm1(d, p, video, B, nullptr, w, lstm1_form, stream));
    s2vt_operand o1[2] = {{w.H1[0] + BH, nullptr, H, H, 0, 0}, {w.H1[1] + BH, w.rev, H, H, 0, 0}};
    RC_TRY(s2vt_gemm(o1, 2, p->lstm2_W, 4 * H, nullptr, nullptr, 0, w.P2, 4 * H, T * B, 4 * H, 0, -1, stream));
    HIP_TRY(hipMemsetAsync(w.C2, 0, BH * 4, hs));
    HIP_TRY(hipMemsetAsync(w.H2, 0, BH * 4, hs));
    RC_TRY(s2vt_lstm_recurrence_fwd(p->lstm2_W, 2 * H + E, p->lstm2_b, w.P2, (int64_t)B * 4 * H, 4 * H, Tv, w.C2, w.H2, nullptr, nullptr, B, H, Tv, 1.0f, 0,
                                    nullptr, nullptr, 0u, -1, w.chain, w.chain_bytes, stream));
    // Tc decode steps on the R rows: every row's chain goes on from ITS VIDEO's slice of the hoisted partial (row % B); step 0 reads the
    // video's encoder state the same way
    const float* cprev = w.C2 + (size_t)Tv * BH;
    const float* hprev = w.H2 + (size_t)Tv * BH;
    const NoiseIds none{nullptr, nullptr, 0};
    for (int t = 0; t < Tc; ++t) {
        float* cn = st + (size_t)(t & 1) * 2 * RH;
        float* hn = cn + RH;
        const int mod = t == 0 ? B : 0;
        ASeg segs[2] = {make_seg(p->Wemb, E, E, 2 * H, 0, tok), make_seg(hprev, H, H, 2 * H + E, mod)};
        HIP_TRY(lstm_call(segs, 2, p->lstm2_W, p->lstm2_b, cprev, mod, cn, hn, out2, nullptr, R, H, 1.0f, none, 0u, -1, hs,
                          w.P2 + (size_t)(Tv + t) * B * 4 * H, 4 * H, B));
        HIP_TRY(hipMemsetAsync(packed, 0, (size_t)R * 8, hs));                      // the pick is an atomicMax on a zeroed word per row
        RC_TRY(s2vt_vocab_pick(out2, H, p->embed_word_W, p->embed_word_b, R, H, V, vid, sid, t, seed, packed, tok, nullptr, -1, stream));
        hipLaunchKernelGGL(bidir_sample_ids_kernel, dim3(nb), dim3(256), 0, hs, B, K, R, Tc, t, 0, tok, sampled_out, greedy_out, vid, sid);
        HIP_TRY(hipGetLastError());
        cprev = cn; hprev = hn;
    }
    return S2VT_OK;
}

int s2vt_bidir_sample_sum(const float* dz, float* out, int32_t T, int32_t B, int32_t S, int32_t C, s2vt_stream stream)
{
    if (!dz || !out || T < 1 || B < 1 || S < 1 || C < 4 || (C & 3) || (long long)S * B > 0x7fffffffLL / T) return S2VT_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(dz) | reinterpret_cast<uintptr_t>(out)) & 15u) return S2VT_E_ALIGN;
    hipLaunchKernelGGL(bidir_sample_sum_kernel, dim3(grid_for((size_t)T * B * (C / 4))), dim3(256), 0, s2vt_api::S(stream), reinterpret_cast<const f32x4*>(dz),
                       reinterpret_cast<f32x4*>(out), T * B, B, S, C / 4);
    HIP_TRY(hipGetLastError());
    return S2VT_OK;
}

size_t s2vt_bidir_rows_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t S)
{
    return bidir_rows_ok(d, B, S) ? bidir_rows_carve(d, B, S, nullptr, 0, nullptr) : 0;
}

int s2vt_bidir_teacher_forced_fwd_rows(const s2vt_dims* d, const s2vt_bidir_params* p, const float* video, int32_t B, int32_t S, const int32_t* caption,
                                       float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id, int32_t lstm1_form, float* logits_out,
                                       void* workspace, size_t workspace_bytes, s2vt_stream stream)
{
    if (!bidir_rows_ok(d, B, S) || !bidir_params_ok(p) || !video || !caption || !logits_out || !workspace || !(keep > 0.0f) || keep > 1.0f ||
        (keep < 1.0f && (!video_id || !sample_id)) || lstm1_form < -1 || lstm1_form > 2)
        return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    BiRowsWs w;
    if (bidir_rows_carve(d, B, S, workspace, workspace_bytes, &w) > workspace_bytes) return S2VT_E_WORKSPACE;
    const int H = d->lstm_dim, E = d->word_dim, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step, T = Tv + Tc, V = d->n_words, N = S * B;
    const size_t BH = (size_t)B * H, NH = (size_t)N * H;
    hipStream_t hs = s2vt_api::S(stream);
    // per VIDEO: LSTM1 and [fw ; bw] @ W2[:2H] for all T steps, on T * B rows
    RC_TRY(bidir_lstm1(d, p, video, B, nullptr, w.b, lstm1_form, stream));
    s2vt_operand o1[2] = {{w.b.H1[0] + BH, nullptr, H, H, 0, 0}, {w.b.H1[1] + BH, w.b.rev, H, H, 0, 0}};
    RC_TRY(s2vt_gemm(o1, 2, p->lstm2_W, 4 * H, nullptr, nullptr, 0, w.b.P2, 4 * H, T * B, 4 * H, 0, -1, stream));
    // per ROW: the encode steps' partial is the video's; a decode step's chain goes on from the video's slice with the fed word's rows of
    // Wemb (continuing a chain from a carried partial is exact: the bits of the one three-segment product on the tiled block)
    hipLaunchKernelGGL(bidir_rows_fed_kernel, dim3(grid_for((size_t)Tc * N)), dim3(256), 0, hs, N, Tc, V, caption, w.fed);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(bidir_tile_rows_kernel, dim3(grid_for((size_t)Tv * N * H)), dim3(256), 0, hs, reinterpret_cast<const f32x4*>(w.b.P2),
                       reinterpret_cast<f32x4*>(w.P2), Tv, B, N, H);
    HIP_TRY(hipGetLastError());
    for (int t = 0; t < Tc; ++t) {
        GemmArgs a;
        std::memset(&a, 0, sizeof(a));
        a.seg[0] = make_seg(p->Wemb, E, E, 2 * H, 0, w.fed + (size_t)t * N);
        a.nseg = 1;
        a.W = p->lstm2_W; a.ldw = 4 * H; a.M = N; a.N = 4 * H;
        a.cinit = w.b.P2 + (size_t)(Tv + t) * B * 4 * H; a.ldcinit = 4 * H; a.cinit_rowmod = B;
        a.C = w.P2 + (size_t)(Tv + t) * N * 4 * H; a.ldc = 4 * H;
        HIP_TRY(launch_gemm(a, EPI_STORE, -1, hs));
    }
    HIP_TRY(hipMemsetAsync(w.C2, 0, NH * 4, hs));
    HIP_TRY(hipMemsetAsync(w.H2, 0, NH * 4, hs));
    // LSTM2 over all T steps on the N rows; its DropoutWrapper on its own Philox codes, keyed per row
    RC_TRY(s2vt_lstm_recurrence_fwd(p->lstm2_W, 2 * H + E, p->lstm2_b, w.P2, (int64_t)N * 4 * H, 4 * H, T, w.C2, w.H2, w.G2, w.O2, N, H, T, keep, seed,
                                    video_id, sample_id, 512u, -1, w.b.chain, w.b.chain_bytes, stream));
    s2vt_operand o{w.O2 + (size_t)Tv * NH, nullptr, H, H, 0, 0};
    return s2vt_gemm(&o, 1, p->embed_word_W, V, p->embed_word_b, nullptr, 0, logits_out, V, Tc * N, V, 0, -1, stream);
}

int s2vt_bidir_bptt_bwd_rows(const s2vt_dims* d, const s2vt_bidir_params* p, const s2vt_bidir_params* grads, const float* video, int32_t B, int32_t S,
                             const float* dlogits, float keep, uint64_t seed, const int32_t* video_id, const int32_t* sample_id, void* workspace,
                             size_t workspace_bytes, s2vt_stream stream)
{
    if (!bidir_rows_ok(d, B, S) || !bidir_params_ok(p) || !bidir_params_ok(grads) || !video || !dlogits || !workspace || !(keep > 0.0f) || keep > 1.0f ||
        (keep < 1.0f && (!video_id || !sample_id)))
        return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    BiRowsWs r;
    if (bidir_rows_carve(d, B, S, workspace, workspace_bytes, &r) > workspace_bytes) return S2VT_E_WORKSPACE;
    const BiWs& w = r.b;
    const int H = d->lstm_dim, E = d->word_dim, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step, T = Tv + Tc, V = d->n_words, D = d->dim_image;
    const int N = S * B;
    const size_t BH = (size_t)B * H, NH = (size_t)N * H;
    const s2vt_bidir_params* g = grads;
    hipStream_t hs = s2vt_api::S(stream);
    // ---- what sees a per-sample operand: N rows
    RC_TRY(s2vt_gemm_tn(r.O2 + (size_t)Tv * NH, H, nullptr, dlogits, V, g->embed_word_W, V, Tc * N, H, V, 1, stream));
    RC_TRY(s2vt_colsum(dlogits, V, Tc * N, V, g->embed_word_b, stream));
    s2vt_operand dl{dlogits, nullptr, V, V, 0, 0};
    RC_TRY(s2vt_gemm_nt(&dl, 1, p->embed_word_W, V, nullptr, nullptr, 0, r.dO2, H, Tc * N, H, 0, -1, stream));
    RC_TRY(s2vt_lstm_recurrence_bwd(p->lstm2_W, 2 * H + E, r.G2, r.C2, r.dO2, (int64_t)NH, H, Tv, r.dZ2, N, H, T, keep, seed, video_id, sample_id, 512u, -1,
                                    r.bchain, r.bchain_bytes, stream));
    float* gW2 = g->lstm2_W;
    const float* dZ2d = r.dZ2 + (size_t)Tv * N * 4 * H;
    RC_TRY(s2vt_gemm_tn(p->Wemb, E, r.fed, dZ2d, 4 * H, gW2 + (size_t)2 * H * 4 * H, 4 * H, Tc * N, E, 4 * H, 1, stream));
    RC_TRY(s2vt_gemm_tn(r.H2, H, nullptr, r.dZ2, 4 * H, gW2 + (size_t)(2 * H + E) * 4 * H, 4 * H, T * N, H, 4 * H, 1, stream));
    s2vt_operand zd{dZ2d, nullptr, 4 * H, 4 * H, 0, 0};
    RC_TRY(s2vt_gemm_nt(&zd, 1, p->lstm2_W + (size_t)2 * H * 4 * H, 4 * H, nullptr, nullptr, 0, r.dE, E, Tc * N, E, 0, -1, stream));
    RC_TRY(s2vt_embed_scatter_add(r.dE, E, r.fed, Tc * N, E, g->Wemb, stream));
    // ---- the sample sum, then what sees the video only: T * B rows
    RC_TRY(s2vt_bidir_sample_sum(r.dZ2, w.dZ2, T, B, S, 4 * H, stream));
    RC_TRY(s2vt_gemm_tn(w.H1[0] + BH, H, nullptr, w.dZ2, 4 * H, gW2, 4 * H, T * B, H, 4 * H, 1, stream));
    RC_TRY(s2vt_gemm_tn(w.H1[1] + BH, H, w.rev, w.dZ2, 4 * H, gW2 + (size_t)H * 4 * H, 4 * H, T * B, H, 4 * H, 1, stream));
    RC_TRY(s2vt_colsum(w.dZ2, 4 * H, T * B, 4 * H, g->lstm2_b, stream));
    s2vt_operand z{w.dZ2, nullptr, 4 * H, 4 * H, 0, 0}, zr{w.dZ2, w.rev, 4 * H, 4 * H, 0, 0};
    RC_TRY(s2vt_gemm_nt(&z, 1, p->lstm2_W, 4 * H, nullptr, nullptr, 0, w.dd[0], H, T * B, H, 0, -1, stream));
    RC_TRY(s2vt_gemm_nt(&zr, 1, p->lstm2_W + (size_t)H * 4 * H, 4 * H, nullptr, nullptr, 0, w.dd[1], H, T * B, H, 0, -1, stream));
    // ---- LSTM1 on B rows, as s2vt_bidir_bptt_bwd
    const float* W1[2] = {p->lstm1_fw_W, p->lstm1_bw_W};
    float* gW1[2] = {g->lstm1_fw_W, g->lstm1_bw_W};
    float* gb1[2] = {g->lstm1_fw_b, g->lstm1_bw_b};
    for (int k = 0; k < 2; ++k) {
        RC_TRY(s2vt_lstm_recurrence_bwd(W1[k], E, w.G1[k], w.C1[k], w.dd[k], (int64_t)BH, H, 0, w.dZ1, B, H, T, 1.0f, 0, nullptr, nullptr, 0u, -1, w.bchain,
                                        w.bchain_bytes, stream));
        const float* dZf = w.dZ1 + (size_t)(k ? Tc : 0) * B * 4 * H;            // the steps that saw a frame
        RC_TRY(s2vt_gemm_tn(w.emb, E, k ? w.framesb : w.tm, dZf, 4 * H, gW1[k], 4 * H, Tv * B, E, 4 * H, 1, stream));
        RC_TRY(s2vt_gemm_tn(w.H1[k], H, nullptr, w.dZ1, 4 * H, gW1[k] + (size_t)E * 4 * H, 4 * H, T * B, H, 4 * H, 1, stream));
        RC_TRY(s2vt_colsum(w.dZ1, 4 * H, T * B, 4 * H, gb1[k], stream));
        s2vt_operand f{dZf, k ? w.srcb : w.srcf, 4 * H, 4 * H, 0, 0};
        RC_TRY(s2vt_gemm_nt(&f, 1, W1[k], 4 * H, nullptr, k ? w.demb[0] : nullptr, k ? E : 0, w.demb[k], E, B * Tv, E, 0, -1, stream));
    }
    RC_TRY(s2vt_gemm_tn(video, D, nullptr, w.demb[1], E, g->encode_image_W, E, B * Tv, D, E, 1, stream));
    return s2vt_colsum(w.demb[1], E, B * Tv, E, g->encode_image_b, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// Batched beam search on this model (final_beam_search.py:201-294 for B videos at once, as beam.hip runs it for the S2VT models).  What a
// hypothesis shares with its video -- both LSTM1 directions, [fw ; bw] @ W2[:2H], LSTM2's encode steps -- is s2vt_bidir_sample's prefix; a
// decode step is that driver's fused cell launch in its gathered-state form (gemm_mfma.h, GS): the Wemb rows by word, h / c by parent and
// the partial by video are all read through index arrays, so nothing is copied into dense scratch first.
namespace {

constexpr int kBeamTopkMax = 16;

// the clamped indices of the step's R rows: idx[0][m] = video (the partial's row), idx[1][m] = the state's row (t = 0: the video, in the
// encode history's slot Tv; else the parent, a row of the other parity buffer), idx[2][m] = the word.  Indices are device data the host
// does not see here: out-of-range values are clamped into range, so nothing is read outside the workspace or the embedding table.
__global__ void bidir_beam_index_kernel(const int32_t* video_of_row, const int32_t* parent, const int32_t* word, int t, int R, int B, int Rmax, int V,
                                        int32_t* idx)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= R) return;
    int vid = video_of_row[m];
    vid = vid < 0 ? 0 : (vid >= B ? B - 1 : vid);
    int src = vid;
    if (t > 0) {
        const int par = parent[m];
        src = par < 0 ? 0 : (par >= Rmax ? Rmax - 1 : par);
    }
    const int wd = word[m];
    idx[m] = vid;
    idx[(size_t)Rmax + m] = src;
    idx[2 * (size_t)Rmax + m] = wd < 0 ? 0 : (wd >= V ? V - 1 : wd);
}

struct BiBeamWs {
    BiWs b;                             // the decode workspace's encode part (bidir_carve, no gates)
    float* st;                          // LSTM2 state of the hypotheses, two parities of (c | h) [Rmax][H]
    float* logits;                      // [Rmax][V] (when the caller does not ask for them)
    int32_t* idx;                       // [3][Rmax]
};
bool bidir_beam_shape_ok(const s2vt_dims* d, int B, int beam)
{
    return bidir_dims_ok(d, B) && beam >= 1 && beam <= kBeamTopkMax && (int64_t)B * beam <= 0x7fffffffLL / 4;
}
size_t bidir_beam_carve(const s2vt_dims* d, int B, int beam, void* base, size_t cap, BiBeamWs* w)
{
    const size_t Rmax = (size_t)B * beam, H = d->lstm_dim, V = d->n_words;
    BiBeamWs t;
    Carver c(base, cap);
    c.off = bidir_carve(d, B, base, cap, &t.b, false);
    t.st = c.take<float>(4 * Rmax * H);
    t.logits = c.take<float>(Rmax * V);
    t.idx = c.take<int32_t>(3 * Rmax);
    if (w) *w = t;
    return c.off;
}

}  // namespace

extern "C" {

size_t s2vt_bidir_beam_workspace_bytes(const s2vt_dims* d, int32_t B, int32_t beam)
{
    return bidir_beam_shape_ok(d, B, beam) ? bidir_beam_carve(d, B, beam, nullptr, 0, nullptr) : 0;
}

int s2vt_bidir_beam_encode(const s2vt_dims* d, const s2vt_bidir_params* p, const float* video, int32_t B, int32_t beam, int32_t lstm1_form,
                           void* workspace, size_t workspace_bytes, s2vt_stream stream)
{
    if (!bidir_beam_shape_ok(d, B, beam) || !bidir_params_ok(p) || !video || !workspace || lstm1_form < -1 || lstm1_form > 2) return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    BiBeamWs bw;
    if (bidir_beam_carve(d, B, beam, workspace, workspace_bytes, &bw) > workspace_bytes) return S2VT_E_WORKSPACE;
    if (chain_fault()) return S2VT_E_CHAIN_TIMEOUT;
    const BiWs& w = bw.b;
    const int H = d->lstm_dim, E = d->word_dim, Tv = d->n_video_lstm_step, Tc = d->n_caption_lstm_step, T = Tv + Tc;
    const size_t BH = (size_t)B * H;
    hipStream_t hs = s2vt_api::S(stream);
    // once per VIDEO, as s2vt_bidir_sample: LSTM1, [fw ; bw] @ W2[:2H] for all T steps, LSTM2's Tv encode steps
    RC_TRY(bidir_lstm1(d, p, video, B, nullptr, w, lstm1_form, stream));
    s2vt_operand o1[2] = {{w.H1[0] + BH, nullptr, H, H, 0, 0}, {w.H1[1] + BH, w.rev, H, H, 0, 0}};
    RC_TRY(s2vt_gemm(o1, 2, p->lstm2_W, 4 * H, nullptr, nullptr, 0, w.P2, 4 * H, T * B, 4 * H, 0, -1, stream));
    HIP_TRY(hipMemsetAsync(w.C2, 0, BH * 4, hs));
    HIP_TRY(hipMemsetAsync(w.H2, 0, BH * 4, hs));
    return s2vt_lstm_recurrence_fwd(p->lstm2_W, 2 * H + E, p->lstm2_b, w.P2, (int64_t)B * 4 * H, 4 * H, Tv, w.C2, w.H2, nullptr, nullptr, B, H, Tv, 1.0f, 0,
                                    nullptr, nullptr, 0u, -1, w.chain, w.chain_bytes, stream);
}

int s2vt_bidir_beam_step(const s2vt_dims* d, const s2vt_bidir_params* p, int32_t B, int32_t beam, int32_t t, int32_t R, const int32_t* video_of_row,
                         const int32_t* parent, const int32_t* word, int32_t k, int32_t* top_ids, float* top_logp, float* logits_out,
                         void* workspace, size_t workspace_bytes, s2vt_stream stream)
{
    if (!bidir_beam_shape_ok(d, B, beam) || !bidir_params_ok(p) || !video_of_row || !parent || !word || !top_ids || !top_logp || !workspace)
        return S2VT_E_BADARG;
    if (t < 0 || t >= d->n_caption_lstm_step || R < 0 || R > B * beam || k < 1 || k > kBeamTopkMax || k > d->n_words) return S2VT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 255u) return S2VT_E_ALIGN;
    BiBeamWs bw;
    if (bidir_beam_carve(d, B, beam, workspace, workspace_bytes, &bw) > workspace_bytes) return S2VT_E_WORKSPACE;
    if (R == 0) return S2VT_OK;
    const BiWs& w = bw.b;
    const int H = d->lstm_dim, E = d->word_dim, Tv = d->n_video_lstm_step, V = d->n_words, Rmax = B * beam;
    const size_t BH = (size_t)B * H, RH = (size_t)Rmax * H;
    hipStream_t hs = s2vt_api::S(stream);
    // 1. the clamped [3][R] indices
    hipLaunchKernelGGL(bidir_beam_index_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, hs, video_of_row, parent, word, (int)t, (int)R, (int)B,
                       Rmax, V, bw.idx);
    HIP_TRY(hipGetLastError());
    const int32_t *vid = bw.idx, *src = bw.idx + Rmax, *wd = bw.idx + 2 * (size_t)Rmax;
    // 2. the fused cell launch, gathered-state form: step t writes parity t & 1 and reads the other (step 0: slot Tv of the encode history)
    float* cn = bw.st + (size_t)(t & 1) * 2 * RH;
    float* hn = cn + RH;
    const float* cprev = t == 0 ? w.C2 + (size_t)Tv * BH : bw.st + (size_t)((t - 1) & 1) * 2 * RH;
    const float* hprev = t == 0 ? w.H2 + (size_t)Tv * BH : cprev + RH;
    ASeg segs[2] = {make_seg(p->Wemb, E, E, 2 * H, 0, wd), make_seg(hprev, H, H, 2 * H + E, 0, src)};
    HIP_TRY(lstm_call(segs, 2, p->lstm2_W, p->lstm2_b, cprev, 0, cn, hn, nullptr, nullptr, R, H, 1.0f, NoiseIds{nullptr, nullptr, 0}, 0u, -1, hs,
                      w.P2 + (size_t)(Tv + t) * B * 4 * H, 4 * H, 0, nullptr, nullptr, nullptr, vid, src));
    // 3. vocabulary logits from h' (no dropout, no residual: no separate `out`), 4. top-k words and their log-probabilities
    float* logits = logits_out ? logits_out : bw.logits;
    ASeg so = make_seg(hn, H, H, 0);
    HIP_TRY(store_call(&so, 1, p->embed_word_W, V, p->embed_word_b, logits, V, R, V, 0, -1, hs));
    HIP_TRY(launch_vocab_topk(logits, V, R, V, k, top_ids, top_logp, hs));
    return S2VT_OK;
}

}  // extern "C"
