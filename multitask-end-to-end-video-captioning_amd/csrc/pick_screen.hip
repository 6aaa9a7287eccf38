// pick_screen.hip -- the sampler's screened vocabulary pick: approximate logits from a bf16 product (bwd_bf16.hip: one
// product, gemm_bf16x1_nt, by default; the three-product split form, gemm_bf16x3_nt, under S2VT_PICK_PRODUCTS=3 or S2VT_PICK_TILE) select, under a proven margin, the few columns of a row that can still win it; only those get the
// exact ascending-k fp32 chain and the exact Gumbel expression of the PICK epilogue (gemm_mfma.h).  The packed pick a row ends with is
// the maximum exact key over a set of columns that contains the exact winner: the ids are those of the fp32 pick, bit for bit.
//
// Why the winner survives: with e >= |exact key - fast key| for every column, w the exact winner and f the fast argmax,
//     fast_w >= exact_w - e >= exact_f - e >= fast_f - 2 e.
// e = m + kGumbelScreenMargin + slack, m = C |h| max_v |W[:, v]|: the three kept products of hi = bf16(x), lo = bf16(x - hi) miss at
// most 2^-15 |h_k w_k| per term (|lo| <= 2^-8 |x|, so the dropped lo x lo product is up to 2^-16 of the term, and |x - hi - lo| <=
// 2^-17 |x| on either operand; measured 3.1e-5 = 1.02 x 2^-15 of sum |h_k w_k| on operands built for it, tests/test_gpu_pick_margins.py),
// the fp32 chain is within K 2^-24 sum |h_k w_k| of the true sum, and 3 K roundings of the bf16 MFMA accumulation within 2^-22
// relative each add 3 K 2^-22 sum |h_k w_k|; sum |h_k w_k| <= |h| |w| -- 0.84 C with C = 2^-10 at K = 1024, C scaled by ceil(K / 1024)
// above.  slack covers the roundings of (logit + bias) + noise on either side.
//
// One product, L1 = sum_k bf16(h_k) bf16(w_k) in fp32: the same e, with m built from what the two casts really miss.  With
// h^ = bf16(h), w^ = bf16(w): h_k w_k - h^_k w^_k = (h_k - h^_k) w_k + h^_k (w_k - w^_k), so by Cauchy-Schwarz
//     |sum h_k w_k - sum h^_k w^_k| <= |h - h^| |w| + |h^| |w - w^|,   |h^| <= (1 + 2^-8) |h|
// (an RNE cast misses by at most half a bf16 ulp, 2^-8 2^e for |x| in [2^e, 2^(e+1)): under 2^-8 relative, approached just above a power of
// two).  |h - h^| is summed by the resolve kernel beside |h| (x - bf16(x) is exact in fp32), max_v |w_v - w^_v| by the prepare kernel beside
// max_v |w_v| (nwmax[1]); both rounded up by 1.001 as the norms are.  The products h^_k w^_k are exact in fp32; K roundings of the
// accumulation within 2^-22 relative each add K 2^-22 sum |h^_k w^_k| <= 1.008 K 2^-22 |h| |w|, and the fp32 chain is within K 2^-24
// sum |h_k w_k| of the true sum: 2^-12 1.008 + 2^-14 = 3.1e-4 at K = 1024, inside kPickAcc1 = 2^-11 = 4.9e-4, scaled by ceil(K / 1024) above.
//     m1 = 2^-11 ceil(K / 1024) |h| max|w| + |h - h^| max|w| + 1.004 |h| max|w - w^|.
// A constant in place of the two measured norms would have to be C1 = 2^-7 + 2^-11 (each cast up to 2^-8 of its operand: the worst-cast
// operands of tests/pick_screen1_cases.py reach 0.994 x 2^-7 of sum |h_k w_k|) -- that is what s2vt_gemm_bf16x1_nt promises on its own, and
// it was measured as a margin: 2.5 - 5.5 survivors per row where the measured form leaves 2.1 - 3.8 (a cast's rms miss is 0.4 x 2^-8 on
// ordinary operands), and the resolve kernel took back most of what the product gave (profiles/NOTES.md).  Squares of misses below 2^-63 underflow, as those of |h| and
// |w| themselves do.  An operand that rounds to +-inf in bf16 makes its miss, the norm and the margin non-finite: the row takes every
// column, exactly.  The price of a margin wider than the three-product one is more survivors per row, each resolved exactly; the product
// drops two of three MFMA passes and two of four operand planes.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "detmath.h"
#include "internal.h"

namespace s2vt {
namespace {

constexpr int kResThreads = 512, kResWaves = kResThreads / 64;
constexpr int kResChunk = 4 * kResThreads, kResList = 2 * kResChunk;   // columns keyed per pass (one group of 4 per thread); survivors listed at most
constexpr int kResRegChunks = 6;                                       // up to 6 chunks (|V| <= 12288) a thread's fast keys stay in registers
constexpr float kPickC3 = 9.765625e-04f;                               // C = 2^-10: the three-product screen's margin constant
constexpr float kPickAcc1 = 4.8828125e-04f;                            // 2^-11: the one-product screen's accumulation share (the casts' misses are measured)

// x - bf16(x) (RNE), exact in fp32 for finite x with a finite bf16(x): what a cast to the hi plane leaves behind
__device__ __forceinline__ float bf16_miss(float x) { return x - __uint_as_float(pack2(x, 0.0f) << 16); }

// Once per sampler call: Wt[v][k] = W[k][v] (fp32, rows ldt apart, zeros for H <= k < ldt) -- a survivor's column of W is then one
// contiguous row instead of H cache lines -- and nwmax = max_v |W[:, v]|_2 rounded up, as the bits of a non-negative float folded with an
// integer atomicMax (a non-finite norm has the larger bits and wins: the resolve kernel then takes every column).  64 columns per
// workgroup, 64 x 64 tiles through LDS; wave w sums the squares of rows k = w (mod 4), the four partials are added in a fixed order.
// nwmax[1] = max_v |W[:, v] - bf16(W[:, v])|_2 the same way: what the cast of W to its hi plane misses, for the one-product screen's margin.
__global__ __launch_bounds__(256) void pick_screen_prepare_kernel(const float* __restrict__ W, int ldw, int H, int V, float* __restrict__ Wt, int ldt,
                                                                  uint32_t* __restrict__ nwmax)
{
    __shared__ float t[64][65];
    __shared__ float part[4][64], partd[4][64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c0 = blockIdx.x * 64, col = c0 + lane;
    const int vv = tid >> 2, q = tid & 3;                    // the transposed store: column c0 + vv, k quarter q of the tile
    float s = 0.0f, sd = 0.0f;
    for (int k0 = 0; k0 < ldt; k0 += 64) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int kk = w + 4 * j;
            const float x = k0 + kk < H && col < V ? W[(size_t)(k0 + kk) * ldw + col] : 0.0f;
            const float d = bf16_miss(x);
            s += x * x;
            sd += d * d;
            t[kk][lane] = x;
        }
        __syncthreads();
        if (c0 + vv < V)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kk = q * 16 + i * 4;
                if (k0 + kk < ldt)                              // (ldt % 4 == 0: the four floats lie inside the row)
                    *reinterpret_cast<float4*>(Wt + (size_t)(c0 + vv) * ldt + k0 + kk) = make_float4(t[kk][vv], t[kk + 1][vv], t[kk + 2][vv], t[kk + 3][vv]);
            }
        __syncthreads();
    }
    part[w][lane] = s;
    partd[w][lane] = sd;
    __syncthreads();
    if (w == 0) {
        // (the sum of squares is within (H / 4 + 4) 2^-24 relative of the true one, its root within half of that: 1.001 rounds up)
        float n = col < V ? sqrtf((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane])) * 1.001f : 0.0f;
        float nd = col < V ? sqrtf((partd[0][lane] + partd[1][lane]) + (partd[2][lane] + partd[3][lane])) * 1.001f : 0.0f;
        uint32_t b = __float_as_uint(n), bd = __float_as_uint(nd);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)b, off, 64), od = (uint32_t)__shfl_xor((int)bd, off, 64);
            b = o > b ? o : b;
            bd = od > bd ? od : bd;
        }
        if (lane == 0) { atomicMax(nwmax, b); atomicMax(nwmax + 1, bd); }
    }
}

struct PickResolveArgs {
    float* L; int ldl;                       // approximate logits [R][ldl], ldl % 4 == 0, 16-byte aligned rows; read once and left as they are
                                             // up to 12288 columns, overwritten with the fast keys above (nothing reads either afterwards)
    const float* bias;                       // [V]
    const float* h; int ldh;                 // the step's fp32 rows [R][H]
    const float* Wt; int ldt;                // embed_word_W^T [V][ldt], ldt % 4 == 0, zeros past H
    const int32_t* vid; const int32_t* sid;
    uint32_t seed_lo, seed_hi; int step;
    unsigned long long* pick; int pick_stride;
    const float* nwmax;                      // [0] max_v |W[:, v]|, [1] max_v |W[:, v] - bf16(W[:, v])|, both rounded up
    unsigned long long* counters;            // PickScreenWs::counters
    int H, V; float C;
    int one;                                 // the one-product screen: m also takes the casts' measured misses
};

// the approximate logits of columns c0 .. c0 + 3 (c0 % 4 == 0, c0 < V); columns >= V come back as 0
__device__ __forceinline__ void load_logits4(const PickResolveArgs& a, const float* Lr, int c0, float (&l)[4])
{
    if (c0 + 4 <= a.V) {
        const float4 x = *reinterpret_cast<const float4*>(Lr + c0);
        l[0] = x.x; l[1] = x.y; l[2] = x.z; l[3] = x.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) l[j] = c0 + j < a.V ? Lr[c0 + j] : 0.0f;
    }
}

// v = L~ + bias and the fast key of columns c0 .. c0 + 3 from their logits l: one Philox block, counter (col >> 2, video, sample, step) as
// the PICK epilogue's; argmax rows (sid < 0) carry no noise.  Columns >= V are not looked at.
__device__ __forceinline__ void screen_keys4(const PickResolveArgs& a, const float (&l)[4], int c0, int vid, int sid, float (&v)[4],
                                             float (&ka)[4])
{
    u32x4 blk = {0u, 0u, 0u, 0u};
    if (sid >= 0) blk = philox4x32_10((uint32_t)c0 >> 2, (uint32_t)vid, (uint32_t)sid, (uint32_t)a.step, a.seed_lo, a.seed_hi);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = l[j] + (c0 + j < a.V ? a.bias[c0 + j] : 0.0f);
        ka[j] = sid >= 0 ? v[j] + gumbel_fast_from_word(pick_word(blk, (uint32_t)j)) : v[j];
    }
}

// The exact keys of the listed columns, one survivor per wave at a time, folded into *best.  Lane l holds terms k = l CH .. l CH + CH - 1
// of the row (registers, once) and of the column (its row of Wt); the chain then walks the lanes in order:
// every lane continues the running sum with its own CH terms, and lane l's result is the one carried on -- one ascending-k fmaf chain
// from +0, the PICK epilogue's instruction sequence, then + bias, + noise, + 0.  (Terms past H are 0 * 0: they leave the sum as it is.)
template <int CH>
__device__ __forceinline__ void resolve_listed(const PickResolveArgs& a, const float* hs, const int* list, int n, int wave, int lane, int vid,
                                               int sid, unsigned long long* best)
{
    float hr[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) hr[i] = lane * CH + i < a.H ? hs[lane * CH + i] : 0.0f;
    const int nl = (a.H + CH - 1) / CH;
    for (int s = wave; s < n; s += kResWaves) {
        const int col = list[s];
        float wr[CH];
#pragma unroll
        for (int i = 0; i < CH; i += 4) {
            const int k = lane * CH + i;
            const float4 x = k < a.ldt ? *reinterpret_cast<const float4*>(a.Wt + (size_t)col * a.ldt + k) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            wr[i] = x.x; wr[i + 1] = x.y; wr[i + 2] = x.z; wr[i + 3] = x.w;
        }
        float acc = 0.0f;
        for (int l = 0; l < nl; ++l) {
            float x = acc;
#pragma unroll
            for (int i = 0; i < CH; ++i) x = __builtin_fmaf(hr[i], wr[i], x);
            acc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l));
        }
        float v = acc + a.bias[col];
        if (sid >= 0) {
            const u32x4 blk = philox4x32_10((uint32_t)col >> 2, (uint32_t)vid, (uint32_t)sid, (uint32_t)a.step, a.seed_lo, a.seed_hi);
            v = v + gumbel_from_word(pick_word(blk, (uint32_t)col & 3u));
        }
        v = v + 0.0f;  // -0 -> +0 so that the integer order equals the float order
        if (lane == 0) atomicMax(best, ((unsigned long long)orderable(v) << 32) | (uint32_t)(~(uint32_t)col));
    }
}

// One workgroup per row; no grid-wide waits, every loop bounded by V or H.  Pass 1 keys every column and takes the row's fast maximum,
// the largest magnitude and |h|; pass 2 counts the survivors among the keys, lists them in LDS and resolves them.  A row with more
// survivors than the list holds goes chunk by chunk instead: no survivor is ever dropped.  A row with a non-finite key, norm or margin
// takes every column (slow, equal).
// A thread owns the same 4 columns of every chunk of kResChunk in every pass.  REG (|V| <= kResRegChunks chunks): its keys stay in a
// statically indexed register array from pass 1 on -- the logits are read once, all chunks' loads issued ahead of the Philox work, and
// nothing is written back.  Otherwise pass 1 leaves the keys where the logits were and pass 2 reads them back (each thread its own).
template <bool REG>
__global__ __launch_bounds__(kResThreads) void pick_resolve_kernel(PickResolveArgs a)
{
    __shared__ float hs[kPickScreenMaxH];
    __shared__ int list[kResList];
    __shared__ int nlist;
    __shared__ float red[4][kResWaves];
    __shared__ int nwave[kResWaves];
    __shared__ unsigned long long best;
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sid = a.sid[row], vid = a.vid[row];
    float* const Lr = a.L + (size_t)row * a.ldl;
    const float inf = __builtin_inff();

    float mx = -inf, amax = 0.0f, ss = 0.0f, sd = 0.0f;
    int bad = 0;
    auto fold = [&](int c0, const float (&v)[4], const float (&ka)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c0 + j < a.V) {
                mx = fmaxf(mx, ka[j]);
                amax = fmaxf(amax, fmaxf(fabsf(v[j]), fabsf(ka[j])));
                bad |= !(fabsf(ka[j]) < inf);
            }
    };
    float kr[REG ? kResRegChunks : 1][4];                                  // REG: the fast keys of columns tid * 4 + c * kResChunk + j
    if constexpr (REG) {
        // every chunk's 16 bytes first, without a branch: a group that starts below V lies inside the row (ldl = V rounded up to 4; what
        // it holds past V is not looked at), one that starts past V reads the row's last group instead
        float4 x[kResRegChunks];
#pragma unroll
        for (int c = 0; c < kResRegChunks; ++c) x[c] = *reinterpret_cast<const float4*>(Lr + min(tid * 4 + c * kResChunk, a.ldl - 4));
#pragma unroll
        for (int c = 0; c < kResRegChunks; ++c) {
            const int c0 = tid * 4 + c * kResChunk;
            kr[c][0] = kr[c][1] = kr[c][2] = kr[c][3] = 0.0f;
            if (c0 < a.V) {
                const float l[4] = {x[c].x, x[c].y, x[c].z, x[c].w};
                float v[4];
                screen_keys4(a, l, c0, vid, sid, v, kr[c]);
                fold(c0, v, kr[c]);
            }
        }
    } else {
        for (int c0 = tid * 4; c0 < a.V; c0 += kResChunk) {
            float l[4], v[4], ka[4];
            load_logits4(a, Lr, c0, l);
            screen_keys4(a, l, c0, vid, sid, v, ka);
            fold(c0, v, ka);
            // the fast keys take the logits' place: pass 2 reads them back (each thread its own) instead of drawing the noise again
            if (c0 + 4 <= a.V) *reinterpret_cast<float4*>(Lr + c0) = make_float4(ka[0], ka[1], ka[2], ka[3]);
            else
                for (int j = 0; c0 + j < a.V; ++j) Lr[c0 + j] = ka[j];
        }
    }
    for (int k = tid; k < a.H; k += kResThreads) {
        const float x = a.h[(size_t)row * a.ldh + k], d = bf16_miss(x);
        hs[k] = x;
        ss += x * x;
        sd += d * d;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        amax = fmaxf(amax, __shfl_xor(amax, off, 64));
        ss += __shfl_xor(ss, off, 64);
        sd += __shfl_xor(sd, off, 64);
    }
    if (lane == 0) { red[0][wave] = mx; red[1][wave] = amax; red[2][wave] = ss; red[3][wave] = sd; }
    if (tid == 0) { best = 0ull; nlist = 0; }
    bad = __syncthreads_or(bad);
    float rmx = red[0][0], rabs = red[1][0], sq = red[2][0], sqd = red[3][0];
#pragma unroll
    for (int w = 1; w < kResWaves; ++w) { rmx = fmaxf(rmx, red[0][w]); rabs = fmaxf(rabs, red[1][w]); sq += red[2][w]; sqd += red[3][w]; }
    const float nh = sqrtf(sq) * 1.001f;
    float m = a.C * nh * *a.nwmax;
    // one product: + |h - bf16(h)| max|w| + |bf16(h)| max|w - bf16(w)|, |bf16(h)| <= (1 + 2^-8) |h| (the header comment)
    if (a.one) m = m + (sqrtf(sqd) * 1.001f * a.nwmax[0] + 1.004f * nh * a.nwmax[1]);
    // the roundings of (logit + bias) + noise, on the fast and on the exact side: each within 2^-24 of a value no larger than rabs + m
    const float slack = (rabs + m + 1.0f) * 9.5367431640625e-07f;          // 2^-20
    const float margin = 2.0f * (m + kGumbelScreenMargin + slack);
    const bool all = bad || !(margin < inf);
    const float thr = rmx - margin;
    const int need = (a.H + 63) / 64;                                      // terms per lane of the chain

    auto resolve = [&](int n) {
        if (need <= 4) resolve_listed<4>(a, hs, list, n, wave, lane, vid, sid, &best);
        else if (need <= 8) resolve_listed<8>(a, hs, list, n, wave, lane, vid, sid, &best);
        else if (need <= 16) resolve_listed<16>(a, hs, list, n, wave, lane, vid, sid, &best);
        else resolve_listed<32>(a, hs, list, n, wave, lane, vid, sid, &best);
    };
    // f(column) for every survivor among this thread's four columns of chunk c (its own keys of pass 1).  REG: from the registers -- where
    // c is not a constant (the overflow path), a select over the statically indexed array
    auto survivors4 = [&](int c, auto&& f) {
        const int c0 = tid * 4 + c * kResChunk;
        float ka[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (REG) {
#pragma unroll
            for (int cc = 0; cc < kResRegChunks; ++cc)
                if (cc == c) { ka[0] = kr[cc][0]; ka[1] = kr[cc][1]; ka[2] = kr[cc][2]; ka[3] = kr[cc][3]; }
        } else if (c0 + 4 <= a.V) {
            const float4 x = *reinterpret_cast<const float4*>(Lr + c0);
            ka[0] = x.x; ka[1] = x.y; ka[2] = x.z; ka[3] = x.w;
        } else {
            for (int j = 0; c0 + j < a.V; ++j) ka[j] = Lr[c0 + j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c0 + j < a.V && (all || ka[j] >= thr)) f(c0 + j);
    };
    // the same over every chunk in which this thread has a column, in ascending order
    auto survivors = [&](auto&& f) {
        if constexpr (REG) {
#pragma unroll
            for (int c = 0; c < kResRegChunks; ++c)
                if (tid * 4 + c * kResChunk < a.V) survivors4(c, f);
        } else {
            for (int c = 0; tid * 4 + c * kResChunk < a.V; ++c) survivors4(c, f);
        }
    };
    int cnt = 0;
    survivors([&](int) { ++cnt; });
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) nwave[wave] = cnt;
    __syncthreads();
    unsigned total = 0;
#pragma unroll
    for (int w = 0; w < kResWaves; ++w) total += (unsigned)nwave[w];
    if (total <= (unsigned)kResList) {
        // the usual row: one list, one round
        survivors([&](int c) { list[atomicAdd(&nlist, 1)] = c; });
        __syncthreads();
        resolve((int)total);
        __syncthreads();
    } else {
        // more survivors than the list holds: chunk by chunk, resolving whenever the next chunk might not fit behind what is listed
        for (int base = 0; base < a.V; base += kResChunk) {
            if (base + tid * 4 < a.V) survivors4(base / kResChunk, [&](int c) { list[atomicAdd(&nlist, 1)] = c; });
            __syncthreads();
            const int n = nlist;
            __syncthreads();                                               // (everyone has read the count before the next chunk adds to it)
            if (n <= kResList - kResChunk && base + kResChunk < a.V) continue;
            resolve(n);
            __syncthreads();
            if (tid == 0) nlist = 0;
            __syncthreads();
        }
    }
    if (tid == 0) {
        if (best != 0ull) atomicMax(&a.pick[(size_t)row * a.pick_stride], best);
        uint32_t* const c32 = reinterpret_cast<uint32_t*>(a.counters + 1);
        atomicAdd(a.counters, (unsigned long long)total);
        atomicMax(c32, total);
        if (all) atomicAdd(c32 + 1, 1u);
    }
}

}  // namespace

int pick_screen_products()
{
    static const int n = [] {
        const char* const p = getenv("S2VT_PICK_PRODUCTS");
        const char* const t = getenv("S2VT_PICK_TILE");
        return (p && p[0] == '3' && !p[1]) || (t && (t[0] == '0' || t[0] == '1') && !t[1]) ? 3 : 1;
    }();
    return n;
}

hipError_t launch_pick_screen_prepare(const float* W, int H, int V, const PickScreenWs& s, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(s.counters, 0, kPickScreenHeadBytes, st);
    if (e != hipSuccess) return e;
    // B operand of the NT product: the hi / lo planes of W^T, [V][bf16_pad(H)], zeros past H (one product: the hi plane alone)
    CastTrArgs c{W, V, nullptr, H, V, s.Wh, s.Hp, s.Hp, nullptr, nullptr, nullptr, 0, pick_screen_products() == 1 ? nullptr : s.Wl, nullptr};
    e = launch_cast_tr_bf16(c, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pick_screen_prepare_kernel, dim3((V + 63) / 64), dim3(256), 0, st, W, V, H, V, s.Wt, s.ldt, reinterpret_cast<uint32_t*>(s.nwmax));
    return hipGetLastError();
}

hipError_t launch_pick_screen_step(const float* h, int ldh, const float* W, const float* bias, int R, int H, int V, const int32_t* vid,
                                   const int32_t* sid, uint64_t seed, int step, unsigned long long* pick, int pick_stride, const PickScreenWs& s,
                                   hipStream_t st)
{
    if (R <= 0) return hipSuccess;
    if (H > kPickScreenMaxH) return hipErrorInvalidValue;
    const bool one = pick_screen_products() == 1;
    hipError_t e = launch_cast_rows_bf16(h, ldh, nullptr, R, H, s.hh, s.Hp, st, one ? nullptr : s.hl);
    if (e != hipSuccess) return e;
    e = one ? launch_gemm_bf16x1_nt(s.hh, s.Hp, s.Wh, s.Hp, s.L, s.ldl, R, V, s.Hp, 0, 2, st)
            : launch_gemm_bf16x3_nt(s.hh, s.hl, s.Hp, s.Wh, s.Wl, s.Hp, s.L, s.ldl, R, V, s.Hp, 0, nullptr, 0, 2, st, gemm_bf16x3_pick_tile(R, V));
    if (e != hipSuccess) return e;
    PickResolveArgs a;
    a.L = s.L; a.ldl = s.ldl; a.bias = bias; a.h = h; a.ldh = ldh; a.Wt = s.Wt; a.ldt = s.ldt; a.vid = vid; a.sid = sid;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.step = step;
    a.pick = pick; a.pick_stride = pick_stride > 0 ? pick_stride : 1;
    a.nwmax = s.nwmax; a.counters = s.counters; a.H = H; a.V = V;
    a.C = (one ? kPickAcc1 : kPickC3) * (float)((H + 1023) / 1024);        // per 1024 reduction steps
    a.one = one ? 1 : 0;
    if (V <= kResRegChunks * kResChunk) hipLaunchKernelGGL(pick_resolve_kernel<true>, dim3((unsigned)R), dim3(kResThreads), 0, st, a);
    else hipLaunchKernelGGL(pick_resolve_kernel<false>, dim3((unsigned)R), dim3(kResThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace s2vt
