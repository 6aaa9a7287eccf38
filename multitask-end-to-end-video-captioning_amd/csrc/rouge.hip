// rouge.hip -- ROUGE-L of sampled token-id rows against their video's references, on the device (include/s2vt.h, s2vt_rouge_l_score;
// the arithmetic contract: DESIGN.md §3).  One wavefront per row; one launch, no workspace, no atomics.
//
//   * The row's candidate (the ids before its first <eos>, m <= 128 of them) is staged once in LDS; every lane reads it at the same
//     address (a broadcast, no bank conflicts).
//   * Lanes stride over the video's references (a video with more than 64 takes a second pass).  A lane computes LCS(candidate, its
//     reference) bit-parallel (Allison & Dix 1986 / Hyyro 2004): a 128-bit vector V over the candidate's positions, all ones at the
//     start; per reference token y with match mask M (bit i set where candidate[i] == y)
//         V = (V + (V & M)) | (V & ~M)
//     and LCS = the number of ZERO bits among V's low m bits.  Integer, exact: the same l_j as the classic table of csrc_host/rouge.cpp
//     and of the tests' restatement -- three derivations of one number.  No per-lane table in LDS, no runtime-indexed registers.
//   * One wave max of the integers l_j (p = max l / m: one division, the same double the per-reference maximum of l_j / m is, since
//     x -> x / m is monotone and correctly rounded) and one of the doubles l_j / len r_j, then lane 0 evaluates the F-measure in IEEE
//     double, one operation at a time (-ffp-contract=off for the whole library, and the pragma below).
#include "api_util.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int kRougeMaxTc = 128;
constexpr int kRowsPerBlock = 4;          // one wave each

struct RougeArgs {
    const int32_t* tokens;
    const int32_t* ref_offsets;
    const int32_t* video_refs;
    int32_t n_videos;
    const int32_t* ids;
    int32_t ld, N, Tc, eos_id;
    const int32_t* video_of_row;
    double beta2;
    float* out;
    double* pr_out;
};

__device__ inline int wave_max_i(int v)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ inline double wave_max_d(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(64 * kRowsPerBlock) void rouge_l_kernel(RougeArgs a)
{
    __shared__ int32_t cand_s[kRowsPerBlock][kRougeMaxTc];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * kRowsPerBlock + wave;
    const bool have = row < a.N;                                    // wave-uniform
    int32_t* cand = cand_s[wave];
    int m = 0, v = -1;
    if (have) {
        const int32_t* w = a.ids + (size_t)row * a.ld;
        // the ids before the first <eos>: two ballots cover Tc <= 128
        const int32_t x0 = lane < a.Tc ? w[lane] : a.eos_id;
        const int32_t x1 = lane + 64 < a.Tc ? w[lane + 64] : a.eos_id;
        const unsigned long long e0 = __ballot(x0 == a.eos_id), e1 = __ballot(x1 == a.eos_id);
        m = e0 ? __ffsll((long long)e0) - 1 : (e1 ? 64 + __ffsll((long long)e1) - 1 : kRougeMaxTc);
        if (m > a.Tc) m = a.Tc;
        cand[lane] = x0;
        cand[lane + 64] = x1;
        v = a.video_of_row[row];
    }
    __syncthreads();                                                // every wave of the block arrives: nothing returns before it
    if (!have) return;
    if (v < 0 || v >= a.n_videos) {                                 // device data the host could not check: loud, never a clamped reward
        if (lane == 0) {
            a.out[row] = nanf("");
            if (a.pr_out) { a.pr_out[2 * (size_t)row] = nan(""); a.pr_out[2 * (size_t)row + 1] = nan(""); }
        }
        return;
    }
    const int r0 = a.video_refs[v], r1 = a.video_refs[v + 1];
    int best_l = 0;
    double best_r = 0.0;
    for (int base = r0; base < r1; base += 64) {                    // wave-uniform trip count
        const int j = base + lane;
        int t0 = 0, len = 0;
        if (j < r1) { t0 = a.ref_offsets[j]; len = a.ref_offsets[j + 1] - t0; }
        const int maxlen = wave_max_i(len);
        unsigned long long vlo = ~0ull, vhi = ~0ull;
        for (int t = 0; t < maxlen; ++t) {
            const bool on = t < len;
            const int32_t y = on ? a.tokens[t0 + t] : 0;
            unsigned long long mlo = 0, mhi = 0;
            for (int i = 0; i < m && i < 64; ++i) mlo |= (unsigned long long)(cand[i] == y) << i;
            for (int i = 64; i < m; ++i) mhi |= (unsigned long long)(cand[i] == y) << (i - 64);
            if (on) {
                const unsigned long long ulo = vlo & mlo, uhi = vhi & mhi;
                const unsigned long long slo = vlo + ulo;
                const unsigned long long shi = vhi + uhi + (slo < vlo ? 1ull : 0ull);
                vlo = slo | (vlo & ~mlo);
                vhi = shi | (vhi & ~mhi);
            }
        }
        const unsigned long long klo = m >= 64 ? ~0ull : ((1ull << m) - 1ull);
        const unsigned long long khi = m >= 128 ? ~0ull : (m > 64 ? ((1ull << (m - 64)) - 1ull) : 0ull);
        const int l = __popcll(~vlo & klo) + __popcll(~vhi & khi);
        if (j < r1) {
            best_l = max(best_l, l);
            if (len > 0) best_r = fmax(best_r, (double)l / (double)len);
        }
    }
    best_l = wave_max_i(best_l);
    best_r = wave_max_d(best_r);
    if (lane == 0) {
        const double p = m > 0 ? (double)best_l / (double)m : 0.0;
        const double r = best_r;
        double score = 0.0;
        if (!(p == 0.0 || r == 0.0)) {
            const double num = ((1.0 + a.beta2) * p) * r;
            const double den = r + a.beta2 * p;
            score = num / den;
        }
        a.out[row] = (float)score;
        if (a.pr_out) { a.pr_out[2 * (size_t)row] = p; a.pr_out[2 * (size_t)row + 1] = r; }
    }
}

}  // namespace

extern "C" int s2vt_rouge_l_score(const s2vt_rouge_refs* refs, const int32_t* ids, int32_t ld, int32_t N, int32_t Tc, int32_t eos_id,
                                  const int32_t* video_of_row, double beta2, float* out, double* pr_out, s2vt_stream stream)
{
    using namespace s2vt_api;
    if (!refs || !refs->tokens || !refs->ref_offsets || !refs->video_refs || !ids || !video_of_row || !out) return S2VT_E_BADARG;
    if (Tc < 1 || Tc > kRougeMaxTc || ld < Tc || N < 0 || refs->n_videos < 1 || refs->n_refs < 0) return S2VT_E_BADARG;
    if (!std::isfinite(beta2) || beta2 < 0.0) return S2VT_E_BADARG;
    if (N == 0) return S2VT_OK;
    RougeArgs a{refs->tokens, refs->ref_offsets, refs->video_refs, refs->n_videos, ids, ld, N, Tc, eos_id, video_of_row, beta2, out, pr_out};
    hipLaunchKernelGGL(rouge_l_kernel, dim3((N + kRowsPerBlock - 1) / kRowsPerBlock), dim3(64 * kRowsPerBlock), 0, S(stream), a);
    HIP_TRY(hipGetLastError());
    return S2VT_OK;
}
