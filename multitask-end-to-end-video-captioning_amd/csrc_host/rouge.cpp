// rouge.cpp -- ROUGE-L reward on integer token ids (include/s2vt_host.h).  Host code, OpenMP over rows.  The classic LCS table and the
// F-measure of DESIGN.md §3 in IEEE double, one operation at a time (built with -ffp-contract=off): bit-equal to the device kernel
// (csrc/rouge.hip), which finds the same integers by another route.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "../../include/s2vt_host.h"

struct s2vt_rouge {
    int32_t n_videos;
    std::vector<int32_t> tokens;            // every reference's ids, the references grouped by video
    std::vector<int64_t> ref_off;           // [n_refs + 1] into tokens
    std::vector<int32_t> video_refs;        // [n_videos + 1] into ref_off
    int64_t max_len;
};

extern "C" {

s2vt_rouge* s2vt_rouge_create(const int32_t* tokens, const int64_t* offsets, const int32_t* video_of_ref, int32_t n_refs, int32_t n_videos)
{
    if (!tokens || !offsets || !video_of_ref || n_refs <= 0 || n_videos <= 0) return nullptr;
    for (int r = 0; r < n_refs; ++r)
        if (video_of_ref[r] < 0 || video_of_ref[r] >= n_videos || offsets[r + 1] < offsets[r]) return nullptr;
    s2vt_rouge* h = new (std::nothrow) s2vt_rouge;
    if (!h) return nullptr;
    h->n_videos = n_videos;
    h->max_len = 0;
    h->video_refs.assign((size_t)n_videos + 1, 0);
    for (int r = 0; r < n_refs; ++r) h->video_refs[(size_t)video_of_ref[r] + 1] += 1;
    for (int v = 0; v < n_videos; ++v) h->video_refs[(size_t)v + 1] += h->video_refs[v];
    // a stable counting sort of the references by video (the caller's order inside a video is kept)
    std::vector<int32_t> slot(h->video_refs.begin(), h->video_refs.end() - 1), order((size_t)n_refs);
    for (int r = 0; r < n_refs; ++r) order[(size_t)slot[video_of_ref[r]]++] = r;
    h->ref_off.assign(1, 0);
    h->tokens.reserve((size_t)(offsets[n_refs] - offsets[0]));
    for (int q = 0; q < n_refs; ++q) {
        const int r = order[q];
        h->tokens.insert(h->tokens.end(), tokens + offsets[r], tokens + offsets[r + 1]);
        h->ref_off.push_back((int64_t)h->tokens.size());
        h->max_len = std::max(h->max_len, offsets[r + 1] - offsets[r]);
    }
    return h;
}

void s2vt_rouge_destroy(s2vt_rouge* h) { delete h; }

int s2vt_rouge_score(const s2vt_rouge* h, const int32_t* ids, int32_t N, int32_t Tc, int32_t eos_id, const int32_t* video_of_row,
                     double beta2, float* out, int32_t n_threads)
{
    if (!h || !ids || !video_of_row || !out || N < 0 || Tc <= 0 || !std::isfinite(beta2) || beta2 < 0.0) return -1;
    for (int n = 0; n < N; ++n)
        if (video_of_row[n] < 0 || video_of_row[n] >= h->n_videos) return -1;
#ifdef _OPENMP
    const int nt = n_threads > 1 ? n_threads : 1;
#pragma omp parallel num_threads(nt) if (nt > 1)
#endif
    {
        std::vector<int32_t> table((size_t)(h->max_len + 1) * 2);          // two rows of the LCS table, per thread, once per call
#ifdef _OPENMP
#pragma omp for schedule(static)
#endif
        for (int n = 0; n < N; ++n) {
            const int32_t* c = ids + (size_t)n * Tc;
            int m = 0;
            while (m < Tc && c[m] != eos_id) ++m;                           // words before the first <eos>
            const int32_t v = video_of_row[n];
            double p = 0.0, r = 0.0;
            for (int32_t j = h->video_refs[v]; j < h->video_refs[(size_t)v + 1]; ++j) {
                const int32_t* y = h->tokens.data() + h->ref_off[j];
                const int64_t len = h->ref_off[(size_t)j + 1] - h->ref_off[j];
                int32_t* prev = table.data();
                int32_t* cur = prev + (h->max_len + 1);
                std::fill(prev, prev + len + 1, 0);
                for (int i = 0; i < m; ++i) {                               // rows: candidate words; columns: reference words
                    cur[0] = 0;
                    for (int64_t k = 0; k < len; ++k)
                        cur[k + 1] = c[i] == y[k] ? prev[k] + 1 : std::max(prev[k + 1], cur[k]);
                    std::swap(prev, cur);
                }
                const int32_t l = prev[len];
                if (m > 0) p = std::max(p, (double)l / (double)m);
                if (len > 0) r = std::max(r, (double)l / (double)len);
            }
            double score = 0.0;
            if (!(p == 0.0 || r == 0.0)) {
                const double num = ((1.0 + beta2) * p) * r;
                const double den = r + beta2 * p;
                score = num / den;
            }
            out[n] = (float)score;
        }
    }
    return 0;
}

}  // extern "C"
