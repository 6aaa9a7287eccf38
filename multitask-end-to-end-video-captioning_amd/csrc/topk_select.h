// topk_select.h -- the total order of a vocabulary top-k and the per-thread candidate list that keeps it, shared by vocab_topk_kernel
// (beam.hip) and topk_mix_fwd_kernel (topk_feed.hip): value descending, then index ascending on exact ties -- deterministic, and the
// order tf.nn.top_k returns.  A NaN never compares better, so it never enters a list.
#pragma once
#include <hip/hip_runtime.h>

namespace s2vt {

__device__ __forceinline__ bool tk_better(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

// insert (v, i) into a list of KMAX (value, index) pairs kept sorted best first; the list's empty slots hold (-inf, INT_MAX)
template <int KMAX>
__device__ __forceinline__ void tk_insert(float (&tv)[KMAX], int (&ti)[KMAX], float v, int i)
{
    if (!tk_better(v, i, tv[KMAX - 1], ti[KMAX - 1])) return;
    tv[KMAX - 1] = v; ti[KMAX - 1] = i;
#pragma unroll
    for (int j = KMAX - 1; j > 0; --j) {
        if (tk_better(tv[j], ti[j], tv[j - 1], ti[j - 1])) {
            const float fv = tv[j]; tv[j] = tv[j - 1]; tv[j - 1] = fv;
            const int fi = ti[j]; ti[j] = ti[j - 1]; ti[j - 1] = fi;
        }
    }
}

}  // namespace s2vt
