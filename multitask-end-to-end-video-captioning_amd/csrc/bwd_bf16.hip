// bwd_bf16.hip -- the opt-in bf16 mode of the S2VT backward's gradient contractions (s2vt_bptt_bwd_bf16):
// fp32 -> bf16 casts (a row form, and a transpose form through LDS that can also write the row form and add the fp32 column
// sums of its input) and gemm_bf16_nt, C[M,N] (+)= A[M,Kp] B[N,Kp]^T on bf16 MFMA with fp32 accumulation.  Gradients only:
// nothing here decides a token.  No atomics anywhere: two runs give the same bits.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "internal.h"

namespace s2vt {
namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// RNE, NaN kept (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t pack2(float a, float b)
{
    const f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

// ---------------------------------------------------------------------------------------------
// row form: dst[r][k] = bf16(src[row(r)][k]) for k < K, 0 for K <= k < bf16_pad(K).  One 16-byte store per 8 elements.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cast_rows_bf16_kernel(const float* __restrict__ src, int ld, const int32_t* __restrict__ rowidx,
                                                             int R, int K, uint16_t* __restrict__ dst, int ldd, int vec)
{
    const int cpr = bf16_pad(K) / 8;
    const long total = (long)R * cpr;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int r = (int)(i / cpr), k0 = (int)(i % cpr) * 8;
        const float* s = src + (size_t)(rowidx ? rowidx[r] : r) * ld + k0;
        float v[8];
        if (vec && k0 + 8 <= K) {
            const float4 a = *reinterpret_cast<const float4*>(s), b = *reinterpret_cast<const float4*>(s + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = k0 + j < K ? s[j] : 0.0f;
        }
        uint4 o;
        o.x = pack2(v[0], v[1]); o.y = pack2(v[2], v[3]); o.z = pack2(v[4], v[5]); o.w = pack2(v[6], v[7]);
        *reinterpret_cast<uint4*>(dst + (size_t)r * ldd + k0) = o;
    }
}

// ---------------------------------------------------------------------------------------------
// transpose form: workgroup = 64 columns x kTrRows rows, 64 x 64 tiles through LDS.  dst[c][r] = bf16(src[row(r)][c]) for
// r < R, 0 for R <= r < Rp; optional row-form copy rdst[r][c] (c < bf16_pad(C), zeros past C); optional column sums of the
// fp32 input: part[blockIdx.y][c], summed in a fixed order by colsum_parts_kernel.
// ---------------------------------------------------------------------------------------------
constexpr int kTrRows = 256;

__global__ __launch_bounds__(256) void cast_tr_bf16_kernel(CastTrArgs a, int vec)
{
    __shared__ float t[64][65];
    __shared__ float cs[4][64];
    const int tid = threadIdx.x, c0 = blockIdx.x * 64;
    const int rbeg = blockIdx.y * kTrRows, rend = min(rbeg + kTrRows, a.Rp);
    float csum = 0.0f;
    for (int r0 = rbeg; r0 < rend; r0 += 64) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int rr = p * 16 + (tid >> 4), cc = (tid & 15) * 4;
            const int r = r0 + rr, c = c0 + cc;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (r < a.R) {
                const float* s = a.src + (size_t)(a.rowidx ? a.rowidx[r] : r) * a.ld + c;
                if (vec && c + 4 <= a.C) {
                    const float4 x = *reinterpret_cast<const float4*>(s);
                    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = c + j < a.C ? s[j] : 0.0f;
                }
                if (a.rdst) {
                    uint2 o;
                    o.x = pack2(v[0], v[1]); o.y = pack2(v[2], v[3]);
                    *reinterpret_cast<uint2*>(a.rdst + (size_t)r * a.rldd + c) = o;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) t[rr][cc + j] = v[j];
        }
        __syncthreads();
        for (int i = tid >> 6; i < 64; i += 4) csum += t[i][tid & 63];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int cc = p * 32 + (tid >> 3), rr = (tid & 7) * 8;
            if (c0 + cc < a.C) {
                uint4 o;
                o.x = pack2(t[rr][cc], t[rr + 1][cc]); o.y = pack2(t[rr + 2][cc], t[rr + 3][cc]);
                o.z = pack2(t[rr + 4][cc], t[rr + 5][cc]); o.w = pack2(t[rr + 6][cc], t[rr + 7][cc]);
                *reinterpret_cast<uint4*>(a.dst + (size_t)(c0 + cc) * a.ldd + r0 + rr) = o;
            }
        }
        __syncthreads();
    }
    if (a.colsum) {
        cs[tid >> 6][tid & 63] = csum;
        __syncthreads();
        if (tid < 64 && c0 + tid < a.C) a.part[(size_t)blockIdx.y * a.C + c0 + tid] = (cs[0][tid] + cs[1][tid]) + (cs[2][tid] + cs[3][tid]);
    }
}

__global__ __launch_bounds__(256) void colsum_parts_kernel(const float* __restrict__ part, int nparts, int C, float* __restrict__ colsum)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float s = 0.0f;
    for (int p = 0; p < nparts; ++p) s += part[(size_t)p * C + c];
    colsum[c] += s;
}

// ---------------------------------------------------------------------------------------------
// gemm_bf16_nt: 128 x 128 output tile per 256-thread workgroup, 2 x 2 waves of 64 x 64, K step 64.  Operands global ->
// registers -> LDS (two buffers, one barrier per K step: the next step's loads are in flight during this step's MFMAs);
// rows of 64 bf16 with their 16-byte groups XOR-swizzled by (row >> 1) & 7 (a fragment read of 16 rows hits distinct
// banks).  MF = 16: v_mfma_f32_16x16x32_bf16 (4 x 4 per wave), 32: v_mfma_f32_32x32x16_bf16 (2 x 2 per wave).
// ---------------------------------------------------------------------------------------------
struct GemmBf16Args {
    const uint16_t* A; int lda; const uint16_t* B; int ldb; float* C; int ldc;
    int M, N, Kp, accumulate, tiles_m, tiles_n;
};

constexpr int kTile = 128, kBK = 64, kTileElems = kTile * kBK;

__device__ __forceinline__ int swz(int r, int ch) { return r * kBK + ((ch ^ ((r >> 1) & 7)) << 3); }

template <int MF>
__global__ __launch_bounds__(256) void gemm_bf16_nt_kernel(GemmBf16Args g)
{
    __shared__ __attribute__((aligned(16))) uint16_t lds[2][2][kTileElems];     // [buffer][A | B]
    // XCD-aware order (bijective remap): consecutive tiles of one XCD share their B rows (tm fastest)
    const int nwg = g.tiles_m * g.tiles_n, orig = blockIdx.x;
    const int xcd = orig & 7, q = nwg >> 3, rem = nwg & 7;
    const int wgid = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (orig >> 3);
    const int tm = wgid % g.tiles_m, tn = wgid / g.tiles_m;
    const int m0 = tm * kTile, n0 = tn * kTile;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;

    uint4 ra[4], rb[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int idx = p * 256 + tid, r = idx >> 3, ch = idx & 7;
            const int gm = m0 + r, gn = n0 + r;
            ra[p] = gm < g.M ? *reinterpret_cast<const uint4*>(g.A + (size_t)gm * g.lda + k0 + ch * 8) : make_uint4(0, 0, 0, 0);
            rb[p] = gn < g.N ? *reinterpret_cast<const uint4*>(g.B + (size_t)gn * g.ldb + k0 + ch * 8) : make_uint4(0, 0, 0, 0);
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int idx = p * 256 + tid, r = idx >> 3, ch = idx & 7;
            *reinterpret_cast<uint4*>(&lds[buf][0][swz(r, ch)]) = ra[p];
            *reinterpret_cast<uint4*>(&lds[buf][1][swz(r, ch)]) = rb[p];
        }
    };

    constexpr int RM = MF == 16 ? 4 : 2;                  // fragment repeats per wave in M and in N
    typedef typename std::conditional<MF == 16, f32x4, f32x16>::type acc_t;
    constexpr int NACC = MF == 16 ? 4 : 16;
    acc_t acc[RM][RM];
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RM; ++j)
#pragma unroll
            for (int e = 0; e < NACC; ++e) acc[i][j][e] = 0.0f;

    const int nk = g.Kp / kBK;
    if (nk > 0) { load(0); store(0); }
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) load((kt + 1) * kBK);
        const uint16_t* As = lds[cur][0];
        const uint16_t* Bs = lds[cur][1];
        if constexpr (MF == 16) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int ch = kk * 4 + (lane >> 4);
                bf16x8 af[4], bfr[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int ra_ = wr * 64 + i * 16 + (lane & 15), rb_ = wc * 64 + i * 16 + (lane & 15);
                    af[i] = *reinterpret_cast<const bf16x8*>(As + swz(ra_, ch));
                    bfr[i] = *reinterpret_cast<const bf16x8*>(Bs + swz(rb_, ch));
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int ch = kk * 2 + (lane >> 5);
                bf16x8 af[2], bfr[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int ra_ = wr * 64 + i * 32 + (lane & 31), rb_ = wc * 64 + i * 32 + (lane & 31);
                    af[i] = *reinterpret_cast<const bf16x8*>(As + swz(ra_, ch));
                    bfr[i] = *reinterpret_cast<const bf16x8*>(Bs + swz(rb_, ch));
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
            }
        }
        if (kt + 1 < nk) store(cur ^ 1);
        __syncthreads();
    }
    // epilogue: C/D maps of the two shapes (cdna guide §3)
#pragma unroll
    for (int i = 0; i < RM; ++i)
#pragma unroll
        for (int j = 0; j < RM; ++j)
#pragma unroll
            for (int e = 0; e < NACC; ++e) {
                int row, col;
                if constexpr (MF == 16) {
                    row = m0 + wr * 64 + i * 16 + (lane >> 4) * 4 + e;
                    col = n0 + wc * 64 + j * 16 + (lane & 15);
                } else {
                    row = m0 + wr * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                    col = n0 + wc * 64 + j * 32 + (lane & 31);
                }
                if (row < g.M && col < g.N) {
                    float* c = g.C + (size_t)row * g.ldc + col;
                    *c = g.accumulate ? *c + acc[i][j][e] : acc[i][j][e];
                }
            }
}

}  // namespace

hipError_t launch_cast_rows_bf16(const float* src, int ld, const int32_t* rowidx, int R, int K, uint16_t* dst, int ldd, hipStream_t st)
{
    if (R <= 0 || K <= 0) return hipSuccess;
    const int vec = !((reinterpret_cast<uintptr_t>(src) & 15) || (ld & 3));
    const long chunks = (long)R * (bf16_pad(K) / 8);
    const long blocks = (chunks + 255) / 256;
    hipLaunchKernelGGL(cast_rows_bf16_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, src, ld, rowidx, R, K, dst, ldd, vec);
    return hipGetLastError();
}

size_t cast_tr_part_floats(int Rp, int C)
{
    return (size_t)((Rp + kTrRows - 1) / kTrRows) * (size_t)C;
}

hipError_t launch_cast_tr_bf16(const CastTrArgs& a, hipStream_t st)
{
    if (a.C <= 0 || a.Rp <= 0) return hipSuccess;
    const int vec = !((reinterpret_cast<uintptr_t>(a.src) & 15) || (a.ld & 3));
    const int ny = (a.Rp + kTrRows - 1) / kTrRows;
    hipLaunchKernelGGL(cast_tr_bf16_kernel, dim3((a.C + 63) / 64, ny), dim3(256), 0, st, a, vec);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !a.colsum) return e;
    hipLaunchKernelGGL(colsum_parts_kernel, dim3((a.C + 255) / 256), dim3(256), 0, st, (const float*)a.part, ny, a.C, a.colsum);
    return hipGetLastError();
}

int gemm_bf16_default_mfma()
{
    static const int v = [] { const char* e = getenv("S2VT_BF16_MFMA"); const int x = e ? atoi(e) : 16; return x == 32 ? 32 : 16; }();   // dev knob
    return v;
}

hipError_t launch_gemm_bf16_nt(const uint16_t* A, int lda, const uint16_t* B, int ldb, float* C, int ldc, int M, int N, int Kp, int accumulate,
                               int mfma, hipStream_t st)
{
    if (M <= 0 || N <= 0) return hipSuccess;
    GemmBf16Args g;
    g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.Kp = Kp; g.accumulate = accumulate;
    g.tiles_m = (M + kTile - 1) / kTile; g.tiles_n = (N + kTile - 1) / kTile;
    const dim3 grid((unsigned)(g.tiles_m * g.tiles_n));
    if ((mfma ? mfma : gemm_bf16_default_mfma()) == 32) hipLaunchKernelGGL(gemm_bf16_nt_kernel<32>, grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL(gemm_bf16_nt_kernel<16>, grid, dim3(256), 0, st, g);
    return hipGetLastError();
}

}  // namespace s2vt
