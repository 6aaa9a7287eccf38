// bwd_bf16.hip -- the bf16 MFMA forms of the S2VT backward's gradient contractions:
// fp32 -> bf16 casts (a row form, and a transpose form through LDS that can also write the row form and add the fp32 column
// sums of its input) and gemm_bf16_nt, C[M,N] (+)= A[M,Kp] B[N,Kp]^T on bf16 MFMA with fp32 accumulation -- the opt-in bf16
// mode (s2vt_bptt_bwd_bf16); the split forms of the same casts (hi = bf16(x), lo = bf16(x - hi), one read of x) and
// gemm_bf16x3_nt, C (+)= Ah Bh^T + Ah Bl^T + Al Bh^T -- the default fp32 mode's split-bf16 products (s2vt_bptt_bwd_split).
// Gradients only: nothing here decides a token.  No atomics anywhere: two runs give the same bits.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "internal.h"

namespace s2vt {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------
// row form: dst[r][k] = bf16(src[row(r)][k]) for k < K, 0 for K <= k < bf16_pad(K).  One 16-byte store per 8 elements.
// SPLIT: dst the hi plane, dst_lo the lo plane (same ldd).  ones: the row is bf16_pad(K + 1) wide and column K holds 1 (hi 1, lo 0) -- as
// the K-major operand A of gemm_bf16x3_tn it makes output row K the column sums of B (a bias gradient riding in the product).
// width (a multiple of 8): the columns written per row, bf16_pad(K + ones) unless the caller places the row inside a wider one.
// ---------------------------------------------------------------------------------------------
template <bool SPLIT>
__global__ __launch_bounds__(256) void cast_rows_bf16_kernel(const float* __restrict__ src, int ld, const int32_t* __restrict__ rowidx,
                                                             int R, int K, uint16_t* __restrict__ dst, int ldd, int vec,
                                                             uint16_t* __restrict__ dst_lo, int ones, int width)
{
    const int cpr = width / 8;
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
            for (int j = 0; j < 8; ++j) v[j] = k0 + j < K ? s[j] : ones && k0 + j == K ? 1.0f : 0.0f;
        }
        uint4 o;
        if constexpr (SPLIT) {
            uint4 l;
            split2(v[0], v[1], o.x, l.x); split2(v[2], v[3], o.y, l.y); split2(v[4], v[5], o.z, l.z); split2(v[6], v[7], o.w, l.w);
            *reinterpret_cast<uint4*>(dst_lo + (size_t)r * ldd + k0) = l;
        } else {
            o.x = pack2(v[0], v[1]); o.y = pack2(v[2], v[3]); o.z = pack2(v[4], v[5]); o.w = pack2(v[6], v[7]);
        }
        *reinterpret_cast<uint4*>(dst + (size_t)r * ldd + k0) = o;
    }
}

// ---------------------------------------------------------------------------------------------
// transpose form: workgroup = 64 columns x kTrRows rows, 64 x 64 tiles through LDS.  dst[c][r] = bf16(src[row(r)][c]) for
// r < R, 0 for R <= r < Rp; optional row-form copy rdst[r][c] (c < bf16_pad(C), zeros past C); optional column sums of the
// fp32 input: part[blockIdx.y][c], summed in a fixed order by colsum_parts_kernel.  SPLIT: dst / rdst the hi planes, dst_lo /
// rdst_lo the lo planes.
// ---------------------------------------------------------------------------------------------
constexpr int kTrRows = 256;

template <bool SPLIT>
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
                    if constexpr (SPLIT) {
                        uint2 l;
                        split2(v[0], v[1], o.x, l.x); split2(v[2], v[3], o.y, l.y);
                        *reinterpret_cast<uint2*>(a.rdst_lo + (size_t)r * a.rldd + c) = l;
                    } else {
                        o.x = pack2(v[0], v[1]); o.y = pack2(v[2], v[3]);
                    }
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
                if constexpr (SPLIT) {
                    uint4 l;
                    split2(t[rr][cc], t[rr + 1][cc], o.x, l.x); split2(t[rr + 2][cc], t[rr + 3][cc], o.y, l.y);
                    split2(t[rr + 4][cc], t[rr + 5][cc], o.z, l.z); split2(t[rr + 6][cc], t[rr + 7][cc], o.w, l.w);
                    *reinterpret_cast<uint4*>(a.dst_lo + (size_t)(c0 + cc) * a.ldd + r0 + rr) = l;
                } else {
                    o.x = pack2(t[rr][cc], t[rr + 1][cc]); o.y = pack2(t[rr + 2][cc], t[rr + 3][cc]);
                    o.z = pack2(t[rr + 4][cc], t[rr + 5][cc]); o.w = pack2(t[rr + 6][cc], t[rr + 7][cc]);
                }
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


// ---------------------------------------------------------------------------------------------
// gemm_bf16x3_nt: C[M,N] (+)= Ah Bh^T + Ah Bl^T + Al Bh^T over Kp, fp32 accumulation in one accumulator per output element.
// 128 x 128 output tile per 512-thread workgroup: waves 0-3 are MFMA waves (2 x 2 of 64 x 64, v_mfma_f32_16x16x32_bf16, 4 x 4
// per wave), waves 4-7 loader waves -- loader wave p moves plane p (Ah, Al, Bh, Bl) global -> LDS by LDS-DMA
// (buffer_load_dwordx4 ... lds), 8 instructions of 16 rows x 32 k per K step, into a ring of kX3Slots K steps of 32.  Loaders keep
// up to three K steps in flight and publish K step k + 1 at barrier k (counted vmcnt, raw s_barrier); the MFMA waves read K
// step k + 1's fragments while they multiply K step k's, and free K step k's ring slot at barrier k.  LDS images are linear per
// DMA instruction (16 rows x 64 bytes); the 16-byte k groups of a row are XOR-swizzled by (row >> 2) & 3 on the SOURCE address, so a
// fragment read (16 rows, one k group each) covers all 64 banks.  (The LDS serves a ds_read_b128 in four 16-lane groups that mix two k
// groups, and this swizzle is 2-way there: SQ_LDS_BANK_CONFLICT = 4 cycles per read.  The swizzle -(row >> 2) & 3 measured 0 conflicts
// and the same kernel times -- the reads are not what the kernel waits for, profiles/NOTES.md -- so it stays as it was.)  Out-of-range rows load zeros (buffer range check).  Split-K
// (blockIdx.y = slab of nk_slab K steps): slab s writes its partial tile to part + s * M * N, and reduce_slabs_kernel adds the
// slabs in slab order -- deterministic, no atomics.
//
// TN = true, gemm_bf16x3_tn: C[M,N] (+)= sum_k A[k][m] B[k][n], the planes stored by rows of the REDUCTION index ([K][lda], [K][ldb]: a
// weight gradient's operands as they lie in memory, no transposed copies).  Same tile, ring, waits, K steps and MFMA order -- on planes
// that are each other's transposes TN and NT give the same bits.  A plane's K step is the LDS image [32 k][128 m] (256-byte k rows, one
// DMA instruction = 4 k rows); the MFMA waves take a 16x16x32 operand with two transposed reads (ds_read_b64_tr_b16: a 16-lane group
// g reads k rows 8g .. 8g+3, then 8g+4 .. 8g+7, of its 16 columns).  The 32-byte column blocks of k row k are XOR-permuted by
// (k & 3) | ((k >> 1) & 4) on the SOURCE address: the 8 k rows a 32-lane half reads lie in 8 distinct blocks = all 64 banks.  k rows
// past K load zeros (buffer range check: the descriptor ends behind row K - 1); a tile's columns past lda / ldb come from the next
// row and only reach outputs that are not stored.  bias (optional): output row M -- the product of A's column M, which the caller
// filled with ones (cast_rows_bf16 ones) -- is added to bias[n] instead of a C row: the column sums of B.
//
// FORM = kX3NN, gemm_bf16x3_nn: C[M,N] (+)= sum_k A[m][k] B[k][n], a forward product -- A by rows ([M][lda], what cast_rows_bf16 writes) and
// B K-major ([K][ldb], a weight as it lies in memory).  A plane's loader and fragment reads do not depend on the other operand's: loader
// waves 4-5 and the A fragments take the NT code, loader waves 6-7 and the B fragments the TN code (both issue kX3Dma instructions per K
// step, so the counted waits hold).  A's columns in [K, bf16_pad(K)) are read (finite by contract); B's k rows >= K load zeros, so whatever
// A holds there adds exact zeros.  cbias (optional): C = acc + cbias[col], once per stored column -- by the reduce kernel under split-K.
// ---------------------------------------------------------------------------------------------
struct GemmX3Args {
    const uint16_t *Ah, *Al; int lda; const uint16_t *Bh, *Bl; int ldb; float* C; int ldc;
    int M, N, nk, nk_slab, accumulate, tiles_m, tiles_n;
    float* part;                                      // split-K slabs [slabs][Mo][N], or nullptr: the tile goes to C
    int K;                                            // TN: rows of the planes
    float* bias; int Mo;                              // TN: optional [N] += output row M; Mo = M + (bias ? 1 : 0) output rows (NT, NN: Mo = M)
    const float* cbias;                               // NN: optional [N], added once to every stored column (non-accumulating launches)
};

// the three forms: which of the two operands lie K-major ([K][ld], the TN loader and the transposed fragment reads)
enum : int { kX3NT = 0, kX3TN = 1, kX3NN = 2 };
// kX1NT: the one-product NT form, C = Ah Bh^T -- the hi planes alone (Al, Bl are neither loaded nor read), one MFMA pass per K step.  What
// it leaves is bf16 x bf16 in fp32: a screen's product (pick_screen.hip proves the bound), never a gradient's.  192 x 96 tiles only.
enum : int { kX1NT = 3 };

constexpr int kX3BK = 32, kX3Slots = 4, kX3Plane = kTile * kX3BK;   // a plane's K step: 128 rows x 32 bf16 = 8 KB
constexpr int kX3TileM = 192, kX3TileN = 96;                         // the second NT geometry
// LDS of a tile geometry: 4 slots x (2 A planes + 2 B planes) x 64 bytes a row -- 128 KB at 128 x 128, 144 KB at 192 x 96: one workgroup per CU
constexpr int x3_lds_bytes(int tm, int tn) { return kX3Slots * 2 * (tm + tn) * kX3BK * 2; }
constexpr int x1_lds_bytes(int tm, int tn) { return kX3Slots * (tm + tn) * kX3BK * 2; }   // the hi planes alone: 72 KB at 192 x 96
constexpr int kX3Dma = kTile / 16;                                   // DMA instructions per plane per K step (per loader wave)
typedef __attribute__((address_space(3))) void* x3_lds_ptr;
typedef short i16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) i16x4* x3_tr_ptr;

// A loader wave of the NT form on a tile whose planes differ in height: the rows [r0, r0 + 16 ND) of one plane (descriptor rs starts at row
// r0), ND DMA instructions per K step into pdst + slot * slot_elems.  ND is a constant of the plane, so the counted waits are immediates;
// the ring, the waits and the barriers are those of the 128 x 128 loader in the kernel below.  (FORM only names the specialization: the
// one-product kernel takes its own -- the host pass fails to look up a specialization that another kernel instantiation already took.)
template <int ND, int FORM = kX3NT>
__device__ __forceinline__ void x3_nt_loader(__amdgpu_buffer_rsrc_t rs, int r0, int rows, int ld, uint16_t* pdst, int slot_elems, int kbeg, int nk, int lane)
{
    static_assert(3 * ND < 64, "vmcnt is a 6-bit counter");
    uint32_t voff[ND];
    const int rr = lane >> 2, kg = (lane & 3) ^ ((rr >> 2) & 3);
#pragma unroll
    for (int b = 0; b < ND; ++b) {
        const int r = b * 16 + rr;
        voff[b] = r0 + r < rows ? (uint32_t)(r * ld + kg * 8) * 2u : kOob;
    }
    auto issue = [&](int ks) __attribute__((always_inline)) {
        uint16_t* const dst = pdst + (ks % kX3Slots) * slot_elems;
        const uint32_t soff = (uint32_t)(kbeg + ks) * kX3BK * 2u;
#pragma unroll
        for (int b = 0; b < ND; ++b)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (x3_lds_ptr)(dst + b * 16 * kX3BK), 16, voff[b], soff, 0, 0);
    };
    auto wait_younger = [](int n) __attribute__((always_inline)) {
        if (n >= 2) wait_vmcnt<2 * ND>();
        else if (n == 1) wait_vmcnt<ND>();
        else wait_vmcnt<0>();
    };
    const int pro = min(kX3Slots, nk);
    for (int ks = 0; ks < pro; ++ks) issue(ks);
    if (pro - 1 >= 3) wait_vmcnt<3 * ND>();                   // K step 0 has landed
    else wait_younger(pro - 1);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    for (int k = 0; k < nk; ++k) {
        wait_younger(min(k + 3, nk - 1) - (k + 1));           // K step k + 1 has landed
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();                         // barrier k: the MFMA waves are done reading K step k
        asm volatile("" ::: "memory");
        if (k + kX3Slots < nk) issue(k + kX3Slots);           // into K step k's slot
    }
}

// BM x BN: the output tile.  128 x 128 in every form; the NT form also as 192 x 96 (2 x 2 MFMA waves of 96 x 48 = 6 x 3 fragments, 18
// accumulators; A-plane loaders issue 12 DMA instructions per K step, B-plane loaders 6) -- the same ring, waits, K steps and MFMA order,
// one accumulator per output element: the bits do not depend on the tile.  Unsplit launches only (g.part == nullptr).
// kX1NT on that geometry: a slot holds [Ah | Bh]; loader waves 4-5 take the upper and lower 96 rows of Ah (6 DMA instructions per K step
// each), 6-7 the two 48-row halves of Bh (3 each) -- all eight waves exist and meet at the same barriers; 18 MFMAs per K step and wave.
template <int FORM, int BM = kTile, int BN = kTile>
__global__ __launch_bounds__(512) void gemm_bf16x3_kernel(GemmX3Args g)
{
    constexpr bool X1 = FORM == kX1NT;
    static_assert(BM == BN ? BM == kTile && !X1 : (FORM == kX3NT || X1) && BM % 32 == 0 && BN % 32 == 0, "K-major planes come as 128 x 128 tiles only");
    constexpr bool ATN = FORM == kX3TN, BTN = FORM == kX3TN || FORM == kX3NN;   // A's planes / B's planes K-major
    constexpr int WM = BM / 2, WN = BN / 2, FI = WM / 16, FJ = WN / 16; // an MFMA wave's part of the tile, in rows / columns and in fragments
    constexpr int kPlaneA = BM * kX3BK, kPlaneB = BN * kX3BK, kSlot = (X1 ? 1 : 2) * (kPlaneA + kPlaneB);
    extern __shared__ __attribute__((aligned(16))) uint16_t x3lds[];   // [slot][Ah | Al | Bh | Bl][rows][32]
    const int nwg = g.tiles_m * g.tiles_n, orig = blockIdx.x;
    const int xcd = orig & 7, q = nwg >> 3, rem = nwg & 7;
    const int wgid = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (orig >> 3);
    const int tm = wgid % g.tiles_m, tn = wgid / g.tiles_m;
    const int m0 = tm * BM, n0 = tn * BN;
    const int kbeg = blockIdx.y * g.nk_slab, nk = min(g.nk_slab, g.nk - kbeg);
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);

    if constexpr (BM != BN) {
        if (w >= 4) {
            // ================= loader wave of the NT form, plane p: rows / 16 DMA instructions per K step (x3_nt_loader)
            const int p = w - 4;
            if constexpr (X1) {
                // half (p & 1) of the hi plane of A (p < 2) or B; a half that starts past the last row loads nothing but zeros (every offset kOob)
                const int hr = (p < 2 ? BM : BN) / 2 * (p & 1);
                const int r0 = (p < 2 ? m0 : n0) + hr, rows = p < 2 ? g.M : g.N, ld = p < 2 ? g.lda : g.ldb;
                const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>((p < 2 ? g.Ah : g.Bh) + (size_t)min(r0, rows) * ld), 0, (int)kOob, 0x00020000);
                uint16_t* const pdst = x3lds + (p < 2 ? 0 : kPlaneA) + hr * kX3BK;
                if (p < 2) x3_nt_loader<BM / 32, kX1NT>(rs, r0, rows, ld, pdst, kSlot, kbeg, nk, lane);
                else x3_nt_loader<BN / 32, kX1NT>(rs, r0, rows, ld, pdst, kSlot, kbeg, nk, lane);
                return;
            } else {
                const uint16_t* const plane = p == 0 ? g.Ah : p == 1 ? g.Al : p == 2 ? g.Bh : g.Bl;
                const int r0 = p < 2 ? m0 : n0, rows = p < 2 ? g.M : g.N, ld = p < 2 ? g.lda : g.ldb;
                const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(plane + (size_t)r0 * ld), 0, (int)kOob, 0x00020000);
                uint16_t* const pdst = x3lds + (p < 2 ? p * kPlaneA : 2 * kPlaneA + (p - 2) * kPlaneB);
                if (p < 2) x3_nt_loader<BM / 16>(rs, r0, rows, ld, pdst, kSlot, kbeg, nk, lane);
                else x3_nt_loader<BN / 16>(rs, r0, rows, ld, pdst, kSlot, kbeg, nk, lane);
                return;
            }
        }
    } else if (w >= 4) {
        // ================= loader wave: plane p, 8 DMA instructions per K step
        const int p = w - 4;
        // this plane's layout: a constant in the NT and TN forms (the branches below fold), wave-uniform in NN -- A's planes by rows, B's K-major
        const bool TN = ATN == BTN ? ATN : p >= 2;
        const uint16_t* const plane = p == 0 ? g.Ah : p == 1 ? g.Al : p == 2 ? g.Bh : g.Bl;
        const int r0 = p < 2 ? m0 : n0, rows = p < 2 ? g.M : g.N, ld = p < 2 ? g.lda : g.ldb;
        // NT: the descriptor starts at the tile's first row; TN: at its first column, and ends behind k row K - 1
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(plane + (TN ? (size_t)r0 : (size_t)r0 * ld)), 0,
                                                                            TN ? (int)(((uint32_t)g.K * (uint32_t)ld - (uint32_t)r0) * 2u) : (int)kOob, 0x00020000);
        uint32_t voff[kX3Dma];
        if (TN) {
            // lane -> (k row lane >> 4 of a 4-row block, LDS 16-byte slot s = lane & 15): loads the 16-byte piece s & 1 of column block
            // (s >> 1) ^ swz(k), swz(k) = (k & 3) | ((k >> 1) & 4) = kr | ((b & 2) << 1) for k = 4 b + kr
            const int kr = lane >> 4, s = lane & 15;
#pragma unroll
            for (int b = 0; b < kX3Dma; ++b)
                voff[b] = (uint32_t)((b * 4 + kr) * ld + ((((s >> 1) ^ (kr | ((b & 2) << 1))) << 1) | (s & 1)) * 8) * 2u;
        } else {
            // lane -> (row lane >> 2 of a 16-row block, LDS 16-byte slot lane & 3): loads k group (lane & 3) ^ ((row >> 2) & 3)
            const int rr = lane >> 2, kg = (lane & 3) ^ ((rr >> 2) & 3);
#pragma unroll
            for (int b = 0; b < kX3Dma; ++b) {
                const int r = b * 16 + rr;
                voff[b] = r0 + r < rows ? (uint32_t)(r * ld + kg * 8) * 2u : kOob;
            }
        }
        auto issue = [&](int ks) __attribute__((always_inline)) {
            uint16_t* const dst = x3lds + ((ks % kX3Slots) * 4 + p) * kX3Plane;
            if (TN) {
                // (the K step goes into the VECTOR offset: that is the part of the address the range check sees)
                const uint32_t koff = (uint32_t)(kbeg + ks) * kX3BK * (uint32_t)ld * 2u;
#pragma unroll
                for (int b = 0; b < kX3Dma; ++b)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (x3_lds_ptr)(dst + b * 4 * kTile), 16, voff[b] + koff, 0, 0, 0);
            } else {
                const uint32_t soff = (uint32_t)(kbeg + ks) * kX3BK * 2u;
#pragma unroll
                for (int b = 0; b < kX3Dma; ++b)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (x3_lds_ptr)(dst + b * 16 * kX3BK), 16, voff[b], soff, 0, 0);
            }
        };
        // K steps younger than the one that must have landed: 0, 1 or 2 (x 8 DMA instructions each)
        auto wait_younger = [](int n) __attribute__((always_inline)) {
            if (n >= 2) wait_vmcnt<2 * kX3Dma>();
            else if (n == 1) wait_vmcnt<kX3Dma>();
            else wait_vmcnt<0>();
        };
        const int pro = min(kX3Slots, nk);
        for (int ks = 0; ks < pro; ++ks) issue(ks);
        if (pro - 1 >= 3) wait_vmcnt<3 * kX3Dma>();                   // K step 0 has landed
        else wait_younger(pro - 1);
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        for (int k = 0; k < nk; ++k) {
            wait_younger(min(k + 3, nk - 1) - (k + 1));                   // K step k + 1 has landed
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_barrier();                                 // barrier k: the MFMA waves are done reading K step k
            asm volatile("" ::: "memory");
            if (k + kX3Slots < nk) issue(k + kX3Slots);                   // into K step k's slot
        }
        return;
    }

    // ================= MFMA waves
    const int wr = w >> 1, wc = w & 1;
    const int fofs = (lane & 15) * kX3BK + (((lane >> 4) ^ ((lane >> 2) & 3)) << 3);   // + 16 rows per fragment repeat
    // TN: lane 4 q + pp of group gq addresses k row 8 gq + q (second read: + 4 rows, the same swz), elements 4 pp .. 4 pp + 3 of its block
    const int gq = lane >> 4, tq = (lane >> 2) & 3, tswz = tq | ((gq & 1) << 2);
    const int tofs = (gq * 8 + tq) * kTile + (lane & 3) * 4;                           // + ((column block ^ tswz) << 4) elements
    f32x4 acc[FI][FJ];
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    // fragments of one K step: [plane][repeat] (FI repeats of an A plane, FJ of a B plane)
    constexpr int FX = FI > FJ ? FI : FJ, NPL = X1 ? 2 : 4;               // (kX1NT: [0] = Ah, [1] = Bh)
    auto read = [&](int ks, bf16x8 (&f)[NPL][FX]) __attribute__((always_inline)) {
        const uint16_t* const s = x3lds + (ks % kX3Slots) * kSlot;
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl)
#pragma unroll
            for (int i = 0; i < FX; ++i)
                if constexpr (X1) {
                    if (i < (pl == 0 ? FI : FJ))
                        f[pl][i] = *reinterpret_cast<const bf16x8*>(s + (pl == 0 ? wr * WM * kX3BK : kPlaneA + wc * WN * kX3BK) + i * 16 * kX3BK + fofs);
                } else if constexpr (BM != BN) {                                  // (NT only) planes of two sizes
                    if (i < (pl < 2 ? FI : FJ))
                        f[pl][i] = *reinterpret_cast<const bf16x8*>(s + (pl < 2 ? pl * kPlaneA + wr * WM * kX3BK : 2 * kPlaneA + (pl - 2) * kPlaneB + wc * WN * kX3BK) +
                                                                    i * 16 * kX3BK + fofs);
                } else if constexpr (ATN != BTN) {                        // NN: A's planes by rows, B's K-major
                    if (pl < 2) {
                        f[pl][i] = *reinterpret_cast<const bf16x8*>(s + pl * kX3Plane + (wr * 64 + i * 16) * kX3BK + fofs);
                    } else {
                        const uint16_t* const a = s + pl * kX3Plane + tofs + (((wc * 4 + i) ^ tswz) << 4);
                        const i16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((x3_tr_ptr)a);
                        const i16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((x3_tr_ptr)(a + 4 * kTile));
                        f[pl][i] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo4, hi4, 0, 1, 2, 3, 4, 5, 6, 7));
                    }
                } else if constexpr (ATN) {
                    const uint16_t* const a = s + pl * kX3Plane + tofs + ((((pl < 2 ? wr : wc) * 4 + i) ^ tswz) << 4);
                    const i16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((x3_tr_ptr)a);
                    const i16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((x3_tr_ptr)(a + 4 * kTile));
                    f[pl][i] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo4, hi4, 0, 1, 2, 3, 4, 5, 6, 7));
                } else {
                    f[pl][i] = *reinterpret_cast<const bf16x8*>(s + pl * kX3Plane + ((pl < 2 ? wr : wc) * 64 + i * 16) * kX3BK + fofs);
                }
    };
    auto mul = [&](const bf16x8 (&f)[NPL][FX]) __attribute__((always_inline)) {
        if constexpr (X1) {
#pragma unroll
            for (int i = 0; i < FI; ++i)
#pragma unroll
                for (int j = 0; j < FJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[0][i], f[1][j], acc[i][j], 0, 0, 0);
        } else {
            // small products first, each pass over all FI x FJ accumulators (no back-to-back dependent MFMAs)
#pragma unroll
            for (int i = 0; i < FI; ++i)
#pragma unroll
                for (int j = 0; j < FJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[0][i], f[3][j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < FI; ++i)
#pragma unroll
                for (int j = 0; j < FJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[1][i], f[2][j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < FI; ++i)
#pragma unroll
                for (int j = 0; j < FJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[0][i], f[2][j], acc[i][j], 0, 0, 0);
        }
    };
    bf16x8 fa[NPL][FX], fb[NPL][FX];
    __syncthreads();                                                      // K step 0 has landed
    if (nk > 0) read(0, fa);
    // barrier k publishes K step k + 1 and frees K step k's slot (its fragments are in registers: lgkmcnt(0) first)
    auto step = [&](int k, bf16x8 (&cur)[NPL][FX], bf16x8 (&nxt)[NPL][FX]) __attribute__((always_inline)) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
        if (k + 1 < nk) read(k + 1, nxt);
        mul(cur);
    };
    for (int k = 0; k < nk; k += 2) {                                     // (nk is even: Kp % 64 == 0, slabs of an even count)
        step(k, fa, fb);
        step(k + 1, fb, fa);
    }
    float* const out = g.part ? g.part + (size_t)blockIdx.y * g.Mo * g.N : g.C;
    const int ldo = g.part ? g.N : g.ldc;
    const bool add = !g.part && g.accumulate;
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m0 + wr * WM + i * 16 + (lane >> 4) * 4 + e, col = n0 + wc * WN + j * 16 + (lane & 15);
                if (row < g.M && col < g.N) {
                    float* c = out + (size_t)row * ldo + col;
                    if constexpr (FORM == kX3NN) {
                        const float v = !g.part && g.cbias ? acc[i][j][e] + g.cbias[col] : acc[i][j][e];
                        *c = add ? *c + v : v;
                    } else {
                        *c = add ? *c + acc[i][j][e] : acc[i][j][e];
                    }
                } else if (FORM == kX3TN && row == g.M && g.bias && col < g.N) {
                    if (g.part) out[(size_t)row * ldo + col] = acc[i][j][e];
                    else g.bias[col] += acc[i][j][e];                      // (a bias gradient accumulates, as its weight's)
                }
            }
}

// C (+)= sum over slabs of part[s] (slab order); slab row M (Mo = M + 1 rows, gemm_bf16x3_tn's bias row) is ADDED to bias
__global__ __launch_bounds__(256) void reduce_slabs_kernel(const float* __restrict__ part, int slabs, int M, int N, float* __restrict__ C, int ldc,
                                                           int accumulate, int Mo, float* __restrict__ bias, const float* __restrict__ cbias)
{
    const size_t MN = (size_t)Mo * N;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < MN; i += (size_t)gridDim.x * 256) {
        float s = part[i];
        for (int k = 1; k < slabs; ++k) s += part[(size_t)k * MN + i];
        const size_t r = i / N;
        if (r < (size_t)M) {
            float* c = C + r * ldc + i % N;
            if (cbias) s = s + cbias[i % N];
            *c = accumulate ? *c + s : s;
        } else {
            bias[i % N] += s;
        }
    }
}
}  // namespace

hipError_t launch_cast_rows_bf16(const float* src, int ld, const int32_t* rowidx, int R, int K, uint16_t* dst, int ldd, hipStream_t st,
                                 uint16_t* dst_lo, int ones, int width)
{
    if (R <= 0 || K <= 0) return hipSuccess;
    ones = ones ? 1 : 0;
    if (width <= 0) width = bf16_pad(K + ones);
    if ((width & 7) || width < K + ones) return hipErrorInvalidValue;
    const int vec = !((reinterpret_cast<uintptr_t>(src) & 15) || (ld & 3));
    const long chunks = (long)R * (width / 8);
    const long blocks = (chunks + 255) / 256;
    const dim3 grid((unsigned)(blocks < 8192 ? blocks : 8192));
    if (dst_lo) hipLaunchKernelGGL(cast_rows_bf16_kernel<true>, grid, dim3(256), 0, st, src, ld, rowidx, R, K, dst, ldd, vec, dst_lo, ones, width);
    else hipLaunchKernelGGL(cast_rows_bf16_kernel<false>, grid, dim3(256), 0, st, src, ld, rowidx, R, K, dst, ldd, vec, dst_lo, ones, width);
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
    if (a.dst_lo) hipLaunchKernelGGL(cast_tr_bf16_kernel<true>, dim3((a.C + 63) / 64, ny), dim3(256), 0, st, a, vec);
    else hipLaunchKernelGGL(cast_tr_bf16_kernel<false>, dim3((a.C + 63) / 64, ny), dim3(256), 0, st, a, vec);
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

static int x3_cus()
{
    static const int cus = [] {
        int dev = 0, n = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
        return n > 0 ? n : 256;
    }();
    return cus;
}

int gemm_bf16x3_slabs(int M, int N, int Kp)
{
    // split-K where the tiles do not fill the chip (one workgroup per CU, one round): slabs of at least 16 K steps of 32
    const int tiles = ((M + kTile - 1) / kTile) * ((N + kTile - 1) / kTile), nk = Kp / kX3BK, cus = x3_cus();
    int s = 1;
    while (s < 8 && tiles * (s * 2) <= cus && nk / (s * 2) >= 16) s *= 2;
    return s;
}

int gemm_bf16x3_nt_tile_choice(int M, int N, int cus)
{
    // one workgroup per CU with either tile: rounds of workgroups x the tile's area is the work of the longest-running CU
    const auto up = [](long long a, long long b) { return (a + b - 1) / b; };
    const long long t192 = up(M, kX3TileM) * up(N, kX3TileN), t128 = up(M, kTile) * up(N, kTile);
    return up(t192, cus) * (kX3TileM * kX3TileN) < up(t128, cus) * (kTile * kTile) ? 1 : 0;
}

int gemm_bf16x3_pick_tile(int M, int N)
{
    static const int knob = [] { const char* e = getenv("S2VT_PICK_TILE"); return e && (e[0] == '0' || e[0] == '1') && !e[1] ? e[0] - '0' : -1; }();
    return knob >= 0 ? knob : gemm_bf16x3_nt_tile_choice(M, N, x3_cus());
}

size_t gemm_bf16x3_part_floats(int M, int N, int Kp)
{
    const int s = gemm_bf16x3_slabs(M, N, Kp);
    return s > 1 ? (size_t)s * M * N : 0;
}

namespace {
// the launch of any form (TN, NN: Kp = the reduction length K, any count; NT: Kp % 64 == 0); a tile other than 128 x 128 takes no split-K scratch
template <int FORM, int BM = kTile, int BN = kTile>
hipError_t launch_x3(const uint16_t* Ah, const uint16_t* Al, int lda, const uint16_t* Bh, const uint16_t* Bl, int ldb, float* C, int ldc, int M, int N,
                     int Kp, int accumulate, float* bias, float* part, size_t part_floats, int cls, hipStream_t st, const float* cbias = nullptr)
{
    constexpr bool kWide = BM != BN, kOne = FORM == kX1NT;
    constexpr int kLds = kOne ? x1_lds_bytes(BM, BN) : x3_lds_bytes(BM, BN), kCfg = kOne ? 18 : kWide ? 17 : 16;     // (the launch profiler's tile id)
    if (M <= 0 || N <= 0) return hipSuccess;
    if (kWide && part) return hipErrorInvalidValue;
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_bf16x3_kernel<FORM, BM, BN>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
    if (attr != hipSuccess) return attr;
    GemmX3Args g;
    g.Ah = Ah; g.Al = Al; g.lda = lda; g.Bh = Bh; g.Bl = Bl; g.ldb = ldb; g.C = C; g.ldc = ldc; g.M = M; g.N = N;
    g.K = Kp; g.bias = bias; g.Mo = M + (bias ? 1 : 0); g.cbias = cbias;
    const int Kr = bf16_pad(Kp);
    g.nk = Kr / kX3BK; g.accumulate = accumulate;
    g.tiles_m = (g.Mo + BM - 1) / BM; g.tiles_n = (N + BN - 1) / BN;
    int slabs = part ? gemm_bf16x3_slabs(g.Mo, N, Kr) : 1;
    if ((size_t)slabs * g.Mo * N > part_floats) slabs = 1;
    g.nk_slab = ((g.nk + slabs - 1) / slabs + 1) & ~1;                    // >= nk / slabs (so no more slabs than the scratch holds), even:
    slabs = g.nk_slab ? (g.nk + g.nk_slab - 1) / g.nk_slab : 1;           // the MFMA loop takes K steps in pairs
    g.part = slabs > 1 ? part : nullptr;
    const dim3 grid((unsigned)(g.tiles_m * g.tiles_n), (unsigned)slabs);
    const bool prof = prof_wants(cls, kCfg);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (prof) {
        hipError_t pe = prof_events(&e0, &e1);
        if (pe != hipSuccess) return pe;
        (void)hipEventRecord(e0, st);
    }
    hipLaunchKernelGGL((gemm_bf16x3_kernel<FORM, BM, BN>), grid, dim3(512), kLds, st, g);
    if (slabs > 1) {
        const size_t MN = (size_t)g.Mo * N, blocks = (MN + 255) / 256;
        hipLaunchKernelGGL(reduce_slabs_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, (const float*)part, slabs, M, N, C, ldc,
                           accumulate, g.Mo, bias, cbias);
    }
    if (prof) {
        (void)hipEventRecord(e1, st);
        const char* const name = kOne ? (cls == 2 ? "x1_192x96(dma) pick screen" : "x1_192x96(dma)")
                                 : kWide ? (cls == 2 ? "x3_192x96(dma) pick screen" : cls == 3 ? "x3_192x96(dma) wgrad" : "x3_192x96(dma) dgrad")
                                       : cls == 0 ? "x3_128x128(dma) fwd" : cls == 2 ? "x3_128x128(dma) pick screen" : cls == 3 ? "x3_128x128(dma) wgrad" : "x3_128x128(dma) dgrad";
        prof_record(cls, kCfg, name, 2.0 * M * (double)N * Kp, e0, e1);
    }
    return hipGetLastError();
}
}  // namespace

hipError_t launch_gemm_bf16x3_nt(const uint16_t* Ah, const uint16_t* Al, int lda, const uint16_t* Bh, const uint16_t* Bl, int ldb, float* C, int ldc,
                                 int M, int N, int Kp, int accumulate, float* part, size_t part_floats, int cls, hipStream_t st, int tile)
{
    if (tile == 1 && !part) return launch_x3<kX3NT, kX3TileM, kX3TileN>(Ah, Al, lda, Bh, Bl, ldb, C, ldc, M, N, Kp, accumulate, nullptr, nullptr, 0, cls, st);
    return launch_x3<kX3NT>(Ah, Al, lda, Bh, Bl, ldb, C, ldc, M, N, Kp, accumulate, nullptr, part, part_floats, cls, st);
}

hipError_t launch_gemm_bf16x1_nt(const uint16_t* Ah, int lda, const uint16_t* Bh, int ldb, float* C, int ldc, int M, int N, int Kp, int accumulate, int cls,
                                 hipStream_t st)
{
    return launch_x3<kX1NT, kX3TileM, kX3TileN>(Ah, nullptr, lda, Bh, nullptr, ldb, C, ldc, M, N, Kp, accumulate, nullptr, nullptr, 0, cls, st);
}

bool gemm_bf16x3_tn_ok(int lda, int ldb, int K)
{
    // the loader forms byte offsets of the planes in 32 bits (K steps up to bf16_pad(K) rows, a tile's 256 bytes behind them)
    const unsigned long long ld = (unsigned long long)(lda > ldb ? lda : ldb);
    return K >= 0 && lda > 0 && ldb > 0 && ((unsigned long long)bf16_pad(K) + 1) * ld * 2ull + 512ull < (1ull << 31);
}

hipError_t launch_gemm_bf16x3_tn(const uint16_t* Ah, const uint16_t* Al, int lda, const uint16_t* Bh, const uint16_t* Bl, int ldb, float* C, int ldc,
                                 int M, int N, int K, int accumulate, float* bias, float* part, size_t part_floats, int cls, hipStream_t st)
{
    if (!gemm_bf16x3_tn_ok(lda, ldb, K)) return hipErrorInvalidValue;
    return launch_x3<kX3TN>(Ah, Al, lda, Bh, Bl, ldb, C, ldc, M, N, K, accumulate, bias, part, part_floats, cls, st);
}

hipError_t launch_gemm_bf16x3_nn(const uint16_t* Ah, const uint16_t* Al, int lda, const uint16_t* Bh, const uint16_t* Bl, int ldb, float* C, int ldc,
                                 int M, int N, int K, int accumulate, const float* cbias, float* part, size_t part_floats, int cls, hipStream_t st)
{
    if (!gemm_bf16x3_tn_ok(ldb, ldb, K) || lda < bf16_pad(K) || (cbias && accumulate)) return hipErrorInvalidValue;
    return launch_x3<kX3NN>(Ah, Al, lda, Bh, Bl, ldb, C, ldc, M, N, K, accumulate, nullptr, part, part_floats, cls, st, cbias);
}

}  // namespace s2vt
