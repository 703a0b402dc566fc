// bf16 TN GEMM on MFMA for gfx950:  C[M,N] = epi( A[M,K] . W[N,K]^T )
//
// Both operands are K-contiguous (activations row-major, nn.Linear weights [out,in]), which is
// exactly the lane layout v_mfma_f32_16x16x32_bf16 wants: lane l supplies 8 consecutive k
// (16 bytes) of row l&15, k-group l>>4.  Tiles are staged global -> registers -> LDS
// (double-buffered, one barrier per K-step); the LDS image is [rows][64 k] bf16 with the 16-byte
// chunk index XOR-swizzled by (row>>1)&7 so that the 16 rows x 4 chunks a ds_read_b128 fragment
// read touches land on 16 distinct 16-byte slots of the 256-byte bank row (conflict-free).
//
// Block = 256 threads = 4 waves arranged WM x WN; wave tile (BM/WM) x (BN/WN) of 16x16 MFMA tiles.
// blockIdx -> tile mapping is XCD-aware: consecutive tile ids (which share the same W panel)
// are dealt to the same XCD so a panel is fetched into one L2 instead of eight.
#include <stdlib.h>
#include "common.h"

#define BK 64

// One BM x BN output tile at (m0, n0) over the K steps [kb, nk) of BK: the whole tile code, shared by gemm_bf16_tn_kernel and the
// grouped form below (rows >= M and columns >= N are masked; m0 need not be a multiple of BM).
template <int BM, int BN, int WM, int WN>
__device__ __forceinline__ void gemm_bf16_tn_tile(
    const bf16_t* __restrict__ A, int64_t lda, const bf16_t* __restrict__ W, int64_t ldw,
    const float* __restrict__ bias, int M, int N, int K, float alpha, int act, const float* residual,
    bf16_t* out_bf16, float* out_f32, int64_t ldc, int m0, int n0, int kb, int nk) {
    constexpr int TM = BM / WM / 16;  // 16-row MFMA tiles per wave along M
    constexpr int TN = BN / WN / 16;
    constexpr int A_CHUNKS = BM * (BK / 8) / 256;  // 16-byte chunks per thread per tile
    constexpr int B_CHUNKS = BN * (BK / 8) / 256;
    static_assert(A_CHUNKS >= 1 && B_CHUNKS >= 1, "tile too small for 256 threads");

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // layout: [buf][A tile | B tile]
    constexpr int A_BYTES = BM * BK * 2;
    constexpr int B_BYTES = BN * BK * 2;
    constexpr int STAGE_BYTES = A_BYTES + B_BYTES;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int fr = lane & 15, fq = lane >> 4;

    float4_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (float4_t){0.f, 0.f, 0.f, 0.f};

    uint4 ra[A_CHUNKS], rb[B_CHUNKS];

    auto gload = [&](int kt) {
        const int k0 = kt * BK;
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) {
            const int id = tid + i * 256;
            const int row = id >> 3, c = id & 7;
            const int gm = m0 + row, gk = k0 + c * 8;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (gm < M && gk < K) v = *reinterpret_cast<const uint4*>(A + (int64_t)gm * lda + gk);
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < B_CHUNKS; ++i) {
            const int id = tid + i * 256;
            const int row = id >> 3, c = id & 7;
            const int gn = n0 + row, gk = k0 + c * 8;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (gn < N && gk < K) v = *reinterpret_cast<const uint4*>(W + (int64_t)gn * ldw + gk);
            rb[i] = v;
        }
    };
    auto lstore = [&](int buf) {
        unsigned char* sa = smem + buf * STAGE_BYTES;
        unsigned char* sb = sa + A_BYTES;
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) {
            const int id = tid + i * 256;
            const int row = id >> 3, c = id & 7;
            *reinterpret_cast<uint4*>(sa + row * 128 + ((c ^ ((row >> 1) & 7)) << 4)) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < B_CHUNKS; ++i) {
            const int id = tid + i * 256;
            const int row = id >> 3, c = id & 7;
            *reinterpret_cast<uint4*>(sb + row * 128 + ((c ^ ((row >> 1) & 7)) << 4)) = rb[i];
        }
    };

    gload(kb);
    lstore(0);
    __syncthreads();

    for (int kt = kb; kt < nk; ++kt) {
        const int cur = (kt - kb) & 1;
        if (kt + 1 < nk) gload(kt + 1);
        const unsigned char* sa = smem + cur * STAGE_BYTES;
        const unsigned char* sb = sa + A_BYTES;
#pragma unroll
        for (int ks = 0; ks < BK / 32; ++ks) {
            short8_t af[TM], bfr[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = wm * (BM / WM) + i * 16 + fr;
                const int c = ks * 4 + fq;
                af[i] = *reinterpret_cast<const short8_t*>(sa + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int row = wn * (BN / WN) + j * 16 + fr;
                const int c = ks * 4 + fq;
                bfr[j] = *reinterpret_cast<const short8_t*>(sb + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < nk) lstore(cur ^ 1);
        __syncthreads();
    }

    // ---- epilogue: C/D map of 16x16 MFMA: col = lane&15, row = (lane>>4)*4 + reg ----
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn * (BN / WN) + j * 16 + fr;
            if (n >= N) continue;
            const float b = bias ? bias[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm * (BM / WM) + i * 16 + fq * 4 + r;
                if (m >= M) continue;
                float v = (acc[i][j][r] + b) * alpha;
                v = devqa_act(v, act);
                const int64_t o = (int64_t)m * ldc + n;
                if (residual) v += residual[o];
                if (out_f32) out_f32[o] = v;
                if (out_bf16) out_bf16[o] = f32_to_bf16(v);
            }
        }
    }
}

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void gemm_bf16_tn_kernel(
    const bf16_t* __restrict__ A, int64_t lda, const bf16_t* __restrict__ W, int64_t ldw,
    const float* __restrict__ bias, int M, int N, int K, float alpha, int act, const float* residual,
    bf16_t* out_bf16, float* out_f32, int64_t ldc, int tiles_m, int tiles_n, int steps_per_split) {
    // ---- XCD-aware tile id: blocks b and b+8 share an XCD; give each XCD a contiguous run ----
    const int nwg = tiles_m * tiles_n;
    int bid = blockIdx.x;
    {
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    // m fastest: consecutive blocks walk down M for one N panel (W panel stays L2 resident)
    const int tile_m = bid % tiles_m;
    const int tile_n = bid / tiles_m;
    // split-K: blockIdx.y owns K steps [kb, nk) and writes a raw fp32 partial slab (steps_per_split > 0)
    const int nk_all = (K + BK - 1) / BK;
    const int kb = steps_per_split > 0 ? (int)blockIdx.y * steps_per_split : 0;
    const int nk = steps_per_split > 0 ? min(nk_all, kb + steps_per_split) : nk_all;
    if (steps_per_split > 0) out_f32 += (int64_t)blockIdx.y * M * ldc;
    gemm_bf16_tn_tile<BM, BN, WM, WN>(A, lda, W, ldw, bias, M, N, K, alpha, act, residual, out_bf16, out_f32, ldc, tile_m * BM, tile_n * BN, kb, nk);
}

// ---- grouped form (the post-edit tail of the batched FT_VL evaluation): every row tile has its OWN weight matrix.  tab: int32
// [n_mt][3] = (edit e, first row m0, end row m1 of e's segment) per row tile; rows [m0, min(m0 + BM, m1)) of y += A . W_e^T.  Same
// tile code, same K order as one gemm_bf16_tn_kernel launch per edit: same bits.
template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void gemm_bf16_tn_grouped_kernel(
    const bf16_t* __restrict__ A, int64_t lda, const bf16_t* __restrict__ W, int64_t ldw, int64_t w_stride_e, const int32_t* __restrict__ tab,
    int n_mt, int E, int R, int N, int K, float* y, int64_t ldc) {
    const int t = blockIdx.x % n_mt, tile_n = blockIdx.x / n_mt;     // m fastest: the edits of one column panel side by side
    const int e = tab[3 * t], m0 = tab[3 * t + 1], m1 = tab[3 * t + 2];
    if (e < 0 || e >= E || m0 < 0 || m1 > R || m0 >= m1) return;    // (uniform per workgroup)
    gemm_bf16_tn_tile<BM, BN, WM, WN>(A, lda, W + (int64_t)e * w_stride_e, ldw, nullptr, m1, N, K, 1.0f, 0, y, nullptr, y, ldc, m0, tile_n * BN, 0,
                                      (K + BK - 1) / BK);
}

extern "C" int devqa_gemm_grouped_bf16(const devqa_bf16* A, int64_t lda, const devqa_bf16* W, int64_t ldw, int64_t w_stride_e, const int32_t* tile_tab,
                                       int n_tiles, int bm, int E, int R, int N, int K, float* y, int64_t ldc, void* stream) {
    DEVQA_CHECK_ARG(A && W && tile_tab && y, "gemm_grouped: null pointer");
    if (n_tiles == 0 || N == 0) return DEVQA_OK;
    DEVQA_CHECK_ARG(bm == 32 || bm == 64, "gemm_grouped: row tile %d (32 or 64)", bm);
    DEVQA_CHECK_SHAPE(n_tiles > 0 && E > 0 && R > 0 && N > 0 && K > 0, "gemm_grouped: bad dims");
    DEVQA_CHECK_SHAPE(K % 8 == 0 && lda % 8 == 0 && ldw % 8 == 0 && w_stride_e % 8 == 0 && lda >= K && ldw >= K && ldc >= N,
                      "gemm_grouped: K / leading dims must be multiples of 8 and cover the matrices");
    DEVQA_CHECK_SHAPE((((uintptr_t)A) & 15) == 0 && (((uintptr_t)W) & 15) == 0, "gemm_grouped: operands must be 16-byte aligned");
    // one launch per edit would split a long K over workgroups (devqa_gemm_bf16's small-M rule, from 8 K steps on): not this kernel's order
    DEVQA_CHECK_SHAPE(devqa_gemm_grouped_supported(DEVQA_DTYPE_BF16, K), "gemm_grouped: K=%d takes the split-K path per edit", K);
    hipStream_t st = (hipStream_t)stream;
    const int tiles_n = (N + 127) / 128;
    const size_t smem = 2 * (size_t)(bm + 128) * BK * 2;
    if (bm == 32)
        hipLaunchKernelGGL((gemm_bf16_tn_grouped_kernel<32, 128, 1, 4>), dim3(n_tiles * tiles_n), dim3(256), smem, st, A, lda, W, ldw, w_stride_e,
                           tile_tab, n_tiles, E, R, N, K, y, ldc);
    else
        hipLaunchKernelGGL((gemm_bf16_tn_grouped_kernel<64, 128, 2, 2>), dim3(n_tiles * tiles_n), dim3(256), smem, st, A, lda, W, ldw, w_stride_e,
                           tile_tab, n_tiles, E, R, N, K, y, ldc);
    DEVQA_LAUNCH_CHECK("gemm_grouped");
    return DEVQA_OK;
}

// 1 when one devqa_gemm_bf16 / devqa_gemm_f32 call per edit (few rows, reduction length K) sums K in ONE k-ordered chain -- the order of
// the grouped kernels -- whatever its row count: below the split-K rules of the two dispatchers
extern "C" int devqa_gemm_grouped_supported(int dtype, int K) {
    if (dtype == DEVQA_DTYPE_BF16) return K > 0 && K % 8 == 0 && (K + BK - 1) / BK / 4 < 2;
    return dtype == DEVQA_DTYPE_F32 && K > 0 && K % 4 == 0 && K < 2048;
}

#include <mutex>
#include <vector>
// ---- split-K for skinny problems with a very long K (dH = dlogits . E: M <= 256, N = 2560, K = 50272) ----
__global__ void splitk_reduce_kernel(const float* __restrict__ part, int splits, int64_t mn4, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < mn4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 s = reinterpret_cast<const float4*>(part)[i];
        for (int k = 1; k < splits; ++k) {
            const float4 p = reinterpret_cast<const float4*>(part)[(int64_t)k * mn4 + i];
            s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
        }
        reinterpret_cast<float4*>(out)[i] = s;
    }
}

extern "C" int devqa_gemm_bf16_splitk(const devqa_bf16* A, int64_t lda, const devqa_bf16* W, int64_t ldw, int M, int N, int K,
                                      int splits, float* partial_ws, float* out_f32, void* stream) {
    DEVQA_CHECK_ARG(A && W && partial_ws && out_f32, "gemm_splitk: null pointer");
    if (M == 0 || N == 0) return DEVQA_OK;
    DEVQA_CHECK_SHAPE(M > 0 && M <= 256 && N > 0 && N % 4 == 0 && K > 0, "gemm_splitk: needs 0 < M <= 256, N %% 4 == 0");
    DEVQA_CHECK_SHAPE(K % 8 == 0 && lda % 8 == 0 && ldw % 8 == 0 && lda >= K && ldw >= K, "gemm_splitk: bad K / leading dims");
    DEVQA_CHECK_SHAPE((((uintptr_t)A) & 15) == 0 && (((uintptr_t)W) & 15) == 0, "gemm_splitk: operands must be 16-byte aligned");
    const int nk = (K + BK - 1) / BK;
    DEVQA_CHECK_SHAPE(splits >= 1 && splits <= nk && splits <= 1024, "gemm_splitk: bad split count %d", splits);
    const int steps = (nk + splits - 1) / splits;
    const int used = (nk + steps - 1) / steps;  // every launched split owns >= 1 step
    hipStream_t st = (hipStream_t)stream;
    const int tiles_n = (N + 127) / 128;
    // one row tile covers all M rows, so W (the long operand: 257 MB for dH = dlogits . E) streams through the chip ONCE per call
    if (M <= 64) {
        auto kern = gemm_bf16_tn_kernel<64, 128, 2, 2>;
        hipLaunchKernelGGL(kern, dim3(tiles_n, used), dim3(256), 2 * (64 + 128) * BK * 2, st, A, lda, W, ldw, (const float*)nullptr, M,
                           N, K, 1.0f, 0, (const float*)nullptr, (bf16_t*)nullptr, partial_ws, (int64_t)N, 1, tiles_n, steps);
    } else if (M <= 128) {
        auto kern = gemm_bf16_tn_kernel<128, 128, 2, 2>;
        static bool attr128 = false;
        if (!attr128) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (128 + 128) * BK * 2);
            attr128 = true;
        }
        hipLaunchKernelGGL(kern, dim3(tiles_n, used), dim3(256), 2 * (128 + 128) * BK * 2, st, A, lda, W, ldw, (const float*)nullptr, M,
                           N, K, 1.0f, 0, (const float*)nullptr, (bf16_t*)nullptr, partial_ws, (int64_t)N, 1, tiles_n, steps);
    } else {
        auto kern = gemm_bf16_tn_kernel<256, 128, 2, 2>;
        static bool attr256 = false;
        if (!attr256) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (256 + 128) * BK * 2);
            attr256 = true;
        }
        hipLaunchKernelGGL(kern, dim3(tiles_n, used), dim3(256), 2 * (256 + 128) * BK * 2, st, A, lda, W, ldw, (const float*)nullptr, M,
                           N, K, 1.0f, 0, (const float*)nullptr, (bf16_t*)nullptr, partial_ws, (int64_t)N, 1, tiles_n, steps);
    }
    DEVQA_LAUNCH_CHECK("gemm_splitk");
    const int64_t mn4 = (int64_t)M * N / 4;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((mn4 + 255) / 256 < 1024 ? (mn4 + 255) / 256 : 1024)), dim3(256), 0, st,
                       partial_ws, used, mn4, out_f32);
    DEVQA_LAUNCH_CHECK("splitk_reduce");
    return DEVQA_OK;
}

// Kernel-selection mode for A/B measurements (debugging aid, process-wide by design: it selects among kernels that issue the same
// MFMA sequence per output element, so a launch that races with a mode change still computes the same result).
static std::atomic<int> g_gemm_mode_a{-1};
static int gemm_mode() {
    int m = g_gemm_mode_a.load(std::memory_order_relaxed);
    if (m < 0) {
        const char* e = getenv("DEVQA_GEMM");
        int want = e ? atoi(e) : 0;
        if (want < 0 || (want > 3 && (want < 10 || want > 28))) want = 0;
        int expect = -1;
        g_gemm_mode_a.compare_exchange_strong(expect, want);
        m = g_gemm_mode_a.load(std::memory_order_relaxed);
    }
    return m;
}
extern "C" int devqa_gemm_set_mode(int mode) {
    if (mode < 0 || (mode > 3 && (mode < 10 || mode > 28))) return devqa_fail(DEVQA_E_ARG, "gemm_set_mode: bad mode %d", mode);
    g_gemm_mode_a.store(mode);
    return DEVQA_OK;
}

int launch_gemm_pipe(int id, const bf16_t*, int64_t, const bf16_t*, int64_t, const float*, int, int, int, float, int, const float*,
                     bf16_t*, float*, int64_t, hipStream_t);  // gemm_bf16_pipe.hip
int launch_gemm_pp(int id, const bf16_t*, int64_t, const bf16_t*, int64_t, const float*, int, int, int, float, int, const float*,
                   bf16_t*, float*, int64_t, hipStream_t);    // gemm_bf16_pp.hip
// LDS-DMA staged variants (gemm_bf16_glds.hip)
int launch_gemm_glds_64x128(const bf16_t*, int64_t, const bf16_t*, int64_t, const float*, int, int, int, float, int, const float*,
                            bf16_t*, float*, int64_t, hipStream_t);
int launch_gemm_glds_128x128(const bf16_t*, int64_t, const bf16_t*, int64_t, const float*, int, int, int, float, int, const float*,
                             bf16_t*, float*, int64_t, hipStream_t);
template <int BM, int BN, int WM, int WN>
static int launch_gemm(const bf16_t* A, int64_t lda, const bf16_t* W, int64_t ldw, const float* bias, int M, int N,
                       int K, float alpha, int act, const float* residual, bf16_t* out_bf16, float* out_f32,
                       int64_t ldc, hipStream_t st) {
    const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
    const size_t smem = 2 * (BM + BN) * BK * 2;
    auto kern = gemm_bf16_tn_kernel<BM, BN, WM, WN>;
    static std::atomic<unsigned> attr_done{0};
    if (smem > 48 * 1024) devqa_set_max_smem(kern, smem, attr_done);
    const int ph = devqa_prof_begin(BM == 32 ? 0 : (BM == 64 ? 1 : 2), st);
    hipLaunchKernelGGL(kern, dim3(tiles_m * tiles_n), dim3(256), smem, st, A, lda, W, ldw, bias, M, N, K, alpha, act,
                       residual, out_bf16, out_f32, ldc, tiles_m, tiles_n, 0);
    devqa_prof_end(ph, 2.0 * (double)M * (double)N * (double)K, st);
    DEVQA_LAUNCH_CHECK("gemm_bf16");
    return DEVQA_OK;
}

// ---- small-M GEMMs (M <= 64: B = 1 probes, the MEND / T-Patcher edit passes) are weight streams: with one 64x128 tile per
// 128 output columns a [64 x 10240 x 2560] product runs on 80 workgroups and ~1 TB/s.  Split K over enough workgroups to fill
// the chip (fp32 partials in a library-owned, per-stream workspace), then one pass sums the partials and applies the usual
// epilogue (bias, alpha, activation, residual, bf16 / fp32 outputs).
__global__ void splitk_reduce_epilogue_kernel(const float* __restrict__ part, int splits, int M, int N, const float* __restrict__ bias,
                                              float alpha, int act, const float* residual, bf16_t* out_bf16, float* out_f32,
                                              int64_t ldc) {
    const int n4 = N >> 2;
    const int64_t mn4 = (int64_t)M * n4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < mn4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 s = reinterpret_cast<const float4*>(part)[i];
        for (int k = 1; k < splits; ++k) {
            const float4 p = reinterpret_cast<const float4*>(part)[(int64_t)k * mn4 + i];
            s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
        }
        const int m = (int)(i / n4), n = (int)(i - (int64_t)m * n4) * 4;
        if (bias) {
            const float4 b = *reinterpret_cast<const float4*>(bias + n);
            s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w;
        }
        s.x *= alpha; s.y *= alpha; s.z *= alpha; s.w *= alpha;
        s = devqa_act4(s, act);
        const int64_t o = (int64_t)m * ldc + n;
        if (residual) {
            const float4 r = *reinterpret_cast<const float4*>(residual + o);
            s.x += r.x; s.y += r.y; s.z += r.z; s.w += r.w;
        }
        if (out_f32) *reinterpret_cast<float4*>(out_f32 + o) = s;
        if (out_bf16) {
            uint2 p;
            p.x = pack_bf16x2(s.x, s.y);
            p.y = pack_bf16x2(s.z, s.w);
            *reinterpret_cast<uint2*>(out_bf16 + o) = p;
        }
    }
}

namespace {
constexpr size_t SPLITK_WS_BYTES = 36u << 20;
struct SplitKWs { hipStream_t st; int dev; float* p; size_t bytes; };
SplitKWs g_skws[8] = {};
std::mutex g_skws_mu;
float* splitk_workspace(hipStream_t st, size_t bytes) {   // one buffer per (device, stream): concurrent streams never share
    std::lock_guard<std::mutex> lock(g_skws_mu);          // host threads (the training prefetch thread) may race for a slot
    int dev = 0;
    (void)hipGetDevice(&dev);
    SplitKWs* slot = nullptr;
    for (auto& w : g_skws)
        if (w.p && w.st == st && w.dev == dev) { slot = &w; break; }
    if (!slot)
        for (auto& w : g_skws)
            if (!w.p) { slot = &w; break; }
    if (!slot) return nullptr;
    // ONE fixed-size buffer per (device, stream), allocated at first use and never freed or regrown: the largest request of the
    // small-M rule is 512/tiles slabs of <= tiles x (128 x 128) fp32 = 32 MiB, so the launch path never synchronises or frees.
    if (bytes > SPLITK_WS_BYTES) return nullptr;
    if (!slot->p) {
        if (hipMalloc(reinterpret_cast<void**>(&slot->p), SPLITK_WS_BYTES) != hipSuccess) { (void)hipGetLastError(); slot->p = nullptr; return nullptr; }
        slot->bytes = SPLITK_WS_BYTES; slot->st = st; slot->dev = dev;
    }
    return slot->p;
}
}  // namespace

// shared with gemm_f32.hip: the per-(device, stream) partial-sum workspace and the reduce + epilogue pass
float* devqa_splitk_workspace(hipStream_t st, size_t bytes) { return splitk_workspace(st, bytes); }
void devqa_launch_splitk_reduce_epilogue(const float* ws, int splits, int M, int N, const float* bias, float alpha, int act,
                                         const float* residual, bf16_t* out_bf16, float* out_f32, int64_t ldc, hipStream_t st) {
    const int64_t mn4 = (int64_t)M * N / 4;
    hipLaunchKernelGGL(splitk_reduce_epilogue_kernel, dim3((unsigned)((mn4 + 255) / 256 < 2048 ? (mn4 + 255) / 256 : 2048)), dim3(256), 0,
                       st, ws, splits, M, N, bias, alpha, act, residual, out_bf16, out_f32, ldc);
}

// 1 when a fused-SwiGLU call of this shape takes the 256 x 256 ping-pong kernel under the current mode (the dispatch rule of devqa_gemm_bf16 below)
extern "C" int devqa_gemm_bf16_swiglu_supported(int M, int N, int K) {
    const int g_gemm_mode = gemm_mode();
    if (M <= 64 || N <= 0 || K <= 0 || N % 256 != 0 || K % 64 != 0) return 0;
    if (g_gemm_mode == 1 || g_gemm_mode == 2 || g_gemm_mode == 3 || (g_gemm_mode >= 10 && g_gemm_mode < 20)) return 0;
    if (g_gemm_mode >= 20) return 1;
    const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128);
    const long t256 = (long)((M + 255) / 256) * ((N + 255) / 256);
    return (t128 >= 384 && t256 >= 128) ? 1 : 0;
}

extern "C" int devqa_gemm_bf16(const devqa_bf16* A, int64_t lda, const devqa_bf16* W, int64_t ldw, const float* bias,
                               int M, int N, int K, float alpha, int act, const float* residual, devqa_bf16* out_bf16,
                               float* out_f32, int64_t ldc, void* stream) {
    return devqa_gemm_bf16_as(M, A, lda, W, ldw, bias, M, N, K, alpha, act, residual, out_bf16, out_f32, ldc, stream);
}

// devqa_gemm_bf16 on M rows with every dispatch decision (kernel family, split-K slicing) taken as for Md >= M rows: a row of the
// result then has the bits the same row has in an Md-row call -- the K order of an output element depends on the kernel and the
// slicing, never on its tile-mates (devqa_llm_prefix_rows: the kept rows of the last layer)
int devqa_gemm_bf16_as(int Md, const devqa_bf16* A, int64_t lda, const devqa_bf16* W, int64_t ldw, const float* bias,
                       int M, int N, int K, float alpha, int act, const float* residual, devqa_bf16* out_bf16,
                       float* out_f32, int64_t ldc, void* stream) {
    DEVQA_CHECK_ARG(A && W, "gemm: null operand");
    DEVQA_CHECK_ARG(Md >= M, "gemm: dispatch rows %d < rows %d", Md, M);
    DEVQA_CHECK_ARG(out_bf16 || out_f32, "gemm: no output");
    DEVQA_CHECK_ARG(act >= 0 && act <= DEVQA_ACT_SWIGLU_IL16, "gemm: bad act %d", act);
    if (M == 0 || N == 0) return DEVQA_OK;
    DEVQA_CHECK_SHAPE(M > 0 && N > 0 && K > 0, "gemm: bad dims %d %d %d", M, N, K);
    DEVQA_CHECK_SHAPE(K % 8 == 0 && lda % 8 == 0 && ldw % 8 == 0, "gemm: K/lda/ldw must be multiples of 8 (K=%d lda=%lld ldw=%lld)",
                      K, (long long)lda, (long long)ldw);
    DEVQA_CHECK_SHAPE(lda >= K && ldw >= K && ldc >= (act == DEVQA_ACT_SWIGLU_IL16 ? N / 2 : N), "gemm: leading dims too small");
    DEVQA_CHECK_SHAPE((((uintptr_t)A) & 15) == 0 && (((uintptr_t)W) & 15) == 0, "gemm: operands must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int g_gemm_mode = gemm_mode();
    if (act == DEVQA_ACT_SWIGLU_IL16) {      // fused SwiGLU: the 256 x 256 kernel only (devqa_gemm_bf16_swiglu_supported says when)
        if (!devqa_gemm_bf16_swiglu_supported(Md, N, K)) return devqa_fail(DEVQA_E_SHAPE, "gemm_bf16: fused SwiGLU is not available for M=%d N=%d K=%d in this mode", M, N, K);
        const int ph = devqa_prof_begin(3, st);
        const int rc = launch_gemm_pp(g_gemm_mode >= 20 ? g_gemm_mode - 20 : 2, A, lda, W, ldw, bias, M, N, K, alpha, act, residual, out_bf16, out_f32, ldc, st);
        devqa_prof_end(ph, 2.0 * (double)M * (double)N * (double)K, st);
        return rc;
    }
    // Skinny problems are weight streams: with one 64x128 (128x128) tile per 128 output columns a [64 x 10240 x 2560] product runs
    // on 80 workgroups, and the 257-row GEMMs of a single-image ViT pass on 33-165.  When the tiles cover less than half the chip,
    // split K over enough workgroups to fill it (fp32 partials in the per-stream workspace, one reduce + epilogue pass).
    static int splitk_max_m = -1;     // DEVQA_SPLITK_MAXM (default 1024; 64 = the small-M rule only) for A/B runs
    if (splitk_max_m < 0) {
        const char* e = getenv("DEVQA_SPLITK_MAXM");
        splitk_max_m = e ? atoi(e) : 1024;
    }
    if (Md <= splitk_max_m && g_gemm_mode == 0 && N % 4 == 0 && ldc % 4 == 0 &&
        ((((uintptr_t)out_f32) | ((uintptr_t)residual) | ((uintptr_t)bias)) & 15) == 0 && (((uintptr_t)out_bf16) & 7) == 0) {
        const int bm = Md <= 64 ? 64 : 128;
        const int tiles_m = (M + bm - 1) / bm, tiles_n = (N + 127) / 128, nk = (K + BK - 1) / BK;
        const int tiles = tiles_m * tiles_n, tiles_d = (Md + bm - 1) / bm * tiles_n;     // launched / deciding
        int splits = (Md <= 64 || tiles_d < 128) ? 512 / tiles_d : 1;
        if (splits > nk / 4) splits = nk / 4;
        if (splits >= 2) {
            const int steps = (nk + splits - 1) / splits;
            const int used = (nk + steps - 1) / steps;
            float* ws = splitk_workspace(st, (size_t)used * Md * N * sizeof(float));
            if (ws) {
                if (bm == 64) {
                    auto kern = gemm_bf16_tn_kernel<64, 128, 2, 2>;
                    hipLaunchKernelGGL(kern, dim3(tiles, used), dim3(256), 2 * (64 + 128) * BK * 2, st, A, lda, W, ldw, (const float*)nullptr,
                                       M, N, K, 1.0f, 0, (const float*)nullptr, (bf16_t*)nullptr, ws, (int64_t)N, tiles_m, tiles_n, steps);
                } else {
                    auto kern = gemm_bf16_tn_kernel<128, 128, 2, 2>;
                    static std::atomic<unsigned> attr_done{0};
                    devqa_set_max_smem(kern, 2 * (128 + 128) * BK * 2, attr_done);
                    hipLaunchKernelGGL(kern, dim3(tiles, used), dim3(256), 2 * (128 + 128) * BK * 2, st, A, lda, W, ldw, (const float*)nullptr,
                                       M, N, K, 1.0f, 0, (const float*)nullptr, (bf16_t*)nullptr, ws, (int64_t)N, tiles_m, tiles_n, steps);
                }
                DEVQA_LAUNCH_CHECK("gemm_small_m_splitk");
                const int64_t mn4 = (int64_t)M * N / 4;
                hipLaunchKernelGGL(splitk_reduce_epilogue_kernel, dim3((unsigned)((mn4 + 255) / 256 < 2048 ? (mn4 + 255) / 256 : 2048)),
                                   dim3(256), 0, st, ws, used, M, N, bias, alpha, act, residual, out_bf16, out_f32, ldc);
                DEVQA_LAUNCH_CHECK("splitk_reduce_epilogue");
                return DEVQA_OK;
            }
        }
    }
    if (Md <= 32) return launch_gemm<32, 128, 1, 4>(A, lda, W, ldw, bias, M, N, K, alpha, act, residual, out_bf16, out_f32, ldc, st);
    // mode 0: LDS-DMA staging when K % 64 == 0, 256x256 tiles for large problems (default); 1: force the
    // register-staged kernels; 2: LDS-DMA staging but no 256x256 tiles; 10..17: experimental ring variants
    // (A/B testing via devqa_gemm_set_mode / DEVQA_GEMM)
    // the LDS-DMA kernels use 16-byte epilogue accesses: need N, ldc multiples of 4 and 16-byte aligned pointers
    const bool vec_ok = (N % 4 == 0) && (ldc % 4 == 0) && ((((uintptr_t)out_f32) | ((uintptr_t)residual) | ((uintptr_t)bias)) & 15) == 0 &&
                        (((uintptr_t)out_bf16) & 7) == 0;
    const bool glds = (K % 64 == 0) && g_gemm_mode != 1 && vec_ok;
    if (glds && g_gemm_mode >= 20 && Md > 64)  // 256x256 ping-pong variants (gemm_bf16_pp.hip)
        return launch_gemm_pp(g_gemm_mode - 20, A, lda, W, ldw, bias, M, N, K, alpha, act, residual, out_bf16, out_f32, ldc, st);
    if (glds && g_gemm_mode >= 10 && Md > 64)  // experimental N-stage ring variants (gemm_bf16_pipe.hip)
        return launch_gemm_pipe(g_gemm_mode - 10, A, lda, W, ldw, bias, M, N, K, alpha, act, residual, out_bf16, out_f32, ldc, st);
    const long t128 = (long)((Md + 127) / 128) * ((N + 127) / 128);
    const long t256 = (long)((Md + 255) / 256) * ((N + 255) / 256);
    int variant;  // 1: 64x128, 2: 128x128, 3: 256x256 ping-pong (gemm_bf16_pp.hip; mode 3 = the simple 2-stage 256x256 ring)
    if (Md <= 64 || t128 < 384) variant = 1;
    else if (glds && g_gemm_mode != 2 && t256 >= 128) variant = 3;
    else variant = 2;
    if (!glds) {
        if (variant == 1)
            return launch_gemm<64, 128, 2, 2>(A, lda, W, ldw, bias, M, N, K, alpha, act, residual, out_bf16, out_f32, ldc, st);
        return launch_gemm<128, 128, 2, 2>(A, lda, W, ldw, bias, M, N, K, alpha, act, residual, out_bf16, out_f32, ldc, st);
    }
    const int ph = devqa_prof_begin(variant, st);
    int rc;
    if (variant == 1) rc = launch_gemm_glds_64x128(A, lda, W, ldw, bias, M, N, K, alpha, act, residual, out_bf16, out_f32, ldc, st);
    else if (variant == 2) rc = launch_gemm_glds_128x128(A, lda, W, ldw, bias, M, N, K, alpha, act, residual, out_bf16, out_f32, ldc, st);
    else if (g_gemm_mode == 3 || (int64_t)Md * lda * 2 >= (1ll << 32) || (int64_t)N * ldw * 2 >= (1ll << 32))  // mode 3: previous default
        rc = launch_gemm_pipe(7, A, lda, W, ldw, bias, M, N, K, alpha, act, residual, out_bf16, out_f32, ldc, st);
    else rc = launch_gemm_pp(2, A, lda, W, ldw, bias, M, N, K, alpha, act, residual, out_bf16, out_f32, ldc, st);
    devqa_prof_end(ph, 2.0 * (double)M * (double)N * (double)K, st);
    return rc;
}
