// The two ends of the sentence encoder (include/devqa_text.h): BertEmbeddings (gather + sum + LayerNorm in one pass) and the
// sentence pooling over packed rows.  Both are HBM-bound row kernels in the style of rowwise.hip: 16-byte fp32 accesses, one wave
// per row where a row reduction is needed; LDS only where the pooling kernel's row groups and its four waves' norms meet.
#include "common.h"
#include "../../include/devqa_text.h"

typedef __bf16 tx_bf16x2_t __attribute__((ext_vector_type(2)));
typedef float tx_f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t tx_pack2(float a, float b) {   // v_cvt_pk_bf16_f32: RNE, NaN stays NaN
    tx_f32x2_t f = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, tx_bf16x2_t));
}
__device__ __forceinline__ float4 tx_load4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 tx_load4(const bf16_t* p) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                       __uint_as_float(u.y & 0xffff0000u));
}

// ------------------------------------------------------------------------------------------
// Embedding + LayerNorm: one wave per row, the row in registers (NV float4 pieces per lane, D <= 256 * NV), the three table reads of
// a row issued before its first reduction.  Statistics as layernorm_kernel: mean, then the centred sum of squares.
// ------------------------------------------------------------------------------------------
#define TX_MAXV 16
template <typename T, int NV>
__global__ __launch_bounds__(256) void text_embed_ln_kernel(const int32_t* __restrict__ token, const int32_t* __restrict__ pos,
                                                            const T* __restrict__ word, const T* __restrict__ position,
                                                            const T* __restrict__ type0, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, int R, int D, int V, int P, float eps,
                                                            bf16_t* __restrict__ out_bf16, float* __restrict__ out_f32) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const int nv = D >> 2;
    int t = token[row], p = pos[row];
    t = t < 0 ? 0 : (t >= V ? V - 1 : t);      // the host has checked both; an index outside its table must still not leave it
    p = p < 0 ? 0 : (p >= P ? P - 1 : p);
    const T* wr = word + (int64_t)t * D;
    const T* pr = position + (int64_t)p * D;
    float4 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = i * 64 + lane;
        if (c < nv) {
            const float4 a = tx_load4(wr + c * 4), b = tx_load4(type0 + c * 4), e = tx_load4(pr + c * 4);
            v[i] = make_float4((a.x + b.x) + e.x, (a.y + b.y) + e.y, (a.z + b.z) + e.z, (a.w + b.w) + e.w);
        } else {
            v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);     // padding pieces are zero
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (i * 64 + lane < nv) {
            const float a = v[i].x - mean, b = v[i].y - mean, cc = v[i].z - mean, d = v[i].w - mean;
            q += (a * a + b * b) + (cc * cc + d * d);
        }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
    const float4* g4 = reinterpret_cast<const float4*>(gamma);
    const float4* b4 = reinterpret_cast<const float4*>(beta);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = i * 64 + lane;
        if (c < nv) {
            const float4 g = g4[c], b = b4[c];
            float4 o;
            o.x = (v[i].x - mean) * rstd * g.x + b.x;
            o.y = (v[i].y - mean) * rstd * g.y + b.y;
            o.z = (v[i].z - mean) * rstd * g.z + b.z;
            o.w = (v[i].w - mean) * rstd * g.w + b.w;
            if (out_f32) reinterpret_cast<float4*>(out_f32 + (int64_t)row * D)[c] = o;
            if (out_bf16) {
                uint2 pk;
                pk.x = tx_pack2(o.x, o.y);
                pk.y = tx_pack2(o.z, o.w);
                reinterpret_cast<uint2*>(out_bf16 + (int64_t)row * D)[c] = pk;
            }
        }
    }
}

template <typename T>
static int launch_text_embed_ln(const int32_t* token, const int32_t* pos, const T* word, const T* position, const T* type0,
                                const float* gamma, const float* beta, int R, int D, int V, int P, float eps, bf16_t* out_bf16,
                                float* out_f32, void* stream) {
    DEVQA_CHECK_ARG(token && pos && word && position && type0 && gamma && beta && (out_bf16 || out_f32), "text_embed_ln: null pointer");
    DEVQA_CHECK_SHAPE(R >= 0 && D > 0 && D % 4 == 0 && D <= 64 * 4 * TX_MAXV && V > 0 && P > 0,
                      "text_embed_ln: R=%d D=%d V=%d P=%d unsupported (D %% 4 == 0, D <= %d)", R, D, V, P, 64 * 4 * TX_MAXV);
    if (R == 0) return DEVQA_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((R + 3) / 4), block(256);
#define TX_ARGS token, pos, word, position, type0, gamma, beta, R, D, V, P, eps, out_bf16, out_f32
    const int nvl = (D / 4 + 63) / 64;      // float4 pieces per lane
    if (nvl <= 1) hipLaunchKernelGGL((text_embed_ln_kernel<T, 1>), grid, block, 0, st, TX_ARGS);
    else if (nvl <= 2) hipLaunchKernelGGL((text_embed_ln_kernel<T, 2>), grid, block, 0, st, TX_ARGS);
    else if (nvl <= 4) hipLaunchKernelGGL((text_embed_ln_kernel<T, 4>), grid, block, 0, st, TX_ARGS);
    else if (nvl <= 8) hipLaunchKernelGGL((text_embed_ln_kernel<T, 8>), grid, block, 0, st, TX_ARGS);
    else hipLaunchKernelGGL((text_embed_ln_kernel<T, 16>), grid, block, 0, st, TX_ARGS);
#undef TX_ARGS
    DEVQA_LAUNCH_CHECK("text_embed_ln");
    return DEVQA_OK;
}

extern "C" int devqa_text_embed_ln(const int32_t* token, const int32_t* pos, const devqa_bf16* word, const devqa_bf16* position,
                                   const devqa_bf16* type0, const float* gamma, const float* beta, int R, int D, int V, int P,
                                   float eps, devqa_bf16* out_bf16, float* out_f32, void* stream) {
    return launch_text_embed_ln<bf16_t>(token, pos, word, position, type0, gamma, beta, R, D, V, P, eps, out_bf16, out_f32, stream);
}
extern "C" int devqa_text_embed_ln_f32(const int32_t* token, const int32_t* pos, const float* word, const float* position,
                                       const float* type0, const float* gamma, const float* beta, int R, int D, int V, int P,
                                       float eps, devqa_bf16* out_bf16, float* out_f32, void* stream) {
    return launch_text_embed_ln<float>(token, pos, word, position, type0, gamma, beta, R, D, V, P, eps, out_bf16, out_f32, stream);
}

// ------------------------------------------------------------------------------------------
// Sentence pooling: one workgroup per sequence.  The 256 threads form G = 4 / 2 / 1 row groups of nvp = 64 / 128 / 256 column
// threads (nvp: the float4 column groups of a row, rounded up to whole waves), so that D = 384 keeps 192 threads busy instead of 96.
// Group g walks rows g, g + G, ... in ascending order; the G partial rows meet in LDS and group 0 combines them in group order, so a
// column's result has one summation order whatever the launch.  The squared norm goes lane -> wave (xor shuffles) -> the four
// waves through LDS, added in wave order.  The pooled row is written once unnormalised and rescaled by the thread that wrote it.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 pool_step(float4 a, float4 u, bool is_max) {
    if (is_max) return make_float4(fmaxf(a.x, u.x), fmaxf(a.y, u.y), fmaxf(a.z, u.z), fmaxf(a.w, u.w));
    return make_float4(a.x + u.x, a.y + u.y, a.z + u.z, a.w + u.w);
}
__global__ __launch_bounds__(256) void seq_pool_kernel(const float* __restrict__ x, const int32_t* __restrict__ seq_start,
                                                       const int32_t* __restrict__ seq_len, int R, int D, int mode, int normalize,
                                                       float* __restrict__ out) {
    __shared__ float part[4];
    __shared__ float4 acc[256];
    const int s = blockIdx.x;
    const int tid = threadIdx.x;
    const int nv = D >> 2;
    int r0 = seq_start[s], n = seq_len[s];
    if (r0 < 0) r0 = 0;
    if (n < 0) n = 0;
    if (r0 > R) r0 = R;
    if (n > R - r0) n = R - r0;                       // rows at or beyond R are not read
    const float4* base = reinterpret_cast<const float4*>(x + (int64_t)r0 * D);
    float4* orow = reinterpret_cast<float4*>(out + (int64_t)s * D);
    const float inv_len = 1.f / fmaxf((float)n, 1e-9f);
    const bool is_max = mode == DEVQA_POOL_MAX;
    const float fill = is_max ? -INFINITY : 0.f;
    const int nvp = (nv + 63) & ~63;
    const int G = nvp <= 64 ? 4 : (nvp <= 128 ? 2 : 1);          // uniform over the workgroup
    float sq = 0.f;
    if (G == 1) {                                                // wide rows: thread t owns the column groups t, t + 256, ...
        for (int c = tid; c < nv; c += 256) {
            float4 a = make_float4(fill, fill, fill, fill);
            if (mode == DEVQA_POOL_CLS) {
                if (n > 0) a = base[c];
            } else {
                for (int r = 0; r < n; ++r) a = pool_step(a, base[(int64_t)r * nv + c], is_max);
                if (!is_max) { a.x *= inv_len; a.y *= inv_len; a.z *= inv_len; a.w *= inv_len; }
            }
            orow[c] = a;
            sq += (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w);
        }
    } else {
        const int g = tid / nvp, c = tid - g * nvp;              // G * nvp == 256: every thread has a group
        const bool live = c < nv;
        float4 a = make_float4(fill, fill, fill, fill);
        if (live && mode != DEVQA_POOL_CLS)
            for (int r = g; r < n; r += G) a = pool_step(a, base[(int64_t)r * nv + c], is_max);
        acc[tid] = a;
        __syncthreads();
        if (g == 0 && live) {
            if (mode == DEVQA_POOL_CLS) {
                if (n > 0) a = base[c];
            } else {
                for (int k = 1; k < G; ++k) a = pool_step(a, acc[k * nvp + c], is_max);
                if (!is_max) { a.x *= inv_len; a.y *= inv_len; a.z *= inv_len; a.w *= inv_len; }
            }
            orow[c] = a;
            sq = (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w);
        }
    }
    if (!normalize) return;                            // uniform over the workgroup
    sq = wave_sum(sq);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sq;
    __syncthreads();
    const float norm = sqrtf((part[0] + part[1]) + (part[2] + part[3]));
    const float inv = n > 0 ? 1.f / fmaxf(norm, 1e-12f) : 1.f;     // an empty sequence keeps its fill (zeros, or -inf for max): no -inf * 0
    for (int c = tid; c < nv; c += 256) {             // the column groups this thread wrote above (G > 1: threads 0 .. nv - 1)
        float4 a = orow[c];
        a.x *= inv; a.y *= inv; a.z *= inv; a.w *= inv;
        orow[c] = a;
    }
}

extern "C" int devqa_seq_pool(const float* x, const int32_t* seq_start, const int32_t* seq_len, int R, int S, int D, int mode,
                              int normalize, float* out, void* stream) {
    DEVQA_CHECK_ARG(x && seq_start && seq_len && out, "seq_pool: null pointer");
    DEVQA_CHECK_ARG(mode == DEVQA_POOL_MEAN || mode == DEVQA_POOL_CLS || mode == DEVQA_POOL_MAX, "seq_pool: unknown mode %d", mode);
    DEVQA_CHECK_SHAPE(R >= 0 && S >= 0 && D > 0 && D % 4 == 0, "seq_pool: R=%d S=%d D=%d unsupported (D %% 4 == 0)", R, S, D);
    if (S == 0) return DEVQA_OK;
    hipLaunchKernelGGL(seq_pool_kernel, dim3(S), dim3(256), 0, (hipStream_t)stream, x, seq_start, seq_len, R, D, mode, normalize, out);
    DEVQA_LAUNCH_CHECK("seq_pool");
    return DEVQA_OK;
}
