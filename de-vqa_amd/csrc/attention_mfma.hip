// MFMA flash attention for the packed varlen descriptor of include/devqa.h (bf16 in/out, fp32
// softmax statistics and accumulation).  ViT (257x257, dh 88), Q-Former (32x32 / 32x257, dh 64) and
// OPT (causal + visible prefix, dh 80) all go through this kernel.
//
// Workgroup = (sequence, head, 64-query tile); 4 waves x 16 query rows; keys stream through a double-buffered LDS image in
// 64-key chunks (K and V row-major [64][DHP] bf16, rows padded so that both the ds_read_b128 K-fragment reads and the
// ds_read_b64_tr_b16 V reads are conflict-free), one barrier per chunk.
//
// Operand orientation (no LDS round trip for P, no transposed V image):
//   S^T = K . Q^T   -> a lane's 16x16 accumulator holds, for ONE query (lane&15), the keys
//                      16t + 4*(lane>>4) + r of key tile t  -> softmax row statistics need only two
//                      cross-lane steps (xor 16, 32);
//   O^T = V^T . P^T -> the same registers, converted to bf16, ARE the B operand (n = query) of that product if the
//                      k index of the MFMA enumerates keys in the order (tile 2s, r=0..3, tile 2s+1,
//                      r=0..3) for lane group lane>>4; the matching A operand (m = channel) is read from the row-major V
//                      image with ds_read_b64_tr_b16 (4 keys x 16 channels per 16-lane group).  The accumulator then holds,
//                      for the lane's OWN query, 4 consecutive channels per 16-channel tile: the rescale factor and the
//                      normaliser never cross lanes and the output leaves in 8-byte packed stores.
// head dims that are not multiples of 32 (88, 80) are zero-padded in LDS to DHP = 96.
#include <stdlib.h>
#include <atomic>
#include <mutex>
#include "common.h"
#include <type_traits>

typedef __attribute__((ext_vector_type(4))) short short4_t;
typedef __attribute__((address_space(3))) short4_t* lds_s4_ptr;

typedef __bf16 am_bf16x2_t __attribute__((ext_vector_type(2)));
typedef float am_f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t am_pack2(float a, float b) {   // v_cvt_pk_bf16_f32 (RNE)
    am_f32x2_t f = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, am_bf16x2_t));
}

#define AM_KC 64  // keys per chunk
#define AM_QT 64  // queries per workgroup of the register-staged kernel (4 waves x 16 queries)

// Reductions over the 4 lanes {fr, fr + 16, fr + 32, fr + 48} that hold one query's scores, on the VALU: gfx950's
// v_permlane16_swap / v_permlane32_swap exchange 16- / 32-lane halves between two registers, so a butterfly step is one swap + one
// op instead of a ds_bpermute round trip through the LDS crossbar (8 of those sat on every chunk's critical path).
// (Inline asm: clang 22 folds op(r[0], r[1]) of __builtin_amdgcn_permlane{16,32}_swap's two results into r[0] alone.)
__device__ __forceinline__ void am_swap16(float x, float& a, float& b) {
    asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %2\n\ts_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "=&v"(a), "=&v"(b) : "v"(x));
}
__device__ __forceinline__ void am_swap32(float x, float& a, float& b) {
    asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %2\n\ts_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "=&v"(a), "=&v"(b) : "v"(x));
}
// max of the 16 scores a lane holds after the S^T MFMAs, as ONE asm block: 7 v_max3_f32 + 1 v_max_f32 without the v_max_f32 x, x
// canonicalisation clang puts in front of every fmaxf operand that comes out of an MFMA (IEEE sNaN quieting; scores are finite or
// -inf here).  The block opens with wait states: on gfx9 a VALU read of an MFMA result is a SOFTWARE-managed hazard, which the
// compiler resolves for its own instructions but not for inline asm -- an unprotected v_max3 here read stale accumulators now and
// then (run-to-run differences at rounding level, since softmax is invariant to its reference point; found by
// tools/debug/att_determinism.py).  12 wait states cover the 4-pass v_mfma_f32_16x16x32_bf16.
__device__ __forceinline__ float am_max16(const float4_t& a, const float4_t& b, const float4_t& c, const float4_t& d) {
    float r;
    asm volatile("s_nop 11\n\t"
                 "v_max3_f32 %0, %1, %2, %3\n\t"
                 "v_max3_f32 %0, %0, %4, %5\n\t"
                 "v_max3_f32 %0, %0, %6, %7\n\t"
                 "v_max3_f32 %0, %0, %8, %9\n\t"
                 "v_max3_f32 %0, %0, %10, %11\n\t"
                 "v_max3_f32 %0, %0, %12, %13\n\t"
                 "v_max3_f32 %0, %0, %14, %15\n\t"
                 "v_max_f32 %0, %0, %16"
                 : "=&v"(r)
                 : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]), "v"(c[0]), "v"(c[1]), "v"(c[2]),
                   "v"(c[3]), "v"(d[0]), "v"(d[1]), "v"(d[2]), "v"(d[3]));
    return r;
}
__device__ __forceinline__ float am_max4(float x) {
    float a, b;
    am_swap16(x, a, b);
    x = fmaxf(a, b);
    am_swap32(x, a, b);
    return fmaxf(a, b);
}
__device__ __forceinline__ float am_sum4(float x) {
    float a, b;
    am_swap16(x, a, b);
    x = a + b;
    am_swap32(x, a, b);
    return a + b;
}

// blockIdx -> (sequence, head, q tile).  The hardware deals workgroups round-robin to the 8 XCDs (blockIdx % 8), each with its own L2.  The q
// tiles of one (sequence, head) GROUP share K / V, and the heads of one sequence share cache lines (adjacent column slices of the same rows),
// so a UNIT of `unit` consecutive groups stays on one XCD and consecutive units go to consecutive XCDs: a unit is n_seq / 64 whole sequences
// (~64 units per launch: enough to balance 8 XCDs, and the sequences of one edit+eval cycle -- an image prefix and the texts that read its K / V
// -- stay together: dealing single sequences round-robin cost the BLIP-2 + MEND_VL config 13 %), one group when there are few sequences.  (Round 2 gave every XCD one contiguous RANGE of groups: in a mixed pack
// -- LLaVA's decoder: 64 prefix sequences of 577 rows first, 192 probe texts of ~20 rows after -- two XCDs then carried all the long
// sequences: 2649 us against 886 us for the same work, tools/debug/att_llava_bench.py.)
// The grid is 8 * ceil(units / 8) * unit * q_tiles workgroups; ids past the last group exit.
__host__ __device__ __forceinline__ int am_unit(int n_seq, int H) { return n_seq >= 32 ? (n_seq >= 128 ? n_seq / 64 : 1) * H : 1; }
__device__ __forceinline__ bool am_remap(int b, int q_tiles, int n_seq, int H, int& bid) {
    if (n_seq < 0) {        // (-n_seq: the round-2 mapping, one contiguous range of ids per XCD; grid = groups * q_tiles exactly)
        const int nwg = gridDim.x, qq = nwg >> 3, rr = nwg & 7, xcd = b & 7, idx = b >> 3;
        bid = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + idx;
        return true;
    }
    const int unit = am_unit(n_seq, H);
    const int per = unit * q_tiles;                 // workgroups of a unit
    const int xcd = b & 7, idx = b >> 3;
    const int ul = idx / per, in_u = idx - ul * per;
    const int g = (ul * 8 + xcd) * unit + in_u / q_tiles;
    bid = g * q_tiles + in_u % q_tiles;
    return g < n_seq * H;
}

// ---- register-staged kernel: 64-query tiles of 4 waves, K / V chunks global -> registers -> ONE LDS image (sequences below 224 rows) ----
template <int DHP>
__global__ __launch_bounds__(4 * 64, 2) void attention_mfma_kernel(const bf16_t* __restrict__ q, int64_t ldq,
                                                             const bf16_t* __restrict__ k, int64_t ldk,
                                                             const bf16_t* __restrict__ v, int64_t ldv,
                                                             bf16_t* __restrict__ out, int64_t ldo,
                                                             const int32_t* __restrict__ seq_desc, int H, int dh,
                                                             float scale, int causal, int q_tiles, int n_seq) {
    // bytes per LDS row: the padding makes 8 consecutive rows start in 8 different 4-bank groups (ds_read_b128 K fragments,
    // ds_write_b128 staging) and 4 consecutive rows in 4 different 8-bank groups (ds_read_b64_tr_b16 V fragments); 32 bytes do
    // that for every row size.
    constexpr int STRIDE = 2 * DHP + 32;
    constexpr int KS = DHP / 32;          // k-steps of the S^T product
    constexpr int DT = DHP / 16;          // 16-channel output tiles
    constexpr int BUF = AM_KC * STRIDE;   // one chunk image
    constexpr int NT = 4 * 64;            // threads per workgroup
    constexpr int QT = AM_QT;             // queries per workgroup
    // ONE image per operand, two barriers per chunk (all reads done -> refill -> visible); the next chunk waits in registers meanwhile.
    // Measured on ViT-g (tools/attention_bench.py): 184.8 us against 199.3 us for a double-buffered image with one barrier per chunk --
    // the refill of the next chunk right behind the barrier competes with the K-fragment reads that open the compute segment.
    __shared__ __attribute__((aligned(16))) unsigned char Kimg[BUF];
    __shared__ __attribute__((aligned(16))) unsigned char Vimg[BUF];

    int bid;
    if (!am_remap(blockIdx.x, q_tiles, n_seq, H, bid)) return;
    const int qt = bid % q_tiles;
    const int h = (bid / q_tiles) % H;
    const int s = bid / (q_tiles * H);
    const int32_t* d = seq_desc + s * 6;
    const int q_start = d[0], q_len = d[1], kp_start = d[2], kp_len = d[3], ko_start = d[4], ko_len = d[5];
    const int q0 = qt * QT;
    if (q0 >= q_len) return;  // uniform per workgroup
    const int nq = min(QT, q_len - q0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int causal_off = ko_len - q_len;  // query i sees own keys 0..i+causal_off
    const int own_hi = causal ? max(0, min(ko_len, q0 + nq + causal_off)) : ko_len;
    const int n_keys = kp_len + own_hi;

    // ---- Q fragments (B operand of S^T = K.Q^T): query row = wave*16 + fr, channels 32ks + 8fq .. +8 ----
    const int qrow = q0 + wave * 16 + fr;  // (index inside the sequence)
    short8_t qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int c = ks * 32 + fq * 8;
        uint4 u = make_uint4(0, 0, 0, 0);
        if (qrow < q_len && c < dh) u = *reinterpret_cast<const uint4*>(q + (int64_t)(q_start + qrow) * ldq + h * dh + c);
        qf[ks] = *reinterpret_cast<short8_t*>(&u);
    }

    float4_t o[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i) o[i] = (float4_t){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;  // statistics of query fr (replicated over the 4 lane groups)
    const float sc2 = scale * 1.44269504088896340736f;

    constexpr int CH = DHP / 8;  // 16-byte chunks per row
    constexpr int LD = AM_KC * CH / NT;  // 16-byte pieces of K (and of V) per thread and chunk
    static_assert(AM_KC * CH % NT == 0, "chunk must split evenly over the workgroup");
    typedef unsigned am_u32x4_t __attribute__((ext_vector_type(4)));   // (a struct uint4 copied straight from global memory is not
    am_u32x4_t kreg[LD], vreg[LD];                                     //  promoted out of scratch by this compiler)
    // loop-invariant part of this thread's LD staging pieces: LDS offset, channel base pointers, row inside the chunk.  The loads are
    // UNPREDICATED: a row past the last key re-reads the last key (its scores are masked to -inf and p = 0 multiplies a finite V row),
    // a 16-byte piece in the channel padding (dh..DHP) re-reads the last 8 real channels (K: multiplied by Q's zero padding; V: lands
    // in output columns >= dh, which are never stored) -- no exec-masked branches around 2 x LD loads per chunk.
    int st_off[LD], st_row[LD], st_col[LD];
#pragma unroll
    for (int j = 0; j < LD; ++j) {
        const int i = tid + j * NT;
        const int r = i / CH, cv = i - r * CH;
        st_row[j] = r;
        st_off[j] = r * STRIDE + cv * 16;
        st_col[j] = h * dh + min(cv * 8, dh - 8);
    }
#define AM_FETCH(C0)                                                                                                        \
    _Pragma("unroll") for (int j = 0; j < LD; ++j) {                                                                        \
        const int kidx = min((C0) + st_row[j], n_keys - 1);                                                                 \
        const int64_t grow = (kidx < kp_len) ? (int64_t)(kp_start + kidx) : (int64_t)(ko_start + kidx - kp_len);            \
        kreg[j] = *reinterpret_cast<const am_u32x4_t*>(k + grow * ldk + st_col[j]);                                         \
        vreg[j] = *reinterpret_cast<const am_u32x4_t*>(v + grow * ldv + st_col[j]);                                         \
    }
    // Fast form for chunks that lie entirely inside ONE contiguous key range -- the own range of a sequence without a visible
    // prefix, or a visible range alone (every ViT / Q-Former chunk but the last): uniform 64-bit base (SGPRs) + a per-thread 32-bit
    // element offset fixed for the whole loop -> `global_load_dwordx4 v, voff, s[base]` with NO per-chunk vector address arithmetic.
    // (The general form above spends ~50 VALU instructions per chunk on it, 18 of them quarter-rate 32x32 multiplies -- as many
    // cycles as the softmax itself.)
    const bool one_range = kp_len == 0 || own_hi == 0;       // all keys of this tile come from ONE contiguous row range
    const bool fast_rows = one_range && (int64_t)(AM_KC - 1) * max(ldk, ldv) + h * dh + DHP < (1ll << 31);
    uint32_t fk_off[LD], fv_off[LD];
#pragma unroll
    for (int j = 0; j < LD; ++j) {
        fk_off[j] = (uint32_t)(st_row[j] * (int)ldk + st_col[j]);
        fv_off[j] = (uint32_t)(st_row[j] * (int)ldv + st_col[j]);
    }
    const bf16_t* const k_own = k + (int64_t)(kp_len == 0 ? ko_start : kp_start) * ldk;
    const bf16_t* const v_own = v + (int64_t)(kp_len == 0 ? ko_start : kp_start) * ldv;
#define AM_FETCH_ANY(C0)                                                                                                    \
    if (fast_rows && (C0) + AM_KC <= n_keys) {                                                                              \
        const bf16_t* kb = k_own + (int64_t)(C0) * ldk;                                                                     \
        const bf16_t* vb = v_own + (int64_t)(C0) * ldv;                                                                     \
        _Pragma("unroll") for (int j = 0; j < LD; ++j) {                                                                    \
            kreg[j] = *reinterpret_cast<const am_u32x4_t*>(kb + fk_off[j]);                                                 \
            vreg[j] = *reinterpret_cast<const am_u32x4_t*>(vb + fv_off[j]);                                                 \
        }                                                                                                                   \
    } else { AM_FETCH(C0) }
    const bool wave_has_rows = q0 + wave * 16 < q_len;  // waves without a query still stage K/V and hit the barriers
#define AM_PARK()                                                                                                           \
    _Pragma("unroll") for (int j = 0; j < LD; ++j) {                                                                        \
        *reinterpret_cast<am_u32x4_t*>(Kimg + st_off[j]) = kreg[j];                                                         \
        *reinterpret_cast<am_u32x4_t*>(Vimg + st_off[j]) = vreg[j];                                                         \
    }
    if (n_keys > 0) {
        AM_FETCH_ANY(0)
        AM_PARK()
        if (AM_KC < n_keys) { AM_FETCH_ANY(AM_KC) }
    }
    for (int c0 = 0; c0 < n_keys; c0 += AM_KC) {
        __syncthreads();                // chunk 0 (parked by the prologue) is visible / the previous chunk is consumed
        if (c0 > 0) {
            AM_PARK()
            __syncthreads();
            if (c0 + AM_KC < n_keys) { AM_FETCH_ANY(c0 + AM_KC) }  // next chunk's loads fly under this chunk's MFMAs
        }
        if (!wave_has_rows) continue;
        const unsigned char* Ks = Kimg;     // (the body reads through these locals: naming the arrays in it compiles to another schedule)
        const unsigned char* Vs = Vimg;
        // FULL chunks (64 keys, none hidden by the causal rule) take a branch-free instantiation of the body
        auto body = [&](auto full_tag) {
            constexpr bool FULLC = decltype(full_tag)::value;
        const int nt = FULLC ? 4 : min(4, (n_keys - c0 + 15) >> 4);  // 16-key tiles of this chunk that hold a key (uniform)

            // ---- S^T tiles: keys 16t + (4fq + r), query fr ----
            float4_t st[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                st[t] = (float4_t){0.f, 0.f, 0.f, 0.f};
                if (!FULLC && t >= nt) continue;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const short8_t kf = *reinterpret_cast<const short8_t*>(Ks + (16 * t + fr) * STRIDE + (32 * ks + 8 * fq) * 2);
                    st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], st[t], 0, 0, 0);
                }
            }
            // ---- mask, online softmax for query fr.  Scores stay unscaled: with c = scale * log2(e) > 0,
            // softmax(scale * s) = exp2(c * s - c * max s); masking is needed only in chunks that hold a key past the end
            // or a causally hidden key (uniform per workgroup) ----
            const bool need_mask = !FULLC && ((c0 + AM_KC > n_keys) || (causal && c0 + AM_KC > kp_len));
            float mloc;
            if (FULLC) {
                mloc = am_max16(st[0], st[1], st[2], st[3]);
            } else {
                // only the nt (wave-uniform) key tiles that hold a key are touched; the others keep st = 0, which IS their p
                mloc = -INFINITY;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (t >= nt) continue;
                    if (need_mask) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int kidx = c0 + 16 * t + 4 * fq + r;
                            bool ok = kidx < n_keys;
                            if (causal && kidx >= kp_len) ok = ok && (kidx - kp_len) <= qrow + causal_off;
                            st[t][r] = ok ? st[t][r] : -INFINITY;
                        }
                    }
                    mloc = fmaxf(fmaxf(mloc, fmaxf(st[t][0], st[t][1])), fmaxf(st[t][2], st[t][3]));   // compiler-scheduled
                }
            }
            mloc = am_max4(mloc);
            float m_new = fmaxf(m_run, mloc);                   // running max of the UNSCALED scores
            // Lazy rescale: the reference point of the exponentials only has to be CLOSE to the running max.  Unless some query
            // of this wave saw its max grow by more than 2^8 (always true for a query's first visible keys), every lane keeps
            // its previous reference: p <= 256 is harmless in bf16 / fp32, l and O stay consistent, and the alpha broadcast
            // (4 cross-lane gathers) plus the O rescale are skipped for the chunk.
            const bool grow = (m_new - m_run) * sc2 > 8.f;      // m_run = -inf, m_new finite -> true; both -inf -> NaN -> false
            const bool rescale = __builtin_amdgcn_ballot_w64(grow) != 0;   // wave-uniform
            if (!rescale) m_new = m_run;
            float alpha = 1.f, lloc = 0.f;
            if (FULLC || m_new != -INFINITY) {   // a full chunk shows 64 valid, visible keys to every query: m_new is finite
                const float mc = m_new * sc2;
                if (rescale) alpha = __builtin_amdgcn_exp2f(m_run * sc2 - mc);   // m_run = -inf -> 0
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (!FULLC && t >= nt) continue;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float p = __builtin_amdgcn_exp2f(fmaf(st[t][r], sc2, -mc));   // masked (-inf) -> 0
                        st[t][r] = p;
                        lloc += p;
                    }
                }
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) st[t] = (float4_t){0.f, 0.f, 0.f, 0.f};
            }
            lloc = am_sum4(lloc);
            l_run = l_run * alpha + lloc;
            m_run = m_new;
            // ---- P fragments (A operand of O = P.V): k order = (tile 2s: r 0..3, tile 2s+1: r 0..3) ----
            short8_t pf[2];
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                uint4 u;
                u.x = am_pack2(st[2 * s2][0], st[2 * s2][1]);
                u.y = am_pack2(st[2 * s2][2], st[2 * s2][3]);
                u.z = am_pack2(st[2 * s2 + 1][0], st[2 * s2 + 1][1]);
                u.w = am_pack2(st[2 * s2 + 1][2], st[2 * s2 + 1][3]);
                pf[s2] = *reinterpret_cast<short8_t*>(&u);
            }
            // ---- rescale O^T: its COLUMN is query fr, the query whose alpha this lane already holds ----
            if (rescale) {
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
            }
            // ---- O^T += V^T.P^T: the transposed LDS reads of the row-major V image deliver, for channel fr' and key group fq, the
            // 8 keys of a k-step -- that is the A operand (m = channel) as well as the B operand (n = channel) layout; with P as
            // the B operand (n = query fr, same registers as before) the accumulator tile is O^T: row = channel 16dt + 4fq + r,
            // column = query fr.  Every per-query quantity (alpha, l) then lives in the lane that needs it, and a lane owns 4
            // CONSECUTIVE channels of its query: 8-byte packed stores instead of 2-byte ones. ----
            const int tq = fr >> 2, tp = fr & 3;  // lane 4q+p of a 16-lane group addresses row q, columns 4p..4p+3
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    if (!FULLC && 2 * s2 >= nt) continue;   // both key tiles of this k-step are past the last key (P = 0 there)
                    const short4_t b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (lds_s4_ptr)(Vs + (16 * (2 * s2) + 4 * fq + tq) * STRIDE + (16 * dt + 4 * tp) * 2));
                    const short4_t b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (lds_s4_ptr)(Vs + (16 * (2 * s2 + 1) + 4 * fq + tq) * STRIDE + (16 * dt + 4 * tp) * 2));
                    const short8_t vf = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[s2], o[dt], 0, 0, 0);
                }
            }
        };
        // ... also causal chunks that lie entirely at or below the diagonal of this tile's FIRST query (visible to all its rows)
        const bool all_visible = !causal || c0 + AM_KC <= kp_len || (c0 + AM_KC - 1 - kp_len) <= q0 + causal_off;
        if (c0 + AM_KC <= n_keys && all_visible) body(std::true_type{}); else body(std::false_type{});
    }

    // ---- normalise and store: O^T row = channel 16dt + 4fq + r, column = query fr ----
    // (a one-trip loop on purpose: behind a plain `if` or an early return the same statements change the register allocation of the whole kernel)
#pragma unroll
    for (int once = 0; once < 1; ++once) {
        if (qrow >= q_len) continue;
        const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
        bf16_t* orow = out + (int64_t)(q_start + qrow) * ldo + h * dh;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const int c = 16 * dt + 4 * fq;
            if (c < dh) {      // dh % 8 == 0: a lane's 4 channels are all inside or all outside
                uint2 u;
                u.x = am_pack2(o[dt][0] * inv, o[dt][1] * inv);
                u.y = am_pack2(o[dt][2] * inv, o[dt][3] * inv);
                *reinterpret_cast<uint2*>(orow + c) = u;
            }
        }
    }
}

// ---- LDS-DMA staged variant (the default) ----------------------------------------------------------------------------------------
// Same tiling, operand orientation, softmax and results as attention_mfma_kernel<DHP>, different K / V staging: timing-only
// variants of that kernel (since removed; profiles/r02_summary.md) showed that on ViT-g neither the softmax
// VALU work (no exp: +-0 %) nor the barriers (-3 %) bound it but the global -> register -> ds_write_b128 staging of every chunk
// (-24 % without the loads, -39 % without loads and LDS stores).  Here every wave moves its share of the next chunk with
// `global_load_lds_dwordx4` (no staging VGPRs, no LDS store instructions; 64 lanes x 16 B land at consecutive LDS addresses), into the
// other half of a double-buffered image, one barrier per chunk.  The DMA fixes the image layout to plain row-major pieces
// (piece p of 16 bytes at byte 16 p, CH = DHP / 8 pieces per key row, no row padding), so bank conflicts are avoided by a
// source-side permutation instead: LDS position (row R, piece c') holds global piece c' ^ x(R), with x(R) = (R >> 1) & 3 for 4 / 12
// pieces per row, R & 7 for 8, 2R & 15 for 16 -- found by simulating the guide's bank rules for ds_read_b128 (K fragments, 4 x 16
// lane groups) and ds_read_b64_tr_b16 (V fragments, 2 x 32): conflict-free for both images (tools/debug/lds_swizzle_search.py).
typedef __attribute__((address_space(1))) const void* am_gptr_t;
typedef __attribute__((address_space(3))) void* am_lptr_t;
template <int CH>
__device__ __forceinline__ int am_swz(int R) {
    return CH == 8 ? (R & 7) : CH == 16 ? ((2 * R) & 15) : ((R >> 1) & 3);
}

// SB (single-buffered, NW = 2: 32-query tiles) is the form for packs of SHORT sequences (the decoder pack of the edit+eval path: 32 image
// tokens or <= ~25 text tokens per sequence behind a 32-key visible prefix, one or two chunks each): nothing to overlap a second image with,
// so one image (24 KiB at dh 80: 6 workgroups per CU instead of 3) and two waves per (sequence, head) double the pairs in flight per CU.
// Four V^T fragments (ds_read_b64_tr_b16 at byte offsets O0..O3 from one lane address) as ONE asm block that ends with its own lgkmcnt(0).
// Why not the builtin: the compiler cannot tell which LDS-DMA write a transposing read may alias and puts `s_waitcnt vmcnt(0)` in front of
// every one of them -- the P.V half of a round then waits for the chunk just put in flight, i.e. the prefetch overlapped the S = K.Q^T
// half only (seen in the ISA of every instantiation of the kernel below; the plain ds_read_b128 K reads get no such wait).  An asm read is
// invisible to that pass; the DMA / read ordering is the kernel's own (vmcnt + barrier per round).
template <int O0, int O1, int O2, int O3>
__device__ __forceinline__ void am_tr_read4(uint32_t addr, short4_t& a, short4_t& b, short4_t& c, short4_t& d) {
    asm volatile("ds_read_b64_tr_b16 %0, %4 offset:%5\n\t"
                 "ds_read_b64_tr_b16 %1, %4 offset:%6\n\t"
                 "ds_read_b64_tr_b16 %2, %4 offset:%7\n\t"
                 "ds_read_b64_tr_b16 %3, %4 offset:%8\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(d)
                 : "v"(addr), "n"(O0), "n"(O1), "n"(O2), "n"(O3)
                 : "memory");
}
template <int O0, int O1>
__device__ __forceinline__ void am_tr_read2(uint32_t addr, short4_t& a, short4_t& b) {
    asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%3\n\t"
                 "ds_read_b64_tr_b16 %1, %2 offset:%4\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(a), "=&v"(b)
                 : "v"(addr), "n"(O0), "n"(O1)
                 : "memory");
}
// lane id behind an asm the optimiser cannot hoist: per-DMA row / column arithmetic stays in the chunk loop instead of becoming (spilled) lane constants
__device__ __forceinline__ int am_lane_opaque() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
// dot product of 8 bf16 pairs (a MFMA operand fragment against 16 bytes of a row) on the VALU, fp32 accumulate
__device__ __forceinline__ float am_dot8(const short8_t& a, const uint4& b, float acc) {
    const uint4 ua = *reinterpret_cast<const uint4*>(&a);
    const uint32_t aw[4] = {ua.x, ua.y, ua.z, ua.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        acc = fmaf(__uint_as_float(aw[i] << 16), __uint_as_float(bw[i] << 16), acc);
        acc = fmaf(__uint_as_float(aw[i] & 0xffff0000u), __uint_as_float(bw[i] & 0xffff0000u), acc);
    }
    return acc;
}

template <int DHP, int NW, bool SB = false>
__global__ __launch_bounds__(64 * NW, ((NW == 8 && DHP <= 96) || SB) ? 4 : 2) void attention_mfma_dma_kernel(const bf16_t* __restrict__ q, int64_t ldq,
                                                                 const bf16_t* __restrict__ k, int64_t ldk,
                                                                 const bf16_t* __restrict__ v, int64_t ldv,
                                                                 bf16_t* __restrict__ out, int64_t ldo,
                                                                 const int32_t* __restrict__ seq_desc, int H, int dh,
                                                                 float scale, int causal, int q_tiles, int n_seq) {
    constexpr int ROWB = 2 * DHP;          // bytes per key row in LDS (unpadded)
    constexpr int KS = DHP / 32;
    constexpr int DT = DHP / 16;
    constexpr int CH = DHP / 8;            // 16-byte pieces per row
    constexpr int IMG = AM_KC * ROWB;      // one chunk image
    constexpr int NI = AM_KC * CH / 64;    // DMA instructions (64 lanes x 16 B) per image and chunk
    constexpr int LD = 2 * NI / NW;        // ... per wave and chunk, K and V images together: instruction j * NW + wave of the list K | V
    constexpr int QT = 16 * NW;            // queries per workgroup
    static_assert(2 * NI % NW == 0, "chunk must split evenly over the waves");
    __shared__ __attribute__((aligned(1024))) unsigned char Ks2[(SB ? 1 : 2) * IMG];
    __shared__ __attribute__((aligned(1024))) unsigned char Vs2[(SB ? 1 : 2) * IMG];

    int bid;
    if (!am_remap(blockIdx.x, q_tiles, n_seq, H, bid)) return;
    const int qt = bid % q_tiles;
    const int h = (bid / q_tiles) % H;
    const int s = bid / (q_tiles * H);
    const int32_t* d = seq_desc + s * 6;
    const int q_start = d[0], q_len = d[1], kp_start = d[2], kp_len = d[3], ko_start = d[4], ko_len = d[5];
    const int q0 = qt * QT;
    if (q0 >= q_len) return;  // uniform per workgroup
    const int nq = min(QT, q_len - q0);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    const int causal_off = ko_len - q_len;
    const int own_hi = causal ? max(0, min(ko_len, q0 + nq + causal_off)) : ko_len;
    const int n_keys = kp_len + own_hi;

    const int qrow = q0 + wave * 16 + fr;
    short8_t qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int c = ks * 32 + fq * 8;
        uint4 u = make_uint4(0, 0, 0, 0);
        if (qrow < q_len && c < dh) u = *reinterpret_cast<const uint4*>(q + (int64_t)(q_start + qrow) * ldq + h * dh + c);
        qf[ks] = *reinterpret_cast<short8_t*>(&u);
    }
    float4_t o[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i) o[i] = (float4_t){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    const float sc2 = scale * 1.44269504088896340736f;
    // ---- staging: DMA instruction j of this wave fills LDS bytes [(j * 4 + wave) * 1024, + 1024) of an image ----
    // SB: the K and the V piece j, j + LD / 2 of a wave are the same block of their images (LD / 2 * NW == NI), so their row / column
    // constants are kept once and the fast path's element offset is formed at use (two waves per workgroup: registers, not issue slots,
    // bound how many of them a CU holds)
    constexpr int LDH = SB ? LD / 2 : LD;
    static_assert(!SB || (LD % 2 == 0 && (LD / 2 * NW) % NI == 0), "K / V pieces of a wave must pair up");
    int st_row[LDH], st_col[LDH];
    uint32_t f_off[SB ? 1 : LD];
#pragma unroll
    for (int j = 0; j < LDH; ++j) {
        const int blk = (j * NW + wave) % NI;                 // 1-KiB block of its image (wave-uniform, as is the image)
        const int p = blk * 64 + lane;
        const int R = p / CH, cp = p - R * CH;
        const int c = cp ^ am_swz<CH>(R);
        st_row[j] = R;
        st_col[j] = h * dh + min(c * 8, dh - 8);     // channel padding re-reads the last real channels (see the kernel above)
    }
    if constexpr (!SB) {
#pragma unroll
        for (int j = 0; j < LD; ++j) {
            const bool is_v = (j * NW + wave) >= NI;
            f_off[j] = (uint32_t)(st_row[j] * (int)(is_v ? ldv : ldk) + st_col[j]);
        }
    }
    const bool one_range = kp_len == 0 || own_hi == 0;
    const bool fast_rows = one_range && (int64_t)(AM_KC - 1) * max(ldk, ldv) + h * dh + DHP < (1ll << 31);
    const bf16_t* const k_own = k + (int64_t)(kp_len == 0 ? ko_start : kp_start) * ldk;
    const bf16_t* const v_own = v + (int64_t)(kp_len == 0 ? ko_start : kp_start) * ldv;
#define AMD_STAGE(C0, BUFI)                                                                                                  \
    _Pragma("unroll") for (int j = 0; j < LD; ++j) {                                                                        \
        const int blk = (j * NW + wave) % NI;                                                                               \
        const bool is_v = (j * NW + wave) >= NI;                                                                            \
        if (blk * 64 / CH >= ((n_keys - (C0) + 31) & ~31)) continue;   /* a last, partial chunk: only the 32-key k-steps of P.V that hold a key (their rows must be finite: p = 0 multiplies them) */ \
        unsigned char* dst = (is_v ? Vs2 : Ks2) + (BUFI) * IMG + blk * 1024;                                                \
        const int64_t ld = is_v ? ldv : ldk;                                                                                \
        const int jj = SB ? j % LDH : j;                                                                                    \
        if (fast_rows && (C0) + AM_KC <= n_keys) {                                                                          \
            const bf16_t* gb = (is_v ? v_own : k_own) + (int64_t)(C0) * ld;                                                 \
            const uint32_t fo = SB ? (uint32_t)(st_row[jj] * (int)ld + st_col[jj]) : f_off[SB ? 0 : j];                     \
            __builtin_amdgcn_global_load_lds((am_gptr_t)(gb + fo), (am_lptr_t)dst, 16, 0, 0);                               \
        } else {                                                                                                            \
            const int kidx = min((C0) + st_row[jj], n_keys - 1);                                                            \
            const int64_t grow = (kidx < kp_len) ? (int64_t)(kp_start + kidx) : (int64_t)(ko_start + kidx - kp_len);        \
            __builtin_amdgcn_global_load_lds((am_gptr_t)((is_v ? v : k) + grow * ld + st_col[jj]), (am_lptr_t)dst, 16, 0, 0); \
        }                                                                                                                   \
    }
    // ---- fragment addresses inside an image (lane constants; tile / k-step offsets are immediates) ----
    int koff[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) koff[ks] = fr * ROWB + (((4 * ks + fq) ^ am_swz<CH>(fr)) * 16);
    const int tq = fr >> 2, tp = fr & 3;
    int voff[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
        voff[dt] = (4 * fq + tq) * ROWB + (((2 * dt + (tp >> 1)) ^ am_swz<CH>(4 * fq + tq)) * 16) + 8 * (tp & 1);

    const bool wave_has_rows = q0 + wave * 16 < q_len;
    if (n_keys > 0) { AMD_STAGE(0, 0) }
    int bi = 0;
    for (int c0 = 0; c0 < n_keys; c0 += AM_KC, bi ^= 1) {
        if constexpr (SB) {
            if (c0 > 0) {
                __syncthreads();                            // every wave is done with chunk c0 - 64: the one image can be refilled
                AMD_STAGE(c0, 0)
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of chunk c0 have landed
            __syncthreads();                                    // ... everybody's have, and buffer bi ^ 1 (chunk c0 - 64) is consumed
            if (c0 + AM_KC < n_keys) { AMD_STAGE(c0 + AM_KC, bi ^ 1) }
        }
        if (!wave_has_rows) continue;
        const unsigned char* Ks = Ks2 + (SB ? 0 : bi) * IMG;
        const unsigned char* Vs = Vs2 + (SB ? 0 : bi) * IMG;
        auto body = [&](auto full_tag) {
            constexpr bool FULLC = decltype(full_tag)::value;
            const int nt = FULLC ? 4 : min(4, (n_keys - c0 + 15) >> 4);
            float4_t st[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                st[t] = (float4_t){0.f, 0.f, 0.f, 0.f};
                if (!FULLC && t >= nt) continue;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const short8_t kf = *reinterpret_cast<const short8_t*>(Ks + 16 * t * ROWB + koff[ks]);
                    st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], st[t], 0, 0, 0);
                }
            }
            const bool need_mask = !FULLC && ((c0 + AM_KC > n_keys) || (causal && c0 + AM_KC > kp_len));
            float mloc;
            if (FULLC) {
                mloc = am_max16(st[0], st[1], st[2], st[3]);
            } else {
                mloc = -INFINITY;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (t >= nt) continue;
                    if (need_mask) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int kidx = c0 + 16 * t + 4 * fq + r;
                            bool ok = kidx < n_keys;
                            if (causal && kidx >= kp_len) ok = ok && (kidx - kp_len) <= qrow + causal_off;
                            st[t][r] = ok ? st[t][r] : -INFINITY;
                        }
                    }
                    mloc = fmaxf(fmaxf(mloc, fmaxf(st[t][0], st[t][1])), fmaxf(st[t][2], st[t][3]));
                }
            }
            mloc = am_max4(mloc);
            float m_new = fmaxf(m_run, mloc);
            const bool grow = (m_new - m_run) * sc2 > 8.f;
            const bool rescale = __builtin_amdgcn_ballot_w64(grow) != 0;
            if (!rescale) m_new = m_run;
            float alpha = 1.f, lloc = 0.f;
            if (FULLC || m_new != -INFINITY) {
                const float mc = m_new * sc2;
                if (rescale) alpha = __builtin_amdgcn_exp2f(m_run * sc2 - mc);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (!FULLC && t >= nt) continue;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float p = __builtin_amdgcn_exp2f(fmaf(st[t][r], sc2, -mc));
                        st[t][r] = p;
                        lloc += p;
                    }
                }
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) st[t] = (float4_t){0.f, 0.f, 0.f, 0.f};
            }
            lloc = am_sum4(lloc);
            l_run = l_run * alpha + lloc;
            m_run = m_new;
            short8_t pf[2];
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                uint4 u;
                u.x = am_pack2(st[2 * s2][0], st[2 * s2][1]);
                u.y = am_pack2(st[2 * s2][2], st[2 * s2][3]);
                u.z = am_pack2(st[2 * s2 + 1][0], st[2 * s2 + 1][1]);
                u.w = am_pack2(st[2 * s2 + 1][2], st[2 * s2 + 1][3]);
                pf[s2] = *reinterpret_cast<short8_t*>(&u);
            }
            if (rescale) {
#pragma unroll
                for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
            }
            if constexpr (SB) {        // one image, never read while a DMA is in flight: the builtin's vmcnt(0) costs nothing there
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        if (!FULLC && 2 * s2 >= nt) continue;
                        const short4_t b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_ptr)(Vs + 16 * (2 * s2) * ROWB + voff[dt]));
                        const short4_t b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_ptr)(Vs + 16 * (2 * s2 + 1) * ROWB + voff[dt]));
                        const short8_t vf = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
                        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[s2], o[dt], 0, 0, 0);
                    }
                }
            } else {
                const uint32_t vs_lds = (uint32_t)reinterpret_cast<uintptr_t>((am_lptr_t)Vs);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    short4_t b00, b01, b10, b11;
                    if (FULLC || nt > 2) {
                        am_tr_read4<0, 16 * ROWB, 32 * ROWB, 48 * ROWB>(vs_lds + (uint32_t)voff[dt], b00, b01, b10, b11);
                    } else {
                        am_tr_read2<0, 16 * ROWB>(vs_lds + (uint32_t)voff[dt], b00, b01);
                        b10 = b00;
                        b11 = b01;
                    }
                    const short8_t vf0 = {b00[0], b00[1], b00[2], b00[3], b01[0], b01[1], b01[2], b01[3]};
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf0, pf[0], o[dt], 0, 0, 0);
                    if (FULLC || nt > 2) {
                        const short8_t vf1 = {b10[0], b10[1], b10[2], b10[3], b11[0], b11[1], b11[2], b11[3]};
                        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf1, pf[1], o[dt], 0, 0, 0);
                    }
                }
            }
        };
        const bool all_visible = !causal || c0 + AM_KC <= kp_len || (c0 + AM_KC - 1 - kp_len) <= q0 + causal_off;
        if (c0 + AM_KC <= n_keys && all_visible) body(std::true_type{}); else body(std::false_type{});
    }
#undef AMD_STAGE
    const int qi = q0 + wave * 16 + fr;
    if (qi >= q_len) return;
    const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
    bf16_t* orow = out + (int64_t)(q_start + qi) * ldo + h * dh;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        const int c = 16 * dt + 4 * fq;
        if (c < dh) {
            uint2 u;
            u.x = am_pack2(o[dt][0] * inv, o[dt][1] * inv);
            u.y = am_pack2(o[dt][2] * inv, o[dt][3] * inv);
            *reinterpret_cast<uint2*>(orow + c) = u;
        }
    }
}

// ---- ring variant: NON-CAUSAL attention over long sequences (ViT-g 257 tokens, CLIP-L 577) ------------------------------------------------
// The two-image kernel above on ViT-g (508 images x 16 heads per launch): 643 us in the bench, 2.3 TB/s of HBM, MFMA pipes 17 % busy; two
// workgroups per CU (117 registers), five staging rounds per workgroup and three workgroups per (image, head) -- the third for the 257th query
// alone -- that all stream the whole K / V.  In-kernel stamps (-DAM_TIMING) put a quarter of a workgroup's life into its prologue (descriptor,
// Q rows, first chunk: nothing to issue) and showed the waits for the DMA to be short: what the kernel lacks is other workgroups to run
// meanwhile, not a deeper prefetch.  Here:
//   * one lean body: a partial last chunk stages clamped rows (finite) and masks their scores -- no second (masked) instantiation, no staging
//     constants (row / column of a piece are re-derived at each DMA, ~12 VALU per KiB moved; am_lane_opaque keeps them from being hoisted and
//     spilled), fragment offsets as one / two lane constants + immediates: 72 registers instead of 117 = THREE workgroups per CU with two
//     chunk images per operand (48 KiB each);
//   * NW = 9: 144-query tiles (waves 0..7 stage, all nine compute) -- 257 queries are two tiles, K / V pass L2 -> LDS twice instead of three
//     times and no workgroup exists for one query;
//   * n_keys % 64 == 1 FOLDS the last key: its K / V rows ride into 512 spare bytes of LDS with chunk 0 and it is processed after the last chunk,
//     where the chunk loop would have met it, on the VALU (a dot product over the Q fragments the lane holds, one lazy-rescale step) -- instead of
//     a whole round (barrier + DMA flight) for a chunk of one key: 257 keys = 4 rounds.  Same order of operations as the unfolded form, so results
//     differ from it only where the fp32 score does (VALU fma chain against the MFMA's internal sum), not by a different softmax reference point;
//   * V^T fragments are read by am_tr_read4 (see there), the round's barrier is a bare s_barrier (__syncthreads() carries a fence that lowers
//     to vmcnt(0));
//   * two chunk images per operand, the LDS-DMA one chunk ahead.  (The name is from a ring of THREE images with the DMA two chunks ahead: 72 KiB =
//     two workgroups per CU measured 575 against 493 us, tools/debug/att_vit_bench.py -- occupancy beats prefetch depth here; removed.)
// Descriptor semantics, operand orientation, lazy rescale and output are those of attention_mfma_dma_kernel with causal == 0.
#ifdef AM_TIMING   /* tools/debug/am_timing.hip (includes this file with -DAM_TIMING): where a round's time goes (debug builds only) */
__device__ unsigned long long* g_am_stamps;
#define AM_STAMP(i) do { if (lane == 0 && (wave == 0 || wave == 7)) g_am_stamps[((size_t)blockIdx.x * 2 + (wave == 7)) * 64 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
__device__ int g_am_hs;            // layout experiment of the harness: element offset between heads of q / k / v (0: h * dh, the product layout)
#define AMR_HOFF (g_am_hs ? h * g_am_hs : h * dh)
#else
#define AM_STAMP(i) do { } while (0)
#define AMR_HOFF (h * dh)
#endif
template <int DHP, int NW>
__global__ __launch_bounds__(64 * NW, DHP > 96 ? 4 : (NW == 9 ? 7 : 6)) void attention_ring_kernel(const bf16_t* __restrict__ q, int64_t ldq,
                                                                                 const bf16_t* __restrict__ k, int64_t ldk,
                                                                                 const bf16_t* __restrict__ v, int64_t ldv,
                                                                                 bf16_t* __restrict__ out, int64_t ldo,
                                                                                 const int32_t* __restrict__ seq_desc, int H, int dh,
                                                                                 float scale, int fold_ok, int q_tiles, int n_seq) {
    constexpr int ROWB = 2 * DHP;
    constexpr int KS = DHP / 32;
    constexpr int DT = DHP / 16;
    constexpr int CH = DHP / 8;
    constexpr int IMG = AM_KC * ROWB;
    constexpr int NI = AM_KC * CH / 64;
    constexpr int NS = 8;                  // staging waves
    constexpr int LD = 2 * NI / NS;        // DMA instructions per staging wave and chunk (K and V images together)
    constexpr int QT = 16 * NW;
    static_assert(NW == 8 || NW == 9, "8 or 9 waves");
    static_assert(2 * NI % NS == 0, "chunk must split evenly over the staging waves");
    extern __shared__ __attribute__((aligned(1024))) unsigned char am_ring_smem[];      // 4 * IMG + 512 bytes
    unsigned char* const Ks3 = am_ring_smem;
    unsigned char* const Vs3 = am_ring_smem + 2 * IMG;

    int bid;
    if (!am_remap(blockIdx.x, q_tiles, n_seq, H, bid)) return;
    const int qt = bid % q_tiles;
    const int h = (bid / q_tiles) % H;
    const int s = bid / (q_tiles * H);
    const int32_t* d = seq_desc + s * 6;
    const int q_start = d[0], q_len = d[1], kp_start = d[2], kp_len = d[3], ko_start = d[4], ko_len = d[5];
    const int q0 = qt * QT;
    if (q0 >= q_len) return;  // uniform per workgroup
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    // fold_ok bit 1 (value 2): the own key range is causal (query i sees own keys 0 .. i + ko_len - q_len); a tile's chunk loop then ends at its
    // last query's diagonal, and a wave whose 16 queries all lie above a chunk skips it
    const bool causal = (fold_ok & 2) != 0;
    const int causal_off = ko_len - q_len;
    const int own_hi = causal ? max(0, min(ko_len, q0 + min(QT, q_len - q0) + causal_off)) : ko_len;
    const int n_all = kp_len + own_hi;
    const bool fold = (fold_ok & 1) && !causal && (n_all & (AM_KC - 1)) == 1 && n_all > 1;
    const int n_keys = n_all - (fold ? 1 : 0);        // keys that go through the chunk loop (a folded key has index n_keys)
    AM_STAMP(0);

    const int qrow = q0 + wave * 16 + fr;
    // first key this lane's query does NOT see, and the same for the first / last query of the wave (uniform)
    const int lim = causal ? min(n_keys, kp_len + max(0, qrow + causal_off + 1)) : n_keys;
    const int lim_lo = causal ? min(n_keys, kp_len + max(0, q0 + wave * 16 + causal_off + 1)) : n_keys;
    const int lim_hi = causal ? min(n_keys, kp_len + max(0, q0 + wave * 16 + 15 + causal_off + 1)) : n_keys;
    short8_t qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int c = ks * 32 + fq * 8;
        uint4 u = make_uint4(0, 0, 0, 0);
        if (qrow < q_len && c < dh) u = *reinterpret_cast<const uint4*>(q + (int64_t)(q_start + qrow) * ldq + AMR_HOFF + c);
        qf[ks] = *reinterpret_cast<short8_t*>(&u);
    }
    // the folded key's rows of K and V go into 512 bytes behind the images (one DMA of wave 0, issued before -- so landed with -- chunk 0): piece i of
    // the K row at byte 16 i, of the V row at 256 + 16 i
    unsigned char* const odd = am_ring_smem + 4 * IMG;
    if (fold && wave == 0 && (lane < CH || (lane >= 16 && lane < 16 + CH))) {
        const int64_t grow = n_keys < kp_len ? (int64_t)(kp_start + n_keys) : (int64_t)(ko_start + n_keys - kp_len);
        const int c = min((lane & 15) * 8, dh - 8);
        const bf16_t* src = (lane < 16 ? k + grow * ldk : v + grow * ldv) + AMR_HOFF + c;
        __builtin_amdgcn_global_load_lds((am_gptr_t)src, (am_lptr_t)odd, 16, 0, 0);
    }
    // ---- staging: DMA instruction j of staging wave w fills LDS bytes [(j * 8 + w) * 1024, + 1024) of the K | V image pair; rows past the last
    // key re-read it (finite data under p = 0), channel padding re-reads the last real channels (multiplied by the zero padding of Q / dropped) ----
#define AMR_STAGE(C0, BUFI)                                                                                                  \
    if (wave < NS) {                                                                                                        \
        const int ln_ = am_lane_opaque();                                                                                   \
        _Pragma("unroll") for (int j = 0; j < LD; ++j) {                                                                    \
            const int blk = (j * NS + wave) % NI;                                                                           \
            const bool is_v = (j * NS + wave) >= NI;                                                                        \
            unsigned char* dst = (is_v ? Vs3 : Ks3) + (BUFI) * IMG + blk * 1024;                                            \
            const int p = blk * 64 + ln_;                                                                                   \
            const int p_row = p / CH;                                                                                       \
            const int p_col = AMR_HOFF + min(((p - p_row * CH) ^ am_swz<CH>(p_row)) * 8, dh - 8);                           \
            const int kidx = min((C0) + p_row, n_keys - 1);                                                                 \
            const int64_t grow = (kidx < kp_len) ? (int64_t)(kp_start + kidx) : (int64_t)(ko_start + kidx - kp_len);        \
            __builtin_amdgcn_global_load_lds((am_gptr_t)((is_v ? v : k) + grow * (is_v ? ldv : ldk) + p_col), (am_lptr_t)dst, 16, 0, 0); \
        }                                                                                                                   \
    }
    // fragment addresses inside an image.  CH == 12 swizzles the two low piece bits only: (4 ks + fq) ^ x = 4 ks + (fq ^ x) and
    // (2 dt + hb) ^ x = 4 (dt >> 1) + ((2 (dt & 1) + hb) ^ x): one (K) / two (V) lane constants + immediates
    constexpr bool AFF = CH == 12;
    const int tq = fr >> 2, tp = fr & 3;
    int koff[AFF ? 1 : KS], voff[AFF ? 2 : DT];
    if constexpr (AFF) {
        koff[0] = fr * ROWB + ((fq ^ am_swz<CH>(fr)) * 16);
        voff[0] = (4 * fq + tq) * ROWB + (((tp >> 1) ^ am_swz<CH>(4 * fq + tq)) * 16) + 8 * (tp & 1);
        voff[1] = (4 * fq + tq) * ROWB + (((2 + (tp >> 1)) ^ am_swz<CH>(4 * fq + tq)) * 16) + 8 * (tp & 1);
    } else {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) koff[AFF ? 0 : ks] = fr * ROWB + (((4 * ks + fq) ^ am_swz<CH>(fr)) * 16);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
            voff[AFF ? 0 : dt] = (4 * fq + tq) * ROWB + (((2 * dt + (tp >> 1)) ^ am_swz<CH>(4 * fq + tq)) * 16) + 8 * (tp & 1);
    }
#define AMR_KOFF(ks) (AFF ? koff[0] + (ks) * 64 : koff[AFF ? 0 : (ks)])
#define AMR_VOFF(dt) (AFF ? voff[AFF ? (dt) & 1 : 0] + ((dt) >> 1) * 64 : voff[AFF ? 0 : (dt)])

    float4_t o[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i) o[i] = (float4_t){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    const float sc2 = scale * 1.44269504088896340736f;
    const bool wave_has_rows = q0 + wave * 16 < q_len;
    if (n_keys > 0) { AMR_STAGE(0, 0) }
    int bi = 0;
    AM_STAMP(1);
    // (the image index steps and selects exactly as written here: `bi ^= 1` / `bi ^ 1` compute the same and compile to a different schedule)
    for (int c0 = 0; c0 < n_keys; c0 += AM_KC, bi = (bi == 1 ? 0 : bi + 1)) {
        AM_STAMP(2 + (c0 >> 6) * 6);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                     // this wave's pieces of chunk c0 have landed
        AM_STAMP(3 + (c0 >> 6) * 6);
        // LDS reads of the previous round are complete (their values fed MFMAs); DMA writes are covered by the wait above
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // everybody's pieces have landed, image bi ^ 1 (chunk c0 - 64) is consumed
        AM_STAMP(4 + (c0 >> 6) * 6);
        if (c0 + AM_KC < n_keys) { AMR_STAGE(c0 + AM_KC, (bi == 0 ? 1 : bi - 1)) }
        AM_STAMP(5 + (c0 >> 6) * 6);
        if (!wave_has_rows || c0 >= lim_hi) continue;          // (causal: every query of this wave lies above the chunk)
        const unsigned char* Ks = Ks3 + bi * IMG;
        const uint32_t vs_lds = (uint32_t)reinterpret_cast<uintptr_t>((am_lptr_t)(Vs3 + bi * IMG));
        float4_t st[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            st[t] = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const short8_t kf = *reinterpret_cast<const short8_t*>(Ks + 16 * t * ROWB + AMR_KOFF(ks));
                st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], st[t], 0, 0, 0);
            }
        }
        if (c0 + AM_KC > lim_lo) {            // (uniform per wave) a partial last chunk or the causal diagonal: hidden keys score -inf
            const int rel = lim - c0 - 4 * fq;            // score (t, r) of this lane is visible iff 16 t + r < rel
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) st[t][r] = (16 * t + r < rel) ? st[t][r] : -INFINITY;
        }
        float mloc = am_max4(am_max16(st[0], st[1], st[2], st[3]));
        float m_new = fmaxf(m_run, mloc);
        const bool grow = (m_new - m_run) * sc2 > 8.f;
        const bool rescale = __builtin_amdgcn_ballot_w64(grow) != 0;
        if (!rescale) m_new = m_run;
        float alpha = 1.f, lloc = 0.f;
        const float mc = m_new == -INFINITY ? 0.f : m_new * sc2;       // (-inf: a causal query that sees no key yet -- its p are exp2(-inf) = 0)
        if (rescale) alpha = __builtin_amdgcn_exp2f(m_run * sc2 - mc);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(fmaf(st[t][r], sc2, -mc));
                st[t][r] = p;
                lloc += p;
            }
        lloc = am_sum4(lloc);
        l_run = l_run * alpha + lloc;
        m_run = m_new;
        short8_t pf[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            uint4 u;
            u.x = am_pack2(st[2 * s2][0], st[2 * s2][1]);
            u.y = am_pack2(st[2 * s2][2], st[2 * s2][3]);
            u.z = am_pack2(st[2 * s2 + 1][0], st[2 * s2 + 1][1]);
            u.w = am_pack2(st[2 * s2 + 1][2], st[2 * s2 + 1][3]);
            pf[s2] = *reinterpret_cast<short8_t*>(&u);
        }
        if (rescale) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
        }
        AM_STAMP(6 + (c0 >> 6) * 6);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            short4_t b00, b01, b10, b11;
            am_tr_read4<0, 16 * ROWB, 32 * ROWB, 48 * ROWB>(vs_lds + (uint32_t)AMR_VOFF(dt), b00, b01, b10, b11);
            const short8_t vf0 = {b00[0], b00[1], b00[2], b00[3], b01[0], b01[1], b01[2], b01[3]};
            const short8_t vf1 = {b10[0], b10[1], b10[2], b10[3], b11[0], b11[1], b11[2], b11[3]};
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf0, pf[0], o[dt], 0, 0, 0);
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf1, pf[1], o[dt], 0, 0, 0);
        }
        AM_STAMP(7 + (c0 >> 6) * 6);
    }
    if (fold && wave_has_rows) {
        // the folded key, after the last chunk (where the chunk loop would have met it), on the VALU: score = dot of the lane's Q fragments with
        // its channels of the K row (summed over the four lanes of the query), then the same lazy-rescale step as a chunk with this one score;
        // P is rounded to bf16 for the product as the MFMA operand would be, the normaliser takes it unrounded (as in the chunk body)
        float sp = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) sp = am_dot8(qf[ks], *reinterpret_cast<const uint4*>(odd + 16 * (4 * ks + fq)), sp);
        const float sod = am_sum4(sp);
        float m_new = fmaxf(m_run, sod);
        const bool grow = (m_new - m_run) * sc2 > 8.f;
        const bool rescale = __builtin_amdgcn_ballot_w64(grow) != 0;
        if (!rescale) m_new = m_run;
        const float mc = m_new * sc2;
        const float alpha = rescale ? __builtin_amdgcn_exp2f(m_run * sc2 - mc) : 1.f;
        const float p = __builtin_amdgcn_exp2f(fmaf(sod, sc2, -mc));
        l_run = l_run * alpha + p;
        m_run = m_new;
        const float pb = __uint_as_float(am_pack2(p, 0.f) << 16);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const uint2 u = *reinterpret_cast<const uint2*>(odd + 256 + 32 * dt + 8 * fq);
            const float vv[4] = {__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
#pragma unroll
            for (int r = 0; r < 4; ++r) o[dt][r] = fmaf(pb, vv[r], rescale ? o[dt][r] * alpha : o[dt][r]);
        }
    }
#undef AMR_STAGE
#undef AMR_KOFF
#undef AMR_VOFF
    if (!wave_has_rows) return;
    const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
    // ---- output: whole row slices.  A lane holds 4 channels of ONE query per 16-channel tile: stored as they stand, a wave instruction writes 16 rows
    // x 32 bytes -- 16 cache lines for 512 bytes, six times per wave, and the CU's address path (a line per cycle) is what bounds this kernel.  Waves
    // 0..7 pass their 16 x dh block through a quarter of the chunk image that is free (image `bi`: consumed a round ago, nothing in flight into it
    // after the last round's vmcnt(0)) and store 16-byte pieces of consecutive channels: ~5.8 rows of dh x 2 contiguous bytes per instruction.
    // The ninth wave (16 rows of tile 0, one of ViT-g's tile 1) and head dims that are not multiples of 8 keep the direct form. ----
    if (wave < 8 && (dh & 7) == 0) {
        unsigned char* ob = (wave < 4 ? Ks3 : Vs3) + bi * IMG + (wave & 3) * (16 * ROWB);
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            uint2 u;
            u.x = am_pack2(o[dt][0] * inv, o[dt][1] * inv);
            u.y = am_pack2(o[dt][2] * inv, o[dt][3] * inv);
            *reinterpret_cast<uint2*>(ob + fr * ROWB + 32 * dt + 8 * fq) = u;
        }
        const int np = dh >> 3;                                  // 16-byte pieces per row
        const int magic = 65536 / np + 1;                        // p / np for p < 256 (np <= 16)
        const int row0 = q0 + wave * 16;
#pragma unroll
        for (int j = 0; j < (16 * CH + 63) / 64; ++j) {
            const int p_ = j * 64 + lane;
            const int r = (p_ * magic) >> 16;
            const int c = p_ - r * np;
            if (r < 16 && row0 + r < q_len) {
                const uint4 u = *reinterpret_cast<const uint4*>(ob + r * ROWB + c * 16);
                *reinterpret_cast<uint4*>(out + (int64_t)(q_start + row0 + r) * ldo + h * dh + c * 8) = u;
            }
        }
        return;
    }
    if (qrow >= q_len) return;
    bf16_t* orow = out + (int64_t)(q_start + qrow) * ldo + h * dh;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        const int c = 16 * dt + 4 * fq;
        if (c < dh) {
            uint2 u;
            u.x = am_pack2(o[dt][0] * inv, o[dt][1] * inv);
            u.y = am_pack2(o[dt][2] * inv, o[dt][3] * inv);
            *reinterpret_cast<uint2*>(orow + c) = u;
        }
    }
}

// Variant switches (A/B measurements and the variant tests): read from the environment ONCE, and again only when the host asks
// (devqa_attention_reload_env; lib.attention re-reads when it sees a DEVQA_ATTENTION_* variable change).  -1 = unset.
namespace {
struct AttnEnv { int nw = -1, dma = -1, shrt = -1, xcd = -1, ring = -1, fold = -1; };
AttnEnv g_attn_env;
std::atomic<int> g_attn_env_ready{0};
std::mutex g_attn_env_mu;
int env_int(const char* name) { const char* e = getenv(name); return e ? atoi(e) : -1; }
void attn_env_load() {
    std::lock_guard<std::mutex> lock(g_attn_env_mu);
    AttnEnv e;
    e.nw = env_int("DEVQA_ATTENTION_NW");
    e.dma = env_int("DEVQA_ATTENTION_DMA");
    e.shrt = env_int("DEVQA_ATTENTION_SHORT");
    e.xcd = env_int("DEVQA_ATTENTION_XCD");
    e.ring = env_int("DEVQA_ATTENTION_RING");
    e.fold = env_int("DEVQA_ATTENTION_FOLD");
    g_attn_env = e;
    g_attn_env_ready.store(1, std::memory_order_release);
}
}  // namespace

extern "C" int devqa_attention_reload_env() {
    attn_env_load();
    return DEVQA_OK;
}

int launch_attention_mfma(const bf16_t* q, int64_t ldq, const bf16_t* k, int64_t ldk, const bf16_t* v, int64_t ldv, bf16_t* out,
                          int64_t ldo, const int32_t* seq_desc, int n_seq, int max_q_len, int H, int dh, float scale,
                          int causal, void* stream) {
    const int dhp = (dh + 31) / 32 * 32;
    if (dhp != 32 && dhp != 64 && dhp != 96 && dhp != 128) return devqa_fail(DEVQA_E_SHAPE, "attention: dh=%d unsupported", dh);
    if (!g_attn_env_ready.load(std::memory_order_acquire)) attn_env_load();
    const AttnEnv env = g_attn_env;
    causal &= 3;      // bit 2 (value 4, the caller's self-attention promise of include/devqa.h) is accepted and has no effect
    const bool nw_env = env.nw != -1, dma_env = env.dma != -1, short_env = env.shrt != -1;

    // ---- the form ----
    // LDS-DMA staging for long sequences only: on the decoder pack of the bench (960 sequences of 32-80 keys, visible prefix + causal own
    // range, one or two chunks each) the DMA kernel measured 198 us against 135 us for the register-staged one (rocprofv3 trace of
    // bench.py) -- nothing to overlap the DMA with; DEVQA_ATTENTION_DMA=1 forces it, =0 disables it
    const bool dma = dma_env ? env.dma != 0 : max_q_len >= 224;
    // 128-query tiles (8 waves) halve the K / V staging per query, which is what bounds the kernel on long sequences (ViT-g, T = 256:
    // 133 -> 116 us); short sequences fill 64-query tiles better (T = 128: 43.6 vs 47.3 us)
    int dma_nw = max_q_len >= 224 ? 8 : 4;
    // dh 128, causal (the LLaMA decoders of LLaVA / MiniGPT-4: 577-row image prefixes): 64-query tiles of 4 waves measured 565 us against 685 us for
    // 128-query tiles of 8 on the prefix pack of a 16-cycle batch (tools/debug/att_llava_bench.py) -- a causal tile's K / V range ends at its last
    // query, so the larger tile stages more keys per query than it saves
    if (dhp == 128 && (causal & 1)) dma_nw = 4;
    if (env.nw == 8 || env.nw == 4) dma_nw = env.nw;
    // non-causal long sequences (ViT-g, CLIP-L): the ring kernel (attention_ring_kernel).  144-query tiles of 9 waves when they cover the
    // longest sequence with fewer tiles than 128-query ones (257 tokens: 2 instead of 3).  DEVQA_ATTENTION_RING=0 keeps the tiled LDS-DMA kernel,
    // DEVQA_ATTENTION_NW=8 / 9 picks the tile, DEVQA_ATTENTION_FOLD=0 turns the folding of key n_keys - 1 (n_keys % 64 == 1) off -- the staging
    // variants are bit-identical to each other only without it.
    // causal long sequences (the LLaMA decoders' 577-row image prefixes): the same kernel with the diagonal masked per lane and chunks above a
    // wave's queries skipped, 128-query tiles.  The LLaVA decoder pack of a 16-cycle batch (64 prefixes of 577 rows + 192 texts behind them, 32
    // heads x 128; tools/debug/att_llava_bench.py): 986 -> 606 us against attention_mfma_dma_kernel<128, 4> (167 registers, two 4-wave
    // workgroups per CU; here 106 registers, two 8-wave workgroups), bit-identical outputs.
    const bool ring = dma && (causal == 0 ? dhp <= 96 : (causal & 1) != 0) && max_q_len >= 224 && env.ring != 0 &&
                      (!nw_env || env.nw == 8 || env.nw == 9);
    if (ring) dma_nw = nw_env ? env.nw : ((causal & 1) ? 8 : ((max_q_len + 143) / 144 < (max_q_len + 127) / 128 ? 9 : 8));
    // causal packs of short sequences (decoder probes): 32-query tiles of two waves on ONE LDS-DMA image (attention_mfma_dma_kernel<D, 2, true>);
    // non-causal short-query calls (Q-Former: 32 queries over 257 keys) keep the register-staged kernel.
    // Measured on a 127-cycle probe pack (tools/debug/att_pack_bench.py, 2159 sequences): OPT heads (dh 80) 368.6 us against 362.6 us for the
    // register-staged kernel -- the pack is bound by the instructions issued per (sequence, head), not by the pairs in flight, and both forms
    // issue about the same; LLaMA heads (dh 128, where the register-staged form holds two workgroups per CU) 57.8 against 72.1 us.  Default:
    // dh 128 only; DEVQA_ATTENTION_SHORT=1 forces it for every head size, =0 turns it off; so does any DEVQA_ATTENTION_DMA / _NW
    const bool dma_short = causal && !dma && !dma_env && !nw_env && max_q_len <= 64 && (short_env ? env.shrt != 0 : dhp == 128);

    // ---- the grid ----
    const int qt = dma_short ? 32 : dma ? 16 * dma_nw : AM_QT;
    const int q_tiles = (max_q_len + qt - 1) / qt;
    // workgroup -> XCD mapping (am_remap): sequence units for CAUSAL packs with LONG sequences (balance: the LLaMA decoders' mixed packs of
    // 577-row prefixes and 20-row texts), the contiguous ranges of round 2 otherwise -- uniform packs (ViT: every sequence costs the same, ranges
    // keep neighbouring images' lines in one L2) and packs of short sequences (a cycle's texts read their image prefix's K / V through the same
    // L2).  Measured in situ on one box: units everywhere cost the BLIP-2 + FT_VL bench 0.6 % and the MEND_VL config 8 %.
    // DEVQA_ATTENTION_XCD=0 / 1 forces ranges / units.
    const bool units = env.xcd == -1 ? ((causal & 1) && max_q_len >= 224) : env.xcd != 0;
    const long unit = am_unit(n_seq, H);
    const long grid = units ? ((((long)n_seq * H + unit - 1) / unit + 7) / 8) * 8 * unit * q_tiles : (long)n_seq * H * q_tiles;
    const int n_seq_arg = units ? n_seq : -n_seq;
    DEVQA_CHECK_SHAPE(grid < 2147483647L, "attention: grid too large");
    hipStream_t st = (hipStream_t)stream;

    // ---- one launch per form ----
    const int fold_ok = (env.fold != 0 ? 1 : 0) | ((causal & 1) ? 2 : 0);       // the ring kernel's flag word
#define AM_GO(KERN, NW, SMEM, FLAGS)                                                                                         \
    hipLaunchKernelGGL(KERN, dim3((unsigned)grid), dim3(64 * NW), SMEM, st, q, ldq, k, ldk, v, ldv, out, ldo, seq_desc, H, dh, scale, FLAGS, \
                       q_tiles, n_seq_arg)
#define AM_GO_RING(D, NW)                                                                                                   \
    do {                                                                                                                    \
        static std::atomic<unsigned> attr{0};                                                                               \
        const size_t smem = (size_t)4 * AM_KC * 2 * D + 512;      /* two chunk images per operand + the folded key's rows */ \
        devqa_set_max_smem(attention_ring_kernel<D, NW>, smem, attr);                                                       \
        AM_GO((attention_ring_kernel<D, NW>), NW, smem, fold_ok);                                                           \
    } while (0)
#define LAUNCH(D)                                                                                                           \
    do {                                                                                                                    \
        if (dma_short) AM_GO((attention_mfma_dma_kernel<D, 2, true>), 2, 0, causal);                                        \
        else if (ring && dma_nw == 9) AM_GO_RING(D, 9);                                                                     \
        else if (ring) AM_GO_RING(D, 8);                                                                                    \
        else if (dma && dma_nw == 8) AM_GO((attention_mfma_dma_kernel<D, 8>), 8, 0, causal);                                \
        else if (dma) AM_GO((attention_mfma_dma_kernel<D, 4>), 4, 0, causal);                                               \
        else AM_GO((attention_mfma_kernel<D>), 4, 0, causal);                                                               \
    } while (0)
    // FLOPs as launched (4 Tq Tk dh per head with Tq = Tk = max_q_len: an upper bound for ragged / causal batches, exact for ViT)
    const int ph = devqa_prof_begin(DEVQA_PROF_ATTENTION, st);
    if (dhp == 32) LAUNCH(32);
    else if (dhp == 64) LAUNCH(64);
    else if (dhp == 96) LAUNCH(96);
    else LAUNCH(128);
#undef LAUNCH
#undef AM_GO_RING
#undef AM_GO
    devqa_prof_end(ph, 4.0 * (double)n_seq * H * (double)max_q_len * (double)max_q_len * dh * ((causal & 1) ? 0.5 : 1.0), st);
    DEVQA_LAUNCH_CHECK("attention_mfma");
    return DEVQA_OK;
}
