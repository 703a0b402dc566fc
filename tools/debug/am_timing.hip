// Stand-alone timing program for the ring attention kernel (not part of the library): in-kernel stamps (AM_STAMP) of where a staging round's
// time goes on the ViT-g geometry (508 images x 16 heads x T tokens, dh 88), and the fused-qkv against a head-major padded layout.
// Includes the product kernel file with its stamp hooks compiled in:
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -DAM_TIMING -I de-vqa_amd/csrc -I include tools/debug/am_timing.hip -o build/am_timing
//   build/am_timing [T]        (T = tokens per image, default 257)
#ifndef AM_TIMING
#error "compile with -DAM_TIMING"
#endif
#include "../../de-vqa_amd/csrc/attention_mfma.hip"
#include <cstdarg>
#include <cstdio>
#include <vector>
#include <algorithm>
int devqa_fail(int code, const char* fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); return code; }
int devqa_prof_begin(int, hipStream_t) { return -1; }
void devqa_prof_end(int, double, hipStream_t) {}
int main(int argc, char** argv) {
    const int n_seq = 508, H = 16, dh = 88, T = argc > 1 ? atoi(argv[1]) : 257;
    const size_t M = (size_t)n_seq * T, ld = 3 * H * dh;
    bf16_t *qkv, *out; int32_t* desc; unsigned long long* st;
    hipMalloc(&qkv, M * ld * 2); hipMalloc(&out, M * H * dh * 2); hipMalloc(&desc, n_seq * 24);
    std::vector<unsigned short> h(M * ld);
    unsigned x = 1;
    for (auto& v : h) { x = x * 1664525u + 1013904223u; v = (unsigned short)(0x3c00 + ((x >> 9) & 0x3ff) - ((x >> 3) & 0x8000)); }
    hipMemcpy(qkv, h.data(), h.size() * 2, hipMemcpyHostToDevice);
    std::vector<int32_t> hd(n_seq * 6);
    for (int i = 0; i < n_seq; ++i) { hd[i * 6] = i * T; hd[i * 6 + 1] = T; hd[i * 6 + 2] = 0; hd[i * 6 + 3] = 0; hd[i * 6 + 4] = i * T; hd[i * 6 + 5] = T; }
    hipMemcpy(desc, hd.data(), hd.size() * 4, hipMemcpyHostToDevice);
    // layout experiment: the same values head-major and padded, [3][H][M][96] (rows of one head contiguous: whole-line requests)
    bf16_t* hm;
    hipMalloc(&hm, (size_t)3 * H * M * 96 * 2);
    {
        std::vector<unsigned short> g((size_t)3 * H * M * 96, 0);
        for (size_t r = 0; r < M; ++r)
            for (int w = 0; w < 3; ++w)
                for (int hh = 0; hh < H; ++hh)
                    for (int c = 0; c < dh; ++c) g[(((size_t)w * H + hh) * M + r) * 96 + c] = h[r * ld + (size_t)w * H * dh + hh * dh + c];
        hipMemcpy(hm, g.data(), g.size() * 2, hipMemcpyHostToDevice);
    }
    for (int lay = 0; lay < 2; ++lay) {
        const int hs = lay ? (int)(M * 96) : 0;
        hipMemcpyToSymbol(HIP_SYMBOL(g_am_hs), &hs, sizeof(hs));
        const bf16_t* qp = lay ? hm : qkv;
        const bf16_t* kp = lay ? hm + (size_t)H * M * 96 : qkv + H * dh;
        const bf16_t* vp = lay ? hm + (size_t)2 * H * M * 96 : qkv + 2 * H * dh;
        const int64_t ldl = lay ? 96 : (int64_t)ld;
        const int q_tiles = (T + 143) / 144;
        const long grid = (long)n_seq * H * q_tiles;
        hipMalloc(&st, (size_t)grid * 2 * 64 * 8);
        hipMemcpyToSymbol(HIP_SYMBOL(g_am_stamps), &st, sizeof(st));
        hipFuncSetAttribute(reinterpret_cast<const void*>(attention_ring_kernel<96, 9>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 64 * 192 + 512);
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
        float best = 1e9f;
        for (int rep = 0; rep < 12; ++rep) {
            hipEventRecord(e0, nullptr);
            hipLaunchKernelGGL((attention_ring_kernel<96, 9>), dim3((unsigned)grid), dim3(576), 4 * 64 * 192 + 512, nullptr, qp, ldl, kp, ldl, vp, ldl, out,
                               (int64_t)(H * dh), desc, H, dh, 0.1066f, 1, q_tiles, -n_seq);
            hipEventRecord(e1, nullptr);
            hipEventSynchronize(e1);
            float ms = 0;
            hipEventElapsedTime(&ms, e0, e1);
            if (rep >= 2) best = std::min(best, ms);
        }
        printf("layout %s: ring<96, 9> best of 10: %.1f us (stamped build)\n", lay ? "head-major padded [3][H][M][96]" : "row-major fused qkv [M][3 H dh]", best * 1e3);
        hipFree(st);
    }
    { const int hs = 0; hipMemcpyToSymbol(HIP_SYMBOL(g_am_hs), &hs, sizeof(hs)); }
    for (int nw = 8; nw <= 9; ++nw) {
        const int qt = 16 * nw, q_tiles = (T + qt - 1) / qt;
        const long grid = (long)n_seq * H * q_tiles;
        hipMalloc(&st, (size_t)grid * 2 * 64 * 8);
        hipMemset(st, 0, (size_t)grid * 2 * 64 * 8);
        hipMemcpyToSymbol(HIP_SYMBOL(g_am_stamps), &st, sizeof(st));
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
        float ms = 0;
        for (int rep = 0; rep < 6; ++rep) {
            if (rep == 5) hipEventRecord(e0, nullptr);
            if (nw == 9) {
                hipFuncSetAttribute(reinterpret_cast<const void*>(attention_ring_kernel<96, 9>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 64 * 192 + 512);
                hipLaunchKernelGGL((attention_ring_kernel<96, 9>), dim3((unsigned)grid), dim3(576), 4 * 64 * 192 + 512, nullptr, qkv, (int64_t)ld, qkv + H * dh, (int64_t)ld,
                                   qkv + 2 * H * dh, (int64_t)ld, out, (int64_t)(H * dh), desc, H, dh, 0.1066f, 1, q_tiles, -n_seq);
            } else {
                hipFuncSetAttribute(reinterpret_cast<const void*>(attention_ring_kernel<96, 8>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 64 * 192 + 512);
                hipLaunchKernelGGL((attention_ring_kernel<96, 8>), dim3((unsigned)grid), dim3(512), 4 * 64 * 192 + 512, nullptr, qkv, (int64_t)ld, qkv + H * dh, (int64_t)ld,
                                   qkv + 2 * H * dh, (int64_t)ld, out, (int64_t)(H * dh), desc, H, dh, 0.1066f, 1, q_tiles, -n_seq);
            }
            if (rep == 5) hipEventRecord(e1, nullptr);
        }
        hipDeviceSynchronize();
        hipEventElapsedTime(&ms, e0, e1);
        std::vector<unsigned long long> hs((size_t)grid * 2 * 64);
        hipMemcpy(hs.data(), st, hs.size() * 8, hipMemcpyDeviceToHost);
        auto med = [](std::vector<double>& v) { if (v.empty()) return 0.0; std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
        printf("T %d, %d waves: %.1f us (stamped build), %ld workgroups\n", T, nw, ms * 1e3, grid);
        for (int tile = 0; tile < q_tiles; ++tile) {
            for (int wsel = 0; wsel < 2; ++wsel) {
                std::vector<double> pro, total;
                std::vector<double> ph[5][5];
                for (long b = tile; b < grid; b += q_tiles) {
                    // the kernel remaps blockIdx -> (seq, head, tile); tile = bid % q_tiles after the remap, not of blockIdx: classify by stamps only
                    const unsigned long long* s_ = &hs[((size_t)b * 2 + wsel) * 64];
                    if (s_[0] == 0 || s_[1] == 0) continue;
                    pro.push_back((double)(s_[1] - s_[0]));
                    int r = 0;
                    for (; r < 5 && s_[2 + r * 6] != 0; ++r) {
                        const unsigned long long* p_ = s_ + 2 + r * 6;
                        ph[r][0].push_back((double)(p_[1] - p_[0]));       // DMA wait
                        ph[r][1].push_back((double)(p_[2] - p_[1]));       // barrier
                        ph[r][2].push_back((double)(p_[3] - p_[2]));       // stage issue
                        if (p_[4] != 0) ph[r][3].push_back((double)(p_[4] - p_[3]));       // S + softmax
                        if (p_[5] != 0) ph[r][4].push_back((double)(p_[5] - p_[4]));       // P.V
                    }
                }
                printf("  blockIdx %% q_tiles == %d, wave %d: prologue %.0f;", tile, wsel ? 7 : 0, med(pro));
                for (int r = 0; r < 5; ++r)
                    if (!ph[r][0].empty())
                        printf("  round %d: wait %.0f bar %.0f stage %.0f S+softmax %.0f PV %.0f |", r, med(ph[r][0]), med(ph[r][1]), med(ph[r][2]), med(ph[r][3]), med(ph[r][4]));
                printf("\n");
            }
        }
        hipFree(st);
    }
    return 0;
}
