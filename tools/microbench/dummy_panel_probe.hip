// The panel stream of the joint column that ends in dummy unknowns (panel8x1_dpp: 8 pivots, 8 columns) against the full
// 16-pivot stream (panel16x1_dpp) on a panel with that structure: rows / columns 8..15 of the diagonal tile are the identity
// with exactly zero coupling, the rows below have zeros in columns 8..15.  One wavefront per workgroup; s_memtime around the
// stream.  Prints the median cycles of each and whether L and 1 / L_jj compare equal (== : the sign of a zero may differ).
//   hipcc --offload-arch=gfx950 -O3 -I paper_gorbani_2025_humanoids_multi-rate-mpc-ironcub_amd/csrc -o dummy_panel_probe dummy_panel_probe.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>
#define VS_DEV __device__ __forceinline__
#include "vsmpc_panel_asm.inc"

constexpr int ROWS = 80, N = ROWS * 17, NO = N + 16;

// VARIANT 0: panel16x1_dpp, 1: panel8x1_dpp (+ 1 / L_jj = 1 of the dummy pivots, as panel_dummy_dpp writes it)
template <int VARIANT>
__global__ __launch_bounds__(64) void probe(const double* __restrict__ in, double* __restrict__ out, unsigned long long* cyc) {
    __shared__ double sT[NO];
    const int lane = threadIdx.x;
    for (int i = lane; i < N; i += 64) sT[i] = in[i];
    __syncthreads();
    double g[16], inv_last;
    const unsigned row = unsigned(reinterpret_cast<uintptr_t>(sT + (16 + lane) * 17));
    const unsigned dg = unsigned(reinterpret_cast<uintptr_t>(sT + (lane & 15) * 17));
    const unsigned iv = unsigned(reinterpret_cast<uintptr_t>(sT + N));
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    if constexpr (VARIANT == 0) {
        panel16x1_dpp(row, row, dg, iv, g, inv_last);
    } else {
        panel8x1_dpp(row, row, dg, iv, g, inv_last);
        if (lane >= 8 && lane < 16) sT[N + lane] = 1.0;
    }
    __syncthreads();
    if (lane < 16) {
#pragma unroll
        for (int c = 0; c < 16; ++c) sT[lane * 17 + c] = g[c];
    }
    __syncthreads();
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (blockIdx.x == 0)
        for (int i = lane; i < NO; i += 64) out[i] = sT[i];
    if (lane == 0) cyc[blockIdx.x] = t1 - t0;
}

int main() {
    constexpr int G = 256;
    std::vector<double> h(N, 0.0);
    unsigned s = 2024u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return double(s >> 8) / double(1u << 24) - 0.5; };
    for (int r = 0; r < ROWS; ++r)
        for (int c = 0; c < 8; ++c) h[r * 17 + c] = rnd();
    for (int r = 0; r < 16; ++r)
        for (int c = 0; c < 16; ++c) {
            const bool dr = r >= 8, dc = c >= 8;
            h[r * 17 + c] = (dr || dc) ? (r == c ? 1.0 : 0.0) : (r == c ? 3.0 + 0.1 * r : 0.2 * h[std::max(r, c) * 17 + std::min(r, c)]);
        }
    for (int r = 0; r < 8; ++r)
        for (int c = 0; c < r; ++c) h[c * 17 + r] = h[r * 17 + c];
    double *din, *dout;
    unsigned long long* dcyc;
    (void)hipMalloc(&din, N * 8); (void)hipMalloc(&dout, NO * 8); (void)hipMalloc(&dcyc, G * 8);
    (void)hipMemcpy(din, h.data(), N * 8, hipMemcpyHostToDevice);
    std::vector<double> res[2];
    const char* names[2] = {"panel16x1_dpp (16 pivots)          ", "panel8x1_dpp (8 pivots, 8 columns) "};
    for (int v = 0; v < 2; ++v) {
        std::vector<unsigned long long> med;
        for (int rep = 0; rep < 5; ++rep) {
            if (v == 0) hipLaunchKernelGGL(probe<0>, dim3(G), dim3(64), 0, 0, din, dout, dcyc);
            else hipLaunchKernelGGL(probe<1>, dim3(G), dim3(64), 0, 0, din, dout, dcyc);
            if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
            std::vector<unsigned long long> c(G);
            (void)hipMemcpy(c.data(), dcyc, G * 8, hipMemcpyDeviceToHost);
            std::sort(c.begin(), c.end());
            med.push_back(c[G / 2]);
        }
        std::sort(med.begin(), med.end());
        res[v].resize(NO);
        (void)hipMemcpy(res[v].data(), dout, NO * 8, hipMemcpyDeviceToHost);
        printf("%s: median %llu cycles (runs %llu .. %llu)\n", names[v], med[2], med[0], med[4]);
    }
    int diff = 0;
    for (int i = 0; i < NO; ++i) {
        if (i < N && i % 17 == 16) continue;                // row padding
        if (i < 16 * 17 && i % 17 > i / 17) continue;       // above the diagonal: leftovers
        if (!(res[0][i] == res[1][i])) {
            if (diff < 8) printf("  differs at %d: %.17g vs %.17g\n", i, res[0][i], res[1][i]);
            ++diff;
        }
    }
    printf(diff ? "DIFFERS: %d entries\n" : "L and 1/L_jj equal to the 16-pivot stream\n", diff);
    return diff != 0;
}
