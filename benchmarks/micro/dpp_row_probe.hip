// dpp_row_probe.hip -- two facts behind the 9-column fix of csrc/ttl_state.hip,
// read off one wave on the GPU:
//   1. what `v_mov_b32_dpp row_shr:1` (from_prev_lane) hands the first lane of a 16-lane
//      row: lanes 16 and 32 print 0, not the value of lanes 15 and 31;
//   2. which of two lanes of ONE 16-byte store instruction wins when they write the same
//      bytes: lane 32 writes -1 over columns 125..127, which lane 31 writes as 225..227.
// Build and run:  hipcc --offload-arch=gfx950 -O3 dpp_row_probe.hip -o dpp_row_probe && ./dpp_row_probe
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float v4f __attribute__((ext_vector_type(4)));
typedef v4f v4f_dword_aligned __attribute__((aligned(4)));
__device__ __forceinline__ float from_prev_lane(float v) {
    return __int_as_float(
        __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, false));
}
__global__ void probe(float *shifted, float *row) {
    const int lane = threadIdx.x;
    if (lane > 32) return;
    const float mine = (float)(lane + 1);
    shifted[lane] = from_prev_lane(mine);
    // lanes 0..31 write columns 4 lane .. 4 lane + 3 with 100 + column; lane 32 writes the
    // 16 bytes that end at column 128: columns 125..127 with -1 and column 128
    v4f v{100.f + 4 * lane, 101.f + 4 * lane, 102.f + 4 * lane, 103.f + 4 * lane};
    int at = 4 * lane;
    if (lane == 32) { v = v4f{-1.f, -1.f, -1.f, 228.f}; at = 125; }
    *reinterpret_cast<v4f_dword_aligned *>(row + at) = v;
}
int main() {
    float *d_s, *d_r, s[64], r[136];
    if (hipMalloc(&d_s, sizeof(s)) != hipSuccess || hipMalloc(&d_r, sizeof(r)) != hipSuccess) return 2;
    (void)hipMemset(d_s, 0, sizeof(s));
    (void)hipMemset(d_r, 0, sizeof(r));
    for (int rep = 0; rep < 1; ++rep) {
        hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d_s, d_r);
        if (hipDeviceSynchronize() != hipSuccess) return 3;
        (void)hipMemcpy(s, d_s, sizeof(s), hipMemcpyDeviceToHost);
        (void)hipMemcpy(r, d_r, sizeof(r), hipMemcpyDeviceToHost);
        printf("row_shr:1 lanes 15 16 17 31 32: %g %g %g %g %g\n", s[15], s[16], s[17], s[31], s[32]);
        printf("columns 124..128: %g %g %g %g %g\n", r[124], r[125], r[126], r[127], r[128]);
    }
    (void)hipFree(d_s);
    (void)hipFree(d_r);
    return 0;
}
