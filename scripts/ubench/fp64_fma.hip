// Microbenchmark: whole-chip issue rate of v_fma_f64 on gfx950 (the FP64 VALU peak the audio decoder's bound uses,
// scripts/demod_rate.py).  Build: hipcc --offload-arch=gfx950 -O3 fp64_fma.hip -o fp64_fma
// Every lane of GRID x 256 lanes runs ITER iterations of 16 independent FMA chains (inline asm, so the compiler can
// neither fuse nor drop them); HIP events around the launch; FLOP = 2 per FMA.  Prints one line per grid size.
#include <hip/hip_runtime.h>
#include <cstdio>

#define ITER 2048
#define BODY16(OP) OP(0) OP(1) OP(2) OP(3) OP(4) OP(5) OP(6) OP(7) OP(8) OP(9) OP(10) OP(11) OP(12) OP(13) OP(14) OP(15)

__global__ __launch_bounds__(256) void fma64(double *out) {
    double a[16];
    const double s = 1.0000001 + threadIdx.x * 1e-12, t = 1e-9;
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = i + threadIdx.x;
    for (int it = 0; it < ITER; ++it) {
#define OP(i) asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(a[i]) : "v"(s), "v"(t));
        BODY16(OP)
#undef OP
    }
    double r = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) r += a[i];
    out[blockIdx.x * blockDim.x + threadIdx.x] = r;
}

int main() {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, 0) != hipSuccess) return 1;
    const int cus = p.multiProcessorCount;
    double *out = nullptr;
    const int max_grid = cus * 32;
    if (hipMalloc(&out, (size_t)max_grid * 256 * sizeof(double)) != hipSuccess) return 1;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    printf("# fp64_fma: %d CUs, clock %d MHz (reported), %d iterations x 16 v_fma_f64 per lane, 256 lanes per workgroup\n",
           cus, p.clockRate / 1000, ITER);
    for (int per_cu = 1; per_cu <= 32; per_cu *= 2) {
        const int grid = cus * per_cu;
        hipLaunchKernelGGL(fma64, dim3(grid), dim3(256), 0, 0, out);   // warm-up
        float best = 1e30f;
        for (int r = 0; r < 5; ++r) {
            (void)hipEventRecord(e0, 0);
            hipLaunchKernelGGL(fma64, dim3(grid), dim3(256), 0, 0, out);
            (void)hipEventRecord(e1, 0);
            (void)hipEventSynchronize(e1);
            float ms = 0;
            (void)hipEventElapsedTime(&ms, e0, e1);
            if (ms < best) best = ms;
        }
        const double fmas = (double)grid * 256 * ITER * 16;
        printf("workgroups/CU %2d  %9.3f ms  %8.2f TFLOP/s f64 (FMA = 2)\n", per_cu, best, 2 * fmas / (best * 1e-3) / 1e12);
    }
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    (void)hipFree(out);
    return 0;
}
