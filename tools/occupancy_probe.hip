// Diagnostic: how many workgroups of a given shape and dynamic LDS size run at once per CU.
// Launches 256 x k workgroups that each spin ~20 us; the launch takes ~one spin per round, so
// the time jumps when k exceeds the resident workgroups per CU.
//   hipcc --offload-arch=gfx950 -O3 tools/occupancy_probe.hip -o /tmp/occ && /tmp/occ
//   /tmp/occ 256 31936 32256 32768     (threads per workgroup, then the LDS sizes to try)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

__global__ void spin(float* out, int iters) {
  extern __shared__ float lds[];
  float x = threadIdx.x;
  for (int i = 0; i < iters; i++) x = x * 1.0000001f + 0.5f;
  lds[threadIdx.x] = x;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = lds[(threadIdx.x + 1) % blockDim.x];
}

int main(int argc, char** argv) {
  float* out;
  if (hipMalloc(&out, 4 * 4096 * sizeof(float)) != hipSuccess) return 1;
  hipFuncSetAttribute((const void*)spin, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipEvent_t t0, t1;
  hipEventCreate(&t0);
  hipEventCreate(&t1);
  const int threads = argc > 1 ? atoi(argv[1]) : 384, iters = 20000;
  std::vector<int> sizes = {20480, 32768, 39936, 40448, 40768, 40960, 41984, 53248};
  if (argc > 2) {
    sizes.clear();
    for (int i = 2; i < argc; i++) sizes.push_back(atoi(argv[i]));
  }
  if (threads < 64 || threads > 1024) return 2;
  for (int lds : sizes) {
    if (lds < threads * 4 || lds > 160 * 1024) return 2;
    printf("LDS %6d B:", lds);
    for (int k : {2, 3, 4, 5, 6}) {
      spin<<<256 * k, threads, lds>>>(out, iters);
      hipEventRecord(t0);
      spin<<<256 * k, threads, lds>>>(out, iters);
      hipEventRecord(t1);
      hipEventSynchronize(t1);
      float ms;
      hipEventElapsedTime(&ms, t0, t1);
      printf("  %d/CU %.1f us", k, ms * 1e3);
    }
    int nb = 0;
    hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)spin, threads, lds);
    printf("  | runtime says %d per CU\n", nb);
  }
  hipFree(out);
  return 0;
}
