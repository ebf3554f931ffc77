// Workgroups per CU that the runtime grants a one-wavefront workgroup of 256 VGPRs at several static LDS
// sizes around the limb tile kernel's (hs_limb.h, LimbShared<.., true>: 17,856 B before the wavefront
// constants, 20,240 B with them; 20,480 B = 160 KiB / 8 is the most that leaves 8 per CU, 2 waves per SIMD).
// Tuning aid only.   hipcc --offload-arch=gfx950 -O2 tools/lds_occupancy_probe.hip -o tools/bin/lds_occupancy_probe
#include <hip/hip_runtime.h>
#include <stdio.h>

template <int BYTES>
__global__ __launch_bounds__(64) void probe(double* out) {
  __shared__ double s[BYTES / 8];
  s[threadIdx.x] = out[threadIdx.x];
  __syncthreads();
  asm volatile("" ::: "v255");  // 256 VGPRs, as the limb kernel
  out[threadIdx.x] = s[(threadIdx.x * 7) % (BYTES / 8)];
}

template <int BYTES>
int report() {
  int n = -1;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, probe<BYTES>, 64, 0);
  printf("static LDS %6d B, 64 threads, 256 VGPRs: %d workgroups per CU (%s)\n", BYTES, n, hipGetErrorString(e));
  return e == hipSuccess ? 0 : 1;
}

int main() {
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, 0) != hipSuccess) return 2;
  printf("%s: %zu B LDS per workgroup at most, %zu B per CU\n", p.gcnArchName, p.sharedMemPerBlock,
         p.maxSharedMemoryPerMultiProcessor);
  return report<17856>() | report<20240>() | report<20480>() | report<20488>() | report<23400>();
}
