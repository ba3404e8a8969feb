// Reverse-engineer ds_read_b64_tr_b8: fill LDS so that byte e holds e (low
// byte in pass 0, high byte in pass 1), give lane a the address base + 8 a,
// and dump which bytes each lane receives.  Byte index e = 8 * (supplying
// lane) + (byte within that lane's 8).
//   hipcc --offload-arch=gfx950 -O2 scripts/probe_tr8.hip -o probe_tr8
#include <hip/hip_runtime.h>
#include <cstdio>

using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;

__global__ void tr8_probe(unsigned* out, int hi_pass) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[512];
  const int lane = threadIdx.x & 63;
  for (int e = lane; e < 512; e += 64)
    lds[e] = (unsigned char)(hi_pass ? (e >> 8) : (e & 255));
  __builtin_amdgcn_s_barrier();
  const unsigned a = (unsigned)(uintptr_t)(
      (__attribute__((address_space(3))) unsigned char*)lds) + 8 * lane;
  u32x2 r;
  asm volatile("ds_read_b64_tr_b8 %0, %1\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(r) : "v"(a) : "memory");
  __builtin_amdgcn_sched_barrier(0);
  out[lane * 2] = r[0];
  out[lane * 2 + 1] = r[1];
}

int main() {
  unsigned* d;
  if (hipMalloc(&d, 128 * sizeof(unsigned)) != hipSuccess) return 1;
  unsigned lo[128], hi[128];
  hipLaunchKernelGGL(tr8_probe, dim3(1), dim3(64), 0, 0, d, 0);
  if (hipMemcpy(lo, d, sizeof lo, hipMemcpyDeviceToHost) != hipSuccess)
    return 1;
  hipLaunchKernelGGL(tr8_probe, dim3(1), dim3(64), 0, 0, d, 1);
  if (hipMemcpy(hi, d, sizeof hi, hipMemcpyDeviceToHost) != hipSuccess)
    return 1;
  // the guess to confirm: lane 16 g + i receives byte i of the 16-byte rows
  // that lanes 16 g + 2 j, 16 g + 2 j + 1 supply, j = 0 .. 7
  int ok = 1;
  for (int l = 0; l < 64; ++l) {
    printf("lane %2d:", l);
    for (int j = 0; j < 8; ++j) {
      const int e = ((lo[2 * l + j / 4] >> (8 * (j % 4))) & 255) +
                    256 * ((hi[2 * l + j / 4] >> (8 * (j % 4))) & 255);
      printf(" %3d.%d", e >> 3, e & 7);          // supplying lane . byte
      const int i = l & 15, g = l >> 4;
      ok &= e == 8 * (16 * g + 2 * j + (i >> 3)) + (i & 7);
    }
    printf("\n");
  }
  printf("row-pair transpose guess: %s\n", ok ? "CONFIRMED" : "WRONG");
  return 0;
}
