// The read-only pass of a fine-tile ADI step against the passes that write, on the bare access pattern of fine_x_kernel
// (qp_adi_fine.inc), without its arithmetic:
//   hipcc --offload-arch=gfx950 -O3 tools/tile_readonly.hip -o tools/bin/tile_readonly && tools/bin/tile_readonly
// One wave per 64 x 32 tile (x-chunk tx x rows [64 ty, 64 ty + 64)) of an N x N fp64 plane, lane = (h, column c), register
// r = row 64 ty + 32 h + r: 32 row loads of two 256-byte segments each, a dependent chain through them, then
//   rmw   : 32 row stores in place + 2 interface stores per lane (today's sweeps: 16 B per cell)
//   read  : 2 interface stores per lane only, no plane store (the reduce pass R: 8 B per cell)
// Blocks are dealt like fine_block (the two tiles of a 64 x 64 super-tile on one XCD).  Plane filled with ordinary numbers
// (see tile_ceiling.hip: zeros run faster), half a second of warm-up first.  Prints the time of one pass.
#include <hip/hip_runtime.h>
#include <cstdio>

template <bool STORE>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4)))
tile_fine(double* __restrict__ a, double* __restrict__ iface, int n) {
  const int lane = threadIdx.x, h = lane >> 5, c = lane & 31;
  const int nsx = n / 64, ns = nsx * (n / 64);
  const int bid = blockIdx.x, group = bid >> 4, rr = bid & 15;
  const int m = min(8, ns - group * 8);
  const int S = group * 8 + rr % m, sub = rr / m;
  const int tx = 2 * (S % nsx) + sub, ty = S / nsx;
  // wave-uniform tile origin + a 32-bit lane offset, as in fine_x_kernel (64-bit row addresses spill)
  double* tile = a + (long)(ty * 64) * n + tx * 32;
  unsigned off = (unsigned)(h * 32) * (unsigned)n + (unsigned)c;
  double v[32];
#pragma unroll
  for (int r = 0; r < 32; ++r) v[r] = tile[off + (unsigned)(r * n)];
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < 32; ++r) { s = fma(s, 0.25, 0.75 * v[r]); v[r] = s; }
#pragma unroll
  for (int r = 31; r >= 0; --r) { s = fma(s, 0.25, 0.75 * v[r]); v[r] = s; }
  if (STORE) {
    asm volatile("" : "+v"(off));
#pragma unroll
    for (int r = 0; r < 32; ++r) tile[off + (unsigned)(r * n)] = v[r];
  }
  double yf = 0.0, yl = 0.0;
#pragma unroll
  for (int r = 0; r < 32; ++r) { yf = fma(yf, 0.5, v[r]); yl = fma(yl, 0.25, v[31 - r]); }
  const int yc = 2 * ty + h;
  double* ir = iface + (long)tx * 32 + c;
  ir[(long)(2 * yc + 1) * n] = yf;
  ir[(long)(2 * yc + 2) * n] = yl;
}

template <bool STORE>
static void run(double* a, double* iface, int n) {
  const int tiles = (n / 32) * (n / 64);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  for (int r = 0; r < 3; ++r) tile_fine<STORE><<<tiles, 64>>>(a, iface, n);
  hipDeviceSynchronize();
  const int reps = 50;
  hipEventRecord(e0);
  for (int r = 0; r < reps; ++r) tile_fine<STORE><<<tiles, 64>>>(a, iface, n);
  hipEventRecord(e1);
  hipEventSynchronize(e1);
  float ms;
  hipEventElapsedTime(&ms, e0, e1);
  const double us = 1e3 * ms / reps;
  const double bytes = (STORE ? 16.0 : 8.0) * n * n;
  printf("N=%5d %-5s tiles=%6d  %8.2f us  %6.2f TB/s (plane bytes)\n", n, STORE ? "rmw" : "read", tiles, us,
         bytes / us / 1e6);
  hipEventDestroy(e0);
  hipEventDestroy(e1);
}

__global__ void fill(double* a, long n, double scale) {
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long)gridDim.x * blockDim.x)
    a[t] = scale * (1.0 + 1e-3 * (double)((t * 2654435761u) % 1000));
}

int main() {
  const int nmax = 4096;
  double *a, *iface;
  if (hipMalloc(&a, (size_t)nmax * nmax * 8) != hipSuccess) return 1;
  // interface rows: 2 P + 2 rows of n lines, P = n / 32 chunks per column
  if (hipMalloc(&iface, (size_t)(2 * (nmax / 32) + 2) * nmax * 8) != hipSuccess) return 1;
  fill<<<8192, 256>>>(a, (long)nmax * nmax, 1e-4);
  hipDeviceSynchronize();
  for (int r = 0; r < 10000; ++r) tile_fine<true><<<(nmax / 32) * (nmax / 64), 64>>>(a, iface, nmax);
  hipDeviceSynchronize();
  const int sizes[] = {1024, 2048, 4096};
  for (int n : sizes) {
    for (int rep = 0; rep < 2; ++rep) {
      run<true>(a, iface, n);
      run<false>(a, iface, n);
    }
  }
  printf("status: %s\n", hipGetErrorString(hipDeviceSynchronize()));
  return 0;
}
