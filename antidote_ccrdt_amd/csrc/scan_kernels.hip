// scan_kernels.hip — the generic segment scan of the device calls
// (scan_kernels.hpp): per-key capacities, then their exclusive scan in three
// passes (block totals, the scan of the totals, the blocks' own scans).
#include "scan_kernels.hpp"

namespace ccrdt {

// caps[k] = cnt[k*stride] (0 if cnt == nullptr) + ops of key k; then an
// exclusive scan of caps into off[0..n], off[n] = total.
__global__ void caps_kernel(const uint64_t* key_ptr, const uint32_t* cnt, uint32_t stride,
                            uint64_t n, uint64_t* caps) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  caps[k] = (key_ptr ? key_ptr[k + 1] - key_ptr[k] : 0) + (cnt ? cnt[k * stride] : 0u);
}

constexpr int SC_BLOCK = 256;
__device__ __forceinline__ uint64_t block_excl_scan(uint64_t v, uint64_t& total) {
  __shared__ uint64_t ws[SC_BLOCK / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t o = (uint64_t)shfl64((int64_t)inc, lane >= off ? lane - off : lane);
    if (lane >= off) inc += o;
  }
  if (lane == 63) ws[w] = inc;
  __syncthreads();
  uint64_t pre = 0, tot = 0;
  for (int j = 0; j < SC_BLOCK / 64; ++j) {
    if (j < w) pre += ws[j];
    tot += ws[j];
  }
  __syncthreads();
  total = tot;
  return pre + inc - v;
}
__global__ __launch_bounds__(SC_BLOCK) void scan_partials_kernel(const uint64_t* in, uint64_t n,
                                                                 uint64_t* part) {
  const uint64_t i = (uint64_t)blockIdx.x * SC_BLOCK + threadIdx.x;
  uint64_t tot;
  (void)block_excl_scan(i < n ? in[i] : 0, tot);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
__global__ __launch_bounds__(SC_BLOCK) void scan_tops_kernel(uint64_t* part, uint64_t nb) {
  __shared__ uint64_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint64_t b0 = 0; b0 < nb; b0 += SC_BLOCK) {
    const uint64_t b = b0 + threadIdx.x;
    uint64_t tot;
    const uint64_t ex = block_excl_scan(b < nb ? part[b] : 0, tot);
    if (b < nb) part[b] = ex + carry;
    __syncthreads();
    if (threadIdx.x == 0) carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) part[nb] = carry;
}
__global__ __launch_bounds__(SC_BLOCK) void scan_apply_kernel(const uint64_t* in, uint64_t n,
                                                              const uint64_t* part, uint64_t* out,
                                                              uint64_t nb) {
  const uint64_t i = (uint64_t)blockIdx.x * SC_BLOCK + threadIdx.x;
  uint64_t tot;
  const uint64_t ex = block_excl_scan(i < n ? in[i] : 0, tot);
  if (i < n) out[i] = part[blockIdx.x] + ex;
  if (i == 0) out[n] = part[nb];
}

int ScanScratch::exclusive_scan(const uint64_t* key_ptr, const uint32_t* cnt, uint32_t stride, uint64_t n,
                                uint64_t* off) {
  CCRDT_TRY(ensure(n));  // (the caller's up-front ensure() made this a no-op)
  uint64_t* const caps = caps_.as<uint64_t>();
  uint64_t* const part = part_.as<uint64_t>();
  const hipStream_t st = stream;
  const uint64_t nb = (n + SC_BLOCK - 1) / SC_BLOCK;
  if (n) {
    hipLaunchKernelGGL(caps_kernel, dim3((unsigned)nb), dim3(SC_BLOCK), 0, st, key_ptr, cnt, stride, n,
                       caps);
    hipLaunchKernelGGL(scan_partials_kernel, dim3((unsigned)nb), dim3(SC_BLOCK), 0, st, caps, n, part);
  }
  hipLaunchKernelGGL(scan_tops_kernel, dim3(1), dim3(SC_BLOCK), 0, st, part, nb);
  if (n)
    hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)nb), dim3(SC_BLOCK), 0, st, caps, n, part, off,
                       nb);
  else
    CCRDT_HIP(hipMemsetAsync(off, 0, 8, st));
  CCRDT_HIP(hipGetLastError());
  return CCRDT_OK;
}

int ScanScratch::ensure(uint64_t n) {
  CCRDT_TRY(caps_.ensure((n + 1) * 8));
  return part_.ensure(((n + SC_BLOCK - 1) / SC_BLOCK + 2) * 8);
}

void ScanScratch::release() {
  caps_.release();
  part_.release();
}

}  // namespace ccrdt
