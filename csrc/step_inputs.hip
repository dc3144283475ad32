// Device-side resolution of async-scheduling placeholders.
//
// With async scheduling the host builds step N+1 while step N still runs, so
// a decode row's input token may not exist on the host yet: it carries -1 and
// names its row in step N's sampled-token tensor. This kernel fills those
// rows on the device, in stream order behind step N's sampling kernel, so the
// host never reads device data to launch a step.
#include <hip/hip_runtime.h>

#include <cstdint>

// tokens[i] = prev_row[i] >= 0 ? prev_tokens[prev_row[i]] : tokens[i]
// A prev_row past the previous tensor leaves the row untouched.
__global__ void resolve_placeholders_kernel(
    int64_t* __restrict__ tokens,             // [n]
    const int32_t* __restrict__ prev_row,     // [n]
    const int64_t* __restrict__ prev_tokens,  // [n_prev]
    int n, int n_prev) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int r = prev_row[i];
  if (r >= 0 && r < n_prev) tokens[i] = prev_tokens[r];
}

extern "C" int ps_resolve_placeholders(void* tokens, const void* prev_row,
                                       const void* prev_tokens, long n,
                                       long n_prev, hipStream_t stream) {
  if (n <= 0) return 0;  // nothing to resolve: no launch
  if (n > INT32_MAX || n_prev < 0 || n_prev > INT32_MAX) return 1;
  const int threads = 256;
  const unsigned blocks = (unsigned)((n + threads - 1) / threads);
  resolve_placeholders_kernel<<<dim3(blocks), threads, 0, stream>>>(
      static_cast<int64_t*>(tokens), static_cast<const int32_t*>(prev_row),
      static_cast<const int64_t*>(prev_tokens), (int)n, (int)n_prev);
  return 0;
}
