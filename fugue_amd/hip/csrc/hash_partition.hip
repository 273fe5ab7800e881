// Hashing and bucket-partition family: row hashes over fixed-width and
// string columns, bucket ids, histogram and scatter.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "relational.h"

// ------------------------------------------------------------------ //
// hashing: combine one column into the running row-hash               //
// ------------------------------------------------------------------ //
template <typename T>
__global__ __launch_bounds__(BLOCK) void hash_col_kernel(
    const T* __restrict__ data,
    const bool* __restrict__ valid,  // may be null
    uint64_t* __restrict__ out,
    int64_t n,
    int is_first) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    uint64_t v;
    if (valid != nullptr && !valid[i]) {
      v = 0x9e3779b97f4a7c15ULL;  // canonical NULL hash
    } else {
      if constexpr (sizeof(T) == 8) {
        v = mix64(*reinterpret_cast<const uint64_t*>(&data[i]));
      } else if constexpr (sizeof(T) == 4) {
        uint32_t raw = *reinterpret_cast<const uint32_t*>(&data[i]);
        v = mix64((uint64_t)raw);
      } else {
        v = mix64((uint64_t)(uint8_t)data[i]);
      }
    }
    out[i] = is_first ? v : hash_combine(out[i], v);
  }
}

extern "C" {

void launch_hash_col_i64(const int64_t* data, const bool* valid, uint64_t* out,
                         int64_t n, int is_first, hipStream_t stream) {
  hipLaunchKernelGGL(hash_col_kernel<int64_t>, dim3(grid_for(n)), dim3(BLOCK),
                     0, stream, data, valid, out, n, is_first);
}
void launch_hash_col_i32(const int32_t* data, const bool* valid, uint64_t* out,
                         int64_t n, int is_first, hipStream_t stream) {
  hipLaunchKernelGGL(hash_col_kernel<int32_t>, dim3(grid_for(n)), dim3(BLOCK),
                     0, stream, data, valid, out, n, is_first);
}
void launch_hash_col_f64(const double* data, const bool* valid, uint64_t* out,
                         int64_t n, int is_first, hipStream_t stream) {
  hipLaunchKernelGGL(hash_col_kernel<double>, dim3(grid_for(n)), dim3(BLOCK),
                     0, stream, data, valid, out, n, is_first);
}
void launch_hash_col_f32(const float* data, const bool* valid, uint64_t* out,
                         int64_t n, int is_first, hipStream_t stream) {
  hipLaunchKernelGGL(hash_col_kernel<float>, dim3(grid_for(n)), dim3(BLOCK),
                     0, stream, data, valid, out, n, is_first);
}
void launch_hash_col_i8(const int8_t* data, const bool* valid, uint64_t* out,
                        int64_t n, int is_first, hipStream_t stream) {
  hipLaunchKernelGGL(hash_col_kernel<int8_t>, dim3(grid_for(n)), dim3(BLOCK),
                     0, stream, data, valid, out, n, is_first);
}

}  // extern "C"

// ------------------------------------------------------------------ //
// radix partition: histogram + scatter by bucket                      //
// ------------------------------------------------------------------ //
__global__ __launch_bounds__(BLOCK) void bucket_of_kernel(
    const uint64_t* __restrict__ hashes, int32_t* __restrict__ buckets,
    int64_t n, int32_t num_buckets) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    buckets[i] = (int32_t)(hashes[i] % (uint64_t)num_buckets);
  }
}

__global__ __launch_bounds__(BLOCK) void histogram_kernel(
    const int32_t* __restrict__ buckets, int64_t* __restrict__ hist,
    int64_t n, int32_t num_buckets) {
  extern __shared__ int64_t lhist[];
  for (int i = threadIdx.x; i < num_buckets; i += blockDim.x) lhist[i] = 0;
  __syncthreads();
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    atomicAdd((unsigned long long*)&lhist[buckets[i]], 1ULL);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < num_buckets; i += blockDim.x) {
    if (lhist[i] > 0)
      atomicAdd((unsigned long long*)&hist[i], (unsigned long long)lhist[i]);
  }
}

// scatter: stable within bucket is NOT guaranteed (atomic claim);
// relational semantics don't require row order stability here.
__global__ __launch_bounds__(BLOCK) void scatter_kernel(
    const int32_t* __restrict__ buckets, int64_t* __restrict__ cursor,
    int64_t* __restrict__ perm, int64_t n) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t pos = (int64_t)atomicAdd((unsigned long long*)&cursor[buckets[i]],
                                     1ULL);
    perm[pos] = i;
  }
}

extern "C" {

void launch_bucket_of(const uint64_t* hashes, int32_t* buckets, int64_t n,
                      int32_t num_buckets, hipStream_t stream) {
  hipLaunchKernelGGL(bucket_of_kernel, dim3(grid_for(n)), dim3(BLOCK), 0,
                     stream, hashes, buckets, n, num_buckets);
}

void launch_histogram(const int32_t* buckets, int64_t* hist, int64_t n,
                      int32_t num_buckets, hipStream_t stream) {
  size_t shm = (size_t)num_buckets * sizeof(int64_t);
  hipLaunchKernelGGL(histogram_kernel, dim3(grid_for(n)), dim3(BLOCK), shm,
                     stream, buckets, hist, n, num_buckets);
}

void launch_scatter(const int32_t* buckets, int64_t* cursor, int64_t* perm,
                    int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(scatter_kernel, dim3(grid_for(n)), dim3(BLOCK), 0, stream,
                     buckets, cursor, perm, n);
}

}  // extern "C"

// ------------------------------------------------------------------ //
// string hashing: per-row xx-style mix over the UTF-8 bytes           //
// (offsets int64 [n+1], bytes uint8).  One thread per row; fine for   //
// typical short keys — wave-cooperative long-string variant later.    //
// ------------------------------------------------------------------ //
__device__ __forceinline__ uint64_t hash_bytes(
    const uint8_t* __restrict__ data, int64_t len) {
  uint64_t h = 0x27d4eb2f165667c5ULL ^ (uint64_t)len;
  int64_t i = 0;
  for (; i + 8 <= len; i += 8) {
    uint64_t k;
    memcpy(&k, data + i, 8);
    h = hash_combine(h, k);
  }
  uint64_t tail = 0;
  for (int64_t j = i; j < len; ++j) tail = (tail << 8) | data[j];
  if (i < len) h = hash_combine(h, tail);
  return mix64(h);
}

__global__ __launch_bounds__(BLOCK) void hash_string_col_kernel(
    const int64_t* __restrict__ offsets,
    const uint8_t* __restrict__ bytes,
    const bool* __restrict__ valid,
    uint64_t* __restrict__ out,
    int64_t n,
    int is_first) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    uint64_t v;
    if (valid != nullptr && !valid[i]) {
      v = 0x9e3779b97f4a7c15ULL;
    } else {
      int64_t lo = offsets[i];
      v = hash_bytes(bytes + lo, offsets[i + 1] - lo);
    }
    out[i] = is_first ? v : hash_combine(out[i], v);
  }
}

// seed an output hash buffer (for independent second hashes)
__global__ __launch_bounds__(BLOCK) void hash_seed_kernel(
    uint64_t* __restrict__ out, int64_t n, uint64_t seed) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    out[i] = mix64(seed + (uint64_t)1);
}

extern "C" {

void launch_hash_string_col(const int64_t* offsets, const uint8_t* bytes,
                            const bool* valid, uint64_t* out, int64_t n,
                            int is_first, hipStream_t stream) {
  hipLaunchKernelGGL(hash_string_col_kernel, dim3(grid_for(n)), dim3(BLOCK),
                     0, stream, offsets, bytes, valid, out, n, is_first);
}

void launch_hash_seed(uint64_t* out, int64_t n, uint64_t seed,
                      hipStream_t stream) {
  hipLaunchKernelGGL(hash_seed_kernel, dim3(grid_for(n)), dim3(BLOCK), 0,
                     stream, out, n, seed);
}

}  // extern "C"
