// CDNA4 (gfx950 / MI355X) relational kernels for the fugue_amd HIP engine.
//
// Design notes (see /opt/skills/guides/cdna_hip_programming.md):
//  * wave64: blocks are multiples of 64 threads (256 used throughout).
//  * memory-bound kernels use grid-stride loops capped at ~8192 blocks
//    (256 CUs x 8 blocks/CU x headroom) — guide §6 G11.
//  * hash tables are open-addressing in HBM with linear probing;
//    the group-by kernel additionally has an LDS-resident pre-aggregation
//    variant (per-workgroup table in shared memory, flushed once) for
//    low-cardinality keys — the LDS-hash-table requirement of the north
//    star ("LDS-resident hash tables").
//  * all cross-workgroup updates use device-scope atomics (guide §6 G16:
//    per-XCD L2s are not coherent; atomicAdd on global memory is
//    device-scope by default).
//
// These kernels replace the reference framework's delegation of
// repartition/groupby/join to Spark/Dask/DuckDB.

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>

#define WAVE 64
#define BLOCK 256
#define MAX_GRID 8192

static inline int grid_for(int64_t n, int per_thread = 1) {
  int64_t blocks = (n + (int64_t)BLOCK * per_thread - 1) / ((int64_t)BLOCK * per_thread);
  if (blocks < 1) blocks = 1;
  if (blocks > MAX_GRID) blocks = MAX_GRID;
  return (int)blocks;
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  // splitmix64 finalizer — full-avalanche 64-bit mix
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdULL;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ULL;
  x ^= x >> 33;
  return x;
}

__device__ __forceinline__ uint64_t hash_combine(uint64_t h, uint64_t v) {
  return mix64(h ^ (v + 0x9e3779b97f4a7c15ULL + (h << 6) + (h >> 2)));
}

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
// global (keyless) column reductions                                   //
//   wave-level SUM reduction uses the f64 matrix core:                 //
//   ones[16x4] x partials[4x16] via v_mfma_f64_16x16x4_f64 collapses   //
//   64 lane partials to 16 column sums in ONE instruction (lanes       //
//   0..15), finished by 4 shuffle rounds.  min/max/count use plain     //
//   shuffle trees.  (north-star: "MFMA-vectorised reductions shown in  //
//   rocprof")                                                          //
// ------------------------------------------------------------------ //
typedef double v4d __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void atomic_min_f64(double* addr, double val);
__device__ __forceinline__ void atomic_max_f64(double* addr, double val);

__device__ __forceinline__ double wave_reduce_sum_mfma(double v) {
#if defined(__gfx950__) || defined(__gfx90a__) || defined(__gfx940__) || \
    defined(__gfx942__)
  v4d acc = {0.0, 0.0, 0.0, 0.0};
  // A = ones (16x4), B = lane partials (4x16): D[i][j] = sum_k B[k][j]
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(1.0, v, acc, 0, 0, 0);
  double s = acc[0];  // col j = lane&15 sum, replicated across rows
  s += __shfl_down(s, 8, 16);
  s += __shfl_down(s, 4, 16);
  s += __shfl_down(s, 2, 16);
  s += __shfl_down(s, 1, 16);
  return s;  // valid on lane 0
#else
  for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
  return v;
#endif
}

__global__ __launch_bounds__(BLOCK) void reduce_cols_kernel(
    const double* __restrict__ vals,   // [n_aggs, n]
    const bool* __restrict__ valids,   // [n_aggs, n] or null
    const int32_t* __restrict__ ops,   // [n_aggs] 0=sum 1=min 2=max
    int n_aggs, int64_t n,
    double* __restrict__ out,          // [n_aggs] pre-initialized
    int64_t* __restrict__ out_count) { // [n_aggs] zero-initialized
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int lane = threadIdx.x & (WAVE - 1);
  for (int a = 0; a < n_aggs; ++a) {
    int op = ops[a];
    double acc = op == 1 ? INFINITY : (op == 2 ? -INFINITY : 0.0);
    int64_t cnt = 0;
    const double* col = vals + (int64_t)a * n;
    const bool* cv = valids == nullptr ? nullptr : valids + (int64_t)a * n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
      if (cv != nullptr && !cv[i]) continue;
      double v = col[i];
      ++cnt;
      if (op == 0) acc += v;
      else if (op == 1) acc = v < acc ? v : acc;
      else acc = v > acc ? v : acc;
    }
    // wave reduce
    if (op == 0) {
      acc = wave_reduce_sum_mfma(acc);
    } else {
      for (int off = WAVE / 2; off > 0; off >>= 1) {
        double o = __shfl_down(acc, off, WAVE);
        if (op == 1) acc = o < acc ? o : acc;
        else acc = o > acc ? o : acc;
      }
    }
    for (int off = WAVE / 2; off > 0; off >>= 1)
      cnt += __shfl_down(cnt, off, WAVE);
    if (lane == 0) {
      if (cnt > 0) {
        if (op == 0) atomicAdd(&out[a], acc);
        else if (op == 1) atomic_min_f64(&out[a], acc);
        else atomic_max_f64(&out[a], acc);
        atomicAdd((unsigned long long*)&out_count[a],
                  (unsigned long long)cnt);
      }
    }
  }
}

extern "C" {
void launch_reduce_cols(const double* vals, const bool* valids,
                        const int32_t* ops, int n_aggs, int64_t n,
                        double* out, int64_t* out_count,
                        hipStream_t stream) {
  hipLaunchKernelGGL(reduce_cols_kernel, dim3(grid_for(n, 8)), dim3(BLOCK),
                     0, stream, vals, valids, ops, n_aggs, n, out, out_count);
}
}  // extern "C"

// ------------------------------------------------------------------ //
// group-by aggregation: open-addressing HBM hash table                //
//   key: exact int64 (multi-column keys packed by the python layer)   //
//   aggs: fp64 matrix [n_aggs, n_rows]; per-agg op code:              //
//     0=sum 1=min 2=max 3=count(valid)                                //
//   count of rows per group always collected (slot -1 of aggs)        //
// ------------------------------------------------------------------ //

#define GB_EMPTY 0x8000000000000000LL

__device__ __forceinline__ void atomic_min_f64(double* addr, double val) {
  unsigned long long* a = (unsigned long long*)addr;
  unsigned long long old = *a, assumed;
  do {
    assumed = old;
    double cur = __longlong_as_double(assumed);
    if (!(val < cur)) break;
    old = atomicCAS(a, assumed, __double_as_longlong(val));
  } while (old != assumed);
}

__device__ __forceinline__ void atomic_max_f64(double* addr, double val) {
  unsigned long long* a = (unsigned long long*)addr;
  unsigned long long old = *a, assumed;
  do {
    assumed = old;
    double cur = __longlong_as_double(assumed);
    if (!(val > cur)) break;
    old = atomicCAS(a, assumed, __double_as_longlong(val));
  } while (old != assumed);
}

// probe/insert into the global table; returns the claimed slot.
// Aggregation is keyed by SLOT (not a dense group id): slots are
// compacted after the kernel (torch.nonzero over tkeys != EMPTY), which
// avoids any in-kernel id-publication wait (an intra-wave spin on
// another lane's store can deadlock under divergent-branch
// serialization).
__device__ __forceinline__ int64_t gb_probe_insert(
    int64_t key, int64_t* __restrict__ tkeys, int64_t tsize) {
  uint64_t h = mix64((uint64_t)key);
  int64_t slot = (int64_t)(h & (uint64_t)(tsize - 1));
  while (true) {
    // plain load first; the CAS (global RMW) only runs for empty slots
    int64_t cur = tkeys[slot];
    if (cur == key) return slot;
    if (cur == GB_EMPTY) {
      long long prev = (long long)atomicCAS(
          (unsigned long long*)&tkeys[slot], (unsigned long long)GB_EMPTY,
          (unsigned long long)key);
      if (prev == GB_EMPTY || prev == key) return slot;
      // lost the race to a different key: fall through and advance (a
      // re-read could serve a stale line from the per-XCD cache)
    }
    slot = (slot + 1) & (tsize - 1);
  }
}

__global__ __launch_bounds__(BLOCK) void gb_aggregate_kernel(
    const int64_t* __restrict__ keys,
    const double* __restrict__ vals,    // [n_aggs, n] row-major
    const bool* __restrict__ valids,    // [n_aggs, n] or null
    const int32_t* __restrict__ ops,    // [n_aggs]
    int n_aggs,
    int64_t n,
    int64_t* __restrict__ tkeys,        // [tsize] init GB_EMPTY
    double* __restrict__ gaggs,         // [n_aggs, tsize]
    int64_t* __restrict__ gcount,       // [tsize] row counts per slot
    int64_t tsize) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t key = keys[i];
    int64_t slot = gb_probe_insert(key, tkeys, tsize);
    atomicAdd((unsigned long long*)&gcount[slot], 1ULL);
    for (int a = 0; a < n_aggs; ++a) {
      bool ok = (valids == nullptr) || valids[(int64_t)a * n + i];
      if (!ok) continue;
      double v = vals[(int64_t)a * n + i];
      double* dst = &gaggs[(int64_t)a * tsize + slot];
      switch (ops[a]) {
        case 0: atomicAdd(dst, v); break;
        case 1: atomic_min_f64(dst, v); break;
        case 2: atomic_max_f64(dst, v); break;
        case 3: atomicAdd(dst, 1.0); break;
      }
    }
  }
}

// LDS pre-aggregation variant: per-workgroup table (keys+sum/count only,
// the common fast path: all ops are sum or count), flushed to the global
// table at block end.  LDS budget: 1024 entries x (8B key + 8B*n_aggs)
// must fit 160KiB; python chooses this path only when n_aggs<=4.
#define LDS_SLOTS 1024

__global__ __launch_bounds__(BLOCK) void gb_aggregate_lds_kernel(
    const int64_t* __restrict__ keys,
    const double* __restrict__ vals,
    const bool* __restrict__ valids,
    const int32_t* __restrict__ ops,   // all must be 0 (sum) or 3 (count)
    int n_aggs,
    int64_t n,
    int64_t* __restrict__ tkeys,
    double* __restrict__ gaggs,
    int64_t* __restrict__ gcount,
    int64_t tsize) {
  __shared__ int64_t lkeys[LDS_SLOTS];
  __shared__ double laggs[4 * LDS_SLOTS];
  __shared__ long long lcount[LDS_SLOTS];
  for (int i = threadIdx.x; i < LDS_SLOTS; i += blockDim.x) {
    lkeys[i] = GB_EMPTY;
    lcount[i] = 0;
    for (int a = 0; a < n_aggs; ++a) laggs[a * LDS_SLOTS + i] = 0.0;
  }
  __syncthreads();
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t key = keys[i];
    uint64_t h = mix64((uint64_t)key);
    int slot = (int)(h & (LDS_SLOTS - 1));
    bool in_lds = false;
    for (int probe = 0; probe < 16; ++probe) {
      long long prev = (long long)atomicCAS(
          (unsigned long long*)&lkeys[slot], (unsigned long long)GB_EMPTY,
          (unsigned long long)key);
      if (prev == GB_EMPTY || prev == key) { in_lds = true; break; }
      slot = (slot + 1) & (LDS_SLOTS - 1);
    }
    if (in_lds) {
      atomicAdd((unsigned long long*)&lcount[slot], 1ULL);
      for (int a = 0; a < n_aggs; ++a) {
        bool ok = (valids == nullptr) || valids[(int64_t)a * n + i];
        if (!ok) continue;
        double v = (ops[a] == 3) ? 1.0 : vals[(int64_t)a * n + i];
        atomicAdd(&laggs[a * LDS_SLOTS + slot], v);
      }
    } else {
      // overflow: straight to the global table
      int64_t gslot = gb_probe_insert(key, tkeys, tsize);
      atomicAdd((unsigned long long*)&gcount[gslot], 1ULL);
      for (int a = 0; a < n_aggs; ++a) {
        bool ok = (valids == nullptr) || valids[(int64_t)a * n + i];
        if (!ok) continue;
        double v = (ops[a] == 3) ? 1.0 : vals[(int64_t)a * n + i];
        atomicAdd(&gaggs[(int64_t)a * tsize + gslot], v);
      }
    }
  }
  __syncthreads();
  // flush the LDS table into the global table
  for (int i = threadIdx.x; i < LDS_SLOTS; i += blockDim.x) {
    int64_t key = lkeys[i];
    if (key == GB_EMPTY) continue;
    int64_t gslot = gb_probe_insert(key, tkeys, tsize);
    atomicAdd((unsigned long long*)&gcount[gslot],
              (unsigned long long)lcount[i]);
    for (int a = 0; a < n_aggs; ++a) {
      atomicAdd(&gaggs[(int64_t)a * tsize + gslot], laggs[a * LDS_SLOTS + i]);
    }
  }
}

// ------------------------------------------------------------------ //
// partitioned group-by (high cardinality): phase 1 scatter rows into   //
// hash-partitioned order, phase 2 per-partition LDS aggregation.       //
// Partition id = TOP bits of mix64(key); LDS slots use LOW bits, so    //
// keys within one partition still spread across the LDS table.         //
// ------------------------------------------------------------------ //

#define PART_MAX 4096

// LDS-privatized histogram (global atomics only on the per-block flush)
__global__ __launch_bounds__(BLOCK) void gb_part_hist_kernel(
    const int64_t* __restrict__ keys, int64_t n, int shift,
    int64_t* __restrict__ hist, int num_parts) {
  __shared__ int lhist[PART_MAX];
  for (int i = threadIdx.x; i < num_parts; i += blockDim.x) lhist[i] = 0;
  __syncthreads();
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + stride < n; i += 2 * stride) {
    int64_t k1 = keys[i];
    int64_t k2 = keys[i + stride];
    int p1 = (int)(mix64((uint64_t)k1) >> shift);
    int p2 = (int)(mix64((uint64_t)k2) >> shift);
    atomicAdd(&lhist[p1], 1);
    atomicAdd(&lhist[p2], 1);
  }
  for (; i < n; i += stride) {
    int64_t k = keys[i];
    int p = (int)(mix64((uint64_t)k) >> shift);
    atomicAdd(&lhist[p], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < num_parts; i += blockDim.x) {
    if (lhist[i] > 0)
      atomicAdd((unsigned long long*)&hist[i], (unsigned long long)lhist[i]);
  }
}

// Chunked scatter with per-block LDS range reservation: each block
// histograms a chunk in LDS, reserves contiguous per-partition ranges
// with ONE global atomic per touched partition, then scatters the chunk
// (the chunk's keys re-read from L2).  Cuts global atomics from one per
// row to one per (block, partition).
#define SCATTER_CHUNK (BLOCK * 16)

__global__ __launch_bounds__(BLOCK) void gb_part_scatter_kernel(
    const int64_t* __restrict__ keys,
    const double* __restrict__ vals,   // [n_aggs, n]
    int n_aggs, int64_t n, int shift,
    int64_t* __restrict__ cursor,      // [P] exclusive offsets (mutated)
    int64_t* __restrict__ out_keys,
    double* __restrict__ out_vals,
    int num_parts,
    int32_t* __restrict__ out_pos,    // optional layout record
    int64_t chunk) {  // rows per reservation (SCATTER_CHUNK by default)
  __shared__ int lhist[PART_MAX];
  __shared__ int64_t lbase[PART_MAX];
  for (int64_t start = (int64_t)blockIdx.x * chunk; start < n;
       start += (int64_t)gridDim.x * chunk) {
    int64_t end = start + chunk;
    if (end > n) end = n;
    for (int i = threadIdx.x; i < num_parts; i += blockDim.x) lhist[i] = 0;
    __syncthreads();
    for (int64_t i = start + threadIdx.x; i < end; i += blockDim.x) {
      int p = (int)(mix64((uint64_t)keys[i]) >> shift);
      atomicAdd(&lhist[p], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < num_parts; i += blockDim.x) {
      int c = lhist[i];
      lbase[i] =
          c > 0
              ? (int64_t)atomicAdd((unsigned long long*)&cursor[i],
                                   (unsigned long long)c)
              : 0;
      lhist[i] = 0;
    }
    __syncthreads();
    for (int64_t i = start + threadIdx.x; i < end; i += blockDim.x) {
      int64_t key = keys[i];
      int p = (int)(mix64((uint64_t)key) >> shift);
      int64_t pos = lbase[p] + atomicAdd(&lhist[p], 1);
      out_keys[pos] = key;
      if (out_pos != nullptr) out_pos[i] = (int32_t)pos;
      for (int a = 0; a < n_aggs; ++a)
        out_vals[(int64_t)a * n + pos] = vals[(int64_t)a * n + i];
    }
    __syncthreads();
  }
}

// one workgroup per partition (grid-stride over partitions); ops must be
// sum (0) or count (3)
__global__ __launch_bounds__(BLOCK) void gb_aggregate_part_kernel(
    const int64_t* __restrict__ part_keys,
    const double* __restrict__ part_vals,  // [n_aggs, n]
    const int32_t* __restrict__ ops,
    int n_aggs, int64_t n,
    const int64_t* __restrict__ offsets,   // [P+1]
    int64_t num_parts,
    int64_t* __restrict__ tkeys,
    double* __restrict__ gaggs,
    int64_t* __restrict__ gcount,
    int64_t tsize) {
  __shared__ int64_t lkeys[LDS_SLOTS];
  __shared__ double laggs[4 * LDS_SLOTS];
  __shared__ long long lcount[LDS_SLOTS];
  for (int64_t p = blockIdx.x; p < num_parts; p += gridDim.x) {
    for (int i = threadIdx.x; i < LDS_SLOTS; i += blockDim.x) {
      lkeys[i] = GB_EMPTY;
      lcount[i] = 0;
      for (int a = 0; a < n_aggs; ++a) laggs[a * LDS_SLOTS + i] = 0.0;
    }
    __syncthreads();
    int64_t lo = offsets[p], hi = offsets[p + 1];
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
      int64_t key = part_keys[i];
      uint64_t h = mix64((uint64_t)key);
      int slot = (int)(h & (LDS_SLOTS - 1));
      bool in_lds = false;
      for (int probe = 0; probe < 32; ++probe) {
        long long prev = (long long)atomicCAS(
            (unsigned long long*)&lkeys[slot], (unsigned long long)GB_EMPTY,
            (unsigned long long)key);
        if (prev == GB_EMPTY || prev == key) { in_lds = true; break; }
        slot = (slot + 1) & (LDS_SLOTS - 1);
      }
      if (in_lds) {
        atomicAdd((unsigned long long*)&lcount[slot], 1ULL);
        for (int a = 0; a < n_aggs; ++a) {
          double v = (ops[a] == 3) ? 1.0 : part_vals[(int64_t)a * n + i];
          atomicAdd(&laggs[a * LDS_SLOTS + slot], v);
        }
      } else {
        int64_t gslot = gb_probe_insert(key, tkeys, tsize);
        atomicAdd((unsigned long long*)&gcount[gslot], 1ULL);
        for (int a = 0; a < n_aggs; ++a) {
          double v = (ops[a] == 3) ? 1.0 : part_vals[(int64_t)a * n + i];
          atomicAdd(&gaggs[(int64_t)a * tsize + gslot], v);
        }
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < LDS_SLOTS; i += blockDim.x) {
      int64_t key = lkeys[i];
      if (key == GB_EMPTY) continue;
      int64_t gslot = gb_probe_insert(key, tkeys, tsize);
      atomicAdd((unsigned long long*)&gcount[gslot],
                (unsigned long long)lcount[i]);
      for (int a = 0; a < n_aggs; ++a)
        atomicAdd(&gaggs[(int64_t)a * tsize + gslot],
                  laggs[a * LDS_SLOTS + i]);
    }
    __syncthreads();
  }
}

// LDS write-staged scatter: stage the first E rows of each partition
// per chunk in LDS and flush them as contiguous runs, so the bulk of
// the scattered writes leave the CU coalesced instead of as isolated 8B
// transactions.  Overflow rows (partition skew beyond E within a chunk)
// are written directly.  Single-agg-column variant (the common case
// after the COUNT-from-rowcount optimization).  The row loop keeps four
// key loads / hashes / value loads in flight before the LDS cursor
// atomics (the ILP-2 loop it replaced is in profiles/NOTES.md).
// Templated on the partition count P and staging depth E so the
// occupancy/granularity variants (512/8, 1024/4, 2048/2) can be
// A/B-tested at runtime (FUGUE_GB_PARTS).
template <typename KT, int P, int E>
__global__ __launch_bounds__(BLOCK) void gb_part_scatter_staged_kernel_v4(
    const int64_t* __restrict__ keys,
    const double* __restrict__ vals,
    int64_t n, int shift,
    int64_t* __restrict__ cursor,
    KT* __restrict__ out_keys,
    double* __restrict__ out_vals,
    int64_t chunk,
    int* __restrict__ ovf) {
  __shared__ int lhist[P];
  __shared__ int64_t lbase[P];
  __shared__ int lcnt[P];
  __shared__ KT skey[P * E];
  __shared__ double sval[P * E];
  for (int64_t start = (int64_t)blockIdx.x * chunk; start < n;
       start += (int64_t)gridDim.x * chunk) {
    int64_t end = start + chunk;
    if (end > n) end = n;
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
      lhist[i] = 0;
      lcnt[i] = 0;
    }
    __syncthreads();
    const int64_t stride = (int64_t)blockDim.x;
    {
      int64_t i = start + threadIdx.x;
      for (; i + 3 * stride < end; i += 4 * stride) {
        int64_t k[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) k[u] = keys[i + u * stride];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          atomicAdd(&lhist[(int)(mix64((uint64_t)k[u]) >> shift)], 1);
      }
      for (; i < end; i += stride) {
        int p = (int)(mix64((uint64_t)keys[i]) >> shift);
        atomicAdd(&lhist[p], 1);
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
      int c = lhist[i];
      lbase[i] =
          c > 0
              ? (int64_t)atomicAdd((unsigned long long*)&cursor[i],
                                   (unsigned long long)c)
              : 0;
    }
    __syncthreads();
    {
      int64_t i = start + threadIdx.x;
      for (; i + 3 * stride < end; i += 4 * stride) {
        int64_t k[4];
        int p[4];
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) k[u] = keys[i + u * stride];
        if constexpr (sizeof(KT) == 4) {
          if (ovf != nullptr &&
              ((uint64_t)k[0] >= (1ULL << 31) || (uint64_t)k[1] >= (1ULL << 31) ||
               (uint64_t)k[2] >= (1ULL << 31) || (uint64_t)k[3] >= (1ULL << 31))) {
            atomicOr(ovf, 1);
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          p[u] = (int)(mix64((uint64_t)k[u]) >> shift);
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = vals[i + u * stride];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          int pos = atomicAdd(&lcnt[p[u]], 1);
          if (pos < E) {
            skey[p[u] * E + pos] = (KT)k[u];
            sval[p[u] * E + pos] = v[u];
          } else {
            int64_t gpos = lbase[p[u]] + pos;
            out_keys[gpos] = (KT)k[u];
            out_vals[gpos] = v[u];
          }
        }
      }
      for (; i < end; i += stride) {
        int64_t key = keys[i];
        if constexpr (sizeof(KT) == 4) {
          if (ovf != nullptr && (uint64_t)key >= (1ULL << 31)) {
            atomicOr(ovf, 1);
          }
        }
        int p = (int)(mix64((uint64_t)key) >> shift);
        int pos = atomicAdd(&lcnt[p], 1);
        double v = vals[i];
        if (pos < E) {
          skey[p * E + pos] = (KT)key;
          sval[p * E + pos] = v;
        } else {
          int64_t gpos = lbase[p] + pos;
          out_keys[gpos] = (KT)key;
          out_vals[gpos] = v;
        }
      }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < P * E; t += blockDim.x) {
      int p = t / E;
      int e = t % E;
      int c = lcnt[p];
      if (e < c && e < E) {
        int64_t gpos = lbase[p] + e;
        out_keys[gpos] = skey[t];
        out_vals[gpos] = sval[t];
      }
    }
    __syncthreads();
  }
}

// phase-3 variant for the staged path: after partitioning, ANY
// contiguous chunk of rows spans at most a couple of partitions (so only
// a few thousand distinct keys) — partition boundaries are irrelevant to
// correctness (the LDS table just absorbs duplicates; flushes are
// atomic).  Chunk-striding restores full grid parallelism regardless of
// the partition count.  4096 slots / 80KB LDS → 2 blocks/CU.
#define AGG_CHUNK (BLOCK * 128)  // 32768 rows per chunk (sweep-tuned)

// empty-slot sentinel for the LDS table: int64 path uses GB_EMPTY;
// int32 (narrow, packed width <=31 so keys are >=0) uses -1
template <typename KT> __device__ __forceinline__ KT lds_empty();
template <> __device__ __forceinline__ int64_t lds_empty<int64_t>() {
  return GB_EMPTY;
}
template <> __device__ __forceinline__ int32_t lds_empty<int32_t>() {
  return -1;
}

__device__ __forceinline__ long long lds_key_cas(int64_t* addr, int64_t cmp,
                                                 int64_t val) {
  return (long long)atomicCAS((unsigned long long*)addr,
                              (unsigned long long)cmp,
                              (unsigned long long)val);
}
__device__ __forceinline__ int lds_key_cas(int32_t* addr, int32_t cmp,
                                           int32_t val) {
  return (int)atomicCAS((unsigned int*)addr, (unsigned int)cmp,
                        (unsigned int)val);
}

// slow path of the per-row LDS upsert: first-slot read missed (empty or
// different key) — probe/claim, spilling to the global table after 32
// displacements
template <int SLOTS, typename KT>
__device__ __forceinline__ void gb_lds_upsert(
    KT key, double v, int slot, KT EMPTY, KT* __restrict__ lkeys,
    double* __restrict__ laggs, int* __restrict__ lcount,
    int64_t* __restrict__ tkeys, double* __restrict__ gaggs,
    int64_t* __restrict__ gcount, int64_t tsize) {
  bool in_lds = false;
  for (int probe = 0; probe < 32; ++probe) {
    KT cur = lkeys[slot];
    if (cur == key) { in_lds = true; break; }
    if (cur == EMPTY) {
      KT prev = (KT)lds_key_cas(&lkeys[slot], EMPTY, key);
      if (prev == EMPTY || prev == key) { in_lds = true; break; }
    }
    slot = (slot + 1) & (SLOTS - 1);
  }
  if (in_lds) {
    atomicAdd(&lcount[slot], 1);
    atomicAdd(&laggs[slot], v);
  } else {
    int64_t gslot = gb_probe_insert((int64_t)key, tkeys, tsize);
    atomicAdd((unsigned long long*)&gcount[gslot], 1ULL);
    atomicAdd(&gaggs[gslot], v);
  }
}

// ILP-4 row loop: four independent key loads / hashes / first-slot LDS
// reads in flight per iteration — deeper latency hiding at the
// 2-blocks/CU occupancy the 4096-slot table runs at (the ILP-1/ILP-2
// loops it replaced are in profiles/NOTES.md)
template <typename KT, int SLOTS>
__global__ __launch_bounds__(BLOCK) void gb_aggregate_part_big_kernel_v4(
    const KT* __restrict__ part_keys,
    const double* __restrict__ part_vals,
    const int32_t* __restrict__ ops,
    int64_t n,
    int64_t* __restrict__ tkeys,
    double* __restrict__ gaggs,
    int64_t* __restrict__ gcount,
    int64_t tsize, int64_t chunk) {
  __shared__ KT lkeys[SLOTS];
  __shared__ double laggs[SLOTS];
  __shared__ int lcount[SLOTS];
  const KT EMPTY = lds_empty<KT>();
  bool is_count = ops[0] == 3;
  for (int64_t start = (int64_t)blockIdx.x * chunk; start < n;
       start += (int64_t)gridDim.x * chunk) {
    int64_t end = start + chunk;
    if (end > n) end = n;
    for (int i = threadIdx.x; i < SLOTS; i += blockDim.x) {
      lkeys[i] = EMPTY;
      lcount[i] = 0;
      laggs[i] = 0.0;
    }
    __syncthreads();
    int64_t i = start + threadIdx.x;
    const int64_t stride = (int64_t)blockDim.x;
    for (; i + 3 * stride < end; i += 4 * stride) {
      KT k[4];
      int s[4];
      KT c[4];
      double v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) k[u] = part_keys[i + u * stride];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        s[u] = (int)(mix64((uint64_t)(int64_t)k[u]) & (SLOTS - 1));
#pragma unroll
      for (int u = 0; u < 4; ++u) c[u] = lkeys[s[u]];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        v[u] = is_count ? 1.0 : part_vals[i + u * stride];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (c[u] == k[u]) {
          atomicAdd(&lcount[s[u]], 1);
          atomicAdd(&laggs[s[u]], v[u]);
        } else {
          gb_lds_upsert<SLOTS, KT>(k[u], v[u], s[u], EMPTY, lkeys, laggs, lcount,
                            tkeys, gaggs, gcount, tsize);
        }
      }
    }
    for (; i < end; i += stride) {
      KT key = part_keys[i];
      int slot = (int)(mix64((uint64_t)(int64_t)key) & (SLOTS - 1));
      double v = is_count ? 1.0 : part_vals[i];
      KT cur = lkeys[slot];
      if (cur == key) {
        atomicAdd(&lcount[slot], 1);
        atomicAdd(&laggs[slot], v);
      } else {
        gb_lds_upsert<SLOTS, KT>(key, v, slot, EMPTY, lkeys, laggs, lcount, tkeys,
                          gaggs, gcount, tsize);
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SLOTS; i += blockDim.x) {
      KT key = lkeys[i];
      if (key == EMPTY) continue;
      int64_t gslot = gb_probe_insert((int64_t)key, tkeys, tsize);
      atomicAdd((unsigned long long*)&gcount[gslot],
                (unsigned long long)lcount[i]);
      atomicAdd(&gaggs[gslot], laggs[i]);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------
// fused multi-column row gather: one pass reads idx once per row and
// materializes up to GATHER_MAX_COLS columns of one element width
// (replaces per-column at::index_select launches on the join/sort
// output-materialization path)
#define GATHER_MAX_COLS 16

struct GatherPtrs {
  uint64_t src[GATHER_MAX_COLS];
  uint64_t dst[GATHER_MAX_COLS];
};

template <typename T>
__global__ __launch_bounds__(BLOCK) void gather_cols_kernel(
    GatherPtrs ptrs, int ncols, const int64_t* __restrict__ idx,
    int64_t n) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t j = idx[i];
#pragma unroll 4
    for (int c = 0; c < ncols; ++c) {
      reinterpret_cast<T*>(ptrs.dst[c])[i] =
          reinterpret_cast<const T*>(ptrs.src[c])[j];
    }
  }
}

extern "C" {
void launch_gather_cols(const uint64_t* src_ptrs, const uint64_t* dst_ptrs,
                        int ncols, int elem_size, const int64_t* idx,
                        int64_t n, hipStream_t stream) {
  GatherPtrs ptrs;
  for (int c = 0; c < ncols; ++c) {
    ptrs.src[c] = src_ptrs[c];
    ptrs.dst[c] = dst_ptrs[c];
  }
  dim3 g(grid_for(n, 2)), b(BLOCK);
  if (elem_size == 8)
    hipLaunchKernelGGL(gather_cols_kernel<uint64_t>, g, b, 0, stream, ptrs,
                       ncols, idx, n);
  else if (elem_size == 4)
    hipLaunchKernelGGL(gather_cols_kernel<uint32_t>, g, b, 0, stream, ptrs,
                       ncols, idx, n);
  else if (elem_size == 2)
    hipLaunchKernelGGL(gather_cols_kernel<uint16_t>, g, b, 0, stream, ptrs,
                       ncols, idx, n);
  else
    hipLaunchKernelGGL(gather_cols_kernel<uint8_t>, g, b, 0, stream, ptrs,
                       ncols, idx, n);
}
}  // extern "C"

// ---------------------------------------------------------------------
// fused filter-predicate interpreter: evaluates a postfix expression
// program over typed columns in ONE pass, replacing the chain of
// elementwise compare/and/arith kernel launches the torch evaluator
// emits.  Values ride a tagged 8-byte stack (exact int64 compares, no
// double round-trip); null semantics match the python evaluator
// (arith propagates invalid, comparisons on null -> false, AND/OR
// treat null as false, IS NULL inspects the validity bit).
#define EXPR_MAX_OPS 48
#define EXPR_MAX_COLS 12
#define EXPR_STACK 12

// opcodes
enum {
  XOP_COL = 0,   // aux = column index
  XOP_LIT_D = 1, // aux = imm index (double)
  XOP_LIT_I = 2, // aux = imm index (int64 bits)
  XOP_ADD = 3, XOP_SUB = 4, XOP_MUL = 5, XOP_DIV = 6,
  XOP_LT = 7, XOP_LE = 8, XOP_GT = 9, XOP_GE = 10, XOP_EQ = 11,
  XOP_NE = 12,
  XOP_AND = 13, XOP_OR = 14, XOP_NOT = 15,
  XOP_ISNULL = 16, XOP_NOTNULL = 17,
  XOP_NEG = 18,
};

// column dtype tags
enum { XDT_F64 = 0, XDT_F32 = 1, XDT_I64 = 2, XDT_I32 = 3, XDT_I16 = 4,
       XDT_I8 = 5, XDT_BOOL = 6 };

struct ExprProg {
  int n_ops;
  unsigned char op[EXPR_MAX_OPS];
  signed char aux[EXPR_MAX_OPS];
  unsigned long long imm[EXPR_MAX_COLS];
  unsigned long long col_data[EXPR_MAX_COLS];
  unsigned long long col_valid[EXPR_MAX_COLS];  // 0 = none
  unsigned char col_dt[EXPR_MAX_COLS];
};

struct XVal {
  long long bits;   // double bits, int64, or bool(0/1)
  unsigned char tag;  // 0=double 1=int64 2=bool
  bool valid;
};

__device__ __forceinline__ double xv_as_f64(const XVal& v) {
  if (v.tag == 0) return __longlong_as_double(v.bits);
  return (double)v.bits;
}

__device__ __forceinline__ void expr_step(
    const ExprProg& prog, int op, int aux, XVal* st, int& sp, int64_t i) {

      if (op == XOP_COL) {
    const void* dp = reinterpret_cast<const void*>(prog.col_data[aux]);
    XVal v;
    v.valid = true;
    switch (prog.col_dt[aux]) {
      case XDT_F64:
        v.bits = reinterpret_cast<const long long*>(dp)[i];
        v.tag = 0;
        break;
      case XDT_F32: {
        double d = (double)reinterpret_cast<const float*>(dp)[i];
        v.bits = __double_as_longlong(d);
        v.tag = 0;
        break;
      }
      case XDT_I64:
        v.bits = reinterpret_cast<const long long*>(dp)[i];
        v.tag = 1;
        break;
      case XDT_I32:
        v.bits = (long long)reinterpret_cast<const int*>(dp)[i];
        v.tag = 1;
        break;
      case XDT_I16:
        v.bits = (long long)reinterpret_cast<const short*>(dp)[i];
        v.tag = 1;
        break;
      case XDT_I8:
        v.bits = (long long)reinterpret_cast<const signed char*>(dp)[i];
        v.tag = 1;
        break;
      default:  // bool
        v.bits = reinterpret_cast<const bool*>(dp)[i] ? 1 : 0;
        v.tag = 2;
    }
    if (prog.col_valid[aux] != 0ULL) {
      v.valid = reinterpret_cast<const bool*>(prog.col_valid[aux])[i];
    }
    st[sp++] = v;
  } else if (op == XOP_LIT_D) {
    XVal v;
    v.bits = (long long)prog.imm[aux];
    v.tag = 0;
    v.valid = true;
    st[sp++] = v;
  } else if (op == XOP_LIT_I) {
    XVal v;
    v.bits = (long long)prog.imm[aux];
    v.tag = 1;
    v.valid = true;
    st[sp++] = v;
  } else if (op == XOP_NOT) {
    XVal& a = st[sp - 1];
    bool b = a.valid && (a.tag == 0 ? xv_as_f64(a) != 0.0 : a.bits != 0);
    a.bits = b ? 0 : 1;
    a.tag = 2;
    a.valid = true;
  } else if (op == XOP_ISNULL || op == XOP_NOTNULL) {
    XVal& a = st[sp - 1];
    bool b = (op == XOP_ISNULL) ? !a.valid : a.valid;
    a.bits = b ? 1 : 0;
    a.tag = 2;
    a.valid = true;
  } else if (op == XOP_NEG) {
    XVal& a = st[sp - 1];
    if (a.tag == 0)
      a.bits = __double_as_longlong(-xv_as_f64(a));
    else
      a.bits = -a.bits;
  } else if (op == XOP_AND || op == XOP_OR) {
    XVal b = st[--sp];
    XVal& a = st[sp - 1];
    bool ab = a.valid && (a.tag == 0 ? xv_as_f64(a) != 0.0 : a.bits != 0);
    bool bb = b.valid && (b.tag == 0 ? xv_as_f64(b) != 0.0 : b.bits != 0);
    bool r = (op == XOP_AND) ? (ab && bb) : (ab || bb);
    a.bits = r ? 1 : 0;
    a.tag = 2;
    a.valid = true;
  } else {
    XVal b = st[--sp];
    XVal& a = st[sp - 1];
    bool both_int = (a.tag != 0 && b.tag != 0);
    bool valid = a.valid && b.valid;
    if (op >= XOP_ADD && op <= XOP_DIV) {
      if (op == XOP_DIV || !both_int) {
        double x = xv_as_f64(a), y = xv_as_f64(b);
        double r = op == XOP_ADD   ? x + y
                   : op == XOP_SUB ? x - y
                   : op == XOP_MUL ? x * y
                                   : x / y;
        a.bits = __double_as_longlong(r);
        a.tag = 0;
      } else {
        long long x = a.bits, y = b.bits;
        long long r = op == XOP_ADD   ? x + y
                      : op == XOP_SUB ? x - y
                                      : x * y;
        a.bits = r;
        a.tag = 1;
      }
      a.valid = valid;
    } else {  // comparisons: null -> false, result always valid
      bool r;
      if (both_int) {
        long long x = a.bits, y = b.bits;
        r = op == XOP_LT   ? x < y
            : op == XOP_LE ? x <= y
            : op == XOP_GT ? x > y
            : op == XOP_GE ? x >= y
            : op == XOP_EQ ? x == y
                           : x != y;
      } else {
        double x = xv_as_f64(a), y = xv_as_f64(b);
        r = op == XOP_LT   ? x < y
            : op == XOP_LE ? x <= y
            : op == XOP_GT ? x > y
            : op == XOP_GE ? x >= y
            : op == XOP_EQ ? x == y
                           : x != y;
      }
      a.bits = (r && valid) ? 1 : 0;
      a.tag = 2;
      a.valid = true;
    }
  }
}

__global__ __launch_bounds__(BLOCK) void expr_filter_kernel(
    ExprProg prog, int64_t n, bool* __restrict__ out) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    XVal st[EXPR_STACK];
    int sp = 0;
    for (int p = 0; p < prog.n_ops; ++p) {
      expr_step(prog, prog.op[p], prog.aux[p], st, sp, i);
    }
    const XVal& top = st[0];
    out[i] = top.valid && (top.tag == 0 ? xv_as_f64(top) != 0.0
                                        : top.bits != 0);
  }
}

// value-producing variant: writes the top-of-stack value (as f64 or
// exact i64 per OUT_INT) plus a validity mask — fuses compound
// arithmetic in SELECT/assign/aggregate-input expressions
template <bool OUT_INT>
__global__ __launch_bounds__(BLOCK) void expr_value_kernel(
    ExprProg prog, int64_t n, void* __restrict__ out_v,
    bool* __restrict__ out_valid) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    XVal st[EXPR_STACK];
    int sp = 0;
    for (int p = 0; p < prog.n_ops; ++p) {
      int op = prog.op[p];
      int aux = prog.aux[p];
      expr_step(prog, op, aux, st, sp, i);
    }
    const XVal& top = st[0];
    if (OUT_INT) {
      long long r = top.tag == 0 ? (long long)xv_as_f64(top) : top.bits;
      reinterpret_cast<long long*>(out_v)[i] = r;
    } else {
      reinterpret_cast<double*>(out_v)[i] = xv_as_f64(top);
    }
    out_valid[i] = top.valid;
  }
}

extern "C" {
void launch_expr_filter(const void* prog, int64_t n, bool* out,
                        hipStream_t stream) {
  const ExprProg* pg = reinterpret_cast<const ExprProg*>(prog);
  hipLaunchKernelGGL(expr_filter_kernel, dim3(grid_for(n, 2)), dim3(BLOCK),
                     0, stream, *pg, n, out);
}

void launch_expr_value(const void* prog, int64_t n, int out_int, void* out_v,
                       bool* out_valid, hipStream_t stream) {
  const ExprProg* pg = reinterpret_cast<const ExprProg*>(prog);
  if (out_int)
    hipLaunchKernelGGL(expr_value_kernel<true>, dim3(grid_for(n, 2)),
                       dim3(BLOCK), 0, stream, *pg, n, out_v, out_valid);
  else
    hipLaunchKernelGGL(expr_value_kernel<false>, dim3(grid_for(n, 2)),
                       dim3(BLOCK), 0, stream, *pg, n, out_v, out_valid);
}
}  // extern "C"

// P/E-variant dispatch for the staged scatter: 512/8 (baseline), 1024/4
// and 2048/2 trade staging depth for finer partitions (smaller phase-3
// LDS tables -> higher phase-3 occupancy)
template <typename KT>
static void launch_scatter_v4_dispatch(int num_parts, dim3 g, dim3 b,
                                       hipStream_t stream,
                                       const int64_t* keys,
                                       const double* vals, int64_t n,
                                       int shift, int64_t* cursor, KT* ok,
                                       double* out_vals, int64_t chunk,
                                       int* ovf) {
  switch (num_parts) {
    case 1024:
      hipLaunchKernelGGL((gb_part_scatter_staged_kernel_v4<KT, 1024, 4>), g,
                         b, 0, stream, keys, vals, n, shift, cursor, ok,
                         out_vals, chunk, ovf);
      break;
    case 2048:
      hipLaunchKernelGGL((gb_part_scatter_staged_kernel_v4<KT, 2048, 2>), g,
                         b, 0, stream, keys, vals, n, shift, cursor, ok,
                         out_vals, chunk, ovf);
      break;
    default:
      hipLaunchKernelGGL((gb_part_scatter_staged_kernel_v4<KT, 512, 8>), g,
                         b, 0, stream, keys, vals, n, shift, cursor, ok,
                         out_vals, chunk, ovf);
  }
}

// SLOTS-variant dispatch for the staged aggregate: 4096 (64KB LDS, 2
// blocks/CU), 2048 (32KB, 5 blocks/CU), 1024 (16KB, 8 blocks/CU)
template <typename KT>
static void launch_agg_v4_dispatch(int slots, dim3 g, dim3 b,
                                   hipStream_t stream, const KT* pk,
                                   const double* part_vals,
                                   const int32_t* ops, int64_t n,
                                   int64_t* tkeys, double* gaggs,
                                   int64_t* gcount, int64_t tsize,
                                   int64_t chunk) {
  switch (slots) {
    case 1024:
      hipLaunchKernelGGL((gb_aggregate_part_big_kernel_v4<KT, 1024>), g, b, 0,
                         stream, pk, part_vals, ops, n, tkeys, gaggs, gcount,
                         tsize, chunk);
      break;
    case 2048:
      hipLaunchKernelGGL((gb_aggregate_part_big_kernel_v4<KT, 2048>), g, b, 0,
                         stream, pk, part_vals, ops, n, tkeys, gaggs, gcount,
                         tsize, chunk);
      break;
    default:
      hipLaunchKernelGGL((gb_aggregate_part_big_kernel_v4<KT, 4096>), g, b, 0,
                         stream, pk, part_vals, ops, n, tkeys, gaggs, gcount,
                         tsize, chunk);
  }
}

extern "C" {

void launch_gb_part_scatter_staged(const int64_t* keys, const double* vals,
                                   int64_t n, int shift, int64_t* cursor,
                                   void* out_keys, double* out_vals,
                                   int64_t chunk, int narrow, int* ovf,
                                   int num_parts, hipStream_t stream) {
  if (chunk <= 0) chunk = SCATTER_CHUNK;
  int64_t blocks = (n + chunk - 1) / chunk;
  if (blocks > MAX_GRID) blocks = MAX_GRID;
  if (blocks < 1) blocks = 1;
  dim3 g((int)blocks), b(BLOCK);
  // ovf (speculative narrow: a key fell outside [0, 2^31)) only means
  // something for int32 spill keys
  if (narrow)
    launch_scatter_v4_dispatch<int32_t>(num_parts, g, b, stream, keys, vals,
                                        n, shift, cursor, (int32_t*)out_keys,
                                        out_vals, chunk, ovf);
  else
    launch_scatter_v4_dispatch<int64_t>(num_parts, g, b, stream, keys, vals,
                                        n, shift, cursor, (int64_t*)out_keys,
                                        out_vals, chunk, nullptr);
}

void launch_gb_aggregate_part_big(const void* part_keys,
                                  const double* part_vals,
                                  const int32_t* ops, int64_t n,
                                  int64_t* tkeys, double* gaggs,
                                  int64_t* gcount, int64_t tsize,
                                  int64_t chunk, int narrow, int slots,
                                  hipStream_t stream) {
  // default chunk sweep-tuned per table size: 32K rows at 4096 slots
  // (2 blocks/CU), 16K at 2048 slots (5 blocks/CU; measured 4.03 vs
  // 4.42 ms on the 125M-row bench shape)
  if (chunk <= 0) chunk = (slots == 2048) ? (BLOCK * 64) : AGG_CHUNK;
  int64_t blocks = (n + chunk - 1) / chunk;
  if (blocks > MAX_GRID) blocks = MAX_GRID;
  if (blocks < 1) blocks = 1;
  dim3 g((int)blocks), b(BLOCK);
  if (narrow)
    launch_agg_v4_dispatch<int32_t>(slots, g, b, stream,
                                    (const int32_t*)part_keys, part_vals, ops,
                                    n, tkeys, gaggs, gcount, tsize, chunk);
  else
    launch_agg_v4_dispatch<int64_t>(slots, g, b, stream,
                                    (const int64_t*)part_keys, part_vals, ops,
                                    n, tkeys, gaggs, gcount, tsize, chunk);
}

void launch_gb_part_hist(const int64_t* keys, int64_t n, int shift,
                         int64_t* hist, int num_parts, hipStream_t stream) {
  hipLaunchKernelGGL(gb_part_hist_kernel, dim3(grid_for(n, 4)), dim3(BLOCK),
                     0, stream, keys, n, shift, hist, num_parts);
}

void launch_gb_part_scatter(const int64_t* keys, const double* vals,
                            int n_aggs, int64_t n, int shift, int64_t* cursor,
                            int64_t* out_keys, double* out_vals,
                            int num_parts, int32_t* out_pos,
                            int64_t chunk, hipStream_t stream) {
  // a layout recorded for the tile-coalesced replay scatter asks for a
  // reservation chunk equal to the replay tile (see scatter_tile_kernel)
  if (chunk <= 0) chunk = SCATTER_CHUNK;
  int64_t blocks = (n + chunk - 1) / chunk;
  if (blocks > MAX_GRID) blocks = MAX_GRID;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(gb_part_scatter_kernel, dim3((int)blocks), dim3(BLOCK),
                     0, stream, keys, vals, n_aggs, n, shift, cursor,
                     out_keys, out_vals, num_parts, out_pos, chunk);
}

void launch_gb_aggregate_part(const int64_t* part_keys,
                              const double* part_vals, const int32_t* ops,
                              int n_aggs, int64_t n, const int64_t* offsets,
                              int64_t num_parts, int64_t* tkeys,
                              double* gaggs, int64_t* gcount, int64_t tsize,
                              hipStream_t stream) {
  int grid = (int)std::min<int64_t>(num_parts, 8192);
  hipLaunchKernelGGL(gb_aggregate_part_kernel, dim3(grid), dim3(BLOCK), 0,
                     stream, part_keys, part_vals, ops, n_aggs, n, offsets,
                     num_parts, tkeys, gaggs, gcount, tsize);
}

}  // extern "C"

extern "C" {

void launch_gb_aggregate(const int64_t* keys, const double* vals,
                         const bool* valids, const int32_t* ops, int n_aggs,
                         int64_t n, int64_t* tkeys, double* gaggs,
                         int64_t* gcount, int64_t tsize, int use_lds,
                         hipStream_t stream) {
  if (use_lds && n_aggs <= 4) {
    hipLaunchKernelGGL(gb_aggregate_lds_kernel, dim3(grid_for(n, 4)),
                       dim3(BLOCK), 0, stream, keys, vals, valids, ops, n_aggs,
                       n, tkeys, gaggs, gcount, tsize);
  } else {
    hipLaunchKernelGGL(gb_aggregate_kernel, dim3(grid_for(n, 4)), dim3(BLOCK),
                       0, stream, keys, vals, valids, ops, n_aggs, n, tkeys,
                       gaggs, gcount, tsize);
  }
}

}  // extern "C"

// ------------------------------------------------------------------ //
// hash join (int64 keys): chained-bucket build + 2-pass probe         //
// ------------------------------------------------------------------ //

__global__ __launch_bounds__(BLOCK) void join_build_kernel(
    const int64_t* __restrict__ keys, int64_t n,
    int32_t* __restrict__ heads,   // [tsize] init -1
    int32_t* __restrict__ next,    // [n]
    int64_t tsize) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    uint64_t h = mix64((uint64_t)keys[i]);
    int64_t slot = (int64_t)(h & (uint64_t)(tsize - 1));
    int32_t old = atomicExch(&heads[slot], (int32_t)i);
    next[i] = old;
  }
}

// post-build pass: set dup when any key occurs twice (chains are fully
// linked here — doing this inside the build kernel would race with
// other threads' unwritten next[] entries)
__global__ __launch_bounds__(BLOCK) void join_dup_check_kernel(
    const int64_t* __restrict__ keys, int64_t n,
    const int32_t* __restrict__ heads, const int32_t* __restrict__ next,
    int64_t tsize, int32_t* __restrict__ dup) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    if (*dup != 0) return;
    int64_t key = keys[i];
    uint64_t h = mix64((uint64_t)key);
    int32_t cur = heads[(int64_t)(h & (uint64_t)(tsize - 1))];
    // a duplicate exists iff a DIFFERENT row with my key precedes me
    while (cur >= 0 && cur != (int32_t)i) {
      if (keys[cur] == key) {
        atomicOr(dup, 1);
        return;
      }
      cur = next[cur];
    }
  }
}

// single-pass emit for UNIQUE build keys (≤1 match per probe): walks
// the chain once and appends via a global cursor — replaces the
// count+scan+emit 3-kernel pipeline.  mode: 0=inner 2=semi 3=anti
// (left is handled positionally by join_left_unique_kernel).
__global__ __launch_bounds__(BLOCK) void join_emit_unique_kernel(
    const int64_t* __restrict__ pkeys, int64_t np,
    const int64_t* __restrict__ bkeys,
    const int64_t* __restrict__ ph2, const int64_t* __restrict__ bh2,
    const int32_t* __restrict__ heads, const int32_t* __restrict__ next,
    int64_t tsize, int mode,
    int64_t* __restrict__ out_pi, int64_t* __restrict__ out_bi,
    int64_t* __restrict__ cursor) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < np;
       i += stride) {
    int64_t key = pkeys[i];
    uint64_t h = mix64((uint64_t)key);
    int32_t cur = heads[(int64_t)(h & (uint64_t)(tsize - 1))];
    int32_t match = -1;
    while (cur >= 0) {
      if (bkeys[cur] == key && (ph2 == nullptr || bh2[cur] == ph2[i])) {
        match = cur;
        break;
      }
      cur = next[cur];
    }
    bool emit = mode == 3 ? (match < 0) : (match >= 0);
    // wave-aggregated cursor reservation: one atomic per 64 lanes
    unsigned long long ballot = __ballot(emit);
    if (ballot != 0ULL) {
      int lane = __lane_id();
      int leader = __ffsll((long long)ballot) - 1;
      long long base = 0;
      if (lane == leader) {
        base = (long long)atomicAdd((unsigned long long*)cursor,
                                    (unsigned long long)__popcll(ballot));
      }
      base = __shfl(base, leader);
      if (emit) {
        int64_t pos =
            base + __popcll(ballot & ((1ULL << lane) - 1ULL));
        out_pi[pos] = i;
        if (out_bi != nullptr) out_bi[pos] = mode == 3 ? -1 : match;
      }
    }
  }
}

// positional left join for unique build keys: out slot i = probe i
// ILP-4: four interleaved chain walks per thread hide the dependent
// random-load latency (heads -> bkeys/next) that bounds this kernel;
// out_pi is optional — the compaction path emits indices itself.
__global__ __launch_bounds__(BLOCK) void join_left_unique_kernel(
    const int64_t* __restrict__ pkeys, int64_t np,
    const int64_t* __restrict__ bkeys,
    const int64_t* __restrict__ ph2, const int64_t* __restrict__ bh2,
    const int32_t* __restrict__ heads, const int32_t* __restrict__ next,
    int64_t tsize,
    int64_t* __restrict__ out_pi, int64_t* __restrict__ out_bi,
    bool* __restrict__ out_mask, int mask_neg) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  uint64_t tmask = (uint64_t)(tsize - 1);
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       base < np; base += stride * 4) {
    int64_t idx[4], key[4], h2v[4];
    int32_t cur[4], match[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      idx[j] = base + (int64_t)j * stride;
      match[j] = -1;
      if (idx[j] < np) {
        key[j] = pkeys[idx[j]];
        h2v[j] = ph2 != nullptr ? ph2[idx[j]] : 0;
        cur[j] = heads[(int64_t)(mix64((uint64_t)key[j]) & tmask)];
      } else {
        cur[j] = -1;
      }
    }
    bool any = true;
    while (any) {
      any = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (cur[j] >= 0) {
          int32_t c = cur[j];
          if (bkeys[c] == key[j] && (ph2 == nullptr || bh2[c] == h2v[j])) {
            match[j] = c;
            cur[j] = -1;
          } else {
            cur[j] = next[c];
            if (cur[j] >= 0) any = true;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (idx[j] < np) {
        if (out_pi != nullptr) out_pi[idx[j]] = idx[j];
        out_bi[idx[j]] = match[j];
        if (out_mask != nullptr)
          out_mask[idx[j]] = mask_neg ? match[j] < 0 : match[j] >= 0;
      }
    }
  }
}

// pass 1: per-probe-row match count.  ph2/bh2 (optional) carry a second
// independent 64-bit hash for string keys: a match requires both hashes
// equal (128-bit verification).
__global__ __launch_bounds__(BLOCK) void join_count_kernel(
    const int64_t* __restrict__ pkeys, int64_t np,
    const int64_t* __restrict__ bkeys,
    const int64_t* __restrict__ ph2, const int64_t* __restrict__ bh2,
    const int32_t* __restrict__ heads, const int32_t* __restrict__ next,
    int64_t tsize, int32_t* __restrict__ counts) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < np;
       i += stride) {
    int64_t key = pkeys[i];
    uint64_t h = mix64((uint64_t)key);
    int32_t cur = heads[(int64_t)(h & (uint64_t)(tsize - 1))];
    int32_t c = 0;
    while (cur >= 0) {
      if (bkeys[cur] == key && (ph2 == nullptr || bh2[cur] == ph2[i])) ++c;
      cur = next[cur];
    }
    counts[i] = c;
  }
}

// pass 2: emit (probe_idx, build_idx) pairs at offsets
// mode: 0=inner 1=left (emit (i,-1) when no match) 2=semi 3=anti
__global__ __launch_bounds__(BLOCK) void join_emit_kernel(
    const int64_t* __restrict__ pkeys, int64_t np,
    const int64_t* __restrict__ bkeys,
    const int64_t* __restrict__ ph2, const int64_t* __restrict__ bh2,
    const int32_t* __restrict__ heads, const int32_t* __restrict__ next,
    int64_t tsize, const int64_t* __restrict__ offsets,
    int64_t* __restrict__ out_p, int64_t* __restrict__ out_b, int mode) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < np;
       i += stride) {
    int64_t key = pkeys[i];
    uint64_t h = mix64((uint64_t)key);
    int32_t cur = heads[(int64_t)(h & (uint64_t)(tsize - 1))];
    int64_t pos = offsets[i];
    bool any = false;
    while (cur >= 0) {
      if (bkeys[cur] == key && (ph2 == nullptr || bh2[cur] == ph2[i])) {
        any = true;
        if (mode == 0 || mode == 1) {
          out_p[pos] = i;
          out_b[pos] = cur;
          ++pos;
        } else if (mode == 2) {  // semi: first match only
          out_p[pos] = i;
          out_b[pos] = cur;
          ++pos;
          break;
        } else {  // anti: presence is enough
          break;
        }
      }
      cur = next[cur];
    }
    if (!any && (mode == 1 || mode == 3)) {
      out_p[pos] = i;
      out_b[pos] = -1;
    }
  }
}

// single-scalar total of output rows for a join mode (no per-row counts
// array, no prefix sum): per-thread count -> wave reduce -> one device
// atomic per wave
__global__ __launch_bounds__(BLOCK) void join_total_kernel(
    const int64_t* __restrict__ pkeys, int64_t np,
    const int64_t* __restrict__ bkeys,
    const int64_t* __restrict__ ph2, const int64_t* __restrict__ bh2,
    const int32_t* __restrict__ heads, const int32_t* __restrict__ next,
    int64_t tsize, int mode, int64_t* __restrict__ total) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t mine = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < np;
       i += stride) {
    int64_t key = pkeys[i];
    uint64_t h = mix64((uint64_t)key);
    int32_t cur = heads[(int64_t)(h & (uint64_t)(tsize - 1))];
    int64_t c = 0;
    while (cur >= 0) {
      if (bkeys[cur] == key && (ph2 == nullptr || bh2[cur] == ph2[i])) {
        ++c;
        if (mode >= 2) break;  // semi/anti: presence is enough
      }
      cur = next[cur];
    }
    if (mode == 0) mine += c;
    else if (mode == 1) mine += (c > 0 ? c : 1);
    else if (mode == 2) mine += (c > 0 ? 1 : 0);
    else mine += (c == 0 ? 1 : 0);
  }
  for (int off = WAVE / 2; off > 0; off >>= 1)
    mine += __shfl_down(mine, off, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0 && mine > 0)
    atomicAdd((unsigned long long*)total, (unsigned long long)mine);
}

// chunked single-reservation emit: each block counts its chunk's output
// rows (chain walk; the chunk's keys and table lines stay hot in L1/L2
// for the second walk), reserves one contiguous range with a single
// global atomic, then emits.  Replaces the per-row counts array +
// device-wide prefix sum + offset reads of the 2-pass scheme.
#define JOIN_CHUNK (BLOCK * 16)
// per-wave sub-chunks: each wave counts its rows (chain walk), does a
// wave-local exclusive scan + ONE global atomic reservation, then emits
// re-walking the same rows (hot in L1/L2).  No LDS, no cross-wave sync.
#define JOIN_SUB (JOIN_CHUNK / (BLOCK / WAVE))
__global__ __launch_bounds__(BLOCK) void join_emit_chunked_kernel(
    const int64_t* __restrict__ pkeys, int64_t np,
    const int64_t* __restrict__ bkeys,
    const int64_t* __restrict__ ph2, const int64_t* __restrict__ bh2,
    const int32_t* __restrict__ heads, const int32_t* __restrict__ next,
    int64_t tsize, int64_t* __restrict__ cursor,
    int64_t* __restrict__ out_p, int64_t* __restrict__ out_b, int mode) {
  int wave = threadIdx.x / WAVE;
  int lane = threadIdx.x & (WAVE - 1);
  for (int64_t cstart = (int64_t)blockIdx.x * JOIN_CHUNK; cstart < np;
       cstart += (int64_t)gridDim.x * JOIN_CHUNK) {
    int64_t start = cstart + (int64_t)wave * JOIN_SUB;
    int64_t end = start + JOIN_SUB;
    if (end > np) end = np;
    int64_t mine = 0;
    for (int64_t i = start + lane; i < end; i += WAVE) {
      int64_t key = pkeys[i];
      uint64_t h = mix64((uint64_t)key);
      int32_t cur = heads[(int64_t)(h & (uint64_t)(tsize - 1))];
      int c = 0;
      while (cur >= 0) {
        if (bkeys[cur] == key && (ph2 == nullptr || bh2[cur] == ph2[i])) {
          ++c;
          if (mode >= 2) break;
        }
        cur = next[cur];
      }
      if (mode == 0) mine += c;
      else if (mode == 1) mine += (c > 0 ? c : 1);
      else if (mode == 2) mine += (c > 0 ? 1 : 0);
      else mine += (c == 0 ? 1 : 0);
    }
    // wave-local inclusive scan -> exclusive offset + total
    int64_t inc = mine;
    for (int d = 1; d < WAVE; d <<= 1) {
      int64_t nv = __shfl_up(inc, d, WAVE);
      if (lane >= d) inc += nv;
    }
    int64_t tot = __shfl(inc, WAVE - 1, WAVE);
    int64_t base = 0;
    if (lane == 0 && tot > 0)
      base = (int64_t)atomicAdd((unsigned long long*)cursor,
                                (unsigned long long)tot);
    base = __shfl(base, 0, WAVE);
    if (tot == 0) continue;
    int64_t pos = base + (inc - mine);
    for (int64_t i = start + lane; i < end; i += WAVE) {
      int64_t key = pkeys[i];
      uint64_t h = mix64((uint64_t)key);
      int32_t cur = heads[(int64_t)(h & (uint64_t)(tsize - 1))];
      bool any = false;
      while (cur >= 0) {
        if (bkeys[cur] == key && (ph2 == nullptr || bh2[cur] == ph2[i])) {
          any = true;
          if (mode <= 2) {
            out_p[pos] = i;
            out_b[pos] = cur;
            ++pos;
            if (mode == 2) break;
          } else {
            break;
          }
        }
        cur = next[cur];
      }
      if (!any && (mode == 1 || mode == 3)) {
        out_p[pos] = i;
        out_b[pos] = -1;
        ++pos;
      }
    }
  }
}

// match-flag on the build side (for right/full outer): mark matched rows
__global__ __launch_bounds__(BLOCK) void join_mark_build_kernel(
    const int64_t* __restrict__ pkeys, int64_t np,
    const int64_t* __restrict__ bkeys,
    const int64_t* __restrict__ ph2, const int64_t* __restrict__ bh2,
    const int32_t* __restrict__ heads, const int32_t* __restrict__ next,
    int64_t tsize, bool* __restrict__ bmatched) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < np;
       i += stride) {
    int64_t key = pkeys[i];
    uint64_t h = mix64((uint64_t)key);
    int32_t cur = heads[(int64_t)(h & (uint64_t)(tsize - 1))];
    while (cur >= 0) {
      if (bkeys[cur] == key && (ph2 == nullptr || bh2[cur] == ph2[i]))
        bmatched[cur] = true;
      cur = next[cur];
    }
  }
}

extern "C" {

void launch_join_build(const int64_t* keys, int64_t n, int32_t* heads,
                       int32_t* next, int64_t tsize, int32_t* dup,
                       hipStream_t stream) {
  hipLaunchKernelGGL(join_build_kernel, dim3(grid_for(n)), dim3(BLOCK), 0,
                     stream, keys, n, heads, next, tsize);
  if (dup != nullptr) {
    hipLaunchKernelGGL(join_dup_check_kernel, dim3(grid_for(n)), dim3(BLOCK),
                       0, stream, keys, n, heads, next, tsize, dup);
  }
}

void launch_join_emit_unique(const int64_t* pkeys, int64_t np,
                             const int64_t* bkeys, const int64_t* ph2,
                             const int64_t* bh2, const int32_t* heads,
                             const int32_t* next, int64_t tsize, int mode,
                             int64_t* out_pi, int64_t* out_bi,
                             int64_t* cursor, bool* out_mask, int mask_neg,
                             hipStream_t stream) {
  if (mode == 1) {
    hipLaunchKernelGGL(join_left_unique_kernel, dim3(grid_for(np, 4)),
                       dim3(BLOCK), 0, stream, pkeys, np, bkeys, ph2, bh2,
                       heads, next, tsize, out_pi, out_bi, out_mask,
                       mask_neg);
  } else {
    hipLaunchKernelGGL(join_emit_unique_kernel, dim3(grid_for(np)),
                       dim3(BLOCK), 0, stream, pkeys, np, bkeys, ph2, bh2,
                       heads, next, tsize, mode, out_pi, out_bi, cursor);
  }
}

void launch_join_count(const int64_t* pkeys, int64_t np, const int64_t* bkeys,
                       const int64_t* ph2, const int64_t* bh2,
                       const int32_t* heads, const int32_t* next,
                       int64_t tsize, int32_t* counts, hipStream_t stream) {
  hipLaunchKernelGGL(join_count_kernel, dim3(grid_for(np)), dim3(BLOCK), 0,
                     stream, pkeys, np, bkeys, ph2, bh2, heads, next, tsize,
                     counts);
}

void launch_join_total(const int64_t* pkeys, int64_t np,
                       const int64_t* bkeys, const int64_t* ph2,
                       const int64_t* bh2, const int32_t* heads,
                       const int32_t* next, int64_t tsize, int mode,
                       int64_t* total, hipStream_t stream) {
  hipLaunchKernelGGL(join_total_kernel, dim3(grid_for(np, 4)), dim3(BLOCK), 0,
                     stream, pkeys, np, bkeys, ph2, bh2, heads, next, tsize,
                     mode, total);
}

void launch_join_emit_chunked(const int64_t* pkeys, int64_t np,
                              const int64_t* bkeys, const int64_t* ph2,
                              const int64_t* bh2, const int32_t* heads,
                              const int32_t* next, int64_t tsize,
                              int64_t* cursor, int64_t* out_p,
                              int64_t* out_b, int mode, hipStream_t stream) {
  int64_t blocks = (np + JOIN_CHUNK - 1) / JOIN_CHUNK;
  if (blocks > MAX_GRID) blocks = MAX_GRID;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(join_emit_chunked_kernel, dim3((int)blocks), dim3(BLOCK),
                     0, stream, pkeys, np, bkeys, ph2, bh2, heads, next,
                     tsize, cursor, out_p, out_b, mode);
}

void launch_join_emit(const int64_t* pkeys, int64_t np, const int64_t* bkeys,
                      const int64_t* ph2, const int64_t* bh2,
                      const int32_t* heads, const int32_t* next, int64_t tsize,
                      const int64_t* offsets, int64_t* out_p, int64_t* out_b,
                      int mode, hipStream_t stream) {
  hipLaunchKernelGGL(join_emit_kernel, dim3(grid_for(np)), dim3(BLOCK), 0,
                     stream, pkeys, np, bkeys, ph2, bh2, heads, next, tsize,
                     offsets, out_p, out_b, mode);
}

void launch_join_mark_build(const int64_t* pkeys, int64_t np,
                            const int64_t* bkeys, const int64_t* ph2,
                            const int64_t* bh2, const int32_t* heads,
                            const int32_t* next, int64_t tsize, bool* bmatched,
                            hipStream_t stream) {
  hipLaunchKernelGGL(join_mark_build_kernel, dim3(grid_for(np)), dim3(BLOCK),
                     0, stream, pkeys, np, bkeys, ph2, bh2, heads, next,
                     tsize, bmatched);
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

// representative-row + second-hash verification pass for hashed
// (string-keyed) group-by: probes the table built by gb_aggregate over
// h1, records one representative row per slot and flags h2 mismatches
// (h1 collision between distinct keys → caller falls back).
__global__ __launch_bounds__(BLOCK) void gb_mark_reps_kernel(
    const int64_t* __restrict__ h1,
    const int64_t* __restrict__ h2,
    const int64_t* __restrict__ tkeys,
    int64_t tsize,
    int64_t* __restrict__ rep,      // [tsize] init -1
    int64_t* __restrict__ th2,      // [tsize] init GB_EMPTY
    int64_t* __restrict__ conflict, // [1]
    int64_t n) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t key = h1[i];
    uint64_t h = mix64((uint64_t)key);
    int64_t slot = (int64_t)(h & (uint64_t)(tsize - 1));
    while (tkeys[slot] != key) slot = (slot + 1) & (tsize - 1);
    atomicCAS((unsigned long long*)&rep[slot],
              (unsigned long long)(int64_t)-1, (unsigned long long)i);
    long long prev = (long long)atomicCAS((unsigned long long*)&th2[slot],
                                          (unsigned long long)GB_EMPTY,
                                          (unsigned long long)h2[i]);
    if (prev != GB_EMPTY && prev != h2[i])
      atomicAdd((unsigned long long*)conflict, 1ULL);
  }
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

void launch_gb_mark_reps(const int64_t* h1, const int64_t* h2,
                         const int64_t* tkeys, int64_t tsize, int64_t* rep,
                         int64_t* th2, int64_t* conflict, int64_t n,
                         hipStream_t stream) {
  hipLaunchKernelGGL(gb_mark_reps_kernel, dim3(grid_for(n)), dim3(BLOCK), 0,
                     stream, h1, h2, tkeys, tsize, rep, th2, conflict, n);
}

}  // extern "C"

// ------------------------------------------------------------------ //
// fused stream compaction: write the masked rows of up to 8 eight-byte
// columns in one pass.  Each block reserves a contiguous output range
// for its chunk (one global atomic), so writes coalesce; output order is
// block-nondeterministic (frames are unordered collections).
// ------------------------------------------------------------------ //
#define COMPACT_CHUNK (BLOCK * 16)

__global__ __launch_bounds__(BLOCK) void compact8_kernel(
    const bool* __restrict__ mask, int64_t n,
    int64_t* __restrict__ cursor,  // [1]
    const uint64_t* __restrict__ s0, const uint64_t* __restrict__ s1,
    const uint64_t* __restrict__ s2, const uint64_t* __restrict__ s3,
    const uint64_t* __restrict__ s4, const uint64_t* __restrict__ s5,
    const uint64_t* __restrict__ s6, const uint64_t* __restrict__ s7,
    uint64_t* __restrict__ d0, uint64_t* __restrict__ d1,
    uint64_t* __restrict__ d2, uint64_t* __restrict__ d3,
    uint64_t* __restrict__ d4, uint64_t* __restrict__ d5,
    uint64_t* __restrict__ d6, uint64_t* __restrict__ d7,
    int ncols) {
  const uint64_t* srcs[8] = {s0, s1, s2, s3, s4, s5, s6, s7};
  uint64_t* dsts[8] = {d0, d1, d2, d3, d4, d5, d6, d7};
  __shared__ int lcount;
  __shared__ long long lbase;
  for (int64_t start = (int64_t)blockIdx.x * COMPACT_CHUNK; start < n;
       start += (int64_t)gridDim.x * COMPACT_CHUNK) {
    int64_t end = start + COMPACT_CHUNK;
    if (end > n) end = n;
    if (threadIdx.x == 0) lcount = 0;
    __syncthreads();
    int local = 0;
    for (int64_t i = start + threadIdx.x; i < end; i += blockDim.x)
      if (mask[i]) ++local;
    atomicAdd(&lcount, local);
    __syncthreads();
    if (threadIdx.x == 0) {
      lbase = lcount > 0
                  ? (long long)atomicAdd((unsigned long long*)cursor,
                                         (unsigned long long)lcount)
                  : 0;
      lcount = 0;
    }
    __syncthreads();
    for (int64_t i = start + threadIdx.x; i < end; i += blockDim.x) {
      if (!mask[i]) continue;
      int64_t pos = (int64_t)lbase + atomicAdd(&lcount, 1);
      for (int c = 0; c < ncols; ++c)
        dsts[c][pos] = srcs[c] != nullptr ? srcs[c][i] : (uint64_t)i;
    }
    __syncthreads();
  }
}

extern "C" {

void launch_compact8(const bool* mask, int64_t n, int64_t* cursor,
                     const uint64_t** srcs, uint64_t** dsts, int ncols,
                     hipStream_t stream) {
  int64_t blocks = (n + COMPACT_CHUNK - 1) / COMPACT_CHUNK;
  if (blocks > MAX_GRID) blocks = MAX_GRID;
  if (blocks < 1) blocks = 1;
  const uint64_t* z = nullptr;
  hipLaunchKernelGGL(
      compact8_kernel, dim3((int)blocks), dim3(BLOCK), 0, stream, mask, n,
      cursor, ncols > 0 ? srcs[0] : z, ncols > 1 ? srcs[1] : z,
      ncols > 2 ? srcs[2] : z, ncols > 3 ? srcs[3] : z,
      ncols > 4 ? srcs[4] : z, ncols > 5 ? srcs[5] : z,
      ncols > 6 ? srcs[6] : z, ncols > 7 ? srcs[7] : z,
      ncols > 0 ? dsts[0] : nullptr, ncols > 1 ? dsts[1] : nullptr,
      ncols > 2 ? dsts[2] : nullptr, ncols > 3 ? dsts[3] : nullptr,
      ncols > 4 ? dsts[4] : nullptr, ncols > 5 ? dsts[5] : nullptr,
      ncols > 6 ? dsts[6] : nullptr, ncols > 7 ? dsts[7] : nullptr, ncols);
}

}  // extern "C"

// ------------------------------------------------------------------ //
// fused key-column min/max + pack (group-by key preparation)          //
//                                                                     //
// Replaces the torch residue measured in profiles/NOTES.md r02: per   //
// key column min().item() + max().item() (2 reduce kernels + 2 host   //
// syncs EACH) and the 6+ elementwise shift/or/where packing ops.      //
// One pass computes all columns' min/max (one host read), a second    //
// packs every column into the int64 group key.                        //
// ------------------------------------------------------------------ //

struct PackCols {
  const void* data[8];   // int64/int32/int16 per dwidth
  const bool* valid[8];  // may be null
  int dwidth[8];         // element bytes: 8, 4 or 2
  int64_t mins[8];       // pack phase only
  int shifts[8];         // pack phase only
};

__device__ __forceinline__ int64_t pc_load(const PackCols& pc, int c,
                                           int64_t i) {
  switch (pc.dwidth[c]) {
    case 8:
      return ((const int64_t*)pc.data[c])[i];
    case 4:
      return (int64_t)((const int32_t*)pc.data[c])[i];
    default:
      return (int64_t)((const int16_t*)pc.data[c])[i];
  }
}

// signed→unsigned order-preserving map so atomicMin/Max work on u64
__device__ __forceinline__ uint64_t s2u(int64_t v) {
  return (uint64_t)v ^ 0x8000000000000000ULL;
}

__global__ __launch_bounds__(BLOCK) void minmax_init_kernel(
    uint64_t* __restrict__ out, int ncols) {
  int i = threadIdx.x;
  if (i < ncols) {
    out[2 * i] = ~0ULL;      // min slot: u64 max
    out[2 * i + 1] = 0ULL;   // max slot: u64 min
  }
}

template <int NC>
__global__ __launch_bounds__(BLOCK) void minmax_cols_kernel(
    PackCols pc, int64_t n, uint64_t* __restrict__ out) {
  uint64_t lmin[NC], lmax[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    lmin[c] = ~0ULL;
    lmax[c] = 0ULL;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      uint64_t u = s2u(pc_load(pc, c, i));
      lmin[c] = u < lmin[c] ? u : lmin[c];
      lmax[c] = u > lmax[c] ? u : lmax[c];
    }
  }
  // wave reduce -> LDS -> one atomic per block per col (same-address
  // atomics serialize in L2 even wave-aggregated — profiles/NOTES.md)
  __shared__ uint64_t smin[NC][BLOCK / WAVE];
  __shared__ uint64_t smax[NC][BLOCK / WAVE];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    for (int off = WAVE / 2; off > 0; off >>= 1) {
      uint64_t omin = __shfl_down(lmin[c], off, WAVE);
      uint64_t omax = __shfl_down(lmax[c], off, WAVE);
      lmin[c] = omin < lmin[c] ? omin : lmin[c];
      lmax[c] = omax > lmax[c] ? omax : lmax[c];
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
      smin[c][threadIdx.x / WAVE] = lmin[c];
      smax[c][threadIdx.x / WAVE] = lmax[c];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      uint64_t bmin = smin[c][0], bmax = smax[c][0];
      for (int w = 1; w < BLOCK / WAVE; ++w) {
        bmin = smin[c][w] < bmin ? smin[c][w] : bmin;
        bmax = smax[c][w] > bmax ? smax[c][w] : bmax;
      }
      atomicMin((unsigned long long*)&out[2 * c], bmin);
      atomicMax((unsigned long long*)&out[2 * c + 1], bmax);
    }
  }
}

template <int NC>
__global__ __launch_bounds__(BLOCK) void pack_cols_kernel(
    PackCols pc, int64_t n, int64_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t packed = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      int64_t code = pc_load(pc, c, i) - pc.mins[c] + 1;  // 0 = NULL
      if (pc.valid[c] != nullptr && !pc.valid[c][i]) code = 0;
      packed |= code << pc.shifts[c];
    }
    out[i] = packed;
  }
}

// unpack one column out of the packed group key (code 0 = NULL)
__global__ __launch_bounds__(BLOCK) void unpack_col_kernel(
    const int64_t* __restrict__ packed, int64_t n, int shift, int64_t mask,
    int64_t lo, int dwidth, int has_nulls, void* __restrict__ out,
    bool* __restrict__ valid) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t code = (packed[i] >> shift) & mask;
    int64_t v = code - 1 + lo;
    if (has_nulls) valid[i] = code != 0;
    switch (dwidth) {
      case 8:
        ((int64_t*)out)[i] = v;
        break;
      case 4:
        ((int32_t*)out)[i] = (int32_t)v;
        break;
      default:
        ((int16_t*)out)[i] = (int16_t)v;
        break;
    }
  }
}


static void launch_minmax_dispatch(int ncols, dim3 g, dim3 b,
                                   hipStream_t stream, PackCols pc,
                                   int64_t n, uint64_t* out) {
  switch (ncols) {
    case 1: hipLaunchKernelGGL(minmax_cols_kernel<1>, g, b, 0, stream, pc, n, out); break;
    case 2: hipLaunchKernelGGL(minmax_cols_kernel<2>, g, b, 0, stream, pc, n, out); break;
    case 3: hipLaunchKernelGGL(minmax_cols_kernel<3>, g, b, 0, stream, pc, n, out); break;
    case 4: hipLaunchKernelGGL(minmax_cols_kernel<4>, g, b, 0, stream, pc, n, out); break;
    case 5: hipLaunchKernelGGL(minmax_cols_kernel<5>, g, b, 0, stream, pc, n, out); break;
    case 6: hipLaunchKernelGGL(minmax_cols_kernel<6>, g, b, 0, stream, pc, n, out); break;
    case 7: hipLaunchKernelGGL(minmax_cols_kernel<7>, g, b, 0, stream, pc, n, out); break;
    default: hipLaunchKernelGGL(minmax_cols_kernel<8>, g, b, 0, stream, pc, n, out); break;
  }
}

static void launch_pack_dispatch(int ncols, dim3 g, dim3 b,
                                 hipStream_t stream, PackCols pc, int64_t n,
                                 int64_t* out) {
  switch (ncols) {
    case 1: hipLaunchKernelGGL(pack_cols_kernel<1>, g, b, 0, stream, pc, n, out); break;
    case 2: hipLaunchKernelGGL(pack_cols_kernel<2>, g, b, 0, stream, pc, n, out); break;
    case 3: hipLaunchKernelGGL(pack_cols_kernel<3>, g, b, 0, stream, pc, n, out); break;
    case 4: hipLaunchKernelGGL(pack_cols_kernel<4>, g, b, 0, stream, pc, n, out); break;
    case 5: hipLaunchKernelGGL(pack_cols_kernel<5>, g, b, 0, stream, pc, n, out); break;
    case 6: hipLaunchKernelGGL(pack_cols_kernel<6>, g, b, 0, stream, pc, n, out); break;
    case 7: hipLaunchKernelGGL(pack_cols_kernel<7>, g, b, 0, stream, pc, n, out); break;
    default: hipLaunchKernelGGL(pack_cols_kernel<8>, g, b, 0, stream, pc, n, out); break;
  }
}

extern "C" {

void launch_pack_cols(const void** data, const bool** valid,
                      const int* dwidth, const int64_t* mins,
                      const int* shifts, int ncols, int64_t n, int64_t* out,
                      hipStream_t stream) {
  PackCols pc;
  memset(&pc, 0, sizeof(pc));
  for (int c = 0; c < ncols; ++c) {
    pc.data[c] = data[c];
    pc.valid[c] = valid[c];
    pc.dwidth[c] = dwidth[c];
    pc.mins[c] = mins[c];
    pc.shifts[c] = shifts[c];
  }
  launch_pack_dispatch(ncols, dim3(grid_for(n, 2)), dim3(BLOCK), stream, pc,
                       n, out);
}

void launch_unpack_col(const int64_t* packed, int64_t n, int shift,
                       int64_t mask, int64_t lo, int dwidth, int has_nulls,
                       void* out, bool* valid, hipStream_t stream) {
  hipLaunchKernelGGL(unpack_col_kernel, dim3(grid_for(n, 2)), dim3(BLOCK), 0,
                     stream, packed, n, shift, mask, lo, dwidth, has_nulls,
                     out, valid);
}

}  // extern "C"

// ------------------------------------------------------------------ //
// sampled distinct-count estimator (Chao83 inputs d/f1/f2)            //
//                                                                     //
// Replaces the torch.unique(sample) path (rocPRIM merge-sort + multi  //
// sync) with one hash-insert pass + one table scan; the host reads a  //
// single 3-element tensor.                                            //
// ------------------------------------------------------------------ //

#define DS_EMPTY 0x8000000000000001LL  // improbable sentinel key

__device__ __forceinline__ uint64_t pc_row_hash(const PackCols& pc,
                                                int ncols, int64_t i) {
  uint64_t h = 0x9e3779b97f4a7c15ULL;
  for (int c = 0; c < ncols; ++c) {
    uint64_t v = (uint64_t)pc_load(pc, c, i);
    if (pc.valid[c] != nullptr && !pc.valid[c][i]) v = 0xdeadULL;
    h = hash_combine(h, v);
  }
  return h;
}

__global__ __launch_bounds__(BLOCK) void distinct_init_kernel(
    int64_t* __restrict__ slots, int32_t* __restrict__ counts, int tsize,
    int64_t* __restrict__ out3) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 3) out3[i] = 0;
  for (; i < tsize; i += gridDim.x * blockDim.x) {
    slots[i] = DS_EMPTY;
    counts[i] = 0;
  }
}

__global__ __launch_bounds__(BLOCK) void distinct_insert_kernel(
    PackCols pc, int ncols, int64_t nsamples, int64_t stride,
    int64_t* __restrict__ slots, int32_t* __restrict__ counts, int tmask) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       s < nsamples; s += (int64_t)gridDim.x * blockDim.x) {
    int64_t k = (int64_t)pc_row_hash(pc, ncols, s * stride);
    if (k == DS_EMPTY) k ^= 1;  // estimator: sentinel remap is harmless
    uint32_t h = (uint32_t)mix64((uint64_t)k) & tmask;
    for (;;) {
      int64_t prev = (int64_t)atomicCAS((unsigned long long*)&slots[h],
                                        (unsigned long long)DS_EMPTY,
                                        (unsigned long long)k);
      if (prev == DS_EMPTY || prev == k) {
        atomicAdd(&counts[h], 1);
        break;
      }
      h = (h + 1) & tmask;
    }
  }
}

__global__ __launch_bounds__(BLOCK) void distinct_stats_kernel(
    const int32_t* __restrict__ counts, int tsize,
    int64_t* __restrict__ out3) {
  int d = 0, f1 = 0, f2 = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < tsize;
       i += gridDim.x * blockDim.x) {
    int c = counts[i];
    if (c > 0) ++d;
    if (c == 1) ++f1;
    if (c == 2) ++f2;
  }
  __shared__ int sd[BLOCK / WAVE], sf1[BLOCK / WAVE], sf2[BLOCK / WAVE];
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    d += __shfl_down(d, off, WAVE);
    f1 += __shfl_down(f1, off, WAVE);
    f2 += __shfl_down(f2, off, WAVE);
  }
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    sd[threadIdx.x / WAVE] = d;
    sf1[threadIdx.x / WAVE] = f1;
    sf2[threadIdx.x / WAVE] = f2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < BLOCK / WAVE; ++w) {
      d += sd[w];
      f1 += sf1[w];
      f2 += sf2[w];
    }
    atomicAdd((unsigned long long*)&out3[0], (unsigned long long)d);
    atomicAdd((unsigned long long*)&out3[1], (unsigned long long)f1);
    atomicAdd((unsigned long long*)&out3[2], (unsigned long long)f2);
  }
}

extern "C" {

// One fused launch set for group-by key preparation: per-column min/max
// (first 2*ncols slots of `out`) and a sampled distinct-row estimate
// (d, f1, f2 in the last 3 slots).  The host reads `out` ONCE — this
// replaces 2 reduce kernels + 2 syncs per key column plus a
// torch.unique (rocPRIM sort) sampling pass (profiles/NOTES.md r02).
void launch_gb_key_stats(const void** data, const bool** valid,
                         const int* dwidth, int ncols, int64_t n,
                         int64_t nsamples, int64_t* slots, int32_t* counts,
                         int tsize, int do_minmax, uint64_t* out,
                         hipStream_t stream) {
  PackCols pc;
  memset(&pc, 0, sizeof(pc));
  for (int c = 0; c < ncols; ++c) {
    pc.data[c] = data[c];
    pc.valid[c] = valid[c];
    pc.dwidth[c] = dwidth[c];
  }
  int64_t* out3 = (int64_t*)out + 2 * ncols;
  if (do_minmax) {
    hipLaunchKernelGGL(minmax_init_kernel, dim3(1), dim3(BLOCK), 0, stream,
                       out, ncols);
    int mg = grid_for(n, 8);
    if (mg > 4096) mg = 4096;
    launch_minmax_dispatch(ncols, dim3(mg), dim3(BLOCK), stream, pc, n, out);
  }
  int64_t stride = n / nsamples;
  if (stride < 1) stride = 1;
  int64_t eff = n / stride;
  if (eff > nsamples) eff = nsamples;
  hipLaunchKernelGGL(distinct_init_kernel, dim3(grid_for(tsize)), dim3(BLOCK),
                     0, stream, slots, counts, tsize, out3);
  hipLaunchKernelGGL(distinct_insert_kernel, dim3(grid_for(eff)), dim3(BLOCK),
                     0, stream, pc, ncols, eff, stride, slots, counts,
                     tsize - 1);
  hipLaunchKernelGGL(distinct_stats_kernel, dim3(grid_for(tsize)),
                     dim3(BLOCK), 0, stream, counts, tsize, out3);
}

}  // extern "C"

// ------------------------------------------------------------------ //
// deterministic group-table compaction                                //
//                                                                     //
// Replaces occupied = (tkeys != EMPTY).nonzero() + per-column          //
// index_select with a 3-kernel own pipeline (count / scan / emit) that //
// preserves slot order (deterministic output) and moves each byte      //
// once.  total lands in bases[nblocks] for a single host read.         //
// ------------------------------------------------------------------ //

#define GBC_CHUNK (BLOCK * 32)

__global__ __launch_bounds__(BLOCK) void gbc_count_kernel(
    const int64_t* __restrict__ tkeys, int64_t tsize,
    int64_t* __restrict__ bcounts) {
  __shared__ int lcount;
  int64_t start = (int64_t)blockIdx.x * GBC_CHUNK;
  if (threadIdx.x == 0) lcount = 0;
  __syncthreads();
  int64_t end = start + GBC_CHUNK < tsize ? start + GBC_CHUNK : tsize;
  int local = 0;
  for (int64_t i = start + threadIdx.x; i < end; i += blockDim.x)
    if (tkeys[i] != GB_EMPTY) ++local;
  atomicAdd(&lcount, local);
  __syncthreads();
  if (threadIdx.x == 0) bcounts[blockIdx.x] = lcount;
}

// single-block exclusive scan of bcounts (nblocks <= 65536); writes the
// total into bases[nblocks]
__global__ __launch_bounds__(BLOCK) void gbc_scan_kernel(
    const int64_t* __restrict__ bcounts, int nblocks,
    int64_t* __restrict__ bases) {
  __shared__ int64_t carry;
  __shared__ int64_t tile[BLOCK];
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int t0 = 0; t0 < nblocks; t0 += BLOCK) {
    int i = t0 + threadIdx.x;
    int64_t v = i < nblocks ? bcounts[i] : 0;
    tile[threadIdx.x] = v;
    __syncthreads();
    // inclusive scan in LDS
    for (int off = 1; off < BLOCK; off <<= 1) {
      int64_t add = threadIdx.x >= off ? tile[threadIdx.x - off] : 0;
      __syncthreads();
      tile[threadIdx.x] += add;
      __syncthreads();
    }
    if (i < nblocks) bases[i] = carry + tile[threadIdx.x] - v;  // exclusive
    __syncthreads();
    if (threadIdx.x == 0) carry += tile[BLOCK - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) bases[nblocks] = carry;  // total
}

struct GbcAggs {
  const double* src[6];
  double* dst[6];
};

__global__ __launch_bounds__(BLOCK) void gbc_emit_kernel(
    const int64_t* __restrict__ tkeys, const int64_t* __restrict__ gcount,
    GbcAggs ag, int n_aggs, int64_t tsize,
    const int64_t* __restrict__ bases, int64_t* __restrict__ out_keys,
    int64_t* __restrict__ out_count, const int64_t* __restrict__ extra_src,
    int64_t* __restrict__ extra_dst) {
  __shared__ int64_t wbase[BLOCK / WAVE];
  __shared__ int64_t sbase;
  int64_t start = (int64_t)blockIdx.x * GBC_CHUNK;
  int64_t end = start + GBC_CHUNK < tsize ? start + GBC_CHUNK : tsize;
  if (threadIdx.x == 0) sbase = bases[blockIdx.x];
  int wave = threadIdx.x / WAVE;
  int lane = threadIdx.x % WAVE;
  __syncthreads();
  for (int64_t i0 = start; i0 < end; i0 += blockDim.x) {
    int64_t i = i0 + threadIdx.x;
    bool occ = i < end && tkeys[i] != GB_EMPTY;
    uint64_t mask = __ballot(occ);
    int rank = __popcll(mask & ((1ULL << lane) - 1ULL));
    if (lane == 0) wbase[wave] = __popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
      int64_t acc = sbase;
      for (int w = 0; w < BLOCK / WAVE; ++w) {
        int64_t c = wbase[w];
        wbase[w] = acc;
        acc += c;
      }
      sbase = acc;
    }
    __syncthreads();
    if (occ) {
      int64_t pos = wbase[wave] + rank;
      out_keys[pos] = tkeys[i];
      out_count[pos] = gcount[i];
      if (extra_src != nullptr) extra_dst[pos] = extra_src[i];
      for (int a = 0; a < n_aggs; ++a) ag.dst[a][pos] = ag.src[a][i];
    }
    __syncthreads();
  }
}

extern "C" {

void launch_gb_compact(const int64_t* tkeys, const int64_t* gcount,
                       const double** agg_src, double** agg_dst, int n_aggs,
                       int64_t tsize, int64_t* bcounts, int64_t* bases,
                       int64_t* out_keys, int64_t* out_count,
                       const int64_t* extra_src, int64_t* extra_dst,
                       hipStream_t stream) {
  int nblocks = (int)((tsize + GBC_CHUNK - 1) / GBC_CHUNK);
  hipLaunchKernelGGL(gbc_count_kernel, dim3(nblocks), dim3(BLOCK), 0, stream,
                     tkeys, tsize, bcounts);
  hipLaunchKernelGGL(gbc_scan_kernel, dim3(1), dim3(BLOCK), 0, stream,
                     bcounts, nblocks, bases);
  GbcAggs ag;
  memset(&ag, 0, sizeof(ag));
  for (int a = 0; a < n_aggs; ++a) {
    ag.src[a] = agg_src[a];
    ag.dst[a] = agg_dst[a];
  }
  hipLaunchKernelGGL(gbc_emit_kernel, dim3(nblocks), dim3(BLOCK), 0, stream,
                     tkeys, gcount, ag, n_aggs, tsize, bases, out_keys,
                     out_count, extra_src, extra_dst);
}

}  // extern "C"

// ------------------------------------------------------------------ //
// segmented rank over a sorted permutation                            //
//                                                                     //
// perm is a stable sort permutation by (partition key, order keys);   //
// pkeys and the order columns stay in original row order and are      //
// gathered through perm.  Sorted position i carries a head flag (new  //
// partition) and a peer flag (new partition or any order column       //
// differs from position i-1).  From those:                            //
//   row_number = i - seg_start + 1                                    //
//   rank       = peer_start - seg_start + 1                           //
//   dense_rank = #peer flags in [seg_start, i]                        //
// Window mode scatters the rank to out[perm[i]] (original row order); //
// take mode keeps row_number <= n_take and emits the kept perm values //
// in sorted order through count -> gbc_scan_kernel -> emit.           //
//                                                                     //
// Chunks of SEG_CHUNK positions are chained by separate launches      //
// (summary -> single-block scan -> apply): no block ever waits for    //
// another block inside a launch.                                      //
// ------------------------------------------------------------------ //

#define SEG_CHUNK (BLOCK * 32)
#define SEG_ITERS (SEG_CHUNK / BLOCK)
#define SEG_MAX_COLS 4
#define SEG_WAVES (BLOCK / WAVE)

struct SegCols {
  const int64_t* data[SEG_MAX_COLS];   // 8-byte values, original row order
  const uint8_t* valid[SEG_MAX_COLS];  // optional validity, nullptr = all
  int is_float[SEG_MAX_COLS];          // compare as double (NaN == NaN)
};

// (last head position, last peer position, peer flags since that head)
// of a range of sorted positions; seg < 0 means the range has no head
// and cnt counts every peer flag of the range.
struct SegAgg {
  int64_t seg;
  int64_t peer;
  int64_t cnt;
};

__device__ __forceinline__ SegAgg seg_combine(SegAgg a, SegAgg b) {
  SegAgg r;
  r.seg = b.seg >= 0 ? b.seg : a.seg;
  r.peer = b.peer >= 0 ? b.peer : a.peer;
  r.cnt = b.seg >= 0 ? b.cnt : a.cnt + b.cnt;
  return r;
}

__device__ __forceinline__ int64_t seg_row(const int64_t* __restrict__ perm,
                                           int64_t i, int64_t n) {
  int64_t j = perm[i];
  // a malformed permutation must not read or write out of bounds
  return (uint64_t)j < (uint64_t)n ? j : 0;
}

// head/peer flags of sorted position i.  Neighbouring lanes hand their
// gathered values down with a shuffle; lane 0 fetches its predecessor.
// Must be called by every lane of the wave.
__device__ __forceinline__ void seg_flags(
    const int64_t* __restrict__ perm, const int64_t* __restrict__ pkeys,
    const SegCols& oc, int ncols, int64_t i, int64_t n, int lane, int64_t& j,
    bool& h, bool& p) {
  bool in = i < n;
  j = in ? seg_row(perm, i, n) : 0;
  bool fetch_prev = in && lane == 0 && i > 0;
  int64_t jp = fetch_prev ? seg_row(perm, i - 1, n) : 0;
  int64_t k = in ? pkeys[j] : 0;
  int64_t kp = __shfl_up(k, 1);
  if (fetch_prev) kp = pkeys[jp];
  h = in && (i == 0 || k != kp);
  bool diff = false;
  for (int c = 0; c < ncols; ++c) {
    const int64_t* d = oc.data[c];
    const uint8_t* vd = oc.valid[c];
    int64_t v = in ? d[j] : 0;
    int ok = (in && vd != nullptr) ? (int)(vd[j] != 0) : 1;
    int64_t vp = __shfl_up(v, 1);
    int okp = __shfl_up(ok, 1);
    if (fetch_prev) {
      vp = d[jp];
      okp = vd != nullptr ? (int)(vd[jp] != 0) : 1;
    }
    bool eq;
    if (ok && okp) {
      if (oc.is_float[c]) {
        double a = __longlong_as_double(v), b = __longlong_as_double(vp);
        eq = a == b || (a != a && b != b);
      } else {
        eq = v == vp;
      }
    } else {
      eq = ok == okp;  // null/null equal, null/value different
    }
    diff |= !eq;
  }
  p = in && (h || diff);
}

__device__ __forceinline__ int seg_top_bit(uint64_t m) {
  return 63 - __clzll((long long)m);
}

// Resolve (seg_start, peer_start, dense count) of this lane's position
// from the block's flags.  carry is the aggregate of everything before
// this iteration's 256 positions and is advanced past them; ws is the
// LDS exchange buffer of this iteration's parity (double-buffered by the
// caller, so one barrier per call is enough).  Block-uniform call.
__device__ __forceinline__ SegAgg seg_block_step(bool h, bool p, int64_t i0,
                                                 int lane, int wave,
                                                 SegAgg& carry, SegAgg* ws) {
  uint64_t hmask = __ballot(h);
  uint64_t pmask = __ballot(p);
  int64_t w0 = i0 + (int64_t)wave * WAVE;
  if (lane == 0) {
    SegAgg s;
    if (hmask != 0) {
      int hb = seg_top_bit(hmask);
      s.seg = w0 + hb;
      s.cnt = __popcll(pmask >> hb);
    } else {
      s.seg = -1;
      s.cnt = __popcll(pmask);
    }
    s.peer = pmask != 0 ? w0 + seg_top_bit(pmask) : -1;
    ws[wave] = s;
  }
  __syncthreads();
  SegAgg in = carry;
  SegAgg tot = carry;
#pragma unroll
  for (int w = 0; w < SEG_WAVES; ++w) {
    SegAgg s = ws[w];
    if (w < wave) in = seg_combine(in, s);
    tot = seg_combine(tot, s);
  }
  carry = tot;
  uint64_t le = (2ULL << lane) - 1ULL;  // lanes <= this one
  uint64_t mh = hmask & le, mp = pmask & le;
  SegAgg r;
  if (mh != 0) {
    int hb = seg_top_bit(mh);
    r.seg = w0 + hb;
    r.cnt = __popcll(mp >> hb);
  } else {
    r.seg = in.seg;
    r.cnt = in.cnt + __popcll(mp);
  }
  r.peer = mp != 0 ? w0 + seg_top_bit(mp) : in.peer;
  return r;
}

// per-chunk aggregate of the flags
__global__ __launch_bounds__(BLOCK) void seg_rank_summary_kernel(
    const int64_t* __restrict__ perm, const int64_t* __restrict__ pkeys,
    SegCols oc, int ncols, int64_t n, int64_t* __restrict__ sum_seg,
    int64_t* __restrict__ sum_peer, int64_t* __restrict__ sum_cnt) {
  __shared__ int s_head, s_peer, s_cnt;
  int64_t start = (int64_t)blockIdx.x * SEG_CHUNK;
  int lane = threadIdx.x % WAVE;
  if (threadIdx.x == 0) {
    s_head = -1;
    s_peer = -1;
    s_cnt = 0;
  }
  __syncthreads();
  uint32_t pbits = 0;
  int lhead = -1, lpeer = -1;
#pragma unroll 4
  for (int it = 0; it < SEG_ITERS; ++it) {
    int rel = it * BLOCK + (int)threadIdx.x;
    int64_t i = start + rel;
    if (start + (int64_t)it * BLOCK >= n) break;  // block-uniform
    int64_t j;
    bool h, p;
    seg_flags(perm, pkeys, oc, ncols, i, n, lane, j, h, p);
    if (h) lhead = rel;
    if (p) {
      lpeer = rel;
      pbits |= 1u << it;
    }
  }
  if (lhead >= 0) atomicMax(&s_head, lhead);
  if (lpeer >= 0) atomicMax(&s_peer, lpeer);
  __syncthreads();
  int bhead = s_head;
  // peer flags at or after the chunk's last head (all of them if none):
  // this thread's positions are it*BLOCK + tid
  int local = 0;
  if (bhead < 0) {
    local = __popc(pbits);
  } else {
    int it0 = bhead / BLOCK;
    if ((int)threadIdx.x < bhead % BLOCK) ++it0;
    local = it0 < 32 ? __popc(pbits >> it0) : 0;
  }
  if (local) atomicAdd(&s_cnt, local);
  __syncthreads();
  if (threadIdx.x == 0) {
    sum_seg[blockIdx.x] = bhead >= 0 ? start + bhead : -1;
    sum_peer[blockIdx.x] = s_peer >= 0 ? start + s_peer : -1;
    sum_cnt[blockIdx.x] = s_cnt;
  }
}

// single-block exclusive segmented scan of the chunk aggregates: chunk b
// receives the aggregate of chunks [0, b)
__global__ __launch_bounds__(BLOCK) void seg_rank_scan_kernel(
    const int64_t* __restrict__ sum_seg, const int64_t* __restrict__ sum_peer,
    const int64_t* __restrict__ sum_cnt, int nblocks,
    int64_t* __restrict__ car_seg, int64_t* __restrict__ car_peer,
    int64_t* __restrict__ car_cnt) {
  __shared__ SegAgg tile[BLOCK];
  SegAgg carry;  // same value in every thread
  carry.seg = -1;
  carry.peer = -1;
  carry.cnt = 0;
  for (int t0 = 0; t0 < nblocks; t0 += BLOCK) {
    int i = t0 + (int)threadIdx.x;
    SegAgg v;
    v.seg = -1;
    v.peer = -1;
    v.cnt = 0;
    if (i < nblocks) {
      v.seg = sum_seg[i];
      v.peer = sum_peer[i];
      v.cnt = sum_cnt[i];
    }
    tile[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < BLOCK; off <<= 1) {
      SegAgg self = tile[threadIdx.x];
      bool has = (int)threadIdx.x >= off;
      SegAgg left = self;
      if (has) left = tile[threadIdx.x - off];
      __syncthreads();
      if (has) tile[threadIdx.x] = seg_combine(left, self);
      __syncthreads();
    }
    if (i < nblocks) {
      SegAgg e = carry;
      if (threadIdx.x > 0) e = seg_combine(carry, tile[threadIdx.x - 1]);
      car_seg[i] = e.seg;
      car_peer[i] = e.peer;
      car_cnt[i] = e.cnt;
    }
    carry = seg_combine(carry, tile[BLOCK - 1]);
    __syncthreads();
  }
}

// window mode: kind 0 row_number, 1 rank, 2 dense_rank
__global__ __launch_bounds__(BLOCK) void seg_rank_apply_kernel(
    const int64_t* __restrict__ perm, const int64_t* __restrict__ pkeys,
    SegCols oc, int ncols, int64_t n, const int64_t* __restrict__ car_seg,
    const int64_t* __restrict__ car_peer, const int64_t* __restrict__ car_cnt,
    int kind, int64_t* __restrict__ out) {
  __shared__ SegAgg ws[2][SEG_WAVES];
  int64_t start = (int64_t)blockIdx.x * SEG_CHUNK;
  int lane = threadIdx.x % WAVE;
  int wave = threadIdx.x / WAVE;
  SegAgg carry;
  carry.seg = car_seg[blockIdx.x];
  carry.peer = car_peer[blockIdx.x];
  carry.cnt = car_cnt[blockIdx.x];
  for (int it = 0; it < SEG_ITERS; ++it) {
    int64_t i0 = start + (int64_t)it * BLOCK;
    if (i0 >= n) break;  // block-uniform
    int64_t i = i0 + threadIdx.x;
    int64_t j;
    bool h, p;
    seg_flags(perm, pkeys, oc, ncols, i, n, lane, j, h, p);
    SegAgg r = seg_block_step(h, p, i0, lane, wave, carry, ws[it & 1]);
    if (i < n) {
      int64_t v = kind == 0 ? i - r.seg + 1
                            : (kind == 1 ? r.peer - r.seg + 1 : r.cnt);
      out[j] = v;
    }
  }
}

// take mode, pass 1: kept rows per chunk
__global__ __launch_bounds__(BLOCK) void seg_take_count_kernel(
    const int64_t* __restrict__ perm, const int64_t* __restrict__ pkeys,
    SegCols oc, int64_t n, const int64_t* __restrict__ car_seg,
    int64_t n_take, int64_t* __restrict__ bcounts) {
  __shared__ SegAgg ws[2][SEG_WAVES];
  __shared__ int lcount;
  int64_t start = (int64_t)blockIdx.x * SEG_CHUNK;
  int lane = threadIdx.x % WAVE;
  int wave = threadIdx.x / WAVE;
  if (threadIdx.x == 0) lcount = 0;
  SegAgg carry;
  carry.seg = car_seg[blockIdx.x];
  carry.peer = -1;
  carry.cnt = 0;
  int local = 0;
  for (int it = 0; it < SEG_ITERS; ++it) {
    int64_t i0 = start + (int64_t)it * BLOCK;
    if (i0 >= n) break;  // block-uniform
    int64_t i = i0 + threadIdx.x;
    int64_t j;
    bool h, p;
    seg_flags(perm, pkeys, oc, 0, i, n, lane, j, h, p);
    SegAgg r = seg_block_step(h, p, i0, lane, wave, carry, ws[it & 1]);
    if (i < n && i - r.seg < n_take) ++local;
  }
  __syncthreads();
  if (local) atomicAdd(&lcount, local);
  __syncthreads();
  if (threadIdx.x == 0) bcounts[blockIdx.x] = lcount;
}

// take mode, pass 2: emit kept perm values in sorted order
__global__ __launch_bounds__(BLOCK) void seg_take_emit_kernel(
    const int64_t* __restrict__ perm, const int64_t* __restrict__ pkeys,
    SegCols oc, int64_t n, const int64_t* __restrict__ car_seg,
    int64_t n_take, const int64_t* __restrict__ bases, int64_t cap,
    int64_t* __restrict__ out) {
  __shared__ SegAgg ws[2][SEG_WAVES];
  __shared__ int wkeep[2][SEG_WAVES];
  int64_t start = (int64_t)blockIdx.x * SEG_CHUNK;
  int lane = threadIdx.x % WAVE;
  int wave = threadIdx.x / WAVE;
  SegAgg carry;
  carry.seg = car_seg[blockIdx.x];
  carry.peer = -1;
  carry.cnt = 0;
  int64_t base = bases[blockIdx.x];  // same value in every thread
  for (int it = 0; it < SEG_ITERS; ++it) {
    int64_t i0 = start + (int64_t)it * BLOCK;
    if (i0 >= n) break;  // block-uniform
    int64_t i = i0 + threadIdx.x;
    int64_t j;
    bool h, p;
    seg_flags(perm, pkeys, oc, 0, i, n, lane, j, h, p);
    SegAgg r = seg_block_step(h, p, i0, lane, wave, carry, ws[it & 1]);
    bool keep = i < n && i - r.seg < n_take;
    uint64_t mask = __ballot(keep);
    int rank = __popcll(mask & ((1ULL << lane) - 1ULL));
    if (lane == 0) wkeep[it & 1][wave] = __popcll(mask);
    __syncthreads();
    int64_t pos = base;
    int tot = 0;
#pragma unroll
    for (int w = 0; w < SEG_WAVES; ++w) {
      int c = wkeep[it & 1][w];
      if (w < wave) pos += c;
      tot += c;
    }
    base += tot;
    pos += rank;
    if (keep && pos < cap) out[pos] = j;
  }
}

extern "C" {

int64_t seg_rank_chunk_size() { return SEG_CHUNK; }

static SegCols seg_make_cols(const int64_t* const* col_data,
                             const uint8_t* const* col_valid,
                             const int* col_is_float, int ncols) {
  SegCols oc;
  memset(&oc, 0, sizeof(oc));
  for (int c = 0; c < ncols; ++c) {
    oc.data[c] = col_data[c];
    oc.valid[c] = col_valid[c];
    oc.is_float[c] = col_is_float[c];
  }
  return oc;
}

// work: 6 * nblocks int64 (chunk aggregates, then chunk carries)
void launch_seg_rank(const int64_t* perm, const int64_t* pkeys,
                     const int64_t* const* col_data,
                     const uint8_t* const* col_valid, const int* col_is_float,
                     int ncols, int64_t n, int kind, int64_t* work,
                     int64_t* out, hipStream_t stream) {
  if (n <= 0) return;
  int nblocks = (int)((n + SEG_CHUNK - 1) / SEG_CHUNK);
  SegCols oc = seg_make_cols(col_data, col_valid, col_is_float, ncols);
  int64_t* w = work;
  hipLaunchKernelGGL(seg_rank_summary_kernel, dim3(nblocks), dim3(BLOCK), 0,
                     stream, perm, pkeys, oc, ncols, n, w, w + nblocks,
                     w + 2 * (int64_t)nblocks);
  hipLaunchKernelGGL(seg_rank_scan_kernel, dim3(1), dim3(BLOCK), 0, stream, w,
                     w + nblocks, w + 2 * (int64_t)nblocks, nblocks,
                     w + 3 * (int64_t)nblocks, w + 4 * (int64_t)nblocks,
                     w + 5 * (int64_t)nblocks);
  hipLaunchKernelGGL(seg_rank_apply_kernel, dim3(nblocks), dim3(BLOCK), 0,
                     stream, perm, pkeys, oc, ncols, n,
                     w + 3 * (int64_t)nblocks, w + 4 * (int64_t)nblocks,
                     w + 5 * (int64_t)nblocks, kind, out);
}

// work: 6 * nblocks int64; bcounts: nblocks; bases: nblocks + 1 (total in
// bases[nblocks]); out: capacity n
void launch_seg_take(const int64_t* perm, const int64_t* pkeys, int64_t n,
                     int64_t n_take, int64_t* work, int64_t* bcounts,
                     int64_t* bases, int64_t* out, hipStream_t stream) {
  if (n <= 0) return;
  int nblocks = (int)((n + SEG_CHUNK - 1) / SEG_CHUNK);
  SegCols oc;
  memset(&oc, 0, sizeof(oc));
  int64_t* w = work;
  hipLaunchKernelGGL(seg_rank_summary_kernel, dim3(nblocks), dim3(BLOCK), 0,
                     stream, perm, pkeys, oc, 0, n, w, w + nblocks,
                     w + 2 * (int64_t)nblocks);
  hipLaunchKernelGGL(seg_rank_scan_kernel, dim3(1), dim3(BLOCK), 0, stream, w,
                     w + nblocks, w + 2 * (int64_t)nblocks, nblocks,
                     w + 3 * (int64_t)nblocks, w + 4 * (int64_t)nblocks,
                     w + 5 * (int64_t)nblocks);
  hipLaunchKernelGGL(seg_take_count_kernel, dim3(nblocks), dim3(BLOCK), 0,
                     stream, perm, pkeys, oc, n, w + 3 * (int64_t)nblocks,
                     n_take, bcounts);
  hipLaunchKernelGGL(gbc_scan_kernel, dim3(1), dim3(BLOCK), 0, stream, bcounts,
                     nblocks, bases);
  hipLaunchKernelGGL(seg_take_emit_kernel, dim3(nblocks), dim3(BLOCK), 0,
                     stream, perm, pkeys, oc, n, w + 3 * (int64_t)nblocks,
                     n_take, bases, n, out);
}

}  // extern "C"

// ------------------------------------------------------------------ //
// fast single-comparison filters                                      //
//                                                                     //
// The general expr_filter interpreter keeps its value stack in        //
// scratch memory (dynamically indexed), which costs ~10x SOL on a     //
// simple `col < imm` predicate (profiles r02c).  Single comparisons   //
// — the dominant WHERE shape — get dedicated one-pass kernels.        //
// ------------------------------------------------------------------ //

template <typename CT>
__device__ __forceinline__ bool cmp_apply(CT a, CT b, int op) {
  switch (op) {
    case 0: return a == b;
    case 1: return a != b;
    case 2: return a < b;
    case 3: return a <= b;
    case 4: return a > b;
    default: return a >= b;
  }
}

// col vs immediate; CT is the comparison domain (int64_t or double)
template <typename T, typename CT>
__global__ __launch_bounds__(BLOCK) void cmp_imm_kernel(
    const T* __restrict__ a, const bool* __restrict__ valid, CT imm, int op,
    int64_t n, bool* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    bool r = cmp_apply<CT>((CT)a[i], imm, op);
    out[i] = (valid == nullptr || valid[i]) && r;
  }
}

// col vs col (same storage type); comparison in CT
template <typename T, typename CT>
__global__ __launch_bounds__(BLOCK) void cmp_col_kernel(
    const T* __restrict__ a, const bool* __restrict__ va,
    const T* __restrict__ b, const bool* __restrict__ vb, int op, int64_t n,
    bool* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    bool r = cmp_apply<CT>((CT)a[i], (CT)b[i], op);
    out[i] = (va == nullptr || va[i]) && (vb == nullptr || vb[i]) && r;
  }
}

extern "C" {

// dtype codes: 0 i64, 1 i32, 2 i16, 3 f64, 4 f32 (int compare domain for
// 0-2 with an integral immediate, double otherwise)
void launch_cmp_imm(const void* a, const bool* valid, int dtype,
                    int64_t imm_i, double imm_d, int use_int, int op,
                    int64_t n, bool* out, hipStream_t stream) {
  dim3 g(grid_for(n, 4)), b(BLOCK);
#define CI(T)                                                              \
  if (use_int) {                                                           \
    hipLaunchKernelGGL((cmp_imm_kernel<T, int64_t>), g, b, 0, stream,      \
                       (const T*)a, valid, (int64_t)imm_i, op, n, out);    \
  } else {                                                                 \
    hipLaunchKernelGGL((cmp_imm_kernel<T, double>), g, b, 0, stream,       \
                       (const T*)a, valid, imm_d, op, n, out);             \
  }
  switch (dtype) {
    case 0: CI(int64_t) break;
    case 1: CI(int32_t) break;
    case 2: CI(int16_t) break;
    case 3: CI(double) break;
    default: CI(float) break;
  }
#undef CI
}

void launch_cmp_col(const void* a, const bool* va, const void* b,
                    const bool* vb, int dtype, int op, int64_t n, bool* out,
                    hipStream_t stream) {
  dim3 g(grid_for(n, 4)), blk(BLOCK);
  switch (dtype) {
    case 0:
      hipLaunchKernelGGL((cmp_col_kernel<int64_t, int64_t>), g, blk, 0,
                         stream, (const int64_t*)a, va, (const int64_t*)b,
                         vb, op, n, out);
      break;
    case 1:
      hipLaunchKernelGGL((cmp_col_kernel<int32_t, int64_t>), g, blk, 0,
                         stream, (const int32_t*)a, va, (const int32_t*)b,
                         vb, op, n, out);
      break;
    case 2:
      hipLaunchKernelGGL((cmp_col_kernel<int16_t, int64_t>), g, blk, 0,
                         stream, (const int16_t*)a, va, (const int16_t*)b,
                         vb, op, n, out);
      break;
    case 3:
      hipLaunchKernelGGL((cmp_col_kernel<double, double>), g, blk, 0,
                         stream, (const double*)a, va, (const double*)b, vb,
                         op, n, out);
      break;
    default:
      hipLaunchKernelGGL((cmp_col_kernel<float, double>), g, blk, 0, stream,
                         (const float*)a, va, (const float*)b, vb, op, n,
                         out);
      break;
  }
}

}  // extern "C"

// 128-bit string-equality mask: (h1==l1 && h2==l2 [&& valid]) ^ neg,
// literal hashes read from device memory (no host sync, no torch
// compare_scalar residue).
__global__ __launch_bounds__(BLOCK) void eq2_mask_kernel(
    const int64_t* __restrict__ h1, const int64_t* __restrict__ h2,
    const int64_t* __restrict__ l1, const int64_t* __restrict__ l2,
    const bool* __restrict__ valid, int neg, int64_t n,
    bool* __restrict__ out) {
  int64_t a = l1[0], b = l2[0];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    bool eq = h1[i] == a && h2[i] == b;
    if (neg) eq = !eq;
    out[i] = eq && (valid == nullptr || valid[i]);
  }
}

extern "C" {
void launch_eq2_mask(const int64_t* h1, const int64_t* h2, const int64_t* l1,
                     const int64_t* l2, const bool* valid, int neg,
                     int64_t n, bool* out, hipStream_t stream) {
  hipLaunchKernelGGL(eq2_mask_kernel, dim3(grid_for(n, 4)), dim3(BLOCK), 0,
                     stream, h1, h2, l1, l2, valid, neg, n, out);
}
}  // extern "C"

// ------------------------------------------------------------------ //
// own top-k select (k <= 16): torch.topk's rocPRIM path runs a        //
// merge-sort cascade (~0.3 ms/step on q3's LIMIT 10); two own passes  //
// — per-thread register top-k + LDS log-merge per block, then one     //
// block over the per-block candidates — read the data once.          //
// ------------------------------------------------------------------ //

#define TOPK_MAX 16
#define TOPK_BLOCKS 512

template <typename T, bool LARGEST>
__device__ __forceinline__ bool tk_before(T a, int64_t ia, T b, int64_t ib) {
  // strict ordering with index tiebreak (deterministic)
  if (a != b) return LARGEST ? (a > b) : (a < b);
  return ia < ib;
}

template <typename T, bool LARGEST>
__device__ void tk_insert(T v, int64_t idx, T* tv, int64_t* ti, int k) {
  if (ti[k - 1] >= 0 && !tk_before<T, LARGEST>(v, idx, tv[k - 1], ti[k - 1]))
    return;
  int p = k - 1;
  while (p > 0 &&
         (ti[p - 1] < 0 || tk_before<T, LARGEST>(v, idx, tv[p - 1], ti[p - 1]))) {
    tv[p] = tv[p - 1];
    ti[p] = ti[p - 1];
    --p;
  }
  tv[p] = v;
  ti[p] = idx;
}

// merge two sorted k-lists (a <- top k of a ∪ b); idx<0 marks empty
template <typename T, bool LARGEST>
__device__ void tk_merge(T* av, int64_t* ai, const T* bv, const int64_t* bi,
                         int k) {
  T mv[TOPK_MAX];
  int64_t mi[TOPK_MAX];
  int pa = 0, pb = 0;
  for (int o = 0; o < k; ++o) {
    bool take_a;
    if (pa < k && ai[pa] >= 0) {
      take_a = !(pb < k && bi[pb] >= 0) ||
               tk_before<T, LARGEST>(av[pa], ai[pa], bv[pb], bi[pb]);
    } else {
      take_a = false;
    }
    if (take_a) {
      mv[o] = av[pa];
      mi[o] = ai[pa];
      ++pa;
    } else if (pb < k && bi[pb] >= 0) {
      mv[o] = bv[pb];
      mi[o] = bi[pb];
      ++pb;
    } else {
      mi[o] = -1;
    }
  }
  for (int o = 0; o < k; ++o) {
    av[o] = mv[o];
    ai[o] = mi[o];
  }
}

template <typename T, bool LARGEST>
__global__ __launch_bounds__(BLOCK) void topk_stage1_kernel(
    const T* __restrict__ vals, int64_t n, int k, T* __restrict__ cand_v,
    int64_t* __restrict__ cand_i) {
  __shared__ T sv[BLOCK * TOPK_MAX];
  __shared__ int64_t si[BLOCK * TOPK_MAX];
  T tv[TOPK_MAX];
  int64_t ti[TOPK_MAX];
  for (int j = 0; j < k; ++j) ti[j] = -1;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    tk_insert<T, LARGEST>(vals[i], i, tv, ti, k);
  for (int j = 0; j < k; ++j) {
    sv[threadIdx.x * k + j] = tv[j];
    si[threadIdx.x * k + j] = ti[j];
  }
  __syncthreads();
  for (int stride = 1; stride < BLOCK; stride <<= 1) {
    if ((threadIdx.x & (2 * stride - 1)) == 0) {
      tk_merge<T, LARGEST>(&sv[threadIdx.x * k], &si[threadIdx.x * k],
                           &sv[(threadIdx.x + stride) * k],
                           &si[(threadIdx.x + stride) * k], k);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    for (int j = 0; j < k; ++j) {
      cand_v[blockIdx.x * k + j] = sv[j];
      cand_i[blockIdx.x * k + j] = si[j];
    }
  }
}

template <typename T, bool LARGEST>
__global__ __launch_bounds__(BLOCK) void topk_stage2_kernel(
    const T* __restrict__ cand_v, const int64_t* __restrict__ cand_i,
    int nblocks, int k, T* __restrict__ out_v, int64_t* __restrict__ out_i) {
  __shared__ T sv[BLOCK * TOPK_MAX];
  __shared__ int64_t si[BLOCK * TOPK_MAX];
  T tv[TOPK_MAX];
  int64_t ti[TOPK_MAX];
  for (int j = 0; j < k; ++j) ti[j] = -1;
  int64_t total = (int64_t)nblocks * k;
  for (int64_t i = threadIdx.x; i < total; i += blockDim.x)
    if (cand_i[i] >= 0)
      tk_insert<T, LARGEST>(cand_v[i], cand_i[i], tv, ti, k);
  for (int j = 0; j < k; ++j) {
    sv[threadIdx.x * k + j] = tv[j];
    si[threadIdx.x * k + j] = ti[j];
  }
  __syncthreads();
  for (int stride = 1; stride < BLOCK; stride <<= 1) {
    if ((threadIdx.x & (2 * stride - 1)) == 0) {
      tk_merge<T, LARGEST>(&sv[threadIdx.x * k], &si[threadIdx.x * k],
                           &sv[(threadIdx.x + stride) * k],
                           &si[(threadIdx.x + stride) * k], k);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    for (int j = 0; j < k; ++j) {
      out_v[j] = sv[j];
      out_i[j] = si[j];
    }
  }
}

static void launch_topk_dispatch(int dtype, int largest, dim3 g1, dim3 b,
                                 hipStream_t stream, const void* vals,
                                 int64_t n, int k, void* cand_v,
                                 int64_t* cand_i, void* out_v,
                                 int64_t* out_i) {
#define TK(T, L)                                                            \
  do {                                                                      \
    hipLaunchKernelGGL((topk_stage1_kernel<T, L>), g1, b, 0, stream,        \
                       (const T*)vals, n, k, (T*)cand_v, cand_i);           \
    hipLaunchKernelGGL((topk_stage2_kernel<T, L>), dim3(1), b, 0, stream,   \
                       (const T*)cand_v, cand_i, (int)g1.x, k, (T*)out_v,   \
                       out_i);                                              \
  } while (0)
  if (dtype == 0) {
    if (largest) TK(int64_t, true); else TK(int64_t, false);
  } else {
    if (largest) TK(double, true); else TK(double, false);
  }
#undef TK
}

extern "C" {
void launch_topk(const void* vals, int dtype, int largest, int64_t n, int k,
                 void* cand_v, int64_t* cand_i, void* out_v, int64_t* out_i,
                 hipStream_t stream) {
  int blocks = grid_for(n, 8);
  if (blocks > TOPK_BLOCKS) blocks = TOPK_BLOCKS;
  launch_topk_dispatch(dtype, largest, dim3(blocks), dim3(BLOCK), stream,
                       vals, n, k, cand_v, cand_i, out_v, out_i);
}
}  // extern "C"

// ------------------------------------------------------------------ //
// open-addressed unique join (int64 keys, no h2)                      //
//                                                                     //
// The chained layout costs ~3 random cache lines per probe (heads ->  //
// bkeys -> next); a 16-byte (key, idx) entry costs ~1 line at 50%     //
// load factor.  Reserved key sentinel: a build key equal to it sets   //
// a flag and the caller falls back to the chained join (read in the   //
// same single sync as the dup flag).                                  //
// ------------------------------------------------------------------ //

#define JOA_EMPTY 0x8000000000000000LL

__global__ __launch_bounds__(BLOCK) void joinoa_init_kernel(
    int64_t* __restrict__ table, int64_t tsize) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tsize;
       i += (int64_t)gridDim.x * blockDim.x) {
    table[2 * i] = JOA_EMPTY;
  }
}

__global__ __launch_bounds__(BLOCK) void joinoa_build_kernel(
    const int64_t* __restrict__ bkeys, int64_t nb,
    int64_t* __restrict__ table, int64_t tsize,
    int64_t* __restrict__ flags) {  // flags[0]=dup, flags[1]=sentinel
  uint64_t tmask = (uint64_t)(tsize - 1);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nb;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t k = bkeys[i];
    if (k == JOA_EMPTY) {
      flags[1] = 1;  // racy write of constant is fine
      continue;
    }
    uint64_t h = mix64((uint64_t)k) & tmask;
    for (;;) {
      int64_t prev = (int64_t)atomicCAS((unsigned long long*)&table[2 * h],
                                        (unsigned long long)JOA_EMPTY,
                                        (unsigned long long)k);
      if (prev == JOA_EMPTY) {
        table[2 * h + 1] = i;  // idx read only after this kernel completes
        break;
      }
      if (prev == k) {
        flags[0] = 1;  // duplicate build key
        break;
      }
      h = (h + 1) & tmask;
    }
  }
}

// ILP-4 positional probe: out_bi[i] = build idx or -1; optional pi/mask
__global__ __launch_bounds__(BLOCK) void joinoa_probe_kernel(
    const int64_t* __restrict__ pkeys, int64_t np,
    const int64_t* __restrict__ table, int64_t tsize,
    int64_t* __restrict__ out_pi, int64_t* __restrict__ out_bi,
    bool* __restrict__ out_mask, int mask_neg) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  uint64_t tmask = (uint64_t)(tsize - 1);
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       base < np; base += stride * 4) {
    int64_t idx[4], key[4], match[4];
    uint64_t h[4];
    bool act[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      idx[j] = base + (int64_t)j * stride;
      match[j] = -1;
      act[j] = idx[j] < np;
      if (act[j]) {
        key[j] = pkeys[idx[j]];
        h[j] = mix64((uint64_t)key[j]) & tmask;
      }
    }
    bool any = true;
    while (any) {
      any = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (act[j]) {
          int64_t k = table[2 * h[j]];
          if (k == key[j]) {
            match[j] = table[2 * h[j] + 1];
            act[j] = false;
          } else if (k == JOA_EMPTY) {
            act[j] = false;
          } else {
            h[j] = (h[j] + 1) & tmask;
            any = true;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (idx[j] < np) {
        if (out_pi != nullptr) out_pi[idx[j]] = idx[j];
        out_bi[idx[j]] = match[j];
        if (out_mask != nullptr)
          out_mask[idx[j]] = mask_neg ? match[j] < 0 : match[j] >= 0;
      }
    }
  }
}

extern "C" {

void launch_joinoa_build(const int64_t* bkeys, int64_t nb, int64_t* table,
                         int64_t tsize, int64_t* flags, hipStream_t stream) {
  hipLaunchKernelGGL(joinoa_init_kernel, dim3(grid_for(tsize, 2)),
                     dim3(BLOCK), 0, stream, table, tsize);
  if (nb > 0) {
    hipLaunchKernelGGL(joinoa_build_kernel, dim3(grid_for(nb)), dim3(BLOCK),
                       0, stream, bkeys, nb, table, tsize, flags);
  }
}

void launch_joinoa_probe(const int64_t* pkeys, int64_t np,
                         const int64_t* table, int64_t tsize,
                         int64_t* out_pi, int64_t* out_bi, bool* out_mask,
                         int mask_neg, hipStream_t stream) {
  hipLaunchKernelGGL(joinoa_probe_kernel, dim3(grid_for(np, 4)), dim3(BLOCK),
                     0, stream, pkeys, np, table, tsize, out_pi, out_bi,
                     out_mask, mask_neg);
}

}  // extern "C"


// ------------------------------------------------------------------ //
// shuffle-layout reuse (Spark shuffle-reuse analog)                   //
//                                                                     //
// Re-aggregating the SAME key column with fresh values (iterative     //
// pipelines) skips hist + key scatter entirely.  Two replay forms:    //
//                                                                     //
//  * plain replay (any single aggregate): the recorded per-row spill  //
//    position places the new values (scatter_by_pos_kernel) and the   //
//    cached partitioned keys feed phase 3 unchanged.                  //
//  * dense replay (single SUM over a null-free fp64 column): with the //
//    keys fixed, the set of groups, their counts, their output order  //
//    and each row's group are fixed too.  They are computed ONCE when //
//    the layout is recorded (gb_dense_count/assign kernels: a dense   //
//    int32 group id per partitioned row, partition-major and          //
//    key-ascending inside a partition, plus the output keys/counts),  //
//    so a replayed step is the tile-coalesced value scatter           //
//    (scatter_tile_kernel) and one LDS f64 add per row                //
//    (gb_dense_aggregate_kernel): no keys, hashing, CAS, counting,    //
//    table fills, compaction or host readback.                        //
// ------------------------------------------------------------------ //

__global__ __launch_bounds__(BLOCK) void scatter_by_pos_kernel(
    const double* __restrict__ vals, const int32_t* __restrict__ pos,
    int64_t n, double* __restrict__ out_vals) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    out_vals[pos[i]] = vals[i];
  }
}

extern "C" {
void launch_scatter_by_pos(const double* vals, const int32_t* pos, int64_t n,
                           double* out_vals, hipStream_t stream) {
  hipLaunchKernelGGL(scatter_by_pos_kernel, dim3(grid_for(n, 2)), dim3(BLOCK),
                     0, stream, vals, pos, n, out_vals);
}
}  // extern "C"


// ------------------------------------------------------------------ //
// dense replay: one-time preparation                                  //
// ------------------------------------------------------------------ //

// LDS table used to assign ids inside one partition; a partition with
// more than DENSE_ASSIGN_MAX distinct keys declines the dense layout
// (the caller keeps the plain replay).  The racy capacity check can
// overshoot by one insert per thread, which still leaves the table
// far from full, so probing always terminates.
#define DENSE_ASSIGN_SLOTS 4096
#define DENSE_ASSIGN_MAX 2048
#define DENSE_ASSIGN_POISON (1 << 20)

// in-place ascending bitonic sort of n (power of 2) LDS elements by the
// whole block; ends with a barrier
template <typename T>
__device__ __forceinline__ void lds_bitonic_sort(T* x, int n) {
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (n >> 1); t += blockDim.x) {
        int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        int l = i | j;
        bool up = (i & k) == 0;
        T a = x[i], b = x[l];
        if ((a > b) == up) {
          x[i] = b;
          x[l] = a;
        }
      }
      __syncthreads();
    }
  }
}

// distinct keys of rows [lo, hi) into the LDS set lkeys (pre-filled
// with GB_EMPTY); *ndist counts them.  A key equal to the sentinel
// poisons the count so that the partition is declined.
__device__ __forceinline__ void dense_insert_keys(
    const int64_t* __restrict__ pkeys, int64_t lo, int64_t hi,
    int64_t* __restrict__ lkeys, int* __restrict__ ndist) {
  for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
    int64_t key = pkeys[i];
    if (key == GB_EMPTY) {
      atomicAdd(ndist, DENSE_ASSIGN_POISON);
      continue;
    }
    int slot = (int)(mix64((uint64_t)key) & (DENSE_ASSIGN_SLOTS - 1));
    for (int probe = 0; probe < DENSE_ASSIGN_SLOTS; ++probe) {
      int64_t cur = lkeys[slot];
      if (cur == key) break;
      if (cur == GB_EMPTY) {
        if (*(volatile int*)ndist > DENSE_ASSIGN_MAX) break;  // declined
        int64_t prev = (int64_t)lds_key_cas(&lkeys[slot], (int64_t)GB_EMPTY, key);
        if (prev == GB_EMPTY) {
          atomicAdd(ndist, 1);
          break;
        }
        if (prev == key) break;
      }
      slot = (slot + 1) & (DENSE_ASSIGN_SLOTS - 1);
    }
  }
}

// pass 1: distinct keys per partition (one block per partition)
__global__ __launch_bounds__(BLOCK) void gb_dense_count_kernel(
    const int64_t* __restrict__ pkeys, const int64_t* __restrict__ offsets,
    int num_parts, int64_t* __restrict__ distinct) {
  __shared__ int64_t lkeys[DENSE_ASSIGN_SLOTS];
  __shared__ int ndist;
  for (int p = blockIdx.x; p < num_parts; p += gridDim.x) {
    for (int i = threadIdx.x; i < DENSE_ASSIGN_SLOTS; i += blockDim.x)
      lkeys[i] = GB_EMPTY;
    if (threadIdx.x == 0) ndist = 0;
    __syncthreads();
    dense_insert_keys(pkeys, offsets[p], offsets[p + 1], lkeys, &ndist);
    __syncthreads();
    if (threadIdx.x == 0) distinct[p] = ndist;
    __syncthreads();
  }
}

// pass 2 (only when no partition was declined): sort the partition's
// distinct keys, id = group_base[p] + rank of the key; writes the dense
// id of every partitioned row and the output keys/counts in id order
__global__ __launch_bounds__(BLOCK) void gb_dense_assign_kernel(
    const int64_t* __restrict__ pkeys, const int64_t* __restrict__ offsets,
    const int64_t* __restrict__ group_base, int num_parts,
    int32_t* __restrict__ gid, int64_t* __restrict__ out_keys,
    int64_t* __restrict__ out_count) {
  __shared__ int64_t lkeys[DENSE_ASSIGN_SLOTS];
  __shared__ int lcount[DENSE_ASSIGN_MAX];
  __shared__ int ndist;
  for (int p = blockIdx.x; p < num_parts; p += gridDim.x) {
    for (int i = threadIdx.x; i < DENSE_ASSIGN_SLOTS; i += blockDim.x)
      lkeys[i] = GB_EMPTY;
    for (int i = threadIdx.x; i < DENSE_ASSIGN_MAX; i += blockDim.x)
      lcount[i] = 0;
    if (threadIdx.x == 0) ndist = 0;
    __syncthreads();
    int64_t lo = offsets[p], hi = offsets[p + 1];
    dense_insert_keys(pkeys, lo, hi, lkeys, &ndist);
    __syncthreads();
    int d = ndist;
    if (d > DENSE_ASSIGN_MAX) d = 0;  // not reached: pass 1 declined
    // GB_EMPTY is INT64_MIN: empties sort first, keys fill the tail
    lds_bitonic_sort<int64_t>(lkeys, DENSE_ASSIGN_SLOTS);
    const int64_t* sorted = lkeys + (DENSE_ASSIGN_SLOTS - d);
    int64_t gb = group_base[p];
    if (d > 0) {
      for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        int64_t key = pkeys[i];
        int a = 0, b = d - 1;  // key is present: lower bound
        while (a < b) {
          int mid = (a + b) >> 1;
          if (sorted[mid] < key) a = mid + 1; else b = mid;
        }
        gid[i] = (int32_t)(gb + a);
        atomicAdd(&lcount[a], 1);
      }
    }
    __syncthreads();
    for (int r = threadIdx.x; r < d; r += blockDim.x) {
      out_keys[gb + r] = sorted[r];
      out_count[gb + r] = lcount[r];
    }
    __syncthreads();
  }
}

// Tile-coalesced value scatter, preparation: per tile of C input rows,
// sort the rows by destination.  rank[i] = tile-local rank of row i,
// dst[tile*C + r] = destination of the tile's r-th ranked row.  Works
// for any permutation `pos`; with a layout recorded at a reservation
// chunk equal to C, the rows of one (tile, partition) are consecutive
// ranks with consecutive destinations.
__global__ __launch_bounds__(BLOCK) void scatter_tile_prep_kernel(
    const int32_t* __restrict__ pos, int64_t n, int C,
    uint16_t* __restrict__ rank, int32_t* __restrict__ dst) {
  extern __shared__ unsigned long long tile_sort[];
  int64_t ntiles = (n + C - 1) / C;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int64_t t0 = tile * C;
    int cnt = (int)((n - t0) < (int64_t)C ? (n - t0) : (int64_t)C);
    for (int i = threadIdx.x; i < C; i += blockDim.x) {
      tile_sort[i] = i < cnt ? (((unsigned long long)(uint32_t)pos[t0 + i]
                                 << 16) | (unsigned long long)i)
                             : ~0ULL;
    }
    __syncthreads();
    lds_bitonic_sort<unsigned long long>(tile_sort, C);
    for (int r = threadIdx.x; r < cnt; r += blockDim.x) {
      unsigned long long e = tile_sort[r];
      dst[t0 + r] = (int32_t)(e >> 16);
      rank[t0 + (int)(e & 0xffffULL)] = (uint16_t)r;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ //
// dense replay: per-step kernels                                      //
// ------------------------------------------------------------------ //

// out[dst[tile*C + r]] = value of the tile's r-th ranked row: values are
// loaded coalesced, permuted through LDS, and leave with consecutive
// lanes on consecutive ranks, so the rows of one (tile, partition) run
// are one contiguous segment instead of isolated 8-byte stores.
__global__ __launch_bounds__(BLOCK) void scatter_tile_kernel(
    const double* __restrict__ vals, const uint16_t* __restrict__ rank,
    const int32_t* __restrict__ dst, int64_t n, int C,
    double* __restrict__ out) {
  extern __shared__ double tile_vals[];
  int64_t ntiles = (n + C - 1) / C;
  const int stride = blockDim.x;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int64_t t0 = tile * C;
    int cnt = (int)((n - t0) < (int64_t)C ? (n - t0) : (int64_t)C);
    const double* tv = vals + t0;
    const uint16_t* tr = rank + t0;
    int i = threadIdx.x;
    for (; i + 3 * stride < cnt; i += 4 * stride) {
      double v[4];
      int r[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = tv[i + u * stride];
#pragma unroll
      for (int u = 0; u < 4; ++u) r[u] = tr[i + u * stride];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (r[u] < cnt) tile_vals[r[u]] = v[u];
    }
    for (; i < cnt; i += stride) {
      int r = tr[i];
      if (r < cnt) tile_vals[r] = tv[i];
    }
    __syncthreads();
    const int32_t* td = dst + t0;
    i = threadIdx.x;
    for (; i + 3 * stride < cnt; i += 4 * stride) {
      int64_t d[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) d[u] = td[i + u * stride];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if ((uint64_t)d[u] < (uint64_t)n) out[d[u]] = tile_vals[i + u * stride];
    }
    for (; i < cnt; i += stride) {
      int64_t d = td[i];
      if ((uint64_t)d < (uint64_t)n) out[d] = tile_vals[i];
    }
    __syncthreads();
  }
}

// Dense replay aggregate: one LDS f64 add per row into a table indexed
// by gid - base, base = first id of the partition holding the chunk's
// first row.  Ids of one partition are contiguous and partitions are in
// id order, so a chunk's ids start at base; a row whose id falls past
// the table (chunk spanning more partitions than the table covers) adds
// straight to out_sum.  Correct for ANY chunk/partition geometry.
// LDS per block is SLOTS*8 B: 2048 -> 16KB, 4096 -> 32KB, 8192 -> 64KB.
template <int SLOTS>
__global__ __launch_bounds__(BLOCK) void gb_dense_aggregate_kernel(
    const int32_t* __restrict__ gid, const double* __restrict__ part_vals,
    int64_t n, const int64_t* __restrict__ offsets,
    const int64_t* __restrict__ group_base, int num_parts, int64_t n_groups,
    double* __restrict__ out_sum, int64_t chunk) {
  __shared__ double lsum[SLOTS];
  __shared__ int sbase;
  for (int64_t start = (int64_t)blockIdx.x * chunk; start < n;
       start += (int64_t)gridDim.x * chunk) {
    int64_t end = start + chunk;
    if (end > n) end = n;
    for (int i = threadIdx.x; i < SLOTS; i += blockDim.x) lsum[i] = 0.0;
    if (threadIdx.x == 0) {
      // largest p with offsets[p] <= start (skips empty partitions)
      int lo = 0, hi = num_parts;
      while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (offsets[mid] <= start) lo = mid; else hi = mid;
      }
      sbase = (int)group_base[lo];
    }
    __syncthreads();
    const int base = sbase;
    int64_t i = start + threadIdx.x;
    const int64_t stride = (int64_t)blockDim.x;
    for (; i + 3 * stride < end; i += 4 * stride) {
      int g[4];
      double v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) g[u] = gid[i + u * stride];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = part_vals[i + u * stride];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        unsigned rel = (unsigned)(g[u] - base);
        if (rel < (unsigned)SLOTS) {
          atomicAdd(&lsum[rel], v[u]);
        } else if ((uint64_t)g[u] < (uint64_t)n_groups) {
          atomicAdd(&out_sum[g[u]], v[u]);
        }
      }
    }
    for (; i < end; i += stride) {
      int g = gid[i];
      double v = part_vals[i];
      unsigned rel = (unsigned)(g - base);
      if (rel < (unsigned)SLOTS) {
        atomicAdd(&lsum[rel], v);
      } else if ((uint64_t)g < (uint64_t)n_groups) {
        atomicAdd(&out_sum[g], v);
      }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < SLOTS; s += blockDim.x) {
      double v = lsum[s];
      if (v != 0.0 && (int64_t)base + s < n_groups)
        atomicAdd(&out_sum[(int64_t)base + s], v);
    }
    __syncthreads();
  }
}

extern "C" {

int dense_assign_max() { return DENSE_ASSIGN_MAX; }

void launch_gb_dense_count(const int64_t* pkeys, const int64_t* offsets,
                           int num_parts, int64_t* distinct,
                           hipStream_t stream) {
  hipLaunchKernelGGL(gb_dense_count_kernel, dim3(num_parts), dim3(BLOCK), 0,
                     stream, pkeys, offsets, num_parts, distinct);
}

void launch_gb_dense_assign(const int64_t* pkeys, const int64_t* offsets,
                            const int64_t* group_base, int num_parts,
                            int32_t* gid, int64_t* out_keys,
                            int64_t* out_count, hipStream_t stream) {
  hipLaunchKernelGGL(gb_dense_assign_kernel, dim3(num_parts), dim3(BLOCK), 0,
                     stream, pkeys, offsets, group_base, num_parts, gid,
                     out_keys, out_count);
}

// tile must be a power of 2 in [512, 8192]: the value tile (tile*8 B of
// LDS) then stays within the 64KB a block gets without opting in
void launch_scatter_tile_prep(const int32_t* pos, int64_t n, int tile,
                              uint16_t* rank, int32_t* dst,
                              hipStream_t stream) {
  int64_t blocks = (n + tile - 1) / tile;
  if (blocks > MAX_GRID) blocks = MAX_GRID;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(scatter_tile_prep_kernel, dim3((int)blocks), dim3(BLOCK),
                     (size_t)tile * sizeof(unsigned long long), stream, pos,
                     n, tile, rank, dst);
}

void launch_scatter_tile(const double* vals, const uint16_t* rank,
                         const int32_t* dst, int64_t n, int tile,
                         double* out, hipStream_t stream) {
  int64_t blocks = (n + tile - 1) / tile;
  if (blocks > MAX_GRID) blocks = MAX_GRID;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(scatter_tile_kernel, dim3((int)blocks), dim3(BLOCK),
                     (size_t)tile * sizeof(double), stream, vals, rank, dst,
                     n, tile, out);
}

void launch_gb_dense_aggregate(const int32_t* gid, const double* part_vals,
                               int64_t n, const int64_t* offsets,
                               const int64_t* group_base, int num_parts,
                               int64_t n_groups, double* out_sum,
                               int64_t chunk, int slots,
                               hipStream_t stream) {
  // sweep on the 125M-row bench shape (ms per call, profiles/NOTES.md
  // r03): 4096 slots 0.310/0.296/0.284/0.278/0.278 at 4K/8K/16K/32K/64K
  // rows per chunk; 2048 slots the same within 2%; 8192 slots slower
  // below 64K (0.488 at 4K)
  if (chunk <= 0) chunk = BLOCK * 128;
  int64_t blocks = (n + chunk - 1) / chunk;
  if (blocks > MAX_GRID) blocks = MAX_GRID;
  if (blocks < 1) blocks = 1;
  dim3 g((int)blocks), b(BLOCK);
  switch (slots) {
    case 2048:
      hipLaunchKernelGGL((gb_dense_aggregate_kernel<2048>), g, b, 0, stream,
                         gid, part_vals, n, offsets, group_base, num_parts,
                         n_groups, out_sum, chunk);
      break;
    case 8192:
      hipLaunchKernelGGL((gb_dense_aggregate_kernel<8192>), g, b, 0, stream,
                         gid, part_vals, n, offsets, group_base, num_parts,
                         n_groups, out_sum, chunk);
      break;
    default:
      hipLaunchKernelGGL((gb_dense_aggregate_kernel<4096>), g, b, 0, stream,
                         gid, part_vals, n, offsets, group_base, num_parts,
                         n_groups, out_sum, chunk);
  }
}

}  // extern "C"
