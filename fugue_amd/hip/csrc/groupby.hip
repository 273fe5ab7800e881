// Group-by family: keyless column reductions, the HBM/LDS hash
// aggregation, the partitioned (simple and staged) path, representative
// rows for hashed keys, and key preparation (stats, pack, unpack).
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "relational.h"

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
  __shared__ double laggs[GB_LDS_MAX_AGGS * LDS_SLOTS];
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
  __shared__ double laggs[GB_LDS_MAX_AGGS * LDS_SLOTS];
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
  dim3 g(chunk_grid(n, chunk)), b(BLOCK);
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
  dim3 g(chunk_grid(n, chunk)), b(BLOCK);
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
  hipLaunchKernelGGL(gb_part_scatter_kernel, dim3(chunk_grid(n, chunk)),
                     dim3(BLOCK), 0, stream, keys, vals, n_aggs, n, shift,
                     cursor, out_keys, out_vals, num_parts, out_pos, chunk);
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
  if (use_lds && n_aggs <= GB_LDS_MAX_AGGS) {
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

void launch_gb_mark_reps(const int64_t* h1, const int64_t* h2,
                         const int64_t* tkeys, int64_t tsize, int64_t* rep,
                         int64_t* th2, int64_t* conflict, int64_t n,
                         hipStream_t stream) {
  hipLaunchKernelGGL(gb_mark_reps_kernel, dim3(grid_for(n)), dim3(BLOCK), 0,
                     stream, h1, h2, tkeys, tsize, rep, th2, conflict, n);
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
  const void* data[PACK_MAX_COLS];   // int64/int32/int16 per dwidth
  const bool* valid[PACK_MAX_COLS];  // may be null
  int dwidth[PACK_MAX_COLS];         // element bytes: 8, 4 or 2
  int64_t mins[PACK_MAX_COLS];       // pack phase only
  int shifts[PACK_MAX_COLS];         // pack phase only
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
