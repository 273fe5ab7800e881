// CDNA4 (gfx950 / MI355X) relational kernels for the fugue_amd HIP engine:
// what every kernel family shares on the device side.  One .hip file per
// family (hash_partition, groupby, groupby_replay, join, select,
// segmented); relational.h is the boundary to bindings.cpp.
//
// Design notes:
//  * wave64: blocks are multiples of 64 threads (256 used throughout).
//  * memory-bound kernels use grid-stride loops capped at ~8192 blocks
//    (256 CUs x 8 blocks/CU x headroom).
//  * hash tables are open-addressing in HBM with linear probing;
//    the group-by kernel additionally has an LDS-resident pre-aggregation
//    variant (per-workgroup table in shared memory, flushed once) for
//    low-cardinality keys — the LDS-hash-table requirement of the north
//    star ("LDS-resident hash tables").
//  * all cross-workgroup updates use device-scope atomics (per-XCD L2s
//    are not coherent; atomicAdd on global memory is device-scope by
//    default).
//
// These kernels replace the reference framework's delegation of
// repartition/groupby/join to Spark/Dask/DuckDB.
#pragma once

// every .hip file also names <hip/hip_runtime.h> itself: torch's hipify
// pass rewrites a device source that does not into a *_hip.hip copy
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>

#include "relational.h"

#define WAVE 64
#define MAX_GRID 8192

// blocks for n items at `chunk` items per block, clamped to [1, MAX_GRID]
// (the kernels loop over chunks with a grid stride)
static inline int chunk_grid(int64_t n, int64_t chunk) {
  int64_t blocks = (n + chunk - 1) / chunk;
  if (blocks > MAX_GRID) blocks = MAX_GRID;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

static inline int grid_for(int64_t n, int per_thread = 1) {
  return chunk_grid(n, (int64_t)BLOCK * per_thread);
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

// key compare-and-swap of the LDS hash tables (int64 and narrow int32)
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

// one comparison in domain CT; op codes 0 == 1 != 2 < 3 <= 4 > 5 >= (the
// single-comparison filters of select.hip and join_unique_select)
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
