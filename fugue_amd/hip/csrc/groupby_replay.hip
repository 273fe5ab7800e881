// Group-by replay family: re-aggregation over a recorded shuffle layout.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "relational.h"

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
//    table fills, compaction or host readback.  The values are laid   //
//    out by bins of M consecutive partitions (M chosen on the host so //
//    a bin's ids fit the LDS table), which makes the scatter's runs M //
//    times longer (scatter_tile_prep_binned_kernel,                   //
//    gb_dense_aggregate_binned_kernel); M = 1 is the partition layout.//
//    The compact form of the binned layout drops the per-row           //
//    destination for a [tiles, bins] table and keeps 16-bit ids        //
//    relative to the bin (scatter_tile_prep_compact_kernel,            //
//    scatter_tile_compact_kernel with a register-pipelined tile loop,  //
//    gb_dense_aggregate_compact_kernel): 28 instead of 34 B/row moved. //
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

// Binned value layout.  The replay does not need the recorded layout's
// hash partitions, only that the ids of a stretch of rows fit the
// aggregate's LDS table.  M consecutive partitions form a bin (one
// contiguous id range); rows are re-placed bin-major, and inside a bin in
// tile order, so a (tile, bin) run is M times longer than a (tile,
// partition) run.  bin_offsets is [B+1]: the first recorded position of
// every bin, i.e. offsets[::M].

// largest b in [0, nb) with bounds[b] <= x, for ascending bounds[0] <= x
__device__ __forceinline__ int bin_of(const int64_t* __restrict__ bounds,
                                      int nb, int64_t x) {
  int lo = 0, hi = nb;
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (bounds[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// counts[tile][b] = rows of the tile whose recorded position is in bin b
__global__ __launch_bounds__(BLOCK) void scatter_bin_count_kernel(
    const int32_t* __restrict__ pos, int64_t n, int C,
    const int64_t* __restrict__ bin_offsets, int nbins,
    int32_t* __restrict__ counts) {
  __shared__ int lhist[BIN_MAX];
  int64_t ntiles = (n + C - 1) / C;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    for (int b = threadIdx.x; b < nbins; b += blockDim.x) lhist[b] = 0;
    __syncthreads();
    int64_t t0 = tile * C;
    int cnt = (int)((n - t0) < (int64_t)C ? (n - t0) : (int64_t)C);
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
      int64_t p = (int64_t)(uint32_t)pos[t0 + i];
      if (p < n) atomicAdd(&lhist[bin_of(bin_offsets, nbins, p)], 1);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nbins; b += blockDim.x)
      counts[tile * nbins + b] = lhist[b];
    __syncthreads();
  }
}

// scatter_tile_prep_kernel for the binned layout.  The sort by recorded
// position already groups a tile's rows by bin, so the tile's r-th ranked
// row goes to run_delta[tile][b] + r, where run_delta[tile][b] =
// bin_offsets[b] + (rows of bin b in earlier tiles) - (first rank of bin
// b in this tile), prepared by the caller from the count matrix.  The
// row's dense id moves with it: gid_new[new] = gid_old[old].  The sort
// buffer is all of the LDS, so bin_offsets is searched in global memory.
__global__ __launch_bounds__(BLOCK) void scatter_tile_prep_binned_kernel(
    const int32_t* __restrict__ pos, int64_t n, int C,
    const int64_t* __restrict__ bin_offsets, int nbins,
    const int64_t* __restrict__ run_delta,
    const int32_t* __restrict__ gid_old, uint16_t* __restrict__ rank,
    int32_t* __restrict__ dst, int32_t* __restrict__ gid_new) {
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
      int64_t p = (int64_t)(e >> 16);
      rank[t0 + (int)(e & 0xffffULL)] = (uint16_t)r;
      // a position outside [0, n) (not a permutation) gets a destination
      // the scatter's own bound check drops
      int64_t d = -1;
      if (p < n) {
        d = run_delta[tile * nbins + bin_of(bin_offsets, nbins, p)] + r;
        if ((uint64_t)d < (uint64_t)n) gid_new[d] = gid_old[p]; else d = -1;
      }
      dst[t0 + r] = (int32_t)d;
    }
    __syncthreads();
  }
}

// Compact form of the binned layout.  The destination of a tile's r-th
// ranked row is a [tiles, bins] table plus r, and an id is a 16-bit offset
// from its bin's first id, so neither the [n] dst nor the 32-bit gid is
// materialised: the kernel writes rank (as scatter_tile_prep_binned_kernel
// does) and rel[d] = gid_old[p] - bin_group_base[bin] at the destination
// d = tile_delta[tile][bin] + r the binned kernel would have stored.  The
// caller has checked that no bin is wider than 65536 ids.  gid_new, when
// not null, also gets the 32-bit id in the new order.
__global__ __launch_bounds__(BLOCK) void scatter_tile_prep_compact_kernel(
    const int32_t* __restrict__ pos, int64_t n, int C,
    const int64_t* __restrict__ bin_offsets,
    const int64_t* __restrict__ bin_group_base, int nbins,
    const int32_t* __restrict__ tile_delta,
    const int32_t* __restrict__ gid_old, uint16_t* __restrict__ rank,
    uint16_t* __restrict__ rel, int32_t* __restrict__ gid_new) {
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
      int64_t p = (int64_t)(e >> 16);
      rank[t0 + (int)(e & 0xffffULL)] = (uint16_t)r;
      if (p < n) {
        int b = bin_of(bin_offsets, nbins, p);
        int64_t d = (int64_t)tile_delta[tile * nbins + b] + r;
        if ((uint64_t)d < (uint64_t)n) {
          int32_t g = gid_old[p];
          rel[d] = (uint16_t)((int64_t)g - bin_group_base[b]);
          if (gid_new != nullptr) gid_new[d] = g;  // for the 32-bit aggregate
        }
      }
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

// scatter_tile_kernel over the compact binned layout.  tile_start is
// [tiles, bins + 1] (first tile-local rank of every bin, then the tile's
// placed rows), tile_delta [tiles, bins]; both rows of the tile sit in LDS
// behind the value tile (768 B at 128 bins).  A wave stores a contiguous
// span of ranks, 64 at a time: each lane searches its first rank's bin
// once and then only walks forward, because its ranks ascend.  Ranks at or
// past the tile's placed rows (positions that were no permutation) are
// dropped, and the parent's bound check on the destination stays.
//
// The loop over tiles is software-pipelined: the next tile's values and
// ranks are loaded into registers before the current tile is stored, so
// the loads are in flight during the store phase.  NT threads hold
// 8192 / NT rows each.
template <int NT>
__global__ __launch_bounds__(NT, NT / 128) void scatter_tile_compact_kernel(
    const double* __restrict__ vals, const uint16_t* __restrict__ rank,
    const uint16_t* __restrict__ tile_start,
    const int32_t* __restrict__ tile_delta, int nbins, int64_t n, int C,
    double* __restrict__ out) {
  constexpr int R = 8192 / NT;  // value rows per thread
  // table entries per thread: SCATTER_COMPACT_MAX_BINS + 1 over NT threads
  constexpr int TB = (SCATTER_COMPACT_MAX_BINS + NT) / NT;
  extern __shared__ double tile_vals[];
  int32_t* td = (int32_t*)(tile_vals + C);
  uint16_t* ts = (uint16_t*)(td + nbins);
  const int64_t ntiles = (n + C - 1) / C;
  const int tid = threadIdx.x;
  // rows per thread at this tile size, and this lane's first rank
  const int rc = C >= NT ? C / NT : 1;
  const int i0 = (tid >> 6) * (rc << 6) + (tid & 63);
  double v[R];
  unsigned r[R], ps[TB];
  int pd[TB];
  // Loads of one tile into registers, nothing else: every load is
  // unconditional off a scalar base (an index past the end is clamped and
  // the row dropped when the registers are consumed), so no instruction
  // after the loads has to wait for them.
  auto load_tile = [&](int64_t t) {
    const int64_t t0 = t * C;
    const int cnt = (int)((n - t0) < (int64_t)C ? (n - t0) : (int64_t)C);
    const double* tv = vals + t0;
    const uint16_t* tr = rank + t0;
#pragma unroll
    for (int u = 0; u < R; ++u) {
      int i = tid + u * NT;
      unsigned ii = (unsigned)(i < cnt ? i : cnt - 1);
      v[u] = tv[ii];
      r[u] = tr[ii];
    }
    const int32_t* gd = tile_delta + t * nbins;
    const uint16_t* gs = tile_start + t * (nbins + 1);
#pragma unroll
    for (int k = 0; k < TB; ++k) {
      int b = tid + k * NT;
      pd[k] = gd[(unsigned)(b < nbins ? b : nbins - 1)];
      ps[k] = gs[(unsigned)(b < nbins ? b : nbins)];
    }
  };
  int64_t tile = blockIdx.x;
  if (tile < ntiles) load_tile(tile);
  for (; tile < ntiles; tile += gridDim.x) {
    const int64_t t0 = tile * C;
    const int cnt = (int)((n - t0) < (int64_t)C ? (n - t0) : (int64_t)C);
#pragma unroll
    for (int u = 0; u < R; ++u)
      if (tid + u * NT < cnt && r[u] < (unsigned)cnt) tile_vals[r[u]] = v[u];
#pragma unroll
    for (int k = 0; k < TB; ++k) {
      int b = tid + k * NT;
      if (b < nbins) td[b] = pd[k];
      if (b <= nbins) ts[b] = (uint16_t)ps[k];
    }
    __syncthreads();
    const int64_t next = tile + gridDim.x;
    if (next < ntiles) load_tile(next);  // in flight during the stores
    int lim = (int)ts[nbins];
    if (lim > cnt) lim = cnt;
    if (i0 < lim) {
      int b = 0, hi = nbins;  // largest b with ts[b] <= i0 (ts[0] == 0)
      while (hi - b > 1) {
        int mid = (b + hi) >> 1;
        if ((int)ts[mid] <= i0) b = mid; else hi = mid;
      }
      // not unrolled: the registers belong to the next tile's rows
#pragma unroll 1
      for (int i = i0, e = i0 + (rc << 6); i < e && i < lim; i += 64) {
        while (b + 1 < nbins && (int)ts[b + 1] <= i) ++b;
        int64_t d = (int64_t)td[b] + i;
        if ((uint64_t)d < (uint64_t)n) out[d] = tile_vals[i];
      }
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

// Dense replay aggregate over the binned layout: block work is a chunk of
// one bin, never a chunk of the whole row range, so the table base is the
// bin's first id and a bin no wider than the table adds nothing to global
// memory before the flush.  Virtual chunk v belongs to the bin b with
// bin_chunk_base[b] <= v < bin_chunk_base[b + 1] ([B+1], the prefix of
// ceil(rows_b / chunk)); empty bins own no chunk.  The out-of-table guard
// of gb_dense_aggregate_kernel stays, so any geometry is exact.  Every
// thread searches bin_chunk_base itself (block-uniform, B+1 entries):
// with 8192 slots lsum is the whole 64KB and there is no room for a
// shared base.
template <int SLOTS>
__global__ __launch_bounds__(BLOCK) void gb_dense_aggregate_binned_kernel(
    const int32_t* __restrict__ gid, const double* __restrict__ part_vals,
    int64_t n, const int64_t* __restrict__ bin_offsets,
    const int64_t* __restrict__ bin_group_base,
    const int64_t* __restrict__ bin_chunk_base, int nbins,
    int64_t total_chunks, int64_t n_groups, double* __restrict__ out_sum,
    int64_t chunk) {
  __shared__ double lsum[SLOTS];
  for (int64_t vc = blockIdx.x; vc < total_chunks; vc += gridDim.x) {
    for (int i = threadIdx.x; i < SLOTS; i += blockDim.x) lsum[i] = 0.0;
    const int b = bin_of(bin_chunk_base, nbins, vc);
    int64_t start = bin_offsets[b] + (vc - bin_chunk_base[b]) * chunk;
    int64_t end = start + chunk;
    const int64_t bin_end = bin_offsets[b + 1];
    if (end > bin_end) end = bin_end;
    // rows read stay inside [0, n) whatever the bin arrays hold
    if (start < 0) start = 0;
    if (end > n) end = n;
    const int base = (int)bin_group_base[b];
    __syncthreads();
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

// gb_dense_aggregate_binned_kernel over 16-bit ids: rel[j] is the id of
// row j less its bin's first id, so the table index needs no subtraction
// and a row costs 10 bytes instead of 12.  A rel past the table (a bin
// wider than SLOTS) adds straight to out_sum[base + rel], as there.  rel
// and part_vals are 16-byte aligned at row 0 (whole allocations).
//
// A block owns a contiguous range of virtual chunks, total_chunks split
// evenly over the grid (sizes differ by at most one), and walks it bin by
// bin: the chunks of one bin in the range are ONE row interval, so the
// table is carried across them and flushed (and zeroed again) only where
// the bin changes and at the end of the range.  The row loop over an
// interval is software-pipelined with two register sets of one four-row
// group per lane: the next set's loads are issued before the current
// set's LDS adds.  Loads are unconditional off clamped indices; a group
// past the interval is dropped when it is consumed.  No block waits on
// another; every loop is bounded by the arguments.
template <int SLOTS>
__global__ __launch_bounds__(BLOCK) void gb_dense_aggregate_compact_kernel(
    const uint16_t* __restrict__ rel, const double* __restrict__ part_vals,
    int64_t n, const int64_t* __restrict__ bin_offsets,
    const int64_t* __restrict__ bin_group_base,
    const int64_t* __restrict__ bin_chunk_base, int nbins,
    int64_t total_chunks, int64_t n_groups, double* __restrict__ out_sum,
    int64_t chunk) {
  __shared__ double lsum[SLOTS];
  const int tid = threadIdx.x;
  const int64_t q = total_chunks / gridDim.x, rem = total_chunks % gridDim.x;
  const int64_t bx = blockIdx.x;
  int64_t vc = bx * q + (bx < rem ? bx : rem);
  const int64_t vc1 = vc + q + (bx < rem ? 1 : 0);
  if (vc >= vc1) return;
  for (int i = tid; i < SLOTS; i += BLOCK) lsum[i] = 0.0;
  __syncthreads();
  while (vc < vc1) {
    const int b = bin_of(bin_chunk_base, nbins, vc);
    const int64_t cb = bin_chunk_base[b];
    int64_t ve = bin_chunk_base[b + 1];
    if (ve > vc1) ve = vc1;
    if (ve <= vc) ve = vc + 1;  // progress whatever the bin arrays hold
    const int64_t base = bin_group_base[b];
    int64_t start = bin_offsets[b] + (vc - cb) * chunk;
    int64_t end = bin_offsets[b] + (ve - cb) * chunk;
    const int64_t bin_end = bin_offsets[b + 1];
    if (end > bin_end) end = bin_end;
    // rows read stay inside [0, n) whatever the bin arrays hold
    if (start < 0) start = 0;
    if (end > n) end = n;
    if (start > end) start = end;
    auto add = [&](unsigned g, double v) {
      if (g < (unsigned)SLOTS) {
        atomicAdd(&lsum[g], v);
      } else if ((uint64_t)(base + g) < (uint64_t)n_groups) {
        atomicAdd(&out_sum[base + g], v);
      }
    };
    // A lane takes four consecutive rows: their ids are one 8-byte load
    // (2-byte loads per lane were slower than the 32-bit ids they replace)
    // and their values two 16-byte loads.  Rows before the first multiple
    // of four and after the last go one per lane.
    int64_t a0 = (start + 3) & ~(int64_t)3;
    if (a0 > end) a0 = end;
    const int64_t ng = (end - a0) >> 2;  // four-row groups
    const int64_t a1 = a0 + (ng << 2);
    if (tid < 4) {
      int64_t h = start + tid;
      if (h < a0) add(rel[h], part_vals[h]);
      int64_t t = a1 + tid;
      if (t < end) add(rel[t], part_vals[t]);
    }
    if (ng > 0) {
      const uint16_t* rp = rel + a0;
      const double* vp = part_vals + a0;
      uint2 ga, gb;
      double2 va0, va1, vb0, vb1;
      // group j of the interval, clamped to the last one
      auto load = [&](uint2& g, double2& v0, double2& v1, int64_t j) {
        if (j >= ng) j = ng - 1;
        g = *(const uint2*)(rp + 4 * j);
        v0 = *(const double2*)(vp + 4 * j);
        v1 = *(const double2*)(vp + 4 * j + 2);
      };
      auto consume = [&](uint2 g, double2 v0, double2 v1, int64_t j) {
        if (j < ng) {
          add(g.x & 0xffffu, v0.x);
          add(g.x >> 16, v0.y);
          add(g.y & 0xffffu, v1.x);
          add(g.y >> 16, v1.y);
        }
      };
      load(ga, va0, va1, tid);
      for (int64_t j = tid; j < ng; j += 2 * BLOCK) {
        load(gb, vb0, vb1, j + BLOCK);  // in flight during the adds of j
        consume(ga, va0, va1, j);
        load(ga, va0, va1, j + 2 * BLOCK);
        consume(gb, vb0, vb1, j + BLOCK);
      }
    }
    vc = ve;
    // flush and zero in one pass; the table is then ready for the next bin
    __syncthreads();
    for (int s = tid; s < SLOTS; s += BLOCK) {
      double v = lsum[s];
      if (v != 0.0) {
        if ((uint64_t)(base + s) < (uint64_t)n_groups)
          atomicAdd(&out_sum[base + s], v);
        lsum[s] = 0.0;
      }
    }
    if (vc < vc1) __syncthreads();
  }
}

extern "C" {

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
  hipLaunchKernelGGL(scatter_tile_prep_kernel, dim3(chunk_grid(n, tile)),
                     dim3(BLOCK), (size_t)tile * sizeof(unsigned long long),
                     stream, pos, n, tile, rank, dst);
}

void launch_scatter_tile(const double* vals, const uint16_t* rank,
                         const int32_t* dst, int64_t n, int tile,
                         double* out, hipStream_t stream) {
  hipLaunchKernelGGL(scatter_tile_kernel, dim3(chunk_grid(n, tile)),
                     dim3(BLOCK), (size_t)tile * sizeof(double), stream, vals,
                     rank, dst, n, tile, out);
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
  dim3 g(chunk_grid(n, chunk)), b(BLOCK);
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

// one-time preparation of the binned layout (nbins <= BIN_MAX)
void launch_scatter_bin_count(const int32_t* pos, int64_t n, int tile,
                              const int64_t* bin_offsets, int nbins,
                              int32_t* counts, hipStream_t stream) {
  hipLaunchKernelGGL(scatter_bin_count_kernel, dim3(chunk_grid(n, tile)),
                     dim3(BLOCK), 0, stream, pos, n, tile, bin_offsets, nbins,
                     counts);
}

void launch_scatter_tile_prep_binned(const int32_t* pos, int64_t n, int tile,
                                     const int64_t* bin_offsets, int nbins,
                                     const int64_t* run_delta,
                                     const int32_t* gid_old, uint16_t* rank,
                                     int32_t* dst, int32_t* gid_new,
                                     hipStream_t stream) {
  hipLaunchKernelGGL(scatter_tile_prep_binned_kernel,
                     dim3(chunk_grid(n, tile)), dim3(BLOCK),
                     (size_t)tile * sizeof(unsigned long long), stream, pos, n,
                     tile, bin_offsets, nbins, run_delta, gid_old, rank, dst,
                     gid_new);
}

// chunk > 0 is the one bin_chunk_base was built with
void launch_gb_dense_aggregate_binned(
    const int32_t* gid, const double* part_vals, int64_t n,
    const int64_t* bin_offsets, const int64_t* bin_group_base,
    const int64_t* bin_chunk_base, int nbins, int64_t total_chunks,
    int64_t n_groups, double* out_sum, int64_t chunk, int slots,
    hipStream_t stream) {
  dim3 g(chunk_grid(total_chunks, 1)), b(BLOCK);
  switch (slots) {
    case 2048:
      hipLaunchKernelGGL((gb_dense_aggregate_binned_kernel<2048>), g, b, 0,
                         stream, gid, part_vals, n, bin_offsets,
                         bin_group_base, bin_chunk_base, nbins, total_chunks,
                         n_groups, out_sum, chunk);
      break;
    case 4096:
      hipLaunchKernelGGL((gb_dense_aggregate_binned_kernel<4096>), g, b, 0,
                         stream, gid, part_vals, n, bin_offsets,
                         bin_group_base, bin_chunk_base, nbins, total_chunks,
                         n_groups, out_sum, chunk);
      break;
    default:
      hipLaunchKernelGGL((gb_dense_aggregate_binned_kernel<8192>), g, b, 0,
                         stream, gid, part_vals, n, bin_offsets,
                         bin_group_base, bin_chunk_base, nbins, total_chunks,
                         n_groups, out_sum, chunk);
  }
}

// ---- compact binned layout ----

void launch_scatter_tile_prep_compact(
    const int32_t* pos, int64_t n, int tile, const int64_t* bin_offsets,
    const int64_t* bin_group_base, int nbins, const int32_t* tile_delta,
    const int32_t* gid_old, uint16_t* rank, uint16_t* rel, int32_t* gid_new,
    hipStream_t stream) {
  hipLaunchKernelGGL(scatter_tile_prep_compact_kernel,
                     dim3(chunk_grid(n, tile)), dim3(BLOCK),
                     (size_t)tile * sizeof(unsigned long long), stream, pos, n,
                     tile, bin_offsets, bin_group_base, nbins, tile_delta,
                     gid_old, rank, rel, gid_new);
}

}  // extern "C"

namespace {
template <int NT>
hipError_t scatter_tile_compact_launch(
    const double* vals, const uint16_t* rank, const uint16_t* tile_start,
    const int32_t* tile_delta, int nbins, int64_t n, int tile, double* out,
    hipStream_t stream) {
  // value tile, then the tile's delta and start rows; past 64KB the block
  // opts in to the large LDS of CDNA4 (160KB per CU)
  size_t lds = (size_t)tile * sizeof(double) + (size_t)nbins * 4 +
               (((size_t)nbins + 1) * 2 + 7) / 8 * 8;
  if (lds > 65536) {
    // once per device and instantiation, for the most the kernel asks for
    static bool opted[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !opted[dev]) {
      e = hipFuncSetAttribute(
          reinterpret_cast<const void*>(&scatter_tile_compact_kernel<NT>),
          hipFuncAttributeMaxDynamicSharedMemorySize,
          8192 * 8 + SCATTER_COMPACT_MAX_BINS * 4 +
              (SCATTER_COMPACT_MAX_BINS + 8) * 2);
      if (e != hipSuccess) return e;
      if (dev >= 0 && dev < 64) opted[dev] = true;
    }
  }
  hipLaunchKernelGGL((scatter_tile_compact_kernel<NT>),
                     dim3(chunk_grid(n, tile)), dim3(NT), lds, stream, vals,
                     rank, tile_start, tile_delta, nbins, n, tile, out);
  return hipGetLastError();
}

// The grid is the blocks the device holds at once (CUs x blocks per CU at
// this instantiation's LDS, asked once per device), each with one
// contiguous range of the virtual chunks.
template <int SLOTS>
void dense_aggregate_compact_launch(
    const uint16_t* rel, const double* part_vals, int64_t n,
    const int64_t* bin_offsets, const int64_t* bin_group_base,
    const int64_t* bin_chunk_base, int nbins, int64_t total_chunks,
    int64_t n_groups, double* out_sum, int64_t chunk, hipStream_t stream) {
  static int resident[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  int grid = dev >= 0 && dev < 64 ? resident[dev] : 0;
  if (grid == 0) {
    int cus = 0, per_cu = 0;
    if (dev < 0 ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                              dev) != hipSuccess ||
        cus < 1)
      cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &per_cu,
            reinterpret_cast<const void*>(
                &gb_dense_aggregate_compact_kernel<SLOTS>),
            BLOCK, 0) != hipSuccess ||
        per_cu < 1)
      per_cu = 1;
    grid = cus * per_cu;
    if (grid > MAX_GRID) grid = MAX_GRID;
    if (dev >= 0 && dev < 64) resident[dev] = grid;
  }
  if (total_chunks < grid) grid = (int)total_chunks;
  hipLaunchKernelGGL((gb_dense_aggregate_compact_kernel<SLOTS>), dim3(grid),
                     dim3(BLOCK), 0, stream, rel, part_vals, n, bin_offsets,
                     bin_group_base, bin_chunk_base, nbins, total_chunks,
                     n_groups, out_sum, chunk);
}
}  // namespace

extern "C" {

// nbins <= SCATTER_COMPACT_MAX_BINS; threads is 512 or 1024 (0: the
// default).  Returns the HIP error of the launch.
int launch_scatter_tile_compact(const double* vals, const uint16_t* rank,
                                const uint16_t* tile_start,
                                const int32_t* tile_delta, int nbins,
                                int64_t n, int tile, double* out, int threads,
                                hipStream_t stream) {
  switch (threads) {
    case 512:
      return (int)scatter_tile_compact_launch<512>(
          vals, rank, tile_start, tile_delta, nbins, n, tile, out, stream);
    default:
      return (int)scatter_tile_compact_launch<1024>(
          vals, rank, tile_start, tile_delta, nbins, n, tile, out, stream);
  }
}

void launch_gb_dense_aggregate_compact(
    const uint16_t* rel, const double* part_vals, int64_t n,
    const int64_t* bin_offsets, const int64_t* bin_group_base,
    const int64_t* bin_chunk_base, int nbins, int64_t total_chunks,
    int64_t n_groups, double* out_sum, int64_t chunk, int slots,
    hipStream_t stream) {
  switch (slots) {
    case 2048:
      dense_aggregate_compact_launch<2048>(
          rel, part_vals, n, bin_offsets, bin_group_base, bin_chunk_base,
          nbins, total_chunks, n_groups, out_sum, chunk, stream);
      break;
    case 4096:
      dense_aggregate_compact_launch<4096>(
          rel, part_vals, n, bin_offsets, bin_group_base, bin_chunk_base,
          nbins, total_chunks, n_groups, out_sum, chunk, stream);
      break;
    default:
      dense_aggregate_compact_launch<8192>(
          rel, part_vals, n, bin_offsets, bin_group_base, bin_chunk_base,
          nbins, total_chunks, n_groups, out_sum, chunk, stream);
  }
}

}  // extern "C"
