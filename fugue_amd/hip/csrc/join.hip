// Join family: chained-bucket hash join and the open-addressed unique join.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "relational.h"

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

// ------------------------------------------------------------------ //
// fused unique inner join + residual comparison + projection          //
//                                                                     //
// One block per ROWS probe rows (COMPACT_CHUNK, or fewer for a small   //
// probe side: launch_join_unique_select), grid-stride.  Phase A is the //
// ILP-4 chain walk of join_left_unique_kernel over the block's chunk   //
// (the dependent random loads heads -> bkeys/next bound the kernel);   //
// the comparison runs on the matched rows and the surviving match      //
// index stays in LDS.  Phase B reserves one output range per block     //
// (LDS counter, ONE global atomic, as compact8_kernel).  Phase C       //
// writes the projected columns, probe-side at the probe row and        //
// build-side at the match, straight into the range: no bi/mask arrays, //
// no materialised join result, no second compaction.                   //
// ------------------------------------------------------------------ //

__device__ __forceinline__ long long jsel_operand(const JoinSelPred& p, int s,
                                                  int64_t i, int32_t m) {
  if (p.kind[s] == JSEL_IMM) return (long long)p.imm[s];
  const long long* col = reinterpret_cast<const long long*>(p.ptr[s]);
  return p.kind[s] == JSEL_BUILD ? col[m] : col[i];
}

// int64/int64 compares exactly; anything else in fp64 as cmp_col_kernel
// does (so a NaN operand fails every OP but !=, IEEE as there)
__device__ __forceinline__ bool jsel_pred(const JoinSelPred& p, int64_t i,
                                          int32_t m) {
  if (p.op < 0) return true;
  long long a = jsel_operand(p, 0, i, m);
  long long b = jsel_operand(p, 1, i, m);
  if (p.use_int) return cmp_apply<long long>(a, b, p.op);
  double x = p.is_f64[0] ? __longlong_as_double(a) : (double)a;
  double y = p.is_f64[1] ? __longlong_as_double(b) : (double)b;
  return cmp_apply<double>(x, y, p.op);
}

// ROWS probe rows per block (a multiple of 4 * BLOCK): COMPACT_CHUNK for
// large probes, fewer for small ones so that the grid fills the device
template <int ROWS>
__global__ __launch_bounds__(BLOCK) void join_unique_select_kernel(
    const int64_t* __restrict__ pkeys, int64_t np,
    const int64_t* __restrict__ bkeys, const int32_t* __restrict__ heads,
    const int32_t* __restrict__ next, int64_t tsize, JoinSelPred pred,
    JoinSelCols cols, int64_t* __restrict__ cursor) {
  static_assert(ROWS % (4 * BLOCK) == 0, "whole rounds of four rows");
  __shared__ int32_t smatch[ROWS];  // surviving match or -1
  __shared__ int lcount;
  __shared__ long long lbase;
  uint64_t tmask = (uint64_t)(tsize - 1);
  for (int64_t start = (int64_t)blockIdx.x * ROWS; start < np;
       start += (int64_t)gridDim.x * ROWS) {
    int64_t end = start + ROWS;
    if (end > np) end = np;
    if (threadIdx.x == 0) lcount = 0;
    __syncthreads();
    int local = 0;
    for (int g = 0; g < ROWS / BLOCK; g += 4) {
      int64_t idx[4], key[4];
      int32_t cur[4], match[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        idx[j] = start + (int64_t)(g + j) * BLOCK + threadIdx.x;
        match[j] = -1;
        if (idx[j] < end) {
          key[j] = pkeys[idx[j]];
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
            if (bkeys[c] == key[j]) {
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
        if (match[j] >= 0 && !jsel_pred(pred, idx[j], match[j])) match[j] = -1;
        smatch[(g + j) * BLOCK + threadIdx.x] = match[j];
        if (match[j] >= 0) ++local;
      }
    }
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
    // a thread reads back only the slots it wrote
    for (int r = 0; r < ROWS / BLOCK; ++r) {
      int32_t m = smatch[r * BLOCK + threadIdx.x];
      if (m < 0) continue;
      int64_t i = start + (int64_t)r * BLOCK + threadIdx.x;
      int64_t pos = (int64_t)lbase + atomicAdd(&lcount, 1);
#pragma unroll
      for (int c = 0; c < COMPACT_MAX_COLS; ++c) {
        if (c < cols.ncols) {
          const uint64_t* src = reinterpret_cast<const uint64_t*>(cols.src[c]);
          reinterpret_cast<uint64_t*>(cols.dst[c])[pos] =
              cols.side[c] == JSEL_BUILD ? src[m] : src[i];
        }
      }
    }
    __syncthreads();
  }
}

namespace {
// CUs of the current device, asked once per device
int device_cus() {
  static int cus[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cus[dev] == 0) {
    int c = 0;
    if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount,
                              dev) != hipSuccess ||
        c < 1)
      c = 256;
    cus[dev] = c;
  }
  return cus[dev];
}
}  // namespace

extern "C" {

// block_rows: probe rows per block, 1024, 2048 or COMPACT_CHUNK; 0 picks
// the largest that still gives every CU four blocks (a block is one wave
// per SIMD, and the chain walk is bound by latency), else the smallest
void launch_join_unique_select(const int64_t* pkeys, int64_t np,
                               const int64_t* bkeys, const int32_t* heads,
                               const int32_t* next, int64_t tsize,
                               const JoinSelPred* pred,
                               const JoinSelCols* cols, int64_t* cursor,
                               int block_rows, hipStream_t stream) {
  if (block_rows <= 0) {
    const int64_t want = (int64_t)4 * device_cus();
    block_rows = COMPACT_CHUNK;
    while (block_rows > 1024 && np / block_rows < want) block_rows /= 2;
  }
#define JSEL_RUN(ROWS)                                                     \
  hipLaunchKernelGGL(join_unique_select_kernel<ROWS>,                      \
                     dim3(chunk_grid(np, ROWS)), dim3(BLOCK), 0, stream,   \
                     pkeys, np, bkeys, heads, next, tsize, *pred, *cols,   \
                     cursor)
  if (block_rows >= COMPACT_CHUNK) {
    JSEL_RUN(COMPACT_CHUNK);
  } else if (block_rows >= 2048) {
    JSEL_RUN(2048);
  } else {
    JSEL_RUN(1024);
  }
#undef JSEL_RUN
}

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
  hipLaunchKernelGGL(join_emit_chunked_kernel,
                     dim3(chunk_grid(np, JOIN_CHUNK)), dim3(BLOCK), 0, stream,
                     pkeys, np, bkeys, ph2, bh2, heads, next, tsize, cursor,
                     out_p, out_b, mode);
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
          // empty first: a probe key equal to the sentinel must not
          // "match" an empty slot (its idx half is uninitialized); a
          // build-side sentinel has already set flags[1]
          if (k == JOA_EMPTY) {
            act[j] = false;
          } else if (k == key[j]) {
            match[j] = table[2 * h[j] + 1];
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
