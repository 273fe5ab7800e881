// Block-scan family: order-preserving pipelines built on per-block counts
// and the single-block scan gbc_scan_kernel, which both share: the
// group-table compaction and the segmented rank / take.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "relational.h"

// ------------------------------------------------------------------ //
// deterministic group-table compaction                                //
//                                                                     //
// Replaces occupied = (tkeys != EMPTY).nonzero() + per-column          //
// index_select with a 3-kernel own pipeline (count / scan / emit) that //
// preserves slot order (deterministic output) and moves each byte      //
// once.  total lands in bases[nblocks] for a single host read.         //
// ------------------------------------------------------------------ //

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
  const double* src[GBC_MAX_AGGS];
  double* dst[GBC_MAX_AGGS];
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

#define SEG_ITERS (SEG_CHUNK / BLOCK)
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

// ------------------------------------------------------------------ //
// value windows over the same sorted permutation                       //
//                                                                      //
// seg_shift: LAG/LEAD, a segment-bounded shift of one 8-byte column.   //
// seg_scan: running SUM/MIN/MAX and COUNT of the non-null values from  //
// the partition's first sorted position to the current one.  vals and  //
// valid are in original row order and gathered through perm; results   //
// land in original row order (out[perm[i]]).  The scan chains its      //
// chunks like the rank: summary -> single-block scan -> apply.         //
// ------------------------------------------------------------------ //

// Precondition: perm sorts by partition key first, so equal keys are
// contiguous and "the row d positions back has my key" means "it is in
// my partition".  d > 0 looks back (LAG), d < 0 ahead (LEAD); the
// launcher clamps d to [-n, n].  Moves bits only.
__global__ __launch_bounds__(BLOCK) void seg_shift_kernel(
    const int64_t* __restrict__ perm, const int64_t* __restrict__ pkeys,
    const int64_t* __restrict__ vals, const uint8_t* __restrict__ valid,
    int64_t n, int64_t d, int64_t* __restrict__ out,
    uint8_t* __restrict__ out_valid) {
  int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  int64_t j = seg_row(perm, i, n);
  int64_t s = i - d;
  int64_t v = 0;
  uint8_t ok = 0;
  if (s >= 0 && s < n) {
    int64_t js = seg_row(perm, s, n);
    if (pkeys[js] == pkeys[j]) {
      v = vals[js];
      ok = valid != nullptr ? (uint8_t)(valid[js] != 0) : (uint8_t)1;
    }
  }
  out[j] = v;
  out_valid[j] = ok;
}

#define SEG_OP_SUM 0
#define SEG_OP_MIN 1
#define SEG_OP_MAX 2
// seg_total and seg_frame only: the first / last non-null value in sorted
// order
#define SEG_OP_FIRST 3
#define SEG_OP_LAST 4

// sign bit of a count in seg_total's scratch: the position starts a
// partition
#define SEG_HEAD_BIT ((int64_t)0x8000000000000000LL)

// Scan element of a range of sorted positions: head says the range holds
// a partition start, and then acc/cnt cover the positions from the LAST
// start on; otherwise they cover the whole range.  cnt is the number of
// non-null values folded into acc; cnt == 0 is the identity (acc is 0
// then), so MIN and MAX need no sentinel value.
struct SegVal {
  int head;
  int64_t acc;  // int64, or the bits of a double
  int64_t cnt;
};

__device__ __forceinline__ SegVal seg_val_identity() {
  SegVal r;
  r.head = 0;
  r.acc = 0;
  r.cnt = 0;
  return r;
}

// op of two non-empty sides.  Integer SUM adds unsigned: overflow wraps.
// NaN never arrives here (the caller passes it as null).
__device__ __forceinline__ int64_t seg_val_op(int64_t a, int64_t b, int op,
                                              int is_float) {
  if (op == SEG_OP_FIRST) return a;
  if (op == SEG_OP_LAST) return b;
  if (is_float) {
    double x = __longlong_as_double(a), y = __longlong_as_double(b);
    double r = op == SEG_OP_SUM ? x + y
                                : (op == SEG_OP_MIN ? (y < x ? y : x)
                                                    : (y > x ? y : x));
    return __double_as_longlong(r);
  }
  if (op == SEG_OP_SUM) return (int64_t)((uint64_t)a + (uint64_t)b);
  if (op == SEG_OP_MIN) return b < a ? b : a;
  return b > a ? b : a;
}

__device__ __forceinline__ SegVal seg_val_combine(SegVal a, SegVal b, int op,
                                                  int is_float) {
  if (b.head) return b;
  SegVal r;
  r.head = a.head;
  r.cnt = a.cnt + b.cnt;
  r.acc = a.cnt == 0 ? b.acc
                     : (b.cnt == 0 ? a.acc
                                   : seg_val_op(a.acc, b.acc, op, is_float));
  return r;
}

// Inclusive segmented scan of x over this iteration's 256 positions,
// continued from carry (everything before them), which is advanced past
// them.  Each wave scans its 64 lanes with shuffles; wave totals meet in
// ws (double-buffered by the caller: one barrier per call).  The combine
// tree depends on the position alone, so a rerun repeats every bit.
// Block-uniform call.
__device__ __forceinline__ SegVal seg_val_block_step(SegVal x, int lane,
                                                     int wave, int op,
                                                     int is_float,
                                                     SegVal& carry,
                                                     SegVal* ws) {
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    SegVal t;
    t.head = __shfl_up(x.head, off);
    t.acc = __shfl_up(x.acc, off);
    t.cnt = __shfl_up(x.cnt, off);
    if (lane >= off) x = seg_val_combine(t, x, op, is_float);
  }
  if (lane == WAVE - 1) ws[wave] = x;
  __syncthreads();
  SegVal in = carry;
  SegVal tot = carry;
#pragma unroll
  for (int w = 0; w < SEG_WAVES; ++w) {
    SegVal s = ws[w];
    if (w < wave) in = seg_val_combine(in, s, op, is_float);
    tot = seg_val_combine(tot, s, op, is_float);
  }
  carry = tot;
  return seg_val_combine(in, x, op, is_float);
}

// scan element of sorted position i (identity past the end); j is its
// row.  Must be called by every lane of the wave.
__device__ __forceinline__ SegVal seg_val_load(
    const int64_t* __restrict__ perm, const int64_t* __restrict__ pkeys,
    const SegCols& none, const int64_t* __restrict__ vals,
    const uint8_t* __restrict__ valid, int64_t i, int64_t n, int lane,
    int64_t& j) {
  bool h, p;
  seg_flags(perm, pkeys, none, 0, i, n, lane, j, h, p);
  SegVal x = seg_val_identity();
  if (i < n) {
    bool ok = valid == nullptr || valid[j] != 0;
    x.head = h ? 1 : 0;
    x.cnt = ok ? 1 : 0;
    x.acc = ok ? vals[j] : 0;
  }
  return x;
}

// per-chunk aggregate, folded in the same order as the apply kernel
__global__ __launch_bounds__(BLOCK) void seg_scan_summary_kernel(
    const int64_t* __restrict__ perm, const int64_t* __restrict__ pkeys,
    const int64_t* __restrict__ vals, const uint8_t* __restrict__ valid,
    int64_t n, int op, int is_float, int64_t* __restrict__ sum_head,
    int64_t* __restrict__ sum_acc, int64_t* __restrict__ sum_cnt) {
  __shared__ SegVal ws[2][SEG_WAVES];
  int64_t start = (int64_t)blockIdx.x * SEG_CHUNK;
  int lane = threadIdx.x % WAVE;
  int wave = threadIdx.x / WAVE;
  SegCols none;
  memset(&none, 0, sizeof(none));
  SegVal carry = seg_val_identity();  // same value in every thread
  for (int it = 0; it < SEG_ITERS; ++it) {
    int64_t i0 = start + (int64_t)it * BLOCK;
    if (i0 >= n) break;  // block-uniform
    int64_t j;
    SegVal x = seg_val_load(perm, pkeys, none, vals, valid,
                            i0 + threadIdx.x, n, lane, j);
    seg_val_block_step(x, lane, wave, op, is_float, carry, ws[it & 1]);
  }
  if (threadIdx.x == 0) {
    sum_head[blockIdx.x] = carry.head;
    sum_acc[blockIdx.x] = carry.acc;
    sum_cnt[blockIdx.x] = carry.cnt;
  }
}

// single-block exclusive segmented scan of the chunk aggregates: chunk b
// receives the aggregate of chunks [0, b)
__global__ __launch_bounds__(BLOCK) void seg_scan_scan_kernel(
    const int64_t* __restrict__ sum_head, const int64_t* __restrict__ sum_acc,
    const int64_t* __restrict__ sum_cnt, int nblocks, int op, int is_float,
    int64_t* __restrict__ car_head, int64_t* __restrict__ car_acc,
    int64_t* __restrict__ car_cnt) {
  __shared__ SegVal tile[BLOCK];
  SegVal carry = seg_val_identity();  // same value in every thread
  for (int t0 = 0; t0 < nblocks; t0 += BLOCK) {
    int i = t0 + (int)threadIdx.x;
    SegVal v = seg_val_identity();
    if (i < nblocks) {
      v.head = (int)sum_head[i];
      v.acc = sum_acc[i];
      v.cnt = sum_cnt[i];
    }
    tile[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < BLOCK; off <<= 1) {
      SegVal self = tile[threadIdx.x];
      bool has = (int)threadIdx.x >= off;
      SegVal left = self;
      if (has) left = tile[threadIdx.x - off];
      __syncthreads();
      if (has) tile[threadIdx.x] = seg_val_combine(left, self, op, is_float);
      __syncthreads();
    }
    if (i < nblocks) {
      SegVal e = carry;
      if (threadIdx.x > 0)
        e = seg_val_combine(carry, tile[threadIdx.x - 1], op, is_float);
      car_head[i] = e.head;
      car_acc[i] = e.acc;
      car_cnt[i] = e.cnt;
    }
    carry = seg_val_combine(carry, tile[BLOCK - 1], op, is_float);
    __syncthreads();
  }
}

// The apply step of the scan.  SORTED = false writes acc and cnt of every
// row, null rows included (they carry the running value through; acc is
// 0 while cnt is 0), to out[perm[i]].  SORTED = true is the forward pass
// of seg_total: the same values land coalesced at out[i], and the sign
// bit of out_cnt[i] marks a partition start (cnt is never negative).
template <bool SORTED>
__device__ __forceinline__ void seg_scan_apply(
    const int64_t* __restrict__ perm, const int64_t* __restrict__ pkeys,
    const int64_t* __restrict__ vals, const uint8_t* __restrict__ valid,
    int64_t n, int op, int is_float, const int64_t* __restrict__ car_head,
    const int64_t* __restrict__ car_acc, const int64_t* __restrict__ car_cnt,
    int64_t* __restrict__ out_acc, int64_t* __restrict__ out_cnt,
    SegVal (*ws)[SEG_WAVES]) {
  int64_t start = (int64_t)blockIdx.x * SEG_CHUNK;
  int lane = threadIdx.x % WAVE;
  int wave = threadIdx.x / WAVE;
  SegCols none;
  memset(&none, 0, sizeof(none));
  SegVal carry;
  carry.head = (int)car_head[blockIdx.x];
  carry.acc = car_acc[blockIdx.x];
  carry.cnt = car_cnt[blockIdx.x];
  for (int it = 0; it < SEG_ITERS; ++it) {
    int64_t i0 = start + (int64_t)it * BLOCK;
    if (i0 >= n) break;  // block-uniform
    int64_t i = i0 + threadIdx.x;
    int64_t j;
    SegVal x = seg_val_load(perm, pkeys, none, vals, valid, i, n, lane, j);
    SegVal r =
        seg_val_block_step(x, lane, wave, op, is_float, carry, ws[it & 1]);
    if (i < n) {
      if (SORTED) {
        out_acc[i] = r.acc;
        out_cnt[i] = x.head ? (r.cnt | SEG_HEAD_BIT) : r.cnt;
      } else {
        out_acc[j] = r.acc;
        out_cnt[j] = r.cnt;
      }
    }
  }
}

__global__ __launch_bounds__(BLOCK) void seg_scan_apply_kernel(
    const int64_t* __restrict__ perm, const int64_t* __restrict__ pkeys,
    const int64_t* __restrict__ vals, const uint8_t* __restrict__ valid,
    int64_t n, int op, int is_float, const int64_t* __restrict__ car_head,
    const int64_t* __restrict__ car_acc, const int64_t* __restrict__ car_cnt,
    int64_t* __restrict__ out_acc, int64_t* __restrict__ out_cnt) {
  __shared__ SegVal ws[2][SEG_WAVES];
  seg_scan_apply<false>(perm, pkeys, vals, valid, n, op, is_float, car_head,
                        car_acc, car_cnt, out_acc, out_cnt, ws);
}

// ------------------------------------------------------------------ //
// seg_total: whole-partition SUM/MIN/MAX/FIRST/LAST and COUNT           //
//                                                                      //
// Every row receives the aggregate of all non-null values of its       //
// partition.  The forward pass is the running scan above, kept in      //
// sorted-position order in scratch: its value at a partition's last    //
// position IS the total, with the bits seg_scan gives there.  The      //
// backward pass resolves, for every position, the last position of its //
// partition (the nearest one at or after it whose successor starts a   //
// partition), chunks chained by summary -> single-block scan -> apply  //
// like everything here, and copies that position's (acc, cnt) to       //
// out[perm[i]].  A copy, so all rows of a partition agree bit for bit; //
// -1 marks "no partition end seen yet", which leaves cnt == 0 free to  //
// be a payload.  The head bits in scratch spare the backward pass the  //
// key gather.                                                          //
// ------------------------------------------------------------------ //

__global__ __launch_bounds__(BLOCK) void seg_total_forward_kernel(
    const int64_t* __restrict__ perm, const int64_t* __restrict__ pkeys,
    const int64_t* __restrict__ vals, const uint8_t* __restrict__ valid,
    int64_t n, int op, int is_float, const int64_t* __restrict__ car_head,
    const int64_t* __restrict__ car_acc, const int64_t* __restrict__ car_cnt,
    int64_t* __restrict__ fwd_acc, int64_t* __restrict__ fwd_cnt) {
  __shared__ SegVal ws[2][SEG_WAVES];
  seg_scan_apply<true>(perm, pkeys, vals, valid, n, op, is_float, car_head,
                       car_acc, car_cnt, fwd_acc, fwd_cnt, ws);
}

// is sorted position i (< n) the last of its partition?
__device__ __forceinline__ bool seg_is_tail(const int64_t* __restrict__ fwd_cnt,
                                            int64_t i, int64_t n) {
  return i + 1 >= n || fwd_cnt[i + 1] < 0;
}

// first partition end of each chunk, -1 if it has none
__global__ __launch_bounds__(BLOCK) void seg_total_summary_kernel(
    const int64_t* __restrict__ fwd_cnt, int64_t n,
    int64_t* __restrict__ sum_tail) {
  __shared__ int s_tail;
  int64_t start = (int64_t)blockIdx.x * SEG_CHUNK;
  if (threadIdx.x == 0) s_tail = SEG_CHUNK;
  __syncthreads();
  int ltail = SEG_CHUNK;
  for (int it = SEG_ITERS - 1; it >= 0; --it) {
    int rel = it * BLOCK + (int)threadIdx.x;
    int64_t i = start + rel;
    if (i < n && seg_is_tail(fwd_cnt, i, n)) ltail = rel;
  }
  if (ltail < SEG_CHUNK) atomicMin(&s_tail, ltail);
  __syncthreads();
  if (threadIdx.x == 0)
    sum_tail[blockIdx.x] = s_tail < SEG_CHUNK ? start + s_tail : -1;
}

// single-block exclusive scan from the right: chunk b receives the first
// partition end of chunks (b, nblocks), -1 if there is none
__global__ __launch_bounds__(BLOCK) void seg_total_scan_kernel(
    const int64_t* __restrict__ sum_tail, int nblocks,
    int64_t* __restrict__ car_tail) {
  __shared__ int64_t tile[BLOCK];
  int64_t carry = -1;  // same value in every thread
  int ntiles = (nblocks + BLOCK - 1) / BLOCK;
  for (int t = ntiles - 1; t >= 0; --t) {
    int i = t * BLOCK + (int)threadIdx.x;
    tile[threadIdx.x] = i < nblocks ? sum_tail[i] : -1;
    __syncthreads();
    for (int off = 1; off < BLOCK; off <<= 1) {
      int64_t self = tile[threadIdx.x];
      int64_t right = -1;
      if ((int)threadIdx.x + off < BLOCK) right = tile[threadIdx.x + off];
      __syncthreads();
      if (self < 0) tile[threadIdx.x] = right;
      __syncthreads();
    }
    if (i < nblocks) {
      int64_t e = threadIdx.x + 1 < BLOCK ? tile[threadIdx.x + 1] : -1;
      car_tail[i] = e >= 0 ? e : carry;
    }
    if (tile[0] >= 0) carry = tile[0];
    __syncthreads();
  }
}

__global__ __launch_bounds__(BLOCK) void seg_total_apply_kernel(
    const int64_t* __restrict__ perm, int64_t n,
    const int64_t* __restrict__ car_tail, const int64_t* __restrict__ fwd_acc,
    const int64_t* __restrict__ fwd_cnt, int64_t* __restrict__ out_acc,
    int64_t* __restrict__ out_cnt) {
  __shared__ int64_t ws[2][SEG_WAVES];
  int64_t start = (int64_t)blockIdx.x * SEG_CHUNK;
  int lane = threadIdx.x % WAVE;
  int wave = threadIdx.x / WAVE;
  int64_t carry = car_tail[blockIdx.x];  // same value in every thread
  for (int it = SEG_ITERS - 1; it >= 0; --it) {
    int64_t i0 = start + (int64_t)it * BLOCK;
    if (i0 >= n) continue;  // block-uniform
    int64_t i = i0 + threadIdx.x;
    int64_t w0 = i0 + (int64_t)wave * WAVE;
    uint64_t tmask = __ballot(i < n && seg_is_tail(fwd_cnt, i, n));
    if (lane == 0)
      ws[it & 1][wave] = tmask != 0 ? w0 + __ffsll((long long)tmask) - 1 : -1;
    __syncthreads();
    // nearest end in a later wave of these 256 positions, else the carry
    int64_t in = carry;
    int64_t tot = carry;
#pragma unroll
    for (int w = SEG_WAVES - 1; w >= 0; --w) {
      int64_t s = ws[it & 1][w];
      if (s >= 0) {
        if (w > wave) in = s;
        tot = s;
      }
    }
    carry = tot;
    uint64_t m = tmask & (~0ULL << lane);  // lanes >= this one
    int64_t t = m != 0 ? w0 + __ffsll((long long)m) - 1 : in;
    if (i < n) {
      int64_t j = seg_row(perm, i, n);
      // position n - 1 always ends a partition, so t is in [i, n); the
      // test keeps a corrupted scratch from reading out of bounds
      bool ok = (uint64_t)t < (uint64_t)n;
      out_acc[j] = ok ? fwd_acc[t] : 0;
      out_cnt[j] = ok ? (fwd_cnt[t] & ~SEG_HEAD_BIT) : 0;
    }
  }
}

// ------------------------------------------------------------------ //
// seg_frame: SUM/MIN/MAX/FIRST/LAST and COUNT over a moving ROWS frame  //
//                                                                      //
// Sorted position i of a partition folds the non-null values at sorted //
// positions [i + lo, i + hi] that lie in its partition.  One block      //
// handles a tile of SEG_FRAME_TILE positions: it gathers key, value     //
// bits and validity of the tile and of a halo of max(0, -lo) positions //
// before and max(0, hi) after it (clipped to [0, n)) into LDS, reading  //
// perm coalesced, so the random gather through perm happens once per    //
// staged position and not once per frame element.  Each lane then walks //
// its positions' frames in ascending order from LDS; an element counts  //
// when its key equals the row's (the precondition of seg_shift: equal   //
// keys are contiguous) and it is valid.  Consecutive lanes read         //
// consecutive words.  A sum starts from 0 and only ever adds, left to   //
// right, fresh for every row: its bits depend on the frame alone.       //
// ------------------------------------------------------------------ //

#define SEG_FRAME_STAGE (SEG_FRAME_TILE + SEG_FRAME_MAX_REACH)

__global__ __launch_bounds__(BLOCK) void seg_frame_kernel(
    const int64_t* __restrict__ perm, const int64_t* __restrict__ pkeys,
    const int64_t* __restrict__ vals, const uint8_t* __restrict__ valid,
    int64_t n, int lo, int hi, int op, int is_float,
    int64_t* __restrict__ out_acc, int64_t* __restrict__ out_cnt) {
  __shared__ int64_t s_key[SEG_FRAME_STAGE];
  __shared__ int64_t s_val[SEG_FRAME_STAGE];
  __shared__ uint8_t s_ok[SEG_FRAME_STAGE];
  int64_t t0 = (int64_t)blockIdx.x * SEG_FRAME_TILE;
  int64_t t1 = t0 + SEG_FRAME_TILE < n ? t0 + SEG_FRAME_TILE : n;
  int64_t g0 = t0 - (lo < 0 ? -lo : 0);
  int64_t g1 = t1 + (hi > 0 ? hi : 0);
  if (g0 < 0) g0 = 0;
  if (g1 > n) g1 = n;
  // the launcher bounds the reach; a wider frame must not overrun LDS
  if (g1 - g0 > SEG_FRAME_STAGE) return;  // block-uniform
  int staged = (int)(g1 - g0);
  for (int r = threadIdx.x; r < staged; r += BLOCK) {
    int64_t j = seg_row(perm, g0 + r, n);
    s_key[r] = pkeys[j];
    s_val[r] = vals[j];
    s_ok[r] = valid != nullptr ? (uint8_t)(valid[j] != 0) : (uint8_t)1;
  }
  __syncthreads();
  for (int64_t i = t0 + threadIdx.x; i < t1; i += BLOCK) {
    // frame clipped to the staged range [g0, g1): a holds a >= g0 and
    // b < g1, so every r below is in [0, staged)
    int64_t a = i + lo < g0 ? g0 : i + lo;
    int64_t b = i + hi > g1 - 1 ? g1 - 1 : i + hi;
    int64_t k = s_key[i - g0];
    int64_t acc = 0, cnt = 0;
    for (int64_t g = a; g <= b; ++g) {
      int r = (int)(g - g0);
      if (s_key[r] == k && s_ok[r]) {
        int64_t v = s_val[r];
        // 0 is the start of a sum (+0.0 as a double); the others take
        // their first value as it is: no sentinels
        acc = (cnt == 0 && op != SEG_OP_SUM) ? v
                                             : seg_val_op(acc, v, op, is_float);
        ++cnt;
      }
    }
    int64_t j = seg_row(perm, i, n);
    out_acc[j] = acc;
    out_cnt[j] = cnt;
  }
}

extern "C" {

void launch_seg_frame(const int64_t* perm, const int64_t* pkeys,
                      const int64_t* vals, const uint8_t* valid, int64_t n,
                      int64_t lo, int64_t hi, int op, int is_float,
                      int64_t* out_acc, int64_t* out_cnt,
                      hipStream_t stream) {
  if (n <= 0) return;
  // beyond ±n nothing is in a frame; clamping keeps i + lo from overflowing
  lo = lo > n ? n : (lo < -n ? -n : lo);
  hi = hi > n ? n : (hi < -n ? -n : hi);
  if (lo > hi) {  // every frame is empty: any such pair writes the zeros
    lo = 1;
    hi = 0;
  }
  int64_t reach = (lo < 0 ? -lo : 0) + (hi > 0 ? hi : 0);
  if (reach > SEG_FRAME_MAX_REACH) return;  // the binding refuses these
  int64_t nblocks = (n + SEG_FRAME_TILE - 1) / SEG_FRAME_TILE;
  hipLaunchKernelGGL(seg_frame_kernel, dim3((unsigned)nblocks), dim3(BLOCK), 0,
                     stream, perm, pkeys, vals, valid, n, (int)lo, (int)hi, op,
                     is_float, out_acc, out_cnt);
}

void launch_seg_shift(const int64_t* perm, const int64_t* pkeys,
                      const int64_t* vals, const uint8_t* valid, int64_t n,
                      int64_t d, int64_t* out, uint8_t* out_valid,
                      hipStream_t stream) {
  if (n <= 0) return;
  // |d| >= n never finds a source; clamping keeps i - d from overflowing
  d = d > n ? n : (d < -n ? -n : d);
  int64_t nblocks = (n + BLOCK - 1) / BLOCK;
  hipLaunchKernelGGL(seg_shift_kernel, dim3((unsigned)nblocks), dim3(BLOCK), 0,
                     stream, perm, pkeys, vals, valid, n, d, out, out_valid);
}

// work: 6 * nblocks int64 (chunk aggregates, then chunk carries)
void launch_seg_scan(const int64_t* perm, const int64_t* pkeys,
                     const int64_t* vals, const uint8_t* valid, int64_t n,
                     int op, int is_float, int64_t* work, int64_t* out_acc,
                     int64_t* out_cnt, hipStream_t stream) {
  if (n <= 0) return;
  int nblocks = (int)((n + SEG_CHUNK - 1) / SEG_CHUNK);
  int64_t* w = work;
  hipLaunchKernelGGL(seg_scan_summary_kernel, dim3(nblocks), dim3(BLOCK), 0,
                     stream, perm, pkeys, vals, valid, n, op, is_float, w,
                     w + nblocks, w + 2 * (int64_t)nblocks);
  hipLaunchKernelGGL(seg_scan_scan_kernel, dim3(1), dim3(BLOCK), 0, stream, w,
                     w + nblocks, w + 2 * (int64_t)nblocks, nblocks, op,
                     is_float, w + 3 * (int64_t)nblocks,
                     w + 4 * (int64_t)nblocks, w + 5 * (int64_t)nblocks);
  hipLaunchKernelGGL(seg_scan_apply_kernel, dim3(nblocks), dim3(BLOCK), 0,
                     stream, perm, pkeys, vals, valid, n, op, is_float,
                     w + 3 * (int64_t)nblocks, w + 4 * (int64_t)nblocks,
                     w + 5 * (int64_t)nblocks, out_acc, out_cnt);
}

// work: SEG_TOTAL_WORK(n) int64: the scan's 6 * nblocks, the backward
// pass's 2 * nblocks, then the forward values (acc, cnt) of n positions
void launch_seg_total(const int64_t* perm, const int64_t* pkeys,
                      const int64_t* vals, const uint8_t* valid, int64_t n,
                      int op, int is_float, int64_t* work, int64_t* out_acc,
                      int64_t* out_cnt, hipStream_t stream) {
  if (n <= 0) return;
  int nblocks = (int)((n + SEG_CHUNK - 1) / SEG_CHUNK);
  int64_t nb = nblocks;
  int64_t* w = work;
  int64_t* sum_tail = w + 6 * nb;
  int64_t* car_tail = w + 7 * nb;
  int64_t* fwd_acc = w + 8 * nb;
  int64_t* fwd_cnt = fwd_acc + n;
  hipLaunchKernelGGL(seg_scan_summary_kernel, dim3(nblocks), dim3(BLOCK), 0,
                     stream, perm, pkeys, vals, valid, n, op, is_float, w,
                     w + nb, w + 2 * nb);
  hipLaunchKernelGGL(seg_scan_scan_kernel, dim3(1), dim3(BLOCK), 0, stream, w,
                     w + nb, w + 2 * nb, nblocks, op, is_float, w + 3 * nb,
                     w + 4 * nb, w + 5 * nb);
  hipLaunchKernelGGL(seg_total_forward_kernel, dim3(nblocks), dim3(BLOCK), 0,
                     stream, perm, pkeys, vals, valid, n, op, is_float,
                     w + 3 * nb, w + 4 * nb, w + 5 * nb, fwd_acc, fwd_cnt);
  hipLaunchKernelGGL(seg_total_summary_kernel, dim3(nblocks), dim3(BLOCK), 0,
                     stream, fwd_cnt, n, sum_tail);
  hipLaunchKernelGGL(seg_total_scan_kernel, dim3(1), dim3(BLOCK), 0, stream,
                     sum_tail, nblocks, car_tail);
  hipLaunchKernelGGL(seg_total_apply_kernel, dim3(nblocks), dim3(BLOCK), 0,
                     stream, perm, n, car_tail, fwd_acc, fwd_cnt, out_acc,
                     out_cnt);
}

}  // extern "C"

extern "C" {

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
