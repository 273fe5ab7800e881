// Row-selection family: fused gather, the expression interpreter, mask
// compaction, single-comparison filters and top-k.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "relational.h"

// ---------------------------------------------------------------------
// fused multi-column row gather: one pass reads idx once per row and
// materializes up to GATHER_MAX_COLS columns of one element width
// (replaces per-column at::index_select launches on the join/sort
// output-materialization path)

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
void launch_expr_filter(const ExprProg* prog, int64_t n, bool* out,
                        hipStream_t stream) {
  hipLaunchKernelGGL(expr_filter_kernel, dim3(grid_for(n, 2)), dim3(BLOCK),
                     0, stream, *prog, n, out);
}

void launch_expr_value(const ExprProg* prog, int64_t n, int out_int,
                       void* out_v, bool* out_valid, hipStream_t stream) {
  if (out_int)
    hipLaunchKernelGGL(expr_value_kernel<true>, dim3(grid_for(n, 2)),
                       dim3(BLOCK), 0, stream, *prog, n, out_v, out_valid);
  else
    hipLaunchKernelGGL(expr_value_kernel<false>, dim3(grid_for(n, 2)),
                       dim3(BLOCK), 0, stream, *prog, n, out_v, out_valid);
}
}  // extern "C"

// ------------------------------------------------------------------ //
// fused stream compaction: write the masked rows of up to 8 eight-byte
// columns in one pass.  Each block reserves a contiguous output range
// for its chunk (one global atomic), so writes coalesce; output order is
// block-nondeterministic (frames are unordered collections).
// ------------------------------------------------------------------ //
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
  const uint64_t* z = nullptr;
  hipLaunchKernelGGL(
      compact8_kernel, dim3(chunk_grid(n, COMPACT_CHUNK)), dim3(BLOCK), 0,
      stream, mask, n, cursor, ncols > 0 ? srcs[0] : z, ncols > 1 ? srcs[1] : z,
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
// fast single-comparison filters                                      //
//                                                                     //
// The general expr_filter interpreter keeps its value stack in        //
// scratch memory (dynamically indexed), which costs ~10x SOL on a     //
// simple `col < imm` predicate (profiles r02c).  Single comparisons   //
// — the dominant WHERE shape — get dedicated one-pass kernels.        //
// ------------------------------------------------------------------ //

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

// NaN test that folds to false for the integer instantiations
__device__ __forceinline__ bool tk_nan(int64_t) { return false; }
__device__ __forceinline__ bool tk_nan(double v) { return v != v; }

template <typename T, bool LARGEST>
__device__ __forceinline__ bool tk_before(T a, int64_t ia, T b, int64_t ib) {
  // strict total order with index tiebreak (deterministic); NaN ranks
  // after every number in both directions, NaNs tie with each other
  bool na = tk_nan(a), nb = tk_nan(b);
  if (na || nb) return na != nb ? nb : ia < ib;
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
