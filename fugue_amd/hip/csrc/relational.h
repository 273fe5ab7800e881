// Host/device boundary of the CDNA4 relational kernels: the launcher
// prototypes, the limits both sides size buffers by, and the structs
// passed across.  Included by bindings.cpp (plain host C++) and by every
// .hip file that defines a launcher, so a prototype that drifts from
// its definition is a compile error on one side or the other.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#define BLOCK 256  // threads per block, every kernel

// empty-slot key of the group-by hash tables.  Kernel contract: no key
// handed to a group-by kernel equals GB_EMPTY (a probe would take the
// first empty slot for a match without claiming it, and the table
// compaction drops the slot).  ops.groupby_aggregate aggregates such
// rows apart with the keyless reduction and appends the group.
#define GB_EMPTY 0x8000000000000000LL
// most SUM/COUNT aggregates of the LDS pre-aggregating group-by kernels
// (gb_aggregate_lds_kernel, gb_aggregate_part_kernel): laggs is
// [GB_LDS_MAX_AGGS x LDS_SLOTS]
#define GB_LDS_MAX_AGGS 4
// partitioned group-by: most hash partitions (LDS histogram size)
#define PART_MAX 4096
// dense replay: most distinct keys per partition the id table accepts
#define DENSE_ASSIGN_MAX 2048
// binned dense replay: most bins (LDS histogram of the bin count kernel)
#define BIN_MAX 4096
// compact binned replay: most bins (two table rows of the tile sit in LDS
// behind the 64KB value tile)
#define SCATTER_COMPACT_MAX_BINS 512

// group-by key preparation: most key columns per pack / key-stats launch
#define PACK_MAX_COLS 8
// gb_compact: most aggregate columns, table slots per block
#define GBC_MAX_AGGS 6
#define GBC_CHUNK (BLOCK * 32)

// fused gather: most columns of one element width per launch
#define GATHER_MAX_COLS 16

// chunked compaction (compact8, join_unique_select): rows per block and
// reservation, most 8-byte columns per launch
#define COMPACT_CHUNK (BLOCK * 16)
#define COMPACT_MAX_COLS 8

// join_unique_select: residual comparison `lhs OP rhs` and projection,
// passed to the kernel by value.  An operand or output column is read on
// the probe side at the probe row, on the build side at the matched row.
enum { JSEL_PROBE = 0, JSEL_BUILD = 1, JSEL_IMM = 2 };
struct JoinSelPred {
  int op;       // -1: no predicate; else 0 == 1 != 2 < 3 <= 4 > 5 >=
  int use_int;  // both operands int64: exact compare; else in fp64
  int kind[2];  // JSEL_PROBE / JSEL_BUILD / JSEL_IMM
  int is_f64[2];               // operand holds fp64 bits (else int64)
  unsigned long long ptr[2];   // column base (kinds PROBE, BUILD)
  unsigned long long imm[2];   // immediate bits (kind IMM)
};
struct JoinSelCols {
  int ncols;
  int side[COMPACT_MAX_COLS];  // JSEL_PROBE / JSEL_BUILD
  unsigned long long src[COMPACT_MAX_COLS];
  unsigned long long dst[COMPACT_MAX_COLS];
};

// expression interpreter program limits
#define EXPR_MAX_OPS 48
#define EXPR_MAX_COLS 12
#define EXPR_STACK 12

// postfix program + column table, passed to the kernel by value
struct ExprProg {
  int n_ops;
  unsigned char op[EXPR_MAX_OPS];
  signed char aux[EXPR_MAX_OPS];
  unsigned long long imm[EXPR_MAX_COLS];
  unsigned long long col_data[EXPR_MAX_COLS];
  unsigned long long col_valid[EXPR_MAX_COLS];  // 0 = none
  unsigned char col_dt[EXPR_MAX_COLS];
};

// segmented rank: sorted positions per block, most order columns
#define SEG_CHUNK (BLOCK * 32)
#define SEG_MAX_COLS 4
// seg_total work buffer in int64 words: 8 per chunk (chunk aggregates and
// carries of both passes), then the forward (acc, cnt) of every position
#define SEG_TOTAL_WORK(n) \
  (8 * (((int64_t)(n) + SEG_CHUNK - 1) / SEG_CHUNK) + 2 * (int64_t)(n))

// seg_frame: sorted positions per block, and the largest frame reach
// (positions before plus positions after the current row) it takes.  A
// block stages SEG_FRAME_TILE + SEG_FRAME_MAX_REACH positions of 17 bytes
// (key, value, validity) in LDS: 34 KiB, under the 64 KiB static limit.
#define SEG_FRAME_TILE 1024
#define SEG_FRAME_MAX_REACH 1024

// top-k select: largest k, most stage-1 blocks (candidate rows = blocks * k)
#define TOPK_MAX 16
#define TOPK_BLOCKS 512

extern "C" {

// ---- hash_partition.hip ----
void launch_hash_col_i64(const int64_t* data, const bool* valid, uint64_t* out,
                         int64_t n, int is_first, hipStream_t stream);
void launch_hash_col_i32(const int32_t* data, const bool* valid, uint64_t* out,
                         int64_t n, int is_first, hipStream_t stream);
void launch_hash_col_f64(const double* data, const bool* valid, uint64_t* out,
                         int64_t n, int is_first, hipStream_t stream);
void launch_hash_col_f32(const float* data, const bool* valid, uint64_t* out,
                         int64_t n, int is_first, hipStream_t stream);
void launch_hash_col_i8(const int8_t* data, const bool* valid, uint64_t* out,
                        int64_t n, int is_first, hipStream_t stream);
void launch_bucket_of(const uint64_t* hashes, int32_t* buckets, int64_t n,
                      int32_t num_buckets, hipStream_t stream);
void launch_histogram(const int32_t* buckets, int64_t* hist, int64_t n,
                      int32_t num_buckets, hipStream_t stream);
void launch_scatter(const int32_t* buckets, int64_t* cursor, int64_t* perm,
                    int64_t n, hipStream_t stream);
void launch_hash_string_col(const int64_t* offsets, const uint8_t* bytes,
                            const bool* valid, uint64_t* out, int64_t n,
                            int is_first, hipStream_t stream);
void launch_hash_seed(uint64_t* out, int64_t n, uint64_t seed,
                      hipStream_t stream);

// ---- groupby.hip ----
void launch_reduce_cols(const double* vals, const bool* valids,
                        const int32_t* ops, int n_aggs, int64_t n,
                        double* out, int64_t* out_count, hipStream_t stream);
void launch_gb_aggregate(const int64_t* keys, const double* vals,
                         const bool* valids, const int32_t* ops, int n_aggs,
                         int64_t n, int64_t* tkeys, double* gaggs,
                         int64_t* gcount, int64_t tsize, int use_lds,
                         hipStream_t stream);
void launch_gb_part_hist(const int64_t* keys, int64_t n, int shift,
                         int64_t* hist, int num_parts, hipStream_t stream);
void launch_gb_part_scatter(const int64_t* keys, const double* vals,
                            int n_aggs, int64_t n, int shift, int64_t* cursor,
                            int64_t* out_keys, double* out_vals,
                            int num_parts, int32_t* out_pos, int64_t chunk,
                            hipStream_t stream);
void launch_gb_aggregate_part(const int64_t* part_keys,
                              const double* part_vals, const int32_t* ops,
                              int n_aggs, int64_t n, const int64_t* offsets,
                              int64_t num_parts, int64_t* tkeys,
                              double* gaggs, int64_t* gcount, int64_t tsize,
                              hipStream_t stream);
void launch_gb_part_scatter_staged(const int64_t* keys, const double* vals,
                                   int64_t n, int shift, int64_t* cursor,
                                   void* out_keys, double* out_vals,
                                   int64_t chunk, int narrow, int* ovf,
                                   int num_parts, hipStream_t stream);
void launch_gb_aggregate_part_big(const void* part_keys,
                                  const double* part_vals,
                                  const int32_t* ops, int64_t n,
                                  int64_t* tkeys, double* gaggs,
                                  int64_t* gcount, int64_t tsize,
                                  int64_t chunk, int narrow, int slots,
                                  hipStream_t stream);
void launch_gb_mark_reps(const int64_t* h1, const int64_t* h2,
                         const int64_t* tkeys, int64_t tsize, int64_t* rep,
                         int64_t* th2, int64_t* conflict, int64_t n,
                         hipStream_t stream);
void launch_gb_key_stats(const void** data, const bool** valid,
                         const int* dwidth, int ncols, int64_t n,
                         int64_t nsamples, int64_t* slots, int32_t* counts,
                         int tsize, int do_minmax, uint64_t* out,
                         hipStream_t stream);
void launch_pack_cols(const void** data, const bool** valid,
                      const int* dwidth, const int64_t* mins,
                      const int* shifts, int ncols, int64_t n, int64_t* out,
                      hipStream_t stream);
void launch_unpack_col(const int64_t* packed, int64_t n, int shift,
                       int64_t mask, int64_t lo, int dwidth, int has_nulls,
                       void* out, bool* valid, hipStream_t stream);

// ---- groupby_replay.hip ----
void launch_scatter_by_pos(const double* vals, const int32_t* pos, int64_t n,
                           double* out_vals, hipStream_t stream);
void launch_gb_dense_count(const int64_t* pkeys, const int64_t* offsets,
                           int num_parts, int64_t* distinct,
                           hipStream_t stream);
void launch_gb_dense_assign(const int64_t* pkeys, const int64_t* offsets,
                            const int64_t* group_base, int num_parts,
                            int32_t* gid, int64_t* out_keys,
                            int64_t* out_count, hipStream_t stream);
void launch_scatter_tile_prep(const int32_t* pos, int64_t n, int tile,
                              uint16_t* rank, int32_t* dst,
                              hipStream_t stream);
void launch_scatter_tile(const double* vals, const uint16_t* rank,
                         const int32_t* dst, int64_t n, int tile, double* out,
                         hipStream_t stream);
void launch_gb_dense_aggregate(const int32_t* gid, const double* part_vals,
                               int64_t n, const int64_t* offsets,
                               const int64_t* group_base, int num_parts,
                               int64_t n_groups, double* out_sum,
                               int64_t chunk, int slots, hipStream_t stream);
void launch_scatter_bin_count(const int32_t* pos, int64_t n, int tile,
                              const int64_t* bin_offsets, int nbins,
                              int32_t* counts, hipStream_t stream);
void launch_scatter_tile_prep_binned(const int32_t* pos, int64_t n, int tile,
                                     const int64_t* bin_offsets, int nbins,
                                     const int64_t* run_delta,
                                     const int32_t* gid_old, uint16_t* rank,
                                     int32_t* dst, int32_t* gid_new,
                                     hipStream_t stream);
void launch_gb_dense_aggregate_binned(
    const int32_t* gid, const double* part_vals, int64_t n,
    const int64_t* bin_offsets, const int64_t* bin_group_base,
    const int64_t* bin_chunk_base, int nbins, int64_t total_chunks,
    int64_t n_groups, double* out_sum, int64_t chunk, int slots,
    hipStream_t stream);
void launch_scatter_tile_prep_compact(
    const int32_t* pos, int64_t n, int tile, const int64_t* bin_offsets,
    const int64_t* bin_group_base, int nbins, const int32_t* tile_delta,
    const int32_t* gid_old, uint16_t* rank, uint16_t* rel, int32_t* gid_new,
    hipStream_t stream);
int launch_scatter_tile_compact(const double* vals, const uint16_t* rank,
                                const uint16_t* tile_start,
                                const int32_t* tile_delta, int nbins,
                                int64_t n, int tile, double* out, int threads,
                                hipStream_t stream);
void launch_gb_dense_aggregate_compact(
    const uint16_t* rel, const double* part_vals, int64_t n,
    const int64_t* bin_offsets, const int64_t* bin_group_base,
    const int64_t* bin_chunk_base, int nbins, int64_t total_chunks,
    int64_t n_groups, double* out_sum, int64_t chunk, int slots,
    hipStream_t stream);

// ---- join.hip ----
void launch_join_build(const int64_t* keys, int64_t n, int32_t* heads,
                       int32_t* next, int64_t tsize, int32_t* dup,
                       hipStream_t stream);
void launch_join_emit_unique(const int64_t* pkeys, int64_t np,
                             const int64_t* bkeys, const int64_t* ph2,
                             const int64_t* bh2, const int32_t* heads,
                             const int32_t* next, int64_t tsize, int mode,
                             int64_t* out_pi, int64_t* out_bi,
                             int64_t* cursor, bool* out_mask, int mask_neg,
                             hipStream_t stream);
void launch_join_count(const int64_t* pkeys, int64_t np, const int64_t* bkeys,
                       const int64_t* ph2, const int64_t* bh2,
                       const int32_t* heads, const int32_t* next,
                       int64_t tsize, int32_t* counts, hipStream_t stream);
void launch_join_total(const int64_t* pkeys, int64_t np,
                       const int64_t* bkeys, const int64_t* ph2,
                       const int64_t* bh2, const int32_t* heads,
                       const int32_t* next, int64_t tsize, int mode,
                       int64_t* total, hipStream_t stream);
void launch_join_emit_chunked(const int64_t* pkeys, int64_t np,
                              const int64_t* bkeys, const int64_t* ph2,
                              const int64_t* bh2, const int32_t* heads,
                              const int32_t* next, int64_t tsize,
                              int64_t* cursor, int64_t* out_p,
                              int64_t* out_b, int mode, hipStream_t stream);
void launch_join_emit(const int64_t* pkeys, int64_t np, const int64_t* bkeys,
                      const int64_t* ph2, const int64_t* bh2,
                      const int32_t* heads, const int32_t* next, int64_t tsize,
                      const int64_t* offsets, int64_t* out_p, int64_t* out_b,
                      int mode, hipStream_t stream);
void launch_join_mark_build(const int64_t* pkeys, int64_t np,
                            const int64_t* bkeys, const int64_t* ph2,
                            const int64_t* bh2, const int32_t* heads,
                            const int32_t* next, int64_t tsize, bool* bmatched,
                            hipStream_t stream);
// inner join against UNIQUE build keys + residual comparison + projection
// in one pass.  Contract: heads/next come from launch_join_build over
// bkeys (tsize a power of two, every chain ends at -1); np >= 1; every
// dst holds np elements (capacity mode); *cursor is 0 on entry and holds
// the number of rows written on exit; rows land in no defined order.  Any
// int64 key value is admitted.  A build key that occurs twice makes the
// walk stop at the first match in chain order: the caller must not use
// the result then.  block_rows: probe rows per block, 1024, 2048 or
// COMPACT_CHUNK; 0 lets the launcher pick by np and the device's CUs.
void launch_join_unique_select(const int64_t* pkeys, int64_t np,
                               const int64_t* bkeys, const int32_t* heads,
                               const int32_t* next, int64_t tsize,
                               const JoinSelPred* pred,
                               const JoinSelCols* cols, int64_t* cursor,
                               int block_rows, hipStream_t stream);
void launch_joinoa_build(const int64_t* bkeys, int64_t nb, int64_t* table,
                         int64_t tsize, int64_t* flags, hipStream_t stream);
void launch_joinoa_probe(const int64_t* pkeys, int64_t np,
                         const int64_t* table, int64_t tsize,
                         int64_t* out_pi, int64_t* out_bi, bool* out_mask,
                         int mask_neg, hipStream_t stream);

// ---- select.hip ----
void launch_gather_cols(const uint64_t* src_ptrs, const uint64_t* dst_ptrs,
                        int ncols, int elem_size, const int64_t* idx,
                        int64_t n, hipStream_t stream);
void launch_expr_filter(const ExprProg* prog, int64_t n, bool* out,
                        hipStream_t stream);
void launch_expr_value(const ExprProg* prog, int64_t n, int out_int,
                       void* out_v, bool* out_valid, hipStream_t stream);
void launch_compact8(const bool* mask, int64_t n, int64_t* cursor,
                     const uint64_t** srcs, uint64_t** dsts, int ncols,
                     hipStream_t stream);
void launch_cmp_imm(const void* a, const bool* valid, int dtype,
                    int64_t imm_i, double imm_d, int use_int, int op,
                    int64_t n, bool* out, hipStream_t stream);
void launch_cmp_col(const void* a, const bool* va, const void* b,
                    const bool* vb, int dtype, int op, int64_t n, bool* out,
                    hipStream_t stream);
void launch_eq2_mask(const int64_t* h1, const int64_t* h2, const int64_t* l1,
                     const int64_t* l2, const bool* valid, int neg,
                     int64_t n, bool* out, hipStream_t stream);
void launch_topk(const void* vals, int dtype, int largest, int64_t n, int k,
                 void* cand_v, int64_t* cand_i, void* out_v, int64_t* out_i,
                 hipStream_t stream);

// ---- segmented.hip ----
void launch_gb_compact(const int64_t* tkeys, const int64_t* gcount,
                       const double** agg_src, double** agg_dst, int n_aggs,
                       int64_t tsize, int64_t* bcounts, int64_t* bases,
                       int64_t* out_keys, int64_t* out_count,
                       const int64_t* extra_src, int64_t* extra_dst,
                       hipStream_t stream);
void launch_seg_rank(const int64_t* perm, const int64_t* pkeys,
                     const int64_t* const* col_data,
                     const uint8_t* const* col_valid, const int* col_is_float,
                     int ncols, int64_t n, int kind, int64_t* work,
                     int64_t* out, hipStream_t stream);
void launch_seg_take(const int64_t* perm, const int64_t* pkeys, int64_t n,
                     int64_t n_take, int64_t* work, int64_t* bcounts,
                     int64_t* bases, int64_t* out, hipStream_t stream);
void launch_seg_shift(const int64_t* perm, const int64_t* pkeys,
                      const int64_t* vals, const uint8_t* valid, int64_t n,
                      int64_t d, int64_t* out, uint8_t* out_valid,
                      hipStream_t stream);
void launch_seg_scan(const int64_t* perm, const int64_t* pkeys,
                     const int64_t* vals, const uint8_t* valid, int64_t n,
                     int op, int is_float, int64_t* work, int64_t* out_acc,
                     int64_t* out_cnt, hipStream_t stream);
// op 0..2 as launch_seg_scan, 3 FIRST, 4 LAST; work: SEG_TOTAL_WORK(n)
void launch_seg_total(const int64_t* perm, const int64_t* pkeys,
                      const int64_t* vals, const uint8_t* valid, int64_t n,
                      int op, int is_float, int64_t* work, int64_t* out_acc,
                      int64_t* out_cnt, hipStream_t stream);
// op as launch_seg_total over the frame [i + lo, i + hi] of every sorted
// position i, clipped to its partition; lo and hi are clamped to [-n, n]
// and the reach max(0, -lo) + max(0, hi) must not exceed
// SEG_FRAME_MAX_REACH (nothing is launched otherwise)
void launch_seg_frame(const int64_t* perm, const int64_t* pkeys,
                      const int64_t* vals, const uint8_t* valid, int64_t n,
                      int64_t lo, int64_t hi, int op, int is_float,
                      int64_t* out_acc, int64_t* out_cnt, hipStream_t stream);

}  // extern "C"
