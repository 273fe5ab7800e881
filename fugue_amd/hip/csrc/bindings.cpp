// Torch-extension bindings for the CDNA4 relational kernels (the .hip
// files beside this one; launchers and shared limits in relational.h).
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "relational.h"

namespace {

hipStream_t current_stream() {
  return (hipStream_t)c10::hip::getCurrentHIPStream().stream();
}

void check_gpu(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on the GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

const bool* opt_valid_ptr(const c10::optional<at::Tensor>& v) {
  if (!v.has_value()) return nullptr;
  return v->data_ptr<bool>();
}

// ---- shared pieces of the partitioned group-by ----

// partition id = mix64(key) >> part_shift(P): the top log2(P) hash bits
int part_shift(int64_t num_parts) {
  int shift = 64;
  for (int64_t p = num_parts; p > 1; p >>= 1) --shift;
  return shift;
}

// phase-3 LDS table sized for ~0.5 load at the partition granularity:
// 512 parts -> 4096 slots, 1024 -> 2048, 2048 -> 1024
int part_slots(int64_t num_parts) {
  return num_parts == 1024 ? 2048 : (num_parts == 2048 ? 1024 : 4096);
}

// partition histogram of int64 `keys` as exclusive offsets [P+1]
at::Tensor part_offsets(const at::Tensor& keys, int64_t num_parts, int shift,
                        hipStream_t stream) {
  auto hist = at::zeros({num_parts}, keys.options());
  launch_gb_part_hist(keys.data_ptr<int64_t>(), keys.numel(), shift,
                      hist.data_ptr<int64_t>(), (int)num_parts, stream);
  auto offsets = at::zeros({num_parts + 1}, keys.options());
  offsets.narrow(0, 1, num_parts).copy_(at::cumsum(hist, 0));
  return offsets;
}

// empty global group table: keys at GB_EMPTY, aggregates and counts 0
struct GroupTable {
  at::Tensor tkeys, gaggs, gcount;
};
GroupTable empty_group_table(int64_t n_aggs, int64_t tsize,
                             const at::Tensor& vals) {
  auto kopts = vals.options().dtype(at::kLong);
  return {at::full({tsize}, (int64_t)GB_EMPTY, kopts),
          at::zeros({n_aggs, tsize}, vals.options()),
          at::zeros({tsize}, kopts)};
}

}  // namespace


// Combine one column into the running row hash (out int64 viewed as u64).
void hash_column(at::Tensor data, c10::optional<at::Tensor> valid,
                 at::Tensor out, bool is_first) {
  check_gpu(data, "data");
  check_gpu(out, "out");
  int64_t n = data.numel();
  TORCH_CHECK(out.numel() == n, "out size mismatch");
  auto stream = current_stream();
  uint64_t* optr = reinterpret_cast<uint64_t*>(out.data_ptr<int64_t>());
  const bool* vptr = opt_valid_ptr(valid);
  switch (data.scalar_type()) {
    case at::kLong:
      launch_hash_col_i64(data.data_ptr<int64_t>(), vptr, optr, n, is_first,
                          stream);
      break;
    case at::kInt:
      launch_hash_col_i32(data.data_ptr<int32_t>(), vptr, optr, n, is_first,
                          stream);
      break;
    case at::kDouble:
      launch_hash_col_f64(data.data_ptr<double>(), vptr, optr, n, is_first,
                          stream);
      break;
    case at::kFloat:
      launch_hash_col_f32(data.data_ptr<float>(), vptr, optr, n, is_first,
                          stream);
      break;
    case at::kChar:
    case at::kBool:
      launch_hash_col_i8((const int8_t*)data.data_ptr(), vptr, optr, n,
                         is_first, stream);
      break;
    default:
      TORCH_CHECK(false, "unsupported dtype for hash_column");
  }
}

at::Tensor bucket_of(at::Tensor hashes, int64_t num_buckets) {
  check_gpu(hashes, "hashes");
  int64_t n = hashes.numel();
  auto buckets = at::empty({n}, hashes.options().dtype(at::kInt));
  launch_bucket_of(
      reinterpret_cast<const uint64_t*>(hashes.data_ptr<int64_t>()),
      buckets.data_ptr<int32_t>(), n, (int32_t)num_buckets, current_stream());
  return buckets;
}

at::Tensor bucket_histogram(at::Tensor buckets, int64_t num_buckets) {
  check_gpu(buckets, "buckets");
  auto hist = at::zeros({num_buckets}, buckets.options().dtype(at::kLong));
  launch_histogram(buckets.data_ptr<int32_t>(), hist.data_ptr<int64_t>(),
                   buckets.numel(), (int32_t)num_buckets, current_stream());
  return hist;
}

at::Tensor bucket_scatter(at::Tensor buckets, at::Tensor offsets) {
  // offsets: exclusive prefix sum of the histogram (int64, on device);
  // mutated in-place as the scatter cursor.
  check_gpu(buckets, "buckets");
  check_gpu(offsets, "offsets");
  int64_t n = buckets.numel();
  auto perm = at::empty({n}, buckets.options().dtype(at::kLong));
  launch_scatter(buckets.data_ptr<int32_t>(), offsets.data_ptr<int64_t>(),
                 perm.data_ptr<int64_t>(), n, current_stream());
  return perm;
}

std::vector<at::Tensor> gb_aggregate(at::Tensor keys, at::Tensor vals,
                                     c10::optional<at::Tensor> valids,
                                     at::Tensor ops, int64_t tsize,
                                     bool use_lds) {
  check_gpu(keys, "keys");
  check_gpu(vals, "vals");
  check_gpu(ops, "ops");
  TORCH_CHECK((tsize & (tsize - 1)) == 0, "tsize must be a power of 2");
  int64_t n = keys.numel();
  int n_aggs = (int)vals.size(0);
  TORCH_CHECK(vals.dim() == 2 && vals.size(1) == n, "vals must be [A, n]");
  auto t = empty_group_table(n_aggs, tsize, vals);
  // init aggs to op-appropriate identity: sum/count -> 0; min -> +inf; max -> -inf
  auto ops_cpu = ops.to(at::kCPU);
  for (int a = 0; a < n_aggs; ++a) {
    int op = ops_cpu[a].item<int32_t>();
    if (op == 1) t.gaggs[a].fill_(std::numeric_limits<double>::infinity());
    if (op == 2) t.gaggs[a].fill_(-std::numeric_limits<double>::infinity());
  }
  launch_gb_aggregate(keys.data_ptr<int64_t>(), vals.data_ptr<double>(),
                      opt_valid_ptr(valids), ops.data_ptr<int32_t>(), n_aggs,
                      n, t.tkeys.data_ptr<int64_t>(),
                      t.gaggs.data_ptr<double>(),
                      t.gcount.data_ptr<int64_t>(), tsize, use_lds ? 1 : 0,
                      current_stream());
  return {t.tkeys, t.gaggs, t.gcount};
}

std::vector<at::Tensor> gb_aggregate_partitioned(
    at::Tensor keys, at::Tensor vals, at::Tensor ops, int64_t num_parts,
    int64_t tsize, int64_t scatter_chunk, int64_t agg_chunk, int64_t narrow,
    bool record_layout, bool force_simple, int64_t record_chunk) {
  check_gpu(keys, "keys");
  check_gpu(vals, "vals");
  TORCH_CHECK((tsize & (tsize - 1)) == 0, "tsize must be a power of 2");
  TORCH_CHECK((num_parts & (num_parts - 1)) == 0,
              "num_parts must be a power of 2");
  TORCH_CHECK(num_parts <= PART_MAX, "num_parts must be <= ", PART_MAX);
  int64_t n = keys.numel();
  int n_aggs = (int)vals.size(0);
  auto stream = current_stream();
  int shift = part_shift(num_parts);
  bool staged =
      (n_aggs == 1 &&
       (num_parts == 512 || num_parts == 1024 || num_parts == 2048));
  // layout recording goes through the simple scatter (it has each
  // row's spill position in hand); replay restores the staged-path
  // spill format (narrow keys done by the caller)
  record_layout = record_layout && n_aggs == 1 && n < (int64_t(1) << 31);
  if (record_layout || force_simple) staged = false;
  // the simple per-partition kernel holds its aggregates in a fixed
  // [GB_LDS_MAX_AGGS x 1024] LDS array
  TORCH_CHECK(staged || n_aggs <= GB_LDS_MAX_AGGS,
              "the partitioned group-by takes at most ", GB_LDS_MAX_AGGS,
              " aggregates per call, got ", n_aggs);
  // narrow < 0 = speculative: run the int32 path with an in-kernel
  // overflow flag; the CALLER checks the returned flag at its existing
  // sync point and re-runs wide if set (no mid-pipeline sync here)
  bool speculative = staged && narrow < 0;
  if (speculative) narrow = 1;
  // phase 1: histogram + scan
  auto offsets = part_offsets(keys, num_parts, shift, stream);
  auto cursor = offsets.narrow(0, 0, num_parts).clone();
  // phase 2: scatter into partitioned order
  bool use_narrow = staged && narrow > 0;
  auto pkeys = use_narrow
                   ? at::empty({n}, keys.options().dtype(at::kInt))
                   : at::empty({n}, keys.options());
  auto pvals = at::empty({n_aggs, n}, vals.options());
  auto ovf = at::zeros({1}, keys.options().dtype(at::kInt));
  auto pos = at::empty({record_layout ? n : 0},
                       keys.options().dtype(at::kInt));
  if (staged) {
    launch_gb_part_scatter_staged(
        keys.data_ptr<int64_t>(), vals.data_ptr<double>(), n, shift,
        cursor.data_ptr<int64_t>(), pkeys.data_ptr(),
        pvals.data_ptr<double>(), scatter_chunk, use_narrow ? 1 : 0,
        (use_narrow && speculative) ? ovf.data_ptr<int32_t>() : nullptr,
        (int)num_parts, stream);
  } else {
    launch_gb_part_scatter(keys.data_ptr<int64_t>(), vals.data_ptr<double>(),
                           n_aggs, n, shift, cursor.data_ptr<int64_t>(),
                           pkeys.data_ptr<int64_t>(), pvals.data_ptr<double>(),
                           (int)num_parts,
                           record_layout ? pos.data_ptr<int32_t>() : nullptr,
                           record_layout ? record_chunk : 0, stream);
  }
  // phase 3: per-partition LDS aggregation into the global table
  auto t = empty_group_table(n_aggs, tsize, vals);
  if (staged) {
    launch_gb_aggregate_part_big(
        pkeys.data_ptr(), pvals.data_ptr<double>(),
        ops.data_ptr<int32_t>(), n, t.tkeys.data_ptr<int64_t>(),
        t.gaggs.data_ptr<double>(), t.gcount.data_ptr<int64_t>(), tsize,
        agg_chunk, use_narrow ? 1 : 0, part_slots(num_parts), stream);
  } else {
    launch_gb_aggregate_part(
        pkeys.data_ptr<int64_t>(), pvals.data_ptr<double>(),
        ops.data_ptr<int32_t>(), n_aggs, n, offsets.data_ptr<int64_t>(),
        num_parts, t.tkeys.data_ptr<int64_t>(), t.gaggs.data_ptr<double>(),
        t.gcount.data_ptr<int64_t>(), tsize, stream);
  }
  return {t.tkeys, t.gaggs, t.gcount, ovf, pkeys, pos};
}

// Phase 2+3 only, with a recorded layout: place the fresh values at
// the recorded spill positions and aggregate against the cached
// partitioned keys (phase 1 + key scatter skipped entirely).
std::vector<at::Tensor> gb_aggregate_replay(at::Tensor pkeys_cached,
                                            at::Tensor pos, at::Tensor vals,
                                            at::Tensor ops, int64_t num_parts,
                                            int64_t tsize,
                                            int64_t agg_chunk) {
  check_gpu(pkeys_cached, "pkeys");
  check_gpu(pos, "pos");
  check_gpu(vals, "vals");
  TORCH_CHECK(vals.size(0) == 1, "replay supports single-agg spills");
  int64_t n = pos.numel();
  auto stream = current_stream();
  auto pvals = at::empty({1, n}, vals.options());
  launch_scatter_by_pos(vals.data_ptr<double>(), pos.data_ptr<int32_t>(), n,
                        pvals.data_ptr<double>(), stream);
  auto t = empty_group_table(1, tsize, vals);
  launch_gb_aggregate_part_big(
      pkeys_cached.data_ptr(), pvals.data_ptr<double>(),
      ops.data_ptr<int32_t>(), n, t.tkeys.data_ptr<int64_t>(),
      t.gaggs.data_ptr<double>(), t.gcount.data_ptr<int64_t>(), tsize,
      agg_chunk, pkeys_cached.element_size() == 4 ? 1 : 0,
      part_slots(num_parts), stream);
  return {t.tkeys, t.gaggs, t.gcount};
}

// ---- dense replay (groupby_replay.hip "shuffle-layout reuse") ----

namespace {
void check_tile(int64_t tile) {
  TORCH_CHECK(tile >= 512 && tile <= 8192 && (tile & (tile - 1)) == 0,
              "tile must be a power of 2 in [512, 8192]");
}
void check_dense_slots(int64_t slots) {
  TORCH_CHECK(slots == 2048 || slots == 4096 || slots == 8192,
              "dense table slots must be 2048, 4096 or 8192");
}
}  // namespace

// Preparation pass 1: per-partition offsets of the recorded partitioned
// keys (re-histogrammed: same hash, same partition ids) and the number
// of distinct keys in every partition.  A count above dense_assign_max
// means the partition overflowed the id-assignment table.
std::vector<at::Tensor> gb_dense_count(at::Tensor pkeys, int64_t num_parts) {
  check_gpu(pkeys, "pkeys");
  TORCH_CHECK(pkeys.scalar_type() == at::kLong, "pkeys must be int64");
  TORCH_CHECK(num_parts >= 1 && num_parts <= PART_MAX &&
                  (num_parts & (num_parts - 1)) == 0,
              "num_parts must be a power of 2 <= ", PART_MAX);
  auto stream = current_stream();
  auto offsets =
      part_offsets(pkeys, num_parts, part_shift(num_parts), stream);
  auto distinct = at::empty({num_parts}, pkeys.options());
  launch_gb_dense_count(pkeys.data_ptr<int64_t>(),
                        offsets.data_ptr<int64_t>(), (int)num_parts,
                        distinct.data_ptr<int64_t>(), stream);
  return {offsets, distinct};
}

// Preparation pass 2: dense group id of every partitioned row plus the
// output keys and counts in id order.  group_base is the exclusive scan
// of the pass-1 distinct counts ([P+1]); the caller has checked that no
// count exceeds dense_assign_max and that n_groups < 2^31.
std::vector<at::Tensor> gb_dense_assign(at::Tensor pkeys, at::Tensor offsets,
                                        at::Tensor group_base,
                                        int64_t n_groups) {
  check_gpu(pkeys, "pkeys");
  check_gpu(offsets, "offsets");
  check_gpu(group_base, "group_base");
  TORCH_CHECK(pkeys.scalar_type() == at::kLong, "pkeys must be int64");
  TORCH_CHECK(offsets.scalar_type() == at::kLong &&
                  group_base.scalar_type() == at::kLong,
              "offsets/group_base must be int64");
  int64_t num_parts = offsets.numel() - 1;
  TORCH_CHECK(num_parts >= 1 && group_base.numel() == num_parts + 1,
              "offsets/group_base must be [P+1]");
  TORCH_CHECK(n_groups >= 0 && n_groups < (int64_t(1) << 31),
              "n_groups must fit int32");
  int64_t n = pkeys.numel();
  auto gid = at::empty({n}, pkeys.options().dtype(at::kInt));
  auto out_keys = at::empty({n_groups}, pkeys.options());
  auto out_count = at::empty({n_groups}, pkeys.options());
  launch_gb_dense_assign(pkeys.data_ptr<int64_t>(),
                         offsets.data_ptr<int64_t>(),
                         group_base.data_ptr<int64_t>(), (int)num_parts,
                         gid.data_ptr<int32_t>(), out_keys.data_ptr<int64_t>(),
                         out_count.data_ptr<int64_t>(), current_stream());
  return {gid, out_keys, out_count};
}

// Preparation of the tile-coalesced scatter for a permutation `pos`:
// (rank [n] int16 holding uint16 tile-local ranks, dst [n] int32).
std::vector<at::Tensor> scatter_tile_prepare(at::Tensor pos, int64_t tile) {
  check_gpu(pos, "pos");
  TORCH_CHECK(pos.scalar_type() == at::kInt, "pos must be int32");
  check_tile(tile);
  int64_t n = pos.numel();
  auto rank = at::empty({n}, pos.options().dtype(at::kShort));
  auto dst = at::empty({n}, pos.options());
  if (n > 0) {
    launch_scatter_tile_prep(pos.data_ptr<int32_t>(), n, (int)tile,
                             (uint16_t*)rank.data_ptr<int16_t>(),
                             dst.data_ptr<int32_t>(), current_stream());
  }
  return {rank, dst};
}

namespace {
void scatter_tile_into(const at::Tensor& vals, const at::Tensor& rank,
                       const at::Tensor& dst, int64_t tile, at::Tensor& out) {
  check_gpu(vals, "vals");
  check_gpu(rank, "rank");
  check_gpu(dst, "dst");
  check_tile(tile);
  int64_t n = dst.numel();
  TORCH_CHECK(vals.scalar_type() == at::kDouble && vals.numel() == n,
              "vals must be fp64 [n]");
  TORCH_CHECK(rank.scalar_type() == at::kShort && rank.numel() == n,
              "rank must be int16 [n]");
  TORCH_CHECK(dst.scalar_type() == at::kInt, "dst must be int32");
  if (n > 0) {
    launch_scatter_tile(vals.data_ptr<double>(),
                        (const uint16_t*)rank.data_ptr<int16_t>(),
                        dst.data_ptr<int32_t>(), n, (int)tile,
                        out.data_ptr<double>(), current_stream());
  }
}

void dense_aggregate_into(const at::Tensor& gid, const at::Tensor& pvals,
                          const at::Tensor& offsets,
                          const at::Tensor& group_base, int64_t chunk,
                          int64_t slots, at::Tensor& out_sum) {
  check_gpu(gid, "gid");
  check_gpu(pvals, "pvals");
  check_gpu(offsets, "offsets");
  check_gpu(group_base, "group_base");
  check_dense_slots(slots);
  int64_t n = gid.numel();
  TORCH_CHECK(gid.scalar_type() == at::kInt, "gid must be int32");
  TORCH_CHECK(pvals.scalar_type() == at::kDouble && pvals.numel() == n,
              "pvals must be fp64 [n]");
  TORCH_CHECK(offsets.scalar_type() == at::kLong &&
                  group_base.scalar_type() == at::kLong &&
                  offsets.numel() >= 2 &&
                  group_base.numel() == offsets.numel(),
              "offsets/group_base must be int64 [P+1]");
  TORCH_CHECK(chunk >= 0, "chunk must be >= 0");
  if (n > 0) {
    launch_gb_dense_aggregate(
        gid.data_ptr<int32_t>(), pvals.data_ptr<double>(), n,
        offsets.data_ptr<int64_t>(), group_base.data_ptr<int64_t>(),
        (int)(offsets.numel() - 1), out_sum.numel(),
        out_sum.data_ptr<double>(), chunk, (int)slots, current_stream());
  }
}
}  // namespace

// out[pos[i]] = vals[i] through the prepared (rank, dst) tile layout
at::Tensor scatter_tile(at::Tensor vals, at::Tensor rank, at::Tensor dst,
                        int64_t tile) {
  auto out = at::empty({dst.numel()}, vals.options());
  scatter_tile_into(vals, rank, dst, tile, out);
  return out;
}

// out_sum[g] = sum of pvals[j] over gid[j] == g, for partition-major ids
at::Tensor gb_dense_aggregate(at::Tensor gid, at::Tensor pvals,
                              at::Tensor offsets, at::Tensor group_base,
                              int64_t n_groups, int64_t chunk,
                              int64_t slots) {
  TORCH_CHECK(n_groups >= 0 && n_groups < (int64_t(1) << 31),
              "n_groups must fit int32");
  auto out_sum = at::zeros({n_groups}, pvals.options());
  dense_aggregate_into(gid, pvals, offsets, group_base, chunk, slots,
                       out_sum);
  return out_sum;
}

// One replayed step: place the fresh values and add them per dense
// group id.  The layout carries either (rank, dst) for the
// tile-coalesced scatter or the recorded positions `pos`.  Returns the
// [G] sums in id order.
at::Tensor gb_replay_dense(at::Tensor vals, at::Tensor gid,
                           at::Tensor offsets, at::Tensor group_base,
                           int64_t n_groups, int64_t chunk, int64_t slots,
                           int64_t tile, c10::optional<at::Tensor> rank,
                           c10::optional<at::Tensor> dst,
                           c10::optional<at::Tensor> pos) {
  check_gpu(vals, "vals");
  int64_t n = gid.numel();
  TORCH_CHECK(vals.scalar_type() == at::kDouble && vals.numel() == n,
              "vals must be fp64 [1, n]");
  TORCH_CHECK(n_groups >= 0 && n_groups < (int64_t(1) << 31),
              "n_groups must fit int32");
  TORCH_CHECK(pos.has_value() != (rank.has_value() && dst.has_value()),
              "pass either pos or rank and dst");
  auto pvals = at::empty({n}, vals.options());
  if (pos.has_value()) {
    check_gpu(*pos, "pos");
    TORCH_CHECK(pos->scalar_type() == at::kInt && pos->numel() == n,
                "pos must be int32 [n]");
    if (n > 0) {
      launch_scatter_by_pos(vals.data_ptr<double>(), pos->data_ptr<int32_t>(),
                            n, pvals.data_ptr<double>(), current_stream());
    }
  } else {
    TORCH_CHECK(dst->numel() == n, "dst must be int32 [n]");
    scatter_tile_into(vals.view({n}), *rank, *dst, tile, pvals);
  }
  auto out_sum = at::zeros({n_groups}, vals.options());
  dense_aggregate_into(gid, pvals, offsets, group_base, chunk, slots,
                       out_sum);
  return out_sum;
}

// ---- binned dense replay: values laid out by bins of M partitions ----

namespace {
// bin arrays are int64 [B+1] on the GPU; returns B
int64_t check_bins(const at::Tensor& bin_offsets) {
  check_gpu(bin_offsets, "bin_offsets");
  TORCH_CHECK(bin_offsets.scalar_type() == at::kLong &&
                  bin_offsets.dim() == 1 && bin_offsets.numel() >= 2 &&
                  bin_offsets.numel() - 1 <= BIN_MAX,
              "bin_offsets must be int64 [B+1], B <= ", BIN_MAX);
  return bin_offsets.numel() - 1;
}

void dense_aggregate_binned_into(const at::Tensor& gid,
                                 const at::Tensor& pvals,
                                 const at::Tensor& bin_offsets,
                                 const at::Tensor& bin_group_base,
                                 const at::Tensor& bin_chunk_base,
                                 int64_t total_chunks, int64_t chunk,
                                 int64_t slots, at::Tensor& out_sum) {
  check_gpu(gid, "gid");
  check_gpu(pvals, "pvals");
  int64_t nbins = check_bins(bin_offsets);
  check_gpu(bin_group_base, "bin_group_base");
  check_gpu(bin_chunk_base, "bin_chunk_base");
  check_dense_slots(slots);
  int64_t n = gid.numel();
  TORCH_CHECK(gid.scalar_type() == at::kInt, "gid must be int32");
  TORCH_CHECK(pvals.scalar_type() == at::kDouble && pvals.numel() == n,
              "pvals must be fp64 [n]");
  TORCH_CHECK(bin_group_base.scalar_type() == at::kLong &&
                  bin_chunk_base.scalar_type() == at::kLong &&
                  bin_group_base.numel() == nbins + 1 &&
                  bin_chunk_base.numel() == nbins + 1,
              "bin_group_base/bin_chunk_base must be int64 [B+1]");
  TORCH_CHECK(chunk >= 1, "chunk must be >= 1");
  TORCH_CHECK(total_chunks >= 0, "total_chunks must be >= 0");
  if (n > 0 && total_chunks > 0) {
    launch_gb_dense_aggregate_binned(
        gid.data_ptr<int32_t>(), pvals.data_ptr<double>(), n,
        bin_offsets.data_ptr<int64_t>(), bin_group_base.data_ptr<int64_t>(),
        bin_chunk_base.data_ptr<int64_t>(), (int)nbins, total_chunks,
        out_sum.numel(), out_sum.data_ptr<double>(), chunk, (int)slots,
        current_stream());
  }
}
}  // namespace

// Preparation of the tile-coalesced scatter into the binned layout.  pos
// is every row's recorded position, gid the dense ids by recorded
// position, bin_offsets [B+1] the first recorded position of every bin.
// A row goes to bin_offsets[b] + (rows of bin b in earlier tiles) + (its
// rank among the bin-b rows of its own tile, by recorded position), so
// every (tile, bin) is one contiguous run and the runs of consecutive
// tiles are adjacent.  Returns (rank, dst, gid in the new order).
std::vector<at::Tensor> scatter_tile_prepare_binned(at::Tensor pos,
                                                    at::Tensor gid,
                                                    at::Tensor bin_offsets,
                                                    int64_t tile) {
  check_gpu(pos, "pos");
  check_gpu(gid, "gid");
  TORCH_CHECK(pos.scalar_type() == at::kInt, "pos must be int32");
  int64_t n = pos.numel();
  TORCH_CHECK(gid.scalar_type() == at::kInt && gid.numel() == n,
              "gid must be int32 [n]");
  check_tile(tile);
  int64_t nbins = check_bins(bin_offsets);
  auto rank = at::empty({n}, pos.options().dtype(at::kShort));
  auto dst = at::empty({n}, pos.options());
  auto gid_new = at::empty({n}, pos.options());
  if (n == 0) return {rank, dst, gid_new};
  auto stream = current_stream();
  int64_t ntiles = (n + tile - 1) / tile;
  auto counts = at::empty({ntiles, nbins}, pos.options());
  launch_scatter_bin_count(pos.data_ptr<int32_t>(), n, (int)tile,
                           bin_offsets.data_ptr<int64_t>(), (int)nbins,
                           counts.data_ptr<int32_t>(), stream);
  // run_delta[t][b] = bin_offsets[b] + rows of bin b in tiles before t
  //                   - rows of tile t in bins before b
  auto run_delta = (bin_offsets.slice(0, 0, nbins).unsqueeze(0) +
                    (counts.cumsum(0, at::kLong) - counts) -
                    (counts.cumsum(1, at::kLong) - counts))
                       .contiguous();
  launch_scatter_tile_prep_binned(
      pos.data_ptr<int32_t>(), n, (int)tile, bin_offsets.data_ptr<int64_t>(),
      (int)nbins, run_delta.data_ptr<int64_t>(), gid.data_ptr<int32_t>(),
      (uint16_t*)rank.data_ptr<int16_t>(), dst.data_ptr<int32_t>(),
      gid_new.data_ptr<int32_t>(), stream);
  return {rank, dst, gid_new};
}

// out_sum[g] = sum of pvals[j] over gid[j] == g for rows laid out by
// bins.  bin_group_base [B+1] is the first id of every bin,
// bin_chunk_base [B+1] the prefix of ceil(rows_b / chunk) and
// total_chunks its last entry.
at::Tensor gb_dense_aggregate_binned(at::Tensor gid, at::Tensor pvals,
                                     at::Tensor bin_offsets,
                                     at::Tensor bin_group_base,
                                     at::Tensor bin_chunk_base,
                                     int64_t total_chunks, int64_t n_groups,
                                     int64_t chunk, int64_t slots) {
  TORCH_CHECK(n_groups >= 0 && n_groups < (int64_t(1) << 31),
              "n_groups must fit int32");
  auto out_sum = at::zeros({n_groups}, pvals.options());
  dense_aggregate_binned_into(gid, pvals, bin_offsets, bin_group_base,
                              bin_chunk_base, total_chunks, chunk, slots,
                              out_sum);
  return out_sum;
}

// One replayed step over the binned layout: the tile scatter with the
// binned (rank, dst), then the bin-aligned aggregate.
at::Tensor gb_replay_binned(at::Tensor vals, at::Tensor gid, at::Tensor rank,
                            at::Tensor dst, at::Tensor bin_offsets,
                            at::Tensor bin_group_base,
                            at::Tensor bin_chunk_base, int64_t total_chunks,
                            int64_t n_groups, int64_t chunk, int64_t slots,
                            int64_t tile) {
  check_gpu(vals, "vals");
  int64_t n = gid.numel();
  TORCH_CHECK(vals.scalar_type() == at::kDouble && vals.numel() == n,
              "vals must be fp64 [1, n]");
  TORCH_CHECK(n_groups >= 0 && n_groups < (int64_t(1) << 31),
              "n_groups must fit int32");
  TORCH_CHECK(dst.numel() == n, "dst must be int32 [n]");
  auto pvals = at::empty({n}, vals.options());
  scatter_tile_into(vals.view({n}), rank, dst, tile, pvals);
  auto out_sum = at::zeros({n_groups}, vals.options());
  dense_aggregate_binned_into(gid, pvals, bin_offsets, bin_group_base,
                              bin_chunk_base, total_chunks, chunk, slots,
                              out_sum);
  return out_sum;
}

// ---- compact binned dense replay: no per-row dst, 16-bit ids ----

namespace {
void scatter_tile_compact_into(const at::Tensor& vals, const at::Tensor& rank,
                               const at::Tensor& tile_start,
                               const at::Tensor& tile_delta, int64_t tile,
                               int64_t threads, at::Tensor& out) {
  check_gpu(vals, "vals");
  check_gpu(rank, "rank");
  check_gpu(tile_start, "tile_start");
  check_gpu(tile_delta, "tile_delta");
  check_tile(tile);
  TORCH_CHECK(threads == 0 || threads == 512 || threads == 1024,
              "threads must be 0, 512 or 1024");
  int64_t n = rank.numel();
  int64_t ntiles = (n + tile - 1) / tile;
  TORCH_CHECK(vals.scalar_type() == at::kDouble && vals.numel() == n &&
                  vals.is_contiguous(),
              "vals must be contiguous fp64 [n]");
  TORCH_CHECK(rank.scalar_type() == at::kShort && rank.is_contiguous(),
              "rank must be contiguous int16 [n]");
  TORCH_CHECK(tile_delta.scalar_type() == at::kInt && tile_delta.dim() == 2 &&
                  tile_delta.is_contiguous() &&
                  tile_delta.size(0) == ntiles && tile_delta.size(1) >= 1 &&
                  tile_delta.size(1) <= SCATTER_COMPACT_MAX_BINS,
              "tile_delta must be int32 [tiles, B], B <= ",
              SCATTER_COMPACT_MAX_BINS);
  int64_t nbins = tile_delta.size(1);
  TORCH_CHECK(tile_start.scalar_type() == at::kShort &&
                  tile_start.dim() == 2 && tile_start.is_contiguous() &&
                  tile_start.size(0) == ntiles &&
                  tile_start.size(1) == nbins + 1,
              "tile_start must be int16 [tiles, B+1]");
  if (n > 0) {
    int err = launch_scatter_tile_compact(
        vals.data_ptr<double>(), (const uint16_t*)rank.data_ptr<int16_t>(),
        (const uint16_t*)tile_start.data_ptr<int16_t>(),
        tile_delta.data_ptr<int32_t>(), (int)nbins, n, (int)tile,
        out.data_ptr<double>(), (int)threads, current_stream());
    TORCH_CHECK(err == 0, "scatter_tile_compact launch failed: HIP error ",
                err);
  }
}

void dense_aggregate_compact_into(const at::Tensor& rel,
                                  const at::Tensor& pvals,
                                  const at::Tensor& bin_offsets,
                                  const at::Tensor& bin_group_base,
                                  const at::Tensor& bin_chunk_base,
                                  int64_t total_chunks, int64_t chunk,
                                  int64_t slots, at::Tensor& out_sum) {
  check_gpu(rel, "rel");
  check_gpu(pvals, "pvals");
  int64_t nbins = check_bins(bin_offsets);
  check_gpu(bin_group_base, "bin_group_base");
  check_gpu(bin_chunk_base, "bin_chunk_base");
  check_dense_slots(slots);
  int64_t n = rel.numel();
  TORCH_CHECK(rel.scalar_type() == at::kShort && rel.is_contiguous(),
              "rel must be contiguous int16");
  TORCH_CHECK(pvals.scalar_type() == at::kDouble && pvals.numel() == n &&
                  pvals.is_contiguous(),
              "pvals must be contiguous fp64 [n]");
  // the kernel reads four ids and two pairs of values per load
  TORCH_CHECK(n == 0 ||
                  ((uintptr_t)rel.data_ptr() % 8 == 0 &&
                   (uintptr_t)pvals.data_ptr() % 16 == 0),
              "rel must be 8-byte and pvals 16-byte aligned");
  TORCH_CHECK(bin_group_base.scalar_type() == at::kLong &&
                  bin_chunk_base.scalar_type() == at::kLong &&
                  bin_group_base.numel() == nbins + 1 &&
                  bin_chunk_base.numel() == nbins + 1,
              "bin_group_base/bin_chunk_base must be int64 [B+1]");
  TORCH_CHECK(chunk >= 1, "chunk must be >= 1");
  TORCH_CHECK(total_chunks >= 0, "total_chunks must be >= 0");
  if (n > 0 && total_chunks > 0) {
    launch_gb_dense_aggregate_compact(
        (const uint16_t*)rel.data_ptr<int16_t>(), pvals.data_ptr<double>(), n,
        bin_offsets.data_ptr<int64_t>(), bin_group_base.data_ptr<int64_t>(),
        bin_chunk_base.data_ptr<int64_t>(), (int)nbins, total_chunks,
        out_sum.numel(), out_sum.data_ptr<double>(), chunk, (int)slots,
        current_stream());
  }
}
}  // namespace

// scatter_tile_prepare_binned without the per-row arrays it can do
// without: the same layout (same destination for every row), returned as
//   rank       [n] int16 holding uint16, identical to the binned one
//   rel        [n] int16 holding uint16, in binned order: the row's dense
//              id less bin_group_base[its bin]
//   tile_start [tiles, B+1] int16: first tile-local rank of every bin (the
//              exclusive row prefix of the count matrix); the last column
//              is the tile's placed rows, below the tile's row count only
//              when pos is no permutation
//   tile_delta [tiles, B] int32: destination of rank r of bin b is
//              tile_delta[t][b] + r
// With keep_gid a fifth tensor follows: gid [n] int32 in binned order, as
// scatter_tile_prepare_binned returns it (for the 32-bit aggregate).
// One host readback checks that no bin is wider than 65536 ids.
std::vector<at::Tensor> scatter_tile_prepare_compact(
    at::Tensor pos, at::Tensor gid, at::Tensor bin_offsets,
    at::Tensor bin_group_base, int64_t tile, bool keep_gid) {
  check_gpu(pos, "pos");
  check_gpu(gid, "gid");
  check_gpu(bin_group_base, "bin_group_base");
  TORCH_CHECK(pos.scalar_type() == at::kInt, "pos must be int32");
  int64_t n = pos.numel();
  TORCH_CHECK(gid.scalar_type() == at::kInt && gid.numel() == n,
              "gid must be int32 [n]");
  check_tile(tile);
  int64_t nbins = check_bins(bin_offsets);
  TORCH_CHECK(nbins <= SCATTER_COMPACT_MAX_BINS, "at most ",
              SCATTER_COMPACT_MAX_BINS, " bins in the compact layout");
  TORCH_CHECK(bin_group_base.scalar_type() == at::kLong &&
                  bin_group_base.numel() == nbins + 1,
              "bin_group_base must be int64 [B+1]");
  auto i16 = pos.options().dtype(at::kShort);
  int64_t ntiles = (n + tile - 1) / tile;
  auto rank = at::empty({n}, i16);
  auto rel = at::empty({n}, i16);
  at::Tensor gid_new;
  if (keep_gid) gid_new = at::empty({n}, pos.options());
  if (n == 0) {
    std::vector<at::Tensor> res = {rank, rel, at::empty({0, nbins + 1}, i16),
                                   at::empty({0, nbins}, pos.options())};
    if (keep_gid) res.push_back(gid_new);
    return res;
  }
  TORCH_CHECK((bin_group_base.slice(0, 1) - bin_group_base.slice(0, 0, nbins))
                      .max()
                      .item<int64_t>() <= 65536,
              "a bin wider than 65536 ids does not fit 16-bit ids");
  auto stream = current_stream();
  auto counts = at::empty({ntiles, nbins}, pos.options());
  launch_scatter_bin_count(pos.data_ptr<int32_t>(), n, (int)tile,
                           bin_offsets.data_ptr<int64_t>(), (int)nbins,
                           counts.data_ptr<int32_t>(), stream);
  auto row_incl = counts.cumsum(1, at::kLong);
  auto start = row_incl - counts;
  // bin_offsets[b] + rows of bin b in tiles before t - start[t][b]; never
  // below -tile, and n < 2^31 because pos is int32
  auto tile_delta = (bin_offsets.slice(0, 0, nbins).unsqueeze(0) +
                     (counts.cumsum(0, at::kLong) - counts) - start)
                        .to(at::kInt)
                        .contiguous();
  auto tile_start = at::cat({start, row_incl.slice(1, nbins - 1, nbins)}, 1)
                        .to(at::kShort)
                        .contiguous();
  launch_scatter_tile_prep_compact(
      pos.data_ptr<int32_t>(), n, (int)tile, bin_offsets.data_ptr<int64_t>(),
      bin_group_base.data_ptr<int64_t>(), (int)nbins,
      tile_delta.data_ptr<int32_t>(), gid.data_ptr<int32_t>(),
      (uint16_t*)rank.data_ptr<int16_t>(), (uint16_t*)rel.data_ptr<int16_t>(),
      keep_gid ? gid_new.data_ptr<int32_t>() : nullptr, stream);
  std::vector<at::Tensor> res = {rank, rel, tile_start, tile_delta};
  if (keep_gid) res.push_back(gid_new);
  return res;
}

// out[tile_delta[t][bin of r] + r] = value of tile t's r-th ranked row.
// `out` (fp64 [n], contiguous) is written in place when given.
at::Tensor scatter_tile_compact(at::Tensor vals, at::Tensor rank,
                                at::Tensor tile_start, at::Tensor tile_delta,
                                int64_t tile, int64_t threads,
                                c10::optional<at::Tensor> out_opt) {
  if (out_opt.has_value()) {
    check_gpu(*out_opt, "out");
    TORCH_CHECK(out_opt->scalar_type() == at::kDouble &&
                    out_opt->is_contiguous() &&
                    out_opt->numel() == rank.numel(),
                "out must be contiguous fp64 [n]");
  }
  auto out = out_opt.has_value() ? *out_opt
                                 : at::empty({rank.numel()}, vals.options());
  scatter_tile_compact_into(vals, rank, tile_start, tile_delta, tile, threads,
                            out);
  return out;
}

// gb_dense_aggregate_binned over the 16-bit ids of the compact layout.
// With `out` (contiguous fp64, at least n_groups long) the sums are ADDED
// to its first n_groups elements and that view is returned.
at::Tensor gb_dense_aggregate_compact(at::Tensor rel, at::Tensor pvals,
                                      at::Tensor bin_offsets,
                                      at::Tensor bin_group_base,
                                      at::Tensor bin_chunk_base,
                                      int64_t total_chunks, int64_t n_groups,
                                      int64_t chunk, int64_t slots,
                                      c10::optional<at::Tensor> out_opt) {
  TORCH_CHECK(n_groups >= 0 && n_groups < (int64_t(1) << 31),
              "n_groups must fit int32");
  if (out_opt.has_value()) {
    check_gpu(*out_opt, "out");
    TORCH_CHECK(out_opt->scalar_type() == at::kDouble &&
                    out_opt->is_contiguous() && out_opt->dim() == 1 &&
                    out_opt->numel() >= n_groups,
                "out must be contiguous fp64 of at least n_groups");
  }
  auto out_sum = out_opt.has_value() ? out_opt->narrow(0, 0, n_groups)
                                     : at::zeros({n_groups}, pvals.options());
  dense_aggregate_compact_into(rel, pvals, bin_offsets, bin_group_base,
                               bin_chunk_base, total_chunks, chunk, slots,
                               out_sum);
  return out_sum;
}

// One replayed step over the compact binned layout: the compact tile
// scatter, then the aggregate `rel` selects: int16 (uint16 ids relative to
// the bin) the 16-bit one, int32 (the binned gid) the binned one.
at::Tensor gb_replay_compact(at::Tensor vals, at::Tensor rel, at::Tensor rank,
                             at::Tensor tile_start, at::Tensor tile_delta,
                             at::Tensor bin_offsets,
                             at::Tensor bin_group_base,
                             at::Tensor bin_chunk_base, int64_t total_chunks,
                             int64_t n_groups, int64_t chunk, int64_t slots,
                             int64_t tile, int64_t threads) {
  check_gpu(vals, "vals");
  int64_t n = rel.numel();
  TORCH_CHECK(vals.scalar_type() == at::kDouble && vals.numel() == n,
              "vals must be fp64 [1, n]");
  TORCH_CHECK(n_groups >= 0 && n_groups < (int64_t(1) << 31),
              "n_groups must fit int32");
  TORCH_CHECK(rank.numel() == n, "rank must be int16 [n]");
  auto pvals = at::empty({n}, vals.options());
  scatter_tile_compact_into(vals.view({n}), rank, tile_start, tile_delta, tile,
                            threads, pvals);
  auto out_sum = at::zeros({n_groups}, vals.options());
  if (rel.scalar_type() == at::kInt) {
    dense_aggregate_binned_into(rel, pvals, bin_offsets, bin_group_base,
                                bin_chunk_base, total_chunks, chunk, slots,
                                out_sum);
  } else {
    dense_aggregate_compact_into(rel, pvals, bin_offsets, bin_group_base,
                                 bin_chunk_base, total_chunks, chunk, slots,
                                 out_sum);
  }
  return out_sum;
}

std::vector<at::Tensor> join_build(at::Tensor keys, int64_t tsize) {
  check_gpu(keys, "keys");
  TORCH_CHECK((tsize & (tsize - 1)) == 0, "tsize must be a power of 2");
  int64_t n = keys.numel();
  auto heads = at::full({tsize}, -1, keys.options().dtype(at::kInt));
  auto next = at::empty({std::max<int64_t>(n, 1)},
                        keys.options().dtype(at::kInt));
  auto dup = at::zeros({1}, keys.options().dtype(at::kInt));
  if (n > 0) {
    launch_join_build(keys.data_ptr<int64_t>(), n, heads.data_ptr<int32_t>(),
                      next.data_ptr<int32_t>(), tsize,
                      dup.data_ptr<int32_t>(), current_stream());
  }
  return {heads, next, dup};
}


namespace {
const int64_t* opt_i64_ptr(const c10::optional<at::Tensor>& v) {
  if (!v.has_value()) return nullptr;
  return v->data_ptr<int64_t>();
}
}  // namespace

std::vector<at::Tensor> join_emit_unique(
    at::Tensor pkeys, at::Tensor bkeys, c10::optional<at::Tensor> ph2,
    c10::optional<at::Tensor> bh2, at::Tensor heads, at::Tensor next,
    int64_t mode, bool want_pi, bool want_mask, bool mask_neg) {
  check_gpu(pkeys, "pkeys");
  int64_t np = pkeys.numel();
  int64_t tsize = heads.numel();
  // positional mode (1) with want_pi=false skips the pi write — the
  // compaction kernel emits row indices itself; want_mask emits the
  // matched mask in the same pass (no separate compare kernel)
  auto out_pi = at::empty({(mode == 1 && !want_pi) ? 0 : np},
                          pkeys.options());
  auto out_bi = at::empty({np}, pkeys.options());
  auto cursor = at::zeros({1}, pkeys.options());
  auto out_mask = at::empty({want_mask && mode == 1 ? np : 0},
                            pkeys.options().dtype(at::kBool));
  if (np > 0) {
    launch_join_emit_unique(
        pkeys.data_ptr<int64_t>(), np, bkeys.data_ptr<int64_t>(),
        opt_i64_ptr(ph2), opt_i64_ptr(bh2), heads.data_ptr<int32_t>(),
        next.data_ptr<int32_t>(), tsize, (int)mode,
        out_pi.numel() > 0 ? out_pi.data_ptr<int64_t>() : nullptr,
        out_bi.data_ptr<int64_t>(), cursor.data_ptr<int64_t>(),
        out_mask.numel() > 0 ? out_mask.data_ptr<bool>() : nullptr,
        mask_neg ? 1 : 0, current_stream());
  }
  return {out_pi, out_bi, cursor, out_mask};
}

namespace {
// one operand of the join_unique_select comparison: (kind, value) with
// kind JSEL_PROBE / JSEL_BUILD and a column of that side's length, or
// JSEL_IMM and a Python int or float
void jsel_operand(const py::handle& spec, int s, int64_t np, int64_t nb,
                  JoinSelPred* p) {
  auto t = py::cast<py::tuple>(spec);
  TORCH_CHECK(t.size() == 2, "operand is (kind, value)");
  int kind = py::cast<int>(t[0]);
  p->kind[s] = kind;
  if (kind == JSEL_IMM) {
    if (py::isinstance<py::float_>(t[1])) {
      double d = py::cast<double>(t[1]);
      std::memcpy(&p->imm[s], &d, 8);
      p->is_f64[s] = 1;
    } else {
      TORCH_CHECK(py::isinstance<py::int_>(t[1]) &&
                      !py::isinstance<py::bool_>(t[1]),
                  "immediate must be an int or a float");
      p->imm[s] = (unsigned long long)py::cast<int64_t>(t[1]);
      p->is_f64[s] = 0;
    }
    return;
  }
  TORCH_CHECK(kind == JSEL_PROBE || kind == JSEL_BUILD, "operand kind");
  auto col = py::cast<at::Tensor>(t[1]);
  check_gpu(col, "predicate column");
  TORCH_CHECK(col.scalar_type() == at::kLong ||
                  col.scalar_type() == at::kDouble,
              "predicate columns are int64 or float64");
  TORCH_CHECK(col.numel() == (kind == JSEL_PROBE ? np : nb),
              "predicate column length does not match its side");
  p->ptr[s] = reinterpret_cast<unsigned long long>(col.data_ptr());
  p->is_f64[s] = col.scalar_type() == at::kDouble ? 1 : 0;
}
}  // namespace

// Inner join against unique build keys with an optional residual
// comparison and a projection, one kernel (join.hip).  heads/next: the
// chained table of join_build over build_keys.  pred: None, or
// (op, lhs, rhs) with op 0 == 1 != 2 < 3 <= 4 > 5 >= and operands as
// jsel_operand takes them.  out_specs: up to COMPACT_MAX_COLS pairs
// (side, column) of 8-byte columns, side 0 probe / 1 build.  Returns the
// output columns at probe length (capacity mode) followed by the cursor
// [1]: the caller narrows to its value.  Row order is not defined.  An
// empty probe or build side returns empty columns without a launch.
// block_rows forces the probe rows per block (tests); 0 is by probe length.
std::vector<at::Tensor> join_unique_select(
    at::Tensor pkeys, at::Tensor bkeys, at::Tensor heads, at::Tensor next,
    py::object pred, std::vector<std::pair<int64_t, at::Tensor>> out_specs,
    int64_t block_rows) {
  TORCH_CHECK(block_rows == 0 || block_rows == 1024 || block_rows == 2048 ||
                  block_rows == COMPACT_CHUNK,
              "block_rows is 0 (by probe length), 1024, 2048 or ",
              COMPACT_CHUNK);
  check_gpu(pkeys, "probe_keys");
  check_gpu(bkeys, "build_keys");
  check_gpu(heads, "heads");
  check_gpu(next, "next");
  TORCH_CHECK(pkeys.scalar_type() == at::kLong &&
                  bkeys.scalar_type() == at::kLong,
              "join keys must be int64");
  TORCH_CHECK(heads.scalar_type() == at::kInt &&
                  next.scalar_type() == at::kInt,
              "heads/next must be int32");
  TORCH_CHECK(out_specs.size() >= 1 && out_specs.size() <= COMPACT_MAX_COLS,
              "1..", COMPACT_MAX_COLS, " output columns");
  int64_t np = pkeys.numel(), nb = bkeys.numel();
  int64_t tsize = heads.numel();
  TORCH_CHECK(tsize > 0 && (tsize & (tsize - 1)) == 0,
              "heads length must be a power of 2");
  TORCH_CHECK(next.numel() >= nb, "next is shorter than the build side");
  TORCH_CHECK(nb <= std::numeric_limits<int32_t>::max(),
              "build side too long for int32 chain links");
  bool empty = np == 0 || nb == 0;
  JoinSelPred p;
  std::memset(&p, 0, sizeof(p));
  p.op = -1;
  if (!pred.is_none()) {
    auto t = py::cast<py::tuple>(pred);
    TORCH_CHECK(t.size() == 3, "pred is (op, lhs, rhs)");
    p.op = py::cast<int>(t[0]);
    TORCH_CHECK(p.op >= 0 && p.op <= 5, "comparison op code 0..5");
    jsel_operand(t[1], 0, np, nb, &p);
    jsel_operand(t[2], 1, np, nb, &p);
    p.use_int = (!p.is_f64[0] && !p.is_f64[1]) ? 1 : 0;
  }
  JoinSelCols c;
  std::memset(&c, 0, sizeof(c));
  c.ncols = (int)out_specs.size();
  std::vector<at::Tensor> outs;
  for (size_t i = 0; i < out_specs.size(); ++i) {
    int64_t side = out_specs[i].first;
    const at::Tensor& col = out_specs[i].second;
    TORCH_CHECK(side == JSEL_PROBE || side == JSEL_BUILD, "column side");
    check_gpu(col, "output column");
    TORCH_CHECK(col.element_size() == 8, "8-byte columns only");
    TORCH_CHECK(col.numel() == (side == JSEL_PROBE ? np : nb),
                "output column length does not match its side");
    auto out = at::empty({empty ? 0 : np}, col.options());
    c.side[i] = (int)side;
    c.src[i] = reinterpret_cast<unsigned long long>(col.data_ptr());
    c.dst[i] = reinterpret_cast<unsigned long long>(out.data_ptr());
    outs.push_back(out);
  }
  auto cursor = at::zeros({1}, pkeys.options());
  if (!empty) {
    launch_join_unique_select(
        pkeys.data_ptr<int64_t>(), np, bkeys.data_ptr<int64_t>(),
        heads.data_ptr<int32_t>(), next.data_ptr<int32_t>(), tsize, &p, &c,
        cursor.data_ptr<int64_t>(), (int)block_rows, current_stream());
  }
  outs.push_back(cursor);
  return outs;
}

at::Tensor join_count(at::Tensor pkeys, at::Tensor bkeys,
                      c10::optional<at::Tensor> ph2,
                      c10::optional<at::Tensor> bh2, at::Tensor heads,
                      at::Tensor next, int64_t tsize) {
  check_gpu(pkeys, "pkeys");
  int64_t np = pkeys.numel();
  auto counts = at::zeros({np}, pkeys.options().dtype(at::kInt));
  if (np > 0) {
    launch_join_count(pkeys.data_ptr<int64_t>(), np,
                      bkeys.data_ptr<int64_t>(), opt_i64_ptr(ph2),
                      opt_i64_ptr(bh2), heads.data_ptr<int32_t>(),
                      next.data_ptr<int32_t>(), tsize,
                      counts.data_ptr<int32_t>(), current_stream());
  }
  return counts;
}

std::vector<at::Tensor> join_pairs(at::Tensor pkeys, at::Tensor bkeys,
                                   c10::optional<at::Tensor> ph2,
                                   c10::optional<at::Tensor> bh2,
                                   at::Tensor heads, at::Tensor next,
                                   int64_t tsize, int64_t mode) {
  // one-scalar total + chunked single-reservation emit (no per-row
  // counts array / prefix sum)
  check_gpu(pkeys, "pkeys");
  int64_t np = pkeys.numel();
  auto stream = current_stream();
  auto total_t = at::zeros({1}, pkeys.options());
  if (np > 0) {
    launch_join_total(pkeys.data_ptr<int64_t>(), np,
                      bkeys.data_ptr<int64_t>(), opt_i64_ptr(ph2),
                      opt_i64_ptr(bh2), heads.data_ptr<int32_t>(),
                      next.data_ptr<int32_t>(), tsize, (int)mode,
                      total_t.data_ptr<int64_t>(), stream);
  }
  int64_t out_n = total_t.cpu().item<int64_t>();
  auto out_p = at::empty({out_n}, pkeys.options());
  auto out_b = at::empty({out_n}, pkeys.options());
  if (np > 0 && out_n > 0) {
    auto cursor = at::zeros({1}, pkeys.options());
    launch_join_emit_chunked(
        pkeys.data_ptr<int64_t>(), np, bkeys.data_ptr<int64_t>(),
        opt_i64_ptr(ph2), opt_i64_ptr(bh2), heads.data_ptr<int32_t>(),
        next.data_ptr<int32_t>(), tsize, cursor.data_ptr<int64_t>(),
        out_p.data_ptr<int64_t>(), out_b.data_ptr<int64_t>(), (int)mode,
        stream);
  }
  return {out_p, out_b};
}

std::vector<at::Tensor> join_emit(at::Tensor pkeys, at::Tensor bkeys,
                                  c10::optional<at::Tensor> ph2,
                                  c10::optional<at::Tensor> bh2,
                                  at::Tensor heads, at::Tensor next,
                                  int64_t tsize, at::Tensor offsets,
                                  int64_t out_n, int64_t mode) {
  check_gpu(pkeys, "pkeys");
  int64_t np = pkeys.numel();
  auto out_p = at::empty({out_n}, pkeys.options());
  auto out_b = at::empty({out_n}, pkeys.options());
  if (np > 0 && out_n > 0) {
    launch_join_emit(pkeys.data_ptr<int64_t>(), np, bkeys.data_ptr<int64_t>(),
                     opt_i64_ptr(ph2), opt_i64_ptr(bh2),
                     heads.data_ptr<int32_t>(), next.data_ptr<int32_t>(),
                     tsize, offsets.data_ptr<int64_t>(),
                     out_p.data_ptr<int64_t>(), out_b.data_ptr<int64_t>(),
                     (int)mode, current_stream());
  }
  return {out_p, out_b};
}

at::Tensor join_mark_build(at::Tensor pkeys, at::Tensor bkeys,
                           c10::optional<at::Tensor> ph2,
                           c10::optional<at::Tensor> bh2, at::Tensor heads,
                           at::Tensor next, int64_t tsize, int64_t n_build) {
  check_gpu(pkeys, "pkeys");
  auto matched = at::zeros({n_build}, pkeys.options().dtype(at::kBool));
  if (pkeys.numel() > 0 && n_build > 0) {
    launch_join_mark_build(pkeys.data_ptr<int64_t>(), pkeys.numel(),
                           bkeys.data_ptr<int64_t>(), opt_i64_ptr(ph2),
                           opt_i64_ptr(bh2), heads.data_ptr<int32_t>(),
                           next.data_ptr<int32_t>(), tsize,
                           matched.data_ptr<bool>(), current_stream());
  }
  return matched;
}

void hash_string_column(at::Tensor offsets, at::Tensor bytes,
                        c10::optional<at::Tensor> valid, at::Tensor out,
                        bool is_first) {
  check_gpu(offsets, "offsets");
  check_gpu(out, "out");
  int64_t n = out.numel();
  launch_hash_string_col(
      offsets.data_ptr<int64_t>(), bytes.data_ptr<uint8_t>(),
      opt_valid_ptr(valid),
      reinterpret_cast<uint64_t*>(out.data_ptr<int64_t>()), n, is_first,
      current_stream());
}

void hash_seed(at::Tensor out, int64_t seed) {
  check_gpu(out, "out");
  launch_hash_seed(reinterpret_cast<uint64_t*>(out.data_ptr<int64_t>()),
                   out.numel(), (uint64_t)seed, current_stream());
}

std::vector<at::Tensor> gb_mark_reps(at::Tensor h1, at::Tensor h2,
                                     at::Tensor tkeys, int64_t tsize) {
  check_gpu(h1, "h1");
  auto rep = at::full({tsize}, -1, h1.options());
  auto th2 = at::full({tsize}, (int64_t)GB_EMPTY, h1.options());
  auto conflict = at::zeros({1}, h1.options());
  if (h1.numel() > 0) {
    launch_gb_mark_reps(h1.data_ptr<int64_t>(), h2.data_ptr<int64_t>(),
                        tkeys.data_ptr<int64_t>(), tsize,
                        rep.data_ptr<int64_t>(), th2.data_ptr<int64_t>(),
                        conflict.data_ptr<int64_t>(), h1.numel(),
                        current_stream());
  }
  return {rep, th2, conflict};
}

// Compact up to 8 eight-byte columns by mask in one pass.
// Returns the output tensors (sized by mask.sum(), computed on device
// and read back once).
std::vector<at::Tensor> compact_columns(at::Tensor mask,
                                        std::vector<at::Tensor> cols,
                                        int64_t out_n) {
  check_gpu(mask, "mask");
  TORCH_CHECK(cols.size() >= 1 && cols.size() <= 8, "1..8 columns");
  int64_t n = mask.numel();
  auto cursor = at::zeros({1}, mask.options().dtype(at::kLong));
  const uint64_t* srcs[8];
  uint64_t* dsts[8];
  std::vector<at::Tensor> outs;
  for (size_t c = 0; c < cols.size(); ++c) {
    check_gpu(cols[c], "col");
    TORCH_CHECK(cols[c].element_size() == 8, "8-byte columns only");
    auto out = at::empty({out_n}, cols[c].options());
    srcs[c] = reinterpret_cast<const uint64_t*>(cols[c].data_ptr());
    dsts[c] = reinterpret_cast<uint64_t*>(out.data_ptr());
    outs.push_back(out);
  }
  launch_compact8(mask.data_ptr<bool>(), n, cursor.data_ptr<int64_t>(),
                  srcs, dsts, (int)cols.size(), current_stream());
  return outs;
}

// Capacity-mode compaction: outputs are allocated at mask length and the
// caller narrows using the returned cursor (total) — skips the separate
// mask.sum() reduction + its host sync (profiles/NOTES.md r02).
std::vector<at::Tensor> compact_columns_cap(
    at::Tensor mask, std::vector<c10::optional<at::Tensor>> cols) {
  check_gpu(mask, "mask");
  TORCH_CHECK(cols.size() >= 1 && cols.size() <= 8, "1..8 columns");
  int64_t n = mask.numel();
  auto cursor = at::zeros({1}, mask.options().dtype(at::kLong));
  const uint64_t* srcs[8];
  uint64_t* dsts[8];
  std::vector<at::Tensor> outs;
  for (size_t c = 0; c < cols.size(); ++c) {
    at::Tensor out;
    if (cols[c].has_value()) {  // nullopt -> emit the row index
      check_gpu(*cols[c], "col");
      TORCH_CHECK(cols[c]->element_size() == 8, "8-byte columns only");
      srcs[c] = reinterpret_cast<const uint64_t*>(cols[c]->data_ptr());
      out = at::empty({n}, cols[c]->options());
    } else {
      srcs[c] = nullptr;
      out = at::empty({n}, mask.options().dtype(at::kLong));
    }
    dsts[c] = reinterpret_cast<uint64_t*>(out.data_ptr());
    outs.push_back(out);
  }
  launch_compact8(mask.data_ptr<bool>(), n, cursor.data_ptr<int64_t>(),
                  srcs, dsts, (int)cols.size(), current_stream());
  outs.push_back(cursor);
  return outs;
}


namespace {
int cmp_dtype_code(const at::Tensor& t) {
  switch (t.scalar_type()) {
    case at::kLong: return 0;
    case at::kInt: return 1;
    case at::kShort: return 2;
    case at::kDouble: return 3;
    case at::kFloat: return 4;
    default: TORCH_CHECK(false, "unsupported compare dtype"); return -1;
  }
}
}  // namespace




// Open-addressed unique join for int64 keys (no h2): one 16B (key,idx)
// entry per slot — ~1 random cache line per probe vs ~3 for the
// chained layout.  flags = [dup_build_key, sentinel_key_seen]; either
// nonzero means the caller must fall back to the chained join.
std::vector<at::Tensor> join_open_unique(at::Tensor pkeys, at::Tensor bkeys,
                                         bool want_pi, bool want_mask,
                                         bool mask_neg) {
  check_gpu(pkeys, "pkeys");
  check_gpu(bkeys, "bkeys");
  int64_t np = pkeys.numel();
  int64_t nb = bkeys.numel();
  int64_t tsize = 16;
  while (tsize < nb * 2) tsize <<= 1;
  auto table = at::empty({2 * tsize}, bkeys.options());
  auto flags = at::zeros({2}, bkeys.options());
  launch_joinoa_build(nb > 0 ? bkeys.data_ptr<int64_t>() : nullptr, nb,
                      table.data_ptr<int64_t>(), tsize,
                      flags.data_ptr<int64_t>(), current_stream());
  auto out_pi = at::empty({want_pi ? np : 0}, pkeys.options());
  auto out_bi = at::empty({np}, pkeys.options());
  auto out_mask =
      at::empty({want_mask ? np : 0}, pkeys.options().dtype(at::kBool));
  if (np > 0) {
    launch_joinoa_probe(
        pkeys.data_ptr<int64_t>(), np, table.data_ptr<int64_t>(), tsize,
        want_pi ? out_pi.data_ptr<int64_t>() : nullptr,
        out_bi.data_ptr<int64_t>(),
        want_mask ? out_mask.data_ptr<bool>() : nullptr, mask_neg ? 1 : 0,
        current_stream());
  }
  return {out_pi, out_bi, out_mask, flags};
}

// Own top-k select for k <= 16 (see select.hip); returns
// (values[k], indices[k]) sorted, index-tiebroken (deterministic).
std::vector<at::Tensor> topk_select(at::Tensor vals, int64_t k,
                                    bool largest) {
  check_gpu(vals, "vals");
  // checked before k narrows to the launcher's int
  TORCH_CHECK(k >= 1 && k <= TOPK_MAX, "k must be in [1, ", TOPK_MAX, "]");
  int dt;
  if (vals.scalar_type() == at::kLong) {
    dt = 0;
  } else if (vals.scalar_type() == at::kDouble) {
    dt = 1;
  } else {
    TORCH_CHECK(false, "topk_select supports int64/float64");
  }
  int64_t n = vals.numel();
  TORCH_CHECK(n >= 1, "empty input");
  auto cand_v = at::empty({TOPK_BLOCKS * k}, vals.options());
  auto cand_i = at::empty({TOPK_BLOCKS * k}, vals.options().dtype(at::kLong));
  auto out_v = at::empty({k}, vals.options());
  auto out_i = at::empty({k}, vals.options().dtype(at::kLong));
  launch_topk(vals.data_ptr(), dt, largest ? 1 : 0, n, (int)k,
              cand_v.data_ptr(), cand_i.data_ptr<int64_t>(),
              out_v.data_ptr(), out_i.data_ptr<int64_t>(),
              current_stream());
  return {out_v, out_i};
}

at::Tensor eq2_mask(at::Tensor h1, at::Tensor h2, at::Tensor l1,
                    at::Tensor l2, c10::optional<at::Tensor> valid,
                    bool neg) {
  check_gpu(h1, "h1");
  check_gpu(h2, "h2");
  auto out = at::empty({h1.numel()}, h1.options().dtype(at::kBool));
  launch_eq2_mask(h1.data_ptr<int64_t>(), h2.data_ptr<int64_t>(),
                  l1.data_ptr<int64_t>(), l2.data_ptr<int64_t>(),
                  opt_valid_ptr(valid), neg ? 1 : 0, h1.numel(),
                  out.data_ptr<bool>(), current_stream());
  return out;
}

// Fast path for single-comparison WHERE filters (see select.hip).
at::Tensor cmp_imm(at::Tensor a, c10::optional<at::Tensor> valid,
                   int64_t imm_i, double imm_d, bool use_int, int64_t op) {
  check_gpu(a, "a");
  int dt = cmp_dtype_code(a);
  bool ui = use_int && dt <= 2;
  auto out = at::empty({a.numel()}, a.options().dtype(at::kBool));
  launch_cmp_imm(a.data_ptr(), opt_valid_ptr(valid), dt, imm_i, imm_d,
                 ui ? 1 : 0, (int)op, a.numel(), out.data_ptr<bool>(),
                 current_stream());
  return out;
}

at::Tensor cmp_col(at::Tensor a, c10::optional<at::Tensor> va, at::Tensor b,
                   c10::optional<at::Tensor> vb, int64_t op) {
  check_gpu(a, "a");
  check_gpu(b, "b");
  TORCH_CHECK(a.scalar_type() == b.scalar_type(), "same dtype required");
  int dt = cmp_dtype_code(a);
  auto out = at::empty({a.numel()}, a.options().dtype(at::kBool));
  launch_cmp_col(a.data_ptr(), opt_valid_ptr(va), b.data_ptr(),
                 opt_valid_ptr(vb), dt, (int)op, a.numel(),
                 out.data_ptr<bool>(), current_stream());
  return out;
}

static ExprProg build_expr_prog(at::Tensor& ops, at::Tensor& aux,
                                at::Tensor& imm,
                                std::vector<at::Tensor>& col_data,
                                std::vector<at::Tensor>& col_valid,
                                at::Tensor& col_dt) {
  TORCH_CHECK(ops.numel() <= EXPR_MAX_OPS, "program too long");
  TORCH_CHECK(col_data.size() <= EXPR_MAX_COLS, "too many columns");
  TORCH_CHECK(imm.numel() <= EXPR_MAX_COLS, "too many immediates");
  ExprProg prog;
  std::memset(&prog, 0, sizeof(prog));
  prog.n_ops = (int)ops.numel();
  auto ops_c = ops.to(at::kByte).cpu();
  auto aux_c = aux.to(at::kChar).cpu();
  auto imm_c = imm.cpu();
  auto dt_c = col_dt.to(at::kByte).cpu();
  for (int i = 0; i < prog.n_ops; ++i) {
    prog.op[i] = ops_c[i].item<uint8_t>();
    prog.aux[i] = aux_c[i].item<int8_t>();
  }
  for (int i = 0; i < (int)imm_c.numel(); ++i) {
    prog.imm[i] = (unsigned long long)imm_c[i].item<int64_t>();
  }
  for (size_t c = 0; c < col_data.size(); ++c) {
    check_gpu(col_data[c], "col");
    TORCH_CHECK(col_data[c].is_contiguous(), "columns must be contiguous");
    prog.col_data[c] = reinterpret_cast<unsigned long long>(
        col_data[c].data_ptr());
    prog.col_dt[c] = dt_c[c].item<uint8_t>();
    if (col_valid[c].defined() && col_valid[c].numel() > 0) {
      check_gpu(col_valid[c], "valid");
      prog.col_valid[c] = reinterpret_cast<unsigned long long>(
          col_valid[c].data_ptr());
    }
  }
  return prog;
}

std::vector<at::Tensor> expr_value(at::Tensor ops, at::Tensor aux,
                                   at::Tensor imm,
                                   std::vector<at::Tensor> col_data,
                                   std::vector<at::Tensor> col_valid,
                                   at::Tensor col_dt, int64_t n,
                                   int64_t out_int) {
  TORCH_CHECK(col_data.size() >= 1, "needs at least one column");
  auto prog = build_expr_prog(ops, aux, imm, col_data, col_valid, col_dt);
  auto opts = col_data[0].options();
  auto out = at::empty({n}, opts.dtype(out_int ? at::kLong : at::kDouble));
  auto valid = at::empty({n}, opts.dtype(at::kBool));
  if (n > 0) {
    launch_expr_value(&prog, n, (int)out_int, out.data_ptr(),
                      valid.data_ptr<bool>(), current_stream());
  }
  return {out, valid};
}

at::Tensor expr_filter(at::Tensor ops, at::Tensor aux, at::Tensor imm,
                       std::vector<at::Tensor> col_data,
                       std::vector<at::Tensor> col_valid,
                       at::Tensor col_dt, int64_t n) {
  TORCH_CHECK(col_data.size() >= 1, "needs at least one column");
  auto prog = build_expr_prog(ops, aux, imm, col_data, col_valid, col_dt);
  auto out = at::empty({n}, col_data[0].options().dtype(at::kBool));
  if (n > 0) {
    launch_expr_filter(&prog, n, out.data_ptr<bool>(), current_stream());
  }
  return out;
}

std::vector<at::Tensor> gather_columns(at::Tensor idx,
                                       std::vector<at::Tensor> cols) {
  check_gpu(idx, "idx");
  TORCH_CHECK(cols.size() >= 1 && cols.size() <= GATHER_MAX_COLS, "1..",
              GATHER_MAX_COLS, " columns");
  int64_t n = idx.numel();
  // group by element width: one fused launch per width class
  std::vector<at::Tensor> outs(cols.size());
  for (int width : {8, 4, 2, 1}) {
    uint64_t srcs[GATHER_MAX_COLS];
    uint64_t dsts[GATHER_MAX_COLS];
    int k = 0;
    for (size_t c = 0; c < cols.size(); ++c) {
      if (cols[c].element_size() != width) continue;
      check_gpu(cols[c], "col");
      TORCH_CHECK(cols[c].is_contiguous(), "columns must be contiguous");
      auto out = at::empty({n}, cols[c].options());
      srcs[k] = reinterpret_cast<uint64_t>(cols[c].data_ptr());
      dsts[k] = reinterpret_cast<uint64_t>(out.data_ptr());
      outs[c] = out;
      ++k;
    }
    if (k > 0 && n > 0) {
      launch_gather_cols(srcs, dsts, k, width, idx.data_ptr<int64_t>(), n,
                         current_stream());
    } else if (k > 0) {
      // n == 0: outputs already sized 0
    }
  }
  return outs;
}

std::vector<at::Tensor> reduce_columns(at::Tensor vals,
                                       c10::optional<at::Tensor> valids,
                                       at::Tensor ops) {
  check_gpu(vals, "vals");
  int n_aggs = (int)vals.size(0);
  int64_t n = vals.size(1);
  auto out = at::zeros({n_aggs}, vals.options());
  auto ops_cpu = ops.cpu();
  for (int a = 0; a < n_aggs; ++a) {
    int op = (int)ops_cpu[a].item<int32_t>();
    if (op == 1) out[a] = std::numeric_limits<double>::infinity();
    if (op == 2) out[a] = -std::numeric_limits<double>::infinity();
  }
  auto cnt = at::zeros({n_aggs}, vals.options().dtype(at::kLong));
  const bool* vptr = nullptr;
  if (valids.has_value()) {
    vptr = valids.value().data_ptr<bool>();
  }
  if (n > 0) {
    launch_reduce_cols(vals.data_ptr<double>(), vptr,
                       ops.data_ptr<int32_t>(), n_aggs, n,
                       out.data_ptr<double>(), cnt.data_ptr<int64_t>(),
                       current_stream());
  }
  return {out, cnt};
}


// ---- fused group-by key preparation --------------------------------- //

// One launch set + ONE host readback for everything the group-by sizing
// needs: per-column min/max (2*ncols leading slots, signed order
// preserved via the s2u bias) and the sampled distinct estimate
// (d, f1, f2 in the last 3 slots).  Replaces per-column
// min().item()/max().item() and the torch.unique Chao83 sampling
// (profiles/NOTES.md r02 host-sync findings).
at::Tensor gb_key_stats(std::vector<at::Tensor> cols,
                        std::vector<c10::optional<at::Tensor>> valids,
                        int64_t nsamples, int64_t tsize, bool do_minmax) {
  int k = (int)cols.size();
  TORCH_CHECK(k >= 1 && k <= PACK_MAX_COLS, "1..", PACK_MAX_COLS,
              " key columns");
  TORCH_CHECK((tsize & (tsize - 1)) == 0, "tsize must be a power of 2");
  int64_t n = cols[0].numel();
  const void* data[PACK_MAX_COLS];
  const bool* valid[PACK_MAX_COLS];
  int dwidth[PACK_MAX_COLS];
  for (int c = 0; c < k; ++c) {
    check_gpu(cols[c], "key col");
    int es = (int)cols[c].element_size();
    TORCH_CHECK(es == 8 || es == 4 || es == 2, "2/4/8-byte key columns");
    data[c] = cols[c].data_ptr();
    valid[c] = opt_valid_ptr(valids[c]);
    dwidth[c] = es;
  }
  auto out = at::empty({2 * k + 3}, cols[0].options().dtype(at::kLong));
  auto slots = at::empty({tsize}, cols[0].options().dtype(at::kLong));
  auto counts = at::empty({tsize}, cols[0].options().dtype(at::kInt));
  launch_gb_key_stats(data, valid, dwidth, k, n, nsamples,
                      slots.data_ptr<int64_t>(), counts.data_ptr<int32_t>(),
                      (int)tsize, do_minmax ? 1 : 0,
                      reinterpret_cast<uint64_t*>(out.data_ptr<int64_t>()),
                      current_stream());
  return out;
}

// Pack up to 8 integer key columns into one int64 group key in a single
// pass (code 0 = NULL; valid values offset by 1 from the column min).
at::Tensor pack_columns(std::vector<at::Tensor> cols,
                        std::vector<c10::optional<at::Tensor>> valids,
                        std::vector<int64_t> mins,
                        std::vector<int64_t> shifts) {
  int k = (int)cols.size();
  TORCH_CHECK(k >= 1 && k <= PACK_MAX_COLS, "1..", PACK_MAX_COLS,
              " key columns");
  int64_t n = cols[0].numel();
  const void* data[PACK_MAX_COLS];
  const bool* valid[PACK_MAX_COLS];
  int dwidth[PACK_MAX_COLS];
  int shift_i[PACK_MAX_COLS];
  for (int c = 0; c < k; ++c) {
    check_gpu(cols[c], "key col");
    int es = (int)cols[c].element_size();
    TORCH_CHECK(es == 8 || es == 4 || es == 2, "2/4/8-byte key columns");
    data[c] = cols[c].data_ptr();
    valid[c] = opt_valid_ptr(valids[c]);
    dwidth[c] = es;
    shift_i[c] = (int)shifts[c];
  }
  auto out = at::empty({n}, cols[0].options().dtype(at::kLong));
  launch_pack_cols(data, valid, dwidth, mins.data(), shift_i, k, n,
                   out.data_ptr<int64_t>(), current_stream());
  return out;
}

// Unpack one column from packed group keys; returns (data, valid) where
// valid is an empty tensor when the source column had no nulls.
std::vector<at::Tensor> unpack_column(at::Tensor packed, int64_t shift,
                                      int64_t width, int64_t lo,
                                      int64_t dwidth, bool has_nulls) {
  check_gpu(packed, "packed");
  int64_t n = packed.numel();
  auto dt = dwidth == 8 ? at::kLong : (dwidth == 4 ? at::kInt : at::kShort);
  auto out = at::empty({n}, packed.options().dtype(dt));
  at::Tensor valid;
  if (has_nulls) {
    valid = at::empty({n}, packed.options().dtype(at::kBool));
  } else {
    valid = at::empty({0}, packed.options().dtype(at::kBool));
  }
  int64_t mask = width >= 64 ? -1 : ((int64_t(1) << width) - 1);
  launch_unpack_col(packed.data_ptr<int64_t>(), n, (int)shift, mask, lo,
                    (int)dwidth, has_nulls ? 1 : 0, out.data_ptr(),
                    has_nulls ? valid.data_ptr<bool>() : nullptr,
                    current_stream());
  return {out, valid};
}

// Deterministic compaction of the group hash table: drops EMPTY slots
// from tkeys/gcount/gaggs in slot order.  Returns capacity-sized outputs
// plus the block-base scan whose last element is the total (single host
// read; caller narrows).
std::vector<at::Tensor> gb_compact(at::Tensor tkeys, at::Tensor gcount,
                                   at::Tensor gaggs,
                                   c10::optional<at::Tensor> extra) {
  check_gpu(tkeys, "tkeys");
  check_gpu(gcount, "gcount");
  int64_t tsize = tkeys.numel();
  int n_aggs = gaggs.numel() > 0 ? (int)gaggs.size(0) : 0;
  TORCH_CHECK(n_aggs <= GBC_MAX_AGGS, "at most ", GBC_MAX_AGGS,
              " aggregate columns");
  int64_t nblocks = (tsize + GBC_CHUNK - 1) / GBC_CHUNK;
  auto bcounts = at::empty({nblocks}, tkeys.options());
  auto bases = at::empty({nblocks + 1}, tkeys.options());
  auto out_keys = at::empty({tsize}, tkeys.options());
  auto out_count = at::empty({tsize}, gcount.options());
  at::Tensor out_aggs = at::empty({n_aggs, tsize}, gaggs.options());
  const double* asrc[GBC_MAX_AGGS];
  double* adst[GBC_MAX_AGGS];
  for (int a = 0; a < n_aggs; ++a) {
    asrc[a] = gaggs[a].data_ptr<double>();
    adst[a] = out_aggs[a].data_ptr<double>();
  }
  at::Tensor out_extra;
  const int64_t* esrc = nullptr;
  int64_t* edst = nullptr;
  if (extra.has_value()) {
    check_gpu(*extra, "extra");
    out_extra = at::empty({tsize}, extra->options());
    esrc = extra->data_ptr<int64_t>();
    edst = out_extra.data_ptr<int64_t>();
  } else {
    out_extra = at::empty({0}, tkeys.options());
  }
  launch_gb_compact(tkeys.data_ptr<int64_t>(), gcount.data_ptr<int64_t>(),
                    asrc, adst, n_aggs, tsize, bcounts.data_ptr<int64_t>(),
                    bases.data_ptr<int64_t>(), out_keys.data_ptr<int64_t>(),
                    out_count.data_ptr<int64_t>(), esrc, edst,
                    current_stream());
  return {out_keys, out_count, out_aggs, out_extra, bases};
}

// Segmented rank over a sorted permutation, window mode: the rank of each
// row lands at its ORIGINAL row position.  kind 0 row_number, 1 rank,
// 2 dense_rank.  Order columns are 8-byte (int64 bits or float64) in
// original row order, each with an optional bool validity tensor.
int64_t seg_rank_chunk() { return SEG_CHUNK; }

static void seg_check_inputs(const at::Tensor& perm, const at::Tensor& pkeys) {
  check_gpu(perm, "perm");
  check_gpu(pkeys, "pkeys");
  TORCH_CHECK(perm.scalar_type() == at::kLong && perm.is_contiguous(),
              "perm must be contiguous int64");
  TORCH_CHECK(pkeys.scalar_type() == at::kLong && pkeys.is_contiguous(),
              "pkeys must be contiguous int64");
  TORCH_CHECK(perm.numel() == pkeys.numel(), "perm/pkeys length mismatch");
}

at::Tensor seg_rank(at::Tensor perm, at::Tensor pkeys,
                    std::vector<at::Tensor> col_data,
                    std::vector<c10::optional<at::Tensor>> col_valid,
                    int64_t kind) {
  seg_check_inputs(perm, pkeys);
  int64_t n = perm.numel();
  int ncols = (int)col_data.size();
  TORCH_CHECK(ncols <= SEG_MAX_COLS, "at most ", SEG_MAX_COLS,
              " order columns");
  TORCH_CHECK(col_valid.size() == col_data.size(), "col_valid size mismatch");
  TORCH_CHECK(kind >= 0 && kind <= 2, "kind must be 0, 1 or 2");
  const int64_t* cd[SEG_MAX_COLS] = {};
  const uint8_t* cv[SEG_MAX_COLS] = {};
  int cf[SEG_MAX_COLS] = {};
  for (int c = 0; c < ncols; ++c) {
    check_gpu(col_data[c], "order column");
    TORCH_CHECK(col_data[c].is_contiguous() && col_data[c].numel() == n &&
                    col_data[c].element_size() == 8,
                "order columns must be contiguous 8-byte tensors of length n");
    cf[c] = col_data[c].is_floating_point() ? 1 : 0;
    cd[c] = reinterpret_cast<const int64_t*>(col_data[c].data_ptr());
    if (col_valid[c].has_value()) {
      const at::Tensor& v = *col_valid[c];
      check_gpu(v, "order validity");
      TORCH_CHECK(v.scalar_type() == at::kBool && v.is_contiguous() &&
                      v.numel() == n,
                  "validity must be contiguous bool of length n");
      cv[c] = reinterpret_cast<const uint8_t*>(v.data_ptr());
    }
  }
  auto out = at::empty({n}, perm.options());
  if (n == 0) return out;
  int64_t nblocks = (n + SEG_CHUNK - 1) / SEG_CHUNK;
  auto work = at::empty({6 * nblocks}, perm.options());
  launch_seg_rank(perm.data_ptr<int64_t>(), pkeys.data_ptr<int64_t>(), cd, cv,
                  cf, ncols, n, (int)kind, work.data_ptr<int64_t>(),
                  out.data_ptr<int64_t>(), current_stream());
  return out;
}

// Take mode: the first n_take sorted positions of every segment, emitted
// as a capacity-n index vector in sorted order plus the block-base scan
// whose last element is the total (single host read; caller narrows).
std::vector<at::Tensor> seg_take(at::Tensor perm, at::Tensor pkeys,
                                 int64_t n_take) {
  seg_check_inputs(perm, pkeys);
  int64_t n = perm.numel();
  int64_t nblocks = (n + SEG_CHUNK - 1) / SEG_CHUNK;
  auto out = at::empty({n}, perm.options());
  if (n == 0) return {out, at::zeros({1}, perm.options())};
  auto work = at::empty({6 * nblocks}, perm.options());
  auto bcounts = at::empty({nblocks}, perm.options());
  auto bases = at::empty({nblocks + 1}, perm.options());
  launch_seg_take(perm.data_ptr<int64_t>(), pkeys.data_ptr<int64_t>(), n,
                  n_take, work.data_ptr<int64_t>(),
                  bcounts.data_ptr<int64_t>(), bases.data_ptr<int64_t>(),
                  out.data_ptr<int64_t>(), current_stream());
  return {out, bases};
}

// One 8-byte value column of a value window (int64 bits or float64, in
// original row order) and its optional bool validity.
static const uint8_t* seg_check_value(const at::Tensor& data,
                                      const c10::optional<at::Tensor>& valid,
                                      int64_t n) {
  check_gpu(data, "value column");
  TORCH_CHECK(data.is_contiguous() && data.numel() == n &&
                  data.element_size() == 8 &&
                  (data.scalar_type() == at::kLong ||
                   data.scalar_type() == at::kDouble),
              "value column must be contiguous int64/float64 of length n");
  if (!valid.has_value()) return nullptr;
  const at::Tensor& v = *valid;
  check_gpu(v, "value validity");
  TORCH_CHECK(v.scalar_type() == at::kBool && v.is_contiguous() &&
                  v.numel() == n,
              "validity must be contiguous bool of length n");
  return reinterpret_cast<const uint8_t*>(v.data_ptr());
}

// LAG/LEAD: row i takes the value `offset` sorted positions back (ahead
// when negative) if that row is in its partition.  Returns (data, valid)
// in original row order; data keeps the input dtype.
std::vector<at::Tensor> seg_shift(at::Tensor perm, at::Tensor pkeys,
                                  at::Tensor data,
                                  c10::optional<at::Tensor> valid,
                                  int64_t offset) {
  seg_check_inputs(perm, pkeys);
  int64_t n = perm.numel();
  const uint8_t* vp = seg_check_value(data, valid, n);
  auto out = at::empty_like(data);
  auto out_valid = at::empty({n}, perm.options().dtype(at::kBool));
  launch_seg_shift(perm.data_ptr<int64_t>(), pkeys.data_ptr<int64_t>(),
                   reinterpret_cast<const int64_t*>(data.data_ptr()), vp, n,
                   offset, reinterpret_cast<int64_t*>(out.data_ptr()),
                   reinterpret_cast<uint8_t*>(out_valid.data_ptr()),
                   current_stream());
  return {out, out_valid};
}

// Running SUM (op 0) / MIN (1) / MAX (2) of the non-null values from the
// partition's first sorted position to each row, and their count.
// Returns (acc in the input dtype, cnt int64) in original row order.
std::vector<at::Tensor> seg_scan(at::Tensor perm, at::Tensor pkeys,
                                 at::Tensor data,
                                 c10::optional<at::Tensor> valid, int64_t op) {
  seg_check_inputs(perm, pkeys);
  int64_t n = perm.numel();
  const uint8_t* vp = seg_check_value(data, valid, n);
  TORCH_CHECK(op >= 0 && op <= 2, "op must be 0, 1 or 2");
  auto acc = at::empty_like(data);
  auto cnt = at::empty({n}, perm.options());
  if (n == 0) return {acc, cnt};
  int64_t nblocks = (n + SEG_CHUNK - 1) / SEG_CHUNK;
  auto work = at::empty({6 * nblocks}, perm.options());
  launch_seg_scan(perm.data_ptr<int64_t>(), pkeys.data_ptr<int64_t>(),
                  reinterpret_cast<const int64_t*>(data.data_ptr()), vp, n,
                  (int)op, data.is_floating_point() ? 1 : 0,
                  work.data_ptr<int64_t>(),
                  reinterpret_cast<int64_t*>(acc.data_ptr()),
                  cnt.data_ptr<int64_t>(), current_stream());
  return {acc, cnt};
}

// Whole-partition SUM (op 0) / MIN (1) / MAX (2) / FIRST (3) / LAST (4)
// of the non-null values, and their count, given to every row of the
// partition.  Returns (acc in the input dtype, cnt int64) in original
// row order.
std::vector<at::Tensor> seg_total(at::Tensor perm, at::Tensor pkeys,
                                  at::Tensor data,
                                  c10::optional<at::Tensor> valid,
                                  int64_t op) {
  seg_check_inputs(perm, pkeys);
  int64_t n = perm.numel();
  const uint8_t* vp = seg_check_value(data, valid, n);
  TORCH_CHECK(op >= 0 && op <= 4, "op must be 0..4");
  auto acc = at::empty_like(data);
  auto cnt = at::empty({n}, perm.options());
  if (n == 0) return {acc, cnt};
  auto work = at::empty({SEG_TOTAL_WORK(n)}, perm.options());
  launch_seg_total(perm.data_ptr<int64_t>(), pkeys.data_ptr<int64_t>(),
                   reinterpret_cast<const int64_t*>(data.data_ptr()), vp, n,
                   (int)op, data.is_floating_point() ? 1 : 0,
                   work.data_ptr<int64_t>(),
                   reinterpret_cast<int64_t*>(acc.data_ptr()),
                   cnt.data_ptr<int64_t>(), current_stream());
  return {acc, cnt};
}

int64_t seg_frame_tile() { return SEG_FRAME_TILE; }
int64_t seg_frame_max_reach() { return SEG_FRAME_MAX_REACH; }

// SUM (op 0) / MIN (1) / MAX (2) / FIRST (3) / LAST (4) of the non-null
// values in the frame [i + lo, i + hi] of every sorted position i,
// clipped to its partition, and their count.  Returns (acc in the input
// dtype, cnt int64) in original row order.  lo > hi is an empty frame.
std::vector<at::Tensor> seg_frame(at::Tensor perm, at::Tensor pkeys,
                                  at::Tensor data,
                                  c10::optional<at::Tensor> valid, int64_t op,
                                  int64_t lo, int64_t hi) {
  seg_check_inputs(perm, pkeys);
  int64_t n = perm.numel();
  const uint8_t* vp = seg_check_value(data, valid, n);
  TORCH_CHECK(op >= 0 && op <= 4, "op must be 0..4");
  lo = lo > n ? n : (lo < -n ? -n : lo);
  hi = hi > n ? n : (hi < -n ? -n : hi);
  TORCH_CHECK(lo > hi || (lo < 0 ? -lo : 0) + (hi > 0 ? hi : 0) <=
                             SEG_FRAME_MAX_REACH,
              "frame reach beyond ", SEG_FRAME_MAX_REACH);
  auto acc = at::empty_like(data);
  auto cnt = at::empty({n}, perm.options());
  if (n == 0) return {acc, cnt};
  launch_seg_frame(perm.data_ptr<int64_t>(), pkeys.data_ptr<int64_t>(),
                   reinterpret_cast<const int64_t*>(data.data_ptr()), vp, n,
                   lo, hi, (int)op, data.is_floating_point() ? 1 : 0,
                   reinterpret_cast<int64_t*>(acc.data_ptr()),
                   cnt.data_ptr<int64_t>(), current_stream());
  return {acc, cnt};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  // limits the python layer plans by (ops.py keeps copies for hosts
  // without the extension; a GPU test compares them)
  m.attr("PACK_MAX_COLS") = (int64_t)PACK_MAX_COLS;
  m.attr("GB_LDS_MAX_AGGS") = (int64_t)GB_LDS_MAX_AGGS;
  m.def("hash_column", &hash_column,
        "combine a column into the running row hash");
  m.def("bucket_of", &bucket_of, "hash -> bucket id");
  m.def("bucket_histogram", &bucket_histogram, "bucket histogram");
  m.def("bucket_scatter", &bucket_scatter,
        "scatter row indices into bucket-contiguous order");
  m.def("gb_aggregate", &gb_aggregate, "hash group-by aggregation",
        py::arg("keys"), py::arg("vals"), py::arg("valids"), py::arg("ops"),
        py::arg("tsize"), py::arg("use_lds"));
  m.def("gb_aggregate_replay", &gb_aggregate_replay,
        "re-aggregate with a recorded shuffle layout", py::arg("pkeys"),
        py::arg("pos"), py::arg("vals"), py::arg("ops"),
        py::arg("num_parts"), py::arg("tsize"), py::arg("agg_chunk"));
  m.def("gb_aggregate_partitioned", &gb_aggregate_partitioned,
        "partitioned (2-phase) hash group-by aggregation", py::arg("keys"),
        py::arg("vals"), py::arg("ops"), py::arg("num_parts"),
        py::arg("tsize"), py::arg("scatter_chunk"), py::arg("agg_chunk"),
        py::arg("narrow"), py::arg("record_layout"),
        py::arg("force_simple"), py::arg("record_chunk") = 0);
  m.def("dense_assign_max", []() { return (int64_t)DENSE_ASSIGN_MAX; },
        "largest per-partition distinct count the dense layout accepts");
  m.def("gb_dense_count", &gb_dense_count,
        "dense replay preparation: offsets + distinct keys per partition",
        py::arg("pkeys"), py::arg("num_parts"));
  m.def("gb_dense_assign", &gb_dense_assign,
        "dense replay preparation: group ids, output keys and counts",
        py::arg("pkeys"), py::arg("offsets"), py::arg("group_base"),
        py::arg("n_groups"));
  m.def("scatter_tile_prepare", &scatter_tile_prepare,
        "tile-coalesced scatter preparation (rank, dst) of a permutation");
  m.def("scatter_tile", &scatter_tile, "tile-coalesced value scatter");
  m.def("gb_dense_aggregate", &gb_dense_aggregate,
        "sum per dense group id (LDS table per chunk)", py::arg("gid"),
        py::arg("pvals"), py::arg("offsets"), py::arg("group_base"),
        py::arg("n_groups"), py::arg("chunk"), py::arg("slots"));
  m.def("gb_replay_dense", &gb_replay_dense,
        "replayed step: value scatter + dense aggregate", py::arg("vals"),
        py::arg("gid"), py::arg("offsets"), py::arg("group_base"),
        py::arg("n_groups"), py::arg("chunk"), py::arg("slots"),
        py::arg("tile") = 0, py::arg("rank") = py::none(),
        py::arg("dst") = py::none(), py::arg("pos") = py::none());
  m.def("scatter_tile_prepare_binned", &scatter_tile_prepare_binned,
        "tile scatter preparation into the binned layout: rank, dst, gid",
        py::arg("pos"), py::arg("gid"), py::arg("bin_offsets"),
        py::arg("tile"));
  m.def("gb_dense_aggregate_binned", &gb_dense_aggregate_binned,
        "sum per dense group id over the binned layout", py::arg("gid"),
        py::arg("pvals"), py::arg("bin_offsets"), py::arg("bin_group_base"),
        py::arg("bin_chunk_base"), py::arg("total_chunks"),
        py::arg("n_groups"), py::arg("chunk"), py::arg("slots"));
  m.def("gb_replay_binned", &gb_replay_binned,
        "replayed step over the binned layout: scatter + aggregate",
        py::arg("vals"), py::arg("gid"), py::arg("rank"), py::arg("dst"),
        py::arg("bin_offsets"), py::arg("bin_group_base"),
        py::arg("bin_chunk_base"), py::arg("total_chunks"),
        py::arg("n_groups"), py::arg("chunk"), py::arg("slots"),
        py::arg("tile"));
  m.def("scatter_tile_prepare_compact", &scatter_tile_prepare_compact,
        "compact binned preparation: rank, rel, tile_start, tile_delta",
        py::arg("pos"), py::arg("gid"), py::arg("bin_offsets"),
        py::arg("bin_group_base"), py::arg("tile"),
        py::arg("keep_gid") = false);
  m.def("scatter_tile_compact", &scatter_tile_compact,
        "tile-coalesced value scatter over the compact binned layout",
        py::arg("vals"), py::arg("rank"), py::arg("tile_start"),
        py::arg("tile_delta"), py::arg("tile"), py::arg("threads") = 0,
        py::arg("out") = py::none());
  m.def("gb_dense_aggregate_compact", &gb_dense_aggregate_compact,
        "sum per group over the binned layout, 16-bit ids", py::arg("rel"),
        py::arg("pvals"), py::arg("bin_offsets"), py::arg("bin_group_base"),
        py::arg("bin_chunk_base"), py::arg("total_chunks"),
        py::arg("n_groups"), py::arg("chunk"), py::arg("slots"),
        py::arg("out") = py::none());
  m.def("gb_replay_compact", &gb_replay_compact,
        "replayed step over the compact binned layout: scatter + aggregate",
        py::arg("vals"), py::arg("rel"), py::arg("rank"),
        py::arg("tile_start"), py::arg("tile_delta"), py::arg("bin_offsets"),
        py::arg("bin_group_base"), py::arg("bin_chunk_base"),
        py::arg("total_chunks"), py::arg("n_groups"), py::arg("chunk"),
        py::arg("slots"), py::arg("tile"), py::arg("threads") = 0);
  m.attr("COMPACT_CHUNK") = (int64_t)COMPACT_CHUNK;
  m.attr("COMPACT_MAX_COLS") = (int64_t)COMPACT_MAX_COLS;
  m.def("join_build",&join_build, "build chained hash table");
  m.def("join_unique_select", &join_unique_select,
        "unique inner join + residual comparison + projection, one pass",
        py::arg("probe_keys"), py::arg("build_keys"), py::arg("heads"),
        py::arg("next"), py::arg("pred"), py::arg("out_specs"),
        py::arg("block_rows") = 0);
  m.def("join_emit_unique", &join_emit_unique,
        "single-pass join emit for unique build keys");
  m.def("hash_string_column", &hash_string_column,
        "combine a string column into the running row hash");
  m.def("hash_seed", &hash_seed, "seed a row-hash buffer");
  m.def("gb_mark_reps", &gb_mark_reps,
        "representative rows + h2 verification for hashed group-by");
  m.def("expr_value", &expr_value,
        "fused value-expression interpreter");
  m.def("expr_filter", &expr_filter,
        "fused filter-predicate interpreter");
  m.def("gather_columns", &gather_columns,
        "fused multi-column row gather");
  m.def("gb_key_stats", &gb_key_stats,
        "fused key min/max + sampled distinct estimate");
  m.def("pack_columns", &pack_columns, "pack key columns into int64");
  m.def("unpack_column", &unpack_column, "unpack one key column");
  m.def("seg_rank_chunk", &seg_rank_chunk,
        "sorted positions per block of the segmented rank kernels");
  m.def("seg_rank", &seg_rank,
        "segmented row_number/rank/dense_rank in original row order");
  m.def("seg_take", &seg_take,
        "deterministic first-n-per-segment index vector");
  m.def("seg_shift", &seg_shift,
        "segment-bounded shift (LAG/LEAD) in original row order");
  m.def("seg_scan", &seg_scan,
        "segmented running sum/min/max + non-null count");
  m.def("seg_total", &seg_total,
        "whole-partition sum/min/max/first/last + non-null count");
  m.def("seg_frame_tile", &seg_frame_tile,
        "sorted positions per block of the frame kernel");
  m.def("seg_frame_max_reach", &seg_frame_max_reach,
        "largest frame reach the frame kernel takes");
  m.def("seg_frame", &seg_frame,
        "moving-frame sum/min/max/first/last + non-null count");
  m.def("gb_compact", &gb_compact,
        "deterministic group-table compaction");
  m.def("compact_columns_cap", &compact_columns_cap,
        "mask compaction, capacity outputs + cursor");
  m.def("join_open_unique", &join_open_unique,
        "open-addressed unique int join (build+probe)");
  m.def("topk_select", &topk_select, "own top-k (k<=16) select");
  m.def("eq2_mask", &eq2_mask, "128-bit string equality mask");
  m.def("cmp_imm", &cmp_imm, "single col-vs-literal comparison mask");
  m.def("cmp_col", &cmp_col, "single col-vs-col comparison mask");
  m.def("compact_columns", &compact_columns,
        "fused masked compaction of 8-byte columns");
  m.def("join_count", &join_count, "count matches per probe row");
  m.def("join_emit", &join_emit, "emit join pairs");
  m.def("reduce_columns", &reduce_columns,
        "global column reductions (MFMA-reduced sums)");
  m.def("join_pairs", &join_pairs,
        "total + chunked-reservation join pair emission");
  m.def("join_mark_build", &join_mark_build, "mark matched build rows");
}
