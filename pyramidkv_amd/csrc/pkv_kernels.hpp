// pkv_kernels.hpp — kernel parameter blocks and launch prototypes (internal to libpkv).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

// records the hipError_t pkv_last_hip_error() reports for this thread (defined in pkv_api.hip; internal to libpkv)
extern "C" __attribute__((visibility("hidden"))) void pkv_set_last_hip_error(int e);

namespace pkv {

// Per-kernel timing (pkv_prof_*): while a single-kernel profiling scope is open the API layer points g_kev at a pair of
// events and the launcher attaches them to the dispatch itself (hipExtLaunchKernelGGL): they carry the kernel's own begin
// and end timestamps, the same interval rocprofv3 reports, with no extra barrier packets in the stream.
struct KernelEvents { hipEvent_t start, stop; bool used; };
extern thread_local KernelEvents* g_kev;
#define PKV_KLAUNCH(kernel, grid, block, lds, st, ...)                                                              \
  do {                                                                                                              \
    if (pkv::g_kev) {                                                                                               \
      hipExtLaunchKernelGGL(kernel, grid, block, lds, st, pkv::g_kev->start, pkv::g_kev->stop, 0, __VA_ARGS__);     \
      pkv::g_kev->used = true;                                                                                      \
    } else {                                                                                                        \
      hipLaunchKernelGGL(kernel, grid, block, lds, st, __VA_ARGS__);                                                \
    }                                                                                                               \
  } while (0)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) only when a (kernel, device) pair needs MORE dynamic LDS than it was last
// granted - not on every launch (one runtime call per update_kv saved for top-k at S >= 16k; bench.py `host_us`).
// The grant belongs to the loaded code object: a host that calls hipDeviceReset() (or otherwise re-creates the context) must
// call pkv_runtime_reset() afterwards (include/pkv.h), which empties this table - the attribute is then set again on the next
// launch.  A table that is full (64 kernels x devices) stops caching: the attribute is then simply set on every launch.
struct DynLdsRec { const void* fn; int dev; size_t have; };
struct DynLdsTable { DynLdsRec recs[64]; int n; unsigned epoch; };
extern unsigned g_dyn_lds_epoch;                       // bumped by pkv_runtime_reset(): every thread's table is stale
inline hipError_t dyn_lds(const void* fn, size_t bytes) {
  static thread_local DynLdsTable t = {{}, 0, 0};
  if (t.epoch != g_dyn_lds_epoch) { t.n = 0; t.epoch = g_dyn_lds_epoch; }
  int dev = 0;
  (void)hipGetDevice(&dev);
  DynLdsRec* hit = nullptr;
  for (int i = 0; i < t.n; ++i)
    if (t.recs[i].fn == fn && t.recs[i].dev == dev) { hit = &t.recs[i]; break; }
  if (hit && hit->have >= bytes) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return e;
  if (hit) hit->have = bytes;
  else if (t.n < 64) t.recs[t.n++] = {fn, dev, bytes};
  return hipSuccess;
}

// Measurement hooks (phase stamps, per-workgroup wall clocks, ablations that produce WRONG results) exist only in the
// -DPKV_DEBUG build (make debug -> libpkv_debug.so, loaded by tools/ through PKV_LIB); in the release library the
// accessors below are compile-time constants, so the hot loops carry no trace/ablation branches at all.
#ifdef PKV_DEBUG
#define PKV_ABLATE(p) ((p).ablate)
#define PKV_WGTRACE(p) ((p).wgtrace)
#define PKV_TRACE(p) ((p).trace)
#else
#define PKV_ABLATE(p) 0
#define PKV_WGTRACE(p) (static_cast<unsigned long long*>(nullptr))
#define PKV_TRACE(p) (static_cast<unsigned long long*>(nullptr))
#endif

// Route of the last window-score call (pkv_debug_score_route, debug build, host only): the launchers write the instantiation
// they launch, do_score_window the rest.  Word order: include/pkv.h.
enum ScoreRouteWord {
  SR_KERNEL, SR_VARIANT, SR_TILE, SR_LDS_OPTIN, SR_NST, SR_NT, SR_LAST_NH, SR_STRADDLE_STAGE, SR_STRADDLE_WG, SR_ST_MODE,
  SR_FIN_W, SR_FIN_PPT, SR_HALO_SPREAD, SR_FIN_BLOCKS, SR_NTLOAD, SR_FEXP, SR_WORDS
};
#ifdef PKV_DEBUG
extern int g_score_route[SR_WORDS];
#define PKV_SCORE_ROUTE(i, v) (pkv::g_score_route[(i)] = (v))
#else
#define PKV_SCORE_ROUTE(i, v) ((void)0)
#endif

// Route of the last LOOK-M merge (pkv_debug_merge_route, debug build): launch_merge and launch_merge_t / launch_merge_f32_t
// write the host's choices; the last word is read back from the device, where the merge kernels of the debug build OR one bit
// per data-dependent path into the spare word behind MergeParams::ndrop (the workspace layout is the release one: the ndrop
// slot is 256 bytes, 4 of them used).  Word order: include/pkv.h.
enum MergeRouteWord {
  MR_DROPLIST, MR_DROP_GRID, MR_PIVOT, MR_KS, MR_NT_LOAD, MR_PF, MR_NST, MR_PIVOT_GRID, MR_WG_PER_HEAD, MR_LAST_NH,
  MR_BUCKET_FAST, MR_BUCKET_RANGES, MR_SCATTER_BLOCK, MR_BITMAP_BYTES, MR_NTP, MR_FLAGS, MR_WORDS
};
enum MergeFlag : unsigned int {
  MF_P2_SIGNED = 1u << 0,        // merge_pivot2_kernel: a stage finished on the signed-integer key loop
  MF_P2_REDO = 1u << 1,          // ... was redone with the exact keys (a row's maximum not above +0)
  MF_P2_NAN_EXACT = 1u << 2,     // ... took the exact keys because of kept_bad / a bad row in the wave
  MF_P2_MUL = 1u << 3,           // bf16: unit rows by multiplication with the reciprocal
  MF_P2_DIVC = 1u << 4,          // bf16: unit rows by div_const (a zero / subnormal / non-finite norm in the wave)
  MF_P2_PREFETCH = 1u << 5,      // a prefetch was issued inside stage() (s + PF < nh)
  MF_P2_RAGGED = 1u << 6,        // a workgroup with nh < nst
  MF_P2_PAST_END = 1u << 7,      // a workgroup past the end of the drop list
  MF_P1_EXACT = 1u << 8,         // merge_pivot_kernel with the NaN-exact keys
  MF_BUCKET_FAST = 1u << 9,
  MF_BUCKET_RANGES = 1u << 10,   // the ranged path with more than one range
  MF_SC_GROUP0 = 1u << 11,       // merge_scatter_kernel: a kept row nothing merges into
  MF_SC_OVER_CAP = 1u << 12,     // ... a group of more than MS_CAP rows (several list passes)
  MF_SC_TAIL_LO = 1u << 13,      // ... a 64-row block with a tail of 1..31 rows
  MF_SC_TAIL_HI = 1u << 14,      // ... of 33..63 rows
  MF_ZERO_LOOK = 1u << 15,       // a row whose maximum is zero was looked at again (first zero of either sign wins)
};
#ifdef PKV_DEBUG
extern int g_merge_route[MR_WORDS];
extern const unsigned int* g_merge_flags;      // device address of the flags word of the last merge
#define PKV_MERGE_ROUTE(i, v) (pkv::g_merge_route[(i)] = (int)(v))
#define PKV_MERGE_FLAG(p, bit) atomicOr(reinterpret_cast<unsigned int*>((p).ndrop) + 1, (unsigned int)(bit))
#else
#define PKV_MERGE_ROUTE(i, v) ((void)0)
#define PKV_MERGE_FLAG(p, bit) ((void)0)
#endif

// Route of the last 16-bit H2O score call (pkv_debug_h2o_route / pkv_debug_h2o_rows, debug build): launch_h2o_stats and
// launch_h2o_colsum write the host's choices; every workgroup of h2o_stats_kernel of the debug build stores the code of the path
// it took (enum H2OWgRoute) as one int32 at slot (bh, blockIdx.x) of the spare half of the rowstat slot - the workspace sizes that
// slot for the fp32 form's float2 per row, the 16-bit kernels use B*H*S floats of it, and the codes start right behind them (the
// workspace layout is the release one).  The last four words are counted from those codes.  launch_h2o_f32 records nothing.
// Word order: include/pkv.h.
enum H2ORouteWord {
  H2R_DTYPE, H2R_KS, H2R_STATS_GRID_X, H2R_STATS_GRID_Y, H2R_COLSUM_GRID_X, H2R_COLSUM_GRID_Y, H2R_NTILES, H2R_T_PLAIN,
  H2R_STATS_LDS, H2R_COLSUM_LDS, H2R_STATS_DYN_LDS, H2R_COLSUM_DYN_LDS, H2R_N_FROZEN, H2R_N_REPEAT, H2R_N_WIDE, H2R_N_SHORT, H2R_WORDS
};
enum H2OWgRoute : int {
  H2O_WG_FROZEN = 1,             // frozen reference point, no row overflowed
  H2O_WG_REPEAT = 2,             // frozen, a row overflowed: the row range ran again with the tracked maximum
  H2O_WG_WIDE = 3,               // the look at the first 16 keys found a wide row: tracked maximum from the start
  H2O_WG_SHORT = 4,              // t_plain == 0: tracked maximum, every tile through the edge body
};
#ifdef PKV_DEBUG
extern int g_h2o_route[H2R_WORDS];
extern const float* g_h2o_rowstat;             // device address of c_row [B*H][S] of the last 16-bit H2O call; the codes follow it
extern long long g_h2o_rows, g_h2o_wgs;        // B*H*S and B*H*grid.x of that call
#define PKV_H2O_ROUTE(i, v) (pkv::g_h2o_route[(i)] = (int)(v))
#define PKV_H2O_WG(p, bh, tid, code)                                                                                \
  do {                                                                                                              \
    if ((tid) == 0)                                                                                                 \
      reinterpret_cast<int*>((p).rowstat + (int64_t)(p).B * (p).H * (p).S)[(int64_t)(bh) * gridDim.x + blockIdx.x] = (code); \
  } while (0)
#else
#define PKV_H2O_ROUTE(i, v) ((void)0)
#define PKV_H2O_WG(p, bh, tid, code) ((void)0)
#endif

struct LogitsParams {
  unsigned long long* wgtrace = nullptr; // debug: per-workgroup (start,end) wall clock, may be null
  const void* q = nullptr;
  const void* k = nullptr;
  void* logits = nullptr; // [B*H*w][Sp] model dtype
  float2* partial = nullptr; // [B*H*w][nT] (tile row max, tile sum exp)
  int B = 0, H = 0, S = 0, w = 0, G = 0; // G = kv_group
  int D = 0;         // head size: 64, 128 or 256 (logits2_kernel: 128 only)
  int Sp = 0, nT = 0;
  int tile = 0;      // keys per workgroup: 128 or 256 (nT = ceil(S / tile))
  int nt = 0;        // nontemporal K loads
  int nst = 0;       // logits2_kernel: 128-key stages per workgroup (nT = chunks per head)
  int ablate = 0;    // 0 = full kernel; 1..3 = measurement-only ablations (PKV_LOGITS_ABLATE)
  int fexp = 0;      // logits2_kernel: hardware exp2 for the partial (max, sum exp) statistics
  int st_mode = 0;   // logits2_kernel: logits stores 0 = plain, 1 = nontemporal, 2 = write-through (sc1)
  uint32_t logits_bytes = 0; // extent of the logits buffer (raw-buffer stores)
  int64_t qs_b = 0, qs_h = 0, qs_s = 0;
  int64_t ks_b = 0, ks_h = 0, ks_s = 0;
  int scale_mode = 0;
  float sqrt_d = 0, rcp_sqrt_d = 0;
};

struct FinalizeParams {
  const void* logits = nullptr;
  const float2* partial = nullptr;
  void* scores = nullptr; // [B*H][scores_stride]
  int64_t scores_stride = 0;
  int B = 0, H = 0, S = 0, w = 0, Sp = 0, nT = 0;
  int pool_kind = 0, pool_kernel = 0, reduce = 0;
  void* cmax = nullptr;   // [B*H][cmax_stride] max pooled score of every 8-position chunk (may be null)
  int64_t cmax_stride = 0;
  unsigned long long* trace = nullptr; // debug: phase timestamps of block (0,0) (may be null)
  unsigned long long* wgtrace = nullptr;
  // Ada-SnapKV (round 5): the sum over ALL pooled scores of a row (:710 `attn_score.sum(dim=-1)`) as one fp64 partial per
  // workgroup, [B*H][rowsum_np] with rowsum_np = the grid's x dimension (1024 positions each); added in workgroup order by the
  // budget kernel (a fixed order: run-to-run identical).  May be null.
  double* rowsum_part = nullptr;
  int rowsum_np = 0;
};

struct TopkParams {
  const void* scores = nullptr; // [rows][scores_stride] model dtype
  int64_t scores_stride = 0;
  int L = 0, k = 0;
  const int32_t* k_per_row = nullptr;
  const void* cmax = nullptr; // optional: per-chunk (8 scores) maxima written by finalize_kernel, [rows][cmax_stride]
  int64_t cmax_stride = 0;
  int32_t* idx_out = nullptr; // [rows][idx_stride]
  int64_t idx_stride = 0;
  unsigned long long* trace = nullptr; // debug: phase timestamps of row 0 (may be null)
  unsigned long long* wgtrace = nullptr;
  int Lw = 0;            // keys per wave (multiple of 512)
  int kpad = 0;          // words reserved for the selection list (see topk_lds_bytes)
  int dual = 0;          // second 32 KB counter / radix scratch region present in LDS
  int algo = 0;          // small-k fast path: 1 = one-level histogram + bucket counting sort, 0 = two-level select + radix ordering
  int nseg = 0, seg_len = 0; // long rows: workgroup r handles segment r % nseg (seg_len keys) of row r / nseg and writes
                         // row-global indices to idx_out row r; L stays the full row length.  nseg <= 1: off
  // Ada-SnapKV (round 5, topk_kernel<T, true>): the selection also hands over every head's ADAPTIVE list (:706-711) as
  // order-preserving 16-bit keys in output order: the winners' raw scores, times the head's ratio sum(top base) / sum(all)
  // (:710; the row total comes from finalize_kernel's per-workgroup fp64 partials), rounded to the model dtype (:711).  The
  // budget step then only has to find the global threshold over those keys.
  void* list_out = nullptr;   // [rows][list_stride] uint16 keys, or null
  int64_t list_stride = 0;
  const double* rowsum_part = nullptr; // [rows][rowsum_np] finalize_kernel's partial sums of the row (normalize only)
  int rowsum_np = 0;
  int ada_base = 0;          // base capacity: the ratio's numerator sums the first ada_base entries of the list
  int ada_normalize = 0;
};

struct SortParams {
  const void* scores = nullptr;
  int64_t scores_stride = 0;
  int L = 0, n = 0;      // n = power of two >= L
  int32_t* sorted_idx = nullptr; // [rows][L]
  void* sorted_val = nullptr; // [rows][L] or null
  unsigned long long* trace = nullptr; // debug: phase stamps of row 0 (may be null)
};

struct GatherParams {
  unsigned long long* wgtrace = nullptr; // debug: per-workgroup (start,end) wall clock, may be null
  const void* kptr = nullptr;
  const void* vptr = nullptr;
  void* k_out = nullptr;
  void* v_out = nullptr;
  const int32_t* idx = nullptr; // [B*H][idx_stride] or null (identity: StreamingLLM)
  int64_t idx_stride = 0;
  const int32_t* head_k = nullptr; // per-(b,h) selected count (flat layout) or null -> uniform k
  const int32_t* cu_rows = nullptr; // per-(b,h) first output row (flat layout) or null -> bh*(k+w)
  int B = 0, H = 0, S = 0, w = 0, nsel = 0, G = 0; // nsel = uniform selected-row count k
  int D = 0;                 // head size: 64, 128 or 256 (a row is D*2 bytes = D/8 lanes x 16 B)
  int64_t ks_b = 0, ks_h = 0, ks_s = 0;
  int64_t vs_b = 0, vs_h = 0, vs_s = 0;
  int rpt = 0;               // rows per lane and tensor: 2, 4 or 8 (16*rpt rows per workgroup)
  int xcd_map = 0;           // place the blocks of head bh on XCD bh % 8 (where top-k wrote its indices)
  int nblk = 0;              // row blocks per head (set by launch_gather)
  int64_t out_rows = 0;      // rows the output buffers hold: nothing is stored at or beyond it
};

struct BudgetParams {
  const void* sorted_val = nullptr; // [H][L] descending, or null when the list is given as (sorted_idx, scores)
  const int32_t* sorted_idx = nullptr; // [H][idx_stride]: the first L entries of every head's descending order (top-L indices), or null
  int64_t idx_stride = 0;
  const void* scores = nullptr; // [H][scores_stride] un-sorted score rows of length Lrow (with sorted_idx)
  int64_t scores_stride = 0;
  int Lrow = 0;
  int H = 0, L = 0, base = 0; // L = entries per head in the sorted list
  float one_minus_floor = 0; // (float)(1.0 - floor_ratio), the fp32 scalar ATen multiplies by
  int floor_capacity = 0;    // int(base * floor_ratio)
  int normalize = 0;
  int32_t* head_capacity = nullptr; // [H]
  int window = 0;            // with head_lens_out / cu_klen_out: the var-len metadata of :682-691 from the same launch
  int32_t* head_lens_out = nullptr; // [H] or null
  int32_t* cu_klen_out = nullptr; // [H+1] or null
  int32_t* cu_headlens_out = nullptr; // [H] inclusive prefix (:687) or null
  void* adaptive_out = nullptr; // optional: dtype [H][L] - emit every head's adaptive list (:711) and stop (head-sharded exchange)
  unsigned long long* host_mirror = nullptr; // optional: device-visible PINNED HOST memory, uint64 [H]: word h = host_seq << 32 | ran_out << 31 | cap_h
  int32_t host_seq = 0;
  int short_list = 0;        // the lists are SHORTER than min(L, H*base): bit 31 of the mirror words reports a head whose list ran out
  int unsorted = 0;          // 1: `scores` are the un-sorted rows [H][scores_stride] of length Lrow and no list is given
  void* list_ws = nullptr;    // optional: H * roundup(L,8) * 2 bytes, 16-B aligned - the looked-up lists travel through it
  void* ws = nullptr;         // 1024 B ratios + 2 * H*256 int32
  unsigned long long* trace = nullptr; // debug: phase timestamps of the one-launch budget kernel (may be null)
};

struct MergeParams {         // LOOK-M pivot merge (pkv_merge.hip)
  const void* kptr = nullptr;
  const void* vptr = nullptr;
  const int32_t* idx = nullptr; // [B*H][idx_stride] selected past tokens (top-k order)
  int64_t idx_stride = 0;
  void* k_out = nullptr;      // [B,H,k+w,D]  rows ordered [window, selected]
  void* v_out = nullptr;      // [B,H,k+w,D]  rows ordered [selected, window]
  int B = 0, H = 0, S = 0, w = 0, k = 0, G = 0;
  int64_t ks_b = 0, ks_h = 0, ks_s = 0;
  int64_t vs_b = 0, vs_h = 0, vs_s = 0;
  uint8_t* mask = nullptr;    // [S] 1 = selected by some (b,h)
  int32_t* ndrop = nullptr;   // number of dropped positions
  int32_t* drop = nullptr;    // [S] dropped positions, ascending
  int32_t* pivot = nullptr;   // [B*H][S] kept-row number (KEY order) every dropped row merges into
  void* tn = nullptr;         // [B*H][ntp][D] unit-norm kept keys
  int ntp = 0;
  int D = 0;                 // head size: 64, 128 or 256
  int32_t* kept_bad = nullptr; // [B*H] != 0: a kept key of the head has no finite unit-norm form (zeroed with the mask)
  int32_t* bstart = nullptr;  // [B*H][k+w+1] first entry of every kept row's group in blist (last = number of dropped rows)
  int32_t* blist = nullptr;   // [B*H][S] dropped positions grouped by the kept row they merge into
};

struct FlattenParams {
  const void* cache = nullptr;
  const void* state = nullptr;
  const int32_t* head_lens = nullptr;
  const int32_t* cu_klen = nullptr;
  void* out = nullptr;
  int H = 0, row_bytes = 0;
};

struct L2NormParams {        // key-norm scan of the L2Norm policy (pkv_l2norm.hip)
  const void* kptr = nullptr; // [B, Hkv, S, D], element strides below
  void* neg_out = nullptr;    // [B*Hkv][Lp] model dtype: -norm (+0 for a zero norm, -inf for a NaN norm); Lp % 8 == 0, Lp >= S.
                             // The padding S..Lp-1 is NOT neutral: it holds copies of row S-1's value, so whatever reads
                             // the row must mask by L = S (topk_kernel, topk_f32_kernel and sort_rows_kernel all do)
  void* norm_out = nullptr;   // [B*Hkv][S] model dtype: the norms themselves, or null
  int B = 0, Hkv = 0, S = 0, D = 0, Lp = 0;
  int64_t ks_b = 0, ks_h = 0, ks_s = 0;
  int nblk = 0;              // row blocks per head (set by launch_l2norm)
  int norm_vec = 0;          // norm_out takes 16-byte stores (set by launch_l2norm)
};

// ThinK key-channel pruning (pkv_think.hip).  The two sizes below fix the order of every fp32 sum and the shape of every
// output span; they depend on nothing but the tensor shape (pyramidkv_amd/_native.py mirrors them for the tests).
constexpr int THINK_SCAN_ROWS = 128;      // key rows per workgroup of think_scan_kernel = per fp32 partial
constexpr int THINK_TILE_BYTES = 16384;   // input bytes per workgroup of think_compact_kernel (16384 / (D * e) rows)
constexpr int THINK_QROWS = 32;           // the reference's literal: q_states[..., -32:, :] (pyramidkv_utils.py:17)
struct ThinkParams {
  const void* q = nullptr;    // [B, H, S, D], element strides below
  const void* kc = nullptr;   // [B, H, N, D] contiguous: the compacted keys
  float* part = nullptr;      // [B*H][nck + 1][D] fp32 sums of rounded squares: nck key chunks, then the query rows
  void* k_out = nullptr;      // [B*H][R][D - nprune] contiguous
  uint8_t* keep = nullptr;    // [B*H][D] 1 = kept
  int32_t* keep_idx = nullptr; // [B*H][D - nprune] ascending
  void* stats = nullptr;      // [B*H][3][D] model dtype (qe, ke, score) or null
  int B = 0, H = 0, S = 0, D = 0;
  int N = 0, R = 0;           // rows of kc; R = N - recent rows are compacted
  int nprune = 0, nq = 0;     // nq = min(THINK_QROWS, S)
  int nck = 0;                // ceil(N / THINK_SCAN_ROWS)
  int64_t qs_b = 0, qs_h = 0, qs_s = 0;
};

// Single-query attention over the flat var-len cache, or over the ThinK cache (pkv_decode.hip).  The chunk length
// PKV_DECODE_CHUNK (include/pkv.h) and `splits` fix the order of every fp32 sum; for the ThinK kernel `kept` as well.
constexpr int DECODE_TILE_BYTES = 16384;  // pruned-key bytes decode_think_kernel stages in LDS at a time (whole rows of kept * e bytes)
struct DecodeParams {
  const void* q = nullptr;    // [H][q_stride] model dtype, head_dim elements used
  const void* k = nullptr;    // flat: [sum_h n_h][D] contiguous.  ThinK: the full-width keys, [H] heads of n_full rows, k_stride apart
  const void* v = nullptr;    // flat: as k.  ThinK: [H] heads of n_pruned + n_full rows, v_stride apart
  const int32_t* cu_klen = nullptr; // flat: [H+1].  ThinK: null - that is how the launcher and the combine kernel tell the two apart
  const uint8_t* keep = nullptr;    // ThinK: [H][D], non-zero = kept channel
  const void* k_pruned = nullptr;   // ThinK: [H][n_pruned][kept] contiguous, 16-byte aligned base
  int kept = 0, n_pruned = 0, n_full = 0;
  int64_t k_stride = 0, v_stride = 0;   // ThinK: elements between heads
  void* out = nullptr;        // [H][D] model dtype
  float* lse = nullptr;       // [H] or null
  float* part_ml = nullptr;   // splits > 1: [H][splits][2] (max, sum) of every (head, split) that holds a chunk
  float* part_acc = nullptr;  // splits > 1: [H][splits][D] its un-normalised accumulator
  int H = 0, D = 0, splits = 0;
  int64_t q_stride = 0;
  float scale = 0;
};

struct H2OParams {
  const void* q = nullptr;
  const void* k = nullptr;
  float* rowstat = nullptr; // [B*H][S] c_row = -log2 sum_j exp(x_ij) of every query row
  void* scores = nullptr;
  int64_t scores_stride = 0;
  int B = 0, H = 0, S = 0, w = 0, G = 0;
  int D = 0;          // head size: 64, 128 or 256
  int64_t qs_b = 0, qs_h = 0, qs_s = 0;
  int64_t ks_b = 0, ks_h = 0, ks_s = 0;
  int scale_mode = 0;
  float sqrt_d = 0, rcp_sqrt_d = 0;
};

hipError_t launch_logits(int dtype, const LogitsParams& p, hipStream_t st);
hipError_t launch_logits2(int dtype, const LogitsParams& p, hipStream_t st);
hipError_t launch_finalize(int dtype, const FinalizeParams& p, hipStream_t st);
size_t topk_lds_bytes(int L, int k, int* Lw_out, int* kpad_out);
hipError_t launch_topk(int dtype, int rows, const TopkParams& p, size_t lds, hipStream_t st);
// long-row merge helpers: candidate scores of the per-segment winners, and the final index look-up
hipError_t launch_topk_merge_prep(int dtype, int rows, int L, int k, int nseg, int seg_len, const void* scores, int64_t scores_stride,
                                  const int32_t* cand_idx, void* cand_score, int64_t cand_stride, hipStream_t st);
hipError_t launch_topk_merge_finish(int rows, int k, const int32_t* cand_idx, int64_t cand_stride, const int32_t* pos, int32_t* idx_out,
                                    int64_t idx_stride, hipStream_t st);
// PKV_TIE_ATEN_ROCM: rows of k <= 32 canonical indices -> the order PyTorch-ROCm's topk gives them (16-bit scores)
hipError_t launch_aten_small_order(int dtype, int rows, int k, const void* scores, int64_t scores_stride, int32_t* idx, int64_t idx_stride,
                                   hipStream_t st);
hipError_t launch_sort_rows(int dtype, int rows, const SortParams& p, hipStream_t st);
hipError_t launch_gather(const GatherParams& p, int max_rows, hipStream_t st);
hipError_t launch_budget(int dtype, const BudgetParams& p, hipStream_t st);
// Ada-SnapKV budgets + metadata in ONE single-workgroup launch from the adaptive key lists topk_kernel<T, true> left behind
// (p.L entries per head at list[h * Lpad]); ada_fused_fits() = the lists of all heads fit one workgroup's LDS next to the counters
bool ada_fused_fits(int H, int M);
hipError_t launch_ada_fused(const BudgetParams& p, const void* list, int Lpad, hipStream_t st);
int finalize_blocks(int S, int w, int BH);     // workgroups per (b, h) row of finalize_kernel = row-sum partials per head (BH = B * H rows in the launch)
hipError_t launch_ada_final(const BudgetParams& p, int32_t* cum_hi, int32_t* cum_lo, const int32_t* above_hi, hipStream_t st);
hipError_t launch_budget_f32(const BudgetParams& p, hipStream_t st);      // fp32 score rows (pkv_f32.hip), ws: 1024 + 4*H*256*4 + 4*H*4 bytes
int budget_f32_max_row();
hipError_t launch_ada_metadata(int H, int w, const int32_t* cap, int32_t* head_lens, int32_t* cu_klen, hipStream_t st,
                               int32_t* cu_headlens = nullptr);
hipError_t launch_flatten(const FlattenParams& p, hipStream_t st);
hipError_t launch_merge(int dtype, const MergeParams& p, hipStream_t st);
size_t merge_max_seq();      // longest sequence the merge takes (LDS bitmap of the scatter kernel)
hipError_t launch_l2norm(int dtype, const L2NormParams& p, hipStream_t st);
// dst [BH][n] = src row bh / G (stride src_stride), entries 0..n-1
hipError_t launch_idx_expand(const int32_t* src, int64_t src_stride, int32_t* dst, int BH, int n, int G, hipStream_t st);
hipError_t launch_think(int dtype, const ThinkParams& p, hipStream_t st);      // scan -> select -> compaction, three launches
hipError_t launch_decode_attn(int dtype, const DecodeParams& p, hipStream_t st);   // one launch; splits > 1: + the combine launch; cu_klen == null: the ThinK kernel
hipError_t launch_debug_sqrt(const float* in, float* out, int64_t n, hipStream_t st);
hipError_t launch_debug_exp(const float* in, float* out, int64_t n, hipStream_t st);
hipError_t launch_debug_round(int dtype, const float* in, uint16_t* out, int64_t n, hipStream_t st);
hipError_t launch_debug_unit_div(int dtype, const uint16_t* x, const uint16_t* nrm, uint16_t* out_div, uint16_t* out_divc, uint16_t* out_mul,
                                 uint8_t* out_mul_ok, int64_t n, hipStream_t st);
// fp32 tensors (pkv_f32.hip)
hipError_t launch_logits_f32(const LogitsParams& p, hipStream_t st);
hipError_t launch_finalize_f32(const FinalizeParams& p, hipStream_t st);
hipError_t launch_topk_f32(int rows, const TopkParams& p, hipStream_t st);
int topk_f32_max_k();
hipError_t launch_h2o_f32(const H2OParams& p, hipStream_t st);            // fp32 tensors (pkv_f32.hip): rowstat = float2 (max, 1/sum) per row
hipError_t launch_h2o_stats(int dtype, const H2OParams& p, hipStream_t st);
hipError_t launch_h2o_colsum(int dtype, const H2OParams& p, hipStream_t st);

}  // namespace pkv
