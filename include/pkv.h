/* pkv.h — C ABI of libpkv: the MI355X (gfx950) prefill-time KV-cache eviction path.
 *
 * This is the drop-in boundary for the reference's
 *     pyramidkv/pyramidkv_utils.py  *KVCluster.update_kv        (Zefan-Cai/PyramidKV @ 2024-12-20)
 * The reference has no FFI for this path (it is eager PyTorch); each entry point below names the
 * reference lines it replaces.  Plain pointers and sizes only: no torch types, no pybind.
 * The only native symbol the reference does export is the decode-time flat-cache append
 *     csrc/csrc/cuda_api.cu:55-91  tiny_api_cuda.update_flatten_view
 * which pkv_update_flatten_view() replaces.
 *
 * Conventions
 *   - all pointers are DEVICE pointers on the device that is current when the call is made;
 *   - every launch goes to `stream` (a hipStream_t passed as void*); no call synchronises the
 *     device or allocates user-visible memory; workspaces are caller-provided;
 *   - tensors are [B,H,S,D] with ELEMENT strides for b,h,s and D contiguous (stride 1);
 *     base pointers and strides must keep every row 16-byte aligned;
 *   - return value 0 = success, negative = pkv_status; pkv_strerror() names it.  Nothing aborts.
 */
#ifndef PKV_H
#define PKV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PKV_VERSION 204 /* still 0.2.4: + pkv_debug_h2o_route, pkv_debug_h2o_rows (two debug hooks added within 0.2.4: no struct layout
                           change, no workspace change; the release library answers PKV_ERR_UNSUPPORTED).
                           + pkv_decode_attn_think (one more symbol added within 0.2.4 on the same terms as the three below).
                           + pkv_decode_attn_splits, pkv_decode_attn_workspace_bytes, pkv_decode_attn_flat (three more symbols
                           added within 0.2.4, exactly as the ThinK ones below: no struct layout change, no profiling class, PKV_K_COUNT
                           stays 9; a host that needs them checks for the symbols).
                           + pkv_think_workspace_bytes, pkv_think_prune (two symbols added within 0.2.4: no struct layout
                           change, PKV_K_COUNT stays 9 - the ThinK kernels have no profiling class - so a host built against 204
                           keeps working; a host that needs them checks for the symbols).
                           0.2.4: + pkv_l2norm_workspace_bytes, pkv_compress_l2norm, pkv_debug_sqrt, PKV_K_L2NORM; no struct layout change,
                           but PKV_K_COUNT grows from 8 to 9: pkv_prof_read now writes 9 entries, so a host built against 203
                           with arrays of 8 must check pkv_version() (or be rebuilt) before it reads the profile.
                           0.2.3: + pkv_debug_merge_route, pkv_debug_unit_div; no layout change.
                           0.2.2: + pkv_debug_score_route; no layout change.
                           0.2.1: + pkv_runtime_reset, pkv_debug_scale_multiplier; pkv_ada_budget_rows validates its host
                           mirror (8-byte aligned uint64 [H], host_seq >= 0) like pkv_ada_select; no layout change.  0.2.0: pkv_desc starts with struct_size (the struct can grow without breaking hosts built against an
                           older header); pkv_ada_select's budget step is one launch; host mirrors are uint64 [H] of
                           self-validating words; fp32 at D = 256; 0.1.2: short Ada-SnapKV candidate lists */
/* libpkv.so is built with -fvisibility=hidden: the entry points below are its whole dynamic symbol table (plus nothing). */
#define PKV_API __attribute__((visibility("default")))

typedef void* pkv_stream_t; /* hipStream_t */

enum pkv_status {
  PKV_OK = 0,
  PKV_ERR_DTYPE = -1,       /* dtype not bf16 / fp16 / fp32 */
  PKV_ERR_SHAPE = -2,       /* D not in {64,128,256}, window/topk out of range, k > L ... */
  PKV_ERR_ALIGN = -3,       /* pointer or stride breaks 16-byte row alignment */
  PKV_ERR_WORKSPACE = -4,   /* workspace too small */
  PKV_ERR_UNSUPPORTED = -5, /* valid request outside the limits of this build */
  PKV_ERR_HIP = -6,         /* a HIP runtime call failed; see pkv_last_hip_error() */
  PKV_ERR_NULL = -7,
  PKV_ERR_COLLECTIVE = -8,  /* an RCCL call failed; see pkv_last_nccl_error() */
  PKV_ERR_ABI = -9          /* pkv_desc.struct_size is not a size this library knows (host built against another pkv.h) */
};

/* PKV_F32: pkv_score_window, pkv_score_h2o, pkv_topk(_ws), pkv_gather_compact, pkv_gather_streaming, pkv_gather_flat,
 * pkv_compress, pkv_compress_h2o, pkv_compress_l2norm, pkv_think_prune, pkv_select, pkv_merge_compact, pkv_ada_budget_rows, pkv_ada_metadata and
 * pkv_update_flatten_view, pkv_decode_attn_flat and pkv_decode_attn_think, D in {64,128,256} (256 since 0.2.0), topk <= 4096; every other entry point (pkv_sort_rows, pkv_ada_budget,
 * pkv_ada_budget_topm, pkv_ada_adaptive_lists, pkv_ada_select) answers PKV_ERR_DTYPE / PKV_ERR_UNSUPPORTED. */
enum pkv_dtype { PKV_BF16 = 0, PKV_F16 = 1, PKV_F32 = 2 };
enum pkv_pool { PKV_POOL_NONE = 0, PKV_POOL_AVG = 1, PKV_POOL_MAX = 2 };
enum pkv_reduce { PKV_REDUCE_SUM = 0, PKV_REDUCE_MEAN = 1 };
/* how A/sqrt(D) is evaluated (pyramidkv_utils.py:317): DIV = fp32 division (ATen CPU),
 * RCP = multiply by fp32 reciprocal (ATen GPU kernels for a host-scalar divisor). */
enum pkv_scale { PKV_SCALE_DIV = 0, PKV_SCALE_RCP = 1 };
/* Order of EQUAL scores in the selected rows (pyramidkv_utils.py:334: `tensor.topk` leaves it to the backend).
 * CANONICAL = (value descending, index ascending) = a stable descending sort - what PyTorch-ROCm's topk produces for k > 32.
 * ATEN_ROCM: for topk <= 32 additionally reproduce the order PyTorch-ROCm's topk leaves equal scores in (its k <= 32 results go
 * through an unstable 32-element bitonic network, ATen/native/hip/SortUtils.cuh bitonicSortKVInPlace): the cache rows of
 * PyramidKV's upper layers (k = 17..32) then sit in the order of a reference run on the same GPU.  Same token set either way. */
enum pkv_tie { PKV_TIE_CANONICAL = 0, PKV_TIE_ATEN_ROCM = 1 };

/* The descriptor GROWS at its end from version to version.  The caller stores sizeof(pkv_desc) of the header it was compiled
 * against in struct_size; the library reads exactly that many bytes - never more - and takes every field the caller's
 * struct does not have yet as 0 (each new field is defined so that 0 = the behaviour before it existed).  A size below
 * PKV_DESC_MIN_SIZE or above the library's own sizeof(pkv_desc) returns PKV_ERR_ABI from every entry point that takes a
 * descriptor (pkv_workspace_bytes / pkv_merge_workspace_bytes return 0). */
typedef struct pkv_desc {
  uint32_t struct_size; /* sizeof(pkv_desc) as the CALLER compiled it */
  int32_t dtype;        /* pkv_dtype of q,k,v and of every score buffer */
  int32_t B, H, S, D;   /* H = number of query heads; D = 64, 128 or 256 (all entry points) */
  int32_t kv_group;     /* 1: k,v have H heads (post-repeat_kv, the reference contract).
                           g>1: k,v have H/g heads (un-expanded GQA); head h reads kv head h/g */
  int32_t reserved0;    /* must be 0 (keeps the strides 8-byte aligned without implicit padding) */
  int64_t q_stride[3];  /* element strides of q for b,h,s */
  int64_t k_stride[3];
  int64_t v_stride[3];
  int32_t window;       /* w = window_size, 1..128 (scoring entry points; kv_group * window <= 256) */
  int32_t pool_kind;    /* pkv_pool */
  int32_t pool_kernel;  /* odd, <= 17; padding = kernel/2, stride 1 (pyramidkv_utils.py:328-331) */
  int32_t reduce;       /* pkv_reduce: SUM for SnapKV/PyramidKV (:327), MEAN for AdaKV/HeadKV (:661) */
  int32_t scale_mode;   /* pkv_scale */
  int32_t topk;         /* k = past tokens kept per head, 1..S-window (host-resolved per layer) */
  int32_t tie_order;    /* a pkv_tie value, honoured by the selecting entry points pkv_compress, pkv_compress_h2o, pkv_select on
                           bf16 / fp16 scores; 0 = canonical; any other value than 0 / 1 returns PKV_ERR_SHAPE from every entry
                           point that validates the descriptor (since 0.1.1) */
  int32_t reserved1;    /* must be 0 (explicit tail padding: sizeof(pkv_desc) is a multiple of 8 without implicit padding) */
} pkv_desc;
#define PKV_DESC_MIN_SIZE 136u /* sizeof(pkv_desc) of 0.2.0, the first layout that carries struct_size */

PKV_API int pkv_version(void);
PKV_API const char* pkv_strerror(int status);
PKV_API int pkv_last_hip_error(void); /* hipError_t of the last PKV_ERR_HIP on this thread */
/* libpkv remembers, per (kernel, device), how much dynamic LDS it has asked the runtime for (hipFuncSetAttribute is then not
 * called on every launch).  That grant dies with the context: a host that calls hipDeviceReset() - or unloads and re-creates
 * the primary context in any other way - calls this afterwards; the attribute is then set again on the next launch. */
PKV_API int pkv_runtime_reset(void);

/* Bytes of scratch pkv_score_window / pkv_score_h2o / pkv_compress need for `d` (256-B aligned). */
PKV_API size_t pkv_workspace_bytes(const pkv_desc* d);

/* Observation-window score (pyramidkv_utils.py:317-333, AdaKV :649-672):
 *   logits = (Q[-w:] K^T)/sqrt(D) -> causal corner mask -> fp32 softmax over all S keys -> round
 *   -> sum/mean of the w rows over columns [0,S-w) -> round -> avg/max pool.
 * scores_out: [B*H rows][scores_stride] elements of d->dtype, columns [0, S-w) written. */
PKV_API int pkv_score_window(const pkv_desc* d, const void* q, const void* k, void* scores_out,
                     int64_t scores_stride, void* ws, size_t ws_bytes, pkv_stream_t stream);

/* H2O score (pyramidkv_utils.py:544-554,561): all S query rows, SxS never materialised.
 * Same output layout as pkv_score_window; no pooling. */
PKV_API int pkv_score_h2o(const pkv_desc* d, const void* q, const void* k, void* scores_out,
                  int64_t scores_stride, void* ws, size_t ws_bytes, pkv_stream_t stream);

/* Top-k token selection (pyramidkv_utils.py:334, :238, :270, :562): for each of `rows` score rows
 * of length L pick the k largest, emitted in (value desc, index asc) order as int32.
 * scores: [rows][scores_stride] of dtype; idx_out: [rows][idx_stride] int32.
 * k_per_row (device int32[rows], may be NULL) overrides k per row (k = upper bound then). */
PKV_API int pkv_topk(int32_t dtype, int32_t rows, int32_t L, int32_t k, const void* scores,
             int64_t scores_stride, const int32_t* k_per_row, int32_t* idx_out, int64_t idx_stride,
             pkv_stream_t stream);

/* Rows longer than one workgroup's LDS (L > 57 344 keys; k <= 32 768): the same selection through per-segment
 * top-k + a top-k over the segment winners; needs pkv_topk_workspace_bytes() of 16-B aligned scratch (0 for rows
 * pkv_topk handles itself; k_per_row is not supported on long rows). */
PKV_API size_t pkv_topk_workspace_bytes(int32_t rows, int32_t L, int32_t k);
PKV_API int pkv_topk_ws(int32_t dtype, int32_t rows, int32_t L, int32_t k, const void* scores,
                int64_t scores_stride, const int32_t* k_per_row, int32_t* idx_out, int64_t idx_stride,
                void* ws, size_t ws_bytes, pkv_stream_t stream);

/* Gather-compaction (pyramidkv_utils.py:335,341-346): K_out/V_out[b,h] = rows idx[b,h,0..k) of
 * K/V[b,h,:S-w] followed by the w window rows S-w..S-1.  Outputs are contiguous [B,H,k+w,D].
 * idx: int32 [B*H][idx_stride].  d->topk = k.  Uses d->k_stride/v_stride/kv_group. */
PKV_API int pkv_gather_compact(const pkv_desc* d, const void* k, const void* v, const int32_t* idx,
                       int64_t idx_stride, void* k_out, void* v_out, pkv_stream_t stream);

/* StreamingLLM (pyramidkv_utils.py:607-620): idx = 0..k-1 for every head; no scoring. */
PKV_API int pkv_gather_streaming(const pkv_desc* d, const void* k, const void* v, void* k_out, void* v_out,
                         pkv_stream_t stream);

/* Fused update_kv for SnapKV / PyramidKV (pyramidkv_utils.py:306-347, :197-283; k resolved by the
 * host per layer): score -> top-k -> gather on `stream`.  idx_out (int32 [B*H][d->topk]) may be NULL
 * (then it lives in ws). */
PKV_API int pkv_compress(const pkv_desc* d, const void* q, const void* k, const void* v, void* k_out,
                 void* v_out, int32_t* idx_out, void* ws, size_t ws_bytes, pkv_stream_t stream);

/* Fused update_kv for H2O (pyramidkv_utils.py:533-575). */
PKV_API int pkv_compress_h2o(const pkv_desc* d, const void* q, const void* k, const void* v, void* k_out,
                     void* v_out, int32_t* idx_out, void* ws, size_t ws_bytes, pkv_stream_t stream);

/* Fused update_kv for L2Norm (pyramidkv_utils.py:405-429, L2NormCluster): keep the d->topk keys of SMALLEST L2 norm, in
 * (norm ascending, index ascending) order; no query, no observation window, no pooling.  Norm scan (:419) -> the canonical
 * top-k on the negated norms (:420) -> gather (:423-427), on `stream`.
 *   norm = fp32 sum of squares -> correctly rounded fp32 sqrt -> ONE round-to-nearest-even to d->dtype (what torch.norm
 *   gives up to the order of the fp32 sum).  Equal norms are kept lowest index first (`argsort` leaves their order to the
 *   backend).  +inf norms sort last, by index; a NaN norm is ordered with them.
 * d->window must be 0 (PKV_ERR_SHAPE otherwise; every other entry point keeps rejecting window < 1); d->topk = cap with
 * 1 <= cap <= S (cap == S returns the full permutation); q_stride, pool_kind, pool_kernel, reduce and scale_mode are
 * ignored; the order is always canonical.  d->kv_group = g: k, v have H/g heads; norms and selection run ONCE per KV head
 * and every query head of a group receives its rows.
 *   k_out, v_out: contiguous [B,H,cap,D] (no window rows are appended).
 *   idx_out:      int32 [B*H][cap], may be NULL.
 *   norm_out:     d->dtype [B*(H/g)][S] contiguous, the norms themselves; may be NULL; 16-byte aligned.
 *   ws:           pkv_l2norm_workspace_bytes(d), 16-B aligned (0 = the descriptor is not one this entry point takes).
 * Limits = those of the selection: one workgroup up to S = 57 344 with cap <= 16 384; longer rows in segments with
 * cap <= 4096; a complete sort of the row for larger cap up to S = 32 768 (16-bit dtypes); PKV_F32: cap <= 4096.
 * PKV_ERR_UNSUPPORTED beyond. */
PKV_API size_t pkv_l2norm_workspace_bytes(const pkv_desc* d);
PKV_API int pkv_compress_l2norm(const pkv_desc* d, const void* k, const void* v, void* k_out, void* v_out, int32_t* idx_out,
                        void* norm_out, void* ws, size_t ws_bytes, pkv_stream_t stream);

/* ThinK key-channel pruning (pyramidkv_utils.py:13-26 key_pruner_query_driven, called from :390 SnapKVCluster.update_think): a
 * second pass over the keys a compress call has compacted.  Every key channel gets a score, the n_prune channels of smallest
 * score are dropped from all but the last `recent` keys.  Three launches on `stream` (channel-energy scan -> select -> channel
 * compaction), no host synchronisation (the reference's boolean-mask index is a nonzero() with one).
 *   energy of a channel over n rows = every element squared and the square rounded to d->dtype (torch.pow in the model dtype;
 *     fp32: one rounded multiply) -> fp32 sum of the rounded squares (the order is the library's own and fixed: two calls give
 *     the same bits) -> ONE correctly rounded fp32 division by n -> ONE round-to-nearest-even to d->dtype;
 *   qe = energy over the last min(32, S) rows of q (the 32 is the reference's literal, :17), ke = energy over all n_rows rows
 *     of kc, score = dtype(float(qe) * float(ke));
 *   pruned = the n_prune channels first in (score ascending, channel index ascending); NaN scores rank behind +inf, by index
 *     (`torch.topk(largest=False)` leaves equal scores to the backend).
 * The descriptor supplies dtype, B, H, S, D and q_stride; kv_group must divide H and is otherwise ignored, window, topk, the
 * pooling fields and k_stride / v_stride are not looked at.
 *   q:             [B,H,S,D] through d->q_stride (the model's transposed view is taken as it is).
 *   kc:            d->dtype [B,H,n_rows,D] contiguous, n_rows >= 1.
 *   recent:        0 <= recent < n_rows; n_prune: 0 <= n_prune < D (the host's int(D * ratio)); PKV_ERR_SHAPE otherwise.
 *   k_pruned_out:  d->dtype [B*H][n_rows - recent][D - n_prune] contiguous: the kept channels, ascending, of rows
 *                  0 .. n_rows - recent - 1, bit copies.  Nothing outside these bytes is written.
 *   keep_out:      uint8 [B*H][D], 1 = kept (the reference's ~mask).
 *   keep_idx_out:  int32 [B*H][D - n_prune] ascending, may be NULL (then it lives in ws); 4-byte aligned.
 *   stats_out:     d->dtype [B*H][3][D] = qe, ke, score; may be NULL.
 *   q, kc, k_pruned_out, stats_out, ws: 16-byte aligned.  ws: pkv_think_workspace_bytes(d, n_rows) (0 = the descriptor or
 *   n_rows is not one this entry point takes).
 * The rows n_rows - recent .. n_rows - 1 keep all D channels: the caller's view kc[:, :, n_rows - recent:, :], no kernel. */
PKV_API size_t pkv_think_workspace_bytes(const pkv_desc* d, int32_t n_rows);
PKV_API int pkv_think_prune(const pkv_desc* d, const void* q, const void* kc, int32_t n_rows, int32_t recent, int32_t n_prune,
                    void* k_pruned_out, uint8_t* keep_out, int32_t* keep_idx_out /* may be NULL */,
                    void* stats_out /* may be NULL */, void* ws, size_t ws_bytes, pkv_stream_t stream);

/* Selection only: the front half of pkv_compress / pkv_compress_h2o (score -> top-k), idx_out int32 [B*H][d->topk].
 * What a caller needs when something other than the plain gather follows (the merge below).  ws: pkv_workspace_bytes(d). */
PKV_API int pkv_select(const pkv_desc* d, const void* q, const void* k, int32_t h2o, int32_t* idx_out, void* ws, size_t ws_bytes,
               pkv_stream_t stream);

/* LOOK-M pivot merge (pyramidkv_utils.py:119-170 merge_kv(..., merge="pivot"), called from :242,:274,:338,:566,:611 when the
 * cluster's `merge` is set) instead of the plain gather: every position NO (batch, head) selected - the window positions
 * included (:128-133) - is merged into its most cosine-similar kept key (first maximum, :150-151) as (x + pivot)/2, and the
 * kept rows become the scatter-mean of what reached them (:158-162).  As in the reference k_out is ordered
 * [window, selected] (:146) and v_out [selected, window] (:148), and the value merge uses the key order's pivot numbers.
 * idx: int32 [B*H][idx_stride] (d->topk = k entries per row, from pkv_select / pkv_topk).  Outputs [B,H,k+w,D] contiguous.
 * ws: pkv_merge_workspace_bytes(d), 16-B aligned.  Rounding points: oracle/pkv_oracle.py merge_kv_explicit.
 * bf16 / fp16 / fp32 (since 0.1.2; D = 256 since 0.2.0) at D = 64 / 128 / 256, fp32 with topk <= 4096; S <= 393 216 and
 * k + window <= 65 535 (PKV_ERR_UNSUPPORTED beyond). */
PKV_API size_t pkv_merge_workspace_bytes(const pkv_desc* d);
PKV_API int pkv_merge_compact(const pkv_desc* d, const void* k, const void* v, const int32_t* idx, int64_t idx_stride,
                      void* k_out, void* v_out, void* ws, size_t ws_bytes, pkv_stream_t stream);

/* ---- Ada-SnapKV / HeadKV (pyramidkv_utils.py:674-757, :808-878): flat var-len output ---- */

/* Per-row full descending sort (:706 attn_score.sort(descending=True)), ties index-ascending.
 * sorted_idx: int32 [rows][L]; sorted_val (may be NULL): dtype [rows][L].  L <= 32768. */
PKV_API int pkv_sort_rows(int32_t dtype, int32_t rows, int32_t L, const void* scores, int64_t scores_stride,
                  int32_t* sorted_idx, void* sorted_val, pkv_stream_t stream);

/* Head budgets (:709-719): optional normalisation, global top-(H*base) over the flattened sorted
 * scores, per-head counts, cap_h = round(count*(1-floor) + int(base*floor)).
 * sorted_val: dtype [H][L] (from pkv_sort_rows).  Writes int32 head_capacity[H] (device).
 * ws: >= 1024 + 2*H*256*4 bytes.  H <= 256.  B must be 1 (:724). */
PKV_API int pkv_ada_budget(int32_t dtype, int32_t H, int32_t L, const void* sorted_val, int32_t base_capacity,
                   double floor_ratio, int32_t normalize, int32_t* head_capacity, void* ws,
                   size_t ws_bytes, pkv_stream_t stream);

/* The same budgets WITHOUT a full sort: one head can receive at most H*base entries of the global top-(H*base), so the
 * first M = min(L, H*base) entries of every head's descending order decide everything.  top_idx: int32 [H][idx_stride],
 * row h = pkv_topk(scores row h, k = M) (canonical order); scores: dtype [H][scores_stride], the un-sorted rows of length
 * L (the sum over all scores of :710 is taken from them).  M >= min(L, H*base) is checked.  Same ws as pkv_ada_budget.
 * head_lens / cu_klen (both or neither; device int32 [H] / [H+1]): when given, the var-len metadata of pkv_ada_metadata
 * for `window` is written by the same launch. */
PKV_API int pkv_ada_budget_topm(int32_t dtype, int32_t H, int32_t L, int32_t M, const void* scores, int64_t scores_stride,
                        const int32_t* top_idx, int64_t idx_stride, int32_t base_capacity, double floor_ratio,
                        int32_t normalize, int32_t window, int32_t* head_capacity, int32_t* head_lens, int32_t* cu_klen,
                        void* ws, size_t ws_bytes, pkv_stream_t stream);

/* The same budgets from the UN-SORTED score rows alone (no sort, no top-M list): what :706-719 consume of the order is, per
 * head, the sum of its `base` largest scores (:710) and how many of its adaptive scores lie above / at the global threshold
 * (:712-717) - selections and counts, computed by histograms over the whole row.  For H*base > 4096 (budget 2048), where
 * min(L, H*base) is the whole row.  scores: dtype [H][scores_stride], rows of length L <= 65536; PKV_F32 rows (L <= 32768;
 * 32-bit keys, four radix levels; ws >= 1024 + 4*H*256*4 + 4*H*4 bytes) are accepted here and nowhere else among the budget
 * entry points - an fp32 `sum()` ratio has no bit-level target (ATen's order depends on the host), see DESIGN.md section 5.  cu_headlens (optional,
 * int32 [H]): inclusive prefix of head_lens (:687).  host_mirror (optional): device-visible PINNED HOST uint64 [H], 8-byte
 * aligned: word h = host_seq << 32 | ran_out << 31 | cap_h, one system-scope store per head (0.2.0; before: int32 [H+1] with a
 * fence and a flag word) - the host polls until every word carries host_seq instead of copy + stream synchronise.
 * The gather then needs, per head, its first cap_h entries of the canonical order: pkv_topk with k_per_row = head_capacity. */
PKV_API int pkv_ada_budget_rows(int32_t dtype, int32_t H, int32_t L, const void* scores, int64_t scores_stride, int32_t base_capacity,
                        double floor_ratio, int32_t normalize, int32_t window, int32_t* head_capacity, int32_t* head_lens,
                        int32_t* cu_klen, int32_t* cu_headlens, uint64_t* host_mirror, int32_t host_seq, void* ws, size_t ws_bytes,
                        pkv_stream_t stream);

/* Head-sharded Ada-SnapKV: the budget of :712-717 couples ALL heads, so the ranks exchange one
 * thing - every head's ADAPTIVE list (:709-711: sorted scores x sum(top base)/sum(all), model dtype), first M entries.
 * lists_out: dtype [H][M] for this rank's H heads; after the all-gather every rank calls pkv_ada_budget(sorted_val = the
 * gathered lists, L = M, normalize = 0).  M >= min(S-w, H_total*base) keeps that exact (see pkv_ada_budget_topm). */
PKV_API int pkv_ada_adaptive_lists(int32_t dtype, int32_t H, int32_t L, int32_t M, const void* scores, int64_t scores_stride,
                           const int32_t* top_idx, int64_t idx_stride, int32_t base_capacity, int32_t normalize,
                           void* lists_out, void* ws, size_t ws_bytes, pkv_stream_t stream);

/* Fused front half of AdaKVCluster.update_kv / HeadKVCluster.update_kv (:674-731 / :808-852) in ONE call: window score
 * (d->reduce = PKV_REDUCE_MEAN, :661) -> top-M indices of every head (d->topk = M, canonical order) -> head budgets +
 * var-len metadata.  Ada-SnapKV: given_capacity = NULL, M >= min(S-w, H*base); writes head_capacity, head_lens, cu_klen.
 * Short lists (0.1.2): with a host_mirror, base <= M < min(S-w, H*base) is accepted as well.  The budgets are then exact
 * unless some head's list runs out at the global threshold; the kernel reports that in bit 31 of every mirror word
 * (word h = host_seq << 32 | ran_out << 31 | cap_h; host_seq >= 0) and the caller repeats the call with the full M.
 * (A head of a real prompt takes a few base budgets, not H of them: max(4 x base, 512) entries per head instead of H x base
 * cut the selection from 21 to 14 us at S = 32768, H = 32, base = 120.)  With lists that fit one workgroup (H x M <= 45 056)
 * the budget step is ONE launch: the selection leaves every head's adaptive list behind as 16-bit keys and a single
 * workgroup selects the global threshold (5 us against 19 us for the three launches of 0.1.x).
 * HeadKV: given_capacity = device int32 [H] (host-derived, :855), M >= max capacity; writes head_lens, cu_klen only.
 * The host then reads the capacities back (klen_sum / max_seqlen_k are Python ints at the boundary, :685-686; the
 * reference has the same sync at :718) and calls pkv_gather_flat(top_idx, idx_stride = M, ...).  ws: pkv_workspace_bytes(d). */
PKV_API int pkv_ada_select(const pkv_desc* d, const void* q, const void* k, int32_t base_capacity, double floor_ratio,
                   int32_t normalize, const int32_t* given_capacity, int32_t* top_idx, int32_t* head_capacity,
                   int32_t* head_lens, int32_t* cu_klen, int32_t* cu_headlens /* [H] inclusive prefix (:687), may be NULL */,
                   uint64_t* host_mirror /* may be NULL: device-visible PINNED HOST uint64 [H]; the budget kernel stores
                                            host_seq << 32 | ran_out << 31 | cap_h in word h (whole 64-bit stores, no fence):
                                            the host polls until every word carries host_seq instead of copying +
                                            synchronising */,
                   int32_t host_seq, void* ws, size_t ws_bytes, pkv_stream_t stream);

/* Var-len metadata (:682-698) from head_capacity: head_lens[H] = cap_h + w, cu_klen[H+1]
 * (exclusive prefix + total).  All device int32. */
PKV_API int pkv_ada_metadata(int32_t H, int32_t window, const int32_t* head_capacity, int32_t* head_lens,
                     int32_t* cu_klen, pkv_stream_t stream);

/* Flat gather (:733-757): for head h rows sorted_idx[h][0..cap_h) then the window tail, written at
 * row cu_klen[h] of the flat [sum_h(cap_h+w), D] outputs.  B must be 1.  d->topk, if > 0, is an upper
 * bound on max_h cap_h (sizes the launch); 0 = unknown (S-w).  out_rows = rows k_out / v_out hold (> 0: nothing is
 * stored at or beyond it - the outputs may be sized by a bound before the capacities are known on the host; 0 = not
 * checked). */
PKV_API int pkv_gather_flat(const pkv_desc* d, const void* k, const void* v, const int32_t* sorted_idx,
                    int64_t idx_stride, const int32_t* head_capacity, const int32_t* cu_klen,
                    void* k_out, void* v_out, int64_t out_rows, pkv_stream_t stream);

/* Decode-time flat-cache append (csrc/csrc/cuda_api.cu:11-85 update_flatten_view): out has
 * origin_rows + H rows; head h: copy head_lens[h] rows from cache row cu_klen[h] to out row
 * cu_klen[h]+h, then state[h] at out row cu_klen[h+1]+h.  head_dim elements of dtype per row. */
PKV_API int pkv_update_flatten_view(int32_t dtype, int32_t H, int32_t head_dim, const void* cache,
                            const void* state, const int32_t* head_lens, const int32_t* cu_klen,
                            void* out, pkv_stream_t stream);

/* Decode-time attention over the flat cache (llama_model.py:2377-2388: flash_attn_varlen_func(q, k_flat, v_flat, cu_qlen,
 * cu_klen, 1, max_seqlen_k, causal=True) at :2386, one query row per head; with one query row the causal mask hides
 * nothing).  Head h owns rows a = cu_klen[h] .. cu_klen[h+1] of k_flat / v_flat, n_h of them:
 *   s_j    = fp32(sum_d q[h,d] * k[a+j,d]) * scale     fp32 products and sums of the inputs as they are: no rounding to dtype
 *   out[h] = dtype(sum_j softmax_fp32(s)_j * v[a+j])   fp32 accumulator, ONE correctly rounded fp32 division by the fp32 sum of
 *                                                      the weights, ONE round-to-nearest-even to dtype; exp = the accurate one of
 *                                                      the window scores (pkv_debug_exp)
 *   lse[h] = max_j s_j + log(sum_j exp(s_j - max))     fp32 (the logarithm in fp64, rounded once)
 * A head with n_h = 0 gets zeros and lse = -inf, never NaN (the library's definition).  The order of the fp32 sums is the
 * library's own and a function of (head_dim, dtype, splits) and PKV_DECODE_CHUNK alone: two calls give the same bits, and
 * neither max_seqlen_k nor the other heads' lengths change a head's bits at equal `splits`.
 * Every head is walked in chunks of PKV_DECODE_CHUNK rows, chunk c belongs to split c % splits, the grid is (H, splits).
 * splits == 1: one launch.  splits > 1: the first launch leaves fp32 partials (max, sum, accumulator[head_dim]) per (head, split)
 * in ws, a second small launch merges them in split order (two launches, no hand-off between workgroups inside one).
 *   q:             dtype [H] rows of head_dim elements, q_stride ELEMENTS between heads (>= head_dim, keeps rows 16-byte aligned)
 *   k_flat/v_flat: dtype [sum_h n_h][head_dim] contiguous;  cu_klen: device int32 [H+1], non-decreasing
 *   max_seqlen_k:  >= 1; only picks the default split count - a head longer than it is still attended in full
 *   splits:        0 = pkv_decode_attn_splits(H, head_dim, max_seqlen_k), else 1 .. PKV_DECODE_MAX_SPLITS
 *   out:           dtype [H][head_dim] contiguous;  lse_out: float [H], may be NULL
 *   ws:            pkv_decode_attn_workspace_bytes(H, head_dim, splits) bytes (0 for splits == 1, ws may then be NULL)
 * Nothing outside out, lse_out and ws is written.  q, k_flat, v_flat, out, ws: 16-byte aligned.
 * PKV_ERR_DTYPE: dtype; PKV_ERR_SHAPE: H < 1, head_dim not in {64,128,256}, max_seqlen_k < 1, q_stride < head_dim, splits out of
 * range, a scale that is not finite; PKV_ERR_NULL; PKV_ERR_ALIGN: a pointer or q_stride breaks 16-byte rows; PKV_ERR_WORKSPACE.
 * All of them are answered before any HIP call.  Non-finite scores are outside the contract (a NaN score counts as -inf).
 * pkv_decode_attn_splits is host-only and a pure function of its arguments (no device query): about four workgroups per CU
 * of the 256-CU part, never more splits than ceil(max_seqlen_k / PKV_DECODE_CHUNK); >= 1, non-decreasing in max_seqlen_k;
 * an argument <= 0 gives 0. */
#define PKV_DECODE_CHUNK 128     /* rows per chunk: one batch of 16-byte loads of a 256-thread workgroup at 256-byte rows */
#define PKV_DECODE_MAX_SPLITS 64
PKV_API int pkv_decode_attn_splits(int32_t H, int32_t head_dim, int32_t max_seqlen_k);
PKV_API size_t pkv_decode_attn_workspace_bytes(int32_t H, int32_t head_dim, int32_t splits);
PKV_API int pkv_decode_attn_flat(int32_t dtype, int32_t H, int32_t head_dim, const void* q, int64_t q_stride /* elements between heads */,
                                 const void* k_flat, const void* v_flat, const int32_t* cu_klen /* device int32 [H+1] */,
                                 int32_t max_seqlen_k /* launch hint, >= 1 */, float scale, int32_t splits /* 0 = default */,
                                 void* out /* dtype [H][head_dim] contiguous */, float* lse_out /* [H], may be NULL */,
                                 void* ws, size_t ws_bytes, pkv_stream_t stream);

/* The same decode step over the ThinK cache (llama_model_think.py:175-195; the cache update_think and pkv_think_prune leave):
 * per head n_pruned keys that keep `kept` = Dk of their head_dim channels, then n_full full-width keys, and n_pruned + n_full
 * values.  With c_0 < c_1 < ... the channels of head h with keep[h][c] != 0, ascending:
 *   s_j = fp32(sum_{p < kept} q[h,c_p] * k_pruned[h,j,p]) * scale          j < n_pruned
 *   s_j = fp32(sum_{d < head_dim} q[h,d] * k_full[h,j - n_pruned,d]) * scale   j >= n_pruned
 *   out[h] = dtype(sum_j softmax_fp32(s)_j * v[h,j]),  lse[h]
 * with the rounding points of the flat-cache call above (products and sums of the inputs as they are, the accurate exp, ONE
 * correctly rounded fp32 division, ONE round-to-nearest-even to dtype, the logarithm of lse in fp64) and the sum of a score's
 * products taken in fp64 and rounded to fp32 ONCE before the multiplication by scale: s_j is the correctly rounded fp32 dot
 * product times scale.  n_pruned + n_full = 0 gives zeros and lse = -inf.  The mask is device data and not checked: the first `kept` set channels of a head are used, a
 * head with fewer meets the missing ones as a zero query, and no mask content makes the library read out of range.
 * Chunks of PKV_DECODE_CHUNK rows: first ceil(n_pruned / chunk) of pruned rows, then ceil(n_full / chunk) of full-width rows (a
 * chunk never straddles the two parts); chunk c belongs to split c % splits, the grid is (H, splits), splits > 1 adds the
 * combine launch over the same partials.  The order of every fp32 sum is a function of (head_dim, kept, dtype, splits) and
 * PKV_DECODE_CHUNK alone: two calls give the same bits.
 *   q:        dtype [H] rows of head_dim elements, q_stride ELEMENTS between heads
 *   keep:     uint8 [H][head_dim] contiguous, non-zero = kept (a torch bool mask as it is)
 *   k_pruned: dtype [H][n_pruned][kept] contiguous.  A row is kept * e bytes, so rows and head bases are not 16-byte aligned in
 *             general; the library fetches the 16-byte blocks that enclose the bytes it needs.  The base must be 16-byte
 *             aligned and the ALLOCATION must extend to the next 16-byte multiple behind the last element (every device
 *             allocator's granularity does that); what lies in those bytes does not matter.  May be NULL when n_pruned == 0.
 *   k_full:   dtype [H] heads of [n_full][head_dim] rows, k_full_stride ELEMENTS between heads; may be NULL when n_full == 0
 *   v:        dtype [H] heads of [n_pruned + n_full][head_dim] rows, v_stride ELEMENTS between heads
 *   splits:   0 = the flat-cache default for H heads of n_pruned + n_full rows (at least 1), else 1 .. PKV_DECODE_MAX_SPLITS
 *   out, lse_out, ws: as above; the workspace size is the flat-cache one for the same (H, head_dim, splits)
 * Nothing outside out, lse_out and ws is written.
 * PKV_ERR_DTYPE: dtype; PKV_ERR_SHAPE: H < 1, head_dim not in {64,128,256}, kept not in 1 .. head_dim, n_pruned < 0, n_full < 0,
 * a stride shorter than its rows, splits out of range, a scale that is not finite; PKV_ERR_NULL; PKV_ERR_ALIGN: q, k_full, v,
 * out, ws or one of the three strides breaks 16-byte rows, or k_pruned is not 16-byte aligned; PKV_ERR_WORKSPACE.  In that
 * order, all before any HIP call. */
PKV_API int pkv_decode_attn_think(int32_t dtype, int32_t H, int32_t head_dim, int32_t kept /* Dk */,
                                  const void* q, int64_t q_stride /* elements between heads */,
                                  const uint8_t* keep /* [H][head_dim], non-zero = kept: the cache's bool mask as it is */,
                                  const void* k_pruned /* dtype [H][n_pruned][kept] contiguous */, int32_t n_pruned,
                                  const void* k_full, int64_t k_full_stride /* elements between heads */, int32_t n_full,
                                  const void* v, int64_t v_stride /* dtype [H][n_pruned + n_full][head_dim], elements between heads */,
                                  float scale, int32_t splits /* 0 = default */, void* out, float* lse_out /* may be NULL */,
                                  void* ws, size_t ws_bytes, pkv_stream_t stream);

/* ---- multi-GPU: the one exchange step of the head-sharded path (the reference has no
 * collective: run_longbench.py:390 only places layers with device_map="auto") ----
 * Every rank holds idx_local int32 [B][H_local][k] (its heads, from pkv_compress); after the call every rank holds
 * idx_all int32 [B][nranks*H_local][k] (heads in rank order).  ONE ncclAllGather on `stream`; for B > 1 plus one small
 * regroup kernel (rank-major -> head-major), which needs ws >= nranks*B*H_local*k*4 bytes (ws may be NULL for B == 1).
 * nccl_comm is the caller's ncclComm_t (libpkv creates none and does not link RCCL: the entry points are taken from the
 * RCCL already loaded in the process - PyTorch's or the host's own; only a process without one gets the library named
 * by PKV_RCCL_LIB, else librccl.so.1: a process must hold ONE RCCL, two copies corrupt the heap at exit).
 * PyTorch does not expose its communicator, so the Python host issues the same collective through torch.distributed
 * (pyramidkv_amd/dist.py); a C/C++ host calls this. */
PKV_API int pkv_allgather_indices(void* nccl_comm, const int32_t* idx_local, int32_t* idx_all, int32_t B, int32_t H_local,
                          int32_t k, void* ws, size_t ws_bytes, pkv_stream_t stream);
PKV_API int pkv_last_nccl_error(void); /* ncclResult_t of the last PKV_ERR_COLLECTIVE on this thread */

/* ---- per-kernel device timing (hipEvent pairs on `stream`), used by bench.py ---- */
enum pkv_kernel_id {
  PKV_K_LOGITS = 0, PKV_K_FINALIZE = 1, PKV_K_TOPK = 2, PKV_K_GATHER = 3, PKV_K_H2O_STATS = 4,
  PKV_K_H2O_COLSUM = 5, PKV_K_SORT = 6, PKV_K_BUDGET = 7, PKV_K_L2NORM = 8, PKV_K_COUNT = 9
};
PKV_API int pkv_prof_enable(int on);                                   /* returns previous state */
PKV_API int pkv_prof_read(double* ms_sum, int64_t* launches, int reset); /* arrays of PKV_K_COUNT (9 since 0.2.4); syncs events */

/* ---- debug / test hooks (not part of the drop-in surface) ----
 * The trace hooks and the PKV_LOGITS_ABLATE measurement knob exist only in the -DPKV_DEBUG build (libpkv_debug.so,
 * `make -C pyramidkv_amd/csrc debug`); the release library returns PKV_ERR_UNSUPPORTED for a non-NULL buffer and
 * never reads the environment variable. */
PKV_API int pkv_debug_build(void);                    /* 1 = this library was built with -DPKV_DEBUG */
PKV_API int pkv_debug_topk_trace(void* device_u64x8); /* NULL disables; row 0 of every later top-k launch stamps 7 phase clocks */
PKV_API int pkv_debug_wg_trace(void* device_u64);     /* NULL disables; 2*262144 u64: per-workgroup (start,end) wall clock, 100 MHz */
/* Host-only route record of the last window-score call on this library (debug build; the release library answers
 * PKV_ERR_UNSUPPORTED).  Copies min(n, 16) int32 words to `out`:
 *   0 logits kernel (1 logits2_kernel, 2 logits_kernel, 3 the fp32 path)   1 instantiation (logits2: 0 window 8 / group 1,
 *   1 one 16-column tile, 2 two; logits: MFMA k-steps 2/4/8)   2 logits tile (logits_kernel: 128/256 keys)   3 > 64 KB LDS opt-in
 *   4 nst (logits2: 128-key stages per workgroup)   5 workgroups per head group (grid.x)   6 stages of the last workgroup
 *   7 window keys straddle a stage boundary   8 ... a workgroup boundary   9 logits store mode   10 finalize_kernel window
 *   constant (8, 32, 0 = run time)   11 positions per thread (4/8)   12 halo_spread   13 finalize blocks per row
 *   14 nontemporal K loads   15 hardware exp2 in the partial statistics.  Words that do not apply are 0. */
PKV_API int pkv_debug_score_route(int32_t* out, int n);
/* Route record of the last pkv_merge_compact on this library (debug build; the release library answers PKV_ERR_UNSUPPORTED).
 * Waits for the device, then copies min(n, 16) int32 words to `out`:
 *   0 drop-list kernel (2 merge_droplist2_kernel, 1 merge_droplist_kernel)   1 its grid   2 pivot kernel (2 merge_pivot2_kernel,
 *   1 merge_pivot_kernel, 3 merge_pivot_f32_kernel)   3 its KS (fp32: KSF)   4 pivot2: nontemporal row loads   5 pivot2: PF
 *   6 pivot2: nst (128-row stages per workgroup)   7 pivot grid (workgroups)   8 workgroups per head (grid.x)   9 pivot2: stages
 *   the last workgroup of a head would run over S rows   10 bucket fast path   11 bucket ranges (passes over the pivots)
 *   12 scatter workgroup size   13 scatter bitmap bytes   14 ntp (row pitch of the unit-norm kept keys)
 *   15 device flags: one bit per data-dependent path a merge kernel took (enum MergeFlag, pkv_kernels.hpp): 0 pivot2 signed-key
 *   loop finished a stage, 1 pivot2 redo, 2 pivot2 exact keys by NaN, 3 bf16 multiply form, 4 bf16 div_const form, 5 a prefetch
 *   was issued, 6 ragged workgroup, 7 workgroup past the drop list, 8 merge_pivot_kernel exact, 9 bucket fast, 10 bucket with
 *   more than one range, 11 scatter group of 0 rows, 12 of more than 2048 rows, 13 / 14 a 64-row block with a tail of 1..31 /
 *   33..63 rows, 15 a row whose maximum is zero was looked at again.  Words that do not apply are 0. */
PKV_API int pkv_debug_merge_route(int32_t* out, int n);
/* Route record of the last bf16 / fp16 H2O score call on this library (pkv_score_h2o, pkv_compress_h2o, pkv_select with h2o;
 * debug build; the release library answers PKV_ERR_UNSUPPORTED).  The fp32 form records nothing: after an fp32 call both hooks
 * still answer for the last 16-bit one.  Waits for the device, then copies min(n, 16) int32 words to `out`:
 *   0 dtype   1 KS (MFMA k-steps: head_dim / 32)   2, 3 grid of h2o_stats_kernel (x = 256-row workgroups per head, y = B*H)
 *   4, 5 grid of h2o_colsum_kernel   6 ntiles (64-key tiles per row)   7 t_plain (tiles that end at or before S - window)
 *   8 LDS bytes of pass 1   9 of pass 2   10 pass 1 asked for the > 64 KB LDS opt-in   11 pass 2 did
 *   12..15 workgroups of pass 1 by the path they took: frozen reference point / frozen and repeated with the tracked maximum
 *   after an overflow / tracked from the start (a row's first 16 logits span more than 40) / short prompt (t_plain == 0).
 * The record reads the workspace of that call: ask before the workspace is reused or freed. */
PKV_API int pkv_debug_h2o_route(int32_t* out, int n);
/* ... and its per-row results (host pointers): wg_route[n_wg] receives the path code of every pass-1 workgroup (1 frozen,
 * 2 repeat, 3 wide, 4 short; slot bh * grid.x + blockIdx.x, n_wg <= words 2 * 3 above), c_row[n_rows] the pass-1 output
 * c_row = -log2 sum_j exp(x_ij) of every query row ([B*H][S], n_rows <= B*H*S).  PKV_ERR_SHAPE for more than was recorded. */
PKV_API int pkv_debug_h2o_rows(int32_t* wg_route, int64_t n_wg, float* c_row, int64_t n_rows);
/* Test hooks of the RELEASE library (tests/test_gpu_parity.py): two element-wise kernels that expose device functions the
 * hot kernels inline - the accurate exp() of finalize_kernel and the fp32 -> dtype rounding of every rounding point - so
 * that the suite checks the shipped code, not a copy.  Nothing on the product path launches them (~2 KB of code). */
PKV_API int pkv_debug_exp(const float* in, float* out, int64_t n, pkv_stream_t stream);
PKV_API int pkv_debug_round(int32_t dtype, const float* in, void* out, int64_t n, pkv_stream_t stream);
/* ... and the fp32 square root the key-norm scan of pkv_compress_l2norm inlines (correctly rounded: tests/test_gpu_l2norm.py
 * compares it with the float64 square root, so a build flag that trades it for the bare hardware instruction fails there). */
PKV_API int pkv_debug_sqrt(const float* in, float* out, int64_t n, pkv_stream_t stream);
/* Test hook of the RELEASE library: "element / norm, rounded to the model dtype" of the LOOK-M merge in the three forms the merge
 * kernels inline (pkv_common.hpp: unit_div, unit_div_const, unit_mul), element-wise over n (x, norm) pairs of 16-bit values
 * (device pointers): out_div / out_divc / out_mul receive the rounded results, out_mul_ok[i] = 1 where merge_pivot2_kernel's
 * guard lets a lane take the multiply form (bf16 only takes it; the guard itself is dtype-blind). */
PKV_API int pkv_debug_unit_div(int32_t dtype, const void* x, const void* norm, void* out_div, void* out_divc, void* out_mul,
                               void* out_mul_ok, int64_t n, pkv_stream_t stream);
/* Host-only: the fp32 constant the bf16 / fp16 kernels multiply a logit by in place of "/ math.sqrt(head_dim)"
 * (pyramidkv_utils.py:317) for this dtype, head size and pkv_scale mode; tests/test_abi_and_host.py checks, over every finite
 * 16-bit input, that the multiply reproduces ATen's division ("div") / reciprocal multiply ("rcp") bit for bit. */
PKV_API float pkv_debug_scale_multiplier(int32_t dtype, int32_t D, int32_t scale_mode);

#ifdef __cplusplus
}
#endif
#endif /* PKV_H */
