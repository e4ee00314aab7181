// pkv_decode.hip — single-query attention over the flat var-len Ada-SnapKV / HeadKV cache and over the ThinK cache (gfx950).
//
//   decode_attn_kernel     reference llama_model.py:2377-2388  flash_attn_varlen_func(q, k_flat, v_flat, cu_qlen, cu_klen, 1,
//                          max_seqlen_k, causal=True): one query row per head over rows cu_klen[h] .. cu_klen[h+1] of the cache
//   decode_think_kernel    reference llama_model_think.py:175-195  the ThinK decode step: one query row per head over n_pruned
//                          keys that keep `kept` of their D channels (contiguous rows of kept elements), then n_full full-width keys
//   decode_combine_kernel  the second launch of the splits > 1 route of either: merges the per-(head, split) partials
//
// Rounding points (include/pkv.h pkv_decode_attn_flat).  s_j = fp32 dot product of the inputs as they
// are (no rounding to the model dtype) times `scale`; softmax in fp32 with the accurate pkv_exp; out = fp32 accumulator, ONE
// correctly rounded fp32 division by the fp32 sum of the weights, ONE round-to-nearest-even to the model dtype.
// The order of every fp32 sum is fixed by (head_dim, dtype, splits) and PKV_DECODE_CHUNK alone: a lane adds its rows in
// ascending order, the row slots of a wave are merged by a butterfly, the four waves in wave order, the splits in split order.
// Neither the launch hint max_seqlen_k nor the other heads' lengths enter it.  No atomics: two calls give the same bits.
// decode_think_kernel: the same, with (head_dim, kept, dtype, splits), and with one difference in the score: the products of a
// row's dot product (exact in fp64) are summed in fp64 and the sum is rounded to fp32 ONCE before it is multiplied by `scale`,
// where decode_attn_kernel rounds after every FMA.  With one or two rows lse IS a score, and an fp32 chain over 64 - 256 products
// sat 1 - 2 ulp of lse from float64; the fp64 sum, rounded once, is the correctly rounded fp32 dot product but for fp64's own rounding.  The order is fixed all
// the same: a pruned row's dot product is summed by TPR = 256 / TR
// lanes (TR = rows per staging tile, the largest power of two <= 128 whose rows fit DECODE_TILE_BYTES: a function of kept and the
// dtype), lane i adding the stored columns i, i + TPR, ... in ascending order, the TPR lanes merged by a butterfly.  From the
// scores on, pruned and full-width rows take the one path below: chunks never straddle the two parts, chunk c (pruned chunks
// first) belongs to split c % splits.
//
// Roofline: HBM / MALL.  The floor is reading K and V once, 2 * sum_h n_h * D * e bytes; q, out and the partials are H * D
// elements.  No MFMA: M = 1.  K / V rows go straight to registers with 16-byte loads (a row is CH = D*e/16 lanes, a wave covers
// 64 / CH rows per load instruction), up to 8 K and 8 V loads per lane in flight; nothing is staged in LDS.
// The pruned keys of decode_think_kernel are the exception: a row is kept * e bytes (154 at D = 128, ratio 0.4, 16-bit), so
// neither a row nor a head base is 16-byte aligned.  A tile of rows is ONE contiguous span; the 16-byte blocks that enclose it
// are fetched with aligned loads into LDS (the inverse of think_compact_kernel's stores) and the dot products read it there.
#include "../../include/pkv.h"
#include "pkv_common.hpp"
#include "pkv_kernels.hpp"

#include <type_traits>

namespace pkv {

// 16 bytes of the model dtype -> fp32 (exact)
template <int DT> __device__ __forceinline__ void decode_unpack(const u32x4 d, float* x) {
  if constexpr (DT == 2) {
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = __uint_as_float(d[e]);
  } else if constexpr (DT == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { x[2 * e] = __uint_as_float(d[e] << 16); x[2 * e + 1] = __uint_as_float(d[e] & 0xffff0000u); }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) { x[2 * e] = Elem<F16>::to_f32((uint16_t)(d[e] & 0xffffu)); x[2 * e + 1] = Elem<F16>::to_f32((uint16_t)(d[e] >> 16)); }
  }
}

template <int DT> __device__ __forceinline__ void decode_store(void* out, int64_t i, float x) {
  if constexpr (DT == 2) static_cast<float*>(out)[i] = x;
  else static_cast<uint16_t*>(out)[i] = Elem<typename std::conditional<DT == 0, BF16, F16>::type>::from_f32(x);
}

// max + log(sum): the logarithm is taken in fp64 and the sum rounded to fp32 once
__device__ __forceinline__ float decode_lse(float m, float l) { return (float)((double)m + log((double)l)); }

// ---- the ThinK kernel's pieces --------------------------------------------------------------------------------------------
// decode_chunk / decode_finish restate the chunk body and the end of decode_attn_kernel below for decode_think_kernel,
// operation for operation but for the fp64 sum of a row's dot product (file header).  decode_attn_kernel keeps its own inlined text: built from these functions it took more registers
// (bf16, D = 128: 126 -> 134 VGPRs, 4 -> 3 waves per SIMD), and sharing code must not cost the flat cache anything.
//
// One chunk of nr rows (1 .. PKV_DECODE_CHUNK) into the lane's running state.  A row is CH lanes x 16 bytes, the workgroup holds
// SLOTS = 256 / CH row slots; slot s takes rows s, s + SLOTS, ... of the chunk, RB of them per batch.  kb / vb: row 0 of the
// chunk at this lane's 16-byte column slice.  SC: the scores (already times `scale`) are in sc[0 .. nr) instead, kb is not read.
// pkv_exp gives +0 for -inf and for NaN, so a slot that has seen no row yet (m = -inf, m - m = NaN) needs no branch.
template <int DT, int CH, bool SC>
__device__ __forceinline__ void decode_chunk(const char* kb, const char* vb, const float* sc, const int nr, const int slot, const float* qf,
                                             const float scale, float& m, float& l, float* acc) {
  constexpr int EPC = DT == 2 ? 4 : 8;
  constexpr int ES = DT == 2 ? 4 : 2;
  constexpr int SLOTS = 256 / CH;
  constexpr int RPS = PKV_DECODE_CHUNK / SLOTS;          // rows per slot and chunk: 4, 8, 16, 32 for CH = 8, 16, 32, 64
  constexpr int RB = RPS < 8 ? RPS : 8;                  // ... per batch of loads
  constexpr int NB = RPS / RB;
  constexpr int64_t ROW = (int64_t)CH * EPC * ES;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (b * RB * SLOTS >= nr) break;                     // workgroup-uniform
    u32x4 kd[RB], vd[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) {                       // one load instruction = SLOTS consecutive rows; rows at or beyond nr
      const int r = min((b * RB + j) * SLOTS + slot, nr - 1);        // re-read the chunk's last row (never out of bounds), not used
      if constexpr (!SC) kd[j] = *reinterpret_cast<const u32x4*>(kb + r * ROW);
      vd[j] = *reinterpret_cast<const u32x4*>(vb + r * ROW);
    }
    float s[RB], bm = -INFINITY;
#pragma unroll
    for (int j = 0; j < RB; ++j) {
      if constexpr (SC) {
        const int r = (b * RB + j) * SLOTS + slot;
        s[j] = r < nr ? sc[r] : -INFINITY;
      } else {
        float x[EPC];
        double d = 0.0;                                   // products exact, sum in fp64: ONE rounding to fp32 below
        decode_unpack<DT>(kd[j], x);
#pragma unroll
        for (int e = 0; e < EPC; ++e) d = fma((double)qf[e], (double)x[e], d);
#pragma unroll
        for (int o = CH / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);       // all CH lanes of the row end with the same bits
        s[j] = (b * RB + j) * SLOTS + slot < nr ? (float)d * scale : -INFINITY;
      }
      bm = fmaxf(bm, s[j]);
    }
    const float mn = fmaxf(m, bm);
    const float w = pkv_exp(m - mn);
    l *= w;
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[e] *= w;
#pragma unroll
    for (int j = 0; j < RB; ++j) {
      const float pj = pkv_exp(s[j] - mn);
      if ((b * RB + j) * SLOTS + slot < nr) {
        float x[EPC];
        decode_unpack<DT>(vd[j], x);
        l += pj;
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[e] = fmaf(pj, x[e], acc[e]);
      }
    }
    m = mn;
  }
}

// The end of a workgroup that has seen at least one row: the row slots of a wave, the four waves, then out / lse (one split)
// or the (max, sum, accumulator) partial of (head, split).  red: 4 * (D + 4) floats of LDS.
template <int DT, int CH>
__device__ __forceinline__ void decode_finish(const DecodeParams& p, float* red, const int h, const int sp, const int nsp, float m, float l,
                                              float* acc) {
  constexpr int EPC = DT == 2 ? 4 : 8;
  constexpr int D = CH * EPC;
  constexpr int WS = D + 4;                              // floats one wave leaves in LDS: acc[D], m, l (+ 2: 16-byte rows)
  const int tid = threadIdx.x;
  const int chunk = tid % CH;
  // the row slots of a wave: butterfly over lane distance CH, 2 CH, ... 32
#pragma unroll
  for (int off = CH; off < 64; off <<= 1) {
    const float mo = __shfl_xor(m, off, 64), lo = __shfl_xor(l, off, 64);
    const float M = fmaxf(m, mo);
    const float wa = pkv_exp(m - M), wb = pkv_exp(mo - M);
    l = l * wa + lo * wb;
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[e] = acc[e] * wa + __shfl_xor(acc[e], off, 64) * wb;
    m = M;
  }
  // the four waves, through LDS, in wave order
  const int wave = tid >> 6, lane = tid & 63;
  if (lane < CH) {
#pragma unroll
    for (int e = 0; e < EPC; e += 4)
      *reinterpret_cast<float4*>(red + wave * WS + chunk * EPC + e) = make_float4(acc[e], acc[e + 1], acc[e + 2], acc[e + 3]);
    if (lane == 0) { red[wave * WS + D] = m; red[wave * WS + D + 1] = l; }
  }
  __syncthreads();
  if (tid < D) {
    float M = red[D];
#pragma unroll
    for (int w = 1; w < 4; ++w) M = fmaxf(M, red[w * WS + D]);          // finite: the workgroup has seen a row
    float L = 0.f, A = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float ww = pkv_exp(red[w * WS + D] - M);
      L += red[w * WS + D + 1] * ww;
      A += red[w * WS + tid] * ww;
    }
    if (nsp == 1) {
      decode_store<DT>(p.out, (int64_t)h * D + tid, A / L);
      if (tid == 0 && p.lse) p.lse[h] = decode_lse(M, L);
    } else {
      const int64_t ps = (int64_t)h * nsp + sp;
      p.part_acc[ps * D + tid] = A;
      if (tid == 0) { p.part_ml[2 * ps] = M; p.part_ml[2 * ps + 1] = L; }
    }
  }
}

// A workgroup without a chunk (workgroup-uniform): with one split the head is empty and gets zeros and lse = -inf here (the
// combine launch does it otherwise).
template <int DT, int D> __device__ __forceinline__ void decode_no_chunk(const DecodeParams& p, const int h, const int nsp) {
  if (nsp == 1) {
    if (threadIdx.x < D) decode_store<DT>(p.out, (int64_t)h * D + threadIdx.x, 0.f);
    if (threadIdx.x == 0 && p.lse) p.lse[h] = -INFINITY;
  }
}

// Workgroup (h, sp) walks chunks sp, sp + splits, ... of head h (PKV_DECODE_CHUNK rows each).  A row is CH lanes x 16 bytes,
// the workgroup holds SLOTS = 256 / CH row slots; slot s takes rows s, s + SLOTS, ... of a chunk, RB of them per batch.
// Every lane keeps the running (max, sum) of its slot and the fp32 accumulator of its own 16-byte column slice.
// pkv_exp gives +0 for -inf and for NaN, so a slot that has seen no row yet (m = -inf, m - m = NaN) needs no branch.
template <int DT, int CH>
__global__ __launch_bounds__(256) void decode_attn_kernel(DecodeParams p) {
  constexpr int EPC = DT == 2 ? 4 : 8;                   // elements per 16-byte slice
  constexpr int ES = DT == 2 ? 4 : 2;
  constexpr int D = CH * EPC;
  constexpr int SLOTS = 256 / CH;
  constexpr int RPS = PKV_DECODE_CHUNK / SLOTS;          // rows per slot and chunk: 4, 8, 16, 32 for CH = 8, 16, 32, 64
  constexpr int RB = RPS < 8 ? RPS : 8;                  // ... per batch of loads
  constexpr int NB = RPS / RB;
  constexpr int WS = D + 4;                              // floats one wave leaves in LDS: acc[D], m, l (+ 2: 16-byte rows)
  __shared__ __attribute__((aligned(16))) float red[4 * WS];
  const int tid = threadIdx.x;
  const int chunk = tid % CH;
  const int slot = tid / CH;
  const int h = blockIdx.x, sp = blockIdx.y, nsp = gridDim.y;
  const int a = p.cu_klen[h];
  const int n = p.cu_klen[h + 1] - a;
  if ((int64_t)sp * PKV_DECODE_CHUNK >= n) {             // no chunk of this head for this split (workgroup-uniform)
    if (nsp == 1) {                                      // an empty head: zeros and lse = -inf (the combine launch does it otherwise)
      if (tid < D) decode_store<DT>(p.out, (int64_t)h * D + tid, 0.f);
      if (tid == 0 && p.lse) p.lse[h] = -INFINITY;
    }
    return;
  }

  float qf[EPC];
  decode_unpack<DT>(*reinterpret_cast<const u32x4*>(static_cast<const char*>(p.q) + ((int64_t)h * p.q_stride + chunk * EPC) * ES), qf);
  const char* kb = static_cast<const char*>(p.k) + ((int64_t)a * D + chunk * EPC) * ES;
  const char* vb = static_cast<const char*>(p.v) + ((int64_t)a * D + chunk * EPC) * ES;
  constexpr int64_t ROW = (int64_t)D * ES;

  float m = -INFINITY, l = 0.f, acc[EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) acc[e] = 0.f;

  for (int64_t r0 = (int64_t)sp * PKV_DECODE_CHUNK; r0 < n; r0 += (int64_t)nsp * PKV_DECODE_CHUNK) {
    const int nr = (int)((int64_t)n - r0 < PKV_DECODE_CHUNK ? (int64_t)n - r0 : PKV_DECODE_CHUNK);   // rows of this chunk, >= 1
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (b * RB * SLOTS >= nr) break;                   // workgroup-uniform
      u32x4 kd[RB], vd[RB];
#pragma unroll
      for (int j = 0; j < RB; ++j) {                     // one load instruction = SLOTS consecutive rows; rows at or beyond nr
        const int r = min((b * RB + j) * SLOTS + slot, nr - 1);      // re-read the chunk's last row (never out of bounds), not used
        kd[j] = *reinterpret_cast<const u32x4*>(kb + (r0 + r) * ROW);
        vd[j] = *reinterpret_cast<const u32x4*>(vb + (r0 + r) * ROW);
      }
      float s[RB], bm = -INFINITY;
#pragma unroll
      for (int j = 0; j < RB; ++j) {
        float x[EPC], d = 0.f;
        decode_unpack<DT>(kd[j], x);
#pragma unroll
        for (int e = 0; e < EPC; ++e) d = fmaf(qf[e], x[e], d);
#pragma unroll
        for (int o = CH / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);       // all CH lanes of the row end with the same bits
        s[j] = (b * RB + j) * SLOTS + slot < nr ? d * p.scale : -INFINITY;
        bm = fmaxf(bm, s[j]);
      }
      const float mn = fmaxf(m, bm);
      const float sc = pkv_exp(m - mn);
      l *= sc;
#pragma unroll
      for (int e = 0; e < EPC; ++e) acc[e] *= sc;
#pragma unroll
      for (int j = 0; j < RB; ++j) {
        const float pj = pkv_exp(s[j] - mn);
        if ((b * RB + j) * SLOTS + slot < nr) {
          float x[EPC];
          decode_unpack<DT>(vd[j], x);
          l += pj;
#pragma unroll
          for (int e = 0; e < EPC; ++e) acc[e] = fmaf(pj, x[e], acc[e]);
        }
      }
      m = mn;
    }
  }

  // the row slots of a wave: butterfly over lane distance CH, 2 CH, ... 32
#pragma unroll
  for (int off = CH; off < 64; off <<= 1) {
    const float mo = __shfl_xor(m, off, 64), lo = __shfl_xor(l, off, 64);
    const float M = fmaxf(m, mo);
    const float wa = pkv_exp(m - M), wb = pkv_exp(mo - M);
    l = l * wa + lo * wb;
#pragma unroll
    for (int e = 0; e < EPC; ++e) acc[e] = acc[e] * wa + __shfl_xor(acc[e], off, 64) * wb;
    m = M;
  }
  // the four waves, through LDS, in wave order
  const int wave = tid >> 6, lane = tid & 63;
  if (lane < CH) {
#pragma unroll
    for (int e = 0; e < EPC; e += 4)
      *reinterpret_cast<float4*>(red + wave * WS + chunk * EPC + e) = make_float4(acc[e], acc[e + 1], acc[e + 2], acc[e + 3]);
    if (lane == 0) { red[wave * WS + D] = m; red[wave * WS + D + 1] = l; }
  }
  __syncthreads();
  if (tid < D) {
    float M = red[D];
#pragma unroll
    for (int w = 1; w < 4; ++w) M = fmaxf(M, red[w * WS + D]);          // finite: the workgroup has seen a row
    float L = 0.f, A = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float ww = pkv_exp(red[w * WS + D] - M);
      L += red[w * WS + D + 1] * ww;
      A += red[w * WS + tid] * ww;
    }
    if (nsp == 1) {
      decode_store<DT>(p.out, (int64_t)h * D + tid, A / L);
      if (tid == 0 && p.lse) p.lse[h] = decode_lse(M, L);
    } else {
      const int64_t ps = (int64_t)h * nsp + sp;
      p.part_acc[ps * D + tid] = A;
      if (tid == 0) { p.part_ml[2 * ps] = M; p.part_ml[2 * ps + 1] = L; }
    }
  }
}

// ThinK: head h has cp = ceil(n_pruned / C) chunks of pruned rows, then cf = ceil(n_full / C) chunks of full-width rows
// (C = PKV_DECODE_CHUNK); V row j belongs to score row j of the two parts laid end to end.
//   qp[0 .. kept)   the query at the head's first `kept` channels with keep != 0, ascending: a prefix count over the D mask
//                   bytes (one ballot per wave, the waves' counts through LDS).  A mask with fewer ones leaves zeros behind,
//                   one with more is cut: no mask content moves an index out of qp.
//   a pruned chunk  is walked in tiles of TR rows.  A tile is the contiguous span of ntr * kept elements that starts at
//                   element (h * n_pruned + row) * kept of k_pruned - 2- or 4-byte aligned, no more.  Lane t copies the
//                   16-byte blocks t, t + 256, ... that enclose the span (the first at or after k_pruned itself, the last
//                   within the 16-byte multiple the allocation extends to), so byte `off0 + i` of LDS is byte i of the span;
//                   bytes outside the span are copied and never read back.  TPR lanes then sum one row each against qp and
//                   leave score * scale in sc[row of the chunk]; decode_chunk takes the chunk from there with its V rows.
// LDS: tile 16 400 + qp 1 024 + sc 512 + red <= 4 160 + 16 bytes, all static.
template <int DT, int CH>
__global__ __launch_bounds__(256) void decode_think_kernel(DecodeParams p) {
  typedef typename std::conditional<DT == 2, uint32_t, uint16_t>::type E;
  constexpr int EPC = DT == 2 ? 4 : 8;
  constexpr int ES = DT == 2 ? 4 : 2;
  constexpr int D = CH * EPC;
  constexpr int C = PKV_DECODE_CHUNK;
  constexpr int64_t ROW = (int64_t)D * ES;
  __shared__ __attribute__((aligned(16))) unsigned char tile[DECODE_TILE_BYTES + 16];
  __shared__ __attribute__((aligned(16))) float red[4 * (D + 4)];
  __shared__ __attribute__((aligned(16))) float qp[256];
  __shared__ __attribute__((aligned(16))) float sc[C];
  __shared__ int wcnt[4];
  const int tid = threadIdx.x;
  const int chunk = tid % CH;
  const int slot = tid / CH;
  const int h = blockIdx.x, sp = blockIdx.y, nsp = gridDim.y;
  const int cp = (int)(((int64_t)p.n_pruned + C - 1) / C), cf = (int)(((int64_t)p.n_full + C - 1) / C);
  if (sp >= cp + cf) {
    decode_no_chunk<DT, D>(p, h, nsp);
    return;
  }

  float qf[EPC];
  decode_unpack<DT>(*reinterpret_cast<const u32x4*>(static_cast<const char*>(p.q) + ((int64_t)h * p.q_stride + chunk * EPC) * ES), qf);
  const int kept = p.kept;
  if (sp < cp) {                                         // this workgroup walks a pruned chunk (workgroup-uniform)
    const int wave = tid >> 6, lane = tid & 63;
    const bool on = tid < D && p.keep[(int64_t)h * D + tid] != 0;
    const unsigned long long b = __ballot(on);
    if (lane == 0) wcnt[wave] = __popcll(b);
    qp[tid] = 0.f;
    __syncthreads();
    int pos = __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += wcnt[w];
    if (on && pos < kept) {                              // kept <= D <= 256 = the size of qp
      const E x = static_cast<const E*>(p.q)[(int64_t)h * p.q_stride + tid];
      if constexpr (DT == 2) qp[pos] = __uint_as_float(x);
      else qp[pos] = Elem<typename std::conditional<DT == 0, BF16, F16>::type>::to_f32(x);
    }
    __syncthreads();
  }
  const int rowb = kept * ES;                            // bytes of a pruned row
  int ltpr = 1;                                          // TPR = 2 .. 16 lanes per row, TR = 256 / TPR = 128 .. 16 rows per tile
  while ((256 >> ltpr) * rowb > DECODE_TILE_BYTES) ++ltpr;
  const int TR = 256 >> ltpr, TPR = 1 << ltpr;
  const char* kfb = static_cast<const char*>(p.k) + ((int64_t)h * p.k_stride + chunk * EPC) * ES;
  const char* vb = static_cast<const char*>(p.v) + ((int64_t)h * p.v_stride + chunk * EPC) * ES;

  float m = -INFINITY, l = 0.f, acc[EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
  for (int c = sp; c < cp + cf; c += nsp) {
    if (c < cp) {
      const int r0 = c * C;
      const int nr = min(C, p.n_pruned - r0);            // >= 1
      for (int t0 = 0; t0 < nr; t0 += TR) {
        const int ntr = min(TR, nr - t0);
        const uintptr_t g0 = reinterpret_cast<uintptr_t>(p.k_pruned) + ((int64_t)h * p.n_pruned + r0 + t0) * rowb;
        const int off0 = (int)(g0 & 15);
        const u32x4* src = reinterpret_cast<const u32x4*>(g0 - off0);
        const int nv = (off0 + ntr * rowb + 15) >> 4;    // <= DECODE_TILE_BYTES / 16 + 1
        for (int v0 = 0; v0 < nv; v0 += 1024) {
          u32x4 t[4];
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (v0 + tid + i * 256 < nv) t[i] = src[v0 + tid + i * 256];
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (v0 + tid + i * 256 < nv) reinterpret_cast<u32x4*>(tile)[v0 + tid + i * 256] = t[i];
        }
        __syncthreads();
        const int row = tid >> ltpr, sub = tid & (TPR - 1);
        double d = 0.0;
        if (row < ntr) {
          const E* x = reinterpret_cast<const E*>(tile + off0 + row * rowb);
          for (int j = sub; j < kept; j += TPR) {
            if constexpr (DT == 2) d = fma((double)qp[j], (double)__uint_as_float(x[j]), d);
            else d = fma((double)qp[j], (double)Elem<typename std::conditional<DT == 0, BF16, F16>::type>::to_f32(x[j]), d);
          }
        }
        for (int o = TPR >> 1; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
        if (sub == 0 && row < ntr) sc[t0 + row] = (float)d * p.scale;
        __syncthreads();                                 // sc is complete; the tile may be overwritten
      }
      decode_chunk<DT, CH, true>(nullptr, vb + r0 * ROW, sc, nr, slot, qf, p.scale, m, l, acc);
    } else {
      const int r0 = (c - cp) * C;
      const int nr = min(C, p.n_full - r0);
      decode_chunk<DT, CH, false>(kfb + r0 * ROW, vb + ((int64_t)p.n_pruned + r0) * ROW, nullptr, nr, slot, qf, p.scale, m, l, acc);
    }
  }
  decode_finish<DT, CH>(p, red, h, sp, nsp, m, l, acc);
}

// One workgroup of D threads per head.  Chunk c belongs to split c % splits, so the splits that hold a chunk - the only ones
// whose partials were written - are 0 .. min(splits, chunks of the head) - 1; the others count as m = -inf, l = 0.
template <int DT>
__global__ __launch_bounds__(256) void decode_combine_kernel(DecodeParams p) {
  const int h = blockIdx.x, d = threadIdx.x;
  const int D = p.D, nsp = p.splits;
  int64_t chunks;                                        // flat cache: of the head's rows; ThinK: pruned chunks + full-width chunks
  if (p.cu_klen) {
    const int n = p.cu_klen[h + 1] - p.cu_klen[h];
    chunks = n > 0 ? ((int64_t)n + PKV_DECODE_CHUNK - 1) / PKV_DECODE_CHUNK : 0;
  } else {
    chunks = ((int64_t)p.n_pruned + PKV_DECODE_CHUNK - 1) / PKV_DECODE_CHUNK + ((int64_t)p.n_full + PKV_DECODE_CHUNK - 1) / PKV_DECODE_CHUNK;
  }
  const int have = (int)(chunks < nsp ? chunks : nsp);
  const float* ml = p.part_ml + (int64_t)h * nsp * 2;
  const float* pa = p.part_acc + (int64_t)h * nsp * D + d;
  float M = -INFINITY;
  for (int s = 0; s < have; ++s) M = fmaxf(M, ml[2 * s]);
  float L = 0.f, A = 0.f;
  for (int s = 0; s < have; ++s) {
    const float w = pkv_exp(ml[2 * s] - M);
    L += ml[2 * s + 1] * w;
    A += pa[(int64_t)s * D] * w;
  }
  decode_store<DT>(p.out, (int64_t)h * D + d, have ? A / L : 0.f);
  if (d == 0 && p.lse) p.lse[h] = have ? decode_lse(M, L) : -INFINITY;
}

hipError_t launch_decode_attn(int dtype, const DecodeParams& p, hipStream_t st) {
  const int ch = p.D * (dtype == 2 ? 4 : 2) / 16;        // 8, 16, 32 (16-bit) / 16, 32, 64 (fp32)
  const dim3 grid((unsigned)p.H, (unsigned)p.splits);
  const bool think = p.cu_klen == nullptr;               // the ThinK cache has no row table: pkv_decode_attn_think
#define PKV_DA(DT, C)                                                                              \
  do {                                                                                             \
    if (think) hipLaunchKernelGGL((decode_think_kernel<DT, C>), grid, dim3(256), 0, st, p);        \
    else hipLaunchKernelGGL((decode_attn_kernel<DT, C>), grid, dim3(256), 0, st, p);               \
  } while (0)
  if (dtype == 2) {
    if (ch == 16) PKV_DA(2, 16); else if (ch == 32) PKV_DA(2, 32); else PKV_DA(2, 64);
  } else if (dtype == 0) {
    if (ch == 8) PKV_DA(0, 8); else if (ch == 16) PKV_DA(0, 16); else PKV_DA(0, 32);
  } else {
    if (ch == 8) PKV_DA(1, 8); else if (ch == 16) PKV_DA(1, 16); else PKV_DA(1, 32);
  }
#undef PKV_DA
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || p.splits == 1) return e;
  if (dtype == 2) hipLaunchKernelGGL(decode_combine_kernel<2>, dim3((unsigned)p.H), dim3((unsigned)p.D), 0, st, p);
  else if (dtype == 0) hipLaunchKernelGGL(decode_combine_kernel<0>, dim3((unsigned)p.H), dim3((unsigned)p.D), 0, st, p);
  else hipLaunchKernelGGL(decode_combine_kernel<1>, dim3((unsigned)p.H), dim3((unsigned)p.D), 0, st, p);
  return hipGetLastError();
}

}  // namespace pkv
