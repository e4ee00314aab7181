// pkv_decode.hip — single-query attention over the flat var-len Ada-SnapKV / HeadKV cache (gfx950).
//
//   decode_attn_kernel     reference llama_model.py:2377-2388  flash_attn_varlen_func(q, k_flat, v_flat, cu_qlen, cu_klen, 1,
//                          max_seqlen_k, causal=True): one query row per head over rows cu_klen[h] .. cu_klen[h+1] of the cache
//   decode_combine_kernel  the second launch of the splits > 1 route: merges the per-(head, split) partials
//
// Rounding points (include/pkv.h pkv_decode_attn_flat).  s_j = fp32 dot product of the inputs as they
// are (no rounding to the model dtype) times `scale`; softmax in fp32 with the accurate pkv_exp; out = fp32 accumulator, ONE
// correctly rounded fp32 division by the fp32 sum of the weights, ONE round-to-nearest-even to the model dtype.
// The order of every fp32 sum is fixed by (head_dim, dtype, splits) and PKV_DECODE_CHUNK alone: a lane adds its rows in
// ascending order, the row slots of a wave are merged by a butterfly, the four waves in wave order, the splits in split order.
// Neither the launch hint max_seqlen_k nor the other heads' lengths enter it.  No atomics: two calls give the same bits.
//
// Roofline: HBM / MALL.  The floor is reading K and V once, 2 * sum_h n_h * D * e bytes; q, out and the partials are H * D
// elements.  No MFMA: M = 1.  K / V rows go straight to registers with 16-byte loads (a row is CH = D*e/16 lanes, a wave covers
// 64 / CH rows per load instruction), up to 8 K and 8 V loads per lane in flight; nothing is staged in LDS.
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

// One workgroup of D threads per head.  Chunk c belongs to split c % splits, so the splits that hold a chunk - the only ones
// whose partials were written - are 0 .. min(splits, chunks of the head) - 1; the others count as m = -inf, l = 0.
template <int DT>
__global__ __launch_bounds__(256) void decode_combine_kernel(DecodeParams p) {
  const int h = blockIdx.x, d = threadIdx.x;
  const int D = p.D, nsp = p.splits;
  const int n = p.cu_klen[h + 1] - p.cu_klen[h];
  const int64_t chunks = n > 0 ? ((int64_t)n + PKV_DECODE_CHUNK - 1) / PKV_DECODE_CHUNK : 0;
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
#define PKV_DA(DT, C) hipLaunchKernelGGL((decode_attn_kernel<DT, C>), grid, dim3(256), 0, st, p)
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
