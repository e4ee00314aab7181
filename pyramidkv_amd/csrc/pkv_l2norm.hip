// pkv_l2norm.hip — key-norm scan of the L2Norm policy (gfx950).
//
//   l2norm_kernel      reference pyramidkv_utils.py:419  token_norms = torch.norm(key_states, p=2, dim=-1)
//   idx_expand_kernel  the selection runs once per KV head (the policy never looks at Q); the gather reads one index row
//                      per query head
//
// The policy keeps the max_capacity_prompt keys of SMALLEST norm in ascending-norm order (:420-427).  "Norm ascending, index
// ascending" is the canonical top-k order (value descending, index ascending) of the NEGATED norm, so this kernel writes
// -norm into a score row and the existing selection does the rest (pkv_api.hip pkv_compress_l2norm).
//
// Rounding points (measured against torch.norm on bf16 / fp16 / fp32): fp32 sum of squares (the order
// of the sum is this kernel's own: 8 or 4 elements per lane in sequence, then a butterfly over the lanes of the row),
// correctly rounded fp32 sqrt, ONE round-to-nearest-even to the model dtype.  The squares of 16-bit elements are exact in
// fp32.  Sums beyond the fp32 range give +inf like the reference's; squares below it vanish like the reference's.
// The score row gets: -norm; +0 for a zero norm (never -0); -inf for a NaN norm, so that a NaN is ordered with +inf norms,
// by index (the reference puts NaN behind +inf; outside the parity contract).
//
// Pure streaming read.  Roofline: HBM.  Algorithmic bytes per call  B * Hkv * S * D * e  read,  B * Hkv * S * e  written
// (twice with norm_out).  Geometry of gather_kernel: a row is CH = D*e/16 lanes x 16 B, 256 / CH rows per load instruction
// and workgroup, every lane keeps L2_RPT = 8 independent 16-B nontemporal loads in flight.  A lane's 8 rows are CONSECUTIVE
// (row = block + slot * 8 + j): the first lane of a slot ends up with 8 consecutive results = one 16-byte store.
#include "pkv_common.hpp"
#include "pkv_kernels.hpp"

#include <type_traits>

namespace pkv {

constexpr int L2_RPT = 8;

// sqrt as the kernel takes it: hipcc's default keeps fp32 sqrt correctly rounded (the Makefile passes no fast-math flag);
// pkv_debug_sqrt runs this function element-wise and tests/test_gpu_l2norm.py compares it with the float64 square root
__device__ __forceinline__ float pkv_sqrt_rn(float x) { return __builtin_sqrtf(x); }

template <int CTRL> __device__ __forceinline__ float dpp_xadd(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// sum over the CH lanes of a row slot (CH = 8 .. 64, slots aligned to CH lanes), the same value in every lane: DPP inside
// the 16-lane rows (lane ^ 1, lane ^ 2, half mirror, mirror: every step adds two equal-sized partial sums, a + b == b + a),
// one / two cross-row steps for rows of 32 / 64 lanes
template <int CH> __device__ __forceinline__ float slot_sum(float v) {
  v = dpp_xadd<0xB1>(v);                    // quad_perm [1,0,3,2]
  v = dpp_xadd<0x4E>(v);                    // quad_perm [2,3,0,1]
  v = dpp_xadd<0x141>(v);                   // row_half_mirror: 8 lanes
  if (CH >= 16) v = dpp_xadd<0x140>(v);     // row_mirror: 16 lanes
  if (CH >= 32) v += __shfl_xor(v, 16, 64);
  if (CH >= 64) v += __shfl_xor(v, 32, 64);
  return v;
}

// DT: 0 bf16, 1 fp16, 2 fp32 (pkv_dtype)
template <int DT> __device__ __forceinline__ float chunk_sumsq(const u32x4 d) {
  float a = 0.f;
  if constexpr (DT == 2) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float x = __uint_as_float(d[e]); a = fmaf(x, x, a); }
  } else {
    typedef typename std::conditional<DT == 0, BF16, F16>::type T;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float lo = Elem<T>::to_f32((uint16_t)(d[e] & 0xffffu)), hi = Elem<T>::to_f32((uint16_t)(d[e] >> 16));
      a = fmaf(lo, lo, a);
      a = fmaf(hi, hi, a);
    }
  }
  return a;
}

template <int DT, int CH>
__global__ __launch_bounds__(256) void l2norm_kernel(L2NormParams p) {
  constexpr int SLOTS = 256 / CH;
  constexpr int ROWS = SLOTS * L2_RPT;
  const int tid = threadIdx.x;
  const int chunk = tid % CH;
  const int slot = tid / CH;
  const int bh = blockIdx.x / p.nblk;                   // b * Hkv + hk
  const int blk = blockIdx.x - bh * p.nblk;
  const int b = bh / p.Hkv;
  const int hk = bh - b * p.Hkv;
  const int r0 = blk * ROWS + slot * L2_RPT;            // this lane's first row (a multiple of 8)
  constexpr int EPC = DT == 2 ? 4 : 8;                  // elements per 16-byte chunk
  const int64_t base = (int64_t)b * p.ks_b + (int64_t)hk * p.ks_h + chunk * EPC;
  const int last = p.S - 1;

  // rows at or beyond S re-read the last row (never out of bounds); their results land in the padding of the score row:
  // live copies of row S-1's value, not a neutral one - every reader of the row masks by L = S (L2NormParams)
  u32x4 d[L2_RPT];
#pragma unroll
  for (int j = 0; j < L2_RPT; ++j) {
    const int r = min(r0 + j, last);
    if constexpr (DT == 2)
      d[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(reinterpret_cast<const float*>(p.kptr) + base + (int64_t)r * p.ks_s));
    else
      d[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(reinterpret_cast<const uint16_t*>(p.kptr) + base + (int64_t)r * p.ks_s));
  }
  float n[L2_RPT];
#pragma unroll
  for (int j = 0; j < L2_RPT; ++j) n[j] = slot_sum<CH>(chunk_sumsq<DT>(d[j]));
  if (chunk != 0 || r0 >= p.S) return;
#pragma unroll
  for (int j = 0; j < L2_RPT; ++j) n[j] = pkv_sqrt_rn(n[j]);

  if constexpr (DT == 2) {
    u32x4 pos[2], neg[2];
#pragma unroll
    for (int j = 0; j < L2_RPT; ++j) {
      const float x = n[j];
      pos[j >> 2][j & 3] = __float_as_uint(x);
      neg[j >> 2][j & 3] = x != x ? 0xff800000u : (x == 0.f ? 0u : __float_as_uint(x) ^ 0x80000000u);
    }
    float* so = reinterpret_cast<float*>(p.neg_out) + (int64_t)bh * p.Lp + r0;          // Lp % 8 == 0: the padding holds rows S..Lp-1
    *reinterpret_cast<u32x4*>(so) = neg[0];
    *reinterpret_cast<u32x4*>(so + 4) = neg[1];
    if (p.norm_out) {
      float* no = reinterpret_cast<float*>(p.norm_out) + (int64_t)bh * p.S + r0;
      if (p.norm_vec) {                                  // S % 8 == 0 and a 16-byte aligned buffer
        *reinterpret_cast<u32x4*>(no) = pos[0];
        *reinterpret_cast<u32x4*>(no + 4) = pos[1];
      } else {
#pragma unroll
        for (int j = 0; j < L2_RPT; ++j)
          if (r0 + j < p.S) no[j] = n[j];
      }
    }
  } else {
    typedef typename std::conditional<DT == 0, BF16, F16>::type T;
    u32x4 pos, neg;
    uint16_t h[L2_RPT];
#pragma unroll
    for (int j = 0; j < L2_RPT; j += 2) {
      const uint32_t w = round_pack2<T>(n[j], n[j + 1]);                                // the one rounding to the model dtype
      h[j] = (uint16_t)(w & 0xffffu);
      h[j + 1] = (uint16_t)(w >> 16);
      uint32_t ng = 0;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const uint16_t x = h[j + e];
        const uint16_t y = Elem<T>::is_nan(x) ? Elem<T>::neg_inf() : (x == 0 ? (uint16_t)0 : (uint16_t)(x ^ 0x8000u));
        ng |= (uint32_t)y << (16 * e);
      }
      pos[j >> 1] = w;
      neg[j >> 1] = ng;
    }
    uint16_t* so = reinterpret_cast<uint16_t*>(p.neg_out) + (int64_t)bh * p.Lp + r0;
    *reinterpret_cast<u32x4*>(so) = neg;
    if (p.norm_out) {
      uint16_t* no = reinterpret_cast<uint16_t*>(p.norm_out) + (int64_t)bh * p.S + r0;
      if (p.norm_vec) {
        *reinterpret_cast<u32x4*>(no) = pos;
      } else {
#pragma unroll
        for (int j = 0; j < L2_RPT; ++j)
          if (r0 + j < p.S) no[j] = h[j];
      }
    }
  }
}

hipError_t launch_l2norm(int dtype, const L2NormParams& p0, hipStream_t st) {
  L2NormParams p = p0;
  const int ch = p.D * (dtype == 2 ? 4 : 2) / 16;            // 8, 16, 32 (16-bit) / 16, 32, 64 (fp32)
  const int rows = (256 / ch) * L2_RPT;
  p.nblk = (p.S + rows - 1) / rows;
  p.norm_vec = p.norm_out && (p.S & 7) == 0 && (reinterpret_cast<uintptr_t>(p.norm_out) & 15) == 0 ? 1 : 0;
  const int64_t nwg = (int64_t)p.nblk * p.B * p.Hkv;
  if (nwg > 0x7fffffff) return hipErrorInvalidValue;
  dim3 grid((unsigned)nwg);
#define PKV_L2(DT, C) PKV_KLAUNCH((l2norm_kernel<DT, C>), grid, dim3(256), 0, st, p)
  if (dtype == 2) {
    if (ch == 16) PKV_L2(2, 16); else if (ch == 32) PKV_L2(2, 32); else PKV_L2(2, 64);
  } else if (dtype == 0) {
    if (ch == 8) PKV_L2(0, 8); else if (ch == 16) PKV_L2(0, 16); else PKV_L2(0, 32);
  } else {
    if (ch == 8) PKV_L2(1, 8); else if (ch == 16) PKV_L2(1, 16); else PKV_L2(1, 32);
  }
#undef PKV_L2
  return hipGetLastError();
}

// dst[bh][0..n) = src[bh / G][0..n): the index rows of a KV head, once per query head of its group (bh = b * H + h and
// G divides H, so bh / G = b * Hkv + h / G)
__global__ __launch_bounds__(256) void idx_expand_kernel(const int32_t* src, int64_t src_stride, int32_t* dst, int n, int G) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int bh = blockIdx.y;
  if (i < n) dst[(int64_t)bh * n + i] = src[(int64_t)(bh / G) * src_stride + i];
}

hipError_t launch_idx_expand(const int32_t* src, int64_t src_stride, int32_t* dst, int BH, int n, int G, hipStream_t st) {
  hipLaunchKernelGGL(idx_expand_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)BH), dim3(256), 0, st, src, src_stride, dst, n, G);
  return hipGetLastError();
}

__global__ void debug_sqrt_kernel(const float* in, float* out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = pkv_sqrt_rn(in[i]);
}
hipError_t launch_debug_sqrt(const float* in, float* out, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL(debug_sqrt_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, out, n);
  return hipGetLastError();
}

}  // namespace pkv
