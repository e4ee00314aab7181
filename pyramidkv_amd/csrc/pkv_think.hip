// pkv_think.hip — ThinK key-channel pruning (gfx950): a second pass over the keys update_kv has compacted.
//
//   think_scan_kernel     reference pyramidkv_utils.py:17-18  torch.pow(x, 2).mean(dim=2), the sums of it
//   think_select_kernel   :17-23  the means, queries_norm * keys_norm, topk(largest=False), the mask
//   think_compact_kernel  :26     kv_states[:, :, :seqlen - recent_size, :][~mask_k].reshape(1, -1, seqlen - recent_size, head_dim - k)
//
// The reference's drop is a boolean-mask index: a nonzero() with a host synchronisation in the middle of prefill.  Here the
// three launches go to the caller's stream and nothing comes back to the host.
//
// Rounding points (include/pkv.h pkv_think_prune).  Energy of a channel over n rows: every element is
// squared and the square rounded to the model dtype (what torch.pow gives in the model dtype; fp32: one rounded multiply, the
// build passes -ffp-contract=off), the rounded squares are summed in fp32 in THIS file's order, the sum gets one correctly
// rounded fp32 division by n and the quotient one rounding to the model dtype.  score = dtype(float(qe) * float(ke)).
// The order of the sum is fixed: a lane adds its rows in ascending order, the row slots of a workgroup are added in slot
// order, the chunks of a head in chunk order.  No atomics: two runs give the same bits.
//
// Roofline: HBM / MALL.  Per head the scan reads N*D*e bytes (+ min(32, S) query rows), the compaction reads R*D*e and
// writes R*(D - n_prune)*e; the select kernel touches a few KB.
#include "pkv_common.hpp"
#include "pkv_kernels.hpp"

#include <type_traits>

namespace pkv {

// ---- channel-energy scan ---------------------------------------------------------------------------------------------
// Geometry of l2norm_kernel: a row is CH = D*e/16 lanes x 16 B, 256 / CH row slots per workgroup, a lane keeps up to 8
// independent 16-byte loads in flight.  Where the norm scan reduces ALONG the row, this one reduces DOWN the rows: a lane
// owns one 16-byte column slice and carries one fp32 sum per channel of it.  blockIdx.x < nck: rows [x * 128, x * 128 + 128)
// of the compacted keys; blockIdx.x == nck: the last nq = min(32, S) query rows, through Q's strides.
template <int DT> __device__ __forceinline__ void add_rounded_squares(float* acc, const u32x4 d) {
  if constexpr (DT == 2) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float x = __uint_as_float(d[e]); const float sq = x * x; acc[e] += sq; }
  } else {
    typedef typename std::conditional<DT == 0, BF16, F16>::type T;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float lo = Elem<T>::to_f32((uint16_t)(d[e] & 0xffffu)), hi = Elem<T>::to_f32((uint16_t)(d[e] >> 16));
      const uint32_t w = round_pack2<T>(lo * lo, hi * hi);          // the squares (exact in fp32) rounded to the model dtype
      acc[2 * e] += Elem<T>::to_f32((uint16_t)(w & 0xffffu));
      acc[2 * e + 1] += Elem<T>::to_f32((uint16_t)(w >> 16));
    }
  }
}

template <int DT, int CH>
__global__ __launch_bounds__(256) void think_scan_kernel(ThinkParams p) {
  constexpr int SLOTS = 256 / CH;
  constexpr int EPC = DT == 2 ? 4 : 8;                   // elements per 16-byte slice
  constexpr int D = CH * EPC;
  constexpr int RPT = THINK_SCAN_ROWS / SLOTS < 8 ? THINK_SCAN_ROWS / SLOTS : 8;
  constexpr int NB = THINK_SCAN_ROWS / (SLOTS * RPT);    // batches of RPT loads per lane: 1, 1, 2, 4 for CH = 8, 16, 32, 64
  constexpr int ES = DT == 2 ? 4 : 2;
  __shared__ __attribute__((aligned(16))) float red[SLOTS * D];
  const int tid = threadIdx.x;
  const int chunk = tid % CH;
  const int slot = tid / CH;
  const int bh = blockIdx.y;
  const int ck = blockIdx.x;
  const char* src;
  int64_t row_bytes;
  int n;                                                 // rows of this workgroup (>= 1)
  if (ck == p.nck) {                                     // wave-uniform
    const int b = bh / p.H, h = bh - b * p.H;
    src = static_cast<const char*>(p.q) + ((int64_t)b * p.qs_b + (int64_t)h * p.qs_h + (int64_t)(p.S - p.nq) * p.qs_s) * ES;
    row_bytes = p.qs_s * ES;
    n = p.nq;
  } else {
    const int first = ck * THINK_SCAN_ROWS;
    src = static_cast<const char*>(p.kc) + ((int64_t)bh * p.N + first) * D * ES;
    row_bytes = (int64_t)D * ES;
    n = min(THINK_SCAN_ROWS, p.N - first);
  }
  src += chunk * 16;

  float acc[EPC];
#pragma unroll
  for (int e = 0; e < EPC; ++e) acc[e] = 0.f;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    if (nb * RPT * SLOTS >= n) break;                    // workgroup-uniform
    u32x4 d[RPT];
#pragma unroll
    for (int j = 0; j < RPT; ++j) {                      // one load instruction = SLOTS consecutive rows; rows at or beyond n
      const int r = min((nb * RPT + j) * SLOTS + slot, n - 1);      // re-read the last row (never out of bounds), not added
      d[j] = *reinterpret_cast<const u32x4*>(src + (int64_t)r * row_bytes);
    }
#pragma unroll
    for (int j = 0; j < RPT; ++j)
      if ((nb * RPT + j) * SLOTS + slot < n) add_rounded_squares<DT>(acc, d[j]);
  }
  float* mine = red + slot * D + chunk * EPC;
#pragma unroll
  for (int e = 0; e < EPC; e += 4) *reinterpret_cast<float4*>(mine + e) = make_float4(acc[e], acc[e + 1], acc[e + 2], acc[e + 3]);
  __syncthreads();
  if (tid < D) {
    float s = red[tid];
#pragma unroll
    for (int sl = 1; sl < SLOTS; ++sl) s += red[sl * D + tid];
    p.part[((int64_t)bh * (p.nck + 1) + ck) * D + tid] = s;
  }
}

// ---- select ----------------------------------------------------------------------------------------------------------
// One workgroup per (b, h), one channel per lane.  Channel c's rank = the number of channels ahead of it in (score ascending, index ascending), NaN
// behind +inf by index; the n_prune channels of lowest rank go.  The scores are products of two non-negative values, so an
// fp32 bit pattern orders them; -0 cannot occur but is folded onto +0 all the same.
__device__ __forceinline__ uint32_t think_key(float s) {
  if (s != s) return 0xffffffffu;
  if (s == 0.f) s = 0.f;
  const uint32_t u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <int DT>
__global__ __launch_bounds__(256) void think_select_kernel(ThinkParams p) {
  __shared__ __attribute__((aligned(16))) uint32_t key[256];
  __shared__ __attribute__((aligned(16))) uint8_t kept[256];
  const int c = threadIdx.x;                              // one channel per lane; lanes at or beyond D only wait at the barriers
  const int bh = blockIdx.x;
  const int D = p.D, W = D - p.nprune;
  const float* part = p.part + (int64_t)bh * (p.nck + 1) * D;
  if (c < D) {
    float ks = 0.f;                                       // chunk order; 8 independent loads in flight, added in sequence
    for (int c0 = 0; c0 < p.nck; c0 += 8) {
      float t[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) t[i] = part[(int64_t)min(c0 + i, p.nck - 1) * D + c];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (c0 + i < p.nck) ks += t[i];
    }
    const float km = ks / (float)p.N;                     // correctly rounded (no fast-math flag in the build)
    const float qm = part[(int64_t)p.nck * D + c] / (float)p.nq;
    float sc;
    if constexpr (DT == 2) {
      sc = qm * km;
      if (p.stats) {
        float* st = static_cast<float*>(p.stats) + (int64_t)bh * 3 * D + c;
        st[0] = qm; st[D] = km; st[2 * D] = sc;
      }
    } else {
      typedef typename std::conditional<DT == 0, BF16, F16>::type T;
      const uint16_t qe = Elem<T>::from_f32(qm), ke = Elem<T>::from_f32(km);
      const uint16_t sh = Elem<T>::from_f32(Elem<T>::to_f32(qe) * Elem<T>::to_f32(ke));   // the fp32 product is exact: one rounding
      sc = Elem<T>::to_f32(sh);
      if (p.stats) {
        uint16_t* st = static_cast<uint16_t*>(p.stats) + (int64_t)bh * 3 * D + c;
        st[0] = qe; st[D] = ke; st[2 * D] = sh;
      }
    }
    key[c] = think_key(sc);
  }
  __syncthreads();
  if (c < D) {
    const uint32_t mine = key[c];
    int rank = 0;
#pragma unroll 4
    for (int j = 0; j < D; j += 4) {                      // four keys per LDS read, the same address in every lane
      const uint4 o = *reinterpret_cast<const uint4*>(key + j);
      rank += (o.x < mine || (o.x == mine && j < c)) ? 1 : 0;
      rank += (o.y < mine || (o.y == mine && j + 1 < c)) ? 1 : 0;
      rank += (o.z < mine || (o.z == mine && j + 2 < c)) ? 1 : 0;
      rank += (o.w < mine || (o.w == mine && j + 3 < c)) ? 1 : 0;
    }
    const uint8_t kp = rank >= p.nprune ? 1 : 0;
    kept[c] = kp;
    p.keep[(int64_t)bh * D + c] = kp;
  }
  __syncthreads();
  if (c < D && kept[c]) {
    int pos = 0;                                          // kept channels below c: the 0 / 1 bytes, four per word
    const uint32_t* words = reinterpret_cast<const uint32_t*>(kept);
    const int full = c >> 2;
    for (int w = 0; w < full; ++w) pos += __popc(words[w]);
    pos += __popc(words[full] & ((1u << (8 * (c & 3))) - 1u));
    p.keep_idx[(int64_t)bh * W + pos] = c;               // exactly W channels are kept: pos < W
  }
}

// ---- channel compaction ----------------------------------------------------------------------------------------------
// Workgroup (x, bh) copies rows [x * TR, x * TR + TR) of head bh (TR = 16 KB of input rows), R = N - recent rows per head in
// all.  The rows go to LDS as they are (16-byte loads and LDS writes); the output of the tile is ONE contiguous span of
// nr * W elements of the output stream, which starts wherever the rows before it end: neither a row (W * e = 154 bytes) nor
// a head base is 16-byte aligned in general.  Every 16-byte aligned piece inside the span is assembled from LDS through
// keep_idx and written with one vector store; what lies before the first and behind the last boundary goes out element by
// element.  Nothing outside the span is written.
template <int ES>
__global__ __launch_bounds__(256) void think_compact_kernel(ThinkParams p) {
  typedef typename std::conditional<ES == 2, uint16_t, uint32_t>::type E;
  constexpr int EPV = 16 / ES;
  constexpr int NV = THINK_TILE_BYTES / 16 / 256;        // 16-byte loads per lane and tile
  __shared__ __attribute__((aligned(16))) unsigned char tile[THINK_TILE_BYTES];
  __shared__ uint16_t kidx[256];
  const int tid = threadIdx.x;
  const int bh = blockIdx.y;
  const int D = p.D, W = D - p.nprune;
  const int TR = THINK_TILE_BYTES / (D * ES);
  const int r0 = blockIdx.x * TR;
  const int nr = min(TR, p.R - r0);                      // >= 1 by the grid
  for (int j = tid; j < W; j += 256) kidx[j] = (uint16_t)p.keep_idx[(int64_t)bh * W + j];
  {
    const u32x4* src = reinterpret_cast<const u32x4*>(static_cast<const char*>(p.kc) + ((int64_t)bh * p.N + r0) * D * ES);
    const int nv = nr * (D * ES / 16);
    u32x4 t[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (tid + i * 256 < nv) t[i] = src[tid + i * 256];
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (tid + i * 256 < nv) reinterpret_cast<u32x4*>(tile)[tid + i * 256] = t[i];
  }
  __syncthreads();
  const E* rows = reinterpret_cast<const E*>(tile);
  char* out = static_cast<char*>(p.k_out) + ((int64_t)bh * p.R + r0) * W * ES;           // the span: [out, out + len)
  const int len = nr * W * ES;                                                            // <= THINK_TILE_BYTES
  const int mis = (int)(reinterpret_cast<uintptr_t>(out) & 15);                           // a multiple of ES
  const int head = mis ? min(16 - mis, len) : 0;                                          // bytes before the first boundary
  const int nvec = (len - head) / 16;
  const int tail0 = head + nvec * 16;                                                     // bytes; what follows is < 16 bytes
  for (int v = tid; v < nvec; v += 256) {
    const int o = (head + v * 16) / ES;                  // element of the span this piece starts with
    int row = o / W, j = o - row * W;
    u32x4 w = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < EPV; ++i) {
      const uint32_t x = rows[row * D + kidx[j]];
      if (++j == W) { j = 0; ++row; }
      if constexpr (ES == 2) {
        if (i & 1) w[i >> 1] |= x << 16; else w[i >> 1] = x;
      } else {
        w[i] = x;
      }
    }
    *reinterpret_cast<u32x4*>(out + head + v * 16) = w;
  }
  const int nh = head / ES, nt = (len - tail0) / ES;     // < EPV each
  if (tid < nh + nt) {
    const int o = tid < nh ? tid : tail0 / ES + (tid - nh);
    const int row = o / W, j = o - row * W;
    reinterpret_cast<E*>(out)[o] = rows[row * D + kidx[j]];
  }
}

hipError_t launch_think(int dtype, const ThinkParams& p, hipStream_t st) {
  const int BH = p.B * p.H;
  const int es = dtype == 2 ? 4 : 2;
  const int ch = p.D * es / 16;                          // 8, 16, 32 (16-bit) / 16, 32, 64 (fp32)
  const dim3 sgrid((unsigned)(p.nck + 1), (unsigned)BH);
#define PKV_TS(DT, C) hipLaunchKernelGGL((think_scan_kernel<DT, C>), sgrid, dim3(256), 0, st, p)
  if (dtype == 2) {
    if (ch == 16) PKV_TS(2, 16); else if (ch == 32) PKV_TS(2, 32); else PKV_TS(2, 64);
  } else if (dtype == 0) {
    if (ch == 8) PKV_TS(0, 8); else if (ch == 16) PKV_TS(0, 16); else PKV_TS(0, 32);
  } else {
    if (ch == 8) PKV_TS(1, 8); else if (ch == 16) PKV_TS(1, 16); else PKV_TS(1, 32);
  }
#undef PKV_TS
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (dtype == 2) hipLaunchKernelGGL(think_select_kernel<2>, dim3((unsigned)BH), dim3(256), 0, st, p);
  else if (dtype == 0) hipLaunchKernelGGL(think_select_kernel<0>, dim3((unsigned)BH), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(think_select_kernel<1>, dim3((unsigned)BH), dim3(256), 0, st, p);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const int tr = THINK_TILE_BYTES / (p.D * es);
  const dim3 cgrid((unsigned)((p.R + tr - 1) / tr), (unsigned)BH);
  if (es == 2) hipLaunchKernelGGL(think_compact_kernel<2>, cgrid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL(think_compact_kernel<4>, cgrid, dim3(256), 0, st, p);
  return hipGetLastError();
}

}  // namespace pkv
