// Pairwise product + SimpleClassifier (nnue.py:660-666, :713-738) forward and backward on gfx950.
//
//   l0 = pairwise ? cat(x[:, :h] * x[:, h:], x[:, :h]) : x           (h = L1/2; never materialised)
//   h1 = act(l0 W1^T + b1)   h2 = act(h1 W2^T + b2)   logits = h2 W3^T + b3
//
// Only the L1-wide layer is a real contraction (B x L1 x L2; 134 MFLOP at B=512, 1024 -> 128).  It
// runs on the f32 MFMA (v_mfma_f32_16x16x4_f32, exact fp32 products, fp32 accumulate) when the
// shape allows (L1 % 32 == 0, L2 % 16 == 0), split over K so that >= 512 waves are in flight, and
// on plain-VALU "simple" kernels otherwise.  The two narrow layers (L2 -> L3 -> C) are a per-sample
// tail kernel working out of LDS.  Split-K partials are summed in fixed order: reproducible.
#include <type_traits>
#include <tuple>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "small_wgrad.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// ReLU, or clamp(0, clip) when clip > 0, keeping a NaN as torch.relu / torch.clamp do (fmaxf / fminf would drop it)
__device__ __forceinline__ float act_fn(float z, float clip) {
  const float r = z <= 0.0f ? 0.0f : z;
  return (clip > 0.0f && r > clip) ? clip : r;
}
// d passed back through act_fn where it produced h, as torch's autograd does: relu's gradient is blocked only where
// h <= 0 (a NaN h passes it), clamp's is kept only inside the range (a NaN h blocks it).  A select, not a product, so a
// blocked NaN gradient becomes 0 as in torch.  (torch's clamp also passes the gradient at z == 0 and z == clip.)
__device__ __forceinline__ float gate_fn(float d, float h, float clip) {
  if (clip > 0.0f) return (h > 0.0f && h < clip) ? d : 0.0f;
  return h <= 0.0f ? 0.0f : d;
}

// element k of the (virtual) l0 row built from x row `xr`
__device__ __forceinline__ float l0_at(const float* __restrict__ xr, int k, int half, int pairwise) {
  if (!pairwise) return xr[k];
  return k < half ? xr[k] * xr[k + half] : xr[k - half];
}

// ------------------------------------------------------------------ layer 1, any shape
// wave per output (b, j): lanes stride over K; pre-activation, bias not yet added.
__global__ __launch_bounds__(256) void l1_forward_simple(const float* __restrict__ x, int pairwise,
                                                         const float* __restrict__ w1, int B, int L1, int L2,
                                                         float* __restrict__ part, Buckets bk) {
  const long long o = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (o >= (long long)B * L2) return;
  const int b = (int)(o / L2), j = (int)(o - (long long)b * L2);
  const int lane = threadIdx.x & 63, half = L1 / 2;
  const float* __restrict__ xr = x + (size_t)b * L1;
  const float* __restrict__ wr = w1 + ((size_t)(bk.bucket ? bk.bucket[b] : 0) * L2 + j) * L1;
  float acc = 0.f;
  for (int k = lane; k < L1; k += 64) acc = fmaf(l0_at(xr, k, half, pairwise), wr[k], acc);
  acc = wave_sum(acc);
  if (lane == 0) part[o] = acc;
}

// d_w1[i, j] = sum_b d_z1[b, i] * l0[b, j]; thread per (i, j)
__global__ __launch_bounds__(256) void l1_backward_w_simple(const float* __restrict__ x, int pairwise,
                                                            const float* __restrict__ d_z1, int B, int L1, int L2,
                                                            float* __restrict__ d_w1, Buckets bk) {
  const int i = blockIdx.x % L2, kb = blockIdx.x / L2;  // grid.x = K * L2
  const int j = blockIdx.y * 256 + threadIdx.x;
  if (j >= L1) return;
  const int half = L1 / 2;
  float acc = 0.f;
  if (bk.rows) {  // the samples of bucket kb, ascending
    for (int g = bk.seg[kb]; g < bk.seg[kb + 1]; ++g) {
      const int b = bk.rows[g];
      if (b >= 0) acc = fmaf(d_z1[(size_t)b * L2 + i], l0_at(x + (size_t)b * L1, j, half, pairwise), acc);
    }
  } else {
    for (int b = 0; b < B; ++b) acc = fmaf(d_z1[(size_t)b * L2 + i], l0_at(x + (size_t)b * L1, j, half, pairwise), acc);
  }
  d_w1[((size_t)kb * L2 + i) * L1 + j] = acc;
}

// d_l0 = d_z1 W1, then the pairwise block's own backward; thread per (b, j)
__global__ __launch_bounds__(256) void l1_backward_x_simple(const float* __restrict__ x, int pairwise,
                                                            const float* __restrict__ w1,
                                                            const float* __restrict__ d_z1, int B, int L1, int L2,
                                                            float* __restrict__ d_x, Buckets bk) {
  const int b = blockIdx.x;
  const int j = blockIdx.y * 256 + threadIdx.x;
  const int half = L1 / 2;
  const float* __restrict__ dz = d_z1 + (size_t)b * L2;
  if (bk.bucket) w1 += (size_t)bk.bucket[b] * L2 * L1;
  if (pairwise) {
    if (j >= half) return;
    float lo = 0.f, hi = 0.f;
    for (int k = 0; k < L2; ++k) {
      lo = fmaf(dz[k], w1[(size_t)k * L1 + j], lo);
      hi = fmaf(dz[k], w1[(size_t)k * L1 + j + half], hi);
    }
    const float* __restrict__ xr = x + (size_t)b * L1;
    d_x[(size_t)b * L1 + j] = fmaf(lo, xr[j + half], hi);
    d_x[(size_t)b * L1 + j + half] = lo * xr[j];
  } else {
    if (j >= L1) return;
    float acc = 0.f;
    for (int k = 0; k < L2; ++k) acc = fmaf(dz[k], w1[(size_t)k * L1 + j], acc);
    d_x[(size_t)b * L1 + j] = acc;
  }
}

// ------------------------------------------------------------------ layer 1 on the f32 MFMA
// Lane map of v_mfma_f32_16x16x4_f32: lane l = 16*q + r supplies A[row r][k q] and B[k q][col r];
// accumulator register t holds D[row 4*q + t][col r].
//
// Forward ("NT": both operands contiguous along K).  A wave owns a 16-sample x 64-unit tile and a
// K slice.  Each lane loads float4 along K, i.e. K elements kb + 4q .. 4q+3, and MFMA step t uses
// element t on BOTH operands -- a permutation of the K order, which a sum does not care about.
constexpr int kFwdTileN = 4;  // 16x16 tiles along L2 per wave

__global__ __launch_bounds__(256) void l1_forward_mfma(const float* __restrict__ x, int pairwise,
                                                       const float* __restrict__ w1, int B, int L1, int L2,
                                                       int ksplit, float* __restrict__ part, Buckets bk) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, q = lane >> 4;
  const int n_groups = (L2 + 16 * kFwdTileN - 1) / (16 * kFwdTileN);
  const int m_tiles = bk.rows ? bk.tiles : (B + 15) / 16;
  long long wid = (long long)blockIdx.x * 4 + wave;
  if (wid >= (long long)m_tiles * n_groups * ksplit) return;
  const int ks = (int)(wid % ksplit);
  wid /= ksplit;
  const int ng = (int)(wid % n_groups);
  const int mt = (int)(wid / n_groups);
  const int klen = L1 / ksplit;  // multiple of 16, inside one half when pairwise (ksplit even)
  const int k_lo = ks * klen;
  const int half = L1 / 2;
  int row = mt * 16 + r;
  int orow[4];  // sample behind accumulator register e (row 4 q + e of the tile)
#pragma unroll
  for (int e = 0; e < 4; ++e) orow[e] = mt * 16 + 4 * q + e;
  if (bk.rows) {  // a tile of one bucket: its rows are samples gathered by the grouping, its weights that bucket's
    const int kb = bk.tile_bucket[mt];  // wave-uniform
    if (kb < 0) return;
    w1 += (size_t)kb * L2 * L1;
    row = bk.rows[row];
#pragma unroll
    for (int e = 0; e < 4; ++e) orow[e] = bk.rows[orow[e]];
  }
  const bool row_ok = row >= 0 && row < B;
  const float* __restrict__ xr = x + (size_t)(row_ok ? row : 0) * L1;
  // pairwise: first half of l0 = x[k] * x[k + half]; second half = x[k - half]
  const bool prod = pairwise && k_lo < half;
  const int xoff = (pairwise && !prod) ? -half : 0;

  f32x4 acc[kFwdTileN];
#pragma unroll
  for (int t = 0; t < kFwdTileN; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float* wrow[kFwdTileN];
  bool col_ok[kFwdTileN];
#pragma unroll
  for (int t = 0; t < kFwdTileN; ++t) {
    const int col = (ng * kFwdTileN + t) * 16 + r;
    col_ok[t] = col < L2;
    wrow[t] = w1 + (size_t)(col_ok[t] ? col : 0) * L1;
  }
  // software pipeline: the operands of K block i+1 are requested before the MFMAs of block i issue
  auto load_a = [&](int kb) {
    const int k = kb + 4 * q;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row_ok) {
      a = *reinterpret_cast<const float4*>(xr + k + xoff);
      if (prod) {
        const float4 a2 = *reinterpret_cast<const float4*>(xr + k + half);
        a.x *= a2.x; a.y *= a2.y; a.z *= a2.z; a.w *= a2.w;
      }
    }
    return a;
  };
  auto load_b = [&](int kb, int t) {
    return col_ok[t] ? *reinterpret_cast<const float4*>(wrow[t] + kb + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  const int k_hi = k_lo + klen;
  float4 a = load_a(k_lo), bv[kFwdTileN];
#pragma unroll
  for (int t = 0; t < kFwdTileN; ++t) bv[t] = load_b(k_lo, t);
  for (int kb = k_lo; kb < k_hi; kb += 16) {
    const int kn = kb + 16 < k_hi ? kb + 16 : kb;  // last iteration re-reads its own block (harmless)
    const float4 an = load_a(kn);
    float4 bn[kFwdTileN];
#pragma unroll
    for (int t = 0; t < kFwdTileN; ++t) bn[t] = load_b(kn, t);
#pragma unroll
    for (int t = 0; t < kFwdTileN; ++t) {
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bv[t].x, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bv[t].y, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bv[t].z, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bv[t].w, acc[t], 0, 0, 0);
    }
    a = an;
#pragma unroll
    for (int t = 0; t < kFwdTileN; ++t) bv[t] = bn[t];
  }
  float* __restrict__ out = part + (size_t)ks * B * L2;
#pragma unroll
  for (int t = 0; t < kFwdTileN; ++t) {
    const int col = (ng * kFwdTileN + t) * 16 + r;
    if (col >= L2) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (orow[e] >= 0 && orow[e] < B) out[(size_t)orow[e] * L2 + col] = acc[t][e];
  }
}

// d_w1 = d_z1^T l0 ("TN": both operands contiguous along the non-K dimension; K = batch).  A wave
// owns 2 x 4 tiles (32 units x 64 columns) and a slice of the batch; per K step (4 samples) every
// lane loads one dword per tile row/column block.
constexpr int kBwTileM = 2, kBwTileN = 4;

// Bucketed (bk.rows): a wave owns the same tile of ONE bucket's d_w1 and slice ks of that bucket's row range
// [seg[kb] + ks*klen, .. + klen); a slice that starts past the bucket's end writes nothing (the slab sum knows, see
// bucket_slabs).  Slab layout [ksplit][K * L2 * L1].
__device__ __forceinline__ void l1_backward_w_body(const float* __restrict__ x, int pairwise, const float* __restrict__ d_z1,
                                                   int B, int L1, int L2, int ksplit, int klen, float* __restrict__ part,
                                                   long long block, const Buckets& bk) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, q = lane >> 4;
  const int m_groups = L2 / (16 * kBwTileM);  // L2 % 32 == 0
  const int n_groups = L1 / (16 * kBwTileN);  // L1 % 64 == 0
  long long wid = block * 4 + wave;
  if (wid >= (long long)m_groups * n_groups * ksplit * bk.K) return;
  const int ks = (int)(wid % ksplit);
  wid /= ksplit;
  const int ng = (int)(wid % n_groups);
  wid /= n_groups;
  const int mg = (int)(wid % m_groups);
  const int kb = (int)(wid / m_groups);
  const int half = L1 / 2;
  int b_lo = ks * klen, b_hi = min(B, b_lo + klen);
  if (bk.rows) {
    const int s_lo = bk.seg[kb], s_hi = bk.seg[kb + 1];
    b_lo = s_lo + ks * klen;
    b_hi = min(s_hi, b_lo + klen);
    if (b_lo >= s_hi && !(ks == 0 && ksplit == 1)) return;  // empty slice; an unsplit product still writes its zeros
  }
  f32x4 acc[kBwTileM][kBwTileN];
#pragma unroll
  for (int i = 0; i < kBwTileM; ++i)
#pragma unroll
    for (int t = 0; t < kBwTileN; ++t) acc[i][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // column j of l0 for each of this lane's N tiles; a 16-column tile never straddles `half` (half % 16 == 0)
  int cj[kBwTileN], cj2[kBwTileN];
#pragma unroll
  for (int t = 0; t < kBwTileN; ++t) {
    const int j = (ng * kBwTileN + t) * 16 + r;
    if (!pairwise) { cj[t] = j; cj2[t] = -1; }
    else if (j < half) { cj[t] = j; cj2[t] = j + half; }
    else { cj[t] = j - half; cj2[t] = -1; }
  }
  auto load_step = [&](int b0, float (&a)[kBwTileM], float (&bv)[kBwTileN]) {
    int b = b0 + q;
    bool ok = b < b_hi;
    if (bk.rows) {
      b = ok ? bk.rows[b] : -1;
      ok = b >= 0;
    }
    const float* __restrict__ dz = d_z1 + (size_t)(ok ? b : 0) * L2 + mg * 16 * kBwTileM + r;
    const float* __restrict__ xr = x + (size_t)(ok ? b : 0) * L1;
#pragma unroll
    for (int i = 0; i < kBwTileM; ++i) a[i] = ok ? dz[16 * i] : 0.f;
#pragma unroll
    for (int t = 0; t < kBwTileN; ++t) {
      float v = ok ? xr[cj[t]] : 0.f;
      if (cj2[t] >= 0 && ok) v *= xr[cj2[t]];
      bv[t] = v;
    }
  };
  constexpr int kSteps = 8;  // K steps (of 4 samples) whose loads are issued together
  for (int b0 = b_lo; b0 < b_hi; b0 += 4 * kSteps) {
    float a[kSteps][kBwTileM], bv[kSteps][kBwTileN];
#pragma unroll
    for (int u = 0; u < kSteps; ++u) load_step(b0 + 4 * u, a[u], bv[u]);  // rows >= b_hi load as zero
#pragma unroll
    for (int u = 0; u < kSteps; ++u)
#pragma unroll
      for (int i = 0; i < kBwTileM; ++i)
#pragma unroll
        for (int t = 0; t < kBwTileN; ++t)
          acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][i], bv[u][t], acc[i][t], 0, 0, 0);
  }
  float* __restrict__ out = part + ((size_t)ks * bk.K + kb) * L2 * L1;
#pragma unroll
  for (int i = 0; i < kBwTileM; ++i)
#pragma unroll
    for (int t = 0; t < kBwTileN; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int orow = (mg * kBwTileM + i) * 16 + 4 * q + e;
        const int ocol = (ng * kBwTileN + t) * 16 + r;
        out[(size_t)orow * L1 + ocol] = acc[i][t][e];
      }
}

// fixed-order sum of split-K slabs: out[i] = sum_s part[s][i]
__global__ __launch_bounds__(256) void slab_sum_kernel(const float* __restrict__ part, int slabs, long long count,
                                                       float* __restrict__ out, Buckets bk, int klen) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= count) return;  // count % 4 == 0
  if (bk.rows) {  // only the slices of this element's bucket that hold rows were written (l1_backward_w_body)
    const int kb = (int)(i / (count / bk.K));
    const int nz = (bk.seg[kb + 1] - bk.seg[kb] + klen - 1) / klen;
    slabs = nz < slabs ? nz : slabs;
    if (slabs == 0) {
      *reinterpret_cast<float4*>(out + i) = make_float4(0.f, 0.f, 0.f, 0.f);
      return;
    }
  }
  float4 acc = *reinterpret_cast<const float4*>(part + i);
  for (int s = 1; s < slabs; ++s) {
    const float4 v = *reinterpret_cast<const float4*>(part + (size_t)s * count + i);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  *reinterpret_cast<float4*>(out + i) = acc;
}

// d_x = (d_z1 W1) through the pairwise block ("NN": A contiguous along K = L2, B along N).  A wave
// owns 16 samples x two 16-column tiles: columns j and j + L1/2 when pairwise (the pairwise backward
// needs both), adjacent tiles otherwise.
//
// The tile's pieces are shared with tail_dx_train_kernel (which reads d_z1 out of LDS and requests its W1
// operands before the per-sample tail runs): same operands, same MFMA order, so d_x is bitwise the same.
// K is walked in chunks of up to 4 blocks of 16; every load of a chunk is issued before its MFMAs, so a
// wave pays one L2 round trip per chunk (L2 = 128: two) instead of one per block
constexpr int kBwxKC = 4;
struct BwxChunk {
  float4 a[kBwxKC];
  float b0[kBwxKC][4], b1[kBwxKC][4];
};

// B operand of one 16-column tile (columns c..c+15)
__device__ __forceinline__ void bwx_load_b_tile(float (&b)[kBwxKC][4], const float* __restrict__ w1, int kb0, int L1, int L2, int c,
                                                int r, int q) {
#pragma unroll
  for (int u = 0; u < kBwxKC; ++u) {
    const int kb = kb0 + 16 * u;
    const bool in = kb < L2;  // wave-uniform
    const int k = (in ? kb : 0) + 4 * q;
    const float* __restrict__ wk = w1 + (size_t)k * L1 + r;
#pragma unroll
    for (int e = 0; e < 4; ++e) b[u][e] = in ? wk[(size_t)e * L1 + c] : 0.f;
  }
}

__device__ __forceinline__ void bwx_load_b(BwxChunk& ch, const float* __restrict__ w1, int kb0, int L1, int L2, int c0, int c1,
                                           int r, int q) {
  bwx_load_b_tile(ch.b0, w1, kb0, L1, L2, c0, r, q);
  bwx_load_b_tile(ch.b1, w1, kb0, L1, L2, c1, r, q);
}

// dz: this lane's d_z1 row (global or LDS)
__device__ __forceinline__ void bwx_load_a(BwxChunk& ch, const float* dz, bool row_ok, int kb0, int L2, int q) {
#pragma unroll
  for (int u = 0; u < kBwxKC; ++u) {
    const int kb = kb0 + 16 * u;
    const bool in = kb < L2;
    const int k = (in ? kb : 0) + 4 * q;
    const float4 v = *reinterpret_cast<const float4*>(dz + k);  // in bounds for every lane (a padding row reads row 0 / its own)
    ch.a[u] = (row_ok && in) ? v : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

__device__ __forceinline__ void bwx_mma(const BwxChunk& ch, f32x4& acc0, f32x4& acc1) {
#pragma unroll
  for (int u = 0; u < kBwxKC; ++u) {
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ch.a[u].x, ch.b0[u][0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ch.a[u].x, ch.b1[u][0], acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ch.a[u].y, ch.b0[u][1], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ch.a[u].y, ch.b1[u][1], acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ch.a[u].z, ch.b0[u][2], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ch.a[u].z, ch.b1[u][2], acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ch.a[u].w, ch.b0[u][3], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ch.a[u].w, ch.b1[u][3], acc1, 0, 0, 0);
  }
}

// the MFMAs of one of the two tiles, in the order bwx_mma gives that tile's accumulator
__device__ __forceinline__ void bwx_mma_tile(const float4 (&a)[kBwxKC], const float (&b)[kBwxKC][4], f32x4& acc) {
#pragma unroll
  for (int u = 0; u < kBwxKC; ++u) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].x, b[u][0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].y, b[u][1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].z, b[u][2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].w, b[u][3], acc, 0, 0, 0);
  }
}

// the x values the pairwise epilogue multiplies by (accumulator register e = sample orows[e])
__device__ __forceinline__ void bwx_load_x(float (&xv0)[4], float (&xv1)[4], const float* __restrict__ x, const int (&orows)[4], int B,
                                           int L1, int c0, int c1, int r) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool ok = orows[e] >= 0 && orows[e] < B;
    const float* __restrict__ xr = x + (size_t)(ok ? orows[e] : 0) * L1;
    const float a = xr[c0 + r], b = xr[c1 + r];  // unconditional (row 0 for a padding row): no branch per load
    xv0[e] = ok ? a : 0.f;
    xv1[e] = ok ? b : 0.f;
  }
}

__device__ __forceinline__ void bwx_store(const f32x4& acc0, const f32x4& acc1, const float (&xv0)[4], const float (&xv1)[4],
                                          const int (&orows)[4], int pairwise, int B, int L1, int c0, int c1, int r,
                                          float* __restrict__ d_x) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int orow = orows[e];
    if (orow < 0 || orow >= B) continue;
    float* __restrict__ o = d_x + (size_t)orow * L1;
    if (pairwise) {
      o[c0 + r] = fmaf(acc0[e], xv1[e], acc1[e]);
      o[c1 + r] = acc0[e] * xv0[e];
    } else {
      o[c0 + r] = acc0[e];
      o[c1 + r] = acc1[e];
    }
  }
}

__device__ __forceinline__ void l1_backward_x_body(const float* __restrict__ x, int pairwise, const float* __restrict__ w1,
                                                   const float* __restrict__ d_z1, int B, int L1, int L2,
                                                   float* __restrict__ d_x, long long block, const Buckets& bk) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, q = lane >> 4;
  const int half = L1 / 2;
  const int n_pairs = L1 / 32;
  const int m_tiles = bk.rows ? bk.tiles : (B + 15) / 16;
  const long long wid = block * 4 + wave;
  if (wid >= (long long)m_tiles * n_pairs) return;
  const int np = (int)(wid % n_pairs);
  const int mt = (int)(wid / n_pairs);
  const int c0 = pairwise ? np * 16 : np * 32;
  const int c1 = pairwise ? c0 + half : c0 + 16;
  int row = mt * 16 + r;
  int orows[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) orows[e] = mt * 16 + 4 * q + e;
  if (bk.rows) {  // tile of one bucket (see l1_forward_mfma)
    const int kb = bk.tile_bucket[mt];
    if (kb < 0) return;
    w1 += (size_t)kb * L2 * L1;
    row = bk.rows[row];
#pragma unroll
    for (int e = 0; e < 4; ++e) orows[e] = bk.rows[orows[e]];
  }
  const bool row_ok = row >= 0 && row < B;
  const float* __restrict__ dz = d_z1 + (size_t)(row_ok ? row : 0) * L2;
  f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
  for (int kb0 = 0; kb0 < L2; kb0 += 16 * kBwxKC) {  // L2 % 16 == 0
    BwxChunk ch;
    bwx_load_a(ch, dz, row_ok, kb0, L2, q);
    bwx_load_b(ch, w1, kb0, L1, L2, c0, c1, r, q);
    bwx_mma(ch, acc0, acc1);
  }
  float xv0[4] = {0.f, 0.f, 0.f, 0.f}, xv1[4] = {0.f, 0.f, 0.f, 0.f};
  if (pairwise) bwx_load_x(xv0, xv1, x, orows, B, L1, c0, c1, r);
  bwx_store(acc0, acc1, xv0, xv1, orows, pairwise, B, L1, c0, c1, r, d_x);
}

__global__ __launch_bounds__(256) void l1_backward_w_mfma(const float* __restrict__ x, int pairwise,
                                                          const float* __restrict__ d_z1, int B, int L1, int L2,
                                                          int ksplit, int klen, float* __restrict__ part, Buckets bk) {
  l1_backward_w_body(x, pairwise, d_z1, B, L1, L2, ksplit, klen, part, blockIdx.x, bk);
}

__global__ __launch_bounds__(256) void l1_backward_x_mfma(const float* __restrict__ x, int pairwise,
                                                          const float* __restrict__ w1,
                                                          const float* __restrict__ d_z1, int B, int L1, int L2,
                                                          float* __restrict__ d_x, Buckets bk) {
  l1_backward_x_body(x, pairwise, w1, d_z1, B, L1, L2, d_x, blockIdx.x, bk);
}

// d_x and the d_w1 slabs in one launch: both only need d_z1, so the two small products share the chip instead of
// running back to back.  Blocks [0, w_blocks) form the weight-gradient slabs (the longer product, dispatched first),
// the rest d_x.
__global__ __launch_bounds__(256) void l1_backward_xw_mfma(const float* __restrict__ x, int pairwise,
                                                           const float* __restrict__ w1, const float* __restrict__ d_z1,
                                                           int B, int L1, int L2, float* __restrict__ d_x, int w_blocks,
                                                           int ksplit, int klen, float* __restrict__ part, Buckets bk) {
  if ((int)blockIdx.x < w_blocks) l1_backward_w_body(x, pairwise, d_z1, B, L1, L2, ksplit, klen, part, blockIdx.x, bk);
  else l1_backward_x_body(x, pairwise, w1, d_z1, B, L1, L2, d_x, (long long)blockIdx.x - w_blocks, bk);
}

// ------------------------------------------------------------------ narrow layers (per sample, LDS)
__global__ __launch_bounds__(128) void tail_forward_kernel(const float* __restrict__ part, int ksplit,
                                                           const float* __restrict__ b1, const float* __restrict__ w2,
                                                           const float* __restrict__ b2, const float* __restrict__ w3,
                                                           const float* __restrict__ b3, float clip, int B, int L2,
                                                           int L3, int C, float* __restrict__ h1,
                                                           float* __restrict__ h2, float* __restrict__ logits, Buckets bk) {
  extern __shared__ float lds[];  // h1 [L2], h2 [L3]
  float* h1s = lds;
  float* h2s = lds + L2;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (bk.bucket) {  // this sample's layer stack
    const int kb = bk.bucket[b];
    b1 += (size_t)kb * L2; w2 += (size_t)kb * L3 * L2; b2 += (size_t)kb * L3; w3 += (size_t)kb * C * L3; b3 += (size_t)kb * C;
  }
  for (int j = tid; j < L2; j += 128) {
    float z = b1[j];
    for (int s = 0; s < ksplit; ++s) z += part[((size_t)s * B + b) * L2 + j];
    const float h = act_fn(z, clip);
    h1s[j] = h;
    h1[(size_t)b * L2 + j] = h;
  }
  __syncthreads();
  for (int j = tid; j < L3; j += 128) {
    const float* __restrict__ wr = w2 + (size_t)j * L2;
    float z = b2[j];
    for (int k = 0; k < L2; ++k) z = fmaf(wr[k], h1s[k], z);
    const float h = act_fn(z, clip);
    h2s[j] = h;
    h2[(size_t)b * L3 + j] = h;
  }
  __syncthreads();
  for (int c = tid; c < C; c += 128) {
    const float* __restrict__ wr = w3 + (size_t)c * L3;
    float z = b3[c];
    for (int k = 0; k < L3; ++k) z = fmaf(wr[k], h2s[k], z);
    logits[(size_t)b * C + c] = z;
  }
}

__global__ __launch_bounds__(128) void tail_backward_kernel(const float* __restrict__ d_logits,
                                                            const float* __restrict__ h1, const float* __restrict__ h2,
                                                            const float* __restrict__ w2, const float* __restrict__ w3,
                                                            float clip, int L2, int L3, int C,
                                                            float* __restrict__ d_z1, float* __restrict__ d_z2, Buckets bk) {
  extern __shared__ float lds[];  // d_logits [C], d_z2 [L3]
  float* dls = lds;
  float* dz2s = lds + C;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (bk.bucket) {
    const int kb = bk.bucket[b];
    w2 += (size_t)kb * L3 * L2; w3 += (size_t)kb * C * L3;
  }
  for (int c = tid; c < C; c += 128) dls[c] = d_logits[(size_t)b * C + c];
  __syncthreads();
  for (int j = tid; j < L3; j += 128) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) s = fmaf(dls[c], w3[(size_t)c * L3 + j], s);
    const float v = gate_fn(s, h2[(size_t)b * L3 + j], clip);
    dz2s[j] = v;
    d_z2[(size_t)b * L3 + j] = v;
  }
  __syncthreads();
  for (int k = tid; k < L2; k += 128) {
    float s = 0.f;
    for (int j = 0; j < L3; ++j) s = fmaf(dz2s[j], w2[(size_t)j * L2 + k], s);
    d_z1[(size_t)b * L2 + k] = gate_fn(s, h1[(size_t)b * L2 + k], clip);
  }
}

__global__ __launch_bounds__(256) void small_wgrad_kernel(SmallWgrad a) {
  __shared__ float red[1024];
  small_wgrad_body(a, (int)blockIdx.x, red);
}

// ------------------------------------------------------------------ fused narrow layers + loss (training)
// Per sample, out of LDS: h1 = act(sum of split-K slabs + b1), h2, logits, softmax cross-entropy, d_logits,
// then back through the two narrow layers to d_z2 and d_z1.  Replaces tail_forward + cross_entropy +
// tail_backward (three launches and two round trips of logits / d_logits through memory).
// Dot products use 4 threads per output (coalesced 16-byte runs of each weight row).
template <int NT>
__device__ __forceinline__ float block_reduce_nt(float v, bool is_max, float* red) {  // red: NT / 64 floats
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const float o = __shfl_xor(v, s);
    v = is_max ? fmaxf(v, o) : v + o;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int i = 1; i < NT / 64; ++i) r = is_max ? fmaxf(r, red[i]) : r + red[i];
  __syncthreads();
  return r;
}

// Per-output arithmetic of the tail, shared with tail_dx_train_kernel so that both form every value with the same
// expression (same operation order, same fma contractions) whatever the thread mapping around it.
// One of four chains of a layer-2 / logit dot product: z += w . h over one float4 run
__device__ __forceinline__ float tail_dot4(const float4& w, const float4& h, float z) {
  return fmaf(w.w, h.w, fmaf(w.z, h.z, fmaf(w.y, h.y, fmaf(w.x, h.x, z))));
}

// max and sum of exp over the C <= 64 logits of N samples (lane c holds logit c of each): the same 64-lane butterflies
// in every wave, lanes >= C add 0 / max -inf; the N samples' chains are interleaved
template <int N>
__device__ __forceinline__ void ce_wave_stats(const float (&v)[N], bool in, float (&mx)[N], float (&se)[N]) {
#pragma unroll
  for (int n = 0; n < N; ++n) mx[n] = in ? v[n] : -INFINITY;
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1)
#pragma unroll
    for (int n = 0; n < N; ++n) mx[n] = fmaxf(mx[n], __shfl_xor(mx[n], sh));
#pragma unroll
  for (int n = 0; n < N; ++n) se[n] = in ? expf(v[n] - mx[n]) : 0.0f;
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1)
#pragma unroll
    for (int n = 0; n < N; ++n) se[n] += __shfl_xor(se[n], sh);
}

// v of lane (lane ^ SH): the same value __shfl_xor(v, SH) gives, through DPP (SH 1, 2) or ds_swizzle (4 .. 16) instead
// of an LDS round trip through ds_bpermute
template <int SH>
__device__ __forceinline__ float lane_xor(float v) {
  const int i = __float_as_int(v);
  if constexpr (SH == 1) return __int_as_float(__builtin_amdgcn_update_dpp(i, i, 0xB1, 0xF, 0xF, false));  // quad_perm 1,0,3,2
  else if constexpr (SH == 2) return __int_as_float(__builtin_amdgcn_update_dpp(i, i, 0x4E, 0xF, 0xF, false));  // quad_perm 2,3,0,1
  else if constexpr (SH < 32) return __int_as_float(__builtin_amdgcn_ds_swizzle(i, 0x1F | (SH << 10)));  // bit mode: lane ^ SH
  else return __shfl_xor(v, SH);
}

// ce_wave_stats with lane_xor: the same butterflies (same operands, same order), cheaper exchanges
template <int N>
__device__ __forceinline__ void ce_wave_stats_fast(const float (&v)[N], bool in, float (&mx)[N], float (&se)[N]) {
#pragma unroll
  for (int n = 0; n < N; ++n) mx[n] = in ? v[n] : -INFINITY;
#define NNUE_MAX_STEP(SH) _Pragma("unroll") for (int n = 0; n < N; ++n) mx[n] = fmaxf(mx[n], lane_xor<SH>(mx[n]));
  NNUE_MAX_STEP(32) NNUE_MAX_STEP(16) NNUE_MAX_STEP(8) NNUE_MAX_STEP(4) NNUE_MAX_STEP(2) NNUE_MAX_STEP(1)
#undef NNUE_MAX_STEP
#pragma unroll
  for (int n = 0; n < N; ++n) se[n] = in ? expf(v[n] - mx[n]) : 0.0f;
#define NNUE_SUM_STEP(SH) _Pragma("unroll") for (int n = 0; n < N; ++n) se[n] += lane_xor<SH>(se[n]);
  NNUE_SUM_STEP(32) NNUE_SUM_STEP(16) NNUE_SUM_STEP(8) NNUE_SUM_STEP(4) NNUE_SUM_STEP(2) NNUE_SUM_STEP(1)
#undef NNUE_SUM_STEP
}

// d loss / d logit z of a sample with a valid label
__device__ __forceinline__ float ce_dlogit(float z, float mx, float inv, bool is_y, float scale_over_b) {
  return (expf(z - mx) * inv - (is_y ? 1.0f : 0.0f)) * scale_over_b;
}

// ---- the SOFT arm of the two tail kernels (soft targets, include/nnue_hip.h): the kernels take a trailing pack that is
// empty (the plain kernels: the arguments and the code they have always had) or one SoftTargets

// the smoothing term's sum_c (mx - z_c) over the C <= 64 logits of N samples: one more 64-lane butterfly beside those of
// ce_wave_stats (FAST: the exchanges of ce_wave_stats_fast), lanes >= C add 0
template <int N, bool FAST>
__device__ __forceinline__ void ce_wave_csum(const float (&v)[N], bool in, const float (&mx)[N], float (&cs)[N]) {
#pragma unroll
  for (int n = 0; n < N; ++n) cs[n] = in ? mx[n] - v[n] : 0.0f;
  if constexpr (FAST) {
#define NNUE_SUM_STEP(SH) _Pragma("unroll") for (int n = 0; n < N; ++n) cs[n] += lane_xor<SH>(cs[n]);
    NNUE_SUM_STEP(32) NNUE_SUM_STEP(16) NNUE_SUM_STEP(8) NNUE_SUM_STEP(4) NNUE_SUM_STEP(2) NNUE_SUM_STEP(1)
#undef NNUE_SUM_STEP
  } else {
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1)
#pragma unroll
      for (int n = 0; n < N; ++n) cs[n] += __shfl_xor(cs[n], sh);
  }
}

// d loss / d logit z of a sample that counts, against the soft target t.  The explicit fma is the contraction the compiler
// picks for ce_dlogit's p - onehot: with t = 1 or 0 the two agree bitwise (left to itself it folds t's own sum into p - t)
__device__ __forceinline__ float ce_dlogit_soft(float z, float mx, float inv, float t, float scale_over_b) {
  return fmaf(expf(z - mx), inv, -t) * scale_over_b;
}

// ---- the DISTILL arm (the teacher term of include/nnue_hip.h, "soft targets"): the trailing pack is one DistillTargets; it
// holds the SOFT arm's values too (SOFT is true with it) and adds a teacher row per sample.  Per-element arithmetic: common.h.

// a[n] over the 64 lanes, max or sum, in place: the butterflies of ce_wave_stats (FAST: the exchanges of ce_wave_stats_fast)
template <int N, bool FAST, bool MAX>
__device__ __forceinline__ void ce_wave_all(float (&a)[N]) {
  if constexpr (FAST) {
#define NNUE_ALL_STEP(SH) _Pragma("unroll") for (int n = 0; n < N; ++n) { const float o = lane_xor<SH>(a[n]); a[n] = MAX ? fmaxf(a[n], o) : a[n] + o; }
    NNUE_ALL_STEP(32) NNUE_ALL_STEP(16) NNUE_ALL_STEP(8) NNUE_ALL_STEP(4) NNUE_ALL_STEP(2) NNUE_ALL_STEP(1)
#undef NNUE_ALL_STEP
  } else {
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1)
#pragma unroll
      for (int n = 0; n < N; ++n) {
        const float o = __shfl_xor(a[n], sh);
        a[n] = MAX ? fmaxf(a[n], o) : a[n] + o;
      }
  }
}

// every statistic of the DISTILL arm for N samples with C <= 64 (lane c holds logit v and teacher logit u of class c), in TWO
// butterflies' depth -- the plain kernels' -- whatever their number: the exchanges of independent chains are issued together,
// a chain's values do not depend on what runs beside it.  First the two maxima (mx = max v, mu = max u), then the five sums:
// se and cs (those of ce_wave_stats and ce_wave_csum, bit for bit), sU = sum eu, sT = sum ez, ks = sum eu ((mx - v) - (mu - u)),
// with eu = exp((u - mu) / T) and ez = exp((v - mx) / T) of this lane (0 past C).
template <int N, bool FAST>
__device__ __forceinline__ void ce_wave_distill(const float (&v)[N], const float (&u)[N], bool in, float T, float (&mx)[N], float (&se)[N],
                                                float (&cs)[N], float (&mu)[N], float (&eu)[N], float (&ez)[N], float (&sU)[N],
                                                float (&sT)[N], float (&ks)[N]) {
  float m[2 * N], a[5 * N];
#pragma unroll
  for (int n = 0; n < N; ++n) m[n] = in ? v[n] : -INFINITY, m[N + n] = in ? u[n] : -INFINITY;
  ce_wave_all<2 * N, FAST, true>(m);
#pragma unroll
  for (int n = 0; n < N; ++n) {
    mx[n] = m[n], mu[n] = m[N + n];
    eu[n] = in ? nnue_distill_exp(u[n], mu[n], T) : 0.0f;
    ez[n] = in ? nnue_distill_exp(v[n], mx[n], T) : 0.0f;
    a[n] = in ? expf(v[n] - mx[n]) : 0.0f;
    a[N + n] = in ? mx[n] - v[n] : 0.0f;
    a[2 * N + n] = eu[n];
    a[3 * N + n] = ez[n];
    a[4 * N + n] = in ? nnue_distill_kl_acc(0.0f, eu[n], v[n], mx[n], u[n], mu[n]) : 0.0f;
  }
  ce_wave_all<5 * N, FAST, false>(a);
#pragma unroll
  for (int n = 0; n < N; ++n) se[n] = a[n], cs[n] = a[N + n], sU[n] = a[2 * N + n], sT[n] = a[3 * N + n], ks[n] = a[4 * N + n];
}

// class slice cp (of S) of d_z2[j] = sum_c d_logits[c] w3[c][j]: four chains over c = cp, cp + S, ...  (w3j = w3 + j)
template <int S>
__device__ __forceinline__ float dz2_slice(const float* dl, const float* w3j, int cp, int C, int L3) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int c = cp;
  for (; c + 3 * S < C; c += 4 * S) {
    s0 = fmaf(dl[c], w3j[(size_t)c * L3], s0);
    s1 = fmaf(dl[c + S], w3j[(size_t)(c + S) * L3], s1);
    s2 = fmaf(dl[c + 2 * S], w3j[(size_t)(c + 2 * S) * L3], s2);
    s3 = fmaf(dl[c + 3 * S], w3j[(size_t)(c + 3 * S) * L3], s3);
  }
  for (; c < C; c += S) s0 = fmaf(dl[c], w3j[(size_t)c * L3], s0);
  return (s0 + s1) + (s2 + s3);
}

// the S slices of one d_z2 value in a fixed pairwise tree: (p0 + p1) + (p2 + p3) ...
template <int S>
__device__ __forceinline__ float slice_tree(float (&q)[S]) {
#pragma unroll
  for (int w = 1; w < S; w *= 2)
#pragma unroll
    for (int i = 0; i + w < S; i += 2 * w) q[i] += q[i + w];
  return q[0];
}

// NT threads per sample: 128 for the usual class counts, 512 when C is large (1000 classes at 224x224: the logits,
// the softmax and the d_z2 sum are then 4x wider per pass).
template <int NT, bool VEC, typename... Soft>
__global__ __launch_bounds__(NT) void tail_train_kernel(const float* __restrict__ part, int ksplit,
                                                        const float* __restrict__ b1, const float* __restrict__ w2,
                                                        const float* __restrict__ b2, const float* __restrict__ w3,
                                                        const float* __restrict__ b3, float clip,
                                                        const int64_t* __restrict__ labels, float scale_over_b, int B,
                                                        int L2, int L3, int C, float* __restrict__ h1,
                                                        float* __restrict__ h2, float* __restrict__ logits,
                                                        float* __restrict__ sample_loss, float* __restrict__ d_logits,
                                                        float* __restrict__ d_z1, float* __restrict__ d_z2, Buckets bk,
                                                        const float* __restrict__ x, int L1, float* __restrict__ x_g,
                                                        float* __restrict__ d_z1_g, Soft... soft) {
  constexpr bool SOFT = sizeof...(Soft) == 1;
  constexpr bool DISTILL = (std::is_same_v<Soft, DistillTargets> || ...);
  extern __shared__ float lds[];  // h1 [L2] | h2 [L3] | logits / d_logits [C] | d_z2 [L3] | red [8] | DISTILL: teacher row [C]
  constexpr int S = NT / 32;      // class slices of the d_z2 sum
  __shared__ float part_s[S][32];
  float* h1s = lds;
  float* h2s = h1s + L2;
  float* lgs = h2s + L3;
  float* dz2s = lgs + C;
  float* red = dz2s + L3;
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  // Grouped mode (d_z1_g != NULL; bucketed stacks whose d_w1 product rides in nnue_ftm_backward_bucketed): one workgroup per
  // GROUPED row g.  It also leaves the operands of that product in grouped row order -- x_g[g] = x[b] (the
  // FeatureTransformer output) and d_z1_g[g] = d_z1[b] -- and a padding row leaves zeros in both.
  const int g = blockIdx.x;
  if (d_z1_g) {
    b = bk.rows[g];  // workgroup-uniform
    if (b < 0) {
      for (int i = tid; i < L1; i += NT) x_g[(size_t)g * L1 + i] = 0.0f;
      for (int i = tid; i < L2; i += NT) d_z1_g[(size_t)g * L2 + i] = 0.0f;
      return;
    }
    for (int i = tid * 4; i < L1; i += NT * 4)  // L1 % 4 == 0 (the rider's shapes); nothing below waits for this copy
      *reinterpret_cast<float4*>(x_g + (size_t)g * L1 + i) = *reinterpret_cast<const float4*>(x + (size_t)b * L1 + i);
  }
  if (bk.bucket) {  // this sample's layer stack
    const int kb = bk.bucket[b];
    b1 += (size_t)kb * L2; w2 += (size_t)kb * L3 * L2; b2 += (size_t)kb * L3; w3 += (size_t)kb * C * L3; b3 += (size_t)kb * C;
  }
  const int og = tid >> 2, part4 = tid & 3;
  // VEC (L2 % 4 == 0, L3 % 4 == 0, 16-byte aligned w2 / w3): a thread's share of a weight row is float4 runs, and the
  // first pass's runs are requested before the slab sum so that their latency hides behind it
  constexpr int kPre2 = 8, kPre3 = 2;
  float4 w2v[kPre2], w3v[kPre3];
  if constexpr (VEC) {
#pragma unroll
    for (int i = 0; i < kPre2; ++i) {
      const int k = 4 * (part4 + 4 * i);
      w2v[i] = (og < L3 && k < L2) ? *reinterpret_cast<const float4*>(w2 + (size_t)og * L2 + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < kPre3; ++i) {
      const int k = 4 * (part4 + 4 * i);
      w3v[i] = (og < C && k < L3) ? *reinterpret_cast<const float4*>(w3 + (size_t)og * L3 + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  const float b2v = (VEC && og < L3) ? b2[og] : 0.0f, b3v = (VEC && og < C) ? b3[og] : 0.0f;
  const int64_t y = labels[b];
  int64_t y2 = y;
  float lam = 1.0f, eps = 0.0f;
  if constexpr (SOFT) {
    const SoftTargets st = (soft, ...);
    eps = st.eps;
    if (st.labels_b) y2 = st.labels_b[b], lam = st.lam[b];
  }
  // DISTILL: the teacher row is read once, strided by thread; the first kPreU values per thread are requested here and
  // parked in LDS behind the slab sum, whose loads hide their latency (1024 classes at NT = 512), the rest goes straight
  constexpr int kPreU = 2;
  float* us = red + 8;
  float alpha = 0.0f, T = 1.0f, uv[kPreU];
  if constexpr (DISTILL) {
    const DistillTargets dt = (soft, ...);
    alpha = dt.alpha, T = dt.temperature;
    const float* __restrict__ ur = dt.teacher + (size_t)b * C;
#pragma unroll
    for (int i = 0; i < kPreU; ++i) uv[i] = tid + NT * i < C ? ur[tid + NT * i] : 0.0f;
    for (int c = tid + NT * kPreU; c < C; c += NT) us[c] = ur[c];
  }
  for (int j = tid; j < L2; j += NT) {
    float z = b1[j];
    int s = 0;
    for (; s + 8 <= ksplit; s += 8) {  // eight loads in flight, summed in slab order
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = part[((size_t)(s + u) * B + b) * L2 + j];
#pragma unroll
      for (int u = 0; u < 8; ++u) z += v[u];
    }
    for (; s < ksplit; ++s) z += part[((size_t)s * B + b) * L2 + j];
    const float h = act_fn(z, clip);
    h1s[j] = h;
    h1[(size_t)b * L2 + j] = h;
  }
  if constexpr (DISTILL) {
#pragma unroll
    for (int i = 0; i < kPreU; ++i)
      if (tid + NT * i < C) us[tid + NT * i] = uv[i];
  }
  __syncthreads();
  for (int j0 = 0; j0 < L3; j0 += NT / 4) {
    const int j = j0 + og;
    float z = 0.f;
    if (j < L3) {
      const float* __restrict__ wr = w2 + (size_t)j * L2;
      if constexpr (VEC) {
        int k = 4 * part4;
        if (j0 == 0) {
#pragma unroll
          for (int i = 0; i < kPre2; ++i) {
            const int kk = 4 * (part4 + 4 * i);
            if (kk < L2) z = tail_dot4(w2v[i], *reinterpret_cast<const float4*>(h1s + kk), z);
          }
          k += 16 * kPre2;
        }
        for (; k < L2; k += 16) z = tail_dot4(*reinterpret_cast<const float4*>(wr + k), *reinterpret_cast<const float4*>(h1s + k), z);
      } else {
        for (int k = part4; k < L2; k += 4) z = fmaf(wr[k], h1s[k], z);
      }
    }
    z += __shfl_xor(z, 1);
    z += __shfl_xor(z, 2);
    if (j < L3 && part4 == 0) {
      const float h = act_fn(z + ((VEC && j0 == 0) ? b2v : b2[j]), clip);
      h2s[j] = h;
      h2[(size_t)b * L3 + j] = h;
    }
  }
  __syncthreads();
  for (int c0 = 0; c0 < C; c0 += NT / 4) {
    const int c = c0 + og;
    float z = 0.f;
    if (c < C) {
      const float* __restrict__ wr = w3 + (size_t)c * L3;
      if constexpr (VEC) {
        int k = 4 * part4;
        if (c0 == 0) {
#pragma unroll
          for (int i = 0; i < kPre3; ++i) {
            const int kk = 4 * (part4 + 4 * i);
            if (kk < L3) z = tail_dot4(w3v[i], *reinterpret_cast<const float4*>(h2s + kk), z);
          }
          k += 16 * kPre3;
        }
        for (; k < L3; k += 16) z = tail_dot4(*reinterpret_cast<const float4*>(wr + k), *reinterpret_cast<const float4*>(h2s + k), z);
      } else {
        for (int k = part4; k < L3; k += 4) z = fmaf(wr[k], h2s[k], z);
      }
    }
    z += __shfl_xor(z, 1);
    z += __shfl_xor(z, 2);
    if (c < C && part4 == 0) {
      z += (VEC && c0 == 0) ? b3v : b3[c];
      lgs[c] = z;
      logits[(size_t)b * C + c] = z;
    }
  }
  __syncthreads();
  // softmax cross-entropy of this sample and its gradient
  float mx = -INFINITY, se = 0.f, csum = 0.f;  // csum (SOFT): sum_c (mx - z_c), the smoothing term
  float mu = -INFINITY, sU = 0.f, sT = 0.f, ksum = 0.f;  // DISTILL: the teacher's max and the three sums of the definition
  if (C <= 64) {  // every wave forms the same two reductions by itself: no block barriers
    const int lane = tid & 63;
    const float v[1] = {lane < C ? lgs[lane] : -INFINITY};
    float m1[1], s1[1];
    if constexpr (DISTILL) {
      const float u[1] = {lane < C ? us[lane] : 0.0f};
      float c1[1], mu1[1], eu[1], ez[1], su1[1], st1[1], k1[1];
      ce_wave_distill<1, false>(v, u, lane < C, T, m1, s1, c1, mu1, eu, ez, su1, st1, k1);
      csum = c1[0], mu = mu1[0], sU = su1[0], sT = st1[0], ksum = k1[0];
    } else {
      ce_wave_stats<1>(v, lane < C, m1, s1);
    }
    mx = m1[0];
    se = s1[0];
    if constexpr (SOFT && !DISTILL) {
      float c1[1];
      ce_wave_csum<1, false>(v, lane < C, m1, c1);
      csum = c1[0];
    }
  } else {
    for (int c = tid; c < C; c += NT) mx = fmaxf(mx, lgs[c]);
    mx = block_reduce_nt<NT>(mx, true, red);
    for (int c = tid; c < C; c += NT) se += expf(lgs[c] - mx);
    se = block_reduce_nt<NT>(se, false, red);
    if constexpr (SOFT) {
      for (int c = tid; c < C; c += NT) csum += mx - lgs[c];
      csum = block_reduce_nt<NT>(csum, false, red);
    }
    if constexpr (DISTILL) {
      for (int c = tid; c < C; c += NT) mu = fmaxf(mu, us[c]);
      mu = block_reduce_nt<NT>(mu, true, red);
      for (int c = tid; c < C; c += NT) {
        const float eu = nnue_distill_exp(us[c], mu, T);
        sU += eu;
        sT += nnue_distill_exp(lgs[c], mx, T);
        ksum = nnue_distill_kl_acc(ksum, eu, lgs[c], mx, us[c], mu);
      }
      sU = block_reduce_nt<NT>(sU, false, red);
      sT = block_reduce_nt<NT>(sT, false, red);
      ksum = block_reduce_nt<NT>(ksum, false, red);
    }
  }
  const bool ok = SOFT ? nnue_soft_counts(y, y2, lam, C) : y >= 0 && y < C;
  if constexpr (DISTILL) {
    if (tid == 0) {
      const float ls = ok ? nnue_ce_soft_sample_loss(mx, lgs[y], lgs[y2 >= 0 && y2 < C ? y2 : y], se, csum, lam, eps, C) : 0.0f;
      sample_loss[b] = ok ? nnue_distill_sample_loss(ls, sT, sU, ksum, alpha, T) : 0.0f;
    }
  } else if constexpr (SOFT) {
    if (tid == 0)
      sample_loss[b] = ok ? nnue_ce_soft_sample_loss(mx, lgs[y], lgs[y2 >= 0 && y2 < C ? y2 : y], se, csum, lam, eps, C) : 0.0f;
  } else {
    if (tid == 0) sample_loss[b] = ok ? nnue_ce_sample_loss(mx, lgs[y], se) : 0.0f;
  }
  const float inv = 1.0f / se;
  __syncthreads();  // every thread has read lgs[y] / the logits it needs before they are overwritten
  for (int c = tid; c < C; c += NT) {
    float g;
    if constexpr (DISTILL) {
      const float soft_g = fmaf(expf(lgs[c] - mx), inv, -nnue_soft_target(c == y, c == y2, lam, eps, C));
      g = ok ? nnue_distill_dlogit(soft_g, nnue_distill_exp(lgs[c], mx, T), 1.0f / sT, nnue_distill_exp(us[c], mu, T), 1.0f / sU, alpha, T,
                                   scale_over_b)
             : 0.0f;
    } else if constexpr (SOFT) g = ok ? ce_dlogit_soft(lgs[c], mx, inv, nnue_soft_target(c == y, c == y2, lam, eps, C), scale_over_b) : 0.0f;
    else g = ok ? ce_dlogit(lgs[c], mx, inv, c == y, scale_over_b) : 0.0f;
    lgs[c] = g;
    d_logits[(size_t)b * C + c] = g;
  }
  __syncthreads();
  // d_z2[j] = sum_c d_logits[c] w3[c][j]: 32 units x S class slices per pass, four independent chains per thread
  // (a single serial chain over C = 1000 classes cost 60 us of the 224x224 configuration's step)
  for (int j0 = 0; j0 < L3; j0 += 32) {
    const int j = j0 + (tid & 31), cp = tid >> 5;
    part_s[cp][tid & 31] = j < L3 ? dz2_slice<S>(lgs, w3 + j, cp, C, L3) : 0.0f;
    __syncthreads();
    if (cp == 0 && j < L3) {
      float q[S];
#pragma unroll
      for (int i = 0; i < S; ++i) q[i] = part_s[i][tid];
      const float v = gate_fn(slice_tree<S>(q), h2s[j], clip);
      dz2s[j] = v;
      d_z2[(size_t)b * L3 + j] = v;
    }
    __syncthreads();
  }
  for (int k = tid; k < L2; k += NT) {
    float s = 0.f;
    int j = 0;
    for (; j + 16 <= L3; j += 16) {  // sixteen rows in flight, summed in row order
      float w[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) w[u] = w2[(size_t)(j + u) * L2 + k];
#pragma unroll
      for (int u = 0; u < 16; ++u) s = fmaf(dz2s[j + u], w[u], s);
    }
    for (; j < L3; ++j) s = fmaf(dz2s[j], w2[(size_t)j * L2 + k], s);
    const float v = gate_fn(s, h1s[k], clip);
    d_z1[(size_t)b * L2 + k] = v;
    if (d_z1_g) d_z1_g[(size_t)g * L2 + k] = v;
  }
  __syncthreads();
}

// ------------------------------------------------------------------ fused tail + d_x (training, phases bit 64)
// The per-sample tail above and the d_x product in ONE launch.  A d_x tile of 16 rows only needs d_z1 of those rows,
// and d_z1 only needs their layer-1 slabs, the small weights and the labels, so the workgroup that forms a d_x tile
// runs the tail for its own 16 rows first instead of waiting for a separate launch.  Workgroup = one 16-row tile x one
// column group of 4 pairs of 16-column tiles (c0, c0 + L1/2), one tile per wave.  Every workgroup of a row tile runs
// the same tail; the one of column group 0 writes its outputs (h1, h2, logits, sample_loss, d_logits, d_z2, d_z1 --
// what the merged FeatureTransformer backward's riders read), the others keep d_z1 in LDS only.
//
// The slab sum (slab order, skip-not-add), act_fn / gate_fn, the 64-lane softmax butterflies and the loss are those of
// tail_train_kernel; the four small products run on the f32 MFMA (below), and d_x is formed by the l1_backward_x_body
// pieces.  At the shapes this kernel takes every phase combination runs it (DX = false: the tail alone), so the launch
// forms agree bitwise; tail_train_kernel serves every other shape.
//
// Loads: the W1 column slice, the x values of the pairwise epilogue, the small products' B fragments, biases, labels and
// the tile's first 16 slabs are all requested at entry (one dependent load level).  Placement: blocks are numbered so that all
// column groups of a row tile share blockIdx % 8 (round-robin dispatch puts them on one XCD, whose L2 then serves the 7
// repeated reads of the tile's 128 KB of slabs); results do not depend on it.
constexpr int kTdxRows = 16, kTdxThreads = 512, kTdxMaxC = 64;

// Timing-only hooks (NNUE_ABLATIONS builds, tools/debug/tail_abl.sh).  SKIP (a template parameter, so that the kernel
// with the knob off is the shipped code; NNUE_CLS_ABL_SKIP_TAIL_PRODUCTS=1 launches it): the four small products are
// not formed -- WRONG results, their outputs are stored as zeros.  clocks (NNUE_CLS_ABL_TAIL_CLOCKS=1) =
// [workgroup][kTdxClocks] shader-clock readings, one per phase boundary, taken by thread 0 and written with ordinary
// stores.  A default build compiles neither.
#ifdef NNUE_ABLATIONS
constexpr int kTdxClocks = 10;
struct TdxAbl { long long* clocks; };
#define NNUE_TDX_ABL_PARAM , TdxAbl abl
#define NNUE_TDX_CLOCK(i) do { if (abl.clocks && threadIdx.x == 0) abl.clocks[(size_t)blockIdx.x * kTdxClocks + (i)] = clock64(); } while (0)
#else
#define NNUE_TDX_ABL_PARAM
#define NNUE_TDX_CLOCK(i) do { } while (0)
#endif

// ---- the tile tail's four small products on the f32 MFMA (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 sums)
// The tile has 16 rows = the M of one MFMA, so every product of the tail is a few 16 x 16 output tiles; lane (r, q) =
// (lane & 15, lane >> 4) gives A[row r][k = q] and B[k = q][column r] and receives D[row 4 q + e][column r], e = 0..3.
// The k walk of every product is the same: groups g of 16, step e of a group takes k = 16 g + 4 q + e from lane q (one
// float4 of the A row per group), so a row's sums depend on that row's inputs only and have one fixed order.
//   h2     16 x 32, K = 128: wave = 2 kq + t forms K quarter kq of column tile t; the four partials are summed from
//          LDS in the order 0..3, then + b2 and act_fn (a 32-MFMA chain in two waves cost 4x the 8 of a quarter)
//   logits 16 x C,  K = 32:  wave w < ceil(C / 16) forms classes 16 w .. 16 w + 15, then + b3
//   d_z2   16 x 32, K = C:   wave 4 + 2 kh + t forms class half kh (32 classes) of column tile t, groups of 16 classes
//          wholly past C left out; the two partials are summed in the order 0, 1, then gate_fn
//   d_z1   16 x 128, K = 32: wave w forms columns 16 w .. 16 w + 15, gate_fn on the accumulator
// The B fragments come straight from global memory at kernel entry (24 floats per lane, beside the other entry loads);
// classes >= C are read from a clamped address and replaced by exact zeros on both operands where they are used.
struct TailFrags {
  float w2f[8];  // h2:   w2[16 t + r][32 kq + 16 g + 4 q + e]
  float w2b[8];  // d_z1: w2[16 g + 4 q + e][16 wave + r]
  float w3f[8];  // waves 0..3 (logits): w3[16 wave + r][16 g + 4 q + e]; waves 4..7 (d_z2): w3[32 kh + 16 g + 4 q + e][16 t + r]
  float b3v;     // b3[16 (wave & 3) + r]
};

template <int L2, int L3>
__device__ __forceinline__ void tail_load_frags(TailFrags& f, const float* __restrict__ w2, const float* __restrict__ w3,
                                                const float* __restrict__ b3, int C, int wave, int r, int q) {
  static_assert(L2 == 128 && L3 == 32, "tail_load_frags: the wave roles are laid out for 128 / 32");
  const int t = wave & 1, kq = wave >> 1, kh = (wave >> 1) & 1;
  const bool lg = wave < 4;  // wave-uniform
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = 16 * (i >> 2) + 4 * q + (i & 3);
    f.w2f[i] = w2[(16 * t + r) * L2 + 32 * kq + k];
    f.w2b[i] = w2[k * L2 + 16 * wave + r];
    const int cls = lg ? 16 * wave + r : 32 * kh + k, unit = lg ? k : 16 * t + r;
    f.w3f[i] = w3[min(cls, C - 1) * L3 + unit];
  }
  f.b3v = b3[min(16 * (wave & 3) + r, C - 1)];
}

// acc += A B over one group of 16 k: a = the lane's float4 of its A row, b = its four B values
__device__ __forceinline__ f32x4 tail_mma4(const float4& a, float b0, float b1, float b2, float b3, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b2, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b3, acc, 0, 0, 0);
  return acc;
}

// DX: the d_x tiles follow the tail (phases 123).  !DX: the tail alone, one workgroup per row tile (n_cg = 1; x, w1 and
// d_x are not read) -- what every other phase combination runs at these shapes, so that all of them form the tail's
// values with the same arithmetic.
template <int L2, int L3, bool DX, bool SKIP = false, typename... Soft>
__global__ __launch_bounds__(kTdxThreads) void tail_dx_train_kernel(
    const float* __restrict__ part, int ksplit, const float* __restrict__ b1, const float* __restrict__ w2,
    const float* __restrict__ b2, const float* __restrict__ w3, const float* __restrict__ b3, float clip,
    const int64_t* __restrict__ labels, float scale_over_b, int B, int C, float* __restrict__ h1, float* __restrict__ h2,
    float* __restrict__ logits, float* __restrict__ sample_loss, float* __restrict__ d_logits, float* __restrict__ d_z1,
    float* __restrict__ d_z2, const float* __restrict__ x, const float* __restrict__ w1, int L1, float* __restrict__ d_x,
    int m_tiles, int n_cg NNUE_TDX_ABL_PARAM, Soft... soft) {
  constexpr bool SOFT = sizeof...(Soft) == 1;
  constexpr bool DISTILL = (std::is_same_v<Soft, DistillTargets> || ...);
  constexpr int T = kTdxRows, NT = kTdxThreads, NWAVE = NT / 64;
  constexpr int NI = T * L2 / 4 / NT;       // float4 slots of the tile's slab rows per thread
  constexpr int NCH = L2 / (16 * kBwxKC);   // K chunks of the d_x product
  static_assert(NI >= 1 && NI * NT * 4 == T * L2 && T * L3 == NT && NWAVE == 8 && T == 16,
                "tail_dx_train_kernel: unsupported layer widths");
  // rows are padded by 4 floats: the 16 rows' float4 A reads of one k group then fall in 16 different bank groups
  __shared__ __attribute__((aligned(16))) float h1s[T][L2 + 4];
  __shared__ __attribute__((aligned(16))) float dz1s[T][L2 + 4];
  __shared__ __attribute__((aligned(16))) float h2s[T][L3 + 4];
  __shared__ __attribute__((aligned(16))) float dz2s[T][L3 + 4];
  __shared__ float ps[T][4][L3];  // partial h2 sums [row][K quarter][unit], then partial d_z2 sums [row][class half][unit]
  __shared__ __attribute__((aligned(16))) float lgs[T][kTdxMaxC + 4];  // logits, then d_logits
  __shared__ int64_t ys[SOFT ? 3 * T : T];  // SOFT: then the second labels, then lam (its bits)
  __shared__ f32x4 xch[DX ? NWAVE : 1][64];  // d_x accumulators swapped between the two waves of a pair

  const int blk = blockIdx.x, slot = blk >> 3;
  const int mt = (slot / n_cg) * 8 + (blk & 7), cg = slot % n_cg;
  if (mt >= m_tiles) return;  // whole workgroup (the numbering rounds the tile count up to a multiple of 8)
  const bool writer = cg == 0;
  const int row0 = mt * T;
  const int tid = threadIdx.x;
  constexpr bool skip = SKIP;
  NNUE_TDX_CLOCK(0);

  // ---- the d_x operands: a pair of 16-column tiles (c0, c0 + L1/2) per two waves, one tile per wave; this wave's W1
  // column slice and the x values of its epilogue are requested first and used after the tail
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int r = lane & 15, q = lane >> 4;
  const int half = L1 / 2;
  const int hi = wave & 1;  // 0: tile c0 (acc0 of l1_backward_x_body), 1: tile c1 (acc1)
  const int c0 = (cg * (NWAVE / 2) + (wave >> 1)) * 16, c1 = c0 + half, cm = hi ? c1 : c0;
  int orows[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) orows[e] = row0 + 4 * q + e;
  float bw[NCH][kBwxKC][4];
  float xv[4];  // the c1 tile's wave multiplies by x[c0], the c0 tile's by x[c1]
  if constexpr (DX) {
#pragma unroll
    for (int n = 0; n < NCH; ++n) bwx_load_b_tile(bw[n], w1, n * 16 * kBwxKC, L1, L2, cm, r, q);
#pragma unroll
    for (int e = 0; e < 4; ++e) xv[e] = x[(size_t)min(orows[e], B - 1) * L1 + (hi ? c0 : c1) + r];  // a padding row stores nothing
  }

  // ---- then the small products' B fragments, biases, labels and the slabs.  Every load is unconditional from an
  // in-bounds address and masked afterwards: a guarded load becomes a branch with a wait of its own.
  TailFrags fr;
  tail_load_frags<L2, L3>(fr, w2, w3, b3, C, wave, r, q);
  const float b2v = b2[tid % L3];
  const int64_t yv = labels[min(row0 + (tid % T), B - 1)];
  int64_t y2v = yv;
  float lamv = 1.0f, eps = 0.0f;
  if constexpr (SOFT) {
    const SoftTargets st = (soft, ...);
    eps = st.eps;
    if (st.labels_b) y2v = st.labels_b[min(row0 + (tid % T), B - 1)], lamv = st.lam[min(row0 + (tid % T), B - 1)];  // uniform
  }
  // DISTILL: the teacher logit of class `lane` of each row this wave takes in the softmax phase below (rows wave,
  // wave + NWAVE): one coalesced float per lane and row, requested here so that the slab sum hides its latency; a lane
  // past C and a padding row read a clamped address and feed nothing
  float alpha = 0.0f, tmp = 1.0f, uv[T / NWAVE];
  if constexpr (DISTILL) {
    const DistillTargets dt = (soft, ...);
    alpha = dt.alpha, tmp = dt.temperature;
#pragma unroll
    for (int it = 0; it < T / NWAVE; ++it) uv[it] = dt.teacher[(size_t)min(row0 + wave + NWAVE * it, B - 1) * C + min(lane, C - 1)];
  }
  int srow[NI], scol[NI];
  float4 z4[NI];
  const float* prow[NI];  // this thread's slab row (a padding row of the last tile reads row B - 1: it feeds no output)
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int f = tid + NT * i;
    srow[i] = f / (L2 / 4);
    scol[i] = 4 * (f % (L2 / 4));
    prow[i] = part + (size_t)min(row0 + srow[i], B - 1) * L2 + scol[i];
    z4[i] = make_float4(b1[scol[i]], b1[scol[i] + 1], b1[scol[i] + 2], b1[scol[i] + 3]);
  }
  // z = b1[j] + part[0] + part[1] + ... in slab order, in batches of 16 slabs whose loads are all in flight together (a
  // slab past the end re-reads the last one and is not added -- skipped, not added as 0, which would turn a -0 into +0)
  const size_t slab = (size_t)B * L2;
  auto load_batch = [&](int s0, float4 (&v)[NI][16]) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int u = 0; u < 16; ++u) v[i][u] = *reinterpret_cast<const float4*>(prow[i] + (size_t)min(s0 + u, ksplit - 1) * slab);
  };
  auto sum_batch = [&](int s0, const float4 (&v)[NI][16]) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const bool add = s0 + u < ksplit;  // uniform
        z4[i].x = add ? z4[i].x + v[i][u].x : z4[i].x;
        z4[i].y = add ? z4[i].y + v[i][u].y : z4[i].y;
        z4[i].z = add ? z4[i].z + v[i][u].z : z4[i].z;
        z4[i].w = add ? z4[i].w + v[i][u].w : z4[i].w;
      }
  };
  {
    float4 v[NI][16];
    load_batch(0, v);
    if (tid < T) ys[tid] = row0 + tid < B ? yv : -1;
    if constexpr (SOFT) {
      if (tid < T) ys[T + tid] = y2v, ys[2 * T + tid] = __float_as_int(lamv);
    }
    sum_batch(0, v);
  }
  for (int s0 = 16; s0 < ksplit; s0 += 16) {
    float4 v[NI][16];
    load_batch(s0, v);
    sum_batch(s0, v);
  }

  // ---- h1 = act(z)
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    float4 h;
    h.x = act_fn(z4[i].x, clip); h.y = act_fn(z4[i].y, clip); h.z = act_fn(z4[i].z, clip); h.w = act_fn(z4[i].w, clip);
    *reinterpret_cast<float4*>(&h1s[srow[i]][scol[i]]) = h;
    if (writer && row0 + srow[i] < B) *reinterpret_cast<float4*>(h1 + (size_t)(row0 + srow[i]) * L2 + scol[i]) = h;
  }
  __syncthreads();
  NNUE_TDX_CLOCK(1);

  const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int orow_t = tid / L3, ounit = tid % L3;  // the (row, unit) of T x L3 values this thread finishes
  // ---- h2 = act(w2 h1 + b2): K quarter kq of column tile t per wave, then the quarters in order
  {
    const int t = wave & 1, kq = wave >> 1;
    f32x4 acc = zero4;
    if constexpr (!skip) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const float4 a = *reinterpret_cast<const float4*>(&h1s[r][32 * kq + 16 * g + 4 * q]);
        acc = tail_mma4(a, fr.w2f[4 * g], fr.w2f[4 * g + 1], fr.w2f[4 * g + 2], fr.w2f[4 * g + 3], acc);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) ps[4 * q + e][kq][16 * t + r] = acc[e];
  }
  __syncthreads();
  NNUE_TDX_CLOCK(2);
  {
    float z = ps[orow_t][0][ounit];
    z += ps[orow_t][1][ounit];
    z += ps[orow_t][2][ounit];
    z += ps[orow_t][3][ounit];
    const float h = act_fn(z + b2v, clip);
    h2s[orow_t][ounit] = h;
    if (writer && row0 + orow_t < B) h2[(size_t)(row0 + orow_t) * L3 + ounit] = h;
  }
  __syncthreads();
  NNUE_TDX_CLOCK(3);
  // ---- logits = w3 h2 + b3: classes 16 wave .. 16 wave + 15 in wave < ceil(C / 16); the others go on to the barrier
  if (16 * wave < C) {  // wave-uniform; C <= kTdxMaxC = 64: waves 0..3, the ones that hold the logits fragments
    const int n = 16 * wave + r;
    const bool n_in = n < C;
    f32x4 acc = zero4;
    if constexpr (!skip) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const float4 a = *reinterpret_cast<const float4*>(&h2s[r][16 * g + 4 * q]);
        acc = tail_mma4(a, n_in ? fr.w3f[4 * g] : 0.f, n_in ? fr.w3f[4 * g + 1] : 0.f, n_in ? fr.w3f[4 * g + 2] : 0.f,
                        n_in ? fr.w3f[4 * g + 3] : 0.f, acc);
      }
    }
    if (n_in) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int rr = 4 * q + e;
        const float z = acc[e] + fr.b3v;
        lgs[rr][n] = z;
        if (writer && row0 + rr < B) logits[(size_t)(row0 + rr) * C + n] = z;
      }
    }
  }
  __syncthreads();
  NNUE_TDX_CLOCK(4);
  // ---- softmax cross-entropy and d_logits: rows wave, wave + NWAVE, ... of the tile (interleaved), lane = class
  {
    constexpr int RW = T / NWAVE;
    const bool in = lane < C;
    float v[RW], mx[RW], se[RW];
#pragma unroll
    for (int it = 0; it < RW; ++it) v[it] = in ? lgs[wave + NWAVE * it][lane] : -INFINITY;
    float cs[RW];  // SOFT: sum_c (mx - z_c), the smoothing term
    float mu[RW], eu[RW], ez[RW], sU[RW], sT[RW], ks[RW];  // DISTILL: the teacher's max, the numerators of q and pT, the three sums
    if constexpr (DISTILL) ce_wave_distill<RW, true>(v, uv, in, tmp, mx, se, cs, mu, eu, ez, sU, sT, ks);
    else ce_wave_stats_fast<RW>(v, in, mx, se);
    if constexpr (SOFT && !DISTILL) ce_wave_csum<RW, true>(v, in, mx, cs);
#pragma unroll
    for (int it = 0; it < RW; ++it) {
      const int rr = wave + NWAVE * it;
      const int64_t y = ys[rr];
      int64_t y2 = y;
      float lam = 1.0f;
      if constexpr (SOFT) y2 = ys[T + rr], lam = __int_as_float((int)ys[2 * T + rr]);
      const bool ok = SOFT ? nnue_soft_counts(y, y2, lam, C) : y >= 0 && y < C;
      const float zy = ok ? lgs[rr][y] : 0.f;  // read by every lane before any lane overwrites its logit
      if constexpr (SOFT) {
        const float zy2 = ok ? lgs[rr][y2 >= 0 && y2 < C ? y2 : y] : 0.f;
        if constexpr (DISTILL) {
          if (writer && lane == 0 && row0 + rr < B) {
            const float ls = ok ? nnue_ce_soft_sample_loss(mx[it], zy, zy2, se[it], cs[it], lam, eps, C) : 0.0f;
            sample_loss[row0 + rr] = ok ? nnue_distill_sample_loss(ls, sT[it], sU[it], ks[it], alpha, tmp) : 0.0f;
          }
        } else if (writer && lane == 0 && row0 + rr < B)
          sample_loss[row0 + rr] = ok ? nnue_ce_soft_sample_loss(mx[it], zy, zy2, se[it], cs[it], lam, eps, C) : 0.0f;
      } else {
        if (writer && lane == 0 && row0 + rr < B) sample_loss[row0 + rr] = ok ? nnue_ce_sample_loss(mx[it], zy, se[it]) : 0.0f;
      }
      const float inv = 1.0f / se[it];
      if (in) {
        float g;
        if constexpr (DISTILL) {
          const float soft_g = fmaf(expf(v[it] - mx[it]), inv, -nnue_soft_target(lane == y, lane == y2, lam, eps, C));
          g = ok ? nnue_distill_dlogit(soft_g, ez[it], 1.0f / sT[it], eu[it], 1.0f / sU[it], alpha, tmp, scale_over_b) : 0.0f;
        } else if constexpr (SOFT) g = ok ? ce_dlogit_soft(v[it], mx[it], inv, nnue_soft_target(lane == y, lane == y2, lam, eps, C), scale_over_b) : 0.0f;
        else g = ok ? ce_dlogit(v[it], mx[it], inv, lane == y, scale_over_b) : 0.0f;
        lgs[rr][lane] = g;
        if (writer && row0 + rr < B) d_logits[(size_t)(row0 + rr) * C + lane] = g;
      }
    }
  }
  __syncthreads();
  NNUE_TDX_CLOCK(5);
  // ---- d_z2 = gate(w3^T d_logits): class half kh of column tile t in wave 4 + 2 kh + t, then the halves in order
  if (wave >= 4) {
    const int t = wave & 1, kh = (wave >> 1) & 1;
    f32x4 acc = zero4;
    if constexpr (!skip) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int cb = 32 * kh + 16 * g;
        if (cb < C) {  // uniform: a group of 16 classes wholly past C adds nothing
          const int c = cb + 4 * q;
          float4 a = *reinterpret_cast<const float4*>(&lgs[r][c]);  // LDS past class C was never written: select, not multiply
          a.x = c < C ? a.x : 0.f; a.y = c + 1 < C ? a.y : 0.f; a.z = c + 2 < C ? a.z : 0.f; a.w = c + 3 < C ? a.w : 0.f;
          acc = tail_mma4(a, c < C ? fr.w3f[4 * g] : 0.f, c + 1 < C ? fr.w3f[4 * g + 1] : 0.f, c + 2 < C ? fr.w3f[4 * g + 2] : 0.f,
                          c + 3 < C ? fr.w3f[4 * g + 3] : 0.f, acc);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) ps[4 * q + e][kh][16 * t + r] = acc[e];
  }
  __syncthreads();
  NNUE_TDX_CLOCK(6);
  {
    const float s = ps[orow_t][0][ounit] + ps[orow_t][1][ounit];
    const float v = gate_fn(s, h2s[orow_t][ounit], clip);
    dz2s[orow_t][ounit] = v;
    if (writer && row0 + orow_t < B) d_z2[(size_t)(row0 + orow_t) * L3 + ounit] = v;
  }
  __syncthreads();
  NNUE_TDX_CLOCK(7);
  // ---- d_z1 = gate(w2^T d_z2): columns 16 wave .. 16 wave + 15 per wave
  {
    f32x4 acc = zero4;
    if constexpr (!skip) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const float4 a = *reinterpret_cast<const float4*>(&dz2s[r][16 * g + 4 * q]);
        acc = tail_mma4(a, fr.w2b[4 * g], fr.w2b[4 * g + 1], fr.w2b[4 * g + 2], fr.w2b[4 * g + 3], acc);
      }
    }
    const int k = 16 * wave + r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int rr = 4 * q + e;
      const float v = gate_fn(acc[e], h1s[rr][k], clip);
      dz1s[rr][k] = v;
      if (writer && row0 + rr < B) d_z1[(size_t)(row0 + rr) * L2 + k] = v;
    }
  }
  __syncthreads();
  NNUE_TDX_CLOCK(8);
  // ---- d_x: this wave's tile with l1_backward_x_body's operands and MFMA order, then the pairwise epilogue with the
  // partner wave's accumulator
  if constexpr (DX) {
    const bool row_ok = row0 + r < B;
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int n = 0; n < NCH; ++n) {
      BwxChunk ch;
      bwx_load_a(ch, &dz1s[r][0], row_ok, n * 16 * kBwxKC, L2, q);
      bwx_mma_tile(ch.a, bw[n], acc);
    }
    xch[wave][lane] = acc;
    __syncthreads();
    const f32x4 other = xch[wave ^ 1][lane];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int orow = orows[e];
      if (orow >= B) continue;
      float* __restrict__ o = d_x + (size_t)orow * L1;
      if (hi) o[c1 + r] = other[e] * xv[e];           // acc0 * x[c0]
      else o[c0 + r] = fmaf(acc[e], xv[e], other[e]);  // fma(acc0, x[c1], acc1)
    }
  }
  NNUE_TDX_CLOCK(9);
}

// ---- bucket selector + grouping (one workgroup; B a few thousand at most matters for speed, any B is correct) -----
// bucket[b] = min(K-1, n[b] * K / (P + 1))  (P = flat ids of the map; P == 0: n[b] already IS the bucket, clamped)
// then a stable counting sort of the samples into bucket-homogeneous 16-row tiles.
#include "bucket_group.h"

constexpr int kGroupThreads = 1024;  // one pass over a batch of 1024: every phase of the kernel is a latency, not work
__global__ __launch_bounds__(kGroupThreads) void bucket_group_kernel(GroupArgs ga) {
  __shared__ int lds[kGroupLdsInts];
  bucket_group_body<kGroupThreads>(ga, lds);
}

}  // namespace

// d_x and the small weight/bias gradients + mean loss in one launch: both only read what the per-sample tail kernel
// left (d_z1 resp. d_logits, d_z2, h1, h2), so the two launch-sized jobs share the chip (x blocks first).
__global__ __launch_bounds__(256) void l1_backward_x_small_wgrad(const float* __restrict__ x, int pairwise, const float* __restrict__ w1,
                                                                 const float* __restrict__ d_z1, int B, int L1, int L2,
                                                                 float* __restrict__ d_x, int x_blocks, SmallWgrad a) {
  if ((int)blockIdx.x < x_blocks) l1_backward_x_body(x, pairwise, w1, d_z1, B, L1, L2, d_x, blockIdx.x, a.bk);
  else {
    __shared__ float red[1024];
    small_wgrad_body(a, (int)blockIdx.x - x_blocks, red);
  }
}

// =============================================================================== host half
// What the shape decides (ClsPlan), where things lie in scratch (BackwardLayout, TrainLayout), what one training-step call
// launches (TrainStepPlan), one launcher per product, and the C ABI.  Nothing below this line runs on the device.

// ---- timing-only hooks (NNUE_BUILD_ABLATIONS=1 of csrc/build.py; tools/debug/tail_abl.sh, tools/debug/tail_clocks.py): WRONG
// results by design.  The dispatch calls abl_skip_small() and launch_tail_dx_kernel() unconditionally; a default build has the
// constant and the plain forms.
#ifdef NNUE_ABLATIONS
namespace {
long long* g_tdx_clocks = nullptr;  // the last tail_dx_train_kernel launch's phase clocks (NNUE_CLS_ABL_TAIL_CLOCKS=1)
int g_tdx_clock_blocks = 0;
int abl_knob(const char* name) { const char* e = getenv(name); return e ? atoi(e) : 0; }
// the d_x blocks alone -- what the launch would cost if the small gradients rode elsewhere
bool abl_skip_small() { static const int v = abl_knob("NNUE_CLS_ABL_SKIP_SMALL"); return v != 0; }

template <bool DX, typename... Soft, typename... Args> void launch_tail_dx_kernel(int grid, hipStream_t s, std::tuple<Soft...> soft, Args... args) {
  static const int skip = abl_knob("NNUE_CLS_ABL_SKIP_TAIL_PRODUCTS"), clocks = abl_knob("NNUE_CLS_ABL_TAIL_CLOCKS");
  if (clocks && grid > g_tdx_clock_blocks) {  // eager launches only: this allocates
    if (g_tdx_clocks) (void)hipFree(g_tdx_clocks);
    g_tdx_clocks = nullptr;
    g_tdx_clock_blocks = hipMalloc(&g_tdx_clocks, (size_t)grid * kTdxClocks * sizeof(long long)) == hipSuccess ? grid : 0;
  }
  if (clocks && g_tdx_clocks) (void)hipMemsetAsync(g_tdx_clocks, 0, (size_t)g_tdx_clock_blocks * kTdxClocks * sizeof(long long), s);
  const TdxAbl abl{clocks ? g_tdx_clocks : nullptr};
  std::apply([&](auto... st) {
    if (skip) hipLaunchKernelGGL((tail_dx_train_kernel<128, 32, DX, true, Soft...>), dim3(grid), dim3(kTdxThreads), 0, s, args..., abl, st...);
    else hipLaunchKernelGGL((tail_dx_train_kernel<128, 32, DX, false, Soft...>), dim3(grid), dim3(kTdxThreads), 0, s, args..., abl, st...);
  }, soft);
}
}  // namespace

// the phase clocks of the last tail_dx_train_kernel launch: out[workgroup][kTdxClocks]; returns the workgroup count (or -1)
extern "C" int nnue_cls_abl_tail_clocks(long long* out, int max_blocks) {
  if (!g_tdx_clocks || !out) return -1;
  const int n = g_tdx_clock_blocks < max_blocks ? g_tdx_clock_blocks : max_blocks;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpy(out, g_tdx_clocks, (size_t)n * kTdxClocks * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return n;
}
#else
namespace {
constexpr bool abl_skip_small() { return false; }
// soft: empty (the plain kernel) or one SoftTargets, the kernel's trailing argument
template <bool DX, typename... Soft, typename... Args> void launch_tail_dx_kernel(int grid, hipStream_t s, std::tuple<Soft...> soft, Args... args) {
  std::apply([&](auto... st) {
    hipLaunchKernelGGL((tail_dx_train_kernel<128, 32, DX, false, Soft...>), dim3(grid), dim3(kTdxThreads), 0, s, args..., st...);
  }, soft);
}
}  // namespace
#endif

namespace {

// ------------------------------------------------------------------ shape policy (shared by scratch + launch)
struct ClsPlan {
  bool fwd_mfma, bww_mfma, bwx_mfma;
  int fwd_ksplit;            // K slabs of the forward partial sums
  int bww_ksplit, bww_klen;  // batch slabs of d_w1
};

int bucket_tiles(int B, int K) { return (B + 15) / 16 + K; }  // sum_k ceil(c_k / 16) <= B / 16 + K
// 16-row tiles of the first-layer products; a grouping (buckets_from) was made for bucket_tiles(B, K) of them
int row_tiles(int B, int K) { return K > 1 ? bucket_tiles(B, K) : (B + 15) / 16; }

// tail_dx_train_kernel's shapes: one layer stack, the pairwise block, whole 4-wave column groups, a wave per row of
// logits, and the layer widths it is instantiated for (those of every shipped configuration)
bool tail_dx_supported(int B, int L1, int L2, int L3, int C, int K, int pairwise) {
  return B > 0 && K == 1 && pairwise && L1 > 0 && L1 % 128 == 0 && C >= 1 && C <= kTdxMaxC && L2 == 128 && L3 == 32;
}

ClsPlan make_plan(int B, int L1, int L2, int pairwise, int K = 1) {
  ClsPlan p{};
  p.fwd_mfma = (L1 % 32 == 0) && (L2 % 16 == 0);
  p.fwd_ksplit = 1;
  if (p.fwd_mfma) {
    // enough K slabs for >= ~1024 waves, each slab a multiple of 16 and (pairwise) inside one half
    const int tiles = row_tiles(B, K) * ((L2 + 63) / 64);
    int ks = 1;
    while (tiles * ks < 1024 && L1 % (ks * 2 * 16) == 0 && L1 / (ks * 2) >= 64) ks *= 2;
    if (pairwise && ks == 1) ks = 2;
    static const int force_ks = [] { const char* e = getenv("NNUE_CLS_FWD_KSPLIT"); return e ? atoi(e) : 0; }();  // developer knob
    if (force_ks >= 2 && (force_ks & (force_ks - 1)) == 0 && L1 % (force_ks * 16) == 0 && L1 / force_ks >= 32) ks = force_ks;
    p.fwd_ksplit = ks;
  }
  p.bww_mfma = (L1 % 64 == 0) && (L2 % 32 == 0);
  p.bww_ksplit = 1;
  p.bww_klen = B;
  if (p.bww_mfma) {
    // K > 1, per bucket: slices of klen rows of its own segment; a bucket that holds every sample gets ks slices, one that
    // holds B / K of them one -- the number of non-empty slices (= slabs written and summed) is <= ks + K
    const int tiles = (L2 / 32) * (L1 / 64), want = K > 1 ? 512 : 1024, min_rows = K > 1 ? 64 : 32, unit = K > 1 ? 16 : 4;
    int ks = 1;
    while (tiles * ks < want && B / (ks * 2) >= min_rows) ks *= 2;
    p.bww_ksplit = ks;
    p.bww_klen = ((B + ks - 1) / ks + unit - 1) / unit * unit;
  }
  p.bwx_mfma = (L1 % 32 == 0) && (L2 % 16 == 0);
  return p;
}

// d_w1 is formed as bww_ksplit batch slabs per stack that a second pass sums (MFMA form only: make_plan splits nothing else)
bool slab_pass(const ClsPlan& p) { return p.bww_mfma && p.bww_ksplit > 1; }
long long dw1_floats(int K, int L1, int L2) { return (long long)K * L2 * L1; }
int64_t slab_floats(const ClsPlan& p, int L1, int L2, int K) { return p.bww_ksplit > 1 ? (int64_t)p.bww_ksplit * dw1_floats(K, L1, L2) : 0; }
unsigned slab_sum_blocks(long long count) { return (unsigned)((count / 4 + 255) / 256); }  // a float4 per thread

// ------------------------------------------------------------------ scratch layouts (float offsets): one author each
// nnue_classifier_forward keeps its fwd_ksplit partial sums at the start of the buffer, nnue_classifier_backward d_z1, d_z2
// and the d_w1 slabs; `total` covers whichever is more.
struct BackwardLayout { int64_t part, d_z1, d_z2, slabs, total; };
BackwardLayout backward_layout(const ClsPlan& p, int B, int L1, int L2, int L3, int K = 1) {
  BackwardLayout t{};
  t.part = t.d_z1 = 0;  // the two calls use the buffer one after the other
  t.d_z2 = t.d_z1 + nnue_round_up((int64_t)B * L2, 4);
  t.slabs = t.d_z2 + nnue_round_up((int64_t)B * L3, 4);
  // The total is the one nnue_classifier_scratch has always answered: the UNROUNDED sizes + 64 floats.  The two round-ups
  // above take at most 6 of the 64; the other 58 are slack.
  const int64_t fwd = (int64_t)p.fwd_ksplit * B * L2;
  const int64_t bwd = (int64_t)B * L2 + (int64_t)B * L3 + slab_floats(p, L1, L2, K);
  t.total = (fwd > bwd ? fwd : bwd) + 64;
  return t;
}

struct TrainLayout { int64_t part, d_z1, d_z2, d_logits, slabs, d_z1_g, x_g, total; };
TrainLayout train_layout(const ClsPlan& p, int B, int L1, int L2, int L3, int C, int K = 1) {
  TrainLayout t{};
  int64_t off = 0;
  auto take = [&](int64_t n) { const int64_t o = off; off += nnue_round_up(n, 4); return o; };
  // the layer-1 slabs come from this module's own forward (fwd_ksplit of them) or from the fused FeatureTransformer
  // forward (one per 64 columns of L1, NNUE_CLS_L1_SLABS_GIVEN): room for whichever is more
  const int64_t ext = (L1 % 64 == 0) ? L1 / 64 : 0;
  t.part = take((p.fwd_ksplit > ext ? (int64_t)p.fwd_ksplit : ext) * B * L2);
  t.d_z1 = take((int64_t)B * L2);
  t.d_z2 = take((int64_t)B * L3);
  t.d_logits = take((int64_t)B * C);
  t.slabs = take(slab_floats(p, L1, L2, K));
  // bucketed stacks: grouped-row copies of d_z1 and of the block's input for the d_w1 product in nnue_ftm_backward_bucketed
  const int64_t grows = K > 1 ? (int64_t)bucket_tiles(B, K) * 16 : 0;
  t.d_z1_g = take(grows * L2);
  t.x_g = take(grows * L1);
  t.total = off + 4;
  return t;
}

// ------------------------------------------------------------------ the plan of one nnue_classifier_train_step call
constexpr int kClsBothPhases = NNUE_CLS_PHASE_DX | NNUE_CLS_PHASE_SMALL;
constexpr int kClsPhaseBits = kClsBothPhases | NNUE_CLS_DW1_BESIDE_DX | NNUE_CLS_L1_SLABS_GIVEN | NNUE_CLS_DW1_RIDES | NNUE_CLS_SMALL_RIDE;
// NNUE_CLS_TAIL_IN_DX exists in one combination only: on top of everything that leaves this call nothing but d_x
constexpr int kClsFusedStep = (kClsPhaseBits & ~NNUE_CLS_DW1_BESIDE_DX) | NNUE_CLS_TAIL_IN_DX;

bool phases_valid(int ph) {
  constexpr int ride_needs = kClsBothPhases | NNUE_CLS_DW1_RIDES;
  if (ph == kClsFusedStep) return true;
  if ((ph & ~kClsPhaseBits) || !(ph & kClsBothPhases)) return false;  // a negative value has bits outside the mask
  if ((ph & NNUE_CLS_DW1_BESIDE_DX) && (ph & NNUE_CLS_DW1_RIDES)) return false;
  return !(ph & NNUE_CLS_SMALL_RIDE) || (ph & ride_needs) == ride_needs;
}

// The checks that need nothing but the plan's inputs: the first one the call fails, in the order the call has always made
// them.  The entry point words them, with its pointer checks in between.
enum class Refusal { none, bad_phases, slabs_many_stacks, dw1_rides_stack_shape, slabs_shape, sizes, odd_l1, tail_lds, small_ride_no_dx,
                     fused_tail_shape };
enum class TailLaunch { none, tile, sample128, sample512 };  // tail_dx_train_kernel without d_x tiles, or tail_train_kernel<NT, vec>
// with_tail: tail_dx_train_kernel with its d_x tiles (kClsFusedStep), the whole call | with_dw1: l1_backward_xw_mfma, the d_w1
// product beside d_x (NNUE_CLS_DW1_BESIDE_DX) | with_small: l1_backward_x_small_wgrad, where the small gradients and the mean
// loss ride (dx_hosts_small) or could | alone: launch_l1_backward_x
enum class DxLaunch { none, with_tail, with_dw1, with_small, alone };

struct TrainStepPlan {
  Refusal refusal;
  ClsPlan p;
  TrainLayout t;
  bool l1_forward;                  // launch_l1_forward (false: NNUE_CLS_L1_SLABS_GIVEN, or no NNUE_CLS_PHASE_DX)
  TailLaunch tail;
  bool tail_vec;                    // tail_train_kernel's float4 form
  int tail_grid, tail_slabs;        // tail_train_kernel: a workgroup per sample or per grouped row; layer-1 slabs either tail sums
  int64_t tail_lds;                 // bytes
  int tdx_cg, tdx_grid;             // tail_dx_train_kernel: column groups per row tile, workgroups
  bool grouped;                     // K > 1 with d_w1 left to nnue_ftm_backward_bucketed: the tail also leaves that product's grouped operands
  DxLaunch dx;
  bool dx_hosts_small;              // with_small: false under NNUE_CLS_SMALL_RIDE (they ride in nnue_ftm_backward's launch instead)
  bool dw1_product, small_wgrad;    // NNUE_CLS_PHASE_SMALL: launch_l1_backward_w; small_wgrad_kernel, with the piggy-backed d_w1 slab sum:
  int sum_slabs, slab_blocks;       // slabs it sums (0: none) in that many workgroups more
};

TrainStepPlan train_step_plan(int pairwise, int B, int L1, int L2, int L3, int C, int K, int phases, bool want_dx, bool tail_vec_ok) {
  // The entry point calls this before it has checked the sizes: nothing above Refusal::sizes reads more of them than L1 % n,
  // and make_plan and the layouts are reached only with positive sizes.
  TrainStepPlan sp{};
  auto refuse = [&](Refusal r) { sp.refusal = r; return sp; };
  if (!phases_valid(phases)) return refuse(Refusal::bad_phases);
  const bool fused = phases == kClsFusedStep;
  const bool slabs_given = phases & NNUE_CLS_L1_SLABS_GIVEN, dw1_rides = phases & NNUE_CLS_DW1_RIDES;
  const bool small_ride = phases & NNUE_CLS_SMALL_RIDE, beside = phases & NNUE_CLS_DW1_BESIDE_DX;
  if (K != 1 && slabs_given) return refuse(Refusal::slabs_many_stacks);
  if (K != 1 && dw1_rides && !(pairwise && L1 % 4 == 0)) return refuse(Refusal::dw1_rides_stack_shape);
  if (slabs_given && !(pairwise && L1 % 64 == 0)) return refuse(Refusal::slabs_shape);
  if (!(B > 0 && L1 > 0 && L2 > 0 && L3 > 0 && C > 0)) return refuse(Refusal::sizes);
  if (pairwise && L1 % 2 != 0) return refuse(Refusal::odd_l1);
  sp.tail_lds = ((int64_t)L2 + 2 * L3 + C + 8) * 4;
  if (sp.tail_lds > 64 * 1024) return refuse(Refusal::tail_lds);
  const ClsPlan& p = sp.p = make_plan(B, L1, L2, pairwise, K);
  sp.t = train_layout(p, B, L1, L2, L3, C, K);
  sp.grouped = K > 1 && dw1_rides;
  sp.tail_grid = sp.grouped ? bucket_tiles(B, K) * 16 : B;
  sp.tail_slabs = slabs_given ? L1 / 64 : p.fwd_ksplit;
  sp.sum_slabs = slab_pass(p) && !dw1_rides ? p.bww_ksplit : 0;
  sp.slab_blocks = sp.sum_slabs ? (int)slab_sum_blocks(dw1_floats(K, L1, L2)) : 0;
  // the d_w1 product runs in the d_x launch (both MFMA forms, d_x requested); a later NNUE_CLS_PHASE_SMALL call with the same
  // bit then only sums its slabs
  const bool early_bww = beside && p.bwx_mfma && p.bww_mfma && want_dx;
  // both phases in one call with d_w1 left to nnue_ftm_backward: the small gradients ride in the d_x launch
  const bool small_in_dx = (phases & kClsBothPhases) == kClsBothPhases && dw1_rides && p.bwx_mfma && want_dx;
  if (small_ride && !small_in_dx) return refuse(Refusal::small_ride_no_dx);
  // The tile tail (tail_dx_train_kernel): at every shape the fused predicate takes, EVERY phase combination forms the
  // per-sample tail with it -- followed by the d_x tiles in the same launch (kClsFusedStep) or alone, one workgroup per row
  // tile -- so that the launch forms agree bitwise.  Every other shape keeps tail_train_kernel.
  const bool tile_tail = tail_dx_supported(B, L1, L2, L3, C, K, pairwise);
  if (fused && !tile_tail) return refuse(Refusal::fused_tail_shape);
  sp.tdx_cg = fused ? L1 / 32 / (kTdxThreads / 128) : 1;  // pairs of 16-column tiles / pairs per workgroup
  sp.tdx_grid = (row_tiles(B, K) + 7) / 8 * 8 * sp.tdx_cg;
  // fused: the slabs are in scratch, d_w1 and the small gradients ride in nnue_ftm_backward's launch (small_in_dx holds)
  if (fused) sp.dx = DxLaunch::with_tail;
  else if (phases & NNUE_CLS_PHASE_DX) {
    sp.l1_forward = !slabs_given;  // else part[L1/64][B][L2] was written by nnue_ftm_forward_l1 (the FeatureTransformer forward's epilogue)
    sp.tail = tile_tail ? TailLaunch::tile : C > 256 ? TailLaunch::sample512 : TailLaunch::sample128;
    sp.tail_vec = L2 % 4 == 0 && L3 % 4 == 0 && tail_vec_ok;
    if (want_dx) sp.dx = early_bww ? DxLaunch::with_dw1 : small_in_dx ? DxLaunch::with_small : DxLaunch::alone;
    sp.dx_hosts_small = sp.dx == DxLaunch::with_small && !small_ride;
  }
  if ((phases & NNUE_CLS_PHASE_SMALL) && !small_in_dx) {  // needs NNUE_CLS_PHASE_DX's h1, h2, d_logits, d_z1, d_z2 (scratch)
    sp.dw1_product = !early_bww && !dw1_rides;  // else it ran beside d_x, or rides in nnue_ftm_backward's launch
    sp.small_wgrad = true;
  }
  return sp;
}

// ------------------------------------------------------------------ one launcher per product
// what every first-layer product reads
struct L1Call { const float* x; int pairwise, B, L1, L2; Buckets bk; hipStream_t s; };
unsigned wave_blocks(long long waves) { return (unsigned)((waves + 3) / 4); }  // 256-thread workgroups of four waves
// workgroups of the MFMA d_x product and of the MFMA d_w1 product
int bwx_blocks(const L1Call& c) { return (int)wave_blocks((long long)row_tiles(c.B, c.bk.K) * (c.L1 / 32)); }
int bww_blocks(const ClsPlan& p, const L1Call& c) { return (int)wave_blocks((long long)c.bk.K * (c.L2 / 32) * (c.L1 / 64) * p.bww_ksplit); }

// part[fwd_ksplit][B][L2] = slabs of l0 W1^T
void launch_l1_forward(const ClsPlan& p, const L1Call& c, const float* w1, float* part) {
  if (p.fwd_mfma)
    hipLaunchKernelGGL(l1_forward_mfma, dim3(wave_blocks((long long)row_tiles(c.B, c.bk.K) * ((c.L2 + 63) / 64) * p.fwd_ksplit)), dim3(256),
                       0, c.s, c.x, c.pairwise, w1, c.B, c.L1, c.L2, p.fwd_ksplit, part, c.bk);
  else
    hipLaunchKernelGGL(l1_forward_simple, dim3(wave_blocks((long long)c.B * c.L2)), dim3(256), 0, c.s, c.x, c.pairwise, w1, c.B, c.L1, c.L2,
                       part, c.bk);
}

// d_w1 = d_z1^T l0: into `slabs` where a slab pass follows (slab_pass(p)), else into d_w1
void launch_l1_backward_w(const ClsPlan& p, const L1Call& c, const float* d_z1, float* slabs, float* d_w1) {
  if (p.bww_mfma)
    hipLaunchKernelGGL(l1_backward_w_mfma, dim3((unsigned)bww_blocks(p, c)), dim3(256), 0, c.s, c.x, c.pairwise, d_z1, c.B, c.L1, c.L2,
                       p.bww_ksplit, p.bww_klen, slab_pass(p) ? slabs : d_w1, c.bk);
  else
    hipLaunchKernelGGL(l1_backward_w_simple, dim3(c.bk.K * c.L2, (c.L1 + 255) / 256), dim3(256), 0, c.s, c.x, c.pairwise, d_z1, c.B, c.L1,
                       c.L2, d_w1, c.bk);
}

// d_x = (d_z1 W1) through the pairwise block
void launch_l1_backward_x(const ClsPlan& p, const L1Call& c, const float* w1, const float* d_z1, float* d_x) {
  if (p.bwx_mfma)
    hipLaunchKernelGGL(l1_backward_x_mfma, dim3((unsigned)bwx_blocks(c)), dim3(256), 0, c.s, c.x, c.pairwise, w1, d_z1, c.B, c.L1, c.L2, d_x,
                       c.bk);
  else
    hipLaunchKernelGGL(l1_backward_x_simple, dim3(c.B, ((c.pairwise ? c.L1 / 2 : c.L1) + 255) / 256), dim3(256), 0, c.s, c.x, c.pairwise, w1,
                       d_z1, c.B, c.L1, c.L2, d_x, c.bk);
}

// The small-gradient family's arguments.  loss_out NULL: no mean-loss block (its workgroup is not counted).  The piggy-backed
// d_w1 slab sum runs where n_slabs > 0; slab_count is what the callers have always passed (0 from nnue_classifier_backward).
struct SlabSum { const float* slabs; int n_slabs; long long slab_count; float* d_w1; };
SmallWgrad small_wgrad_args(const ClsPlan& p, int B, int L2, int L3, int C, const Buckets& bk, const float* d_logits, const float* d_z2,
                            const float* d_z1, const float* h1, const float* h2, float* d_b1, float* d_w2, float* d_b2, float* d_w3,
                            float* d_b3, const float* sample_loss, float* loss_out, const SlabSum& sum) {
  SmallWgrad a{};
  a.d_logits = d_logits, a.d_z2 = d_z2, a.d_z1 = d_z1, a.h1 = h1, a.h2 = h2;
  a.B = B, a.L2 = L2, a.L3 = L3, a.C = C;
  a.d_w3 = d_w3, a.d_b3 = d_b3, a.d_w2 = d_w2, a.d_b2 = d_b2, a.d_b1 = d_b1;
  a.sample_loss = sample_loss, a.loss_out = loss_out;
  a.wgrad_blocks = small_wgrad_tiles(L2, L3, C) * bk.K + (loss_out ? 1 : 0);
  a.slabs = sum.slabs, a.n_slabs = sum.n_slabs, a.slab_count = sum.slab_count, a.d_w1 = sum.d_w1;
  a.bk = bk, a.bww_klen = p.bww_klen;
  return a;
}

// host-side check + conversion of the C struct; NULL or K == 1 -> the reference path whatever the pointers say
int buckets_from(const nnue_buckets* c, int B, Buckets* out, const char* who) {
  *out = Buckets{1, nullptr, nullptr, nullptr, nullptr, 0};
  if (!c || c->K <= 1) return NNUE_OK;
  NNUE_REQUIRE(c->K <= kMaxBuckets, NNUE_E_SHAPE, "%s: %d layer stacks (at most %d)", who, c->K, kMaxBuckets);
  NNUE_REQUIRE(c->bucket && c->rows && c->tile_bucket && c->seg, NNUE_E_ARG, "%s: null bucket pointer", who);
  NNUE_REQUIRE(c->tiles == bucket_tiles(B, c->K), NNUE_E_SHAPE, "%s: bucket grouping was made for another batch (tiles %d, expected %d)", who,
               c->tiles, bucket_tiles(B, c->K));
  *out = Buckets{c->K, c->bucket, c->rows, c->tile_bucket, c->seg, c->tiles};
  return NNUE_OK;
}

}  // namespace

// =============================================================================== C ABI
// Every plain entry point is its *_bucketed form without a grouping (buckets_from(NULL): one layer stack).
extern "C" int64_t nnue_classifier_scratch(int B, int L1, int L2, int L3) { return nnue_classifier_scratch_bucketed(B, L1, L2, L3, 1); }

extern "C" int64_t nnue_classifier_scratch_bucketed(int B, int L1, int L2, int L3, int K) {
  if (B <= 0 || L1 <= 0 || L2 <= 0 || L3 <= 0 || K <= 0) return 0;
  const int64_t a = backward_layout(make_plan(B, L1, L2, 0, K), B, L1, L2, L3, K).total;
  const int64_t b = backward_layout(make_plan(B, L1, L2, 1, K), B, L1, L2, L3, K).total;
  return (a > b ? a : b) * (int64_t)sizeof(float);
}

extern "C" int nnue_bucket_tile_count(int B, int K) { return (B > 0 && K > 0) ? bucket_tiles(B, K) : 0; }

extern "C" int nnue_bucket_group(const int32_t* n, int B, int P, int K, int32_t* bucket, int32_t* rows, int32_t* tile_bucket,
                                 int32_t* seg, nnue_stream_t stream) {
  NNUE_REQUIRE(n && bucket && rows && tile_bucket && seg, NNUE_E_ARG, "nnue_bucket_group: null pointer");
  NNUE_REQUIRE(B > 0 && P >= 0 && K >= 1, NNUE_E_ARG, "nnue_bucket_group: B=%d P=%d K=%d out of range", B, P, K);
  NNUE_REQUIRE(K <= kMaxBuckets, NNUE_E_SHAPE, "nnue_bucket_group: %d layer stacks (at most %d)", K, kMaxBuckets);
  hipLaunchKernelGGL(bucket_group_kernel, dim3(1), dim3(kGroupThreads), 0, static_cast<hipStream_t>(stream),
                     GroupArgs{n, B, P, K, bucket, rows, tile_bucket, seg, bucket_tiles(B, K)});
  return nnue_launch_status("nnue_bucket_group");
}

extern "C" int nnue_classifier_forward(const float* x, int pairwise, const float* w1, const float* b1, const float* w2, const float* b2,
                                       const float* w3, const float* b3, float clip, int B, int L1, int L2, int L3, int C, float* h1,
                                       float* h2, float* logits, void* scratch, int64_t scratch_bytes, nnue_stream_t stream) {
  return nnue_classifier_forward_bucketed(x, pairwise, w1, b1, w2, b2, w3, b3, clip, B, L1, L2, L3, C, h1, h2, logits, scratch,
                                          scratch_bytes, nullptr, stream);
}

extern "C" int nnue_classifier_forward_bucketed(const float* x, int pairwise, const float* w1, const float* b1, const float* w2,
                                                const float* b2, const float* w3, const float* b3, float clip, int B, int L1, int L2,
                                                int L3, int C, float* h1, float* h2, float* logits, void* scratch,
                                                int64_t scratch_bytes, const nnue_buckets* buckets, nnue_stream_t stream) {
  Buckets bk;
  const int rc = buckets_from(buckets, B, &bk, "nnue_classifier_forward_bucketed");
  if (rc != NNUE_OK) return rc;
  NNUE_REQUIRE(x && w1 && b1 && w2 && b2 && w3 && b3 && h1 && h2 && logits && scratch, NNUE_E_ARG,
               "nnue_classifier_forward: null pointer");
  NNUE_REQUIRE(B > 0 && L1 > 0 && L2 > 0 && L3 > 0 && C > 0, NNUE_E_ARG,
               "nnue_classifier_forward: B=%d L1=%d L2=%d L3=%d C=%d must be positive", B, L1, L2, L3, C);
  NNUE_REQUIRE(!pairwise || L1 % 2 == 0, NNUE_E_SHAPE, "nnue_classifier_forward: pairwise needs an even L1 (got %d)", L1);
  NNUE_REQUIRE((int64_t)(L2 + L3) * 4 <= 64 * 1024, NNUE_E_SHAPE, "nnue_classifier_forward: L2+L3 too large for the LDS tail");
  const ClsPlan p = make_plan(B, L1, L2, pairwise, bk.K);
  const BackwardLayout t = backward_layout(p, B, L1, L2, L3, bk.K);
  NNUE_REQUIRE(scratch_bytes >= t.total * (int64_t)sizeof(float), NNUE_E_SCRATCH,
               "nnue_classifier_forward: scratch %lld bytes too small", (long long)scratch_bytes);
  NNUE_REQUIRE(nnue_aligned16(x) && nnue_aligned16(w1) && nnue_aligned16(scratch), NNUE_E_ARG,
               "nnue_classifier_forward: pointers must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* part = static_cast<float*>(scratch) + t.part;
  launch_l1_forward(p, L1Call{x, pairwise, B, L1, L2, bk, s}, w1, part);
  hipLaunchKernelGGL(tail_forward_kernel, dim3(B), dim3(128), (size_t)(L2 + L3) * sizeof(float), s, part, p.fwd_ksplit, b1,
                     w2, b2, w3, b3, clip, B, L2, L3, C, h1, h2, logits, bk);
  return nnue_launch_status("nnue_classifier_forward");
}

extern "C" int nnue_classifier_backward(const float* x, int pairwise, const float* w1, const float* w2, const float* w3, float clip,
                                        const float* h1, const float* h2, const float* d_logits, int B, int L1, int L2, int L3, int C,
                                        float* d_x, float* d_w1, float* d_b1, float* d_w2, float* d_b2, float* d_w3, float* d_b3,
                                        void* scratch, int64_t scratch_bytes, nnue_stream_t stream) {
  return nnue_classifier_backward_bucketed(x, pairwise, w1, w2, w3, clip, h1, h2, d_logits, B, L1, L2, L3, C, d_x, d_w1, d_b1, d_w2, d_b2,
                                           d_w3, d_b3, scratch, scratch_bytes, nullptr, stream);
}

extern "C" int nnue_classifier_backward_bucketed(const float* x, int pairwise, const float* w1, const float* w2, const float* w3,
                                                 float clip, const float* h1, const float* h2, const float* d_logits, int B, int L1,
                                                 int L2, int L3, int C, float* d_x, float* d_w1, float* d_b1, float* d_w2, float* d_b2,
                                                 float* d_w3, float* d_b3, void* scratch, int64_t scratch_bytes,
                                                 const nnue_buckets* buckets, nnue_stream_t stream) {
  Buckets bk;
  const int rc = buckets_from(buckets, B, &bk, "nnue_classifier_backward_bucketed");
  if (rc != NNUE_OK) return rc;
  NNUE_REQUIRE(x && w1 && w2 && w3 && h1 && h2 && d_logits && scratch, NNUE_E_ARG, "nnue_classifier_backward: null input pointer");
  NNUE_REQUIRE(d_w1 && d_b1 && d_w2 && d_b2 && d_w3 && d_b3, NNUE_E_ARG, "nnue_classifier_backward: null gradient pointer");
  NNUE_REQUIRE(B > 0 && L1 > 0 && L2 > 0 && L3 > 0 && C > 0, NNUE_E_ARG,
               "nnue_classifier_backward: B=%d L1=%d L2=%d L3=%d C=%d must be positive", B, L1, L2, L3, C);
  NNUE_REQUIRE(!pairwise || L1 % 2 == 0, NNUE_E_SHAPE, "nnue_classifier_backward: pairwise needs an even L1 (got %d)", L1);
  NNUE_REQUIRE((int64_t)(C + L3) * 4 <= 64 * 1024, NNUE_E_SHAPE, "nnue_classifier_backward: C+L3 too large for the LDS tail");
  const ClsPlan p = make_plan(B, L1, L2, pairwise, bk.K);
  const BackwardLayout t = backward_layout(p, B, L1, L2, L3, bk.K);
  NNUE_REQUIRE(scratch_bytes >= t.total * (int64_t)sizeof(float), NNUE_E_SCRATCH,
               "nnue_classifier_backward: scratch %lld bytes too small", (long long)scratch_bytes);
  NNUE_REQUIRE(nnue_aligned16(x) && nnue_aligned16(w1) && nnue_aligned16(scratch) && nnue_aligned16(d_w1), NNUE_E_ARG,
               "nnue_classifier_backward: pointers must be 16-byte aligned");
  const L1Call l1{x, pairwise, B, L1, L2, bk, static_cast<hipStream_t>(stream)};
  float* base = static_cast<float*>(scratch);
  float *d_z1 = base + t.d_z1, *d_z2 = base + t.d_z2, *slabs = base + t.slabs;
  hipLaunchKernelGGL(tail_backward_kernel, dim3(B), dim3(128), (size_t)(C + L3) * sizeof(float), l1.s, d_logits, h1, h2, w2, w3,
                     clip, L2, L3, C, d_z1, d_z2, bk);
  const SmallWgrad sw = small_wgrad_args(p, B, L2, L3, C, bk, d_logits, d_z2, d_z1, h1, h2, d_b1, d_w2, d_b2, d_w3, d_b3, nullptr, nullptr,
                                         SlabSum{});  // no mean loss here, and the slab sum is a launch of its own
  hipLaunchKernelGGL(small_wgrad_kernel, dim3((unsigned)sw.wgrad_blocks), dim3(256), 0, l1.s, sw);
  launch_l1_backward_w(p, l1, d_z1, slabs, d_w1);
  const long long count = dw1_floats(bk.K, L1, L2);
  if (slab_pass(p))
    hipLaunchKernelGGL(slab_sum_kernel, dim3(slab_sum_blocks(count)), dim3(256), 0, l1.s, slabs, p.bww_ksplit, count, d_w1, bk, p.bww_klen);
  if (d_x) launch_l1_backward_x(p, l1, w1, d_z1, d_x);
  return nnue_launch_status("nnue_classifier_backward");
}

// ---------------------------------------------------------------- fused training step of the classifier block
extern "C" int64_t nnue_classifier_train_scratch(int B, int L1, int L2, int L3, int C) {
  return nnue_classifier_train_scratch_bucketed(B, L1, L2, L3, C, 1);
}

extern "C" int64_t nnue_classifier_train_scratch_bucketed(int B, int L1, int L2, int L3, int C, int K) {
  if (B <= 0 || L1 <= 0 || L2 <= 0 || L3 <= 0 || C <= 0 || K <= 0) return 0;
  const int64_t a = train_layout(make_plan(B, L1, L2, 0, K), B, L1, L2, L3, C, K).total;
  const int64_t b = train_layout(make_plan(B, L1, L2, 1, K), B, L1, L2, L3, C, K).total;
  return (a > b ? a : b) * (int64_t)sizeof(float);
}

extern "C" int nnue_classifier_train_fused_tail_supported(int B, int L1, int L2, int L3, int C, int K, int pairwise) {
  return tail_dx_supported(B, L1, L2, L3, C, K, pairwise) ? 1 : 0;
}

extern "C" int64_t nnue_classifier_train_dz1_offset(int B, int L1, int L2, int L3, int C, int pairwise) {
  if (B <= 0 || L1 <= 0 || L2 <= 0 || L3 <= 0 || C <= 0) return -1;
  return train_layout(make_plan(B, L1, L2, pairwise), B, L1, L2, L3, C).d_z1 * (int64_t)sizeof(float);
}

extern "C" int64_t nnue_classifier_train_dz1_grouped_offset(int B, int L1, int L2, int L3, int C, int K) {
  if (B <= 0 || L1 <= 0 || L2 <= 0 || L3 <= 0 || C <= 0 || K <= 1 || K > kMaxBuckets) return -1;
  return train_layout(make_plan(B, L1, L2, 1, K), B, L1, L2, L3, C, K).d_z1_g * (int64_t)sizeof(float);
}

extern "C" int64_t nnue_classifier_train_x_grouped_offset(int B, int L1, int L2, int L3, int C, int K) {
  if (B <= 0 || L1 <= 0 || L2 <= 0 || L3 <= 0 || C <= 0 || K <= 1 || K > kMaxBuckets) return -1;
  return train_layout(make_plan(B, L1, L2, 1, K), B, L1, L2, L3, C, K).x_g * (int64_t)sizeof(float);
}

// The arguments of the small-gradient tile family for a step run with NNUE_CLS_SMALL_RIDE (host side only): those of the
// step's own launch (small_wgrad_args) with no slab sum -- d_w1 belongs to nnue_ftm_backward's rider in this mode
extern "C" int nnue_classifier_train_rider(int pairwise, int B, int L1, int L2, int L3, int C, const float* h1, const float* h2,
                                           const float* sample_loss, float* loss, float* d_b1, float* d_w2, float* d_b2, float* d_w3,
                                           float* d_b3, void* scratch, int64_t scratch_bytes, const nnue_buckets* buckets,
                                           nnue_cls_rider* out) {
  NNUE_REQUIRE(h1 && h2 && sample_loss && loss && d_b1 && d_w2 && d_b2 && d_w3 && d_b3 && scratch && out, NNUE_E_ARG,
               "nnue_classifier_train_rider: null pointer");
  NNUE_REQUIRE(B > 0 && L1 > 0 && L2 > 0 && L3 > 0 && C > 0, NNUE_E_ARG, "nnue_classifier_train_rider: sizes must be positive");
  Buckets bk;
  const int rc = buckets_from(buckets, B, &bk, "nnue_classifier_train_rider");
  if (rc != NNUE_OK) return rc;
  const ClsPlan p = make_plan(B, L1, L2, pairwise, bk.K);
  const TrainLayout t = train_layout(p, B, L1, L2, L3, C, bk.K);
  NNUE_REQUIRE(scratch_bytes >= t.total * (int64_t)sizeof(float), NNUE_E_SCRATCH, "nnue_classifier_train_rider: scratch %lld < %lld bytes",
               (long long)scratch_bytes, (long long)(t.total * 4));
  float* base = static_cast<float*>(scratch);
  const SmallWgrad sw = small_wgrad_args(p, B, L2, L3, C, bk, base + t.d_logits, base + t.d_z2, base + t.d_z1, h1, h2, d_b1, d_w2, d_b2, d_w3,
                                         d_b3, sample_loss, loss, SlabSum{nullptr, 0, dw1_floats(bk.K, L1, L2), nullptr});
  static_assert(sizeof(SmallWgrad) <= sizeof(nnue_cls_rider), "nnue_cls_rider is too small");
  memset(out, 0, sizeof(*out));
  memcpy(out, &sw, sizeof(sw));
  return NNUE_OK;
}

namespace {
// The one launcher behind the six entry points.  soft NULL: the plain step; distill (with soft = its SoftTargets half): the
// teacher arm.  Checks in the order they have always had, then one arm per field of the plan (train_step_plan)
int train_step(const float* x, int pairwise, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
               const float* b3, float clip, const int64_t* labels, float grad_scale, int B, int L1, int L2, int L3, int C, float* h1,
               float* h2, float* logits, float* sample_loss, float* loss, float* d_x, float* d_w1, float* d_b1, float* d_w2, float* d_b2,
               float* d_w3, float* d_b3, void* scratch, int64_t scratch_bytes, int phases, const nnue_buckets* buckets, nnue_stream_t stream,
               const SoftTargets* soft, const DistillTargets* distill = nullptr) {
  Buckets bk;
  const int rc = buckets_from(buckets, B, &bk, "nnue_classifier_train_step_bucketed");
  if (rc != NNUE_OK) return rc;
  NNUE_REQUIRE(x && w1 && b1 && w2 && b2 && w3 && b3 && labels && h1 && h2 && logits && sample_loss && loss && scratch,
               NNUE_E_ARG, "nnue_classifier_train_step: null pointer");
  const int K = bk.K;
  const TrainStepPlan sp = train_step_plan(pairwise, B, L1, L2, L3, C, K, phases, d_x != nullptr, nnue_aligned16(w2) && nnue_aligned16(w3));
  const ClsPlan& p = sp.p;
  const TrainLayout& t = sp.t;
  NNUE_REQUIRE(sp.refusal != Refusal::bad_phases, NNUE_E_ARG,
               "nnue_classifier_train_step: phases = 1 (activations + d_x) | 2 (weight gradients + loss) [| 4: first-layer weight product beside "
               "d_x] [| 8: layer-1 slabs already at the start of scratch] [| 16 (not with 4): d_w1 comes from nnue_ftm_backward] [| 32 (with 1, 2 "
               "and 16): the small gradients and the mean loss ride in nnue_ftm_backward's launch as well] [| 64 (only as 123 = 59 + 64): the "
               "per-sample tail runs in the d_x launch]");
  NNUE_REQUIRE(sp.refusal != Refusal::slabs_many_stacks, NNUE_E_ARG,
               "nnue_classifier_train_step: phases bit 8 (layer-1 slabs formed in the FeatureTransformer forward's epilogue) exists for one layer stack only");
  NNUE_REQUIRE(sp.refusal != Refusal::dw1_rides_stack_shape, NNUE_E_SHAPE,
               "nnue_classifier_train_step: phases bit 16 with K > 1 needs the pairwise block and L1 %% 4 == 0");
  NNUE_REQUIRE(sp.refusal != Refusal::slabs_shape, NNUE_E_SHAPE,
               "nnue_classifier_train_step: phases bit 8 needs the pairwise block and L1 %% 64 == 0 (got L1=%d)", L1);
  NNUE_REQUIRE(d_w1 && d_b1 && d_w2 && d_b2 && d_w3 && d_b3, NNUE_E_ARG, "nnue_classifier_train_step: null gradient pointer");
  NNUE_REQUIRE(sp.refusal != Refusal::sizes, NNUE_E_ARG, "nnue_classifier_train_step: B=%d L1=%d L2=%d L3=%d C=%d must be positive", B, L1, L2,
               L3, C);
  NNUE_REQUIRE(sp.refusal != Refusal::odd_l1, NNUE_E_SHAPE, "nnue_classifier_train_step: pairwise needs an even L1 (got %d)", L1);
  NNUE_REQUIRE(sp.refusal != Refusal::tail_lds, NNUE_E_SHAPE, "nnue_classifier_train_step: L2+2*L3+C too large for the LDS tail");
  // the DISTILL arm of tail_train_kernel keeps the teacher row in LDS beside the logits
  const int64_t tail_lds = sp.tail_lds + (distill ? (int64_t)C * 4 : 0);
  NNUE_REQUIRE(tail_lds <= 64 * 1024, NNUE_E_SHAPE, "nnue_classifier_train_step_distill: L2+2*L3+2*C too large for the LDS tail");
  NNUE_REQUIRE(scratch_bytes >= t.total * (int64_t)sizeof(float), NNUE_E_SCRATCH,
               "nnue_classifier_train_step: scratch %lld < %lld bytes", (long long)scratch_bytes, (long long)(t.total * 4));
  NNUE_REQUIRE(nnue_aligned16(x) && nnue_aligned16(w1) && nnue_aligned16(scratch) && nnue_aligned16(d_w1) && nnue_aligned16(h1) &&
                   nnue_aligned16(h2),
               NNUE_E_ARG, "nnue_classifier_train_step: pointers must be 16-byte aligned");
  NNUE_REQUIRE(sp.refusal != Refusal::small_ride_no_dx, NNUE_E_SHAPE,
               "nnue_classifier_train_step: phases bit 32 needs the d_x launch the small gradients otherwise ride in (MFMA shapes, d_x requested)");
  NNUE_REQUIRE(sp.refusal != Refusal::fused_tail_shape, NNUE_E_SHAPE,
               "nnue_classifier_train_step: phases 123 (tail inside the d_x launch) needs nnue_classifier_train_fused_tail_supported "
               "(B=%d L1=%d L2=%d L3=%d C=%d K=%d pairwise=%d)", B, L1, L2, L3, C, K, pairwise);
  NNUE_REQUIRE(sp.dx != DxLaunch::with_tail || (nnue_aligned16(w2) && nnue_aligned16(w3)), NNUE_E_ARG,
               "nnue_classifier_train_step: phases 123 needs 16-byte aligned w2 and w3");

  const L1Call l1{x, pairwise, B, L1, L2, bk, static_cast<hipStream_t>(stream)};
  hipStream_t s = l1.s;
  float* base = static_cast<float*>(scratch);
  float *part = base + t.part, *d_z1 = base + t.d_z1, *d_z2 = base + t.d_z2, *d_logits = base + t.d_logits, *slabs = base + t.slabs;
  float *d_z1_g = sp.grouped ? base + t.d_z1_g : nullptr, *x_g = sp.grouped ? base + t.x_g : nullptr;
  // one launch: the small weight/bias gradients (per layer stack), the mean loss and (piggy-backed) the d_w1 slab sum
  const SmallWgrad sw = small_wgrad_args(p, B, L2, L3, C, bk, d_logits, d_z2, d_z1, h1, h2, d_b1, d_w2, d_b2, d_w3, d_b3, sample_loss, loss,
                                         SlabSum{slabs, sp.sum_slabs, dw1_floats(K, L1, L2), d_w1});
  // st: nothing (the plain kernels) or one SoftTargets (their SOFT arm)
  auto tile_tail = [&](auto with_dx, auto... st) {
    launch_tail_dx_kernel<decltype(with_dx)::value>(sp.tdx_grid, s, std::make_tuple(st...), part, sp.tail_slabs, b1, w2, b2, w3, b3, clip, labels,
                                                    grad_scale / (float)B, B, C, h1, h2, logits, sample_loss, d_logits, d_z1, d_z2, x, w1, L1, d_x,
                                                    row_tiles(B, K), sp.tdx_cg);
  };
#define NNUE_TAIL(NT, V, ...)                                                                                                             \
  hipLaunchKernelGGL((tail_train_kernel<NT, V>), dim3(sp.tail_grid), dim3(NT), (size_t)tail_lds, s, part, sp.tail_slabs, b1, w2, b2, w3, b3, \
                     clip, labels, grad_scale / (float)B, B, L2, L3, C, h1, h2, logits, sample_loss, d_logits, d_z1, d_z2, bk, x, L1, x_g,     \
                     d_z1_g, ##__VA_ARGS__)

  // A kernel template's instantiations stand in the code object in the order of their first use here: tail_dx_train_kernel
  // with, then without d_x tiles, tail_train_kernel<512, .>, <128, .>.  A new arm goes behind them, so that no kernel moves:
  // the SOFT arms follow in the same order, then the DISTILL arms.
  const bool plain = soft == nullptr;
  if (plain && sp.dx == DxLaunch::with_tail) tile_tail(std::true_type{});  // the whole call: nothing below is planned with it
  if (sp.l1_forward) launch_l1_forward(p, l1, w1, part);
  if (plain) {
    if (sp.tail == TailLaunch::tile) tile_tail(std::false_type{});
    else if (sp.tail == TailLaunch::sample512) { if (sp.tail_vec) NNUE_TAIL(512, true); else NNUE_TAIL(512, false); }
    else if (sp.tail == TailLaunch::sample128) { if (sp.tail_vec) NNUE_TAIL(128, true); else NNUE_TAIL(128, false); }
  } else if (!distill) {  // the same launches with the kernels' SOFT arm
    if (sp.dx == DxLaunch::with_tail) tile_tail(std::true_type{}, *soft);
    else if (sp.tail == TailLaunch::tile) tile_tail(std::false_type{}, *soft);
    else if (sp.tail == TailLaunch::sample512) { if (sp.tail_vec) NNUE_TAIL(512, true, *soft); else NNUE_TAIL(512, false, *soft); }
    else if (sp.tail == TailLaunch::sample128) { if (sp.tail_vec) NNUE_TAIL(128, true, *soft); else NNUE_TAIL(128, false, *soft); }
  } else {  // and with their DISTILL arm
    if (sp.dx == DxLaunch::with_tail) tile_tail(std::true_type{}, *distill);
    else if (sp.tail == TailLaunch::tile) tile_tail(std::false_type{}, *distill);
    else if (sp.tail == TailLaunch::sample512) { if (sp.tail_vec) NNUE_TAIL(512, true, *distill); else NNUE_TAIL(512, false, *distill); }
    else if (sp.tail == TailLaunch::sample128) { if (sp.tail_vec) NNUE_TAIL(128, true, *distill); else NNUE_TAIL(128, false, *distill); }
  }
#undef NNUE_TAIL
  if (sp.dx == DxLaunch::with_dw1) {
    const int w_blocks = bww_blocks(p, l1);
    hipLaunchKernelGGL(l1_backward_xw_mfma, dim3((unsigned)(w_blocks + bwx_blocks(l1))), dim3(256), 0, s, x, pairwise, w1, d_z1, B, L1, L2, d_x,
                       w_blocks, p.bww_ksplit, p.bww_klen, slab_pass(p) ? slabs : d_w1, bk);
  } else if (sp.dx == DxLaunch::with_small) {
    const int x_blocks = bwx_blocks(l1), small_blocks = sp.dx_hosts_small && !abl_skip_small() ? sw.wgrad_blocks : 0;
    hipLaunchKernelGGL(l1_backward_x_small_wgrad, dim3((unsigned)(x_blocks + small_blocks)), dim3(256), 0, s, x, pairwise, w1,
                       (const float*)d_z1, B, L1, L2, d_x, x_blocks, sw);
  } else if (sp.dx == DxLaunch::alone) launch_l1_backward_x(p, l1, w1, d_z1, d_x);
  if (sp.dw1_product) launch_l1_backward_w(p, l1, d_z1, slabs, d_w1);
  if (sp.small_wgrad) hipLaunchKernelGGL(small_wgrad_kernel, dim3(sw.wgrad_blocks + sp.slab_blocks), dim3(256), 0, s, sw);
  return nnue_launch_status("nnue_classifier_train_step");
}
}  // namespace

extern "C" int nnue_classifier_train_step(const float* x, int pairwise, const float* w1, const float* b1, const float* w2, const float* b2,
                                          const float* w3, const float* b3, float clip, const int64_t* labels, float grad_scale, int B,
                                          int L1, int L2, int L3, int C, float* h1, float* h2, float* logits, float* sample_loss,
                                          float* loss, float* d_x, float* d_w1, float* d_b1, float* d_w2, float* d_b2, float* d_w3,
                                          float* d_b3, void* scratch, int64_t scratch_bytes, int phases, nnue_stream_t stream) {
  return train_step(x, pairwise, w1, b1, w2, b2, w3, b3, clip, labels, grad_scale, B, L1, L2, L3, C, h1, h2, logits, sample_loss, loss, d_x,
                    d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, scratch, scratch_bytes, phases, nullptr, stream, nullptr);
}

extern "C" int nnue_classifier_train_step_bucketed(const float* x, int pairwise, const float* w1, const float* b1, const float* w2,
                                                   const float* b2, const float* w3, const float* b3, float clip, const int64_t* labels,
                                                   float grad_scale, int B, int L1, int L2, int L3, int C, float* h1, float* h2,
                                                   float* logits, float* sample_loss, float* loss, float* d_x, float* d_w1, float* d_b1,
                                                   float* d_w2, float* d_b2, float* d_w3, float* d_b3, void* scratch,
                                                   int64_t scratch_bytes, int phases, const nnue_buckets* buckets, nnue_stream_t stream) {
  return train_step(x, pairwise, w1, b1, w2, b2, w3, b3, clip, labels, grad_scale, B, L1, L2, L3, C, h1, h2, logits, sample_loss, loss, d_x,
                    d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, scratch, scratch_bytes, phases, buckets, stream, nullptr);
}

extern "C" int nnue_classifier_train_step_soft(const float* x, int pairwise, const float* w1, const float* b1, const float* w2,
                                               const float* b2, const float* w3, const float* b3, float clip, const int64_t* labels,
                                               float grad_scale, int B, int L1, int L2, int L3, int C, float* h1, float* h2, float* logits,
                                               float* sample_loss, float* loss, float* d_x, float* d_w1, float* d_b1, float* d_w2,
                                               float* d_b2, float* d_w3, float* d_b3, void* scratch, int64_t scratch_bytes, int phases,
                                               const int64_t* labels_b, const float* lam, float eps, nnue_stream_t stream) {
  return nnue_classifier_train_step_soft_bucketed(x, pairwise, w1, b1, w2, b2, w3, b3, clip, labels, grad_scale, B, L1, L2, L3, C, h1, h2,
                                                  logits, sample_loss, loss, d_x, d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, scratch, scratch_bytes,
                                                  phases, labels_b, lam, eps, nullptr, stream);
}

extern "C" int nnue_classifier_train_step_soft_bucketed(const float* x, int pairwise, const float* w1, const float* b1, const float* w2,
                                                        const float* b2, const float* w3, const float* b3, float clip,
                                                        const int64_t* labels, float grad_scale, int B, int L1, int L2, int L3, int C,
                                                        float* h1, float* h2, float* logits, float* sample_loss, float* loss, float* d_x,
                                                        float* d_w1, float* d_b1, float* d_w2, float* d_b2, float* d_w3, float* d_b3,
                                                        void* scratch, int64_t scratch_bytes, int phases, const int64_t* labels_b,
                                                        const float* lam, float eps, const nnue_buckets* buckets, nnue_stream_t stream) {
  NNUE_REQUIRE(eps >= 0.0f && eps < 1.0f, NNUE_E_ARG, "nnue_classifier_train_step_soft: eps = %g is outside [0, 1)", (double)eps);
  NNUE_REQUIRE(lam || !labels_b, NNUE_E_ARG, "nnue_classifier_train_step_soft: labels_b without lam");
  const SoftTargets soft{labels_b, labels_b ? lam : nullptr, eps};  // lam without labels_b mixes a label with itself: not read
  return train_step(x, pairwise, w1, b1, w2, b2, w3, b3, clip, labels, grad_scale, B, L1, L2, L3, C, h1, h2, logits, sample_loss, loss, d_x,
                    d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, scratch, scratch_bytes, phases, buckets, stream, &soft);
}

extern "C" int nnue_classifier_train_step_distill(const float* x, int pairwise, const float* w1, const float* b1, const float* w2,
                                                  const float* b2, const float* w3, const float* b3, float clip, const int64_t* labels,
                                                  float grad_scale, int B, int L1, int L2, int L3, int C, float* h1, float* h2,
                                                  float* logits, float* sample_loss, float* loss, float* d_x, float* d_w1, float* d_b1,
                                                  float* d_w2, float* d_b2, float* d_w3, float* d_b3, void* scratch, int64_t scratch_bytes,
                                                  int phases, const int64_t* labels_b, const float* lam, float eps, const float* teacher,
                                                  float alpha, float temperature, nnue_stream_t stream) {
  return nnue_classifier_train_step_distill_bucketed(x, pairwise, w1, b1, w2, b2, w3, b3, clip, labels, grad_scale, B, L1, L2, L3, C, h1, h2,
                                                     logits, sample_loss, loss, d_x, d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, scratch,
                                                     scratch_bytes, phases, labels_b, lam, eps, teacher, alpha, temperature, nullptr, stream);
}

extern "C" int nnue_classifier_train_step_distill_bucketed(const float* x, int pairwise, const float* w1, const float* b1, const float* w2,
                                                           const float* b2, const float* w3, const float* b3, float clip,
                                                           const int64_t* labels, float grad_scale, int B, int L1, int L2, int L3, int C,
                                                           float* h1, float* h2, float* logits, float* sample_loss, float* loss,
                                                           float* d_x, float* d_w1, float* d_b1, float* d_w2, float* d_b2, float* d_w3,
                                                           float* d_b3, void* scratch, int64_t scratch_bytes, int phases,
                                                           const int64_t* labels_b, const float* lam, float eps, const float* teacher,
                                                           float alpha, float temperature, const nnue_buckets* buckets,
                                                           nnue_stream_t stream) {
  NNUE_REQUIRE(alpha >= 0.0f && alpha <= 1.0f, NNUE_E_ARG, "nnue_classifier_train_step_distill: alpha = %g is outside [0, 1]", (double)alpha);
  NNUE_REQUIRE(temperature > 0.0f && temperature < INFINITY, NNUE_E_ARG,
               "nnue_classifier_train_step_distill: temperature = %g must be finite and positive", (double)temperature);
  NNUE_REQUIRE(teacher || alpha == 0.0f, NNUE_E_ARG, "nnue_classifier_train_step_distill: alpha > 0 without teacher logits");
  NNUE_REQUIRE(eps >= 0.0f && eps < 1.0f, NNUE_E_ARG, "nnue_classifier_train_step_distill: eps = %g is outside [0, 1)", (double)eps);
  NNUE_REQUIRE(lam || !labels_b, NNUE_E_ARG, "nnue_classifier_train_step_distill: labels_b without lam");
  DistillTargets dt;
  dt.labels_b = labels_b, dt.lam = labels_b ? lam : nullptr, dt.eps = eps;
  dt.teacher = teacher, dt.alpha = alpha, dt.temperature = temperature;
  // alpha == 0 is the soft call: the same launches, the teacher is not read
  return train_step(x, pairwise, w1, b1, w2, b2, w3, b3, clip, labels, grad_scale, B, L1, L2, L3, C, h1, h2, logits, sample_loss, loss, d_x,
                    d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, scratch, scratch_bytes, phases, buckets, stream, &dt, alpha > 0.0f ? &dt : nullptr);
}
