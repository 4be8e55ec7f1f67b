// The live float32 parameters of an NNUE quantised into the integer engine's tensors, in place, in one launch
// (nnue_engine_quantize_model): the arithmetic of the serialiser (serialize.py:218-222, :234-237 after the clamp of
// nnue.py:528-539), written in the layout EngineModel.load gives the bytes of the file.
//
// The FeatureTransformer table is the only large tensor: workgroups stream it in units of kQuantUnit elements, every lane
// turning two 16-byte loads into one 16-byte store of eight int16 (scalar loads for a source view that is not 16-byte aligned,
// scalar loads and stores for the ragged last group).  The small tensors follow in the same launch, one destination element
// per lane, the destination index mapped back to its source element or to a padding zero.  The segment table rides in the kernel
// arguments, so a call copies nothing to the device.
#include <limits.h>
#include "common.h"

namespace {

constexpr int kQuantUnit = 8192;         // table elements per work unit: 256 lanes x 4 groups of 8
constexpr int kQuantTableBlocks = 2048;  // table grid cap: a workgroup then streams units b, b + 2048, ...
constexpr int kQuantSegs = 8;
constexpr float kQuantScale = 64.0f;     // serialize.py:218 (every layer's scale)

enum { kClampedWeight = 0, kPlainWeight = 1, kBias = 2 };

// A small tensor: destination [stacks][drows][dcols] (int8 for the weight kinds, int32 for kBias) from the source
// [stacks][srows][scols]; destination rows and columns the source lacks are the engine's padding and written as zero.
struct QuantSeg {
  const float* src;
  void* dst;
  int32_t block0;  // the segment's first workgroup among the small-tensor workgroups
  int32_t count;   // destination elements
  int32_t srows, scols, drows, dcols;
  int32_t kind;
};

struct QuantArgs {
  const float* table;  // [table_count]
  int16_t* table_q;    // 16-byte aligned
  int64_t table_count, units;
  int32_t* bad;
  int32_t table_blocks, nseg;
  QuantSeg seg[kQuantSegs];
};
static_assert(sizeof(QuantArgs) <= 4096, "the segment table must fit the 4 KiB kernel-argument budget");

typedef short short8 __attribute__((ext_vector_type(8)));

// clamp(round_half_even(w * 64), -127, 127); clamp1: the weight is first clamped to [-1, 1] (in registers only).
__device__ __forceinline__ int quant_weight(float w, bool clamp1, int& bad) {
  if (!isfinite(w)) {
    ++bad;
    return 0;
  }
  if (clamp1) w = fminf(fmaxf(w, -1.0f), 1.0f);
  return (int)fminf(fmaxf(rintf(w * kQuantScale), -127.0f), 127.0f);
}

// round_half_even(b * 64) as int32, unclamped; a value int32 cannot hold is written as 0 and counted.
__device__ __forceinline__ int quant_bias(float b, int& bad) {
  const float r = rintf(b * kQuantScale);
  if (!isfinite(b) || !(r >= -2147483648.0f && r < 2147483648.0f)) {
    ++bad;
    return 0;
  }
  return (int)r;
}

__device__ __forceinline__ short8 quant_table8(const float4 a, const float4 b, int& bad) {
  short8 q;
  q[0] = (short)quant_weight(a.x, true, bad);
  q[1] = (short)quant_weight(a.y, true, bad);
  q[2] = (short)quant_weight(a.z, true, bad);
  q[3] = (short)quant_weight(a.w, true, bad);
  q[4] = (short)quant_weight(b.x, true, bad);
  q[5] = (short)quant_weight(b.y, true, bad);
  q[6] = (short)quant_weight(b.z, true, bad);
  q[7] = (short)quant_weight(b.w, true, bad);
  return q;
}

// eight consecutive source elements from element i: two 16-byte loads, or eight 4-byte loads for a view at another offset
__device__ __forceinline__ void load8(const float* __restrict__ src, int64_t i, bool vec, float4& a, float4& b) {
  if (vec) {
    a = *reinterpret_cast<const float4*>(src + i);
    b = *reinterpret_cast<const float4*>(src + i + 4);
  } else {
    a = make_float4(src[i], src[i + 1], src[i + 2], src[i + 3]);
    b = make_float4(src[i + 4], src[i + 5], src[i + 6], src[i + 7]);
  }
}

__global__ __launch_bounds__(256) void quantize_model_kernel(const QuantArgs A) {
  const int tid = threadIdx.x;
  int bad = 0;
  if ((int)blockIdx.x < A.table_blocks) {
    const float* __restrict__ src = A.table;
    int16_t* __restrict__ dst = A.table_q;
    const bool vec = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    for (int64_t u = blockIdx.x; u < A.units; u += A.table_blocks) {
      const int64_t base = u * kQuantUnit + 8 * tid;  // group j of the lane: elements base + j*2048 .. + 7
      if ((u + 1) * kQuantUnit <= A.table_count) {
        float4 a[4], b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) load8(src, base + j * 2048, vec, a[j], b[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<short8*>(dst + base + j * 2048) = quant_table8(a[j], b[j], bad);
      } else {  // the last unit: whole groups as above, then the ragged group element by element
        for (int j = 0; j < 4; ++j) {
          const int64_t i = base + j * 2048;
          if (i + 8 <= A.table_count) {
            float4 a, b;
            load8(src, i, vec, a, b);
            *reinterpret_cast<short8*>(dst + i) = quant_table8(a, b, bad);
          } else {
            for (int64_t e = i; e < A.table_count; ++e) dst[e] = (int16_t)quant_weight(src[e], true, bad);
          }
        }
      }
    }
  } else {
    const int sb = (int)blockIdx.x - A.table_blocks;  // wave-uniform: the table below is read with scalar loads
    int s = 0;
    while (s + 1 < A.nseg && A.seg[s + 1].block0 <= sb) ++s;
    const QuantSeg& S = A.seg[s];
    const int d = (sb - S.block0) * 256 + tid;
    if (d < S.count) {
      const int per = S.drows * S.dcols;
      const int k = d / per, in = d - k * per;
      const int r = in / S.dcols, c = in - r * S.dcols;
      int q = 0;
      if (r < S.srows && c < S.scols) {
        const float x = S.src[((int64_t)k * S.srows + r) * S.scols + c];
        q = S.kind == kBias ? quant_bias(x, bad) : quant_weight(x, S.kind == kClampedWeight, bad);
      }
      if (S.kind == kBias) static_cast<int32_t*>(S.dst)[d] = q;
      else static_cast<int8_t*>(S.dst)[d] = (int8_t)q;
    }
  }
  // one vector atomic per wave that saw an element it could not represent
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
  if ((tid & 63) == 0 && bad) atomicAdd(A.bad, bad);
}

bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" int nnue_engine_quantize_model(const float* conv_w, const float* ft_w, const float* ft_b, const float* w1,
                                          const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                                          int oc, int F, int L1, int L2, int L3, int C, int K, int stack,
                                          const nnue_engine_model* dst, const nnue_engine_stacks* dst_stacks,
                                          int32_t* bad_count, nnue_stream_t stream) {
  const char* fn = "nnue_engine_quantize_model";
  NNUE_REQUIRE(conv_w && ft_w && ft_b && w1 && b1 && w2 && b2 && w3 && b3 && dst && bad_count, NNUE_E_ARG, "%s: null pointer", fn);
  NNUE_REQUIRE(K >= 1 && K <= 64, NNUE_E_ARG, "%s: %d layer stacks (1..64)", fn, K);
  NNUE_REQUIRE(oc > 0 && F > 0 && L1 > 0 && L2 > 0 && L3 > 0 && C > 0, NNUE_E_ARG,
               "%s: oc=%d F=%d L1=%d L2=%d L3=%d C=%d must be positive", fn, oc, F, L1, L2, L3, C);
  NNUE_REQUIRE(L1 % 2 == 0, NNUE_E_SHAPE, "%s: L1=%d must be even (the pairwise block splits it in two)", fn, L1);
  NNUE_REQUIRE(dst->oc == oc && dst->num_features == F && dst->l1 == L1 && dst->l2 == L2 && dst->l3 == L3 && dst->classes == C,
               NNUE_E_SHAPE, "%s: destination is oc=%d F=%d L1=%d L2=%d L3=%d C=%d, the model oc=%d F=%d L1=%d L2=%d L3=%d C=%d", fn,
               dst->oc, dst->num_features, dst->l1, dst->l2, dst->l3, dst->classes, oc, F, L1, L2, L3, C);
  const bool all = dst_stacks != nullptr;
  if (all) {
    NNUE_REQUIRE(dst_stacks->count == K, NNUE_E_SHAPE, "%s: destination holds %d layer stacks, the model %d", fn,
                 dst_stacks->count, K);
  } else {
    NNUE_REQUIRE(stack >= 0 && stack < K, NNUE_E_ARG, "%s: stack %d outside [0, %d)", fn, stack, K);
  }
  const void* d_l1_w = all ? (const void*)dst_stacks->l1_w : dst->l1_w;
  const void* d_l1_b = all ? (const void*)dst_stacks->l1_b : dst->l1_b;
  const void* d_l2_w = all ? (const void*)dst_stacks->l2_w : dst->l2_w;
  const void* d_l2_b = all ? (const void*)dst_stacks->l2_b : dst->l2_b;
  const void* d_out_w = all ? (const void*)dst_stacks->out_w : dst->out_w;
  const void* d_out_b = all ? (const void*)dst_stacks->out_b : dst->out_b;
  NNUE_REQUIRE(dst->conv_w && dst->ft_w && dst->ft_b && d_l1_w && d_l1_b && d_l2_w && d_l2_b && d_out_w && d_out_b, NNUE_E_ARG,
               "%s: destination tensor missing", fn);
  NNUE_REQUIRE(aligned4(conv_w) && aligned4(ft_w) && aligned4(ft_b) && aligned4(w1) && aligned4(b1) && aligned4(w2) && aligned4(b2) &&
                   aligned4(w3) && aligned4(b3) && aligned4(bad_count),
               NNUE_E_ARG, "%s: source pointers must be 4-byte aligned", fn);
  NNUE_REQUIRE(nnue_aligned16(dst->ft_w) && aligned4(dst->ft_b) && aligned4(d_l1_b) && aligned4(d_l2_b) && aligned4(d_out_b),
               NNUE_E_ARG, "%s: destination table must be 16-byte aligned, int32 tensors 4-byte aligned", fn);
  const int stacks = all ? K : 1;
  const int64_t widest = (int64_t)stacks * (L2 + 1) * L1 + (int64_t)stacks * L3 * 2 * L2 + (int64_t)stacks * C * L3 + (int64_t)oc * 27;
  NNUE_REQUIRE(widest < (1ll << 30) && L1 < (1 << 24) && L2 < (1 << 24) && L3 < (1 << 24) && C < (1 << 24), NNUE_E_SHAPE,
               "%s: layer sizes too large", fn);

  QuantArgs A;
  A.table = ft_w;
  A.table_q = const_cast<int16_t*>(dst->ft_w);
  A.table_count = (int64_t)F * L1;
  A.units = (A.table_count + kQuantUnit - 1) / kQuantUnit;
  A.table_blocks = (int32_t)(A.units < kQuantTableBlocks ? A.units : kQuantTableBlocks);
  A.bad = bad_count;
  A.nseg = kQuantSegs;
  const int64_t s1 = all ? 0 : stack;  // a single-stack destination takes that stack of the source
  int32_t blocks = 0;
  int n = 0;
  auto add = [&](const float* src, const void* to, int kind, int st, int srows, int scols, int drows, int dcols) {
    QuantSeg& S = A.seg[n++];
    S.src = src;
    S.dst = const_cast<void*>(to);
    S.kind = kind;
    S.srows = srows;
    S.scols = scols;
    S.drows = drows;
    S.dcols = dcols;
    S.count = st * drows * dcols;
    S.block0 = blocks;
    blocks += (S.count + 255) / 256;
  };
  add(conv_w, dst->conv_w, kPlainWeight, 1, 1, oc * 27, 1, oc * 27);
  add(ft_b, dst->ft_b, kBias, 1, 1, L1, 1, L1);
  add(w1 + s1 * L2 * L1, d_l1_w, kClampedWeight, stacks, L2, L1, L2 + 1, L1);
  add(b1 + s1 * L2, d_l1_b, kBias, stacks, 1, L2, 1, L2 + 1);
  add(w2 + s1 * L3 * L2, d_l2_w, kClampedWeight, stacks, L3, L2, L3, 2 * L2);
  add(b2 + s1 * L3, d_l2_b, kBias, stacks, 1, L3, 1, L3);
  add(w3 + s1 * C * L3, d_out_w, kClampedWeight, stacks, C, L3, C, L3);
  add(b3 + s1 * C, d_out_b, kBias, stacks, 1, C, 1, C);

  hipLaunchKernelGGL(quantize_model_kernel, dim3((unsigned)(A.table_blocks + blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), A);
  return nnue_launch_status(fn);
}
