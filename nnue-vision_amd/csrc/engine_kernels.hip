// Batched GPU restatement of the reference C++ engine's integer inference,
// NNUEEvaluator::evaluate_logits (engine/src/nnue_engine.cpp:704-734), on the quantised tensors of a `.nnue` file:
// what evaluate_compiled_model (evaluate.py:88-385) obtains from one `nnue_inference` subprocess per image.
// All arithmetic is the engine's integer arithmetic, so results are bit-identical to it; three of its behaviours are
// reproduced on purpose (see oracle/nnue_engine_oracle.py): the image buffer is indexed HWC, the conv weight bytes
// are read as [oc][kh][kw][ic], and the conv's dense [out_h][out_w][oc] output is read back flat with row length g.
#include "common.h"

namespace {

constexpr int kMaxColsPerThread = 8;  // L1 <= 2048

// ConvLayer::forward (nnue_engine.cpp:48-158) into the zero-filled flat [g*g*oc] buffer of nnue_engine.cpp:679-681.
// grid (ceil(F / 256), B); thread = one byte of the flat buffer.
__global__ __launch_bounds__(256) void engine_conv_kernel(const float* __restrict__ images, const int8_t* __restrict__ w,
                                                          const int32_t* __restrict__ bias, float scale, int H, int W,
                                                          int stride, int OH, int OW, int oc, int F,
                                                          int8_t* __restrict__ conv) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= F) return;
  const int b = blockIdx.y;
  int8_t result = 0;
  if (o < OH * OW * oc) {
    const int c = o % oc, pos = o / oc;
    const int oh = pos / OW, ow = pos - oh * OW;
    const float* __restrict__ img = images + (size_t)b * H * W * 3;
    int32_t acc = bias[c];
    for (int kh = 0; kh < 3; ++kh)
      for (int kw = 0; kw < 3; ++kw) {
        const int ih = oh * stride + kh - 1, iw = ow * stride + kw - 1;
        if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
#pragma unroll
        for (int ic = 0; ic < 3; ++ic)
          acc += (int32_t)(img[(ih * W + iw) * 3 + ic] * scale) * (int32_t)w[((c * 3 + kh) * 3 + kw) * 3 + ic];
      }
    int32_t q = acc / (int32_t)scale;  // truncating division, as the engine
    q = q < -127 ? -127 : (q > 127 ? 127 : q);
    result = (int8_t)q;
  }
  conv[(size_t)b * F + o] = result;
}

__device__ __forceinline__ int32_t clamp_i(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// LayerStack::forward_multiclass (nnue_engine.cpp:480-539) of one image, from the clipped accumulator ft [L1] (LDS) to its
// logits row; shared by the batched and the per-stream kernels.  The caller synchronises after writing ft.
__device__ __forceinline__ void engine_tail(const int32_t* ft, int32_t* pair, int32_t* h1, int32_t* h2,
                                            const int8_t* __restrict__ l1_w, const int32_t* __restrict__ l1_b, float l1_scale,
                                            const int8_t* __restrict__ l2_w, const int32_t* __restrict__ l2_b, int l2_scale,
                                            const int8_t* __restrict__ out_w, const int32_t* __restrict__ out_b, float out_scale,
                                            int L1, int L2, int L3, int C, float* __restrict__ logits_row) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // pairwise: (a * b) / 128 clamped to [0, 127] | a clamped to [0, 127]
  const int half = L1 / 2;
  for (int i = tid; i < L1; i += 256) {
    int32_t v = 0;
    if (i < half) v = clamp_i((ft[i] * ft[i + half]) / 128, 0, 127);
    else if (i < 2 * half) v = clamp_i(ft[i - half], 0, 127);
    pair[i] = v;
  }
  __syncthreads();

  // layer 1 (dense_forward_scalar: float division, truncation, clamp to [0, 127]); one wave per output
  for (int o = wave; o < L2; o += 4) {
    const int8_t* __restrict__ wr = l1_w + (size_t)o * L1;
    int32_t s = 0;
    for (int k = lane; k < L1; k += 64) s += pair[k] * (int32_t)wr[k];
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) s += __shfl_xor(s, sh);
    if (lane == 0) {
      const float r = (float)(s + l1_b[o]) / l1_scale;
      h1[o] = clamp_i((int32_t)r, 0, 127);
    }
  }
  __syncthreads();

  // layer 2: integer division, clamp to [-127, 127], ReLU; weights are [L3][2 * L2], first L2 columns used
  for (int o = tid; o < L3; o += 256) {
    const int8_t* __restrict__ wr = l2_w + (size_t)o * 2 * L2;
    int32_t s = l2_b[o];
    for (int k = 0; k < L2; ++k) s += h1[k] * (int32_t)wr[k];
    int32_t r = clamp_i(s / l2_scale, -127, 127);
    h2[o] = r > 0 ? r : 0;
  }
  __syncthreads();

  for (int c = tid; c < C; c += 256) {
    const int8_t* __restrict__ wr = out_w + (size_t)c * L3;
    int32_t s = out_b[c];
    for (int j = 0; j < L3; ++j) s += h2[j] * (int32_t)wr[j];
    logits_row[c] = (float)s / out_scale;
  }
}

// Which layer stack a workgroup's image goes through.  NoStackSel: the one stack of the kernel's own arguments (the plain
// entry points; nothing is added to the kernel).  StackSel: K stacks packed stack-major behind those same pointers, chosen per
// image -- stack_in[b] when given (outside [0, K) = stack 0, nnue_engine.cpp:705-707), else the training rule on the engine's own
// count, min(K-1, n*K / (F+1)) (nnue.bucket_of).  The three scales of every stack travel by value in the kernel arguments.
constexpr int kMaxStacks = 64;

struct NoStackSel {
  static constexpr bool kSelect = false;
};

struct StackSel {
  static constexpr bool kSelect = true;
  int K;
  const int32_t* stack_in;
  int32_t* stack_out;
  float l1_scale[kMaxStacks];
  int l2_scale[kMaxStacks];
  float out_scale[kMaxStacks];
};

// Resolves the stack of image b from its active-feature count n (uniform over the workgroup), records it, and moves the tail's
// weights, biases and scales to that stack.
__device__ __forceinline__ void engine_select_stack(const StackSel& sel, int b, int n, int F, int L1, int L2, int L3, int C,
                                                    const int8_t* __restrict__& l1_w, const int32_t* __restrict__& l1_b,
                                                    float& l1_scale, const int8_t* __restrict__& l2_w,
                                                    const int32_t* __restrict__& l2_b, int& l2_scale,
                                                    const int8_t* __restrict__& out_w, const int32_t* __restrict__& out_b,
                                                    float& out_scale) {
  int k;
  if (sel.stack_in) {
    k = sel.stack_in[b];
    if (k < 0 || k >= sel.K) k = 0;
  } else {
    k = (int)((unsigned)(n * sel.K) / (unsigned)(F + 1));  // n <= F and F * K < 2^31 (checked on the host)
    if (k > sel.K - 1) k = sel.K - 1;
  }
  k = __builtin_amdgcn_readfirstlane(k);
  if (threadIdx.x == 0) sel.stack_out[b] = k;
  l1_w += (size_t)k * (L2 + 1) * L1;
  l1_b += (size_t)k * (L2 + 1);
  l2_w += (size_t)k * L3 * 2 * L2;
  l2_b += (size_t)k * L3;
  out_w += (size_t)k * C * L3;
  out_b += (size_t)k * C;
  l1_scale = sel.l1_scale[k];
  l2_scale = sel.l2_scale[k];
  out_scale = sel.out_scale[k];
}

// One workgroup per image: feature grid + FeatureTransformer (int16 wrap-around) + clipped ReLU + forward_multiclass
// (nnue_engine.h:236-283, simd_scalar.cpp:78-96, nnue_engine.cpp:726-729, :480-539).
// dynamic LDS: ft [L1] i32 | pair [L1] i32 | h1 [L2] i32 | h2 [L3] i32 | counts [4] i32
// Sel = StackSel: the image's stack is resolved from `count` before the tail (see engine_select_stack).
template <class Sel>
__global__ __launch_bounds__(256) void engine_stack_kernel(const int8_t* __restrict__ conv, float threshold, int F, int oc,
                                                           const int16_t* __restrict__ ft_w, const int32_t* __restrict__ ft_b,
                                                           int quantized_one, const int8_t* __restrict__ l1_w,
                                                           const int32_t* __restrict__ l1_b, float l1_scale,
                                                           const int8_t* __restrict__ l2_w, const int32_t* __restrict__ l2_b,
                                                           int l2_scale, const int8_t* __restrict__ out_w,
                                                           const int32_t* __restrict__ out_b, float out_scale, int L1, int L2,
                                                           int L3, int C, float* __restrict__ logits, float* __restrict__ density, Sel sel) {
  extern __shared__ int32_t lds[];
  int32_t* ft = lds;
  int32_t* pair = ft + L1;
  int32_t* h1 = pair + L1;
  int32_t* h2 = h1 + L2;
  int32_t* counts = h2 + L3;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int8_t* __restrict__ cv = conv + (size_t)b * F;

  // active features, ascending: every wave forms the same ballots and adds the rows to its own columns
  int32_t acc[kMaxColsPerThread];
#pragma unroll
  for (int j = 0; j < kMaxColsPerThread; ++j) acc[j] = 0;
  int count = 0;
  for (int f0 = 0; f0 < F; f0 += 64) {
    const int f = f0 + lane;
    const bool on = f < F && (float)cv[f] > threshold && (f % oc) < 64;  // 64 channels per cell are bit-packed
    unsigned long long mask = __ballot(on);
    count += __popcll(mask);
    while (mask) {
      const int row = f0 + __builtin_ctzll(mask);
      mask &= mask - 1;
      const int16_t* __restrict__ wr = ft_w + (size_t)row * L1;
#pragma unroll
      for (int j = 0; j < kMaxColsPerThread; ++j) {
        const int col = tid + 256 * j;
        if (col < L1) acc[j] += (int32_t)wr[col];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kMaxColsPerThread; ++j) {
    const int col = tid + 256 * j;
    if (col < L1) {
      const int16_t v = (int16_t)((int32_t)(int16_t)ft_b[col] + acc[j]);  // int16 accumulator wraps
      ft[col] = clamp_i((int32_t)v, 0, quantized_one);
    }
  }
  if (tid == 0) density[b] = (float)count / (float)F;
  __syncthreads();

  if constexpr (Sel::kSelect)
    engine_select_stack(sel, b, count, F, L1, L2, L3, C, l1_w, l1_b, l1_scale, l2_w, l2_b, l2_scale, out_w, out_b, out_scale);
  engine_tail(ft, pair, h1, h2, l1_w, l1_b, l1_scale, l2_w, l2_b, l2_scale, out_w, out_b, out_scale, L1, L2, L3, C,
              logits + (size_t)b * C);
  (void)counts;
}


// Per-stream state of nnue_engine_stream_step, one device buffer (offsets in bytes; W64 = ceil(F / 64)):
//   valid  [S] i32  at 0              0 = refresh the stream from the bias on its next step (a zero-filled state is fresh)
//   parity [S] i32  at 4 S            which of the two bit-word slots holds the stream's current feature set
//   bits   [2][S][W64] u64            at align16(8 S): the active-feature sets, ping-pong
//   acc    [S][L1] i16                after bits: the wrapped accumulator, bias included, BEFORE the clipped ReLU
struct StreamLayout {
  int64_t parity, bits, acc, total;
};

__host__ __device__ inline StreamLayout stream_layout(int64_t S, int64_t F, int64_t L1) {
  StreamLayout l;
  const int64_t w64 = (F + 63) / 64;
  l.parity = 4 * S;
  l.bits = (8 * S + 15) / 16 * 16;
  l.acc = l.bits + 2 * S * w64 * 8;
  l.total = (l.acc + 2 * S * L1 + 15) / 16 * 16;
  return l;
}

// NNUEEvaluator::evaluate_incremental (nnue_engine.cpp:739-786) for S independent streams, one workgroup per stream: the new
// feature set, the difference to the stream's previous one, and FeatureTransformer::update_accumulator (:257-267) on the
// stored int16 accumulator -- or refresh_accumulator (:806-816) from the bias when the stream is not valid, or when the
// difference holds more features than the new set (then a refresh reads fewer table rows).  Both give the same bits: the
// accumulator is int16 and wraps, and addition mod 2^16 does not depend on the order or the history of the terms.
// Then the clipped ReLU and engine_tail, as engine_stack_kernel.
// kFeatures: the set is given as a uint8 map active [S][F] (non-zero = on, every id counts: the reference's entry that takes
// feature indices applies no per-cell channel mask); otherwise it is formed from the conv bytes with engine_stack_kernel's
// predicate.
// Read/write hazard on the bit words: they ping-pong between two slots ([2][S][W64] + a per-stream parity that flips at the
// end of the step).  Every wave may read the old words at any time during the step while the new ones are stored into the
// other slot, so no barrier has to order those reads before the stores, and a launch never reads a word it writes.
// dynamic LDS: ft [L1] i32 | pair [L1] i32 | h1 [L2] i32 | h2 [L3] i32 | counts [8] i32 | (8-byte aligned) new [W64] u64 |
// old [W64] u64
// Sel = StackSel: the stream's stack is resolved from `n_new` before the tail (see engine_select_stack); the state is the same.
template <bool kFeatures, class Sel>
__global__ __launch_bounds__(256) void engine_stream_kernel(const int8_t* __restrict__ conv, const uint8_t* __restrict__ active,
                                                            float threshold, int F, int oc, int S, const int16_t* __restrict__ ft_w,
                                                            const int32_t* __restrict__ ft_b, int quantized_one,
                                                            const int8_t* __restrict__ l1_w, const int32_t* __restrict__ l1_b,
                                                            float l1_scale, const int8_t* __restrict__ l2_w,
                                                            const int32_t* __restrict__ l2_b, int l2_scale,
                                                            const int8_t* __restrict__ out_w, const int32_t* __restrict__ out_b,
                                                            float out_scale, int L1, int L2, int L3, int C, uint8_t* __restrict__ state,
                                                            float* __restrict__ logits, float* __restrict__ density,
                                                            int32_t* __restrict__ changed, Sel sel) {
  extern __shared__ int32_t lds[];
  int32_t* ft = lds;
  int32_t* pair = ft + L1;
  int32_t* h1 = pair + L1;
  int32_t* h2 = h1 + L2;
  int32_t* counts = h2 + L3;  // [wave] new, [4 + wave] difference
  const int W64 = (F + 63) / 64;
  unsigned long long* new_s = reinterpret_cast<unsigned long long*>(lds + ((2 * L1 + L2 + L3 + 8 + 1) & ~1));
  unsigned long long* old_s = new_s + W64;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  const StreamLayout lay = stream_layout(S, F, L1);
  int32_t* __restrict__ valid = reinterpret_cast<int32_t*>(state);
  int32_t* __restrict__ parity = reinterpret_cast<int32_t*>(state + lay.parity);
  unsigned long long* __restrict__ bits = reinterpret_cast<unsigned long long*>(state + lay.bits);
  int16_t* __restrict__ accs = reinterpret_cast<int16_t*>(state + lay.acc) + (size_t)b * L1;
  const bool was_valid = valid[b] != 0;
  const int par = parity[b] & 1;
  const unsigned long long* __restrict__ old_w = bits + ((size_t)par * S + b) * W64;
  unsigned long long* __restrict__ new_w = bits + ((size_t)(par ^ 1) * S + b) * W64;

  // pass 1: wave w forms the ballots of chunks w, w + 4, ...: new set -> its slot and LDS, old set -> LDS, both popcounts
  int n_new = 0, n_diff = 0;
  for (int c = wave; c < W64; c += 4) {
    const int f = c * 64 + lane;
    bool on;
    if constexpr (kFeatures) on = f < F && active[(size_t)b * F + f] != 0;
    else on = f < F && (float)conv[(size_t)b * F + f] > threshold && (f % oc) < 64;  // 64 channels per cell are bit-packed
    const unsigned long long m = __ballot(on);
    const unsigned long long o = was_valid ? old_w[c] : 0ull;
    n_new += __popcll(m);
    n_diff += __popcll(m ^ o);
    if (lane == 0) {
      new_w[c] = m;
      new_s[c] = m;
      old_s[c] = o;
    }
  }
  if (lane == 0) {
    counts[wave] = n_new;
    counts[4 + wave] = n_diff;
  }
  __syncthreads();
  n_new = counts[0] + counts[1] + counts[2] + counts[3];
  n_diff = counts[4] + counts[5] + counts[6] + counts[7];
  const bool refresh = !was_valid || n_diff > n_new;

  // pass 2: every wave walks the same words and updates its own columns in int32 registers seeded from the state or the bias
  int32_t acc[kMaxColsPerThread];
#pragma unroll
  for (int j = 0; j < kMaxColsPerThread; ++j) {
    const int col = tid + 256 * j;
    acc[j] = col < L1 ? (refresh ? (int32_t)(int16_t)ft_b[col] : (int32_t)accs[col]) : 0;
  }
  for (int c = 0; c < W64; ++c) {
    const unsigned long long m = new_s[c], o = refresh ? 0ull : old_s[c];
    unsigned long long add = m & ~o, sub = o & ~m;
    while (add) {
      const int16_t* __restrict__ wr = ft_w + (size_t)(c * 64 + __builtin_ctzll(add)) * L1;
      add &= add - 1;
#pragma unroll
      for (int j = 0; j < kMaxColsPerThread; ++j) {
        const int col = tid + 256 * j;
        if (col < L1) acc[j] += (int32_t)wr[col];
      }
    }
    while (sub) {
      const int16_t* __restrict__ wr = ft_w + (size_t)(c * 64 + __builtin_ctzll(sub)) * L1;
      sub &= sub - 1;
#pragma unroll
      for (int j = 0; j < kMaxColsPerThread; ++j) {
        const int col = tid + 256 * j;
        if (col < L1) acc[j] -= (int32_t)wr[col];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kMaxColsPerThread; ++j) {
    const int col = tid + 256 * j;
    if (col < L1) {
      const int16_t v = (int16_t)acc[j];  // int16 accumulator wraps
      accs[col] = v;
      ft[col] = clamp_i((int32_t)v, 0, quantized_one);
    }
  }
  if (tid == 0) {
    density[b] = (float)n_new / (float)F;
    changed[b] = was_valid ? n_diff : n_new;
    valid[b] = 1;
    parity[b] = par ^ 1;
  }
  __syncthreads();

  if constexpr (Sel::kSelect)
    engine_select_stack(sel, b, n_new, F, L1, L2, L3, C, l1_w, l1_b, l1_scale, l2_w, l2_b, l2_scale, out_w, out_b, out_scale);
  engine_tail(ft, pair, h1, h2, l1_w, l1_b, l1_scale, l2_w, l2_b, l2_scale, out_w, out_b, out_scale, L1, L2, L3, C,
              logits + (size_t)b * C);
}

}  // namespace

extern "C" int64_t nnue_engine_scratch(const nnue_engine_model* m, int B) {
  if (!m || B <= 0 || m->num_features <= 0) return 0;
  return (int64_t)B * m->num_features;
}

// A call runs the model's own stack (st == nullptr: the plain entry points) or the K packed stacks of an nnue_engine_stacks,
// in which case the model's stack pointers and stack scales are not read.
static bool engine_has_tensors(const nnue_engine_model* m, const nnue_engine_stacks* st) {
  if (!(m->conv_w && m->conv_b && m->ft_w && m->ft_b)) return false;
  if (st) return st->l1_w && st->l1_b && st->l2_w && st->l2_b && st->out_w && st->out_b;
  return m->l1_w && m->l1_b && m->l2_w && m->l2_b && m->out_w && m->out_b;
}

// What the stack-selecting entry points check before they read anything behind st.
static int engine_check_stacks(const nnue_engine_stacks* st, const void* stack_out, const char* fn) {
  NNUE_REQUIRE(st && stack_out, NNUE_E_ARG, "%s: null pointer", fn);
  NNUE_REQUIRE(st->count >= 1 && st->count <= kMaxStacks, NNUE_E_ARG, "%s: %d layer stacks (1..%d)", fn, st->count, kMaxStacks);
  NNUE_REQUIRE(st->scales, NNUE_E_ARG, "%s: null pointer", fn);
  return NNUE_OK;
}

// Shape and scale checks shared by the engine's entry points (fn names the caller in the message).
static int engine_check_model(const nnue_engine_model* m, const nnue_engine_stacks* st, const char* fn) {
  const int g = m->grid, oc = m->oc, F = m->num_features;
  NNUE_REQUIRE(g > 0 && oc > 0 && F == g * g * oc, NNUE_E_SHAPE, "%s: num_features %d != %d*%d*%d", fn, F, g, g, oc);
  NNUE_REQUIRE(m->l1 >= 2 && m->l1 <= 256 * kMaxColsPerThread && m->l2 >= 1 && m->l3 >= 1 && m->classes >= 1, NNUE_E_SHAPE,
               "%s: L1=%d (2..%d) L2=%d L3=%d C=%d", fn, m->l1, 256 * kMaxColsPerThread, m->l2, m->l3, m->classes);
  bool scales_ok = m->conv_scale >= 1.0f;
  if (st) {
    for (int k = 0; k < st->count; ++k)
      scales_ok = scales_ok && st->scales[3 * k + 1] >= 1.0f && st->scales[3 * k] > 0.0f && st->scales[3 * k + 2] > 0.0f;
    // the selector's n * K (n <= F) stays inside 32 bits
    NNUE_REQUIRE(F <= INT32_MAX / kMaxStacks, NNUE_E_SHAPE, "%s: num_features %d too large for stack selection", fn, F);
  } else {
    scales_ok = scales_ok && m->l2_scale >= 1.0f && m->l1_scale > 0.0f && m->out_scale > 0.0f;
  }
  NNUE_REQUIRE(scales_ok, NNUE_E_ARG, "%s: scales must be positive (integer scales >= 1)", fn);
  return NNUE_OK;
}

// The engine's own stride rule, ceil((H-1)/(g-1)) (nnue_engine.cpp:710-718) -- not the training stride -- and the
// rejection of an image whose conv map would overrun the engine's grid buffer.
static int engine_conv_geometry(const nnue_engine_model* m, int H, int W, const char* fn, int* stride_out, int* oh_out, int* ow_out) {
  const int g = m->grid, oc = m->oc, F = m->num_features;
  int stride = g > 1 ? (H - 1 + g - 2) / (g - 1) : (H > 1 ? H : 1);
  if (stride < 1) stride = 1;
  const int OH = (H + 2 - 3) / stride + 1, OW = (W + 2 - 3) / stride + 1;
  NNUE_REQUIRE(OH > 0 && OW > 0 && (long long)OH * OW * oc <= F, NNUE_E_SHAPE,
               "%s: a %dx%d image gives a %dx%d map that overruns the engine's %dx%d grid buffer", fn, H, W, OH, OW, g, g);
  *stride_out = stride;
  *oh_out = OH;
  *ow_out = OW;
  return NNUE_OK;
}

// The tail's tensors as the kernels take them: the model's stack, or the base of the packed stacks (their scales travel in
// the StackSel instead).
struct EngineTailArgs {
  const int8_t* l1_w;
  const int32_t* l1_b;
  float l1_scale;
  const int8_t* l2_w;
  const int32_t* l2_b;
  int l2_scale;
  const int8_t* out_w;
  const int32_t* out_b;
  float out_scale;
};

static EngineTailArgs engine_tail_args(const nnue_engine_model* m, const nnue_engine_stacks* st) {
  if (st) return {st->l1_w, st->l1_b, 0.0f, st->l2_w, st->l2_b, 1, st->out_w, st->out_b, 0.0f};
  return {m->l1_w, m->l1_b, m->l1_scale, m->l2_w, m->l2_b, (int)m->l2_scale, m->out_w, m->out_b, m->out_scale};
}

static StackSel engine_stack_sel(const nnue_engine_stacks* st, const int32_t* stack_in, int32_t* stack_out) {
  StackSel sel{};
  sel.K = st->count;
  sel.stack_in = stack_in;
  sel.stack_out = stack_out;
  for (int k = 0; k < st->count; ++k) {
    sel.l1_scale[k] = st->scales[3 * k];
    sel.l2_scale[k] = (int)st->scales[3 * k + 1];
    sel.out_scale[k] = st->scales[3 * k + 2];
  }
  return sel;
}

template <class Sel>
static void engine_launch_stack(const nnue_engine_model* m, const EngineTailArgs& t, const int8_t* conv, int B, size_t lds,
                                float* logits, float* density, Sel sel, hipStream_t s) {
  hipLaunchKernelGGL((engine_stack_kernel<Sel>), dim3(B), dim3(256), lds, s, conv, m->threshold, m->num_features, m->oc, m->ft_w,
                     m->ft_b, (int)(int16_t)m->quantized_one, t.l1_w, t.l1_b, t.l1_scale, t.l2_w, t.l2_b, t.l2_scale, t.out_w,
                     t.out_b, t.out_scale, m->l1, m->l2, m->l3, m->classes, logits, density, sel);
}

// nnue_engine_evaluate_logits (select == false; st, stack_in and stack_out unused) and nnue_engine_evaluate_logits_stacks.
static int engine_evaluate(const char* fn, const nnue_engine_model* m, bool select, const nnue_engine_stacks* st,
                           const float* images, int B, int H, int W, const int32_t* stack_in, float* logits, float* density,
                           int32_t* stack_out, void* scratch, int64_t scratch_bytes, nnue_stream_t stream) {
  NNUE_REQUIRE(m && images && logits && density && scratch, NNUE_E_ARG, "%s: null pointer", fn);
  if (select)
    if (int rc = engine_check_stacks(st, stack_out, fn)) return rc;
  NNUE_REQUIRE(engine_has_tensors(m, st), NNUE_E_ARG, "%s: model tensor missing", fn);
  NNUE_REQUIRE(B > 0 && H > 0 && W > 0, NNUE_E_ARG, "%s: B=%d H=%d W=%d must be positive", fn, B, H, W);
  if (int rc = engine_check_model(m, st, fn)) return rc;
  const int oc = m->oc, F = m->num_features;
  int stride, OH, OW;
  if (int rc = engine_conv_geometry(m, H, W, fn, &stride, &OH, &OW)) return rc;
  NNUE_REQUIRE(scratch_bytes >= (int64_t)B * F, NNUE_E_SCRATCH, "%s: scratch %lld < %lld bytes", fn, (long long)scratch_bytes,
               (long long)B * F);
  NNUE_REQUIRE((long long)B * H * W * 3 < (1ll << 40), NNUE_E_SHAPE, "%s: batch too large", fn);
  const size_t lds = (size_t)(2 * m->l1 + m->l2 + m->l3 + 4) * sizeof(int32_t);
  NNUE_REQUIRE(lds <= 64 * 1024, NNUE_E_SHAPE, "%s: layer sizes need %zu bytes of LDS", fn, lds);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int8_t* conv = static_cast<int8_t*>(scratch);
  hipLaunchKernelGGL(engine_conv_kernel, dim3((F + 255) / 256, B), dim3(256), 0, s, images, m->conv_w, m->conv_b, m->conv_scale, H, W,
                     stride, OH, OW, oc, F, conv);
  const EngineTailArgs t = engine_tail_args(m, st);
  if (select) engine_launch_stack(m, t, conv, B, lds, logits, density, engine_stack_sel(st, stack_in, stack_out), s);
  else engine_launch_stack(m, t, conv, B, lds, logits, density, NoStackSel{}, s);
  return nnue_launch_status(fn);
}

extern "C" int nnue_engine_evaluate_logits(const nnue_engine_model* m, const float* images, int B, int H, int W, float* logits,
                                           float* density, void* scratch, int64_t scratch_bytes, nnue_stream_t stream) {
  return engine_evaluate("nnue_engine_evaluate_logits", m, false, nullptr, images, B, H, W, nullptr, logits, density, nullptr, scratch,
                         scratch_bytes, stream);
}

extern "C" int nnue_engine_evaluate_logits_stacks(const nnue_engine_model* m, const nnue_engine_stacks* st, const float* images,
                                                  int B, int H, int W, const int32_t* stack_in, float* logits, float* density,
                                                  int32_t* stack_out, void* scratch, int64_t scratch_bytes, nnue_stream_t stream) {
  return engine_evaluate("nnue_engine_evaluate_logits_stacks", m, true, st, images, B, H, W, stack_in, logits, density, stack_out,
                         scratch, scratch_bytes, stream);
}

extern "C" int64_t nnue_engine_stream_state_bytes(const nnue_engine_model* m, int S) {
  if (!m || S <= 0 || m->num_features <= 0 || m->l1 <= 0) return 0;
  return stream_layout(S, m->num_features, m->l1).total;
}

template <bool kFeatures, class Sel>
static void engine_launch_stream(const nnue_engine_model* m, const EngineTailArgs& t, const int8_t* conv, const uint8_t* active,
                                 int S, size_t lds, uint8_t* state, float* logits, float* density, int32_t* changed, Sel sel,
                                 hipStream_t s) {
  hipLaunchKernelGGL((engine_stream_kernel<kFeatures, Sel>), dim3(S), dim3(256), lds, s, conv, active, m->threshold, m->num_features,
                     m->oc, S, m->ft_w, m->ft_b, (int)(int16_t)m->quantized_one, t.l1_w, t.l1_b, t.l1_scale, t.l2_w, t.l2_b,
                     t.l2_scale, t.out_w, t.out_b, t.out_scale, m->l1, m->l2, m->l3, m->classes, state, logits, density, changed, sel);
}

// nnue_engine_stream_step (select == false; st, stack_in and stack_out unused) and nnue_engine_stream_step_stacks.
static int engine_stream_step(const char* fn, const nnue_engine_model* m, bool select, const nnue_engine_stacks* st,
                              const float* images, const uint8_t* active, int S, int H, int W, const int32_t* stack_in, void* state,
                              int64_t state_bytes, float* logits, float* density, int32_t* changed, int32_t* stack_out,
                              void* scratch, int64_t scratch_bytes, nnue_stream_t stream) {
  NNUE_REQUIRE(m && state && logits && density && changed, NNUE_E_ARG, "%s: null pointer", fn);
  if (select)
    if (int rc = engine_check_stacks(st, stack_out, fn)) return rc;
  NNUE_REQUIRE((images != nullptr) != (active != nullptr), NNUE_E_ARG, "%s: pass exactly one of images and active", fn);
  NNUE_REQUIRE(nnue_aligned16(state), NNUE_E_ARG, "%s: state must be 16-byte aligned", fn);
  NNUE_REQUIRE(engine_has_tensors(m, st), NNUE_E_ARG, "%s: model tensor missing", fn);
  NNUE_REQUIRE(S > 0, NNUE_E_ARG, "%s: S=%d must be positive", fn, S);
  if (int rc = engine_check_model(m, st, fn)) return rc;
  const int oc = m->oc, F = m->num_features, L1 = m->l1, W64 = (F + 63) / 64;
  const int64_t need = nnue_engine_stream_state_bytes(m, S);
  NNUE_REQUIRE(state_bytes >= need, NNUE_E_SCRATCH, "%s: state %lld < %lld bytes", fn, (long long)state_bytes, (long long)need);
  const size_t lds = (size_t)((2 * L1 + m->l2 + m->l3 + 8 + 1) & ~1) * sizeof(int32_t) + (size_t)2 * W64 * sizeof(uint64_t);
  NNUE_REQUIRE(lds <= 64 * 1024, NNUE_E_SHAPE, "%s: layer and feature sizes need %zu bytes of LDS", fn, lds);
  int stride = 1, OH = 0, OW = 0;
  if (images) {
    NNUE_REQUIRE(H > 0 && W > 0, NNUE_E_ARG, "%s: H=%d W=%d must be positive", fn, H, W);
    if (int rc = engine_conv_geometry(m, H, W, fn, &stride, &OH, &OW)) return rc;
    NNUE_REQUIRE(scratch, NNUE_E_ARG, "%s: images need scratch", fn);
    NNUE_REQUIRE(scratch_bytes >= (int64_t)S * F, NNUE_E_SCRATCH, "%s: scratch %lld < %lld bytes", fn, (long long)scratch_bytes,
                 (long long)S * F);
    NNUE_REQUIRE((long long)S * H * W * 3 < (1ll << 40), NNUE_E_SHAPE, "%s: batch too large", fn);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint8_t* sp = static_cast<uint8_t*>(state);
  const EngineTailArgs t = engine_tail_args(m, st);
  if (images) {
    int8_t* conv = static_cast<int8_t*>(scratch);
    hipLaunchKernelGGL(engine_conv_kernel, dim3((F + 255) / 256, S), dim3(256), 0, s, images, m->conv_w, m->conv_b, m->conv_scale, H,
                       W, stride, OH, OW, oc, F, conv);
    if (select)
      engine_launch_stream<false>(m, t, conv, nullptr, S, lds, sp, logits, density, changed, engine_stack_sel(st, stack_in, stack_out), s);
    else engine_launch_stream<false>(m, t, conv, nullptr, S, lds, sp, logits, density, changed, NoStackSel{}, s);
  } else {
    if (select)
      engine_launch_stream<true>(m, t, nullptr, active, S, lds, sp, logits, density, changed, engine_stack_sel(st, stack_in, stack_out), s);
    else engine_launch_stream<true>(m, t, nullptr, active, S, lds, sp, logits, density, changed, NoStackSel{}, s);
  }
  return nnue_launch_status(fn);
}

extern "C" int nnue_engine_stream_step(const nnue_engine_model* m, const float* images, const uint8_t* active, int S, int H, int W,
                                       void* state, int64_t state_bytes, float* logits, float* density, int32_t* changed,
                                       void* scratch, int64_t scratch_bytes, nnue_stream_t stream) {
  return engine_stream_step("nnue_engine_stream_step", m, false, nullptr, images, active, S, H, W, nullptr, state, state_bytes, logits,
                            density, changed, nullptr, scratch, scratch_bytes, stream);
}

extern "C" int nnue_engine_stream_step_stacks(const nnue_engine_model* m, const nnue_engine_stacks* st, const float* images,
                                              const uint8_t* active, int S, int H, int W, const int32_t* stack_in, void* state,
                                              int64_t state_bytes, float* logits, float* density, int32_t* changed,
                                              int32_t* stack_out, void* scratch, int64_t scratch_bytes, nnue_stream_t stream) {
  return engine_stream_step("nnue_engine_stream_step_stacks", m, true, st, images, active, S, H, W, stack_in, state, state_bytes, logits,
                            density, changed, stack_out, scratch, scratch_bytes, stream);
}
