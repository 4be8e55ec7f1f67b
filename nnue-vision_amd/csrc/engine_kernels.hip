// Batched GPU restatement of the reference C++ engine's integer inference,
// NNUEEvaluator::evaluate_logits (engine/src/nnue_engine.cpp:704-734), on the quantised tensors of a `.nnue` file:
// what evaluate_compiled_model (evaluate.py:88-385) obtains from one `nnue_inference` subprocess per image.
// All arithmetic is the engine's integer arithmetic, so results are bit-identical to it; three of its behaviours are
// reproduced on purpose (see oracle/nnue_engine_oracle.py): the image buffer is indexed HWC, the conv weight bytes
// are read as [oc][kh][kw][ic], and the conv's dense [out_h][out_w][oc] output is read back flat with row length g.
#include <cstdlib>

#include "common.h"
#include "engine_u8.h"

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

// What a per-image kernel reads of the network, by value in its arguments: the table, one layer stack -- the model's own, or
// stack 0 of K packed stack-major, which engine_select_stack moves to the image's stack -- and the sizes.  engine_net builds it.
struct EngineNet {
  const int16_t* __restrict__ ft_w;
  const int32_t* __restrict__ ft_b;
  const int8_t* __restrict__ l1_w;
  const int32_t* __restrict__ l1_b;
  const int8_t* __restrict__ l2_w;
  const int32_t* __restrict__ l2_b;
  const int8_t* __restrict__ out_w;
  const int32_t* __restrict__ out_b;
  float l1_scale;
  int l2_scale;
  float out_scale, threshold;
  int quantized_one, F, oc, L1, L2, L3, C;
};

// Dynamic LDS of the per-image kernels, offsets in int32 words from its start:
//   ft [L1] | pair [L1] | h1 [L2] | h2 [L3] | counts [n_counts] | work_n [2] work [n_work] (only with n_work > 0) |
//   (8-byte aligned) n_word_arrays x [W64] u64, W64 = ceil(F / 64)
// The kernels take their pointers from it and the entry points the byte count they launch with and check against 64 KB.
struct EngineLds {
  int pair, h1, h2, counts, work_n, work, words;
  size_t bytes;
};

__host__ __device__ inline EngineLds engine_lds(const EngineNet& net, int n_counts, int n_work, int n_word_arrays) {
  EngineLds l;
  l.pair = net.L1;
  l.h1 = l.pair + net.L1;
  l.h2 = l.h1 + net.L2;
  l.counts = l.h2 + net.L3;
  l.work_n = l.counts + n_counts;
  l.work = l.work_n + (n_work ? 2 : 0);
  const int end = l.work + n_work;
  l.words = (end + 1) & ~1;
  l.bytes = (size_t)(n_word_arrays ? l.words : end) * sizeof(int32_t) + (size_t)n_word_arrays * ((net.F + 63) / 64) * sizeof(uint64_t);
  return l;
}

// Ids of one phase that the row walk of engine_stream_update_kernel takes per round (LDS work list, int32 each).
constexpr int kUpdateChunk = 1024;

// The three uses.  Batched kernels (gather and matrix tail): counts = one active count per wave (the gather form has its count
// in registers and leaves the four words unused).  Stream step: counts = [wave] new, [4 + wave] difference; words = new | old.
// Stream update: the same counts, the work list, words = the current set.
__host__ __device__ inline EngineLds batch_lds(const EngineNet& net) { return engine_lds(net, 4, 0, 0); }
__host__ __device__ inline EngineLds stream_lds(const EngineNet& net) { return engine_lds(net, 8, 0, 2); }
__host__ __device__ inline EngineLds update_lds(const EngineNet& net) { return engine_lds(net, 8, kUpdateChunk, 1); }

// LayerStack::forward_multiclass (nnue_engine.cpp:480-539) of one image, from the clipped accumulator ft [L1] at the start of
// the LDS to its logits row; shared by all per-image kernels.  The caller synchronises after writing ft.
__device__ __forceinline__ void engine_tail(const EngineNet& net, int32_t* lds, const EngineLds& lay, float* __restrict__ logits_row) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L1 = net.L1, L2 = net.L2, L3 = net.L3;
  const int32_t* ft = lds;
  int32_t *pair = lds + lay.pair, *h1 = lds + lay.h1, *h2 = lds + lay.h2;
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
    const int8_t* __restrict__ wr = net.l1_w + (size_t)o * L1;
    int32_t s = 0;
    for (int k = lane; k < L1; k += 64) s += pair[k] * (int32_t)wr[k];
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) s += __shfl_xor(s, sh);
    if (lane == 0) {
      const float r = (float)(s + net.l1_b[o]) / net.l1_scale;
      h1[o] = clamp_i((int32_t)r, 0, 127);
    }
  }
  __syncthreads();

  // layer 2: integer division, clamp to [-127, 127], ReLU; weights are [L3][2 * L2], first L2 columns used
  for (int o = tid; o < L3; o += 256) {
    const int8_t* __restrict__ wr = net.l2_w + (size_t)o * 2 * L2;
    int32_t s = net.l2_b[o];
    for (int k = 0; k < L2; ++k) s += h1[k] * (int32_t)wr[k];
    int32_t r = clamp_i(s / net.l2_scale, -127, 127);
    h2[o] = r > 0 ? r : 0;
  }
  __syncthreads();

  for (int c = tid; c < net.C; c += 256) {
    const int8_t* __restrict__ wr = net.out_w + (size_t)c * L3;
    int32_t s = net.out_b[c];
    for (int j = 0; j < L3; ++j) s += h2[j] * (int32_t)wr[j];
    logits_row[c] = (float)s / net.out_scale;
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
__device__ __forceinline__ void engine_select_stack(const StackSel& sel, int b, int n, EngineNet& net) {
  int k;
  if (sel.stack_in) {
    k = sel.stack_in[b];
    if (k < 0 || k >= sel.K) k = 0;
  } else {
    k = (int)((unsigned)(n * sel.K) / (unsigned)(net.F + 1));  // n <= F and F * K < 2^31 (checked on the host)
    if (k > sel.K - 1) k = sel.K - 1;
  }
  k = __builtin_amdgcn_readfirstlane(k);
  if (threadIdx.x == 0) sel.stack_out[b] = k;
  net.l1_w += (size_t)k * (net.L2 + 1) * net.L1;
  net.l1_b += (size_t)k * (net.L2 + 1);
  net.l2_w += (size_t)k * net.L3 * 2 * net.L2;
  net.l2_b += (size_t)k * net.L3;
  net.out_w += (size_t)k * net.C * net.L3;
  net.out_b += (size_t)k * net.C;
  net.l1_scale = sel.l1_scale[k];
  net.l2_scale = sel.l2_scale[k];
  net.out_scale = sel.out_scale[k];
}

// The epilogue of every per-image kernel, after a barrier behind the stores to ft: the stack of image b, chosen from its active
// count n where the call selects, and the tail into the image's logits row.
template <class Sel>
__device__ __forceinline__ void engine_epilogue(EngineNet net, const Sel& sel, int b, int n, int32_t* lds, const EngineLds& lay,
                                                float* __restrict__ logits) {
  if constexpr (Sel::kSelect) engine_select_stack(sel, b, n, net);
  engine_tail(net, lds, lay, logits + (size_t)b * net.C);
}

// Whether feature f of a row of F map bytes is on, as one lane of a ballot.  kFeatures: the row is a caller's map, non-zero = on,
// every id counts (the reference's entry that takes feature indices applies no per-cell channel mask); otherwise conv bytes,
// and the division by oc is reached only where the byte passes the threshold.  matrix_a_chunk states the same rule on the
// bytes of a chunk with a running channel (through a shared helper the product kernels compile to 40 more instructions).
template <bool kFeatures>
__device__ __forceinline__ bool feature_on(const uint8_t* __restrict__ row, int f, const EngineNet& net) {
  if (f >= net.F) return false;
  if constexpr (kFeatures) return row[f] != 0;
  else return (float)(int8_t)row[f] > net.threshold && (f % net.oc) < 64;  // 64 channels per cell are bit-packed
}

// A thread's columns of the accumulator, tid + 256 j (those below L1), in int32 registers; the int16 accumulator they stand for
// wraps, and addition mod 2^16 does not depend on the width it is carried in.  acc_seed: from stored sums, or from the bias
// (accs == nullptr).  row_add: plus or minus one table row.  acc_finish: the bias where the sums do not hold it yet (kBias),
// wrap to int16, store the sums where the kernel keeps them (kStore), clipped ReLU into ft.
__device__ __forceinline__ void acc_seed(const EngineNet& net, const int16_t* __restrict__ accs, int32_t (&acc)[kMaxColsPerThread]) {
#pragma unroll
  for (int j = 0; j < kMaxColsPerThread; ++j) {
    const int col = threadIdx.x + 256 * j;
    acc[j] = col < net.L1 ? (accs ? (int32_t)accs[col] : (int32_t)(int16_t)net.ft_b[col]) : 0;
  }
}

template <bool kAdd>
__device__ __forceinline__ void row_add(const EngineNet& net, int row, int32_t (&acc)[kMaxColsPerThread]) {
  const int tid = threadIdx.x;
  const int16_t* __restrict__ wr = net.ft_w + (size_t)row * net.L1;
#pragma unroll
  for (int j = 0; j < kMaxColsPerThread; ++j) {
    const int col = tid + 256 * j;
    if (col < net.L1) acc[j] += kAdd ? (int32_t)wr[col] : -(int32_t)wr[col];
  }
}

// max(0, min(v, q1)) in the engine's order (nnue_engine.cpp:726-729): with a negative quantized_one the result is 0 everywhere,
// where a clamp that tests the lower bound first would give quantized_one for every v >= 0.
__device__ __forceinline__ int32_t wrap_clip(int32_t sum, int quantized_one) {
  const int32_t v = (int32_t)(int16_t)sum;  // int16 accumulator wraps
  const int32_t m = v < quantized_one ? v : quantized_one;
  return m > 0 ? m : 0;
}

template <bool kBias, bool kStore>
__device__ __forceinline__ void acc_finish(const EngineNet& net, const int32_t (&acc)[kMaxColsPerThread], int16_t* __restrict__ accs,
                                           int32_t* ft) {
#pragma unroll
  for (int j = 0; j < kMaxColsPerThread; ++j) {
    const int col = threadIdx.x + 256 * j;
    if (col < net.L1) {
      const int32_t sum = kBias ? (int32_t)(int16_t)net.ft_b[col] + acc[j] : acc[j];
      if (kStore) accs[col] = (int16_t)sum;
      ft[col] = wrap_clip(sum, net.quantized_one);
    }
  }
}

// One workgroup per image: feature grid + FeatureTransformer (int16 wrap-around) + clipped ReLU + forward_multiclass
// (nnue_engine.h:236-283, simd_scalar.cpp:78-96, nnue_engine.cpp:726-729, :480-539).  dynamic LDS: batch_lds.
// Sel = StackSel: the image's stack is resolved from `count` before the tail (see engine_select_stack).
template <class Sel>
__global__ __launch_bounds__(256) void engine_stack_kernel(EngineNet net, const uint8_t* __restrict__ conv, float* __restrict__ logits,
                                                           float* __restrict__ density, Sel sel) {
  extern __shared__ int32_t lds[];
  const int b = blockIdx.x, lane = threadIdx.x & 63, F = net.F;
  const uint8_t* __restrict__ cv = conv + (size_t)b * F;

  // active features, ascending: every wave forms the same ballots and adds the rows to its own columns
  int32_t acc[kMaxColsPerThread] = {};  // the bias joins at the finish: its loads up front would delay the first rows
  int count = 0;
  for (int f0 = 0; f0 < F; f0 += 64) {
    unsigned long long mask = __ballot(feature_on<false>(cv, f0 + lane, net));
    count += __popcll(mask);
    while (mask) {
      const int row = f0 + __builtin_ctzll(mask);
      mask &= mask - 1;
      row_add<true>(net, row, acc);
    }
  }
  acc_finish<true, false>(net, acc, nullptr, lds);
  if (threadIdx.x == 0) density[b] = (float)count / (float)F;
  __syncthreads();
  engine_epilogue(net, sel, b, count, lds, batch_lds(net), logits);
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

// Stream b's part of the state: its valid flag, its parity, its accumulator, and the bit words of either slot.
struct StreamView {
  int32_t* __restrict__ valid;
  int32_t* __restrict__ parity;
  int16_t* __restrict__ accs;
  unsigned long long* bits;  // slot 0 of the stream
  size_t slot_stride;        // in words
  __device__ __forceinline__ unsigned long long* words(int slot) const { return bits + slot * slot_stride; }
};

__device__ __forceinline__ StreamView stream_view(uint8_t* state, int S, int F, int L1, int b) {
  const StreamLayout lay = stream_layout(S, F, L1);
  const size_t W64 = (F + 63) / 64;
  StreamView v;
  v.valid = reinterpret_cast<int32_t*>(state) + b;
  v.parity = reinterpret_cast<int32_t*>(state + lay.parity) + b;
  v.accs = reinterpret_cast<int16_t*>(state + lay.acc) + (size_t)b * L1;
  v.bits = reinterpret_cast<unsigned long long*>(state + lay.bits) + b * W64;
  v.slot_stride = S * W64;
  return v;
}

// NNUEEvaluator::evaluate_incremental (nnue_engine.cpp:739-786) for S independent streams, one workgroup per stream: the new
// feature set, the difference to the stream's previous one, and FeatureTransformer::update_accumulator (:257-267) on the
// stored int16 accumulator -- or refresh_accumulator (:806-816) from the bias when the stream is not valid, or when the
// difference holds more features than the new set (then a refresh reads fewer table rows).  Both give the same bits: the
// accumulator is int16 and wraps, and addition mod 2^16 does not depend on the order or the history of the terms.
// Then the clipped ReLU and engine_tail, as engine_stack_kernel.
// kFeatures: src is a uint8 map active [S][F], otherwise the conv bytes (see feature_on).
// Read/write hazard on the bit words: they ping-pong between two slots ([2][S][W64] + a per-stream parity that flips at the
// end of the step).  Every wave may read the old words at any time during the step while the new ones are stored into the
// other slot, so no barrier has to order those reads before the stores, and a launch never reads a word it writes.
// dynamic LDS: stream_lds.
// Sel = StackSel: the stream's stack is resolved from `n_new` before the tail (see engine_select_stack); the state is the same.
template <bool kFeatures, class Sel>
__global__ __launch_bounds__(256) void engine_stream_kernel(EngineNet net, const uint8_t* __restrict__ src, int S,
                                                            uint8_t* __restrict__ state, float* __restrict__ logits,
                                                            float* __restrict__ density, int32_t* __restrict__ changed, Sel sel) {
  extern __shared__ int32_t lds[];
  const EngineLds lay = stream_lds(net);
  const int F = net.F, W64 = (F + 63) / 64;
  int32_t* counts = lds + lay.counts;  // [wave] new, [4 + wave] difference
  unsigned long long* new_s = reinterpret_cast<unsigned long long*>(lds + lay.words);
  unsigned long long* old_s = new_s + W64;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  const StreamView sv = stream_view(state, S, F, net.L1, b);
  const bool was_valid = *sv.valid != 0;
  const int par = *sv.parity & 1;
  const unsigned long long* __restrict__ old_w = sv.words(par);
  unsigned long long* __restrict__ new_w = sv.words(par ^ 1);

  // pass 1: wave w forms the ballots of chunks w, w + 4, ...: new set -> its slot and LDS, old set -> LDS, both popcounts
  int n_new = 0, n_diff = 0;
  for (int c = wave; c < W64; c += 4) {
    const unsigned long long m = __ballot(feature_on<kFeatures>(src + (size_t)b * F, c * 64 + lane, net));
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
  acc_seed(net, refresh ? nullptr : sv.accs, acc);
  for (int c = 0; c < W64; ++c) {
    const unsigned long long m = new_s[c], o = refresh ? 0ull : old_s[c];
    unsigned long long add = m & ~o, sub = o & ~m;
    for (; add; add &= add - 1) row_add<true>(net, c * 64 + __builtin_ctzll(add), acc);
    for (; sub; sub &= sub - 1) row_add<false>(net, c * 64 + __builtin_ctzll(sub), acc);
  }
  acc_finish<false, true>(net, acc, sv.accs, lds);
  if (tid == 0) {
    density[b] = (float)n_new / (float)F;
    changed[b] = was_valid ? n_diff : n_new;
    *sv.valid = 1;
    *sv.parity = par ^ 1;
  }
  __syncthreads();
  engine_epilogue(net, sel, b, n_new, lds, lay, logits);
}

// Stream b's range of a CSR list, clipped to the id buffer: [off[b], off[b + 1]) cut to [0, n], a reversed range = empty.  A
// list with n == 0 is never dereferenced (its pointers may be null).
__device__ __forceinline__ void update_range(const int32_t* __restrict__ off, int n, int b, int& lo, int& hi) {
  lo = hi = 0;
  if (n <= 0) return;
  lo = off[b];
  hi = off[b + 1];
  lo = lo < 0 ? 0 : (lo > n ? n : lo);
  hi = hi < 0 ? 0 : (hi > n ? n : hi);
  if (hi < lo) hi = lo;
}

// One phase of the update: ids[lo, hi) are cleared from (kAdd == false) or set in (kAdd == true) the stream's bit words in LDS.
// A 64-bit LDS atomic returns the word as it was, so of all threads that name one id -- duplicates included -- exactly the one
// that flipped its bit appends the id to the work list; ids outside [0, F) and ids whose bit already has the wanted value flip
// nothing.  After a barrier all 256 threads walk the list and subtract or add those table rows in their own columns (walk ==
// false: the bits only, the caller re-forms the sums afterwards).  Four rows per trip, padded with row 0 times 0, so that the
// loads of a trip do not wait for one another.  The list's counter only grows: `done` is its value before this round, known to
// every thread, so a round needs no reset and two barriers -- appends | walk | next round's appends.
template <bool kAdd>
__device__ __forceinline__ void update_phase(const int32_t* __restrict__ ids, int lo, int hi, int F, int L1, bool walk,
                                             const int16_t* __restrict__ ft_w, unsigned long long* cur, int32_t* work,
                                             unsigned* work_n, unsigned& done, int32_t (&acc)[kMaxColsPerThread]) {
  const int tid = threadIdx.x;
  for (int base = lo, len; base < hi; base += len) {  // lo, hi are uniform over the workgroup; no sum here can pass hi <= 2^31 - 1
    len = hi - base < kUpdateChunk ? hi - base : kUpdateChunk;
    for (int i = tid; i < len; i += 256) {
      const int id = ids[(size_t)base + i];
      if ((unsigned)id >= (unsigned)F) continue;
      const unsigned long long bit = 1ull << (id & 63);
      const unsigned long long was = kAdd ? atomicOr(&cur[id >> 6], bit) : atomicAnd(&cur[id >> 6], ~bit);
      if (((was & bit) != 0) != kAdd) work[atomicAdd(work_n, 1u) - done] = id;  // at most len <= kUpdateChunk appends
    }
    __syncthreads();
    const int n = (int)(*work_n - done);  // unsigned: the counter may wrap, the difference does not
    done += (unsigned)n;
    if (walk) {
      for (int i = 0; i < n; i += 4) {
        const int16_t* __restrict__ wr[4];
        int32_t mul[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bool in = i + u < n;
          wr[u] = ft_w + (size_t)(in ? work[i + u] : 0) * L1;
          mul[u] = in ? (kAdd ? 1 : -1) : 0;
        }
#pragma unroll
        for (int j = 0; j < kMaxColsPerThread; ++j) {
          const int col = tid + 256 * j;
          if (col < L1) {
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[j] += mul[u] * (int32_t)wr[u][col];
          }
        }
      }
    }
    __syncthreads();  // the walk has read the list and its counter before the next round appends
  }
}

// FeatureTransformer::update_accumulator (nnue_engine.cpp:257-267; NNUEEvaluator::update_features, :818-821) for S independent
// streams from two CSR id lists, one workgroup per stream, on the state of engine_stream_kernel -- with set semantics: the stored
// set stays the true set, new = (old \ removed) + added, and the accumulator stays bias + sum of rows(set) mod 2^16.  Ids outside
// [0, F) are ignored (add_feature / remove_feature, :233-234), a removed id that is off and an added id that is on are ignored,
// a duplicate counts once; an id in both lists ends up on (removed first, then added: on a feature that was on the two rows
// cancel mod 2^16).  On lists without such entries this is update_accumulator bit for bit.  A stream that is not valid starts from
// the empty set and the bias and ignores `removed`: refresh_accumulator(added) (:806-816).  rebuild != 0 (all streams): the
// delta goes into the bits only and every accumulator is re-formed from the bias and the rows of its new set, the stored sums
// being ignored (they belong to another table).  Then the clipped ReLU and engine_tail, as engine_stream_kernel.
// Read/write hazard on the bit words: the stream's CURRENT slot is updated in place and the parity stays.  A workgroup touches
// only its own stream's words, and within it word c belongs to thread c % 256 alone: that thread copies it to LDS at the start,
// and at the end reads it again (the old set, for `changed`) and only then stores the new word over it, in program order.  All
// other traffic on the words is LDS atomics between barriers.  No thread reads a global word another thread writes.
// dynamic LDS: update_lds.
template <class Sel>
__global__ __launch_bounds__(256) void engine_stream_update_kernel(
    EngineNet net, const int32_t* __restrict__ added, const int32_t* __restrict__ added_off, int n_added,
    const int32_t* __restrict__ removed, const int32_t* __restrict__ removed_off, int n_removed, int rebuild, int S,
    uint8_t* __restrict__ state, float* __restrict__ logits, float* __restrict__ density, int32_t* __restrict__ changed, Sel sel) {
  extern __shared__ int32_t lds[];
  const EngineLds lay = update_lds(net);
  const int F = net.F, W64 = (F + 63) / 64;
  int32_t* counts = lds + lay.counts;  // [wave] new, [4 + wave] difference
  unsigned* work_n = reinterpret_cast<unsigned*>(lds + lay.work_n);
  int32_t* work = lds + lay.work;
  unsigned long long* cur = reinterpret_cast<unsigned long long*>(lds + lay.words);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  const StreamView sv = stream_view(state, S, F, net.L1, b);
  const bool was_valid = *sv.valid != 0;
  unsigned long long* words = sv.words(*sv.parity & 1);

  for (int c = tid; c < W64; c += 256) cur[c] = was_valid ? words[c] : 0ull;
  if (tid == 0) *work_n = 0;
  const bool walk = rebuild == 0;
  int32_t acc[kMaxColsPerThread];
  acc_seed(net, was_valid && walk ? sv.accs : nullptr, acc);
  __syncthreads();

  // removed before added, with the phases' barriers between them: an id in both lists ends up on
  int lo, hi;
  unsigned done = 0;
  if (was_valid) {
    update_range(removed_off, n_removed, b, lo, hi);
    update_phase<false>(removed, lo, hi, F, net.L1, walk, net.ft_w, cur, work, work_n, done, acc);
  }
  update_range(added_off, n_added, b, lo, hi);
  update_phase<true>(added, lo, hi, F, net.L1, walk, net.ft_w, cur, work, work_n, done, acc);

  if (!walk) {  // every wave walks the same words of the new set, as pass 2 of engine_stream_kernel on a refresh
    for (int c = 0; c < W64; ++c)
      for (unsigned long long m = cur[c]; m; m &= m - 1) row_add<true>(net, c * 64 + __builtin_ctzll(m), acc);
  }

  int n_new = 0, n_diff = 0;
  for (int c = tid; c < W64; c += 256) {
    const unsigned long long m = cur[c], o = was_valid ? words[c] : 0ull;
    n_new += __popcll(m);
    n_diff += __popcll(m ^ o);
    if (!was_valid || m != o) words[c] = m;
  }
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) {
    n_new += __shfl_xor(n_new, sh);
    n_diff += __shfl_xor(n_diff, sh);
  }
  if (lane == 0) {
    counts[wave] = n_new;
    counts[4 + wave] = n_diff;
  }
  acc_finish<false, true>(net, acc, sv.accs, lds);
  __syncthreads();
  n_new = counts[0] + counts[1] + counts[2] + counts[3];
  n_diff = counts[4] + counts[5] + counts[6] + counts[7];
  if (tid == 0) {
    density[b] = (float)n_new / (float)F;
    changed[b] = was_valid ? n_diff : n_new;
    *sv.valid = 1;
  }
  engine_epilogue(net, sel, b, n_new, lds, lay, logits);
}

// What the region step reads besides the network: the uint8 frames (the fields of nnue_engine_u8_frames, layout hwc), the conv's
// bytes, the engine's geometry of an H x W frame, and the CSR list of dirty rectangles [n_rects][4] = y0, x0, y1, x1.
struct RegionFront {
  const uint8_t* __restrict__ data;
  const int64_t* __restrict__ indices;
  int64_t count;
  const int8_t* __restrict__ w;
  const int32_t* __restrict__ bias;
  const int32_t* __restrict__ rects;
  const int32_t* __restrict__ rect_off;
  int n_rects;
  float mean0, mean1, mean2, inv0, inv1, inv2, scale;
  int H, W, stride, OH, OW;
};

// LDS of the region step: update_lds, then the 768-word quantisation table (update_lds ends on an 8-byte boundary).
__host__ __device__ inline size_t regions_lds_bytes(const EngineNet& net) { return update_lds(net).bytes + kU8Table * sizeof(int32_t); }

// The conv byte of cell (oh, ow), channel c, from the frame's bytes: engine_conv_u8_kernel's arithmetic under layout hwc -- the
// table's q, the taps in [oc][kh][kw][ic] order, zero padding outside the frame, truncating division, clamp.  No byte outside
// the frame's 3 * H * W is read.
__device__ __forceinline__ int32_t region_conv_byte(const RegionFront& a, const uint8_t* __restrict__ img, const int32_t* tab, int oh,
                                                    int ow, int c) {
  const int8_t* __restrict__ wr = a.w + c * 27;
  int32_t acc = a.bias[c];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int ih = oh * a.stride + kh - 1;
    if (ih < 0 || ih >= a.H) continue;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int iw = ow * a.stride + kw - 1;
      if (iw < 0 || iw >= a.W) continue;
      const uint8_t* __restrict__ px = img + (ih * a.W + iw) * 3;  // 3 * H * W < 2^31 (checked on the host)
#pragma unroll
      for (int ic = 0; ic < 3; ++ic) acc += tab[ic * 256 + px[ic]] * (int32_t)wr[(kh * 3 + kw) * 3 + ic];
    }
  }
  const int32_t q = acc / (int32_t)a.scale;  // truncating division, as the engine
  return q < -127 ? -127 : (q > 127 ? 127 : q);
}

// Cells of one axis whose three taps, at cell * stride - 1 .. + 1, meet the pixels [p0, p1) (already clipped to the frame, p0 <
// p1): cell * stride + 1 >= p0 and cell * stride - 1 <= p1 - 1, cut to [0, n).  Exact; lo > hi = no cell (at stride >= 3 the
// pixels between two cells' windows belong to none).
__device__ __forceinline__ void region_cells(int p0, int p1, int stride, int n, int& lo, int& hi) {
  lo = p0 <= 1 ? 0 : (p0 - 1 + stride - 1) / stride;
  hi = p1 / stride;
  if (hi > n - 1) hi = n - 1;
}

// One block of candidates of the region step, a candidate being one (cell, channel) pair, in rounds of at most kUpdateChunk.
// full == false: the n candidates are the cells [oh_lo, ..) x [ow_lo, ow_lo + nw) times the oc channels.  full == true: they are
// the ids [0, F) themselves, the ids behind the conv map standing for the zero bytes of the engine's zero-filled buffer.  A
// thread forms its candidate's byte, hence the wanted bit (feature_on's rule), and where the stream's LDS word disagrees sets or
// clears the bit with a 64-bit LDS atomic; the atomic returns the word as it was, so of all threads that name one feature the one
// that flipped it appends the id -- ~id for a feature that went off -- to the work list.  Then all 256 threads walk the list over
// their own columns, four rows per trip, as update_phase (counter, `done` and barriers as there).
__device__ __forceinline__ void regions_phase(const EngineNet& net, const RegionFront& a, const uint8_t* __restrict__ img,
                                              const int32_t* tab, bool full, int n, int oh_lo, int ow_lo, int nw,
                                              unsigned long long* cur, int32_t* work, unsigned* work_n, unsigned& done,
                                              int32_t (&acc)[kMaxColsPerThread]) {
  const int tid = threadIdx.x, oc = net.oc, L1 = net.L1;
  const int map = a.OH * a.OW * oc;  // <= F (checked on the host)
  for (int base = 0, len; base < n; base += len) {  // n <= F, uniform over the workgroup
    len = n - base < kUpdateChunk ? n - base : kUpdateChunk;
    for (int i = tid; i < len; i += 256) {
      const int idx = base + i;
      int id, c;
      int32_t q = 0;
      if (full) {
        id = idx;
        const int pos = id / oc;
        c = id - pos * oc;
        if (id < map) {
          const int oh = pos / a.OW;
          q = region_conv_byte(a, img, tab, oh, pos - oh * a.OW, c);
        }
      } else {
        const int cell = idx / oc, r = cell / nw;
        c = idx - cell * oc;
        const int oh = oh_lo + r, ow = ow_lo + cell - r * nw;
        id = (oh * a.OW + ow) * oc + c;
        q = region_conv_byte(a, img, tab, oh, ow, c);
      }
      const bool want = (float)(int8_t)q > net.threshold && c < 64;  // 64 channels per cell are bit-packed
      const unsigned long long bit = 1ull << (id & 63);
      if (((cur[id >> 6] & bit) != 0) == want) continue;
      const unsigned long long was = want ? atomicOr(&cur[id >> 6], bit) : atomicAnd(&cur[id >> 6], ~bit);
      if (((was & bit) != 0) != want) work[atomicAdd(work_n, 1u) - done] = want ? id : ~id;  // at most len <= kUpdateChunk appends
    }
    __syncthreads();
    const int m = (int)(*work_n - done);  // unsigned: the counter may wrap, the difference does not
    done += (unsigned)m;
    for (int i = 0; i < m; i += 4) {
      const int16_t* __restrict__ wr[4];
      int32_t mul[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool in = i + u < m;
        const int32_t e = in ? work[i + u] : 0;
        wr[u] = net.ft_w + (size_t)(e < 0 ? ~e : e) * L1;
        mul[u] = in ? (e < 0 ? -1 : 1) : 0;
      }
#pragma unroll
      for (int j = 0; j < kMaxColsPerThread; ++j) {
        const int col = tid + 256 * j;
        if (col < L1) {
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[j] += mul[u] * (int32_t)wr[u][col];
        }
      }
    }
    __syncthreads();  // the walk has read the list and its counter before the next round appends
  }
}

// evaluate_incremental / update_features (nnue_engine.cpp:739-786, :818-821) for S streams whose feature lists are derived on
// the device from the dirty rectangles of uint8 frames, one workgroup per stream, on the state of engine_stream_kernel.  Set
// arithmetic: every feature of a cell whose 3 x 3 window meets one of the stream's rectangles (each clipped to the frame) takes
// the value the whole-frame u8 step would give it on this frame (ConvLayer::forward, :48-158, on the bytes; feature_on's rule);
// every other bit of the stored set keeps its value; the accumulator stays bias + sum of rows(set) mod 2^16.  Overlapping and
// repeated rectangles recompute a cell to the same bit and flip nothing; an empty, inverted or outside rectangle selects no
// cell.  A stream that is not valid ignores its rectangles: every id of [0, F) is a candidate, from the empty set and the bias.
// Then the popcounts, the clipped ReLU and engine_tail, as engine_stream_update_kernel.
// Read/write hazard on the bit words: as engine_stream_update_kernel -- the current slot is updated in place, word c belongs to
// thread c % 256 alone at both ends, all other traffic on the words is LDS atomics and reads of bits no other thread of the
// round names, between barriers.
// dynamic LDS: regions_lds_bytes.
template <class Sel>
__global__ __launch_bounds__(256) void engine_stream_regions_kernel(EngineNet net, RegionFront a, int S, uint8_t* __restrict__ state,
                                                                    float* __restrict__ logits, float* __restrict__ density,
                                                                    int32_t* __restrict__ changed, Sel sel) {
  extern __shared__ int32_t lds[];
  const EngineLds lay = update_lds(net);
  const int F = net.F, W64 = (F + 63) / 64;
  int32_t* counts = lds + lay.counts;  // [wave] new, [4 + wave] difference
  unsigned* work_n = reinterpret_cast<unsigned*>(lds + lay.work_n);
  int32_t* work = lds + lay.work;
  unsigned long long* cur = reinterpret_cast<unsigned long long*>(lds + lay.words);
  int32_t* tab = reinterpret_cast<int32_t*>(cur + W64);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  const StreamView sv = stream_view(state, S, F, net.L1, b);
  const bool was_valid = *sv.valid != 0;
  unsigned long long* words = sv.words(*sv.parity & 1);

  for (int c = tid; c < W64; c += 256) cur[c] = was_valid ? words[c] : 0ull;
  tab[tid] = u8_quantise(tid, a.mean0, a.inv0, a.scale);
  tab[256 + tid] = u8_quantise(tid, a.mean1, a.inv1, a.scale);
  tab[512 + tid] = u8_quantise(tid, a.mean2, a.inv2, a.scale);
  if (tid == 0) *work_n = 0;
  int32_t acc[kMaxColsPerThread];
  acc_seed(net, was_valid ? sv.accs : nullptr, acc);

  int64_t idx = b;  // without indices: frame b, and count >= S (checked on the host)
  if (a.indices) {
    idx = a.indices[b];
    idx = idx < 0 ? 0 : (idx >= a.count ? a.count - 1 : idx);  // as load_batch_kernel
  }
  const uint8_t* __restrict__ img = a.data + (size_t)idx * 3 * a.H * a.W;
  __syncthreads();

  unsigned done = 0;
  if (!was_valid) {
    regions_phase(net, a, img, tab, true, F, 0, 0, 1, cur, work, work_n, done, acc);
  } else {
    int lo, hi;
    update_range(a.rect_off, a.n_rects, b, lo, hi);
    for (int r = lo; r < hi; ++r) {  // uniform over the workgroup: every thread reads the same four words
      const int32_t* __restrict__ rc = a.rects + (size_t)r * 4;
      int y0 = rc[0], x0 = rc[1], y1 = rc[2], x1 = rc[3];
      y0 = y0 < 0 ? 0 : y0, x0 = x0 < 0 ? 0 : x0;
      y1 = y1 > a.H ? a.H : y1, x1 = x1 > a.W ? a.W : x1;
      if (y0 >= y1 || x0 >= x1) continue;
      int oh_lo, oh_hi, ow_lo, ow_hi;
      region_cells(y0, y1, a.stride, a.OH, oh_lo, oh_hi);
      region_cells(x0, x1, a.stride, a.OW, ow_lo, ow_hi);
      if (oh_lo > oh_hi || ow_lo > ow_hi) continue;
      const int nw = ow_hi - ow_lo + 1;
      regions_phase(net, a, img, tab, false, (oh_hi - oh_lo + 1) * nw * net.oc, oh_lo, ow_lo, nw, cur, work, work_n, done, acc);
    }
  }

  int n_new = 0, n_diff = 0;
  for (int c = tid; c < W64; c += 256) {
    const unsigned long long m = cur[c], o = was_valid ? words[c] : 0ull;
    n_new += __popcll(m);
    n_diff += __popcll(m ^ o);
    if (!was_valid || m != o) words[c] = m;
  }
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) {
    n_new += __shfl_xor(n_new, sh);
    n_diff += __shfl_xor(n_diff, sh);
  }
  if (lane == 0) {
    counts[wave] = n_new;
    counts[4 + wave] = n_diff;
  }
  acc_finish<false, true>(net, acc, sv.accs, lds);
  __syncthreads();
  n_new = counts[0] + counts[1] + counts[2] + counts[3];
  n_diff = counts[4] + counts[5] + counts[6] + counts[7];
  if (tid == 0) {
    density[b] = (float)n_new / (float)F;
    changed[b] = was_valid ? n_diff : n_new;
    *sv.valid = 1;
  }
  engine_epilogue(net, sel, b, n_new, lds, lay, logits);
}

// ---- whole batches on the int8 matrix unit --------------------------------------------------------------------------
// The accumulate step of engine_stack_kernel as a matrix product: sums [B][L1] int32 = A [B][F] . table, with A the 0/1 byte map
// of the active features and the int16 table as one int8 plane (every value fits a byte) or two (lo, hi: w == lo + 256 * hi
// mod 2^16, hi may wrap).  Addition mod 2^16 does not depend on the order or on the accumulator's width, so the int32 sums,
// truncated to int16 by the tail, are the engine's wrapped int16 sums bit for bit.  F < 2^24 keeps every int32 partial sum of
// int8 products inside int32 (F * 128 < 2^31).
// Plane layout (engine_pack_table_kernel writes it, the product's B-operand loads read it): [Kpad / 16][Npad][16] bytes, the 16
// bytes being 16 consecutive features of one column -- one 16-byte load is one lane's B fragment of v_mfma_i32_32x32x32_i8
// (lane l: column l & 31, features 16 * (l >> 5) .. + 15 of the 32).  Kpad, Npad: F, L1 rounded up to the K and N tile, zero-filled.
constexpr int kMxBM = 128, kMxBN = 128, kMxBK = 64;
constexpr int kMxAPitch = kMxBK + 16;  // LDS row pitch of the A tile in bytes (16-byte aligned rows, banks staggered)
constexpr int kMxMaxFeatures = 1 << 24;
constexpr int kMxMinTilesPerSlab = 4;

typedef int mx_i32x4 __attribute__((ext_vector_type(4)));
typedef int mx_i32x16 __attribute__((ext_vector_type(16)));

union MxChunk {
  uint4 v;
  mx_i32x4 i;
  uint8_t b[16];
};

struct MatrixLayout {
  int64_t kpad, npad, plane_bytes, sums, total;  // sums: byte offset of the int32 [B][L1] sums in the scratch
};

__host__ __device__ inline MatrixLayout matrix_layout(int64_t B, int64_t F, int64_t L1) {
  MatrixLayout l;
  l.kpad = (F + kMxBK - 1) / kMxBK * kMxBK;
  l.npad = (L1 + kMxBN - 1) / kMxBN * kMxBN;
  l.plane_bytes = l.kpad * l.npad;
  l.sums = (B * F + 255) / 256 * 256;
  l.total = l.sums + B * L1 * 4;
  return l;
}

// One thread = the 16 bytes of (16 features, one column) of every plane.  kPlanes == 1: an element outside [-128, 127] is packed
// as its low byte and counted into misfit[0], one atomic per wave that saw any.
template <int kPlanes>
__global__ __launch_bounds__(256) void engine_pack_table_kernel(const int16_t* __restrict__ ft_w, int F, int L1, int npad,
                                                                int64_t chunks, int64_t plane_bytes, int8_t* __restrict__ planes,
                                                                int32_t* __restrict__ misfit) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int bad = 0;
  if (c < chunks) {
    const int64_t kb = c / npad;
    const int n = (int)(c - kb * npad);
    MxChunk lo, hi;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int64_t k = kb * 16 + j;
      const int32_t w = (k < F && n < L1) ? (int32_t)ft_w[k * L1 + n] : 0;
      const int8_t l = (int8_t)(w & 0xff);
      lo.b[j] = (uint8_t)l;
      hi.b[j] = (uint8_t)((w - (int32_t)l) >> 8);  // may wrap as int8: 256 * 256 == 0 (mod 2^16)
      if (kPlanes == 1 && w != (int32_t)l) ++bad;
    }
    *reinterpret_cast<uint4*>(planes + c * 16) = lo.v;
    if (kPlanes == 2) *reinterpret_cast<uint4*>(planes + plane_bytes + c * 16) = hi.v;
  }
  if (kPlanes == 1) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(misfit, bad);
  }
}

// The 0/1 bytes of features f0 .. f0 + 15 of image b (zeros beyond B or F).  kFeatures: src is the caller's map, non-zero = on,
// every id counts; otherwise the conv bytes under feature_on's rule.
template <bool kFeatures>
__device__ __forceinline__ uint4 matrix_a_chunk(const uint8_t* __restrict__ src, int b, int f0, int B, int F, float threshold, int oc,
                                                bool aligned) {
  MxChunk raw, out;
  raw.v = make_uint4(0, 0, 0, 0);
  out.v = make_uint4(0, 0, 0, 0);
  if (b >= B || f0 >= F) return out.v;
  const uint8_t* __restrict__ p = src + (size_t)b * F + f0;
  const int n = F - f0 < 16 ? F - f0 : 16;
  if (aligned) {  // F is a multiple of 16 here, so the chunk lies inside the row
    raw.v = *reinterpret_cast<const uint4*>(p);
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j < n) raw.b[j] = p[j];
  }
  int ch = kFeatures ? 0 : f0 % oc;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    bool on;  // feature_on's rule, stated a second time on purpose (see there)
    if constexpr (kFeatures) {
      on = raw.b[j] != 0;
    } else {
      on = (float)(int8_t)raw.b[j] > threshold && ch < 64;  // 64 channels per cell are bit-packed
      if (++ch == oc) ch = 0;
    }
    out.b[j] = (j < n && on) ? 1 : 0;
  }
  return out.v;
}

// grid (Npad / 128, ceil(B / 128), slabs), 256 threads = 2 x 2 waves of 64 x 64 results (2 x 2 MFMA tiles of 32 x 32 per plane).
// A K tile of 64 features: the A bytes are formed from src while staging (matrix_a_chunk) into LDS rows, the plane bytes are
// copied as they lie; both products of a two-plane table share the A fragments and combine as lo + (hi << 8) before the wrap.
// A slab covers tiles_per_slab K tiles; with more than one slab the partial sums meet by integer atomics in the zeroed sums
// (bit-exact for any slab count: integer addition is associative).
template <int kPlanes, bool kFeatures>
__global__ __launch_bounds__(256) void engine_matrix_product_kernel(const uint8_t* __restrict__ src, float threshold, int oc, int B,
                                                                    int F, int L1, int npad, int64_t plane_bytes,
                                                                    const int8_t* __restrict__ planes, int ktiles, int tiles_per_slab,
                                                                    int aligned, int atomic, int32_t* __restrict__ sums) {
  __shared__ __attribute__((aligned(16))) uint8_t a_s[kMxBM * kMxAPitch];
  __shared__ __attribute__((aligned(16))) uint8_t b_s[kPlanes][(kMxBK / 16) * kMxBN * 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;
  const int n0 = blockIdx.x * kMxBN, m0 = blockIdx.y * kMxBM;
  const int kt0 = blockIdx.z * tiles_per_slab;
  const int kt1 = kt0 + tiles_per_slab < ktiles ? kt0 + tiles_per_slab : ktiles;

  mx_i32x16 acc[kPlanes][2][2];
#pragma unroll
  for (int p = 0; p < kPlanes; ++p)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[p][i][j][e] = 0;

  uint4 a_reg[2], b_reg[kPlanes][2];
  auto load = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i;  // A: 128 rows x 4 chunks; planes: 4 feature blocks x 128 columns
      a_reg[i] = matrix_a_chunk<kFeatures>(src, m0 + (c >> 2), kt * kMxBK + 16 * (c & 3), B, F, threshold, oc, aligned != 0);
      const int64_t chunk = ((int64_t)kt * (kMxBK / 16) + (c >> 7)) * npad + n0 + (c & 127);
#pragma unroll
      for (int p = 0; p < kPlanes; ++p) b_reg[p][i] = *reinterpret_cast<const uint4*>(planes + p * plane_bytes + chunk * 16);
    }
  };
  if (kt0 < kt1) load(kt0);
  for (int kt = kt0; kt < kt1; ++kt) {
    __syncthreads();  // the previous tile's fragment reads are done
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = tid + 256 * i;
      *reinterpret_cast<uint4*>(a_s + (c >> 2) * kMxAPitch + 16 * (c & 3)) = a_reg[i];
#pragma unroll
      for (int p = 0; p < kPlanes; ++p) *reinterpret_cast<uint4*>(b_s[p] + c * 16) = b_reg[p][i];
    }
    __syncthreads();
    if (kt + 1 < kt1) load(kt + 1);  // in flight under the products
#pragma unroll
    for (int ks = 0; ks < kMxBK / 32; ++ks) {
      mx_i32x4 af[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        af[i] = *reinterpret_cast<const mx_i32x4*>(a_s + (wm * 64 + i * 32 + r) * kMxAPitch + ks * 32 + 16 * h);
#pragma unroll
      for (int p = 0; p < kPlanes; ++p)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const mx_i32x4 bf = *reinterpret_cast<const mx_i32x4*>(b_s[p] + ((ks * 2 + h) * kMxBN + wn * 64 + j * 32 + r) * 16);
#pragma unroll
          for (int i = 0; i < 2; ++i) acc[p][i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[i], bf, acc[p][i][j], 0, 0, 0);
        }
    }
  }

  // C/D map of the 32 x 32 MFMA: column = lane & 31, row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn * 64 + j * 32 + r;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        uint32_t v = (uint32_t)acc[0][i][j][e];
        if (kPlanes == 2) v += (uint32_t)acc[kPlanes - 1][i][j][e] << 8;
        if (row < B && col < L1) {
          int32_t* dst = sums + (size_t)row * L1 + col;
          if (atomic) atomicAdd(dst, (int32_t)v);
          else *dst = (int32_t)v;
        }
      }
    }
}

// One workgroup per image, as engine_stack_kernel after its gather: the image's active count under the product's predicate
// (once per image, for density and the stack selector), the wrapped int16 accumulator from the int32 sums, clipped ReLU, tail.
// dynamic LDS: batch_lds.
template <bool kFeatures, class Sel>
__global__ __launch_bounds__(256) void engine_matrix_tail_kernel(EngineNet net, const uint8_t* __restrict__ src,
                                                                 const int32_t* __restrict__ sums, float* __restrict__ logits,
                                                                 float* __restrict__ density, Sel sel) {
  extern __shared__ int32_t lds[];
  const EngineLds lay = batch_lds(net);
  int32_t* counts = lds + lay.counts;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, F = net.F;
  const uint8_t* __restrict__ row = src + (size_t)b * F;
  int count = 0;
  for (int f0 = wave * 64; f0 < F; f0 += 256) count += __popcll(__ballot(feature_on<kFeatures>(row, f0 + lane, net)));
  if (lane == 0) counts[wave] = count;
  for (int col = tid; col < net.L1; col += 256)
    lds[col] = wrap_clip((int32_t)((uint32_t)net.ft_b[col] + (uint32_t)sums[(size_t)b * net.L1 + col]), net.quantized_one);
  __syncthreads();
  count = counts[0] + counts[1] + counts[2] + counts[3];
  if (tid == 0) density[b] = (float)count / (float)F;
  engine_epilogue(net, sel, b, count, lds, lay, logits);
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

struct ConvGeometry {
  int H, W, stride, OH, OW;
};

// The engine's own stride rule, ceil((H-1)/(g-1)) (nnue_engine.cpp:710-718) -- not the training stride -- and the
// rejection of an image whose conv map would overrun the engine's grid buffer.
static int engine_conv_geometry(const nnue_engine_model* m, int H, int W, const char* fn, ConvGeometry* out) {
  NNUE_REQUIRE(H > 0 && W > 0, NNUE_E_ARG, "%s: H=%d W=%d must be positive", fn, H, W);
  const int g = m->grid, oc = m->oc, F = m->num_features;
  int stride = g > 1 ? (H - 1 + g - 2) / (g - 1) : (H > 1 ? H : 1);
  if (stride < 1) stride = 1;
  const int OH = (H + 2 - 3) / stride + 1, OW = (W + 2 - 3) / stride + 1;
  NNUE_REQUIRE(OH > 0 && OW > 0 && (long long)OH * OW * oc <= F, NNUE_E_SHAPE,
               "%s: a %dx%d image gives a %dx%d map that overruns the engine's %dx%d grid buffer", fn, H, W, OH, OW, g, g);
  *out = {H, W, stride, OH, OW};
  return NNUE_OK;
}

static void engine_launch_conv(const nnue_engine_model* m, const float* images, int n, const ConvGeometry& g, void* conv, hipStream_t s) {
  const int F = m->num_features;
  hipLaunchKernelGGL(engine_conv_kernel, dim3((F + 255) / 256, n), dim3(256), 0, s, images, m->conv_w, m->conv_b, m->conv_scale, g.H,
                     g.W, g.stride, g.OH, g.OW, m->oc, F, static_cast<int8_t*>(conv));
}

// Where a call's conv bytes come from: float images through engine_conv_kernel, or uint8 frames through the front of
// engine_u8_kernels.hip (u8 == true; the descriptor may still be null, which the entry point refuses).  Either way the bytes
// land in the same scratch and every consumer behind them is the same launch.
struct EngineFrames {
  const float* images;
  const nnue_engine_u8_frames* src;
  bool u8;
  bool given() const { return u8 ? (src && src->data) : images != nullptr; }
};

// The checks of a u8 call that follow the model's and the geometry's (none for float images).
static int engine_check_frames(const char* fn, const nnue_engine_model* m, const EngineFrames& in, int n, const ConvGeometry& g,
                               EngineU8Plan* plan) {
  if (!in.u8) return NNUE_OK;
  return nnue_engine_u8_plan(fn, m, n, g.H, g.W, g.stride, g.OH, g.OW, plan);
}

static void engine_launch_front(const nnue_engine_model* m, const EngineFrames& in, int n, const ConvGeometry& g,
                                const EngineU8Plan& plan, void* conv, hipStream_t s) {
  if (in.u8) nnue_engine_u8_launch(m, in.src, n, g.H, g.W, g.stride, g.OH, g.OW, plan, conv, s);
  else engine_launch_conv(m, in.images, n, g, conv, s);
}

// What every launching entry point checks first: the call's pointers (`pointers`: all of them given), then the stacks argument
// of a selecting call.  Its own argument checks, the model's tensors, a positive count and engine_check_model follow in the
// entry point, in the order the ABI tests pin.
static int engine_check_call(const char* fn, bool pointers, bool select, const nnue_engine_stacks* st, const void* stack_out) {
  NNUE_REQUIRE(pointers, NNUE_E_ARG, "%s: null pointer", fn);
  return select ? engine_check_stacks(st, stack_out, fn) : NNUE_OK;
}

// The kernels' argument block of a checked call: the model's own stack, or the base of the packed stacks (their scales travel
// in the StackSel instead).
static EngineNet engine_net(const nnue_engine_model* m, const nnue_engine_stacks* st) {
  const float threshold = m->threshold;
  const int q1 = (int)(int16_t)m->quantized_one, F = m->num_features, oc = m->oc, L1 = m->l1, L2 = m->l2, L3 = m->l3, C = m->classes;
  if (st)
    return {m->ft_w, m->ft_b, st->l1_w, st->l1_b, st->l2_w, st->l2_b, st->out_w, st->out_b, 0.0f, 1, 0.0f, threshold, q1, F, oc, L1, L2, L3, C};
  return {m->ft_w, m->ft_b, m->l1_w, m->l1_b, m->l2_w, m->l2_b, m->out_w, m->out_b, m->l1_scale, (int)m->l2_scale, m->out_scale,
          threshold, q1, F, oc, L1, L2, L3, C};
}

// Calls fn with the selector of the call: the StackSel of st, or NoStackSel without stacks.
template <class Fn>
static void engine_with_sel(const nnue_engine_stacks* st, const int32_t* stack_in, int32_t* stack_out, Fn fn) {
  if (!st) return fn(NoStackSel{});
  StackSel sel{};
  sel.K = st->count;
  sel.stack_in = stack_in;
  sel.stack_out = stack_out;
  for (int k = 0; k < st->count; ++k) {
    sel.l1_scale[k] = st->scales[3 * k];
    sel.l2_scale[k] = (int)st->scales[3 * k + 1];
    sel.out_scale[k] = st->scales[3 * k + 2];
  }
  fn(sel);
}

// nnue_engine_evaluate_logits (select == false; st, stack_in and stack_out unused) and nnue_engine_evaluate_logits_stacks.
static int engine_evaluate(const char* fn, const nnue_engine_model* m, bool select, const nnue_engine_stacks* st,
                           const EngineFrames& in, int B, int H, int W, const int32_t* stack_in, float* logits, float* density,
                           int32_t* stack_out, void* scratch, int64_t scratch_bytes, nnue_stream_t stream) {
  if (int rc = engine_check_call(fn, m && in.given() && logits && density && scratch, select, st, stack_out)) return rc;
  NNUE_REQUIRE(engine_has_tensors(m, st), NNUE_E_ARG, "%s: model tensor missing", fn);
  NNUE_REQUIRE(B > 0 && H > 0 && W > 0, NNUE_E_ARG, "%s: B=%d H=%d W=%d must be positive", fn, B, H, W);
  if (int rc = engine_check_model(m, st, fn)) return rc;
  if (in.u8)
    if (int rc = nnue_engine_u8_check(fn, m, in.src, B)) return rc;
  const EngineNet net = engine_net(m, st);
  ConvGeometry geo{};
  if (int rc = engine_conv_geometry(m, H, W, fn, &geo)) return rc;
  NNUE_REQUIRE(scratch_bytes >= (int64_t)B * net.F, NNUE_E_SCRATCH, "%s: scratch %lld < %lld bytes", fn, (long long)scratch_bytes,
               (long long)B * net.F);
  NNUE_REQUIRE((long long)B * H * W * 3 < (1ll << 40), NNUE_E_SHAPE, "%s: batch too large", fn);
  const size_t lds = batch_lds(net).bytes;
  NNUE_REQUIRE(lds <= 64 * 1024, NNUE_E_SHAPE, "%s: layer sizes need %zu bytes of LDS", fn, lds);
  EngineU8Plan plan{};
  if (int rc = engine_check_frames(fn, m, in, B, geo, &plan)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint8_t* conv = static_cast<const uint8_t*>(scratch);
  engine_launch_front(m, in, B, geo, plan, scratch, s);
  engine_with_sel(st, stack_in, stack_out, [&](auto sel) {
    hipLaunchKernelGGL((engine_stack_kernel<decltype(sel)>), dim3(B), dim3(256), lds, s, net, conv, logits, density, sel);
  });
  return nnue_launch_status(fn);
}

extern "C" int nnue_engine_evaluate_logits(const nnue_engine_model* m, const float* images, int B, int H, int W, float* logits,
                                           float* density, void* scratch, int64_t scratch_bytes, nnue_stream_t stream) {
  return engine_evaluate("nnue_engine_evaluate_logits", m, false, nullptr, {images, nullptr, false}, B, H, W, nullptr, logits, density,
                         nullptr, scratch, scratch_bytes, stream);
}

extern "C" int nnue_engine_evaluate_logits_stacks(const nnue_engine_model* m, const nnue_engine_stacks* st, const float* images,
                                                  int B, int H, int W, const int32_t* stack_in, float* logits, float* density,
                                                  int32_t* stack_out, void* scratch, int64_t scratch_bytes, nnue_stream_t stream) {
  return engine_evaluate("nnue_engine_evaluate_logits_stacks", m, true, st, {images, nullptr, false}, B, H, W, stack_in, logits,
                         density, stack_out, scratch, scratch_bytes, stream);
}

extern "C" int nnue_engine_evaluate_logits_u8(const nnue_engine_model* m, const nnue_engine_stacks* st,
                                              const nnue_engine_u8_frames* src, int B, int H, int W, const int32_t* stack_in,
                                              float* logits, float* density, int32_t* stack_out, void* scratch,
                                              int64_t scratch_bytes, nnue_stream_t stream) {
  return engine_evaluate("nnue_engine_evaluate_logits_u8", m, st != nullptr, st, {nullptr, src, true}, B, H, W, stack_in, logits,
                         density, stack_out, scratch, scratch_bytes, stream);
}

extern "C" int64_t nnue_engine_stream_state_bytes(const nnue_engine_model* m, int S) {
  if (!m || S <= 0 || m->num_features <= 0 || m->l1 <= 0) return 0;
  return stream_layout(S, m->num_features, m->l1).total;
}

// The state checks of the stream entry points, after the prologue: the buffer's size and the kernel's LDS.
static int engine_check_state(const char* fn, const nnue_engine_model* m, int S, int64_t state_bytes, size_t lds) {
  const int64_t need = nnue_engine_stream_state_bytes(m, S);
  NNUE_REQUIRE(state_bytes >= need, NNUE_E_SCRATCH, "%s: state %lld < %lld bytes", fn, (long long)state_bytes, (long long)need);
  NNUE_REQUIRE(lds <= 64 * 1024, NNUE_E_SHAPE, "%s: layer and feature sizes need %zu bytes of LDS", fn, lds);
  return NNUE_OK;
}

// nnue_engine_stream_step (select == false; st, stack_in and stack_out unused) and nnue_engine_stream_step_stacks.
static int engine_stream_step(const char* fn, const nnue_engine_model* m, bool select, const nnue_engine_stacks* st,
                              const EngineFrames& in, const uint8_t* active, int S, int H, int W, const int32_t* stack_in,
                              void* state, int64_t state_bytes, float* logits, float* density, int32_t* changed,
                              int32_t* stack_out, void* scratch, int64_t scratch_bytes, nnue_stream_t stream) {
  if (int rc = engine_check_call(fn, m && state && logits && density && changed, select, st, stack_out)) return rc;
  const bool images = in.given();
  if (in.u8) NNUE_REQUIRE(images, NNUE_E_ARG, "%s: null pointer", fn);
  NNUE_REQUIRE(images != (active != nullptr), NNUE_E_ARG, "%s: pass exactly one of images and active", fn);
  NNUE_REQUIRE(nnue_aligned16(state), NNUE_E_ARG, "%s: state must be 16-byte aligned", fn);
  NNUE_REQUIRE(engine_has_tensors(m, st), NNUE_E_ARG, "%s: model tensor missing", fn);
  NNUE_REQUIRE(S > 0, NNUE_E_ARG, "%s: S=%d must be positive", fn, S);
  if (int rc = engine_check_model(m, st, fn)) return rc;
  if (in.u8)
    if (int rc = nnue_engine_u8_check(fn, m, in.src, S)) return rc;
  const EngineNet net = engine_net(m, st);
  const size_t lds = stream_lds(net).bytes;
  if (int rc = engine_check_state(fn, m, S, state_bytes, lds)) return rc;
  ConvGeometry geo{};
  EngineU8Plan plan{};
  if (images) {
    if (int rc = engine_conv_geometry(m, H, W, fn, &geo)) return rc;
    NNUE_REQUIRE(scratch, NNUE_E_ARG, "%s: images need scratch", fn);
    NNUE_REQUIRE(scratch_bytes >= (int64_t)S * net.F, NNUE_E_SCRATCH, "%s: scratch %lld < %lld bytes", fn, (long long)scratch_bytes,
                 (long long)S * net.F);
    NNUE_REQUIRE((long long)S * H * W * 3 < (1ll << 40), NNUE_E_SHAPE, "%s: batch too large", fn);
    if (int rc = engine_check_frames(fn, m, in, S, geo, &plan)) return rc;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint8_t* sp = static_cast<uint8_t*>(state);
  if (images) engine_launch_front(m, in, S, geo, plan, scratch, s);
  engine_with_sel(st, stack_in, stack_out, [&](auto sel) {
    if (images)
      hipLaunchKernelGGL((engine_stream_kernel<false, decltype(sel)>), dim3(S), dim3(256), lds, s, net,
                         static_cast<const uint8_t*>(scratch), S, sp, logits, density, changed, sel);
    else
      hipLaunchKernelGGL((engine_stream_kernel<true, decltype(sel)>), dim3(S), dim3(256), lds, s, net, active, S, sp, logits, density,
                         changed, sel);
  });
  return nnue_launch_status(fn);
}

extern "C" int nnue_engine_stream_step(const nnue_engine_model* m, const float* images, const uint8_t* active, int S, int H, int W,
                                       void* state, int64_t state_bytes, float* logits, float* density, int32_t* changed,
                                       void* scratch, int64_t scratch_bytes, nnue_stream_t stream) {
  return engine_stream_step("nnue_engine_stream_step", m, false, nullptr, {images, nullptr, false}, active, S, H, W, nullptr, state,
                            state_bytes, logits, density, changed, nullptr, scratch, scratch_bytes, stream);
}

extern "C" int nnue_engine_stream_step_stacks(const nnue_engine_model* m, const nnue_engine_stacks* st, const float* images,
                                              const uint8_t* active, int S, int H, int W, const int32_t* stack_in, void* state,
                                              int64_t state_bytes, float* logits, float* density, int32_t* changed,
                                              int32_t* stack_out, void* scratch, int64_t scratch_bytes, nnue_stream_t stream) {
  return engine_stream_step("nnue_engine_stream_step_stacks", m, true, st, {images, nullptr, false}, active, S, H, W, stack_in, state,
                            state_bytes, logits, density, changed, stack_out, scratch, scratch_bytes, stream);
}

extern "C" int nnue_engine_stream_step_u8(const nnue_engine_model* m, const nnue_engine_stacks* st, const nnue_engine_u8_frames* src,
                                          int S, int H, int W, const int32_t* stack_in, void* state, int64_t state_bytes,
                                          float* logits, float* density, int32_t* changed, int32_t* stack_out, void* scratch,
                                          int64_t scratch_bytes, nnue_stream_t stream) {
  return engine_stream_step("nnue_engine_stream_step_u8", m, st != nullptr, st, {nullptr, src, true}, nullptr, S, H, W, stack_in,
                            state, state_bytes, logits, density, changed, stack_out, scratch, scratch_bytes, stream);
}

extern "C" int nnue_engine_stream_update(const nnue_engine_model* m, const nnue_engine_stacks* st, const int32_t* added,
                                         const int32_t* added_off, int64_t n_added, const int32_t* removed,
                                         const int32_t* removed_off, int64_t n_removed, int S, int rebuild, const int32_t* stack_in,
                                         void* state, int64_t state_bytes, float* logits, float* density, int32_t* changed,
                                         int32_t* stack_out, nnue_stream_t stream) {
  const char* fn = "nnue_engine_stream_update";
  if (int rc = engine_check_call(fn, m && state && logits && density && changed, st != nullptr, st, stack_out)) return rc;
  NNUE_REQUIRE(n_added >= 0 && n_removed >= 0, NNUE_E_ARG, "%s: n_added=%lld n_removed=%lld must not be negative", fn,
               (long long)n_added, (long long)n_removed);
  NNUE_REQUIRE((n_added == 0 || (added && added_off)) && (n_removed == 0 || (removed && removed_off)), NNUE_E_ARG,
               "%s: a list with ids needs its id and offset pointers", fn);
  NNUE_REQUIRE(nnue_aligned16(state), NNUE_E_ARG, "%s: state must be 16-byte aligned", fn);
  NNUE_REQUIRE(engine_has_tensors(m, st), NNUE_E_ARG, "%s: model tensor missing", fn);
  NNUE_REQUIRE(S > 0, NNUE_E_ARG, "%s: S=%d must be positive", fn, S);
  if (int rc = engine_check_model(m, st, fn)) return rc;
  const EngineNet net = engine_net(m, st);
  const size_t lds = update_lds(net).bytes;
  if (int rc = engine_check_state(fn, m, S, state_bytes, lds)) return rc;
  // the offsets are int32, so ids beyond 2^31 - 1 of a buffer are out of every range's reach
  const int na = (int)(n_added > INT32_MAX ? INT32_MAX : n_added), nr = (int)(n_removed > INT32_MAX ? INT32_MAX : n_removed);
  hipStream_t s = static_cast<hipStream_t>(stream);
  engine_with_sel(st, stack_in, stack_out, [&](auto sel) {
    hipLaunchKernelGGL((engine_stream_update_kernel<decltype(sel)>), dim3(S), dim3(256), lds, s, net, added, added_off, na, removed,
                       removed_off, nr, (int)(rebuild != 0), S, static_cast<uint8_t*>(state), logits, density, changed, sel);
  });
  return nnue_launch_status(fn);
}

extern "C" int nnue_engine_stream_step_u8_regions(const nnue_engine_model* m, const nnue_engine_stacks* st,
                                                  const nnue_engine_u8_frames* src, int S, int H, int W, const int32_t* rects,
                                                  const int32_t* rect_off, int64_t n_rects, const int32_t* stack_in, void* state,
                                                  int64_t state_bytes, float* logits, float* density, int32_t* changed,
                                                  int32_t* stack_out, nnue_stream_t stream) {
  const char* fn = "nnue_engine_stream_step_u8_regions";
  if (int rc = engine_check_call(fn, m && state && logits && density && changed, st != nullptr, st, stack_out)) return rc;
  NNUE_REQUIRE(src && src->data, NNUE_E_ARG, "%s: null pointer", fn);
  NNUE_REQUIRE(n_rects >= 0, NNUE_E_ARG, "%s: n_rects=%lld must not be negative", fn, (long long)n_rects);
  NNUE_REQUIRE(n_rects == 0 || (rects && rect_off), NNUE_E_ARG, "%s: a list with rectangles needs its rectangle and offset pointers", fn);
  NNUE_REQUIRE(nnue_aligned16(state), NNUE_E_ARG, "%s: state must be 16-byte aligned", fn);
  NNUE_REQUIRE(engine_has_tensors(m, st), NNUE_E_ARG, "%s: model tensor missing", fn);
  NNUE_REQUIRE(S > 0, NNUE_E_ARG, "%s: S=%d must be positive", fn, S);
  if (int rc = engine_check_model(m, st, fn)) return rc;
  if (int rc = nnue_engine_u8_check(fn, m, src, S)) return rc;
  NNUE_REQUIRE(src->layout == 1, NNUE_E_ARG,
               "%s: layout %d: only hwc (1) is accepted, under chw a pixel rectangle does not map to neighbouring taps", fn, src->layout);
  const EngineNet net = engine_net(m, st);
  const size_t lds = regions_lds_bytes(net);
  if (int rc = engine_check_state(fn, m, S, state_bytes, lds)) return rc;
  ConvGeometry geo{};
  if (int rc = engine_conv_geometry(m, H, W, fn, &geo)) return rc;
  NNUE_REQUIRE(3ll * H * W < (1ll << 31), NNUE_E_SHAPE, "%s: a %dx%d frame holds 2^31 bytes or more", fn, H, W);
  NNUE_REQUIRE((long long)S * H * W * 3 < (1ll << 40), NNUE_E_SHAPE, "%s: batch too large", fn);
  RegionFront a{};
  a.data = src->data;
  a.indices = src->indices;
  a.count = src->count;
  a.w = m->conv_w;
  a.bias = m->conv_b;
  a.rects = rects;
  a.rect_off = rect_off;
  // the offsets are int32, so rectangles beyond 2^31 - 1 of a buffer are out of every range's reach
  a.n_rects = (int)(n_rects > INT32_MAX ? INT32_MAX : n_rects);
  a.mean0 = src->mean255[0], a.mean1 = src->mean255[1], a.mean2 = src->mean255[2];
  a.inv0 = src->inv_std255[0], a.inv1 = src->inv_std255[1], a.inv2 = src->inv_std255[2];
  a.scale = m->conv_scale;
  a.H = H, a.W = W, a.stride = geo.stride, a.OH = geo.OH, a.OW = geo.OW;
  hipStream_t s = static_cast<hipStream_t>(stream);
  engine_with_sel(st, stack_in, stack_out, [&](auto sel) {
    hipLaunchKernelGGL((engine_stream_regions_kernel<decltype(sel)>), dim3(S), dim3(256), lds, s, net, a, S,
                       static_cast<uint8_t*>(state), logits, density, changed, sel);
  });
  return nnue_launch_status(fn);
}

// ---- the matrix form's entry points ---------------------------------------------------------------------------------
// What the matrix form itself can run: the plane count, the tail's LDS, and F small enough that no int32 sum can overflow.
static bool engine_matrix_shape_ok(const nnue_engine_model* m, int planes) {
  if (planes != 1 && planes != 2) return false;
  if (m->num_features <= 0 || m->num_features >= kMxMaxFeatures) return false;
  if (m->l1 < 2 || m->l1 > 256 * kMaxColsPerThread || m->l2 < 1 || m->l3 < 1) return false;
  return batch_lds(engine_net(m, nullptr)).bytes <= 64 * 1024;
}

extern "C" int nnue_engine_matrix_supported(const nnue_engine_model* m, int B, int planes) {
  if (!m || B <= 0) return 0;
  return engine_matrix_shape_ok(m, planes) ? 1 : 0;
}

extern "C" int64_t nnue_engine_table_planes_bytes(const nnue_engine_model* m, int planes) {
  if (!m || (planes != 1 && planes != 2) || m->num_features <= 0 || m->l1 <= 0) return 0;
  return planes * matrix_layout(1, m->num_features, m->l1).plane_bytes;
}

extern "C" int64_t nnue_engine_matrix_scratch(const nnue_engine_model* m, int B, int planes) {
  if (!m || B <= 0 || (planes != 1 && planes != 2) || m->num_features <= 0 || m->l1 <= 0) return 0;
  return matrix_layout(B, m->num_features, m->l1).total;
}

extern "C" int nnue_engine_pack_table(const nnue_engine_model* m, int planes, void* table_planes, int64_t bytes, int32_t* misfit,
                                      nnue_stream_t stream) {
  const char* fn = "nnue_engine_pack_table";
  NNUE_REQUIRE(m && table_planes && misfit, NNUE_E_ARG, "%s: null pointer", fn);
  NNUE_REQUIRE(m->ft_w, NNUE_E_ARG, "%s: model tensor missing", fn);
  NNUE_REQUIRE(nnue_aligned16(table_planes) && (reinterpret_cast<uintptr_t>(misfit) & 3u) == 0, NNUE_E_ARG,
               "%s: table_planes must be 16-byte aligned, misfit 4-byte aligned", fn);
  NNUE_REQUIRE(m->num_features > 0 && m->l1 >= 2 && m->l1 <= 256 * kMaxColsPerThread, NNUE_E_SHAPE, "%s: F=%d L1=%d (2..%d)", fn,
               m->num_features, m->l1, 256 * kMaxColsPerThread);
  NNUE_REQUIRE(planes == 1 || planes == 2, NNUE_E_SHAPE, "%s: planes=%d (1 or 2)", fn, planes);
  NNUE_REQUIRE(m->num_features < kMxMaxFeatures, NNUE_E_SHAPE, "%s: num_features %d >= 2^24", fn, m->num_features);
  const MatrixLayout lay = matrix_layout(1, m->num_features, m->l1);
  NNUE_REQUIRE(bytes >= planes * lay.plane_bytes, NNUE_E_SCRATCH, "%s: table_planes %lld < %lld bytes", fn, (long long)bytes,
               (long long)(planes * lay.plane_bytes));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t chunks = lay.plane_bytes / 16;
  const dim3 grid((unsigned)((chunks + 255) / 256));
  int8_t* dst = static_cast<int8_t*>(table_planes);
  if (planes == 1)
    hipLaunchKernelGGL((engine_pack_table_kernel<1>), grid, dim3(256), 0, s, m->ft_w, m->num_features, m->l1, (int)lay.npad, chunks,
                       lay.plane_bytes, dst, misfit);
  else
    hipLaunchKernelGGL((engine_pack_table_kernel<2>), grid, dim3(256), 0, s, m->ft_w, m->num_features, m->l1, (int)lay.npad, chunks,
                       lay.plane_bytes, dst, misfit);
  return nnue_launch_status(fn);
}

// Slabs along K: enough workgroups for two per CU where the (B, L1) tile grid alone leaves CUs idle, every slab at least
// kMxMinTilesPerSlab K tiles deep.  NNUE_ENGINE_MATRIX_KSPLIT (developer knob, read per call; 0 = this policy) forces the count.
static int engine_matrix_slabs(int tiles, int ktiles) {
  const char* e = std::getenv("NNUE_ENGINE_MATRIX_KSPLIT");
  int slabs = e && *e ? std::atoi(e) : 0;
  if (slabs <= 0) {
    slabs = tiles >= 256 ? 1 : (512 + tiles - 1) / tiles;
    const int deep = ktiles / kMxMinTilesPerSlab;
    if (slabs > deep) slabs = deep;
  }
  if (slabs > ktiles) slabs = ktiles;
  return slabs < 1 ? 1 : slabs;
}

template <int kPlanes, bool kFeatures>
static void engine_launch_product(const nnue_engine_model* m, const uint8_t* src, int B, const MatrixLayout& lay, const int8_t* planes,
                                  int32_t* sums, hipStream_t s) {
  const int F = m->num_features, L1 = m->l1;
  const int tiles_n = (int)(lay.npad / kMxBN), tiles_m = (B + kMxBM - 1) / kMxBM, ktiles = (int)(lay.kpad / kMxBK);
  const int want = engine_matrix_slabs(tiles_n * tiles_m, ktiles);
  const int per = (ktiles + want - 1) / want, slabs = (ktiles + per - 1) / per;
  if (slabs > 1) nnue_zero_floats(reinterpret_cast<float*>(sums), (size_t)B * L1, s);  // zero bits either way
  const int aligned = F % 16 == 0 && nnue_aligned16(src);
  hipLaunchKernelGGL((engine_matrix_product_kernel<kPlanes, kFeatures>), dim3(tiles_n, tiles_m, slabs), dim3(256), 0, s, src,
                     m->threshold, m->oc, B, F, L1, (int)lay.npad, lay.plane_bytes, planes, ktiles, per, aligned, slabs > 1 ? 1 : 0,
                     sums);
}

// The product and the tail over one source of bytes: the conv map (kFeatures == false) or the caller's feature map.
template <bool kFeatures, class Sel>
static void engine_launch_matrix(const nnue_engine_model* m, const EngineNet& net, int planes, const uint8_t* src, int B,
                                 const MatrixLayout& lay, const int8_t* tp, int32_t* sums, float* logits, float* density, Sel sel,
                                 hipStream_t s) {
  if (planes == 1) engine_launch_product<1, kFeatures>(m, src, B, lay, tp, sums, s);
  else engine_launch_product<2, kFeatures>(m, src, B, lay, tp, sums, s);
  hipLaunchKernelGGL((engine_matrix_tail_kernel<kFeatures, Sel>), dim3(B), dim3(256), batch_lds(net).bytes, s, net, src, sums, logits,
                     density, sel);
}

// nnue_engine_evaluate_logits_matrix and its u8 twin.
static int engine_evaluate_matrix(const char* fn, const nnue_engine_model* m, const nnue_engine_stacks* st, const void* table_planes,
                                  int planes, const EngineFrames& in, const uint8_t* active, int B, int H, int W,
                                  const int32_t* stack_in, float* logits, float* density, int32_t* stack_out, void* scratch,
                                  int64_t scratch_bytes, nnue_stream_t stream) {
  const bool images = in.given();
  if (int rc = engine_check_call(fn, m && table_planes && logits && density && scratch, st != nullptr, st, stack_out)) return rc;
  if (in.u8) NNUE_REQUIRE(images, NNUE_E_ARG, "%s: null pointer", fn);
  NNUE_REQUIRE(images != (active != nullptr), NNUE_E_ARG, "%s: pass exactly one of images and active", fn);
  NNUE_REQUIRE(nnue_aligned16(table_planes), NNUE_E_ARG, "%s: table_planes must be 16-byte aligned", fn);
  NNUE_REQUIRE(engine_has_tensors(m, st), NNUE_E_ARG, "%s: model tensor missing", fn);
  NNUE_REQUIRE(B > 0, NNUE_E_ARG, "%s: B=%d must be positive", fn, B);
  if (int rc = engine_check_model(m, st, fn)) return rc;
  if (in.u8)
    if (int rc = nnue_engine_u8_check(fn, m, in.src, B)) return rc;
  const EngineNet net = engine_net(m, st);
  NNUE_REQUIRE(planes == 1 || planes == 2, NNUE_E_SHAPE, "%s: planes=%d (1 or 2)", fn, planes);
  NNUE_REQUIRE(net.F < kMxMaxFeatures, NNUE_E_SHAPE, "%s: num_features %d >= 2^24 (an int32 sum could overflow)", fn, net.F);
  NNUE_REQUIRE(batch_lds(net).bytes <= 64 * 1024, NNUE_E_SHAPE, "%s: layer sizes need %zu bytes of LDS", fn, batch_lds(net).bytes);
  ConvGeometry geo{};
  if (images) {
    if (int rc = engine_conv_geometry(m, H, W, fn, &geo)) return rc;
    NNUE_REQUIRE((long long)B * H * W * 3 < (1ll << 40), NNUE_E_SHAPE, "%s: batch too large", fn);
  }
  const MatrixLayout lay = matrix_layout(B, net.F, net.L1);
  NNUE_REQUIRE(scratch_bytes >= lay.total, NNUE_E_SCRATCH, "%s: scratch %lld < %lld bytes", fn, (long long)scratch_bytes,
               (long long)lay.total);
  NNUE_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 3u) == 0, NNUE_E_ARG, "%s: scratch must be 4-byte aligned", fn);
  EngineU8Plan plan{};
  if (images)
    if (int rc = engine_check_frames(fn, m, in, B, geo, &plan)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint8_t* conv = static_cast<uint8_t*>(scratch);
  int32_t* sums = reinterpret_cast<int32_t*>(conv + lay.sums);
  const int8_t* tp = static_cast<const int8_t*>(table_planes);
  if (images) engine_launch_front(m, in, B, geo, plan, conv, s);
  engine_with_sel(st, stack_in, stack_out, [&](auto sel) {
    if (images) engine_launch_matrix<false>(m, net, planes, conv, B, lay, tp, sums, logits, density, sel, s);
    else engine_launch_matrix<true>(m, net, planes, active, B, lay, tp, sums, logits, density, sel, s);
  });
  return nnue_launch_status(fn);
}

extern "C" int nnue_engine_evaluate_logits_matrix(const nnue_engine_model* m, const nnue_engine_stacks* st, const void* table_planes,
                                                  int planes, const float* images, const uint8_t* active, int B, int H, int W,
                                                  const int32_t* stack_in, float* logits, float* density, int32_t* stack_out,
                                                  void* scratch, int64_t scratch_bytes, nnue_stream_t stream) {
  return engine_evaluate_matrix("nnue_engine_evaluate_logits_matrix", m, st, table_planes, planes, {images, nullptr, false}, active,
                                B, H, W, stack_in, logits, density, stack_out, scratch, scratch_bytes, stream);
}

extern "C" int nnue_engine_evaluate_logits_matrix_u8(const nnue_engine_model* m, const nnue_engine_stacks* st, const void* table_planes,
                                                     int planes, const nnue_engine_u8_frames* src, int B, int H, int W,
                                                     const int32_t* stack_in, float* logits, float* density, int32_t* stack_out,
                                                     void* scratch, int64_t scratch_bytes, nnue_stream_t stream) {
  return engine_evaluate_matrix("nnue_engine_evaluate_logits_matrix_u8", m, st, table_planes, planes, {nullptr, src, true}, nullptr,
                                B, H, W, stack_in, logits, density, stack_out, scratch, scratch_bytes, stream);
}
