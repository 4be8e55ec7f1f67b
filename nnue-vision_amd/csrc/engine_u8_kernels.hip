// The engine's conv front from uint8 frames: ConvLayer::forward (engine/src/nnue_engine.cpp:48-158) on the flat float buffer
// x[0 .. 3HW) that a frame's bytes u[0 .. 3HW) stand for, without that buffer ever existing:
//   layout 0 (chw)  x[i] = norm(u[(i mod HW) * 3 + i div HW], i div HW) -- the memory nnue_load_batch(augment = 0) writes for the
//                   image, a CHW tensor handed to the engine flat (evaluate.py:150-161), which the engine indexes HWC;
//   layout 1 (hwc)  x[i] = norm(u[i], i mod 3) -- the frame is what the engine's indexing means;
//   norm(v, c) = ((float)v - mean255[c]) * inv_std255[c]   (input_kernels.hip, load_batch_kernel; data/datasets.py:366-369).
// The engine's first act on x is q = (int32)(x[i] * conv_scale).  A byte has 256 values and a channel three, so q is a table of
// 768 int32, formed once per workgroup by exactly that expression (three separately rounded float operations, then the
// conversion), and everything behind it is integer arithmetic: the bits are those of engine_conv_kernel on the float batch.
//
// One 256-thread workgroup = (image, band of output rows).  It stages q of the flat input rows the band's taps reach into LDS,
// one zero element-triple of padding on either side and zero rows outside the image, so the 27-tap loop has no bounds test;
// at stride >= 3 those are three rows per output row, the rows between them are never read.  A thread keeps the 27 weights of
// its channel in registers and walks the band's positions; all channels of a position read the same LDS words (broadcast).
// The band's bytes are collected in LDS and leave in aligned 16-byte stores; the bytes of the image's F behind the map are
// zero-filled by the image's bands together.
#include "engine_u8.h"

#include <cmath>

namespace {

constexpr int kU8LdsBudget = 24 * 1024;     // the plan's target per workgroup: six or more workgroups share a CU's 160 KB
constexpr int kU8LdsMax = 64 * 1024;
constexpr int kU8MinWorkgroups = 1024;      // bands are halved while a launch would have fewer (256 CUs)

struct U8Front {
  const uint8_t* __restrict__ data;
  const int64_t* __restrict__ indices;
  int64_t count;
  const int8_t* __restrict__ w;
  const int32_t* __restrict__ bias;
  int8_t* __restrict__ conv;
  float mean0, mean1, mean2, inv0, inv1, inv2, scale;
  int layout, H, W, stride, OH, OW, oc, F;
  int rows, bands, row_len, oc_log2, rows_words;  // rows_words: int32 words of the staged rows, a multiple of 4
};

// Bytes [0, n) behind the global address `first`, from src (LDS, laid out so that src[first & 15] is the first byte) or zeros
// (src == nullptr): chunks [j0, j1) of the 16-byte grid over [first - (first & 15), ...), whole chunks as one store, the
// partial ones at either end byte by byte.  Nothing outside [first, first + n) is written.
__device__ __forceinline__ void u8_store_span(uintptr_t first, int64_t n, const uint8_t* src, int64_t j0, int64_t j1) {
  const int64_t mis = (int64_t)(first & 15), end = mis + n;
  const uintptr_t base = first - (uintptr_t)mis;
  for (int64_t j = j0 + threadIdx.x; j < j1; j += 256) {
    const int64_t lo = 16 * j;
    if (lo >= mis && lo + 16 <= end) {
      *reinterpret_cast<uint4*>(base + lo) = src ? *reinterpret_cast<const uint4*>(src + lo) : make_uint4(0, 0, 0, 0);
    } else {
      for (int64_t k = lo < mis ? mis : lo; k < lo + 16 && k < end; ++k) *reinterpret_cast<uint8_t*>(base + k) = src ? src[k] : (uint8_t)0;
    }
  }
}

// grid (n * bands); dynamic LDS: table [768] i32 | rows [slots][row_len] i32 (rows_words) | band bytes [rows * OW * oc + 16]
__global__ __launch_bounds__(256) void engine_conv_u8_kernel(U8Front a) {
  extern __shared__ __attribute__((aligned(16))) int32_t u8_lds[];
  int32_t* tab = u8_lds;
  int32_t* rows = u8_lds + kU8Table;
  uint8_t* out_s = reinterpret_cast<uint8_t*>(rows + a.rows_words);
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.bands, band = blockIdx.x - b * a.bands;
  const int H = a.H, W = a.W, stride = a.stride, OW = a.OW, oc = a.oc, F = a.F, row_len = a.row_len;
  const int HW = H * W, W3 = 3 * W;  // 3 * H * W < 2^31 (checked on the host)

  tab[tid] = u8_quantise(tid, a.mean0, a.inv0, a.scale);
  tab[256 + tid] = u8_quantise(tid, a.mean1, a.inv1, a.scale);
  tab[512 + tid] = u8_quantise(tid, a.mean2, a.inv2, a.scale);

  int8_t* __restrict__ image_out = a.conv + (size_t)b * F;
  const int map_bytes = a.OH * OW * oc;
  if (map_bytes < F) {  // the zero-filled rest of the grid buffer (nnue_engine.cpp:679-681), an equal share per band
    const uintptr_t first = reinterpret_cast<uintptr_t>(image_out + map_bytes);
    const int64_t chunks = ((int64_t)(first & 15) + (F - map_bytes) + 15) >> 4;
    const int64_t per = (chunks + a.bands - 1) / a.bands, j0 = band * per;
    u8_store_span(first, F - map_bytes, nullptr, j0, j0 + per < chunks ? j0 + per : chunks);
  }

  int64_t idx = b;  // without indices: frame b, and count >= n (checked on the host)
  if (a.indices) {
    idx = a.indices[b];
    idx = idx < 0 ? 0 : (idx >= a.count ? a.count - 1 : idx);  // as load_batch_kernel
  }
  const uint8_t* __restrict__ img = a.data + (size_t)idx * 3 * HW;

  const int oh0 = band * a.rows;
  const int R = a.OH - oh0 < a.rows ? a.OH - oh0 : a.rows;
  const bool sparse = stride >= 3;  // three staged rows per output row; below that the band's rows are one contiguous run
  const int slots = sparse ? 3 * R : (R - 1) * stride + 3;
  __syncthreads();  // the table
  for (int slot = 0; slot < slots; ++slot) {
    const int ih = sparse ? (oh0 + slot / 3) * stride + slot % 3 - 1 : oh0 * stride - 1 + slot;
    const bool inside = ih >= 0 && ih < H;
    const int i0 = inside ? ih * W3 : 0;  // the row's first element of x
    const int p0 = i0 / HW, r0 = i0 - p0 * HW;
    int32_t* row = rows + slot * row_len;
    for (int k = tid; k < row_len; k += 256) {
      const int j = k - 3;  // element of the flat row; the first and last three are the padding
      int32_t q = 0;
      if (inside && j >= 0 && j < W3) {
        int byte, ch;
        if (a.layout == 1) {
          byte = i0 + j;  // < 3HW
          ch = j % 3;     // i0 is a multiple of 3
        } else {
          int pos = r0 + j;  // i0 + j < 3HW: at most two plane boundaries lie ahead of r0
          ch = p0;
          if (pos >= HW) pos -= HW, ++ch;
          if (pos >= HW) pos -= HW, ++ch;
          byte = pos * 3 + ch;  // pos < HW, ch <= 2: < 3HW
        }
        q = tab[ch * 256 + img[byte]];
      }
      row[k] = q;
    }
  }
  __syncthreads();

  const uintptr_t first = reinterpret_cast<uintptr_t>(image_out + (size_t)oh0 * OW * oc);
  const int mis = (int)(first & 15);
  const int lanes = 1 << a.oc_log2, npos = R * OW, step = 256 >> a.oc_log2;
  const int32_t div = (int32_t)a.scale;
  for (int c = tid & (lanes - 1); c < oc; c += lanes) {
    int32_t wr[27];
#pragma unroll
    for (int t = 0; t < 27; ++t) wr[t] = (int32_t)a.w[c * 27 + t];  // [oc][kh][kw][ic], the file's bytes
    const int32_t bias = a.bias[c];
    for (int pos = tid >> a.oc_log2; pos < npos; pos += step) {
      const int r = pos / OW, ow = pos - r * OW;
      const int32_t* tap = rows + (sparse ? 3 * r : r * stride) * row_len + ow * stride * 3;
      int32_t acc = bias;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc += tap[kh * row_len + t] * wr[kh * 9 + t];
      int32_t q = acc / div;  // truncating division, as the engine
      q = q < -127 ? -127 : (q > 127 ? 127 : q);
      out_s[mis + pos * oc + c] = (uint8_t)(int8_t)q;
    }
  }
  __syncthreads();
  const int n = npos * oc;
  u8_store_span(first, n, out_s, 0, (mis + n + 15) >> 4);
}

int u8_slots(int rows, int stride) { return stride >= 3 ? 3 * rows : (rows - 1) * stride + 3; }

void u8_fill_plan(EngineU8Plan& p, int rows, int stride, int OH, int OW, int oc) {
  p.rows = rows;
  p.bands = (OH + rows - 1) / rows;
  p.slots = u8_slots(rows, stride);
  p.rows_bytes = nnue_round_up((int64_t)p.slots * p.row_len * 4, 16);
  p.lds_bytes = kU8Table * 4 + p.rows_bytes + nnue_round_up((int64_t)rows * OW * oc + 16, 16);
}

}  // namespace

int nnue_engine_u8_check(const char* fn, const nnue_engine_model* m, const nnue_engine_u8_frames* src, int n) {
  NNUE_REQUIRE(src->layout == 0 || src->layout == 1, NNUE_E_ARG, "%s: layout %d (0 chw, 1 hwc)", fn, src->layout);
  NNUE_REQUIRE(src->count >= 1, NNUE_E_ARG, "%s: count=%lld must be positive", fn, (long long)src->count);
  NNUE_REQUIRE(src->indices || src->count >= n, NNUE_E_ARG, "%s: %lld frames for %d without indices", fn, (long long)src->count, n);
  for (int c = 0; c < 3; ++c) {
    const float mean = src->mean255[c], inv = src->inv_std255[c];
    NNUE_REQUIRE(std::isfinite(mean) && std::isfinite(inv) && inv > 0.0f, NNUE_E_ARG,
                 "%s: channel %d: mean255 %g, inv_std255 %g (finite, std > 0)", fn, c, (double)mean, (double)inv);
    for (int v = 0; v <= 255; v += 255) {  // the table is monotone in v: its extremes are its ends
      const float x = ((float)v - mean) * inv;
      const float q = x * m->conv_scale;
      NNUE_REQUIRE(std::isfinite(q) && std::fabs(q) < 2147483648.0f, NNUE_E_ARG,
                   "%s: channel %d: byte %d times conv_scale %g is %g, outside int32", fn, c, v, (double)m->conv_scale, (double)q);
    }
  }
  return NNUE_OK;
}

int nnue_engine_u8_plan(const char* fn, const nnue_engine_model* m, int n, int H, int W, int stride, int OH, int OW, EngineU8Plan* plan) {
  NNUE_REQUIRE(3ll * H * W < (1ll << 31), NNUE_E_SHAPE, "%s: a %dx%d frame holds 2^31 bytes or more", fn, H, W);
  EngineU8Plan p{};
  const int oc = m->oc;
  p.row_len = 3 * (W + 2);
  for (p.oc_log2 = 0; p.oc_log2 < 8 && (1 << p.oc_log2) < oc; ++p.oc_log2) {}
  u8_fill_plan(p, 1, stride, OH, OW, oc);
  NNUE_REQUIRE(p.lds_bytes <= kU8LdsMax, NNUE_E_SHAPE, "%s: one output row of a %d-wide frame with %d channels needs %lld bytes of LDS",
               fn, W, oc, (long long)p.lds_bytes);
  int rows = 1;
  for (EngineU8Plan q = p; rows < OH; ++rows) {
    u8_fill_plan(q, rows + 1, stride, OH, OW, oc);
    if (q.lds_bytes > kU8LdsBudget) break;
  }
  while (rows > 1 && (int64_t)n * ((OH + rows - 1) / rows) < kU8MinWorkgroups) rows = (rows + 1) / 2;
  u8_fill_plan(p, rows, stride, OH, OW, oc);
  NNUE_REQUIRE((int64_t)n * p.bands < (1ll << 31), NNUE_E_SHAPE, "%s: batch too large", fn);
  *plan = p;
  return NNUE_OK;
}

void nnue_engine_u8_launch(const nnue_engine_model* m, const nnue_engine_u8_frames* src, int n, int H, int W, int stride, int OH,
                           int OW, const EngineU8Plan& plan, void* conv, hipStream_t s) {
  U8Front a{};
  a.data = src->data;
  a.indices = src->indices;
  a.count = src->count;
  a.w = m->conv_w;
  a.bias = m->conv_b;
  a.conv = static_cast<int8_t*>(conv);
  a.mean0 = src->mean255[0], a.mean1 = src->mean255[1], a.mean2 = src->mean255[2];
  a.inv0 = src->inv_std255[0], a.inv1 = src->inv_std255[1], a.inv2 = src->inv_std255[2];
  a.scale = m->conv_scale;
  a.layout = src->layout;
  a.H = H, a.W = W, a.stride = stride, a.OH = OH, a.OW = OW, a.oc = m->oc, a.F = m->num_features;
  a.rows = plan.rows, a.bands = plan.bands, a.row_len = plan.row_len, a.oc_log2 = plan.oc_log2;
  a.rows_words = (int)(plan.rows_bytes / 4);
  hipLaunchKernelGGL(engine_conv_u8_kernel, dim3((unsigned)(n * plan.bands)), dim3(256), (size_t)plan.lds_bytes, s, a);
}
