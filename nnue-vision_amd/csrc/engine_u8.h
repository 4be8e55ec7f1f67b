// The uint8 front of the engine calls (engine_u8_kernels.hip): ConvLayer::forward (nnue_engine.cpp:48-158) straight from uint8
// frames, into the conv bytes the float front (engine_conv_kernel) writes.  The entry points in engine_kernels.hip check a call
// with nnue_engine_u8_check and nnue_engine_u8_plan before anything is launched, then launch the front and the float twin's
// consumers.
#pragma once
#include "common.h"

// The 768 possible q = (int32)(x * conv_scale) of a byte in a channel, one table per workgroup: [channel][byte], int32 entries.
// Shared by the whole-frame front and the region step of engine_kernels.hip, so that both form every entry by one expression.
constexpr int kU8Table = 3 * 256;

__device__ __forceinline__ int32_t u8_quantise(int v, float mean255, float inv_std255, float scale) {
  const float x = ((float)v - mean255) * inv_std255;  // the float load_batch_kernel stores
  return (int32_t)(x * scale);                        // what engine_conv_kernel makes of it
}

// How one launch splits the work: a workgroup = (image, band of `rows` output rows).
struct EngineU8Plan {
  int rows, bands, slots, row_len, oc_log2;
  int64_t rows_bytes, lds_bytes;
};

// The descriptor's own fields (layout, constants, count against n frames) and the int32 range of every table entry under the
// model's conv_scale.  NNUE_E_ARG with a message naming fn.  The caller has checked src, src->data and the model's scales.
int nnue_engine_u8_check(const char* fn, const nnue_engine_model* m, const nnue_engine_u8_frames* src, int n);

// The band height for n frames of H x W (stride, OH, OW: the engine's geometry).  NNUE_E_SHAPE where one output row's source
// rows do not fit a workgroup's LDS, or a frame holds 2^31 bytes or more.
int nnue_engine_u8_plan(const char* fn, const nnue_engine_model* m, int n, int H, int W, int stride, int OH, int OW, EngineU8Plan* plan);

void nnue_engine_u8_launch(const nnue_engine_model* m, const nnue_engine_u8_frames* src, int n, int H, int W, int stride, int OH,
                           int OW, const EngineU8Plan& plan, void* conv, hipStream_t s);
