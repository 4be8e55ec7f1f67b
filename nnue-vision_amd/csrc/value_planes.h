// The table rows the value gradient of the batch-512 STE ride reads, as pre-split bf16 planes: the layout of the plane buffer
// and the writer that rides in the conv launch (feature_kernels.hip) -- one definition for the writer and for the reader
// (gemm_tile_val_planes, ftm_kernels.hip).  Include after forward_planes.h, inside the including file's anonymous namespace.
//
// d_val = (d_out W^T) . A contracts along L1, so a chunk here is 8 consecutive j (L1 index) of ONE table row -- the forward's
// planes (8 consecutive table rows of one column) cannot serve.  What the reader would do per load is done by the writer:
//   column n of value tile tile_n (ValSteEpi::prow: channel n / 8, grid position 8 tile_n + n % 8 clamped to G - 1) reads table
//   row val_plane_row(...), rows >= F - 1 clamped to F - 1 (nnue.py:701); j >= L1 (a ragged last K tile) holds zeros.
// Layout: one block of kValPlaneBlock bytes per (column tile tile_n of 64, K tile kt of 128), block index tile_n * ktiles + kt;
// inside a block plane p (0 hi, 1 mid, 2 lo; hi + mid + lo == w exactly, bf16_split.h) starts at p * kValPlaneBytes and is in
// FRAGMENT order: the 1 KB at val_plane_frag(w, kb) holds, at lane * 16 with lane = 16 q + r, the 8 bf16
//   j = 128 kt + 32 kb + 8 q .. + 7 of column 16 w + r
// i.e. exactly what lane (r, q) of wave w feeds v_mfma_f32_16x16x32_bf16 as the B operand of 32-k block kb: one wave-level
// 16-byte load reads 1 KB of contiguous memory.
#pragma once

constexpr int kValPlaneBytes = 64 * kBfK * 2;       // one plane of a block: 16 KB
constexpr int kValPlaneBlock = 3 * kValPlaneBytes;  // 48 KB

__device__ __forceinline__ int val_plane_frag(int w, int kb) { return (w * (kBfK / 32) + kb) * 1024; }

// table row of tile-local column n of value tile tile_n (G grid positions, 8 channels, F table rows)
__device__ __forceinline__ int val_plane_row(int tile_n, int n, int G, int F) {
  const int hw = tile_n * 8 + (n & 7);
  const int p = (n >> 3) * G + (hw < G ? hw : G - 1);
  return p < F - 1 ? p : F - 1;
}

struct ValPlaneArgs {
  const float* __restrict__ weight;    // table [F][L1]
  unsigned char* __restrict__ planes;  // tiles_n * ktiles blocks
  unsigned w_bytes;                    // the table's window: F * L1 * 4
  int L1, F, G, ktiles, parts;         // parts: workgroups per block (256 / threads of the launch)
};

// One workgroup's share of one block.  `rider` in [0, blocks * parts); blockDim.x in {64, 128, 256}.  A thread of the 256 that
// write a block owns four chunks per plane, 256 chunks apart, so that a wave's stores are 1 KB runs and its loads whole 128-byte
// lines of 16 table rows.  Every load goes through the table's window (a chunk at j >= L1 gets an offset outside it: zeros).
// No LDS, no barrier.
__device__ __forceinline__ void value_planes_write(const ValPlaneArgs& a, int rider) {
  const int block = rider / a.parts, part = rider - block * a.parts;
  const int tile_n = block / a.ktiles, kt = block - tile_n * a.ktiles;
  const int vt = part * (int)blockDim.x + (int)threadIdx.x;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.weight), 0, a.w_bytes, 0x00020000);
  u32x4 raw[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ci = vt + 256 * i, lane = ci & 63, g = ci >> 6;  // g = 4 w + kb
    const int n = (g >> 2) * 16 + (lane & 15), j = kt * kBfK + (g & 3) * 32 + (lane >> 4) * 8;
    const bool in = j < a.L1;  // L1 % 8 == 0: a chunk is inside or outside as a whole
    const int off = (val_plane_row(tile_n, n, a.G, a.F) * a.L1 + j) * 4;
    raw[i][0] = __builtin_amdgcn_raw_buffer_load_b128(rs, in ? off : 0x7ffffff0, 0, 0);
    raw[i][1] = __builtin_amdgcn_raw_buffer_load_b128(rs, in ? off + 16 : 0x7ffffff0, 0, 0);
  }
  unsigned char* __restrict__ dst = a.planes + (size_t)block * kValPlaneBlock;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u32x4 hi, mid, lo;
    split8(raw[i][0], raw[i][1], hi, mid, lo);
    const int at = (vt + 256 * i) * 16;
    *reinterpret_cast<u32x4*>(dst + at) = hi;
    *reinterpret_cast<u32x4*>(dst + kValPlaneBytes + at) = mid;
    *reinterpret_cast<u32x4*>(dst + 2 * kValPlaneBytes + at) = lo;
  }
}
