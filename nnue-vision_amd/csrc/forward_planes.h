// The table of the fused-L1 forward as pre-split bf16 planes: the layout of the plane buffer, the image of a 128-deep K tile
// (bf_img) and the writer that rides in the conv launch (feature_kernels.hip) -- one definition for the writer and for the
// reader (gemm_tile_bf with PL, ftm_kernels.hip).  Include inside the including file's anonymous namespace.
//
// Layout: one block of kFwdPlaneBlock bytes per (column tile tile_n of 64, K tile kt of 128), block index tile_n * ktiles + kt;
// a block is byte for byte what gemm_tile_bf<32, 64, true, FwdL1Epi> stages behind its A image for that K tile:
//   block + plane * 64 * 256 + bf_img(n, chunk)   = the 8 bf16 (k = 128 kt + 8 chunk .. + 7) of plane `plane` (0 hi, 1 mid, 2 lo)
//                                                   of table column NNUE_FWD_L1_COL(64 tile_n + n, L1 / 2), rows k >= direct as zeros
// so a forward thread copies 16 * (tid + 256 j), j < 12, from the block to the same linear offset of its LDS.
#pragma once

using u32x4 = __attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned;

constexpr int kBfK = 128;  // K tile depth of gemm_tile_bf

// byte offset of 16-byte chunk `chunk` of image row `row`
__device__ __forceinline__ int bf_img(int row, int chunk) { return row * (kBfK * 2) + ((chunk ^ (row & 15)) << 4); }

#include "bf16_split.h"  // split3 / split_block / split8, stage_map_k / stage_map_m

// Table / ft column of the fused forward's tile-local column index n_abs = 64 * tile + n_local: a tile's 64 columns are two
// 32-column runs `half` apart (FwdL1Epi, ftm_kernels.hip).  One definition for FwdL1Epi::col and the planes' writer -- a macro,
// not a function: as a forceinline function called from col() it is inlined in another order and an instruction of four
// existing forward kernels moves.
#define NNUE_FWD_L1_COL(n_abs, half) ((((n_abs) >> 6) << 5) + ((n_abs) & 31) + (((n_abs) & 32) ? (half) : 0))

// A table beyond this many bytes does not stay in the caches over a launch: the tiles stream it (non-temporal loads) and
// the planes-fed forward does not take it (planes would be 1.5x its bytes, written and read every step).
constexpr unsigned kStreamTableBytes = 64u << 20;

constexpr int kFwdPlaneBlock = 3 * 64 * kBfK * 2;  // 48 KB

struct FwdPlaneArgs {
  const float* __restrict__ weight;     // table [F][L1]
  unsigned char* __restrict__ planes;   // tiles_n * ktiles blocks
  unsigned w_bytes;                     // window of the rows the map reaches: direct * L1 * 4 (rows past it read as zero)
  int L1, ktiles, parts;                // parts: workgroups per block (256 / threads of the launch)
};

// One workgroup's share of one block: what fetch + stage of gemm_tile_bf do for B (the same 8 k x 4 n block per thread, the
// same windowed buffer loads, the same split), stored to memory instead of LDS.  `rider` in [0, blocks * parts); blockDim.x
// in {64, 128, 256}.  No LDS, no barrier.
__device__ __forceinline__ void forward_planes_write(const FwdPlaneArgs& a, int rider) {
  const int block = rider / a.parts, part = rider - block * a.parts;
  const int tile_n = block / a.ktiles, kt = block - tile_n * a.ktiles;
  const int vt = part * (int)blockDim.x + (int)threadIdx.x;  // thread of the 256 that stage a K tile
  const int lane = vt & 63, wave = vt >> 6;
  const int bn4 = ((lane & 1) | ((lane >> 3) << 1)) * 4, bk8 = (((lane >> 1) & 3) | (wave << 2)) * 8;
  const int n_abs = tile_n * 64 + bn4;
  const int b_off = NNUE_FWD_L1_COL(n_abs, a.L1 / 2) * 4;
  const __amdgpu_buffer_rsrc_t rsb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.weight), 0, a.w_bytes, 0x00020000);
  u32x4 rb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) rb[j] = __builtin_amdgcn_raw_buffer_load_b128(rsb, (kt * kBfK + bk8 + j) * a.L1 * 4 + b_off, 0, 0);
  u32x4 pl[3][4];  // [plane][n]: 8 bf16
  split_block<4>(rb, pl);
  unsigned char* __restrict__ dst = a.planes + (size_t)block * kFwdPlaneBlock;
#pragma unroll
  for (int pnum = 0; pnum < 3; ++pnum)
#pragma unroll
    for (int e = 0; e < 4; ++e) *reinterpret_cast<u32x4*>(dst + pnum * (64 * kBfK * 2) + bf_img(bn4 + e, bk8 >> 3)) = pl[pnum][e];
}
