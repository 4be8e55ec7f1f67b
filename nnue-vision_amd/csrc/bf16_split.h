// The pieces every bf16-split tile is built from: the exact three-way split of an f32 operand and the staging of the byte map
// into bf16 LDS images (include inside ftm_kernels.hip's anonymous namespace, after u32x4 / f32x4).  gemm_tile_bf, gemm_tile_bf64,
// gemm_tile_bf6 and the fused update + forward pass (update_forward.h) all call these: the values they stage have one definition.
// An LDS image is named by a function object img(row, chunk) -> byte offset of the 16-byte chunk (8 k) of a row: the images
// differ in row length and swizzle.  (Function objects with forced inlining, not lambdas: those are inlined late and the listings
// of the kernels change.)
using bf16x8 = __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16;
using u32x2 = __attribute__((__vector_size__(2 * sizeof(unsigned)))) unsigned;

// x = hi + mid + lo by truncation, each term a bf16 in the top half of its word
__device__ __forceinline__ void split3(float x, unsigned& hi, unsigned& mid, unsigned& lo) {
  const unsigned hb = __float_as_uint(x) & 0xffff0000u;
  const float r1 = x - __uint_as_float(hb);
  const unsigned mb = __float_as_uint(r1) & 0xffff0000u;
  const float r2 = r1 - __uint_as_float(mb);
  hi = hb; mid = mb; lo = __float_as_uint(r2);
}
// the bf16 of two k-neighbours as one word: k in the low half, k + 1 in the high half
__device__ __forceinline__ unsigned pack_k2(unsigned k0, unsigned k1) { return __builtin_amdgcn_perm(k1, k0, 0x07060302u); }

// 2 NW k x 4 n block of floats (row k of it: a float4 or the four words of one 16-byte load) -> per plane and column e the NW
// words (2 NW bf16 along k) pl[plane][e]
__device__ __forceinline__ float block_elem(const u32x4& row, int e) { return __uint_as_float(row[e]); }
__device__ __forceinline__ float block_elem(const float4& row, int e) { return e == 0 ? row.x : e == 1 ? row.y : e == 2 ? row.z : row.w; }
template <int NW, class V, class Row>
__device__ __forceinline__ void split_block(const Row (&x)[2 * NW], V (&pl)[3][4]) {
#pragma unroll
  for (int t = 0; t < NW; ++t) {
    unsigned h[2][4], m[2][4], l[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const float xs[4] = {block_elem(x[2 * t + u], 0), block_elem(x[2 * t + u], 1), block_elem(x[2 * t + u], 2), block_elem(x[2 * t + u], 3)};
#pragma unroll
      for (int e = 0; e < 4; ++e) split3(xs[e], h[u][e], m[u][e], l[u][e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {  // word t of column e: k = 2 t (low half) and 2 t + 1 (high half)
      pl[0][e][t] = pack_k2(h[0][e], h[1][e]);
      pl[1][e][t] = pack_k2(m[0][e], m[1][e]);
      pl[2][e][t] = pack_k2(l[0][e], l[1][e]);
    }
  }
}

// 8 consecutive k (two float4) -> one 16-byte chunk of 8 bf16 per plane
__device__ __forceinline__ void split8(const u32x4& v0, const u32x4& v1, u32x4& hi, u32x4& mid, u32x4& lo) {
  unsigned h[8], m[8], l[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) split3(__uint_as_float(e < 4 ? v0[e] : v1[e - 4]), h[e], m[e], l[e]);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    hi[t] = pack_k2(h[2 * t], h[2 * t + 1]);
    mid[t] = pack_k2(m[2 * t], m[2 * t + 1]);
    lo[t] = pack_k2(l[2 * t], l[2 * t + 1]);
  }
}

// four {0,1} bytes -> four bf16 (two words)
__device__ __forceinline__ void bytes_to_bf16(unsigned x, unsigned& w0, unsigned& w1) {
  w0 = ((x & 0xffu) | ((x & 0xff00u) << 8)) * 0x3f80u;
  w1 = (((x >> 16) & 0xffu) | ((x >> 8) & 0xff0000u)) * 0x3f80u;
}

// Map staging along k (the bytes are contiguous along k): 16 bytes of map row `row` -> chunks c and c + 1 of its image row
template <class Img>
__device__ __forceinline__ void stage_map_k(unsigned char* As, Img img, int row, int c, const u32x4& raw) {
  u32x4 lo, hi;
  unsigned a, b;
  bytes_to_bf16(raw[0], a, b); lo[0] = a; lo[1] = b;
  bytes_to_bf16(raw[1], a, b); lo[2] = a; lo[3] = b;
  bytes_to_bf16(raw[2], a, b); hi[0] = a; hi[1] = b;
  bytes_to_bf16(raw[3], a, b); hi[2] = a; hi[3] = b;
  *reinterpret_cast<u32x4*>(As + img(row, c)) = lo;
  *reinterpret_cast<u32x4*>(As + img(row, c + 1)) = hi;
}

// Map staging along m (the bytes are contiguous along m): eight words = 8 consecutive k x 4 m -> chunk c of image rows
// m4 .. m4 + 3 (byte e of the eight words = 8 consecutive k of row m4 + e)
template <class Img>
__device__ __forceinline__ void stage_map_m(unsigned char* As, Img img, int m4, int c, const unsigned (&rat)[8]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    u32x4 v;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const unsigned sel = 0x0c000c00u | (unsigned)e | ((unsigned)(4 + e) << 16);  // [lo.byte e, 0, hi.byte e, 0]
      v[t] = __builtin_amdgcn_perm(rat[2 * t + 1], rat[2 * t], sel) * 0x3f80u;
    }
    *reinterpret_cast<u32x4*>(As + img(m4 + e, c)) = v;
  }
}
