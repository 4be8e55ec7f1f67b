// Input pipeline on the GPU: what GenericVisionDataset.__getitem__ + the DataLoader's collate
// do per batch in the reference (data/datasets.py:173-195 "light" augmentation, :358-372 Normalize + ToTensorV2),
// as ONE kernel over a uint8 dataset that lives in HBM: gather by index, optional light augmentation,
// Normalize(ImageNet mean/std, max_pixel_value 255), HWC uint8 -> CHW float32, labels gathered to int64.
//
// Randomness is a counter-based hash of (seed, step, dataset index): reproducible and order-independent, but
// it is NOT albumentations' random stream -- the augmented path is "parity unpinned" (albumentations is not
// installed in this environment); the un-augmented path is an exact formula.
//
// nnue_load_batch_policy (below) is the same gather with a policy -- none, light or the reference's default "medium"
// (data/datasets.py:301-350) -- and the closing A.Resize (data/datasets.py:357-361); nnue_load_batch's kernel stays as it was.
#include "common.h"

namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t z) {  // splitmix64 finaliser
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ float u01(uint64_t h) { return (float)(h >> 40) * (1.0f / 16777216.0f); }  // [0, 1)

struct Aug {
  bool flip, bc, drop;
  float alpha, beta255;
  int y0, x0, hh, hw;
};

__device__ __forceinline__ Aug draw_aug(uint64_t seed, uint64_t step, int64_t index, int H, int W) {
  const uint64_t base = mix64(seed ^ mix64((uint64_t)index * 0xd1342543de82ef95ull + step));
  Aug a;
  a.flip = u01(mix64(base + 1)) < 0.5f;                       // A.HorizontalFlip(p=0.5)
  a.bc = u01(mix64(base + 2)) < 0.2f;                         // A.RandomBrightnessContrast(0.1, 0.1, p=0.2)
  a.alpha = 1.0f + (u01(mix64(base + 3)) * 0.2f - 0.1f);      //   contrast factor
  a.beta255 = (u01(mix64(base + 4)) * 0.2f - 0.1f) * 255.0f;  //   brightness shift, by max value
  a.drop = u01(mix64(base + 5)) < 0.2f;                       // A.CoarseDropout(1 hole, 5% x 5%, p=0.2)
  a.hh = max(1, (int)(0.05f * H));
  a.hw = max(1, (int)(0.05f * W));
  a.y0 = (int)(u01(mix64(base + 6)) * (float)(H - a.hh + 1));
  a.x0 = (int)(u01(mix64(base + 7)) * (float)(W - a.hw + 1));
  return a;
}

// grid (B, ceil(H*W / 256)); thread = output pixel, all three channels
__global__ __launch_bounds__(256) void load_batch_kernel(const unsigned char* __restrict__ data,
                                                         const int64_t* __restrict__ labels_all,
                                                         const int64_t* __restrict__ indices, int H, int W, int64_t N,
                                                         int augment, uint64_t seed, uint64_t step,
                                                         float* __restrict__ out, int64_t* __restrict__ labels_out) {
  const int b = blockIdx.x;
  int64_t idx = indices[b];
  idx = idx < 0 ? 0 : (idx >= N ? N - 1 : idx);  // stays in bounds; the host validates indices
  const int hw = blockIdx.y * 256 + threadIdx.x;
  if (hw == 0) labels_out[b] = labels_all[idx];
  if (hw >= H * W) return;
  const int h = hw / W, x = hw - h * W;
  Aug a{};
  if (augment) a = draw_aug(seed, step, idx, H, W);
  const int sx = (augment && a.flip) ? W - 1 - x : x;
  const unsigned char* __restrict__ px = data + (((size_t)idx * H + h) * W + sx) * 3;
  const bool hole = augment && a.drop && h >= a.y0 && h < a.y0 + a.hh && x >= a.x0 && x < a.x0 + a.hw;
  // Normalize: (v - 255*mean) * (1 / (255*std))
  const float mean255[3] = {0.485f * 255.0f, 0.456f * 255.0f, 0.406f * 255.0f};
  const float inv_std255[3] = {1.0f / (0.229f * 255.0f), 1.0f / (0.224f * 255.0f), 1.0f / (0.225f * 255.0f)};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = (float)px[c];
    if (augment && a.bc) v = floorf(fminf(fmaxf(v * a.alpha + a.beta255, 0.0f), 255.0f));  // uint8 LUT semantics
    if (hole) v = 0.0f;
    out[(((size_t)b * 3 + c) * H + h) * W + x] = (v - mean255[c]) * inv_std255[c];
  }
}

// ---- nnue_load_batch_policy: the policies (none / light / medium) with a resize, one launch per batch ----------------------
// The reference's "medium" list (data/datasets.py:303-339) and the closing A.Resize (:357-361).  The fired geometric stages
// and the resize compose into ONE 2x3 map from output pixel to source pixel and the image is sampled once (bilinear);
// every later stage works on float levels in [0, 255] without rounding to uint8.  Both are stated differences from
// albumentations (one resampling per stage, uint8 between stages); include/nnue_hip.h has the whole definition.

enum : unsigned { PF_FLIP = 1, PF_ROT90 = 2, PF_ROTATE = 4, PF_AFFINE = 8, PF_BC = 16, PF_HSV = 32, PF_BLUR = 64, PF_NOISE = 128, PF_DROP = 256 };
constexpr int kPolicyParams = 32;  // floats per image in params_out (layout: include/nnue_hip.h)
constexpr int kTile = 16;          // output tile side: one 256-thread workgroup

struct Map23 {  // x' = a x + b y + c ; y' = d x + e y + f
  float a, b, c, d, e, f;
};
__device__ __forceinline__ Map23 compose(const Map23& A, const Map23& B) {  // A after B
  return {A.a * B.a + A.b * B.d, A.a * B.b + A.b * B.e, A.a * B.c + A.b * B.f + A.c,
          A.d * B.a + A.e * B.d, A.d * B.b + A.e * B.e, A.d * B.c + A.e * B.f + A.f};
}

struct Policy {  // what one image's workgroups need; built by thread 0, read from LDS by all
  Map23 m;
  unsigned flags;
  int constant;  // Rotate or Affine fired: taps outside the source read 0; otherwise the coordinate is clamped
  float alpha, beta255, hue, sat, val, noise_sigma;
  float w[9];  // the 3x3 blur kernel
  int y0, x0, hh, hw;
  uint64_t base;
};

// thread 0 of a workgroup: draws, composed map, record
__device__ void draw_policy(Policy& p, float* __restrict__ rec, int policy, uint64_t seed, uint64_t step, int64_t index, int H, int W,
                            int Ho, int Wo) {
  const uint64_t base = mix64(seed ^ mix64((uint64_t)index * 0xd1342543de82ef95ull + step));
  auto U = [&](int k) { return u01(mix64(base + (uint64_t)k)); };
  p.base = base;
  p.flags = 0;
  p.constant = 0;
  p.alpha = 1.0f;
  p.beta255 = 0.0f;
  p.hue = p.sat = p.val = p.noise_sigma = 0.0f;
  p.y0 = p.x0 = p.hh = p.hw = 0;
  int k90 = 0, kind = 0, dir = 0;
  float rot = 0.0f, aff_rot = 0.0f, aff_scale = 1.0f, aff_tx = 0.0f, aff_ty = 0.0f, beta = 0.0f, sigma = 0.0f;
  const float rx = (float)W / (float)Wo, ry = (float)H / (float)Ho;
  Map23 m{rx, 0.0f, 0.5f * rx - 0.5f, 0.0f, ry, 0.5f * ry - 0.5f};  // A.Resize: s = (o + 0.5) * (src / dst) - 0.5
  const Map23 flip{-1.0f, 0.0f, (float)(Wo - 1), 0.0f, 1.0f, 0.0f};
  if (policy == 1) {  // the light policy: load_batch_kernel's draws and arithmetic, in output space
    const Aug a = draw_aug(seed, step, index, Ho, Wo);
    if (a.flip) p.flags |= PF_FLIP, m = compose(m, flip);
    if (a.bc) p.flags |= PF_BC;
    if (a.drop) p.flags |= PF_DROP;
    p.alpha = a.alpha, p.beta255 = a.beta255, beta = a.beta255 * (1.0f / 255.0f);
    p.y0 = a.y0, p.x0 = a.x0, p.hh = a.hh, p.hw = a.hw;
  } else if (policy == 2) {
    const float cx = 0.5f * (float)(Wo - 1), cy = 0.5f * (float)(Ho - 1);
    if (U(16) < 0.5f) p.flags |= PF_FLIP, m = compose(m, flip);  // A.HorizontalFlip(p=0.5)
    if (U(17) < 0.5f) p.flags |= PF_ROT90;                         // A.RandomRotate90(p=0.5)
    k90 = min(3, (int)(U(18) * 4.0f));
    if ((p.flags & PF_ROT90) && k90) {  // through normalised coordinates: H != W stays defined
      const float wh = (float)Wo / (float)Ho, hw = (float)Ho / (float)Wo;
      const Map23 r1{0.0f, -wh, (float)Wo - 0.5f - 0.5f * wh, hw, 0.0f, 0.5f * hw - 0.5f};
      const Map23 r2{-1.0f, 0.0f, (float)(Wo - 1), 0.0f, -1.0f, (float)(Ho - 1)};
      const Map23 r3{0.0f, wh, 0.5f * wh - 0.5f, -hw, 0.0f, (float)Ho - 0.5f - 0.5f * hw};
      m = compose(m, k90 == 1 ? r1 : (k90 == 2 ? r2 : r3));
    }
    if (U(19) < 0.3f) p.flags |= PF_ROTATE;  // A.Rotate(limit=15, p=0.3)
    rot = (U(20) * 2.0f - 1.0f) * 15.0f;
    if (p.flags & PF_ROTATE) {
      float sn, cs;
      sincosf(rot * 0.017453292519943295f, &sn, &cs);
      m = compose(m, Map23{cs, -sn, cx - cs * cx + sn * cy, sn, cs, cy - sn * cx - cs * cy});
    }
    if (U(21) < 0.3f) p.flags |= PF_AFFINE;  // A.Affine(translate_percent +-0.1, scale 0.9..1.1, rotate +-15, p=0.3)
    aff_tx = (U(22) * 0.2f - 0.1f) * (float)Wo;
    aff_ty = (U(23) * 0.2f - 0.1f) * (float)Ho;
    aff_scale = 0.9f + U(24) * 0.2f;
    aff_rot = (U(25) * 2.0f - 1.0f) * 15.0f;
    if (p.flags & PF_AFFINE) {
      float sn, cs;
      sincosf(aff_rot * 0.017453292519943295f, &sn, &cs);
      const float is = 1.0f / aff_scale, qx = cx + aff_tx, qy = cy + aff_ty;
      m = compose(m, Map23{is * cs, is * sn, cx - is * (cs * qx + sn * qy), -is * sn, is * cs, cy - is * (cs * qy - sn * qx)});
    }
    p.constant = (p.flags & (PF_ROTATE | PF_AFFINE)) != 0;
    if (U(26) < 0.3f) p.flags |= PF_BC;  // A.RandomBrightnessContrast(0.2, 0.2, p=0.3)
    p.alpha = 1.0f + (U(27) * 0.4f - 0.2f);
    beta = U(28) * 0.4f - 0.2f;
    p.beta255 = beta * 255.0f;
    if (U(29) < 0.3f) p.flags |= PF_HSV;  // A.HueSaturationValue(10, 15, 10, p=0.3)
    p.hue = (U(30) * 2.0f - 1.0f) * 10.0f;
    p.sat = (U(31) * 2.0f - 1.0f) * 15.0f;
    p.val = (U(32) * 2.0f - 1.0f) * 10.0f;
    if (U(33) < 0.2f) p.flags |= PF_BLUR;  // A.OneOf([Blur, GaussianBlur, MotionBlur], blur_limit=3, p=0.2)
    kind = min(2, (int)(U(34) * 3.0f));
    sigma = 0.5f + U(35) * 2.5f;
    dir = min(3, (int)(U(36) * 4.0f));
    if (U(37) < 0.2f) p.flags |= PF_NOISE;  // A.GaussNoise(std_range=(0.01, 0.05), p=0.2)
    p.noise_sigma = (0.01f + U(38) * 0.04f) * 255.0f;
    if (U(39) < 0.3f) p.flags |= PF_DROP;  // A.CoarseDropout(1 hole, 5..15 % of each side, p=0.3)
    p.hh = min(Ho, max(1, (int)((0.05f + U(40) * 0.1f) * (float)Ho)));
    p.hw = min(Wo, max(1, (int)((0.05f + U(41) * 0.1f) * (float)Wo)));
    p.y0 = min(Ho - p.hh, (int)(U(42) * (float)(Ho - p.hh + 1)));
    p.x0 = min(Wo - p.hw, (int)(U(43) * (float)(Wo - p.hw + 1)));
  }
  p.m = m;
  for (int j = 0; j < 9; ++j) p.w[j] = 0.0f;
  if (kind == 0) {
    for (int j = 0; j < 9; ++j) p.w[j] = 1.0f / 9.0f;
  } else if (kind == 1) {
    const float e = expf(-0.5f / (sigma * sigma)), n = 1.0f / (1.0f + 2.0f * e);
    const float g[3] = {e * n, n, e * n};
    for (int j = 0; j < 9; ++j) p.w[j] = g[j / 3] * g[j % 3];
  } else {  // one of the four 3-tap lines through the centre: -, |, \, /
    const int first = dir == 0 ? 3 : (dir == 1 ? 1 : (dir == 2 ? 0 : 2));
    p.w[first] = p.w[4] = p.w[8 - first] = 1.0f / 3.0f;
  }
  if (rec) {
    const float r[kPolicyParams] = {(float)p.flags, (float)k90, rot, aff_rot, aff_scale, aff_tx, aff_ty, m.a, m.b, m.c, m.d, m.e, m.f,
                                    p.alpha, beta, p.hue, p.sat, p.val, (float)kind, sigma, (float)dir, p.noise_sigma,
                                    (float)p.y0, (float)p.x0, (float)p.hh, (float)p.hw, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = 0; j < kPolicyParams; ++j) rec[j] = r[j];
  }
}

__device__ __forceinline__ float tap(const unsigned char* __restrict__ img, int H, int W, int y, int x, int c) {
  return (x >= 0 && x < W && y >= 0 && y < H) ? (float)img[((size_t)y * W + x) * 3 + c] : 0.0f;
}

// stages 1-6 at one output pixel: the one bilinear sample, brightness/contrast, HSV shifts
__device__ __forceinline__ void point_chain(const Policy& p, int policy, const unsigned char* __restrict__ img, int H, int W, int ox,
                                            int oy, float v[3]) {
  float sx = p.m.a * (float)ox + p.m.b * (float)oy + p.m.c;
  float sy = p.m.d * (float)ox + p.m.e * (float)oy + p.m.f;
  if (p.constant) {  // everything outside is 0: two pixels beyond the border say the same as any farther point
    sx = fminf(fmaxf(sx, -2.0f), (float)W + 1.0f);
    sy = fminf(fmaxf(sy, -2.0f), (float)H + 1.0f);
  } else {
    sx = fminf(fmaxf(sx, 0.0f), (float)(W - 1));
    sy = fminf(fmaxf(sy, 0.0f), (float)(H - 1));
  }
  const float flx = floorf(sx), fly = floorf(sy);
  const float fx = sx - flx, fy = sy - fly;
  const int x0 = (int)flx, y0 = (int)fly;
  int x1 = x0 + 1, y1 = y0 + 1;
  if (!p.constant) x1 = min(x1, W - 1), y1 = min(y1, H - 1);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float p00 = tap(img, H, W, y0, x0, c), p01 = tap(img, H, W, y0, x1, c);
    const float p10 = tap(img, H, W, y1, x0, c), p11 = tap(img, H, W, y1, x1, c);
    const float top = p00 + fx * (p01 - p00), bot = p10 + fx * (p11 - p10);
    v[c] = top + fy * (bot - top);
  }
  if (p.flags & PF_BC) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (policy == 1)
        v[c] = floorf(fminf(fmaxf(v[c] * p.alpha + p.beta255, 0.0f), 255.0f));  // uint8 LUT semantics, as load_batch_kernel
      else
        v[c] = fminf(fmaxf(v[c] * p.alpha + p.beta255, 0.0f), 255.0f);
    }
  }
  if (p.flags & PF_HSV) {  // OpenCV's float HSV: H in degrees, S and V in [0, 1]
    const float r = v[0] * (1.0f / 255.0f), g = v[1] * (1.0f / 255.0f), b = v[2] * (1.0f / 255.0f);
    const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b)), d = mx - mn;
    float h = 0.0f;
    if (d > 0.0f) {
      if (mx == r)
        h = 60.0f * (g - b) / d;
      else if (mx == g)
        h = 120.0f + 60.0f * (b - r) / d;
      else
        h = 240.0f + 60.0f * (r - g) / d;
    }
    float s = mx > 0.0f ? d / mx : 0.0f;
    h += 2.0f * p.hue;  // the shift is on OpenCV's uint8 scale of 0..180
    h -= 360.0f * floorf(h * (1.0f / 360.0f));
    s = fminf(fmaxf(s + p.sat * (1.0f / 255.0f), 0.0f), 1.0f);
    const float val = fminf(fmaxf(mx + p.val * (1.0f / 255.0f), 0.0f), 1.0f);
    const float h6 = h * (1.0f / 60.0f);
    const float fl = floorf(h6), f = h6 - fl;
    const int sext = ((int)fl % 6 + 6) % 6;
    const float pp = val * (1.0f - s), q = val * (1.0f - s * f), t = val * (1.0f - s * (1.0f - f));
    float R, G, B;
    switch (sext) {
      case 0: R = val, G = t, B = pp; break;
      case 1: R = q, G = val, B = pp; break;
      case 2: R = pp, G = val, B = t; break;
      case 3: R = pp, G = q, B = val; break;
      case 4: R = t, G = pp, B = val; break;
      default: R = val, G = pp, B = q; break;
    }
    v[0] = R * 255.0f, v[1] = G * 255.0f, v[2] = B * 255.0f;
  }
}

__device__ __forceinline__ int reflect101(int i, int n) {  // ...2 1 | 0 1 2 ... n-2 n-1 | n-2 ...
  i = i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
  return min(max(i, 0), n - 1);
}

// grid (B, tiles of 16 x 16 output pixels); thread = output pixel, all three channels
__global__ __launch_bounds__(256) void load_batch_policy_kernel(const unsigned char* __restrict__ data, const int64_t* __restrict__ labels_all,
                                                                const int64_t* __restrict__ indices, int H, int W, int64_t N, int Ho,
                                                                int Wo, int tiles_x, int policy, uint64_t seed, uint64_t step,
                                                                float* __restrict__ out, int64_t* __restrict__ labels_out,
                                                                float* __restrict__ params_out) {
  __shared__ Policy sp;
  __shared__ float halo[3][kTile + 2][kTile + 3];  // stages 1-6 of the tile and a one-pixel ring, for the blur
  const int b = blockIdx.x;
  int64_t idx = indices[b];
  idx = idx < 0 ? 0 : (idx >= N ? N - 1 : idx);  // stays in bounds; the host validates indices
  if (threadIdx.x == 0) {
    const bool first = blockIdx.y == 0;
    if (first) labels_out[b] = labels_all[idx];
    draw_policy(sp, (first && params_out) ? params_out + (size_t)b * kPolicyParams : nullptr, policy, seed, step, idx, H, W, Ho, Wo);
  }
  __syncthreads();
  const Policy& p = sp;
  const int ty0 = (blockIdx.y / tiles_x) * kTile, tx0 = (blockIdx.y % tiles_x) * kTile;
  const int ox = tx0 + (threadIdx.x & (kTile - 1)), oy = ty0 + (threadIdx.x >> 4);
  const bool inside = ox < Wo && oy < Ho;
  const unsigned char* __restrict__ img = data + (size_t)idx * H * W * 3;
  float v[3] = {0.0f, 0.0f, 0.0f};
  if (p.flags & PF_BLUR) {  // uniform over the workgroup
    for (int e = threadIdx.x; e < (kTile + 2) * (kTile + 2); e += 256) {
      const int hy = e / (kTile + 2), hx = e - hy * (kTile + 2);
      const int gy = ty0 + hy - 1, gx = tx0 + hx - 1;
      if (gy >= -1 && gy <= Ho && gx >= -1 && gx <= Wo) {  // cv2.BORDER_REFLECT_101 at the output image's borders
        float t[3];
        point_chain(p, policy, img, H, W, reflect101(gx, Wo), reflect101(gy, Ho), t);
        halo[0][hy][hx] = t[0], halo[1][hy][hx] = t[1], halo[2][hy][hx] = t[2];
      }
    }
    __syncthreads();
    if (inside) {
      const int hy = (threadIdx.x >> 4), hx = (threadIdx.x & (kTile - 1));
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 9; ++j) acc += p.w[j] * halo[c][hy + j / 3][hx + j % 3];
        v[c] = acc;
      }
    }
  } else if (inside) {
    point_chain(p, policy, img, H, W, ox, oy, v);
  }
  if (!inside) return;
  const bool hole = (p.flags & PF_DROP) && oy >= p.y0 && oy < p.y0 + p.hh && ox >= p.x0 && ox < p.x0 + p.hw;
  const float mean255[3] = {0.485f * 255.0f, 0.456f * 255.0f, 0.406f * 255.0f};
  const float inv_std255[3] = {1.0f / (0.229f * 255.0f), 1.0f / (0.224f * 255.0f), 1.0f / (0.225f * 255.0f)};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float x = v[c];
    if (p.flags & PF_NOISE) {  // Box-Muller from a hash of (base, output pixel, channel)
      const uint64_t h = mix64(p.base + (1ull << 32) + (uint64_t)(((size_t)oy * Wo + ox) * 3 + c));
      const float u1 = ((float)(h >> 40) + 1.0f) * (1.0f / 16777216.0f);             // (0, 1]
      const float u2 = (float)((h >> 16) & 0xffffffull) * (1.0f / 16777216.0f);      // [0, 1)
      x = fminf(fmaxf(x + p.noise_sigma * sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2), 0.0f), 255.0f);
    }
    if (hole) x = 0.0f;
    out[(((size_t)b * 3 + c) * Ho + oy) * Wo + ox] = (x - mean255[c]) * inv_std255[c];
  }
}

}  // namespace

extern "C" int nnue_load_batch(const uint8_t* images_u8, const int64_t* labels_all, const int64_t* indices, int B, int H, int W,
                               int64_t N, int augment, uint64_t seed, uint64_t step, float* out, int64_t* labels_out,
                               nnue_stream_t stream) {
  NNUE_REQUIRE(images_u8 && labels_all && indices && out && labels_out, NNUE_E_ARG, "nnue_load_batch: null pointer");
  NNUE_REQUIRE(B > 0 && H > 0 && W > 0 && N > 0, NNUE_E_ARG, "nnue_load_batch: B=%d H=%d W=%d N=%lld must be positive", B, H, W, (long long)N);
  NNUE_REQUIRE((long long)H * W < (1ll << 24), NNUE_E_SHAPE, "nnue_load_batch: image too large");
  hipLaunchKernelGGL(load_batch_kernel, dim3(B, (H * W + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), images_u8, labels_all,
                     indices, H, W, N, augment, seed, step, out, labels_out);
  return nnue_launch_status("nnue_load_batch");
}

extern "C" int nnue_load_batch_params_count(void) { return kPolicyParams; }

extern "C" int nnue_load_batch_policy(const uint8_t* images_u8, const int64_t* labels_all, const int64_t* indices, int B, int H, int W,
                                      int64_t N, int Ho, int Wo, int policy, uint64_t seed, uint64_t step, float* out,
                                      int64_t* labels_out, float* params_out, nnue_stream_t stream) {
  NNUE_REQUIRE(images_u8 && labels_all && indices && out && labels_out, NNUE_E_ARG, "nnue_load_batch_policy: null pointer");
  NNUE_REQUIRE(B > 0 && H > 0 && W > 0 && N > 0 && Ho > 0 && Wo > 0, NNUE_E_ARG,
               "nnue_load_batch_policy: B=%d H=%d W=%d N=%lld Ho=%d Wo=%d must be positive", B, H, W, (long long)N, Ho, Wo);
  NNUE_REQUIRE(policy >= 0 && policy <= 2, NNUE_E_ARG, "nnue_load_batch_policy: policy %d is none of 0 (none), 1 (light), 2 (medium)", policy);
  NNUE_REQUIRE((long long)H * W < (1ll << 24) && (long long)Ho * Wo < (1ll << 24), NNUE_E_SHAPE, "nnue_load_batch_policy: image too large");
  const int tiles_x = (Wo + kTile - 1) / kTile, tiles_y = (Ho + kTile - 1) / kTile;
  NNUE_REQUIRE((long long)tiles_x * tiles_y <= 65535, NNUE_E_SHAPE, "nnue_load_batch_policy: %d x %d output tiles exceed one grid dimension",
               tiles_y, tiles_x);
  hipLaunchKernelGGL(load_batch_policy_kernel, dim3(B, tiles_x * tiles_y), dim3(256), 0, static_cast<hipStream_t>(stream), images_u8,
                     labels_all, indices, H, W, N, Ho, Wo, tiles_x, policy, seed, step, out, labels_out, params_out);
  return nnue_launch_status("nnue_load_batch_policy");
}

// ---------------------------------------------------------------- batch-level mixing (mixup / CutMix; include/nnue_hip.h)
namespace {

struct MixArgs { int B, H, W, mode; float lam; int y0, x0, hh, hw; };

// grid (chunks of an image, pairs): pair p = samples (p, B-1-p); a thread reads V consecutive elements of both images and
// writes both -- safe in place.  V = 4: float4 runs (W % 4 == 0: a run stays inside one row).  The pair's labels_b_out and
// lam_out are written by the first thread of its first workgroup; the middle sample of an odd batch keeps its pixels.
template <int V>
__global__ __launch_bounds__(256) void mix_batch_kernel(float* __restrict__ images, const int64_t* __restrict__ labels, MixArgs a,
                                                        float lam_eff, int64_t* __restrict__ labels_b_out, float* __restrict__ lam_out) {
  const int i = blockIdx.y, j = a.B - 1 - i;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t li = labels[i], lj = labels[j];
    labels_b_out[i] = lj, labels_b_out[j] = li;
    lam_out[i] = lam_eff, lam_out[j] = lam_eff;
  }
  if (a.mode == 0 || i == j) return;
  const int hw = a.H * a.W, n = 3 * hw;
  const int e = ((int)blockIdx.x * 256 + (int)threadIdx.x) * V;
  if (e >= n) return;
  float* __restrict__ pi = images + (size_t)i * n + e;
  float* __restrict__ pj = images + (size_t)j * n + e;
  float xi[V], xj[V];
  if constexpr (V == 4) {
    const float4 vi = *reinterpret_cast<const float4*>(pi), vj = *reinterpret_cast<const float4*>(pj);
    xi[0] = vi.x, xi[1] = vi.y, xi[2] = vi.z, xi[3] = vi.w;
    xj[0] = vj.x, xj[1] = vj.y, xj[2] = vj.z, xj[3] = vj.w;
  } else {
    xi[0] = *pi, xj[0] = *pj;
  }
  float oi[V], oj[V];
  if (a.mode == 1) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      oi[k] = a.lam * xi[k] + (1.0f - a.lam) * xj[k];
      oj[k] = a.lam * xj[k] + (1.0f - a.lam) * xi[k];
    }
  } else {
    const int pix = e % hw, y = pix / a.W, x = pix - y * a.W;
    const bool row_in = y >= a.y0 && y < a.y0 + a.hh;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const bool in = row_in && x + k >= a.x0 && x + k < a.x0 + a.hw;
      oi[k] = in ? xj[k] : xi[k];
      oj[k] = in ? xi[k] : xj[k];
    }
  }
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(pi) = make_float4(oi[0], oi[1], oi[2], oi[3]);
    *reinterpret_cast<float4*>(pj) = make_float4(oj[0], oj[1], oj[2], oj[3]);
  } else {
    *pi = oi[0], *pj = oj[0];
  }
}

}  // namespace

extern "C" int nnue_mix_batch(float* images, const int64_t* labels, int B, int H, int W, int mode, float lam, int y0, int x0, int hh,
                              int hw, int64_t* labels_b_out, float* lam_out, nnue_stream_t stream) {
  NNUE_REQUIRE(images && labels && labels_b_out && lam_out, NNUE_E_ARG, "nnue_mix_batch: null pointer");
  NNUE_REQUIRE(B > 0 && H > 0 && W > 0, NNUE_E_ARG, "nnue_mix_batch: B=%d H=%d W=%d must be positive", B, H, W);
  NNUE_REQUIRE((long long)H * W < (1ll << 24), NNUE_E_SHAPE, "nnue_mix_batch: image too large");
  NNUE_REQUIRE(mode >= 0 && mode <= 2, NNUE_E_ARG, "nnue_mix_batch: mode %d is none of 0 (none), 1 (mixup), 2 (CutMix)", mode);
  NNUE_REQUIRE(mode != 1 || (lam >= 0.0f && lam <= 1.0f), NNUE_E_ARG, "nnue_mix_batch: lam = %g is outside [0, 1]", (double)lam);
  NNUE_REQUIRE(mode != 2 || (y0 >= 0 && x0 >= 0 && hh >= 0 && hw >= 0 && hh <= H - y0 && hw <= W - x0), NNUE_E_ARG,
               "nnue_mix_batch: the box [%d, %d+%d) x [%d, %d+%d) leaves the %d x %d image", y0, y0, hh, x0, x0, hw, H, W);
  NNUE_REQUIRE(B <= 2 * 65535, NNUE_E_SHAPE, "nnue_mix_batch: B=%d exceeds one grid dimension of pairs", B);
  const float lam_eff = mode == 1 ? lam : mode == 2 ? (float)(H * W - hh * hw) / (float)(H * W) : 1.0f;
  const MixArgs a{B, H, W, mode, lam, y0, x0, hh, hw};
  const int n = 3 * H * W, pairs = (B + 1) / 2;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mode != 0 && W % 4 == 0 && nnue_aligned16(images))
    hipLaunchKernelGGL(mix_batch_kernel<4>, dim3((n / 4 + 255) / 256, pairs), dim3(256), 0, s, images, labels, a, lam_eff, labels_b_out, lam_out);
  else
    hipLaunchKernelGGL(mix_batch_kernel<1>, dim3(mode == 0 ? 1 : (n + 255) / 256, pairs), dim3(256), 0, s, images, labels, a, lam_eff,
                       labels_b_out, lam_out);
  return nnue_launch_status("nnue_mix_batch");
}
