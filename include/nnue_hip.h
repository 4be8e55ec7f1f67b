/*
 * nnue_hip.h -- C ABI of libnnue_hip.so: the MI355X (gfx950) kernels behind the
 * NNUE training hot path of marict/nnue-vision.
 *
 * The reference has no FFI seam for this path: the seam is the Python module
 * surface of nnue.py.  This library is what a ctypes
 * binding under that surface calls; every entry point below names the
 * reference code (file:line under the reference root) whose arithmetic it
 * replaces.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, ints, floats; no torch / C++ types;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*;
 *     NULL = the null stream) and never synchronises, allocates or frees:
 *     scratch memory is passed in, so calls can be captured into a hipGraph;
 *   - tensors are dense row-major float32 unless stated; ids are int32 inside
 *     the library and int64 at the reference boundary (nnue_ft_prepare);
 *   - return 0 on success, a negative NNUE_E_* code otherwise; nothing throws.
 *     nnue_hip_last_error() returns a thread-local description of the last
 *     failure.  Arguments are validated BEFORE any launch: a call that returns
 *     an error has launched nothing.
 *   - all float pointers must be 16-byte aligned (torch allocations are).
 *
 * Active-feature list ("act list") layout shared by the calls below, capacity
 * `cap` entries per sample:
 *     rows[b*cap + k]  int32  table row, already clamped to [0, F-1]
 *     coef[b*cap + k]  float  multiplier (feature value; 1.0 for binary features)
 *     pos [b*cap + k]  int32  where the entry's value-gradient goes
 *     n[b]             int32  number of valid entries of sample b (k < n[b])
 * and the transposed coefficient matrix
 *     coefT[f*ldb + b] float  sum of coef over the entries of sample b that map to row f
 * with ldb >= B a multiple of 64.  Entries keep the caller's order.
 */
#ifndef NNUE_HIP_H
#define NNUE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNUE_HIP_ABI_VERSION 39

#define NNUE_OK 0
#define NNUE_E_ARG (-1)     /* null pointer, non-positive size, bad alignment */
#define NNUE_E_SHAPE (-2)   /* sizes inconsistent with each other */
#define NNUE_E_LAUNCH (-3)  /* HIP reported a launch error */
#define NNUE_E_SCRATCH (-4) /* scratch buffer too small */

typedef void* nnue_stream_t; /* hipStream_t */
/* arguments of the classifier's small-gradient tile family when it rides in nnue_ftm_backward's launch (opaque; filled by
 * nnue_classifier_train_rider, read by nnue_ftm_backward[_bucketed]) */
typedef struct nnue_cls_rider { unsigned char opaque[256]; } nnue_cls_rider;

int nnue_hip_abi_version(void);
const char* nnue_hip_last_error(void);

/* ---- front end ---------------------------------------------------------------- */

/* nn.Conv2d(3, fps, 3, stride, padding=1, bias=False)  (nnue.py:486-493, call :640).
 * images [B,3,H,W], weight [fps,3,3,3] (OIHW), conv_out [B,fps,Gh,Gw] with
 * Gh = (H-1)/stride + 1, Gw = (W-1)/stride + 1.  Each output is one fmaf chain over
 * (ci, kh, kw) in that order, so results do not depend on the launch shape. */
int nnue_conv3x3_forward(const float* images, const float* weight, float* conv_out,
                         int B, int H, int W, int fps, int stride, nnue_stream_t stream);

/* Gradient of that conv w.r.t. its input (autograd of nnue.py:640; the training step never needs it -- offered
 * so that NNUE.forward's autograd node differentiates w.r.t. the pixels without a stock op):
 *   d_images[b,ci,y,x] = sum_{c,kh,kw : y = oh*stride+kh-1, x = ow*stride+kw-1} d_conv_out[b,c,oh,ow] * weight[c,ci,kh,kw]
 * one fixed-order fmaf chain per pixel and channel. */
int nnue_conv3x3_backward_input(const float* d_conv_out, const float* weight, int B, int H, int W, int fps,
                                int stride, float* d_images, nnue_stream_t stream);

/* The value half of NNUE._to_sparse_features (nnue.py:601-606, :628-633): the values are the map's own entries at the
 * active ids:  val[b,i] = map[b, idx[b,i]]  (idx >= 0; 0 for the -1 padding);  map [B,P], idx int64 [B,M]. */
int nnue_sparse_values(const float* map, const int64_t* idx, int B, int P, int M, float* val, nnue_stream_t stream);
/* ... and its autograd (CopySlices / IndexBackward of nnue.py:628-633): the values stay attached to the map,
 *   d_map[b,idx[b,i]] = d_val[b,i], every other element 0 (ids of a sample are distinct). */
int nnue_sparse_values_backward(const float* d_val, const int64_t* idx, int B, int P, int M, float* d_map,
                                nnue_stream_t stream);

/* StraightThroughBinary.forward + NNUE._to_sparse_features  (nnue.py:19-25, :590-635)
 * without the data-dependent width: per sample, ascending flat ids p = c*Gh*Gw + h*Gw + w
 * with conv_out > thr[c], written as an act list of capacity P = fps*Gh*Gw
 * (rows = min(p, F-1), pos = p, coef = 1) and as coefT [F, ldb] (rows < F-1: the bit;
 * row F-1: the number of active ids >= F-1 -- the clamp of nnue.py:701).  Ids are bit-exact
 * given conv_out.  Every element of rows/pos/coef beyond n[b] is left untouched;
 * coefT is fully overwritten: its pad columns B <= b < ldb are zero in every row. */
int nnue_binarize_features(const float* conv_out, const float* thr,
                           int B, int fps, int Gh, int Gw, int F,
                           int32_t* rows, int32_t* pos, float* coef, int32_t* n,
                           float* coefT, int ldb, nnue_stream_t stream);

/* Same ids in the reference's own format (nnue.py:609-633): idx [B,M] int64 padded with -1,
 * val [B,M] float32 padded with 0, from an act list whose max n[b] the caller has read
 * back (M = max(max n, 1)). */
int nnue_act_to_padded(const int32_t* pos, const float* coef, const int32_t* n, int cap,
                       int B, int M, int64_t* idx, float* val, nnue_stream_t stream);

/* StraightThroughBinary.backward for the threshold + conv weight gradient
 * (nnue.py:28-54; autograd of the conv at nnue.py:640).
 *   d_thr[c]            = -sum_{b,h,w} d_conv_out * k*s*(1-s),  s = sigmoid(k*(x - thr[c])), k = 10
 *   d_weight[c,ci,kh,kw] = sum_{b,h,w} d_conv_out[b,c,h,w] * images[b,ci,h*stride+kh-1,w*stride+kw-1]
 * Deterministic two-stage sum; scratch >= nnue_ste_conv_backward_scratch(...) bytes.
 * stages: 3 = both; 1 = stage 1 only: the per-workgroup partials stay at the start of scratch as
 * partial[(c*28+q)*chunks + k], k < nnue_ste_conv_backward_chunks(...), q < 27 the conv-weight terms, q = 27 the
 * threshold term, and d_thr / d_weight are not written -- finish with stages = 2 (same arguments) or hand the
 * partials to nnue_sgd_step, whose norm launch then carries the second stage. */
int64_t nnue_ste_conv_backward_scratch(int B, int fps, int Gh, int Gw);
int64_t nnue_ste_conv_backward_chunks(int B, int fps, int Gh, int Gw);
int nnue_ste_conv_backward(const float* images, const float* conv_out, const float* thr,
                           const float* d_conv_out, int B, int H, int W, int fps, int stride,
                           float* d_thr, float* d_weight, void* scratch, int64_t scratch_bytes,
                           int stages, nnue_stream_t stream);
/* The same sums (nnue.py:28-54; autograd of the conv at nnue.py:640) from the im2col form of the images that
 * nnue_ftm_conv_binarize_patches leaves: patches [27][B*Gh*Gw] f32, term-major, read coalesced along positions instead of pixels
 * gathered at the conv stride, and conv_out (required).  d_thr, d_weight and the stage-1 partials are BITWISE those of
 * nnue_ste_conv_backward.  fps <= 64. */
int nnue_ste_conv_backward_patches(const float* patches, const float* conv_out, const float* thr,
                                   const float* d_conv_out, int B, int fps, int Gh, int Gw,
                                   float* d_thr, float* d_weight, void* scratch, int64_t scratch_bytes,
                                   int stages, nnue_stream_t stream);

/* ---- FeatureTransformer ------------------------------------------------------- */

/* Turns the reference-format inputs of FeatureTransformer.forward (nnue.py:686: idx int64
 * [B,M], -1 = padding, any order, repeats allowed; val float32 [B,M]) into an act list of
 * capacity M (valid entries compacted in order, rows clamped as nnue.py:701, pos = original
 * column) and coefT [F, ldb].  coefT is zeroed by the call.  Repeats accumulate. */
int nnue_ft_prepare(const int64_t* idx, const float* val, int B, int M, int F,
                    int32_t* rows, int32_t* pos, float* coef, int32_t* n,
                    float* coefT, int ldb, nnue_stream_t stream);

/* FeatureTransformer.forward  (nnue.py:686-710):
 *   out[b,:] = bias + sum_{k<n[b]} coef[b,k] * weight[rows[b,k], :]
 * weight [F,L1], out [B,L1]. */
int nnue_ft_forward(const float* weight, const float* bias,
                    const int32_t* rows, const float* coef, const int32_t* n, int cap,
                    int B, int F, int L1, float* out, nnue_stream_t stream);

/* Gradient of the above w.r.t. weight and bias (autograd IndexBackward + index_put_
 * (accumulate) of nnue.py:702-708), as a per-row gather-sum over coefT -- no atomics,
 * bitwise reproducible:
 *   d_weight[f,:] = sum_b coefT[f,b] * d_out[b,:]      d_bias = sum_b d_out[b,:]
 * Either output may be NULL. */
int nnue_ft_backward_weight(const float* d_out, const float* coefT, int ldb,
                            int B, int F, int L1, float* d_weight, float* d_bias,
                            nnue_stream_t stream);

/* Gradient w.r.t. the feature values (autograd of nnue.py:705-707):
 *   dst[b*dst_ld + pos[b,k]] = < d_out[b,:], weight[rows[b,k],:] >   for k < n[b]
 * dst is zero-filled first ([B, dst_ld]); dst_ld = M for the stand-alone op, P when the
 * values are the binary map (the gradient then IS d_conv_out, nnue.py:628-633 + :33). */
int nnue_ft_backward_values(const float* d_out, const float* weight,
                            const int32_t* rows, const int32_t* pos, const int32_t* n, int cap,
                            int B, int F, int L1, float* dst, int dst_ld, nnue_stream_t stream);

/* ---- FeatureTransformer for binary grid features: bit masks, tile lists, LDS-staged tiles ---------
 *
 * Inside NNUE.forward the feature values are exactly {0,1} and the ids ascend (nnue.py:590-635), so
 * the act list collapses to
 *     maskW[b*pw64 + w]  uint64  bit (p & 63) of word p >> 6 = flat position p of sample b is active
 *     maskT[f*bw64 + w]  uint64  bit (b & 63) of word b >> 6 = sample b selects table row f (f < F-1: its
 *                                own position; f = F-1: sink[b] != 0; f = F: every sample -- the bias row)
 *     sink[b]            float   number of active positions >= F-1 (they all clamp to row F-1, nnue.py:701)
 * (pw64, bw64 even) and, per output and per tile of 128 staged rows, a padded list of the rows to add:
 *     tlW [B][tiles_fwd][128] u16 / tcW [B][tiles_fwd] u8       sample b   x table-row tile
 *     tlT [F+1][tiles_bwd][128] u16 / tcT [F+1][tiles_bwd] u8   output row x batch tile
 * Entries are LDS byte offsets (local row or sample index * 256), ascending, padded with 32768 (= an all-zero
 * row); entry e sits in slot ((e>>2)&3)*32 + (e>>4)*4 + (e&3); tc holds the entry count.  The list buffers
 * are passed as uint8_t* (256 bytes per record).
 * A workgroup stages a tile of the table (or of d_out) in LDS once and all its samples (rows) gather from
 * LDS, so memory-side traffic is the table once per sample tile instead of once per sample.  L1 must be 256,
 * 512 or 1024 (nnue_ftb_supported); other widths use the list kernels above. */
int nnue_ftb_supported(int L1);
int nnue_ftb_list_tiles(int B, int F, int P, int* tiles_fwd, int* tiles_bwd);
int64_t nnue_ftb_scratch(int B, int F, int P, int L1); /* bytes for nnue_ftb_forward / _backward_weight */

/* StraightThroughBinary.forward + _to_sparse_features as bit masks and tile lists (nnue.py:19-25,
 * :590-635).  Also writes n[b] = number of active positions.  Bit-exact given conv_out.
 * stages: 1 = per-sample outputs (maskW, sink, n, tlW/tcW), 2 = transposed outputs (maskT, tlT/tcT; needs
 * sink from stage 1), 3 = both.  The transposed outputs are only read by nnue_ftb_backward_weight, so a
 * caller may run stage 2 on a second stream beside the forward. */
int nnue_binarize_bits(const float* conv_out, const float* thr, int B, int fps, int Gh, int Gw, int F,
                       uint64_t* maskW, int pw64, uint64_t* maskT, int bw64, float* sink, int32_t* n,
                       uint8_t* tlW, uint8_t* tcW, uint8_t* tlT, uint8_t* tcT, int stages, nnue_stream_t stream);

/* FeatureTransformer.forward for binary features (nnue.py:686-710):
 *   out[b,:] = bias + sum_{p active, p < min(F-1,P)} weight[p,:] + sink[b] * weight[F-1,:] */
int nnue_ftb_forward(const float* weight, const float* bias, const uint8_t* tlW, const uint8_t* tcW,
                     const float* sink, int B, int F, int P, int L1, float* out,
                     void* scratch, int64_t scratch_bytes, nnue_stream_t stream);

/* Its weight/bias gradient (autograd of nnue.py:702-708), fixed summation order, no atomics.
 * Either output may be NULL. */
int nnue_ftb_backward_weight(const float* d_out, const uint8_t* tlT, const uint8_t* tcT, const float* sink,
                             int B, int F, int P, int L1, float* d_weight, float* d_bias,
                             void* scratch, int64_t scratch_bytes, nnue_stream_t stream);

/* Its value gradient scattered to the map (autograd of nnue.py:705-707 and :628-633; identity STE :33):
 *   d_conv_out[b,p] = active(b,p) ? < d_out[b,:], weight[min(p,F-1),:] > : 0     for every p < P */
int nnue_ftb_backward_values(const float* d_out, const float* weight, const uint64_t* maskW, int pw64,
                             int B, int F, int P, int L1, float* d_conv_out, nnue_stream_t stream);

/* ---- FeatureTransformer for binary grid features as dense products on the f32 MFMA ----------------
 *
 * At the reference's threshold 43 % of the grid features are active (414 of 968 at 32x32), so the products
 *     out      = A W + bias,   d_weight = A^T d_out,   d_value = (d_out W^T) . A
 * with A[b][f] = membership of table row f in sample b are dense enough to run as matrix products
 * (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulate; summation order differs from the gather
 * kernels).  A is the binary map itself as a byte {0,1} matrix bits[B][P] (P = fps*Gh*Gw, nnue.py:19-25),
 * widened to float while tiles are staged; no masks or id lists are built.  sink[b] = number of active positions >= F-1 (they clamp to row F-1,
 * nnue.py:701), a rank-one term.  P and L1 must be multiples of 4 (nnue_ftm_supported). */
int nnue_ftm_supported(int F, int P, int L1);
int64_t nnue_ftm_scratch(int B, int F, int P, int L1); /* bytes for nnue_ftm_forward (split-K slabs) */

/* StraightThroughBinary.forward as a byte matrix (nnue.py:19-25): bits[b,p] = conv_out[b,p] > thr[channel of p],
 * n[b] = active positions (nnue.py:603-607), sink[b] as above.  Bit-exact given conv_out. */
int nnue_ftm_binarize(const float* conv_out, const float* thr, int B, int fps, int Gh, int Gw, int F,
                      uint8_t* bits, int32_t* n, float* sink, nnue_stream_t stream);

/* nnue_conv3x3_forward + nnue_ftm_binarize in one launch (self.conv + StraightThroughBinary.forward, nnue.py:640,
 * :646-647, :19-25): conv_out, bits, n and sink are bitwise what the two calls give. */
int nnue_ftm_conv_binarize(const float* images, const float* weight, const float* thr, int B, int H, int W,
                           int fps, int stride, int F, float* conv_out, uint8_t* bits, int32_t* n, float* sink,
                           nnue_stream_t stream);
/* The same launch (nnue.py:640, :646-647, :19-25) also leaving the im2col form of the images for the backward:
 * patches[q][b*Gh*Gw + hw] = the pixel under tap q = ci*9 + kh*3 + kw of position hw (0 where the tap falls off the image),
 * 27*B*Gh*Gw floats: with a stride above 3 the taps of neighbouring positions do not overlap and the patches are a fraction of
 * the images (0.18 at 224x224, stride 7).  conv_out is required.  conv_out, bits, n and sink are bitwise nnue_ftm_conv_binarize's. */
int nnue_ftm_conv_binarize_patches(const float* images, const float* weight, const float* thr, int B, int H, int W,
                                   int fps, int stride, int F, float* patches, float* conv_out, uint8_t* bits,
                                   int32_t* n, float* sink, nnue_stream_t stream);

/* FeatureTransformer.forward for the binary map (nnue.py:686-710):
 *   out[b,:] = bias + sum_{p active, p < min(F-1,P)} weight[p,:] + sink[b] * weight[F-1,:] */
int nnue_ftm_forward(const uint8_t* bits, const float* sink, const float* weight, const float* bias,
                     int B, int F, int P, int L1, float* out,
                     void* scratch, int64_t scratch_bytes, nnue_stream_t stream);

int nnue_ftm_forward_l1_supported(int B, int F, int P, int L1, int L2); /* shapes nnue_ftm_forward_l1 takes */

/* nnue_ftm_forward that also forms, in its epilogue, each 64-column tile's share of the pairwise block and the
 * classifier's first Linear (nnue.py:660-666, :728-730): part[t][b][j] for t < L1/64, to be consumed by
 * nnue_classifier_train_step with phases bit 8 (part = the start of its scratch).  out (the FeatureTransformer
 * output) is bitwise what nnue_ftm_forward writes.  Shapes: nnue_ftm_forward_l1_supported (declared above). */
int nnue_ftm_forward_l1(const uint8_t* bits, const float* sink, const float* weight, const float* bias,
                        const float* w1, int B, int F, int P, int L1, int L2, float* out, float* part,
                        nnue_stream_t stream);

/* The table of nnue_ftm_forward_l1 as pre-split bf16 planes, written once per step by rider workgroups of the conv launch and
 * read by the 32-row bf16 fused forward in place of the table (every row tile of nnue_ftm_forward_l1's bf16 form splits its own
 * slab of the table again).  Plane buffer: one 48 KB block per (64-column tile t, 128-row K tile kt), block t * ktiles + kt
 * (ktiles = ceil(min(F-1, P) / 128)); inside a block, plane p (0 hi, 1 mid, 2 lo: weight = hi + mid + lo exactly, each a bf16)
 * of table column c(n) = 32 t + (n & 31) + (n & 32 ? L1/2 : 0), n < 64, rows k = 128 kt + 8 ch .. + 7 as eight bf16 at byte
 *     p * 16384 + n * 256 + ((ch ^ (n & 15)) << 4);          rows k >= min(F-1, P) are zeros.
 * _supported: nnue_ftm_forward_l1_supported shapes whose 32-row tiles fill the chip (>= 256 workgroups) where 64-row ones do not,
 * with a table of at most 64 MB.  _bytes: the size of the plane buffer (0 for sizes no such buffer exists for). */
int nnue_ftm_forward_l1_planes_supported(int B, int F, int P, int L1, int L2);
int64_t nnue_ftm_forward_planes_bytes(int B, int F, int P, int L1);

/* nnue_ftm_conv_binarize (self.conv + StraightThroughBinary.forward, nnue.py:640, :646-647, :19-25) whose launch also writes the
 * planes of `table` (input.weight [F][L1], the operand of nnue.py:702-708) into `planes`: conv_out, bits, n and sink are bitwise
 * nnue_ftm_conv_binarize's.  Shapes: nnue_ftm_forward_l1_planes_supported with P = fps * Gh * Gw.  There is no form that also
 * leaves the im2col patches (nnue_ftm_conv_binarize_patches): a caller that wants those keeps the two plain calls. */
int nnue_ftm_conv_binarize_planes(const float* images, const float* weight, const float* thr, int B, int H, int W,
                                  int fps, int stride, int F, const float* table, int L1, int L2, void* planes,
                                  int64_t planes_bytes, float* conv_out, uint8_t* bits, int32_t* n, float* sink,
                                  nnue_stream_t stream);

/* nnue_ftm_forward_l1 (nnue.py:686-710 + :660-666, :728-730) reading the planes nnue_ftm_conv_binarize_planes wrote from the
 * same `weight`; weight itself is read for the clamp-sink row F-1 only.  out and part are bitwise what nnue_ftm_forward_l1
 * gives with its 32-row bf16 tiles (NNUE_FTM_BF_BM=32).  Up to 7 K tiles of 128 (min(F - 1, P) <= 896) each wave loads its
 * fragments of the planes straight into the MFMA's operands; deeper shapes, and NNUE_FTM_FWD_STREAM=0 (read per call), stage
 * the planes through LDS -- the same bits. */
int nnue_ftm_forward_l1_planes(const uint8_t* bits, const float* sink, const void* planes, int64_t planes_bytes,
                               const float* weight, const float* bias, const float* w1, int B, int F, int P, int L1,
                               int L2, float* out, float* part, nnue_stream_t stream);

/* Its weight/bias gradient (autograd of nnue.py:702-708); fixed summation order, no atomics.  Rows the map
 * cannot reach are written as zero.  Either output may be NULL. */
int nnue_ftm_backward_weight(const uint8_t* bits, const float* sink, const float* d_out,
                             int B, int F, int P, int L1, float* d_weight, float* d_bias,
                             nnue_stream_t stream);

/* Its value gradient on the map (autograd of nnue.py:705-707 and :628-633; identity STE :33):
 *   d_conv_out[b,p] = active(b,p) ? < d_out[b,:], weight[min(p,F-1),:] > : 0     for every p < P */
int nnue_ftm_backward_values(const uint8_t* bits, const float* d_out, const float* weight,
                             int B, int F, int P, int L1, float* d_conv_out, nnue_stream_t stream);
/* nnue_ftm_backward_values (autograd of nnue.py:702-708 and :628-633), argument checks and result included, under a
 * workspace-taking signature.  No shape needs a workspace: nnue_ftm_backward_values_scratch returns 0 and scratch may be
 * NULL.  The entry point exists because callers time the value gradient by this name. */
int64_t nnue_ftm_backward_values_scratch(int B, int F, int P, int L1);
int nnue_ftm_backward_values_ws(const uint8_t* bits, const float* d_out, const float* weight, int B, int F, int P, int L1,
                                float* d_conv_out, void* scratch, int64_t scratch_bytes, nnue_stream_t stream);

int nnue_ftm_backward_cw_supported(int B, int F, int P, int L1, int L2); /* shapes whose nnue_ftm_backward takes d_w1 */
int64_t nnue_ftm_backward_sq_count(int B, int F, int P, int L1); /* floats nnue_ftm_backward's sq_partial receives; 0: none */
/* runs of STE partials nnue_ftm_backward's ste_partial receives (fps == 8 image grids of the merged launch); 0: not taken */
int64_t nnue_ftm_backward_ste_chunks(int B, int F, int P, int L1, int H, int W, int stride);
int nnue_ftm_backward_ste_supported(int B, int F, int P, int L1, int H, int W, int stride); /* nnue_ftm_backward_ste_chunks > 0 */

/* nnue_ftm_backward_weight + nnue_ftm_backward_values as ONE launch (autograd of nnue.py:702-708, :628-633): the
 * two products and the tail rows are independent, so their workgroups share the chip.  Same results, bit for bit,
 * as the two separate calls.  d_weight, d_bias and d_conv_out are required.
 * Optional rider (d_w1 != NULL, shapes: nnue_ftm_backward_cw_supported, declared above): the weight gradient of the
 * classifier's first Linear, d_w1[L2][L1] = d_z1^T l0 (autograd of nnue.py:728-730 through the pairwise block
 * nnue.py:660-666), from ft[B][L1] (the FeatureTransformer output) and d_z1[B][L2] (left in the classifier's scratch
 * by nnue_classifier_train_step, at nnue_classifier_train_dz1_offset); pair with phases bit 16 there.  Beside bf16
 * weight tiles (nnue_ftm_uses_bf16(2, ...)) the rider runs as six bf16 plane products, the value gradient's
 * arithmetic: terms below an f32 rounding of a product are dropped and an Inf operand gives NaN; with NNUE_FTM_BF16=0
 * it runs on the f32 MFMA.
 * sq_partial (may be NULL): nnue_ftm_backward_sq_count(B, F, P, L1) floats (declared above) that receive, per
 * weight-gradient tile, the sum of the squares of the elements it wrote -- together the squared norm of
 * d_weight[0 .. min(F-1, P)) -- so that nnue_sgd_step (ext_partial) need not read those rows again for
 * clip_grad_norm_ (train.py:363-364).
 * small != NULL (filled by nnue_classifier_train_rider; merged-launch shapes only): the classifier's small batch-reduced
 * gradients (d_w3, d_w2, the three bias gradients; autograd of nnue.py:728-734) and the mean loss (train.py:250-254) run as
 * one more tile family of this launch -- ~30 workgroups beside a few hundred -- instead of beside the classifier's d_x tiles
 * (nnue_classifier_train_step phases bit 32).
 * ste_partial != NULL (shapes with nnue_ftm_backward_ste_chunks > 0): the value-gradient tiles also reduce d_conv_out into the
 * partial sums of the threshold and conv-weight gradients -- stage 1 of nnue_ste_conv_backward (the straight-through
 * threshold nnue.py:28-54 and the conv's autograd at nnue.py:640) -- from ste_images [B][3][H][W] (or, when ste_patches !=
 * NULL, the im2col patches [27][B * Gh * Gw] of nnue_ftm_conv_binarize_patches: the same bits), ste_conv_out [B][P] and
 * ste_thr [fps]: [fps * 28][chunks] floats (ste_partial_bytes >= 4 * fps * 28 * chunks), whose second stage is
 * nnue_sgd_step's ste argument (clip_grad_norm_ + SGD, train.py:363-366).  d_conv_out may then be NULL (not stored). */
int nnue_ftm_backward(const uint8_t* bits, const float* sink, const float* d_out, const float* weight,
                      int B, int F, int P, int L1, float* d_weight, float* d_bias, float* d_conv_out,
                      const float* ft, const float* d_z1, int L2, float* d_w1, float* sq_partial,
                      const nnue_cls_rider* small, const float* ste_images, const float* ste_patches, const float* ste_conv_out,
                      const float* ste_thr, int H, int W, int stride, float* ste_partial, int64_t ste_partial_bytes,
                      nnue_stream_t stream);

/* The table rows the value gradient d_val = (d_out W^T) . A of the STE ride reads, as pre-split bf16 planes written once per step
 * by rider workgroups of the conv launch.  The contraction runs along L1, so a 16-byte chunk is 8 consecutive j (L1 index) of one
 * table row; the writer applies the value tiles' column order (tile t, column n: channel n / 8, grid position min(8 t + n % 8,
 * G - 1), G = P / 8) and the row clamp p >= F-1 -> F-1 (nnue.py:701).  One 48 KB block per (column tile t, 128-deep K tile kt),
 * block t * ktiles + kt (ktiles = ceil(L1 / 128)); inside a block plane p (0 hi, 1 mid, 2 lo: weight = hi + mid + lo exactly) of
 * column n = 16 w + r, j = 128 kt + 32 kb + 8 q .. + 7 sits at byte p * 16384 + ((4 w + kb) * 64 + 16 q + r) * 16 (the MFMA's
 * fragment order); j >= L1 are zeros.
 * _supported: shapes whose merged backward takes the STE ride on 32-row value tiles (nnue_ftm_backward_ste_chunks > 0 with
 * ceil(B / 32) row tiles), L1 % 8 == 0, at least 256 value tiles (NNUE_FTM_VAL_PLANES_MIN_TILES, read per call, lowers the floor
 * for tests), NNUE_FTM_VAL_PLANES != 0 (read per call).  _bytes: the size of the plane buffer (0 where none exists). */
int nnue_ftm_value_planes_supported(int B, int F, int P, int L1, int H, int W, int stride);
int64_t nnue_ftm_value_planes_bytes(int B, int F, int P, int L1);

/* nnue_ftm_conv_binarize_planes (self.conv + StraightThroughBinary.forward, nnue.py:640, :646-647, :19-25) whose launch also
 * writes the value planes of `table` into `val_planes`: more rider workgroups behind the forward's.  conv_out, bits, n, sink and
 * `planes` are bitwise nnue_ftm_conv_binarize_planes'.  Shapes: both _supported queries; planes == NULL: the value planes alone
 * (nnue_ftm_value_planes_supported shapes), no forward riders. */
int nnue_ftm_conv_binarize_value_planes(const float* images, const float* weight, const float* thr, int B, int H, int W,
                                        int fps, int stride, int F, const float* table, int L1, int L2, void* planes,
                                        int64_t planes_bytes, void* val_planes, int64_t val_planes_bytes, float* conv_out,
                                        uint8_t* bits, int32_t* n, float* sink, nnue_stream_t stream);

/* nnue_ftm_backward (autograd of nnue.py:702-708 and :628-633) whose 32-row value tiles read the table from `val_planes` (written
 * this step by nnue_ftm_conv_binarize_value_planes from the same `weight`) as six bf16 plane products instead of the f32 MFMA.
 * Taken where nnue_ftm_value_planes_supported says yes and ste_partial != NULL; every other call launches what nnue_ftm_backward
 * launches (val_planes must still be a valid pointer).  d_weight, d_bias, d_w1, sq_partial and the small gradients are bitwise
 * nnue_ftm_backward's; d_conv_out and the STE partials differ by the summation order and the dropped mid.lo + lo.mid + lo.lo
 * terms (below 2^-23 of a product). */
int nnue_ftm_backward_planes(const uint8_t* bits, const float* sink, const float* d_out, const float* weight,
                             int B, int F, int P, int L1, float* d_weight, float* d_bias, float* d_conv_out,
                             const float* ft, const float* d_z1, int L2, float* d_w1, float* sq_partial,
                             const nnue_cls_rider* small, const float* ste_images, const float* ste_patches, const float* ste_conv_out,
                             const float* ste_thr, int H, int W, int stride, float* ste_partial, int64_t ste_partial_bytes,
                             const void* val_planes, int64_t val_planes_bytes, nnue_stream_t stream);

/* ---- pairwise product + SimpleClassifier -------------------------------------- */

/* Forward of  l0 = cat(x[:, :L1/2] * x[:, L1/2:], x[:, :L1/2])  (nnue.py:660-666, when
 * `pairwise` != 0; l0 = x otherwise) followed by Linear(L1,L2)+act, Linear(L2,L3)+act,
 * Linear(L3,C)  (nnue.py:728-734).  act = ReLU, or min(ReLU, clip) when clip > 0 (build
 * extension, off = reference).  Saves h1 [B,L2], h2 [B,L3] (post-activation) for backward.
 * scratch >= nnue_classifier_scratch(B, L1, L2, L3) bytes (covers forward and backward). */
int64_t nnue_classifier_scratch(int B, int L1, int L2, int L3);
int nnue_classifier_forward(const float* x, int pairwise,
                            const float* w1, const float* b1, const float* w2, const float* b2,
                            const float* w3, const float* b3, float clip,
                            int B, int L1, int L2, int L3, int C,
                            float* h1, float* h2, float* logits,
                            void* scratch, int64_t scratch_bytes, nnue_stream_t stream);

/* Backward of the above (autograd of nnue.py:660-669 and :728-734 in the reference).  d_x [B,L1]
 * is the gradient w.r.t. x (through the pairwise block when `pairwise`); NULL skips it.  Weight/bias gradients are overwritten, not accumulated. */
int nnue_classifier_backward(const float* x, int pairwise,
                             const float* w1, const float* w2, const float* w3, float clip,
                             const float* h1, const float* h2, const float* d_logits,
                             int B, int L1, int L2, int L3, int C,
                             float* d_x, float* d_w1, float* d_b1, float* d_w2, float* d_b2,
                             float* d_w3, float* d_b3,
                             void* scratch, int64_t scratch_bytes, nnue_stream_t stream);

/* The bits of nnue_classifier_train_step's `phases` (described there). */
#define NNUE_CLS_PHASE_DX 1        /* activations, per-sample losses and d_x */
#define NNUE_CLS_PHASE_SMALL 2     /* the mean loss and the six weight/bias gradients */
#define NNUE_CLS_DW1_BESIDE_DX 4   /* the first-layer weight product shares the d_x launch */
#define NNUE_CLS_L1_SLABS_GIVEN 8  /* the layer-1 slabs are at the start of scratch already */
#define NNUE_CLS_DW1_RIDES 16      /* d_w1 is left to nnue_ftm_backward's rider */
#define NNUE_CLS_SMALL_RIDE 32     /* ... and so are the small gradients and the mean loss */
#define NNUE_CLS_TAIL_IN_DX 64     /* the per-sample tail runs inside the d_x launch (only as 123) */

/* The three calls above as ONE training step of the pairwise/classifier block with mean cross-entropy
 * (nnue.py:660-669, :728-734 + compute_loss, train.py:250-254, and their autograd): same results as
 * nnue_classifier_forward -> nnue_cross_entropy(grad_scale) -> nnue_classifier_backward, but the narrow
 * layers, the loss and their backward run per sample in a single kernel.  d_x may be NULL.
 * phases is a sum of the NNUE_CLS_* bits below.  NNUE_CLS_PHASE_DX (1) = activations, per-sample losses and d_x (the
 * critical path of a training step), NNUE_CLS_PHASE_SMALL (2) = the mean loss and the six weight/bias gradients (needs
 * NNUE_CLS_PHASE_DX on the same scratch; nothing downstream waits for it, so a caller may run it on a second stream),
 * 3 = both.  NNUE_CLS_DW1_BESIDE_DX (4; phases 5 then 6, or 7) moves the first-layer weight product into the d_x launch
 * -- both only need d_z1, so the two small products share the chip; the NNUE_CLS_PHASE_SMALL call (same arguments)
 * then only sums its slabs.  Results are identical either way.  NNUE_CLS_L1_SLABS_GIVEN (8) says the layer-1
 * pre-activation slabs part[L1/64][B][L2] are already at the START of scratch, written by nnue_ftm_forward_l1 (the
 * FeatureTransformer forward forms them in its epilogue); NNUE_CLS_PHASE_DX then launches no layer-1 product of its
 * own.  NNUE_CLS_DW1_RIDES (16, not together with NNUE_CLS_DW1_BESIDE_DX) says d_w1 is produced by nnue_ftm_backward's
 * rider from the d_z1 this call leaves in scratch at byte offset nnue_classifier_train_dz1_offset (-1 for non-positive
 * sizes): no first-layer weight product and no slab sum are launched here, d_w1 is not written; with both phases in the
 * one call (19, 27) the small weight/bias gradients and the mean loss share the d_x launch -- unless
 * NNUE_CLS_SMALL_RIDE (32) is added as well (51, 59): then they are left to nnue_ftm_backward's launch too (its `small`
 * argument, filled by nnue_classifier_train_rider with the same tensors and scratch), and the d_x launch holds only d_x
 * tiles.  NNUE_CLS_TAIL_IN_DX (64) exists in that one combination only (123 = 59 + 64; any other use of it is refused
 * as a bad phases value): the per-sample tail runs inside the d_x launch -- each d_x row tile recomputes the tail of its
 * own 16 rows, so NNUE_CLS_PHASE_DX is one launch -- with outputs bitwise those of 59.  It needs
 * nnue_classifier_train_fused_tail_supported(B, L1, L2, L3, C, 1, pairwise) (else NNUE_E_SHAPE) and 16-byte aligned w2
 * and w3.
 * scratch >= nnue_classifier_train_scratch(B, L1, L2, L3, C) bytes. */
int64_t nnue_classifier_train_scratch(int B, int L1, int L2, int L3, int C);
int64_t nnue_classifier_train_dz1_offset(int B, int L1, int L2, int L3, int C, int pairwise);
int nnue_classifier_train_step(const float* x, int pairwise,
                               const float* w1, const float* b1, const float* w2, const float* b2,
                               const float* w3, const float* b3, float clip,
                               const int64_t* labels, float grad_scale,
                               int B, int L1, int L2, int L3, int C,
                               float* h1, float* h2, float* logits, float* sample_loss, float* loss,
                               float* d_x, float* d_w1, float* d_b1, float* d_w2, float* d_b2,
                               float* d_w3, float* d_b3,
                               void* scratch, int64_t scratch_bytes, int phases, nnue_stream_t stream);
/* 1 when nnue_classifier_train_step takes phases 123 at this shape (K layer stacks), 0 otherwise: K == 1, the pairwise
 * block (nnue.py:660-666), C <= 64, L1 % 128 == 0, and L2 = 128, L3 = 32 (the widths the fused kernel is built for;
 * nnue.py:713-738).  Other shapes keep phases 59's two launches. */
int nnue_classifier_train_fused_tail_supported(int B, int L1, int L2, int L3, int C, int K, int pairwise);
/* A host-side call (no launch) that fills `out` with the arguments of the small-gradient tile family for a step run with
 * phases bit 32 -- d_w3, d_w2, d_b3, d_b2, d_b1 (autograd of nnue.py:728-734) and the mean loss (train.py:250-254) then run
 * inside nnue_ftm_backward's launch (its `small` argument).  Same tensors and scratch as the train step; buckets = NULL
 * for one layer stack. */
int nnue_classifier_train_rider(int pairwise, int B, int L1, int L2, int L3, int C, const float* h1, const float* h2,
                                const float* sample_loss, float* loss, float* d_b1, float* d_w2, float* d_b2,
                                float* d_w3, float* d_b3, void* scratch, int64_t scratch_bytes,
                                const struct nnue_buckets* buckets, nnue_cls_rider* out);

/* ---- bucketed layer stacks (build extension; BASELINE configs[2]) -------------------------------------------------
 *
 * The reference trains ONE SimpleClassifier (nnue.py:713-738; serialize.py:57 writes num_ls_buckets = 1) while its
 * engine still loads N LayerStacks (engine/src/nnue_engine.cpp:619-635).  K > 1 here = K independent weight sets
 * w1 [K][L2][L1], b1 [K][L2], w2 [K][L3][L2], b2 [K][L3], w3 [K][C][L3], b3 [K][C], one selected per sample:
 *     bucket[b] = min(K-1, n[b] * K / (P + 1)),  n[b] = active features of sample b, P = flat ids of the map
 * -- a by-product of the binarise kernels.  There is no reference for K > 1 (parity unpinned; oracle/nnue_oracle.py
 * holds the CPU restatement); with K == 1 every *_bucketed entry point is exactly its plain counterpart.
 * nnue_bucket_group sorts the samples by bucket (stable) into bucket-homogeneous 16-row tiles so that each MFMA
 * tile of the first layer multiplies by one bucket's weights:
 *     rows[16 t + i]   sample in row i of tile t (-1 = padding)     tile_bucket[t]  its bucket (-1 = unused tile)
 *     seg[k], seg[k+1] row range of bucket k (multiples of 16)      t < nnue_bucket_tile_count(B, K) = ceil(B/16) + K
 * All arrays are int32 device memory; the struct itself is read on the host. */
typedef struct nnue_buckets {
  int32_t K;                  /* layer stacks; <= 1: single stack, pointers ignored */
  const int32_t* bucket;      /* [B] */
  const int32_t* rows;        /* [tiles * 16] */
  const int32_t* tile_bucket; /* [tiles] */
  const int32_t* seg;         /* [K + 1] */
  int32_t tiles;              /* nnue_bucket_tile_count(B, K) */
} nnue_buckets;

int nnue_bucket_tile_count(int B, int K);
/* Selector + grouping in one single-workgroup launch (the K = 1 case of the structure is nnue.py:713-738; header field
 * serialize.py:57).  P == 0: n[b] is taken as the bucket itself (clamped to [0, K-1]) -- the stand-alone classifier
 * call.  K <= 64. */
int nnue_bucket_group(const int32_t* n, int B, int P, int K, int32_t* bucket, int32_t* rows,
                      int32_t* tile_bucket, int32_t* seg, nnue_stream_t stream);

/* nnue_ftm_forward (nnue.py:686-710) with nnue_bucket_group riding in the same launch as one extra workgroup: the grouping
 * only needs the binarise kernel's counts n, like the product itself, so it costs no launch of its own.  Same outputs as
 * the two calls. */
int nnue_ftm_forward_grouping(const uint8_t* bits, const float* sink, const float* weight, const float* bias,
                              int B, int F, int P, int L1, float* out, void* scratch, int64_t scratch_bytes,
                              const int32_t* n, int K, int32_t* bucket, int32_t* rows, int32_t* tile_bucket,
                              int32_t* seg, nnue_stream_t stream);

/* nnue_classifier_forward / _backward / _train_step (nnue.py:660-666, :728-734 and their autograd) with stacked
 * weights and gradients [K][...] and the grouping above.  train_step: phases bits 8 and 16 are refused for K > 1
 * (those products live in the FeatureTransformer launches, which know one stack).  d_w1 of a bucket is summed over
 * slices of that bucket's own rows; scratch sizes from the *_scratch_bucketed functions. */
int64_t nnue_classifier_scratch_bucketed(int B, int L1, int L2, int L3, int K);
int64_t nnue_classifier_train_scratch_bucketed(int B, int L1, int L2, int L3, int C, int K);
int nnue_classifier_forward_bucketed(const float* x, int pairwise,
                                     const float* w1, const float* b1, const float* w2, const float* b2,
                                     const float* w3, const float* b3, float clip,
                                     int B, int L1, int L2, int L3, int C,
                                     float* h1, float* h2, float* logits,
                                     void* scratch, int64_t scratch_bytes, const nnue_buckets* buckets,
                                     nnue_stream_t stream);
/* autograd of the bucketed forward (nnue.py:728-734 per stack): gradients [K][...], d_x [B][L1]. */
int nnue_classifier_backward_bucketed(const float* x, int pairwise,
                                      const float* w1, const float* w2, const float* w3, float clip,
                                      const float* h1, const float* h2, const float* d_logits,
                                      int B, int L1, int L2, int L3, int C,
                                      float* d_x, float* d_w1, float* d_b1, float* d_w2, float* d_b2,
                                      float* d_w3, float* d_b3,
                                      void* scratch, int64_t scratch_bytes, const nnue_buckets* buckets,
                                      nnue_stream_t stream);
/* forward + mean cross-entropy + backward of the bucketed block in one call (train.py:250-254, :360-361 on top of
 * nnue.py:728-734 per stack).  phases bit 16 with K > 1 (pairwise block, L1 % 4 == 0): d_w1 is left to
 * nnue_ftm_backward_bucketed; the per-sample kernel then runs once per GROUPED row and leaves that product's operands in
 * grouped row order inside scratch -- d_z1 [tiles*16][L2] at nnue_classifier_train_dz1_grouped_offset and the block's
 * input x [tiles*16][L1] at nnue_classifier_train_x_grouped_offset (byte offsets; padding rows zero; -1 for K <= 1). */
int64_t nnue_classifier_train_dz1_grouped_offset(int B, int L1, int L2, int L3, int C, int K);
int64_t nnue_classifier_train_x_grouped_offset(int B, int L1, int L2, int L3, int C, int K);
int nnue_classifier_train_step_bucketed(const float* x, int pairwise,
                                        const float* w1, const float* b1, const float* w2, const float* b2,
                                        const float* w3, const float* b3, float clip,
                                        const int64_t* labels, float grad_scale,
                                        int B, int L1, int L2, int L3, int C,
                                        float* h1, float* h2, float* logits, float* sample_loss, float* loss,
                                        float* d_x, float* d_w1, float* d_b1, float* d_w2, float* d_b2,
                                        float* d_w3, float* d_b3,
                                        void* scratch, int64_t scratch_bytes, int phases,
                                        const nnue_buckets* buckets, nnue_stream_t stream);

/* ---- soft targets (build extension: label smoothing, mixup, CutMix) -------------------------------------------------
 *
 * The reference's loop trains on one integer label per sample (compute_loss, train.py:250-254); label smoothing is one
 * argument of its F.cross_entropy and mixup / CutMix two lines around the batch.  Here the loss sits inside the
 * classifier's tail kernels, so the soft form is an arm of those kernels.  Per sample b: labels a = labels[b] and
 * a2 = labels_b[b], a weight lam[b] in [0, 1], and one smoothing constant eps in [0, 1) per call; labels_b == NULL
 * means a2 = a and lam = 1 (lam is then not read).  With mx = max_c z_c and se = sum_c exp(z_c - mx):
 *     t_c       = (1-eps) (lam [c == a] + (1-lam) [c == a2]) + eps/C
 *     loss_b    = log(se) + (1-eps) (lam (mx - z_a) + (1-lam) (mx - z_a2)) + (eps/C) sum_c (mx - z_c)
 *     d_logit_c = (exp(z_c - mx)/se - t_c) grad_scale / B
 * = lam CE(z, a) + (1-lam) CE(z, a2), each with label_smoothing = eps as F.cross_entropy defines it.  Every term of the
 * loss is non-negative and each mx - z is formed before anything is summed (the form of the plain loss), so it stays
 * accurate with logits near 1e4.  A sample counts iff a is in [0, C) and (lam == 1 or a2 is in [0, C)); otherwise its
 * loss is 0 and its gradient row is 0 (the padding rule of the plain kernels; -1 pads a short batch).  The mean is over
 * B, summed in sample order.  With eps = 0, lam = 1 the values are those of the plain entry points.
 *
 * Distillation (the teacher arm; knowledge distillation in Hinton's form, (1-alpha) CE + alpha T^2 KL(q || pT)): beside
 * the soft target a row of teacher logits u = teacher[b] (float32 [B][C], row stride C, finite) per sample, and one weight
 * alpha in [0, 1] and one temperature T > 0 per call.  With mu = max_c u_c, sT = sum_c exp((z_c - mx)/T) and
 * sU = sum_c exp((u_c - mu)/T):
 *     q_c       = exp((u_c - mu)/T) / sU           (the teacher at temperature T)
 *     pT_c      = exp((z_c - mx)/T) / sT           (the student at temperature T; max_c z_c/T = mx/T: no second maximum)
 *     KL_b      = log sT - log sU + (1/T) sum_c q_c ((mx - z_c) - (mu - u_c))        ( = sum_c q_c (log q_c - log pT_c) )
 *     loss_b    = (1-alpha) L_soft_b + alpha T^2 KL_b                   (L_soft_b: the loss_b above)
 *     d_logit_c = ((1-alpha) (exp(z_c - mx)/se - t_c) + alpha T (pT_c - q_c)) grad_scale / B
 * Every mx - z and mu - u is formed before anything is summed.  A sample counts iff the rule above says so; one that does
 * not has loss 0 and a zero gradient row exactly, whatever its teacher row holds (NaN included).  alpha == 0: teacher may
 * be NULL and is not read; the call IS the soft call (the same launches, the same bits). */

/* nnue_classifier_train_step / _bucketed (nnue.py:660-669, :728-734 + compute_loss, train.py:250-254, and their autograd)
 * on the soft targets above: the same phases, plan, scratch layout, refusals and launches, with the SOFT arm of the
 * per-sample tail (whichever kernel the plan picks) in place of the plain one; h1, h2 and logits do not depend on the
 * loss and are bitwise the plain call's.  Two more refusals, both NNUE_E_ARG with nothing launched: eps outside [0, 1),
 * and labels_b without lam. */
int nnue_classifier_train_step_soft(const float* x, int pairwise,
                                    const float* w1, const float* b1, const float* w2, const float* b2,
                                    const float* w3, const float* b3, float clip,
                                    const int64_t* labels, float grad_scale,
                                    int B, int L1, int L2, int L3, int C,
                                    float* h1, float* h2, float* logits, float* sample_loss, float* loss,
                                    float* d_x, float* d_w1, float* d_b1, float* d_w2, float* d_b2,
                                    float* d_w3, float* d_b3,
                                    void* scratch, int64_t scratch_bytes, int phases,
                                    const int64_t* labels_b, const float* lam, float eps, nnue_stream_t stream);
/* the bucketed form of the call above (train.py:250-254, :360-361 on top of nnue.py:728-734 per stack); the grouped mode of
 * phases bit 16 comes with it. */
int nnue_classifier_train_step_soft_bucketed(const float* x, int pairwise,
                                             const float* w1, const float* b1, const float* w2, const float* b2,
                                             const float* w3, const float* b3, float clip,
                                             const int64_t* labels, float grad_scale,
                                             int B, int L1, int L2, int L3, int C,
                                             float* h1, float* h2, float* logits, float* sample_loss, float* loss,
                                             float* d_x, float* d_w1, float* d_b1, float* d_w2, float* d_b2,
                                             float* d_w3, float* d_b3,
                                             void* scratch, int64_t scratch_bytes, int phases,
                                             const int64_t* labels_b, const float* lam, float eps,
                                             const nnue_buckets* buckets, nnue_stream_t stream);

/* nnue_classifier_train_step_soft (nnue.py:660-669, :728-734 + compute_loss, train.py:250-254, and their autograd) with the
 * teacher arm defined under "soft targets": the same phases, plan, scratch layout, refusals and launches with the DISTILL arm
 * of the per-sample tail; it reads B*C*4 bytes more.  h1, h2 and logits are bitwise the plain call's.  Three more refusals,
 * NNUE_E_ARG with nothing launched: alpha outside [0, 1] (or NaN), temperature not finite or <= 0, teacher == NULL with
 * alpha > 0.  NNUE_E_SHAPE where the per-sample tail's LDS row of teacher logits does not fit (L2 + 2 L3 + 2 C + 8 floats
 * over 64 KiB). */
int nnue_classifier_train_step_distill(const float* x, int pairwise,
                                       const float* w1, const float* b1, const float* w2, const float* b2,
                                       const float* w3, const float* b3, float clip,
                                       const int64_t* labels, float grad_scale,
                                       int B, int L1, int L2, int L3, int C,
                                       float* h1, float* h2, float* logits, float* sample_loss, float* loss,
                                       float* d_x, float* d_w1, float* d_b1, float* d_w2, float* d_b2,
                                       float* d_w3, float* d_b3,
                                       void* scratch, int64_t scratch_bytes, int phases,
                                       const int64_t* labels_b, const float* lam, float eps,
                                       const float* teacher, float alpha, float temperature, nnue_stream_t stream);
/* the bucketed form of the call above (train.py:250-254, :360-361 on top of nnue.py:728-734 per stack), grouped mode included;
 * teacher rows are in sample order, like labels. */
int nnue_classifier_train_step_distill_bucketed(const float* x, int pairwise,
                                                const float* w1, const float* b1, const float* w2, const float* b2,
                                                const float* w3, const float* b3, float clip,
                                                const int64_t* labels, float grad_scale,
                                                int B, int L1, int L2, int L3, int C,
                                                float* h1, float* h2, float* logits, float* sample_loss, float* loss,
                                                float* d_x, float* d_w1, float* d_b1, float* d_w2, float* d_b2,
                                                float* d_w3, float* d_b3,
                                                void* scratch, int64_t scratch_bytes, int phases,
                                                const int64_t* labels_b, const float* lam, float eps,
                                                const float* teacher, float alpha, float temperature,
                                                const nnue_buckets* buckets, nnue_stream_t stream);

/* The table's weight gradient consumed where it is produced (single rank, SGD): clip_grad_norm_ needs the global norm
 * before any parameter moves (train.py:363-366), and
 *     || A^T D ||_F^2 = sum_{b,b'} (A A^T)_{bb'} (D D^T)_{bb'}      (A = the map [B][direct], D = d_out [B][L1])
 * gives the table's share from two B x B Gram matrices without forming the [direct][L1] gradient.
 * nnue_ftm_gram_sqnorm leaves nnue_ftm_gram_sq_count(B, L1) partial sums (unscaled; sum = that squared norm, formed as
 * sum (G_A D) . D so that D D^T is not needed either) for nnue_sgd_step(ext_partial, ..., coef_out,
 * ext_applied_elsewhere = 1); gram is nnue_ftm_gram_scratch(B, F, P) floats of scratch whose first B*B hold A A^T afterwards
 * (formed on the i8 matrix unit straight from the byte map; K slices leave int32 slabs behind it, added in slice order:
 * no atomics, nothing to clear).  nnue_ftm_backward_tail_rows forms the rows the product does not cover (d_bias, row F-1, zero
 * rows: what nnue_ftm_backward_weight adds to its product).  nnue_ftm_backward_weight_update then runs the product
 * d_W = A^T d_out (autograd of nnue.py:702-708) and, element by element in its epilogue, the optimizer's update
 *     g = coef[0]*grad_scale*d_W + wd*w ;  m = first_step ? g : momentum*m + g ;  w -= lr*m       (train.py:457-464)
 * on table rows [0, direct) -- the same arithmetic nnue_sgd_step applies -- so d_weight is never written or read back
 * (268 MB each way at the 224x224 configuration).  momentum_rows may be NULL when momentum == 0. */
int64_t nnue_ftm_gram_sq_count(int B, int L1);
/* floats of scratch behind nnue_ftm_gram_sqnorm's gram pointer (clip_grad_norm_, train.py:363-366: see above) */
int64_t nnue_ftm_gram_scratch(int B, int F, int P);
int nnue_ftm_gram_sqnorm(const uint8_t* bits, const float* d_out, int B, int F, int P, int L1,
                         float* gram, float* sq_partial, nnue_stream_t stream);
/* nnue_ftm_gram_sqnorm with nnue_ftm_backward_tail_rows' workgroups riding in its first launch (clip_grad_norm_, train.py:363-366 +
 * autograd of nnue.py:691, :701-708): both only read the map / d_out; the same results, one launch fewer. */
int nnue_ftm_gram_sqnorm_tail(const uint8_t* bits, const float* sink, const float* d_out, int B, int F, int P, int L1,
                              float* gram, float* sq_partial, float* d_weight, float* d_bias, nnue_stream_t stream);
/* (autograd of nnue.py:691, :701-708 for the bias row and the clamp-sink row F-1) */
int nnue_ftm_backward_tail_rows(const float* sink, const float* d_out, int B, int F, int P, int L1,
                                float* d_weight, float* d_bias, nnue_stream_t stream);
/* (autograd of nnue.py:702-708 + train.py:363-366, :457-464, see above) */
int nnue_ftm_backward_weight_update(const uint8_t* bits, const float* d_out, int B, int F, int P, int L1,
                                    float* weight, float* momentum_rows, const float* coef,
                                    float lr, float momentum, float weight_decay, float grad_scale,
                                    int first_step, const float* lr_dev, nnue_stream_t stream);

/* nnue_ftm_backward_weight_update of step t and nnue_ftm_forward of step t+1 in ONE pass over the table (inside a group of
 * steps whose batches are already resident: the optimizer of train.py:457-464 followed by FeatureTransformer.forward,
 * nnue.py:686-710, of the next loop iteration, train.py:359-366).  The update leaves every new table tile in registers and
 * the next forward contracts exactly those tiles, so the forward's own read of the table (268 MB at the 224x224
 * configuration) disappears.  bits_next / sink_next: the next batch's map (nnue_ftm_conv_binarize under the conv weights
 * nnue_sgd_step has just updated; a different buffer than bits); bias and weight row F-1 must already hold their updated
 * values (nnue_sgd_step applies them); out_next [B][L1]; scratch as nnue_ftm_forward (nnue_ftm_scratch bytes).  Table,
 * momentum and out_next are BITWISE what the two separate calls produce.  B = rows of bits / d_out (the batch -- or, under the
 * factor exchange, the all-gathered global batch: 64, 128, 256, 512 or 1024 rows), B_next = rows of the next map and of out_next
 * (<= 128).  Only where the forward is a split-K product over a big table (nnue_ftm_update_forward_supported: L1 % 64 == 0,
 * >= 4096 table rows); NNUE_E_SHAPE otherwise. */
int nnue_ftm_update_forward_supported(int B, int B_next, int F, int P, int L1);
/* (train.py:457-464 + nnue.py:686-710 of the next step, see above) */
int nnue_ftm_backward_weight_update_forward(const uint8_t* bits, const float* d_out, int B, int F, int P, int L1,
                                            float* weight, float* momentum_rows, const float* coef,
                                            float lr, float momentum, float weight_decay, float grad_scale,
                                            int first_step, const float* lr_dev,
                                            const uint8_t* bits_next, const float* sink_next, int B_next, const float* bias,
                                            float* out_next, void* scratch, int64_t scratch_bytes, nnue_stream_t stream);

/* The same two passes for the reference's other optimizer, torch.optim.Adam (create_optimizer, train.py:465-471): the product
 * d_W = A^T d_out (autograd of nnue.py:702-708) and, element by element in its epilogue, clip_grad_norm_ + Adam
 *     g = coef[0]*grad_scale*d_W + wd*w ;  m = b1 m + (1-b1) g ;  v = b2 v + (1-b2) g^2
 *     w -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)                                  (train.py:363-366, :465-470)
 * on table rows [0, direct) and the matching rows of exp_avg / exp_avg_sq (16-byte aligned) -- the arithmetic of
 * nnue_adam_step -- so d_weight is never written or read back.  t = step_counter[0] is read, not advanced: run it after
 * nnue_adam_step_ext(ext_applied_elsewhere = 1) of the same step, which advances the counter and leaves coef.  lr_dev as in
 * nnue_sgd_step.  Rejected like nnue_adam_step: betas outside [0,1), eps <= 0; B*L1 > 2^24 (the Gram norm's limit): NNUE_E_SHAPE. */
int nnue_ftm_backward_weight_update_adam(const uint8_t* bits, const float* d_out, int B, int F, int P, int L1,
                                         float* weight, float* exp_avg_rows, float* exp_avg_sq_rows, const float* coef,
                                         const int32_t* step_counter, float lr, float beta1, float beta2, float eps,
                                         float weight_decay, float grad_scale, const float* lr_dev, nnue_stream_t stream);
/* nnue_ftm_backward_weight_update_adam of step t and nnue_ftm_forward of step t+1 in ONE pass over the table (train.py:465-470 +
 * FeatureTransformer.forward, nnue.py:686-710, of the next loop iteration): arguments and shapes as
 * nnue_ftm_backward_weight_update_forward (nnue_ftm_update_forward_supported is the shape query for both); table, both moments
 * and out_next are BITWISE what the two separate calls produce. */
int nnue_ftm_backward_weight_update_forward_adam(const uint8_t* bits, const float* d_out, int B, int F, int P, int L1,
                                                 float* weight, float* exp_avg_rows, float* exp_avg_sq_rows, const float* coef,
                                                 const int32_t* step_counter, float lr, float beta1, float beta2, float eps,
                                                 float weight_decay, float grad_scale, const float* lr_dev,
                                                 const uint8_t* bits_next, const float* sink_next, int B_next, const float* bias,
                                                 float* out_next, void* scratch, int64_t scratch_bytes, nnue_stream_t stream);

/* Reporting only: 1 when the product of this shape runs on the bf16 matrix unit (exact three-way split of the f32
 * operand), 0 on the f32 MFMA.  which: 0 forward, 1 stand-alone weight gradient, 2 weight-gradient tiles of the merged
 * backward launch, 3 weight gradient with the update in its epilogue; 4 stand-alone value gradient, 5 value-gradient tiles
 * of the merged launch (both operands f32: six bf16 plane products hi.hi, hi.mid, mid.hi, mid.mid, hi.lo, lo.hi of the
 * two truncation splits -- what is left out is below 2^-23 of a product). */
int nnue_ftm_uses_bf16(int which, int B, int F, int P, int L1);

/* nnue_ftm_backward for bucketed layer stacks (declared with the FeatureTransformer entry points above): d_w1 [K][L2][L1],
 * ft_grouped / d_z1_grouped in grouped row order (grouped_rows = 16 * nnue_bucket_tile_count rows, padding rows zero),
 * seg [K+1] the buckets' row ranges.  The rider's tile family repeats per bucket and contracts only that bucket's rows
 * (autograd of nnue.py:728-730 per stack, through the pairwise block nnue.py:660-666).  K == 1: nnue_ftm_backward. */
int nnue_ftm_backward_bucketed(const uint8_t* bits, const float* sink, const float* d_out, const float* weight,
                               int B, int F, int P, int L1, float* d_weight, float* d_bias, float* d_conv_out,
                               const float* ft_grouped, const float* d_z1_grouped, int L2, float* d_w1,
                               float* sq_partial, int K, const int32_t* seg, int grouped_rows,
                               const nnue_cls_rider* small, const float* ste_images, const float* ste_patches, const float* ste_conv_out,
                               const float* ste_thr, int H, int W, int stride, float* ste_partial, int64_t ste_partial_bytes,
                               nnue_stream_t stream);

/* ---- loss + step tail ---------------------------------------------------------- */

/* F.cross_entropy(logits, labels) (mean over the batch, train.py:250-254) and its gradient
 * d_logits = (softmax - onehot) * grad_scale / B (may be NULL: forward only).
 * sample_loss [B] receives the per-sample losses, loss (device scalar) their mean, summed in
 * sample order (deterministic).  Labels outside [0, C) contribute loss 0 and a zero gradient
 * row -- the caller validates labels; the kernel only stays in bounds. */
int nnue_cross_entropy(const float* logits, const int64_t* labels, int B, int C, float grad_scale,
                       float* sample_loss, float* loss, float* d_logits, nnue_stream_t stream);

/* nnue_cross_entropy (compute_loss, train.py:250-254) on soft targets, as defined under "soft targets" above: labels_b and
 * lam may both be NULL (a2 = a, lam = 1), eps in [0, 1) is F.cross_entropy's label_smoothing.  sample_loss, loss and
 * d_logits (may be NULL) as nnue_cross_entropy.  NNUE_E_ARG, nothing launched: eps outside [0, 1), labels_b without lam. */
int nnue_cross_entropy_soft(const float* logits, const int64_t* labels, const int64_t* labels_b, const float* lam, float eps,
                            int B, int C, float grad_scale, float* sample_loss, float* loss, float* d_logits,
                            nnue_stream_t stream);

/* nnue_cross_entropy_soft (compute_loss, train.py:250-254) with the teacher arm defined under "soft targets": teacher
 * float32 [B][C], alpha in [0, 1], temperature > 0.  d_logits may be NULL; the loss values do not depend on it.  alpha == 0
 * is nnue_cross_entropy_soft (teacher may be NULL).  NNUE_E_ARG, nothing launched: alpha outside [0, 1], temperature not
 * finite or <= 0, teacher == NULL with alpha > 0, and the soft call's refusals. */
int nnue_cross_entropy_distill(const float* logits, const int64_t* labels, const int64_t* labels_b, const float* lam, float eps,
                               int B, int C, float grad_scale, float* sample_loss, float* loss, float* d_logits,
                               const float* teacher, float alpha, float temperature, nnue_stream_t stream);

/* Prediction bookkeeping of compute_metrics / evaluate_model (evaluate.py:23-59, :62-87): adds this batch to
 * confusion[truth*K + pred] (uint64, K = C, or 2 when C == 1).  pred = first arg-max of the row (numpy's
 * rule); C == 1 uses the reference's binary rule (output > 0.5, target > 0.5).  Accumulates: zero the matrix
 * once before the first batch.  Integer atomics: the result does not depend on execution order. */
int nnue_confusion_accumulate(const float* logits, const int64_t* labels, int B, int C,
                              uint64_t* confusion, nnue_stream_t stream);

/* ---- the compiled engine's integer inference, batched --------------------------------
 *
 * The quantised tensors of a `.nnue` file (layout: serialize.py:33-63, :103-136, :394-491; loader
 * engine/src/nnue_engine.cpp:544-657) in device memory, scalars by value.  The struct itself is read on the
 * host.  l1_w holds the (L2+1) x L1 bytes of the file (the last row is not used by the multiclass path);
 * l2_w is [L3][2*L2] (first L2 columns used). */
typedef struct nnue_engine_model {
  int32_t num_features, l1, l2, l3, classes, grid, oc;
  float conv_scale, threshold, quantized_one, l1_scale, l2_scale, out_scale;
  const int8_t* conv_w;  /* [oc*27], the file's bytes */
  const int32_t* conv_b; /* [oc] */
  const int16_t* ft_w;   /* [num_features][l1] */
  const int32_t* ft_b;   /* [l1] */
  const int8_t* l1_w;
  const int32_t* l1_b;
  const int8_t* l2_w;
  const int32_t* l2_b;
  const int8_t* out_w;   /* [classes][l3] */
  const int32_t* out_b;
} nnue_engine_model;

/* NNUEEvaluator::evaluate_logits (engine/src/nnue_engine.cpp:704-734) for B images at once -- what
 * evaluate_compiled_model obtains from one nnue_inference subprocess per image (evaluate.py:143-176,
 * engine/nnue_inference.cpp:42-60).  images: B flat buffers of 3*H*W floats, indexed HWC exactly as the engine
 * indexes them.  logits [B][classes], density [B] = active features / num_features.  Integer arithmetic
 * throughout: bit-identical to the engine.  Returns NNUE_E_SHAPE where the engine itself would write past its
 * grid buffer (conv map larger than grid x grid).  scratch >= nnue_engine_scratch(m, B) bytes. */
int64_t nnue_engine_scratch(const nnue_engine_model* m, int B);
int nnue_engine_evaluate_logits(const nnue_engine_model* m, const float* images, int B, int H, int W,
                                float* logits, float* density, void* scratch, int64_t scratch_bytes,
                                nnue_stream_t stream);

/* NNUEEvaluator::evaluate_incremental (engine/src/nnue_engine.cpp:739-786) for S independent streams at once (video: one
 * stream per camera, one call per frame), returning the multiclass logits of evaluate_logits as its consumer reads them
 * (evaluate.py:143-176).  Every stream keeps its wrapped int16 accumulator and its last active-feature set in `state`; a
 * step adds the table rows of the features that turned on and subtracts those that turned off
 * (FeatureTransformer::update_accumulator, nnue_engine.cpp:257-267), or refreshes from the bias (refresh_accumulator,
 * :806-816) when the stream is not valid or when that reads fewer rows.  The accumulator wraps mod 2^16, so every step's
 * logits and density are bit-identical to nnue_engine_evaluate_logits on the same frame, whatever the history.
 * Exactly one input: images (S flat buffers of 3*H*W floats, as nnue_engine_evaluate_logits; H x W may change between
 * steps; scratch >= nnue_engine_scratch(m, S) bytes) or active (uint8 [S][num_features], non-zero = on, every id counts;
 * scratch unused).  Outputs: logits [S][classes], density [S], changed [S] = features that differ from the stream's
 * previous set (all active features for a stream that was not valid).
 * state: 16-byte aligned, >= nnue_engine_stream_state_bytes(m, S) bytes; zero-filled = every stream fresh.  Its first S
 * int32 are the valid flags: writing 0 to one makes that stream refresh on its next step (the step sets it to 1).
 * NNUE_E_SCRATCH for too small a state or scratch; NNUE_E_SHAPE where num_features needs more LDS than a workgroup has. */
int64_t nnue_engine_stream_state_bytes(const nnue_engine_model* m, int S);
int nnue_engine_stream_step(const nnue_engine_model* m, const float* images, const uint8_t* active, int S, int H, int W,
                            void* state, int64_t state_bytes, float* logits, float* density, int32_t* changed,
                            void* scratch, int64_t scratch_bytes, nnue_stream_t stream);

/* ---- the engine's integer inference with the layer stack chosen per image -------------------------------------
 *
 * A `.nnue` file holds K layer stacks (serialize.py:394-491; loader engine/src/nnue_engine.cpp:619-635) and the engine takes a
 * layer_stack_index per call (nnue_engine.cpp:704-707; an index outside [0, K) means stack 0).  The calls below take all K
 * stacks, packed stack-major, and choose one per image: stack_in[b] when stack_in != NULL (outside [0, K) = stack 0), else
 *     stack[b] = min(K-1, n[b] * K / (num_features + 1)),   n[b] = the features the kernel counts as active
 * (the numerator of density[b]) -- the rule the bucketed model is trained with (nnue.bucket_of), applied to the engine's own
 * map, which is not the training map (ceil stride, HWC read, quantised conv), so the index may differ from the training one.
 * The struct is read on the host; `scales` is a HOST array (the scales reach the kernel by value in its arguments), every
 * other pointer is device memory.  No call copies between host and device or synchronises. */
typedef struct nnue_engine_stacks {
  int32_t count;        /* K, 1..64 (the range NNUE accepts) */
  const float* scales;  /* HOST [K][3]: l1_scale, l2_scale, out_scale -- validated like the single-stack scalars */
  const int8_t* l1_w;   /* stack-major: [K][(l2+1)*l1] */
  const int32_t* l1_b;  /* [K][l2+1] */
  const int8_t* l2_w;   /* [K][l3*2*l2] */
  const int32_t* l2_b;  /* [K][l3] */
  const int8_t* out_w;  /* [K][classes*l3] */
  const int32_t* out_b; /* [K][classes] */
} nnue_engine_stacks;

/* NNUEEvaluator::evaluate_logits with its layer_stack_index (engine/src/nnue_engine.cpp:704-734) for B images at once, the
 * index chosen per image as above -- what evaluate_compiled_model's per-image engine call (evaluate.py:143-176) would obtain
 * with that index.  Arguments, checks and results as nnue_engine_evaluate_logits, bit-identical to the engine stack by stack;
 * m supplies the conv, the table and the sizes, its own stack pointers and stack scales are not read.  stack_out [B] (device,
 * required) receives the stack each image used.  NNUE_E_ARG also for a null st, a count outside 1..64, a missing stack tensor
 * or a scale the single-stack call would refuse. */
int nnue_engine_evaluate_logits_stacks(const nnue_engine_model* m, const nnue_engine_stacks* st, const float* images,
                                       int B, int H, int W, const int32_t* stack_in, float* logits, float* density,
                                       int32_t* stack_out, void* scratch, int64_t scratch_bytes, nnue_stream_t stream);

/* NNUEEvaluator::evaluate_incremental (engine/src/nnue_engine.cpp:739-786) for S streams with the stack of every stream chosen
 * per step as above (from the step's new feature set; the logits are those its consumer reads, evaluate.py:143-176).
 * Arguments, checks and results as nnue_engine_stream_step; the state has the same layout and holds nothing about stacks, so
 * one state buffer may pass between the two calls from step to step.  stack_out [S] (device, required) receives the stack
 * each stream used.  NNUE_E_ARG also as nnue_engine_evaluate_logits_stacks. */
int nnue_engine_stream_step_stacks(const nnue_engine_model* m, const nnue_engine_stacks* st, const float* images,
                                   const uint8_t* active, int S, int H, int W, const int32_t* stack_in, void* state,
                                   int64_t state_bytes, float* logits, float* density, int32_t* changed, int32_t* stack_out,
                                   void* scratch, int64_t scratch_bytes, nnue_stream_t stream);

/* NNUEEvaluator::update_features(added, removed) (engine/src/nnue_engine.cpp:818-821, which runs
 * FeatureTransformer::update_accumulator, :257-267) for S streams at once on the state of nnue_engine_stream_step, followed by
 * the rest of evaluate_incremental (:739-786): the caller names the features that turned on and off instead of handing over the
 * whole new set, so a step costs O(changes), and gets the logits its consumer reads (evaluate.py:143-176).
 * Lists: CSR in device memory, int32 -- stream b adds added[added_off[b] .. added_off[b+1]) and removes
 * removed[removed_off[b] .. removed_off[b+1]); n_added, n_removed are the lengths of the id buffers.  Every range is clipped to
 * [0, n] and a reversed range is empty, so no offset can make the kernel read outside an id buffer.  A list with n == 0 may pass
 * NULL for both of its pointers.
 * Set semantics -- the stored set stays the true set and the accumulator bias + sum of rows(set) mod 2^16:
 *     new = (old \ removed) + added;
 * an id outside [0, num_features) is ignored (add_feature / remove_feature, :233-234), a removed id that is off and an added id
 * that is on are ignored, a duplicate within a list counts once, an id in both lists ends up on (it is removed first and added
 * again, which on a feature that was on nets to nothing mod 2^16).  On well-formed input -- added disjoint from the old set,
 * removed a subset of it, no duplicates -- this is update_accumulator bit for bit.  A stream that is not valid (fresh, or its
 * flag cleared) starts from the empty set and the bias and ignores `removed`: refresh_accumulator(added) (:806-816); the step
 * sets its flag.  rebuild != 0, for all streams: after the delta went into the bits, every accumulator is re-formed from the
 * bias and the rows of its new set and the stored sums are ignored -- for a table that changed under sets that are still right.
 * save_accumulator / restore_accumulator (:792-804) need no call: a copy of `state` is the whole stream.
 * st == NULL: m's own stack; else the stack of every stream is chosen as nnue_engine_stream_step_stacks chooses it, from the
 * new set's size (stack_in, stack_out as there; stack_out is required iff st).  Outputs as nnue_engine_stream_step: logits
 * [S][classes], density [S] = |new| / num_features, changed [S] = |new xor old| (|new| for a stream that was not valid).
 * The state keeps its layout; this call, nnue_engine_stream_step and nnue_engine_stream_step_stacks may follow one another in
 * any order on one buffer.  Checks and codes as those two; NNUE_E_ARG also for a negative n and for n > 0 with a NULL id or
 * offset pointer.  Every refusal comes before anything is launched. */
int nnue_engine_stream_update(const nnue_engine_model* m, const nnue_engine_stacks* st /* NULL: m's own stack */,
                              const int32_t* added, const int32_t* added_off, int64_t n_added,
                              const int32_t* removed, const int32_t* removed_off, int64_t n_removed,
                              int S, int rebuild, const int32_t* stack_in, void* state, int64_t state_bytes,
                              float* logits, float* density, int32_t* changed, int32_t* stack_out,
                              nnue_stream_t stream);

/* ---- the engine's integer inference as a matrix product (int8 matrix unit) --------------------------------------
 *
 * The accumulate step of the calls above, acc[b] = bias + sum of the table rows of b's active features taken mod 2^16
 * (FeatureTransformer, engine/src/nnue_engine.cpp:236-283 of the header, :726-729), is the product of the 0/1 feature map
 * [B][F] with the int16 table [F][L1].  Integer addition mod 2^16 depends neither on the order of the terms nor on the width of
 * the accumulator, so int32 sums truncated to int16 are the engine's wrapped sums bit for bit, and the table splits exactly into
 * int8 planes: lo = (int8)(w & 0xff), hi = (int8)((w - lo) >> 8), sum(lo) + 256 * sum(hi) == sum(w) (mod 2^16).  A table the
 * serialiser wrote is clamped to +-127 (serialize.py:218-222) and needs the lo plane only.
 * nnue_engine_matrix_supported: 1 where nnue_engine_evaluate_logits_matrix can run (planes 1 or 2, num_features < 2^24 so that
 * no int32 sum of int8 products can overflow, layer sizes inside a workgroup's LDS), else 0; never launches.
 * nnue_engine_table_planes_bytes: size of the packed planes (num_features and L1 padded to the product's tiles).
 * nnue_engine_matrix_scratch: >= nnue_engine_scratch(m, B): the conv bytes and the int32 sums [B][L1]. */
int nnue_engine_matrix_supported(const nnue_engine_model* m, int B, int planes);
int64_t nnue_engine_table_planes_bytes(const nnue_engine_model* m, int planes);
int64_t nnue_engine_matrix_scratch(const nnue_engine_model* m, int B, int planes);

/* Packs m->ft_w (int16 [F][L1], the file's table: serialize.py:103-136; the engine reads it as
 * engine/src/nnue_engine.cpp:236-283 adds its rows) into `planes` int8 planes in the layout the product reads, lo then hi,
 * zero-padded, in one streaming launch: no host copy, no synchronisation.  table_planes: device, 16-byte aligned,
 * bytes >= nnue_engine_table_planes_bytes(m, planes).  planes == 1: an element outside [-128, 127] is packed as its low byte and
 * ADDED to misfit[0] (device int32; the caller zeroes it), one atomic per wave that saw any; planes == 2 leaves misfit alone.
 * NNUE_E_ARG: null or misaligned pointer; NNUE_E_SHAPE: planes outside {1, 2}, L1 outside 2..2048, num_features >= 2^24;
 * NNUE_E_SCRATCH: bytes too small. */
int nnue_engine_pack_table(const nnue_engine_model* m, int planes, void* table_planes, int64_t bytes, int32_t* misfit,
                           nnue_stream_t stream);

/* NNUEEvaluator::evaluate_logits (engine/src/nnue_engine.cpp:704-734) for B images at once -- the logits
 * evaluate_compiled_model's per-image engine call obtains (evaluate.py:143-176) -- with the accumulate step on the int8 matrix
 * unit; bit-identical to nnue_engine_evaluate_logits / nnue_engine_evaluate_logits_stacks.  st == NULL: m's own stack; else the
 * stack of every image is chosen as nnue_engine_evaluate_logits_stacks chooses it (stack_in, stack_out as there; stack_out is
 * required iff st).  table_planes, planes: what nnue_engine_pack_table wrote for m->ft_w as it is now.
 * Exactly one input, as nnue_engine_stream_step: images (B flat buffers of 3*H*W floats; a feature is on under the gather
 * call's rule, conv byte > threshold and channel < 64) or active (uint8 [B][num_features], non-zero = on, every id counts; H, W
 * and the conv part of the scratch are unused).  density[b] = the image's active count / num_features, counted once per image.
 * scratch: 4-byte aligned, >= nnue_engine_matrix_scratch(m, B, planes) bytes.  Where the (B, L1) tile grid leaves CUs idle the
 * features are split over workgroups and the int32 partial sums meet by integer atomics in sums zeroed on `stream`: the same
 * bits for any split.  Codes as the gather calls; NNUE_E_SHAPE also where nnue_engine_matrix_supported is 0. */
int nnue_engine_evaluate_logits_matrix(const nnue_engine_model* m, const nnue_engine_stacks* st, const void* table_planes,
                                       int planes, const float* images, const uint8_t* active, int B, int H, int W,
                                       const int32_t* stack_in, float* logits, float* density, int32_t* stack_out,
                                       void* scratch, int64_t scratch_bytes, nnue_stream_t stream);

/* ---- the engine's integer inference from uint8 frames -------------------------------------------------------------
 *
 * Every source of images is uint8 -- the dataset store of nnue_load_batch ([N][H][W][3]), a camera's frames -- and the engine's
 * first act on a float is q = (int32)(x * conv_scale) (ConvLayer::forward, engine/src/nnue_engine.cpp:48-158).  The calls below
 * take the bytes themselves: a frame is 3*H*W uint8 u[0 .. 3HW), HWC, and stands for the flat float buffer x[0 .. 3HW) the
 * engine indexes HWC,
 *     layout 0 (chw)  x[i] = norm(u[(i mod HW)*3 + i div HW], i div HW) -- the memory nnue_load_batch(augment = 0) writes for the
 *                     image, a CHW tensor, handed to the engine flat as the reference hands it (evaluate.py:150-161): the
 *                     reference's compiled metric, quirk included;
 *     layout 1 (hwc)  x[i] = norm(u[i], i mod 3) -- the frame is what the engine's indexing means;
 *     norm(v, c) = ((float)v - mean255[c]) * inv_std255[c] in float32, in this order (A.Normalize, data/datasets.py:366-369),
 *     mean255[c] = mean[c] * 255.0f and inv_std255[c] = 1.0f / (std[c] * 255.0f) formed by the caller in float32; with the
 *     ImageNet constants they are nnue_load_batch's own, bit for bit.
 * From x on everything is the float call: with layout 0 and those constants a u8 call is bit-identical to its float twin on
 * nnue_load_batch(augment = 0) of the same indices -- logits, density, changed and the stacks used.  The float batch is never
 * written: the front forms the 768 possible q once per workgroup by the expression above and the conv is integer arithmetic.
 * The struct is read on the host; data and indices are device memory.  indices[b] is clamped to [0, count) as nnue_load_batch
 * clamps it; without indices frame b is data + b*3*H*W.  No load touches a byte outside [data, data + count*3*H*W). */
typedef struct nnue_engine_u8_frames {
  const uint8_t* data;    /* device: count frames of 3*H*W bytes, HWC; any byte alignment */
  const int64_t* indices; /* device [B] into data, or NULL: frame b is data + b*3*H*W (then count >= B) */
  int64_t count;          /* frames in data, >= 1 */
  int32_t layout;         /* 0 chw (the memory nnue_load_batch writes), 1 hwc */
  float mean255[3], inv_std255[3];
} nnue_engine_u8_frames;

/* NNUEEvaluator::evaluate_logits (engine/src/nnue_engine.cpp:704-734) for B uint8 frames -- the logits
 * evaluate_compiled_model's per-image engine call obtains (evaluate.py:150-161) on Normalize's output (data/datasets.py:366-369)
 * -- with the conv (nnue_engine.cpp:48-158) read from the bytes as defined above.  st == NULL: m's own stack, as
 * nnue_engine_evaluate_logits; else per-image selection as nnue_engine_evaluate_logits_stacks (stack_in, stack_out as there;
 * stack_out required iff st).  scratch >= nnue_engine_scratch(m, B).  Checks and codes as those two calls; NNUE_E_ARG also for a
 * null src or src->data, a layout outside {0, 1}, count < 1, count < B without indices, a constant that is not finite,
 * inv_std255 <= 0, and constants under which a byte times m->conv_scale leaves int32; NNUE_E_SHAPE also where the source rows
 * of one output row exceed a workgroup's LDS (frames wider than about 1700 pixels) or a frame holds 2^31 bytes.  No call copies
 * between host and device, allocates or synchronises; fit for stream capture. */
int nnue_engine_evaluate_logits_u8(const nnue_engine_model* m, const nnue_engine_stacks* st /* NULL: m's own stack */,
                                   const nnue_engine_u8_frames* src, int B, int H, int W, const int32_t* stack_in,
                                   float* logits, float* density, int32_t* stack_out, void* scratch, int64_t scratch_bytes,
                                   nnue_stream_t stream);

/* nnue_engine_evaluate_logits_matrix (NNUEEvaluator::evaluate_logits, engine/src/nnue_engine.cpp:704-734; evaluate.py:150-161)
 * with the conv bytes formed from uint8 frames (nnue_engine.cpp:48-158 on Normalize's output, data/datasets.py:366-369) as
 * nnue_engine_evaluate_logits_u8 forms them; the product and the tail are the float twin's launches.  table_planes, planes,
 * scratch (>= nnue_engine_matrix_scratch(m, B, planes), 4-byte aligned) and codes as the float twin, src and its refusals as
 * nnue_engine_evaluate_logits_u8. */
int nnue_engine_evaluate_logits_matrix_u8(const nnue_engine_model* m, const nnue_engine_stacks* st, const void* table_planes,
                                          int planes, const nnue_engine_u8_frames* src, int B, int H, int W,
                                          const int32_t* stack_in, float* logits, float* density, int32_t* stack_out,
                                          void* scratch, int64_t scratch_bytes, nnue_stream_t stream);

/* NNUEEvaluator::evaluate_incremental (engine/src/nnue_engine.cpp:739-786) for S streams whose frames arrive as uint8: the
 * step of nnue_engine_stream_step / nnue_engine_stream_step_stacks (st == NULL / given) on the conv bytes formed from src
 * (nnue_engine.cpp:48-158 on Normalize's output, data/datasets.py:366-369; the logits its consumer reads, evaluate.py:150-161).
 * Same state, same outputs; this call and every other stream call may follow one another on one state buffer.  scratch >=
 * nnue_engine_scratch(m, S).  Codes as the float twin, src and its refusals as nnue_engine_evaluate_logits_u8. */
int nnue_engine_stream_step_u8(const nnue_engine_model* m, const nnue_engine_stacks* st, const nnue_engine_u8_frames* src,
                               int S, int H, int W, const int32_t* stack_in, void* state, int64_t state_bytes,
                               float* logits, float* density, int32_t* changed, int32_t* stack_out, void* scratch,
                               int64_t scratch_bytes, nnue_stream_t stream);

/* nnue_engine_stream_step_u8 from the dirty rectangles of the frames: NNUEEvaluator::evaluate_incremental /
 * update_features (engine/src/nnue_engine.cpp:739-786, :818-821) with the added and removed feature lists derived on the device
 * from the pixels -- the conv (nnue_engine.cpp:48-158 on Normalize's output, data/datasets.py:366-369; the logits its consumer
 * reads, evaluate.py:150-161) is re-run only on the grid cells a rectangle touches, and only the table rows that flipped are
 * walked.  A step costs O(touched cells + flips) per stream and needs no scratch.
 * Rectangles: CSR in device memory, int32 -- stream s owns rects[rect_off[s] .. rect_off[s+1]), each y0, x0, y1, x1, half-open,
 * in frame pixels; n_rects is the number of rectangles in the buffer.  Every range is clipped to [0, n_rects] and a reversed
 * range is empty, as the ranges of nnue_engine_stream_update; with n_rects == 0 both pointers may be NULL.
 * Definition, as set arithmetic.  Geometry is the engine's: stride = ceil((H-1)/(grid-1)), OH = (H-1)/stride + 1, OW =
 * (W-1)/stride + 1; cell (oh, ow) reads frame rows oh*stride-1 .. oh*stride+1 and columns ow*stride-1 .. ow*stride+1, zero
 * padding outside the frame.  For stream s let cells(s) be the cells whose window meets any of its rectangles, each rectangle
 * first clipped to [0,H) x [0,W).  For every such cell and every channel c < oc, feature (oh*OW + ow)*oc + c takes the value
 * nnue_engine_stream_step_u8 would give it on this frame (the same 768-entry table, taps, truncating division, clamp, and
 * (float)(int8)q > threshold && c < 64); every other bit of the stream's stored set keeps its value.  The accumulator, logits,
 * density = |new| / num_features, changed = |new xor old| and the stack choice follow as in the other stream calls.
 * Hence: if the frame differs from the one behind the stored set only inside the rectangles -- same H x W, layout, constants and
 * model tensors -- every output is bit-identical to nnue_engine_stream_step_u8 on the whole frame.  That condition is the
 * caller's promise; breaking it is not undefined behaviour, the result is the set arithmetic above.
 * Overlapping and repeated rectangles are harmless; an empty or inverted rectangle, and one wholly outside the frame, select
 * nothing; a stream without rectangles returns its unchanged logits with changed == 0.  A stream that is not valid ignores its
 * rectangles: it is evaluated over the whole frame from the empty set and the bias, as the whole-frame step evaluates it, and
 * becomes valid.  Only src->layout == 1 (hwc) is accepted: under chw a pixel rectangle does not map to neighbouring taps
 * (NNUE_E_ARG).  The state keeps its layout; this call and every other stream call may follow one another on one buffer.
 * No scratch, no allocation, no host-device copy, no synchronisation: fit for stream capture.  Checks and codes as
 * nnue_engine_stream_step_u8 and nnue_engine_stream_update (stack_out required iff st); NNUE_E_ARG also for n_rects < 0 and for
 * n_rects > 0 with a NULL rects or rect_off; NNUE_E_SHAPE where the kernel's LDS (that of nnue_engine_stream_update plus the
 * table) exceeds 64 KB or a frame holds 2^31 bytes.  Every refusal comes before anything is launched. */
int nnue_engine_stream_step_u8_regions(const nnue_engine_model* m, const nnue_engine_stacks* st /* NULL: m's own stack */,
                                       const nnue_engine_u8_frames* src, int S, int H, int W,
                                       const int32_t* rects /* device [n_rects][4]: y0, x0, y1, x1, half-open, frame pixels */,
                                       const int32_t* rect_off /* device [S + 1], CSR over rects */, int64_t n_rects,
                                       const int32_t* stack_in, void* state, int64_t state_bytes,
                                       float* logits, float* density, int32_t* changed, int32_t* stack_out, nnue_stream_t stream);

/* ---- the engine's tensors from a live model ------------------------------------------------------------------------
 *
 * What serialize_model followed by a load of the file leaves in device memory, formed from the model's float32 parameters in
 * ONE launch, without the file, a host copy or a change to the parameters (the reference's training loop quantises through the
 * file after every epoch: train.py:389-421).  Sources (device float32, any 4-byte aligned view): conv_w [oc][3][3][3], ft_w
 * [F][L1], ft_b [L1], and the classifier's w1 [K][L2][L1], b1 [K][L2], w2 [K][L3][L2], b2 [K][L3], w3 [K][C][L3], b3 [K][C]
 * (K = 1: the reference's SimpleClassifier).  Destination: the tensors of `dst` -- conv_w in the source's flat order, ft_w int16
 * [F][L1] (16-byte aligned), ft_b -- and the six stack tensors with the engine's padding (serialize.py:423-491): l1_w
 * [L2+1][L1] with a zero last row, l1_b [L2+1] with a zero last element, l2_w [L3][2*L2] with a zero second half of every row,
 * l2_b, out_w [C][L3], out_b.  dst_stacks != NULL (count == K): all K stacks, stack-major, into its tensors; dst's own stack
 * pointers are not read.  dst_stacks == NULL: stack `stack` (in [0, K)) into dst's own stack tensors.  conv_b and every scalar of
 * the structs are the caller's (the reference's conv has no bias: its quantised bias is zero).
 * Arithmetic, element for element the serialiser's (serialize.py:218-222, :234-237 after the clamp of nnue.py:528-539):
 *     weight: clamp(round_half_even(w * 64), -127, 127) with w first clamped to [-1, 1] -- in registers, the source is never
 *             written -- except the conv's, which is not clamped;      bias: round_half_even(b * 64) as int32, unclamped;
 * w * 64 is the float32 product, the rounding rintf.  A source element that is not finite, and a bias whose scaled value int32
 * cannot hold, is written as 0 and ADDED to bad_count[0] (device int32; the caller zeroes it), one atomic per wave that saw any.
 * NNUE_E_ARG: null pointer, K outside 1..64, a non-positive size, stack outside [0, K), a missing destination tensor, a
 * misaligned pointer; NNUE_E_SHAPE: odd L1, sizes of dst (or the count of dst_stacks) that differ from the arguments. */
int nnue_engine_quantize_model(const float* conv_w, const float* ft_w, const float* ft_b, const float* w1, const float* b1,
                               const float* w2, const float* b2, const float* w3, const float* b3,
                               int oc, int F, int L1, int L2, int L3, int C, int K, int stack,
                               const nnue_engine_model* dst, const nnue_engine_stacks* dst_stacks,
                               int32_t* bad_count, nnue_stream_t stream);

/* Data parallel for bandwidth-sized tables ("exchange only touched rows"; the reference itself is single-device,
 * train.py:263).  The table's weight gradient of the GLOBAL batch is d_W = A^T D with A the {0,1} map [world*B][P] and
 * D = d_ft [world*B][L1]: the ranks all-gather those FACTORS (the map as one bit per position) instead of reducing the
 * F x L1 product (1.5 MB per rank instead of 269 MB at the 224x224 configuration), and every rank runs the single-rank fused
 * path on them (nnue_ftm_gram_sqnorm, nnue_sgd_step, nnue_ftm_backward_weight_update with B = world*B): the gradient of the
 * mean loss over the global batch and clip_grad_norm_ on its global norm (train.py:359-366), identical on every rank.
 * One rank's chunk of the all-gather (byte offsets from nnue_dp_factor_offset, which = 0 d_ft, 1 sink, 2 small, 3 bits):
 *     d_ft [B][L1] f32 | sink [B] f32 | small [small_count] f32 | map bits [B][ceil(P/128)*16] (bit k of byte j = position 8j+k)
 * d_ft and sink are written in place by their producers (the trainer's buffers are views of its own chunk).
 * nnue_dp_factor_pack fills the bits from the byte map and "small" with every gradient the product does not cover:
 * grads[0, head_count) ++ grads[tail_lo, tail_lo + tail_count) of the flat gradient buffer (threshold and conv weight;
 * table rows >= direct, bias, classifier).  nnue_dp_factor_unpack takes the world gathered chunks (rank-major) and leaves
 * the global byte map g_bits [world*B][P], g_sink [world*B], g_dft [world*B][L1], and in grads the SUM of the ranks' small
 * parts in rank order (the all-reduce of the small gradients as a deterministic reduction: one collective per step).
 * P and L1 multiples of 4; all pointers 16-byte aligned. */
int64_t nnue_dp_factor_chunk_bytes(int B, int P, int L1, int64_t small_count);
int64_t nnue_dp_factor_offset(int which, int B, int P, int L1, int64_t small_count);
int nnue_dp_factor_pack(const uint8_t* bits, const float* grads, int64_t head_count, int64_t tail_lo, int64_t tail_count,
                        int B, int P, int L1, void* chunk, nnue_stream_t stream);
/* (train.py:359-366 over the global batch, see above) */
int nnue_dp_factor_unpack(const void* chunks, int world, int B, int P, int L1, int64_t head_count, int64_t tail_lo,
                          int64_t tail_count, uint8_t* g_bits, float* g_sink, float* g_dft, float* grads, nnue_stream_t stream);

/* The first stage of the clip norm below, alone: nparts block partials of sum g^2 (unscaled, fixed order) -- what a rank contributes
 * when the clip norm of clip_grad_norm_ (train.py:363-364) spans gradient shards held by different ranks: the partials are
 * all-gathered and handed to every rank's nnue_sgd_step as ext_partial over its whole shard. */
int nnue_sqnorm_partials(const float* grads, int64_t count, float* partial, int nparts, nnue_stream_t stream);

/* clip_grad_norm_ + SGD(momentum, weight_decay) on flat buffers (train.py:363-366, :457-464):
 *   g <- g * grad_scale              (1/world after a summed all-reduce)
 *   norm = ||g||_2 ; c = min(1, max_norm/(norm+1e-6)) if max_norm > 0 else 1
 *   g <- c*g + wd*p ; m <- first_step ? g : momentum*m + g ; p <- p - lr*m
 * norm_out (device float, may be NULL) receives the pre-clip norm.  Deterministic
 * two-stage norm; scratch >= nnue_sgd_scratch(count) bytes.
 * ste_partial != NULL: the second stage of a deferred nnue_ste_conv_backward (stages = 1; nnue.py:28-54) runs as extra
 * workgroups of the norm launch: d_thr[c] / d_weight[c*27+q] are summed from ste_partial (same order as stage 2, same
 * bits), written, and enter the norm.  ste_d_thr and ste_d_weight must lie in grads and together form its first
 * elements (a multiple of 4 of them); ste_fps * 28 <= 4096.  All five are NULL / 0 otherwise.
 * ext_partial != NULL: ext_count sums of squares (unscaled) that a producer formed for grads[ext_lo, ext_hi) (multiples of
 * 4, e.g. nnue_ftm_backward's sq_partial for the FeatureTransformer weight rows): the norm launch skips that range and
 * the partials enter the norm in index order, multiplied by grad_scale^2.  ext_count <= 65536.
 * coef_out != NULL: the clip coefficient c is also left in that device float.  ext_applied_elsewhere != 0 (needs
 * ext_partial and coef_out): grads[ext_lo, ext_hi) does not exist -- its producer applies the update itself afterwards
 * (nnue_ftm_backward_weight_update, reading coef_out) -- so this call neither reads that range of grads nor touches that
 * range of params / momentum_buf.
 * lr_dev != NULL (here, in nnue_adam_step and in nnue_ftm_backward_weight_update): the learning rate is read from that device
 * float instead of the `lr` argument -- an optimizer's lr changes between steps (a scheduler stepping param_groups, the
 * counterpart of train.py:457-471's optimizers) without re-recording or re-capturing a step that was captured into a graph. */
int64_t nnue_sgd_scratch(int64_t count);
int nnue_sgd_step(float* params, float* grads, float* momentum_buf, int64_t count,
                  float lr, float momentum, float weight_decay, float max_norm, float grad_scale,
                  int first_step, float* norm_out, void* scratch, int64_t scratch_bytes,
                  const float* ste_partial, int ste_chunks, int ste_fps,
                  float* ste_d_thr, float* ste_d_weight,
                  const float* ext_partial, int ext_count, int64_t ext_lo, int64_t ext_hi,
                  float* coef_out, int ext_applied_elsewhere, const float* lr_dev, nnue_stream_t stream);

/* One step of a per-iteration learning-rate schedule, on the device, so that it can sit inside a captured step graph ahead of
 * the optimizer launches that read lr_dev.  The reference fixes the rate when it builds its optimizers (train.py:457-471) and
 * defines the per-iteration schedule its configs ask for in training_utils.py:283-336 (get_lr: warm-up, cosine decay, cyclical
 * modulation); `table` holds that schedule -- or any other -- tabulated on the host, n float32 values, one per optimizer step.
 *   i = clamp(position[0], 0, n-1) ; lr_out[0] = table[i] ; position[0] = min(position[0] + 1, INT32_MAX)
 * (past the end of the table the last value holds; the counter saturates, it never wraps).  One launch of one wavefront;
 * table, position and lr_out are device pointers.  NNUE_E_ARG: a null pointer, n <= 0 or n > INT32_MAX; nothing is launched
 * then. */
int nnue_lr_schedule_step(const float* table, int64_t n, int32_t* position, float* lr_out, nnue_stream_t stream);

/* ---- input pipeline ------------------------------------------------------------------------------
 * One batch of GenericVisionDataset.__getitem__ + collate (data/datasets.py:173-195, :358-372) from a uint8
 * dataset resident in HBM: images_u8 [N,H,W,3], labels_all [N]; indices [B] select the samples.  Writes
 * out [B,3,H,W] float32 = Normalize(ImageNet mean/std, max 255) of the (optionally augmented) pixels, CHW, and
 * labels_out [B].  augment != 0 applies the reference's "light" policy: HorizontalFlip p=0.5,
 * RandomBrightnessContrast(0.1, 0.1) p=0.2 (uint8 LUT semantics), CoarseDropout (one 5% x 5% hole, fill 0)
 * p=0.2.  Random draws are a counter-based hash of (seed, step, dataset index): reproducible, but not
 * albumentations' stream (parity unpinned for augment != 0; the plain path is an exact formula). */
int nnue_load_batch(const uint8_t* images_u8, const int64_t* labels_all, const int64_t* indices,
                    int B, int H, int W, int64_t N, int augment, uint64_t seed, uint64_t step,
                    float* out, int64_t* labels_out, nnue_stream_t stream);

/* nnue_load_batch with a policy and a resize: the reference's augmentation_strength (data/datasets.py:173-195 "light",
 * :301-350 "medium", the default) and the A.Resize(target_size) that closes every transform list (data/datasets.py:357-361),
 * then Normalize + ToTensorV2 (:364-371).  out is [B,3,Ho,Wo]; one launch, no scratch.  policy: 0 = none (resize only),
 * 1 = light, 2 = medium; anything else is NNUE_E_ARG.  H*W and Ho*Wo below 2^24, at most 65535 tiles of 16 x 16 output
 * pixels (NNUE_E_SHAPE).  nnue_load_batch_params_count() = P, the floats per image of params_out.
 *
 * Draws: base = mix64(seed ^ mix64(index*C + step)), draw k = u01(mix64(base + k)) as nnue_load_batch.  Policy 1 uses draws
 * 1..7 exactly as nnue_load_batch does (sizes taken from Ho x Wo) and its arithmetic (floor to uint8 levels included): at
 * Ho == H, Wo == W it equals nnue_load_batch(augment = 1) bit for bit, and policy 0 equals augment = 0.  Policy 2 uses draws
 * 16..43; per-pixel noise hashes mix64(base + 2^32 + (oy*Wo + ox)*3 + c).
 *
 * Geometry: the fired geometric stages and the resize compose into ONE map from output pixel (ox, oy) to source pixel
 *   sx = m0*ox + m1*oy + m2 ; sy = m3*ox + m4*oy + m5
 * and the source is sampled once, bilinearly.  From the output side: Affine^-1, Rotate^-1, Rot90^-1, Flip^-1, then the
 * resize map s = (o + 0.5)*(src/dst) - 0.5.  With c = ((Wo-1)/2, (Ho-1)/2) and R(t) = [[cos t, -sin t], [sin t, cos t]]:
 *   Affine^-1: p -> c + R(-angle)(p - c - (tx, ty)) / scale      Rotate^-1: p -> c + R(angle)(p - c)
 *   Rot90^-1 (k quarter turns, on the Ho x Wo rectangle through u = (x+0.5)/Wo, v = (y+0.5)/Ho):
 *     k = 1: (u, v) -> (1 - v, u) ; k = 2: (1 - u, 1 - v) ; k = 3: (v, 1 - u)            Flip^-1: x -> Wo - 1 - x
 * If Rotate or Affine fired, a tap outside the source reads 0 (albumentations' constant fill); otherwise the sample
 * coordinate is clamped into the image (cv2.resize).  albumentations resamples once per stage and rounds to uint8 between
 * stages; this samples once and keeps float levels in [0, 255] throughout -- stated differences.
 *
 * Policy 2, in this order (probabilities and ranges of data/datasets.py:303-339):
 *   1 HorizontalFlip p=.5   2 RandomRotate90 p=.5, k uniform in 0..3   3 Rotate p=.3, +-15 deg
 *   4 Affine p=.3: translate +-10 % of each output side, isotropic scale .9..1.1, rotate +-15 deg
 *   5 RandomBrightnessContrast p=.3: clamp(v*alpha + beta*255), alpha-1 and beta in +-.2
 *   6 HueSaturationValue p=.3 in float HSV (H degrees, S and V in [0,1], H = 0 where max == min): H + 2*shift (+-10, wraps),
 *     S + shift/255 (+-15, clamped), V + shift/255 (+-10, clamped)
 *   7 OneOf blur p=.2, kind uniform: 0 box 3x3, 1 Gaussian 3x3 with sigma in [.5, 3] (weights exp(-d^2/(2 sigma^2)),
 *     normalised, separable), 2 motion: the 3-tap line through the centre in direction 0 '-', 1 '|', 2 '\', 3 '/'; the
 *     neighbours are stage 1-6 values, reflect-101 at the OUTPUT image's borders
 *   8 GaussNoise p=.2: sigma in [.01, .05]*255, Box-Muller z = sqrt(-2 ln u1) cos(2 pi u2) per pixel and channel, clamped
 *   9 CoarseDropout p=.3: one hole, each side uniform in [.05, .15] of the output side (>= 1 pixel), uniform position, fill 0
 * Omitted from the medium list (each p <= .2): RandomShadow, RandomFog, GridDistortion, ElasticTransform, CLAHE, ColorJitter,
 * Posterize, Equalize.  "heavy" (medium plus a second pass of stronger stages) is not built.
 *
 * params_out (may be NULL) receives per image what was drawn, P = 32 floats (values are recorded whether or not their stage
 * fired; policy 0/1 leave the unused ones at their neutral value):
 *   [0] stage flags: 1 flip, 2 rot90, 4 rotate, 8 affine, 16 brightness/contrast, 32 HSV, 64 blur, 128 noise, 256 dropout
 *   [1] k   [2] Rotate angle (deg)   [3] Affine angle (deg)   [4] Affine scale   [5] tx   [6] ty (output pixels)
 *   [7..12] m0..m5, the composed map as the kernel used it   [13] alpha   [14] beta
 *   [15] hue shift   [16] saturation shift   [17] value shift   [18] blur kind   [19] Gaussian sigma   [20] motion direction
 *   [21] noise sigma (levels)   [22] hole y0   [23] hole x0   [24] hole height   [25] hole width   [26..31] 0 */
int nnue_load_batch_policy(const uint8_t* images_u8, const int64_t* labels_all, const int64_t* indices,
                           int B, int H, int W, int64_t N, int Ho, int Wo, int policy, uint64_t seed, uint64_t step,
                           float* out, int64_t* labels_out, float* params_out, nnue_stream_t stream);
int nnue_load_batch_params_count(void);

/* Batch-level mixing (build extension): one stage behind the per-image transform list (data/datasets.py:301-350) and the
 * collate (data/loaders.py:95-120), in place on images [B,3,H,W] float32.  Sample i is paired with j = B-1-i; one thread
 * reads an element of both and writes both; for odd B the middle sample keeps itself.  One draw per batch (host
 * arguments):
 *   mode 1, mixup:  x_i' = lam x_i + (1-lam) x_j and x_j' = lam x_j + (1-lam) x_i, both from the original values;
 *                   lam_out = lam (in [0, 1])
 *   mode 2, CutMix: inside the box [y0, y0+hh) x [x0, x0+hw) (inside the image; hh or hw may be 0) the two samples swap
 *                   pixels, a bitwise select; lam_out = (float)(H*W - hh*hw) / (float)(H*W)
 *   mode 0:         the images are left alone, lam_out = 1
 * In every mode labels_b_out[i] = labels[B-1-i] and lam_out[i] is the value above: what the soft-target entry points take
 * beside labels.  labels_b_out must not overlap labels.  NNUE_E_ARG, nothing launched: a null pointer, non-positive sizes,
 * another mode, lam outside [0, 1] (mode 1), a box that leaves the image (mode 2). */
int nnue_mix_batch(float* images, const int64_t* labels, int B, int H, int W, int mode, float lam, int y0, int x0, int hh,
                   int hw, int64_t* labels_b_out, float* lam_out, nnue_stream_t stream);

/* clip_grad_norm_ + torch.optim.Adam(lr, weight_decay) on flat buffers -- the optimizer create_optimizer picks
 * when optimizer_type != "sgd" (train.py:363-366, :465-470; torch defaults betas (0.9, 0.999), eps 1e-8, L2
 * weight decay added to the gradient, no amsgrad):
 *   g <- clip * grad_scale * g + wd * p ; m <- b1 m + (1-b1) g ; v <- b2 v + (1-b2) g^2
 *   p <- p - lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * t = ++step_counter[0] is kept in device memory so the call takes no per-step host argument (hipGraph replay).
 * scratch >= nnue_sgd_scratch(count) bytes; norm_out may be NULL. */
int nnue_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int32_t* step_counter,
                   int64_t count, float lr, float beta1, float beta2, float eps, float weight_decay,
                   float max_norm, float grad_scale, float* norm_out,
                   void* scratch, int64_t scratch_bytes, const float* lr_dev, nnue_stream_t stream);

/* nnue_adam_step with what nnue_sgd_step offers a producer of part of the gradient (clip_grad_norm_ + Adam, train.py:363-366,
 * :465-470; the arithmetic and the step counter of nnue_adam_step): ext_partial / ext_count / ext_lo / ext_hi / coef_out /
 * ext_applied_elsewhere exactly as there -- the norm launch skips grads[ext_lo, ext_hi) and takes that range's share from the
 * producer's partials (nnue_ftm_gram_sqnorm), the clip coefficient is left in coef_out, and with ext_applied_elsewhere the
 * apply pass touches neither params nor the moments in that range (nnue_ftm_backward_weight_update_adam applies it, reading
 * coef_out and step_counter).  The counter is advanced once, by the norm launch. */
int nnue_adam_step_ext(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int32_t* step_counter,
                       int64_t count, float lr, float beta1, float beta2, float eps, float weight_decay,
                       float max_norm, float grad_scale, float* norm_out, void* scratch, int64_t scratch_bytes,
                       const float* ext_partial, int ext_count, int64_t ext_lo, int64_t ext_hi,
                       float* coef_out, int ext_applied_elsewhere, const float* lr_dev, nnue_stream_t stream);

/* clip_grad_norm_ + SGD(momentum, weight_decay) over a LIST of n separate tensors -- torch.optim's parameter list with its
 * param groups, as the reference's loop steps it (train.py:363-366; the optimizer of create_optimizer, train.py:455-471):
 * segment i is params[i] / grads[i] / momentum_bufs[i], counts[i] > 0 elements, with its own lr[i], momentum[i],
 * weight_decay[i] and first_step[i] (no momentum buffer yet: it is written, not read).  The norm is the global one over all
 * segments; per element the arithmetic of nnue_sgd_step (grad_scale 1):
 *   c = min(1, max_norm/(norm+1e-6)) if max_norm > 0 else 1 ; g <- c*g + wd*p ; m <- first ? g : momentum*m + g ; p <- p - lr*m
 * momentum[i] == 0: momentum_bufs may be NULL or hold NULL there, and nothing is written to it.
 * The arrays are HOST arrays (pointers to device memory, counts and hyperparameters); the call packs them into kernel-argument
 * tables of 45 segments, so a step has no host-to-device copy and launches 2 kernels per 45 segments (1 without a norm).
 * Any sizes, any 4-byte-aligned views: 16-byte accesses where the segment's pointers share their offset within 16 bytes.
 * The norm is summed in fixed-size chunks in list order and re-derived in double: two runs give the same bits whatever the
 * pointers.  scratch >= nnue_multi_optim_scratch(counts, n) bytes (0 on invalid arguments).  norm_out (device float, may be
 * NULL) receives the pre-clip norm -- what clip_grad_norm_ returns.  lr_dev (may be NULL): n device floats that replace lr[]. */
int64_t nnue_multi_optim_scratch(const int64_t* counts, int n);
int nnue_multi_sgd_step(float* const* params, float* const* grads, float* const* momentum_bufs, const int64_t* counts, int n,
                        const float* lr, const float* momentum, const float* weight_decay, const int32_t* first_step,
                        float max_norm, float* norm_out, void* scratch, int64_t scratch_bytes, const float* lr_dev,
                        nnue_stream_t stream);

/* clip_grad_norm_ + Adam(lr, betas, eps, weight_decay) over a list of n separate tensors (train.py:363-366, :455-471; torch's
 * L2 weight decay, no amsgrad): segment i carries exp_avgs[i], exp_avg_sqs[i] and its own step counter step_counters[i]
 * (one device int32 per tensor, so a tensor that skips a step keeps its own count), with lr[i], beta1[i], beta2[i], eps[i],
 * weight_decay[i].  The norm launch advances every listed counter by one; per element the arithmetic of nnue_adam_step at
 * that segment's t.  Tables, alignment, scratch, norm_out and lr_dev as nnue_multi_sgd_step. */
int nnue_multi_adam_step(float* const* params, float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                         int32_t* const* step_counters, const int64_t* counts, int n, const float* lr, const float* beta1,
                         const float* beta2, const float* eps, const float* weight_decay, float max_norm, float* norm_out,
                         void* scratch, int64_t scratch_bytes, const float* lr_dev, nnue_stream_t stream);

/* ---- weight clip (build extension: the export range held during training) ----------------------------------------------
 * The reference's export (serialize.py:508-510 -> NNUE.get_quantized_model_data -> NNUE._clip_weights, nnue.py:528-539) clamps
 * input.weight and the classifier's Linear weights to [-1, 1] before it quantises them; the trainers this model family descends
 * from call _clip_weights after every optimizer step (the reference's loop, train.py:366, lost the call).  The entry points below
 * are the optimizer entry points above with that clamp inside the launch that applies the update.  With bound c = weight_clip,
 * every element w of a clipped tensor that the update leaves becomes
 *     w > c ? c : (w < -c ? -c : w)
 * -- torch.clamp_(-c, c) bit for bit: a NaN stays a NaN, -0.0 stays -0.0 -- before it is stored, and, in the fused update +
 * next-forward pass, before it becomes the operand of the next step's forward.  Momentum and both Adam moments are formed from
 * the un-clamped arithmetic and are never clamped; nothing else of a step reads the clamped value.  A step with the clamp is
 * therefore, bit for bit, the plain step followed by clamp_ on the clipped tensors.
 * weight_clip = 0 is "off": the call then launches exactly what the entry point without the suffix launches (both are one
 * implementation).  A bound that is negative, infinite or NaN is refused with NNUE_E_ARG.  No entry point here takes more
 * scratch or adds a launch.
 * Flat buffers (nnue_sgd_step_clip, nnue_adam_step_clip, nnue_adam_step_ext_clip) name the clipped elements by clip_ranges: a
 * HOST array of n_clip_ranges <= 4 pairs (lo, hi), half-open element ranges inside [0, count]; elements outside every range are
 * not clamped.  A range applies to what the call itself updates: with ext_applied_elsewhere the rows left to the producer are
 * clamped by the producer's own _clip entry point.  The 16-byte kernel is taken only where every boundary is a multiple of 4.
 * The table forms take the bound alone (every element they update belongs to input.weight); the multi-tensor forms take one
 * bound per segment (weight_clip[i], a HOST array like lr[]; NULL or 0: that segment is not clamped). */

/* nnue_sgd_step with the weight clip above (_clip_weights, nnue.py:528-539, after optimizer.step(), train.py:366). */
int nnue_sgd_step_clip(float* params, float* grads, float* momentum_buf, int64_t count, float lr, float momentum,
                       float weight_decay, float max_norm, float grad_scale, int first_step, float* norm_out, void* scratch,
                       int64_t scratch_bytes, const float* ste_partial, int ste_chunks, int ste_fps, float* ste_d_thr,
                       float* ste_d_weight, const float* ext_partial, int ext_count, int64_t ext_lo, int64_t ext_hi, float* coef_out,
                       int ext_applied_elsewhere, const float* lr_dev, float weight_clip, const int64_t* clip_ranges,
                       int n_clip_ranges, nnue_stream_t stream);

/* nnue_adam_step with the weight clip above (_clip_weights, nnue.py:528-539, after optimizer.step(), train.py:366). */
int nnue_adam_step_clip(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int32_t* step_counter, int64_t count,
                        float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, float grad_scale,
                        float* norm_out, void* scratch, int64_t scratch_bytes, const float* lr_dev, float weight_clip,
                        const int64_t* clip_ranges, int n_clip_ranges, nnue_stream_t stream);

/* nnue_adam_step_ext with the weight clip above (_clip_weights, nnue.py:528-539, after optimizer.step(), train.py:366). */
int nnue_adam_step_ext_clip(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int32_t* step_counter, int64_t count,
                            float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, float grad_scale,
                            float* norm_out, void* scratch, int64_t scratch_bytes, const float* ext_partial, int ext_count,
                            int64_t ext_lo, int64_t ext_hi, float* coef_out, int ext_applied_elsewhere, const float* lr_dev,
                            float weight_clip, const int64_t* clip_ranges, int n_clip_ranges, nnue_stream_t stream);

/* nnue_ftm_backward_weight_update with the weight clip above on the table rows it updates (_clip_weights, nnue.py:528-539,
 * after optimizer.step(), train.py:366). */
int nnue_ftm_backward_weight_update_clip(const uint8_t* bits, const float* d_out, int B, int F, int P, int L1, float* weight,
                                         float* momentum_rows, const float* coef, float lr, float momentum, float weight_decay,
                                         float grad_scale, int first_step, float weight_clip, const float* lr_dev,
                                         nnue_stream_t stream);

/* nnue_ftm_backward_weight_update_forward with the weight clip above (_clip_weights, nnue.py:528-539, after optimizer.step(),
 * train.py:366): the next step's forward contracts the clamped tiles, the ones the pass stores. */
int nnue_ftm_backward_weight_update_forward_clip(const uint8_t* bits, const float* d_out, int B, int F, int P, int L1, float* weight,
                                                 float* momentum_rows, const float* coef, float lr, float momentum,
                                                 float weight_decay, float grad_scale, int first_step, float weight_clip,
                                                 const float* lr_dev, const uint8_t* bits_next, const float* sink_next, int B_next,
                                                 const float* bias, float* out_next, void* scratch, int64_t scratch_bytes,
                                                 nnue_stream_t stream);

/* nnue_ftm_backward_weight_update_adam with the weight clip above on the table rows it updates (_clip_weights,
 * nnue.py:528-539, after optimizer.step(), train.py:366). */
int nnue_ftm_backward_weight_update_adam_clip(const uint8_t* bits, const float* d_out, int B, int F, int P, int L1, float* weight,
                                              float* exp_avg_rows, float* exp_avg_sq_rows, const float* coef,
                                              const int32_t* step_counter, float lr, float beta1, float beta2, float eps,
                                              float weight_decay, float grad_scale, float weight_clip, const float* lr_dev,
                                              nnue_stream_t stream);

/* nnue_ftm_backward_weight_update_forward_adam with the weight clip above (_clip_weights, nnue.py:528-539, after
 * optimizer.step(), train.py:366): the next step's forward contracts the clamped tiles, the ones the pass stores. */
int nnue_ftm_backward_weight_update_forward_adam_clip(const uint8_t* bits, const float* d_out, int B, int F, int P, int L1,
                                                      float* weight, float* exp_avg_rows, float* exp_avg_sq_rows, const float* coef,
                                                      const int32_t* step_counter, float lr, float beta1, float beta2, float eps,
                                                      float weight_decay, float grad_scale, float weight_clip, const float* lr_dev,
                                                      const uint8_t* bits_next, const float* sink_next, int B_next, const float* bias,
                                                      float* out_next, void* scratch, int64_t scratch_bytes, nnue_stream_t stream);

/* nnue_multi_sgd_step with the weight clip above per segment (_clip_weights, nnue.py:528-539, after optimizer.step(),
 * train.py:366). */
int nnue_multi_sgd_step_clip(float* const* params, float* const* grads, float* const* momentum_bufs, const int64_t* counts, int n,
                             const float* lr, const float* momentum, const float* weight_decay, const int32_t* first_step,
                             const float* weight_clip, float max_norm, float* norm_out, void* scratch, int64_t scratch_bytes,
                             const float* lr_dev, nnue_stream_t stream);

/* nnue_multi_adam_step with the weight clip above per segment (_clip_weights, nnue.py:528-539, after optimizer.step(),
 * train.py:366). */
int nnue_multi_adam_step_clip(float* const* params, float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                              int32_t* const* step_counters, const int64_t* counts, int n, const float* lr, const float* beta1,
                              const float* beta2, const float* eps, const float* weight_decay, const float* weight_clip,
                              float max_norm, float* norm_out, void* scratch, int64_t scratch_bytes, const float* lr_dev,
                              nnue_stream_t stream);

/* ---- weight average (build extension: a moving average of the weights kept by the launches that store them) --------------
 * Training recipes with mixup, label smoothing and a cosine schedule evaluate and export an exponential moving average of the
 * weights; the reference's loop (train.py:359-366) has none.  The entry points below are the optimizer entry points above with
 * that average inside the launch that applies the update.  With omd = float32(1 - float64(decay)), every element e of the average
 * whose weight the launch stores as w_new becomes
 *     ema_update(e, w_new, omd) = fmaf(omd, w_new - e, e)
 * -- one rounding of the difference, one of the fused multiply-add.  w_new is the value the launch stores: after the update, and
 * after the clamp where the weight clip is on (a convex combination of clamped weights stays inside the bound, so with
 * weight_clip = 1 the average is already the network the export writes).  Momentum and both Adam moments never see the average,
 * and nothing else of a step reads it: a step with the average is, bit for bit, the plain step on parameters and optimizer
 * state plus one ema_update per element -- nnue_ema_update, the stand-alone pass, applied to the old average and the new weights.
 * The rate reaches the kernels as one float by value (ema_omd) or, where ema_omd_dev is not NULL, through that device float,
 * which then replaces it exactly as lr_dev replaces lr (a warm-up changes it without re-recording or re-capturing anything).
 * ema == NULL is "off": the call launches exactly what its _clip sibling launches (one implementation), whatever the rate.
 * With ema != NULL and ema_omd_dev == NULL, ema_omd outside (0, 1] or NaN is refused with NNUE_E_ARG; nothing is launched.
 * Flat buffers: ema is laid out like params (count floats).  Under ext_applied_elsewhere the rows left to the producer are
 * averaged by the producer's own _ema entry point, as with the clip.  Table forms: ema holds the rows that match `weight`
 * (16-byte aligned).  Multi-tensor forms: one pointer and one rate per segment (HOST arrays like lr[]; ema == NULL or ema[i] ==
 * NULL: that segment is off; a list with an average packs 38 segments per launch, one without keeps its 45).
 * The fused update + next-forward pass carries the average too (the kEma forms of its kernel): the new tile is
 * averaged after the clamp and stored behind the parameters; the next step's forward never reads the average, so out_next stays
 * bitwise what the _clip form gives. */

/* The stand-alone pass of the average (after optimizer.step(), train.py:366): ema[i] <- ema_update(ema[i], params[i], omd) for i
 * in [0, count).  Any 4-byte-aligned pointers: 16-byte accesses where both are 16-byte aligned, 4-byte ones otherwise.
 * ema_omd_dev (device float, may be NULL) replaces omd.  NNUE_E_ARG, nothing launched: a NULL ema or params, count <= 0, omd
 * outside (0, 1] or NaN without ema_omd_dev. */
int nnue_ema_update(float* ema, const float* params, int64_t count, float omd, const float* ema_omd_dev, nnue_stream_t stream);

/* nnue_sgd_step_clip with the weight average above (after optimizer.step(), train.py:366). */
int nnue_sgd_step_ema(float* params, float* grads, float* momentum_buf, int64_t count, float lr, float momentum,
                      float weight_decay, float max_norm, float grad_scale, int first_step, float* norm_out, void* scratch,
                      int64_t scratch_bytes, const float* ste_partial, int ste_chunks, int ste_fps, float* ste_d_thr,
                      float* ste_d_weight, const float* ext_partial, int ext_count, int64_t ext_lo, int64_t ext_hi, float* coef_out,
                      int ext_applied_elsewhere, const float* lr_dev, float weight_clip, const int64_t* clip_ranges,
                      int n_clip_ranges, float* ema, float ema_omd, const float* ema_omd_dev, nnue_stream_t stream);

/* nnue_adam_step_clip with the weight average above (after optimizer.step(), train.py:366). */
int nnue_adam_step_ema(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int32_t* step_counter, int64_t count,
                       float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, float grad_scale,
                       float* norm_out, void* scratch, int64_t scratch_bytes, const float* lr_dev, float weight_clip,
                       const int64_t* clip_ranges, int n_clip_ranges, float* ema, float ema_omd, const float* ema_omd_dev,
                       nnue_stream_t stream);

/* nnue_adam_step_ext_clip with the weight average above (after optimizer.step(), train.py:366). */
int nnue_adam_step_ext_ema(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int32_t* step_counter, int64_t count,
                           float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, float grad_scale,
                           float* norm_out, void* scratch, int64_t scratch_bytes, const float* ext_partial, int ext_count,
                           int64_t ext_lo, int64_t ext_hi, float* coef_out, int ext_applied_elsewhere, const float* lr_dev,
                           float weight_clip, const int64_t* clip_ranges, int n_clip_ranges, float* ema, float ema_omd,
                           const float* ema_omd_dev, nnue_stream_t stream);

/* nnue_ftm_backward_weight_update_clip with the weight average above on the table rows it updates (after optimizer.step(),
 * train.py:366): ema = the average's rows that match `weight`. */
int nnue_ftm_backward_weight_update_ema(const uint8_t* bits, const float* d_out, int B, int F, int P, int L1, float* weight,
                                        float* momentum_rows, const float* coef, float lr, float momentum, float weight_decay,
                                        float grad_scale, int first_step, float weight_clip, const float* lr_dev, float* ema,
                                        float ema_omd, const float* ema_omd_dev, nnue_stream_t stream);

/* nnue_ftm_backward_weight_update_forward_clip with the weight average above on the table rows it updates (after
 * optimizer.step(), train.py:366): ema = the average's rows that match `weight`. */
int nnue_ftm_backward_weight_update_forward_ema(const uint8_t* bits, const float* d_out, int B, int F, int P, int L1, float* weight,
                                                float* momentum_rows, const float* coef, float lr, float momentum,
                                                float weight_decay, float grad_scale, int first_step, float weight_clip,
                                                const float* lr_dev, const uint8_t* bits_next, const float* sink_next, int B_next,
                                                const float* bias, float* out_next, void* scratch, int64_t scratch_bytes,
                                                float* ema, float ema_omd, const float* ema_omd_dev, nnue_stream_t stream);

/* nnue_ftm_backward_weight_update_adam_clip with the weight average above on the table rows it updates (after
 * optimizer.step(), train.py:366): ema = the average's rows that match `weight`. */
int nnue_ftm_backward_weight_update_adam_ema(const uint8_t* bits, const float* d_out, int B, int F, int P, int L1, float* weight,
                                             float* exp_avg_rows, float* exp_avg_sq_rows, const float* coef,
                                             const int32_t* step_counter, float lr, float beta1, float beta2, float eps,
                                             float weight_decay, float grad_scale, float weight_clip, const float* lr_dev,
                                             float* ema, float ema_omd, const float* ema_omd_dev, nnue_stream_t stream);

/* nnue_ftm_backward_weight_update_forward_adam_clip with the weight average above on the table rows it updates (after
 * optimizer.step(), train.py:366): ema = the average's rows that match `weight`. */
int nnue_ftm_backward_weight_update_forward_adam_ema(const uint8_t* bits, const float* d_out, int B, int F, int P, int L1,
                                                     float* weight, float* exp_avg_rows, float* exp_avg_sq_rows, const float* coef,
                                                     const int32_t* step_counter, float lr, float beta1, float beta2, float eps,
                                                     float weight_decay, float grad_scale, float weight_clip, const float* lr_dev,
                                                     const uint8_t* bits_next, const float* sink_next, int B_next, const float* bias,
                                                     float* out_next, void* scratch, int64_t scratch_bytes, float* ema,
                                                     float ema_omd, const float* ema_omd_dev, nnue_stream_t stream);

/* nnue_multi_sgd_step_clip with the weight average above per segment (after optimizer.step(), train.py:366). */
int nnue_multi_sgd_step_ema(float* const* params, float* const* grads, float* const* momentum_bufs, const int64_t* counts, int n,
                            const float* lr, const float* momentum, const float* weight_decay, const int32_t* first_step,
                            const float* weight_clip, float max_norm, float* norm_out, void* scratch, int64_t scratch_bytes,
                            const float* lr_dev, float* const* ema, const float* ema_omd, nnue_stream_t stream);

/* nnue_multi_adam_step_clip with the weight average above per segment (after optimizer.step(), train.py:366). */
int nnue_multi_adam_step_ema(float* const* params, float* const* grads, float* const* exp_avgs, float* const* exp_avg_sqs,
                             int32_t* const* step_counters, const int64_t* counts, int n, const float* lr, const float* beta1,
                             const float* beta2, const float* eps, const float* weight_decay, const float* weight_clip,
                             float max_norm, float* norm_out, void* scratch, int64_t scratch_bytes, const float* lr_dev,
                             float* const* ema, const float* ema_omd, nnue_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NNUE_HIP_H */
