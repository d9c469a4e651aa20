/* C ABI of libdca_hip.so -- the MI355X (gfx950) kernels behind the DCANet cost-volume hot path.
 *
 * The reference (cocowy1/Cost-Volume-Aggregation-in-Stereo-Matching-Revisited) has no FFI of its own
 * on this path: every step is a PyTorch op called from Python.  The boundary a maintainer binds is
 * therefore "one extern-C launcher per op the Python path calls", taking raw device pointers,
 * explicit sizes and the HIP stream to enqueue on.  No allocation, no synchronisation and no
 * torch types inside; the caller owns all memory.  Every function returns a hipError_t as int
 * (0 = hipSuccess; invalid arguments -> hipErrorInvalidValue before anything is launched).
 *
 * Tensors are dense fp32 NC[D]HW (the reference's layout).  File:line citations are into the
 * reference tree.  The ctypes binding in cost-volume-aggregation-in-stereo-matching-revisited_amd/_lib.py is read
 * from this header at import; INTEGRATION.md shows how the reference's own modules would call it.
 *
 * What that reader relies on:
 *   - one declaration per `int|long dca_*( ... );`, starting in column 0, every parameter named;
 *   - a parameter is a pointer, a hipStream_t, or a scalar int, long, float or double (anything else is refused);
 *   - an integer `#define DCA_* <literal>` is on one line.
 */
#ifndef DCA_HIP_H
#define DCA_HIP_H

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an argument list below changes (21: dca_gwc_volume_bwd_rows joined the volume entries); the ctypes loader (_lib.py) refuses a library built from another
 * version of this header. */
#define DCA_ABI_VERSION 21
int dca_abi_version(void);

/* storage types of the reduced-precision inference path (0 = fp32) */
#define DCA_BF16 1
#define DCA_FP16 2

/* ---- cost volumes ------------------------------------------------------------------------------
 * build_gwc_volume(refimg_fea, targetimg_fea, maxdisp, num_groups)  models/submodule.py:157-167
 * (groupwise_correlation, submodule.py:148-154).  ref,tgt: (B,C,H,W); vol: (B,G,maxdisp,H,W). */
int dca_gwc_volume_fwd(const float* ref, const float* tgt, float* vol, int B, int C, int H, int W, int maxdisp,
                       int num_groups, hipStream_t stream);
/* autograd of the above (the reference back-propagates through maxdisp slice-assign nodes). */
int dca_gwc_volume_bwd(const float* gvol, const float* ref, const float* tgt, float* gref, float* gtgt, int B, int C,
                       int H, int W, int maxdisp, int num_groups, hipStream_t stream);
/* Which kernel serves dca_gwc_volume_bwd at a shape (host arithmetic, no device call): > 0 = the row-persistent register-
 * blocked kernel, and the value is its grid.x (a workgroup walks the rows y = blockIdx.x, + grid.x, ...), given 16-byte
 * aligned gvol / ref / tgt / gref / gtgt; 0 = the plain kernel, one workgroup per row (also what misaligned tensors get at
 * any shape); < 0 = dca_gwc_volume_bwd refuses these sizes. */
long dca_gwc_volume_bwd_rows(int B, int C, int H, int W, int maxdisp, int num_groups);
/* build_concat_volume(refimg_fea, targetimg_fea, maxdisp)  models/submodule.py:134-145; vol: (B,2C,maxdisp,H,W) */
int dca_concat_volume_fwd(const float* ref, const float* tgt, float* vol, int B, int C, int H, int W, int maxdisp,
                          hipStream_t stream);
int dca_concat_volume_bwd(const float* gvol, float* gref, float* gtgt, int B, int C, int H, int W, int maxdisp,
                          hipStream_t stream);

/* Fused builder (volume_fused.hip): gwc volume and, when Cc > 0, the concat volume written into ONE tensor
 * vol (B, num_groups + 2*Cc, maxdisp, H, W) -- no torch.cat((gwc_volume, concat_volume), 1) (models/gwcnet_dca_g.py:217-220)
 * -- from `nseg` (1..3) channel segments of the correlation features: refs[s], tgts[s]: (B, seg_channels[s], H, W), read
 * in place instead of their concatenation gwc_feature = torch.cat((l2, l3, l4), 1) (gwcnet_dca_g.py:60).  refs / tgts /
 * seg_channels are HOST arrays.  cref, ctgt: (B, Cc, H, W) or NULL.  dtype: 0 = fp32 volume, DCA_BF16 / DCA_FP16 = the
 * reduced-precision inference path's storage type.  W % 4 == 0, 16-byte aligned tensors; every segment width must be a
 * multiple of channels / num_groups.  maxdisp % 4 == 0 for the fp32 volume; any maxdisp for the 2-byte volumes (the
 * disparities are walked four at a time and the last quad may be partial). */
int dca_cost_volume_fwd(const float* const* refs, const float* const* tgts, const int* seg_channels, int nseg,
                        const float* cref, const float* ctgt, int Cc, void* vol, int B, int H, int W, int maxdisp,
                        int num_groups, int dtype, unsigned* vmax, hipStream_t stream);
/* vmax (may be null; fp32 volume without concat part, B * H <= DCA_AMAX_CSLOTS): per-channel slots [g][b * H + y] that receive
 * max |volume| of group g for the f16x2 convolution that reads it (no separate dca_cmax_f32 pass) */

/* ---- softmax over dim 1 / disparity_regression ---------------------------------------------------
 * x: (B,K,HW).  mode 0: out (B,K,HW) = F.softmax(x, dim=1)   (models/gwcnet_dca_g.py:238,248,...)
 *               mode 1: out (B,HW)   = disparity_regression(F.softmax(x,1), K)  (gwcnet_dca_g.py:238-239,263-264)
 *               mode 2: out (B,HW)   = disparity_regression(x, K)               (models/submodule.py:127-131)
 * bwd: mode 0: aux = softmax output, g = (B,K,HW); mode 1: aux = logits x, g = (B,HW); mode 2: g = (B,HW). */
int dca_softargmin_fwd(const float* x, float* out, int B, int K, long HW, int mode, hipStream_t stream);
int dca_softargmin_bwd(const float* aux, const float* g, float* gx, int B, int K, long HW, int mode,
                       hipStream_t stream);

/* Fused training head: disparity_regression(F.softmax(F.upsample(logits[:,None], scale_factor=(s,s,s),
 * mode='trilinear').squeeze(1), 1), s*n)  -- models/gwcnet_dca_g.py:261-264 (s = 8) and the four heads of the baseline
 * models/gwcnet.py:219-237 (s = 4).  s in {2,4,8}; logits: (B,n,hc,wc), n <= 64;
 * disp: (B,1,s*hc,s*wc).  bwd needs g1 = B*n*(s*hc)*(s*wc) floats of scratch. */
int dca_up_softargmin_fwd(const float* logits, float* disp, int B, int n, int hc, int wc, int scale, hipStream_t stream);
int dca_up_softargmin_bwd(const float* logits, const float* gdisp, float* g1, float* glogits, int B, int n, int hc,
                          int wc, int scale, hipStream_t stream);

/* ---- 3D convolutions (nn.Conv3d / nn.ConvTranspose3d, bias=False) ----------------------------------
 * models/submodule.py:121-124 (convbn_3d), models/gwcnet_dca_g.py:141-168, models/augment/cva.py:13-55,
 * models/augment/SelfAttention_bn.py:136-160.
 *
 * dca_conv3d_prep_weight re-lays a PyTorch weight out as wt[tap][a][b] (a < Apad contraction channels,
 * b < Bpad output channels, zero padded), K = 27 or 1 taps:
 *   src_ab = 0: src is [B][A][K]  (Conv3d weight (Cout,Cin,k,k,k) used forward: A = Cin, B = Cout)
 *   src_ab = 1: src is [A][B][K]  (ConvTranspose3d weight (Cin,Cout,...) used forward, or a Conv3d
 *                                  weight used for its backward-data pass: A = Cout, B = Cin)
 *   flip = 1 reverses the taps (backward-data of a stride-1 convolution).
 * Padding rules: Apad = Cin rounded up to 8 (ksize 3) or exactly 32/64 (ksize 1);
 *                Bpad = 32 if (ksize 1 | transposed | (stride 1 & Cout <= 32)) else 64.
 * Btotal / b_off: the source has Btotal output channels of which this call lays out the slice [b_off, b_off+B)
 * (layers with more output channels than one launch produces are run as several launches). */
int dca_conv3d_prep_weight(const float* w, float* wt, int A, int B, int Apad, int Bpad, int K, int src_ab, int flip,
                           int Btotal, int b_off, hipStream_t stream);
/* y = epilogue(conv(x [, x2], wt)).  ksize 3: pad 1, stride 1|2, or transposed (stride 2, pad 1,
 * output_padding 1).  ksize 1: Cin = 32 or 64; if x2 != NULL the input is cat([x, x2], dim=1) with 32
 * channels each (cva.py:69 without materialising the cat).  C1 = channels of x when x2 is given.
 * epilogue(v) = act(v*scale[co] + shift[co] + res_pre) + res_post, act(v) = v > 0 ? v : slope*v
 * (slope 1: none, 0: ReLU, 0.1: LeakyReLU); scale/shift/res_pre/res_post may be NULL.
 * One launch produces Cout <= 64 (3x3x3 conv) or <= 32 (transposed, 1x1x1) channels and writes them at channel
 * offset co_off of a CoutTotal-channel y (scale/shift/res_* are indexed in the full tensor).
 * Backward-data passes reuse this entry with re-laid-out weights:
 *   stride-1 conv   -> stride-1 conv,   src_ab = 1, flip = 1
 *   stride-2 conv   -> transposed conv, src_ab = 1, flip = 0
 *   transposed conv -> stride-2 conv,   src_ab = 0, flip = 0 */
int dca_conv3d_forward(const float* x, const float* x2, const float* wt, float* y, const float* scale,
                       const float* shift, const float* res_pre, const float* res_post, float slope, int N, int Cin,
                       int C1, int Cout, int CinPad, int CoutTotal, int co_off, int Di, int Hi, int Wi, int Do, int Ho,
                       int Wo, int ksize, int stride, int transposed, hipStream_t stream);
/* dw[cy*s_cy + cx*s_cx + k] = sum_{n,o} dy[n,cy,o] x[n,cx,stride*o-1+k]  (ksize 3) / sum dy*x (ksize 1).
 * x: (N,Cx,Di,Hi,Wi), dy: (N,Cy,Do,Ho,Wo).  Conv3d: x = input, dy = grad of output, dw layout
 * (Cout,Cin,K).  ConvTranspose3d: x = grad of output (fine), dy = input (coarse), stride 2, dw layout
 * (Cin,Cout,K).  `part` is scratch of dca_conv3d_wgrad_workspace(...) floats. */
long dca_conv3d_wgrad_workspace(int N, int Cx, int Cy, int Do, int Ho, int Wo, int ksize, int stride);
int dca_conv3d_wgrad(const float* x, const float* dy, float* part, float* dw, int N, int Cx, int Cy, int Di, int Hi,
                     int Wi, int Do, int Ho, int Wo, int ksize, int stride, long s_cy, long s_cx, hipStream_t stream);

/* Backward of y = conv1x1x1(x [, x2]; w) followed by z = act(BN(y)) as one pass (conv1_bwd_fused.hip): from dz, y, the
 * BatchNorm's stats = [mean | invstd | scale | shift] and dgb (dca_bn_backward_reduce) it forms the gradient of y in
 * registers -- the values dca_bn_backward writes as dy, never stored -- and from it
 *   dx (N,32,S) = W[:, :32]^T dy,  dx2 (N,32,S) = W[:, 32:]^T dy (x2 != null),  dw[cy*s_cy + cx*s_cx] = sum dy[cy] x[cx]
 * with x2's block at dw + 32*s_cx; the bits are those of dca_conv3d_wgrad (ksize 1) and of dca_conv1_x3_forward with the
 * transposed weight (the bf16x3 product) over that dy.
 * Cout == 32, (C1,C2) in {(32,0),(32,32)}, S % 4 == 0, dz / y / x / x2 16-byte aligned, N*32*S*4 < 0x7ffff000
 * (hipErrorInvalidValue otherwise: callers use dca_bn_backward + dca_conv1_x3_forward + dca_conv3d_wgrad).
 * w: the fp32 weight (32, C1+C2); part: scratch of dca_conv1_bwd_fused_workspace(N, S, x2 != null) floats. */
long dca_conv1_bwd_fused_workspace(int N, long S, int two);
int dca_conv1_bwd_fused(const float* dz, const float* y, const float* stats, const float* dgb, float slope, int training,
                        const float* x, const float* x2, const float* w, float* part, float* dx, float* dx2, float* dw,
                        long s_cy, long s_cx, int N, int C1, int C2, int Cout, long S, hipStream_t stream);

/* 1x1x1 convolutions with fp32 tensors on the bf16 matrix pipe, fp32-grade (conv1_x3.hip: the exact three-way split of
 * conv3d_bf16x3.hip on an LDS-free data path): same contract as dca_conv3d_forward(ksize 1) -- x (N,C1,S) [, x2 (N,C2,S)],
 * y (N,CoutTotal,S) channels [co_off, co_off+Cout), Cout <= 32, (C1,C2) in {(32,0),(64,0),(32,32)}, S % 4 == 0.
 * wfrag (dca_conv1_x3_weight_bytes(A) bytes) from w read as W[b][a] = src_ab ? w[a*Btotal + b_off + b] : w[(b_off+b)*A + a]. */
long dca_conv1_x3_weight_bytes(int A);
int dca_conv1_x3_prep_weight(const float* w, void* wfrag, int A, int Bn, int src_ab, int Btotal, int b_off,
                             hipStream_t stream);
int dca_conv1_x3_forward(const float* x, const float* x2, const void* wfrag, float* y, const float* scale,
                         const float* shift, const float* res_pre, const float* res_post, float slope, int N, int C1,
                         int C2, int Cout, int CoutTotal, int co_off, long S, hipStream_t stream);

/* Batched weight re-layout: ONE launch for n descriptors of dca_conv3d_prep_weight (kind 0) / dca_conv3d_x3_prep_weight
 * (kind 1) work (prep_many.hip) -- a training step re-packs every conv weight after the optimizer update, and ~130
 * separate 5-us launches cost more than the work.  table: n device-resident 72-byte records
 *   { const float* src; void* dst; int kind, A, Bn, Apad, Bpad, K, src_ab, flip, Btotal, b_off, NCH, pad; long total; }
 * (kind 1 uses A, Bn, src_ab, flip, NCH = ceil(A/16), total = dca_conv3d_x3_weight_bytes/2; kind 0 total = K*Apad*Bpad;
 * kind 3 = dca_conv3d_x2_prep_weight with the fields of kind 1 and total = (dca_conv3d_x2_weight_bytes - 16)/2). */
int dca_conv3d_prep_many(const void* table, int n, hipStream_t stream);

/* The tile walk of the persistent 3x3x3 kernels (csrc/dca_tiles.h), on the HOST: of a launch of `grid` workgroups over
 * `tiles` tiles, workgroup wg visits walk[0], walk[0] + walk[2], ... < walk[1] ({begin, end, step}; walk: 3 host ints).
 * The very function the kernels call, so a CPU test can check that the walks of a launch visit every tile exactly once.
 * No device is touched.  hipErrorInvalidValue unless 0 <= tiles < 0x7fffffff, grid > 0 and 0 <= wg < grid. */
int dca_tile_walk(long tiles, int grid, int wg, int* walk);

/* "bf16x3" split-precision 3x3x3 / stride-1 / pad-1 convolution (conv3d_bf16x3.hip): every fp32 operand is split exactly
 * into three bf16 terms and the six partial products >= 2^-16 run on the bf16 matrix pipe with fp32 accumulation --
 * fp32-grade results (dropped terms <= 2^-23 relative, no range restriction) at 2.67x fewer matrix-pipe cycles than
 * the fp32 MFMA kernel.  Replaces the same nn.Conv3d calls as dca_conv3d_forward (models/submodule.py:121-124,
 * models/augment/cva.py:13-55) and, with src_ab = 1 / flip = 1, their backward-data.
 *   dca_conv3d_x3_weight_bytes(Cin, Cout): size of the pre-split weight image wx.
 *   dca_conv3d_x3_prep_weight: w is the PyTorch weight; A contraction channels, B output channels;
 *       src_ab ? w[a][b][27] : w[b][a][27]; flip reverses the tap order (backward-data).  wx 16-byte aligned.
 *   dca_conv3d_x3_forward: y (N,Cout,D,H,W) = act((conv(x, w)) * scale[c] + shift[c] + res_pre) + res_post, the epilogue
 *       contract of dca_conv3d_forward; any Cin / Cout (zero padded to 16 / 32 internally); Cin*D*H*W*4 < 2^31. */
long dca_conv3d_x3_weight_bytes(int Cin, int Cout);
int dca_conv3d_x3_prep_weight(const float* w, void* wx, int A, int B, int src_ab, int flip, hipStream_t stream);
int dca_conv3d_x3_forward(const float* x, const void* wx, float* y, const float* scale, const float* shift,
                          const float* res_pre, const float* res_post, float slope, int N, int Cin, int Cout, int D,
                          int H, int W, hipStream_t stream);

/* ConvTranspose3d(k 3, stride 2, padding 1, output_padding 1) with fp32 tensors on the bf16 matrix pipe, same exact
 * three-way split (deconv3d_x3.hip): `cost_agg.conv3` forward (models/augment/cva.py:21-29) and the backward-data of
 * `cost_agg.conv1` (cva.py:16-17).  x (N,Cin,Di,Hi,Wi) -> y (N,Cout<=32,2Di,2Hi,2Wi) = act(deconv * scale + shift +
 * res_pre) + res_post, the epilogue contract of dca_conv3d_forward.  wx = dca_conv3d_x3_prep_weight(w, wx, A = Cin,
 * B = Cout, src_ab, flip 0) (w[a][b][27] for src_ab 1).  Requires Wi % 4 == 0, 16-byte aligned x / wx, 8-byte aligned y and
 * residuals (hipErrorInvalidValue otherwise: callers use dca_conv3d_forward(transposed 1)). */
int dca_deconv3d_x3_forward(const float* x, const void* wx, float* y, const float* scale, const float* shift,
                            const float* res_pre, const float* res_post, float slope, int N, int Cin, int Cout, int Di,
                            int Hi, int Wi, hipStream_t stream);

/* The same convolution without epilogue, fused with the BatchNorm batch statistics of its output (training-mode
 * convbn_3d, models/submodule.py:121-124; csrc/bn_fused_stats.h): part (Cout * nchunk * 4 doubles, nchunk =
 * dca_conv3d_x3_stats_chunks(...)) receives ONE partial per (channel, workgroup), part[(c*nchunk + i)*4 + {0,1,2,3}] =
 * {K, n, sum (y - K), sum (y - K)^2} with a shift K taken from the partial's own data (no loss of variance for
 * |mean| >> std); dca_bn_finalize_centered(part, nchunk, ...) re-centres and sums them in double.  Fixed summation order,
 * a function of the data alone: bitwise reproducible. */
long dca_conv3d_x3_stats_chunks(int N, int Cout, int D, int H, int W);
int dca_conv3d_x3_forward_stats(const float* x, const void* wx, float* y, double* stat_part, int N, int Cin, int Cout,
                                int D, int H, int W, hipStream_t stream);
/* The same for the 1x1x1 convolutions (conv1_x3.hip; part covers all CoutTotal channels, every channel slice of a sliced
 * convolution fills its own channels) and the transposed convolution (deconv3d_x3.hip). */
long dca_conv1_x3_stats_chunks(int N, long S);
int dca_conv1_x3_forward_stats(const float* x, const float* x2, const void* wfrag, float* y, double* stat_part, int N,
                               int C1, int C2, int Cout, int CoutTotal, int co_off, long S, hipStream_t stream);
long dca_deconv3d_x3_stats_chunks(int N, int Di, int Hi, int Wi);
int dca_deconv3d_x3_forward_stats(const float* x, const void* wx, float* y, double* stat_part, int N, int Cin, int Cout,
                                  int Di, int Hi, int Wi, hipStream_t stream);
/* [mean | invstd | scale | shift] (4*C floats) from those partials, with the running-statistics update of training-mode
 * nn.BatchNorm3d (momentum, unbiased variance); running_mean / running_var may both be null. */
int dca_bn_finalize_centered(const double* part, int nchunk, const float* gamma, const float* beta, float* running_mean,
                             float* running_var, float momentum, float eps, float* stats, int* zexps,
                             const unsigned* rpre_slots, int rpre_n, const unsigned* rpost_slots, int rpost_n, int C,
                             hipStream_t stream);

/* Weight gradient of the 3x3x3 / stride-1 / pad-1 convolution on the bf16 matrix pipe with the same exact three-way
 * bf16 split (conv3d_wgrad_bf16x3.hip); replaces dca_conv3d_wgrad for ksize 3, stride 1 (autograd's dW of the nn.Conv3d
 * calls above).  dw[cy*s_cy + cx*s_cx + tap] = sum_{n,voxels} dy[n][cy] * x[n][cx] shifted by the tap; x (N,Cx,D,H,W),
 * dy (N,Cy,D,H,W); part = scratch of dca_conv3d_wgrad_x3_workspace floats.  Requires W % 4 == 0 and 16-byte aligned
 * x / dy (hipErrorInvalidValue otherwise: callers use dca_conv3d_wgrad).  Deterministic, no atomics. */
long dca_conv3d_wgrad_x3_workspace(int N, int Cx, int Cy, int D, int H, int W);
int dca_conv3d_wgrad_x3(const float* x, const float* dy, float* part, float* dw, int N, int Cx, int Cy, int D, int H,
                        int W, long s_cy, long s_cx, hipStream_t stream);

/* "f16x2" split-precision 3x3x3 / stride-1 / pad-1 convolution and weight gradient (conv3d_f16x2.hip,
 * conv3d_wgrad_f16x2.hip, conv3d_wgrad_s2_f16x2.hip) -- the kernels the models run: every CHANNEL of an fp32 operand is
 * scaled by its own power of two 2^exps[c] (scaled maximum in [2^14, 2^15): inside the f16 range whatever the channel's
 * magnitude and whatever the other channels'), split into two f16 terms (|x - h - l| <= 2^-22 |x|) and the three partial
 * products >= 2^-11 run on the f16 matrix pipe with fp32 accumulation; the result is scaled back exactly (v_ldexp_f32).
 * Half the matrix-pipe cycles of the bf16x3 kernels at the same measured error against fp64, per output channel
 * (tests/test_gpu_parity.py::test_f16x2_per_channel_scales).  Same operators as dca_conv3d_x3_forward /
 * dca_conv3d_wgrad_x3 (models/submodule.py:121-124, models/augment/cva.py:13-55) and, with src_ab = 1 / flip = 1, their
 * backward-data.
 *   Per-channel maxima ("slots"): slots[c * DCA_AMAX_CSLOTS + s], s < nslots = the bit patterns of partial maxima of |x| over
 *       channel c, one slot per producing workgroup (plain stores, one writer per slot, nothing to zero-initialise; the
 *       consumer takes the unsigned maximum).  Filled by dca_bn_apply (zmax), dca_bn_backward (dmax),
 *       dca_conv3d_x2_forward (y_cmax) for the tensors they write, or by dca_cmax_f32 (a read pass; nslots =
 *       dca_bn_num_chunks(C, S)).  dca_cmax_exps: exps[c] from the slots.
 *   Packed operand "px2": the fp32 tensor (N,C,D,H,W), C % 8 == 0, as its two scaled f16 terms, per sample
 *       [term 2][C/8][D][H][W][8] f16 (4 bytes per element, like fp32), written by dca_bn_apply_pack / dca_bn_backward_pack
 *       (or dca_bn_apply_pack with stats = null: plain packing) together with the exponents it was scaled by.  Consumers:
 *       dca_conv3d_x2_forward[_stats] (packed = 1) and dca_conv3d_wgrad_x2 (x_packed / dy_packed).
 *   dca_conv3d_x2_prep_weight: packs w for ONE launch over an operand with exponents xexps (it folds 2^-xexps[k] into
 *       the weight rows and gives every output channel its own scale): x_slots == null -> xexps is an input;
 *       else xexps is derived from the slots and written (A ints) for later users of the same operand.
 *   dca_conv3d_x2_forward[_stats]: contracts of dca_conv3d_x3_forward[_stats]; y_cmax (may be null; forces the fused
 *       epilogue variant) = per-channel slots that receive max |y|, nslots = dca_conv3d_x2_stats_chunks(...).
 *   dca_conv3d_wgrad_x2 / _s2_x2: contracts of dca_conv3d_wgrad_x3 / the stride-2 form below; exps of both operands. */
#define DCA_AMAX_CSLOTS 1024
int dca_cmax_f32(const float* x, int N, int C, long S, unsigned* slots, hipStream_t stream);
int dca_cmax_exps(const unsigned* slots, int nslots, int C, int* exps, hipStream_t stream);
long dca_conv3d_x2_weight_bytes(int Cin, int Cout);
int dca_conv3d_x2_prep_weight(const float* w, void* wx, int A, int B, int src_ab, int flip, const unsigned* x_slots,
                              int nslots, int* xexps, hipStream_t stream);
int dca_conv3d_x2_forward(const void* x, int packed, const int* xexps, const void* wx, float* y, const float* scale,
                          const float* shift, const float* res_pre, const float* res_post, float slope, unsigned* y_cmax,
                          int N, int Cin, int Cout, int D, int H, int W, hipStream_t stream);
long dca_conv3d_x2_stats_chunks(int N, int Cout, int D, int H, int W);
int dca_conv3d_x2_forward_stats(const void* x, int packed, const int* xexps, const void* wx, float* y, double* stat_part,
                                int N, int Cin, int Cout, int D, int H, int W, hipStream_t stream);
/* dca_conv3d_wgrad_s2_x2: the same arithmetic for the weight gradient of the STRIDE-2 convolution `cost_agg.conv1` and of
 * the transposed convolution `cost_agg.conv3` (models/augment/cva.py:16-29; conv3d_wgrad_s2_f16x2.hip):
 * dw[cy*s_cy + cx*s_cx + tap] = sum_{n,o} c[n][cy][o] * f[n][cx][2o + tap - 1], f = fine tensor (N,Cx,D,H,W), c = coarse tensor
 * (N,Cy,(D+1)/2,(H+1)/2,(W+1)/2); for the transposed convolution f = dy, c = x.  Requires W % 4 == 0, (W+1)/2 % 4 == 0 and
 * 16-byte aligned tensors (hipErrorInvalidValue otherwise: callers use dca_conv3d_wgrad). */
long dca_conv3d_wgrad_s2_x2_workspace(int N, int Cx, int Cy, int D, int H, int W);
int dca_conv3d_wgrad_s2_x2(const float* f, const int* f_exps, const float* c, const int* c_exps, float* part,
                           float* dw, int N, int Cx, int Cy, int D, int H, int W, long s_cy, long s_cx, hipStream_t stream);
/* The STRIDE-2 3x3x3 convolution itself (padding 1) with the f16x2 arithmetic (conv3d_s2_f16x2.hip): `cost_agg.conv1` =
 * Conv3d(32, 64, 3, stride 2, padding 1) forward (models/augment/cva.py:16-17) and the backward-data of `cost_agg.conv3` =
 * ConvTranspose3d(64, 32, 3, stride 2, ...) (cva.py:21-29: the same operator over dy, weight read as [output][contraction]).
 * x (N,Cin,Di,Hi,Wi) fp32, Wi % 4 == 0, 16-byte aligned -> y (N,Cout,(Di+1)/2,(Hi+1)/2,(Wi+1)/2) = act(conv * scale + shift) +
 * res_post (all optional: the training launches use none; inference folds the BatchNorm; no res_pre); y_cmax (may be null) =
 * per-channel slots [c][s], s < dca_conv3d_s2x2_out_slots(...), that receive max |y| for an f16x2 convolution reading y.  Weights are packed per launch like
 * dca_conv3d_x2_prep_weight (another fragment layout: K-steps of 4 channels x 4 taps, output-channel blocks of 64). */
long dca_conv3d_s2x2_weight_bytes(int Cin, int Cout);
int dca_conv3d_s2x2_prep_weight(const float* w, void* wx, int A, int B, int src_ab, int flip, const unsigned* x_slots,
                                int nslots, int* xexps, hipStream_t stream);
long dca_conv3d_s2x2_out_slots(int N, int Cout, int Di, int Hi, int Wi);
int dca_conv3d_s2x2_forward(const float* x, const int* xexps, const void* wx, float* y, const float* scale, const float* shift,
                            float slope, const float* res_post, unsigned* y_cmax, int N, int Cin, int Cout, int Di, int Hi, int Wi,
                            hipStream_t stream);
long dca_conv3d_wgrad_x2_workspace(int N, int Cx, int Cy, int D, int H, int W);
int dca_conv3d_wgrad_x2(const void* x, int x_packed, const int* xexps, const void* dy, int dy_packed, const int* yexps,
                        float* part, float* dw, int N, int Cx, int Cy, int D, int H, int W, long s_cy, long s_cx,
                        hipStream_t stream);

/* Single-output-channel 3x3x3 convolution (the logit heads: nn.Conv3d(32, 1, 3, padding=1, bias=False),
 * models/gwcnet_dca_g.py:154-168 `classif*.2`, models/augment/cva.py:51-53 `classify.2`).  w is the PyTorch weight
 * (1,C,3,3,3) as is.  The 27 taps become a GEMM axis so forward / weight gradient reuse the matrix-core kernels:
 *   forward: T (N,27,D,H,W) = dca_conv3d_forward(ksize 1, weight laid out [ci][tap]);  y = dca_conv3d_c1_gather(T)
 *   wgrad:   G (N,27,D,H,W) = dca_conv3d_c1_expand(dy);  dW = dca_conv3d_wgrad(x, G, ksize 1, s_cy 1, s_cx 27)
 *   bwd_data: dy (N,1,..) -> dx (N,C,..) directly. */
int dca_conv3d_c1_gather(const float* T, float* y, int N, int D, int H, int W, hipStream_t stream);
/* wgrad without the expanded tensor (round 3): dw[ci*27 + tap] = sum x[ci][v] dy[v - offset(tap)], the tap-shifted views of dy
 * are built while the tiles are fetched.  W % 4 == 0, 16-byte aligned x / dy, N*C*D*H*W*4 < 2^31 (hipErrorInvalidValue
 * otherwise: use the expand form); part = dca_conv3d_wgrad_workspace(N, C, 27, D, H, W, 1, 1) floats. */
int dca_conv3d_c1_wgrad(const float* x, const float* dy, float* part, float* dw, int N, int C, int D, int H, int W,
                        hipStream_t stream);
int dca_conv3d_c1_expand(const float* dy, float* G, int N, int D, int H, int W, hipStream_t stream);
int dca_conv3d_c1_bwd_data(const float* dy, const float* w, float* dx, int N, int C, int D, int H, int W,
                           hipStream_t stream);

/* ---- BatchNorm3d + activation + residual -------------------------------------------------------------
 * nn.BatchNorm3d defaults (eps 1e-5, momentum 0.1) as used by convbn_3d, models/submodule.py:121-124.
 * dca_bn_stats:    part[(c*nchunk+i)*2+{0,1}] = partial (sum, sum of squares) of x - K_c in double, with the per-channel
 *                  shift K_c = x[0,c,0] at part[C*nchunk*2 + c] (no catastrophic cancellation when |mean| >> std);
 *                  nchunk = dca_bn_num_chunks(C, S); part holds C*nchunk*2 + C doubles.
 * dca_bn_finalize: stats = [mean | invstd | scale | shift] (4*C floats); training != 0 uses the batch
 *                  statistics and updates running_mean/var (unbiased), else uses the running stats.
 * dca_bn_apply:    z = act(scale*y + shift + res_pre) + res_post.
 * dca_bn_backward: given dz -> dy (grad of the conv output), dgb = [dgamma | dbeta | ...] (4*C floats),
 *                  optional g_out = grad w.r.t. res_pre (= dz masked by the activation).
 * zmax / dmax (dca_bn_apply: of z, dca_bn_backward: of dy; may be null): per-channel slots (see "f16x2" above; nslots =
 *                  dca_bn_num_chunks(C, S)) that receive max |.| of the tensor written; ymax (dca_bn_apply[_pack]; may be
 *                  null): slots that receive max |y - mean| per channel (it bounds |xhat| for the backward pass' scale).
 * zexps (dca_bn_finalize[_centered]; may be null, training only): per-channel scale exponents for z = act(BN(y) + res_pre) +
 *                  res_post from the bound |z| <= |gamma| sqrt(count) + |beta| + max |res_pre| + max |res_post| (the residual
 *                  tensors' per-channel slots rpre_slots / rpost_slots, may be null) -- known before z is written, so that
 * dca_bn_apply_pack writes z directly in the packed px2 format (stats = null: plain packing of y with zexps) and, with
 *                  zf != null, a second fp32 copy for the other readers of z (zmax: its per-channel slots); nslots of ymax / zmax =
 *                  dca_bn_pack_chunks(C, S).
 * dca_bn_backward_pack: dca_bn_backward (no res_pre / g_out) writing dy in the packed px2 format; dyexps (C ints, out) =
 *                  the exponents it was scaled by (bound from max |g|, this launch's reduce pass, and max |xhat| = invstd *
 *                  ymax); gmax = scratch of C * DCA_AMAX_CSLOTS words. */
int dca_bn_num_chunks(int C, long S);
int dca_bn_pack_chunks(int C, long S);
int dca_bn_stats(const float* x, double* part, int N, int C, long S, hipStream_t stream);
int dca_bn_finalize(const double* part, int nchunk, double count, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float momentum, float eps, int training, float* stats,
                    int* zexps, const unsigned* rpre_slots, int rpre_n, const unsigned* rpost_slots, int rpost_n, int C,
                    hipStream_t stream);
int dca_bn_apply(const float* y, const float* stats, const float* res_pre, const float* res_post, float* z, int N,
                 int C, long S, float slope, unsigned* zmax, unsigned* ymax, hipStream_t stream);
int dca_bn_apply_pack(const float* y, const float* stats, const int* zexps, void* zp, int N, int C, long S, float slope,
                      unsigned* ymax, const float* res_pre, const float* res_post, float* zf, unsigned* zmax,
                      hipStream_t stream);
int dca_bn_backward(const float* dz, const float* y, const float* res_pre, const float* stats, double* part,
                    float* dgb, float* dy, float* g_out, int N, int C, long S, float slope, int training,
                    unsigned* dmax, hipStream_t stream);
/* the reduce and finalize passes of dca_bn_backward alone (no res_pre): dgb only, for dca_conv1_bwd_fused */
int dca_bn_backward_reduce(const float* dz, const float* y, const float* stats, double* part, float* dgb, int N, int C,
                           long S, float slope, int training, hipStream_t stream);
int dca_bn_backward_pack(const float* dz, const float* y, const float* stats, double* part, float* dgb, void* dyp,
                         int* dyexps, unsigned* gmax, const unsigned* ymax, int ymax_slots, int N, int C, long S,
                         float slope, int training, hipStream_t stream);
/* dca_bn_backward_pack for the BatchNorm in front of a logit head (ConvBn3d -> ReLU -> Conv3d(C, 1, 3)), with the head's
 * backward-data folded in: dz = the gradient of the head's input is never a tensor, both passes form it from the head's
 * 1-channel output gradient dlogit (N,1,D,H,W) and weight w_head (1,C,3,3,3) -- the 27-tap stencil of
 * dca_conv3d_c1_bwd_data, same rounding -- while they stream y.  No dca_conv3d_c1_bwd_data launch, no write and no
 * two reads of a (N,C,D,H,W) tensor.  Every output is, bit for bit, what dca_conv3d_c1_bwd_data + dca_bn_backward_pack give:
 * the reduce pass keeps that entry's chunks and per-lane summation order.  C == 32, W % 4 == 0, 16-byte aligned dlogit / y /
 * dyp, C*D*H*W*4 < 2^31 (hipErrorInvalidValue otherwise: use the two entries).  part = C * dca_bn_backward_pack_c1_chunks(N, D,
 * H, W) * 2 doubles (= dca_bn_num_chunks(32, D*H*W) chunks); dca_bn_backward_pack_c1_grid: the persistent workgroups of the
 * apply pass (4 x 8 x 32 tiles; for tests); the other arguments as dca_bn_backward_pack. */
int dca_bn_backward_pack_c1_chunks(int N, int D, int H, int W);
int dca_bn_backward_pack_c1_grid(int N, int D, int H, int W);
int dca_bn_backward_pack_c1(const float* dlogit, const float* w_head, const float* y, const float* stats, double* part,
                            float* dgb, void* dyp, int* dyexps, unsigned* gmax, const unsigned* ymax, int ymax_slots, int N,
                            int C, int D, int H, int W, float slope, int training, hipStream_t stream);
/* The output BatchNorm of a block whose pre-activation residual is ITSELF a slope-1 BatchNorm without residuals over batch
 * statistics (models/augment/cva.py:26-31: relu(BN_d(deconv) + BN_r(redir))), with that skip BatchNorm folded in: the
 * residual is never stored, every kernel forms res_pre = fma(y_r, scale_r, shift_r) in registers from the skip's input y_r
 * and its statistics stats_r -- the bits dca_bn_apply(y_r, stats_r, slope 1) writes.
 * dca_bn_skip_max:        slots (C * DCA_AMAX_CSLOTS words, nslots = dca_bn_num_chunks(C, S)) receive the per-channel maxima of
 *                  |res_pre| that dca_bn_apply would emit as zmax while writing it -- a read pass over y_r, no store; handed
 *                  to dca_bn_finalize[_centered] as rpre_slots, so zexps are those of the route that stores the residual.
 * dca_bn_apply_pack_skip: dca_bn_apply_pack with (y_r, stats_r) in place of res_pre.
 * dca_bn_backward_skip:   dca_bn_backward with (y_r, stats_r) in place of res_pre; g_out is required (the skip's producer
 *                  reads it as its dz) and the reduce pass also forms the skip BatchNorm's sums (part_r, as large as part),
 *                  so that dgb_r = the dgb of dca_bn_backward_reduce(g_out, y_r, stats_r, slope 1), bit for bit, without
 *                  that pass. */
int dca_bn_skip_max(const float* y_r, const float* stats_r, int N, int C, long S, unsigned* slots, hipStream_t stream);
int dca_bn_apply_pack_skip(const float* y, const float* stats, const int* zexps, void* zp, int N, int C, long S, float slope,
                           unsigned* ymax, const float* y_r, const float* stats_r, const float* res_post, float* zf,
                           unsigned* zmax, hipStream_t stream);
int dca_bn_backward_skip(const float* dz, const float* y, const float* y_r, const float* stats, const float* stats_r,
                         double* part, double* part_r, float* dgb, float* dgb_r, float* dy, float* g_out, int N, int C,
                         long S, float slope, int training, unsigned* dmax, hipStream_t stream);

/* ---- AvgPool3d((3,3,3), stride 2, padding 1) -- models/augment/cva.py:39 ---------------------------- */
int dca_avgpool3d_fwd(const float* x, float* y, long NC, int Di, int Hi, int Wi, hipStream_t stream);
/* res (may be null): another gradient of the pooled tensor's input, added to gx on the way (ops._PoolFork) */
int dca_avgpool3d_bwd(const float* gy, float* gx, const float* res, const float* res2, long NC, int Di, int Hi, int Wi,
                     hipStream_t stream);   /* res / res2 (may be null): further gradients of the same input, added on the way */

/* ---- F.interpolate(scale_factor=(s,s,s), mode='trilinear'), align_corners=False -----------------------
 * models/augment/cva.py:64 (s = 2), models/gwcnet_dca_g.py:251,256 (s = 2), :261 (s = 8). */
int dca_trilinear_fwd(const float* x, float* y, long NC, int Di, int Hi, int Wi, int scale, hipStream_t stream);
int dca_trilinear_bwd(const float* gy, float* gx, long NC, int Di, int Hi, int Wi, int scale, hipStream_t stream);

/* ---- homogeneous-region context injection -- SemanticLevelContext.forward, semantic_level.py:96-126 ---
 * x,key: (B,C,n,HW); preds: (B,n,HW) logits.  key = feats_sl + x.  Side outputs (saved for backward):
 * kstar (B,HW) int32 argmax class, e (B,HW), pm (B,HW) = p[k*], denom (B,n).  part: scratch of
 * B*ceil(HW/256)*n floats (per-workgroup class sums, added in a fixed order: bitwise reproducible). */
int dca_context_inject_fwd(const float* x, const float* preds, float* key, int* kstar, float* e, float* pm,
                           float* denom, float* part, int B, int C, int n, long HW, hipStream_t stream);
int dca_context_inject_bwd(const float* dkey, const float* x, const float* preds, const int* kstar, const float* e,
                           const float* pm, const float* denom, float* dx, float* dpreds, float* dw, float* T,
                           float* part, int B, int C, int n, long HW, hipStream_t stream);

/* ---- per-pixel disparity attention core -- SelfAttentionBlock.forward, SelfAttention_bn.py:70-94 ------
 * q,k,v,out: (B,C,n,HW), heads of 8 channels, softmax(q k^T / sqrt(8)) v over the n bins (n <= 64). */
int dca_disp_attention_fwd(const float* q, const float* k, const float* v, float* out, int B, int C, int n, long HW,
                           hipStream_t stream);
int dca_disp_attention_bwd(const float* q, const float* k, const float* v, const float* dout, float* dq, float* dk,
                           float* dv, int B, int C, int n, long HW, hipStream_t stream);

/* ---- the steps right after the path ------------------------------------------------------
 * Convex x4 up-sampling, PropgationNet_4x.forward after its conv (models/submodule.py:366-373, copy
 * models/gwcnet_dca_g.py:114-124): mask_logits (B,144,h,w) with channel = k*16 + i*4 + j, disp (B,1,h,w) in 1/4-res
 * pixels -> up (B,1,4h,4w) = sum_k softmax_k(mask)[k,i,j] * 4*disp[3x3 zero-padded neighbour k].
 * bwd: glogits (B,144,h,w), gdisp (B,1,h,w); wk = B*9*h*w floats of scratch. */
int dca_convex_up4_fwd(const float* mask_logits, const float* disp, float* up, int B, int h, int w, hipStream_t stream);
int dca_convex_up4_bwd(const float* mask_logits, const float* disp, const float* gup, float* glogits, float* gdisp,
                       float* wk, int B, int h, int w, hipStream_t stream);

/* Stereo focal loss, StereoFocalLoss.loss_per_level + LaplaceDisp2Prob (models/loss.py:206-240, 60-128), for `nlev`
 * estimates of equal shape (B,K,HW) that share one ground truth gt (B,HW) ALREADY scaled/pooled to that resolution
 * (loss.py:210-215 stays on the host: one adaptive pooling per resolution).  ests / gests / weights are HOST arrays of
 * nlev (<= 8) device pointers / floats.  out: nlev+1 floats = the per-level losses (un-weighted, loss.py:238) and
 * sum_l weights[l]*loss_l (focal_loss, loss.py:16-24).  K <= 256.  work: dca_focal_loss_workspace(...) doubles, must be
 * handed unchanged to the backward call, which writes gests[l] = d(out[nlev]) / d(ests[l]) * gloss[0]. */
long dca_focal_loss_workspace(int nlev, int B, long HW);
int dca_focal_loss_fwd(const float* const* ests, const float* weights, int nlev, const float* gt, double* work,
                       float* out, int B, int K, long HW, float focal_coefficient, hipStream_t stream);
int dca_focal_loss_bwd(const float* const* ests, float* const* gests, const float* weights, int nlev, const float* gt,
                       const double* work, const float* gloss, int B, int K, long HW, float focal_coefficient,
                       hipStream_t stream);

/* ---- reduced-precision inference path (BASELINE configs 2 "bf16" and 5 "fp16") ---------------------------------
 * Activations stored as bf16 / fp16, ONE native MFMA product per multiply, fp32 accumulation and fp32 epilogue
 * arithmetic (folded BatchNorm affine, activation, residuals); forward only.  dtype codes: */
/* 3x3x3 stride-1 convolution (convbn_3d + ReLU of models/submodule.py:121-124 in eval mode).  wx: dca_conv3d_lp_weight_bytes
 * bytes, filled by dca_conv3d_lp_prep_weight (A, B, src_ab, flip as in dca_conv3d_prep_weight).  x: (N,Cin,D,H,W) in the
 * 2-byte type, or fp32 when in_f32; y, res_pre, res_post: (N,Cout,D,H,W) in the 2-byte type, or fp32 when out_f32.
 * y = act(conv * scale + shift + res_pre) + res_post. */
long dca_conv3d_lp_weight_bytes(int Cin, int Cout);
int dca_conv3d_lp_prep_weight(const float* w, void* wx, int A, int B, int src_ab, int flip, int dtype,
                              hipStream_t stream);
int dca_conv3d_lp_forward(const void* x, const void* wx, void* y, const float* scale, const float* shift,
                          const void* res_pre, const void* res_post, float slope, int N, int Cin, int Cout, int D, int H,
                          int W, int dtype, int in_f32, int out_f32, hipStream_t stream);

/* 1x1x1 convolution (pointwise GEMM), Cout <= 32, over one or two 2-byte inputs (implicit channel concat: the `fuse` conv
 * of models/augment/cva.py:55,69; `cost_agg.redir`, cva.py:23; the tap-expansion GEMM of the logit heads).  w: (Cout,
 * C1 + C2) fp32 row major -> wfrag (dca_conv1_lp_weight_bytes bytes).  x: (N,C1,S), x2: (N,C2,S) or NULL (C2 = 0);
 * y / res_pre / res_post: (N,Cout,S) in the 2-byte type, or fp32 when out_f32.  S % 4 == 0. */
long dca_conv1_lp_weight_bytes(int C1, int C2);
int dca_conv1_lp_prep_weight(const float* w, void* wfrag, int Cout, int C1, int C2, int dtype, hipStream_t stream);
int dca_conv1_lp_forward(const void* x, const void* x2, const void* wfrag, void* y, const float* scale,
                         const float* shift, const void* res_pre, const void* res_post, float slope, int N, int C1,
                         int C2, int Cout, long S, int dtype, int out_f32, hipStream_t stream);

/* Mixed-storage forms of dca_conv3d_forward (exact-fp32 MFMA arithmetic, wt as for dca_conv3d_forward with Bpad 64 /
 * 32): transposed == 0: 3x3x3 stride-2 conv, x (N,Cin,Di,Hi,Wi) 2-byte -> y (N,Cout<=64,Do,Ho,Wo) fp32, no residuals
 * (cost_agg.conv1, models/augment/cva.py:16-17); transposed == 1: ConvTranspose3d(3,s2,p1,op1), x fp32 -> y, res_pre,
 * res_post (N,Cout<=32,2Di,2Hi,2Wi) 2-byte (cost_agg.conv3 + ReLU(. + redir(x)) [+ outer residual], cva.py:21-29). */
int dca_conv3d_forward_mixed(const void* x, const float* wt, void* y, const float* scale, const float* shift,
                             const void* res_pre, const void* res_post, float slope, int N, int Cin, int Cout, int CinPad,
                             int Di, int Hi, int Wi, int Do, int Ho, int Wo, int transposed, int dtype,
                             hipStream_t stream);
/* Reduced-precision 3x3x3 stride-2 convolution (conv3d_s2_lp.hip; cost_agg.conv1 = convbn_3d(32, 64, 3, 2, 1) + ReLU,
 * cva.py:16-17): x (N,Cin,D,H,W) 2-byte, ONE MFMA product, fp32 accumulation -> y (N,Cout<=64,ceil(D/2),..) fp32 =
 * act(conv * scale + shift).  w: (Cout,Cin,3,3,3) fp32 -> wx (dca_conv3d_s2_lp_weight_bytes(Cin) bytes).  W % 4 == 0. */
long dca_conv3d_s2_lp_weight_bytes(int Cin);
int dca_conv3d_s2_lp_prep_weight(const float* w, void* wx, int Cin, int Cout, int dtype, hipStream_t stream);
int dca_conv3d_s2_lp_forward(const void* x, const void* wx, float* y, const float* scale, const float* shift, float slope,
                             int N, int Cin, int Cout, int D, int H, int W, int dtype, hipStream_t stream);
/* Reduced-precision ConvTranspose3d(3, s2, p1, op1) (deconv3d_lp.hip; cost_agg.conv3 + ReLU(. + redir) [+ outer residual],
 * cva.py:21-29): x (N,Cin<=64,Di,Hi,Wi) fp32 rounded on the fly, ONE MFMA product, fp32 accumulation; y, res_pre, res_post
 * (N,Cout<=32,2Di,2Hi,2Wi) 2-byte.  wx = dca_conv3d_lp_prep_weight(w (Cin,Cout,3,3,3), wx, Cin, Cout, src_ab 1, flip 0, dtype). */
int dca_deconv3d_lp_forward(const float* x, const void* wx, void* y, const float* scale, const float* shift,
                            const void* res_pre, const void* res_post, float slope, int N, int Cin, int Cout, int Di,
                            int Hi, int Wi, int dtype, hipStream_t stream);
/* nn.AvgPool3d((3,3,3), 2, 1) (cva.py:39): x (NC,Di,Hi,Wi) 2-byte -> y (NC,ceil/2...) fp32; Wi % 4 == 0.
 * F.interpolate(scale_factor=(2,2,2), mode='trilinear') (cva.py:64): x (NC,Di,Hi,Wi) fp32 -> y (NC,2Di,2Hi,2Wi) 2-byte. */
int dca_avgpool3d_lp_fwd(const void* x, float* y, long NC, int Di, int Hi, int Wi, int dtype, hipStream_t stream);
int dca_trilinear_up2_lp_fwd(const float* x, void* y, long NC, int Di, int Hi, int Wi, int dtype, hipStream_t stream);

/* ---- evaluation step (eval_metrics.hip): the tail of main_dca.py:143-246 `mytest` without a host round trip -------------
 * All results are bitwise reproducible run to run: counts are integers, floating sums are fp64 per-workgroup partials
 * reduced in a fixed order.
 *
 * dca_disp_metrics: pred (B,H+top_pad,W+right_pad) fp32 -- the padded frame; the crop `[:, top_pad:, :W]` of
 * main_dca.py:171-174 is done by addressing -- gt (B,H,W) fp32, mask (B,H,W) bytes (non-zero = use) or NULL:
 * mask = gt > 0 && gt < maxdisp (main_dca.py:151).  rec: (B, DCA_EVAL_REC) doubles, one record PER IMAGE, with
 * e = |pred - gt| evaluated in fp32:
 *   [0] #mask  [1] #(gt > 0)  [2] sum e  [3] sum smooth_l1(e), beta 1  [4] #(e > 1)  [5] #(e > 2)  [6] #(e > 3)
 *   [7] #(e > 3 && e / |gt| > 0.05)
 * workspace: dca_disp_metrics_workspace(B, H, W) bytes. */
#define DCA_EVAL_REC 8
long dca_disp_metrics_workspace(int B, int H, int W);
int dca_disp_metrics(const float* pred, const float* gt, const unsigned char* mask, double* rec, void* workspace, int B,
                     int H, int W, int top_pad, int right_pad, float maxdisp, hipStream_t stream);
/* dca_region_confusion: nvol (1..3) volumes (B,C,hp,wp) fp32 at 1/8 resolution, gt (B,H,W).  With h = H / 8, w = W / 8
 * (integer division): label(i,j) = floor(adaptive_avg_pool2d(gt / 8, (h, w))) (main_dca.py:210; window
 * [floor(i H / h), ceil((i + 1) H / h)), summed row-major in fp32, one division), prediction = arg-max over C (lowest
 * index on ties) of the volume at row i + (hp - h), column j (main_dca.py:211-213: `argmax(1)[:, 1:, ...]` at 540 rows
 * padded to 544).  Labels outside [0, C) are skipped (main_dca.py:98-104).  cm: (nvol, C, C) int64, rows = label,
 * columns = prediction, counts of THIS call (zeroed by the launcher).  C <= DCA_EVAL_MAX_CLASSES. */
#define DCA_EVAL_MAX_CLASSES 64
int dca_region_confusion(const float* vol0, const float* vol1, const float* vol2, const float* gt, long long* cm,
                         int nvol, int B, int C, int hp, int wp, int H, int W, hipStream_t stream);
/* dca_eval_accumulate: adds one batch (rec of dca_disp_metrics, cm of dca_region_confusion) to the run state, a vector of
 * dca_eval_state_len(C) = DCA_EVAL_STATE_HEAD + 3 C C doubles that the caller zeroes at the start of a run.  Every entry
 * is a sum or a count, so the states of several ranks add up:
 *   [DCA_EVAL_BATCHES]         batches seen
 *   [DCA_EVAL_SUMS + 0..9]     sum over batches of the values `mytest` returns: loss (smooth-L1 mean), epe, 1px, 3px over
 *                              the batch's masked pixels; mpa0, mpa1, mpa2; mIoU0, mIoU1, mIoU2 (np.nanmean over classes:
 *                              0/0 classes left out).  Two quirks of the reference are kept: a batch with an empty mask
 *                              adds 0 to all ten and still counts (main_dca.py:177-195); the metric object is never reset
 *                              between the heads, so mpa1 / mIoU1 come from CM0 + CM1 and mpa2 / mIoU2 from
 *                              CM0 + CM1 + CM2 (main_dca.py:215-232)
 *   [DCA_EVAL_IMG_KEPT]        images that pass the 10 % rule of utils/metrics.py (mask mean / (gt > 0) mean >= 0.1, fp32)
 *                              and have a non-empty mask
 *   [DCA_EVAL_IMG_EPE], [DCA_EVAL_IMG_D1], [DCA_EVAL_IMG_THRES + 0..2]   sum over those images of the per-image EPE, D1,
 *                              Thres(1), Thres(2), Thres(3)
 *   [DCA_EVAL_IMG_SEEN]        images seen          [DCA_EVAL_PIXELS]  masked pixels seen
 *   [.. DCA_EVAL_STATE_HEAD)   reserved, zero
 *   [DCA_EVAL_STATE_HEAD + (k C + label) C + pred]   confusion matrix of head k alone, summed over the run
 * H, W: the size of the ground truth (for the 10 % rule). */
#define DCA_EVAL_BATCHES 0
#define DCA_EVAL_SUMS 1
#define DCA_EVAL_IMG_KEPT 11
#define DCA_EVAL_IMG_EPE 12
#define DCA_EVAL_IMG_D1 13
#define DCA_EVAL_IMG_THRES 14
#define DCA_EVAL_IMG_SEEN 17
#define DCA_EVAL_PIXELS 18
#define DCA_EVAL_STATE_HEAD 32
long dca_eval_state_len(int C);
int dca_eval_accumulate(const double* rec, const long long* cm, double* state, int B, int nvol, int C, int H, int W,
                        hipStream_t stream);

/* ---- inference frame I/O (frame_io.hip): my_img.py:47-110 around the model call, without host arithmetic ----------------
 * The normalisation of my_img.py:59-68 is per image and colour plane (p - mean) / std with the population std in fp64.  A
 * uint8 plane has 256 distinct values, so it is done as histogram -> 256-entry table -> look-up.  Integer atomics only:
 * every result is bitwise reproducible.
 *
 * dca_frame_hist: left, right (H,W,C) interleaved uint8, C = 3 or 4 (a fourth channel is ignored), H W < 2^31 ->
 * hist[2][3][256] counts (zeroed by the launcher). */
int dca_frame_hist(const unsigned char* left, const unsigned char* right, unsigned* hist, int H, int W, int C,
                   hipStream_t stream);
/* dca_frame_lut: hist and the pixel count n = H W -> lut[2][3][256] fp32 and stats[2][3][2] fp64 (mean, std), in this
 * operation order, without fused multiply-adds:  S = sum h[v] v (64-bit integers);  mean = double(S) / double(n);
 * var = (sum over v = 0..255 in this order of double(h[v]) * ((v - mean) * (v - mean))) / n;  std = sqrt(var);
 * lut[v] = float((double(v) - mean) / std).  A constant plane gives std = 0 and NaN at its value (0/0), as numpy does. */
int dca_frame_lut(const unsigned* hist, long n_pixels, float* lut, double* stats, hipStream_t stream);
/* dca_frame_apply: the rows x cols window of the source images that starts at row src_y0, column 0, looked up in
 * lut[2][3][256] (any table: dca_frame_lut's, or a fixed one) and written into the planar fp32 frames out_left,
 * out_right (3,Hc,Wc) at row dst_y0, column 0.  Every other frame element is written as +0.0: the frames need no
 * memset.  The window must fit the source (src_y0 + rows <= H, cols <= W) and the frame. */
int dca_frame_apply(const unsigned char* left, const unsigned char* right, const float* lut, float* out_left,
                    float* out_right, int H, int W, int C, int Hc, int Wc, int src_y0, int dst_y0, int rows, int cols,
                    hipStream_t stream);
/* dca_disp_export: the h x w window of pred (Hc,Wc) fp32 that starts at row y0, column 0 (my_img.py:105-108), as fp32
 * (bit copy) and / or as uint16(pred * scale) (my_img.py:110 with scale 256: fp32 product, truncated toward zero,
 * saturated to [0, 65535], NaN -> 0).  Either output may be NULL, not both. */
int dca_disp_export(const float* pred, float* out_f32, unsigned short* out_u16, int Hc, int Wc, int y0, int h, int w,
                    float scale, hipStream_t stream);

/* ---- training inputs (train_io.hip): the loaders' arithmetic after the decode (dataloader/datasets.py:221-254 SceneFlow,
 * :270-317 KITTI) -- photometric augmentation, crop, occlusion patch, ToTensor + Normalize, ground-truth crop and mask.
 * Brightness, gamma and contrast each map a byte to a byte, so an image needs ONE 256-entry table; only the contrast
 * mean depends on the pixels, and it comes from an exact integer sum.  Integer atomics only: bitwise reproducible.  No
 * host value is needed between the launches: each reads what the one before left in device memory.
 *
 * dca_train_luma_sum: left, right (H,W,C) interleaved uint8, C = 3 or 4, H W < 2^31; bg[2][256] the byte table of each
 * image (gamma o brightness).  S[i] = sum over pixels of (19595 R' + 38470 G' + 7471 B' + 32768) >> 16, X' = bg[i][X]:
 * the sum of PIL's convert("L") of the image after brightness and gamma.  S is zeroed by the launcher. */
int dca_train_luma_sum(const unsigned char* left, const unsigned char* right, const unsigned char* bg, long long* S, int H,
                       int W, int C, hipStream_t stream);
/* dca_train_tables: S of dca_train_luma_sum, n = H W, bg, the two contrast factors and a normalisation table
 * norm[2][3][256] -> U[2][256] bytes, U[i][v] = C_i[bg[i][v]], and T[2][3][256] fp32, T[i][ch][v] = norm[i][ch][U[i][v]].
 * mean_i = int(double(S_i) / double(n) + 0.5);  C_i[v] = blend(mean_i, v, f_i) as PIL's Blend.c: in fp32 without fused
 * multiply-add t = c + f * (v - c); for 0 <= f <= 1 the result is t truncated, otherwise 0 for t <= 0, 255 for t >= 255
 * and truncation in between.  Factors that are not finite are refused. */
int dca_train_tables(const long long* S, long n_pixels, const unsigned char* bg, float f_left, float f_right,
                     const float* norm, unsigned char* U, float* T, hipStream_t stream);
/* dca_train_patch_colour: colour[ch] = floor(sum of U[1][byte] over the th x tw window at (y1, x1) of the right image,
 * channel ch, / (th tw)), 3 bytes: `np.mean(np.mean(right_img, 0), 0)` assigned into a uint8 array (datasets.py:306).
 * sums: 3 64-bit integers of workspace. */
int dca_train_patch_colour(const unsigned char* right, const unsigned char* U, long long* sums, unsigned char* colour,
                           int H, int W, int C, int y1, int x1, int th, int tw, hipStream_t stream);
/* dca_train_crop_norm: the th x tw window at (y1, x1) of both images, looked up in T[2][3][256] (dca_train_tables', or a
 * fixed table: the SceneFlow loader), written to the planar fp32 slots out_left, out_right (3,th,tw) -- slot b of a
 * (B,3,th,tw) batch.  With ph, pw > 0 the rows [py0, py0 + ph) x columns [px0, px0 + pw) of the RIGHT crop are
 * norm[1][ch][colour[ch]] instead; the rectangle must lie inside the crop.  norm and colour may be NULL without a patch.
 * 16-byte stores when tw % 4 == 0 and both slots are 16-byte aligned, 4-byte stores otherwise. */
int dca_train_crop_norm(const unsigned char* left, const unsigned char* right, const float* T, const float* norm,
                        const unsigned char* colour, float* out_left, float* out_right, int H, int W, int C, int y1, int x1,
                        int th, int tw, int py0, int px0, int ph, int pw, hipStream_t stream);
/* dca_train_disp_crop: src (H,W) fp32 (src_u16 = 0) or uint16 (src_u16 = 1) -> gt (th,tw) fp32 = the window at (y1, x1)
 * times scale (1, or 1/256 for KITTI PNGs: exact; scale 1 copies the bits) and mask (th,tw) bytes = gt > 0 && gt < maxdisp
 * (main_dca.py:127; NaN gives 0).  flip_rows: the source is stored bottom-up (a PFM payload) and (y1, x1) addresses the
 * flipped image.  inf_to_zero: +inf becomes 0 (the Middlebury loaders). */
int dca_train_disp_crop(const void* src, int src_u16, float* gt, unsigned char* mask, int H, int W, int y1, int x1, int th,
                        int tw, int flip_rows, float scale, int inf_to_zero, float maxdisp, hipStream_t stream);

/* ---- per-pixel confidence from the disparity distribution (confidence.hip); inference only, no backward ------------------
 * The soft-max over the K = maxdisp/4 disparity bins that the soft-argmin reduces to one number (models/gwcnet_dca_g.py:
 * `logits3`) holds more: how sharp it is, and where its winning mode lies.  The reference computes none of this.
 *
 * dca_softargmin_stats: logits (B,K,HW) fp32 -> out (B,DCA_CONF_PLANES,HW) fp32.  Per pixel, with m = max_k x_k,
 * k* = the lowest k with x_k == m (taken on the logits: exact), e_k = expf(x_k - m), s = sum_k e_k and the window
 * Wn = {k : |k - k*| <= radius} clipped to [0, K-1]:
 *   [DCA_CONF_DISP]  sum_k k e_k / s                  the soft-argmin, bitwise dca_softargmin_fwd's mode 1 (one shared helper)
 *   [DCA_CONF_DUNI]  sum_Wn k e_k / sum_Wn e_k        the soft-argmin of the winning mode alone (1/4-res pixels)
 *   [DCA_CONF_MASS]  sum_Wn e_k / s                   the probability of that mode; radius 0: the peak probability
 *   [DCA_CONF_ENT]   (logf(s) - sum_k e_k (x_k - m) / s) / logf(K)   entropy in [0, 1]; 0 for K = 1.  No 0 log 0: an
 *                    underflowed e_k contributes 0, never NaN
 *   [DCA_CONF_STD]   sqrt(sum_k e_k (k - d)^2 / s), d = plane 0   (two passes; E[k^2] - d^2 would cancel)
 * radius >= 0; radius >= K means the whole range (DUNI = DISP up to rounding, MASS = 1).  K >= 1. */
#define DCA_CONF_DISP 0
#define DCA_CONF_DUNI 1
#define DCA_CONF_MASS 2
#define DCA_CONF_ENT 3
#define DCA_CONF_STD 4
#define DCA_CONF_PLANES 5
int dca_softargmin_stats(const float* logits, float* out, int B, int K, long HW, int radius, hipStream_t stream);
/* dca_convex_up4_planes: dca_convex_up4_fwd for P (1..DCA_CONF_MAX_PLANES) planes through ONE read of the mask logits:
 * mask_logits (B,144,h,w), planes (B,P,h,w), scales: HOST array of P floats -> up (B,P,4h,4w),
 * up_p = sum_k softmax_k(mask)[k,i,j] * scales[p] * planes_p[3x3 neighbour k].  The soft-max of a sub-pixel is computed
 * once and applied to every plane with the loads, product and accumulation order of dca_convex_up4_fwd: a plane with
 * scale 4 is bitwise that function's result.  Neighbours outside the map are 0 for EVERY plane (the reference's F.unfold
 * zero padding, which the disparity already gets): at the frame border a confidence plane falls exactly where the
 * disparity is pulled towards 0.  up must be 16-byte aligned. */
#define DCA_CONF_MAX_PLANES 8
int dca_convex_up4_planes(const float* mask_logits, const float* planes, const float* scales, float* up, int B, int P,
                          int h, int w, hipStream_t stream);
/* dca_conf_histogram: risk-coverage statistics.  conf, pred, gt: (B,HW) fp32; state: (nbins,3) int64 that the launch ADDS
 * into (the caller zeroes it at the start of a run; states of several ranks add up).  A pixel counts if
 * gt > 0 && gt < maxdisp && conf == conf;  bin = min(nbins - 1, (int)(clamp(conf, 0, 1) * nbins)) with the product in
 * fp32;  err = |pred - gt| in fp32;  state[bin] += { 1, (long long)(err * 1048576.f) truncated, err > 3 }.  The error
 * sum is kept in 2^-20 fixed point because integer sums do not depend on the order of the atomics: the state is bitwise
 * reproducible.  2 <= nbins <= DCA_CONF_MAX_BINS. */
#define DCA_CONF_MAX_BINS 1024
#define DCA_CONF_ERR_SCALE 1048576
int dca_conf_histogram(const float* conf, const float* pred, const float* gt, long long* state, int B, long HW, int nbins,
                       float maxdisp, hipStream_t stream);

/* ---- left-right consistency (lr_consistency.hip); inference only, no backward, no counterpart in the reference ------------
 * dca_mirror_pair: left, right (N,H,W) planar fp32 (N = B 3 for frames) -> out_left = flipW(right), out_right = flipW(left)
 * in one launch, as bit copies.  On this mirrored, swapped pair the unchanged network computes the RIGHT view's disparity
 * in mirrored coordinates: with R'(x) = R(W-1-x) and L'(x) = L(W-1-x), corr(R'(x), L'(x-d)) = corr(R(u), L(u+d)) at
 * u = W-1-x.  The outputs must not alias the inputs or each other.
 *
 * dca_lr_consistency: ONE launch, one workgroup per image row.  dl (B,H,W): the left disparity; drm (B,H,W): the right
 * disparity as the mirrored pass produced it -- right-image column i sits at index W-1-i, dR(i) = drm[W-1-i] (no un-flip
 * pass); tau: finite, >= 0; cols, 1 <= cols <= W: the active width -- only columns [0, cols) of either image take part (a
 * frame zero-padded on the right: the padding's disparity is never matched against and never a fill source).
 * Outputs diff, valid, filled, disp_right (B,H,W) fp32; any pointer except valid may be NULL.  Per pixel x < cols, d = dl[x]:
 *   xr = float(x) - d;  inview = d > 0 && xr >= 0;  i0 = floor(xr);  f = xr - i0;  i1 = min(i0 + 1, cols - 1);
 *   r = (1 - f) dR(i0) + f dR(i1)            (fp32, products and sum rounded separately)
 *   diff  = inview ? |d - r| : +inf          NaN when r is NaN; +inf when d is NaN (not in view)
 *   valid = diff <= tau ? 1.0 : 0.0          a NaN never becomes valid and is never a fill source
 *   filled: a valid pixel keeps dl bit for bit.  An invalid one, with l / rt the nearest valid column to its left / right
 *           within [0, cols): both exist -> min(dl[l], dl[rt]) (the occluded band belongs to the background: the KITTI
 *           devkit's background interpolation, rows only); one exists -> its value; none in the row -> dl, unchanged.
 *   disp_right[i] = dR(i): the right view's disparity in its own coordinates.
 * For x >= cols: valid = 0, diff = +inf, filled = dl, disp_right = drm[W-1-x].
 * W <= DCA_LR_MAX_W (both rows are staged in LDS: 2 W floats).  After the comparison everything is integer arithmetic or a
 * copy of an input value: bitwise reproducible. */
#define DCA_LR_MAX_W 8192
int dca_mirror_pair(const float* left, const float* right, float* out_left, float* out_right, int N, int H, int W,
                    hipStream_t stream);
int dca_lr_consistency(const float* dl, const float* drm, float* diff, float* valid, float* filled, float* disp_right,
                       int B, int H, int W, int cols, float tau, hipStream_t stream);

/* ---- geometry from calibrated disparity (geometry.hip); inference only, no backward, no counterpart in the reference -------
 * All functions work on ONE frame.  pred (Hc,Wc) fp32: the disparity; the window is rows x cols pixels starting at frame
 * row y0, column 0, as in dca_disp_export; mask (Hc,Wc) fp32 or NULL, indexed like pred (a confidence, a validity map).
 * Window pixel (r, c), i = r cols + c, has the image coordinates u = c, v = v0 + r (v0: the image row of window row 0 --
 * src_y0 of the placement for a cropped image).  With the calibration f (focal length, pixels), fb = float(f * baseline)
 * rounded once from fp64 by the host, the principal point (cx, cy) and doffs = cx_right - cx_left (0 for KITTI), in fp32,
 * every operation rounded on its own, IEEE division:
 *   den = d + doffs;   Z = fb / den;   X = ((float(u) - cx) * Z) / f;   Y = ((float(v) - cy) * Z) / f
 *   keep = d >= min_disp && den > 0 && Z > 0 && Z <= max_depth && (mask == NULL || mask >= mask_min)
 *          && r % stride == 0 && c % stride == 0
 * A NaN fails every comparison: NaN, +-inf and non-positive-denominator disparities are never kept.  Refused: a window
 * outside the frame, fb or f not positive and finite, min_disp < 0 or not finite, max_depth <= 0 or not finite, stride < 1,
 * cx, cy or doffs not finite, a NaN mask_min with a mask.
 *
 * dca_disp_to_depth: ONE launch -> the dense rows x cols depth map, Z where keep holds (stride 1), +0.0 elsewhere (the
 * KITTI depth convention), as fp32 and / or uint16(Z * scale) (fp32 product, truncated toward zero, saturated to
 * [0, 65535]; scale 256: the KITTI depth PNG; scale > 0, finite).  Either output may be NULL, not both.
 *
 * dca_point_cloud_tiles: ceil(rows cols / DCA_PC_TILE), the workgroups of the compaction; rows cols < 2^31 (0 otherwise).
 *
 * dca_point_cloud: the kept pixels as 16-byte records { float x, y, z; unsigned char r, g, b, a } -- the body of a binary
 * little-endian PLY file byte for byte -- compacted in row-major window order: record k is the k-th kept pixel by i.
 * rgb: the source image (Hsrc,Wsrc,C) interleaved uint8, C = 3 or 4, read at (v0 + r, c), or NULL: r = g = b = 255; a = 255
 * always.  vertices: room for cap records, 16-byte aligned (one 16-byte store per record); nothing is written at or
 * beyond record cap; cap = 0 is legal and vertices may then be NULL.  tile_offsets: tiles + 1 words of workspace AND
 * result: tile_offsets[t] = kept pixels with i < t DCA_PC_TILE, tile_offsets[tiles] = the total.  count: 2 words,
 * count[0] = total kept, count[1] = min(total, cap) = records written.
 * Three launches on the stream -- count per tile (wave ballots), exclusive scan of the tile counts by ONE workgroup,
 * rank and write per tile -- with the kernel boundaries as the only global synchronisation: no atomics, no flag one
 * workgroup polls for another, so the records and their order are bitwise reproducible and nothing can wait on a
 * workgroup that is not resident.  The window must also fit the source when rgb is given (v0 + rows <= Hsrc,
 * cols <= Wsrc). */
#define DCA_PC_TILE 1024
#define DCA_PC_RECORD_BYTES 16
int dca_disp_to_depth(const float* pred, const float* mask, float* out_f32, unsigned short* out_u16, int Hc, int Wc, int y0,
                      int rows, int cols, float fb, float doffs, float min_disp, float max_depth, float mask_min,
                      float scale, hipStream_t stream);
long dca_point_cloud_tiles(int rows, int cols);
int dca_point_cloud(const float* pred, const float* mask, const unsigned char* rgb, int C, int Hsrc, int Wsrc, void* vertices,
                    long cap, unsigned* tile_offsets, long long* count, int Hc, int Wc, int y0, int rows, int cols, int v0,
                    int stride, float f, float fb, float cx, float cy, float doffs, float min_disp, float max_depth,
                    float mask_min, hipStream_t stream);

/* ---- self-supervised loss (selfsup.hip): view synthesis + edge-aware smoothness -----------------------
 * Training without ground truth.  The smoothness term is the reference's util.py:76-86 `loss_disp_smoothness` (defined
 * there, never called); the view-synthesis term has no counterpart in the reference.
 * left = I, right = R: (B,3,H,W) planar fp32, used as given.  disps / gdisps / weights: HOST arrays of nlev
 * (<= DCA_SELFSUP_MAX_LEVELS) device pointers to (B,H,W) fp32 maps in full-resolution pixels / floats w_l.  valid: (B,H,W)
 * device, fp32 (valid_u8 = 0) or one byte per pixel, 0 / 1 (valid_u8 = 1), or NULL (all ones); it carries no gradient.
 * Per level, sample and pixel (y, x), d = d_l(b, y, x):
 *   xs = float(x) - d;  xc = clamp(xs, 0, W-1);  x0 = min(floor(xc), W-2);  t = xc - x0
 *   Y_c = R_c[y, x0] + t (R_c[y, x0+1] - R_c[y, x0]);   inview = 0 <= xs <= W-1   (false for a NaN)
 *   dY_c/dd = -(R_c[y, x0+1] - R_c[y, x0]) where 0 < xs < W-1, and 0 where xs is clamped
 * Photometric term, at interior pixels p (1 <= y <= H-2, 1 <= x <= W-2; the 3x3 window means carry no padding), per
 * channel c with mu = the window mean, var_I = E[I^2] - mu_I^2, var_Y, cov = E[IY] - mu_I mu_Y (evaluated around the
 * window means: the same numbers without the cancellation):
 *   SSIM_c = (2 mu_I mu_Y + c1)(2 cov + c2) / ((mu_I^2 + mu_Y^2 + c1)(var_I + var_Y + c2))
 *   e(p) = alpha mean_c clamp((1 - SSIM_c) / 2, 0, 1) + (1 - alpha) mean_c |I_c - Y_c|
 *   M(p) = inview(p) valid(p)      only the centre pixel is masked; a window may contain clamped samples
 *   photo_l = sum M e / max(sum M, 1)                    sum M is a constant for the gradient
 * Smoothness term, over all H (W-1) horizontal and (H-1) W vertical pairs, independent of valid:
 *   wx(p) = exp(-mean_c |I_c(p) - I_c(p + x^)|), wy likewise;
 *   smooth_l = (sum |d(p) - d(p + x^)| wx + sum |d(p) - d(p + y^)| wy) / (sum wx + sum wy)
 * total = sum_l w_l (photo_scale photo_l + lam smooth_l); photo_scale = 1, or 0: the smoothness term alone, in which case
 * right and valid are not read.  The gradient of |.| at 0 and of the clamps at their ends is 0.
 *
 * dca_selfsup_loss_fwd: TWO launches.  (1) grid (tiles, B, nlev), tiles = ceil(H / DCA_SELFSUP_TILE_H) ceil(W /
 * DCA_SELFSUP_TILE_W): a tile with a one-pixel halo in LDS per channel; the warped image is recomputed, never stored; every
 * workgroup writes DCA_SELFSUP_SUMS doubles (sum M e, sum M, sum |dd| w, sum w) to work, which holds
 * nlev B tiles DCA_SELFSUP_SUMS doubles.  (2) one workgroup adds them in a fixed order and writes out, nlev DCA_SELFSUP_OUT + 1
 * floats: per level (photo_l, smooth_l, sum M, 1 / max(sum M, 1), 1 / (sum wx + sum wy)), then the total.
 * dca_selfsup_loss_bwd: ONE launch, the same tiles with a two-pixel halo; `out` is the forward's, unchanged; gloss: one
 * device float, the incoming gradient.  gdisps[l] = gloss d total / d d_l, every element written exactly once; the gradient
 * at p collects (dS/dmu_Y + 2 Y_p dS/dE[Y^2] + I_p dS/dE[IY]) / 9 from the (up to nine) interior windows that contain p.
 * gdisps[l] must not alias disps[l].
 * No atomics and no host synchronisation: loss and gradients are bitwise reproducible, the launches graph-capturable.
 * Refused: H < 3, W < 3, W > 2^24, 3 H W >= 2^31 (offsets inside a sample are 32-bit), B > 65535, nlev outside
 * [1, DCA_SELFSUP_MAX_LEVELS], alpha outside [0, 1], c1 or c2 not positive, NaN lam or photo_scale, NULL pointers. */
#define DCA_SELFSUP_MAX_LEVELS 8
#define DCA_SELFSUP_TILE_W 64
#define DCA_SELFSUP_TILE_H 16
#define DCA_SELFSUP_SUMS 4
#define DCA_SELFSUP_OUT 5
int dca_selfsup_loss_fwd(const float* left, const float* right, const float* const* disps, const float* weights, int nlev,
                         const void* valid, int valid_u8, double* work, float* out, int B, int H, int W, float alpha,
                         float lam, float c1, float c2, float photo_scale, hipStream_t stream);
int dca_selfsup_loss_bwd(const float* left, const float* right, const float* const* disps, float* const* gdisps,
                         const float* weights, int nlev, const void* valid, int valid_u8, const float* out,
                         const float* gloss, int B, int H, int W, float alpha, float lam, float c1, float c2,
                         float photo_scale, hipStream_t stream);

/* ---- stereo rectification of a raw pair (rectify.hip); inference only, no counterpart in the reference --
 * dca_rectify_pair: ONE launch remaps both images.  left, right: (Hs,Ws,C) interleaved uint8, C = 3 or 4; out_left,
 * out_right: (Hd,Wd,C); maps: four planes of map_plane words each, X_left, Y_left, X_right, Y_right, the first Hd Wd words
 * of a plane the source coordinates of the destination pixels in row-major order with DCA_RECT_FRAC_BITS fractional bits
 * (geometry.RectifyMaps builds them on the host); map_plane >= Hd Wd and a multiple of 4, so that a 16-byte aligned maps
 * keeps every 4-pixel group of every plane aligned.  Per destination pixel with map entry (X, Y):
 *   x0 = X >> 5, a = X & 31, y0 = Y >> 5, b = Y & 31        (arithmetic shift; any int32 is legal)
 *   out_c = ((32-a)(32-b) p(y0,x0) + a(32-b) p(y0,x0+1) + (32-a) b p(y0+1,x0) + a b p(y0+1,x0+1) + 512) >> 10,  c < 3
 * where p(r, x) is source byte c of pixel (r, x) and 0 outside [0,Hs) x [0,Ws) (constant-zero border); a fourth channel is
 * written as 255.  Integer arithmetic only, no atomics: bitwise defined (geometry.rectify_pair_host is the numpy
 * restatement).  A thread writes 4 consecutive destination pixels as one 12- / 16-byte group when maps is 16-byte aligned and
 * the view's output base is 4-byte (C = 3) / 16-byte (C = 4) aligned, byte by byte otherwise and at the image's tail.
 * Refused: NULL pointers, C outside {3, 4}, non-positive sizes, Hs or Ws > DCA_RECT_MAX_SRC, an image of 2^31 bytes or more
 * (offsets are 32-bit).  The outputs must not alias the inputs or each other. */
#define DCA_RECT_FRAC_BITS 5
#define DCA_RECT_MAX_SRC 16384
int dca_rectify_pair(const unsigned char* left, const unsigned char* right, const int* maps, long map_plane,
                     unsigned char* out_left, unsigned char* out_right, int Hs, int Ws, int Hd, int Wd, int C,
                     hipStream_t stream);

/* ---- pictures of a disparity map (visualize.hip): uint8 RGB next to the maps, no host round trip -----
 * Everything below is evaluated in fp32, every operation rounded on its own (no fused multiply-adds), IEEE division, so the
 * results are bitwise defined; tests/_vis_reference.py is the numpy restatement.  No atomics.
 *
 * dca_disp_error_image: ONE launch, the reference's disp_error_image_func.forward (utils/visualization.py:31-55).  pred
 * (B,H+top_pad,W+right_pad) fp32 -- the padded frame, cropped `[:, top_pad:, :W]` by addressing as dca_disp_metrics does --
 * gt (B,H,W) fp32.  Per pixel:
 *   mask = gt > 0;   e = |gt - pred|;   err = min(e / abs_thres, (e / gt) / rel_thres)      (a NaN stays a NaN, as np.minimum)
 *   bin i of DCA_ERRMAP_BINS has 2^(i-5) <= err < 2^(i-4), bin 0 starting at 0 and the last one open: the edges
 *   0, 1/16, 1/8, 1/4, 1/2, 1, 2, 4, 8, 16, +inf of visualization.py:13-22; its colour is DCA_ERRMAP_RGB_i (0xRRGGBB)
 * A pixel outside the mask, or whose err lies in no bin (NaN; +inf, because inf < inf is false) is black.  With legend = 1
 * the pixels of rows < DCA_ERRMAP_LEGEND_ROWS and columns < DCA_ERRMAP_BINS DCA_ERRMAP_LEGEND_STEP take the colour of bin
 * column / DCA_ERRMAP_LEGEND_STEP, over everything else, clipped to the image (visualization.py:51-53).  The reference's
 * dilate_radius is a TODO there and has no counterpart here.
 * out_f32: planar (B,3,H,W), float(byte) / 255.0f (the reference's layout and values); out_u8: interleaved (B,H,W,3), the
 * byte itself (what an image encoder takes).  Either may be NULL, not both.  Refused: NULL inputs, non-positive sizes,
 * negative pads, B (H + top_pad) (W + right_pad) >= 2^31, thresholds that are not positive and finite, legend outside {0, 1}. */
#define DCA_ERRMAP_BINS 10
#define DCA_ERRMAP_RGB_0 0x313695
#define DCA_ERRMAP_RGB_1 0x4575B4
#define DCA_ERRMAP_RGB_2 0x74ADD1
#define DCA_ERRMAP_RGB_3 0xABD9E9
#define DCA_ERRMAP_RGB_4 0xE0F3F8
#define DCA_ERRMAP_RGB_5 0xFEE090
#define DCA_ERRMAP_RGB_6 0xFDAE61
#define DCA_ERRMAP_RGB_7 0xF46D43
#define DCA_ERRMAP_RGB_8 0xD73027
#define DCA_ERRMAP_RGB_9 0xA50026
#define DCA_ERRMAP_LEGEND_ROWS 10
#define DCA_ERRMAP_LEGEND_STEP 20
int dca_disp_error_image(const float* pred, const float* gt, float* out_f32, unsigned char* out_u8, int B, int H, int W,
                         int top_pad, int right_pad, float abs_thres, float rel_thres, int legend, hipStream_t stream);
/* dca_disp_range: disp (B,Hc,Wc) fp32, mask (B,Hc,Wc) fp32 or NULL; the window is rows x cols pixels from row y0, column 0
 * of every image, as in dca_disp_export.  range: (B,2) fp32 = (lo, hi), the minimum and maximum over the window's VALID
 * pixels: finite, > 0 and, with a mask, mask >= mask_min; (0, 0) for an image without one.  TWO launches: one (min, max) pair
 * per workgroup into workspace (dca_disp_range_workspace(B, rows, cols) bytes), then one wave per image; min and max do not
 * depend on the order, so the result is bitwise reproducible.  B <= 65535, B Hc Wc < 2^31. */
long dca_disp_range_workspace(int B, int rows, int cols);
int dca_disp_range(const float* disp, const float* mask, float* range, void* workspace, int B, int Hc, int Wc, int y0,
                   int rows, int cols, float mask_min, hipStream_t stream);
/* dca_disp_colorize: ONE launch colours the rows x cols window at row y0, column 0 of ONE map disp (Hc,Wc) fp32 into out_u8
 * (rows,cols,3) interleaved.  The range is the device pair range = (lo, hi) dca_disp_range wrote (nothing is read back), or,
 * with range NULL, lo = 0 and hi = max_disp (> 0, finite: the KITTI devkit's min(D / max_disp, 1)).  A pixel that is not
 * valid (as in dca_disp_range) is (0,0,0); for the others, in this operation order,
 *   t = min(max((d - lo) / max(hi - lo, 1e-5f), 0), 1)
 *   DCA_CMAP_GRAY:   r = g = b = rintf(t * 255)
 *   DCA_CMAP_KITTI:  the devkit's disp_to_color.  s = t * 1000; C[k] = DCA_KITTI_EDGE_k, k = 0..7; ind = the number of k in
 *                    1..6 with s > C[k];  w = (s - C[ind]) / (C[ind + 1] - C[ind])  (the widths 114, 185, 114, 174, 114, 185,
 *                    114 are exact);  corner k is nibble k of DCA_KITTI_CORNERS, bits (r g b): 000, 001, 100, 101, 010, 011,
 *                    110, 111;  a channel whose corners ind and ind + 1 agree has that value v, a rising one v = w, a falling
 *                    one v = 1 - w;  byte = rintf(v * 255)
 * A range that is not finite gives unspecified colours, never a fault. */
#define DCA_CMAP_GRAY 0
#define DCA_CMAP_KITTI 1
#define DCA_KITTI_EDGE_0 0
#define DCA_KITTI_EDGE_1 114
#define DCA_KITTI_EDGE_2 299
#define DCA_KITTI_EDGE_3 413
#define DCA_KITTI_EDGE_4 587
#define DCA_KITTI_EDGE_5 701
#define DCA_KITTI_EDGE_6 886
#define DCA_KITTI_EDGE_7 1000
#define DCA_KITTI_CORNERS 0x76325410
int dca_disp_colorize(const float* disp, const float* mask, const float* range, unsigned char* out_u8, int Hc, int Wc, int y0,
                      int rows, int cols, float max_disp, float mask_min, int cmap, hipStream_t stream);

/* ---- sparse ground truth from a LiDAR scan (lidar.hip); no counterpart in the reference ----------------
 * dca_lidar_disparity: ONE scan -> sparse maps in the rectified left image.  points: (N,S) fp32 on the device, S >= 3 floats
 * per row; only the leading n <= N rows and their first three columns (X, Y, Z in the LiDAR frame) are read (a KITTI scan
 * has S = 4, the fourth column being the reflectance).  m00 .. m23: the 3x4 matrix of geometry.LidarCalib, LiDAR
 * coordinates -> homogeneous pixels of the rectified left camera, formed in fp64 and rounded once by the host.  In fp32,
 * every operation rounded on its own (no fused multiply-adds), IEEE division, per point:
 *   x = ((m00 X + m01 Y) + m02 Z) + m03        (y and z likewise from rows 1 and 2)
 *   u = x / z;  v = y / z;  uf = floorf(u + 0.5f);  vf = floorf(v + 0.5f)
 *   keep = z >= min_depth && z <= max_depth && uf >= 0 && uf < float(W) && vf >= 0 && vf < float(H)
 * All comparisons are made in float before anything is converted to int: a NaN fails them, an infinity or 1e30 fails
 * them without overflowing an int.  Kept points go into a z-buffer, zbuf[vf W + uf] = the minimum z over the points of
 * the pixel, cleared to the bits of +inf; the minimum is the INTEGER atomicMin on the bit pattern (positive floats order
 * as their bits do), which does not depend on the order of arrival: the maps are the same bits on every run and for
 * every order of the points.
 * Hidden points, per pixel (r, c) with a finite z = zbuf[r, c]: zmin = the minimum of zbuf over rows r-ry .. r+ry and
 * columns c-rx .. c+rx clipped to the image (the pixel itself included);  visible = z <= zmin * occl_scale  with
 * occl_scale = float(1.0 + rel), formed in fp64 and rounded once.  rx = ry = 0 switches the test off (zmin = z).
 *   d = fb / z - doffs;   valid = visible && d >= min_disp && d < max_disp
 * Outputs, (H,W) each; any may be NULL, not all four:
 *   disp      fp32: d at a valid pixel, +0.0 elsewhere (the KITTI convention: mask = gt > 0 && gt < maxdisp)
 *   depth     fp32: z at a valid pixel, +0.0 elsewhere
 *   disp_u16  the KITTI disparity PNG payload: q = d * 256.0f + 0.5f truncated toward zero, saturated to 65535 and at least
 *             1 at a valid pixel; 0 elsewhere
 *   count     2 words: count[0] = valid pixels, count[1] = points that passed keep; integer atomics, one per workgroup
 *             (wave ballots, summed in LDS: thousands of atomics on one word serialise)
 * zbuf: H W words of workspace, 4-byte aligned, the caller's; after the call it holds the z-buffer.
 * THREE launches on the stream: fill zbuf and zero count; scatter the points; resolve every pixel (a workgroup stages
 * a tile of zbuf with the halo in LDS and takes the window minimum along rows, then along columns; eight workgroups per CU
 * walk the tiles).  Everything is
 * passed by value; the host never waits.
 * Refused: n > N, negative n or N, S < 3, n S >= 2^31, non-positive H or W, H W >= 2^31, rx or ry outside
 * [0, DCA_LIDAR_MAX_RADIUS], rel < 0 or not finite, min_depth <= 0, max_depth < min_depth or not finite, min_disp or max_disp
 * not finite, max_disp < min_disp, fb not positive and finite, doffs not finite, a matrix entry that is not finite, NULL
 * points with n > 0, NULL zbuf, four NULL outputs. */
#define DCA_LIDAR_MAX_RADIUS 8
int dca_lidar_disparity(const float* points, long N, int S, long n, float m00, float m01, float m02, float m03, float m10,
                        float m11, float m12, float m13, float m20, float m21, float m22, float m23, int H, int W, float fb,
                        float doffs, float min_depth, float max_depth, float min_disp, float max_disp, int rx, int ry,
                        double rel, float* disp, float* depth, unsigned short* disp_u16, long long* count, unsigned* zbuf,
                        hipStream_t stream);

/* ---- disparity post-filter (postfilter.hip); inference only, no backward, no counterpart in the reference
 * d (B,Hc,Wc) fp32: B independent disparity maps; the window is rows x cols pixels starting at frame row y0, column 0 of every
 * image, as in dca_disp_export; mask (B,Hc,Wc) fp32 or NULL, indexed like d.  Nothing outside the window is ever read as a
 * neighbour.  A window pixel is ACTIVE iff d is finite (not NaN, |d| < inf) and (mask == NULL || mask >= mask_min); -0.0 is
 * a finite value and active.  Outputs are (B,rows,cols).
 *
 * dca_speckle_filter (max_size >= 0; max_diff finite, >= 0): two 4-neighbours inside the window are joined iff both are
 * active and fabsf(a - b) <= max_diff, the subtraction rounded to fp32; equality joins, the relation is symmetric and it
 * is chained -- a ramp with small steps is ONE component.  Components are the connected components of that graph.
 *   size  (int32)  the pixel's component size, 0 for an inactive pixel
 *   valid (fp32)   1.0 where active and size > max_size, 0.0 elsewhere          (max_size = 0: the identity on active pixels)
 *   disp  (fp32)   the input bit for bit where valid, `fill` elsewhere          (+0.0: the project's "no measurement")
 * out_disp and out_size may be NULL; out_valid is always written.  label, count: rows cols B int32 words of workspace
 * each, the caller's; every call writes all of them before it reads any (no clearing between calls).
 * FOUR launches on the stream (three when the window is a single tile), kernel boundaries being the only global
 * synchronisation: (1) one workgroup per DCA_SPK_TILE_H x DCA_SPK_TILE_W tile labels the tile in LDS: label = the window
 * index r cols + c of the pixel's tile-local root, -1 for an inactive pixel, count = the local component's size at that
 * root; (2) the pixel pairs across tile edges unite in global memory; (3) every tile-local root that is not the global
 * root adds its count there, ONE integer atomic per (tile, local component); (4) every pixel reads its root's count.
 * Label invariant: labels only ever decrease, label[x] <= x always, label[x] == x defines a root: every walk to a root
 * strictly descends, every retry of a union strictly lowers one index, no loop waits for another workgroup.  In launch 2
 * every label access is an agent-scope atomic (workgroups on different XCDs share the labels); there are no flags, no
 * tickets, no spin-waits.  After the comparison everything is integer arithmetic or a copy of an input value: bitwise
 * reproducible, whatever the execution order.
 *
 * dca_median_filter (ksize 3 or 5): ONE launch, tile and halo in LDS.  For an active centre the candidates are the active
 * pixels of the ksize x ksize neighbourhood that lie inside the window (no border replication); with n of them the output
 * is the candidate of rank (n - 1) / 2 (0-based, ascending: the lower median for even n) in the total order of the bit key
 * b ^ ((b >> 31) | 0x80000000) (arithmetic shift; -0.0 < +0.0).  The output is an input value bit for bit; an inactive
 * centre is copied unchanged.  out must not alias d.
 * Refused: NULL d / out_valid / label / count / out, B outside [1, 65535], a window outside the frame, Hc Wc >= 2^31,
 * rows cols >= 2^31 (label offsets are 32-bit), max_size < 0, max_diff negative or not finite, ksize outside {3, 5}, a NaN
 * mask_min with a mask.  No launch synchronises or allocates. */
#define DCA_SPK_TILE_H 16
#define DCA_SPK_TILE_W 64
int dca_speckle_filter(const float* d, const float* mask, float* out_disp, float* out_valid, int* out_size, int* label,
                       int* count, int B, int Hc, int Wc, int y0, int rows, int cols, int max_size, float max_diff,
                       float mask_min, float fill, hipStream_t stream);
int dca_median_filter(const float* d, const float* mask, float* out, int B, int Hc, int Wc, int y0, int rows, int cols,
                      int ksize, float mask_min, hipStream_t stream);

/* ---- high-resolution pairs (highres.hip): integer-factor area downscale in front of the network,
 * joint bilateral upsampling of its disparity behind it.  The downscales are the arithmetic of the reference's
 * myImageFloder_middlebury_additional (dataloader/datasets.py:547-673); the upsampler has no counterpart there.  Everything
 * in fp32 is evaluated one operation at a time (no fused multiply-adds), divisions are IEEE: the results are bitwise
 * defined, dcanet_amd/highres.py holds the numpy restatements.  No atomics, no launch synchronises or allocates.
 *
 * With a factor s in 2..DCA_HR_MAX_SCALE an (H,W) image has h = ceil(H / s) rows and w = ceil(W / s) columns of blocks;
 * block (j,i) holds the pixels (y,x) with y / s == j, x / s == i that exist: cnt = (min(H, (j+1) s) - j s) *
 * (min(W, (i+1) s) - i s) of them, fewer than s s in the last partial row or column.
 *
 * dca_area_downscale_u8: ONE launch for both images of a pair.  left, right (H,W,C) uint8 interleaved, C = 3 or 4;
 * out (2,h,w,C) uint8 (left, then right).  Per byte of every channel (a fourth channel is averaged like the others):
 *   out = (sum + cnt / 2) / cnt        in integers, sum over the block's pixels
 * For a full 2x2 block this is (a + b + c + d + 2) >> 2, what OpenCV's INTER_AREA gives for uint8 at fx = fy = 0.5.
 *
 * dca_area_downscale_f32: one map (H,W) fp32 -> (h,w) fp32:
 *   sum = the block's pixels added in row-major order, starting from the first one;  out = (sum / float(cnt)) / float(s)
 * (the mean of the disparities, then the change of unit to pixels of the small image: datasets.py:593-604 resizes, then
 * multiplies by resize_scale).  inf_to_zero = 1: an out that is not finite (an infinity or a NaN anywhere in the block)
 * becomes +0.0 -- the mean is taken with the infinities in it and zeroed afterwards, as the reference does.  flip_rows = 1:
 * the source is a bottom-up PFM payload, row y of the image is stored row H - 1 - y.
 *
 * dca_guided_upsample: ONE frame, ONE launch: joint bilateral upsampling (Kopf et al. 2007) of the network's disparity
 * under the full-resolution left image.  disp_lo (Hc,Wc) fp32, the padded network frame, of which the window of rows x cols
 * pixels at frame row y0, column 0 is the image (as in dca_disp_export); mask_lo (Hc,Wc) fp32 or NULL, indexed like disp_lo;
 * guide_lo (rows,cols,C) uint8, the downscaled left image; guide_hi (H,W,C) uint8 with ceil(H / s) == rows and
 * ceil(W / s) == cols; ws (s, 2r+1) fp32 and wr (DCA_HR_RANGE_LEN) fp32, the spatial and range tables (the host computes
 * them: no transcendental function is evaluated on the device); r in 1..DCA_HR_MAX_RADIUS.  For the output pixel (y,x):
 *   j = y / s;  i = x / s;  py = y % s;  px = x % s;  num = den = 0
 *   for a = -r..r (outer), b = -r..r (inner), in that order: the tap (j+a, i+b) is ACTIVE iff it lies inside the window,
 *   its disparity d is finite and > 0 and (mask_lo == NULL || mask_lo >= mask_min).  For an active tap
 *     k = |dR| + |dG| + |dB| between guide_hi[y,x] and guide_lo[j+a,i+b]          (an integer in 0..765; alpha is ignored)
 *     wgt = (ws[py][a+r] * ws[px][b+r]) * wr[k];   num = num + wgt * d;   den = den + wgt
 *   den > 0:  out = (num / den) * float(s), valid = 1.0;   otherwise out = +0.0, valid = 0.0
 * Nothing outside the window is ever read as a tap.  out, valid: (H,W) fp32, either may be NULL, not both.
 * One workgroup of DCA_HR_THREADS threads per tile of DCA_HR_TILE_H x DCA_HR_TILE_W output pixels; every thread owns
 * DCA_HR_RUN consecutive columns of one row.
 * Refused: NULL inputs or tables, s outside [2, DCA_HR_MAX_SCALE], r outside [1, DCA_HR_MAX_RADIUS], C outside {3, 4},
 * non-positive sizes, H W >= 2^31 or Hc Wc >= 2^31 (pixel offsets are 32-bit), a window outside the frame, a guide_hi whose
 * block counts are not (rows, cols), a NaN mask_min with a mask, two NULL outputs, an output that is an input. */
#define DCA_HR_MAX_SCALE 4
#define DCA_HR_MAX_RADIUS 3
#define DCA_HR_RANGE_LEN 766
#define DCA_HR_THREADS 256
#define DCA_HR_TILE_H 16
#define DCA_HR_TILE_W 64
#define DCA_HR_RUN 4
int dca_area_downscale_u8(const unsigned char* left, const unsigned char* right, unsigned char* out, int H, int W, int C,
                          int s, hipStream_t stream);
int dca_area_downscale_f32(const float* in, float* out, int H, int W, int s, int inf_to_zero, int flip_rows,
                           hipStream_t stream);
int dca_guided_upsample(const float* disp_lo, const float* mask_lo, const unsigned char* guide_lo,
                        const unsigned char* guide_hi, const float* ws, const float* wr, float* out, float* valid, int Hc,
                        int Wc, int y0, int rows, int cols, int H, int W, int C, int s, int r, float mask_min,
                        hipStream_t stream);

/* ---- guided stereo (guided.hip, volume_fused.hip): sparse disparity hints (a LiDAR scan projected by
 * dca_lidar_disparity) modulate the cost volume along the disparity axis (Poggi et al., CVPR 2019).  Nothing in the
 * reference corresponds to it.  No atomics, no launch synchronises or allocates.
 *
 * A full-resolution hint h is VALID iff 0 < h < maxdisp (a NaN or an infinity is not).
 *
 * dca_hints_to_quarter: hints (B,h,w) fp32 -> hints4 (B, Hc/4, Wc/4) fp32 over the network's Hc x Wc frame, Hc % 4 == 0,
 * Wc % 4 == 0.  The image window is rows x cols pixels from source row src_y0, column 0, at frame row dst_y0, column 0 (as
 * in dca_frame_apply).  Cell (Y,X) looks at the frame pixels 4Y..4Y+3 x 4X..4X+3 that lie inside the window:
 *   hints4 = 0.25f * max(valid h in the block),   +0.0 if the block holds none
 * (the largest disparity is the nearest surface).  Every cell is written.  count (int64, may be NULL) receives the number of
 * cells > 0, by a second launch of one workgroup that sums integers in a fixed order.
 *
 * The factor of disparity bin d (an integer) at a cell with the hint h4, for k > 0 and i2c2 = 1 / (2 c^2) > 0:
 *   m(d, h4) = h4 > 0 ?  k * expf(-((d - h4) * (d - h4)) * i2c2)  :  1.0f         every product rounded on its own
 * (csrc/guided_math.h, the one definition both routes below call).
 *
 * dca_volume_modulate: out[b,c,d,y,x] = in[b,c,d,y,x] * m(d, hints4[b,y,x]) on an fp32 (B,C,D,H,W) tensor; out == in is
 * allowed (in place), any other overlap is not.  16-byte accesses when W % 4 == 0 and all three pointers are 16-byte
 * aligned, single floats otherwise; a thread owns (b, d, y, x quad) and walks the C channels with its factors in registers.
 *
 * dca_cost_volume_guided_fwd: dca_cost_volume_fwd with every channel of the volume multiplied by m in the builders' inner
 * loops, before the store's rounding and before the per-row maxima of vmax are taken.  Same arguments and requirements;
 * hints4 (B,H,W) fp32, 16-byte aligned.  The fp32 result is bitwise dca_cost_volume_fwd followed by dca_volume_modulate. */
int dca_hints_to_quarter(const float* hints, float* hints4, long* count, int B, int h, int w, int Hc, int Wc, int src_y0,
                         int dst_y0, int rows, int cols, float maxdisp, hipStream_t stream);
int dca_volume_modulate(const float* in, const float* hints4, float* out, int B, int C, int D, int H, int W, float k,
                        float i2c2, hipStream_t stream);
int dca_cost_volume_guided_fwd(const float* const* refs, const float* const* tgts, const int* seg_channels, int nseg,
                               const float* cref, const float* ctgt, int Cc, void* vol, int B, int H, int W, int maxdisp,
                               int num_groups, int dtype, unsigned* vmax, const float* hints4, float k, float i2c2,
                               hipStream_t stream);

/* ---- ground plane, obstacles and free space from disparity (ground.hip, ground_math.h); inference
 * only, no backward, no counterpart in the reference.  dcanet_amd/ground.py holds the numpy restatements.
 * d (B,Hc,Wc) fp32: B independent disparity maps; the window is rows x cols pixels starting at frame row y0, column 0 of every
 * image, as in dca_speckle_filter; mask (B,Hc,Wc) fp32 or NULL, indexed like d.  NB = max_disp, R = rows.  Every fp32 and
 * fp64 formula below is evaluated one operation at a time (no fused multiply-adds), IEEE division and square root; every
 * accumulation is an integer count or an integer sum (LDS and agent-scope integer atomics, whose result does not depend
 * on the order); there is no floating-point atomic: every output is bitwise defined.
 *
 * A window pixel (r, c) with the disparity d is VALID iff, in this order,
 *   d >= min_disp                           (false for a NaN and for -inf; min_disp >= 0)
 *   t = d * 16.0f + 0.5f;  t < float(16 NB)  (false for +inf);   q = (int)t, the disparity in sixteenths;  bin = q >> 4 < NB
 *   mask == NULL || mask >= mask_min
 *
 * dca_ground_plane.
 * (a) v-disparity (Labayrade et al. 2002): vdisp[b, r, bin] (int32, rows x NB per image) = the number of valid pixels of
 *     window row r in that bin.  One wave per row, the row's histogram in LDS; every word of vdisp is written.
 * (b) line by Hough vote.  Candidates are the integer pairs (d_top, d_bot), the line's disparity at window row 0 and at row
 *     R-1:  d_top in [-NB, NB), d_bot in [1, NB), d_bot - d_top >= min_rise (a wall draws a vertical line: no rise).  So
 *     the horizon lies above the window (d_top >= 0) or in it at or above the row where a line from -NB at the top reaches
 *     0 -- in the upper half whenever d_bot <= NB; a horizon further down is not found.
 *       bin(r) = floor_div(2 (d_top (R-1-r) + d_bot r) + (R-1), 2 (R-1))       floor division: negative above the horizon
 *       vote   = sum of vdisp[r, bin(r)] over the fit rows r in [r_lo, r_hi) with 0 <= bin(r) < NB
 *     The best candidate has the largest vote; ties go to the smallest d_bot, then the smallest d_top: the unsigned
 *     maximum of  vote << 32 | ~(d_bot 2 NB + d_top + NB)  (32 bits).  best vote < min_votes: status 1, nothing is refined.
 * (c) `refine` rounds of least squares with roll for  d = a u' + b v' + c,  u' = c - cols / 2, v' = r - rows / 2 (integer
 *     divisions).  The inliers of a round are the valid pixels of the fit rows with fabsf(d - p) <= tol in fp32, where
 *       round 0:  p = (float(d_top) * float(R-1-r) + float(d_bot) * float(r)) / float(R-1)
 *       later:    p = (a32 * float(u') + b32 * float(v')) + c32,   a32 = (float)a etc.: the record's doubles rounded once
 *     Over them the ten int64 sums  S = { n, Su, Sv, Sq, Suu, Suv, Svv, Suq, Svq, Sqq }  (u = u', v = v', q as above) are
 *     formed exactly, and one thread solves in fp64, with the sums converted to double, in exactly this order:
 *       c00 = Svv n - Sv Sv;   c01 = Suv n - Sv Su;   c02 = Suv Sv - Svv Su
 *       c11 = Suu n - Su Su;   c12 = Suu Sv - Suv Su; c22 = Suu Svv - Suv Suv
 *       det = (Suu c00 - Suv c01) + Su c02
 *       A = ((Suq c00 - Svq c01) + Sq c02) / det;  B = ((Svq c11 - Suq c01) - Sq c12) / det
 *       C = ((Suq c02 - Svq c12) + Sq c22) / det
 *       rss = Sqq - ((A Suq + B Svq) + C Sq);   ms = rss / n;   rms = sqrt(ms > 0 ? ms : 0) / 16
 *       a = A / 16;  b = B / 16;  c = C / 16
 *     n < min_inliers or not det > 0 (the Gram determinant is never negative in exact arithmetic): status 2, the record
 *     keeps the last good plane and the remaining rounds do nothing.  The plane before round 0 is the Hough line:
 *       a = 0;  b = double(d_bot - d_top) / double(R-1);  c = double(d_top) + b * double(rows / 2)
 * Plane record, DCA_GROUND_PLANE_LEN doubles per image:
 *   [0] a  [1] b  [2] c  [3] inliers of the record's plane (0: the Hough line)  [4] their rms residual, pixels
 *   [5] status: 0 fitted, 1 no line (best vote < min_votes), 2 a refinement round failed  [6] d_top  [7] d_bot
 *   [8] best vote  [9] hs  [10..12] the unit normal  [13] cols / 2  [14] rows / 2  [15] refinement rounds that succeeded
 * With calibrated = 1, f, baseline, cx, cy, doffs and v0 (the image row of window row 0) as doubles: in the image
 * coordinates u = col, v = v0 + row the plane is  den = d + doffs = a u + b v + c_img, in the camera frame
 * a X + b Y + nz Z = baseline:
 *   c_img = ((c - a * [13]) - b * (v0 + [14])) + doffs;   nz = ((a * cx + b * cy) + c_img) / f
 *   norm = sqrt((a * a + b * b) + nz * nz);   hs = baseline / norm (the camera's height above the plane, metres);
 *   normal = (a / norm, b / norm, nz / norm);   not norm > 0, or calibrated = 0:  hs = 0 and normal = 0
 * ws: DCA_GROUND_WS_LEN int64 per image of workspace, the caller's, cleared by the first launch of every call:
 *   [0] the Hough key   [8 + 10 k + j] sum j of round k   (the rounds that did nothing leave zeros)
 * Launches: v-disparity, vote, then (sums, solve) per round: 2 + 2 refine; refine = 0 takes 3, the solve kernel writing the
 * record of the Hough line alone.  Kernel boundaries are the only global synchronisation; nothing is allocated, nothing
 * waits, every scalar is passed by value.
 * Exactness: with rows, cols <= DCA_GROUND_MAX_DIM and NB <= DCA_GROUND_MAX_DISP every vote and every count is below 2^31
 * (at most rows cols), every line numerator below 2^27, every int64 sum below 2^59 (rows cols * 2^14 * 2^14); a sum below 2^53
 * converts to double exactly, a larger one is rounded once, to nearest, on the device and in the restatement alike.
 * Refused: NULL d / plane / vdisp / ws, B outside [1, 65535], a window outside the frame, Hc Wc >= 2^31, rows < 2, rows or
 * cols > DCA_GROUND_MAX_DIM, max_disp outside [8, DCA_GROUND_MAX_DISP], fit rows outside 0 <= r_lo < r_hi <= rows,
 * min_rise outside [1, NB], min_votes < 1, refine outside [0, DCA_GROUND_MAX_REFINE], min_inliers < 3, min_disp or tol negative
 * or not finite, a NaN mask_min with a mask, calibrated outside {0, 1}; with calibrated = 1: f or baseline not positive and
 * finite, cx, cy, doffs or v0 not finite.
 *
 * dca_ground_segment: labels, height above the road, free space per column and a bird's-eye occupancy grid from d, the
 * record `plane` of dca_ground_plane (read from device memory; it must have been computed with calibrated = 1 under this
 * calibration) and the fp32 calibration of dca_point_cloud (fb = float(f * baseline), rounded once by the host).
 * Per window pixel, with a32, b32, c32, hs32 the record's doubles rounded once to fp32:
 *   p = (a32 * float(u') + b32 * float(v')) + c32;   den = d + doffs;   pden = p + doffs;   h = (hs32 * (den - pden)) / den
 * h is the height above the road in metres, positive for a surface nearer than the road along the ray.  Labels (uint8),
 * the first rule that matches:
 *   0  no data        the pixel is not valid, or not den > 0, or the record's status is 1, or not hs32 > 0
 *   1  ground         fabsf(d - p) <= tol_d  ||  fabsf(h) <= h_ground
 *   4  below ground   h < 0
 *   3  overhang       h > h_max
 *   2  obstacle       everything else
 * Outputs, any may be NULL (free_row and free_disp together), not all:
 *   label (B,rows,cols) uint8;   height (B,rows,cols) fp32: h, +0.0 where the label is 0
 *   free_row (B,cols) int32, free_disp (B,cols) fp32: walking a column from the bottom row up, the first run of min_run
 *     consecutive pixels of label 2 (any other label starts the count again): free_row = the LOWEST row of that run (the
 *     obstacle's base), free_disp = d there bit for bit;  -1 and +0.0 without such a run
 *   bev (B,2,NZ,NX) int32: channel 0 counts the pixels of label 1, channel 1 those of label 2, per cell, with X and Z of
 *     dca_point_cloud (Z = fb / den;  X = ((float(c) - cx) * Z) / f):
 *       fx = floorf((X - x_min) * inv_cell);   fz = floorf(Z * inv_cell)     inv_cell: fp32, rounded once by the host
 *     a pixel counts iff 0 <= fx < NX, 0 <= fz < NZ (compared in float, then converted) and Z <= max_depth
 * TWO launches: (1) one lane per column walks it (the label is a function of the pixel and the record alone and is evaluated
 * again), and the same launch clears bev; (2) one thread per pixel writes label and height and adds to bev -- one integer
 * atomic per run of consecutive lanes of a wave that hit the same cell.  The kernel boundary orders the clearing before the adds.
 * Refused: NULL d / plane, no output, one of free_row / free_disp without the other, B outside [1, 65535], a window outside the
 * frame, rows or cols > DCA_GROUND_MAX_DIM, max_disp outside [8, DCA_GROUND_MAX_DISP], min_disp, tol_d, h_ground negative or not
 * finite, h_max not finite, min_run < 1, a NaN mask_min with a mask, f or fb not positive and finite, cx, doffs or x_min not
 * finite, with bev: inv_cell or max_depth not positive and finite, NX or NZ < 1, 2 NX NZ >= 2^31. */
#define DCA_GROUND_PLANE_LEN 16
#define DCA_GROUND_WS_LEN 48
#define DCA_GROUND_MAX_REFINE 4
#define DCA_GROUND_MAX_DISP 1024
#define DCA_GROUND_MAX_DIM 32768
int dca_ground_plane(const float* d, const float* mask, double* plane, int* vdisp, long long* ws, int B, int Hc, int Wc, int y0,
                     int rows, int cols, int max_disp, int r_lo, int r_hi, int min_rise, int min_votes, int refine,
                     int min_inliers, float min_disp, float tol, float mask_min, int calibrated, double f, double baseline,
                     double cx, double cy, double doffs, double v0, hipStream_t stream);
int dca_ground_segment(const float* d, const float* mask, const double* plane, unsigned char* label, float* height,
                       int* free_row, float* free_disp, int* bev, int B, int Hc, int Wc, int y0, int rows, int cols,
                       int max_disp, float min_disp, float mask_min, float tol_d, float h_ground, float h_max, int min_run,
                       float f, float fb, float cx, float doffs, float x_min, float inv_cell, float max_depth, int NX, int NZ,
                       hipStream_t stream);

/* ---- stixels: per-column ground / object / sky segments from disparity (stixel.hip, stixel_math.h);
 * inference only, no backward, no counterpart in the reference.  dcanet_amd/stixel.py holds the numpy restatement.
 * d, mask, the window (y0, rows, cols), NB = max_disp, min_disp, mask_min and the VALID test with its quantisation q (the
 * disparity in sixteenths) are those of dca_ground_plane; `plane` is its record (B, DCA_GROUND_PLANE_LEN), read from device
 * memory: a32, b32, c32 are [0], [1], [2] rounded once to fp32.  Everything below is integer arithmetic in units of 1/16 px
 * and (1/16 px)^2 but the one fp32 formula of g; there is no atomic of any kind: every output is bitwise defined.
 *
 * Cells.  CS = cols / width stixel columns (column s covers window columns [s width, (s + 1) width)) of H = rows / row_step cells
 * (integer divisions); cell k = 0 is the BOTTOM cell and covers window rows [rows - (k + 1) row_step, rows - k row_step).  The
 * cols % width columns on the right and the rows % row_step rows at the top are not covered.
 *   q[k] = the lower median -- rank (n - 1) / 2 of the n values in ascending order -- of the q of the cell's valid pixels;
 *          -1 when n < min_valid (min_valid >= 1)
 *   g[k] = floorf(((a32 * float(u') + b32 * float(v')) + c32) * 16.0f + 0.5f) clamped in float to [-16 NB, 16 NB] (a NaN: the
 *          lower end) at the cell's centre pixel: column s width + width / 2, row rows - (k + 1) row_step + row_step / 2,
 *          u' = column - cols / 2, v' = row - rows / 2 (integer divisions throughout)
 * Energy of a column.  A segmentation is a list of segments (kb, kt, c), kb <= kt, that covers the cells [0, H) bottom-up;
 * c = 0 ground, 1 object, 2 sky.  With n, S1, S2 the count, the sum and the sum of squares of the valid q of a segment
 * (a cell with q = -1 costs nothing in any class) and cp the class of the segment below, its cost is data + seg[c] + prior:
 *   data   ground: sum min((q - g)^2, Tg);   sky: sum min(q^2, Ts);
 *          object: S2 - 2 mu S1 + n mu^2 with mu = (2 S1 + n) / (2 n) (integer division: the mean rounded to a sixteenth);
 *          n = 0: data 0 and mu = -1
 *   prior  the bottom segment: first[c];  any other: T[cp][c], where a NEGATIVE entry forbids the pair
 *          + far    for an object with 0 <= mu < mu_min (a bottom segment included)
 *          + below  for an object directly on a ground segment with mu > g[kb] + eps   (its foot would lie under the road)
 *          + hang   for an object directly on a ground segment with mu < g[kb] - eps   (it hangs in the air behind the road);
 *                   both compare mu as it is, -1 for n = 0
 * Recursion.  cost[kt][c] = min over kb <= kt and cp of cost[kb - 1][cp] + prior + data + seg[c] (kb = 0: no cp, nothing below).
 * Ties go to the smallest kb, then the smallest cp: the unsigned minimum of  cost << 12 | kb << 2 | cp  with cp = 3 for kb = 0.
 * The class of the top segment has the smallest cost[H - 1][c], then the smallest c; the back-pointers give the rest.  The prior
 * depends on the segment's own values and the class below only, so the minimum is exact.  A single segment of any class is
 * never forbidden: a segmentation always exists.
 * Bound: with q < 2^14, H <= DCA_STIXEL_MAX_CELLS = 1024 and every constant <= DCA_STIXEL_MAX_CONST = 2^20 the object term is
 * below 2^38, a column's ground or sky terms below 2^30 and all seg + prior below 2^33: every total stays below 2^39 < 2^50.
 * A record of status 1, or without a calibration (not float([9]) > 0): no segmentation -- count 0, energy 0, the list zero,
 * seg_class DCA_STIXEL_NO_CLASS, seg_disp +0.0; cells is written as defined.
 * Outputs, any may be NULL, not all; only those given are written, every word of them on every call:
 *   cells (B,H,CS,2) int16: q, g;   seg_class (B,H,CS) uint8: the class of every cell;
 *   seg_disp (B,H,CS) fp32: float(mu) / 16.0f in the cells of an object with n > 0, +0.0 elsewhere
 *   count (B,CS) int32: the number of segments, also when it exceeds max_segments;   energy (B,CS) int64: the minimum
 *   stixels (B,CS,max_segments,4) int32, bottom-up, the lowest max_segments segments: the segment's first (upper) window row
 *     rows - (kt + 1) row_step, its last (lower) window row rows - kb row_step - 1, c, and mu of an object (-1 for ground, sky
 *     and n = 0); the entries from `count` on are zero
 * ws: (B,H,CS,2) int16 of workspace, the caller's, where (q, g) pass from the first launch to the second; needed only when
 * cells is NULL; never read before it is written.
 * TWO launches (one when only cells is given): (1) one thread per cell; (2) one wave per stixel column: prefix sums in LDS,
 * H dependent steps, the walk back in the same launch.  56 (H + 1) + 6 H bytes of LDS, 63.5 KB at H = 1024.  Nothing is
 * allocated, nothing waits.
 * Refused: NULL d / plane, no output, cells and ws both NULL, B outside [1, 65535], a window outside the frame, Hc Wc >= 2^31,
 * rows or cols > DCA_GROUND_MAX_DIM, max_disp outside [8, DCA_GROUND_MAX_DISP], min_disp negative or not finite, a NaN mask_min
 * with a mask, width outside [1, DCA_STIXEL_MAX_WIDTH], row_step outside [1, DCA_STIXEL_MAX_ROW_STEP], H outside
 * [2, DCA_STIXEL_MAX_CELLS], CS < 1, min_valid outside [1, width row_step], max_segments outside [1, DCA_STIXEL_MAX_SEGMENTS],
 * a constant outside [0, DCA_STIXEL_MAX_CONST], an entry of T outside [-1, DCA_STIXEL_MAX_CONST]. */
#define DCA_STIXEL_MAX_WIDTH 16
#define DCA_STIXEL_MAX_ROW_STEP 8
#define DCA_STIXEL_MAX_CELLS 1024
#define DCA_STIXEL_MAX_SEGMENTS 64
#define DCA_STIXEL_MAX_CONST 1048576
#define DCA_STIXEL_NO_CLASS 255
int dca_stixels(const float* d, const float* mask, const double* plane, short* ws, short* cells, unsigned char* seg_class,
                float* seg_disp, int* count, int* stixels, long long* energy, int B, int Hc, int Wc, int y0, int rows, int cols,
                int max_disp, int width, int row_step, int min_valid, int max_segments, float min_disp, float mask_min, int Tg,
                int Ts, int eps, int below, int hang, int mu_min, int far, int seg0, int seg1, int seg2, int first0, int first1,
                int first2, int t00, int t01, int t02, int t10, int t11, int t12, int t20, int t21, int t22, hipStream_t stream);

/* ---- temporal stereo (temporal.hip, temporal_math.h); inference only, no counterpart in the reference ---
 * The STATE of a sequence is three dense (H,W) maps in image coordinates: disp fp32 (+0.0: nothing), var fp32 (px^2), age uint8
 * (frames since the pixel's filter started).
 *
 * dca_disp_reproject: the previous state warped by the known ego-motion into the current left image.  g00 .. g23: the 3x4
 * matrix G of temporal.reproject_matrix,  G = (1/f) [ K R A | K t / baseline ]  with K = [[f,0,cx],[0,f,cy],[0,0,1]],
 * A = [[1,0,-cx],[0,1,-cy],[0,0,f]] and (R | t) the pose of the previous rectified left camera in the current one; formed in
 * fp64 and rounded once by the host; exactly [I | 0] for the identity pose.  mask (H,W) fp32 or NULL: a source pixel takes
 * part where mask >= mask_min.  In fp32, every operation rounded on its own (no fused multiply-adds), IEEE division, per
 * SOURCE pixel (u = column, v = row) with disparity d:
 *   den = d + doffs
 *   x = ((g00 u + g01 v) + g02) + g03 den        (y and z likewise from rows 1 and 2;  z is Z_cur / Z_prev)
 *   u' = x / z;  v' = y / z;  uf = floorf(u' + 0.5f);  vf = floorf(v' + 0.5f)
 *   den' = den / z;  d' = den' - doffs
 *   keep = d finite && d >= min_disp && mask && z >= min_ratio && 0 <= uf < W && 0 <= vf < H && d' >= min_disp && d' < max_disp
 * All comparisons are made in float before anything is converted to int: a NaN fails them, an infinity or 1e30 fails them
 * without overflowing an int (a point behind the camera has z <= 0 and fails z >= min_ratio, or, with min_ratio = 0 and
 * z = 0, the range of d').  A kept pixel proposes the key  bits(den') << 32 | (0xFFFFFFFF - source index)  to the target
 * word vf W + uf of the workspace, cleared to 0, with an agent-scope, relaxed 64-bit INTEGER fetch_max.  min_disp >= 0 and
 * doffs >= 0 make den' >= 0, whose bits order as the floats do: the nearest surface wins, among equal den' the smallest
 * source index, and the result does not depend on the order of arrival.
 * Per target (r, c) with a non-zero key: denmax = the maximum of the winners' den' over rows r-ry .. r+ry and columns
 * c-rx .. c+rx clipped to the image (the pixel itself included; an empty target counts as 0);
 *   visible = den' + occl_px >= denmax       an ABSOLUTE threshold in pixels; rx = ry = 0 switches the test off
 * It removes background seen through the cracks that forward splatting opens in a magnified foreground.  The payload is
 * gathered from the winning source pixel src:  pred = d';  pred_var = var[src] / (z z) + q  with z recomputed from src by the
 * expression above;  pred_age = min(age[src] + 1, 255);  hints = pred where pred_age >= hint_min_age, else +0.0.
 * Outputs, (H,W) each, +0.0 / 0 where nothing is visible; any may be NULL, not all five:
 *   pred fp32, pred_var fp32, pred_age uint8, hints fp32 (the hint map of dca_hints_to_quarter)
 *   count  2 words: count[0] = visible targets, count[1] = kept sources; integer atomics, one per workgroup
 * No output may overlap an input.  workspace: H W 64-bit words, 8-byte aligned, the caller's; after the call it holds the keys.
 * THREE launches on the stream: clear the workspace and the counters; scatter; resolve (a workgroup stages a tile of the
 * keys' high words with the halo in LDS and takes the window maximum along rows, then along columns; eight workgroups per CU
 * walk the tiles).  No floating-point atomic.  Everything is passed BY VALUE, the twelve matrix entries too: a launch
 * captured into a hipGraph keeps the pose it was captured with, so the operator is launched eagerly, next to the graph.
 * Refused: NULL disp / var / age, non-positive H or W, H W >= 2^31, a matrix entry that is not finite, rx or ry outside
 * [0, DCA_TEMPORAL_MAX_RADIUS], occl_px, q or min_ratio negative or not finite, doffs or min_disp negative or not finite,
 * max_disp not finite or < min_disp, hint_min_age outside [0, 255], a NaN mask_min with a mask, NULL workspace, five NULL
 * outputs.
 *
 * dca_temporal_fuse: prediction and measurement into a new state, ONE launch, per pixel.  pred, pred_var, pred_age: (rows,cols)
 * dense, the outputs of dca_disp_reproject; pred NULL: no prediction anywhere (the first frame of a sequence).  meas: a frame
 * map (Hc,Wc) read through the window rows x cols at frame row y0, column 0, as in dca_disp_export -- never copied; mask
 * (Hc,Wc) fp32 or NULL and meas_var_map (Hc,Wc) fp32 or NULL are indexed like meas; with meas_var_map NULL the measurement's
 * variance is the scalar meas_var.  With m the measurement and vm its variance:
 *   m_ok = m finite && m >= min_disp && mask >= mask_min && 0 < vm < inf
 *   p_ok = pred > 0 && 0 <= pred_var <= var_max
 *   neither                 disp = +0.0   var = +0.0       age = 0
 *   only m_ok               disp = m      var = vm         age = 0
 *   only p_ok (coast)       disp = pred   var = pred_var   age = pred_age
 *   both:  e = m - pred;  s = pred_var + vm
 *     e e <= gate2 s        k = pred_var / s;  disp = pred + k e;  var = pred_var - k pred_var;  age = pred_age
 *     otherwise             disp = m      var = vm         age = 0      (a new surface: the filter starts again)
 * in fp32, every operation rounded on its own.  gate2 = +inf switches the gate off, var_max = +inf the variance limit.
 * Outputs (rows,cols), any may be NULL, not all: disp, var fp32, age uint8, and innov fp32 = |e| where both are valid, else +0.0
 * (a moving-object / mismatch cue).  disp / var / age may be the very buffers pred / pred_var / pred_age, or the buffers
 * dca_disp_reproject read (that launch has finished): a thread reads its pixel before it writes it.
 * Refused: NULL meas, no output, pred without pred_var and pred_age, a window outside the frame, without meas_var_map a
 * meas_var that is not positive and finite, min_disp negative or not finite, gate2 or var_max negative or NaN, a NaN
 * mask_min with a mask. */
#define DCA_TEMPORAL_MAX_RADIUS 8
int dca_disp_reproject(const float* disp, const float* var, const unsigned char* age, const float* mask, float mask_min,
                       float g00, float g01, float g02, float g03, float g10, float g11, float g12, float g13, float g20,
                       float g21, float g22, float g23, int H, int W, float doffs, float min_disp, float max_disp,
                       float min_ratio, int rx, int ry, float occl_px, float q, int hint_min_age, float* pred, float* pred_var,
                       unsigned char* pred_age, float* hints, long long* count, long long* workspace, hipStream_t stream);
int dca_temporal_fuse(const float* pred, const float* pred_var, const unsigned char* pred_age, const float* meas,
                      const float* mask, const float* meas_var_map, float meas_var, float* disp, float* var, unsigned char* age,
                      float* innov, int Hc, int Wc, int y0, int rows, int cols, float min_disp, float mask_min, float gate2,
                      float var_max, hipStream_t stream);
/* dca_disp_reproject_dev: dca_disp_reproject with the twelve floats of G read from DEVICE memory (g: 12 fp32, row-major 3x4,
 * 4-byte aligned), so that a pose estimated on the device (dca_ego_motion) is never read back in the middle of a frame.  The same
 * kernels, the same arithmetic, the same other arguments and refusals.  (Capture into a hipGraph is untested.)  The launcher
 * CANNOT validate a matrix it does not see.  With a NaN in it every float comparison of the keep test fails: no source is
 * kept, the prediction is empty (+0.0 / 0 everywhere), count = (0, 0), and dca_temporal_fuse then starts every pixel again
 * from the measurement -- a failed estimate (dca_ego_motion writes G as NaN) resets the sequence on the device.  Refused
 * besides: NULL or misaligned g. */
int dca_disp_reproject_dev(const float* disp, const float* var, const unsigned char* age, const float* mask, float mask_min,
                           const float* g, int H, int W, float doffs, float min_disp, float max_disp, float min_ratio, int rx,
                           int ry, float occl_px, float q, int hint_min_age, float* pred, float* pred_var,
                           unsigned char* pred_age, float* hints, long long* count, long long* workspace, hipStream_t stream);

/* ---- semi-global matching on a census cost (sgm.hip, sgm_math.h; Hirschmueller 2008, Zabih & Woodfill
 * 1994): a disparity source that needs no weights.  Inference only, no counterpart in the reference.  dcanet_amd/sgm.py holds
 * the numpy restatement.  Integer arithmetic from the first byte to the last: no tolerance, no atomic of any kind, every output
 * bitwise defined and independent of the order of execution.
 *
 * Inputs.  One rectified pair of uint8 images, (H,W) grey (C = 1) or interleaved (H,W,C) with C = 3 or 4 (a fourth channel is
 * ignored).  Colour is reduced to grey by  g = (77 R + 150 G + 29 B + 128) >> 8.
 * Limits: DCA_SGM_MIN_DIM = 7 <= H, W <= DCA_SGM_MAX_DIM = 8192, D = max_disp an integer in [DCA_SGM_MIN_DISP, DCA_SGM_MAX_DISP]
 * = [8, 256], H W D < 2^30.  D need not be a multiple of anything.
 *
 * Census.  The window is 9 wide and 7 high.  Each pixel gets DCA_SGM_CENSUS_BITS = 62 bits in a uint64: the neighbours are
 * visited row-major, dy = -3..3 outer, dx = -4..4 inner, the centre skipped; the first neighbour is bit 61, the last bit 0.  A
 * bit is 1 iff the neighbour lies inside the image and g(neighbour) < g(centre).
 *
 * Matching cost.  C(y,x,d) = popcount(cL(y,x) ^ cR(y,x-d)) for x - d >= 0, and DCA_SGM_COST_OUT = 62 otherwise.
 *
 * Paths.  paths = 4: the predecessor offsets r = (dy,dx) in {(0,+1), (0,-1), (+1,0), (-1,0)};  paths = 8 adds (+1,+1), (+1,-1),
 * (-1,+1), (-1,-1).  If p - r lies outside the image, L_r(p,d) = C(p,d): there is no wrap-around.  Otherwise, with
 * m = min_k L_r(p-r,k):
 *   L_r(p,d) = C(p,d) + min( L_r(p-r,d), L_r(p-r,d-1) + P1 [d >= 1], L_r(p-r,d+1) + P1 [d <= D-2], m + P2 ) - m
 * S = the sum over r of L_r.  1 <= P1 <= P2 <= DCA_SGM_MAX_P = 4095.  Then C <= L_r <= 62 + P2 and S <= 8 * 4157 = 33256: every
 * L_r and S fits uint16 and nothing saturates anywhere.
 *
 * Left disparity.  d* = the lowest index of min_d S(p,d), s = S(p,d*).  Uniqueness u, an integer in 0..99: the pixel passes iff
 * every k with |k - d*| > 1 has  S(p,k) * (100 - u) >= 100 * s  (u = 0 switches the test off).  Sub-pixel step in sixteenths: if
 * 0 < d* < D-1 and den = S(d*-1) + S(d*+1) - 2 s > 0 then
 *   off = (16 * (S(d*-1) - S(d*+1)) + 17 * den) / (2 * den) - 8
 * (the numerator is at least den > 0, so the division is one of positive integers; off lies in [-8, 8] and is 8 (S(d*-1) -
 * S(d*+1)) / den rounded half up), otherwise off = 0;  q = 16 d* + off.  valid = passes && d* >= min_disp, min_disp an integer
 * in 0..D-1.   disp = float(q) / 16.0f where valid, +0.0 elsewhere (one exact fp32 division);  cost = s, for every pixel.
 *
 * Right-view disparity, from the same S.  The bins present at right-image pixel (y,x) are k < min(D, W - x) with
 * S_R(y,x,k) = S(y,x+k,k): the lowest argmin, then the same sub-pixel rule when both neighbours are present.  No uniqueness
 * test; every pixel is written.  disp_right is in the right image's own coordinates, disp_right_mirrored holds column i at index
 * W-1-i (the second argument of dca_lr_consistency).
 *
 * dca_sgm_workspace_bytes(H, W, max_disp): the bytes of `workspace`, 16 H W for the census of both images (2,H,W) uint64
 * followed by 2 H W D for S (H,W,D) uint16, d innermost; -1 for sizes outside the limits.  The workspace is the caller's,
 * 8-byte aligned, and may hold garbage: nothing is read before it is written.
 * dca_sgm_census: grey conversion and census of both images in ONE launch (a tile with its 4 x 3 halo in LDS) into
 * census (2,H,W) uint64, left first.
 * dca_sgm_disparity: the census launch, then ONE launch per path -- one wave per scanline (a row for the horizontal paths; a
 * start column for the others, the column moving by dx per row and starting a new path where it re-enters on the other side),
 * each lane holding ceil(D / 64) consecutive bins, the cost formed from the census words as the scan goes and never stored; the
 * first path writes S, the others add to it -- then the winner-take-all launch of the left view and, only when disp_right or
 * disp_right_mirrored is given, that of the right view.  Outputs (H,W), any may be NULL, not all: disp fp32, valid fp32
 * 1.0 / 0.0, cost int32, disp_right fp32, disp_right_mirrored fp32; only those given are written, every word of them.  All
 * launches go on `stream`; nothing is allocated, nothing waits.
 * Refused: NULL images, census or workspace, a workspace or a census that is not 8-byte aligned, C not 1, 3 or 4, H, W or
 * max_disp outside the limits, H W D >= 2^30, paths not 4 or 8, P1 < 1, P1 > P2, P2 > DCA_SGM_MAX_P, uniqueness outside
 * [0, 99], min_disp outside [0, D-1], no output. */
#define DCA_SGM_MIN_DIM 7
#define DCA_SGM_MAX_DIM 8192
#define DCA_SGM_MIN_DISP 8
#define DCA_SGM_MAX_DISP 256
#define DCA_SGM_MAX_P 4095
#define DCA_SGM_CENSUS_BITS 62
#define DCA_SGM_COST_OUT 62
long dca_sgm_workspace_bytes(int H, int W, int max_disp);
int dca_sgm_census(const unsigned char* left, const unsigned char* right, unsigned long long* census, int H, int W, int C,
                   hipStream_t stream);
int dca_sgm_disparity(const unsigned char* left, const unsigned char* right, void* workspace, float* disp, float* valid,
                      int* cost, float* disp_right, float* disp_right_mirrored, int H, int W, int C, int max_disp, int paths,
                      int P1, int P2, int uniqueness, int min_disp, hipStream_t stream);

/* ---- stereo visual odometry (odometry.hip, odometry_math.h; Comport et al. 2007, Steinbruecker et al.
 * 2011, Kerl et al. 2013): the motion of the left camera between two frames, the pose dca_disp_reproject needs, from the
 * previous frame's disparity and the grey images of both.  Inference only, no counterpart in the reference.  dcanet_amd/odometry.py
 * holds the numpy restatement; every output is bitwise defined and independent of the order of execution.
 *
 * Pyramids.  Level l of an H x W map is (H >> l) x (W >> l) (odd sizes drop the last row or column); a pyramid of `levels`
 * levels is ONE dense buffer of dca_pyramid_len(H, W, levels) elements, level 0 first (-1 for levels outside
 * [1, DCA_ODO_MAX_LEVELS], a coarsest level without a pixel or H W >= 2^31).
 * dca_grey_pyramid: rgb (H,W,C) uint8 interleaved, C = 3 or 4 -> uint8; level 0 is (R + 2 G + B + 2) >> 2, each further level
 * the 2x2 area mean (a + b + c + d + 2) >> 2 of the level above.  One launch per level.
 * dca_disp_pyramid: disp (H,W) fp32 -> fp32; level 0 is a copy, each further level the LARGEST valid value of the 2x2 block
 * (finite and >= min_disp at that level: the nearest surface), times 0.5f, plus 0.0f (so a -0.0, valid at min_disp = 0,
 * leaves as +0.0 whichever zero the maximum kept); +0.0 where none is valid.  One launch per level.
 * Refused: NULL pointers, C not 3 or 4, levels as above, H W >= 2^29, min_disp negative or not finite, out == disp.
 *
 * dca_ego_motion.  prev, cur: the grey pyramids of the previous and the current left image; disp: the disparity pyramid of
 * the previous frame; f, baseline, cx, cy, doffs: the calibration.  The camera of level l, in fp64 and then rounded to fp32:
 * f_l = f / 2^l, cx_l = (cx + 0.5) / 2^l - 0.5 (cy likewise), doffs_l = doffs / 2^l; max_disp_l = max_disp / 2^l; min_disp,
 * min_ratio, grad_min and the Huber radius are the same at every level.  The estimate is T = (R | tau), the pose of the
 * previous camera in the current one with the translation in BASELINES, held in fp64 in the record.  Levels run coarse to
 * fine, `iters` Gauss-Newton iterations each; the count is fixed and nothing is read back.  One iteration is two launches.
 *
 * Sums.  Per source pixel (u, v), 1 <= u <= W_l - 2, 1 <= v <= H_l - 2, of the previous level image Ip, with d its disparity and
 * G_l = (1/f_l) [ K_l R A_l | K_l tau ] (fp64 in the written order of temporal.reproject_matrix, rounded to fp32 once; exactly
 * [I | 0] for the identity), in fp32 with every operation rounded on its own and IEEE division:
 *   valid:    d finite && min_disp <= d < max_disp_l;  den = d + doffs_l
 *             gx = Ip(u+1,v) - Ip(u-1,v);  gy = Ip(u,v+1) - Ip(u,v-1);  |gx| + |gy| >= grad_min
 *   warp:     x = ((g00 u + g01 v) + g02) + g03 den  (y, z likewise);  z >= min_ratio
 *   position: px = floorf((x / z) 16 + 0.5f);  py likewise;  0 <= px < 16 (W_l - 1) and 0 <= py < 16 (H_l - 1), compared in
 *             float: the whole bilinear footprint x0 .. x0 + 1, y0 .. y0 + 1 lies in the current image, x0 = px >> 4, fx = px & 15
 *   residual: r = (16-fy) ((16-fx) I00 + fx I01) + fy ((16-fx) I10 + fx I11) - (Ip(u,v) << 8)     an exact integer, 1/256 grey level
 *   Jacobian: a = u - cx_l;  b = v - cy_l;  af = a / f_l;  bf = b / f_l
 *             J0 = gx den;  J1 = gy den;  J2 = gx (-(af den)) + gy (-(bf den));  J3 = gx (-(af b)) + gy (-(f_l + bf b))
 *             J4 = gx (f_l + af a) + gy (af b);  J5 = gx (-b) + gy a          (inverse-compositional: the gradient of Ip)
 *   quantise: q_i = (int)rintf(J_i 2^e_i);  e_i = 17 - k_i with 510 B_i = m 2^k_i, m in [0.5, 1), in fp64, where B_i bounds
 *             |Ju_i|, |Jv_i| over the level:  A = max(|cx_l|, |W_l - 1 - cx_l|), Bv likewise, Dn = max_disp_l + doffs_l,
 *             B = (Dn, Dn, max(A, Bv) Dn / f_l, max(A Bv / f_l, f_l + Bv Bv / f_l), max(f_l + A A / f_l, A Bv / f_l), max(A, Bv))
 *   weight:   k = rint(huber 256);  w = 64 if |r| <= k else (64 k) / |r|, an integer division
 * and DCA_ODO_SUMS = 29 int64 sums over the pixels that pass: the 21 upper entries w q_i q_j (i <= j, row-major), the six
 * w q_i r, w r r and the count.  |q_i| < 2^18, |r| < 2^16, w <= 2^6: every term is below 2^42 and H W <= 2^20 pixels cannot
 * overflow a sum.  Per-lane registers, a cross-lane reduction, LDS across the waves, then ONE agent-scope relaxed INTEGER
 * atomicAdd per (workgroup, sum); at most one workgroup per CU walks the pixels.  No floating-point atomic.
 *
 * Solve, one thread, fp64, only + - * / in ONE written order (odometry_math.h): A_ij = S_ij 2^(-e_i - e_j) with the diagonal
 * times 1 + 2^-10, c_i = S_ir 2^(-e_i - 7) (r's 2^-8 and the 2 of the central difference); LDL^T and two substitutions give
 * xi = (tau', omega); R' = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a) with a = omega / 2 (Cayley: no sin / cos, whose last
 * bits differ between libraries);  R <- R R'^T, tau <- tau - R tau'  (T <- T [R' | tau']^-1).  It writes the record, G of
 * level 0 and G_l of the next iteration's level, and clears the sums.  With count < min_pixels or a pivot that is not
 * positive it sets status = 1 (failed) and writes both G as NaN; every later launch of the call returns at once.
 *
 * rec: DCA_ODO_REC_LEN = 24 doubles: [0..11] T_cur_from_prev (3,4) row-major with the translation in METRES (tau baseline),
 * [12..14] tau, [15] the count and [16] the mean of w r^2 (w in (0,1], grey levels squared) of the last iteration that ran,
 * [17] status 0 / 1, [18] iterations run, the rest 0.  On failure T keeps the last estimate.
 * g: 24 fp32: G (3,4) of level 0 -- the argument of dca_disp_reproject_dev -- then G_l of the next iteration (scratch).
 * sums: 29 int64 of scratch.  sums_out, or NULL: (levels iters, 29) int64, the sums of every iteration in the order they
 * ran (a debug output; 0 for iterations after a failure).  All of them may hold garbage: the init launch writes them.
 * Start: init_rec, a DEVICE record of an earlier call (R and tau are taken from it; the identity if its status is failed; it may
 * be rec itself), or with init_rec NULL the host pose t00 .. t23 (3,4), translation in metres (the identity: 1 0 0 0 0 1 ...).
 * 1 + 2 levels iters launches on the stream; nothing is allocated, nothing waits.
 * Refused: NULL prev / cur / disp / rec / g / sums, levels as above, H W > 2^20, iters outside [1, DCA_ODO_MAX_ITERS], a
 * calibration that is not finite or f, baseline <= 0 or doffs < 0, min_disp negative, max_disp <= min_disp, min_ratio <= 0
 * (or any of them not finite), grad_min outside [0, 510], rint(huber 256) outside [1, 65280], min_pixels < 6, a host pose
 * that is not finite, misaligned rec / g / sums / sums_out.
 *
 * dca_pose_chain: the world pose of a sequence kept on the device, one launch, one thread.  world: 12 doubles, the (3,4) pose of
 * the current camera in the world (camera coordinates -> world coordinates, as KITTI's poses are).  rec NULL: a sequence
 * starts, world = the identity.  Otherwise, if the record's status is 0, world <- world T^-1 with T = T_cur_from_prev of the
 * record and T^-1 = (R^T | -R^T t), in ONE written order in fp64 (om_chain); a failed record leaves world as it is.
 * out: DCA_ODO_FRAME_LEN = 35 doubles: [0..15] the world pose (4,4), [16..31] the motion T (4,4; the identity when a sequence
 * starts or the estimate failed), [32] count, [33] residual, [34] status.  Refused: NULL world or out, misaligned pointers. */
#define DCA_ODO_MAX_LEVELS 8
#define DCA_ODO_MAX_ITERS 64
#define DCA_ODO_SUMS 29
#define DCA_ODO_REC_LEN 24
#define DCA_ODO_FRAME_LEN 35
long dca_pyramid_len(int H, int W, int levels);
int dca_grey_pyramid(const unsigned char* rgb, int H, int W, int C, int levels, unsigned char* out, hipStream_t stream);
int dca_disp_pyramid(const float* disp, int H, int W, int levels, float min_disp, float* out, hipStream_t stream);
int dca_ego_motion(const unsigned char* prev, const unsigned char* cur, const float* disp, int H, int W, int levels, int iters,
                   double f, double baseline, double cx, double cy, double doffs, float min_disp, float max_disp,
                   float min_ratio, int grad_min, float huber, int min_pixels, const double* init_rec, double t00, double t01,
                   double t02, double t03, double t10, double t11, double t12, double t13, double t20, double t21, double t22,
                   double t23, double* rec, float* g, long long* sums, long long* sums_out, hipStream_t stream);

int dca_pose_chain(const double* rec, double* world, double* out, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DCA_HIP_H */
