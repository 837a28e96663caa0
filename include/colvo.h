/* colvo.h -- C-ABI of the MI355X-native ColVO DCDP+LCC training hot path (libcolvo.so).
 *
 * The upstream reference (HNUicda/CoIVO, /root/reference) defines NO plugin, operator or FFI
 * interface -- it ships README.md and three figures only.  Each entry point
 * below therefore cites the README sentence that names the concept it implements and the function
 * of the frozen specification (oracle/colvo_spec.py) whose results it must reproduce; there is no
 * reference file:line to replace.
 *
 * Conventions
 *   - plain C types only: device pointers + sizes; `stream` is a hipStream_t passed as void*.
 *   - the caller owns every buffer (inputs, outputs, workspace); the library never allocates,
 *     frees or keeps a pointer after return.
 *   - every call only ENQUEUES work on `stream` and returns; no internal synchronisation, no
 *     global mutable state (colvo_run_commands keeps a ring of fork/join events) -> safe under one-process-per-GPU data parallel and under hipGraph
 *     capture.
 *   - return 0 on success, a non-zero hipError_t-style code otherwise; the message is available
 *     from colvo_last_error() (thread-local).  Nothing throws across the ABI.
 *   - images / depth at the boundary: NCHW, contiguous, fp32.  Feature maps inside the conv stack:
 *     NHWC, fp32 (COLVO_F32) or bf16 (COLVO_BF16).
 */
#ifndef COLVO_H_
#define COLVO_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COLVO_ABI_VERSION 29

typedef void* colvo_stream_t; /* hipStream_t */

enum { COLVO_F32 = 0, COLVO_BF16 = 1 };

int colvo_abi_version(void);
const char* colvo_last_error(void);

/* ------------------------------------------------------------------------------------------- *
 * a3..a7  fused  project -> bilinear-sample -> LCC-recalibrate -> SSIM/L1       *
 *   concept: README.md:1 "Photometric Consistency", README.md:7 "alignment of geometric       *
 *   projections between consecutive frames", README.md:5,7 LCC "recalibrating the luminosity  *
 *   values of adjacent frames".   spec: oracle/colvo_spec.py photometric_loss().               *
 * ------------------------------------------------------------------------------------------- */

/* Number of floats of scratch the fwd / bwd calls need for a [B,3,H,W] problem. */
size_t colvo_warp_loss_workspace_floats(int B, int H, int W);

/* Forward.  tgt, ref [B,3,H,W]; depth [B,1,H,W]; pose [B,6]; K [B,3,3]; lcc_a, lcc_b [B].
 * loss_state[4] (device) receives { loss, 1/max(3*n_valid,1), n_valid, masked sum = loss * max(3*n_valid,1) }.  H, W >= 2. */
int colvo_warp_loss_fwd(const float* tgt, const float* ref, const float* depth, const float* pose,
                        const float* K, const float* lcc_a, const float* lcc_b,
                        int B, int H, int W, float ssim_weight,
                        float* workspace, float* loss_state, colvo_stream_t stream);

/* Backward (recomputes the warp; nothing but loss_state is saved by the forward).
 * grad_loss: device scalar dL/dloss.  Outputs: d_depth [B,1,H,W], d_pose [B,6], d_a [B], d_b [B]. */
int colvo_warp_loss_bwd(const float* tgt, const float* ref, const float* depth, const float* pose,
                        const float* K, const float* lcc_a, const float* lcc_b,
                        int B, int H, int W, float ssim_weight,
                        const float* loss_state, const float* grad_loss,
                        float* workspace, float* d_depth, float* d_pose, float* d_a, float* d_b,
                        colvo_stream_t stream);

/* Training path: the loss and its UNNORMALISED gradients in one pass (the backward kernel evaluates everything the
 * forward does).  loss_state as in colvo_warp_loss_fwd; d_depth_raw [B,1,H,W] and grad_partials [B*14] are handed to
 * colvo_warp_loss_fused_bwd, which applies dL/dloss / max(3 n_valid, 1) and writes the four gradients.
 * grad_unit (8*B floats, may be NULL) receives the unnormalised pose / LCC gradients in PoseNet's planar output layout
 * [d_pose B x 6 | d_a B | d_b B] for a consumer that applies the two scale factors itself (colvo_pose_head_bwd). */
int colvo_warp_loss_fused(const float* tgt, const float* ref, const float* depth, const float* pose,
                          const float* K, const float* lcc_a, const float* lcc_b,
                          int B, int H, int W, float ssim_weight,
                          float* workspace, float* loss_state, float* d_depth_raw, float* grad_partials,
                          float* grad_unit, colvo_stream_t stream);
int colvo_warp_loss_fused_bwd(const float* loss_state, const float* grad_loss, const float* d_depth_raw,
                              const float* grad_partials, const float* pose, int B, int H, int W,
                              float* d_depth, float* d_pose, float* d_a, float* d_b, colvo_stream_t stream);
/* The same without the pass over d_depth: only d_pose [B,6], d_a [B], d_b [B].  For callers that hand d_depth_raw and
 * the two scale factors (grad_loss[0], loss_state[1]) to the consumer of the depth gradient instead
 * (colvo_depth_head_bwd_parts): the normalisation is then applied where d_depth is read anyway. */
int colvo_warp_loss_fused_bwd_params(const float* loss_state, const float* grad_loss, const float* grad_partials,
                                     const float* pose, int B, float* d_pose, float* d_a, float* d_b,
                                     colvo_stream_t stream);

/* Data parallel with the spec's batch normalisation (oracle/SPEC.md section 5: ONE masked mean over the whole batch).  The caller
 * adds loss_state[2..3] (valid pixels, masked sum) up over its `world` ranks -- one all-reduce of two floats -- and this call turns
 * the state into the global one: loss_state[0] = the loss of the whole batch, loss_state[1] = world / max(3 n_global, 1), so that
 * (1 / world) x the sum of the ranks' gradients is the gradient of that loss.  Every backward entry point above reads the scale
 * from loss_state[1].  world = 1 leaves the state bit for bit as the forward wrote it. */
int colvo_warp_loss_rescale(float* loss_state, int world, colvo_stream_t stream);
/* The same, for a caller that takes the exchange OFF the critical path (round 6): the backward pass has already run on the
 * UNNORMALISED gradients (its consumers were handed a scale of 1 in place of loss_state[1]) while the two floats were being
 * all-reduced; every parameter gradient is linear in the scale, so it is applied once, behind the gradient all-reduce, by the
 * optimizer: *scale_out = world / max(3 n_global, 1) is what colvo_adam_pack_step_scaled multiplies into its grad_scale.
 * loss_state[0] / [1] are rewritten as by colvo_warp_loss_rescale (the reported loss becomes the whole batch's). */
int colvo_warp_loss_rescale_to(float* loss_state, int world, float* scale_out, colvo_stream_t stream);

/* ------------------------------------------------------------------------------------------- *
 * SURVEY.md §8f-1  geometric consistency (README.md:1 "Considering Geometric and Photometric   *
 *   Consistency", :7 "alignment of geometric projections").  spec: geometric_consistency_loss. *
 * ------------------------------------------------------------------------------------------- */
/* depth_t, depth_r [B,1,H,W]; pose [B,6]; K [B,3,3].  loss_state[4] = { loss, 1/max(n_valid,1), n_valid, 0 }.
 * workspace: colvo_geo_loss_workspace_floats(B,H,W) floats.  Backward recomputes the forward; d_depth_r is zeroed by the
 * call and accumulated with float atomics (the four taps of every sample). */
size_t colvo_geo_loss_workspace_floats(int B, int H, int W);
int colvo_geo_loss_fwd(const float* depth_t, const float* depth_r, const float* pose, const float* K,
                       int B, int H, int W, float* workspace, float* loss_state, colvo_stream_t stream);
int colvo_geo_loss_bwd(const float* depth_t, const float* depth_r, const float* pose, const float* K,
                       int B, int H, int W, const float* loss_state, const float* grad_loss, float* workspace,
                       float* d_depth_t, float* d_depth_r, float* d_pose, colvo_stream_t stream);

/* ------------------------------------------------------------------------------------------- *
 * SURVEY.md §8f-2  edge-aware smoothness of the inverse depth (spec: smoothness_loss) and the  *
 *   2x2 average pooling of the multi-scale photometric term (spec: downsample2).               *
 * ------------------------------------------------------------------------------------------- */
/* depth [B,1,H,W], img [B,3,H,W]; workspace: 2 * B * ceil(H*W/256) floats; loss: one device float. */
int colvo_smooth_loss_fwd(const float* depth, const float* img, int B, int H, int W, float* workspace, float* loss,
                          colvo_stream_t stream);
int colvo_smooth_loss_bwd(const float* depth, const float* img, int B, int H, int W, const float* grad_loss,
                          float* d_depth, colvo_stream_t stream);
/* x [planes,H,W] -> y [planes,H/2,W/2] (mean of each 2x2 block), and its gradient dy -> dx (H, W: the INPUT extent). */
int colvo_avgpool2_fwd(const float* x, int planes, int H, int W, float* y, colvo_stream_t stream);
int colvo_avgpool2_bwd(const float* dy, int planes, int H, int W, float* dx, colvo_stream_t stream);

/* ------------------------------------------------------------------------------------------- *
 * SURVEY.md §8f-1 + §8f-2 in ONE call: the widened objective (spec: dcdp_full_loss)            *
 *   mean_s photometric_loss(pyramid level s) + geo_weight * geometric_consistency_loss        *
 *   + smooth_weight * smoothness_loss, value AND every gradient.                               *
 *   README.md:1 "Considering Geometric and Photometric Consistency", :7.                       *
 * ------------------------------------------------------------------------------------------- */
/* Forward: 3 launches, no host synchronisation -- (1) smoothness (value partials + raw gradient) and two levels of the 2x2-average
 * pyramid of both frames and the target depth in one launch (a fourth level takes one more), (2) the one-pass photometric kernel
 * over ALL levels in one launch (loss + unnormalised gradients; the intrinsics of level s are scaled inside the kernel), whose
 * level-0 part ALSO evaluates the geometric-consistency term on the projection and bilinear taps it has anyway (the reference
 * frame's depth depth_r is a fourth sampled plane), (3) one finalize.  The gradient w.r.t. depth_r is scattered as 64-bit fixed-point
 * atomics (2^-32 units): bit-reproducible.  tgt, ref [B,3,H,W]; depth_t, depth_r [B,1,H,W] (depth_r may be NULL when
 * geo_weight == 0); H, W divisible by 2^(num_scales-1), 1 <= num_scales <= 4.  workspace: colvo_full_objective_workspace_floats()
 * floats, 16-byte aligned, kept untouched until the backward call; loss: one device float.
 * Backward: ONE launch; grad_loss: device scalar dL/dloss; d_depth_t, d_depth_r [B,1,H,W] (d_depth_r may be NULL when
 * geo_weight == 0), d_pose [B,6], d_a, d_b [B].  colvo_full_objective_terms: *state -> 32 device floats inside the workspace:
 * [0] total, [1] geometric term, [2] smoothness term, [4+4s ..] level s: {photometric loss, (1/S)/max(3 n_valid,1), n_valid}. */
size_t colvo_full_objective_workspace_floats(int B, int H, int W, int num_scales);
int colvo_full_objective_fwd(const float* tgt, const float* ref, const float* depth_t, const float* depth_r,
                             const float* pose, const float* K, const float* lcc_a, const float* lcc_b, int B, int H, int W,
                             int num_scales, float ssim_weight, float geo_weight, float smooth_weight, float* workspace,
                             float* loss, colvo_stream_t stream);
int colvo_full_objective_bwd(const float* workspace, const float* grad_loss, const float* pose, int B, int H, int W,
                             int num_scales, float geo_weight, float smooth_weight, float* d_depth_t, float* d_depth_r,
                             float* d_pose, float* d_a, float* d_b, colvo_stream_t stream);
int colvo_full_objective_terms(const float* workspace, int B, int H, int W, int num_scales, const float** state);

/* Un-fused debugging entry (spec: inverse_warp()).  ref [B,C,H,W] -> warped [B,C,H,W], valid [B,1,H,W]. */
int colvo_inverse_warp(const float* ref, const float* depth, const float* pose, const float* K,
                       int B, int C, int H, int W, float* warped, float* valid, colvo_stream_t stream);

/* ------------------------------------------------------------------------------------------- *
 * a1, a2  conv blocks of DepthNet / PoseNet (README.md:5,7 DCDP "depth and pose estimation")  *
 *   spec: oracle/colvo_spec.py DepthNet / PoseNet (F.conv2d + F.relu + nearest up + concat).   *
 *   One implicit-GEMM convolution on NHWC feature maps, MFMA on gfx950; the decoder's nearest  *
 *   2x up-sample and the skip concat are folded into the input gather.                         *
 * ------------------------------------------------------------------------------------------- */
typedef struct ColvoConvDesc {
    int32_t dtype;      /* COLVO_F32 | COLVO_BF16: type of x0, x1, y, dy, dx and of the packed weights */
    int32_t B;          /* images */
    int32_t Ho, Wo;     /* output spatial size */
    int32_t Cout;       /* multiple of 8 */
    int32_t ksize;      /* 3 or 1 (pad = ksize/2) */
    int32_t stride;     /* 1 or 2 */
    int32_t relu;       /* 1: y = max(conv + bias, 0) */
    /* source 0 (and optional source 1, channel-concatenated after source 0) */
    int32_t C0;         /* channels of x0, multiple of 8 */
    int32_t up0;        /* 1: x0 is stored at half resolution and read through nearest 2x up-sampling */
    int32_t C1;         /* channels of x1 (0 = none), multiple of 8 */
    int32_t up1;
    int32_t Hi, Wi;     /* spatial size of the (virtual, i.e. after up-sampling) conv input */
} ColvoConvDesc;

/* y[B,Ho,Wo,Cout] = act(conv(cat(x0,x1)) + bias).  w_fwd: weights packed [Cout][ksize*ksize][C0+C1]
 * in `dtype`; bias fp32 [Cout]. */
int colvo_conv_fwd(const ColvoConvDesc* d, const void* x0, const void* x1, const void* w_fwd,
                   const float* bias, void* y, colvo_stream_t stream);

/* PoseNet's three front layers (8 -> 16 -> 32 -> 64 channels, 3x3, stride 2, bias + ReLU, bf16) as ONE launch: the chain form of
 * COLVO_CMD_CONV_FWD (below; csrc/pose_front.hip).  Plan query, no side effect: reads d1 -- the FIRST layer's descriptor -- and the
 * tuning table, calls no HIP and counts no form.  direction 0: the forward chain (writes all three activation maps; the bits of
 * three colvo_conv_fwd calls).  direction 1: the input-gradient chain, the chain form of COLVO_CMD_CONV_DGRAD_PLANES: from conv3's
 * output gradient g3 it writes g2 = dgrad(conv3) masked by act2 > 0, g1 = dgrad(conv2) masked by act1 > 0 and conv1's input
 * gradient w.r.t. two channels as fp32 planes (the bits of two colvo_conv_dgrad calls and colvo_conv_dgrad_planes; tuning entry
 * `pose_front_bwd` on top of `pose_front`).  Returns 0 when the chain is not selected (tuning entry off, f32, H or W not a multiple
 * of 8, other channel counts, or a batch at which one of the three layers would not take the one-tile form of colvo_conv_fwd --
 * resp. one of the replaced input-gradient launches not k_dgrad_s2 / k_dgrad_planes_s2_mfma: the chain's bits are those forms'
 * bits); otherwise 1, and out (may be NULL) receives {workgroups, conv3 tile rows, conv3 tile columns, LDS bytes}. */
int colvo_pose_front_plan(const ColvoConvDesc* d1, int direction, int32_t* out);

/* PoseNet's deep layers conv5-conv7 (3x3, stride 2, bf16, 128 or 256 input channels of the launch's K) as WHOLE-K RESIDENT launches
 * at small batches (csrc/pose_tail.hip): a workgroup owns 16 output channels x the pixels of whole images, requests its whole weight
 * slab and source maps up front and runs complete K chains out of LDS, instead of walking 4-8 channel chunks one round trip at a
 * time.  Plan query, no side effect: reads d -- the LAYER's descriptor -- and the tuning table, calls no HIP and counts no form.
 * direction 0: the forward pass (the bits of colvo_conv_fwd); direction 1: the input gradient w.r.t. source 0 (the bits of
 * colvo_conv_dgrad without accumulate; tuning entry `pose_tail_bwd` on top of `pose_tail`).  Returns 0 when the layer is not selected:
 * tuning entry off, f32, not stride 2, a second or up-sampled source, K not 128 or 256, output channels not a multiple of 16, more
 * than `pose_tail_max_pairs` images, operands beyond 160 KB of LDS, or a shape at which the plain call would not run the form the
 * bits are tied to (k_conv3x3 over 32-channel chunks forward; k_dgrad_s2, or k_conv3x3 over the zero-dilated dy, backward).
 * Otherwise 1, and out (may be NULL) receives {workgroups, images per workgroup, LDS bytes, kernel kind (0: conv order, 1: k_dgrad_s2
 * order)}.  The form is reached only by explicit request: COLVO_CMD_CONV_FWD with i[0] = -1, COLVO_CMD_CONV_DGRAD with i[2] = 1
 * (below); a request at a shape this query does not select is an error, never a fall-back, and the plain entry points never take it. */
int colvo_pose_tail_plan(const ColvoConvDesc* d, int direction, int32_t* out);

/* Input gradient of source `src` (0 or 1).  dy[B,Ho,Wo,Cout] must already be the gradient w.r.t. the
 * pre-activation (see relu_mask below).  w_bwd: weights packed [C0+C1][ksize*ksize][Cout].
 * dx has the STORED shape of the source (half resolution when up-sampled).
 * relu_mask (may be NULL): the stored output of the layer that produced this source; when given, dx is
 * multiplied by (relu_mask > 0), i.e. dx becomes that producer's pre-activation gradient.
 * accumulate: 0 = overwrite dx, 1 = dx += (fan-out of skip connections). */
int colvo_conv_dgrad(const ColvoConvDesc* d, int src, const void* dy, const void* w_bwd,
                     const void* relu_mask, void* dx, int accumulate, colvo_stream_t stream);
/* The input gradients w.r.t. BOTH sources of a two-source (concat) layer in one launch: dx0 [B][Hi][Wi][C0], dx1 [..][C1];
 * relu_mask0 / relu_mask1 as in colvo_conv_dgrad (may be NULL).  Same results as two colvo_conv_dgrad calls (which it falls
 * back to for strided / up-sampled layers or when C0 is not a multiple of 32). */
int colvo_conv_dgrad_both(const ColvoConvDesc* d, const void* dy, const void* w_bwd, const void* relu_mask0,
                          const void* relu_mask1, void* dx0, void* dx1, colvo_stream_t stream);

/* Input gradient of a 3x3 conv (stride 1 or 2, ONE directly stored source, no ReLU behind it: a network input) w.r.t. a few of its
 * input channels only, as fp32 planes: dst[c][B][1][Hi][Wi] for channels c_begin .. c_begin + c_count - 1 (c_count 1, 2 or 4; every
 * channel a contiguous [B,1,Hi,Wi] tensor of its own).  w_master: the fp32 weights [Cout][9][C0].  PoseNet's first layer: only the
 * two depth channels of its 8-channel input gradient are wanted (DCDP coupling, README.md:7); this replaces the full input gradient +
 * an unpack pass (29 us -> 5 us on the critical path between the two networks' backward passes).  accumulate: dst += . */
int colvo_conv_dgrad_planes(const ColvoConvDesc* d, const void* dy, const float* w_master, int c_begin, int c_count, float* dst,
                            int accumulate, colvo_stream_t stream);

/* The narrow full-resolution layer (bf16, 16 -> 16, stride 1, ReLU, one directly stored source: DepthNet's iconv1) AND the 3x3
 * 16 -> 1 depth head behind it in ONE pass (csrc/fwd16.hip): y = relu(conv(x, w_fwd) + bias) is written (the backward pass needs it)
 * and the head is evaluated on it from LDS -- depth = 1 / (1/max + (1/min - 1/max) sigmoid(conv(y, head_w) + head_b)), [B,1,H,W] fp32 --
 * so the 42 MB tensor is not read back (colvo_conv_fwd + colvo_depth_head_fwd: 21 + 18 us at 16 frames of 256x320).
 * colvo_conv_head_fused_ok: 1 when the layer qualifies. */
int colvo_conv_head_fused_ok(const ColvoConvDesc* d);
/* pose_in (optional; B = 2 * pairs, target frames first): PoseNet's 8-channel bf16 input [pairs][H][W][8] = [tgt rgb | ref rgb |
 * depth_t | depth_r] -- the depth of image b is ALSO written, rounded to bf16, into channel 6 (b < pairs) or 7 of pair b mod pairs;
 * colvo_pack_stem_pose fills the six rgb channels while it packs DepthNet's own input: PoseNet's packing pass disappears. */
int colvo_conv_head_fused(const ColvoConvDesc* d, const void* x, const void* w_fwd, const float* bias, const float* head_w,
                          const float* head_b, float min_depth, float max_depth, void* y, float* depth, void* pose_in,
                          colvo_stream_t stream);
/* frames [B2][3][H][W] fp32 (B2 = 2 * pairs: target frames, then reference frames) -> stem [B2][H][W][8] bf16 (rgb + 5 zero channels,
 * what colvo_pack_nchw writes) AND pose_in [pairs][H][W][8] bf16: rgb channels 0..2 / 3..5, channels 6 / 7 zeroed (the head's pass
 * writes them afterwards). */
int colvo_pack_stem_pose(const float* frames, int B2, int H, int W, void* stem, void* pose_in, colvo_stream_t stream);

/* DepthNet's stem at small batches in ONE launch (csrc/stem.hip): the packing pass above, enc1a (8 -> 32 channels, 3x3, stride 2) and
 * enc1b (32 -> 32, stride 1) behind it, bf16 -- the stem form of COLVO_CMD_PACK_STEM_POSE (below).  A persistent workgroup walks
 * enc1b's output tiles with both weight slabs resident in LDS: the packed input and enc1a's output are written (the backward pass and
 * PoseNet read them) but not read back.  All four tensors hold the bits of colvo_pack_stem_pose and two colvo_conv_fwd calls.
 * Plan query, no side effect: reads d -- ENC1A's descriptor, B = 2 * pairs images; enc1b's is derived from it -- and the tuning
 * table, calls no HIP and counts no form.  Returns 0 when the launch is not selected: tuning entry `stem_fused` off, f32, channel
 * counts other than 8 -> 32 (-> 32), not stride 2, an odd image count, more than `stem_max_pairs` pairs, H or W odd or below 16, a
 * tensor of 1 GiB or more, a tile whose frame patch or LDS does not fit, or a shape at which one of the two plain calls would not run
 * the form the bits are tied to (k_conv3x3 / k_conv3x3_res over one-granule chunks for enc1a, over one 32-channel chunk for enc1b).
 * Otherwise 1, and out (may be NULL) receives {workgroups, tile rows, tile columns, LDS bytes}.  A request at a shape this query does
 * not select is an error, never a fall-back. */
int colvo_stem_plan(const ColvoConvDesc* d, int32_t* out);

/* Input gradient AND weight / bias gradient of a narrow full-resolution layer in ONE pass (csrc/bwd16.hip): bf16, 16 -> 16 channels,
 * stride 1, one directly stored source -- DepthNet's iconv1.  Both backward kernels of such a layer are HBM-bound and read the same
 * two tensors (dy with a halo; the layer's input x as ReLU mask of dx and as second operand of dw): fused, the layer's backward is 3
 * tensor passes instead of 5.  dx = (relu_mask ? x > 0 : 1) * (dy (*) w_bwd), written (not added); dw / db are ADDED to (fp32
 * atomics: colvo_conv_bwd_fused_det is the bitwise repeatable form).  colvo_conv_bwd_fused_ok: 1 when the layer qualifies. */
int colvo_conv_bwd_fused_ok(const ColvoConvDesc* d);
/* head_dpre / head_w (both or neither): the HEAD form for the layer in front of the 3x3 16 -> 1 depth head.  `dy` is then NOT the
 * gradient but the layer's OUTPUT y (post-ReLU) and the gradient is made on the fly from the head's d(pre) plane [B][H][W] (what
 * colvo_depth_head_bwd / _bwd_parts leave in `scratch`; call them with dx = NULL) and its fp32 weights [9][16]:
 * dy[p][c] = (y[p][c] > 0) * sum_t head_w[t][c] * dpre[p + 1 - t] -- the head's input gradient is never written or read back. */
/* head_partials (HEAD form only, optional): the depth head's OWN weight / bias gradient rides along as well -- the kernel has y and
 * d(pre) staged anyway -- as colvo_conv_bwd_fused_head_rows(d) partial rows of 9 * 16 + 1 floats (one per wave, plain stores), which
 * colvo_depth_head_wgrad_reduce then adds to the head's dw [9][16] / db [1] in a fixed order: the 42 MB pass of colvo_depth_head_wgrad
 * over y disappears. */
int colvo_conv_bwd_fused(const ColvoConvDesc* d, const void* dy, const void* w_bwd, const void* x, int relu_mask, void* dx, float* dw,
                         float* db, const float* head_dpre, const float* head_w, float* head_partials, colvo_stream_t stream);
int colvo_conv_bwd_fused_head_rows(const ColvoConvDesc* d);
/* Deterministic form of colvo_conv_bwd_fused: the same pass, but workgroup r STORES its weight / bias sums into row r of `scratch`
 * ([rows][16 * 9 * 16] weight slabs, then [rows][16] bias slabs -- the layout of ColvoWgradSlabs below; every row is written in full,
 * no initialisation needed) and the fixed-tree reduction of colvo_wgrad_reduce_group then ADDS the rows to dw / db in row order, on the
 * same stream right behind the kernel: two launches, no fp32 atomic, bitwise repeatable.  dx is what the atomic form writes, bit for
 * bit.  rows = the launch's grid, a function of (B, H, W), the form and the tuning table alone.  mode: 0 (dy given) or 1 (HEAD form:
 * head_dpre / head_w); head_partials must be NULL -- the head's own weight gradient has no slab form.
 * colvo_conv_bwd_fused_scratch_bytes: rows * 2320 * 4, or 0 for a layer colvo_conv_bwd_fused_ok refuses or another mode; no HIP call,
 * nothing counted.  scratch, dw and db must be 16-byte aligned; a scratch below that size is refused before any launch.
 * dw == NULL: the kernel alone -- dx is written and the rows are left in `scratch` (bias rows hold the sums with db != NULL, which is
 * not written; zeros otherwise); a later colvo_wgrad_reduce_group with {scratch, dw, db, nsplit = scratch bytes / 9280, Cout = 16,
 * Ctot = 16} adds them, on whichever stream the caller orders behind this one (the training step: a weight-gradient stream, like
 * every other layer's second launch).  The scratch must not be written again before that reduction has run. */
size_t colvo_conv_bwd_fused_scratch_bytes(const ColvoConvDesc* d, int mode);
int colvo_conv_bwd_fused_det(const ColvoConvDesc* d, const void* dy, const void* w_bwd, const void* x, int relu_mask, void* dx,
                             float* dw, float* db, const float* head_dpre, const float* head_w, float* head_partials, void* scratch,
                             size_t scratch_bytes, colvo_stream_t stream);
int colvo_depth_head_wgrad_reduce(const float* partials, int rows, float* dw, float* db, colvo_stream_t stream);
/* The 16-channel depth head's weight / bias gradient by MFMA (bf16 feature maps): partial rows ([colvo_depth_head_wgrad_mfma_rows(B, H,
 * W)][9 * 16 + 1] floats, plain stores) from y [B][H][W][16] and the d(pre) plane, then colvo_depth_head_wgrad_reduce.  d(pre) enters
 * the product rounded to bf16 (as y is); fixed order: bitwise repeatable.  colvo_depth_head_wgrad (VALU) stays the fp32 / generic form. */
int colvo_depth_head_wgrad_mfma_rows(int B, int H, int W);
int colvo_depth_head_wgrad_mfma(const void* y, const float* dpre, int B, int H, int W, float* partials, colvo_stream_t stream);

/* Weight + bias gradient, fp32, ADDED into dw[Cout][ksize*ksize][C0+C1] and db[Cout]
 * (the caller zeroes them once per step). */
int colvo_conv_wgrad(const ColvoConvDesc* d, const void* x0, const void* x1, const void* dy,
                     float* dw, float* db, colvo_stream_t stream);
/* The same with a promise: arena_is_zero != 0 says dw and db hold zeros and nothing else writes them while this call runs (the first
 * backward pass behind an optimizer step that cleared the gradients).  Layers whose grid has ONE pixel-range split per weight slab
 * then STORE their sums instead of adding them with fp32 atomics (a third of such a workgroup's life, profiles/r4_wgrad_phases.md);
 * every other layer, and arena_is_zero == 0, is colvo_conv_wgrad.  The result is the same either way. */
int colvo_conv_wgrad_clean(const ColvoConvDesc* d, const void* x0, const void* x1, const void* dy,
                           float* dw, float* db, int arena_is_zero, colvo_stream_t stream);

/* Deterministic weight gradients.  The plain calls end in fp32 atomics (one add per weight and pixel-range split): the sum
 * depends on the order the workgroups finish in, in the last bits.  The _det forms give every split a slab of its own in
 * caller-owned scratch (plain stores) and add the slabs in split order with a second small launch: bitwise repeatable run to
 * run, at the price of that launch.  scratch: >= the matching *_scratch_bytes(), no initialisation needed, private to the call
 * while it runs.  colvo_pose_head_bwd_det needs none: one thread owns each weight column and walks the images in order. */
size_t colvo_conv_wgrad_scratch_bytes(const ColvoConvDesc* d);
int colvo_conv_wgrad_det(const ColvoConvDesc* d, const void* x0, const void* x1, const void* dy, float* dw, float* db,
                         void* scratch, size_t scratch_bytes, colvo_stream_t stream);
/* Grouped form (round 4; optional -- nn.*.group_wgrad -- and NOT the default: see the last sentence).  In-kernel stamps put the fp32
 * atomics that end colvo_conv_wgrad at 6-7.7 us of EVERY launch -- a third of the kernel at 16 frames, whatever the number of splits --
 * against 2.3 us for the slab stores of the _det form, whose per-layer second launch then costs ~7 us again
 * (profiles/r4_wgrad_phases.md).  colvo_conv_wgrad_slabs is the FIRST launch of colvo_conv_wgrad_det only (every pixel-range split
 * stores its sums into its slab of `scratch`; dw / db are not touched; a single split stores a slab too), and
 * colvo_wgrad_reduce_group adds the slabs of up to COLVO_WGRAD_GROUP_MAX such calls to their dw / db in ONE launch, in a fixed order:
 * four or five second launches per backward pass instead of 27, bitwise repeatable.  colvo_conv_wgrad_splits: the number of slabs the
 * call will write (what the group entry needs).  The slabs call refuses a batch it would have to slice (a tensor >= 1 GiB: the slices
 * would share the slabs); use _det there.  IN THE TRAINING STEP the form measured 5 % SLOWER than the atomics at 8 pairs and 2 % at 32
 * (the per-layer _det form: 1.6 %): 180 MB of slabs a step go out to HBM and come back beside bandwidth-bound kernels, and a group's
 * launch waits for both weight-gradient streams, while the atomics -- slow per launch -- ride in L2 under the other streams' kernels. */
#define COLVO_WGRAD_GROUP_MAX 16
typedef struct ColvoWgradSlabs {
    const void* scratch;         /* what colvo_conv_wgrad_slabs wrote: [nsplit][Cout*9*Ctot] weight slabs, then [nsplit][Cout] bias slabs */
    float* dw;                   /* [Cout][9][Ctot], added to */
    float* db;                   /* [Cout] or NULL */
    int32_t nsplit, Cout, Ctot, pad_;
} ColvoWgradSlabs;
int colvo_conv_wgrad_splits(const ColvoConvDesc* d);
int colvo_conv_wgrad_slabs(const ColvoConvDesc* d, const void* x0, const void* x1, const void* dy, void* scratch,
                           size_t scratch_bytes, colvo_stream_t stream);
int colvo_wgrad_reduce_group(const ColvoWgradSlabs* sets, int n, colvo_stream_t stream);
size_t colvo_depth_head_wgrad_scratch_bytes(int B, int H, int W, int C);
int colvo_depth_head_wgrad_det(int dtype, const void* x, const float* dpre, int B, int H, int W, int C, float* dw, float* db,
                               void* scratch, size_t scratch_bytes, colvo_stream_t stream);
int colvo_pose_head_bwd_det(int dtype, const void* x, const float* w, const float* d_pose, const float* d_a, const float* d_b,
                            const float* scale_a, const float* scale_b, int B, int HW, int C, float pose_scale, float lcc_scale,
                            void* dx, float* dw, float* db, colvo_stream_t stream);

/* dy <- dy * (y > 0) in place (first consumer of a ReLU output's gradient when no dgrad produced it). */
int colvo_relu_bwd_inplace(int dtype, const void* y, void* dy, size_t n, colvo_stream_t stream);

/* Master fp32 weights [Cout][kk][Cin] -> the two packed operand layouts in `dtype`:
 * w_fwd [Cout][kk][Cin] and w_bwd [Cin][kk][Cout]. */
int colvo_pack_weights(int dtype, const float* w_master, int Cout, int kk, int Cin,
                       void* w_fwd, void* w_bwd, colvo_stream_t stream);

/* The same for every 3x3 layer of a network in ONE launch.  `table` (device memory) is an array of
 *   struct { int64 w_off, fwd_off, bwd_off; int32 Cout, kk, Cin, blk_begin; }
 * with element offsets into `master` (fp32 arena), `fwd` and `bwd` (flat operand buffers in `dtype`; fwd_off < 0
 * or fwd == NULL skips the forward copy) and the index of the layer's first workgroup; a layer takes
 * kk * ceil(Cout/32) * ceil(Cin/64) workgroups (one 32 x 64 transpose tile of one tap each) and nblocks is their sum. */
int colvo_pack_weights_multi(int dtype, const float* master, const void* table, int nlayers, int nblocks,
                             void* fwd, void* bwd, colvo_stream_t stream);

/* NCHW fp32 planes -> NHWC feature map of `Cpad` channels (zero padded), and back (gradient, fp32 NCHW).
 * src[i] points to an [B,c_i,H,W] tensor; up to 4 sources are concatenated along channels. */
int colvo_pack_nchw(int dtype, const float* const* src, const int32_t* src_channels, int nsrc,
                    int B, int H, int W, int Cpad, void* dst, colvo_stream_t stream);
/* accumulate: bit 0 = add to dst instead of overwriting it; bit 1 = dst is laid out [c_count][B][H][W] (each channel a contiguous
 * [B,1,H,W] tensor of its own) instead of [B,c_count,H,W]. */
int colvo_unpack_nhwc_grad(int dtype, const void* dsrc, int B, int H, int W, int Cpad,
                           int c_begin, int c_count, float* dst_nchw, int accumulate, colvo_stream_t stream);

/* DepthNet head: conv3x3 (C -> 1) + sigmoid + disp_to_depth, output NCHW fp32 [B,1,H,W]; and its
 * backward (d_depth -> dx NHWC [masked by x>0, the producer's ReLU], dw[9*C] += , db[1] +=).
 * scratch: B*H*W floats; it receives the gradient w.r.t. the pre-activation.  dw = db = NULL skips the weight
 * gradient, which colvo_depth_head_wgrad then computes from `scratch` (e.g. on another stream). */
int colvo_depth_head_fwd(int dtype, const void* x, const float* w, const float* bias, int B, int H, int W, int C,
                         float min_depth, float max_depth, float* depth, colvo_stream_t stream);
int colvo_depth_head_bwd(int dtype, const void* x, const float* w, const float* depth, const float* d_depth,
                         int B, int H, int W, int C, float min_depth, float max_depth, float* scratch,
                         void* dx, float* dw, float* db, colvo_stream_t stream);
int colvo_depth_head_wgrad(int dtype, const void* x, const float* dpre, int B, int H, int W, int C,
                           float* dw, float* db, colvo_stream_t stream);
/* colvo_depth_head_bwd with the incoming gradient given in parts (the DCDP step: DepthNet ran on B = 2*Bh images, target
 * frames first): with s = scale_a[0]*scale_b[0], d_depth[b] = g_first[b] + s*g_raw[b] for b < Bh,
 * g_second[b-Bh] + s*g_raw_second[b-Bh] for b >= Bh.  g_first, g_second, g_raw, g_raw_second: [Bh,1,H,W] each, any of them
 * may be NULL (= zero); scale_a, scale_b: device scalars, NULL = 1 (the fused loss hands over d_depth_raw with grad_loss and
 * loss_state + 1; the widened objective hands over finished gradients for both halves).  No concatenated / summed copy is made.
 * dx = NULL: d(pre) only (into `scratch`) -- the input gradient is then made by colvo_conv_bwd_fused's HEAD form. */
int colvo_depth_head_bwd_parts(int dtype, const void* x, const float* w, const float* depth, const float* g_first,
                               const float* g_second, const float* g_raw, const float* g_raw_second, const float* scale_a,
                               const float* scale_b, int B, int H, int W, int C, float min_depth, float max_depth,
                               float* scratch, void* dx, float* dw, float* db, colvo_stream_t stream);

/* PoseNet head: 1x1 conv (C -> 8) + spatial mean + (POSE_SCALE, LCC_SCALE) affine.
 * out (8*B floats) is PLANAR: [ pose B x 6 | lcc_a B | lcc_b B ] so the three results are contiguous views;
 * backward takes the three gradients separately (each may be NULL = zero). */
int colvo_pose_head_fwd(int dtype, const void* x, const float* w, const float* bias, int B, int HW, int C,
                        float pose_scale, float lcc_scale, float* out, colvo_stream_t stream);
/* scale_a, scale_b: device scalars multiplied into the three incoming gradients (NULL = 1): the fused loss hands its
 * gradients over unnormalised together with dL/dloss and 1/max(3 n_valid, 1). */
int colvo_pose_head_bwd(int dtype, const void* x, const float* w, const float* d_pose, const float* d_a,
                        const float* d_b, const float* scale_a, const float* scale_b, int B, int HW, int C,
                        float pose_scale, float lcc_scale, void* dx, float* dw, float* db, colvo_stream_t stream);

/* ------------------------------------------------------------------------------------------- *
 * a8  Adam over the flat parameter arena (torch.optim.Adam semantics, no weight decay)         *
 * ------------------------------------------------------------------------------------------- */
/* step_count: device int32 holding t BEFORE this step (incremented by the kernel, graph-safe).
 * grad_scale multiplies the gradient first (1/world_size for data-parallel sums).  The four arenas must be 16-byte aligned. */
int colvo_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                    float lr, float beta1, float beta2, float eps, float grad_scale,
                    int32_t* step_count, colvo_stream_t stream);
/* The same with the 1-based step number supplied by the host (no device counter, one launch).  Not for steps captured into a
 * hipGraph: the captured t would repeat at every replay -- use colvo_adam_step there. */
int colvo_adam_step_t(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                      float lr, float beta1, float beta2, float eps, float grad_scale, int t, colvo_stream_t stream);
/* fp32 <-> bf16 (round to nearest even) over n elements, 16-byte aligned buffers: the staging copies of a reduced-precision gradient
 * transport (ddp.GradBuckets).  to_bf16 != 0: src fp32 -> dst bf16; 0: src bf16 -> dst fp32 (src is declared const float* for both). */
int colvo_cast_f32_bf16(const float* src, void* dst, size_t n, int to_bf16, colvo_stream_t stream);

/* Zero `bytes` bytes of device memory on `stream` (the gradient arenas, once per step). */
int colvo_zero(void* ptr, size_t bytes, colvo_stream_t stream);
/* Both networks' arenas in ONE launch each (a dependent launch costs ~2.7 us on MI355X before it does anything and the small
 * arena alone does not fill the memory system): colvo_adam_step_t over up to COLVO_MAX_ARENAS arenas with one step number, and
 * the zeroing of up to as many buffers (16-byte aligned, multiples of 16 bytes). */
#define COLVO_MAX_ARENAS 4
typedef struct ColvoAdamArena {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    size_t n;
} ColvoAdamArena;
int colvo_adam_step_multi(const ColvoAdamArena* arenas, int count, float lr, float beta1, float beta2, float eps,
                          float grad_scale, int t, colvo_stream_t stream);
int colvo_zero_multi(void* const* ptrs, const size_t* bytes, int count, colvo_stream_t stream);
/* Adam and the operand copies of the updated weights in ONE pass over any number of arenas: colvo_adam_step[_t] followed by
 * colvo_pack_weights_multi, without the second pass over the parameters (12 bytes per parameter) and its launches.  `table`
 * (device memory) is an array of ColvoAdamPackEntry: kind 0 = the weights of one 3x3 layer ([Cout][kk][Cin] fp32 at element
 * w_off of the four arenas; forward copy at element fwd_off of `fwd` (skipped when fwd is NULL or fwd_off < 0), transposed /
 * tap-flipped copy at bwd_off of `bwd`, both in `dtype`), taking kk * ceil(Cout/32) * ceil(Cin/64) workgroups from blk_begin on;
 * kind 1 = a plain range of n elements at w_off (biases, heads, padding: update only), ceil(n / COLVO_ADAM_PLAIN_PER_WG)
 * workgroups.  nblocks = the sum.  step_count: device step counter (incremented by a second launch; for steps captured into a
 * hipGraph) or NULL, then t is the 1-based step number.  An entry with zero_grad != 0 has its range of `grad` set to ZERO once read
 * (grad is then written, its const notwithstanding): the arena-clearing launch of the next step (colvo_zero_multi, 8.5 us + a
 * dependent launch on the ColVO networks) is not needed. */
#define COLVO_ADAM_PLAIN_PER_WG 2048
typedef struct ColvoAdamPackEntry {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    void* fwd;
    void* bwd;
    int64_t w_off, fwd_off, bwd_off, n;
    int32_t Cout, kk, Cin, blk_begin;
    int32_t kind, zero_grad;
} ColvoAdamPackEntry;
int colvo_adam_pack_step(int dtype, const void* table, int nentries, int nblocks, float lr, float beta1, float beta2,
                         float eps, float grad_scale, int32_t* step_count, int t, colvo_stream_t stream);
/* ... with a second gradient factor read from the DEVICE at execution time (NULL: none): every gradient is multiplied by
 * grad_scale * *grad_scale_dev first.  For data parallel with the loss normalisation taken off the critical path
 * (colvo_warp_loss_rescale_to): grad_scale = 1 / world from the host, *grad_scale_dev = world / max(3 n_global, 1) from the
 * two-float all-reduce that ran beside the backward pass. */
int colvo_adam_pack_step_scaled(int dtype, const void* table, int nentries, int nblocks, float lr, float beta1, float beta2,
                                float eps, float grad_scale, const float* grad_scale_dev, int32_t* step_count, int t,
                                colvo_stream_t stream);

/* ------------------------------------------------------------------------------------------- *
 * SURVEY.md §8f-3  inference: dense depth maps stitched along the integrated trajectory into a  *
 *   world-frame point cloud (README.md:9, :29).  spec: backproject / stitch_point_cloud.        *
 * ------------------------------------------------------------------------------------------- */
/* depth [B,1,H,W], K [B,3,3], cam2world [B,4,4] (row-major; the trajectory integration itself is N tiny 4x4 products and
 * stays on the host) -> points [B,H*W,3] in row-major pixel order. */
int colvo_backproject(const float* depth, const float* K, const float* cam2world, int B, int H, int W,
                      float* points, colvo_stream_t stream);
/* Every `stride`-th pixel (rows and columns) of N frames whose depth is < max_depth, back-projected and compacted in
 * frame-major, row-major order (deterministic: counts + scan, no atomics).  points must hold
 * N*ceil(H/stride)*ceil(W/stride)*3 floats; n_points[0] receives the number of points written.
 * The comparison is the float32 one, d < max_depth with max_depth as this call receives it: NaN and +inf are dropped; -inf, 0 and
 * negative depths are kept.  The world point is float32 in an order that is not pinned (products and sums may be contracted): it
 * lies within 7 u (|r0 px| + |r1 py| + |r2 d| + |t|), u = 2^-24, of the exact value of px = (u - cx) / fx * d, X = r0 px + r1 py +
 * r2 d + t on the float32 inputs (tests/reconstruct_ref.py).
 * workspace: colvo_stitch_workspace_ints(N,H,W,stride) int32; on return it holds the exclusive prefix sums of the kept counts of
 * the 256-sample blocks (ceil(ceil(H/stride)*ceil(W/stride) / 256) per frame, frame-major).
 * Limits: N <= 65535, H*W < 2^30, N * blocks per frame < 2^30 and N*ceil(H/stride)*ceil(W/stride) < 2^31 (a point's row is an
 * int32); a shape beyond them is refused before the pointers are looked at. */
size_t colvo_stitch_workspace_ints(int N, int H, int W, int stride);
int colvo_stitch_point_cloud(const float* depths, const float* K, const float* cam2world, int N, int H, int W,
                             int stride, float max_depth, int32_t* workspace, float* points, int32_t* n_points,
                             colvo_stream_t stream);

/* Fusion of N depth maps into one point per occupied voxel: mean position, mean colour and observation count of
 * the samples that fell into each voxel of a regular grid (lower corner ox, oy, oz; nx * ny * nz voxels of edge voxel_size, each
 * extent a positive multiple of 8; brick = 8x8x8 voxels).  Samples are the pixels colvo_stitch_point_cloud walks with
 * 0 < depth < max_depth; the world point is float32 with every operation individually rounded (no FMA contraction) in the order
 * px = ((u - cx) / fx) * d, X_a = ((r_a0 * px + r_a1 * py) + r_a2 * d) + t_a; g_a = (X_a - o_a) * (1.0f / voxel_size); inside iff
 * 0 <= g_a < n_a; voxel floor(g_a); sub-voxel quantum floor(frac(g_a) * 256); colour quantum clamp(rint(c * 255), 0, 255), NaN -> 0.
 * Per voxel the count and the sums of the quanta are kept as unsigned integers (integer atomics only: bit-identical between calls,
 * streams and frame orders).  Rows come out in ascending (brick index (bz * nby + by) * nbx + bx, local index (lz * 8 + ly) * 8 + lx).
 * Four phases; the caller reads n_bricks back after the plan and M after the count to size the pool and the outputs:
 *   plan        marks the bricks that hold a sample and numbers them in ascending order.  stats (device int32[3]): kept samples,
 *               kept samples outside the grid, occupied bricks.  workspace: colvo_fuse_plan_workspace_bytes bytes.
 *   accumulate  clears the pool (colvo_fuse_pool_bytes(n_bricks) bytes = n_bricks * 512 records of 32 bytes) and adds every inside
 *               sample to its record.  colors [N,3,H,W] in [0,1], or NULL (no colour sums).
 *   count       rows per brick with count >= min_obs, scanned.  stats2 (device int32[3]): occupied voxels, rows M, overflow flag
 *               (a voxel with 2^24 or more samples: its 32-bit sums may have wrapped).  extract_ws:
 *               colvo_fuse_extract_workspace_bytes(n_bricks) bytes.
 *   write       points[m][a] = float(double(o_a) + (double(i_a) + (double(sum q_a) + 0.5 * n) / (256.0 * n)) * double(voxel_size)),
 *               colors[m][k] = float(double(sum c_k) / (255.0 * n)) (NULL: not written), counts[m] = n, voxels[m] = (ix, iy, iz).
 *               min_obs as given to the count; n_rows = M, the rows the outputs hold (no row beyond it is written).
 * Limits: N <= 65535, H*W < 2^30, fewer than 2^31 samples, fewer than 2^28 bricks in the grid, n_bricks < 2^22, voxel_size finite
 * and positive, workspaces, pool 16-byte aligned.  The size functions return 0 for what the calls refuse. */
size_t colvo_fuse_plan_workspace_bytes(int N, int H, int W, int stride, int nx, int ny, int nz);
int colvo_fuse_plan(const float* depths, const float* K, const float* cam2world, int N, int H, int W, int stride, float max_depth,
                    float ox, float oy, float oz, float voxel_size, int nx, int ny, int nz, void* workspace, int32_t* stats,
                    colvo_stream_t stream);
size_t colvo_fuse_pool_bytes(int n_bricks);
int colvo_fuse_accumulate(const float* depths, const float* colors, const float* K, const float* cam2world, int N, int H, int W,
                          int stride, float max_depth, float ox, float oy, float oz, float voxel_size, int nx, int ny, int nz,
                          const void* workspace, int n_bricks, void* pool, colvo_stream_t stream);
size_t colvo_fuse_extract_workspace_bytes(int n_bricks);
int colvo_fuse_count(const void* pool, int n_bricks, int min_obs, void* extract_ws, int32_t* stats2, colvo_stream_t stream);
int colvo_fuse_write(const void* workspace, const void* pool, int n_bricks, int min_obs, float ox, float oy, float oz,
                     float voxel_size, int nx, int ny, int nz, const void* extract_ws, int n_rows, float* points, float* colors,
                     int32_t* counts, int32_t* voxels, colvo_stream_t stream);

/* Surface normals of a fused cloud: a finite-difference normal per sample of the depth maps, summed per voxel as
 * integers in the row the voxel has in the cloud.  depths, K, cam2world, N, H, W, stride, max_depth and the grid are the ones the
 * cloud was fused with (else samples end in stats[3]); voxels [M,3] int32 are the cloud's voxel indices in its ascending (brick,
 * voxel in brick) order; rel_edge is the largest relative depth difference a finite difference may span.  Float32, every operation
 * individually rounded in the order written (no FMA contraction), correctly rounded divisions and square roots; float32 denormals
 * are kept (the library is built with HIP's default float_denorm_mode_32 = 3), as NumPy keeps them.  cam2world's rotation block r is
 * taken as orthonormal and finite.  Per walked sample c = (u, v) of frame b with 0 < d_c < max_depth (the fusion's walk and rule):
 *   points     for c and its four neighbours, ONE pixel away in the full-resolution map whatever the stride:
 *              P = (((u - cx) / fx) * d, ((v - cy) / fy) * d, d).
 *   usable     a neighbour b is usable iff it lies inside the image, 0 < d_b < max_depth and |d_b - d_c| < rel_edge * (d_b + d_c).
 *   tangents   along u: P(u+1) - P(u-1) if both neighbours are usable, P(u+1) - P(c) if only the right one, P(c) - P(u-1) if only
 *              the left one, else none; along v likewise.  No tangent on either axis: no normal.
 *   normal     n = t_u x t_v, each component two products and one subtraction (n_x = t_u.y * t_v.z - t_u.z * t_v.y, cyclic); negated
 *              iff (n_x * P_x + n_y * P_y) + n_z * P_z > 0 with P = P(c), so that it faces the camera.
 *   length     L = sqrtf((n_x^2 + n_y^2) + n_z^2); the sample has a normal iff L > 0 and L < inf (NaN falls out).
 *   world      e = n / L;  N_a = (r_a0 * e_x + r_a1 * e_y) + r_a2 * e_z;  q_a = (int) rintf(N_a * 16384.0f).
 *   voxel      the fusion's routine on (u, v, d_c): brick and local index; the row is the one whose key brick * 512 + local equals
 *              the sample's, found by binary search among the rows' keys (computed from `voxels`).
 *   sums       per row four 64-bit integers: sum q_x, sum q_y, sum q_z, n (native integer atomics: bit-identical between calls,
 *              streams and frame orders).  With n < 2^24 no sum exceeds 2^39.
 * Write-out in float64, every operation individually rounded: len = sqrt((sx * sx + sy * sy) + sz * sz); normals[m][a] =
 * float(s_a / len); coherence[m] = float(len / (16384.0 * n)) -- 1 where all observations agree on the orientation, towards 0 as they
 * disagree --; counts[m] = n; with n = 0 or len = 0 the normal and the coherence are 0.
 * stats (device int32[4]): samples walked and kept; of those, samples with a normal; of those, samples whose voxel is a row of the
 * cloud; and samples whose voxel is not (below the cloud's min_obs, or outside the grid).
 * `voxels` that are not sorted or not the cloud's: unspecified values, but no index leaves the arrays.
 * scratch: colvo_cloud_normals_scratch_bytes(M) bytes, 16-byte aligned (32 bytes of sums and an 8-byte key per row, 16 KiB of counter
 * lines), written by the call; 0 for M < 0.  No read-back and no host synchronisation.
 * Limits: those of colvo_fuse_* (N <= 65535, H*W < 2^30, fewer than 2^31 samples, fewer than 2^28 bricks in the grid, voxel_size
 * finite and positive), 0 <= M < 2^31 (voxels and the three outputs may be NULL when M = 0), max_depth and rel_edge finite and
 * positive; refused before any HIP call with a message that starts `colvo_cloud_normals:`. */
size_t colvo_cloud_normals_scratch_bytes(int M);
int colvo_cloud_normals(const float* depths, const float* K, const float* cam2world, int N, int H, int W, int stride, float max_depth,
                        float ox, float oy, float oz, float voxel_size, int nx, int ny, int nz, const int32_t* voxels, int M,
                        float rel_edge, void* scratch, float* normals, int32_t* counts, float* coherence, int32_t* stats,
                        colvo_stream_t stream);

/* TSDF fusion and surface-net meshing (csrc/tsdf.hip; replica tests/tsdf_ref.py, which the outputs equal bit for
 * bit).  The grid, its 8x8x8 bricks and their ascending order are colvo_fuse_*'s.  T = trunc / voxel_size is a whole number of voxels,
 * 1 <= T <= 7; trunc = (float)T * voxel_size and inv_trunc = 1.0f / trunc are computed in float32 on the host.  Float32 below means
 * every operation individually rounded in the order written (no FMA contraction), divisions correctly rounded.
 *   plan        every sample the fusion walks (stride, 0 < d < max_depth) marks, for k = -(T+1) .. T+1 with d_k = d + (float)k *
 *               voxel_size > 0, the brick that the fusion's world-point routine gives for (u, v, d_k), if inside the grid.  The marks
 *               are numbered in ascending brick order: table [bricks of the grid] int32 = slot or -1, brick_list [min(bricks, 2^22)]
 *               int32 = brick of each slot.  stats (device int32[3]): kept samples, kept samples whose own point (k = 0) lies outside
 *               the grid, allocated bricks.  scratch: colvo_tsdf_plan_scratch_bytes bytes.
 *   integrate   full-resolution depths whatever the plan's stride.  Per voxel (ix, iy, iz) of an allocated brick and per frame, in
 *               any order: c_a = o_a + ((float)i_a + 0.5f) * voxel_size; camera point q = c - t, P_x = (r_00 q_0 + r_10 q_1) + r_20 q_2
 *               (the renderers' routine); Pz > 1e-3f; x = (fx * Px) / Pz + cx, u = (int)floorf(x + 0.5f), 0 <= u < W, y and v
 *               likewise; d = depths[f,0,v,u] with 0 < d < max_depth; sdf = d - Pz; skipped if sdf < -trunc; q = (int)rintf(
 *               (fminf(sdf, trunc) * inv_trunc) * 4096.0f).  pool [n_bricks * 512][2] int32 receives (sum q, n) per voxel, row
 *               slot * 512 + (lz * 8 + ly) * 8 + lx, 8 bytes; with colors [N,3,H,W], color_sums [n_bricks * 512][4] int32 receives
 *               the sums of clamp(rint(c * 255), 0, 255) (NaN -> 0) of the same pixel and a zero, 16 bytes (colors and color_sums
 *               are NULL together).  With N <= 65535 no sum leaves int32 (|sum q| <= 65535 * 4096).  Both arrays are written whole:
 *               they need not be cleared.  Frames that provably add nothing to a brick are skipped (tuning entry tsdf_cull); the
 *               sums are integers, so no bit depends on that.  survivors: NULL, or int32[n_bricks] = frames each brick walked.
 *   mesh        a voxel is observed iff its brick is allocated and n >= min_obs, inside iff sum q < 0.  Cell (i, j, k), considered
 *               iff voxel (i, j, k) lies in an allocated brick, has the voxels (i..i+1, j..j+1, k..k+1) as corners c = x + 2 y + 4 z;
 *               it is active iff all eight are observed and their signs are mixed, open iff the signs of the observed ones are mixed
 *               and one or more is not observed (a voxel outside the grid is not observed).  An active cell has one vertex; vertices
 *               are ordered by (slot, local index) of voxel (i, j, k).  With phi_c = (double)sum q / (double)n, over the 12 edges (a, b)
 *               in the order: axis x, y, z; per axis the two other coordinates (0,0), (1,0), (0,1), (1,1), lower axis first; an edge
 *               whose ends differ in sign adds its crossing a + (b - a) * (phi_a / (phi_a - phi_b)) (the axis coordinate is the
 *               quotient, the others are a's 0.0 or 1.0) to a float64 sum; m = sum / (double)crossings;
 *               vertices[v][a] = float(double(o_a) + ((double(i_a) + 0.5) + m_a) * double(voxel_size)); cells[v] = (i, j, k);
 *               normals[v] = float(g_a / sqrt((g_x g_x + g_y g_y) + g_z g_z)), g_a = ((e_0 + e_1) + e_2) + e_3 with e_p = phi_b -
 *               phi_a of the axis' four edges in the order above: it points to free space; (0, 0, 0) for a zero gradient;
 *               colors[v][k] = float((sum over c = 0..7 of double(sum c_k) / (255.0 * double(n))) / 8.0).  All float64, every
 *               operation rounded once, divisions and the square root correctly rounded: bit for bit the replica's.
 *               vertex_ids [n_bricks * 512] int32 receives every considered cell's vertex, or -1.
 *               The grid edge from voxel v (in an allocated brick) to v + e_axis has a quad iff the four cells around it -- A = v -
 *               e_u - e_w, B = v - e_w, C = v, D = v - e_u, u = axis + 1, w = axis + 2 cyclic -- are active and its ends differ in
 *               sign: triangles (A, B, C), (A, C, D) if v is the inside end, else (A, C, B), (A, D, C): the geometric normal points
 *               from the inside end to the outside end.  faces [F][3] int32, ordered by (slot, local index of v, axis).
 *     count     stats2 (device int32[2]): vertices V, open cells.  scratch: colvo_tsdf_mesh_scratch_bytes(n_bricks) bytes.
 *     vertices  writes the V vertices (n_vertices = V: no row beyond it is written) and vertex_ids, counts the triangles:
 *               n_faces (device int32[1]) = F.
 *     faces     writes the F triangles (n_faces = F, even).
 * Limits: those of colvo_fuse_* (N <= 65535, H*W < 2^30, fewer than 2^31 walked samples, fewer than 2^28 bricks in the grid, n_bricks
 * < 2^22, voxel_size finite and positive), 1 <= T <= 7, min_obs >= 1, F < 2^31; pool, color_sums, table, brick_list and scratch
 * 16-byte aligned.  Refused before any HIP call with a message that starts with the entry's name; the size functions return 0 for
 * what the calls refuse. */
size_t colvo_tsdf_plan_scratch_bytes(int N, int H, int W, int stride, int nx, int ny, int nz);
int colvo_tsdf_plan(const float* depths, const float* K, const float* cam2world, int N, int H, int W, int stride, float max_depth,
                    float ox, float oy, float oz, float voxel_size, int nx, int ny, int nz, int T, void* scratch, int32_t* table,
                    int32_t* brick_list, int32_t* stats, colvo_stream_t stream);
int colvo_tsdf_integrate(const float* depths, const float* colors, const float* K, const float* cam2world, int N, int H, int W,
                         float max_depth, float ox, float oy, float oz, float voxel_size, int nx, int ny, int nz, int T,
                         const int32_t* brick_list, int n_bricks, void* pool, void* color_sums, int32_t* survivors,
                         colvo_stream_t stream);
size_t colvo_tsdf_mesh_scratch_bytes(int n_bricks);
int colvo_tsdf_mesh_count(const void* pool, const int32_t* table, const int32_t* brick_list, int n_bricks, int min_obs, int nx, int ny,
                          int nz, void* scratch, int32_t* stats2, colvo_stream_t stream);
int colvo_tsdf_mesh_vertices(const void* pool, const void* color_sums, const int32_t* table, const int32_t* brick_list, int n_bricks,
                             int min_obs, float ox, float oy, float oz, float voxel_size, int nx, int ny, int nz, void* scratch,
                             int n_vertices, float* vertices, float* colors, float* normals, int32_t* cells, int32_t* vertex_ids,
                             int32_t* n_faces, colvo_stream_t stream);
int colvo_tsdf_mesh_faces(const void* pool, const int32_t* table, const int32_t* brick_list, int n_bricks, int nx, int ny, int nz,
                          const void* scratch, const int32_t* vertex_ids, int n_faces, int32_t* faces, colvo_stream_t stream);

/* Polyp localisation: labelled pixels + depth maps + trajectory -> where each polyp lies, in the camera frame of
 * every frame that shows it and in the world frame, and how large it is.  labels [N,1,H,W] uint8: 0 background, 1..num_labels a
 * polyp id (the same polyp in every frame: association is the detector's or tracker's job), anything above num_labels is ignored
 * and counted.  The walked pixels are colvo_stitch_point_cloud's: (u, v) = (i * stride, j * stride).  A labelled pixel of (n, l) is
 * a walked pixel of frame n carrying label l; a sample is a labelled pixel with 0 < d < max_depth (NaN falls out) that, with clip
 * bounds, also passes the clip test below.
 * Pinned arithmetic, float32, every operation individually rounded (no FMA contraction):
 *   px = ((u - cx) / fx) * d, py = ((v - cy) / fy) * d, pz = d;  q_a = (int32) rintf(p_a * 4096.0f).
 * A record (128 bytes, 16 words of 64 bits) per (n, l), integers only: labelled pixels, samples, sum u, sum v over the samples,
 * sum q_x, q_y, q_z (signed), sum q_a q_b in the order xx, xy, xz, yy, yz, zz (signed), the inclusive bounding box of the
 * labelled pixels.  Added with 64-bit integer adds and 32-bit integer max: bit-identical between calls and streams.  The caller
 * guarantees |p_a| * 4096 < 2^31 and (|p_a| * 4096)^2 * ceil(H/stride) * ceil(W/stride) < 2^62 (localize.py checks both from K and
 * max_depth before any launch).
 *   workspace   colvo_localize_workspace_bytes(N, num_labels) bytes: the records [N][num_labels], then one ignored-pixel count per
 *               frame.  0 for what the calls refuse.
 *   accumulate  clears the workspace and adds every labelled pixel and sample.  clip_bounds: NULL, or [N][num_labels][2] doubles
 *               (mean_z, limit) from colvo_localize_bounds: a sample must then satisfy, in float64,
 *               (double(q_z) / 4096.0 - mean_z)^2 <= limit.  Labelled-pixel counts and boxes do not depend on the clip.
 *   bounds      per (n, l) with n = samples >= 2: mean_z = double(sum q_z) / (4096.0 * double(n)),
 *               var_z = max(0, double(sum q_z q_z) / (16777216.0 * double(n)) - mean_z * mean_z),
 *               limit = (double(clip_sigma) * double(clip_sigma)) * var_z; with n < 2: mean_z = 0, limit = +inf (nothing is clipped).
 *   finish      per (n, l), float64, n = n_samples[n][l], everything NaN where n = 0:
 *                 bbox = (u0, v0, u1, v1), -1 where n_pixels = 0;  pixel = (double(sum u) / double(n), double(sum v) / double(n));
 *                 m_a = center_cam[a] = double(sum q_a) / (4096.0 * double(n));
 *                 cov_cam[ab] = double(sum q_a q_b) / (16777216.0 * double(n)) - m_a * m_b   (order xx, xy, xz, yy, yz, zz);
 *                 center_world[a] = ((r_a0 * m_x + r_a1 * m_y) + r_a2 * m_z) + t_a   (cam2world's float32 entries widened).
 *               per label l, over the frames with n >= min_samples in ascending frame order (a frame below it is skipped), with
 *               C the symmetric cov_cam, c = center_world, T_ab = (r_a0 * C_0b + r_a1 * C_1b) + r_a2 * C_2b,
 *               S_ab = ((T_a0 * r_b0 + T_a1 * r_b1) + T_a2 * r_b2) + c_a * c_b:
 *                 n_frames, n_samples_total = sum n (integers), first_frame, last_frame (-1 if never seen);
 *                 position[a] = p_a = (sum_n double(n) * c_a) / double(n_samples_total);
 *                 cov_world[ab] = (sum_n double(n) * S_ab) / double(n_samples_total) - p_a * p_b;  NaN if never seen.
 *               stats (device int64[2]): labelled pixels, ignored pixels (label above num_labels), over all frames.
 * Limits: N <= 65535, H*W < 2^30, num_labels in 1..255, stride >= 1, max_depth finite and positive, clip_sigma finite and not
 * negative, min_samples >= 1; records and clip_bounds 16-byte aligned. */
size_t colvo_localize_workspace_bytes(int N, int num_labels);
int colvo_localize_accumulate(const float* depths, const uint8_t* labels, const float* K, int N, int H, int W, int stride,
                              float max_depth, int num_labels, const double* clip_bounds, void* records, colvo_stream_t stream);
int colvo_localize_bounds(const void* records, int N, int num_labels, float clip_sigma, double* clip_bounds, colvo_stream_t stream);
int colvo_localize_finish(const void* records, const float* cam2world, int N, int num_labels, int min_samples, int32_t* n_pixels,
                          int32_t* n_samples, int32_t* bbox, double* pixel, double* center_cam, double* cov_cam,
                          double* center_world, int32_t* n_frames, int64_t* n_samples_total, int32_t* first_frame,
                          int32_t* last_frame, double* position, double* cov_world, int64_t* stats, colvo_stream_t stream);

/* Multi-view depth consistency: a pixel of frame i keeps its depth only if neighbouring frames, through the
 * trajectory, see the same surface there.  depths [N,1,H,W], K [N,3,3] (per frame), cam2world [N,4,4], all float32.  The
 * neighbours of frame i are the frames j = i + k * step, k = -window..-1, 1..window, that exist in [0, N): 2 * window slots in
 * ascending j.  Float32, every operation individually rounded in the order written (no FMA contraction), plain divisions:
 *   transforms  for every (i, slot) whose j exists, [R|t] maps frame-i camera coordinates into frame j; float64 from the float32
 *               cam2world (rotation block taken as orthonormal; Ri, ti / Rj, tj its blocks for i / j), each value rounded to float32:
 *                 R[a][b] = (Rj[0][a] * Ri[0][b] + Rj[1][a] * Ri[1][b]) + Rj[2][a] * Ri[2][b],
 *                 t[a]    = (Rj[0][a] * (ti[0] - tj[0]) + Rj[1][a] * (ti[1] - tj[1])) + Rj[2][a] * (ti[2] - tj[2]).
 *   candidate   pixel (i, u, v) with d = depth_i[v][u] is a candidate iff 0 < d < max_depth (NaN falls out).
 *   neighbour   px = ((u - cx_i) / fx_i) * d, py = ((v - cy_i) / fy_i) * d, P_a = ((R_a0 * px + R_a1 * py) + R_a2 * d) + t_a;
 *               front iff P_z > 1e-3f;  x = (fx_j * P_x) / P_z + cx_j, y = (fy_j * P_y) / P_z + cy_j;
 *               inside iff 0 <= x <= W - 1 and 0 <= y <= H - 1;  x0 = floor(x), wx = x - x0, x1 = min(x0 + 1, W - 1), the same in y;
 *               taps t00 = depth_j[y0][x0], t01 = [y0][x1], t10 = [y1][x0], t11 = [y1][x1], valid iff each has 0 < t < max_depth;
 *               s = (((t00 * (1 - wx)) + (t01 * wx)) * (1 - wy)) + (((t10 * (1 - wx)) + (t11 * wx)) * wy);
 *               rel = |P_z - s| / (P_z + s).  The neighbour is visible iff front, inside and taps valid; a visible neighbour counts
 *               as AGREE if rel < rel_tol, else as OCCLUDED if s < P_z (frame j has a surface in front of the point), else as
 *               VIOLATED (frame j sees through the point).
 *   keep        a pixel is kept iff it is a candidate, agree >= min_agree and violated <= max_violated.
 *   outputs     out_depths [N,1,H,W] float32: the input depth where kept, +inf elsewhere (dropped by the `d < max_depth` of
 *               colvo_stitch_point_cloud and by the `0 < d < max_depth` of the fusion and the localisation);
 *               out_votes [N,3,H,W] uint8: planes agree, occluded, violated (0 where no candidate);
 *               out_stats [N,5] int32 per frame: candidates, kept, no_view (a candidate without a visible neighbour that is not kept:
 *               min_agree = 0 keeps it), few_agree (a candidate with a visible neighbour, violated <= max_violated and
 *               agree < min_agree), violated_out (a candidate with violated > max_violated); the last four sum to the first.  Integer sums: identical bits on every call and stream.
 * workspace: colvo_consistency_workspace_bytes(N, window) bytes, 16-byte aligned: the transform table [N][2 * window][12] (R row-major,
 * then t) and the per-frame counters, both written by the call.  0 for what the call refuses.
 * Limits: N <= 65535, H*W < 2^30, window in 1..16, step >= 1, 0 <= min_agree <= 2 * window, max_violated >= 0, rel_tol and
 * max_depth finite and positive. */
size_t colvo_consistency_workspace_bytes(int N, int window);
int colvo_consistency_filter(const float* depths, const float* K, const float* cam2world, int N, int H, int W, int window, int step,
                             float rel_tol, int min_agree, int max_violated, float max_depth, void* workspace, float* out_depths,
                             uint8_t* out_votes, int32_t* out_stats, colvo_stream_t stream);

/* Point cloud into camera views: z-buffered, screen-aligned square splats.  points [M,3] float32 in the world frame,
 * colors [M,3] float32 or NULL, K [N,3,3] (per frame), cam2world [N,4,4] float32 (the rotation block r is taken as orthonormal, t its
 * translation), images of H x W pixels, radius in world units, max_splat the largest half-width of a footprint in pixels.  Float32,
 * every operation individually rounded in the order written (no FMA contraction), plain divisions.  Per frame n and point i (X):
 *   camera      q_a = X_a - t_a,  P_a = (r_0a * q_0 + r_1a * q_1) + r_2a * q_2  (the transposed rotation applied to X - t).
 *   front       iff P_z > 1e-3f and P_z < max_depth (NaN falls out).
 *   centre      x = (fx * P_x) / P_z + cx, y = (fy * P_y) / P_z + cy;  hx = (fx * radius) / P_z, hy = (fy * radius) / P_z;
 *               clipped iff hx > max_splat or hy > max_splat; then hx = hx > max_splat ? max_splat : hx, the same for hy.
 *   on screen   iff x >= -(max_splat + 1), x <= (float)(W + max_splat), y >= -(max_splat + 1), y <= (float)(H + max_splat): NaN and
 *               infinities fail, and what passes converts to an integer safely.
 *   footprint   uc = floor(x + 0.5f), u_lo = max((int)min(ceil(x - hx), uc), 0), u_hi = min((int)max(floor(x + hx), uc), W - 1)
 *               (the inner min / max on floats, the outer on integers), the same in v with y, hy, H: a splat smaller than a pixel
 *               still lands on its nearest pixel.  The point is drawn iff front, on screen, u_lo <= u_hi and v_lo <= v_hi.
 *   key         (uint64(bits(P_z)) << 32) | uint32(i); P_z is positive, so its bits order as unsigned integers.  Every pixel of the
 *               footprint takes the minimum key: the nearest point wins, equal depths go to the smallest index.
 *   outputs     out_depth [N,1,H,W] float32: the winning P_z, +inf where no point landed (dropped by the `d < max_depth` of
 *               colvo_stitch_point_cloud and the `0 < d < max_depth` of the fusion, the localisation and the consistency filter);
 *               out_index [N,1,H,W] int32: the winning point, -1 where empty;  out_colors [N,3,H,W] float32: colors[index], 0 where
 *               empty -- written iff out_colors is given; colors must then be given too (it may be NULL when M = 0) and must be
 *               NULL otherwise;  out_stats [N,4] int32 per frame: points in front, points drawn, points in front and clipped,
 *               covered pixels.  Integer sums and a minimum: identical bits on every call and stream.
 * scratch: colvo_render_scratch_bytes(N, H, W) bytes, 16-byte aligned: the key buffer (N * H * W 64-bit words) and the per-frame
 * counter lines, both written by the call.  0 for a shape the call refuses.  No read-back and no host synchronisation.
 * Limits: 0 <= M < 2^31 (points may be NULL when M = 0), 1 <= N <= 65535, H, W >= 1, H*W < 2^30, N*H*W < 2^31, radius finite and
 * >= 0, max_splat in 0..32, max_depth finite and positive. */
size_t colvo_render_scratch_bytes(int N, int H, int W);
int colvo_render_cloud(const float* points, const float* colors, int M, const float* K, const float* cam2world, int N, int H, int W,
                       float radius, int max_splat, float max_depth, void* scratch, float* out_depth, int32_t* out_index,
                       float* out_colors, int32_t* out_stats, colvo_stream_t stream);

/* Point cloud with normals into camera views: z-buffered oriented discs.  colvo_render_cloud's contract holds --
 * camera, front, centre, clipped, on screen, footprint, the minimum key, outputs, scratch and limits --, with one more input, normals
 * [M,3] float32 in the world frame (any length), and the following differences.  Per frame n and point i (X, N):
 *   has a normal   iff (N_0^2 + N_1^2) + N_2^2 > 0 (NaN fails).  A point without a normal is drawn exactly as colvo_render_cloud draws
 *                  it, a square with one depth, and is counted as flat when it is in front.
 *   camera normal  m_a = (r_0a * N_0 + r_1a * N_1) + r_2a * N_2;  num = (m_x * P_x + m_y * P_y) + m_z * P_z.  A point in front that has
 *                  a normal and num >= 0 faces away from the camera: it draws nothing and is counted as culled.
 *   per pixel      (u, v) of the footprint (the same rectangle) of a point that has a normal and is not culled:
 *                  dx = (float(u) - cx) / fx, dy = (float(v) - cy) / fy;  den = (m_x * dx + m_y * dy) + m_z;  z = num / den;
 *                  e_x = dx * z - P_x, e_y = dy * z - P_y, e_z = z - P_z;  hit iff den < 0, z > 1e-3f, z < max_depth and
 *                  (e_x^2 + e_y^2) + e_z^2 <= radius * radius, all four evaluated (NaN and infinities fail).  A hit offers the key
 *                  (bits(z) << 32) | i.  The nearest pixel (uc, vc), when it lies inside the image and is not hit, offers
 *                  (bits(P_z) << 32) | i: a point in front still lands on at least its nearest pixel.  Any other pixel offers nothing.
 *                  With all normals zero the outputs equal colvo_render_cloud's; with radius = 0 they do unless a point is culled.
 *   outputs        out_depth, out_index, out_colors as there;  out_normal [N,3,H,W] float32 or NULL: the winner's camera normal m,
 *                  0 where the pixel is empty or the winner has no normal;  out_stats [N,6] int32 per frame: points in front, points
 *                  drawn (offered at least one key), points in front and clipped, covered pixels, culled, flat.
 * scratch: colvo_render_scratch_bytes(N, H, W) bytes.  Refusals start `colvo_render_surfels:`; normals may be NULL when M = 0. */
int colvo_render_surfels(const float* points, const float* normals, const float* colors, int M, const float* K, const float* cam2world,
                         int N, int H, int W, float radius, int max_splat, float max_depth, void* scratch, float* out_depth,
                         int32_t* out_index, float* out_colors, float* out_normal, int32_t* out_stats, colvo_stream_t stream);

/* Triangle mesh into camera views: z-buffered rasterisation.  vertices [V,3] float32 in the world frame, faces [F,3]
 * int32 (rows of vertices), colors [V,3] float32 or NULL, K [N,3,3], cam2world [N,4,4] float32 as for colvo_render_cloud, images of
 * H x W pixels, cull_back 0 or 1.  Pixel u has its centre at x = u.  Float32 and float64 operations are individually rounded in the
 * order written (no FMA contraction), plain divisions; edge functions are 64-bit integers.  Per frame n and face f:
 *   camera      each of the three vertices as colvo_render_cloud's camera point P.  A face with an index outside [0, V) is dead in
 *               every frame: never dereferenced, never counted.  A vertex is front iff P_z > 1e-3f and P_z < max_depth (NaN falls
 *               out).  The face is front iff all three are; straddling iff some but not all are: dropped and counted.  There is NO
 *               near-plane clipping: a face that crosses z = 1e-3 or max_depth is lost whole.
 *   projection  of a front face: x = (fx * P_x) / P_z + cx, y = (fy * P_y) / P_z + cy.  In the guard band iff |x| <= 16384 and
 *               |y| <= 16384 for all three vertices (NaN and infinities fail); a front face outside is dropped and counted.
 *               X = (int)rintf(x * 256.0f), Y likewise: 1/256-pixel fixed point, |X|, |Y| <= 2^22.
 *   area        A = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0) in int64.  A == 0: degenerate, dropped and counted.  A < 0: front-facing
 *               (x right, y down: the winding extract_mesh produces).  A > 0: back-facing, always counted, dropped iff cull_back.
 *               When A < 0 vertices 1 and 2 are exchanged and A = -A: the ORIENTED numbering, which everything below uses.
 *   coverage    u_lo = max((min X + 255) >> 8, 0), u_hi = min(max X >> 8, W - 1), the same in v with Y, H (arithmetic shifts).  For the
 *               directed edge a -> b opposite vertex k (1 -> 2, 2 -> 0, 0 -> 1), d = b - a and p = (256 u, 256 v):
 *               E_k = d_x (p_y - a_y) - d_y (p_x - a_x), |E_k| < 2^48, E_0 + E_1 + E_2 = A.  The pixel is covered iff for every k
 *               E_k > 0, or E_k == 0 and the edge is top-left: d_y < 0, or d_y == 0 and d_x > 0.  The pixel centres of a region
 *               tessellated by consistently wound faces are each owned by exactly one face, on shared edges and vertices too.
 *               The face is drawn iff it survived every test above and u_lo <= u_hi and v_lo <= v_hi.
 *   depth       float64: iz_k = 1.0 / (double)P_z,k, w_k = (double)E_k * iz_k, s = (w_0 + w_1) + w_2, z = (float)((double)A / s):
 *               the depth of the ray through the pixel centre on the snapped face.  min P_z,k <= z <= max P_z,k in float32.
 *   key         (uint64(bits(z)) << 32) | uint32(f) into the pixel's minimum: the nearest face wins, equal depths go to the smallest f.
 *   outputs     out_depth [N,1,H,W] float32: the winning z, +inf where empty;  out_index [N,1,H,W] int32: the winning face, -1 where
 *               empty;  out_colors [N,3,H,W] float32 or NULL (colors must be given iff it is; NULL allowed when V = 0):
 *               (float)(((w_0 * c_0 + w_1 * c_1) + w_2 * c_2) / s) of the winner's vertex colours as doubles, 0 where empty;
 *               out_normal [N,3,H,W] float32 or NULL: the winner's unit face normal in the camera frame, float64, the face's own
 *               numbering: a = P_1 - P_0, b = P_2 - P_0, m = a x b (m_x = a_y b_z - a_z b_y, ...), len = sqrt((m_x^2 + m_y^2) +
 *               m_z^2), m / len, negated iff (m_x P_0x + m_y P_0y) + m_z P_0z > 0 of the unit vector, rounded to float32; 0 where
 *               empty or len is 0 or not finite;  out_face_pixels [F] int32 or NULL: the pixels of all frames each face won (cleared
 *               by the call; their sum is the sum of the covered pixels);  out_stats [N,8] int32 per frame: faces front, drawn,
 *               straddling, outside the guard band, back-facing, degenerate, fragments ((face, pixel) offers), covered pixels.
 *               Integer sums (they wrap beyond 2^31) and a minimum: identical bits on every call and stream.
 * scratch: colvo_render_scratch_bytes(N, H, W) bytes, 16-byte aligned.  No read-back and no host synchronisation.
 * Limits, refused before any HIP call with a message that starts `colvo_render_mesh:`: 0 <= V, F < 2^31 (F = 0 or V = 0 gives empty
 * images), 1 <= N <= 65535, 1 <= H, W <= 16384, N*H*W < 2^31, max_depth finite and positive, cull_back in {0, 1}. */
int colvo_render_mesh(const float* vertices, const int32_t* faces, const float* colors, int V, int F, const float* K,
                      const float* cam2world, int N, int H, int W, float max_depth, int cull_back, void* scratch, float* out_depth,
                      int32_t* out_index, float* out_colors, float* out_normal, int32_t* out_face_pixels, int32_t* out_stats,
                      colvo_stream_t stream);

/* Mesh topology: components, edges, boundary loops, areas and lengths, and cleaning (csrc/topology.hip; replica
 * tests/topology_ref.py, which every output equals bit for bit).  vertices [V,3] float32, faces [F,3] int32 (rows of vertices).
 * Definitions.  A face is DEAD iff an index lies outside [0, V) or two of its indices are equal: it joins nothing, has no edges and
 *   no area.  The other faces are live.  A COMPONENT is a class of vertices joined by live faces; a vertex that no live face uses is a
 *   component of its own with no faces.  Components are numbered 0 .. C-1 by ascending smallest vertex.  An EDGE is an unordered pair
 *   of vertices that is a side of a live face; its multiplicity m is the number of live-face sides on it (a face given twice counts
 *   twice); it is BOUNDARY iff m = 1 and NON-MANIFOLD iff m > 2.  A LOOP is a connected component of the graph of the boundary edges
 *   (two rings that touch in a vertex are one loop); loops are numbered 0 .. L-1 by ascending smallest vertex.
 * Measures, float64, every operation individually rounded in the order written (no FMA contraction), division and square root
 *   correctly rounded, coordinates widened from float32.  With `unit` a finite positive float32: area quantum qa = ((double)unit *
 *   (double)unit) * 2^-16, length quantum ql = (double)unit * 2^-16.  Face (i, j, k): a = p_j - p_i, b = p_k - p_i componentwise;
 *   n_x = a_y b_z - a_z b_y, n_y = a_z b_x - a_x b_z, n_z = a_x b_y - a_y b_x; s = (n_x n_x + n_y n_y) + n_z n_z; area = 0.5 *
 *   sqrt(s); quanta = llrint(area / qa), ties to even.  Boundary edge (lo < hi): d = p_hi - p_lo; length = sqrt((d_x d_x + d_y d_y) +
 *   d_z d_z); quanta = llrint(length / ql).  A face or boundary edge whose quotient is NaN or >= 2^62 is UNMEASURED: it adds 0 quanta
 *   and is counted.  The sums are int64 adds (they wrap beyond 2^63).
 * Three calls on one stream, with one scratch of colvo_mesh_topology_scratch_bytes(V, F) bytes (16-byte aligned) that carries state
 * from each to the next, and one stats block (device int32[8], cleared by the first call): [0] C, [1] dead faces, [2] L, [3]
 * unmeasured faces, [4] unmeasured boundary edges, [5] not zero iff a thread exhausted a loop bound (the outputs are then not valid:
 * the caller must raise), [6] sides of live faces, [7] 0.
 *   components  vertex_component [V] int32; face_component [F] int32, -1 for a dead face; stats[0], stats[1].  The caller reads C.
 *   edges       components [C][8] int64: smallest vertex, vertices, faces, edges, boundary edges, non-manifold edges, loops (written
 *               by `loops`; 0 here), area in quanta.  vertex_loop [V] int32: the loop of a vertex on a boundary edge, else -1.
 *               stats[2], [3], [6].  The caller reads L; with L = 0 it is done.
 *   loops       (L >= 1) loops [L][4] int64: smallest vertex, component, edges, length in quanta; adds the loop counts to
 *               components[.][6]; stats[4].
 * Every in-kernel loop has a bound known on entry (a parent chain strictly descends: V links; a union ends or lowers one of its two
 * vertices every round: 2 V + 2 rounds); no thread waits for another thread's store.  One thread per side scans the sides that share
 * its smaller endpoint: quadratic in the edges at one lower endpoint (12 at most on extract_mesh's meshes) -- the limit for general
 * meshes with a vertex of very high degree.
 * Limits, refused before any HIP call with a message that starts with the entry's name: 1 <= V < 2^31, 0 <= F < 2^29 (faces may be
 * NULL when F = 0; the caller handles V = 0 without a call), unit finite and positive, 1 <= C, L <= V.  The size function returns 0 for
 * what the calls refuse. */
size_t colvo_mesh_topology_scratch_bytes(int V, int F);
int colvo_mesh_topology_components(const int32_t* faces, int V, int F, void* scratch, int32_t* vertex_component,
                                   int32_t* face_component, int32_t* stats, colvo_stream_t stream);
int colvo_mesh_topology_edges(const float* vertices, const int32_t* faces, int V, int F, float unit, int C, void* scratch,
                              const int32_t* vertex_component, const int32_t* face_component, int64_t* components,
                              int32_t* vertex_loop, int32_t* stats, colvo_stream_t stream);
int colvo_mesh_topology_loops(const float* vertices, int V, int F, float unit, int C, int L, const void* scratch,
                              const int32_t* vertex_component, const int32_t* vertex_loop, int64_t* components, int64_t* loops,
                              int32_t* stats, colvo_stream_t stream);

/* The mesh without the components a caller drops.  kept [C] uint8: not zero = keep.  Order is preserved.
 *   plan    vertex_map [V] int32: the new row of every vertex of a kept component, -1 for the others; vertex_index [V] int32: the
 *           first V2 entries are the old rows of the new vertices, ascending; face_index [F] int32: the first F2 entries are the old
 *           rows of the live faces of kept components, ascending (a dead face has component -1 and is dropped); counts (device
 *           int32[2]): V2, F2.  A component number outside [0, C) is dropped.  scratch: colvo_mesh_clean_scratch_bytes(V, F) bytes.
 *   write   out_vertices, out_colors, out_normals [V2][3] float32 and out_cells [V2][3] int32: the old rows' bits (colors, normals and
 *           cells may each be NULL with their output); out_faces [F2][3] int32: the old faces' indices through vertex_map.
 * Limits as above; 0 <= V2 <= V, 0 <= F2 <= F, one of them positive.  Refusals start with the entry's name. */
size_t colvo_mesh_clean_scratch_bytes(int V, int F);
int colvo_mesh_clean_plan(const int32_t* vertex_component, const int32_t* face_component, const uint8_t* kept, int V, int F, int C,
                          void* scratch, int32_t* vertex_map, int32_t* vertex_index, int32_t* face_index, int32_t* counts,
                          colvo_stream_t stream);
int colvo_mesh_clean_write(const float* vertices, const float* colors, const float* normals, const int32_t* cells,
                           const int32_t* faces, int V, int F, const int32_t* vertex_map, const int32_t* vertex_index,
                           const int32_t* face_index, int V2, int F2, float* out_vertices, float* out_colors, float* out_normals,
                           int32_t* out_cells, int32_t* out_faces, colvo_stream_t stream);

/* Hole filling: the boundary loops of a mesh as ordered rings, the area each hole spans, and the mesh with the short rings closed by a
 * fan to the ring's mean (csrc/fill.hip; replica tests/fill_ref.py, which every output equals bit for bit).  Inputs:
 * the mesh of colvo_mesh_topology_* (liveness, edges, multiplicity and loops as defined there), that call's vertex_loop [V] and loops
 * [L][4], its `unit`, and the policy max_edges >= 3.
 * Definitions.  A live face (a, b, c) has the directed sides a->b, b->c, c->a.  A side is a BOUNDARY HALF-EDGE iff its unordered edge
 *   has multiplicity 1.  out[v] / in[v] count the boundary half-edges that leave / enter v; succ(v) is the end of the one that leaves v
 *   where out[v] = 1.  A loop is SIMPLE iff every one of its vertices has out = in = 1: its n = loops[l][2] >= 3 half-edges then form one
 *   directed cycle through all its vertices.  Rings that touch in a vertex, borders that run into non-manifold vertices and
 *   inconsistently wound neighbours are not simple.  The RING of a simple loop: ring[0] = loops[l][0] (its smallest vertex), ring[k+1]
 *   = succ(ring[k]).
 * Centre of a simple loop, float64 in the order written (no FMA contraction), q = (double)unit * 2^-16: per ring vertex and coordinate
 *   t = (double)x / q; the loop is UNMEASURED if any t is NaN or |t| >= 2^32; else S = sum of llrint(t) (int64, ties to even) and the
 *   centre's coordinate is (float)(((double)S / (double)n) * q).  Colours (if given) likewise with q = 2^-16; a colour whose t is NaN or
 *   |t| >= 2^32 adds 0 and marks nothing.
 * Fan.  n > 3: ring edge k gives the face (ring[(k+1) mod n], ring[k], c), c the centre's vertex: it holds the reversed half-edge, so
 *   it is wound like its neighbour across the border.  n = 3: the single face (ring[0], ring[2], ring[1]), no new vertex.
 * Hole area: the sum over the fan's faces (i, j, k) of colvo_mesh_topology_*'s face quanta -- a = p_j - p_i, b = p_k - p_i, n = a x b, s
 *   = (n_x n_x + n_y n_y) + n_z n_z, llrint((0.5 * sqrt(s)) / qa) -- with the stored float32 centre widened to double.  A face whose
 *   quotient is NaN or >= 2^62 makes the loop UNMEASURED.  It is computed for every simple loop, filled or not.
 * Centre normal: per fan face the three components 0.5 * n_x, 0.5 * n_y, 0.5 * n_z, each llrint(. / qa) under |t| < 2^62, each summed
 *   as int64 (no second UNMEASURED criterion: |0.5 n_x| <= 0.5 sqrt(s) and a NaN component makes s NaN, so a component fails only on a
 *   face whose area already failed, and such a loop gets no vertex) to (X, Y, Z); len = sqrt((X X + Y Y) + Z Z) in float64; the normal is
 *   ((float)(X / len), (float)(Y / len), (float)(Z / len)), or (0, 0, 0) where len is 0.
 * status [L] int32, the first that applies: 2 NOT_SIMPLE, 3 UNMEASURED, 1 TOO_LONG (n > max_edges), 0 FILLED.
 * Two calls on one stream with one scratch of colvo_mesh_fill_scratch_bytes(V, F, L) bytes (16-byte aligned) that carries state from
 * the first to the second.
 *   plan   status [L]; hole [L][2] int64: the fan faces the write call appends (n, or 1 for n = 3, for a FILLED loop, else 0) and the
 *          hole area in quanta (0 for a NOT_SIMPLE or UNMEASURED loop); ring_offsets [L+1] int32 and ring_vertices [V] int32 (the
 *          first R = ring_offsets[L] entries; the rest 0): the rings of the simple loops in loop order, an empty range for the others;
 *          counts (device int32[8]): [0] R, [1] new vertices, [2] new faces, [3] the longest simple loop's edges, [4] not zero iff a
 *          ranking did not end at its ring's last vertex, [5] simple loops, [6] sides of live faces, [7] not zero iff vertex_loop / loops
 *          are not this mesh's topology.  With [4] or [7] set the outputs are not valid: the caller must raise ([7] is set where a
 *          loop's edge or vertex count, its loops[l][0] not being the smallest vertex on it, or a half-edge off every loop says so).
 *          The ring positions come from ceil(log2(counts[3])) rounds of pointer jumping, one launch each, over (next, distance)
 *          pairs of a list cut at the loop's smallest vertex; the host, which does not know counts[3], launches ceil(log2(min(V,
 *          3 F))) rounds, and those beyond leave at their first instruction.
 *   write  out_vertices, out_colors, out_normals [V + new vertices][3] float32, out_cells likewise int32, out_faces [F + new faces][3]
 *          int32: rows 0 .. V-1 and 0 .. F-1 are the input's bits (dead faces included; colors, normals and cells may each be NULL
 *          with their output).  New vertices in ascending loop number: centre, centre colour, centre normal, cell (-1, -1, -1);
 *          new_vertex_loop [new vertices] int32 their loops.  New faces in (loop, k) order; face_loop [F + new faces] int32: -1 for
 *          the input's faces, else the loop.
 * Every in-kernel loop has a bound known on entry; no thread waits for another thread's store; every index read from vertex_loop,
 * loops or the scratch is checked against its buffer before a gather.  Integer sums: identical bits on every call and stream, and
 * under a permutation of the faces.  One thread per side scans its bucket as in colvo_mesh_topology_edges.
 * Limits, refused before any HIP call with a message that starts with the entry's name: 1 <= V < 2^30, 1 <= F < 2^29, 1 <= L <= V (the
 * caller handles V = 0, F = 0 and L = 0 without a call), unit finite and positive, max_edges >= 3, 0 <= R <= V, new
 * vertices <= L, new faces <= R.  The size function returns 0 for what the calls refuse. */
size_t colvo_mesh_fill_scratch_bytes(int V, int F, int L);
int colvo_mesh_fill_plan(const float* vertices, const int32_t* faces, const float* colors, int V, int F, int L, float unit,
                         int max_edges, const int32_t* vertex_loop, const int64_t* loops, void* scratch, int32_t* status,
                         int64_t* hole, int32_t* ring_offsets, int32_t* ring_vertices, int32_t* counts, colvo_stream_t stream);
int colvo_mesh_fill_write(const float* vertices, const float* colors, const float* normals, const int32_t* cells, const int32_t* faces,
                          int V, int F, int L, int R, int n_new_vertices, int n_new_faces, const void* scratch,
                          const int32_t* vertex_loop, const int32_t* status, const int32_t* ring_offsets, const int32_t* ring_vertices,
                          float* out_vertices, float* out_colors, float* out_normals, int32_t* out_cells, int32_t* out_faces,
                          int32_t* face_loop, int32_t* new_vertex_loop, colvo_stream_t stream);

/* Pose refinement by dense depth and intensity alignment: a few Gauss-Newton steps per edge on the per-pixel geometric
 * and photometric residuals of the two frames it connects, starting from the pose given.  depths [N,1,H,W], frames [N,3,H,W], K [N,3,3]
 * (per frame), float32; edges [E][2] int32 (i, j) ON THE DEVICE.  An edge is (i, j, T): T = [R|t] maps frame-i camera coordinates into
 * frame j, float64 state (T arrays are [E][4][4] row-major; rows 0..2 are read), with a gain a and an offset b (float64 state, 1 and 0
 * at the start).  Each of the 14 values is rounded once to float32 for the per-pixel arithmetic.  Float32 per sample, every operation
 * individually rounded in the order written (no FMA contraction), plain divisions:
 *   intensity   grey = ((r + g) + b) * (1/3) of the frames (the float32 quotient 1.0f / 3.0f); I_i, I_j the grey planes.
 *   geometry    for pixel (u, v) of frame i: candidate, px, py, P, front, x, y, inside, x0, x1, y0, y1, wx, wy, the taps t00 .. t11 of
 *               depth_j, their validity and s exactly as colvo_consistency_filter's "neighbour" (K_i, K_j per frame); the sample is
 *               VISIBLE iff candidate, front, inside and taps valid.  c00 .. c11 are the same four positions of I_j and
 *               c = (((c00 * (1 - wx)) + (c01 * wx)) * (1 - wy)) + (((c10 * (1 - wx)) + (c11 * wx)) * wy).
 *   gradients   sx = ((t01 - t00) * (1 - wy)) + ((t11 - t10) * wy), sy = ((t10 - t00) * (1 - wx)) + ((t11 - t01) * wx); cx, cy likewise
 *               from c00 .. c11.  iz = 1 / P_z.  G(gx, gy): A = gx * fx_j, B = gy * fy_j,
 *                 G = (A * iz, B * iz, -((((A * P_x) + (B * P_y)) * iz) * iz)).
 *               P x g = ((P_y * g_z) - (P_z * g_y), (P_z * g_x) - (P_x * g_z), (P_x * g_y) - (P_y * g_x)).
 *               The update is a left perturbation T <- exp(xi) T, xi = (upsilon, omega): a scalar with P-gradient g has the pose row
 *               [g, P x g].
 *   geometric   den = P_z + s, rel = (P_z - s) / den, k = 2 / (den * den), G = G(sx, sy),
 *               g_r = (-(k * (P_z * G_x)), -(k * (P_z * G_y)), k * (s - (P_z * G_z)));  with w_g = 1.0f / sigma_geo:
 *               e_g = rel * w_g, J_g = [g_r * w_g, (P x g_r) * w_g, 0, 0].  Used iff visible and |rel| < gate_geo.
 *   photometric r_I = ((a * c) + b) - I_i[v][u], G = G(cx, cy), h = a * G;  with w_p = 1.0f / sigma_photo:
 *               e_p = r_I * w_p, J_p = [h * w_p, (P x h) * w_p, c * w_p, 1 * w_p].  Used iff visible and |r_I| < gate_photo.
 *   sums        per edge, float64: the 36 upper-triangle entries of sum J^T J (row-major: (0,0) .. (0,7), (1,1) ..) and the 8 of
 *               sum J^T e over the used samples of the enabled terms; C_g = sum over the visible samples of min(e_g^2, cap_g),
 *               cap_g = the square of the float32 product gate_geo * w_g, and C_p likewise; the integer counts n_visible, n_geo,
 *               n_photo.  A disabled term adds nothing (its count and C are 0).  Rows and residuals are float32, so every product
 *               is exact in float64; the order of the float64 additions is fixed by the kernels (per thread over its samples, a
 *               fixed tree over the workgroup, the workgroups' rows in a fixed order): identical bits on every call and stream.
 *   solve       float64, one thread per edge: the unknowns are the 6 pose entries, and a, b as well iff the photometric term and
 *               the brightness are enabled; H + damping * diag(H), Cholesky, delta = -H^-1 sum J^T e; T <- exp(delta_1..6) T by the
 *               closed form (its series below |omega|^2 = 1e-8), a += delta_7, b += delta_8.  An edge FREEZES -- initial T, a, b,
 *               for the rest of the call -- with status 1 if n_visible < min_samples and status 2 at a pivot that is not positive.
 *   loop        `iterations` times sums and solve, then the sums of the final state.  With F = (C_g + C_p) / n_visible, an edge
 *               whose F_final > F_initial is REVERTED to its initial state, status 3.  history [E][iterations + 1][5] float64 holds
 *               n_visible, n_geo, C_g, n_photo, C_p of every evaluation.  status 0: refined.  status 4: an edge with i == j or an
 *               index outside [0, N) -- the edge list is on the device, so the call cannot refuse it; the kernels read nothing
 *               through it, its history is 0 and its outputs are its inputs.
 * terms: bit 0 geometric, bit 1 photometric, bit 2 brightness (a, b unknowns); at least one of bits 0 and 1.
 * colvo_refine_accumulate: the sums of one evaluation at the states given (gain / offset NULL: 1 and 0): out_sums [E][48] float64 (the
 * 36, the 8, C_g, C_p, two zeros), out_counts [E][4] int32 (n_visible, n_geo, n_photo, 0).
 * colvo_refine_edges: the whole loop; out_T [E][4][4] (last row 0 0 0 1), out_gain, out_offset [E] float64, status [E] int32.  out_T
 * must not alias T_init.  No read-back and no host synchronisation.
 * workspace: colvo_refine_workspace_bytes(E, N, H, W, iterations) bytes, 16-byte aligned, written by the call (the per-workgroup rows,
 * the grey planes, the float32 states); 0 for what the calls refuse.  `iterations` is range-checked (0 .. 64) and otherwise reserved:
 * the size does not depend on it today (colvo_refine_accumulate's workspace is the same size).
 * Limits: E <= 65535, N <= 65535, H*W < 2^30, 1 <= iterations <= 64, sigma_geo, sigma_photo, gate_geo, gate_photo and max_depth
 * finite and positive, damping >= 0 and finite, min_samples >= 1. */
size_t colvo_refine_workspace_bytes(int E, int N, int H, int W, int iterations);
int colvo_refine_accumulate(const float* depths, const float* frames, const float* K, int N, int H, int W, const int32_t* edges, int E,
                            const double* T, const double* gain, const double* offset, float sigma_geo, float sigma_photo,
                            float gate_geo, float gate_photo, int terms, float max_depth, void* workspace, double* out_sums,
                            int32_t* out_counts, colvo_stream_t stream);
int colvo_refine_edges(const float* depths, const float* frames, const float* K, int N, int H, int W, const int32_t* edges, int E,
                       const double* T_init, int iterations, float sigma_geo, float sigma_photo, float gate_geo, float gate_photo,
                       double damping, int min_samples, int terms, float max_depth, void* workspace, double* out_T, double* out_gain,
                       double* out_offset, double* history, int32_t* status, colvo_stream_t stream);

/* ------------------------------------------------------------------------------------------- *
 * SURVEY.md §6  evaluation: depth error measures with per-image median scaling. *
 * ------------------------------------------------------------------------------------------- */
/* pred, gt [N,1,H,W] fp32; mask [N,1,H,W] uint8 or NULL.  A pixel is valid iff min_depth < gt < max_depth and mask != 0.
 * Per image: s = med(gt) / med(pred) over the valid pixels (exact lower medians, rank (n-1)/2; s = 1 when median_scaling is 0),
 * p = clamp(s * pred, min_depth, max_depth), and per_image[n][0..6] = abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 over the valid
 * pixels; scale[n] = s, n_valid[n] = valid pixel count.  An image without a valid pixel gets NaN metrics and scale, n_valid 0.
 * Deterministic (integer atomics only, fixed-order float reductions).  workspace: colvo_depth_metrics_workspace_bytes(N,H,W)
 * bytes, 16-byte aligned (0 for a shape the call refuses).  N <= 65535, H*W < 2^30. */
size_t colvo_depth_metrics_workspace_bytes(int N, int H, int W);
int colvo_depth_metrics(const float* pred, const float* gt, const uint8_t* mask, int N, int H, int W, float min_depth,
                        float max_depth, int median_scaling, void* workspace, double* per_image, float* scale,
                        int32_t* n_valid, colvo_stream_t stream);

/* ------------------------------------------------------------------------------------------- *
 * SURVEY.md §6  evaluation of the reconstruction: exact truncated nearest neighbours between two  *
 * point clouds (NumPy replica tests/cloud_ref.py).                               *
 * ------------------------------------------------------------------------------------------- */
/* query Q [N,3], ref P [M,3] float32, contiguous; max_dist > 0.  Pinned arithmetic: float32, every operation individually rounded
 * (no FMA contraction).
 *   valid     a point is valid iff its three coordinates are finite.  Invalid points take no part on either side and are counted.
 *   d2(q,p)   ((dx*dx + dy*dy) + dz*dz) with dx = qx - px, dy = qy - py, dz = qz - pz.
 *   md2       float32(max_dist) * float32(max_dist), rounded once.
 *   reach     p is within reach of q iff d2(q,p) < md2 (strict).
 *   dist2[q]  the minimum of d2 over the valid p within reach; nearest[q] the smallest original index p attaining it (the minimum
 *             of the 64-bit keys (bits(d2) << 32) | p).  No point within reach, or q invalid: dist2[q] = md2, nearest[q] = -1.
 *   dist[q]   sqrtf(dist2[q]), correctly rounded.
 *   stats     device uint64[12], exact integers over the query cloud:
 *               [0] n_valid    valid queries            [1] n_reached  valid queries with a point within reach
 *               [2..9]         for threshold k < n_thresholds the valid queries with dist2 < float32(tau_k) * float32(tau_k); 0 beyond
 *               [10]           sum over the valid queries of quantum(dist) = uint32(rint(dist * s)), s = float32(2^20) / float32(max_dist)
 *                              (one IEEE division, the product rounded to float32, ties to even); the mean truncated distance is
 *                              double(sum) / (double(s) * n_valid).  With N < 2^30 the sum stays below 2^51.
 *               [11]           reference records examined, over all valid queries (a cost figure: it depends on the grid, not on
 *                              the schedule).
 * Every output bit follows from the inputs alone: the minimum does not depend on the order, the sums are integers; not on the
 * schedule, the stream or the order in which atomics land.
 * colvo_cloud_index_build sorts the valid reference points by the cell of a uniform grid over their bounding box (bounds, histogram,
 * exclusive scan, scatter of 16-byte records x, y, z, original index) and writes origin, edge and dims into a device header at the
 * head of the workspace: colvo_cloud_query reads them there, no read-back lies between the two.  The cell edge is
 * max(max_dist * (1 + 2^-10), largest extent / 126), at most 128 cells per axis and 2^21 in all: the grid never outgrows the workspace,
 * a wide box gets larger cells (DESIGN.md §3.6h has the argument that the 27 cells around a query's hold everything within reach
 * although the cell index is computed in float32).  A box whose extent or cell edge is not finite is searched as one cell.
 * colvo_cloud_query: the same max_dist as the build's.  thresholds: HOST array of n_thresholds <= 8 values, finite, positive,
 * non-descending, each <= max_dist (as float32).  It clears and writes the counter lines of the workspace: one query at a time per
 * workspace.  dist, dist2 [N] float32, nearest [N] int32.
 * colvo_cloud_transform: out[i][a] = ((s * ((r_a0 * x + r_a1 * y) + r_a2 * z)) + t_a), pinned as above; Rts: HOST array of 13 floats,
 * R row-major, t, s; out may be the input.
 * Limits: N, M < 2^30 (0 is legal: an empty side launches nothing that indexes; the pointers of an empty cloud may be NULL);
 * max_dist finite and positive with a finite, positive float32 square; workspace 16-byte aligned,
 * colvo_cloud_workspace_bytes(N, M) bytes (0 for what the calls refuse; it does not depend on N today). */
size_t colvo_cloud_workspace_bytes(int N, int M);
int colvo_cloud_index_build(const float* ref, int M, float max_dist, void* workspace, colvo_stream_t stream);
int colvo_cloud_query(const float* query, int N, int M, float max_dist, const float* thresholds, int n_thresholds, void* workspace,
                      float* dist, float* dist2, int32_t* nearest, uint64_t* stats, colvo_stream_t stream);
int colvo_cloud_transform(const float* points, int N, const float* Rts, float* out, colvo_stream_t stream);

/* ------------------------------------------------------------------------------------------- *
 * Point-to-surface distances: exact truncated nearest point OF THE TRIANGLES of a mesh         *
 * (NumPy replica tests/surface_ref.py, brute force, no grid).                  *
 * ------------------------------------------------------------------------------------------- */
/* query Q [N,3] float32, vertices [V,3] float32, faces [F,3] int32 (rows of vertices), contiguous; max_dist > 0 as the cloud calls take
 * it; up to 8 thresholds as colvo_cloud_query takes them.
 *   validity  A face is DEAD exactly as for colvo_mesh_topology_*: an index outside [0, V) or a repeated index.  A live face with a
 *             coordinate that is not finite is SKIPPED.  Dead and skipped faces take no part and are counted.  A query with a
 *             coordinate that is not finite is invalid: it takes no part, is not counted as valid, and gets the sentinels below.
 *   arithmetic  float64 on coordinates widened from float32, every operation individually rounded in the order written (no FMA
 *             contraction), division and square root correctly rounded.  For query p and face (a, b, c), componentwise:
 *               ab = b - a, ac = c - a, bc = c - b, ca = a - c, pa = p - a, pb = p - b, pc = p - c;
 *               n_x = ab_y ac_z - ab_z ac_y, n_y = ab_z ac_x - ab_x ac_z, n_z = ab_x ac_y - ab_y ac_x;
 *               s = (n_x n_x + n_y n_y) + n_z n_z;   h = (n_x pa_x + n_y pa_y) + n_z pa_z;
 *               T(e, w) = (n_x c_x + n_y c_y) + n_z c_z with c_x = e_y w_z - e_z w_y, c_y = e_z w_x - e_x w_z, c_z = e_x w_y - e_y w_x.
 *             Up to four candidates (d2, point), tried in this order; only a strictly smaller d2 replaces the running one:
 *               plane   used iff s > 0 (and finite) and T(ab, pa) >= 0, T(bc, pb) >= 0, T(ca, pc) >= 0:
 *                       k = h / s, d2 = (h h) / s, point_j = p_j - n_j k.
 *               ab, bc, ca   segment (u, e, w) = (a, ab, pa), (b, bc, pb), (c, ca, pc): ee = (e_x e_x + e_y e_y) + e_z e_z,
 *                       we = (w_x e_x + w_y e_y) + w_z e_z, t = min(max(we / ee, 0), 1) if ee > 0 else 0, point_j = u_j + t e_j,
 *                       d_j = p_j - point_j, d2 = (d_x d_x + d_y d_y) + d_z d_z.
 *             Every candidate is a point of the triangle; a degenerate live face (collinear: s = 0 exactly, since equal products
 *             round alike; coincident vertices) degrades to its segments or a point and never yields a NaN.
 *   reach     md2 = double(max_dist)^2, exact.  A face is within reach iff its d2 < md2 (strict).  The winner is the least
 *             (d2, face index) in lexicographic order over the faces within reach.
 *   outputs   dist2 [N] float64: the winner's d2.  dist [N] float32: sqrt(dist2) in float64, rounded once to float32.  face [N] int32.
 *             closest [N][3] float32: the winning candidate's point, rounded once.  side [N] int8: the sign of h on the winning face
 *             (+1: the side the normal ab x ac points to -- free space, for extract_mesh's winding), 0 where h = 0 or s is not > 0.
 *             Nothing within reach, or an invalid query: md2, float32(max_dist), -1, the query itself (zeros for an invalid query), 0.
 *   stats     device uint64[19], exact integers.  [0..11] have colvo_cloud_query's meaning and order (the thresholds compare dist2
 *             with double(float32(tau_k))^2; the quanta are taken from the float32 dist with the same s; [11] counts the records and
 *             oversize faces examined).  [12] valid queries with side > 0, [13] with side < 0, [14] reached queries whose winning
 *             candidate is the plane one, [15] dead faces, [16] skipped faces, [17] (cell, face) pairs in the index, [18] faces on the
 *             oversize list.
 * Every output bit follows from the inputs alone, as for the cloud calls.
 * Index.  The grid of colvo_cloud_index_build over the bounding box of the vertices of the live, not skipped faces: cell edge
 * max(max_dist * (1 + 2^-10), largest extent / 126).  A face is entered into every cell of the box [c(min_a) .. c(max_a)] of its own
 * axis-aligned bounds (c: the clamped floor of the pinned float32 cell coordinate); DESIGN.md §3.6p has the argument that the 27 cells
 * around a query's cell then hold every face within reach.  A face whose box spans more than the tuning entry surface_span_limit (4)
 * cells on an axis goes onto an oversize list that every valid query examines whole.  Neither the list nor a face met in several
 * cells can change a bit: the minimum is over (d2, face).
 *   plan    bounds, grid, per-face counts, the ordered scan; counts (device int64[8]): pairs, oversize faces, dead, skipped,
 *           record_bytes, three zeros.  record_bytes is 4 (a record is a face index; the query gathers through faces and vertices)
 *           or 48 (the face's nine coordinates, its index and two words of padding, read as three 16-byte words), by the tuning
 *           entry surface_copy_records when the plan is made.  The caller reads counts back -- the one read-back -- and allocates
 *           records: pairs * record_bytes bytes, 16-byte aligned.
 *   fill    the faces sorted by cell into records.  pairs, record_bytes: the plan's.
 *   query   with the same vertices, faces, max_dist, scratch, records, pairs and record_bytes.  It clears and writes the counter lines of the
 *           scratch: one query at a time per scratch; any number of queries may follow one plan / fill.
 * scratch: colvo_surface_scratch_bytes(V, F) bytes, 16-byte aligned, carries the index's header, cell starts and oversize list from
 * each call to the next.
 * Limits, refused before any HIP call with a message that starts with the entry's name: 0 <= V, 0 <= F < 2^29, 0 <= N < 2^30,
 * 0 <= pairs < 2^30, record_bytes 4 or 48; max_dist and thresholds as the cloud calls refuse them.  Empty sides are legal and launch nothing that indexes
 * (their pointers may be NULL).  The size function returns 0 for what the calls refuse. */
size_t colvo_surface_scratch_bytes(int V, int F);
int colvo_surface_index_plan(const float* vertices, const int32_t* faces, int V, int F, float max_dist, void* scratch, int64_t* counts,
                             colvo_stream_t stream);
int colvo_surface_index_fill(const float* vertices, const int32_t* faces, int V, int F, void* scratch, int64_t pairs, int record_bytes,
                             void* records, colvo_stream_t stream);
int colvo_surface_query(const float* query, int N, const float* vertices, const int32_t* faces, int V, int F, float max_dist,
                        const float* thresholds, int n_thresholds, void* scratch, const void* records, int64_t pairs, int record_bytes,
                        double* dist2, float* dist, int32_t* face, float* closest, int8_t* side, uint64_t* stats, colvo_stream_t stream);

/* ------------------------------------------------------------------------------------------- *
 * Registration of two point clouds: point-to-plane (or point-to-point) ICP over the index of    *
 * colvo_cloud_index_build (NumPy replica tests/register_ref.py).               *
 * ------------------------------------------------------------------------------------------- */
/* source Q [N,3], target P [M,3] and the target's normals Nrm [M,3] (world frame; a zero normal means "none", as
 * colvo_cloud_normals delivers it; NULL with the point metric), float32, contiguous.  index: the workspace
 * colvo_cloud_index_build(P, M, max_dist, ...) wrote, with the same M and max_dist; it is only read.  state: 13 float64 values on the
 * device, R row-major, t, s, with x' = s R x + t.  pivot c: float32[3] on the device.
 *   per point  float32, every operation individually rounded (no FMA contraction), the state rounded to float32 first:
 *              x'_a = ((s * ((r_a0 * x + r_a1 * y) + r_a2 * z)) + t_a)   -- colvo_cloud_transform's formula;
 *              the nearest target point p by colvo_cloud_query's rule UNCHANGED (the same routine, csrc/cloud_grid.h): x' is valid
 *              iff its coordinates are finite, reach is strict (d2 < md2), the minimum is taken over the keys (bits(d2) << 32) | index,
 *              so ties go to the smallest original index; the grid walk, its clamps and the cell margin are the query's.
 *              e = x' - p, y = x' - c, per component.
 *   plane      with n = Nrm[index of p]: the pair is USED iff x' is valid and reached and (n_x*n_x + n_y*n_y) + n_z*n_z > 0 (NaN fails);
 *              r = (n_x*e_x + n_y*e_y) + n_z*e_z;  J = [n_x, n_y, n_z, (y x n)_x, (y x n)_y, (y x n)_z, (n_x*y_x + n_y*y_y) + n_z*y_z],
 *              y x n = ((y_y * n_z) - (y_z * n_y), (y_z * n_x) - (y_x * n_z), (y_x * n_y) - (y_y * n_x)).
 *   point      used iff valid and reached; three rows with r_a = e_a:
 *              (1,0,0, 0, y_z, -y_y, y_x), (0,1,0, -y_z, 0, y_x, y_y), (0,0,1, y_y, -y_x, 0, y_z).
 *   cost       of a valid x': plane, used: min(double(r)^2, double(md2)); point, used: double(d2); valid and not used: double(md2).
 *              C is their sum and F = C / n_valid the call's own measure.
 *   sums       float64: the 28 upper-triangle entries of sum J^T J (row-major: (0,0) .. (0,6), (1,1) ..), the 7 of sum J^T r, C, and
 *              sum r^2 over the used rows -- 37 values -- and the integers n_valid, n_reached, n_used.  Rows and residuals are
 *              float32, so every product is exact in float64; every term enters by one rounded addition, in an order fixed by the
 *              kernels and a function of N alone (per thread over its 4 points, a fixed reduction over the wave and the workgroup, the
 *              workgroups' rows in a fixed order; no floating-point atomics): identical bits on every call and stream.
 *   step       float64, one thread: the unknowns are (v, omega) and, in mode sim3, sigma -- 6 or 7; H + damping * diag(H), Cholesky,
 *              delta = -H^-1 sum J^T r; about the pivot: R <- Exp(omega) R, t <- e^sigma Exp(omega) (t - c) + c + v, s <- e^sigma s,
 *              Exp by the closed form (Rodrigues; its series below |omega|^2 = 1e-8).  In mode se3 sigma = 0 and s is not touched.
 *   loop       `iterations` times sums and step, then the sums of the final state.  history [iterations + 1][5] float64 holds
 *              n_valid, n_reached, n_used, C, sum r^2 of every evaluation.  The state FREEZES -- it is the initial one, to the bit, for
 *              the rest of the call -- with status 1 (too few) if n_used < min_pairs at an evaluation a step follows, and with
 *              status 2 (not positive definite) at a pivot of the Cholesky factor that is not positive.  A call whose F_final >
 *              F_initial is REVERTED to its initial state, to the bit, status 3.  Status 0: registered.  normal_matrix [7][7]: the
 *              undamped sum J^T J of the final evaluation, symmetric -- a surface with a free motion (a perfect cylinder) shows there
 *              as a vanishing pivot, and gives status 2 where the pivot is exactly zero; a nearly singular problem may step far and
 *              is caught by the revert.  There is no convergence test and no early exit: both would need a read-back.
 * mode: 0 se3, 1 sim3.  metric: 0 plane, 1 point.
 * colvo_register_accumulate: the sums of one evaluation at the state given: out_sums [40] float64 (the 37 and three zeros),
 * out_counts [4] int64 (n_valid, n_reached, n_used, 0).
 * colvo_register_clouds: the whole loop; out_state [13] float64 (it must not alias state_init), status [1] int32.  No read-back and no
 * host synchronisation.
 * workspace: colvo_register_scratch_bytes(N) bytes, 16-byte aligned, written by the call (one row of 40 doubles per 1024 source points,
 * the float32 state); 0 for an N the calls refuse.  The index is not written: several registrations may share one.
 * Whatever the index's header, its cell starts, its records or the normals hold, no address leaves its array: the cell counts and
 * dims are clamped as the query clamps them, record positions to [0, M), and P and Nrm are read only at a record's index in [0, M).
 * Limits: N, M < 2^30 (0 is legal: an empty side launches nothing that indexes; the pointers of an empty cloud may be NULL);
 * max_dist as colvo_cloud_index_build takes it; 1 <= iterations <= 64; damping finite and >= 0; min_pairs >= 1; workspace and
 * index 16-byte aligned.  Everything is refused before any HIP call with a message that starts `colvo_register_`. */
size_t colvo_register_scratch_bytes(int N);
int colvo_register_accumulate(const float* source, int N, const float* target, const float* normals, int M, float max_dist,
                              const void* index, const double* state, const float* pivot, int metric, void* workspace,
                              double* out_sums, int64_t* out_counts, colvo_stream_t stream);
int colvo_register_clouds(const float* source, int N, const float* target, const float* normals, int M, float max_dist,
                          const void* index, const double* state_init, const float* pivot, int mode, int metric, int iterations,
                          double damping, int min_pairs, void* workspace, double* out_state, double* history, int32_t* status,
                          double* normal_matrix, colvo_stream_t stream);

/* ------------------------------------------------------------------------------------------- *
 * SURVEY.md §8f-4  frames as a decoder delivers them -> the path's input format.                *
 *   (README.md:13 dataset; spec: resize_frames_u8)                                              *
 * ------------------------------------------------------------------------------------------- */
/* frames [B,h,w,3] uint8 interleaved RGB (device) -> out [B,3,H,W] fp32 in [0,1]: bilinear resize with half-pixel
 * centres (source index = (h/H)*(y+0.5)-0.5 clamped at 0), channel de-interleave and /255 in one pass. */
int colvo_frames_u8_to_f32(const uint8_t* frames, int B, int h, int w, int H, int W, float* out,
                           colvo_stream_t stream);

/* The same pass with a per-frame augmentation folded in: crop / mirror / resize, a 3x4 colour map, clamp and
 * gamma, one launch, the source read once.  `params` (device, 16-byte aligned) holds one ColvoAugRow per frame.  Output pixel
 * (y, x) of frame i reads the source at
 *     fy = fma(sy, y + 0.5, oy - 0.5),   fx = fma(sx, x' + 0.5, ox - 0.5),   x' = flip ? W-1-x : x        (float32, one rounding each)
 * clamped below at 0, taps y0 = min(floor(fy), h-1), y1 = min(y0+1, h-1) (likewise in x) and the bilinear weights of
 * colvo_frames_u8_to_f32; then, on the resized r, g, b in [0,1],
 *     out_c = clamp(A[c][0]*r + A[c][1]*g + A[c][2]*b + A[c][3], 0, 1),   out_c = out_c ** gamma  when gamma != 1.
 * With oy = ox = 0, sy = h/H, sx = w/W, flip = 0, A = [I | 0], gamma = 1 the result equals colvo_frames_u8_to_f32's bit for bit.
 * The kernel is memory-safe for ANY bit pattern in the table (every tap index is clamped into the frame, a NaN coordinate reads
 * pixel 0; the output is finite and in [0,1] whatever the row holds); whether a row makes sense is the caller's business.
 * Same limits as colvo_frames_u8_to_f32. */
typedef struct ColvoAugRow {
    float oy, ox;      /* crop origin in native edge coordinates (pixel i covers [i, i+1)) */
    float sy, sx;      /* source step per output pixel: crop height / H, crop width / W */
    int32_t flip;      /* != 0: mirrored left-right (the reads are reversed, the stores stay in order) */
    float gamma;       /* exponent applied after the clamp; exactly 1 skips it */
    float A[12];       /* row-major 3x4 colour matrix: out_c = A[4c..4c+2] . (r, g, b) + A[4c+3] */
    float pad_[2];     /* 80 bytes: rows of a 16-byte aligned table stay 16-byte aligned */
} ColvoAugRow;
int colvo_frames_u8_augment(const uint8_t* frames, int n, int h, int w, int H, int W, const ColvoAugRow* params, float* out,
                            colvo_stream_t stream);

/* Host side of the same row (no GPU work): n raw frames -- `.npy` files holding [h,w,3] uint8 arrays in C order -- read into
 * dst[n][h][w][3] (the caller's staging buffer, normally pinned) by up to `nthreads` threads; every header is checked against
 * (h, w).  Returns non-zero with the first failing file in colvo_last_error(). */
int colvo_read_npy_u8_frames(const char* const* paths, int n, int h, int w, uint8_t* dst, int nthreads);

/* ------------------------------------------------------------------------------------------- *
 * Command lists: ONE call enqueues a recorded sequence of the entry points above (a network's  *
 * forward or backward) on a main and a side stream -- the host's per-launch cost, not the GPU, *
 * bounded the batch-8 step when every layer was a separate host call.  The same encoding is    *
 * the only way the Python ops reach these entry points: an op outside a recording is ONE       *
 * command issued by colvo_run_command.                                                         *
 * ------------------------------------------------------------------------------------------- */
enum {
    COLVO_CMD_CONV_FWD = 1,      /* p: x0 x1 w_fwd bias y; chain form (i[0] = 3, colvo_pose_front_plan): p: x - w1 b1 y1 w2 b2 y2 w3 b3 y3;
                                    i: 3 and the three output channel counts (16 32 64); desc: the first layer's;
                                    whole-K form (i[0] = -1, colvo_pose_tail_plan): p as in the plain form with x1 NULL */
    COLVO_CMD_CONV_DGRAD,        /* i: src accumulate; p: dy w_bwd relu_mask dx; whole-K form (i[2] = 1, colvo_pose_tail_plan
                                    direction 1): i: 0 0 1, p as in the plain form */
    COLVO_CMD_CONV_WGRAD,        /* p: x0 x1 dy dw db scratch; i: scratch_bytes slabs_only arena_is_zero (scratch != NULL:
                                    colvo_conv_wgrad_det, or with slabs_only colvo_conv_wgrad_slabs; scratch == NULL and arena_is_zero:
                                    colvo_conv_wgrad_clean -- the host patches that integer before each replay) */
    COLVO_CMD_PACK_NCHW,         /* i: dtype c0 c1 c2 c3 nsrc B H W Cpad; p: src0..src3 dst */
    COLVO_CMD_UNPACK_NHWC_GRAD,  /* i: dtype B H W Cpad c_begin c_count accumulate; p: dsrc dst */
    COLVO_CMD_DEPTH_HEAD_FWD,    /* i: dtype B H W C; f: min max; p: x w bias depth */
    COLVO_CMD_DEPTH_HEAD_BWD,    /* i: dtype B H W C; f: min max; p: x w depth d_depth scratch dx dw db */
    COLVO_CMD_DEPTH_HEAD_WGRAD,  /* i: dtype B H W C scratch_bytes; p: x dpre dw db scratch (non-NULL: the _det form) */
    COLVO_CMD_POSE_HEAD_FWD,     /* i: dtype B HW C; f: pose_scale lcc_scale; p: x w bias out */
    COLVO_CMD_POSE_HEAD_BWD,     /* i: dtype B HW C det; f: pose_scale lcc_scale; p: x w d_pose d_a d_b dx dw db scale_a scale_b */
    COLVO_CMD_FORK,              /* side stream waits for the main stream's work so far */
    COLVO_CMD_JOIN,              /* main stream waits for the side stream's work so far */
    COLVO_CMD_DEPTH_HEAD_BWD_PARTS, /* i: dtype B H W C; f: min max; p: x w depth g_first g_second g_raw scale_a scale_b scratch dx g_raw_second */
    COLVO_CMD_CONV_DGRAD_BOTH,    /* p: dy w_bwd relu_mask0 relu_mask1 dx0 dx1 */
    COLVO_CMD_WGRAD_REDUCE_GROUP, /* p: sets (HOST pointer to ColvoWgradSlabs[n], alive as long as the list); i: n */
    COLVO_CMD_CONV_DGRAD_PLANES,  /* p: dy w_master dst; i: c_begin c_count accumulate; chain form (p[3] != NULL, colvo_pose_front_plan
                                   * direction 1): p: g1 w_master dst g3 w_bwd3 w_bwd2 act2 act1 g2 g1 (g2, g1: written); desc: conv1's */
    COLVO_CMD_CONV_BWD_FUSED,     /* p: dy w_bwd x dx dw db head_dpre head_w head_partials scratch; i: relu_mask scratch_bytes
                                   * (p[9] scratch != NULL: colvo_conv_bwd_fused_det; with p[4] dw == NULL the rows stay in the scratch) */
    COLVO_CMD_HEAD_WGRAD_REDUCE,  /* p: partials dw db; i: rows */
    COLVO_CMD_CONV_HEAD_FUSED,    /* p: x w_fwd bias head_w head_b y depth pose_in; f: min_depth max_depth */
    COLVO_CMD_PACK_STEM_POSE,     /* p: frames stem pose_in; i: B2 H W; stem form (p[3] != NULL, colvo_stem_plan): p: frames stem pose_in
                                   * w1 b1 y1 w2 b2 y2 (enc1a's and enc1b's w_fwd, bias and output; all three tensors and both
                                   * outputs are written); desc: enc1a's */
    COLVO_CMD_HEAD_WGRAD_MFMA,    /* p: y dpre partials; i: B H W */
    COLVO_CMD_SIDE_SYNC           /* (side command) the side stream in use waits for everything enqueued so far on every other side
                                    stream: what follows reads what several FORKed commands wrote */
};

typedef struct ColvoCmd {
    int32_t op;                  /* COLVO_CMD_* */
    int32_t stream;              /* 0 = main, 1 = side */
    ColvoConvDesc desc;          /* conv commands */
    const void* p[12];           /* pointer arguments in the order listed above (device memory, caller-owned) */
    int32_t i[12];               /* integer arguments in the order listed above */
    float f[4];
} ColvoCmd;

/* Enqueue cmds[0..n) in order; side_stream may be NULL when no command uses it.  FORK/JOIN use a small ring of
 * library-owned events (host objects; still no device allocation).  Stops at the first failing command. */
int colvo_run_commands(const ColvoCmd* cmds, int n, colvo_stream_t main_stream, colvo_stream_t side_stream);
/* One command on `stream`: the same call of its entry point that colvo_run_commands makes, and nothing else (no events, no
 * capture handling: under stream capture its launches are plain nodes on the capturing stream).  Returns the entry point's
 * code, with its own colvo_last_error() message.  cmd->stream must be 0; FORK, JOIN and SIDE_SYNC are rejected. */
int colvo_run_command(const ColvoCmd* cmd, colvo_stream_t stream);
/* colvo_run_commands spreads consecutive FORKs over the caller's side stream and up to n library-owned ones (default 1,
 * COLVO_SIDE_STREAMS - 1).  A process that drives MORE streams of its own beside the main and the side stream -- RCCL's
 * communicator stream in data-parallel training -- must set n = 0: with four or more hardware queues active and cross-queue
 * dependencies between them the step measured 5.2 ms instead of 1.7. */
int colvo_set_aux_side_streams(int n);
/* hipGraph form.  While main_stream is being CAPTURED (hipStreamBeginCapture) colvo_run_commands turns the list into graph nodes
 * with explicit dependencies on that one stream (hipStreamUpdateCaptureDependencies): the main-stream commands as one chain, the
 * side-stream commands as a second chain -- side_stream itself is not used and no event is recorded.  policy: 0 = one branch (side
 * commands captured in list order on the main chain), 1 = one cross-branch edge per FORK (the eager schedule node for node),
 * 2 (default) = side commands flushed `group` at a time (default 2), each segment depending on the main chain as captured at the
 * flush and on the previous segment, 3 = as 2 with the segments alternating between two side chains.  Every call ends joined.
 * Nodes are created so that the main chain stays the FIRST child of every fork point: ROCm's executor keeps the first child on the
 * parent's stream and opens a stream per further child. */
int colvo_set_capture_policy(int policy, int group);
/* Carry mode of the hipGraph form (default off: every captured colvo_run_commands call ends joined).  on: a list that ends without
 * a JOIN leaves the side chain OPEN -- the next captured call continues it, exactly as the eager schedule's deferred join leaves the
 * weight gradients of one network running beside the next network's backward pass -- and side commands still pending at the end of
 * a call are held back (as copies) until the next call has captured its first main-chain node: created earlier they would become the
 * first child of the main chain's last node and push the main chain onto a new stream (see colvo_set_capture_policy).  The caller
 * must then call colvo_capture_join(stream) wherever the eager schedule joins its side stream (before the optimizer, before a
 * collective that reads the gradients, before the capture ends). */
int colvo_set_capture_carry(int on);
/* The next node captured on `stream` depends on the main chain AND on everything the open side chain(s) hold, pending commands
 * included.  No-op when `stream` is not being captured or nothing is open. */
int colvo_capture_join(colvo_stream_t stream);
/* Structure of what has been built (tests, tools): out[0..7] describe the graph under construction on `stream` when it is being
 * captured -- nodes, edges, root nodes, leaf nodes, nodes with >= 2 children (forks), nodes with >= 2 parents (joins), largest
 * out-degree, largest in-degree -- and are -1 otherwise; out[8..15] count what colvo_run_commands has captured since
 * colvo_graph_stats_reset(): calls, main-chain commands, side-chain commands, side segments, joins, calls that started with
 * carried-over commands, the largest dependency set a call started from, commands pending right now.  n >= COLVO_GRAPH_STATS_N. */
#define COLVO_GRAPH_STATS_N 16
int colvo_graph_stats(colvo_stream_t stream, long long* out, int n);
int colvo_graph_stats_reset(void);
/* Return the library to its pre-capture state: what the last capture left in its bookkeeping (handles of graph nodes that die with
 * the graph, copies of held-back commands, the fork point), capture policy / group / carry mode back to their defaults, the calling
 * thread's launch tap disarmed.  Call it when a captured graph is destroyed or a capture failed (coivo_amd.graph.GraphedTrainStep.close);
 * fails with hipErrorStreamCaptureUnsupported-style code and changes nothing while `stream` (may be NULL) is being captured. */
int colvo_capture_reset(colvo_stream_t stream);

/* Dispatch thresholds (coivo_amd/csrc/tuning.h: ONE table, defaults measured on MI355X; production reads no environment
 * variable).  Developer / test hooks: set or read an entry by name ("quad_min_wgs", "wgrad_atomic_mb", ...); with COLVO_DEV=1 in
 * the environment at load time every entry can also be overridden by COLVO_<UPPER-CASE NAME>. */
/* Which kernel form the dispatchers chose, counted per process since the last reset (developer / test hook: which form ran is
 * invisible in a result; a test that means to cover one asserts that it ran).  Every leaf of the forward, input-gradient and
 * weight-gradient dispatch trees has a counter (k_conv_rt, k_conv_q, k_conv_up2 16- / 32-wide, k_dgrad_s2 and its two-chunk ring,
 * k_dgrad_up2, the one-tile kernel, its two-chunk ring and 512-thread form, the weights-resident kernel stride 1 / 2, the weight
 * gradient's register-tiled, four-class, teams and one-team forms), so do the fused kernels (k_bwd16, k_fwd16_head,
 * k_dgrad_planes_s2_mfma), colvo_conv_dgrad_both's merged launch, and the attributes 32-channel k_conv_rt, 64-wide channel tile
 * of the one-tile and weights-resident kernels, full / halved
 * weight-gradient grid, 64-wide weight-gradient co tile, clean-arena store and image-sliced weight gradient.  One relaxed atomic per
 * launch; plan-only queries count nothing.  colvo_form_counts fills out[0..n) and returns the number of forms (at most 32);
 * colvo_form_name(id) names them (NULL beyond the last). */
int colvo_form_counts(long long* out, int n);
void colvo_form_counts_reset(void);
const char* colvo_form_name(int id);
int colvo_tune_set(const char* name, double value);
int colvo_tune_get(const char* name, double* value);

#ifdef __cplusplus
}
#endif
#endif /* COLVO_H_ */
