/* hvgan.h -- C ABI of libhvgan.so: hand-written gfx950 (MI355X) kernels for the HealthiVert-GAN
 * generator / discriminator train + inference hot path.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless named h_*; every tensor is NHWC, dense in W/H with an
 *     explicit channel stride `*_ld` (elements per pixel) and channel offset `*_coff` so a conv can read or
 *     write a channel slice of a wider (concat) buffer.  Elements are fp32; the activation / gradient tensors INSIDE
 *     a network may be stored as fp16 instead where an `*_f16` flag says so (precision HV_F16 only: their values
 *     are rounded to fp16 as MFMA operands anyway).  A (B,1,H,W) NCHW tensor is bit-identical in NHWC, so all
 *     image-level inputs/outputs of the reference API (always fp32) cross the boundary without a copy.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  No entry point allocates, frees or
 *     synchronises: the caller owns every buffer, including workspaces sized by the *_workspace_bytes calls,
 *     so every call is legal inside a hipGraph capture.
 *   - return value: 0 = ok; HV_ERR_* (negative) = rejected before launch; <= -1000 = -(hipError_t) - 1000.
 *     Nothing throws across the ABI.  The Python host (healthivert-gan_amd/lib.py) turns non-zero into
 *     RuntimeError; there is no CPU fallback.
 *   - `precision`: HV_F32 = exact fp32 MFMA (v_mfma_f32_16x16x4_f32; the |d| <= 1e-3 parity mode),
 *     HV_F16 = operands rounded to fp16 when staged into LDS, fp32 accumulate (v_mfma_f32_16x16x32_f16).
 *
 * Each entry point names the reference code it replaces (paths relative to the reference root).
 */
#ifndef HVGAN_H
#define HVGAN_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HV_OK 0
#define HV_ERR_ARG (-1)         /* null pointer / non-positive size / bad enum */
#define HV_ERR_UNSUPPORTED (-2) /* shape outside what the kernels are built for */
#define HV_ERR_WORKSPACE (-3)   /* workspace too small */

enum { HV_F32 = 0, HV_F16 = 1 };
enum { HV_ACT_NONE = 0, HV_ACT_ELU = 1, HV_ACT_RELU = 2, HV_ACT_LRELU = 3, HV_ACT_SIGMOID = 4, HV_ACT_CLAMP = 5 };
enum { HV_NORM_NONE = 0, HV_NORM_BATCH = 1, HV_NORM_INSTANCE = 2 };

int hv_version(void);
const char* hv_arch(void); /* "gfx950" */
/* which kernel family the calling thread's most recent hv_conv2d / hv_conv2d_wgrad launched (profiling labels):
 * 0 conv_igemm_kernel, 1 narrow_fwd_kernel, 2 conv_halo_kernel, 3 conv_halo2_kernel, 4 thin1_fwd_kernel, 5 head_gemm_kernel, 6 conv_s2t_kernel, 10 wgrad_kernel,
 * 11 wgrad_halo_kernel, 12 wgrad_tr_kernel, 13 wgrad_trd_kernel, 14 conv_px_kernel (one lane per pixel, 4x4x4 MFMA: the thin full-resolution layers) */
int hv_last_kernel_path(void);
/* name of that kernel instantiation as rocprofv3 prints it, e.g. "conv_halo2_kernel<8, 16, 128, 1, 4, 32, 1, 4, 4>" (the gather and weight-
 * gradient kernels are templated on _Float16, which rocprofv3 leaves mangled: _Z12wgrad_kernelIDF16_Li128E... = wgrad_kernel<_Float16, 128, ...>) */
const char* hv_last_kernel_name(void);
/* profiling: the calling thread's NEXT hv_conv2d or hv_conv2d_wgrad records these two hipEvent_t right around its kernel launch (for a weight
 * gradient: around the main kernel; the slab reduction that follows is a separate kernel); the pair is consumed by that call.  NULL, NULL cancels. */
int hv_set_kernel_timing(void* ev_start, void* ev_stop);
/* tuning (tests and A/B tools): which stride-2 data gradients take the fused-parity kernel (path 6): 0 none, 1 the 3x3 filters (default;
 * environment HV_S2T), 2 also the 4x4 filters.  Process-wide; returns the previous mode. */
int hv_set_s2t_mode(int mode);

/* ---------------------------------------------------------------- convolution (implicit GEMM on MFMA)
 * Replaces F.conv2d / F.conv_transpose2d as called by Conv2dBlock.forward (models/inpaint_networks.py:494-503),
 * NLayerDiscriminator (models/networks.py:575-602), Down/UpsampleBlock (models/UnetG_CT_mask.py:69-100), the
 * matching and pasting convolutions of ContextualAttention (models/inpaint_networks.py:348,379) and -- with
 * transposed=1 -- their autograd data-gradients.
 *
 *   y[n,ho,wo,co] (op)= act( alpha * ch_scale[co] * sum_{r,s,ci} x[n,hi,wi,ci] * w[co,(r,s),ci] + bias[co] )
 *   transposed=0: hi = ho*stride - pad + r*dil
 *   transposed=1: hi = (ho + pad - r*dil)/stride where divisible (gather form of conv_transpose2d / dgrad)
 *   in_shift=1 reads x through a fused nearest x2 upsample (physical index = logical >> 1).
 *   w is [Cout][KH*KW][Cin] ("OHWI"); w_bstride != 0 selects per-sample filters (contextual attention).
 */
typedef struct {
    const float* x; int B, H, W;      /* logical input size (after the fused upsample) */
    int in_shift; int x_ld, x_coff, Cin;
    const float* w; long long w_bstride;
    int Cout, KH, KW, stride, pad, dil, transposed;
    const float* bias;                /* [Cout] or NULL */
    const float* ch_scale;            /* [Cout] or NULL */
    long long ch_scale_bstride;
    float alpha; int act; int accumulate;   /* accumulate: 0 y = r; 1 y += r (after act); 2 y = act(r + y) */
    float* y; int Ho, Wo, y_ld, y_coff;
    int precision;
    const void* w_f16;                /* optional fp16 copy of w (same layout, from hv_weight_prep): enables the
                                         halo-tiled kernel for HV_F16, dilation 1, Cin % 16 == 0, shared filters */
    const void* w_f16_tiled;          /* optional: the same fp16 filters in MFMA-fragment order (hv_weight_prep's w_fwd_t / w_bwd_t, or
                                         hv_weight_tile_f16; needs w_f16 too).  The kernels that fetch filter rows straight into MFMA operand
                                         registers then read 1-KB contiguous pieces instead of 16 rows x 64 B that lie a whole filter row apart
                                         (and on one L2 channel): 256 -> 512 4x4 PatchGAN layer 93 -> 76 us.  NULL = plain rows */
    const float* mul_src; int mul_ld, mul_coff, mul_act;
                                      /* optional epilogue factor: r *= act'(m) with m = mul_src[pixel*mul_ld + mul_coff + channel] the OUTPUT
                                         of activation mul_act at the same pixel/channel, applied after act and before accumulate == 1.
                                         Used by data gradients to hand the producer layer its pre-activation gradient directly
                                         (the separate in-place multiply pass over the gradient disappears).  NULL = none */
    int x_f16, y_f16, mul_f16;        /* storage of x / y / mul_src: 0 = fp32 (pointers are float*), 1 = fp16 (the pointers address _Float16
                                         elements; *_ld / *_coff stay in elements).  fp16 storage needs precision == HV_F16 (operands are rounded
                                         to fp16 at staging anyway) and serves the tensors of a network that are only conv / norm operands;
                                         1-channel image tensors and the attention score matrices stay fp32 */
    void* workspace; size_t workspace_bytes;
                                      /* optional scratch (16-byte aligned) of hv_conv2d_workspace_bytes(d) bytes: enables the two-kernel path for
                                         Cout == 1 with many input channels (PatchGAN logits, data gradient of the 1-channel stem), which
                                         streams x once into a [pixel][tap] table and sums the taps afterwards.  NULL = other kernels */
    float* stats;                     /* optional: per-channel partial sums of the OUTPUT as stored (fp16-rounded, after act), written by the conv's own
                                         epilogue: stats[(part * Cout + c) * 2 + {0: sum, 1: sum of squares}] for part < hv_conv2d_stats_parts(d).
                                         Feeds hv_norm_desc.partials (BatchNorm statistics without a reduction pass over the tensor).  Only the
                                         kernels that hv_conv2d_stats_parts reports (> 0) write it; NULL = not wanted */
    const void* x1;                   /* optional ONE extra input channel at the convolution's own resolution, added before bias / activation:
                                         y += sum_taps x1[n][i + dh][j + dw] * w1[co * w1_row + tap * w1_tap] (zero padded like x).  With in_shift = 1 on x this
                                         is a convolution over the concatenation [nearest x2 up-sampling of x | x1] that is never materialised (the coarse
                                         generator's conv19 / conv20: models/inpaint_networks.py:97-106); w1 = channel Cin of the full fp32 forward table
                                         [Cout][taps][CinP] (w1_row = taps * CinP, w1_tap = CinP).  Forward 3x3 stride-1 only, filters-in-LDS kernel only:
                                         HV_ERR_UNSUPPORTED otherwise */
    int x1_f16, x1_ld, x1_coff;
    const float* w1; int w1_row, w1_tap;
    int pool2;                        /* 1: the output is stored 2x2 sum-pooled -- y, mul_src (and the accumulate operand) are (Ho/2) x (Wo/2) tensors and
                                         y[n][i][j][c] (+)= act'(mul_src[n][i][j][c]) * sum of the four fp16-rounded conv outputs at (2i + {0,1}, 2j + {0,1}):
                                         the data gradient of a convolution whose input was the nearest x2 up-sampling of a smaller tensor, without the
                                         full-resolution gradient in memory (replaces conv + hv_copy_channels mode 3 + the in-place act' pass).  Ho, Wo keep
                                         the convolution's own output size (even).  Served by the filters-in-LDS 3x3 kernel only: HV_ERR_UNSUPPORTED otherwise */
    const void* bn_x; int bn_x_ld, bn_x_coff;
    const float* bn_stats; int bn_groups;
    float* bstats;                    /* optional, data-gradient forms whose output y is the gradient at the OUTPUT of a batch normalisation (its act' applied through
                                         mul_src): the normalisation's backward sums out of this conv's epilogue.  bn_x = the normalisation's raw input (same pixels /
                                         channels / storage as y, its own ld / coff), bn_stats = its saved [bn_groups][2][Cout] mean / rstd (hv_norm_desc.stats; the
                                         batch's images fall into bn_groups equal groups), bstats[(part * Cout + c) * 2 + {0, 1}] = sum g, sum g * xhat over the part's
                                         pixels (g = the stored value of y, xhat = (bn_x - mean) * rstd), part < hv_conv2d_bstats_parts(d), parts of whole images in
                                         (group, image) order.  Feeds hv_norm_bwd_desc.partials: hv_norm_act_backward then skips its reduction pass over dy and x.
                                         hv_conv2d returns HV_ERR_UNSUPPORTED (and launches nothing) when the kernel of this shape has no such epilogue */
    const float* xn_stats; const float* xn_gamma; const float* xn_beta; int xn_groups, xn_act;
    void* xn_out; int xn_out_ld, xn_out_coff;
                                      /* optional, forward with Cout == 1 and `workspace` (the [pixel][tap] path of the PatchGAN logits layer) only: x is the RAW input of a
                                         normalisation + activation (models/networks.py:583-595) whose statistics hv_norm_act_forward (y == NULL: statistics only) left in
                                         xn_stats -- [xn_groups][2][Cin] mean / rstd, the batch's images falling into xn_groups equal groups (1 BatchNorm, 2 the fake | real
                                         pass, B InstanceNorm).  The operand is xn_act(((x - mean) * rstd) * gamma + beta) rounded to fp16 -- hv_norm_act_forward's
                                         arithmetic, bit for bit -- made where x is staged (xn_gamma / xn_beta NULL = 1 / 0); xn_out != NULL: the normalised map is also
                                         stored there (fp16 [pixel][xn_out_ld], the write a separate normalisation pass would have made; its read of x and this
                                         convolution's read of the result are what the fusion saves).  hv_conv2d returns HV_ERR_UNSUPPORTED (and launches nothing) when the
                                         kernel of this shape has no such staging */
} hv_conv_desc;
int hv_conv2d(const hv_conv_desc* d, void* stream);
size_t hv_conv2d_bstats_parts(const hv_conv_desc* d);      /* parts of hv_conv_desc.bstats this call would write (0: its kernel has no such epilogue) */
size_t hv_conv2d_workspace_bytes(const hv_conv_desc* d);   /* 0 when no kernel for this shape wants scratch */
size_t hv_conv2d_stats_parts(const hv_conv_desc* d);       /* parts of hv_conv_desc.stats this call would write (0: its kernel has no statistics epilogue) */
int hv_last_weight_tables(void);                           /* which prepared tables the hv_conv2d call this thread made last read: 1 = fp32 (w, w1), 2 = fp16 rows
                                                              (w_f16), 4 = fp16 in MFMA-fragment order (w_f16_tiled); may over-report.  A caller that collects
                                                              this per layer can pass NULL for the unread tables of hv_wprep_layer (hv_weight_prep2) */
int hv_conv2d_supported(const hv_conv_desc* d);            /* 1 when hv_conv2d would serve d.  Only the forms without a generic fallback can be refused for their
                                                              shape -- x1, pool2, stats (hv_conv2d then returns HV_ERR_UNSUPPORTED and launches nothing) -- so a caller
                                                              asks before it drops the materialised alternative.  Runs the dispatch itself without launching */

/* One slab fold: dw[i] (+)= sum_k slabs[k * numel + i] in a fixed order (groups by slab count, then a tree: deterministic), dbias likewise from bias_slabs
 * [nslabs][Cout].  nslabs == 0: the call wrote dw directly (nothing to fold). */
typedef struct {
    const float* slabs; float* dw; long long numel; int nslabs; int accumulate;
    const float* bias_slabs; float* dbias; int Cout; int dbias_accumulate;
} hv_wgrad_fold;

/* Weight gradient: dw[co][(r,s)][ci] = sum_{n,ho,wo} g[n,ho,wo,co] * x[n, ho*stride-pad+r*dil, ..., ci].
 * (autograd of the convs above; for a transposed conv swap the roles of x and g on the caller side).
 * Split over pixel chunks; partial slabs go to `workspace` and are summed in a fixed order (deterministic). */
typedef struct {
    const float* x; int B, H, W; int in_shift; int x_ld, x_coff, Cin;
    const float* g; int Ho, Wo, g_ld, g_coff, Cout;
    int KH, KW, stride, pad, dil;
    float* dw; int accumulate;
    float* workspace; size_t workspace_bytes;
    int precision;
    int x_f16, g_f16;                     /* storage of x / g as in hv_conv_desc (both 0 or both 1) */
    float* dbias; int dbias_accumulate;   /* optional: dbias[co] (+)= sum over pixels of g[.., co] (bias gradient of the same conv), folded
                                             into the kernel that already streams g; NULL = not computed */
    hv_wgrad_fold* pending;               /* optional (HOST pointer): the split-K slabs are LEFT in `workspace` -- which then has to stay untouched until their
                                             fold has run -- and *pending describes that fold; the call launches no slab reduction.  The caller hands the record to
                                             the NEXT weight gradient of the same stream as `carry` (or to hv_wgrad_fold_now).  NULL = fold here */
    const hv_wgrad_fold* carry;           /* optional (HOST pointer): the PREVIOUS weight gradient's recorded fold (another dw, another workspace): it runs as extra
                                             workgroups of this call's main kernel where that kernel leaves room for them (the generators' 3x3 / 5x5 layers),
                                             else as a launch of its own; either way it is done when this call's work is.  Same sums bit for bit as a fold
                                             launched on its own.  One dependent ~5-us launch less per layer of a backward chain */
} hv_wgrad_desc;
int hv_wgrad_fold_now(const hv_wgrad_fold* fold /* host */, void* stream);     /* the fold of a `pending` record as a launch of its own (the last of a chain) */
size_t hv_conv2d_wgrad_workspace_bytes(const hv_wgrad_desc* d);
int hv_conv2d_wgrad(const hv_wgrad_desc* d, void* stream);

/* ---------------------------------------------------------------- weight preparation / spectral norm
 * Batched over layers: one workgroup per layer.  Replaces torch.nn.utils.spectral_norm's forward pre-hook
 * (used at models/inpaint_networks.py:449-450,491-492): optional power iteration (in-place u,v), sigma,
 * W/sigma, written directly in the kernels' OHWI layouts (forward: [Cout][taps][CinP]; data-gradient:
 * [CinP'][taps][Cout'] ...).  With sn=0 it is a pure layout transform (discriminator / U-Net weights). */
typedef struct {
    const float* w_orig;  /* [Cout][Cin][KH][KW] (torch layout); for conv_transpose [Cin][Cout][KH][KW] with transposed_src=1 */
    float* u; float* v;   /* [Cout], [Cin*KH*KW]; NULL when sn=0 */
    float* sigma;         /* [4] scratch: [0] = sigma out (1.0 when sn=0), [1] = <dWsn,Wsn> written by the backward */
    float* w_fwd;         /* [CoutF][taps][CinP]  rows >= Cout and channels >= Cin are zero; NULL = not wanted (hv_weight_prep2 only: every table is optional there) */
    float* w_bwd;         /* [CinB][taps][CoutP]  or NULL */
    void* w_fwd_h; void* w_bwd_h;   /* optional fp16 copies of w_fwd / w_bwd (same layouts) or NULL */
    void* w_fwd_t; void* w_bwd_t;   /* optional fp16 copies in MFMA-fragment order (hv_conv_desc.w_f16_tiled; layout at hv_weight_tile_f16) or NULL;
                                       hv_weight_tiled_elems(CoutF, taps, CinP) / (CinB, taps, CoutP) halfs, zero-filled once by the caller */
    int Cout, Cin, taps, CinP, CoutF, CoutP, CinB;
    int sn, power_iter, transposed_src;
    void* w_fwd_t2; int K2;   /* optional: the first K2 (32 or 64) input channels of the forward table once more in MFMA-fragment order, as a table of its
                                 own ([CoutF][taps][K2]: hv_weight_tiled_elems(CoutF, taps, K2) halfs) -- the filters of hv_conv_desc.x1 layers; written by
                                 hv_weight_prep2 only */
} hv_wprep_layer;
int hv_weight_prep(const hv_wprep_layer* d_layers, int n_layers, long long max_numel, void* stream); /* d_layers: DEVICE array; max_numel = largest w_fwd+w_bwd element count of a layer */
/* The same tables with all six of a layer written from one read of its weights (32 x 32 filter x channel tiles through LDS, whole MFMA fragments per store).
 * any_sn: some layer has sn = 1 (otherwise the sigma kernel is not launched: sigma[0] must already hold 1.0); any_legacy: some layer is a conv_transpose
 * source (those take the element-wise kernels of hv_weight_prep). */
int hv_weight_prep2(const hv_wprep_layer* d_layers, int n_layers, long long max_numel, int any_sn, int any_legacy, void* stream);

/* MFMA-fragment order of an fp16 filter table w[rows][taps][K] (K = padded input channels; T = 32 when K % 32 == 0, 16 when K % 16 == 0, otherwise
 * there is no tiled form): element (row, tap, k) lives at half index
 *     (row / 16) * 16 * taps * K  +  ((tap * K + k) / T) * 16 * T  +  (((k % T) / (T/4)) * 16 + row % 16) * (T/4)  +  k % (T/4)
 * i.e. per 16-row block one contiguous 16 x T fragment per (tap, T-channel chunk), stored so that lane l of a wave reads bytes [l*T/2, (l+1)*T/2)
 * of it as its `v_mfma_f32_16x16x{32,16}_f16` A operand.  Rows are padded to a multiple of 16 with zeros.
 * hv_weight_tiled_elems: halfs the tiled table takes (0: no tiled form).  hv_weight_tile_f16: plain -> tiled (writes the zero rows too). */
size_t hv_weight_tiled_elems(int rows, int taps, int K);
int hv_weight_tile_f16(const void* w_f16, void* w_tiled, int rows, int taps, int K, void* stream);

/* Backward of the above: dw_orig = (dWsn - <dWsn, Wsn> u v^T) / sigma  (sn=1) or a layout transform (sn=0).
 * dw_ohwi is the hv_conv2d_wgrad output [Cout][taps][CinP]. */
typedef struct {
    const float* dw_ohwi; const float* w_fwd; const float* u; const float* v; const float* sigma;
    float* dw_orig; int Cout, Cin, taps, CinP, sn, transposed_src, accumulate;
} hv_wprep_bwd_layer;
int hv_weight_prep_backward(const hv_wprep_bwd_layer* d_layers, int n_layers, long long max_numel, int any_sn, void* stream);

/* 1-channel heads (models/inpaint_networks.py:115,230: clamp / sigmoid heads): loss seed -> the head's gradient carrier in one pass.
 * carrier_f16[p][0] = seed[p] * act'(y[p]) (fp16; channels 1-3 of the [pixel][4] carrier are zeroed), dbias (+)= sum_p of the stored values.
 * workspace: hv_head_seed_workspace_bytes(npix) bytes when dbias != NULL. */
size_t hv_head_seed_workspace_bytes(long long npix);
int hv_head_seed_backward(const float* seed, const void* y, int y_f16, int y_ld, int y_coff, void* carrier_f16, long long npix, int act, float* dbias,
                          int dbias_accumulate, float* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- activation gradient + bias gradient
 * g[p,c] = dy[p,c] * act'(y[p,c]) in place over dy; dbias[c] (+)= sum_p g[p,c] when dbias != NULL.
 * (autograd of nn.ELU/ReLU/Sigmoid/clamp after the conv, models/inpaint_networks.py:459-474,115,230). */
int hv_act_backward(void* dy, int dy_f16, const void* y, int y_f16 /* storage of dy / y: 0 fp32, 1 fp16 */, long long npix, int C, int dy_ld, int dy_coff,
                    int y_ld, int y_coff, int act, float* dbias, int dbias_accumulate, float* workspace, size_t workspace_bytes, void* stream);
size_t hv_act_backward_workspace_bytes(long long npix, int C);

/* ---------------------------------------------------------------- normalisation + activation (discriminator, U-Net)
 * BatchNorm2d (train: batch statistics + running-stat update, eval: running stats) or InstanceNorm2d (no affine)
 * followed by LeakyReLU(0.2)/ReLU/none (+ optional sigmoid), models/networks.py:18-36,583-595 and
 * models/UnetG_CT_mask.py:73-100.  `stats` (2*G*C floats: mean, rstd; G = 1 for batch, B for instance) is kept
 * for the backward. */
typedef struct {
    const void* x; void* y; int B, HW, C; int x_ld, x_coff, y_ld, y_coff;      /* x, y: fp32, or fp16 elements when f16 != 0.  y == NULL: statistics only (stats and
                                                                                  the running statistics are written, no pass over x beyond the reduction): the
                                                                                  consumer normalises at its own staging (hv_conv_desc.xn_stats) */
    int norm; int training; float eps, momentum;
    const float* gamma; const float* beta; float* running_mean; float* running_var; long long* num_batches_tracked;
    float* stats; int act; int post_sigmoid;
    float* workspace; size_t workspace_bytes;
    int groups;   /* batch norm: the batch is split into `groups` equal parts with separate statistics, running stats updated
                     part by part (fake | real halves of one discriminator launch == two consecutive calls); 0/1 = one group */
    int f16;      /* storage of x and y (statistics, affine parameters and all arithmetic stay fp32 / fp64) */
    const float* partials; int n_partials;
                  /* optional (batch norm, training): the producing conv's hv_conv_desc.stats -- [n_partials][C][2] partial sums of x, parts of whole
                     images in image order (groups > 1: group g is the g-th of `groups` equal ranges of them; n_partials must divide accordingly, else x is reduced here).
                     The reduction pass over x is skipped; the partials are folded in double precision in a fixed order.  NULL = reduce x here */
} hv_norm_desc;
size_t hv_norm_workspace_bytes(int B, int HW, int C);
int hv_norm_act_forward(const hv_norm_desc* d, void* stream);
/* dx from dy (gradient wrt the activation output y); dgamma/dbeta (+)= when non-NULL.  act == HV_ACT_NONE (and no post_sigmoid): dy is the
 * gradient at the normalisation's own output -- the consumer's data-gradient epilogue already applied act'(y) through hv_conv_desc.mul_src -- and
 * y is never read (may be NULL): one tensor less in both passes. */
typedef struct {
    const void* dy; const void* y; const void* x; void* dx; int B, HW, C;     /* fp32, or fp16 elements when f16 != 0 (all four alike) */
    int dy_ld, dy_coff, y_ld, y_coff, x_ld, x_coff, dx_ld, dx_coff;
    int norm; int training; const float* gamma; const float* stats;
    int act; int post_sigmoid;
    float* dgamma; float* dbeta; int param_accumulate;
    float* workspace; size_t workspace_bytes;
    int groups;
    int f16;
    const float* partials; int n_partials;
                  /* optional (batch norm, training, act == HV_ACT_NONE): hv_conv_desc.bstats of the data gradient that produced dy -- [n_partials][C][2] sums
                     (sum dy, sum dy * xhat), parts of whole images in (group, image) order, n_partials a multiple of `groups`.  The reduction pass over dy and x
                     is skipped.  NULL = reduce here */
} hv_norm_bwd_desc;
int hv_norm_act_backward(const hv_norm_bwd_desc* d, void* stream);

/* ---------------------------------------------------------------- layout / resampling helpers
 * NCHW <-> NHWC (API edge only), nearest x2 upsample + channel concat (F.interpolate + torch.cat,
 * models/inpaint_networks.py:97-99,105-106), channel copies, zero fill. */
int hv_nchw_to_nhwc(const float* src, void* dst, int dst_f16, int B, int C, int H, int W, int dst_ld, int dst_coff, void* stream);
int hv_nhwc_to_nchw(const void* src, int src_f16, float* dst, int B, int C, int H, int W, int src_ld, int src_coff, int accumulate, void* stream);
/* Copies C channels into a channel slice of dst; H,W are the dst size.  mode 0: same size; 1: src is half size
 * (nearest x2 upsample); 2: src is double size (nearest x1/2 downsample, even indices); 3: dst(half) (+)= sum of the
 * 2x2 block of src(full) [adjoint of 1]; 4: dst(full) (+)= src(half) at even indices, 0 elsewhere [adjoint of 2].
 * Modes 1 and 4 need even H and W (HV_ERR_UNSUPPORTED otherwise); modes 0, 2, 3 take any size.  16 B per lane when C, both strides and both offsets
 * are multiples of 4 and both base pointers 16-byte aligned, element by element otherwise: same result. */
int hv_copy_channels(const void* src, int src_f16, void* dst, int dst_f16, int B, int H, int W, int C, int src_ld, int src_coff, int dst_ld,
                     int dst_coff, int mode, int accumulate, void* stream);   /* *_f16: storage of src / dst (may differ: the copy converts) */
/* dst = a + b over C channels of same-size [npix] tensors, each with its own storage / channel stride / offset: a gradient with two contributions
 * (models/pix2pix_model.py:310-330 backpropagates x_stage1 and coarse_seg through a loss AND through the refinement generator) in one pass. */
int hv_add_channels(const void* a, int a_f16, int a_ld, int a_coff, const void* b, int b_f16, int b_ld, int b_coff, void* dst, int dst_f16, int dst_ld,
                    int dst_coff, long long npix, int C, void* stream);

/* ---------------------------------------------------------------- generator heads and inputs
 * cat[x, ratio-plane, mask] / cat[x, coarse_seg, mask, ratio-plane] (models/inpaint_networks.py:71-77,173-179)
 * written as a CP-channel NHWC buffer (pad channels zero).  order: 0 = coarse, 1 = fine.  CP a multiple of 4, >= 4; seg may be NULL for order 0
 * only; the ratio plane is slice_ratio rounded to fp32. */
int hv_gen_input(const float* x, const float* seg, const float* mask, const double* slice_ratio, void* dst, int dst_f16,
                 int B, int H, int W, int CP, int order, void* stream);
/* AdaptiveAvgPool2d(1) -> Linear(C,1) -> sigmoid (models/inpaint_networks.py:90-93,211-214).  C a power of two <= 256 (HV_ERR_UNSUPPORTED otherwise),
 * x_ld >= C; workspace: hv_gap_fc_workspace_bytes(B, C) bytes (HV_ERR_WORKSPACE when shorter). */
size_t hv_gap_fc_workspace_bytes(int B, int C);
int hv_gap_fc_sigmoid(const void* x, int x_f16, int B, int HW, int C, int x_ld, const float* fc_w, const float* fc_b,
                      float* pooled /*[B][C]*/, float* pred /*[B]*/, float* workspace, size_t workspace_bytes, void* stream);
/* backward: dx[n,p,c] += dpred[n]*pred(1-pred)*w[c]/HW [* act'(mul_src[n,p,c]) when mul_src: dx then holds the gradient wrt the PRE-activation of the
 * pooled tensor, like hv_conv_desc.mul_src]; dw[c] (+)= sum_n dl_n*pooled[n,c]; db (+)= sum_n dl_n.  `accumulate` is about dw / db only: dx is
 * always added to (in its storage type).  C <= 1024, mul_ld >= C. */
int hv_gap_fc_sigmoid_backward(const float* dpred, const float* pred, const float* pooled, const float* fc_w,
                               void* dx, int dx_f16, int B, int HW, int C, int dx_ld, float* dw, float* db, int accumulate,
                               const void* mul_src, int mul_f16, int mul_ld, int mul_act, void* stream);

/* ---------------------------------------------------------------- contextual attention pieces
 * (models/inpaint_networks.py:247-410).  The two big contractions (patch matching :348, patch pasting :379) and
 * their gradients go through hv_conv2d with per-sample filters; these are the memory-bound stages around them.
 * Score matrices are [b][p][l]: p = foreground position, l = background patch (contiguous), L = (H/2)*(W/2). */
/* x1/2 nearest downsample fd[B][h][w][C]; 3x3 zero-padded patches wp[B][L][9][C] (+ transposed wpT[B][9*C][L]);
 * norm[B][L] = max(||patch||, 1e-4) and rnorm = 1/norm  (:282-294, :341-345). */
int hv_ca_patches(const void* f, int f_f16 /* storage of f: 0 fp32, 1 fp16 */, int B, int H, int W, int C, int f_ld, float* fd, float* wp, float* wpT, float* norm,
                  float* rnorm, void* stream);
/* 4x4 stride-2 'same' patches of a full-resolution map (:270-277): raw[B][L][16][C] and/or rawT[B][C][16][L]. */
int hv_ca_raw_patches(const float* f, int B, int H, int W, int C, int f_ld, float* raw, float* rawT, void* stream);
/* mm[l] = 1 iff the 3x3 patch of the x1/8-downsampled mask of SAMPLE 0 is all zero (:304-317). */
int hv_ca_mask(const float* mask, int Himg, int Wimg, int h, int w, float* mm, void* stream);
/* the same for every sample's own mask: mm[B][h*w] -- a batch that stands for B independent single-sample calls (the reference's inference
 * loop runs the generator at batch 1, eval_3d_sagittal_twostage.py:101), not for one training batch (which shares sample 0's mask) */
int hv_ca_mask_batched(const float* mask, int B, long long mask_bstride, int Himg, int Wimg, int h, int w, float* mm, void* stream);
/* score fusion (two diagonal 3-tap sums with the (h,w)<->(w,h) transposes, :352-361); adjoint=1 applies the
 * transposed operator (backward).  h and w need not be equal. */
int hv_ca_fuse(const float* S, float* out, int B, int h, int w, int adjoint, void* stream);
/* A[b][p][l] = softmax_l(S*mm*scale)*mm (:364-366); optional argmax over l -> argmax[b*L+p] (:368). */
int hv_ca_softmax(const float* S, const float* mm, float* A, int B, int L, float scale, int* argmax, void* stream);
int hv_ca_softmax_batched(const float* S, const float* mm, long long mm_bstride, float* A, int B, int L, float scale, int* argmax,
                          void* stream);   /* mm_bstride = L: per-sample masks from hv_ca_mask_batched; 0: shared */
/* offset_flow of the reference's 7-tuple (:368,:389-410 + inpaint_tools.flow_to_image/compute_color :73-100,181-211): the arg-max offsets
 * coloured with the Middlebury wheel (double precision, running maximum radius over samples 0..b like the reference's batch loop), as
 * uint8/255 and nearest-upsampled x`up` (rate*4): flow[B][3][h*up][w*up] (NCHW like the reference's tensor). */
int hv_ca_flow(const int* argmax, int B, int h, int w, int up, float* flow, void* stream);
/* dS[b][p][l] = scale*mm[l]*A[b][p][l]*(dA[b][p][l] - sum_l' dA[b][p][l']*A[b][p][l']).  hv_ca_softmax_backward(_f16) take ONE mask mm[L] and apply it
 * to every sample: they are valid only after a shared-mask forward (hv_ca_softmax, or mm_bstride = 0); after a per-sample-mask forward they would read
 * sample 0's mask for all samples (the engine refuses that backward). */
int hv_ca_softmax_backward(const float* dA, const float* A, const float* mm, float* dS, int B, int L, float scale, void* stream);
int hv_transpose_batched(const float* src, float* dst, int B, int R, int C, void* stream); /* dst[b][c][r] = src[b][r][c] */
/* Batched "NT" matrix product on fp16 MFMA (fp32 accumulation and result; A / B are fp32 -- converted when staged -- or, with a_f16 / b_f16, fp16
 * tables such as hv_ca_raw_patches_f16 / hv_transpose_batched_f16 write: half the operand bytes through the vector memory path, which bounds the
 * fp32-operand form):
 *   C[b][m][n] = alpha * colscale[b][n] * sum_k A[b][m][k] * B[b][n][k]        (colscale may be NULL; strides in elements)
 * The fp16 mode's route for ContextualAttention's five big contractions (scores, paste, and their three gradients): they are plain products of
 * per-sample matrices that exist with the contraction index contiguous (csrc/bgemm.hip lists them).  K % 32 == 0, N % 4 == 0, 16-byte aligned rows.
 * b_split > 0 reads B's rows in another order: logical row n = t * b_split + c is stored as row c * (N / b_split) + t (the [channel][tap] patch
 * tables consumed in [tap][channel] order, so that C's rows hold whole channel vectors per tap).
 * hv_ca_fold: col2im of 4x4 stride-2 pad-1 patches src[b][p][tap][c] into dst[b][y][x][c] (+)= alpha * (the 4 taps reaching the pixel) -- the tail of
 * F.conv_transpose2d(..., stride=2, padding=1) (models/inpaint_networks.py:379) after the contraction, and the adjoint of hv_ca_raw_patches. */
int hv_bgemm_nt(const void* A, int a_f16, int lda, long long strideA, const void* B, int b_f16, int ldb, long long strideB, float* C, int ldc,
                long long strideC, int M, int N, int K, int batch, float alpha, const float* colscale, long long strideS, int b_split, void* stream);
int hv_ca_fold(const float* src, void* dst, int dst_f16 /* storage of dst */, int B, int H, int W, int C, int dst_ld, float alpha, int accumulate, void* stream);
/* the same pair with the product stored as fp16 (it only feeds the fold, whose result is stored as fp16 as well): half the bytes written and read */
int hv_bgemm_nt_h(const void* A, int a_f16, int lda, long long strideA, const void* B, int b_f16, int ldb, long long strideB, void* C_h, int ldc,
                  long long strideC, int M, int N, int K, int batch, float alpha, const float* colscale, long long strideS, int b_split, void* stream);
int hv_ca_fold_h(const void* src_h, void* dst, int dst_f16, int B, int H, int W, int C, int dst_ld, float alpha, int accumulate, void* stream);
/* fp16-stored forms of two operand producers (same layouts as hv_ca_raw_patches / hv_transpose_batched) */
int hv_ca_raw_patches_f16(const void* f, int f_f16 /* storage of f */, int B, int H, int W, int C, int f_ld, void* raw_h, void* rawT_h, void* stream);
int hv_transpose_batched_f16(const float* src, void* dst_h, int B, int R, int C, void* stream);
/* The GEMM route's fp16 operand copies written by their producers (round 3): hv_ca_patches_h = hv_ca_patches that also stores the [b][l][tap][c] patch
 * table as fp16 (wp_h: both operands of the score GEMM, same rounding as the GEMM's own staging of an fp32 operand -> same bits);
 * hv_ca_softmax_f16 = hv_ca_softmax(_batched) with the attention matrix stored as fp16 only (its readers are the paste GEMM, the transpose for the
 * d(raw patches) GEMM and the soft-max backward; models/inpaint_networks.py:364-381); hv_ca_softmax_backward_f16 reads that matrix;
 * hv_transpose_batched_h2h: fp16 -> fp16 (exact). */
int hv_ca_patches_h(const void* f, int f_f16, int B, int H, int W, int C, int f_ld, float* fd, float* wp, void* wp_h, float* norm, float* rnorm,
                    void* stream);
int hv_ca_softmax_f16(const float* S, const float* mm, long long mm_bstride /* L: per-sample masks, 0: shared */, void* A_h, int B, int L, float scale,
                      int* argmax, void* stream);
int hv_ca_softmax_backward_f16(const float* dA, const void* A_h, const float* mm, float* dS, int B, int L, float scale, void* stream);
int hv_transpose_batched_h2h(const void* src_h, void* dst_h, int B, int R, int C, void* stream);
/* Gs[b][i][j] = dS[b][j][i]*rnorm[b][i] + dS[b][i][j]*rnorm[b][j];  coef[b][l] = -(sum_p dS[p][l]*S0[p][l])/norm[l]^2.
 * coef must hold 17*B*L floats: the first B*L are the result, the rest is scratch for the row-chunk partial sums. */
int hv_ca_score_backward_prep(const float* dS, const float* S0, const float* norm, const float* rnorm, float* Gs, float* coef,
                              int B, int L, void* stream);
/* hv_ca_fuse(adjoint) + hv_ca_score_backward_prep in one pass for the 32 x 32 attention map (csrc/attention.hip ca_fuse_adj_prep32_kernel): dS1 is the gradient
 * of the FUSED scores; the gradient of the plain scores stays on chip.  Gs has the bits of the two-call route, coef its value in a different summation order
 * (32 row blocks).  coef must hold 33*B*L floats.  HV_ERR_UNSUPPORTED unless h = w = 32 (the caller keeps the two calls for other maps). */
int hv_ca_fuse_backward_prep(const float* dS1, const float* S0, const float* norm, const float* rnorm, float* Gs, float* coef, int B, int h, int w,
                             void* stream);
/* col2im of (dwp + coef*wp) back to the even positions of the full-resolution map (adjoint of hv_ca_patches). */
int hv_ca_patches_backward(const float* dwp, const float* wp, const float* coef, float* df, int B, int H, int W, int C,
                           int df_ld, int accumulate, void* stream);

/* The matching scores and their gradient on the PIXEL Gram matrix (csrc/attention_gram.hip; fp16 mode, C = 64, attention map width 32 or 64): the 3x3
 * patches are both filters and inputs of models/inpaint_networks.py:327-344, so S0[p][l] = rnorm[l] * sum over the 3x3 offsets t of <fd[p + t], fd[l + t]>
 * (K = C instead of 9 C; no patch tables), and d fd = box(Gs) fd + (3x3 sum of coef) fd with Gs / coef from hv_ca_score_backward_prep.
 * hv_ca_gram_down: nearest 1/2 downsampling of the fp16 map f [B][H][W][f_ld] -> fd_h [B][L][C], fdT_h [B][C][L] (fp16), q [B][L] = |fd|^2.
 * hv_ca_gram_scores: S0 [B][L][L] (row p, column l), norm / rnorm [B][L] (= hv_ca_patches' outputs).
 * hv_ca_gram_backward: df[b][2y][2x][c] += the gradient wrt fd (replaces the L x 9C gradient GEMM + hv_ca_patches_backward).
 * HV_ERR_UNSUPPORTED for other shapes (the caller keeps the patch-table route). */
int hv_ca_gram_down(const void* f, int f_f16, int B, int H, int W, int C, int f_ld, void* fd_h, void* fdT_h, float* q, void* stream);
int hv_ca_gram_scores(const void* fd_h, const float* q, int B, int h, int w, int C, float* S0, float* norm, float* rnorm, void* stream);
int hv_ca_gram_backward(const float* Gs, const void* fd_h, const void* fdT_h, const float* coef, int B, int h, int w, int C, float* df, int df_ld,
                        void* stream);

/* ---------------------------------------------------------------- step-level fused operators (Pix2PixModel)
 * Sobel edge magnitude (models/edge_operator.py:29-49). */
int hv_sobel(const float* img, float* out, int B, int H, int W, void* stream);
/* Everything Pix2PixModel.forward does after netG (models/pix2pix_model.py:191-264), one launch, no host sync:
 * pred_h = pred*maxheight; seg thresholds; SHRM compositing of fake_B / fake_B_coarse with per-sample row
 * bounds computed on the device; local crops; writes rows[B][4] = {xu2, xb2, xu1, xb1}. */
typedef struct {
    const float* real_B; const float* mask; const float* x_stage1; const float* x_stage2;
    const float* fine_seg; const float* coarse_seg; const float* pred1; const float* pred2;
    const long long* height; const long long* x1; const long long* x2; const long long* maxheight;
    float* fake_B; float* fake_B_coarse; float* fake_B_local; float* real_B_local;
    float* fine_bin; float* coarse_bin; float* pred1_h; float* pred2_h; int* rows;
    int B, H, W, half_band;
} hv_postg_desc;
int hv_post_generator(const hv_postg_desc* d, void* stream);
/* Generic SHRM compositing of one image set (train.py:81-99, eval_3d_sagittal_twostage.py:103-130). */
int hv_shrm_composite(const float* gen, const float* real, const float* pred_scaled, const long long* height,
                      const long long* x1, const long long* x2, float* out, int* rows, int B, int H, int W, void* stream);

/* GAN loss on PatchGAN logits (models/networks.py:212-278): loss (+)= weight*mean(l(z,t)); dz = weight_grad * dl/dz / n
 * mode 0 vanilla (BCE with logits), 1 lsgan (MSE). loss may be NULL (gradient only) and dz may be NULL. */
int hv_gan_loss(const float* z, long long n, int target_is_real, int mode, float loss_weight, float* loss, int loss_accumulate,
                float grad_weight, float* dz, void* stream);
/* the same over many workgroups (the one-workgroup form needs ~19 us for the 14 400 PatchGAN logits): per-workgroup partial sums in the caller's
 * scratch (hv_gan_loss_workspace_bytes(n) bytes, 4-byte aligned), added in index order by a second stage -- deterministic */
size_t hv_gan_loss_workspace_bytes(long long n);
int hv_gan_loss_ws(const float* z, long long n, int target_is_real, int mode, float loss_weight, float* loss, int loss_accumulate,
                   float grad_weight, float* dz, void* workspace, size_t workspace_bytes, void* stream);

/* The PatchGAN loss head in two launches: hv_gan_loss_ws + d loss / d logit written into the logits layer's padded fp16 gradient carrier
 * (carrier_f16[i][0]; channels 1-3 of the [n][4] carrier zeroed) + the logits layer's bias gradient dbias[0] (+)= sum of the stored values.
 * dz (fp32) and loss, dbias are optional.  workspace: hv_gan_loss_head_workspace_bytes(n) bytes. */
size_t hv_gan_loss_head_workspace_bytes(long long n);
int hv_gan_loss_head(const float* z, long long n, int target_is_real, int mode, float loss_weight, float* loss, int loss_accumulate, float grad_weight,
                     float* dz, void* carrier_f16, float* dbias, int dbias_accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* The same head for up to TWO logit ranges in ONE launch (the fake | real halves of a batched discriminator pass, models/pix2pix_model.py:272-283:
 * criterionGAN(pred_fake, False), criterionGAN(pred_real, True); or one range with n1 = 0): per range its own target and loss slot, the carrier written in place,
 * dbias[0] (+)= the sum of both ranges' stored gradients (range 0 first).  Each range's mean is over its own n.  The workgroup that finishes last folds the block
 * sums in block order (deterministic): four tiny dependent launches between a discriminator's forward and backward become one.
 * workspace: hv_gan_loss_head_pair_workspace_bytes(n0, n1) bytes of scratch; ticket: ONE zero-initialised unsigned that stays with the call site (the kernel
 * leaves it at zero; launches that share it must be ordered on one stream). */
size_t hv_gan_loss_head_pair_workspace_bytes(long long n0, long long n1);
int hv_gan_loss_head_pair(const float* z0, long long n0, int real0, float* loss0, void* carrier0_f16, const float* z1, long long n1, int real1, float* loss1,
                          void* carrier1_f16, int mode, float loss_weight, int loss_accumulate, float grad_weight, float* dbias, int dbias_accumulate,
                          void* workspace, size_t workspace_bytes, unsigned* ticket, void* stream);

/* Generator losses and their gradient seeds (models/pix2pix_model.py:331-353): writes
 * losses[0..5] = {G_maskL1, G_Dice, coarse_Dice, edge, h, sum of those five} and the seeds
 * d_fake_B (L1 part), d_fake_B_coarse, d_fine_seg, d_coarse_seg, d_pred1 (raw sigmoid output), d_pred2.
 * The four image seeds are written when all four pointers are given and none of them otherwise (losses only); d_pred1 / d_pred2 are optional one by
 * one.  Any B: up to 64 samples are finalized in one pass, more through a spill into the workspace (same results).  The mask must have a non-zero
 * element.  workspace: hv_generator_losses_workspace_bytes(B) bytes, 8-byte aligned. */
typedef struct {
    const float* fake_B; const float* fake_B_coarse; const float* real_B; const float* mask;
    const float* fine_seg; const float* coarse_seg; const float* real_B_mask; const float* normal_vert;
    const float* fake_edges; const float* real_edges; const float* pred1_h; const float* pred2_h;
    const long long* height; const long long* maxheight;
    float lambda_L1;
    float* losses; float* d_fake_B; float* d_fake_B_coarse; float* d_fine_seg; float* d_coarse_seg;
    float* d_pred1; float* d_pred2;
    int B, H, W;
    float* workspace; size_t workspace_bytes;
    float grad_scale;   /* the six gradient seeds are multiplied by this (0 = 1): the gradient (loss) scale of the fp16 storage mode, a power of two
                           removed again from the parameter gradients by the caller (the losses themselves are not scaled) */
    /* optional bookkeeping folded into the same launches (each was a 1-element kernel at the head of the generator backward):
       loss_G_GAN = gan_terms[0] + ... + gan_terms[n_gan_terms-1] (in this order), loss_G = losses[5] + loss_G_GAN;
       add_d_fake_B: d_fake_B[i] += add_d_fake_B[i] (the discriminator's gradient wrt the composited image) */
    const float* gan_terms; int n_gan_terms; float* loss_G_GAN; float* loss_G;
    const float* add_d_fake_B;
} hv_gloss_desc;
size_t hv_generator_losses_workspace_bytes(int B);
int hv_generator_losses(const hv_gloss_desc* d, void* stream);
/* Gradient of the compositing + local crop: d_gen[row] = (d_fake[row] + d_local[row]*mask*band) for xu<=row<xb else 0.
 * which: 0 -> rows[b][0..1] (stage 2), 1 -> rows[b][2..3] (stage 1).  band: columns W/2 - half_band <= col < W/2 + half_band.  d_fake and d_local may
 * each be NULL (that term is absent; mask is read only with d_local); accumulate: d_gen += instead of =. */
int hv_shrm_backward(const float* d_fake, const float* d_local, const float* mask, const int* rows, int which,
                     float* d_gen, int B, int H, int W, int half_band, int accumulate, void* stream);

/* ---------------------------------------------------------------- optimiser
 * Multi-tensor Adam, torch.optim.Adam semantics (models/pix2pix_model.py:127-130): one launch per optimiser.
 * `state[0]` holds the step count as float (incremented by the kernel), lr is read from d_lr[0] so a captured
 * graph follows the scheduler. */
typedef struct { float* p; const float* g; float* m; float* v; long long n; } hv_adam_tensor;
int hv_adam_step(const hv_adam_tensor* d_tensors, int n_tensors, long long max_numel, const float* d_lr, float beta1,
                 float beta2, float eps, float* d_step, void* stream);
/* The same behind an overflow guard (fp16 storage mode: scaled gradients may have overflowed to inf / nan in an fp16 gradient buffer):
 * flat_grad[n_grad] -- the network's flat gradient buffer, after any all-reduce -- is checked first and multiplied by grad_mul on the way (1 / the loss
 * scale, a power of two; 1 = left alone); if it holds a non-finite value the whole step is skipped (weights, moments and step count unchanged) and
 * d_state[2] counts it.  d_state: 8 floats {step count, scratch, skipped steps, scratch, ticket, -, -, -}, zero-initialised by the caller.  Two launches
 * (check + update); device-side only (no host read): safe inside a captured graph.
 * "Non-finite" is the test !(|g| <= 3.0e38) on the values before the multiplication: inf and nan, and also the finite fp32 values above 3.0e38 (up to
 * FLT_MAX = 3.4e38) count as an overflow; 3.0e38 itself passes.  The multiplication by grad_mul happens on good and skipped steps alike: after the call
 * flat_grad holds the unscaled gradient either way (a non-finite element stays non-finite).  After every call d_state[1] and the ticket d_state[4] are back
 * at zero and d_state[3] says whether THIS step was skipped (1) or taken (0).  Returns HV_ERR_ARG -- before any launch -- for a NULL pointer,
 * n_tensors / max_numel / n_grad <= 0, a flat_grad that is not 16-byte aligned or a grad_mul that is not > 0 (nan included). */
int hv_adam_step_guarded(const hv_adam_tensor* d_tensors, int n_tensors, long long max_numel, const float* d_lr, float beta1,
                         float beta2, float eps, float* d_state, float* flat_grad, long long n_grad, float grad_mul, void* stream);

/* misc */
int hv_threshold(const float* x, float* y, long long n, float thr, float value, void* stream); /* y = x > thr ? value : 0 (torch.where(seg > 0.5, ...)) */
int hv_fill(float* p, long long n, float value, void* stream);
int hv_axpy(float* y, const float* x, long long n, float a, void* stream); /* y += a*x */
int hv_affine(float* y, const float* x, long long n, float a, float b, void* stream); /* y = a*x + b (e.g. 1 - CAM) */
int hv_mul(float* y, const float* x, long long n, void* stream);                  /* y *= x (pred_h = pred * maxheight) */
int hv_mul3(float* y, const float* x, const float* z, long long n, void* stream); /* y = (y*x)*z (mask * image * centre band, pix2pix_model.py:254-263) */

/* ---- in-training evaluation metrics (reference train.py:37-48 dice_score / iou_score, :101-141 per-sample body of evaluate_model;
 * SURVEY.md section 8f row f3).  All images (B,1,H,W) fp32: `inpainted` = the SHRM-composited stage-2 output (hv_shrm_composite with
 * pred_h = pred2*maxheight), gt = real_B, coarse_bin / fine_bin = (seg > 0.5) (hv_threshold), normal_vert / label / mask as loaded;
 * pred_h [B] fp32, height [B] int64.  out[B][5] = { SSIM(gt*mask, inpainted*mask; data_range = max(inpainted) - min(inpainted)),
 * PSNR(gt*mask, inpainted*mask; data_range = max(inpainted) - min(gt)), dice(coarse_bin, normal_vert), iou(fine_bin, label),
 * |pred_h - height| / height * 100 }.  SSIM / PSNR follow scikit-image 0.22's published algorithm (7x7 uniform window, sample
 * covariance, K1 0.01, K2 0.03, 3-pixel border cropped; float64 means) -- see csrc/eval_metrics.hip. */
size_t hv_eval_metrics_workspace_bytes(int B, int H, int W);
int hv_eval_metrics(const float* inpainted, const float* gt, const float* mask, const float* coarse_bin, const float* normal_vert,
                    const float* fine_bin, const float* label, const float* pred_h, const long long* height, int B, int H, int W, float* out,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- RHLV quantification (reference evaluation/RHLV_quantification.py:41-147,160-178) ----
 * fake / label: straightened label volumes of the generated and the original vertebra, element (h, w, z) at
 * base[h*stride_h + w*stride_w + z*stride_z] (strides in elements); dtype 0 = float32, 1 = uint8.  A voxel belongs to the vertebra if it
 * equals label_index (label_index < 0: if it is non-zero).  z_lo == INT_MIN: the slice range is derived from the original vertebra's
 * z-extent like the reference (centre = int(mean z), half-length = (max_z - min_z) // length_divisor, numpy slice rules), else [z_lo, z_hi).
 * out (14 doubles, device): all / pre / mid / post RHLV, relative height of the original, the eight mean heights
 * (all_f, all_l, pre_f, pre_l, mid_f, mid_l, post_f, post_l), and 1.0 / 0.0 = the original vertebra exists. */
size_t hv_rhlv_workspace_bytes(int W, int Z);
int hv_rhlv(const void* fake, const void* label, int dtype, long long stride_h, long long stride_w, long long stride_z, int H, int W, int Z,
            float label_index, int length_divisor, int z_lo, int z_hi, double height_threshold, double* out, void* workspace,
            size_t workspace_bytes, void* stream);

/* ---- RHLV in the sagittal and / or the coronal view from one pass over the volumes (the six features of evaluation/SVM_grading_2.5d.py:
 * reference evaluation/RHLV_quantification.py and evaluation/RHLV_quantification_coronal.py, :41-147 and the per-vertebra body of
 * process_datasets_to_excel) ----
 * Volumes, dtype, strides and label_index as for hv_rhlv.  Both scripts start from the table cnt[z][w] = #{h : vol[h][w][z] is the vertebra}, which
 * is built once; the sagittal view walks it as slices z with columns w, the coronal view (the reference's [:, z, :]) as slices w with columns z,
 * its range taken from the original vertebra's extent along w.  `views`: HV_RHLV_SAGITTAL, HV_RHLV_CORONAL or both; h_sagittal / h_coronal (host)
 * carry each requested view's length_divisor, explicit slice range [lo, hi) (lo == INT_MIN: derived like the reference) and height_threshold.
 * The coronal view follows the coronal script's own arithmetic: rescale ratio label.max() / fake.max() without the sagittal script's + 1e-6
 * (inf where a third of the generated vertebra is empty: those columns then select nothing), and where a participating slice's pre or mid third
 * of columns is empty the script raises ValueError (max() of an empty array) -- the record's flag says so.
 * out (device): one 16-double record per requested view, sagittal first: hv_rhlv's 14 values, [14] = 1.0 if the reference would have raised
 * (coronal view only), [15] = 0.  hv_rhlv_views_batch: n_pairs pairs of equal shape, dtype and strides; pairs = DEVICE table
 * {fake_0, label_0, fake_1, label_1, ...} of volume pointers, label_indices = DEVICE [n_pairs]; out [n_pairs][views][16]; nothing is read back,
 * and n_pairs == 1 gives hv_rhlv_views' bits.  workspace: hv_rhlv_views_workspace_bytes(W, Z, views, n_pairs) bytes, 8-byte aligned. */
enum { HV_RHLV_SAGITTAL = 1, HV_RHLV_CORONAL = 2 };
typedef struct {
    int length_divisor, lo, hi;
    double height_threshold;
} hv_rhlv_view;
size_t hv_rhlv_views_workspace_bytes(int W, int Z, int views, int n_pairs);
int hv_rhlv_views(const void* fake, const void* label, int dtype, long long stride_h, long long stride_w, long long stride_z, int H, int W, int Z,
                  float label_index, int views, const hv_rhlv_view* h_sagittal, const hv_rhlv_view* h_coronal, double* out, void* workspace,
                  size_t workspace_bytes, void* stream);
int hv_rhlv_views_batch(const void* pairs, const float* label_indices, int n_pairs, int dtype, long long stride_h, long long stride_w,
                        long long stride_z, int H, int W, int Z, int views, const hv_rhlv_view* h_sagittal, const hv_rhlv_view* h_coronal,
                        double* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- per-column height-loss maps and profiles of RHLV (the distribution of height loss over the vertebra's cross-section and the curve of
 * height loss along it, reference README "Clinical value"; the same lines of the two scripts as hv_rhlv_views) ----
 * Arguments, records (`out`, [n_pairs][views][16], bit for bit hv_rhlv_views' / hv_rhlv_views_batch's) and the pass over the volumes as for
 * hv_rhlv_views / hv_rhlv_views_batch; in addition, per requested view (S slices of C columns: sagittal S = Z, C = W; coronal S = W, C = Z), what the
 * script computes per column of a slice before it folds it into means.  For a slice s the script visits (inside [lo, hi) after numpy slice
 * normalisation, both volumes non-empty there) and a column c:
 *   height_fake[s][c]  = cnt_fake[s][c] * all_scale_ratio[s]  (all_height_fake * all_scale_ratio, :93; the view's own ratio arithmetic)
 *   height_label[s][c] = cnt_label[s][c]                      (:70)
 *   flags[s][c]: bits 0-1 = 0 pre (c < one_third_y), 1 mid (c < two_third_y), 2 post (:60-61); bit 2 = height_fake > center_height_fake *
 *                all_scale_ratio * height_threshold (:99); bit 3 = height_label > center_height_label * height_threshold (:100); bit 4 = visited
 *   loss[s][c]         = (height_fake - height_label) / (height_fake + 1e-6) where bit 2 is set, NaN elsewhere (the formula of :139 per column)
 * and a slice that is not visited is a row of NaN losses, zero heights and zero flags.
 *   column_profile [3][C]: profile_fake[c] = sum over s of the bit-2 height_fake / their number, profile_label[c] the same of the bit-3 height_label,
 *                  curve[c] = (profile_fake - profile_label) / (profile_fake + 1e-6); NaN where no slice selects the column
 *   slice_profile [3][S]: the same three per slice s over its columns
 *   range [2]: lo, hi after normalisation (0, 0 where the original lacks the vertebra)
 * Sums run in ascending index order, one lane each: the results do not change from run to run or between the single and the batched entry.
 * Every hv_rhlv_map_out pointer is a DEVICE pointer or NULL = not wanted; the structs themselves (h_*) are host memory, NULL = nothing wanted of
 * that view.  hv_rhlv_maps_batch: every array gains a leading [n_pairs] axis.  workspace: hv_rhlv_maps_workspace_bytes bytes, 8-byte aligned. */
typedef struct {
    double* loss;           /* [S][C] */
    double* height_fake;    /* [S][C] */
    double* height_label;   /* [S][C] */
    uint8_t* flags;         /* [S][C] */
    double* column_profile; /* [3][C] */
    double* slice_profile;  /* [3][S] */
    int* range;             /* [2] */
} hv_rhlv_map_out;
size_t hv_rhlv_maps_workspace_bytes(int W, int Z, int views, int n_pairs);
int hv_rhlv_maps(const void* fake, const void* label, int dtype, long long stride_h, long long stride_w, long long stride_z, int H, int W, int Z,
                 float label_index, int views, const hv_rhlv_view* h_sagittal, const hv_rhlv_view* h_coronal, const hv_rhlv_map_out* h_sagittal_out,
                 const hv_rhlv_map_out* h_coronal_out, double* out, void* workspace, size_t workspace_bytes, void* stream);
int hv_rhlv_maps_batch(const void* pairs, const float* label_indices, int n_pairs, int dtype, long long stride_h, long long stride_w,
                       long long stride_z, int H, int W, int Z, int views, const hv_rhlv_view* h_sagittal, const hv_rhlv_view* h_coronal,
                       const hv_rhlv_map_out* h_sagittal_out, const hv_rhlv_map_out* h_coronal_out, double* out, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- RHLV parameter sweep: every (length_divisor, height_threshold) of a grid from one pass over the volumes (the tuning the reference's
 * evaluation/RHLV_quantification.py imports sklearn's ParameterGrid for; its defaults are 5 / 0.64, its main() passes 0.7) ----
 * pairs, label_indices, dtype, strides and `views` as for hv_rhlv_views_batch.  Neither parameter touches the column-count table or a slice's
 * thirds, maxima, rescale ratios and centre heights: the volumes are read once per pair, the threshold then only selects columns of the
 * L2-resident table and the divisor only selects which slices are folded.  h_grid (HOST, copied into the kernel arguments: 328 bytes) lists
 * 1 ... HV_RHLV_MAX_DIVISORS divisors (each > 0) and 1 ... HV_RHLV_MAX_THRESHOLDS thresholds; a count outside that, a divisor <= 0 or a shape
 * with H * max(W, Z) > INT_MAX returns HV_ERR_UNSUPPORTED with nothing launched.  The slice range always derives from the original vertebra's
 * extent (hv_rhlv_view's explicit [lo, hi) form is not part of the sweep).
 * out (device): [n_pairs][n_divisors][n_thresholds][views][16] doubles, each record laid out like hv_rhlv_views' ([13] the original exists,
 * [14] the coronal script would have raised -- a property of the divisor's slices, not of the threshold) and bit for bit the record
 * hv_rhlv_views_batch gives at that single setting, whatever the rest of the grid and of the batch.  No atomics, no cross-lane floating-point
 * sums.  workspace: hv_rhlv_sweep_workspace_bytes(W, Z, views, n_pairs, n_divisors, n_thresholds) bytes (0 for arguments the entry refuses),
 * 8-byte aligned: the one-setting entries' slab plus 64 bytes per (slice, threshold) of every view and pair. */
enum { HV_RHLV_MAX_DIVISORS = 16, HV_RHLV_MAX_THRESHOLDS = 32 };
typedef struct {
    int n_divisors;
    int divisor[HV_RHLV_MAX_DIVISORS];
    int n_thresholds;
    double threshold[HV_RHLV_MAX_THRESHOLDS];
} hv_rhlv_grid;
size_t hv_rhlv_sweep_workspace_bytes(int W, int Z, int views, int n_pairs, int n_divisors, int n_thresholds);
int hv_rhlv_sweep(const void* pairs, const float* label_indices, int n_pairs, int dtype, long long stride_h, long long stride_w,
                  long long stride_z, int H, int W, int Z, int views, const hv_rhlv_grid* h_grid, double* out, void* workspace,
                  size_t workspace_bytes, void* stream);

/* ---- batch assembly on the device (reference data/aligned_dataset.py:204-280, AlignedDataset.__getitem__) ----
 * One item = one sagittal slice of a vertebra volume whose four uint8 planes [H][W] are resident on the device: ct = ct_data.astype(uint8)
 * (:245), vert = component-filtered vertebra mask * 255 (:247-248), normal = the patient's normal vertebrae as 0/255 (:190-196), cam =
 * (CAM * 255).astype(uint8) (:167,250) -- the reference quantises per item, a resident volume is quantised once.  [min_x, max_x) is the
 * masked band (:214-226), x1 / x2 the vertebra's first / last row (:205).  Outputs are the six float32 planes [B][H][W] the loader
 * collates: A = norm(ct), B = norm(restack(ct)), A_mask = vert / 255, mask = band, normal_vert = restack(normal) / 255,
 * CAM = restack(cam) / 255, with restack(v)[r] = v[r + x1 - min_x] above the band, v[x2 + r - max_x] below it, 0 inside (:232-243),
 * norm(u) = (u / 255 - 0.5) / 0.5 (torchvision ToTensor + Normalize((0.5,), (0.5,)), float32 arithmetic, bit-identical).
 * Every source row an item addresses must lie in [0, H) (the reference raises a broadcasting error otherwise): HV_ERR_ARG is NOT
 * detected for device-side descriptors -- the host mirror validates before upload. */
typedef struct {
    const uint8_t* ct; const uint8_t* vert; const uint8_t* normal; const uint8_t* cam;
    int x1, x2, min_x, max_x;
} hv_assemble_item;
int hv_assemble_batch(const hv_assemble_item* d_items, int B, int H, int W, float* A, float* Bimg, float* A_mask, float* mask,
                      float* normal_vert, float* CAM, void* stream);   /* d_items: DEVICE array of B descriptors */

/* ---- slice preparation of the inference driver on the device (reference eval_3d_sagittal_twostage.py:15-30,46-98; 8f rows f1 / f2) ----
 * hv_slice_components: per slice s of label [S][H][W]: 8-connected components of (label == value), components with fewer than min_size
 * pixels dropped (remove_small_connected_components); stats[s] = {pixel count, first row, last row, sum of row indices} of what remains
 * (count 0: first row -1).  workspace: hv_slice_components_workspace_bytes(S, H, W) bytes.  HV_ERR_UNSUPPORTED, before any launch, unless
 * H * W <= 2^24 and H * W * (H - 1) / 2 <= INT_MAX (the row sum of a full slice is an int); the same for hv_slice_components_u8.
 * hv_infer_prepare: from those stats the rows run_model works with (x1, x2, height; the 40-row window around the mean row when the vertebra
 * is taller than maxheight) and the generator's four input planes [S][1][H][W]: ct_masked / cam = uint8-quantised slice re-stacked around the
 * band [min_x, max_x), ori_ct = the quantised slice, mask = rows [min_x, max_x] -- ToTensor / Normalize applied.  ct / cam: [S][H][W] float32 in
 * [0, 256).  selected (or NULL = all): slices this stage runs on.  valid[s] = vertebra present and selected; slices that are not valid get
 * rows that keep the re-compositing in bounds (x1 = x2 = 0, height = H) and zero planes.
 * hv_select_slices: dst[s] = flag[s] ? src[s] : (keep_unflagged ? dst[s] : 0)  -- slices without the vertebra pass a stage unchanged.
 * hv_slice_components_u8: the same component filter on a uint8 mask plane [S][H][W] (pixels == value, 1..255) -- the loader's
 * remove_small_connected_components on a drawn slice (data/aligned_dataset.py:16-31,:186-188) for every slice of a resident volume at once;
 * filtered (NULL, or [S][H][W], may be `plane` itself) receives the mask without the dropped components; stats as above
 * (count / first row / last row feed the loader's slice acceptance test and band rows, aligned_dataset.py:126-146,:198-226).
 * hv_slice_count: count[s] = number of elements of slice s ([S][per_slice] floats) equal to value -- the `> 200 pixels of the neighbour on the
 * original labels` gate of the volume driver (eval_3d_sagittal_twostage.py:208,217). */
size_t hv_slice_components_workspace_bytes(int S, int H, int W);
int hv_slice_components(const float* label, int S, int H, int W, float value, int min_size, int* stats, void* workspace,
                        size_t workspace_bytes, void* stream);
int hv_infer_prepare(const float* ct, const float* cam, const int* stats, const int* selected, int S, int H, int W, int maxheight,
                     float* ct_masked, float* ori_ct, float* mask, float* cam_out, long long* x1, long long* x2, long long* height,
                     int* valid, void* stream);
int hv_select_slices(const int* flag, const float* src, float* dst, int S, long long per_slice, int keep_unflagged, void* stream);
int hv_slice_components_u8(const void* plane /* uint8 */, int S, int H, int W, int value, int min_size, int* stats, void* filtered /* uint8 */,
                           void* workspace, size_t workspace_bytes, void* stream);
int hv_slice_count(const float* label, int S, long long per_slice, float value, int* count, void* stream);

/* Volume intake / output of the inference driver (reference eval_3d_sagittal_twostage.py:186-197,:208,:217,:236-239): the float64 [H][W][Z] volumes
 * (z fastest, as nibabel hands them over) are uploaded as they lie and everything else happens on the device.
 * hv_volume_scan: counts[j * Z + z] = number of voxels of slice z equal to id_j, j = 0..2 (an unused id is passed as a negative number; no id may
 *   be 0) -- the vertebra's z-extent (`np.any(label == vert_id)` per slice, :186-190) and the two neighbours' `> 200 pixels` gates (:208,:217) from
 *   one pass over the label volume.  counts: 3 * Z ints, zeroed by the call.  Z <= 2048.
 * hv_volume_slices: out[s][p] = (float)vol[p * Z + z0 + s], s < S, p < HW: the z-range cut out, converted (C cast = numpy astype) and transposed
 *   to [S][H*W] float32 slices.
 * hv_volume_merge: out[p * Z + z] = (z0 <= z < z0 + S and flag[z - z0]) ? (double)src[(z - z0) * HW + p] : 0 for ALL z < Z: the float64 output
 *   volume as the reference builds it (np.zeros, then the processed slices, :236-239). */
int hv_volume_scan(const double* label, long long HW, int Z, double id0, double id1, double id2, int* counts, void* stream);
int hv_volume_slices(const double* vol, long long HW, int Z, int z0, int S, float* out, void* stream);
int hv_volume_merge(const float* src, const int* flag, long long HW, int Z, int z0, int S, double* out, void* stream);
/* The same three for either in-plane slice axis of a C-contiguous volume [A0][A1][A2] (element (a0, a1, a2) at (a0 * A1 + a1) * A2 + a2) of dtype HV_DT_F64,
 * HV_DT_F32 or HV_DT_U8 (codes below; uint8 is what hv_straighten_crop leaves for labels): axis = 2 slices `[:, :, k]` (sagittal, planes [A0][A1]: the
 * entries above, bit for bit on float64), axis = 1 slices `[:, k, :]` (coronal, planes [A0][A2]: evaluation/RHLV_quantification_coronal.py:51-54).  N = the
 * size of the slice axis, C = the other in-plane axis (A1 for axis 2, A2 for axis 1).
 * hv_volume_scan_view: counts[j * N + k] = number of voxels of slice k equal to id_j (id rules as hv_volume_scan).  counts: 3 * N ints, zeroed by the
 *   call.  axis 2: A2 <= 2048.
 * hv_volume_slices_view: out[s][a0][c] = (float)vol[...] for slices k0 .. k0 + S - 1: the range cut out, converted (C cast) and laid out as [S][A0][C] float32.
 * hv_volume_merge_view: every element of out ([A0][A1][A2], out_dtype HV_DT_F64 -- the reference's volume -- or HV_DT_F32 -- what a resident consumer
 *   such as hv_rhlv reads without a conversion) is written: src[k - k0][a0][c] where k0 <= k < k0 + S and flag[k - k0], 0 elsewhere.
 * HV_ERR_ARG: null pointer, non-positive size, axis other than 1 / 2, unknown dtype, an id of 0, k0 < 0, S <= 0, k0 + S > N.  HV_ERR_UNSUPPORTED: A0 * A1 or
 *   A0 * A2 > 2^31, A2 > 2048 (scan, axis 2), S (slices) or N (merge) > 65535 on axis 1 / > 32 * 65535 on axis 2. */
int hv_volume_scan_view(const void* label, int dtype, int A0, int A1, int A2, int axis, double id0, double id1, double id2, int* counts, void* stream);
int hv_volume_slices_view(const void* vol, int dtype, int A0, int A1, int A2, int axis, int k0, int S, float* out, void* stream);
int hv_volume_merge_view(const float* src, const int* flag, int A0, int A1, int A2, int axis, int k0, int S, int out_dtype, void* out, void* stream);

/* ---- spine straightening and per-vertebra volume extraction (reference straighten/location_json_local.py:14-16,33-45,
 * straighten/straighten_mask_3d.py:123-146,172-184,222-247,463-563, straighten/curve.py:54-102) ----
 * Volumes are [D0][D1][D2] (the NIfTI axes as nibabel hands them over), element (i, j, k) at base[i*s0 + j*s1 + k*s2] (strides in elements,
 * any order: a Fortran-ordered array passes as it lies).  dtype codes below; the CT may be HV_DT_I16 / F32 / F64, the label any of them.
 * hv_straighten_stats: one read of each volume into `stats` (hv_straighten_stats_bytes(D1) bytes, zeroed by the call; ct may be NULL: labels
 *   only), 64-bit words:
 *   [0] ~key(min CT), [1] key(max CT) with key(v) = the double's bits, sign bit flipped for v >= 0, all bits flipped for v < 0;
 *   [2] non-zero if a label is not an integer in [0, 255]; [4 + l] voxel count of label l (1..255; label 0 is not counted);
 *   [260 + 3 l + a] sum of the axis-a index over the voxels of label l; [1028 ...] presence bits of the raw geometry (below).
 * Presence bits (remove_spine_labels_after_split): for a volume whose height axis has R rows, word l * ceil((R - R/2) / 64) + h / 64, bit h % 64
 *   is set if label l occurs in row R/2 + h of the centre column (all of axis 0, axis 2 at its centre); hv_straighten_presence_bytes(R) bytes.
 * hv_straighten_sample: the straight volumes [N][PA][PB] (interpolate_along(vol, (PB, PA)), 128 x 128 in the reference): sample (n, a, b) at
 *   knots[n] + basis[n][:,1] (b - PB/2) + basis[n][:,2] (a - PA/2) (knots [N][3], basis [N][3][3] row-major, fp64), trilinear on the CT
 *   (windowed when `window`: 255 (v - win_min) / (win_max - win_min) clipped to [0, 255]), nearest on the label, 0 outside [0, D - 1];
 *   presence (hv_straighten_presence_bytes(PA) bytes, zeroed by the call) for the straight label.
 * hv_straighten_sample_sp: the same for a scan with anisotropic voxels (Interpolator(curve, step, spacing=...), curve.py:26-52,74,160-195).
 *   spacing (HOST pointer, 3 doubles: millimetres per voxel along axes 0, 1, 2; copied into the kernel's arguments, no device allocation);
 *   knots and basis are those of the curve in millimetres (curve * spacing) and sample (n, a, b) lies at
 *   (knots[n] + basis[n][:,1] (b - PB/2) + basis[n][:,2] (a - PA/2)) / spacing, per axis, in voxel indices of the scan; everything after the
 *   coordinate is hv_straighten_sample's.  The straight volumes are on a 1 mm grid whatever the scan's spacing.  hv_straighten_sample is
 *   this entry with spacing {1, 1, 1} (x / 1.0 is exact: the same bits).  HV_ERR_ARG as for hv_straighten_sample, and for a NULL,
 *   non-positive or non-finite spacing: nothing is launched and nothing is written.
 * hv_straighten_crop: extract_3d_volume for V vertebrae in one launch from a source volume (the straight ones: dtype F64 / U8, D1 = PA; or the
 *   raw ones, windowed when `window`): boxes (device, V x 9 ints) {lo0, lo1, lo2, len0, len1, len2, start0, start1, start2}: output (i, j, k)
 *   of vertebra v = source (lo + (i, j, k) - start) where 0 <= (i, j, k) - start < len, else 0.  A label voxel in a source row (axis 1) at or
 *   past its label's cutoff (the first row >= D1/2 whose presence bit is clear) becomes 0.  ct_out [V][O0][O1][O2] fp64, label_out the same
 *   in uint8.  Labels must have passed hv_straighten_stats (the flag) first. */
enum { HV_DT_U8 = 0, HV_DT_I16 = 1, HV_DT_I32 = 2, HV_DT_I64 = 3, HV_DT_F32 = 4, HV_DT_F64 = 5 };
size_t hv_straighten_presence_bytes(int rows);
size_t hv_straighten_stats_bytes(int D1);
int hv_straighten_stats(const void* ct, int ct_dtype, long long cs0, long long cs1, long long cs2, const void* label, int label_dtype,
                        long long ls0, long long ls1, long long ls2, int D0, int D1, int D2, uint64_t* stats, size_t stats_bytes, void* stream);
int hv_straighten_sample(const void* ct, int ct_dtype, long long cs0, long long cs1, long long cs2, const void* label, int label_dtype,
                         long long ls0, long long ls1, long long ls2, int D0, int D1, int D2, const double* knots, const double* basis, int N,
                         int PA, int PB, int window, double win_min, double win_max, double* straight_ct, uint8_t* straight_label,
                         uint64_t* presence, size_t presence_bytes, void* stream);
int hv_straighten_sample_sp(const void* ct, int ct_dtype, long long cs0, long long cs1, long long cs2, const void* label, int label_dtype,
                            long long ls0, long long ls1, long long ls2, int D0, int D1, int D2, const double* knots, const double* basis, int N,
                            int PA, int PB, int window, double win_min, double win_max, double* straight_ct, uint8_t* straight_label,
                            uint64_t* presence, size_t presence_bytes, const double* spacing, void* stream);
int hv_straighten_crop(const void* ct, int ct_dtype, long long cs0, long long cs1, long long cs2, const void* label, int label_dtype,
                       long long ls0, long long ls1, long long ls2, int D1, int window, double win_min, double win_max, const uint64_t* presence,
                       const int* boxes, int V, int O0, int O1, int O2, double* ct_out, uint8_t* label_out, void* stream);

/* ---- de-pedicling of label crops (reference straighten/straighten_mask_3d.py:189-219 process_layer / process_3d_array and :249-280
 * find_single_component_layers).  V volumes [A0][A1][Z]: element (i0, i1, z) of volume v at
 * label[v*lsv + i0*ls0 + i1*ls1 + z*ls2] (strides in elements, any order; label_dtype one of the HV_DT_* codes above), values integers in
 * [0, 255].  Per slice [:, :, z], with the raster index p = i0*A1 + i1: pixels are joined iff they are 4-neighbours (never diagonal) holding
 * the same non-zero value (the union over the values of scipy.ndimage.label(layer == value) with the default structure); a component's
 * identity is its smallest raster index; per value the component with the smallest (min i1 over the component, identity) is kept and every
 * other pixel of that value becomes 0.
 * out: uint8, element at out[v*osv + i0*os0 + i1*os1 + z*os2]; may be the label buffer itself when that is uint8 with the same strides (a
 *   slice is read completely before it is written).  NULL with counts != NULL: the counts only.
 * counts: NULL or [V][Z][256] int32: the number of components of every value 1..255 in the slice (0 for an absent value); entry 0 is 0, or -1
 *   for a slice whose labelling hit its iteration bound.
 * status: [V] int32, zeroed by the call; bit 0: the volume holds a value that is not an integer in [0, 255] (nothing else is promised for
 *   that slice), bit 1: a slice did not converge (see counts).
 * The labelling state lives in LDS (one 16-bit parent per pixel), no workspace.  HV_ERR_ARG: label or status NULL, out and counts both NULL,
 * a non-positive size, an unknown dtype code.  HV_ERR_UNSUPPORTED: A0 * A1 > 65536 (128 KiB of parents is what fits the 160 KiB of LDS; the
 * reference's crops are 256 x 256 x 64) or V > 65535.  In both cases nothing is launched and nothing is written. */
int hv_depedicle(const void* label, int label_dtype, long long ls0, long long ls1, long long ls2, long long lsv, int A0, int A1, int Z, int V,
                 uint8_t* out, long long os0, long long os1, long long os2, long long osv, int* counts, int* status, void* stream);

/* ---- restore of a straightened (synthesized) vertebra crop to patient CT space (reference straighten/straighten/curve.py:104-150,223-239
 * Interpolator.global_to_local / _to_local / _transform / interpolate_coords, which the reference runs one point at a time; DESIGN.md section
 * 8 row f8).  One lane per voxel p = (x, y, z) of the patient-space box region = {x0, y0, z0, nx, ny, nz} (HOST pointer, inside [D0][D1][D2]):
 *   local = global_to_local(p): per knot n d = p - knots[n], to_origin = |d|, q = basis[n]^T d, to_plane = q[0], coords = q + (cumlen[n],
 *   centre1, centre2); idx = the first minimum of to_origin, replaced by the n with sign(to_plane[n+1]) != sign(to_plane[n]) (sign(0) = 0)
 *   nearest to it (the lowest on ties) if there is one; coords interpolated linearly to to_plane = 0 over the planes [max(0, idx - 2),
 *   min(N, idx + 2)) (stable sort by to_plane, searchsorted left, segment clipped to [1, len - 1], slope * (0 - x_lo) + y_lo).
 *   knots [N][3], basis [N][3][3] row-major, cumlen [N] = cumulative_length(knots) (device, fp64), N >= 2; they are staged in LDS up to 630
 *   knots and read from global memory beyond.
 *   Crop coordinate: the straight volume is indexed (n, a, b) = (local[0], local[2], local[1]) (interpolate_along's meshgrid puts frame vector
 *   2 on axis 1); c = that - lo + start with box = {lo0, lo1, lo2, len0, len1, len2, start0, start1, start2} (HOST pointer, the row
 *   hv_straighten_crop took for the vertebra).  p is covered iff start_i <= c_i <= start_i + len_i - 1 on all three axes and local is
 *   finite: the crop's zero padding is never read.  CT sample: trilinear (map_coordinates order 1) on crop_ct ([O0][O1][O2], HV_DT_F32 or
 *   HV_DT_F64, strides in elements); label sample: crop_label (uint8) at floor(c + 0.5) (order 0).
 *   knots == NULL (the single-centroid branch: the crop was cut from the raw volume): c = p - lo + start in integers, covered iff
 *   0 <= p - lo < len.
 * where = HV_RESTORE_CROP: every covered voxel is written; HV_RESTORE_VERTEBRA: a covered voxel is written only if the label sample equals
 *   vert_id or patient_label (any HV_DT_* code, strides in elements; may be NULL for HV_RESTORE_CROP) holds vert_id at p.
 * A written voxel gets the CT sample into ct_out (fp64), the label sample into label_out (uint8) and 1 into covered (uint8, may be NULL), all
 *   [D0][D1][D2] with their own strides; every other voxel is left as it is.  local_out: NULL or [nx][ny][nz][3] fp64, the local coordinate of
 *   every box voxel (NaN where it is not finite; p itself with knots == NULL).  One call per vertebra; calls on one stream apply in order.
 * HV_ERR_ARG: null pointer, non-positive size, crop dtype not F32 / F64, unknown `where`, vert_id outside 0..255, N < 2, a box that leaves the
 *   crop, a region that leaves the patient volume: nothing is launched and nothing is written.  An empty region or box is HV_OK.
 * hv_restore_volume_sp: the same for a scan with anisotropic voxels: spacing (HOST pointer, 3 doubles, millimetres per voxel along axes
 *   0, 1, 2; copied into the kernel's arguments), knots / basis / cumlen those of the curve in millimetres; a box voxel p enters the knot
 *   scans as p * spacing (pixel_to_spatial, curve.py:108,160-176) and everything after the local coordinate is unchanged (the crop is on
 *   the 1 mm grid of the straight volumes).  With knots == NULL the spacing plays no part.  hv_restore_volume is this entry with spacing
 *   {1, 1, 1} (x * 1.0 is exact: the same bits).  A NULL, non-positive or non-finite spacing is HV_ERR_ARG as above.
 * hv_curve_points: Interpolator.global_to_local / local_to_global (curve.py:104-150,223-239) for M points ([M][3] fp64, device), one lane
 *   per point, with the knot scans and the interpolation of hv_restore_volume_sp (one device function serves both; knots, frame and
 *   cumulative lengths in LDS up to 630 knots, global memory beyond).
 *   direction = HV_CURVE_TO_LOCAL: out[m] = global_to_local(points[m] * spacing), points in voxel indices of the scan.
 *   direction = HV_CURVE_TO_GLOBAL: per knot n q = points[m] - (cumlen[n], centre1, centre2), to_plane = q[0], g = basis[n] q (summed over
 *     the frame's columns, einsum 'nij,nj->ni'), to_origin = |g|, coords = g + knots[n]; the same choice of idx and the same window and
 *     interpolation to to_plane = 0 as above; out[m] = that / spacing, in voxel indices of the scan.
 *   The local coordinate keeps the reference's order (cumulative length, offset along frame vector 1, offset along frame vector 2): the
 *   in-plane swap described above, which hv_restore_volume applies to index the crop, is NOT part of this entry; straight-volume index
 *   (n, a, b) is local (n, b, a).  A row whose result is not finite is NaN.  out may be points.
 *   HV_ERR_ARG: null pointer, M <= 0, N < 2, a non-positive or non-finite spacing, an unknown direction: nothing is launched or written. */
enum { HV_RESTORE_CROP = 0, HV_RESTORE_VERTEBRA = 1 };
enum { HV_CURVE_TO_LOCAL = 0, HV_CURVE_TO_GLOBAL = 1 };
int hv_restore_volume(const void* crop_ct, int crop_dtype, long long cs0, long long cs1, long long cs2, const uint8_t* crop_label,
                      long long ls0, long long ls1, long long ls2, int O0, int O1, int O2, const int* box, const double* knots,
                      const double* basis, const double* cumlen, int N, double centre1, double centre2, const void* patient_label,
                      int label_dtype, long long ps0, long long ps1, long long ps2, int D0, int D1, int D2, const int* region, int where,
                      int vert_id, double* ct_out, long long os0, long long os1, long long os2, uint8_t* label_out, long long qs0,
                      long long qs1, long long qs2, uint8_t* covered, long long vs0, long long vs1, long long vs2, double* local_out,
                      void* stream);
int hv_restore_volume_sp(const void* crop_ct, int crop_dtype, long long cs0, long long cs1, long long cs2, const uint8_t* crop_label,
                         long long ls0, long long ls1, long long ls2, int O0, int O1, int O2, const int* box, const double* knots,
                         const double* basis, const double* cumlen, int N, double centre1, double centre2, const void* patient_label,
                         int label_dtype, long long ps0, long long ps1, long long ps2, int D0, int D1, int D2, const int* region, int where,
                         int vert_id, double* ct_out, long long os0, long long os1, long long os2, uint8_t* label_out, long long qs0,
                         long long qs1, long long qs2, uint8_t* covered, long long vs0, long long vs1, long long vs2, double* local_out,
                         const double* spacing, void* stream);
int hv_curve_points(const double* points, long long M, const double* knots, const double* basis, const double* cumlen, int N, double centre1,
                    double centre2, const double* spacing, int direction, double* out, void* stream);

/* ---- cubic B-spline resampling (order 3) for the straightening and the restore (reference straighten/straighten/curve.py:77-102:
 * interpolate_along hands `order` to scipy.ndimage.map_coordinates, and map_coordinates(v, coords, order=3, mode='constant', cval=0) is a
 * prefilter, spline_filter(v, 3, mode='mirror') in float64, followed by a 4 x 4 x 4-tap sample) ----
 * hv_spline_prefilter: the float64 B-spline coefficients of a 3-D source [D0][D1][D2] (HV_DT_I16 / F32 / F64, element (i, j, k) at
 *   src[i*s0 + j*s1 + k*s2], strides in elements: a sub-box of a larger array is its first element's pointer and the array's strides) into
 *   coef, [D0][D1][D2] contiguous doubles.  `window`: every voxel is windowed (255 (v - win_min) / (win_max - win_min) clipped to [0, 255]) as
 *   it is first read, the reference's order (window the volume, then interpolate).  Along each axis in turn (0, 1, 2), with z = sqrt(3) - 2,
 *   every line c[0..n-1] is scaled by (1 - z)(1 - 1/z), then c[0] = (c[0] + z^(n-1) c[n-1] + sum_{i=1..n-2} (z^i + z^(2n-2-i)) c[i]) /
 *   (1 - z^(2n-2)), c[i] += z c[i-1], c[n-1] = z / (z^2 - 1) (c[n-1] + z c[n-2]), c[i] = z (c[i+1] - c[i]); a line of length 1 is left as
 *   it is.  For n > 32 the sum for c[0] stops after 32 terms (|z|^32 = 5e-19, below one rounding).  One lane per line, no atomics: the same
 *   input gives the same bits on every run.  Up to three launches, no workspace beyond coef (8 bytes per voxel: 839 MB for a 512 x 512 x 400
 *   scan).  HV_ERR_ARG: null pointer, non-positive size, another dtype, coef not 8-byte aligned; nothing is launched, nothing written.
 * Sampling a coefficient volume at u (all three coordinates inside [0, n - 1]; outside it the sample is 0 as for order 1): i = floor(u),
 *   t = u - i, taps i - 1 .. i + 2 with the cubic B-spline weights ((1-t)^3 / 6, (t^2 (t - 2) 3 + 4) / 6, ((1-t)^2 ((1-t) - 2) 3 + 4) / 6,
 *   the rest to 1), tap indices outside the line mirrored (-1 -> 1, n -> n - 2).  There is NO clipping: a cubic sample of windowed [0, 255]
 *   data may leave that interval, as it does in scipy.
 * hv_straighten_sample_spline: hv_straighten_sample_sp with the CT sampled cubically from coef = hv_spline_prefilter of the whole scan (the
 *   window fused in there).  Coordinates, the spacing division, the outside rule, the label, the presence bits and the output layout are the
 *   order-1 kernel's (one kernel template): straight_label and presence are bit-identical to hv_straighten_sample_sp's.  HV_ERR_ARG /
 *   HV_ERR_WORKSPACE as there.
 * hv_restore_volume_spline: hv_restore_volume_sp with the CT sampled cubically from crop_coef = hv_spline_prefilter of the crop's filled
 *   sub-box alone: source pointer at crop element (start0, start1, start2), sizes (len0, len1, len2) of the box row, the crop's strides; the
 *   mirror is at the sub-box's own edges and the crop's zero padding is never read.  The sample lies at c - start.  The covered rule, the
 *   label sample (from crop_label, [O0][O1][O2]), the write rules and local_out are unchanged.  knots == NULL is HV_ERR_ARG here: the
 *   single-centroid un-crop copies voxels (a cubic sample at a lattice point is the voxel itself), use hv_restore_volume_sp. */
int hv_spline_prefilter(const void* src, int dtype, long long s0, long long s1, long long s2, int D0, int D1, int D2, int window, double win_min,
                        double win_max, double* coef, void* stream);
int hv_straighten_sample_spline(const double* coef, const void* label, int label_dtype, long long ls0, long long ls1, long long ls2, int D0,
                                int D1, int D2, const double* knots, const double* basis, int N, int PA, int PB, double* straight_ct,
                                uint8_t* straight_label, uint64_t* presence, size_t presence_bytes, const double* spacing, void* stream);
int hv_restore_volume_spline(const double* crop_coef, const uint8_t* crop_label, long long ls0, long long ls1, long long ls2, int O0, int O1,
                             int O2, const int* box, const double* knots, const double* basis, const double* cumlen, int N, double centre1,
                             double centre2, const void* patient_label, int label_dtype, long long ps0, long long ps1, long long ps2, int D0,
                             int D1, int D2, const int* region, int where, int vert_id, double* ct_out, long long os0, long long os1,
                             long long os2, uint8_t* label_out, long long qs0, long long qs1, long long qs2, uint8_t* covered, long long vs0,
                             long long vs1, long long vs2, double* local_out, const double* spacing, void* stream);

/* ---- generation-quality evaluation of a synthesized volume (reference evaluation/generation_eval_sagittal.py:11-37 calculate_iou /
 * calculate_dice / relative_volume_difference, :39-103 process_images; generation_eval_coronal.py the same with the slice axis 1; SURVEY.md
 * row 17).  Four [H][W][Z] volumes: element (h, w, z) of the CTs at base[h*cs0 + w*cs1 + z*cs2], of the labels
 * at base[h*ls0 + w*ls1 + z*ls2] (strides in elements, any order); ct_dtype HV_DT_F32 / F64, label_dtype HV_DT_U8 / F32 / F64; all
 * arithmetic in float64.  view 2 = sagittal (slices [:, :, z]), 1 = coronal ([:, z, :]).  ori = (ori_seg == label), fake = (fake_seg == label).
 * Slices z0..z1 (the ori's extent along the view axis), n = z1 - z0 + 1, m = (4n)//5, evaluated: z in [z0 + (n - m)//2, +m) whose ori has
 * more than 400 voxels.  Per evaluated slice: rows x1..x2 (the ori's first / last row) x the whole other axis is the patch; PSNR
 * 10 log10(R^2 / mean squared error) and SSIM (scikit-image 0.22: 7x7 uniform window, covariance 49/48, C1 (0.01 R)^2, C2 (0.03 R)^2,
 * 3-pixel border cropped) of the patch and of the whole slice, R = max - min of the ori CT over the patch / slice.
 * out[16]: [0] global psnr, [1] global ssim, [2] patch psnr, [3] patch ssim (means over the evaluated slices of the non-NaN values, 0 if
 * none), [4] iou, [5] rv_diff, [6] dice (exact integer counts), [7] 1 if the ori is empty (the reference raises), [8] 1 if an evaluated
 * slice's patch or side is shorter than 7 (structural_similarity raises), [9] evaluated slices, [10..12] |ori|, |fake|, |ori & fake|,
 * [13] z0, [14] z1, [15] records written.  slices (NULL or 9 doubles per slice along the view axis): per slice of the 4/5 range in order
 * { z, x1, x2, R_patch, R_global, psnr_patch, ssim_patch, psnr_global, ssim_global }, z = -1 where the slice is not evaluated.  ori_ct = fake_ct = NULL: the counts and [4..12]
 * only.  No host synchronisation; workspace 16-byte aligned, hv_gen_eval_workspace_bytes bytes. */
size_t hv_gen_eval_workspace_bytes(int H, int W, int Z, int view);
int hv_gen_eval(const void* ori_ct, const void* fake_ct, int ct_dtype, long long cs0, long long cs1, long long cs2, const void* ori_seg,
                const void* fake_seg, int label_dtype, long long ls0, long long ls1, long long ls2, int H, int W, int Z, int view, double label,
                double* out, double* slices, void* workspace, size_t workspace_bytes, void* stream);
/* The same for a set, as the reference's main() (:124-162) scores it: N originals, each against E synthesized volumes (one per experiment
 * folder), in one launch sequence whose length does not depend on N or E.  ori_ct / ori_seg: DEVICE tables of N device pointers; fake_ct /
 * fake_seg: device tables of N * E device pointers, item i's experiment e at [i * E + e]; labels: device array of N vertebra ids.  Every
 * volume of a call has the shape, the two dtypes and the two stride triples of the call (rules as above); ori_ct = fake_ct = NULL: the
 * counts only.  out [N][E][16] and slices (NULL or [N][E][S][9], S the extent of the view axis) in hv_gen_eval's field layout, each pair's
 * values the SAME BITS hv_gen_eval gives for that pair alone: the kernels share its device functions and its summation orders, whatever N,
 * E and the order of items and experiments are.  What depends on the original alone (its counts, z0 / z1, the selection, x1 / x2, both data
 * ranges, the SSIM window sums of x and x^2) is computed once per item.  A pair's [7] / [8] flags concern that pair's item only.
 * HV_ERR_ARG: hv_gen_eval's conditions, N < 1, E < 1, labels NULL, a workspace that is NULL, not 16-byte aligned or smaller than
 * hv_gen_eval_batch_workspace_bytes(H, W, Z, view, N, E); HV_ERR_UNSUPPORTED: N * E > 65535.  Nothing is launched on an error.  No host
 * synchronisation. */
size_t hv_gen_eval_batch_workspace_bytes(int H, int W, int Z, int view, int N, int E);
int hv_gen_eval_batch(const void* const* ori_ct, const void* const* fake_ct, int ct_dtype, long long cs0, long long cs1, long long cs2,
                      const void* const* ori_seg, const void* const* fake_seg, int label_dtype, long long ls0, long long ls1, long long ls2,
                      int H, int W, int Z, int view, const double* labels, int N, int E, double* out, double* slices, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- SVM grading of the RHLV features at every point of a parameter grid (reference evaluation/SVM_grading.py:21-52,63-71 and
 * evaluation/SVM_grading_2.5d.py:33-59: StandardScaler fitted on the train + test rows, SVC(kernel='linear', class_weight='balanced'),
 * StratifiedKFold(5), each fold's model applied to the val rows, confusion matrix / macro F1 / precision / recall / accuracy per fold, their
 * mean and np.var over the folds).  Float64 throughout, every reduction in a fixed order: a grid point's results
 * are the same bits whether it is graded alone or inside a larger grid.  No workspace (the scaler is fused into the kernels' staging).
 * hv_svm_grade_plan: HOST arithmetic only, nothing is launched.  y_tt [M] / y_val [Mv]: the grades of the train + test / val rows, classes [K]:
 *   the sorted (strictly increasing, non-negative) list of all grades, fold [M]: the test fold (0..4) of every train + test row (the unshuffled
 *   StratifiedKFold assignment; it depends on the labels only).  Writes into `plan` (host memory, hv_svm_grade_plan_bytes(M, Mv) bytes) what
 *   the kernels read: per fold and class the bound on alpha n_train / (n_classes_in_train * count(class)) (class_weight='balanced', C = 1) and
 *   whether the class occurs in the fold's training rows, the class index of every row, the fold ids; *max_rows = the largest number of
 *   training rows of one class pair in one fold.  The caller uploads the plan as it is.  HV_ERR_ARG: null pointer, non-positive size, a
 *   fold id outside 0..4, classes not sorted, a grade that is not in classes; HV_ERR_UNSUPPORTED: K < 2, K > HV_SVM_MAX_CLASSES, *max_rows >
 *   HV_SVM_MAX_ROWS (the solver keeps a pair's rows in LDS: (F + 4) * 8 bytes per row, 1792 rows x 80 B = 140 KiB of the 160 KiB);
 *   HV_ERR_WORKSPACE: plan_bytes too small.
 * hv_svm_grade_grid: X_tt [G][M][F], X_val [G][Mv][F] (device, F = 3 or 6), plan (device copy of the plan), max_rows as the plan call gave it.
 *   One wave per (class pair, fold, grid point) solves libsvm's C-SVC dual of that pair's training rows (the +1 side is the lower class) by
 *   SMO -- maximal violating pair with the second-order choice of the second row, ties to the lowest row -- until the KKT gap m(alpha) -
 *   M(alpha) <= tol or max_iter iterations; one wave per (fold, grid point) then votes in libsvm's way (a decision w.x - b > 0 votes for the
 *   pair's lower class, ties among the vote counts go to the lowest class, classes absent from the fold's training rows are never predicted)
 *   and scores by scikit-learn's rule (macro averages over the classes that occur in y_val or in the predictions; an empty denominator
 *   contributes 0).  With P = K (K - 1) / 2 pairs in the order (0,1), (0,2), ..., (K-2,K-1) of class indices:
 *   w [G][5][P][F], b [G][5][P] (libsvm's rho: decision = w.x - b), gap [G][5][P] (the final KKT gap), info [G][5][P][4] = { iterations, status,
 *   support vectors, rows }, pred [G][5][Mv] (class index; -1 for an unusable grid point), confusion [G][5][K][K] (true class x predicted class),
 *   scores [G][5][4] = { F1, precision, recall, accuracy }, mean / var [G][4] over the folds (ddof 0), unusable [G] (1: a feature of that grid
 *   point is not finite -- nothing is solved, scores / mean / var are NaN, the other grid points are not affected), decision (NULL or
 *   [G][5][Mv][P]; NaN for a pair that was not solved).  A problem that hit max_iter is voted with what it has; its status says so.
 *   HV_ERR_ARG: null pointer (decision excepted), non-positive size, max_iter < 1, tol <= 0; HV_ERR_UNSUPPORTED: F not 3 or 6, K < 2 or >
 *   HV_SVM_MAX_CLASSES, max_rows > HV_SVM_MAX_ROWS, G > 65535.  In both cases nothing is launched and nothing is written. */
enum { HV_SVM_FOLDS = 5, HV_SVM_MAX_CLASSES = 4, HV_SVM_MAX_ROWS = 1792 };
enum { HV_SVM_CONVERGED = 0, HV_SVM_MAX_ITER = 1, HV_SVM_ABSENT = 2 /* a class of the pair is missing from the fold's training rows */,
       HV_SVM_UNUSABLE = 3 /* non-finite feature at that grid point */, HV_SVM_BAD_PLAN = 4 /* the plan does not belong to these sizes */ };
size_t hv_svm_grade_plan_bytes(int M, int Mv);
int hv_svm_grade_plan(const int* y_tt, const int* fold, int M, const int* y_val, int Mv, const int* classes, int K, void* plan,
                      size_t plan_bytes, int* max_rows);
int hv_svm_grade_grid(const double* X_tt, const double* X_val, const void* plan, int G, int M, int Mv, int F, int K, int max_rows, double tol,
                      int max_iter, double* w, double* b, double* gap, int* info, int* pred, int* confusion, double* scores, double* mean,
                      double* var, int* unusable, double* decision, void* stream);

/* ---- fit the grader at one chosen setting, keep the model, grade rows that were not in the table ----
 * The same scaler, solver and vote as hv_svm_grade_grid (one solver body and one row-vote body in csrc/svm_grade.hip, called by both): a fit on
 * the rows `fold != f` of a table gives bit for bit that call's w, b, gap and info of fold f, and hv_svm_predict of that model on the val rows its
 * pred and decision.  Float64, fixed-order reductions, no workspace; a grid point's bytes do not depend on G or on its place in the grid.
 * hv_svm_fit_plan: HOST arithmetic only.  y [M]: the grade of every row, train [M] (NULL = every row): non-zero = the row enters the solver,
 *   classes [K] sorted, strictly increasing, non-negative.  Writes into `plan` (host, hv_svm_fit_plan_bytes(M) bytes): the bound on alpha per class
 *   n_train / (n_classes_in_train * count(class)) over the train rows (0 for a class without train rows), present [K], the class index and the
 *   train flag of every row; *max_rows = the train rows of the largest class pair.  HV_ERR_ARG: null pointer, M <= 0, classes not sorted, a grade
 *   not in classes; HV_ERR_UNSUPPORTED: K outside 2..HV_SVM_MAX_CLASSES, *max_rows > HV_SVM_MAX_ROWS (then *max_rows is still set);
 *   HV_ERR_WORKSPACE: plan_bytes too small.  A refusal leaves `plan` untouched.
 * hv_svm_fit: X [G][M][F] (device, F = 3 or 6), plan (device copy).  One wave per (class pair, grid point): StandardScaler over ALL M rows of the
 *   grid point (the reference scales before it splits), then the C-SVC dual of the pair's train rows, the lower class first, each class in row
 *   order.  mean, scale [G][F], w [G][P][F], b, gap [G][P], info [G][P][4] = { iterations, status, support vectors, rows }.  A non-finite feature
 *   among the M rows: every pair of that grid point reports HV_SVM_UNUSABLE and its w, b, mean, scale are NaN; the other grid points are not
 *   affected.  HV_SVM_ABSENT: a class of the pair has no train row.
 * hv_svm_predict: X [G][N][F] (device), present [K] (device: the plan's present flags), the model of hv_svm_fit.  One lane per row:
 *   pred [G][N] the class index, -1 where the row has a non-finite feature, the model is unusable or no class is present; decision [G][N][P]
 *   (w.x_scaled - b, NaN for a pair that was not solved), votes [G][N][K], contrib [G][N][P][F] = w[p][c] * x_scaled[c] -- its sum in column
 *   order minus b is the decision, bit for bit.  decision, votes, contrib may be NULL.  A bad row has pred -1, NaN decision and contrib, zero
 *   votes and touches nothing else.
 * hv_svm_features: records [N][2][16] (what hv_rhlv_views_batch leaves on the device, both views) -> X [N][F]: columns 1..3 of view first_view
 *   (0 sagittal, 1 coronal), with F = 6 followed by the other view's.  The row is NaN where the original lacks the vertebra (sagittal [13] == 0)
 *   or the coronal script would have raised (coronal [14] != 0).
 * All three device entries refuse before any launch -- HV_ERR_ARG: null required pointer, G, M or N <= 0, tol <= 0, max_iter < 1, first_view not
 * 0 / 1; HV_ERR_UNSUPPORTED: F not 3 or 6, K outside 2..HV_SVM_MAX_CLASSES, max_rows > HV_SVM_MAX_ROWS, G > 65535. */
size_t hv_svm_fit_plan_bytes(int M);
int hv_svm_fit_plan(const int* y, const int* train, int M, const int* classes, int K, void* plan, size_t plan_bytes, int* max_rows);
int hv_svm_fit(const double* X, const void* plan, int G, int M, int F, int K, int max_rows, double tol, int max_iter, double* mean, double* scale,
               double* w, double* b, double* gap, int* info, void* stream);
int hv_svm_predict(const double* X, int G, int N, int F, int K, const int* present, const double* mean, const double* scale, const double* w,
                   const double* b, const int* info, int* pred, double* decision, int* votes, double* contrib, void* stream);
int hv_svm_features(const double* records, int N, int first_view, int F, double* X, void* stream);

/* ---- exact Euclidean distance transform and the surface-distance metrics on it (csrc/edt.hip).  The reference has
 * no such metric: the transform is scipy.ndimage.distance_transform_edt, the metric definitions are MedPy's (metric.binary hd / hd95 / asd / assd).
 * hv_edt: vol [A0][A1][A2], element (i, j, k) at vol[i*s0 + j*s1 + k*s2] (strides in elements, any order), dtype HV_DT_U8 / F32 / F64.  T = {vol ==
 *   value}.  out (device, [A0][A1][A2] contiguous doubles): the distance of every voxel to the nearest voxel of T with the axes scaled by spacing[3]
 *   (HOST pointer, copied into the kernel arguments), i.e. distance_transform_edt(vol != value, sampling=spacing).  One pass per axis over squared
 *   distances: integers at unit spacing (int32 in the workspace while A0^2 + A1^2 + A2^2 < 2^31, else int64 in out's own slots), else the double sum
 *   ((s0 d0)^2 + (s1 d1)^2) + (s2 d2)^2; one correctly rounded square root per voxel.  box (HOST, NULL = the whole volume): { lo0, lo1, lo2, n0, n1,
 *   n2 } limits both the voxels written and the part of T considered; out is not touched outside it.  status (device int): 1 if T (inside the box)
 *   is empty -- every voxel written is then +inf -- else 0.  workspace: 16-byte aligned, hv_edt_workspace_bytes(A0, A1, A2) bytes.
 *   HV_ERR_ARG: a NULL pointer (box excepted), a non-positive size, an unknown dtype, a spacing that is not positive and finite, a box that is
 *   empty or leaves the volume, out not 8-byte or workspace not 16-byte aligned, a workspace smaller than queried; HV_ERR_UNSUPPORTED: an A1 or A2
 *   line above 64 KiB of carried values (16 384 at unit spacing, 8 192 otherwise), more than 2^30 voxels.  Nothing is launched or written then.
 * hv_surface_distance: a, b label volumes of one shape, dtype and stride triple (rules as above); A = {a == value}, B = {b == value}.  A voxel of a
 *   set is a surface voxel if one of its six face neighbours is not in the set, a neighbour outside the volume counting as such (X & ~binary_erosion(
 *   X, generate_binary_structure(3, 1), border_value=0)).  out[16] (device): [0] n_a, [1] n_b the surface counts, [2] max_ab = max over p in S_A of
 *   d(p, S_B), [3] max_ba, [4] asd_ab, [5] asd_ba the directed means, [6] hd = max([2], [3]), [7] hd95 = the 95th percentile (numpy's linear rule:
 *   v = (n - 1) 0.95, lo / hi the order statistics floor(v) and floor(v) + 1, t = v - floor(v), lo + (hi - lo) t for t < 0.5, else hi - (hi - lo)
 *   (1 - t)) of both directed lists joined, [8] assd = ([4] + [5]) / 2, [9] 1 if S_A is empty, [10] 1 if S_B is empty (then [2..8] are NaN),
 *   [11..15] 0.  restricted 1: the two transforms run inside the bounding box of A | B, found on the device (every surface voxel lies inside it, so
 *   the distances are exact); 0: over the whole volume; the 16 doubles are the same bits either way.  Sums are per-slice partials (axis 0) folded in
 *   ascending order by one lane: the same bits on every run.  No host synchronisation; workspace 16-byte aligned,
 *   hv_surface_distance_workspace_bytes bytes.  HV_ERR_ARG / HV_ERR_UNSUPPORTED as for hv_edt, and HV_ERR_ARG for restricted other than 0 / 1. */
size_t hv_edt_workspace_bytes(int A0, int A1, int A2);
int hv_edt(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, double value, const double* spacing,
           const int* box, double* out, int* status, void* workspace, size_t workspace_bytes, void* stream);
size_t hv_surface_distance_workspace_bytes(int A0, int A1, int A2);
int hv_surface_distance(const void* a, const void* b, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, double value,
                        const double* spacing, int restricted, double* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- 3-D connected components of a volume, and the clean-up of a synthesized label volume on them (csrc/ccl3d.hip).
 * The reference filters components per 2-D slice only (hv_slice_components, hv_depedicle); these are scipy.ndimage.label / binary_fill_holes.
 * The volume is described as for hv_edt: vol [A0][A1][A2], element (i, j, k) at vol[i*s0 + j*s1 + k*s2] (strides in elements, any order), dtype
 * HV_DT_U8 / F32 / F64.  Foreground: vol == value (mode HV_CCL_EQ) or vol != value (HV_CCL_NE; with value 0 scipy's label(vol)).  connectivity
 * 1 / 2 / 3 = generate_binary_structure(3, c): 6, 18 or 26 neighbours.
 * hv_label3d: labels (device, contiguous int32 [A0][A1][A2]): 0 = background, 1..n the components in ascending order of the smallest raster index
 *   (i*A1 + j)*A2 + k of their voxels -- scipy.ndimage.label's numbering.  table (device int32 [4 + table_cap]): [0] n, [1] the label of the largest
 *   component (equal sizes: the lowest label, np.argmax(np.bincount(labels.ravel())[1:]) + 1; 0 if n = 0), [2] its size, [3] status (bit 0: no
 *   foreground voxel), [4 + i] the size of component i + 1 for i < min(n, table_cap) and 0 from n on.  [0..2] are exact whatever table_cap (>= 0) is.
 *   Tiles of hv_label3d_tile's shape are labelled in LDS, their seams joined by lock-free unions in global memory, the roots ranked by a prefix
 *   sum, the sizes counted by integer atomics: the same bytes on every run.  No host synchronisation.
 * hv_clean_components: out (dtype of vol, strides os0..os2) = vol with the foreground voxels of dropped components set to `fill`; every other voxel
 *   is copied unchanged.  A component is kept iff it has >= min_size voxels (min_size <= 1: no size rule; the reference's rule drops < min_size) and,
 *   with keep_largest = 1, is the largest one ([1] above).  out may be vol itself with the same strides: the launch that writes out then does not
 *   read vol.  table (device int32 [4]): [0..3] as above, of the labelling before the filter.
 * hv_fill_holes: the voxels that are not foreground and from which no face of the volume is reached through 6-connected non-foreground voxels
 *   become `fill` in out (scipy.ndimage.binary_fill_holes with the default structure); everything else is copied, out as above.  table (device
 *   int32 [4]): [0] the number of holes (6-connected components filled), [2] the voxels filled, [1] and [3] 0.
 * hv_label3d_tile (host only): dims[3] = the tile shape of the first pass.  hv_label3d_workspace_bytes: the workspace of all three entries, 16-byte
 *   aligned: 4 bytes per voxel of parents, 4 per voxel + 4 of sizes, 4 per voxel of labels (used by the two clean-ups), 4 per 1 024 voxels of
 *   block counts, each of the four rounded up to 16, + 16: 12 bytes per voxel in all.
 * Refusals, before any launch and with nothing written -- HV_ERR_ARG: a NULL pointer, a non-positive size, an unknown dtype or mode, connectivity
 *   outside 1..3, keep_largest other than 0 / 1, table_cap < 0, labels or table not 4-byte aligned, a workspace that is not 16-byte aligned or smaller
 *   than queried, out == vol with other strides; HV_ERR_UNSUPPORTED: more than 2^30 voxels (raster indices are int32). */
enum { HV_CCL_EQ = 0, HV_CCL_NE = 1 };
size_t hv_label3d_workspace_bytes(int A0, int A1, int A2);
int hv_label3d_tile(int* dims);
int hv_label3d(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, double value, int mode,
               int connectivity, int* labels, int* table, int table_cap, void* workspace, size_t workspace_bytes, void* stream);
int hv_clean_components(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, double value, int mode,
                        int connectivity, int min_size, int keep_largest, double fill, void* out, long long os0, long long os1, long long os2,
                        int* table, void* workspace, size_t workspace_bytes, void* stream);
int hv_fill_holes(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, double value, int mode, double fill,
                  void* out, long long os0, long long os1, long long os2, int* table, void* workspace, size_t workspace_bytes, void* stream);

/* ---- 3-D binary morphology of a volume, and a mask written back into a label volume (csrc/morph.hip).  The reference
 * only dilates 2-D masks (skimage dilation(seg, square(2)) in its cv2 mask scripts); these are scipy.ndimage.binary_dilation / binary_erosion /
 * binary_opening / binary_closing, bit for bit.  The volume is described as for hv_label3d: vol [A0][A1][A2], element (i, j, k) at vol[i*s0 + j*s1 +
 * k*s2] (strides in elements, any order), dtype HV_DT_U8 / F32 / F64, foreground vol == value (HV_CCL_EQ) or vol != value (HV_CCL_NE).  out: a
 * uint8 mask of 0 / 1, element (i, j, k) at out[i*os0 + j*os1 + k*os2]; it must not overlap vol.  op: HV_MORPH_DILATE / ERODE / OPEN (erosion then
 * dilation) / CLOSE (dilation then erosion); border_value 0 / 1 is what the voxels outside the volume hold, in both halves of a compound op.
 * hv_morph_ball: the structuring element is the set of integer offsets o with ((s0 o0)^2 + (s1 o1)^2) + (s2 o2)^2 <= radius * radius, float64 in
 *   this order (hv_edt's ordered sum), s = spacing[3] (HOST pointer); radius 0 is the identity.  One pass per axis; no distance is formed: the
 *   passes carry the step count to the nearest member along axis 0 and the remaining reach along axis 2 (uint8 while both stay <= 254 steps, else
 *   uint16), every line scan is bounded by the largest step count d with (s_a d)^2 <= radius^2, the erosion is the dilation of the complement.
 * hv_morph_struct: the structuring element is generate_binary_structure(3, connectivity) (7 / 19 / 27 cells), applied `iterations` times; OPEN /
 *   CLOSE run `iterations` times the first half, then `iterations` times the second (scipy's iterations=).  One launch per iteration: a 3 x 3 x 3
 *   stencil over a tile of hv_morph_tile's shape with a one-voxel halo in LDS.  iterations < 1 (scipy: until nothing changes) is refused.
 * hv_morph_merge: out (dtype of vol, strides os0..os2) = vol with a mask (uint8, strides ms0..ms2, set = non-zero) written back.  HV_MORPH_GROW
 *   (after a dilation / closing): a voxel whose mask is set and whose value is `background` becomes `value`; HV_MORPH_SHRINK (after an erosion /
 *   opening): a voxel that holds `value` and whose mask is 0 becomes `fill`.  Every other voxel is copied bit for bit, so other labels are never
 *   overwritten.  out may be vol itself with the same strides.
 * hv_morph_tile (host only): dims[3] = the stencil's tile shape.  hv_morph_workspace_bytes (host only; spacing NULL = {1, 1, 1}): the workspace of
 *   hv_morph_ball at that radius -- one count per voxel (1 or 2 bytes) and one byte per voxel of intermediate mask, each rounded up to 16; with
 *   radius 0 (2 bytes per voxel) it is what hv_morph_struct needs.  0 for arguments hv_morph_ball refuses.
 * No host synchronisation, no atomics; the same bytes on every run, whatever the workspace held.  Refusals, before any launch and with nothing
 * written -- HV_ERR_ARG: a NULL pointer, a non-positive size, an unknown dtype, mode, op or rule, border_value other than 0 / 1, a radius that is
 *   negative, not finite or whose square is not finite, a spacing that is not positive and finite, iterations < 1, connectivity outside 1..3, a
 *   workspace that is not 16-byte aligned or smaller than queried, out == vol with other strides (merge); HV_ERR_UNSUPPORTED: more than 2^30
 *   voxels; hv_morph_ball only: A1 or A2 above 32 768 (a line of 16-bit counts must fit 64 KiB of LDS), a reach above 65 534 steps along axis 0
 *   or 2 (radius / spacing, capped by the extent). */
enum { HV_MORPH_DILATE = 0, HV_MORPH_ERODE = 1, HV_MORPH_OPEN = 2, HV_MORPH_CLOSE = 3 };
enum { HV_MORPH_GROW = 0, HV_MORPH_SHRINK = 1 };
size_t hv_morph_workspace_bytes(int A0, int A1, int A2, double radius, const double* spacing);
int hv_morph_tile(int* dims);
int hv_morph_ball(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, double value, int mode, int op,
                  double radius, const double* spacing, int border_value, void* out, long long os0, long long os1, long long os2, void* workspace,
                  size_t workspace_bytes, void* stream);
int hv_morph_struct(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, double value, int mode, int op,
                    int connectivity, int iterations, int border_value, void* out, long long os0, long long os1, long long os2, void* workspace,
                    size_t workspace_bytes, void* stream);
int hv_morph_merge(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, const void* mask, long long ms0,
                   long long ms1, long long ms2, int rule, double value, double background, double fill, void* out, long long os0, long long os1,
                   long long os2, void* stream);

/* ---- per-label intensity statistics and order statistics of volumes (csrc/labelstats.hip).  The reference has no
 * counterpart: the definitions are scipy.ndimage.sum_labels / minimum / maximum / center_of_mass / find_objects and np.percentile (linear).
 * hv_label_stats: vol holds V intensity volumes [V][A0][A1][A2], element (v; i, j, k) at vol[v*sv + i*s0 + j*s1 + k*s2] (strides in elements, any
 *   order), vol_dtype HV_DT_U8 / I16 / F32 / F64.  label: the same logical shape with its own strides, any HV_DT_* code, values integers in [0, 255]
 *   as for hv_straighten_stats; a voxel whose label is not such a value sets HV_LS_BAD_LABEL in every record of its volume and is counted nowhere.
 *   mask (may be NULL): uint8 with its own strides; a voxel counts only where mask != 0.  labels[S] (HOST, 1 <= S <= HV_LS_MAX_LABELS, distinct
 *   values in [0, 255], 0 allowed) and q[Q] (HOST, 0 <= Q <= HV_LS_MAX_Q percentiles in [0, 100]; may be NULL for Q = 0) are copied into the kernel
 *   arguments.  out (device, 8-byte aligned): [V][S][HV_LS_REC] doubles, per (volume, listed label):
 *     [HV_LS_COUNT] the voxel count n; [HV_LS_SUM], [HV_LS_SUMSQ] the sums of v and of v*v -- for U8 / I16 the EXACT int64 sums, stored as the
 *     int64's bit pattern in the double's slot (2^30 voxels x 32768^2 = 2^60 keeps the squares inside int64); for F32 / F64 doubles, the sum of
 *     (double)v and of fl((double)v * (double)v) in an order fixed by the shape (16^3 tiles in raster order; the strides do not enter);
 *     [HV_LS_MIN], [HV_LS_MAX] (+inf / -inf for n = 0); [HV_LS_COORD + a] the sum of index a over the voxels, an exact integer while n * (A_a - 1)
 *     <= 2^53 (every volume with A_a <= 2^23); [HV_LS_LO + a], [HV_LS_HI + a] the inclusive bounding box (n = 0: lo = A_a, hi = -1);
 *     [HV_LS_STATUS] the OR of HV_LS_BAD_LABEL, HV_LS_NONFINITE (a NaN or +-inf met inside this label: it is still counted, summed and ranked by
 *     its key, so the floating fields are meaningless), HV_LS_EMPTY (n = 0); [HV_LS_STATUS + 1] 0; [HV_LS_ORDER + 2t], [HV_LS_ORDER + 2t + 1] for
 *     t < Q the order statistics x[lo], x[hi] of the label's values with vi = (n - 1) * (q[t] / 100) in float64 (numpy's virtual index), lo =
 *     floor(vi), hi = lo + 1, and lo = hi = n - 1 once vi >= n - 1; NaN for n = 0.  The fields from HV_LS_ORDER + 2Q on are NOT written.
 *   Order statistics come from a radix select over an order-preserving key (16 bits for U8 / I16, 32 for F32, 64 for F64: 2 / 4 / 8 passes over
 *   the volumes, none for Q = 0); -0.0 sorts below +0.0.  Only integer atomics; floating sums have a fixed order: the same bytes on every run,
 *   for any strides, single or stacked, whatever the workspace held.  No host synchronisation.  workspace: 16-byte aligned,
 *   hv_label_stats_workspace_bytes(V, A0, A1, A2, S, Q) bytes (0 for sizes the entry refuses).
 *   Refusals, before any launch and with nothing written -- HV_ERR_ARG: a NULL pointer (mask excepted; q for Q = 0), a non-positive size, an
 *   unknown dtype, S outside 1..HV_LS_MAX_LABELS, Q outside 0..HV_LS_MAX_Q, a label value outside [0, 255] or listed twice, a q outside [0, 100]
 *   or not finite, out not 8-byte aligned, a workspace that is not 16-byte aligned or smaller than queried; HV_ERR_UNSUPPORTED: more than 2^30
 *   voxels per volume, V > 65535. */
enum { HV_LS_REC = 32, HV_LS_MAX_LABELS = 64, HV_LS_MAX_Q = 8 };
enum { HV_LS_COUNT = 0, HV_LS_SUM = 1, HV_LS_SUMSQ = 2, HV_LS_MIN = 3, HV_LS_MAX = 4, HV_LS_COORD = 5, HV_LS_LO = 8, HV_LS_HI = 11, HV_LS_STATUS = 14,
       HV_LS_ORDER = 16 };
enum { HV_LS_BAD_LABEL = 1, HV_LS_NONFINITE = 2, HV_LS_EMPTY = 4 };
size_t hv_label_stats_workspace_bytes(int V, int A0, int A1, int A2, int S, int Q);
int hv_label_stats(const void* vol, int vol_dtype, long long sv, long long s0, long long s1, long long s2, const void* label, int label_dtype,
                   long long lsv, long long ls0, long long ls1, long long ls2, const void* mask, long long msv, long long ms0, long long ms1,
                   long long ms2, int V, int A0, int A1, int A2, const int* labels, int S, const double* q, int Q, double* out, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ---- per-label 3-D grey-level co-occurrence matrices of volumes (csrc/texture.hip).  The reference has no
 * counterpart: the definition is Haralick's (1973), skimage.feature.graycomatrix carried to three dimensions and restricted to a label.
 * hv_glcm: vol, vol_dtype and strides, label, label_dtype and strides, mask and strides, V, A0..A2 and labels[S] exactly as for hv_label_stats
 *   (vol HV_DT_U8 / I16 / F32 / F64; a label value that is no integer in [0, 255] sets HV_LS_BAD_LABEL for its whole volume and has no slot).
 *   The SLOT of a voxel p is the s with label(p) == labels[s] if mask is NULL or mask(p) != 0; otherwise it has none.  Its LEVEL: x = (double)v;
 *   a non-finite x takes the voxel out of every pair and ORs HV_LS_NONFINITE into info[v][s][0] of the slot it would have had; otherwise
 *   t = (x - lo) / width, those two IEEE float64 operations (no contraction, no reciprocal), and the level is 0 if t < 0, G - 1 if t >= G, else
 *   (int)t.  offsets (HOST, [D][3] ints, 1 <= D <= HV_GLCM_MAX_OFFSETS, every component in [-HV_GLCM_MAX_REACH, HV_GLCM_MAX_REACH], no offset
 *   twice; (0, 0, 0) allowed: the slot's level histogram on the diagonal) are copied into the kernel arguments.  G in 2..HV_GLCM_MAX_LEVELS.
 *   out (device, 8-byte aligned): [V][S][D][G][G] int64.  For every offset d and every voxel p with p + d inside the volume and
 *   slot(p) == slot(p + d) == s: out[v][s][d][level(p)][level(p + d)] += 1, and with HV_GLCM_SYMMETRIC in flags also
 *   out[v][s][d][level(p + d)][level(p)] += 1 (P + P^T, the diagonal doubled, as graycomatrix(symmetric=True)).  No boundary modes: a pair that
 *   leaves the volume is not counted.  info (device, 8-byte aligned): [V][S][HV_GLCM_INFO] int64 -- [0] the OR of HV_LS_BAD_LABEL,
 *   HV_LS_NONFINITE, HV_LS_EMPTY (no finite voxel in the slot); [1] the number of finite voxels of the slot; [2] how many of them were clamped
 *   from below (t < 0); [3] how many from above (t >= G).
 *   The entry zeroes out and info itself on the stream.  Only integer atomics: the same bytes on every run, for any strides, single or stacked,
 *   whatever out, info and the workspace held.  No host synchronisation.  workspace: 16-byte aligned, hv_glcm_workspace_bytes(V, A0, A1, A2,
 *   S, D, G) bytes (0 for sizes the entry refuses).
 *   Refusals, before any launch and with nothing written -- HV_ERR_ARG: a NULL pointer (mask excepted), a non-positive size, an unknown dtype, S
 *   outside 1..HV_LS_MAX_LABELS, D outside 1..HV_GLCM_MAX_OFFSETS, G outside 2..HV_GLCM_MAX_LEVELS, a label value outside [0, 255] or listed
 *   twice, an offset component beyond HV_GLCM_MAX_REACH, an offset listed twice, lo not finite, width not finite or not > 0, unknown flag bits,
 *   out or info not 8-byte aligned, a workspace that is not 16-byte aligned or smaller than queried; HV_ERR_UNSUPPORTED: more than 2^30 voxels
 *   per volume, V > 65535. */
enum { HV_GLCM_MAX_LEVELS = 64, HV_GLCM_MAX_OFFSETS = 26, HV_GLCM_MAX_REACH = 4, HV_GLCM_INFO = 4 };
enum { HV_GLCM_SYMMETRIC = 1 };
size_t hv_glcm_workspace_bytes(int V, int A0, int A1, int A2, int S, int D, int G);
int hv_glcm(const void* vol, int vol_dtype, long long sv, long long s0, long long s1, long long s2, const void* label, int label_dtype,
            long long lsv, long long ls0, long long ls1, long long ls2, const void* mask, long long msv, long long ms0, long long ms1,
            long long ms2, int V, int A0, int A1, int A2, const int* labels, int S, const int* offsets, int D, double lo, double width, int G,
            int flags, long long* out, long long* info, void* workspace, size_t workspace_bytes, void* stream);

/* ---- per-label 3-D grey-level run-length matrices, dependence matrices and neighbourhood grey-tone sums of volumes (csrc/texture_runs.hip;
 * DESIGN.md section 8 row f21).  The reference has no counterpart: the definitions are Galloway's (1975) for run lengths, Sun and Wee's (1983)
 * for dependence and Amadasun and King's (1989) for the neighbourhood grey-tone difference, in the forms the pyradiomics documentation gives,
 * in three dimensions and restricted to a label.
 * Both entries: vol, vol_dtype and strides, label, label_dtype and strides, mask and strides, V, A0..A2, labels[S], lo, width and G exactly as
 *   for hv_glcm, and so are the SLOT and the LEVEL of a voxel, HV_LS_NONFINITE, HV_LS_BAD_LABEL and info[v][s][0..3].  Two voxels are ALIKE if
 *   both lie inside the volume, both have a slot, the same one, and both have the same level (a non-finite voxel has no slot here).
 *   Both zero their outputs and info themselves on the stream.  Only integer atomics: the same bytes on every run, for any strides, single or
 *   stacked, whatever the outputs, info and the workspace held.  No host synchronisation.  workspace: 16-byte aligned, the queried bytes (the
 *   per-volume bad-label words and one 16-bit code per voxel; 0 for sizes the entry refuses).
 * hv_glrlm: offsets (HOST, [D][3] ints, 1 <= D <= HV_GLRLM_MAX_OFFSETS, every component in {-1, 0, 1}, no offset (0, 0, 0), none listed twice and
 *   none beside its negative: d and -d give the same runs) are copied into the kernel arguments.  R >= 1: the run-length bins.  A RUN along d is
 *   a maximal sequence p, p + d, ..., p + (L - 1) d of voxels that have a slot and are pairwise alike: p - d is not alike p, p + L d is not
 *   alike p.  out (device, 8-byte aligned): [V][S][D][G][R] int64; for every run out[v][s][d][level][min(L, R) - 1] += 1.  info (device, 8-byte
 *   aligned): [V][S][HV_GLRLM_INFO] int64 -- [0..3] as hv_glcm's; [4 + d] the number of runs along offset d with L > R (counted in the last
 *   bin), 0 for d >= D.
 * hv_gldm: the neighbourhood of a voxel p is the 26 offsets at Chebyshev distance 1; alpha in 0..G - 1.  For every voxel p with slot s and
 *   level i: N(p) the neighbours inside the volume with slot s, n = |N(p)|, A the sum of their levels, k how many of them have
 *   |level - i| <= alpha.  dep (device, 8-byte aligned): [V][S][G][27] int64, dep[v][s][i][k] += 1 (column k + 1 of the pyradiomics matrix).
 *   ngt (device, 8-byte aligned): [V][S][G][27][2] int64, ngt[v][s][i][n][0] += 1 and ngt[v][s][i][n][1] += |i n - A|: NGTDM's n_i is the sum
 *   over n >= 1 of [..][0] and its s_i the sum over n >= 1 of [..][1] / n, exact and independent of any summation order.  info (device, 8-byte
 *   aligned): [V][S][HV_GLCM_INFO] int64 as hv_glcm's.
 *   Refusals, before any launch and with nothing written -- HV_ERR_ARG: a NULL pointer (mask excepted), a non-positive size, an unknown dtype, S
 *   outside 1..HV_LS_MAX_LABELS, G outside 2..HV_GLCM_MAX_LEVELS, a label value outside [0, 255] or listed twice, lo not finite, width not finite
 *   or not > 0, an output or info not 8-byte aligned, a workspace that is not 16-byte aligned or smaller than queried; hv_glrlm: D outside
 *   1..HV_GLRLM_MAX_OFFSETS, an offset component outside {-1, 0, 1}, a zero offset, an offset listed twice or beside its negative, R < 1;
 *   hv_gldm: alpha outside 0..G - 1; HV_ERR_UNSUPPORTED: more than 2^30 voxels per volume, V > 65535. */
enum { HV_GLRLM_MAX_OFFSETS = 13, HV_GLRLM_INFO = 17, HV_GLDM_NEIGHBOURS = 27 };
size_t hv_glrlm_workspace_bytes(int V, int A0, int A1, int A2, int S, int D, int G, int R);
int hv_glrlm(const void* vol, int vol_dtype, long long sv, long long s0, long long s1, long long s2, const void* label, int label_dtype,
             long long lsv, long long ls0, long long ls1, long long ls2, const void* mask, long long msv, long long ms0, long long ms1,
             long long ms2, int V, int A0, int A1, int A2, const int* labels, int S, const int* offsets, int D, double lo, double width, int G,
             int R, long long* out, long long* info, void* workspace, size_t workspace_bytes, void* stream);
size_t hv_gldm_workspace_bytes(int V, int A0, int A1, int A2, int S, int G);
int hv_gldm(const void* vol, int vol_dtype, long long sv, long long s0, long long s1, long long s2, const void* label, int label_dtype,
            long long lsv, long long ls0, long long ls1, long long ls2, const void* mask, long long msv, long long ms0, long long ms1,
            long long ms2, int V, int A0, int A1, int A2, const int* labels, int S, double lo, double width, int G, int alpha, long long* dep,
            long long* ngt, long long* info, void* workspace, size_t workspace_bytes, void* stream);

/* ---- separable linear filtering of a volume, and the weighted composite of two volumes (csrc/filter3d.hip).  The
 * reference filters nothing in 3-D; the definitions are scipy.ndimage.correlate1d / gaussian_filter1d / gaussian_filter (odd-length weights,
 * origin 0) applied to the float64 copy of the input, bit for bit on finite results, NaN where scipy has NaN.
 * hv_separable_filter: vol [A0][A1][A2], element (i, j, k) at vol[i*s0 + j*s1 + k*s2] (strides in elements, any order; a sub-box of a larger
 *   array is its first element's pointer with the array's strides), dtype HV_DT_U8 / I16 / F32 / F64.  in_mode HV_FILT_IN_VALUE: the voxel as a
 *   double; HV_FILT_IN_EQ: the indicator vol == value as 0.0 / 1.0 (a label's mask is never materialised).  axes: three hv_filter_axis in HOST
 *   memory, one per axis, copied into the kernel arguments of that axis' launch.  radius < 0 skips the axis (scipy skips sigma <= 1e-15); else
 *   w[0 .. 2 radius] are the correlation weights, centre at w[radius], radius <= HV_FILT_MAX_RADIUS, and form says how they are summed -- +1
 *   symmetric, -1 antisymmetric, 0 general; scipy picks +1 iff every |w[r+i] - w[r-i]| <= DBL_EPSILON, else -1 iff every |w[r+i] + w[r-i]| <=
 *   DBL_EPSILON, and the caller hands that choice over.  With x the line extended by the boundary mode, c the output's place in it, r the radius:
 *     +1: t = x[c] w[r]; for i = -r .. -1: t += (x[c+i] + x[c-i]) w[i+r]        -1: the same with (x[c+i] - x[c-i])
 *      0: t = x[c+r] w[2r]; for i = 0 .. 2r-1: t += x[c-r+i] w[i]               (NI_Correlate1D starts the general sum with the last tap)
 *   all float64, no fma, axes in the order 0, 1, 2, each pass on the doubles of the pass before.  mode: HV_FILT_REFLECT (d c b a | a b c d | d c b
 *   a), CONSTANT (cval; with HV_FILT_IN_EQ cval is in the indicator's domain), NEAREST, MIRROR (d c b | a b c d | c b a) or WRAP, scipy's modes of
 *   those names for 1-D filters; the patterns repeat, so a radius above the extent and an extent of 1 are legal in every mode.
 *   out, element (i, j, k) at out[i*os0 + j*os1 + k*os2]: out_dtype HV_DT_F64 the filtered doubles (8-byte aligned); HV_DT_U8 the mask t >=
 *   threshold as 0 / 1, formed in the last pass so that its doubles are never stored.  With all three axes skipped out is the converted (or
 *   thresholded) input.  The address ranges of out and vol must not intersect.
 *   workspace: 16-byte aligned, hv_filter_workspace_bytes(A0, A1, A2, axes) bytes (host only; 0 for arguments the entry refuses): 16 bytes for
 *   at most one filtered axis, else one C-ordered double volume (rounded up to 16 bytes) per pass after the first.  A float64 out uses one of
 *   them (the passes alternate between out and the workspace); a uint8 out after three passes needs both, and the query does not know out_dtype.
 *   hv_filter_tile (host only): dims[3] = the outputs per workgroup along each axis when that axis is filtered; the halo of `radius` elements on
 *   either side is resolved through the boundary map while the tile is staged in LDS, so a line's length is not limited.
 * hv_blend_lerp: out[i][j][k] = ((1 - w) * a) + (w * b) in float64, in this order.  a, b: HV_DT_I16 / F32 / F64, w: HV_DT_F64, or HV_DT_U8 as
 *   a mask (non-zero = 1.0); every operand has its own strides.  out: doubles, 8-byte aligned; it may be a itself (float64, the same strides)
 *   and must not intersect b, w, or a in any other way.
 * No atomics, no host synchronisation, no scratch; the same bytes on every run, whatever the workspace held; nothing outside the described
 * boxes is read or written.  Refusals, before any launch and with nothing written -- HV_ERR_ARG: a NULL pointer, a non-positive size, an
 *   unknown dtype, in_mode, boundary mode or form, a weight or cval that is not finite, out_dtype other than F64 / U8, a float64 out that is not
 *   8-byte aligned, a workspace that is not 16-byte aligned or smaller than queried, out intersecting an input; HV_ERR_UNSUPPORTED: a radius above
 *   HV_FILT_MAX_RADIUS, more than 2^30 voxels. */
enum { HV_FILT_MAX_RADIUS = 64, HV_FILT_MAX_TAPS = 129 };   /* HV_FILT_MAX_TAPS = 2 * HV_FILT_MAX_RADIUS + 1 */
enum { HV_FILT_IN_VALUE = 0, HV_FILT_IN_EQ = 1 };
enum { HV_FILT_REFLECT = 0, HV_FILT_CONSTANT = 1, HV_FILT_NEAREST = 2, HV_FILT_MIRROR = 3, HV_FILT_WRAP = 4 };
typedef struct {
    int radius, form;
    double w[HV_FILT_MAX_TAPS];
} hv_filter_axis;
size_t hv_filter_workspace_bytes(int A0, int A1, int A2, const hv_filter_axis* axes);
int hv_filter_tile(int* dims);
int hv_separable_filter(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, int in_mode, double value,
                        const hv_filter_axis* axes, int mode, double cval, void* out, int out_dtype, double threshold, long long os0,
                        long long os1, long long os2, void* workspace, size_t workspace_bytes, void* stream);
int hv_blend_lerp(const void* a, int a_dtype, long long as0, long long as1, long long as2, const void* b, int b_dtype, long long bs0,
                  long long bs1, long long bs2, const void* w, int w_dtype, long long ws0, long long ws1, long long ws2, int A0, int A1, int A2,
                  double* out, long long os0, long long os1, long long os2, void* stream);

/* ---- 3-D rank filters (csrc/rankfilt.hip): scipy.ndimage.rank_filter with a footprint of at most 9 x 9 x 9 cells,
 * which is what median_filter, percentile_filter, minimum_filter / maximum_filter and the flat grey-scale morphology are built from.
 * hv_rank_filter: vol [A0][A1][A2], element (i, j, k) at vol[i*s0 + j*s1 + k*s2] (strides in elements, any order; a sub-box of a larger array
 *   passes as it lies), dtype HV_DT_U8 / I16 / F32 / F64; out has the same dtype and its own strides, and its bytes must not intersect the bytes
 *   vol spans.  fp (HOST memory, copied into the kernel arguments): the footprint as a set of integer offsets o with |o_a| <= 4 -- bit
 *   ((o0 + 4) * 9 + (o1 + 4)) * 9 + (o2 + 4) of `bits` (bit b is bit b % 64 of bits[b / 64]) is set for each member, n is their number.
 *   out[p] = the rank-th smallest (0-based) of { ext(vol)[p + o] : o in the footprint }, ext the boundary extension of hv_separable_filter
 *   (mode: the HV_FILT_* codes; the patterns repeat, so an extent of 1 and a reach above the extent are legal).  The comparison is on
 *   order-preserving integer keys of the element's own width: for floats the sign-flipped bits, so -0.0 sorts just below +0.0 and NaNs sort at
 *   the two ends by their sign bit; the voxel written is one of the window's own voxels or cval, bit for bit.  A window without NaN is not
 *   affected by NaNs elsewhere; for a window with a NaN the answer is the key order's (scipy's depends on its selection algorithm).
 *   hv_rank_tile (host only): dims[3] = the outputs per workgroup along each axis, whatever the strides.
 * No atomics, no workspace, no host synchronisation, no scratch; the same bytes on every run.  Refusals, before any launch and with nothing
 *   written -- HV_ERR_ARG: a NULL pointer, a non-positive size, an unknown dtype or mode, n < 1, n other than the number of set bits, a bit set
 *   above index 728, rank outside [0, n), a cval that is not finite or not exactly representable in dtype (scipy compares such a cval as a
 *   double and truncates it on output: not offered), out intersecting vol; HV_ERR_UNSUPPORTED: more than 2^30 voxels. */
enum { HV_RANK_REACH = 4, HV_RANK_WORDS = 12 };             /* offsets -4 .. 4 per axis: 729 bits in 12 words */
typedef struct {
    int n;
    unsigned long long bits[HV_RANK_WORDS];
} hv_rank_footprint;
int hv_rank_tile(int* dims);
int hv_rank_filter(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, const hv_rank_footprint* fp,
                   int rank, int mode, double cval, void* out, long long os0, long long os1, long long os2, void* stream);

/* ---- 3-D affine resampling (csrc/resample.hip): scipy.ndimage.affine_transform, zoom and shift of a volume at spline
 * order 0, 1 or 3, mode constant (and nearest at order 0), scipy's bytes.
 * hv_resample: vol [A0][A1][A2], element (i, j, k) at vol[i*s0 + j*s1 + k*s2] (strides in elements, any order; a sub-box of a larger array
 *   passes as it lies), dtype HV_DT_U8 / I16 / F32 / F64.  For order 3 vol is the float64 coefficient volume hv_spline_prefilter leaves (window
 *   off), so dtype is HV_DT_F64 there.  out [O0][O1][O2] with its own dtype (any of the four) and strides; its bytes must not intersect the bytes
 *   vol spans.  desc (HOST memory, copied into the kernel arguments; no host-to-device copy): for output index o and input axis h, in float64
 *   without fused multiply-add,
 *     form HV_RESAMPLE_MATRIX:    u_h = ((o0 matrix[3h] + o1 matrix[3h+1]) + o2 matrix[3h+2]) + offset[h]   (summed from 0.0, the offset last)
 *     form HV_RESAMPLE_ZOOMSHIFT: u_h = (o_h + shift[h]) * zoom[h]                                          (scipy's zoom_shift)
 *   mode (the HV_FILT_* codes) HV_FILT_CONSTANT: u_h < 0 or u_h > A_h - 1 on any axis gives cval; HV_FILT_NEAREST (order 0 only): u_h is clamped
 *   to [0, A_h - 1].  order 0: the voxel at floor(u + 0.5); order 1: taps floor(u), floor(u) + 1 with the weights w0 = 1 - y, 1 - w0; order 3:
 *   the four taps and weights of the spline sampler above.  Tap indices beyond the ends are mirrored about the end points.  The sum runs over
 *   the taps with the last axis fastest, each term ((c w0) w1) w2, added from 0.0.  Output: float64 as it is; float32 rounded once; int16
 *   t > 0 ? t + 0.5 : t - 0.5, clamped, truncated; uint8 t > 0 ? t + 0.5 : 0, clamped, truncated.
 *   hv_resample_tile (host only): dims[3] = the outputs per workgroup along each axis, whatever the strides.
 * One launch, no atomics, no workspace, no host synchronisation, no scratch; the same bytes on every run; nothing outside the two boxes is read
 *   or written.  Refusals, before any launch and with nothing written -- HV_ERR_ARG: a NULL pointer, a non-positive extent, an unknown dtype,
 *   form, order (other than 0, 1, 3) or mode, a matrix, offset, zoom, shift or cval that is not finite (every field is checked, whatever the
 *   form), a cval that is not a value of an integer out_dtype, order 3 on anything but float64, a pointer not aligned to its element, out
 *   intersecting vol; HV_ERR_UNSUPPORTED: modes reflect / mirror / wrap, nearest at order 1 (scipy's edge rule there is not a clamp of the
 *   coordinate) or 3 (scipy pre-pads by 12 voxels), more than 2^30 voxels on either side. */
enum { HV_RESAMPLE_MATRIX = 0, HV_RESAMPLE_ZOOMSHIFT = 1 };
typedef struct {
    int form;
    double matrix[9], offset[3], zoom[3], shift[3];
    int order, mode;
    double cval;
} hv_resample_desc;
int hv_resample_tile(int* dims);
int hv_resample(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, void* out, int out_dtype,
                long long os0, long long os1, long long os2, int O0, int O1, int O2, const hv_resample_desc* desc, void* stream);

/* ---- deformable 3-D resampling (csrc/warp.hip): a volume sampled at coordinates the caller supplies
 * (scipy.ndimage.map_coordinates, or a dense displacement field) or at an affine lattice deformed by a coarse control grid.  vol, out, order,
 * mode and cval are hv_resample's, and from the coordinate u on everything is hv_resample's rule: outside test (a NaN coordinate fails it and
 * gives cval in mode constant; the nearest form clamps it to 0, as scipy does), taps, weights, mirrored indices, term order, output conversion.
 * hv_map_coordinates: coords holds three planes over the output lattice, component h of output (i, j, k) at coords[h*cp + i*c0 + j*c1 + k*c2]
 *   (strides in elements, any order: a [3][O0][O1][O2] array, a permuted view of one, an [O0][O1][O2][3] array and a sub-box all pass as they
 *   lie), coord_dtype HV_DT_F32 (widened exactly) or HV_DT_F64.  coord_kind HV_COORDS_ABSOLUTE: u_h = c_h(o); HV_COORDS_DISPLACEMENT:
 *   u_h = (double)o_h + c_h(o), a displacement field in source voxels.
 * hv_warp_grid: grid [3][G0][G1][G2], float64, component h at (a, b, c) at grid[h*gp + a*g0 + b*g1 + c*g2]: the displacement along source axis
 *   h in source voxels at that control point.  desc (HOST memory, copied into the kernel arguments): base is the lattice, order, mode and cval
 *   as for hv_resample.  For output index o, in float64 without fused multiply-add, in this order:
 *     q_a = (o_a + gshift[a]) * gzoom[a], then clamped to [0, G_a - 1] as q >= 0 ? (q <= hi ? q : hi) : 0
 *     d_h = the sampler's sum on grid[h] at q at order gorder: 1 the taps floor(q), floor(q) + 1 with the weights 1 - y, 1 - (1 - y); 3 the
 *           four taps and weights of the spline sampler applied to the control values themselves, with no prefilter (the approximating cubic
 *           B-spline of free-form deformation).  Tap indices mirrored about the ends, last axis fastest, each term ((g w0) w1) w2, from 0.0
 *     u_h = base_h(o) + d_h, base_h hv_resample's expression for base.form
 *   hv_map_coordinates_tile / hv_warp_grid_tile (host only): dims[3] = the outputs per workgroup along each axis, whatever the strides.
 * One launch per call, no atomics, no workspace, no host synchronisation, no scratch; the same bytes on every run and for any strides; nothing
 *   outside the stated boxes is read or written.  Refusals, before any launch and with nothing written -- hv_resample's own list, and
 *   HV_ERR_ARG: a NULL coords / grid, a coord_dtype other than F32 / F64, an unknown coord_kind, coords or grid not aligned to its element,
 *   out intersecting coords or grid, a gorder other than 1 or 3, a non-positive grid extent, a gzoom or gshift that is not finite;
 *   HV_ERR_UNSUPPORTED: more than 2^30 control points. */
enum { HV_COORDS_ABSOLUTE = 0, HV_COORDS_DISPLACEMENT = 1 };
typedef struct {
    hv_resample_desc base;
    double gzoom[3], gshift[3];
    int gorder;
} hv_warp_desc;
int hv_map_coordinates_tile(int* dims);
int hv_warp_grid_tile(int* dims);
int hv_map_coordinates(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, const void* coords,
                       int coord_dtype, long long cp, long long c0, long long c1, long long c2, int coord_kind, void* out, int out_dtype,
                       long long os0, long long os1, long long os2, int O0, int O1, int O2, int order, int mode, double cval, void* stream);
int hv_warp_grid(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, const double* grid, long long gp,
                 long long g0, long long g1, long long g2, int G0, int G1, int G2, void* out, int out_dtype, long long os0, long long os1,
                 long long os2, int O0, int O1, int O2, const hv_warp_desc* desc, void* stream);

/* ---- joint intensity histograms of a fixed and a moving volume under a list of affine poses (csrc/similarity.hip):
 * what mutual information, its normalised form and the entropy correlation coefficient are computed from.  The reference has no counterpart.
 * hv_joint_hist: fixed [O0][O1][O2], element (i, j, k) at fixed[i*fs0 + j*fs1 + k*fs2]; moving [A0][A1][A2] likewise; both HV_DT_U8 / I16 /
 *   F32 / F64, strides in elements, any order (a sub-box passes as it lies).  At order 3 moving is the float64 coefficient volume of
 *   hv_spline_prefilter, as for hv_resample.  mask (may be NULL): uint8 over the fixed lattice with its own strides.  poses (HOST, [K][12]
 *   doubles: matrix[9] then offset[3], 1 <= K <= HV_JH_MAX_POSES) are copied into the kernel arguments; no host-to-device copy.
 *   For every fixed voxel o and every pose k, in this order:
 *     1. mask != NULL and mask(o) == 0: the voxel is in no pair; info[k][2] += 1.
 *     2. x = (double)fixed(o) not finite: in no pair; info[k][3] += 1.
 *     3. u_h = ((o0 m[3h] + o1 m[3h+1]) + o2 m[3h+2]) + off[h], summed from 0.0, float64 without fma: hv_resample's HV_RESAMPLE_MATRIX form.
 *     4. u_h < 0 or u_h > A_h - 1 on any axis (a NaN counts as outside): the pair is not counted; info[k][4] += 1.  No cval is invented: only
 *        the overlap is measured.
 *     5. y = hv_resample's float64 sum at `order` 0 / 1 / 3 (taps, weights, mirrored indices, last axis fastest, ((c w0) w1) w2 from 0.0), with
 *        no output conversion.  y not finite: not counted; info[k][3] += 1.
 *     6. levels by hv_glcm's rule: t = (x - flo) / fwidth, two IEEE operations; lf = 0 if t < 0, Gf - 1 if t >= Gf, else (int)t; lm the same
 *        from y, mlo, mwidth, Gm.  out[k][lf][lm] += 1.
 *   out (device, 8-byte aligned): [K][Gf][Gm] int64.  info (device, 8-byte aligned): [K][HV_JH_INFO] int64 -- [0] HV_LS_NONFINITE if [3] > 0,
 *   ORed with HV_LS_EMPTY if [1] == 0; [1] counted pairs; [2] masked out; [3] non-finite (fixed or sampled); [4] outside; [5], [6] the counted
 *   pairs whose fixed level was clamped from below / from above; [7] the counted pairs whose moving level was clamped from below or above.
 *   For every k: [1] + [2] + [3] + [4] == O0 * O1 * O2 and the sum of out[k] == [1].
 *   The entry zeroes out and info itself on the stream.  Only integer atomics: the same bytes on every run, for any strides, whatever the
 *   buffers held.  No host synchronisation.  workspace: hv_joint_hist_workspace_bytes bytes, which is 0 -- the tables live in LDS -- so NULL
 *   is accepted; a pointer that is given must be 16-byte aligned.
 *   Refusals, before any launch and with nothing written -- HV_ERR_ARG: a NULL pointer (mask and workspace excepted), a non-positive extent,
 *   an unknown dtype, order other than 0 / 1 / 3, order 3 on a moving volume that is not float64, K outside 1..HV_JH_MAX_POSES, Gf or Gm
 *   outside 2..HV_JH_MAX_LEVELS, a pose entry, flo or mlo that is not finite, a width that is not finite or not > 0, fixed or moving not
 *   aligned to its element, out or info not 8-byte aligned, out or info intersecting fixed, moving, mask or each other, a misaligned
 *   workspace; HV_ERR_UNSUPPORTED: more than 2^30 voxels on either side. */
enum { HV_JH_MAX_LEVELS = 64, HV_JH_MAX_POSES = 16, HV_JH_INFO = 8 };
size_t hv_joint_hist_workspace_bytes(int O0, int O1, int O2, int K, int Gf, int Gm);
int hv_joint_hist(const void* fixed, int fixed_dtype, long long fs0, long long fs1, long long fs2, int O0, int O1, int O2, const void* moving,
                  int moving_dtype, long long ms0, long long ms1, long long ms2, int A0, int A1, int A2, const void* mask, long long ks0,
                  long long ks1, long long ks2, const double* poses, int K, int order, double flo, double fwidth, int Gf, double mlo,
                  double mwidth, int Gm, long long* out, long long* info, void* workspace, size_t workspace_bytes, void* stream);

/* ---- per-label 3-D shape records: the 2 x 2 x 2 cell-configuration histogram (Minkowski measures), coordinate moments and directional extents
 * (csrc/shape.hip).  The reference has no counterpart.
 * hv_shape: label, label_dtype and strides, mask and strides, V, A0..A2 and labels[S] exactly as for hv_label_stats and hv_glcm (a label value
 *   that is no integer in [0, 255] sets HV_LS_BAD_LABEL for its whole volume and has no slot).  The slot of voxel p is the s with
 *   label(p) == labels[s], provided mask is NULL or mask(p) != 0; otherwise, and outside the volume, the voxel has no slot.
 *   out (device, 8-byte aligned): [V][S][HV_SHAPE_REC] int64, per (volume, listed label):
 *     [0 .. 255] the configuration histogram over the cells c = (i, j, k), i in [-1, A0 - 1], j in [-1, A1 - 1], k in [-1, A2 - 1] -- the
 *       (A0 + 1)(A1 + 1)(A2 + 1) cells of the lattice padded by one background layer.  For slot s, code = the sum of bit (4 d0 + 2 d1 + d2) over
 *       d in {0, 1}^3 with slot(c + d) == s; out[v][s][code] += 1 for code != 0, and out[v][s][0] is the cell count minus the rest, so every
 *       histogram sums to the cell count.  A cell whose corners hold several listed labels counts once in each of those slots, with that
 *       slot's code.
 *     [HV_SHAPE_COUNT] n, the voxel count; [HV_SHAPE_SUM + a] the sum of p_a; [HV_SHAPE_SUM2 + 0 .. 5] the sums of p_a p_b in the order 00, 01,
 *       02, 11, 12, 22 -- all exact int64.
 *     [HV_SHAPE_EXTENT + 2t], [HV_SHAPE_EXTENT + 2t + 1], t < 13: the minimum and the maximum of the integer dot product d_t . p over the
 *       slot's voxels, d_t the t-th of the 13 offsets (a, b, c) > (0, 0, 0) in lexicographic order; n = 0: INT64_MAX and INT64_MIN.
 *     [HV_SHAPE_STATUS] the OR of HV_LS_BAD_LABEL and HV_LS_EMPTY (n = 0); the words after it are 0.
 *   The entry initialises out itself on the stream.  Only integer atomics: the same bytes on every run, for any strides, single or stacked,
 *   whatever out and the workspace held.  No host synchronisation.  workspace: 16-byte aligned, hv_shape_workspace_bytes(V, A0, A1, A2, S) bytes.
 *   Refusals, before any launch and with nothing written -- HV_ERR_ARG: a NULL pointer (mask excepted), a non-positive size, an unknown dtype,
 *   S outside 1..HV_LS_MAX_LABELS, a label value outside [0, 255] or listed twice, out not 8-byte aligned, a misaligned or too small workspace;
 *   HV_ERR_UNSUPPORTED: more than 2^30 voxels per volume, V > 65535, or A0 A1 A2 max(A_a - 1)^2 >= 2^62 (the second moments would leave int64).
 *   hv_shape_workspace_bytes returns 0 for all of these. */
enum { HV_SHAPE_REC = 320, HV_SHAPE_COUNT = 256, HV_SHAPE_SUM = 257, HV_SHAPE_SUM2 = 260, HV_SHAPE_EXTENT = 266, HV_SHAPE_STATUS = 292 };
size_t hv_shape_workspace_bytes(int V, int A0, int A1, int A2, int S);
int hv_shape(const void* label, int label_dtype, long long lsv, long long ls0, long long ls1, long long ls2, const void* mask, long long msv,
             long long ms0, long long ms1, long long ms2, int V, int A0, int A1, int A2, const int* labels, int S, long long* out,
             void* workspace, size_t workspace_bytes, void* stream);

/* ---- parallel-beam projections of a volume under a list of affine poses (csrc/projection.hip): what a radiograph
 * (line integral), a minimum / maximum intensity projection, a thickness map and an areal density are computed from.  The reference has no
 * counterpart.  A projection is hv_resample's HV_RESAMPLE_MATRIX lattice (p0, p1, t), reduced over t without ever being written.
 * hv_project: vol [A0][A1][A2], element (i, j, k) at vol[i*s0 + j*s1 + k*s2] (strides in elements, any order; a sub-box passes as it lies),
 *   dtype HV_DT_U8 / I16 / F32 / F64; at order 3 vol is the float64 coefficient volume of hv_spline_prefilter, as for hv_resample.  label (may be
 *   NULL): the same logical shape with its own strides ls0..ls2, any HV_DT_* code, with label_value.  poses (HOST, [K][12] doubles: matrix[9]
 *   then offset[3], 1 <= K <= HV_PROJ_MAX_POSES) are copied into the kernel arguments; no host-to-device copy.  Detector P0 x P1, T steps.
 *   For every pose k, pixel (p0, p1) and step t = 0 .. T - 1, in float64 without fused multiply-add, in this order:
 *     1. u_h = ((p0 m[3h] + p1 m[3h+1]) + t m[3h+2]) + off[h], summed from 0.0, the offset last: hv_resample's expression.
 *     2. u_h < 0 or u_h > A_h - 1 on any axis (a NaN counts as outside): info[k][2] += 1.  Nothing is padded: only the part of a ray inside
 *        the volume is measured.
 *     3. label != NULL and (double)label(q) != label_value, q_h = floor(u_h + 0.5): info[k][3] += 1.
 *     4. y = hv_resample's float64 sum at `order` 0 / 1 / 3 (taps, weights, mirrored indices, last axis fastest, ((c w0) w1) w2 from 0.0), with
 *        no output conversion.  y not finite: info[k][4] += 1.
 *     5. otherwise the sample is counted: info[k][1] += 1.
 *   Per pixel, over the counted samples:
 *     sum: the steps are cut into chunks of HV_PROJ_CHUNK consecutive t; a chunk's sum is taken sequentially from +0.0 in increasing t; the
 *       chunk sums are added sequentially from +0.0 in increasing chunk order, every chunk, the empty ones included.  This order is the
 *       definition, not an implementation note: the result is the same bytes on every run and equals a restatement in that order.
 *     min, max: by value, from +inf / -inf; the stored word is m + 0.0, so a zero extreme is always +0.0.
 *     count, first, last: the number of counted steps, the smallest and the largest counted t.
 *     No counted step: sum +0.0, min +inf, max -inf, count 0, first T, last -1.
 *   acc (device, 8-byte aligned): [K][3][P0][P1] float64 -- sum, min, max.  idx (device, 4-byte aligned): [K][3][P0][P1] int32 -- count, first,
 *   last.  info (device, 8-byte aligned): [K][HV_PROJ_INFO] int64 -- [0] HV_LS_NONFINITE if [4] > 0, ORed with HV_LS_EMPTY if [1] == 0; [1]
 *   counted; [2] outside; [3] rejected by the label; [4] non-finite; [5 .. 7] 0.  For every k: [1] + [2] + [3] + [4] == P0 * P1 * T and the sum
 *   of count == [1].
 *   hv_project_tile (host only): dims[5] = HV_PROJ_CHUNK; the pixels per workgroup and the lanes per ray R when the ray runs along adjacent
 *   lanes; the same two when a detector axis does (each for a ray of at least R chunks; a shorter ray takes the power of two of lanes that
 *   covers its chunks and the workgroup 256 / R pixels).
 *   The entry zeroes info itself on the stream; every word of acc and idx is written.  Only integer atomics: the same bytes on every run,
 *   for any strides, whatever the buffers held.  No host synchronisation, no scratch.  workspace: hv_project_workspace_bytes bytes, which is 0
 *   -- the running words live in registers and LDS -- so NULL is accepted; a pointer that is given must be 16-byte aligned.
 *   Refusals, before any launch and with nothing written -- HV_ERR_ARG: a NULL pointer (label and workspace excepted), a non-positive extent,
 *   K or T, K > HV_PROJ_MAX_POSES, an unknown dtype or order, order 3 on anything but float64, a pose entry or label_value that is not finite (with or
 *   without a label), with a label an unknown label_dtype, a pointer not aligned to its element, an output intersecting an input or another
 *   output; HV_ERR_UNSUPPORTED: more than 2^30 voxels, P0 * P1 * T > 2^30. */
enum { HV_PROJ_CHUNK = 16, HV_PROJ_MAX_POSES = 16, HV_PROJ_INFO = 8 };
int hv_project_tile(int* dims);
size_t hv_project_workspace_bytes(int A0, int A1, int A2, int K, int P0, int P1, int T);
int hv_project(const void* vol, int dtype, long long s0, long long s1, long long s2, int A0, int A1, int A2, const void* label,
               int label_dtype, long long ls0, long long ls1, long long ls2, double label_value, const double* poses, int K, int P0, int P1,
               int T, int order, double* acc, int* idx, long long* info, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
