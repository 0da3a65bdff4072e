/* libwct_hip.so -- C ABI of the MI355X (gfx950) stylize hot path.
 *
 * The reference (eridgd/WCT-TF) has no FFI: its boundary is the Python API that
 * drives one TensorFlow session.  Each entry point below names the reference
 * interface it replaces (paths relative to the reference tree).  INTEGRATION.md
 * shows the ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative wct_status on failure;
 *     wct_last_error() returns a thread-local message.  No exceptions cross the ABI.
 *   - one wct_ctx = one GPU + one HIP stream; calls on a ctx are serialised
 *     (the reference's predict() is blocking and not re-entrant, wct.py:70-106);
 *     distinct contexts are independent (one per process/GPU for multi-GPU).
 *   - "host" pointers are caller-owned and only read/written during the call;
 *     "dev" pointers are device memory obtained from wct_dev_alloc (or any
 *     hipMalloc'ed / torch CUDA pointer on the same device).
 *   - images: uint8 HxWx3 RGB, row-major (wct.py:60-68).  features: float32
 *     NHWC with batch 1, i.e. [H*W][C] pixel-major (ops.py:32-33 squeeze).
 *   - weights: float32 HWIO, exactly what vgg_normalised.py:33 / Keras Conv2D hold.
 */
#ifndef WCT_HIP_H
#define WCT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wct_ctx wct_ctx;

enum wct_status { WCT_STATUS_OK = 0, WCT_STATUS_HIP = -1, WCT_STATUS_ARG = -2,
                  WCT_STATUS_STATE = -3, WCT_STATUS_NOMEM = -4,
                  /* An eigendecomposition behind the call (the stand-in for tf.svd / np.linalg.svd, ops.py:53-65,110,123)
                   * did not converge within its sweep budget (16 sweeps; 4-6 are typical at C = 512, 7-10 on graded
                   * rank-deficient spectra; the test hook WCT_JACOBI_MAX_SWEEPS can only lower it), or met NaN/Inf
                   * in a covariance.  The outputs of the call ARE written (best effort, as LAPACK does with info > 0)
                   * but must not be trusted; the reference's own worry at this spot is ops.py:57-65.  Reported by the
                   * blocking calls themselves and, for wct_stylize_batch_dev (asynchronous), by the next wct_sync. */
                  WCT_STATUS_NOCONV = -5 };

/* transform semantics: wct_np (ops.py:92-140) or the live-graph wct_tf (ops.py:24-90) */
enum wct_mode { WCT_NP = 0, WCT_TF = 1 };

/* flags for wct_stylize* */
enum wct_flags {
  WCT_FLAG_ADAIN = 1,      /* --adain: AdaIN at every level instead of WCT (model.py:148-158) */
  WCT_FLAG_MODE_NP = 2,    /* use wct_np semantics instead of the graph's wct_tf */
  WCT_FLAG_SWAP5 = 4,      /* --swap5: style-swap at relu5_1 (wins over ADAIN there, model.py:148-152) */
  WCT_FLAG_STYLE_SHARED = 8, /* wct_stylize_batch_dev only: `style` is ONE image shared by all B pairs (stylize_video.py
                              keeps one style for every frame but re-runs it per frame, stylize_video.py:88-106);
                              the style pass, statistics and eigensystems run once per call, results are identical */
  WCT_FLAG_IMAGES_F32 = 16, /* content / style point at float32 images already in [0,1] (WCT.preprocess applied by the
                              caller: a FLOAT input of predict() is divided by 255 without rounding, wct.py:60-64)
                              instead of uint8 ones; the output stays uint8 */
  WCT_FLAG_CONTENT_COLORS = 32, /* luminance-only colour preservation: every frame keeps its stylized luminance and takes the
                              colours of its content (see wct_content_colors).  Honoured by every wct_stylize* call, with
                              any of the flags above; the frame equals wct_content_colors(the unflagged frame, the content)
                              bit for bit.  Without the flag nothing changes */
  WCT_FLAG_GUIDED = 64     /* guided smoothing, the photo mode: every frame is filtered with its content as guide (see
                              wct_guided_filter), radius and eps_q from wct_set_guided, the guide from wct_set_guided_guide.  Honoured by every wct_stylize* call that
                              ends in the whole-image chain, with any of the flags above; the frame equals wct_guided_filter(the
                              unflagged frame, the content) bit for bit, and with WCT_FLAG_CONTENT_COLORS as well
                              wct_content_colors(that, the content): the colour op runs last.  The banded, texture and wrap
                              calls refuse it (WCT_STATUS_ARG, a message that names it) */
};

/* the guide of guided smoothing (wct_guided_filter_guide, wct_set_guided_guide) */
enum wct_guide { WCT_GUIDE_GREY = 0,   /* the grey of the content: one channel, one division per pixel and channel */
                 WCT_GUIDE_COLOR = 1   /* its three channels: a 3 x 3 solve per pixel; sees an edge between colours of equal luminance */ };

/* ---- lifecycle: replaces WCT.__init__'s tf.Session setup (wct.py:29-44) ---- */
int  wct_create(int device, wct_ctx** out);
void wct_destroy(wct_ctx* ctx);
const char* wct_last_error(void);
int  wct_sync(wct_ctx* ctx);                       /* block until the ctx stream is idle; WCT_STATUS_NOCONV if an
                                                       eigensolve of the work just completed failed (see above) */
int  wct_device_count(int* n);
/* The ctx's HIP stream (a hipStream_t), so that a caller can order its own device work -- e.g. the RCCL gather of the
 * finished frames, multi-GPU runs -- behind wct_stylize_batch_dev without a host sync (record an event on it, wait for
 * the event on the other stream).  The reference has no counterpart: its session is blocking (wct.py:97-104). */
int  wct_get_stream(wct_ctx* ctx, void** stream_out);

/* ---- weights: replace vgg_from_t7 (vgg_normalised.py:10-55) and the per-decoder
 * Saver.restore (wct.py:46-58).  The library copies, folds the 1x1 'preprocess'
 * into conv1_1 and repacks to its fp16 MFMA-fragment layout [Cout/32][tap][Cin/16][lane][8].
 *   pre_w [3][3] (in,out) and pre_b [3]: the 1x1 preprocess conv;
 *   w[i] HWIO 3x3 and b[i] for conv1_1, conv1_2, conv2_1, conv2_2, conv3_1..3_4,
 *   conv4_1..4_4, conv5_1 (13 layers). */
int wct_set_encoder(wct_ctx* ctx, const float* pre_w, const float* pre_b,
                    const float* const* w, const float* const* b, int n_layers);
/* decoder for relu<level>_1, level 1..5; conv layers in execution order
 * (model.py:283-298): 2, 3, 5, 9, 13 layers for level 1..5. */
int wct_set_decoder(wct_ctx* ctx, int level, const float* const* w, const float* const* b,
                    int n_layers);

/* ---- op level (host pointers), for parity tests -------------------------------- */
/* wct_np / wct_tf (ops.py:24-140): content [Nc][C], style [Ns][C], out [Nc][C].
 * eps: the reference functions' `eps` argument (wct_np: added inside the spectral gains,
 * default 1e-5; wct_tf: added to the covariance diagonal, default 1e-8); eps < 0 = default.
 * Cut-off: the reference keeps eigenvalues > 1e-5 (ops.py:68-69 / 112,125).  So does this path, with one refinement for
 * covariances whose float32 rounding noise is ABOVE that absolute threshold (N < C pixels at feature scales from ~10 up: the
 * exact zeros come out as +-1.5e-7 ||cov||): a covariance is positive semi-definite, its most negative computed eigenvalue -r
 * measures that noise, and eigenvalues <= max(1e-5, 2 r) are dropped -- the outcome of the reference's formula in exact
 * arithmetic, inside the band of kept counts its own float32 evaluation can land on (csrc/spectral.hip spectral_cut). */
int wct_transform(wct_ctx* ctx, const float* content, int Nc, const float* style, int Ns,
                  int C, float alpha, int mode, float eps, float* out,
                  int* sweeps_out /* [2] (content, style) or NULL: Jacobi sweeps used, > 0 when converged;
                                     -sweeps when still rotating after the sweep budget; <= -1000 for non-finite
                                     input.  Any negative entry also makes the call return WCT_STATUS_NOCONV */);
/* adain (ops.py:282-294), epsilon as in the reference signature */
int wct_adain(wct_ctx* ctx, const float* content, int Nc, const float* style, int Ns,
              int C, float alpha, float epsilon, float* out);
/* Style mixes -- interpolation between styles (Li et al. 2017, sec. 4.2 "controlling the style"; the reference's README
 * TODO "Interpolation between styles", the original Torch WCT's -style a,b -styleInterpWeights w1,w2):
 *   lambda_k = weights[k] / sum(weights),   mix(fc) = sum_k lambda_k T(fc, fs_k, alpha)
 * with T the single-style transform of the call below it.  K = 1 .. 8 styles of any pixel counts Ns[k]; weights finite,
 * >= 0, summing to > 0 -- else WCT_STATUS_ARG.  T is affine in the colouring side, so the mix is ONE transform: the content
 * is whitened once, the K colouring matrices and style means are mixed (fp32, k in order, from 0), then one blend and one
 * apply.  K = 1, and one-hot weights, give the single-style call's output bit for bit.
 * wct_transform_mix: wct_np / wct_tf (ops.py:24-140) as wct_transform; NOCONV under wct_transform's rules.
 *   sweeps_out [1 + K] or NULL: the content's sweeps, then style k's (wct_transform's contract). */
int wct_transform_mix(wct_ctx* ctx, const float* content, int Nc, const float* const* styles, const int* Ns, int K,
                      const float* weights, int C, float alpha, int mode, float eps, float* out, int* sweeps_out);
/* adain (ops.py:282-294) with sqrt(var_s) -> sum_k lambda_k sqrt(var_k) and mean_s -> sum_k lambda_k mean_k */
int wct_adain_mix(wct_ctx* ctx, const float* content, int Nc, const float* const* styles, const int* Ns, int K,
                  const float* weights, int C, float alpha, float epsilon, float* out);
/* Spatial control -- a label map picks the style of each region (Li et al. 2017, sec. 4.2 and Fig. 7 "spatial control"; the
 * reference's README TODO "Spatial control/masking"): with K = 1 .. 8 styles and a label in 0 .. K - 1 per content row,
 *   out[rows of k] = T(content[rows of k], style k, alpha)
 * with T the single-style transform of the call below it and region k's own statistics (mean, covariance with 1 / (N_k - 1),
 * cut-off).  A label with fewer than 2 rows passes its rows through unchanged (N_k - 1 = 0); a label with none is skipped.
 * A label >= K, or K outside 1 .. 8, is WCT_STATUS_ARG.  Every region comes out bit for bit as the single-style call on its
 * rows alone, so K = 1 gives that call's output, and a region's rows do not depend on the other regions' styles.
 * wct_transform_masked: wct_np / wct_tf (ops.py:24-140) as wct_transform; labels [Nc]; styles[k] [Ns[k]][C].
 *   sweeps_out [2K] or NULL: label k's content sweeps at 2k, its style's at 2k + 1 (wct_transform's contract); 0 for a label
 *   with fewer than 2 rows. */
int wct_transform_masked(wct_ctx* ctx, const float* content, int Nc, const uint8_t* labels, const float* const* styles,
                         const int* Ns, int K, int C, float alpha, int mode, float eps, float* out, int* sweeps_out);
/* adain (ops.py:282-294) per region, with that region's moments and its style's */
int wct_adain_masked(wct_ctx* ctx, const float* content, int Nc, const uint8_t* labels, const float* const* styles,
                     const int* Ns, int K, int C, float alpha, float epsilon, float* out);
/* the device's stable partition of an h x w feature map's rows by label, row (i, j) labelled
 * mask[min(i * stride, Hm - 1)][min(j * stride, Wm - 1)]: perm_out [h * w] lists the rows of label 0 in order, then those of
 * label 1, ...; seg_off_out [K + 1] where each label starts (what the masked calls use; a check of their first pass) */
int wct_mask_compact(wct_ctx* ctx, const uint8_t* mask, int Hm, int Wm, int h, int w, int stride, int K, int* perm_out,
                     int* seg_off_out);
/* the same for B <= 32 label maps masks [B][Hm][Wm] in ONE launch of each pass (the frame is a grid axis; what the masked batch
 * call uses): perm_out [B][h * w], seg_off_out [B][K + 1], frame f's being what wct_mask_compact gives for masks[f] alone.  Like
 * wct_mask_compact this is a check of the masked calls' first pass (tests/test_gpu_mask_video.py), not a call to build on */
int wct_mask_compact_batch(wct_ctx* ctx, const uint8_t* masks, int B, int Hm, int Wm, int h, int w, int stride, int K,
                           int* perm_out, int* seg_off_out);
/* wct_style_swap (ops.py:145-278): content [hc*wc][C], style [hs*ws][C], out [hc*wc][C]; `alpha` is the
 * reference's ss_alpha; eps < 0 = its default 1e-8.  (hc, wc) must survive the patch/stride round trip
 * (utils.swap_filter_fit, wct.py:84-90) -- always true for stride 1. */
int wct_style_swap(wct_ctx* ctx, const float* content, int hc, int wc, const float* style, int hs, int ws,
                   int C, float alpha, int patch_size, int stride, float eps, float* out);
/* style-swap settings used by wct_stylize* when WCT_FLAG_SWAP5 is set: WCT(ss_patch_size, ss_stride)
 * (wct.py:17-18) and predict(ss_alpha) (wct.py:70).  Defaults 0.6 / 3 / 1 (stylize.py:34-37). */
int wct_set_style_swap(wct_ctx* ctx, float ss_alpha, int patch_size, int stride);
/* symmetric eigendecomposition used in place of tf.svd / np.linalg.svd (ops.py:53-55,110,123):
 * A [nmat][C][C] in; evals [nmat][C], evecs [nmat][C][C] (columns) out.  The UPPER triangle of A (a[i][j],
 * i <= j) is authoritative: the entry point mirrors it into the lower one on its staged copy before the
 * solve (the solver reads an element from whichever triangle is contiguous for the kernel at hand), so a
 * matrix that is symmetric only to round-off, or upper-only data, is solved as that symmetric matrix; the
 * lower triangle may hold anything (NaN included) and the caller's array is not written.  evals is not
 * sorted: column j of evecs belongs to evals[j], and eigenpair j is the one that grew out of coordinate j,
 * so a matrix that is already diagonal comes back exact and in place: evals = its diagonal, evecs = I.
 * Accepted: C a multiple of 32 with 32 <= C <= 1024, 1 <= nmat <= 64, ctx / A / evals / evecs non-null.
 * Anything else returns WCT_ERR_ARG ("invalid argument") from the first line of the call: a refused call
 * reads no host memory, stages and launches nothing, and leaves the context as it was.
 * Batch guarantee: the evals, evecs and sweeps of a matrix are, bit for bit, those of the same matrix solved
 * alone (nmat = 1) -- they depend neither on nmat, nor on the matrix' position in the batch, nor on what its
 * neighbours are (a neighbour that fails, by running out of sweeps or on non-finite input, included). */
int wct_eigh(wct_ctx* ctx, const float* A, int C, int nmat, float* evals, float* evecs,
             int* sweeps_out /* [nmat] or NULL; same contract as wct_transform's */);
/* Conv2DReflect (ops.py:17-19): x [H][W][Cin] fp32, w HWIO, y [Ho][Wo][Cout] fp32;
 * upsample!=0 applies UpSampling2D x2 first (model.py:293). fp16 operands, fp32 accumulate.
 * Cin and Cout must be multiples of 64 (every 3x3 layer of the path but conv1_1 / the output conv). */
int wct_conv3x3(wct_ctx* ctx, const float* x, int H, int W, int Cin, const float* w_hwio,
                const float* bias, int Cout, int relu, int upsample, float* y);
/* The same layer as the stylize pipeline runs it (Conv2DReflect, ops.py:17-19; cuDNN picks the algorithm for Keras' Conv2D,
 * vgg_normalised.py:35-40 / model.py:291): a batch x [B][H][W][Cin], fp16 activations out (returned as fp32), optionally with the
 * following MaxPooling2D(padding='same') fused (vgg_normalised.py:42; needs relu).  algo 0: the kernel the pipeline uses for
 * this layer shape; 1: the direct implicit-GEMM kernel; 2: the reduced-FLOP kernel (Winograd F(2,3) along y, csrc/conv_wino.hip).
 * y [B][Ho][Wo][Cout]. */
int wct_conv3x3_f16(wct_ctx* ctx, const float* x, int B, int H, int W, int Cin, const float* w_hwio,
                    const float* bias, int Cout, int relu, int upsample, int pool, int algo, float* y);
/* MaxPooling2D(padding='same') (vgg_normalised.py:42): y [(H+1)/2][(W+1)/2][C] */
int wct_maxpool(wct_ctx* ctx, const float* x, int H, int W, int C, float* y);
/* encoder to relu<level>_1 (model.py:135-139): img01 [H][W][3] in [0,1]; feat [h][w][C] */
int wct_encode(wct_ctx* ctx, const float* img01, int H, int W, int level, float* feat);
/* decoder for relu<level>_1 (model.py:245-304): feat [h][w][C]; img [h*2^(l-1)][w*2^(l-1)][3] */
int wct_decode(wct_ctx* ctx, const float* feat, int h, int w, int level, float* img);
/* coral_numpy / preserve_colors_np (coral.py:13-39, utils.py:87-90), the O(pixels) parts:
 *   wct_coral_stats: exact integer moments of a uint8 image on the GPU:
 *     sums[0..2] = sum_c x, sums[3..8] = sum x_i x_j for (i,j) = 00,01,02,11,12,22.
 *   wct_coral_apply: out = (M ((x/255 - src_mean)/src_std)) * tgt_std + tgt_mean in float64,
 *     and its clip/x255/truncate uint8 image (utils.py:89).  Either output may be NULL.
 * The 3x3 step between them (coral.py:30-33: X X^T + I, matSqrt through the SVD, inverse) stays on
 * the host in the caller: the reference's matSqrt multiplies U sqrt(D) by U -- not U^T -- so its
 * value is defined by LAPACK's singular-vector signs, and only LAPACK reproduces that. */
int wct_coral_stats(wct_ctx* ctx, const uint8_t* img, int H, int W, double sums[9]);
int wct_coral_apply(wct_ctx* ctx, const uint8_t* src, int H, int W, const double M[9],
                    const double src_mean[3], const double src_std[3],
                    const double tgt_mean[3], const double tgt_std[3],
                    uint8_t* out_u8, double* out_f64);
/* Luminance-only colour preservation (Gatys et al. 2016, "Preserving Color in Neural Artistic Style Transfer", luminance-only
 * transfer in its post-hoc form; jcjohnson/neural-style's -original_colors).  The reference's own answer to the same need is
 * CORAL on the style (utils.py:87-90, above), which makes the style depend on the content; this one touches the finished frame
 * only, so it goes with every stylize call.  Integers only -- stylized s [Ho][Wo][3], content c [Hc][Wc][3], Ho >= Hc, Wo >= Wc:
 *   p      = c[min(y, Hc - 1)][min(x, Wc - 1)]        (the clamp of the label maps: a frame can be larger than its content)
 *   Y(q)   = 77 q.R + 150 q.G + 29 q.B                 (BT.601 x 256; the weights sum to 256)
 *   d      = Y(s[y][x]) - Y(p)
 *   out.ch = clamp((256 p.ch + d + 128) >> 8, 0, 255)  for ch in R, G, B; >> is arithmetic (floor)
 * i.e. Y from s, U and V from p, for any luma-weighted YUV.  s == c gives c; a grey content gives a grey frame.
 * WCT_FLAG_CONTENT_COLORS is this rule fused into the last launch of a stylize call: s is the decoded frame under the call's
 * output rule uint8(clip(x, 0, 1) * 255.f) (truncating), c the content bytes as given -- with WCT_FLAG_IMAGES_F32 the float
 * content under that same output rule.  Hence  stylize(flag) == wct_content_colors(stylize(no flag), content)  bit for bit.
 * wct_content_colors: host pointers, blocking.  wct_content_colors_batch_dev: device pointers, B = 1 .. 32 frames
 *   [B][Ho][Wo][3] and contents [B][Hc][Wc][3], asynchronous on the ctx stream; out_dev may be stylized_dev (in place).
 * Ho < Hc, Wo < Wc, a null pointer or B outside 1 .. 32 is WCT_STATUS_ARG and leaves the ctx usable. */
int wct_content_colors(wct_ctx* ctx, const uint8_t* stylized, int Ho, int Wo, const uint8_t* content, int Hc, int Wc,
                       uint8_t* out);
int wct_content_colors_batch_dev(wct_ctx* ctx, const uint8_t* stylized_dev, int Ho, int Wo, const uint8_t* content_dev, int Hc,
                                 int Wc, int B, uint8_t* out_dev);
/* Guided smoothing (He, Sun, Tang, "Guided Image Filtering", ECCV 2010; the smoothing step of the fast variant of Li et al. 2018,
 * "A Closed-form Solution to Photorealistic Image Stylization"): the stylized frame filtered with the grey content as guide --
 * the frame keeps an edge wherever the content has one and is averaged wherever the content is flat.  Integers only (the rule
 * and its bounds: csrc/guided_rule.h) -- stylized s [Ho][Wo][3], content c [Hc][Wc][3], Ho >= Hc, Wo >= Wc, radius r in 1 .. 64,
 * eps_q in 1 .. 65025 (grey levels squared: round(eps * 65025) of the usual [0,1]^2 eps, at least 1):
 *   rdiv(a, b) = floor((2a + b) / (2b))                                  (nearest, halves up, a true floor for negative a)
 *   I(y, x)    = (77 p.R + 150 p.G + 29 p.B + 128) >> 8, p = c[min(y, Hc - 1)][min(x, Wc - 1)]    (the clamp of wct_content_colors)
 *   window     = rows max(0, y - r) .. min(Ho - 1, y + r) x the same in x, n pixels (the border-normalised box of He et al.)
 *   pass 1, per channel: SI, SII, Sp, SIp = the window sums of I, I^2, s.ch, I s.ch
 *              a_q = rdiv((n SIp - SI Sp) 2^12, n SII - SI^2 + eps_q n^2),  b_q = rdiv(Sp 2^12 - a_q SI, n)
 *   pass 2:    out.ch = clamp(rdiv(I sum a_q + sum b_q, n 2^12), 0, 255), the sums over the same window
 * A constant frame comes back exactly; the result stays within 0.54 of the float64 filter with the same guide and box.
 * wct_guided_filter: host pointers, blocking.  wct_guided_filter_batch_dev: device pointers, B = 1 .. 32 frames [B][Ho][Wo][3]
 *   and contents [B][Hc][Wc][3], two launches, asynchronous on the ctx stream; out_dev may be stylized_dev (in place).  The
 *   24 B per pixel between the passes live in a workspace of the ctx.
 * wct_set_guided: the radius and eps_q of WCT_FLAG_GUIDED (initially 8 and 650).  With WCT_FLAG_IMAGES_F32 the float content is
 *   taken under the output rule uint8(clip(x, 0, 1) * 255.f), as the colour op takes it.
 * Ho < Hc, Wo < Wc, a null pointer, B outside 1 .. 32, a radius or eps_q out of range, or B * Ho * Wo * 3 >= 2^31 is
 * WCT_STATUS_ARG and leaves the ctx (and the flag's settings) as they were.
 * The colour guide (He et al., eqs. 19-21; the rule, its bounds and its distance from the float64 filter: csrc/guided_color_rule.h).
 * The grey guide is blind to an edge between two colours of equal luminance and blurs the frame across it; with WCT_GUIDE_COLOR
 * the guide is the three content bytes I = (p.R, p.G, p.B) of the same clamped pixel, and pass 1 solves a 3 x 3 system (F = 4;
 * i, j the guide's channels, ch the frame's; U the unit matrix; >> the arithmetic shift):
 *   pass 1:    the 21 window sums S_i, S_ij (i <= j), S_ch, S_i,ch
 *              V_ij = rdiv(2^F (n S_ij - S_i S_j), n^2),  M = V + 2^F eps_q U,  c_i,ch = rdiv(2^F (n S_i,ch - S_i S_ch), n^2)
 *              adj = the adjugate of M,  det = sum_j M_0j adj_0j,  u_i,ch = sum_j adj_ij c_j,ch,  k = max(0, bitlength(det) - 43)
 *              a_q[i][ch] = rdiv((u_i,ch >> k) 2^12, det >> k),  b_q[ch] = rdiv(S_ch 2^12 - sum_i a_q[i][ch] S_i, n)
 *   pass 2:    out.ch = clamp(rdiv(sum_i I_i sum a_q[i][ch] + sum b_q[ch], n 2^12), 0, 255)
 * A constant frame comes back exactly.  48 B per pixel between the passes.
 * wct_guided_filter_guide, wct_guided_filter_guide_batch_dev: the two calls above with the guide as one more argument;
 *   WCT_GUIDE_GREY gives their bytes.  wct_set_guided_guide: the guide of WCT_FLAG_GUIDED (initially WCT_GUIDE_GREY); every
 *   flagged frame equals wct_guided_filter_guide(the unflagged frame, the content, that guide) bit for bit.  A guide that is
 *   neither value is WCT_STATUS_ARG and keeps the earlier setting.
 * Not served: the banded / texture / wrap calls, radii above 64, a guide other than the content.  (The subsampled "fast guided
 * filter" is wct_guided_upsample below.) */
int wct_guided_filter(wct_ctx* ctx, const uint8_t* stylized, int Ho, int Wo, const uint8_t* content, int Hc, int Wc, int radius,
                      int eps_q, uint8_t* out);
int wct_guided_filter_batch_dev(wct_ctx* ctx, const uint8_t* stylized_dev, int Ho, int Wo, const uint8_t* content_dev, int Hc, int Wc,
                                int B, int radius, int eps_q, uint8_t* out_dev);
int wct_set_guided(wct_ctx* ctx, int radius, int eps_q);
int wct_guided_filter_guide(wct_ctx* ctx, const uint8_t* stylized, int Ho, int Wo, const uint8_t* content, int Hc, int Wc, int radius,
                            int eps_q, int guide, uint8_t* out);
int wct_guided_filter_guide_batch_dev(wct_ctx* ctx, const uint8_t* stylized_dev, int Ho, int Wo, const uint8_t* content_dev, int Hc,
                                      int Wc, int B, int radius, int eps_q, int guide, uint8_t* out_dev);
int wct_set_guided_guide(wct_ctx* ctx, int guide);
/* Temporal guided smoothing: the grey-guide filter above with its box extended along time, against the flicker of a video whose
 * frames were stylized one by one.  Where the content does not change between neighbouring frames the stylized frames are averaged
 * over them; where it moves, the guide's variance in the window is large and the result follows the guide, as at a spatial edge.
 * The rule and its bounds: csrc/guided_time_rule.h.  A clip is F frames, s [F][Ho][Wo][3] and c [F][Hc][Wc][3]; T = frames_t is
 * the number of frames on each side, 0 .. 3; I(f, y, x) is the guide above of content frame f:
 *   window     = the box above at (y, x) in each frame of max(0, f - T) .. min(F - 1, f + T): cut at the clip's ends as it is cut
 *                at the image's borders, n = rows x columns x frames of it
 *   pass 1:    SI, SII, Sp, SIp over that window; a_q, b_q of (f, y, x) by the formulas above with this n
 *   pass 2:    out.ch(f, y, x) = clamp(rdiv(I(f, y, x) sum a_q + sum b_q, n 2^12), 0, 255), the sums over the same window
 * T = 0 is wct_guided_filter_batch_dev, bit for bit; a one-frame clip is too, whatever T.  Parameters: those of wct_guided_filter,
 * 0 <= T <= 3, and (2r + 1)^2 (2T + 1) <= 33025 (= floor(2^31 / 65025): every window sum of pass 1 stays below 2^31), which is
 * r <= 64 / 51 / 40 / 33 at T = 0 / 1 / 2 / 3 -- wct_guided_time_max_radius(T), 0 for a T outside 0 .. 3.
 * wct_guided_filter_time: host pointers, blocking, the whole clip, F = 1 .. 32.
 * wct_guided_filter_time_batch_dev: device pointers, two launches, asynchronous on the ctx stream; F = 1 .. 32 resident frames,
 *   0 <= f0 < f1 <= F; writes out_dev [f1 - f0][Ho][Wo][3], the filtered frames f0 .. f1 - 1 of THIS clip of F frames.  out_dev may
 *   be stylized_dev + f0 Ho Wo 3 (in place).  The 24 B per pixel of the F frames live in the workspace of wct_guided_filter.
 *   A frame depends on the stylized frames up to 2T away (pass 2 reads coefficients T frames away, each made from frames T further):
 *   a caller that wants the bytes of a longer video gives 2T real frames of halo on each side of [f0, f1), except at the video's
 *   own ends.  A halo of T frames does not give them.
 * A null pointer, F outside 1 .. 32, a range that is not 0 <= f0 < f1 <= F, Ho < Hc, Wo < Wc, parameters outside the above, or
 * F * Ho * Wo * 3 >= 2^31 is WCT_STATUS_ARG with a message and leaves the ctx usable.
 * The colour guide along time is wct_guided_filter_time_guide below.
 * Not served: T above 3, motion compensation of any kind (a flat region that pans has its stylized
 * texture averaged along time), WCT_FLAG_GUIDED along time (a frame would need frames that come after it). */
int wct_guided_filter_time(wct_ctx* ctx, const uint8_t* stylized, int Ho, int Wo, const uint8_t* content, int Hc, int Wc, int F,
                           int radius, int eps_q, int frames_t, uint8_t* out);
int wct_guided_filter_time_batch_dev(wct_ctx* ctx, const uint8_t* stylized_dev, int Ho, int Wo, const uint8_t* content_dev, int Hc,
                                     int Wc, int F, int radius, int eps_q, int frames_t, int f0, int f1, uint8_t* out_dev);
int wct_guided_time_max_radius(int frames_t);
/* Temporal guided smoothing along camera motion: the filter above with one global integer translation per frame, so that a clip
 * that pans is averaged along the motion, not across it (with equal windows a textured scene that moves looks like an edge
 * everywhere along time).  The rule and its bounds: csrc/guided_motion_rule.h.
 *   positions  pos [F][2] int32 (py, px), host memory; pos[0] is arbitrary, only differences are used.  The scene point at pixel
 *              (y, x) of frame f is at pixel (y + pos[g][0] - pos[f][0], x + pos[g][1] - pos[f][1]) of frame g.  Every step
 *              |pos[f + 1] - pos[f]| is at most 16 on both axes.
 *   window     of (f, y, x): in each frame g of max(0, f - T) .. min(F - 1, f + T) the (2r + 1)^2 box centred at the shifted pixel
 *              (y + Dy, x + Dx), cut at the image's borders; it may be empty.  ext(c, L, r) = max(0, min(L - 1, c + r) -
 *              max(0, c - r) + 1);  n = sum over g of ext(y + Dy, H, r) ext(x + Dx, W, r)
 *   pass 1:    SI, SII, Sp, SIp over that window; a_q, b_q of (f, y, x) by the formulas above with this n
 *   pass 2:    out.ch(f, y, x) = clamp(rdiv(I(f, y, x) sum a_q + sum b_q, n 2^12), 0, 255), the sums over the same window
 * Equal positions give wct_guided_filter_time_batch_dev's bytes.  The own frame gives n >= 1 and n <= (2r + 1)^2 (2T + 1): the
 * parameters, the radius limits and the 2T halo of a longer video are those above.
 * wct_guided_filter_motion: host pointers, blocking, the whole clip, F = 1 .. 32.
 * wct_guided_filter_motion_batch_dev: device frames, host positions (read before the call returns), two launches, asynchronous on
 *   the ctx stream; frames f0 .. f1 - 1 of THIS clip; out_dev may be stylized_dev + f0 Ho Wo 3.
 * The estimator: for every pair of consecutive contents the step d = (dy, dx), |dy|, |dx| <= range, that minimises the mean absolute
 * difference of the grey guides I (at content size) over the samples (y, x), both even, inside frame f with (y + dy, x + dx) inside
 * frame f + 1:  SAD(d) = sum |I_f(y, x) - I_{f+1}(y + dy, x + dx)|, cnt(d) their number; d wins over d' when SAD(d) cnt(d') <
 * SAD(d') cnt(d) (int64), and at equality the smaller (dy^2 + dx^2, dy, dx) wins: a flat or an unchanged pair gives (0, 0).
 * pos[0] = (0, 0), pos[f + 1] = pos[f] + d_f.  range is 1 .. 16, Hc and Wc at least 4 range, Hc Wc <= 2^28.  A scene cut yields an
 * arbitrary step, which the filter treats like any edge.
 * wct_motion_global: host contents [F][Hc][Wc][3], blocking -> pos_out [F][2] int32, host memory.
 * wct_motion_global_batch_dev: device contents; three launches on the ctx stream, then it BLOCKS on its 8 F byte result (pos_out
 *   is host memory).  It uses the workspace of the guided ops: enqueue it before the filter of the same clip, not between its
 *   passes (a ctx serves one stream, so this is the natural order).
 * A null pointer, what wct_guided_filter_time refuses, a step above 16, a range outside 1 .. 16, Hc or Wc below 4 range or
 * Hc Wc > 2^28 is WCT_STATUS_ARG with a message that names it, and leaves the ctx usable.
 * The colour guide along time and along motion is wct_guided_filter_time_guide below.
 * Not served: per-block or dense motion, sub-pixel shifts, rotation and zoom. */
int wct_motion_global(wct_ctx* ctx, const uint8_t* contents, int Hc, int Wc, int F, int range, int32_t* pos_out);
int wct_motion_global_batch_dev(wct_ctx* ctx, const uint8_t* content_dev, int Hc, int Wc, int F, int range, int32_t* pos_out);
int wct_guided_filter_motion(wct_ctx* ctx, const uint8_t* stylized, int Ho, int Wo, const uint8_t* content, int Hc, int Wc, int F,
                             int radius, int eps_q, int frames_t, const int32_t* pos, uint8_t* out);
int wct_guided_filter_motion_batch_dev(wct_ctx* ctx, const uint8_t* stylized_dev, int Ho, int Wo, const uint8_t* content_dev, int Hc,
                                       int Wc, int F, int radius, int eps_q, int frames_t, const int32_t* pos, int f0, int f1,
                                       uint8_t* out_dev);
/* Temporal guided smoothing under a chosen guide: the two temporal filters above with the guide as one more argument, and with
 * WCT_GUIDE_COLOR the colour guide along time -- the 3 x 3 rule of wct_guided_filter_guide over the 3-D, optionally shifted, window
 * of wct_guided_filter_motion, for a video whose content has edges between colours of equal luminance (which the grey guide
 * blurs) and flickers on its flat areas (which the per-frame colour guide leaves).  The rule and its bounds:
 * csrc/guided_color_time_rule.h.  Clip, T, positions, window and n are those of wct_guided_filter_motion; pos == NULL means no
 * motion (every position equal), the window and n of wct_guided_filter_time.  I(f, y, x) = (p.R, p.G, p.B) of the clamped content
 * pixel of frame f:
 *   pass 1:    the 21 window sums S_i, S_ij (i <= j), S_ch, S_i,ch over that window; V, M, c, adj, det, u, k, a_q[i][ch] and
 *              b_q[ch] of (f, y, x) by the formulas of the colour guide above with this n
 *   pass 2:    out.ch(f, y, x) = clamp(rdiv(sum_i I_i(f, y, x) sum a_q[i][ch] + sum b_q[ch], n 2^12), 0, 255), the sums over the
 *              same window
 * T = 0, or a one-frame clip, is wct_guided_filter_guide_batch_dev with WCT_GUIDE_COLOR, bit for bit.  Equal positions, whatever
 * their value, give the bytes of pos == NULL.  A constant clip comes back exactly.  Parameters, radius limits (r <= 64 / 51 / 40 /
 * 33 at T = 0 .. 3, n <= 33025), the steps of at most 16 and the 2T halo of a longer video are those above; the result stays
 * within the distance of csrc/guided_color_rule.h (no n in it) of the float64 filter on the same window.
 * WCT_GUIDE_GREY gives the bytes of wct_guided_filter_time (pos == NULL) or wct_guided_filter_motion (otherwise).
 * wct_guided_filter_time_guide: host pointers, blocking, the whole clip, F = 1 .. 32.
 * wct_guided_filter_time_guide_batch_dev: device frames, host positions (read before the call returns) or NULL, two launches,
 *   asynchronous on the ctx stream; frames f0 .. f1 - 1 of THIS clip; out_dev may be stylized_dev + f0 Ho Wo 3.  The 48 B per
 *   pixel of the F frames (twice the grey guide's) live in the workspace of wct_guided_filter, sized before any launch.
 * A guide that is neither value, a null image pointer, or what wct_guided_filter_time / wct_guided_filter_motion refuse is
 * WCT_STATUS_ARG with their message and leaves the ctx usable; a workspace that cannot be had is the allocation's own status.
 * Not served: the colour guide along time under upsampling, fp32 contents, T above 3, per-block or sub-pixel motion, a motion
 * estimator on colour (wct_motion_global works on the grey guide). */
int wct_guided_filter_time_guide(wct_ctx* ctx, const uint8_t* stylized, int Ho, int Wo, const uint8_t* content, int Hc, int Wc, int F,
                                 int radius, int eps_q, int frames_t, int guide, const int32_t* pos, uint8_t* out);
int wct_guided_filter_time_guide_batch_dev(wct_ctx* ctx, const uint8_t* stylized_dev, int Ho, int Wo, const uint8_t* content_dev, int Hc,
                                           int Wc, int F, int radius, int eps_q, int frames_t, int guide, const int32_t* pos, int f0,
                                           int f1, uint8_t* out_dev);
/* On-device resize (the reference's resize_to, utils.py:55-67, behind --content-size, stylize_video.py:29; webcam.py:163,189
 * resizes every frame by --scale): img [H][W][3] uint8 -> [h][w][3] uint8, the bytes of Pillow's Image.resize((w, h), Image.BILINEAR).
 * Pillow's 8-bit resampler is an integer rule.  Per axis (`in` the input length, `out` the output length; everything up to the
 * integer taps is IEEE double, evaluated in exactly this order, without fused multiply-adds):
 *   scale = in / out;  fs = max(scale, 1.0);  support = fs;  ksize = (int)ceil(support) * 2 + 1
 *   for xx in 0 .. out-1:
 *     center = (xx + 0.5) * scale
 *     xmin = max((int)(center - support + 0.5), 0)                        (int): truncation
 *     n    = min((int)(center + support + 0.5), in) - xmin
 *     w[x] = tri((x + xmin - center + 0.5) * (1.0 / fs)),  x in 0 .. n-1,   tri(t) = |t| < 1 ? 1 - |t| : 0
 *     ww = sum w[x] in order;  if ww != 0: w[x] /= ww
 *     k[x] = (int)(0.5 + w[x] * 4194304.0)                                (22 bits; bilinear taps are never negative)
 *   byte = clamp((2097152 + sum_x k[x] * src[xmin + x]) >> 22, 0, 255)    int32 throughout
 * The image is resized along x first, into a uint8 intermediate of H x w (it stays on the chip), which is then resized along y.
 * An axis whose length does not change reproduces its bytes; h == H and w == W is a copy.
 * wct_resize: host pointers, blocking.  wct_resize_batch_dev: device pointers, B = 1 .. 32 frames [B][H][W][3] ->
 *   [B][h][w][3] in one launch, asynchronous on the ctx stream, no workspace; out_dev must not overlap in_dev.  The tap tables
 *   of the last geometry (H, W, h, w) stay in the ctx: a call with another geometry waits for the stream while it replaces them.
 * A null pointer, a size < 1, B outside 1 .. 32, input or output bytes >= 2^31 in one call (every index is a 32-bit one), an
 * overlap, or a vertical reduction so strong that the input rows one output row taps do not fit the kernel's 16 KB of LDS at
 * min(w, 64) columns (H / h above about 42 at w >= 64) is WCT_STATUS_ARG and leaves the ctx usable. */
int wct_resize(wct_ctx* ctx, const uint8_t* img, int H, int W, int h, int w, uint8_t* out);
int wct_resize_batch_dev(wct_ctx* ctx, const uint8_t* in_dev, int H, int W, int B, int h, int w, uint8_t* out_dev);

/* ---- the hot path: WCT.predict (wct.py:70-106) -------------------------------------
 * levels: relu levels in pipeline order, e.g. {5,4,3,2,1}.  Output size: wct_output_size. */
/* Images must keep a feature map of at least 2x2 at the deepest level (every conv reflect-pads by one pixel, and
 * tf.pad REFLECT refuses a 1-pixel map just the same): H, W >= 2^(level-1) + 1, else WCT_STATUS_ARG. */
int wct_output_size(int Hc, int Wc, const int* levels, int n_levels, int* Ho, int* Wo);
int wct_stylize(wct_ctx* ctx, const uint8_t* content, int Hc, int Wc,
                const uint8_t* style, int Hs, int Ws,
                const int* levels, int n_levels, float alpha, unsigned flags,
                uint8_t* out);
/* WCT.predict with a style mix at every level (see wct_transform_mix): styles[k] is an Hs[k] x Ws[k] image (sizes may differ),
 * lambda_k = weights[k] / sum(weights).  Every level applies the mix; each level encodes the clipped decode of the level before.
 * Honours WCT_FLAG_MODE_NP, WCT_FLAG_ADAIN, WCT_FLAG_IMAGES_F32 (all K images), and WCT_FLAG_SWAP5 only at K = 1 (style-swap is
 * not linear: K > 1 is WCT_STATUS_ARG); K = 1, and one-hot weights, give wct_stylize's frame bit for bit. */
int wct_stylize_mix(wct_ctx* ctx, const uint8_t* content, int Hc, int Wc, const uint8_t* const* styles, const int* Hs,
                    const int* Ws, int K, const float* weights, const int* levels, int n_levels, float alpha, unsigned flags,
                    uint8_t* out);
/* WCT.predict with spatial control at every level (see wct_transform_masked): mask [Hc][Wc] labels 0 .. K - 1, styles[k] an
 * Hs[k] x Ws[k] image (sizes may differ).  At level l (stride s = 2^(l-1)) feature pixel (i, j) of the h x w map has the label
 * mask[min(i s, Hc - 1)][min(j s, Wc - 1)] (the clamp: a later level's input, the decode of the level before, can be larger than
 * the content).  A label with fewer than 2 pixels at a level keeps that level's features.  Honours WCT_FLAG_MODE_NP,
 * WCT_FLAG_ADAIN, WCT_FLAG_IMAGES_F32 (all K + 1 images), and WCT_FLAG_SWAP5 only at K = 1 (style-swap is not a per-region
 * affine map: K > 1 is WCT_STATUS_ARG); WCT_FLAG_STYLE_SHARED is WCT_STATUS_ARG.  K = 1 gives wct_stylize's frame bit for bit. */
int wct_stylize_masked(wct_ctx* ctx, const uint8_t* content, int Hc, int Wc, const uint8_t* mask, const uint8_t* const* styles,
                       const int* Hs, const int* Ws, int K, const int* levels, int n_levels, float alpha, unsigned flags,
                       uint8_t* out);
/* batched, device-resident variant: B independent pairs (same sizes), content [B][Hc][Wc][3],
 * style [B][Hs][Ws][3], out [B][Ho][Wo][3], all device pointers; asynchronous on the ctx
 * stream (call wct_sync).  This is what bench.py times. */
int wct_stylize_batch_dev(wct_ctx* ctx, const uint8_t* content_dev, int Hc, int Wc,
                          const uint8_t* style_dev, int Hs, int Ws, int B,
                          const int* levels, int n_levels, float alpha, unsigned flags,
                          uint8_t* out_dev);

/* ---- prepared styles: the style side once, any number of contents -------------------------
 * Every call above takes a style IMAGE and redoes the whole style side from it -- the style encoder pass, the style statistics
 * and covariance of every level, the style eigendecompositions and colouring matrices -- as the reference does: predict() feeds
 * the style through the graph once per call (wct.py:70-106), and stylize_video.py calls it once per frame of a video whose style
 * never changes (stylize_video.py:88-121).  A wct_style is that style side, computed once and owned by the ctx.
 *
 * wct_style_prepare: style is an Hs x Ws x 3 host image (uint8, or float32 in [0,1] with WCT_FLAG_IMAGES_F32); levels is the SET
 *   of relu levels the handle serves (order and repeats do not matter).  Blocking.  The handle keeps the image on the device
 *   and, per level, a small cache of states -- colouring matrix and style mean (WCT), mean and variance (AdaIN) -- keyed by what
 *   their bits depend on: the partial-sum layout of the (content, style) pair (it follows the LARGER of the two feature maps)
 *   and the mode (wct_tf, wct_np, AdaIN).  This call fills the entries for a content as large as the style, in the mode that
 *   WCT_FLAG_ADAIN / WCT_FLAG_MODE_NP name; a stylize call that needs another key computes it from the kept image in front of its
 *   content chain, keeps it (4 keys per level, oldest out) and reuses it afterwards.  So one handle serves any content size,
 *   either mode, AdaIN and every alpha (alpha enters in the blend and the bias only, which are not part of a state).
 *   If a style eigensolve does not converge: WCT_STATUS_NOCONV and no handle (*out = NULL); a state computed later inside a
 *   stylize call is checked the same way before it is kept, and that call then returns WCT_STATUS_NOCONV without a frame.
 * wct_style_free: waits for the ctx stream, then releases the handle; NULL, a freed or a foreign handle is a no-op.
 *   wct_destroy frees what is left.
 * wct_stylize_prepared           = wct_stylize's frame, bit for bit, for the same images, levels, alpha and flags;
 * wct_stylize_prepared_batch_dev = wct_stylize_batch_dev with WCT_FLAG_STYLE_SHARED, bit for bit (asynchronous like it, except
 *   that a call which has to compute a new state blocks while it does);
 * wct_stylize_prepared_mix       = wct_stylize_mix, bit for bit (so K = 1 and one-hot weights give wct_stylize's frame): new
 *   weights for the same K handles cost one content side, one mix of K cached matrices and one apply.
 * flags: WCT_FLAG_MODE_NP, WCT_FLAG_ADAIN, and WCT_FLAG_IMAGES_F32 for the CONTENT (the style is what it was when prepared).
 *   WCT_FLAG_SWAP5 is WCT_STATUS_ARG (style-swap needs the style's relu5_1 map and patches, not its moments), and so is
 *   WCT_FLAG_STYLE_SHARED, as in the mix / masked calls.  The levels of a call (any order, repeats allowed) must all be in the
 *   handle's set, else WCT_STATUS_ARG.  A handle that is not live in THIS ctx -- freed, or another context's -- is
 *   WCT_STATUS_STATE; it is recognised by its address and never dereferenced.  A refusal leaves the ctx usable. */
typedef struct wct_style wct_style;
int  wct_style_prepare(wct_ctx* ctx, const uint8_t* style, int Hs, int Ws, const int* levels, int n_levels, unsigned flags,
                       wct_style** out);
void wct_style_free(wct_ctx* ctx, wct_style* style);
int  wct_stylize_prepared(wct_ctx* ctx, const uint8_t* content, int Hc, int Wc, const wct_style* style, const int* levels,
                          int n_levels, float alpha, unsigned flags, uint8_t* out);
int  wct_stylize_prepared_batch_dev(wct_ctx* ctx, const uint8_t* content_dev, int Hc, int Wc, int B, const wct_style* style,
                                    const int* levels, int n_levels, float alpha, unsigned flags, uint8_t* out_dev);
int  wct_stylize_prepared_mix(wct_ctx* ctx, const uint8_t* content, int Hc, int Wc, const wct_style* const* styles, int K,
                              const float* weights, const int* levels, int n_levels, float alpha, unsigned flags,
                              uint8_t* out);
/* Guided upsampling (He, Sun, "Fast Guided Filter", 2015): stylize small, deliver at the content's size.  The guided filter's
 * output a I + b is a linear function of the guide per pixel with smooth coefficients: they are computed on the small frame,
 * interpolated, and evaluated against the FULL content, which returns every edge of the content at full sharpness.  Integers only
 * (the rule, its bounds and the derivation of its distance from the float64 filter: csrc/guided_up_rule.h) -- s [h][w][3] the small
 * stylized frame, c [hc][wc][3] the small content (hc <= h, wc <= w, the clamp above), C [H][W][3] the full content (H >= hc,
 * W >= wc), radius and eps_q as in wct_guided_filter, in pixels of the small frame:
 *   1. a_q, b_q on h x w: pass 1 of wct_guided_filter, unchanged
 *   2. per small pixel and channel, n, SA = sum a_q, SB = sum b_q of pass 2's window:  am = rdiv(SA, n), bm = rdiv(SB, n)
 *      (2^-12 units); only rows < hc and columns < wc are read afterwards (the rest of s is padding)
 *   3. per axis, N the full length, m the small content length (hc or wc), P the full coordinate (half-pixel centres):
 *        t = clamp((2P + 1) m - N, 0, 2N (m - 1)),  p0 = t div 2N,  f = rdiv((t - p0 2N) 256, 2N) (0 .. 256),  p1 = min(p0 + 1, m - 1)
 *      the axis weights are 256 - f and f; with w_k their four products (sum 65536) and I the guide of C[Y][X]:
 *        v = sum_k w_k (am_k I + bm_k),   out = clamp((v + 2^27) >> 28, 0, 255)        (>> arithmetic: no division at full size)
 * A constant small frame comes back as that constant at every full size.  At H = hc, W = wc the result is within 1 grey level of
 * wct_guided_filter, NOT bit-equal to it (am, bm are rounded once more).  Before the clamp the result is within
 * 0.5 + 256 2^-12 + D 2^-8 of the float64 fast guided filter with the same guide, box and half-pixel bilinear map, D the spread
 * (max - min) of the pixel's four (am_k I + bm_k) 2^-12.
 * wct_guided_upsample: host pointers, blocking.  wct_guided_upsample_batch_dev: device pointers, B = 1 .. 32 frames [B][h][w][3],
 *   contents [B][hc][wc][3] and [B][H][W][3], out [B][H][W][3]; three launches (pass 1, the means, the full-size pass),
 *   asynchronous on the ctx stream; out must not overlap an input.  The 48 B per SMALL pixel between the launches live in the
 *   workspace of wct_guided_filter.
 * wct_stylize_prepared_upsampled / _batch_dev: full contents [B][H][W][3], a prepared style and a working size (hc, wc): the
 *   contents are resized on the device (wct_resize_batch_dev; H == hc && W == wc skips it), stylized by the prepared batch chain
 *   and quantised by the chain's own rule, upsampled against the full contents still resident, and with WCT_FLAG_CONTENT_COLORS
 *   recoloured at full size against the full content.  The frame [B][H][W][3] equals wct_resize -> wct_stylize_prepared ->
 *   wct_guided_upsample -> wct_content_colors bit for bit.  flags: those of wct_stylize_prepared; WCT_FLAG_GUIDED is
 *   WCT_STATUS_ARG, and so is WCT_FLAG_IMAGES_F32 unless H == hc && W == wc (the resize takes uint8).
 * WCT_STATUS_ARG with a message that names the argument, the ctx usable afterwards: H < hc or W < wc, h < hc or w < wc, a null
 *   pointer, B outside 1 .. 32, a radius or eps_q out of range, B * H * W * 3 >= 2^31, an overlap, and whatever wct_resize refuses
 *   (its LDS limit near H / hc = 42).
 * Not served: mixes, masks and strength maps in the fused driver (the stand-alone op takes any frame); down-scaling; ratios the
 * resize refuses; full contents of 2^31 bytes and more.  (The colour guide under upsampling is served by the wct_*_guide calls
 * below, the temporal box under upsampling by wct_guided_upsample_time.) */
int  wct_guided_upsample(wct_ctx* ctx, const uint8_t* stylized, int h, int w, const uint8_t* content_small, int hc, int wc,
                         const uint8_t* content_full, int H, int W, int radius, int eps_q, uint8_t* out);
int  wct_guided_upsample_batch_dev(wct_ctx* ctx, const uint8_t* stylized_dev, int h, int w, const uint8_t* content_small_dev, int hc,
                                   int wc, const uint8_t* content_full_dev, int H, int W, int B, int radius, int eps_q,
                                   uint8_t* out_dev);
int  wct_stylize_prepared_upsampled(wct_ctx* ctx, const uint8_t* content, int H, int W, int hc, int wc, const wct_style* style,
                                    const int* levels, int n_levels, float alpha, unsigned flags, int radius, int eps_q,
                                    uint8_t* out);
int  wct_stylize_prepared_upsampled_batch_dev(wct_ctx* ctx, const uint8_t* content_dev, int H, int W, int B, int hc, int wc,
                                              const wct_style* style, const int* levels, int n_levels, float alpha, unsigned flags,
                                              int radius, int eps_q, uint8_t* out_dev);
/* Guided upsampling with a choice of guide: the four calls above with `int guide` as one more argument.  WCT_GUIDE_GREY gives their
 * bytes through their kernels.  WCT_GUIDE_COLOR is the upsampling rule with the coefficients of the colour-guide filter, which
 * keeps an edge between two colours of equal luminance at full sharpness (the rule, its bounds and the derivation of its distance
 * from the float64 filter: csrc/guided_up_color_rule.h).  Notation as above:
 *   1. a_q[i][p], b_q[p] on h x w: pass 1 of wct_guided_filter_guide(..., WCT_GUIDE_COLOR), unchanged (12 int32 per small pixel)
 *   2. per small pixel, n, SA_ip = sum a_q[i][p], SB_p = sum b_q[p] of pass 2's window:  am[i][p] = rdiv(SA_ip, n),
 *      bm[p] = rdiv(SB_p, n)  (2^-12 units, |am| <= 288400, |bm| <= 2.22e8); only rows < hc and columns < wc are read afterwards
 *   3. the axis taps and weights of step 3 above, unchanged; with I_i the three channels of C[Y][X]:
 *        v_p = sum_k w_k (sum_i am_k[i][p] I_i + bm_k[p]),   out_p = clamp((v_p + 2^27) >> 28, 0, 255)      (|v| < 2.91e13 < 2^45)
 * A constant small frame comes back as that constant at every full size.  At H = hc, W = wc the result is within 1 grey level of
 * wct_guided_filter_guide(..., WCT_GUIDE_COLOR), NOT bit-equal to it.  Before the clamp the result is within
 * 0.5 + 766 2^-12 + 765 2^-35 + D 2^-8 + E(eps_q) of the float64 fast guided filter with the colour guide (np.linalg.solve on the
 * small pair's window covariances, the same box and half-pixel bilinear map), D the spread of the pixel's four corner values and
 * E(eps_q) = 255 sqrt(3) 2^-5 (sqrt(3) + 191.25 / sqrt(eps_q)) / (eps_q - 3 2^-5) the worst case of the colour rule's covariance
 * quantisation: 0.0005 at eps_q = 65025, 0.2 at 650, above a grey level from eps_q of a few hundred downwards, where it is no
 * useful bound (measured: at most 0.55 at eps_q >= 7, up to 0.78 at eps_q = 1).
 * Three launches (the colour pass 1, the means of the twelve coefficient planes, the full-size pass); the 96 B per SMALL pixel
 * between them live in the workspace of wct_guided_filter (16-byte aligned): the colour guide adds no limit beyond that size.
 * wct_stylize_prepared_upsampled_guide / _batch_dev equal wct_resize -> wct_stylize_prepared -> wct_guided_upsample_guide ->
 * wct_content_colors bit for bit; WCT_FLAG_IMAGES_F32 only without a resize, as above.
 * WCT_STATUS_ARG: a guide that is neither of the two, with a message that names the argument; every refusal of the calls above,
 *   with the same words.
 * Not served: the colour guide along time (wct_guided_upsample_time takes the grey guide); mixes, masks and strength maps in the
 * fused driver; down-scaling; full contents of 2^31 bytes and more. */
int  wct_guided_upsample_guide(wct_ctx* ctx, const uint8_t* stylized, int h, int w, const uint8_t* content_small, int hc, int wc,
                               const uint8_t* content_full, int H, int W, int radius, int eps_q, int guide, uint8_t* out);
int  wct_guided_upsample_guide_batch_dev(wct_ctx* ctx, const uint8_t* stylized_dev, int h, int w, const uint8_t* content_small_dev,
                                         int hc, int wc, const uint8_t* content_full_dev, int H, int W, int B, int radius, int eps_q,
                                         int guide, uint8_t* out_dev);
int  wct_stylize_prepared_upsampled_guide(wct_ctx* ctx, const uint8_t* content, int H, int W, int hc, int wc, const wct_style* style,
                                          const int* levels, int n_levels, float alpha, unsigned flags, int radius, int eps_q,
                                          int guide, uint8_t* out);
int  wct_stylize_prepared_upsampled_guide_batch_dev(wct_ctx* ctx, const uint8_t* content_dev, int H, int W, int B, int hc, int wc,
                                                    const wct_style* style, const int* levels, int n_levels, float alpha,
                                                    unsigned flags, int radius, int eps_q, int guide, uint8_t* out_dev);
/* Temporal guided upsampling: guided upsampling above with the temporal box of wct_guided_filter_time, optionally along camera
 * motion (wct_guided_filter_motion), where the coefficients are formed -- on the SMALL frames.  Video stylized at a small working
 * size and delivered at its own size, without the flicker of the per-frame filter.  The rule, its bounds, identities and the
 * derivation of its distance from the float64 filter: csrc/guided_up_time_rule.h.  A clip is F frames: s [F][h][w][3] the small
 * stylized frames, c [F][hc][wc][3] the small contents, C [.][H][W][3] the full contents; T = frames_t is 0 .. 3; pos [F][2] int32
 * (py, px) are positions in pixels of the small frame as in wct_guided_filter_motion, host memory, or NULL: equal positions.
 *   1. a_q, b_q of (f, y, x): pass 1 of wct_guided_filter_motion on the small clip, unchanged -- the sums over the window of
 *      (f, y, x), in each frame g of max(0, f - T) .. min(F - 1, f + T) the (2r + 1)^2 box centred at the shifted pixel, n its
 *      pixels.  With pos NULL or equal positions that is pass 1 of wct_guided_filter_time.
 *   2. am = rdiv(SA, n), bm = rdiv(SB, n): SA, SB the sums of a_q, b_q over the SAME 3-D window and n its count  (2^-12 units)
 *   3. step 3 of wct_guided_upsample on frame f's own (am, bm) and frame f's full content, unchanged.  No other frame is read at
 *      full size.
 * |SA| < 33025 2^18 and |SB| < 2.3e12 (doubled plus n below 2^63), |am| < 2^18 and |bm| < 6.8e7 as in wct_guided_upsample: every bound
 * of step 3 holds unchanged, and so does the distance from the float64 filter with the same window, 0.5 + 256 2^-12 + D 2^-8.
 * T = 0, or F = 1 at any T, gives wct_guided_upsample_batch_dev's bytes.  A constant clip comes back as that constant.  At H = hc,
 * W = wc the result is within 1 grey level of wct_guided_filter_time / _motion.  The parameters are those of
 * wct_guided_filter_time: r <= 64 / 51 / 40 / 33 at T = 0 / 1 / 2 / 3.
 * wct_guided_upsample_time: host pointers, blocking, the whole clip, F = 1 .. 32; content_full and out are [F][H][W][3].
 * wct_guided_upsample_time_batch_dev: device frames, host positions (read before the call returns); F = 1 .. 32 resident SMALL
 *   frames, 0 <= f0 < f1 <= F; content_full_dev [f1 - f0][H][W][3] holds the full contents of the delivered frames f0 .. f1 - 1 ONLY,
 *   out_dev [f1 - f0][H][W][3] the delivered frames.  Three launches (pass 1 of the temporal or motion filter over frames
 *   max(0, f0 - T) .. min(F, f1 + T) - 1, the window means, the full-size pass of wct_guided_upsample), asynchronous on the ctx
 *   stream; out_dev must not overlap an input.  24 B per small pixel of the F frames and 24 B per small pixel of the delivered
 *   frames live in the workspace of wct_guided_filter.
 *   A frame depends on the small frames up to 2T away and on ONE full content, its own: a caller that wants the bytes of a longer
 *   video gives 2T real SMALL frames of halo on each side of [f0, f1), except at the video's own ends.  A halo of T does not.
 * WCT_STATUS_ARG with a message that names what was wrong, the ctx usable afterwards: a null image pointer, what
 *   wct_guided_filter_time refuses on the small clip (F, the range, h < hc or w < wc, T, the radius for that T, eps_q,
 *   F * h * w * 3 >= 2^31), what wct_guided_upsample refuses (H < hc or W < wc, (f1 - f0) * H * W * 3 >= 2^31), a step of pos above
 *   16 on either axis, an overlap.
 * Not served: the colour guide along time; a fused driver that keeps the full contents resident between the resize and the
 * upsampling; mixes, masks and strength maps under upsampling; T above 3; per-block, sub-pixel or non-translational motion; fp32
 * contents. */
int  wct_guided_upsample_time(wct_ctx* ctx, const uint8_t* stylized, int h, int w, const uint8_t* content_small, int hc, int wc,
                              const uint8_t* content_full, int H, int W, int F, int radius, int eps_q, int frames_t,
                              const int32_t* pos, uint8_t* out);
int  wct_guided_upsample_time_batch_dev(wct_ctx* ctx, const uint8_t* stylized_dev, int h, int w, const uint8_t* content_small_dev,
                                        int hc, int wc, const uint8_t* content_full_dev, int H, int W, int F, int radius, int eps_q,
                                        int frames_t, const int32_t* pos, int f0, int f1, uint8_t* out_dev);
/* Spatial control on prepared styles, and on a batch of frames with one label map each (a video with a segmentation per frame).
 * wct_stylize_prepared_masked = wct_stylize_masked's frame, bit for bit, for the same content, mask, levels, alpha and flags and
 *   the images the K handles were prepared from: host pointers, blocking, like wct_stylize_prepared.  It is the B = 1 case of
 * wct_stylize_prepared_masked_batch_dev: content_dev [B][Hc][Wc][3] and out_dev [B][Ho][Wo][3] are DEVICE pointers, masks_host
 *   [B][Hc][Wc] is on the HOST (the labels of every level and frame are counted there before any launch -- the counts size the
 *   launches and the slot layout, nothing is read back -- and the B maps are then uploaded once, by a copy enqueued on the ctx
 *   stream: keep masks_host valid until wct_sync), B = 1 .. 32, the K handles are shared by all frames.  Asynchronous on the ctx
 *   stream like wct_stylize_prepared_batch_dev; it blocks only while it computes a style state it does not hold.  Frame f is wct_stylize_prepared_masked(content f, mask f), bit for bit -- so also
 *   wct_stylize_masked's.  Per level the live (frame, region) pairs run in groups of at most 32 (one batched eigensolve each; the
 *   style slots are dead); a matrix's eigensystem does not depend on its batch, so the grouping does not show in the frames.
 * Per frame the semantics are wct_stylize_masked's: feature pixel (i, j) at stride s has the label mask[min(i s, Hc - 1)][min(j s,
 *   Wc - 1)], a label with fewer than 2 pixels at a level keeps that level's features, a label with none is skipped.
 * States: region k of frame f takes handle k's state under the key of (N_fk rows, style k) -- the key follows the LARGER of the
 *   region and the style map, so regions no larger than the style all share the state made by wct_style_prepare, and larger
 *   regions of different sizes need one state each.  A state that the running call uses is never evicted: a level's cache then
 *   holds more than 4 keys -- as many as the most demanding call needed, at most B per handle and level -- and keeps that size.
 * flags: WCT_FLAG_MODE_NP, WCT_FLAG_ADAIN, and WCT_FLAG_IMAGES_F32 for the content.  WCT_FLAG_SWAP5 and WCT_FLAG_STYLE_SHARED are
 *   WCT_STATUS_ARG; so are K outside 1 .. 8, a label >= K, and a level outside a handle's set.  A handle that is not live in this
 *   ctx is WCT_STATUS_STATE and never dereferenced.  A refusal leaves the ctx usable. */
int  wct_stylize_prepared_masked(wct_ctx* ctx, const uint8_t* content, int Hc, int Wc, const uint8_t* mask,
                                 const wct_style* const* styles, int K, const int* levels, int n_levels, float alpha,
                                 unsigned flags, uint8_t* out);
int  wct_stylize_prepared_masked_batch_dev(wct_ctx* ctx, const uint8_t* content_dev, int Hc, int Wc, int B,
                                           const uint8_t* masks_host, const wct_style* const* styles, int K, const int* levels,
                                           int n_levels, float alpha, unsigned flags, uint8_t* out_dev);

/* ---- style regions: a prepared style from a labelled part of its image --------------------
 * Spatial control gives every region of the CONTENT its own style, but each of those styles is a whole image.  Semantic matching
 * (sky from the sky of a painting; the label-matched transfer of Li et al. 2018) needs the other half: the style statistics of a
 * level from a selected part of the style image.  A style Hs x Ws x 3 comes with a uint8 label map [Hs][Ws] on the host.
 * Semantics (the content side's rule): at relu<l>_1, stride s = 2^(l - 1), feature pixel (i, j) of the style's h x w map has the
 *   label map[min(i s, Hs - 1)][min(j s, Ws - 1)]; the region of a label is the feature rows with that label, in pixel order; the
 *   style side of the level is what a whole-image handle computes, from those n rows alone: mean, covariance with 1 / (n - 1), the
 *   per-matrix cut-off, the colouring matrix, mean and variance for AdaIN.  The encoder always sees the whole image: only the rows
 *   that enter the statistics are selected (on the device: one compaction of the level's labels, then a gather of n C floats).
 *   A region needs at least 2 rows at EVERY level of the handle, for WCT and AdaIN alike.
 * wct_style_prepare_region: wct_style_prepare for the rows of `label` (0 .. 7; other values of the map just are not selected).
 *   The handle keeps the image AND the map on the device, and the rows of every level counted on the host; it is an ordinary
 *   wct_style -- every call that takes handles takes it, with no change on the content side -- whose state keys follow (content
 *   rows, region rows) instead of (content rows, h w).  A map that labels every pixel `label` gives wct_style_prepare's handle,
 *   bit for bit.  A region with fewer than 2 rows at a served level is WCT_STATUS_ARG (the message names the level and the count)
 *   and no handle.
 * wct_style_prepare_regions: K = 1 .. 8 regions of one image, labels 0 .. K - 1 (a label >= K in the map: WCT_STATUS_ARG): one
 *   upload, ONE encoder pass and ONE compaction per level for all K; the states are then filled region by region.  out[k] is the
 *   handle wct_style_prepare_region(label k) gives, bit for bit, or NULL (status OK) for a label with fewer than 2 rows at some
 *   level, which cannot carry a style.  The handles share the image and the map by reference count: each is freed by
 *   wct_style_free on its own, and refilled on a new key by its own encoder pass.  On an error no handle is made.
 * wct_style_rows: the rows a handle's statistics use at a level of its set (h w for a whole-image handle).
 * wct_transform_region / wct_adain_region = wct_transform / wct_adain on the rows of `label` of a style feature map hs x ws x C,
 *   labels [hs ws] one per row, selected on the device by the same launches: bit for bit wct_transform(content, style[labels ==
 *   label]).  Fewer than 2 rows: WCT_STATUS_ARG.
 * Refused with WCT_STATUS_ARG and a message, the ctx usable afterwards: a NULL map, WCT_FLAG_SWAP5, WCT_FLAG_STYLE_SHARED, K
 *   outside 1 .. 8, a label outside 0 .. 7, and a style past the limit of one launch, as for wct_style_prepare.  Not served: soft
 *   or weighted style regions, style-swap from a region, banded style images. */
int  wct_style_prepare_region(wct_ctx* ctx, const uint8_t* style, int Hs, int Ws, const uint8_t* map, int label, const int* levels,
                              int n_levels, unsigned flags, wct_style** out);
int  wct_style_prepare_regions(wct_ctx* ctx, const uint8_t* style, int Hs, int Ws, const uint8_t* map, int K, const int* levels,
                               int n_levels, unsigned flags, wct_style** out /* [K] */);
int  wct_style_rows(wct_ctx* ctx, const wct_style* style, int level, int* n);
int  wct_transform_region(wct_ctx* ctx, const float* content, int Nc, const float* style, int hs, int ws, int C,
                          const uint8_t* labels, int label, float alpha, int mode, float eps, float* out, int* sweeps_out);
int  wct_adain_region(wct_ctx* ctx, const float* content, int Nc, const float* style, int hs, int ws, int C, const uint8_t* labels,
                      int label, float alpha, float epsilon, float* out);

/* ---- video warm start: solve each frame from the previous frame's basis --------------------
 * stylize_video.py:112-135 calls predict() once per frame, and every call decomposes the frame's content covariances from
 * scratch although consecutive frames have almost the same ones.  A wct_warm holds, per relu level of its set, one C x C fp32
 * basis -- the eigenvectors of the content covariance of the LAST frame of the previous call, re-orthonormalised by one
 * Newton-Schulz step -- and a valid bit.  A call that takes a state with a valid basis V0 rotates every content covariance of
 * the level into it (A' = V0^T A V0, fp32), runs the same batched solver on A' from the identity, and composes V = V0 V'; all
 * the rest of the transform is unchanged.  Such frames are NOT bit-identical to the cold ones (they meet the same tolerances).
 *   - an invalid level (a fresh state, after wct_warm_reset, after a failure) solves cold: today's frames bit for bit;
 *   - all B frames of a batched call start from the same stored basis ("the previous frame" is the last frame of the previous
 *     call); given the same state a frame does not depend on the other frames of its call, and runs are bit-reproducible;
 *   - after the call the state holds the basis of frame B - 1 for every level.  The content size may change between calls; the
 *     set of levels of a stylize call must be the state's set, else WCT_STATUS_ARG;
 *   - a call whose eigensolves end in WCT_STATUS_NOCONV (from the call itself if it blocks, from wct_sync or the next blocking
 *     call after wct_stylize_prepared_batch_dev_warm) leaves every level of the state invalid: the next call is cold;
 *   - WCT_FLAG_ADAIN (no eigensolve) and WCT_FLAG_SWAP5 (not on handles) are WCT_STATUS_ARG.  A state that is not live in THIS
 *     ctx -- freed, or another context's -- is WCT_STATUS_STATE; it is recognised by its address and never dereferenced.  A
 *     refusal leaves the ctx usable.  wct_warm_free of NULL, a freed or a foreign state is a no-op; wct_destroy frees what is left.
 * wct_warm_basis: *valid and, if V_host is not NULL and the level is valid, its C x C basis (eigenvectors in columns, row-major).
 * wct_stylize_prepared_warm / wct_stylize_prepared_batch_dev_warm: wct_stylize_prepared / wct_stylize_prepared_batch_dev with a
 *   state (replacing the per-frame loop of stylize_video.py:112-135).
 * wct_transform_warm: the op-level twin of wct_transform (replacing the decompositions stylize_video.py:112-135 repeats per
 *   frame, ops.py:53-55,110,123) -- flags: WCT_FLAG_MODE_NP or 0 (wct_tf), eps the reference defaults; relu<level>_1 must be in
 *   the state's set and have C channels, else WCT_STATUS_ARG.  Only the content solve is warm; sweeps_out as in wct_transform.
 * The masked and the mix calls take no state. */
typedef struct wct_warm wct_warm;
int  wct_warm_create(wct_ctx* ctx, const int* levels, int n_levels, wct_warm** out);
void wct_warm_free(wct_ctx* ctx, wct_warm* warm);
int  wct_warm_reset(wct_ctx* ctx, wct_warm* warm);                      /* all levels invalid */
int  wct_warm_basis(wct_ctx* ctx, const wct_warm* warm, int level, int* valid, float* V_host /* C*C or NULL */);
int  wct_stylize_prepared_warm(wct_ctx* ctx, const uint8_t* content, int Hc, int Wc, const wct_style* style, const int* levels,
                               int n_levels, float alpha, unsigned flags, wct_warm* warm, uint8_t* out);
int  wct_stylize_prepared_batch_dev_warm(wct_ctx* ctx, const uint8_t* content_dev, int Hc, int Wc, int B, const wct_style* style,
                                         const int* levels, int n_levels, float alpha, unsigned flags, wct_warm* warm,
                                         uint8_t* out_dev);
int  wct_transform_warm(wct_ctx* ctx, const float* content, int Nc, const float* style, int Ns, int C, float alpha,
                        unsigned flags, wct_warm* warm, int level, float* out, int* sweeps_out);

/* ---- strength maps: a per-pixel style strength, blended in the apply ----------------------------
 * Li et al. 2017, sec. 4.2 gives one alpha per call; a strength map lets it vary over the image (keep a face untouched, fade the
 * style in from one side, feather the edge between "stylized" and "kept").  A map is a uint8 image smap[Hc][Wc] of the content's
 * size: 255 means the call's alpha, 0 keeps the content features.  At a level of stride s = 2^(level - 1), feature pixel (i, j)
 * reads v = smap[min(i s, Hc - 1)][min(j s, Wc - 1)] (the rule of the label maps), and its row leaves the transform as
 *   a = alpha * (float(v) / 255.f);   out = a * y + (1.f - a) * x            (float32, each operation rounded once, none fused)
 * with x the row's content features and y its transform at alpha = 1 (wct_tf, wct_np or AdaIN): ops.py:83,133,293 with alpha
 * replaced by a.  The statistics, covariance, eigensystem and colouring matrix of a level are those of the plain call over the
 * whole map; the map enters only the blend.  So v = 0 gives x bit for bit, and v = 255 with alpha = 1 the plain alpha = 1 row.
 * wct_transform_strength / wct_adain_strength: one level, host pointers -- wct_transform / wct_adain on content [Nc][C], the rows
 *   of an h x w feature map (Nc = h w, else WCT_STATUS_ARG), with smap [Hm][Wm] sampled at `stride`; sweeps_out as in wct_transform.
 * wct_stylize_prepared_strength: wct_stylize_prepared with a map [Hc][Wc]; host pointers, blocking.  It is the B = 1 case of
 * wct_stylize_prepared_strength_batch_dev: content_dev [B][Hc][Wc][3], smaps_dev [B][Hc][Wc] and out_dev [B][Ho][Wo][3] are
 *   DEVICE pointers, B = 1 .. 32, one map per frame.  Nothing of a map is read on the host, so the call is asynchronous on the ctx
 *   stream like wct_stylize_prepared_batch_dev (it blocks only while it computes a style state it does not hold).  Frame f is
 *   wct_stylize_prepared_strength(content f, map f), bit for bit.  ..._warm: the same with a warm state, as
 *   wct_stylize_prepared_batch_dev_warm (the levels of the call must be the state's set; no WCT_FLAG_ADAIN).
 * flags: WCT_FLAG_MODE_NP, WCT_FLAG_ADAIN, WCT_FLAG_IMAGES_F32 for the content, WCT_FLAG_CONTENT_COLORS (on the frame: it does not
 *   meet the map).  WCT_STATUS_ARG, with a message: WCT_FLAG_SWAP5, WCT_FLAG_STYLE_SHARED, a NULL map, B outside 1 .. 32, a level
 *   outside the handle's set, and a content past the limit of one launch (the banded call takes no map).  A handle that is not
 *   live in this ctx is WCT_STATUS_STATE and never dereferenced.  A refusal leaves the ctx usable.
 * Mixes, label maps, style-swap, tiles and textures take no strength map. */
int  wct_transform_strength(wct_ctx* ctx, const float* content, int Nc, int h, int w, const uint8_t* smap, int Hm, int Wm,
                            int stride, const float* style, int Ns, int C, float alpha, int mode, float eps, float* out,
                            int* sweeps_out /* [2] or NULL */);
int  wct_adain_strength(wct_ctx* ctx, const float* content, int Nc, int h, int w, const uint8_t* smap, int Hm, int Wm, int stride,
                        const float* style, int Ns, int C, float alpha, float epsilon, float* out);
int  wct_stylize_prepared_strength(wct_ctx* ctx, const uint8_t* content, int Hc, int Wc, const uint8_t* smap, const wct_style* style,
                                   const int* levels, int n_levels, float alpha, unsigned flags, uint8_t* out);
int  wct_stylize_prepared_strength_batch_dev(wct_ctx* ctx, const uint8_t* content_dev, int Hc, int Wc, int B,
                                             const uint8_t* smaps_dev /* [B][Hc][Wc] */, const wct_style* style, const int* levels,
                                             int n_levels, float alpha, unsigned flags, uint8_t* out_dev);
int  wct_stylize_prepared_strength_batch_dev_warm(wct_ctx* ctx, const uint8_t* content_dev, int Hc, int Wc, int B,
                                                  const uint8_t* smaps_dev, const wct_style* style, const int* levels, int n_levels,
                                                  float alpha, unsigned flags, wct_warm* warm, uint8_t* out_dev);

/* ---- texture synthesis: seeded noise on the device, the passes chained there ------------------
 * Li et al. 2017, sec. 4.3: a noise image goes through the multi-level pipeline a few times and comes out as a sample of the
 * style's texture; other noise images give other samples, a style mix gives interpolated textures.  The reference ships it as
 * webcam.py --noise (webcam.py:191-192: the frame is replaced by np.random.randint(0, 256, shape, np.uint8)) and as the
 * commented-out recipe of stylize.py:95-97 (the same noise under gaussian_filter(sigma=0.5)).  Here the noise is a RULE, integers
 * only, so that the device, a host program and NumPy agree bit for bit (all arithmetic mod 2^32):
 *   fmix(h):  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16      (murmur3's finaliser)
 *   key = fmix(seed ^ (sample * 0x9E3779B9))          sample: the index of the image -- one independent image per sample
 *   n   = (y * W + x) * 3 + ch                        the byte's index in its [H][W][3] image
 *   raw = fmix(fmix(n ^ key) + key) >> 24             one uniform byte
 * smooth = 0 (webcam.py:192) gives raw.  smooth != 0 is the recipe of stylize.py:95-97 restated in integers, over the two spatial
 * axes only (the reference's call would also blur across R, G and B, an accident of handing it an [H][W][3] array): the 3-tap
 * weights w = 27 202 27 (sigma = 0.5 to 8 bits; they sum to 256, the taps at +-2 round to 0) along y and along x,
 *   out = (sum_dy sum_dx w[dy] w[dx] raw(sym(y + dy, H), sym(x + dx, W), ch) + 32768) >> 16,   sym(-1, n) = 0, sym(n, n) = n - 1
 * (scipy's mode='reflect', NumPy's 'symmetric' -- not the tf.pad REFLECT of the convolutions).
 * wct_texture_noise_batch_dev (webcam.py:191-192, stylize.py:95-97, Li et al. sec. 4.3): out_dev [B][H][W][3] uint8 on the device,
 *   at any byte address; image b is sample first_sample + b; B = 1 .. 32; one launch, asynchronous on the ctx stream.
 * wct_texture_noise (the same lines): one image into host memory, blocking.
 * A null pointer, B outside 1 .. 32, H or W < 1, or B * H * W * 3 >= 2^31 bytes in one call (the kernel's indices are 32-bit: such
 *   a call is refused, not wrapped) is WCT_STATUS_ARG and leaves the ctx usable. */
int wct_texture_noise_batch_dev(wct_ctx* ctx, int H, int W, int B, unsigned seed, unsigned first_sample, int smooth,
                                uint8_t* out_dev);
int wct_texture_noise(wct_ctx* ctx, int H, int W, unsigned seed, unsigned sample, int smooth, uint8_t* out_host);
/* wct_texture_size (webcam.py:191-192, stylize.py:95-97, Li et al. sec. 4.3): the frame size of a texture from H x W noise --
 *   wct_output_size applied `passes` times (passes = 1 .. 16).  The first pass can grow the frame; later passes keep its size.
 * wct_texture_prepared_batch_dev (the same lines; replaces the host loop "noise, then --passes predictions" of those recipes):
 *   the noise of samples first_sample .. first_sample + B - 1 (B = 1 .. 32) is made in ctx scratch, then `passes` (1 .. 16) runs
 *   of wct_stylize_prepared_batch_dev's body follow, each on the frames of the one before it; the frames between two passes live
 *   in two ctx-owned uint8 buffers that alternate, and nothing goes to the host.  out_dev [B][Ho][Wo][3] (wct_texture_size)
 *   holds the last pass.  Sample f equals `passes` chained wct_stylize_prepared_batch_dev calls on wct_texture_noise(.., sample
 *   f), bit for bit, whatever B and first_sample it came with.  Asynchronous on the ctx stream: the style states of every
 *   geometry the passes meet (at most two: the noise size and the size after pass 1) are asked for before the first launch, so
 *   the call blocks only there, as the prepared calls do; WCT_STATUS_NOCONV surfaces as on wct_stylize_prepared_batch_dev.
 * wct_texture_prepared (the same lines): the B = 1 case, the frame into host memory, blocking like wct_stylize_prepared.
 * flags: WCT_FLAG_MODE_NP and WCT_FLAG_ADAIN.  WCT_STATUS_ARG: WCT_FLAG_SWAP5, WCT_FLAG_STYLE_SHARED, WCT_FLAG_IMAGES_F32,
 *   WCT_FLAG_CONTENT_COLORS (there is no content whose colours could be kept), B outside 1 .. 32, passes outside 1 .. 16, H or W
 *   below the minimum of the deepest level, a level outside the handle's set, a null pointer.  A handle that is not live in this
 *   ctx is WCT_STATUS_STATE and never dereferenced.  A refusal leaves the ctx usable. */
int wct_texture_size(int H, int W, const int* levels, int n_levels, int passes, int* Ho, int* Wo);
int wct_texture_prepared_batch_dev(wct_ctx* ctx, int H, int W, int B, unsigned seed, unsigned first_sample, int smooth,
                                   const wct_style* style, const int* levels, int n_levels, int passes, float alpha,
                                   unsigned flags, uint8_t* out_dev);
int wct_texture_prepared(wct_ctx* ctx, int H, int W, unsigned seed, unsigned sample, int smooth,
                         const wct_style* style, const int* levels, int n_levels, int passes, float alpha,
                         unsigned flags, uint8_t* out_host);

/* ---- banded stylization: contents past the limits of one launch ---------------------------
 * predict() runs every layer over the whole image (wct.py:70-106, model.py:77-101), and so do the calls above: each layer is one
 * launch, and the kernels address one image's activations with 32-bit byte offsets.  A content whose largest map passes 2^31
 * bytes is WCT_STATUS_ARG there: H W >= 2^31 / 256 = 8 388 608 pixels with relu1_1 among the levels (its fp32 tap), 16.7 MP
 * without (the 64-channel fp16 maps).  The calls below run such a content in pieces on the same kernels, exactly:
 *   bands:  band k owns the image rows [k band_rows, (k + 1) band_rows) of a level's input (band_rows a multiple of 16).  The
 *     encoder runs on the band and a halo of real rows (16, 16, 16, 48, 96 image rows for relu1_1 .. relu5_1: what the layer
 *     list needs, rounded up to 16), the decoder on the band's feature rows and 2, 2, 3, 4, 5 feature rows on either side (its
 *     first row moved down to an even one); an edge that is the image's gets the image's own reflect pad.  The interiors are
 *     copied into the full map, so every value has the operands, in the order, of the whole pass: the same bits.
 *   chunks: the transform's content side needs a mean and a covariance, which pool exactly over chunks of whole feature rows:
 *     N = sum n_k, m = sum n_k m_k / N, Cov = [sum (n_k - 1) S_k + sum n_k (m_k - m)(m_k - m)^T] / (N - 1), in double, in chunk
 *     order, rounded to fp32 once, wct_tf's diagonal eps added after it (csrc/pool_rule.h).  The eigensolve, the colouring and
 *     the blend run once on the pooled statistics; the apply runs per chunk with the fp16 scale that covers every chunk.
 *     stat_rows = 0: the fewest equal chunks that fit -- ONE when the map fits, and one chunk is the whole-image transform
 *     itself, bit for bit; stat_rows > 0: that many feature rows per chunk.  The chunks depend on the map and stat_rows alone,
 *     never on band_rows, so frames do not depend on band_rows.  At most 4096 chunks per map.
 * wct_band_rows (reference: none; wct.py:70-106 has no size limit of its own): *band_rows = 0 when the whole-image calls take
 *   this content with these levels, else the automatic band height -- the largest multiple of 16 up to 2048 at which every band
 *   of every level fits.  Too wide for a band of 16 rows: WCT_STATUS_ARG, the width limit in the message.  Pure host code.
 * wct_band_plan (the same lines): the bands of ONE level on an H x W input, band k in rows[6 k ..]: the encoder span [0], [1]
 *   and the interior [2], [3] in image rows, the decoder span [4], [5] in feature rows; the band's interior feature rows are
 *   [rows[2] / s, rows[3] / s), s = 2^(level - 1), the last band's running to the map's end.  band_rows = 0: the automatic
 *   height (one band when the whole-image call runs).  *n_bands is always set; more than max_bands is WCT_STATUS_ARG unless
 *   max_bands = 0 (a query of the count).  Pure host code.
 * wct_encode_banded / wct_decode_banded (model.py:135-139 / model.py:245-304): the banded twins of wct_encode / wct_decode --
 *   host pointers, blocking; equal to the twin bit for bit wherever it runs, and running beyond its limit.  band_rows = 0:
 *   automatic.  Like wct_mask_compact they are checks of the stylize call's stages, not calls to build on.
 * wct_transform_chunked (ops.py:24-140): wct_transform with the content statistics pooled over chunks of chunk_rows rows (a
 *   single left-over row joins the chunk before it; chunk_rows = 1 is WCT_STATUS_ARG).  chunk_rows = 0 or >= Nc: one chunk,
 *   wct_transform's output bit for bit.  Groups of 32 chunks share the launches' workspace; any number up to 4096 works.
 * wct_stylize_prepared_banded_dev (wct.py:70-106): one content [Hc][Wc][3] on the device on a prepared style, the frame
 *   [Ho][Wo][3] (wct_output_size) on the device; asynchronous the way wct_stylize_prepared_batch_dev is (a call that computes a
 *   new state or grows a buffer blocks while it does), WCT_STATUS_NOCONV surfacing as there.  band_rows = 0: automatic (one band
 *   per level when the whole-image call runs).  With stat_rows = 0 and maps that fit, the frame is wct_stylize_prepared's bit
 *   for bit.  wct_stylize_prepared_banded: host pointers, blocking, like wct_stylize_prepared.
 *   The style state is the handle's under the key of the WHOLE map -- the layout of (h w content rows, the style's rows), the
 *   key the whole-image call uses --, whatever the chunks.
 *   flags: WCT_FLAG_MODE_NP, WCT_FLAG_IMAGES_F32, WCT_FLAG_CONTENT_COLORS (its launch indexes with size_t: any frame size).
 *   WCT_STATUS_ARG: WCT_FLAG_ADAIN, WCT_FLAG_SWAP5, WCT_FLAG_STYLE_SHARED, a band_rows that is not a multiple of 16 or whose
 *   bands pass the launch limit, a stat_rows whose chunks do, a level outside the handle's set.  A handle that is not live is
 *   WCT_STATUS_STATE, a failed allocation WCT_STATUS_NOMEM.  A refusal leaves the ctx usable.
 * Out of scope: AdaIN, style-swap, style mixes, masks, warm states and batches on large contents; and large STYLE images --
 *   wct_style_prepare keeps its limit (the same pooling would serve it). */
int wct_band_rows(int Hc, int Wc, const int* levels, int n_levels, int* band_rows);
int wct_band_plan(int H, int W, int level, int band_rows, int max_bands, int* n_bands, int* rows /* [max_bands][6] */);
int wct_encode_banded(wct_ctx* ctx, const float* img01, int H, int W, int level, int band_rows, float* feat);
int wct_decode_banded(wct_ctx* ctx, const float* feat, int h, int w, int level, int band_rows, float* img);
int wct_transform_chunked(wct_ctx* ctx, const float* content, int Nc, const float* style, int Ns, int C, float alpha, int mode,
                          float eps, int chunk_rows, float* out, int* sweeps_out);
int wct_stylize_prepared_banded_dev(wct_ctx* ctx, const uint8_t* content_dev, int Hc, int Wc, const wct_style* style,
                                    const int* levels, int n_levels, float alpha, unsigned flags, int band_rows, int stat_rows,
                                    uint8_t* out_dev);
int wct_stylize_prepared_banded(wct_ctx* ctx, const uint8_t* content, int Hc, int Wc, const wct_style* style, const int* levels,
                                int n_levels, float alpha, unsigned flags, int band_rows, int stat_rows, uint8_t* out);

/* ---- seamless textures: periodic synthesis on wrap-around halos ---------------------------
 * Every conv of the encoder and the decoders reflect-pads its input (model.py:135-139, 245-304), so the left edge of a frame
 * knows nothing of its right edge and a synthesized texture cannot be repeated without a seam.  The calls below run the same
 * network on a torus, on the unchanged kernels: before each encoder and each decoder of the chain the map is extended, on the
 * device, by a halo of its own pixels taken modulo its size; the kernels run on the extended map; the interior is kept; the
 * transform runs on the interior alone (its statistics are those of one period).  A halo as wide as a level's receptive field
 * makes the interior exactly the periodic network's output (the argument of the banded calls, with another halo source):
 *   encoder of relu1_1 .. relu5_1: 16, 16, 16, 48, 96 image pixels on all four sides;
 *   decoder: 2, 2, 4, 4, 6 feature pixels on top and left (even, so that the interior starts on an upsampled pair and a Winograd
 *     row pair), 2, 2, 3, 4, 5 on bottom and right.
 * Size rule: H and W multiples of 2^(l_max - 1), l_max the deepest level of the chain (ceil-mode pooling of an odd size is not
 *   periodic) -- else WCT_STATUS_ARG, the multiple in the message; the minimum size of any content applies; frames have the
 *   size of the tile.  A tile whose padded maps pass the limit of one launch (2^31 bytes) is WCT_STATUS_ARG.
 * wct_wrap_halo (reference: none): the halo of a level -- *enc, *dec_before, *dec_after.  wct_wrap_check: the size rule and the
 *   launch limits of an H x W tile for these levels.  Both pure host code.
 * wct_wrap_pad_batch_dev (reference: none; np.pad(mode='wrap')): in_dev [B][H][W][C] fp32 -> out_dev
 *   [B][top + H + bottom][left + W + right][C], out(y, x) = in((y - top) mod H, (x - left) mod W), the modulo non-negative (a halo
 *   may be several periods wide).  C a multiple of 4 moves 16-byte groups (both pointers 16-byte aligned), any other C floats.
 *   B = 1 .. 32; one launch, asynchronous.  wct_wrap_pad: B = 1, host pointers, blocking.  Checks of the kernel, like
 *   wct_mask_compact; a padded map of 2^31 bytes is WCT_STATUS_ARG.
 * wct_encode_wrap / wct_decode_wrap (model.py:135-139 / 245-304 on a torus): wct_encode / wct_decode of the periodically extended
 *   map, the interior returned -- bit for bit what wct_encode / wct_decode give on the map padded by the halo on the host.  Host
 *   pointers, blocking.  img01 [H][W][3] -> feat [H / s][W / s][C]; feat [h][w][C] -> img [h s][w s][3], s = 2^(level - 1).
 * wct_stylize_prepared_wrap_batch_dev (wct.py:70-106 on a torus): B = 1 .. 32 tiles [B][Hc][Wc][3] on the device on a prepared
 *   style, frames [B][Hc][Wc][3]; per level: pad, encode, crop the tap, transform under the state key of the unpadded map (no
 *   fused epilogue statistics), pad, decode, crop.  A periodic content gives a periodic frame; frame f does not depend on B.
 *   Asynchronous the way wct_stylize_prepared_batch_dev is (states and buffers first).  wct_stylize_prepared_wrap: B = 1, host
 *   pointers, blocking.  flags: WCT_FLAG_MODE_NP, WCT_FLAG_ADAIN, WCT_FLAG_IMAGES_F32.
 * wct_texture_prepared_wrap_batch_dev / wct_texture_prepared_wrap (Li et al. sec. 4.3): wct_texture_prepared_batch_dev /
 *   wct_texture_prepared with the wrap chain in the place of the plain one: the same noise, `passes` wrap runs chained in device
 *   memory, tiles [B][H][W][3].  Sample f equals `passes` chained wct_stylize_prepared_wrap_batch_dev calls on
 *   wct_texture_noise(.., sample f) bit for bit.  flags: WCT_FLAG_MODE_NP, WCT_FLAG_ADAIN.
 * WCT_STATUS_ARG, each with a message: WCT_FLAG_CONTENT_COLORS, WCT_FLAG_SWAP5, WCT_FLAG_STYLE_SHARED, a size that breaks the
 *   size rule or the launch limit, a level outside the handle's set, B outside 1 .. 32, a null pointer.  A handle that is not
 *   live is WCT_STATUS_STATE.  A refusal leaves the ctx usable.
 * Out of scope: tileable mixes, masks, warm states, style-swap and content colours; wrap combined with bands (tiles past the
 *   launch limit); sizes that are not multiples of the deepest stride. */
int wct_wrap_halo(int level, int* enc, int* dec_before, int* dec_after);
int wct_wrap_check(int H, int W, const int* levels, int n_levels);
int wct_wrap_pad_batch_dev(wct_ctx* ctx, const float* in_dev, int B, int H, int W, int C, int top, int bottom, int left, int right,
                           float* out_dev);
int wct_wrap_pad(wct_ctx* ctx, const float* x, int H, int W, int C, int top, int bottom, int left, int right, float* y);
int wct_encode_wrap(wct_ctx* ctx, const float* img01, int H, int W, int level, float* feat);
int wct_decode_wrap(wct_ctx* ctx, const float* feat, int h, int w, int level, float* img);
int wct_stylize_prepared_wrap_batch_dev(wct_ctx* ctx, const uint8_t* content_dev, int Hc, int Wc, int B, const wct_style* style,
                                        const int* levels, int n_levels, float alpha, unsigned flags, uint8_t* out_dev);
int wct_stylize_prepared_wrap(wct_ctx* ctx, const uint8_t* content, int Hc, int Wc, const wct_style* style, const int* levels,
                              int n_levels, float alpha, unsigned flags, uint8_t* out);
int wct_texture_prepared_wrap_batch_dev(wct_ctx* ctx, int H, int W, int B, unsigned seed, unsigned first_sample, int smooth,
                                        const wct_style* style, const int* levels, int n_levels, int passes, float alpha,
                                        unsigned flags, uint8_t* out_dev);
int wct_texture_prepared_wrap(wct_ctx* ctx, int H, int W, unsigned seed, unsigned sample, int smooth,
                              const wct_style* style, const int* levels, int n_levels, int passes, float alpha,
                              unsigned flags, uint8_t* out_host);

/* ---- decoder training (model.py:123-223, train.py:129-196) ---------------------------
 * One optimiser step of the decoder for relu<level>_1 (the encoder is frozen, model.py:202):
 *   F = enc(x); D = dec(F); F' = enc(D);
 *   loss = feature_weight * mse(F', F) + pixel_weight * mse(D, x) + tv_weight * mean_b(total_variation(D))
 *   Adam(lr, beta1, beta2, eps) on the decoder's kernels and biases (tf.train.AdamOptimizer, model.py:199).
 * images: host fp32 [B][H][W][3] in [0,1] (train.py:72-83), H and W multiples of 2^(level-1).
 * step: 1-based step number (Adam bias correction); lr: the already decayed rate (torch_decay, model.py:17-19);
 * lr == 0 computes losses and gradients without touching the weights.  losses_out[4] = feature, pixel, tv, total.
 * Forward in the inference precision (fp16 activations, fp32 accumulate), backward and optimiser in fp32. */
int wct_train_step(wct_ctx* ctx, int level, const float* images, int B, int H, int W,
                   float feature_weight, float pixel_weight, float tv_weight,
                   float lr, float beta1, float beta2, float eps, int step, float* losses_out);
/* conv `layer` (0-based, the 3-channel output conv last) of the decoder for relu<level>_1: its current fp32
 * weights [3][3][Cin][Cout] / bias, and the gradients of the last wct_train_step.  Any pointer may be NULL.
 * This is what a checkpoint writer (tf.train.Saver.save, train.py:183-185) reads. */
int wct_get_decoder_layer(wct_ctx* ctx, int level, int layer, float* w_hwio, float* bias,
                          float* grad_w, float* grad_b);

/* Data-parallel training (one process per GPU): every rank runs wct_train_step(lr = 0) on its own shard of the
 * batch, the ranks average the gradient buffer below with ONE all-reduce (RCCL), then every rank applies the same
 * Adam step.  *grad_dev: one contiguous device buffer of *count floats with the gradients of all layers (the
 * layout is private and identical on every rank).  train_step(lr=0) + train_apply(lr) == train_step(lr), bit for bit. */
int wct_train_grad_buffer(wct_ctx* ctx, int level, float** grad_dev, size_t* count);
int wct_train_apply(wct_ctx* ctx, int level, float lr, float beta1, float beta2, float eps, int step);

/* ---- device memory helpers (thin wrappers so callers need no HIP binding) ----------- */
int wct_dev_alloc(wct_ctx* ctx, size_t bytes, void** out);
int wct_dev_free(wct_ctx* ctx, void* p);
int wct_h2d(wct_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int wct_d2h(wct_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);

/* ---- measurement: per-kernel-class HIP-event timing on the ctx stream ----------------
 * class ids: 0 conv3x3 (MFMA), 1 conv_first, 2 conv_last, 3 pool, 4 wct stats+cov,
 * 5 jacobi eigensolver, 6 wct tbuild+apply, 7 other, 8 conv12 (conv1_1 + conv1_2 + pool in one
 * launch: the content passes of the levels >= 2), 9 conv_wino (the 3x3 launches the reduced-FLOP kernel takes -- csrc/conv_wino.hip,
 * the >= 256-channel layers without a feature tap; flops are the DIRECT convolution's, the kernel executes 2/3 of them), 10
 * unused (was the fused decoder tail, removed).  When enabled every launch group is bracketed by hipEventRecord on the ctx stream;
 * wct_prof_read syncs and accumulates. */
#define WCT_PROF_CLASSES 11
int wct_prof_enable(wct_ctx* ctx, int on);
int wct_prof_reset(wct_ctx* ctx);
int wct_prof_read(wct_ctx* ctx, double ms[WCT_PROF_CLASSES], long long launches[WCT_PROF_CLASSES],
                  double flops[WCT_PROF_CLASSES], double bytes[WCT_PROF_CLASSES]);
/* Eigensolver statistics since the last call (the decompositions that replace tf.svd / np.linalg.svd, ops.py:53-55,
 * 110,123), per size class k = 0..5 (covariances of order 32 * 2^k): out[3k] = matrices solved, out[3k+1] = sum of
 * the sweeps they took, out[3k+2] = the largest sweep count.  Synchronises the ctx stream; cleared on read. */
int wct_eig_stats(wct_ctx* ctx, long long out[18]);

#ifdef __cplusplus
}
#endif
#endif /* WCT_HIP_H */
