"""WCT: the inference facade of wct.py:14-106 on the MI355X path.

    WCT(checkpoints, relu_targets, vgg_path, device='/gpu:0', ss_patch_size=3, ss_stride=1)
    WCT.predict(content, style, alpha=1, swap5=False, ss_alpha=1, adain=False) -> uint8 HxWx3
    WCT.predict_mix(content, styles, weights=None, alpha=1, adain=False, swap5=False, ss_alpha=1) -> uint8 HxWx3
    WCT.predict_masked(content, styles, mask, alpha=1, adain=False, swap5=False, ss_alpha=1) -> uint8 HxWx3
    WCT.prepare_style(style) -> PreparedStyle, which predict / predict_frames / predict_mix take in the place of a style image
    WCT.prepare_style(style, region=(label_map, label)) / prepare_style_regions(style, label_map, k): a style from a labelled part
    of its image; predict_masked(..., style_masks=[...]) matches content region k with label k of style k
    every predict* takes content_colors=True: the frame keeps its luminance and takes the colours of its content
    WCT.synthesize(style, size, seeds=1, seed=0, passes=3) -> uint8 [n][Ho][Wo][3], textures of the style from seeded noise
    predict_frames(wrap=True) / synthesize(tile=True): the network on a torus -- tileable frames, seamless textures

`checkpoints` / `vgg_path`: the reference restores TF checkpoints and a .t7 file
(wct.py:46-58, vgg_normalised.py:16).  Per decoder this class takes either of
  * a TF checkpoint directory (a `checkpoint` state file + V2 bundle, read by
    wct_tf_amd/tf_ckpt.py without TensorFlow) -- the reference's own format,
  * a .npz written by `wct_tf_amd.weights.save_weights` (file, or `decoder_<relu>.npz` in a directory),
or a weights dict via `weights=`; `vgg_path` is the reference's `.t7` or a .npz.  A missing
decoder raises like the reference does (wct.py:58).
"""
import os
import re

import numpy as np

from .context import Context, PreparedStyle, check_prepared, check_resize, check_texture, check_warm, check_wrap, region_rows, split_styles
from .model import WCTModel
from .weights import load_weights


def _device_index(device):
    if isinstance(device, int):
        return device
    m = re.search(r'(\d+)\s*$', str(device))        # '/gpu:0' -> 0
    return int(m.group(1)) if m else 0


def texture_plan(style, size, seeds=1, seed=0, passes=3, batch=16, weights=None, swap5=False):
    """The arguments of WCT.synthesize, checked without a GPU (ValueError): -> (h, w, samples, runs, batch).  `samples` are the
    sample indices in the order asked for; `runs` cuts them into (first_sample, count) pieces of consecutive indices, at most
    `batch` (clamped to 1 .. 32) each -- one device call per piece."""
    if swap5:
        raise ValueError('a texture takes no swap5: style-swap matches patches of a content, and noise has none worth matching')
    mix = isinstance(style, (list, tuple))
    if weights is not None and not mix:
        raise ValueError('weights go with a list of styles (texture interpolation), got one style')
    if mix:
        from ._lib import mix_weights
        mix_weights(weights, len(style))
    batch = max(1, min(32, int(batch)))
    if isinstance(seeds, (int, np.integer)):
        if seeds < 1:
            raise ValueError('seeds is a count >= 1 or a list of sample indices, got %d' % seeds)
        samples = list(range(int(seeds)))
    else:
        samples = [int(v) for v in seeds]
        if not samples:
            raise ValueError('an empty list of sample indices')
    h, w = check_texture(size, passes, 1, seed, min(samples))
    check_texture(size, passes, 1, seed, max(samples))
    runs = []
    for v in samples:
        if runs and runs[-1][0] + runs[-1][1] == v and runs[-1][1] < batch:
            runs[-1][1] += 1
        else:
            runs.append([v, 1])
    return h, w, samples, [tuple(r) for r in runs], batch


class WCT(object):
    '''Stylize images with the WCT model on one MI355X'''

    def __init__(self, checkpoints, relu_targets, vgg_path, device='/gpu:0',
                 ss_patch_size=3, ss_stride=1, weights=None, wct_mode='tf'):
        self.ss_patch_size = ss_patch_size
        self.ss_stride = ss_stride
        self.relu_targets = list(relu_targets)
        self.wct_mode = wct_mode
        self.model = WCTModel(mode='test', relu_targets=relu_targets, vgg_path=vgg_path,
                              ss_patch_size=ss_patch_size, ss_stride=ss_stride)
        self.content_input = self.model.content_input
        self.decoded_output = self.model.decoded_output
        self.sess = Context(_device_index(device))

        if weights is None:
            weights = {'encoder': None, 'decoder': {}}
            if vgg_path is not None:
                if not os.path.exists(vgg_path):
                    raise Exception('No VGG weights found at {}'.format(vgg_path))
                if vgg_path.endswith('.t7'):                 # the reference's own format (vgg_normalised.py:16)
                    from .t7 import vgg_weights_from_t7
                    weights['encoder'] = vgg_weights_from_t7(vgg_path)
                else:
                    weights['encoder'] = load_weights(vgg_path)['encoder']
            for relu_target, checkpoint_dir in zip(relu_targets, checkpoints or []):
                path = checkpoint_dir
                if os.path.isdir(path) and os.path.exists(os.path.join(path, 'checkpoint')):
                    from .tf_ckpt import decoder_weights_from_checkpoint     # tf.train.Saver layout (wct.py:46-58)
                    weights['decoder'][relu_target] = decoder_weights_from_checkpoint(path, relu_target)
                    continue
                if os.path.isdir(path):
                    path = os.path.join(path, 'decoder_{}.npz'.format(relu_target))
                if not os.path.exists(path):
                    raise Exception('No checkpoint found for target {} in dir {}'.format(relu_target, checkpoint_dir))
                dec = load_weights(path)['decoder']
                if relu_target not in dec:
                    raise Exception('No checkpoint found for target {} in dir {}'.format(relu_target, checkpoint_dir))
                weights['decoder'][relu_target] = dec[relu_target]
        if weights.get('encoder') is None:
            raise Exception('No VGG weights given')
        self.sess.set_encoder(weights['encoder'])
        for relu_target in relu_targets:
            if relu_target not in weights['decoder']:
                raise Exception('No checkpoint found for target {}'.format(relu_target))
            self.sess.set_decoder(relu_target, weights['decoder'][relu_target])

    @staticmethod
    def preprocess(image):
        if len(image.shape) == 3:
            image = np.expand_dims(image, 0)
        return image / 255.

    @staticmethod
    def postprocess(image):
        return np.uint8(np.clip(image, 0, 1) * 255)

    def _swap5_setup(self, content, mask, swap5, ss_alpha):
        '''With swap5: the style-swap settings, and the content (and the mask, if any) center-cropped so that the swap's
           filter fits when ss_stride > 1 (a crop, never a resize: H, W fit inside the content).  -> (content, mask)'''
        if swap5 is True and self.ss_stride != 1:
            from .utils import swap_filter_fit, center_crop_to, _centre_window
            should_refit, H, W = swap_filter_fit(content.shape[0], content.shape[1], self.ss_patch_size, self.ss_stride)
            if should_refit:
                content = center_crop_to(content, H, W)
                if mask is not None:
                    mask = np.ascontiguousarray(_centre_window(mask, H, W))
        if swap5:
            self.sess.set_style_swap(ss_alpha, self.ss_patch_size, self.ss_stride)
        return content, mask

    def prepare_style(self, style, adain=False, region=None):
        '''Run the style side of `style` (array in [0,255]) once, for this model's relu_targets, and keep it on the device: the
           PreparedStyle goes wherever predict, predict_frames, predict_mix, predict_masked and predict_frames_masked take a
           style image and gives the same frames bit for bit, without the style encoder pass, the style statistics and the style
           eigendecompositions of every call.  One handle serves every content size and alpha, AdaIN included (`adain` only
           picks what is computed up front; another content -- or region -- size is computed on first use and kept).  Not for
           swap5.  Close it, or the model's context, to release it.
           region=(label_map, label): a style region -- label_map [H][W] integers of the style's size; the statistics of every
           level come from the feature pixels of `label` alone (sky from the sky of a painting), the encoder still sees the
           whole image.  A region needs 2 feature pixels at every relu target.'''
        return self.sess.prepare_style(style, self.relu_targets, adain=adain, wct_mode=self.wct_mode, region=region)

    def prepare_style_regions(self, style, label_map, k, adain=False):
        '''The k regions of ONE style image (label_map [H][W], labels 0 .. k - 1) as prepared styles, from one encoder pass: a
           list of k entries, entry j what prepare_style(style, region=(label_map, j)) gives bit for bit, or None for a region
           too small to carry a style (fewer than 2 feature pixels at some relu target).'''
        return self.sess.prepare_style_regions(style, label_map, k, self.relu_targets, adain=adain, wct_mode=self.wct_mode)

    def _region_handles(self, styles, style_masks, swap5, adain):
        '''The handles of predict_masked / predict_frames_masked with style_masks: style j from label j of style_masks[j] (None:
           the whole image).  Everything is checked before anything is prepared (ValueError); entries that are the same image
           and the same map are prepared together (prepare_style_regions).  A region too small to carry a style is a ValueError
           naming it.  -> the K handles, owned by the caller'''
        from ._lib import style_region_map
        k = len(styles)
        if swap5:
            raise ValueError('swap5 is not served with style_masks: style-swap needs the patches of a style image, not a region\'s moments')
        if len(style_masks) != k:
            raise ValueError('%d style masks for %d styles (one map, or None, per style)' % (len(style_masks), k))
        if any(isinstance(s, PreparedStyle) for s in styles):
            raise ValueError('style_masks go with style images: a PreparedStyle already holds its region (prepare_style(region=...))')
        styles = [np.asarray(s) for s in styles]
        for j, (s, m) in enumerate(zip(styles, style_masks)):
            if s.ndim != 3 or s.shape[2] != 3:
                raise ValueError('expected an HxWx3 style image, got shape %s' % (s.shape,))
            if m is not None:
                m = style_region_map(m, s.shape[:2], label=j)
                for r in self.relu_targets:
                    if region_rows(m, j, r) < 2:
                        raise ValueError('style region %d has %d feature pixels at %s: a region needs at least 2 at every relu target'
                                         % (j, region_rows(m, j, r), r))
        handles = [None] * k
        try:
            for j in range(k):
                if handles[j] is not None:
                    continue
                if style_masks[j] is None:
                    handles[j] = self.prepare_style(styles[j], adain=adain)
                    continue
                same = [i for i in range(j, k) if style_masks[i] is style_masks[j] and styles[i] is styles[j]]
                if len(same) > 1 and np.asarray(style_masks[j]).max() < k:
                    made = self.prepare_style_regions(styles[j], style_masks[j], k, adain=adain)
                    for i, h in enumerate(made):
                        if i in same:
                            handles[i] = h
                        elif h is not None:
                            h.close()
                else:
                    handles[j] = self.prepare_style(styles[j], adain=adain, region=(style_masks[j], j))
            return handles
        except Exception:
            for h in handles:
                if h is not None:
                    h.close()
            raise

    def warm_state(self):
        '''A WarmState for this model's relu_targets: hand it to predict / predict_frames (with a PreparedStyle) as `warm=` and
           the content eigensolves of a call start from the bases the previous call left in it.  For the frames of ONE video, in
           order: the frames meet the tolerances of cold ones but are not bit-identical to them.'''
        return self.sess.warm_state(self.relu_targets)

    def _check_warm(self, warm, style, swap5, adain):
        if not isinstance(style, PreparedStyle):
            raise ValueError('a warm state goes with a PreparedStyle (prepare_style), not a style image')
        check_warm(self.sess, warm, self.relu_targets, adain, swap5)

    def _band_route(self, content, band_rows, swap5, adain, warm):
        '''The band height a predict() goes to the banded call with, or None for the whole-image call.  band_rows None: banded
           only when the whole-image call refuses this content (wct_band_rows), at the automatic height; an int forces banding
           (0: the automatic height).  ValueError before any GPU call for what large contents do not take.'''
        from .context import band_rows as auto_band_rows, check_band_rows
        shape = np.shape(content)
        if len(shape) != 3:
            return None                                      # (the whole-image call reports the shape)
        if band_rows is None:
            need = auto_band_rows(shape[0], shape[1], self.relu_targets)
            if need == 0:
                return None
            rows = need
        else:
            rows = check_band_rows(band_rows)
            need = 0
        for name, on in (('adain', adain), ('swap5', swap5), ('warm', warm is not None)):
            if on:
                if need:
                    raise ValueError('%s is not served on a %dx%d content: it passes the limit of one launch (a map of 2^31 bytes) '
                                     'and runs in bands (band_rows=%d), which take whiten-colour transforms on one style only'
                                     % (name, shape[0], shape[1], need))
                raise ValueError('%s is not served with band_rows: the banded call takes whiten-colour transforms on one style only'
                                 % name)
        return rows

    def _strength_refusals(self, shape, swap5, band_rows, wrap=False):
        """What a strength map does not go with, as a ValueError before any GPU call: swap5, wrap, bands -- asked for, or needed by
        a content of `shape` (H, W) past the limit of one launch."""
        from .context import band_rows as auto_band_rows
        for name, on in (('swap5', swap5), ('wrap', wrap), ('band_rows', band_rows is not None)):
            if on:
                raise ValueError('%s is not served with a strength map: it goes with one style, WCT or AdaIN, on the whole image' % name)
        if auto_band_rows(shape[0], shape[1], self.relu_targets):
            raise ValueError('a strength map is not served on a %dx%d content: it passes the limit of one launch and runs in bands, '
                             'which take no map' % (shape[0], shape[1]))

    @staticmethod
    def _check_guided(guided):
        '''guided=(radius, eps_q) or (radius, eps_q, 'grey' or 'color') of a predict* call, checked: None stays None'''
        from .context import check_guided
        return None if guided is None else check_guided(guided)

    def predict(self, content, style, alpha=1, swap5=False, ss_alpha=1, adain=False, warm=None, content_colors=False,
                band_rows=None, strength=None, guided=None, guided_upsample=None):
        '''Stylize a single content/style pair; arrays in [0,255], returns uint8 HxWx3.
           The /255 preprocess and the clip*255 postprocess run inside the library
           (fused at the ends of the kernel chain).  `style` may be a PreparedStyle (prepare_style); with one, `warm` may be a
           WarmState (warm_state).  content_colors (here and in every predict*): luminance-only colour preservation (Gatys et
           al. 2016; WCT_FLAG_CONTENT_COLORS) -- the frame keeps its stylized luminance and takes the colours of `content`, in
           the last launch of the call; it equals ops.content_colors_np(the plain frame, content) bit for bit.
           band_rows: None sends a content to the banded call (Context.stylize_prepared_banded) only when it passes the limit of
           the whole-image call -- 8.4 MP with relu1_1 among the targets, 16.7 MP without --, an int forces it (a multiple of 16
           image rows per band; 0: the automatic height).  A style image is then prepared, used and closed.  adain, swap5 and
           warm are not served there: ValueError.
           strength: a uint8 map [H][W] of the content's size (Context.stylize_prepared_strength) -- 255 the call's alpha, 0 "keep
           the content features", every level sampling it at its own stride; a style image is prepared for the call.  No swap5,
           warm or bands with it: ValueError.
           guided (here and in predict_frames, predict_mix, predict_masked, predict_frames_masked): (radius, eps_q) -- guided
           smoothing, the photo mode (He et al., "Guided Image Filtering"; WCT_FLAG_GUIDED): the frame is filtered over a
           (2 radius + 1)^2 box with the grey of `content` as guide, eps_q in grey levels squared (_lib.guided_eps_q(eps)); it
           equals ops.guided_filter_np(the plain frame, content, radius, eps_q) bit for bit, and with content_colors the colour op
           runs after it.  (radius, eps_q, 'color') guides with the three channels of `content` (guide='color' of the op), which
           also keeps an edge between two colours of equal luminance; (radius, eps_q, 'grey') is the two-element form.  Not
           served in bands, with wrap or for textures: ValueError.
           guided_upsample (here and in predict_frames): (short_side, radius, eps_q) -- stylize small, deliver at the content's size
           (He & Sun, "Fast Guided Filter"; Context.stylize_prepared_upsampled).  The uint8 content is resized on the device to
           utils.resize_shape(H, W, short_side) (a content whose short side is short_side or less is worked on as it is), stylized
           there, and upsampled against the full content: the frame has the content's size and equals ops.guided_upsample_np(
           predict(the resized content), the resized content, content, radius, eps_q) bit for bit, content_colors_np against the
           full content after it.  (short_side, radius, eps_q, 'color') upsamples under the colour guide (guide='color' of the op);
           (short_side, radius, eps_q, 'grey') is the three-element form.  A style image is prepared for the call.  No swap5, warm,
           bands, strength or guided with it: ValueError.'''
        guided = self._check_guided(guided)                                       # ValueError before any GPU call
        if guided_upsample is not None:
            return self._predict_upsampled(np.asarray(content)[None], style, guided_upsample, alpha, adain, content_colors, 1,
                                           dict(swap5=swap5, warm=warm is not None, band_rows=band_rows is not None and band_rows is not False,
                                                strength=strength is not None, guided=guided is not None))[0]
        if strength is not None:
            from ._lib import strength_map
            content = np.asarray(content)
            if content.ndim != 3 or content.shape[2] != 3:
                raise ValueError('expected an HxWx3 content, got shape %s' % (content.shape,))
            strength = strength_map(strength, content.shape[:2])                  # ValueError before any GPU call
            self._strength_refusals(content.shape, swap5, band_rows)
            if warm is not None:
                raise ValueError('warm is not served with predict(strength=...): predict_frames(strengths=...) takes a warm state')
            if isinstance(style, PreparedStyle):
                check_prepared(self.sess, [style], self.relu_targets)
                return self.sess.stylize_prepared_strength(content, style, strength, self.relu_targets, alpha=alpha, adain=adain,
                                                           wct_mode=self.wct_mode, content_colors=content_colors, guided=guided)
            with self.prepare_style(np.asarray(style), adain=adain) as handle:
                return self.sess.stylize_prepared_strength(content, handle, strength, self.relu_targets, alpha=alpha, adain=adain,
                                                           wct_mode=self.wct_mode, content_colors=content_colors, guided=guided)
        rows = self._band_route(content, band_rows, swap5, adain, warm)           # ValueError before any GPU call
        if rows is not None:
            if guided is not None:
                raise ValueError('guided is not served in bands: filter the frame with ops.guided_filter_np')
            if isinstance(style, PreparedStyle):
                check_prepared(self.sess, [style], self.relu_targets)
                return self.sess.stylize_prepared_banded(np.asarray(content), style, self.relu_targets, alpha=alpha,
                                                         wct_mode=self.wct_mode, band_rows=rows, content_colors=content_colors)
            with self.prepare_style(np.asarray(style)) as handle:
                return self.sess.stylize_prepared_banded(np.asarray(content), handle, self.relu_targets, alpha=alpha,
                                                         wct_mode=self.wct_mode, band_rows=rows, content_colors=content_colors)
        if warm is not None:
            self._check_warm(warm, style, swap5, adain)                           # ValueError before any GPU call
        if isinstance(style, PreparedStyle):
            check_prepared(self.sess, [style], self.relu_targets, swap5)          # ValueError before any GPU call
            return self.sess.stylize_prepared(np.asarray(content), style, self.relu_targets, alpha=alpha, adain=adain,
                                              wct_mode=self.wct_mode, warm=warm, content_colors=content_colors, guided=guided)
        content, _ = self._swap5_setup(np.asarray(content), None, swap5, ss_alpha)
        style = np.asarray(style)
        # uint8 arrays take the fused /255 on the device; float arrays are divided by 255 WITHOUT rounding, as the
        # reference's preprocess does (wct.py:60-64) -- Context.stylize hands them over as float32 images
        return self.sess.stylize(content, style, self.relu_targets, alpha=alpha, adain=adain,
                                 wct_mode=self.wct_mode, swap5=bool(swap5), content_colors=content_colors, guided=guided)

    def _predict_upsampled(self, frames, style, guided_upsample, alpha, adain, content_colors, batch, others):
        '''predict / predict_frames with guided_upsample=(short_side, radius, eps_q[, guide]): uint8 full frames [F][H][W][3] -> [F][H][W][3].
           others: the options that do not go with it, by name -> whether they were given (ValueError before any GPU call)'''
        from .context import check_guided_upsample, upsample_work_size
        g = check_guided_upsample(guided_upsample)
        side, r, e = g[:3]
        guide = g[3] if len(g) == 4 else 'grey'
        for name, on in others.items():
            if on:
                raise ValueError('%s is not served with guided_upsample: one prepared style, WCT or AdaIN, content_colors' % name)
        if frames.ndim != 4 or frames.shape[3] != 3 or frames.size == 0:
            raise ValueError('guided_upsample takes HxWx3 contents, got shape %s' % (frames.shape[1:] if frames.shape[0] == 1 else frames.shape,))
        if frames.dtype != np.uint8:
            raise ValueError('guided_upsample takes uint8 contents (the resize on the device does), got %s' % frames.dtype)
        work = upsample_work_size(frames.shape[1], frames.shape[2], side)
        if isinstance(style, PreparedStyle):
            check_prepared(self.sess, [style], self.relu_targets)
        own = None if isinstance(style, PreparedStyle) else self.prepare_style(np.asarray(style), adain=adain)
        try:
            batch = max(1, min(32, int(batch)))
            return np.concatenate([self.sess.stylize_prepared_upsampled_batch(
                frames[i:i + batch], own or style, self.relu_targets, work, r, e, alpha=alpha, adain=adain, wct_mode=self.wct_mode,
                content_colors=content_colors, guide=guide) for i in range(0, len(frames), batch)], axis=0)
        finally:
            if own is not None:
                own.close()

    @staticmethod
    def _check_upsample_time(guided_upsample, frames_t, motion, others, shape):
        """guided_upsample_frames / guided_upsample_motion of predict_frames, checked before any GPU call
        -> (side, r, e, T, None | ('global', R) | int32 positions [N][2])"""
        from .context import check_guided_motion, check_guided_time, check_guided_upsample, check_motion_search, upsample_work_size
        g = check_guided_upsample(guided_upsample)
        side, r, e = g[:3]
        if len(g) == 4 and g[3] != 'grey':
            raise ValueError("guided_upsample_frames goes with the grey guide: the 'color' guide has no form along time")
        r, e, t = check_guided_time(r, e, frames_t)
        for name, on in others.items():
            if on:
                raise ValueError('%s is not served with guided_upsample: one prepared style, WCT or AdaIN, content_colors%s'
                                 % (name, ' (along time: guided_upsample_frames / guided_upsample_motion)' if name.startswith('guided_') else ''))
        if len(shape) != 4 or shape[3] != 3 or 0 in shape:
            raise ValueError('guided_upsample takes [F][H][W][3] contents, got shape %s' % (shape,))
        if motion is None:
            return side, r, e, t, None
        if isinstance(motion, str) or (isinstance(motion, tuple) and len(motion) == 2 and isinstance(motion[0], str)):
            name, search = (motion, 8) if isinstance(motion, str) else motion
            if name != 'global':
                raise ValueError("guided_upsample_motion is None, 'global', ('global', R) or an int array [N][2] of positions, got %r: "
                                 "per-block or dense motion, sub-pixel shifts, rotation and zoom are not served" % (motion,))
            hc, wc = upsample_work_size(shape[1], shape[2], side)
            return side, r, e, t, ('global', check_motion_search(search, hc, wc))
        return side, r, e, t, check_guided_motion(motion, shape[0])

    def _predict_upsampled_time(self, frames, style, guided_upsample, frames_t, motion, alpha, adain, content_colors, batch, others):
        '''predict_frames with guided_upsample and guided_upsample_frames >= 1: the frames resized to the working size on the device,
        stylized plain there, the positions estimated on the small contents when asked, all frames of the call delivered as one
        clip (Context.guided_upsample_time_clip), then the colour op against the full contents'''
        from .context import upsample_time_chunk, upsample_work_size
        side, r, e, t, motion = self._check_upsample_time(guided_upsample, frames_t, motion, others, np.shape(frames))
        if frames.dtype != np.uint8:
            raise ValueError('guided_upsample takes uint8 contents (the resize on the device does), got %s' % frames.dtype)
        work = upsample_work_size(frames.shape[1], frames.shape[2], side)
        if isinstance(style, PreparedStyle):
            check_prepared(self.sess, [style], self.relu_targets)
        step = min(32, upsample_time_chunk(frames.shape[1], frames.shape[2], 0))      # full frames of one upload
        small = np.concatenate([self.sess.resize_batch(frames[i:i + step], work) for i in range(0, len(frames), step)], axis=0)
        plain = self.predict_frames(small, style, alpha=alpha, adain=adain, batch=batch)
        positions = self.sess.motion_global(small, motion[1]) if isinstance(motion, tuple) else motion
        out = self.sess.guided_upsample_time_clip(plain, small, frames, r, e, t, positions=positions)
        if content_colors:
            out = np.concatenate([self.sess.content_colors_batch(out[i:i + step], frames[i:i + step]) for i in range(0, len(out), step)], axis=0)
        return out

    def predict_mix(self, content, styles, weights=None, alpha=1, adain=False, swap5=False, ss_alpha=1, content_colors=False,
                    guided=None):
        '''Stylize with a weighted mix of several styles (Li et al. 2017, sec. 4.2; the reference's README TODO
           "Interpolation between styles"): every level applies sum_k lambda_k T(content, style_k), lambda = weights /
           sum(weights); weights=None means equal weights.  Arrays in [0,255], returns uint8 HxWx3.  One style gives
           predict(content, style) bit for bit, as do one-hot weights.  swap5 takes one style only (style-swap is not linear).'''
        from ._lib import mix_weights
        guided = self._check_guided(guided)
        handles, styles = split_styles(list(styles))             # ValueError: images and prepared styles in one list
        if handles:
            weights = mix_weights(weights, len(handles))
            check_prepared(self.sess, handles, self.relu_targets, swap5)
            return self.sess.stylize_prepared_mix(np.asarray(content), handles, weights, self.relu_targets, alpha=alpha,
                                                  adain=adain, wct_mode=self.wct_mode, content_colors=content_colors, guided=guided)
        styles = [np.asarray(s) for s in styles]
        weights = mix_weights(weights, len(styles))              # ValueError before any GPU call
        if swap5 and len(styles) > 1:
            raise ValueError('swap5 takes one style: style-swap is not linear in the style')
        content, _ = self._swap5_setup(np.asarray(content), None, swap5, ss_alpha)
        return self.sess.stylize_mix(content, styles, weights, self.relu_targets, alpha=alpha, adain=adain,
                                     wct_mode=self.wct_mode, swap5=bool(swap5), content_colors=content_colors, guided=guided)

    def predict_masked(self, content, styles, mask, alpha=1, adain=False, swap5=False, ss_alpha=1, content_colors=False,
                       guided=None, style_masks=None):
        '''Stylize each region of a label map with its own style (Li et al. 2017, sec. 4.2, Fig. 7; the reference's README TODO
           "Spatial control/masking"): `mask` [H][W] holds a label 0 .. K-1 per content pixel, `styles` K images (sizes may
           differ), and at every level the pixels of label k are transformed with style k alone, with their own statistics
           (a label with fewer than 2 pixels at a level keeps that level's features).  Arrays in [0,255], returns uint8 HxWx3.
           One style with an all-zero mask gives predict(content, style) bit for bit.  swap5 takes one style only.
           `styles` may be K PreparedStyle objects (prepare_style) instead: the same frame, without the K style sides; the
           entries are all handles or all images (a mixed list is a ValueError), and swap5 takes images.
           style_masks: one label map [Hs][Ws] (of style k's size), or None, per style image -- style k is then taken from the
           pixels of ITS image labelled k (semantic matching: content region k from style region k), prepared here for the call
           (prepare_style(region=...)).  Not with swap5 or PreparedStyle entries: ValueError.'''
        from ._lib import mask_labels
        guided = self._check_guided(guided)
        if style_masks is not None:
            styles = list(styles)
            content = np.asarray(content)
            mask = mask_labels(mask, len(styles), content.shape[:2])            # ValueError before any GPU call
            own = self._region_handles(styles, list(style_masks), swap5, adain)
            try:
                return self.sess.stylize_prepared_masked(content, own, mask, self.relu_targets, alpha=alpha, adain=adain,
                                                         wct_mode=self.wct_mode, content_colors=content_colors, guided=guided)
            finally:
                for h in own:
                    h.close()
        handles, styles = split_styles(list(styles))             # ValueError: images and prepared styles in one list
        content = np.asarray(content)
        if handles:
            mask = mask_labels(mask, len(handles), content.shape[:2])
            check_prepared(self.sess, handles, self.relu_targets, swap5)
            return self.sess.stylize_prepared_masked(content, handles, mask, self.relu_targets, alpha=alpha, adain=adain,
                                                     wct_mode=self.wct_mode, content_colors=content_colors, guided=guided)
        styles = [np.asarray(s) for s in styles]
        mask = mask_labels(mask, len(styles), content.shape[:2])        # ValueError before any GPU call
        if swap5 and len(styles) > 1:
            raise ValueError('swap5 takes one style: style-swap is not a per-region affine map')
        content, mask = self._swap5_setup(content, mask, swap5, ss_alpha)
        return self.sess.stylize_masked(content, styles, mask, self.relu_targets, alpha=alpha, adain=adain,
                                        wct_mode=self.wct_mode, swap5=bool(swap5), content_colors=content_colors, guided=guided)

    def predict_frames_masked(self, frames, styles, masks, alpha=1, adain=False, batch=16, content_colors=False, resize=None,
                              guided=None, style_masks=None):
        '''Spatial control of a video: same-sized frames [F][H][W][3], a label map per frame `masks` [F][H][W] (or one [H][W] map
           used for every frame), `styles` K images -- prepared once here -- or K PreparedStyle objects.  Frame f equals
           predict_masked(frames[f], styles, masks[f]) bit for bit; the frames go through the device in batches of `batch`
           (<= 32), the regions of a batch sharing every launch and the eigensolves.  Returns uint8 [F][Ho][Wo][3].
           resize (h, w): as in predict_frames; the label maps are given at the resized size.
           style_masks: as in predict_masked -- one label map or None per style image, style k from label k of its map.'''
        from ._lib import mask_labels_frames
        guided = self._check_guided(guided)
        frames = np.asarray(frames)
        if frames.ndim != 4 or frames.shape[3] != 3:
            raise ValueError('expected [F][H][W][3] frames, got shape %s' % (frames.shape,))
        if resize is not None:
            resize = check_resize(resize)                        # ValueError before any GPU call
        handles, images = split_styles(list(styles))             # ValueError: images and prepared styles in one list
        k = len(handles) or len(images)
        masks = mask_labels_frames(masks, k, len(frames), resize or frames.shape[1:3])    # ValueError before any GPU call
        if handles:
            check_prepared(self.sess, handles, self.relu_targets)
        if frames.dtype != np.uint8:
            frames = np.uint8(np.clip(frames, 0, 255))
        if style_masks is not None:
            own = self._region_handles(list(styles), list(style_masks), False, adain)
        else:
            own = [] if handles else [self.prepare_style(np.asarray(s), adain=adain) for s in images]
        try:
            batch = max(1, min(32, int(batch)))
            return np.concatenate([self.sess.stylize_prepared_masked_batch(frames[i:i + batch], own or handles, masks[i:i + batch],
                                                                           self.relu_targets, alpha=alpha, adain=adain,
                                                                           wct_mode=self.wct_mode, content_colors=content_colors, guided=guided,
                                                                           resize=resize)
                                   for i in range(0, len(frames), batch)], axis=0)
        finally:
            for h in own:
                h.close()

    @staticmethod
    def _check_guided_frames(guided, guided_frames, swap5, wrap, guided_frames_guide=None):
        '''guided_frames and guided_frames_guide of predict_frames, checked before any GPU call -> whether the frames take the
        temporal route'''
        from .context import check_guide, check_guided_time
        if guided_frames_guide is not None:
            check_guide(guided_frames_guide)
        if guided is None:
            if guided_frames:
                raise ValueError('guided_frames needs guided=(radius, eps_q): it extends that filter along time')
            if guided_frames_guide is not None:
                raise ValueError('guided_frames_guide needs guided=(radius, eps_q) and guided_frames >= 1: it chooses the guide of that '
                                 'filter along time')
            return False
        t = check_guided_time(guided[0], guided[1], guided_frames)[2]
        if t == 0:
            if guided_frames_guide is not None:
                raise ValueError('guided_frames_guide needs guided_frames >= 1: it chooses the guide of that filter along time')
            return False
        if len(guided) == 3 and guided[2] != 'grey':
            raise ValueError("guided_frames goes with the grey guide of guided=: the 'color' guide of the per-frame filter has no form "
                             "along time (guided_frames_guide='color' chooses the guide of the filter along time)")
        for name, on in (('swap5', swap5), ('wrap', wrap)):
            if on:
                raise ValueError('guided_frames is not served with %s' % name)
        return True

    @staticmethod
    def _check_guided_motion(guided_motion, temporal, frames, resize):
        """guided_motion of predict_frames, checked before any GPU call -> None, ('global', R) or int32 positions [N][2]"""
        from .context import check_guided_motion, check_motion_search
        if guided_motion is None:
            return None
        if not temporal:
            raise ValueError('guided_motion needs guided_frames >= 1: it shifts the windows of that filter along time')
        shape = np.shape(frames)
        if len(shape) != 4 or shape[3] != 3:
            raise ValueError('expected [F][H][W][3] frames, got shape %s' % (shape,))
        if isinstance(guided_motion, str) or (isinstance(guided_motion, tuple) and len(guided_motion) == 2 and isinstance(guided_motion[0], str)):
            name, search = (guided_motion, 8) if isinstance(guided_motion, str) else guided_motion
            if name != 'global':
                raise ValueError("guided_motion is None, 'global', ('global', R) or an int array [N][2] of positions, got %r: per-block or "
                                 "dense motion, sub-pixel shifts, rotation and zoom are not served" % (guided_motion,))
            h, w = check_resize(resize) if resize is not None else shape[1:3]
            return ('global', check_motion_search(search, h, w))
        return check_guided_motion(guided_motion, shape[0])

    def _predict_frames_smoothed(self, frames, style, guided, frames_t, content_colors, resize, kw, motion=None, guide='grey'):
        '''predict_frames with guided_frames >= 1: the plain frames of the call, filtered along time as one clip against their
        contents (the resized ones with resize=), then the colour op.  motion: None, ('global', R) -- the positions are estimated
        from those contents (on the grey guide, whatever `guide` is) -- or positions [N][2]; guide: that of the filter along time'''
        if frames.ndim != 4 or frames.shape[3] != 3:
            raise ValueError('expected [F][H][W][3] frames, got shape %s' % (frames.shape,))
        if frames.dtype != np.uint8:
            frames = np.uint8(np.clip(frames, 0, 255))
        if resize is not None:
            resize = check_resize(resize)                                         # ValueError before any GPU call
        plain = self.predict_frames(frames, style, resize=resize, **kw)
        contents = frames if resize is None else np.concatenate(
            [self.sess.resize_batch(frames[i:i + 32], resize) for i in range(0, len(frames), 32)], axis=0)
        positions = self.sess.motion_global(contents, motion[1]) if isinstance(motion, tuple) else motion
        out = self.sess.guided_filter_time_clip(plain, contents, guided[0], guided[1], frames_t, positions=positions, guide=guide)
        if content_colors:
            out = np.concatenate([self.sess.content_colors_batch(out[i:i + 32], contents[i:i + 32]) for i in range(0, len(out), 32)], axis=0)
        return out

    def predict_frames(self, frames, style, alpha=1, swap5=False, ss_alpha=1, adain=False, batch=16, warm=None,
                       content_colors=False, resize=None, wrap=False, strengths=None, guided=None, guided_frames=0, guided_motion=None,
                       guided_upsample=None, guided_upsample_frames=0, guided_upsample_motion=None, guided_frames_guide=None):
        '''Stylize same-sized frames [F][H][W][3] with ONE style image (the loop of stylize_video.py:112-121,
           which calls predict() once per frame and so re-runs the style encoder, the style statistics and the
           style eigendecompositions every frame).  Here the style side runs once per batch of `batch` frames;
           every frame equals predict(frame, style) bit for bit.  Returns uint8 [F][Ho][Wo][3].
           With a PreparedStyle (prepare_style) the style side does not run at all; the frames are the same.
           With a PreparedStyle and `warm` (a WarmState) every batch starts its content eigensolves from the last frame of the
           batch before it (the state's, for the first): frames within tolerance of the cold ones, not bit-identical.
           resize (h, w): the frames are raw and are resized to h x w on the device, in front of the call and on its stream
           (Context.resize_batch_dev: Pillow's bilinear bytes) -- predict_frames on utils._imresize(frame, (h, w)), bit for bit.
           wrap: the network on a torus (Context.stylize_prepared_wrap_batch) -- every conv sees the frame continued periodically,
           so a tileable frame stays tileable.  Prepared styles only; H and W multiples of the deepest level's stride; no swap5,
           warm, content_colors or resize (ValueError before any GPU call).  Frames keep their size.
           strengths: a strength map per frame, uint8 [F][H][W] (or one [H][W] map for all frames), at the resized size with
           resize -- frame f equals predict(frames[f], style, strength=strengths[f]) bit for bit (cold).  A style image is prepared
           once here; warm then needs a PreparedStyle as always.  No swap5 or wrap with it: ValueError.
           guided_frames T (0 .. 3; needs guided=(radius, eps_q), the grey guide): temporal guided smoothing against flicker -- the
           filter's box also covers the T frames on each side of a frame (ops.guided_filter_time_np).  0, the default, is the
           per-frame filter fused into the batches.  With T >= 1 the batches run plain, then all frames of THIS call are filtered
           as one clip against their (resized) contents, then the colour op if content_colors: the result equals
           ops.guided_filter_time_np(predict_frames(frames, ...), contents, radius, eps_q, T), and content_colors_np after it, bit
           for bit, whatever `batch` is.  The radius is at most 51 / 40 / 33 at T = 1 / 2 / 3.  No swap5 or wrap with it.
           guided_motion (needs guided_frames >= 1): the temporal filter along camera motion -- one global integer translation per
           frame shifts the window in every neighbouring frame, so a clip that pans is averaged along its motion.  None, the
           default: no shift.  'global' or ('global', R): the positions are estimated from the contents the filter guides with
           (the resized ones with resize=; Context.motion_global, search range R = 8 by default, 1 .. 16).  An int array [F][2] of
           (py, px): the caller's positions, steps of at most 16.  The result equals ops.guided_filter_time_np(plain frames,
           contents, radius, eps_q, T, positions=ops.motion_global_np(contents, R)) bit for bit, whatever `batch` is.  A scene cut
           yields an arbitrary step, which the filter treats like any edge.  Per-block or dense motion, sub-pixel shifts, rotation
           and zoom are not served.
           guided_frames_guide (needs guided_frames >= 1): the guide of the filter along time -- None or 'grey', the grey of the
           contents, or 'color', their three channels (Context.guided_filter_time(..., guide='color')), which keeps an edge between
           two colours of equal luminance that the grey guide blurs.  It goes with guided_motion (the positions are estimated on
           the grey guide), runs before content_colors, and the result equals ops.guided_filter_time_np(plain frames, contents,
           radius, eps_q, T, positions=..., guide='color') bit for bit, whatever `batch` is.  Not served with guided_upsample.
           guided_upsample (short_side, radius, eps_q): as in predict -- every raw uint8 frame goes up at its own size, is resized
           and stylized at the working size and upsampled against itself; frame f equals predict(frames[f], style,
           guided_upsample=...) bit for bit, at the frames' size.  No swap5, warm, resize, wrap, strengths or guided* with it.
           guided_upsample_frames T (0 .. 3; needs guided_upsample, the grey guide): guided upsampling with the temporal box -- the
           frames are resized to the working size on the device and stylized plain there, then all frames of THIS call are
           delivered as one clip: the coefficients of the upsampling and their means are formed over the T frames on each side of
           a frame of the SMALL clip (ops.guided_upsample_time_np), every frame is evaluated against its own full content, then the
           colour op if content_colors.  The result equals ops.guided_upsample_time_np(predict_frames(small contents, ...), small
           contents, frames, radius, eps_q, T), and content_colors_np after it, bit for bit, whatever `batch` is.  0, the default,
           is the call above, untouched; T >= 1 on one frame gives its bytes.  The radius is at most 51 / 40 / 33 at T = 1 / 2 / 3.
           guided_upsample_motion (needs guided_upsample_frames >= 1): as guided_motion, in pixels of the SMALL frames -- None,
           'global' or ('global', R) (Context.motion_global on the small contents), or an int array [F][2] of positions.'''
        guided = self._check_guided(guided)                                       # ValueError before any GPU call
        frames = np.asarray(frames)
        if guided_upsample is None and (guided_upsample_frames or guided_upsample_motion is not None):
            raise ValueError('guided_upsample_frames and guided_upsample_motion need guided_upsample=(short_side, radius, eps_q): they '
                             'extend that call along time')
        if guided_upsample is not None and not guided_upsample_frames and guided_upsample_motion is not None:
            raise ValueError('guided_upsample_motion needs guided_upsample_frames >= 1: it shifts the windows of that box along time')
        if guided_upsample is not None and guided_upsample_frames:
            return self._predict_upsampled_time(frames, style, guided_upsample, guided_upsample_frames, guided_upsample_motion, alpha,
                                                adain, content_colors, batch,
                                                dict(swap5=swap5, warm=warm is not None, resize=resize is not None, wrap=wrap,
                                                     strengths=strengths is not None, guided=guided is not None,
                                                     guided_frames=bool(guided_frames), guided_motion=guided_motion is not None,
                                                     guided_frames_guide=guided_frames_guide is not None))
        if guided_upsample is not None:
            return self._predict_upsampled(frames, style, guided_upsample, alpha, adain, content_colors, batch,
                                           dict(swap5=swap5, warm=warm is not None, resize=resize is not None, wrap=wrap,
                                                strengths=strengths is not None, guided=guided is not None,
                                                guided_frames=bool(guided_frames), guided_motion=guided_motion is not None,
                                                     guided_frames_guide=guided_frames_guide is not None))
        temporal = self._check_guided_frames(guided, guided_frames, swap5, wrap, guided_frames_guide)
        motion = self._check_guided_motion(guided_motion, temporal, frames, resize)
        if temporal:
            return self._predict_frames_smoothed(frames, style, guided, int(guided_frames), content_colors, resize,
                                                 dict(alpha=alpha, adain=adain, batch=batch, warm=warm, strengths=strengths), motion,
                                                 guide=guided_frames_guide or 'grey')
        if strengths is not None:
            from ._lib import strength_maps_frames
            if frames.ndim != 4 or frames.shape[3] != 3:
                raise ValueError('expected [F][H][W][3] frames, got shape %s' % (frames.shape,))
            if resize is not None:
                resize = check_resize(resize)                                     # ValueError before any GPU call
            shape = resize or frames.shape[1:3]
            strengths = strength_maps_frames(strengths, len(frames), shape)       # ValueError before any GPU call
            self._strength_refusals(shape, swap5, None, wrap)
            if warm is not None:
                self._check_warm(warm, style, swap5, adain)
            if isinstance(style, PreparedStyle):
                check_prepared(self.sess, [style], self.relu_targets)
            if frames.dtype != np.uint8:
                frames = np.uint8(np.clip(frames, 0, 255))
            own = None if isinstance(style, PreparedStyle) else self.prepare_style(np.asarray(style), adain=adain)
            try:
                batch = max(1, min(32, int(batch)))
                return np.concatenate([self.sess.stylize_prepared_strength_batch(
                    frames[i:i + batch], own or style, strengths[i:i + batch], self.relu_targets, alpha=alpha, adain=adain,
                    wct_mode=self.wct_mode, warm=warm, content_colors=content_colors, guided=guided, resize=resize)
                    for i in range(0, len(frames), batch)], axis=0)
            finally:
                if own is not None:
                    own.close()
        if wrap:
            if not isinstance(style, PreparedStyle):
                raise ValueError('wrap takes a PreparedStyle (prepare_style), not a style image')
            for name, on in (('swap5', swap5), ('warm', warm is not None), ('content_colors', content_colors),
                             ('resize', resize is not None), ('guided', guided is not None)):
                if on:
                    raise ValueError('%s is not served with wrap: the periodic path takes one prepared style, WCT or AdaIN' % name)
            if frames.ndim != 4 or frames.shape[3] != 3:
                raise ValueError('expected [F][H][W][3] frames, got shape %s' % (frames.shape,))
            check_wrap(frames.shape[1], frames.shape[2], self.relu_targets)
            check_prepared(self.sess, [style], self.relu_targets)
            if frames.dtype != np.uint8:
                frames = np.uint8(np.clip(frames, 0, 255))
            batch = max(1, min(32, int(batch)))
            return np.concatenate([self.sess.stylize_prepared_wrap_batch(frames[i:i + batch], style, self.relu_targets, alpha=alpha,
                                                                         adain=adain, wct_mode=self.wct_mode)
                                   for i in range(0, len(frames), batch)], axis=0)
        if warm is not None:
            self._check_warm(warm, style, swap5, adain)                           # ValueError before any GPU call
        if resize is not None:
            resize = check_resize(resize)                                         # ValueError before any GPU call
            if swap5 is True and self.ss_stride != 1:
                raise ValueError('resize with swap5 needs ss_stride 1: a larger stride crops the resized frames on the host')
        if isinstance(style, PreparedStyle):
            check_prepared(self.sess, [style], self.relu_targets, swap5)          # ValueError before any GPU call
            assert frames.ndim == 4
            if frames.dtype != np.uint8:
                frames = np.uint8(np.clip(frames, 0, 255))
            batch = max(1, min(32, int(batch)))
            return np.concatenate([self.sess.stylize_prepared_batch(frames[i:i + batch], style, self.relu_targets, alpha=alpha,
                                                                    adain=adain, wct_mode=self.wct_mode, warm=warm,
                                                                    content_colors=content_colors, guided=guided, resize=resize)
                                   for i in range(0, len(frames), batch)], axis=0)
        style = np.asarray(style)
        assert frames.ndim == 4 and style.ndim == 3
        if frames.dtype != np.uint8:
            frames = np.uint8(np.clip(frames, 0, 255))
        if style.dtype != np.uint8:
            style = np.uint8(np.clip(style, 0, 255))
        if swap5 is True and self.ss_stride != 1:
            from .utils import swap_filter_fit, center_crop_to
            should_refit, H, W = swap_filter_fit(frames.shape[1], frames.shape[2], self.ss_patch_size, self.ss_stride)
            if should_refit:
                frames = np.stack([center_crop_to(f, H, W) for f in frames])
        if swap5:
            self.sess.set_style_swap(ss_alpha, self.ss_patch_size, self.ss_stride)
        batch = max(1, min(32, int(batch)))
        outs = [self.sess.stylize_batch(frames[i:i + batch], style, self.relu_targets, alpha=alpha, adain=adain,
                                        wct_mode=self.wct_mode, swap5=bool(swap5), content_colors=content_colors, guided=guided, resize=resize)
                for i in range(0, len(frames), batch)]
        return np.concatenate(outs, axis=0)

    def synthesize(self, style, size, seeds=1, seed=0, passes=3, alpha=1, adain=False, smooth=False, batch=16, weights=None,
                   swap5=False, tile=False):
        '''Texture synthesis (Li et al. 2017, sec. 4.3; the reference's webcam.py --noise and the recipe of stylize.py:95-97): seeded
           noise images of `size` (H, W) go through the pipeline `passes` times and come out as samples of the style's texture.
           `style` is an image (array in [0,255]: prepared here and closed afterwards) or a PreparedStyle.  `seeds` is a count n
           -- samples 0 .. n-1 of `seed` -- or a list of sample indices; every (seed, sample) is its own noise image
           (ops.texture_noise_np gives it), so a sample does not depend on which others were asked for with it.  `smooth`: the
           noise under the 27 202 27 filter of stylize.py:95-97.  Returns uint8 [n][Ho][Wo][3]; the first pass can grow the frame
           (Context.texture_size).  The noise is made on the device and the passes feed each other there, for up to `batch`
           (<= 32) consecutive sample indices per call; each sample equals predict_frames repeated `passes` times on its noise,
           bit for bit.
           Texture interpolation (Fig. 9 of the paper): `style` is a LIST of images or of PreparedStyle objects and `weights` the
           mix weights (None: equal).  Each sample then takes its noise from texture_noise_np and `passes` x predict_mix on the
           handles -- one sample at a time, through the host between passes, because the mix path is single-frame.  Batched
           mixes, masks and warm states are not part of this call.
           tile: seamless textures (Context.texture_prepared_wrap_batch) -- every pass runs on a torus, so a sample can be
           repeated in both directions without a seam.  One style only (a list is a ValueError: the mix path is single-frame);
           H and W multiples of the deepest level's stride; the samples keep the noise's size.'''
        h, w, samples, runs, batch = texture_plan(style, size, seeds, seed, passes, batch, weights, swap5)   # ValueError, no GPU call
        if tile:
            if isinstance(style, (list, tuple)):
                raise ValueError('tile takes one style: texture interpolation runs on the single-frame mix path, which has no '
                                 'periodic form')
            check_wrap(h, w, self.relu_targets)                                                             # ValueError, no GPU call
        if isinstance(style, (list, tuple)):
            from .ops import texture_noise_np
            handles, images = split_styles(list(style))
            if handles:
                check_prepared(self.sess, handles, self.relu_targets)
            own = [] if handles else [self.prepare_style(np.asarray(s), adain=adain) for s in images]
            try:
                outs = []
                for v in samples:
                    img = texture_noise_np(h, w, seed, v, smooth, ctx=self.sess)
                    for _ in range(passes):
                        img = self.predict_mix(img, handles or own, weights, alpha=alpha, adain=adain)
                    outs.append(img)
                return np.stack(outs)
            finally:
                for hd in own:
                    hd.close()
        if isinstance(style, PreparedStyle):
            check_prepared(self.sess, [style], self.relu_targets)
        handle = style if isinstance(style, PreparedStyle) else self.prepare_style(np.asarray(style), adain=adain)
        call = self.sess.texture_prepared_wrap_batch if tile else self.sess.texture_prepared_batch
        try:
            return np.concatenate([call(h, w, n, seed, first, handle, self.relu_targets, passes=passes, alpha=alpha, adain=adain,
                                        wct_mode=self.wct_mode, smooth=smooth)
                                   for first, n in runs], axis=0)
        finally:
            if handle is not style:
                handle.close()
