"""Drop-in ``DDP`` segmentor (plugin surface #1) for MMSegmentation-style configs.

Keeps the constructor kwargs, attribute names, ``state_dict`` keys and the inference methods of
segmentation/mmseg/models/segmentors/ddp.py:49-290 (``extract_feat``, ``encode_decode``, ``whole_inference``,
``inference``, ``simple_test``, ``aug_test``, ``ddim_sample``, ``ddpm_sample``, ``_decode_head_forward_test``,
``_get_sampling_timesteps``) while
the K-step loop itself runs in libddp_mi355x.so through ``DDPEngine``.  Unlike the reference, whose
sampler only works for one image per call (ddp.py:219-223 allocates the noisy map with batch
``randsteps``), ``ddim_sample`` accepts b >= 1 images and draws independent noise for each.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import schedule
from ..registry import SEGMENTORS, build_backbone, build_head, build_neck


class LearnedSinusoidalPosEmb(nn.Module):
    """parameter holder for time_mlp.0 (ddp.py:31-46); evaluated on device by k_sinusoid."""

    def __init__(self, dim):
        super().__init__()
        assert dim % 2 == 0
        self.weights = nn.Parameter(torch.randn(dim // 2))


class _Conv1x1(nn.Module):
    """``ConvModule(cin, cout, 1, norm_cfg=None, act_cfg=None)`` parameter holder: key ``conv.*``."""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 1)


def _build_neck(neck):
    if neck is None:
        return None
    if isinstance(neck, (list, tuple)):      # the DDP configs chain FPN -> MultiStageMerging: one fused C entry (necks/chain.py)
        from ..necks import NeckChain
        return NeckChain(*[build_neck(n) for n in neck])
    return build_neck(neck)


class _SamplerMixin:
    """engine cache shared by the task variants.

    One ``PackedWeights`` blob per (device, weights version) and a small LRU of engines keyed by everything EXCEPT the
    geometry: a new (batch, h, w) - the normal case under the reference's test protocol, one keep-ratio-resized image per
    call (segmentation/tools/test.py:214-219, mmseg/apis/test.py:87-89) - re-uses the engine through ``set_geometry`` (positional
    tables + workspace carve only; no weight repacking, no ``ddp_prepare``)."""
    ENGINE_CACHE_SIZE = 4

    def _weights_version(self):
        return sum(p._version for p in self.parameters())

    def _packed_weights(self, device, task, num_layers):
        from ..engine import PackedWeights
        ver = self._weights_version()
        cache = self.__dict__.setdefault('_weights_cache', {})
        key = (str(device), task, num_layers)
        hit = cache.get(key)
        if hit is None or hit[0] != ver:
            hit = (ver, PackedWeights(self.hot_path_state_dict(), task, num_layers, device))
            cache[key] = hit
        return hit[1]

    def _given(self, image_base=None, call=None, *, hints=None, prior=None, t_start=None, class_prior=None, score_prior=None,
               on_device=False):
        """the keyword arguments that were given, to be handed down the call chain - a None produces no key, so that a model without
        conditioning and without ``noise_seed`` calls its (possibly replaced) members with the reference's positional arguments and
        nothing else.  ``image_base`` / ``call`` (the noise key) travel only with ``noise_seed``; ``prior`` and ``t_start`` travel
        together whenever either is given; ``on_device`` only when true."""
        kw = dict(hints=hints, class_prior=class_prior, score_prior=score_prior)
        if getattr(self, 'noise_seed', None) is not None:
            kw.update(image_base=image_base, call=call)
        kw = {k: v for k, v in kw.items() if v is not None}
        if prior is not None or t_start is not None:
            kw.update(prior=prior, t_start=t_start)
        if on_device:
            kw['on_device'] = True
        return kw

    # what cannot be given per slide window or per augmentation, in the order each entry has always refused it: who, its one buffer
    _FRAME_BOUND = {'score_prior': ('score_prior is', 'score prior map'), 'prior': ('prior / t_start are', 'prior map'),
                    'hints': ('hints are', 'hint map')}
    _FRAMES = {'slide inference': ('one {} per sampler call, not per window', ('score_prior', 'prior', 'hints')),
               'aug_test': ('every augmentation has its own frame', ('score_prior', 'hints', 'prior'))}

    @classmethod
    def _refuse_frame_bound(cls, where, hints=None, prior=None, t_start=None, score_prior=None):
        """ValueError for an input that lives in the frame of one sampler call, given to ``where`` = 'slide inference' | 'aug_test'"""
        why, order = cls._FRAMES[where]
        given = dict(score_prior=score_prior, prior=prior if prior is not None else t_start, hints=hints)
        for name in order:
            if given[name] is not None:
                who, buffer = cls._FRAME_BOUND[name]
                raise ValueError(f'{who} not built for {where} ({why.format(buffer)})')

    @staticmethod
    def _hint_map(hints, b, h, w, dtype):
        """``hints`` (b, Hh, Wh) in the frame of the network input ``img`` (or a one-element augmentation list of it) -> the (b, h, w)
        hint map of the engine (DDP_FLAG_X0_HINTS), brought to the map resolution with ``F.interpolate(mode='nearest')`` - the rule
        ``forward_train`` resamples its label map with (segmentors/ddp.py:149).  Depth uses nearest too: a sparse map's holes (0 =
        free) must not be averaged into their neighbours."""
        if isinstance(hints, (list, tuple)):
            if len(hints) != 1:
                raise ValueError('hints: test-time augmentation takes no hints (one hint map per batch, not one per augmentation)')
            hints = hints[0]
        if not torch.is_tensor(hints) or hints.dim() != 3 or hints.shape[0] != b:
            raise ValueError(f'hints must be a (batch, H, W) tensor for a batch of {b} images, got '
                             f'{tuple(hints.shape) if torch.is_tensor(hints) else type(hints)}')
        m = F.interpolate(hints[:, None].float(), size=(h, w), mode='nearest')[:, 0]
        return m.to(dtype).contiguous()

    @classmethod
    def _prior_map(cls, prior, b, h, w, dtype):
        """``prior`` (b, Hp, Wp) in the frame of the network input -> the (b, h, w) prior map of the engine (DDP_FLAG_PRIOR_START),
        brought to the map resolution with nearest resampling by the rule of ``_hint_map`` (classes and bit words cannot be averaged;
        a depth map's holes must not leak into their neighbours).  Integer maps are resampled by index, so that bit words above 2^24
        survive."""
        if isinstance(prior, (list, tuple)):
            if len(prior) != 1:
                raise ValueError('prior: test-time augmentation takes no prior (one prior map per batch, not one per augmentation)')
            prior = prior[0]
        if not torch.is_tensor(prior) or prior.dim() != 3 or prior.shape[0] != b:
            raise ValueError(f'prior must be a (batch, H, W) tensor for a batch of {b} images, got '
                             f'{tuple(prior.shape) if torch.is_tensor(prior) else type(prior)}')
        if prior.dtype.is_floating_point:
            return cls._hint_map(prior, b, h, w, dtype)
        # F.interpolate(mode='nearest'): src = min(floor(dst * (in / out)), in - 1), the scale in float32 as ATen computes it
        H, W = prior.shape[1:]
        iy = (torch.arange(h, dtype=torch.float32) * torch.tensor(H / h, dtype=torch.float32)).floor().long().clamp(max=H - 1)
        ix = (torch.arange(w, dtype=torch.float32) * torch.tensor(W / w, dtype=torch.float32)).floor().long().clamp(max=W - 1)
        return prior[:, iy.to(prior.device)][:, :, ix.to(prior.device)].to(dtype).contiguous()

    def _class_prior_table(self, class_prior, b, device, repeat=1):
        """``class_prior`` (b, num_classes) float -> the float32 rows of the engine's class prior table (DDP_FLAG_CLASS_PRIOR) on
        ``device``.  An image-level prior has no frame: ``repeat`` > 1 tiles the rows for the windows of a slide chunk (window-major,
        the order of the chunk's maps), every window of image i getting row i."""
        if not torch.is_tensor(class_prior) or class_prior.dim() != 2 or tuple(class_prior.shape) != (b, self.num_classes) \
                or not class_prior.dtype.is_floating_point:
            raise ValueError(f'class_prior must be a float (batch, num_classes) = ({b}, {self.num_classes}) tensor, got '
                             f'{tuple(class_prior.shape) if torch.is_tensor(class_prior) else type(class_prior)}')
        t = class_prior.to(device=device, dtype=torch.float32)
        return (t.repeat(repeat, 1) if repeat > 1 else t).contiguous()

    def _score_prior_map(self, score_prior, b, h, w, device):
        """``score_prior`` (b, num_classes, H, W) float -> the float32 NCHW map of the engine (DDP_FLAG_SCORE_PRIOR) on ``device``: a map
        that is not at the map resolution (h, w) is resized there as the scores are resized on the way out,
        ``F.interpolate(mode='bilinear', align_corners=self.align_corners)``, on the device.  (Bilinear weights mix neighbours: an
        excluded class, ``-inf``, stays excluded only on pixels all of whose neighbours exclude it - give such a map at (h, w).)"""
        if not torch.is_tensor(score_prior) or score_prior.dim() != 4 or tuple(score_prior.shape[:2]) != (b, self.num_classes) \
                or not score_prior.dtype.is_floating_point:
            raise ValueError(f'score_prior must be a float (batch, num_classes, H, W) = ({b}, {self.num_classes}, H, W) tensor, got '
                             f'{tuple(score_prior.shape) if torch.is_tensor(score_prior) else type(score_prior)}')
        t = score_prior.to(device=device, dtype=torch.float32)
        if tuple(t.shape[2:]) != (h, w):
            t = F.interpolate(t, size=(h, w), mode='bilinear', align_corners=self.align_corners)
        return t.contiguous()

    @staticmethod
    def _check_t_start(prior, t_start):
        if prior is not None and t_start is None:
            raise ValueError('prior= needs t_start= (the time the prior map is noised to; 1.0 drowns it in noise)')

    def _conditioning(self, b, h, w, device, dtype, hints=None, prior=None, t_start=None, class_prior=None, score_prior=None):
        """the call-time inputs of one sampler call on a (b, h, w) map -> (what they ask of the engine: True per input given, ``prior``
        and ``t_start`` together whenever either is; {engine input: its tensor, resampled to the map, on ``device``}).  ``dtype``: the
        task's hint / prior map dtype."""
        self._check_t_start(prior, t_start)
        maps = {}
        if hints is not None:
            maps['hints'] = self._hint_map(hints, b, h, w, dtype).to(device)
        if prior is not None:
            maps['prior'] = self._prior_map(prior, b, h, w, dtype).to(device)
        if class_prior is not None:
            maps['class_prior'] = self._class_prior_table(class_prior, b, device)
        if score_prior is not None:
            maps['score_prior'] = self._score_prior_map(score_prior, b, h, w, device)
        asks = dict.fromkeys(maps, True)
        if prior is not None or t_start is not None:
            asks.update(prior=prior is not None, t_start=t_start)
        return asks, maps

    def _run(self, eng, maps, x, noise=None, step_noise=None, return_steps=False, image_base=0, call=0):
        """write ``maps`` (of ``_conditioning``) to the engine and sample: on ``noise`` (and ``step_noise``), or - None - on the noise
        of (noise_seed, image_base, call); -> out, or with ``return_steps`` (out, step record, step disagreement)"""
        for name, t in maps.items():
            getattr(eng, 'set_' + name)(t)
        x = x.contiguous().float()
        if noise is None:
            out = eng.sample(x, seed=self.noise_seed, image_base=image_base, call=call)
        else:
            out = eng.sample(x, noise.contiguous().float(), None if step_noise is None else step_noise.contiguous().float())
        return (out, eng.step_record(), eng.step_disagreement()) if return_steps else out

    def _get_engine(self, key, factory, geometry=None):
        cache = self.__dict__.setdefault('_engine_cache', {})
        ver = self._weights_version()
        for k in [k for k in cache if k[-1] != ver]:      # weights changed: every cached engine is stale
            del cache[k]
        key = key + (ver,)
        eng = cache.pop(key, None)
        if eng is None:
            eng = factory()
            while len(cache) >= self.ENGINE_CACHE_SIZE:
                cache.pop(next(iter(cache)))               # least recently used
        elif geometry is not None:
            eng.set_geometry(*geometry)
        cache[key] = eng                                   # most recently used last
        return eng


@SEGMENTORS.register_module()
class DDP(nn.Module, _SamplerMixin):
    task = 'seg'
    # not a reference kwarg (the constructor's stay the reference's): set ``model.ddpm_chain = True`` to run ``diffusion='ddpm'`` /
    # ``ddpm_sample`` on the fused step boundary of the ddim sampler (DDP_FLAG_DDPM_CHAIN); results agree with the default route to
    # rounding.  Part of the engine key: flipping it builds (or re-uses) the other engine
    ddpm_chain = False

    def __init__(self, bit_scale=0.1, timesteps=1, randsteps=1, time_difference=1, learned_sinusoidal_dim=16,
                 sample_range=(0, 0.999), noise_schedule='cosine', diffusion='ddim', accumulation=False,
                 backbone=None, neck=None, decode_head=None, auxiliary_head=None, train_cfg=None, test_cfg=None,
                 pretrained=None, init_cfg=None, noise_seed=None):
        """``noise_seed`` (not a reference kwarg): None - the noise is drawn with torch.randn per call, as the reference does; an
        integer - start and step noise are generated on the device (DDP_FLAG_SEEDED_NOISE) from (noise_seed, image index, call),
        so an image's result does not depend on the batch it was in, on the rank it ran on or on the calls before it."""
        super().__init__()
        self.noise_seed = noise_seed
        if noise_schedule not in schedule.NOISE_SCHEDULES:
            raise ValueError(f'invalid noise schedule {noise_schedule}')            # ddp.py:90
        if learned_sinusoidal_dim != 16:
            raise ValueError('libddp_mi355x is built for learned_sinusoidal_dim=16')
        self.backbone = build_backbone(backbone) if backbone is not None else None
        self.neck = _build_neck(neck)
        self.decode_head = build_head(decode_head)
        self.auxiliary_head = None           # training-only deep supervision: out of scope
        self.align_corners = self.decode_head.align_corners
        self.num_classes = self.decode_head.num_classes
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.bit_scale, self.timesteps, self.randsteps = bit_scale, timesteps, randsteps
        self.diffusion, self.time_difference = diffusion, time_difference
        self.sample_range, self.noise_schedule = sample_range, noise_schedule
        self.use_gt = False
        self.accumulation = accumulation
        c = self.decode_head.in_channels[0]
        self.embedding_table = nn.Embedding(self.num_classes + 1, c)
        self.transform = _Conv1x1(c * 2, c)
        time_dim = c * 4
        self.time_mlp = nn.Sequential(LearnedSinusoidalPosEmb(learned_sinusoidal_dim),
                                      nn.Linear(learned_sinusoidal_dim + 1, time_dim), nn.GELU(),
                                      nn.Linear(time_dim, time_dim))

    # -- plugin surface ------------------------------------------------------------------------
    @property
    def with_neck(self):
        return self.neck is not None

    def extract_feat(self, img):
        x = self.backbone(img)
        if self.with_neck:
            x = self.neck(x)
        return x

    def _get_sampling_timesteps(self, batch, *, device):
        times = []
        for t_now, t_next in schedule.get_sampling_timesteps(self.timesteps, self.time_difference,
                                                             self.sample_range[0]):
            t = torch.tensor([t_now, t_next], device=device)
            times.append(t[:, None].repeat(1, batch))
        return times

    def _engine_for(self, b, h, w, device, sampler, timesteps=None, randsteps=None, accumulation=None, kind='sample',
                    record_steps=False, seeded=False, hints=False, prior=False, t_start=None, class_prior=False,
                    score_prior=False):
        from ..decode_heads.fcn_head_with_time import FCNHeadWithTime
        K = self.timesteps if timesteps is None else timesteps
        r = self.randsteps if randsteps is None else randsteps
        acc = self.accumulation if accumulation is None else accumulation
        common = dict(batch=b, randsteps=r, timesteps=K, num_classes=self.num_classes, bit_scale=self.bit_scale,
                      time_difference=self.time_difference, sample_range0=self.sample_range[0],
                      noise_schedule=self.noise_schedule, sampler=sampler, accumulation=acc, device=device,
                      record_steps=record_steps, seeded_noise=seeded)
        ts = 1.0 if t_start is None else float(t_start)
        chain = bool(self.ddpm_chain) and sampler == 'ddpm'
        key = (kind, str(device), sampler, K, r, acc, self.bit_scale, self.time_difference, self.sample_range[0],
               self.noise_schedule, bool(record_steps), bool(seeded), chain, bool(hints), bool(prior), ts, bool(class_prior),
               bool(score_prior))
        if isinstance(self.decode_head, FCNHeadWithTime):
            if score_prior:
                raise ValueError('score_prior is built for the deformable head\'s sampler: the FCNHeadWithTime loop takes none')
            if class_prior:
                raise ValueError('class_prior is built for the deformable head\'s sampler: the FCNHeadWithTime loop takes none')
            if prior or ts != 1.0:
                raise ValueError('prior / t_start are built for the deformable head\'s sampler: the FCNHeadWithTime loop starts from noise')
            if hints:
                raise ValueError('hints are built for the deformable head\'s sampler: the FCNHeadWithTime loop takes none')
            if chain:
                raise ValueError('ddpm_chain is a route of the deformable head\'s sampler: the FCNHeadWithTime loop has no u chain')
            # any registered head goes through _decode_head_forward_test in the reference (ddp.py:192-196); here the loop
            # around FCNHeadWithTime is its own C entry (ddp_sample_fcn), one engine per geometry
            def factory():
                from ..engine import FcnSamplerEngine
                return FcnSamplerEngine(self.hot_path_state_dict(), self.decode_head, h=h, w=w, **common)
            return self._get_engine(key + ('fcn', b, h, w), factory)

        def factory():
            from ..engine import DDPEngine, count_layers
            nl = count_layers(self.hot_path_state_dict())
            return DDPEngine(None, 'seg', h=h, w=w, feat_channels=256, weights=self._packed_weights(device, 'seg', nl),
                             ddpm_chain=chain, x0_hints=bool(hints), prior_start=bool(prior), t_start=ts,
                             class_prior=bool(class_prior), score_prior=bool(score_prior), **common)
        return self._get_engine(key, factory, geometry=(b, h, w))

    def hot_path_state_dict(self):
        return {k: v for k, v in self.state_dict().items()
                if not k.startswith(('backbone.', 'neck.', 'auxiliary_head.'))}

    def _check_feature(self, x):
        if not x.is_cuda:
            raise RuntimeError('ddp_amd has no CPU path: features must live on an MI355X (HIP) device')
        if x.shape[1] != self.decode_head.in_channels[0]:
            raise RuntimeError(f'expected {self.decode_head.in_channels[0]} feature channels, got {x.shape[1]}')

    @torch.no_grad()
    def ddim_sample(self, x, img_metas=None, noise=None, return_steps=False, image_base=0, call=0, hints=None, prior=None,
                    t_start=None, class_prior=None, score_prior=None):
        """``score_prior`` (b, num_classes, H, W) float (call-time only; DDP_FLAG_SCORE_PRIOR): entry [i][k][y][x] is added to the
        conv_seg score of class k at that pixel of image i at every step, in front of the argmax that is fed back, the accumulated
        softmax and the scores returned - what the sampler computes when the decode head returns ``scores + score_prior[i]``.  A map
        that is not at (h, w) is resized there (bilinear, ``align_corners`` of the model).  ``-inf`` excludes a class at a pixel; NaN
        reads as 0; adds to ``class_prior``.
        ``class_prior`` (b, num_classes) float (call-time only; DDP_FLAG_CLASS_PRIOR): row i is added to the conv_seg scores of
        image i at every step, in front of the argmax that is fed back, the accumulated softmax and the scores returned - what a
        model with ``conv_seg.bias + class_prior[i]`` would compute for image i.  ``-inf`` excludes a class
        (``ddp_amd.engine.class_mask_to_prior``); NaN reads as 0.
        ``prior`` (b,Hp,Wp) uint8 in the frame of the network input with ``t_start`` in (sample_range[0], 1] (call-time only;
        DDP_FLAG_PRIOR_START): the chain starts from the prior's classes (a value >= num_classes: the ignore row) noised to
        ``t_start`` instead of from pure noise, and the K steps divide [sample_range[0], t_start]; resampled to (h,w) with nearest.
        ``t_start`` alone: the same time grid on the given / drawn ``noise`` as the start map.
        ``hints`` (b,Hh,Wh) uint8 in the frame of the network input (call-time only; DDP_FLAG_X0_HINTS): a class < num_classes is
        fed back as x0 at that pixel in place of the argmax at every step, any other value (255) leaves the pixel free; resampled to
        (h,w) with nearest.  The scores returned (and ``return_steps``' record) stay the model's own; ``timesteps=1``: no effect.
        x (b,256,h,w) -> (b,K,h,w).  ``noise`` (b,r,256,h,w) may be injected (parity tests);
        by default it is drawn with torch.randn like the reference (ddp.py:220).
        With ``self.noise_seed`` set and no ``noise``: image i of the batch gets the noise of (noise_seed, image_base + i, call).
        ``return_steps``: -> (out, record (K,b,r,h,w) uint8 - every step's argmax class, the reference's ``outs`` as decisions -,
        disagreement (b,h,w) - the fraction of them that differ from the output's argmax)."""
        self._check_feature(x)
        return self._sample_with('ddim', x, noise, None, return_steps, image_base, call, hints=hints, prior=prior, t_start=t_start,
                                 class_prior=class_prior, score_prior=score_prior)

    def _sample_with(self, sampler, x, noise, step_noise, return_steps, image_base, call, **given):
        """the one body of ``ddim_sample`` and ``ddpm_sample``: the engine of (sampler, what is given), conditioned, run on the noise
        given, on the noise of ``noise_seed``, or on noise drawn here as the reference draws it"""
        b, c, h, w = x.shape
        asks, maps = self._conditioning(b, h, w, x.device, torch.uint8, **given)
        seeded = noise is None and step_noise is None and self.noise_seed is not None
        if not seeded:
            if noise is None:
                noise = torch.randn((b, self.randsteps, c, h, w), device=x.device)
            if step_noise is None and sampler == 'ddpm':
                step_noise = torch.randn((self.timesteps, b, self.randsteps, c, h, w), device=x.device)
        eng = self._engine_for(b, h, w, x.device, sampler, record_steps=return_steps, seeded=seeded, **asks)
        return self._run(eng, maps, x, noise, step_noise, return_steps, image_base, call)

    @torch.no_grad()
    def ddpm_sample(self, x, img_metas=None, noise=None, step_noise=None, return_steps=False, image_base=0, call=0, hints=None,
                    prior=None, t_start=None, class_prior=None, score_prior=None):
        """``hints``, ``prior``, ``t_start``, ``class_prior``, ``score_prior``: as ``ddim_sample``"""
        self._check_feature(x)
        return self._sample_with('ddpm', x, noise, step_noise, return_steps, image_base, call, hints=hints, prior=prior, t_start=t_start,
                                 class_prior=class_prior, score_prior=score_prior)

    def _decode_head_forward_test(self, x, t, img_metas=None):
        return self.decode_head.forward_test(x, t, img_metas, self.test_cfg)

    def encode_decode(self, img, img_metas=None, image_base=0, call=0, class_prior=None, score_prior=None):
        """ddp.py:114-129.  ``score_prior``: see ``ddim_sample``."""
        x = self.extract_feat(img)[0]
        kw = self._given(image_base, call, class_prior=class_prior, score_prior=score_prior)
        if self.diffusion == 'ddim':
            out = self.ddim_sample(x, img_metas, **kw)
        elif self.diffusion == 'ddpm':
            out = self.ddpm_sample(x, img_metas, **kw)
        else:
            raise NotImplementedError
        return F.interpolate(out, size=img.shape[2:], mode='bilinear', align_corners=self.align_corners)

    def whole_inference(self, img, img_meta=None, rescale=False, image_base=0, call=0, class_prior=None, score_prior=None):
        """encoder_decoder.py:229-248: crop to img_shape and resize to ori_shape when rescale.  ``score_prior``: see ``ddim_sample``."""
        seg_logit = self.encode_decode(img, img_meta, **self._given(image_base, call, class_prior=class_prior, score_prior=score_prior))
        if rescale and img_meta:
            rs = img_meta[0]['img_shape'][:2]
            seg_logit = seg_logit[:, :, :rs[0], :rs[1]]
            seg_logit = F.interpolate(seg_logit, size=tuple(img_meta[0]['ori_shape'][:2]), mode='bilinear',
                                      align_corners=self.align_corners)
        return seg_logit

    def _mode(self):
        """encoder_decoder.py:266-271: ``test_cfg.mode`` in ('slide', 'whole'); every shipped DDP config is 'whole'
        (configs/ade/*:111, configs/cityscapes/*:96-98)."""
        cfg = self.test_cfg
        mode = (cfg.get('mode') if isinstance(cfg, dict) else getattr(cfg, 'mode', None)) if cfg is not None else None
        if mode not in (None, 'whole', 'slide'):
            raise AssertionError(f"test_cfg.mode must be 'slide' or 'whole', got {mode!r}")
        return mode or 'whole'

    def _sample(self, x, img_meta=None, image_base=0, call=0, class_prior=None):
        kw = self._given(image_base, call, class_prior=class_prior)
        if self.diffusion == 'ddim':
            return self.ddim_sample(x, img_meta, **kw)
        if self.diffusion == 'ddpm':
            return self.ddpm_sample(x, img_meta, **kw)
        raise NotImplementedError

    SLIDE_WINDOWS_PER_CALL = 16          # windows x images sampled in one call of the loop (memory bound of the workspace)

    def _slide(self, img, img_meta, rescale, want, flip=None, image_base=0, call=0, class_prior=None):
        """Sliding-window inference (encoder_decoder.py:180-227).  The reference runs ``encode_decode`` - backbone, neck and a
        K-step loop - window by window; the windows all have one size, so here they go through backbone + loop as ONE batch
        (chunks of SLIDE_WINDOWS_PER_CALL maps, independent noise per window as in the reference) and only their LOW-RESOLUTION
        scores are kept.  ``ddp_seg_slide_postprocess`` then does, per output pixel, what the reference does with image-size
        tensors: resize per window, ``preds += pad(...)`` in window order, ``/ count_mat``, crop to img_shape, resize to
        ori_shape, [softmax, flip-undo, argmax].
        With ``self.noise_seed`` set, every window-chunk is a sampler call of its own ``call`` value (``call`` + the chunk's index)
        and its maps - windows x images, window-major - draw the noise of images ``image_base``, ``image_base`` + 1, ...: no two
        windows of a call share noise, and no two chunks do."""
        from ..engine import seg_slide_postprocess, slide_windows
        cfg = self.test_cfg
        get = (lambda k: cfg[k]) if isinstance(cfg, dict) else (lambda k: getattr(cfg, k))
        ys, xs, (ch, cw) = slide_windows(img.shape[2:], get('crop_size'), get('stride'))
        b = img.shape[0]
        crops = [img[:, :, y1:y1 + ch, x1:x1 + cw] for y1 in ys for x1 in xs]
        per = max(1, self.SLIDE_WINDOWS_PER_CALL // b)
        lows = []
        for i in range(0, len(crops), per):
            chunk = crops[i:i + per]
            x = self.extract_feat(torch.cat(chunk, dim=0))[0]
            # (a class prior is image-level: every window of image i gets row i - the chunk's maps are window-major)
            rows = None if class_prior is None else self._class_prior_table(class_prior, b, x.device, repeat=len(chunk))
            low = self._sample(x, img_meta, **self._given(image_base, call + i // per, class_prior=rows))
            lows.append(low.reshape(len(chunk), b, self.num_classes, x.shape[2], x.shape[3]))
        scores = torch.cat(lows, dim=0)
        keep = out = None
        if rescale and img_meta:
            keep = tuple(img_meta[0]['img_shape'][:2])
            out = tuple(img_meta[0]['ori_shape'][:2])
        return seg_slide_postprocess(scores, ys, xs, (ch, cw), img.shape[2:], keep, out, self.align_corners, flip, want)

    def slide_inference(self, img, img_meta, rescale, image_base=0, call=0, hints=None, prior=None, t_start=None, class_prior=None,
                        score_prior=None):
        """``class_prior`` (b, num_classes): every window of image i samples with row i (see ``ddim_sample``).
        ``score_prior`` is not built for slide inference (ValueError).
        encoder_decoder.py:180-227: the window-averaged scores (b,K,H,W) (at ori_shape when ``rescale``)."""
        self._refuse_frame_bound('slide inference', hints, prior, t_start, score_prior)
        return self._slide(img, img_meta, rescale, 'scores', **self._given(image_base, call, class_prior=class_prior))

    def inference(self, img, img_meta, rescale, image_base=0, call=0, class_prior=None):
        """``class_prior`` (b, num_classes): see ``ddim_sample``.
        encoder_decoder.py:251-287, mode 'whole' (what every DDP config sets): class probabilities at ``ori_shape`` with
        the test-time flip undone - the building block of ``aug_test``.  ``simple_test`` does not go through here: its
        fused epilogue never materialises these (B,K,H,W) tensors."""
        mode = self._mode()
        kw = self._given(image_base, call, class_prior=class_prior)
        if img_meta:
            ori_shape = img_meta[0]['ori_shape']
            assert all(m['ori_shape'] == ori_shape for m in img_meta)
        if mode == 'slide':
            fl = None
            if img_meta and img_meta[0].get('flip', False):
                fl = img_meta[0].get('flip_direction', 'horizontal')
                assert fl in ('horizontal', 'vertical')
            return self._slide(img, img_meta, rescale, 'prob', fl, **kw)
        output = F.softmax(self.whole_inference(img, img_meta, rescale, **kw), dim=1)
        if img_meta and img_meta[0].get('flip', False):
            direction = img_meta[0].get('flip_direction', 'horizontal')
            assert direction in ('horizontal', 'vertical')
            output = output.flip(dims=(3,) if direction == 'horizontal' else (2,))
        return output

    AUG_CALL_STRIDE = 1 << 16            # seeded noise: augmentation a owns the call values [a * stride, (a + 1) * stride)

    @staticmethod
    def _deliver(seg, on_device):
        """the return value of the test entry points: int64 host arrays as in the reference, or - ``on_device`` - the uint8 device
        maps the epilogue wrote (no copy, no cast; ``ddp_amd.evaluation.seg_pre_eval`` reduces them where they are)"""
        if on_device:
            return list(seg if seg.dtype == torch.uint8 else seg.to(torch.uint8))
        return list(seg.cpu().numpy().astype('int64'))

    def aug_test(self, imgs, img_metas, rescale=True, image_base=0, hints=None, prior=None, t_start=None, class_prior=None,
                 score_prior=None, on_device=False):
        """``on_device``: see ``simple_test``.
        ``class_prior`` (b, num_classes): an image-level prior has no frame - every augmentation of image i samples with row i.
        ``hints``, ``prior``, ``t_start`` and ``score_prior`` are not built for test-time augmentation (ValueError).
        With ``self.noise_seed`` set, augmentation a samples with ``call`` = a (slide mode: a * AUG_CALL_STRIDE + the window-chunk
        index), so no two augmentations of an image share noise.
        encoder_decoder.py:306-331: mean of the per-augmentation probabilities (multi-scale / flip), then argmax.
        Every augmentation runs the full sampling loop with its own noise, as in the reference; only the LOW-RESOLUTION
        scores of each are kept, and one fused epilogue (``ddp_seg_aug_postprocess``) does resize -> crop -> resize ->
        softmax -> flip-undo for all of them, the mean and the argmax per output pixel: the (1,K,H,W) tensors ``inference``
        materialises per augmentation and the running sum at ori_shape never exist."""
        from ..engine import seg_aug_postprocess
        self._refuse_frame_bound('aug_test', hints, prior, t_start, score_prior)
        assert rescale, 'aug_test rescales every augmentation back to ori_shape'
        if len(imgs) != len(img_metas):
            raise ValueError(f'num of augmentations ({len(imgs)}) != num of image meta ({len(img_metas)})')
        if self._mode() == 'slide':
            # no shipped config combines sliding windows with test-time augmentation: the reference's own composition
            # (running mean of ``inference``, encoder_decoder.py:306-331) over the fused per-augmentation slide epilogue
            prob = self.inference(imgs[0], img_metas[0], rescale, **self._given(image_base, 0, class_prior=class_prior))
            for a, (img, meta) in enumerate(zip(imgs[1:], img_metas[1:]), 1):
                prob += self.inference(img, meta, rescale, **self._given(image_base, a * self.AUG_CALL_STRIDE, class_prior=class_prior))
            prob /= len(imgs)
            return self._deliver(prob.argmax(dim=1), on_device)
        ori_shape = tuple(img_metas[0][0]['ori_shape'][:2])
        scores, metas = [], []
        for a, (img, meta) in enumerate(zip(imgs, img_metas)):
            assert all(tuple(m['ori_shape'][:2]) == ori_shape for m in meta)
            scores.append(self._sample(self.extract_feat(img)[0], meta, **self._given(image_base, a, class_prior=class_prior)))
            metas.append(dict(img_size=tuple(img.shape[2:]), crop_size=tuple(meta[0]['img_shape'][:2]),
                              flip=meta[0].get('flip_direction', 'horizontal') if meta[0].get('flip', False) else None))
        seg = seg_aug_postprocess(scores, metas, ori_shape, self.align_corners)
        return self._deliver(seg, on_device)

    @staticmethod
    def _epilogue_args(meta, rescale):
        crop = out_size = flip = None
        if meta:
            if rescale:
                crop = tuple(meta['img_shape'][:2])
                out_size = tuple(meta['ori_shape'][:2])
            if meta.get('flip', False):
                flip = meta.get('flip_direction', 'horizontal')
        return crop, out_size, flip

    def simple_test(self, img, img_meta=None, rescale=True, image_base=0, hints=None, prior=None, t_start=None, class_prior=None,
                    score_prior=None, on_device=False):
        """``on_device=True``: return the list of uint8 (H, W) DEVICE tensors the epilogue wrote instead of int64 host arrays - no
        ``.cpu()``, no cast (``ddp_amd.apis.single_gpu_test(device_eval=True)``, ``ddp_amd.evaluation.seg_pre_eval``).
        ``score_prior`` (b, num_classes, H, W) float, in the frame of ``img`` or at the map resolution: see ``ddim_sample``; slide
        mode raises ValueError.
        ``class_prior`` (b, num_classes) float: see ``ddim_sample``; in slide mode every window of image i gets row i.
        ``prior`` (b,Hp,Wp) uint8 in the frame of ``img`` and ``t_start``: see ``ddim_sample``; slide mode raises ValueError.
        ``hints`` (b,Hh,Wh) uint8 in the frame of ``img``: see ``ddim_sample``; slide mode raises ValueError.
        encoder_decoder.py:250-304 (mode='whole'), post-loop epilogue fused into one kernel:
        the (1,K,H,W) resized scores / probabilities of the reference are never materialised.  ``img`` may hold
        b >= 1 images (§8 f4): the loop runs once on the whole batch with independent noise per image, and every
        image gets the crop / rescale / flip of its OWN ``img_meta`` entry (one epilogue launch per distinct geometry)."""
        from ..engine import seg_postprocess
        if self._mode() == 'slide':
            self._refuse_frame_bound('slide inference', hints, prior, t_start, score_prior)
            if img_meta and any(self._epilogue_args(m, rescale) != self._epilogue_args(img_meta[0], rescale) for m in img_meta):
                raise ValueError('slide inference: the images of a batch must share img_shape / ori_shape / flip')
            fl = self._epilogue_args(img_meta[0], rescale)[2] if img_meta else None
            # ('seg' = argmax of the window-averaged SCORES; the reference takes argmax of their softmax, encoder_decoder.py:277,296.
            # softmax is monotone, so the two agree except where fp32 rounding of exp / the division makes two probabilities EQUAL
            # that came from different scores - the reference then returns the lower class index, this path the class with the
            # larger score.  test_slide_epilogue_golden bounds it: identical wherever the reference's top-2 margin exceeds 1e-5.)
            return self._deliver(self._slide(img, img_meta, rescale, 'seg', fl, **self._given(image_base, 0, class_prior=class_prior)), on_device)
        kw = self._given(image_base, 0, hints=hints, prior=prior, t_start=t_start, class_prior=class_prior, score_prior=score_prior)
        x = self.extract_feat(img)[0]
        if self.diffusion == 'ddim':
            out = self.ddim_sample(x, img_meta, **kw)
        elif self.diffusion == 'ddpm':
            out = self.ddpm_sample(x, img_meta, **kw)
        else:
            raise NotImplementedError
        b = out.shape[0]
        if img_meta and len(img_meta) not in (1, b):
            raise ValueError(f'{len(img_meta)} img_metas for a batch of {b} images')
        args = [self._epilogue_args(img_meta[i if len(img_meta) == b else 0] if img_meta else None, rescale)
                for i in range(b)]
        if all(a == args[0] for a in args):
            seg = seg_postprocess(out, img.shape[2:], args[0][0], args[0][1], self.align_corners, args[0][2])
            return self._deliver(seg, on_device)
        res = []
        for i, (crop, out_size, flip) in enumerate(args):
            seg = seg_postprocess(out[i:i + 1].contiguous(), img.shape[2:], crop, out_size, self.align_corners, flip)
            res.extend(self._deliver(seg, on_device))
        return res

    def forward(self, img, img_metas=None, return_loss=False, rescale=True, image_base=0, hints=None, prior=None, t_start=None,
                class_prior=None, score_prior=None, on_device=False, **kwargs):
        """``on_device``: see ``simple_test``.
        ``score_prior``: see ``simple_test`` (``aug_test`` raises ValueError when given one).
        ``class_prior``: see ``simple_test`` / ``aug_test``.
        ``hints``, ``prior``, ``t_start``: see ``simple_test`` (``aug_test`` raises ValueError when given any).
        base.py:62-110 ``forward`` / ``forward_test``: ``img`` / ``img_metas`` may be the one-element
        augmentation lists the test pipeline produces."""
        if return_loss:
            raise NotImplementedError('training is out of scope of ddp_amd (SURVEY.md §8)')
        kw = self._given(image_base, hints=hints, prior=prior, t_start=t_start, class_prior=class_prior, score_prior=score_prior,
                         on_device=on_device)
        if isinstance(img, (list, tuple)):
            if len(img) != 1:
                if img_metas is None or len(img_metas) != len(img):
                    raise ValueError(f'num of augmentations ({len(img)}) != num of image meta ({0 if img_metas is None else len(img_metas)})')
                return self.aug_test(list(img), list(img_metas), rescale, **kw)
            img = img[0]
            if img_metas is not None:
                img_metas = img_metas[0]
        return self.simple_test(img, img_metas, rescale, **kw)

    def forward_train(self, *a, **k):
        raise NotImplementedError('training is out of scope of ddp_amd (SURVEY.md §8)')


@SEGMENTORS.register_module()
class SelfAlignedDDP(DDP):
    """segmentation/mmseg/models/segmentors/self_aligned_ddp.py:48-129: the self-aligned variant differs from DDP only
    in ``forward_train`` (:131-186); its inference surface - constructor kwargs, state_dict keys, ``encode_decode`` /
    ``ddim_sample`` / ``ddpm_sample`` - is DDP's, so the two Cityscapes ``*_aligned`` configs resolve to the same MI355X
    path.  The one piece of ``forward_train`` that is an inference pass - the no-grad "self-aligned denoising" pre-pass
    (:150-164) - is exposed as ``self_aligned_predict``."""

    @torch.no_grad()
    def self_aligned_predict(self, x, noise=None, return_logits=False, image_base=0, call=0, class_prior=None, score_prior=None):
        """``score_prior`` (b, num_classes, H, W): added to the pass's scores in front of the argmax (see ``ddim_sample``).
        ``class_prior`` (b, num_classes): added to the pass's scores in front of the argmax (see ``ddim_sample``).
        self_aligned_ddp.py:150-164: ONE decoder pass at t = 1 on pure noise, then the x0 projection:
            feat = transform(cat[x, noise]); logits = decode_head(feat, time_mlp(log_snr(1)))
            preds = (sigmoid(embedding_table(argmax(logits))) * 2 - 1) * bit_scale
        x (b,256,h,w) -> preds (b,256,h,w) [, logits (b,K,h,w)].  ``noise`` (b,256,h,w) replaces ``torch.randn_like(x)``.
        Runs as a 1-step sampler call (the step's t_now is 1 for every K; no update, no accumulation) followed by
        ``ddp_seg_x0_project``."""
        import ctypes as C

        from .. import _lib
        self._check_feature(x)
        b, c, h, w = x.shape
        asks, maps = self._conditioning(b, h, w, x.device, torch.uint8, class_prior=class_prior, score_prior=score_prior)
        seeded = noise is None and self.noise_seed is not None
        if noise is None and not seeded:
            noise = torch.randn_like(x)
        # the head dispatch of _engine_for (the reference's pre-pass goes through the generic _decode_head_forward_test)
        eng = self._engine_for(b, h, w, x.device, 'ddim', timesteps=1, randsteps=1, accumulation=False, kind='self_aligned',
                               seeded=seeded, **asks)
        logits = self._run(eng, maps, x, None if seeded else noise.reshape(b, 1, c, h, w), image_base=image_base, call=call)
        preds = torch.empty((b, 256, h, w), dtype=torch.float32, device=x.device)
        emb = self.embedding_table.weight.detach().float().contiguous()
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().ddp_seg_x0_project(logits.data_ptr(), b, self.num_classes, h * w, emb.data_ptr(),
                                                      C.c_float(self.bit_scale), preds.data_ptr(),
                                                      torch.cuda.current_stream(x.device).cuda_stream))
        return (preds, logits) if return_logits else preds
