"""Drop-in depth ``DDP`` + ``DeformableHeadWithTime`` (depth/depth/models/depther/ddp.py:34-247;
depth/depth/models/decode_heads/deformable_head_with_time.py:20-169): ``down`` concat-conv over
256+1 channels, raw-t time embedding, 3x3 ``conv_depth`` regression head, cosine-gamma DDIM step - and the toolbox's test
entry around it (depther/base.py:50-115 ``forward`` / ``forward_test``; encoder_decoder.py:130-235 ``whole_inference`` /
``inference`` / ``simple_test`` / ``aug_test``), so that ``depth/tools/test.py`` runs unchanged: ``model(return_loss=False,
**data)`` (depth/depth/apis/test.py:88,204).  Everything after the loop is ONE kernel (``ddp_depth_postprocess``)."""
import torch
import torch.nn as nn

from ..decode_heads.deformable_head_with_time import DeformableHeadWithTime as _SegHead
from ..registry import DEPTHER, HEADS, build_backbone, build_head
from ..segmentors.ddp import LearnedSinusoidalPosEmb, _Conv1x1, _SamplerMixin, _build_neck
from .. import _lib, schedule


@HEADS.register_module(name='DepthDeformableHeadWithTime')
class DepthDeformableHeadWithTime(_SegHead):
    task = 'depth'
    head_conv = 'conv_depth'

    def __init__(self, min_depth=1e-3, max_depth=None, scale_up=False, classify=False, use_eps=True, n_bins=256,
                 bins_strategy='UD', norm_strategy='linear', init_inputs=False, **kwargs):
        self.min_depth, self.max_depth = min_depth, max_depth
        self.scale_up, self.classify, self.use_eps = scale_up, classify, use_eps
        self.n_bins = n_bins
        if classify:
            # binned depth (decode_head.py:91-96,233-250): conv_depth to n_bins channels, expectation over the bin centres
            assert bins_strategy in ["UD", "SID"], "Support bins_strategy: UD, SID"
            assert norm_strategy in ["linear", "softmax", "sigmoid"], "Support norm_strategy: linear, softmax, sigmoid"
            if not isinstance(n_bins, int) or not 1 <= n_bins <= _lib.MAX_DEPTH_BINS:
                raise ValueError(f'libddp_mi355x supports 1..{_lib.MAX_DEPTH_BINS} depth bins, got n_bins={n_bins!r}')
            self.bins_strategy, self.norm_strategy = bins_strategy, norm_strategy
        kwargs.setdefault('num_classes', 1)
        super().__init__(**kwargs)

    def _make_head_conv(self):
        self.conv_depth = nn.Conv2d(self.channels, self.n_bins if self.classify else 1, kernel_size=3, padding=1, stride=1)

    def depth_bins(self):
        """The bin centres of a binned head, by the reference's own torch call (decode_head.py:238-241; CPU fp32): 'UD' linspace,
        'SID' logspace - base-10 exponents taken literally, as the reference does."""
        if not self.classify:
            return None
        if self.bins_strategy == 'UD':
            return torch.linspace(self.min_depth, self.max_depth, self.n_bins)
        return torch.logspace(self.min_depth, self.max_depth, self.n_bins)

    def _engine_kwargs(self):
        # the head alone: its own range is both the eps range and (unused by a head call) the x0 normalisation
        hmax = self.max_depth if self.max_depth is not None else 80.0
        kw = dict(min_depth=self.min_depth, max_depth=hmax, depth_scale_up=bool(self.scale_up), depth_use_eps=bool(self.use_eps))
        if self.classify:
            kw.update(depth_bins=self.depth_bins(), depth_norm=self.norm_strategy)
        return kw


@DEPTHER.register_module(name='DepthDDP')
class DDP(nn.Module, _SamplerMixin):
    task = 'depth'

    def __init__(self, bit_scale=1, bits=8, timesteps=1, randsteps=1, time_difference=1, learned_sinusoidal_dim=16,
                 sample_range=(0, 0.999), ddim=True, rule=None, min_depth=1e-3, max_depth=80, backbone=None,
                 neck=None, decode_head=None, train_cfg=None, test_cfg=None, pretrained=None, init_cfg=None, noise_seed=None):
        """``noise_seed`` (not a reference kwarg): None - torch.randn per call; an integer - the start noise is generated on the
        device (DDP_FLAG_SEEDED_NOISE) from (noise_seed, image index, call)."""
        super().__init__()
        self.noise_seed = noise_seed
        if not ddim:
            raise NotImplementedError('the reference references ddpm_step but never defines it (depther/ddp.py:244)')
        if learned_sinusoidal_dim != 16:
            raise ValueError('libddp_mi355x is built for learned_sinusoidal_dim=16')
        self.backbone = build_backbone(backbone) if backbone is not None else None
        self.neck = _build_neck(neck)
        if isinstance(decode_head, dict) and decode_head.get('type') == 'DeformableHeadWithTime':
            decode_head = dict(decode_head, type='DepthDeformableHeadWithTime')
        self.decode_head = build_head(decode_head)
        self.align_corners = self.decode_head.align_corners
        self.bit_scale, self.BITS, self.timesteps, self.randsteps = bit_scale, bits, timesteps, randsteps
        self.time_difference, self.sample_range, self.ddim = time_difference, sample_range, ddim
        self.min_depth, self.max_depth = min_depth, max_depth
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        c = self.decode_head.in_channels[0]
        self.down = _Conv1x1(c + 1, c)
        self.time_mlp = nn.Sequential(LearnedSinusoidalPosEmb(learned_sinusoidal_dim),
                                      nn.Linear(learned_sinusoidal_dim + 1, c * 4), nn.GELU(), nn.Linear(c * 4, c * 4))

    def extract_feat(self, img):
        x = self.backbone(img)
        if self.neck is not None:
            x = self.neck(x)
        return x

    def hot_path_state_dict(self):
        return {k: v for k, v in self.state_dict().items() if not k.startswith(('backbone.', 'neck.'))}

    def _get_sampling_timesteps(self, batch, *, device):
        return [torch.tensor([a, b], device=device)[:, None].repeat(1, batch)
                for a, b in schedule.get_sampling_timesteps(self.timesteps, self.time_difference, 0.0)]

    @torch.no_grad()
    def sample(self, x, img_metas=None, noise=None, return_steps=False, image_base=0, call=0, hints=None, prior=None, t_start=None):
        """``prior`` (b,Hp,Wp) float32 metric depth in the frame of the network input with ``t_start`` in (0, 1] (call-time only;
        DDP_FLAG_PRIOR_START): the chain starts from the prior depth (the previous frame, the coarse scale; 0, negative, NaN or inf:
        the middle of the range) noised to ``t_start`` instead of from pure noise, and the K steps divide [0, t_start]; resampled to
        (h,w) with nearest.  ``t_start`` alone: the same time grid on the given / drawn ``noise`` as the start map.
        ``hints`` (b,Hh,Wh) float32 metric depth in the frame of the network input (call-time only; DDP_FLAG_X0_HINTS) - sparse
        LiDAR depth turns prediction into completion: a finite value > 0 replaces ``depth_pred`` in the x0 normalisation of every
        step (depther/ddp.py:240-241, clamped like a prediction); 0, negative, NaN or inf leaves the pixel free.  Resampled to (h,w)
        with NEAREST (the rule of segmentors/ddp.py:149; bilinear would average the holes of a sparse map into their neighbours).
        The depth returned (and ``return_steps``' record) stays the model's own prediction; ``timesteps=1``: no effect.
        With ``self.noise_seed`` set and no ``noise``: image i of the batch gets the noise of (noise_seed, image_base + i, call).
        ``return_steps``: -> (out, record (K,b,r,h,w) float32 - every step's ``depth_pred`` (depther/ddp.py:239) -, disagreement
        (b,h,w) - their standard deviation per pixel)."""
        if not x.is_cuda:
            raise RuntimeError('ddp_amd has no CPU path: features must live on an MI355X (HIP) device')
        b, c, h, w = x.shape
        self._check_t_start(prior, t_start)
        ts = 1.0 if t_start is None else float(t_start)
        seeded = noise is None and self.noise_seed is not None
        if noise is None and not seeded:
            noise = torch.randn((b, self.randsteps, 1, h, w), device=x.device)

        head = self.decode_head
        su, ue = bool(getattr(head, 'scale_up', False)), bool(getattr(head, 'use_eps', True))
        # two depth ranges: the depther's normalises x0 (depther/ddp.py:240-241); the head's gives the regression head its eps and
        # the binned head its bins (decode_head.py:239-241,258-266).  A head built without max_depth: the depther's stands in (its
        # eps reads max_depth only with scale_up, where the reference would fail on None)
        hmin = getattr(head, 'min_depth', self.min_depth)
        hmax = getattr(head, 'max_depth', None)
        hmin = self.min_depth if hmin is None else hmin
        hmax = self.max_depth if hmax is None else hmax
        classify = bool(getattr(head, 'classify', False))
        bins = head.depth_bins() if classify else None
        norm = head.norm_strategy if classify else 'linear'

        def factory():
            from ..engine import DDPEngine
            return DDPEngine(self.hot_path_state_dict(), 'depth', h=h, w=w, batch=b, randsteps=self.randsteps,
                             timesteps=self.timesteps, bit_scale=self.bit_scale, time_difference=self.time_difference,
                             min_depth=self.min_depth, max_depth=self.max_depth, depth_scale_up=su, depth_use_eps=ue,
                             head_min_depth=hmin, head_max_depth=hmax, depth_bins=bins, depth_norm=norm, device=x.device,
                             record_steps=return_steps, seeded_noise=seeded, x0_hints=hints is not None,
                             prior_start=prior is not None, t_start=ts)
        # keyed without the geometry: a new (b, h, w) re-uses the engine through set_geometry (no weight repacking)
        bins_key = None if bins is None else (getattr(head, 'bins_strategy', None), head.n_bins, norm)
        eng = self._get_engine(('depth', str(x.device), self.timesteps, self.randsteps, self.bit_scale, self.time_difference,
                                self.min_depth, self.max_depth, su, ue, hmin, hmax, bins_key, bool(return_steps), seeded,
                                hints is not None, prior is not None, ts), factory, geometry=(b, h, w))
        # (resampled behind the engine, as ever: what is wrong with the engine is said first)
        _, maps = self._conditioning(b, h, w, x.device, torch.float32, hints=hints, prior=prior, t_start=t_start)
        return self._run(eng, maps, x, noise, None, return_steps, image_base, call)

    def _decode_head_forward_test(self, x, t, img_metas=None):
        return self.decode_head.forward_test(x, t, img_metas, self.test_cfg)

    # -- the toolbox's test entry (depth/depth/models/depther/base.py:50-115, encoder_decoder.py:130-235) ----------------
    @property
    def with_neck(self):
        return self.neck is not None

    @property
    def with_decode_head(self):
        return self.decode_head is not None

    @property
    def with_auxiliary_head(self):
        return False                     # training-only deep supervision: out of scope

    def _check_mode(self):
        """encoder_decoder.py:183-187: ``test_cfg.mode`` in ('slide', 'whole'); 'slide' is NotImplementedError there too."""
        cfg = self.test_cfg
        mode = (cfg.get('mode') if isinstance(cfg, dict) else getattr(cfg, 'mode', None)) if cfg is not None else None
        if mode not in (None, 'whole', 'slide'):
            raise AssertionError(f"test_cfg.mode must be 'slide' or 'whole', got {mode!r}")
        if mode == 'slide':
            raise NotImplementedError("test_cfg.mode='slide' (the reference raises here as well: encoder_decoder.py:186-187)")

    def _low_res(self, img, img_metas, image_base=0, call=0, hints=None, prior=None, t_start=None):
        """backbone + neck + the K-step loop: the (b,1,h/4,w/4) map every epilogue below starts from."""
        return self.sample(self.extract_feat(img)[0], img_metas, **self._given(image_base, call, hints=hints, prior=prior, t_start=t_start))

    def _post(self, maps, flips, size):
        from ..engine import depth_postprocess
        # torch.clamp(out, min=head.min_depth, max=head.max_depth) (depther/ddp.py:101): a head built without max_depth does not
        # clamp from above
        lo = self.decode_head.min_depth if self.decode_head.min_depth is not None else float('-inf')
        hi = self.decode_head.max_depth if self.decode_head.max_depth is not None else float('inf')
        return depth_postprocess(maps, flips, size, lo, hi, self.align_corners)

    def encode_decode(self, img, img_metas=None, rescale=False, image_base=0, call=0):
        """depther/ddp.py:95-109: clamp to the head's depth range, resize to the network input when ``rescale`` - one fused
        kernel (``ddp_depth_postprocess``), no intermediate (b,1,h,w) clamp result."""
        d = self._low_res(img, img_metas, **self._given(image_base, call))
        return self._post([d], [None], img.shape[2:] if rescale else d.shape[2:])

    def whole_inference(self, img, img_meta, rescale, image_base=0, call=0):
        """encoder_decoder.py:160-166."""
        return self.encode_decode(img, img_meta, rescale, **self._given(image_base, call))

    @staticmethod
    def _flip_of(img_meta):
        if img_meta and img_meta[0].get('flip', False):
            direction = img_meta[0].get('flip_direction', 'horizontal')
            assert direction in ('horizontal', 'vertical')
            return direction
        return None

    def inference(self, img, img_meta, rescale, image_base=0, call=0, hints=None, prior=None, t_start=None):
        """``hints``, ``prior``, ``t_start``: see ``sample``.
        encoder_decoder.py:168-196 (mode 'whole'): ``whole_inference`` with the test-time flip undone, the flip folded into
        the same kernel (it reads the mirrored source pixel)."""
        self._check_mode()
        if img_meta:
            ori_shape = img_meta[0]['ori_shape']
            assert all(m['ori_shape'] == ori_shape for m in img_meta)
        d = self._low_res(img, img_meta, **self._given(image_base, call, hints=hints, prior=prior, t_start=t_start))
        return self._post([d], [self._flip_of(img_meta)], img.shape[2:] if rescale else d.shape[2:])

    def simple_test(self, img, img_meta, rescale=True, image_base=0, hints=None, prior=None, t_start=None, on_device=False):
        """``on_device=True``: return the list of float32 (1,H,W) DEVICE tensors the epilogue wrote instead of host arrays
        (``ddp_amd.apis.single_gpu_test(device_eval=True)``, ``ddp_amd.evaluation.depth_pre_eval``).
        encoder_decoder.py:198-209: list (batch) of (1,H,W) float32 arrays.  ``img`` may hold b >= 1 images (independent
        noise per image; the reference's sampler is b = 1 only, depther/ddp.py:232).  ``hints`` (b,Hh,Wh) float32, ``prior`` (b,Hp,Wp)
        float32 with ``t_start``: see ``sample``."""
        out = self.inference(img, img_meta, rescale, **self._given(image_base, 0, hints=hints, prior=prior, t_start=t_start))
        return list(out) if on_device else list(out.cpu().numpy())

    def aug_test(self, imgs, img_metas, rescale=True, image_base=0, hints=None, prior=None, t_start=None, on_device=False):
        """``on_device``: see ``simple_test``.
        ``hints``, ``prior`` and ``t_start`` are not built for test-time augmentation (ValueError).
        encoder_decoder.py:210-229: mean over the augmentations (KITTI / NYU test pipelines: plain + horizontal flip,
        depth/configs/_base_/datasets/kitti.py:30-33).  Every augmentation runs the full sampling loop with its own noise; only the
        LOW-RESOLUTION maps are kept and ONE kernel does clamp -> resize -> flip-undo -> running sum -> / n per output pixel."""
        self._refuse_frame_bound('aug_test', hints, prior, t_start)
        assert rescale, 'aug_test rescales every augmentation back to the network input'
        self._check_mode()
        sizes = {tuple(img.shape[2:]) for img in imgs}
        if len(sizes) != 1:
            # the reference adds the per-augmentation maps in place (:222-224): they must have one size
            raise RuntimeError(f'aug_test: augmentations of different input sizes {sorted(sizes)} cannot be averaged')
        maps, flips = [], []
        for a, (img, meta) in enumerate(zip(imgs, img_metas)):
            if meta:
                ori_shape = meta[0]['ori_shape']
                assert all(m['ori_shape'] == ori_shape for m in meta)
            maps.append(self._low_res(img, meta, **self._given(image_base, a)))      # (seeded noise: the augmentation index is the `call`)
            flips.append(self._flip_of(meta))
        out = self._post(maps, flips, imgs[0].shape[2:])
        return list(out) if on_device else list(out.cpu().numpy())

    def forward_test(self, imgs, img_metas, **kwargs):
        """base.py:62-92: the outer lists are the test-time augmentations."""
        for var, name in [(imgs, 'imgs'), (img_metas, 'img_metas')]:
            if not isinstance(var, list):
                raise TypeError(f'{name} must be a list, but got {type(var)}')
        if len(imgs) != len(img_metas):
            raise ValueError(f'num of augmentations ({len(imgs)}) != num of image meta ({len(img_metas)})')
        for img_meta in img_metas:
            for key in ('ori_shape', 'img_shape', 'pad_shape'):
                vals = [m[key] for m in img_meta if key in m]
                assert all(v == vals[0] for v in vals), f'{key} differs inside one augmentation batch'
        if len(imgs) == 1:
            return self.simple_test(imgs[0], img_metas[0], **kwargs)
        return self.aug_test(imgs, img_metas, **kwargs)

    def forward(self, img, img_metas, return_loss=True, **kwargs):
        """base.py:94-108; what the harness calls: ``model(return_loss=False, **data)`` (depth/depth/apis/test.py:88,204)."""
        if return_loss:
            return self.forward_train(img, img_metas, **kwargs)
        return self.forward_test(img, img_metas, **kwargs)

    def forward_dummy(self, img):
        """encoder_decoder.py:124-128."""
        return self.encode_decode(img, None)

    def val_step(self, data_batch, **kwargs):
        """base.py:150-158."""
        return self(**data_batch, **kwargs)

    def forward_train(self, *a, **k):
        raise NotImplementedError('training is out of scope of ddp_amd (SURVEY.md §8)')

    def train_step(self, *a, **k):
        raise NotImplementedError('training is out of scope of ddp_amd (SURVEY.md §8)')
