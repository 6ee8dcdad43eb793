"""Drop-in BEV map-segmentation sampler (bev/mmdet3d/models/fusion_models/ddp.py:65-114,268-301) and
head (bev/mmdet3d/models/heads/segm/deformable_head_with_time.py:57-235).  The reference class
derives from BEVFusion (sensor encoders, out of scope); this one keeps only the diffusion members and
``ddim_sample(x: list[Tensor], head)``."""
import math

import torch
import torch.nn as nn

from ..decode_heads.deformable_head_with_time import DeformableHeadWithTime as _SegHead
from ..registry import FUSIONMODELS, HEADS
from ..segmentors.ddp import LearnedSinusoidalPosEmb, _Conv1x1, _SamplerMixin
from .. import schedule


@HEADS.register_module(name='BEVDeformableHeadWithTime')
class BEVDeformableHeadWithTime(_SegHead):
    """runs BEVGridTransform before the encoder and returns sigmoid maps (reference :179-235)."""
    task = 'bev'

    def __init__(self, num_feature_levels=1, encoder=None, positional_encoding=None, classes=(), loss='focal',
                 grid_transform=None, in_channels=256, seg_conv_kernel=1, **kwargs):
        if seg_conv_kernel not in (1, 3):
            # (the reference builds a 3x3 conv_seg for ANY value other than 1, reference :136-139; only 1 and 3 are accepted here)
            raise ValueError(f'seg_conv_kernel must be 1 or 3, got {seg_conv_kernel!r}')
        self.classes = list(classes)
        self.loss = loss
        self.grid_transform = dict(grid_transform or {})
        self.seg_conv_kernel = seg_conv_kernel
        p = float(self.grid_transform.get('prescale_factor', 1))
        if not (p > 0 and math.isfinite(p)):
            raise ValueError(f'prescale_factor must be a positive float, got {p!r}')
        self.prescale_factor = p
        super().__init__(num_feature_levels=num_feature_levels, encoder=encoder,
                         positional_encoding=positional_encoding, in_channels=[in_channels], channels=in_channels,
                         num_classes=len(self.classes), **kwargs)

    def _make_head_conv(self):
        # (reference :136-139; with 3 the parameter holder of a (K,256,3,3) checkpoint tensor)
        k = self.seg_conv_kernel
        self.conv_seg = nn.Conv2d(self.channels, self.num_classes, kernel_size=k, padding=k // 2)

    def _engine_kwargs(self):
        return dict(num_classes=self.num_classes, bev_input_scope=self.grid_transform['input_scope'],
                    bev_output_scope=self.grid_transform['output_scope'], bev_prescale=self.prescale_factor,
                    bev_seg_kernel=self.seg_conv_kernel)

    def forward(self, inputs, times, target=None):
        return super().forward(inputs, times)


@FUSIONMODELS.register_module(name='BEVDDP')
class DDP(nn.Module, _SamplerMixin):
    task = 'bev'

    def __init__(self, bit_scale=1, timesteps=1, randsteps=1, time_difference=1, learned_sinusoidal_dim=16,
                 sample_range=(0, 0.999), noise_schedule='cosine', diffusion='ddim', threshold=0.5,
                 feat_channels=512, tmp_channels=256, noise_seed=None, **kwargs):
        """``noise_seed`` (not a reference kwarg): None - torch.randn per call; an integer - the start noise is generated on the
        device (DDP_FLAG_SEEDED_NOISE) from (noise_seed, image index, call)."""
        super().__init__()
        self.noise_seed = noise_seed
        if noise_schedule not in schedule.NOISE_SCHEDULES:
            raise ValueError(f'invalid noise schedule {noise_schedule}')
        if tmp_channels != 256:
            raise ValueError('libddp_mi355x is built for tmp_channels=256')
        if learned_sinusoidal_dim != 16:
            raise ValueError('libddp_mi355x is built for learned_sinusoidal_dim=16')
        self.bit_scale, self.timesteps, self.randsteps = bit_scale, timesteps, randsteps
        self.diffusion, self.time_difference, self.sample_range = diffusion, time_difference, sample_range
        self.noise_schedule = noise_schedule
        self.num_classes = 6
        self.threshold = threshold
        self.feat_channels = feat_channels
        self.embedding_table = nn.Embedding(self.num_classes + 1, tmp_channels)
        self.transform = _Conv1x1(tmp_channels + feat_channels, tmp_channels)
        self.time_mlp = nn.Sequential(LearnedSinusoidalPosEmb(learned_sinusoidal_dim),
                                      nn.Linear(learned_sinusoidal_dim + 1, tmp_channels * 4), nn.GELU(),
                                      nn.Linear(tmp_channels * 4, tmp_channels * 4))

    @torch.no_grad()
    def ddim_sample(self, x, head, noise=None, return_steps=False, image_base=0, call=0, hints=None, prior=None, t_start=None):
        """``prior`` (b,Hp,Wp) int32 bit words (bit c = class c present) with ``t_start`` in (0, 1] (call-time only;
        DDP_FLAG_PRIOR_START): the chain starts from the prior map noised to ``t_start`` instead of from pure noise, and the K steps
        divide [0, t_start]; brought to (h,w) with nearest resampling.  ``t_start`` alone: the same time grid on the given / drawn
        ``noise`` as the start map.
        ``hints``: not built for the bev sampler (ValueError; DDP_FLAG_X0_HINTS is a seg / depth flag).
        With ``self.noise_seed`` set and no ``noise``: image i of the batch gets the noise of (noise_seed, image_base + i, call).
        ``return_steps``: -> (out, record (K,b,r,head_h,head_w) int32 bit words - bit c = the step's prob_c > threshold
        (fusion_models/ddp.py:290) -, disagreement (b,head_h,head_w) - the fraction of recorded bits that differ from
        out > threshold)."""
        if hints is not None:
            raise ValueError('hints are not built for the bev sampler (DDP_FLAG_X0_HINTS exists for seg and depth)')
        x0 = x[0]
        if not x0.is_cuda:
            raise RuntimeError('ddp_amd has no CPU path: features must live on an MI355X (HIP) device')
        b, c, h, w = x0.shape
        self._check_t_start(prior, t_start)
        ts = 1.0 if t_start is None else float(t_start)
        seeded = noise is None and self.noise_seed is not None
        if noise is None and not seeded:
            noise = torch.randn((b, self.randsteps, 256, h, w), device=x0.device)
        sd = dict(self.state_dict())
        sd.update({'decode_head.' + k: v for k, v in head.state_dict().items()})

        def factory():
            from ..engine import DDPEngine
            return DDPEngine(sd, 'bev', h=h, w=w, batch=b, randsteps=self.randsteps, timesteps=self.timesteps,
                             num_classes=self.num_classes, feat_channels=c, bit_scale=self.bit_scale,
                             time_difference=self.time_difference, noise_schedule=self.noise_schedule,
                             threshold=self.threshold, bev_input_scope=head.grid_transform['input_scope'],
                             bev_output_scope=head.grid_transform['output_scope'],
                             bev_prescale=getattr(head, 'prescale_factor', 1.0),
                             bev_seg_kernel=getattr(head, 'seg_conv_kernel', 1), device=x0.device,
                             record_steps=return_steps, seeded_noise=seeded, prior_start=prior is not None, t_start=ts)
        ver = sum(p._version for p in head.parameters())
        # everything of the head that shapes the engine: its identity, grid transform (scopes, prescale) and conv_seg kernel
        gt = head.grid_transform
        hkey = (id(head), repr(gt['input_scope']), repr(gt['output_scope']), getattr(head, 'prescale_factor', 1.0),
                getattr(head, 'seg_conv_kernel', 1), bool(return_steps), seeded, prior is not None, ts)
        eng = self._get_engine((b, c, h, w, str(x0.device), self.timesteps, self.randsteps, ver) + hkey, factory)
        # (resampled behind the engine, as ever: what is wrong with the engine is said first)
        _, maps = self._conditioning(b, h, w, x0.device, torch.int32, prior=prior, t_start=t_start)
        return self._run(eng, maps, x0, noise, None, return_steps, image_base, call)
