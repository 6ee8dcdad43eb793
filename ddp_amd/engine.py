"""DDPEngine: owns the device-side state of one configured sampling problem and calls the C ABI.

PyTorch is plumbing here: it allocates device memory (weights blob, workspace, inputs/outputs) and
provides the current HIP stream; every FLOP of the loop runs in libddp_mi355x.so.
"""
import ctypes as C
from collections import namedtuple

import torch

from . import _lib
from . import schedule

DEPTH_NORMS = {'linear': _lib.DEPTH_NORM_LINEAR, 'softmax': _lib.DEPTH_NORM_SOFTMAX, 'sigmoid': _lib.DEPTH_NORM_SIGMOID}
TASKS = {'seg': _lib.TASK_SEG, 'depth': _lib.TASK_DEPTH, 'bev': _lib.TASK_BEV}
SAMPLERS = {'ddim': _lib.SAMPLER_DDIM, 'ddpm': _lib.SAMPLER_DDPM}
GEMM_MODES = {'f32': _lib.GEMM_F32_MFMA, 'bf16x3': _lib.GEMM_BF16X3}


def default_gemm_mode():
    """'bf16x3' (fp32-accurate 3-way bf16 split on the bf16 matrix cores) unless DDP_GEMM_MODE=f32 selects the
    exact f32-input MFMA path."""
    import os
    return os.environ.get('DDP_GEMM_MODE', 'bf16x3')

_LAYER_KEYS = {
    'sampling_offsets_w': 'attentions.0.sampling_offsets.weight', 'sampling_offsets_b': 'attentions.0.sampling_offsets.bias',
    'attention_weights_w': 'attentions.0.attention_weights.weight', 'attention_weights_b': 'attentions.0.attention_weights.bias',
    'value_proj_w': 'attentions.0.value_proj.weight', 'value_proj_b': 'attentions.0.value_proj.bias',
    'output_proj_w': 'attentions.0.output_proj.weight', 'output_proj_b': 'attentions.0.output_proj.bias',
    'ffn0_w': 'ffns.0.layers.0.0.weight', 'ffn0_b': 'ffns.0.layers.0.0.bias',
    'ffn1_w': 'ffns.0.layers.1.weight', 'ffn1_b': 'ffns.0.layers.1.bias',
    'norm0_w': 'norms.0.weight', 'norm0_b': 'norms.0.bias', 'norm1_w': 'norms.1.weight', 'norm1_b': 'norms.1.bias',
    'time_w': 'time_mlp.1.weight', 'time_b': 'time_mlp.1.bias',
}


def check_bev_head(prescale, seg_kernel, h, w):
    """(bev_prescale, bev_seg_kernel) of ``ddp_cfg`` from the head's grid_transform['prescale_factor'] and seg_conv_kernel.
    The reference builds a 3x3 conv_seg for ANY seg_conv_kernel other than 1 (heads/segm/deformable_head_with_time.py:136-139);
    here only 1 and 3 are accepted.
    The ABI field is a FLOAT and the library sizes the prescaled map as floor(h * double(float p)); F.interpolate uses the Python
    double.  For a factor float cannot hold (0.9 on a 10-wide map: 8 against 9) the returned value is the float next to
    float32(p) that gives the double's sizes on both axes; if neither neighbour does, the factor is refused."""
    import math
    import numpy as np
    if seg_kernel not in (1, 3):
        raise ValueError(f'seg_conv_kernel must be 1 or 3, got {seg_kernel!r}')
    p = float(prescale)
    if not (p > 0 and math.isfinite(p)):
        raise ValueError(f'prescale_factor must be a positive float, got {prescale!r}')
    want = (math.floor(h * p), math.floor(w * p))
    if min(want) < 1:
        raise ValueError(f'prescale_factor {p}: the prescaled {h} x {w} map is empty')
    p32 = np.float32(p)
    for cand in (p32, np.nextafter(p32, np.float32(np.inf)), np.nextafter(p32, np.float32(0))):
        if (math.floor(h * float(cand)), math.floor(w * float(cand))) == want:
            return float(cand), int(seg_kernel)
    raise ValueError(f'prescale_factor {p}: no float32 next to it gives the {want[0]} x {want[1]} prescaled map of the reference')


def hot_path_keys(task, num_layers, head_prefix='decode_head.'):
    """(struct field, state_dict key) pairs of the hot path (SURVEY.md §8b checkpoint layout)."""
    conv = 'down.conv' if task == 'depth' else 'transform.conv'
    top = [('transform_w', conv + '.weight'), ('transform_b', conv + '.bias'),
           ('time_freq', 'time_mlp.0.weights'), ('time1_w', 'time_mlp.1.weight'), ('time1_b', 'time_mlp.1.bias'),
           ('time3_w', 'time_mlp.3.weight'), ('time3_b', 'time_mlp.3.bias')]
    if task != 'depth':
        top.append(('embedding', 'embedding_table.weight'))
    hc = 'conv_depth' if task == 'depth' else 'conv_seg'
    top += [('head_w', head_prefix + hc + '.weight'), ('head_b', head_prefix + hc + '.bias')]
    layers = []
    for l in range(num_layers):
        p = f'{head_prefix}encoder.layers.{l}.'
        layers.append([(f, p + k) for f, k in _LAYER_KEYS.items()])
    return top, layers


def count_layers(state_dict, head_prefix='decode_head.'):
    n = 0
    while f'{head_prefix}encoder.layers.{n}.norms.0.weight' in state_dict:
        n += 1
    return n


class PackedWeights:
    """All hot-path parameters in ONE flat fp32 device buffer (256-byte aligned sub-tensors): a
    single allocation, a single RCCL broadcast, and stable pointers for the ``ddp_weights`` table."""

    def __init__(self, state_dict, task, num_layers, device, head_prefix='decode_head.', depth_bins=None):
        """``depth_bins``: (n_bins) bin centres of a binned depth head (``classify=True``), stored after the parameters."""
        top, layers = hot_path_keys(task, num_layers, head_prefix)
        if depth_bins is not None:
            if task != 'depth':
                raise ValueError('depth_bins belong to a depth head')
            state_dict = dict(state_dict, **{'<depth_bins>': torch.as_tensor(depth_bins, dtype=torch.float32).reshape(-1)})
            top = top + [('depth_bins', '<depth_bins>')]
        entries = []
        for f, k in top:
            entries.append((None, f, k))
        for l, lk in enumerate(layers):
            for f, k in lk:
                entries.append((l, f, k))
        offs, total, numel = {}, 0, {}
        for l, f, k in entries:
            if k not in state_dict:
                if f in ('time_w', 'time_b'):     # layer built without use_time_mlp
                    continue
                raise KeyError(f'hot-path parameter {k!r} missing from state_dict')
            n = state_dict[k].numel()
            offs[(l, f)] = (total, k)
            numel[(l, f)] = n
            total += (n + 63) // 64 * 64
        flat = torch.zeros(total, dtype=torch.float32, device=device)
        for (l, f), (o, k) in offs.items():
            flat[o:o + state_dict[k].numel()].copy_(state_dict[k].detach().reshape(-1))
        self.flat = flat
        self.offsets = offs
        self.numel = numel
        self.task = task
        self.num_layers = num_layers
        self.n_bins = state_dict['<depth_bins>'].numel() if depth_bins is not None else 0
        self.struct = self._build_struct()

    def _build_struct(self):
        w = _lib.DdpWeights()
        base = self.flat.data_ptr()
        for (l, f), (o, _) in self.offsets.items():
            tgt = w if l is None else w.layers[l]
            setattr(tgt, f, base + 4 * o)
        return w

    def broadcast(self, src=0, force=False):
        """Replicate the frozen weights from rank ``src`` to every rank (RCCL over xGMI; the only
        collective of the inference path - SURVEY.md §8e).  ``force``: run the collective at world size 1 too."""
        from .parallel import broadcast_weights
        broadcast_weights(self.flat, src=src, force=force)


def noise_key_words(seed, image_base=0, stream_base=0, call=0):
    """The 8 uint32 words of the device key of DDP_FLAG_SEEDED_NOISE (include/ddp_mi355x.h):
    {seed_lo, seed_hi, image_base, stream_base, call, 0, 0, 0}; ``seed`` is taken modulo 2^64, the others modulo 2^32."""
    seed = int(seed)
    m = 0xFFFFFFFF
    return [seed & m, (seed >> 32) & m, int(image_base) & m, int(stream_base) & m, int(call) & m, 0, 0, 0]


class _SeededNoise:
    """What DDPEngine and FcnSamplerEngine share for ``seeded_noise=True``: the 8-word device key tensor, the argument checks of
    ``sample()`` and the view of the start-noise buffer; and ``_region()``, the view of any buffer of ``caller_regions``
    (``_workspace_bytes()`` is the engine's own workspace query)."""

    def _region(self, name, dtype, shape):
        off, nbytes = caller_regions(self.cfg, self._workspace_bytes())[name]
        v = self.workspace.view(torch.uint8)[off:off + nbytes]
        return (v if dtype == torch.uint8 else v.view(dtype)).view(shape)

    def _init_key(self):
        self.seeded = bool(self.cfg.flags & _lib.FLAG_SEEDED_NOISE)
        self._key_words = None
        self._key = torch.zeros(8, dtype=torch.int32, device=self.device) if self.seeded else None

    def _write_key(self, seed=None, image_base=None, stream_base=None, call=None):
        """update the given words of the key (the others keep their value) and copy it to the device on the current stream"""
        import numpy as np
        old = self._key_words
        if old is None:
            if seed is None:
                raise _lib.DdpError('seeded_noise engine: sample() / capture() need seed=')
            old = noise_key_words(0)
        new = noise_key_words(seed if seed is not None else old[0] | (old[1] << 32),
                              old[2] if image_base is None else image_base, old[3] if stream_base is None else stream_base,
                              old[4] if call is None else call)
        self._key_words = new
        host = torch.from_numpy(np.array(new, dtype=np.uint32).view(np.int32))
        with torch.cuda.device(self.device):
            self._key.copy_(host)

    def _noise_args(self, noise, step_noise, seed):
        """-> True when the call is a seeded one; refuses the combinations that make no sense"""
        if self.seeded:
            if noise is not None or step_noise is not None:
                raise _lib.DdpError('seeded_noise engine: the noise is generated on the device - pass seed=, not noise= / step_noise=')
            return True
        if seed is not None:
            raise _lib.DdpError('seed= needs an engine built with seeded_noise=True')
        if noise is None:
            raise _lib.DdpError('sample() needs noise= (or an engine built with seeded_noise=True and seed=)')
        return False

    def last_noise(self):
        """(B, r, Cm, h, w) float32 VIEW of the workspace buffer that holds the start noise the LAST seeded sample() call (or
        graph replay) generated; valid until the next call."""
        if not self.seeded:
            raise _lib.DdpError('last_noise() needs an engine built with seeded_noise=True')
        if self.cfg.flags & _lib.FLAG_PRIOR_START:
            raise _lib.DdpError('prior_start engine: the seeded-noise buffer is mixed in place and holds the start map after the '
                                'call - use last_start() instead')
        if not getattr(self, '_sampled', False):
            raise _lib.DdpError('no noise yet: call sample() first')
        c = self.cfg
        return self._region('seed_noise', torch.float32, (c.batch, c.randsteps, 1 if c.task == _lib.TASK_DEPTH else 256, c.h, c.w))


class DDPEngine(_SeededNoise):
    """One configured problem: (task, sizes, schedule) + weights + workspace."""

    def __init__(self, state_dict, task='seg', *, h, w, batch=1, randsteps=1, timesteps=3, num_classes=150,
                 feat_channels=256, bit_scale=0.01, time_difference=1, sample_range0=0.0, noise_schedule='cosine',
                 sampler='ddim', accumulation=False, min_depth=1e-3, max_depth=80.0, threshold=0.5,
                 head_hw=None, bev_input_scope=None, bev_output_scope=None, device=None, head_prefix='decode_head.',
                 weights=None, gemm=None, fused_layer=None, fused_prologue=None, lib_path=None, record_x0=False,
                 gather_guess_zero=False, force_x0=False, fused_tail=None, nchw_head=None, depth_scale_up=False,
                 depth_use_eps=True, depth_bins=None, depth_norm='linear', head_min_depth=None, head_max_depth=None,
                 bev_prescale=1.0, bev_seg_kernel=1, record_steps=False, seeded_noise=False, ddpm_chain=None, x0_hints=False,
                 prior_start=False, t_start=1.0, class_prior=False, score_prior=False):
        """``score_prior`` (DDP_FLAG_SCORE_PRIOR; seg): a per-pixel additive prior on the conv_seg scores, in front of everything that
        reads them at every step - ``set_score_prior()`` / ``score_prior_view()`` / ``clear_score_prior()``,
        ``SampleGraph.replay(score_prior=)``.  (B, num_classes, h, w) float32, NCHW; ``-inf`` excludes a class at a pixel, NaN reads
        as 0; adds to ``class_prior``.  The engine writes zeros (no prior) whenever it allocates or regrows the workspace and on every
        ``set_geometry``.
        ``class_prior`` (DDP_FLAG_CLASS_PRIOR; seg): a per-image additive prior on the conv_seg scores, in front of everything that
        reads them at every step - ``set_class_prior()`` / ``class_prior_view()`` / ``clear_class_prior()``,
        ``SampleGraph.replay(class_prior=)``.  (B, num_classes) float32; ``-inf`` excludes a class (``class_mask_to_prior``), NaN
        reads as 0.  The engine writes zeros (no prior) whenever it allocates or regrows the workspace and on every ``set_geometry``.
        ``prior_start`` (DDP_FLAG_PRIOR_START; all three tasks): the chain starts from the caller's prior map noised to ``t_start``
        instead of from pure noise - ``set_prior()`` / ``prior_view()`` / ``clear_prior()``, ``SampleGraph.replay(prior=)``,
        ``last_start()``.  seg: (B, h, w) uint8 classes, a value >= num_classes is the ignore row; depth: (B, h, w) float32 metric
        depth, 0 / negative / NaN / inf is the middle of the range; bev: (B, h, w) int32 bit words, bit c = class c present.  The
        engine clears the prior (seg 255, depth 0, bev 0) whenever it allocates the workspace and on every ``set_geometry``.
        ``t_start`` in (sample_range0, 1]: the time the K steps begin at (``schedule.get_sampling_timesteps``); independent of
        ``prior_start`` - a flag-clear engine with ``t_start < 1`` runs on whatever start map the caller passes as ``noise``.
        ``x0_hints`` (DDP_FLAG_X0_HINTS; seg and depth): where the caller knows the answer it is fed back as x0 at every step in
        place of the model's own prediction - ``set_hints()`` / ``hints_view()`` / ``clear_hints()``, ``SampleGraph.replay(hints=)``.
        seg: (B, h, w) uint8 classes, a value >= num_classes (255) leaves the pixel free; depth: (B, h, w) float32 metric depth, 0 /
        negative / NaN / inf leaves it free.  Unset hints are no hints: the engine sets everything free whenever it allocates or
        regrows the workspace and on every ``set_geometry``.  Hints act through the update, i.e. from the second step on:
        ``timesteps=1`` is accepted and they have no effect.  The output and the step record stay the model's own prediction.
        ``ddpm_chain`` (DDP_FLAG_DDPM_CHAIN; seg + sampler='ddpm' only): ddpm_sample on the fused step boundary of the ddim
        sampler, the step noise folded into u by one pre-pass per noise-adding step.  ``None`` reads the environment variable
        ``DDP_DDPM_CHAIN`` (default off; ignored for any other task or sampler); ``True`` elsewhere raises ValueError.
        ``seeded_noise`` (DDP_FLAG_SEEDED_NOISE): start noise and ddpm step noise are generated on the device from a key -
        ``sample(x, seed=...)``, ``last_noise()``; ``noise=`` / ``step_noise=`` are refused.
        ``record_steps`` (DDP_FLAG_STEP_RECORD): keep every step's prediction and compute the step-disagreement map on the
        device - ``step_record()`` / ``step_disagreement()`` after ``sample()``.
        depth: ``min_depth`` / ``max_depth`` are the depther's range (x0 normalisation); ``head_min_depth`` / ``head_max_depth``
        the decode head's (eps of the regression head; default: the depther's).  ``depth_bins`` (n_bins) = the bin centres of a
        binned head (``classify=True``: conv_depth has n_bins outputs, ``depth_norm`` in 'linear' / 'softmax' / 'sigmoid'); with
        ``weights`` given, the bins are the ones packed there.
        bev: ``bev_prescale`` = grid_transform['prescale_factor'] of the head, ``bev_seg_kernel`` = its seg_conv_kernel (1 or 3; with
        3 the state dict's conv_seg.weight is (K,256,3,3))."""
        self.lib = _lib.load(lib_path)
        if not torch.cuda.is_available():
            raise _lib.DdpError('no HIP device visible: ddp_amd has no CPU path')
        self.device = torch.device(device if device is not None else f'cuda:{torch.cuda.current_device()}')
        self.task = task
        num_layers = count_layers(state_dict, head_prefix) if weights is None else weights.num_layers
        if num_layers > _lib.MAX_LAYERS:     # (the weights table has DDP_MAX_LAYERS slots: refuse before packing, as validate() would)
            raise _lib.DdpError(f'num_layers {num_layers} out of range: the library supports at most {_lib.MAX_LAYERS} encoder layers')
        self.weights = weights if weights is not None else PackedWeights(state_dict, task, num_layers, self.device,
                                                                        head_prefix, depth_bins=depth_bins)
        if depth_norm not in DEPTH_NORMS:
            raise ValueError(f'depth_norm must be one of {sorted(DEPTH_NORMS)}, got {depth_norm!r}')
        cfg = _lib.DdpCfg()
        cfg.abi_version = _lib.ABI_VERSION
        cfg.task = TASKS[task]
        cfg.sampler = SAMPLERS[sampler]
        cfg.batch, cfg.randsteps, cfg.timesteps, cfg.num_layers = batch, randsteps, timesteps, num_layers
        cfg.num_classes = 1 if task == 'depth' else num_classes
        cfg.feat_channels = feat_channels
        cfg.h, cfg.w = h, w
        if task == 'bev':
            if bev_input_scope is None or bev_output_scope is None:
                raise ValueError('bev needs bev_input_scope / bev_output_scope (grid_transform of the head)')
            out_sizes = []
            for a, ((imin, imax, _), (omin, omax, ostep)) in enumerate(zip(bev_input_scope, bev_output_scope)):
                n = int(torch.arange(omin + ostep / 2, omax, ostep).numel())
                out_sizes.append(n)
                cfg.bev_in_min[a], cfg.bev_in_max[a] = imin, imax
                cfg.bev_out_first[a], cfg.bev_out_step[a] = omin + ostep / 2, ostep
            cfg.head_h, cfg.head_w = out_sizes
            # (the defaults stay zeroed fields: an ABI-6 configuration is the same bytes as before)
            p, k = check_bev_head(bev_prescale, bev_seg_kernel, h, w)
            cfg.bev_prescale, cfg.bev_seg_kernel = (p if p != 1.0 else 0.0), (k if k != 1 else 0)
            n_head = self.weights.numel[(None, 'head_w')]      # (a packed 1x1 tensor read as a 3x3 one would be read 9x past its end)
            if n_head != num_classes * 256 * (9 if cfg.bev_seg_kernel == 3 else 1):
                raise ValueError(f'conv_seg.weight has {n_head} elements: not a {k}x{k} '
                                 f'convolution from 256 channels to {num_classes} classes')
        elif bev_prescale != 1.0 or bev_seg_kernel != 1:
            raise ValueError('bev_prescale / bev_seg_kernel configure the bev head only')
        else:
            cfg.head_h, cfg.head_w = (h, w) if head_hw is None else head_hw
        self.gemm = gemm if gemm is not None else default_gemm_mode()
        cfg.gemm_mode = GEMM_MODES[self.gemm]
        # diagnostics (A/B runs, tests of the unfused kernels): DDP_LAYER_FUSED=0 / DDP_PROLOGUE_FUSED=0 or the kwargs
        import os
        if fused_layer is None:
            fused_layer = os.environ.get('DDP_LAYER_FUSED', '1') != '0'
        if fused_prologue is None:
            fused_prologue = os.environ.get('DDP_PROLOGUE_FUSED', '1') != '0'
        if fused_tail is None:     # DDP_TAIL_FUSED=0: the step boundary as the launches it was fused from (DDP_FLAG_UNFUSED_TAIL: seg - the last
                                   # layer and the tail as two kernels; depth / bev - the round-5 GEMM heads and update kernels; A/B runs, tests)
            fused_tail = os.environ.get('DDP_TAIL_FUSED', '1') != '0'
        if nchw_head is None:      # DDP_NCHW_HEAD=0: the first step's head through the SB conversions + x-projection GEMM + MODE 2
            nchw_head = os.environ.get('DDP_NCHW_HEAD', '1') != '0'
        cfg.flags = ((0 if fused_layer else _lib.FLAG_UNFUSED_LAYER) | (0 if fused_prologue else _lib.FLAG_UNFUSED_PROLOGUE) |
                     (0 if fused_tail else _lib.FLAG_UNFUSED_TAIL) | (0 if nchw_head else _lib.FLAG_SB_HEAD))
        if task == 'depth' and self.weights.n_bins:   # binned head (decode_head.py:233-250): scale_up / use_eps play no part
            cfg.depth_n_bins, cfg.depth_norm = self.weights.n_bins, DEPTH_NORMS[depth_norm]
        elif task == 'depth':      # head variants of depth_pred (decode_head.py:252-262)
            cfg.flags |= (_lib.FLAG_DEPTH_SCALE_UP if depth_scale_up else 0) | (0 if depth_use_eps else _lib.FLAG_DEPTH_NO_EPS)
        if task == 'depth':        # the head's own depth range (eps); the depther's pair below normalises x0
            cfg.head_min_depth = min_depth if head_min_depth is None else head_min_depth
            cfg.head_max_depth = max_depth if head_max_depth is None else head_max_depth
        if record_x0:
            cfg.flags |= _lib.FLAG_RECORD_X0
        if force_x0:               # test instrument (seg): teacher forcing, see set_x0_decisions()
            if task != 'seg':
                raise ValueError('force_x0 is a segmentation test instrument')
            cfg.flags |= _lib.FLAG_FORCE_X0
        if gather_guess_zero:      # diagnostic: forces the LDS gather's refill branch (identical results)
            cfg.flags |= _lib.FLAG_GATHER_GUESS_ZERO
        if record_steps:
            cfg.flags |= _lib.FLAG_STEP_RECORD
        if seeded_noise:
            cfg.flags |= _lib.FLAG_SEEDED_NOISE
        if ddpm_chain is None:     # DDP_DDPM_CHAIN=1: A/B runs of scripts that build their engines without the kwarg
            ddpm_chain = task == 'seg' and sampler == 'ddpm' and os.environ.get('DDP_DDPM_CHAIN', '0') != '0'
        if ddpm_chain:
            if task != 'seg' or sampler != 'ddpm':
                raise ValueError(f"ddpm_chain is a route of the segmentation ddpm sampler (task {task!r}, sampler {sampler!r})")
            cfg.flags |= _lib.FLAG_DDPM_CHAIN
        asked = dict(x0_hints=x0_hints, prior_start=prior_start, class_prior=class_prior, score_prior=score_prior)
        for row in reversed(CALLER_INPUTS):      # (hints first: the order these refusals have had since each was added)
            if not asked[row.kwarg]:
                continue
            if cfg.task not in row.dtypes:
                raise ValueError(f'{row.kwarg} is built for the {row.built_for} ({row.flag_name}): '
                                 + row.wrong_task.format(task=task))
            if row.name == 'hints' and force_x0:
                raise ValueError('x0_hints cannot be combined with force_x0 (DDP_FLAG_X0_HINTS / DDP_FLAG_FORCE_X0)')
            if row.name == 'prior' and task == 'bev' and num_classes > 32:
                raise ValueError('prior_start: a bev prior is one 32-bit word per pixel (DDP_FLAG_PRIOR_START, num_classes <= 32)')
            cfg.flags |= row.flag
        self.t_start = float(t_start)
        self.fused_layer = bool(fused_layer)
        cfg.accumulation = int(bool(accumulation))
        cfg.bit_scale, cfg.min_depth, cfg.max_depth, cfg.threshold = bit_scale, min_depth, max_depth, threshold
        self.cfg = cfg
        self.sampler = sampler
        recs = schedule.step_records(task, timesteps, time_difference, sample_range0, noise_schedule, sampler, t_start=self.t_start)
        self.steps = (_lib.DdpStep * timesteps)()
        for i, r in enumerate(recs):
            for k, v in r.items():
                setattr(self.steps[i], k, v)
        nbytes = C.c_size_t(0)
        _lib.check(self.lib.ddp_query_workspace(C.byref(cfg), C.byref(nbytes)), self.lib)
        self.workspace = torch.empty(nbytes.value // 4, dtype=torch.float32, device=self.device)
        cbytes = C.c_size_t(0)
        _lib.check(self.lib.ddp_query_const_workspace(C.byref(cfg), C.byref(cbytes)), self.lib)
        self._const_floats = cbytes.value // 4       # model region: a prefix of the workspace, independent of the geometry
        self._prepared = False
        self._sampled = False
        self.geometry_changes = 0
        self._init_key()
        for row in CALLER_INPUTS:
            self._clear_input(row, _if_any=True)

    def _workspace_bytes(self):
        nbytes = C.c_size_t(0)
        _lib.check(self.lib.ddp_query_workspace(C.byref(self.cfg), C.byref(nbytes)), self.lib)
        return nbytes.value

    # ---- the caller-written inputs: every method below is its row of CALLER_INPUTS ---------------
    def _input_view(self, row):
        """VIEW of the row's caller-written region inside the workspace, in the dtype of the engine's task"""
        c = self.cfg
        if not c.flags & row.flag:
            raise _lib.DdpError(f'{row.needs} an engine built with {row.kwarg}=True')
        return self._region(row.region, row.dtypes[c.task], row.shape(c))

    def _write_input(self, row, src):
        """the checks and the stream-ordered copy of every set_*: ``src`` must be a tensor of the dtype the row accepts (the view's,
        or any 'floating-point' one) with the shape of the slice the row writes, on the engine's device"""
        dst = row.dst(self._input_view(row), self.cfg)
        kind = row.accepts or dst.dtype
        ok = isinstance(src, torch.Tensor) and (src.dtype.is_floating_point if kind == 'floating-point' else src.dtype == kind)
        if not ok:
            raise _lib.DdpError(f'{row.name} must be a {kind} tensor, got {getattr(src, "dtype", type(src))}')
        if tuple(src.shape) != tuple(dst.shape):
            raise _lib.DdpError(f'{row.name} must have shape {tuple(dst.shape)} ({row.dims}), got {tuple(src.shape)}')
        if src.device != self.device:
            raise _lib.DdpError(f'engine lives on {self.device}: {row.where} on {src.device}')
        with torch.cuda.device(self.device):
            dst.copy_(src, non_blocking=True)

    def _clear_input(self, row, _if_any=False):
        """the row's "nothing given" value over the whole region; ``_if_any``: only where the engine has the region"""
        if _if_any and not self.cfg.flags & row.flag:
            return
        v = self._input_view(row)
        with torch.cuda.device(self.device):
            v.fill_(row.clear[v.dtype])

    # ---- DDP_FLAG_X0_HINTS ---------------------------------------------------------------------
    def hints_view(self):
        """(B, h, w) VIEW of the caller-written hint map inside the workspace - uint8 (seg) or float32 (depth); the kernels read it
        when they run (a captured graph picks up what it holds at replay).  Place: include/ddp_mi355x.h, "x0 hints"."""
        return self._input_view(_ROW['hints'])

    def set_hints(self, hints):
        """copy ``hints`` (B, h, w) - uint8 for seg, float32 for depth, on the engine's device - into the hint map (stream-ordered)"""
        self._write_input(_ROW['hints'], hints)

    def clear_hints(self, _if_any=False):
        """every pixel free (seg: 255, depth: 0)"""
        self._clear_input(_ROW['hints'], _if_any)

    # ---- DDP_FLAG_PRIOR_START ------------------------------------------------------------------
    def _prior_places(self):
        c = self.cfg
        if not c.flags & _lib.FLAG_PRIOR_START:
            raise _lib.DdpError('the prior map and last_start() need an engine built with prior_start=True')
        return prior_start_places(c, self._workspace_bytes())

    def prior_view(self):
        """(B, h, w) VIEW of the caller-written prior map inside the workspace - uint8 (seg), float32 (depth) or int32 bit words
        (bev; the C side's uint32); the kernel reads it when it runs (a captured graph picks up what it holds at replay).  Place:
        include/ddp_mi355x.h, "prior start"."""
        return self._input_view(_ROW['prior'])

    def set_prior(self, prior):
        """copy ``prior`` (B, h, w) - uint8 for seg, float32 for depth, int32 for bev, on the engine's device - into the prior map
        (stream-ordered)"""
        self._write_input(_ROW['prior'], prior)

    def clear_prior(self, _if_any=False):
        """no prior knowledge anywhere: seg 255 (the ignore row), depth 0 (the middle of the range), bev 0 (no class present)"""
        self._clear_input(_ROW['prior'], _if_any)

    def last_start(self):
        """(B, r, Cm, h, w) float32 VIEW of the start map the LAST sample() call (or graph replay) formed from the prior and its
        noise; valid until the next call.  (With ``seeded_noise`` this is the seeded-noise buffer, mixed in place.)"""
        c = self.cfg
        self._prior_places()
        if not getattr(self, '_sampled', False):
            raise _lib.DdpError('no start map yet: call sample() first')
        return self._region('seed_noise' if c.flags & _lib.FLAG_SEEDED_NOISE else 'prior_start', torch.float32,
                            (c.batch, c.randsteps, 1 if c.task == _lib.TASK_DEPTH else 256, c.h, c.w))

    # ---- DDP_FLAG_CLASS_PRIOR ------------------------------------------------------------------
    def class_prior_view(self):
        """(B, 256) float32 VIEW of the caller-written class prior table inside the workspace; columns >= num_classes are ignored.
        The library reads it when ddp_sample runs (a captured graph picks up what it holds at replay).  Place:
        include/ddp_mi355x.h, "class prior"."""
        return self._input_view(_ROW['class_prior'])

    def set_class_prior(self, prior):
        """copy ``prior`` (B, num_classes) - a floating-point tensor on the engine's device - into the table (stream-ordered)"""
        self._write_input(_ROW['class_prior'], prior)

    def clear_class_prior(self, _if_any=False):
        """no prior: every entry 0 (the bits of the flag-clear call)"""
        self._clear_input(_ROW['class_prior'], _if_any)

    # ---- DDP_FLAG_SCORE_PRIOR ------------------------------------------------------------------
    def score_prior_view(self):
        """(B, num_classes, h, w) float32 VIEW of the caller-written score prior map inside the workspace.  The library reads it when
        ddp_sample runs (a captured graph picks up what it holds at replay).  Place: include/ddp_mi355x.h, "score prior"."""
        return self._input_view(_ROW['score_prior'])

    def set_score_prior(self, prior):
        """copy ``prior`` (B, num_classes, h, w) - a floating-point tensor on the engine's device - into the map (stream-ordered)"""
        self._write_input(_ROW['score_prior'], prior)

    def clear_score_prior(self, _if_any=False):
        """no prior: every entry 0 (the bits of the flag-clear call)"""
        self._clear_input(_ROW['score_prior'], _if_any)

    # ------------------------------------------------------------------------------------------
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def geometry(self):
        return (self.cfg.batch, self.cfg.h, self.cfg.w)

    def set_geometry(self, batch=None, h=None, w=None, grow=1.25):
        """Switch the engine to another (batch, h, w) WITHOUT touching anything derived from the weights: the reference's
        test protocol is one image per call with a new size almost every call (segmentation/tools/test.py:214-219).
        The model region of the workspace (split weight planes, weight streams, LUTs, time / FiLM vectors) is kept - moved
        with one device-to-device copy if the buffer has to grow - and only ``ddp_prepare_geometry`` runs (positional
        tables + the zero border of the padded value maps)."""
        c = self.cfg
        nb = c.batch if batch is None else int(batch)
        nh = c.h if h is None else int(h)
        nw = c.w if w is None else int(w)
        if (nb, nh, nw) == (c.batch, c.h, c.w):
            return self
        # everything is validated / grown / prepared on a COPY of the cfg; self.cfg changes only on success, so a failed
        # switch (too many tokens, out of memory, a launch error) leaves the engine on its old, still prepared geometry
        n = _lib.DdpCfg.from_buffer_copy(c)
        n.batch, n.h, n.w = nb, nh, nw
        if self.task != 'bev' and (c.head_h, c.head_w) == (c.h, c.w):
            n.head_h, n.head_w = nh, nw             # the decoder grid follows the map (bev: the grid transform's output scope;
                                                    # a constructor head_hw that differs from the map is kept as given)
        nbytes = C.c_size_t(0)
        _lib.check(self.lib.ddp_query_workspace(C.byref(n), C.byref(nbytes)), self.lib)
        need = nbytes.value // 4
        ws = self.workspace
        if need > ws.numel():
            ws = torch.empty(int(need * grow), dtype=torch.float32, device=self.device)
            if self._prepared:
                ws[:self._const_floats].copy_(self.workspace[:self._const_floats])
        if self._prepared:
            with torch.cuda.device(self.device):
                _lib.check(self.lib.ddp_prepare_geometry(C.byref(n), ws.data_ptr(), self._stream()), self.lib)
        self.cfg, self.workspace = n, ws
        self.geometry_changes += 1
        self._x0_set = False       # force_x0: the decisions buffer belongs to the geometry region
        self._sampled = False      # (so do the step record and the disagreement map)
        for row in CALLER_INPUTS:  # (and the caller-written inputs: another geometry or another buffer - an unset input is none)
            self._clear_input(row, _if_any=True)
        return self

    def out_shape(self):
        c = self.cfg
        if self.task == 'depth':
            return (c.batch, 1, c.h, c.w)
        return (c.batch, c.num_classes, c.head_h, c.head_w)

    def prepare(self):
        with torch.cuda.device(self.device):       # launches go to the CURRENT device: make it the workspace's
            _lib.check(self.lib.ddp_prepare(C.byref(self.cfg), C.byref(self.weights.struct), self.steps,
                                            self.workspace.data_ptr(), self._stream()), self.lib)
        self._prepared = True

    def sample(self, x, noise=None, step_noise=None, out=None, *, seed=None, image_base=0, call=0, stream_base=0, _key_ready=False):
        """x (B,Cx,h,w); noise (B,r,Cm,h,w); step_noise (K,B,r,Cm,h,w) for ddpm -> output tensor.
        ``seeded_noise=True`` engines: ``seed`` (64 bit), ``image_base`` (image b of the batch draws the noise of image
        ``image_base + b``), ``call`` (separates the sampler calls that belong to one image) and ``stream_base`` make the key, which
        is written to the engine's device key tensor on the current stream in front of the call."""
        c = self.cfg
        cm = 1 if self.task == 'depth' else 256
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        assert tuple(x.shape) == (c.batch, c.feat_channels, c.h, c.w), (tuple(x.shape), (c.batch, c.feat_channels, c.h, c.w))
        if self._noise_args(noise, step_noise, seed):
            if not _key_ready:
                self._write_key(seed, image_base, stream_base, call)
            noise = self._key
        else:
            assert noise.is_cuda and noise.dtype == torch.float32 and noise.is_contiguous()
            assert noise.numel() == c.batch * c.randsteps * cm * c.h * c.w
            if self.sampler == 'ddpm':
                assert step_noise is not None and step_noise.is_contiguous() and step_noise.numel() == c.timesteps * noise.numel()
        if not self._prepared:
            self.prepare()
        if (c.flags & _lib.FLAG_FORCE_X0) and not getattr(self, '_x0_set', False):
            raise _lib.DdpError('force_x0 engine: call set_x0_decisions() before sample()')
        if out is None:
            out = torch.empty(self.out_shape(), dtype=torch.float32, device=self.device)
        if x.device != self.device or noise.device != self.device or out.device != self.device:
            raise _lib.DdpError(f'engine lives on {self.device}: x / noise / out must be on the same device')
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ddp_sample(C.byref(c), C.byref(self.weights.struct), self.steps, x.data_ptr(),
                                           noise.data_ptr(), step_noise.data_ptr() if step_noise is not None else None,
                                           out.data_ptr(), self.workspace.data_ptr(), self._stream()), self.lib)
        self._sampled = True
        return out

    def _step_base(self):
        if not self.cfg.flags & _lib.FLAG_STEP_RECORD:
            raise _lib.DdpError('step_record() / step_disagreement() need an engine built with record_steps=True')
        if not getattr(self, '_sampled', False):
            raise _lib.DdpError('no step record yet: call sample() first')
        p = C.c_void_p()
        _lib.check(self.lib.ddp_x0_trace(C.byref(self.cfg), self.workspace.data_ptr(), C.byref(p)), self.lib)
        return p.value - self.workspace.data_ptr()

    def step_record(self):
        """(K, B, r, H, W): what every step of the LAST sample() call predicted, per noise replica - seg uint8 argmax class, depth
        float32 metric depth, bev int32 bit words (bit c = prob_c > threshold; the C side's uint32).  A fresh tensor."""
        return step_record_view(self.workspace, self._step_base(), self.cfg).clone()

    def step_disagreement(self):
        """(B, H, W) float32: where the K * r recorded predictions of the LAST sample() call disagree with its output - seg / bev
        the fraction of differing decisions, depth the standard deviation (include/ddp_mi355x.h).  A fresh tensor."""
        return step_disagreement_view(self.workspace, self._step_base(), self.cfg).clone()

    def capture(self, x, noise=None, step_noise=None, *, seed=None, image_base=0, call=0, stream_base=0):
        """``seeded_noise=True`` engines: ``capture(x, seed=...)`` - the graph holds no noise tensor; the kernels read the key
        from the engine's device key tensor, which ``SampleGraph.replay(seed=...)`` rewrites in front of the launch.
        One ``sample()`` call as a hipGraph (``torch.cuda.CUDAGraph`` is hipGraph on ROCm): ``ddp_sample`` neither
        synchronises nor touches host memory after enqueue - its ~45 launches (kernels, device-to-device copies, memsets) go to
        the stream it is given, the schedule scalars travel as kernel arguments - so the whole K-step loop records under stream
        capture and replays with ONE host call.  What that buys is host time: one image per call (the reference's protocol, and
        the strong-scaling shard) is ~4 ms of GPU work behind ~45 launches, issued by 8 ranks that share the node's cores with
        their data loaders.  Inputs are copied into the graph's own static buffers at replay; -> ``SampleGraph``."""
        if not self._prepared:
            self.prepare()
        kw = {}
        if self._noise_args(noise, step_noise, seed):
            self._write_key(seed, image_base, stream_base, call)      # (host -> device: in front of the capture, never inside it)
            torch.cuda.synchronize(self.device)
            sn = ssn = None
            kw = dict(seed=seed, _key_ready=True)
        else:
            sn = noise.detach().clone()
            ssn = step_noise.detach().clone() if step_noise is not None else None
        sx = x.detach().clone()
        out = torch.empty(self.out_shape(), dtype=torch.float32, device=self.device)
        cur = torch.cuda.current_stream(self.device)
        side = torch.cuda.Stream(self.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):              # warm-up on the capture stream: one-time attribute calls happen here
            self.sample(sx, sn, ssn, out=out, **kw)
        cur.wait_stream(side)
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            self.sample(sx, sn, ssn, out=out, **kw)
        return SampleGraph(self, g, sx, sn, ssn, out)

    def _x0_view(self, which):
        c = self.cfg
        p = C.c_void_p()
        _lib.check(self.lib.ddp_x0_trace(C.byref(c), self.workspace.data_ptr(), C.byref(p)), self.lib)
        n = c.timesteps * c.batch * c.randsteps * c.head_h * c.head_w
        off = p.value - self.workspace.data_ptr() + which * n
        return self.workspace.view(torch.uint8)[off:off + n].view(c.timesteps, c.batch * c.randsteps, c.head_h, c.head_w)

    def x0_trace(self):
        """(K, B*r, h, w) uint8: the argmax class every step of the LAST sample() call found (needs record_x0=True or
        force_x0=True; record_x0: that is also what the step fed back, force_x0: the step fed back set_x0_decisions()'s)."""
        return self._x0_view(1 if self.cfg.flags & _lib.FLAG_FORCE_X0 else 0).clone()

    def set_x0_decisions(self, decisions):
        """force_x0=True (test instrument, DDP_FLAG_FORCE_X0): the classes (K, B*r, h, w) every step of the following sample()
        calls feeds back instead of its own argmax - e.g. the decisions a reference run recorded (tests/golden/full_*.npz)."""
        if not self.cfg.flags & _lib.FLAG_FORCE_X0:
            raise _lib.DdpError('set_x0_decisions needs an engine built with force_x0=True')
        v = self._x0_view(0)
        d = decisions.to(device=self.device, dtype=torch.uint8).reshape(v.shape)
        if int(d.max()) >= self.cfg.num_classes:
            raise ValueError('decision outside [0, num_classes)')
        v.copy_(d)
        self._x0_set = True

    def head_forward(self, feat, temb):
        """DeformableHeadWithTime.forward on (R,256,h,w) + (1|R,1024) time embedding."""
        c = self.cfg
        R = c.batch * c.randsteps
        assert feat.is_cuda and feat.is_contiguous() and tuple(feat.shape) == (R, 256, c.h, c.w)
        t = None
        if temb is not None:
            t = temb.reshape(-1, 1024)[0].contiguous()
        shape = (R, 1, c.h, c.w) if self.task == 'depth' else (R, c.num_classes, c.head_h, c.head_w)
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ddp_head_forward(C.byref(c), C.byref(self.weights.struct), feat.data_ptr(),
                                                 t.data_ptr() if t is not None else None, out.data_ptr(),
                                                 self.workspace.data_ptr(), self._stream()), self.lib)
        self._prepared = False      # head_forward rewrites the FiLM slot of step 0
        return out


def step_record_sizes(cfg):
    """(record_bytes, map_bytes) of include/ddp_mi355x.h (DDP_FLAG_STEP_RECORD), as formulas of the cfg"""
    n = cfg.batch * cfg.head_h * cfg.head_w
    return cfg.timesteps * cfg.randsteps * n * (1 if cfg.task == _lib.TASK_SEG else 4), n * 4


def _round256(n):
    return (n + 255) // 256 * 256


def caller_regions(cfg, workspace_bytes):
    """{name: (offset, nbytes)}, in workspace order, of the buffers at the END of a sampler workspace that the caller reads or writes
    directly or that lie between them: THE host-side table of the ordered list in include/ddp_mi355x.h (at ddp_query_workspace;
    csrc/ddp_api.hip carve_caller_regions is the same table in C).  ``workspace_bytes`` = ddp_query_workspace(cfg), or
    ddp_sample_fcn_workspace(cfg, ...) for the FCN loop, whose cfg can only carry the last two groups.  Each buffer is rounded up
    to 256 bytes and exists only with its flag; the last one ends at ``workspace_bytes``."""
    f = cfg.flags
    seg, depth = cfg.task == _lib.TASK_SEG, cfg.task == _lib.TASK_DEPTH
    n = cfg.batch * cfg.h * cfg.w
    px = 1 if seg else 4                                            # bytes per pixel of a hint / prior map
    noise = n * cfg.randsteps * (1 if depth else 256) * 4           # a (B, r, Cm, h, w) float map: start noise, start map
    rec, smap = step_record_sizes(cfg)
    sp, cp, ps, xh, sn, sr = (bool(f & b) for b in (_lib.FLAG_SCORE_PRIOR, _lib.FLAG_CLASS_PRIOR, _lib.FLAG_PRIOR_START,
                                                    _lib.FLAG_X0_HINTS, _lib.FLAG_SEEDED_NOISE, _lib.FLAG_STEP_RECORD))
    kp = (cfg.num_classes + 63) // 64 * 64                          # the score prior's row length: whole 64-class chunks
    table = [('sprior_rows', n * kp * 4, sp), ('sprior_map', n * cfg.num_classes * 4, sp),
             ('cprior_rows', 2 * cfg.batch * 256 * 4, cp), ('cprior_table', cfg.batch * 256 * 4, cp),
             ('prior_start', noise, ps and not sn), ('prior_map', n * px, ps),
             ('hint_rows', n * cfg.randsteps * px, xh), ('hint_map', n * px, xh),
             ('seed_noise', noise, sn),
             ('step_rec', rec, sr), ('step_map', smap, sr)]
    out, end = [], workspace_bytes
    for name, nbytes, present in reversed(table):
        if present:
            end -= _round256(nbytes)
            out.append((name, (end, nbytes)))
    return dict(reversed(out))


CallerInput = namedtuple('CallerInput', 'name kwarg flag flag_name region dtypes shape dst accepts clear '
                                        'needs dims where built_for wrong_task fcn')
CallerInput.__doc__ = """One input the caller writes into the workspace in front of a sampler call: what ``DDPEngine`` (views, setters,
clears, the constructor's task check), ``SampleGraph.replay`` and ``FcnSamplerEngine`` know about it.
``name``: the public name (``<name>_view`` / ``set_<name>`` / ``clear_<name>``, ``replay(<name>=)``); ``kwarg``: the constructor's keyword;
``flag`` / ``flag_name``: the bit and how the header spells it; ``region``: the caller-written buffer of ``caller_regions``; ``dtypes``:
{task: the view's dtype} - its keys are the tasks the input exists for; ``shape(cfg)``: the view's; ``dst(view, cfg)``: the slice
``set_<name>`` writes; ``accepts``: 'floating-point', or None for exactly the view's dtype; ``clear``: {dtype: the value that says "nothing
given"}.  The phrases of its messages: ``needs`` (view / set / clear on a flag-clear engine), ``dims`` and ``where`` (a wrong shape, a
wrong device), ``built_for`` and ``wrong_task`` (the constructor, for a task outside ``dtypes``), ``fcn`` (the FCN-head loop)."""


def _whole(view, cfg):
    return view


def _class_columns(view, cfg):
    return view[:, :cfg.num_classes]


def _bhw(cfg):
    return (cfg.batch, cfg.h, cfg.w)


def _bkhw(cfg):
    return (cfg.batch, cfg.num_classes, cfg.h, cfg.w)


def _b256(cfg):
    return (cfg.batch, 256)


# the rows of caller_regions that the caller writes, in its order
CALLER_INPUTS = (
    CallerInput(name='score_prior', kwarg='score_prior', flag=_lib.FLAG_SCORE_PRIOR, flag_name='DDP_FLAG_SCORE_PRIOR',
                region='sprior_map', dtypes={_lib.TASK_SEG: torch.float32}, shape=_bkhw, dst=_whole,
                accepts='floating-point', clear={torch.float32: 0},
                needs='the score prior needs', dims='batch, num_classes, h, w', where='the score prior is',
                built_for='segmentation sampler', wrong_task='task {task!r} takes none', fcn='takes no score prior'),
    CallerInput(name='class_prior', kwarg='class_prior', flag=_lib.FLAG_CLASS_PRIOR, flag_name='DDP_FLAG_CLASS_PRIOR',
                region='cprior_table', dtypes={_lib.TASK_SEG: torch.float32}, shape=_b256, dst=_class_columns,
                accepts='floating-point', clear={torch.float32: 0},
                needs='the class prior needs', dims='batch, num_classes', where='the class prior is',
                built_for='segmentation sampler', wrong_task='task {task!r} takes none', fcn='takes no class prior'),
    CallerInput(name='prior', kwarg='prior_start', flag=_lib.FLAG_PRIOR_START, flag_name='DDP_FLAG_PRIOR_START',
                region='prior_map', dtypes={_lib.TASK_SEG: torch.uint8, _lib.TASK_DEPTH: torch.float32, _lib.TASK_BEV: torch.int32},
                shape=_bhw, dst=_whole, accepts=None, clear={torch.uint8: 255, torch.float32: 0, torch.int32: 0},
                needs='the prior map and last_start() need', dims='batch, h, w', where='the prior is',
                built_for='seg, depth and bev samplers', wrong_task='task {task!r} takes none', fcn='starts from noise'),
    CallerInput(name='hints', kwarg='x0_hints', flag=_lib.FLAG_X0_HINTS, flag_name='DDP_FLAG_X0_HINTS',
                region='hint_map', dtypes={_lib.TASK_SEG: torch.uint8, _lib.TASK_DEPTH: torch.float32},
                shape=_bhw, dst=_whole, accepts=None, clear={torch.uint8: 255, torch.float32: 0},
                needs='hints need', dims='batch, h, w', where='hints are',
                built_for='seg and depth samplers', wrong_task='the {task} sampler takes no hints', fcn='takes no hints'),
)
_ROW = {row.name: row for row in CALLER_INPUTS}


def prior_start_places(cfg, workspace_bytes):
    """(prior_offset, prior_bytes, start_offset, start_bytes) of include/ddp_mi355x.h ("prior start"), in bytes from the start of a
    workspace of ``workspace_bytes`` = ddp_query_workspace(cfg).  With DDP_FLAG_SEEDED_NOISE the start map is the seeded-noise buffer."""
    r = caller_regions(cfg, workspace_bytes)
    return r['prior_map'] + r['seed_noise' if cfg.flags & _lib.FLAG_SEEDED_NOISE else 'prior_start']


def class_prior_places(cfg, workspace_bytes):
    """(table_offset, table_bytes, bias_offset, bias_bytes) of include/ddp_mi355x.h ("class prior"), in bytes from the start of a
    workspace of ``workspace_bytes`` = ddp_query_workspace(cfg): the caller's table, the library's per-image vectors in front of it."""
    r = caller_regions(cfg, workspace_bytes)
    return r['cprior_table'] + r['cprior_rows']


def score_prior_places(cfg, workspace_bytes):
    """(map_offset, map_bytes, rows_offset, rows_bytes) of include/ddp_mi355x.h ("score prior"), in bytes from the start of a
    workspace of ``workspace_bytes`` = ddp_query_workspace(cfg): the caller's NCHW map, the library's token-major rows in front of it."""
    r = caller_regions(cfg, workspace_bytes)
    return r['sprior_map'] + r['sprior_rows']


def class_mask_to_prior(mask):
    """bool (B, K) "class k can occur in image b" -> the float32 class prior that says exactly that: 0 where True, -inf where False"""
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool or mask.dim() != 2:
        raise ValueError(f'class_mask_to_prior takes a bool (B, K) tensor, got {getattr(mask, "dtype", type(mask))} '
                         f'{tuple(getattr(mask, "shape", ()))}')
    out = torch.zeros(mask.shape, dtype=torch.float32, device=mask.device)
    return out.masked_fill_(~mask, float('-inf'))


def step_record_view(workspace, base, cfg):
    dtype = {_lib.TASK_SEG: torch.uint8, _lib.TASK_DEPTH: torch.float32, _lib.TASK_BEV: torch.int32}[cfg.task]
    nbytes = step_record_sizes(cfg)[0]
    return workspace.view(torch.uint8)[base:base + nbytes].view(dtype).view(cfg.timesteps, cfg.batch, cfg.randsteps, cfg.head_h, cfg.head_w)


def step_disagreement_view(workspace, base, cfg):
    rec, nbytes = step_record_sizes(cfg)
    off = base + _round256(rec)
    return workspace.view(torch.uint8)[off:off + nbytes].view(torch.float32).view(cfg.batch, cfg.head_h, cfg.head_w)


class SampleGraph:
    """A captured ``DDPEngine.sample`` call (``DDPEngine.capture``).  ``replay(x, noise)`` copies the inputs into the graph's
    static buffers (stream-ordered, on the current stream) and launches the graph; the returned tensor is the graph's static
    output buffer (clone it to keep a result across replays).  Valid for the geometry and schedule it was captured with."""

    def __init__(self, engine, graph, x, noise, step_noise, out):
        self.engine, self.graph = engine, graph
        self.x, self.noise, self.step_noise, self.out = x, noise, step_noise, out
        self.geometry = engine.geometry()
        # the graph has the workspace's ADDRESS baked into every launch: keep that allocation alive for as long as the graph
        # exists (a replay can then never touch freed memory) and refuse to replay once the engine has moved to another one
        self.workspace = engine.workspace
        self.workspace_ptr = engine.workspace.data_ptr()

    def replay(self, x=None, noise=None, step_noise=None, seed=None, image_base=None, call=None, hints=None, prior=None,
               class_prior=None, score_prior=None):
        """``score_prior`` (score_prior engines): written to the engine's map in front of the launch (``DDPEngine.set_score_prior``);
        None: the graph runs on what the map holds.
        ``class_prior`` (class_prior engines): written to the engine's table in front of the launch (``DDPEngine.set_class_prior``);
        None: the graph runs on what the table holds.
        ``prior`` (prior_start engines): written to the engine's prior map in front of the launch (``DDPEngine.set_prior``); None:
        the graph runs on what the map holds.
        ``hints`` (x0_hints engines): written to the engine's hint map in front of the launch (``DDPEngine.set_hints``); None: the
        graph runs on what the map holds.
        seeded engines: ``seed`` / ``image_base`` / ``call`` given here replace those words of the engine's device key (stream-
        ordered, in front of the launch); none given: the graph repeats the last key."""
        eng = self.engine
        if eng.seeded:
            if noise is not None or step_noise is not None:
                raise _lib.DdpError('seeded_noise engine: replay(seed=...), not noise= / step_noise=')
        elif seed is not None or image_base is not None or call is not None:
            raise _lib.DdpError('seed= / image_base= / call= need an engine built with seeded_noise=True')
        if eng.geometry() != self.geometry:
            raise _lib.DdpError(f'graph captured for geometry {self.geometry}, engine is now at {eng.geometry()}')
        if eng.workspace.data_ptr() != self.workspace_ptr:
            raise _lib.DdpError('stale graph: the engine\'s workspace was reallocated after the capture (set_geometry grew it); '
                                'capture again')
        if not eng._prepared:      # head_forward() rewrote the FiLM slot of step 0: restore the constants (same addresses)
            eng.prepare()
        if x is not None:
            self.x.copy_(x, non_blocking=True)
        if noise is not None:
            self.noise.copy_(noise.reshape(self.noise.shape), non_blocking=True)
        if step_noise is not None:
            self.step_noise.copy_(step_noise.reshape(self.step_noise.shape), non_blocking=True)
        if seed is not None or image_base is not None or call is not None:
            eng._write_key(seed, image_base, None, call)
        given = dict(hints=hints, prior=prior, class_prior=class_prior, score_prior=score_prior)
        for row in CALLER_INPUTS:
            if given[row.name] is not None:
                eng._write_input(row, given[row.name])
        self.graph.replay()
        return self.out


class FcnSamplerEngine(_SeededNoise):
    """The K-step sampler with ``FCNHeadWithTime`` as decode head (``ddp_sample_fcn``): same inputs,
    schedule and outputs as ``DDPEngine`` for task 'seg'.  ``head`` is a ``ddp_amd.FCNHeadWithTime`` (parameter holder)."""

    def __init__(self, state_dict, head, *, h, w, batch=1, randsteps=1, timesteps=3, num_classes=150, bit_scale=0.01,
                 time_difference=1, sample_range0=0.0, noise_schedule='cosine', sampler='ddim', accumulation=False,
                 device=None, head_prefix='decode_head.', lib_path=None, record_steps=False, seeded_noise=False, x0_hints=False,
                 prior_start=False, class_prior=False, score_prior=False):
        asked = dict(x0_hints=x0_hints, prior_start=prior_start, class_prior=class_prior, score_prior=score_prior)
        for row in CALLER_INPUTS:
            if asked[row.kwarg]:
                raise ValueError(f'{row.kwarg} is built for ddp_sample only ({row.flag_name}): the FCN-head loop {row.fcn}')
        self.lib = _lib.load(lib_path)
        if not torch.cuda.is_available():
            raise _lib.DdpError('no HIP device visible: ddp_amd has no CPU path')
        self.device = torch.device(device if device is not None else f'cuda:{torch.cuda.current_device()}')
        self.weights = PackedWeights(state_dict, 'seg', 0, self.device, head_prefix)      # transform, time_mlp, embedding, conv_seg
        self.head = head
        self.convs, self._keep = head.conv_array()
        for t in self._keep:
            if t.device != self.device:
                raise _lib.DdpError(f'FCN head parameters live on {t.device}, engine on {self.device}')
        cfg = _lib.DdpCfg()
        cfg.abi_version = _lib.ABI_VERSION
        cfg.task, cfg.sampler = _lib.TASK_SEG, SAMPLERS[sampler]
        cfg.batch, cfg.randsteps, cfg.timesteps, cfg.num_layers = batch, randsteps, timesteps, 0
        cfg.num_classes, cfg.feat_channels = num_classes, 256
        cfg.h = cfg.head_h = h
        cfg.w = cfg.head_w = w
        cfg.gemm_mode = _lib.GEMM_BF16X3
        cfg.flags = (_lib.FLAG_STEP_RECORD if record_steps else 0) | (_lib.FLAG_SEEDED_NOISE if seeded_noise else 0)
        cfg.accumulation, cfg.bit_scale = int(bool(accumulation)), bit_scale
        self.cfg, self.sampler = cfg, sampler
        recs = schedule.step_records('seg', timesteps, time_difference, sample_range0, noise_schedule, sampler)
        self.steps = (_lib.DdpStep * timesteps)()
        for i, r in enumerate(recs):
            for k, v in r.items():
                setattr(self.steps[i], k, v)
        nbytes = C.c_size_t(0)
        _lib.check(self.lib.ddp_sample_fcn_workspace(C.byref(cfg), head.num_convs, head.dilation, C.byref(nbytes)), self.lib)
        self._ws_bytes = nbytes.value
        self.workspace = torch.empty(nbytes.value // 4 + 64, dtype=torch.float32, device=self.device)
        self._prepared = False
        self._sampled = False
        self._init_key()

    def _workspace_bytes(self):
        return self._ws_bytes

    def prepare(self):
        """``ddp_prepare_fcn``: everything that depends on weights and schedule only (time embeddings, x0 table, concat-conv
        column blocks, per (step, conv) FiLM -> folded affine -> scaled, split weights as stage images) once per engine; every
        ``sample()`` afterwards runs with ``DDP_FLAG_FCN_PREPARED`` and launches none of those kernels."""
        c = self.cfg
        c.flags &= ~_lib.FLAG_FCN_PREPARED
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ddp_prepare_fcn(C.byref(c), C.byref(self.weights.struct), self.convs, self.head.num_convs,
                                                self.head.dilation, self.steps, self.workspace.data_ptr(),
                                                torch.cuda.current_stream(self.device).cuda_stream), self.lib)
        c.flags |= _lib.FLAG_FCN_PREPARED
        self._prepared = True

    def sample(self, x, noise=None, step_noise=None, out=None, *, seed=None, image_base=0, call=0, stream_base=0):
        """as ``DDPEngine.sample`` (seeded engines: ``seed=`` ... in place of ``noise=`` / ``step_noise=``)"""
        c = self.cfg
        if not self._prepared:
            self.prepare()
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (c.batch, 256, c.h, c.w)
        if self._noise_args(noise, step_noise, seed):
            self._write_key(seed, image_base, stream_base, call)
            noise = self._key
        else:
            assert noise.is_cuda and noise.is_contiguous() and noise.numel() == c.batch * c.randsteps * 256 * c.h * c.w
            if self.sampler == 'ddpm':
                assert step_noise is not None and step_noise.is_contiguous() and step_noise.numel() == c.timesteps * noise.numel()
        if out is None:
            out = torch.empty((c.batch, c.num_classes, c.h, c.w), dtype=torch.float32, device=self.device)
        if x.device != self.device or noise.device != self.device or out.device != self.device:
            raise _lib.DdpError(f'engine lives on {self.device}: x / noise / out must be on the same device')
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ddp_sample_fcn(C.byref(c), C.byref(self.weights.struct), self.convs, self.head.num_convs,
                                               self.head.dilation, self.steps, x.data_ptr(), noise.data_ptr(),
                                               step_noise.data_ptr() if step_noise is not None else None, out.data_ptr(),
                                               self.workspace.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream),
                       self.lib)
        self._sampled = True
        return out

    def _step_base(self):
        if not self.cfg.flags & _lib.FLAG_STEP_RECORD:
            raise _lib.DdpError('step_record() / step_disagreement() need an engine built with record_steps=True')
        if not self._sampled:
            raise _lib.DdpError('no step record yet: call sample() first')
        return caller_regions(self.cfg, self._ws_bytes)['step_rec'][0]

    def step_record(self):
        """(K, B, r, h, w) uint8: the argmax class every step of the LAST sample() call fed back.  A fresh tensor."""
        return step_record_view(self.workspace, self._step_base(), self.cfg).clone()

    def step_disagreement(self):
        """(B, h, w) float32: the fraction of the K * r recorded decisions that differ from the output's argmax.  A fresh tensor."""
        return step_disagreement_view(self.workspace, self._step_base(), self.cfg).clone()


def seg_postprocess(scores, img_size, crop_size=None, out_size=None, align_corners=False, flip=None, out=None):
    """Fused post-loop epilogue: class map (B,out_h,out_w) uint8 from scores (B,K,h,w).

    Replaces resize -> crop -> resize -> softmax -> flip -> argmax of the reference
    (segmentors/ddp.py:124-128, encoder_decoder.py:229-296).  CUDA tensors only; no CPU path.
    """
    if not scores.is_cuda:
        raise _lib.DdpError('seg_postprocess: scores must be a CUDA tensor (no CPU path)')
    scores = scores.contiguous().float()
    B, K, h, w = scores.shape
    H, W = int(img_size[0]), int(img_size[1])
    ch, cw = (H, W) if crop_size is None else (int(crop_size[0]), int(crop_size[1]))
    oh, ow = (ch, cw) if out_size is None else (int(out_size[0]), int(out_size[1]))
    fl = {None: 0, False: 0, 'horizontal': 1, 'vertical': 2}[flip]
    if out is None:
        out = torch.empty((B, oh, ow), dtype=torch.uint8, device=scores.device)
    lib = _lib.load()
    with torch.cuda.device(scores.device):
        _lib.check(lib.ddp_seg_postprocess(scores.data_ptr(), B, K, h, w, H, W, ch, cw, oh, ow, int(bool(align_corners)), fl,
                                           out.data_ptr(), torch.cuda.current_stream(scores.device).cuda_stream))
    return out


def seg_aug_postprocess(scores_list, metas, out_size, align_corners=False, return_prob=False):
    """Fused multi-scale / flip epilogue (``ddp_seg_aug_postprocess``): class map (B,out_h,out_w) uint8 from the low-resolution
    scores of every augmentation.  Replaces, per augmentation, resize -> crop -> resize -> softmax -> flip of the reference's
    ``inference`` and the running mean + argmax of ``aug_test`` (encoder_decoder.py:229-331) without materialising any
    (B,K,H,W) tensor.  ``metas[i]`` = dict(img_size=(H,W), crop_size=(h,w) or None, flip=None|'horizontal'|'vertical')."""
    if not scores_list or len(scores_list) != len(metas) or len(scores_list) > _lib.MAX_AUGS:
        raise ValueError(f'seg_aug_postprocess: 1..{_lib.MAX_AUGS} augmentations with one meta each')
    dev = scores_list[0].device
    if not scores_list[0].is_cuda:
        raise _lib.DdpError('seg_aug_postprocess: scores must be CUDA tensors (no CPU path)')
    B, K = scores_list[0].shape[:2]
    keep = []
    augs = (_lib.DdpSegAug * len(scores_list))()
    for i, (sc, m) in enumerate(zip(scores_list, metas)):
        sc = sc.contiguous().float()
        if sc.device != dev or sc.shape[0] != B or sc.shape[1] != K:
            raise ValueError('seg_aug_postprocess: every augmentation needs the same batch / classes / device')
        keep.append(sc)
        H, W = int(m['img_size'][0]), int(m['img_size'][1])
        ch, cw = (H, W) if m.get('crop_size') is None else (int(m['crop_size'][0]), int(m['crop_size'][1]))
        augs[i].d_scores = sc.data_ptr()
        augs[i].h, augs[i].w = sc.shape[2], sc.shape[3]
        augs[i].img_h, augs[i].img_w, augs[i].crop_h, augs[i].crop_w = H, W, ch, cw
        augs[i].flip = {None: 0, False: 0, 'horizontal': 1, 'vertical': 2}[m.get('flip')]
    oh, ow = int(out_size[0]), int(out_size[1])
    seg = torch.empty((B, oh, ow), dtype=torch.uint8, device=dev)
    prob = torch.empty((B, K, oh, ow), dtype=torch.float32, device=dev) if return_prob else None
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.ddp_seg_aug_postprocess(augs, len(keep), B, K, oh, ow, int(bool(align_corners)), seg.data_ptr(),
                                               prob.data_ptr() if prob is not None else None,
                                               torch.cuda.current_stream(dev).cuda_stream), lib)
    return (seg, prob) if return_prob else seg


def slide_windows(img_hw, crop_size, stride):
    """The window grid of ``slide_inference`` (encoder_decoder.py:186-206): -> (row origins y1, column origins x1, window size).
    A crop larger than the image shrinks to the image ("the small patch will be used to decode without padding")."""
    H, W = int(img_hw[0]), int(img_hw[1])
    (h_crop, w_crop), (h_stride, w_stride) = crop_size, stride
    h_grids = max(H - h_crop + h_stride - 1, 0) // h_stride + 1
    w_grids = max(W - w_crop + w_stride - 1, 0) // w_stride + 1
    ys = [max(min(i * h_stride + h_crop, H) - h_crop, 0) for i in range(h_grids)]
    xs = [max(min(j * w_stride + w_crop, W) - w_crop, 0) for j in range(w_grids)]
    return ys, xs, (min(h_crop, H), min(w_crop, W))


def seg_slide_postprocess(scores, ys, xs, crop_hw, img_size, keep_size=None, out_size=None, align_corners=False, flip=None,
                          want='seg'):
    """Fused sliding-window epilogue (``ddp_seg_slide_postprocess``).  ``scores`` (n_rows*n_cols, B, K, h, w): the sampler's
    low-resolution output for every window, row-major over the grid (ys x xs).  want: 'seg' -> uint8 class map (B,oh,ow);
    'prob' -> softmax probabilities (B,K,oh,ow) (``inference``); 'scores' -> the window-averaged scores (``slide_inference``).
    Replaces, per window, the resize of ``encode_decode`` and ``preds += F.pad(...)``, then ``/ count_mat``, crop, resize, softmax,
    flip, argmax (encoder_decoder.py:180-227, 266-296).  CUDA tensors only; no CPU path."""
    if not scores.is_cuda:
        raise _lib.DdpError('seg_slide_postprocess: scores must be a CUDA tensor (no CPU path)')
    n_rows, n_cols = len(ys), len(xs)
    scores = scores.contiguous().float()
    if scores.dim() != 5 or scores.shape[0] != n_rows * n_cols or n_rows * n_cols > _lib.MAX_WINDOWS:
        raise ValueError(f'seg_slide_postprocess: scores (windows, B, K, h, w) with windows = {n_rows} x {n_cols} <= {_lib.MAX_WINDOWS}')
    _, B, K, h, w = scores.shape
    H, W = int(img_size[0]), int(img_size[1])
    kh, kw = (H, W) if keep_size is None else (int(keep_size[0]), int(keep_size[1]))
    oh, ow = (kh, kw) if out_size is None else (int(out_size[0]), int(out_size[1]))
    dev = scores.device
    ptrs = (_lib._fp * (n_rows * n_cols))(*[scores[i].data_ptr() for i in range(n_rows * n_cols)])
    y1 = (C.c_int * n_rows)(*[int(v) for v in ys])
    x1 = (C.c_int * n_cols)(*[int(v) for v in xs])
    seg = torch.empty((B, oh, ow), dtype=torch.uint8, device=dev) if want == 'seg' else None
    prob = torch.empty((B, K, oh, ow), dtype=torch.float32, device=dev) if want != 'seg' else None
    mode = {'seg': 0, 'prob': 1, 'scores': 2}[want]
    fl = {None: 0, False: 0, 'horizontal': 1, 'vertical': 2}[flip]
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.ddp_seg_slide_postprocess(ptrs, y1, x1, n_rows, n_cols, B, K, h, w, int(crop_hw[0]), int(crop_hw[1]), H, W, kh, kw,
                                                 oh, ow, int(bool(align_corners)), fl, mode, seg.data_ptr() if seg is not None else None,
                                                 prob.data_ptr() if prob is not None else None,
                                                 torch.cuda.current_stream(dev).cuda_stream), lib)
    return seg if want == 'seg' else prob


def depth_postprocess(depth_list, flips, out_size, min_depth, max_depth, align_corners=False, out=None):
    """Fused post-loop epilogue of the depth toolbox (``ddp_depth_postprocess``): (B,1,out_h,out_w) fp32 from the low-resolution
    maps of every augmentation.  Replaces clamp -> bilinear resize (depth/depth/models/depther/ddp.py:95-109), the flip-undo of
    ``inference`` (encoder_decoder.py:187-194) and the running mean of ``aug_test`` (:210-229).  ``depth_list[i]`` (B,1,h_i,w_i)
    = the sampler's output for augmentation i; ``flips[i]`` None | 'horizontal' | 'vertical'.  One augmentation = ``simple_test``.
    CUDA tensors only; no CPU path."""
    if not depth_list or len(depth_list) != len(flips) or len(depth_list) > _lib.MAX_AUGS:
        raise ValueError(f'depth_postprocess: 1..{_lib.MAX_AUGS} augmentations with one flip entry each')
    if not depth_list[0].is_cuda:
        raise _lib.DdpError('depth_postprocess: depth maps must be CUDA tensors (no CPU path)')
    dev, B = depth_list[0].device, depth_list[0].shape[0]
    keep = []
    augs = (_lib.DdpDepthAug * len(depth_list))()
    for i, (d, fl) in enumerate(zip(depth_list, flips)):
        d = d.contiguous().float()
        if d.dim() != 4 or d.shape[1] != 1 or d.shape[0] != B or d.device != dev:
            raise ValueError('depth_postprocess: every augmentation needs a (B,1,h,w) map on the same device')
        keep.append(d)
        augs[i].d_depth = d.data_ptr()
        augs[i].h, augs[i].w = d.shape[2], d.shape[3]
        augs[i].flip = {None: 0, False: 0, 'horizontal': 1, 'vertical': 2}[fl]
    oh, ow = int(out_size[0]), int(out_size[1])
    if out is None:
        out = torch.empty((B, 1, oh, ow), dtype=torch.float32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.ddp_depth_postprocess(augs, len(keep), B, oh, ow, int(bool(align_corners)), C.c_float(min_depth),
                                             C.c_float(max_depth), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), lib)
    return out


def msda_forward_lds(value, samp, h, w, guess=None):
    """The deformable-attention core computed by the kernel the sampling loop runs (``ddp_msda_forward_lds``):
    value (R, h*w, 256), samp (R*h*w, 96) as for ``ddp_msda_forward``; guess (8,2) optional per-head window guess."""
    if not value.is_cuda:
        raise _lib.DdpError('msda_forward_lds: CUDA tensors only (no CPU path)')
    value, samp = value.contiguous().float(), samp.contiguous().float()
    rows = samp.shape[0]
    lib = _lib.load()
    nbytes = C.c_size_t(0)
    _lib.check(lib.ddp_msda_forward_lds_workspace(rows, h, w, C.byref(nbytes)), lib)
    ws = torch.empty(nbytes.value // 4 + 64, dtype=torch.float32, device=value.device)
    out = torch.empty((rows, 256), dtype=torch.float32, device=value.device)
    g = guess.contiguous().float() if guess is not None else None
    with torch.cuda.device(value.device):
        _lib.check(lib.ddp_msda_forward_lds(value.data_ptr(), samp.data_ptr(), g.data_ptr() if g is not None else None,
                                            out.data_ptr(), rows, h, w, ws.data_ptr(),
                                            torch.cuda.current_stream(value.device).cuda_stream), lib)
    return out
