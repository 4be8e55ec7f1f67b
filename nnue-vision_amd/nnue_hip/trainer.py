"""Training step of the NNUE hot path on MI355X, one process per GPU.

What train.py:359-366 does per batch (zero_grad, forward, cross-entropy, backward, clip_grad_norm_,
SGD step) is one fixed sequence of HIP kernels here, working on preallocated buffers:

    conv -> binarise+compact -> FT gather-accumulate -> pairwise+classifier -> cross-entropy
         -> classifier backward -> FT weight gather-sum -> FT value gather-dot -> STE/conv backward
         -> [all-reduce of ONE flat gradient buffer over RCCL when world > 1] -> fused clip + SGD

* every trainable parameter (all but nnue2score, which never has a gradient) lives in one flat fp32
  buffer; the module's parameters are views into it, so state_dict()/serialize keep working.  Gradients
  and momentum have matching flat buffers -- the all-reduce is a single call on a single buffer
  (3.8 MB at the CIFAR configs: latency-bound on xGMI, so one message, not one per tensor);
* shapes are static, nothing synchronises with the host, so the local part of the step is captured into
  a hipGraph and replayed (the C ABI launches on torch's current stream);
* data parallel = each rank takes an equal slice of the global batch; mean-loss gradients are summed
  by the all-reduce and scaled by 1/world inside the SGD kernel, where the *global* gradient norm is
  clipped -- every rank therefore applies the identical update.  Default: ONE all-reduce of the whole
  flat gradient buffer after the local step (the value gradient now leaves in the same launch as the
  weight gradient, so only ~16 us of STE kernels could still hide a first bucket -- less than a second
  collective costs).  NNUE_DP_BUCKETS=2 keeps the earlier split: everything except the threshold /
  conv-weight gradients (99.98 % of the bytes) is all-reduced while the STE/conv backward kernels run,
  the 232-float tail bucket follows.

``FlatLayout`` and ``DataParallel`` are device-agnostic plumbing (covered by gloo tests on CPU);
``NnueTrainer`` is GPU-only.
"""
from __future__ import annotations

import contextlib
import ctypes
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import os
import warnings

import torch
import torch.distributed as dist

from . import lib, step_mode

SKIP = ("nnue2score",)  # no gradient ever reaches it (reference tests/test_model.py:179-182)


def _checked_label_smoothing(value) -> float:
    value = float(value)
    if not 0.0 <= value < 1.0:
        raise ValueError(f"label_smoothing = {value} must lie in [0, 1)")
    return value


# The tensors NNUE._clip_weights clamps (nnue.py:528-539): the FeatureTransformer's table and the classifier's Linear weights (for
# num_ls_buckets > 1 the stacked [K, out, in] BucketedLinear weights).  Never the conv weights, the thresholds or a bias.
CLIPPED = ("input.weight", "classifier.classifier.0.weight", "classifier.classifier.2.weight", "classifier.classifier.4.weight")


def clip_ranges(layout: "FlatLayout"):
    """The clipped tensors as half-open element ranges of the layout's flat buffers, each extended to the next tensor's start
    (the last one to the buffers' end): the zero padding behind a tensor is clamped with it -- a no-op -- and every boundary is a
    multiple of the layout's alignment, so the float4 kernels see no ragged case."""
    ends = list(layout.offsets[1:]) + [layout.count]
    return [(layout.offsets[i], ends[i]) for i, k in enumerate(layout.names) if k in CLIPPED]


def _checked_schedule(values, position) -> Tuple[torch.Tensor, int]:
    """(values as a float32 CPU vector, position) of a per-step schedule, or ValueError."""
    values = torch.as_tensor(values).detach().to(device="cpu", dtype=torch.float32).contiguous()
    if values.dim() != 1 or values.numel() < 1:
        raise ValueError(f"a schedule is a 1-D sequence of at least one value, got shape {tuple(values.shape)}")
    if values.numel() > 2**31 - 1:
        raise ValueError("a schedule has at most 2^31 - 1 values")
    position = int(position)
    if not 0 <= position <= 2**31 - 1:
        raise ValueError(f"schedule position {position} must lie in 0 .. 2^31 - 1")
    return values, position


@dataclass
class FlatLayout:
    names: List[str]
    shapes: List[Tuple[int, ...]]
    offsets: List[int]
    count: int  # padded element count of the flat buffers

    @staticmethod
    def of(model: torch.nn.Module, align: int = 4, pad_to: int = 1) -> "FlatLayout":
        """pad_to: the flat buffers' length becomes a multiple of it (equal, float4-aligned shards per rank)."""
        names, shapes, offsets, off = [], [], [], 0
        for k, p in model.named_parameters():
            if k in SKIP:
                continue
            names.append(k)
            shapes.append(tuple(p.shape))
            offsets.append(off)
            off += (p.numel() + align - 1) // align * align  # 16-byte aligned starts for the float4 kernels
        return FlatLayout(names, shapes, offsets, (off + pad_to - 1) // pad_to * pad_to)

    def views(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        out = {}
        for k, s, o in zip(self.names, self.shapes, self.offsets):
            n = 1
            for d in s:
                n *= d
            out[k] = flat[o:o + n].view(s)
        return out

    def pack(self, tensors: Dict[str, torch.Tensor], device=None) -> torch.Tensor:
        some = next(iter(tensors.values()))
        flat = torch.zeros(self.count, dtype=torch.float32, device=device if device is not None else some.device)
        for k, v in self.views(flat).items():
            v.copy_(tensors[k])
        return flat


class DataParallel:
    """Batch sharding + the one collective of the step.  Backend: "nccl" (= RCCL over xGMI) on GPUs,
    "gloo" in the CPU tests."""

    def __init__(self, group=None):
        self.group = group
        self.enabled = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if self.enabled else 1
        self.rank = dist.get_rank(group) if self.enabled else 0
        # NNUE_DP_FORCE_COLLECTIVES=1 keeps the bucketed all-reduce path on even with one rank (rehearses the
        # RCCL + hipGraph interplay on a single-GPU box; a 1-rank all-reduce is the identity)
        self.collectives = self.enabled and (self.world > 1 or os.environ.get("NNUE_DP_FORCE_COLLECTIVES") == "1")
        self.buckets = 2 if os.environ.get("NNUE_DP_BUCKETS", "1") == "2" else 1
        self.backend = dist.get_backend(group) if self.enabled else None

    @property
    def grad_scale(self) -> float:
        return 1.0 / self.world

    def shard(self, global_batch: int) -> slice:
        if global_batch % self.world:
            raise ValueError(f"global batch {global_batch} is not divisible by world size {self.world}")
        per = global_batch // self.world
        return slice(self.rank * per, (self.rank + 1) * per)

    def broadcast(self, flat: torch.Tensor) -> None:
        if self.world > 1:
            dist.broadcast(flat, src=dist.get_global_rank(self.group, 0) if self.group is not None else 0, group=self.group)

    def allreduce_sum(self, flat: torch.Tensor, async_op: bool = False):
        if self.collectives:
            return dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group, async_op=async_op)
        return None

    # ---- sharded update (reduce-scatter the gradient, update one shard per rank, all-gather the parameters): the same
    # wire bytes as the all-reduce, 1/world of the optimizer's memory traffic per rank -- for flat buffers that are
    # bandwidth- rather than latency-sized (the 269 MB of the 224x224 configuration)
    def shard_of(self, flat: torch.Tensor) -> torch.Tensor:
        per = flat.numel() // self.world
        if per * self.world != flat.numel():
            raise ValueError("flat buffer length must be a multiple of the world size (FlatLayout.of(pad_to=...))")
        return flat[self.rank * per:(self.rank + 1) * per]

    def reduce_scatter_sum(self, flat: torch.Tensor, out_shard: torch.Tensor) -> None:
        """out_shard <- this rank's shard of the sum over ranks of `flat`."""
        if not self.collectives:
            out_shard.copy_(self.shard_of(flat))
        elif self.backend == "nccl":
            dist.reduce_scatter_tensor(out_shard, flat, op=dist.ReduceOp.SUM, group=self.group)
        else:  # gloo has no reduce-scatter: all-reduce, keep the own slice (CPU tests / rehearsals only)
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group)
            out_shard.copy_(self.shard_of(flat))

    def all_gather(self, flat_out: torch.Tensor, shard: torch.Tensor) -> None:
        """flat_out <- the ranks' shards side by side (shard may be flat_out's own slice)."""
        if not self.collectives:
            if shard.data_ptr() != self.shard_of(flat_out).data_ptr():
                self.shard_of(flat_out).copy_(shard)
        elif self.backend == "nccl":
            dist.all_gather_into_tensor(flat_out, shard, group=self.group)
        else:
            per = flat_out.numel() // self.world
            parts = [flat_out[r * per:(r + 1) * per] for r in range(self.world)]
            dist.all_gather(parts, shard.clone(), group=self.group)


    def all_gather_chunks(self, chunks: torch.Tensor) -> None:
        """chunks [world][n] (any dtype): row r <- rank r's row; every rank sends its own row in place."""
        if not self.collectives:
            return
        if self.backend == "nccl":
            dist.all_gather_into_tensor(chunks.view(-1), chunks[self.rank], group=self.group)
        else:
            dist.all_gather([chunks[r] for r in range(self.world)], chunks[self.rank].clone(), group=self.group)


class NnueTrainer:
    """Owns the flat buffers and the activation workspace for one (batch, H, W) shape."""

    def __init__(self, model, batch_size: int, image_hw: Tuple[int, int], lr: float, momentum: float = 0.0,
                 weight_decay: float = 0.0, max_grad_norm: float = 0.0, group=None, use_graph: bool = True,
                 input_slots: int = 1, optimizer: str = "sgd", betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 ft_path: Optional[str] = None, label_smoothing: float = 0.0, two_labels: bool = False, weight_clip: float = 0.0,
                 distill_alpha: float = 0.0, distill_temperature: float = 1.0, ema_decay: float = 0.0, ema_warmup: bool = False):
        """ft_path: the FeatureTransformer kernel family, as lib.ft_path's ``mode`` (None: NNUE_FT_PATH decides).
        label_smoothing (F.cross_entropy's, in [0, 1)) and two_labels (a second label and a weight per sample: mixup, CutMix) make
        the classifier step train on soft targets (include/nnue_hip.h, "soft targets"); with both at their defaults the step is
        the plain one, launch for launch.
        weight_clip (0: off; 1.0 is the reference's _clip_weights, nnue.py:528-539): after every optimizer update the table and the
        classifier's weights are clamped to [-weight_clip, weight_clip] inside the launches that apply the update (include/nnue_hip.h,
        "weight clip") -- bit for bit the plain step followed by ``clamp_`` on those four tensors, in every step mode.
        distill_alpha (in [0, 1]) and distill_temperature (> 0): with alpha > 0 the loss is (1 - alpha) times the (soft) cross-entropy
        plus alpha T^2 KL(teacher at T || student at T) (include/nnue_hip.h, "soft targets": the teacher arm) on the teacher logits
        of ``teacher_inputs[s]`` (float32 [B, C] per input slot; ``step(..., teacher_logits=)`` or a loader's teacher fills them).
        With alpha == 0 nothing is allocated and no call changes.
        ema_decay (0: off, nothing is allocated and no call changes; else in (0, 1)): a moving average of every trainable parameter,
        ``flat_ema``, kept by the launches that apply the update (include/nnue_hip.h, "weight average") -- bit for bit the plain step
        plus ``e <- fmaf(omd, w_new - e, e)`` per element with omd = float32(1 - decay); read it through ``ema_state()`` and
        ``ema_weights()``.  ema_warmup: step t (from 0) averages with decay_t = min(ema_decay, (1 + t) / (10 + t))."""
        self._ema_decay = lib.checked_ema_decay(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        if self.ema_warmup and not self._ema_decay:
            raise ValueError("ema_warmup needs ema_decay > 0")
        self._label_smoothing, self.two_labels = _checked_label_smoothing(label_smoothing), bool(two_labels)
        self.distill_alpha, self.distill_temperature = lib.check_distill(distill_alpha, distill_temperature)
        weight_clip = lib.checked_weight_clip(weight_clip)
        lib.load()
        p0 = next(model.parameters())
        if not p0.is_cuda:
            raise lib.NnueHipError("NnueTrainer needs the model on the GPU (no CPU fallback)")
        self.model, self.dev = model, p0.device
        self._hyper = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, max_grad_norm=max_grad_norm, weight_clip=weight_clip)
        if optimizer not in ("sgd", "adam"):
            raise ValueError(f"optimizer must be 'sgd' or 'adam', got {optimizer!r}")
        self.optimizer, self.betas, self.eps = optimizer, betas, eps
        self.dp = DataParallel(group)
        self.B, (self.H, self.W) = batch_size, image_hw
        self.stride = int(model.conv.stride[0])
        self.fps = model.conv.out_channels
        self.F, self.L1 = model.input.weight.shape
        lin = model.classifier._linears()
        self.L2, self.L3, self.C = lin[0].out_features, lin[1].out_features, lin[2].out_features
        # bucketed layer stacks (BASELINE configs[2]): stacked [K, out, in] classifier parameters, one stack per sample
        self.K = int(getattr(model, "num_ls_buckets", 1))
        self.clip = float(model.classifier.clip_activations or 0.0)
        self.gh, self.gw = lib.conv_out_hw(self.H, self.W, self.stride)
        self.P = self.fps * self.gh * self.gw

        # ---- flat parameter / gradient / momentum buffers; module parameters become views
        self.layout = FlatLayout.of(model, pad_to=4 * self.dp.world)
        f32 = dict(dtype=torch.float32, device=self.dev)
        state = {k: p.detach() for k, p in model.named_parameters() if k not in SKIP}
        self.flat_params = self.layout.pack(state)
        self.flat_grads = torch.zeros(self.layout.count, **f32)
        self.flat_momentum = torch.zeros(self.layout.count, **f32) if (momentum and optimizer == "sgd") else None
        # Adam state (torch.optim.Adam semantics); the step number lives on the device so the update graph replays
        self.flat_exp_avg = torch.zeros(self.layout.count, **f32) if optimizer == "adam" else None
        self.flat_exp_avg_sq = torch.zeros(self.layout.count, **f32) if optimizer == "adam" else None
        self.adam_step_count = torch.zeros(1, dtype=torch.int32, device=self.dev) if optimizer == "adam" else None
        self.dp.broadcast(self.flat_params)  # identical replicas even if ranks were seeded differently
        # the weight average: a clone of the (broadcast) parameters; its rate lives in a device scalar the kernels read, so
        # ``trainer.ema_decay = x`` is one fill and a warm-up moves it per step -- plans and graphs stay valid either way
        self.flat_ema = self.ema_omd_dev = self._ema = self._ema_table = self._ema_spare = None
        self.ema_table = self.ema_pos = None
        self.ema_position = 0
        self._ema_swapped = False  # inside ``ema_weights()``: the live parameters hold the average
        if self._ema_decay:
            self.flat_ema = self.flat_params.clone()
            self.ema_omd_dev = torch.full((1,), lib.ema_omd(self._ema_decay), **f32)
            self._ema = lib.WeightAverage(self.flat_ema, lib.ema_omd(self._ema_decay), self.ema_omd_dev)
            # (the table's own rows of it, for _table_update; the two share the device rate, and _set_ema_decay keeps their omd alike)
            self._ema_table = lib.WeightAverage(self.layout.views(self.flat_ema)["input.weight"], self._ema.omd, self.ema_omd_dev)
            if self.ema_warmup:
                self.ema_table = lib.ema_warmup_table(self._ema_decay).to(self.dev)
                self.ema_pos = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        self.p = self.layout.views(self.flat_params)
        self.g = self.layout.views(self.flat_grads)
        # gradient buckets: [threshold, conv weight] come last out of the backward and lead the flat buffer
        assert self.layout.names[:2] == ["visual_threshold", "conv.weight"]
        self.bucket_split = self.layout.offsets[2]
        self._clip_ranges = clip_ranges(self.layout)  # (built once; the bound is a constant of the update plans)
        for k, prm in model.named_parameters():
            if k not in SKIP:
                prm.data = self.p[k]
                prm.grad = self.g[k]

        # ---- the step mode: every launch decision, resolved once from shape, optimizer, ranks and knobs (step_mode.py)
        B = self.B
        # the table rows the product d_W = A^T d_out covers, as a range of the flat buffers
        tbl_lo = self.layout.offsets[self.layout.names.index("input.weight")]
        tbl_hi = tbl_lo + min(self.F - 1, self.P) * self.L1
        # ``self.mode`` is the one store: MODE_NAMES (below the class) makes its flags readable on the trainer, read-only
        self.mode = step_mode.resolve(
            B=B, H=self.H, W=self.W, stride=self.stride, fps=self.fps, F=self.F, L1=self.L1, L2=self.L2, L3=self.L3, C=self.C,
            K=self.K, optimizer=optimizer, dp=step_mode.DpFacts(self.dp.collectives, self.dp.world, self.dp.buckets, self.dp.backend),
            use_graph=use_graph, lead_names=self.layout.names[:3], tbl_lo=tbl_lo, tbl_hi=tbl_hi, count=self.layout.count, ft_path=ft_path)
        # the two names that are not the mode's: capture_collectives is run-time state (a failed capture clears it, the mode gives
        # its start), and ``val_planes`` further down is the plane BUFFER (the flag is ``self.mode.val_planes``)
        self.capture_collectives = self.mode.capture_collectives

        # ---- static activations and scratch, allocated from the mode
        # input ring: a loader fills slot k while slot k-1 trains; kernels read the slots in place
        self.inputs = [(torch.empty((B, 3, self.H, self.W), **f32), torch.empty((B,), dtype=torch.int64, device=self.dev))
                       for _ in range(max(1, input_slots))]
        self.images, self.labels = self.inputs[0]
        # two_labels: per slot the second labels and the weights of the first ones (-1 / 1: one label per sample)
        self.soft_inputs = None
        self.labels_b = self.lam = None
        if self.two_labels:
            self.soft_inputs = [(torch.full((B,), -1, dtype=torch.int64, device=self.dev), torch.ones((B,), **f32))
                                for _ in self.inputs]
            self.labels_b, self.lam = self.soft_inputs[0]
        # distill_alpha > 0: per slot the teacher's logits (a padding row is never read into a result: its label is -1)
        self.teacher_inputs = self.teacher = None
        if self.distill_alpha > 0.0:
            self.teacher_inputs = [torch.zeros((B, self.C), **f32) for _ in self.inputs]
            self.teacher = self.teacher_inputs[0]
        self.conv_out = torch.empty((B, self.fps, self.gh, self.gw), **f32)
        # the live map of the step, in the mode's kernel family (``fm`` / ``bits`` / ``act`` name it by family)
        self.feats = lib.FT_FAMILIES[self.mode.ft_path].empty(B, self.P, self.F, self.L1, self.dev)
        self.patches = torch.empty((27, B * self.gh * self.gw), **f32) if self.mode.use_patches else None  # the images' im2col form
        self.fx = None
        if self.mode.factor_exchange:
            self.fx = lib.FactorExchange(self.dp.world, self.dp.rank, B, self.P, self.F, self.L1, head=tbl_lo, tail_lo=tbl_hi,
                                         tail=self.layout.count - tbl_hi, device=self.dev)
            self.feats.sink = self.fx.sink  # written by the binarise kernel straight into this rank's chunk
        self.ft = torch.empty((B, self.L1), **f32)
        self.h1 = torch.empty((B, self.L2), **f32)
        self.h2 = torch.empty((B, self.L3), **f32)
        self.logits = torch.empty((B, self.C), **f32)
        self.sample_loss = torch.empty((B,), **f32)
        self.loss = torch.zeros((), **f32)
        self.loss_ring = torch.zeros((max(1, input_slots),), **f32)  # step_many's per-step mean losses
        self.d_logits = torch.empty((B, self.C), **f32)
        self.d_ft = self.fx.d_ft if self.fx is not None else torch.empty((B, self.L1), **f32)  # (the chunk's view: sent in place)
        self.d_conv_out = torch.empty((B, self.P), **f32)
        self.grad_norm = torch.zeros((), **f32)
        u8 = dict(dtype=torch.uint8, device=self.dev)
        self.cls_scratch = torch.empty((max(lib.classifier_scratch_bytes(B, self.L1, self.L2, self.L3, self.K),
                                            lib.classifier_train_scratch_bytes(B, self.L1, self.L2, self.L3, self.C, self.K)),), **u8)
        self.bucket_plan = lib.BucketPlan(B, self.K, self.dev) if self.K > 1 else None
        # the STE launch's own scratch, or the partials the merged backward's ride leaves (fps * 28 outputs, float)
        self.ste_scratch = torch.empty((max(16, lib.load().nnue_ste_conv_backward_scratch(B, self.fps, self.gh, self.gw),
                                            self.fps * 28 * self.mode.ste_chunks * 4 if self.mode.ride_ste else 0),), **u8)
        self.sgd_scratch = torch.empty((lib.sgd_scratch_bytes(self.layout.count),), **u8)
        self.planes = (torch.empty((lib.ftm_forward_planes_bytes(B, self.F, self.P, self.L1),), **u8) if self.mode.fwd_planes else None)
        if self.mode.sharded_update:
            per = self.layout.count // self.dp.world
            self.grad_shard = torch.empty((per,), **f32)
            self.norm_parts = 256
            self.local_partials = torch.empty((self.norm_parts,), **f32)
            self.all_partials = torch.empty((self.norm_parts * self.dp.world,), **f32)
        # the learning rate lives in a device scalar the optimizer kernels read: ``trainer.lr = x`` (a scheduler's hook) is one
        # tiny fill, the recorded plans and captured graphs stay valid (the other hyper-parameters are constants of the plans)
        self.lr_dev = torch.full((1,), float(lr), **f32)
        # a per-step schedule (set_lr_schedule): a device table the step's first optimizer-side launch indexes into lr_dev, its
        # position on the device, and the host's mirrors of both (no read-back anywhere)
        self.lr_table = self.lr_pos = self._lr_values = None
        self.lr_position = 0
        self.steps_done = 0
        self.use_graph = use_graph
        self._g_local, self._g_update = {}, None
        self._plan_local = self._plan_seg = self._plan_update_first = self._plan_update = None
        self._plan_slot = 0
        self._side = torch.cuda.Stream(device=self.dev) if use_graph else None
        # sq_partial: the sums of squares of the table's share (flat_grads[sq_range]) of the clip norm, left by its producer;
        # the Gram form (m.sq == "gram") also takes its scratch and leaves the clip coefficient for the table's update
        self.sq_partial = torch.empty((self.mode.sq_count,), **f32) if self.mode.sq != "none" else None
        self.gram = self.clip_coef = None
        if self.mode.sq == "gram":
            self.gram = torch.zeros((lib.ftm_gram_scratch(self.fx.g_fm if self.mode.factor_exchange else self.feats),), **f32)
            self.clip_coef = torch.ones((), **f32)
        self.val_planes = torch.empty((lib.ftm_value_planes_bytes(B, self.F, self.P, self.L1),), **u8) if self.mode.val_planes else None
        self.fm_alt = lib.FeatureMatrix.empty(B, self.P, self.F, self.L1, self.dev) if self.mode.fuse_next_forward else None
        if self.fm_alt is not None and self.fx is not None:
            self.fm_alt.sink = self.fx.sink  # (both local maps' sink counts live in this rank's chunk: only one of them is live at a time)
        self._last_alt = False  # the last step's map is the second one (an even-length step group)
        self.d_z1 = self.ft_rider = None  # the operands of the merged backward's d_w1 rider, out of the classifier's scratch
        if self.mode.ride_dw1 and self.K == 1:
            off = lib.classifier_train_dz1_offset(B, self.L1, self.L2, self.L3, self.C, True)
            self.d_z1 = self.cls_scratch[off:off + B * self.L2 * 4].view(torch.float32).view(B, self.L2)
            self.ft_rider = self.ft
        elif self.mode.ride_dw1:
            # bucketed stacks: the rider contracts each bucket's own rows, so its operands are the grouped-row copies
            # the classifier's per-sample kernel leaves in the scratch
            rows = self.bucket_plan.tiles * 16
            o_dz, o_x = lib.classifier_train_grouped_offsets(B, self.L1, self.L2, self.L3, self.C, self.K)
            self.d_z1 = self.cls_scratch[o_dz:o_dz + rows * self.L2 * 4].view(torch.float32).view(rows, self.L2)
            self.ft_rider = self.cls_scratch[o_x:o_x + rows * self.L1 * 4].view(torch.float32).view(rows, self.L1)
        self._riders = {}  # mean-loss destination -> host struct (kept alive: recorded plans hold pointers to them)

    # ------------------------------------------------------------------ hyper-parameters
    # The learning rate is a device scalar (``lr_dev``) every optimizer kernel reads: changing it costs one fill and keeps
    # every plan and graph -- per-step schedules are fine; with ranks every rank must set the same value.  Momentum, weight
    # decay, the clip norm and the weight clip are constants of the recorded update plan (and of every graph captured from it): changing one
    # re-records that plan and drops the graphs that contain it; the local (forward/backward) plan is untouched.
    # ``trainer.lr = x`` and ``trainer.set_lr(x)`` are the same thing.
    def _set_hyper(self, key: str, value: float) -> None:
        if self._hyper[key] == value:
            return
        if key == "lr":
            self._hyper[key] = value
            self.lr_dev.fill_(value)
            return
        if key == "weight_clip":
            value = lib.checked_weight_clip(value)
        if key == "momentum" and self.optimizer == "sgd" and bool(value) != (self.flat_momentum is not None):
            raise ValueError("momentum cannot be switched on or off after construction (the buffer layout is fixed)")
        self._hyper[key] = value
        self._drop_update_plans()

    def _drop_update_plans(self) -> None:
        """The update plans are re-recorded at the next step and every graph that contains an update is dropped; the local
        plan and the graphs of the local step alone stay."""
        self._plan_update_first = self._plan_update = None
        self._g_update = None
        for key_ in [k for k in self._g_local if k[1] in step_mode.UPDATE_GRAPH_KINDS]:
            del self._g_local[key_]

    def _get_lr(self) -> float:
        if self._lr_values is not None:  # the value the next step will use
            return float(self._lr_values[min(self.lr_position, self._lr_values.numel() - 1)])
        return self._hyper["lr"]

    def _assign_lr(self, value: float) -> None:
        if self._lr_values is not None:
            raise ValueError("a learning-rate schedule is attached and would overwrite this value at the next step: "
                             "clear the schedule first (clear_lr_schedule)")
        self._set_hyper("lr", float(value))

    lr = property(_get_lr, _assign_lr)
    lr_last = property(lambda self: self._hyper["lr"], doc="the rate lr_dev holds: under a schedule, the last step's")
    momentum = property(lambda self: self._hyper["momentum"], lambda self, v: self._set_hyper("momentum", float(v)))
    weight_decay = property(lambda self: self._hyper["weight_decay"], lambda self, v: self._set_hyper("weight_decay", float(v)))
    max_grad_norm = property(lambda self: self._hyper["max_grad_norm"], lambda self, v: self._set_hyper("max_grad_norm", float(v)))
    weight_clip = property(lambda self: self._hyper["weight_clip"], lambda self, v: self._set_hyper("weight_clip", float(v)))

    # The weight average's decay: its rate omd = float32(1 - decay) is a device scalar (``ema_omd_dev``) like the learning rate, so
    # a change costs one fill and keeps every plan and graph.  Under a warm-up the rate comes from a per-step table instead: a new
    # decay makes a new table and re-records the update plans, as a new learning-rate schedule does.  The average cannot be
    # switched on or off after construction (its buffer is an argument of the recorded calls).
    def _set_ema_decay(self, value: float) -> None:
        value = lib.checked_ema_decay(value)
        if bool(value) != (self.flat_ema is not None):
            raise ValueError("the weight average cannot be switched on or off after construction")
        if value == self._ema_decay:
            return
        self._ema_decay = value
        self._ema.omd = self._ema_table.omd = lib.ema_omd(value)
        if self.ema_table is None:
            self.ema_omd_dev.fill_(self._ema.omd)
        else:  # (ema_omd_dev keeps the last step's rate; the next step's comes out of the new table at the same position)
            self.ema_table = lib.ema_warmup_table(value).to(self.dev)
            self._drop_update_plans()

    ema_decay = property(lambda self: self._ema_decay, _set_ema_decay)

    def _flat_ema(self, lo: int = 0, hi: Optional[int] = None) -> Optional[lib.WeightAverage]:
        """The weight average as the flat optimizer calls take it, or None when it is off; [lo, hi): the slice of the flat
        buffers the call covers (the sharded update's shard)."""
        if self._ema is None:
            return None
        return self._ema if hi is None else self._ema.window(lo, hi)

    def _ema_tick(self) -> None:
        """The warm-up's launch of one optimizer step, beside _lr_tick: this step's rate out of the table into ema_omd_dev."""
        if self.ema_table is not None:
            lib.lr_schedule_step(self.ema_table, self.ema_pos, self.ema_omd_dev)

    def _flat_clip(self, lo: int = 0, hi: Optional[int] = None) -> Optional[lib.WeightClip]:
        """The weight clip as the flat optimizer calls take it, or None when it is off; [lo, hi): the slice of the flat buffers
        the call covers (the sharded update's shard)."""
        if not self.weight_clip:
            return None
        clip = lib.WeightClip(self.weight_clip, self._clip_ranges)
        return clip if hi is None else clip.window(lo, hi)

    # Label smoothing is a constant of the recorded LOCAL plan (an argument of the classifier step): changing it re-records that
    # plan and drops every graph of the local step; the update plans are untouched.
    def _set_label_smoothing(self, value: float) -> None:
        value = _checked_label_smoothing(value)
        if value == self._label_smoothing:
            return
        self._label_smoothing = value
        self._plan_local = self._plan_seg = None
        self._g_local.clear()

    label_smoothing = property(lambda self: self._label_smoothing, _set_label_smoothing)

    def set_lr(self, lr: float) -> None:
        """Learning rate for the following steps (a scheduler's hook)."""
        self.lr = lr

    # A per-step schedule (the reference's get_lr, training_utils.py:283-336, tabulated by lr_schedule.LrSchedule -- or any
    # other table): one tiny launch at the head of every step's optimizer side copies the step's value into ``lr_dev`` and moves
    # the position on.  The launch is part of the recorded plans, hence inside every captured graph: a step group replays
    # with a different rate per step.  With ranks every rank attaches the same values; the counters advance alike without
    # any communication.  Attaching, replacing or clearing re-records the update plans like a change of momentum.
    def set_lr_schedule(self, values, position: int = 0) -> None:
        """Optimizer step number t, counted from position 0, uses ``values[min(t, len - 1)]``; the next step is number
        ``position``."""
        values, position = _checked_schedule(values, position)
        self._lr_values = values.clone()
        self.lr_table = values.to(self.dev)
        self.lr_pos = torch.full((1,), position, dtype=torch.int32, device=self.dev)
        self.lr_position = position
        self._drop_update_plans()

    def clear_lr_schedule(self) -> None:
        """Detaches the schedule; the rate stays at the last value used (``trainer.lr`` reads and sets it again)."""
        if self._lr_values is None:
            return
        self.lr_table = self.lr_pos = self._lr_values = None
        self.lr_position = 0
        self._drop_update_plans()

    def _lr_tick(self) -> None:
        """The schedule's launch of one optimizer step: called once per step, ahead of the first launch that reads lr_dev
        (_small_update and the sharded update's own optimizer call are the two places a step's optimizer side begins)."""
        if self.lr_table is not None:
            lib.lr_schedule_step(self.lr_table, self.lr_pos, self.lr_dev)

    def _advance(self, steps: int) -> None:
        """The host's count of optimizer steps, and the schedule's mirrors with it (lr_position; _hyper['lr'] = what lr_dev
        now holds)."""
        self.steps_done += steps
        if self.ema_table is not None:
            self.ema_position = min(self.ema_position + steps, 2**31 - 1)
        if self._lr_values is not None:
            self.lr_position = min(self.lr_position + steps, 2**31 - 1)
            self._hyper["lr"] = float(self._lr_values[min(self.lr_position - 1, self._lr_values.numel() - 1)])

    # ------------------------------------------------------------------ kernel sequences
    def _cls_params(self):
        p = self.p
        return [p[f"classifier.classifier.{i}.{n}"] for i in (0, 2, 4) for n in ("weight", "bias")]

    def _cls_grads(self):
        return tuple(self.g[f"classifier.classifier.{i}.{n}"] for i in (0, 2, 4) for n in ("weight", "bias"))

    # The step is cut into segments so that a captured graph can run the ones nothing waits for beside the
    # critical path (conv -> bits -> FT forward -> classifier activations/d_x -> value gradient -> STE):
    #   front      conv, per-sample bit masks + forward tile lists                       main
    #   transpose  transposed masks + backward tile lists (only the FT weight gradient reads them)   side 1
    #   forward    FT forward, classifier phase 1 (activations, loss per sample, d_ft)  main
    #   ft_wgrad   FT weight/bias gradient                                              side 1
    #   cls_wgrad  classifier weight/bias gradients + mean loss                         side 2
    #   tail       FT value gradient -> d(conv_out) -> threshold / conv-weight gradients main  (bucket "b")
    SEGMENTS = ("front", "transpose", "forward", "ft_wgrad", "cls_wgrad", "tail")

    def _cls_step(self, phases: int) -> None:
        soft = (self.labels_b, self.lam, self._label_smoothing) if (self.two_labels or self._label_smoothing != 0.0) else None
        distill = (self.teacher, self.distill_alpha, self.distill_temperature) if self.distill_alpha > 0.0 else None
        lib.classifier_train_step(self.ft, True, *self._cls_params(), self.labels, 1.0, self.clip, scratch=self.cls_scratch,
                                  out=(self.h1, self.h2, self.logits), loss_out=(self.sample_loss, self.loss),
                                  grads=self._cls_grads(), d_x=self.d_ft, phases=phases, buckets=self.bucket_plan, soft=soft,
                                  distill=distill)

    def _rider(self, loss: torch.Tensor):
        """The small-gradient tile family's arguments with `loss` as the mean loss's destination (one host struct per
        destination: step_many gives every step of a group its own)."""
        key = loss.data_ptr()
        if key not in self._riders:
            self._riders[key] = lib.classifier_train_rider(True, self.B, self.L1, self.L2, self.L3, self.C, self.h1, self.h2,
                                                           self.sample_loss, loss, self._cls_grads(), self.cls_scratch, self.bucket_plan)
        return self._riders[key]

    def _segment(self, name: str) -> None:
        """The branches here are the launches only the product family has (plane riders, fused layer 1, merged backward, Gram
        norm / table update, factor exchange: the mode has them on that family alone); everything else is the live map's own
        member, whatever its family."""
        p, g, feats = self.p, self.g, self.feats
        if name == "front":
            if self.mode.conv_planes:  # conv + {0,1} map + counts, and the table's bf16 planes from the same launch's riders
                lib.ftm_conv_binarize_planes(self.images, p["conv.weight"], p["visual_threshold"], self.stride, p["input.weight"], self.L2,
                                             self.planes, conv_out=self.conv_out, fm=feats, val_planes=self.val_planes)
            else:  # the product family: one launch; the gather families: conv, then the per-sample half of their binarise
                feats.front(self.images, p["conv.weight"], p["visual_threshold"], self.stride, self.conv_out, patches=self.patches)
        elif name == "transpose":  # (the bit family's transposed masks; nothing in the other two)
            feats.binarize(self.conv_out, p["visual_threshold"], stages=2)
        elif name == "forward":
            if self.mode.fuse_l1:
                # the forward's epilogue also forms the classifier's layer-1 slabs (start of its scratch)
                if self.mode.fwd_planes:
                    lib.ftm_forward_l1_planes(p["input.weight"], p["input.bias"], feats, self.planes, p["classifier.classifier.0.weight"],
                                              self.cls_scratch, out=self.ft)
                else:
                    lib.ftm_forward_l1(p["input.weight"], p["input.bias"], feats, p["classifier.classifier.0.weight"], self.cls_scratch,
                                       out=self.ft)
            else:
                # several stacks: the stack of each sample from the counts the binarise kernel just wrote (product family: one
                # extra workgroup of the forward launch; gather families: a launch ahead of it)
                feats.forward(p["input.weight"], p["input.bias"], out=self.ft, group=self.bucket_plan)
            self._cls_step(self.mode.phases)
        elif name == "ft_wgrad":
            if self.mode.factor_exchange:
                # this rank's share of the rows the product does not cover; they travel with the small gradients, the
                # norm and the product wait for the global factors (_exchange_and_update)
                lib.ftm_backward_tail_rows(self.d_ft, feats, g["input.weight"], g["input.bias"])
            elif self.mode.fuse_table_update:
                # rows the product does not cover (bias, clamp-sink row, unreachable rows) + the Gram form of the norm;
                # the product itself is part of the update (_update)
                # (the tail rows' workgroups ride in the Gram product's launch)
                lib.ftm_gram_sqnorm(feats, self.d_ft, self.gram, self.sq_partial, tail=(g["input.weight"], g["input.bias"]))
            elif self.mode.merged_backward_launch:
                # weight gradient, value gradient and tail rows share one launch (independent work, all read d_ft)
                lib.ftm_backward(self.d_ft, p["input.weight"], feats, d_weight=g["input.weight"], d_bias=g["input.bias"],
                                 dst=None if self.mode.ride_ste else self.d_conv_out, ft=self.ft_rider, d_z1=self.d_z1,
                                 d_w1=g["classifier.classifier.0.weight"] if self.mode.ride_dw1 else None, sq_partial=self.sq_partial,
                                 buckets=self.bucket_plan, small=self._rider(self.loss) if self.mode.ride_small else None,
                                 ste=((self.images, self.conv_out, p["visual_threshold"], self.stride, self.ste_scratch, self.patches)
                                      if self.mode.ride_ste else None), val_planes=self.val_planes)
            else:
                feats.backward_weight(self.d_ft, d_weight=g["input.weight"], d_bias=g["input.bias"])
        elif name == "cls_wgrad":
            if not self.mode.ride_dw1:  # else the small gradients already rode in the d_x launch of "forward"
                self._cls_step(lib.CLS_PHASE_SMALL | lib.CLS_DW1_BESIDE_DX)
        elif name == "tail":
            if not self.mode.merged_backward_launch:  # (else d_conv_out came out of the merged launch in "ft_wgrad")
                feats.backward_values(self.d_ft, p["input.weight"], dst=self.d_conv_out)
            if self.mode.ride_ste:
                return  # stage 1 rode in the merged launch ("ft_wgrad"), stage 2 rides in the norm launch
            if self.mode.use_patches:
                lib.ste_conv_backward_patches(self.patches, self.conv_out, p["visual_threshold"], self.d_conv_out, self.gh, self.gw,
                                              d_thr=g["visual_threshold"], d_weight=g["conv.weight"], scratch=self.ste_scratch,
                                              stages=self.mode.ste_stages)
            else:
                lib.ste_conv_backward(self.images, self.conv_out, p["visual_threshold"], self.d_conv_out, self.stride,
                                      d_thr=g["visual_threshold"], d_weight=g["conv.weight"], scratch=self.ste_scratch,
                                      stages=self.mode.ste_stages)
        else:
            raise KeyError(name)

    def _forward(self) -> None:
        for name in ("front", "forward"):
            self._segment(name)

    def _local_step(self) -> None:
        """forward + loss + backward into the flat gradient buffer (every element is overwritten)."""
        for name in self.SEGMENTS:
            self._segment(name)

    def _small_update(self, first: bool, scale: float) -> None:
        """The optimizer's launch on the flat buffers: clip norm + update of every tensor.  Where the table's gradient is never
        materialised (fuse_table_update, factor_exchange) it takes the table's share of the norm from the Gram partials, leaves
        the table's rows alone and the clip coefficient in ``clip_coef`` for _table_update.  It is the first launch of a step that
        reads lr_dev, so the schedule's launch goes ahead of it."""
        self._lr_tick()
        self._ema_tick()
        ext = (self.sq_partial, *self.mode.sq_range) if self.mode.sq != "none" else None
        elsewhere = self.mode.sq == "gram"
        clip = self._flat_clip()  # (the table rows left to _table_update are clamped there)
        ema = self._flat_ema()  # (... and averaged there)
        if self.optimizer == "adam":
            lib.adam_step(self.flat_params, self.flat_grads, self.flat_exp_avg, self.flat_exp_avg_sq, self.adam_step_count,
                          self.lr, self.betas, self.eps, self.weight_decay, self.max_grad_norm, scale, self.grad_norm,
                          self.sgd_scratch, lr_dev=self.lr_dev, ext=ext, coef_out=self.clip_coef, ext_applied_elsewhere=elsewhere, clip=clip,
                          ema=ema)
            return
        ste = ((self.ste_scratch, self.mode.ste_chunks, self.fps, self.g["visual_threshold"], self.g["conv.weight"])
               if self.mode.defer_ste else None)
        lib.sgd_step(self.flat_params, self.flat_grads, self.flat_momentum, self.lr, self.momentum, self.weight_decay,
                     self.max_grad_norm, scale, first, self.grad_norm, self.sgd_scratch, ste=ste, ext=ext,
                     coef_out=self.clip_coef, ext_applied_elsewhere=elsewhere, lr_dev=self.lr_dev, clip=clip, ema=ema)

    def _table_update(self, first: bool, scale: float, d_ft: torch.Tensor, fm, nxt=None) -> None:
        """The product d_W = A^T d_ft (A: map `fm`) with the table's update in its epilogue, after _small_update: SGD on the
        momentum's rows or Adam on the two moments' rows.  nxt: the same pass over the table also forms the FeatureTransformer
        forward of map `nxt` into ``self.ft`` (_next_map has written it; the small update the bias and table row F-1)."""
        lo, hi = self.mode.sq_range
        forward = () if nxt is None else (nxt, self.p["input.bias"], self.ft)
        if self.optimizer == "adam":
            fn = lib.ftm_backward_weight_update_adam if nxt is None else lib.ftm_backward_weight_update_forward_adam
            opt = (self.flat_exp_avg[lo:hi], self.flat_exp_avg_sq[lo:hi], self.clip_coef, self.adam_step_count, self.lr, self.betas,
                   self.eps, self.weight_decay, scale)
        else:
            fn = lib.ftm_backward_weight_update if nxt is None else lib.ftm_backward_weight_update_forward
            mom = self.flat_momentum[lo:hi] if self.flat_momentum is not None else None
            opt = (mom, self.clip_coef, self.lr, self.momentum, self.weight_decay, scale, first)
        fn(d_ft, fm, self.p["input.weight"], *opt, *forward, lr_dev=self.lr_dev, weight_clip=self.weight_clip, ema=self._ema_table)

    def _next_map(self, slot: int, nxt) -> None:
        """conv + {0,1} map of input slot `slot` into map `nxt`, between the two halves of an update that forms the next step's
        forward: it needs the conv weights and thresholds the small update has just written."""
        nxt.front(self.inputs[slot][0], self.p["conv.weight"], self.p["visual_threshold"], self.stride, self.conv_out, patches=self.patches)

    def _update(self, first: bool, grad_scale: Optional[float] = None) -> None:
        scale = self.dp.grad_scale if grad_scale is None else grad_scale
        self._small_update(first, scale)
        if self.mode.fuse_table_update:  # the product runs LAST and applies the table's share
            self._table_update(first, scale, self.d_ft, self.feats)

    def _exchange_and_update(self, first: bool, grad_scale: Optional[float] = None, alt: bool = False,
                             next_slot: Optional[int] = None) -> None:
        """Everything after the local kernels of a data-parallel step, as launches on the current stream: the gradient
        exchange and the optimizer.  Capturable (no host synchronisation).  alt: this step's local map is the second one;
        next_slot (step groups under the factor exchange): the table update also forms the forward of the step on that slot."""
        if self.mode.factor_exchange:
            fx, scale = self.fx, (self.dp.grad_scale if grad_scale is None else grad_scale)
            fx.pack(self.fm_alt if alt else self.feats, self.flat_grads)
            self.dp.all_gather_chunks(fx.chunks)  # the step's one collective
            fx.unpack(self.flat_grads)
            lib.ftm_gram_sqnorm(fx.g_fm, fx.g_dft, self.gram, self.sq_partial)
            self._small_update(first, scale)
            nxt = None if next_slot is None else (self.feats if alt else self.fm_alt)
            if nxt is not None:
                self._next_map(next_slot, nxt)
            self._table_update(first, scale, fx.g_dft, fx.g_fm, nxt)
            return
        if not self.mode.sharded_update:
            self.dp.allreduce_sum(self.flat_grads, async_op=False)
            self._update(first, grad_scale)
            return
        dp = self.dp
        scale = dp.grad_scale if grad_scale is None else grad_scale
        dp.reduce_scatter_sum(self.flat_grads, self.grad_shard)
        lib.sqnorm_partials(self.grad_shard, self.local_partials)
        dp.all_gather(self.all_partials, self.local_partials)  # rank-major, fixed order: every rank forms the identical norm
        mom = dp.shard_of(self.flat_momentum) if self.flat_momentum is not None else None
        self._lr_tick()
        self._ema_tick()
        per = self.grad_shard.numel()
        lib.sgd_step(dp.shard_of(self.flat_params), self.grad_shard, mom, self.lr, self.momentum, self.weight_decay, self.max_grad_norm,
                     scale, first, self.grad_norm, self.sgd_scratch, ext=(self.all_partials, 0, per), lr_dev=self.lr_dev,
                     clip=self._flat_clip(dp.rank * per, (dp.rank + 1) * per), ema=self._flat_ema(dp.rank * per, (dp.rank + 1) * per))
        dp.all_gather(self.flat_params, dp.shard_of(self.flat_params))

    def _ranks_agree(self, ok: bool) -> bool:
        """True only when `ok` holds on EVERY rank (an eager MIN all-reduce; every rank reaches it at the same step).  A step
        graph with the collective inside must exist on all ranks or on none: a rank that replays while another issues the
        eager collective would pair different operations."""
        if self.dp.world <= 1:
            return ok
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=self.dev if self.dp.backend == "nccl" else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.dp.group)
        return bool(int(flag.item()))

    def _gather_momentum_shards(self) -> None:
        """Under the sharded update with more than one rank every rank owns only its shard of the momentum: all-gathers the
        shards into every rank's flat buffer once the stream has finished them.  A COLLECTIVE where the condition holds."""
        if self.mode.sharded_update and self.flat_momentum is not None and self.dp.world > 1 and self.steps_done > 0:
            torch.cuda.current_stream(self.dev).synchronize()
            self.dp.all_gather(self.flat_momentum, self.dp.shard_of(self.flat_momentum))

    def _gather_ema_shards(self) -> None:
        """The same for the weight average: under the sharded update every rank averages its own shard of the parameters, and
        the shards meet only when somebody asks (ema_state, ema_weights, state_dict, rebuilt).  A COLLECTIVE where the condition
        holds."""
        if self.mode.sharded_update and self.flat_ema is not None and self.dp.world > 1 and self.steps_done > 0:
            torch.cuda.current_stream(self.dev).synchronize()
            self.dp.all_gather(self.flat_ema, self.dp.shard_of(self.flat_ema))

    def _optimizer_buffers(self):
        return [t for t in (self.flat_momentum, self.flat_exp_avg, self.flat_exp_avg_sq, self.adam_step_count) if t is not None]

    def _capture(self, fn) -> torch.cuda.CUDAGraph:
        """Captures fn(main_stream) into a graph."""
        graph = torch.cuda.CUDAGraph()
        self._side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self._side):
            # thread_local: the collective's watchdog thread may query events while we capture
            with torch.cuda.graph(graph, stream=self._side, capture_error_mode="thread_local"):
                fn(torch.cuda.current_stream(self.dev))
        torch.cuda.current_stream(self.dev).wait_stream(self._side)
        return graph

    def _capture_agreed(self, key, fn, ring: Optional[torch.Tensor] = None) -> bool:
        """Captures fn(main_stream), a whole step or step group with its exchange inside, into ``_g_local[key]`` (with `ring`, a
        group's loss ring: as (graph, ring)) -- on every rank or on none.  A stack that cannot capture its collectives keeps them
        eager from here on: the key is dropped, ``capture_collectives`` cleared and False returned on ALL ranks.  Without
        collectives there is nobody to agree with and a failed capture raises."""
        captured = True
        try:
            graph = self._capture(fn)
            self._g_local[key] = graph if ring is None else (graph, ring)
        except RuntimeError as exc:
            if not self.dp.collectives:
                raise
            warnings.warn(f"collectives could not be captured into the step graph ({exc}); using the eager collective")
            captured = False
            torch.cuda.synchronize(self.dev)
        if self.dp.collectives and not self._ranks_agree(captured):
            self._g_local.pop(key, None)
            self.capture_collectives = False
            return False
        return True

    def _run_local(self, slot: int, part: str, main: torch.cuda.Stream, timers=None, loss=None, alt: bool = False,
                   forward_done: bool = False) -> None:
        """Launches the local segments of `part` ("all" | "a" | "b") in order on `main`.  `loss`: a device scalar that
        receives the mean loss instead of ``self.loss`` (step_many's per-step results)."""
        seg = lambda name: self._seg_plan(slot, name, loss, alt)  # noqa: E731
        m = main.cuda_stream
        if forward_done:
            # step_many with the next forward fused into the previous step's table update: this step's map and FeatureTransformer
            # output already exist (alt: in the second map)
            assert part == "all"
            lib.run_plan([c for c in seg("forward") if c[0] != "nnue_ftm_forward"], m, timers)
            for name in ("ft_wgrad", "cls_wgrad", "tail"):
                lib.run_plan(seg(name), m, timers)
            return
        if part == "b":
            lib.run_plan(seg("tail"), m, timers)
            return
        for name in ("front", "transpose", "forward", "ft_wgrad", "cls_wgrad"):
            lib.run_plan(seg(name), m, timers)
        if part == "all":
            lib.run_plan(seg("tail"), m, timers)

    def _plans(self, slot: int = 0):
        """Records the three fixed call sequences once (this also executes them once; the update plans are
        recorded on throw-away copies of the buffers' contents, which are restored afterwards).  The local plan is
        recorded on the input slot of the step that triggers it (no other slot is read or written)."""
        if self._plan_local is None:
            self._plan_seg = {}
            self._plan_slot = slot
            self.images, self.labels = self.inputs[slot]
            if self.soft_inputs is not None:
                self.labels_b, self.lam = self.soft_inputs[slot]
            if self.teacher_inputs is not None:
                self.teacher = self.teacher_inputs[slot]
            for name in self.SEGMENTS:
                with lib.record_calls() as calls:
                    self._segment(name)
                self._plan_seg[name] = list(calls)
            self._plan_local = [c for name in self.SEGMENTS for c in self._plan_seg[name]]
        if self._plan_update is None and (self.mode.sharded_update or self.mode.factor_exchange):
            self._plan_update_first = self._plan_update = []  # these modes issue exchange + update themselves (_exchange_and_update)
        if self._plan_update is None:
            live = [self.flat_params, self.flat_grads, self.grad_norm] + self._optimizer_buffers()
            if self.lr_table is not None:  # (recording would otherwise move the schedule two steps)
                live += [self.lr_pos, self.lr_dev]
            if self.flat_ema is not None:
                live += [self.flat_ema, self.ema_omd_dev] + ([self.ema_pos] if self.ema_pos is not None else [])
            keep = [t.clone() for t in live]  # recording executes the updates: put everything back afterwards
            with lib.record_calls() as calls:
                self._update(True)
            self._plan_update_first = list(calls)
            with lib.record_calls() as calls:
                self._update(False)
            self._plan_update = list(calls)
            for t, k in zip(live, keep):
                t.copy_(k)
        return self._plan_local, self._plan_update_first, self._plan_update

    def _alt_swap(self) -> dict:
        """Pointer substitutions that make a recorded call use the second map (fuse_next_forward)."""
        a, b = self.feats, self.fm_alt
        return {a.bits.data_ptr(): b.bits.data_ptr(), a.n.data_ptr(): b.n.data_ptr(), a.sink.data_ptr(): b.sink.data_ptr(),
                a.scratch.data_ptr(): b.scratch.data_ptr()}

    def _seg_plan(self, slot: int, name: str, loss: Optional[torch.Tensor] = None, alt: bool = False):
        """The recorded calls of one segment with the recorded slot's input pointers swapped for `slot`'s (and the mean
        loss's destination for `loss`; `alt`: the map's buffers for the second map's)."""
        src, swap, riders = self._plan_slot, {}, None
        if slot != src:
            held = self.inputs if self.soft_inputs is None else [i + s for i, s in zip(self.inputs, self.soft_inputs)]
            if self.teacher_inputs is not None:
                held = [h + (t,) for h, t in zip(held, self.teacher_inputs)]
            swap.update({a.data_ptr(): b.data_ptr() for a, b in zip(held[src], held[slot])})
        if alt:
            swap.update(self._alt_swap())
        if loss is not None:
            swap[self.loss.data_ptr()] = loss.data_ptr()
            if self.mode.ride_small:  # the mean loss's destination sits inside the rider's host struct: use the struct made for `loss`
                riders = {ctypes.addressof(self._rider(self.loss)): ctypes.pointer(self._rider(loss))}
        return lib.retarget_plan(self._plan_seg[name], swap, riders)

    # ------------------------------------------------------------------ public
    def step(self, images: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None, slot: int = 0,
             timers=None, global_count: Optional[int] = None, labels_b: Optional[torch.Tensor] = None,
             lam: Optional[torch.Tensor] = None, teacher_logits: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One optimizer step on this rank's slice.  Returns the local mean loss (device scalar, no sync).

        A short batch (fewer than the B images the trainer was built for; possibly none on some ranks) is padded; with
        more than one rank pass ``global_count`` = the number of real samples over ALL ranks in this step (the loader knows
        it), so that every rank scales the summed gradient by B / global_count -- the exact mean over the real samples.

        ``images``/``labels`` are copied into input slot ``slot`` first; pass None to train on what the slot
        already holds (zero-copy: fill ``trainer.inputs[slot]`` directly).  With ``timers`` ({C entry point:
        list}) the step runs eagerly from the recorded plan and brackets the named calls with HIP events on the
        launch stream (bench.py's per-kernel durations).

        ``labels_b``/``lam`` (a trainer built with two_labels; both or neither, beside ``images``): the second labels and the
        weights of the first ones, copied into ``soft_inputs[slot]`` and padded with -1 / 1 the way labels are padded.  Without
        them a copied batch has one label per sample.

        ``teacher_logits`` (a trainer built with distill_alpha > 0, which needs them beside every copied batch; float32 [n, C]):
        the teacher's logits for ``images``, copied into ``teacher_inputs[slot]``; the rows behind a short batch are zeroed and,
        their labels being -1, do not count."""
        self._not_swapped()
        ragged = self._stage(slot, images, labels, labels_b, lam, global_count, teacher_logits)
        _, upd_first, upd = self._plans(slot)
        self._last_alt = False
        first, graphs = self.steps_done == 0, self.use_graph and timers is None
        main = torch.cuda.current_stream(self.dev)
        scale = self.dp.grad_scale * ragged if ragged is not None else None  # (None: the plans' own, dp.grad_scale)

        def form_now():  # (asked again after a capture that the ranks agreed to do without)
            return step_mode.step_form(graphs=graphs, first=first, ragged=ragged is not None, collectives=self.dp.collectives,
                                       buckets=self.dp.buckets, capture_collectives=self.capture_collectives,
                                       own_exchange=self.mode.sharded_update or self.mode.factor_exchange,
                                       async_op=os.environ.get("NNUE_DP_ASYNC_OP") == "1")
        form = form_now()
        if graphs:  # capture everything this step replays before any collective is enqueued
            for part in form.parts:
                if (slot, part) not in self._g_local:
                    self._g_local[(slot, part)] = self._capture(lambda st, part=part: self._run_local(slot, part, st))
            if self._g_update is None and upd:
                self._g_update = self._capture(lambda st: lib.run_plan(upd, st.cuda_stream))
        if form.graph is not None and (slot, form.graph) not in self._g_local:
            def whole_step(st, with_exchange=form.name == "graph_dp"):
                self._run_local(slot, "all", st)
                if with_exchange:
                    self._exchange_and_update(False)
                else:
                    lib.run_plan(upd, st.cuda_stream)
            if not self._capture_agreed((slot, form.graph), whole_step):
                form = form_now()

        def run(part):
            if graphs:
                self._g_local[(slot, part)].replay()
            else:
                self._run_local(slot, part, main, timers=timers)

        if form.graph is not None:  # steady state: ONE graph, one replay per step
            self._g_local[(slot, form.graph)].replay()
        elif form.name == "own_exchange":
            run("all")
            with lib.time_calls(timers):
                self._exchange_and_update(first, grad_scale=scale)
        else:
            if form.name == "two_buckets":
                # big bucket is complete after part a: its all-reduce runs on the collective's own stream while part b
                # (STE/conv backward) still computes; the tail bucket follows part b
                run("a")
                big = self.dp.allreduce_sum(self.flat_grads[self.bucket_split:], async_op=True)
                run("b")
                small = self.dp.allreduce_sum(self.flat_grads[:self.bucket_split], async_op=True)
                big.wait()
                small.wait()
            else:
                run("all")
            if form.name == "one_message":
                # one message: the whole flat gradient buffer, after the local graph; the wait is a stream dependency.
                # A blocking (for the stream, not the host) collective: measured 25 us/step cheaper than async_op + wait()
                # in the 1-rank RCCL rehearsal (0.1395 vs 0.1643 ms); NNUE_DP_ASYNC_OP=1 restores the latter
                work = self.dp.allreduce_sum(self.flat_grads, async_op=form.async_op)
                if form.async_op:
                    work.wait()
            # the update tail of "local", "one_message" and "two_buckets"
            if ragged is not None:
                self._update(first, grad_scale=scale)
            elif first:
                lib.run_plan(upd_first, main.cuda_stream, timers)
            elif graphs:
                self._g_update.replay()
            else:
                lib.run_plan(upd, main.cuda_stream, timers)
        self._advance(1)
        # a short batch's kernels divided by B: the mean over the real samples (a whole-step graph never runs one)
        return self.loss * ragged if ragged is not None else self.loss

    def _stage(self, slot: int, images, labels, labels_b, lam, global_count, teacher_logits=None) -> Optional[float]:
        """Checks step()'s inputs and copies them into input slot `slot`, a short batch padded.  Returns the factor that restores
        the exact mean over the real samples where the kernels divide by B (gradients and loss are scaled by it), else None."""
        buf_images, buf_labels = self.inputs[slot]
        ragged = None
        if (labels_b is None) != (lam is None) or (labels_b is not None and (images is None or not self.two_labels)):
            raise ValueError("labels_b and lam come together, beside images, on a trainer built with two_labels=True")
        if teacher_logits is not None and (images is None or self.teacher_inputs is None):
            raise ValueError("teacher_logits come beside images, on a trainer built with distill_alpha > 0")
        if teacher_logits is None and images is not None and self.teacher_inputs is not None:
            raise ValueError("a trainer built with distill_alpha > 0 needs teacher_logits beside images")
        if images is not None:
            if labels is None or images.shape[1:] != buf_images.shape[1:] or labels.shape[0] != images.shape[0] \
                    or not 0 <= images.shape[0] <= self.B or (images.shape[0] == 0 and self.dp.world == 1):
                raise ValueError(f"trainer was built for images {tuple(buf_images.shape)} / labels ({self.B},)")
            n = images.shape[0]
            if n == self.B:
                buf_images.copy_(images, non_blocking=True)
                buf_labels.copy_(labels, non_blocking=True)
            else:
                # short last batch of an epoch: pad with blank images whose label -1 the loss kernel ignores (zero
                # loss, zero gradient row); the kernels divide by B, the exact mean over the n real samples is
                # restored by scaling gradients and loss with B/n
                if self.dp.world > 1 and global_count is None:
                    raise ValueError("a short batch with more than one rank needs global_count (real samples over all ranks)")
                ragged = self.B / n if self.dp.world == 1 else self.B * self.dp.world / int(global_count)
                buf_images.zero_()
                buf_images[:n].copy_(images, non_blocking=True)
                buf_labels.fill_(-1)
                buf_labels[:n].copy_(labels, non_blocking=True)
            if labels_b is not None and (labels_b.shape != labels.shape or lam.shape != labels.shape):
                raise ValueError(f"labels_b {tuple(labels_b.shape)} and lam {tuple(lam.shape)} must have labels' shape {tuple(labels.shape)}")
            if self.soft_inputs is not None:
                buf_b, buf_lam = self.soft_inputs[slot]
                buf_b.fill_(-1)
                buf_lam.fill_(1.0)
                if labels_b is not None:
                    buf_b[:n].copy_(labels_b, non_blocking=True)
                    buf_lam[:n].copy_(lam, non_blocking=True)
            if teacher_logits is not None:
                if tuple(teacher_logits.shape) != (n, self.C) or teacher_logits.dtype != torch.float32:
                    raise ValueError(f"teacher_logits must be float32 {(n, self.C)}, got {teacher_logits.dtype} {tuple(teacher_logits.shape)}")
                buf_t = self.teacher_inputs[slot]
                if n < self.B:
                    buf_t.zero_()
                buf_t[:n].copy_(teacher_logits, non_blocking=True)
        if ragged is None and global_count is not None and self.dp.world > 1 and int(global_count) != self.B * self.dp.world:
            ragged = self.B * self.dp.world / int(global_count)  # this rank's slot is full but others are short: the same global mean
        return ragged

    def _run_many(self, st: torch.cuda.Stream, slots, ring: torch.Tensor, upd, timers=None) -> None:
        """The launches of ``len(slots)`` consecutive steps on stream `st` (the current stream): what step_many captures, and
        -- with `timers` -- what it runs eagerly with HIP events around the named entry points."""
        fuse = self._group_fuses(slots)
        for i, s in enumerate(slots):
            alt = fuse and i % 2 == 1
            self._run_local(s, "all", st, timers=timers, loss=ring[i], alt=alt, forward_done=fuse and i > 0)
            if self.dp.collectives:
                with lib.time_calls(timers):
                    self._exchange_and_update(False, alt=alt, next_slot=slots[i + 1] if fuse and i + 1 < len(slots) else None)
            elif fuse and i + 1 < len(slots):
                # small tensors (and the clip coefficient) first: the next map needs the updated conv weights and thresholds,
                # the next forward's finish the updated bias and table row F-1
                cur, nxt = (self.fm_alt, self.feats) if alt else (self.feats, self.fm_alt)
                with lib.time_calls(timers):
                    self._small_update(False, self.dp.grad_scale)
                    self._next_map(slots[i + 1], nxt)
                    self._table_update(False, self.dp.grad_scale, self.d_ft, cur, nxt)
            else:
                lib.run_plan(lib.retarget_plan(upd, self._alt_swap() if alt else None), st.cuda_stream, timers)

    def _group_fuses(self, slots) -> bool:
        """In a group on `slots` the table update of every step but the last also forms the next step's forward."""
        return self.mode.fuse_next_forward and len(slots) > 1  # (the mode has it only on a single rank or under the factor exchange)

    def _ends_on_alt(self, slots) -> bool:
        """The last step of a group on `slots` leaves its map in the second one (the maps alternate within a fused group)."""
        return self._group_fuses(slots) and len(slots) % 2 == 0

    def _ring(self, n: int) -> torch.Tensor:
        """The ring of per-step mean losses, grown to at least n entries."""
        if self.loss_ring.numel() < n:
            self.loss_ring = torch.zeros((n,), dtype=torch.float32, device=self.dev)
        return self.loss_ring

    def step_many(self, slots, timers=None) -> torch.Tensor:
        """``len(slots)`` consecutive optimizer steps on what the named input slots already hold (fill
        ``trainer.inputs[s]`` first; a slot may repeat), replayed as ONE hipGraph: the same kernels in the same order as
        ``step(slot=s)`` for each s, without the gap between two graph launches (measured 5 us at the CIFAR batch-512
        configuration, 5 % of its step).  With a big table (``fuse_next_forward``) the table update of every step but the last
        also forms the next step's FeatureTransformer forward -- one pass over the table instead of two, bitwise the same
        results.  Returns the mean loss of every step (device vector, no sync; a view of a ring
        the next call overwrites); ``self.loss`` is not written.  Falls back to single steps while the plans are not recorded yet, without graphs, or with an eager
        collective.  ``timers`` ({C entry point: list}): the same launches issued eagerly with HIP events around the named
        calls (bench.py's per-kernel durations of the group form)."""
        self._not_swapped()
        slots = tuple(int(s) for s in slots)
        if not slots or min(slots) < 0 or max(slots) >= len(self.inputs):
            raise ValueError(f"slots must name input slots 0..{len(self.inputs) - 1}")
        recorded = self.steps_done > 0 and self._plan_local is not None
        one_graph = self.use_graph and recorded and (not self.dp.collectives or self.capture_collectives)
        if timers is not None and recorded:
            # (with ranks: the collectives are issued eagerly, in the same order on every rank)
            _, _, upd = self._plans(slots[0])
            ring = self._ring(len(slots))
            self._run_many(torch.cuda.current_stream(self.dev), slots, ring, upd, timers)
        else:
            if one_graph and (slots, "many") not in self._g_local:
                _, _, upd = self._plans(slots[0])
                ring = self._ring(len(slots))
                one_graph = self._capture_agreed((slots, "many"), lambda st: self._run_many(st, slots, ring, upd), ring)
            if not one_graph:  # single steps: they advance the counters themselves
                ring = self._ring(len(slots))
                for i, s in enumerate(slots):
                    ring[i].copy_(self.step(slot=s), non_blocking=True)
                return ring[:len(slots)]
            graph, ring = self._g_local[(slots, "many")]
            graph.replay()
        self._last_alt = self._ends_on_alt(slots)  # (the maps alternate within a fused group)
        self._advance(len(slots))
        return ring[:len(slots)]

    # ------------------------------------------------------------------ the weight average's surface
    def _not_swapped(self) -> None:
        if self._ema_swapped:
            raise RuntimeError("a step inside ema_weights(): the live parameters hold the average; leave the context first")

    def ema_state(self) -> Dict[str, torch.Tensor]:
        """The averaged parameters, name -> view of ``flat_ema``, under the keys ``model.state_dict()`` has for them (nnue2score,
        which never trains, is not averaged).  A COLLECTIVE under the sharded update with more than one rank: the shards are
        gathered first."""
        if self.flat_ema is None:
            raise ValueError("this trainer keeps no weight average (ema_decay = 0)")
        self._gather_ema_shards()
        return self.layout.views(self.flat_ema)

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the model's live parameters hold the averaged values -- ``evaluate``, ``model(images)``,
        ``serialize_model``, ``EngineModel.from_model`` and ``requantize`` see the averaged network unchanged; on exit the exact
        bits of the trained parameters are back (a spare buffer, allocated on first use, keeps them).  No step may be taken
        inside.  A COLLECTIVE where ema_state() is one."""
        if self.flat_ema is None:
            raise ValueError("this trainer keeps no weight average (ema_decay = 0)")
        self._not_swapped()
        self._gather_ema_shards()
        if self._ema_spare is None:
            self._ema_spare = torch.empty_like(self.flat_params)
        self._ema_spare.copy_(self.flat_params)
        self.flat_params.copy_(self.flat_ema)
        self._ema_swapped = True
        try:
            yield self
        finally:
            self.flat_params.copy_(self._ema_spare)
            self._ema_swapped = False

    def rebuilt(self, ft_path: str) -> "NnueTrainer":
        """A trainer for the same model, shapes, hyper-parameters and optimizer state that uses another FeatureTransformer
        kernel family (``"mfma"`` | ``"bits"`` | ``"list"`` | ``"auto"``: the constructor's ``ft_path``) -- the train loop's density check
        calls this at an epoch boundary when the learnable thresholds have moved the active-feature density across the
        measured crossover of the dense-product and gather forms.  This trainer must not be used afterwards (the module's
        parameters become views of the new trainer's buffers)."""
        torch.cuda.synchronize(self.dev)
        new = NnueTrainer(self.model, self.B, (self.H, self.W), group=self.dp.group, use_graph=self.use_graph, input_slots=len(self.inputs),
                          optimizer=self.optimizer, betas=self.betas, eps=self.eps, ft_path=ft_path, label_smoothing=self._label_smoothing,
                          two_labels=self.two_labels, distill_alpha=self.distill_alpha, distill_temperature=self.distill_temperature,
                          ema_decay=self._ema_decay, ema_warmup=self.ema_warmup, **self._hyper)
        self._gather_momentum_shards()
        if self.flat_ema is not None:  # the average, its rate (a warm-up's last one) and the warm-up's position carry over
            self._gather_ema_shards()
            new.flat_ema.copy_(self.flat_ema)
            new.ema_omd_dev.copy_(self.ema_omd_dev)
            if self.ema_pos is not None:
                new.ema_pos.copy_(self.ema_pos)
                new.ema_position = self.ema_position
        for src, dst in zip(self._optimizer_buffers(), new._optimizer_buffers()):
            dst.copy_(src)
        new.steps_done = self.steps_done
        if self._lr_values is not None:  # (lr_dev already holds the last value used: the constructor got _hyper's)
            new.set_lr_schedule(self._lr_values, self.lr_position)
        return new

    # ------------------------------------------------------------------ run state (checkpoint / resume)
    def state_dict(self) -> dict:
        """Everything the trainer carries from step to step, apart from the model's parameters (``model.state_dict()`` has
        those): tensors, numbers, strings, dicts and lists only, so ``torch.load(..., weights_only=True)`` reads it back.  A
        COLLECTIVE exactly where optimizer_state_dict() is one (sharded update with more than one rank)."""
        schedule = None
        if self._lr_values is not None:
            schedule = {"values": self._lr_values.clone(), "position": int(self.lr_position)}
        ema = None
        if self.flat_ema is not None:
            ema = {"decay": float(self._ema_decay), "warmup": bool(self.ema_warmup), "position": int(self.ema_position),
                   "omd": self.ema_omd_dev.detach().clone(), "state": {k: v.clone() for k, v in self.ema_state().items()}}
        return {"version": 1, "ema": ema, "optimizer_type": self.optimizer, "optimizer": self.optimizer_state_dict(),
                "steps_done": int(self.steps_done), "lr": float(self._hyper["lr"]), "lr_schedule": schedule,
                "label_smoothing": float(self._label_smoothing), "weight_clip": float(self.weight_clip),
                "distill_alpha": float(self.distill_alpha), "distill_temperature": float(self.distill_temperature)}

    def _checked_optimizer_state(self, sd: dict, steps_done: int):
        """The flat-buffer sources of a torch optimizer state dict, {buffer name: {parameter name: tensor}}, after checking
        them against this trainer's optimizer, momentum and layout (ValueError otherwise; nothing is changed here)."""
        if not isinstance(sd, dict) or "state" not in sd:
            raise ValueError("not a torch optimizer state dict (no 'state')")
        index = {k: i for i, (k, _) in enumerate(self.model.named_parameters())}
        state = sd["state"]
        keys = (("exp_avg", "exp_avg_sq") if self.optimizer == "adam" else
                (("momentum_buffer",) if self.flat_momentum is not None else ()))
        out = {key: {} for key in keys}
        if steps_done == 0 and not state:
            return out  # a trainer that has not stepped yet: nothing to restore
        foreign = {"sgd": ("exp_avg", "exp_avg_sq"), "adam": ("momentum_buffer",)}[self.optimizer]
        for k, shape in zip(self.layout.names, self.layout.shapes):
            entry = state.get(index[k], state.get(str(index[k])))
            if entry is None:
                if keys:
                    raise ValueError(f"optimizer state has no entry for parameter {k!r}")
                continue
            if any(f in entry for f in foreign):
                raise ValueError(f"optimizer state of parameter {k!r} belongs to another optimizer type than {self.optimizer!r}")
            if not keys and entry.get("momentum_buffer") is not None:
                raise ValueError("the state has momentum buffers but this trainer was built without momentum")
            for key in keys:
                t = entry.get(key)
                if not torch.is_tensor(t):
                    raise ValueError(f"optimizer state of parameter {k!r} has no {key!r}"
                                     + (" (momentum missing)" if key == "momentum_buffer" else ""))
                if tuple(t.shape) != tuple(shape):
                    raise ValueError(f"{key} of {k!r}: shape {tuple(t.shape)} does not match the layout's {tuple(shape)}")
                out[key][k] = t
        return out

    def load_optimizer_state_dict(self, sd: dict, steps_done: int) -> None:
        """Restores the optimizer state from a torch optimizer state dict (optimizer_state_dict()'s format: the
        ``optimizer_state_dict`` of a ``best-model.ckpt``) IN PLACE, and the step count with it: no buffer is re-bound, so
        recorded plans and captured graphs stay valid.  Validates first; on ValueError nothing has changed."""
        steps_done = int(steps_done)
        if steps_done < 0:
            raise ValueError(f"steps_done = {steps_done} must not be negative")
        self._apply_optimizer_state(self._checked_optimizer_state(sd, steps_done), steps_done)

    def _apply_optimizer_state(self, sources: dict, steps_done: int) -> None:
        flats = {"momentum_buffer": self.flat_momentum, "exp_avg": self.flat_exp_avg, "exp_avg_sq": self.flat_exp_avg_sq}
        for key, tensors in sources.items():
            if not tensors:  # (a state taken before the first step: the buffers' initial zeros)
                flats[key].zero_()
                continue
            for k, v in self.layout.views(flats[key]).items():
                v.copy_(tensors[k])
        if self.adam_step_count is not None:
            self.adam_step_count.fill_(steps_done)
        # with steps_done > 0 the momentum-initialising first-step plan never runs again (step() reads steps_done)
        self.steps_done = steps_done
        self._last_alt = False

    def load_state_dict(self, sd: dict) -> None:
        """state_dict()'s counterpart, on a fresh trainer or on a used one between steps.  Validates first (optimizer type,
        presence of momentum, every tensor's shape against the layout, the label smoothing and the weight clip the state was trained
        with -- a state without either key counts as 0 -- and its distill_alpha / distill_temperature -- 0 and 1 without the keys;
        ValueError, nothing changed), then copies in place: the
        momentum or both moments into the flat buffers, Adam's step into adam_step_count, the rate into lr_dev, the schedule's
        values and position into lr_table / lr_pos / lr_position, and steps_done.  No buffer is re-bound -- recorded plans and
        captured graphs hold raw pointers and stay valid; only a schedule of another length than the attached one (or a
        schedule where none is attached, or none where one is) goes through set_lr_schedule / clear_lr_schedule and their
        rules.  The model's parameters are not in this dict: ``model.load_state_dict`` restores them, in place too."""
        if not isinstance(sd, dict) or sd.get("version") != 1:
            raise ValueError("not a trainer state dict of version 1")
        if sd.get("optimizer_type") != self.optimizer:
            raise ValueError(f"the state is of optimizer type {sd.get('optimizer_type')!r}, this trainer's is {self.optimizer!r}")
        steps_done = int(sd["steps_done"])
        if steps_done < 0:
            raise ValueError(f"steps_done = {steps_done} must not be negative")
        sources = self._checked_optimizer_state(sd["optimizer"], steps_done)
        schedule = sd.get("lr_schedule")
        if schedule is not None:
            values, position = _checked_schedule(schedule["values"], schedule["position"])
        lr = float(sd["lr"])
        if float(sd.get("label_smoothing", 0.0)) != self._label_smoothing:  # (a state from before the key existed: 0)
            raise ValueError(f"the state was trained with label_smoothing = {float(sd.get('label_smoothing', 0.0))}, "
                             f"this trainer's is {self._label_smoothing}")
        if float(sd.get("weight_clip", 0.0)) != self.weight_clip:  # (a state from before the key existed: 0)
            raise ValueError(f"the state was trained with weight_clip = {float(sd.get('weight_clip', 0.0))}, "
                             f"this trainer's is {self.weight_clip}")
        held = (float(sd.get("distill_alpha", 0.0)), float(sd.get("distill_temperature", 1.0)))  # (before the keys existed: 0, 1)
        if held != (self.distill_alpha, self.distill_temperature):
            raise ValueError(f"the state was trained with distill_alpha = {held[0]}, distill_temperature = {held[1]}, "
                             f"this trainer's are {self.distill_alpha}, {self.distill_temperature}")
        ema = sd.get("ema")  # (a state from before the key existed, or of a trainer without the average: None)
        if (ema is None) != (self.flat_ema is None):
            raise ValueError("the state " + ("has no" if ema is None else "carries a") + " weight average, this trainer "
                             + ("keeps one" if ema is None else "keeps none") + f" (ema_decay = {self._ema_decay})")
        if ema is not None:
            if float(ema["decay"]) != self._ema_decay or bool(ema["warmup"]) != self.ema_warmup:
                raise ValueError(f"the state's weight average has ema_decay = {float(ema['decay'])}, ema_warmup = {bool(ema['warmup'])}, "
                                 f"this trainer's are {self._ema_decay}, {self.ema_warmup}")
            if not 0 <= int(ema["position"]) <= 2**31 - 1:
                raise ValueError(f"the weight average's warm-up position {int(ema['position'])} must lie in 0 .. 2^31 - 1")
            for k, shape in zip(self.layout.names, self.layout.shapes):
                t = ema["state"].get(k)
                if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
                    raise ValueError(f"the state's weight average has no tensor of shape {tuple(shape)} for {k!r}")
            if tuple(torch.as_tensor(ema["omd"]).shape) != (1,):
                raise ValueError("the state's weight average has no rate ('omd': one float32)")
        # ---- validated: from here on only in-place copies
        self._apply_optimizer_state(sources, steps_done)
        if ema is not None:
            for k, v in self.layout.views(self.flat_ema).items():
                v.copy_(ema["state"][k])
            self.ema_omd_dev.copy_(torch.as_tensor(ema["omd"], dtype=torch.float32))
            if self.ema_pos is not None:
                self.ema_position = int(ema["position"])
                self.ema_pos.fill_(self.ema_position)
        if schedule is None:
            self.clear_lr_schedule()
        elif self._lr_values is None or self._lr_values.numel() != values.numel():
            self.set_lr_schedule(values, position)
        else:
            self._lr_values.copy_(values)
            self.lr_table.copy_(values)
            self.lr_pos.fill_(position)
            self.lr_position = position
        self._hyper["lr"] = lr
        self.lr_dev.fill_(lr)

    def optimizer_state_dict(self) -> dict:
        """The optimizer state in torch.optim's own state_dict format (SGD momentum buffers, or Adam's step /
        exp_avg / exp_avg_sq), indexed like ``model.parameters()`` -- what checkpoint_manager.py:45-51 stores and
        ``optimizer.load_state_dict`` (checkpoint_manager.py:75-85) expects.

        With the sharded update (more than one rank, bandwidth-sized buffers) every rank owns only its shard of the
        momentum, so this call first all-gathers the shards: it is then a COLLECTIVE and every rank must make it (the
        train loop does: all ranks reach the same best-F1 decision)."""
        self._gather_momentum_shards()
        params = list(self.model.parameters())
        if self.optimizer == "adam":
            opt = torch.optim.Adam(params, lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay)
        else:
            opt = torch.optim.SGD(params, lr=self.lr, momentum=self.momentum, weight_decay=self.weight_decay)
        sd = opt.state_dict()
        if self.steps_done == 0:
            return sd
        index = {k: i for i, (k, _) in enumerate(self.model.named_parameters())}
        for k in self.layout.names:
            if self.optimizer == "adam":
                sd["state"][index[k]] = {"step": torch.tensor(float(self.steps_done)),
                                         "exp_avg": self.layout.views(self.flat_exp_avg)[k].clone(),
                                         "exp_avg_sq": self.layout.views(self.flat_exp_avg_sq)[k].clone()}
            elif self.flat_momentum is not None:
                sd["state"][index[k]] = {"momentum_buffer": self.layout.views(self.flat_momentum)[k].clone()}
        return sd

    @torch.no_grad()
    def evaluate(self, images: torch.Tensor) -> torch.Tensor:
        """Forward only on a full-size batch; returns logits (a view of the static buffer)."""
        self.images.copy_(images, non_blocking=True)  # the slot the eager segments read (slot 0 unless a plan was recorded elsewhere)
        self._forward()
        return self.logits

    def active_stats(self) -> Tuple[float, int]:
        """(mean, max) active features per image of the last batch -- reads back; not for timed regions."""
        n = (self.fm_alt if self._last_alt else self.feats).n.float()  # (_last_alt: only where the mode has the second map)
        return float(n.mean()), int(n.max())


# The mode's flags as read-only attributes of the trainer (bench.py and the tests read them there): ``self.mode`` is the only
# store, so an assignment to one of these names raises instead of leaving the two views apart.
MODE_NAMES = ("ft_path", "use_mfma", "use_bits", "use_patches", "fuse_l1", "fwd_planes", "merge_backward", "ride_dw1", "ride_small",
              "fuse_tail_dx", "defer_ste", "ride_ste", "ste_chunks", "fuse_table_update", "fuse_next_forward", "grads_materialised",
              "factor_exchange", "sharded_update", "sq_range")
for _name in MODE_NAMES:
    setattr(NnueTrainer, _name, property(lambda self, _name=_name: getattr(self.mode, _name)))
# the live map under its family's name (None for the other two families)
for _name, _family in (("fm", "mfma"), ("bits", "bits"), ("act", "list")):
    setattr(NnueTrainer, _name, property(lambda self, _family=_family: self.feats if self.feats.family == _family else None))
