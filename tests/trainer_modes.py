"""The step modes NnueTrainer resolves to (nnue_hip/step_mode.py::resolve, consumed by nnue_hip/trainer.py), as a table of
named configurations with the mode each one must take, and the driver that holds a whole optimizer step in that mode to the
float64 oracle (oracle.loss_and_grads_explicit + oracle.sgd_step / oracle.adam_step).  A helper, not a test module:
tests/test_trainer_modes_policy.py holds the trainer's own resolver to the table on any machine (it is launch-free),
tests/test_gpu_trainer_modes.py runs every row on the GPU.  The bars are written once, in ``compare_held``, over plain tensors:
``check_step`` applies them to a single-rank trainer, tests/dp_modes.py to each rank of a process group.

A mode is the dict ``A_MODES`` shows: the trainer's flags, where the table's share of the clip norm comes from (``sq``: the
weight-gradient tiles, the Gram product, or nowhere: the optimizer reads the rows), the classifier's phase mask of the forward
segment, the ``stages`` of the STE launch (None: it rides in the merged backward) and -- derived from those by ``launches_of``
-- the ordered C entry points of one steady-state step.

NNUE_FTM_SPLIT_BACKWARD and NNUE_FTM_RIDE_STE_V64 are read once per process by the C side and cannot be switched inside one
test process: ``merge_backward`` is part of the mode but takes one value only.
"""
import contextlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

# every environment variable the resolution reads, in the trainer or behind the launch-free queries: a row clears all of them
# before it sets its own
KNOBS = ("NNUE_FT_PATH", "NNUE_CONV_PATCHES", "NNUE_DEFER_STE", "NNUE_FUSE_L1", "NNUE_FTM_FWD_PLANES", "NNUE_FTM_SPLIT_BACKWARD",
         "NNUE_FTM_RIDE_DW1", "NNUE_FUSE_TABLE_UPDATE", "NNUE_NORM_PARTIALS", "NNUE_FTM_RIDE_STE", "NNUE_FTM_VAL_PLANES",
         "NNUE_FUSE_NEXT_FORWARD", "NNUE_CLS_RIDE_SMALL", "NNUE_CLS_FUSE_TAIL_DX", "NNUE_FTM_VAL_PLANES_MIN_TILES",
         "NNUE_FTM_FWD_PLANES_MIN_WG", "NNUE_FTM_FWD_STREAM", "NNUE_FTM_BF16", "NNUE_FTM_BF_BM", "NNUE_FTM_BF_WM",
         "NNUE_FTM_RIDE_STE_V64", "NNUE_CLS_FWD_KSPLIT", "NNUE_SGD_SCALAR", "NNUE_DP_FORCE_COLLECTIVES", "NNUE_DP_BUCKETS",
         "NNUE_DP_FACTOR_EXCHANGE", "NNUE_DP_SHARDED_UPDATE", "NNUE_DP_CAPTURE")

# base "A": the CIFAR map (11 x 11 positions of 8 features over a 10 x 10 table: P 968, F 800, a clamp sink) at batch 200
A = dict(grid=10, fps=8, image=32, l1=256, l2=32, l3=16, classes=10, batch=200, K=1, clip=None, optimizer="sgd", momentum=0.9)
A_MODES = dict(ft_path="mfma", use_patches=False, fuse_l1=True, fwd_planes=False, merge_backward=True, ride_dw1=True,
               ride_small=True, fuse_tail_dx=False, defer_ste=True, ride_ste=True, ste_chunks=112, val_planes=False,
               fuse_table_update=False, fuse_next_forward=False, sq="tiles", grouped=False, optimizer="sgd", phases=59,
               ste_launch=None)
FLAGS = ("use_patches", "fuse_l1", "fwd_planes", "ride_dw1", "ride_small", "fuse_tail_dx", "defer_ste", "ride_ste", "val_planes",
         "fuse_table_update", "fuse_next_forward", "grouped")  # (merge_backward: one value per process, see above)
PHASES = (5, 13, 19, 27, 51, 59, 123)

SGD = dict(lr=0.01, weight_decay=2e-4)   # tests/test_gpu_step_shapes.py::OPT (momentum: the row's)
ADAM = dict(lr=1e-3, weight_decay=2e-4)  # tests/test_gpu_adam_table_update.py, the 224x224 group
SHORT = 13  # rows the short last batch lacks


@dataclass
class Row:
    name: str
    cfg: Dict = field(default_factory=dict)     # over A
    env: Dict = field(default_factory=dict)
    expect: Dict = field(default_factory=dict)  # over A_MODES
    # every kernel of the step sums in a fixed order (the only float atomics add small integers), so eager steps, graph steps
    # and step groups are bitwise the same in every row; a row that is not says why here and its graph run is held to the
    # oracle's bars instead
    bitwise: bool = True
    why_not_bitwise: str = ""

    @property
    def config(self) -> Dict:
        return {**A, **self.cfg}

    @property
    def modes(self) -> Dict:
        return {**A_MODES, **self.expect}


G8 = dict(grid=8, image=32)                                  # stride 4: 8 x 8 positions, P = F
G16 = dict(grid=16, image=96, batch=160)                     # stride 6: the images are more than twice their patches
T8192 = dict(grid=32, fps=8, image=96, batch=64)             # an 8192 x 256 table, P = F
BITS = dict(grid=5, fps=3, image=40, batch=40)               # 75 table rows: below the product kernels' shapes
FTU = {"NNUE_FUSE_TABLE_UPDATE": "1"}
NO_RIDE = dict(ride_ste=False, ste_chunks=0, ste_launch=1)   # the STE launch leaves partials, the norm launch finishes them
NO_L1 = dict(fuse_l1=False, phases=51)
GATHER = dict(fuse_l1=False, ride_dw1=False, ride_small=False, ride_ste=False, ste_chunks=0, ste_launch=1, sq="none", phases=5)
GRAM = dict(fuse_table_update=True, sq="gram", ride_dw1=False, ride_small=False, ride_ste=False, ste_chunks=0, ste_launch=1)

ROWS: List[Row] = [
    Row("A"),
    Row("A_planes", env={"NNUE_FTM_VAL_PLANES_MIN_TILES": "1", "NNUE_FTM_FWD_PLANES_MIN_WG": "1"},
        expect=dict(fwd_planes=True, val_planes=True)),
    Row("A_tail_in_dx", cfg=dict(l2=128, l3=32), expect=dict(fuse_tail_dx=True, phases=123)),
    Row("A_adam", cfg=dict(optimizer="adam"), expect=dict(optimizer="adam", defer_ste=False, ride_ste=False, ste_chunks=0,
                                                          ste_launch=3, sq="none")),
    Row("A_k4_clip", cfg=dict(K=4, clip=1.0), expect=dict(grouped=True, **NO_L1)),
    Row("A_k4_adam", cfg=dict(K=4, optimizer="adam"),
        expect=dict(grouped=True, optimizer="adam", defer_ste=False, ride_ste=False, ste_chunks=0, ste_launch=3, sq="none", **NO_L1)),
    Row("A_b96", cfg=dict(batch=96), expect=dict(ste_chunks=48, **NO_L1)),
    Row("A_b37_l1_128", cfg=dict(batch=37, l1=128), expect=dict(ste_chunks=32, **NO_L1)),
    Row("A_l1_192", cfg=dict(l1=192), expect=dict(ride_dw1=False, ride_small=False, phases=13)),
    Row("A_l1_72", cfg=dict(l1=72), expect=dict(fuse_l1=False, ride_dw1=False, ride_small=False, phases=5)),
    Row("A_l2_7", cfg=dict(l2=7, l3=5, classes=3), expect=dict(ride_dw1=False, ride_small=False, phases=13)),
    Row("g8_fps4", cfg=dict(fps=4, **G8), expect=NO_RIDE),
    Row("g8_fps12", cfg=dict(fps=12, **G8), expect=NO_RIDE),
    Row("g4_fps160", cfg=dict(grid=4, fps=160, image=16, l1=128, batch=40),
        expect=dict(defer_ste=False, ride_ste=False, ste_chunks=0, ste_launch=3, **NO_L1)),
    Row("g5_bits", cfg=BITS, expect=dict(ft_path="bits", **GATHER)),
    Row("g5_bits_k3", cfg=dict(K=3, **BITS), expect=dict(ft_path="bits", grouped=True, **GATHER)),
    Row("g5_list", cfg=dict(BITS, l1=24, l2=7, l3=5, classes=3, batch=21), expect=dict(ft_path="list", **GATHER)),
    Row("A_forced_bits", env={"NNUE_FT_PATH": "bits"}, expect=dict(ft_path="bits", **GATHER)),
    Row("A_forced_list_k4", cfg=dict(K=4), env={"NNUE_FT_PATH": "list"}, expect=dict(ft_path="list", grouped=True, **GATHER)),
    Row("g16_patches", cfg=G16, expect=dict(use_patches=True, ste_chunks=160)),
    Row("g16_pixels", cfg=G16, env={"NNUE_CONV_PATCHES": "0"}, expect=dict(ste_chunks=160)),
    Row("g16_patches_k4", cfg=dict(K=4, **G16), expect=dict(use_patches=True, grouped=True, ste_chunks=160, **NO_L1)),
    Row("t8192", cfg=T8192, expect=dict(fuse_l1=False, ride_dw1=False, ride_small=False, phases=5, **NO_RIDE)),
    Row("t8192_ftu", cfg=T8192, env=FTU, expect=dict(fuse_l1=False, fuse_next_forward=True, phases=5, **GRAM)),
    Row("t8192_ftu_adam", cfg=dict(optimizer="adam", **T8192), env=FTU,
        expect=dict(GRAM, optimizer="adam", fuse_l1=False, fuse_next_forward=True, phases=5, defer_ste=False, ste_launch=3)),
    Row("t8192_ftu_plain", cfg=dict(momentum=0.0, **T8192), env=FTU, expect=dict(fuse_l1=False, fuse_next_forward=True, phases=5, **GRAM)),
    Row("t8192_ftu_k4", cfg=dict(K=4, **T8192), env=FTU, expect=dict(fuse_l1=False, grouped=True, phases=5, **GRAM)),
    Row("t8192_ftu_b200", cfg=dict(T8192, batch=200), env=FTU, expect=dict(phases=13, **GRAM)),
    Row("A_ftu", env=FTU, expect=dict(phases=13, **GRAM)),
    Row("t16384_b160", cfg=dict(grid=32, fps=16, image=96, batch=160),
        expect=dict(ride_dw1=False, ride_small=False, phases=13, **NO_RIDE)),
    Row("A_small_beside_dx", env={"NNUE_CLS_RIDE_SMALL": "0"}, expect=dict(ride_small=False, phases=27)),
    Row("A_b96_small_beside_dx", cfg=dict(batch=96), env={"NNUE_CLS_RIDE_SMALL": "0"},
        expect=dict(fuse_l1=False, ride_small=False, phases=19, ste_chunks=48)),
    Row("A_no_dw1_rider", env={"NNUE_FTM_RIDE_DW1": "0"}, expect=dict(ride_dw1=False, ride_small=False, phases=13)),
    Row("A_no_ste_ride", env={"NNUE_FTM_RIDE_STE": "0"}, expect=NO_RIDE),
    Row("A_no_deferred_ste", env={"NNUE_DEFER_STE": "0"}, expect=dict(defer_ste=False, ride_ste=False, ste_chunks=0, ste_launch=3)),
    Row("A_no_l1_fusion", env={"NNUE_FUSE_L1": "0"}, expect=NO_L1),
    # ---- what the census of the rows above left out: each kind of plane alone (the conv launch's riders write one set only),
    # the tail beside the d_x launch at the shape that can fuse it, the optimizer reading the table's rows for the norm, the
    # table update without the next forward at one stack, and the patch form of the STE launch in each of its stages
    Row("A_value_planes_alone", env={"NNUE_FTM_VAL_PLANES_MIN_TILES": "1"}, expect=dict(val_planes=True)),
    Row("A_forward_planes_alone", env={"NNUE_FTM_FWD_PLANES_MIN_WG": "1"}, expect=dict(fwd_planes=True)),
    Row("A_tail_beside_dx", cfg=dict(l2=128, l3=32), env={"NNUE_CLS_FUSE_TAIL_DX": "0"}),
    Row("A_no_norm_partials", env={"NNUE_NORM_PARTIALS": "0"}, expect=dict(sq="none")),
    Row("A_forced_patches", env={"NNUE_CONV_PATCHES": "1"}, expect=dict(use_patches=True)),
    Row("t8192_ftu_no_next_forward", cfg=T8192, env={**FTU, "NNUE_FUSE_NEXT_FORWARD": "0"}, expect=dict(fuse_l1=False, phases=5, **GRAM)),
    Row("g16_patches_no_ste_ride", cfg=G16, env={"NNUE_FTM_RIDE_STE": "0"}, expect=dict(use_patches=True, **NO_RIDE)),
    Row("g16_patches_adam", cfg=dict(optimizer="adam", **G16),
        expect=dict(use_patches=True, optimizer="adam", defer_ste=False, ride_ste=False, ste_chunks=0, ste_launch=3, sq="none")),
]
ROW_NAMES = [r.name for r in ROWS]
BY_NAME = {r.name: r for r in ROWS}


def set_knobs(monkeypatch, row: Row) -> None:
    """Clears every knob the resolution reads, then sets the row's own: an outer knob run cannot change a row."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in row.env.items():
        assert k in KNOBS, k
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------------------ the resolution
def geometry(cfg: Dict) -> Dict:
    """Shapes as nnue.NNUE and the trainer derive them: stride, map side, positions P, table rows F, table range of the flat
    buffers (FlatLayout.of: visual_threshold, conv.weight, input.weight, ... each padded to four floats)."""
    stride = max(1, (cfg["image"] - 1) // (cfg["grid"] - 1))
    side = (cfg["image"] - 1) // stride + 1
    p, f = cfg["fps"] * side * side, cfg["grid"] ** 2 * cfg["fps"]
    lo = (cfg["fps"] + 3) // 4 * 4 + (cfg["fps"] * 27 + 3) // 4 * 4
    hi = lo + min(f - 1, p) * cfg["l1"]
    return dict(stride=stride, side=side, P=p, F=f, tbl_lo=lo, tbl_hi=hi)


LEAD = ["visual_threshold", "conv.weight", "input.weight"]  # FlatLayout.of's first names (test_geometry_is_the_flat_layouts)


def step_mode_of(cfg: Dict, dp=None, use_graph: bool = True, count: Optional[int] = None, ft_path: Optional[str] = None):
    """nnue_hip.step_mode.resolve -- the policy the trainer itself uses -- at this configuration under the current
    environment, from the launch-free queries alone (no GPU).  dp: step_mode.DpFacts (default: one rank); count: the flat
    buffers' length (default: up to the table's end -- only the sharded update's threshold reads it); ft_path: the kernel
    family as an argument (default: NNUE_FT_PATH decides)."""
    from nnue_hip import step_mode
    g = geometry(cfg)
    return step_mode.resolve(B=cfg["batch"], H=cfg["image"], W=cfg["image"], stride=g["stride"], fps=cfg["fps"], F=g["F"],
                             L1=cfg["l1"], L2=cfg["l2"], L3=cfg["l3"], C=cfg["classes"], K=cfg["K"], optimizer=cfg["optimizer"],
                             dp=dp or step_mode.DpFacts(), use_graph=use_graph, lead_names=LEAD, tbl_lo=g["tbl_lo"],
                             tbl_hi=g["tbl_hi"], count=g["tbl_hi"] if count is None else count, ft_path=ft_path)


def resolve(cfg: Dict) -> Dict:
    """The mode a single-rank trainer of this configuration takes, as the dict the table uses."""
    sm = step_mode_of(cfg)
    m = {k: getattr(sm, k) for k in A_MODES if k not in ("grouped", "optimizer", "ste_chunks", "ste_launch")}
    m.update(grouped=cfg["K"] > 1, optimizer=cfg["optimizer"], ste_chunks=sm.ste_chunks if sm.ride_ste else 0, ste_launch=sm.ste_stages)
    return m


def launches_of(m: Dict) -> List[str]:
    """The C entry points of one steady-state step in mode `m`, in launch order (_segment over SEGMENTS, then _update)."""
    mfma, bits, grouped = m["ft_path"] == "mfma", m["ft_path"] == "bits", m["grouped"]
    cls = "nnue_classifier_train_step_bucketed" if grouped else "nnue_classifier_train_step"
    out = []
    # front (+ transpose)
    if m["val_planes"]:
        out.append("nnue_ftm_conv_binarize_value_planes")
    elif m["fwd_planes"]:
        out.append("nnue_ftm_conv_binarize_planes")
    elif mfma:
        out.append("nnue_ftm_conv_binarize_patches" if m["use_patches"] else "nnue_ftm_conv_binarize")
    else:
        out += ["nnue_conv3x3_forward"] + (["nnue_binarize_bits"] * 2 if bits else ["nnue_binarize_features"])
    # forward
    if grouped and not mfma:
        out.append("nnue_bucket_group")
    if m["fuse_l1"]:
        out.append("nnue_ftm_forward_l1_planes" if m["fwd_planes"] else "nnue_ftm_forward_l1")
    elif mfma:
        out.append("nnue_ftm_forward_grouping" if grouped else "nnue_ftm_forward")
    else:
        out.append("nnue_ftb_forward" if bits else "nnue_ft_forward")
    out.append(cls)
    # ft_wgrad, cls_wgrad
    if m["fuse_table_update"]:
        out.append("nnue_ftm_gram_sqnorm_tail")
    elif mfma and m["merge_backward"]:
        out.append("nnue_ftm_backward_planes" if m["val_planes"] else "nnue_ftm_backward_bucketed" if grouped else "nnue_ftm_backward")
    elif mfma:
        out.append("nnue_ftm_backward_weight")
    else:
        out.append("nnue_ftb_backward_weight" if bits else "nnue_ft_backward_weight")
    if not m["ride_dw1"]:
        out.append(cls)
    # tail
    if mfma and (m["fuse_table_update"] or not m["merge_backward"]):
        out.append("nnue_ftm_backward_values_ws")
    elif not mfma:
        out.append("nnue_ftb_backward_values" if bits else "nnue_ft_backward_values")
    if not m["ride_ste"]:
        out.append("nnue_ste_conv_backward_patches" if m["use_patches"] else "nnue_ste_conv_backward")
    # update
    adam = m["optimizer"] == "adam"
    if adam:
        out.append("nnue_adam_step_ext" if m["sq"] != "none" else "nnue_adam_step")
    else:
        out.append("nnue_sgd_step")
    if m["fuse_table_update"]:
        out.append("nnue_ftm_backward_weight_update_adam" if adam else "nnue_ftm_backward_weight_update")
    return out


# ------------------------------------------------------------------------------------------------ what a live trainer took
class CallLog:
    """Context manager: the C entry points the trainer issues while it is open, in order, as (route, name, args) with route
    "call" (a wrapper through lib._call: eager segments, plan recording) or "plan" (a recorded plan through lib.run_plan)."""

    def __enter__(self):
        from nnue_hip import lib
        self.lib, self.entries = lib, []
        self._call, self._run_plan = lib._call, lib.run_plan

        def log_call(name, *args):
            self.entries.append(("call", name, args[:-1]))
            self._call(name, *args)

        def log_plan(plan, stream_ptr, timers=None):
            self.entries.extend(("plan", c[0], c[2]) for c in plan)
            self._run_plan(plan, stream_ptr, timers)

        lib._call, lib.run_plan = log_call, log_plan
        return self

    def __exit__(self, *exc):
        self.lib._call, self.lib.run_plan = self._call, self._run_plan
        return False


def flags_of(tr) -> Dict:
    """The part of the mode a trainer's attributes state."""
    m = {k: bool(getattr(tr, k)) for k in FLAGS if k not in ("val_planes", "grouped")}
    m.update(ft_path=tr.ft_path, merge_backward=bool(tr.merge_backward), val_planes=tr.val_planes is not None,
             grouped=tr.bucket_plan is not None, optimizer=tr.optimizer, ste_chunks=int(tr.ste_chunks) if tr.ride_ste else 0)
    m["sq"] = "none" if tr.sq_partial is None else ("tiles" if tr.grads_materialised else "gram")
    return m


def modes_of(tr, log: Optional[CallLog] = None) -> Tuple[Dict, List[str]]:
    """(mode, entry points of one eager step).  `log`: what a CallLog saw during one full-batch eager step after the first
    (its recorded plans are what ran; a hyper-parameter change may have re-recorded the update plan through the wrappers
    first).  Without one, the trainer takes such a step on what input slot 0 holds."""
    if log is None:
        assert tr.steps_done > 0, "the first step records the plans through the wrappers"
        with CallLog() as log:
            tr.step(slot=0, timers={})  # an empty timer dict: the eager form, no events
    ran = [(name, args) for route, name, args in log.entries if route == "plan"]
    m = flags_of(tr)
    cls = [args for name, args in ran if name.startswith("nnue_classifier_train_step")]
    # (the phase mask is the last argument before the stream; the bucketed entry point has the plan after it)
    m["phases"] = int(cls[0][-2] if tr.bucket_plan is not None else cls[0][-1]) if cls else None
    ste = [args for name, args in ran if name.startswith("nnue_ste_conv_backward")]
    m["ste_launch"] = int(ste[0][-1]) if ste else None
    return m, [name for name, _ in ran]


def differences(got: Dict, want: Dict) -> List[str]:
    return [f"{k} is {got.get(k)!r}, the table says {want[k]!r}" for k in want if got.get(k) != want[k]]


# ------------------------------------------------------------------------------------------------ the oracle driver
def build_model(cfg: Dict):
    import nnue
    torch.manual_seed(0)
    model = nnue.NNUE(nnue.GridFeatureSet(cfg["grid"], cfg["fps"]), cfg["l1"], cfg["l2"], cfg["l3"], num_classes=cfg["classes"],
                      input_size=cfg["image"], num_ls_buckets=cfg["K"], clip_activations=cfg["clip"])
    if cfg["K"] > 1:
        with torch.no_grad():
            model.conv.weight.abs_()  # an image offset then moves all conv outputs of a sample the same way (spread_images)
    return model


def hyper(cfg: Dict) -> Dict:
    if cfg["optimizer"] == "adam":
        return dict(optimizer="adam", **ADAM)
    return dict(momentum=cfg["momentum"], **SGD)


def draw_batch(cfg: Dict, params64: Dict, stride: int, gen: torch.Generator, count: int):
    """`count` samples for the parameters of the step they are used in: clean_batch's margins against the `>` and ReLU
    gates at one stack, spread_images (feature counts over the whole range) at several."""
    if cfg["K"] == 1:
        from test_gpu_step_shapes import clean_batch
        return clean_batch(dict(cfg, batch=count), params64, stride, gen)
    from test_gpu_buckets import spread_images
    return spread_images(count, cfg["image"], gen), torch.randint(0, cfg["classes"], (count,), generator=gen)


def oracle_steps(cfg: Dict, params: Dict[str, torch.Tensor], seed: int = 77):
    """Three optimizer steps in float64 from `params`: a full batch with the clip active (max_grad_norm = half the gradient's
    own norm), a full batch with it inactive (twice the norm), a short batch of B - SHORT rows with it active.  Yields, per
    step, what the trainer is fed and what it must then hold."""
    import nnue_oracle as orc
    g = geometry(cfg)
    p = {k: v.double() for k, v in params.items()}
    gen = torch.Generator().manual_seed(seed)
    hp, state = hyper(cfg), {}
    for s, (count, clip_at) in enumerate(((cfg["batch"], 0.5), (cfg["batch"], 2.0), (cfg["batch"] - SHORT, 0.5))):
        images, labels = draw_batch(cfg, p, g["stride"], gen, count)
        before = {k: v.clone() for k, v in p.items()}
        logits, loss, grads, keep = orc.loss_and_grads_explicit(p, images.double(), labels, g["stride"], cfg["clip"])
        if cfg["K"] > 1:
            stacks = len(set(keep["bucket"].tolist()))
            assert stacks >= min(3, cfg["K"]), f"step {s}: the batch reaches {stacks} of {cfg['K']} stacks"
        norm = float(torch.sqrt(sum((grads[k] ** 2).sum() for k in orc.TRAINABLE_KEYS)))
        max_norm = clip_at * norm
        if cfg["optimizer"] == "adam":
            ref_norm = orc.adam_step(p, grads, state, hp["lr"], hp["weight_decay"], max_norm)
        else:
            ref_norm = orc.sgd_step(p, grads, state, hp["lr"], hp["momentum"], hp["weight_decay"], max_norm)
        assert abs(float(ref_norm) - norm) <= 1e-6 * norm
        yield dict(step=s, images=images, labels=labels, max_grad_norm=max_norm, logits=logits, loss=float(loss), norm=norm,
                   grads=grads, n=keep["n"], before=before, after={k: v.clone() for k, v in p.items()},
                   state={k: (dict(v) if isinstance(v, dict) else (None if v is None else v.clone())) for k, v in state.items()})


def _ratio_grad(got, ref, rtol=1e-4) -> float:
    """conftest.assert_close_grad's error over its bar."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).abs().max()) / (rtol * max(float(ref.abs().max()), 1e-12))


def _ratio_logits(got, ref, rtol=1e-4) -> float:
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float(((got - ref).abs() / (rtol * torch.clamp(ref.abs(), min=1.0))).max())


def compare_held(held: Dict, ref: Dict, B: int, n: int, scale: Optional[float], what: str, ratios: Dict[str, float]) -> List[str]:
    """What a trainer holds after one step, as plain tensors, against one oracle step at the project's bars
    (tests/test_gpu_step_shapes.py; Adam: test_a_step_group_at_the_224_shape_follows_the_oracle_with_adam): the one place the
    bars are written.  Returns the failures; ``ratios`` keeps the worst error over its bar per kind of check.

    held (every key optional but ``optimizer``; a missing one is not compared): ``logits`` [>= n, C], ``loss``, ``norm``,
    ``grads`` {name: tensor, as the kernels leave them: sums over the rows divided by B}, ``params`` and ``was`` {name:
    parameters after / before the step}, ``momentum`` | ``exp_avg`` + ``exp_avg_sq`` {name: tensor}, ``optimizer``, and
    ``sink``: the table row F - 1 of a clamp-sink map (P > F), else None.  A name is looked up in ``ref`` as it stands, so a
    caller that holds only a piece of a tensor passes the same piece of the oracle's under the same name.  scale: what
    restores the oracle's mean over the real samples from the held gradients (None: B / n, the single-rank short batch)."""
    import nnue_oracle as orc
    scale = B / n if scale is None else scale
    fails: List[str] = []

    def note(kind: str, ratio: float, detail: str = "") -> None:
        ratios[kind] = max(ratios.get(kind, 0.0), ratio)
        if not ratio <= 1.0:
            fails.append(f"{what} {kind} {detail}: {ratio:.3g} x its bar")

    def parts(k: str):
        """The tensor, and at a clamp-sink map (P > F) also the table rows the product covers on their own: row F - 1
        sums the gradient of every position past it, two orders above the other rows, and a per-tensor bar scaled by it
        would let an error confined to the product's rows (1e-3 of them, in _table_update's scale) pass."""
        yield "", slice(None)
        if k == "input.weight" and held.get("sink") is not None:
            yield " (rows below the sink)", slice(0, held["sink"])

    if "logits" in held and n > 0:
        note("logits", _ratio_logits(held["logits"][:n], ref["logits"]))
    if "loss" in held:
        note("loss", abs(float(held["loss"]) - ref["loss"]) / (1e-4 * max(1.0, abs(ref["loss"]))))
    if "norm" in held:
        note("norm", abs(float(held["norm"]) - ref["norm"]) / (1e-4 * ref["norm"]))
    for k, got in held.get("grads", {}).items():  # (a short batch: the kernels divide by B, the update's scale restores the mean over n)
        for label, rows in parts(k):
            note("grad", _ratio_grad(got[rows] * scale, ref["grads"][k][rows]), k + label)
    adam = held["optimizer"] == "adam"
    for k in (orc.TRAINABLE_KEYS if "params" in held else ()):
        for label, rows in parts(k):
            p_ref, p_got = ref["after"][k][rows], held["params"][k][rows]
            if adam:
                # Adam divides by sqrt(v): an element whose gradient is ~0 amplifies rounding, so compare on the update scale
                note("adam parameters", float((p_got.cpu().double() - p_ref).abs().max()) / (2e-5 + 1e-4 * float(p_ref.abs().max())), k + label)
                continue
            note("parameters", _ratio_grad(p_got, p_ref, rtol=1e-5), k + label)
            got_d, ref_d = (p_got - held["was"][k][rows]).cpu().double(), p_ref - ref["before"][k][rows]
            floor = 2 * 2.0 ** -23 * float(p_ref.abs().max())  # a float32 parameter cannot move by less than its own rounding
            note("update", float((got_d - ref_d).abs().max()) / (2e-4 * float(ref_d.abs().max()) + floor), k + label)
    for kind, of in (("exp_avg", lambda st: st["m"]), ("exp_avg_sq", lambda st: st["v"]), ("momentum", lambda st: st)):
        for k, got in held.get(kind, {}).items():
            for label, rows in parts(k):
                note(kind, _ratio_grad(got[rows], of(ref["state"][k])[rows]), k + label)
    return fails


def held_by(tr, was: Optional[Dict[str, torch.Tensor]] = None) -> Dict:
    """compare_held's ``held`` of a trainer whose flat buffers are whole (a single rank, or a replica after an all-reduce),
    without logits, loss and norm."""
    held = dict(optimizer=tr.optimizer, sink=tr.F - 1 if tr.P > tr.F else None, params=tr.p, was=was)
    if tr.grads_materialised:
        held["grads"] = tr.layout.views(tr.flat_grads)
    if tr.optimizer == "adam":
        held.update(exp_avg=tr.layout.views(tr.flat_exp_avg), exp_avg_sq=tr.layout.views(tr.flat_exp_avg_sq))
    elif tr.flat_momentum is not None:
        held["momentum"] = tr.layout.views(tr.flat_momentum)
    return held


def check_step(tr, ref: Dict, was: Dict[str, torch.Tensor], loss: torch.Tensor, what: str, ratios: Dict[str, float]) -> None:
    """One trainer step against one oracle step at compare_held's bars.  `was`: the trainer's parameters before the step.
    ratios: the worst error over its bar per kind of check, kept for the record before anything is asserted."""
    from conftest import assert_close_grad, assert_close_logits
    n, B = ref["images"].shape[0], tr.B
    torch.cuda.synchronize()
    if n == B:
        n_mean, n_max = tr.active_stats()
        assert n_max == int(ref["n"].max()) and abs(n_mean - float(ref["n"].float().mean())) < 1e-2, f"{what}: feature counts differ"
    fails = compare_held(dict(held_by(tr, was), logits=tr.logits, loss=loss, norm=tr.grad_norm), ref, B, n, None, what, ratios)
    assert not fails, "; ".join(fails)
    # the same bars through the project's own assertions
    assert_close_logits(tr.logits[:n], ref["logits"], f"{what} logits")
    if tr.grads_materialised:
        for k, g in ref["grads"].items():
            assert_close_grad(tr.layout.views(tr.flat_grads)[k] * (B / n), g, f"{what} grad {k}")


def snapshot(tr) -> List[torch.Tensor]:
    return [tr.flat_params.clone()] + [t.clone() for t in tr._optimizer_buffers()]


def same(a: List[torch.Tensor], b: List[torch.Tensor]) -> bool:
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@contextlib.contextmanager
def trainer_for(cfg: Dict, **kw):
    """A trainer of the row's configuration on a fresh model with the seed's parameters."""
    from nnue_hip.trainer import NnueTrainer
    model = build_model(cfg)
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tr = NnueTrainer(model.to("cuda"), cfg["batch"], (cfg["image"], cfg["image"]), max_grad_norm=1.0, **hyper(cfg), **kw)
    try:
        yield tr, params
    finally:
        torch.cuda.synchronize()
