"""The training step's launch policy: shape, optimizer, data-parallel state and the NNUE_* knobs in, one frozen ``StepMode`` out.

``resolve`` allocates nothing and launches nothing: it asks only the library's launch-free queries, so it answers on any
machine (``print(step_mode.resolve(...).describe())``).  NnueTrainer allocates from the mode and its segments read it;
tests/trainer_modes.py is the table that holds it still.  The knobs are read from ``os.environ`` here because the library reads
the same ones from the process environment behind its queries.

``step_form`` (at the end) is the second, per-call decision: which run form one call of ``NnueTrainer.step`` takes.
"""
from __future__ import annotations

import os
from collections import namedtuple
from dataclasses import dataclass, fields
from typing import Optional, Sequence, Tuple

from . import lib

# what the policy reads of trainer.DataParallel (the default: one rank, no collectives)
DpFacts = namedtuple("DpFacts", "collectives world buckets backend", defaults=(False, 1, 1, None))


@dataclass(frozen=True)
class StepMode:
    ft_path: str                 # "mfma" | "bits" | "list"
    use_patches: bool
    factor_exchange: bool
    defer_ste: bool
    fuse_l1: bool
    fwd_planes: bool
    sharded_update: bool
    capture_collectives: bool    # (the trainer clears its own copy when a capture fails)
    merge_backward: bool
    fuse_table_update: bool
    grads_materialised: bool
    ride_dw1: bool
    sq: str                      # the table's share of the clip norm: "tiles" | "gram" | "none" (the optimizer reads the rows)
    sq_range: Optional[Tuple[int, int]]  # the table rows the product covers, in the flat buffers (None: sq == "none")
    sq_count: int                # partial sums the producer leaves
    ride_ste: bool
    ste_chunks: int              # partials per output of STE stage 1, in the merged backward or in the STE launch
    val_planes: bool
    fuse_next_forward: bool
    ride_small: bool
    fuse_tail_dx: bool
    phases: int                  # classifier_train_step's mask in the forward segment (lib.CLS_*)
    ste_stages: Optional[int]    # ``stages`` of the STE launch; None: no launch, stage 1 rides in the merged backward
    merged_backward_launch: bool  # one launch produces weight gradient, value gradient (d_conv_out) and tail rows

    conv_planes = property(lambda self: self.fwd_planes or self.val_planes)  # the conv launch's riders leave planes of the table
    use_mfma = property(lambda self: self.ft_path == "mfma")
    use_bits = property(lambda self: self.ft_path == "bits")

    def describe(self) -> str:
        """One line, as a row of profiles/trainer_modes.md: path | flags on | sq | phases | STE."""
        usual = ("merge_backward", "grads_materialised", "merged_backward_launch")  # on by default: not part of that form
        on = [f.name for f in fields(self) if f.type == "bool" and f.name not in usual and getattr(self, f.name)]
        ste = f"ride, {self.ste_chunks} chunks" if self.ste_stages is None else f"stages={self.ste_stages}"
        return f"{self.ft_path} | {', '.join(on) or '-'} | sq {self.sq} | phases {self.phases} | STE {ste}"


def _on(knob: str) -> bool:
    return os.environ.get(knob, "1") != "0"


def resolve(*, B: int, H: int, W: int, stride: int, fps: int, F: int, L1: int, L2: int, L3: int, C: int, K: int, optimizer: str,
            dp: DpFacts = DpFacts(), use_graph: bool = True, lead_names: Sequence[str], tbl_lo: int, tbl_hi: int,
            count: int, ft_path: Optional[str] = None) -> StepMode:
    """lead_names: the first parameters of the flat layout; tbl_lo/tbl_hi: the table rows the product d_W = A^T d_out covers, as
    a range of the flat buffers; count: their length (FlatLayout); ft_path: lib.ft_path's ``mode`` (None: NNUE_FT_PATH)."""
    gh, gw = lib.conv_out_hw(H, W, stride)
    P = fps * gh * gw
    sgd, lead = optimizer == "sgd", list(lead_names)
    # binary features: float {0,1} map + dense MFMA products when the shape allows, else bit masks + LDS-staged
    # gather kernels, else id lists
    ft_path = lib.ft_path(F, P, L1, B, mode=ft_path)
    mfma = ft_path == "mfma"
    # Large strides (the taps of neighbouring positions do not overlap: 224x224 at stride 7 reads 3 of every 7 rows and the
    # backward would gather them again): the conv launch also leaves the im2col form of the images -- 27 floats per position,
    # 0.18 of the image bytes -- and the STE backward reads the patches instead of the images (bitwise).
    # NNUE_CONV_PATCHES=0|1|auto (auto: images more than twice their patches).
    pm = os.environ.get("NNUE_CONV_PATCHES", "auto")
    use_patches = mfma and fps <= 64 and pm != "0" and (pm == "1" or 3 * H * W > 2 * 27 * gh * gw)
    # every form that leaves the table's rows to the product's launch (their sums of squares, their update) needs the range
    # non-empty and float4-aligned
    tbl_ok = tbl_hi > tbl_lo and tbl_lo % 4 == 0 and tbl_hi % 4 == 0
    big_table = F * L1 * 4 >= (32 << 20)
    gb = B * dp.world
    # Data parallel with a bandwidth-sized table: the ranks all-gather the FACTORS of the table's gradient (the map as
    # bits + d_ft, ~1.5 MB per rank at the 224x224 shape) instead of reducing the 269 MB product, and every rank runs the
    # fused single-rank path (Gram norm, update in the product's epilogue) on the global factors: no big collective, no
    # materialised d_W, bitwise identical replicas.  The other gradients travel in the same all-gather and are summed in
    # rank order (lib.FactorExchange).  NNUE_DP_FACTOR_EXCHANGE=auto|1|0; auto = tables of 32 MB or more.
    fx_mode = os.environ.get("NNUE_DP_FACTOR_EXCHANGE", "auto")
    factor_exchange = (dp.collectives and mfma and sgd and dp.buckets == 1 and tbl_ok
                       and lead[:3] == ["visual_threshold", "conv.weight", "input.weight"]
                       and gb * L1 <= (1 << 24) and ((gb + 15) // 16) * ((L1 + 15) // 16) <= 65536
                       and fx_mode != "0" and (fx_mode == "1" or big_table))
    # single rank + SGD: the second stage of the STE / conv-weight gradient sum rides in the optimizer's norm launch
    # (with collectives the gradients must be complete before the all-reduce)
    defer_ste = (not dp.collectives and sgd and _on("NNUE_DEFER_STE") and fps * 28 <= 4096
                 and lead[:2] == ["visual_threshold", "conv.weight"])
    # K > 1: the first layer's weights differ per sample, so its product is the classifier's own grouped launch
    # (bucket-homogeneous MFMA tiles) instead of the FeatureTransformer forward's epilogue / backward rider
    fuse_l1 = K == 1 and mfma and _on("NNUE_FUSE_L1") and lib.ftm_forward_l1_supported(B, F, P, L1, L2)
    # Where that forward runs 32-row tiles (the CIFAR batch-512 shape), the conv launch's rider workgroups leave the table as
    # pre-split bf16 planes once per step and the forward reads those on the bf16 matrix unit (nnue_ftm_conv_binarize_planes
    # -> nnue_ftm_forward_l1_planes) instead of the table on the f32 one.  NNUE_FTM_FWD_PLANES=0 keeps the two plain calls.
    fwd_planes = (fuse_l1 and not use_patches and _on("NNUE_FTM_FWD_PLANES")
                  and lib.ftm_forward_l1_planes_supported(B, F, P, L1, L2))
    # Sharded update for bandwidth-sized flat buffers under collectives (SGD): reduce-scatter, per-shard clip + SGD with
    # the norm assembled from all-gathered block partials, all-gather of the parameters.  NNUE_DP_SHARDED_UPDATE=0|1|auto
    shard_mode = os.environ.get("NNUE_DP_SHARDED_UPDATE", "auto")
    sharded_update = (dp.collectives and sgd and dp.buckets == 1 and shard_mode != "0" and not factor_exchange
                      and (shard_mode == "1" or count * 4 >= (64 << 20)))
    # the collective(s) captured into the step graph (torch's NCCL path is capturable): one replay per step, no host
    # round trip between the local kernels, the exchange and the update.  NNUE_DP_CAPTURE=0 keeps the eager collective.
    capture_collectives = dp.collectives and use_graph and dp.backend == "nccl" and dp.buckets == 1 and _on("NNUE_DP_CAPTURE")
    merge_backward = os.environ.get("NNUE_FTM_SPLIT_BACKWARD", "0") != "1"
    # Big tables on a single rank (SGD or Adam): the FeatureTransformer weight gradient is never materialised.  Its squared
    # norm comes from two B x B Gram matrices (nnue_ftm_gram_sqnorm), the optimizer's norm/apply pass skips those rows
    # and leaves the clip coefficient in a device scalar, and the product d_W = A^T d_out runs LAST, applying the update
    # to the table (Adam: and to its two moments) in its epilogue (nnue_ftm_backward_weight_update[_adam]): no 268 MB write
    # + read at the 224x224 shape.
    want = os.environ.get("NNUE_FUSE_TABLE_UPDATE", "auto")
    fuse_table_update = (mfma and not dp.collectives and tbl_ok and B * L1 <= (1 << 24) and want != "0"
                         and (big_table or want == "1"))
    # With the fused table update ``model.input.weight.grad`` (a view of flat_grads) is never written: rows the product
    # covers stay at the zeros they were allocated with.  ``grads_materialised`` says so; callers that want the table's
    # gradient for logging or custom clipping set NNUE_FUSE_TABLE_UPDATE=0.
    grads_materialised = not (fuse_table_update or factor_exchange)
    merged_backward_launch = mfma and merge_backward and grads_materialised
    # the classifier's first-layer weight gradient rides in the merged FeatureTransformer backward launch (a third
    # tile family reading d_z1 out of the classifier's scratch) where that launch is used
    ride_dw1 = merged_backward_launch and _on("NNUE_FTM_RIDE_DW1") and lib.ftm_backward_cw_supported(B, F, P, L1, L2)
    # the sums of squares of the table's share (flat_grads[sq_range]) of the clip norm, left by its producer
    if not grads_materialised:  # the Gram form; under the factor exchange on the global factors (B * world rows)
        sq, sq_count = "gram", int(lib.load().nnue_ftm_gram_sq_count(gb, L1))
    elif merged_backward_launch and not dp.collectives and sgd and tbl_ok and _on("NNUE_NORM_PARTIALS"):
        # single rank + SGD: the FT weight-gradient tiles leave their sums of squares, so the clip norm does not read
        # those rows of the flat gradient buffer again (268 MB at the 224x224 configuration)
        sq_count = lib.ftm_backward_sq_count(B, F, P, L1)
        sq = "tiles" if sq_count > 0 else "none"
    else:
        sq, sq_count = "none", 0
    # Single rank + SGD with the merged FeatureTransformer backward: its value-gradient tiles also reduce d_conv_out into the
    # STE partials (stage 1 of ste_conv_backward) in their epilogue, so the STE launch disappears and d_conv_out is not
    # stored; the second stage stays in the norm launch.  With the im2col patches the epilogue reads them instead of the images
    # (the same bits, as the STE kernel's two forms).  NNUE_FTM_RIDE_STE=0 keeps the STE launch.
    ride_chunks = lib.ftm_backward_ste_chunks(B, F, P, L1, H, W, stride) if mfma else 0
    ride_ste = defer_ste and merged_backward_launch and ride_chunks > 0 and _on("NNUE_FTM_RIDE_STE")
    ste_chunks = ride_chunks if ride_ste else lib.ste_conv_backward_chunks(B, fps, gh, gw)
    # Where the ride runs 32-row value tiles on a chip-filling launch (the CIFAR batch-512 shape, where the forward takes its
    # planes too), the conv launch's riders also leave the table rows the value gradient reads as bf16 planes, and the merged
    # backward's value tiles read those on the bf16 matrix unit (nnue_ftm_conv_binarize_value_planes ->
    # nnue_ftm_backward_planes).  Written by a step's conv launch and read by that step's backward only: the table is updated
    # after it.  NNUE_FTM_VAL_PLANES=0 keeps the f32 tiles.
    val_planes = ride_ste and not use_patches and not K > 1 and lib.ftm_value_planes_supported(B, F, P, L1, H, W, stride)
    # Inside a step group (step_many) the table's update of step t and the FeatureTransformer forward of step t+1 are ONE
    # pass over the table (nnue_ftm_backward_weight_update_forward: the next batch is resident, its map only needs the conv
    # weights the small tensors' update has just written, and the update leaves every new table tile in registers) -- the
    # forward's own 268 MB read of the table disappears.  Two maps alternate (the update still reads step t's while step
    # t+1's is being written).  Bitwise the separate kernels.  NNUE_FUSE_NEXT_FORWARD=0 keeps them separate.
    # (Under the factor exchange the update contracts the all-gathered GLOBAL batch, the next forward this rank's own next map.)
    fuse_next_forward = (not grads_materialised and not fuse_l1 and K == 1 and _on("NNUE_FUSE_NEXT_FORWARD")
                         and lib.ftm_update_forward_supported(gb if factor_exchange else B, F, P, L1, B))
    # ... and so do the classifier's small gradients + mean loss (one more tile family of the merged backward launch; the
    # classifier's d_x launch then holds only d_x tiles).  NNUE_CLS_RIDE_SMALL=0 keeps them beside d_x.
    ride_small = ride_dw1 and _on("NNUE_CLS_RIDE_SMALL")
    # ... and then the classifier's per-sample tail runs inside its d_x launch (each d_x row tile recomputes the tail of its
    # own 16 rows; bitwise the two launches).  NNUE_CLS_FUSE_TAIL_DX=0 keeps the two launches.
    fuse_tail_dx = (fuse_l1 and ride_small and _on("NNUE_CLS_FUSE_TAIL_DX")
                    and lib.classifier_train_fused_tail_supported(B, L1, L2, L3, C, K))
    # the forward segment's classifier call: d_x always; the layer-1 slabs come from the fused forward's epilogue; d_w1 either
    # beside d_x (the cls_wgrad segment then sums its slabs: CLS_PHASE_SMALL | CLS_DW1_BESIDE_DX) or left to the merged
    # backward's rider, and then both phases are this one call
    phases = lib.CLS_PHASE_DX | (lib.CLS_L1_SLABS_GIVEN if fuse_l1 else 0)
    if ride_dw1:
        phases |= (lib.CLS_PHASE_SMALL | lib.CLS_DW1_RIDES | (lib.CLS_SMALL_RIDE if ride_small else 0)
                   | (lib.CLS_TAIL_IN_DX if fuse_tail_dx else 0))
    else:
        phases |= lib.CLS_DW1_BESIDE_DX
    return StepMode(
        ft_path=ft_path, use_patches=use_patches, factor_exchange=factor_exchange, defer_ste=defer_ste, fuse_l1=fuse_l1,
        fwd_planes=fwd_planes, sharded_update=sharded_update, capture_collectives=capture_collectives, merge_backward=merge_backward,
        fuse_table_update=fuse_table_update, grads_materialised=grads_materialised, ride_dw1=ride_dw1, sq=sq,
        sq_range=(tbl_lo, tbl_hi) if sq != "none" else None, sq_count=sq_count, ride_ste=ride_ste, ste_chunks=ste_chunks,
        val_planes=val_planes, fuse_next_forward=fuse_next_forward, ride_small=ride_small, fuse_tail_dx=fuse_tail_dx, phases=phases,
        ste_stages=None if ride_ste else (1 if defer_ste else 3), merged_backward_launch=merged_backward_launch)


# ---- The run form of ONE call of NnueTrainer.step.  ``StepMode`` is per trainer and fixed at construction; ``StepForm`` is per
# call: it depends on whether this is the first step, whether the batch is short, whether timers were passed, and on the trainer's
# run-time copy of ``capture_collectives`` (a failed capture clears it).  Launch-free like ``resolve``.
#
# form name -> the kind of the ``_g_local`` key (slot, kind) of the ONE graph that is the whole step -- local kernels, exchange
# and update -- or None where the call runs its parts, its exchange and its update one after the other:
#   graph_dp      local kernels + _exchange_and_update(False), captured together (steady state, captured collectives)
#   graph         local kernels + the ``upd`` plan, captured together (steady state, no collectives)
#   local         part "all", then the update tail (no collectives: first step, short batch, timers, no graphs)
#   own_exchange  part "all", then an eager _exchange_and_update, which updates itself (sharded update, factor exchange)
#   one_message   part "all", one all-reduce of the whole flat gradient buffer (blocking, or async_op + wait()), the update tail
#   two_buckets   part "a", async all-reduce of the big bucket, part "b", async all-reduce of the tail bucket, both waited, the
#                 update tail
# A part is a replay of graph (slot, part) with graphs, else its recorded segments run eagerly.  The update tail is, in order:
# short batch -> eager _update with the scaled gradient (the loss is scaled too); first step -> the ``upd_first`` plan; graphs ->
# a replay of ``_g_update``; else the ``upd`` plan run eagerly.
FORMS = {"graph_dp": "full_dp", "graph": "full", "local": None, "own_exchange": None, "one_message": None, "two_buckets": None}
# the kinds of ``_g_local`` key whose graph contains an optimizer update (a change of the update plans drops them): the whole-step
# graphs above and step_many's group graph (slots, "many")
UPDATE_GRAPH_KINDS = tuple(kind for kind in FORMS.values() if kind is not None) + ("many",)


@dataclass(frozen=True)
class StepForm:
    name: str                  # a key of FORMS
    parts: Tuple[str, ...]     # the local parts the call runs, captured ahead of any collective: ("all",) | ("a", "b")
    async_op: bool = False     # one_message only: async_op + wait() instead of the blocking collective

    graph = property(lambda self: FORMS[self.name])  # the kind of the whole-step graph the call replays, or None


def step_form(*, graphs: bool, first: bool, ragged: bool, collectives: bool, buckets: int, capture_collectives: bool,
              own_exchange: bool, async_op: bool = False) -> StepForm:
    """graphs: the trainer uses graphs and the call has no timers; first: no step has been taken; ragged: a short-batch factor
    applies; collectives, buckets: DataParallel's; capture_collectives: the trainer's run-time copy; own_exchange: the mode's
    sharded_update or factor_exchange; async_op: NNUE_DP_ASYNC_OP=1 at this call.  The trainer reaches only combinations in which
    capture_collectives implies collectives, graphs on the trainer and one bucket, and own_exchange implies collectives and one
    bucket; any other combination gets what the same order of questions gives it -- none is special-cased."""
    parts = ("a", "b") if collectives and buckets == 2 else ("all",)
    steady = graphs and not first and not ragged
    if steady and capture_collectives:
        name = "graph_dp"
    elif steady and not collectives:
        name = "graph"
    elif not collectives:
        name = "local"
    elif own_exchange:
        name = "own_exchange"
    elif buckets != 2:
        name = "one_message"
    else:
        name = "two_buckets"
    return StepForm(name, parts, bool(async_op) and name == "one_message")
