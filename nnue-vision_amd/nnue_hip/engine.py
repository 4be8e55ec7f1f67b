"""The compiled engine's integer inference on the GPU.

``EngineModel.load(path)`` parses a ``.nnue`` file the way ``NNUEEvaluator::load_model`` does
(engine/src/nnue_engine.cpp:544-657; same rejections) and keeps its quantised tensors in device memory;
``evaluate_logits(images)`` is ``NNUEEvaluator::evaluate_logits`` (nnue_engine.cpp:704-734) for a whole batch --
bit-identical to the C++ engine (tests/golden/engine_cases.npz and engine_shapes.npz hold outputs of the real engine).
``stream(S)`` is ``NNUEEvaluator::evaluate_incremental`` (nnue_engine.cpp:739-786) for S independent frame sequences: each
step updates a stored int16 accumulator by the features that changed, with the same bits as ``evaluate_logits``; its
``update(added, removed)`` takes just those features as two id lists (``NNUEEvaluator::update_features``, :818-821).
``EngineModel.load(path, bucket="auto")`` keeps all K layer stacks of the file; both calls then choose the stack of every image
from its own active-feature count (``stack_of``, the rule a ``num_ls_buckets=K`` model is trained with) or take it from the
caller -- the engine's ``layer_stack_index`` (nnue_engine.cpp:704-707), bit-identical to the engine stack by stack.
``EngineModel.from_model(model)`` builds the same tensors from a live ``nnue.NNUE`` on the device, without the file and without
touching the model (one launch, include/nnue_hip.h: nnue_engine_quantize_model); ``requantize(model)`` repeats that launch into
the tensors the engine already holds -- what a training loop does after every epoch.
``evaluate_logits(..., path="matrix")`` and ``evaluate_features(active)`` run the accumulate step as one product on the int8
matrix unit (include/nnue_hip.h: nnue_engine_evaluate_logits_matrix) over int8 planes of the table packed once
(``prepare_matrix``): the same bits, since addition mod 2^16 depends on neither order nor accumulator width.
``evaluate_logits_u8(store, indices)`` and ``EngineStream.step_u8`` take uint8 ``[N,H,W,3]`` frames -- the dataset store of
``GpuImageDataset``, a camera's frames -- and form the conv bytes straight from them (include/nnue_hip.h:
nnue_engine_evaluate_logits_u8): with the defaults, the bits of the float call on ``lib.load_batch`` of the same indices,
without the float batch.  ``EngineStream.step_u8_regions(frames, rects)`` is that step from the frames' dirty rectangles: the conv re-run
only on the grid cells a rectangle touches, the flipped table rows walked, no conv scratch (include/nnue_hip.h:
nnue_engine_stream_step_u8_regions).
"""
from __future__ import annotations

import ctypes
import os
import struct
from pathlib import Path
from typing import Iterable, Optional, Tuple, Union

import numpy as np
import torch

from . import lib


_STACK_TENSORS = ("l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b")

_PATHS = ("gather", "matrix", "auto")
# path="auto" takes the matrix form from this many map bytes (B * num_features) upwards.  The sweep of tools/bench_engine.py
# --shape {c2,224} (profiles/engine_matrix.json; gather / matrix ms, matrix p90 below gather p10 at every point):
#   CIFAR shape (F = 800, L1 = 1024)     B = 16: 0.261 / 0.052   128: 0.265 / 0.058   512: 0.270 / 0.065   4096: 0.624 / 0.226
#   224x224 shape (F = 65536, L1 = 512)  B = 2: 26.7 / 0.114     64: 27.4 / 0.183     128: 27.4 / 0.258    1024: 37.2 / 1.24
# The matrix form won at every measured point, so the constant is the smallest of them (CIFAR, B = 16); below it auto stays on
# the gather form, which nothing measured there contradicts.
_MATRIX_MIN_MAP_BYTES = 12800


class _CModel(ctypes.Structure):  # include/nnue_hip.h: nnue_engine_model
    _fields_ = ([(n, ctypes.c_int32) for n in ("num_features", "l1", "l2", "l3", "classes", "grid", "oc")]
                + [(n, ctypes.c_float) for n in ("conv_scale", "threshold", "quantized_one", "l1_scale", "l2_scale", "out_scale")]
                + [(n, ctypes.c_void_p) for n in ("conv_w", "conv_b", "ft_w", "ft_b", "l1_w", "l1_b", "l2_w", "l2_b", "out_w", "out_b")])


class _CStacks(ctypes.Structure):  # include/nnue_hip.h: nnue_engine_stacks
    _fields_ = ([("count", ctypes.c_int32), ("scales", ctypes.POINTER(ctypes.c_float))]
                + [(n, ctypes.c_void_p) for n in _STACK_TENSORS])


class _CU8Frames(ctypes.Structure):  # include/nnue_hip.h: nnue_engine_u8_frames
    _fields_ = [("data", ctypes.c_void_p), ("indices", ctypes.c_void_p), ("count", ctypes.c_int64), ("layout", ctypes.c_int32),
                ("mean255", ctypes.c_float * 3), ("inv_std255", ctypes.c_float * 3)]


U8_LAYOUTS = {"chw": 0, "hwc": 1}
# A.Normalize's defaults in the reference's transform lists (data/datasets.py:366-369)
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def u8_constants(mean=None, std=None) -> Tuple[np.ndarray, np.ndarray]:
    """(mean255, inv_std255) float32 [3] as the u8 calls take them: mean * 255 and 1 / (std * 255), every operation in float32
    (with the defaults: the constants of ``lib.load_batch``, bit for bit).  ValueError for anything but three finite numbers,
    or a std that is not positive."""
    out = []
    for name, given, default in (("mean", mean, IMAGENET_MEAN), ("std", std, IMAGENET_STD)):
        try:
            a = np.asarray(default if given is None else given, dtype=np.float32).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"{name}: expected three numbers, got {given!r}") from None
        if a.shape != (3,) or not np.all(np.isfinite(a)):
            raise ValueError(f"{name}: expected three finite numbers, got {given!r}")
        out.append(a)
    mean32, std32 = out
    if np.any(std32 <= 0):
        raise ValueError(f"std: every channel must be positive, got {std!r}")
    return mean32 * np.float32(255.0), np.float32(1.0) / (std32 * np.float32(255.0))


class EngineFormatError(ValueError):
    pass


def stack_of(active_counts: torch.Tensor, num_stacks: int, num_features: int) -> torch.Tensor:
    """The layer stack of an image with ``active_counts`` active features: min(K-1, n*K // (num_features+1)), the training
    rule (``nnue.bucket_of``) on the engine's feature count -- density * num_features of the engine calls."""
    from nnue import bucket_of
    return bucket_of(active_counts, num_stacks, num_features)


class _Reader:
    def __init__(self, data: bytes):
        self.data, self.off = data, 0

    def take(self, fmt: str):
        try:
            vals = struct.unpack_from("<" + fmt, self.data, self.off)
        except struct.error as e:
            raise EngineFormatError(f"truncated file: {e}") from None
        self.off += struct.calcsize("<" + fmt)
        return vals if len(vals) > 1 else vals[0]

    def array(self, dtype, count: int) -> np.ndarray:
        nbytes = np.dtype(dtype).itemsize * count
        if count < 0 or self.off + nbytes > len(self.data):
            raise EngineFormatError("truncated file")
        a = np.frombuffer(self.data, dtype=dtype, count=count, offset=self.off).copy()
        self.off += nbytes
        return a


class EngineModel:
    """Quantised tensors of one `.nnue` file on the device + the scalars of its header.  ``stack_scales`` (loaded with
    bucket="auto"): the six stack tensors hold all K stacks, stack-major, and every call selects a stack per image."""

    def __init__(self, header: dict, tensors: dict, device, stack_scales: Optional[np.ndarray] = None,
                 table_planes: Optional[int] = None):
        self.header = header
        self.device = torch.device(device)
        # int8 planes of ft_w for the matrix form, outside self.tensors: 1 when every table value fits a byte, else 2 (lo, hi);
        # None = not known on the host, prepare_matrix finds out from the one-plane pack's misfit count
        ft_w = tensors.get("ft_w")
        if table_planes is None and isinstance(ft_w, np.ndarray) and ft_w.size:
            table_planes = 2 if int(ft_w.min()) < -128 or int(ft_w.max()) > 127 else 1
        self.table_planes: Optional[int] = table_planes
        self._planes: Optional[torch.Tensor] = None
        self._misfit: Optional[torch.Tensor] = None
        self._matrix_scratch: Optional[torch.Tensor] = None
        self.tensors = {k: (v if torch.is_tensor(v) else torch.from_numpy(v)).to(self.device) for k, v in tensors.items()}
        c = _CModel()
        for k in ("num_features", "l1", "l2", "l3", "classes", "grid", "oc"):
            setattr(c, k, int(header[k]))
        for k in ("conv_scale", "threshold", "quantized_one", "l1_scale", "l2_scale", "out_scale"):
            setattr(c, k, float(header[k]))
        for k, t in self.tensors.items():
            setattr(c, k, t.data_ptr())
        self._c = c  # of a stack-selecting model: its stack 0 (the packed tensors begin with it)
        self._scratch: Optional[torch.Tensor] = None
        self._stacks: Optional[_CStacks] = None
        self.generation = 0  # advanced by requantize: an EngineStream's accumulators are sums over the table of one generation
        self._stack_index = 0  # of a single-stack model built by from_model: the source stack requantize reads
        self._bad: Optional[torch.Tensor] = None  # device int32: elements the last quantise launches could not represent
        self._bad_known_zero = False
        if stack_scales is not None:
            self._scales = np.ascontiguousarray(stack_scales, dtype=np.float32)  # host [K][3], read by every call
            st = _CStacks()
            st.count = int(self._scales.shape[0])
            st.scales = self._scales.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
            for k in _STACK_TENSORS:
                setattr(st, k, self.tensors[k].data_ptr())
            self._stacks = st

    @property
    def num_classes(self) -> int:
        return int(self.header["classes"])

    @property
    def num_stacks(self) -> int:
        """Layer stacks the model selects among: K after load(bucket="auto"), else 1."""
        return 1 if self._stacks is None else int(self._stacks.count)

    def _on_device(self, t: torch.Tensor) -> bool:
        """Whether ``t`` is a device tensor on the model's device."""
        return t.is_cuda and (self.device.index is None or t.device.index == self.device.index)

    def _outputs(self, n: int, changed: bool = False, zero_stacks: bool = False):
        """What a call on n images or streams writes: (logits [n, C] float32, density [n] float32, changed [n] int32 or None,
        used [n] int32).  ``used`` takes the stacks of a stack-selecting model; a single-stack model has None there, or zeros
        where the caller returns them (zero_stacks)."""
        logits = torch.empty((n, self.num_classes), dtype=torch.float32, device=self.device)
        density = torch.empty((n,), dtype=torch.float32, device=self.device)
        delta = torch.empty((n,), dtype=torch.int32, device=self.device) if changed else None
        if self._stacks is not None:
            used = torch.empty((n,), dtype=torch.int32, device=self.device)
        else:
            used = torch.zeros((n,), dtype=torch.int32, device=self.device) if zero_stacks else None
        return logits, density, delta, used

    def _stack_arg(self, stacks: Optional[torch.Tensor], n: int, what: str) -> Optional[torch.Tensor]:
        """The caller's stack indices as the int32 [n] device tensor the C call takes (outside [0, K) = stack 0)."""
        if stacks is None:
            return None
        if self._stacks is None:
            raise ValueError(f"{what}: stacks= needs a model loaded with bucket=\"auto\" (this one holds a single stack)")
        if not isinstance(stacks, torch.Tensor) or stacks.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{what}: stacks must be an int32 or int64 tensor")
        if not stacks.is_cuda or tuple(stacks.shape) != (n,):
            raise ValueError(f"{what}: stacks must be a device tensor of shape ({n},), got {tuple(stacks.shape)} on {stacks.device}")
        if stacks.dtype == torch.int64:  # an index beyond int32 must not wrap into the range
            stacks = torch.where((stacks >= 0) & (stacks < self.num_stacks), stacks, torch.zeros_like(stacks)).to(torch.int32)
        return stacks.contiguous()

    @staticmethod
    def load(path, device=None, bucket: Union[int, str] = 0) -> "EngineModel":
        """bucket: the one layer stack to keep (an index the file lacks means stack 0, nnue_engine.cpp:705-707), or "auto":
        all of them, packed for per-image selection (their class counts and bias lengths must agree)."""
        auto = isinstance(bucket, str)
        if auto and bucket != "auto":
            raise ValueError(f"bucket: expected an index or \"auto\", got {bucket!r}")
        if not torch.cuda.is_available():
            raise lib.NnueHipError("the engine restatement runs on the GPU only (no CPU fallback in this build)")
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        r = _Reader(Path(path).read_bytes())
        if r.data[:4] != b"NNUE":
            raise EngineFormatError("Invalid magic number")
        r.off = 4
        version = r.take("I")
        if version != 2:
            raise EngineFormatError(f"Unsupported version: {version}")
        h = {}
        h["num_features"], h["l1"], h["l2"], h["l3"], h["buckets"] = r.take("5I")
        h["nnue2score"], h["quantized_one"], h["threshold"] = r.take("3f")
        r.take("I")  # layer type
        h["conv_scale"] = r.take("f")
        oc, ic, kh, kw = r.take("4I")
        if ic != 3 or kh != 3 or kw != 3 or oc <= 0:
            raise EngineFormatError("Failed to load conv layer")
        t = {"conv_w": r.array(np.int8, oc * 27)}
        if r.take("I") != oc:
            raise EngineFormatError("Failed to load conv layer")
        t["conv_b"] = r.array(np.int32, oc)
        if h["num_features"] == 0 or h["num_features"] % oc:
            raise EngineFormatError("Invalid feature/channel configuration")
        g = int(np.sqrt(h["num_features"] // oc))
        if g * g * oc != h["num_features"]:
            raise EngineFormatError("Invalid feature grid calculation")
        h["oc"], h["grid"] = oc, g
        r.take("f")  # ft scale (unused by the engine's forward)
        f, l1 = r.take("2I")
        if f != h["num_features"] or l1 != h["l1"]:
            raise EngineFormatError("Feature transformer architecture mismatch")
        t["ft_w"] = r.array(np.int16, f * l1)
        if r.take("I") != l1:
            raise EngineFormatError("Failed to load feature transformer")
        t["ft_b"] = r.array(np.int32, l1)
        if h["buckets"] < 1:
            raise EngineFormatError("no layer stack in the file")
        chosen = 0 if auto or bucket >= h["buckets"] else bucket  # nnue_engine.cpp:705-707
        packed = []
        for i in range(h["buckets"]):
            scales = r.take("4f")
            o, n = r.take("2I")
            if n != h["l1"] or o - 1 != h["l2"]:
                raise EngineFormatError("Layer stack architecture mismatch")
            l1_w, l1_b = r.array(np.int8, o * n), r.array(np.int32, r.take("I"))
            o, n = r.take("2I")
            if n != h["l1"] or o <= h["l2"]:
                raise EngineFormatError(f"Failed to load layer stack {i}")
            r.array(np.int8, o * n)
            r.array(np.int32, r.take("I"))  # factoriser: not on the multiclass path
            o, n = r.take("2I")
            if n != 2 * h["l2"] or o != h["l3"]:
                raise EngineFormatError("Layer stack architecture mismatch")
            l2_w, l2_b = r.array(np.int8, o * n), r.array(np.int32, r.take("I"))
            o, n = r.take("2I")
            if n != h["l3"] or o < 1:
                raise EngineFormatError(f"Invalid output layer dimensions: {n} -> {o}")
            out_w, out_b = r.array(np.int8, o * n), r.array(np.int32, r.take("I"))
            if i == chosen:
                h["l1_scale"], h["l2_scale"], h["out_scale"], _ = scales
                h["classes"] = o
                t.update(l1_w=l1_w, l1_b=l1_b, l2_w=l2_w, l2_b=l2_b, out_w=out_w, out_b=out_b)
            if auto:
                if o != h["classes"]:
                    raise EngineFormatError(f"layer stack {i} has {o} classes, stack 0 has {h['classes']}")
                if (l1_b.size, l2_b.size, out_b.size) != (h["l2"] + 1, h["l3"], o):
                    raise EngineFormatError(f"layer stack {i}: bias lengths {(l1_b.size, l2_b.size, out_b.size)} != "
                                            f"{(h['l2'] + 1, h['l3'], o)}")
                packed.append((scales[:3], dict(l1_w=l1_w, l1_b=l1_b, l2_w=l2_w, l2_b=l2_b, out_w=out_w, out_b=out_b)))
        if not auto:
            return EngineModel(h, t, device)
        if len(packed) > 64:
            raise EngineFormatError(f"{len(packed)} layer stacks: per-image selection takes at most 64")
        for k in _STACK_TENSORS:
            t[k] = np.stack([tensors[k] for _, tensors in packed])
        return EngineModel(h, t, device, np.array([sc for sc, _ in packed], dtype=np.float32))

    # ---- from a live model ---------------------------------------------------------------------
    @staticmethod
    def _arch(model) -> dict:
        """Sizes of an ``nnue.NNUE`` under the header's names (what ``load`` reads from the file ``serialize_model`` writes)."""
        w = model.input.weight
        return {"num_features": int(w.shape[0]), "l1": int(w.shape[1]), "l2": int(model.l2_size), "l3": int(model.l3_size),
                "buckets": int(model.num_ls_buckets), "oc": int(model.conv.weight.shape[0]), "classes": int(model.num_classes)}

    @staticmethod
    def _scalars(model) -> dict:
        """The header scalars, formed with the expressions of ``NNUE.get_quantized_model_data`` (nnue.py:541-588) on the
        model's own device: the threshold's float32 mean is the one the file would carry."""
        from serialize import QUANT_SCALE
        return {"nnue2score": model.nnue2score.item(), "quantized_one": 127.0,
                "threshold": float(model.visual_threshold.detach().mean().cpu().item()), "conv_scale": QUANT_SCALE,
                "l1_scale": QUANT_SCALE, "l2_scale": QUANT_SCALE, "out_scale": QUANT_SCALE}

    def _quantize_from(self, model, check: bool) -> None:
        """The one launch: every engine tensor from the model's parameters (padding included; conv_b stays zero)."""
        a, b, c = model.classifier._linears()
        src = [lib._need(p.detach(), torch.float32, name) for name, p in (
            ("conv.weight", model.conv.weight), ("input.weight", model.input.weight), ("input.bias", model.input.bias),
            ("classifier.0.weight", a.weight), ("classifier.0.bias", a.bias), ("classifier.2.weight", b.weight),
            ("classifier.2.bias", b.bias), ("classifier.4.weight", c.weight), ("classifier.4.bias", c.bias))]
        h = self.header
        if not self._bad_known_zero:  # after an unchecked call, or one that raised
            self._bad.zero_()
        self._bad_known_zero = False
        lib._call("nnue_engine_quantize_model", *[t.data_ptr() for t in src], h["oc"], h["num_features"], h["l1"], h["l2"], h["l3"],
                  h["classes"], h["buckets"], self._stack_index, ctypes.addressof(self._c),
                  None if self._stacks is None else ctypes.addressof(self._stacks), self._bad.data_ptr(), lib._stream(src[1]))
        if self._planes is not None:  # the matrix form's planes follow the table: same stream, same memory, nothing allocated
            self._pack_planes(lib._stream(src[1]))
        if check:
            bad = int(self._bad.item())  # one scalar, once per call
            if bad:
                raise ValueError(f"{bad} parameter(s) are not finite or do not fit the engine's integers (written as 0)")
            self._bad_known_zero = True

    @classmethod
    def from_model(cls, model, bucket: Union[int, str, None] = None, check: bool = True) -> "EngineModel":
        """What ``EngineModel.load`` returns for the file ``serialize_model`` would write for ``model`` (an ``nnue.NNUE`` on the
        GPU), built on the device in one launch; the model -- parameters, ``training`` flag, gradients -- is not changed.
        bucket: None = "auto" for a model with several layer stacks, else 0; an index keeps that stack (``load``'s rule for
        one the model lacks).  check: read back the count of parameters that are not finite (or biases beyond int32 once
        scaled; both are written as 0) and raise ValueError when it is not zero."""
        if isinstance(bucket, str) and bucket != "auto":
            raise ValueError(f"bucket: expected an index, None or \"auto\", got {bucket!r}")
        if not torch.cuda.is_available():
            raise lib.NnueHipError("the engine restatement runs on the GPU only (no CPU fallback in this build)")
        import nnue
        if not isinstance(model, nnue.NNUE):
            raise TypeError(f"from_model: expected an nnue.NNUE, got {type(model).__name__}")
        device = lib._need(model.input.weight.detach(), torch.float32, "input.weight").device
        h = cls._arch(model)
        k = h["buckets"]
        auto = bucket == "auto" or (bucket is None and k > 1)
        if not auto and bucket is not None and bucket < 0:
            raise ValueError(f"bucket: expected a non-negative index, got {bucket}")
        if h["num_features"] % h["oc"]:
            raise EngineFormatError("Invalid feature/channel configuration")
        g = int(np.sqrt(h["num_features"] // h["oc"]))
        if g * g * h["oc"] != h["num_features"]:
            raise EngineFormatError("Invalid feature grid calculation")
        h["grid"] = g
        h.update(cls._scalars(model))
        f, l1, l2, l3, c, oc = h["num_features"], h["l1"], h["l2"], h["l3"], h["classes"], h["oc"]
        lead = (k,) if auto else ()
        shapes = {"conv_w": ((oc * 27,), torch.int8), "conv_b": ((oc,), torch.int32), "ft_w": ((f * l1,), torch.int16),
                  "ft_b": ((l1,), torch.int32), "l1_w": (lead + ((l2 + 1) * l1,), torch.int8), "l1_b": (lead + (l2 + 1,), torch.int32),
                  "l2_w": (lead + (l3 * 2 * l2,), torch.int8), "l2_b": (lead + (l3,), torch.int32),
                  "out_w": (lead + (c * l3,), torch.int8), "out_b": (lead + (c,), torch.int32)}
        tensors = {name: torch.zeros(shape, dtype=dtype, device=device) for name, (shape, dtype) in shapes.items()}
        scales = np.full((k, 3), h["conv_scale"], dtype=np.float32) if auto else None
        engine = cls(h, tensors, device, scales, table_planes=1)  # the quantiser clamps the table to +-127
        engine._stack_index = 0 if auto or bucket is None or bucket >= k else int(bucket)  # nnue_engine.cpp:705-707
        engine._bad = torch.zeros((1,), dtype=torch.int32, device=device)
        engine._bad_known_zero = True
        engine._quantize_from(model, check)
        return engine

    def requantize(self, model, check: bool = True) -> None:
        """``from_model`` again, into the tensors this engine already holds: no allocation, every ``data_ptr()`` unchanged (a
        captured graph over ``evaluate_logits`` stays valid; the matrix form's planes, once prepared, are re-packed in place
        right after the quantise launch), the by-value scalars refreshed.  Streams of this model refresh
        their accumulators on their next step.  A model of another architecture or stack count is refused."""
        if self._bad is None:
            raise ValueError("requantize: this engine was loaded from a file; build it with EngineModel.from_model")
        arch = self._arch(model)
        mine = {k: self.header[k] for k in arch}
        if arch != mine:
            raise ValueError(f"requantize: the model is {arch}, this engine {mine}")
        lib._need(model.input.weight.detach(), torch.float32, "input.weight")
        scalars = self._scalars(model)
        self.header.update(scalars)
        self._c.threshold = scalars["threshold"]
        self.generation += 1
        self._quantize_from(model, check)

    def stream(self, num_streams: int) -> "EngineStream":
        """Incremental evaluation of ``num_streams`` frame sequences (see EngineStream)."""
        return EngineStream(self, num_streams)

    def _u8_frames(self, images_u8, indices, layout, mean, std, what: str, count: Optional[int] = None):
        """The host descriptor of a u8 call: (struct, the tensors it points at, B, H, W).  ``count``: the number of frames the
        call needs (a stream's S), None = whatever the arguments name."""
        if not isinstance(images_u8, torch.Tensor):
            raise TypeError(f"{what}: expected a tensor, got {type(images_u8).__name__}")
        if images_u8.dtype != torch.uint8:
            raise TypeError(f"{what}: expected torch.uint8, got {images_u8.dtype}")
        if not self._on_device(images_u8):
            raise ValueError(f"{what}: tensor is on {images_u8.device}, the model on {self.device} (no CPU fallback in this build)")
        if images_u8.dim() != 4 or images_u8.shape[3] != 3 or min(images_u8.shape) < 1:
            raise ValueError(f"{what}: expected uint8 [N,H,W,3], got {tuple(images_u8.shape)}")
        if not images_u8.is_contiguous():
            raise ValueError(f"{what}: the frames must be contiguous (a view with a storage offset is fine)")
        if layout not in U8_LAYOUTS:
            raise ValueError(f"{what}: layout must be one of {tuple(U8_LAYOUTS)}, got {layout!r}")
        mean255, inv_std255 = u8_constants(mean, std)
        n, h, w = (int(v) for v in images_u8.shape[:3])
        if indices is None:
            b = n
        else:
            if not isinstance(indices, torch.Tensor) or indices.dtype != torch.int64:
                raise TypeError(f"{what}: indices must be an int64 tensor")
            if not self._on_device(indices) or indices.dim() != 1 or indices.numel() < 1:
                raise ValueError(f"{what}: indices must be a device tensor of shape (B,), got {tuple(indices.shape)} on {indices.device}")
            indices = indices.contiguous()
            b = int(indices.numel())
        if count is not None and b != count:
            raise ValueError(f"{what}: expected {count} frames, got {b}")
        c = _CU8Frames()
        c.data, c.indices, c.count, c.layout = images_u8.data_ptr(), lib._ptr(indices) or None, n, U8_LAYOUTS[layout]
        c.mean255[:], c.inv_std255[:] = mean255.tolist(), inv_std255.tolist()
        return c, (images_u8, indices), b, h, w

    def evaluate_logits_u8(self, images_u8: torch.Tensor, indices: Optional[torch.Tensor] = None, layout: str = "chw",
                           mean=None, std=None, stacks: Optional[torch.Tensor] = None, return_stacks: bool = False,
                           path: Optional[str] = None):
        """``evaluate_logits`` straight from uint8 frames: ``images_u8`` is a contiguous uint8 device tensor [N,H,W,3] (the store
        of a ``GpuImageDataset``, or frames; a view with a storage offset is fine), ``indices`` a device int64 [B] into it
        (clamped to [0, N) as ``lib.load_batch`` clamps them) or None for all N in order.
        layout="chw" (default): the float buffer of every image is the memory ``lib.load_batch(augment=False)`` writes for it,
        a CHW tensor handed to the engine flat as the reference does (evaluate.py:150-161) -- with the default ``mean`` /
        ``std`` (the ImageNet constants, data/datasets.py:366-369) the results are bit-identical to
        ``evaluate_logits(lib.load_batch(images_u8, labels, indices, False, 0, 0)[0])``.  layout="hwc": the frame's bytes are
        what the engine's HWC indexing means, x[i] = norm(u[i], i % 3).  norm(v, c) = (v - 255 mean[c]) / (255 std[c]) in
        float32 (include/nnue_hip.h has the exact expression).  ``stacks``, ``return_stacks`` and ``path`` as ``evaluate_logits``.
        TypeError for a tensor that is not uint8 / indices that are not int64, ValueError for shape, device, contiguity, layout
        and constants."""
        src, keep, b, h, w = self._u8_frames(images_u8, indices, layout, mean, std, "images_u8")
        stacks = self._stack_arg(stacks, b, "evaluate_logits_u8")
        logits, density, _, used = self._outputs(b, zero_stacks=return_stacks)
        st, used_ptr = (None, None) if self._stacks is None else (ctypes.addressof(self._stacks), used.data_ptr())
        if self._path(path, b, "evaluate_logits_u8") == "matrix":
            self.prepare_matrix()
            scratch = self._matrix_scratch_for(b)
            lib._call("nnue_engine_evaluate_logits_matrix_u8", ctypes.addressof(self._c), st, self._planes.data_ptr(),
                      self.table_planes, ctypes.addressof(src), b, h, w, lib._ptr(stacks) or None, logits.data_ptr(),
                      density.data_ptr(), used_ptr, scratch.data_ptr(), scratch.numel(), lib._stream(images_u8))
        else:
            scratch = self._scratch_for(b)
            lib._call("nnue_engine_evaluate_logits_u8", ctypes.addressof(self._c), st, ctypes.addressof(src), b, h, w,
                      lib._ptr(stacks) or None, logits.data_ptr(), density.data_ptr(), used_ptr, scratch.data_ptr(), scratch.numel(),
                      lib._stream(images_u8))
        del keep
        return (logits, density, used) if return_stacks else (logits, density)

    def _frames(self, images: torch.Tensor, height: Optional[int], width: Optional[int]) -> Tuple[int, int, int]:
        if images.dim() == 4:
            b, h, w = images.shape[0], images.shape[2], images.shape[3]
            if images.shape[1] != 3:
                raise ValueError(f"images: expected [B,3,H,W], got {tuple(images.shape)}")
        elif images.dim() == 2 and height and width and images.shape[1] == 3 * height * width:
            b, h, w = images.shape[0], height, width
        else:
            raise ValueError("images: expected [B,3,H,W], or [B,3*H*W] with height and width")
        return b, h, w

    # ---- the matrix form -------------------------------------------------------------------------
    def _pack_planes(self, stream: int) -> None:
        lib._call("nnue_engine_pack_table", ctypes.addressof(self._c), self.table_planes, self._planes.data_ptr(),
                  self._planes.numel(), self._misfit.data_ptr(), stream)

    def matrix_supported(self, batch: int = 1) -> bool:
        """Whether the matrix form can run this model (include/nnue_hip.h: nnue_engine_matrix_supported)."""
        return bool(lib.load().nnue_engine_matrix_supported(ctypes.byref(self._c), int(batch), self.table_planes or 1))

    def prepare_matrix(self) -> None:
        """Packs the int8 planes of the table for the matrix form (done by the first matrix call otherwise).  One launch; a
        table whose range the host does not know is packed as one plane first and its misfit count read back, here only."""
        if self._planes is not None:
            return
        if not self.matrix_supported():
            raise lib.NnueHipError("prepare_matrix: the matrix form does not support this model "
                                   f"(num_features={self.header['num_features']}, L1={self.header['l1']})")
        if torch.cuda.is_current_stream_capturing():
            raise lib.NnueHipError("prepare_matrix: call it before the capture (it allocates and may read a counter back)")
        L = lib.load()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            self._misfit = torch.zeros((1,), dtype=torch.int32, device=self.device)
            probe = self.table_planes is None
            if probe:
                self.table_planes = 1
            try:
                nbytes = int(L.nnue_engine_table_planes_bytes(ctypes.byref(self._c), self.table_planes))
                self._planes = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
                self._pack_planes(stream)
                if probe and int(self._misfit.item()):
                    self.table_planes = 2
                    nbytes = int(L.nnue_engine_table_planes_bytes(ctypes.byref(self._c), 2))
                    self._planes = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
                    self._pack_planes(stream)
            except Exception:
                self._planes = None
                if probe:
                    self.table_planes = None
                raise

    def _path(self, path: Optional[str], b: int, what: str) -> str:
        """"gather" or "matrix" for a call on images (None = NNUE_ENGINE_PATH, default auto)."""
        if path is None:
            path = os.environ.get("NNUE_ENGINE_PATH", "auto")
        if path not in _PATHS:
            raise ValueError(f"{what}: path must be one of {_PATHS}, got {path!r}")
        if path == "auto":
            ready = self._planes is not None or not torch.cuda.is_current_stream_capturing()
            big = b * int(self.header["num_features"]) >= _MATRIX_MIN_MAP_BYTES
            return "matrix" if big and ready and self.matrix_supported(b) else "gather"
        if path == "matrix" and not self.matrix_supported(b):
            raise lib.NnueHipError(f"{what}: path=\"matrix\" does not support this model "
                                   f"(num_features={self.header['num_features']}, L1={self.header['l1']})")
        return path

    def _evaluate_matrix(self, images: Optional[torch.Tensor], active: Optional[torch.Tensor], b: int, h: int, w: int,
                         stacks: Optional[torch.Tensor], return_stacks: bool):
        self.prepare_matrix()
        scratch = self._matrix_scratch_for(b)
        logits, density, _, used = self._outputs(b, zero_stacks=return_stacks)
        src = images if images is not None else active
        st, used_ptr = (None, 0) if self._stacks is None else (ctypes.addressof(self._stacks), used.data_ptr())
        lib._call("nnue_engine_evaluate_logits_matrix", ctypes.addressof(self._c), st, self._planes.data_ptr(), self.table_planes,
                  lib._ptr(images), lib._ptr(active), b, h, w, lib._ptr(stacks), logits.data_ptr(), density.data_ptr(), used_ptr,
                  scratch.data_ptr(), scratch.numel(), lib._stream(src))
        return (logits, density, used) if return_stacks else (logits, density)

    def evaluate_features(self, active: torch.Tensor, stacks: Optional[torch.Tensor] = None, return_stacks: bool = False,
                          path: Optional[str] = None):
        """``evaluate_logits`` from active-feature maps: bool or uint8 [B, num_features] on the device, non-zero = on, every id
        counts (the rule of ``EngineStream.step_features``; no per-cell channel mask).  Always the matrix form -- the gather
        kernels take no feature map -- so path="gather" raises ValueError and an unsupported model NnueHipError."""
        if path is None:
            path = os.environ.get("NNUE_ENGINE_PATH", "auto")
            path = "matrix" if path == "gather" else path  # the variable chooses among forms that exist for the call
        if path not in _PATHS:
            raise ValueError(f"evaluate_features: path must be one of {_PATHS}, got {path!r}")
        if path == "gather":
            raise ValueError("evaluate_features: the gather kernels have no feature-map input; use path=\"matrix\"")
        if not isinstance(active, torch.Tensor):
            raise TypeError(f"active: expected a tensor, got {type(active).__name__}")
        if active.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"active: expected dtype torch.bool or torch.uint8, got {active.dtype}")
        if not self._on_device(active):
            raise ValueError(f"active: tensor is on {active.device}, the model on {self.device} (no CPU fallback in this build)")
        f = int(self.header["num_features"])
        if active.dim() != 2 or active.shape[0] < 1 or active.shape[1] != f:
            raise ValueError(f"active: expected shape (B, {f}), got {tuple(active.shape)}")
        b = int(active.shape[0])
        self._path("matrix", b, "evaluate_features")
        stacks = self._stack_arg(stacks, b, "evaluate_features")
        return self._evaluate_matrix(None, active.contiguous(), b, 0, 0, stacks, return_stacks)

    def _matrix_scratch_for(self, b: int) -> torch.Tensor:
        """The matrix form's own buffer: growing it never moves the scratch a captured gather call points at."""
        need = int(lib.load().nnue_engine_matrix_scratch(ctypes.byref(self._c), b, self.table_planes))
        if self._matrix_scratch is None or self._matrix_scratch.numel() < need:
            self._matrix_scratch = torch.empty((max(16, need),), dtype=torch.uint8, device=self.device)
        return self._matrix_scratch

    def _scratch_for(self, b: int) -> torch.Tensor:
        need = int(lib.load().nnue_engine_scratch(ctypes.byref(self._c), b))
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty((max(16, need),), dtype=torch.uint8, device=self.device)
        return self._scratch

    def evaluate_logits(self, images: torch.Tensor, height: Optional[int] = None, width: Optional[int] = None,
                        stacks: Optional[torch.Tensor] = None, return_stacks: bool = False, path: Optional[str] = None):
        """(logits [B, C] float32, density [B] float32).  ``images`` is what the reference hands the engine: per sample
        a flat buffer of 3*H*W floats which the engine indexes as HWC -- for a [B,3,H,W] tensor that is its memory as
        it stands (evaluate.py:150-161 passes shape[1], shape[2] as H, W), which is reproduced, not corrected.
        A model loaded with bucket="auto" puts every image through the stack ``stack_of`` gives for its active-feature
        count, or through ``stacks`` (device int32/int64 [B]; outside [0, K) = stack 0).  return_stacks: also return the
        stack every image used, int32 [B] (zeros for a single-stack model).
        path: "gather" (one workgroup per image adds its active table rows), "matrix" (one product on the int8 matrix
        unit), or "auto" (matrix from the measured crossover upwards where the model allows it; inside a stream capture only
        with the planes already prepared); None reads NNUE_ENGINE_PATH, default auto.  The bits are the same either way."""
        images = lib._need(images, torch.float32, "images")
        b, h, w = self._frames(images, height, width)
        stacks = self._stack_arg(stacks, b, "evaluate_logits")
        if self._path(path, b, "evaluate_logits") == "matrix":
            return self._evaluate_matrix(images, None, b, h, w, stacks, return_stacks)
        self._scratch_for(b)
        logits, density, _, used = self._outputs(b, zero_stacks=return_stacks)
        if self._stacks is None:
            lib._call("nnue_engine_evaluate_logits", ctypes.addressof(self._c), images.data_ptr(), b, h, w, logits.data_ptr(),
                      density.data_ptr(), self._scratch.data_ptr(), self._scratch.numel(), lib._stream(images))
        else:
            lib._call("nnue_engine_evaluate_logits_stacks", ctypes.addressof(self._c), ctypes.addressof(self._stacks),
                      images.data_ptr(), b, h, w, lib._ptr(stacks), logits.data_ptr(), density.data_ptr(), used.data_ptr(),
                      self._scratch.data_ptr(), self._scratch.numel(), lib._stream(images))
        return (logits, density, used) if return_stacks else (logits, density)


_INT32_MIN, _INT32_MAX = -2 ** 31, 2 ** 31 - 1


def pack_feature_lists(lists, num_streams: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``num_streams`` per-stream id lists (Python sequences, numpy arrays or tensors of integers, any mix, any of them empty) as
    the CSR pair ``EngineStream.update`` takes: (ids int32 [total], offsets int32 [num_streams + 1]) on the CPU; stream b's ids
    are ids[offsets[b]:offsets[b + 1]].  Pure host work, no device is touched.  An id outside int32 becomes -1 (ignored by the
    kernel, never wrapped into the range).  ValueError for another number of lists, for ids that are not integers and for more
    ids than int32 offsets can address."""
    s = int(num_streams)
    if isinstance(lists, (torch.Tensor, np.ndarray, str, bytes)) or not hasattr(lists, "__len__"):
        raise ValueError(f"pack_feature_lists: expected a sequence of {s} id lists, got {type(lists).__name__}")
    if len(lists) != s:
        raise ValueError(f"pack_feature_lists: expected {s} id lists (one per stream), got {len(lists)}")
    parts = []
    for b, ids in enumerate(lists):
        if isinstance(ids, torch.Tensor):
            if ids.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
                raise ValueError(f"pack_feature_lists: list {b} holds {ids.dtype}, expected integer ids")
            a = ids.detach().cpu().numpy()
        else:
            a = np.asarray(ids)
            if a.size == 0:
                a = a.astype(np.int64)
            elif a.dtype.kind not in "iu":
                raise ValueError(f"pack_feature_lists: list {b} holds {a.dtype} values, expected integer ids")
        if a.ndim != 1:
            raise ValueError(f"pack_feature_lists: list {b} has shape {a.shape}, expected one dimension")
        if a.dtype == np.uint64:
            a = np.where(a > _INT32_MAX, np.uint64(_INT32_MAX + 1), a)
        a = a.astype(np.int64)
        parts.append(np.where((a < _INT32_MIN) | (a > _INT32_MAX), -1, a).astype(np.int32))
    offsets = np.zeros(s + 1, dtype=np.int64)
    np.cumsum([p.size for p in parts], out=offsets[1:])
    if offsets[-1] > _INT32_MAX:
        raise ValueError(f"pack_feature_lists: {int(offsets[-1])} ids are more than int32 offsets can address")
    if np.any(np.diff(offsets) < 0):
        raise ValueError("pack_feature_lists: offsets are not monotone")
    ids = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
    return torch.from_numpy(ids.astype(np.int32, copy=False)), torch.from_numpy(offsets.astype(np.int32))


def pack_rect_lists(lists, num_streams: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``num_streams`` per-stream lists of rectangles (each a sequence of 4 integers y0, x0, y1, x1, half-open, in frame pixels;
    any list may be empty) as the CSR pair ``EngineStream.step_u8_regions`` takes: (rects int32 [total, 4], offsets int32
    [num_streams + 1]) on the CPU.  Pure host work.  A coordinate outside int32 is saturated, which leaves the rectangle's
    intersection with any frame where it was.  ValueError for another number of lists and for entries that are not 4 integers."""
    s = int(num_streams)
    if isinstance(lists, (torch.Tensor, np.ndarray, str, bytes)) or not hasattr(lists, "__len__"):
        raise ValueError(f"pack_rect_lists: expected a sequence of {s} rectangle lists, got {type(lists).__name__}")
    if len(lists) != s:
        raise ValueError(f"pack_rect_lists: expected {s} rectangle lists (one per stream), got {len(lists)}")
    parts = []
    for b, rects in enumerate(lists):
        a = rects.detach().cpu().numpy() if isinstance(rects, torch.Tensor) else np.asarray(rects)
        if a.size == 0:
            a = np.zeros((0, 4), dtype=np.int64)
        elif a.dtype.kind not in "iu":
            raise ValueError(f"pack_rect_lists: list {b} holds {a.dtype} values, expected integer coordinates")
        if a.ndim != 2 or a.shape[1] != 4:
            raise ValueError(f"pack_rect_lists: list {b} has shape {a.shape}, expected (n, 4): y0, x0, y1, x1 per rectangle")
        if a.dtype == np.uint64:
            a = np.minimum(a, np.uint64(_INT32_MAX))
        parts.append(np.clip(a.astype(np.int64), _INT32_MIN, _INT32_MAX).astype(np.int32))
    offsets = np.zeros(s + 1, dtype=np.int64)
    np.cumsum([p.shape[0] for p in parts], out=offsets[1:])
    if offsets[-1] > _INT32_MAX:
        raise ValueError(f"pack_rect_lists: {int(offsets[-1])} rectangles are more than int32 offsets can address")
    rects = np.concatenate(parts) if parts else np.zeros((0, 4), dtype=np.int32)
    return torch.from_numpy(rects.astype(np.int32, copy=False)), torch.from_numpy(offsets.astype(np.int32))


class EngineStreamSnapshot:
    """What ``EngineStream.snapshot`` returns: a device copy of the stream state (sets, accumulators, flags), the stacks of the
    last step, and the model generation the accumulators belong to."""

    def __init__(self, model: "EngineModel", num_streams: int, state: torch.Tensor, stacks: torch.Tensor, generation: int,
                 frame_hw: Optional[Tuple[int, int]] = None):
        self.model, self.num_streams, self.state, self.stacks, self.generation = model, num_streams, state, stacks, generation
        self.frame_hw = frame_hw


class EngineStream:
    """S independent frame sequences (for example one per camera) evaluated incrementally on the device: every stream keeps
    the engine's wrapped int16 accumulator and its last active-feature set, and a step applies only the features that
    turned on or off (FeatureTransformer::update_accumulator, nnue_engine.cpp:257-267).  Every step's logits and density
    are bit-identical to ``EngineModel.evaluate_logits`` on the same frames, whatever came before: int16 addition wraps,
    so the order and history of the terms do not matter.  A new stream, one passed to ``reset``, and every stream after the
    model's ``requantize``, is refreshed from the bias on its next step.  ``step`` (images) and ``step_features`` (feature maps) may be mixed on one stream.
    ``update(added, removed)`` takes the two short id lists of the features that turned on and off instead of the whole new state
    (NNUEEvaluator::update_features, nnue_engine.cpp:818-821), so a step costs O(changes); it mixes with the other two, keeps the
    stored sets across a ``requantize`` (it rebuilds the sums once instead of forgetting the sets), and ``refresh`` /
    ``snapshot`` / ``restore`` are the reference's refresh_accumulator and save / restore_accumulator (:792-816).
    ``step_u8_regions(frames_u8, rects)`` derives those lists on the device from the dirty rectangles of uint8 frames.
    On a model loaded with bucket="auto" every step chooses each stream's layer stack from the step's own feature count
    (or takes ``stacks=``, as ``evaluate_logits``); ``stacks`` holds the stacks of the last step, int32 [S]."""

    def __init__(self, model: EngineModel, num_streams: int):
        s = int(num_streams)
        if s <= 0:
            raise ValueError(f"num_streams must be positive, got {num_streams}")
        self.model, self.num_streams = model, s
        self.num_features = int(model.header["num_features"])
        nbytes = int(lib.load().nnue_engine_stream_state_bytes(ctypes.byref(model._c), s))
        # zero-filled = every stream invalid; the first S int32 of the state are the valid flags (include/nnue_hip.h)
        self.state = torch.zeros((nbytes,), dtype=torch.uint8, device=model.device)
        self._valid = self.state[:4 * s].view(torch.int32)
        self.stacks = torch.zeros((s,), dtype=torch.int32, device=model.device)
        self._generation = model.generation
        self._frame_hw: Optional[Tuple[int, int]] = None  # H x W of the last step that took frames (step, step_u8, step_u8_regions)
        self._unit_offsets: Optional[torch.Tensor] = None  # arange(S + 1) int32, for one rectangle per stream

    def reset(self, streams: Optional[Iterable[int]] = None) -> None:
        """Marks all streams, or the given indices, for a refresh from the bias on the next step."""
        if streams is None:
            self._valid.fill_(0)
            self._frame_hw = None  # no stored set is left to belong to a frame size
            return
        idx = sorted({int(i) for i in streams})
        if idx and (idx[0] < 0 or idx[-1] >= self.num_streams):
            raise ValueError(f"reset: stream indices must lie in [0, {self.num_streams})")
        for i in idx:
            self._valid[i:i + 1].fill_(0)

    def _check(self, t, what: str, dtypes) -> None:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: expected a tensor, got {type(t).__name__}")
        if t.dtype not in dtypes:
            raise ValueError(f"{what}: expected dtype {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
        if not self.model._on_device(t):
            raise ValueError(f"{what}: tensor is on {t.device}, the stream's state on {self.model.device} "
                             "(no CPU fallback in this build)")
        if t.dim() < 1 or t.shape[0] != self.num_streams:
            raise ValueError(f"{what}: expected {self.num_streams} streams in dim 0, got shape {tuple(t.shape)}")

    def _run(self, images: Optional[torch.Tensor], active: Optional[torch.Tensor], h: int, w: int,
             stacks: Optional[torch.Tensor] = None, u8=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        m, s = self.model, self.num_streams
        if self._generation != m.generation:  # the model was requantised: the accumulators are sums over the old table
            self._valid.fill_(0)
            self._generation = m.generation
        stacks = m._stack_arg(stacks, s, "EngineStream")
        logits, density, changed, used = m._outputs(s, changed=True)
        scratch = m._scratch_for(s) if images is not None else None
        src = images if images is not None else active
        if images is not None:
            self._frame_hw = (h, w)
        if u8 is not None:  # (descriptor, the uint8 frames): `images` is those frames, the state and the outputs are the same
            st, used_ptr = (None, None) if m._stacks is None else (ctypes.addressof(m._stacks), used.data_ptr())
            lib._call("nnue_engine_stream_step_u8", ctypes.addressof(m._c), st, ctypes.addressof(u8), s, h, w, lib._ptr(stacks) or None,
                      self.state.data_ptr(), self.state.numel(), logits.data_ptr(), density.data_ptr(), changed.data_ptr(), used_ptr,
                      scratch.data_ptr(), scratch.numel(), lib._stream(src))
            if m._stacks is not None:
                self.stacks = used
        elif m._stacks is None:
            lib._call("nnue_engine_stream_step", ctypes.addressof(m._c), lib._ptr(images), lib._ptr(active), s, h, w,
                      self.state.data_ptr(), self.state.numel(), logits.data_ptr(), density.data_ptr(), changed.data_ptr(),
                      lib._ptr(scratch), 0 if scratch is None else scratch.numel(), lib._stream(src))
        else:
            lib._call("nnue_engine_stream_step_stacks", ctypes.addressof(m._c), ctypes.addressof(m._stacks), lib._ptr(images),
                      lib._ptr(active), s, h, w, lib._ptr(stacks), self.state.data_ptr(), self.state.numel(), logits.data_ptr(),
                      density.data_ptr(), changed.data_ptr(), used.data_ptr(), lib._ptr(scratch),
                      0 if scratch is None else scratch.numel(), lib._stream(src))
            self.stacks = used
        return logits, density, changed

    def step(self, frames: torch.Tensor, height: Optional[int] = None, width: Optional[int] = None,
             stacks: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """One frame per stream, in the forms ``evaluate_logits`` takes ([S,3,H,W], or [S,3*H*W] with height and width;
        H x W may change between steps).  Returns (logits [S, C] float32, density [S] float32, changed [S] int32): changed
        = features that differ from the stream's previous set, or all active ones on a refresh."""
        self._check(frames, "frames", (torch.float32,))
        _, h, w = self.model._frames(frames, height, width)
        return self._run(frames.contiguous(), None, h, w, stacks)

    def step_u8(self, frames_u8: torch.Tensor, indices: Optional[torch.Tensor] = None, layout: str = "chw", mean=None, std=None,
                stacks: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``step`` from uint8 frames, in the forms ``EngineModel.evaluate_logits_u8`` takes: ``frames_u8`` uint8 [N,H,W,3] on
        the device and ``indices`` int64 [S] into it, or None with N == S (stream s takes frame s).  Returns what ``step``
        returns, on the same state -- bit-identical to ``evaluate_logits_u8`` on the same frames -- and mixes freely with
        ``step``, ``step_features`` and ``update``."""
        src, keep, _, h, w = self.model._u8_frames(frames_u8, indices, layout, mean, std, "frames_u8", count=self.num_streams)
        return self._run(keep[0], None, h, w, stacks, u8=src)

    def step_features(self, active: torch.Tensor, stacks: Optional[torch.Tensor] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """One active-feature map per stream: bool or uint8 [S, num_features] on the device, non-zero = on.  Every id
        counts (the reference's evaluate_incremental(current_features) takes the indices as given)."""
        self._check(active, "active", (torch.bool, torch.uint8))
        if tuple(active.shape) != (self.num_streams, self.num_features):
            raise ValueError(f"active: expected shape {(self.num_streams, self.num_features)}, got {tuple(active.shape)}")
        return self._run(None, active.contiguous(), 0, 0, stacks)

    # ---- sparse add / remove lists ------------------------------------------------------------
    def _csr(self, lists, what: str) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        """One list argument of ``update`` as (ids int32 [n], offsets int32 [S + 1]) on the device, or (None, None)."""
        if lists is None:
            return None, None
        dev, s = self.model.device, self.num_streams
        if isinstance(lists, tuple) and len(lists) == 2 and all(isinstance(t, torch.Tensor) for t in lists):
            ids, offsets = lists  # device CSR: no host work, no synchronisation
            for t, name in ((ids, "ids"), (offsets, "offsets")):
                if t.dtype not in (torch.int32, torch.int64):
                    raise ValueError(f"{what}: {name} must be int32 or int64, got {t.dtype}")
                if not self.model._on_device(t):
                    raise ValueError(f"{what}: {name} is on {t.device}, the stream's state on {dev} (no CPU fallback in this build)")
            if ids.dim() != 1 or ids.numel() > _INT32_MAX:
                raise ValueError(f"{what}: ids must have one dimension and fewer than 2^31 elements, got shape {tuple(ids.shape)}")
            if tuple(offsets.shape) != (s + 1,):
                raise ValueError(f"{what}: offsets must have shape ({s + 1},), got {tuple(offsets.shape)}")
            if ids.dtype == torch.int64:  # an id beyond int32 must not wrap into the range
                ids = torch.where((ids >= _INT32_MIN) & (ids <= _INT32_MAX), ids, torch.full_like(ids, -1)).to(torch.int32)
            if offsets.dtype == torch.int64:  # the kernel clips to [0, n] with n < 2^31: saturating keeps every clip where it was
                offsets = offsets.clamp(_INT32_MIN, _INT32_MAX).to(torch.int32)
            return ids.contiguous(), offsets.contiguous()
        ids, offsets = pack_feature_lists(lists, s)
        packed = torch.cat((offsets, ids)).to(dev)  # one copy
        return packed[s + 1:], packed[:s + 1]

    def _update(self, added, removed, stacks: Optional[torch.Tensor], fresh: bool
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        m, s = self.model, self.num_streams
        a_ids, a_off = self._csr(added, "added")
        r_ids, r_off = self._csr(removed, "removed")
        stacks = m._stack_arg(stacks, s, "EngineStream")
        logits, density, changed, used = m._outputs(s, changed=True)
        if fresh:
            self._valid.fill_(0)
        # after a requantize the stored sets are still right and only the sums are stale: one rebuild instead of a reset
        rebuild = int(self._generation != m.generation)
        lib._call("nnue_engine_stream_update", ctypes.addressof(m._c), None if used is None else ctypes.addressof(m._stacks),
                  lib._ptr(a_ids), lib._ptr(a_off), 0 if a_ids is None else a_ids.numel(), lib._ptr(r_ids), lib._ptr(r_off),
                  0 if r_ids is None else r_ids.numel(), s, rebuild, lib._ptr(stacks), self.state.data_ptr(), self.state.numel(),
                  logits.data_ptr(), density.data_ptr(), changed.data_ptr(), lib._ptr(used), lib._stream(self.state))
        self._generation = m.generation
        if used is not None:
            self.stacks = used
        return logits, density, changed

    def update(self, added, removed=None, stacks: Optional[torch.Tensor] = None
               ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """One step from the features that turned on (``added``) and off (``removed``) per stream -- O(changes), where ``step``
        and ``step_features`` read the whole new state.  Each list is a tuple ``(ids, offsets)`` of device tensors -- ids int32 or
        int64 [n], offsets int32 or int64 [S + 1], stream b's ids being ids[offsets[b]:offsets[b + 1]]; no host work, no
        synchronisation, fit for a stream capture -- or a sequence of S per-stream id sequences or tensors, packed on the host
        (``pack_feature_lists``) and copied once; None = empty.  A tuple of two tensors is always read as (ids, offsets): hand
        per-stream tensors over in a list.  Set semantics: new = (old - removed) | added; ids outside [0, num_features), removed ids
        that are off, added ids that are on and duplicates are ignored, an id in both lists ends up on; offsets are clipped to the
        id buffer.  A stream that is not valid takes ``added`` as its whole set.  Returns what ``step`` returns, bit-identical to
        ``evaluate_features`` on the resulting sets; ``stacks`` as in ``step``."""
        return self._update(added, removed, stacks, False)

    def refresh(self, features, stacks: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``reset()`` followed by ``update(features)``: every stream's set becomes its list
        (NNUEEvaluator::refresh_accumulator, nnue_engine.cpp:806-816).  A refused call resets nothing."""
        return self._update(features, None, stacks, True)

    # ---- dirty rectangles of uint8 frames -------------------------------------------------------
    def _rect_csr(self, rects) -> Tuple[torch.Tensor, torch.Tensor]:
        """The ``rects`` argument of ``step_u8_regions`` as (rects int32 [R, 4], offsets int32 [S + 1]) on the device."""
        dev, s = self.model.device, self.num_streams
        what = "rects"
        pair = isinstance(rects, tuple) and len(rects) == 2 and all(isinstance(t, torch.Tensor) for t in rects)
        if isinstance(rects, torch.Tensor) or pair:  # device forms: no host work, no synchronisation
            boxes, offsets = rects if pair else (rects, None)
            if boxes.dtype != torch.int32:
                raise ValueError(f"{what}: rectangles must be int32, got {boxes.dtype}")
            if not self.model._on_device(boxes):
                raise ValueError(f"{what}: tensor is on {boxes.device}, the stream's state on {dev} (no CPU fallback in this build)")
            if boxes.dim() != 2 or boxes.shape[1] != 4 or boxes.shape[0] > _INT32_MAX:
                raise ValueError(f"{what}: expected shape (R, 4) -- y0, x0, y1, x1 per rectangle -- got {tuple(boxes.shape)}")
            if offsets is None:
                if boxes.shape[0] != s:
                    raise ValueError(f"{what}: a single tensor holds one rectangle per stream, expected shape ({s}, 4), got "
                                     f"{tuple(boxes.shape)}; pass (rects, offsets) for another count")
                if self._unit_offsets is None:
                    self._unit_offsets = torch.arange(s + 1, dtype=torch.int32, device=dev)
                offsets = self._unit_offsets
            else:
                if offsets.dtype not in (torch.int32, torch.int64):
                    raise ValueError(f"{what}: offsets must be int32 or int64, got {offsets.dtype}")
                if not self.model._on_device(offsets):
                    raise ValueError(f"{what}: offsets are on {offsets.device}, the stream's state on {dev}")
                if tuple(offsets.shape) != (s + 1,):
                    raise ValueError(f"{what}: offsets must have shape ({s + 1},), got {tuple(offsets.shape)}")
                if offsets.dtype == torch.int64:  # saturating keeps every clip to [0, R] where it was
                    offsets = offsets.clamp(_INT32_MIN, _INT32_MAX).to(torch.int32)
            return boxes.contiguous(), offsets.contiguous()
        boxes, offsets = pack_rect_lists(rects, s)
        packed = torch.cat((offsets, boxes.reshape(-1))).to(dev)  # one copy
        return packed[s + 1:].view(-1, 4), packed[:s + 1]

    def step_u8_regions(self, frames_u8: torch.Tensor, rects, indices: Optional[torch.Tensor] = None, mean=None, std=None,
                        stacks: Optional[torch.Tensor] = None, layout: str = "hwc"
                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``step_u8(layout="hwc")`` from the dirty rectangles of the frames: the conv is re-run only on the grid cells whose
        3 x 3 window touches a rectangle and only the table rows that flipped are walked -- O(touched cells + flips) per stream,
        no conv scratch (include/nnue_hip.h: nnue_engine_stream_step_u8_regions has the definition as set arithmetic).
        ``frames_u8`` and ``indices`` as ``step_u8``.  ``rects``: rectangles y0, x0, y1, x1, half-open, in frame pixels, as an
        int32 device tensor [S, 4] (one per stream), a tuple ``(rects int32 [R, 4], offsets int32 or int64 [S + 1])`` of device
        tensors (stream s owns rects[offsets[s]:offsets[s + 1]]) -- both without host work, fit for a stream capture -- or a
        sequence of S per-stream sequences of 4-tuples, packed on the host (``pack_rect_lists``) and copied once.
        If the frames differ from those behind the stored sets only inside the rectangles, the result is bit-identical to
        ``step_u8(frames_u8, indices, layout="hwc")``; otherwise only the touched cells' features are replaced.  Overlapping,
        repeated, empty, inverted and outside rectangles are harmless; a stream without rectangles returns its previous logits
        and changed == 0; a stream that is not valid (new, ``reset``, or after ``requantize``) is evaluated over its whole frame.
        Only layout="hwc" exists: under "chw" a pixel rectangle does not map to neighbouring taps.  ValueError for that, for a
        wrong dtype or shape of ``rects``, and for an H x W other than that of the stream's last step that took frames
        (``reset()`` of all streams, or a whole-frame step, changes the size)."""
        if layout != "hwc":
            raise ValueError(f"step_u8_regions: layout must be \"hwc\", got {layout!r} (under \"chw\" a pixel rectangle does not "
                             "map to neighbouring taps)")
        m, s = self.model, self.num_streams
        src, keep, _, h, w = m._u8_frames(frames_u8, indices, layout, mean, std, "frames_u8", count=s)
        boxes, offsets = self._rect_csr(rects)
        stale = self._generation != m.generation  # the model was requantised: sets and sums belong to the old tensors
        if not stale and self._frame_hw is not None and self._frame_hw != (h, w):
            raise ValueError(f"step_u8_regions: frames are {h}x{w}, the stream's last frame step was {self._frame_hw[0]}x"
                             f"{self._frame_hw[1]}: the stored sets belong to another grid (reset() all streams, or take a "
                             "whole-frame step)")
        if stale:
            self._valid.fill_(0)
            self._generation = m.generation
        stacks = m._stack_arg(stacks, s, "EngineStream")
        logits, density, changed, used = m._outputs(s, changed=True)
        st, used_ptr = (None, None) if m._stacks is None else (ctypes.addressof(m._stacks), used.data_ptr())
        lib._call("nnue_engine_stream_step_u8_regions", ctypes.addressof(m._c), st, ctypes.addressof(src), s, h, w,
                  lib._ptr(boxes) or None, lib._ptr(offsets) or None, int(boxes.shape[0]), lib._ptr(stacks) or None,
                  self.state.data_ptr(), self.state.numel(), logits.data_ptr(), density.data_ptr(), changed.data_ptr(), used_ptr,
                  lib._stream(keep[0]))
        del keep
        self._frame_hw = (h, w)
        if m._stacks is not None:
            self.stacks = used
        return logits, density, changed

    def snapshot(self) -> EngineStreamSnapshot:
        """A point to come back to (save_accumulator, nnue_engine.cpp:792-797, for the whole stream state: sets included)."""
        return EngineStreamSnapshot(self.model, self.num_streams, self.state.clone(), self.stacks.clone(), self._generation,
                                    self._frame_hw)

    def restore(self, snap: EngineStreamSnapshot) -> None:
        """Takes every stream back to ``snap`` (restore_accumulator, nnue_engine.cpp:799-804) with one device copy and no
        synchronisation.  If the model was requantised since the snapshot, the next ``update`` rebuilds the sums and the next
        ``step`` / ``step_features`` refreshes.  ValueError for a snapshot of another model or stream count."""
        if not isinstance(snap, EngineStreamSnapshot):
            raise TypeError(f"restore: expected an EngineStreamSnapshot, got {type(snap).__name__}")
        if snap.model is not self.model or snap.num_streams != self.num_streams or snap.state.numel() != self.state.numel():
            raise ValueError("restore: the snapshot belongs to another model or stream count")
        self.state.copy_(snap.state)
        self.stacks = snap.stacks.clone()
        self._generation = snap.generation
        self._frame_hw = snap.frame_hw
