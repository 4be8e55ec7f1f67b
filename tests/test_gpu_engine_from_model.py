"""The integer engine built from a live model on the device (EngineModel.from_model / requantize, one launch of
nnue_engine_quantize_model), evaluated with one read-back (evaluate.evaluate_engine) and reported per epoch by the driver
(run_training(compiled_eval=True)).  The reference everywhere is the file path: serialize_model into a file, EngineModel.load of
that file.  "Equal" = torch.equal on every tensor, == on every header scalar and on the stack scales.  ``-m gpu``."""
import copy
import math

import numpy as np
import pytest
import torch

import evaluate
import nnue
import serialize
from conftest import GOLDEN, golden_model, load_npz
from nnue_hip import train_loop
from nnue_hip.engine import EngineModel
from test_train_loop import make_loader, write_config

pytestmark = pytest.mark.gpu

UNIT = 8192  # table elements per work unit of the quantise kernel (csrc/quantize_kernels.hip: kQuantUnit)


def build(cfg, state=None, buckets=1):
    m = nnue.NNUE(nnue.GridFeatureSet(cfg["grid"], cfg["fps"]), cfg["l1"], cfg["l2"], cfg["l3"], num_classes=cfg["classes"],
                  input_size=cfg.get("input_size", 32), num_ls_buckets=buckets)
    if state is not None:
        m.load_state_dict(state)
    return m


def bucketed_model(k=8):  # the shape of test_serialize_bytes.bucketed_model
    torch.manual_seed(5)
    return nnue.NNUE(nnue.GridFeatureSet(10, 8), 64, 32, 8, num_classes=10, num_ls_buckets=k)


def c1arch():
    cfg, params, _, _ = golden_model("c1arch")
    return build(cfg, params)


def file_engine(model, tmp_path, bucket=None, name="m.nnue"):
    """The file path on a copy of the model (serialize_model clamps and flips to eval()), on the model's own device."""
    if bucket is None:
        bucket = "auto" if model.num_ls_buckets > 1 else 0
    path = tmp_path / name
    serialize.serialize_model(copy.deepcopy(model), path)
    return EngineModel.load(path, bucket=bucket)


def assert_equal(got, want, threshold=None):
    """threshold: the value the header must carry where it is not ``want``'s (test 1)."""
    assert set(got.tensors) == set(want.tensors)
    for k, t in want.tensors.items():
        assert got.tensors[k].dtype == t.dtype and got.tensors[k].shape == t.shape, k
        assert torch.equal(got.tensors[k], t), (k, int((got.tensors[k] != t).sum()))
    assert set(got.header) == set(want.header)
    for k, v in want.header.items():
        v = threshold if k == "threshold" and threshold is not None else v
        assert got.header[k] == v, (k, got.header[k], v)
    for k in ("conv_scale", "threshold", "quantized_one", "l1_scale", "l2_scale", "out_scale"):
        v = threshold if k == "threshold" and threshold is not None else getattr(want._c, k)
        assert getattr(got._c, k) == v, (k, getattr(got._c, k), v)
    assert got.num_stacks == want.num_stacks
    if want._stacks is not None:
        assert np.array_equal(got._scales, want._scales)


def snapshot(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


# 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("tiny4x4", "grid8", "c1arch", "saturated"))
def test_equals_the_load_of_the_references_own_file(name, nnue_index):
    """Every tensor and every header scalar equal those of the reference's file -- with one scalar apart.  The header's threshold
    is ``visual_threshold.mean()`` in float32, formed on the model's own device (as serialize_model forms it): the reference
    wrote these files from CPU models, and the device's reduction adds the same terms in another order (tiny4x4, eight
    thresholds of 0.1f: 0.10000000149011612 on the device, 0.10000000894069672 in the file).  So the file's value must be
    exactly the same expression on the CPU copy of the model, the engine's exactly the expression on the device model, and
    the two may differ by the rounding of an n-term float32 sum at most: n * 2^-24 * max|threshold|."""
    if name == "saturated":  # clamp-then-quantise and quantise-then-clamp differ here
        state = {k: torch.from_numpy(v) for k, v in load_npz("nnue_saturated_state.npz").items()}
        model = build(nnue_index["nnue_saturated.nnue"]["cfg"], state)
        assert float(model.input.weight.detach().abs().max()) > 1.0
    else:
        cfg, params, _, _ = golden_model(name)
        model = build(cfg, params)
    on_host = float(model.visual_threshold.detach().mean().cpu().item())
    model = model.cuda()
    before = snapshot(model)
    on_device = float(model.visual_threshold.detach().mean().cpu().item())
    want = EngineModel.load(GOLDEN / f"nnue_{name}.nnue")
    assert want.header["threshold"] == on_host
    n, top = model.visual_threshold.numel(), float(model.visual_threshold.detach().abs().max())
    print(name, "threshold: file", on_host, "device", on_device)
    assert abs(on_device - on_host) <= n * 2.0 ** -24 * top
    assert_equal(EngineModel.from_model(model), want, threshold=on_device)
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items()) and model.training


# 2 ------------------------------------------------------------------------------------------------------------------
def test_ties_edges_and_padded_layout(tmp_path):
    model = nnue.NNUE(nnue.GridFeatureSet(4, 3), 10, 3, 5, num_classes=7)  # all odd or ragged: every padded row and half-row exists
    ties = [(k + 0.5) / 64 for k in range(-70, 71)]  # on both sides of zero and beyond +-1
    edges = [1.0, -1.0, 1.0 + 2.0 ** -20, -1.0 - 2.0 ** -20, -0.0, 1e-40, -1e-40]
    a, b, c = model.classifier._linears()
    with torch.no_grad():
        for shift, w in enumerate((model.input.weight, a.weight, b.weight, c.weight)):
            vals = torch.tensor(edges + ties, dtype=torch.float32).roll(-37 * shift)
            w.copy_(vals.repeat(w.numel() // vals.numel() + 1)[:w.numel()].view_as(w))
        conv = torch.tensor([5.0, -5.0, 127.5 / 64, -127.5 / 64, 126.5 / 64] + ties, dtype=torch.float32)  # +-127 is live here only
        model.conv.weight.copy_(conv[:model.conv.weight.numel()].view_as(model.conv.weight))
        bias = torch.tensor([1e6, -1e6] + ties, dtype=torch.float32)
        for shift, t in enumerate((model.input.bias, a.bias, b.bias, c.bias)):
            t.copy_(bias.roll(-5 * shift)[:t.numel()])
    model = model.cuda().train()
    before = snapshot(model)
    got = EngineModel.from_model(model)
    assert_equal(got, file_engine(model, tmp_path))
    assert int(got.tensors["ft_w"].max()) == 64 and int(got.tensors["ft_w"].min()) == -64  # the table is clamped to [-1, 1] first
    assert int(got.tensors["conv_w"].max()) == 127 and int(got.tensors["conv_w"].min()) == -127
    assert int(got.tensors["ft_b"].max()) == 64000000 and int(got.tensors["ft_b"].min()) == -64000000  # biases are not clamped
    after = model.state_dict()
    assert all(v.dtype == torch.float32 and torch.equal(after[k].reshape(-1).view(torch.int32), v.reshape(-1).view(torch.int32))
               for k, v in before.items())  # bitwise: -0.0 and the denormals included
    assert float(model.input.weight.detach().abs().max()) > 1.0 and model.training
    assert all(p.grad is None for p in model.parameters())


# 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", (1, 2, 3))
def test_views_at_any_offset_and_unit_boundaries(shift, tmp_path):
    torch.manual_seed(11)
    model = nnue.NNUE(nnue.GridFeatureSet(8, 5), 66, 4, 8, num_classes=3)
    with torch.no_grad():
        model.input.weight.mul_(8.0)  # beyond +-1 in places
    model = model.cuda()
    count = model.input.weight.numel()
    assert count == 21120 and count >= 2 * UNIT + 1 and count % UNIT != 0  # three units, the last one ragged
    params = list(model.parameters())
    flat = torch.zeros(sum(p.numel() + 8 for p in params) + 8, device="cuda")
    off = 0
    for p in params:  # every parameter a view at element offset = shift mod 4 of one flat buffer
        off += (shift - off) % 4
        view = flat[off:off + p.numel()].view_as(p)
        view.copy_(p.data)
        p.data = view
        off += p.numel()
        assert p.data_ptr() % 16 == 4 * shift
    assert_equal(EngineModel.from_model(model), file_engine(model, tmp_path))


def test_table_with_a_ragged_last_group(tmp_path):
    torch.manual_seed(12)
    model = nnue.NNUE(nnue.GridFeatureSet(5, 3), 6, 3, 5, num_classes=7).cuda()  # 450 table elements: no multiple of 8
    assert model.input.weight.numel() % 8 == 2
    assert_equal(EngineModel.from_model(model), file_engine(model, tmp_path))


# 4 ------------------------------------------------------------------------------------------------------------------
def test_layer_stacks(tmp_path):
    model = bucketed_model().cuda()
    path = tmp_path / "k8.nnue"
    serialize.serialize_model(copy.deepcopy(model), path)
    auto = EngineModel.from_model(model)
    assert auto.num_stacks == 8
    assert_equal(auto, EngineModel.load(path, bucket="auto"))
    assert_equal(EngineModel.from_model(model, bucket="auto"), EngineModel.load(path, bucket="auto"))
    assert_equal(EngineModel.from_model(model, bucket=3), EngineModel.load(path, bucket=3))
    assert_equal(EngineModel.from_model(model, bucket=99), EngineModel.load(path, bucket=99))  # a stack the model lacks = stack 0
    assert not torch.equal(EngineModel.from_model(model, bucket=3).tensors["l1_w"], EngineModel.from_model(model, bucket=0).tensors["l1_w"])


# 5 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("buckets", (1, 8))
def test_requantize_in_place(buckets, tmp_path):
    model = (c1arch() if buckets == 1 else bucketed_model()).cuda()
    engine = EngineModel.from_model(model)
    ptrs = {k: t.data_ptr() for k, t in engine.tensors.items()}
    gen = torch.Generator().manual_seed(4)
    frames = torch.randn(5, 3, 32, 32, generator=gen).cuda()
    stream = engine.stream(5)
    first = stream.step(frames)
    assert torch.equal(first[0], engine.evaluate_logits(frames)[0])
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.randn(p.shape, generator=gen).cuda() * 0.05)
    generation = engine.generation
    engine.requantize(model)
    assert engine.generation == generation + 1
    assert {k: t.data_ptr() for k, t in engine.tensors.items()} == ptrs
    assert_equal(engine, EngineModel.from_model(model))
    l2, l3 = model.l2_size, model.l3_size
    lead = (buckets,) if buckets > 1 else ()
    assert not engine.tensors["l1_w"].view(*lead, l2 + 1, -1)[..., l2, :].any()  # the padding is still zero
    assert not engine.tensors["l1_b"].view(*lead, l2 + 1)[..., l2].any()
    assert not engine.tensors["l2_w"].view(*lead, l3, 2 * l2)[..., l2:].any()
    assert not engine.tensors["conv_b"].any()
    loaded = file_engine(model, tmp_path)
    want = loaded.evaluate_logits(frames)
    got = engine.evaluate_logits(frames)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], first[0])
    # a stream stepped before the requantise holds sums over the old table: its next step must refresh, not update
    moved = frames.clone()
    moved[:, :, :4, :4] += 1.0
    second = stream.step(moved)
    want = loaded.evaluate_logits(moved)
    assert torch.equal(second[0], want[0]) and torch.equal(second[1], want[1])
    other = nnue.NNUE(nnue.GridFeatureSet(10, 8), 32, 32, 8, num_classes=10, num_ls_buckets=buckets).cuda()
    with pytest.raises(ValueError, match="requantize"):
        engine.requantize(other)
    if buckets > 1:
        with pytest.raises(ValueError, match="requantize"):
            engine.requantize(c1arch().cuda())


# 6 ------------------------------------------------------------------------------------------------------------------
def test_non_finite_parameters_are_zeroed_and_counted(tmp_path):
    model = c1arch().cuda()
    places = ((model.input.weight, (3, 5), float("nan")), (model.input.weight, (700, 1), float("inf")), (model.input.bias, (2,), 1e12))
    with torch.no_grad():
        for t, at, v in places:
            t[at] = v
    with pytest.raises(ValueError, match=r"^3 "):
        EngineModel.from_model(model)
    engine = EngineModel.from_model(model, check=False)
    zeroed = copy.deepcopy(model)
    with torch.no_grad():
        zeroed.input.weight[3, 5] = 0.0
        zeroed.input.weight[700, 1] = 0.0
        zeroed.input.bias[2] = 0.0
    assert_equal(engine, file_engine(zeroed, tmp_path))
    l1 = model.l1_size
    assert int(engine.tensors["ft_w"][3 * l1 + 5]) == 0 and int(engine.tensors["ft_w"][700 * l1 + 1]) == 0 and int(engine.tensors["ft_b"][2]) == 0
    with pytest.raises(ValueError, match=r"^3 "):  # the count is this call's, not the sum with the unchecked one before it
        engine.requantize(model)
    engine.requantize(zeroed)


# 7 ------------------------------------------------------------------------------------------------------------------
def small_loader(seed=21):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, 3, 32, 32, generator=gen), torch.randint(0, 10, (n,), generator=gen)) for n in (16, 16, 5)]


@pytest.mark.parametrize("buckets", (1, 8))
def test_evaluate_engine_equals_evaluate_compiled_model(buckets):
    model = (c1arch() if buckets == 1 else bucketed_model()).cuda()
    loader = small_loader()
    want = evaluate.evaluate_compiled_model(copy.deepcopy(model), loader, "nnue")
    engine = EngineModel.from_model(model)
    got = evaluate.evaluate_engine(engine, loader)
    print(got, want)
    assert set(got) == set(want) == {"acc", "f1", "precision", "recall", "ms_per_sample", "latent_density"}
    for k in ("acc", "f1", "precision", "recall"):
        assert got[k] == want[k], k
    # both are float64 sums of 37 terms in [0, 1], in different orders
    assert abs(got["latent_density"] - want["latent_density"]) <= 1e-12 * abs(want["latent_density"])
    assert 0.0 < want["latent_density"] < 1.0
    assert math.isfinite(got["ms_per_sample"]) and got["ms_per_sample"] > 0.0
    with pytest.raises(ValueError, match="empty loader"):
        evaluate.evaluate_engine(engine, [])
    with pytest.raises(ValueError, match="labels lie outside"):
        evaluate.evaluate_engine(engine, [(loader[0][0], loader[0][1] + 5)])


# 8 ------------------------------------------------------------------------------------------------------------------
def test_driver_reports_compiled_metrics_and_leaves_the_run_alone(tmp_path):
    cfg = train_loop.load_config(write_config(tmp_path, opt="sgd", lr=0.02, epochs=2))
    train, val = make_loader(3, 16, 1, last=7), make_loader(2, 16, 2)
    keys = {"compiled/f1", "compiled/accuracy", "compiled/ms_per_sample", "compiled/latent_density"}
    runs = {}
    for on in (True, False):
        torch.manual_seed(0)
        model = train_loop.build_model(cfg, "cuda")
        logs = []
        res = train_loop.run_training(cfg, train, val, model=model, log=logs.append, compiled_eval=on)
        runs[on] = (model, res, logs)
    model, res, logs = runs[True]
    assert len(res.history) == 2 and all(keys <= set(row) for row in res.history)
    assert all("Compiled F1: " in line and "ms/sample, Density: " in line for line in logs)
    final = train_loop.build_model(cfg, "cuda")  # a copy: the trained module carries captured graphs, which deepcopy cannot take
    final.load_state_dict(model.state_dict())
    want = evaluate.evaluate_compiled_model(final, val, "nnue")
    last = res.history[-1]
    print(last, want)
    assert last["compiled/f1"] == want["f1"] and last["compiled/accuracy"] == want["acc"]
    assert abs(last["compiled/latent_density"] - want["latent_density"]) <= 1e-12 * abs(want["latent_density"])
    assert math.isfinite(last["compiled/ms_per_sample"]) and last["compiled/ms_per_sample"] > 0.0
    plain, plain_res, plain_logs = runs[False]
    assert len(plain_res.history) == 2 and not any(keys & set(row) for row in plain_res.history)
    assert not any("Compiled" in line for line in plain_logs)
    for (k, p), (_, q) in zip(model.named_parameters(), plain.named_parameters()):
        assert torch.equal(p, q), k
    # the config attribute turns it on as well
    cfg.compiled_eval = True
    cfg.max_epochs = 1
    torch.manual_seed(0)
    res = train_loop.run_training(cfg, train, val, log=lambda s: None)
    assert keys <= set(res.history[0])
