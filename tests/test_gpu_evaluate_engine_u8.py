"""evaluate.evaluate_engine(source="u8") and run_training's ``compiled_eval_source``: the compiled metrics straight from the
uint8 store of a GpuLoader's dataset are those of the float batches, exactly -- the confusion-derived keys and latent_density
are equal, only ms_per_sample (a time) may differ -- and a source the u8 form cannot read is refused.  ``-m gpu``."""
import numpy as np
import pytest
import torch

import evaluate
import nnue
from nnue_hip import train_loop
from nnue_hip.engine import EngineModel
from nnue_hip.input_pipeline import GpuImageDataset
from test_train_loop import write_config

pytestmark = pytest.mark.gpu

N, BATCH = 300, 128  # a ragged last batch of 44


@pytest.fixture(scope="module")
def data():
    rng = np.random.RandomState(3)
    labels = rng.randint(0, 10, size=N)
    images = np.clip(rng.randint(0, 160, size=(N, 32, 32, 3)) + labels[:, None, None, None] * 9, 0, 255).astype(np.uint8)
    return images, labels


@pytest.mark.parametrize("stacks", [1, 4])
def test_u8_source_gives_the_float_source_metrics(data, stacks):
    images, labels = data
    torch.manual_seed(stacks)
    model = nnue.NNUE(nnue.GridFeatureSet(10, 8), 64, 16, 16, num_classes=10, num_ls_buckets=stacks).cuda()
    engine = EngineModel.from_model(model)
    assert engine.num_stacks == stacks
    loader = GpuImageDataset(images, labels).loader(BATCH)
    assert len(loader) == 3
    base = evaluate.evaluate_engine(engine, loader)
    assert evaluate.evaluate_engine(engine, loader, source="float").keys() == base.keys()
    got = evaluate.evaluate_engine(engine, loader, source="u8")
    assert got.keys() == base.keys()
    for k in base:
        if k == "ms_per_sample":
            assert np.isfinite(got[k]) and got[k] > 0.0
        elif isinstance(base[k], float) and np.isnan(base[k]):
            assert np.isnan(got[k]), k
        else:
            assert got[k] == base[k], (k, got[k], base[k])
    assert 0.0 < base["latent_density"] < 1.0
    shuffled = GpuImageDataset(images, labels).loader(BATCH, shuffle=True, generator=torch.Generator().manual_seed(1))
    again = evaluate.evaluate_engine(engine, shuffled, source="u8")  # another order: the same confusion matrix
    assert again["acc"] == base["acc"] and again["f1"] == base["f1"]


def test_sources_the_u8_form_cannot_read_are_refused(data):
    images, labels = data
    torch.manual_seed(0)
    engine = EngineModel.from_model(nnue.NNUE(nnue.GridFeatureSet(10, 8), 64, 16, 16, num_classes=10).cuda())
    plain = GpuImageDataset(images, labels)
    for bad in (GpuImageDataset(images, labels, augment=True).loader(BATCH), GpuImageDataset(images, labels, augment="medium").loader(BATCH),
                GpuImageDataset(images, labels, out_hw=24).loader(BATCH), [plain.batch(torch.arange(8, device="cuda"))],
                iter(plain.loader(BATCH))):
        with pytest.raises(ValueError, match="u8"):
            evaluate.evaluate_engine(engine, bad, source="u8")
    with pytest.raises(ValueError, match="source"):
        evaluate.evaluate_engine(engine, plain.loader(BATCH), source="uint8")
    assert GpuImageDataset(images, labels, out_hw=32).loader(BATCH).dataset.output_hw == (32, 32)  # a resize to the stored size is none
    evaluate.evaluate_engine(engine, GpuImageDataset(images, labels, out_hw=32).loader(BATCH), source="u8")


def test_run_training_passes_the_source_through(data, tmp_path):
    images, labels = data
    cfg = train_loop.load_config(write_config(tmp_path, opt="sgd", lr=0.02, epochs=2))
    keys = ("compiled/f1", "compiled/accuracy", "compiled/latent_density")
    rows = {}
    for source in (None, "u8"):
        if source is not None:
            cfg.compiled_eval_source = source
        train = GpuImageDataset(images[:200], labels[:200]).loader(16)
        val = GpuImageDataset(images[200:], labels[200:]).loader(16)
        torch.manual_seed(0)
        res = train_loop.run_training(cfg, train, val, log=lambda line: None, compiled_eval=True)
        rows[source] = res.history
    assert len(rows[None]) == len(rows["u8"]) == 2
    for a, b in zip(rows[None], rows["u8"]):
        assert all(a[k] == b[k] for k in keys), (a, b)
        assert b["compiled/ms_per_sample"] > 0.0
    cfg.compiled_eval_source = "bytes"
    with pytest.raises(ValueError, match="source"):
        train_loop.run_training(cfg, GpuImageDataset(images[:32], labels[:32]).loader(16), GpuImageDataset(images[200:], labels[200:]).loader(16),
                                log=lambda line: None, compiled_eval=True)
