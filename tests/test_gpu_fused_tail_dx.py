"""The classifier's per-sample tail inside its d_x launch (nnue_classifier_train_step phases 123 = 59 + 64): every output
bitwise that of phases 59's two launches (tail kernel, then the d_x tiles), at the entry point and through the trainer;
shapes outside the fused kernel keep the two launches.  ``-m gpu``."""
import pytest
import torch

import nnue
from nnue_hip import lib as hip
from nnue_hip.trainer import NnueTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRAD_SCALE = 0.5
L2, L3, C = 128, 32, 10


def bits(t):
    return t.contiguous().view(torch.int32)


def entry_case(B, L1, seed):
    """Layer-1 slabs in scratch (as the FeatureTransformer forward leaves them) and the classifier's other operands.
    Labels include -1 (padded rows); b3 puts logits near +1e4 / -1e4 into every row; some rows' slabs are 100x larger."""
    g = torch.Generator().manual_seed(seed)
    S = L1 // 64
    x = torch.rand(B, L1, generator=g)
    w1 = 0.05 * torch.randn(L2, L1, generator=g)
    b1 = 0.1 * torch.randn(L2, generator=g)
    w2 = 0.2 * torch.randn(L3, L2, generator=g)
    b2 = 0.1 * torch.randn(L3, generator=g)
    w3 = 0.3 * torch.randn(C, L3, generator=g)
    b3 = torch.randn(C, generator=g)
    b3[0], b3[1] = 1e4, -1e4
    labels = torch.randint(0, C, (B,), generator=g)
    labels[torch.rand(B, generator=g) < 0.1] = -1
    slabs = 0.3 * torch.randn(S, B, L2, generator=g)
    slabs[:, ::7] *= 100.0
    dev = [t.to(DEV) for t in (x, w1, b1, w2, b2, w3, b3, labels)]
    scratch = torch.full((hip.classifier_train_scratch_bytes(B, L1, L2, L3, C),), 0x7F, dtype=torch.uint8, device=DEV)
    scratch[:S * B * L2 * 4].view(torch.float32).copy_(slabs.reshape(-1).to(DEV))
    return dev, scratch


def run_entry(case, B, L1, clip, phases):
    (x, w1, b1, w2, b2, w3, b3, labels), scratch0 = case
    scratch = scratch0.clone()
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    out = (nan(B, L2), nan(B, L3), nan(B, C))
    loss_out = (nan(B), nan())
    d_x = nan(B, L1)
    grads = [nan(L2, L1), nan(L2), nan(L3, L2), nan(L3), nan(C, L3), nan(C)]
    hip.classifier_train_step(x, True, w1, b1, w2, b2, w3, b3, labels, GRAD_SCALE, clip, scratch=scratch, out=out,
                              loss_out=loss_out, grads=grads, d_x=d_x, phases=phases)
    torch.cuda.synchronize()
    off = hip.classifier_train_dz1_offset(B, L1, L2, L3, C, True)
    r4 = lambda n: (n + 3) // 4 * 4  # noqa: E731
    o_dz2 = off + r4(B * L2) * 4
    o_dl = o_dz2 + r4(B * L3) * 4
    f = lambda o, n: scratch[o:o + 4 * n].view(torch.float32)  # noqa: E731
    named = {"h1": out[0], "h2": out[1], "logits": out[2], "sample_loss": loss_out[0], "d_x": d_x,
             "d_z1": f(off, B * L2), "d_z2": f(o_dz2, B * L3), "d_logits": f(o_dl, B * C)}
    return named, scratch


# C2 with clip off and on; a batch that ends inside a 16-row tile; 8 slabs (one short batch) and 32 slabs (two batches)
CASES = [(512, 1024, 0.0), (512, 1024, 1.0), (200, 1024, 1.0), (40, 512, 0.0), (72, 2048, 1.0)]


@pytest.mark.parametrize("B,L1,clip", CASES)
def test_fused_launch_is_bitwise_the_two_launches(B, L1, clip):
    assert hip.classifier_train_fused_tail_supported(B, L1, L2, L3, C)
    case = entry_case(B, L1, seed=B + L1)
    ref, ref_scratch = run_entry(case, B, L1, clip, 59)
    got, got_scratch = run_entry(case, B, L1, clip, 123)
    for name, r in ref.items():
        assert torch.isfinite(r).all(), f"reference {name} is complete"
        assert torch.equal(bits(got[name]), bits(r)), name
    assert torch.equal(got_scratch, ref_scratch), "scratch beyond the named outputs"
    # the large-logit rows really are in the softmax's saturated regime
    assert ref["logits"].abs().max() > 5e3


def test_fused_launch_is_deterministic():
    case = entry_case(512, 1024, seed=7)
    a, sa = run_entry(case, 512, 1024, 1.0, 123)
    b, sb = run_entry(case, 512, 1024, 1.0, 123)
    for name in a:
        assert torch.equal(bits(a[name]), bits(b[name])), name
    assert torch.equal(sa, sb)


def test_unsupported_shapes_report_unsupported_and_are_refused():
    assert hip.classifier_train_fused_tail_supported(512, 1024, L2, L3, 10)
    assert not hip.classifier_train_fused_tail_supported(512, 1024, L2, L3, 100)           # C > 64
    assert not hip.classifier_train_fused_tail_supported(512, 1024, L2, L3, 10, buckets=2)  # K > 1
    assert not hip.classifier_train_fused_tail_supported(512, 1088, L2, L3, 10)            # L1 % 128 != 0
    assert not hip.classifier_train_fused_tail_supported(512, 1024, L2, L3, 10, pairwise=False)
    B, L1, C100 = 64, 1024, 100
    x, w1 = torch.rand(B, L1, device=DEV), torch.randn(L2, L1, device=DEV)
    small = [torch.randn(s, device=DEV) for s in ((L2,), (L3, L2), (L3,), (C100, L3), (C100,))]
    labels = torch.zeros(B, dtype=torch.int64, device=DEV)
    with pytest.raises(hip.NnueHipError, match="123"):
        hip.classifier_train_step(x, True, w1, *small, labels, 1.0, 0.0, phases=123)


def c2_trainer(fuse, monkeypatch, classes=10, seed=0):
    monkeypatch.setenv("NNUE_CLS_FUSE_TAIL_DX", "1" if fuse else "0")
    torch.manual_seed(seed)
    model = nnue.NNUE(nnue.GridFeatureSet(10, 8), 1024, 128, 32, num_classes=classes).to(DEV)
    return NnueTrainer(model, 512, (32, 32), lr=0.01, momentum=0.9, weight_decay=2e-4, max_grad_norm=1.0, use_graph=True,
                       input_slots=5)


def train(tr, seed=1):
    g = torch.Generator().manual_seed(seed)
    for _ in range(3):
        tr.step(torch.randn(512, 3, 32, 32, generator=g).to(DEV), torch.randint(0, 10, (512,), generator=g).to(DEV))
    for s in range(5):
        tr.inputs[s][0].copy_(torch.randn(512, 3, 32, 32, generator=g))
        tr.inputs[s][1].copy_(torch.randint(0, 10, (512,), generator=g))
    ring = tr.step_many(range(5)).clone()
    torch.cuda.synchronize()
    return ring


def test_trainer_fused_and_two_launches_are_bitwise_equal(monkeypatch):
    on = c2_trainer(True, monkeypatch)
    off = c2_trainer(False, monkeypatch)
    assert on.fuse_tail_dx and not off.fuse_tail_dx
    ring_on, ring_off = train(on), train(off)
    assert torch.isfinite(ring_on).all()
    assert torch.equal(bits(ring_on), bits(ring_off)), "loss ring"
    assert torch.equal(bits(on.flat_params), bits(off.flat_params)), "flat_params"
    assert torch.equal(bits(on.flat_momentum), bits(off.flat_momentum)), "flat_momentum"
    assert torch.equal(bits(on.logits), bits(off.logits)), "logits"


def test_trainer_keeps_two_launches_where_unsupported(monkeypatch):
    tr = c2_trainer(True, monkeypatch, classes=100)
    assert tr.ride_small and not tr.fuse_tail_dx
