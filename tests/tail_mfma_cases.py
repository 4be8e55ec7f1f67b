"""Cases, launches and float64 references of tests/test_gpu_tail_mfma.py: the classifier's tile tail (tail_dx_train_kernel: the
four small products of a 16-row tile on the f32 MFMA) at the entry point nnue_classifier_train_step.

A case is the launch's own inputs -- layer-1 slabs [L1 / 64, B, 128] at the start of scratch (what the FeatureTransformer
forward leaves), b1, W2, b2, W3, b3, labels, x, W1 -- float32 on the CPU.  `launch` runs one phase combination and returns
every output by name; `reference` restates the tail in float64 torch, each stage from the kernel's OWN previous stage, with
the element-wise bounds of tests/test_gpu_classifier_train.py (gamma_n * sum|terms| + n * 2^-126, the cross-entropy bars,
torch's select gates): imported, not restated.
"""
import torch
import torch.nn.functional as F

from nnue_hip import lib as hip
from test_gpu_classifier_train import CE_RTOL, TINY, act64, c64, gamma, gate64

DEV = "cuda"
L2, L3 = 128, 32   # the only widths the kernel is built for
G = 0.5            # grad_scale / B of every launch: grad_scale = G * B, so that a row alone (B = 1) sees the same scale
BAND = 64          # floats of NaN on either side of a banded buffer (keeps 16-byte alignment)
NAMES = ("h1", "h2", "logits", "sample_loss", "d_logits", "d_z2", "d_z1", "d_x")


def make_case(B, L1, C, seed, big_logits=True, odd_labels=True):
    """Continuous random operands.  big_logits: b3 puts logits near +1e4 / -1e4 into every row (C >= 2), the regime of
    tests/test_gpu_fused_tail_dx.py; odd_labels: the first row's label is -1 and the last row's is C."""
    g = torch.Generator().manual_seed(seed)
    S = L1 // 64
    c = dict(B=B, L1=L1, C=C)
    c["slabs"] = 0.3 * torch.randn(S, B, L2, generator=g)
    c["x"] = torch.rand(B, L1, generator=g)
    c["w1"] = 0.05 * torch.randn(L2, L1, generator=g)
    c["b1"] = 0.1 * torch.randn(L2, generator=g)
    c["w2"] = 0.2 * torch.randn(L3, L2, generator=g)
    c["b2"] = 0.1 * torch.randn(L3, generator=g)
    c["w3"] = 0.3 * torch.randn(C, L3, generator=g)
    c["b3"] = torch.randn(C, generator=g)
    if big_logits and C >= 2:
        c["b3"][0], c["b3"][1] = 1e4, -1e4
    c["labels"] = torch.randint(0, C, (B,), generator=g)
    if odd_labels:
        c["labels"][0] = -1
        c["labels"][B - 1] = C if B > 1 else -1
    return c


def make_grid_case(B, L1, C, seed):
    """Operands on binary grids so coarse that every product and every partial sum of the four small products is exact in
    float32 in any order (asserted on the reference by `grid_reference`): slabs, b1, W2, b2 multiples of 1/8, W3 in
    {-1, 0, 1}, b3 = -2048 c, so that class 0 wins every row by more than exp's float32 range and the softmax is an exact
    one-hot; d_logits is then exactly +-G or 0."""
    g = torch.Generator().manual_seed(seed)
    S = L1 // 64
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
    c = dict(B=B, L1=L1, C=C)
    c["slabs"] = ri(-2, 2, S, B, L2) / 8
    c["x"] = ri(0, 4, B, L1) / 4
    c["w1"] = ri(-2, 2, L2, L1) / 8
    c["b1"] = ri(-2, 2, L2) / 8
    c["w2"] = ri(-2, 2, L3, L2) / 8
    c["b2"] = ri(-4, 4, L3) / 8
    c["w3"] = ri(-1, 1, C, L3)
    c["b3"] = -2048.0 * torch.arange(C, dtype=torch.float32)
    c["labels"] = torch.randint(0, C, (B,), generator=g)
    return c


def permuted(c, perm):
    out = dict(c)
    out["slabs"] = c["slabs"][:, perm].contiguous()
    out["x"], out["labels"] = c["x"][perm].contiguous(), c["labels"][perm].contiguous()
    return out


def rows_of(c, rows):
    out = permuted(c, torch.as_tensor(rows))
    out["B"] = len(rows)
    return out


def banded(t):
    """A device copy of t inside its own NaN-filled allocation; returns (view, whole allocation)."""
    whole = torch.full((t.numel() + 2 * BAND,), float("nan"), device=DEV)
    view = whole[BAND:BAND + t.numel()].view(t.shape)
    view.copy_(t)
    return view, whole


def bits(t):
    return t.contiguous().view(torch.int32)


def launch(c, clip, phases, band_w3=False):
    """One nnue_classifier_train_step call.  Scratch is NaN everywhere but the slabs, outputs are NaN before the call.
    Returns ({name: tensor}, scratch, w3's whole allocation or None)."""
    B, L1, C = c["B"], c["L1"], c["C"]
    assert hip.classifier_train_fused_tail_supported(B, L1, L2, L3, C), "the fused predicate takes this shape"
    S = L1 // 64
    d = {k: c[k].to(DEV) for k in ("x", "w1", "b1", "w2", "b2", "b3", "labels")}
    w3, w3_whole = banded(c["w3"]) if band_w3 else (c["w3"].to(DEV), None)
    n_bytes = hip.classifier_train_scratch_bytes(B, L1, L2, L3, C)
    scratch = torch.full((n_bytes // 4,), float("nan"), device=DEV).view(torch.uint8)
    scratch[:S * B * L2 * 4].view(torch.float32).copy_(c["slabs"].reshape(-1))
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    out, loss_out, d_x = (nan(B, L2), nan(B, L3), nan(B, C)), (nan(B), nan()), nan(B, L1)
    grads = [nan(L2, L1), nan(L2), nan(L3, L2), nan(L3), nan(C, L3), nan(C)]
    hip.classifier_train_step(d["x"], True, d["w1"], d["b1"], d["w2"], d["b2"], w3, d["b3"], d["labels"], G * B, clip,
                              scratch=scratch, out=out, loss_out=loss_out, grads=grads, d_x=d_x, phases=phases)
    torch.cuda.synchronize()
    off = hip.classifier_train_dz1_offset(B, L1, L2, L3, C, True)
    r4 = lambda n: (n + 3) // 4 * 4  # noqa: E731
    o_dz2 = off + r4(B * L2) * 4
    o_dl = o_dz2 + r4(B * L3) * 4
    f = lambda o, *s: scratch[o:o + 4 * s[0] * s[1]].view(torch.float32).view(*s)  # noqa: E731
    named = {"h1": out[0], "h2": out[1], "logits": out[2], "sample_loss": loss_out[0], "d_logits": f(o_dl, B, C),
             "d_z2": f(o_dz2, B, L3), "d_z1": f(off, B, L2), "d_x": d_x}
    named["_spans"] = [(off, B * L2), (o_dz2, B * L3), (o_dl, B * C)]
    return named, scratch, w3_whole


def scratch_bands_untouched(c, named, scratch):
    """Everything in scratch past the slabs that is not d_z1 / d_z2 / d_logits is still the NaN it was filled with (phases 123
    writes nothing else there)."""
    S = c["L1"] // 64
    keep = torch.ones(scratch.numel() // 4, dtype=torch.bool, device=DEV)
    keep[:S * c["B"] * L2] = False
    for o, n in named["_spans"]:
        keep[o // 4:o // 4 + n] = False
    return bool(torch.isnan(scratch.view(torch.float32)[keep]).all())


def reference(c, got, clip):
    """{name: (float64 reference, element-wise bound)}, each stage from the kernel's own previous one."""
    B, L1, C = c["B"], c["L1"], c["C"]
    s64, b1, w2, b2, w3, b3, w1, x = (c64(c[k]) for k in ("slabs", "b1", "w2", "b2", "w3", "b3", "w1", "x"))
    h1k, h2k, lgk, dlk, dz2k, dz1k = (c64(got[k]) for k in ("h1", "h2", "logits", "d_logits", "d_z2", "d_z1"))
    y = c["labels"]
    ok = (y >= 0) & (y < C)
    ys = torch.where(ok, y, torch.zeros_like(y))
    ref = {}
    n1 = s64.shape[0] + 2
    ref["h1"] = (act64(s64.sum(0) + b1, clip), gamma(n1) * (s64.abs().sum(0) + b1.abs()) + n1 * TINY)
    n2 = L2 + 4
    ref["h2"] = (act64(h1k @ w2.t() + b2, clip), gamma(n2) * (h1k.abs() @ w2.abs().t() + b2.abs()) + n2 * TINY)
    n3 = L3 + 4
    ref["logits"] = (h2k @ w3.t() + b3, gamma(n3) * (h2k.abs() @ w3.abs().t() + b3.abs()) + n3 * TINY)
    # a label outside [0, C): zero loss and zero d_logits, exactly
    okf = ok.double()
    per = F.cross_entropy(lgk, ys, reduction="none") * okf
    ref["sample_loss"] = (per, CE_RTOL * per.abs().clamp(min=1.0) * okf)
    sm, onehot = torch.softmax(lgk, dim=1), F.one_hot(ys, C).double()
    ref["d_logits"] = ((sm - onehot) * G * okf[:, None], (CE_RTOL * (sm + onehot) * G + TINY) * okf[:, None])
    nC = C + 8
    ref["d_z2"] = (gate64(dlk @ w3, h2k, clip), gate64(gamma(nC) * (dlk.abs() @ w3.abs()) + nC * TINY, h2k, clip))
    nL3 = L3 + 4
    ref["d_z1"] = (gate64(dz2k @ w2, h1k, clip), gate64(gamma(nL3) * (dz2k.abs() @ w2.abs()) + nL3 * TINY, h1k, clip))
    nL2 = L2 + 4
    d_l0, a_l0, h = dz1k @ w1, dz1k.abs() @ w1.abs(), L1 // 2
    xa, xb = x[:, :h], x[:, h:]
    ref["d_x"] = (torch.cat([d_l0[:, :h] * xb + d_l0[:, h:], d_l0[:, :h] * xa], dim=1),
                  gamma(nL2) * torch.cat([a_l0[:, :h] * xb.abs() + a_l0[:, h:], a_l0[:, :h] * xa.abs()], dim=1) + nL2 * TINY)
    return ref


def float32_restatement(c, clip):
    """The tail in plain float32 torch on the CPU from the launch's inputs: what a float32 evaluation in another order loses
    against float64 (the figures a GPU ratio is read against)."""
    f = lambda k: c[k].float()  # noqa: E731
    act = lambda z: z.clamp(0, clip) if clip > 0 else torch.relu(z)  # noqa: E731
    h1 = act(f("slabs").sum(0) + f("b1"))
    h2 = act(h1 @ f("w2").t() + f("b2"))
    return {"h1": h1, "h2": h2, "logits": h2 @ f("w3").t() + f("b3")}


def grid_reference(c):
    """The whole tail of a grid case in float64 from the launch's inputs, ReLU, with the exactness it relies on asserted: every
    value is a float32 number, class 0 wins every row by more than 110 (exp(-110) is 0 in float32)."""
    s64, b1, w2, b2, w3, b3 = (c64(c[k]) for k in ("slabs", "b1", "w2", "b2", "w3", "b3"))
    C, y = c["C"], c["labels"]
    h1 = torch.relu(s64.sum(0) + b1)
    h2 = torch.relu(h1 @ w2.t() + b2)
    logits = h2 @ w3.t() + b3
    if C > 1:
        top2 = logits.topk(2, dim=1).values
        assert bool((logits.argmax(1) == 0).all()) and float((top2[:, 0] - top2[:, 1]).min()) > 110.0
    dl = (F.one_hot(torch.zeros_like(y), C).double() - F.one_hot(y, C).double()) * G
    dz2 = gate64(dl @ w3, h2, 0.0)
    dz1 = gate64(dz2 @ w2, h1, 0.0)
    ref = {"h1": h1, "h2": h2, "logits": logits, "d_logits": dl, "d_z2": dz2, "d_z1": dz1}
    for k, v in ref.items():
        assert torch.equal(v.float().double(), v), f"grid reference {k} is not a float32 number"
    # partial sums: the sum of the magnitudes of every dot stays an exact float32 integer multiple of its grid
    for m, grid in ((h1.abs() @ w2.abs().t() + b2.abs(), 64.0), (h2.abs() @ w3.abs().t() + b3.abs(), 64.0),
                    (dl.abs() @ w3.abs(), 1.0 / G), (dz2.abs() @ w2.abs(), 8.0 / G)):
        assert float(m.max()) * grid < 2 ** 24
    return ref
