"""nnue_hip.optim.SGD / Adam on the GPU (nnue_multi_sgd_step / nnue_multi_adam_step): element by element against float64
clip_grad_norm_ + torch.optim.SGD / Adam (foreach=False) fed our own float32 state of the step before, with the bounds that
tests/test_gpu_optim.py's header states (K float32 roundings per term, NORM_RTOL on clipped terms); the reference loop's
goldens with the clip folded into the step; state hand-over to and from torch.optim and NnueTrainer; schedulers;
bitwise reproducibility whatever the gradient pointers; no allocation after the first step.  ``-m gpu``."""
import json
import math

import pytest
import torch
import torch.nn.functional as F

import nnue
from conftest import assert_close_grad, load_npz
from nnue_hip import optim
from test_gpu_optim import K, NORM_RTOL, U, assert_norm, assert_within, f32

pytestmark = pytest.mark.gpu
DEV = "cuda"


def view_at(src: torch.Tensor, off: int) -> torch.Tensor:
    """A contiguous device copy of src that starts `off` floats into its own allocation (off 1-3: not 16-byte aligned)."""
    base = torch.zeros(src.numel() + off, device=DEV)
    out = base[off:].view(src.shape)
    out.copy_(src)
    return out


def make_params(shapes_offsets, gen):
    return [torch.nn.Parameter(view_at(torch.randn(s, generator=gen), off)) for s, off in shapes_offsets]


class Reference:
    """One float64 step of clip_grad_norm_ + torch.optim (foreach=False) over a list, from our float32 state, with bounds."""

    def __init__(self, kind, ps, opt, max_norm, rounded=True):
        self.kind, self.max_norm = kind, max_norm
        self.p_old = [p.detach().cpu().double() for p in ps]
        self.live = [p.grad is not None for p in ps]
        self.P = [torch.nn.Parameter(x.clone()) for x in self.p_old]
        for P, p in zip(self.P, ps):
            P.grad = None if p.grad is None else p.grad.detach().cpu().double()
        grads = [P.grad for P in self.P if P.grad is not None]
        self.norm = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads])))
        self.coef = min(max_norm / (self.norm + 1e-6), 1.0) if max_norm > 0 else 1.0
        if max_norm > 0 and math.isnan(self.norm):
            self.coef = float("nan")
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([P for P in self.P if P.grad is not None], max_norm, foreach=False)
        self.g_abs = [None if P.grad is None else P.grad.abs() for P in self.P]
        groups = []
        for g in opt.param_groups:
            idx = [i for i, p in enumerate(ps) if any(p is q for q in g["params"])]
            # the hyperparameters the kernel gets: float32 (as test_gpu_optim's references take them); rounded=False: the
            # values as given, for torch's own float32 optimizers, which compute with them unrounded
            r32 = f32 if rounded else float
            cfg = {k: (tuple(r32(b) for b in g[k]) if k == "betas" else r32(g[k]))
                   for k in (("lr", "momentum", "weight_decay") if kind == "sgd" else ("lr", "betas", "eps", "weight_decay"))}
            groups.append(dict(params=[self.P[i] for i in idx], **cfg))
            for i in idx:
                self.P[i]._cfg = cfg
        cls = torch.optim.SGD if kind == "sgd" else torch.optim.Adam
        self.opt = cls(groups, foreach=False)
        self.state_old = []
        for P, p in zip(self.P, ps):
            st = {k: (v.detach().cpu().double().clone() if k != "step" else v.clone()) for k, v in opt.state[p].items()} if p in opt.state else {}
            if st:
                self.opt.state[P] = st
            self.state_old.append({k: v.clone() for k, v in st.items()})
        self.opt.step()

    def check(self, what, ps, opt):
        clip_rtol = NORM_RTOL if self.coef < 1.0 else 0.0
        for i, (P, p) in enumerate(zip(self.P, ps)):
            got = p.detach().cpu().double()
            if not self.live[i]:
                assert torch.equal(got, self.p_old[i]), f"{what}: parameter {i} without a gradient moved"
                continue
            cfg, p_old, t_g, old = P._cfg, self.p_old[i], self.g_abs[i], self.state_old[i]
            lr, wd = cfg["lr"], cfg["weight_decay"]
            if self.kind == "sgd":
                mom = cfg["momentum"]
                t_rest = wd * p_old.abs() + (mom * old["momentum_buffer"].abs() if "momentum_buffer" in old else 0.0)
                m_bound = K * U * (t_rest + t_g) + clip_rtol * t_g
                assert_within(got, P.detach(), K * U * p_old.abs() + lr * m_bound, f"{what}: parameter {i}")
                assert_within(got - p_old, P.detach() - p_old, 2 * U * P.detach().abs() + lr * m_bound, f"{what}: update {i}")
                if mom != 0:
                    assert_within(opt.state[p]["momentum_buffer"], self.opt.state[P]["momentum_buffer"], m_bound, f"{what}: momentum {i}")
                else:
                    assert "momentum_buffer" not in opt.state[p]
            else:
                b1, b2 = cfg["betas"]
                st = self.opt.state[P]
                t = float(st["step"])
                m_old = old.get("exp_avg", torch.zeros_like(p_old))
                v_old = old.get("exp_avg_sq", torch.zeros_like(p_old))
                d = wd * p_old.abs() + t_g
                m_bound = K * U * (b1 * m_old.abs() + (1 - b1) * d) + clip_rtol * (1 - b1) * t_g
                v_bound = K * U * (b2 * v_old.abs() + (1 - b2) * d * d) + 2 * clip_rtol * (1 - b2) * d * t_g
                bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
                m_ref, v_ref = st["exp_avg"], st["exp_avg_sq"]
                denom = v_ref.sqrt() / math.sqrt(bc2) + cfg["eps"]
                sqrt_err = torch.where(v_bound > 0, 2 * v_bound / (v_ref.sqrt() + v_bound.sqrt()), torch.zeros_like(v_bound))
                dir_err = (m_bound / bc1 + (m_ref / bc1).abs() * (sqrt_err / math.sqrt(bc2) + K * U * denom) / denom) / denom
                step = (P.detach() - p_old).abs()
                assert_within(got, P.detach(), K * U * (p_old.abs() + step) + lr * dir_err, f"{what}: parameter {i}")
                assert_within(opt.state[p]["exp_avg"], m_ref, m_bound, f"{what}: exp_avg {i}")
                assert_within(opt.state[p]["exp_avg_sq"], v_ref, v_bound, f"{what}: exp_avg_sq {i}")
                assert float(opt.state[p]["step"]) == t


def set_grads(ps, gen, amp, none=()):
    """randn gradients of global norm ~amp (element 0 of the first live one set to amp)."""
    total = sum(p.numel() for i, p in enumerate(ps) if i not in none)
    first = True
    for i, p in enumerate(ps):
        if i in none:
            p.grad = None
            continue
        g = torch.randn(p.shape, generator=gen) * (amp / math.sqrt(total))
        if first:
            g.view(-1)[0] = amp
            first = False
        p.grad = view_at(g, (i * 3 + 1) % 4)  # gradient views at offsets 0-3 as well


def run_chain(kind, shapes, groups_of, steps, seed, **kw):
    gen = torch.Generator().manual_seed(seed)
    ps = make_params(shapes, gen)
    cls = optim.SGD if kind == "sgd" else optim.Adam
    opt = cls(groups_of(ps), **kw)
    for s, (amp, none) in enumerate(steps):
        set_grads(ps, gen, amp, none)
        r = Reference(kind, ps, opt, kw.get("max_grad_norm", 0.0))
        if kw.get("max_grad_norm", 0.0) > 0:
            assert (r.coef < 1.0) == (amp > 1.0), "the step does not reach the clip state it is meant to test"
        opt.step()
        torch.cuda.synchronize()
        if kw.get("max_grad_norm", 0.0) > 0:
            assert_norm(float(opt.grad_norm), r.norm, f"step {s} norm")
        else:
            assert opt.grad_norm is None
        r.check(f"{kind} step {s}", ps, opt)
    return ps, opt


# shapes with odd counts, views at float offsets 1-3, a size past one chunk and one past one unit
SHAPES = [((3, 5), 0), ((7,), 1), ((4096,), 2), ((16385,), 3), ((64, 33), 0), ((1,), 1), ((20001,), 0)]
STEPS = [(50.0, ()), (1e-3, (1,)), (20.0, (4,)), (0.5, ())]  # clip on / off, None gradients at steps 1 and 2


def two_groups(ps):
    return [{"params": ps[::2]}, {"params": ps[1::2], "lr": 0.02, "weight_decay": 1e-2}]


@pytest.mark.parametrize("momentum,wd", [(0.0, 0.0), (0.9, 0.0), (0.9, 2e-4), (0.0, 2e-4)])
@pytest.mark.parametrize("max_norm", (1.0, 0.0))
def test_sgd_against_float64_torch(momentum, wd, max_norm):
    run_chain("sgd", SHAPES, two_groups, STEPS, 1, lr=0.05, momentum=momentum, weight_decay=wd, max_grad_norm=max_norm)


@pytest.mark.parametrize("wd", (0.0, 1e-2))
@pytest.mark.parametrize("max_norm", (1.0, 0.0))
def test_adam_against_float64_torch(wd, max_norm):
    run_chain("adam", SHAPES, two_groups, STEPS * 2, 2, lr=1e-2, weight_decay=wd, max_grad_norm=max_norm)


@pytest.mark.parametrize("kind", ("sgd", "adam"))
def test_more_segments_than_one_table(kind):
    """300 small tensors: six tables, six norm and six apply launches over disjoint partial ranges."""
    shapes = [((1 + (i * 37) % 300,), i % 4) for i in range(300)]
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-3) if kind == "sgd" else dict(lr=1e-2, weight_decay=1e-3)
    run_chain(kind, shapes, lambda ps: ps, [(50.0, ()), (1e-3, (7, 150, 299))], 3, max_grad_norm=1.0, **kw)


def test_big_segment_beside_tiny_ones():
    shapes = [((3,), 1), ((1 << 24,), 0), ((5,), 2)]
    run_chain("sgd", shapes, lambda ps: ps, [(50.0, ()), (0.5, ())], 4, lr=0.05, momentum=0.9, weight_decay=2e-4, max_grad_norm=1.0)


@pytest.mark.parametrize("bad", ("nan", "inf"))
@pytest.mark.parametrize("kind", ("sgd", "adam"))
def test_non_finite_gradient(bad, kind):
    """A NaN norm gives a NaN coefficient, an Inf norm a zero one (the Inf element NaN), as torch's clip does."""
    gen = torch.Generator().manual_seed(5)
    ps = make_params([((100,), 0), ((37,), 1)], gen)
    opt = (optim.SGD(ps, lr=0.05, momentum=0.9, max_grad_norm=1.0) if kind == "sgd"
           else optim.Adam(ps, lr=1e-2, max_grad_norm=1.0))
    set_grads(ps, gen, 0.5)
    ps[1].grad[11] = float(bad)
    r = Reference(kind, ps, opt, 1.0)
    opt.step()
    torch.cuda.synchronize()
    assert_norm(float(opt.grad_norm), r.norm)
    r.check(f"{bad} gradient", ps, opt)


# ------------------------------------------------------------------------------------------------- the reference loop
def build(cfg, state):
    m = nnue.NNUE(nnue.GridFeatureSet(cfg["grid"], cfg["fps"]), cfg["l1"], cfg["l2"], cfg["l3"], num_classes=cfg["classes"],
                  input_size=cfg["input_size"])
    m.load_state_dict(state)
    return m.to(DEV)


@pytest.mark.parametrize("name,kind", [("c1arch", "sgd"), ("tiny96", "sgd"), ("adam_c1arch", "adam")])
def test_reference_loop_reproduces_goldens(name, kind):
    """train.py:359-366 with the optimizer line changed and the clip_grad_norm_ line dropped."""
    z = load_npz(f"step_{name}.npz")
    cfg = json.loads(str(z["cfg"]))
    model = build(cfg, {k[7:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("state0/")})
    if kind == "sgd":
        opt = optim.SGD(model.parameters(), lr=cfg["lr"], momentum=cfg["momentum"], weight_decay=cfg["weight_decay"],
                        max_grad_norm=cfg["max_grad_norm"])
    else:
        opt = optim.Adam(model.parameters(), lr=cfg["lr"], weight_decay=cfg["weight_decay"], max_grad_norm=cfg["max_grad_norm"])
    model.train()
    for s in range(3):
        opt.zero_grad()
        loss = F.cross_entropy(model(torch.from_numpy(z[f"images{s}"]).to(DEV)), torch.from_numpy(z[f"labels{s}"]).to(DEV).long())
        loss.backward()
        opt.step()
        assert model.nnue2score.grad is None
        assert abs(float(loss.detach()) - float(z[f"loss{s}"])) <= 2e-4 * max(1.0, abs(float(z[f"loss{s}"])))
        assert abs(float(opt.grad_norm) - float(z[f"gradnorm{s}"])) <= 2e-4 * float(z[f"gradnorm{s}"])
        for k, v in model.state_dict().items():
            assert_close_grad(v, torch.from_numpy(z[f"state{s + 1}/{k}"]), f"step {s} {k}", rtol=2e-4)
    if kind == "adam":
        assert "step" not in opt.state[model.nnue2score] and float(opt.state[model.input.weight]["step"]) == 3.0


# ------------------------------------------------------------------------------------------------- hand-over of state
@pytest.mark.parametrize("kind", ("sgd", "adam"))
def test_state_hand_over_to_torch(kind):
    """Two steps with ours, state_dict into torch.optim, a third step there == three steps with ours (element bounds)."""
    gen = torch.Generator().manual_seed(8)
    shapes = [((300,), 1), ((64, 5), 0)]
    ps_a = make_params(shapes, gen)
    ps_b = [torch.nn.Parameter(view_at(p.detach().cpu(), off)) for p, (_, off) in zip(ps_a, shapes)]
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-3) if kind == "sgd" else dict(lr=1e-2, weight_decay=1e-3)
    ours_a = (optim.SGD if kind == "sgd" else optim.Adam)(ps_a, **kw)
    ours_b = (optim.SGD if kind == "sgd" else optim.Adam)(ps_b, **kw)
    for s in range(2):
        set_grads(ps_a, torch.Generator().manual_seed(s), 0.7)
        set_grads(ps_b, torch.Generator().manual_seed(s), 0.7)
        ours_a.step()
        ours_b.step()
    assert all(torch.equal(a, b) for a, b in zip(ps_a, ps_b))
    tor = (torch.optim.SGD if kind == "sgd" else torch.optim.Adam)(ps_b, foreach=False, **kw)
    tor.load_state_dict(ours_b.state_dict())
    set_grads(ps_a, torch.Generator().manual_seed(2), 0.7)
    set_grads(ps_b, torch.Generator().manual_seed(2), 0.7)
    r = Reference(kind, ps_a, ours_a, 0.0)
    r_t = Reference(kind, ps_b, tor, 0.0, rounded=False)
    ours_a.step()
    tor.step()
    torch.cuda.synchronize()
    r.check("ours, step 3", ps_a, ours_a)
    r_t.check("torch after the hand-over, step 3", ps_b, tor)
    for k in r.opt.state[r.P[0]]:  # torch continued from our state: its reference state before the step was ours, bit for bit
        assert torch.equal(r.state_old[0][k], r_t.state_old[0][k]), k


@pytest.mark.parametrize("kind", ("sgd", "adam"))
def test_state_from_trainer(kind):
    """NnueTrainer.optimizer_state_dict() after two steps loads into ours; our third step == the trainer's third step."""
    from nnue_hip.trainer import NnueTrainer
    z = load_npz("step_c1arch.npz")
    cfg = json.loads(str(z["cfg"]))
    state0 = {k[7:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("state0/")}
    kw = dict(lr=cfg["lr"], momentum=cfg["momentum"]) if kind == "sgd" else dict(lr=1e-3, optimizer="adam")
    model_t = build(cfg, state0)
    tr = NnueTrainer(model_t, cfg["batch"], (32, 32), weight_decay=cfg["weight_decay"], max_grad_norm=cfg["max_grad_norm"],
                     use_graph=False, **kw)
    data = [(torch.from_numpy(z[f"images{s}"]).to(DEV), torch.from_numpy(z[f"labels{s}"]).to(DEV).long()) for s in range(3)]
    for s in range(2):
        tr.step(*data[s])
    torch.cuda.synchronize()
    model = build(cfg, {k: v.detach().cpu() for k, v in model_t.state_dict().items()})
    opt = (optim.SGD(model.parameters(), lr=cfg["lr"], momentum=cfg["momentum"], weight_decay=cfg["weight_decay"],
                     max_grad_norm=cfg["max_grad_norm"]) if kind == "sgd"
           else optim.Adam(model.parameters(), lr=1e-3, weight_decay=cfg["weight_decay"], max_grad_norm=cfg["max_grad_norm"]))
    opt.load_state_dict(tr.optimizer_state_dict())
    tr.step(*data[2])
    opt.zero_grad()
    F.cross_entropy(model(data[2][0]), data[2][1]).backward()
    opt.step()
    torch.cuda.synchronize()
    assert abs(float(opt.grad_norm) - float(tr.grad_norm)) <= 1e-4 * float(tr.grad_norm)
    for (k, v), (_, w) in zip(model.state_dict().items(), model_t.state_dict().items()):
        assert_close_grad(v, w, f"{kind} {k} after the trainer's state", rtol=2e-4)


def test_step_lr_scheduler_changes_the_applied_rate():
    gen = torch.Generator().manual_seed(9)
    ps_a = make_params([((257,), 1), ((33,), 0)], gen)
    ps_b = [torch.nn.Parameter(p.detach().clone()) for p in ps_a]
    a, b = optim.SGD(ps_a, lr=0.1, momentum=0.0), torch.optim.SGD(ps_b, lr=0.1, momentum=0.0)
    sa, sb = torch.optim.lr_scheduler.StepLR(a, 2, gamma=0.5), torch.optim.lr_scheduler.StepLR(b, 2, gamma=0.5)
    for s in range(6):
        before = [p.detach().clone() for p in ps_a]
        for pa, pb in zip(ps_a, ps_b):
            pa.grad = torch.ones_like(pa)
            pb.grad = torch.ones_like(pb)
        a.step()
        b.step()
        assert a.param_groups[0]["lr"] == b.param_groups[0]["lr"] == 0.1 * 0.5 ** (s // 2)
        for p, q in zip(ps_a, before):  # p - lr * 1 exactly: the rate the scheduler set is the one applied
            assert torch.equal(p.detach(), q - torch.tensor(a.param_groups[0]["lr"], dtype=torch.float32))
        sa.step()
        sb.step()


@pytest.mark.parametrize("kind", ("sgd", "adam"))
def test_bitwise_reproducible_whatever_the_pointers(kind):
    """The same gradients at other addresses (other offsets within 16 bytes): the same bits in norm, parameters and state."""
    results = []
    for shift in (0, 1, 2):
        gen = torch.Generator().manual_seed(10)
        ps = make_params([((40000,), 0), ((16385,), 1), ((7, 9), 2)], gen)
        opt = (optim.SGD(ps, lr=0.05, momentum=0.9, weight_decay=1e-3, max_grad_norm=1.0) if kind == "sgd"
               else optim.Adam(ps, lr=1e-2, weight_decay=1e-3, max_grad_norm=1.0))
        norms = []
        for s in range(3):
            g = torch.Generator().manual_seed(20 + s)
            for i, p in enumerate(ps):
                p.grad = view_at(torch.randn(p.shape, generator=g) * 0.1, (i + shift) % 4)
            opt.step()
            norms.append(opt.grad_norm.clone())
        torch.cuda.synchronize()
        key = "momentum_buffer" if kind == "sgd" else "exp_avg_sq"
        results.append((torch.stack(norms).cpu(), [p.detach().cpu() for p in ps], [opt.state[p][key].cpu() for p in ps]))
    for other in results[1:]:
        assert torch.equal(other[0].view(torch.int32), results[0][0].view(torch.int32))
        for x, y in zip(other[1] + other[2], results[0][1] + results[0][2]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@pytest.mark.parametrize("kind", ("sgd", "adam"))
def test_no_allocation_after_the_first_step(kind):
    gen = torch.Generator().manual_seed(11)
    ps = make_params([((1000,), 0), ((33, 3), 1)], gen)
    opt = (optim.SGD(ps, lr=0.05, momentum=0.9, max_grad_norm=1.0) if kind == "sgd" else optim.Adam(ps, lr=1e-2, max_grad_norm=1.0))
    grads = [torch.randn(p.shape, generator=gen).to(DEV) for p in ps]
    for p, g in zip(ps, grads):
        p.grad = g
    opt.step()
    torch.cuda.synchronize()
    for s in range(4):
        for p in ps:  # fresh gradient tensors every step, as after zero_grad(set_to_none=True)
            p.grad = None
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        before = torch.cuda.memory_allocated()
        opt.step()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before, f"step {s + 2} allocated"
