"""The gather-family FeatureTransformer kernels (csrc/ft_kernels.hip: id lists; csrc/ftb_kernels.hip: bit masks + LDS tiles):
which kernel instantiation a shape launches, restated launch-free in Python, the smallest shapes that together launch every
one of them, and their operands with float64 references.  Nothing here touches the GPU.

List family -- ``list_forms(l1, cap)`` restates the choices of nnue_ft_forward / nnue_ft_backward_weight / nnue_ft_backward_values
(S = L1 / 256 where L1 % 256 == 0):

  forward   wide:{1,2,3}w  S < 4: one block of S waves                    narrow  L1 <= 256 and L1 % 256 != 0
            wide:4w        S % 4 == 0: full blocks only                   simple  L1 > 256 and L1 % 256 != 0
            wide:4w+tail   S > 4, S % 4 != 0: the last blockIdx.y has waves that return at once
  weight    the same wide forms, simple for every other width
  values    wide<S>        S in {1, 2, 4, 8}
            simple         every other width (768 .. 1792 columns per dot product at S in {3, 5, 6, 7}), after a zero fill
            simple+stride  ... with cap > 4096: the grid stops at 64 blocks per sample and each block strides over the list

Bits family -- ``plan_gather(n_out, nt, col_tiles)`` restates the C function of the same name; ``gather_cell`` turns its plan into
the instantiation (MODE, sw, NBUF, split) of ftb_gather_kernel (split: tiles over grid.z, slabs finished by ftb_finish_kernel<MODE>).
MODE 0 = forward (n_out = B, nt = ceil(min(F - 1, P) / 128)), MODE 1 = weight gradient (n_out = F + 1, nt = ceil(B / 128)).  A split
plan always has sw = 2 and at least two tiles per split (NBUF = 3); an unsplit one has NBUF = 1 exactly when nt <= 1.

Instantiation                    case            why the case has that shape
-------------------------------  --------------  ------------------------------------------------------------------------------
ft_forward_simple                l300            L1 = 300: two column blocks, the second 44 wide; B = 70 is no multiple of 64
ft_backward_weight_simple        l300            (the same)
ft_backward_values_simple        l300, l768,     300 / 768 / 1280 columns per dot product: a ragged last 64-lane stride at 300
                                 l1280
ft_forward_wide, 3 waves         l768            S = 3: the three-wave block; B = 37
ft_backward_weight_wide, 3 w     l768            (the same)
ft_forward_wide, 4 w + tail      l1280           S = 5: second blockIdx.y runs one wave, three return; B = 130 = 2 * 64 + 2 samples
ft_backward_weight_wide, tail    l1280           (the same; three 64-sample ballots, the last with two live lanes)
ft_forward_narrow                cap4200         L1 = 24 (Lp = 32, 32 list slices)
ft_backward_values_simple+stride cap4200         2 x 4200-position map: ceil(cap / 64) = 66 > 64 blocks, so blocks stride
ft_forward_wide 1 / 2 / 4 waves  b_tiny, m0_split, m1_sw4_one   L1 = 256 / 512 / 1024 (the bits cases run the list kernels too)
ft_backward_values_wide<1,2,4>   b_tiny, m0_split, m1_sw4_one   (the same)
ft_*_wide at S = 8, values<8>    l2048           L1 = 2048: two full blockIdx.y
ftb_gather<1, 0, 1>              b_tiny, m1_split          B = 5 / 900, one table tile
ftb_gather<1, 0, 3>              m1_split_sink   B = 1024, 7 table tiles (nt < 8: no split), 128 groups < 200
ftb_gather<2, 0, 1>              m0_sw2_one      B = 385 at L1 = 1024: ceil(385 / 32) * 16 = 208 >= 200 > ceil(385 / 64) * 16; F = 4: one tile
ftb_gather<2, 0, 3>              m_sw2_ring      B = 385, direct = 200 rows: two tiles
ftb_gather<4, 0, 1>              m0_sw4_one      B = 769 at L1 = 1024: ceil(769 / 64) * 16 = 208 >= 200; F = 4: one tile
ftb_gather<4, 0, 3>              m0_sw4_ring     B = 769, direct = 149 rows: two tiles
ftb_gather<2, 0, 3> split        m0_split        direct = 899 rows: 8 tiles, 16 groups < 192 -> 4 splits of 2; clamp sink in ftb_finish<0>
ftb_gather<1, 1, 1>              b_tiny, m0_split          B <= 128: one batch tile, few table rows
ftb_gather<1, 1, 3>              m0_sw2_one, m0_sw4_one, m0_sw4_ring   B = 385 / 769: 4 / 7 batch tiles, F + 1 <= 151 outputs
ftb_gather<2, 1, 1>              m1_sw2_one      F + 1 = 401 at L1 = 1024: ceil(401 / 32) * 16 = 208 >= 200 > 112; B = 70
ftb_gather<2, 1, 3>              m_sw2_ring      F + 1 = 401, B = 385: 4 batch tiles
ftb_gather<4, 1, 1>              m1_sw4_one      F + 1 = 801 at L1 = 1024: ceil(801 / 64) * 16 = 208; B = 70
ftb_gather<4, 1, 3>              m1_sw4_ring     F + 1 = 801, B = 130: two batch tiles
ftb_gather<2, 1, 3> split        m1_split        B = 900: nt = 8, F + 1 = 5 outputs: 4 groups < 192 -> 4 splits of 2; ftb_finish<1>
                                 m1_split_sink   B = 1024, F = 800 < P = 968: 104 groups -> 3 splits of 3, 3, 2; the valued sink row 799
                                                 crosses the slabs; L1 = 256

Operands come in two kinds.  ``randn``: as tests/test_gpu_ftb.py draws them.  ``exact``: weight = k / 2^8 (|k| <= 2^8), bias and
d_out = k / 8 (|k| <= 8), list coefficients in {+-1, +-1/2, 2} (1 for a binary map).  Every partial sum a kernel can form, in
any order, is then a multiple of 2^-11 below 2^13 in magnitude (forward: <= 4200 terms of at most 2 each, multiples of 2^-9;
weight gradient: <= 1024 terms of at most 170 each, multiples of 2^-4; value gradient: <= 2048 terms of at most 1 each, multiples
of 2^-11), hence a float32 number: results are compared with the float64 reference for equality.  ``reference`` asserts that each
float64 reference of the exact kind is a float32 number.
"""
from dataclasses import dataclass

import torch

import nnue_oracle as orc

KWAVES, KRT, KTC = 16, 128, 64  # waves per gather workgroup, staged rows per LDS tile, columns per workgroup (ftb_kernels.hip)


# ------------------------------------------------------------------ list family
def _wide_form(l1):
    s = l1 // 256
    if s < 4:
        return f"wide:{s}w"
    return "wide:4w" if s % 4 == 0 else "wide:4w+tail"


def list_forms(l1, cap):
    """{entry point: kernel form} of the list family at width l1 and list capacity cap."""
    wide = l1 % 256 == 0
    s = l1 // 256 if wide else 0
    if s in (1, 2, 4, 8):
        values = f"wide<{s}>"
    else:
        values = "simple+stride" if (cap + 63) // 64 > 64 else "simple"
    return dict(forward=_wide_form(l1) if wide else ("narrow" if l1 <= 256 else "simple"),
                weight=_wide_form(l1) if wide else "simple", values=values)


_WIDE = {"wide:1w", "wide:2w", "wide:3w", "wide:4w", "wide:4w+tail"}
LIST_CELLS = ({("forward", f) for f in _WIDE | {"narrow", "simple"}} | {("weight", f) for f in _WIDE | {"simple"}}
              | {("values", f) for f in ("wide<1>", "wide<2>", "wide<4>", "wide<8>", "simple", "simple+stride")})


# ------------------------------------------------------------------ bits family
def list_tiles(b, f, p):
    """nnue_ftb_list_tiles: (table tiles of the forward lists, batch tiles of the backward lists)."""
    d = min(f - 1, p)
    return ((d + KRT - 1) // KRT if d > 0 else 1), (b + KRT - 1) // KRT


def plan_gather(n_out, nt, col_tiles):
    """(sw, splits, tiles_per_split) as plan_gather of csrc/ftb_kernels.hip computes them."""
    def groups(sw):
        return (n_out + KWAVES * sw - 1) // (KWAVES * sw) * col_tiles
    if groups(2) < 192 and nt >= 8:
        want = min((256 + groups(2) - 1) // groups(2), nt // 2, 16)
        tps = (nt + want - 1) // want
        return 2, (nt + tps - 1) // tps, tps
    sw = 4
    while sw > 1 and groups(sw) < 200:
        sw >>= 1
    return sw, 1, (nt if nt > 0 else 1)


def gather_cell(mode, b, f, p, l1):
    """(MODE, sw, NBUF, split) of the ftb_gather_kernel a (B, F, P, L1) launches for the forward (0) / the weight gradient (1)."""
    ntf, ntb = list_tiles(b, f, p)
    sw, splits, tps = plan_gather(b if mode == 0 else f + 1, ntf if mode == 0 else ntb, l1 // KTC)
    return mode, sw, 3 if tps > 1 else 1, splits > 1


def ftb_scratch(b, f, p, l1):
    """nnue_ftb_scratch: bytes of split-slab workspace."""
    if b <= 0 or f <= 0 or p <= 0 or l1 <= 0 or l1 % KTC:
        return 0
    ntf, ntb = list_tiles(b, f, p)
    a, w = plan_gather(b, ntf, l1 // KTC), plan_gather(f + 1, ntb, l1 // KTC)
    fa = a[1] * b * l1 if a[1] > 1 else 0
    fb = w[1] * (f + 1) * l1 if w[1] > 1 else 0
    return (max(fa, fb) + 4) * 4


GATHER_CELLS = ({(m, sw, nbuf, False) for m in (0, 1) for sw in (1, 2, 4) for nbuf in (1, 3)} | {(0, 2, 3, True), (1, 2, 3, True)})


# ------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Case:
    name: str
    kind: str      # "prepare": id / value lists through nnue_ft_prepare (B, M, F, L1); "map": a binary map (B, fps, Gh, Gw, F, L1)
    shape: tuple
    cells: tuple   # the cells the case exists for
    why: str

    @property
    def batch(self):
        return self.shape[0]

    @property
    def rows(self):
        return self.shape[-2]

    @property
    def l1(self):
        return self.shape[-1]

    @property
    def positions(self):
        """List capacity: M of a prepared list, P = fps * Gh * Gw of a map."""
        return self.shape[1] if self.kind == "prepare" else self.shape[1] * self.shape[2] * self.shape[3]

    @property
    def bits(self):
        """Whether the bits family takes the case (a binary map at a width it supports)."""
        return self.kind == "map" and self.l1 in (256, 512, 1024)

    def reached(self):
        """Every cell the case launches: (family, ...) tuples."""
        out = {("list", ep, form) for ep, form in list_forms(self.l1, self.positions).items()}
        if self.bits:
            out |= {("bits",) + gather_cell(m, self.batch, self.rows, self.positions, self.l1) for m in (0, 1)}
        return out


def _l(ep, form):
    return ("list", ep, form)


def _b(mode, sw, nbuf, split=False):
    return ("bits", mode, sw, nbuf, split)


CASES = (
    Case("l300", "prepare", (70, 40, 50, 300), (_l("forward", "simple"), _l("weight", "simple"), _l("values", "simple")),
         "L1 > 256, no multiple of 256: the one-column-per-thread kernels; batch 70 is no multiple of 64"),
    Case("l768", "prepare", (37, 40, 50, 768), (_l("forward", "wide:3w"), _l("weight", "wide:3w"), _l("values", "simple")),
         "S = 3: the three-wave block; the value gradient falls to the simple kernel at 768 columns"),
    Case("l1280", "prepare", (130, 40, 50, 1280), (_l("forward", "wide:4w+tail"), _l("weight", "wide:4w+tail"), _l("values", "simple")),
         "S = 5: a second blockIdx.y with three waves that return; batch 130 = three ballots, the last of two samples"),
    Case("l2048", "prepare", (5, 20, 30, 2048), (_l("forward", "wide:4w"), _l("weight", "wide:4w"), _l("values", "wide<8>")),
         "S = 8: two full blockIdx.y, the widest value-gradient instantiation"),
    Case("cap4200", "map", (2, 8, 21, 25, 4100, 24), (_l("forward", "narrow"), _l("values", "simple+stride")),
         "cap = 4200 > 4096: the value gradient's grid stops at 64 blocks and strides; 100 positions fold into row F - 1"),
    Case("b_tiny", "map", (5, 2, 3, 3, 4, 256), (_b(0, 1, 1), _b(1, 1, 1), _l("forward", "wide:1w"), _l("values", "wide<1>")),
         "one tile each way, a handful of outputs; 15 of 18 positions fold into the sink"),
    Case("m1_split", "map", (900, 2, 3, 3, 4, 256), (_b(1, 2, 3, True),),
         "B >= 897: eight batch tiles split 4 x 2 over grid.z, finished by ftb_finish_kernel<1>"),
    Case("m1_split_sink", "map", (1024, 8, 11, 11, 800, 256), (_b(1, 2, 3, True), _b(0, 1, 3)),
         "CIFAR map at batch 1024, L1 256: 3 splits of 3, 3, 2 tiles with the valued clamp-sink row 799"),
    Case("m0_split", "map", (33, 8, 11, 11, 900, 512), (_b(0, 2, 3, True), _l("forward", "wide:2w"), _l("values", "wide<2>")),
         "direct = 899 rows: eight table tiles split 4 x 2, the sink added by ftb_finish_kernel<0>; L1 512"),
    Case("m0_sw2_one", "map", (385, 2, 3, 3, 4, 1024), (_b(0, 2, 1), _b(1, 1, 3)),
         "385 samples x 16 column tiles: 208 groups at sw 2, 112 at sw 4; one table tile"),
    Case("m_sw2_ring", "map", (385, 8, 5, 5, 400, 1024), (_b(0, 2, 3), _b(1, 2, 3)),
         "sw 2 with the three-slot ring in both modes: two table tiles, four batch tiles, 401 outputs"),
    Case("m1_sw2_one", "map", (70, 8, 5, 5, 400, 1024), (_b(1, 2, 1),),
         "401 outputs at sw 2 over one batch tile"),
    Case("m0_sw4_one", "map", (769, 2, 3, 3, 4, 1024), (_b(0, 4, 1), _b(1, 1, 3)),
         "769 samples x 16 column tiles: 208 groups at sw 4; one table tile"),
    Case("m0_sw4_ring", "map", (769, 8, 5, 5, 150, 1024), (_b(0, 4, 3),),
         "sw 4 over two table tiles (direct = 149)"),
    Case("m1_sw4_one", "map", (70, 8, 11, 11, 800, 1024), (_b(1, 4, 1), _l("forward", "wide:4w"), _l("values", "wide<4>")),
         "801 outputs at sw 4 over one batch tile"),
    Case("m1_sw4_ring", "map", (130, 8, 11, 11, 800, 1024), (_b(1, 4, 3),),
         "801 outputs at sw 4 over two batch tiles, the second of two samples"),
)
BY_NAME = {c.name: c for c in CASES}


# ------------------------------------------------------------------ operands and references
_INPUTS, _REFS = {}, {}


def inputs(case, exact):
    """CPU float32 operands of a case, drawn once: weight, bias, d_out and (prepare) idx, val / (map) conv_out, thr."""
    key = (case.name, exact)
    if key in _INPUTS:
        return _INPUTS[key]
    gen = torch.Generator().manual_seed(sum(case.shape) + 10007 * exact)
    b, f, l1, m = case.batch, case.rows, case.l1, case.positions
    if exact:
        weight = torch.randint(-256, 257, (f, l1), generator=gen).float() / 256
        bias = torch.randint(-8, 9, (l1,), generator=gen).float() / 8
        d_out = torch.randint(-8, 9, (b, l1), generator=gen).float() / 8
    else:
        weight, bias, d_out = torch.randn(f, l1, generator=gen) * 0.1, torch.randn(l1, generator=gen) * 0.1, torch.randn(b, l1, generator=gen)
    c = dict(weight=weight, bias=bias, d_out=d_out)
    if case.kind == "prepare":
        # ids: per sample a random subset of [0, F + 1) without repeats -- F - 1 and F both land on row F - 1, so a row
        # collects at most two entries of a sample and nnue_ft_prepare's coefficient atomics stay order-free; about a
        # quarter of the slots are padding (-1), scattered; one sample is empty and one is full
        perm = torch.stack([torch.randperm(f + 1, generator=gen)[:m] for _ in range(b)])
        hole = torch.rand(b, m, generator=gen) < 0.25
        hole[0], hole[b - 1] = True, False
        c["idx"] = torch.where(hole, torch.full_like(perm, -1), perm)
        if exact:
            c["val"] = torch.tensor([1.0, -1.0, 0.5, -0.5, 2.0])[torch.randint(0, 5, (b, m), generator=gen)]
        else:
            c["val"] = torch.randn(b, m, generator=gen)
    else:
        _, fps, gh, gw, _, _ = case.shape
        if exact:
            on = torch.rand(b, fps, gh, gw, generator=gen) < 0.4
            c["conv_out"], c["thr"] = on.float() * 2 - 1, torch.zeros(fps)
        else:
            c["conv_out"], c["thr"] = torch.randn(b, fps, gh, gw, generator=gen), torch.randn(fps, generator=gen) * 0.3
    _INPUTS[key] = c
    return c


def reference(case, exact):
    """float64 results of the three products through oracle/nnue_oracle.py, and for each element the sum of the magnitudes of
    its terms and their number (the derived float32 bound is n * 2^-23 * sum |terms|).  Computed once, never modified.

    out [B, L1], d_w [F, L1], d_b [L1], d_val [B, M] (prepare: by list slot) or [B, P] (map: by position)."""
    key = (case.name, exact)
    if key in _REFS:
        return _REFS[key]
    c = inputs(case, exact)
    w, bias, d_out = c["weight"].double(), c["bias"].double(), c["d_out"].double()
    b, f = case.batch, case.rows
    if case.kind == "prepare":
        idx, val = c["idx"], c["val"].double()
    else:
        idx, _ = orc.active_lists(c["conv_out"], c["thr"])
        val = (idx >= 0).double()
    keep = idx >= 0
    n_act = keep.sum(1)
    r = dict(out=orc.ft_forward(w, bias, idx, val))
    r["d_w"], r["d_b"], d_val = orc.ft_backward(w, idx, val, d_out)
    c_abs = orc.coefficient_matrix(idx, val.abs(), f)
    g_abs = d_out.abs() @ w.abs().t()
    val_abs = torch.where(keep, torch.gather(g_abs, 1, idx.clamp(0, f - 1)), torch.zeros_like(val))
    if case.kind == "map":  # list slot -> position
        rows = keep.nonzero(as_tuple=True)[0]
        by_pos, by_pos_abs = torch.zeros(b, case.positions, dtype=torch.float64), torch.zeros(b, case.positions, dtype=torch.float64)
        by_pos[rows, idx[keep]] = d_val[keep]
        by_pos_abs[rows, idx[keep]] = val_abs[keep]
        d_val, val_abs = by_pos, by_pos_abs
    r["d_val"] = d_val
    r["abs"] = dict(out=bias.abs() + c_abs @ w.abs(), d_w=c_abs.t() @ d_out.abs(), d_b=d_out.abs().sum(0), d_val=val_abs)
    r["terms"] = dict(out=(n_act + 1).double().unsqueeze(1), d_w=(c_abs != 0).sum(0).double().unsqueeze(1), d_b=float(b), d_val=float(case.l1))
    r["n"] = n_act
    if exact:
        for k in ("out", "d_w", "d_b", "d_val"):
            assert torch.equal(r[k].float().double(), r[k]), f"{case.name}: the float64 {k} is no float32 number"
    _REFS[key] = r
    return r


def term_bound(ref, what):
    """n * 2^-23 * sum |terms| per element of ref[what]."""
    return ref["terms"][what] * 2.0 ** -23 * ref["abs"][what]
