"""tests/gather_forms.py against itself and against the C side, without a GPU: CASES reaches every kernel instantiation of the
two gather families, each case launches the cells it names, and the restated plan_gather reproduces nnue_ftb_scratch /
nnue_ftb_list_tiles (launch-free queries whose formulas sit in csrc/ftb_kernels.hip).  CPU only."""
import ctypes
import itertools

import pytest
import torch

import gather_forms as gf
from nnue_hip import lib


def test_cases_reach_every_cell_of_both_families():
    reached = set().union(*(c.reached() for c in gf.CASES))
    want = {("list",) + cell for cell in gf.LIST_CELLS} | {("bits",) + cell for cell in gf.GATHER_CELLS}
    assert want - reached == set(), f"no case launches {sorted(want - reached, key=str)}"
    assert reached - want == set(), f"cells outside the restatement's own lists: {sorted(reached - want, key=str)}"


@pytest.mark.parametrize("case", gf.CASES, ids=lambda c: c.name)
def test_a_case_launches_the_cells_it_names(case):
    assert case.cells and set(case.cells) <= case.reached(), (case.name, sorted(set(case.cells) - case.reached(), key=str))


def test_the_cases_the_plan_asks_for_are_there():
    shapes = {c.shape for c in gf.CASES}
    assert (900, 2, 3, 3, 4, 256) in shapes and (1024, 8, 11, 11, 800, 256) in shapes
    assert {300, 768, 1280} <= {c.l1 for c in gf.CASES if c.kind == "prepare"}
    assert any(c.batch % 64 for c in gf.CASES if c.kind == "prepare")
    assert any(c.positions > 4096 and c.l1 <= 256 and c.l1 % 256 for c in gf.CASES)
    assert max(c.batch * max(c.positions, c.l1) for c in gf.CASES) <= 1024 * 968  # the largest batch-sized tensor: the 1024 x 968 map
    assert max(c.rows * c.l1 for c in gf.CASES) <= 1024 * 968
    # the split with the clamp sink: three ragged splits; the plain split: four even ones
    assert gf.plan_gather(801, 8, 4) == (2, 3, 3) and gf.plan_gather(5, 8, 4) == (2, 4, 2) and gf.plan_gather(33, 8, 8) == (2, 4, 2)


def test_list_forms_at_the_widths_the_kernels_branch_on():
    f = gf.list_forms
    assert f(24, 4096)["values"] == "simple" and f(24, 4097)["values"] == "simple+stride"
    assert f(256, 10) == dict(forward="wide:1w", weight="wide:1w", values="wide<1>")
    assert f(255, 10) == dict(forward="narrow", weight="simple", values="simple")
    assert f(257, 10) == dict(forward="simple", weight="simple", values="simple")
    for s, form in ((3, "wide:3w"), (5, "wide:4w+tail"), (6, "wide:4w+tail"), (7, "wide:4w+tail")):
        assert f(256 * s, 10) == dict(forward=form, weight=form, values="simple")
    assert f(2048, 10) == dict(forward="wide:4w", weight="wide:4w", values="wide<8>")
    assert f(3072, 10) == dict(forward="wide:4w", weight="wide:4w", values="simple")


def _c_queries(b, f, p, l1):
    L = lib.load()
    tf, tb = ctypes.c_int(), ctypes.c_int()
    assert L.nnue_ftb_list_tiles(b, f, p, ctypes.byref(tf), ctypes.byref(tb)) == 0
    return (tf.value, tb.value), int(L.nnue_ftb_scratch(b, f, p, l1))


@pytest.mark.parametrize("case", [c for c in gf.CASES if c.bits], ids=lambda c: c.name)
def test_the_restated_plan_is_the_c_plan_at_every_case(case):
    b, f, p, l1 = case.batch, case.rows, case.positions, case.l1
    tiles, scratch = _c_queries(b, f, p, l1)
    assert gf.list_tiles(b, f, p) == tiles and gf.ftb_scratch(b, f, p, l1) == scratch
    split = max(s * n for (_, _, _, s), n in ((gf.gather_cell(0, b, f, p, l1), b), (gf.gather_cell(1, b, f, p, l1), f + 1)))
    assert (scratch > 16) == bool(split)  # a split cell is exactly a case with slabs


def test_the_restated_plan_is_the_c_plan_on_a_sweep():
    """844 shapes around every threshold of plan_gather: 192 / 200 groups at the three widths, 1 / 2 / 7 / 8 / 9 tiles each
    way, splits capped by nt / 2 and by 16."""
    batches = (1, 5, 128, 129, 384, 385, 768, 769, 896, 897, 1024, 1025, 1537, 2049, 3137, 6145)
    tables = (1, 2, 4, 129, 130, 384, 400, 767, 768, 800, 897, 898, 1025, 3071, 3200, 6200)
    maps = (1, 18, 128, 200, 896, 968, 4096)
    n = 0
    for b, f, p, l1 in itertools.product(batches, tables, maps, (256, 512, 1024)):
        if (b * 7 + f * 3 + p + l1) % 6:  # one shape in six
            continue
        tiles, scratch = _c_queries(b, f, p, l1)
        assert gf.list_tiles(b, f, p) == tiles, (b, f, p, l1)
        assert gf.ftb_scratch(b, f, p, l1) == scratch, (b, f, p, l1)
        n += 1
    assert n >= 300
    assert _c_queries(5, 4, 18, 100)[1] == 0 == gf.ftb_scratch(5, 4, 18, 100)  # a width the column tiles do not divide


def test_exact_operands_have_float32_references():
    """reference() asserts it per case; here the two cases with the longest sums of each product."""
    for name in ("cap4200", "l2048", "b_tiny"):
        case = gf.BY_NAME[name]
        ref = gf.reference(case, True)
        assert ref["out"].dtype == torch.float64 and ref["out"].shape == (case.batch, case.l1)
        bound = gf.term_bound(ref, "d_w")
        assert bound.shape == ref["d_w"].shape and bool((bound[ref["abs"]["d_w"] == 0] == 0).all())
