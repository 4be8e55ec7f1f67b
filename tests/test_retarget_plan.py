"""lib.retarget_plan on hand-made (name, fn, args) calls: which arguments it replaces, which it keeps, and that it never
touches its input.  No GPU, no library call."""
import ctypes

from nnue_hip import lib


def _fn(*args):
    raise AssertionError("a plan is not run here")


def _plan():
    rider, other = lib.NnueClsRider(), lib.NnueClsRider()
    p_rider, p_other = ctypes.pointer(rider), ctypes.pointer(other)
    plan = [("nnue_a", _fn, (0x1000, 0x2000, 7, 1.5, None, p_rider)),
            ("nnue_b", _fn, (0x2000, 0x3000, p_other, "text", 0x1000)),
            ("nnue_c", _fn, ())]
    return plan, (rider, other, p_rider, p_other)


def _frozen(plan):
    return [(n, f, tuple(a)) for n, f, a in plan]


def test_integers_in_the_map_are_replaced_and_everything_else_is_kept():
    plan, (rider, other, p_rider, p_other) = _plan()
    before = _frozen(plan)
    out = lib.retarget_plan(plan, {0x1000: 0x9000, 0x3000: 0x3000, 1: 99})
    assert out is not plan and [c[:2] for c in out] == [c[:2] for c in plan]
    assert out[0][2] == (0x9000, 0x2000, 7, 1.5, None, p_rider) and out[0][2][5] is p_rider
    assert out[1][2] == (0x2000, 0x3000, p_other, "text", 0x9000) and out[1][2][2] is p_other
    assert out[2][2] == ()
    assert type(out[0][2][3]) is float  # (1.5 is no key, and a float is never looked up)
    assert plan == before and all(a is b for c, d in zip(plan, before) for a, b in zip(c[2], d[2]))


def test_a_rider_pointer_is_replaced_by_its_target_address():
    plan, (rider, other, p_rider, p_other) = _plan()
    new = lib.NnueClsRider()
    p_new = ctypes.pointer(new)
    out = lib.retarget_plan(plan, {}, {ctypes.addressof(rider): p_new})
    assert out is not plan
    assert out[0][2][5] is p_new and out[0][2][:5] == plan[0][2][:5]
    assert out[1][2][2] is p_other and out[1][2] == plan[1][2]  # another struct's address is no key
    assert plan[0][2][5] is p_rider
    # a second pointer object to the same struct is the same target
    again = [("nnue_a", _fn, (ctypes.pointer(rider), ctypes.POINTER(lib.NnueClsRider)()))]  # (and a NULL pointer passes through)
    out = lib.retarget_plan(again, {0x1: 0x2}, {ctypes.addressof(rider): p_new})
    assert out[0][2][0] is p_new and not out[0][2][1]
    # both maps at once
    out = lib.retarget_plan(plan, {0x2000: 0x8000}, {ctypes.addressof(other): p_new})
    assert out[0][2] == (0x1000, 0x8000, 7, 1.5, None, p_rider) and out[1][2] == (0x8000, 0x3000, p_new, "text", 0x1000)


def test_nothing_to_replace_returns_the_same_list():
    plan, (rider, other, p_rider, p_other) = _plan()
    before = _frozen(plan)
    unused = lib.NnueClsRider()
    for pointers, structs in (({}, None), (None, None), ({}, {}), ({0x7777: 0x1}, None), ({0x1000: 0x1000}, None),
                              ({}, {ctypes.addressof(unused): p_other}), ({0x7777: 0x1}, {ctypes.addressof(unused): p_other})):
        assert lib.retarget_plan(plan, pointers, structs) is plan
    assert plan == before
