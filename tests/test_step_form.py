"""step_mode.step_form -- which run form one call of NnueTrainer.step takes -- held to a table written out by hand from the
chain of ``if``s that ``step`` was before the forms had names (DESIGN, "The run forms of a step").  Launch-free: no GPU.

Reachable inputs: capture_collectives implies collectives, one bucket and a trainer with graphs (a call with timers still has
graphs=False); own_exchange implies collectives and one bucket; NNUE_DP_BUCKETS=2 may be set where there are no collectives.
"""
import itertools

import pytest

from nnue_hip import step_mode

L, G, GD, OWN, ONE, TWO = "local", "graph", "graph_dp", "own_exchange", "one_message", "two_buckets"
ALL, AB = ("all",), ("a", "b")
# columns: (graphs, first, ragged) -- only (True, False, False), the steady state with graphs, can replay a whole-step graph
CALLS = ((False, False, False), (False, False, True), (False, True, False), (False, True, True),
         (True, False, False), (True, False, True), (True, True, False), (True, True, True))
# rows: (collectives, buckets, capture_collectives, own_exchange) -> the parts, and the form of each column
TABLE = {
    (False, 1, False, False): (ALL, (L, L, L, L, G, L, L, L)),
    (False, 2, False, False): (ALL, (L, L, L, L, G, L, L, L)),
    (True, 1, False, False): (ALL, (ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE)),
    (True, 1, True, False): (ALL, (ONE, ONE, ONE, ONE, GD, ONE, ONE, ONE)),
    (True, 1, False, True): (ALL, (OWN, OWN, OWN, OWN, OWN, OWN, OWN, OWN)),
    (True, 1, True, True): (ALL, (OWN, OWN, OWN, OWN, GD, OWN, OWN, OWN)),
    (True, 2, False, False): (AB, (TWO, TWO, TWO, TWO, TWO, TWO, TWO, TWO)),
}
# what no trainer reaches follows the same order of questions (the old chain's): a whole-step graph first, then the absence of
# collectives, then the mode's own exchange, then the buckets -- (graphs, first, ragged, collectives, buckets, capture, own)
UNREACHABLE = {
    (True, False, False, False, 1, True, False): (GD, ALL),   # captured collectives without collectives: still asked first
    (True, True, False, False, 1, True, True): (L, ALL),      # ... and on a first step the absence of collectives decides
    (True, False, False, True, 2, True, False): (GD, AB),     # captured collectives with two buckets: the parts are the buckets'
    (False, False, False, True, 2, False, True): (OWN, AB),   # an own exchange with two buckets
    (True, False, True, True, 2, True, True): (OWN, AB),
}


def _ask(graphs, first, ragged, collectives, buckets, capture, own, async_op):
    return step_mode.step_form(graphs=graphs, first=first, ragged=ragged, collectives=collectives, buckets=buckets,
                               capture_collectives=capture, own_exchange=own, async_op=async_op)


def test_the_table_covers_every_reachable_combination():
    reachable = {(c, b, cap, own) for c, b, cap, own in itertools.product((False, True), (1, 2), (False, True), (False, True))
                 if (not cap or (c and b == 1)) and (not own or (c and b == 1))}
    assert reachable == set(TABLE)
    assert set(CALLS) == set(itertools.product((False, True), repeat=3)) and len(CALLS) == 8


@pytest.mark.parametrize("dp", sorted(TABLE))
@pytest.mark.parametrize("async_op", (False, True))
def test_step_form_follows_the_table(dp, async_op):
    parts, names = TABLE[dp]
    for call, name in zip(CALLS, names):
        form = _ask(*call, *dp, async_op)
        # the async flag reaches only the one-message all-reduce
        assert (form.name, form.parts, form.async_op) == (name, parts, async_op and name == ONE), (call, dp)
        assert form.graph == {G: "full", GD: "full_dp"}.get(name)


@pytest.mark.parametrize("case", sorted(UNREACHABLE))
def test_an_unreachable_combination_follows_the_same_order(case):
    name, parts = UNREACHABLE[case]
    form = _ask(*case, False)
    assert (form.name, form.parts) == (name, parts)


def test_the_forms_name_the_graphs_that_hold_an_update():
    assert set(step_mode.FORMS) == {L, G, GD, OWN, ONE, TWO}
    assert sorted(step_mode.UPDATE_GRAPH_KINDS) == ["full", "full_dp", "many"]
    with pytest.raises(Exception):
        _ask(True, False, False, False, 1, False, False, False).name = L  # frozen
