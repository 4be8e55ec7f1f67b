"""Every row of tests/dp_modes.py's table on the GPU, on every rank: the live trainer inside a process group takes the mode the
table says, three eager optimizer steps -- clip active, clip inactive, a short last batch that leaves the last rank short or
empty -- follow the float64 oracle of the GLOBAL batch at the project's bars on each rank, the same steps as graph steps and
as one step group are bitwise the eager ones, and the replicas are bitwise each other after every step.  One spawn per group
(two ranks and four ranks over gloo sharing the GPU, one rank over RCCL with the collectives forced on), one test per row;
``-m gpu``.  Each row prints one ``DP_MODE {json}`` line (mode, launches of one eager step on rank 0, worst error over each bar
per rank): profiles/dp_modes.md is that record."""
import json

import pytest
import torch.distributed as dist

from dp_modes import BY_NAME, GROUPS, ROW_NAMES, check_row, oracle_key, run_group

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    """The directory of the run and the oracles the groups share (each computed once)."""
    return tmp_path_factory.mktemp("dp_modes"), {}


def _group_fixture(group):
    @pytest.fixture(scope="module")
    def records(shared):
        if group[1] == "nccl" and not dist.is_nccl_available():
            return None
        return run_group(group, *shared)
    return records


gloo_2, gloo_4, nccl_1 = (_group_fixture(g) for g in ((2, "gloo"), (4, "gloo"), (1, "nccl")))
FIXTURE = {(2, "gloo"): "gloo_2", (4, "gloo"): "gloo_4", (1, "nccl"): "nccl_1"}
assert sorted(FIXTURE) == GROUPS


@pytest.mark.parametrize("name", ROW_NAMES)
def test_every_rank_of_the_row_takes_its_mode_and_follows_the_oracle(name, request, shared):
    row = BY_NAME[name]
    if row.backend == "nccl" and not dist.is_nccl_available():
        pytest.skip("torch.distributed has no NCCL (RCCL) backend in this build")
    run = request.getfixturevalue(FIXTURE[row.group])
    records = run["records"][name]
    missing = [r for r, rec in enumerate(records) if rec is None]
    assert not missing, f"{name}: no record from rank(s) {missing}; the group's spawn: {run['died'] or 'ended normally'}"
    fails, ratios = check_row(row, records, shared[1][oracle_key(row)])
    print("DP_MODE " + json.dumps(dict(row=name, mode=records[0].get("mode"), launches=records[0].get("launches"),
                                       ratios=[{k: round(v, 4) for k, v in r.items()} for r in ratios],
                                       graph_ratios=[rec.get("graph_ratios") for rec in records] if not row.bitwise else None,
                                       seconds=[rec["seconds"] for rec in records], group_seconds=run["seconds"]), sort_keys=True))
    assert not fails, f"{name}: " + "; ".join(fails)
    assert run["died"] is None, f"{name}: its records are whole but the group's spawn died: {run['died']}"
