"""tests/golden/engine_edges.npz (outputs RECORDED from the real C++ engine on models whose scales, quantized_one, thresholds,
table and biases leave what serialize.py writes; tests/golden/make_golden_engine_edges.py) on the CPU:

1. the numpy oracle reproduces every record -- logits and density bit-equal as uint32, ids equal;
2. a census, from the oracle's intermediates, of how often the recorded evaluations take each branch of the engine's
   arithmetic that the other engine fixtures never take.  The counts are conditions on the fixture's inputs, not measurements
   of any code under test: if one falls short after the fixture is regenerated, change the inputs, not the bound.

No GPU, and neither the reference nor its binaries take part."""
import numpy as np
import pytest

import engine_edges_record
import nnue_engine_oracle as eo

MIN_COUNT = 5


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    paths, cases = engine_edges_record.load(tmp_path_factory.mktemp("edges"))
    return {name: eo.load_nnue(path) for name, path in paths.items()}, cases


def test_fixture_holds_what_the_generator_promises(record):
    models, cases = record
    assert len(models) == 16 and len(cases) == 2 * 16 + 4
    assert sorted((c.model, c.layout, c.h, c.w) for c in cases if c.layout) == [
        ("conv2_7_thr5", "chw", 32, 32), ("conv2_7_thr5", "hwc", 32, 20), ("odd_scales", "chw", 32, 20), ("odd_scales", "hwc", 32, 32)]
    for c in cases:
        m = models[c.model]
        assert (m["grid"], m["oc"], m["l1"], m["l2"], m["l3"]) == (4, 8, 48, 6, 5) and c.logits.shape[2] == 3
        assert c.stacks == ([0, 1, 2, 3] if c.model == "k3" else [0])
        assert (c.h, c.w, c.count) in ((32, 32, 6), (32, 20, 2)) or c.layout
        assert fractional(m["conv_scale"]) == (c.model == "odd_scales" or c.model.startswith("conv"))
    k3 = models["k3"]
    assert k3["buckets"] == 3
    triples = [(s["l1_scale"], s["l2_scale"], s["out_scale"]) for s in k3["stacks"]]
    assert len({t[j] for t in triples for j in range(3)}) == 7  # three triples, nothing shared but the 64s of the last
    assert not np.array_equal(k3["stacks"][0]["l1_w"], k3["stacks"][1]["l1_w"])
    # the GPU engine refuses conv_scale < 1 and l2_scale < 1 (engine_check_model): the fixture stays where it answers
    assert all(m["conv_scale"] >= 1 and s["l2_scale"] >= 1 for m in models.values() for s in m["stacks"])


def test_oracle_reproduces_every_record(record):
    models, cases = record
    for c in cases:
        m = models[c.model]
        for i in range(c.count):
            conv, _ = eo.conv_forward(m, c.images[i], c.h, c.w)
            assert np.array_equal(eo.active_features(m, conv), c.ids[i]), (c, i)
            for j, k in enumerate(c.stacks):
                logits, density = eo.evaluate_logits(m, c.images[i], c.h, c.w, bucket=k)
                assert logits.dtype == np.float32 and np.array_equal(logits.view(np.uint32), c.logits[i, j]), (c, i, k)
                assert np.float32(density).view(np.uint32) == c.density[i], (c, i)
    # the k3 record names two stacks by the free rule min(K-1, n*K // (F+1)) and index 3 gave stack 0's logits
    k3 = [c for c in cases if c.model == "k3"]
    assert {min(2, a.size * 3 // 129) for c in k3 for a in c.ids} == {1, 2}
    assert all(np.array_equal(c.logits[:, 3], c.logits[:, 0]) and not np.array_equal(c.logits[:, 1], c.logits[:, 0]) for c in k3)


def fractional(x) -> bool:
    return float(x) != int(x)


def test_census_of_the_edges_the_record_reaches(record):
    models, cases = record
    n = dict.fromkeys(("wrapped sum", "a*b/128 > 127", "a > 127", "byte == threshold", "byte == 5 at threshold 5",
                       "byte == -127 at threshold -127, inactive", "byte == 127 at threshold 126.5, active",
                       "layer-1 quotient > 127", "layer-1 quotient in (-1, 0)", "layer-2 quotient < -127",
                       "layer-2 quotient > 127", "negative layer-2 sum with a remainder", "|acc1| > 2^24", "|acc3| > 2^24",
                       "(float)acc1 rounds", "(float)acc3 rounds", "rounded acc1 changes the layer-1 quotient",
                       "conv: int(scale) and scale divide differently", "layer 2: int(scale) and scale divide differently",
                       "features a conv division by the float scale would switch", "evaluations it would change",
                       "u8 evaluations it would change", "evaluations an input times int(scale) would change",
                       "evaluations an exact layer-1 quotient would change", "evaluations x * (1 / l1_scale) would change"), 0)
    for c in cases:
        m = models[c.model]
        thr, cs = np.float32(m["threshold"]), np.float32(m["conv_scale"])
        for i in range(c.count):
            acc, _ = eo.conv_accumulate(m, c.images[i], c.h, c.w)
            conv, _ = eo.conv_forward(m, c.images[i], c.h, c.w)
            byte = conv.reshape(-1).astype(np.int64)  # the produced bytes; flat index = feature id
            on = np.isin(np.arange(byte.size), c.ids[i])
            n["byte == threshold"] += int((byte.astype(np.float32) == thr).sum())
            if thr == 5:
                n["byte == 5 at threshold 5"] += int((~on[byte == 5]).sum())
            if thr == -127:
                n["byte == -127 at threshold -127, inactive"] += int((~on[byte == -127]).sum())
            if thr == np.float32(126.5):
                n["byte == 127 at threshold 126.5, active"] += int(on[byte == 127].sum())
            if fractional(cs):
                n["conv: int(scale) and scale divide differently"] += int(
                    (eo._trunc_div(acc, int(cs)) != np.trunc(acc / np.float64(cs))).sum())
                # what reaches the outputs: the id sets under the conv quotient a kernel dividing by the scale as it stands
                # (float32, as it would) gives, and under an input quantised with the truncated scale
                by_float = np.clip(np.trunc(acc.astype(np.float32) / cs), -127, 127).astype(np.int8)
                switched = np.setxor1d(eo.active_features(m, by_float), c.ids[i]).size
                n["features a conv division by the float scale would switch"] += switched
                n["evaluations it would change"] += int(switched > 0)
                n["u8 evaluations it would change"] += int(switched > 0 and c.layout is not None)
                coarse, _ = eo.conv_forward(dict(m, conv_scale=float(int(cs))), c.images[i], c.h, c.w)
                n["evaluations an input times int(scale) would change"] += int(
                    np.setxor1d(eo.active_features(m, coarse), c.ids[i]).size > 0)
            total = eo.ft_accumulate(m, c.ids[i])
            n["wrapped sum"] += int(((total < -32768) | (total > 32767)).sum())
            ft = eo.ft_forward(m, c.ids[i])
            for k in c.stacks:
                s = m["stacks"][k if k < m["buckets"] else 0]
                t = eo.stack_trace(s, ft, m["l1"], m["l2"], m["l3"])
                l1s, l2s = np.float32(s["l1_scale"]), np.float32(s["l2_scale"])
                n["a*b/128 > 127"] += int((t["prod"] > 127).sum())
                n["a > 127"] += int((t["a"] > 127).sum())
                n["layer-1 quotient > 127"] += int((t["quot1"] > 127).sum())
                exact1 = t["acc1"].astype(np.float32) / l1s
                n["layer-1 quotient in (-1, 0)"] += int(((exact1 > -1) & (exact1 < 0)).sum())
                # the float32 conversion and division against the same quotient in exact arithmetic (big_biases has one output
                # built for it; a float32 quotient next to an integer crosses it now and then as well)
                n["rounded acc1 changes the layer-1 quotient"] += int((t["quot1"] != np.trunc(t["acc1"] / np.float64(l1s))).sum())
                if np.abs(t["acc1"]).max() > 2 ** 24:  # where the float conversion rounds: do other roundings reach a logit?
                    exact = eo.stack_trace(s, ft, m["l1"], m["l2"], m["l3"], lambda u: np.trunc(u["acc1"] / np.float64(l1s)))
                    n["evaluations an exact layer-1 quotient would change"] += int(
                        not np.array_equal(exact["logits"].view(np.uint32), t["logits"].view(np.uint32)))
                    recip = eo.stack_trace(s, ft, m["l1"], m["l2"], m["l3"],
                                           lambda u: np.trunc(u["acc1"].astype(np.float32) * (np.float32(1) / l1s)))
                    n["evaluations x * (1 / l1_scale) would change"] += int(
                        not np.array_equal(recip["logits"].view(np.uint32), t["logits"].view(np.uint32)))
                n["layer-2 quotient < -127"] += int((t["quot2"] < -127).sum())
                n["layer-2 quotient > 127"] += int((t["quot2"] > 127).sum())
                n["negative layer-2 sum with a remainder"] += int(((t["acc2"] < 0) & (np.abs(t["acc2"]) % int(l2s) != 0)).sum())
                for key in ("acc1", "acc3"):
                    n[f"|{key}| > 2^24"] += int((np.abs(t[key]) > 2 ** 24).sum())
                    n[f"(float){key} rounds"] += int((t[key].astype(np.float32).astype(np.int64) != t[key]).sum())
                if fractional(l2s):
                    n["layer 2: int(scale) and scale divide differently"] += int(
                        (t["quot2"] != np.trunc(t["acc2"] / np.float64(l2s))).sum())
    print(n)
    short = {key: count for key, count in n.items() if count < MIN_COUNT}
    assert not short, short
