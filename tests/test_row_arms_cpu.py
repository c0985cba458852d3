"""CPU side of tests/test_gpu_row_arms.py: the case table of the LayerNorm row kernels is checked without a GPU.
  * an fp32 torch evaluation of the reference expressions (rounded to bf16 for the bf16 cases) sits inside the bounds the GPU test
    applies to the kernels, for every case: a correct implementation passes;
  * the table reaches every dispatch arm of csrc/rowops.hip, rowops_bf16.hip and rowops_bwd.hip (helpers.row_ref.expected_arm
    mirrors their conditions), each kernel's second grid-stride pass included;
  * no case is large."""
import pytest
import torch

from helpers import row_ref as R

BF = torch.bfloat16


def _as_kernel(t, dt):
    """What a correct kernel would store: the fp32 value, rounded to bf16 in a bf16 case."""
    return t.to(BF).float() if dt == "bf16" else t


@pytest.mark.parametrize("case", R.CASES, ids=lambda k: k["id"])
def test_fp32_evaluation_is_inside_the_bounds(case):
    inp, douts, ref = R.reference(case)
    got = R.evaluate(case, inp, torch.float32, douts)
    dt = case["dt"]
    ratios = {"out": R.ratio_data(_as_kernel(got["out"], dt), ref["out"], dt)}
    if case["stats"]:
        ratios["mean"] = R.ratio_data(got["mean"], ref["mean"], "f32")
        ratios["rstd"] = R.ratio_rstd(got["rstd"], ref["rstd"])
    for i, (g, r) in enumerate(zip(got["bwd"], ref["bwd"])):
        ratios[f"dx{i}"] = R.ratio_data(_as_kernel(g["dx"], dt), r["dx"], dt)
        ratios[f"dgamma{i}"] = R.ratio_param(g["dgamma"], r["dgamma"], r["tgamma"])
        ratios[f"dbeta{i}"] = R.ratio_param(g["dbeta"], r["dbeta"], r["tbeta"])
        if case["op"] == "up":
            assert float(R.cropped_quarter(case, r["dx"]).abs().sum()) == 0.0
    print(case["id"], {k: f"{v:.3g}" for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, ratios
    # the families are what they claim: a constant row has rstd = eps^-1/2, a far row is unit-variance values around 30
    if case["fam"] == "mix" and ref["rstd"].numel() >= 5 and case["op"] == "ln":
        assert abs(float(ref["rstd"][1]) - R.EPS ** -0.5) < 1e-6
        assert abs(float(ref["mean"][3])) > 25.0 and float(ref["rstd"][3]) < 100.0     # unit-variance values around 30


def test_every_dispatch_arm_is_reached():
    reached = {}
    for case in R.CASES:
        for arm in R.arms_of(case):
            reached.setdefault(arm, []).append(case["id"])
    for arm in R.ARMS:
        ids = reached.get(arm, [])
        print(f"{arm}: {len(ids)} case(s), C in {sorted({int(i.split('-C')[1].split('-')[0]) for i in ids})}, e.g. {ids[:1]}")
    missing = [a for a in R.ARMS if a not in reached]
    assert not missing, f"no case reaches {missing}"
    unknown = [a for a in reached if a not in R.ARMS and not a.endswith(":pass2")]
    assert not unknown, f"arms outside the list: {unknown}"


def test_second_pass_cases_isolate_the_pass():
    """Every backward kernel has a case whose rows end 4 to 6 rows into the second grid-stride pass, so that a second call with
    `dout` zeroed elsewhere takes dgamma / dbeta from those rows alone."""
    seen = set()
    for case in R.CASES:
        t = R.tail_rows(case)
        if t:
            assert 4 <= t <= 6, (case["id"], t)
            if case["op"] == "up":
                assert case["H"] == 2 * case["H2"], case["id"]     # the last rows of dout are then the second pass's
            seen.add(R.expected_arm(case["op"] + "_bwd", case["dt"], case["C"], R.strides_of(case, "bwd")))
    want = {a[:-6] for a in R.ARMS if a.endswith(":pass2") and "_bwd_" in a}
    assert want <= seen, want - seen


def test_mirror_of_the_dispatch_conditions():
    e = R.expected_arm
    assert e("ln_fwd", "bf16", 192, (192, 192)) == "ln_fwd_bf16_v8_l32"
    assert e("ln_fwd", "bf16", 192, (196, 192)) == "ln_fwd_bf16_nv1"
    assert e("ln_fwd", "bf16", 384, (384, 388)) == "ln_fwd_bf16_nv2"
    assert e("ln_fwd", "bf16", 512, (512, 512)) == "ln_fwd_bf16_v8_l64"
    assert e("ln_fwd", "bf16", 768, (768, 768)) == "ln_fwd_bf16_nv4"
    assert e("ln_bwd", "bf16", 264, (264,)) == "ln_bwd_bf16_v8_l64"
    assert e("ln_bwd", "bf16", 504, (504,)) == "ln_bwd_bf16_v8_l64"
    assert e("ln_bwd", "bf16", 272, (272,)) == e("ln_bwd", "bf16", 512, (512,)) == "ln_bwd_bf16_v16"
    assert e("ln_bwd", "bf16", 384, (388,)) == "ln_bwd_bf16_nv2"
    assert e("ln_bwd", "bf16", 516, (516,)) == "ln_bwd_bf16_nv4"
    assert e("down_fwd", "bf16", 256, (256,)) == "down_fwd_bf16_v16"
    assert e("down_bwd", "bf16", 192, (196,)) == "down_bwd_bf16_nv4"
    assert [e("down_fwd", "f32", C, (C,))[-1] for C in (40, 64, 72, 128, 136)] == list("11224")
    assert e("up_fwd", "bf16", 256) == "up_fwd_bf16_v8" and e("up_bwd", "bf16", 260) == "up_bwd_bf16_nv2"
    assert R.grid_rows("ln_bwd_f32_nv1") == 2048 * 4 and R.grid_rows("ln_fwd_f32_nv4") == 8192 * 4


def test_no_case_is_large():
    for case in R.CASES:
        assert R.case_bytes(case) <= R.MAX_CASE_BYTES, (case["id"], R.case_bytes(case))


def test_a_lost_second_pass_row_is_caught_only_by_the_isolating_call():
    """Why the second-pass cases call the backward twice: one row lost out of 32 773 sits at the edge of the parameter-gradient
    bound of the full call (the bound scales with the number of rows: here 0.02 to 1.1 of it, channel by channel) and thousands
    of times outside the bound of the call whose `dout` is zero outside the second pass."""
    case = next(k for k in R.CASES if k["id"].startswith("ln-bf16-C8-N32773"))
    inp, douts, ref = R.reference(case)
    lost = [d.clone() for d in douts]
    for d in lost:
        d[-1] = 0.0
    got = R.evaluate(case, inp, torch.float32, lost)
    full, tail = (R.ratio_param(g["dbeta"], r["dbeta"], r["tbeta"]) for g, r in zip(got["bwd"], ref["bwd"]))
    assert full < 1.0 < tail, (full, tail)
    err = (got["bwd"][1]["dbeta"].double() - ref["bwd"][1]["dbeta"]).abs().max()
    assert float(err / (R.PARAM_REL * ref["bwd"][1]["tbeta"].max())) > 1000.0
    assert R.ratio_param(got["bwd"][1]["dgamma"], ref["bwd"][1]["dgamma"], ref["bwd"][1]["tgamma"]) > 1.0


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_a_lost_lane_is_caught(dt):
    """The failure the data bounds aim at: statistics that miss one lane's 4 (of 1024) channels move the output by ~1e-3."""
    case = next(k for k in R.CASES if k["id"].startswith(f"ln-{dt}-C1024-N17") and k["fam"] == "uniform")
    inp, _, ref = R.reference(case)
    x = inp["x"]
    mean = x[:, :-4].sum(-1, keepdim=True) / 1024
    rstd = torch.rsqrt(((x[:, :-4] - mean) ** 2).sum(-1, keepdim=True) / 1024 + R.EPS)
    out = inp["shortcut"] + case["scale"] * ((x - mean) * rstd * inp["gamma"] + inp["beta"])
    assert R.ratio_data(_as_kernel(out, dt), ref["out"], dt) > 1.0
