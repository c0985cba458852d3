"""Every dispatch arm of the LayerNorm row kernels (ln_residual, downsample_ln, upsample_ln; forward and backward; fp32 and bf16)
against fp64 references, through the public wrappers of ops.py / ops_bf16.py.  Cases, references and the elementwise bounds are
in tests/helpers/row_ref.py; tests/test_row_arms_cpu.py proves on the CPU that the table reaches every arm and that an fp32
evaluation of the references passes these bounds.  Every test prints max(error / bound) per output before it asserts."""
import pytest
import torch

from helpers import row_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENTINEL = -7.5          # exact in bf16


@pytest.fixture(scope="module")
def P():
    import pangu_pytorch_amd as P
    assert torch.cuda.is_available()
    P._lib.load()
    return P


def _ops(P, case):
    from pangu_pytorch_amd import ops, ops_bf16
    return ops if case["dt"] == "f32" else ops_bf16


def _dev(t, case):
    return t.to(torch.float32 if case["dt"] == "f32" else BF).cuda()


def _strided(t, ld, fill, case):
    """`t` on the device as a view of rows `ld` apart (0: dense), the gap columns filled with `fill`; -> (view, buffer)."""
    if not ld:
        t = _dev(t, case)
        return t, t
    buf = torch.full((t.shape[0], ld), fill, dtype=torch.float32 if case["dt"] == "f32" else BF, device="cuda")
    buf[:, :t.shape[1]] = _dev(t, case)
    return buf[:, :t.shape[1]], buf


def _untouched(buf, width):
    gap = buf[:, width:]
    want = torch.full_like(gap, SENTINEL)
    return torch.equal(gap.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8))


def _report(case, ratios):
    print(case["id"], {k: f"{v:.3g}" for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, (case["id"], ratios)


def _forward(P, case, call):
    """call(ops, host inputs) -> out, or (out, stats) where the case asks for the statistics"""
    inp, _, ref = R.reference(case)
    got = call(_ops(P, case), inp)
    stats = None
    if case["stats"]:
        got, stats = got
    assert got.dtype == (torch.float32 if case["dt"] == "f32" else BF) and tuple(got.shape) == tuple(ref["out"].shape)
    assert bool(torch.isfinite(got).all())
    ratios = {"out": R.ratio_data(got, ref["out"], case["dt"])}
    if stats is not None:
        assert tuple(stats.shape) == (ref["out"].shape[0], 2)
        ratios["mean"] = R.ratio_data(stats[:, 0], ref["mean"], "f32")
        ratios["rstd"] = R.ratio_rstd(stats[:, 1], ref["rstd"])
    _report(case, ratios)


def _backward(P, case, call):
    """call(ops, host inputs, host dout) -> (dx, dgamma, dbeta); run once per upstream gradient of the case:
    the full one, and (second-pass cases) the one that is zero outside the rows of the second grid-stride pass."""
    inp, douts, ref = R.reference(case)
    ratios = {}
    for i, (dout, r) in enumerate(zip(douts, ref["bwd"])):
        dx, dg, db = call(_ops(P, case), inp, dout)
        assert dx.dtype == (torch.float32 if case["dt"] == "f32" else BF) and dg.dtype == db.dtype == torch.float32
        assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dg).all()) and bool(torch.isfinite(db).all())
        ratios[f"dx{i}"] = R.ratio_data(dx, r["dx"], case["dt"])
        ratios[f"dgamma{i}"] = R.ratio_param(dg, r["dgamma"], r["tgamma"])
        ratios[f"dbeta{i}"] = R.ratio_param(db, r["dbeta"], r["tbeta"])
        if case["op"] == "up":       # the cropped quarter of dy is exactly zero
            assert float(R.cropped_quarter(case, dx.float().cpu()).abs().sum()) == 0.0
            assert float(R.cropped_quarter(case, r["dx"]).abs().sum()) == 0.0
    _report(case, ratios)


_ids = lambda k: k["id"]


@pytest.mark.parametrize("case", R.cases_for("ln", "fwd"), ids=_ids)
def test_ln_residual(P, case):
    def call(ops, inp):
        C = case["C"]
        y, g, b = _dev(inp["x"], case), inp["gamma"].cuda(), inp["beta"].cuda()
        sc, _ = _strided(inp["shortcut"], case["lds"], float("nan"), case)
        kw = {"want_stats": True} if case["stats"] else {}
        if not case["ldo"]:
            return ops.ln_residual(y, sc, g, b, branch_scale=case["scale"], **kw)
        out, buf = _strided(torch.full_like(inp["x"], SENTINEL), case["ldo"], SENTINEL, case)
        res = ops.ln_residual(y, sc, g, b, out=out, branch_scale=case["scale"], **kw)
        assert (res[0] if case["stats"] else res) is out
        assert _untouched(buf, C), "ln_residual wrote between the rows of a strided out"
        return res
    _forward(P, case, call)


@pytest.mark.parametrize("case", R.cases_for("ln", "bwd"), ids=_ids)
def test_ln_residual_bwd(P, case):
    def call(ops, inp, dout):
        d, _ = _strided(dout, case["lddo"], float("nan"), case)
        return ops.ln_residual_bwd(d, _dev(inp["x"], case), inp["gamma"].cuda(), branch_scale=case["scale"])
    _backward(P, case, call)


@pytest.mark.parametrize("case", R.cases_for("down", "fwd"), ids=_ids)
def test_downsample_ln(P, case):
    def call(ops, inp):
        x, _ = _strided(inp["x"], case["ldx"], float("nan"), case)
        kw = {"want_stats": True} if case["stats"] else {}
        return ops.downsample_ln(x, inp["gamma"].cuda(), inp["beta"].cuda(), case["Z"], case["H"], case["W"], **kw)
    _forward(P, case, call)


@pytest.mark.parametrize("case", R.cases_for("down", "bwd"), ids=_ids)
def test_downsample_ln_bwd(P, case):
    def call(ops, inp, dout):
        x, _ = _strided(inp["x"], case["ldx"], float("nan"), case)
        add = _dev(inp["add"], case) if case["add"] else None
        return ops.downsample_ln_bwd(_dev(dout, case), x, inp["gamma"].cuda(), case["Z"], case["H"], case["W"], add=add)
    _backward(P, case, call)


@pytest.mark.parametrize("case", R.cases_for("up", "fwd"), ids=_ids)
def test_upsample_ln(P, case):
    def call(ops, inp):
        kw = {"want_stats": True} if case["stats"] else {}
        return ops.upsample_ln(_dev(inp["x"], case), inp["gamma"].cuda(), inp["beta"].cuda(), case["Z"], case["H2"], case["W2"],
                               case["H"], **kw)
    _forward(P, case, call)


@pytest.mark.parametrize("case", R.cases_for("up", "bwd"), ids=_ids)
def test_upsample_ln_bwd(P, case):
    def call(ops, inp, dout):
        return ops.upsample_ln_bwd(_dev(dout, case), _dev(inp["x"], case), inp["gamma"].cuda(), case["Z"], case["H2"], case["W2"],
                                   case["H"])
    _backward(P, case, call)
