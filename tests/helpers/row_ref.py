"""fp64 references, bounds and the case table of the LayerNorm row kernels (ln_residual, downsample_ln, upsample_ln; forward and
backward; fp32 and bf16).  Plain torch on the CPU: no CUDA, and the project's library is never loaded here.

The references are evaluated from the operands the kernel sees (for a bf16 case the operands are rounded to bf16 first and then
lifted), in the dtype the caller asks for: float64 is the reference, float32 is the "a correct implementation passes" evaluation
of tests/test_row_arms_cpu.py.

Bounds (elementwise; `ratio_*` return max(error / bound), <= 1 passes):
  fp32 data   |got - ref| <= 1e-5 * max|ref|                       an fp32 evaluation sits at ~1.5e-7; summation order and a 1-2 ulp
                                                                   hardware rsq are far below; a lost lane / divisor / row is >= 1e-3
  bf16 data   |got - ref| <= 2^-7 * |ref| + 1e-5 * max|ref|        one output rounding (2^-8) x 2, plus the fp32 floor
  dgamma/dbeta|got - ref| <= 1e-4 * sum_rows |term|  per channel   ~16 rows per lane in registers + <= 2048 atomics: 2100 * 2^-24
  rstd        |got - ref| <= 1e-5 * |ref|                          half the relative error of a C-term fp32 sum of squares
                                                                   (<= (log2 C + 3) * 2^-24 ~ 1e-6) plus one rsq: >= 10x margin
  mean        the fp32 data bound over the mean column

Input families: every case's rows are the suite's usual uniform rows (unit variance, shift 0.3); in a "mix" case row r is exactly
constant when r % 5 == 1 (variance 0, rstd = eps^-1/2) and sits 30 standard deviations from zero when r % 5 == 3.
  * The constants are +-0.25 / 0.125: k * v is exact in fp32 for every k <= 1024, so the row sum is exact in any summation order
    and the mean is off by at most one ulp (mean = sum * fl(1/C) in the fast kernels).  xhat of such a row is (x - mean) * 316:
    a one-ulp mean leaves 0.25 * 2^-24 * 316 = 4.7e-6 in the output, under a quarter of the fp32 floor (max|ref| >= 2).  A
    constant that is not exactly summable would put the summation order itself (a few ulp * 316) at the bound.
  * The first two values of a far row are 29 and 31: the sample variance of a 4-channel row is then at least 0.5.  Without
    them a few of the 6500 far rows of a 4-channel second-pass case have a variance near zero, and rstd (up to 316) multiplies
    the 30 * 2^-24 rounding of their mean past the fp32 floor in ANY fp32 evaluation (the CPU check showed it).
  * A case of one or two rows is built from pairs 0.3 +- (0.25 + |u|), so that no |xhat| is below ~0.1: dgamma[c] of a single row is
    g * xhat[c], and its bound 1e-4 * |g * xhat[c]| drops under the 1e-7 absolute rounding of xhat wherever |xhat[c]| < 1e-3 --
    one channel in a few hundred of a uniform row (the CPU check showed 0.66 of the bound at C = 516).  With more rows
    the per-channel sum of |term| is dominated by the rows where xhat is O(1).
  * The upstream gradient of a constant row is scaled by 2^-8 ~ eps^1/2, so its dy (which carries rstd = 316) is O(1) like every
    other row's and does not inflate max|ref| -- the bound stays sharp for the uniform rows.
"""
import torch
import torch.nn.functional as F

import synth

EPS = 1e-5
FLOOR = 1e-5
BF16_REL = 2.0 ** -7
PARAM_REL = 1e-4
STAT_REL = 1e-5
CONST_GAIN = 2.0 ** -8
CONSTS = (0.25, -0.25, 0.125)
MAX_CASE_BYTES = 64 << 20


# ---- the expressions ---------------------------------------------------------------------------------------------------------
def layer_norm(x, gamma, beta):
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = torch.rsqrt((d * d).mean(-1, keepdim=True) + EPS)
    xhat = d * rstd
    return xhat * gamma + beta, xhat, mean[:, 0], rstd[:, 0]


def downsample_rows(x, Z, H, W):
    """(Z*H*W, C) tokens -> (Z*H2*W2, 4C) rows: pad H to even with a zero row, gather 2x2 (dh, dw, c)."""
    C, H2, W2 = x.shape[1], (H + 1) // 2, W // 2
    xr = F.pad(x.view(Z, H, W, C), (0, 0, 0, 0, 0, 2 * H2 - H)).view(Z, H2, 2, W2, 2, C)
    return xr.permute(0, 1, 3, 2, 4, 5).reshape(-1, 4 * C)


def upsample_rows(y, Z, H2, W2, H):
    """(Z*H2*W2, 4Co) coarse tokens -> (Z*H*2W2, Co) fine rows: scatter (dh, dw, c) into 2x2, crop to H."""
    Co = y.shape[1] // 4
    yr = y.view(Z, H2, W2, 2, 2, Co).permute(0, 1, 3, 2, 4, 5).reshape(Z, 2 * H2, 2 * W2, Co)
    return yr[:, :H].reshape(-1, Co)


def evaluate(case, inp, dtype=torch.float64, douts=()):
    """The case's forward (out, mean, rstd) and, per upstream gradient in `douts`, its backward by autograd
    (dx, dgamma, dbeta and the per-channel sums of |term| that bound the two parameter gradients), all in `dtype`."""
    gamma = inp["gamma"].to(dtype).requires_grad_(True)
    beta = inp["beta"].to(dtype).requires_grad_(True)
    x = inp["x"].to(dtype).requires_grad_(True)
    scale = 1.0
    if case["op"] == "ln":
        scale = case["scale"]
        ln, xhat, mean, rstd = layer_norm(x, gamma, beta)
        out = inp["shortcut"].to(dtype) + scale * ln
    elif case["op"] == "down":
        out, xhat, mean, rstd = layer_norm(downsample_rows(x, case["Z"], case["H"], case["W"]), gamma, beta)
    else:
        out, xhat, mean, rstd = layer_norm(upsample_rows(x, case["Z"], case["H2"], case["W2"], case["H"]), gamma, beta)
    res = {"out": out.detach(), "mean": mean.detach(), "rstd": rstd.detach(), "bwd": []}
    for i, d in enumerate(douts):
        d = d.to(dtype)
        dx, dg, db = torch.autograd.grad(out, (x, gamma, beta), d, retain_graph=i + 1 < len(douts))
        if case.get("add"):
            dx = dx + inp["add"].to(dtype)
        res["bwd"].append({"dx": dx, "dgamma": dg, "dbeta": db,
                           "tgamma": (scale * d * xhat.detach()).abs().sum(0), "tbeta": (scale * d).abs().sum(0)})
    return res


# ---- bounds ------------------------------------------------------------------------------------------------------------------
def _ratio(err, bound):
    r = torch.where(err <= bound, err / bound.clamp_min(1e-300), torch.full_like(err, float("inf")))
    r = torch.where(err == 0, torch.zeros_like(r), r)
    return float(torch.nan_to_num(r, nan=float("inf")).max()) if r.numel() else 0.0


def ratio_data(got, ref, dt):
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    floor = FLOOR * ref.abs().max()
    bound = floor.expand_as(ref) if dt == "f32" else BF16_REL * ref.abs() + floor
    return _ratio((got - ref).abs(), bound)


def ratio_param(got, ref, termsum):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return _ratio((got - ref.double()).abs(), PARAM_REL * termsum.double())


def ratio_rstd(got, ref):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return _ratio((got - ref.double()).abs(), STAT_REL * ref.double().abs())


# ---- dispatch mirror ---------------------------------------------------------------------------------------------------------
def _nv(width):
    return 1 if width <= 256 else 2 if width <= 512 else 4


def expected_arm(op, dtype, C, ld=()):
    """The kernel `op` ("ln_fwd", "ln_bwd", "down_fwd", "down_bwd", "up_fwd", "up_bwd") launches for `dtype` ("f32" / "bf16"),
    channel count C and the row strides `ld` it is given; mirrors csrc/rowops.hip, rowops_bf16.hip and rowops_bwd.hip."""
    width = 4 * C if op.startswith("down") else C
    generic = f"{op}_{dtype}_nv{_nv(width)}"      # rowops.hip:306-308,319-321,332-334; PANGU_NVB rowops_bf16.hip:389-394;
    if dtype == "f32":                            # PANGU_NV_DISPATCH rowops_bwd.hip:671-677
        return generic
    ld8 = all(l % 8 == 0 for l in ld)
    if op == "ln_fwd" and C % 8 == 0 and C <= 512 and ld8:                 # rowops_bf16.hip:403
        return "ln_fwd_bf16_v8_l32" if C <= 256 else "ln_fwd_bf16_v8_l64"  # rowops_bf16.hip:405,409
    if op == "ln_bwd" and C % 8 == 0 and C <= 512 and ld8:                 # rowops_bwd.hip:731
        if C <= 256:                                                       # rowops_bwd.hip:740
            return "ln_bwd_bf16_v8_l32"
        return "ln_bwd_bf16_v16" if C % 16 == 0 else "ln_bwd_bf16_v8_l64"  # rowops_bwd.hip:742,746
    if op.startswith("down") and C % 16 == 0 and C <= 256 and ld8:         # rowops_bf16.hip:427, rowops_bwd.hip:765
        return f"{op}_bf16_v16"
    if op.startswith("up") and C % 8 == 0 and C <= 256:                    # rowops_bf16.hip:444, rowops_bwd.hip:783
        return f"{op}_bf16_v8"
    return generic


def grid_rows(arm):
    """Rows one pass of the grid covers (workgroup cap x rows per workgroup); more rows than this start the second pass."""
    if "_nv" in arm:       # one row per wave, 4 waves: forward cap 8192 (rowops.hip:292, rowops_bf16.hip:382), backward 2048
        return (8192 if "_fwd_" in arm else 2048) * 4                      # (rowops_bwd.hip:666)
    rows = {"ln_fwd_bf16_v8_l32": 16, "ln_fwd_bf16_v8_l64": 8,             # rowops_bf16.hip:87,406,410
            "ln_bwd_bf16_v8_l32": 16, "ln_bwd_bf16_v8_l64": 8,             # rowops_bwd.hip:129,735
            "ln_bwd_bf16_v16": 16,                                         # rowops_bwd.hip:231,743
            "down_fwd_bf16_v16": 8, "down_bwd_bf16_v16": 8,                # rowops_bf16.hip:216,428; rowops_bwd.hip:355,766
            "up_fwd_bf16_v8": 16, "up_bwd_bf16_v8": 16}[arm]               # rowops_bf16.hip:282,445; rowops_bwd.hip:458,784
    return 2048 * rows


def _arm_list():
    arms = []
    for op in ("ln_fwd", "ln_bwd", "down_fwd", "down_bwd", "up_fwd", "up_bwd"):
        arms += [f"{op}_{dt}_nv{nv}" for dt in ("f32", "bf16") for nv in (1, 2, 4)]
    arms += ["ln_fwd_bf16_v8_l32", "ln_fwd_bf16_v8_l64", "ln_bwd_bf16_v8_l32", "ln_bwd_bf16_v8_l64", "ln_bwd_bf16_v16",
             "down_fwd_bf16_v16", "down_bwd_bf16_v16", "up_fwd_bf16_v8", "up_bwd_bf16_v8"]
    # the second grid-stride pass of every kernel (each __global__ template, at its smallest width; the two lane layouts of the
    # ln_residual v8 kernels have different rows per workgroup and are listed apart)
    arms += [f"{op}_{dt}_nv1:pass2" for op in ("ln_fwd", "ln_bwd", "down_fwd", "down_bwd", "up_fwd", "up_bwd")
             for dt in ("f32", "bf16")]
    arms += [a + ":pass2" for a in arms if "_v" in a and ":" not in a]
    return arms


ARMS = _arm_list()


def rows_of(case, direction):
    """Rows the kernel iterates over (the up-sampling backward also visits the cropped fine rows)."""
    if case["op"] == "ln":
        return case["N"]
    if case["op"] == "down":
        return case["Z"] * ((case["H"] + 1) // 2) * (case["W"] // 2)
    return case["Z"] * (case["H"] if direction == "fwd" else 2 * case["H2"]) * 2 * case["W2"]


def strides_of(case, direction):
    C = case["C"]
    if case["op"] == "ln":
        return (case["lds"] or C, case["ldo"] or C) if direction == "fwd" else (case["lddo"] or C,)
    return (case["ldx"] or C,) if case["op"] == "down" else ()


def arms_of(case):
    """Arm names (with ":pass2" where the grid-stride loop comes round again) the case reaches in the directions it runs."""
    out = []
    for d in case["dirs"]:
        arm = expected_arm(f"{case['op']}_{d}", case["dt"], case["C"], strides_of(case, d))
        out.append(arm)
        if rows_of(case, d) > grid_rows(arm):
            out.append(arm + ":pass2")
    return out


def tail_rows(case):
    """Backward rows left to the second grid-stride pass (0: one pass): `dout` restricted to them isolates that pass."""
    if "bwd" not in case["dirs"]:
        return 0
    arm = expected_arm(f"{case['op']}_bwd", case["dt"], case["C"], strides_of(case, "bwd"))
    rows, one = rows_of(case, "bwd"), grid_rows(arm)
    return rows - one if one < rows < 2 * one else 0


# ---- case table --------------------------------------------------------------------------------------------------------------
def _ld8(C):
    return (C // 8 + 2) * 8       # a multiple of 8 larger than C


def _ln(dt, C, N, lds=0, ldo=0, lddo=0, scale=1.0, fam="mix", stats=False, dirs=("fwd", "bwd")):
    cid = f"ln-{dt}-C{C}-N{N}-s{lds}-o{ldo}-d{lddo}-b{scale}-{fam}" + ("-st" if stats else "") + "-" + "".join(d[0] for d in dirs)
    return dict(id=cid, op="ln", dt=dt, C=C, N=N, lds=lds, ldo=ldo, lddo=lddo, scale=scale, fam=fam,
                stats=stats and dt == "f32", dirs=dirs)


def _down(dt, C, Z, H, W, ldx=0, add=False, fam="mix", stats=False, dirs=("fwd", "bwd")):
    cid = f"down-{dt}-C{C}-{Z}x{H}x{W}-x{ldx}-{'add-' if add else ''}{fam}" + ("-st" if stats else "") + "-" + "".join(d[0] for d in dirs)
    return dict(id=cid, op="down", dt=dt, C=C, Z=Z, H=H, W=W, ldx=ldx, add=add, fam=fam, stats=stats and dt == "f32", dirs=dirs)


def _up(dt, Co, Z, H2, W2, H, fam="mix", stats=False, dirs=("fwd", "bwd")):
    cid = f"up-{dt}-C{Co}-{Z}x{H2}x{W2}-H{H}-{fam}" + ("-st" if stats else "") + "-" + "".join(d[0] for d in dirs)
    return dict(id=cid, op="up", dt=dt, C=Co, Z=Z, H2=H2, W2=W2, H=H, fam=fam, stats=stats and dt == "f32", dirs=dirs)


LN_WIDTHS = (4, 8, 40, 192, 256, 260, 264, 272, 384, 504, 512, 516, 768, 1024)
DOWN_WIDTHS = (4, 16, 40, 64, 72, 128, 136, 192, 256)
UP_WIDTHS = (4, 8, 36, 192, 256, 260, 384, 516, 1024)
FWD, BWD = ("fwd",), ("bwd",)


def _cases():
    c = []
    for dt in ("f32", "bf16"):
        # width arms: 17 rows are no multiple of the 2, 4, 8 or 16 rows a wave or workgroup takes and fill more than one workgroup
        for C in LN_WIDTHS:
            c.append(_ln(dt, C, 17, fam="mix", stats=True))
            c.append(_ln(dt, C, 17, scale=1.25, fam="uniform"))
        # stride arms: shortcut / out / dout strided by a multiple of 8, by C + 4 (bf16: forces the generic kernel at a fast
        # width), a strided out= alone, a strided shortcut with the wrapper's own out
        for C in (8, 192, 264, 384, 516):
            c.append(_ln(dt, C, 17, lds=_ld8(C), ldo=_ld8(C), lddo=_ld8(C), scale=1.25))
            c.append(_ln(dt, C, 17, lds=C + 4, lddo=C + 4))
            c.append(_ln(dt, C, 17, ldo=C + 4, scale=1.25, dirs=FWD))
            c.append(_ln(dt, C, 17, ldo=_ld8(C), dirs=FWD))
        # row tails at the smallest width of every kernel
        for C in (4, 8, 264, 272, 516):
            for N in (1, 3, 5):
                c.append(_ln(dt, C, N, scale=1.25 if N == 3 else 1.0, stats=N == 5))
        for C in DOWN_WIDTHS:        # 2 x 5 x 6 tokens: a padded latitude row, 18 output rows
            c.append(_down(dt, C, 2, 5, 6, fam="mix", stats=True, add=True))
            c.append(_down(dt, C, 2, 5, 6, fam="uniform"))
        for C in (16, 40, 192):      # geometry and the token stride
            c.append(_down(dt, C, 2, 4, 6, add=True))                 # even H: no padded row
            c.append(_down(dt, C, 3, 5, 2, stats=True))               # W2 = 1
            c.append(_down(dt, C, 1, 7, 4, add=True))                 # Z = 1
            c.append(_down(dt, C, 2, 5, 6, ldx=_ld8(C), add=True))
            c.append(_down(dt, C, 2, 5, 6, ldx=C + 4))                # bf16: the generic kernel at a fast width
        for C in (4, 16, 72, 136):   # 1, 3, 5 and 17 output rows
            for Z, H, W in ((1, 1, 2), (1, 5, 2), (1, 2, 10), (1, 33, 2)):
                c.append(_down(dt, C, Z, H, W, add=H == 5))
        for Co in UP_WIDTHS:         # 2 x 3 x 2 coarse tokens -> 5 (cropped) or 6 latitudes x 4 longitudes
            c.append(_up(dt, Co, 2, 3, 2, 5, fam="mix", stats=True))
            c.append(_up(dt, Co, 2, 3, 2, 6, fam="uniform"))
        for Co in (8, 36, 192, 260):
            c.append(_up(dt, Co, 2, 3, 1, 5))                         # W2 = 1
            c.append(_up(dt, Co, 1, 3, 2, 6, stats=True))             # Z = 1, not cropped
            c.append(_up(dt, Co, 1, 3, 2, 5))                         # Z = 1, cropped
        # row tails: a fine grid has an even number of rows (2, 6, 10, 34 forward; the backward also visits the cropped ones)
        for Co in (4, 8, 260, 516):
            for H2, H in ((1, 1), (2, 3), (3, 5), (9, 17)):
                c.append(_up(dt, Co, 1, H2, 1, H))
    # the grid-stride second pass: rows = cap x rows per workgroup + 5 at the smallest width that reaches the kernel
    for dt in ("f32", "bf16"):
        c.append(_ln(dt, 4, 8192 * 4 + 5, dirs=FWD, stats=True))
        c.append(_ln(dt, 4, 2048 * 4 + 5, scale=1.25, dirs=BWD))
        c.append(_down(dt, 4, 1, 25, 2 * 2521, dirs=FWD, stats=True))   # 13 x 2521 = 8192 * 4 + 5 rows, padded latitude
        c.append(_down(dt, 4, 1, 13, 2 * 1171, add=True, dirs=BWD))     # 7 x 1171 = 2048 * 4 + 5
        # a fine grid has an even row count (forward) and the backward's a multiple of 4: + 6 and + 4 rows instead of + 5;
        # the backward case is not cropped, so that its second-pass rows are real ones
        c.append(_up(dt, 4, 1, 4, 2341, 7, dirs=FWD, stats=True))       # 7 x 2 x 2341 = 8192 * 4 + 6
        c.append(_up(dt, 4, 1, 3, 683, 6, dirs=BWD))                    # 6 x 2 x 683 = 2048 * 4 + 4
    c.append(_ln("bf16", 8, 2048 * 16 + 5))                           # v8, 32 lanes per row, forward and backward
    c.append(_ln("bf16", 264, 2048 * 8 + 5, scale=1.25))              # v8, 64 lanes per row, forward and backward
    c.append(_ln("bf16", 272, 2048 * 16 + 5, dirs=BWD))                 # v16 backward
    c.append(_down("bf16", 16, 1, 53, 2 * 607, add=True))             # v16: 27 x 607 = 2048 * 8 + 5, padded latitude
    c.append(_up("bf16", 8, 1, 4, 2341, 7, dirs=FWD))                   # v8 forward: 7 x 2 x 2341 = 2048 * 16 + 6
    c.append(_up("bf16", 8, 1, 3, 2731, 6, dirs=BWD))                   # v8 backward: 6 x 2 x 2731 = 2048 * 16 + 4
    ids = [k["id"] for k in c]
    assert len(set(ids)) == len(ids), "duplicate case id"
    return c


CASES = _cases()


def cases_for(op, direction):
    return [k for k in CASES if k["op"] == op and direction in k["dirs"]]


def case_bytes(case):
    """Bytes of every operand the kernels of the case touch (inputs, outputs, parameter gradients, stats)."""
    e, C, fwd, bwd = (4 if case["dt"] == "f32" else 2), case["C"], "fwd" in case["dirs"], "bwd" in case["dirs"]
    if case["op"] == "ln":
        rows, width = case["N"], C
        n = rows * (C + fwd * ((case["lds"] or C) + (case["ldo"] or C)) + bwd * ((case["lddo"] or C) + C))
    elif case["op"] == "down":
        tok, rows, width = case["Z"] * case["H"] * case["W"], rows_of(case, "fwd"), 4 * C
        n = tok * (case["ldx"] or C) + fwd * rows * width + bwd * (rows * width + tok * C * (2 if case["add"] else 1))
    else:
        coarse, rows, width = case["Z"] * case["H2"] * case["W2"], rows_of(case, "fwd"), C
        n = coarse * 4 * C + fwd * rows * C + bwd * (rows * C + coarse * 4 * C)
    return e * n + 4 * 4 * width + (8 * rows if case["stats"] else 0)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def _family(rows, gain, fam, seed):
    """Overlay the constant (r % 5 == 1) and far-from-zero (r % 5 == 3) rows on uniform `rows`; `gain` (n,) is the factor the
    upstream gradient of each row takes."""
    if fam != "mix":
        return
    r = torch.arange(rows.shape[0])
    const, far = r % 5 == 1, r % 5 == 3
    rows[const] = torch.tensor(CONSTS)[(r[const] // 5) % 3][:, None].expand(-1, rows.shape[1])
    rows[far] = synth.uniform((int(far.sum()), rows.shape[1]), seed, 1.0, 30.0)
    rows[far, 0], rows[far, 1] = 29.0, 31.0
    gain[const] = CONST_GAIN


def make_inputs(case):
    """CPU float32 operands of the case (exactly bf16-representable for a bf16 case), dense; `dout` in the kernel's layout."""
    sd = lambda tag: synth.name_seed(case["id"] + tag)
    op, C = case["op"], case["C"]
    rows = rows_of(case, "fwd")
    width = 4 * C if op == "down" else C
    full = rows_of(case, "bwd") if op == "up" else rows        # up-sampling: the uncropped fine grid
    g = synth.uniform((full, width), sd("x"), 1.0, 0.3)
    gain = torch.ones(full)
    _family(g, gain, case["fam"], sd("far"))
    if rows <= 2:                # one or two rows: no xhat near zero (module docstring)
        a = 0.25 + (g[:, 0::2] - 0.3).abs()
        g[:, 0::2], g[:, 1::2] = 0.3 + a, 0.3 - a
    dout = synth.uniform((full, width), sd("dout")) * gain[:, None]
    inp = {"gamma": synth.uniform((width,), sd("gamma"), 0.1, 1.0), "beta": synth.uniform((width,), sd("beta"), 0.1)}
    if op == "ln":
        inp["x"], inp["dout"] = g, dout
        inp["shortcut"] = synth.uniform((rows, C), sd("shortcut"), 1.0, 0.3)
    elif op == "down":           # the inverse of downsample_rows; the padded latitude's quarter of the rows is dropped
        Z, H, W, H2, W2 = case["Z"], case["H"], case["W"], (case["H"] + 1) // 2, case["W"] // 2
        inp["x"] = g.view(Z, H2, W2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(Z, 2 * H2, W, C)[:, :H].reshape(-1, C).contiguous()
        inp["dout"] = dout
        if case["add"]:
            inp["add"] = synth.uniform((Z * H * W, C), sd("add"))
    else:                        # the inverse of upsample_rows before the crop; dout is cropped like the output
        Z, H2, W2, H = case["Z"], case["H2"], case["W2"], case["H"]
        inp["x"] = g.view(Z, H2, 2, W2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, 4 * C).contiguous()
        inp["dout"] = dout.view(Z, 2 * H2, 2 * W2, C)[:, :H].reshape(-1, C).contiguous()
    if case["dt"] == "bf16":
        for k in ("x", "dout", "shortcut", "add"):
            if k in inp:
                inp[k] = inp[k].to(torch.bfloat16).float()
    return inp


def tail_dout(case, dout):
    """`dout` zeroed everywhere except the rows of the second grid-stride pass (the last `tail_rows`)."""
    d = torch.zeros_like(dout)
    t = tail_rows(case)
    d[-t:] = dout[-t:]
    return d


def douts_of(case, inp):
    return [inp["dout"]] + ([tail_dout(case, inp["dout"])] if tail_rows(case) else [])


_kept = {}


def reference(case):
    """(inputs, upstream gradients, fp64 results) of the case: computed once and shared, unchanged, by the tests that need it
    (the forward and the backward test of a case); the few large cases are recomputed instead of kept."""
    hit = _kept.get(case["id"])
    if hit is None:
        inp = make_inputs(case)
        douts = douts_of(case, inp) if "bwd" in case["dirs"] else []
        hit = (inp, douts, evaluate(case, inp, torch.float64, douts))
        if case_bytes(case) <= 1 << 20:
            _kept[case["id"]] = hit
    return hit


def cropped_quarter(case, dy):
    """The part of the up-sampling dy (coarse layout) that belongs to cropped fine rows h >= H (empty when H = 2 H2)."""
    Z, H2, W2, H, Co = case["Z"], case["H2"], case["W2"], case["H"], case["C"]
    fine = dy.view(Z, H2, W2, 2, 2, Co).permute(0, 1, 3, 2, 4, 5).reshape(Z, 2 * H2, 2 * W2, Co)
    return fine[:, H:]
