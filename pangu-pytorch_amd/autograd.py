"""torch.autograd.Function wrappers: one per reference layer, each a hand-scheduled chain of HIP kernels.

Per-sample 2-D token tensors (N, C).  Nothing of size (..,144,144) is saved: attention backward recomputes
the probabilities from q, k, v and the per-row log-sum-exp, so a whole training step keeps ~64 GB of fp32
activations and needs no block re-computation (the reference re-runs every block forward in backward,
models/layers.py:115-119).

Gradient of a projection y = a @ W^T + b:   da = dy @ W  (the forward GEMM with W^T),  dW, db = wgrad(dy, a).

The layer Functions of the whole-model training step serve both precisions.  Their `sh` input is None for fp32, or the model's
fused_bf16.WeightShadow for bf16 mixed precision (BASELINE configs[2]): fp32 master parameters and parameter gradients, bf16
weight shadows / activations / activation gradients (32 GB saved instead of 64 GB), fp32 LayerNorm + softmax + accumulation.
"""
import torch

from . import ops
from . import ops_bf16 as ob


def _wt(w):
    """(out,in[,1]) weight -> contiguous (in,out): the `W` operand of ops.linear for the input gradient."""
    return w.reshape(w.shape[0], -1).t().contiguous()


class _F32:
    """fp32: the kernels of `ops`, reading the parameters themselves."""
    k, dtype = ops, torch.float32
    f32_out = {}                                            # ops.linear writes fp32 as it is
    w = staticmethod(lambda p: p)                           # forward GEMM operand
    wt = staticmethod(_wt)                                  # input-gradient GEMM operand
    table = staticmethod(lambda p: p[0] if p.dim() == 5 else p)      # attention's bias table / QKV bias


class _BF16:
    """bf16: the kernels of `ops_bf16`, reading the bf16 images that the WeightShadow `sh` keeps of the fp32 parameters."""
    k, dtype = ob, torch.bfloat16
    f32_out = {"out_dtype": torch.float32}                  # for the GEMMs whose result leaves the bf16 domain

    def __init__(self, sh):
        self.w, self.wt, self.table = sh.get, sh.get_t, sh.get


def _precision(sh):
    """What separates the two precisions of a layer Function outside its explicit branches: kernel module `k` (linear_wgrad and
    lora_wgrad included), operand accessors `w` / `wt` / `table`, activation `dtype`, `f32_out`."""
    return _F32 if sh is None else _BF16(sh)


def _adapters(ctx, ab, n):
    """The `ad` argument of _wgrad for each of a Function's n projections, in the order of its `lora` scalings (None where not
    adapted, and for all n when the Function ran without adapters).  ab: the saved (A, B) pairs, the Function's trailing inputs."""
    if ctx.lora is None:
        return (None,) * n
    p = len(ctx.needs_input_grad) - len(ab)
    return tuple(None if s is None else (s, ab[2 * i], ab[2 * i + 1], p + 2 * i) for i, s in enumerate(ctx.lora))


def _dropout_fwd(pr, lora, ab, i, x, y, act=ops.ACT_NONE, h=None):
    """After the forward launch y = x W_eff^T (+ b) of a Function's projection i (its place in `lora`): the adapter-dropout
    correction y += s ((c * x) A^T) B^T in place, when that projection's `lora` entry is (scaling, p, seed) -- layers.lora_args,
    dropout active; nothing otherwise.  act=ACT_GELU: h = gelu(y) is produced as well -> whether it ran."""
    e = lora[i] if lora is not None else None
    if type(e) is not tuple:
        return False
    pr.k.lora_dropout_fwd(x, y, ab[2 * i], ab[2 * i + 1], *e, act=act, h=h)
    return True


def _dropout_dx(ctx, ad, dx, pre=None):
    """After the input-gradient GEMM of the same projection: dx += c * (V A) in place on that GEMM's result `dx` (never the
    incoming gradient), V kept by _wgrad.  pre: see ops.lora_dropout_dx (the projection behind a GELU) -> dx."""
    if ad is not None and type(ad[0]) is tuple:
        ctx.pr.k.lora_dropout_dx(dx, ctx.lora_V.pop(ad[3]), ad[1], ad[0][1], ad[0][2], pre=pre)
    return dx


def _wgrad(ctx, dy, x, w, b=None, ad=None, db_into=None, shape=None):
    """Parameter gradients of one projection y = x @ W_eff^T (+ b), W_eff = W (+ s B A when adapted).  w / b: input positions of
    the base weight and bias (b None: no bias); ad: None or (s, A, B, input position of A), from _adapters.  linear_wgrad (of ctx.pr:
    _precision) runs only if W or b asks for a gradient, its lora_wgrad only if A or B does.  With active adapter dropout (s is
    (scaling, p, seed)) the dropout variant runs instead, always: its third result V = s dy B stays on ctx for _dropout_dx
    -> (dW (in `shape` if given), db, dA, dB), None where not computed.  Both run at the same point of the backward, so an adapter
    keeps no activation gradient alive for longer."""
    need = ctx.needs_input_grad
    dw = db = da = dbb = None
    if need[w] or (b is not None and need[b]):
        dw, db = ctx.pr.k.linear_wgrad(dy, x, want_bias=b is not None, db_into=db_into)
        if shape is not None:
            dw = dw.reshape(shape)
    if ad is not None and type(ad[0]) is tuple:
        da, dbb, V = ctx.pr.k.lora_wgrad_dropout(dy, x, ad[1], ad[2], *ad[0])
        if getattr(ctx, "lora_V", None) is None:
            ctx.lora_V = {}
        ctx.lora_V[ad[3]] = V
    elif ad is not None and (need[ad[3]] or need[ad[3] + 1]):
        da, dbb = ctx.pr.k.lora_wgrad(dy, x, ad[1], ad[2], ad[0])
    return dw, db, da, dbb


def _keep_needed(ctx, grads):
    """One gradient per input (inputs past the end of `grads` get None).  Gradients of inputs that do not ask for one (the frozen
    base parameters of a LoRA run -- e.g. the LayerNorm-affine and bias-table gradients that the backward kernels write on every
    call) are discarded instead of returned."""
    need = ctx.needs_input_grad
    return tuple(g if n else None for g, n in zip(tuple(grads) + (None,) * len(need), need))


class EarthBlockFn(torch.autograd.Function):
    """reference models/layers.py:183-253 (+ attention :360-421, Mlp :264-270) for one sample."""

    # the inputs in order; A / B of the adapted projections follow `lora` (the order of its scalings)
    _INPUTS = ("x", "n1w", "n1b", "n2w", "n2b", "m1w", "m1b", "m2w", "m2b", "esb", "a1w", "a1b", "a2w", "a2b", "geom", "s1", "s2",
               "dst", "sh", "lora", "m1A", "m1B", "m2A", "m2B", "a1A", "a1B", "a2A", "a2B")

    @staticmethod
    def forward(ctx, x, n1w, n1b, n2w, n2b, m1w, m1b, m2w, m2b, esb, a1w, a1b, a2w, a2b, geom, s1, s2, dst=None, sh=None, lora=None,
                *ab):
        # dst: optional 1-tuple holding the (N, C) row-strided tensor the block writes its result into (one half of the
        # skip-concat buffer of reference pangu_model.py:81); wrapped so that autograd does not see a tensor argument.
        # lora: scalings of (linear.linear1, linear.linear2, attention.linear1, attention.linear2), None where not adapted, or None
        # without adapters (layers.lora_args); m1w / m2w / a1w / a2w are then the W_eff tensors and ab = (A, B) per linear.  Where
        # an entry is (scaling, p, seed) the projection's adapter dropout is active: _dropout_fwd follows its launch
        out = dst[0] if dst else None
        Z, H, W, heads, shifted = geom
        ctx.pr = pr = _precision(sh)
        K = pr.k
        ctx.geom, ctx.s1, ctx.s2, ctx.lora = geom, s1, s2, lora
        saved = [x, n1w, n2w, m1w, m2w, esb, a1w, a1b, a2w, *ab]
        x1 = x
        if s1 != 0.0:
            qkv = K.linear(x, pr.w(a1w), a1b)
            _dropout_fwd(pr, lora, ab, 2, x, qkv)
            o, lse = K.window_attention(qkv, pr.table(a1b), pr.table(esb), Z, H, W, heads, shifted, want_lse=True)
            y = K.linear(o, pr.w(a2w), a2b)
            _dropout_fwd(pr, lora, ab, 3, o, y)
            # (a dropped MLP branch -- s2 == 0 -- makes x1 the block's result: written straight into `out`, no copy afterwards)
            x1 = K.ln_residual(y, x, n1w, n1b, branch_scale=s1, out=out if s2 == 0.0 else None)
            saved += [qkv, o, lse, y]
        # MLP branch of the bf16 training forward (mode 1, C = 192 / 384 with contiguous rows): ONE launch that keeps the hidden
        # activation on chip and writes only what the backward needs (pre, m); the backward's data-gradient GEMM re-creates
        # h = GELU(pre) for the W2 weight gradient.  Mode 0, what fp32, other widths and row-strided inputs take: three launches
        # (MLP-up + GELU writing pre AND h, MLP-down, LayerNorm + residual), +2.3-3.1 ms per bf16 step where mode 1 applies.
        # (Recomputing the MLP-up GEMM in the backward instead of saving `pre` -- the reference's answer to activation memory,
        # layers.py:115-119 -- measured +2.7 ms per step and was removed in round 4; so were the QKV-inside-attention training
        # forward, +0.3 ms, and weight gradients on a second stream, +0.5 ms.  DESIGN.md keeps the numbers.)
        # Active adapter dropout on linear.linear1 / linear.linear2: the one launch keeps h on chip, where it cannot be corrected, so
        # the forward takes the three launches with their corrections -- but where mode 1 would have applied it still saves
        # (x1, pre, m) only and the backward stays mode 1 (linear_gelu_bwd re-creates the h that the correction wrote: gelu of the
        # stored bf16 pre): peak memory does not grow by the hidden tensor.
        ctx.mlp_mode = mode = 1 if (sh is not None and x.shape[1] in (192, 384) and x1.is_contiguous()) else 0
        mlp_drop = lora is not None and (type(lora[0]) is tuple or type(lora[1]) is tuple)
        if s2 != 0.0 and mode and not mlp_drop:
            x2, pre, m = ob.mlp_ln_residual_train(x1, sh.get_mlp(m1w, m2w), m1b, m2b, n2w, n2b, branch_scale=s2, out=out)
            saved += [x1, pre, m]
        elif s2 != 0.0:
            pre = torch.empty((x.shape[0], m1w.shape[0]), dtype=x.dtype, device=x.device)
            if lora is not None and type(lora[0]) is tuple:      # the GEMM without its GELU epilogue; the correction makes pre and h
                h = torch.empty_like(pre)
                _dropout_fwd(pr, lora, ab, 0, x1, K.linear(x1, pr.w(m1w), m1b, out=pre), act=ops.ACT_GELU, h=h)
            else:
                h = K.linear(x1, pr.w(m1w), m1b, act=ops.ACT_GELU, aux=pre)
            m = K.linear(h, pr.w(m2w), m2b)
            _dropout_fwd(pr, lora, ab, 1, h, m)
            x2 = K.ln_residual(m, x1, n2w, n2b, out=out, branch_scale=s2)
            saved += [x1, pre, m] if mode else [x1, pre, h, m]
        elif out is not None:
            if x1 is not out:
                out.copy_(x1)                     # both branches dropped: the block is the identity
            x2 = out
        else:
            x2 = x1
        ctx.save_for_backward(*saved)
        return x2

    @staticmethod
    def backward(ctx, dout):
        # (every atomically accumulated gradient buffer of the whole backward pass comes out of ONE zero fill: ops._zeros)
        Z, H, W, heads, shifted = ctx.geom
        s1, s2, pr = ctx.s1, ctx.s2, ctx.pr
        K = pr.k
        sv = ctx.saved_tensors
        x, n1w, n2w, m1w, m2w, esb, a1w, a1b, a2w = sv[:9]
        ab = sv[9:9 + 2 * len(ctx.lora or ())]
        rest = sv[9 + len(ab):]
        ad_m1, ad_m2, ad_a1, ad_a2 = _adapters(ctx, ab, 4)
        need = dict(zip(EarthBlockFn._INPUTS, ctx.needs_input_grad))
        g = {}
        if s1 != 0.0:
            qkv, o, lse, y = rest[:4]
            rest = rest[4:]
        dx1 = dout
        # _wgrad's input positions: m1w 5, m1b 6, m2w 7, m2b 8, a1w 10, a1b 11, a2w 12, a2b 13
        if s2 != 0.0:
            if ctx.mlp_mode == 1:
                x1, pre, m = rest
            else:
                x1, pre, h, m = rest
            dm, g["n2w"], g["n2b"] = K.ln_residual_bwd(dout, m, n2w, s2)
            # the W2 weight gradient is launched before the GELU-backward GEMM in fp32, after it in bf16 (where mode 1 gets h from it)
            if pr is _F32:
                g["m2w"], g["m2b"], g["m2A"], g["m2B"] = _wgrad(ctx, dm, h, 7, 8, ad_m2)
            if ctx.mlp_mode == 1:          # h = GELU(pre) comes out of the data-gradient GEMM's epilogue (never stored by the forward)
                dpre, h = ob.linear_gelu_bwd(dm, pr.wt(m2w), pre,
                                             want_h=need["m2w"] or need["m2b"] or need.get("m2A", False) or need.get("m2B", False)
                                             or (ad_m2 is not None and type(ad_m2[0]) is tuple))
            else:
                dpre = K.linear(dm, pr.wt(m2w), None, act=ops.ACT_GELU_BWD, aux=pre)
            if pr is not _F32:
                g["m2w"], g["m2b"], g["m2A"], g["m2B"] = _wgrad(ctx, dm, h, 7, 8, ad_m2)
            _dropout_dx(ctx, ad_m2, dpre, pre=pre)          # (after _wgrad, which leaves the V it reads)
            del dm, h
            g["m1w"], g["m1b"], g["m1A"], g["m1B"] = _wgrad(ctx, dpre, x1, 5, 6, ad_m1)
            if dout.is_contiguous():      # residual gradient added in the GEMM epilogue (no extra pass over N x C)
                dx1 = K.linear(dpre, pr.wt(m1w), act=ops.ACT_ADD, aux=dout)
            else:
                dx1 = K.linear(dpre, pr.wt(m1w))
                dx1 += dout
            _dropout_dx(ctx, ad_m1, dx1)
            del dpre
        dx = dx1
        if s1 != 0.0:
            dy, g["n1w"], g["n1b"] = K.ln_residual_bwd(dx1, y, n1w, s1)
            g["a2w"], g["a2b"], g["a2A"], g["a2B"] = _wgrad(ctx, dy, o, 12, 13, ad_a2)
            do = _dropout_dx(ctx, ad_a2, K.linear(dy, pr.wt(a2w)))
            del dy
            # (the bias-table gradient goes straight into the DP flat buffer)
            dqkv, dqb_pad, desb = K.window_attention_bwd(qkv, pr.table(a1b), pr.table(esb), o, lse, do, Z, H, W, heads, shifted,
                                                         desb_out=ops.grad_slot(esb) if need["esb"] else None)
            del do
            g["esb"] = desb.unsqueeze(0)
            # linear1's bias gradient = column sums of dqkv + the pad-slot term already in dqb_pad: the kernel adds into that buffer
            g["a1w"], g["a1b"], g["a1A"], g["a1B"] = _wgrad(ctx, dqkv, x, 10, 11, ad_a1, db_into=dqb_pad)
            if dx1.is_contiguous():
                dx = K.linear(dqkv, pr.wt(a1w), act=ops.ACT_ADD, aux=dx1)
            else:
                dx = K.linear(dqkv, pr.wt(a1w))
                dx += dx1
            _dropout_dx(ctx, ad_a1, dx)
        elif not dx.is_contiguous():
            dx = dx.contiguous()
        g["x"] = dx
        if s1 == 0.0 or s2 == 0.0:        # a dropped branch: only what asks for a gradient is filled (frozen parameters get nothing)
            like = {"n1w": n1w, "n1b": n1w, "n2w": n2w, "n2b": n2w, "m1w": m1w, "m1b": m1w[:, 0], "m2w": m2w, "m2b": n2w, "esb": esb,
                    "a1w": a1w, "a1b": a1b, "a2w": a2w, "a2b": n1w, **dict(zip(EarthBlockFn._INPUTS[20:], ab))}
            ops.fill_dropped_grads(g, {k: t for k, t in like.items() if need.get(k)})
        return _keep_needed(ctx, [g.get(k) for k in EarthBlockFn._INPUTS])


class AttentionWindowsFn(torch.autograd.Function):
    """reference models/layers.py:360-421 (EarthAttention3D.forward taken on its own) on partitioned rows: xw (n_lon*types*144, C)
    in window-slot order, esb (1, types, heads, 144, 144), mask None | (n_lon, types, 144, 144) | (types, 144, 144)."""

    @staticmethod
    def forward(ctx, xw, w1, b1, w2, b2, esb, mask, geom, lora=None, *ab):
        # lora: scalings of (linear1, linear2) (layers.lora_args), w1 / w2 then the W_eff tensors, ab = (A1, B1, A2, B2)
        n_lon, types, heads = geom
        qkv = ops.linear(xw, w1, b1)
        _dropout_fwd(_F32, lora, ab, 0, xw, qkv)
        o = ops.attention_windows(qkv, esb[0], mask, n_lon, types, heads)
        ctx.save_for_backward(xw, qkv, o, w1, w2, esb, mask, *ab)
        ctx.geom, ctx.lora, ctx.pr = geom, lora, _F32
        y = ops.linear(o, w2, b2)
        _dropout_fwd(_F32, lora, ab, 1, o, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        xw, qkv, o, w1, w2, esb, mask, *ab = ctx.saved_tensors
        ad1, ad2 = _adapters(ctx, ab, 2)
        n_lon, types, heads = ctx.geom
        dy = dy.contiguous()
        dw2, db2, dA2, dB2 = _wgrad(ctx, dy, o, 3, 4, ad2)
        do = _dropout_dx(ctx, ad2, ops.linear(dy, _wt(w2)))
        dqkv, desb = ops.attention_windows_bwd(qkv, esb[0], mask, do, n_lon, types, heads)
        dw1, db1, dA1, dB1 = _wgrad(ctx, dqkv, xw, 1, 2, ad1)
        dx = _dropout_dx(ctx, ad1, ops.linear(dqkv, _wt(w1)))
        return _keep_needed(ctx, (dx, dw1, db1, dw2, db2, desb.unsqueeze(0), None, None, None, dA1, dB1, dA2, dB2))


class MlpFn(torch.autograd.Function):
    """reference models/layers.py:264-270 (Mlp.forward taken on its own: linear1 -> exact-erf GELU -> linear2) on (M, C) rows."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, lora=None, *ab):
        # lora: scalings of (linear1, linear2) (layers.lora_args), w1 / w2 then the W_eff tensors, ab = (A1, B1, A2, B2)
        pre = torch.empty((x.shape[0], w1.shape[0]), dtype=x.dtype, device=x.device)
        if lora is not None and type(lora[0]) is tuple:      # (as in EarthBlockFn: the correction makes pre and h)
            h = torch.empty_like(pre)
            _dropout_fwd(_F32, lora, ab, 0, x, ops.linear(x, w1, b1, out=pre), act=ops.ACT_GELU, h=h)
        else:
            h = ops.linear(x, w1, b1, act=ops.ACT_GELU, aux=pre)
        ctx.save_for_backward(x, pre, h, w1, w2, *ab)
        ctx.lora, ctx.pr = lora, _F32
        m = ops.linear(h, w2, b2)
        _dropout_fwd(_F32, lora, ab, 1, h, m)
        return m

    @staticmethod
    def backward(ctx, dm):
        x, pre, h, w1, w2, *ab = ctx.saved_tensors
        ad1, ad2 = _adapters(ctx, ab, 2)
        dm = dm.contiguous()
        dw2, db2, dA2, dB2 = _wgrad(ctx, dm, h, 3, 4, ad2)
        dpre = _dropout_dx(ctx, ad2, ops.linear(dm, _wt(w2), None, act=ops.ACT_GELU_BWD, aux=pre), pre=pre)
        dw1, db1, dA1, dB1 = _wgrad(ctx, dpre, x, 1, 2, ad1)
        return _keep_needed(ctx, (_dropout_dx(ctx, ad1, ops.linear(dpre, _wt(w1))), dw1, db1, dw2, db2, None, dA1, dB1, dA2, dB2))


def refuse_constant_grads(maps, const_h, statistics=()):
    """The constant operands of the patch embedding (maps, const_h, the normalisation statistics) get no gradient from this
    build; asking for one must not return None silently."""
    for name, t in (("maps", maps), ("const_h", const_h)) + tuple((f"statistics[{i}]", t) for i, t in enumerate(statistics)):
        if torch.is_tensor(t) and t.requires_grad:
            raise RuntimeError(f"PanguModel (MI355X build): {name}.requires_grad is set, but gradients with respect to the constant maps, "
                               "const_h and the normalisation statistics are not implemented (input / input_surface are)")


class PatchEmbedFn(torch.autograd.Function):
    """reference models/layers.py:40-93 for one sample.  The raw fields get their gradient when they ask for it
    (`input.requires_grad_()`, plain autograd in the reference): d_input = scatter-adjoint of the gather of (dx @ W) / std."""

    @staticmethod
    def forward(ctx, cw, cb, sw, sb, inp, inp_s, s_mean, s_std, u_mean, u_std, maps, const_h, levels_reversed=False, sh=None):
        ctx.pr = pr = _precision(sh)
        a_s, a_u = pr.k.patch_embed_gather(inp, inp_s, s_mean, s_std, u_mean, u_std, maps, const_h, levels_reversed)
        n_s = a_s.shape[0]
        x = torch.empty((n_s + a_u.shape[0], cw.shape[0]), dtype=pr.dtype, device=inp.device)
        # the bf16 gather writes the surface rows 128 wide (112 columns + padding): its GEMM takes a weight image padded alike
        pr.k.linear(a_s, sw if sh is None else sh.get(sw, pad_k=128), sb, out=x[:n_s])
        pr.k.linear(a_u, pr.w(cw), cb, out=x[n_s:])
        ctx.save_for_backward(a_s, a_u, cw, sw, s_std, u_std)
        ctx.geom = (inp.shape[-2], inp.shape[-1], bool(levels_reversed))
        return x

    @staticmethod
    def backward(ctx, dx):
        a_s, a_u, cw, sw, s_std, u_std = ctx.saved_tensors
        pr = ctx.pr
        n_s = a_s.shape[0]
        if pr is _F32:
            dx = dx.contiguous()
        need = ctx.needs_input_grad
        dsw, dsb = _wgrad(ctx, dx[:n_s], a_s, 2, 3)[:2]
        if dsw is not None:
            if pr is not _F32:
                dsw = dsw[:, :sw.shape[1]]                              # (192, 128): columns 112.. are padding
            dsw = dsw.reshape(sw.shape)
        dcw, dcb = _wgrad(ctx, dx[n_s:], a_u, 0, 1, shape=cw.shape)[:2]
        d_in = d_in_s = None
        if need[4] or need[5]:
            # the raw fields asked for their gradient: dA for the A-matrix columns with a field behind them, the first 64 of 112
            # (surface) / 160 of 192 (upper), as an fp32 result; then the fp32 scatter adjoint of the gather, divided by the std
            LAT, LON, rev = ctx.geom
            dx = dx.contiguous()
            da_s = pr.k.linear(dx[:n_s], pr.wt(sw)[:64].contiguous(), **pr.f32_out)
            da_u = pr.k.linear(dx[n_s:], pr.wt(cw)[:160].contiguous(), **pr.f32_out)
            d_in, d_in_s = ops.patch_embed_gather_bwd(da_s, da_u, s_std, u_std, LAT, LON, rev)
        return _keep_needed(ctx, (dcw, dcb, dsw, dsb, d_in, d_in_s))


class DownSampleFn(torch.autograd.Function):
    """reference models/layers.py:432-459 for one sample."""

    @staticmethod
    def forward(ctx, x, lw, nw, nb, geom, skip_grad=None, sh=None, lora=None, *ab):
        # skip_grad: a one-slot list shared with PatchRecoverHalvesFn -- x is the skip connection (reference pangu_model.py:62, :81),
        # whose OTHER gradient (through the channel concat) that function leaves in the slot instead of handing it to autograd:
        # the backward below sums the two inside the down-sampling kernel (no elementwise add over the 200-400 MB)
        Z, H, W = geom
        ctx.pr = pr = _precision(sh)
        g = pr.k.downsample_ln(x, nw, nb, Z, H, W)
        ctx.save_for_backward(x, g, lw, nw, *ab)
        ctx.geom, ctx.skip_grad = geom, skip_grad
        ctx.lora = lora          # (scaling,) of an adapted linear (layers.lora_args): lw is then W_eff, ab = (A, B)
        if skip_grad is not None:
            skip_grad[1] = True                  # armed: this node's backward will consume the slot
        y = pr.k.linear(g, pr.w(lw))
        _dropout_fwd(pr, lora, ab, 0, g, y)
        return y

    @staticmethod
    def backward(ctx, dout):
        x, g, lw, nw, *ab = ctx.saved_tensors
        Z, H, W = ctx.geom
        dout = dout.contiguous()
        ad = _adapters(ctx, ab, 1)[0]
        dlw, _, dA, dB = _wgrad(ctx, dout, g, 1, ad=ad)
        dg = _dropout_dx(ctx, ad, ctx.pr.k.linear(dout, ctx.pr.wt(lw)))
        add = None
        if ctx.skip_grad is not None:
            add, ctx.skip_grad[0] = ctx.skip_grad[0], None
        dx, dnw, dnb = ctx.pr.k.downsample_ln_bwd(dg, x, nw, Z, H, W, add=add)
        return _keep_needed(ctx, (dx, dlw, dnw, dnb, None, None, None, None, dA, dB))


class UpSampleFn(torch.autograd.Function):
    """reference models/layers.py:474-499 for one sample."""

    @staticmethod
    def forward(ctx, x, l1w, l2w, nw, nb, geom, sh=None, lora=None, *ab):
        # lora: scalings of (linear1, linear2) (layers.lora_args), l1w / l2w then the W_eff tensors, ab = (A1, B1, A2, B2)
        Z, H2, W2, H = geom
        ctx.pr = pr = _precision(sh)
        y = pr.k.linear(x, pr.w(l1w))
        _dropout_fwd(pr, lora, ab, 0, x, y)
        g = pr.k.upsample_ln(y, nw, nb, Z, H2, W2, H)
        ctx.save_for_backward(x, y, g, l1w, l2w, nw, *ab)
        ctx.geom, ctx.lora = geom, lora
        out = pr.k.linear(g, pr.w(l2w))
        _dropout_fwd(pr, lora, ab, 1, g, out)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, y, g, l1w, l2w, nw, *ab = ctx.saved_tensors
        ad1, ad2 = _adapters(ctx, ab, 2)
        Z, H2, W2, H = ctx.geom
        pr = ctx.pr
        dout = dout.contiguous()
        dl2w, _, dA2, dB2 = _wgrad(ctx, dout, g, 2, ad=ad2)
        dg = _dropout_dx(ctx, ad2, pr.k.linear(dout, pr.wt(l2w)))
        dy, dnw, dnb = pr.k.upsample_ln_bwd(dg, y, nw, Z, H2, W2, H)
        dl1w, _, dA1, dB1 = _wgrad(ctx, dy, x, 1, ad=ad1)
        dx = _dropout_dx(ctx, ad1, pr.k.linear(dy, pr.wt(l1w)))
        return _keep_needed(ctx, (dx, dl1w, dl2w, dnw, dnb, None, None, None, dA1, dB1, dA2, dB2))


class PatchRecoverFn(torch.autograd.Function):
    """reference models/layers.py:511-545 for one sample: x (N, C) -> (5,13,LAT,LON), (4,LAT,LON)."""

    @staticmethod
    def forward(ctx, x, cw, cb, sw, sb, geom):
        n_s, LAT, LON = geom
        y_s = ops.linear(x[:n_s], sw, sb)
        y_u = ops.linear(x[n_s:], cw, cb)
        ctx.save_for_backward(x, cw, sw)
        ctx.geom, ctx.pr = geom, _F32
        return ops.patch_recover_scatter(y_u, y_s, LAT, LON)

    @staticmethod
    def backward(ctx, d_out, d_out_s):
        x, cw, sw = ctx.saved_tensors
        n_s, LAT, LON = ctx.geom
        dy_u, dy_s = ops.patch_recover_gather_bwd(d_out.contiguous(), d_out_s.contiguous())
        dcw, dcb = _wgrad(ctx, dy_u, x[n_s:], 1, 2, shape=cw.shape)[:2]
        dsw, dsb = _wgrad(ctx, dy_s, x[:n_s], 3, 4, shape=sw.shape)[:2]
        dx = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
        ops.linear(dy_s, _wt(sw), out=dx[:n_s])
        ops.linear(dy_u, _wt(cw), out=dx[n_s:])
        return _keep_needed(ctx, (dx, dcw, dcb, dsw, dsb))


class PatchRecoverHalvesFn(torch.autograd.Function):
    """The same layer on the channel concat of reference pangu_model.py:81 given as its two (N, C) halves, which are the two
    halves of ONE (N, 2C) buffer (layer 0 / layer 3 wrote them in place): no concat copy in the forward, and each half gets
    its own DENSE gradient in the backward (two N = C products instead of row-strided views of one N = 2C product).  The last
    layer of the whole-model driver in training and inference: without a graph its forward is the inference recovery."""

    @staticmethod
    def forward(ctx, skip, x, cw, cb, sw, sb, geom, skip_grad=None, sh=None, split=None):
        # split: frozen fp32 inference only (the caller decides: a forward cannot read grad mode) -- the split images
        # (surface, upper air) of the two conv weights, either None where that launch stays on the fp32-MFMA kernel
        ctx.skip_grad = skip_grad
        ctx.pr = pr = _precision(sh)
        n_s, LAT, LON = geom
        N, C = skip.shape
        assert skip.stride() == (2 * C, 1) and x.stride() == (2 * C, 1) and x.data_ptr() == skip.data_ptr() + skip.element_size() * C
        cat = torch.as_strided(skip, (N, 2 * C), (2 * C, 1), skip.storage_offset())
        img_s, img_u = split if split is not None and sh is None else (None, None)
        y_s = ops.linear_split(cat[:n_s], img_s, sw.shape[0], sb) if img_s is not None else \
            pr.k.linear(cat[:n_s], pr.w(sw), sb, **pr.f32_out)
        y_u = ops.linear_split(cat[n_s:], img_u, cw.shape[0], cb) if img_u is not None else \
            pr.k.linear(cat[n_s:], pr.w(cw), cb, **pr.f32_out)
        ctx.save_for_backward(cat, cw, sw)
        ctx.geom = geom
        return ops.patch_recover_scatter(y_u, y_s, LAT, LON)

    @staticmethod
    def backward(ctx, d_out, d_out_s):
        cat, cw, sw = ctx.saved_tensors
        n_s, LAT, LON = ctx.geom
        C = cat.shape[1] // 2
        pr = ctx.pr
        dy_u, dy_s = pr.k.patch_recover_gather_bwd(d_out.contiguous(), d_out_s.contiguous())
        dcw, dcb = _wgrad(ctx, dy_u, cat[n_s:], 2, 3, shape=cw.shape)[:2]
        dsw, dsb = _wgrad(ctx, dy_s, cat[:n_s], 4, 5, shape=sw.shape)[:2]
        wt_s, wt_u = pr.wt(sw), pr.wt(cw)                                  # (2C, 64), (2C, 160): rows = input channels
        d_skip = torch.empty((cat.shape[0], C), dtype=cat.dtype, device=cat.device)
        d_x = torch.empty_like(d_skip)
        for dst, rows in ((d_skip, slice(0, C)), (d_x, slice(C, 2 * C))):
            pr.k.linear(dy_s, wt_s[rows], out=dst[:n_s])
            pr.k.linear(dy_u, wt_u[rows], out=dst[n_s:])
        sg = ctx.skip_grad
        if sg is not None and sg[1] and ctx.needs_input_grad[0]:
            sg[0], d_skip = d_skip, None          # the down-sampling backward adds it in its own pass (DownSampleFn)
            # (if autograd pruned that node -- `torch.autograd.grad(loss, inputs=[layer-3 parameters])` -- nothing consumes the
            # slot: it is emptied when this backward pass ends instead of pinning 200-400 MB until the next forward)
            torch.autograd.Variable._execution_engine.queue_callback(lambda sg=sg: sg.__setitem__(0, None))
        return _keep_needed(ctx, (d_skip, d_x, dcw, dcb, dsw, dsb))
