"""Compositions of the HIP kernels for each reference layer, and the whole-model forward of both precisions, training and inference.

The functions behind the modules of layers.py take token tensors (B, N, C); B is folded into rows for projections / LayerNorm and
looped for the geometry-dependent kernels (the reference itself is B=1 only, models/layers.py:219,227).  Their autograd arm and the
whole-model driver `forward_model` share the `sample_*` functions on 2-D (N, C) rows: the one call site of each layer Function and
of each layer's per-sample inference composition.
"""
import torch

from . import ops, ops_bf16 as ob
from .autograd import DownSampleFn, EarthBlockFn, MlpFn, PatchEmbedFn, PatchRecoverFn, PatchRecoverHalvesFn, UpSampleFn
from . import layers as _layers      # (layers imports this module: attribute access at call time)


def _train_path(module, *tensors):
    """Autograd path iff grad mode is on and something upstream (a parameter or an activation) needs a gradient."""
    if not torch.is_grad_enabled():
        return False
    return any(p.requires_grad for p in module.parameters()) or any(t.requires_grad for t in tensors)


def _stack(outs, B):
    return outs[0].unsqueeze(0) if B == 1 else torch.stack(outs, 0)


def _samples(x):
    """Per-sample contiguous tensors of a batched activation for the autograd path.  `x[b]` would put a SelectBackward
    into the graph (a zero fill + a copy of the whole activation per layer in backward: 2.8 ms of the fp32 step); the
    B = 1 case is a pure view, B > 1 goes through one unbind."""
    if x.shape[0] == 1:
        t = x.reshape(x.shape[1:])
        return [t if t.stride(-1) == 1 and t.dim() == 2 else t.contiguous()]      # row-strided rows are fine for every kernel
    return [t.contiguous() for t in x.unbind(0)]


def _tok2d(x):
    """(B,N,C) -> 2-D row view (B*N, C) (row-strided views stay views)."""
    B, N, C = x.shape
    if x.stride(2) != 1 or (B > 1 and x.stride(0) != N * x.stride(1)):
        x = x.contiguous()
    return x.as_strided((B * N, C), (x.stride(1), 1), x.storage_offset())


def drop_path_scales(blk):
    """The block's two DropPath keep factors (reference layers.py:250-251), drawn attention branch first."""
    dp = blk.drop_path
    if not hasattr(dp, "sample_scale"):
        return 1.0, 1.0
    return dp.sample_scale(blk.training), dp.sample_scale(blk.training)


def embed_constants(statistics, maps, const_h, LAT, LON, dev):
    """The normalisation statistics and constant maps as the patch-embedding gather reads them: contiguous fp32 on `dev`
    -> s_mean (4,), s_std (4,), u_mean (13, 5), u_std (13, 5), maps (3, 4*H4, LON), const_h (13, LAT, LON)."""
    f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    s_mean, s_std, u_mean, u_std = statistics
    return (f32(s_mean).reshape(-1), f32(s_std).reshape(-1), f32(u_mean).reshape(13, 5), f32(u_std).reshape(13, 5),
            f32(maps).reshape(3, 4 * ((LAT + 3) // 4), LON), f32(const_h).reshape(13, LAT, LON))


def concat_halves(x):
    """The skip-concat buffer of reference pangu_model.py:81 of the whole-model driver, as its two (N, C) halves: layer 0 / layer 3
    write their results straight into them, so the concat costs no copy.  The halves SHARE the storage of one (N, 2C) buffer
    without being autograd views of it (a view returned by a custom Function whose base is written again -- the other half -- is
    refused by autograd).  x: (N, C) or (1, N, C), giving shape, dtype and device."""
    N, C = x.shape[-2:]
    cat = torch.empty((N, 2 * C), dtype=x.dtype, device=x.device)
    return [torch.empty(0, dtype=x.dtype, device=x.device).set_(cat.untyped_storage(), cat.storage_offset() + off, (N, C), (2 * C, 1))
            for off in (0, C)]


def mlp(m, x2d):
    """Mlp.forward on its own (reference layers.py:264-270; the block never comes through here): differentiable."""
    if _train_path(m, x2d) or _drops(m):
        return MlpFn.apply(x2d.contiguous(), _layers.eff_weight(m.linear1), m.linear1.bias, _layers.eff_weight(m.linear2),
                           m.linear2.bias, *_layers.lora_args(m.linear1, m.linear2))
    h = ops.linear(x2d, _layers.eff_weight(m.linear1), m.linear1.bias, act=ops.ACT_GELU)
    return ops.linear(h, _layers.eff_weight(m.linear2), m.linear2.bias)


# (N, K) of the projections that stay on the fp32-MFMA kernel although the exact-split kernel serves them.  Keyed by shape alone: a
# shape is held back in every role (block projection, projection + LayerNorm, resampling / embedding / recovery) or in none.  What
# decides is speed and the 7-step rollout's step-7 fingerprint error against the reference, which tests/test_gpu_rollout.py bounds
# by 1e-3 and which moves between 7.5e-4 and 1.5e-3 with rounding detail alone (each split arm is more accurate per launch than
# the fp32 kernel: profiles/f32_split_ln_per_shape.md).  No block shape is listed: (384, 384) was while the attention core was
# fp32 MFMA; with everything dispatched step 7 reads 7.46e-4 and the step is the fastest (profiles/attn_f32_split_rollout.md).
# The two surface launches (M = 65160, under 0.1 ms of the step together) are: patch recovery (64, 384) measured 0.94 - 0.99 x
# per launch (N = 64 in a 192-column tile triples its matrix work); patch embedding (192, 112) measured 38 -> 25 us, but the
# headline and the rollout error were taken without it, so it waits until both are re-taken (profiles/f32_split_resampling.md).
_SPLIT_NOT_DISPATCHED = {(192, 112), (64, 384)}


def _split_image_of(owner, lin):
    """The cached split image of the weight the projection `lin` of `owner` (a block, or the resampling / embedding / recovery
    module) computes with in frozen fp32 inference, or None where the launch stays on the fp32-MFMA kernel: owner's
    split_projections flag is off (PanguModel.use_split_projections), the shape is listed in _SPLIT_NOT_DISPATCHED, or the kernel
    does not serve it (N % 4, K % 16).  A LoRA layer's image is that of its W_eff, keyed by the stamps of W, A and B: a model with
    adapters, the same model merged and (with B = 0) the base model compute the same bits, as they do on the fp32-MFMA kernels."""
    w = _layers.eff_weight(lin)
    N = w.shape[0]
    if not getattr(owner, "split_projections", True) or (N, w.numel() // N) in _SPLIT_NOT_DISPATCHED:      # Conv1d(k=1): (out, in, 1)
        return None
    return ops.split_image(lin, w, None if w is lin.weight else ("lora",) + tuple(lin._stamp()))


def _plain_proj(blk, lin, x2, act=ops.ACT_NONE):
    """A block's plain projection (qkv, MLP-up) in frozen fp32 inference: the exact-split bf16-MFMA kernel from the weight's image
    (_split_image_of), the fp32-MFMA kernel otherwise."""
    image = _split_image_of(blk, lin)
    if image is not None:
        return ops.linear_split(x2, image, lin.weight.shape[0], lin.bias, act=act)
    return ops.linear(x2, _layers.eff_weight(lin), lin.bias, act=act)


def _ln_proj(blk, lin, x2, shortcut, norm, out=None, branch_scale=1.0):
    """A block's fused projection (attention out-projection, MLP-down) + LayerNorm + residual in frozen fp32 inference, C = 192 /
    384: like _plain_proj the exact-split kernel from the weight's image, the fp32-MFMA kernel otherwise."""
    image = _split_image_of(blk, lin)
    if image is not None:
        return ops.linear_ln_residual_split(x2, image, lin.weight.shape[0], lin.bias, shortcut, norm.weight, norm.bias, out=out,
                                            branch_scale=branch_scale)
    return ops.linear_ln_residual(x2, _layers.eff_weight(lin), lin.bias, shortcut, norm.weight, norm.bias, out=out,
                                  branch_scale=branch_scale)


# C of the blocks whose attention core stays on the fp32-MFMA kernel (csrc/attn_f32.hip) although the exact-split kernel
# (csrc/attn_f32_split.hip) serves them: same form and same reason as _SPLIT_NOT_DISPATCHED; empty for the same measurement
# (profiles/attn_f32_split_rollout.md: with attention split at C = 384 only, step 7 reads 1.11e-3).
_ATTN_SPLIT_NOT_DISPATCHED = set()


def _block_rows(blk, x2, B, Z, H, W, roll, out=None):
    """The inference composition of a block on the 2-D rows x2 (B*N, C) of B samples -> (B*N, C), written into the 2-D `out` if
    given: 5 kernel launches per sample (qkv, attention core, proj+LN+residual, MLP-up+GELU, MLP-down+LN+residual).  With the
    block's split_projections flag set (PanguModel.use_split_projections) the attention core is the exact-split bf16-MFMA kernel
    for every C not in _ATTN_SPLIT_NOT_DISPATCHED, like the projections around it; otherwise the fp32-MFMA kernel."""
    N, C = x2.shape[0] // B, x2.shape[1]
    att = blk.attention
    s1, s2 = drop_path_scales(blk)
    if s1 != 0.0:
        qkv = _plain_proj(blk, att.linear1, x2)      # (B*N, 3C)
        # inference on the paper's compact bias table (PanguModel.use_compact_bias): 10 MB instead of 62 MB per block
        esb_c = getattr(att, "_esb_compact", None)
        if esb_c is not None:                 # stale table (weights changed since it was folded): the expanded parameter
            p = att.earth_specific_bias
            if getattr(att, "_esb_compact_stamp", None) != ops.param_stamp(p) or esb_c.device != p.device:
                att._esb_compact = esb_c = None
        cp = esb_c is not None
        esb = esb_c if cp else att.earth_specific_bias[0]
        sp = bool(getattr(blk, "split_projections", True)) and C not in _ATTN_SPLIT_NOT_DISPATCHED
        o = torch.cat([ops.window_attention(qkv[b * N:(b + 1) * N], att.linear1.bias, esb, Z, H, W,
                                            att.head_number, roll, compact=cp, split=sp) for b in range(B)], 0) if B > 1 else \
            ops.window_attention(qkv, att.linear1.bias, esb, Z, H, W, att.head_number, roll, compact=cp, split=sp)
        if C in (192, 384):     # projection + post-norm residual in one launch (the GEMM tile spans the row)
            x1 = _ln_proj(blk, att.linear2, o, x2, blk.norm1, branch_scale=s1)
        else:
            y = ops.linear(o, _layers.eff_weight(att.linear2), att.linear2.bias)
            x1 = ops.ln_residual(y, x2, blk.norm1.weight, blk.norm1.bias, branch_scale=s1)
    else:
        x1 = x2
    if s2 == 0.0:
        return x1 if out is None else out.copy_(x1)
    if C in (192, 384):
        h = _plain_proj(blk, blk.linear.linear1, x1, act=ops.ACT_GELU)
        return _ln_proj(blk, blk.linear.linear2, h, x1, blk.norm2, out=out, branch_scale=s2)
    return ops.ln_residual(mlp(blk.linear, x1), x1, blk.norm2.weight, blk.norm2.bias, out=out, branch_scale=s2)


def _block_rows_bf16(blk, sh, x, Z, H, W, roll, out=None):
    """The bf16 inference composition of a block: x (N,C) bf16 -> (N,C) bf16.  DropPath (reference layers.py:250-251) is the
    identity in eval(); in train() mode under no_grad each branch draws its per-sample keep factor like the fp32 path (a dropped
    branch is not computed)."""
    att = blk.attention
    s1, s2 = drop_path_scales(blk)
    C = x.shape[1]
    # attention projection + post-norm residual in one launch (the branch never round-trips HBM; -1.2 % on the forward at C = 384)
    fuse_proj = x.is_contiguous() and s1 == 1.0 and s2 == 1.0 and C in (192, 384)
    if s1 != 0.0:
        if C in (192, 384):
            # QKV projection inside the attention kernel: the (N, 3C) qkv tensor never reaches HBM
            o = ob.window_attention_qkv(x, sh.get_lin(att.linear1), att.linear1.bias, sh.get(att.earth_specific_bias),
                                        Z, H, W, att.head_number, roll)
        else:
            qkv = ob.linear(x, sh.get_lin(att.linear1), att.linear1.bias)
            o = ob.window_attention(qkv, sh.get(att.linear1.bias), sh.get(att.earth_specific_bias), Z, H, W,
                                    att.head_number, roll)
        if fuse_proj:
            x1 = ob.linear_ln_residual(o, sh.get_lin(att.linear2), att.linear2.bias, x, blk.norm1.weight, blk.norm1.bias)
        else:
            y = ob.linear(o, sh.get_lin(att.linear2), att.linear2.bias)
            x1 = ob.ln_residual(y, x, blk.norm1.weight, blk.norm1.bias, branch_scale=s1)
    else:
        x1 = x
    if s2 == 0.0:
        return x1 if out is None else out.copy_(x1)
    if C in (192, 384):
        # whole MLP branch + LayerNorm + residual in one launch: the (N, 4C) hidden activation never reaches HBM
        return ob.mlp_ln_residual(x1, sh.get_mlp_lin(blk.linear.linear1, blk.linear.linear2),
                                  blk.linear.linear1.bias, blk.linear.linear2.bias, blk.norm2.weight, blk.norm2.bias,
                                  out=out, branch_scale=s2)
    h = ob.linear(x1, sh.get_lin(blk.linear.linear1), blk.linear.linear1.bias, act=ob.ACT_GELU)
    m = ob.linear(h, sh.get_lin(blk.linear.linear2), blk.linear.linear2.bias)
    return ob.ln_residual(m, x1, blk.norm2.weight, blk.norm2.bias, out=out, branch_scale=s2)


# ---- one sample, one layer, on 2-D rows (N, C): THE call site of each layer Function and of its inference composition.
# sh: None for fp32, the model's fused_bf16.WeightShadow for bf16.  infer: nothing in the whole model asks for a gradient (`not
# grad_path` of PanguModel.forward); the default is a layer called on its own.
def _drops(layer):
    """A layer in train() mode with an active LoRA adapter dropout: it takes its Function also without a graph (the inference
    compositions have no place for the dropout corrections, and a train-mode output must not depend on grad mode)."""
    return layer.training and _layers.dropout_active(layer)


def _infer_arm(layer, sh, infer, *tensors):
    """Which arm a layer takes.  fp32: the inference composition iff the layer is frozen and no gradient arrives (_train_path
    false) and no adapter dropout is active (_drops), whatever `infer` says.  bf16: `infer` and nothing else -- on the model's
    autograd path a frozen bf16 layer runs its Function too, and a fully frozen bf16 model run with grad mode on takes the inference
    kernels (grad mode alone cannot tell)."""
    if sh is not None:
        if infer and _drops(layer):
            raise RuntimeError("LoRA adapter dropout in a bf16 train()-mode forward runs on the gradient path only (the inference "
                               "kernels have no materialised projections to correct): call eval() first")
        return infer
    return not (_train_path(layer, *tensors) or _drops(layer))


def sample_block(blk, x, Z, H, W, roll, out=None, sh=None, infer=False):
    """reference layers.py:183-253 for one sample, x (N, C) -> (N, C).  out: the 2-D (N, C) row-strided tensor the block writes its
    result into (a half of the skip-concat buffer, concat_halves) -- no copy."""
    if _infer_arm(blk, sh, infer, x):
        return _block_rows(blk, x, 1, Z, H, W, roll, out) if sh is None else _block_rows_bf16(blk, sh, x, Z, H, W, roll, out)
    att = blk.attention
    s1, s2 = drop_path_scales(blk)
    return EarthBlockFn.apply(
        x, blk.norm1.weight, blk.norm1.bias, blk.norm2.weight, blk.norm2.bias,
        _layers.eff_weight(blk.linear.linear1), blk.linear.linear1.bias,
        _layers.eff_weight(blk.linear.linear2), blk.linear.linear2.bias, att.earth_specific_bias,
        _layers.eff_weight(att.linear1), att.linear1.bias, _layers.eff_weight(att.linear2), att.linear2.bias,
        (Z, H, W, att.head_number, bool(roll)), s1, s2, None if out is None else (out,), sh,
        *_layers.lora_args(blk.linear.linear1, blk.linear.linear2, att.linear1, att.linear2))


def _resample_proj(m, lin, x2, out=None):
    """A projection outside the blocks (down/up-sampling, patch embedding, patch recovery) in frozen fp32 inference: like
    _plain_proj the exact-split kernel from the weight's image, the fp32-MFMA kernel otherwise.  x2 / out may be row-strided."""
    image = _split_image_of(m, lin)
    if image is not None:
        return ops.linear_split(x2, image, lin.weight.shape[0], lin.bias, out=out)
    return ops.linear(x2, _layers.eff_weight(lin), lin.bias, out=out)


def _embed_rows(m, inp, inp_surface, consts, levels_reversed, out):
    a_s, a_u = ops.patch_embed_gather(inp, inp_surface, *consts, levels_reversed)
    n_s = a_s.shape[0]
    _resample_proj(m, m.conv_surface, a_s, out=out[:n_s])
    _resample_proj(m, m.conv, a_u, out=out[n_s:])
    return out


def sample_embed(m, inp, inp_surface, consts, levels_reversed=False, sh=None):
    """reference layers.py:40-93 for one sample: contiguous inp (5, 13, LAT, LON), inp_surface (4, LAT, LON); consts: embed_constants.
    (bf16 has no inference arm: the conv weights are never adapted, and without a graph PatchEmbedFn's forward IS the inference
    composition, launch for launch.)"""
    if sh is None and not _train_path(m, inp, inp_surface):
        LAT, LON = inp.shape[-2], inp.shape[-1]
        x = torch.empty((8 * ((LAT + 3) // 4) * (LON // 4), m.conv.weight.shape[0]), dtype=torch.float32, device=inp.device)
        return _embed_rows(m, inp, inp_surface, consts, levels_reversed, x)
    return PatchEmbedFn.apply(m.conv.weight, m.conv.bias, m.conv_surface.weight, m.conv_surface.bias, inp, inp_surface, *consts,
                              levels_reversed, sh)


def sample_down(m, x, Z, H, W, skip_grad=None, sh=None, infer=False):
    """reference layers.py:432-459 for one sample.  skip_grad: the slot shared with PatchRecoverHalvesFn (see DownSampleFn)."""
    if _infer_arm(m, sh, infer, x):
        if sh is not None:        # (get_lin: the bf16 image of W_eff where the projection carries adapters)
            return ob.linear(ob.downsample_ln(x, m.norm.weight, m.norm.bias, Z, H, W), sh.get_lin(m.linear))
        return _resample_proj(m, m.linear, ops.downsample_ln(x, m.norm.weight, m.norm.bias, Z, H, W))
    return DownSampleFn.apply(x, _layers.eff_weight(m.linear), m.norm.weight, m.norm.bias, (Z, H, W), skip_grad, sh,
                              *_layers.lora_args(m.linear))


def _up_rows(m, x2, B, Z, H2, W2, H):
    y = _resample_proj(m, m.linear1, x2)                       # (B*N, 4Co)
    N, Co, Nf = x2.shape[0] // B, y.shape[1] // 4, Z * H * 2 * W2
    out = torch.empty((B * Nf, Co), dtype=torch.float32, device=x2.device)
    for b in range(B):
        g = ops.upsample_ln(y[b * N:(b + 1) * N], m.norm.weight, m.norm.bias, Z, H2, W2, H)
        _resample_proj(m, m.linear2, g, out=out[b * Nf:(b + 1) * Nf])
    return out


def sample_up(m, x, Z, H2, W2, H, sh=None, infer=False):
    """reference layers.py:474-499 for one sample."""
    if _infer_arm(m, sh, infer, x):
        if sh is not None:
            g = ob.upsample_ln(ob.linear(x, sh.get_lin(m.linear1)), m.norm.weight, m.norm.bias, Z, H2, W2, H)
            return ob.linear(g, sh.get_lin(m.linear2))
        return _up_rows(m, x, 1, Z, H2, W2, H)
    return UpSampleFn.apply(x, _layers.eff_weight(m.linear1), _layers.eff_weight(m.linear2), m.norm.weight, m.norm.bias,
                            (Z, H2, W2, H), sh, *_layers.lora_args(m.linear1, m.linear2))


def forward_model(model, inp, inp_surface, statistics, maps, const_h, levels_reversed=False, sh=None, grad_path=True):
    """The forward of the whole model (reference pangu_model.py:50-87), sample by sample on the per-sample layers above: bf16
    (sh = the model's WeightShadow, any B) and fp32 (sh None, B = 1: PanguModel._forward_dispatch).  grad_path: the model-level
    decision of PanguModel.forward; without it every layer takes its inference arm and no Function records a graph."""
    B, LAT, LON = inp.shape[0], inp.shape[-2], inp.shape[-1]
    H4, W4 = (LAT + 3) // 4, LON // 4
    H2, W2 = (H4 + 1) // 2, W4 // 2
    consts = embed_constants(statistics, maps, const_h, LAT, LON, inp.device)
    rec, infer = model._output_layer, not grad_path

    def run_layer(layer, x, H, W, out=None):
        last = len(layer.blocks) - 1
        for i, blk in enumerate(layer.blocks):
            x = sample_block(blk, x, 8, H, W, i % 2 == 1, out if i == last else None, sh, infer)
        return x

    res = []
    for b in range(B):
        x = sample_embed(model._input_layer, inp[b].contiguous(), inp_surface[b].contiguous(), consts, levels_reversed, sh)
        halves = concat_halves(x)                 # layer 0 / layer 3 write straight into them
        skip = run_layer(model.layers[0], x, H4, W4, halves[0])
        skip_grad = [None, False]                 # [the concat path's gradient of `skip`, armed]: see DownSampleFn
        x = sample_down(model.downsample, skip, 8, H4, W4, skip_grad, sh, infer)
        x = run_layer(model.layers[1], x, H2, W2)
        x = run_layer(model.layers[2], x, H2, W2)
        x = sample_up(model.upsample, x, 8, H2, W2, H4, sh, infer)
        x = run_layer(model.layers[3], x, H4, W4, halves[1])
        # frozen fp32 inference: the recovery's two products from their split images (the Function cannot read grad mode)
        split = (_split_image_of(rec, rec.conv_surface), _split_image_of(rec, rec.conv)) if infer and sh is None else None
        res.append(PatchRecoverHalvesFn.apply(skip, x, rec.conv.weight, rec.conv.bias, rec.conv_surface.weight,
                                              rec.conv_surface.bias, (H4 * W4, LAT, LON), skip_grad, sh, split))
    return tuple(_stack(t, B) for t in zip(*res))       # (B = 1: a view, no 286 MB stack copy)


# ---- the batched (B, N, C) functions behind the modules of layers.py, usable and differentiable on their own
def earth_block(blk, x, Z, H, W, roll, out=None):
    """x (B,N,C) -> (B,N,C), into the (B,N,C) `out` if given (a half of the inference concat buffer)."""
    B, N, C = x.shape
    if _train_path(blk, x) or _drops(blk):
        y = _stack([sample_block(blk, xb, Z, H, W, roll) for xb in _samples(x)], B)
        return y if out is None else out.copy_(y)
    y = _block_rows(blk, _tok2d(x), B, Z, H, W, roll, None if out is None else _tok2d(out))
    return y.view(B, N, C) if out is None else out


def patch_embed(m, inp, inp_surface, statistics, maps, const_h, levels_reversed=False):
    """reference layers.py:40-93 -> (B, 8*181*360, 192)."""
    B, LAT, LON = inp.shape[0], inp.shape[-2], inp.shape[-1]
    consts = embed_constants(statistics, maps, const_h, LAT, LON, inp.device)
    if _train_path(m, inp, inp_surface):
        return _stack([sample_embed(m, inp[b].contiguous(), inp_surface[b].contiguous(), consts, levels_reversed) for b in range(B)], B)
    x = torch.empty((B, 8 * ((LAT + 3) // 4) * (LON // 4), m.conv.weight.shape[0]), dtype=torch.float32, device=inp.device)
    for b in range(B):
        _embed_rows(m, inp[b].contiguous(), inp_surface[b].contiguous(), consts, levels_reversed, x[b])
    return x


def down_sample(m, x, Z, H, W):
    B = x.shape[0]
    rows = _samples(x) if _train_path(m, x) or _drops(m) else [_tok2d(x[b:b + 1]) for b in range(B)]
    return _stack([sample_down(m, xb, Z, H, W) for xb in rows], B)


def up_sample(m, x, Z, H2, W2, H):
    B = x.shape[0]
    if _train_path(m, x) or _drops(m):
        return _stack([sample_up(m, xb, Z, H2, W2, H) for xb in _samples(x)], B)
    return _up_rows(m, _tok2d(x), B, Z, H2, W2, H).view(B, Z * H * 2 * W2, -1)


def patch_recover(m, x, Z, H, W, LAT=721, LON=1440):
    """x (B, Z*H*W, C) (may be a row-strided view) -> (B,5,13,LAT,LON), (B,4,LAT,LON).  reference layers.py:511-545."""
    B, N, C = x.shape
    n_s = H * W
    if _train_path(m, x):
        res = [PatchRecoverFn.apply(xb, m.conv.weight, m.conv.bias, m.conv_surface.weight,
                                    m.conv_surface.bias, (n_s, LAT, LON)) for xb in _samples(x)]
        return _stack([r[0] for r in res], B), _stack([r[1] for r in res], B)
    outs, outs_s = [], []
    for b in range(B):
        xb = _tok2d(x[b:b + 1])
        y_s = _resample_proj(m, m.conv_surface, xb[:n_s])     # (the launches of forward_model's recovery: B = 2 == two B = 1, bit for bit)
        y_u = _resample_proj(m, m.conv, xb[n_s:])
        o, os_ = ops.patch_recover_scatter(y_u, y_s, LAT, LON)
        outs.append(o)
        outs_s.append(os_)
    return _stack(outs, B), _stack(outs_s, B)
