"""The projections outside the blocks in frozen fp32 inference -- down-sampling, the two of up-sampling, patch embedding, patch
recovery -- on the exact-split kernel (fused._resample_proj, PatchRecoverHalvesFn's `split`) under the modules'
split_projections flag.  Needs an MI355X: run with `-m gpu`.

Geometry LAT = 25, LON = 48: H4 = 7, W4 = 12 (672 stage-0 tokens: five 128-row tiles and a 32-row remainder), H2 = 4, W2 = 6 (the
up-sampling crops 8 -> 7 rows).  Each layer against the oracle's restatement of it evaluated in fp64 on the same fp32 inputs:
  flag off: the bits of the composition of ops.linear launches;
  flag on:  rel-L2 error <= 1.5 x the flag-off error on the same inputs (the margin covers a different summation order: the rule
            of tests/test_gpu_linear_split.py)."""
import pytest
import torch

import pangu_oracle as O

pytestmark = pytest.mark.gpu
LAT, LON = 25, 48
Z, H4, W4, H2, W2 = 8, 7, 12, 4, 6
N0, N1 = Z * H4 * W4, Z * H2 * W2


@pytest.fixture(scope="module")
def P():
    import pangu_pytorch_amd as P
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    P._lib.load()
    return P


@pytest.fixture(scope="module")
def net(P):
    torch.manual_seed(11)
    m = P.PanguModel(depths=[1, 1, 1, 1], device="cuda").cuda().eval()
    with torch.no_grad():
        for mod in (m.downsample, m.upsample):
            mod.norm.weight.normal_(1.0, 0.3)
            mod.norm.bias.normal_(0.0, 0.3)
    return m


def _p64(net):
    return {k: v.detach().double().cpu() for k, v in net.state_dict().items()
            if k.startswith(("downsample.", "upsample.", "_input_layer.", "_output_layer."))}


def _l2(got, ref):
    return ((got.double().cpu() - ref).norm() / ref.norm()).item()


def _on_off(net, run):
    """-> (flag-on result, flag-off result) of run(); the flag is left on."""
    with torch.no_grad():
        net.use_split_projections(False)
        off = run()
        net.use_split_projections(True)
        on = run()
    return on, off


def _rule(tag, on, off, ref):
    e_on, e_off = _l2(on, ref), _l2(off, ref)
    print(f"{tag}: split {e_on:.3e} fp32 {e_off:.3e} ratio {e_on / max(e_off, 1e-30):.3f}")
    assert e_off < 2e-6 and e_on <= 1.5 * e_off, (tag, e_on, e_off)
    assert not torch.equal(on, off), tag                       # (the two arms really are different kernels)


def test_sample_down(P, net):
    m = net.downsample
    x = torch.randn(N0, 192, device="cuda")
    on, off = _on_off(net, lambda: P.fused.sample_down(m, x, Z, H4, W4))
    assert m.linear in P.ops._split_images
    g = P.ops.downsample_ln(x, m.norm.weight, m.norm.bias, Z, H4, W4)
    assert off.shape == (N1, 384) and torch.equal(off, P.ops.linear(g, m.linear.weight))
    assert torch.equal(on, P.ops.linear_split(g, P.ops.split_weight_image(m.linear.weight), 384))
    _rule("down", on, off, O.down_sample(_p64(net), x.double().cpu()[None], Z, H4, W4)[0])


def test_sample_up(P, net):
    m = net.upsample
    x = torch.randn(N1, 384, device="cuda")
    on, off = _on_off(net, lambda: P.fused.sample_up(m, x, Z, H2, W2, H4))
    assert m.linear1 in P.ops._split_images and m.linear2 in P.ops._split_images
    y = P.ops.linear(x, m.linear1.weight)
    g = P.ops.upsample_ln(y, m.norm.weight, m.norm.bias, Z, H2, W2, H4)
    assert off.shape == (N0, 192) and torch.equal(off, P.ops.linear(g, m.linear2.weight))
    _rule("up", on, off, O.up_sample(_p64(net), x.double().cpu()[None], Z, H2, W2, H4)[0])


def _embed_inputs():
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g)
    inp, inp_s = r(1, 5, 13, LAT, LON), r(1, 4, LAT, LON)
    stats = (0.3 * r(4), 1.2 + 0.2 * torch.rand(4, generator=g), 0.3 * r(13, 1, 1, 5), 1.2 + 0.2 * torch.rand(13, 1, 1, 5, generator=g))
    return inp, inp_s, stats, r(1, 3, 4 * H4, LON), r(1, 1, 1, 13, LAT, LON)


def test_sample_embed(P, net):
    m = net._input_layer
    inp, inp_s, stats, maps, const_h = _embed_inputs()
    consts = (stats[0].cuda(), stats[1].cuda(), stats[2].reshape(13, 5).cuda(), stats[3].reshape(13, 5).cuda(), maps[0].cuda(),
              const_h.reshape(13, LAT, LON).cuda())
    gi, gs = inp[0].cuda(), inp_s[0].cuda()
    on, off = _on_off(net, lambda: P.fused.sample_embed(m, gi, gs, consts))
    assert m.conv in P.ops._split_images
    a_s, a_u = P.ops.patch_embed_gather(gi, gs, *consts, False)
    want = torch.cat([P.ops.linear(a_s, m.conv_surface.weight, m.conv_surface.bias), P.ops.linear(a_u, m.conv.weight, m.conv.bias)], 0)
    assert off.shape == (N0, 192) and torch.equal(off, want)
    d = lambda t: t.double()
    ref = O.patch_embed(_p64(net), d(inp), d(inp_s), tuple(d(s) for s in stats), d(maps), d(const_h))[0]
    _rule("embed", on, off, ref)


def test_patch_recovery(P, net):
    """The forward of PatchRecoverHalvesFn on the two halves of one (N, 2C) buffer (lda = 2C), the decision passed in."""
    from pangu_pytorch_amd.autograd import PatchRecoverHalvesFn
    rec = net._output_layer
    halves = P.fused.concat_halves(torch.empty(N0, 192, device="cuda"))
    for h in halves:
        h.copy_(torch.randn(N0, 192, device="cuda"))
    cat = torch.cat(halves, 1)
    n_s = H4 * W4

    def run():
        split = (P.fused._split_image_of(rec, rec.conv_surface), P.fused._split_image_of(rec, rec.conv))
        return PatchRecoverHalvesFn.apply(halves[0], halves[1], rec.conv.weight, rec.conv.bias, rec.conv_surface.weight,
                                          rec.conv_surface.bias, (n_s, LAT, LON), None, None, split)

    with torch.no_grad():
        net.use_split_projections(False)
        assert P.fused._split_image_of(rec, rec.conv) is None
        off, off_s = run()
        mod, mod_s = P.fused.patch_recover(rec, cat[None], Z, H4, W4, LAT, LON)      # the module's (batched) inference arm
        assert torch.equal(mod[0], off) and torch.equal(mod_s[0], off_s)
        net.use_split_projections(True)
        on, on_s = run()
        mod, mod_s = P.fused.patch_recover(rec, cat[None], Z, H4, W4, LAT, LON)
        assert torch.equal(mod[0], on) and torch.equal(mod_s[0], on_s)               # B > 1 forwards == B = 1 forwards, bit for bit
        assert rec.conv in P.ops._split_images
        y_s = P.ops.linear(cat[:n_s], rec.conv_surface.weight, rec.conv_surface.bias)
        y_u = P.ops.linear(cat[n_s:], rec.conv.weight, rec.conv.bias)
        want, want_s = P.ops.patch_recover_scatter(y_u, y_s, LAT, LON)
    assert off.shape == (5, 13, LAT, LON) and off_s.shape == (4, LAT, LON)
    assert torch.equal(off, want) and torch.equal(off_s, want_s)
    ref, ref_s = O.patch_recover(_p64(net), cat.double().cpu()[None], Z, H4, W4, levels=13, lat=LAT)
    _rule("recover", on, off, ref[0])
    e_on, e_off = _l2(on_s, ref_s[0]), _l2(off_s, ref_s[0])
    print(f"recover surface: split-flag {e_on:.3e} fp32 {e_off:.3e}")
    assert e_off < 2e-6 and e_on <= 1.5 * e_off
    # a surface launch listed as not dispatched is the fp32 kernel under either flag
    if tuple(rec.conv_surface.weight.shape[:2]) in P.fused._SPLIT_NOT_DISPATCHED:
        assert torch.equal(on_s, off_s) and rec.conv_surface not in P.ops._split_images


def test_lora_edit_and_drop(P, net):
    """A LoRA down-sampling projection with B = 0 gives the base layer's bits; a weight edited in place gets a new image;
    use_split_projections(False) drops the images and every launch is the fp32-MFMA one again."""
    import copy
    m = net.downsample
    x = torch.randn(N0, 192, device="cuda")
    with torch.no_grad():
        net.use_split_projections(True)
        base = P.fused.sample_down(m, x, Z, H4, W4)
        ml = copy.deepcopy(m)
        ml.linear = P.layers.LoraLinear.from_linear(ml.linear, 4, 4)
        ml.eval()
        assert ml.split_projections and torch.equal(P.fused.sample_down(ml, x, Z, H4, W4), base)
        ml.linear.lora_B.normal_()
        w_eff = P.layers.eff_weight(ml.linear)
        g = P.ops.downsample_ln(x, m.norm.weight, m.norm.bias, Z, H4, W4)
        assert w_eff is not ml.linear.weight
        assert torch.equal(P.fused.sample_down(ml, x, Z, H4, W4), P.ops.linear_split(g, P.ops.split_weight_image(w_eff), 384))
        # in-place edit
        image = P.ops.split_image(m.linear, m.linear.weight)
        assert image is P.ops._split_images[m.linear][1]
        keep = m.linear.weight.clone()
        m.linear.weight.copy_(torch.randn_like(keep) / 768 ** 0.5)
        edited = P.fused.sample_down(m, x, Z, H4, W4)
        image2 = P.ops._split_images[m.linear][1]
        assert image2 is not image and torch.equal(image2, P.ops.split_weight_image(m.linear.weight))
        assert torch.equal(edited, P.ops.linear_split(g, image2, 384)) and not torch.equal(edited, base)
        m.linear.weight.copy_(keep)
        # the switch
        P.fused.sample_up(net.upsample, torch.randn(N1, 384, device="cuda"), Z, H2, W2, H4)
        mods = (m, net.upsample, net._input_layer, net._output_layer)
        assert all(mod.split_projections for mod in mods)
        assert m.linear in P.ops._split_images and net.upsample.linear1 in P.ops._split_images
        net.use_split_projections(False)
        assert not any(mod.split_projections for mod in mods)
        for lin in (m.linear, net.upsample.linear1, net.upsample.linear2, net._input_layer.conv, net._output_layer.conv):
            assert lin not in P.ops._split_images
        assert torch.equal(P.fused.sample_down(m, x, Z, H4, W4), P.ops.linear(g, m.linear.weight))
        assert m.linear not in P.ops._split_images
        net.use_split_projections(True)
